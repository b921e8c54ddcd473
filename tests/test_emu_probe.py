"""The i-frame size probe and pfv_encoder's i-frame byte budget on the CPU emulator build of the kernel sources: the shared checks of
tests/probe_cases.py, exact against the ladder model's payloads and the numpy entropy oracle's counts.  The GPU twin is tests/test_gpu_probe.py."""
import pytest

import probe_cases as pc

LANES = [1, 2]      # PFV_LANES_PER_MB_8, PFV_LANES_PER_MB_16: k_probe_iframe has both mappings


@pytest.mark.parametrize("int_transform", [False, True], ids=["f32", "i32"])
@pytest.mark.parametrize("lanes", LANES, ids=["lanes8", "lanes16"])
@pytest.mark.parametrize("w,h,n", pc.SHAPES)
def test_emu_probe_session(pkg, emu_ctx, oracle, w, h, n, lanes, int_transform):
    pc.check_session_probe(pkg, emu_ctx, oracle, w, h, n, lane_mapping=lanes, int_transform=int_transform)


@pytest.mark.parametrize("w,h,n,lanes,int_transform", pc.INTERIOR_CASES, ids=pc.INTERIOR_IDS)
def test_emu_probe_session_interior(pkg, emu_ctx, oracle, w, h, n, lanes, int_transform):
    pc.check_session_probe(pkg, emu_ctx, oracle, w, h, n, lane_mapping=lanes, int_transform=int_transform)


@pytest.mark.parametrize("lanes", LANES, ids=["lanes8", "lanes16"])
def test_emu_probe_all_eleven_rungs(pkg, emu_ctx, oracle, lanes):
    pc.check_session_probe(pkg, emu_ctx, oracle, 50, 38, 3, lane_mapping=lanes, qualities=pc.FULL_LADDER, sets=[0, 2])


def test_emu_probe_no_side_effects(pkg, emu_ctx, oracle):
    pc.check_no_side_effects(pkg, emu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_emu_probe_is_what_the_encoder_writes(pkg, emu_ctx, oracle, device_entropy):
    pc.check_probe_is_what_the_encoder_writes(pkg, emu_ctx, oracle, device_entropy)


@pytest.mark.parametrize("lanes", LANES, ids=["lanes8", "lanes16"])
def test_emu_probe_window_and_stride(pkg, emu_ctx, oracle, lanes):
    pc.check_window_stride(pkg, emu_ctx, oracle, lane_mapping=lanes)


def test_emu_probe_graph(pkg, emu_ctx, oracle):
    pc.check_graph(pkg, emu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_emu_probe_budget(pkg, emu_ctx, oracle, device_entropy):
    pc.check_budget(pkg, emu_ctx, oracle, device_entropy)
    pc.check_budget_equal_sizes(pkg, emu_ctx, oracle, device_entropy)


def test_emu_probe_arguments(pkg, emu_ctx, oracle):
    pc.check_arguments(pkg, emu_ctx, oracle)


def test_emu_probe_cpp_mirror(pkg, emu_ctx, oracle, tmp_path):
    import conftest
    exe = str(tmp_path / "probe_budget_emu")
    pc.build_cpp(conftest.build_emulator(), exe)
    pc.check_cpp(oracle, exe, tmp_path)
