"""The i-frame rate-distortion probe and pfv_encoder's i-frame quality floor on the CPU emulator build of the kernel sources: the shared checks
of tests/rdprobe_cases.py, exact against the ladder model's payloads, the numpy entropy oracle's counts and the model's reconstructions.  The GPU
twin is tests/test_gpu_rdprobe.py."""
import pytest

import rdprobe_cases as rc

LANES = [1, 2]      # PFV_LANES_PER_MB_8, PFV_LANES_PER_MB_16: k_probe_iframe_rd has both mappings


@pytest.mark.parametrize("int_transform", [False, True], ids=["f32", "i32"])
@pytest.mark.parametrize("lanes", LANES, ids=["lanes8", "lanes16"])
@pytest.mark.parametrize("w,h,n", rc.lc.SHAPES)
def test_emu_rdprobe_session(pkg, emu_ctx, oracle, w, h, n, lanes, int_transform):
    rc.check_session_probe(pkg, emu_ctx, oracle, w, h, n, lane_mapping=lanes, int_transform=int_transform)


@pytest.mark.parametrize("w,h,n,lanes,int_transform", rc.pc.INTERIOR_CASES, ids=rc.pc.INTERIOR_IDS)
def test_emu_rdprobe_session_interior(pkg, emu_ctx, oracle, w, h, n, lanes, int_transform):
    rc.check_session_probe(pkg, emu_ctx, oracle, w, h, n, lane_mapping=lanes, int_transform=int_transform)


def test_emu_rdprobe_all_eleven_rungs(pkg, emu_ctx, oracle):
    rc.check_session_probe(pkg, emu_ctx, oracle, 50, 38, 3, qualities=rc.FULL_LADDER, sets=[0, 2])


def test_emu_rdprobe_agrees_with_size_probe(pkg, emu_ctx, oracle):
    rc.check_agrees_with_size_probe(pkg, emu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_emu_rdprobe_is_what_the_encoder_writes(pkg, emu_ctx, oracle, device_entropy):
    rc.check_probe_is_what_the_encoder_writes(pkg, emu_ctx, oracle, device_entropy)


def test_emu_rdprobe_no_side_effects(pkg, emu_ctx, oracle):
    rc.check_no_side_effects(pkg, emu_ctx, oracle)


@pytest.mark.parametrize("lanes", LANES, ids=["lanes8", "lanes16"])
def test_emu_rdprobe_window_and_stride(pkg, emu_ctx, oracle, lanes):
    rc.check_window_stride(pkg, emu_ctx, oracle, lane_mapping=lanes)


def test_emu_rdprobe_graph(pkg, emu_ctx, oracle):
    rc.check_graph(pkg, emu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_emu_rdprobe_quality_floor(pkg, emu_ctx, oracle, device_entropy):
    rc.check_floor(pkg, emu_ctx, oracle, device_entropy)
    rc.check_floor_ties_and_one_rung(pkg, emu_ctx, oracle, device_entropy)


def test_emu_rdprobe_arguments(pkg, emu_ctx, oracle):
    rc.check_arguments(pkg, emu_ctx, oracle)


def test_emu_rdprobe_cpp_mirror(pkg, emu_ctx, oracle, tmp_path):
    import conftest
    exe = str(tmp_path / "rd_floor_emu")
    rc.build_cpp(conftest.build_emulator(), exe)
    rc.check_cpp(oracle, exe, tmp_path)
