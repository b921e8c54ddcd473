"""The i-frame size probe and pfv_encoder's i-frame byte budget on a real MI355X: the shared checks of tests/probe_cases.py at the shapes of
the emulator twin (tests/test_emu_probe.py), exact against the ladder model's payloads and the numpy entropy oracle's counts."""
import pytest

import probe_cases as pc

pytestmark = pytest.mark.gpu

LANES = [1, 2]      # PFV_LANES_PER_MB_8, PFV_LANES_PER_MB_16: k_probe_iframe has both mappings


@pytest.mark.parametrize("int_transform", [False, True], ids=["f32", "i32"])
@pytest.mark.parametrize("lanes", LANES, ids=["lanes8", "lanes16"])
@pytest.mark.parametrize("w,h,n", pc.SHAPES)
def test_gpu_probe_session(pkg, gpu_ctx, oracle, w, h, n, lanes, int_transform):
    pc.check_session_probe(pkg, gpu_ctx, oracle, w, h, n, lane_mapping=lanes, int_transform=int_transform)


@pytest.mark.parametrize("w,h,n,lanes,int_transform", pc.INTERIOR_CASES, ids=pc.INTERIOR_IDS)
def test_gpu_probe_session_interior(pkg, gpu_ctx, oracle, w, h, n, lanes, int_transform):
    pc.check_session_probe(pkg, gpu_ctx, oracle, w, h, n, lane_mapping=lanes, int_transform=int_transform)


@pytest.mark.parametrize("lanes", LANES, ids=["lanes8", "lanes16"])
def test_gpu_probe_all_eleven_rungs(pkg, gpu_ctx, oracle, lanes):
    pc.check_session_probe(pkg, gpu_ctx, oracle, 50, 38, 3, lane_mapping=lanes, qualities=pc.FULL_LADDER, sets=[0, 2])


def test_gpu_probe_no_side_effects(pkg, gpu_ctx, oracle):
    pc.check_no_side_effects(pkg, gpu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_gpu_probe_is_what_the_encoder_writes(pkg, gpu_ctx, oracle, device_entropy):
    pc.check_probe_is_what_the_encoder_writes(pkg, gpu_ctx, oracle, device_entropy)


@pytest.mark.parametrize("lanes", LANES, ids=["lanes8", "lanes16"])
def test_gpu_probe_window_and_stride(pkg, gpu_ctx, oracle, lanes):
    pc.check_window_stride(pkg, gpu_ctx, oracle, lane_mapping=lanes)


def test_gpu_probe_graph(pkg, gpu_ctx, oracle):
    pc.check_graph(pkg, gpu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_gpu_probe_budget(pkg, gpu_ctx, oracle, device_entropy):
    pc.check_budget(pkg, gpu_ctx, oracle, device_entropy)
    pc.check_budget_equal_sizes(pkg, gpu_ctx, oracle, device_entropy)


def test_gpu_probe_arguments(pkg, gpu_ctx, oracle):
    pc.check_arguments(pkg, gpu_ctx, oracle)


def test_gpu_probe_cpp_mirror(graft, pkg, gpu_ctx, oracle, tmp_path):
    import os
    lib = graft.build_hip()
    if os.environ.get("PFV_TEST_EMU_AS_GPU") == "1":          # developer dry-run without a GPU (tests/conftest.py)
        import conftest
        lib = conftest.build_emulator()
    exe = str(tmp_path / "probe_budget")
    pc.build_cpp(lib, exe)
    pc.check_cpp(oracle, exe, tmp_path)
