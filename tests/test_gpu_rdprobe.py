"""The i-frame rate-distortion probe and pfv_encoder's i-frame quality floor on a real MI355X: the shared checks of tests/rdprobe_cases.py at
the shapes of the emulator twin (tests/test_emu_rdprobe.py), exact against the ladder model's payloads, the numpy entropy oracle's counts and
the model's reconstructions."""
import pytest

import rdprobe_cases as rc

pytestmark = pytest.mark.gpu

LANES = [1, 2]      # PFV_LANES_PER_MB_8, PFV_LANES_PER_MB_16: k_probe_iframe_rd has both mappings


@pytest.mark.parametrize("int_transform", [False, True], ids=["f32", "i32"])
@pytest.mark.parametrize("lanes", LANES, ids=["lanes8", "lanes16"])
@pytest.mark.parametrize("w,h,n", rc.lc.SHAPES)
def test_gpu_rdprobe_session(pkg, gpu_ctx, oracle, w, h, n, lanes, int_transform):
    rc.check_session_probe(pkg, gpu_ctx, oracle, w, h, n, lane_mapping=lanes, int_transform=int_transform)


@pytest.mark.parametrize("w,h,n,lanes,int_transform", rc.pc.INTERIOR_CASES, ids=rc.pc.INTERIOR_IDS)
def test_gpu_rdprobe_session_interior(pkg, gpu_ctx, oracle, w, h, n, lanes, int_transform):
    rc.check_session_probe(pkg, gpu_ctx, oracle, w, h, n, lane_mapping=lanes, int_transform=int_transform)


def test_gpu_rdprobe_all_eleven_rungs(pkg, gpu_ctx, oracle):
    rc.check_session_probe(pkg, gpu_ctx, oracle, 50, 38, 3, qualities=rc.FULL_LADDER, sets=[0, 2])


def test_gpu_rdprobe_agrees_with_size_probe(pkg, gpu_ctx, oracle):
    rc.check_agrees_with_size_probe(pkg, gpu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_gpu_rdprobe_is_what_the_encoder_writes(pkg, gpu_ctx, oracle, device_entropy):
    rc.check_probe_is_what_the_encoder_writes(pkg, gpu_ctx, oracle, device_entropy)


def test_gpu_rdprobe_no_side_effects(pkg, gpu_ctx, oracle):
    rc.check_no_side_effects(pkg, gpu_ctx, oracle)


@pytest.mark.parametrize("lanes", LANES, ids=["lanes8", "lanes16"])
def test_gpu_rdprobe_window_and_stride(pkg, gpu_ctx, oracle, lanes):
    rc.check_window_stride(pkg, gpu_ctx, oracle, lane_mapping=lanes)


def test_gpu_rdprobe_graph(pkg, gpu_ctx, oracle):
    rc.check_graph(pkg, gpu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_gpu_rdprobe_quality_floor(pkg, gpu_ctx, oracle, device_entropy):
    rc.check_floor(pkg, gpu_ctx, oracle, device_entropy)
    rc.check_floor_ties_and_one_rung(pkg, gpu_ctx, oracle, device_entropy)


def test_gpu_rdprobe_arguments(pkg, gpu_ctx, oracle):
    rc.check_arguments(pkg, gpu_ctx, oracle)


def test_gpu_rdprobe_cpp_mirror(graft, pkg, gpu_ctx, oracle, tmp_path):
    import os
    lib = graft.build_hip()
    if os.environ.get("PFV_TEST_EMU_AS_GPU") == "1":          # developer dry-run without a GPU (tests/conftest.py)
        import conftest
        lib = conftest.build_emulator()
    exe = str(tmp_path / "rd_floor")
    rc.build_cpp(lib, exe)
    rc.check_cpp(oracle, exe, tmp_path)
