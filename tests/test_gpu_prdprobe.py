"""The p-frame rate-distortion probe, pfv_encoder's p-frame quality floor and the frame type it gives pfv_encoder_encode_frame on a real
MI355X: the shared checks of tests/prdprobe_cases.py at the shapes of the emulator twin (tests/test_emu_prdprobe.py), exact against the ladder
model's payloads, the numpy entropy oracle's counts and the model's reconstructions."""
import pytest

import prdprobe_cases as prd

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("int_transform", [False, True], ids=["f32", "i32"])
@pytest.mark.parametrize("w,h,n", prd.SHAPES)
def test_gpu_prdprobe_session(pkg, gpu_ctx, oracle, w, h, n, int_transform):
    prd.check_session_probe(pkg, gpu_ctx, oracle, w, h, n, int_transform=int_transform)


@pytest.mark.parametrize("w,h,n,int_transform", prd.pp.INTERIOR_CASES, ids=prd.pp.INTERIOR_IDS)
def test_gpu_prdprobe_session_interior(pkg, gpu_ctx, oracle, w, h, n, int_transform):
    prd.check_session_probe(pkg, gpu_ctx, oracle, w, h, n, int_transform=int_transform)


def test_gpu_prdprobe_all_eleven_rungs(pkg, gpu_ctx, oracle):
    prd.check_session_probe(pkg, gpu_ctx, oracle, 50, 38, 3, qualities=prd.FULL_LADDER, sets=[1, 2, 6])


def test_gpu_prdprobe_agrees_with_size_probe(pkg, gpu_ctx, oracle):
    prd.check_agrees_with_size_probe(pkg, gpu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_gpu_prdprobe_is_what_the_encoder_writes(pkg, gpu_ctx, oracle, device_entropy):
    prd.check_probe_is_what_the_encoder_writes(pkg, gpu_ctx, oracle, device_entropy)


def test_gpu_prdprobe_no_side_effects(pkg, gpu_ctx, oracle):
    prd.check_no_side_effects(pkg, gpu_ctx, oracle)


def test_gpu_prdprobe_window_and_stride(pkg, gpu_ctx, oracle):
    prd.check_window_stride(pkg, gpu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_gpu_prdprobe_is_what_the_encoder_writes_interior(pkg, gpu_ctx, oracle, device_entropy):
    prd.check_probe_is_what_the_encoder_writes(pkg, gpu_ctx, oracle, device_entropy, 400, 80)


def test_gpu_prdprobe_window_and_stride_interior(pkg, gpu_ctx, oracle):
    prd.check_window_stride(pkg, gpu_ctx, oracle, 400, 80, 3)


def test_gpu_prdprobe_strip_on_the_right_border(pkg, gpu_ctx, oracle):
    prd.pp.check_strip_on_the_right_border(pkg, gpu_ctx, oracle, rig_class=prd.PRdRig)


def test_gpu_prdprobe_graph(pkg, gpu_ctx, oracle):
    prd.check_graph(pkg, gpu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_gpu_prdprobe_quality_floor(pkg, gpu_ctx, oracle, device_entropy):
    prd.check_floor(pkg, gpu_ctx, oracle, device_entropy)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_gpu_prdprobe_rd_frame_type(pkg, gpu_ctx, oracle, device_entropy):
    prd.check_rd_frame_type(pkg, gpu_ctx, oracle, device_entropy)


def test_gpu_prdprobe_arguments(pkg, gpu_ctx, oracle):
    prd.check_arguments(pkg, gpu_ctx, oracle)


def test_gpu_prdprobe_cpp_mirror(graft, pkg, gpu_ctx, oracle, tmp_path):
    import os
    lib = graft.build_hip()
    if os.environ.get("PFV_TEST_EMU_AS_GPU") == "1":          # developer dry-run without a GPU (tests/conftest.py)
        import conftest
        lib = conftest.build_emulator()
    exe = str(tmp_path / "prd_floor")
    prd.build_cpp(lib, exe)
    prd.check_cpp(oracle, exe, tmp_path)
