"""The p-frame size probe, pfv_encoder's hard p-frame budget and its automatic frame type on a real MI355X: the shared checks of
tests/pprobe_cases.py at the shapes of the emulator twin (tests/test_emu_pprobe.py), exact against the ladder model's payloads and the numpy
entropy oracle's counts."""
import pytest

import pprobe_cases as pp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("int_transform", [False, True], ids=["f32", "i32"])
@pytest.mark.parametrize("w,h,n", pp.SHAPES)
def test_gpu_pprobe_session(pkg, gpu_ctx, oracle, w, h, n, int_transform):
    pp.check_session_probe(pkg, gpu_ctx, oracle, w, h, n, int_transform=int_transform)


@pytest.mark.parametrize("w,h,n,int_transform", pp.INTERIOR_CASES, ids=pp.INTERIOR_IDS)
def test_gpu_pprobe_session_interior(pkg, gpu_ctx, oracle, w, h, n, int_transform):
    pp.check_session_probe(pkg, gpu_ctx, oracle, w, h, n, int_transform=int_transform)


@pytest.mark.parametrize("int_transform", [False, True], ids=["f32", "i32"])
def test_gpu_pprobe_all_eleven_rungs(pkg, gpu_ctx, oracle, int_transform):
    pp.check_session_probe(pkg, gpu_ctx, oracle, 50, 38, 3, int_transform=int_transform, qualities=pp.FULL_LADDER)


def test_gpu_pprobe_no_side_effects(pkg, gpu_ctx, oracle):
    pp.check_no_side_effects(pkg, gpu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_gpu_pprobe_is_what_the_encoder_writes(pkg, gpu_ctx, oracle, device_entropy):
    pp.check_probe_is_what_the_encoder_writes(pkg, gpu_ctx, oracle, device_entropy)


def test_gpu_pprobe_window_and_stride(pkg, gpu_ctx, oracle):
    pp.check_window_stride(pkg, gpu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_gpu_pprobe_is_what_the_encoder_writes_interior(pkg, gpu_ctx, oracle, device_entropy):
    pp.check_probe_is_what_the_encoder_writes(pkg, gpu_ctx, oracle, device_entropy, 400, 80)


def test_gpu_pprobe_window_and_stride_interior(pkg, gpu_ctx, oracle):
    pp.check_window_stride(pkg, gpu_ctx, oracle, 400, 80, 3)


def test_gpu_pprobe_strip_on_the_right_border(pkg, gpu_ctx, oracle):
    pp.check_strip_on_the_right_border(pkg, gpu_ctx, oracle)


def test_gpu_pprobe_graph(pkg, gpu_ctx, oracle):
    pp.check_graph(pkg, gpu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_gpu_pprobe_hard_budget(pkg, gpu_ctx, oracle, device_entropy):
    pp.check_hard_budget(pkg, gpu_ctx, oracle, device_entropy)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_gpu_pprobe_auto_frame_type(pkg, gpu_ctx, oracle, device_entropy):
    pp.check_auto(pkg, gpu_ctx, oracle, device_entropy)


def test_gpu_pprobe_arguments(pkg, gpu_ctx, oracle):
    pp.check_arguments(pkg, gpu_ctx, oracle)


def test_gpu_pprobe_cpp_mirror(graft, pkg, gpu_ctx, oracle, tmp_path):
    import os
    lib = graft.build_hip()
    if os.environ.get("PFV_TEST_EMU_AS_GPU") == "1":          # developer dry-run without a GPU (tests/conftest.py)
        import conftest
        lib = conftest.build_emulator()
    exe = str(tmp_path / "pprobe_auto")
    pp.build_cpp(lib, exe)
    pp.check_cpp(oracle, exe, tmp_path)
