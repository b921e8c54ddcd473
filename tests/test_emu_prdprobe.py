"""The p-frame rate-distortion probe, pfv_encoder's p-frame quality floor and the frame type it gives pfv_encoder_encode_frame on the CPU
emulator build of the kernel sources: the shared checks of tests/prdprobe_cases.py, exact against the ladder model's payloads, the numpy entropy
oracle's counts and the model's reconstructions.  The GPU twin is tests/test_gpu_prdprobe.py."""
import pytest

import prdprobe_cases as prd


def test_emu_prdprobe_inputs_cover(oracle):
    prd.check_inputs_cover(oracle)


@pytest.mark.parametrize("int_transform", [False, True], ids=["f32", "i32"])
@pytest.mark.parametrize("w,h,n", prd.SHAPES)
def test_emu_prdprobe_session(pkg, emu_ctx, oracle, w, h, n, int_transform):
    prd.check_session_probe(pkg, emu_ctx, oracle, w, h, n, int_transform=int_transform)


@pytest.mark.parametrize("w,h,n,int_transform", prd.pp.INTERIOR_CASES, ids=prd.pp.INTERIOR_IDS)
def test_emu_prdprobe_session_interior(pkg, emu_ctx, oracle, w, h, n, int_transform):
    prd.check_session_probe(pkg, emu_ctx, oracle, w, h, n, int_transform=int_transform)


def test_emu_prdprobe_all_eleven_rungs(pkg, emu_ctx, oracle):
    prd.check_session_probe(pkg, emu_ctx, oracle, 50, 38, 3, qualities=prd.FULL_LADDER, sets=[1, 2, 6])


def test_emu_prdprobe_agrees_with_size_probe(pkg, emu_ctx, oracle):
    prd.check_agrees_with_size_probe(pkg, emu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_emu_prdprobe_is_what_the_encoder_writes(pkg, emu_ctx, oracle, device_entropy):
    prd.check_probe_is_what_the_encoder_writes(pkg, emu_ctx, oracle, device_entropy)


def test_emu_prdprobe_no_side_effects(pkg, emu_ctx, oracle):
    prd.check_no_side_effects(pkg, emu_ctx, oracle)


def test_emu_prdprobe_window_and_stride(pkg, emu_ctx, oracle):
    prd.check_window_stride(pkg, emu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_emu_prdprobe_is_what_the_encoder_writes_interior(pkg, emu_ctx, oracle, device_entropy):
    prd.check_probe_is_what_the_encoder_writes(pkg, emu_ctx, oracle, device_entropy, 400, 80)


def test_emu_prdprobe_window_and_stride_interior(pkg, emu_ctx, oracle):
    prd.check_window_stride(pkg, emu_ctx, oracle, 400, 80, 3)


def test_emu_prdprobe_strip_on_the_right_border(pkg, emu_ctx, oracle):
    prd.pp.check_strip_on_the_right_border(pkg, emu_ctx, oracle, rig_class=prd.PRdRig)


def test_emu_prdprobe_graph(pkg, emu_ctx, oracle):
    prd.check_graph(pkg, emu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_emu_prdprobe_quality_floor(pkg, emu_ctx, oracle, device_entropy):
    prd.check_floor(pkg, emu_ctx, oracle, device_entropy)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_emu_prdprobe_rd_frame_type(pkg, emu_ctx, oracle, device_entropy):
    prd.check_rd_frame_type(pkg, emu_ctx, oracle, device_entropy)


def test_emu_prdprobe_arguments(pkg, emu_ctx, oracle):
    prd.check_arguments(pkg, emu_ctx, oracle)


def test_emu_prdprobe_poisoned_encoder(tmp_path):
    """emulator only: the failure that poisons an encoder comes from a seam in the emulator build (tests/cpp/poison_seam.h)"""
    exe = str(tmp_path / "prd_floor_seam")
    prd.build_poison(exe)
    prd.check_poisoned(exe, tmp_path)


def test_emu_prdprobe_cpp_mirror(pkg, emu_ctx, oracle, tmp_path):
    import conftest
    exe = str(tmp_path / "prd_floor_emu")
    prd.build_cpp(conftest.build_emulator(), exe)
    prd.check_cpp(oracle, exe, tmp_path)
