"""The p-frame size probe, pfv_encoder's hard p-frame budget and its automatic frame type on the CPU emulator build of the kernel sources: the
shared checks of tests/pprobe_cases.py, exact against the ladder model's payloads and the numpy entropy oracle's counts.  The GPU twin is
tests/test_gpu_pprobe.py."""
import pytest

import pprobe_cases as pp


@pytest.mark.parametrize("int_transform", [False, True], ids=["f32", "i32"])
@pytest.mark.parametrize("w,h,n", pp.SHAPES)
def test_emu_pprobe_session(pkg, emu_ctx, oracle, w, h, n, int_transform):
    pp.check_session_probe(pkg, emu_ctx, oracle, w, h, n, int_transform=int_transform)


@pytest.mark.parametrize("w,h,n", pp.INTERIOR_SHAPES)
def test_emu_pprobe_interior_inputs(oracle, w, h, n):
    """the oracle alone: no device, emulated or real"""
    pp.check_inputs_cover(oracle, w, h, n)
    pp.check_interior_inputs(oracle, w, h, n)


@pytest.mark.parametrize("w,h,n,int_transform", pp.INTERIOR_CASES, ids=pp.INTERIOR_IDS)
def test_emu_pprobe_session_interior(pkg, emu_ctx, oracle, w, h, n, int_transform):
    pp.check_session_probe(pkg, emu_ctx, oracle, w, h, n, int_transform=int_transform)


@pytest.mark.parametrize("int_transform", [False, True], ids=["f32", "i32"])
def test_emu_pprobe_all_eleven_rungs(pkg, emu_ctx, oracle, int_transform):
    pp.check_session_probe(pkg, emu_ctx, oracle, 50, 38, 3, int_transform=int_transform, qualities=pp.FULL_LADDER)


def test_emu_pprobe_no_side_effects(pkg, emu_ctx, oracle):
    pp.check_no_side_effects(pkg, emu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_emu_pprobe_is_what_the_encoder_writes(pkg, emu_ctx, oracle, device_entropy):
    pp.check_probe_is_what_the_encoder_writes(pkg, emu_ctx, oracle, device_entropy)


def test_emu_pprobe_window_and_stride(pkg, emu_ctx, oracle):
    pp.check_window_stride(pkg, emu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_emu_pprobe_is_what_the_encoder_writes_interior(pkg, emu_ctx, oracle, device_entropy):
    pp.check_probe_is_what_the_encoder_writes(pkg, emu_ctx, oracle, device_entropy, 400, 80)


def test_emu_pprobe_window_and_stride_interior(pkg, emu_ctx, oracle):
    pp.check_window_stride(pkg, emu_ctx, oracle, 400, 80, 3)


def test_emu_pprobe_strip_on_the_right_border(pkg, emu_ctx, oracle):
    pp.check_strip_on_the_right_border(pkg, emu_ctx, oracle)


def test_emu_pprobe_graph(pkg, emu_ctx, oracle):
    pp.check_graph(pkg, emu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_emu_pprobe_hard_budget(pkg, emu_ctx, oracle, device_entropy):
    pp.check_hard_budget(pkg, emu_ctx, oracle, device_entropy)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_emu_pprobe_auto_frame_type(pkg, emu_ctx, oracle, device_entropy):
    pp.check_auto(pkg, emu_ctx, oracle, device_entropy)


def test_emu_pprobe_arguments(pkg, emu_ctx, oracle):
    pp.check_arguments(pkg, emu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_emu_pprobe_poisoned_encoder(oracle, tmp_path, device_entropy):
    """emulator only: the failure that poisons an encoder comes from a seam in the emulator build (tests/cpp/poison_seam.h)"""
    exe = str(tmp_path / "pprobe_poison")
    pp.build_poison(exe)
    pp.check_poisoned(oracle, exe, tmp_path, device_entropy)


def test_emu_pprobe_cpp_mirror(pkg, emu_ctx, oracle, tmp_path):
    import conftest
    exe = str(tmp_path / "pprobe_auto_emu")
    pp.build_cpp(conftest.build_emulator(), exe)
    pp.check_cpp(oracle, exe, tmp_path)
