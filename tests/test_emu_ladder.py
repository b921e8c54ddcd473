"""The encoders' quality ladder and pfv_encoder's p-frame byte budget on the CPU emulator
build of the kernel sources: the shared checks of tests/ladder_cases.py, exact against a ladder model made of the oracle's plane-level
functions.  The GPU twin is tests/test_gpu_ladder.py."""
import pytest

import ladder_cases as lc


@pytest.mark.parametrize("w,h,n", lc.SHAPES)
def test_emu_ladder_session_rungs(pkg, emu_ctx, oracle, w, h, n):
    lc.check_session_rungs(pkg, emu_ctx, oracle, w, h, n)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_emu_ladder_encoder(pkg, emu_ctx, oracle, device_entropy):
    lc.check_encoder_ladder(pkg, emu_ctx, oracle, device_entropy)


def test_emu_ladder_one_rung_is_todays_encoder(pkg, emu_ctx, oracle):
    lc.check_one_rung_is_todays_encoder(pkg, emu_ctx, oracle)


@pytest.mark.parametrize("w,h,device_entropy", [(64, 48, True), (50, 38, True), (50, 38, False)], ids=["64x48", "50x38", "50x38_host_entropy"])
def test_emu_ladder_rate_controller(pkg, emu_ctx, oracle, w, h, device_entropy):
    lc.check_rate_controller(pkg, emu_ctx, oracle, w, h, device_entropy)


def test_emu_ladder_arguments(pkg, emu_ctx):
    lc.check_arguments(pkg, emu_ctx)


def test_emu_ladder_cpp_mirror(pkg, emu_ctx, oracle, tmp_path):
    import conftest
    exe = str(tmp_path / "ladder_rate_emu")
    lc.build_cpp(conftest.build_emulator(), exe)
    lc.check_cpp_rate(pkg, emu_ctx, oracle, exe, tmp_path)
