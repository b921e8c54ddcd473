"""The encoders' quality ladder and pfv_encoder's p-frame byte budget on a real MI355X: the
shared checks of tests/ladder_cases.py at the shapes of the emulator twin (tests/test_emu_ladder.py), exact against a ladder model made of
the oracle's plane-level functions."""
import pytest

import ladder_cases as lc

pytestmark = pytest.mark.gpu

LANES = [1, 2]      # PFV_LANES_PER_MB_8, PFV_LANES_PER_MB_16: the existing kernels are launched with new table pointers under both mappings


@pytest.mark.parametrize("lanes", LANES, ids=["lanes8", "lanes16"])
@pytest.mark.parametrize("w,h,n", lc.SHAPES)
def test_gpu_ladder_session_rungs(pkg, gpu_ctx, oracle, w, h, n, lanes):
    lc.check_session_rungs(pkg, gpu_ctx, oracle, w, h, n, lane_mapping=lanes)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_gpu_ladder_encoder(pkg, gpu_ctx, oracle, device_entropy):
    lc.check_encoder_ladder(pkg, gpu_ctx, oracle, device_entropy)


def test_gpu_ladder_one_rung_is_todays_encoder(pkg, gpu_ctx, oracle):
    lc.check_one_rung_is_todays_encoder(pkg, gpu_ctx, oracle)


@pytest.mark.parametrize("w,h,device_entropy", [(64, 48, True), (50, 38, True), (50, 38, False)], ids=["64x48", "50x38", "50x38_host_entropy"])
def test_gpu_ladder_rate_controller(pkg, gpu_ctx, oracle, w, h, device_entropy):
    lc.check_rate_controller(pkg, gpu_ctx, oracle, w, h, device_entropy)


def test_gpu_ladder_arguments(pkg, gpu_ctx):
    lc.check_arguments(pkg, gpu_ctx)


def test_gpu_ladder_cpp_mirror(graft, pkg, gpu_ctx, oracle, tmp_path):
    import os
    lib = graft.build_hip()
    if os.environ.get("PFV_TEST_EMU_AS_GPU") == "1":          # developer dry-run without a GPU (tests/conftest.py)
        import conftest
        lib = conftest.build_emulator()
    exe = str(tmp_path / "ladder_rate")
    lc.build_cpp(lib, exe)
    lc.check_cpp_rate(pkg, gpu_ctx, oracle, exe, tmp_path)
