"""Frame resize (pfv_scale_taps / _table, pfv_scaler_*, pfv_frames_scale) on a real MI355X: the shared checks of tests/scale_cases.py at the
shapes of the emulator twin (tests/test_emu_scale.py), every pixel check an equality with the numpy restatement of the header's arithmetic;
and quarter-1080p frames down to 640x360 and up to 1920x1080 -- many tiles per plane, interior tiles on the dword path (960, 480, 640, 320,
1920 are multiples of 4) and, from a source base offset by one byte into an odd destination stride, the same frames on the byte path."""
import numpy as np
import pytest

import scale_cases as sc

pytestmark = pytest.mark.gpu


def test_gpu_scale_tables(pkg, gpu_ctx):
    sc.check_tables(pkg)


@pytest.mark.parametrize("sw,sh,dw,dh", sc.SHAPES)
def test_gpu_scale_shapes(pkg, gpu_ctx, sw, sh, dw, dh):
    sc.check_shape(pkg, gpu_ctx, sw, sh, dw, dh)


def test_gpu_scale_constant(pkg, gpu_ctx):
    sc.check_constant(pkg, gpu_ctx)


@pytest.mark.parametrize("sw,sh,dw,dh", [(144, 80, 96, 54), (130, 34, 66, 18), (18, 10, 34, 22)])
def test_gpu_scale_layouts(pkg, gpu_ctx, sw, sh, dw, dh):
    sc.check_layouts(pkg, gpu_ctx, sw, sh, dw, dh)


def test_gpu_scale_bad_arguments(pkg, gpu_ctx):
    sc.check_bad_arguments(pkg, gpu_ctx)


def test_gpu_scale_graph(pkg, gpu_ctx):
    sc.check_graph(pkg, gpu_ctx)


@pytest.fixture(scope="module")
def qhd_frames():
    return sc.hard_frames(960, 540, 2, np.random.default_rng(540))


@pytest.mark.parametrize("kind", list(sc.KINDS))
@pytest.mark.parametrize("dw,dh", [(640, 360), (1920, 1080)])
def test_gpu_scale_qhd(pkg, gpu_ctx, qhd_frames, dw, dh, kind):
    sc.check_big(pkg, gpu_ctx, qhd_frames, 960, 540, dw, dh, kind)


@pytest.mark.parametrize("rgb", [False, True], ids=["no_rgb", "rgb_beside"])
@pytest.mark.parametrize("planar", [False, True], ids=["scaled_only", "planar_beside"])
@pytest.mark.parametrize("deblock", ["off", "auto", "fixed"])
def test_gpu_scale_dec_session(pkg, gpu_ctx, oracle, deblock, planar, rgb):
    sc.check_dec_session(pkg, gpu_ctx, oracle, deblock, planar, rgb)


def test_gpu_scale_dec_session_forms(pkg, gpu_ctx, oracle):
    sc.check_dec_forms(pkg, gpu_ctx, oracle)


def test_gpu_scale_dec_session_graph(pkg, gpu_ctx, oracle):
    sc.check_dec_graph(pkg, gpu_ctx, oracle)


@pytest.mark.parametrize("deblock", ["off", "auto"])
@pytest.mark.parametrize("device_out", [False, True], ids=["host_out", "device_out"])
@pytest.mark.parametrize("entropy", ["device", "host"])
def test_gpu_scale_decoder(pkg, gpu_ctx, oracle, entropy, device_out, deblock):
    sc.check_decoder(pkg, gpu_ctx, oracle, entropy, device_out, deblock)


@pytest.mark.parametrize("kind", list(sc.KINDS))
def test_gpu_scale_enc_session(pkg, gpu_ctx, kind):
    sc.check_enc_session(pkg, gpu_ctx, kind)


@pytest.mark.parametrize("config", list(sc.ENCODER_CONFIGS))
def test_gpu_scale_encoder(pkg, gpu_ctx, config):
    sc.check_encoder(pkg, gpu_ctx, config)


def test_gpu_scale_bad_arguments_sessions(pkg, gpu_ctx, oracle):
    sc.check_bad_arguments_sessions(pkg, gpu_ctx, oracle)


def _lib(graft):
    import os
    lib = graft.build_hip()
    if os.environ.get("PFV_TEST_EMU_AS_GPU") == "1":          # developer dry-run without a GPU (tests/conftest.py)
        import conftest
        lib = conftest.build_emulator()
    return lib


def test_gpu_scale_cpp_mirror(graft, pkg, gpu_ctx, oracle, tmp_path):
    exe = str(tmp_path / "scale_report")
    sc.build_cpp(_lib(graft), exe)
    sc.check_cpp(pkg, gpu_ctx, oracle, exe, tmp_path)


def test_gpu_scale_rd_tool(graft, pkg, gpu_ctx):
    sc.check_rd_tool(pkg, _lib(graft))
