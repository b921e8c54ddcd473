"""Frame resize (pfv_scale_taps / _table, pfv_scaler_*, pfv_frames_scale) on the CPU emulator build of the kernel sources: the shared checks of
tests/scale_cases.py, every pixel check an equality with the numpy restatement of the header's arithmetic.  The GPU twin is
tests/test_gpu_scale.py."""
import pytest

import scale_cases as sc


def test_scale_tables(pkg, emu_ctx):
    sc.check_tables(pkg)


@pytest.mark.parametrize("sw,sh,dw,dh", sc.SHAPES)
def test_emu_scale_shapes(pkg, emu_ctx, sw, sh, dw, dh):
    sc.check_shape(pkg, emu_ctx, sw, sh, dw, dh)


def test_emu_scale_constant(pkg, emu_ctx):
    sc.check_constant(pkg, emu_ctx)


@pytest.mark.parametrize("sw,sh,dw,dh", [(144, 80, 96, 54), (130, 34, 66, 18), (18, 10, 34, 22)])
def test_emu_scale_layouts(pkg, emu_ctx, sw, sh, dw, dh):
    sc.check_layouts(pkg, emu_ctx, sw, sh, dw, dh)


def test_emu_scale_bad_arguments(pkg, emu_ctx):
    sc.check_bad_arguments(pkg, emu_ctx)


def test_emu_scale_graph(pkg, emu_ctx):
    sc.check_graph(pkg, emu_ctx)


@pytest.mark.parametrize("rgb", [False, True], ids=["no_rgb", "rgb_beside"])
@pytest.mark.parametrize("planar", [False, True], ids=["scaled_only", "planar_beside"])
@pytest.mark.parametrize("deblock", ["off", "auto", "fixed"])
def test_emu_scale_dec_session(pkg, emu_ctx, oracle, deblock, planar, rgb):
    sc.check_dec_session(pkg, emu_ctx, oracle, deblock, planar, rgb)


def test_emu_scale_dec_session_forms(pkg, emu_ctx, oracle):
    sc.check_dec_forms(pkg, emu_ctx, oracle)


def test_emu_scale_dec_session_graph(pkg, emu_ctx, oracle):
    sc.check_dec_graph(pkg, emu_ctx, oracle)


@pytest.mark.parametrize("deblock", ["off", "auto"])
@pytest.mark.parametrize("device_out", [False, True], ids=["host_out", "device_out"])
@pytest.mark.parametrize("entropy", ["device", "host"])
def test_emu_scale_decoder(pkg, emu_ctx, oracle, entropy, device_out, deblock):
    sc.check_decoder(pkg, emu_ctx, oracle, entropy, device_out, deblock)


@pytest.mark.parametrize("kind", list(sc.KINDS))
def test_emu_scale_enc_session(pkg, emu_ctx, kind):
    sc.check_enc_session(pkg, emu_ctx, kind)


@pytest.mark.parametrize("config", list(sc.ENCODER_CONFIGS))
def test_emu_scale_encoder(pkg, emu_ctx, config):
    sc.check_encoder(pkg, emu_ctx, config)


def test_emu_scale_bad_arguments_sessions(pkg, emu_ctx, oracle):
    sc.check_bad_arguments_sessions(pkg, emu_ctx, oracle)


def test_emu_scale_cpp_mirror(pkg, emu_ctx, oracle, tmp_path):
    import conftest
    exe = str(tmp_path / "scale_report_emu")
    sc.build_cpp(conftest.build_emulator(), exe)
    sc.check_cpp(pkg, emu_ctx, oracle, exe, tmp_path)


def test_emu_scale_rd_tool(pkg, emu_ctx):
    import conftest
    sc.check_rd_tool(pkg, conftest.build_emulator())
