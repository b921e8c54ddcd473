"""The denoising pre-filter (pfv_denoiser_*, pfv_frames_denoise, pfv_enc_denoise_dev, pfv_encoder_set_denoise, tools/rd_curve.py --denoise) on
the CPU emulator build of the kernel sources: the shared checks of tests/denoise_cases.py, every one an equality with the numpy restatement
of the header's text.  The GPU twin is tests/test_gpu_denoise.py."""
import pytest

import denoise_cases as dc


@pytest.mark.parametrize("w,h", dc.SHAPES)
def test_emu_denoise_shapes(pkg, emu_ctx, w, h):
    dc.check_shape(pkg, emu_ctx, w, h)


def test_emu_denoise_traps(pkg, emu_ctx):
    dc.check_traps(pkg, emu_ctx)


def test_emu_denoise_borders(pkg, emu_ctx):
    dc.check_borders(pkg, emu_ctx)


def test_emu_denoise_properties(pkg, emu_ctx):
    dc.check_properties(pkg, emu_ctx)


@pytest.mark.parametrize("w,h,px,py", [(144, 48, 16, 5), (144, 48, 128, 5), (144, 48, 5, 16), (50, 38, 49, 37)])
def test_emu_denoise_locality(pkg, emu_ctx, w, h, px, py):
    assert dc.check_locality(pkg, emu_ctx, w, h, px, py) >= 2


def test_emu_denoise_bad_arguments(pkg, emu_ctx):
    dc.check_bad_arguments(pkg, emu_ctx)


def test_emu_denoise_graph(pkg, emu_ctx):
    dc.check_graph(pkg, emu_ctx)


def test_emu_denoise_enc_session(pkg, emu_ctx):
    dc.check_enc_session(pkg, emu_ctx)


@pytest.mark.parametrize("config", list(dc.ENCODER_CONFIGS))
def test_emu_denoise_encoder(pkg, emu_ctx, oracle, config):
    dc.check_encoder(pkg, emu_ctx, oracle, config)


@pytest.mark.parametrize("quality", dc.EFFECT_QUALITIES)
def test_emu_denoise_effect(pkg, emu_ctx, quality):
    dc.check_effect(pkg, emu_ctx, quality)


def test_emu_denoise_cpp_mirror(pkg, emu_ctx, tmp_path):
    import conftest
    exe = str(tmp_path / "denoise_report_emu")
    dc.build_cpp(conftest.build_emulator(), exe)
    dc.check_cpp(pkg, emu_ctx, exe, tmp_path)


def test_emu_denoise_rd_tool(pkg, emu_ctx, oracle, tmp_path):
    import conftest
    dc.check_rd_tool(pkg, oracle, conftest.build_emulator(), tmp_path)
