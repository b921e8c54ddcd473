"""The denoising pre-filter (pfv_denoiser_*, pfv_frames_denoise, pfv_enc_denoise_dev, pfv_encoder_set_denoise) on a real MI355X: the shared
checks of tests/denoise_cases.py at the shapes of the emulator twin (tests/test_emu_denoise.py), every one an equality with the numpy
restatement of the header's text."""
import pytest

import denoise_cases as dc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("w,h", dc.SHAPES)
def test_gpu_denoise_shapes(pkg, gpu_ctx, w, h):
    dc.check_shape(pkg, gpu_ctx, w, h)


def test_gpu_denoise_traps(pkg, gpu_ctx):
    dc.check_traps(pkg, gpu_ctx)


def test_gpu_denoise_borders(pkg, gpu_ctx):
    dc.check_borders(pkg, gpu_ctx)


def test_gpu_denoise_properties(pkg, gpu_ctx):
    dc.check_properties(pkg, gpu_ctx)


@pytest.mark.parametrize("w,h,px,py", [(144, 48, 16, 5), (144, 48, 128, 5), (144, 48, 5, 16), (50, 38, 49, 37)])
def test_gpu_denoise_locality(pkg, gpu_ctx, w, h, px, py):
    assert dc.check_locality(pkg, gpu_ctx, w, h, px, py) >= 2


def test_gpu_denoise_bad_arguments(pkg, gpu_ctx):
    dc.check_bad_arguments(pkg, gpu_ctx)


def test_gpu_denoise_graph(pkg, gpu_ctx):
    dc.check_graph(pkg, gpu_ctx)


def test_gpu_denoise_enc_session(pkg, gpu_ctx):
    dc.check_enc_session(pkg, gpu_ctx)


@pytest.mark.parametrize("config", list(dc.ENCODER_CONFIGS))
def test_gpu_denoise_encoder(pkg, gpu_ctx, oracle, config):
    dc.check_encoder(pkg, gpu_ctx, oracle, config)


@pytest.mark.parametrize("quality", dc.EFFECT_QUALITIES)
def test_gpu_denoise_effect(pkg, gpu_ctx, quality):
    dc.check_effect(pkg, gpu_ctx, quality)


def _lib(graft):
    import os
    lib = graft.build_hip()
    if os.environ.get("PFV_TEST_EMU_AS_GPU") == "1":          # developer dry-run without a GPU (tests/conftest.py)
        import conftest
        lib = conftest.build_emulator()
    return lib


def test_gpu_denoise_cpp_mirror(graft, pkg, gpu_ctx, tmp_path):
    exe = str(tmp_path / "denoise_report")
    dc.build_cpp(_lib(graft), exe)
    dc.check_cpp(pkg, gpu_ctx, exe, tmp_path)


def test_gpu_denoise_rd_tool(graft, pkg, gpu_ctx, oracle, tmp_path):
    dc.check_rd_tool(pkg, oracle, _lib(graft), tmp_path)
