"""Distortion on the device (pfv_frames_sse*, pfv_psnr, pfv_enc / pfv_dec_distortion_dev, pfv_encoder's frame reports) on a real MI355X:
the shared checks of tests/quality_cases.py at the shapes of the emulator twin (tests/test_emu_quality.py), exact against numpy and the
oracle."""
import pytest

import quality_cases as qc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("w,h", qc.SHAPES)
def test_gpu_quality_plane_shapes(pkg, gpu_ctx, w, h):
    qc.check_plane_shape(pkg, gpu_ctx, w, h)


@pytest.mark.parametrize("w,h", [(18, 34), (64, 48)])
def test_gpu_quality_strided_streams(pkg, gpu_ctx, w, h):
    qc.check_strided_streams(pkg, gpu_ctx, w, h)


def test_gpu_quality_same_buffer(pkg, gpu_ctx):
    qc.check_same_buffer(pkg, gpu_ctx, 50, 38)


@pytest.mark.parametrize("w,h", qc.SHAPES)
def test_gpu_quality_corner_pixel(pkg, gpu_ctx, w, h):
    qc.check_corner_pixel(pkg, gpu_ctx, w, h)


def test_gpu_quality_extremes(pkg, gpu_ctx):
    qc.check_extremes(pkg, gpu_ctx)


def test_gpu_quality_bad_arguments(pkg, gpu_ctx):
    qc.check_bad_arguments(pkg, gpu_ctx)


def test_gpu_quality_psnr(pkg, gpu_ctx):
    qc.check_psnr(pkg)


def test_gpu_quality_enc_session(pkg, gpu_ctx, oracle):
    qc.check_enc_session(pkg, gpu_ctx, oracle)


def test_gpu_quality_enc_session_window(pkg, gpu_ctx, oracle):
    qc.check_enc_session_window(pkg, gpu_ctx, oracle)


def test_gpu_quality_enc_session_stride(pkg, gpu_ctx, oracle):
    qc.check_enc_session_stride(pkg, gpu_ctx, oracle)


def test_gpu_quality_dec_session(pkg, gpu_ctx, oracle):
    qc.check_dec_session(pkg, gpu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_gpu_quality_encoder_reports(pkg, gpu_ctx, oracle, device_entropy):
    qc.check_encoder_reports(pkg, gpu_ctx, oracle, device_entropy)


def test_gpu_quality_graph(pkg, gpu_ctx, oracle):
    qc.check_graph(pkg, gpu_ctx, oracle)


def test_gpu_quality_cpp_mirror(graft, pkg, gpu_ctx, tmp_path):
    import os
    lib = graft.build_hip()
    if os.environ.get("PFV_TEST_EMU_AS_GPU") == "1":          # developer dry-run without a GPU (tests/conftest.py)
        import conftest
        lib = conftest.build_emulator()
    exe = str(tmp_path / "quality_report")
    qc.build_cpp(lib, exe)
    qc.check_cpp_reports(pkg, gpu_ctx, exe, tmp_path)
