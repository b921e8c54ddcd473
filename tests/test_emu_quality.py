"""Distortion on the device (pfv_frames_sse*, pfv_psnr, pfv_enc / pfv_dec_distortion_dev, pfv_encoder's frame reports, tools/rd_curve.py)
on the CPU emulator build of the kernel sources: the shared checks of tests/quality_cases.py, exact against numpy and the oracle.  The GPU
twin is tests/test_gpu_quality.py."""
import pytest

import quality_cases as qc


@pytest.mark.parametrize("w,h", qc.SHAPES)
def test_emu_quality_plane_shapes(pkg, emu_ctx, w, h):
    qc.check_plane_shape(pkg, emu_ctx, w, h)


@pytest.mark.parametrize("w,h", [(18, 34), (64, 48)])
def test_emu_quality_strided_streams(pkg, emu_ctx, w, h):
    qc.check_strided_streams(pkg, emu_ctx, w, h)


def test_emu_quality_same_buffer(pkg, emu_ctx):
    qc.check_same_buffer(pkg, emu_ctx, 50, 38)


@pytest.mark.parametrize("w,h", qc.SHAPES)
def test_emu_quality_corner_pixel(pkg, emu_ctx, w, h):
    qc.check_corner_pixel(pkg, emu_ctx, w, h)


def test_emu_quality_extremes(pkg, emu_ctx):
    qc.check_extremes(pkg, emu_ctx)


def test_emu_quality_bad_arguments(pkg, emu_ctx):
    qc.check_bad_arguments(pkg, emu_ctx)


def test_emu_quality_psnr(pkg, emu_ctx):
    qc.check_psnr(pkg)


def test_emu_quality_enc_session(pkg, emu_ctx, oracle):
    qc.check_enc_session(pkg, emu_ctx, oracle)


def test_emu_quality_enc_session_window(pkg, emu_ctx, oracle):
    qc.check_enc_session_window(pkg, emu_ctx, oracle)


def test_emu_quality_enc_session_stride(pkg, emu_ctx, oracle):
    qc.check_enc_session_stride(pkg, emu_ctx, oracle)


def test_emu_quality_dec_session(pkg, emu_ctx, oracle):
    qc.check_dec_session(pkg, emu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_emu_quality_encoder_reports(pkg, emu_ctx, oracle, device_entropy):
    qc.check_encoder_reports(pkg, emu_ctx, oracle, device_entropy)


def test_emu_quality_graph(pkg, emu_ctx, oracle):
    qc.check_graph(pkg, emu_ctx, oracle)


def test_emu_quality_cpp_mirror(pkg, emu_ctx, tmp_path):
    import conftest
    exe = str(tmp_path / "quality_report_emu")
    qc.build_cpp(conftest.build_emulator(), exe)
    qc.check_cpp_reports(pkg, emu_ctx, exe, tmp_path)


def test_emu_quality_rd_tool(pkg, emu_ctx, oracle):
    import conftest
    qc.check_rd_tool(pkg, oracle, conftest.build_emulator())
