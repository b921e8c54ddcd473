"""Structural similarity on the device (pfv_frames_ssim*, pfv_ssim, pfv_ssim_windows, pfv_enc / pfv_dec_ssim_dev, pfv_encoder's frame SSIM,
tools/rd_curve.py --ssim) on the CPU emulator build of the kernel sources: the shared checks of tests/ssim_cases.py against numpy and the
oracle, inside the tolerance derived there and exact where the value is known.  The GPU twin is tests/test_gpu_ssim.py."""
import pytest

import ssim_cases as sc


@pytest.mark.parametrize("w,h", sc.SHAPES)
def test_emu_ssim_plane_shapes(pkg, emu_ctx, w, h):
    sc.check_plane_shape(pkg, emu_ctx, w, h)


def test_emu_ssim_windows_and_value(pkg, emu_ctx):
    sc.check_windows(pkg)
    sc.check_ssim_value(pkg)


@pytest.mark.parametrize("w,h", [(18, 34), (50, 38), (144, 48), (64, 48)])
def test_emu_ssim_near_copy(pkg, emu_ctx, w, h):
    sc.check_near_copy(pkg, emu_ctx, w, h)


@pytest.mark.parametrize("w,h", [(20, 20), (144, 48)])
def test_emu_ssim_checkerboard(pkg, emu_ctx, w, h):
    sc.check_checkerboard(pkg, emu_ctx, w, h)


@pytest.mark.parametrize("w,h", sc.SHAPES)
def test_emu_ssim_identical(pkg, emu_ctx, w, h):
    sc.check_identical(pkg, emu_ctx, w, h)


def test_emu_ssim_extremes(pkg, emu_ctx):
    sc.check_extremes(pkg, emu_ctx)


@pytest.mark.parametrize("w,h", [(18, 34), (64, 48)])
def test_emu_ssim_strided_streams(pkg, emu_ctx, w, h):
    sc.check_strided_streams(pkg, emu_ctx, w, h)


@pytest.mark.parametrize("w,h,px,py,n_owners", [(144, 48, 16, 5, 2), (144, 48, 128, 5, 2), (144, 48, 5, 16, 2), (50, 38, 49, 37, 0)])
def test_emu_ssim_single_pixel(pkg, emu_ctx, w, h, px, py, n_owners):
    assert len(sc.check_single_pixel(pkg, emu_ctx, w, h, px, py)) == n_owners


def test_emu_ssim_bad_arguments(pkg, emu_ctx):
    sc.check_bad_arguments(pkg, emu_ctx)


def test_emu_ssim_enc_session(pkg, emu_ctx, oracle):
    sc.check_enc_session(pkg, emu_ctx, oracle)


def test_emu_ssim_enc_session_window(pkg, emu_ctx, oracle):
    sc.check_enc_session_window(pkg, emu_ctx, oracle)


def test_emu_ssim_enc_session_stride(pkg, emu_ctx, oracle):
    sc.check_enc_session_stride(pkg, emu_ctx, oracle)


def test_emu_ssim_dec_session(pkg, emu_ctx, oracle):
    sc.check_dec_session(pkg, emu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_emu_ssim_encoder_frame_ssim(pkg, emu_ctx, oracle, device_entropy):
    sc.check_encoder_ssim(pkg, emu_ctx, oracle, device_entropy)


def test_emu_ssim_encoder_both_switches(pkg, emu_ctx):
    sc.check_encoder_ssim_with_reports(pkg, emu_ctx)


def test_emu_ssim_graph(pkg, emu_ctx, oracle):
    sc.check_graph(pkg, emu_ctx, oracle)


def test_emu_ssim_cpp_mirror(pkg, emu_ctx, tmp_path):
    import conftest
    exe = str(tmp_path / "ssim_report_emu")
    sc.build_cpp(conftest.build_emulator(), exe)
    sc.check_cpp_ssim(pkg, emu_ctx, exe, tmp_path)


def test_emu_ssim_rd_tool(pkg, emu_ctx, oracle):
    import conftest
    sc.check_rd_tool(pkg, oracle, conftest.build_emulator())
