"""Structural similarity on the device (pfv_frames_ssim*, pfv_ssim, pfv_ssim_windows, pfv_enc / pfv_dec_ssim_dev, pfv_encoder's frame SSIM)
on a real MI355X: the shared checks of tests/ssim_cases.py at the shapes of the emulator twin (tests/test_emu_ssim.py), against numpy and
the oracle, inside the tolerance derived there and exact where the value is known."""
import pytest

import ssim_cases as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("w,h", sc.SHAPES)
def test_gpu_ssim_plane_shapes(pkg, gpu_ctx, w, h):
    sc.check_plane_shape(pkg, gpu_ctx, w, h)


def test_gpu_ssim_windows_and_value(pkg, gpu_ctx):
    sc.check_windows(pkg)
    sc.check_ssim_value(pkg)


@pytest.mark.parametrize("w,h", [(18, 34), (50, 38), (144, 48), (64, 48)])
def test_gpu_ssim_near_copy(pkg, gpu_ctx, w, h):
    sc.check_near_copy(pkg, gpu_ctx, w, h)


@pytest.mark.parametrize("w,h", [(20, 20), (144, 48)])
def test_gpu_ssim_checkerboard(pkg, gpu_ctx, w, h):
    sc.check_checkerboard(pkg, gpu_ctx, w, h)


@pytest.mark.parametrize("w,h", sc.SHAPES)
def test_gpu_ssim_identical(pkg, gpu_ctx, w, h):
    sc.check_identical(pkg, gpu_ctx, w, h)


def test_gpu_ssim_extremes(pkg, gpu_ctx):
    sc.check_extremes(pkg, gpu_ctx)


@pytest.mark.parametrize("w,h", [(18, 34), (64, 48)])
def test_gpu_ssim_strided_streams(pkg, gpu_ctx, w, h):
    sc.check_strided_streams(pkg, gpu_ctx, w, h)


@pytest.mark.parametrize("w,h,px,py,n_owners", [(144, 48, 16, 5, 2), (144, 48, 128, 5, 2), (144, 48, 5, 16, 2), (50, 38, 49, 37, 0)])
def test_gpu_ssim_single_pixel(pkg, gpu_ctx, w, h, px, py, n_owners):
    assert len(sc.check_single_pixel(pkg, gpu_ctx, w, h, px, py)) == n_owners


def test_gpu_ssim_bad_arguments(pkg, gpu_ctx):
    sc.check_bad_arguments(pkg, gpu_ctx)


def test_gpu_ssim_enc_session(pkg, gpu_ctx, oracle):
    sc.check_enc_session(pkg, gpu_ctx, oracle)


def test_gpu_ssim_enc_session_window(pkg, gpu_ctx, oracle):
    sc.check_enc_session_window(pkg, gpu_ctx, oracle)


def test_gpu_ssim_enc_session_stride(pkg, gpu_ctx, oracle):
    sc.check_enc_session_stride(pkg, gpu_ctx, oracle)


def test_gpu_ssim_dec_session(pkg, gpu_ctx, oracle):
    sc.check_dec_session(pkg, gpu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_gpu_ssim_encoder_frame_ssim(pkg, gpu_ctx, oracle, device_entropy):
    sc.check_encoder_ssim(pkg, gpu_ctx, oracle, device_entropy)


def test_gpu_ssim_encoder_both_switches(pkg, gpu_ctx):
    sc.check_encoder_ssim_with_reports(pkg, gpu_ctx)


def test_gpu_ssim_graph(pkg, gpu_ctx, oracle):
    sc.check_graph(pkg, gpu_ctx, oracle)


def test_gpu_ssim_cpp_mirror(graft, pkg, gpu_ctx, tmp_path):
    import os
    lib = graft.build_hip()
    if os.environ.get("PFV_TEST_EMU_AS_GPU") == "1":          # developer dry-run without a GPU (tests/conftest.py)
        import conftest
        lib = conftest.build_emulator()
    exe = str(tmp_path / "ssim_report")
    sc.build_cpp(lib, exe)
    sc.check_cpp_ssim(pkg, gpu_ctx, exe, tmp_path)


def test_gpu_ssim_rd_tool(graft, pkg, gpu_ctx, oracle):
    import os
    lib = graft.build_hip()
    if os.environ.get("PFV_TEST_EMU_AS_GPU") == "1":
        import conftest
        lib = conftest.build_emulator()
    sc.check_rd_tool(pkg, oracle, lib)
