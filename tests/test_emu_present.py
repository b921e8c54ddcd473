"""RGB / RGBA texture output (pfv_frames_to_rgb*, pfv_dec_get_frame_rgb*, pfv_dec_set_output_rgb_dev, pfv_decoder_set_output_rgb,
tools/rd_curve.py --time-present) on the CPU emulator build of the kernel sources: the shared checks of tests/present_cases.py, every one an
equality with the numpy oracle's yuv420_to_rgb.  The GPU twin is tests/test_gpu_present.py."""
import pytest

import present_cases as pc


@pytest.mark.parametrize("w,h", pc.SHAPES)
def test_emu_present_shapes(pkg, emu_ctx, w, h):
    pc.check_shape(pkg, emu_ctx, w, h)


@pytest.mark.parametrize("w,h", [(144, 48), (18, 18)])
def test_emu_present_alignment(pkg, emu_ctx, w, h):
    pc.check_alignment(pkg, emu_ctx, w, h)


def test_emu_present_exhaustive_reduced(pkg, emu_ctx):
    pc.check_exhaustive(pkg, emu_ctx, full=False)


@pytest.mark.parametrize("fmt", list(pc.FORMATS))
@pytest.mark.parametrize("planar", [False, True], ids=["rgb_only", "planar_beside"])
@pytest.mark.parametrize("deblock", ["off", "auto", "fixed"])
def test_emu_present_dec_session(pkg, emu_ctx, oracle, deblock, planar, fmt):
    pc.check_dec_session(pkg, emu_ctx, oracle, deblock, planar, fmt)


def test_emu_present_dec_session_forms(pkg, emu_ctx, oracle):
    pc.check_dec_forms(pkg, emu_ctx, oracle)


def test_emu_present_dec_session_graph(pkg, emu_ctx, oracle):
    pc.check_dec_graph(pkg, emu_ctx, oracle)


@pytest.mark.parametrize("deblock", ["off", "auto"])
@pytest.mark.parametrize("device_out", [False, True], ids=["host_out", "device_out"])
@pytest.mark.parametrize("entropy", ["device", "host"])
def test_emu_present_decoder(pkg, emu_ctx, oracle, entropy, device_out, deblock):
    pc.check_decoder(pkg, emu_ctx, oracle, entropy, device_out, deblock)


def test_emu_present_bad_arguments(pkg, emu_ctx, oracle):
    pc.check_bad_arguments(pkg, emu_ctx, oracle)


def test_emu_present_cpp_mirror(pkg, emu_ctx, oracle, tmp_path):
    import conftest
    exe = str(tmp_path / "present_report_emu")
    pc.build_cpp(conftest.build_emulator(), exe)
    pc.check_cpp(pkg, emu_ctx, oracle, exe, tmp_path)


def test_emu_present_rd_tool(pkg, emu_ctx):
    import conftest
    pc.check_rd_tool(pkg, conftest.build_emulator())
