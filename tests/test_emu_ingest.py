"""RGB / RGBA picture input (pfv_frames_from_rgb*, pfv_enc_ingest_rgb_dev, pfv_encoder_set_input_rgb, tools/rd_curve.py --time-ingest) on the
CPU emulator build of the kernel sources: the shared checks of tests/ingest_cases.py, every one an equality with the numpy oracle's
rgb_to_yuv420 (POINT) or the header's BOX rule over the oracle's per-pixel values.  The GPU twin is tests/test_gpu_ingest.py."""
import pytest

import ingest_cases as ic


@pytest.mark.parametrize("w,h", ic.SHAPES)
def test_emu_ingest_shapes(pkg, emu_ctx, w, h):
    ic.check_shape(pkg, emu_ctx, w, h)


@pytest.mark.parametrize("w,h", [(144, 48), (18, 18), (24, 6)])
def test_emu_ingest_alignment(pkg, emu_ctx, w, h):
    ic.check_alignment(pkg, emu_ctx, w, h)


@pytest.mark.parametrize("w,h", [(144, 48), (34, 130)])
def test_emu_ingest_point_equals_helper(pkg, emu_ctx, w, h):
    ic.check_point_equals_helper(pkg, emu_ctx, w, h)


def test_emu_ingest_exhaustive_reduced(pkg, emu_ctx):
    ic.check_exhaustive_reduced(pkg, emu_ctx)


@pytest.mark.parametrize("fmt,chroma", [("rgb8", "point"), ("rgb8", "box"), ("bgra8", "point"), ("rgba8", "box")])
def test_emu_ingest_enc_session(pkg, emu_ctx, fmt, chroma):
    ic.check_enc_session(pkg, emu_ctx, fmt, chroma)


def test_emu_ingest_enc_session_graph(pkg, emu_ctx):
    ic.check_enc_graph(pkg, emu_ctx)


@pytest.mark.parametrize("config", list(ic.ENCODER_CONFIGS))
def test_emu_ingest_encoder(pkg, emu_ctx, config):
    ic.check_encoder(pkg, emu_ctx, config)


@pytest.mark.parametrize("fmt", ["rgb8", "bgra8"])
def test_emu_ingest_end_to_end(pkg, emu_ctx, oracle, fmt):
    ic.check_end_to_end(pkg, emu_ctx, oracle, fmt)


def test_emu_ingest_bad_arguments(pkg, emu_ctx):
    ic.check_bad_arguments(pkg, emu_ctx)


def test_emu_ingest_cpp_mirror(pkg, emu_ctx, tmp_path):
    import conftest
    exe = str(tmp_path / "ingest_report_emu")
    ic.build_cpp(conftest.build_emulator(), exe)
    ic.check_cpp(pkg, emu_ctx, exe, tmp_path)


def test_emu_ingest_rd_tool(pkg, emu_ctx):
    import conftest
    ic.check_rd_tool(pkg, conftest.build_emulator())
