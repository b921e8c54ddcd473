"""RGB / RGBA picture input (pfv_frames_from_rgb*, pfv_enc_ingest_rgb_dev, pfv_encoder_set_input_rgb) on a real MI355X: the shared checks of
tests/ingest_cases.py at the shapes of the emulator twin (tests/test_emu_ingest.py), every one an equality with the numpy oracle; and the
exhaustive pictures -- every (R, G, B) triple's Y in each of four, every triple's U and V once over the four -- through the wide path."""
import pytest

import ingest_cases as ic

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("w,h", ic.SHAPES)
def test_gpu_ingest_shapes(pkg, gpu_ctx, w, h):
    ic.check_shape(pkg, gpu_ctx, w, h)


@pytest.mark.parametrize("w,h", [(144, 48), (18, 18), (24, 6)])
def test_gpu_ingest_alignment(pkg, gpu_ctx, w, h):
    ic.check_alignment(pkg, gpu_ctx, w, h)


@pytest.mark.parametrize("w,h", [(144, 48), (34, 130)])
def test_gpu_ingest_point_equals_helper(pkg, gpu_ctx, w, h):
    ic.check_point_equals_helper(pkg, gpu_ctx, w, h)


@pytest.mark.parametrize("k", range(4))
def test_gpu_ingest_exhaustive(pkg, gpu_ctx, k):
    ic.check_exhaustive(pkg, gpu_ctx, k)


@pytest.mark.parametrize("fmt,chroma", [("rgb8", "point"), ("rgb8", "box"), ("bgra8", "point"), ("rgba8", "box")])
def test_gpu_ingest_enc_session(pkg, gpu_ctx, fmt, chroma):
    ic.check_enc_session(pkg, gpu_ctx, fmt, chroma)


def test_gpu_ingest_enc_session_graph(pkg, gpu_ctx):
    ic.check_enc_graph(pkg, gpu_ctx)


@pytest.mark.parametrize("config", list(ic.ENCODER_CONFIGS))
def test_gpu_ingest_encoder(pkg, gpu_ctx, config):
    ic.check_encoder(pkg, gpu_ctx, config)


@pytest.mark.parametrize("fmt", ["rgb8", "bgra8"])
def test_gpu_ingest_end_to_end(pkg, gpu_ctx, oracle, fmt):
    ic.check_end_to_end(pkg, gpu_ctx, oracle, fmt)


def test_gpu_ingest_bad_arguments(pkg, gpu_ctx):
    ic.check_bad_arguments(pkg, gpu_ctx)


def _lib(graft):
    import os
    lib = graft.build_hip()
    if os.environ.get("PFV_TEST_EMU_AS_GPU") == "1":          # developer dry-run without a GPU (tests/conftest.py)
        import conftest
        lib = conftest.build_emulator()
    return lib


def test_gpu_ingest_cpp_mirror(graft, pkg, gpu_ctx, tmp_path):
    exe = str(tmp_path / "ingest_report")
    ic.build_cpp(_lib(graft), exe)
    ic.check_cpp(pkg, gpu_ctx, exe, tmp_path)


def test_gpu_ingest_rd_tool(graft, pkg, gpu_ctx):
    ic.check_rd_tool(pkg, _lib(graft))
