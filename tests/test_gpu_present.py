"""RGB / RGBA texture output (pfv_frames_to_rgb*, pfv_dec_get_frame_rgb*, pfv_dec_set_output_rgb_dev, pfv_decoder_set_output_rgb) on a real
MI355X: the shared checks of tests/present_cases.py at the shapes of the emulator twin (tests/test_emu_present.py), every one an equality
with the numpy oracle's yuv420_to_rgb; and the exhaustive frame -- every (Y, U, V) triple once -- through the wide path."""
import pytest

import present_cases as pc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("w,h", pc.SHAPES)
def test_gpu_present_shapes(pkg, gpu_ctx, w, h):
    pc.check_shape(pkg, gpu_ctx, w, h)


@pytest.mark.parametrize("w,h", [(144, 48), (18, 18)])
def test_gpu_present_alignment(pkg, gpu_ctx, w, h):
    pc.check_alignment(pkg, gpu_ctx, w, h)


def test_gpu_present_exhaustive(pkg, gpu_ctx):
    pc.check_exhaustive(pkg, gpu_ctx, full=True)


@pytest.mark.parametrize("fmt", list(pc.FORMATS))
@pytest.mark.parametrize("planar", [False, True], ids=["rgb_only", "planar_beside"])
@pytest.mark.parametrize("deblock", ["off", "auto", "fixed"])
def test_gpu_present_dec_session(pkg, gpu_ctx, oracle, deblock, planar, fmt):
    pc.check_dec_session(pkg, gpu_ctx, oracle, deblock, planar, fmt)


def test_gpu_present_dec_session_forms(pkg, gpu_ctx, oracle):
    pc.check_dec_forms(pkg, gpu_ctx, oracle)


def test_gpu_present_dec_session_graph(pkg, gpu_ctx, oracle):
    pc.check_dec_graph(pkg, gpu_ctx, oracle)


@pytest.mark.parametrize("deblock", ["off", "auto"])
@pytest.mark.parametrize("device_out", [False, True], ids=["host_out", "device_out"])
@pytest.mark.parametrize("entropy", ["device", "host"])
def test_gpu_present_decoder(pkg, gpu_ctx, oracle, entropy, device_out, deblock):
    pc.check_decoder(pkg, gpu_ctx, oracle, entropy, device_out, deblock)


def test_gpu_present_bad_arguments(pkg, gpu_ctx, oracle):
    pc.check_bad_arguments(pkg, gpu_ctx, oracle)


def _lib(graft):
    import os
    lib = graft.build_hip()
    if os.environ.get("PFV_TEST_EMU_AS_GPU") == "1":          # developer dry-run without a GPU (tests/conftest.py)
        import conftest
        lib = conftest.build_emulator()
    return lib


def test_gpu_present_cpp_mirror(graft, pkg, gpu_ctx, oracle, tmp_path):
    exe = str(tmp_path / "present_report")
    pc.build_cpp(_lib(graft), exe)
    pc.check_cpp(pkg, gpu_ctx, oracle, exe, tmp_path)


def test_gpu_present_rd_tool(graft, pkg, gpu_ctx):
    pc.check_rd_tool(pkg, _lib(graft))
