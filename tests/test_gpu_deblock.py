"""Out-of-loop deblocking (pfv_frames_deblock*, pfv_deblock_strength, pfv_dec_set_deblock, pfv_decoder_set_deblock) on a real MI355X: the
shared checks of tests/deblock_cases.py at the shapes of the emulator twin (tests/test_emu_deblock.py), every one an equality with the numpy
restatement of the header's text."""
import pytest

import deblock_cases as dc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("w,h", dc.SHAPES)
def test_gpu_deblock_shapes(pkg, gpu_ctx, w, h):
    dc.check_shape(pkg, gpu_ctx, w, h)


def test_gpu_deblock_traps(pkg, gpu_ctx):
    dc.check_traps(pkg, gpu_ctx)


def test_gpu_deblock_properties(pkg, gpu_ctx):
    dc.check_properties(pkg, gpu_ctx)


@pytest.mark.parametrize("w,h,px,py", [(144, 48, 16, 5), (144, 48, 128, 5), (144, 48, 5, 16), (50, 38, 49, 37)])
def test_gpu_deblock_locality(pkg, gpu_ctx, w, h, px, py):
    assert dc.check_locality(pkg, gpu_ctx, w, h, px, py) >= 1


def test_gpu_deblock_bad_arguments(pkg, gpu_ctx):
    dc.check_bad_arguments(pkg, gpu_ctx)


def test_gpu_deblock_strength(pkg, gpu_ctx):
    dc.check_strength(pkg)


@pytest.mark.parametrize("path", ["get_frame", "output", "strided"])
def test_gpu_deblock_dec_session(pkg, gpu_ctx, oracle, path):
    dc.check_dec_session(pkg, gpu_ctx, oracle, path)


def test_gpu_deblock_dec_session_graph(pkg, gpu_ctx, oracle):
    dc.check_dec_graph(pkg, gpu_ctx, oracle)


@pytest.mark.parametrize("device_out", [False, True], ids=["host_out", "device_out"])
@pytest.mark.parametrize("entropy", ["device", "host"])
def test_gpu_deblock_decoder(pkg, gpu_ctx, oracle, entropy, device_out):
    dc.check_decoder(pkg, gpu_ctx, oracle, entropy, device_out)


@pytest.mark.parametrize("quality", [0, 2, 5, 10])
def test_gpu_deblock_effect(pkg, gpu_ctx, oracle, quality):
    dc.check_effect(pkg, gpu_ctx, oracle, quality)


def _lib(graft):
    import os
    lib = graft.build_hip()
    if os.environ.get("PFV_TEST_EMU_AS_GPU") == "1":          # developer dry-run without a GPU (tests/conftest.py)
        import conftest
        lib = conftest.build_emulator()
    return lib


def test_gpu_deblock_cpp_mirror(graft, pkg, gpu_ctx, oracle, tmp_path):
    exe = str(tmp_path / "deblock_report")
    dc.build_cpp(_lib(graft), exe)
    dc.check_cpp(pkg, gpu_ctx, oracle, exe, tmp_path)


def test_gpu_deblock_rd_tool(graft, pkg, gpu_ctx, oracle, tmp_path):
    dc.check_rd_tool(pkg, oracle, _lib(graft), tmp_path)
