"""Out-of-loop deblocking (pfv_frames_deblock*, pfv_deblock_strength, pfv_dec_set_deblock, pfv_decoder_set_deblock, tools/rd_curve.py
--deblock) on the CPU emulator build of the kernel sources: the shared checks of tests/deblock_cases.py, every one an equality with the
numpy restatement of the header's text.  The GPU twin is tests/test_gpu_deblock.py."""
import pytest

import deblock_cases as dc


@pytest.mark.parametrize("w,h", dc.SHAPES)
def test_emu_deblock_shapes(pkg, emu_ctx, w, h):
    dc.check_shape(pkg, emu_ctx, w, h)


def test_emu_deblock_traps(pkg, emu_ctx):
    dc.check_traps(pkg, emu_ctx)


def test_emu_deblock_properties(pkg, emu_ctx):
    dc.check_properties(pkg, emu_ctx)


@pytest.mark.parametrize("w,h,px,py", [(144, 48, 16, 5), (144, 48, 128, 5), (144, 48, 5, 16), (50, 38, 49, 37)])
def test_emu_deblock_locality(pkg, emu_ctx, w, h, px, py):
    assert dc.check_locality(pkg, emu_ctx, w, h, px, py) >= 1


def test_emu_deblock_bad_arguments(pkg, emu_ctx):
    dc.check_bad_arguments(pkg, emu_ctx)


def test_emu_deblock_strength(pkg, emu_ctx):
    dc.check_strength(pkg)


@pytest.mark.parametrize("path", ["get_frame", "output", "strided"])
def test_emu_deblock_dec_session(pkg, emu_ctx, oracle, path):
    dc.check_dec_session(pkg, emu_ctx, oracle, path)


def test_emu_deblock_dec_session_graph(pkg, emu_ctx, oracle):
    dc.check_dec_graph(pkg, emu_ctx, oracle)


@pytest.mark.parametrize("device_out", [False, True], ids=["host_out", "device_out"])
@pytest.mark.parametrize("entropy", ["device", "host"])
def test_emu_deblock_decoder(pkg, emu_ctx, oracle, entropy, device_out):
    dc.check_decoder(pkg, emu_ctx, oracle, entropy, device_out)


@pytest.mark.parametrize("quality", [0, 2, 5, 10])
def test_emu_deblock_effect(pkg, emu_ctx, oracle, quality):
    dc.check_effect(pkg, emu_ctx, oracle, quality)


def test_emu_deblock_cpp_mirror(pkg, emu_ctx, oracle, tmp_path):
    import conftest
    exe = str(tmp_path / "deblock_report_emu")
    dc.build_cpp(conftest.build_emulator(), exe)
    dc.check_cpp(pkg, emu_ctx, oracle, exe, tmp_path)


def test_emu_deblock_rd_tool(pkg, emu_ctx, oracle, tmp_path):
    import conftest
    dc.check_rd_tool(pkg, oracle, conftest.build_emulator(), tmp_path)
