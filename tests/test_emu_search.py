"""The exhaustive motion search (PFV_SEARCH_FULL: k_pf_search_full + k_pf_transform, pfv_enc_session_ / pfv_encoder_ / pfv_gop_encoder_
set_motion_search, tools/rd_curve.py --search) on the CPU emulator build of the kernel sources: the shared checks of tests/search_cases.py,
every one an equality with the numpy restatement of the header's rule.  The GPU twin is tests/test_gpu_search.py."""
import pytest

import search_cases as sc


@pytest.mark.parametrize("R", sc.RADII)
@pytest.mark.parametrize("w,h", sc.SHAPES)
def test_emu_search_shapes(pkg, emu_ctx, w, h, R):
    sc.check_shape(pkg, emu_ctx, w, h, R)


def test_emu_search_options(pkg, emu_ctx):
    sc.check_options(pkg, emu_ctx)


def test_emu_search_ties(pkg, emu_ctx):
    sc.check_ties(pkg, emu_ctx)


def test_emu_search_found_where_fourstep_is_lost(pkg, emu_ctx, oracle):
    sc.check_lost(pkg, emu_ctx, oracle)


def test_emu_search_dominance(pkg, emu_ctx, oracle):
    sc.check_dominance(pkg, emu_ctx, oracle)


@pytest.mark.parametrize("config", sc.STREAM_CONFIGS)
def test_emu_search_streams(pkg, emu_ctx, oracle, config):
    sc.check_stream(pkg, emu_ctx, oracle, config)


def test_emu_search_graph(pkg, emu_ctx):
    sc.check_graph(pkg, emu_ctx)


def test_emu_search_off_means_off(pkg, emu_ctx):
    sc.check_off(pkg, emu_ctx)


def test_emu_search_refusals(pkg, emu_ctx):
    sc.check_refusals(pkg, emu_ctx)


def test_emu_search_cpp_mirror(pkg, emu_ctx, tmp_path):
    import conftest
    exe = str(tmp_path / "search_report_emu")
    sc.build_cpp(conftest.build_emulator(), exe)
    sc.check_cpp(pkg, emu_ctx, exe, tmp_path)


def test_emu_search_rd_tool(pkg, emu_ctx, tmp_path):
    import conftest
    sc.check_rd_tool(pkg, conftest.build_emulator(), tmp_path)
    sc.check_time_tool(conftest.build_emulator())


@pytest.mark.parametrize("R", sc.SWEEP_RADII)
def test_emu_search_sweep(pkg, emu_ctx, R):
    sc.check_sweep(pkg, emu_ctx, R)


def test_emu_search_ladder_session(pkg, emu_ctx, oracle):
    sc.check_ladder_session(pkg, emu_ctx, oracle, "full", sc.LADDER_R, sc.full_ladder_model)


@pytest.mark.parametrize("device_entropy", [False, True])
def test_emu_search_ladder_encoder(pkg, emu_ctx, oracle, device_entropy):
    sc.check_ladder_encoder(pkg, emu_ctx, oracle, "full", sc.LADDER_R, sc.full_ladder_model, device_entropy)


@pytest.mark.parametrize("transform", [0, 1])
@pytest.mark.parametrize("name", list(sc.GROUP_SETS))
def test_emu_search_groups(pkg, emu_ctx, name, transform):
    sc.check_groups(pkg, emu_ctx, name, transform)


def test_emu_search_largest(pkg, emu_ctx):
    sc.check_largest(pkg, emu_ctx)
