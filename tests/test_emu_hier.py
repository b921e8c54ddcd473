"""The wide-range hierarchical motion search (PFV_SEARCH_HIER: k_halve + k_pf_search_coarse + k_pf_refine + k_pf_transform,
pfv_*_set_motion_search, pfv_enc_session_coarse_vectors) on the CPU emulator build of the kernel sources: the shared checks of
tests/hier_cases.py, every one an equality with the numpy restatement of the header's rule.  The GPU twin is tests/test_gpu_hier.py."""
import pytest

import hier_cases as hc
import search_cases as sc


@pytest.mark.parametrize("R", hc.RADII)
@pytest.mark.parametrize("w,h", hc.SHAPES)
def test_emu_hier_shapes(pkg, emu_ctx, w, h, R):
    hc.check_shape(pkg, emu_ctx, w, h, R)


def test_emu_hier_coarse_edges(pkg, emu_ctx):
    hc.check_coarse_edges(pkg, emu_ctx)


def test_emu_hier_ties(pkg, emu_ctx):
    hc.check_ties(pkg, emu_ctx)


def test_emu_hier_limits(pkg, emu_ctx):
    hc.check_limits(pkg, emu_ctx)


def test_emu_hier_reach(pkg, emu_ctx):
    hc.check_reach(pkg, emu_ctx)


@pytest.mark.parametrize("config", hc.STREAM_CONFIGS)
def test_emu_hier_streams(pkg, emu_ctx, oracle, config):
    hc.check_stream(pkg, emu_ctx, oracle, config)


def test_emu_hier_graph(pkg, emu_ctx):
    hc.check_graph(pkg, emu_ctx)


def test_emu_hier_off_means_off(pkg, emu_ctx):
    hc.check_off(pkg, emu_ctx)


def test_emu_hier_refusals(pkg, emu_ctx):
    hc.check_refusals(pkg, emu_ctx)


def test_emu_hier_cpp_mirror(pkg, emu_ctx, tmp_path):
    import conftest
    exe = str(tmp_path / "hier_report_emu")
    hc.build_cpp(conftest.build_emulator(), exe)
    hc.check_cpp(pkg, emu_ctx, exe, tmp_path)


def test_emu_hier_rd_tool(pkg, emu_ctx):
    import conftest
    hc.check_rd_tool(conftest.build_emulator())
    hc.check_time_tool(conftest.build_emulator())


@pytest.mark.parametrize("R", hc.SWEEP_RADII)
def test_emu_hier_sweep(pkg, emu_ctx, R):
    hc.check_sweep(pkg, emu_ctx, R)


def test_emu_hier_ladder_session(pkg, emu_ctx, oracle):
    sc.check_ladder_session(pkg, emu_ctx, oracle, "hier", hc.LADDER_R, hc.hier_ladder_model)


@pytest.mark.parametrize("device_entropy", [False, True])
def test_emu_hier_ladder_encoder(pkg, emu_ctx, oracle, device_entropy):
    sc.check_ladder_encoder(pkg, emu_ctx, oracle, "hier", hc.LADDER_R, hc.hier_ladder_model, device_entropy)


@pytest.mark.parametrize("device_entropy", [False, True])
def test_emu_hier_rate_rungs(pkg, emu_ctx, oracle, device_entropy):
    hc.check_rate_rungs(pkg, emu_ctx, oracle, device_entropy)


def test_emu_hier_largest(pkg, emu_ctx):
    hc.check_largest(pkg, emu_ctx)


def test_emu_hier_field_edge(pkg, emu_ctx):
    hc.check_field_edge(pkg, emu_ctx)
