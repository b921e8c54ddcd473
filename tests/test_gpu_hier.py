"""The wide-range hierarchical motion search (PFV_SEARCH_HIER: k_halve + k_pf_search_coarse + k_pf_refine + k_pf_transform,
pfv_*_set_motion_search, pfv_enc_session_coarse_vectors) on a real MI355X: the shared checks of tests/hier_cases.py at the shapes of
the emulator twin (tests/test_emu_hier.py), every one an equality with the numpy restatement of the header's rule."""
import pytest

import hier_cases as hc
import search_cases as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("R", hc.RADII)
@pytest.mark.parametrize("w,h", hc.SHAPES)
def test_gpu_hier_shapes(pkg, gpu_ctx, w, h, R):
    hc.check_shape(pkg, gpu_ctx, w, h, R)


def test_gpu_hier_coarse_edges(pkg, gpu_ctx):
    hc.check_coarse_edges(pkg, gpu_ctx)


def test_gpu_hier_ties(pkg, gpu_ctx):
    hc.check_ties(pkg, gpu_ctx)


def test_gpu_hier_limits(pkg, gpu_ctx):
    hc.check_limits(pkg, gpu_ctx)


def test_gpu_hier_reach(pkg, gpu_ctx):
    hc.check_reach(pkg, gpu_ctx)


@pytest.mark.parametrize("config", hc.STREAM_CONFIGS)
def test_gpu_hier_streams(pkg, gpu_ctx, oracle, config):
    hc.check_stream(pkg, gpu_ctx, oracle, config)


def test_gpu_hier_graph(pkg, gpu_ctx):
    hc.check_graph(pkg, gpu_ctx)


def test_gpu_hier_off_means_off(pkg, gpu_ctx):
    hc.check_off(pkg, gpu_ctx)


def test_gpu_hier_refusals(pkg, gpu_ctx):
    hc.check_refusals(pkg, gpu_ctx)


def _lib(graft):
    import os
    lib = graft.build_hip()
    if os.environ.get("PFV_TEST_EMU_AS_GPU") == "1":          # developer dry-run without a GPU (tests/conftest.py)
        import conftest
        lib = conftest.build_emulator()
    return lib


def test_gpu_hier_cpp_mirror(graft, pkg, gpu_ctx, tmp_path):
    exe = str(tmp_path / "hier_report")
    hc.build_cpp(_lib(graft), exe)
    hc.check_cpp(pkg, gpu_ctx, exe, tmp_path)


def test_gpu_hier_rd_tool(graft, pkg, gpu_ctx):
    hc.check_rd_tool(_lib(graft))
    hc.check_time_tool(_lib(graft))


@pytest.mark.parametrize("R", hc.SWEEP_RADII)
def test_gpu_hier_sweep(pkg, gpu_ctx, R):
    hc.check_sweep(pkg, gpu_ctx, R)


def test_gpu_hier_ladder_session(pkg, gpu_ctx, oracle):
    sc.check_ladder_session(pkg, gpu_ctx, oracle, "hier", hc.LADDER_R, hc.hier_ladder_model)


@pytest.mark.parametrize("device_entropy", [False, True])
def test_gpu_hier_ladder_encoder(pkg, gpu_ctx, oracle, device_entropy):
    sc.check_ladder_encoder(pkg, gpu_ctx, oracle, "hier", hc.LADDER_R, hc.hier_ladder_model, device_entropy)


@pytest.mark.parametrize("device_entropy", [False, True])
def test_gpu_hier_rate_rungs(pkg, gpu_ctx, oracle, device_entropy):
    hc.check_rate_rungs(pkg, gpu_ctx, oracle, device_entropy)


def test_gpu_hier_largest(pkg, gpu_ctx):
    hc.check_largest(pkg, gpu_ctx)


def test_gpu_hier_field_edge(pkg, gpu_ctx):
    hc.check_field_edge(pkg, gpu_ctx)
