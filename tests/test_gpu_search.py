"""The exhaustive motion search (PFV_SEARCH_FULL: k_pf_search_full + k_pf_transform, pfv_enc_session_ / pfv_encoder_ / pfv_gop_encoder_
set_motion_search) on a real MI355X: the shared checks of tests/search_cases.py at the shapes of the emulator twin
(tests/test_emu_search.py), every one an equality with the numpy restatement of the header's rule."""
import pytest

import search_cases as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("R", sc.RADII)
@pytest.mark.parametrize("w,h", sc.SHAPES)
def test_gpu_search_shapes(pkg, gpu_ctx, w, h, R):
    sc.check_shape(pkg, gpu_ctx, w, h, R)


def test_gpu_search_options(pkg, gpu_ctx):
    sc.check_options(pkg, gpu_ctx)


def test_gpu_search_ties(pkg, gpu_ctx):
    sc.check_ties(pkg, gpu_ctx)


def test_gpu_search_found_where_fourstep_is_lost(pkg, gpu_ctx, oracle):
    sc.check_lost(pkg, gpu_ctx, oracle)


def test_gpu_search_dominance(pkg, gpu_ctx, oracle):
    sc.check_dominance(pkg, gpu_ctx, oracle)


@pytest.mark.parametrize("config", sc.STREAM_CONFIGS)
def test_gpu_search_streams(pkg, gpu_ctx, oracle, config):
    sc.check_stream(pkg, gpu_ctx, oracle, config)


def test_gpu_search_graph(pkg, gpu_ctx):
    sc.check_graph(pkg, gpu_ctx)


def test_gpu_search_off_means_off(pkg, gpu_ctx):
    sc.check_off(pkg, gpu_ctx)


def test_gpu_search_refusals(pkg, gpu_ctx):
    sc.check_refusals(pkg, gpu_ctx)


def _lib(graft):
    import os
    lib = graft.build_hip()
    if os.environ.get("PFV_TEST_EMU_AS_GPU") == "1":          # developer dry-run without a GPU (tests/conftest.py)
        import conftest
        lib = conftest.build_emulator()
    return lib


def test_gpu_search_cpp_mirror(graft, pkg, gpu_ctx, tmp_path):
    exe = str(tmp_path / "search_report")
    sc.build_cpp(_lib(graft), exe)
    sc.check_cpp(pkg, gpu_ctx, exe, tmp_path)


def test_gpu_search_rd_tool(graft, pkg, gpu_ctx, tmp_path):
    sc.check_rd_tool(pkg, _lib(graft), tmp_path)
    sc.check_time_tool(_lib(graft))


@pytest.mark.parametrize("R", sc.SWEEP_RADII)
def test_gpu_search_sweep(pkg, gpu_ctx, R):
    sc.check_sweep(pkg, gpu_ctx, R)


def test_gpu_search_ladder_session(pkg, gpu_ctx, oracle):
    sc.check_ladder_session(pkg, gpu_ctx, oracle, "full", sc.LADDER_R, sc.full_ladder_model)


@pytest.mark.parametrize("device_entropy", [False, True])
def test_gpu_search_ladder_encoder(pkg, gpu_ctx, oracle, device_entropy):
    sc.check_ladder_encoder(pkg, gpu_ctx, oracle, "full", sc.LADDER_R, sc.full_ladder_model, device_entropy)


@pytest.mark.parametrize("transform", [0, 1])
@pytest.mark.parametrize("name", list(sc.GROUP_SETS))
def test_gpu_search_groups(pkg, gpu_ctx, name, transform):
    sc.check_groups(pkg, gpu_ctx, name, transform)


def test_gpu_search_largest(pkg, gpu_ctx):
    sc.check_largest(pkg, gpu_ctx)
