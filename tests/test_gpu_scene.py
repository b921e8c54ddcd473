"""Scene-cut detection (pfv_scene_detector_*, pfv_frames_scene, pfv_scene_score_q8, pfv_scene_plan, pfv_encoder_set_scene_cut) on a real
MI355X: the shared checks of tests/scene_cases.py at the shapes of the emulator twin (tests/test_emu_scene.py), every numeric one an equality
with the numpy restatement of the header's text."""
import pytest

import scene_cases as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("w,h", sc.SHAPES)
def test_gpu_scene_shapes(pkg, gpu_ctx, w, h):
    sc.check_shape(pkg, gpu_ctx, w, h)


@pytest.mark.parametrize("radius", sc.RADII)
def test_gpu_scene_radii(pkg, gpu_ctx, radius):
    sc.check_radius(pkg, gpu_ctx, radius)


def test_gpu_scene_traps(pkg, gpu_ctx):
    sc.check_traps(pkg, gpu_ctx)


@pytest.mark.parametrize("w,h,qx,qy,least", [(144, 80, 8, 5, 2), (144, 80, 9, 9, 4), (144, 80, 35, 19, 0), (322, 194, 40, 24, 2)])
def test_gpu_scene_locality(pkg, gpu_ctx, w, h, qx, qy, least):
    assert sc.check_locality(pkg, gpu_ctx, w, h, qx, qy) >= least


def test_gpu_scene_state(pkg, gpu_ctx):
    sc.check_state(pkg, gpu_ctx)


def test_gpu_scene_graph(pkg, gpu_ctx):
    sc.check_graph(pkg, gpu_ctx)


def test_gpu_scene_bad_arguments(pkg, gpu_ctx):
    sc.check_bad_arguments(pkg, gpu_ctx)


def test_gpu_scene_decision(pkg, gpu_ctx):
    sc.check_decision(pkg, gpu_ctx)


def test_gpu_scene_plan(pkg, gpu_ctx):
    sc.check_plan(pkg)


@pytest.mark.parametrize("config", list(sc.ENCODER_CONFIGS))
def test_gpu_scene_encoder(pkg, gpu_ctx, config):
    sc.check_encoder(pkg, gpu_ctx, config)


def test_gpu_scene_encoder_switch(pkg, gpu_ctx):
    sc.check_encoder_switch(pkg, gpu_ctx)


def _lib(graft):
    import os
    lib = graft.build_hip()
    if os.environ.get("PFV_TEST_EMU_AS_GPU") == "1":          # developer dry-run without a GPU (tests/conftest.py)
        import conftest
        lib = conftest.build_emulator()
    return lib


def test_gpu_scene_cpp_mirror(graft, pkg, gpu_ctx, tmp_path):
    exe = str(tmp_path / "scene_report")
    sc.build_cpp(_lib(graft), exe)
    sc.check_cpp(pkg, gpu_ctx, exe, tmp_path)


def test_gpu_scene_rd_tool(graft, pkg, gpu_ctx):
    sc.check_rd_tool(pkg, _lib(graft))
