"""Scene-cut detection (pfv_scene_detector_*, pfv_frames_scene, pfv_scene_score_q8, pfv_scene_plan, pfv_encoder_set_scene_cut,
tools/rd_curve.py --scene-cut) on the CPU emulator build of the kernel sources: the shared checks of tests/scene_cases.py, every numeric one an
equality with the numpy restatement of the header's text.  The GPU twin is tests/test_gpu_scene.py."""
import pytest

import scene_cases as sc


@pytest.mark.parametrize("w,h", sc.SHAPES)
def test_emu_scene_shapes(pkg, emu_ctx, w, h):
    sc.check_shape(pkg, emu_ctx, w, h)


@pytest.mark.parametrize("radius", sc.RADII)
def test_emu_scene_radii(pkg, emu_ctx, radius):
    sc.check_radius(pkg, emu_ctx, radius)


def test_emu_scene_traps(pkg, emu_ctx):
    sc.check_traps(pkg, emu_ctx)


@pytest.mark.parametrize("w,h,qx,qy,least", [(144, 80, 8, 5, 2), (144, 80, 9, 9, 4), (144, 80, 35, 19, 0), (322, 194, 40, 24, 2)])
def test_emu_scene_locality(pkg, emu_ctx, w, h, qx, qy, least):
    assert sc.check_locality(pkg, emu_ctx, w, h, qx, qy) >= least


def test_emu_scene_state(pkg, emu_ctx):
    sc.check_state(pkg, emu_ctx)


def test_emu_scene_graph(pkg, emu_ctx):
    sc.check_graph(pkg, emu_ctx)


def test_emu_scene_bad_arguments(pkg, emu_ctx):
    sc.check_bad_arguments(pkg, emu_ctx)


def test_emu_scene_decision(pkg, emu_ctx):
    sc.check_decision(pkg, emu_ctx)


def test_emu_scene_plan(pkg, emu_ctx):
    sc.check_plan(pkg)


@pytest.mark.parametrize("config", list(sc.ENCODER_CONFIGS))
def test_emu_scene_encoder(pkg, emu_ctx, config):
    sc.check_encoder(pkg, emu_ctx, config)


def test_emu_scene_encoder_switch(pkg, emu_ctx):
    sc.check_encoder_switch(pkg, emu_ctx)


def test_emu_scene_cpp_mirror(pkg, emu_ctx, tmp_path):
    import conftest
    exe = str(tmp_path / "scene_report_emu")
    sc.build_cpp(conftest.build_emulator(), exe)
    sc.check_cpp(pkg, emu_ctx, exe, tmp_path)


def test_emu_scene_rd_tool(pkg, emu_ctx):
    import conftest
    sc.check_rd_tool(pkg, conftest.build_emulator())
    sc.check_time_tool(pkg, conftest.build_emulator())
