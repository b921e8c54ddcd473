"""The SSIM probes, pfv_encoder's SSIM floors and the frame type they give pfv_encoder_encode_frame on a real MI355X: the shared checks of
tests/ssimprobe_cases.py at the shapes of the emulator twin (tests/test_emu_ssimprobe.py) -- sizes, counts and squared errors exact against the
ladder model, SSIM inside the derived tolerance of numpy's value on the model's reconstructions and EQUAL to the shipped device path."""
import pytest

import ssimprobe_cases as ssp

pytestmark = pytest.mark.gpu

LANES = [1, 2]      # PFV_LANES_PER_MB_8, PFV_LANES_PER_MB_16: k_probe_iframe_ssim has both mappings


@pytest.mark.parametrize("int_transform", [False, True], ids=["f32", "i32"])
@pytest.mark.parametrize("lanes", LANES, ids=["lanes8", "lanes16"])
@pytest.mark.parametrize("w,h,n", ssp.SHAPES)
def test_gpu_ssimprobe_iframe_session(pkg, gpu_ctx, oracle, w, h, n, lanes, int_transform):
    ssp.check_iframe_session_probe(pkg, gpu_ctx, oracle, w, h, n, lane_mapping=lanes, int_transform=int_transform)


@pytest.mark.parametrize("int_transform", [False, True], ids=["f32", "i32"])
@pytest.mark.parametrize("w,h,n", ssp.SHAPES)
def test_gpu_ssimprobe_session(pkg, gpu_ctx, oracle, w, h, n, int_transform):
    ssp.check_session_probe(pkg, gpu_ctx, oracle, w, h, n, int_transform=int_transform)


@pytest.mark.parametrize("w,h,n,lanes,int_transform", ssp.pc.INTERIOR_CASES, ids=ssp.pc.INTERIOR_IDS)
def test_gpu_ssimprobe_iframe_session_interior(pkg, gpu_ctx, oracle, w, h, n, lanes, int_transform):
    ssp.check_iframe_session_probe(pkg, gpu_ctx, oracle, w, h, n, lane_mapping=lanes, int_transform=int_transform)


@pytest.mark.parametrize("w,h,n,int_transform", ssp.pp.INTERIOR_CASES, ids=ssp.pp.INTERIOR_IDS)
def test_gpu_ssimprobe_session_interior(pkg, gpu_ctx, oracle, w, h, n, int_transform):
    ssp.check_session_probe(pkg, gpu_ctx, oracle, w, h, n, int_transform=int_transform)


def test_gpu_ssimprobe_all_eleven_rungs(pkg, gpu_ctx, oracle):
    ssp.check_session_probe(pkg, gpu_ctx, oracle, 50, 38, 3, qualities=ssp.FULL_LADDER, sets=[1, 2, 6])
    ssp.check_iframe_session_probe(pkg, gpu_ctx, oracle, 50, 38, 3, qualities=ssp.FULL_LADDER, sets=[0, 2])


def test_gpu_ssimprobe_agrees_with_rd_probes(pkg, gpu_ctx, oracle):
    ssp.check_agrees_with_rd_probes(pkg, gpu_ctx, oracle)


@pytest.mark.parametrize("w,h,n", [(50, 38, 3), (144, 80, 1), (8, 8, 1)])
def test_gpu_ssimprobe_equals_encoded_ssim(pkg, gpu_ctx, oracle, w, h, n):
    ssp.check_equals_encoded_ssim(pkg, gpu_ctx, oracle, w, h, n)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_gpu_ssimprobe_is_what_the_encoder_writes(pkg, gpu_ctx, oracle, device_entropy):
    ssp.check_probe_is_what_the_encoder_writes(pkg, gpu_ctx, oracle, device_entropy)


def test_gpu_ssimprobe_no_side_effects(pkg, gpu_ctx, oracle):
    ssp.check_no_side_effects(pkg, gpu_ctx, oracle)


def test_gpu_ssimprobe_window_and_stride(pkg, gpu_ctx, oracle):
    ssp.check_window_stride(pkg, gpu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_gpu_ssimprobe_is_what_the_encoder_writes_interior(pkg, gpu_ctx, oracle, device_entropy):
    ssp.check_probe_is_what_the_encoder_writes(pkg, gpu_ctx, oracle, device_entropy, 400, 80)


def test_gpu_ssimprobe_window_and_stride_interior(pkg, gpu_ctx, oracle):
    ssp.check_window_stride(pkg, gpu_ctx, oracle, 400, 80, 3)


def test_gpu_ssimprobe_strip_on_the_right_border(pkg, gpu_ctx, oracle):
    ssp.pp.check_strip_on_the_right_border(pkg, gpu_ctx, oracle, rig_class=ssp.PSsimRig)


def test_gpu_ssimprobe_graph(pkg, gpu_ctx, oracle):
    ssp.check_graph(pkg, gpu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_gpu_ssimprobe_pframe_floor(pkg, gpu_ctx, oracle, device_entropy):
    ssp.check_floor(pkg, gpu_ctx, oracle, device_entropy)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_gpu_ssimprobe_iframe_floor(pkg, gpu_ctx, oracle, device_entropy):
    ssp.check_iframe_floor(pkg, gpu_ctx, oracle, device_entropy)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_gpu_ssimprobe_floor_off_and_one_rung(pkg, gpu_ctx, oracle, device_entropy):
    ssp.check_floor_off_and_one_rung(pkg, gpu_ctx, oracle, device_entropy)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_gpu_ssimprobe_frame_type(pkg, gpu_ctx, oracle, device_entropy):
    ssp.check_frame_type(pkg, gpu_ctx, oracle, device_entropy)


def test_gpu_ssimprobe_arguments(pkg, gpu_ctx, oracle):
    ssp.check_arguments(pkg, gpu_ctx, oracle)


def test_gpu_ssimprobe_cpp_mirror(graft, pkg, gpu_ctx, oracle, tmp_path):
    import os
    lib = graft.build_hip()
    if os.environ.get("PFV_TEST_EMU_AS_GPU") == "1":          # developer dry-run without a GPU (tests/conftest.py)
        import conftest
        lib = conftest.build_emulator()
    exe = str(tmp_path / "ssim_floor")
    ssp.build_cpp(lib, exe)
    ssp.check_cpp(oracle, exe, tmp_path)
