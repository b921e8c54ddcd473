"""The SSIM probes, pfv_encoder's SSIM floors and the frame type they give pfv_encoder_encode_frame on the CPU emulator build of the kernel
sources: the shared checks of tests/ssimprobe_cases.py -- sizes, counts and squared errors exact against the ladder model, SSIM inside the
derived tolerance of numpy's value on the model's reconstructions and EQUAL to the shipped device path.  The GPU twin is
tests/test_gpu_ssimprobe.py."""
import pytest

import ssimprobe_cases as ssp

LANES = [1, 2]      # PFV_LANES_PER_MB_8, PFV_LANES_PER_MB_16: k_probe_iframe_ssim has both mappings


def test_emu_ssimprobe_inputs_cover(oracle):
    ssp.check_inputs_cover(oracle)


@pytest.mark.parametrize("int_transform", [False, True], ids=["f32", "i32"])
@pytest.mark.parametrize("lanes", LANES, ids=["lanes8", "lanes16"])
@pytest.mark.parametrize("w,h,n", ssp.SHAPES)
def test_emu_ssimprobe_iframe_session(pkg, emu_ctx, oracle, w, h, n, lanes, int_transform):
    ssp.check_iframe_session_probe(pkg, emu_ctx, oracle, w, h, n, lane_mapping=lanes, int_transform=int_transform)


@pytest.mark.parametrize("int_transform", [False, True], ids=["f32", "i32"])
@pytest.mark.parametrize("w,h,n", ssp.SHAPES)
def test_emu_ssimprobe_session(pkg, emu_ctx, oracle, w, h, n, int_transform):
    ssp.check_session_probe(pkg, emu_ctx, oracle, w, h, n, int_transform=int_transform)


@pytest.mark.parametrize("w,h,n,lanes,int_transform", ssp.pc.INTERIOR_CASES, ids=ssp.pc.INTERIOR_IDS)
def test_emu_ssimprobe_iframe_session_interior(pkg, emu_ctx, oracle, w, h, n, lanes, int_transform):
    ssp.check_iframe_session_probe(pkg, emu_ctx, oracle, w, h, n, lane_mapping=lanes, int_transform=int_transform)


@pytest.mark.parametrize("w,h,n,int_transform", ssp.pp.INTERIOR_CASES, ids=ssp.pp.INTERIOR_IDS)
def test_emu_ssimprobe_session_interior(pkg, emu_ctx, oracle, w, h, n, int_transform):
    ssp.check_session_probe(pkg, emu_ctx, oracle, w, h, n, int_transform=int_transform)


def test_emu_ssimprobe_all_eleven_rungs(pkg, emu_ctx, oracle):
    ssp.check_session_probe(pkg, emu_ctx, oracle, 50, 38, 3, qualities=ssp.FULL_LADDER, sets=[1, 2, 6])
    ssp.check_iframe_session_probe(pkg, emu_ctx, oracle, 50, 38, 3, qualities=ssp.FULL_LADDER, sets=[0, 2])


def test_emu_ssimprobe_agrees_with_rd_probes(pkg, emu_ctx, oracle):
    ssp.check_agrees_with_rd_probes(pkg, emu_ctx, oracle)


@pytest.mark.parametrize("w,h,n", [(50, 38, 3), (144, 80, 1), (8, 8, 1)])
def test_emu_ssimprobe_equals_encoded_ssim(pkg, emu_ctx, oracle, w, h, n):
    ssp.check_equals_encoded_ssim(pkg, emu_ctx, oracle, w, h, n)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_emu_ssimprobe_is_what_the_encoder_writes(pkg, emu_ctx, oracle, device_entropy):
    ssp.check_probe_is_what_the_encoder_writes(pkg, emu_ctx, oracle, device_entropy)


def test_emu_ssimprobe_no_side_effects(pkg, emu_ctx, oracle):
    ssp.check_no_side_effects(pkg, emu_ctx, oracle)


def test_emu_ssimprobe_window_and_stride(pkg, emu_ctx, oracle):
    ssp.check_window_stride(pkg, emu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_emu_ssimprobe_is_what_the_encoder_writes_interior(pkg, emu_ctx, oracle, device_entropy):
    ssp.check_probe_is_what_the_encoder_writes(pkg, emu_ctx, oracle, device_entropy, 400, 80)


def test_emu_ssimprobe_window_and_stride_interior(pkg, emu_ctx, oracle):
    ssp.check_window_stride(pkg, emu_ctx, oracle, 400, 80, 3)


def test_emu_ssimprobe_strip_on_the_right_border(pkg, emu_ctx, oracle):
    ssp.pp.check_strip_on_the_right_border(pkg, emu_ctx, oracle, rig_class=ssp.PSsimRig)


def test_emu_ssimprobe_graph(pkg, emu_ctx, oracle):
    ssp.check_graph(pkg, emu_ctx, oracle)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_emu_ssimprobe_pframe_floor(pkg, emu_ctx, oracle, device_entropy):
    ssp.check_floor(pkg, emu_ctx, oracle, device_entropy)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_emu_ssimprobe_iframe_floor(pkg, emu_ctx, oracle, device_entropy):
    ssp.check_iframe_floor(pkg, emu_ctx, oracle, device_entropy)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_emu_ssimprobe_floor_off_and_one_rung(pkg, emu_ctx, oracle, device_entropy):
    ssp.check_floor_off_and_one_rung(pkg, emu_ctx, oracle, device_entropy)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device_entropy", "host_entropy"])
def test_emu_ssimprobe_frame_type(pkg, emu_ctx, oracle, device_entropy):
    ssp.check_frame_type(pkg, emu_ctx, oracle, device_entropy)


def test_emu_ssimprobe_arguments(pkg, emu_ctx, oracle):
    ssp.check_arguments(pkg, emu_ctx, oracle)


def test_emu_ssimprobe_poisoned_encoder(tmp_path):
    """emulator only: the failure that poisons an encoder comes from a seam in the emulator build (tests/cpp/poison_seam.h)"""
    exe = str(tmp_path / "ssim_floor_seam")
    ssp.build_poison(exe)
    ssp.check_poisoned(exe, tmp_path)


def test_emu_ssimprobe_cpp_mirror(pkg, emu_ctx, oracle, tmp_path):
    import conftest
    exe = str(tmp_path / "ssim_floor_emu")
    ssp.build_cpp(conftest.build_emulator(), exe)
    ssp.check_cpp(oracle, exe, tmp_path)
