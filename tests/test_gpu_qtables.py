"""Any q-table set and any per-plane q-table index on a real MI355X (tests/qtable_cases.py): streams written from parts through Decoder,
GopDecoder and BatchDecoder against the oracle's stream decoder call by call, and the decoder session's every entry point on hostile
tables and coefficients whose dequantised products wrap i32, against the oracle's decoder frame by frame."""
import pytest

import qtable_cases as qc

pytestmark = pytest.mark.gpu

GEOMS = [(64, 48), (100, 60), (34, 18)]          # whole strips / chroma not a multiple of 16 / one chroma macroblock row


@pytest.fixture(params=["lanes8", "lanes16"])
def forced_lanes(request, pkg, gpu_ctx):
    """both lane mappings of the codec kernels (pfv_kernels.hip, "Lane mappings"), forced; sessions read the option when they are created"""
    L = pkg._lib
    gpu_ctx.set_option(L.PFV_OPT_LANE_MAPPING, L.PFV_LANES_PER_MB_8 if request.param == "lanes8" else L.PFV_LANES_PER_MB_16)
    yield request.param
    gpu_ctx.set_option(L.PFV_OPT_LANE_MAPPING, L.PFV_LANES_AUTO)


@pytest.mark.parametrize("w,h", GEOMS)
@pytest.mark.parametrize("name,pattern", [("one", "IPPDIPP"), ("perm4", "IPPIPPP"), ("hostile7", "IPDPPIPP"), ("t256", "IPIPP"),
                                          ("t300", "IPPIP")])
def test_gpu_qtables_stream_sets(pkg, gpu_ctx, oracle, name, pattern, w, h):
    """every decoder object: Decoder with entropy host / device / auto and look-ahead 0 / default, GopDecoder host / device with batch
    shapes (4,4), (3,4), (2,2), (8,15)"""
    kinds = qc.check_stream_case(pkg, gpu_ctx, oracle, w, h, name, pattern, seed=w + h, hostile_every=4 if name == "hostile7" else 0)
    assert kinds.count("frame") == sum(c != "D" for c in pattern) and kinds[-1] == "eof"


def test_gpu_qtables_stream_above_auto_threshold(pkg, gpu_ctx, oracle):
    """640 x 360 with hostile coefficients in every other macroblock: every payload exceeds the 64 KiB from which `auto` reads the run
    streams on the device"""
    sizes = qc.check_stream_case(pkg, gpu_ctx, oracle, 640, 360, "hostile7", "IPPIP", seed=7, hostile_every=2, return_sizes=True)
    print("payload bytes:", sizes)
    assert min(sizes) > 64 << 10


def test_gpu_qtables_zero_tables(pkg, gpu_ctx, oracle):
    qc.check_zero_tables(pkg, gpu_ctx, oracle)


def test_gpu_qtables_out_of_range_index(pkg, gpu_ctx, oracle):
    qc.check_out_of_range_index(pkg, gpu_ctx, oracle)


@pytest.mark.parametrize("w,h", [(100, 60), (640, 360)])
def test_gpu_qtables_gop_variation(pkg, gpu_ctx, oracle, w, h):
    assert qc.check_gop_variation(pkg, gpu_ctx, oracle, w, h) == 17


@pytest.mark.parametrize("w,h", [(100, 60), (34, 18)])
def test_gpu_qtables_batch_decoder(pkg, gpu_ctx, oracle, w, h):
    qc.check_batch_decoder_qidx(pkg, gpu_ctx, oracle, w, h, n_streams=3)


@pytest.mark.parametrize("w,h,n_streams,n_tables", [(64, 48, 3, 5), (100, 60, 2, 9), (34, 18, 3, 7), (272, 144, 2, 6)])
def test_gpu_qtables_session_hostile(pkg, gpu_ctx, oracle, forced_lanes, w, h, n_streams, n_tables):
    r = qc.check_session_hostile(pkg, gpu_ctx, oracle, w, h, n_streams, n_tables, seed=w + n_tables)
    print("measured:", r)
    assert r["frames"] == 9 * n_streams + 2 * (n_streams - 1) and r["c1_min"] >= 0.25 and r["c2_min"] >= 0.5


def test_gpu_qtables_session_moderate_tables(pkg, gpu_ctx, oracle, forced_lanes):
    """tables in [200, 2000): most products stay inside i32, the wrapping classes still wrap"""
    r = qc.check_session_hostile(pkg, gpu_ctx, oracle, 100, 60, 2, 6, seed=3, table_range=(200, 1999))
    print("measured:", r)
    assert r["c1_min"] >= 0.25


def test_gpu_qtables_session_auto_lanes_1080p(pkg, gpu_ctx, oracle):
    """the automatic lane mapping at 1080p x 3 streams = 4 590 strips (>= 4 096: the 8-lane mapping is the automatic one for the full
    window; the windowed frames fall below and take the 16-lane one)"""
    L = pkg._lib
    assert gpu_ctx.get_option(L.PFV_OPT_LANE_MAPPING) == L.PFV_LANES_AUTO
    r = qc.check_session_hostile(pkg, gpu_ctx, oracle, 1920, 1080, 3, 6, seed=1080)
    print("measured:", r)
    assert r["frames"] == 9 * 3 + 2 * 2 and r["c1_min"] >= 0.25 and r["c2_min"] >= 0.5


def test_gpu_qtables_plane_ops_zero_entries(pkg, gpu_ctx, oracle, forced_lanes):
    assert qc.check_plane_ops_zero_entries(pkg, gpu_ctx, oracle, sizes=((48, 32), (100, 60), (640, 360))) == 9
