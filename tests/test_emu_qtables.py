"""CPU emulator twins of tests/test_gpu_qtables.py (tests/qtable_cases.py) at small sizes: any q-table set (0, 1, 4, 7 hostile, 256 and
300 tables) and any per-plane index through the stream decoders, and the decoder session's entry points on hostile tables and
coefficients whose dequantised products wrap i32 -- the same kernel sources compiled for the CPU (tests/hipemu)."""
import pytest

import qtable_cases as qc


@pytest.fixture(params=["lanes8", "lanes16"])
def forced_lanes(request, pkg, emu_ctx):
    """kernel-level tests run under both lane mappings of the codec kernels (pfv_kernels.hip, "Lane mappings"); the session reads the
    option when it is created"""
    L = pkg._lib
    emu_ctx.set_option(L.PFV_OPT_LANE_MAPPING, L.PFV_LANES_PER_MB_8 if request.param == "lanes8" else L.PFV_LANES_PER_MB_16)
    yield request.param
    emu_ctx.set_option(L.PFV_OPT_LANE_MAPPING, L.PFV_LANES_AUTO)


DECODERS = (("host", 0), ("device", None), ("auto", 0))       # the emulator runs a subset of the GPU test's entropy / look-ahead grid


@pytest.mark.parametrize("name,w,h,pattern", [("one", 64, 48, "IPPDIP"), ("perm4", 100, 60, "IPPIPP"), ("hostile7", 34, 18, "IPDPPIP"),
                                              ("t256", 64, 48, "IPIP"), ("t300", 64, 48, "IPPI")])
def test_emu_qtables_stream_sets(pkg, emu_ctx, oracle, name, w, h, pattern):
    kinds = qc.check_stream_case(pkg, emu_ctx, oracle, w, h, name, pattern, hostile_every=4 if name == "hostile7" else 0,
                                 decoders=DECODERS, gop_shapes=((3, 4), (2, 2)))
    assert kinds.count("frame") == sum(c != "D" for c in pattern) and kinds[-1] == "eof"


def test_emu_qtables_stream_above_auto_threshold(pkg, emu_ctx, oracle):
    """640 x 360, hostile coefficients in every other macroblock: payloads above the 64 KiB from which `auto` reads on the device"""
    sizes = qc.check_stream_case(pkg, emu_ctx, oracle, 640, 360, "hostile7", "IPPIP", seed=7, hostile_every=2, return_sizes=True,
                                 decoders=(("auto", 0), ("host", None)), gop_shapes=((2, 2),))
    print("payload bytes:", sizes)
    assert min(sizes) > 64 << 10


def test_emu_qtables_zero_tables(pkg, emu_ctx, oracle):
    qc.check_zero_tables(pkg, emu_ctx, oracle, decoders=DECODERS, gop_shapes=((2, 2),))


def test_emu_qtables_out_of_range_index(pkg, emu_ctx, oracle):
    qc.check_out_of_range_index(pkg, emu_ctx, oracle, decoders=DECODERS, gop_shapes=((2, 2),))


def test_emu_qtables_gop_variation(pkg, emu_ctx, oracle):
    assert qc.check_gop_variation(pkg, emu_ctx, oracle, 64, 48, gop_shapes=((4, 4), (3, 4), (2, 2))) == 17


def test_emu_qtables_batch_decoder(pkg, emu_ctx, oracle):
    qc.check_batch_decoder_qidx(pkg, emu_ctx, oracle, 48, 32, n_streams=2)


@pytest.mark.parametrize("w,h,n_streams,n_tables", [(64, 48, 3, 5), (100, 60, 2, 9)])
def test_emu_qtables_session_hostile(pkg, emu_ctx, oracle, forced_lanes, w, h, n_streams, n_tables):
    r = qc.check_session_hostile(pkg, emu_ctx, oracle, w, h, n_streams, n_tables, seed=w + n_tables)
    print("measured:", r)
    assert r["frames"] == 9 * n_streams + 2 * (n_streams - 1) and r["c1_min"] >= 0.25 and r["c2_min"] >= 0.5


def test_emu_qtables_session_moderate_tables(pkg, emu_ctx, oracle, forced_lanes):
    """tables in [200, 2000): most products stay inside i32, the wrapping classes still wrap"""
    r = qc.check_session_hostile(pkg, emu_ctx, oracle, 34, 18, 2, 6, seed=3, table_range=(200, 1999))
    print("measured:", r)
    assert r["c1_min"] >= 0.25


def test_emu_qtables_plane_ops_zero_entries(pkg, emu_ctx, oracle, forced_lanes):
    assert qc.check_plane_ops_zero_entries(pkg, emu_ctx, oracle) == 6
