#!/usr/bin/env python3
"""Generates tests/golden/entropy_vectors.npz: known-answer vectors of the entropy layer (rle_create_huffman, the Huffman tree
and codes, RLE, the i- and p-frame payloads) aimed at the rules tests/test_mutation_sensitivity.py flips: ties in the table,
equal frequencies at insertion, one-symbol and full trees, the i32 wrap of x * 255 (rows of the worked table in
oracle/ENTROPY_WIDTHS.md), zero runs of exactly 15 / 16 / 30, all-zero macroblocks, the last coefficient alone, +-16383, -1, and
p-frames with mixed has_coef / motion vectors.

The outputs come from the numpy restatement (oracle/pfv_oracle_entropy_np.py) and are cross-checked with the C oracle before
the file is written.  python tests/golden/make_entropy_vectors.py"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import entropy_recompute as er        # noqa: E402
from oracle_bind import Oracle        # noqa: E402


def crafted_histograms():
    """(name, 16 bins) -- every row of the worked i32 table, ties at every position, one symbol, all sixteen, holes, extremes"""
    rows = []

    def add(name, bins):
        h = np.zeros(16, np.int64)
        for k, x in bins.items():
            h[k] = x
        assert h.max() <= 2**31 - 1
        rows.append((name, h.astype(np.int32)))

    # rows of the worked table (x = bin 0; a few small bins around it so that the tree has something to sort)
    for x in (8421504, 8421505, 12311503, 20000000):
        add(f"wrap_{x}", {0: x, 1: 3_000_000, 3: 500_000, 15: 40_000})
    add("wrap_17M_of_20M", {0: 17_000_000, 2: 20_000_000, 5: 1_000_000, 9: 7})
    add("wrap_4M_of_20M", {0: 4_000_000, 2: 20_000_000, 5: 1_000_000, 9: 7})
    add("wrap_window_low", {0: 16_843_010, 1: 16_843_009, 4: 9_000_000})
    add("wrap_window_high", {0: 25_264_513, 1: 25_264_514, 4: 12_000_000, 7: 1})
    add("i32_max", {0: 2**31 - 1, 1: 2**31 - 2, 2: 2**30, 6: 1, 7: 2})
    add("ones_and_twos", {0: 1, 1: 2, 2: 1, 3: 2, 4: 2})
    add("min1_floor", {0: 1_000_000, 1: 1, 2: 2, 3: 3000, 8: 3921})
    add("empty", {})
    for k in (0, 5, 15):
        add(f"one_symbol_{k}", {k: 12345})
    add("two_symbols", {3: 10, 12: 1_000_000})
    add("all_16_equal", {k: 100 for k in range(16)})
    add("all_16_ramp", {k: 1000 + 37 * k for k in range(16)})
    add("all_16_fib", {k: v for k, v in enumerate([1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987])})
    add("fib_reversed", {15 - k: v for k, v in enumerate([1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987])})
    add("holes", {0: 500, 3: 500, 7: 90, 11: 90, 15: 7})
    for k in range(15):                                     # a tie between symbols k and k + 1 among distinct others
        bins = {j: 10 + 13 * j for j in range(16)}
        bins[k + 1] = bins[k]
        add(f"tie_at_{k}", bins)
    add("ties_with_merges", {0: 4, 1: 4, 2: 8, 3: 8, 4: 16, 5: 16, 6: 2, 7: 2})
    add("merge_equals_leaf", {0: 6, 1: 3, 2: 3, 3: 6, 4: 12})
    add("typical_frame", {0: 900_000, 1: 310_000, 2: 190_000, 3: 150_000, 4: 120_000, 5: 90_000, 6: 60_000, 7: 30_000, 8: 9_000,
                          9: 2_000, 10: 400, 11: 90, 12: 20, 13: 6, 14: 2, 15: 60_000})
    return rows


def payload_cases():
    """(name, coef [blocks, 256] i16, mv or None, has or None)"""
    rng = np.random.default_rng(20261016)
    cases = []
    # i-frames
    c = np.zeros((12, 256), np.int16)
    cases.append(("all_zero", c, None, None))                       # 17 x (15, 0) + (1, 0) per block
    c = np.zeros((16, 256), np.int16)
    for b, run in enumerate((15, 16, 30, 31, 45, 14, 1, 0)):
        c[b, run] = 3 if b % 2 else -3                              # a run of exactly `run` zeros in front of a value
        c[b, run + 1 + run] = 1                                     # and the same run again behind it
    c[8, 255] = 7                                                   # the last coefficient alone
    c[9, 0] = 16383
    c[9, 1] = -16383
    c[9, 100] = -1
    c[10, :] = -1                                                   # every coefficient -1
    c[11, 240] = 2                                                  # a trailing run of exactly 15
    c[12, 225] = -2                                                 # ... of exactly 30
    c[13, 239] = 5                                                  # ... of exactly 16
    cases.append(("runs", c, None, None))
    for d, nb in ((0.01, 24), (0.1, 16), (0.5, 6), (1.0, 4)):
        c = (rng.integers(-16383, 16384, (nb, 256)) * (rng.random((nb, 256)) < d)).astype(np.int16)
        c[rng.random((nb, 256)) < d / 2] = rng.choice([-1, 1, -2, 2])
        cases.append((f"dense_{d}", c, None, None))
    # p-frames: every (has_mvec, has_coef) combination, vectors at both ends of the legal range
    nb = 20
    c = (rng.integers(-300, 301, (nb, 256)) * (rng.random((nb, 256)) < 0.08)).astype(np.int16)
    c[4] = 0
    c[6, 255] = -16383
    mv = rng.integers(-16, 17, (nb, 2)).astype(np.int8)
    mv[::3] = 0
    mv[1] = (-16, 16)
    mv[2] = (0, -1)
    mv[5] = (16, 0)
    has = (rng.random(nb) < 0.6).astype(np.uint8)
    has[:4] = (0, 1, 0, 1)
    mv[0] = (0, 0); mv[3] = (0, 0)                                  # no vector + no coefficients, no vector + coefficients
    mv[1] = (-16, 16); has[1] = 0                                   # vector without coefficients
    has[2] = 1                                                      # vector and coefficients
    cases.append(("pmixed", c, mv, has))
    cases.append(("pnone", c[:6], np.zeros((6, 2), np.int8), np.zeros(6, np.uint8)))       # nothing coded: an empty table
    cases.append(("pall", c[:8], mv[:8], np.ones(8, np.uint8)))
    return cases


def build():
    v = {}
    rows = crafted_histograms()
    v["hist_names"] = np.array([n for n, _ in rows])
    v["hist"] = np.stack([h for _, h in rows])
    for name, coef, mv, has in payload_cases():
        v[f"pay_{name}_coef"] = coef
        if has is not None:
            v[f"pay_{name}_mv"] = mv
            v[f"pay_{name}_has"] = has
    v.update(er.recompute(v))
    return v


def cross_check(v):
    """the C oracle (oracle/pfv_oracle_entropy.c) must agree with every output"""
    L = Oracle().L
    P = ctypes.c_void_p
    L.pfvo_huffman_from_histogram.argtypes = [P, ctypes.c_int, P, P, P]
    L.pfvo_serialize_iframe.restype = L.pfvo_serialize_pframe.restype = ctypes.c_size_t
    L.pfvo_serialize_iframe.argtypes = [P, ctypes.c_int, P, ctypes.c_size_t]
    L.pfvo_serialize_pframe.argtypes = [P, P, P, ctypes.c_int, P, ctypes.c_size_t]

    def p(a):
        return a.ctypes.data_as(P)

    h = np.ascontiguousarray(v["hist"], np.int32)
    n = h.shape[0]
    t, cv, cl = np.zeros((n, 16), np.uint8), np.zeros((n, 16), np.uint32), np.zeros((n, 16), np.uint8)
    L.pfvo_huffman_from_histogram(p(h), n, p(t), p(cv), p(cl))
    assert np.array_equal(t, v["table"]) and np.array_equal(cv, v["code_val"]) and np.array_equal(cl, v["code_len"])
    for name in er.payload_cases(v):
        coef = np.ascontiguousarray(v[f"pay_{name}_coef"])
        cap = coef.size * 4 + 64
        out = np.zeros(cap, np.uint8)
        if f"pay_{name}_has" in v:
            mv, has = np.ascontiguousarray(v[f"pay_{name}_mv"]), np.ascontiguousarray(v[f"pay_{name}_has"])
            m = L.pfvo_serialize_pframe(p(mv), p(has), p(coef), coef.shape[0], p(out), cap)
        else:
            m = L.pfvo_serialize_iframe(p(coef), coef.shape[0], p(out), cap)
        assert np.array_equal(out[:m], v[f"pay_{name}_bytes"]), name


if __name__ == "__main__":
    v = build()
    cross_check(v)
    np.savez_compressed(er.VECTORS, **v)
    print(f"wrote {er.VECTORS}: {len(v['hist'])} histograms, {len(er.payload_cases(v))} payloads, {os.path.getsize(er.VECTORS)} bytes")
