"""Shared checks of the out-of-loop deblocking filter (include/pfv_hip_ext.h, "out-of-loop deblocking"), driven on the CPU emulator by
tests/test_emu_deblock.py and on a real MI355X by tests/test_gpu_deblock.py at the same small shapes.

The reference is `ref_plane` below: numpy in 64-bit integers, written from the header's text -- two stages, every edge computed from the
stage's input, truncating division as sign * (|a| // n).  Every comparison with it is EQUALITY: the filter is integer arithmetic.  For
sessions and streams the frame that is filtered is what the ORACLE decodes, never a download of the product's own buffers.

Shapes.  The issue lists (129, 17) and (130, 18) among the frame shapes; a frame has even dimensions, so (129, 17) cannot be a frame.  Both
are covered as what they describe -- a second strip 1 or 2 pixels wide and a lower strip row of 1 or 2 rows, without and with an edge
exactly at the seam -- as the chroma planes of (258, 34) and (260, 36), and (130, 18) as a frame as well; (129, 17) as a frame is a
bad-argument case.

Direction of the effect (check_effect): the smallest SSIM gain over the 4 frames x 3 planes is +0.00104 at quality 2 (p-frame luma),
+0.00214 at quality 5 and +0.00393 at quality 10 (p-frame chroma), the largest +0.0573 (i-frame chroma at quality 10); the same figures on
the emulator and on an MI355X.  The issue's own numpy trial gave +0.0010 as the smallest.
"""
import ctypes
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import quality_cases as qc
from quality_cases import PACKED, PADDED, DevBufs, crop, frame_bytes, pad16, padded_frame_bytes, plane_dims, planes_of, to_padded

ROOT = qc.ROOT
# every edge-existence rule and the seams of the strip mapping: 2x2 / 8x8 no edge at all; 10x10 one edge with D the last sample; 16x16 luma
# edges, chroma none; 18x34 / 50x38 ragged, the byte path; 20x20 partial macroblocks; 64x48 aligned, the 16-byte path; 130x18 an edge exactly
# at the strip seam (x = 128, y = 16) with the minimal neighbour; 144x48 / 400x80 interior strips; 258x34 and 260x36: chroma 129x17 / 130x18
SHAPES = [(2, 2), (8, 8), (10, 10), (16, 16), (18, 34), (20, 20), (50, 38), (64, 48), (130, 18), (144, 48), (400, 80), (258, 34), (260, 36)]
STRENGTHS = [(0, 0, 0), (0, 7, 12), (12, 12, 12)]
POISON = 0xA5
P = ctypes.c_void_p


# ------------------------------------------------------------------ the numpy restatement of the normative text
def tdiv(a, n):
    return np.sign(a) * (np.abs(a) // n)


def ref_edge(A, B, C, D, S):
    """one edge on int64 arrays -> (A', B', C', D'); A' and D' are NOT clamped: the text says they need none, check_properties asserts it"""
    d = tdiv(A - 4 * B + 4 * C - D, 8)
    ad = np.abs(d)
    d1 = np.sign(d) * np.maximum(0, ad - np.maximum(0, 2 * (ad - S)))
    lim = np.abs(d1) >> 1
    d2 = np.clip(tdiv(A - D, 4), -lim, lim)
    return A - d2, np.clip(B + d1, 0, 255), np.clip(C - d1, 0, 255), D + d2


def ref_plane(plane, S, stages=2):
    """the filter on one plane (2-D uint8) at strength S -> uint8"""
    h, w = plane.shape
    if S == 0:
        return plane.copy()
    src = plane.astype(np.int64)
    out = src.copy()
    for x in range(8, w - 1, 8):              # x % 8 == 0, x >= 8, x + 1 < w; samples of the INPUT row
        out[:, x - 2], out[:, x - 1], out[:, x], out[:, x + 1] = ref_edge(src[:, x - 2], src[:, x - 1], src[:, x], src[:, x + 1], S)
    if stages == 2:
        src = out.copy()                      # stage 2 works on the stage-1 result
        for y in range(8, h - 1, 8):
            out[y - 2], out[y - 1], out[y], out[y + 1] = ref_edge(src[y - 2], src[y - 1], src[y], src[y + 1], S)
    assert out.min() >= 0 and out.max() <= 255, "A' or D' left 0..255"
    return out.astype(np.uint8)


def ref_frame(frame, w, h, strength):
    return np.concatenate([ref_plane(pl, int(s)).reshape(-1) for pl, s in zip(planes_of(frame, w, h), strength)])


def ref_strength(q0):
    return min(12, int(q0) >> 1)


# ------------------------------------------------------------------ the device call
def deblock_dev(ctx, w, h, frames, layout, strength, src_off=0, src_gap=0, dst_off=0, dst_stride=0, rng=None):
    """pfv_frames_deblock_dev on `frames` ([n, frame bytes of the layout]) -> the n filtered frames.  The source lies src_off bytes into its
    allocation with src_gap random bytes between frames; the destination lies dst_off bytes into a POISONED allocation with 64 guard bytes
    on either side, frames dst_stride apart (0: back to back).  Asserts that every byte outside the n pictures still holds the poison."""
    frames = np.atleast_2d(frames)
    n, sfb = frames.shape
    fb = frame_bytes(w, h)
    rng = rng or np.random.default_rng(7)
    s_stride = sfb + src_gap
    src = rng.integers(0, 256, src_off + n * s_stride + 16, dtype=np.uint8)
    for k in range(n):
        src[src_off + k * s_stride: src_off + k * s_stride + sfb] = frames[k]
    d_stride = dst_stride or fb
    dst = np.full(64 + dst_off + (n - 1) * d_stride + fb + 64, POISON, dtype=np.uint8)
    bufs = DevBufs(ctx)
    try:
        s_dev, d_dev = bufs.put(src), bufs.put(dst)
        st = np.array(strength, dtype=np.uint8)
        rc = ctx._lib.pfv_frames_deblock_dev(ctx.handle, w, h, n, P(s_dev + src_off), layout, s_stride if src_gap else 0, P(d_dev + 64 + dst_off), dst_stride,
                                             st.ctypes.data_as(P))
        ctx.check(rc)
        ctx.download(dst, d_dev)
    finally:
        bufs.close()
    got = np.stack([dst[64 + dst_off + k * d_stride: 64 + dst_off + k * d_stride + fb] for k in range(n)])
    rest = dst.copy()
    for k in range(n):
        rest[64 + dst_off + k * d_stride: 64 + dst_off + k * d_stride + fb] = POISON
    assert (rest == POISON).all(), f"bytes outside the {n} pictures were written: {np.flatnonzero(rest != POISON)[:8]}"
    return got


def odd_stride(fb):
    s = fb + 21
    return s if s % 16 else s + 1


# ------------------------------------------------------------------ 1. exact equality with numpy
def check_shape(pkg, ctx, w, h, seed=1):
    """random bytes, two streams, every strength triple; PACKED and PADDED source (random padding); aligned, and at an unaligned source base
    with a gap between the frames and an unaligned destination whose stride is no multiple of 16.  A picture byte that is not written
    keeps the poison and so differs from numpy's value (which the first assert shows is not the poison everywhere)."""
    rng = np.random.default_rng(seed * 1000 + w * 7 + h)
    fb = frame_bytes(w, h)
    a = rng.integers(0, 256, (2, fb), dtype=np.uint8)
    forms = {PACKED: a, PADDED: np.stack([to_padded(x, w, h, rng) for x in a])}
    assert forms[PADDED].shape[1] == padded_frame_bytes(w, h)
    for strength in STRENGTHS:
        want = np.stack([ref_frame(x, w, h, strength) for x in a])
        assert fb < 64 or (want != POISON).any()
        if strength == (0, 0, 0):
            assert np.array_equal(want, a)
        for layout in (PACKED, PADDED):
            got = deblock_dev(ctx, w, h, forms[layout], layout, strength, rng=rng)
            assert np.array_equal(got, want), (w, h, strength, layout, "aligned", np.flatnonzero(got != want)[:8])
            got = deblock_dev(ctx, w, h, forms[layout], layout, strength, src_off=3, src_gap=37, dst_off=5, dst_stride=odd_stride(fb), rng=rng)
            assert np.array_equal(got, want), (w, h, strength, layout, "unaligned", np.flatnonzero(got != want)[:8])
    # the host entry point and the Python mirror
    got = pkg.frames_deblock(ctx, w, h, a, STRENGTHS[1])
    assert got.dtype == np.uint8 and np.array_equal(got, np.stack([ref_frame(x, w, h, STRENGTHS[1]) for x in a]))


# ------------------------------------------------------------------ 2. arithmetic traps
# (A, B, C, D, S) -> (A', B', C', D'), worked out by hand from the text
TRAPS = [
    # A - 4B + 4C - D = -4: truncation gives d = 0 (floor: -1), nothing moves
    ((100, 101, 100, 100, 12), (100, 101, 100, 100)),
    # = -12: d = -1 (floor: -2)
    ((100, 103, 100, 100, 12), (100, 102, 101, 100)),
    # d = 3, |d1| >> 1 = 1, A - D = -3: tdiv(-3, 4) = 0 (floor: -1), A and D stay
    ((97, 100, 108, 100, 12), (97, 103, 105, 100)),
    # S = 4, A = B = 100, C = D = 100 + k: |d| = 3 (S - 1): d1 = 3 is odd, d2 = tdiv(-8, 4) = -2 is limited to -(3 >> 1) = -1
    ((100, 100, 108, 108, 4), (101, 103, 105, 107)),
    # |d| = 4 (S): d1 = 4, d2 = tdiv(-11, 4) = -2 within the limit 2
    ((100, 100, 111, 111, 4), (102, 104, 107, 109)),
    # |d| = 7 (2S - 1): d1 = 1, limit 0
    ((100, 100, 119, 119, 4), (100, 101, 118, 119)),
    # |d| = 8 (2S) and 9 (2S + 1): a real edge, the output is the input
    ((100, 100, 122, 122, 4), (100, 100, 122, 122)),
    ((100, 100, 124, 124, 4), (100, 100, 124, 124)),
    # the same ramp falling: d = -7, -8
    ((119, 119, 100, 100, 4), (119, 118, 101, 100)),
    ((122, 122, 100, 100, 4), (122, 122, 100, 100)),
    # B + d1 = 261 clips at 255; d2 = tdiv(55, 4) = 13 limited to 3
    ((255, 254, 255, 200, 12), (252, 255, 248, 203)),
    # C - d1 = 261 clips at 255
    ((200, 255, 254, 255, 12), (203, 248, 255, 252)),
    # B + d1 = -6 clips at 0
    ((0, 1, 0, 55, 12), (3, 0, 7, 52)),
    # C - d1 = -6 clips at 0
    ((55, 0, 1, 0, 12), (52, 7, 0, 3)),
    # S = 1: d = 1 moves B and C by one, d = 2 nothing
    ((100, 100, 103, 103, 1), (100, 101, 102, 103)),
    ((100, 100, 106, 106, 1), (100, 100, 106, 106)),
]


def check_traps(pkg, ctx):
    """each trap as a vertical edge (a 16 x 8 frame: rows are independent, no horizontal edge exists) and as a horizontal edge (8 x 16),
    in luma; the hand-worked values, numpy and the device agree"""
    for (A, B, C, D, S), want in TRAPS:
        r = ref_edge(*(np.array([v], dtype=np.int64) for v in (A, B, C, D)), S)
        assert tuple(int(v[0]) for v in r) == want, ((A, B, C, D, S), r, want)
    by_s = {}
    for (A, B, C, D, S), want in TRAPS:
        by_s.setdefault(S, []).append(((A, B, C, D), want))
    rng = np.random.default_rng(5)
    for S, cases in by_s.items():
        for k0 in range(0, len(cases), 8):
            part = cases[k0:k0 + 8]
            for vertical in (True, False):
                w, h = (16, 8) if vertical else (8, 16)
                f = rng.integers(0, 256, frame_bytes(w, h), dtype=np.uint8)
                luma = f[:w * h].reshape(h, w)
                want = f.copy()
                wl = want[:w * h].reshape(h, w)
                for k, (inp, out) in enumerate(part):
                    if vertical:
                        luma[k, 6:10] = inp
                        wl[k, 6:10] = out
                    else:
                        luma[6:10, k] = inp
                        wl[6:10, k] = out
                want[:w * h] = wl.reshape(-1)
                if len(part) == 8:       # all eight lines are traps: every luma sample's expected value is hand-worked or the input
                    assert np.array_equal(ref_frame(f, w, h, (S, 0, 0)), want)
                got = deblock_dev(ctx, w, h, f, PACKED, (S, 0, 0))[0]
                ref = ref_frame(f, w, h, (S, 0, 0))
                assert np.array_equal(got, ref), (S, vertical)
                gl = got[:w * h].reshape(h, w)
                for k, (inp, out) in enumerate(part):
                    line = gl[k, 6:10] if vertical else gl[6:10, k]
                    assert tuple(int(v) for v in line) == out, (inp, S, vertical, line, out)


def check_properties(pkg, ctx, w=64, h=48):
    """A' and D' never leave 0..255 (a property of the arithmetic: all 2^32 inputs are too many, so random rows at every strength, and
    the extremes); a flat plane and S = 0 are copies; a corner sample is touched by both stages"""
    rng = np.random.default_rng(11)
    q = rng.integers(0, 256, (4, 200000)).astype(np.int64)
    ext = np.array(np.meshgrid(*[[0, 1, 127, 128, 254, 255]] * 4)).reshape(4, -1).astype(np.int64)
    for S in range(0, 13):
        for v in (q, ext):
            A2, B2, C2, D2 = ref_edge(v[0], v[1], v[2], v[3], S)
            assert A2.min() >= 0 and A2.max() <= 255 and D2.min() >= 0 and D2.max() <= 255
            assert (np.abs(A2 - v[0]) <= np.abs(v[0] - v[3]) // 4).all() and (A2 - v[0] == v[3] - D2).all()
            if S == 0:
                assert all(np.array_equal(x, y) for x, y in zip((A2, B2, C2, D2), v))
    flat = np.concatenate([np.full(pw * ph, val, dtype=np.uint8) for (pw, ph), val in zip(plane_dims(w, h), (90, 0, 255))])
    for strength in STRENGTHS:
        assert np.array_equal(deblock_dev(ctx, w, h, flat, PACKED, strength)[0], flat)
    a = rng.integers(0, 256, frame_bytes(w, h), dtype=np.uint8)
    assert np.array_equal(deblock_dev(ctx, w, h, a, PACKED, (0, 0, 0))[0], a)
    # a corner: a soft step in both directions at (8, 8), so that the sample there moves in stage 1 and again in stage 2
    f = np.zeros(frame_bytes(16, 16), dtype=np.uint8)
    luma = f[:256].reshape(16, 16)
    luma[:] = 100
    luma[:, 8:] += 8
    luma[8:, :] += 8
    s1 = ref_plane(luma, 12, stages=1)
    s2 = ref_plane(luma, 12)
    assert luma[8, 8] != s1[8, 8] != s2[8, 8]
    got = deblock_dev(ctx, 16, 16, f, PACKED, (12, 12, 12))[0]
    assert np.array_equal(got, ref_frame(f, 16, 16, (12, 12, 12))) and got[8 * 16 + 8] == s2[8, 8]


# ------------------------------------------------------------------ 3. locality
def reach(v, size):
    """the positions along one axis that a change at position v can move: itself, or all four samples of the edge it feeds"""
    for e in range(8, size - 1, 8):
        if e - 2 <= v <= e + 1:
            return set(range(e - 2, e + 2))
    return {v}


def check_locality(pkg, ctx, w, h, px, py):
    """one luma sample changed: the outputs that differ lie within the columns of the vertical edge the sample feeds and, through those,
    within the rows of the horizontal edges; and they are exactly the outputs that differ in numpy"""
    rng = np.random.default_rng(px * 31 + py)
    # a smooth field with small noise, so that the edges are inside the ramp and a change propagates
    yy, xx = np.mgrid[0:h, 0:w]
    luma = (100 + xx // 8 * 3 + yy // 8 * 2 + rng.integers(0, 3, (h, w))).astype(np.uint8)
    a = np.concatenate([luma.reshape(-1), rng.integers(0, 256, frame_bytes(w, h) - w * h, dtype=np.uint8)])
    b = a.copy()
    b[py * w + px] = a[py * w + px] + 9
    strength = (12, 12, 12)
    ra, rb = ref_frame(a, w, h, strength), ref_frame(b, w, h, strength)
    want = set(np.flatnonzero(ra != rb))
    assert want, "the change does not show in the reference"
    cols = reach(px, w)
    rows = set().union(*[reach(r, h) for r in {py}])
    allowed = {r * w + c for r in rows for c in cols}
    assert want <= allowed, (sorted(want - allowed)[:8])
    got = set()
    for layout in (PACKED, PADDED):
        fa = a if layout == PACKED else to_padded(a, w, h, rng)
        fb_ = b if layout == PACKED else to_padded(b, w, h, rng)
        ga, gb = deblock_dev(ctx, w, h, fa, layout, strength)[0], deblock_dev(ctx, w, h, fb_, layout, strength)[0]
        assert np.array_equal(ga, ra) and np.array_equal(gb, rb)
        got = set(np.flatnonzero(ga != gb))
        assert got == want and got <= allowed, (layout, sorted(got ^ want)[:8])
    return len(got)


# ------------------------------------------------------------------ 4. bad arguments
def check_bad_arguments(pkg, ctx):
    L = pkg._lib
    lib = ctx._lib
    w, h = 16, 16
    fb, pfb = frame_bytes(w, h), padded_frame_bytes(w, h)
    bufs = DevBufs(ctx)
    try:
        a = bufs.put(np.zeros(4 * pfb, dtype=np.uint8))
        d = bufs.put(np.zeros(4 * pfb, dtype=np.uint8))
        ok = np.array([1, 2, 3], np.uint8)

        def call(w=w, h=h, n=1, src=a, layout=PACKED, ss=0, dst=d, ds=0, st=ok, ctx_h=ctx.handle):
            return lib.pfv_frames_deblock_dev(ctx_h, w, h, n, P(src) if src else None, layout, ss, P(dst) if dst else None, ds,
                                              st.ctypes.data_as(P) if st is not None else None)
        assert call() == L.PFV_OK and call(n=2, layout=PADDED) == L.PFV_OK
        for bad in ((15, 16), (16, 17), (0, 16), (16, -2), (65536, 16), (129, 17)):          # dimensions a frame cannot have
            assert call(w=bad[0], h=bad[1]) == L.PFV_ERR_BAD_ARG, bad
        assert call(n=0) == L.PFV_ERR_BAD_ARG and call(n=-1) == L.PFV_ERR_BAD_ARG
        assert call(layout=2) == L.PFV_ERR_BAD_ARG and call(layout=-1) == L.PFV_ERR_BAD_ARG
        assert call(src=None) == L.PFV_ERR_BAD_ARG and call(dst=None) == L.PFV_ERR_BAD_ARG and call(st=None) == L.PFV_ERR_BAD_ARG
        assert call(ctx_h=None) == L.PFV_ERR_BAD_ARG
        for k in range(3):
            st = ok.copy()
            st[k] = 13
            assert call(st=st) == L.PFV_ERR_BAD_ARG
            st[k] = 12
            assert call(st=st) == L.PFV_OK
            st[k] = 255
            assert call(st=st) == L.PFV_ERR_BAD_ARG
        assert call(n=2, ds=fb - 1) == L.PFV_ERR_BAD_ARG and call(n=2, ds=fb) == L.PFV_OK              # a short destination stride
        assert call(n=2, ss=fb - 1) == L.PFV_ERR_BAD_ARG and call(n=2, layout=PADDED, ss=pfb - 1) == L.PFV_ERR_BAD_ARG
        assert call(n=2, layout=PADDED, ss=pfb) == L.PFV_OK
        # in-place and overlapping ranges, either way round
        assert call(dst=a) == L.PFV_ERR_BAD_ARG
        assert call(dst=a + fb - 1) == L.PFV_ERR_BAD_ARG and call(dst=a + fb) == L.PFV_OK
        assert call(src=a + fb, dst=a + 1) == L.PFV_ERR_BAD_ARG and call(src=a + fb, dst=a) == L.PFV_OK
        # a range runs from the first frame to the end of the last, gaps included: here the source lies in the destination's gap and last frame
        assert call(n=2, src=a + fb, dst=a, ds=2 * fb) == L.PFV_ERR_BAD_ARG
        assert call(layout=PADDED, dst=a + pfb - 1) == L.PFV_ERR_BAD_ARG and call(layout=PADDED, dst=a + pfb) == L.PFV_OK
        # the host form
        host, out = np.zeros(fb, np.uint8), np.zeros(fb, np.uint8)
        hp = lambda x: x.ctypes.data_as(P)      # noqa: E731
        assert lib.pfv_frames_deblock(ctx.handle, w, h, 1, hp(host), hp(out), hp(ok)) == L.PFV_OK
        assert lib.pfv_frames_deblock(ctx.handle, 15, h, 1, hp(host), hp(out), hp(ok)) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_deblock(ctx.handle, w, h, 0, hp(host), hp(out), hp(ok)) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_deblock(ctx.handle, w, h, 1, None, hp(out), hp(ok)) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_deblock(ctx.handle, w, h, 1, hp(host), None, hp(ok)) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_deblock(ctx.handle, w, h, 1, hp(host), hp(out), None) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_deblock(ctx.handle, w, h, 1, hp(host), hp(out), hp(np.array([0, 13, 0], np.uint8))) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_deblock(None, w, h, 1, hp(host), hp(out), hp(ok)) == L.PFV_ERR_BAD_ARG
        # the switches
        assert lib.pfv_dec_set_deblock(None, 1, None) == L.PFV_ERR_BAD_ARG and lib.pfv_decoder_set_deblock(None, 1, None) == L.PFV_ERR_BAD_ARG
        dec = pkg.DecoderSession(ctx, w, h, np.stack(pkg.qtables_from_quality(5)[:4]), 1)
        try:
            assert lib.pfv_dec_set_deblock(dec.handle, 3, hp(ok)) == L.PFV_ERR_BAD_ARG and lib.pfv_dec_set_deblock(dec.handle, -1, hp(ok)) == L.PFV_ERR_BAD_ARG
            assert lib.pfv_dec_set_deblock(dec.handle, L.PFV_DEBLOCK_FIXED, None) == L.PFV_ERR_BAD_ARG
            assert lib.pfv_dec_set_deblock(dec.handle, L.PFV_DEBLOCK_FIXED, hp(np.array([0, 0, 13], np.uint8))) == L.PFV_ERR_BAD_ARG
            assert lib.pfv_dec_set_deblock(dec.handle, L.PFV_DEBLOCK_AUTO, None) == L.PFV_OK
            assert lib.pfv_dec_set_deblock(dec.handle, L.PFV_DEBLOCK_OFF, None) == L.PFV_OK
            with pytest.raises(pkg.PfvError):
                dec.set_deblock("fixed", (13, 0, 0))
        finally:
            dec.close()
        ctx.sync()
    finally:
        bufs.close()


# ------------------------------------------------------------------ 5. the automatic strength
def check_strength(pkg):
    for quality in range(11):
        tabs = pkg.qtables_from_quality(quality)[:4]
        got = [pkg.deblock_strength(t) for t in tabs]
        assert got == [ref_strength(t.reshape(-1)[0]) for t in tabs], quality
        if quality == 0:
            assert got == [0, 0, 0, 0]
        if quality == 10:
            assert got == [5, 10, 10, 12]
    assert [pkg.deblock_strength(pkg.qtables_from_quality(q)[0]) for q in (2, 5, 10)] == [1, 2, 5]
    for q0, want in ((0, 0), (1, 0), (2, 1), (24, 12), (25, 12), (65535, 12)):
        t = np.full(64, 3, dtype=np.int32)
        t[0] = q0
        assert pkg.deblock_strength(t) == want == ref_strength(q0), q0


# ------------------------------------------------------------------ 6. decoder session, out of loop
def auto_strengths(pkg, quality):
    s = [pkg.deblock_strength(t) for t in pkg.qtables_from_quality(quality)[:4]]
    return {"I": (s[0], s[1], s[1]), "P": (s[2], s[3], s[3])}


def check_dec_session(pkg, ctx, oracle, path, w=64, h=48, quality=5, n=2):
    """I P P against the oracle's decoder, AUTO then FIXED then OFF, through one of the ways a frame leaves the session:
         get_frame   pfv_dec_get_frame (host)
         output      the output buffer of pfv_dec_set_output_dev (64 x 48: the geometry whose crop the decode kernels fuse when the switch is off)
         strided     pfv_dec_set_output_strided_dev with an unaligned stride and a window of slot 1 alone: slot 0's frame and the gaps keep
                     their poison
    After every frame pfv_dec_framebuffer equals the oracle's: the filter never feeds back."""
    from oracle_bind import OracleDecoder
    tabs = np.stack(oracle.qtables(quality)[:4])
    auto = auto_strengths(pkg, quality)
    assert auto["I"] != auto["P"] and any(auto["I"]), auto
    fixed = (3, 0, 9)
    fb = frame_bytes(w, h)
    tb = qc.total_blocks(w, h)
    slots = [1] if path == "strided" else list(range(n))
    stride = odd_stride(fb) if path == "strided" else fb
    for mode in ("auto", "fixed", "off"):
        streams = [pkg.SyntheticStream(w, h, seed=61 + k) for k in range(n)]
        oenc = [oracle.encoder(w, h, quality) for _ in range(n)]
        odec = [OracleDecoder(oracle, w, h, tabs) for _ in range(n)]
        dec = pkg.DecoderSession(ctx, w, h, tabs, n)
        bufs = DevBufs(ctx)
        try:
            out_dev = bufs.put(np.full(n * stride + 64, POISON, np.uint8))
            if path == "output":
                dec.set_output_dev(out_dev)
            elif path == "strided":
                dec.set_output_strided_dev(out_dev, stride)
                dec.set_window(1, 1)
            dec.set_deblock(mode, fixed if mode == "fixed" else None)
            for t in range(3):
                frames = np.stack([s.frame(t) for s in streams])
                kind = "I" if t == 0 else "P"
                if t == 0:
                    coef = np.stack([o.encode_iframe(f) for o, f in zip(oenc, frames)])
                    [odec[k].decode_iframe(coef[k]) for k in slots]
                    if path == "get_frame":
                        dec.decode_iframe(coef)
                    else:
                        dec.decode_iframe_dev(bufs.put(coef))
                else:
                    parts = [o.encode_pframe(f) for o, f in zip(oenc, frames)]
                    mv, has, coef = (np.stack([p[i] for p in parts]) for i in range(3))
                    [odec[k].decode_pframe(*parts[k]) for k in slots]
                    if path == "get_frame":
                        dec.decode_pframe(mv, has, coef)
                    else:
                        dec.decode_pframe_dev(bufs.put(mv), bufs.put(has), bufs.put(coef))
                        dec.check()
                strength = {"auto": auto[kind], "fixed": fixed, "off": (0, 0, 0)}[mode]
                plain = {k: crop(odec[k].framebuffer(), w, h) for k in slots}
                want = {k: ref_frame(plain[k], w, h, strength) for k in slots}
                if mode != "off":
                    assert any(not np.array_equal(want[k], plain[k]) for k in slots), "the filter changes nothing here: the check would be empty"
                if path == "get_frame":
                    got = dec.get_frame()
                    for k in slots:
                        assert np.array_equal(got[k], want[k]), (mode, t, k)
                    dev = bufs.put(np.full(n * fb, POISON, np.uint8))        # and pfv_dec_get_frame_dev
                    dec.get_frame_dev(dev)
                    got2 = np.zeros((n, fb), np.uint8)
                    ctx.download(got2, dev)
                    assert np.array_equal(got2, got)
                else:
                    raw = np.zeros(n * stride + 64, np.uint8)
                    ctx.download(raw, out_dev)
                    for k in slots:
                        assert np.array_equal(raw[k * stride:k * stride + fb], want[k]), (mode, t, k, path)
                        raw[k * stride:k * stride + fb] = POISON
                    assert (raw == POISON).all(), "bytes outside the window's frames were written"
                fbuf = dec.framebuffer()
                for k in slots:
                    assert np.array_equal(fbuf[k], odec[k].framebuffer()), (mode, t, k, "framebuffer")
            if mode != "off" and path == "get_frame":      # back to OFF: the plain crop again, from the same framebuffer
                dec.set_deblock("off")
                assert np.array_equal(dec.get_frame(), np.stack([plain[k] for k in slots]))
        finally:
            bufs.close()
            dec.close()


def check_dec_graph(pkg, ctx, oracle, w=64, h=48, quality=5, n=2):
    """I P P with AUTO on recorded in one graph (three output buffers) and replayed twice: both replays equal numpy-deblock of the oracle's
    frames, bit for bit"""
    from oracle_bind import OracleDecoder
    tabs = np.stack(oracle.qtables(quality)[:4])
    auto = auto_strengths(pkg, quality)
    fb = frame_bytes(w, h)
    streams = [pkg.SyntheticStream(w, h, seed=71 + k) for k in range(n)]
    oenc = [oracle.encoder(w, h, quality) for _ in range(n)]
    odec = [OracleDecoder(oracle, w, h, tabs) for _ in range(n)]
    dec = pkg.DecoderSession(ctx, w, h, tabs, n)
    bufs = DevBufs(ctx)
    graph = pkg.Graph(ctx)
    try:
        steps, want = [], []
        for t in range(3):
            frames = np.stack([s.frame(t) for s in streams])
            if t == 0:
                coef = np.stack([o.encode_iframe(f) for o, f in zip(oenc, frames)])
                [d.decode_iframe(c) for d, c in zip(odec, coef)]
                steps.append((bufs.put(coef),))
            else:
                parts = [o.encode_pframe(f) for o, f in zip(oenc, frames)]
                [d.decode_pframe(*p) for d, p in zip(odec, parts)]
                steps.append(tuple(bufs.put(np.stack([p[i] for p in parts])) for i in range(3)))
            want.append(np.stack([ref_frame(crop(d.framebuffer(), w, h), w, h, auto["I" if t == 0 else "P"]) for d in odec]))
        outs = [bufs.put(np.full(n * fb, POISON, np.uint8)) for _ in range(3)]
        dec.set_deblock("auto")
        with graph:
            for t, st in enumerate(steps):
                dec.set_output_dev(outs[t])
                if t == 0:
                    dec.decode_iframe_dev(*st)
                else:
                    dec.decode_pframe_dev(*st)
        for _ in range(2):
            for o in outs:
                ctx.upload(o, np.full(n * fb, POISON, np.uint8))
            graph.launch()
            for t, o in enumerate(outs):
                got = np.zeros((n, fb), np.uint8)
                ctx.download(got, o)
                assert np.array_equal(got, want[t]), t
        dec.check()
    finally:
        graph.close()
        bufs.close()
        dec.close()


# ------------------------------------------------------------------ 7. pfv_decoder
def oracle_clip(pkg, oracle, w, h, quality, frames, plan):
    from oracle_bind import OracleStreamEncoder
    oenc = OracleStreamEncoder(oracle, w, h, 30, quality)
    for f, kind in zip(frames, plan):
        {"D": lambda f: oenc.encode_dropframe(), "I": oenc.encode_iframe, "P": oenc.encode_pframe}[kind](f)
    oenc.finish()
    return oenc.bytes()


def decode_all(pkg, ctx, dec, w, h, device_out):
    """one entry per advance call that delivered a frame"""
    got = []
    fb = frame_bytes(w, h)

    def take(fr):
        if device_out:
            a = np.zeros(fb, np.uint8)
            ctx.download(a, fr)
            got.append(a)
        else:
            got.append(fr.packed())
    while dec.advance_frame(take):
        pass
    return got


def check_decoder(pkg, ctx, oracle, entropy, device_out, w=48, h=32, quality=5, n_frames=5, gop=3, drop_at=2):
    """a 5-frame .pfv with one drop frame: the callback's frames equal numpy-deblock of the oracle stream decoder's frames at the strengths
    of each packet's tables (AUTO), at the fixed ones (FIXED), and the oracle's frames themselves (OFF); reset() and decoding again
    give the same frames"""
    st = pkg.SyntheticStream(w, h)
    frames = [st.frame(t) for t in range(n_frames)]
    plan = qc.clip_plan(n_frames, gop, drop_at)
    data = oracle_clip(pkg, oracle, w, h, quality, frames, plan)
    shown = qc.oracle_decode(oracle, data)
    auto = auto_strengths(pkg, quality)
    fixed = (12, 1, 6)
    for mode in ("auto", "fixed", "off"):
        want = []
        for fr, kind in zip(shown, plan):
            if fr is not None:
                want.append(ref_frame(fr, w, h, {"auto": auto.get(kind), "fixed": fixed, "off": (0, 0, 0)}[mode]))
        assert len(want) == n_frames - 1
        if mode != "off":
            assert any(not np.array_equal(a, b) for a, b in zip(want, [f for f in shown if f is not None]))
        dec = pkg.Decoder(data, ctx, entropy=entropy)
        try:
            if device_out:
                dec.set_output_device(True)
            dec.set_deblock(mode, fixed if mode == "fixed" else None)
            got = decode_all(pkg, ctx, dec, w, h, device_out)
            assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want)), (mode, entropy, device_out)
            dec.reset()
            again = decode_all(pkg, ctx, dec, w, h, device_out)
            assert len(again) == len(want) and all(np.array_equal(a, b) for a, b in zip(again, want)), (mode, "after reset")
        finally:
            dec.close()


# ------------------------------------------------------------------ 8. direction of the effect
def effect_clip(w=176, h=144, n_frames=4):
    """luma 128 + 60 sin(x/23) cos(y/17) + 40 sin((x+y)/41), rounded and clamped; chroma sampled from the same field at the even positions;
    every frame shifted by (5, 3) against the one before"""
    out = []
    for t in range(n_frames):
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        xx, yy = xx + 5 * t, yy + 3 * t
        field = np.clip(np.rint(128 + 60 * np.sin(xx / 23) * np.cos(yy / 17) + 40 * np.sin((xx + yy) / 41)), 0, 255).astype(np.uint8)
        c = field[::2, ::2]
        out.append(np.concatenate([field.reshape(-1), c.reshape(-1), c.reshape(-1)]))
    return out


def check_effect(pkg, ctx, oracle, quality, w=176, h=144):
    """I + 3 P of the smooth synthetic clip: at qualities 2, 5 and 10 the device SSIM (pfv_frames_ssim) of EVERY plane of EVERY AUTO-deblocked
    frame is strictly above that of the unfiltered frame; at quality 0 the AUTO-deblocked frame is the unfiltered one.  A condition, not a
    tolerance.  The figures are printed before the assert."""
    frames = effect_clip(w, h)
    plan = ["I", "P", "P", "P"]
    data = oracle_clip(pkg, oracle, w, h, quality, frames, plan)
    got = {}
    for mode in ("off", "auto"):
        dec = pkg.Decoder(data, ctx)
        try:
            dec.set_deblock(mode)
            got[mode] = decode_all(pkg, ctx, dec, w, h, False)
        finally:
            dec.close()
    shown = qc.oracle_decode(oracle, data)
    assert len(got["off"]) == len(got["auto"]) == 4 and all(np.array_equal(a, b) for a, b in zip(got["off"], shown))
    if quality == 0:
        assert all(np.array_equal(a, b) for a, b in zip(got["auto"], got["off"]))
        return None
    src = np.stack(frames)
    plain = pkg.frames_ssim(ctx, w, h, src, np.stack(got["off"]))
    filt = pkg.frames_ssim(ctx, w, h, src, np.stack(got["auto"]))
    nw = np.array(pkg.ssim_windows(w, h), dtype=np.float64)
    gain = (filt - plain) / (nw * (1 << 24))
    print(f"deblock effect q{quality}: SSIM gain per frame and plane\n{np.array2string(gain, precision=5)}\nsmallest {gain.min():.5f}")
    assert (filt > plain).all(), (quality, gain)
    return gain


# ------------------------------------------------------------------ 9. C++ mirror and tool
def build_cpp(lib_path, exe):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "deblock_report.cpp"), "-o", exe, lib_path, "-Wl,-rpath," + os.path.dirname(lib_path)], check=True)


def check_cpp(pkg, ctx, oracle, exe, tmp_path, w=48, h=32, quality=5):
    """tests/cpp/deblock_report.cpp (pfv::Decoder::set_deblock, pfv::frames_deblock, pfv::deblock_strength) writes what numpy computes from
    the oracle decoder's frames"""
    st = pkg.SyntheticStream(w, h)
    frames = [st.frame(t) for t in range(4)]
    plan = ["I", "P", "P", "I"]
    data = oracle_clip(pkg, oracle, w, h, quality, frames, plan)
    shown = qc.oracle_decode(oracle, data)
    auto = auto_strengths(pkg, quality)
    src = str(tmp_path / "in.pfv")
    open(src, "wb").write(data)
    fixed = (4, 9, 2)
    for mode, name in ((1, "auto"), (2, "fixed"), (0, "off")):
        o1, o2 = str(tmp_path / f"{name}.yuv"), str(tmp_path / f"{name}_f.yuv")
        r = subprocess.run([exe, src, str(mode), *[str(v) for v in fixed], "9", o1, o2], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert r.stdout.splitlines() == ["strength 4", f"frames 4 of {w}x{h}"]
        want = np.stack([ref_frame(f, w, h, {"auto": auto[k], "fixed": fixed, "off": (0, 0, 0)}[name]) for f, k in zip(shown, plan)])
        got = np.fromfile(o1, dtype=np.uint8).reshape(4, -1)
        assert np.array_equal(got, want), name
        again = np.fromfile(o2, dtype=np.uint8).reshape(4, -1)
        assert np.array_equal(again, np.stack([ref_frame(f, w, h, fixed) for f in want])), name


def check_rd_tool(pkg, oracle, lib_path, tmp_path, w=64, h=48, n_frames=4, gop=3, qualities=(0, 5, 10)):
    """tools/rd_curve.py --deblock --dump on the library at lib_path: the dumped reconstruction is the oracle encoder's, the dumped
    deblocked frames are numpy-deblock of it at the automatic strengths, and the db_ columns equal a recomputation from the dumped frames
    (PSNR exactly, SSIM inside the tolerance tests/ssim_cases.py derives); without the flag the lines are the same minus the new keys"""
    import ssim_cases as sc
    env = dict(os.environ)
    if lib_path:
        env["PFV_HIP_LIB"] = lib_path
    dump = str(tmp_path / "dump")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "rd_curve.py"), str(w), str(h), str(n_frames), "--gop", str(gop),
           "--qualities", ",".join(str(q) for q in qualities)]
    plain = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert plain.returncode == 0, plain.stderr
    r = subprocess.run(cmd + ["--deblock", "--dump", dump], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr
    lines = [json.loads(x) for x in r.stdout.splitlines()]
    new = ("ssim_y", "ssim_u", "ssim_v", "ssim_all", "db_strength_i", "db_strength_p")
    stripped = [{k: v for k, v in d.items() if k not in new and not k.startswith("db_")} for d in lines]
    assert [json.dumps(d) for d in stripped] == plain.stdout.splitlines()
    assert [d["quality"] for d in lines] == list(qualities)
    fb = frame_bytes(w, h)
    nw = np.array(sc.windows_of(w, h), dtype=np.float64)
    st = pkg.SyntheticStream(w, h)
    for d in lines:
        q = d["quality"]
        auto = auto_strengths(pkg, q)
        assert d["db_strength_i"] == list(auto["I"]) and d["db_strength_p"] == list(auto["P"])
        inp, rec, dbl = (np.fromfile(os.path.join(dump, f"q{q}_{name}.yuv"), dtype=np.uint8).reshape(n_frames, fb) for name in ("input", "recon", "deblocked"))
        oenc = oracle.encoder(w, h, q)
        psnr, ssim = [], []
        for t in range(n_frames):
            f = st.frame(t)
            assert np.array_equal(inp[t], f)
            (oenc.encode_iframe if t % gop == 0 else oenc.encode_pframe)(f)
            assert np.array_equal(rec[t], crop(oenc.prev_frame(), w, h)), (q, t)
            assert np.array_equal(dbl[t], ref_frame(rec[t], w, h, auto["I" if t % gop == 0 else "P"])), (q, t)
            sse, _ = qc.ref_sse(f, dbl[t], w, h)
            psnr.append([pkg.psnr(int(sse[i]), pw * ph) for i, (pw, ph) in enumerate(plane_dims(w, h))] + [pkg.psnr(int(sse.sum()), fb)])
            sums, _ = sc.ref_ssim(f, dbl[t], w, h)
            ssim.append(list(sums / (sc.ONE * nw)) + [float(sums.sum() / (sc.ONE * nw.sum()))])
        if q == 0:
            assert np.array_equal(dbl, rec)
        for k, key in enumerate(("db_psnr_y", "db_psnr_u", "db_psnr_v", "db_psnr_yuv")):
            assert d[key] == sum(p[k] for p in psnr) / n_frames, key
        for k, key in enumerate(("db_ssim_y", "db_ssim_u", "db_ssim_v", "db_ssim_all")):
            assert abs(d[key] - float(np.mean([s[k] for s in ssim]))) <= sc.TOL / sc.ONE, key
    return lines
