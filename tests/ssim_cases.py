"""Shared checks of the structural-similarity entry points (include/pfv_hip_ext.h, "structural similarity on the device"), driven on the
CPU emulator by tests/test_emu_ssim.py and on a real MI355X by tests/test_gpu_ssim.py at the same small shapes.

The reference is numpy: the four integers of every window in int64 exactly as the header defines them, the window value a float64
quotient.  For sessions and streams the second operand is what the ORACLE reconstructs / decodes, never a download of the product's own
buffers.

Tolerance (derived, not measured).  The device forms the same four integers exactly and then rounds: four int -> f32 conversions, two
products and one division (allowed 2.5 ulp), each relative 2^-24 or less -- with |ssim| <= 1 under 2^-20 per window, that is 16 units of
2^-24; the final rint adds 1/2.  So
    |device plane sum - sum(ref * 2^24)| <= 16.5 * windows of the plane
    |map entry - its reference|           <= 16.5 * windows of that macroblock
An error in window placement, a halo or a mask moves values by 1e-3 (16 000 units) or more.  Where the value of every window is known
exactly (identical operands: 2^24; all 0 against all 255: 26), and wherever two results of the device are compared, the check is equality.
"""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import quality_cases as qc
from quality_cases import (LAYOUT_PAIRS, PACKED, PADDED, DevBufs, crop, frame_bytes, pad16, padded_frame_bytes, plane_dims, planes_of,
                           to_padded, total_blocks)

ROOT = qc.ROOT
ONE = 1 << 24
TOL = 16.5
C1, C2 = 416, 235963
# 2x2: no windows anywhere; 8x8: one Y window, no chroma windows; 18x34: chroma 9x17 -- 1x3 windows, ignored partial blocks, the byte path;
# 20x20: the fifth block row and column lie in partial macroblocks; 50x38: ragged in both axes; 144x48: windows straddle the strip boundary
# at x = 128, with strips below; 400x80: interior strips, several strips per workgroup, halo rows from the strip below; 64x48: fully
# aligned, the 16-byte path
SHAPES = [(2, 2), (8, 8), (18, 34), (20, 20), (50, 38), (144, 48), (400, 80), (64, 48)]
SUM_SENTINEL, MAP_SENTINEL = -0x2152411021524111, -0x54545455


def windows_of(w, h):
    return [max(0, (pw >> 2) - 1) * max(0, (ph >> 2) - 1) for pw, ph in plane_dims(w, h)]


def mb_dims(pw, ph):
    return pad16(pw) // 16, pad16(ph) // 16


def window_counts(w, h):
    """windows per macroblock, int64 [total_blocks]: those whose top-left pixel lies in the macroblock"""
    out = []
    for pw, ph in plane_dims(w, h):
        mw, mh = mb_dims(pw, ph)
        cnt = np.zeros((mh, mw), dtype=np.int64)
        by, bx = np.mgrid[0:max(0, (ph >> 2) - 1), 0:max(0, (pw >> 2) - 1)]
        np.add.at(cnt, (by.reshape(-1) >> 2, bx.reshape(-1) >> 2), 1)
        out.append(cnt.reshape(-1))
    return np.concatenate(out)


def ref_plane(pa, pb):
    """float64 window values of one plane, shape (bh - 1, bw - 1) (possibly empty)"""
    ph, pw = pa.shape
    bw, bh = pw >> 2, ph >> 2
    if bw < 2 or bh < 2:
        return np.zeros((max(0, bh - 1), max(0, bw - 1)))
    a = pa[:4 * bh, :4 * bw].astype(np.int64)
    b = pb[:4 * bh, :4 * bw].astype(np.int64)

    def win(x):
        blk = x.reshape(bh, 4, bw, 4).sum(axis=(1, 3))
        return blk[:-1, :-1] + blk[:-1, 1:] + blk[1:, :-1] + blk[1:, 1:]
    s1, s2, ss, s12 = win(a), win(b), win(a * a + b * b), win(a * b)
    vars_ = 64 * ss - s1 * s1 - s2 * s2
    covar = 64 * s12 - s1 * s2
    n1, n2, d1, d2 = 2 * s1 * s2 + C1, 2 * covar + C2, s1 * s1 + s2 * s2 + C1, vars_ + C2
    assert max(np.abs(x).max() for x in (n1, n2, d1, d2)) < 2 ** 30 and d1.min() > 0 and d2.min() > 0
    return (n1.astype(np.float64) * n2.astype(np.float64)) / (d1.astype(np.float64) * d2.astype(np.float64))


def ref_ssim(a, b, w, h):
    """numpy reference on packed frames, in units of 2^-24: (sums float64 [3], map float64 [total_blocks])"""
    sums, maps = [], []
    for pa, pb, (pw, ph) in zip(planes_of(a, w, h), planes_of(b, w, h), plane_dims(w, h)):
        v = ref_plane(pa, pb) * ONE
        sums.append(float(v.sum()))
        mw, mh = mb_dims(pw, ph)
        m = np.zeros((mh, mw))
        if v.size:
            by, bx = np.mgrid[0:v.shape[0], 0:v.shape[1]]
            np.add.at(m, (by.reshape(-1) >> 2, bx.reshape(-1) >> 2), v.reshape(-1))
        maps.append(m.reshape(-1))
    return np.array(sums), np.concatenate(maps)


def ref_ssim_many(a, b, w, h):
    r = [ref_ssim(x, y, w, h) for x, y in zip(a, b)]
    return np.stack([s for s, _ in r]), np.stack([m for _, m in r])


def assert_close(sums, mb, want_sums, want_map, w, h, what=""):
    """the derived tolerance, printed figures first; and the exact relation plane sum == sum of its map entries"""
    sums, want_sums = np.atleast_2d(sums), np.atleast_2d(want_sums)
    nw = np.array(windows_of(w, h), dtype=np.float64)
    err = np.abs(sums.astype(np.float64) - want_sums)
    print(f"ssim {what} {w}x{h}: worst plane-sum error per window {np.max(err / np.maximum(nw, 1)):.3f} (bound {TOL})")
    assert (err <= TOL * nw).all(), (what, sums, want_sums)
    if mb is not None:
        mb, want_map = np.atleast_2d(mb), np.atleast_2d(want_map)
        cnt = window_counts(w, h)
        merr = np.abs(mb.astype(np.float64) - want_map)
        print(f"ssim {what} {w}x{h}: worst map error per window {np.max(merr / np.maximum(cnt, 1)):.3f} (bound {TOL})")
        assert (merr <= TOL * cnt).all(), what
        assert_map_sums(sums, mb, w, h)


def assert_map_sums(sums, mb, w, h):
    off = 0
    for p, (pw, ph) in enumerate(plane_dims(w, h)):
        mw, mh = mb_dims(pw, ph)
        assert np.array_equal(mb[:, off:off + mw * mh].astype(np.int64).sum(axis=1), sums[:, p].astype(np.int64)), p
        off += mw * mh
    assert off == mb.shape[1]


def ssim_dev(pkg, ctx, w, h, n, a_buf, a_layout, a_stride, b_buf, b_layout, b_stride, with_map=True, same=False):
    """pfv_frames_ssim_dev on uploaded operands -> (sums int64 [n, 3], map int32 [n, total_blocks] or None); the outputs are preset with a
    sentinel, so an entry the kernels do not write shows"""
    bufs = DevBufs(ctx)
    try:
        a_dev = bufs.put(a_buf)
        b_dev = a_dev if same else bufs.put(b_buf)
        sums = np.full((n, 3), SUM_SENTINEL, dtype=np.int64)
        mb = np.full((n, total_blocks(w, h)), MAP_SENTINEL, dtype=np.int32)
        sums_d = bufs.put(sums)
        mb_d = bufs.put(mb) if with_map else 0
        rc = ctx._lib.pfv_frames_ssim_dev(ctx.handle, w, h, n, ctypes.c_void_p(a_dev), a_layout, a_stride, ctypes.c_void_p(b_dev), b_layout, b_stride,
                                          ctypes.c_void_p(sums_d), ctypes.c_void_p(mb_d))
        ctx.check(rc)
        ctx.download(sums, sums_d)
        if with_map:
            ctx.download(mb, mb_d)
        return sums, (mb if with_map else None)
    finally:
        bufs.close()


def all_layouts(pkg, ctx, w, h, a, b, rng, what):
    """the four layout pairs on one pair of packed frames: every result inside the tolerance, and all four EQUAL"""
    want_sums, want_map = ref_ssim(a, b, w, h)
    forms = {PACKED: (a, b), PADDED: (to_padded(a, w, h, rng), to_padded(b, w, h, rng))}
    first = None
    for la, lb in LAYOUT_PAIRS:
        sums, mb = ssim_dev(pkg, ctx, w, h, 1, forms[la][0], la, 0, forms[lb][1], lb, 0)
        assert_close(sums, mb, want_sums, want_map, w, h, f"{what} layouts {la}{lb}")
        if first is None:
            first = (sums, mb)
        assert np.array_equal(sums, first[0]) and np.array_equal(mb, first[1]), (la, lb)
    return first, forms


# ------------------------------------------------------------------ frames
def check_windows(pkg):
    for w, h in SHAPES + [(1920, 1080), (16, 2), (2, 16), (65534, 4)]:
        assert pkg.ssim_windows(w, h) == tuple(windows_of(w, h)), (w, h)
    assert pkg.ssim_windows(2, 2) == (0, 0, 0) and pkg.ssim_windows(8, 8) == (1, 0, 0) and pkg.ssim_windows(1920, 1080) == (479 * 269, 239 * 134, 239 * 134)
    out = (ctypes.c_uint32 * 3)()
    L = pkg._lib
    for w, h in [(0, 8), (8, 0), (7, 8), (8, 7), (-2, 8), (65536, 8)]:
        assert L.load().pfv_ssim_windows(w, h, out) == L.PFV_ERR_BAD_ARG
    assert L.load().pfv_ssim_windows(8, 8, None) == L.PFV_ERR_BAD_ARG


def check_ssim_value(pkg):
    assert math.isnan(pkg.ssim(0, 0)) and math.isnan(pkg.ssim(5, 0))
    assert pkg.ssim(ONE, 1) == 1.0 and pkg.ssim(-ONE, 1) == -1.0 and pkg.ssim(0, 7) == 0.0 and pkg.ssim(26 * 5, 5) == 26 / ONE
    rng = np.random.default_rng(9)
    for n in rng.integers(1, 2 ** 33, 100):
        q = int(rng.integers(-ONE, ONE + 1)) * int(n)
        assert pkg.ssim(q, int(n)) == q / (float(ONE) * int(n))


def check_plane_shape(pkg, ctx, w, h, seed=1):
    """noise against noise: the four layout pairs, the NULL-map form and the host entry point"""
    rng = np.random.default_rng(seed * 1000 + w * 7 + h)
    a = rng.integers(0, 256, frame_bytes(w, h), dtype=np.uint8)
    b = rng.integers(0, 256, frame_bytes(w, h), dtype=np.uint8)
    (sums, mb), forms = all_layouts(pkg, ctx, w, h, a, b, rng, "noise")
    cnt = window_counts(w, h)
    assert not mb[0][cnt == 0].any()                                                                       # a macroblock without windows gets 0
    only, _ = ssim_dev(pkg, ctx, w, h, 1, a, PACKED, 0, forms[PADDED][1], PADDED, 0, with_map=False)       # map to the context's scratch
    assert np.array_equal(only, sums)
    hs, hm = pkg.frames_ssim(ctx, w, h, a, b, mb_map=True)                                                 # host buffers
    assert hs.dtype == np.int64 and hm.dtype == np.int32 and np.array_equal(hs, sums) and np.array_equal(hm, mb)
    assert np.array_equal(pkg.frames_ssim(ctx, w, h, a, b), sums)
    nw = windows_of(w, h)
    for p in range(3):
        v = pkg.ssim(int(sums[0, p]), nw[p])
        assert math.isnan(v) if nw[p] == 0 else -1.0 <= v <= 1.0
    if (w, h) == (2, 2):
        assert not sums.any() and not mb.any() and all(math.isnan(pkg.ssim(int(s), n)) for s, n in zip(sums[0], nw))


def check_near_copy(pkg, ctx, w, h):
    rng = np.random.default_rng(w * 3 + h)
    a = rng.integers(0, 256, frame_bytes(w, h), dtype=np.uint8)
    b = np.clip(a.astype(np.int16) + rng.integers(-6, 7, a.size), 0, 255).astype(np.uint8)
    (sums, _), _ = all_layouts(pkg, ctx, w, h, a, b, rng, "near-copy")
    nw = windows_of(w, h)
    assert all(0.5 < pkg.ssim(int(s), n) < 1.0 for s, n in zip(sums[0], nw) if n)


def check_checkerboard(pkg, ctx, w, h):
    """a 0/255 checkerboard against its inverse: every window is strongly negative, so signedness is checked on the map, in the plane
    reduction and in the 64-bit sums"""
    parts = []
    for pw, ph in plane_dims(w, h):
        yy, xx = np.mgrid[0:ph, 0:pw]
        parts.append((((xx + yy) & 1) * 255).astype(np.uint8).reshape(-1))
    a = np.concatenate(parts)
    b = 255 - a
    (sums, mb), _ = all_layouts(pkg, ctx, w, h, a, b, np.random.default_rng(3), "checkerboard")
    nw, cnt = windows_of(w, h), window_counts(w, h)
    assert all(int(s) < -0.9 * ONE * n for s, n in zip(sums[0], nw) if n)
    assert (mb[0][cnt > 0] < 0).all()


def check_identical(pkg, ctx, w, h):
    """identical operands -- the same buffer, two copies, packed against padded with random padding: every window is exactly 2^24"""
    rng = np.random.default_rng(w + h)
    a = rng.integers(0, 256, (2, frame_bytes(w, h)), dtype=np.uint8)
    want_sums = np.array([windows_of(w, h)] * 2, dtype=np.int64) * ONE
    want_map = np.stack([window_counts(w, h)] * 2) * ONE
    sums, mb = ssim_dev(pkg, ctx, w, h, 2, a, PACKED, 0, a, PACKED, 0, same=True)
    assert np.array_equal(sums, want_sums) and np.array_equal(mb, want_map)
    pa = np.stack([to_padded(x, w, h, rng) for x in a])
    pb = np.stack([to_padded(x, w, h, rng) for x in a])
    for (la, fa), (lb, fb) in (((PACKED, a), (PACKED, a.copy())), ((PACKED, a), (PADDED, pb)), ((PADDED, pa), (PACKED, a)), ((PADDED, pa), (PADDED, pb))):
        sums, mb = ssim_dev(pkg, ctx, w, h, 2, fa, la, 0, fb, lb, 0)
        assert np.array_equal(sums, want_sums) and np.array_equal(mb, want_map), (la, lb)
    sums, mb = pkg.frames_ssim(ctx, w, h, a, a, mb_map=True)
    assert np.array_equal(sums, want_sums) and np.array_equal(mb, want_map)


def check_extremes(pkg, ctx, w=50, h=38):
    """all 0 against all 255: s1 = 0, s2 = 16 320, vars = covar = 0, so ssim = 416 / (16 320^2 + 416) and every window has q == 26"""
    a = np.zeros(frame_bytes(w, h), dtype=np.uint8)
    b = np.full(frame_bytes(w, h), 255, dtype=np.uint8)
    assert round(416 / (16320 ** 2 + 416) * ONE) == 26
    rng = np.random.default_rng(5)
    for la, lb in LAYOUT_PAIRS:
        fa = a if la == PACKED else to_padded(a, w, h, rng)
        fb = b if lb == PACKED else to_padded(b, w, h, rng)
        for x, y in ((fa, fb), (fb, fa)) if la == lb else ((fa, fb),):
            sums, mb = ssim_dev(pkg, ctx, w, h, 1, x, la, 0, y, lb, 0)
            assert np.array_equal(sums[0], np.array(windows_of(w, h)) * 26) and np.array_equal(mb[0], window_counts(w, h) * 26)


def check_strided_streams(pkg, ctx, w, h, seed=2):
    """three streams, each operand with a stride larger than its frame (one stride keeps 16-byte alignment, the other breaks it); the
    gaps hold random bytes"""
    rng = np.random.default_rng(seed + w)
    n = 3
    a = rng.integers(0, 256, (n, frame_bytes(w, h)), dtype=np.uint8)
    b = np.clip(a.astype(np.int16) + rng.integers(-40, 41, a.shape), 0, 255).astype(np.uint8)
    want_sums, want_map = ref_ssim_many(a, b, w, h)
    first = None
    for la, lb in LAYOUT_PAIRS:
        fa = a if la == PACKED else np.stack([to_padded(x, w, h, rng) for x in a])
        fb = b if lb == PACKED else np.stack([to_padded(x, w, h, rng) for x in b])
        sa, sb = pad16(fa.shape[1]) + 48, fb.shape[1] + 5
        ba, bb = rng.integers(0, 256, (n, sa), dtype=np.uint8), rng.integers(0, 256, (n, sb), dtype=np.uint8)
        ba[:, :fa.shape[1]] = fa
        bb[:, :fb.shape[1]] = fb
        sums, mb = ssim_dev(pkg, ctx, w, h, n, ba, la, sa, bb, lb, sb)
        assert_close(sums, mb, want_sums, want_map, w, h, f"strided {la}{lb}")
        first = first or (sums, mb)
        assert np.array_equal(sums, first[0]) and np.array_equal(mb, first[1])
    sums, mb = pkg.frames_ssim(ctx, w, h, a, b, mb_map=True)
    assert np.array_equal(sums, first[0]) and np.array_equal(mb, first[1])


def check_single_pixel(pkg, ctx, w, h, px, py):
    """a == b except ONE luma pixel: exactly the macroblocks that own a window over that pixel differ from their identical-frames value.
    (16, 5): the fifth block column comes from the neighbouring macroblock's lanes; (128, 5): from the extra load at the end of a strip,
    and the first column of the next strip; (5, 16): the fifth block row comes from the strip below; the bottom-right pixel of a plane
    whose width and height are no multiples of 4 belongs to no block: nothing differs."""
    rng = np.random.default_rng(px * 31 + py)
    a = rng.integers(0, 256, frame_bytes(w, h), dtype=np.uint8)
    b = a.copy()
    b[py * w + px] ^= 0x80
    bw, bh = w >> 2, h >> 2
    mw, _ = mb_dims(w, h)
    owners = set()
    if (px >> 2) < bw and (py >> 2) < bh:
        for bx in ((px >> 2) - 1, px >> 2):
            for by in ((py >> 2) - 1, py >> 2):
                if 0 <= bx < bw - 1 and 0 <= by < bh - 1:
                    owners.add((by >> 2) * mw + (bx >> 2))
    want_sums, want_map = ref_ssim(a, b, w, h)
    same = window_counts(w, h) * ONE
    assert set(np.flatnonzero(np.abs(want_map - same) > 1000)) == owners        # the reference agrees with the geometry, by a wide margin
    for la, lb in LAYOUT_PAIRS:
        fa = a if la == PACKED else to_padded(a, w, h, rng)
        fb = b if lb == PACKED else to_padded(b, w, h, rng)
        sums, mb = ssim_dev(pkg, ctx, w, h, 1, fa, la, 0, fb, lb, 0)
        assert set(np.flatnonzero(mb[0] != same)) == owners, (la, lb, px, py, np.flatnonzero(mb[0] != same), owners)
        assert_close(sums, mb, want_sums, want_map, w, h, f"pixel ({px},{py}) {la}{lb}")
    return owners


def check_bad_arguments(pkg, ctx):
    L = pkg._lib
    lib = ctx._lib
    w, h = 16, 16
    bufs = DevBufs(ctx)
    try:
        a = bufs.put(np.zeros(2 * padded_frame_bytes(w, h), dtype=np.uint8))
        out = bufs.put(np.zeros(6, dtype=np.int64))
        P = ctypes.c_void_p

        def call(w=w, h=h, n=1, a=a, la=PACKED, sa=0, b=a, lb=PACKED, sb=0, out=out):
            return lib.pfv_frames_ssim_dev(ctx.handle, w, h, n, P(a), la, sa, P(b), lb, sb, P(out), None)
        assert call() == L.PFV_OK
        assert call(w=15) == L.PFV_ERR_BAD_ARG and call(h=17) == L.PFV_ERR_BAD_ARG and call(w=0) == L.PFV_ERR_BAD_ARG and call(h=-2) == L.PFV_ERR_BAD_ARG
        assert call(n=0) == L.PFV_ERR_BAD_ARG and call(n=-1) == L.PFV_ERR_BAD_ARG
        assert call(la=2) == L.PFV_ERR_BAD_ARG and call(lb=2) == L.PFV_ERR_BAD_ARG and call(la=-1) == L.PFV_ERR_BAD_ARG
        assert call(sa=frame_bytes(w, h) - 1) == L.PFV_ERR_BAD_ARG and call(sb=frame_bytes(w, h) - 1) == L.PFV_ERR_BAD_ARG
        assert call(lb=PADDED, sb=padded_frame_bytes(w, h) - 1) == L.PFV_ERR_BAD_ARG      # enough for a packed frame, not for a padded one
        assert call(sa=frame_bytes(w, h), lb=PADDED, sb=padded_frame_bytes(w, h)) == L.PFV_OK
        assert call(a=None) == L.PFV_ERR_BAD_ARG and call(b=None) == L.PFV_ERR_BAD_ARG and call(out=None) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_ssim_dev(None, w, h, 1, P(a), 0, 0, P(a), 0, 0, P(out), None) == L.PFV_ERR_BAD_ARG
        host = np.zeros(frame_bytes(w, h), dtype=np.uint8)
        res = np.zeros(3, dtype=np.int64)
        hp = lambda x: x.ctypes.data_as(P)      # noqa: E731
        assert lib.pfv_frames_ssim(ctx.handle, w, h, 1, hp(host), hp(host), hp(res), None) == L.PFV_OK
        assert lib.pfv_frames_ssim(ctx.handle, 15, h, 1, hp(host), hp(host), hp(res), None) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_ssim(ctx.handle, w, h, 0, hp(host), hp(host), hp(res), None) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_ssim(ctx.handle, w, h, 1, None, hp(host), hp(res), None) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_ssim(ctx.handle, w, h, 1, hp(host), None, hp(res), None) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_ssim(ctx.handle, w, h, 1, hp(host), hp(host), None, None) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_enc_ssim_dev(None, P(a), P(out), None) == L.PFV_ERR_BAD_ARG and lib.pfv_dec_ssim_dev(None, P(a), P(out), None) == L.PFV_ERR_BAD_ARG
        enc = pkg.EncoderSession(ctx, w, h, 5, 1)
        try:
            assert lib.pfv_enc_ssim_dev(enc.handle, None, P(out), None) == L.PFV_ERR_BAD_ARG
            assert lib.pfv_enc_ssim_dev(enc.handle, P(a), None, None) == L.PFV_ERR_BAD_ARG
        finally:
            enc.close()
        assert lib.pfv_encoder_set_frame_ssim(None, 1) == L.PFV_ERR_BAD_ARG and lib.pfv_encoder_frame_ssim(None, None) == L.PFV_ERR_BAD_ARG
        ctx.sync()
    finally:
        bufs.close()


# ------------------------------------------------------------------ sessions
def check_enc_session(pkg, ctx, oracle, w=64, h=48, quality=5, n=2):
    """i-frame, then two p-frames: after each step ssim is inside the tolerance of numpy's value between the input frames and the ORACLE's
    reconstruction"""
    streams = [pkg.SyntheticStream(w, h, seed=11 + k) for k in range(n)]
    oenc = [oracle.encoder(w, h, quality) for _ in range(n)]
    enc = pkg.EncoderSession(ctx, w, h, quality, n)
    try:
        for t in range(3):
            frames = np.stack([s.frame(t) for s in streams])
            if t == 0:
                enc.encode_iframe(frames)
                [o.encode_iframe(f) for o, f in zip(oenc, frames)]
            else:
                enc.encode_pframe(frames)
                [o.encode_pframe(f) for o, f in zip(oenc, frames)]
            recon = np.stack([crop(o.prev_frame(), w, h) for o in oenc])
            want_sums, want_map = ref_ssim_many(frames, recon, w, h)
            assert (want_sums[:, 0] < 0.9999 * ONE * windows_of(w, h)[0]).all()        # quality 5 is lossy: the check is not 1 == 1
            sums, mb = enc.ssim(frames, mb_map=True)
            assert sums.dtype == np.int64 and sums.shape == (n, 3) and mb.dtype == np.int32
            assert_close(sums, mb, want_sums, want_map, w, h, f"enc session t={t}")
            assert np.array_equal(enc.ssim(frames), sums)                               # map to the session's scratch
    finally:
        enc.close()


def check_enc_session_window(pkg, ctx, oracle, w=64, h=48, quality=5):
    """a window of 1 slot out of 3: the slot's numbers are the oracle's, the other slots' entries keep what they held"""
    n, slot = 3, 1
    streams = [pkg.SyntheticStream(w, h, seed=21 + k) for k in range(n)]
    oenc = [oracle.encoder(w, h, quality) for _ in range(n)]
    enc = pkg.EncoderSession(ctx, w, h, quality, n)
    bufs = DevBufs(ctx)
    try:
        f0 = np.stack([s.frame(0) for s in streams])
        enc.encode_iframe(f0)
        [o.encode_iframe(f) for o, f in zip(oenc, f0)]
        f1 = np.stack([s.frame(1) for s in streams])
        tb = enc.total_blocks
        frames_dev = bufs.put(f1)
        mv, has, coef = bufs.put(np.zeros(n * tb * 2, np.int8)), bufs.put(np.zeros(n * tb, np.uint8)), bufs.put(np.zeros(n * tb * 256, np.int16))
        enc.set_window(slot, 1)
        enc.encode_pframe_dev(frames_dev, mv, has, coef)
        oenc[slot].encode_pframe(f1[slot])
        want_sums, want_map = ref_ssim(f1[slot], crop(oenc[slot].prev_frame(), w, h), w, h)
        sent = np.full((n, 3), SUM_SENTINEL, dtype=np.int64)
        sent_map = np.full((n, tb), MAP_SENTINEL, dtype=np.int32)
        for frames in (f1, frames_dev):                                  # an array (uploaded) and a device address
            sums, mb = enc.ssim(frames, mb_map=True, out=sent, out_map=sent_map)
            assert_close(sums[slot], mb[slot], want_sums, want_map, w, h, "enc window")
            for k in (0, 2):
                assert np.array_equal(sums[k], sent[k]) and np.array_equal(mb[k], sent_map[k])
        only = enc.ssim(f1, out=sent)
        assert np.array_equal(only[slot], sums[slot]) and np.array_equal(only[[0, 2]], sent[[0, 2]])
    finally:
        bufs.close()
        enc.close()


def check_enc_session_stride(pkg, ctx, oracle, w=64, h=48, quality=5):
    """input frames 2.5 frames apart (an unaligned stride), random bytes between them"""
    n = 2
    fb = frame_bytes(w, h)
    stride = 2 * fb + fb // 2 + 3
    rng = np.random.default_rng(31)
    streams = [pkg.SyntheticStream(w, h, seed=31 + k) for k in range(n)]
    oenc = [oracle.encoder(w, h, quality) for _ in range(n)]
    enc = pkg.EncoderSession(ctx, w, h, quality, n)
    bufs = DevBufs(ctx)
    try:
        frames = np.stack([s.frame(0) for s in streams])
        laid = rng.integers(0, 256, (n, stride), dtype=np.uint8)
        laid[:, :fb] = frames
        frames_dev = bufs.put(laid)
        coef = bufs.put(np.zeros(n * enc.total_blocks * 256, np.int16))
        enc.set_frame_stride(stride)
        enc.encode_iframe_dev(frames_dev, coef)
        [o.encode_iframe(f) for o, f in zip(oenc, frames)]
        want_sums, want_map = ref_ssim_many(frames, np.stack([crop(o.prev_frame(), w, h) for o in oenc]), w, h)
        for src in (laid, frames_dev):
            sums, mb = enc.ssim(src, mb_map=True)
            assert_close(sums, mb, want_sums, want_map, w, h, "enc stride")
    finally:
        bufs.close()
        enc.close()


def check_dec_session(pkg, ctx, oracle, w=64, h=48, quality=5, n=2):
    """DecoderSession.ssim after decoding the ORACLE's coefficients, against the oracle decoder's framebuffer"""
    from oracle_bind import OracleDecoder
    tabs = np.stack(oracle.qtables(quality)[:4])
    streams = [pkg.SyntheticStream(w, h, seed=41 + k) for k in range(n)]
    oenc = [oracle.encoder(w, h, quality) for _ in range(n)]
    odec = [OracleDecoder(oracle, w, h, tabs) for _ in range(n)]
    dec = pkg.DecoderSession(ctx, w, h, tabs, n)
    try:
        for t in range(3):
            frames = np.stack([s.frame(t) for s in streams])
            if t == 0:
                coef = np.stack([o.encode_iframe(f) for o, f in zip(oenc, frames)])
                dec.decode_iframe(coef)
                [d.decode_iframe(c) for d, c in zip(odec, coef)]
            else:
                parts = [o.encode_pframe(f) for o, f in zip(oenc, frames)]
                mv, has, coef = (np.stack([p[i] for p in parts]) for i in range(3))
                dec.decode_pframe(mv, has, coef)
                [d.decode_pframe(*p) for d, p in zip(odec, parts)]
            want_sums, want_map = ref_ssim_many(frames, np.stack([crop(d.framebuffer(), w, h) for d in odec]), w, h)
            sums, mb = dec.ssim(frames, mb_map=True)
            assert_close(sums, mb, want_sums, want_map, w, h, f"dec session t={t}")
            assert np.array_equal(dec.ssim(frames), sums)
        dec.set_window(1, 1)
        sent = np.full((n, 3), SUM_SENTINEL, dtype=np.int64)
        only = dec.ssim(frames, out=sent)
        assert np.array_equal(only[1], sums[1]) and np.array_equal(only[0], sent[0])
    finally:
        dec.close()


def check_graph(pkg, ctx, oracle, w=64, h=48, quality=5, n=2):
    """pfv_enc_iframe_dev + pfv_enc_ssim_dev recorded in one graph and replayed twice == the unrecorded calls, bit for bit; a NULL map
    that would need an allocation inside a recording is refused"""
    streams = [pkg.SyntheticStream(w, h, seed=51 + k) for k in range(n)]
    frames = np.stack([s.frame(0) for s in streams])
    oenc = [oracle.encoder(w, h, quality) for _ in range(n)]
    [o.encode_iframe(f) for o, f in zip(oenc, frames)]
    want_sums, want_map = ref_ssim_many(frames, np.stack([crop(o.prev_frame(), w, h) for o in oenc]), w, h)
    enc = pkg.EncoderSession(ctx, w, h, quality, n)
    enc2 = pkg.EncoderSession(ctx, w, h, quality, n)
    bufs = DevBufs(ctx)
    graph = pkg.Graph(ctx)
    try:
        tb = enc.total_blocks
        frames_dev, coef = bufs.put(frames), bufs.put(np.zeros(n * tb * 256, np.int16))
        sums_d, map_d = bufs.put(np.zeros((n, 3), np.int64)), bufs.put(np.zeros((n, tb), np.int32))
        enc.encode_iframe_dev(frames_dev, coef)                        # the unrecorded calls
        enc.ssim_dev(frames_dev, sums_d, map_d)
        plain_sums, plain_map = np.zeros((n, 3), np.int64), np.zeros((n, tb), np.int32)
        ctx.download(plain_sums, sums_d)
        ctx.download(plain_map, map_d)
        assert_close(plain_sums, plain_map, want_sums, want_map, w, h, "graph, unrecorded")
        with graph:
            enc.encode_iframe_dev(frames_dev, coef)
            enc.ssim_dev(frames_dev, sums_d, map_d)
            enc2.encode_iframe_dev(frames_dev, coef)
            with pytest.raises(pkg.PfvError) as e:                     # enc2 has never measured: its map would have to be allocated now
                enc2.ssim_dev(frames_dev, sums_d, 0)
            assert e.value.code == pkg._lib.PFV_ERR_STATE and "map buffer" in str(e.value) and "before" in str(e.value)
        for _ in range(2):
            ctx.upload(sums_d, np.full((n, 3), SUM_SENTINEL, np.int64))    # a replay recomputes everything: nothing is accumulated or cleared
            ctx.upload(map_d, np.full((n, tb), MAP_SENTINEL, np.int32))
            graph.launch()
            got_sums, got_map = np.zeros((n, 3), np.int64), np.zeros((n, tb), np.int32)
            ctx.download(got_sums, sums_d)
            ctx.download(got_map, map_d)
            assert np.array_equal(got_sums, plain_sums) and np.array_equal(got_map, plain_map)
    finally:
        graph.close()
        bufs.close()
        enc.close()
        enc2.close()


# ------------------------------------------------------------------ pfv_encoder's frame SSIM
def encode_with_ssim(pkg, ctx, w, h, quality, frames, plan, device_entropy, frame_ssim=True):
    import io
    buf = io.BytesIO()
    enc = pkg.Encoder(buf, w, h, 30, quality, ctx, device_entropy=device_entropy, frame_ssim=frame_ssim)
    out = []
    try:
        with pytest.raises(pkg.PfvError) as e:           # before any frame; or the switch off
            enc.last_ssim
        assert e.value.code == pkg._lib.PFV_ERR_STATE
        with pytest.raises(pkg.PfvError) as e:           # the frame reports are a switch of their own, and it is off
            enc.last_report
        assert e.value.code == pkg._lib.PFV_ERR_STATE
        for f, kind in zip(frames, plan):
            if kind == "D":
                enc.encode_dropframe()
            elif kind == "I":
                enc.encode_iframe(pkg.VideoFrame.from_packed(w, h, f))
            else:
                enc.encode_pframe(pkg.VideoFrame.from_packed(w, h, f))
            if frame_ssim:
                out.append(enc.last_ssim)
            else:
                with pytest.raises(pkg.PfvError) as e:
                    enc.last_ssim
                assert e.value.code == pkg._lib.PFV_ERR_STATE
        enc.finish()
    finally:
        enc.close()
    return buf.getvalue(), out


def check_encoder_ssim(pkg, ctx, oracle, device_entropy, w=48, h=32, quality=5, n_frames=5, gop=3, drop_at=2):
    from oracle_bind import OracleStreamEncoder
    st = pkg.SyntheticStream(w, h)
    frames = [st.frame(t) for t in range(n_frames)]
    plan = qc.clip_plan(n_frames, gop, drop_at)
    data, got = encode_with_ssim(pkg, ctx, w, h, quality, frames, plan, device_entropy)
    oenc = OracleStreamEncoder(oracle, w, h, 30, quality)
    for f, kind in zip(frames, plan):
        {"D": lambda f: oenc.encode_dropframe(), "I": oenc.encode_iframe, "P": oenc.encode_pframe}[kind](f)
    oenc.finish()
    assert data == oenc.bytes(), "stream bytes with frame SSIM on differ from the oracle encoder's"
    plain, none = encode_with_ssim(pkg, ctx, w, h, quality, frames, plan, device_entropy, frame_ssim=False)
    assert plain == data and none == [], "stream bytes with frame SSIM on differ from the bytes with it off"
    decoded = qc.oracle_decode(oracle, data)
    assert len(got) == n_frames == len(decoded)
    nw = windows_of(w, h)
    for t, (r, kind, f, shown) in enumerate(zip(got, plan, frames, decoded)):
        assert r.windows == tuple(nw)
        if kind == "D":
            assert r.q24 == (0, 0, 0) and not any(math.isnan(v) for v in r.ssim + (r.ssim_all,))
            continue
        want_sums, _ = ref_ssim(f, shown, w, h)
        assert_close(np.array(r.q24, dtype=np.int64), None, want_sums, None, w, h, f"encoder frame {t}")
        assert r.q24[0] < nw[0] * ONE
        for p in range(3):
            assert r.ssim[p] == pkg.ssim(r.q24[p], nw[p])
        assert r.ssim_all == pkg.ssim(sum(r.q24), sum(nw))
    return got


def check_encoder_ssim_with_reports(pkg, ctx, w=48, h=32, quality=5):
    """both switches on: each keeps its own numbers, and they are those of the switches alone"""
    import io
    st = pkg.SyntheticStream(w, h)
    frames = [st.frame(t) for t in range(3)]
    plan = ["I", "P", "P"]
    _, alone = encode_with_ssim(pkg, ctx, w, h, quality, frames, plan, True)
    _, reports = qc.encode_with_reports(pkg, ctx, w, h, quality, frames, plan, True)
    enc = pkg.Encoder(io.BytesIO(), w, h, 30, quality, ctx, frame_report=True, frame_ssim=True)
    try:
        for f, kind, s, r in zip(frames, plan, alone, reports):
            (enc.encode_iframe if kind == "I" else enc.encode_pframe)(pkg.VideoFrame.from_packed(w, h, f))
            assert enc.last_ssim == s and enc.last_report == r
        enc.finish()
    finally:
        enc.close()


# ------------------------------------------------------------------ C++ mirror and tool
def build_cpp(lib_path, exe):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "ssim_report.cpp"), "-o", exe, lib_path, "-Wl,-rpath," + os.path.dirname(lib_path)], check=True)


def check_cpp_ssim(pkg, ctx, exe, tmp_path, w=48, h=32, quality=5, n_frames=4, gop=3, drop_at=-1):
    """tests/cpp/ssim_report.cpp (pfv::Encoder::set_frame_ssim / last_ssim, pfv::ssim, pfv::ssim_windows) prints what the Python Encoder
    reports for the same clip"""
    st = pkg.SyntheticStream(w, h)
    frames = [st.frame(t) for t in range(n_frames)]
    yuv = str(tmp_path / "in.yuv")
    np.concatenate(frames).tofile(yuv)
    nw = windows_of(w, h)
    for device_entropy in (1, 0):
        data, got = encode_with_ssim(pkg, ctx, w, h, quality, frames, qc.clip_plan(n_frames, gop, drop_at), bool(device_entropy))
        r = subprocess.run([exe, str(w), str(h), str(quality), str(gop), str(drop_at), str(device_entropy), yuv], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        assert len(lines) == n_frames + 2 and lines[-1] == f"stream {len(data)} bytes"
        assert lines[0].split() == ["windows"] + [str(x) for x in nw]
        for t, (line, rep) in enumerate(zip(lines[1:], got)):
            tok = line.split()
            assert tok[0] == "frame" and int(tok[1]) == t and tok[2] == "q24" and tuple(int(x) for x in tok[3:6]) == rep.q24
            assert tok[6] == "windows" and tuple(int(x) for x in tok[7:10]) == rep.windows
            assert tok[10] == "ssim" and tuple(float(x) for x in tok[11:14]) == rep.ssim
            assert tok[14] == "all" and float(tok[15]) == rep.ssim_all == float(tok[16])


def check_rd_tool(pkg, oracle, lib_path, w=64, h=48, n_frames=6, gop=3, qualities=(0, 5, 10)):
    """tools/rd_curve.py --ssim on the library at lib_path: ssim_y / _u / _v / _all are numpy's means over the frames the oracle decoder
    shows; without the flag the lines are the same without those four keys"""
    from oracle_bind import OracleStreamEncoder
    env = dict(os.environ)
    if lib_path:
        env["PFV_HIP_LIB"] = lib_path
    cmd = [sys.executable, os.path.join(ROOT, "tools", "rd_curve.py"), str(w), str(h), str(n_frames), "--gop", str(gop),
           "--qualities", ",".join(str(q) for q in qualities)]
    plain = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert plain.returncode == 0, plain.stderr
    r = subprocess.run(cmd + ["--ssim"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr
    lines = [json.loads(x) for x in r.stdout.splitlines()]
    keys = ("ssim_y", "ssim_u", "ssim_v", "ssim_all")
    stripped = [{k: v for k, v in d.items() if k not in keys} for d in lines]
    assert [json.dumps(d) for d in stripped] == plain.stdout.splitlines(), "rd_curve.py without --ssim does not print the same lines minus the SSIM keys"
    assert all(not any(k in json.loads(x) for k in keys) for x in plain.stdout.splitlines())
    assert [d["quality"] for d in lines] == list(qualities)
    st = pkg.SyntheticStream(w, h)
    frames = [st.frame(t) for t in range(n_frames)]
    nw = np.array(windows_of(w, h), dtype=np.float64)
    for d in lines:
        oenc = OracleStreamEncoder(oracle, w, h, 30, d["quality"])
        for t, f in enumerate(frames):
            (oenc.encode_iframe if t % gop == 0 else oenc.encode_pframe)(f)
        oenc.finish()
        assert d["stream_bytes"] == len(oenc.bytes())
        sums = np.array([ref_ssim(f, shown, w, h)[0] for f, shown in zip(frames, qc.oracle_decode(oracle, oenc.bytes()))])
        want = list(np.mean(sums / (ONE * nw), axis=0)) + [float(np.mean(sums.sum(axis=1) / (ONE * nw.sum())))]
        for key, val in zip(keys, want):
            assert abs(d[key] - val) <= TOL / ONE, (key, d[key], val)      # a mean of per-window means: the per-window bound
    return lines
