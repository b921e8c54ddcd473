"""Shared checks of the frame resize (include/pfv_hip_ext.h, "frame resize"; k_scale), driven on the CPU emulator by tests/test_emu_scale.py
and on a real MI355X by tests/test_gpu_scale.py through the same fixtures.

The reference is the numpy restatement of the header's arithmetic below: `np_table` builds an axis table from the text, `ref_frame` filters a
frame with tables.  Table checks compare the library's tables with `np_table`; every PIXEL check is an EQUALITY between the library's frames
and `ref_frame` run on the tables the library returned.  Destinations are filled with a sentinel first, and every byte between and beyond
the destination frames must still hold it afterwards."""
import ctypes
import io
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import quality_cases as qc
from quality_cases import PACKED, PADDED, DevBufs, frame_bytes, pad16, padded_frame_bytes, plane_dims, planes_of

ROOT = qc.ROOT
KINDS = {"bilinear": 0, "bicubic": 1, "lanczos3": 2}
SUPPORT = {0: 1, 1: 2, 2: 3}
# identity; non-integer upscale; every tap clamped; ratio 8 (T = 16 / 32 / 48); crosses a tile edge, a width that fills no dword (chroma
# 33); the 3:2 ladder step; 256 -> 18 is a reduction of 14.2, beyond the ratio limit: that shape must be REFUSED, and 144x16 -> 18x130 (ratio 8 on
# x, up 8.1 on y, nine tile rows) is what covers down on one axis and up on the other; the u16 limit
SHAPES = [(16, 16, 16, 16), (18, 10, 34, 22), (2, 2, 64, 64), (64, 48, 8, 6), (130, 34, 66, 18), (144, 80, 96, 54), (256, 16, 18, 130),
          (144, 16, 18, 130), (65534, 2, 8192, 2)]
SENTINEL = 0xA5
GUARD = 64
P = ctypes.c_void_p


# ------------------------------------------------------------------ the header's arithmetic in numpy
def np_kernel(kind, t):
    a = abs(t)
    if kind == 0:
        return max(0.0, 1.0 - a)
    if kind == 1:
        if a < 1:
            return (1.5 * a - 2.5) * a * a + 1.0
        if a < 2:
            return ((-0.5 * a + 2.5) * a - 4.0) * a + 2.0
        return 0.0
    if a >= 3:
        return 0.0
    if a == 0:
        return 1.0
    x = math.pi * a
    return (math.sin(x) / x) * (math.sin(x / 3.0) / (x / 3.0))


def np_taps(kind, ns, nd):
    s = SUPPORT[kind]
    return 2 * (-(-s * ns // nd)) if ns > nd else 2 * s


def np_first(kind, ns, nd):
    s, m = SUPPORT[kind], max(ns, nd)
    return [((2 * o + 1) * ns - nd - 2 * s * m) // (2 * nd) + 1 for o in range(nd)]          # Python's // floors


def np_table(kind, ns, nd):
    """(first int32 [nd], coef int64 [nd, T]) of one axis"""
    T = np_taps(kind, ns, nd)
    f = ns / nd if ns > nd else 1.0
    first = np_first(kind, ns, nd)
    coef = np.zeros((nd, T), np.int64)
    for o in range(nd):
        c = ((2 * o + 1) * ns - nd) / (2.0 * nd)
        w = [np_kernel(kind, ((first[o] + k) - c) / f) for k in range(T)]
        total = 0.0
        for x in w:                                # the sum in tap order
            total = total + x
        q = np.rint(np.array([x / total * 16384 for x in w])).astype(np.int64)
        q[int(np.argmax(np.abs(q)))] += 16384 - q.sum()
        coef[o] = q
    return np.array(first, np.int32), coef


def ref_plane(src, tx, ty):
    """one plane [sh, sw] uint8 through the tables tx = (first, coef) and ty -> [dh, dw] uint8; indices clamped to the picture"""
    sh, sw = src.shape
    (fx, cx), (fy, cy) = tx, ty
    cx, cy = cx.astype(np.int64), cy.astype(np.int64)
    ix = np.clip(fx.astype(np.int64)[:, None] + np.arange(cx.shape[1])[None, :], 0, sw - 1)
    t = (src.astype(np.int64)[:, ix] * cx[None]).sum(-1)
    assert np.abs(t).max() < 2 ** 31
    t = np.clip((t + 64) >> 7, -32768, 32767)
    iy = np.clip(fy.astype(np.int64)[:, None] + np.arange(cy.shape[1])[None, :], 0, sh - 1)
    o = (t[iy, :] * cy[:, :, None]).sum(1)
    assert np.abs(o).max() < 2 ** 31
    return np.clip((o + (1 << 20)) >> 21, 0, 255).astype(np.uint8)


def lib_tables(pkg, kind, sw, sh, dw, dh):
    """the four tables the library builds for a size pair: (luma x, luma y, chroma x, chroma y)"""
    return [pkg.scale_table(kind, a, b) for a, b in ((sw, dw), (sh, dh), (sw // 2, dw // 2), (sh // 2, dh // 2))]


def ref_frame(frame, sw, sh, tabs):
    """one packed frame through the tables `tabs` (lib_tables) -> the packed destination frame"""
    pl = planes_of(np.ascontiguousarray(frame, dtype=np.uint8).reshape(-1), sw, sh)
    return np.concatenate([ref_plane(pl[0], tabs[0], tabs[1]).reshape(-1)] + [ref_plane(p, tabs[2], tabs[3]).reshape(-1) for p in pl[1:]])


def ref_frames(frames, sw, sh, tabs):
    return np.stack([ref_frame(f, sw, sh, tabs) for f in frames])


def hard_frames(sw, sh, n, rng):
    """random frames whose even rows hold only 0 and 255: ringing kernels overshoot both clamps there"""
    a = rng.integers(0, 256, (n, frame_bytes(sw, sh)), dtype=np.uint8)
    for f in a:
        for pl in planes_of(f, sw, sh):
            pl[::2] = np.where(rng.random(pl[::2].shape) < 0.5, 0, 255)
    return a


# ------------------------------------------------------------------ 1. tables
TABLE_PAIRS = [(16, 16), (18, 34), (9, 17), (1, 32), (2, 64), (64, 8), (24, 3), (130, 66), (65, 33), (144, 96), (80, 54), (40, 27), (144, 18),
               (8, 65), (5, 13), (199, 25), (1000, 999), (999, 1000)]


def check_tables(pkg):
    lib = pkg._lib.load()
    for kind in KINDS.values():
        for ns, nd in TABLE_PAIRS:
            T = np_taps(kind, ns, nd)
            assert lib.pfv_scale_taps(kind, ns, nd) == T, (kind, ns, nd)
            first, coef = pkg.scale_table(kind, ns, nd)
            assert first.dtype == np.int32 and coef.dtype == np.int16 and coef.shape == (nd, T)
            wf, wc = np_table(kind, ns, nd)
            assert np.array_equal(first, wf), (kind, ns, nd, "first")
            assert (coef.astype(np.int64).sum(1) == 16384).all(), (kind, ns, nd, "row sums")
            assert (np.abs(coef.astype(np.int64)).sum(1) < 65536).all()
            if kind == 2:
                assert np.abs(coef.astype(np.int64) - wc).max() <= 1, (kind, ns, nd)
            else:
                assert np.array_equal(coef, wc), (kind, ns, nd, np.argwhere(coef != wc)[:4])
    # a table depends on the ratio and the output index alone: a chroma axis' table is the head of its luma axis' table (which is why handing the
    # chroma planes the luma tables' POINTERS changes nothing; handing them the luma SIZES clamps to the wrong edge, and the pixel checks see it)
    for kind in KINDS.values():
        for ns, nd in ((18, 34), (64, 8), (130, 66), (144, 96)):
            (f, c), (f2, c2) = pkg.scale_table(kind, ns, nd), pkg.scale_table(kind, ns // 2, nd // 2)
            assert np.array_equal(f[:nd // 2], f2) and np.array_equal(c[:nd // 2], c2), (kind, ns, nd)
    # the u16 limit's luma row table, checked where it is cheap: first[] and the sums
    for kind in KINDS.values():
        first, coef = pkg.scale_table(kind, 65534, 8192)
        assert np.array_equal(first, np.array(np_first(kind, 65534, 8192), np.int32)) and (coef.astype(np.int64).sum(1) == 16384).all()
        assert coef.shape[1] == np_taps(kind, 65534, 8192) == (16, 32, 48)[kind]
    # identity tables: one tap of 16384 at the sample itself
    for kind in KINDS.values():
        first, coef = pkg.scale_table(kind, 16, 16)
        k = np.arange(16) - first
        assert (coef[np.arange(16), k] == 16384).all() and (np.abs(coef.astype(np.int64)).sum(1) == 16384).all()
    # T = 0: kinds that do not exist, sizes outside 1 .. 65535, a reduction beyond 8 (ratio 8 itself is legal)
    assert [lib.pfv_scale_taps(k, 64, 8) for k in (0, 1, 2)] == [16, 32, 48]
    for bad in ((3, 16, 16), (-1, 16, 16), (0, 0, 16), (0, 16, 0), (0, -4, 16), (1, 65536, 65536), (1, 16, 65536), (2, 65, 8), (0, 33, 4), (0, 9, 1)):
        assert lib.pfv_scale_taps(*bad) == 0, bad
    buf_f, buf_c = np.zeros(64, np.int32), np.zeros(64 * 48, np.int16)
    ptr = lambda x: x.ctypes.data_as(P)      # noqa: E731
    L = pkg._lib
    assert lib.pfv_scale_table(1, 16, 16, ptr(buf_f), ptr(buf_c)) == L.PFV_OK
    assert lib.pfv_scale_table(1, 16, 16, None, ptr(buf_c)) == L.PFV_ERR_BAD_ARG and lib.pfv_scale_table(1, 16, 16, ptr(buf_f), None) == L.PFV_ERR_BAD_ARG
    assert lib.pfv_scale_table(3, 16, 16, ptr(buf_f), ptr(buf_c)) == L.PFV_ERR_BAD_ARG and lib.pfv_scale_table(1, 65, 8, ptr(buf_f), ptr(buf_c)) == L.PFV_ERR_BAD_ARG
    with pytest.raises(pkg.PfvError):
        pkg.scale_table("bicubic", 66, 8)


# ------------------------------------------------------------------ 2. one launch
def read_frames(raw, at, n, fb, stride):
    """the n frames that start `at` bytes into `raw`, and `raw` with them put back to the sentinel"""
    rest = raw.copy()
    got = np.zeros((n, fb), np.uint8)
    for k in range(n):
        o = at + k * stride
        got[k] = raw[o:o + fb]
        rest[o:o + fb] = SENTINEL
    return got, rest


def scale_dev(ctx, scaler, frames, layout=PACKED, src_off=0, src_gap=0, dst_off=0, dst_stride=0, rng=None):
    """pfv_scaler_run_dev on `frames` ([n, frame bytes of the layout]) -> the n destination frames.  The source lies src_off bytes into its
    allocation with src_gap random bytes between frames; the destination lies GUARD + dst_off bytes into an allocation full of the sentinel,
    which is asserted to survive everywhere outside the frames."""
    frames = np.atleast_2d(frames)
    n, sfb = frames.shape
    rng = rng or np.random.default_rng(7)
    s_stride = sfb + src_gap
    src = rng.integers(0, 256, src_off + n * s_stride + 16, dtype=np.uint8)
    for k in range(n):
        src[src_off + k * s_stride: src_off + k * s_stride + sfb] = frames[k]
    dfb = scaler.dst_frame_bytes
    e_stride = dst_stride or dfb
    dst = np.full(GUARD + dst_off + (n - 1) * e_stride + dfb + GUARD, SENTINEL, dtype=np.uint8)
    bufs = DevBufs(ctx)
    try:
        s_dev, d_dev = bufs.put(src), bufs.put(dst)
        assert s_dev % 16 == 0 and d_dev % 16 == 0
        ctx.check(ctx._lib.pfv_scaler_run_dev(scaler.handle, n, P(s_dev + src_off), layout, s_stride if src_gap else 0, P(d_dev + GUARD + dst_off), dst_stride))
        ctx.download(dst, d_dev)
    finally:
        bufs.close()
    got, rest = read_frames(dst, GUARD + dst_off, n, dfb, e_stride)
    assert (rest == SENTINEL).all(), f"bytes outside the {n} frames were written: {np.flatnonzero(rest != SENTINEL)[:8]}"
    return got


def to_padded_fill(frame, w, h, fill):
    """a padded frame with the same picture and every padding byte = fill"""
    parts = []
    for pl, (pw, ph) in zip(planes_of(frame, w, h), plane_dims(w, h)):
        buf = np.full((pad16(ph), pad16(pw)), fill, dtype=np.uint8)
        buf[:ph, :pw] = pl
        parts.append(buf.reshape(-1))
    return np.concatenate(parts)


def check_shape(pkg, ctx, sw, sh, dw, dh, n=3, seed=1):
    """hard random frames, all three kinds, n streams: tight PACKED (the dword path where the planes' rows are aligned), PADDED with 0xA5 in the
    padding and gaps between source and destination frames, the host form and the Python mirror -- all equal to numpy on the library's
    tables; the identity shape must also equal its source"""
    rng = np.random.default_rng(seed * 1000 + sw * 7 + sh * 3 + dw)
    a = hard_frames(sw, sh, n, rng)
    if sw > 8 * dw or sh > 8 * dh:                   # beyond the ratio limit: refused, nothing written
        for kind in KINDS:
            with pytest.raises(pkg.PfvError) as e:
                pkg.Scaler(ctx, sw, sh, dw, dh, kind)
            assert e.value.code == pkg._lib.PFV_ERR_BAD_ARG
            with pytest.raises(pkg.PfvError) as e:
                pkg.frames_scale(ctx, sw, sh, dw, dh, a, kind)
            assert e.value.code == pkg._lib.PFV_ERR_BAD_ARG
        return
    padded = np.stack([to_padded_fill(f, sw, sh, SENTINEL) for f in a])
    assert padded.shape[1] == padded_frame_bytes(sw, sh)
    dfb = frame_bytes(dw, dh)
    for kind in KINDS:
        want = ref_frames(a, sw, sh, lib_tables(pkg, kind, sw, sh, dw, dh))
        assert want.shape == (n, dfb)
        if (sw, sh) == (dw, dh):
            assert np.array_equal(want, a), (kind, "the identity tables do not reproduce the source")
        with pkg.Scaler(ctx, sw, sh, dw, dh, kind) as sc:
            got = scale_dev(ctx, sc, a, rng=rng)
            assert np.array_equal(got, want), (sw, sh, dw, dh, kind, "packed", np.argwhere(got != want)[:4])
            got = scale_dev(ctx, sc, padded, PADDED, src_gap=48, dst_stride=(dfb + 19) // 16 * 16 + 16, rng=rng)
            assert np.array_equal(got, want), (sw, sh, dw, dh, kind, "padded", np.argwhere(got != want)[:4])
            got = sc.run(a)
            assert np.array_equal(got, want), (kind, "Scaler.run")
        got = pkg.frames_scale(ctx, sw, sh, dw, dh, a, kind)
        assert got.dtype == np.uint8 and got.shape == (n, dfb) and np.array_equal(got, want), (sw, sh, dw, dh, kind, "pfv_frames_scale")


def rows_aligned(w, h, padded=False):
    """the header's rule for the dword path, given an aligned base and stride: every plane's offset and row pitch are multiples of 4"""
    off = 0
    for pw, ph in plane_dims(w, h):
        rw, rh = (pad16(pw), pad16(ph)) if padded else (pw, ph)
        if off % 4 or rw % 4:
            return False
        off += rw * rh
    return True


def check_big(pkg, ctx, frames, sw, sh, dw, dh, kind):
    """many tiles per plane: tight PACKED and PADDED sources whose rows are all aligned (asserted: the dword path), then a source base offset
    by one byte into an odd destination stride (the byte path for every plane) -- each equal to numpy, computed once"""
    want = ref_frames(frames, sw, sh, lib_tables(pkg, kind, sw, sh, dw, dh))
    assert rows_aligned(sw, sh) and rows_aligned(sw, sh, True) and rows_aligned(dw, dh)
    padded = np.stack([to_padded_fill(f, sw, sh, SENTINEL) for f in frames])
    with pkg.Scaler(ctx, sw, sh, dw, dh, kind) as sc:
        got = scale_dev(ctx, sc, frames)
        assert np.array_equal(got, want), (kind, "dword path, packed", np.argwhere(got != want)[:4])
        got = scale_dev(ctx, sc, padded, PADDED)
        assert np.array_equal(got, want), (kind, "dword path, padded", np.argwhere(got != want)[:4])
        got = scale_dev(ctx, sc, frames, src_off=1, dst_stride=frame_bytes(dw, dh) + 3 | 1)
        assert np.array_equal(got, want), (kind, "byte path", np.argwhere(got != want)[:4])


def check_constant(pkg, ctx):
    """a constant frame stays constant at every ratio and kind (the rows sum to 16384 and the rounding is centred)"""
    for sw, sh, dw, dh in ((18, 10, 34, 22), (64, 48, 8, 6), (130, 34, 66, 18), (2, 2, 64, 64), (34, 22, 18, 10)):
        for value in (0, 1, 77, 200, 255):
            a = np.full((2, frame_bytes(sw, sh)), value, np.uint8)
            for kind in KINDS:
                got = pkg.frames_scale(ctx, sw, sh, dw, dh, a, kind)
                assert (got == value).all(), (sw, sh, dw, dh, value, kind, np.unique(got))


def check_layouts(pkg, ctx, sw, sh, dw, dh, seed=3):
    """the byte path gives the dword path's frames: a source base offset by 1 and by 2 bytes, a source stride that is no multiple of 4, an
    odd dst_stride, a destination base offset by 1 and by 3 -- PACKED and PADDED (padding 0xA5), two streams, the sentinel intact between
    and beyond the frames"""
    rng = np.random.default_rng(seed * 1000 + sw * 7 + sh * 3 + dw)
    a = hard_frames(sw, sh, 2, rng)
    forms = {PACKED: a, PADDED: np.stack([to_padded_fill(f, sw, sh, SENTINEL) for f in a])}
    dfb = frame_bytes(dw, dh)
    cases = {"tight": {}, "src+1": dict(src_off=1), "src+2": dict(src_off=2), "src stride+3": dict(src_gap=3), "dst stride odd": dict(dst_stride=dfb + 5 | 1),
             "dst+1": dict(dst_off=1), "dst+3,src+2": dict(dst_off=3, src_off=2), "aligned gaps": dict(src_gap=32, dst_stride=(dfb + 15) // 16 * 16 + 32)}
    for kind in KINDS:
        want = ref_frames(a, sw, sh, lib_tables(pkg, kind, sw, sh, dw, dh))
        with pkg.Scaler(ctx, sw, sh, dw, dh, kind) as sc:
            for layout in (PACKED, PADDED):
                for name, kw in cases.items():
                    got = scale_dev(ctx, sc, forms[layout], layout, rng=rng, **kw)
                    assert np.array_equal(got, want), (sw, sh, dw, dh, kind, layout, name, np.argwhere(got != want)[:4])


# ------------------------------------------------------------------ 3. bad arguments
def check_bad_arguments(pkg, ctx):
    L = pkg._lib
    lib = ctx._lib
    err = ctypes.c_int(0)

    def create(sw=16, sh=16, dw=32, dh=8, kind=1, ctx_h=ctx.handle, e=err):
        err.value = 0
        h = lib.pfv_scaler_create(ctx_h, sw, sh, dw, dh, kind, ctypes.byref(e) if e is not None else None)
        if h:
            lib.pfv_scaler_destroy(h)
        return bool(h), err.value
    assert create() == (True, L.PFV_OK) and create(e=None)[0]
    assert create(64, 48, 8, 6) == (True, L.PFV_OK)                                 # ratio 8 exactly
    assert create(66, 16, 8, 2) == (False, L.PFV_ERR_BAD_ARG)                       # beyond 8 on x
    assert create(16, 66, 2, 8) == (False, L.PFV_ERR_BAD_ARG)                       # ... on y
    for bad in ((15, 16, 32, 8), (16, 17, 32, 8), (16, 16, 31, 8), (16, 16, 32, 9), (0, 16, 32, 8), (16, -2, 32, 8), (16, 16, 0, 8), (16, 16, 32, -8),
                (65536, 16, 65534, 8), (16, 16, 65536, 8), (16, 16, 32, 65536)):
        assert create(*bad) == (False, L.PFV_ERR_BAD_ARG), bad
    assert create(kind=3) == (False, L.PFV_ERR_BAD_ARG) and create(kind=-1) == (False, L.PFV_ERR_BAD_ARG)
    assert create(ctx_h=None) == (False, L.PFV_ERR_BAD_ARG) and not create(66, 16, 8, 2, e=None)[0]
    lib.pfv_scaler_destroy(None)
    with pytest.raises(pkg.PfvError):
        pkg.Scaler(ctx, 66, 16, 8, 2)
    sw, sh, dw, dh = 16, 16, 32, 8
    sfb, spfb, dfb = frame_bytes(sw, sh), padded_frame_bytes(sw, sh), frame_bytes(dw, dh)
    assert sfb == dfb == 384
    bufs = DevBufs(ctx)
    sc = pkg.Scaler(ctx, sw, sh, dw, dh, "bicubic")
    graph = pkg.Graph(ctx)
    try:
        a = bufs.put(np.zeros(8192, dtype=np.uint8))
        d = bufs.put(np.zeros(8192, dtype=np.uint8))

        def call(n=1, src=a, layout=PACKED, ss=0, dst=d, ds=0, h=sc.handle):
            return lib.pfv_scaler_run_dev(h, n, P(src) if src else None, layout, ss, P(dst) if dst else None, ds)
        assert call() == L.PFV_OK and call(n=2, layout=PADDED) == L.PFV_OK
        assert call(n=0) == L.PFV_ERR_BAD_ARG and call(n=-1) == L.PFV_ERR_BAD_ARG
        assert call(layout=2) == L.PFV_ERR_BAD_ARG and call(layout=-1) == L.PFV_ERR_BAD_ARG
        assert call(src=None) == L.PFV_ERR_BAD_ARG and call(dst=None) == L.PFV_ERR_BAD_ARG and call(h=None) == L.PFV_ERR_BAD_ARG
        assert call(n=2, ss=sfb - 1) == L.PFV_ERR_BAD_ARG and call(n=2, ss=sfb) == L.PFV_OK
        assert call(n=2, layout=PADDED, ss=spfb - 1) == L.PFV_ERR_BAD_ARG and call(n=2, layout=PADDED, ss=spfb) == L.PFV_OK
        assert call(n=2, ds=dfb - 1) == L.PFV_ERR_BAD_ARG and call(n=2, ds=dfb) == L.PFV_OK
        # overlapping ranges, either way round; a range runs from the first frame to the end of the last one
        assert call(dst=a) == L.PFV_ERR_BAD_ARG
        assert call(dst=a + sfb - 1) == L.PFV_ERR_BAD_ARG and call(dst=a + sfb) == L.PFV_OK
        assert call(src=a + dfb - 1, dst=a) == L.PFV_ERR_BAD_ARG and call(src=a + dfb, dst=a) == L.PFV_OK
        assert call(n=2, src=a + dfb, dst=a, ds=2 * dfb) == L.PFV_ERR_BAD_ARG            # the source lies in the gap between the frames
        # the host form
        host, out = np.zeros(sfb, np.uint8), np.zeros(dfb, np.uint8)
        hp = lambda x: x.ctypes.data_as(P)      # noqa: E731

        def hcall(sw=sw, sh=sh, dw=dw, dh=dh, n=1, src=host, dst=out, kind=1, ctx_h=ctx.handle):
            return lib.pfv_frames_scale(ctx_h, sw, sh, dw, dh, n, hp(src) if src is not None else None, hp(dst) if dst is not None else None, kind)
        assert hcall() == L.PFV_OK
        assert hcall(sw=15) == L.PFV_ERR_BAD_ARG and hcall(dh=9) == L.PFV_ERR_BAD_ARG and hcall(n=0) == L.PFV_ERR_BAD_ARG
        assert hcall(src=None) == L.PFV_ERR_BAD_ARG and hcall(dst=None) == L.PFV_ERR_BAD_ARG and hcall(kind=3) == L.PFV_ERR_BAD_ARG
        assert hcall(ctx_h=None) == L.PFV_ERR_BAD_ARG
        big = np.zeros(frame_bytes(66, 16), np.uint8)
        assert hcall(sw=66, sh=16, dw=8, dh=2, src=big) == L.PFV_ERR_BAD_ARG
        # while a graph is being recorded: the host form and the plan's creation refuse, a run is recorded
        with graph:
            assert hcall() == L.PFV_ERR_STATE
            assert create() == (False, L.PFV_ERR_STATE)
            assert call() == L.PFV_OK
        ctx.sync()
    finally:
        graph.close()
        sc.close()
        bufs.close()


def check_graph(pkg, ctx, sw=144, sh=80, dw=96, dh=54, n=2):
    """a run recorded in a graph is one kernel node: replayed twice on changing source bytes it gives numpy's frames each time"""
    rng = np.random.default_rng(17)
    bufs = DevBufs(ctx)
    sc = pkg.Scaler(ctx, sw, sh, dw, dh, "lanczos3")
    graph = pkg.Graph(ctx)
    try:
        tabs = lib_tables(pkg, "lanczos3", sw, sh, dw, dh)
        s_dev = bufs.put(np.zeros(n * frame_bytes(sw, sh), np.uint8))
        d_dev = bufs.put(np.zeros(n * frame_bytes(dw, dh), np.uint8))
        with graph:
            sc.run_dev(n, s_dev, d_dev)
        for _ in range(2):
            a = hard_frames(sw, sh, n, rng)
            ctx.upload(s_dev, a)
            graph.launch()
            got = np.zeros((n, frame_bytes(dw, dh)), np.uint8)
            ctx.download(got, d_dev)
            assert np.array_equal(got, ref_frames(a, sw, sh, tabs))
    finally:
        graph.close()
        sc.close()
        bufs.close()


# ------------------------------------------------------------------ 4. decoder session
def check_dec_session(pkg, ctx, oracle, deblock, planar, rgb, w=144, h=48, dw=96, dh=32, kind="bicubic", quality=5, n=3):
    """I P P, three slots, the window set to slots [1, 3), the resized output with a stride; `planar`: a strided planar output beside it, `rgb`:
    an RGB output beside it, `deblock`: "off" / "auto" / "fixed".  After every decode call the window's frames in the set output equal numpy's
    resize of pfv_dec_get_frame (the filtered picture when the filter is on); slot 0's frame and every gap keep the sentinel.  A twin session
    without the resized output sees the same calls: framebuffer, pfv_dec_get_frame, the planar and the RGB output are bit-identical."""
    import deblock_cases as dc
    import present_cases as pc
    tabs = np.stack(oracle.qtables(quality)[:4])
    steps = pc.session_steps(pkg, oracle, w, h, quality, n, seed=81)
    fb, dfb = frame_bytes(w, h), frame_bytes(dw, dh)
    stride = dfb + 48
    p_stride = dc.odd_stride(fb)
    fixed = (3, 0, 9)
    stabs = lib_tables(pkg, kind, w, h, dw, dh)
    dec, twin = (pkg.DecoderSession(ctx, w, h, tabs, n) for _ in range(2))
    sc = pkg.Scaler(ctx, w, h, dw, dh, kind)
    bufs = DevBufs(ctx)
    try:
        size = GUARD + n * stride + GUARD
        out_dev = bufs.put(np.full(size, SENTINEL, np.uint8))
        outs, rgbs = {}, {}
        for d in (dec, twin):
            d.set_window(1, 2)
            d.set_deblock(deblock, fixed if deblock == "fixed" else None)
            if planar:
                outs[d] = bufs.put(np.full(n * p_stride + 64, SENTINEL, np.uint8))
                d.set_output_strided_dev(outs[d], p_stride)
            if rgb:
                rgbs[d] = bufs.put(np.full(n * w * h * 4, SENTINEL, np.uint8))
                d.set_output_rgb_dev(rgbs[d], "rgba8")
        dec.set_output_scaled_dev(sc, out_dev + GUARD, stride)
        filtered = False
        for t, step in enumerate(steps):
            pc.decode_step(dec, bufs, step)
            pc.decode_step(twin, bufs, step)
            frames = dec.get_frame()
            assert np.array_equal(frames, twin.get_frame()) and np.array_equal(dec.framebuffer(), twin.framebuffer()), (t, "the resized output changed the session")
            if deblock != "off":
                twin.set_deblock("off")
                filtered = filtered or not np.array_equal(twin.get_frame(), frames)
                twin.set_deblock(deblock, fixed if deblock == "fixed" else None)
            for side, nbytes in ((outs, n * p_stride + 64), (rgbs, n * w * h * 4)):
                if side:
                    raw = [np.zeros(nbytes, np.uint8) for _ in range(2)]
                    ctx.download(raw[0], side[dec])
                    ctx.download(raw[1], side[twin])
                    assert np.array_equal(raw[0], raw[1]) and (raw[0] != SENTINEL).any(), (t, "an output beside the resized one")
            want = ref_frames(frames[1:], w, h, stabs)
            raw = np.zeros(size, np.uint8)
            ctx.download(raw, out_dev)
            got, rest = read_frames(raw, GUARD + stride, 2, dfb, stride)          # the window's slots; slot 0 must keep the sentinel
            assert np.array_equal(got, want), (t, "set output", np.argwhere(got != want)[:4])
            assert (rest == SENTINEL).all(), (t, "set output: bytes outside the window's frames were written")
        assert deblock == "off" or filtered, "the filter changes nothing here: the check would be empty"
        # switched off again, a decode call leaves the buffer alone
        dec.set_output_scaled_dev(None, None)
        ctx.upload(out_dev, np.full(size, SENTINEL, np.uint8))
        pc.decode_step(dec, bufs, steps[2])
        raw = np.zeros(size, np.uint8)
        ctx.download(raw, out_dev)
        assert (raw == SENTINEL).all()
    finally:
        bufs.close()
        dec.close()
        twin.close()
        sc.close()


def check_dec_forms(pkg, ctx, oracle, w=144, h=48, dw=66, dh=18, kind="lanczos3", quality=5, n=3):
    """the host, sparse and lists forms of the decode calls write the set output too (full window, tight)"""
    import present_cases as pc
    tabs = np.stack(oracle.qtables(quality)[:4])
    steps = pc.session_steps(pkg, oracle, w, h, quality, n, seed=85)
    dfb = frame_bytes(dw, dh)
    stabs = lib_tables(pkg, kind, w, h, dw, dh)
    dec = pkg.DecoderSession(ctx, w, h, tabs, n)
    sc = pkg.Scaler(ctx, w, h, dw, dh, kind)
    bufs = DevBufs(ctx)
    try:
        out_dev = bufs.put(np.zeros(n * dfb, np.uint8))
        dec.set_output_scaled_dev(sc, out_dev)

        def shown(what):
            raw = np.zeros((n, dfb), np.uint8)
            ctx.download(raw, out_dev)
            ctx.upload(out_dev, np.full(n * dfb, SENTINEL, np.uint8))
            assert np.array_equal(raw, ref_frames(dec.get_frame(), w, h, stabs)), what
        dec.decode_iframe(steps[0][0])
        shown("pfv_dec_iframe")
        mv, has, coef = steps[1]
        dec.decode_pframe(mv, has, coef)
        shown("pfv_dec_pframe")
        mv, has, coef = steps[2]
        flat = coef.reshape(-1).copy()
        flat.reshape(n, -1, 256)[has.reshape(n, -1) == 0] = 0
        idx = np.flatnonzero(flat).astype(np.uint32)
        dec.decode_pframe_sparse(mv, has, idx, flat[idx])
        shown("pfv_dec_pframe_sparse")
        entries, counts = dec.coef_lists(steps[0][0])
        dec.decode_iframe_lists(entries, counts)
        shown("pfv_dec_iframe_lists_dev")
        idx = np.flatnonzero(steps[0][0].reshape(-1)).astype(np.uint32)
        dec.decode_iframe_sparse(idx, steps[0][0].reshape(-1)[idx])
        shown("pfv_dec_iframe_sparse")
    finally:
        bufs.close()
        dec.close()
        sc.close()


def check_dec_graph(pkg, ctx, oracle, w=144, h=48, dw=192, dh=80, kind="bilinear", quality=5, n=3):
    """I P P with deblocking AUTO and no planar output (the filtered picture passes through the session's scratch, allocated by the set calls
    before the recording) recorded in one graph with three resized outputs and replayed twice: both replays equal numpy's resize of the
    frames a twin session returns step by step"""
    import present_cases as pc
    tabs = np.stack(oracle.qtables(quality)[:4])
    steps = pc.session_steps(pkg, oracle, w, h, quality, n, seed=91)
    dfb = frame_bytes(dw, dh)
    stabs = lib_tables(pkg, kind, w, h, dw, dh)
    dec, twin = (pkg.DecoderSession(ctx, w, h, tabs, n) for _ in range(2))
    sc = pkg.Scaler(ctx, w, h, dw, dh, kind)
    bufs = DevBufs(ctx)
    graph = pkg.Graph(ctx)
    try:
        want = []
        twin.set_deblock("auto")
        for step in steps:
            pc.decode_step(twin, bufs, step)
            want.append(ref_frames(twin.get_frame(), w, h, stabs))
        dev_steps = [tuple(bufs.put(x) for x in step) for step in steps]
        outs = [bufs.put(np.full(n * dfb, SENTINEL, np.uint8)) for _ in steps]
        dec.set_deblock("auto")
        dec.set_output_scaled_dev(sc, outs[0])          # the scratch is made here
        with graph:
            for t, st in enumerate(dev_steps):
                dec.set_output_scaled_dev(sc, outs[t])
                if t == 0:
                    dec.decode_iframe_dev(*st)
                else:
                    dec.decode_pframe_dev(*st)
        for _ in range(2):
            for o in outs:
                ctx.upload(o, np.full(n * dfb, SENTINEL, np.uint8))
            graph.launch()
            for t, o in enumerate(outs):
                got = np.zeros((n, dfb), np.uint8)
                ctx.download(got, o)
                assert np.array_equal(got, want[t]), t
        dec.check()
    finally:
        graph.close()
        bufs.close()
        dec.close()
        twin.close()
        sc.close()


# ------------------------------------------------------------------ 5. pfv_decoder
def decoder_callbacks(pkg, ctx, dec, nbytes, device_out):
    """every callback of the advance calls as (y bytes, u - y, v - y, w, h) through the C ABI itself"""
    from ctypes import CFUNCTYPE, c_int, c_void_p
    seen = []

    def cb(_user, y, u, v, w, h):
        a = np.zeros(nbytes, np.uint8)
        if device_out:
            ctx.download(a, int(y))
        else:
            a[:] = np.ctypeslib.as_array(ctypes.cast(y, ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes,))
        seen.append((a, (u - y) if u else None, (v - y) if v else None, w, h))
    fn = CFUNCTYPE(None, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int)(cb)
    while True:
        rc = ctx._lib.pfv_decoder_advance_frame(dec.handle, fn, None)
        ctx.check(min(rc, 0))
        if rc != 1:
            return seen


def check_decoder(pkg, ctx, oracle, entropy, device_out, deblock, w=48, h=32, dw=32, dh=18, quality=5, n_frames=5, gop=3, drop_at=2):
    """a 5-frame .pfv with one drop frame: with the switch on every callback hands over ONE packed dw x dh frame (u, v behind y; width and
    height arguments dw, dh) equal to numpy's resize of the frame the same decoder delivers with the switch off; as many callbacks as
    without; with RGB on top the picture is to_rgb of that resized frame; width() / height() keep the stream's size; the Python mirror gives
    the same frames; switched off again the frames are the plain ones"""
    import deblock_cases as dc
    import present_cases as pc
    st = pkg.SyntheticStream(w, h)
    frames = [st.frame(t) for t in range(n_frames)]
    plan = qc.clip_plan(n_frames, gop, drop_at)
    assert "D" in plan
    data = dc.oracle_clip(pkg, oracle, w, h, quality, frames, plan)
    fb, dfb = frame_bytes(w, h), frame_bytes(dw, dh)
    for kind in KINDS:
        stabs = lib_tables(pkg, kind, w, h, dw, dh)
        dec = pkg.Decoder(data, ctx, entropy=entropy)
        try:
            if device_out:
                dec.set_output_device(True)
            dec.set_deblock(deblock)
            plain = decoder_callbacks(pkg, ctx, dec, fb, device_out)
            assert len(plain) == n_frames - 1 and all(u == w * h and v == w * h + w * h // 4 and (cw, ch) == (w, h) for _, u, v, cw, ch in plain)
            want = [ref_frame(a, w, h, stabs) for a, *_ in plain]
            dec.reset()
            dec.set_output_size(dw, dh, kind)
            assert (dec.width(), dec.height()) == (w, h)
            for again in range(2):
                got = decoder_callbacks(pkg, ctx, dec, dfb, device_out)
                assert len(got) == len(plain), (kind, len(got))
                for t, ((a, u, v, cw, ch), x) in enumerate(zip(got, want)):
                    assert (u, v, cw, ch) == (dw * dh, dw * dh + dw * dh // 4, dw, dh), (kind, t, u, v, cw, ch)
                    assert np.array_equal(a, x), (kind, t, entropy, device_out, deblock, again, np.flatnonzero(a != x)[:4])
                dec.reset()
            dec.set_output_rgb(True, "bgra8")              # the picture of the resized frame
            got = decoder_callbacks(pkg, ctx, dec, dw * dh * 4, device_out)
            assert len(got) == len(plain)
            for t, ((pic, u, v, cw, ch), x) in enumerate(zip(got, want)):
                assert u is None and v is None and (cw, ch) == (dw, dh)
                assert np.array_equal(pic.reshape(dh, dw, 4), pc.to_rgb(x, dw, dh, "bgra8")), (kind, t, "RGB on top")
            dec.reset()
            if not device_out:                       # the Python mirror hands arrays over
                pics = []
                while dec.advance_frame(pics.append):
                    pass
                assert len(pics) == len(plain) and all(np.array_equal(p, pc.to_rgb(x, dw, dh, "bgra8")) for p, x in zip(pics, want))
                dec.reset()
                dec.set_output_rgb(False)
                frs = []
                while dec.advance_frame(frs.append):
                    pass
                assert len(frs) == len(plain) and all((f.width, f.height) == (dw, dh) and np.array_equal(f.packed(), x) for f, x in zip(frs, want))
                dec.reset()
            dec.set_output_rgb(False)
            dec.set_output_size(0)
            back = decoder_callbacks(pkg, ctx, dec, fb, device_out)
            assert len(back) == len(plain) and all(np.array_equal(a, b) and (cw, ch) == (w, h) for (a, _, _, cw, ch), (b, *_) in zip(back, plain))
        finally:
            dec.close()


# ------------------------------------------------------------------ 6. encoder session
def check_enc_session(pkg, ctx, kind, w=96, h=32, sw=144, sh=48, quality=5, n=3):
    """I P P of three slots, the window set to slots [1, 3): pfv_enc_scale_dev with a source stride, then the probe, encode, distortion and
    SSIM calls on the returned pointer, against a twin session fed pfv_frames_scale's frames through the same window"""
    import ingest_cases as ic
    rng = np.random.default_rng(61)
    L = pkg._lib
    fb, sfb = frame_bytes(w, h), frame_bytes(sw, sh)
    s_stride = sfb + 48
    stabs = lib_tables(pkg, kind, sw, sh, w, h)
    enc, twin = (pkg.EncoderSession(ctx, w, h, quality, n) for _ in range(2))
    sc = pkg.Scaler(ctx, sw, sh, w, h, kind)
    bufs = DevBufs(ctx)

    def lay(frames):
        buf = rng.integers(0, 256, n * s_stride, dtype=np.uint8)
        for k in range(n):
            buf[k * s_stride:k * s_stride + sfb] = frames[k]
        return buf
    try:
        tb = enc.total_blocks
        out, tout = ic.EncBufs(ctx, bufs, n, tb), ic.EncBufs(ctx, bufs, n, tb)
        first = hard_frames(sw, sh, n, rng)
        base = enc.scale_dev(sc, bufs.put(lay(first)), s_stride)
        for s in (enc, twin):
            s.set_window(1, 2)
        sizes_d, tsizes_d = (bufs.put(np.full(n, 0x5A5A5A5A, np.uint32)) for _ in range(2))
        for t in range(3):
            src = np.stack([pkg.SyntheticStream(sw, sh, seed=61 + k).frame(t) for k in range(n)])
            frames = pkg.frames_scale(ctx, sw, sh, w, h, src, kind)
            assert np.array_equal(frames, ref_frames(src, sw, sh, stabs))
            ptr = enc.scale_dev(sc, bufs.put(lay(src)), s_stride)
            assert ptr == base and ptr % 16 == 0, "one buffer, owned by the session"
            held = np.zeros((n, fb), np.uint8)
            ctx.download(held, ptr)
            assert np.array_equal(held[1:], frames[1:]) and np.array_equal(held[0], ref_frame(first[0], sw, sh, stabs)), (t, "the session's frame buffer")
            frames_dev = bufs.put(frames)
            enc.probe_iframe_dev(ptr, sizes_d)
            twin.probe_iframe_dev(frames_dev, tsizes_d)
            a, b = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
            ctx.download(a, sizes_d)
            ctx.download(b, tsizes_d)
            assert np.array_equal(a, b) and a[0] == 0x5A5A5A5A and (a[1:] != 0x5A5A5A5A).all(), (t, "pfv_enc_probe_iframe_dev", a, b)
            if t == 0:
                enc.encode_iframe_dev(ptr, out.coef)
                twin.encode_iframe_dev(frames_dev, tout.coef)
            else:
                enc.encode_pframe_dev(ptr, out.mv, out.has, out.coef)
                twin.encode_pframe_dev(frames_dev, tout.mv, tout.has, tout.coef)
            for name, x, y in zip(("coefficients", "motion vectors", "has-coefficient flags"), out.read(), tout.read()):
                assert np.array_equal(x, y), (t, name)
            assert (out.read()[0][1:] != 0x5A5A).any()
            assert np.array_equal(enc.prev_frame(), twin.prev_frame()), (t, "pfv_enc_prev_frame")
            sent = np.full((n, 3), 0x1122334455667788, dtype=np.uint64)
            sse = enc.distortion(int(ptr), out=sent)
            assert np.array_equal(sse, twin.distortion(int(frames_dev), out=sent)) and np.array_equal(sse[0], sent[0]) and sse[1:].sum() > 0, (t, "pfv_enc_distortion_dev")
            ssent = np.full((n, 3), -77, dtype=np.int64)
            q24 = enc.ssim(int(ptr), out=ssent)
            assert np.array_equal(q24, twin.ssim(int(frames_dev), out=ssent)) and np.array_equal(q24[0], ssent[0]), (t, "pfv_enc_ssim_dev")
        # the session's buffer is packed: a frame stride refuses, and its neighbour 0 accepts
        src_dev = bufs.put(lay(src))
        enc.set_frame_stride(fb + 16)
        with pytest.raises(pkg.PfvError) as e:
            enc.scale_dev(sc, src_dev, s_stride)
        assert e.value.code == L.PFV_ERR_STATE
        enc.set_frame_stride(0)
        assert enc.scale_dev(sc, src_dev, s_stride) == base
        # a session whose first call falls inside a recording is refused; this one's is recorded
        late = pkg.EncoderSession(ctx, w, h, quality, n)
        graph = pkg.Graph(ctx)
        try:
            with graph:
                with pytest.raises(pkg.PfvError) as e:
                    late.scale_dev(sc, src_dev, s_stride)
                assert e.value.code == L.PFV_ERR_STATE
                assert enc.scale_dev(sc, src_dev, s_stride) == base
        finally:
            graph.close()
            late.close()
        ctx.sync()
    finally:
        bufs.close()
        enc.close()
        twin.close()
        sc.close()


# ------------------------------------------------------------------ 7. pfv_encoder
ENCODER_CONFIGS = {
    "plain_device": dict(device_entropy=True, kw=dict(quality=5)),
    "plain_host": dict(device_entropy=False, kw=dict(quality=5)),
    "floors_budget": dict(device_entropy=True, kw=dict(quality=None, qualities=[2, 5, 8], iframe_ssim_floor=0.97, pframe_quality_floor=34.0)),
    "encode_frame": dict(device_entropy=True, kw=dict(quality=None, qualities=[1, 5, 10]), auto=True),
    "rgb_device": dict(device_entropy=True, kw=dict(quality=5), rgb=("rgb8", "box")),
    "rgb_host": dict(device_entropy=False, kw=dict(quality=5), rgb=("bgra8", "point")),
}


def check_encoder(pkg, ctx, config, kind="bicubic", w=48, h=32, sw=80, sh=54, n_frames=5):
    """twin encoders, one with set_input_size fed sw x sh frames (with `rgb`: set_input_rgb too, fed sw x sh pictures), one fed the frames
    pfv_frames_scale made of them: the drained bytes are identical after every call, and so are rungs, frame reports, frame SSIM and the six
    probe calls' outputs; switched off again the planar calls give the twin's bytes"""
    import ingest_cases as ic
    cfg = ENCODER_CONFIGS[config]
    rng = np.random.default_rng(83)
    st = pkg.SyntheticStream(sw, sh, seed=83)
    order = [0, 0, 1, 2, 3] if cfg.get("auto") else list(range(n_frames))
    src = [st.frame(t) for t in order]
    if cfg.get("rgb"):
        fmt, chroma = cfg["rgb"]
        ins = [ic.in_format(ic.onp.yuv420_to_rgb(f, sw, sh), fmt, rng) for f in src]
        src = [pkg.frames_from_rgb(ctx, sw, sh, p, fmt, chroma)[0] for p in ins]
    else:
        ins = [pkg.VideoFrame.from_packed(sw, sh, f) for f in src]
    scaled = pkg.frames_scale(ctx, sw, sh, w, h, np.stack(src), kind)
    assert np.array_equal(scaled, ref_frames(src, sw, sh, lib_tables(pkg, kind, sw, sh, w, h)))
    planes = [pkg.VideoFrame.from_packed(w, h, f) for f in scaled]
    a_buf, b_buf = io.BytesIO(), io.BytesIO()
    mk = lambda buf: pkg.Encoder(buf, w, h, 30, ctx=ctx, device_entropy=cfg["device_entropy"], frame_report=True, frame_ssim=True, **cfg["kw"])      # noqa: E731
    a, b = mk(a_buf), mk(b_buf)
    try:
        if cfg.get("rgb"):
            a.set_input_rgb(True, fmt, chroma)
        a.set_input_size(sw, sh, kind)
        for t, (x_in, fr) in enumerate(zip(ins, planes)):
            if t > 0:
                for name in ("probe_iframe", "probe_iframe_rd", "probe_iframe_ssim", "probe_pframe", "probe_pframe_rd", "probe_pframe_ssim"):
                    x, y = getattr(a, name)(x_in), getattr(b, name)(fr)
                    x, y = (x, y) if isinstance(x, tuple) else ((x,), (y,))
                    assert len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y)), (config, t, name, x, y)
            if cfg.get("auto"):
                ta, tb = a.encode_frame(x_in), b.encode_frame(fr)
                assert ta == tb, (config, t, ta, tb)
            elif t in (0, 3):
                a.encode_iframe(x_in)
                b.encode_iframe(fr)
            else:
                a.encode_pframe(x_in)
                b.encode_pframe(fr)
            assert a_buf.getvalue() == b_buf.getvalue(), (config, t, "stream bytes")
            assert a.rung == b.rung and a.last_report == b.last_report and a.last_ssim == b.last_ssim, (config, t, a.last_report, b.last_report)
        # switched off again, the planar calls give the bytes they give on the twin
        a.set_input_size(0)
        if cfg.get("rgb"):
            a.set_input_rgb(False)
        for e in (a, b):
            e.encode_iframe(planes[1])
            e.encode_pframe(planes[2])
            e.finish()
        assert a_buf.getvalue() == b_buf.getvalue(), (config, "after set_input_size(off)")
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ 8. bad arguments of the sessions' and objects' calls
def check_bad_arguments_sessions(pkg, ctx, oracle):
    import deblock_cases as dc
    L = pkg._lib
    lib = ctx._lib
    w, h = 32, 16
    bufs = DevBufs(ctx)
    dec = pkg.DecoderSession(ctx, w, h, np.stack(pkg.qtables_from_quality(5)[:4]), 2)
    enc = pkg.EncoderSession(ctx, w, h, 5, 2)
    down, up, other = pkg.Scaler(ctx, w, h, 16, 8), pkg.Scaler(ctx, 16, 8, w, h), pkg.Scaler(ctx, 64, 16, 16, 8)
    graph = pkg.Graph(ctx)
    try:
        d = bufs.put(np.zeros(8192, np.uint8))
        dfb = frame_bytes(16, 8)
        f = lib.pfv_dec_set_output_scaled_dev
        assert f(None, down.handle, P(d), 0) == L.PFV_ERR_BAD_ARG
        assert f(dec.handle, down.handle, P(d), 0) == L.PFV_OK and f(dec.handle, down.handle, P(d), dfb) == L.PFV_OK
        assert f(dec.handle, down.handle, P(d), dfb - 1) == L.PFV_ERR_BAD_ARG
        assert f(dec.handle, None, P(d), 0) == L.PFV_ERR_BAD_ARG
        assert f(dec.handle, up.handle, P(d), 0) == L.PFV_ERR_BAD_ARG and f(dec.handle, other.handle, P(d), 0) == L.PFV_ERR_BAD_ARG      # source size
        assert f(dec.handle, None, None, 7) == L.PFV_OK and f(dec.handle, other.handle, None, 0) == L.PFV_OK                         # NULL: off, whatever the rest says
        with graph:                                   # deblocking on: the scratch cannot be made inside a recording
            dec.set_deblock("auto")
            assert f(dec.handle, down.handle, P(d), 0) == L.PFV_ERR_STATE
        assert f(dec.handle, down.handle, P(d), 0) == L.PFV_OK
        out = ctypes.c_void_p()
        g = lib.pfv_enc_scale_dev
        assert g(None, up.handle, P(d), 0, ctypes.byref(out)) == L.PFV_ERR_BAD_ARG
        assert g(enc.handle, None, P(d), 0, ctypes.byref(out)) == L.PFV_ERR_BAD_ARG and g(enc.handle, up.handle, None, 0, ctypes.byref(out)) == L.PFV_ERR_BAD_ARG
        assert g(enc.handle, up.handle, P(d), 0, None) == L.PFV_ERR_BAD_ARG
        assert g(enc.handle, down.handle, P(d), 0, ctypes.byref(out)) == L.PFV_ERR_BAD_ARG      # destination size
        assert g(enc.handle, up.handle, P(d), dfb - 1, ctypes.byref(out)) == L.PFV_ERR_BAD_ARG and g(enc.handle, up.handle, P(d), dfb, ctypes.byref(out)) == L.PFV_OK
        st = pkg.SyntheticStream(w, h)
        data = dc.oracle_clip(pkg, oracle, w, h, 5, [st.frame(0)], ["I"])
        sd = pkg.Decoder(data, ctx)
        se = pkg.Encoder(io.BytesIO(), w, h, 30, 5, ctx)
        try:
            for fn, hd in ((lib.pfv_decoder_set_output_size, sd.handle), (lib.pfv_encoder_set_input_size, se.handle)):
                assert fn(None, 16, 8, 1) == L.PFV_ERR_BAD_ARG
                assert fn(hd, 16, 8, 1) == L.PFV_OK and fn(hd, 64, 48, 2) == L.PFV_OK and fn(hd, 0, -5, 9) == L.PFV_OK
                assert fn(hd, 15, 8, 1) == L.PFV_ERR_BAD_ARG and fn(hd, 16, 9, 1) == L.PFV_ERR_BAD_ARG and fn(hd, 16, 8, 3) == L.PFV_ERR_BAD_ARG
                assert fn(hd, 65536, 8, 1) == L.PFV_ERR_BAD_ARG
            assert lib.pfv_decoder_set_output_size(sd.handle, 2, 8, 1) == L.PFV_ERR_BAD_ARG          # 32 -> 2: beyond 8
            assert lib.pfv_encoder_set_input_size(se.handle, 258, 16, 1) == L.PFV_ERR_BAD_ARG        # 258 -> 32: beyond 8
        finally:
            sd.close()
            se.close()
        ctx.sync()
    finally:
        graph.close()
        for x in (dec, enc, down, up, other):
            x.close()
        bufs.close()


# ------------------------------------------------------------------ 9. C++ mirror and tool
def build_cpp(lib_path, exe):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "scale_report.cpp"), "-o", exe, lib_path, "-Wl,-rpath," + os.path.dirname(lib_path)], check=True)


def check_cpp(pkg, ctx, oracle, exe, tmp_path, w=48, h=32, dw=32, dh=18, quality=5):
    """tests/cpp/scale_report.cpp (pfv::Scaler, pfv::frames_scale, pfv::scale_table, pfv::Decoder::set_output_size, pfv::Encoder::set_input_size)
    writes what numpy makes of the oracle decoder's frames, and a stream that decodes to what the oracle makes of the resized frames"""
    import deblock_cases as dc
    st = pkg.SyntheticStream(w, h)
    frames = [st.frame(t) for t in range(4)]
    data = dc.oracle_clip(pkg, oracle, w, h, quality, frames, ["I", "P", "P", "I"])
    shown = qc.oracle_decode(oracle, data)
    src = str(tmp_path / "in.pfv")
    open(src, "wb").write(data)
    for kind, code in KINDS.items():
        o1, o2, o3 = (str(tmp_path / f"{kind}_{x}.bin") for x in ("decoder", "frames", "stream"))
        r = subprocess.run([exe, src, str(dw), str(dh), str(code), o1, o2, o3], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        T = np_taps(code, w, dw)
        assert r.stdout.splitlines() == [f"frames 4 of {w}x{h} resized to {dw}x{dh} taps {T} table ok"], r.stdout
        want = ref_frames(shown, w, h, lib_tables(pkg, kind, w, h, dw, dh))
        for path in (o1, o2):
            assert np.array_equal(np.fromfile(path, dtype=np.uint8).reshape(want.shape), want), (kind, path)
        # o3: the resized frames' encoder fed the decoder's full-size frames through set_input_size == an encoder fed the resized frames
        buf = io.BytesIO()
        e = pkg.Encoder(buf, dw, dh, 30, quality, ctx)
        try:
            for t, f in enumerate(want):
                (e.encode_iframe if t == 0 else e.encode_pframe)(pkg.VideoFrame.from_packed(dw, dh, f))
            e.finish()
        finally:
            e.close()
        assert open(o3, "rb").read() == buf.getvalue(), (kind, "pfv::Encoder::set_input_size")


def check_rd_tool(pkg, lib_path, w=64, h=48):
    """tools/rd_curve.py --time-scale on the library at lib_path prints its rows: the yardstick, then per size pair one line per kind"""
    env = dict(os.environ)
    env["PFV_HIP_LIB"] = lib_path
    cmd = [sys.executable, os.path.join(ROOT, "tools", "rd_curve.py"), str(w), str(h), "1", "--qualities", "", "--time-scale"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr
    rows = [json.loads(x)["time_scale"] for x in r.stdout.splitlines()]
    pairs = [(64, 48, 44, 32), (64, 48, 32, 24), (64, 48, 8, 6), (32, 24, 64, 48)]
    assert [x["case"] for x in rows] == ["crop"] + [f"{a}x{b}->{c}x{d} {k}" for a, b, c, d in pairs for k in KINDS]
    assert rows[0]["bytes"] == frame_bytes(w, h) + padded_frame_bytes(w, h)
    for x, (a, b, c, d) in zip(rows[1:], [p for p in pairs for _ in KINDS]):
        assert x["bytes"] == frame_bytes(a, b) + frame_bytes(c, d) and x["ms"] >= 0 and "rate_over_crop_rate" in x and x["shape"] == f"1 x {w}x{h}", x
    return rows
