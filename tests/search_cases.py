"""Shared checks of the exhaustive motion search (PFV_SEARCH_FULL: k_pf_search_full + k_pf_transform, pfv_*_set_motion_search), run by
tests/test_emu_search.py on the CPU emulator build of the kernel sources and by tests/test_gpu_search.py on the MI355X at the same shapes.

The expected values come from a numpy restatement of the rule in include/pfv_hip_ext.h ("exhaustive motion search"): every (dx, dy) of the
square that stays inside the padded plane, exact integer SSD, the lexicographic minimum of (E, |dx| + |dy|, dy, dx) -- composed with the
oracle's existing pieces (pad_plane, encode_plane / decode_plane, encode_blocks_delta, decode_plane_delta, qtables).  Every comparison is an
equality.  Sections 9 .. 12 (every radius, ladder rungs, k_pf_transform's groups, the largest error) and what they kill:
profiles/search_mutants.md."""
import ctypes
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ladder_cases as lc
import pfv_oracle_np as onp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p

SHAPES = [(16, 16), (17, 33), (144, 48), (304, 80)]
RADII = [1, 7, 15]
QUALITIES = (2, 8)
N_STREAMS = 3


def even(x):
    return x + (x & 1)


def frame_bytes(w, h):
    return w * h + 2 * (w // 2) * (h // 2)


def planes_of(frame, w, h):
    """packed frame -> [(plane [h, w], clear)] for Y, U, V"""
    f = np.ascontiguousarray(frame, dtype=np.uint8).reshape(-1)
    cw, ch = w // 2, h // 2
    return [(f[:w * h].reshape(h, w), 0), (f[w * h:w * h + cw * ch].reshape(ch, cw), 128), (f[w * h + cw * ch:].reshape(ch, cw), 128)]


# ------------------------------------------------------------------ the restatement
def block_errors(img, ref, dx, dy):
    """E(dx, dy) of every macroblock [bh, bw] and whether the candidate lies inside the plane; img, ref: padded planes"""
    ph, pw = img.shape
    bh, bw = ph // 16, pw // 16
    by, bx = np.mgrid[0:bh, 0:bw] * 16
    ok = (bx + dx >= 0) & (bx + dx <= pw - 16) & (by + dy >= 0) & (by + dy <= ph - 16)
    big = np.zeros((ph + 30, pw + 30), np.int64)
    big[15:15 + ph, 15:15 + pw] = ref
    d = img.astype(np.int64) - big[15 + dy:15 + dy + ph, 15 + dx:15 + dx + pw]
    return (d * d).reshape(bh, 16, bw, 16).sum(axis=(1, 3)), ok


def full_search(img, ref, R):
    """-> (mv [n, 2] int8, E [n] int64): the lexicographic minimum of (E, |dx| + |dy|, dy, dx) over the candidates inside the plane"""
    ph, pw = img.shape
    best = np.full((ph // 16, pw // 16), np.iinfo(np.int64).max, np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            e, ok = block_errors(img, ref, dx, dy)
            key = (e << 24) | ((abs(dx) + abs(dy)) << 16) | ((dy + 16) << 8) | (dx + 16)       # E < 2^24
            best = np.where(ok & (key < best), key, best)
    best = best.reshape(-1)
    mv = np.stack([(best & 255) - 16, ((best >> 8) & 255) - 16], axis=1).astype(np.int8)
    return mv, best >> 24


def encode_plane_full(px, ref, q, px_err, clear, R):
    """the rule, then the existing operator: skip test in f32, clip(src - patch, +-255) -> encode_subblock_delta"""
    img = onp.pad_plane(px, clear)
    bw = img.shape[1] // 16
    mv, err = full_search(img, ref, R)
    min_err = np.float32(px_err) * np.float32(px_err) * np.float32(256.0)
    has = (~(err.astype(np.float32) <= min_err)).astype(np.uint8)
    coef = np.zeros((mv.shape[0], 256), np.int16)
    blocks = onp._gather(img)
    idx = np.nonzero(has)[0]
    if idx.size:
        prev = np.stack([ref[(i // bw) * 16 + mv[i, 1]:(i // bw) * 16 + mv[i, 1] + 16, (i % bw) * 16 + mv[i, 0]:(i % bw) * 16 + mv[i, 0] + 16] for i in idx])
        delta = np.clip(blocks[idx].astype(np.int64) - prev.astype(np.int64), -255, 255)
        coef[idx] = onp.encode_blocks_delta(delta, q)
    return mv, has, coef, err


class RefEncoder:
    """the hot-path half of the encoder in numpy, p-frames by the full search at radius R; prev: the three padded planes"""

    def __init__(self, w, h, quality):
        self.w, self.h = w, h
        t = onp.qtables(quality)
        self.q, self.px_err = t[:4], t[4]
        self.prev = None
        self.err = None

    def iframe(self, frame):
        coefs, prev = [], []
        for k, (px, clear) in enumerate(planes_of(frame, self.w, self.h)):
            c, bw, bh = onp.encode_plane(px, self.q[min(k, 1)], clear)
            coefs.append(c)
            prev.append(onp.decode_plane(c, bw, bh, self.q[min(k, 1)]))
        self.prev = prev
        return np.concatenate(coefs)

    def pframe(self, frame, R):
        mvs, hass, coefs, prev, errs = [], [], [], [], []
        for k, (px, clear) in enumerate(planes_of(frame, self.w, self.h)):
            q = self.q[2 + min(k, 1)]
            ref = self.prev[k]
            mv, has, coef, err = encode_plane_full(px, ref, q, self.px_err, clear, R)
            prev.append(onp.decode_plane_delta(mv, has, coef, ref.shape[1] // 16, ref.shape[0] // 16, q, ref))
            mvs.append(mv); hass.append(has); coefs.append(coef); errs.append(err)
        self.prev = prev
        self.err = np.concatenate(errs)
        return np.concatenate(mvs), np.concatenate(hass), np.concatenate(coefs)

    def prev_frame(self):
        return np.concatenate([p.reshape(-1) for p in self.prev])

    def shown(self):
        """what a decoder hands out: the planes cropped to the frame"""
        w, h = self.w, self.h
        return np.concatenate([self.prev[0][:h, :w].reshape(-1), self.prev[1][:h // 2, :w // 2].reshape(-1), self.prev[2][:h // 2, :w // 2].reshape(-1)])


# ------------------------------------------------------------------ content
def moving_clip(w, h, n_frames, seed, reach=12, noise=2):
    """a smoothed random canvas seen through a window that jumps by up to `reach` pixels per frame, plus a little seeded noise: large motion
    over a textured surface.  Chroma is the luma window at the even positions, so it moves by half the luma vector."""
    rng = np.random.default_rng(seed)
    m = 4 * reach + 8
    c = rng.integers(0, 256, (h + 2 * m + 2, w + 2 * m + 2)).astype(np.int64)
    c = (c[:-2, :-2] + c[1:-1, :-2] + c[2:, :-2] + c[:-2, 1:-1] + 2 * c[1:-1, 1:-1] + c[2:, 1:-1] + c[:-2, 2:] + c[1:-1, 2:] + c[2:, 2:]) // 10
    c = np.clip((c - 128) * 3 + 128, 0, 255)
    out, ox, oy = [], m, m
    for _ in range(n_frames):
        y = np.clip(c[oy:oy + h, ox:ox + w] + rng.integers(-noise, noise + 1, (h, w)), 0, 255).astype(np.uint8)
        u = y[::2, ::2][:h // 2, :w // 2]
        v = 255 - u
        out.append(np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]))
        ox = int(np.clip(ox + rng.integers(-reach, reach + 1), m - 2 * reach, m + 2 * reach))
        oy = int(np.clip(oy + rng.integers(-reach, reach + 1), m - 2 * reach, m + 2 * reach))
    return np.stack(out)


class DevBufs:
    """device allocations of one check, freed together"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.ctx.alloc(max(arr.nbytes, 16))
        self.ptrs.append(p)
        if arr.nbytes:
            self.ctx.upload(p, arr)
        return p

    def close(self):
        for p in self.ptrs:
            self.ctx.free(p)
        self.ptrs = []


_REF_CACHE = {}


def reference_run(w, h, quality, R, seeds, n_frames=3):
    """per seed the restatement's outputs of I P P: [(coef0, (mv, has, coef), prev_frame after each frame)]; computed once per case"""
    key = (w, h, quality, R, tuple(seeds), n_frames)
    if key not in _REF_CACHE:
        res = []
        for s in seeds:
            clip = moving_clip(w, h, n_frames, s)
            ref = RefEncoder(w, h, quality)
            steps = [(ref.iframe(clip[0]), ref.prev_frame())]
            for t in range(1, n_frames):
                steps.append((ref.pframe(clip[t], R), ref.prev_frame()))
            res.append((clip, steps))
        _REF_CACHE[key] = res
    return _REF_CACHE[key]


def qtabs(pkg, quality):
    return np.stack(pkg.qtables_from_quality(quality)[:4])


# ------------------------------------------------------------------ 1. shapes x radius
def check_shape(pkg, ctx, w, h, R):
    """I P P of three streams with distinct content at qualities 2 and 8: mv, has_coef, coefficients equal the restatement's, and so does the
    reconstruction, read as the next frame's reference (pfv_enc_prev_frame) and through a decoder session fed the outputs.  Quality 2 runs a
    second time through the device entry points with the window on slots 1..2 of 3 and a frame stride: the same values there, slot 0 untouched."""
    w, h = even(w), even(h)        # 17 x 33 is the PLANE size of the case: frames are even (src/frame.rs:13), chroma then is 9 x 17
    n, fb = N_STREAMS, frame_bytes(w, h)
    seeds = [101 * w + h + k for k in range(n)]
    for quality in QUALITIES:
        runs = reference_run(w, h, quality, R, seeds)
        enc = pkg.EncoderSession(ctx, w, h, quality, n)
        dec = pkg.DecoderSession(ctx, w, h, qtabs(pkg, quality), n)
        try:
            enc.set_motion_search("full", R)
            assert enc.motion_search == (pkg.PFV_SEARCH_FULL, R)
            for t in range(3):
                frames = np.stack([runs[k][0][t] for k in range(n)])
                if t == 0:
                    coef = enc.encode_iframe(frames)
                    dec.decode_iframe(coef)
                    for k in range(n):
                        assert np.array_equal(coef[k], runs[k][1][0][0]), (quality, k, "i-frame coefficients")
                else:
                    mv, has, coef = enc.encode_pframe(frames)
                    dec.decode_pframe(mv, has, coef)
                    for k in range(n):
                        wmv, whas, wcoef = runs[k][1][t][0]
                        assert np.array_equal(mv[k], wmv), (quality, t, k, "motion vectors", np.nonzero((mv[k] != wmv).any(axis=1))[0][:8])
                        assert np.array_equal(has[k], whas), (quality, t, k, "has_coef")
                        assert np.array_equal(coef[k], wcoef), (quality, t, k, "coefficients")
                prev, fbuf = enc.prev_frame(), dec.framebuffer()
                for k in range(n):
                    assert np.array_equal(prev[k], runs[k][1][t][1]), (quality, t, k, "reconstruction")
                    assert np.array_equal(fbuf[k], runs[k][1][t][1]), (quality, t, k, "decoder framebuffer")
        finally:
            enc.close()
            dec.close()
    # window [1, 3) and a frame stride, device entry points
    quality = QUALITIES[0]
    runs = reference_run(w, h, quality, R, seeds)
    stride = fb + 48
    enc = pkg.EncoderSession(ctx, w, h, quality, n)
    bufs = DevBufs(ctx)
    try:
        tb = enc.total_blocks
        enc.set_motion_search("full", R)
        enc.set_window(1, 2)
        enc.set_frame_stride(stride)
        coef_d, mv_d, has_d = bufs.put(np.full(n * tb * 256, 0x5A5A, np.int16)), bufs.put(np.full(n * tb * 2, 0x5A, np.int8)), bufs.put(np.full(n * tb, 0x5A, np.uint8))
        rng = np.random.default_rng(5)
        for t in range(3):
            lay = rng.integers(0, 256, n * stride, dtype=np.uint8)
            for k in range(n):
                lay[k * stride:k * stride + fb] = runs[k][0][t]
            src = bufs.put(lay)
            if t == 0:
                enc.encode_iframe_dev(src, coef_d)
            else:
                enc.encode_pframe_dev(src, mv_d, has_d, coef_d)
            coef, mv, has = np.zeros((n, tb, 256), np.int16), np.zeros((n, tb, 2), np.int8), np.zeros((n, tb), np.uint8)
            ctx.download(coef, coef_d); ctx.download(mv, mv_d); ctx.download(has, has_d)
            assert (coef[0] == 0x5A5A).all() and (mv[0] == 0x5A).all() and (has[0] == 0x5A).all(), (t, "slot 0 is outside the window")
            prev = enc.prev_frame()
            for k in (1, 2):
                want = runs[k][1][t]
                if t == 0:
                    assert np.array_equal(coef[k], want[0]), (t, k, "window: coefficients")
                else:
                    assert np.array_equal(mv[k], want[0][0]) and np.array_equal(has[k], want[0][1]) and np.array_equal(coef[k], want[0][2]), (t, k, "window")
                assert np.array_equal(prev[k], want[1]), (t, k, "window: reconstruction")
    finally:
        bufs.close()
        enc.close()


OPTION_VALUES = [("PFV_OPT_LANE_MAPPING", v) for v in (0, 1, 2)] + [("PFV_OPT_ENC_TRANSFORM", v) for v in (0, 1)] + [("PFV_OPT_TILE_COMPACTION", v) for v in (0, 2)]


def check_options(pkg, ctx, w=304, h=80, R=7, quality=2):
    """the full search under every PFV_OPT_LANE_MAPPING, PFV_OPT_ENC_TRANSFORM and PFV_OPT_TILE_COMPACTION value: one mapping, the same values.
    k_pf_transform runs here on grids the split four-step form never sent it (below the small-grid threshold)."""
    L = pkg._lib
    seeds = [7, 8]
    runs = reference_run(w, h, quality, R, seeds, n_frames=2)
    for name, value in OPTION_VALUES:
        opt = getattr(L, name)
        before = ctx.get_option(opt)
        ctx.set_option(opt, value)
        try:
            enc = pkg.EncoderSession(ctx, w, h, quality, len(seeds))
        finally:
            ctx.set_option(opt, before)
        try:
            enc.set_motion_search("full", R)
            enc.encode_iframe(np.stack([r[0][0] for r in runs]))
            mv, has, coef = enc.encode_pframe(np.stack([r[0][1] for r in runs]))
            prev = enc.prev_frame()
            for k, r in enumerate(runs):
                (wmv, whas, wcoef), wprev = r[1][1]
                assert np.array_equal(mv[k], wmv) and np.array_equal(has[k], whas) and np.array_equal(coef[k], wcoef) and np.array_equal(prev[k], wprev), (name, value, k)
        finally:
            enc.close()


# ------------------------------------------------------------------ 2. ties
def _ipair(pkg, ctx, w, h, quality, first, make_second, R, model_check=None):
    """i-frame `first`, then the p-frame make_second(padded reconstruction planes) in FULL mode at radius R -> (mv, has, restatement's, planes).
    model_check(ref, planes, wmv, whas, wcoef): what a case asserts on the restatement alone, before the device's p-frame is looked at"""
    enc = pkg.EncoderSession(ctx, w, h, quality, 1)
    ref = RefEncoder(w, h, quality)
    try:
        enc.set_motion_search("full", R)
        coef = enc.encode_iframe(first)
        assert np.array_equal(coef[0], ref.iframe(first))
        assert np.array_equal(enc.prev_frame()[0], ref.prev_frame())
        planes = [p.copy() for p in ref.prev]
        second = make_second(planes)
        wmv, whas, wcoef = ref.pframe(second, R)
        if model_check:
            model_check(ref, planes, wmv, whas, wcoef)
        mv, has, coef = enc.encode_pframe(second)
        assert np.array_equal(mv[0], wmv), np.nonzero((mv[0] != wmv).any(axis=1))[0][:8]
        assert np.array_equal(has[0], whas) and np.array_equal(coef[0], wcoef)
        assert np.array_equal(enc.prev_frame()[0], ref.prev_frame())
        return mv[0], has[0], ref, planes
    finally:
        enc.close()


def pack(w, h, y, u, v):
    return np.concatenate([np.ascontiguousarray(y[:h, :w]).reshape(-1), np.ascontiguousarray(u[:h // 2, :w // 2]).reshape(-1), np.ascontiguousarray(v[:h // 2, :w // 2]).reshape(-1)])


def check_ties(pkg, ctx, w=64, h=48, quality=2, R=15):
    """the vector the rule names where errors tie.  w and h are multiples of 32: no plane has padding, so a reference that is flat or periodic
    is so up to its edges."""
    rng = np.random.default_rng(3)
    nl = (w // 16) * (h // 16)
    flat = pack(w, h, np.full((h, w), 100, np.uint8), np.full((h, w), 128, np.uint8), np.full((h, w), 128, np.uint8))
    # a flat reference: every candidate of a macroblock has the same error, (0, 0) wins
    mv, _, _, planes = _ipair(pkg, ctx, w, h, quality, flat, lambda pl: rng.integers(0, 256, frame_bytes(w, h), dtype=np.uint8), R)
    assert all((p == p.flat[0]).all() for p in planes), "the reference is not flat"
    assert (mv == 0).all()
    # horizontal period 8, source shifted by 4: dx = -4 and +4 (and every dy) match exactly; the shortest wins, then the smaller dx
    col = np.array([40, 80, 160, 220, 200, 120, 60, 30], np.uint8)
    stripes = pack(w, h, np.tile(col, (h, w // 8)), np.full((h, w), 128, np.uint8), np.full((h, w), 128, np.uint8))
    mv, has, ref, planes = _ipair(pkg, ctx, w, h, quality, stripes, lambda pl: pack(w, h, np.roll(pl[0], 4, axis=1), pl[1], pl[2]), R)
    y = planes[0]
    assert np.array_equal(y, np.roll(y, 8, axis=1)) and (y == y[0]).all() and not np.array_equal(y, np.roll(y, 4, axis=1)), "the reference lost its period"
    lm = mv[:nl].reshape(h // 16, w // 16, 2)
    assert (lm[:, 1:, 0] == -4).all() and (lm[:, 1:, 1] == 0).all(), lm[..., 0]
    assert (lm[:, 0, 0] == 4).all() and (lm[:, 0, 1] == 0).all(), "at the left edge dx = -4 leaves the plane: +4"
    assert (has == 0).all() and (ref.err == 0).all()
    # the same vertically: dy = -4 beats +4
    rows = pack(w, h, np.tile(col[:, None], (h // 8, w)), np.full((h, w), 128, np.uint8), np.full((h, w), 128, np.uint8))
    mv, has, ref, planes = _ipair(pkg, ctx, w, h, quality, rows, lambda pl: pack(w, h, np.roll(pl[0], 4, axis=0), pl[1], pl[2]), R)
    y = planes[0]
    assert np.array_equal(y, np.roll(y, 8, axis=0)) and (y.T == y.T[0]).all() and not np.array_equal(y, np.roll(y, 4, axis=0)), "the reference lost its period"
    lm = mv[:nl].reshape(h // 16, w // 16, 2)
    assert (lm[1:, :, 1] == -4).all() and (lm[1:, :, 0] == 0).all(), lm[..., 1]
    assert (lm[0, :, 1] == 4).all() and (lm[0, :, 0] == 0).all()
    assert (has == 0).all()
    # a longer vector with strictly smaller error than (0, 0)
    tex = moving_clip(w, h, 1, 9, noise=0)[0]

    def shifted(pl):
        out = []
        for p, (dx, dy) in zip(pl, ((5, -3), (2, -1), (2, -1))):
            q = p.copy()
            ph, pw = p.shape
            q[max(0, -dy):ph - max(0, dy), max(0, -dx):pw - max(0, dx)] = p[max(0, dy):ph - max(0, -dy), max(0, dx):pw - max(0, -dx)]
            out.append(q)
        return pack(w, h, *out)
    mv, has, ref, planes = _ipair(pkg, ctx, w, h, quality, tex, shifted, R)
    lm = mv[:nl].reshape(h // 16, w // 16, 2)
    inner = lm[1:, :-1]
    assert (inner[..., 0] == 5).all() and (inner[..., 1] == -3).all(), lm
    e0, _ = block_errors(onp.pad_plane(planes_of(shifted(planes), w, h)[0][0], 0), planes[0], 0, 0)
    assert (ref.err[:nl].reshape(h // 16, w // 16)[1:, :-1] < e0[1:, :-1]).all()


# ------------------------------------------------------------------ 3. found where the four-step search is lost
LOST_SEED = 2
LOST_VECTOR = (11, -13)


def translate(p, dx, dy):
    """out[y, x] = p[y + dy, x + dx] where that lies inside p, p[y, x] elsewhere"""
    ph, pw = p.shape
    q = p.copy()
    q[max(0, -dy):ph - max(0, dy), max(0, -dx):pw - max(0, dx)] = p[max(0, dy):ph - max(0, -dy), max(0, dx):pw - max(0, -dx)]
    return q


def lost_case(pkg, ctx, oracle, quality=5, w=304, h=80, R=15):
    """Frame A: seeded uniform noise.  Frame B: A's reconstruction after the i-frame, every PADDED plane translated by (11, -13) in its own
    pixels (edges filled from the reconstruction) and cropped to the frame.  A macroblock is EXACT when its source block lies inside the
    unpadded plane (a block that reaches into the padding has clear-colour source pixels no patch equals) and its displaced patch inside the
    padded plane: its error at (11, -13) is 0.  -> dict of what the checks compare"""
    dx, dy = LOST_VECTOR
    rng = np.random.default_rng(LOST_SEED)
    a = rng.integers(0, 256, frame_bytes(w, h), dtype=np.uint8)
    enc = pkg.EncoderSession(ctx, w, h, quality, 1)
    try:
        enc.set_motion_search("full", R)
        enc.encode_iframe(a)
        ref = RefEncoder(w, h, quality)
        ref.iframe(a)
        assert np.array_equal(enc.prev_frame()[0], ref.prev_frame())
        planes = ref.prev
        b = pack(w, h, *[translate(p, dx, dy) for p in planes])
        mv, has, _ = enc.encode_pframe(b)
    finally:
        enc.close()
    exact, four_coded, off = [], 0, 0
    t = onp.qtables(quality)
    for k, ((px, clear), p) in enumerate(zip(planes_of(b, w, h), planes)):
        ph, pw = p.shape
        bw, bh = pw // 16, ph // 16
        omv, ohas, _ = oracle.encode_plane_delta(px, p, t[2 + min(k, 1)], t[4], clear)
        for i in range(bw * bh):
            bx, by = (i % bw) * 16, (i // bw) * 16
            if bx + 16 <= px.shape[1] and by + 16 <= px.shape[0] and 0 <= bx + dx <= pw - 16 and 0 <= by + dy <= ph - 16:
                exact.append(off + i)
                four_coded += int(ohas[i])
        off += bw * bh
    return dict(a=a, b=b, mv=mv[0], has=has[0], exact=np.array(exact), four_coded=four_coded)


def check_lost(pkg, ctx, oracle, quality=5, w=304, h=80):
    """every exact macroblock comes out with exactly (11, -13) and has_coef = 0, while the oracle's four-step encoder CODES some of them
    (asserted first: were it to skip them all the input would prove nothing); and the p-frame's packet is smaller in FULL mode"""
    c = lost_case(pkg, ctx, oracle, quality, w, h)
    print(f"lost case: {c['exact'].size} exact macroblocks, the four-step oracle codes {c['four_coded']} of them")
    assert c["exact"].size >= 40 and c["four_coded"] > 0, c["four_coded"]
    assert (c["mv"][c["exact"]] == np.array(LOST_VECTOR)).all(), c["mv"][c["exact"]]
    assert (c["has"][c["exact"]] == 0).all()
    sizes = {}
    for mode in ("fourstep", "full"):
        buf = io.BytesIO()
        e = pkg.Encoder(buf, w, h, 30, quality, ctx)
        try:
            e.set_motion_search(mode, 15 if mode == "full" else 0)
            e.encode_iframe(pkg.VideoFrame.from_packed(w, h, c["a"]))
            n0 = len(buf.getvalue())
            e.encode_pframe(pkg.VideoFrame.from_packed(w, h, c["b"]))
            sizes[mode] = len(buf.getvalue()) - n0
            e.finish()
        finally:
            e.close()
    print(f"lost case: p-frame packet {sizes['fourstep']} bytes four-step, {sizes['full']} bytes full")
    assert sizes["full"] < sizes["fourstep"], sizes


# ------------------------------------------------------------------ 4. dominance
def check_dominance(pkg, ctx, oracle, w=144, h=48, quality=5, R=15):
    """on random-walk content the full search's error is <= the oracle's four-step error for every macroblock: of the restatement, and of
    the product (whose vectors are the restatement's)"""
    clip = moving_clip(w, h, 3, 77, reach=9)
    enc = pkg.EncoderSession(ctx, w, h, quality, 1)
    ref = RefEncoder(w, h, quality)
    t = onp.qtables(quality)
    try:
        enc.set_motion_search("full", R)
        enc.encode_iframe(clip[0])
        ref.iframe(clip[0])
        better = 0
        for f in clip[1:]:
            planes = [p.copy() for p in ref.prev]
            assert np.array_equal(enc.prev_frame()[0], ref.prev_frame())
            mv, _, _ = enc.encode_pframe(f)
            wmv, _, _ = ref.pframe(f, R)
            assert np.array_equal(mv[0], wmv)
            off = 0
            for k, ((px, clear), p) in enumerate(zip(planes_of(f, w, h), planes)):
                img = onp.pad_plane(px, clear)
                bw = p.shape[1] // 16
                omv, _, _ = oracle.encode_plane_delta(px, p, t[2 + min(k, 1)], t[4], clear)
                for i in range(omv.shape[0]):
                    bx, by = (i % bw) * 16, (i // bw) * 16
                    blk = img[by:by + 16, bx:bx + 16]
                    (ox, oy), (fx, fy) = (int(v) for v in omv[i]), (int(v) for v in mv[0][off + i])
                    e4 = onp.ssd(blk, p[by + oy:by + oy + 16, bx + ox:bx + ox + 16])
                    ef = onp.ssd(blk, p[by + fy:by + fy + 16, bx + fx:bx + fx + 16])
                    assert ef == ref.err[off + i] and ef <= e4, (k, i, ef, e4)
                    better += ef < e4
                off += omv.shape[0]
        assert better > 0, "the content never separates the two searches"
    finally:
        enc.close()


# ------------------------------------------------------------------ 5. streams
def decode_product(pkg, ctx, data):
    d = pkg.Decoder(io.BytesIO(data), ctx)
    got = []
    try:
        while d.advance_frame(lambda fr: got.append(fr.packed())):
            pass
    finally:
        d.close()
    return got


def decode_oracle(oracle, data):
    from oracle_bind import OracleStreamDecoder
    odec = OracleStreamDecoder(oracle, data)
    want = []
    while True:
        rc, fr = odec.advance_frame()
        assert rc >= 0
        if fr is not None:
            want.append(fr)
        if rc == 0:
            break
    return want


STREAM_CONFIGS = ("plain", "rgb", "denoise", "gop", "gop_redo")
STREAM_PATTERN = "IPPIPP"


def _planar_frames(pkg, ctx, config, w, h):
    """-> (what the encoder is handed per frame, the planar frames it encodes)"""
    clip = moving_clip(w, h, len(STREAM_PATTERN), 31, reach=10)
    if config == "rgb":
        pics = [onp.yuv420_to_rgb(f, w, h) for f in clip]
        return pics, [pkg.frames_from_rgb(ctx, w, h, p, "rgb8", "box")[0] for p in pics]
    if config == "denoise":
        return [pkg.VideoFrame.from_packed(w, h, f) for f in clip], list(pkg.frames_denoise(ctx, w, h, clip, (4, 4, 4), (3, 3, 3)))
    return [pkg.VideoFrame.from_packed(w, h, f) for f in clip], list(clip)


def check_stream(pkg, ctx, oracle, config, w=144, h=48, quality=4, R=15):
    """6 frames (I P P I P P) through a stream object in FULL mode: the bytes decode with the product's decoder AND the oracle's container
    decoder to the same frames, and those equal the restatement's closed-loop reconstruction.  "gop" / "gop_redo": pfv_gop_encoder writes
    pfv_encoder's bytes, the second with an arena small enough that every batch is made again on the one-stream redo session."""
    base = "plain" if config.startswith("gop") else config
    ins, planar = _planar_frames(pkg, ctx, base, w, h)
    buf = io.BytesIO()
    e = pkg.Encoder(buf, w, h, 30, quality, ctx)
    try:
        if base == "rgb":
            e.set_input_rgb(True, "rgb8", "box")
        if base == "denoise":
            e.set_denoise(True, (4, 4, 4), (3, 3, 3))
        e.set_motion_search("full", R)
        for c, x in zip(STREAM_PATTERN, ins):
            (e.encode_iframe if c == "I" else e.encode_pframe)(x)
        e.finish()
    finally:
        e.close()
    data = buf.getvalue()
    ref = RefEncoder(w, h, quality)
    want = []
    for c, f in zip(STREAM_PATTERN, planar):
        if c == "I":
            ref.iframe(f)
        else:
            ref.pframe(f, R)
        want.append(ref.shown())
    got, ogot = decode_product(pkg, ctx, data), decode_oracle(oracle, data)
    assert len(got) == len(ogot) == len(want)
    for t in range(len(want)):
        assert np.array_equal(got[t], want[t]), (config, t, "pfv_decoder against the restatement")
        assert np.array_equal(ogot[t], want[t]), (config, t, "the oracle's decoder against the restatement")
    if config.startswith("gop"):
        gbuf = io.BytesIO()
        if config == "gop_redo":
            os.environ["PFV_TEST_GOP_ARENA_BYTES"] = "64"
        try:
            g = pkg.GopEncoder(gbuf, w, h, 30, quality, ctx, max_gops=2, max_gop_frames=3)
        finally:
            os.environ.pop("PFV_TEST_GOP_ARENA_BYTES", None)
        try:
            g.set_motion_search("full", R)
            for c, x in zip(STREAM_PATTERN, ins):
                (g.encode_iframe if c == "I" else g.encode_pframe)(x)
            g.finish()
            st = g.stats()
        finally:
            g.close()
        assert gbuf.getvalue() == data, (config, "pfv_gop_encoder against pfv_encoder")
        assert (st["batches_redone"] >= 1) == (config == "gop_redo"), st
    # an ordinary stream, but not the four-step encoder's
    buf4 = io.BytesIO()
    e = pkg.Encoder(buf4, w, h, 30, quality, ctx)
    try:
        for c, f in zip(STREAM_PATTERN, planar):
            (e.encode_iframe if c == "I" else e.encode_pframe)(pkg.VideoFrame.from_packed(w, h, f))
        e.finish()
    finally:
        e.close()
    assert buf4.getvalue() != data


def check_graph(pkg, ctx, w=144, h=48, quality=4, R=7):
    """a session p-frame in FULL mode recorded once and replayed on new frames gives the restatement's outputs; a mode change after the
    capture does not reach the replays"""
    clip = moving_clip(w, h, 4, 57, reach=6)
    ref = RefEncoder(w, h, quality)
    enc = pkg.EncoderSession(ctx, w, h, quality, 1)
    bufs = DevBufs(ctx)
    graph = pkg.Graph(ctx)
    try:
        tb = enc.total_blocks
        enc.set_motion_search("full", R)
        src = bufs.put(clip[0])
        coef_d, mv_d, has_d = bufs.put(np.zeros(tb * 256, np.int16)), bufs.put(np.zeros(tb * 2, np.int8)), bufs.put(np.zeros(tb, np.uint8))
        enc.encode_iframe_dev(src, coef_d)
        ref.iframe(clip[0])
        ctx.upload(src, clip[1])
        enc.encode_pframe_dev(src, mv_d, has_d, coef_d)      # outside the recording first: the ping-pong index is back where the capture starts
        ref.pframe(clip[1], R)
        ctx.sync()
        # two p-frames per replay: prev[cur] -> prev[cur ^ 1] -> prev[cur], so that every replay starts from the buffer the last one left
        src2 = bufs.put(clip[2])
        with graph:
            enc.encode_pframe_dev(src, mv_d, has_d, coef_d)
            enc.encode_pframe_dev(src2, mv_d, has_d, coef_d)
        enc.set_motion_search("fourstep")
        for a, b in ((2, 3), (3, 1)):
            ctx.upload(src, clip[a])
            ctx.upload(src2, clip[b])
            graph.launch()
            ctx.sync()
            ref.pframe(clip[a], R)
            wmv, whas, wcoef = ref.pframe(clip[b], R)
            coef, mv, has = np.zeros((tb, 256), np.int16), np.zeros((tb, 2), np.int8), np.zeros(tb, np.uint8)
            ctx.download(coef, coef_d); ctx.download(mv, mv_d); ctx.download(has, has_d)
            assert np.array_equal(mv, wmv) and np.array_equal(has, whas) and np.array_equal(coef, wcoef), (a, b)
            assert np.array_equal(enc.prev_frame()[0], ref.prev_frame()), (a, b, "reconstruction")
    finally:
        graph.close()
        bufs.close()
        enc.close()


# ------------------------------------------------------------------ 6. off means off
def check_off(pkg, ctx, w=144, h=48, quality=4):
    """set_motion_search(FOURSTEP, 0), and FULL followed by FOURSTEP, give the bytes of an untouched encoder and session"""
    clip = moving_clip(w, h, 3, 91)
    outs = []
    for prep in (None, lambda o: o.set_motion_search("fourstep", 0), lambda o: (o.set_motion_search("full", 9), o.set_motion_search("fourstep", 0))):
        buf = io.BytesIO()
        e = pkg.Encoder(buf, w, h, 30, quality, ctx)
        s = pkg.EncoderSession(ctx, w, h, quality, 1)
        try:
            for o in (e, s):
                if prep:
                    prep(o)
            assert s.motion_search == (pkg.PFV_SEARCH_FOURSTEP, 0)
            res = []
            for t, f in enumerate(clip):
                (e.encode_iframe if t == 0 else e.encode_pframe)(pkg.VideoFrame.from_packed(w, h, f))
                res.append(s.encode_iframe(f) if t == 0 else s.encode_pframe(f))
            e.finish()
            outs.append((buf.getvalue(), res, s.prev_frame()))
        finally:
            e.close()
            s.close()
    for other in outs[1:]:
        assert other[0] == outs[0][0]
        assert np.array_equal(other[2], outs[0][2])
        assert np.array_equal(other[1][0], outs[0][1][0])
        for t in (1, 2):
            assert all(np.array_equal(x, y) for x, y in zip(other[1][t], outs[0][1][t]))


# ------------------------------------------------------------------ 7. refusals
def check_refusals(pkg, ctx, w=48, h=32, quality=4):
    lib, L = ctx._lib, pkg._lib
    FULL, FOUR = L.PFV_SEARCH_FULL, L.PFV_SEARCH_FOURSTEP
    clip = moving_clip(w, h, 4, 13)
    frames = [pkg.VideoFrame.from_packed(w, h, f) for f in clip]
    s = pkg.EncoderSession(ctx, w, h, None, 1, qualities=[2, 5])
    buf = io.BytesIO()
    e = pkg.Encoder(buf, w, h, 30, None, ctx, qualities=[2, 5])
    gbuf = io.BytesIO()
    g = pkg.GopEncoder(gbuf, w, h, 30, quality, ctx, max_gops=2, max_gop_frames=2)
    bufs = DevBufs(ctx)

    def mode(sess):
        m, r = ctypes.c_int(-1), ctypes.c_int(-1)
        assert lib.pfv_enc_session_get_motion_search(sess.handle, ctypes.byref(m), ctypes.byref(r)) == L.PFV_OK
        return m.value, r.value

    def is_full(encoder):
        """pfv_encoder has no getter: its p-frame probe calls answer PFV_ERR_STATE exactly while its session is in FULL mode"""
        try:
            encoder.probe_pframe(frames[1])
            return False
        except pkg.PfvError as err:
            assert err.code == L.PFV_ERR_STATE
            return True
    try:
        # null handles
        assert lib.pfv_enc_session_set_motion_search(None, FULL, 7) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_enc_session_get_motion_search(None, None, None) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_encoder_set_motion_search(None, FULL, 7) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_gop_encoder_set_motion_search(None, FULL, 7) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_enc_session_get_motion_search(s.handle, None, None) == L.PFV_OK
        # bad mode, radius 0 and 16 in FULL: the mode stays, the next valid call works
        s.set_motion_search("full", 5)
        for fn, h_ in ((lib.pfv_enc_session_set_motion_search, s.handle), (lib.pfv_encoder_set_motion_search, e.handle), (lib.pfv_gop_encoder_set_motion_search, g.handle)):
            for m, r in ((2, 7), (-1, 7), (FULL, 0), (FULL, 16), (FULL, -1)):
                assert fn(h_, m, r) == L.PFV_ERR_BAD_ARG, (m, r)
        assert mode(s) == (FULL, 5)
        s.set_motion_search("full", 15)
        assert mode(s) == (FULL, 15)
        s.set_motion_search("fourstep", 99)          # the radius is ignored
        assert mode(s) == (FOUR, 0)
        # the session's p-frame probes in FULL mode; the i-frame probes go on working
        s.encode_iframe(clip[0])
        s.set_motion_search("full", 7)
        n_r = 2
        sizes_d, sse_d, q24_d, src_d = bufs.put(np.zeros(n_r, np.uint32)), bufs.put(np.zeros(n_r * 3, np.uint64)), bufs.put(np.zeros(n_r * 3, np.int64)), bufs.put(clip[1])
        for call in (lambda: s.probe_pframe(clip[1]), lambda: s.probe_pframe_rd(clip[1]), lambda: s.probe_pframe_ssim(clip[1]),
                     lambda: s.probe_pframe_dev(src_d, sizes_d), lambda: s.probe_pframe_rd_dev(src_d, sizes_d, sse_d),
                     lambda: s.probe_pframe_ssim_dev(src_d, sizes_d, sse_d, q24_d)):
            with pytest.raises(pkg.PfvError) as err:
                call()
            assert err.value.code == L.PFV_ERR_STATE
        assert mode(s) == (FULL, 7)
        assert s.probe_iframe(clip[1]).shape == (1, n_r)
        full_out = s.encode_pframe(clip[1])
        s.set_motion_search("fourstep")
        assert s.probe_pframe(clip[2]).shape == (1, n_r)          # and the p-frame probes are back
        assert full_out[0].shape == (1, s.total_blocks, 2)
        # pfv_encoder: FULL against the p-frame probe, the two p-frame floors and encode_frame, in both orders
        e.encode_iframe(frames[0])
        switches = ((e.set_pframe_probe, True, False), (e.set_pframe_quality_floor, 30.0, 0.0), (e.set_pframe_ssim_floor, 0.5, 0.0))
        for setter, on, off in switches:
            setter(on)
            with pytest.raises(pkg.PfvError) as err:
                e.set_motion_search("full", 7)
            assert err.value.code == L.PFV_ERR_STATE and not is_full(e)
            e.set_motion_search("fourstep")                       # not refused
            setter(off)
            e.set_motion_search("full", 7)
            with pytest.raises(pkg.PfvError) as err:
                setter(on)
            assert err.value.code == L.PFV_ERR_STATE
            setter(off)                                           # switching off is not refused
            assert is_full(e)
            e.set_motion_search("fourstep")
        e.set_motion_search("full", 7)
        n0 = len(buf.getvalue())
        with pytest.raises(pkg.PfvError) as err:
            e.encode_frame(frames[1])
        assert err.value.code == L.PFV_ERR_STATE and len(buf.getvalue()) == n0
        for name in ("probe_pframe", "probe_pframe_rd", "probe_pframe_ssim"):
            with pytest.raises(pkg.PfvError) as err:
                getattr(e, name)(frames[1])
            assert err.value.code == L.PFV_ERR_STATE
        e.probe_iframe(frames[1])
        e.set_rate(100000)                                         # unaffected
        e.set_rung(1)
        e.encode_pframe(frames[1])
        assert len(buf.getvalue()) > n0
        e.set_motion_search("fourstep")
        assert e.encode_frame(frames[2]) in (1, 2, 3)
        e.finish()
        # pfv_gop_encoder: a change while a batch is in flight
        g.set_motion_search("full", 7)
        for t in range(4):                                         # two groups of two fill the batch: it is submitted, the next one collects it
            (g.encode_iframe if t % 2 == 0 else g.encode_pframe)(frames[t])
        g.encode_iframe(frames[0])
        in_flight = lib.pfv_gop_encoder_set_motion_search(g.handle, FOUR, 0)
        assert in_flight == L.PFV_ERR_STATE, in_flight
        g.flush()
        g.set_motion_search("fourstep")
        g.encode_pframe(frames[1])
        g.finish()
        # the refused call changed nothing and the accepted one did: pfv_encoder's bytes under the same sequence of modes
        tbuf = io.BytesIO()
        twin = pkg.Encoder(tbuf, w, h, 30, quality, ctx)
        try:
            twin.set_motion_search("full", 7)
            for t in range(4):
                (twin.encode_iframe if t % 2 == 0 else twin.encode_pframe)(frames[t])
            twin.encode_iframe(frames[0])
            twin.set_motion_search("fourstep")
            twin.encode_pframe(frames[1])
            twin.finish()
        finally:
            twin.close()
        assert gbuf.getvalue() == tbuf.getvalue()
    finally:
        bufs.close()
        s.close()
        e.close()
        g.close()


# ------------------------------------------------------------------ 8. mirrors and tool
def build_cpp(lib_path, exe):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "search_report.cpp"), "-o", exe, lib_path, "-Wl,-rpath," + os.path.dirname(lib_path)], check=True)


def check_cpp(pkg, ctx, exe, tmp_path, w=80, h=48, quality=4, R=7):
    """tests/cpp/search_report.cpp (pfv::EncoderSession / Encoder / GopEncoder ::set_motion_search) prints the vectors and packet sizes of the
    Python path"""
    clip = moving_clip(w, h, 3, 41, reach=6)
    src = str(tmp_path / "in.yuv")
    clip.tofile(src)
    r = subprocess.run([exe, src, str(w), str(h), str(quality), str(R)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = []
    s = pkg.EncoderSession(ctx, w, h, quality, 1)
    buf = io.BytesIO()
    e = pkg.Encoder(buf, w, h, 30, quality, ctx)
    try:
        s.set_motion_search("full", R)
        e.set_motion_search("full", R)
        for t, f in enumerate(clip):
            n0 = len(buf.getvalue())
            if t == 0:
                s.encode_iframe(f)
                e.encode_iframe(pkg.VideoFrame.from_packed(w, h, f))
            else:
                mv, has, _ = s.encode_pframe(f)
                e.encode_pframe(pkg.VideoFrame.from_packed(w, h, f))
                lines.append(f"frame {t} mv " + " ".join(f"{int(x)},{int(y)}" for x, y in mv[0]))
                lines.append(f"frame {t} coded {int(has.sum())}")
            lines.append(f"frame {t} packet {len(buf.getvalue()) - n0}")
        e.finish()
    finally:
        s.close()
        e.close()
    lines.append(f"gop stream {len(buf.getvalue())} bytes identical")
    lines.append(f"mode full radius {R}")
    assert r.stdout.splitlines() == lines


def check_rd_tool(pkg, lib_path, tmp_path, w=64, h=48, n_frames=4, gop=3, qualities=(2, 5), R=7):
    """tools/rd_curve.py --search full,7 on the library at lib_path: without the flag the lines are the same minus the new keys; the full_ and
    four_ columns equal a recomputation through the package; --time-search prints its row"""
    env = dict(os.environ)
    if lib_path:
        env["PFV_HIP_LIB"] = lib_path
    cmd = [sys.executable, os.path.join(ROOT, "tools", "rd_curve.py"), str(w), str(h), str(n_frames), "--gop", str(gop), "--kind", "pan",
           "--qualities", ",".join(str(q) for q in qualities)]
    plain = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert plain.returncode == 0, plain.stderr
    r = subprocess.run(cmd + ["--search", f"full,{R}"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr
    lines = [json.loads(x) for x in r.stdout.splitlines()]
    stripped = [{k: v for k, v in d.items() if not k.startswith(("full_", "four_", "search_"))} for d in lines]
    assert [json.dumps(d) for d in stripped] == plain.stdout.splitlines()
    for d in lines:
        assert d["search_radius"] == R
        for col in ("stream_bytes", "psnr_yuv", "coded", "skipped"):
            assert f"full_{col}" in d and f"four_{col}" in d, (col, d)
        assert d["full_coded"] + d["full_skipped"] == d["four_coded"] + d["four_skipped"] > 0
        assert d["four_stream_bytes"] == d["stream_bytes"]
    return lines


def check_time_tool(lib_path, w=64, h=48):
    """tools/rd_curve.py --time-search at a toy size (the row's shape; the 96 x 1080p figures are a GPU run's, profiles/full_search.md)"""
    env = dict(os.environ)
    if lib_path:
        env["PFV_HIP_LIB"] = lib_path
    cmd = [sys.executable, os.path.join(ROOT, "tools", "rd_curve.py"), str(w), str(h), "2", "--qualities", "5", "--time-search"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr
    row = json.loads(r.stdout.splitlines()[-1])["time_search"]
    assert row["streams"] == 2 and all(row[k] >= 0 for k in ("fourstep_ms", "full_r7_ms", "full_r15_ms"))      # the emulator's events read 0
    return row


# ------------------------------------------------------------------ 9. every radius, the match in the corner of the square
SWEEP_SHAPE = (144, 80)      # the smallest frame with two luma tiles across and two down: luma strips of 8 and of 1 macroblock, a partial
SWEEP_SEED = 23              # 64-macroblock transform group, room for a +-62 vector
SWEEP_QUALITY = 2
SWEEP_RADII = list(range(1, 16))
_SWEEP_FIRST = {}


def sweep_first(w=SWEEP_SHAPE[0], h=SWEEP_SHAPE[1]):
    if (w, h) not in _SWEEP_FIRST:
        _SWEEP_FIRST[w, h] = moving_clip(w, h, 1, SWEEP_SEED, noise=0)[0]
    return _SWEEP_FIRST[w, h]


def inside_blocks(pw, ph, dx, dy):
    """luma macroblocks of a pw x ph plane whose block displaced by (dx, dy) lies inside it"""
    bw = pw // 16
    return np.array([by * bw + bx for by in range(ph // 16) for bx in range(bw) if 0 <= bx * 16 + dx <= pw - 16 and 0 <= by * 16 + dy <= ph - 16], np.int64)


def corner_model_check(dx, dy, coarse):
    """of the restatement: every inside macroblock carries exactly (dx, dy) with E = 0 and has_coef = 0 (HIER: and the coarse vector
    (dx / 2, dy / 2)), and there is one"""
    def check(ref, planes, wmv, whas, wcoef):
        ph, pw = planes[0].shape
        ins = inside_blocks(pw, ph, dx, dy)
        assert ins.size > 0, (dx, dy)
        assert (wmv[ins] == np.array([dx, dy])).all(), (dx, dy, wmv[ins])
        assert (ref.err[ins] == 0).all() and (whas[ins] == 0).all() and (wcoef[ins] == 0).all(), (dx, dy)
        if coarse:
            assert (ref.cmv[ins] == np.array([dx // 2, dy // 2])).all(), (dx, dy, ref.cmv[ins])
    return check


def check_sweep(pkg, ctx, R, w=SWEEP_SHAPE[0], h=SWEEP_SHAPE[1]):
    """I then P at radius R: the p-frame is the i-frame's reconstruction with the luma plane translated by (R, -R), then by (-R, R) -- the
    exact match is the corner candidate of the square, in the last column and the first row of the kernel's walk, then the first column
    and the last row.  Asserted on the restatement first (corner_model_check), then device == restatement (_ipair)."""
    for dx, dy in ((R, -R), (-R, R)):
        _ipair(pkg, ctx, w, h, SWEEP_QUALITY, sweep_first(w, h), lambda pl: pack(w, h, translate(pl[0], dx, dy), pl[1], pl[2]), R,
               model_check=corner_model_check(dx, dy, False))


# ------------------------------------------------------------------ 10. ladder rungs
LADDER_SHAPE = (50, 38)          # ladder_cases' own
LADDER_R = 8
LADDER_SESSION_PLAN = [("I", 3), ("P", 0), ("P", 4), ("P", 1)]      # the rung changes between p-frames: the reference plane is another rung's
LADDER_ENCODER_PLAN = [("I", 3), ("P", 0), ("D", None), ("P", 4), ("I", 1), ("P", None), ("P", 2)]


class SearchLadderModel(lc.LadderModel):
    """ladder_cases.LadderModel with the p-frames of a motion-search mode: plane_encoder(px, ref, q, px_err, clear) -> (mv, has, coef, E, ...)
    with the rung's inter tables and px_err.  .err[k]: E of the vectors of slot k's last p-frame"""

    def __init__(self, oracle, w, h, qualities, n_streams=1, plane_encoder=None):
        super().__init__(oracle, w, h, qualities, n_streams)
        self.plane_encoder = plane_encoder
        self.err = [None] * n_streams

    def pframe(self, k, frame, rung):
        el, ec, px_err = self.tabs[rung][2], self.tabs[rung][3], self.tabs[rung][4]
        mvs, hass, coefs, recon, errs = [], [], [], [], []
        for p, px in enumerate(lc.split(frame, self.w, self.h)):
            q, ref = (el if p == 0 else ec), self.prev[k][p]
            mv, has, c, err = self.plane_encoder(px, ref, q, px_err, self.CLEAR[p])[:4]
            recon.append(self.o.decode_plane_delta(mv, has, c, ref.shape[1] // 16, ref.shape[0] // 16, q, ref))
            mvs.append(mv); hass.append(has); coefs.append(c); errs.append(err)
        self.prev[k] = recon
        self.err[k] = np.concatenate(errs)
        return np.concatenate(mvs), np.concatenate(hass), np.concatenate(coefs)

    def has_at(self, k, rung):
        """has_coef of the last p-frame of slot k had the skip threshold been `rung`'s (the vectors and E do not depend on it)"""
        px_err = self.tabs[rung][4]
        return (~(self.err[k].astype(np.float32) <= np.float32(px_err) * np.float32(px_err) * np.float32(256.0))).astype(np.uint8)


def full_ladder_model(oracle, w, h, qualities, n=1, R=LADDER_R):
    return SearchLadderModel(oracle, w, h, qualities, n, lambda px, ref, q, px_err, clear: encode_plane_full(px, ref, q, px_err, clear, R))


def check_ladder_session(pkg, ctx, oracle, mode, R, make_model, n=3):
    """I at rung 3, P at rung 0, P at rung 4, P at rung 1 of three streams in `mode`: mv, has_coef, coefficients, payloads and the next
    reference equal the mode's ladder model at the rung of the frame.  Of the model first: at every rung > 0 some macroblock's has_coef is
    not what rung 0's px_err would give -- else the case could not see a wrong skip threshold -- and some macroblock is coded."""
    w, h = LADDER_SHAPE
    model = make_model(oracle, w, h, lc.LADDER, n, R)
    clips = [[f.copy() for f in lc.motion_clip(w, h, 11 + k, len(LADDER_SESSION_PLAN))] for k in range(n)]
    rng = np.random.default_rng(17)
    want = []
    for t, (kind, rung) in enumerate(LADDER_SESSION_PLAN):
        row = []
        for k in range(n):
            if t == len(LADDER_SESSION_PLAN) - 1:
                # rung 0's px_err is 0 and rung 1's 3.0: the left 32 luma columns become the picture shown so far with noise of +-2, an
                # error of about 2 per pixel, which rung 1 skips and rung 0 would code
                y, shown = clips[k][t][:w * h].reshape(h, w), model.shown(k)[:w * h].reshape(h, w)
                y[:, :32] = np.clip(shown[:, :32].astype(np.int64) + rng.integers(-2, 3, (h, 32)), 0, 255)
            if kind == "I":
                coef = model.iframe(k, clips[k][t], rung)
                row.append((None, None, coef, model.payload_i(coef, rung), model.prev_frame(k), None))
            else:
                mv, has, coef = model.pframe(k, clips[k][t], rung)
                row.append((mv, has, coef, model.payload_p(mv, has, coef, rung), model.prev_frame(k), model.has_at(k, 0)))
        if kind == "P" and rung > 0:
            assert any((r[1] != r[5]).any() for r in row), (t, rung, "rung 0's px_err gives the same has_coef")
            assert any(r[1].any() for r in row), (t, rung, "nothing coded: the inter tables are not used")
        want.append(row)
    rig = lc.SessionRig(pkg, ctx, w, h, lc.LADDER, n)
    try:
        rig.enc.set_motion_search(mode, R)
        for t, (kind, rung) in enumerate(LADDER_SESSION_PLAN):
            got = rig.step(np.stack([clips[k][t] for k in range(n)]), kind == "P", rung)
            assert rig.enc.rung == rung
            for k in range(n):
                mv, has, coef, pay, prev, _ = want[t][k]
                if kind == "P":
                    assert np.array_equal(got["mv"][k], mv), (t, k, "motion vectors")
                    assert np.array_equal(got["has"][k], has), (t, k, "has_coef", np.nonzero(got["has"][k] != has)[0][:8])
                assert np.array_equal(got["coef"][k], coef), (t, k, "coefficients")
                assert np.array_equal(got["prev"][k], prev), (t, k, "reconstruction")
                assert np.array_equal(rig.enc.prev_frame()[k], prev), (t, k, "prev_frame()")
                assert got["payloads"][k] == pay, (t, k, len(got["payloads"][k]), len(pay))
    finally:
        rig.close()


def check_ladder_encoder(pkg, ctx, oracle, mode, R, make_model, device_entropy):
    """ladder_cases.check_encoder_ladder's plan through pfv_encoder in `mode`: the bytes are the mode's model's, both decoders show its frames"""
    w, h = LADDER_SHAPE
    plan = LADDER_ENCODER_PLAN
    frames = lc.motion_clip(w, h, 41, len(plan))
    data, rungs = lc.run_encoder(pkg, ctx, w, h, frames, plan, device_entropy, qualities=lc.LADDER, search=(mode, R))
    assert rungs == [3, 0, 0, 4, 1, 1, 2]
    full = [(kind, r if r is not None or kind == "D" else rungs[t]) for t, (kind, r) in enumerate(plan)]
    model = make_model(oracle, w, h, lc.LADDER, 1, R)
    want, shown = lc.model_stream(model, frames, full)
    assert data == want, (len(data), len(want))
    got, ofr = lc.decode_both(pkg, ctx, oracle, data)
    assert len(ofr) == len(plan)
    for t, (s, o) in enumerate(zip(shown, ofr)):
        if s is not None:
            assert o is not None and np.array_equal(o, s), t
    delivered = [o for o in ofr if o is not None]
    assert len(got) == len(delivered) and all(np.array_equal(a, b) for a, b in zip(got, delivered))


# ------------------------------------------------------------------ 11. k_pf_transform's groups
GROUPS_R = 4
GROUPS_VECTOR = (3, -2)
# 144 x 80: luma is 9 x 5 macroblocks in 10 strips (strip 2 by: 8 macroblocks, strip 2 by + 1: the one at bx = 8), k_pf_transform takes strips
# 0 .. 7 (rows 0 .. 3) as group 0 and strips 8, 9 (row 4) as group 1; each 5 x 3 chroma plane is three strips in one group.  (by, bx):
_G0_EIGHT = [(0, 0), (0, 7), (0, 8), (1, 2), (2, 8), (3, 0), (3, 7), (3, 8)]
GROUP_SETS = {
    "one": [(2, 3)],
    "eight_in_group0": _G0_EIGHT,
    "nine_in_group0": _G0_EIGHT + [(1, 5)],
    "one_macroblock_strips": [(by, 8) for by in range(5)],
    "group1_only": [(4, bx) for bx in range(9)],
    "all": "all",
}


def groups_second(planes, w, h, name):
    """-> (the p-frame, the macroblocks that must come out coded).  Every luma macroblock's source is the reconstruction's patch displaced by
    (3, -2) -- where that leaves the plane (the top row, the right column) the component is clamped to 0, a plain translation would leave
    those 13 macroblocks without an exact match -- and chroma is the reconstruction: nothing is coded.  Then the macroblocks of the set
    become random bytes."""
    y = planes[0].copy()
    ph, pw = y.shape
    bw = pw // 16
    for by in range(ph // 16):
        for bx in range(bw):
            vx, vy = min(GROUPS_VECTOR[0], pw - 16 - bx * 16), max(GROUPS_VECTOR[1], -by * 16)
            y[by * 16:by * 16 + 16, bx * 16:bx * 16 + 16] = planes[0][by * 16 + vy:by * 16 + vy + 16, bx * 16 + vx:bx * 16 + vx + 16]
    rng = np.random.default_rng(77)
    nl = bw * (ph // 16)
    if GROUP_SETS[name] == "all":
        f = rng.integers(0, 256, frame_bytes(w, h), dtype=np.uint8)
        return f, np.arange(nl + 2 * (planes[1].shape[0] // 16) * (planes[1].shape[1] // 16))
    for by, bx in GROUP_SETS[name]:
        y[by * 16:by * 16 + 16, bx * 16:bx * 16 + 16] = rng.integers(0, 256, (16, 16), dtype=np.uint8)
    return pack(w, h, y, planes[1], planes[2]), np.array(sorted(by * bw + bx for by, bx in GROUP_SETS[name]))


def check_groups(pkg, ctx, name, transform, w=SWEEP_SHAPE[0], h=SWEEP_SHAPE[1]):
    """FULL at radius 4 under PFV_OPT_ENC_TRANSFORM = transform.  Of the restatement: exactly the chosen set is coded, an uncoded
    macroblock's coefficients are zero and its reconstruction is the displaced patch; then device == restatement (_ipair), so the same
    holds of the device's outputs."""
    opt = pkg._lib.PFV_OPT_ENC_TRANSFORM
    chosen = {}

    def second(planes):
        f, chosen["set"] = groups_second(planes, w, h, name)
        return f

    def model(ref, planes, wmv, whas, wcoef):
        assert np.array_equal(np.nonzero(whas)[0], chosen["set"]), (name, np.nonzero(whas)[0], chosen["set"])
        assert (wcoef[whas == 0] == 0).all() and (np.abs(wcoef[whas == 1]).sum(axis=1) > 0).all()
        off = 0
        for before, after in zip(planes, ref.prev):
            bw, bh = before.shape[1] // 16, before.shape[0] // 16
            for i in range(bw * bh):
                if not whas[off + i]:
                    bx, by, (vx, vy) = (i % bw) * 16, (i // bw) * 16, (int(v) for v in wmv[off + i])
                    assert np.array_equal(after[by:by + 16, bx:bx + 16], before[by + vy:by + vy + 16, bx + vx:bx + vx + 16]), (name, off + i)
            off += bw * bh
    before = ctx.get_option(opt)
    ctx.set_option(opt, transform)
    try:
        _ipair(pkg, ctx, w, h, SWEEP_QUALITY, sweep_first(w, h), second, GROUPS_R, model_check=model)
    finally:
        ctx.set_option(opt, before)


# ------------------------------------------------------------------ 12. the largest error
LARGEST_SHAPE = (48, 32)
LARGEST_E = 256 * 255 * 255          # one short step below 2^24: the headroom of the 64-bit keys and the u32 sums


def largest_frames(w, h, first_value):
    grey = np.full((h, w), 128, np.uint8)
    return [pack(w, h, np.full((h, w), v, np.uint8), grey, grey) for v in (first_value, 255 - first_value)]


def largest_model_check(w, h, coarse):
    def check(ref, planes, wmv, whas, wcoef):
        nl = (w // 16) * (h // 16)
        assert all((p == p.flat[0]).all() for p in planes) and planes[0].flat[0] in (0, 255), "the reconstruction is not flat"
        assert (ref.err[:nl] == LARGEST_E).all() and LARGEST_E < 1 << 24, ref.err     # flat against flat: E of every candidate
        assert (wmv == 0).all() and (whas[:nl] == 1).all() and (whas[nl:] == 0).all()
        if coarse:
            assert (ref.cmv == 0).all()
    return check


def check_largest(pkg, ctx, w=LARGEST_SHAPE[0], h=LARGEST_SHAPE[1], R=15):
    """luma all 0 then all 255, and the other way round: every candidate of every luma macroblock has E = 256 x 255^2, (0, 0) wins, all are coded"""
    for v in (0, 255):
        first, second = largest_frames(w, h, v)
        _ipair(pkg, ctx, w, h, SWEEP_QUALITY, first, lambda pl: second, R, model_check=largest_model_check(w, h, False))
