"""Shared checks of the wide-range hierarchical motion search (PFV_SEARCH_HIER: k_halve + k_pf_search_coarse + k_pf_refine + k_pf_transform,
pfv_*_set_motion_search, pfv_enc_session_coarse_vectors), run by tests/test_emu_hier.py on the CPU emulator build of the kernel sources and
by tests/test_gpu_hier.py on the MI355X at the same shapes.

The expected values come from a numpy restatement of the rule in include/pfv_hip_ext.h ("wide-range hierarchical motion search"): `halve`,
`coarse_search`, `fine_search`, composed with the oracle's pad_plane, encode_blocks_delta and decode_plane_delta as tests/search_cases.py
does for PFV_SEARCH_FULL.  Every comparison with the device is an equality."""
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
import pfv_oracle_entropy_np as oen
import search_cases as sc
from search_cases import DevBufs, even, frame_bytes, pack, planes_of, qtabs, translate

ROOT = sc.ROOT

SHAPES = [(16, 16), (18, 34), (160, 144), (304, 208)]
RADII = [2, 30, 62]
QUALITIES = (2, 8)
N_STREAMS = 3
CLIP_REACH = 40          # the moving clip's jump per frame, beyond the +-15 of the other two searches


# ------------------------------------------------------------------ the restatement
def halve(p):
    """step 1: the 2 x 2 rounded mean"""
    p = p.astype(np.int64)
    return ((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def _errors(img, ref, dx, dy, B, margin):
    """SSD of every B x B block of img against ref displaced by (dx, dy), and whether the displaced block lies inside the plane"""
    ph, pw = img.shape
    bh, bw = ph // B, pw // B
    by, bx = np.mgrid[0:bh, 0:bw] * B
    ok = (bx + dx >= 0) & (bx + dx <= pw - B) & (by + dy >= 0) & (by + dy <= ph - B)
    big = np.zeros((ph + 2 * margin, pw + 2 * margin), np.int64)
    big[margin:margin + ph, margin:margin + pw] = ref
    d = img.astype(np.int64) - big[margin + dy:margin + dy + ph, margin + dx:margin + dx + pw]
    return (d * d).reshape(bh, B, bw, B).sum(axis=(1, 3)), ok


def coarse_search(hs, hp, rc):
    """step 2 -> int8 [n, 2]: the lexicographic minimum of (Ec, |cx| + |cy|, cy, cx) over the candidates inside the half plane"""
    ph, pw = hs.shape
    best = np.full((ph // 8, pw // 8), np.iinfo(np.int64).max, np.int64)
    for cy in range(-rc, rc + 1):
        for cx in range(-rc, rc + 1):
            e, ok = _errors(hs, hp, cx, cy, 8, 32)
            key = (e << 24) | ((abs(cx) + abs(cy)) << 16) | ((cy + 32) << 8) | (cx + 32)          # Ec < 2^22
            best = np.where(ok & (key < best), key, best)
    best = best.reshape(-1)
    return np.stack([(best & 255) - 32, ((best >> 8) & 255) - 32], axis=1).astype(np.int8)


def fine_search(img, ref, cmv):
    """step 3 -> (mv int8 [n, 2], E int64 [n]): (0, 0) and the 25 vectors round twice the coarse one, |component| <= 63, inside the plane"""
    ph, pw = img.shape
    bh, bw = ph // 16, pw // 16
    n = bh * bw
    by, bx = (np.mgrid[0:bh, 0:bw] * 16).reshape(2, n)
    blocks = img.astype(np.int64).reshape(bh, 16, bw, 16).transpose(0, 2, 1, 3).reshape(n, 16, 16)
    views = np.lib.stride_tricks.sliding_window_view(ref.astype(np.int64), (16, 16))
    best = np.full(n, np.iinfo(np.int64).max, np.int64)
    cands = [(0, 0, True)] + [(rx, ry, False) for ry in range(-2, 3) for rx in range(-2, 3)]
    for rx, ry, zero in cands:
        dx = np.zeros(n, np.int64) if zero else 2 * cmv[:, 0].astype(np.int64) + rx
        dy = np.zeros(n, np.int64) if zero else 2 * cmv[:, 1].astype(np.int64) + ry
        ok = (abs(dx) <= 63) & (abs(dy) <= 63) & (bx + dx >= 0) & (bx + dx <= pw - 16) & (by + dy >= 0) & (by + dy <= ph - 16)
        d = blocks - views[np.where(ok, by + dy, 0), np.where(ok, bx + dx, 0)]
        e = (d * d).sum(axis=(1, 2))
        key = (e << 24) | ((abs(dx) + abs(dy)) << 16) | ((dy + 64) << 8) | (dx + 64)              # E < 2^24
        best = np.where(ok & (key < best), key, best)
    mv = np.stack([(best & 255) - 64, ((best >> 8) & 255) - 64], axis=1).astype(np.int8)
    return mv, best >> 24


def encode_plane_hier(px, ref, q, px_err, clear, R):
    """steps 1 .. 4: the rule, then the existing operator (tests/search_cases.py: encode_plane_full's tail)"""
    img = onp.pad_plane(px, clear)
    bw = img.shape[1] // 16
    cmv = coarse_search(halve(img), halve(ref), R // 2)
    mv, err = fine_search(img, ref, cmv)
    min_err = np.float32(px_err) * np.float32(px_err) * np.float32(256.0)
    has = (~(err.astype(np.float32) <= min_err)).astype(np.uint8)
    coef = np.zeros((mv.shape[0], 256), np.int16)
    blocks = onp._gather(img)
    idx = np.nonzero(has)[0]
    if idx.size:
        prev = np.stack([ref[(i // bw) * 16 + mv[i, 1]:(i // bw) * 16 + mv[i, 1] + 16, (i % bw) * 16 + mv[i, 0]:(i % bw) * 16 + mv[i, 0] + 16] for i in idx])
        delta = np.clip(blocks[idx].astype(np.int64) - prev.astype(np.int64), -255, 255)
        coef[idx] = onp.encode_blocks_delta(delta, q)
    return mv, has, coef, err, cmv


class RefEncoder(sc.RefEncoder):
    """the hot-path half of the encoder in numpy, p-frames by the hierarchical search; .cmv: the coarse vectors of the last p-frame,
    .err: E of the chosen vectors, .err0: E(0, 0)"""

    def pframe(self, frame, R):
        mvs, hass, coefs, prev, errs, cmvs, err0 = [], [], [], [], [], [], []
        for k, (px, clear) in enumerate(planes_of(frame, self.w, self.h)):
            q = self.q[2 + min(k, 1)]
            ref = self.prev[k]
            mv, has, coef, err, cmv = encode_plane_hier(px, ref, q, self.px_err, clear, R)
            err0.append(sc.block_errors(onp.pad_plane(px, clear), ref, 0, 0)[0].reshape(-1))
            prev.append(onp.decode_plane_delta(mv, has, coef, ref.shape[1] // 16, ref.shape[0] // 16, q, ref))
            mvs.append(mv); hass.append(has); coefs.append(coef); errs.append(err); cmvs.append(cmv)
        self.prev = prev
        self.err, self.err0, self.cmv = np.concatenate(errs), np.concatenate(err0), np.concatenate(cmvs)
        return np.concatenate(mvs), np.concatenate(hass), np.concatenate(coefs)


_REF_CACHE = {}


def reference_run(w, h, quality, R, seeds, n_frames=3):
    """per seed the restatement's outputs of I P P: (clip, [(outputs, prev_frame, coarse vectors) per frame]); computed once per case"""
    key = (w, h, quality, R, tuple(seeds), n_frames)
    if key not in _REF_CACHE:
        res = []
        for s in seeds:
            clip = sc.moving_clip(w, h, n_frames, s, reach=CLIP_REACH)
            ref = RefEncoder(w, h, quality)
            steps = [(ref.iframe(clip[0]), ref.prev_frame(), None)]
            for t in range(1, n_frames):
                steps.append((ref.pframe(clip[t], R), ref.prev_frame(), ref.cmv))
            res.append((clip, steps))
        _REF_CACHE[key] = res
    return _REF_CACHE[key]


def shape_seeds(w, h):
    return [101 * w + h + k for k in range(N_STREAMS)]


# ------------------------------------------------------------------ 1. shapes x radii, 2. the coarse level alone
def check_shape(pkg, ctx, w, h, R, qualities=QUALITIES):
    """I P P of three streams with distinct content at qualities 2 and 8: mv, has_coef, coefficients, the coarse vectors and the next
    reconstruction equal the restatement's.  Quality 2 runs a second time through the device entry points with the window on slots 1..2 of
    3 and a frame stride, into pre-filled buffers: the same values there, slot 0 untouched."""
    w, h = even(w), even(h)
    n, fb = N_STREAMS, frame_bytes(w, h)
    seeds = shape_seeds(w, h)
    for quality in qualities:
        runs = reference_run(w, h, quality, R, seeds)
        if R == 62 and min(w, h) >= 144:
            # the 7-bit field beyond what the half-resolution level alone would reach: asserted on the restatement.  The two small shapes
            # cannot hold such a vector: their padded planes are at most 32 x 48.
            allmv = np.concatenate([runs[k][1][t][0][0].reshape(-1) for k in range(n) for t in (1, 2)])
            assert allmv.max() > 31 and allmv.min() < -31, (allmv.min(), allmv.max())
        enc = pkg.EncoderSession(ctx, w, h, quality, n)
        dec = pkg.DecoderSession(ctx, w, h, qtabs(pkg, quality), n)
        try:
            enc.set_motion_search("hier", R)
            assert enc.motion_search == (pkg.PFV_SEARCH_HIER, R)
            for t in range(3):
                frames = np.stack([runs[k][0][t] for k in range(n)])
                if t == 0:
                    coef = enc.encode_iframe(frames)
                    dec.decode_iframe(coef)
                    for k in range(n):
                        assert np.array_equal(coef[k], runs[k][1][0][0]), (quality, k, "i-frame coefficients")
                else:
                    mv, has, coef = enc.encode_pframe(frames)
                    cmv = enc.coarse_vectors()
                    dec.decode_pframe(mv, has, coef)
                    for k in range(n):
                        wmv, whas, wcoef = runs[k][1][t][0]
                        assert np.array_equal(cmv[k], runs[k][1][t][2]), (quality, t, k, "coarse vectors", np.nonzero((cmv[k] != runs[k][1][t][2]).any(axis=1))[0][:8])
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
    quality = qualities[0]
    runs = reference_run(w, h, quality, R, seeds)
    stride = fb + 48
    enc = pkg.EncoderSession(ctx, w, h, quality, n)
    bufs = DevBufs(ctx)
    try:
        tb = enc.total_blocks
        enc.set_motion_search("hier", R)
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
            if t:
                cmv = enc.coarse_vectors()
                assert cmv.shape == (2, tb, 2)
            for k in (1, 2):
                want = runs[k][1][t]
                if t == 0:
                    assert np.array_equal(coef[k], want[0]), (t, k, "window: coefficients")
                else:
                    assert np.array_equal(mv[k], want[0][0]) and np.array_equal(has[k], want[0][1]) and np.array_equal(coef[k], want[0][2]), (t, k, "window")
                    assert np.array_equal(cmv[k - 1], want[2]), (t, k, "window: coarse vectors")
                assert np.array_equal(prev[k], want[1]), (t, k, "window: reconstruction")
    finally:
        bufs.close()
        enc.close()


def _ipair(pkg, ctx, w, h, quality, first, make_second, R, model_check=None):
    """i-frame `first`, then the p-frame make_second(padded reconstruction planes) in HIER mode at radius R: device == restatement at both
    levels -> (mv, coarse vectors, has, restatement, planes).  model_check(ref, planes, wmv, whas, wcoef): what a case asserts on the
    restatement alone, before the device's p-frame is looked at"""
    enc = pkg.EncoderSession(ctx, w, h, quality, 1)
    ref = RefEncoder(w, h, quality)
    try:
        enc.set_motion_search("hier", R)
        coef = enc.encode_iframe(first)
        assert np.array_equal(coef[0], ref.iframe(first))
        assert np.array_equal(enc.prev_frame()[0], ref.prev_frame())
        planes = [p.copy() for p in ref.prev]
        second = make_second(planes)
        wmv, whas, wcoef = ref.pframe(second, R)
        if model_check:
            model_check(ref, planes, wmv, whas, wcoef)
        mv, has, coef = enc.encode_pframe(second)
        cmv = enc.coarse_vectors()
        assert np.array_equal(cmv[0], ref.cmv), np.nonzero((cmv[0] != ref.cmv).any(axis=1))[0][:8]
        assert np.array_equal(mv[0], wmv), np.nonzero((mv[0] != wmv).any(axis=1))[0][:8]
        assert np.array_equal(has[0], whas) and np.array_equal(coef[0], wcoef)
        assert np.array_equal(enc.prev_frame()[0], ref.prev_frame())
        return mv[0], cmv[0], has[0], ref, planes
    finally:
        enc.close()


def check_coarse_edges(pkg, ctx, w=96, h=64, quality=2, R=62):
    """the coarse level alone where its square leaves the plane on all four sides: at Rc = 31 every macroblock of a 96 x 64 frame (half
    plane 48 x 32) loses candidates to at least two edges, the corner ones to two adjacent ones, and the true motion points out of the
    plane for the blocks of one side.  Equality of the coarse vectors is asserted inside _ipair."""
    tex = sc.moving_clip(w, h, 1, 19, noise=0)[0]
    for dx, dy in ((26, 18), (-26, -18), (22, -14), (-22, 14)):
        _, cmv, _, ref, _ = _ipair(pkg, ctx, w, h, quality, tex, lambda pl: pack(w, h, translate(pl[0], dx, dy), translate(pl[1], dx // 2, dy // 2), translate(pl[2], dx // 2, dy // 2)), R)
        lum = cmv[:(w // 16) * (h // 16)].reshape(h // 16, w // 16, 2)
        inside = [(by, bx) for by in range(h // 16) for bx in range(w // 16) if 0 <= bx * 16 + dx <= w - 16 and 0 <= by * 16 + dy <= h - 16]
        assert inside and all(tuple(lum[by, bx]) == (dx // 2, dy // 2) for by, bx in inside), (dx, dy, lum)


# ------------------------------------------------------------------ 3. ties
def check_ties(pkg, ctx, w=64, h=64, quality=2, R=30):
    """the vector the rule names where errors tie, at both levels.  w and h are multiples of 32: no plane has padding."""
    rng = np.random.default_rng(3)
    nl = (w // 16) * (h // 16)
    grey = np.full((h, w), 128, np.uint8)
    flat = pack(w, h, np.full((h, w), 100, np.uint8), grey, grey)
    # a flat reference: every candidate of a macroblock has the same error at both levels, (0, 0) wins
    mv, cmv, _, _, planes = _ipair(pkg, ctx, w, h, quality, flat, lambda pl: rng.integers(0, 256, frame_bytes(w, h), dtype=np.uint8), R)
    assert all((p == p.flat[0]).all() for p in planes), "the reference is not flat"
    assert (mv == 0).all() and (cmv == 0).all()
    # horizontal period 8 at full resolution (4 at half), source shifted by 4: dx = -4 and +4, and every dy, match exactly at the fine
    # level, cx = -2 and +2 at the coarse one; the shortest wins, then the smaller component
    col = np.array([40, 80, 160, 220, 200, 120, 60, 30], np.uint8)
    stripes = pack(w, h, np.tile(col, (h, w // 8)), grey, grey)
    mv, cmv, has, ref, planes = _ipair(pkg, ctx, w, h, quality, stripes, lambda pl: pack(w, h, np.roll(pl[0], 4, axis=1), pl[1], pl[2]), R)
    y = planes[0]
    assert np.array_equal(y, np.roll(y, 8, axis=1)) and (y == y[0]).all() and not np.array_equal(y, np.roll(y, 4, axis=1)), "the reference lost its period"
    lm, lc = mv[:nl].reshape(h // 16, w // 16, 2), cmv[:nl].reshape(h // 16, w // 16, 2)
    assert (lc[:, 1:, 0] == -2).all() and (lc[:, 1:, 1] == 0).all(), lc[..., 0]
    assert (lc[:, 0, 0] == 2).all() and (lc[:, 0, 1] == 0).all(), "at the left edge cx = -2 leaves the half plane: +2"
    assert (lm[:, 1:, 0] == -4).all() and (lm[:, 1:, 1] == 0).all(), lm[..., 0]
    assert (lm[:, 0, 0] == 4).all() and (lm[:, 0, 1] == 0).all(), "at the left edge dx = -4 leaves the plane: +4"
    assert (has == 0).all() and (ref.err == 0).all()
    # the same vertically: -4 beats +4
    rows = pack(w, h, np.tile(col[:, None], (h // 8, w)), grey, grey)
    mv, cmv, has, ref, planes = _ipair(pkg, ctx, w, h, quality, rows, lambda pl: pack(w, h, np.roll(pl[0], 4, axis=0), pl[1], pl[2]), R)
    y = planes[0]
    assert np.array_equal(y, np.roll(y, 8, axis=0)) and (y.T == y.T[0]).all() and not np.array_equal(y, np.roll(y, 4, axis=0)), "the reference lost its period"
    lm, lc = mv[:nl].reshape(h // 16, w // 16, 2), cmv[:nl].reshape(h // 16, w // 16, 2)
    assert (lc[1:, :, 1] == -2).all() and (lc[1:, :, 0] == 0).all(), lc[..., 1]
    assert (lc[0, :, 1] == 2).all() and (lc[0, :, 0] == 0).all()
    assert (lm[1:, :, 1] == -4).all() and (lm[1:, :, 0] == 0).all(), lm[..., 1]
    assert (lm[0, :, 1] == 4).all() and (lm[0, :, 0] == 0).all()
    assert (has == 0).all()


# ------------------------------------------------------------------ 4. limits
def check_limits(pkg, ctx, w=160, h=96, quality=2, R=62):
    """a true shift of +63 and of -63 (in x and in y) is found at radius 62: the coarse level reaches +-31, the fine level adds the last
    pixel.  A shift of +64 is outside the 7-bit field's positive half: whatever is chosen is the restatement's (asserted in _ipair) and no
    component exceeds 63."""
    tex = sc.moving_clip(w, h, 1, 23, noise=0)[0]
    bw, bh = w // 16, h // 16
    for dx, dy in ((63, 0), (-63, 0), (0, 63), (0, -63), (64, 0), (0, 64)):
        mv, _, has, ref, _ = _ipair(pkg, ctx, w, h, quality, tex, lambda pl: pack(w, h, translate(pl[0], dx, dy), pl[1], pl[2]), R)
        lum = mv[:bw * bh].reshape(bh, bw, 2)
        assert mv.max() <= 63 and mv.min() >= -64
        inside = [(by, bx) for by in range(bh) for bx in range(bw) if 0 <= bx * 16 + dx <= w - 16 and 0 <= by * 16 + dy <= h - 16]
        assert inside, (dx, dy)
        if max(dx, dy) <= 63:
            assert all(tuple(lum[by, bx]) == (dx, dy) for by, bx in inside), (dx, dy, lum)
            assert all(ref.err[by * bw + bx] == 0 and has[by * bw + bx] == 0 for by, bx in inside)
        else:
            assert all(tuple(lum[by, bx]) != (dx, dy) for by, bx in inside)
            assert lum.max() <= 63


# ------------------------------------------------------------------ 5. reach
REACH_SEED = 11
REACH_PANS = ((40, -24), (37, -21))


def _pan_pair(w, h, quality, dx, dy, seed):
    """frame A: the textured canvas; frame B: A's reconstruction after the i-frame, every PADDED plane translated by (dx, dy) (chroma by half
    of it) with the edges filled from the reconstruction, cropped to the frame -- a pan without noise: a macroblock whose source block and
    displaced patch lie inside the plane matches exactly at (dx, dy)"""
    a = sc.moving_clip(w, h, 1, seed, noise=0)[0]
    ref = RefEncoder(w, h, quality)
    ref.iframe(a)
    b = pack(w, h, translate(ref.prev[0], dx, dy), translate(ref.prev[1], dx // 2, dy // 2), translate(ref.prev[2], dx // 2, dy // 2))
    return a, b


def check_reach(pkg, ctx, w=160, h=112, quality=5, R=48):
    """noise-free pans of (40, -24) and (37, -21): HIER at radius 48 against FULL at 15 and the four-step search.  Device equals the
    restatement; per macroblock E_hier <= E(0, 0); HIER codes fewer macroblocks than FULL 15 -- the last two asserted on the restatement
    first (REACH_SEED was picked on the CPU so that they hold there)."""
    nl = (w // 16) * (h // 16)
    for dx, dy in REACH_PANS:
        a, b = _pan_pair(w, h, quality, dx, dy, REACH_SEED)
        ref, full = RefEncoder(w, h, quality), sc.RefEncoder(w, h, quality)
        ref.iframe(a); full.iframe(a)
        wmv, whas, wcoef = ref.pframe(b, R)
        _, fhas, _ = full.pframe(b, 15)
        assert (ref.err <= ref.err0).all()
        assert int(whas.sum()) < int(fhas.sum()), (int(whas.sum()), int(fhas.sum()))
        carried = (wmv[:nl] == np.array([dx, dy])).all(axis=1)
        assert carried.any() and (ref.err[:nl][carried] == 0).all(), "no macroblock carries the pan"
        coded = {}
        for mode, radius in (("hier", R), ("full", 15), ("fourstep", 0)):
            enc = pkg.EncoderSession(ctx, w, h, quality, 1)
            try:
                enc.set_motion_search(mode, radius)
                enc.encode_iframe(a)
                mv, has, coef = enc.encode_pframe(b)
                coded[mode] = int(has.sum())
                if mode == "hier":
                    assert np.array_equal(mv[0], wmv) and np.array_equal(has[0], whas) and np.array_equal(coef[0], wcoef)
                    assert np.array_equal(enc.coarse_vectors()[0], ref.cmv)
                    assert np.array_equal(enc.prev_frame()[0], ref.prev_frame())
                if mode == "full":
                    assert np.array_equal(has[0], fhas)
            finally:
                enc.close()
        print(f"pan ({dx}, {dy}): coded macroblocks hier {coded['hier']}, full15 {coded['full']}, four-step {coded['fourstep']} of {has.size}")
        assert coded["hier"] < coded["full"]


# ------------------------------------------------------------------ 6. streams
STREAM_CONFIGS = ("plain", "device_entropy", "gop", "gop_by_reference", "gop_redo", "rgb_denoise")
STREAM_PATTERN = "IPPIPP"
STREAM_MOVES = ((0, 0), (26, -22), (-24, 20), (0, 0), (-28, 18), (22, -26))


def _stream_clip(w, h, noise_seed=0):
    """six frames of one canvas seen through a window that jumps by the (dx, dy) of STREAM_MOVES: vectors beyond +-16 in both signs"""
    rng = np.random.default_rng(31)
    m = 72
    c = rng.integers(0, 256, (h + 2 * m + 2, w + 2 * m + 2)).astype(np.int64)
    c = (c[:-2, :-2] + c[1:-1, :-2] + c[2:, :-2] + c[:-2, 1:-1] + 2 * c[1:-1, 1:-1] + c[2:, 1:-1] + c[:-2, 2:] + c[1:-1, 2:] + c[2:, 2:]) // 10
    c = np.clip((c - 128) * 3 + 128, 0, 255)
    out, ox, oy = [], m, m
    for dx, dy in STREAM_MOVES:
        ox, oy = ox + dx, oy + dy
        y = np.clip(c[oy:oy + h, ox:ox + w] + rng.integers(-1, 2, (h, w)), 0, 255).astype(np.uint8)
        u = y[::2, ::2][:h // 2, :w // 2]
        out.append(np.concatenate([y.reshape(-1), u.reshape(-1), (255 - u).reshape(-1)]))
    return np.stack(out)


def decode_gop(pkg, ctx, data):
    d = pkg.GopDecoder(data, ctx, max_gops=2, max_gop_frames=4, threads=1)
    got = []
    try:
        while d.advance_frame(lambda fr: got.append(fr.packed())):
            pass
    finally:
        d.close()
    return got


def check_stream(pkg, ctx, oracle, config, w=160, h=96, quality=4, R=40):
    """6 frames (I P P I P P) through a stream object in HIER mode.  The bytes equal the numpy serialiser's (oracle/pfv_oracle_entropy_np.py)
    fed the restatement's blocks; pfv_decoder, pfv_gop_decoder and the oracle's container decoder show the restatement's reconstruction;
    every stream carries a vector component > 16 and one < -16."""
    clip = _stream_clip(w, h)
    if config == "rgb_denoise":
        ins = [onp.yuv420_to_rgb(f, w, h) for f in clip]
        planar = list(pkg.frames_denoise(ctx, w, h, np.stack([pkg.frames_from_rgb(ctx, w, h, p, "rgb8", "box")[0] for p in ins]), (4, 4, 4), (3, 3, 3)))
    else:
        ins, planar = [pkg.VideoFrame.from_packed(w, h, f) for f in clip], list(clip)
    # the restatement, serialised
    ref = RefEncoder(w, h, quality)
    tabs = onp.qtables(quality)
    want, shown = oen.stream_header(w, h, 30, np.stack([np.asarray(t, np.int64).reshape(64) for t in tabs[:4]])), []
    lo, hi = 0, 0
    for c, f in zip(STREAM_PATTERN, planar):
        if c == "I":
            want += oen.packet(oen.PKT_IFRAME, oen.iframe_payload(ref.iframe(f)))
        else:
            mv, has, coef = ref.pframe(f, R)
            lo, hi = min(lo, int(mv.min())), max(hi, int(mv.max()))
            want += oen.packet(oen.PKT_PFRAME, oen.pframe_payload(mv, has, coef))
        shown.append(ref.shown())
    want += oen.packet(oen.PKT_EOF)
    assert hi > 16 and lo < -16, (lo, hi)
    buf = io.BytesIO()
    if config.startswith("gop"):
        if config == "gop_redo":
            os.environ["PFV_TEST_GOP_ARENA_BYTES"] = "64"
        try:
            e = pkg.GopEncoder(buf, w, h, 30, quality, ctx, max_gops=2, max_gop_frames=3)
        finally:
            os.environ.pop("PFV_TEST_GOP_ARENA_BYTES", None)
    else:
        e = pkg.Encoder(buf, w, h, 30, quality, ctx, device_entropy=config != "plain")       # "plain": the host serialisers
    bufs = DevBufs(ctx)
    try:
        if config == "rgb_denoise":
            e.set_input_rgb(True, "rgb8", "box")
            e.set_denoise(True, (4, 4, 4), (3, 3, 3))
        if config == "gop_by_reference":
            e.set_frames_by_reference(True)
        e.set_motion_search("hier", R)
        for c, x, f in zip(STREAM_PATTERN, ins, clip):
            if config == "gop_by_reference":
                d = bufs.put(f)
                (e.encode_iframe_dev if c == "I" else e.encode_pframe_dev)(d)
            else:
                (e.encode_iframe if c == "I" else e.encode_pframe)(x)
        e.finish()
        st = e.stats() if config.startswith("gop") else None
    finally:
        e.close()
        bufs.close()
    data = buf.getvalue()
    assert data == want, (config, len(data), len(want))
    if st is not None:
        assert (st["batches_redone"] >= 1) == (config == "gop_redo"), st
    for name, got in (("pfv_decoder", sc.decode_product(pkg, ctx, data)), ("pfv_gop_decoder", decode_gop(pkg, ctx, data)), ("oracle", sc.decode_oracle(oracle, data))):
        assert len(got) == len(shown), name
        for t in range(len(shown)):
            assert np.array_equal(got[t], shown[t]), (config, name, t)


# ------------------------------------------------------------------ 7. graph
def check_graph(pkg, ctx, w=160, h=96, quality=4, R=30):
    """a session p-frame in HIER mode recorded once and replayed on new frames gives the restatement's outputs (the capture holds kernels
    only: the scratch was allocated by set_motion_search); a mode change after the capture does not reach the replays"""
    clip = sc.moving_clip(w, h, 4, 57, reach=24)
    ref = RefEncoder(w, h, quality)
    enc = pkg.EncoderSession(ctx, w, h, quality, 1)
    bufs = DevBufs(ctx)
    graph = pkg.Graph(ctx)
    try:
        tb = enc.total_blocks
        enc.set_motion_search("hier", R)
        src = bufs.put(clip[0])
        coef_d, mv_d, has_d = bufs.put(np.zeros(tb * 256, np.int16)), bufs.put(np.zeros(tb * 2, np.int8)), bufs.put(np.zeros(tb, np.uint8))
        enc.encode_iframe_dev(src, coef_d)
        ref.iframe(clip[0])
        ctx.upload(src, clip[1])
        enc.encode_pframe_dev(src, mv_d, has_d, coef_d)
        ref.pframe(clip[1], R)
        ctx.sync()
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


# ------------------------------------------------------------------ 8. off means off
def check_off(pkg, ctx, w=144, h=48, quality=4):
    """HIER on -> off: the four-step and the FULL outputs are byte-equal to a fresh encoder's and session's"""
    clip = sc.moving_clip(w, h, 3, 91)
    for mode, radius in (("fourstep", 0), ("full", 9)):
        outs = []
        for prep in (None, lambda o: (o.set_motion_search("hier", 30), o.set_motion_search(mode, radius))):
            buf = io.BytesIO()
            e = pkg.Encoder(buf, w, h, 30, quality, ctx)
            s = pkg.EncoderSession(ctx, w, h, quality, 1)
            try:
                for o in (e, s):
                    o.set_motion_search(mode, radius)
                    if prep:
                        prep(o)
                assert s.motion_search == (pkg._lib.SEARCH_MODES[mode], radius)
                res = []
                for t, f in enumerate(clip):
                    (e.encode_iframe if t == 0 else e.encode_pframe)(pkg.VideoFrame.from_packed(w, h, f))
                    res.append(s.encode_iframe(f) if t == 0 else s.encode_pframe(f))
                e.finish()
                outs.append((buf.getvalue(), res, s.prev_frame()))
            finally:
                e.close()
                s.close()
        assert outs[1][0] == outs[0][0], mode
        assert np.array_equal(outs[1][2], outs[0][2])
        assert np.array_equal(outs[1][1][0], outs[0][1][0])
        for t in (1, 2):
            assert all(np.array_equal(x, y) for x, y in zip(outs[1][1][t], outs[0][1][t]))


# ------------------------------------------------------------------ 9. refusals
def check_refusals(pkg, ctx, w=48, h=32, quality=4):
    lib, L = ctx._lib, pkg._lib
    HIER, FULL, FOUR = L.PFV_SEARCH_HIER, L.PFV_SEARCH_FULL, L.PFV_SEARCH_FOURSTEP
    clip = sc.moving_clip(w, h, 4, 13)
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

    def not_fourstep(encoder):
        """pfv_encoder has no getter: its p-frame probe calls answer PFV_ERR_STATE exactly while its session is not in four-step mode"""
        try:
            encoder.probe_pframe(frames[1])
            return False
        except pkg.PfvError as err:
            assert err.code == L.PFV_ERR_STATE
            return True
    try:
        tb = s.total_blocks
        out = np.zeros((1, tb, 2), np.int8)
        # null handles
        assert lib.pfv_enc_session_set_motion_search(None, HIER, 30) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_encoder_set_motion_search(None, HIER, 30) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_gop_encoder_set_motion_search(None, HIER, 30) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_enc_session_coarse_vectors(None, out.ctypes.data_as(ctypes.c_void_p), out.nbytes) == L.PFV_ERR_BAD_ARG
        # coarse_vectors before any HIER launch
        assert lib.pfv_enc_session_coarse_vectors(s.handle, out.ctypes.data_as(ctypes.c_void_p), out.nbytes) == L.PFV_ERR_STATE
        # bad radii: the mode stays, the next valid call works
        s.set_motion_search("full", 5)
        for fn, h_ in ((lib.pfv_enc_session_set_motion_search, s.handle), (lib.pfv_encoder_set_motion_search, e.handle), (lib.pfv_gop_encoder_set_motion_search, g.handle)):
            for r in (0, 1, 7, 63, 64, -2):
                assert fn(h_, HIER, r) == L.PFV_ERR_BAD_ARG, r
            assert fn(h_, 3, 30) == L.PFV_ERR_BAD_ARG
        assert mode(s) == (FULL, 5)
        assert not not_fourstep(e)
        for r in (2, 62, 30):
            s.set_motion_search("hier", r)
            assert mode(s) == (HIER, r)
        s.set_motion_search("fourstep", 99)
        assert mode(s) == (FOUR, 0)
        # the session's p-frame probes in HIER mode; the i-frame probes go on working
        s.encode_iframe(clip[0])
        s.set_motion_search("hier", 30)
        assert lib.pfv_enc_session_coarse_vectors(s.handle, out.ctypes.data_as(ctypes.c_void_p), out.nbytes) == L.PFV_ERR_STATE     # still no launch
        n_r = 2
        sizes_d, sse_d, q24_d, src_d = bufs.put(np.zeros(n_r, np.uint32)), bufs.put(np.zeros(n_r * 3, np.uint64)), bufs.put(np.zeros(n_r * 3, np.int64)), bufs.put(clip[1])
        for call in (lambda: s.probe_pframe(clip[1]), lambda: s.probe_pframe_rd(clip[1]), lambda: s.probe_pframe_ssim(clip[1]),
                     lambda: s.probe_pframe_dev(src_d, sizes_d), lambda: s.probe_pframe_rd_dev(src_d, sizes_d, sse_d),
                     lambda: s.probe_pframe_ssim_dev(src_d, sizes_d, sse_d, q24_d)):
            with pytest.raises(pkg.PfvError) as err:
                call()
            assert err.value.code == L.PFV_ERR_STATE
        assert mode(s) == (HIER, 30)
        assert s.probe_iframe(clip[1]).shape == (1, n_r)
        s.encode_pframe(clip[1])
        assert s.coarse_vectors().shape == (1, tb, 2)
        assert lib.pfv_enc_session_coarse_vectors(s.handle, out.ctypes.data_as(ctypes.c_void_p), out.nbytes - 2) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_enc_session_coarse_vectors(s.handle, None, out.nbytes) == L.PFV_ERR_BAD_ARG
        s.set_motion_search("fourstep")
        assert s.probe_pframe(clip[2]).shape == (1, n_r)
        s.encode_pframe(clip[2])
        assert lib.pfv_enc_session_coarse_vectors(s.handle, out.ctypes.data_as(ctypes.c_void_p), out.nbytes) == L.PFV_ERR_STATE     # the last launch was four-step
        # pfv_encoder: HIER against the p-frame probe, the two p-frame floors and encode_frame, in both orders
        e.encode_iframe(frames[0])
        switches = ((e.set_pframe_probe, True, False), (e.set_pframe_quality_floor, 30.0, 0.0), (e.set_pframe_ssim_floor, 0.5, 0.0))
        for setter, on, off in switches:
            setter(on)
            with pytest.raises(pkg.PfvError) as err:
                e.set_motion_search("hier", 30)
            assert err.value.code == L.PFV_ERR_STATE and not not_fourstep(e)
            e.set_motion_search("fourstep")
            setter(off)
            e.set_motion_search("hier", 30)
            with pytest.raises(pkg.PfvError) as err:
                setter(on)
            assert err.value.code == L.PFV_ERR_STATE
            setter(off)
            assert not_fourstep(e)
            e.set_motion_search("fourstep")
        e.set_motion_search("hier", 30)
        n0 = len(buf.getvalue())
        with pytest.raises(pkg.PfvError) as err:
            e.encode_frame(frames[1])
        assert err.value.code == L.PFV_ERR_STATE and len(buf.getvalue()) == n0
        for name in ("probe_pframe", "probe_pframe_rd", "probe_pframe_ssim"):
            with pytest.raises(pkg.PfvError) as err:
                getattr(e, name)(frames[1])
            assert err.value.code == L.PFV_ERR_STATE
        e.probe_iframe(frames[1])
        e.set_rate(100000)
        e.set_rung(1)
        e.encode_pframe(frames[1])
        assert len(buf.getvalue()) > n0
        e.set_motion_search("fourstep")
        assert e.encode_frame(frames[2]) in (1, 2, 3)
        e.finish()
        # pfv_gop_encoder: a change while a batch is in flight, to HIER and away from it
        g.set_motion_search("hier", 30)
        for t in range(4):
            (g.encode_iframe if t % 2 == 0 else g.encode_pframe)(frames[t])
        g.encode_iframe(frames[0])
        assert lib.pfv_gop_encoder_set_motion_search(g.handle, FOUR, 0) == L.PFV_ERR_STATE
        assert lib.pfv_gop_encoder_set_motion_search(g.handle, HIER, 62) == L.PFV_ERR_STATE
        g.flush()
        g.set_motion_search("fourstep")
        g.encode_pframe(frames[1])
        g.finish()
        tbuf = io.BytesIO()
        twin = pkg.Encoder(tbuf, w, h, 30, quality, ctx)
        try:
            twin.set_motion_search("hier", 30)
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


# ------------------------------------------------------------------ 10. mirrors
def build_cpp(lib_path, exe):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "hier_report.cpp"), "-o", exe, lib_path, "-Wl,-rpath," + os.path.dirname(lib_path)], check=True)


def check_cpp(pkg, ctx, exe, tmp_path, w=96, h=64, quality=4, R=30):
    """tests/cpp/hier_report.cpp (pfv::EncoderSession / Encoder / GopEncoder ::set_motion_search, EncoderSession::coarse_vectors) prints the
    vectors, coarse vectors and packet sizes of the Python path"""
    clip = sc.moving_clip(w, h, 3, 41, reach=20)
    src = str(tmp_path / "in.yuv")
    clip.tofile(src)
    r = subprocess.run([exe, src, str(w), str(h), str(quality), str(R)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = []
    s = pkg.EncoderSession(ctx, w, h, quality, 1)
    buf = io.BytesIO()
    e = pkg.Encoder(buf, w, h, 30, quality, ctx)
    try:
        s.set_motion_search("hier", R)
        e.set_motion_search("hier", R)
        for t, f in enumerate(clip):
            n0 = len(buf.getvalue())
            if t == 0:
                s.encode_iframe(f)
                e.encode_iframe(pkg.VideoFrame.from_packed(w, h, f))
            else:
                mv, has, _ = s.encode_pframe(f)
                e.encode_pframe(pkg.VideoFrame.from_packed(w, h, f))
                lines.append(f"frame {t} mv " + " ".join(f"{int(x)},{int(y)}" for x, y in mv[0]))
                lines.append(f"frame {t} coarse " + " ".join(f"{int(x)},{int(y)}" for x, y in s.coarse_vectors()[0]))
                lines.append(f"frame {t} coded {int(has.sum())}")
            lines.append(f"frame {t} packet {len(buf.getvalue()) - n0}")
        e.finish()
    finally:
        s.close()
        e.close()
    lines.append(f"gop stream {len(buf.getvalue())} bytes identical")
    lines.append(f"mode hier radius {R}")
    assert r.stdout.splitlines() == lines


def check_rd_tool(lib_path, w=64, h=48, n_frames=4, gop=3, qualities=(2, 5), R=30, pan=(20, -18)):
    """tools/rd_curve.py --search hier,30 --pan 20,-18 on the library at lib_path: without the flags the lines are the same minus the new
    keys; the four_, full_ and hier_ columns are there and count the same macroblocks"""
    env = dict(os.environ)
    if lib_path:
        env["PFV_HIP_LIB"] = lib_path
    cmd = [sys.executable, os.path.join(ROOT, "tools", "rd_curve.py"), str(w), str(h), str(n_frames), "--gop", str(gop), "--kind", "pan",
           "--qualities", ",".join(str(q) for q in qualities)]
    plain = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert plain.returncode == 0, plain.stderr
    r = subprocess.run(cmd + ["--search", f"hier,{R}", "--pan", f"{pan[0]},{pan[1]}"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr
    lines = [json.loads(x) for x in r.stdout.splitlines()]
    stripped = [{k: v for k, v in d.items() if not k.startswith(("full_", "four_", "hier_", "search_"))} for d in lines]
    assert [json.dumps(d) for d in stripped] == plain.stdout.splitlines()
    for d in lines:
        assert d["search_radius"] == R and d["search_pan"] == list(pan)
        for col in ("stream_bytes", "psnr_yuv", "coded", "skipped"):
            assert all(f"{key}_{col}" in d for key in ("four", "full", "hier")), (col, d)
        assert d["hier_coded"] + d["hier_skipped"] == d["full_coded"] + d["full_skipped"] == d["four_coded"] + d["four_skipped"] > 0
    return lines


def check_time_tool(lib_path, w=64, h=48):
    """tools/rd_curve.py --time-search at a toy size: the row carries the HIER launches and their five stages at radius 30 and 62"""
    env = dict(os.environ)
    if lib_path:
        env["PFV_HIP_LIB"] = lib_path
    cmd = [sys.executable, os.path.join(ROOT, "tools", "rd_curve.py"), str(w), str(h), "2", "--qualities", "5", "--time-search"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr
    row = json.loads(r.stdout.splitlines()[-1])["time_search"]
    for key in ("hier_r30", "hier_r62"):
        assert row[f"{key}_ms"] >= 0 and row[f"{key}_coarse_dot4_floor_ms"] > 0
        assert set(row[f"{key}_stages_ms"]) == {"halve_src", "halve_ref", "coarse", "refine", "transform"}
        assert all(v >= 0 for v in row[f"{key}_stages_ms"].values())            # the emulator's events read 0
    assert all(row[k] >= 0 for k in ("fourstep_ms", "full_r7_ms", "full_r15_ms"))
    return row


# ------------------------------------------------------------------ 11. every even radius, the match in the corner of the square
SWEEP_RADII = list(range(2, 63, 2))


def check_sweep(pkg, ctx, R, w=sc.SWEEP_SHAPE[0], h=sc.SWEEP_SHAPE[1]):
    """search_cases.check_sweep in HIER mode: the luma plane translated by (R, -R), then by (-R, R); the coarse vector of an inside
    macroblock is (+-R / 2, -+R / 2), the corner of the coarse square, and the fine level keeps twice that.  Asserted on the restatement
    first, then device == restatement at both levels (_ipair)."""
    for dx, dy in ((R, -R), (-R, R)):
        _ipair(pkg, ctx, w, h, sc.SWEEP_QUALITY, sc.sweep_first(w, h), lambda pl: pack(w, h, translate(pl[0], dx, dy), pl[1], pl[2]), R,
               model_check=sc.corner_model_check(dx, dy, True))


# ------------------------------------------------------------------ 12. ladder rungs
LADDER_R = 30


def hier_ladder_model(oracle, w, h, qualities, n=1, R=LADDER_R):
    return sc.SearchLadderModel(oracle, w, h, qualities, n, lambda px, ref, q, px_err, clear: encode_plane_hier(px, ref, q, px_err, clear, R))


def check_rate_rungs(pkg, ctx, oracle, device_entropy, R=LADDER_R, n_frames=8):
    """pfv_encoder's rate controller moves the rung while HIER p-frames follow: the rungs the encoder reports are taken as they come, and the
    stream's bytes equal the HIER ladder model's at those rungs (every p-frame payload at the rung that wrote it)"""
    w, h = sc.LADDER_SHAPE
    frames = lc.rate_clip(w, h)[:n_frames]
    m = hier_ladder_model(oracle, w, h, lc.RATE_LADDER, 1, R)
    m.iframe(0, frames[0], 2)
    budget = int(1.25 * len(m.payload_p(*m.pframe(0, frames[1], 2), 2)))         # ladder_cases.rate_budget on the mode's model
    plan = [("I", 2)] + [("P", None)] * (len(frames) - 1)
    data, rungs = lc.run_encoder(pkg, ctx, w, h, frames, plan, device_entropy, qualities=lc.RATE_LADDER, rate=budget, search=("hier", R))
    print(f"hier rate run: budget {budget}, rungs {rungs}")
    assert min(rungs[1:]) > 0 and len(set(rungs[1:])) > 1, (rungs, "the controller never moved the rung")
    model = hier_ladder_model(oracle, w, h, lc.RATE_LADDER, 1, R)
    want, shown = lc.model_stream(model, frames, [(kind, rungs[t]) for t, (kind, _) in enumerate(plan)])
    assert data == want, (len(data), len(want), rungs)
    got, _ = lc.decode_both(pkg, ctx, oracle, data)
    assert len(got) == len(shown) and all(np.array_equal(a, b) for a, b in zip(got, shown))


# ------------------------------------------------------------------ 13. the largest error
def check_largest(pkg, ctx, w=sc.LARGEST_SHAPE[0], h=sc.LARGEST_SHAPE[1], R=62):
    """search_cases.check_largest in HIER mode: E = 256 x 255^2 at the fine level, 64 x 255^2 for every coarse candidate; both vectors are 0"""
    for v in (0, 255):
        first, second = sc.largest_frames(w, h, v)
        _ipair(pkg, ctx, w, h, sc.SWEEP_QUALITY, first, lambda pl: second, R, model_check=sc.largest_model_check(w, h, True))


# ------------------------------------------------------------------ 14. one pixel beyond the 7-bit field
def check_field_edge(pkg, ctx, w=sc.SWEEP_SHAPE[0], h=sc.SWEEP_SHAPE[1], R=62):
    """pans of (+-64, 0) and (0, +-64) at radius 62: the exact match is one pixel beyond |component| <= 63.  Of the restatement first: some
    inside macroblock's coarse vector is +-31 along the pan and at most 1 across it, so the 25 vectors round twice of it hold the exact
    match (E = 0) and only the rule's limit keeps it out; no vector component exceeds 63 and no inside macroblock carries the pan.  Then
    device == restatement (_ipair).  (check_limits' pan of 64 at 160 x 96 has no such macroblock: profiles/search_mutants.md.)"""
    for dx, dy in ((64, 0), (-64, 0), (0, 64), (0, -64)):
        def model(ref, planes, wmv, whas, wcoef):
            ins = sc.inside_blocks(planes[0].shape[1], planes[0].shape[0], dx, dy)
            along, across = (0, 1) if dx else (1, 0)
            c = ref.cmv[ins].astype(np.int64)
            tempted = ins[(c[:, along] == (dx + dy) // 64 * 31) & (np.abs(c[:, across]) <= 1)]
            assert tempted.size > 0, (dx, dy, c.tolist())
            assert np.abs(wmv.astype(np.int64)).max() <= 63 and (ref.err[tempted] > 0).all()
            assert not (wmv[ins] == np.array([dx, dy])).all(axis=1).any()
        _ipair(pkg, ctx, w, h, sc.SWEEP_QUALITY, sc.sweep_first(w, h), lambda pl: pack(w, h, translate(pl[0], dx, dy), pl[1], pl[2]), R, model_check=model)
