"""Shared checks of scene-cut detection (include/pfv_hip_ext.h, "scene-cut detection"), driven on the CPU emulator by tests/test_emu_scene.py
and on a real MI355X by tests/test_gpu_scene.py at the same small shapes.

The reference is `RefDetector` below: numpy in 64-bit integers, written from the header's text -- quarter planes from 4 x 4 sums, 8 x 8 blocks,
intra against the rounded mean, every allowed candidate within R with the lexicographic tie rule, the sums per pair, priming and commit.
Every numeric comparison with it is EQUALITY of the stats and of both block maps: the measure is integer arithmetic, no tolerance anywhere.

The decision clip (check_decision, check_encoder): 18 frames of 320 x 192, frames 0 .. 6 of SyntheticStream(SEED, "pan"), frames 7 .. 12 of
SyntheticStream(SEED + 17, "low_motion"), frames 13 .. 17 of SyntheticStream(SEED, "pan") again: splices at frames 7 and 13.  Under the
restatement alone, R = 5 (asserted by check_decision before anything else): every continuous pair scores <= 128, both splices >= 230.
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
from quality_cases import PACKED, PADDED, DevBufs, frame_bytes, padded_frame_bytes, planes_of, to_padded

ROOT = qc.ROOT
# 30x34 no block at all; 32x32 one block whose only candidate is (0, 0); 36x68 candidates clipped to one side; 144x48 the denoiser's strip
# shape; 322x194 packed rows not 16-byte aligned, leftover pixels and quarter samples; 1040x64 32 blocks across; 416x240 the general case
SHAPES = [(30, 34), (32, 32), (36, 68), (144, 48), (322, 194), (1040, 64), (416, 240)]
RADII = list(range(8))
N_STREAMS = 3
POISON = 0xA5
P = ctypes.c_void_p
FIELDS = ("inter", "intra", "zero", "n_blocks", "n_intra", "n_moving", "reserved")


# ------------------------------------------------------------------ the numpy restatement of the normative text
def quarter(luma):
    """Q[y][x] = (sum of the 4 x 4 luma pixels at (4x, 4y) + 8) >> 4 over qw = w >> 2, qh = h >> 2"""
    h, w = luma.shape
    qw, qh = w >> 2, h >> 2
    s = luma[:4 * qh, :4 * qw].astype(np.int64).reshape(qh, 4, qw, 4).sum(axis=(1, 3))
    return (s + 8) >> 4


def candidates(R):
    """every (cx, cy) within R in the order of the tie rule behind S: |cx| + |cy|, then cy, then cx"""
    c = [(cx, cy) for cy in range(-R, R + 1) for cx in range(-R, R + 1)]
    return sorted(c, key=lambda v: (abs(v[0]) + abs(v[1]), v[1], v[0]))


def ref_pair(qprev, qcur, R):
    """(stats tuple, blk uint32 [nby, nbx], vec int8 [nby, nbx, 2]) of one pair of quarter planes; qprev None: no previous frame"""
    qh, qw = qcur.shape
    nbx, nby = qw >> 3, qh >> 3
    blk, vec = np.zeros((nby, nbx), np.uint32), np.zeros((nby, nbx, 2), np.int8)
    if qprev is None or nbx * nby == 0:
        return (0, 0, 0, 0 if qprev is None else nbx * nby, 0, 0, 0), blk, vec
    B = qcur[:8 * nby, :8 * nbx].reshape(nby, 8, nbx, 8).transpose(0, 2, 1, 3)          # [by][bx][8][8]
    mean = (B.sum(axis=(2, 3)) + 32) >> 6
    intra = np.abs(B - mean[:, :, None, None]).sum(axis=(2, 3))
    assert intra.max() <= 16320
    win = np.lib.stride_tricks.sliding_window_view(qprev, (8, 8))                         # [y][x][8][8], y <= qh - 8, x <= qw - 8
    by, bx = np.mgrid[0:nby, 0:nbx]
    cand = candidates(R)
    S = np.full((len(cand), nby, nbx), 1 << 40, dtype=np.int64)
    for i, (cx, cy) in enumerate(cand):
        x, y = 8 * bx + cx, 8 * by + cy
        ok = (x >= 0) & (x <= qw - 8) & (y >= 0) & (y <= qh - 8)
        sad = np.abs(B - win[np.where(ok, y, 0), np.where(ok, x, 0)]).sum(axis=(2, 3))
        S[i] = np.where(ok, sad, 1 << 40)
    pick = S.argmin(axis=0)                                                               # the first minimum: the tie order of `cand`
    best = np.take_along_axis(S, pick[None], axis=0)[0]
    zero = S[cand.index((0, 0))]
    assert best.max() <= 16320 and zero.max() <= 16320
    cxy = np.array(cand, dtype=np.int64)[pick]
    blk = ((best << 16) | intra).astype(np.uint32)
    vec = cxy.astype(np.int8)
    stats = (int(best.sum()), int(intra.sum()), int(zero.sum()), nbx * nby, int((best >= intra).sum()), int((cxy != 0).any(axis=2).sum()), 0)
    return stats, blk, vec


def ref_score(stats):
    inter, intra, _, n_blocks = stats[:4]
    return 0 if n_blocks == 0 else min(65535, inter * 256 // max(intra, 64 * n_blocks))


def ref_plan(scores, threshold, min_interval, max_interval):
    types, last = [], 0
    for k, s in enumerate(scores):
        d = k - last
        i = k == 0 or (max_interval > 0 and d >= max_interval) or (s >= threshold and d >= max(1, min_interval))
        types.append(1 if i else 2)
        last = k if i else last
    return types


class RefDetector:
    """the object of the header's text: per stream the previous quarter plane (None: not primed)"""

    def __init__(self, w, h, n_streams, R=4):
        self.w, self.h, self.n, self.R = w, h, n_streams, R
        self.state = [None] * n_streams

    def reset(self, first=0, n=None):
        for k in range(first, first + (self.n - first if n is None else n)):
            self.state[k] = None

    def luma(self, frame):
        return planes_of(frame, self.w, self.h)[0]

    def run(self, frames, first=0, commit=True):
        """packed frames of streams first .. -> [(stats, blk, vec)]"""
        out = []
        for k, frame in enumerate(np.atleast_2d(frames)):
            q = quarter(self.luma(frame))
            out.append(ref_pair(self.state[first + k], q, self.R))
            if commit:
                self.state[first + k] = q
        return out

    def run_clip(self, frames, stream=0, commit=True):
        out, prev = [], self.state[stream]
        for frame in np.atleast_2d(frames):
            q = quarter(self.luma(frame))
            out.append(ref_pair(prev, q, self.R))
            prev = q
        if commit:
            self.state[stream] = prev
        return out


def ref_sequence(w, h, frames, R):
    """the stats tuples pfv_frames_scene makes of one stream's frames"""
    ref = RefDetector(w, h, 1, R)
    return [ref.run(f)[0][0] for f in frames]


def as_tuples(stats):
    return [tuple(int(r[k]) for k in FIELDS) for r in np.asarray(stats).reshape(-1)]


# ------------------------------------------------------------------ the device call
def run_dev(pkg, ctx, det, w, h, frames, layout=PACKED, first=0, commit=True, src_off=0, src_gap=0, rng=None, clip=False):
    """pfv_scene_detector_run_dev (clip: _run_clip_dev on stream `first`) on `frames` ([n, frame bytes of the layout]) -> (stats tuples, blk,
    vec).  The source lies src_off bytes into its allocation with src_gap random bytes between frames; the stats land in a POISONED allocation
    with two guard entries on either side, which must still hold the poison."""
    from pretty_fast_video_amd.scene import STATS_DTYPE
    frames = np.atleast_2d(frames)
    n, sfb = frames.shape
    rng = rng or np.random.default_rng(7)
    s_stride = sfb + src_gap
    src = rng.integers(0, 256, src_off + n * s_stride + 16, dtype=np.uint8)
    for k in range(n):
        src[src_off + k * s_stride: src_off + k * s_stride + sfb] = frames[k]
    dst = np.full((n + 4) * 40, POISON, dtype=np.uint8)
    bufs = DevBufs(ctx)
    try:
        s_dev, d_dev = bufs.put(src), bufs.put(dst)
        if clip:
            ctx.check(ctx._lib.pfv_scene_detector_run_clip_dev(det.handle, first, n, P(s_dev + src_off), layout, s_stride if src_gap else 0, 1 if commit else 0, P(d_dev + 80)))
        else:
            ctx.check(ctx._lib.pfv_scene_detector_run_dev(det.handle, first, n, P(s_dev + src_off), layout, s_stride if src_gap else 0, 1 if commit else 0, P(d_dev + 80)))
        ctx.download(dst, d_dev)
    finally:
        bufs.close()
    assert (dst[:80] == POISON).all() and (dst[80 + 40 * n:] == POISON).all(), "bytes outside the n stats were written"
    blk, vec = det.maps(0 if clip else first, n)
    return as_tuples(dst[80:80 + 40 * n].view(STATS_DTYPE)), blk, vec


def assert_equal(got, want, what):
    """got: run_dev's triple; want: RefDetector's list of triples"""
    stats, blk, vec = got
    for k, (ws, wb, wv) in enumerate(want):
        assert stats[k] == ws, (what, k, stats[k], ws)
        assert np.array_equal(blk[k], wb), (what, k, "blk", np.argwhere(blk[k] != wb)[:4])
        assert np.array_equal(vec[k], wv), (what, k, "vec", np.argwhere(vec[k] != wv)[:4])


def make_frames(pkg, w, h, n_frames, rng):
    """[frame][stream]: stream 0 seeded random bytes, stream 1 the synthetic pan, stream 2 the synthetic low-motion clip"""
    fb = frame_bytes(w, h)
    pan, low = pkg.SyntheticStream(w, h, seed=11, kind="pan"), pkg.SyntheticStream(w, h, seed=12, kind="low_motion")
    out = np.zeros((n_frames, N_STREAMS, fb), dtype=np.uint8)
    for t in range(n_frames):
        out[t, 0] = rng.integers(0, 256, fb)
        out[t, 1] = pan.frame(t)
        out[t, 2] = low.frame(t)
    return out


def luma_of_q(q):
    """a luma plane whose quarter plane is q exactly: every 4 x 4 cell filled with its sample ((16 v + 8) >> 4 = v)"""
    return np.repeat(np.repeat(np.asarray(q, dtype=np.uint8), 4, axis=0), 4, axis=1)


def frame_of_luma(luma, fill=128):
    h, w = luma.shape
    return np.concatenate([luma.reshape(-1).astype(np.uint8), np.full(2 * (w // 2) * (h // 2), fill, np.uint8)])


# ------------------------------------------------------------------ 1. exact equality with numpy
def check_shape(pkg, ctx, w, h, seed=1, R=4):
    """3 frames x 3 streams; PACKED and PADDED source (random padding); aligned, and at an unaligned source base with a gap between the frames
    (the byte path, a stream stride larger than the frame); frame 1 runs as a window of the middle stream alone.  Stats and both maps after
    every run equal numpy; the host entry point and the Python mirror agree."""
    rng = np.random.default_rng(seed * 1000 + w * 7 + h)
    fb = frame_bytes(w, h)
    clip = make_frames(pkg, w, h, 3, rng)
    for layout in (PACKED, PADDED):
        for unaligned in (False, True):
            kw = dict(src_off=3, src_gap=37) if unaligned else {}
            ref = RefDetector(w, h, N_STREAMS, R)
            with pkg.SceneDetector(ctx, w, h, N_STREAMS, radius=R) as det:
                assert (det.blocks_x, det.blocks_y) == ((w >> 2) >> 3, (h >> 2) >> 3)
                for t in range(3):
                    src = clip[t] if layout == PACKED else np.stack([to_padded(x, w, h, rng) for x in clip[t]])
                    assert src.shape[1] == (fb if layout == PACKED else padded_frame_bytes(w, h))
                    first, n = (1, 1) if t == 1 else (0, N_STREAMS)
                    got = run_dev(pkg, ctx, det, w, h, src[first:first + n], layout, first=first, rng=rng, **kw)
                    assert_equal(got, ref.run(clip[t][first:first + n], first=first), (w, h, layout, unaligned, t))
                    if t == 2 and det.n_blocks:
                        assert got[0][1][3] == det.n_blocks and got[0][0][3] == det.n_blocks      # the middle stream against frame 1, the others against frame 0
    got = pkg.frames_scene(ctx, w, h, clip, R, n_streams=N_STREAMS)
    ref = RefDetector(w, h, N_STREAMS, R)
    want = [[r[0] for r in ref.run(f)] for f in clip]
    assert got.shape == (3, N_STREAMS) and [as_tuples(row) for row in got] == want
    if ((w >> 2) >> 3) * ((h >> 2) >> 3) == 0:
        assert all(s == (0,) * 7 for row in want for s in row)


def check_radius(pkg, ctx, R, w=144, h=80):
    rng = np.random.default_rng(40 + R)
    clip = make_frames(pkg, w, h, 2, rng)
    ref = RefDetector(w, h, N_STREAMS, R)
    with pkg.SceneDetector(ctx, w, h, N_STREAMS, radius=R) as det:
        for t in range(2):
            assert_equal(run_dev(pkg, ctx, det, w, h, clip[t]), ref.run(clip[t]), (R, t))
    if R == 0:
        s = ref_sequence(w, h, clip[:, 1], 0)[1]
        assert s[0] == s[2] and s[5] == 0          # zero motion only: best is zero, nothing moves


# ------------------------------------------------------------------ 2. traps
def pair_dev(pkg, ctx, w, h, prev, cur, R):
    """two frames through a fresh detector -> the second run's (stats tuple, blk, vec), checked against numpy on the way"""
    ref = RefDetector(w, h, 1, R)
    with pkg.SceneDetector(ctx, w, h, 1, radius=R) as det:
        assert_equal(run_dev(pkg, ctx, det, w, h, prev), ref.run(prev), "prev")
        got = run_dev(pkg, ctx, det, w, h, cur)
        assert_equal(got, ref.run(cur), "cur")
    return got[0][0], got[1][0], got[2][0]


def check_traps(pkg, ctx):
    w, h = 144, 80          # quarter plane 36 x 20: 4 x 2 blocks, 4 leftover samples across and down
    nb = 8
    # constant planes: every candidate ties, the chosen vector is (0, 0)
    for a, b in ((0, 0), (17, 17), (10, 200), (255, 0)):
        st, blk, vec = pair_dev(pkg, ctx, w, h, frame_of_luma(np.full((h, w), a, np.uint8)), frame_of_luma(np.full((h, w), b, np.uint8)), 7)
        assert st == (64 * abs(a - b) * nb, 0, 64 * abs(a - b) * nb, nb, nb, 0, 0) and not vec.any(), (a, b, st)
    # prev = 0, cur = 255: best is 16 320 per block and the map packs it
    st, blk, vec = pair_dev(pkg, ctx, w, h, frame_of_luma(np.zeros((h, w), np.uint8)), frame_of_luma(np.full((h, w), 255, np.uint8)), 4)
    assert (blk == (16320 << 16)).all() and st[0] == 16320 * nb and ref_score(st) == 65280 == pkg.scene_score(pkg.SceneStats(*st))
    # period 2 in both directions: cur = prev shifted by (sx, sy) quarter samples, so S = 0 wherever cx = sx, cy = sy modulo 2 and only
    # |cx| + |cy|, then cy, then cx decide; at the left / top border the negative candidate does not exist
    yy, xx = np.mgrid[0:20, 0:36]
    base = lambda sx, sy: (40 + 50 * ((xx + sx) % 2) + 90 * ((yy + sy) % 2)).astype(np.uint8)      # noqa: E731
    for (sx, sy), inner, corner in (((0, 0), (0, 0), (0, 0)), ((1, 0), (-1, 0), (1, 0)), ((0, 1), (0, -1), (0, 1)), ((1, 1), (-1, -1), (1, 1))):
        st, blk, vec = pair_dev(pkg, ctx, w, h, frame_of_luma(luma_of_q(base(0, 0))), frame_of_luma(luma_of_q(base(sx, sy))), 3)
        assert st[0] == 0 and tuple(vec[1, 1]) == inner and tuple(vec[0, 0]) == corner, ((sx, sy), vec[:, :, 0], vec[:, :, 1])
    # the two roundings: 4 x 4 sums of 7, 8 and 24 give the samples 0, 1 and 2 -- read as `zero` against a black previous frame at R = 0
    black = frame_of_luma(np.zeros((h, w), np.uint8))
    for cell_sum, sample in ((7, 0), (8, 1), (24, 2)):
        luma = np.zeros((h, w), np.uint8)
        luma[1::4, 2::4] = cell_sum          # one pixel of every 4 x 4 cell carries the whole sum
        st, _, _ = pair_dev(pkg, ctx, w, h, black, frame_of_luma(luma), 0)
        assert st[2] == 64 * sample * nb and st[1] == 0, (cell_sum, st)
    # block sums of 31, 32 and 33 around the mean's rounding: samples of 0 and 1, mean 0 / 1 / 1, intra 31 / 32 / 31
    for ones, intra in ((31, 31), (32, 32), (33, 31)):
        q = np.zeros((8, 8), np.uint8)
        q.reshape(-1)[:ones] = 1
        st, blk, _ = pair_dev(pkg, ctx, 32, 32, frame_of_luma(np.zeros((32, 32), np.uint8)), frame_of_luma(luma_of_q(q)), 4)
        assert st == (ones, intra, ones, 1, 1 if ones >= intra else 0, 0, 0) and int(blk[0, 0]) == (ones << 16 | intra), (ones, st)
    # best == intra exactly counts in n_intra; one less does too, one more does not
    q = np.zeros((8, 8), np.uint8)
    q[:, 4:] = 2                            # mean 1, intra 64
    for prev_q, best, counted in ((np.ones((8, 8), np.uint8), 64, 1), (q.T.copy(), 64, 1)):
        st, _, _ = pair_dev(pkg, ctx, 32, 32, frame_of_luma(luma_of_q(prev_q)), frame_of_luma(luma_of_q(q)), 4)
        assert st[0] == best and st[1] == 64 and st[4] == counted, st
    q2 = q.copy()
    q2[0, 0] = 1
    q2[0, 4] = 3                            # sum 66, mean 1, intra 31 + 31 + 2 = 64; against all ones best is 64 as well
    st, _, _ = pair_dev(pkg, ctx, 32, 32, frame_of_luma(luma_of_q(np.ones((8, 8), np.uint8))), frame_of_luma(luma_of_q(q2)), 4)
    assert st[0] == 64 and st[1] == 64 and st[4] == 1, st
    prev_q = np.ones((8, 8), np.uint8)
    prev_q[0, 4] = 3                        # matches the 3: best 62 < intra 64 is not counted
    st, _, _ = pair_dev(pkg, ctx, 32, 32, frame_of_luma(luma_of_q(prev_q)), frame_of_luma(luma_of_q(q2)), 4)
    assert st[0] == 62 and st[1] == 64 and st[4] == 0, st
    prev_q[0, 5] = 4                        # the 2 beside it now costs 2 instead of 1: best 63, one below intra, still not counted
    st, _, _ = pair_dev(pkg, ctx, 32, 32, frame_of_luma(luma_of_q(prev_q)), frame_of_luma(luma_of_q(q2)), 4)
    assert st[0] == 63 and st[4] == 0, st


def check_locality(pkg, ctx, w, h, qx, qy, R=4):
    """One changed pixel of the PREVIOUS frame changes only blocks whose search window contains its quarter sample; one of the CURRENT frame
    only the block that holds it.  The current frame is the previous one moved block by block, so that the chosen candidates of neighbouring
    blocks overlap in the windows' overlap; returns the number of blocks the previous frame's pixel changed."""
    rng = np.random.default_rng(w + 31 * h)
    qw, qh = w >> 2, h >> 2
    nbx, nby = qw >> 3, qh >> 3
    qprev = rng.integers(0, 101, (qh, qw)).astype(np.uint8)
    qcur = rng.integers(0, 101, (qh, qw)).astype(np.uint8)
    for by in range(nby):
        for bx in range(nbx):          # even block columns take their content from 2 samples to the right, even rows from 2 samples below
            cx = 2 if bx % 2 == 0 and 8 * bx + 10 <= qw else 0
            cy = 2 if by % 2 == 0 and 8 * by + 10 <= qh else 0
            qcur[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = qprev[8 * by + cy:8 * by + cy + 8, 8 * bx + cx:8 * bx + cx + 8]
    prev, cur = luma_of_q(qprev), luma_of_q(qcur)
    pad = lambda l: frame_of_luma(np.pad(l, ((0, h - l.shape[0]), (0, w - l.shape[1])), constant_values=77))      # noqa: E731
    base = pair_dev(pkg, ctx, w, h, pad(prev), pad(cur), R)
    assert base[0][0] == 0                                                                     # every block finds itself
    by, bx = np.mgrid[0:nby, 0:nbx]
    # the previous frame
    prev2 = prev.copy()
    prev2[4 * qy + 1, 4 * qx + 2] = 255
    got = pair_dev(pkg, ctx, w, h, pad(prev2), pad(cur), R)
    changed = (got[1] != base[1]) | (got[2] != base[2]).any(axis=2)
    allowed = (8 * bx - R <= qx) & (qx <= 8 * bx + 7 + R) & (8 * by - R <= qy) & (qy <= 8 * by + 7 + R)
    assert not (changed & ~allowed).any(), np.argwhere(changed & ~allowed)
    # the current frame
    cur2 = cur.copy()
    cur2[4 * qy + 1, 4 * qx + 2] = 255
    got2 = pair_dev(pkg, ctx, w, h, pad(prev), pad(cur2), R)
    changed2 = (got2[1] != base[1]) | (got2[2] != base[2]).any(axis=2)
    own = (bx == qx >> 3) & (by == qy >> 3)
    assert not (changed2 & ~own).any() and (changed2.any() == bool(own.any()))
    return int(changed.sum())


# ------------------------------------------------------------------ 3. state
def check_state(pkg, ctx, w=144, h=80, R=4):
    rng = np.random.default_rng(5)
    clip = make_frames(pkg, w, h, 6, rng)
    ref = RefDetector(w, h, N_STREAMS, R)
    with pkg.SceneDetector(ctx, w, h, N_STREAMS, max_clip_frames=5, radius=R) as det:
        # unprimed: n_blocks 0, every field and both maps zero; uncommitted leaves it unprimed
        for commit in (False, False, True):
            got = run_dev(pkg, ctx, det, w, h, clip[0], commit=commit)
            assert all(s == (0,) * 7 for s in got[0]) and not got[1].any() and not got[2].any()
            assert_equal(got, ref.run(clip[0], commit=commit), ("unprimed", commit))
        # primed: an uncommitted run measures and changes nothing, twice the same; the committed one measures the same and moves the state
        a = run_dev(pkg, ctx, det, w, h, clip[1], commit=False)
        b = run_dev(pkg, ctx, det, w, h, clip[1], commit=False)
        c = run_dev(pkg, ctx, det, w, h, clip[1], commit=True)
        want = ref.run(clip[1])
        for got in (a, b, c):
            assert_equal(got, want, "commit")
        assert all(s[3] == det.n_blocks and s[0] > 0 for s in c[0])
        d = run_dev(pkg, ctx, det, w, h, clip[1], commit=False)
        assert_equal(d, ref.run(clip[1], commit=False), "same frame")
        assert all(s[0] == 0 and s[2] == 0 and s[5] == 0 for s in d[0])
        # reset of the middle stream alone
        det.reset(1, 1)
        ref.reset(1, 1)
        got = run_dev(pkg, ctx, det, w, h, clip[2])
        assert_equal(got, ref.run(clip[2]), "reset")
        assert got[0][1] == (0,) * 7 and got[0][0][3] == det.n_blocks and got[0][2][3] == det.n_blocks
        # a clip of one stream equals step-by-step runs: on a primed stream (0), on an unprimed one (2, after reset), uncommitted and committed
        det.reset(2, 1)
        ref.reset(2, 1)
        for stream in (0, 2):
            frames = clip[1:6, stream]
            for commit in (False, True):
                step = RefDetector(w, h, 1, R)
                step.state[0] = ref.state[stream]
                want = [step.run(f)[0] for f in frames]
                got = run_dev(pkg, ctx, det, w, h, frames, first=stream, clip=True, commit=commit)
                assert_equal(got, want, ("clip", stream, commit))
                unprimed = ref.state[stream] is None
                assert_equal(got, ref.run_clip(frames, stream, commit=commit), ("clip ref", stream, commit))
                assert unprimed == (stream == 2) and (got[0][0] == (0,) * 7) == unprimed and got[0][1][3] == det.n_blocks
            # the last frame became the state: the other streams are where they were
            got = run_dev(pkg, ctx, det, w, h, clip[0], commit=False)
            assert_equal(got, ref.run(clip[0], commit=False), ("after clip", stream))
        # the device twin of the step-by-step runs: a second detector fed frame by frame gives the clip's bytes
        with pkg.SceneDetector(ctx, w, h, 1, max_clip_frames=5, radius=R) as one, pkg.SceneDetector(ctx, w, h, 1, max_clip_frames=5, radius=R) as two:
            steps = [run_dev(pkg, ctx, one, w, h, f)[0][0] for f in clip[:5, 1]]
            assert run_dev(pkg, ctx, two, w, h, clip[:5, 1], clip=True)[0] == steps
            assert run_dev(pkg, ctx, two, w, h, clip[5, 1])[0] == run_dev(pkg, ctx, one, w, h, clip[5, 1])[0]


def check_graph(pkg, ctx, w=144, h=80, n=2, R=4):
    """a steady-state run recorded once: two replays on the same frames give identical bytes, and numpy's, for three frames; a run that would
    prime inside a recording is refused; a committed steady-state run is recordable"""
    from pretty_fast_video_amd.scene import STATS_DTYPE
    rng = np.random.default_rng(17)
    clip = make_frames(pkg, w, h, 4, rng)[:, :n]
    ref = RefDetector(w, h, n, R)
    bufs = DevBufs(ctx)
    det, fresh = pkg.SceneDetector(ctx, w, h, n, radius=R), pkg.SceneDetector(ctx, w, h, n, radius=R)
    graph, other = pkg.Graph(ctx), pkg.Graph(ctx)
    try:
        s_dev, d_dev = bufs.put(clip[0]), bufs.put(np.full(n * 40, POISON, np.uint8))
        det.run_dev(s_dev, d_dev)
        ref.run(clip[0])
        with graph:
            with pytest.raises(pkg.PfvError) as e:        # not primed: the memset behind the kernels cannot be recorded
                fresh.run_dev(s_dev, d_dev)
            assert e.value.code == pkg._lib.PFV_ERR_STATE
            det.run_dev(s_dev, d_dev, commit=False)
        for t in range(1, 4):
            ctx.upload(s_dev, clip[t])
            want = ref.run(clip[t], commit=False)
            seen = []
            for _ in range(2):
                ctx.upload(d_dev, np.full(n * 40, POISON, np.uint8))
                graph.launch()
                got = np.zeros(n * 40, np.uint8)
                ctx.download(got, d_dev)
                seen.append(got.tobytes())
                blk, vec = det.maps(0, n)
                assert_equal((as_tuples(got.view(STATS_DTYPE)), blk, vec), want, ("graph", t))
            assert seen[0] == seen[1]
        with other:                                       # recorded, never launched: the call itself is what is checked
            det.run_dev(s_dev, d_dev, commit=True)
    finally:
        graph.close()
        other.close()
        det.close()
        fresh.close()
        bufs.close()


def check_bad_arguments(pkg, ctx):
    """every refusal leaves the stats untouched"""
    L, lib = pkg._lib, ctx._lib
    w, h, n = 64, 48, 4
    fb, pfb = frame_bytes(w, h), padded_frame_bytes(w, h)
    bufs = DevBufs(ctx)
    det = pkg.SceneDetector(ctx, w, h, n, max_clip_frames=3)
    graph = pkg.Graph(ctx)
    try:
        a = bufs.put(np.zeros(8 * pfb, dtype=np.uint8))
        d = bufs.put(np.full(8 * 40, POISON, np.uint8))

        def untouched():
            got = np.zeros(8 * 40, np.uint8)
            ctx.download(got, d)
            return bool((got == POISON).all())

        def create(ctx_h=ctx.handle, w=w, h=h, n=1, clip=0):
            err = ctypes.c_int(-99)
            hnd = lib.pfv_scene_detector_create(ctx_h, w, h, n, clip, ctypes.byref(err))
            if hnd:
                lib.pfv_scene_detector_destroy(hnd)
            return bool(hnd), err.value
        assert create() == (True, L.PFV_OK) and create(w=2, h=2) == (True, L.PFV_OK)
        assert lib.pfv_scene_detector_create(None, w, h, 1, 0, None) is None
        for bad in ((15, 16), (16, 17), (0, 16), (16, -2), (65536, 16)):
            assert create(w=bad[0], h=bad[1]) == (False, L.PFV_ERR_BAD_ARG), bad
        assert create(n=0) == (False, L.PFV_ERR_BAD_ARG) and create(n=-1) == (False, L.PFV_ERR_BAD_ARG) and create(clip=-1) == (False, L.PFV_ERR_BAD_ARG)
        assert create(ctx_h=None) == (False, L.PFV_ERR_BAD_ARG)
        lib.pfv_scene_detector_destroy(None)
        # the radius: outside 0 .. 7 it stays as it was
        frames = make_frames(pkg, w, h, 2, np.random.default_rng(3))
        det.set_radius(2)
        for bad in (-1, 8, 255):
            assert lib.pfv_scene_detector_set_radius(det.handle, bad) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_scene_detector_set_radius(None, 2) == L.PFV_ERR_BAD_ARG
        ref = RefDetector(w, h, N_STREAMS, 2)
        for t in range(2):
            assert_equal(run_dev(pkg, ctx, det, w, h, frames[t]), ref.run(frames[t]), ("radius kept", t))
        # reset
        assert lib.pfv_scene_detector_reset(None, 0, 1) == L.PFV_ERR_BAD_ARG
        for first, cnt in ((-1, 1), (0, 0), (0, n + 1), (n, 1), (1, n), (0, -1), (2**31 - 1, 2)):
            assert lib.pfv_scene_detector_reset(det.handle, first, cnt) == L.PFV_ERR_BAD_ARG, (first, cnt)

        def call(first=0, cnt=1, src=a, layout=PACKED, ss=0, commit=1, dst=d, h_=None):
            return lib.pfv_scene_detector_run_dev(det.handle if h_ is None else h_, first, cnt, P(src) if src else None, layout, ss, commit, P(dst) if dst else None)

        def clip_call(stream=0, cnt=1, src=a, layout=PACKED, ss=0, commit=1, dst=d):
            return lib.pfv_scene_detector_run_clip_dev(det.handle, stream, cnt, P(src) if src else None, layout, ss, commit, P(dst) if dst else None)
        assert lib.pfv_scene_detector_run_dev(None, 0, 1, P(a), PACKED, 0, 1, P(d)) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_scene_detector_run_clip_dev(None, 0, 1, P(a), PACKED, 0, 1, P(d)) == L.PFV_ERR_BAD_ARG
        for first, cnt in ((-1, 1), (0, 0), (0, n + 1), (n, 1), (1, n), (0, -1), (2**31 - 1, 2)):      # a window outside n_streams
            assert call(first=first, cnt=cnt) == L.PFV_ERR_BAD_ARG, (first, cnt)
        assert call(layout=2) == L.PFV_ERR_BAD_ARG and call(layout=-1) == L.PFV_ERR_BAD_ARG
        assert call(src=None) == L.PFV_ERR_BAD_ARG and call(dst=None) == L.PFV_ERR_BAD_ARG and call(dst=d + 4) == L.PFV_ERR_BAD_ARG
        assert call(cnt=2, ss=fb - 1) == L.PFV_ERR_BAD_ARG and call(cnt=2, layout=PADDED, ss=pfb - 1) == L.PFV_ERR_BAD_ARG
        for stream, cnt in ((-1, 1), (n, 1), (0, 0), (0, 4), (0, -1)):                                 # no such stream, n_frames outside 1 .. max_clip_frames
            assert clip_call(stream=stream, cnt=cnt) == L.PFV_ERR_BAD_ARG, (stream, cnt)
        assert clip_call(layout=7) == L.PFV_ERR_BAD_ARG and clip_call(src=None) == L.PFV_ERR_BAD_ARG and clip_call(dst=None) == L.PFV_ERR_BAD_ARG
        assert clip_call(cnt=2, ss=fb - 1) == L.PFV_ERR_BAD_ARG and clip_call(dst=d + 4) == L.PFV_ERR_BAD_ARG
        ctx.sync()
        assert untouched()
        assert call(cnt=n) == L.PFV_OK and call(cnt=2, layout=PADDED, ss=pfb) == L.PFV_OK and clip_call(cnt=3, stream=n - 1) == L.PFV_OK
        # the timed form: uncommitted, the run's own numbers
        ms = (ctypes.c_float * 3)()
        timed = lambda first=0, cnt=n, clip=0, h_=det.handle, out=ms: lib.pfv_scene_detector_run_timed_dev(h_, first, cnt, clip, P(a), PACKED, 0, P(d), out)      # noqa: E731
        assert timed(h_=None) == L.PFV_ERR_BAD_ARG and timed(out=None) == L.PFV_ERR_BAD_ARG and timed(first=1) == L.PFV_ERR_BAD_ARG
        assert timed(clip=1, cnt=4) == L.PFV_ERR_BAD_ARG and timed(clip=1, first=n, cnt=1) == L.PFV_ERR_BAD_ARG
        assert timed() == L.PFV_OK and timed(clip=1, cnt=3) == L.PFV_OK and all(v >= 0 for v in ms)
        # the maps
        nb = det.n_blocks
        blk, vec = np.zeros(n * nb, np.uint32), np.zeros(n * nb * 2, np.int8)
        hp = lambda x: x.ctypes.data_as(P)      # noqa: E731
        assert lib.pfv_scene_detector_maps(det.handle, 0, n, hp(blk), hp(vec)) == L.PFV_OK and lib.pfv_scene_detector_maps(det.handle, 1, 1, None, hp(vec)) == L.PFV_OK
        assert lib.pfv_scene_detector_maps(None, 0, 1, hp(blk), hp(vec)) == L.PFV_ERR_BAD_ARG and lib.pfv_scene_detector_maps(det.handle, 0, 1, None, None) == L.PFV_ERR_BAD_ARG
        for first, cnt in ((-1, 1), (0, 0), (0, n + 1), (n, 1)):
            assert lib.pfv_scene_detector_maps(det.handle, first, cnt, hp(blk), hp(vec)) == L.PFV_ERR_BAD_ARG
        # the host form
        host, out = np.zeros(2 * n * fb, np.uint8), np.full(2 * n * 40, POISON, np.uint8)

        def hcall(c=ctx.handle, w=w, h=h, n_=n, nf=2, src=host, R=4, dst=out):
            return lib.pfv_frames_scene(c, w, h, n_, nf, hp(src) if src is not None else None, R, hp(dst) if dst is not None else None)
        assert hcall(c=None) == L.PFV_ERR_BAD_ARG and hcall(w=15) == L.PFV_ERR_BAD_ARG and hcall(h=0) == L.PFV_ERR_BAD_ARG
        assert hcall(n_=0) == L.PFV_ERR_BAD_ARG and hcall(nf=0) == L.PFV_ERR_BAD_ARG and hcall(nf=-1) == L.PFV_ERR_BAD_ARG
        assert hcall(src=None) == L.PFV_ERR_BAD_ARG and hcall(dst=None) == L.PFV_ERR_BAD_ARG and hcall(R=8) == L.PFV_ERR_BAD_ARG and hcall(R=-1) == L.PFV_ERR_BAD_ARG
        assert (out == POISON).all()
        assert hcall() == L.PFV_OK and not (out == POISON).all()
        # the pure host functions
        from pretty_fast_video_amd.scene import STATS_DTYPE
        st, ty = np.zeros(3, STATS_DTYPE), np.full(3, POISON, np.uint8)
        assert lib.pfv_scene_score_q8(None) == 0
        for args in ((None, 3, 1, 0, 0, hp(ty)), (hp(st), 3, 1, 0, 0, None), (hp(st), 0, 1, 0, 0, hp(ty)), (hp(st), -1, 1, 0, 0, hp(ty)), (hp(st), 3, 1, -1, 0, hp(ty)),
                     (hp(st), 3, 1, 0, -1, hp(ty))):
            assert lib.pfv_scene_plan(*args) == L.PFV_ERR_BAD_ARG
        assert (ty == POISON).all()
        # while a graph is being recorded: creation, the maps and the host form refuse; a run that needs the priming memset refuses
        fresh = pkg.SceneDetector(ctx, w, h, n, max_clip_frames=3)
        try:
            ctx.upload(d, np.full(8 * 40, POISON, np.uint8))
            with graph:
                assert create() == (False, L.PFV_ERR_STATE)
                assert hcall() == L.PFV_ERR_STATE
                assert lib.pfv_scene_detector_maps(det.handle, 0, 1, hp(blk), hp(vec)) == L.PFV_ERR_STATE
                assert call(cnt=n, h_=fresh.handle) == L.PFV_ERR_STATE
                assert call(cnt=n, h_=fresh.handle, commit=0) == L.PFV_OK and call(cnt=n) == L.PFV_OK      # recorded, never launched
                assert call(first=1, cnt=1, h_=fresh.handle) == L.PFV_ERR_STATE
                assert lib.pfv_scene_detector_run_timed_dev(det.handle, 0, 1, 0, P(a), PACKED, 0, P(d), (ctypes.c_float * 3)()) == L.PFV_ERR_STATE
                assert lib.pfv_scene_detector_run_clip_dev(fresh.handle, 0, 2, P(a), PACKED, 0, 1, P(d)) == L.PFV_ERR_STATE
            ctx.sync()
            assert untouched()
            assert call(first=1, cnt=1, h_=fresh.handle) == L.PFV_OK
            ctx.sync()
        finally:
            fresh.close()
    finally:
        graph.close()
        det.close()
        bufs.close()


# ------------------------------------------------------------------ 4. the decision
CLIP_W, CLIP_H, CLIP_R = 320, 192, 5
SPLICES = (7, 13)
_clip_cache = {}


def decision_clip(pkg):
    """(frames [18, frame bytes], the restatement's stats tuples at R = 5), made once"""
    if "clip" not in _clip_cache:
        from pretty_fast_video_amd.synth import SEED
        a, b = pkg.SyntheticStream(CLIP_W, CLIP_H, seed=SEED, kind="pan"), pkg.SyntheticStream(CLIP_W, CLIP_H, seed=SEED + 17, kind="low_motion")
        frames = np.stack([(b if SPLICES[0] <= t < SPLICES[1] else a).frame(t) for t in range(18)])
        frames.setflags(write=False)
        _clip_cache["clip"] = (frames, ref_sequence(CLIP_W, CLIP_H, frames, CLIP_R))
    return _clip_cache["clip"]


def check_decision(pkg, ctx):
    frames, want = decision_clip(pkg)
    scores = [ref_score(s) for s in want]
    print("scene scores (q8) of the decision clip under the restatement:", scores)
    # the condition that keeps the test honest, under the restatement alone
    for t in range(1, 18):
        assert (scores[t] >= 230) if t in SPLICES else (scores[t] <= 128), (t, scores)
    assert scores[0] == 0
    got = pkg.frames_scene(ctx, CLIP_W, CLIP_H, frames, CLIP_R)
    assert as_tuples(got) == want
    assert [pkg.scene_score(s) for s in got.reshape(-1)] == scores
    types = pkg.scene_plan(got.reshape(-1), min_interval=1, max_interval=0)
    assert [t for t in range(18) if types[t] == 1] == [0, *SPLICES] and set(types.tolist()) == {1, 2}
    # one launch group over the clip where it lies: the pfv_gop_encoder recipe
    with pkg.SceneDetector(ctx, CLIP_W, CLIP_H, 1, max_clip_frames=18, radius=CLIP_R) as det:
        assert as_tuples(det.run_clip(frames)) == want


def check_plan(pkg):
    """pfv_scene_plan's interval rules and pfv_scene_score_q8 on hand-made stats, host only"""
    from pretty_fast_video_amd.scene import STATS_DTYPE
    mk = lambda inter, intra=1000, nb=10: (inter, intra, 0, nb, 0, 0, 0)      # noqa: E731
    for st in (mk(0), mk(999), mk(1000), mk(687), mk(688), mk(10**9), mk(5, 0), mk(640, 0), mk(641, 639), (5, 5, 5, 0, 0, 0, 0), mk(2**40, 1, 1), mk(2**60, 2**60, 1)):
        assert pkg.scene_score(pkg.SceneStats(*st)) == ref_score(st), st
    assert pkg.scene_score(pkg.SceneStats(*mk(688))) == 176 and pkg.scene_score(pkg.SceneStats(*mk(687))) == 175 and pkg.SceneStats(*mk(688)).score == 176
    assert pkg.scene_score(pkg.SceneStats(*mk(640, 0))) == 256                     # the 64 * n_blocks floor
    hi, lo = mk(1000), mk(100)          # scores 256 and 25
    cases = [
        ([lo] * 6, 176, 0, 0), ([hi] * 6, 176, 0, 0), ([hi] * 6, 176, 1, 0), ([hi] * 6, 176, 2, 0), ([hi] * 7, 176, 3, 0),
        ([lo] * 7, 176, 0, 3), ([lo] * 7, 176, 0, 1), ([lo, lo, hi, lo, lo, lo, lo, hi], 176, 0, 3), ([lo, hi, hi, lo, hi, lo, lo, hi, hi], 176, 2, 4),
        ([lo, hi, lo], 256, 0, 0), ([lo, hi, lo], 257, 0, 0), ([lo, hi, lo], 0, 0, 0), ([hi, hi, hi, hi], 176, 5, 2), ([(9, 9, 9, 0, 0, 0, 0)] * 3, 0, 0, 0),
    ]
    for stats, thr, mn, mx in cases:
        want = ref_plan([ref_score(s) for s in stats], thr, mn, mx)
        got = pkg.scene_plan([pkg.SceneStats(*s) for s in stats], thr, mn, mx)
        assert got.tolist() == want, (stats, thr, mn, mx, got, want)
        arr = np.array(stats, dtype=STATS_DTYPE)
        types = np.zeros(len(stats), np.uint8)
        n_i = pkg._lib.load().pfv_scene_plan(arr.ctypes.data_as(P), len(stats), thr, mn, mx, types.ctypes.data_as(P))
        assert n_i == want.count(1) and types.tolist() == want
    assert pkg.scene_plan([pkg.SceneStats(*hi)] * 6, 176, 2, 0).tolist() == [1, 2, 1, 2, 1, 2]
    assert pkg.scene_plan([pkg.SceneStats(*lo)] * 7, 176, 0, 3).tolist() == [1, 2, 2, 1, 2, 2, 1]
    with pytest.raises(pkg.PfvError):
        pkg.scene_plan([pkg.SceneStats(*hi)], 176, -1, 0)


# ------------------------------------------------------------------ 5. the encoder
ENCODER_CONFIGS = {
    "fourstep": dict(device_entropy=True, search=None),
    "fourstep_host": dict(device_entropy=False, search=None),
    "full": dict(device_entropy=True, search=("full", 7)),
    "hier": dict(device_entropy=True, search=("hier", 30)),
}


def check_encoder(pkg, ctx, config, quality=5):
    """encode_frame with the switch on over the decision clip: type 1 at frame 0 and at the splices (full / hier: 2 everywhere else), last_scene
    after every call = pfv_frames_scene of the frames; the stream equals, byte for byte, a second encoder's that replays the returned types
    through the explicit calls.  With the switch off, encode_frame in full / hier mode still returns PFV_ERR_STATE."""
    cfg = ENCODER_CONFIGS[config]
    frames, want = decision_clip(pkg)
    w, h = CLIP_W, CLIP_H
    a_buf, b_buf = io.BytesIO(), io.BytesIO()
    mk = lambda buf: pkg.Encoder(buf, w, h, 30, quality, ctx, device_entropy=cfg["device_entropy"])      # noqa: E731
    a, b = mk(a_buf), mk(b_buf)
    try:
        for e in (a, b):
            if cfg["search"]:
                e.set_motion_search(*cfg["search"])
        if cfg["search"]:
            with pytest.raises(pkg.PfvError) as err:
                a.encode_frame(pkg.VideoFrame.from_packed(w, h, frames[0]))
            assert err.value.code == pkg._lib.PFV_ERR_STATE and a_buf.getvalue() == b_buf.getvalue()
        with pytest.raises(pkg.PfvError) as err:
            a.last_scene
        assert err.value.code == pkg._lib.PFV_ERR_STATE
        a.set_scene_cut(True, radius=CLIP_R, min_interval=1)
        with pytest.raises(pkg.PfvError) as err:          # on, nothing measured yet
            a.last_scene
        assert err.value.code == pkg._lib.PFV_ERR_STATE
        types = []
        for t, f in enumerate(frames):
            fr = pkg.VideoFrame.from_packed(w, h, f)
            if t in (3, SPLICES[0]):                      # a probe measures uncommitted: the encode of the same picture sees what it saw
                a.probe_iframe(fr)
                assert tuple(a.last_scene) == want[t]
            types.append(a.encode_frame(fr))
            assert tuple(a.last_scene) == want[t], (config, t)
            {1: b.encode_iframe, 2: b.encode_pframe}.get(types[-1], lambda _f: b.encode_dropframe())(fr)
            assert a_buf.getvalue() == b_buf.getvalue(), (config, t, types)
        print(f"scene-cut encoder {config}: types {types}")
        assert all(types[t] == 1 for t in (0, *SPLICES)), types
        if cfg["search"]:
            assert [t for t in range(18) if types[t] == 1] == [0, *SPLICES] and set(types) == {1, 2}, types
        # off again: full / hier refuse as before, and the state is left alone by a drop frame while on
        a.set_scene_cut(False)
        if cfg["search"]:
            with pytest.raises(pkg.PfvError) as err:
                a.encode_frame(pkg.VideoFrame.from_packed(w, h, frames[0]))
            assert err.value.code == pkg._lib.PFV_ERR_STATE
        with pytest.raises(pkg.PfvError):
            a.last_scene
        for e in (a, b):
            e.finish()
        assert a_buf.getvalue() == b_buf.getvalue()
    finally:
        a.close()
        b.close()


def check_encoder_switch(pkg, ctx, w=96, h=64, quality=5):
    """explicit calls: the switch changes no byte, on, off again, or never on; encode_dropframe leaves the detector's state alone; switching
    on again starts without a past; with set_denoise on the measured frame is the filtered one; bad arguments of the switch"""
    stream = pkg.SyntheticStream(w, h, seed=5, kind="pan")
    frames = np.stack([stream.frame(t) for t in range(6)])
    want = ref_sequence(w, h, frames, 3)
    a_buf, b_buf = io.BytesIO(), io.BytesIO()
    a, b = pkg.Encoder(a_buf, w, h, 30, quality, ctx), pkg.Encoder(b_buf, w, h, 30, quality, ctx)
    fr = [pkg.VideoFrame.from_packed(w, h, f) for f in frames]
    try:
        a.set_scene_cut(True, threshold_q8=100, radius=3)
        for t in range(3):
            for e in (a, b):
                (e.encode_iframe if t == 0 else e.encode_pframe)(fr[t])
            assert tuple(a.last_scene) == want[t] and a_buf.getvalue() == b_buf.getvalue()
        a.encode_dropframe()
        b.encode_dropframe()
        assert tuple(a.last_scene) == want[2]
        a.probe_pframe(fr[4])                             # uncommitted: frame 3 is still measured against frame 2
        assert tuple(a.last_scene) == ref_pair(quarter(planes_of(frames[2], w, h)[0]), quarter(planes_of(frames[4], w, h)[0]), 3)[0]
        for e in (a, b):
            e.encode_pframe(fr[3])
        assert tuple(a.last_scene) == want[3] and a_buf.getvalue() == b_buf.getvalue()
        a.set_scene_cut(False)
        for e in (a, b):
            e.encode_pframe(fr[4])
            e.encode_iframe(fr[5])
        assert a_buf.getvalue() == b_buf.getvalue()
        a.set_scene_cut(True, radius=3)                   # on again: no past
        with pytest.raises(pkg.PfvError):
            a.last_scene
        a.encode_pframe(fr[4])
        b.encode_pframe(fr[4])
        assert tuple(a.last_scene) == (0,) * 7 and a_buf.getvalue() == b_buf.getvalue()
        # behind the noise filter
        a.set_denoise(True, (6, 6, 6), (5, 5, 5))
        a.set_scene_cut(False)
        a.set_scene_cut(True, radius=3)
        filt = pkg.frames_denoise(ctx, w, h, frames[:3], (6, 6, 6), (5, 5, 5))
        assert not np.array_equal(filt, frames[:3])
        fwant = ref_sequence(w, h, filt, 3)
        for t in range(3):
            (a.encode_iframe if t == 0 else a.encode_pframe)(fr[t])
            assert tuple(a.last_scene) == fwant[t], t
        assert fwant[1] != want[1]
        lib, L = ctx._lib, pkg._lib
        assert lib.pfv_encoder_set_scene_cut(None, 1, 176, 4, 0) == L.PFV_ERR_BAD_ARG
        for R, mn in ((-1, 0), (8, 0), (4, -1)):
            assert lib.pfv_encoder_set_scene_cut(a.handle, 1, 176, R, mn) == L.PFV_ERR_BAD_ARG
        assert tuple(a.last_scene) == fwant[2]            # a refused call changes nothing
        assert lib.pfv_encoder_last_scene(None, None) == L.PFV_ERR_BAD_ARG and lib.pfv_encoder_last_scene(a.handle, None) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_encoder_set_scene_cut(a.handle, 0, 0, 99, -5) == L.PFV_OK      # off ignores the rest
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ 6. C++ mirror and tool
def build_cpp(lib_path, exe):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "scene_report.cpp"), "-o", exe, lib_path, "-Wl,-rpath," + os.path.dirname(lib_path)], check=True)


def cpp_clip(pkg, w, h):
    from pretty_fast_video_amd.synth import SEED
    a, b = pkg.SyntheticStream(w, h, seed=SEED, kind="pan"), pkg.SyntheticStream(w, h, seed=SEED + 17, kind="low_motion")
    return np.stack([(b if 3 <= t < 6 else a).frame(t) for t in range(8)])


def check_cpp(pkg, ctx, exe, tmp_path, w=128, h=96, quality=5, R=5):
    """tests/cpp/scene_report.cpp (pfv::Encoder::set_scene_cut / last_scene, pfv::frames_scene, pfv::scene_plan, pfv::SceneDetector): the
    stats equal numpy's, the plan equals the restatement's, and the stream equals a Python encoder's that replays the printed types"""
    from pretty_fast_video_amd.scene import STATS_DTYPE
    clip = cpp_clip(pkg, w, h)
    want = ref_sequence(w, h, clip, R)
    scores = [ref_score(s) for s in want]
    src, o1, o2 = str(tmp_path / "in.yuv"), str(tmp_path / "out.pfv"), str(tmp_path / "out.stats")
    clip.tofile(src)
    r = subprocess.run([exe, src, str(w), str(h), str(quality), str(R), "176", o1, o2], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    types = [int(x) for x in lines[0].split()[1:]]
    assert lines[0].startswith("types ") and len(types) == len(clip) and types[0] == 1
    assert lines[1] == "plan " + " ".join(str(x) for x in ref_plan(scores, 176, 1, 0))
    assert lines[2] == "scores " + " ".join(str(x) for x in scores)
    assert lines[3] == f"frames {len(clip)} of {w}x{h}, {frame_bytes(w, h)} bytes each, {((w >> 2) >> 3) * ((h >> 2) >> 3)} blocks"
    assert as_tuples(np.fromfile(o2, dtype=STATS_DTYPE)) == want
    assert any(s >= 176 for s in scores[1:]) and any(s < 176 for s in scores[1:])
    for t in range(1, len(clip)):
        assert types[t] == 1 or scores[t] < 176, (t, types, scores)      # rule 1b; below the threshold rules 2 - 5 choose, an i-frame included
    buf = io.BytesIO()
    e = pkg.Encoder(buf, w, h, 30, quality, ctx)
    try:
        for ty, f in zip(types, clip):
            {1: e.encode_iframe, 2: e.encode_pframe}.get(ty, lambda _f: e.encode_dropframe())(pkg.VideoFrame.from_packed(w, h, f))
        e.finish()
    finally:
        e.close()
    assert open(o1, "rb").read() == buf.getvalue()


def check_rd_tool(pkg, lib_path, w=128, h=96, n_frames=8, quality=5):
    """tools/rd_curve.py --scene-cut on the library at lib_path: the planned types are the restatement's plan of the spliced clip it names, the
    byte counts are those of Python encoders fed the same types; --time-scene prints its row"""
    env = dict(os.environ)
    if lib_path:
        env["PFV_HIP_LIB"] = lib_path
    cmd = [sys.executable, os.path.join(ROOT, "tools", "rd_curve.py"), str(w), str(h), str(n_frames), "--qualities", str(quality), "--scene-cut", "176,5"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout.splitlines()[-1])["scene_cut"]
    assert d["threshold_q8"] == 176 and d["radius"] == 5 and d["frames"] == n_frames
    from pretty_fast_video_amd.synth import SEED
    a, b = pkg.SyntheticStream(w, h, seed=SEED, kind="pan"), pkg.SyntheticStream(w, h, seed=SEED + 17, kind="low_motion")
    clip = np.stack([(b if (t // d["segment"]) % 2 else a).frame(t) for t in range(n_frames)])
    scores = [ref_score(s) for s in ref_sequence(w, h, clip, 5)]
    assert d["scores_q8"] == scores
    assert d["planned_types"] == ref_plan(scores, 176, 1, 15) and d["fixed_types"] == ref_plan([0] * n_frames, 176, 1, 15)
    assert [t for t in range(n_frames) if d["planned_types"][t] == 1] == [0, *d["splices"]]
    assert d["planned_bytes"] > 0 and d["fixed_bytes"] > 0 and d["planned_worst_psnr"] > 0 and d["fixed_worst_psnr"] > 0
    return d


def check_time_tool(pkg, lib_path):
    env = dict(os.environ)
    if lib_path:
        env["PFV_HIP_LIB"] = lib_path
    cmd = [sys.executable, os.path.join(ROOT, "tools", "rd_curve.py"), "64", "48", "2", "--qualities", "5", "--time-scene"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout.splitlines()[-1])["time_scene"]
    keys = ("quarter_ms", "cost_r4_ms", "cost_r7_ms", "sum_ms", "run_dev_r4_ms", "run_dev_r7_ms", "clip_quarter_ms", "clip_cost_r4_ms", "clip_sum_ms", "run_clip_dev_r4_ms", "sse_pair_ms",
            "enc_pframe_ms")
    assert all(d[k] >= 0 for k in keys), d      # the emulator's events read 0
    return d
