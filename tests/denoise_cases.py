"""Shared checks of the denoising pre-filter (include/pfv_hip_ext.h, "denoising pre-filter"), driven on the CPU emulator by
tests/test_emu_denoise.py and on a real MI355X by tests/test_gpu_denoise.py at the same small shapes.

The reference is `RefDenoiser` below: numpy in 64-bit integers, written from the header's text -- the ramp, stage 1 over the eight
neighbours of the INPUT plane with a neighbour outside the picture contributing 0, stage 2 against the previous output with a division that
truncates toward zero, priming and commit.  Every comparison with it is EQUALITY: the filter is integer arithmetic.

The state has no getter.  It is read through the filter itself (`check_state`): with Ss = 0 and St = 16 an UNCOMMITTED run of a constant
frame c gives c + tdiv(3 * phi(P - c, 16), 4), and over the 32 constants of STATE_PROBES that tuple is different for every P in 0 .. 255
(asserted below), so equal probe outputs mean an equal state.

Direction of the effect (check_effect), 176 x 144, I + 5 P of a static smooth field with a slowly moving box plus uniform noise in [-3, 3],
strengths (6, 6, 6) / (6, 6, 6); bytes of the stream, skipped p-frame macroblocks, PSNR-YUV of the input against the clean clip -- the
figures of the numpy restatement with the oracle encoder, and the same on the emulator:
    quality 1:  46 592 -> 14 537 bytes, skipped  10 -> 484 of 795, PSNR 42.12 -> 49.22 dB
    quality 2:   7 871 ->  7 078 bytes, skipped 691 -> 722 of 795, PSNR 42.12 -> 49.22 dB
From quality 3 on the encoder's own skip threshold swallows noise of this size (752 -> 760 skipped at quality 3), so the check runs at the
two qualities where the filter has work to do.
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
from quality_cases import PACKED, PADDED, DevBufs, frame_bytes, pad16, padded_frame_bytes, plane_dims, planes_of, to_padded

ROOT = qc.ROOT
# 2x2 the smallest frame; 16x16 one macroblock; 18x34 partial macroblocks, chroma 9x17; 130x18 crosses the 128-pixel strip end by 2, chroma 65;
# 144x48 two strips across, three down: every halo and lane +-8 seam; 50x38 the general odd-chroma case
SHAPES = [(2, 2), (16, 16), (18, 34), (130, 18), (144, 48), (50, 38)]
SPATIAL, TEMPORAL = (4, 9, 16), (16, 0, 7)
N_STREAMS = 3
POISON = 0xA5
P = ctypes.c_void_p


# ------------------------------------------------------------------ the numpy restatement of the normative text
def tdiv(a, n):
    return np.sign(a) * (np.abs(a) // n)


def phi(d, S):
    """the ramp on int64 arrays: full up to S, back to zero at 2S; phi(d, 0) = 0"""
    a = np.abs(d)
    return np.sign(d) * np.maximum(0, a - np.maximum(0, 2 * (a - S)))


NEIGHBOURS = [(-1, -1, 1), (-1, 0, 2), (-1, 1, 1), (0, -1, 2), (0, 1, 2), (1, -1, 1), (1, 0, 2), (1, 1, 1)]      # dy, dx, weight


def ref_spatial(plane, Ss):
    """stage 1 on one plane (2-D uint8) -> int64; asserts that the result lies inside the 3 x 3 window's minimum and maximum"""
    h, w = plane.shape
    c = plane.astype(np.int64)
    acc = np.zeros((h, w), dtype=np.int64)
    lo, hi = c.copy(), c.copy()
    for dy, dx, g in NEIGHBOURS:
        n = np.zeros((h, w), dtype=np.int64)
        inside = np.zeros((h, w), dtype=bool)
        ys, ye, xs, xe = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
        n[ys:ye, xs:xe] = c[ys + dy:ye + dy, xs + dx:xe + dx]
        inside[ys:ye, xs:xe] = True
        acc += np.where(inside, g * phi(n - c, Ss), 0)         # a neighbour outside w x h contributes 0
        lo, hi = np.where(inside, np.minimum(lo, n), lo), np.where(inside, np.maximum(hi, n), hi)
    s = c + ((acc + 8) >> 4)
    assert (s >= lo).all() and (s <= hi).all(), "stage 1 left the window's minimum / maximum"
    return s


def ref_temporal(s, prev, St):
    """stage 2 on int64 arrays; asserts that the result lies between s and the state"""
    out = s + tdiv(3 * phi(prev - s, St), 4)
    assert (out >= np.minimum(s, prev)).all() and (out <= np.maximum(s, prev)).all(), "stage 2 left the interval between s and P"
    return out


class RefDenoiser:
    """the object of the header's text: per stream the previous output (None: not primed)"""

    def __init__(self, w, h, n_streams, spatial=(0, 0, 0), temporal=(0, 0, 0)):
        self.w, self.h, self.n = w, h, n_streams
        self.state = [None] * n_streams
        self.set_strength(spatial, temporal)

    def set_strength(self, spatial, temporal):
        self.spatial, self.temporal = tuple(int(v) for v in spatial), tuple(int(v) for v in temporal)

    def reset(self, first=0, n=None):
        for k in range(first, first + (self.n - first if n is None else n)):
            self.state[k] = None

    def run(self, frames, first=0, commit=True):
        """packed frames of streams first .. -> the filtered packed frames"""
        frames = np.atleast_2d(frames)
        out = []
        for k, frame in enumerate(frames):
            parts = []
            for i, pl in enumerate(planes_of(frame, self.w, self.h)):
                s = ref_spatial(pl, self.spatial[i])
                if self.state[first + k] is not None:
                    s = ref_temporal(s, planes_of(self.state[first + k], self.w, self.h)[i].astype(np.int64), self.temporal[i])
                assert s.min() >= 0 and s.max() <= 255
                parts.append(s.astype(np.uint8).reshape(-1))
            out.append(np.concatenate(parts))
            if commit:
                self.state[first + k] = out[-1].copy()
        return np.stack(out)


def ref_sequence(w, h, frames, spatial, temporal):
    """what pfv_frames_denoise makes of one stream's frames"""
    ref = RefDenoiser(w, h, 1, spatial, temporal)
    return np.stack([ref.run(f)[0] for f in frames])


# ------------------------------------------------------------------ the device call
def odd_stride(fb):
    s = fb + 21
    return s if s % 16 else s + 1


def run_dev(ctx, dn, w, h, frames, layout=PACKED, first=0, commit=True, src_off=0, src_gap=0, dst_off=0, dst_stride=0, rng=None):
    """pfv_denoiser_run_dev on `frames` ([n, frame bytes of the layout]) as streams first .. -> the n filtered frames.  The source lies src_off
    bytes into its allocation with src_gap random bytes between frames; the destination lies dst_off bytes into a POISONED allocation with 64
    guard bytes on either side, frames dst_stride apart (0: back to back).  Asserts that every byte outside the n frames still holds the poison."""
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
        ctx.check(ctx._lib.pfv_denoiser_run_dev(dn.handle, first, n, P(s_dev + src_off), layout, s_stride if src_gap else 0, P(d_dev + 64 + dst_off), dst_stride,
                                                1 if commit else 0))
        ctx.download(dst, d_dev)
    finally:
        bufs.close()
    got = np.stack([dst[64 + dst_off + k * d_stride: 64 + dst_off + k * d_stride + fb] for k in range(n)])
    rest = dst.copy()
    for k in range(n):
        rest[64 + dst_off + k * d_stride: 64 + dst_off + k * d_stride + fb] = POISON
    assert (rest == POISON).all(), f"bytes outside the {n} frames were written: {np.flatnonzero(rest != POISON)[:8]}"
    return got


STATE_PROBES = [8 + 16 * j for j in range(16)] + [10 + 16 * j for j in range(16)]
_sig = {tuple(int(c + tdiv(3 * phi(np.int64(p - c), 16), 4)) for c in STATE_PROBES) for p in range(256)}
assert len(_sig) == 256, "the state probes do not tell every state value from every other"


def check_state(ctx, dn, ref, w, h):
    """the state of every primed stream equals the restatement's, read through uncommitted runs of constant frames (see the module text);
    an unprimed stream answers with the constant itself.  Strengths are restored; state and flags are not touched."""
    fb = frame_bytes(w, h)
    dn.set_strength((0, 0, 0), (16, 16, 16))
    try:
        for c in STATE_PROBES:
            got = run_dev(ctx, dn, w, h, np.full((ref.n, fb), c, np.uint8), commit=False)
            for k in range(ref.n):
                want = np.full(fb, c, np.int64) if ref.state[k] is None else ref_temporal(np.full(fb, c, np.int64), ref.state[k].astype(np.int64), 16)
                assert np.array_equal(got[k], want), ("state", k, c, np.flatnonzero(got[k] != want)[:8])
    finally:
        dn.set_strength(ref.spatial, ref.temporal)


def smooth(w, h, t, k):
    """a smooth ramp of one frame, drifting with t, per plane"""
    parts = []
    for i, (pw, ph) in enumerate(plane_dims(w, h)):
        yy, xx = np.mgrid[0:ph, 0:pw]
        parts.append((40 + 30 * i + 2 * xx + 3 * yy + 5 * t + 11 * k).reshape(-1))
    return np.concatenate(parts)


def make_frames(w, h, n_frames, n_streams, rng):
    """[frame][stream]: stream 0 seeded random bytes (mostly real edges, the ramp's far side), stream 1 a smooth ramp plus noise within the
    strengths, stream 2 the ramp plus noise that straddles them; clipped, so 0 and 255 occur"""
    fb = frame_bytes(w, h)
    out = np.zeros((n_frames, n_streams, fb), dtype=np.uint8)
    for t in range(n_frames):
        for k in range(n_streams):
            amp = (0, 6, 24)[k % 3]
            out[t, k] = rng.integers(0, 256, fb) if amp == 0 else np.clip(smooth(w, h, t, k) + rng.integers(-amp, amp + 1, fb), 0, 255)
    return out


# ------------------------------------------------------------------ 1. exact equality with numpy
def check_shape(pkg, ctx, w, h, seed=1):
    """3 frames x 3 streams; PACKED and PADDED source (random padding); aligned, and at an unaligned source base with a gap between the
    frames and an unaligned destination whose stride is no multiple of 16 (the byte path).  Output after every committed run and the state
    after the last equal numpy; a picture byte that is not written keeps the poison and so differs."""
    rng = np.random.default_rng(seed * 1000 + w * 7 + h)
    fb = frame_bytes(w, h)
    clip = make_frames(w, h, 3, N_STREAMS, rng)
    ref = RefDenoiser(w, h, N_STREAMS, SPATIAL, TEMPORAL)
    want = np.stack([ref.run(f) for f in clip])
    assert fb < 64 or (want != POISON).any()
    assert not np.array_equal(want, clip) or fb < 64
    for layout in (PACKED, PADDED):
        for unaligned in (False, True):
            kw = dict(src_off=3, src_gap=37, dst_off=5, dst_stride=odd_stride(fb)) if unaligned else {}
            with pkg.Denoiser(ctx, w, h, N_STREAMS, SPATIAL, TEMPORAL) as dn:
                for t in range(3):
                    src = clip[t] if layout == PACKED else np.stack([to_padded(x, w, h, rng) for x in clip[t]])
                    assert src.shape[1] == (fb if layout == PACKED else padded_frame_bytes(w, h))
                    got = run_dev(ctx, dn, w, h, src, layout, rng=rng, **kw)
                    assert np.array_equal(got, want[t]), (w, h, layout, unaligned, t, np.flatnonzero(got != want[t])[:8])
                check_state(ctx, dn, ref, w, h)
    # the host entry point and the Python mirror: frame-major
    got = pkg.frames_denoise(ctx, w, h, clip, SPATIAL, TEMPORAL, n_streams=N_STREAMS)
    assert got.dtype == np.uint8 and np.array_equal(got.reshape(want.shape), want)


# ------------------------------------------------------------------ 2. arithmetic traps
# stage 1: (c, [up-left, up, up-right, left, right, down-left, down, down-right], Ss) -> s, worked out by hand from the text
SPATIAL_TRAPS = [
    # one edge neighbour (weight 2) at distance d, the rest equal to c: the sum is 2 * phi(d)
    ((100, [100, 103, 100, 100, 100, 100, 100, 100], 4), 100),      # |d| = S - 1: 6 + 8 = 14 >> 4 = 0
    ((100, [100, 104, 100, 100, 100, 100, 100, 100], 4), 101),      # |d| = S: the sum is 8: (8 + 8) >> 4 = 1
    ((100, [100, 105, 100, 100, 100, 100, 100, 100], 4), 100),      # |d| = S + 1: phi = 3
    ((100, [100, 100, 100, 107, 107, 100, 107, 107], 4), 100),      # |d| = 2S - 1: phi = 1, sum 2 + 2 + 2 + 1 = 7
    ((100, [100, 108, 100, 108, 108, 100, 108, 100], 4), 100),      # |d| = 2S: phi = 0
    ((100, [109, 109, 109, 109, 109, 109, 109, 109], 4), 100),      # |d| = 2S + 1: a real edge all around, nothing moves
    ((100, [100, 96, 100, 100, 100, 100, 100, 100], 4), 100),       # the sum is -8: (-8 + 8) >> 4 = 0
    ((100, [99, 96, 100, 100, 100, 100, 100, 100], 4), 99),         # the sum is -9: -1 >> 4 = -1 (floor; truncation would give 0)
    ((100, [100, 93, 100, 93, 93, 100, 93, 100], 4), 100),          # falling, |d| = 2S - 1: the sum is -8
    ((100, [100, 92, 100, 92, 92, 100, 92, 100], 4), 100),          # falling, |d| = 2S
    ((100, [100, 91, 100, 91, 91, 100, 91, 100], 4), 100),          # falling, |d| = 2S + 1
    ((100, [100, 97, 100, 100, 100, 100, 100, 100], 4), 100),       # falling, |d| = S - 1: -6 + 8 = 2 >> 4 = 0
    ((100, [100, 95, 100, 100, 100, 100, 100, 100], 4), 100),       # falling, |d| = S + 1: phi = -3, -6 + 8 >> 4 = 0
    ((100, [100, 104, 100, 104, 104, 100, 100, 100], 4), 102),      # the sum is 24: 32 >> 4 = 2
    ((100, [101, 104, 100, 104, 103, 100, 100, 100], 4), 101),      # the sum is 1 + 8 + 8 + 6 = 23: 31 >> 4 = 1
    ((100, [100, 96, 100, 96, 96, 100, 100, 100], 4), 99),          # the sum is -24: -16 >> 4 = -1
    ((100, [99, 96, 100, 96, 96, 100, 100, 100], 4), 98),           # the sum is -25: -17 >> 4 = -2
    ((100, [101, 103, 100, 100, 100, 100, 100, 100], 4), 100),      # the sum is 7: 15 >> 4 = 0
    ((0, [16, 16, 16, 16, 16, 16, 16, 16], 16), 12),                # sample 0, full strength all around: 12 * 16 = 192: 200 >> 4 = 12
    ((255, [239, 239, 239, 239, 239, 239, 239, 239], 16), 243),     # sample 255: -192 + 8 = -184 >> 4 = -12 (exactly)
    ((0, [255, 255, 255, 255, 255, 255, 255, 255], 16), 0),         # the largest difference: far beyond 2S
    ((255, [0, 0, 0, 0, 0, 0, 0, 0], 16), 255),
    ((100, [116, 84, 116, 84, 116, 84, 116, 84], 16), 100),         # +16 and -16 cancel: edges 2 * (-16 - 16 + 16 + 16) = 0, diagonals 16 + 16 - 16 - 16 = 0
    ((7, [9, 9, 9, 9, 9, 9, 9, 9], 1), 7),                          # S = 1: |d| = 2 = 2S, nothing
    ((7, [8, 8, 8, 8, 8, 8, 8, 8], 1), 8),                          # S = 1: 12 + 8 = 20 >> 4 = 1
]
# stage 2: (s, P, St) -> out
TEMPORAL_TRAPS = [
    ((100, 99, 5), 100),        # 3 * -1 = -3: tdiv gives 0 (floor: -1)
    ((100, 98, 5), 99),         # -6: tdiv -1 (floor: -2)
    ((100, 97, 5), 98),         # -9: tdiv -2 (floor: -3)
    ((100, 101, 5), 100),       # 3: 0
    ((100, 102, 5), 101),       # 6: 1
    ((100, 104, 5), 103),       # |d| = S - 1: 12 / 4 = 3
    ((100, 105, 5), 103),       # |d| = S: 15: 3
    ((100, 106, 5), 103),       # |d| = S + 1: phi = 4: 3
    ((100, 109, 5), 100),       # |d| = 2S - 1: phi = 1: 3 / 4 = 0
    ((100, 110, 5), 100),       # |d| = 2S
    ((100, 111, 5), 100),       # |d| = 2S + 1
    ((100, 96, 5), 97),         # falling, S - 1: -12: -3
    ((100, 95, 5), 97),         # falling, S: -15: tdiv -3 (floor: -4)
    ((100, 94, 5), 97),         # falling, S + 1: phi = -4
    ((100, 93, 5), 98),         # falling: phi = -3: -9: tdiv -2
    ((100, 91, 5), 100),        # falling, 2S - 1: phi = -1: -3: 0
    ((100, 90, 5), 100),        # falling, 2S
    ((100, 89, 5), 100),        # falling, 2S + 1
    ((0, 16, 16), 12),          # sample 0: 48 / 4
    ((255, 240, 16), 244),      # sample 255: -45: tdiv -11
    ((0, 255, 16), 0),
    ((255, 0, 16), 255),
    ((100, 107, 0), 100),       # St = 0: stage 2 off
]


def check_traps(pkg, ctx):
    """each stage-1 trap as the 3 x 3 neighbourhood of a luma sample on a 4-pixel grid of a 64 x 48 frame (the rest random), and in the
    picture's interior only, so all eight neighbours exist; each stage-2 trap as a state / input pair at Ss = 0.  The hand-worked values,
    numpy and the device agree.  Corners and edges: see check_borders."""
    w, h = 64, 48
    fb = frame_bytes(w, h)
    rng = np.random.default_rng(5)
    by_s = {}
    for (c, nb, S), want in SPATIAL_TRAPS:
        by_s.setdefault(S, []).append((c, nb, want))
    for S, cases in by_s.items():
        f = rng.integers(0, 256, fb, dtype=np.uint8)
        luma = f[:w * h].reshape(h, w)
        at = []
        for k, (c, nb, want) in enumerate(cases):
            y, x = 2 + 4 * (k // 15), 2 + 4 * (k % 15)
            luma[y - 1:y + 2, x - 1:x + 2] = np.array(nb[:4] + [c] + nb[4:]).reshape(3, 3)
            at.append((y, x, want))
        ref = ref_spatial(luma, S)
        for y, x, want in at:
            assert ref[y, x] == want, ("numpy against the hand-worked value", S, y, x, ref[y, x], want)
        for layout in (PACKED, PADDED):
            with pkg.Denoiser(ctx, w, h, 1, (S, 0, 0), (0, 0, 0)) as dn:
                got = run_dev(ctx, dn, w, h, f if layout == PACKED else to_padded(f, w, h, rng), layout)[0]
            assert np.array_equal(got[:w * h].reshape(h, w), ref) and np.array_equal(got[w * h:], f[w * h:])
            for y, x, want in at:
                assert got[y * w + x] == want, (S, layout, y, x)
    by_t = {}
    for (s, prev, St), want in TEMPORAL_TRAPS:
        by_t.setdefault(St, []).append((s, prev, want))
    for St, cases in by_t.items():
        first, second = rng.integers(0, 256, fb, dtype=np.uint8), rng.integers(0, 256, fb, dtype=np.uint8)
        for k, (s, prev, want) in enumerate(cases):
            first[k], second[k] = prev, s
        ref = RefDenoiser(w, h, 1, (0, 0, 0), (St, St, St))
        with pkg.Denoiser(ctx, w, h, 1, (0, 0, 0), (St, St, St)) as dn:
            assert np.array_equal(run_dev(ctx, dn, w, h, first)[0], first) and np.array_equal(ref.run(first)[0], first)      # unprimed, Ss = 0: a copy
            got, wantf = run_dev(ctx, dn, w, h, second)[0], ref.run(second)[0]
        assert np.array_equal(got, wantf)
        for k, (s, prev, want) in enumerate(cases):
            assert got[k] == want == wantf[k], (St, s, prev, got[k], want)


def check_borders(pkg, ctx):
    """picture corners and edges: a neighbour outside contributes 0, also on a PADDED source whose padding holds 0xFF right beside samples
    of 250 (inside the ramp at S = 16: a padding byte that took part would pull the border up).  2 x 2, 16 x 16, 18 x 34 and 130 x 18 have
    their right / lower borders inside a macroblock, at its end and two samples behind a strip's end."""
    for w, h in ((2, 2), (16, 16), (18, 34), (130, 18)):
        fb = frame_bytes(w, h)
        flat = np.full(fb, 250, np.uint8)
        padded = np.concatenate([np.pad(pl, ((0, pad16(ph) - ph), (0, pad16(pw) - pw)), constant_values=0xFF).reshape(-1)
                                 for pl, (pw, ph) in zip(planes_of(flat, w, h), plane_dims(w, h))])
        assert padded.size == padded_frame_bytes(w, h)
        with pkg.Denoiser(ctx, w, h, 1, (16, 16, 16), (0, 0, 0)) as dn:
            assert np.array_equal(run_dev(ctx, dn, w, h, padded, PADDED)[0], flat), (w, h, "padding took part")
        # a corner sample below its three neighbours: hand-worked, 2 * 8 + 2 * 8 + 8 = 40: 48 >> 4 = 3 (with eight neighbours it would be 96: 6)
        f = np.full(fb, 108, np.uint8)
        luma = f[:w * h].reshape(h, w)
        for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
            luma[y, x] = 100
        want = ref_spatial(luma, 16)
        if w > 2:
            assert want[0, 0] == want[0, w - 1] == want[h - 1, 0] == want[h - 1, w - 1] == 103
            assert want[0, 1] == 107                        # an edge sample beside the corner: five neighbours, one of them 8 below: -16 + 8 >> 4 = -1
        with pkg.Denoiser(ctx, w, h, 1, (16, 0, 0), (0, 0, 0)) as dn:
            for layout in (PACKED, PADDED):
                src = f if layout == PACKED else np.concatenate([np.pad(pl, ((0, pad16(ph) - ph), (0, pad16(pw) - pw)), constant_values=0xFF).reshape(-1)
                                                                 for pl, (pw, ph) in zip(planes_of(f, w, h), plane_dims(w, h))])
                got = run_dev(ctx, dn, w, h, src, layout)[0]
                assert np.array_equal(got[:w * h].reshape(h, w), want), (w, h, layout)


# ------------------------------------------------------------------ 3. properties
def check_properties(pkg, ctx, w=50, h=38):
    rng = np.random.default_rng(11)
    fb = frame_bytes(w, h)
    n = N_STREAMS
    clip = make_frames(w, h, 3, n, rng)
    # the ramp and both stages over every difference and strength, in numpy: bounded by S, odd, zero from 2S on
    d = np.arange(-255, 256, dtype=np.int64)
    for S in range(17):
        f = phi(d, S)
        assert np.abs(f).max() == S and np.array_equal(f, -f[::-1]) and (f[np.abs(d) >= 2 * S] == 0).all() and np.array_equal(f[np.abs(d) <= S], d[np.abs(d) <= S])
    with pkg.Denoiser(ctx, w, h, n) as dn:
        # strengths 0 / 0 copy, primed or not
        for t in range(2):
            assert np.array_equal(run_dev(ctx, dn, w, h, clip[t]), clip[t])
        # constant planes stay constant, whatever the state holds
        dn.set_strength((16, 7, 1), (16, 7, 1))
        flat = np.concatenate([np.full(pw * ph, val, dtype=np.uint8) for (pw, ph), val in zip(plane_dims(w, h), (90, 0, 255))])
        dn.reset()
        for t in range(2):
            assert np.array_equal(run_dev(ctx, dn, w, h, np.stack([flat] * n)), np.stack([flat] * n))
        # spatial only: inside the window's minimum / maximum (ref_spatial asserts it of numpy, equality carries it over)
        dn.reset()
        dn.set_strength((16, 9, 4), (0, 0, 0))
        ref = RefDenoiser(w, h, n, (16, 9, 4), (0, 0, 0))
        for t in range(2):
            assert np.array_equal(run_dev(ctx, dn, w, h, clip[t]), ref.run(clip[t]))
        # temporal only: between s (= the input) and P (= the previous input); identical frames converge to themselves
        dn.reset()
        dn.set_strength((0, 0, 0), (16, 9, 4))
        a, b = clip[0], clip[1]
        assert np.array_equal(run_dev(ctx, dn, w, h, a), a)
        got = run_dev(ctx, dn, w, h, b).astype(np.int64)
        assert (got >= np.minimum(a, b)).all() and (got <= np.maximum(a, b)).all() and not np.array_equal(got, b)
        last = got
        for _ in range(80):      # every step moves a sample that is off by d by at least |d| - tdiv(3|d|, 4) >= 1
            last = run_dev(ctx, dn, w, h, b)
            if np.array_equal(last, b):
                break
        moved = np.abs(got - b.astype(np.int64)) > 0
        assert np.array_equal(last, b), "identical consecutive frames did not converge to themselves"
        assert moved.any()
        # an unprimed stream equals the spatial-only result; reset of a window un-primes only that window
        dn.set_strength(SPATIAL, TEMPORAL)
        ref = RefDenoiser(w, h, n, SPATIAL, TEMPORAL)
        dn.reset()
        only = RefDenoiser(w, h, n, SPATIAL, (0, 0, 0))
        got = run_dev(ctx, dn, w, h, clip[0])
        assert np.array_equal(got, ref.run(clip[0])) and np.array_equal(got, only.run(clip[0]))
        dn.reset(1, 1)
        ref.reset(1, 1)
        got = run_dev(ctx, dn, w, h, clip[1])
        want = ref.run(clip[1])
        assert np.array_equal(got, want)
        assert np.array_equal(got[1], only.run(clip[1])[1]) and not np.array_equal(got[0], only.run(clip[1])[0]) and not np.array_equal(got[2], only.run(clip[1])[2])
        check_state(ctx, dn, ref, w, h)
        # commit = 0 leaves state and flags alone -- on a primed stream and on an unprimed one -- and a committed run of the same frame
        # gives the same output
        dn.reset(2, 1)
        ref.reset(2, 1)
        dry = run_dev(ctx, dn, w, h, clip[2], commit=False)
        assert np.array_equal(dry, ref.run(clip[2], commit=False))
        check_state(ctx, dn, ref, w, h)
        again = run_dev(ctx, dn, w, h, clip[2], commit=False)
        wet = run_dev(ctx, dn, w, h, clip[2])
        assert np.array_equal(again, dry) and np.array_equal(wet, dry) and np.array_equal(wet, ref.run(clip[2]))
        check_state(ctx, dn, ref, w, h)
        # a window of streams: the others' outputs, state and flags stay
        got = run_dev(ctx, dn, w, h, clip[0][1:], first=1)
        assert np.array_equal(got, ref.run(clip[0][1:], first=1))
        check_state(ctx, dn, ref, w, h)


# ------------------------------------------------------------------ 4. locality
def check_locality(pkg, ctx, w, h, px, py):
    """one luma sample changed: the outputs that differ lie within the 3 x 3 around it, in its plane, and are exactly those that differ in
    numpy.  One STATE sample changed (through a first frame filtered with all strengths 0): at most that one output differs."""
    rng = np.random.default_rng(px * 31 + py)
    yy, xx = np.mgrid[0:h, 0:w]
    luma = (100 + xx // 8 * 3 + yy // 8 * 2 + rng.integers(0, 3, (h, w))).astype(np.uint8)        # smooth, so that a change stays inside the ramp
    a = np.concatenate([luma.reshape(-1), rng.integers(0, 256, frame_bytes(w, h) - w * h, dtype=np.uint8)])
    b = a.copy()
    b[py * w + px] = a[py * w + px] + 9
    strengths = ((16, 16, 16), (16, 16, 16))
    allowed = {y * w + x for y in range(max(0, py - 1), min(h, py + 2)) for x in range(max(0, px - 1), min(w, px + 2))}
    ra, rb = RefDenoiser(w, h, 1, *strengths).run(a)[0], RefDenoiser(w, h, 1, *strengths).run(b)[0]
    want = set(np.flatnonzero(ra != rb))
    assert want and want <= allowed and len(want) > 1, sorted(want - allowed)[:8]
    for layout in (PACKED, PADDED):
        out = []
        for f in (a, b):
            with pkg.Denoiser(ctx, w, h, 1, *strengths) as dn:
                out.append(run_dev(ctx, dn, w, h, f if layout == PACKED else to_padded(f, w, h, rng), layout)[0])
        assert np.array_equal(out[0], ra) and np.array_equal(out[1], rb)
        assert set(np.flatnonzero(out[0] != out[1])) == want
    # the state
    nxt = a.copy()
    nxt[:w * h] = np.clip(luma.astype(np.int64) + rng.integers(-2, 3, (h, w)), 0, 255).reshape(-1)
    out, refs = [], []
    for f in (a, b):
        ref = RefDenoiser(w, h, 1)
        with pkg.Denoiser(ctx, w, h, 1) as dn:
            assert np.array_equal(run_dev(ctx, dn, w, h, f)[0], f) and np.array_equal(ref.run(f)[0], f)      # strengths 0: the state is the frame
            dn.set_strength(*strengths)
            ref.set_strength(*strengths)
            out.append(run_dev(ctx, dn, w, h, nxt)[0])
            refs.append(ref.run(nxt)[0])
    assert np.array_equal(out[0], refs[0]) and np.array_equal(out[1], refs[1])
    diff = set(np.flatnonzero(out[0] != out[1]))
    assert diff == {py * w + px}, diff
    return len(want)


# ------------------------------------------------------------------ 5. bad arguments
def check_bad_arguments(pkg, ctx):
    L = pkg._lib
    lib = ctx._lib
    w, h, n = 16, 16, 4
    fb, pfb = frame_bytes(w, h), padded_frame_bytes(w, h)
    bufs = DevBufs(ctx)
    dn = pkg.Denoiser(ctx, w, h, n)
    graph = pkg.Graph(ctx)
    hp = lambda x: x.ctypes.data_as(P)      # noqa: E731
    try:
        a = bufs.put(np.zeros(8 * pfb, dtype=np.uint8))
        d = bufs.put(np.zeros(8 * pfb, dtype=np.uint8))

        def create(ctx_h=ctx.handle, w=w, h=h, n=1):
            err = ctypes.c_int(-99)
            hnd = lib.pfv_denoiser_create(ctx_h, w, h, n, ctypes.byref(err))
            if hnd:
                lib.pfv_denoiser_destroy(hnd)
            return bool(hnd), err.value
        assert create() == (True, L.PFV_OK)
        assert lib.pfv_denoiser_create(None, w, h, 1, None) is None
        for bad in ((15, 16), (16, 17), (0, 16), (16, -2), (65536, 16)):
            assert create(w=bad[0], h=bad[1]) == (False, L.PFV_ERR_BAD_ARG), bad
        assert create(n=0) == (False, L.PFV_ERR_BAD_ARG) and create(n=-1) == (False, L.PFV_ERR_BAD_ARG) and create(ctx_h=None) == (False, L.PFV_ERR_BAD_ARG)
        lib.pfv_denoiser_destroy(None)
        # strengths
        ok = np.array([1, 2, 3], np.uint8)
        assert lib.pfv_denoiser_set_strength(dn.handle, hp(ok), hp(ok)) == L.PFV_OK
        assert lib.pfv_denoiser_set_strength(None, hp(ok), hp(ok)) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_denoiser_set_strength(dn.handle, None, hp(ok)) == L.PFV_ERR_BAD_ARG and lib.pfv_denoiser_set_strength(dn.handle, hp(ok), None) == L.PFV_ERR_BAD_ARG
        for k in range(3):
            for v, rc in ((16, L.PFV_OK), (17, L.PFV_ERR_BAD_ARG), (255, L.PFV_ERR_BAD_ARG)):
                st = ok.copy()
                st[k] = v
                assert lib.pfv_denoiser_set_strength(dn.handle, hp(st), hp(ok)) == rc and lib.pfv_denoiser_set_strength(dn.handle, hp(ok), hp(st)) == rc, (k, v)
        with pytest.raises(pkg.PfvError):
            dn.set_strength((17, 0, 0), (0, 0, 0))
        # reset
        assert lib.pfv_denoiser_reset(dn.handle, 0, n) == L.PFV_OK and lib.pfv_denoiser_reset(dn.handle, n - 1, 1) == L.PFV_OK
        assert lib.pfv_denoiser_reset(None, 0, 1) == L.PFV_ERR_BAD_ARG
        for first, cnt in ((-1, 1), (0, 0), (0, n + 1), (n, 1), (1, n), (0, -1), (2**31 - 1, 2)):
            assert lib.pfv_denoiser_reset(dn.handle, first, cnt) == L.PFV_ERR_BAD_ARG, (first, cnt)

        def call(first=0, cnt=1, src=a, layout=PACKED, ss=0, dst=d, ds=0, commit=1, h_=None):
            return lib.pfv_denoiser_run_dev(dn.handle if h_ is None else h_, first, cnt, P(src) if src else None, layout, ss, P(dst) if dst else None, ds, commit)
        assert call() == L.PFV_OK and call(cnt=n, layout=PADDED) == L.PFV_OK and call(first=n - 1) == L.PFV_OK
        assert lib.pfv_denoiser_run_dev(None, 0, 1, P(a), PACKED, 0, P(d), 0, 1) == L.PFV_ERR_BAD_ARG
        for first, cnt in ((-1, 1), (0, 0), (0, n + 1), (n, 1), (1, n), (0, -1), (2**31 - 1, 2)):      # a window outside n_streams
            assert call(first=first, cnt=cnt) == L.PFV_ERR_BAD_ARG, (first, cnt)
        assert call(layout=2) == L.PFV_ERR_BAD_ARG and call(layout=-1) == L.PFV_ERR_BAD_ARG
        assert call(src=None) == L.PFV_ERR_BAD_ARG and call(dst=None) == L.PFV_ERR_BAD_ARG
        assert call(cnt=2, ds=fb - 1) == L.PFV_ERR_BAD_ARG and call(cnt=2, ds=fb) == L.PFV_OK
        assert call(cnt=2, ss=fb - 1) == L.PFV_ERR_BAD_ARG and call(cnt=2, layout=PADDED, ss=pfb - 1) == L.PFV_ERR_BAD_ARG
        assert call(cnt=2, layout=PADDED, ss=pfb) == L.PFV_OK
        # in-place and overlapping ranges, either way round
        assert call(dst=a) == L.PFV_ERR_BAD_ARG
        assert call(dst=a + fb - 1) == L.PFV_ERR_BAD_ARG and call(dst=a + fb) == L.PFV_OK
        assert call(src=a + fb, dst=a + 1) == L.PFV_ERR_BAD_ARG and call(src=a + fb, dst=a) == L.PFV_OK
        assert call(cnt=2, src=a + fb, dst=a, ds=2 * fb) == L.PFV_ERR_BAD_ARG      # the source lies in the destination's gap
        assert call(layout=PADDED, dst=a + pfb - 1) == L.PFV_ERR_BAD_ARG and call(layout=PADDED, dst=a + pfb) == L.PFV_OK
        # (a buffer overlapping the STATE is refused too, but the ABI hands out no pointer into the denoiser's own allocation: no caller
        # can build that case, and no test here does)
        ctx.sync()
        # the host form
        host, out = np.zeros(2 * n * fb, np.uint8), np.zeros(2 * n * fb, np.uint8)

        def hcall(c=ctx.handle, w=w, h=h, n_=n, nf=2, src=host, dst=out, sp=ok, tp=ok):
            return lib.pfv_frames_denoise(c, w, h, n_, nf, hp(src) if src is not None else None, hp(dst) if dst is not None else None,
                                          hp(sp) if sp is not None else None, hp(tp) if tp is not None else None)
        assert hcall() == L.PFV_OK
        assert hcall(c=None) == L.PFV_ERR_BAD_ARG and hcall(w=15) == L.PFV_ERR_BAD_ARG and hcall(h=0) == L.PFV_ERR_BAD_ARG
        assert hcall(n_=0) == L.PFV_ERR_BAD_ARG and hcall(nf=0) == L.PFV_ERR_BAD_ARG and hcall(nf=-1) == L.PFV_ERR_BAD_ARG
        assert hcall(src=None) == L.PFV_ERR_BAD_ARG and hcall(dst=None) == L.PFV_ERR_BAD_ARG and hcall(sp=None) == L.PFV_ERR_BAD_ARG and hcall(tp=None) == L.PFV_ERR_BAD_ARG
        assert hcall(sp=np.array([0, 17, 0], np.uint8)) == L.PFV_ERR_BAD_ARG and hcall(tp=np.array([0, 0, 17], np.uint8)) == L.PFV_ERR_BAD_ARG
        # while a graph is being recorded: creation and the host form refuse; a run that needs the priming memset refuses, one that does
        # not is recorded
        fresh = pkg.Denoiser(ctx, w, h, n)
        try:
            assert call(cnt=n) == L.PFV_OK          # dn: every stream primed
            with graph:
                assert create() == (False, L.PFV_ERR_STATE)
                assert hcall() == L.PFV_ERR_STATE
                assert call(cnt=n) == L.PFV_OK
                assert call(cnt=n, h_=fresh.handle) == L.PFV_ERR_STATE
                assert call(cnt=n, h_=fresh.handle, commit=0) == L.PFV_OK
                assert call(first=1, cnt=1, h_=fresh.handle) == L.PFV_ERR_STATE
            assert call(first=1, cnt=1, h_=fresh.handle) == L.PFV_OK
            ctx.sync()
        finally:
            fresh.close()
    finally:
        graph.close()
        dn.close()
        bufs.close()


# ------------------------------------------------------------------ 6. graph
def check_graph(pkg, ctx, w=144, h=48, n=2):
    """a steady-state run recorded once and replayed over three frames equals numpy; the first frame, which primes, runs before the recording"""
    rng = np.random.default_rng(17)
    fb = frame_bytes(w, h)
    clip = make_frames(w, h, 4, n, rng)
    ref = RefDenoiser(w, h, n, SPATIAL, TEMPORAL)
    bufs = DevBufs(ctx)
    dn, fresh = pkg.Denoiser(ctx, w, h, n, SPATIAL, TEMPORAL), pkg.Denoiser(ctx, w, h, n, SPATIAL, TEMPORAL)
    graph = pkg.Graph(ctx)
    try:
        s_dev, d_dev = bufs.put(clip[0]), bufs.put(np.full(n * fb, POISON, np.uint8))
        dn.run_dev(s_dev, d_dev)
        got = np.zeros((n, fb), np.uint8)
        ctx.download(got, d_dev)
        assert np.array_equal(got, ref.run(clip[0]))
        with graph:
            with pytest.raises(pkg.PfvError) as e:        # not primed: the memset behind the kernel cannot be recorded
                fresh.run_dev(s_dev, d_dev)
            assert e.value.code == pkg._lib.PFV_ERR_STATE
            dn.run_dev(s_dev, d_dev)
        for t in range(1, 4):
            ctx.upload(s_dev, clip[t])
            ctx.upload(d_dev, np.full(n * fb, POISON, np.uint8))
            graph.launch()
            ctx.download(got, d_dev)
            assert np.array_equal(got, ref.run(clip[t])), t
        check_state(ctx, dn, ref, w, h)
    finally:
        graph.close()
        dn.close()
        fresh.close()
        bufs.close()


# ------------------------------------------------------------------ 7. encoder session
def noisy_clip(pkg, w, h, n_frames, seed, kind="pan"):
    """a synthetic stream plus seeded uniform noise in [-3, 3], clipped"""
    st = pkg.SyntheticStream(w, h, seed=seed, kind=kind)
    rng = np.random.default_rng(seed)
    return np.stack([np.clip(st.frame(t).astype(np.int64) + rng.integers(-3, 4, frame_bytes(w, h)), 0, 255).astype(np.uint8) for t in range(n_frames)])


def check_enc_session(pkg, ctx, w=96, h=32, quality=2, n=3):
    """I P P of three slots, the window set to slots [1, 3): pfv_enc_denoise_dev with a source stride, then one probe and the encode calls on
    the returned pointer, against a twin session fed the restatement's frames through the same window; slot 0 of the session's buffer keeps
    what the first, full-window call put there"""
    import ingest_cases as ic
    rng = np.random.default_rng(61)
    L = pkg._lib
    fb = frame_bytes(w, h)
    s_stride = fb + 48
    strengths = ((6, 5, 4), (8, 6, 16))
    enc, twin = (pkg.EncoderSession(ctx, w, h, quality, n) for _ in range(2))
    dn = pkg.Denoiser(ctx, w, h, n, *strengths)
    ref = RefDenoiser(w, h, n, *strengths)
    bufs = DevBufs(ctx)
    clips = [noisy_clip(pkg, w, h, 4, 61 + k) for k in range(n)]

    def lay(frames):
        buf = rng.integers(0, 256, n * s_stride, dtype=np.uint8)
        for k in range(n):
            buf[k * s_stride:k * s_stride + fb] = frames[k]
        return buf
    try:
        tb = enc.total_blocks
        out, tout = ic.EncBufs(ctx, bufs, n, tb), ic.EncBufs(ctx, bufs, n, tb)
        first = np.stack([c[3] for c in clips])
        base = enc.denoise_dev(dn, bufs.put(lay(first)), s_stride)           # all slots: allocates the buffer, primes every stream
        slot0 = ref.run(first)[0]
        for s in (enc, twin):
            s.set_window(1, 2)
        sizes_d, tsizes_d = (bufs.put(np.full(n, 0x5A5A5A5A, np.uint32)) for _ in range(2))
        for t in range(3):
            src = np.stack([c[t] for c in clips])
            dry = ref.run(src[1:], first=1, commit=False)
            ptr = enc.denoise_dev(dn, bufs.put(lay(src)), s_stride, commit=False)      # what a probe would see
            assert ptr == base and ptr % 16 == 0, "one buffer, owned by the session"
            held = np.zeros((n, fb), np.uint8)
            ctx.download(held, ptr)
            assert np.array_equal(held[1:], dry) and np.array_equal(held[0], slot0), (t, "uncommitted")
            frames = np.concatenate([slot0[None], ref.run(src[1:], first=1)])
            assert np.array_equal(frames[1:], dry)
            assert enc.denoise_dev(dn, bufs.put(lay(src)), s_stride) == base
            ctx.download(held, ptr)
            assert np.array_equal(held, frames), (t, "the session's frame buffer")
            assert not np.array_equal(held[1:], src[1:])
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
            assert (out.read()[0][1:] != 0x5A5A).any() and (out.read()[0][0] == 0x5A5A).all()
            assert np.array_equal(enc.prev_frame(), twin.prev_frame()), (t, "pfv_enc_prev_frame")
        check_state(ctx, dn, ref, w, h)
        # bad arguments
        src_dev = bufs.put(lay(src))
        f = ctx._lib.pfv_enc_denoise_dev
        o = ctypes.c_void_p()
        assert f(None, dn.handle, P(src_dev), s_stride, 1, ctypes.byref(o)) == L.PFV_ERR_BAD_ARG
        assert f(enc.handle, None, P(src_dev), s_stride, 1, ctypes.byref(o)) == L.PFV_ERR_BAD_ARG
        assert f(enc.handle, dn.handle, None, s_stride, 1, ctypes.byref(o)) == L.PFV_ERR_BAD_ARG
        assert f(enc.handle, dn.handle, P(src_dev), s_stride, 1, None) == L.PFV_ERR_BAD_ARG
        assert f(enc.handle, dn.handle, P(src_dev), fb - 1, 1, ctypes.byref(o)) == L.PFV_ERR_BAD_ARG
        assert f(enc.handle, dn.handle, P(base), 0, 1, ctypes.byref(o)) == L.PFV_ERR_BAD_ARG                      # the source is the session's own buffer
        for other in (pkg.Denoiser(ctx, w, h, n + 1), pkg.Denoiser(ctx, w, h - 2, n), pkg.Denoiser(ctx, w + 2, h, n)):
            assert f(enc.handle, other.handle, P(src_dev), s_stride, 1, ctypes.byref(o)) == L.PFV_ERR_BAD_ARG     # stream count, size
            other.close()
        enc.set_frame_stride(fb + 16)
        with pytest.raises(pkg.PfvError) as e:
            enc.denoise_dev(dn, src_dev, s_stride)
        assert e.value.code == L.PFV_ERR_STATE
        enc.set_frame_stride(0)
        # a session whose first call falls inside a recording is refused; this one's is recorded
        late = pkg.EncoderSession(ctx, w, h, quality, n)
        graph = pkg.Graph(ctx)
        try:
            with graph:
                with pytest.raises(pkg.PfvError) as e:
                    late.denoise_dev(dn, src_dev, s_stride)
                assert e.value.code == L.PFV_ERR_STATE
                assert enc.denoise_dev(dn, src_dev, s_stride) == base
        finally:
            graph.close()
            late.close()
        ctx.sync()
    finally:
        bufs.close()
        enc.close()
        twin.close()
        dn.close()


# ------------------------------------------------------------------ 8. pfv_encoder
ENCODER_CONFIGS = {
    "device": dict(device_entropy=True, kw=dict(quality=2)),
    "host": dict(device_entropy=False, kw=dict(quality=2)),
    "budget_device": dict(device_entropy=True, kw=dict(quality=None, qualities=[1, 2, 5], iframe_budget=1500, pframe_quality_floor=38.0)),
    "budget_host": dict(device_entropy=False, kw=dict(quality=None, qualities=[1, 2, 5], iframe_budget=1500, pframe_quality_floor=38.0)),
    "encode_frame": dict(device_entropy=True, kw=dict(quality=None, qualities=[1, 5, 10]), auto=True),
    "chain_device": dict(device_entropy=True, kw=dict(quality=2), rgb=("rgb8", "box"), size=(80, 54)),
    "chain_host": dict(device_entropy=False, kw=dict(quality=2), rgb=("bgra8", "point"), size=(80, 54)),
}
ENC_STRENGTHS = ((6, 4, 5), (8, 16, 3))


def check_encoder(pkg, ctx, oracle, config, w=48, h=32, n_frames=5):
    """twin encoders over (i, p, p, i, p): one with set_denoise (chained configurations: behind set_input_rgb and set_input_size), one fed the
    frames pfv_frames_denoise made of the sequence -- which equal the restatement's.  The drained bytes are identical after every call, and
    so are rungs, frame reports, frame SSIM; the six probe calls between the encodes give the twin's outputs on the filtered frame and
    change nothing in the stream.  The plain configurations' bytes also equal the ORACLE stream encoder's on the restatement's frames.
    Switched off again, the planar calls give the twin's bytes."""
    import ingest_cases as ic
    import scale_cases as scc
    cfg = ENCODER_CONFIGS[config]
    rng = np.random.default_rng(83)
    sw, sh = cfg.get("size", (w, h))
    order = [0, 0, 1, 2, 3] if cfg.get("auto") else list(range(n_frames))
    clip = noisy_clip(pkg, sw, sh, 5, 83)
    src = [clip[t] for t in order]
    if cfg.get("rgb"):
        fmt, chroma = cfg["rgb"]
        ins = [ic.in_format(ic.onp.yuv420_to_rgb(f, sw, sh), fmt, rng) for f in src]
        src = [pkg.frames_from_rgb(ctx, sw, sh, p, fmt, chroma)[0] for p in ins]
    else:
        ins = [pkg.VideoFrame.from_packed(sw, sh, f) for f in src]
    sized = pkg.frames_scale(ctx, sw, sh, w, h, np.stack(src), "bicubic") if cfg.get("size") else np.stack(src)
    filt = pkg.frames_denoise(ctx, w, h, sized, *ENC_STRENGTHS)
    assert np.array_equal(filt, ref_sequence(w, h, sized, *ENC_STRENGTHS)) and not np.array_equal(filt, sized)
    planes = [pkg.VideoFrame.from_packed(w, h, f) for f in filt]
    a_buf, b_buf = io.BytesIO(), io.BytesIO()
    mk = lambda buf: pkg.Encoder(buf, w, h, 30, ctx=ctx, device_entropy=cfg["device_entropy"], frame_report=True, frame_ssim=True, **cfg["kw"])      # noqa: E731
    a, b = mk(a_buf), mk(b_buf)
    try:
        if cfg.get("rgb"):
            a.set_input_rgb(True, fmt, chroma)
        if cfg.get("size"):
            a.set_input_size(sw, sh, "bicubic")
        a.set_denoise(True, *ENC_STRENGTHS)
        for t, (x_in, fr) in enumerate(zip(ins, planes)):
            if t > 0:
                before = a_buf.getvalue()
                for name in ("probe_iframe", "probe_iframe_rd", "probe_iframe_ssim", "probe_pframe", "probe_pframe_rd", "probe_pframe_ssim"):
                    x, y = getattr(a, name)(x_in), getattr(b, name)(fr)
                    x, y = (x, y) if isinstance(x, tuple) else ((x,), (y,))
                    assert len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y)), (config, t, name, x, y)
                assert a_buf.getvalue() == before
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
        if config in ("device", "host"):
            from oracle_bind import OracleStreamEncoder
            so = OracleStreamEncoder(oracle, w, h, 30, cfg["kw"]["quality"])
            for t, f in enumerate(ref_sequence(w, h, sized, *ENC_STRENGTHS)):
                (so.encode_iframe if t in (0, 3) else so.encode_pframe)(f)
            assert a_buf.getvalue() == so.bytes()[:len(a_buf.getvalue())], "the oracle encoder fed the restatement's frames"
        # switched off again, the planar calls give the bytes they give on the twin
        a.set_denoise(False)
        if cfg.get("size"):
            a.set_input_size(0)
        if cfg.get("rgb"):
            a.set_input_rgb(False)
        for e in (a, b):
            e.encode_iframe(planes[1])
            e.encode_pframe(planes[2])
            e.finish()
        assert a_buf.getvalue() == b_buf.getvalue(), (config, "after set_denoise(off)")
        # bad arguments of the switch
        lib, L = ctx._lib, pkg._lib
        ok = np.array([1, 2, 3], np.uint8)
        hp = lambda x: x.ctypes.data_as(P)      # noqa: E731
        assert lib.pfv_encoder_set_denoise(None, 1, hp(ok), hp(ok)) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_encoder_set_denoise(a.handle, 1, None, hp(ok)) == L.PFV_ERR_BAD_ARG and lib.pfv_encoder_set_denoise(a.handle, 1, hp(ok), None) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_encoder_set_denoise(a.handle, 1, hp(np.array([0, 17, 0], np.uint8)), hp(ok)) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_encoder_set_denoise(a.handle, 1, hp(ok), hp(np.array([0, 0, 255], np.uint8))) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_encoder_set_denoise(a.handle, 0, None, None) == L.PFV_OK
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ 9. direction of the effect
EFFECT_STRENGTHS = ((6, 6, 6), (6, 6, 6))
EFFECT_QUALITIES = (1, 2)


def effect_clip(w=176, h=144, n_frames=6):
    """a static smooth field (luma 128 + 60 sin(x/23) cos(y/17) + 40 sin((x+y)/41), chroma sampled from it at the even positions) with a
    40 x 32 box of other content that moves by (2, 1) per frame: slow motion over a background a p-frame can skip"""
    out = []
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    field = np.clip(np.rint(128 + 60 * np.sin(xx / 23) * np.cos(yy / 17) + 40 * np.sin((xx + yy) / 41)), 0, 255).astype(np.uint8)
    for t in range(n_frames):
        f = field.copy()
        x0, y0 = 20 + 2 * t, 30 + t
        f[y0:y0 + 32, x0:x0 + 40] = 200 - f[y0:y0 + 32, x0:x0 + 40] // 2
        c = f[::2, ::2]
        out.append(np.concatenate([f.reshape(-1), c.reshape(-1), c.reshape(-1)]))
    return np.stack(out)


def psnr_yuv(pkg, a, b):
    d = (a.astype(np.int64) - b.astype(np.int64)) ** 2
    return pkg.psnr(int(d.sum()), d.size)


def check_effect(pkg, ctx, quality, w=176, h=144):
    """I + 5 P of the clip plus seeded uniform noise in [-3, 3], clipped, with and without the filter: STRICTLY fewer stream bytes, STRICTLY
    more skipped p-frame macroblocks, and the filtered input STRICTLY closer to the clean clip (PSNR-YUV) than the noisy one.  Conditions,
    not tolerances; the figures are printed before the assert (recorded in the module text and in profiles/denoise.md)."""
    clean = effect_clip(w, h)
    rng = np.random.default_rng(2024)
    noisy = np.clip(clean.astype(np.int64) + rng.integers(-3, 4, clean.shape), 0, 255).astype(np.uint8)
    filt = pkg.frames_denoise(ctx, w, h, noisy, *EFFECT_STRENGTHS)
    res = {}
    for name, on in (("plain", False), ("filtered", True)):
        buf = io.BytesIO()
        e = pkg.Encoder(buf, w, h, 30, quality, ctx)
        sess = pkg.EncoderSession(ctx, w, h, quality, 1)
        try:
            if on:
                e.set_denoise(True, *EFFECT_STRENGTHS)
            skipped = total = 0
            for t, f in enumerate(noisy):
                (e.encode_iframe if t == 0 else e.encode_pframe)(pkg.VideoFrame.from_packed(w, h, f))
                g = filt[t] if on else f
                if t == 0:
                    sess.encode_iframe(g)
                else:
                    _, has, _ = sess.encode_pframe(g)
                    skipped, total = skipped + int((has == 0).sum()), total + has.size
            e.finish()
        finally:
            e.close()
            sess.close()
        res[name] = (len(buf.getvalue()), skipped, total)
    p_noisy, p_filt = psnr_yuv(pkg, noisy, clean), psnr_yuv(pkg, filt, clean)
    print(f"denoise effect q{quality}: bytes {res['plain'][0]} -> {res['filtered'][0]}, skipped {res['plain'][1]} -> {res['filtered'][1]} of {res['plain'][2]}, "
          f"PSNR-YUV against the clean clip {p_noisy:.2f} -> {p_filt:.2f} dB")
    assert res["filtered"][0] < res["plain"][0], res
    assert res["filtered"][1] > res["plain"][1], res
    assert p_filt > p_noisy, (p_noisy, p_filt)
    return res, p_noisy, p_filt


# ------------------------------------------------------------------ 10. C++ mirror and tool
def build_cpp(lib_path, exe):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "denoise_report.cpp"), "-o", exe, lib_path, "-Wl,-rpath," + os.path.dirname(lib_path)], check=True)


def check_cpp(pkg, ctx, exe, tmp_path, w=48, h=32, quality=2):
    """tests/cpp/denoise_report.cpp (pfv::Encoder::set_denoise, pfv::frames_denoise, pfv::Denoiser): the stream equals a plain Python encoder's
    fed numpy's frames, the filtered frames equal numpy's"""
    clip = noisy_clip(pkg, w, h, 5, 29)
    want = ref_sequence(w, h, clip, *ENC_STRENGTHS)
    src, o1, o2 = str(tmp_path / "in.yuv"), str(tmp_path / "out.pfv"), str(tmp_path / "out.yuv")
    clip.tofile(src)
    r = subprocess.run([exe, src, str(w), str(h), str(quality), *[str(v) for v in ENC_STRENGTHS[0] + ENC_STRENGTHS[1]], o1, o2], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == [f"frames 5 of {w}x{h}, {frame_bytes(w, h)} bytes each"]
    assert np.array_equal(np.fromfile(o2, dtype=np.uint8).reshape(5, -1), want)
    buf = io.BytesIO()
    e = pkg.Encoder(buf, w, h, 30, quality, ctx)
    try:
        for t, f in enumerate(want):
            (e.encode_iframe if t % 3 == 0 else e.encode_pframe)(pkg.VideoFrame.from_packed(w, h, f))
        e.finish()
    finally:
        e.close()
    assert open(o1, "rb").read() == buf.getvalue()


def check_rd_tool(pkg, oracle, lib_path, tmp_path, w=64, h=48, n_frames=4, gop=3, qualities=(1, 2), ss=6, st=5):
    """tools/rd_curve.py --denoise --dump on the library at lib_path: the dumped filtered clip is numpy's of the dumped noisy clip, and the
    dn_ / noisy_ columns equal a recomputation from the dumped frames with the ORACLE encoder; without the flag the lines are the same minus
    the new keys.  --time-denoise prints its row."""
    from oracle_bind import OracleStreamEncoder
    env = dict(os.environ)
    if lib_path:
        env["PFV_HIP_LIB"] = lib_path
    dump = str(tmp_path / "dump")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "rd_curve.py"), str(w), str(h), str(n_frames), "--gop", str(gop), "--kind", "low_motion",
           "--qualities", ",".join(str(q) for q in qualities)]
    plain = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert plain.returncode == 0, plain.stderr
    r = subprocess.run(cmd + ["--denoise", f"{ss},{st}", "--dump", dump, "--time-denoise"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr
    lines = [json.loads(x) for x in r.stdout.splitlines()]
    timing = lines.pop()["time_denoise"]
    assert all(timing[k] >= 0 for k in ("denoise_packed_ms", "denoise_padded_ms", "deblock_ms", "crop_ms"))      # the emulator's events read 0
    new = ("pframe_macroblocks",)
    stripped = [{k: v for k, v in d.items() if k not in new and not k.startswith(("dn_", "noisy_"))} for d in lines]
    assert [json.dumps(d) for d in stripped] == plain.stdout.splitlines()
    fb = frame_bytes(w, h)
    stream = pkg.SyntheticStream(w, h, kind="low_motion")
    for d in lines:
        q = d["quality"]
        clean, noisy, filt = (np.fromfile(os.path.join(dump, f"q{q}_{name}.yuv"), dtype=np.uint8).reshape(n_frames, fb) for name in ("clean", "noisy", "denoised"))
        assert all(np.array_equal(clean[t], stream.frame(t)) for t in range(n_frames))
        diff = noisy.astype(np.int64) - clean
        assert diff.min() >= -3 and diff.max() <= 3 and diff.any()
        assert np.array_equal(filt, ref_sequence(w, h, noisy, (ss,) * 3, (st,) * 3))
        assert d["dn_strength"] == [ss, st]
        for key, frames in (("noisy", noisy), ("dn", filt)):
            so, oe = OracleStreamEncoder(oracle, w, h, 30, q), oracle.encoder(w, h, q)
            skipped = total = 0
            for t, f in enumerate(frames):
                if t % gop == 0:
                    so.encode_iframe(f)
                    oe.encode_iframe(f)
                else:
                    so.encode_pframe(f)
                    _, has, _ = oe.encode_pframe(f)
                    skipped, total = skipped + int((has == 0).sum()), total + has.size
            so.finish()
            assert d[f"{key}_stream_bytes"] == len(so.bytes()) and d[f"{key}_bytes_per_frame"] == len(so.bytes()) / n_frames, key
            assert d[f"{key}_skipped"] == skipped and d[f"{key}_skipped_share"] == skipped / total and d["pframe_macroblocks"] == total, key
            assert d[f"{key}_psnr_clean"] == psnr_yuv(pkg, frames, clean), key
    return lines
