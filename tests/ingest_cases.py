"""Shared checks of the RGB / RGBA picture input (include/pfv_hip_ext.h, "RGB / RGBA picture input"; k_ingest_rgb), driven on the CPU emulator
by tests/test_emu_ingest.py and on a real MI355X by tests/test_gpu_ingest.py through the same fixtures.

The references: for POINT `rgb_to_yuv420` of oracle/pfv_oracle_np.py (the reference's load_frame + from_planes in numpy float32), the alpha
dropped and BGRA8's channels reversed by `rgb_of` below; for BOX `box_frame` below, a restatement of the header's rule over the per-pixel u8
U and V of the oracle's own three expressions, pinned to the oracle at the even pixels.  Every comparison is EQUALITY.  Destinations are
filled with a sentinel first, and every byte outside the frames -- gaps between frames, 64 guard bytes on either side -- must still hold it
afterwards.  A frame byte that is not written keeps the sentinel too and so differs from the reference (random pictures)."""
import ctypes
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import deblock_cases as dc
import quality_cases as qc
from golden_recompute import onp
from present_cases import BPP, FORMATS, GUARD, SENTINEL, round_up
from quality_cases import DevBufs, frame_bytes

ROOT = qc.ROOT
CHROMAS = {"point": 0, "box": 1}
# 2x2 one chroma sample; 6x4 no full group; 8x2 exactly one 8-pixel group (and half a band of row pairs); 12x2 a group plus a 4-pixel rest;
# 18x18 a ragged last group of 2; 20x6 chroma rows of 10 bytes; 24x6 the first width with everything aligned; 34x130 / 130x34 more than one
# workgroup, ragged both ways; 144x48 three macroblock rows; 256x16 the wide path throughout.
# The mapping's own seam: a lane owns kIngestPairs = 2 row pairs, so a height with an odd number of row pairs ends in half a band -- on the
# wide path 8x2 and 24x6, on the byte path 2x2, 12x2, 18x18, 20x6, 34x130, 130x34; 24x4 and 16x8 add whole bands at the smallest wide widths.
SHAPES = [(2, 2), (6, 4), (8, 2), (12, 2), (18, 18), (20, 6), (24, 6), (34, 130), (130, 34), (144, 48), (256, 16), (24, 4), (16, 8)]
P = ctypes.c_void_p


# ------------------------------------------------------------------ the references
def rgb_of(pic, fmt):
    """a picture [h, w, 3 or 4] in `fmt` -> [h, w, 3] R, G, B: the alpha dropped, BGRA8's channels reversed"""
    return np.ascontiguousarray(pic[..., :3] if fmt != "bgra8" else pic[..., 2::-1])


def full_planes(rgb):
    """the per-pixel u8 Y, U, V at full resolution: the oracle's three expressions and its _as_u8"""
    f = np.float32
    r, g, b = (rgb[..., k].astype(f) for k in range(3))
    y = (f(0.299) * r + f(0.587) * g) + f(0.114) * b
    u = ((f(128.0) - f(0.168736) * r) - f(0.331264) * g) + f(0.5) * b
    v = ((f(128.0) + f(0.5) * r) - f(0.418688) * g) - f(0.081312) * b
    return onp._as_u8(y), onp._as_u8(u), onp._as_u8(v)


def box_frame(rgb):
    """PFV_CHROMA_BOX of the header: chroma sample (cx, cy) = (a + b + c + d + 2) >> 2 over the u8 values of pixels (2cx + {0,1}, 2cy + {0,1})"""
    h, w = rgb.shape[:2]
    point = onp.rgb_to_yuv420(rgb)
    y, u, v = full_planes(rgb)
    n, nc = w * h, (w // 2) * (h // 2)
    assert np.array_equal(y.reshape(-1), point[:n]) and np.array_equal(u[0::2, 0::2].reshape(-1), point[n:n + nc]) \
        and np.array_equal(v[0::2, 0::2].reshape(-1), point[n + nc:]), "the restatement left the oracle"

    def box(p):
        q = p.astype(np.uint32)
        return ((q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    return np.concatenate([y.reshape(-1), box(u).reshape(-1), box(v).reshape(-1)])


def want_frame(pic, fmt, chroma):
    rgb = rgb_of(pic, fmt)
    return onp.rgb_to_yuv420(rgb) if chroma == "point" else box_frame(rgb)


def want_frames(pics, fmt, chroma):
    return np.stack([want_frame(p, fmt, chroma) for p in pics])


def in_format(rgb, fmt, rng):
    """[..., 3] R, G, B -> the picture in `fmt`; the alpha bytes of the 4-byte formats are random"""
    if fmt == "rgb8":
        return np.ascontiguousarray(rgb)
    alpha = rng.integers(0, 256, rgb.shape[:-1] + (1,), dtype=np.uint8)
    return np.ascontiguousarray(np.concatenate([rgb if fmt == "rgba8" else rgb[..., ::-1], alpha], axis=-1))


def random_pictures(n, w, h, fmt, rng):
    return rng.integers(0, 256, (n, h, w, BPP[fmt]), dtype=np.uint8)


def lay_out(pics, fmt, off, pitch, stride, rng):
    """the pictures `off` bytes into a buffer of random bytes, rows `pitch` apart, pictures `stride` apart"""
    n, h, w = pics.shape[:3]
    row = w * BPP[fmt]
    src = rng.integers(0, 256, off + (n - 1) * stride + h * pitch + 16, dtype=np.uint8)
    for k in range(n):
        for y in range(h):
            o = off + k * stride + y * pitch
            src[o:o + row] = pics[k, y].reshape(-1)
    return src


def ingest_dev(ctx, pics, fmt, chroma, src_off=0, pitch=0, stride=0, dst_off=0, dst_stride=0, rng=None):
    """pfv_frames_from_rgb_dev on `pics` ([n, h, w, bpp]) -> the n frames.  The source lies src_off bytes into its allocation; the destination
    lies GUARD + dst_off bytes into an allocation full of the sentinel, which is asserted to survive everywhere outside the frames."""
    n, h, w = pics.shape[:3]
    rng = rng or np.random.default_rng(7)
    row, fb = w * BPP[fmt], frame_bytes(w, h)
    e_pitch = pitch or row
    e_stride = stride or e_pitch * h
    e_dst = dst_stride or fb
    src = lay_out(pics, fmt, src_off, e_pitch, e_stride, rng)
    dst = np.full(GUARD + dst_off + (n - 1) * e_dst + fb + GUARD, SENTINEL, dtype=np.uint8)
    bufs = DevBufs(ctx)
    try:
        s_dev, d_dev = bufs.put(src), bufs.put(dst)
        assert s_dev % 16 == 0 and d_dev % 16 == 0
        ctx.check(ctx._lib.pfv_frames_from_rgb_dev(ctx.handle, w, h, n, P(s_dev + src_off), FORMATS[fmt], pitch, stride, P(d_dev + GUARD + dst_off), dst_stride,
                                                   CHROMAS[chroma]))
        ctx.download(dst, d_dev)
    finally:
        bufs.close()
    rest = dst.copy()
    got = np.zeros((n, fb), np.uint8)
    for k in range(n):
        o = GUARD + dst_off + k * e_dst
        got[k] = dst[o:o + fb]
        rest[o:o + fb] = SENTINEL
    assert (rest == SENTINEL).all(), f"bytes outside the {n} frames were written: {np.flatnonzero(rest != SENTINEL)[:8]}"
    return got


# ------------------------------------------------------------------ 1. shapes
def check_shape(pkg, ctx, w, h, seed=1):
    """random pictures, all three formats x both chroma modes; one stream tight, and three streams with a gap between the source pictures, a
    pitch above the row and a dst_stride above the frame -- all multiples of 16, so that aligned shapes keep the wide path"""
    rng = np.random.default_rng(seed * 1000 + w * 7 + h)
    fb = frame_bytes(w, h)
    for fmt in FORMATS:
        pics = random_pictures(3, w, h, fmt, rng)
        pitch = round_up(w * BPP[fmt], 16) + 16
        for chroma in CHROMAS:
            want = want_frames(pics, fmt, chroma)
            assert w * h < 64 or (want != SENTINEL).any()
            got = ingest_dev(ctx, pics[:1], fmt, chroma, rng=rng)
            assert np.array_equal(got, want[:1]), (w, h, fmt, chroma, "one stream", np.argwhere(got != want[:1])[:4])
            got = ingest_dev(ctx, pics, fmt, chroma, pitch=pitch, stride=pitch * h + 48, dst_stride=round_up(fb, 16) + 32, rng=rng)
            assert np.array_equal(got, want), (w, h, fmt, chroma, "three streams", np.argwhere(got != want)[:4])
            # the host entry point and the Python mirror
            got = pkg.frames_from_rgb(ctx, w, h, pics, fmt, chroma)
            assert got.dtype == np.uint8 and got.shape == (3, fb) and np.array_equal(got, want), (fmt, chroma, "host form")


# ------------------------------------------------------------------ 2. alignment
def check_alignment(pkg, ctx, w, h, seed=3):
    """tight; pitch = row + 5 (unaligned rows); pitch rounded up to 256; source base off by 1 and by 4; destination base off by 1 and by 4;
    dst_stride = frame + 12: two streams, every format and mode, the sentinel intact around every frame"""
    rng = np.random.default_rng(seed * 1000 + w * 7 + h)
    fb = frame_bytes(w, h)
    for fmt in FORMATS:
        pics = random_pictures(2, w, h, fmt, rng)
        row = w * BPP[fmt]
        cases = {"tight": {}, "pitch+5": dict(pitch=row + 5), "pitch256": dict(pitch=round_up(row, 256)), "src+1": dict(src_off=1), "src+4": dict(src_off=4),
                 "dst+1": dict(dst_off=1), "dst+4": dict(dst_off=4), "dst_stride+12": dict(dst_stride=fb + 12),
                 "src+4,pitch256,stride,dst+4": dict(src_off=4, pitch=round_up(row, 256), stride=round_up(row, 256) * h + 20, dst_off=4, dst_stride=fb + 12)}
        for chroma in CHROMAS:
            want = want_frames(pics, fmt, chroma)
            for name, kw in cases.items():
                got = ingest_dev(ctx, pics, fmt, chroma, rng=rng, **kw)
                assert np.array_equal(got, want), (w, h, fmt, chroma, name, np.argwhere(got != want)[:4])


# ------------------------------------------------------------------ 3. POINT equals the old helper
def check_point_equals_helper(pkg, ctx, w, h, seed=5):
    """pfv_frames_from_rgb_dev(RGB8, POINT) == pfv_rgb_to_yuv420_dev on the same picture"""
    rng = np.random.default_rng(seed * 1000 + w * 7 + h)
    pics = random_pictures(1, w, h, "rgb8", rng)
    fb = frame_bytes(w, h)
    bufs = DevBufs(ctx)
    try:
        s_dev, d_dev = bufs.put(pics), bufs.put(np.zeros(fb, np.uint8))
        ctx.check(ctx._lib.pfv_rgb_to_yuv420_dev(ctx.handle, P(s_dev), w, h, P(d_dev)))
        old = np.zeros(fb, np.uint8)
        ctx.download(old, d_dev)
    finally:
        bufs.close()
    got = ingest_dev(ctx, pics, "rgb8", "point", rng=rng)[0]
    assert np.array_equal(got, old), np.flatnonzero(got != old)[:8]
    assert np.array_equal(old, onp.rgb_to_yuv420(pics[0]))


# ------------------------------------------------------------------ 4. exhaustive arithmetic
def exhaustive_base():
    """4096 x 4096 RGBA8: pixel i = y * 4096 + x holds the triple (i >> 16, (i >> 8) & 255, i & 255) and a varying alpha"""
    i = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    return np.stack([(i >> 16).astype(np.uint8), ((i >> 8) & 255).astype(np.uint8), (i & 255).astype(np.uint8), ((i * 37 + (i >> 11)) & 255).astype(np.uint8)], axis=-1)


def exhaustive_picture(k):
    """picture k of four: the base rolled so that its pixel (x, y) = base((x + (k & 1)) mod w, (y + (k >> 1)) mod h)"""
    return np.ascontiguousarray(np.roll(exhaustive_base(), (-(k >> 1), -(k & 1)), axis=(0, 1)))


def check_exhaustive(pkg, ctx, k):
    """picture k at RGBA8 / POINT (a multiple of 8 wide, tight, aligned: the wide path) equals the numpy oracle: Y for all 2^24 triples, and
    U, V for the triples at this picture's even-even positions -- the four pictures' positions cover every triple exactly once (asserted
    here over all four, from the index arithmetic alone).  The oracle runs band by band to bound its float32 temporaries."""
    w = h = 4096
    pic = exhaustive_picture(k)
    triple = lambda p: (p[..., 0].astype(np.int64) << 16) | (p[..., 1].astype(np.int64) << 8) | p[..., 2]      # noqa: E731
    assert (np.bincount(triple(pic).reshape(-1), minlength=1 << 24) == 1).all(), "the picture does not hold every triple once"
    yy, xx = np.meshgrid(np.arange(0, h, 2), np.arange(0, w, 2), indexing="ij")
    seen = np.zeros(1 << 24, np.int64)
    for j in range(4):                                # base index of picture j's pixel (x, y): ((y + (j >> 1)) mod h) * w + (x + (j & 1)) mod w
        seen += np.bincount((((yy + (j >> 1)) % h) * w + (xx + (j & 1)) % w).reshape(-1), minlength=1 << 24)
    assert (seen == 1).all(), "the four pictures' chroma positions do not cover every triple once"
    assert np.array_equal(triple(pic[0::2, 0::2]), ((yy + (k >> 1)) % h) * w + (xx + (k & 1)) % w)
    got = pkg.frames_from_rgb(ctx, w, h, pic, "rgba8", "point")[0]
    n, nc, band = w * h, (w // 2) * (h // 2), 256
    gy, gu, gv = got[:n].reshape(h, w), got[n:n + nc].reshape(h // 2, w // 2), got[n + nc:].reshape(h // 2, w // 2)
    for y0 in range(0, h, band):
        want = onp.rgb_to_yuv420(np.ascontiguousarray(pic[y0:y0 + band, :, :3]))
        m, mc = w * band, (w // 2) * (band // 2)
        assert np.array_equal(gy[y0:y0 + band].reshape(-1), want[:m]), (k, y0, "Y")
        assert np.array_equal(gu[y0 // 2:(y0 + band) // 2].reshape(-1), want[m:m + mc]), (k, y0, "U")
        assert np.array_equal(gv[y0 // 2:(y0 + band) // 2].reshape(-1), want[m + mc:]), (k, y0, "V")


def check_exhaustive_reduced(pkg, ctx):
    """three 512 x 512 pictures: every (R, G) pair with four B values, every (G, B) pair with four R values, every (R, B) pair with four G
    values (asserted), the pair's 2 x 2 pixels holding the third channel's 0, 255 and two values that vary with the pair; all formats and
    both chroma modes"""
    w = h = 512
    p = np.arange(256 * 256, dtype=np.int64).reshape(256, 256)
    hi, lo = (p >> 8).astype(np.uint8), (p & 255).astype(np.uint8)
    third = np.stack([np.zeros_like(p), np.full_like(p, 255), (p * 7 + 13) & 255, (p * 31 + 101) & 255], axis=-1).astype(np.uint8)
    rng = np.random.default_rng(11)
    for free in range(3):                             # the channel that takes the four values
        rgb = np.zeros((h, w, 3), np.uint8)
        pair = [c for c in range(3) if c != free]
        for i, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            rgb[dy::2, dx::2, pair[0]], rgb[dy::2, dx::2, pair[1]], rgb[dy::2, dx::2, free] = hi, lo, third[..., i]
        pairs = (rgb[..., pair[0]].astype(np.int64) << 8) | rgb[..., pair[1]]
        assert (np.bincount(pairs.reshape(-1), minlength=1 << 16) == 4).all(), "the picture does not hold every pair four times"
        for fmt in FORMATS:
            pic = in_format(rgb, fmt, rng)
            for chroma in CHROMAS:
                got = pkg.frames_from_rgb(ctx, w, h, pic, fmt, chroma)[0]
                want = want_frame(pic, fmt, chroma)
                assert np.array_equal(got, want), (free, fmt, chroma, np.flatnonzero(got != want)[:8])


# ------------------------------------------------------------------ 5. encoder session
def synthetic_pictures(pkg, w, h, n, t, fmt, rng, seed):
    """the pictures of frame t of n synthetic streams (so that consecutive t move): yuv420_to_rgb of the oracle, in `fmt`"""
    return np.stack([in_format(onp.yuv420_to_rgb(pkg.SyntheticStream(w, h, seed=seed + k).frame(t), w, h), fmt, rng) for k in range(n)])


class EncBufs:
    """the output buffers of one session's *_dev encode calls, full of a sentinel"""

    def __init__(self, ctx, bufs, n, tb):
        self.ctx, self.n, self.tb = ctx, n, tb
        self.coef, self.mv, self.has = bufs.put(np.full(n * tb * 256, 0x5A5A, np.int16)), bufs.put(np.full(n * tb * 2, 0x5A, np.int8)), bufs.put(np.full(n * tb, SENTINEL, np.uint8))

    def read(self):
        coef, mv, has = np.zeros((self.n, self.tb * 256), np.int16), np.zeros((self.n, self.tb * 2), np.int8), np.zeros((self.n, self.tb), np.uint8)
        self.ctx.download(coef, self.coef)
        self.ctx.download(mv, self.mv)
        self.ctx.download(has, self.has)
        return coef, mv, has


def check_enc_session(pkg, ctx, fmt, chroma, w=144, h=48, quality=5, n=3):
    """I P P of three slots, the window set to slots [1, 3): pfv_enc_ingest_rgb_dev with a pitch and a stride, then the encode calls on the
    returned pointer, against a twin session fed frames_from_rgb's planes through the same window"""
    rng = np.random.default_rng(61)
    L = pkg._lib
    fb = frame_bytes(w, h)
    row = w * BPP[fmt]
    pitch = round_up(row, 16) + 16
    stride = pitch * h + 48
    enc, twin = (pkg.EncoderSession(ctx, w, h, quality, n) for _ in range(2))
    bufs = DevBufs(ctx)
    try:
        tb = enc.total_blocks
        out, tout = EncBufs(ctx, bufs, n, tb), EncBufs(ctx, bufs, n, tb)
        # all slots first, then the window: slot 0's frame in the session's buffer must stay what the first call made it
        first = random_pictures(n, w, h, fmt, rng)
        base = enc.ingest_rgb_dev(bufs.put(lay_out(first, fmt, 0, pitch, stride, rng)), fmt, pitch, stride, chroma)
        for s in (enc, twin):
            s.set_window(1, 2)
        sizes_d, tsizes_d = (bufs.put(np.full(n, 0x5A5A5A5A, np.uint32)) for _ in range(2))
        for t in range(3):
            pics = synthetic_pictures(pkg, w, h, n, t, fmt, rng, seed=61)
            frames = pkg.frames_from_rgb(ctx, w, h, pics, fmt, chroma)
            assert np.array_equal(frames, want_frames(pics, fmt, chroma))
            ptr = enc.ingest_rgb_dev(bufs.put(lay_out(pics, fmt, 0, pitch, stride, rng)), fmt, pitch, stride, chroma)
            assert ptr == base and ptr % 16 == 0, "one buffer, owned by the session"
            held = np.zeros((n, fb), np.uint8)
            ctx.download(held, ptr)
            assert np.array_equal(held[1:], frames[1:]) and np.array_equal(held[0], want_frame(first[0], fmt, chroma)), (t, "the session's frame buffer")
            frames_dev = bufs.put(frames)
            # the probe, before the encode call moves prev_frame
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
            for name, x, y, sent in zip(("coefficients", "motion vectors", "has-coefficient flags"), out.read(), tout.read(), (0x5A5A, 0x5A, SENTINEL)):
                assert np.array_equal(x, y), (t, name)
                assert (x[0] == np.array(sent).astype(x.dtype)).all(), (t, name, "slot 0 was written")
            assert (out.read()[0][1:] != 0x5A5A).any()
            assert np.array_equal(enc.prev_frame(), twin.prev_frame()), (t, "pfv_enc_prev_frame")
            sent = np.full((n, 3), 0x1122334455667788, dtype=np.uint64)
            sse = enc.distortion(int(ptr), out=sent)
            assert np.array_equal(sse, twin.distortion(int(frames_dev), out=sent)) and np.array_equal(sse[0], sent[0]) and sse[1:].sum() > 0, (t, "pfv_enc_distortion_dev")
            ssent = np.full((n, 3), -77, dtype=np.int64)
            q24 = enc.ssim(int(ptr), out=ssent)
            assert np.array_equal(q24, twin.ssim(int(frames_dev), out=ssent)) and np.array_equal(q24[0], ssent[0]) and (q24[1:] != -77).all(), (t, "pfv_enc_ssim_dev")
        # the session's buffer is packed: a frame stride refuses, and its neighbour 0 accepts
        pics_dev = bufs.put(lay_out(pics, fmt, 0, pitch, stride, rng))
        enc.set_frame_stride(fb + 16)
        with pytest.raises(pkg.PfvError) as e:
            enc.ingest_rgb_dev(pics_dev, fmt, pitch, stride, chroma)
        assert e.value.code == L.PFV_ERR_STATE
        enc.set_frame_stride(0)
        assert enc.ingest_rgb_dev(pics_dev, fmt, pitch, stride, chroma) == base
        ctx.sync()
    finally:
        bufs.close()
        enc.close()
        twin.close()


# ------------------------------------------------------------------ 6. graph
def check_enc_graph(pkg, ctx, w=144, h=48, quality=5, n=3, fmt="bgra8", chroma="box"):
    """I P P recorded in one graph with three picture buffers, each step ingest then encode (the first ingest call made before the recording),
    replayed twice: both replays equal a twin session fed the converted planes step by step.  A session whose first ingest call falls inside
    a recording is refused."""
    rng = np.random.default_rng(71)
    enc, twin, late = (pkg.EncoderSession(ctx, w, h, quality, n) for _ in range(3))
    bufs = DevBufs(ctx)
    graph = pkg.Graph(ctx)
    try:
        tb = enc.total_blocks
        steps = [synthetic_pictures(pkg, w, h, n, t, fmt, rng, seed=71) for t in range(3)]
        pics_dev = [bufs.put(p) for p in steps]
        outs, touts = [EncBufs(ctx, bufs, n, tb) for _ in steps], [EncBufs(ctx, bufs, n, tb) for _ in steps]
        want = []
        for t, p in enumerate(steps):
            frames_dev = bufs.put(pkg.frames_from_rgb(ctx, w, h, p, fmt, chroma))
            if t == 0:
                twin.encode_iframe_dev(frames_dev, touts[t].coef)
            else:
                twin.encode_pframe_dev(frames_dev, touts[t].mv, touts[t].has, touts[t].coef)
            want.append(touts[t].read())
        want_prev = twin.prev_frame()
        enc.ingest_rgb_dev(pics_dev[0], fmt, 0, 0, chroma)            # the session's buffer is made here
        with graph:
            for t in range(3):
                ptr = enc.ingest_rgb_dev(pics_dev[t], fmt, 0, 0, chroma)
                if t == 0:
                    enc.encode_iframe_dev(ptr, outs[t].coef)
                else:
                    enc.encode_pframe_dev(ptr, outs[t].mv, outs[t].has, outs[t].coef)
            with pytest.raises(pkg.PfvError) as e:
                late.ingest_rgb_dev(pics_dev[0], fmt, 0, 0, chroma)
            assert e.value.code == pkg._lib.PFV_ERR_STATE and "before" in str(e.value)
        for _ in range(2):
            for o in outs:
                ctx.upload(o.coef, np.full(n * tb * 256, 0x5A5A, np.int16))
            graph.launch()
            for t in range(3):
                got = outs[t].read()
                assert np.array_equal(got[0], want[t][0]), (t, "coefficients")
                assert t == 0 or (np.array_equal(got[1], want[t][1]) and np.array_equal(got[2], want[t][2])), (t, "block headers")
            assert np.array_equal(enc.prev_frame(), want_prev), "pfv_enc_prev_frame"
        ctx.sync()
    finally:
        graph.close()
        bufs.close()
        for s in (enc, twin, late):
            s.close()


# ------------------------------------------------------------------ 7. pfv_encoder
ENCODER_CONFIGS = {
    "plain_device": dict(fmt="rgb8", chroma="point", device_entropy=True, kw=dict(quality=5)),
    "plain_host": dict(fmt="rgba8", chroma="box", device_entropy=False, kw=dict(quality=5)),
    "iframe_budget": dict(fmt="bgra8", chroma="point", device_entropy=True, kw=dict(quality=None, qualities=[2, 5, 8]), budget_i=True),
    "pframe_probe_budget": dict(fmt="rgb8", chroma="box", device_entropy=False, kw=dict(quality=None, qualities=[2, 5, 8]), budget_p=True),
    "quality_floors": dict(fmt="rgba8", chroma="point", device_entropy=True, kw=dict(quality=None, qualities=[2, 5, 8], iframe_quality_floor=36.0, pframe_quality_floor=34.0)),
    "ssim_floors": dict(fmt="bgra8", chroma="box", device_entropy=True, kw=dict(quality=None, qualities=[2, 5, 8], iframe_ssim_floor=0.97, pframe_ssim_floor=0.95)),
    # encode_frame on a clip whose first frame comes twice; behind the first frame (an i-frame at rung 0) the caller moves to the coarsest rung,
    # where the repeated frame codes nothing: a drop frame
    "encode_frame": dict(fmt="rgb8", chroma="point", device_entropy=True, kw=dict(quality=None, qualities=[1, 5, 10]), auto=True, drop=True),
    "encode_frame_host_floor": dict(fmt="rgba8", chroma="box", device_entropy=False, kw=dict(quality=None, qualities=[2, 5, 8], pframe_quality_floor=34.0), auto=True),
}


def check_encoder(pkg, ctx, config, w=48, h=32, n_frames=5):
    """twin encoders, one with set_input_rgb fed pictures, one fed the converted planes: the drained bytes are identical after every call, and
    so are frame reports, frame SSIM and the six probe calls' outputs"""
    cfg = ENCODER_CONFIGS[config]
    fmt, chroma = cfg["fmt"], cfg["chroma"]
    rng = np.random.default_rng(81)
    st = pkg.SyntheticStream(w, h, seed=81)
    order = [0, 0, 1, 2, 3] if cfg.get("auto") else list(range(n_frames))      # encode_frame: a repeated frame, for a drop frame
    pics = [in_format(onp.yuv420_to_rgb(st.frame(t), w, h), fmt, rng) for t in order]
    planes = [pkg.VideoFrame.from_packed(w, h, want_frame(p, fmt, chroma)) for p in pics]
    a_buf, b_buf = io.BytesIO(), io.BytesIO()
    mk = lambda buf: pkg.Encoder(buf, w, h, 30, ctx=ctx, device_entropy=cfg["device_entropy"], frame_report=True, frame_ssim=True, **cfg["kw"])      # noqa: E731
    a, b = mk(a_buf), mk(b_buf)
    try:
        a.set_input_rgb(True, fmt, chroma)
        if cfg.get("budget_i") or cfg.get("budget_p"):
            sizes = b.probe_iframe(planes[0])
            assert sizes[0] > sizes[1] > sizes[2]
            for e in (a, b):
                e.set_iframe_budget(int(sizes[1]))
                if cfg.get("budget_p"):
                    e.set_rate(int(sizes[1]) // 6)
                    e.set_pframe_probe(True)
        types, rungs = [], []
        for t, (pic, fr) in enumerate(zip(pics, planes)):
            if t > 0:                                 # the six probe calls: the same answers, nothing moved
                for name in ("probe_iframe", "probe_iframe_rd", "probe_iframe_ssim", "probe_pframe", "probe_pframe_rd", "probe_pframe_ssim"):
                    x, y = getattr(a, name)(pic), getattr(b, name)(fr)
                    x, y = (x, y) if isinstance(x, tuple) else ((x,), (y,))
                    assert len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y)), (config, t, name, x, y)
            if t == 1 and cfg.get("drop"):
                a.set_rung(2)
                b.set_rung(2)
            if cfg.get("auto"):
                ta, tb = a.encode_frame(pic), b.encode_frame(fr)
                assert ta == tb, (config, t, ta, tb)
                types.append(tb)
            elif t in (0, 3):
                a.encode_iframe(pic)
                b.encode_iframe(fr)
            else:
                a.encode_pframe(pic)
                b.encode_pframe(fr)
            assert a_buf.getvalue() == b_buf.getvalue(), (config, t, "stream bytes")
            assert a.rung == b.rung and a.last_report == b.last_report and a.last_ssim == b.last_ssim, (config, t, a.last_report, b.last_report)
            rungs.append(b.rung)
        if cfg.get("auto"):
            assert types[0] == 1 and len(set(types)) > 1 and (not cfg.get("drop") or (2 in types and 3 in types)), (config, types)      # of the TWIN: the check is not empty
        if config == "plain_device":
            # a plane beside the picture is refused, by every call that takes (y, u, v); the neighbour (NULL, NULL) has just been accepted
            lib, L = ctx._lib, pkg._lib
            hp = lambda x: x.ctypes.data_as(P)      # noqa: E731
            pic, junk = np.ascontiguousarray(pics[1]), np.zeros(w * h, np.uint8)
            sizes, sse, q24 = np.zeros(1, np.uint32), np.zeros(3, np.uint64), np.zeros(3, np.int64)
            for u, v in ((hp(junk), None), (None, hp(junk)), (hp(junk), hp(junk))):
                assert lib.pfv_encoder_encode_iframe(a.handle, hp(pic), u, v) == L.PFV_ERR_BAD_ARG
                assert lib.pfv_encoder_encode_pframe(a.handle, hp(pic), u, v) == L.PFV_ERR_BAD_ARG
                assert lib.pfv_encoder_encode_frame(a.handle, hp(pic), u, v, None) == L.PFV_ERR_BAD_ARG
                assert lib.pfv_encoder_probe_iframe(a.handle, hp(pic), u, v, hp(sizes)) == L.PFV_ERR_BAD_ARG
                assert lib.pfv_encoder_probe_pframe(a.handle, hp(pic), u, v, hp(sizes)) == L.PFV_ERR_BAD_ARG
                assert lib.pfv_encoder_probe_iframe_rd(a.handle, hp(pic), u, v, hp(sizes), hp(sse)) == L.PFV_ERR_BAD_ARG
                assert lib.pfv_encoder_probe_pframe_rd(a.handle, hp(pic), u, v, hp(sizes), hp(sse)) == L.PFV_ERR_BAD_ARG
                assert lib.pfv_encoder_probe_iframe_ssim(a.handle, hp(pic), u, v, hp(sizes), hp(sse), hp(q24)) == L.PFV_ERR_BAD_ARG
                assert lib.pfv_encoder_probe_pframe_ssim(a.handle, hp(pic), u, v, hp(sizes), hp(sse), hp(q24)) == L.PFV_ERR_BAD_ARG
            assert lib.pfv_encoder_encode_iframe(a.handle, None, None, None) == L.PFV_ERR_BAD_ARG
            assert a_buf.getvalue() == b_buf.getvalue(), "a refused call wrote something"
        # switched off again, the planar calls give the bytes they give on the twin
        a.set_input_rgb(False)
        for e in (a, b):
            e.encode_iframe(planes[1])
            e.encode_pframe(planes[2])
            e.finish()
        assert a_buf.getvalue() == b_buf.getvalue(), (config, "after set_input_rgb(off)")
        if "qualities" not in cfg["kw"]:              # ... and on a fresh encoder (one rung: no rate state to carry over)
            c_buf = io.BytesIO()
            c = mk(c_buf)
            try:
                head = len(c_buf.getvalue())
                c.encode_iframe(planes[1])
                c.encode_pframe(planes[2])
                c.finish()
            finally:
                c.close()
            tail = c_buf.getvalue()[head:]
            assert a_buf.getvalue()[-len(tail):] == tail, (config, "a fresh encoder")
    finally:
        a.close()
        b.close()
    return rungs


# ------------------------------------------------------------------ 8. end to end against the oracle alone
def check_end_to_end(pkg, ctx, oracle, fmt, w=48, h=32, quality=5, plan=("I", "P", "P", "I", "P")):
    """pictures -> Encoder with RGB input -> .pfv bytes -> Decoder with RGB output, against rgb_to_yuv420 -> the oracle's encoder -> the
    oracle's decoder -> yuv420_to_rgb: bytes and pictures are equal (POINT)"""
    rng = np.random.default_rng(91)
    st = pkg.SyntheticStream(w, h, seed=91)
    rgbs = [onp.yuv420_to_rgb(st.frame(t), w, h) for t in range(len(plan))]
    pics = [in_format(r, fmt, rng) for r in rgbs]                       # BGRA8: the test reverses the channels and adds an alpha
    want_data = dc.oracle_clip(pkg, oracle, w, h, quality, [onp.rgb_to_yuv420(r) for r in rgbs], list(plan))
    want_rgb = [onp.yuv420_to_rgb(f, w, h) for f in qc.oracle_decode(oracle, want_data)]
    buf = io.BytesIO()
    enc = pkg.Encoder(buf, w, h, 30, quality, ctx)
    try:
        enc.set_input_rgb(True, fmt, "point")
        for kind, pic in zip(plan, pics):
            (enc.encode_iframe if kind == "I" else enc.encode_pframe)(pic)
        enc.finish()
    finally:
        enc.close()
    assert buf.getvalue() == want_data, "the stream differs from the oracle encoder's"
    dec = pkg.Decoder(buf.getvalue(), ctx)
    got = []
    try:
        dec.set_output_rgb(True, fmt)
        while dec.advance_frame(got.append):
            pass
    finally:
        dec.close()
    assert len(got) == len(want_rgb) == len(plan)
    for t, (g, r) in enumerate(zip(got, want_rgb)):
        assert np.array_equal(rgb_of(g, fmt), r), (fmt, t)
        assert fmt == "rgb8" or (g[..., 3] == 255).all()


# ------------------------------------------------------------------ 9. bad arguments
def check_bad_arguments(pkg, ctx):
    L = pkg._lib
    lib = ctx._lib
    w, h = 16, 16
    fb, pic = frame_bytes(w, h), 64 * h
    bufs = DevBufs(ctx)
    try:
        a = bufs.put(np.zeros(8 * w * h * 4, dtype=np.uint8))
        d = bufs.put(np.zeros(8 * w * h * 4, dtype=np.uint8))

        def call(w=w, h=h, n=1, src=a, fmt=1, pitch=0, stride=0, dst=d, ds=0, chroma=0, ctx_h=ctx.handle):
            return lib.pfv_frames_from_rgb_dev(ctx_h, w, h, n, P(src) if src else None, fmt, pitch, stride, P(dst) if dst else None, ds, chroma)
        assert call() == L.PFV_OK and call(n=2, chroma=1) == L.PFV_OK and call(fmt=0) == L.PFV_OK and call(fmt=2) == L.PFV_OK
        for bad in ((15, 16), (16, 17), (0, 16), (16, -2), (65536, 16), (129, 17)):          # dimensions a frame cannot have
            assert call(w=bad[0], h=bad[1]) == L.PFV_ERR_BAD_ARG, bad
        assert call(n=0) == L.PFV_ERR_BAD_ARG and call(n=-1) == L.PFV_ERR_BAD_ARG
        assert call(fmt=3) == L.PFV_ERR_BAD_ARG and call(fmt=-1) == L.PFV_ERR_BAD_ARG
        assert call(chroma=2) == L.PFV_ERR_BAD_ARG and call(chroma=-1) == L.PFV_ERR_BAD_ARG and call(chroma=1) == L.PFV_OK
        assert call(src=None) == L.PFV_ERR_BAD_ARG and call(dst=None) == L.PFV_ERR_BAD_ARG and call(ctx_h=None) == L.PFV_ERR_BAD_ARG
        assert call(pitch=63) == L.PFV_ERR_BAD_ARG and call(pitch=64) == L.PFV_OK and call(fmt=0, pitch=47) == L.PFV_ERR_BAD_ARG and call(fmt=0, pitch=48) == L.PFV_OK
        assert call(n=2, stride=pic - 1) == L.PFV_ERR_BAD_ARG and call(n=2, stride=pic) == L.PFV_OK
        assert call(n=2, pitch=80, stride=pic) == L.PFV_ERR_BAD_ARG and call(n=2, pitch=80, stride=80 * h) == L.PFV_OK
        assert call(n=2, ds=fb - 1) == L.PFV_ERR_BAD_ARG and call(n=2, ds=fb) == L.PFV_OK
        # overlapping ranges, either way round; the source runs from the first picture to the end of the last row of the last one
        assert call(dst=a) == L.PFV_ERR_BAD_ARG
        assert call(dst=a + pic - 1) == L.PFV_ERR_BAD_ARG and call(dst=a + pic) == L.PFV_OK
        assert call(src=a + fb - 1, dst=a) == L.PFV_ERR_BAD_ARG and call(src=a + fb, dst=a) == L.PFV_OK
        assert call(dst=a + 80 * (h - 1) + 63, pitch=80) == L.PFV_ERR_BAD_ARG and call(dst=a + 80 * (h - 1) + 64, pitch=80) == L.PFV_OK
        assert call(n=2, src=a, dst=a + pic, stride=2 * pic) == L.PFV_ERR_BAD_ARG            # the destination lies in the gap between the pictures
        assert call(n=2, src=a + fb, dst=a, ds=fb + pic + 64) == L.PFV_ERR_BAD_ARG            # the source lies in the gap between the frames
        # the host form
        host, out = np.zeros(w * h * 4, np.uint8), np.zeros(fb, np.uint8)
        hp = lambda x: x.ctypes.data_as(P)      # noqa: E731
        assert lib.pfv_frames_from_rgb(ctx.handle, w, h, 1, hp(host), hp(out), 1, 0) == L.PFV_OK
        assert lib.pfv_frames_from_rgb(ctx.handle, 15, h, 1, hp(host), hp(out), 1, 0) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_from_rgb(ctx.handle, w, h, 0, hp(host), hp(out), 1, 0) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_from_rgb(ctx.handle, w, h, 1, None, hp(out), 1, 0) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_from_rgb(ctx.handle, w, h, 1, hp(host), None, 1, 0) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_from_rgb(ctx.handle, w, h, 1, hp(host), hp(out), 3, 0) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_from_rgb(ctx.handle, w, h, 1, hp(host), hp(out), 1, 2) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_from_rgb(ctx.handle, w, h, 1, hp(host), hp(out), 1, 1) == L.PFV_OK
        assert lib.pfv_frames_from_rgb(None, w, h, 1, hp(host), hp(out), 1, 0) == L.PFV_ERR_BAD_ARG
        # the session's call and the encoder's switch
        got = P()
        ref = ctypes.byref(got)
        assert lib.pfv_enc_ingest_rgb_dev(None, P(a), 1, 0, 0, 0, ref) == L.PFV_ERR_BAD_ARG and lib.pfv_encoder_set_input_rgb(None, 1, 1, 0) == L.PFV_ERR_BAD_ARG
        enc, late = (pkg.EncoderSession(ctx, w, h, 5, 2) for _ in range(2))
        graph = pkg.Graph(ctx)
        try:
            fn = lib.pfv_enc_ingest_rgb_dev
            assert fn(enc.handle, P(a), 1, 0, 0, 0, ref) == L.PFV_OK and got.value and fn(enc.handle, P(a), 0, 48, 48 * h, 1, ref) == L.PFV_OK
            assert fn(enc.handle, None, 1, 0, 0, 0, ref) == L.PFV_ERR_BAD_ARG and fn(enc.handle, P(a), 1, 0, 0, 0, None) == L.PFV_ERR_BAD_ARG
            assert fn(enc.handle, P(a), 3, 0, 0, 0, ref) == L.PFV_ERR_BAD_ARG and fn(enc.handle, P(a), -1, 0, 0, 0, ref) == L.PFV_ERR_BAD_ARG
            assert fn(enc.handle, P(a), 1, 0, 0, 2, ref) == L.PFV_ERR_BAD_ARG and fn(enc.handle, P(a), 1, 0, 0, -1, ref) == L.PFV_ERR_BAD_ARG
            assert fn(enc.handle, P(a), 1, 63, 0, 0, ref) == L.PFV_ERR_BAD_ARG and fn(enc.handle, P(a), 1, 64, 0, 0, ref) == L.PFV_OK
            assert fn(enc.handle, P(a), 1, 80, 80 * h - 1, 0, ref) == L.PFV_ERR_BAD_ARG and fn(enc.handle, P(a), 1, 80, 80 * h, 0, ref) == L.PFV_OK
            enc.set_frame_stride(fb)                  # the smallest non-zero stride there is
            assert fn(enc.handle, P(a), 1, 0, 0, 0, ref) == L.PFV_ERR_STATE
            enc.set_frame_stride(0)
            assert fn(enc.handle, P(a), 1, 0, 0, 0, ref) == L.PFV_OK
            # while a graph is being recorded: the host form refuses, the device forms are recorded, a first session call refuses
            with graph:
                assert lib.pfv_frames_from_rgb(ctx.handle, w, h, 1, hp(host), hp(out), 1, 0) == L.PFV_ERR_STATE
                assert call() == L.PFV_OK and fn(enc.handle, P(a), 1, 0, 0, 0, ref) == L.PFV_OK
                assert fn(late.handle, P(a), 1, 0, 0, 0, ref) == L.PFV_ERR_STATE
            assert fn(late.handle, P(a), 1, 0, 0, 0, ref) == L.PFV_OK
        finally:
            graph.close()
            enc.close()
            late.close()
        se = pkg.Encoder(io.BytesIO(), w, h, 30, 5, ctx)
        try:
            fn = lib.pfv_encoder_set_input_rgb
            assert fn(se.handle, 1, 3, 0) == L.PFV_ERR_BAD_ARG and fn(se.handle, 1, -1, 0) == L.PFV_ERR_BAD_ARG
            assert fn(se.handle, 1, 2, 2) == L.PFV_ERR_BAD_ARG and fn(se.handle, 1, 2, -1) == L.PFV_ERR_BAD_ARG
            assert fn(se.handle, 1, 2, 1) == L.PFV_OK and fn(se.handle, 0, 9, 9) == L.PFV_OK          # off: whatever the rest says
            with pytest.raises(pkg.PfvError):
                se.set_input_rgb(True, 5)
            with pytest.raises(NotImplementedError):
                pkg.GopEncoder.set_input_rgb(None)
            # the encoder's finished rule is unchanged under the switch
            se.set_input_rgb(True, "rgba8")
            se.finish()
            assert lib.pfv_encoder_encode_iframe(se.handle, hp(host), None, None) == L.PFV_ERR_STATE
        finally:
            se.close()
        ctx.sync()
    finally:
        bufs.close()


# ------------------------------------------------------------------ 10. C++ mirror and tool
def build_cpp(lib_path, exe):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "ingest_report.cpp"), "-o", exe, lib_path, "-Wl,-rpath," + os.path.dirname(lib_path)], check=True)


def check_cpp(pkg, ctx, exe, tmp_path, w=48, h=32, quality=5, n=4):
    """tests/cpp/ingest_report.cpp (pfv::frames_from_rgb, pfv::Encoder::set_input_rgb) writes the frames and the .pfv the Python mirror makes"""
    rng = np.random.default_rng(101)
    st = pkg.SyntheticStream(w, h, seed=101)
    for fmt, chroma in (("rgb8", "point"), ("rgba8", "box"), ("bgra8", "point")):
        pics = np.stack([in_format(onp.yuv420_to_rgb(st.frame(t), w, h), fmt, rng) for t in range(n)])
        src, o1, o2 = str(tmp_path / f"{fmt}_pictures.bin"), str(tmp_path / f"{fmt}_frames.bin"), str(tmp_path / f"{fmt}.pfv")
        pics.tofile(src)
        r = subprocess.run([exe, str(w), str(h), str(FORMATS[fmt]), str(CHROMAS[chroma]), str(quality), src, o1, o2], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert r.stdout.splitlines() == [f"pictures {n} of {w}x{h} picture bytes {w * h * BPP[fmt]} frame bytes {frame_bytes(w, h)}"]
        want = pkg.frames_from_rgb(ctx, w, h, pics, fmt, chroma)
        assert np.array_equal(want, want_frames(pics, fmt, chroma))
        assert np.array_equal(np.fromfile(o1, dtype=np.uint8).reshape(want.shape), want), (fmt, chroma, "frames")
        buf = io.BytesIO()
        enc = pkg.Encoder(buf, w, h, 30, quality, ctx)
        try:
            enc.set_input_rgb(True, fmt, chroma)
            for t in range(n):
                (enc.encode_pframe if t else enc.encode_iframe)(pics[t])
            enc.finish()
        finally:
            enc.close()
        assert open(o2, "rb").read() == buf.getvalue(), (fmt, chroma, ".pfv")


def check_rd_tool(pkg, lib_path, w=64, h=48):
    """tools/rd_curve.py --time-ingest on the library at lib_path prints its rows: per shape one line per format and chroma mode with the
    three ways' milliseconds and rates"""
    env = dict(os.environ)
    env["PFV_HIP_LIB"] = lib_path
    cmd = [sys.executable, os.path.join(ROOT, "tools", "rd_curve.py"), str(w), str(h), "1", "--qualities", "", "--time-ingest"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr
    rows = [json.loads(x)["time_ingest"] for x in r.stdout.splitlines()]
    assert [(x["format"], x["chroma"]) for x in rows] == [(f, c) for f in FORMATS for c in CHROMAS] and all(x["shape"] == f"1 x {w}x{h}" for x in rows)
    fb = frame_bytes(w, h)
    for x in rows:
        for key in ("a_ingest_ms", "b_per_stream_ms", "c_present_ms"):
            assert x[key] >= 0, (key, x)
        assert "a_over_b_time" in x and "a_rate_over_c_rate" in x      # ratios of times: None on a device without a clock (the emulator)
        assert x["bytes"] == {"a_ingest": w * h * BPP[x["format"]] + fb, "b_per_stream": w * h * 3 + fb, "c_present": fb + w * h * BPP[x["format"]]}
        assert set(x["GBps"]) == {"a_ingest", "b_per_stream", "c_present"}
    return rows
