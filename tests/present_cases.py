"""Shared checks of the RGB / RGBA texture output (include/pfv_hip_ext.h, "RGB / RGBA texture output"; k_present_rgb), driven on the CPU
emulator by tests/test_emu_present.py and on a real MI355X by tests/test_gpu_present.py through the same fixtures.

The reference is `yuv420_to_rgb` of oracle/pfv_oracle_np.py (the reference's save_frame in numpy float32); `to_rgb` below permutes its
channels and adds the alpha byte.  Every comparison is EQUALITY.  Destinations are filled with a sentinel first, and every byte outside the
pictures' rows -- pitch padding, gaps between pictures, 64 guard bytes on either side -- must still hold it afterwards.  A picture byte that is
not written keeps the sentinel too and so differs from the oracle's value (the random pictures are not the sentinel everywhere)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import deblock_cases as dc
import quality_cases as qc
from golden_recompute import onp
from quality_cases import PACKED, PADDED, DevBufs, frame_bytes, padded_frame_bytes, to_padded

ROOT = qc.ROOT
FORMATS = {"rgb8": 0, "rgba8": 1, "bgra8": 2}
BPP = {"rgb8": 3, "rgba8": 4, "bgra8": 4}
# 2x2 one chroma sample; 6x4 no full lane group; 18x18 crosses a 16-pixel segment and a macroblock; 34x130 / 130x34 ragged, more than one
# workgroup of groups; 144x48 two strips wide, three macroblock rows; 256x16 exactly aligned, the wide path throughout
SHAPES = [(2, 2), (6, 4), (18, 18), (34, 130), (130, 34), (144, 48), (256, 16)]
SENTINEL = 0xA5
GUARD = 64
P = ctypes.c_void_p


def to_rgb(frame, w, h, fmt):
    """one packed frame -> the picture [h, w, 3 or 4] in `fmt`, from the numpy oracle"""
    rgb = onp.yuv420_to_rgb(np.ascontiguousarray(frame, dtype=np.uint8).reshape(-1), w, h)
    if fmt == "rgb8":
        return rgb
    alpha = np.full((h, w, 1), 255, np.uint8)
    return np.concatenate([rgb if fmt == "rgba8" else rgb[..., ::-1], alpha], axis=-1)


def to_rgb_many(frames, w, h, fmt):
    return np.stack([to_rgb(f, w, h, fmt) for f in frames])


def round_up(x, n):
    return (x + n - 1) // n * n


def read_pictures(raw, at, n, w, h, fmt, pitch, stride):
    """the n pictures that start `at` bytes into `raw`, and `raw` with their rows put back to the sentinel"""
    row = w * BPP[fmt]
    rest = raw.copy()
    got = np.zeros((n, h, row), np.uint8)
    for k in range(n):
        for y in range(h):
            o = at + k * stride + y * pitch
            got[k, y] = raw[o:o + row]
            rest[o:o + row] = SENTINEL
    return got.reshape(n, h, w, BPP[fmt]), rest


def present_dev(ctx, w, h, frames, layout, fmt, src_off=0, src_gap=0, dst_off=0, pitch=0, stride=0, rng=None):
    """pfv_frames_to_rgb_dev on `frames` ([n, frame bytes of the layout]) -> the n pictures.  The source lies src_off bytes into its allocation
    with src_gap random bytes between frames; the destination lies GUARD + dst_off bytes into an allocation full of the sentinel, which is
    asserted to survive everywhere outside the pictures' rows."""
    frames = np.atleast_2d(frames)
    n, sfb = frames.shape
    rng = rng or np.random.default_rng(7)
    s_stride = sfb + src_gap
    src = rng.integers(0, 256, src_off + n * s_stride + 16, dtype=np.uint8)
    for k in range(n):
        src[src_off + k * s_stride: src_off + k * s_stride + sfb] = frames[k]
    row = w * BPP[fmt]
    e_pitch = pitch or row
    e_stride = stride or e_pitch * h
    dst = np.full(GUARD + dst_off + (n - 1) * e_stride + h * e_pitch + GUARD, SENTINEL, dtype=np.uint8)
    bufs = DevBufs(ctx)
    try:
        s_dev, d_dev = bufs.put(src), bufs.put(dst)
        assert s_dev % 16 == 0 and d_dev % 16 == 0
        ctx.check(ctx._lib.pfv_frames_to_rgb_dev(ctx.handle, w, h, n, P(s_dev + src_off), layout, s_stride if src_gap else 0, P(d_dev + GUARD + dst_off),
                                                 FORMATS[fmt], pitch, stride))
        ctx.download(dst, d_dev)
    finally:
        bufs.close()
    got, rest = read_pictures(dst, GUARD + dst_off, n, w, h, fmt, e_pitch, e_stride)
    assert (rest == SENTINEL).all(), f"bytes outside the {n} pictures' rows were written: {np.flatnonzero(rest != SENTINEL)[:8]}"
    return got


def random_forms(w, h, n, rng):
    a = rng.integers(0, 256, (n, frame_bytes(w, h)), dtype=np.uint8)
    forms = {PACKED: a, PADDED: np.stack([to_padded(x, w, h, rng) for x in a])}
    assert forms[PADDED].shape[1] == padded_frame_bytes(w, h)
    return a, forms


# ------------------------------------------------------------------ 1. shapes
def check_shape(pkg, ctx, w, h, seed=1):
    """random frames, all three formats, PACKED and PADDED (random padding) sources; one stream tight, and three streams with a gap between the
    source frames, a pitch above the row and a stride above the picture -- all multiples of 16, so that aligned shapes keep the wide path"""
    rng = np.random.default_rng(seed * 1000 + w * 7 + h)
    a, forms = random_forms(w, h, 3, rng)
    for fmt in FORMATS:
        want = to_rgb_many(a, w, h, fmt)
        assert w * h < 64 or (want != SENTINEL).any()
        row = w * BPP[fmt]
        pitch = round_up(row, 16) + 16
        for layout in (PACKED, PADDED):
            got = present_dev(ctx, w, h, forms[layout][:1], layout, fmt, rng=rng)
            assert np.array_equal(got, want[:1]), (w, h, fmt, layout, "one stream", np.argwhere(got != want[:1])[:4])
            got = present_dev(ctx, w, h, forms[layout], layout, fmt, src_gap=48, pitch=pitch, stride=pitch * h + 32, rng=rng)
            assert np.array_equal(got, want), (w, h, fmt, layout, "three streams", np.argwhere(got != want)[:4])
    # the host entry point and the Python mirror
    for fmt in FORMATS:
        got = pkg.frames_to_rgb(ctx, w, h, a, fmt)
        assert got.dtype == np.uint8 and got.shape == (3, h, w, BPP[fmt]) and np.array_equal(got, to_rgb_many(a, w, h, fmt)), fmt


# ------------------------------------------------------------------ 2. alignment and pitch
def check_alignment(pkg, ctx, w, h, seed=3):
    """tight pitch; pitch = tight + 5 (unaligned rows); pitch rounded up to 256; destination base off by 1 and by 4 bytes; source base off by 1:
    two streams, every format and layout, the sentinel intact around every row"""
    rng = np.random.default_rng(seed * 1000 + w * 7 + h)
    a, forms = random_forms(w, h, 2, rng)
    for fmt in FORMATS:
        want = to_rgb_many(a, w, h, fmt)
        row = w * BPP[fmt]
        cases = {"tight": {}, "pitch+5": dict(pitch=row + 5), "pitch256": dict(pitch=round_up(row, 256)), "dst+1": dict(dst_off=1), "dst+4": dict(dst_off=4),
                 "src+1": dict(src_off=1), "dst+4,pitch256,stride": dict(dst_off=4, pitch=round_up(row, 256), stride=round_up(row, 256) * h + 12)}
        for layout in (PACKED, PADDED):
            for name, kw in cases.items():
                got = present_dev(ctx, w, h, forms[layout], layout, fmt, rng=rng, **kw)
                assert np.array_equal(got, want), (w, h, fmt, layout, name, np.argwhere(got != want)[:4])


# ------------------------------------------------------------------ 3. exhaustive arithmetic
def exhaustive_frame(full):
    """full: 4096 x 4096, every (Y, U, V) triple exactly once -- chroma pair p = U * 256 + V owns 64 consecutive chroma samples, sample k of them
    the luma values 4k .. 4k + 3.  Else 512 x 512: every chroma pair once, with the luma values 0, 255 and two that vary with the pair."""
    if full:
        w = h = 4096
        s = np.arange((w // 2) * (h // 2), dtype=np.int64).reshape(h // 2, w // 2)
        p, k = s // 64, s % 64
        quad = np.stack([4 * k, 4 * k + 1, 4 * k + 2, 4 * k + 3], axis=-1)
    else:
        w = h = 512
        p = np.arange((w // 2) * (h // 2), dtype=np.int64).reshape(h // 2, w // 2)
        quad = np.stack([np.zeros_like(p), np.full_like(p, 255), (p * 7 + 13) & 255, (p * 31 + 101) & 255], axis=-1)
    luma = np.zeros((h, w), np.uint8)
    luma[0::2, 0::2], luma[0::2, 1::2], luma[1::2, 0::2], luma[1::2, 1::2] = (quad[..., i] for i in range(4))
    return w, h, np.concatenate([luma.reshape(-1), (p >> 8).astype(np.uint8).reshape(-1), (p & 255).astype(np.uint8).reshape(-1)])


def check_exhaustive(pkg, ctx, full):
    """RGBA8 of the exhaustive frame (a width that is a multiple of 8: the wide path) equals the numpy oracle: truncation, saturation and
    the absence of contraction for every triple.  The oracle runs band by band to bound its float32 temporaries."""
    w, h, frame = exhaustive_frame(full)
    if full:
        triples = (frame[:w * h].reshape(h // 2, 2, w // 2, 2).astype(np.int64) << 16) + (frame[w * h:w * h + w * h // 4].reshape(h // 2, 1, w // 2, 1).astype(np.int64) << 8) \
            + frame[w * h + w * h // 4:].reshape(h // 2, 1, w // 2, 1)
        assert (np.bincount(triples.reshape(-1), minlength=1 << 24) == 1).all(), "the frame does not hold every triple once"
    got = pkg.frames_to_rgb(ctx, w, h, frame, "rgba8")[0]
    assert (got[..., 3] == 255).all()
    y, u, v = frame[:w * h].reshape(h, w), frame[w * h:w * h + w * h // 4].reshape(h // 2, w // 2), frame[w * h + w * h // 4:].reshape(h // 2, w // 2)
    band = 256
    for y0 in range(0, h, band):
        sub = np.concatenate([y[y0:y0 + band].reshape(-1), u[y0 // 2:(y0 + band) // 2].reshape(-1), v[y0 // 2:(y0 + band) // 2].reshape(-1)])
        want = onp.yuv420_to_rgb(sub, w, band)
        part = got[y0:y0 + band, :, :3]
        assert np.array_equal(part, want), (y0, np.argwhere(part != want)[:4])


# ------------------------------------------------------------------ 4. decoder session
def session_steps(pkg, oracle, w, h, quality, n, seed):
    """I P P of n synthetic streams through the oracle's encoders: per step the arrays a decode call takes"""
    streams = [pkg.SyntheticStream(w, h, seed=seed + k) for k in range(n)]
    oenc = [oracle.encoder(w, h, quality) for _ in range(n)]
    steps = []
    for t in range(3):
        frames = np.stack([s.frame(t) for s in streams])
        if t == 0:
            steps.append((np.stack([o.encode_iframe(f) for o, f in zip(oenc, frames)]),))
        else:
            parts = [o.encode_pframe(f) for o, f in zip(oenc, frames)]
            steps.append(tuple(np.stack([p[i] for p in parts]) for i in range(3)))
    return steps


def decode_step(dec, bufs, step):
    if len(step) == 1:
        dec.decode_iframe_dev(bufs.put(step[0]))
    else:
        dec.decode_pframe_dev(*(bufs.put(x) for x in step))
        dec.check()


def check_dec_session(pkg, ctx, oracle, deblock, planar, fmt, w=144, h=48, quality=5, n=3):
    """I P P, three slots, the window set to slots [1, 3), the RGB output with a pitch and a stride, `planar`: a strided planar output beside
    it, `deblock`: "off" / "auto" / "fixed".  After every decode call pfv_dec_get_frame_rgb, pfv_dec_get_frame_rgb_dev and the window's
    pictures in the set output equal to_rgb(pfv_dec_get_frame); slot 0's picture and every gap keep the sentinel.  A twin session without the
    RGB output sees the same calls: framebuffer, pfv_dec_get_frame and the planar output are bit-identical."""
    tabs = np.stack(oracle.qtables(quality)[:4])
    steps = session_steps(pkg, oracle, w, h, quality, n, seed=81)
    fb = frame_bytes(w, h)
    row = w * BPP[fmt]
    pitch = round_up(row, 16) + 16
    stride = pitch * h + 48
    p_stride = dc.odd_stride(fb)
    fixed = (3, 0, 9)
    dec, twin = (pkg.DecoderSession(ctx, w, h, tabs, n) for _ in range(2))
    bufs = DevBufs(ctx)
    try:
        rgb_dev = bufs.put(np.full(GUARD + n * stride + GUARD, SENTINEL, np.uint8))
        for d in (dec, twin):
            d.set_window(1, 2)
            d.set_deblock(deblock, fixed if deblock == "fixed" else None)
        outs = {}
        if planar:
            for d in (dec, twin):
                outs[d] = bufs.put(np.full(n * p_stride + 64, SENTINEL, np.uint8))
                d.set_output_strided_dev(outs[d], p_stride)
        dec.set_output_rgb_dev(rgb_dev + GUARD, fmt, pitch, stride)
        filtered = False
        for t, step in enumerate(steps):
            decode_step(dec, bufs, step)
            decode_step(twin, bufs, step)
            frames = dec.get_frame()
            assert np.array_equal(frames, twin.get_frame()) and np.array_equal(dec.framebuffer(), twin.framebuffer()), (t, "the RGB output changed the session")
            if deblock != "off":
                twin.set_deblock("off")
                filtered = filtered or not np.array_equal(twin.get_frame(), frames)
                twin.set_deblock(deblock, fixed if deblock == "fixed" else None)
            if planar:
                raw = [np.zeros(n * p_stride + 64, np.uint8) for _ in range(2)]
                ctx.download(raw[0], outs[dec])
                ctx.download(raw[1], outs[twin])
                assert np.array_equal(raw[0], raw[1]), (t, "planar output")
                for k in (1, 2):
                    assert np.array_equal(raw[0][k * p_stride:k * p_stride + fb], frames[k]), (t, k, "planar output")
            want = to_rgb_many(frames, w, h, fmt)
            got = dec.get_frame_rgb(fmt)
            assert np.array_equal(got, want), (t, "pfv_dec_get_frame_rgb", np.argwhere(got != want)[:4])
            tmp = bufs.put(np.full(GUARD + n * stride + GUARD, SENTINEL, np.uint8))
            dec.get_frame_rgb_dev(tmp + GUARD, fmt, pitch, stride)
            raw = np.zeros(GUARD + n * stride + GUARD, np.uint8)
            ctx.download(raw, tmp)
            got, rest = read_pictures(raw, GUARD, n, w, h, fmt, pitch, stride)
            assert np.array_equal(got, want) and (rest == SENTINEL).all(), (t, "pfv_dec_get_frame_rgb_dev")
            ctx.download(raw, rgb_dev)
            got, rest = read_pictures(raw, GUARD + stride, 2, w, h, fmt, pitch, stride)     # the window's slots; slot 0 must keep the sentinel
            assert np.array_equal(got, want[1:]), (t, "set output", np.argwhere(got != want[1:])[:4])
            assert (rest == SENTINEL).all(), (t, "set output: bytes outside the window's pictures were written")
        assert deblock == "off" or filtered, "the filter changes nothing here: the check would be empty"
        # switched off again, a decode call leaves the buffer alone
        dec.set_output_rgb_dev(None)
        ctx.upload(rgb_dev, np.full(GUARD + n * stride + GUARD, SENTINEL, np.uint8))
        decode_step(dec, bufs, steps[2])
        raw = np.zeros(GUARD + n * stride + GUARD, np.uint8)
        ctx.download(raw, rgb_dev)
        assert (raw == SENTINEL).all()
    finally:
        bufs.close()
        dec.close()
        twin.close()


def check_dec_forms(pkg, ctx, oracle, w=144, h=48, quality=5, n=3):
    """the host, sparse and lists forms of the decode calls write the set output too (full window, tight RGBA)"""
    tabs = np.stack(oracle.qtables(quality)[:4])
    steps = session_steps(pkg, oracle, w, h, quality, n, seed=85)
    size = n * h * w * 4
    dec = pkg.DecoderSession(ctx, w, h, tabs, n)
    bufs = DevBufs(ctx)
    try:
        rgb_dev = bufs.put(np.zeros(size, np.uint8))
        dec.set_output_rgb_dev(rgb_dev, "rgba8")

        def shown(what):
            raw = np.zeros(size, np.uint8)
            ctx.download(raw, rgb_dev)
            ctx.upload(rgb_dev, np.full(size, SENTINEL, np.uint8))
            assert np.array_equal(raw.reshape(n, h, w, 4), to_rgb_many(dec.get_frame(), w, h, "rgba8")), what
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


def check_dec_graph(pkg, ctx, oracle, w=144, h=48, quality=5, n=3, fmt="bgra8"):
    """I P P with deblocking AUTO and no planar output (the filtered picture passes through the session's scratch, allocated by the set
    calls before the recording) recorded in one graph with three RGB outputs and replayed twice: both replays equal to_rgb of the frames a
    twin session returns step by step"""
    tabs = np.stack(oracle.qtables(quality)[:4])
    steps = session_steps(pkg, oracle, w, h, quality, n, seed=91)
    size = n * h * w * BPP[fmt]
    dec, twin = (pkg.DecoderSession(ctx, w, h, tabs, n) for _ in range(2))
    bufs = DevBufs(ctx)
    graph = pkg.Graph(ctx)
    try:
        want = []
        twin.set_deblock("auto")
        for step in steps:
            decode_step(twin, bufs, step)
            want.append(to_rgb_many(twin.get_frame(), w, h, fmt))
        dev_steps = [tuple(bufs.put(x) for x in step) for step in steps]
        outs = [bufs.put(np.full(size, SENTINEL, np.uint8)) for _ in steps]
        dec.set_deblock("auto")
        dec.set_output_rgb_dev(outs[0], fmt)          # the scratch is made here
        with graph:
            for t, st in enumerate(dev_steps):
                dec.set_output_rgb_dev(outs[t], fmt)
                if t == 0:
                    dec.decode_iframe_dev(*st)
                else:
                    dec.decode_pframe_dev(*st)
        for _ in range(2):
            for o in outs:
                ctx.upload(o, np.full(size, SENTINEL, np.uint8))
            graph.launch()
            for t, o in enumerate(outs):
                got = np.zeros(size, np.uint8)
                ctx.download(got, o)
                assert np.array_equal(got.reshape(want[t].shape), want[t]), t
        dec.check()
    finally:
        graph.close()
        bufs.close()
        dec.close()
        twin.close()


# ------------------------------------------------------------------ 5. pfv_decoder
def decoder_callbacks(pkg, ctx, dec, nbytes, device_out):
    """every callback of the advance calls as (y bytes, u, v) through the C ABI itself"""
    from ctypes import CFUNCTYPE, c_int, c_void_p
    seen = []

    def cb(_user, y, u, v, w, h):
        a = np.zeros(nbytes, np.uint8)
        if device_out:
            ctx.download(a, int(y))
        else:
            a[:] = np.ctypeslib.as_array(ctypes.cast(y, ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes,))
        seen.append((a, u, v))
    fn = CFUNCTYPE(None, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int)(cb)
    while True:
        rc = ctx._lib.pfv_decoder_advance_frame(dec.handle, fn, None)
        ctx.check(min(rc, 0))
        if rc != 1:
            return seen


def check_decoder(pkg, ctx, oracle, entropy, device_out, deblock, w=48, h=32, quality=5, n_frames=5, gop=3, drop_at=2):
    """a 5-frame .pfv with one drop frame: with the switch on, every callback has u == v == NULL and y == to_rgb of the frame the same decoder
    delivers with the switch off (which is the oracle decoder's frame, deblocked by numpy when the filter is on); as many callbacks as
    without; reset() and the Python mirror give the same pictures"""
    st = pkg.SyntheticStream(w, h)
    frames = [st.frame(t) for t in range(n_frames)]
    plan = qc.clip_plan(n_frames, gop, drop_at)
    assert "D" in plan
    data = dc.oracle_clip(pkg, oracle, w, h, quality, frames, plan)
    shown = [f for f in qc.oracle_decode(oracle, data) if f is not None]
    auto = dc.auto_strengths(pkg, quality)
    kinds = [k for k in plan if k != "D"]
    fb = frame_bytes(w, h)
    for fmt in FORMATS:
        dec = pkg.Decoder(data, ctx, entropy=entropy)
        try:
            if device_out:
                dec.set_output_device(True)
            dec.set_deblock(deblock)
            plain = decoder_callbacks(pkg, ctx, dec, fb, device_out)
            assert len(plain) == n_frames - 1 and all(u and v for _, u, v in plain)
            for (a, _, _), f, kind in zip(plain, shown, kinds):
                assert np.array_equal(a, dc.ref_frame(f, w, h, auto[kind]) if deblock == "auto" else f)
            dec.reset()
            dec.set_output_rgb(True, fmt)
            for again in range(2):
                got = decoder_callbacks(pkg, ctx, dec, w * h * BPP[fmt], device_out)
                assert len(got) == len(plain), (fmt, len(got))
                for t, ((pic, u, v), (a, _, _)) in enumerate(zip(got, plain)):
                    assert u is None and v is None, (fmt, t, "u / v must be NULL")
                    assert np.array_equal(pic.reshape(h, w, BPP[fmt]), to_rgb(a, w, h, fmt)), (fmt, t, entropy, device_out, deblock, again)
                dec.reset()
            if not device_out:                       # the Python mirror hands arrays over
                pics = []
                while dec.advance_frame(pics.append):
                    pass
                assert len(pics) == len(plain) and all(np.array_equal(p, to_rgb(a, w, h, fmt)) for p, (a, _, _) in zip(pics, plain))
                dec.reset()
            dec.set_output_rgb(False)
            back = decoder_callbacks(pkg, ctx, dec, fb, device_out)
            assert len(back) == len(plain) and all(u and v and np.array_equal(a, b) for (a, u, v), (b, _, _) in zip(back, plain))
        finally:
            dec.close()


# ------------------------------------------------------------------ 6. bad arguments
def check_bad_arguments(pkg, ctx, oracle):
    L = pkg._lib
    lib = ctx._lib
    w, h = 16, 16
    fb, pfb = frame_bytes(w, h), padded_frame_bytes(w, h)
    bufs = DevBufs(ctx)
    try:
        a = bufs.put(np.zeros(8 * w * h * 4, dtype=np.uint8))
        d = bufs.put(np.zeros(8 * w * h * 4, dtype=np.uint8))

        def call(w=w, h=h, n=1, src=a, layout=PACKED, ss=0, dst=d, fmt=1, pitch=0, stride=0, ctx_h=ctx.handle):
            return lib.pfv_frames_to_rgb_dev(ctx_h, w, h, n, P(src) if src else None, layout, ss, P(dst) if dst else None, fmt, pitch, stride)
        assert call() == L.PFV_OK and call(n=2, layout=PADDED) == L.PFV_OK and call(fmt=0) == L.PFV_OK and call(fmt=2) == L.PFV_OK
        assert [lib.pfv_rgb_row_bytes(w, f) for f in (0, 1, 2, 3, -1)] == [48, 64, 64, 0, 0] and lib.pfv_rgb_row_bytes(0, 0) == 0
        for bad in ((15, 16), (16, 17), (0, 16), (16, -2), (65536, 16), (129, 17)):          # dimensions a frame cannot have
            assert call(w=bad[0], h=bad[1]) == L.PFV_ERR_BAD_ARG, bad
        assert call(n=0) == L.PFV_ERR_BAD_ARG and call(n=-1) == L.PFV_ERR_BAD_ARG
        assert call(layout=2) == L.PFV_ERR_BAD_ARG and call(layout=-1) == L.PFV_ERR_BAD_ARG
        assert call(fmt=3) == L.PFV_ERR_BAD_ARG and call(fmt=-1) == L.PFV_ERR_BAD_ARG
        assert call(src=None) == L.PFV_ERR_BAD_ARG and call(dst=None) == L.PFV_ERR_BAD_ARG and call(ctx_h=None) == L.PFV_ERR_BAD_ARG
        assert call(pitch=63) == L.PFV_ERR_BAD_ARG and call(pitch=64) == L.PFV_OK and call(fmt=0, pitch=47) == L.PFV_ERR_BAD_ARG and call(fmt=0, pitch=48) == L.PFV_OK
        assert call(n=2, stride=64 * h - 1) == L.PFV_ERR_BAD_ARG and call(n=2, stride=64 * h) == L.PFV_OK
        assert call(n=2, pitch=80, stride=64 * h) == L.PFV_ERR_BAD_ARG and call(n=2, pitch=80, stride=80 * h) == L.PFV_OK
        assert call(n=2, ss=fb - 1) == L.PFV_ERR_BAD_ARG and call(n=2, ss=fb) == L.PFV_OK
        assert call(n=2, layout=PADDED, ss=pfb - 1) == L.PFV_ERR_BAD_ARG and call(n=2, layout=PADDED, ss=pfb) == L.PFV_OK
        # overlapping ranges, either way round; a range runs from the first picture to the end of the last row of the last one
        assert call(dst=a) == L.PFV_ERR_BAD_ARG
        assert call(dst=a + fb - 1) == L.PFV_ERR_BAD_ARG and call(dst=a + fb) == L.PFV_OK
        pic = 64 * h
        assert call(src=a + pic - 1, dst=a) == L.PFV_ERR_BAD_ARG and call(src=a + pic, dst=a) == L.PFV_OK
        assert call(src=a + 80 * (h - 1) + 63, dst=a, pitch=80) == L.PFV_ERR_BAD_ARG and call(src=a + 80 * (h - 1) + 64, dst=a, pitch=80) == L.PFV_OK
        assert call(n=2, src=a + pic, dst=a, stride=2 * pic) == L.PFV_ERR_BAD_ARG            # the source lies in the gap between the pictures
        # the host form
        host, out = np.zeros(fb, np.uint8), np.zeros(w * h * 4, np.uint8)
        hp = lambda x: x.ctypes.data_as(P)      # noqa: E731
        assert lib.pfv_frames_to_rgb(ctx.handle, w, h, 1, hp(host), hp(out), 1) == L.PFV_OK
        assert lib.pfv_frames_to_rgb(ctx.handle, 15, h, 1, hp(host), hp(out), 1) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_to_rgb(ctx.handle, w, h, 0, hp(host), hp(out), 1) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_to_rgb(ctx.handle, w, h, 1, None, hp(out), 1) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_to_rgb(ctx.handle, w, h, 1, hp(host), None, 1) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_to_rgb(ctx.handle, w, h, 1, hp(host), hp(out), 3) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_to_rgb(None, w, h, 1, hp(host), hp(out), 1) == L.PFV_ERR_BAD_ARG
        # the session's calls and the decoder's switch
        assert lib.pfv_dec_get_frame_rgb_dev(None, P(d), 1, 0, 0) == L.PFV_ERR_BAD_ARG and lib.pfv_dec_get_frame_rgb(None, hp(out), 1) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_dec_set_output_rgb_dev(None, P(d), 1, 0, 0) == L.PFV_ERR_BAD_ARG and lib.pfv_decoder_set_output_rgb(None, 1, 1) == L.PFV_ERR_BAD_ARG
        dec = pkg.DecoderSession(ctx, w, h, np.stack(pkg.qtables_from_quality(5)[:4]), 2)
        graph = pkg.Graph(ctx)
        try:
            for fn in (lib.pfv_dec_get_frame_rgb_dev, lib.pfv_dec_set_output_rgb_dev):
                assert fn(dec.handle, P(d), 1, 0, 0) == L.PFV_OK and fn(dec.handle, P(d), 0, 48, 48 * h) == L.PFV_OK
                assert fn(dec.handle, P(d), 3, 0, 0) == L.PFV_ERR_BAD_ARG and fn(dec.handle, P(d), -1, 0, 0) == L.PFV_ERR_BAD_ARG
                assert fn(dec.handle, P(d), 1, 63, 0) == L.PFV_ERR_BAD_ARG and fn(dec.handle, P(d), 1, 80, 80 * h - 1) == L.PFV_ERR_BAD_ARG
            assert lib.pfv_dec_get_frame_rgb_dev(dec.handle, None, 1, 0, 0) == L.PFV_ERR_BAD_ARG
            assert lib.pfv_dec_set_output_rgb_dev(dec.handle, None, 7, 1, 1) == L.PFV_OK          # NULL: off, whatever the rest says
            big = np.zeros(2 * w * h * 4, np.uint8)
            assert lib.pfv_dec_get_frame_rgb(dec.handle, hp(big), 1) == L.PFV_OK
            assert lib.pfv_dec_get_frame_rgb(dec.handle, None, 1) == L.PFV_ERR_BAD_ARG and lib.pfv_dec_get_frame_rgb(dec.handle, hp(big), 3) == L.PFV_ERR_BAD_ARG
            with pytest.raises(pkg.PfvError):
                dec.get_frame_rgb(5)
            # while a graph is being recorded: the host forms refuse, the device forms are recorded
            with graph:
                assert lib.pfv_frames_to_rgb(ctx.handle, w, h, 1, hp(host), hp(out), 1) == L.PFV_ERR_STATE
                assert lib.pfv_dec_get_frame_rgb(dec.handle, hp(big), 1) == L.PFV_ERR_STATE
                assert call() == L.PFV_OK and lib.pfv_dec_get_frame_rgb_dev(dec.handle, P(d), 1, 0, 0) == L.PFV_OK
        finally:
            graph.close()
            dec.close()
        st = pkg.SyntheticStream(w, h)
        data = dc.oracle_clip(pkg, oracle, w, h, 5, [st.frame(0)], ["I"])
        sd = pkg.Decoder(data, ctx)
        try:
            assert lib.pfv_decoder_set_output_rgb(sd.handle, 1, 3) == L.PFV_ERR_BAD_ARG and lib.pfv_decoder_set_output_rgb(sd.handle, 1, -1) == L.PFV_ERR_BAD_ARG
            assert lib.pfv_decoder_set_output_rgb(sd.handle, 1, 2) == L.PFV_OK and lib.pfv_decoder_set_output_rgb(sd.handle, 0, 9) == L.PFV_OK
        finally:
            sd.close()
        ctx.sync()
    finally:
        bufs.close()


# ------------------------------------------------------------------ 7. C++ mirror and tool
def build_cpp(lib_path, exe):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "present_report.cpp"), "-o", exe, lib_path, "-Wl,-rpath," + os.path.dirname(lib_path)], check=True)


def check_cpp(pkg, ctx, oracle, exe, tmp_path, w=48, h=32, quality=5):
    """tests/cpp/present_report.cpp (pfv::Decoder::set_output_rgb, pfv::frames_to_rgb, pfv::rgb_row_bytes) writes what the numpy oracle makes
    of the oracle decoder's frames"""
    st = pkg.SyntheticStream(w, h)
    frames = [st.frame(t) for t in range(4)]
    data = dc.oracle_clip(pkg, oracle, w, h, quality, frames, ["I", "P", "P", "I"])
    shown = qc.oracle_decode(oracle, data)
    src = str(tmp_path / "in.pfv")
    open(src, "wb").write(data)
    for fmt, code in FORMATS.items():
        o1, o2 = str(tmp_path / f"{fmt}_pictures.bin"), str(tmp_path / f"{fmt}_converted.bin")
        r = subprocess.run([exe, src, str(code), o1, o2], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert r.stdout.splitlines() == [f"frames 4 pictures 4 of {w}x{h} row {w * BPP[fmt]}"]
        want = to_rgb_many(shown, w, h, fmt)
        for path in (o1, o2):
            assert np.array_equal(np.fromfile(path, dtype=np.uint8).reshape(want.shape), want), (fmt, path)


def check_rd_tool(pkg, lib_path, w=64, h=48):
    """tools/rd_curve.py --time-present on the library at lib_path prints its rows: per shape one line per format with the three ways'
    milliseconds and rates"""
    env = dict(os.environ)
    env["PFV_HIP_LIB"] = lib_path
    cmd = [sys.executable, os.path.join(ROOT, "tools", "rd_curve.py"), str(w), str(h), "1", "--qualities", "", "--time-present"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr
    rows = [json.loads(x)["time_present"] for x in r.stdout.splitlines()]
    assert [x["format"] for x in rows] == list(FORMATS) and all(x["shape"] == f"1 x {w}x{h}" for x in rows)
    fb = frame_bytes(w, h)
    for x in rows:
        for key in ("a_present_ms", "b_crop_plus_per_stream_ms", "c_crop_ms"):
            assert x[key] >= 0, (key, x)
        assert "a_over_b_time" in x and "a_rate_over_c_rate" in x      # ratios of times: None on a device without a clock (the emulator)
        assert x["bytes"] == {"a_present": fb + w * h * BPP[x["format"]], "b_crop_plus_per_stream": 3 * fb + w * h * 3, "c_crop": 2 * fb}
        assert set(x["GBps"]) == {"a_present", "b_crop_plus_per_stream", "c_crop"}
    return rows
