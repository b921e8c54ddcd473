"""Shared checks of the distortion entry points (include/pfv_hip_ext.h, "distortion on the device"), driven on the CPU emulator by
tests/test_emu_quality.py and on a real MI355X by tests/test_gpu_quality.py at the same small shapes.

The reference value everywhere is numpy in 64-bit integers, ((a.astype(np.int64) - b) ** 2).sum() over the picture region; for sessions
and streams the second operand is what the ORACLE reconstructs / decodes, never a download of the product's own buffers.  Every sum
and every map entry must be equal, not close."""
import ctypes
import io
import json
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKED, PADDED = 0, 1
LAYOUT_PAIRS = [(PACKED, PACKED), (PACKED, PADDED), (PADDED, PACKED), (PADDED, PADDED)]
# 2x2: chroma 1x1, one partial macroblock per plane; 18x34: chroma 9x17, odd widths and unaligned packed plane bases (byte path);
# 50x38: ragged in both axes; 144x16: 9 macroblocks wide, a second, partial strip; 400x80: interior strips, several strips per workgroup;
# 64x48: fully aligned, the 16-byte path
SHAPES = [(2, 2), (18, 34), (50, 38), (144, 16), (400, 80), (64, 48)]
HEADER_BYTES = 8 + 4 + 2 + 2 + 2 + 2 + 4 * 64 * 2          # magic, version, width, height, framerate, table count, four q-tables


def pad16(x):
    return (x + 15) // 16 * 16


def plane_dims(w, h):
    return [(w, h), (w // 2, h // 2), (w // 2, h // 2)]


def frame_bytes(w, h):
    return sum(pw * ph for pw, ph in plane_dims(w, h))


def padded_frame_bytes(w, h):
    return sum(pad16(pw) * pad16(ph) for pw, ph in plane_dims(w, h))


def total_blocks(w, h):
    return sum((pad16(pw) // 16) * (pad16(ph) // 16) for pw, ph in plane_dims(w, h))


def planes_of(frame, w, h, padded=False):
    """the three planes of one frame as 2-D views of the PICTURE region"""
    out, off = [], 0
    for pw, ph in plane_dims(w, h):
        sw, sh = (pad16(pw), pad16(ph)) if padded else (pw, ph)
        out.append(frame[off:off + sw * sh].reshape(sh, sw)[:ph, :pw])
        off += sw * sh
    return out


def to_padded(frame, w, h, rng):
    """a padded frame with the same picture and RANDOM padding: counting a padding byte would change the result"""
    parts = []
    for pl, (pw, ph) in zip(planes_of(frame, w, h), plane_dims(w, h)):
        buf = rng.integers(0, 256, (pad16(ph), pad16(pw)), dtype=np.uint8)
        buf[:ph, :pw] = pl
        parts.append(buf.reshape(-1))
    return np.concatenate(parts)


def ref_sse(a, b, w, h):
    """numpy reference on packed frames: (sse int64 [3], map int64 [total_blocks])"""
    sums, maps = [], []
    for pa, pb, (pw, ph) in zip(planes_of(a, w, h), planes_of(b, w, h), plane_dims(w, h)):
        d = (pa.astype(np.int64) - pb) ** 2
        sums.append(int(d.sum()))
        full = np.zeros((pad16(ph), pad16(pw)), dtype=np.int64)
        full[:ph, :pw] = d
        maps.append(full.reshape(pad16(ph) // 16, 16, pad16(pw) // 16, 16).sum(axis=(1, 3)).reshape(-1))
    return np.array(sums, dtype=np.int64), np.concatenate(maps)


def ref_sse_many(a, b, w, h):
    r = [ref_sse(x, y, w, h) for x, y in zip(a, b)]
    return np.stack([s for s, _ in r]), np.stack([m for _, m in r])


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


def sse_dev(pkg, ctx, w, h, n, a_buf, a_layout, a_stride, b_buf, b_layout, b_stride, with_map=True, same=False):
    """pfv_frames_sse_dev on uploaded operands -> (sse uint64 [n, 3], map uint32 [n, total_blocks] or None); outputs are preset with a
    pattern, so an entry the kernels do not write shows"""
    bufs = DevBufs(ctx)
    try:
        a_dev = bufs.put(a_buf)
        b_dev = a_dev if same else bufs.put(b_buf)
        sse = np.full((n, 3), 0xDEADBEEFDEADBEEF, dtype=np.uint64)
        mb = np.full((n, total_blocks(w, h)), 0xABABABAB, dtype=np.uint32)
        sse_d = bufs.put(sse)
        mb_d = bufs.put(mb) if with_map else 0
        rc = ctx._lib.pfv_frames_sse_dev(ctx.handle, w, h, n, ctypes.c_void_p(a_dev), a_layout, a_stride, ctypes.c_void_p(b_dev), b_layout, b_stride,
                                         ctypes.c_void_p(sse_d), ctypes.c_void_p(mb_d))
        ctx.check(rc)
        ctx.download(sse, sse_d)
        if with_map:
            ctx.download(mb, mb_d)
        return sse, (mb if with_map else None)
    finally:
        bufs.close()


def check_plane_shape(pkg, ctx, w, h, seed=1):
    """one frame of random bytes: the four layout pairs, the host entry point and the NULL-map form all give numpy's numbers"""
    rng = np.random.default_rng(seed * 1000 + w * 7 + h)
    a = rng.integers(0, 256, frame_bytes(w, h), dtype=np.uint8)
    b = rng.integers(0, 256, frame_bytes(w, h), dtype=np.uint8)
    want_sse, want_map = ref_sse(a, b, w, h)
    assert int(want_map.sum()) == int(want_sse.sum())
    forms = {PACKED: (a, b), PADDED: (to_padded(a, w, h, rng), to_padded(b, w, h, rng))}
    assert forms[PADDED][0].size == padded_frame_bytes(w, h) == int(ctx._lib.pfv_padded_frame_bytes(w, h))
    for la, lb in LAYOUT_PAIRS:
        sse, mb = sse_dev(pkg, ctx, w, h, 1, forms[la][0], la, 0, forms[lb][1], lb, 0)
        assert np.array_equal(sse[0].astype(np.int64), want_sse), (la, lb, sse, want_sse)
        assert np.array_equal(mb[0].astype(np.int64), want_map), (la, lb)
        off = 0
        for p, (pw, ph) in enumerate(plane_dims(w, h)):       # the map sums to the plane totals
            n = (pad16(pw) // 16) * (pad16(ph) // 16)
            assert int(mb[0, off:off + n].astype(np.int64).sum()) == int(sse[0, p])
            off += n
    sse, _ = sse_dev(pkg, ctx, w, h, 1, a, PACKED, 0, forms[PADDED][1], PADDED, 0, with_map=False)      # map to the context's scratch
    assert np.array_equal(sse[0].astype(np.int64), want_sse)
    sse, mb = pkg.frames_sse(ctx, w, h, a, b, mb_map=True)                                              # host buffers
    assert sse.shape == (1, 3) and np.array_equal(sse[0].astype(np.int64), want_sse) and np.array_equal(mb[0].astype(np.int64), want_map)
    assert np.array_equal(pkg.frames_sse(ctx, w, h, a, b), sse)
    return want_sse


def check_strided_streams(pkg, ctx, w, h, seed=2):
    """three streams, each operand with a stride larger than its frame (one stride keeps 16-byte alignment, the other breaks it); the
    gaps hold random bytes"""
    rng = np.random.default_rng(seed + w)
    n = 3
    a = rng.integers(0, 256, (n, frame_bytes(w, h)), dtype=np.uint8)
    b = rng.integers(0, 256, (n, frame_bytes(w, h)), dtype=np.uint8)
    want_sse, want_map = ref_sse_many(a, b, w, h)
    for la, lb in LAYOUT_PAIRS:
        fa = a if la == PACKED else np.stack([to_padded(x, w, h, rng) for x in a])
        fb = b if lb == PACKED else np.stack([to_padded(x, w, h, rng) for x in b])
        sa, sb = pad16(fa.shape[1]) + 48, fb.shape[1] + 5
        ba, bb = rng.integers(0, 256, (n, sa), dtype=np.uint8), rng.integers(0, 256, (n, sb), dtype=np.uint8)
        ba[:, :fa.shape[1]] = fa
        bb[:, :fb.shape[1]] = fb
        sse, mb = sse_dev(pkg, ctx, w, h, n, ba, la, sa, bb, lb, sb)
        assert np.array_equal(sse.astype(np.int64), want_sse), (la, lb)
        assert np.array_equal(mb.astype(np.int64), want_map), (la, lb)
    sse, mb = pkg.frames_sse(ctx, w, h, a, b, mb_map=True)
    assert np.array_equal(sse.astype(np.int64), want_sse) and np.array_equal(mb.astype(np.int64), want_map)


def check_same_buffer(pkg, ctx, w, h):
    rng = np.random.default_rng(w + h)
    a = rng.integers(0, 256, (2, frame_bytes(w, h)), dtype=np.uint8)
    sse, mb = sse_dev(pkg, ctx, w, h, 2, a, PACKED, 0, a, PACKED, 0, same=True)
    assert not sse.any() and not mb.any()
    sse, mb = pkg.frames_sse(ctx, w, h, a, a, mb_map=True)
    assert sse.shape == (2, 3) and not sse.any() and not mb.any()


def check_corner_pixel(pkg, ctx, w, h):
    """a single differing pixel in the bottom-right corner of each plane: exactly one map entry per plane, with the exact value"""
    rng = np.random.default_rng(w * h)
    a = rng.integers(0, 256, frame_bytes(w, h), dtype=np.uint8)
    b = a.copy()
    deltas, off = [3, 200, 77], 0
    for (pw, ph), d in zip(plane_dims(w, h), deltas):
        off += pw * ph
        b[off - 1] = (int(a[off - 1]) + d) % 256
    want_sse, want_map = ref_sse(a, b, w, h)
    for la, lb in LAYOUT_PAIRS:
        fa = a if la == PACKED else to_padded(a, w, h, rng)
        fb = b if lb == PACKED else to_padded(b, w, h, rng)
        sse, mb = sse_dev(pkg, ctx, w, h, 1, fa, la, 0, fb, lb, 0)
        assert np.array_equal(sse[0].astype(np.int64), want_sse) and np.array_equal(mb[0].astype(np.int64), want_map)
        off = 0
        for p, (pw, ph) in enumerate(plane_dims(w, h)):
            n = (pad16(pw) // 16) * (pad16(ph) // 16)
            nz = np.flatnonzero(mb[0, off:off + n])
            diff = int(b[sum(x * y for x, y in plane_dims(w, h)[:p + 1]) - 1]) - int(a[sum(x * y for x, y in plane_dims(w, h)[:p + 1]) - 1])
            assert list(nz) == [n - 1] and int(mb[0, off + n - 1]) == diff * diff == int(sse[0, p])
            off += n


def check_extremes(pkg, ctx):
    """272 x 256, all 0 against all 255: the Y sum exceeds 2^32, every full macroblock holds the largest possible entry"""
    w, h = 272, 256
    a = np.zeros(frame_bytes(w, h), dtype=np.uint8)
    b = np.full(frame_bytes(w, h), 255, dtype=np.uint8)
    rng = np.random.default_rng(5)
    for la, lb in LAYOUT_PAIRS:
        fa = a if la == PACKED else to_padded(a, w, h, rng)
        fb = b if lb == PACKED else to_padded(b, w, h, rng)
        sse, mb = sse_dev(pkg, ctx, w, h, 1, fa, la, 0, fb, lb, 0)
        assert int(sse[0, 0]) == 69632 * 65025 == 4527820800 and int(sse[0, 0]) > 2 ** 32
        assert int(sse[0, 1]) == int(sse[0, 2]) == 136 * 128 * 65025
        ny = (w // 16) * (h // 16)
        assert (mb[0, :ny] == 16646400).all()                                     # Y: 17 x 16 full macroblocks
        cm = mb[0, ny:ny + 9 * 8].reshape(8, 9)                                   # U: 136 x 128 -> 9 x 8, the last column 8 pixels wide
        assert (cm[:, :8] == 16646400).all() and (cm[:, 8] == 8 * 16 * 65025).all()
        want_sse, want_map = ref_sse(a, b, w, h)
        assert np.array_equal(sse[0].astype(np.int64), want_sse) and np.array_equal(mb[0].astype(np.int64), want_map)


def check_bad_arguments(pkg, ctx):
    L = pkg._lib
    lib = ctx._lib
    w, h = 16, 16
    bufs = DevBufs(ctx)
    try:
        a = bufs.put(np.zeros(2 * padded_frame_bytes(w, h), dtype=np.uint8))
        sse = bufs.put(np.zeros(6, dtype=np.uint64))
        P = ctypes.c_void_p

        def call(w=w, h=h, n=1, a=a, la=PACKED, sa=0, b=a, lb=PACKED, sb=0, sse=sse):
            return lib.pfv_frames_sse_dev(ctx.handle, w, h, n, P(a), la, sa, P(b), lb, sb, P(sse), None)
        assert call() == L.PFV_OK
        assert call(w=15) == L.PFV_ERR_BAD_ARG and call(h=17) == L.PFV_ERR_BAD_ARG and call(w=0) == L.PFV_ERR_BAD_ARG and call(h=-2) == L.PFV_ERR_BAD_ARG
        assert call(n=0) == L.PFV_ERR_BAD_ARG and call(n=-1) == L.PFV_ERR_BAD_ARG
        assert call(la=2) == L.PFV_ERR_BAD_ARG and call(lb=2) == L.PFV_ERR_BAD_ARG and call(la=-1) == L.PFV_ERR_BAD_ARG
        assert call(sa=frame_bytes(w, h) - 1) == L.PFV_ERR_BAD_ARG and call(sb=frame_bytes(w, h) - 1) == L.PFV_ERR_BAD_ARG
        assert call(lb=PADDED, sb=padded_frame_bytes(w, h) - 1) == L.PFV_ERR_BAD_ARG      # enough for a packed frame, not for a padded one
        assert call(sa=frame_bytes(w, h), lb=PADDED, sb=padded_frame_bytes(w, h)) == L.PFV_OK
        assert call(a=None) == L.PFV_ERR_BAD_ARG and call(b=None) == L.PFV_ERR_BAD_ARG and call(sse=None) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_sse_dev(None, w, h, 1, P(a), 0, 0, P(a), 0, 0, P(sse), None) == L.PFV_ERR_BAD_ARG
        host = np.zeros(frame_bytes(w, h), dtype=np.uint8)
        out = np.zeros(3, dtype=np.uint64)
        hp = lambda x: x.ctypes.data_as(P)      # noqa: E731
        assert lib.pfv_frames_sse(ctx.handle, w, h, 1, hp(host), hp(host), hp(out), None) == L.PFV_OK
        assert lib.pfv_frames_sse(ctx.handle, 15, h, 1, hp(host), hp(host), hp(out), None) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_sse(ctx.handle, w, h, 0, hp(host), hp(host), hp(out), None) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_sse(ctx.handle, w, h, 1, None, hp(host), hp(out), None) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_sse(ctx.handle, w, h, 1, hp(host), None, hp(out), None) == L.PFV_ERR_BAD_ARG
        assert lib.pfv_frames_sse(ctx.handle, w, h, 1, hp(host), hp(host), None, None) == L.PFV_ERR_BAD_ARG
        ctx.sync()
    finally:
        bufs.close()


def check_psnr(pkg):
    assert pkg.psnr(0, 100) == math.inf and pkg.psnr(0, 1) == math.inf
    assert math.isnan(pkg.psnr(5, 0)) and math.isnan(pkg.psnr(0, 0))
    rng = np.random.default_rng(9)
    cases = [(1, 1), (65025, 1), (1, 2 ** 40), (2 ** 40, 1), (4527820800, 69632), (16646400, 256), (3, 7)]
    cases += [(int(s), int(n)) for s, n in zip(rng.integers(1, 2 ** 50, 200), rng.integers(1, 2 ** 33, 200))]
    for sse, n in cases:
        want = 10 * np.log10(255.0 ** 2 * n / sse)
        assert abs(pkg.psnr(sse, n) - want) <= 1e-9, (sse, n, pkg.psnr(sse, n), want)


# ------------------------------------------------------------------ sessions
def crop(padded, w, h):
    return np.concatenate([p.reshape(-1) for p in planes_of(padded, w, h, padded=True)])


def check_enc_session(pkg, ctx, oracle, w=64, h=48, quality=5, n=2):
    """i-frame, then two p-frames: after each step distortion == numpy SSE between the input frames and the ORACLE's reconstruction"""
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
            want_sse, want_map = ref_sse_many(frames, recon, w, h)
            assert want_sse.sum() > 0                                   # quality 5 is lossy: the check is not 0 == 0
            sse, mb = enc.distortion(frames, mb_map=True)
            assert sse.dtype == np.uint64 and sse.shape == (n, 3) and np.array_equal(sse.astype(np.int64), want_sse), (t, sse, want_sse)
            assert np.array_equal(mb.astype(np.int64), want_map)
            assert np.array_equal(enc.distortion(frames), sse)          # map to the session's scratch
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
        want_sse, want_map = ref_sse(f1[slot], crop(oenc[slot].prev_frame(), w, h), w, h)
        sent = np.full((n, 3), 0x1122334455667788, dtype=np.uint64)
        sent_map = np.full((n, tb), 0x5A5A5A5A, dtype=np.uint32)
        for frames in (f1, frames_dev):                                  # an array (uploaded) and a device address
            sse, mb = enc.distortion(frames, mb_map=True, out=sent, out_map=sent_map)
            assert np.array_equal(sse[slot].astype(np.int64), want_sse) and np.array_equal(mb[slot].astype(np.int64), want_map)
            for k in (0, 2):
                assert np.array_equal(sse[k], sent[k]) and np.array_equal(mb[k], sent_map[k])
        sse = enc.distortion(f1, out=sent)
        assert np.array_equal(sse[slot].astype(np.int64), want_sse) and np.array_equal(sse[[0, 2]], sent[[0, 2]])
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
        want_sse, want_map = ref_sse_many(frames, np.stack([crop(o.prev_frame(), w, h) for o in oenc]), w, h)
        for src in (laid, frames_dev):
            sse, mb = enc.distortion(src, mb_map=True)
            assert np.array_equal(sse.astype(np.int64), want_sse) and np.array_equal(mb.astype(np.int64), want_map)
    finally:
        bufs.close()
        enc.close()


def check_dec_session(pkg, ctx, oracle, w=64, h=48, quality=5, n=2):
    """DecoderSession.distortion after decoding the ORACLE's coefficients, against the oracle decoder's framebuffer"""
    from oracle_bind import OracleDecoder
    tabs = np.stack(oracle.qtables(quality)[:4])
    streams = [pkg.SyntheticStream(w, h, seed=41 + k) for k in range(n)]
    oenc = [oracle.encoder(w, h, quality) for _ in range(n)]
    odec = [OracleDecoder(oracle, w, h, tabs) for _ in range(n)]
    dec = pkg.DecoderSession(ctx, w, h, tabs, n)
    try:
        for t in range(2):
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
            want_sse, want_map = ref_sse_many(frames, np.stack([crop(d.framebuffer(), w, h) for d in odec]), w, h)
            assert want_sse.sum() > 0
            sse, mb = dec.distortion(frames, mb_map=True)
            assert np.array_equal(sse.astype(np.int64), want_sse) and np.array_equal(mb.astype(np.int64), want_map)
            assert np.array_equal(dec.distortion(frames), sse)
        dec.set_window(1, 1)
        sent = np.full((n, 3), 7, dtype=np.uint64)
        sse = dec.distortion(frames, out=sent)
        assert np.array_equal(sse[1].astype(np.int64), want_sse[1]) and np.array_equal(sse[0], sent[0])
    finally:
        dec.close()


# ------------------------------------------------------------------ pfv_encoder's frame reports
def packets_of(data):
    """(type, len) of every packet of a .pfv stream"""
    out, pos = [], HEADER_BYTES
    while pos < len(data):
        typ, ln = struct.unpack_from("<BI", data, pos)
        out.append((typ, ln))
        pos += 5 + ln
    assert pos == len(data)
    return out


def oracle_decode(oracle, data):
    """the frame the oracle's stream decoder delivers per advance call (None for a drop frame), up to the end of the stream"""
    from oracle_bind import OracleStreamDecoder
    odec = OracleStreamDecoder(oracle, data)
    out = []
    while True:
        rc, fr = odec.advance_frame()
        assert rc >= 0
        if rc == 0:
            break
        out.append(fr)
    return out


def clip_plan(n_frames, gop, drop_at):
    return ["D" if t == drop_at else ("I" if t % gop == 0 else "P") for t in range(n_frames)]


def encode_with_reports(pkg, ctx, w, h, quality, frames, plan, device_entropy, frame_report=True):
    buf = io.BytesIO()
    enc = pkg.Encoder(buf, w, h, 30, quality, ctx, device_entropy=device_entropy, frame_report=frame_report)
    reports = []
    try:
        with pytest.raises(pkg.PfvError) as e:           # before any frame; or reports off
            enc.last_report
        assert e.value.code == pkg._lib.PFV_ERR_STATE
        for f, kind in zip(frames, plan):
            if kind == "D":
                enc.encode_dropframe()
            elif kind == "I":
                enc.encode_iframe(pkg.VideoFrame.from_packed(w, h, f))
            else:
                enc.encode_pframe(pkg.VideoFrame.from_packed(w, h, f))
            if frame_report:
                reports.append(enc.last_report)
            else:
                with pytest.raises(pkg.PfvError) as e:
                    enc.last_report
                assert e.value.code == pkg._lib.PFV_ERR_STATE
        enc.finish()
    finally:
        enc.close()
    return buf.getvalue(), reports


def check_encoder_reports(pkg, ctx, oracle, device_entropy, w=48, h=32, quality=5, n_frames=5, gop=3, drop_at=2):
    from oracle_bind import OracleStreamEncoder
    st = pkg.SyntheticStream(w, h)
    frames = [st.frame(t) for t in range(n_frames)]
    plan = clip_plan(n_frames, gop, drop_at)
    data, reports = encode_with_reports(pkg, ctx, w, h, quality, frames, plan, device_entropy)
    oenc = OracleStreamEncoder(oracle, w, h, 30, quality)
    for f, kind in zip(frames, plan):
        {"D": lambda f: oenc.encode_dropframe(), "I": oenc.encode_iframe, "P": oenc.encode_pframe}[kind](f)
    oenc.finish()
    assert data == oenc.bytes(), "stream bytes with reports on differ from the oracle encoder's"
    plain, none = encode_with_reports(pkg, ctx, w, h, quality, frames, plan, device_entropy, frame_report=False)
    assert plain == data and none == [], "stream bytes with reports on differ from the bytes with reports off"
    packets = packets_of(data)
    decoded = oracle_decode(oracle, data)
    assert len(reports) == n_frames and len(packets) == n_frames + 1 and packets[-1] == (0, 0) and len(decoded) == n_frames
    ny, nc = w * h, (w // 2) * (h // 2)
    for t, (r, kind, f, (ptype, plen), shown) in enumerate(zip(reports, plan, frames, packets, decoded)):
        assert r.packet_bytes == 5 + plen, (t, r, plen)
        assert r.type == {"I": 1, "P": 2, "D": 3}[kind] and ptype == (2 if kind == "P" else 1)
        if kind == "D":
            assert plen == 0 and r.sse == (0, 0, 0)
        else:
            want, _ = ref_sse(f, shown, w, h)
            assert r.sse == tuple(int(x) for x in want), (t, r.sse, want)
            assert sum(r.sse) > 0
        for p in range(3):
            assert r.psnr[p] == pkg.psnr(r.sse[p], nc if p else ny)
        assert r.psnr_yuv == pkg.psnr(sum(r.sse), ny + 2 * nc)
    return reports


def check_graph(pkg, ctx, oracle, w=64, h=48, quality=5, n=2):
    """pfv_enc_iframe_dev + pfv_enc_distortion_dev recorded in one graph and replayed twice == the unrecorded calls; a NULL map that
    would need an allocation inside a recording is refused"""
    streams = [pkg.SyntheticStream(w, h, seed=51 + k) for k in range(n)]
    frames = np.stack([s.frame(0) for s in streams])
    oenc = [oracle.encoder(w, h, quality) for _ in range(n)]
    [o.encode_iframe(f) for o, f in zip(oenc, frames)]
    want_sse, want_map = ref_sse_many(frames, np.stack([crop(o.prev_frame(), w, h) for o in oenc]), w, h)
    enc = pkg.EncoderSession(ctx, w, h, quality, n)
    enc2 = pkg.EncoderSession(ctx, w, h, quality, n)
    bufs = DevBufs(ctx)
    graph = pkg.Graph(ctx)
    try:
        tb = enc.total_blocks
        frames_dev, coef = bufs.put(frames), bufs.put(np.zeros(n * tb * 256, np.int16))
        sse_d, map_d = bufs.put(np.zeros((n, 3), np.uint64)), bufs.put(np.zeros((n, tb), np.uint32))
        enc.encode_iframe_dev(frames_dev, coef)                        # the unrecorded calls
        enc.distortion_dev(frames_dev, sse_d, map_d)
        plain_sse, plain_map = np.zeros((n, 3), np.uint64), np.zeros((n, tb), np.uint32)
        ctx.download(plain_sse, sse_d)
        ctx.download(plain_map, map_d)
        assert np.array_equal(plain_sse.astype(np.int64), want_sse) and np.array_equal(plain_map.astype(np.int64), want_map)
        with graph:
            enc.encode_iframe_dev(frames_dev, coef)
            enc.distortion_dev(frames_dev, sse_d, map_d)
            enc2.encode_iframe_dev(frames_dev, coef)
            with pytest.raises(pkg.PfvError) as e:                     # enc2 has never measured: its map would have to be allocated now
                enc2.distortion_dev(frames_dev, sse_d, 0)
            assert e.value.code == pkg._lib.PFV_ERR_STATE and "map buffer" in str(e.value) and "before" in str(e.value)
        for _ in range(2):
            ctx.upload(sse_d, np.full((n, 3), 99, np.uint64))          # a replay recomputes everything: nothing is accumulated or cleared
            ctx.upload(map_d, np.full((n, tb), 99, np.uint32))
            graph.launch()
            got_sse, got_map = np.zeros((n, 3), np.uint64), np.zeros((n, tb), np.uint32)
            ctx.download(got_sse, sse_d)
            ctx.download(got_map, map_d)
            assert np.array_equal(got_sse, plain_sse) and np.array_equal(got_map, plain_map)
    finally:
        graph.close()
        bufs.close()
        enc.close()
        enc2.close()


# ------------------------------------------------------------------ C++ mirror and tool
def build_cpp(lib_path, exe):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "quality_report.cpp"), "-o", exe, lib_path, "-Wl,-rpath," + os.path.dirname(lib_path)], check=True)


def check_cpp_reports(pkg, ctx, exe, tmp_path, w=48, h=32, quality=5, n_frames=4, gop=3, drop_at=-1):
    """tests/cpp/quality_report.cpp (pfv::Encoder::set_frame_report / last_report) prints what the Python Encoder reports for the same clip"""
    st = pkg.SyntheticStream(w, h)
    frames = [st.frame(t) for t in range(n_frames)]
    yuv = str(tmp_path / "in.yuv")
    np.concatenate(frames).tofile(yuv)
    for device_entropy in (1, 0):
        data, reports = encode_with_reports(pkg, ctx, w, h, quality, frames, clip_plan(n_frames, gop, drop_at), bool(device_entropy))
        r = subprocess.run([exe, str(w), str(h), str(quality), str(gop), str(drop_at), str(device_entropy), yuv], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        assert len(lines) == n_frames + 1 and lines[-1] == f"stream {len(data)} bytes"
        for t, (line, rep) in enumerate(zip(lines, reports)):
            tok = line.split()
            assert tok[0] == "frame" and int(tok[1]) == t and int(tok[3]) == rep.type and int(tok[5]) == rep.packet_bytes
            assert tuple(int(x) for x in tok[7:10]) == rep.sse
            assert tuple(float(x) for x in tok[11:14]) == rep.psnr and float(tok[15]) == rep.psnr_yuv == float(tok[16])


def check_rd_tool(pkg, oracle, lib_path, w=64, h=48, n_frames=6, gop=3, qualities=(0, 5, 10)):
    """tools/rd_curve.py on the library at lib_path: every line parses, its byte totals are the oracle encoder's stream lengths, its
    PSNRs numpy's figures from the oracle decoder's frames.  (Nothing is said about monotonicity over quality.)"""
    from oracle_bind import OracleStreamEncoder
    env = dict(os.environ)
    if lib_path:
        env["PFV_HIP_LIB"] = lib_path
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rd_curve.py"), str(w), str(h), str(n_frames), "--gop", str(gop),
                        "--qualities", ",".join(str(q) for q in qualities)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr
    lines = [json.loads(x) for x in r.stdout.splitlines()]
    assert [d["quality"] for d in lines] == list(qualities)
    st = pkg.SyntheticStream(w, h)
    frames = [st.frame(t) for t in range(n_frames)]
    ny, nc = w * h, (w // 2) * (h // 2)
    for d in lines:
        oenc = OracleStreamEncoder(oracle, w, h, 30, d["quality"])
        for t, f in enumerate(frames):
            (oenc.encode_iframe if t % gop == 0 else oenc.encode_pframe)(f)
        oenc.finish()
        data = oenc.bytes()
        packets = packets_of(data)[:-1]
        assert d["stream_bytes"] == len(data) and d["packet_bytes"] == sum(5 + ln for _, ln in packets) == len(data) - HEADER_BYTES - 5
        ib, pb = [5 + ln for ty, ln in packets if ty == 1], [5 + ln for ty, ln in packets if ty == 2]
        assert d["iframes"] == len(ib) == 2 and d["pframes"] == len(pb) == 4
        assert d["iframe_bytes_per_frame"] == sum(ib) / len(ib) and d["pframe_bytes_per_frame"] == sum(pb) / len(pb)
        assert d["bytes_per_frame"] == (sum(ib) + sum(pb)) / n_frames
        sses = np.array([ref_sse(f, shown, w, h)[0] for f, shown in zip(frames, oracle_decode(oracle, data))], dtype=np.float64)
        with np.errstate(divide="ignore"):
            want = [float(np.mean(10 * np.log10(255.0 ** 2 * n / sses[:, p]))) for p, n in enumerate((ny, nc, nc))]
            want_yuv = float(np.mean(10 * np.log10(255.0 ** 2 * (ny + 2 * nc) / sses.sum(axis=1))))
        for key, val in zip(("psnr_y", "psnr_u", "psnr_v", "psnr_yuv"), want + [want_yuv]):
            assert d[key] == val or abs(d[key] - val) <= 1e-9, (key, d[key], val)
    return lines
