"""Shared checks of the encoders' quality ladder and pfv_encoder's p-frame byte budget (include/pfv_hip_ext.h, "quality
ladder"), driven on the CPU emulator by tests/test_emu_ladder.py and on a real MI355X by tests/test_gpu_ladder.py at the same small shapes.

The reference is a LADDER MODEL built here from the oracle's plane-level functions: per rung oracle.qtables(q); the padded prev planes live
in numpy (Y = 0, U = V = 128); an i-frame is encode_plane + decode_plane per plane, a p-frame encode_plane_delta + decode_plane_delta against
prev; payloads are the oracle serialisers' with bytes 16-18 set to the rung's indices and whole streams come from StreamBuilder with a
header of 4K tables.  Everything is compared for equality."""
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest

from pfv_stream_builder import StreamBuilder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LADDER = [0, 2, 5, 7, 10]
RATE_LADDER = [1, 3, 5, 8, 10]
# (w, h, n_streams).  16x16: one macroblock per plane, chroma padded from 8 to 16; 18x34: padding in both directions, partial strips;
# 130x18: luma 9 macroblocks wide (two strips, the second with one macroblock), chroma 65 -> 80; 50x38 x 3: stream indexing
SHAPES = [(16, 16, 1), (18, 34, 1), (130, 18, 1), (50, 38, 3)]
# shapes with strips that penc_search (csrc/pfv_kernels.hip) takes through its search levels WITHOUT bounds tests, for the probes' session checks;
# the shapes above have none.  400x80: luma strips at x0 = 128 and 256, y0 = 16, 32, 48, no chroma ones (200x40); 544x96 x 2: luma ones, and in
# each 272x48 chroma plane exactly one, at x0 = 128, y0 = 16, where the right and the bottom term of the rule hold with equality; two streams
# over 32 tiles
INTERIOR_SHAPES = [(400, 80, 1), (544, 96, 2)]


def pad16(x):
    return (x + 15) // 16 * 16


def plane_dims(w, h):
    return [(w, h), (w // 2, h // 2), (w // 2, h // 2)]


def frame_bytes(w, h):
    return sum(pw * ph for pw, ph in plane_dims(w, h))


def total_blocks(w, h):
    return sum((pad16(pw) // 16) * (pad16(ph) // 16) for pw, ph in plane_dims(w, h))


def split(frame, w, h):
    out, off = [], 0
    for pw, ph in plane_dims(w, h):
        out.append(np.ascontiguousarray(frame[off:off + pw * ph].reshape(ph, pw)))
        off += pw * ph
    return out


# ------------------------------------------------------------------ the model
class LadderModel:
    CLEAR = (0, 128, 128)

    def __init__(self, oracle, w, h, qualities, n_streams=1):
        self.o, self.w, self.h, self.n = oracle, w, h, n_streams
        self.qualities = list(qualities)
        self.tabs = [oracle.qtables(q) for q in qualities]            # (intra_l, intra_c, inter_l, inter_c, px_err) per rung
        self.tb = total_blocks(w, h)
        self.prev = [[np.full((pad16(ph), pad16(pw)), c, np.uint8) for (pw, ph), c in zip(plane_dims(w, h), self.CLEAR)] for _ in range(n_streams)]

    def header_tables(self):
        return np.stack([t for tabs in self.tabs for t in tabs[:4]])

    def iframe_coef(self, frame, rung):
        """coefficients of `frame` as an i-frame at `rung` and the planes it reconstructs to; prev is not touched"""
        il, ic = self.tabs[rung][0], self.tabs[rung][1]
        coefs, recon = [], []
        for p, px in enumerate(split(frame, self.w, self.h)):
            q = il if p == 0 else ic
            c, bw, bh = self.o.encode_plane(px, q, self.CLEAR[p])
            coefs.append(c)
            recon.append(self.o.decode_plane(c, bw, bh, q))
        return np.concatenate(coefs), recon

    def iframe(self, k, frame, rung):
        coef, self.prev[k] = self.iframe_coef(frame, rung)
        return coef

    def pframe(self, k, frame, rung):
        el, ec, px_err = self.tabs[rung][2], self.tabs[rung][3], self.tabs[rung][4]
        mvs, hass, coefs, recon = [], [], [], []
        for p, px in enumerate(split(frame, self.w, self.h)):
            q, ref = (el if p == 0 else ec), self.prev[k][p]
            mv, has, c = self.o.encode_plane_delta(px, ref, q, px_err, self.CLEAR[p])
            recon.append(self.o.decode_plane_delta(mv, has, c, ref.shape[1] // 16, ref.shape[0] // 16, q, ref))
            mvs.append(mv); hass.append(has); coefs.append(c)
        self.prev[k] = recon
        return np.concatenate(mvs), np.concatenate(hass), np.concatenate(coefs)

    def prev_frame(self, k):
        return np.concatenate([p.reshape(-1) for p in self.prev[k]])

    def shown(self, k):
        """what a decoder shows for the current prev: the picture region, packed"""
        return np.concatenate([p[:ph, :pw].reshape(-1) for p, (pw, ph) in zip(self.prev[k], plane_dims(self.w, self.h))])

    # payloads through the oracle's serialisers, indices of the rung at bytes 16-18 (as StreamBuilder does)
    def builder(self, fps=30):
        return StreamBuilder(self.o, self.w, self.h, fps, self.header_tables(), self.tb)

    @staticmethod
    def qidx(rung, pframe):
        return (4 * rung + 2, 4 * rung + 3, 4 * rung + 3) if pframe else (4 * rung, 4 * rung + 1, 4 * rung + 1)

    def payload_i(self, coef, rung):
        sb = self.builder()
        sb.iframe(coef, self.qidx(rung, False))
        return sb.parts[-1][5:]

    def payload_p(self, mv, has, coef, rung):
        sb = self.builder()
        sb.pframe(mv, has, coef, self.qidx(rung, True))
        return sb.parts[-1][5:]


# ------------------------------------------------------------------ content
def box(a):
    """3x3 box filter with wrap-around"""
    acc = np.zeros(a.shape, np.float64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            acc += np.roll(a, (dy, dx), (0, 1))
    return acc / 9.0


def texture(rng, size=256):
    t = box(box(rng.integers(0, 256, (size, size)).astype(np.float64)))
    t = (t - t.min()) / (t.max() - t.min()) * 255.0           # the smoothing flattens the range: stretch it back
    return t


def texture_for(rng, rows, cols):
    """texture() large enough to slice rows x cols from: the 256 one wherever it suffices (the generator's draws, and so every frame of such a
    shape, stay what they were), else the next multiple of 256"""
    return texture(rng, max(256, (max(rows, cols) + 255) // 256 * 256))


def rate_clip(w, h, seed=7, n_frames=14):
    """luma: a twice box-smoothed noise texture panning 2 px per frame, frames 4-6 blended half and half with fresh noise, frames 9 and
    later static; chroma: a slow sinusoid"""
    rng = np.random.default_rng(seed)
    tex = texture_for(rng, 8 + h, 18 + w)
    frames = []
    for t in range(n_frames):
        s = 2 * min(t, 9)
        y = tex[8:8 + h, s:s + w].copy()
        if 4 <= t <= 6:
            y = 0.5 * y + 0.5 * rng.integers(0, 256, (h, w))
        xx, yy = np.meshgrid(np.arange(w // 2), np.arange(h // 2))
        u = 128 + 60 * np.sin(xx / 9.0 + 0.1 * min(t, 9))
        v = 128 + 60 * np.cos(yy / 7.0 - 0.1 * min(t, 9))
        frames.append(np.concatenate([np.clip(np.rint(pl), 0, 255).astype(np.uint8).reshape(-1) for pl in (y, u, v)]))
    return frames


def motion_clip(w, h, seed, n_frames):
    """a smoothed texture panning by (1, 2) px per frame with a little fresh noise: motion vectors, coded and skipped macroblocks"""
    rng = np.random.default_rng(seed)
    tex = texture_for(rng, n_frames - 1 + max(20 * p + ph for p, (pw, ph) in enumerate(plane_dims(w, h))),
                      2 * (n_frames - 1) + max(30 * p + pw for p, (pw, ph) in enumerate(plane_dims(w, h))))
    frames = []
    for t in range(n_frames):
        planes = []
        for p, (pw, ph) in enumerate(plane_dims(w, h)):
            pl = tex[20 * p + t:20 * p + t + ph, 30 * p + 2 * t:30 * p + 2 * t + pw] + rng.integers(-3, 4, (ph, pw)) * (t % 2)
            planes.append(np.clip(np.rint(pl), 0, 255).astype(np.uint8).reshape(-1))
        frames.append(np.concatenate(planes))
    return frames


def noise_frame(w, h, seed=0):
    return np.random.default_rng(100 + seed).integers(0, 256, frame_bytes(w, h), dtype=np.uint8)


class DevBufs:
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


class SessionRig:
    """an EncoderSession with device buffers for one step of all slots and the entropy stage on"""

    def __init__(self, pkg, ctx, w, h, qualities, n):
        self.pkg, self.ctx, self.w, self.h, self.n = pkg, ctx, w, h, n
        self.enc = pkg.EncoderSession(ctx, w, h, None, n, qualities=qualities)
        self.tb = self.enc.total_blocks
        self.bufs = DevBufs(ctx)
        self.frames_dev = self.bufs.put(np.zeros(n * frame_bytes(w, h), np.uint8))
        self.mv_dev = self.bufs.put(np.zeros(n * self.tb * 2, np.int8))
        self.has_dev = self.bufs.put(np.zeros(n * self.tb, np.uint8))
        self.coef_dev = self.bufs.put(np.zeros(n * self.tb * 256, np.int16))
        self.enc.enable_entropy()

    def close(self):
        self.bufs.close()
        self.enc.close()

    def step(self, frames, pframe, rung=None):
        """-> dict(coef, mv, has, payloads, prev) of all slots after encoding `frames` [n, frame_bytes]"""
        enc, ctx, n, tb = self.enc, self.ctx, self.n, self.tb
        if rung is not None:
            enc.set_rung(rung)
        ctx.upload(self.frames_dev, np.ascontiguousarray(frames, dtype=np.uint8))
        out = {}
        if pframe:
            enc.encode_pframe_dev(self.frames_dev, self.mv_dev, self.has_dev, self.coef_dev)
            enc.pack_pframe_dev(self.mv_dev, self.has_dev, self.coef_dev)
            out["mv"], out["has"] = np.zeros((n, tb, 2), np.int8), np.zeros((n, tb), np.uint8)
            ctx.download(out["mv"], self.mv_dev)
            ctx.download(out["has"], self.has_dev)
        else:
            enc.encode_iframe_dev(self.frames_dev, self.coef_dev)
            enc.pack_iframe_dev(self.coef_dev)
        out["coef"] = np.zeros((n, tb, 256), np.int16)
        ctx.download(out["coef"], self.coef_dev)
        sizes = enc.payload_sizes()
        out["sizes"] = sizes
        out["payloads"] = [enc.payload(k, int(sizes[k])) for k in range(n)]
        prev = np.zeros((n, enc.padded_frame_bytes), np.uint8)
        for k in range(n):
            p = ctx._lib.pfv_enc_prev_frame_dev(enc.handle, k)
            assert p
            ctx.download(prev[k], int(p))
        out["prev"] = prev
        return out


# ------------------------------------------------------------------ check 1: session rungs
SESSION_PLAN = [("I", 3), ("P", 0), ("P", 4), ("I", 1), ("P", 1)]


def check_model_is_the_oracle_encoder(oracle, w=50, h=38, quality=5):
    """the model with a one-rung ladder is oracle.encoder(quality): coefficients, headers and prev_frame"""
    frames = motion_clip(w, h, 3, 3)
    m, o = LadderModel(oracle, w, h, [quality]), oracle.encoder(w, h, quality)
    assert np.array_equal(m.iframe(0, frames[0], 0), o.encode_iframe(frames[0])) and np.array_equal(m.prev_frame(0), o.prev_frame())
    for f in frames[1:]:
        got, want = m.pframe(0, f, 0), o.encode_pframe(f)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)) and np.array_equal(m.prev_frame(0), o.prev_frame())
        assert want[1].any() and want[0].any()               # coded macroblocks and motion vectors exist: not 0 == 0


def check_session_rungs(pkg, ctx, oracle, w, h, n, lane_mapping=None):
    L = pkg._lib
    old = ctx.get_option(L.PFV_OPT_LANE_MAPPING)
    if lane_mapping is not None:
        ctx.set_option(L.PFV_OPT_LANE_MAPPING, lane_mapping)
    rig = None
    try:
        rig = SessionRig(pkg, ctx, w, h, LADDER, n)
        assert rig.enc.n_rungs == len(LADDER) and rig.enc.rung == 0
        model = LadderModel(oracle, w, h, LADDER, n)
        clips = [motion_clip(w, h, 11 + k, len(SESSION_PLAN)) for k in range(n)]
        for t, (kind, rung) in enumerate(SESSION_PLAN):
            frames = np.stack([clips[k][t] for k in range(n)])
            got = rig.step(frames, kind == "P", rung)
            assert rig.enc.rung == rung
            for k in range(n):
                if kind == "I":
                    coef = model.iframe(k, frames[k], rung)
                    pay = model.payload_i(coef, rung)
                else:
                    mv, has, coef = model.pframe(k, frames[k], rung)
                    assert np.array_equal(got["mv"][k], mv) and np.array_equal(got["has"][k], has), (t, k)
                    pay = model.payload_p(mv, has, coef, rung)
                assert np.array_equal(got["coef"][k], coef), (t, k)
                assert np.array_equal(got["prev"][k], model.prev_frame(k)), (t, k)
                assert got["payloads"][k] == pay, (t, k, len(got["payloads"][k]), len(pay))
                assert tuple(pay[16:19]) == model.qidx(rung, kind == "P")
    finally:
        if rig:
            rig.close()
        ctx.set_option(L.PFV_OPT_LANE_MAPPING, old)


# ------------------------------------------------------------------ check 3: the stream object
def run_encoder(pkg, ctx, w, h, frames, plan, device_entropy, qualities=None, quality=None, rate=None, search=None):
    """plan: per frame ('I' | 'P' | 'D', rung or None) -> (stream bytes, rung after every frame); search: (mode, radius) of set_motion_search"""
    buf = io.BytesIO()
    enc = pkg.Encoder(buf, w, h, 30, quality, ctx, device_entropy=device_entropy, qualities=qualities)
    rungs = []
    try:
        if search:
            enc.set_motion_search(*search)
        if rate:
            enc.set_rate(rate)
        for f, (kind, rung) in zip(frames, plan):
            if rung is not None:
                enc.set_rung(rung)
            if kind == "D":
                enc.encode_dropframe()
            elif kind == "I":
                enc.encode_iframe(pkg.VideoFrame.from_packed(w, h, f))
            else:
                enc.encode_pframe(pkg.VideoFrame.from_packed(w, h, f))
            rungs.append(enc.rung)
        enc.finish()
    finally:
        enc.close()
    return buf.getvalue(), rungs


def model_stream(model, frames, plan):
    """the StreamBuilder stream of the plan and what a decoder shows after every packet"""
    sb = model.builder()
    shown = []
    for f, (kind, rung) in zip(frames, plan):
        if kind == "D":
            sb.drop()
        elif kind == "I":
            sb.iframe(model.iframe(0, f, rung), model.qidx(rung, False))
        else:
            mv, has, coef = model.pframe(0, f, rung)
            sb.pframe(mv, has, coef, model.qidx(rung, True))
        shown.append(None if kind == "D" else model.shown(0))
    return sb.bytes(), shown


def decode_both(pkg, ctx, oracle, data):
    """frames of the product's pfv_decoder and of the oracle's stream decoder (the oracle's: None where an advance delivers none)"""
    from oracle_bind import OracleStreamDecoder
    dec = pkg.Decoder(io.BytesIO(data), ctx)
    got = []
    while dec.advance_frame(lambda fr: got.append(fr.packed())):
        pass
    dec.close()
    odec = OracleStreamDecoder(oracle, data)
    want = []
    while True:
        rc, fr = odec.advance_frame()
        assert rc >= 0
        if rc == 0:
            break
        want.append(fr)
    return got, want


def check_encoder_ladder(pkg, ctx, oracle, device_entropy, w=50, h=38):
    plan = [("I", 3), ("P", 0), ("D", None), ("P", 4), ("I", 1), ("P", None), ("P", 2)]
    frames = motion_clip(w, h, 41, len(plan))
    data, rungs = run_encoder(pkg, ctx, w, h, frames, plan, device_entropy, qualities=LADDER)
    assert rungs == [3, 0, 0, 4, 1, 1, 2]                              # of the last frame written; a drop frame leaves it alone
    full = [(kind, r if r is not None or kind == "D" else rungs[t]) for t, (kind, r) in enumerate(plan)]
    model = LadderModel(oracle, w, h, LADDER)
    want, shown = model_stream(model, frames, full)
    assert data == want, (len(data), len(want))
    got, ofr = decode_both(pkg, ctx, oracle, data)
    assert len(ofr) == len(plan)
    for t, (s, o) in enumerate(zip(shown, ofr)):
        if s is not None:
            assert o is not None and np.array_equal(o, s), t
    assert len(got) == len([o for o in ofr if o is not None]) and all(np.array_equal(a, b) for a, b in zip(got, [o for o in ofr if o is not None]))


def check_one_rung_is_todays_encoder(pkg, ctx, oracle, w=50, h=38, quality=5):
    from oracle_bind import OracleStreamEncoder
    check_model_is_the_oracle_encoder(oracle, w, h, quality)      # the reference model itself, at one rung, is the oracle's encoder
    frames = motion_clip(w, h, 43, 3)
    plan = [("I", None), ("P", None), ("P", None)]
    for device_entropy in (True, False):
        a, _ = run_encoder(pkg, ctx, w, h, frames, plan, device_entropy, quality=quality)
        b, rungs = run_encoder(pkg, ctx, w, h, frames, plan, device_entropy, qualities=[quality])
        assert a == b and rungs == [0, 0, 0]
        so = OracleStreamEncoder(oracle, w, h, 30, quality)
        so.encode_iframe(frames[0]); so.encode_pframe(frames[1]); so.encode_pframe(frames[2]); so.finish()
        assert a == so.bytes()


# ------------------------------------------------------------------ check 4: the rate controller
def model_rate_run(oracle, w, h, frames, start_rung, budget_p):
    """the controller on the model: frame 0 is I at start_rung, the rest P -> (stream bytes, rung of every frame, payload sizes)"""
    model = LadderModel(oracle, w, h, RATE_LADDER)
    K = len(RATE_LADDER)
    sb = model.builder()
    rung, rungs, sizes = start_rung, [], []
    for t, f in enumerate(frames):
        if t == 0:
            sb.iframe(model.iframe(0, f, rung), model.qidx(rung, False))
            n = len(sb.parts[-1]) - 5
        else:
            mv, has, coef = model.pframe(0, f, rung)
            sb.pframe(mv, has, coef, model.qidx(rung, True))
            n = len(sb.parts[-1]) - 5
        rungs.append(rung)
        sizes.append(n)
        if t and budget_p:
            if n > budget_p:
                rung = min(rung + 1, K - 1)
            elif 2 * n <= budget_p:
                rung = max(rung - 1, 0)
    return sb.bytes(), rungs, sizes


def rate_budget(oracle, w, h, frames):
    """pframe_budget: 1.25 x the model's size of frame 1 as a p-frame at rung 2 behind frame 0 as an i-frame at rung 2"""
    model = LadderModel(oracle, w, h, RATE_LADDER)
    model.iframe(0, frames[0], 2)
    return int(1.25 * len(model.payload_p(*model.pframe(0, frames[1], 2), 2)))


def check_rate_controller(pkg, ctx, oracle, w, h, device_entropy=True):
    frames = rate_clip(w, h)
    K = len(RATE_LADDER)
    bp = rate_budget(oracle, w, h, frames)
    want, rungs, sizes = model_rate_run(oracle, w, h, frames, 2, bp)
    print(f"rate model {w}x{h}: budget {bp}, rungs {rungs}, payload bytes {sizes}")
    # of the MODEL first: the clip exercises the controller
    steps = np.diff(rungs)
    assert (steps > 0).any() and (steps < 0).any(), "the rung has to move coarser at least once and finer at least once"
    assert any(r == K - 1 and n > bp for r, n in zip(rungs[1:], sizes[1:])), "never clamped at the coarsest rung"
    plan = [("I", 2)] + [("P", None)] * (len(frames) - 1)
    data, got_rungs = run_encoder(pkg, ctx, w, h, frames, plan, device_entropy, qualities=RATE_LADDER, rate=bp)
    assert got_rungs == rungs, (got_rungs, rungs)
    assert data == want
    # budget off: the rung stays where it was set
    want, rungs, _ = model_rate_run(oracle, w, h, frames[:6], 2, 0)
    data, got_rungs = run_encoder(pkg, ctx, w, h, frames[:6], plan[:6], device_entropy, qualities=RATE_LADDER, rate=0)
    assert got_rungs == rungs == [2] * 6 and data == want


# ------------------------------------------------------------------ check 5: arguments
def check_arguments(pkg, ctx, w=50, h=38):
    L, lib = pkg._lib, ctx._lib
    BAD, STATE = L.PFV_ERR_BAD_ARG, L.PFV_ERR_STATE
    ints = lambda v: (ctypes.c_int * max(len(v), 1))(*v)      # noqa: E731
    fb = frame_bytes(w, h)
    frame = noise_frame(w, h)
    P = ctypes.c_void_p
    for make in ("session", "encoder"):
        def create(q, n, out=True):
            hdl = P()
            ref = ctypes.byref(hdl) if out else None
            if make == "session":
                return lib.pfv_enc_session_create_ladder(ctx.handle, w, h, ints(q) if q is not None else None, n, 1, ref), hdl
            return lib.pfv_encoder_create_ladder(ctx.handle, w, h, 30, ints(q) if q is not None else None, n, ref), hdl
        for q, n in (([], 0), (list(range(11)) + [10], 12), ([3, 3], 2), ([5, 2], 2), ([1, 11], 2), ([-1, 2], 2), (None, 2)):
            rc, hdl = create(q, n)
            assert rc == BAD and not hdl.value, (make, q, n, rc)
        assert create([1, 2], 2, out=False)[0] == BAD
    # a session stays usable after every refused call
    s = pkg.EncoderSession(ctx, w, h, None, 1, qualities=[1, 4, 9])
    try:
        for r in (-1, 3, 100):
            assert lib.pfv_enc_session_set_rung(s.handle, r) == BAD and s.rung == 0
        assert lib.pfv_enc_session_set_rung(None, 0) == BAD and lib.pfv_enc_session_rung(None) == BAD and lib.pfv_enc_session_rungs(None) == BAD
        s.set_rung(2)
        coef = s.encode_iframe(frame)
        assert coef.any()
    finally:
        s.close()
    # a ladder under the integer transform (PFV_OPT_ENC_TRANSFORM): same coefficients as the float session at every rung
    L_ = pkg._lib
    old = ctx.get_option(L_.PFV_OPT_ENC_TRANSFORM)
    ctx.set_option(L_.PFV_OPT_ENC_TRANSFORM, L_.PFV_ENC_TRANSFORM_INT)
    try:
        s = pkg.EncoderSession(ctx, w, h, None, 1, qualities=[1, 4, 9])
    finally:
        ctx.set_option(L_.PFV_OPT_ENC_TRANSFORM, old)
    ref = pkg.EncoderSession(ctx, w, h, None, 1, qualities=[1, 4, 9])
    try:
        for r in range(3):
            s.set_rung(r); ref.set_rung(r)
            assert np.array_equal(s.encode_iframe(frame), ref.encode_iframe(frame)), r
    finally:
        s.close()
        ref.close()
    buf = io.BytesIO()
    e = pkg.Encoder(buf, w, h, 30, None, ctx, qualities=[1, 4, 9])
    try:
        for r in (-1, 3):
            assert lib.pfv_encoder_set_rung(e.handle, r) == BAD and e.rung == 0
        assert lib.pfv_encoder_set_rung(None, 0) == BAD and lib.pfv_encoder_rung(None) == BAD and lib.pfv_encoder_rungs(None) == BAD
        assert lib.pfv_encoder_set_rate(None, 0) == BAD
        e.set_rung(2)
        e.encode_iframe(pkg.VideoFrame.from_packed(w, h, frame))
        assert e.rung == 2 and e.n_rungs == 3
        assert fb == frame.size
    finally:
        e.close()


# ------------------------------------------------------------------ check 6: the C++ mirror
def build_cpp(lib_path, exe):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "ladder_rate.cpp"), "-o", exe, lib_path, "-Wl,-rpath," + os.path.dirname(lib_path)], check=True)


def check_cpp_rate(pkg, ctx, oracle, exe, tmp_path, w=64, h=48):
    """tests/cpp/ladder_rate.cpp (pfv::Encoder with a ladder, set_rung, set_rate, rung) encodes the rate clip: same bytes, same rungs"""
    frames = rate_clip(w, h)
    bp = rate_budget(oracle, w, h, frames)
    plan = [("I", 2)] + [("P", None)] * (len(frames) - 1)
    data, rungs = run_encoder(pkg, ctx, w, h, frames, plan, True, qualities=RATE_LADDER, rate=bp)
    yuv, out = str(tmp_path / "rate.yuv"), str(tmp_path / "rate.pfv")
    np.concatenate(frames).tofile(yuv)
    r = subprocess.run([exe, str(w), str(h), ",".join(str(q) for q in RATE_LADDER), "2", str(bp), yuv, out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert [int(x) for x in r.stdout.splitlines()[0].split()[1:]] == rungs
    assert open(out, "rb").read() == data
