"""Shared checks of the SSIM probes (pfv_enc_probe_iframe_ssim*, pfv_enc_probe_pframe_ssim*, pfv_encoder_probe_*frame_ssim), pfv_encoder's SSIM
floors (pfv_encoder_set_iframe_ssim_floor / _set_pframe_ssim_floor) and the frame type they give pfv_encoder_encode_frame (include/pfv_hip_ext.h,
"SSIM probe"), driven on the CPU emulator by tests/test_emu_ssimprobe.py and on a real MI355X by tests/test_gpu_ssimprobe.py at the same small
shapes.

Every expectation comes from the oracles, never from the code under test: sizes and counts are probe_cases.expected / pprobe_cases.facts, the
squared error rdprobe_cases.expected_sse / prdprobe_cases.pframe_sse, and SSIM is ssim_cases.ref_ssim(frame, crop of LadderModel's reconstruction
at rung r) on a copy of the model's state.  Two kinds of SSIM comparison, both ssim_cases.py's rule: against numpy the derived tolerance
|q24 sum - reference| <= 16.5 x windows of the plane (the worst figure is printed); against the shipped device path (pfv_enc_ssim_dev behind a
real encode at rung r, pfv_encoder_frame_ssim of the frame then written at r) equality -- both run the same window function on the same integers.

The floors compare a mean SSIM with a threshold: the model's is float64, the device's the rounded integers, at most 16.5 / 2^24 = 1e-6 apart per
window.  So "just met" / "just missed" sit 4e-6 from a model value, and every case first asserts on the model that no other allowed rung lies
within 2e-6 of the floor; where "largest q24" decides, that the top two are identical reconstructions or more than 2e-6 apart."""
import copy
import ctypes
import io
import math
import os
import subprocess

import numpy as np
import pytest

import ladder_cases as lc
import pprobe_cases as pp
import prdprobe_cases as prd
import probe_cases as pc
import rdprobe_cases as rc
import ssim_cases as sc
from ladder_cases import LADDER, DevBufs, LadderModel, frame_bytes, plane_dims
from pprobe_cases import CODED, FRAME_NAMES, MOVED, clips, state_frames
from probe_cases import FULL_LADDER, SENTINEL, content, frame_sets, options
from rdprobe_cases import NOT_ENCODABLE, SENTINEL64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the p-frame probes' shapes; 144x80: windows straddle the strip seam at x = 128 and the p-frame tile seam at y = 64; 8x8: one luma window, no
# chroma windows; 6x6: no window at all
SHAPES = pp.SHAPES + [(144, 80, 1), (8, 8, 1), (6, 6, 1)]
QSENTINEL = sc.SUM_SENTINEL
ONE = sc.ONE
NEAR, STEP = 2e-6, 4e-6


# ------------------------------------------------------------------ the reference
def crop(planes, w, h):
    return np.concatenate([p[:ph, :pw].reshape(-1) for p, (pw, ph) in zip(planes, plane_dims(w, h))])


def n_windows(w, h):
    return int(sum(sc.windows_of(w, h)))


_ISSIM = {}


def iframe_ssim(oracle, w, h, qualities, frame):
    """(float64 [R, 3] in units of 2^-24, [R] reconstructions packed): SSIM sums per plane of the frame against its i-frame reconstruction at
    every rung"""
    key = (w, h, tuple(qualities), frame.tobytes())
    if key not in _ISSIM:
        model = LadderModel(oracle, w, h, qualities)
        recs = [crop(model.iframe_coef(frame, r)[1], w, h) for r in range(len(qualities))]
        _ISSIM[key] = (np.stack([sc.ref_ssim(frame, rec, w, h)[0] for rec in recs]), recs)
    return _ISSIM[key]


def iframe_ssim_many(oracle, w, h, qualities, frames):
    return np.stack([iframe_ssim(oracle, w, h, qualities, f)[0] for f in frames])


def pframe_ssim(model, k, frame):
    """the same as a p-frame against the model's prev of stream k, which is not touched (as prdprobe_cases.pframe_sse)"""
    sums, recs = [], []
    for r in range(len(model.qualities)):
        m = copy.copy(model)
        m.prev = [list(p) for p in model.prev]
        m.pframe(k, frame, r)
        recs.append(crop(m.prev[k], model.w, model.h))
        sums.append(sc.ref_ssim(frame, recs[-1], model.w, model.h)[0])
    return np.stack(sums), recs


_PSSIM = {}


def ssim_facts(oracle, w, h, qualities, n, state, sets=None):
    """per frame set of state_frames (all, or those named by `sets`: None elsewhere): (q float64 [n, R, 3], recs [n][R]); computed once per
    (shape, ladder, state)"""
    key = (w, h, tuple(qualities), n, state, None if sets is None else tuple(sets))
    if key not in _PSSIM:
        model = pp.model_in_state(oracle, w, h, qualities, n, state)
        out = []
        for t, frames in enumerate(state_frames(w, h, n, state)):
            if sets is not None and t not in sets:
                out.append(None)
                continue
            per = [pframe_ssim(model, k, frames[k]) for k in range(n)]
            out.append((np.stack([p[0] for p in per]), [p[1] for p in per]))
        _PSSIM[key] = out
    return _PSSIM[key]


def assert_q24(got, want, w, h, what):
    """the derived tolerance per plane, the worst figure printed first; a plane without windows reports exactly 0"""
    assert got.dtype == np.int64 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    nw = np.array(sc.windows_of(w, h), dtype=np.float64)
    err = np.abs(got.astype(np.float64) - want)
    print(f"ssim probe {what} {w}x{h}: worst plane-sum error per window {np.max(err / np.maximum(nw, 1)):.3f} (bound {sc.TOL})")
    assert (err <= sc.TOL * nw).all(), (what, got.tolist(), want.tolist())


def mean_ssim(qtot, w, h):
    return float(qtot) / (ONE * n_windows(w, h))


# ------------------------------------------------------------------ check 1: what the inputs exercise (the oracle alone)
def gradient(w=50, h=38):
    return content(w, h, "gradient", seed=0)


def check_inputs_cover(oracle, w=50, h=38, n=3):
    # the gradient i-frame: SSIM and PSNR-YUV rank rungs 2 and 3 in opposite order, and SSIM is not monotone over the ladder
    g = gradient(w, h)
    s = [mean_ssim(x, w, h) for x in iframe_ssim(oracle, w, h, LADDER, g)[0].sum(axis=1)]
    q = rc.psnr_yuv(oracle, w, h, LADDER, g)
    sizes = pc.expected(oracle, w, h, LADDER, g)[0].tolist()
    print(f"gradient i-frame {w}x{h}: sizes {sizes} psnr {[round(x, 2) for x in q]} ssim {[round(x, 5) for x in s]}")
    assert s[3] > s[2] and q[3] < q[2] and sizes[3] < sizes[2]
    assert any(b > a for a, b in zip(s, s[1:])) and any(b < a for a, b in zip(s, s[1:]))
    still_lossy = identical = 0
    for state in (0, 1):
        for (_, _, hass, _), (qs, recs) in zip(pp.facts(oracle, w, h, LADDER, n, state), ssim_facts(oracle, w, h, LADDER, n, state)):
            for k in range(n):
                for r in range(len(LADDER)):
                    still_lossy += int(not hass[k][r].any() and mean_ssim(qs[k][r].sum(), w, h) < 1.0 - 1e-4)
                    identical += int(r > 0 and np.array_equal(recs[k][r], recs[k][r - 1]))
    print(f"ssim probe inputs {w}x{h}x{n}: (frame, rung) pairs with nothing coded and SSIM below 1: {still_lossy}; neighbouring rungs with identical "
          f"reconstructions: {identical}")
    assert still_lossy and identical


# ------------------------------------------------------------------ check 2: the session probes
class ISsimRig(rc.RdRig):
    """RdRig with a device buffer for the SSIM sums; fetch() -> (sizes, stats, sse, q24)"""

    def __init__(self, pkg, ctx, w, h, qualities, n, stride=0):
        super().__init__(pkg, ctx, w, h, qualities, n, stride)
        self.q_dev = self.bufs.put(np.zeros((n, self.R, 3), np.int64))

    def sentinels(self):
        super().sentinels()
        self.ctx.upload(self.q_dev, np.full((self.n, self.R, 3), QSENTINEL, np.int64))

    def fetch(self):
        sizes, stats, sse = super().fetch()
        q = np.zeros((self.n, self.R, 3), np.int64)
        self.ctx.download(q, self.q_dev)
        return sizes, stats, sse, q

    def probe(self, frames, stats=True):
        self.upload(frames)
        self.sentinels()
        self.enc.probe_iframe_ssim_dev(self.frames_dev, self.sizes_dev, self.sse_dev, self.q_dev, self.stats_dev if stats else 0)
        return self.fetch()

    def rd_probe(self, frames):
        return rc.RdRig.probe(self, frames)


class PSsimRig(prd.PRdRig):
    """PRdRig with a device buffer for the SSIM sums; fetch() -> (sizes, stats, sse, q24)"""

    def __init__(self, pkg, ctx, w, h, qualities, n, stride=0):
        super().__init__(pkg, ctx, w, h, qualities, n, stride)
        self.q_dev = self.bufs.put(np.zeros((n, self.R, 3), np.int64))

    def upload(self, frames):
        super().upload(frames)
        self.ctx.upload(self.q_dev, np.full((self.n, self.R, 3), QSENTINEL, np.int64))

    def fetch(self):
        sizes, stats, sse = super().fetch()
        q = np.zeros((self.n, self.R, 3), np.int64)
        self.ctx.download(q, self.q_dev)
        return sizes, stats, sse, q

    def probe(self, frames, stats=True):
        self.upload(frames)
        self.enc.probe_pframe_ssim_dev(self.probe_dev, self.sizes_dev, self.sse_dev, self.q_dev, self.stats_dev if stats else 0)
        return self.fetch()

    def rd_probe(self, frames):
        return prd.PRdRig.probe(self, frames)


def check_iframe_session_probe(pkg, ctx, oracle, w, h, n, lane_mapping=None, int_transform=False, qualities=LADDER, sets=None):
    """sizes, counts, plane sums and SSIM sums of every frame set at every rung; once without the counts and through the host-buffer form"""
    with options(pkg, ctx, lane_mapping, int_transform):
        rig = ISsimRig(pkg, ctx, w, h, qualities, n)
    try:
        all_sets = frame_sets(w, h, n)
        for t, frames in enumerate(all_sets if sets is None else [all_sets[i] for i in sets]):
            want_sizes, want_stats, want_sse = rc.expected_many(oracle, w, h, qualities, frames)
            want_q = iframe_ssim_many(oracle, w, h, qualities, frames)
            sizes, stats, sse, q = rig.probe(frames)
            assert np.array_equal(stats, want_stats), (t, np.argwhere(stats != want_stats)[:4].tolist())
            assert np.array_equal(sizes, want_sizes), (t, sizes.tolist(), want_sizes.tolist())
            assert np.array_equal(sse, want_sse), (t, np.argwhere(sse != want_sse)[:4].tolist(), sse.tolist(), want_sse.tolist())
            assert_q24(q, want_q, w, h, f"i-frame set {t}")
        sizes, stats, sse, q2 = rig.probe(frames, stats=False)
        assert np.array_equal(sizes, want_sizes) and np.array_equal(sse, want_sse) and (stats == SENTINEL).all() and np.array_equal(q2, q)
        sizes, sse, q3 = rig.enc.probe_iframe_ssim(frames)
        assert np.array_equal(sizes, want_sizes) and np.array_equal(sse, want_sse) and np.array_equal(q3, q)
        assert rig.enc.rung == 0
    finally:
        rig.close()


def check_session_probe(pkg, ctx, oracle, w, h, n, int_transform=False, qualities=LADDER, sets=None):
    """real session calls make the states: i-frame at rung 1, probe, p-frame at rung 2, probe again.  Sizes, all 20 counts, the plane sums and the
    SSIM sums of every frame set (or of those named by `sets`, which include 1) at every rung; once without the counts (stats_dev = NULL); the
    host-buffer form agrees; the rung stays"""
    if (w, h, n) in pp.INTERIOR_SHAPES and tuple(qualities) == tuple(LADDER):
        pp.check_interior_inputs(oracle, w, h, n, sets)
    with options(pkg, ctx, None, int_transform):
        rig = PSsimRig(pkg, ctx, w, h, qualities, n)
    try:
        for state in (0, 1):
            cl = clips(w, h, n)
            rig.step(np.stack([c[state] for c in cl]), bool(state), 1 + state)
            fsets = state_frames(w, h, n, state)
            want, want_sse = pp.facts(oracle, w, h, qualities, n, state, sets), prd.sse_facts(oracle, w, h, qualities, n, state, sets)
            want_q = ssim_facts(oracle, w, h, qualities, n, state, sets)
            for t, frames in enumerate(fsets):
                if want[t] is None:
                    continue
                sizes, stats, sse, q = rig.probe(frames)
                assert np.array_equal(stats, want[t][1]), (state, FRAME_NAMES[t], np.argwhere(stats != want[t][1])[:4].tolist())
                assert np.array_equal(sizes, want[t][0]), (state, FRAME_NAMES[t], sizes.tolist(), want[t][0].tolist())
                assert np.array_equal(sse, want_sse[t][0]), (state, FRAME_NAMES[t], sse.tolist(), want_sse[t][0].tolist())
                assert_q24(q, want_q[t][0], w, h, f"p-frame state {state} {FRAME_NAMES[t]}")
                if n_windows(w, h) == 0:
                    assert (q == 0).all()
                if t == 1:
                    q_pan = q
            sizes, stats, sse, q = rig.probe(fsets[1], stats=False)
            assert np.array_equal(sizes, want[1][0]) and np.array_equal(sse, want_sse[1][0]) and (stats == SENTINEL).all() and np.array_equal(q, q_pan)
            sizes, sse, q = rig.enc.probe_pframe_ssim(fsets[1])
            assert np.array_equal(sizes, want[1][0]) and np.array_equal(sse, want_sse[1][0]) and np.array_equal(q, q_pan)
            assert rig.enc.rung == 1 + state
    finally:
        rig.close()


# ------------------------------------------------------------------ check 3: agreement with the shipped paths
def check_agrees_with_rd_probes(pkg, ctx, oracle, w=50, h=38, n=3):
    """sizes, counts and plane sums equal the rate-distortion probes' on the same frames (which leave the SSIM sums alone)"""
    irig = ISsimRig(pkg, ctx, w, h, LADDER, n)
    try:
        for frames in frame_sets(w, h, n)[:2]:
            sizes, stats, sse, _ = irig.probe(frames)
            sizes2, stats2, sse2, q2 = irig.rd_probe(frames)
            assert np.array_equal(sizes, sizes2) and np.array_equal(stats, stats2) and np.array_equal(sse, sse2) and (q2 == QSENTINEL).all()
            assert np.array_equal(sizes, pc.expected_many(oracle, w, h, LADDER, frames)[0])
    finally:
        irig.close()
    rig = PSsimRig(pkg, ctx, w, h, LADDER, n)
    try:
        for state in (0, 1):
            rig.step(np.stack([c[state] for c in clips(w, h, n)]), bool(state), 1 + state)
            for t in (1, 3, 6):
                frames = state_frames(w, h, n, state)[t]
                sizes, stats, sse, _ = rig.probe(frames)
                sizes2, stats2, sse2, q2 = rig.rd_probe(frames)
                assert np.array_equal(sizes, sizes2) and np.array_equal(stats, stats2) and np.array_equal(sse, sse2) and (q2 == QSENTINEL).all()
    finally:
        rig.close()


def check_equals_encoded_ssim(pkg, ctx, oracle, w, h, n):
    """the probe's q24 of rung r == what pfv_enc_ssim_dev returns behind a real session encode of the same frames at rung r, for i-frames and
    for p-frames behind the same i-frame: equality"""
    rig = PSsimRig(pkg, ctx, w, h, LADDER, n)
    irig = ISsimRig(pkg, ctx, w, h, LADDER, n)
    out_dev = rig.bufs.put(np.zeros((n, 3), np.int64))
    try:
        base = np.stack([c[0] for c in clips(w, h, n)])
        for t in (1, 3, 6):                                             # pan1, checker, texture
            frames = state_frames(w, h, n, 0)[t]
            rig.step(base, False, 1)
            _, _, _, pq = rig.probe(frames)
            _, _, _, iq = irig.probe(frames)
            for r in range(len(LADDER)):
                for pframe, q in ((True, pq), (False, iq)):
                    rig.step(base, False, 1)
                    rig.step(frames, pframe, r)
                    got = np.zeros((n, 3), np.int64)
                    rig.enc.ssim_dev(rig.frames_dev, out_dev)
                    ctx.download(got, out_dev)
                    assert np.array_equal(q[:, r], got), (FRAME_NAMES[t], r, pframe, q[:, r].tolist(), got.tolist())
    finally:
        irig.close()
        rig.close()


def check_probe_is_what_the_encoder_writes(pkg, ctx, oracle, device_entropy, w=50, h=38):
    """pfv_encoder with frame reports and frame SSIM: the probed (size, sse, q24) of rung r == (packet_bytes - 5, sse, q24) of the frame then
    encoded at rung r, as an i-frame and as a p-frame behind the same i-frame"""
    base = clips(w, h, 1)[0][0]
    fsets = state_frames(w, h, 1, 0)
    want, want_sse = pp.facts(oracle, w, h, LADDER, 1, 0), prd.sse_facts(oracle, w, h, LADDER, 1, 0)
    enc = pkg.Encoder(io.BytesIO(), w, h, 30, None, ctx, device_entropy=device_entropy, frame_report=True, frame_ssim=True, qualities=LADDER)
    try:
        for t in (1, 6):                                                # pan1, texture
            f = fsets[t][0]
            vf = pkg.VideoFrame.from_packed(w, h, f)
            for r in range(len(LADDER)):
                enc.set_rung(1)
                enc.encode_iframe(pkg.VideoFrame.from_packed(w, h, base))
                sizes, sse, q = enc.probe_pframe_ssim(vf)
                assert np.array_equal(sizes, want[t][0][0]) and np.array_equal(sse, want_sse[t][0][0]) and enc.rung == 1
                enc.set_rung(r)
                enc.encode_pframe(vf)
                rep, ss = enc.last_report, enc.last_ssim
                assert enc.rung == r and rep.type == 2 and rep.packet_bytes - 5 == int(sizes[r])
                assert [int(x) for x in rep.sse] == [int(x) for x in sse[r]] and [int(x) for x in ss.q24] == [int(x) for x in q[r]], (t, r)
                isizes, isse, iq = enc.probe_iframe_ssim(vf)
                assert np.array_equal(isizes, pc.expected(oracle, w, h, LADDER, f)[0]) and np.array_equal(isse, rc.expected_sse(oracle, w, h, LADDER, f))
                enc.encode_iframe(vf)
                rep, ss = enc.last_report, enc.last_ssim
                assert rep.type == 1 and rep.packet_bytes - 5 == int(isizes[r])
                assert [int(x) for x in rep.sse] == [int(x) for x in isse[r]] and [int(x) for x in ss.q24] == [int(x) for x in iq[r]], (t, r)
    finally:
        enc.close()


# ------------------------------------------------------------------ check 4: no side effects, window and stride, graph
def check_no_side_effects(pkg, ctx, oracle, w=50, h=38, n=3):
    """i-frame at rung 1, then a p-frame at rung 3: prev_frame, the pointers, the rung and every output of the p-frame are the model's whether or
    not SSIM probes of OTHER frames (both kinds, device form and host-buffer form) run in between"""
    cl = clips(w, h, n)
    other, want_other, sse_other = state_frames(w, h, n, 0)[5], pp.facts(oracle, w, h, LADDER, n, 0)[5], prd.sse_facts(oracle, w, h, LADDER, n, 0)[5]
    q_other = ssim_facts(oracle, w, h, LADDER, n, 0)[5][0]
    outs = []
    for with_probe in (False, True):
        rig = PSsimRig(pkg, ctx, w, h, LADDER, n)
        try:
            rig.step(np.stack([c[0] for c in cl]), False, 1)
            if with_probe:
                before = rig.enc.prev_frame()
                ptr_before = [ctx._lib.pfv_enc_prev_frame_dev(rig.enc.handle, k) for k in range(n)]
                sizes, stats, sse, q = rig.probe(other)
                assert np.array_equal(sizes, want_other[0]) and np.array_equal(stats, want_other[1]) and np.array_equal(sse, sse_other[0])
                assert_q24(q, q_other, w, h, "side effects")
                sizes, sse, q2 = rig.enc.probe_pframe_ssim(other)
                assert np.array_equal(sizes, want_other[0]) and np.array_equal(sse, sse_other[0]) and np.array_equal(q2, q)
                sizes, sse, q3 = rig.enc.probe_iframe_ssim(other)
                assert np.array_equal(sizes, pc.expected_many(oracle, w, h, LADDER, other)[0])
                assert_q24(q3, iframe_ssim_many(oracle, w, h, LADDER, other), w, h, "side effects, i-frame")
                assert rig.enc.rung == 1 and np.array_equal(rig.enc.prev_frame(), before)
                assert ptr_before == [ctx._lib.pfv_enc_prev_frame_dev(rig.enc.handle, k) for k in range(n)]
            outs.append(rig.step(np.stack([c[1] for c in cl]), True, 3))
        finally:
            rig.close()
    model = LadderModel(oracle, w, h, LADDER, n)
    for k in range(n):
        model.iframe(k, cl[k][0], 1)
        mv, has, coef = model.pframe(k, cl[k][1], 3)
        pay = model.payload_p(mv, has, coef, 3)
        for out in outs:
            assert np.array_equal(out["mv"][k], mv) and np.array_equal(out["has"][k], has) and np.array_equal(out["coef"][k], coef)
            assert np.array_equal(out["prev"][k], model.prev_frame(k)) and out["payloads"][k] == pay


def check_window_stride(pkg, ctx, oracle, w=50, h=38, n=3):
    """window (1, 2) with the frames frame_bytes + 48 apart: slots 1 and 2 right, the entries of slot 0 left at the sentinels (32- and 64-bit);
    the host form is refused under a window"""
    rig = PSsimRig(pkg, ctx, w, h, LADDER, n, stride=frame_bytes(w, h) + 48)
    irig = ISsimRig(pkg, ctx, w, h, LADDER, n, stride=frame_bytes(w, h) + 48)
    try:
        rig.to_state(1)
        for g in (rig, irig):
            g.enc.set_frame_stride(g.stride)
            g.enc.set_window(1, 2)
        fsets, want, want_sse = state_frames(w, h, n, 1), pp.facts(oracle, w, h, LADDER, n, 1), prd.sse_facts(oracle, w, h, LADDER, n, 1)
        want_q = ssim_facts(oracle, w, h, LADDER, n, 1)
        for t in (1, 4):
            sizes, stats, sse, q = rig.probe(fsets[t])
            assert (sizes[0] == SENTINEL).all() and (stats[0] == SENTINEL).all() and (sse[0] == SENTINEL64).all() and (q[0] == QSENTINEL).all()
            assert np.array_equal(sizes[1:], want[t][0][1:]) and np.array_equal(stats[1:], want[t][1][1:]) and np.array_equal(sse[1:], want_sse[t][0][1:])
            assert_q24(q[1:], want_q[t][0][1:], w, h, "window, p-frame")
            isz, ist, isse, iq = irig.probe(fsets[t])
            wsz, wst, wsse = rc.expected_many(oracle, w, h, LADDER, fsets[t])
            assert (isz[0] == SENTINEL).all() and (ist[0] == SENTINEL).all() and (isse[0] == SENTINEL64).all() and (iq[0] == QSENTINEL).all()
            assert np.array_equal(isz[1:], wsz[1:]) and np.array_equal(ist[1:], wst[1:]) and np.array_equal(isse[1:], wsse[1:])
            assert_q24(iq[1:], iframe_ssim_many(oracle, w, h, LADDER, fsets[t])[1:], w, h, "window, i-frame")
        for call in (rig.enc.probe_pframe_ssim, irig.enc.probe_iframe_ssim):
            with pytest.raises(pkg.PfvError) as e:                      # the host-buffer forms work on all slots, packed
                call(fsets[1])
            assert e.value.code == pkg._lib.PFV_ERR_STATE
        rig.enc.set_window(0, n)                                        # ... and the whole session again, still strided
        sizes, stats, sse, q = rig.probe(fsets[4])
        assert np.array_equal(sizes, want[4][0]) and np.array_equal(stats, want[4][1]) and np.array_equal(sse, want_sse[4][0])
        assert_q24(q, want_q[4][0], w, h, "window reset")
    finally:
        irig.close()
        rig.close()


def check_graph(pkg, ctx, oracle, w=50, h=38, n=3):
    """both launch groups recorded once and replayed on three contents: every replay right (nothing of the map or the accumulators needs a
    host-side clear); a session that has never probed is refused inside a recording"""
    rig = PSsimRig(pkg, ctx, w, h, LADDER, n)
    irig = ISsimRig(pkg, ctx, w, h, LADDER, n)
    fresh = pkg.EncoderSession(ctx, w, h, None, n, qualities=LADDER)
    graph, igraph = pkg.Graph(ctx), pkg.Graph(ctx)
    try:
        rig.to_state(0)
        fsets, want, want_sse = state_frames(w, h, n, 0), pp.facts(oracle, w, h, LADDER, n, 0), prd.sse_facts(oracle, w, h, LADDER, n, 0)
        want_q = ssim_facts(oracle, w, h, LADDER, n, 0)
        firsts = {}
        for t in (1, 5, 0, 2):                                          # unrecorded calls: they make the map and the accumulators, and the values
            firsts[t] = (rig.probe(fsets[t])[3], irig.probe(fsets[t])[3])
            assert_q24(firsts[t][0], want_q[t][0], w, h, f"graph, unrecorded {FRAME_NAMES[t]}")
        with graph:
            rig.enc.probe_pframe_ssim_dev(rig.probe_dev, rig.sizes_dev, rig.sse_dev, rig.q_dev, rig.stats_dev)
            for call in (fresh.probe_pframe_ssim_dev, fresh.probe_iframe_ssim_dev):
                with pytest.raises(pkg.PfvError) as e:
                    call(rig.probe_dev, rig.sizes_dev, rig.sse_dev, rig.q_dev)
                assert e.value.code == pkg._lib.PFV_ERR_STATE and "before pfv_graph_begin" in str(e.value)
        with igraph:
            irig.enc.probe_iframe_ssim_dev(irig.frames_dev, irig.sizes_dev, irig.sse_dev, irig.q_dev, irig.stats_dev)
        for t in (5, 0, 2):
            rig.upload(fsets[t])
            graph.launch()
            sizes, stats, sse, q = rig.fetch()
            assert np.array_equal(stats, want[t][1]) and np.array_equal(sizes, want[t][0]) and np.array_equal(sse, want_sse[t][0]), FRAME_NAMES[t]
            assert np.array_equal(q, firsts[t][0]), FRAME_NAMES[t]
            irig.upload(fsets[t])
            irig.sentinels()
            igraph.launch()
            isz, ist, isse, iq = irig.fetch()
            wsz, wst, wsse = rc.expected_many(oracle, w, h, LADDER, fsets[t])
            assert np.array_equal(isz, wsz) and np.array_equal(ist, wst) and np.array_equal(isse, wsse) and np.array_equal(iq, firsts[t][1])
    finally:
        graph.close()
        igraph.close()
        fresh.close()
        irig.close()
        rig.close()


# ------------------------------------------------------------------ the encoder's rules on the model
def choose_rung(sizes, tot, qtot, budget, floor_db, floor_ssim, w, h):
    """the floors' rule on sizes [K], total squared errors [K] and total SSIM sums [K] (float64, units of 2^-24)"""
    K = len(sizes)
    sizes, tot = [int(x) for x in sizes], [int(x) for x in tot]
    allowed = [r for r in range(K) if sizes[r] != NOT_ENCODABLE and (not budget or sizes[r] <= budget)]
    if not allowed:
        return K - 1
    nw = n_windows(w, h)

    def meets(r):
        return (not floor_db or prd.psnr_yuv(tot[r], w, h) >= floor_db) and (not floor_ssim or nw == 0 or mean_ssim(qtot[r], w, h) >= floor_ssim)
    m = [r for r in allowed if meets(r)]
    if m:
        return min(m, key=lambda r: (sizes[r], r))
    if floor_ssim and nw:
        return min(allowed, key=lambda r: (-qtot[r], tot[r], sizes[r], r))
    return min(allowed, key=lambda r: (tot[r], sizes[r], r))


class SsimEncoderModel(prd.RdEncoderModel):
    """prdprobe_cases.RdEncoderModel with the two SSIM floors; with both at 0 it is that model"""

    def __init__(self, oracle, w, h, qualities, sfloor_p=0.0, sfloor_i=0.0, **kw):
        super().__init__(oracle, w, h, qualities, **kw)
        self.sfloor_p, self.sfloor_i = sfloor_p, sfloor_i
        self.pss = []                                                   # (sizes, squared errors, SSIM sums) of every p-frame the SSIM floor probed

    def pfloor(self):
        return (self.floor_p > 0 or self.sfloor_p > 0) and self.K > 1

    def p_q(self, f):
        return pframe_ssim(self.model, 0, f)[0].sum(axis=1)

    def i_q(self, f):
        return iframe_ssim(self.o, self.w, self.h, self.q, f)[0].sum(axis=1)

    def iframe_rung(self, f):
        if self.K == 1 or not self.sfloor_i > 0:
            return super().iframe_rung(f)
        sizes, tot = self.i_rd(f)
        return choose_rung(sizes, tot, self.i_q(f), self.budget_i, self.floor_i, self.sfloor_i, self.w, self.h)

    def iframe(self, f):
        self.rung = self.iframe_rung(f)
        saved = (self.budget_i, self.floor_i, self.sfloor_i)
        self.budget_i, self.floor_i, self.sfloor_i = 0, 0.0, 0.0       # the rung is settled
        try:
            return pp.EncoderModel.iframe(self, f)
        finally:
            self.budget_i, self.floor_i, self.sfloor_i = saved

    def pframe(self, f, rung_settled=False):
        if not (self.pfloor() and self.sfloor_p > 0):
            return super().pframe(f, rung_settled)
        if not rung_settled:
            sizes, _, tot = self.p_rd(f)
            q = self.p_q(f)
            self.pss.append((sizes, tot, q))
            self.rung = choose_rung(sizes, tot, q, self.budget_p, self.floor_p, self.sfloor_p, self.w, self.h)
        pprobe, self.pprobe = self.pprobe, True                         # no soft rule under the floor
        try:
            return pp.EncoderModel.pframe(self, f, rung_settled=True)
        finally:
            self.pprobe = pprobe

    def frame(self, f):
        """pfv_encoder_encode_frame -> (type, why); with the p-frame SSIM floor on rule 4 weighs the candidates by both p-frame floors"""
        if not self.pfloor():
            return pp.EncoderModel.frame(self, f)
        if self.n_written == 0 or (self.gop > 0 and self.since_i >= self.gop):
            return self.iframe(f), "forced"
        w, h = self.w, self.h
        psize, stats, ptot = self.p_rd(f)
        pq = self.p_q(f)
        rp = choose_rung(psize, ptot, pq, self.budget_p, self.floor_p, self.sfloor_p, w, h)
        if stats[rp][CODED] == 0 and stats[rp][MOVED] == 0:
            return self.drop(), "still"
        isize, itot = self.i_rd(f)
        iq = self.i_q(f)
        ri = self.iframe_rung(f)
        pb, ib, pe, ie, ps, is_ = int(psize[rp]), int(isize[ri]), int(ptot[rp]), int(itot[ri]), float(pq[rp]), float(iq[ri])
        assert pb != NOT_ENCODABLE and ib != NOT_ENCODABLE
        nw = n_windows(w, h)

        def meets(e, s):
            return (not self.floor_p > 0 or prd.psnr_yuv(e, w, h) >= self.floor_p) and (not self.sfloor_p > 0 or nw == 0 or mean_ssim(s, w, h) >= self.sfloor_p)
        pm, im = meets(pe, ps), meets(ie, is_)
        self.last_pair = (pm, im, mean_ssim(ps, w, h), mean_ssim(is_, w, h)) if nw and self.sfloor_p > 0 else None
        if pm != im:
            take_i, why = im, "only i" if im else "only p"
        elif pm:
            take_i = ib <= pb
            why = "both, i" if take_i else "both, p"
        else:
            take_i = (-is_, ie, ib) <= (-ps, pe, pb) if nw and self.sfloor_p > 0 else (ie, ib) <= (pe, pb)
            why = "neither, i" if take_i else "neither, p"
        if take_i:
            self.rung = ri
            saved = (self.budget_i, self.floor_i, self.sfloor_i)
            self.budget_i, self.floor_i, self.sfloor_i = 0, 0.0, 0.0   # the rung is settled
            try:
                return self.iframe(f), why
            finally:
                self.budget_i, self.floor_i, self.sfloor_i = saved
        self.rung = rp
        return self.pframe(f, rung_settled=True), why


def run_encoder(pkg, ctx, w, h, frames, plan, device_entropy, qualities=None, quality=None, rung=None, budget_p=0, budget_i=0, pprobe=None, gop=None,
                floor_p=None, floor_i=None, sfloor_p=None, sfloor_i=None, sfloors=None, ctor=None):
    """plan: per frame 'I' | 'P' | 'A' (encode_frame); a floor of None: its setter is never called; sfloors: {frame index: p-frame SSIM floor set
    before it}; ctor: constructor keywords -> (stream bytes, rung after every frame, type of every frame)"""
    buf = io.BytesIO()
    enc = pkg.Encoder(buf, w, h, 30, quality, ctx, device_entropy=device_entropy, qualities=qualities, frame_report=True, **(ctor or {}))
    rungs, types = [], []
    try:
        if rung is not None:
            enc.set_rung(rung)
        if budget_p:
            enc.set_rate(budget_p)
        if budget_i:
            enc.set_iframe_budget(budget_i)
        if pprobe is not None:
            enc.set_pframe_probe(pprobe)
        if gop is not None:
            enc.set_gop(gop)
        if floor_i is not None:
            enc.set_iframe_quality_floor(floor_i)
        if floor_p is not None:
            enc.set_pframe_quality_floor(floor_p)
        if sfloor_i is not None:
            enc.set_iframe_ssim_floor(sfloor_i)
        if sfloor_p is not None:
            enc.set_pframe_ssim_floor(sfloor_p)
        for t, (f, kind) in enumerate(zip(frames, plan)):
            vf = pkg.VideoFrame.from_packed(w, h, f)
            if sfloors and t in sfloors:
                enc.set_pframe_ssim_floor(sfloors[t])
            if kind == "A":
                types.append(enc.encode_frame(vf))
            else:
                enc.encode_iframe(vf) if kind == "I" else enc.encode_pframe(vf)
                types.append(1 if kind == "I" else 2)
            assert enc.last_report.type == types[-1]
            rungs.append(enc.rung)
        enc.finish()
    finally:
        enc.close()
    return buf.getvalue(), rungs, types


def model_run(oracle, w, h, frames, plan, qualities=LADDER, sfloors=None, **kw):
    """the same run on the model -> (model, types, whys, rung of every frame)"""
    em = SsimEncoderModel(oracle, w, h, qualities, **kw)
    types, whys, rungs = [], [], []
    for t, (f, kind) in enumerate(zip(frames, plan)):
        if sfloors and t in sfloors:
            em.sfloor_p = sfloors[t]
        if kind == "A":
            ty, why = em.frame(f)
        else:
            ty, why = (em.iframe(f), "I") if kind == "I" else (em.pframe(f), "P")
        types.append(ty); whys.append(why); rungs.append(em.last_rung)
    return em, types, whys, rungs


def clear_of(floor, values, allowed):
    """no allowed rung's model value within NEAR of the floor"""
    return all(abs(values[r] - floor) > NEAR for r in allowed)


def top_two_decided(q, recs, allowed, w, h):
    """where the largest q24 decides: the best two allowed rungs are identical reconstructions or more than NEAR apart"""
    order = sorted(allowed, key=lambda r: -q[r])
    return len(order) < 2 or np.array_equal(recs[order[0]], recs[order[1]]) or (q[order[0]] - q[order[1]]) / (ONE * n_windows(w, h)) > NEAR


# ------------------------------------------------------------------ check 5: the SSIM floors
def check_floor(pkg, ctx, oracle, device_entropy, w=50, h=38):
    K = len(LADDER)
    frames, plan = prd.floor_clip(w, h), "IPPP"
    model = pp.model_in_state(oracle, w, h, LADDER, 1, 0)
    pan = state_frames(w, h, 1, 0)[1][0]
    sizes = [int(x) for x in pp.facts(oracle, w, h, LADDER, 1, 0)[1][0][0]]                      # the pan behind the first frame: state 0, "pan1"
    tot = [int(x) for x in prd.sse_facts(oracle, w, h, LADDER, 1, 0)[1][0][0].astype(np.int64).sum(axis=1)]
    qs, recs = pframe_ssim(model, 0, pan)
    q = [float(x) for x in qs.sum(axis=1)]
    s = [mean_ssim(x, w, h) for x in q]
    psnr = [prd.psnr_yuv(t, w, h) for t in tot]
    print(f"p-frame SSIM floor model: pan1 sizes {sizes} ssim {[round(x, 6) for x in s]} psnr {[round(x, 3) for x in psnr]}")
    every = list(range(K))
    order = sorted(every, key=lambda r: s[r])                                                    # rungs by similarity

    def first(floor, bp=0, db=0.0):
        return choose_rung(sizes, tot, q, bp, db, floor, w, h)

    # every case: (SSIM floor, PSNR floor, p-frame budget, name); what it lands on is asserted on the model first
    cases = []
    lo = min(s) - 0.01                                                                           # every rung meets it: the fewest bytes
    assert lo > 0 and first(lo) == int(np.argmin(sizes)) == K - 1
    cases.append((lo, 0.0, 0, "coarsest"))
    between = 0.5 * (s[order[1]] + s[order[2]])
    r_mid = first(between)
    assert 0 < r_mid < K - 1 and clear_of(between, s, every), (r_mid, s)
    cases.append((between, 0.0, 0, "middle"))
    assert first(s[r_mid] - STEP) == r_mid and first(s[r_mid] + STEP) != r_mid                   # 4e-6 either side of a model value
    assert clear_of(s[r_mid] - STEP, s, [r for r in every if r != r_mid]) and clear_of(s[r_mid] + STEP, s, [r for r in every if r != r_mid])
    cases.append((s[r_mid] - STEP, 0.0, 0, "just met"))
    cases.append((s[r_mid] + STEP, 0.0, 0, "just missed"))
    none = 0.5 * (max(s) + 1.0)                                                                  # none meets: the largest q24 total
    assert max(s) < 1.0 - 1e-4 and first(none) == int(np.argmax(q)) and top_two_decided(q, recs, every, w, h)
    cases.append((none, 0.0, 0, "none meets"))
    assert first(1.0) == int(np.argmax(q))
    cases.append((1.0, 0.0, 0, "floor 1.0"))
    bp = sizes[r_mid] - 1                                                                        # the budget excludes the rung the floor alone would take
    r_b = first(between, bp)
    allowed_b = [r for r in every if sizes[r] <= bp]
    assert r_b != r_mid and sizes[r_b] <= bp and (any(s[r] >= between for r in allowed_b) or top_two_decided(q, recs, allowed_b, w, h))
    cases.append((between, 0.0, bp, "floor and budget"))
    assert min(sizes) > 1 and first(between, min(sizes) - 1) == K - 1                            # nothing allowed: the coarsest
    cases.append((between, 0.0, min(sizes) - 1, "nothing allowed"))
    db = psnr[r_mid] + 1e-6                                                                      # both floors: the PSNR floor excludes the SSIM floor's rung
    r_both = first(between, 0, db)
    assert r_both != r_mid and all(abs(psnr[r] - db) > 1e-9 for r in every)
    if not any(s[r] >= between and psnr[r] >= db for r in every):
        assert top_two_decided(q, recs, every, w, h)
    cases.append((between, db, 0, "both floors"))
    for sfloor, floor_db, budget_p, name in cases:
        em, _, _, rungs = model_run(oracle, w, h, frames, plan, rung=1, sfloor_p=sfloor, floor_p=floor_db, budget_p=budget_p)
        assert rungs[1] == first(sfloor, budget_p, floor_db) and len(em.pss) == 3
        for sizes_t, tot_t, q_t in em.pss[1:]:                                                   # the later frames of the clip decide clearly as well
            st = [mean_ssim(x, w, h) for x in q_t]
            al = [r for r in every if not budget_p or int(sizes_t[r]) <= budget_p]
            assert clear_of(sfloor, st, al), (name, st)
            if not any(st[r] >= sfloor for r in al) and al:
                o = sorted(al, key=lambda r: -q_t[r])
                assert len(o) < 2 or abs(st[o[0]] - st[o[1]]) > NEAR or (q_t[o[0]] == q_t[o[1]] and tot_t[o[0]] == tot_t[o[1]]), (name, st)
        data, got, _ = run_encoder(pkg, ctx, w, h, frames, plan, device_entropy, qualities=LADDER, rung=1, sfloor_p=sfloor,
                                   floor_p=floor_db or None, budget_p=budget_p)
        print(f"p-frame SSIM floor {sfloor!r} psnr floor {floor_db!r} budget {budget_p} ({name}): rungs {got}, model {rungs}")
        assert got == rungs, (name, sfloor, got, rungs)
        assert data == em.sb.bytes(), (name, len(data), len(em.sb.bytes()))
    # the constructor argument is the setter
    em, _, _, rungs = model_run(oracle, w, h, frames, plan, rung=1, sfloor_p=between)
    data, got, _ = run_encoder(pkg, ctx, w, h, frames, plan, device_entropy, qualities=LADDER, rung=1, ctor={"pframe_ssim_floor": between})
    assert got == rungs and data == em.sb.bytes()


def check_iframe_floor(pkg, ctx, oracle, device_entropy, w=50, h=38):
    """the gradient i-frame: an SSIM floor of 0.9713 takes rung 3, a PSNR floor of 33.8 dB pays for rung 2; with a budget; the constructor"""
    g = gradient(w, h)
    sizes = [int(x) for x in pc.expected(oracle, w, h, LADDER, g)[0]]
    tot = [int(x) for x in rc.expected_sse(oracle, w, h, LADDER, g).astype(np.int64).sum(axis=1)]
    qs, recs = iframe_ssim(oracle, w, h, LADDER, g)
    q = [float(x) for x in qs.sum(axis=1)]
    s = [mean_ssim(x, w, h) for x in q]
    every = list(range(len(LADDER)))
    assert choose_rung(sizes, tot, q, 0, 0.0, 0.9713, w, h) == 3 and choose_rung(sizes, tot, q, 0, 33.8, 0.0, w, h) == 2 and clear_of(0.9713, s, every)
    budget = sizes[1] - 1                                               # the best-looking rung is out of reach: floor 1.0 takes the best that fits
    allowed = [r for r in every if sizes[r] <= budget]
    best = choose_rung(sizes, tot, q, budget, 0.0, 1.0, w, h)
    assert best == max(allowed, key=lambda r: q[r]) and top_two_decided(q, recs, allowed, w, h)
    for kw, want in (({"sfloor_i": 0.9713}, 3), ({"floor_i": 33.8}, 2), ({"sfloor_i": 1.0, "budget_i": budget}, best),
                     ({"sfloor_i": 0.9713, "floor_i": 33.8}, choose_rung(sizes, tot, q, 0, 33.8, 0.9713, w, h))):
        em, _, _, rungs = model_run(oracle, w, h, [g, g], "II", rung=0, **kw)
        assert rungs == [want, want]
        data, got, _ = run_encoder(pkg, ctx, w, h, [g, g], "II", device_entropy, qualities=LADDER, **kw)
        assert got == rungs and data == em.sb.bytes(), (kw, got, rungs)
    em, _, _, rungs = model_run(oracle, w, h, [g], "I", sfloor_i=0.9713)
    data, got, _ = run_encoder(pkg, ctx, w, h, [g], "I", device_entropy, qualities=LADDER, ctor={"iframe_ssim_floor": 0.9713})
    assert got == rungs == [3] and data == em.sb.bytes()


def check_floor_off_and_one_rung(pkg, ctx, oracle, device_entropy, w=50, h=38):
    """floor 0, with and without the calls: today's bytes under pfv_encoder_set_rate's soft rule and under the hard budget; a one-rung encoder
    never probes; a frame without windows (6x6) meets every SSIM floor"""
    clip = lc.rate_clip(w, h)[:8]
    hard_bp = pp.hard_budget(oracle, w, h, lc.rate_clip(w, h))[0]
    for pprobe in (None, True):
        want = pp.EncoderModel(oracle, w, h, lc.RATE_LADDER, rung=2, budget_p=hard_bp, pprobe=bool(pprobe))
        want_rungs = []
        for t, f in enumerate(clip):
            want.iframe(f) if t == 0 else want.pframe(f)
            want_rungs.append(want.last_rung)
        assert len(set(want_rungs[1:])) >= 2                                                     # the rule under test moves the rung
        for floor in (None, 0.0):
            data, got, _ = run_encoder(pkg, ctx, w, h, clip, "I" + "P" * 7, device_entropy, qualities=lc.RATE_LADDER, rung=2, budget_p=hard_bp,
                                       pprobe=pprobe, sfloor_p=floor, sfloor_i=floor)
            assert got == want_rungs and data == want.sb.bytes(), (pprobe, floor, got, want_rungs)
    frames, plan = prd.floor_clip(w, h), "IPPP"
    plain, _, _ = run_encoder(pkg, ctx, w, h, frames, plan, device_entropy, quality=4)
    for floor in (0.5, 1.0):
        data, got, _ = run_encoder(pkg, ctx, w, h, frames, plan, device_entropy, qualities=[4], sfloor_p=floor, sfloor_i=floor, budget_p=100)
        assert data == plain and got == [0] * 4
    tiny = clips(6, 6, 1)[0][:3]
    em, _, _, rungs = model_run(oracle, 6, 6, tiny, "IPA", rung=1, sfloor_p=1.0, sfloor_i=1.0)
    data, got, _ = run_encoder(pkg, ctx, 6, 6, tiny, "IPA", device_entropy, qualities=LADDER, rung=1, sfloor_p=1.0, sfloor_i=1.0)
    assert got == rungs and data == em.sb.bytes() and rungs[0] == int(np.argmin(pc.expected(oracle, 6, 6, LADDER, tiny[0])[0])), (got, rungs)


# ------------------------------------------------------------------ check 6: the frame type under the SSIM floor
SS_GOP = 3
SS_BUDGET_P = prd.RD_BUDGET_P


def ssim_clip(w, h):
    """prdprobe_cases.rd_clip's frames with a p-frame SSIM floor set before each (None: it stays)"""
    frames = [f for f, _ in prd.rd_clip(w, h)]
    floors = SS_FLOORS
    assert len(floors) == len(frames)
    return list(zip(frames, floors))


# chosen on the model (the prints of check_frame_type show every candidate's mean SSIM): see the branches asserted there
SS_FLOORS = [0.90, None, None, None, 0.97, 0.90, 0.9999, 0.80, None, None, None]


def check_frame_type(pkg, ctx, oracle, device_entropy, w=50, h=38):
    clip = ssim_clip(w, h)
    frames = [f for f, _ in clip]
    sfloors = {t: fl for t, (_, fl) in enumerate(clip) if fl is not None}
    plan = "A" * len(frames)
    em = SsimEncoderModel(oracle, w, h, LADDER, rung=1, sfloor_p=sfloors[0], gop=SS_GOP, budget_p=SS_BUDGET_P)
    types, whys, rungs = [], [], []
    for t, f in enumerate(frames):
        if t in sfloors:
            em.sfloor_p = sfloors[t]
        em.last_pair = None
        ty, why = em.frame(f)
        types.append(ty); whys.append(why); rungs.append(em.last_rung)
        print(f"ssim frame type {t}: floor {em.sfloor_p} -> {why} at rung {em.last_rung}; (p meets, i meets, p ssim, i ssim) {em.last_pair}")
        if em.last_pair is not None:                                    # the candidates' values are clear of the floor, and of each other where q24 decides
            pm, im, ps, is_ = em.last_pair
            assert abs(ps - em.sfloor_p) > NEAR and abs(is_ - em.sfloor_p) > NEAR
            if not pm and not im:
                assert abs(ps - is_) > NEAR
    print(f"ssim frame types {types} ({whys}), rungs {rungs}")
    for why in ("forced", "still", "only i", "only p", "both, p", "both, i"):                     # of the MODEL first
        assert why in whys, (why, whys)
    assert whys[0] == "forced" and "forced" in whys[1:] and ("neither, i" in whys or "neither, p" in whys)
    _, old_types, old_whys, _ = prd.model_run(oracle, w, h, frames, plan, rung=1, gop=SS_GOP, budget_p=SS_BUDGET_P)
    print(f"the size rule's types {old_types} ({old_whys})")
    assert any(a != b for a, b in zip(types, old_types))
    data, got_rungs, got_types = run_encoder(pkg, ctx, w, h, frames, plan, device_entropy, qualities=LADDER, rung=1, gop=SS_GOP, sfloor_p=sfloors[0],
                                             sfloors=sfloors, budget_p=SS_BUDGET_P)
    assert got_types == types and got_rungs == rungs, (got_types, types, got_rungs, rungs)
    assert data == em.sb.bytes()
    got, ofr = lc.decode_both(pkg, ctx, oracle, data)
    assert len(ofr) == len(frames)
    for t, (s, o) in enumerate(zip(em.shown, ofr)):
        if s is not None:
            assert o is not None and np.array_equal(o, s), t
    shown = [o for o in ofr if o is not None]
    assert len(got) == len(shown) and all(np.array_equal(a, b) for a, b in zip(got, shown))
    # once more with an i-frame SSIM floor and both budgets set: ri is encode_iframe's own choice from the same probe results
    bi = int(pc.expected(oracle, w, h, LADDER, frames[0])[0][1])
    bp = int(pp.facts(oracle, w, h, LADDER, 1, 0)[1][0][0][1])
    em, types, whys, rungs = model_run(oracle, w, h, frames, plan, rung=3, sfloor_p=sfloors[0], sfloors=sfloors, gop=SS_GOP, sfloor_i=0.95, budget_i=bi,
                                       budget_p=bp)
    print(f"ssim frame types under an i-frame SSIM floor and both budgets: {types} ({whys}), rungs {rungs}")
    assert 1 in types[1:] and 2 in types and len(set(rungs)) >= 3
    data, got_rungs, got_types = run_encoder(pkg, ctx, w, h, frames, plan, device_entropy, qualities=LADDER, rung=3, gop=SS_GOP, sfloor_p=sfloors[0],
                                             sfloors=sfloors, sfloor_i=0.95, budget_i=bi, budget_p=bp)
    assert got_types == types and got_rungs == rungs, (got_types, types, got_rungs, rungs)
    assert data == em.sb.bytes()


# ------------------------------------------------------------------ check 7: arguments and states
def check_arguments(pkg, ctx, oracle, w=50, h=38):
    L, lib = pkg._lib, ctx._lib
    BAD, STATE = L.PFV_ERR_BAD_ARG, L.PFV_ERR_STATE
    P = ctypes.c_void_p
    frame = clips(w, h, 1)[0][1]
    vf = pkg.VideoFrame.from_packed(w, h, frame)
    bufs = DevBufs(ctx)
    s = pkg.EncoderSession(ctx, w, h, 4, 1)                            # one rung: one size, three sums of each kind
    try:
        frames_dev, sizes_dev = bufs.put(frame), bufs.put(np.zeros(1, np.uint32))
        sse_dev, q_dev = bufs.put(np.zeros(3, np.uint64)), bufs.put(np.zeros(3, np.int64))
        host, host_sse, host_q = np.zeros(1, np.uint32), np.zeros(3, np.uint64), np.zeros(3, np.int64)
        hp, hs, hq, fp = host.ctypes.data_as(P), host_sse.ctypes.data_as(P), host_q.ctypes.data_as(P), frame.ctypes.data_as(P)
        model = LadderModel(oracle, w, h, [4])                         # against the blank reference of a new session
        for name, pframe in (("iframe", False), ("pframe", True)):
            dev, hostf = getattr(lib, f"pfv_enc_probe_{name}_ssim_dev"), getattr(lib, f"pfv_enc_probe_{name}_ssim")
            good = [s.handle, P(frames_dev), P(sizes_dev), P(sse_dev), P(q_dev)]
            for k in range(5):                                          # every NULL argument (stats_dev may be NULL)
                assert dev(*[None if j == k else a for j, a in enumerate(good)], None) == BAD, (name, k)
            good = [s.handle, fp, hp, hs, hq]
            for k in range(5):
                assert hostf(*[None if j == k else a for j, a in enumerate(good)]) == BAD, (name, k)
            if pframe:
                want, want_sse = pp.pframe_facts(model, 0, frame)[0], prd.pframe_sse(model, 0, frame)[0].astype(np.uint64)
                want_q = pframe_ssim(model, 0, frame)[0]
                sizes, sse, q = s.probe_pframe_ssim(frame)
                s.probe_pframe_ssim_dev(frames_dev, sizes_dev, sse_dev, q_dev)    # usable after every refused call
            else:
                want, want_sse = pc.expected(oracle, w, h, [4], frame)[0], rc.expected_sse(oracle, w, h, [4], frame)
                want_q = iframe_ssim(oracle, w, h, [4], frame)[0]
                sizes, sse, q = s.probe_iframe_ssim(frame)
                s.probe_iframe_ssim_dev(frames_dev, sizes_dev, sse_dev, q_dev)
            assert sizes.shape == (1, 1) and sse.shape == (1, 1, 3) and q.shape == (1, 1, 3)
            assert np.array_equal(sizes[0], want) and np.array_equal(sse[0], want_sse)
            assert_q24(q[0], want_q, w, h, f"arguments, {name}")
            ctx.download(host, sizes_dev); ctx.download(host_sse, sse_dev); ctx.download(host_q, q_dev)
            assert np.array_equal(host, want) and np.array_equal(host_sse, want_sse[0]) and np.array_equal(host_q, q[0][0])
    finally:
        s.close()
        bufs.close()
    y, u, v = (pl.pixels.ctypes.data_as(P) for pl in (vf.plane_y, vf.plane_u, vf.plane_v))
    e = pkg.Encoder(io.BytesIO(), w, h, 30, None, ctx, qualities=[1, 4, 9])
    try:
        out, out_sse, out_q = np.zeros(3, np.uint32), np.zeros((3, 3), np.uint64), np.zeros((3, 3), np.int64)
        good = [e.handle, y, u, v, out.ctypes.data_as(P), out_sse.ctypes.data_as(P), out_q.ctypes.data_as(P)]
        for fn in (lib.pfv_encoder_probe_iframe_ssim, lib.pfv_encoder_probe_pframe_ssim):
            for k in range(7):
                assert fn(*[None if j == k else a for j, a in enumerate(good)]) == BAD, k
        for setter in (lib.pfv_encoder_set_iframe_ssim_floor, lib.pfv_encoder_set_pframe_ssim_floor):
            assert setter(None, 0.5) == BAD
            for bad in (math.nan, -1.0, -1e-300, 1.0 + 1e-9):
                assert setter(e.handle, bad) == BAD
            for good_floor in (0.0, 0.5, 1.0, 0.0):
                assert setter(e.handle, good_floor) == 0
        model = LadderModel(oracle, w, h, [1, 4, 9])
        sizes, sse, q = e.probe_pframe_ssim(vf)                        # usable after every refused call
        assert np.array_equal(sizes, pp.pframe_facts(model, 0, frame)[0]) and np.array_equal(sse, prd.pframe_sse(model, 0, frame)[0].astype(np.uint64))
        assert_q24(q, pframe_ssim(model, 0, frame)[0], w, h, "arguments, encoder")
        sizes, sse, q = e.probe_iframe_ssim(vf)
        assert np.array_equal(sizes, pc.expected(oracle, w, h, [1, 4, 9], frame)[0])
        assert_q24(q, iframe_ssim(oracle, w, h, [1, 4, 9], frame)[0], w, h, "arguments, encoder i-frame")
        assert e.rung == 0
        e.finish()
        with pytest.raises(pkg.PfvError) as err:                       # a finished encoder
            e.probe_pframe_ssim(vf)
        assert err.value.code == STATE
    finally:
        e.close()


def build_poison(exe):
    """tests/cpp/ssim_floor.cpp in its `poison` mode against pprobe_cases.build_poison's seam build of the library sources on the CPU emulator"""
    emu = os.path.join(ROOT, "tests", "hipemu")
    pp.build_poison(exe + "_size_probe")                               # makes (or finds) libpfv_emu_seam.so
    lib = os.path.join(emu, "libpfv_emu_seam.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-DSSIM_FLOOR_SEAM", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "ssim_floor.cpp"), "-o", exe, lib, "-Wl,-rpath," + emu], check=True)


def check_poisoned(exe, tmp_path, w=50, h=38):
    """a p-frame fails behind its encode kernel (the seam fails the payload-size download): pfv_encoder_probe_pframe_ssim returns PFV_ERR_STATE
    until an i-frame has been written"""
    STATE = -9                                                         # PFV_ERR_STATE, include/pfv_hip_core.h
    yuv = str(tmp_path / "poison.yuv")
    np.concatenate(clips(w, h, 1)[0][:2]).tofile(yuv)
    r = subprocess.run([exe, "poison", str(w), str(h), ",".join(str(q) for q in LADDER), yuv], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert [ln[0] for ln in lines] == ["failed", "poisoned", "recovered"]
    assert int(lines[0][1]) < 0 and int(lines[1][1]) == STATE and int(lines[2][1]) == 0


# ------------------------------------------------------------------ check 8: the C++ mirror
def build_cpp(lib_path, exe):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "ssim_floor.cpp"), "-o", exe, lib_path, "-Wl,-rpath," + os.path.dirname(lib_path)], check=True)


def check_cpp(oracle, exe, tmp_path, w=50, h=38):
    """tests/cpp/ssim_floor.cpp (pfv::Encoder::probe_pframe_ssim, set_pframe_ssim_floor) on the floor clip: the model's sizes, plane sums, rungs
    and bytes, and q24 within the tolerance"""
    frames = prd.floor_clip(w, h)
    model = pp.model_in_state(oracle, w, h, LADDER, 1, 0)
    s = sorted(mean_ssim(x, w, h) for x in pframe_ssim(model, 0, frames[1])[0].sum(axis=1))
    floor = 0.5 * (s[1] + s[2])
    em = SsimEncoderModel(oracle, w, h, LADDER, rung=1, sfloor_p=floor)
    want_sizes, want_sse, want_q, rungs = [], [], [], []
    for t, f in enumerate(frames):
        if t:
            want_sizes.append(pp.pframe_facts(em.model, 0, f)[0].tolist())
            want_sse.append(prd.pframe_sse(em.model, 0, f)[0].reshape(-1).tolist())
            want_q.append(pframe_ssim(em.model, 0, f)[0])
        em.iframe(f) if t == 0 else em.pframe(f)
        rungs.append(em.last_rung)
    for sizes_t, _, q_t in em.pss:
        assert clear_of(floor, [mean_ssim(x, w, h) for x in q_t], range(len(LADDER)))
    yuv, out = str(tmp_path / "sfloor.yuv"), str(tmp_path / "sfloor.pfv")
    np.concatenate(frames).tofile(yuv)
    r = subprocess.run([exe, "run", str(w), str(h), ",".join(str(q) for q in LADDER), "1", repr(floor), yuv, out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 3 * (len(frames) - 1) + 1
    for t in range(len(frames) - 1):
        assert [int(x) for x in lines[3 * t].split()[1:]] == want_sizes[t]
        assert [int(x) for x in lines[3 * t + 1].split()[1:]] == want_sse[t]
        assert_q24(np.array([int(x) for x in lines[3 * t + 2].split()[1:]], np.int64).reshape(-1, 3), want_q[t], w, h, f"c++ frame {t + 1}")
    assert [int(x) for x in lines[-1].split()[1:]] == rungs and 0 < rungs[1] < len(LADDER) - 1
    assert open(out, "rb").read() == em.sb.bytes()
