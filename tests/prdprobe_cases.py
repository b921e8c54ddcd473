"""Shared checks of the p-frame rate-distortion probe (pfv_enc_probe_pframe_rd*, pfv_encoder_probe_pframe_rd), pfv_encoder's p-frame quality floor
(pfv_encoder_set_pframe_quality_floor) and the frame type it gives pfv_encoder_encode_frame (include/pfv_hip_ext.h, "p-frame rate-distortion
probe"), driven on the CPU emulator by tests/test_emu_prdprobe.py and on a real MI355X by tests/test_gpu_prdprobe.py at the same small shapes.

Every expectation comes from the oracles, never from the code under test: sizes and counts are pprobe_cases.facts; the squared error of a frame
as a p-frame at rung r is numpy int64 over recon[:ph, :pw] - source, per plane, of LadderModel.pframe(k, frame, r) on a COPY of the model's prev
planes; i-frame sizes and errors are probe_cases.expected and rdprobe_cases.expected_sse.  Everything is compared for equality."""
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
import probe_cases as pc
import rdprobe_cases as rc
from ladder_cases import LADDER, DevBufs, LadderModel, frame_bytes, plane_dims
from pprobe_cases import CODED, FRAME_NAMES, MOVED, NSTATS, SHAPES, clips, state_frames
from probe_cases import FULL_LADDER, SENTINEL, content, options
from rdprobe_cases import NOT_ENCODABLE, SENTINEL64, psnr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the reference
def pframe_sse(model, k, frame):
    """-> (sse int64 [R, 3], padded int64 [R, 3]): squared error per plane of `frame` against the reconstruction the model's p-frame at every rung
    leaves, inside the picture -- and over the whole padded planes, the source padded with the plane's clear value as the encoder pads it (what
    the motion search's own error covers: it must NOT be what the probe reports); the model's prev is not touched"""
    src = lc.split(frame, model.w, model.h)
    sse, padded = [], []
    for r in range(len(model.qualities)):
        m = copy.copy(model)
        m.prev = [list(p) for p in model.prev]                 # as pprobe_cases.pframe_facts
        m.pframe(k, frame, r)
        row, prow = [], []
        for rec, s, (pw, ph), clear in zip(m.prev[k], src, plane_dims(model.w, model.h), model.CLEAR):
            row.append(int(((rec[:ph, :pw].astype(np.int64) - s.astype(np.int64)) ** 2).sum()))
            full = np.full(rec.shape, clear, np.int64)
            full[:ph, :pw] = s
            prow.append(int(((rec.astype(np.int64) - full) ** 2).sum()))
        sse.append(row)
        padded.append(prow)
    return np.array(sse, np.int64), np.array(padded, np.int64)


_SSE = {}


def sse_facts(oracle, w, h, qualities, n, state, sets=None):
    """per frame set of state_frames (all, or those named by `sets`: None elsewhere): (sse uint64 [n, R, 3], padded int64 [n, R, 3]); computed
    once per (shape, ladder, state)"""
    key = (w, h, tuple(qualities), n, state, None if sets is None else tuple(sets))
    if key not in _SSE:
        model = pp.model_in_state(oracle, w, h, qualities, n, state)
        out = []
        for t, frames in enumerate(state_frames(w, h, n, state)):
            if sets is not None and t not in sets:
                out.append(None)
                continue
            per = [pframe_sse(model, k, frames[k]) for k in range(n)]
            out.append((np.stack([p[0] for p in per]).astype(np.uint64), np.stack([p[1] for p in per])))
        _SSE[key] = out
    return _SSE[key]


def psnr_yuv(tot, w, h):
    return psnr(int(tot), frame_bytes(w, h))


# ------------------------------------------------------------------ check 1: what the inputs exercise (the oracle alone)
def check_inputs_cover(oracle, w=50, h=38, n=3):
    pp.check_inputs_cover(oracle, w, h, n)
    still_wrong = padded_differs = smaller_worse = larger = nonmono = 0
    R = len(LADDER)
    for state in (0, 1):
        fsets = state_frames(w, h, n, state)
        for (sizes, stats, hass, _), (sse, padded), frames in zip(pp.facts(oracle, w, h, LADDER, n, state), sse_facts(oracle, w, h, LADDER, n, state), fsets):
            for k in range(n):
                isizes = pc.expected(oracle, w, h, LADDER, frames[k])[0].astype(np.int64)
                itot = rc.expected_sse(oracle, w, h, LADDER, frames[k]).astype(np.int64).sum(axis=1)
                ptot = sse[k].astype(np.int64).sum(axis=1)
                psz = sizes[k].astype(np.int64)
                smaller_worse += int(((psz < isizes) & (ptot > itot)).any())
                larger += int((psz > isizes).any())
                q = [psnr_yuv(t, w, h) for t in ptot]
                nonmono += int(any(b > a for a, b in zip(q, q[1:])))
                for r in range(R):
                    if not hass[k][r].any():
                        still_wrong += int(ptot[r] != 0)
                        padded_differs += int((padded[k][r] != sse[k][r].astype(np.int64)).any())
    print(f"p-frame rd probe inputs {w}x{h}x{n}: (frame, rung) pairs with nothing coded and an error {still_wrong}, of them with another error over "
          f"the padded planes {padded_differs}; frames with a rung where the p-frame is smaller and worse than the i-frame {smaller_worse}, with a "
          f"rung where it is larger {larger}, with a coarser rung of higher PSNR-YUV {nonmono}")
    assert still_wrong and padded_differs and smaller_worse and larger


# ------------------------------------------------------------------ check 2: the session probe
class PRdRig(pp.PProbeRig):
    """PProbeRig with a device buffer for the plane sums"""

    def __init__(self, pkg, ctx, w, h, qualities, n, stride=0):
        super().__init__(pkg, ctx, w, h, qualities, n, stride)
        self.sse_dev = self.bufs.put(np.zeros((n, self.R, 3), np.uint64))

    def upload(self, frames):
        super().upload(frames)
        self.ctx.upload(self.sse_dev, np.full((self.n, self.R, 3), SENTINEL64, np.uint64))

    def fetch(self):
        sizes, stats = super().fetch()
        sse = np.zeros((self.n, self.R, 3), np.uint64)
        self.ctx.download(sse, self.sse_dev)
        return sizes, stats, sse

    def probe(self, frames, stats=True):
        self.upload(frames)
        self.enc.probe_pframe_rd_dev(self.probe_dev, self.sizes_dev, self.sse_dev, self.stats_dev if stats else 0)
        return self.fetch()

    def size_probe(self, frames):
        self.upload(frames)
        self.enc.probe_pframe_dev(self.probe_dev, self.sizes_dev, self.stats_dev)
        return self.fetch()


def check_session_probe(pkg, ctx, oracle, w, h, n, int_transform=False, qualities=LADDER, sets=None):
    """real session calls make the states: i-frame at rung 1, probe, p-frame at rung 2, probe again.  Sizes, all 20 counts and the plane sums
    of every frame set (or of those named by `sets`, which include 1) at every rung; once without the counts (stats_dev = NULL); the host-buffer
    form agrees; the rung stays"""
    check_inputs_cover(oracle)
    if (w, h, n) in pp.INTERIOR_SHAPES and tuple(qualities) == tuple(LADDER):
        pp.check_interior_inputs(oracle, w, h, n, sets)
    with options(pkg, ctx, None, int_transform):
        rig = PRdRig(pkg, ctx, w, h, qualities, n)
    try:
        for state in (0, 1):
            cl = clips(w, h, n)
            rig.step(np.stack([c[state] for c in cl]), bool(state), 1 + state)
            fsets = state_frames(w, h, n, state)
            want, want_sse = pp.facts(oracle, w, h, qualities, n, state, sets), sse_facts(oracle, w, h, qualities, n, state, sets)
            for t, frames in enumerate(fsets):
                if want[t] is None:
                    continue
                sizes, stats, sse = rig.probe(frames)
                print(f"p-frame rd probe {w}x{h}x{n} state {state} {FRAME_NAMES[t]}: sse[0] {sse[0].tolist()} want {want_sse[t][0][0].tolist()}")
                assert np.array_equal(stats, want[t][1]), (state, FRAME_NAMES[t], np.argwhere(stats != want[t][1])[:4].tolist())
                assert np.array_equal(sizes, want[t][0]), (state, FRAME_NAMES[t], sizes.tolist(), want[t][0].tolist())
                assert np.array_equal(sse, want_sse[t][0]), (state, FRAME_NAMES[t], np.argwhere(sse != want_sse[t][0])[:4].tolist(), sse.tolist(),
                                                              want_sse[t][0].tolist())
            sizes, stats, sse = rig.probe(fsets[1], stats=False)
            assert np.array_equal(sizes, want[1][0]) and np.array_equal(sse, want_sse[1][0]) and (stats == SENTINEL).all()
            sizes, sse = rig.enc.probe_pframe_rd(fsets[1])
            assert np.array_equal(sizes, want[1][0]) and np.array_equal(sse, want_sse[1][0])
            assert rig.enc.rung == 1 + state
    finally:
        rig.close()


# ------------------------------------------------------------------ check 3: agreement with the shipped paths
def check_agrees_with_size_probe(pkg, ctx, oracle, w=50, h=38, n=3):
    """sizes and counts equal pfv_enc_probe_pframe_dev's on the same frames, in both states"""
    rig = PRdRig(pkg, ctx, w, h, LADDER, n)
    try:
        for state in (0, 1):
            rig.step(np.stack([c[state] for c in clips(w, h, n)]), bool(state), 1 + state)
            want = pp.facts(oracle, w, h, LADDER, n, state)
            for t in (1, 3, 6):
                frames = state_frames(w, h, n, state)[t]
                sizes, stats, _ = rig.probe(frames)
                sizes2, stats2, sse2 = rig.size_probe(frames)
                assert np.array_equal(sizes, sizes2) and np.array_equal(stats, stats2) and (sse2 == SENTINEL64).all()
                assert np.array_equal(sizes, want[t][0]) and np.array_equal(stats, want[t][1])
    finally:
        rig.close()


def check_probe_is_what_the_encoder_writes(pkg, ctx, oracle, device_entropy, w=50, h=38):
    """pfv_encoder with frame reports: behind the same i-frame, the probed (size, sse) of rung r == (packet_bytes - 5, sse) of the report of the
    p-frame then encoded at rung r == the model's; an i-frame between the rungs brings the reference back"""
    base = clips(w, h, 1)[0][0]
    fsets, want, want_sse = state_frames(w, h, 1, 0), pp.facts(oracle, w, h, LADDER, 1, 0), sse_facts(oracle, w, h, LADDER, 1, 0)
    enc = pkg.Encoder(io.BytesIO(), w, h, 30, None, ctx, device_entropy=device_entropy, frame_report=True, qualities=LADDER)
    try:
        for t in (1, 2, 6):                                             # pan1, pan4, texture
            vf = pkg.VideoFrame.from_packed(w, h, fsets[t][0])
            for r in range(len(LADDER)):
                enc.set_rung(1)
                enc.encode_iframe(pkg.VideoFrame.from_packed(w, h, base))
                sizes, sse = enc.probe_pframe_rd(vf)
                assert np.array_equal(sizes, want[t][0][0]) and np.array_equal(sse, want_sse[t][0][0]), (t, r, sizes.tolist(), sse.tolist())
                assert enc.rung == 1
                enc.set_rung(r)
                enc.encode_pframe(vf)
                rep = enc.last_report
                assert enc.rung == r and rep.type == 2 and rep.packet_bytes - 5 == int(sizes[r])
                assert [int(x) for x in rep.sse] == [int(x) for x in sse[r]], (t, r, list(rep.sse), sse[r].tolist())
    finally:
        enc.close()


# ------------------------------------------------------------------ check 4: no side effects, window and stride, graph
def check_no_side_effects(pkg, ctx, oracle, w=50, h=38, n=3):
    """i-frame at rung 1, then a p-frame at rung 3: prev_frame, the rung and every output of the p-frame are the model's whether or not probes of
    OTHER frames (device form and host-buffer form) run in between"""
    cl = clips(w, h, n)
    other, want_other, sse_other = state_frames(w, h, n, 0)[5], pp.facts(oracle, w, h, LADDER, n, 0)[5], sse_facts(oracle, w, h, LADDER, n, 0)[5]
    outs = []
    for with_probe in (False, True):
        rig = PRdRig(pkg, ctx, w, h, LADDER, n)
        try:
            rig.step(np.stack([c[0] for c in cl]), False, 1)
            if with_probe:
                before = rig.enc.prev_frame()
                ptr_before = [ctx._lib.pfv_enc_prev_frame_dev(rig.enc.handle, k) for k in range(n)]
                sizes, stats, sse = rig.probe(other)
                assert np.array_equal(sizes, want_other[0]) and np.array_equal(stats, want_other[1]) and np.array_equal(sse, sse_other[0])
                sizes, sse = rig.enc.probe_pframe_rd(other)
                assert np.array_equal(sizes, want_other[0]) and np.array_equal(sse, sse_other[0])
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
    """window (1, 2) with the frames frame_bytes + 48 apart: slots 1 and 2 exact, the entries of slot 0 left at the sentinels (64-bit for the sums)"""
    rig = PRdRig(pkg, ctx, w, h, LADDER, n, stride=frame_bytes(w, h) + 48)
    try:
        rig.to_state(1)
        rig.enc.set_frame_stride(rig.stride)
        rig.enc.set_window(1, 2)
        fsets, want, want_sse = state_frames(w, h, n, 1), pp.facts(oracle, w, h, LADDER, n, 1), sse_facts(oracle, w, h, LADDER, n, 1)
        for t in (1, 4):
            sizes, stats, sse = rig.probe(fsets[t])
            assert (sizes[0] == SENTINEL).all() and (stats[0] == SENTINEL).all() and (sse[0] == SENTINEL64).all()
            assert np.array_equal(sizes[1:], want[t][0][1:]) and np.array_equal(stats[1:], want[t][1][1:]) and np.array_equal(sse[1:], want_sse[t][0][1:])
        with pytest.raises(pkg.PfvError) as e:                          # the host-buffer form works on all slots, packed
            rig.enc.probe_pframe_rd(fsets[1])
        assert e.value.code == pkg._lib.PFV_ERR_STATE
        rig.enc.set_window(0, n)                                        # ... and the whole session again, still strided
        sizes, stats, sse = rig.probe(fsets[4])
        assert np.array_equal(sizes, want[4][0]) and np.array_equal(stats, want[4][1]) and np.array_equal(sse, want_sse[4][0])
    finally:
        rig.close()


def check_graph(pkg, ctx, oracle, w=50, h=38, n=3):
    """the launch pair recorded once and replayed on three contents: every replay exact (it finds both accumulators as k_pprobe_rd_sizes left
    them); a session that has never probed cannot start inside a recording"""
    rig = PRdRig(pkg, ctx, w, h, LADDER, n)
    fresh = pkg.EncoderSession(ctx, w, h, None, n, qualities=LADDER)
    graph = pkg.Graph(ctx)
    try:
        rig.to_state(0)
        fsets, want, want_sse = state_frames(w, h, n, 0), pp.facts(oracle, w, h, LADDER, n, 0), sse_facts(oracle, w, h, LADDER, n, 0)
        sizes, stats, sse = rig.probe(fsets[1])                         # the unrecorded call (it makes the accumulators)
        assert np.array_equal(sizes, want[1][0]) and np.array_equal(stats, want[1][1]) and np.array_equal(sse, want_sse[1][0])
        with graph:
            rig.enc.probe_pframe_rd_dev(rig.probe_dev, rig.sizes_dev, rig.sse_dev, rig.stats_dev)
            with pytest.raises(pkg.PfvError) as e:
                fresh.probe_pframe_rd_dev(rig.probe_dev, rig.sizes_dev, rig.sse_dev)
            assert e.value.code == pkg._lib.PFV_ERR_STATE and "before pfv_graph_begin" in str(e.value)
        for t in (5, 0, 2):
            rig.upload(fsets[t])
            graph.launch()
            sizes, stats, sse = rig.fetch()
            assert np.array_equal(stats, want[t][1]) and np.array_equal(sizes, want[t][0]) and np.array_equal(sse, want_sse[t][0]), FRAME_NAMES[t]
    finally:
        graph.close()
        fresh.close()
        rig.close()


# ------------------------------------------------------------------ the encoder's rules on the model
def choose_rung(sizes, tot, budget, floor, w, h):
    """the floor's rule (pfv_encoder_set_iframe_quality_floor / _set_pframe_quality_floor) on sizes [K] and total squared errors [K]"""
    K = len(sizes)
    sizes, tot = [int(x) for x in sizes], [int(x) for x in tot]
    allowed = [r for r in range(K) if sizes[r] != NOT_ENCODABLE and (not budget or sizes[r] <= budget)]
    if not allowed:
        return K - 1
    meets = [r for r in allowed if psnr_yuv(tot[r], w, h) >= floor]
    if meets:
        return min(meets, key=lambda r: (sizes[r], r))
    return min(allowed, key=lambda r: (tot[r], sizes[r], r))


class RdEncoderModel(pp.EncoderModel):
    """pprobe_cases.EncoderModel with the two quality floors; with both at 0 it is that model"""

    def __init__(self, oracle, w, h, qualities, floor_p=0.0, floor_i=0.0, **kw):
        super().__init__(oracle, w, h, qualities, **kw)
        self.floor_p, self.floor_i = floor_p, floor_i
        self.prd = []                                                   # (sizes, total squared errors) of every p-frame the floor probed

    def pfloor(self):
        return self.floor_p > 0 and self.K > 1

    def p_rd(self, f):
        sizes, stats, _, _ = pp.pframe_facts(self.model, 0, f)
        return sizes, stats, pframe_sse(self.model, 0, f)[0].sum(axis=1)

    def i_rd(self, f):
        return pc.expected(self.o, self.w, self.h, self.q, f)[0], rc.expected_sse(self.o, self.w, self.h, self.q, f).astype(np.int64).sum(axis=1)

    def iframe_rung(self, f):
        """the rung encode_iframe takes for `f`"""
        if self.K == 1 or not (self.budget_i or self.floor_i > 0):
            return self.rung
        sizes, tot = self.i_rd(f)
        return choose_rung(sizes, tot, self.budget_i, self.floor_i, self.w, self.h) if self.floor_i > 0 else self.fit(sizes, self.budget_i)

    def iframe(self, f):
        self.rung = self.iframe_rung(f)
        budget_i, self.budget_i = self.budget_i, 0                      # the rung is settled
        try:
            return super().iframe(f)
        finally:
            self.budget_i = budget_i

    def pframe(self, f, rung_settled=False):
        if not self.pfloor():
            return super().pframe(f, rung_settled)
        if not rung_settled:
            sizes, _, tot = self.p_rd(f)
            self.prd.append((sizes, tot))
            self.rung = choose_rung(sizes, tot, self.budget_p, self.floor_p, self.w, self.h)
        pprobe, self.pprobe = self.pprobe, True                         # no soft rule under the floor
        try:
            return super().pframe(f, rung_settled=True)
        finally:
            self.pprobe = pprobe

    def frame(self, f):
        """pfv_encoder_encode_frame -> (type, why); with the p-frame floor on rule 4 weighs the p-frame at rp against the i-frame at ri"""
        if not self.pfloor():
            return super().frame(f)
        if self.n_written == 0 or (self.gop > 0 and self.since_i >= self.gop):
            return self.iframe(f), "forced"
        psize, stats, ptot = self.p_rd(f)
        rp = choose_rung(psize, ptot, self.budget_p, self.floor_p, self.w, self.h)
        if stats[rp][CODED] == 0 and stats[rp][MOVED] == 0:
            return self.drop(), "still"
        isize, itot = self.i_rd(f)
        ri = self.iframe_rung(f)
        pb, ib, pe, ie = int(psize[rp]), int(isize[ri]), int(ptot[rp]), int(itot[ri])
        assert pb != NOT_ENCODABLE and ib != NOT_ENCODABLE
        pm, im = psnr_yuv(pe, self.w, self.h) >= self.floor_p, psnr_yuv(ie, self.w, self.h) >= self.floor_p
        if pm != im:
            take_i, why = im, "only i" if im else "only p"
        elif pm:
            take_i = ib <= pb
            why = "both, i" if take_i else "both, p"
        else:
            take_i = (ie, ib) <= (pe, pb)
            why = "neither, i" if take_i else "neither, p"
        if take_i:
            self.rung = ri
            floor_i, budget_i, self.floor_i, self.budget_i = self.floor_i, self.budget_i, 0.0, 0          # the rung is settled
            try:
                return self.iframe(f), why
            finally:
                self.floor_i, self.budget_i = floor_i, budget_i
        self.rung = rp
        return self.pframe(f, rung_settled=True), why


def run_encoder(pkg, ctx, w, h, frames, plan, device_entropy, qualities=None, quality=None, rung=None, budget_p=0, budget_i=0, pprobe=None, gop=None,
                floor_p=None, floor_i=None, floors=None, ctor_floor=None):
    """plan: per frame 'I' | 'P' | 'A' (encode_frame); floor_p None: pfv_encoder_set_pframe_quality_floor is never called; floors: {frame index:
    p-frame floor set before it}; ctor_floor: the constructor's pframe_quality_floor -> (stream bytes, rung after every frame, type of every frame)"""
    buf = io.BytesIO()
    kw = {} if ctor_floor is None else {"pframe_quality_floor": ctor_floor}
    enc = pkg.Encoder(buf, w, h, 30, quality, ctx, device_entropy=device_entropy, qualities=qualities, frame_report=True, **kw)
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
        for t, (f, kind) in enumerate(zip(frames, plan)):
            vf = pkg.VideoFrame.from_packed(w, h, f)
            if floors and t in floors:
                enc.set_pframe_quality_floor(floors[t])
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


def model_run(oracle, w, h, frames, plan, qualities=LADDER, floors=None, **kw):
    """the same run on the model -> (model, types, whys, rung of every frame)"""
    em = RdEncoderModel(oracle, w, h, qualities, **kw)
    types, whys, rungs = [], [], []
    for t, (f, kind) in enumerate(zip(frames, plan)):
        if floors and t in floors:
            em.floor_p = floors[t]
        if kind == "A":
            ty, why = em.frame(f)
        else:
            ty, why = (em.iframe(f), "I") if kind == "I" else (em.pframe(f), "P")
        types.append(ty); whys.append(why); rungs.append(em.last_rung)
    return em, types, whys, rungs


# ------------------------------------------------------------------ check 5: the p-frame floor
def floor_clip(w, h):
    """the clip of the session checks: its first frame (an i-frame at rung 1, state 0), then the pan"""
    return clips(w, h, 1)[0][:4]


def check_floor(pkg, ctx, oracle, device_entropy, w=50, h=38):
    K = len(LADDER)
    frames, plan = floor_clip(w, h), "IPPP"
    sizes = [int(x) for x in pp.facts(oracle, w, h, LADDER, 1, 0)[1][0][0]]                      # the pan behind the first frame: state 0, "pan1"
    tot = [int(x) for x in sse_facts(oracle, w, h, LADDER, 1, 0)[1][0][0].astype(np.int64).sum(axis=1)]
    q = [psnr_yuv(t, w, h) for t in tot]
    print(f"p-frame floor model: pan1 sizes {sizes} psnr {[round(x, 3) for x in q]}")
    order = sorted(range(K), key=lambda r: q[r])                                                 # rungs by fidelity

    def first(floor, bp=0):
        return choose_rung(sizes, tot, bp, floor, w, h)

    # every case: (floor, p-frame budget, name); what it lands on is asserted on the model first
    cases = []
    lo = min(q) - 1.0                                                                            # every rung meets it: the fewest bytes = the coarsest rung
    assert first(lo) == K - 1 and sizes[K - 1] == min(sizes)
    cases.append((lo, 0, "coarsest"))
    between = 0.5 * (q[order[1]] + q[order[2]])                                                  # midway between two rungs' model PSNRs
    r_mid = first(between)
    assert 0 < r_mid < K - 1, (r_mid, q)
    cases.append((between, 0, "middle"))
    assert first(q[r_mid] - 1e-9) == r_mid and first(q[r_mid] + 1e-9) not in (r_mid, K - 1)      # at a model value -+ 1e-9 dB: just met, just missed
    cases.append((q[r_mid] - 1e-9, 0, "just met"))
    cases.append((q[r_mid] + 1e-9, 0, "just missed"))
    none = max(q) + 1.0                                                                          # none meets the floor: the smallest error wins
    assert first(none) == int(np.argmin(tot))
    cases.append((none, 0, "none meets"))
    assert first(math.inf) == int(np.argmin(tot))
    cases.append((math.inf, 0, "+inf"))
    bp = sizes[r_mid] - 1                                                                        # the budget excludes the rung the floor alone would take
    r_b = first(between, bp)
    assert r_b != r_mid and sizes[r_b] <= bp
    cases.append((between, bp, "floor and budget"))
    assert min(sizes) > 1 and first(between, min(sizes) - 1) == K - 1                            # nothing allowed: the coarsest
    cases.append((between, min(sizes) - 1, "nothing allowed"))
    for floor, budget_p, name in cases:
        em, _, _, rungs = model_run(oracle, w, h, frames, plan, rung=1, floor_p=floor, budget_p=budget_p)
        assert rungs[1] == first(floor, budget_p) and len(em.prd) == 3
        data, got, _ = run_encoder(pkg, ctx, w, h, frames, plan, device_entropy, qualities=LADDER, rung=1, floor_p=floor, budget_p=budget_p)
        print(f"p-frame floor {floor!r} budget {budget_p} ({name}): rungs {got}, model {rungs}")
        assert got == rungs, (name, floor, got, rungs)
        assert data == em.sb.bytes(), (name, len(data), len(em.sb.bytes()))
    # the budget is a hard cap under the floor with the size probe's switch on as well, and the constructor argument is the setter
    em, _, _, rungs = model_run(oracle, w, h, frames, plan, rung=1, floor_p=between, budget_p=bp, pprobe=True)
    for kw in ({"floor_p": between}, {"ctor_floor": between}):
        data, got, _ = run_encoder(pkg, ctx, w, h, frames, plan, device_entropy, qualities=LADDER, rung=1, budget_p=bp, pprobe=True, **kw)
        assert got == rungs and data == em.sb.bytes()
    # floor 0, with and without the call: today's bytes -- pfv_encoder_set_rate's soft rule alone, and the hard budget of pfv_encoder_set_pframe_probe
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
                                       pprobe=pprobe, floor_p=floor)
            assert got == want_rungs and data == want.sb.bytes(), (pprobe, floor, got, want_rungs)
    # a one-rung encoder never probes: today's bytes
    plain, _, _ = run_encoder(pkg, ctx, w, h, frames, plan, device_entropy, quality=4)
    for floor in (1.0, 99.0, math.inf):
        data, got, _ = run_encoder(pkg, ctx, w, h, frames, plan, device_entropy, qualities=[4], floor_p=floor, budget_p=bp)
        assert data == plain and got == [0] * 4


# ------------------------------------------------------------------ check 6: the frame type under the floor
RD_GOP = 3


def rd_clip(w, h):
    """frames of the session checks and the p-frame floor set before each (None: it stays): the clip's first frame twice (a drop), the pan, a
    texture cut (under RD_BUDGET_P no p-frame rung reaches the floor, the i-frame does), the texture again under a floor only the p-frame
    reaches, a gradient (cheaper as an i-frame), the pan under a floor nothing reaches, then the pan past max_interval"""
    cl = clips(w, h, 1)[0]
    tex, grad = content(w, h, "texture", seed=0), content(w, h, "gradient", seed=0)
    return [(cl[0], 27.0), (cl[0], None), (cl[1], None), (tex, None), (tex, 30.0), (grad, 26.0), (cl[2], 60.0), (cl[3], 20.0), (cl[4], None),
            (cl[5], None), (cl[6], None)]


RD_BUDGET_P = 1200           # between the texture's p-frame sizes at rungs 1 and 2 behind the pan: the finer rungs are out of reach


def check_rd_frame_type(pkg, ctx, oracle, device_entropy, w=50, h=38):
    clip = rd_clip(w, h)
    frames = [f for f, _ in clip]
    floors = {t: fl for t, (_, fl) in enumerate(clip) if fl is not None}
    plan = "A" * len(frames)
    em, types, whys, rungs = model_run(oracle, w, h, frames, plan, rung=1, floor_p=floors[0], floors=floors, gop=RD_GOP, budget_p=RD_BUDGET_P)
    print(f"rd frame types {types} ({whys}), rungs {rungs}")
    for why in ("forced", "still", "only i", "only p", "both, p", "both, i"):                     # of the MODEL first
        assert why in whys, (why, whys)
    assert whys[0] == "forced" and "forced" in whys[1:] and ("neither, i" in whys or "neither, p" in whys)
    # today's rule 4 on the same clip (the model with the floor off) types at least one frame differently
    _, old_types, old_whys, _ = model_run(oracle, w, h, frames, plan, rung=1, gop=RD_GOP, budget_p=RD_BUDGET_P)
    print(f"the size rule's types {old_types} ({old_whys})")
    assert any(a != b for a, b in zip(types, old_types))
    data, got_rungs, got_types = run_encoder(pkg, ctx, w, h, frames, plan, device_entropy, qualities=LADDER, rung=1, gop=RD_GOP, floor_p=floors[0],
                                             floors=floors, budget_p=RD_BUDGET_P)
    assert got_types == types and got_rungs == rungs, (got_types, types, got_rungs, rungs)
    assert data == em.sb.bytes()
    got, ofr = lc.decode_both(pkg, ctx, oracle, data)
    assert len(ofr) == len(frames)
    for t, (s, o) in enumerate(zip(em.shown, ofr)):
        if s is not None:
            assert o is not None and np.array_equal(o, s), t
    shown = [o for o in ofr if o is not None]
    assert len(got) == len(shown) and all(np.array_equal(a, b) for a, b in zip(got, shown))
    # ri is encode_iframe's own choice: with an i-frame floor and an i-frame budget set, from the same probe results
    bi = int(pc.expected(oracle, w, h, LADDER, frames[0])[0][1])
    em, types, whys, rungs = model_run(oracle, w, h, frames, plan, rung=3, floor_p=floors[0], floors=floors, gop=RD_GOP, floor_i=30.0, budget_i=bi,
                                       budget_p=int(pp.facts(oracle, w, h, LADDER, 1, 0)[1][0][0][1]))
    print(f"rd frame types under an i-frame floor and both budgets: {types} ({whys}), rungs {rungs}")
    assert 1 in types[1:] and 2 in types and len(set(rungs)) >= 3
    data, got_rungs, got_types = run_encoder(pkg, ctx, w, h, frames, plan, device_entropy, qualities=LADDER, rung=3, gop=RD_GOP, floor_p=floors[0],
                                             floors=floors, floor_i=30.0, budget_i=bi, budget_p=int(pp.facts(oracle, w, h, LADDER, 1, 0)[1][0][0][1]))
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
    s = pkg.EncoderSession(ctx, w, h, 4, 1)                            # one rung: one size, three sums
    try:
        frames_dev, sizes_dev, sse_dev = bufs.put(frame), bufs.put(np.zeros(1, np.uint32)), bufs.put(np.zeros(3, np.uint64))
        host, host_sse = np.zeros(1, np.uint32), np.zeros(3, np.uint64)
        hp, hs, fp = host.ctypes.data_as(P), host_sse.ctypes.data_as(P), frame.ctypes.data_as(P)
        assert lib.pfv_enc_probe_pframe_rd_dev(None, P(frames_dev), P(sizes_dev), P(sse_dev), None) == BAD
        assert lib.pfv_enc_probe_pframe_rd_dev(s.handle, None, P(sizes_dev), P(sse_dev), None) == BAD
        assert lib.pfv_enc_probe_pframe_rd_dev(s.handle, P(frames_dev), None, P(sse_dev), None) == BAD
        assert lib.pfv_enc_probe_pframe_rd_dev(s.handle, P(frames_dev), P(sizes_dev), None, None) == BAD
        assert lib.pfv_enc_probe_pframe_rd(None, fp, hp, hs) == BAD
        assert lib.pfv_enc_probe_pframe_rd(s.handle, None, hp, hs) == BAD
        assert lib.pfv_enc_probe_pframe_rd(s.handle, fp, None, hs) == BAD
        assert lib.pfv_enc_probe_pframe_rd(s.handle, fp, hp, None) == BAD
        model = LadderModel(oracle, w, h, [4])                         # against the blank reference of a new session
        want, want_sse = pp.pframe_facts(model, 0, frame)[0], pframe_sse(model, 0, frame)[0].astype(np.uint64)
        sizes, sse = s.probe_pframe_rd(frame)
        assert sizes.shape == (1, 1) and sse.shape == (1, 1, 3) and np.array_equal(sizes[0], want) and np.array_equal(sse[0], want_sse)
        s.probe_pframe_rd_dev(frames_dev, sizes_dev, sse_dev)          # usable after every refused call
        ctx.download(host, sizes_dev)
        ctx.download(host_sse, sse_dev)
        assert np.array_equal(host, want) and np.array_equal(host_sse, want_sse[0])
    finally:
        s.close()
        bufs.close()
    y, u, v = (pl.pixels.ctypes.data_as(P) for pl in (vf.plane_y, vf.plane_u, vf.plane_v))
    buf = io.BytesIO()
    e = pkg.Encoder(buf, w, h, 30, None, ctx, qualities=[1, 4, 9])
    try:
        out, out_sse = np.zeros(3, np.uint32), np.zeros((3, 3), np.uint64)
        op, os_ = out.ctypes.data_as(P), out_sse.ctypes.data_as(P)
        assert lib.pfv_encoder_probe_pframe_rd(None, y, u, v, op, os_) == BAD
        assert lib.pfv_encoder_probe_pframe_rd(e.handle, None, u, v, op, os_) == BAD
        assert lib.pfv_encoder_probe_pframe_rd(e.handle, y, None, v, op, os_) == BAD
        assert lib.pfv_encoder_probe_pframe_rd(e.handle, y, u, None, op, os_) == BAD
        assert lib.pfv_encoder_probe_pframe_rd(e.handle, y, u, v, None, os_) == BAD
        assert lib.pfv_encoder_probe_pframe_rd(e.handle, y, u, v, op, None) == BAD
        assert lib.pfv_encoder_set_pframe_quality_floor(None, 30.0) == BAD
        for bad in (math.nan, -1.0, -math.inf, -1e-300):
            assert lib.pfv_encoder_set_pframe_quality_floor(e.handle, bad) == BAD
        for good in (0.0, 35.5, math.inf, 0.0):
            assert lib.pfv_encoder_set_pframe_quality_floor(e.handle, good) == 0
        model = LadderModel(oracle, w, h, [1, 4, 9])
        sizes, sse = e.probe_pframe_rd(vf)                             # usable after every refused call
        assert np.array_equal(sizes, pp.pframe_facts(model, 0, frame)[0]) and np.array_equal(sse, pframe_sse(model, 0, frame)[0].astype(np.uint64))
        assert e.rung == 0
        e.finish()
        with pytest.raises(pkg.PfvError) as err:                       # a finished encoder
            e.probe_pframe_rd(vf)
        assert err.value.code == STATE
    finally:
        e.close()


def build_poison(exe):
    """tests/cpp/prd_floor.cpp in its `poison` mode against pprobe_cases.build_poison's seam build of the library sources on the CPU emulator"""
    emu = os.path.join(ROOT, "tests", "hipemu")
    pp.build_poison(exe + "_size_probe")                               # makes (or finds) libpfv_emu_seam.so
    lib = os.path.join(emu, "libpfv_emu_seam.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-DPRD_FLOOR_SEAM", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "prd_floor.cpp"), "-o", exe, lib, "-Wl,-rpath," + emu], check=True)


def check_poisoned(exe, tmp_path, w=50, h=38):
    """a p-frame fails behind its encode kernel (the seam fails the payload-size download): pfv_encoder_probe_pframe_rd returns PFV_ERR_STATE
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
                    os.path.join(ROOT, "tests", "cpp", "prd_floor.cpp"), "-o", exe, lib_path, "-Wl,-rpath," + os.path.dirname(lib_path)], check=True)


def check_cpp(oracle, exe, tmp_path, w=50, h=38):
    """tests/cpp/prd_floor.cpp (pfv::Encoder::probe_pframe_rd, set_pframe_quality_floor, set_rate) on the floor clip: the model's sizes, plane
    sums, rungs and bytes"""
    frames = floor_clip(w, h)
    tot = sse_facts(oracle, w, h, LADDER, 1, 0)[1][0][0].astype(np.int64).sum(axis=1)
    q = sorted(psnr_yuv(t, w, h) for t in tot)
    floor = 0.5 * (q[1] + q[2])
    em = RdEncoderModel(oracle, w, h, LADDER, rung=1, floor_p=floor)
    want_sizes, want_sse, rungs = [], [], []
    for t, f in enumerate(frames):
        if t:
            want_sizes.append(pp.pframe_facts(em.model, 0, f)[0].tolist())
            want_sse.append(pframe_sse(em.model, 0, f)[0].reshape(-1).tolist())
        em.iframe(f) if t == 0 else em.pframe(f)
        rungs.append(em.last_rung)
    yuv, out = str(tmp_path / "pfloor.yuv"), str(tmp_path / "pfloor.pfv")
    np.concatenate(frames).tofile(yuv)
    r = subprocess.run([exe, "run", str(w), str(h), ",".join(str(q) for q in LADDER), "1", repr(floor), yuv, out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 2 * (len(frames) - 1) + 1
    for t in range(len(frames) - 1):
        assert [int(x) for x in lines[2 * t].split()[1:]] == want_sizes[t]
        assert [int(x) for x in lines[2 * t + 1].split()[1:]] == want_sse[t]
    assert [int(x) for x in lines[-1].split()[1:]] == rungs and 0 < rungs[1] < len(LADDER) - 1
    assert open(out, "rb").read() == em.sb.bytes()
