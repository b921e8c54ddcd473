"""Shared checks of the i-frame rate-distortion probe (pfv_enc_probe_iframe_rd*, pfv_encoder_probe_iframe_rd) and pfv_encoder's i-frame quality
floor (include/pfv_hip_ext.h, "i-frame rate-distortion probe"), driven on the CPU emulator by tests/test_emu_rdprobe.py and on a real MI355X
by tests/test_gpu_rdprobe.py at the same small shapes.

Every expectation comes from the oracles, never from the code under test: sizes and counts as tests/probe_cases.py has them; the squared error
of a frame at rung r is numpy int64 over recon[:ph, :pw] - source of LadderModel.iframe_coef(frame, r), per plane.  Everything is compared for
equality."""
import ctypes
import io
import math
import os
import subprocess

import numpy as np
import pytest

import ladder_cases as lc
import probe_cases as pc
from ladder_cases import LADDER, DevBufs, LadderModel, frame_bytes, plane_dims
from probe_cases import FULL_LADDER, SENTINEL, content, frame_sets, options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL64 = 0xDEADBEEFDEADBEEF
NOT_ENCODABLE = pc.NOT_ENCODABLE


# ------------------------------------------------------------------ the reference
_SSE = {}


def expected_sse(oracle, w, h, qualities, frame):
    """uint64 [R, 3]: squared error per plane of the frame against its i-frame reconstruction at every rung, inside the picture"""
    key = (w, h, tuple(qualities), frame.tobytes())
    if key not in _SSE:
        model = LadderModel(oracle, w, h, qualities)
        src = lc.split(frame, w, h)
        out = []
        for r in range(len(qualities)):
            recon = model.iframe_coef(frame, r)[1]
            out.append([int(((rec[:ph, :pw].astype(np.int64) - s.astype(np.int64)) ** 2).sum()) for rec, s, (pw, ph) in zip(recon, src, plane_dims(w, h))])
        _SSE[key] = np.array(out, np.uint64)
    return _SSE[key]


def expected_many(oracle, w, h, qualities, frames):
    """(sizes [n, R], stats [n, R, 17], sse [n, R, 3])"""
    sizes, stats = pc.expected_many(oracle, w, h, qualities, frames)
    return sizes, stats, np.stack([expected_sse(oracle, w, h, qualities, f) for f in frames])


def psnr(sse, n):
    """pfv_psnr in numpy doubles"""
    return math.inf if sse == 0 else 10.0 * math.log10(255.0 * 255.0 * float(n) / float(sse))


def psnr_yuv(oracle, w, h, qualities, frame):
    tot = expected_sse(oracle, w, h, qualities, frame).astype(np.int64).sum(axis=1)
    return [psnr(int(t), frame_bytes(w, h)) for t in tot]


def check_inputs_cover(oracle):
    """with the oracle, before the library is asked: the inputs hold frames whose PSNR-YUV is not monotone over the rungs (a finer rung that
    looks worse than a coarser one), and a frame without any error at every rung (16x16 flat: 40 bytes, SSE 0 everywhere)"""
    nonmono = 0
    for fs in frame_sets(50, 38, 3):
        for f in fs:
            q = psnr_yuv(oracle, 50, 38, LADDER, f)
            nonmono += any(b > a for a, b in zip(q, q[1:]))
    print(f"rd probe inputs 50x38x3: {nonmono} of 15 frames with a coarser rung of higher PSNR-YUV than its finer neighbour")
    assert nonmono > 0
    flat = content(16, 16, "flat")
    assert any(np.array_equal(f, flat) for fs in frame_sets(16, 16, 1) for f in fs)
    assert (pc.expected(oracle, 16, 16, LADDER, flat)[0] == 40).all() and (expected_sse(oracle, 16, 16, LADDER, flat) == 0).all()


# ------------------------------------------------------------------ check 1: the session probe
class RdRig(pc.ProbeRig):
    """ProbeRig with a device buffer for the plane sums"""

    def __init__(self, pkg, ctx, w, h, qualities, n, stride=0):
        super().__init__(pkg, ctx, w, h, qualities, n, stride)
        self.sse_dev = self.bufs.put(np.zeros((n, self.R, 3), np.uint64))

    def fetch(self):
        sizes, stats = super().fetch()
        sse = np.zeros((self.n, self.R, 3), np.uint64)
        self.ctx.download(sse, self.sse_dev)
        return sizes, stats, sse

    def sentinels(self):
        self.ctx.upload(self.sizes_dev, np.full((self.n, self.R), SENTINEL, np.uint32))
        self.ctx.upload(self.stats_dev, np.full((self.n, self.R, 17), SENTINEL, np.uint32))
        self.ctx.upload(self.sse_dev, np.full((self.n, self.R, 3), SENTINEL64, np.uint64))

    def probe(self, frames, stats=True):
        self.upload(frames)
        self.sentinels()
        self.enc.probe_iframe_rd_dev(self.frames_dev, self.sizes_dev, self.sse_dev, self.stats_dev if stats else 0)
        return self.fetch()


def check_session_probe(pkg, ctx, oracle, w, h, n, lane_mapping=None, int_transform=False, qualities=LADDER, sets=None):
    """sizes, counts and plane sums of every frame set at every rung; once more without the counts (stats_dev = NULL) and through the
    host-buffer form"""
    check_inputs_cover(oracle)
    with options(pkg, ctx, lane_mapping, int_transform):
        rig = RdRig(pkg, ctx, w, h, qualities, n)
    try:
        all_sets = frame_sets(w, h, n)
        for t, frames in enumerate(all_sets if sets is None else [all_sets[i] for i in sets]):
            want_sizes, want_stats, want_sse = expected_many(oracle, w, h, qualities, frames)
            sizes, stats, sse = rig.probe(frames)
            print(f"rd probe {w}x{h}x{n} set {t}: sse[0] {sse[0].tolist()} want {want_sse[0].tolist()}")
            assert np.array_equal(stats, want_stats), (t, np.argwhere(stats != want_stats)[:4].tolist())
            assert np.array_equal(sizes, want_sizes), (t, sizes.tolist(), want_sizes.tolist())
            assert np.array_equal(sse, want_sse), (t, np.argwhere(sse != want_sse)[:4].tolist(), sse.tolist(), want_sse.tolist())
        sizes, stats, sse = rig.probe(frames, stats=False)
        assert np.array_equal(sizes, want_sizes) and np.array_equal(sse, want_sse) and (stats == SENTINEL).all()
        want_sizes, _, want_sse = expected_many(oracle, w, h, qualities, all_sets[1])
        sizes, sse = rig.enc.probe_iframe_rd(all_sets[1])
        assert np.array_equal(sizes, want_sizes) and np.array_equal(sse, want_sse)
        assert rig.enc.rung == 0
    finally:
        rig.close()


# ------------------------------------------------------------------ check 2: agreement with the shipped paths
def check_agrees_with_size_probe(pkg, ctx, oracle, w=50, h=38, n=3):
    """sizes and counts equal pfv_enc_probe_iframe_dev's on the same frames"""
    rig = RdRig(pkg, ctx, w, h, LADDER, n)
    try:
        for frames in frame_sets(w, h, n)[:2]:
            sizes, stats, _ = rig.probe(frames)
            rig.sentinels()
            rig.enc.probe_iframe_dev(rig.frames_dev, rig.sizes_dev, rig.stats_dev)
            sizes2, stats2, _ = rig.fetch()
            assert np.array_equal(sizes, sizes2) and np.array_equal(stats, stats2)
            assert np.array_equal(sizes, pc.expected_many(oracle, w, h, LADDER, frames)[0])
    finally:
        rig.close()


def check_probe_is_what_the_encoder_writes(pkg, ctx, oracle, device_entropy, w=50, h=38):
    """pfv_encoder: the probed (size, sse) of rung r == (packet_bytes - 5, sse) of the frame report when the frame is then encoded at rung r
    == the model's"""
    frames = [content(w, h, kind, seed=3) for kind in ("texture", "gradient")]
    enc = pkg.Encoder(io.BytesIO(), w, h, 30, None, ctx, device_entropy=device_entropy, frame_report=True, qualities=LADDER)
    try:
        for t, f in enumerate(frames):
            vf = pkg.VideoFrame.from_packed(w, h, f)
            want, want_sse = pc.expected(oracle, w, h, LADDER, f)[0], expected_sse(oracle, w, h, LADDER, f)
            for r in range(len(LADDER)):
                enc.set_rung(r)
                sizes, sse = enc.probe_iframe_rd(vf)
                assert np.array_equal(sizes, want) and np.array_equal(sse, want_sse), (t, r, sizes.tolist(), want.tolist(), sse.tolist(), want_sse.tolist())
                enc.encode_iframe(vf)
                rep = enc.last_report
                assert enc.rung == r and rep.packet_bytes - 5 == int(sizes[r])
                assert [int(x) for x in rep.sse] == [int(x) for x in sse[r]], (t, r, list(rep.sse), sse[r].tolist())
    finally:
        enc.close()


# ------------------------------------------------------------------ check 3: no side effects, window and stride, graph replay
def check_no_side_effects(pkg, ctx, oracle, w=50, h=38, n=3):
    """an i-frame at rung 1, then a p-frame at rung 3: prev_frame, the rung and every output of the p-frame are the model's whether or not a
    probe of OTHER frames runs between the two (device form and host-buffer form)"""
    clips = [lc.motion_clip(w, h, 61 + k, 2) for k in range(n)]
    other = frame_sets(w, h, n)[3]
    outs = []
    for with_probe in (False, True):
        rig = lc.SessionRig(pkg, ctx, w, h, LADDER, n)
        try:
            sizes_dev = rig.bufs.put(np.zeros((n, len(LADDER)), np.uint32))
            sse_dev = rig.bufs.put(np.zeros((n, len(LADDER), 3), np.uint64))
            other_dev = rig.bufs.put(other)
            rig.step(np.stack([c[0] for c in clips]), False, 1)
            if with_probe:
                before = rig.enc.prev_frame()
                rig.enc.probe_iframe_rd_dev(other_dev, sizes_dev, sse_dev)
                got, got_sse = np.zeros((n, len(LADDER)), np.uint32), np.zeros((n, len(LADDER), 3), np.uint64)
                ctx.download(got, sizes_dev)
                ctx.download(got_sse, sse_dev)
                want_sizes, _, want_sse = expected_many(oracle, w, h, LADDER, other)
                assert np.array_equal(got, want_sizes) and np.array_equal(got_sse, want_sse)
                sizes, sse = rig.enc.probe_iframe_rd(other)
                assert np.array_equal(sizes, got) and np.array_equal(sse, got_sse)
                assert rig.enc.rung == 1 and np.array_equal(rig.enc.prev_frame(), before)
            outs.append(rig.step(np.stack([c[1] for c in clips]), True, 3))
        finally:
            rig.close()
    model = LadderModel(oracle, w, h, LADDER, n)
    for k in range(n):
        model.iframe(k, clips[k][0], 1)
        mv, has, coef = model.pframe(k, clips[k][1], 3)
        pay = model.payload_p(mv, has, coef, 3)
        for out in outs:
            assert np.array_equal(out["mv"][k], mv) and np.array_equal(out["has"][k], has) and np.array_equal(out["coef"][k], coef)
            assert np.array_equal(out["prev"][k], model.prev_frame(k)) and out["payloads"][k] == pay


def check_window_stride(pkg, ctx, oracle, w=50, h=38, n=3, lane_mapping=None):
    """window (1, 2) with the frames frame_bytes + 48 apart: slots 1 and 2 exact, the entries of slot 0 left at the sentinel in all outputs"""
    with options(pkg, ctx, lane_mapping):
        rig = RdRig(pkg, ctx, w, h, LADDER, n, stride=frame_bytes(w, h) + 48)
    try:
        rig.enc.set_frame_stride(rig.stride)
        rig.enc.set_window(1, 2)
        for frames in frame_sets(w, h, n)[2:4]:
            want_sizes, want_stats, want_sse = expected_many(oracle, w, h, LADDER, frames)
            sizes, stats, sse = rig.probe(frames)
            assert (sizes[0] == SENTINEL).all() and (stats[0] == SENTINEL).all() and (sse[0] == SENTINEL64).all()
            assert np.array_equal(sizes[1:], want_sizes[1:]) and np.array_equal(stats[1:], want_stats[1:]) and np.array_equal(sse[1:], want_sse[1:])
        with pytest.raises(pkg.PfvError) as e:                          # the host-buffer form works on all slots, packed
            rig.enc.probe_iframe_rd(frames)
        assert e.value.code == pkg._lib.PFV_ERR_STATE
        rig.enc.set_window(0, n)                                        # ... and the whole session again, still strided
        sizes, stats, sse = rig.probe(frames)
        assert np.array_equal(sizes, want_sizes) and np.array_equal(stats, want_stats) and np.array_equal(sse, want_sse)
    finally:
        rig.close()


def check_graph(pkg, ctx, oracle, w=50, h=38, n=3):
    """the probe recorded once and replayed on three contents: all exact (a replay finds both accumulators as k_probe_rd_sizes left them); a
    session that has never probed cannot start inside a recording"""
    sets = frame_sets(w, h, n)
    rig = RdRig(pkg, ctx, w, h, LADDER, n)
    fresh = pkg.EncoderSession(ctx, w, h, None, n, qualities=LADDER)
    graph = pkg.Graph(ctx)
    try:
        want = expected_many(oracle, w, h, LADDER, sets[0])
        got = rig.probe(sets[0])                                        # the unrecorded call (it makes the accumulators)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        with graph:
            rig.enc.probe_iframe_rd_dev(rig.frames_dev, rig.sizes_dev, rig.sse_dev, rig.stats_dev)
            with pytest.raises(pkg.PfvError) as e:
                fresh.probe_iframe_rd_dev(rig.frames_dev, rig.sizes_dev, rig.sse_dev)
            assert e.value.code == pkg._lib.PFV_ERR_STATE and "before pfv_graph_begin" in str(e.value)
        for frames in (sets[3], sets[1], sets[4]):
            want = expected_many(oracle, w, h, LADDER, frames)
            rig.upload(frames)
            rig.sentinels()
            graph.launch()
            got = rig.fetch()
            assert all(np.array_equal(a, b) for a, b in zip(got, want))
    finally:
        graph.close()
        fresh.close()
        rig.close()


# ------------------------------------------------------------------ check 4: the quality floor
def model_floor_rung(oracle, w, h, qualities, frame, floor, budget_i):
    """the rule of pfv_encoder_set_iframe_quality_floor on the model's sizes and plane sums"""
    K = len(qualities)
    sizes = [int(x) for x in pc.expected(oracle, w, h, qualities, frame)[0]]
    tot = [int(x) for x in expected_sse(oracle, w, h, qualities, frame).astype(np.int64).sum(axis=1)]
    allowed = [r for r in range(K) if sizes[r] != NOT_ENCODABLE and (not budget_i or sizes[r] <= budget_i)]
    if not allowed:
        return K - 1
    meets = [r for r in allowed if psnr(tot[r], frame_bytes(w, h)) >= floor]
    if meets:
        return min(meets, key=lambda r: (sizes[r], r))
    return min(allowed, key=lambda r: (tot[r], sizes[r], r))


def model_floor_run(oracle, w, h, qualities, frames, plan, floor, budget_i, budget_p):
    """pfv_encoder's rules on the model -> (stream bytes, rung of every frame); floor 0: probe_cases.model_budget_run"""
    if not floor:
        return pc.model_budget_run(oracle, w, h, qualities, frames, plan, budget_i, budget_p)
    model = LadderModel(oracle, w, h, qualities)
    K = len(qualities)
    sb = model.builder()
    rung, rungs = 0, []
    for f, kind in zip(frames, plan):
        if kind == "I":
            if K > 1:
                rung = model_floor_rung(oracle, w, h, qualities, f, floor, budget_i)
            sb.iframe(model.iframe(0, f, rung), model.qidx(rung, False))
            rungs.append(rung)
        else:
            mv, has, coef = model.pframe(0, f, rung)
            sb.pframe(mv, has, coef, model.qidx(rung, True))
            rungs.append(rung)
            n = len(sb.parts[-1]) - 5
            if budget_p:
                if n > budget_p:
                    rung = min(rung + 1, K - 1)
                elif 2 * n <= budget_p:
                    rung = max(rung - 1, 0)
    return sb.bytes(), rungs


def run_floor_encoder(pkg, ctx, w, h, qualities, frames, plan, device_entropy, floor, budget_i, budget_p, call=True, quality=None, auto=False):
    """`call` False: pfv_encoder_set_iframe_quality_floor is never called; `auto`: the i-frames of the plan through pfv_encoder_encode_frame
    (a first frame is a forced i-frame there)"""
    buf = io.BytesIO()
    enc = pkg.Encoder(buf, w, h, 30, quality, ctx, device_entropy=device_entropy, qualities=qualities)
    rungs = []
    try:
        if call:
            enc.set_iframe_quality_floor(floor)
        if budget_i:
            enc.set_iframe_budget(budget_i)
        if budget_p:
            enc.set_rate(budget_p)
        for t, (f, kind) in enumerate(zip(frames, plan)):
            vf = pkg.VideoFrame.from_packed(w, h, f)
            if kind == "I" and auto and t == 0:
                assert enc.encode_frame(vf) == 1
            elif kind == "I":
                enc.encode_iframe(vf)
            else:
                enc.encode_pframe(vf)
            rungs.append(enc.rung)
        enc.finish()
    finally:
        enc.close()
    return buf.getvalue(), rungs


def midway(a, b):
    return 0.5 * (a + b)


def check_floor(pkg, ctx, oracle, device_entropy, w=50, h=38):
    K = len(LADDER)
    clip = pc.budget_clip(w, h)
    grad = content(w, h, "gradient", seed=3)
    model = LadderModel(oracle, w, h, LADDER)
    model.iframe(0, clip[0], 2)
    bp = int(1.25 * len(model.payload_p(*model.pframe(0, clip[1], 2), 2)))            # as ladder_cases.rate_budget
    p0 = psnr_yuv(oracle, w, h, LADDER, clip[0])
    s0 = [int(x) for x in pc.expected(oracle, w, h, LADDER, clip[0])[0]]
    pg = psnr_yuv(oracle, w, h, LADDER, grad)
    sg = [int(x) for x in pc.expected(oracle, w, h, LADDER, grad)[0]]
    print(f"floor model: clip frame 0 sizes {s0} psnr {[round(x, 3) for x in p0]}; gradient sizes {sg} psnr {[round(x, 3) for x in pg]}")
    assert sg == [2792, 1028, 725, 660, 577] and [round(x, 2) for x in pg] == [31.18, 32.59, 31.30, 30.18, 28.79]
    mid = sorted(range(K), key=lambda r: p0[r])                                        # rungs of clip frame 0 by fidelity

    def first_rung(frame, floor, bi=0):
        return model_floor_rung(oracle, w, h, LADDER, frame, floor, bi)

    # every case: (frames, plan, floor, i-frame budget, the outcome it has to land on -- asserted from the model first)
    cases = []
    lo = min(p0) - 1.0                                                                 # every rung meets it: the fewest bytes = the coarsest rung
    assert first_rung(clip[0], lo) == K - 1 and s0[K - 1] == min(s0)
    cases.append((clip, pc.BUDGET_PLAN, lo, 0, "coarsest"))
    between = midway(p0[mid[1]], p0[mid[2]])                                           # midway between two rungs' model PSNRs
    r_mid = first_rung(clip[0], between)
    assert 0 < r_mid < K - 1, (r_mid, p0)
    cases.append((clip, pc.BUDGET_PLAN, between, 0, "middle"))
    for eps, want_rung in ((-1e-9, r_mid), (1e-9, r_mid - 1)):                         # at a model value -+ 1e-9 dB: just met, just missed
        assert first_rung(clip[0], p0[r_mid] + eps) == want_rung and s0[r_mid - 1] > s0[r_mid]
        cases.append((clip, pc.BUDGET_PLAN, p0[r_mid] + eps, 0, "just met" if eps < 0 else "just missed"))
    totg = expected_sse(oracle, w, h, LADDER, grad).astype(np.int64).sum(axis=1)
    none = max(pg) + 1.0                                                               # none meets the floor: the smallest SSE, which is
    assert first_rung(grad, none) == int(np.argmin(totg)) == 1                         # neither the finest rung nor the one with the fewest bytes
    cases.append(([grad, clip[1], clip[3]], "IPI", none, 0, "none meets"))
    assert first_rung(grad, 31.0) == 2 and sg[2] == 725 and first_rung(grad, 32.0) == 1   # the dominated rung 0 is skipped
    cases.append(([grad, grad], "II", 31.0, 0, "dominated skipped"))
    cases.append(([grad, grad], "IP", 32.0, 0, "dominated skipped"))
    assert first_rung(grad, math.inf) == 1                                             # the best-looking rung
    cases.append(([grad, clip[0]], "II", math.inf, 0, "+inf"))
    bi = sg[1] - 1                                                                      # the budget excludes the rung the floor alone would take
    r_b = first_rung(grad, 32.0, bi)
    assert first_rung(grad, 32.0) == 1 and r_b != 1 and sg[r_b] <= bi
    cases.append(([grad, clip[1]], "IP", 32.0, bi, "floor and budget"))
    assert first_rung(grad, 32.0, sg[K - 1] - 1) == K - 1                              # nothing allowed: the coarsest
    cases.append(([grad], "I", 32.0, sg[K - 1] - 1, "nothing allowed"))
    for frames, plan, floor, budget_i, name in cases:
        want, rungs = model_floor_run(oracle, w, h, LADDER, frames, plan, floor, budget_i, bp)
        data, got = run_floor_encoder(pkg, ctx, w, h, LADDER, frames, plan, device_entropy, floor, budget_i, bp)
        print(f"floor {floor!r} budget {budget_i} ({name}): rungs {got}, model {rungs}")
        assert got == rungs, (name, floor, got, rungs)
        assert data == want, (name, len(data), len(want))
    # pfv_encoder_encode_frame reaches the rule through encode_iframe
    want, rungs = model_floor_run(oracle, w, h, LADDER, [grad, grad], "IP", 32.0, 0, bp)
    data, got = run_floor_encoder(pkg, ctx, w, h, LADDER, [grad, grad], "IP", device_entropy, 32.0, 0, bp, auto=True)
    assert got == rungs and rungs[0] == 1 and data == want
    # floor 0: today's encoder byte for byte, with and without the call; with a budget the budget rule's bytes
    for budget_i in (0, s0[2]):
        want, rungs = pc.model_budget_run(oracle, w, h, LADDER, clip, pc.BUDGET_PLAN, budget_i, bp)
        for call in (True, False):
            data, got = run_floor_encoder(pkg, ctx, w, h, LADDER, clip, pc.BUDGET_PLAN, device_entropy, 0.0, budget_i, bp, call=call)
            assert got == rungs and data == want, (budget_i, call, got, rungs)
        assert (data, got) == pc.run_budget_encoder(pkg, ctx, w, h, LADDER, clip, pc.BUDGET_PLAN, device_entropy, budget_i, bp)


def check_floor_ties_and_one_rung(pkg, ctx, oracle, device_entropy):
    """16x16 flat: 40 bytes and no error at every rung -- any floor takes rung 0 (ties go to the lower index); a one-rung encoder never
    probes and writes today's bytes"""
    w, h = 16, 16
    f = content(w, h, "flat")
    for floor in (30.0, math.inf):
        assert model_floor_rung(oracle, w, h, LADDER, f, floor, 0) == 0
        want, rungs = model_floor_run(oracle, w, h, LADDER, [f, f], "IP", floor, 0, 0)
        data, got = run_floor_encoder(pkg, ctx, w, h, LADDER, [f, f], "IP", device_entropy, floor, 0, 0)
        assert got == rungs == [0, 0] and data == want
    w, h = 50, 38
    frames = lc.motion_clip(w, h, 73, 2)
    plain, _ = run_floor_encoder(pkg, ctx, w, h, None, frames, "IP", device_entropy, 0.0, 0, 0, call=False, quality=4)
    for floor in (1.0, 99.0, math.inf):
        data, rungs = run_floor_encoder(pkg, ctx, w, h, None, frames, "IP", device_entropy, floor, 0, 0, quality=4)
        assert data == plain and rungs == [0, 0]
    e = pkg.Encoder(io.BytesIO(), w, h, 30, None, ctx, qualities=[4], iframe_quality_floor=40.0)
    try:
        e.encode_iframe(pkg.VideoFrame.from_packed(w, h, frames[0]))
        assert e.rung == 0 and e.n_rungs == 1
    finally:
        e.close()


# ------------------------------------------------------------------ check 5: arguments
def check_arguments(pkg, ctx, oracle, w=50, h=38):
    L, lib = pkg._lib, ctx._lib
    BAD = L.PFV_ERR_BAD_ARG
    P = ctypes.c_void_p
    frame = content(w, h, "texture", seed=9)
    vf = pkg.VideoFrame.from_packed(w, h, frame)
    bufs = DevBufs(ctx)
    s = pkg.EncoderSession(ctx, w, h, 4, 1)                            # one rung: one size, three sums
    try:
        frames_dev, sizes_dev, sse_dev = bufs.put(frame), bufs.put(np.zeros(1, np.uint32)), bufs.put(np.zeros(3, np.uint64))
        host, host_sse = np.zeros(1, np.uint32), np.zeros(3, np.uint64)
        hp, hs, fp = host.ctypes.data_as(P), host_sse.ctypes.data_as(P), frame.ctypes.data_as(P)
        assert lib.pfv_enc_probe_iframe_rd_dev(None, P(frames_dev), P(sizes_dev), P(sse_dev), None) == BAD
        assert lib.pfv_enc_probe_iframe_rd_dev(s.handle, None, P(sizes_dev), P(sse_dev), None) == BAD
        assert lib.pfv_enc_probe_iframe_rd_dev(s.handle, P(frames_dev), None, P(sse_dev), None) == BAD
        assert lib.pfv_enc_probe_iframe_rd_dev(s.handle, P(frames_dev), P(sizes_dev), None, None) == BAD
        assert lib.pfv_enc_probe_iframe_rd(None, fp, hp, hs) == BAD
        assert lib.pfv_enc_probe_iframe_rd(s.handle, None, hp, hs) == BAD
        assert lib.pfv_enc_probe_iframe_rd(s.handle, fp, None, hs) == BAD
        assert lib.pfv_enc_probe_iframe_rd(s.handle, fp, hp, None) == BAD
        want, want_sse = pc.expected(oracle, w, h, [4], frame)[0], expected_sse(oracle, w, h, [4], frame)
        sizes, sse = s.probe_iframe_rd(frame)
        assert sizes.shape == (1, 1) and sse.shape == (1, 1, 3) and np.array_equal(sizes[0], want) and np.array_equal(sse[0], want_sse)
        s.probe_iframe_rd_dev(frames_dev, sizes_dev, sse_dev)          # usable after every refused call
        ctx.download(host, sizes_dev)
        ctx.download(host_sse, sse_dev)
        assert np.array_equal(host, want) and np.array_equal(host_sse, want_sse[0])
    finally:
        s.close()
        bufs.close()
    y, u, v = (pl.pixels.ctypes.data_as(P) for pl in (vf.plane_y, vf.plane_u, vf.plane_v))
    e = pkg.Encoder(io.BytesIO(), w, h, 30, None, ctx, qualities=[1, 4, 9])
    try:
        out, out_sse = np.zeros(3, np.uint32), np.zeros((3, 3), np.uint64)
        op, os_ = out.ctypes.data_as(P), out_sse.ctypes.data_as(P)
        assert lib.pfv_encoder_probe_iframe_rd(None, y, u, v, op, os_) == BAD
        assert lib.pfv_encoder_probe_iframe_rd(e.handle, None, u, v, op, os_) == BAD
        assert lib.pfv_encoder_probe_iframe_rd(e.handle, y, u, v, None, os_) == BAD
        assert lib.pfv_encoder_probe_iframe_rd(e.handle, y, u, v, op, None) == BAD
        assert lib.pfv_encoder_set_iframe_quality_floor(None, 30.0) == BAD
        for bad in (math.nan, -1.0, -math.inf, -1e-300):
            assert lib.pfv_encoder_set_iframe_quality_floor(e.handle, bad) == BAD
        for good in (0.0, 35.5, math.inf, 0.0):
            assert lib.pfv_encoder_set_iframe_quality_floor(e.handle, good) == 0
        sizes, sse = e.probe_iframe_rd(vf)
        assert np.array_equal(sizes, pc.expected(oracle, w, h, [1, 4, 9], frame)[0]) and np.array_equal(sse, expected_sse(oracle, w, h, [1, 4, 9], frame))
        assert e.rung == 0
    finally:
        e.close()


# ------------------------------------------------------------------ check 6: the C++ mirror
def build_cpp(lib_path, exe):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "rd_floor.cpp"), "-o", exe, lib_path, "-Wl,-rpath," + os.path.dirname(lib_path)], check=True)


def check_cpp(oracle, exe, tmp_path, w=50, h=38):
    """tests/cpp/rd_floor.cpp (pfv::Encoder::probe_iframe_rd, set_iframe_quality_floor, set_rate) on the budget clip: the model's sizes, plane
    sums, rungs and bytes"""
    frames = pc.budget_clip(w, h)
    p0 = psnr_yuv(oracle, w, h, LADDER, frames[0])
    order = sorted(range(len(LADDER)), key=lambda r: p0[r])
    floor = midway(p0[order[1]], p0[order[2]])
    model = LadderModel(oracle, w, h, LADDER)
    model.iframe(0, frames[0], 2)
    bp = int(1.25 * len(model.payload_p(*model.pframe(0, frames[1], 2), 2)))
    want, rungs = model_floor_run(oracle, w, h, LADDER, frames, pc.BUDGET_PLAN, floor, 0, bp)
    yuv, out = str(tmp_path / "floor.yuv"), str(tmp_path / "floor.pfv")
    np.concatenate(frames).tofile(yuv)
    r = subprocess.run([exe, str(w), str(h), ",".join(str(q) for q in LADDER), repr(floor), str(bp), "3", yuv, out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 2 * len(frames) + 1
    for t, f in enumerate(frames):
        assert [int(x) for x in lines[2 * t].split()[1:]] == pc.expected(oracle, w, h, LADDER, f)[0].tolist()
        assert [int(x) for x in lines[2 * t + 1].split()[1:]] == expected_sse(oracle, w, h, LADDER, f).reshape(-1).tolist()
    assert [int(x) for x in lines[-1].split()[1:]] == rungs and 0 < rungs[0] < len(LADDER) - 1
    assert open(out, "rb").read() == want
