"""Shared checks of the i-frame size probe (pfv_enc_probe_iframe*, pfv_encoder_probe_iframe) and pfv_encoder's i-frame byte budget
(include/pfv_hip_ext.h, "i-frame size probe"), driven on the CPU emulator by tests/test_emu_probe.py and on a real MI355X by
tests/test_gpu_probe.py at the same small shapes.

Every expectation comes from the oracles, never from the code under test: the size of a frame at rung r is the length of the payload that the
oracle's serialiser writes for the ladder model's coefficients, len(LadderModel.payload_i(LadderModel.iframe_coef(frame, r)[0], r)); the counts
are pfv_oracle_entropy_np.histogram of those coefficients and the sum of coeff_size over the non-zero ones.  Everything is compared for
equality."""
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest

import ladder_cases as lc
import pfv_oracle_entropy_np as enp
from ladder_cases import LADDER, SHAPES, DevBufs, LadderModel, frame_bytes, plane_dims

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_LADDER = list(range(11))
KINDS = ["flat", "gradient", "texture", "noise", "checker"]
# ladder_cases.INTERIOR_SHAPES for the i-frame probes: (w, h, n_streams, lane mapping, integer transform) -- both mappings and both transforms
# at 400x80, the context's mapping and the float transform at 544x96 x 2
INTERIOR_CASES = [(400, 80, 1, 1, False), (400, 80, 1, 1, True), (400, 80, 1, 2, False), (400, 80, 1, 2, True), (544, 96, 2, None, False)]
INTERIOR_IDS = ["400x80x1-lanes8-f32", "400x80x1-lanes8-i32", "400x80x1-lanes16-f32", "400x80x1-lanes16-i32", "544x96x2-f32"]
SENTINEL = 0xDEADBEEF
NOT_ENCODABLE = 0xFFFFFFFF


# ------------------------------------------------------------------ content
def content(w, h, kind, seed=0):
    """one packed frame: flat 128 / a two-axis gradient / ladder_cases.texture / uniform noise / a 0/255 checkerboard (luma: single pixels, chroma: 8x8 cells)"""
    rng = np.random.default_rng(1000 + 17 * seed + KINDS.index(kind))
    planes = []
    for p, (pw, ph) in enumerate(plane_dims(w, h)):
        yy, xx = np.meshgrid(np.arange(ph), np.arange(pw), indexing="ij")
        if kind == "flat":
            pl = np.full((ph, pw), 128.0)
        elif kind == "gradient":
            pl = (xx / (pw - 1) * (150 - 20 * p) + yy / (ph - 1) * (105 + 20 * p) + 7 * seed) % 256     # a full-range ramp along both axes
        elif kind == "texture":
            pl = lc.texture(rng, 64)[(yy + 7 * p) % 64, (xx + 3 * seed) % 64]
        elif kind == "noise":
            pl = rng.integers(0, 256, (ph, pw))
        else:
            cell = 8 if p else 1                     # chroma: whole 8x8 blocks of 0 or 255 (the largest DC terms: -1024 at q = 1)
            pl = ((xx // cell + yy // cell + seed + p) & 1) * 255
        planes.append(np.clip(np.rint(pl), 0, 255).astype(np.uint8).reshape(-1))
    return np.concatenate(planes)


def frame_sets(w, h, n):
    """five launches' worth of frames [5][n, frame_bytes]: stream k of set t holds kind (t + k) % 5, so every stream sees every kind and the
    streams of one launch differ"""
    return [np.stack([content(w, h, KINDS[(t + k) % 5], seed=k) for k in range(n)]) for t in range(5)]


# ------------------------------------------------------------------ the reference
_EXPECTED = {}


def coeff_sizes_sum(coef):
    c = np.abs(np.asarray(coef, np.int64).reshape(-1))
    c = c[c != 0] & 0xFFFF
    return int(sum(int(v).bit_length() + 1 for v in c.tolist()))


def expected(oracle, w, h, qualities, frame):
    """(sizes uint32 [R], stats uint32 [R, 17]) of one frame, computed once per (shape, ladder, frame)"""
    key = (w, h, tuple(qualities), frame.tobytes())
    if key not in _EXPECTED:
        model = LadderModel(oracle, w, h, qualities)
        sizes, stats = [], []
        for r in range(len(qualities)):
            coef = model.iframe_coef(frame, r)[0]
            sizes.append(len(model.payload_i(coef, r)))
            stats.append(list(enp.histogram(coef)) + [coeff_sizes_sum(coef)])
        _EXPECTED[key] = (np.array(sizes, np.uint32), np.array(stats, np.uint32))
    return _EXPECTED[key]


def expected_many(oracle, w, h, qualities, frames):
    got = [expected(oracle, w, h, qualities, f) for f in frames]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


def check_inputs_cover(oracle, w, h, n):
    """what the five frame sets exercise, established with the numpy oracle before anything is asked of the probe: every num_zeroes symbol
    0..15, fillers, runs that cross a subblock boundary, closing runs, coefficient sizes of 12 bits and more, and payload sizes that fall
    strictly from rung to rung -- except where a frame quantises to the same coefficients at every rung (flat 128 without luma padding)"""
    model = LadderModel(oracle, w, h, LADDER)
    runs, fillers, crossing, closing, max_size = np.zeros(16, np.int64), 0, 0, 0, 0
    for frames in frame_sets(w, h, n):
        for f in frames:
            sizes, _ = expected(oracle, w, h, LADDER, f)
            coefs = [model.iframe_coef(f, r)[0] for r in range(len(LADDER))]
            same = all(np.array_equal(coefs[0], c) for c in coefs[1:])
            steps = np.diff(sizes.astype(np.int64))
            assert (steps == 0).all() if same else (steps < 0).all(), (w, h, sizes)
            for coef in coefs:
                for mb in np.asarray(coef, np.int16).reshape(-1, 256):
                    nz = np.nonzero(mb)[0]
                    prev = np.concatenate([[-1], nz[:-1]]) if nz.size else nz
                    run = nz - prev - 1                                   # zeros in front of every value
                    tail = 255 - (int(nz[-1]) if nz.size else -1)         # ... and behind the last one
                    n_fill = np.where(run > 15, (run - 1) // 15, 0)
                    np.add.at(runs, run - 15 * n_fill, 1)
                    fillers += int(n_fill.sum()) + ((tail - 1) // 15 if tail > 15 else 0)
                    crossing += int((run > (nz % 64)).sum())              # the run starts in an earlier subblock
                    closing += int(tail > 0)
                    if nz.size:
                        max_size = max(max_size, max(enp.coeff_size(v) for v in mb[nz].tolist()))
    print(f"probe inputs {w}x{h}x{n}: num_zeroes counts {runs.tolist()}, fillers {fillers}, runs across subblocks {crossing}, closing runs {closing}, "
          f"largest coeff_size {max_size}")
    assert (runs > 0).all() and fillers >= 500 and crossing > 0 and closing > 0 and max_size >= 12


# ------------------------------------------------------------------ check 1: the session probe
class ProbeRig:
    """an EncoderSession with device buffers for the frames of all slots (`stride` bytes apart), the sizes and the counts"""

    def __init__(self, pkg, ctx, w, h, qualities, n, stride=0):
        self.ctx, self.n, self.R = ctx, n, len(qualities)
        self.fb, self.stride = frame_bytes(w, h), stride or frame_bytes(w, h)
        self.enc = pkg.EncoderSession(ctx, w, h, None, n, qualities=qualities)
        self.bufs = DevBufs(ctx)
        self.frames_dev = self.bufs.put(np.zeros(n * self.stride, np.uint8))
        self.sizes_dev = self.bufs.put(np.zeros((n, self.R), np.uint32))
        self.stats_dev = self.bufs.put(np.zeros((n, self.R, 17), np.uint32))

    def close(self):
        self.bufs.close()
        self.enc.close()

    def upload(self, frames):
        buf = np.full((self.n, self.stride), 0xA5, np.uint8)               # the gaps of a strided layout hold something
        buf[:, :self.fb] = frames
        self.ctx.upload(self.frames_dev, buf)

    def fetch(self):
        sizes, stats = np.zeros((self.n, self.R), np.uint32), np.zeros((self.n, self.R, 17), np.uint32)
        self.ctx.download(sizes, self.sizes_dev)
        self.ctx.download(stats, self.stats_dev)
        return sizes, stats

    def probe(self, frames, stats=True):
        """sentinels into both outputs, the frames up, one probe -> (sizes, stats) as they lie in device memory afterwards"""
        self.upload(frames)
        self.ctx.upload(self.sizes_dev, np.full((self.n, self.R), SENTINEL, np.uint32))
        self.ctx.upload(self.stats_dev, np.full((self.n, self.R, 17), SENTINEL, np.uint32))
        self.enc.probe_iframe_dev(self.frames_dev, self.sizes_dev, self.stats_dev if stats else 0)
        return self.fetch()


class options:
    """context options for the sessions created inside the block (an encoder session takes them at creation)"""

    def __init__(self, pkg, ctx, lane_mapping=None, int_transform=False):
        L = pkg._lib
        self.ctx, self.want = ctx, []
        if lane_mapping is not None:
            self.want.append((L.PFV_OPT_LANE_MAPPING, lane_mapping))
        if int_transform:
            self.want.append((L.PFV_OPT_ENC_TRANSFORM, L.PFV_ENC_TRANSFORM_INT))

    def __enter__(self):
        self.old = [(o, self.ctx.get_option(o)) for o, _ in self.want]
        for o, v in self.want:
            self.ctx.set_option(o, v)

    def __exit__(self, *a):
        for o, v in self.old:
            self.ctx.set_option(o, v)


def check_session_probe(pkg, ctx, oracle, w, h, n, lane_mapping=None, int_transform=False, qualities=LADDER, sets=None):
    """sizes and counts of every frame set at every rung; once more without the counts (stats_dev = NULL) and through the host-buffer form"""
    if tuple(qualities) == tuple(LADDER):
        check_inputs_cover(oracle, w, h, n)
    with options(pkg, ctx, lane_mapping, int_transform):
        rig = ProbeRig(pkg, ctx, w, h, qualities, n)
    try:
        all_sets = frame_sets(w, h, n)
        for t, frames in enumerate(all_sets if sets is None else [all_sets[i] for i in sets]):
            want_sizes, want_stats = expected_many(oracle, w, h, qualities, frames)
            sizes, stats = rig.probe(frames)
            assert np.array_equal(stats, want_stats), (t, np.argwhere(stats != want_stats)[:4].tolist())
            assert np.array_equal(sizes, want_sizes), (t, sizes.tolist(), want_sizes.tolist())
        sizes, stats = rig.probe(frames, stats=False)
        assert np.array_equal(sizes, want_sizes) and (stats == SENTINEL).all()
        assert np.array_equal(rig.enc.probe_iframe(all_sets[1]), expected_many(oracle, w, h, qualities, all_sets[1])[0])
        assert rig.enc.rung == 0
    finally:
        rig.close()


# ------------------------------------------------------------------ check 2: no side effects
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
            other_dev = rig.bufs.put(other)
            rig.step(np.stack([c[0] for c in clips]), False, 1)
            if with_probe:
                before = rig.enc.prev_frame()
                rig.enc.probe_iframe_dev(other_dev, sizes_dev)
                got = np.zeros((n, len(LADDER)), np.uint32)
                ctx.download(got, sizes_dev)
                assert np.array_equal(got, expected_many(oracle, w, h, LADDER, other)[0])
                assert np.array_equal(rig.enc.probe_iframe(other), got)
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


def check_probe_is_what_the_encoder_writes(pkg, ctx, oracle, device_entropy, w=50, h=38):
    """pfv_encoder: the probed size of rung r == packet_bytes - 5 of the frame report when the frame is then encoded at rung r == the model's"""
    frames = [content(w, h, kind, seed=3) for kind in ("texture", "checker")]
    enc = pkg.Encoder(io.BytesIO(), w, h, 30, None, ctx, device_entropy=device_entropy, frame_report=True, qualities=LADDER)
    try:
        for t, f in enumerate(frames):
            vf = pkg.VideoFrame.from_packed(w, h, f)
            want = expected(oracle, w, h, LADDER, f)[0]
            for r in range(len(LADDER)):
                enc.set_rung(r)
                sizes = enc.probe_iframe(vf)
                assert np.array_equal(sizes, want), (t, r, sizes.tolist(), want.tolist())
                enc.encode_iframe(vf)
                assert enc.rung == r and enc.last_report.packet_bytes - 5 == int(sizes[r])
    finally:
        enc.close()


# ------------------------------------------------------------------ check 3: window and frame stride
def check_window_stride(pkg, ctx, oracle, w=50, h=38, n=3, lane_mapping=None):
    """window (1, 2) with the frames frame_bytes + 48 apart: slots 1 and 2 exact, the entries of slot 0 left at the sentinel"""
    with options(pkg, ctx, lane_mapping):
        rig = ProbeRig(pkg, ctx, w, h, LADDER, n, stride=frame_bytes(w, h) + 48)
    try:
        rig.enc.set_frame_stride(rig.stride)
        rig.enc.set_window(1, 2)
        for frames in frame_sets(w, h, n)[2:4]:
            want_sizes, want_stats = expected_many(oracle, w, h, LADDER, frames)
            sizes, stats = rig.probe(frames)
            assert (sizes[0] == SENTINEL).all() and (stats[0] == SENTINEL).all()
            assert np.array_equal(sizes[1:], want_sizes[1:]) and np.array_equal(stats[1:], want_stats[1:])
        with pytest.raises(pkg.PfvError) as e:                          # the host-buffer form works on all slots, packed, like pfv_enc_iframe
            rig.enc.probe_iframe(frames)
        assert e.value.code == pkg._lib.PFV_ERR_STATE
        rig.enc.set_window(0, n)                                        # ... and the whole session again, still strided
        sizes, stats = rig.probe(frames)
        assert np.array_equal(sizes, want_sizes) and np.array_equal(stats, want_stats)
    finally:
        rig.close()


# ------------------------------------------------------------------ check 4: a recorded probe
def check_graph(pkg, ctx, oracle, w=50, h=38, n=3):
    """the probe recorded once and replayed on two different frame contents: both exact (a replay finds the accumulator as k_probe_sizes left
    it); a session that has never probed cannot start inside a recording"""
    sets = frame_sets(w, h, n)
    rig = ProbeRig(pkg, ctx, w, h, LADDER, n)
    fresh = pkg.EncoderSession(ctx, w, h, None, n, qualities=LADDER)
    graph = pkg.Graph(ctx)
    try:
        want_sizes, want_stats = expected_many(oracle, w, h, LADDER, sets[0])
        sizes, stats = rig.probe(sets[0])                               # the unrecorded call (it makes the accumulator)
        assert np.array_equal(sizes, want_sizes) and np.array_equal(stats, want_stats)
        with graph:
            rig.enc.probe_iframe_dev(rig.frames_dev, rig.sizes_dev, rig.stats_dev)
            with pytest.raises(pkg.PfvError) as e:
                fresh.probe_iframe_dev(rig.frames_dev, rig.sizes_dev)
            assert e.value.code == pkg._lib.PFV_ERR_STATE and "before pfv_graph_begin" in str(e.value)
        for frames in (sets[3], sets[1], sets[3]):
            want_sizes, want_stats = expected_many(oracle, w, h, LADDER, frames)
            rig.upload(frames)
            ctx.upload(rig.sizes_dev, np.full((n, rig.R), SENTINEL, np.uint32))
            ctx.upload(rig.stats_dev, np.full((n, rig.R, 17), SENTINEL, np.uint32))
            graph.launch()
            sizes, stats = rig.fetch()
            assert np.array_equal(stats, want_stats) and np.array_equal(sizes, want_sizes)
    finally:
        graph.close()
        fresh.close()
        rig.close()


# ------------------------------------------------------------------ check 5: the i-frame byte budget
BUDGET_PLAN = "IPPIP"


def model_budget_run(oracle, w, h, qualities, frames, plan, budget_i, budget_p, start_rung=0):
    """pfv_encoder's rules on the model -> (stream bytes, rung of every frame): an i-frame under a budget takes the finest rung whose model
    payload fits (the coarsest if none does) and leaves it as the current rung; p-frames follow pfv_encoder_set_rate's rule from there"""
    model = LadderModel(oracle, w, h, qualities)
    K = len(qualities)
    sb = model.builder()
    rung, rungs = start_rung, []
    for f, kind in zip(frames, plan):
        if kind == "I":
            if budget_i and K > 1:
                sizes = expected(oracle, w, h, qualities, f)[0]
                fits = [r for r in range(K) if int(sizes[r]) <= budget_i]
                rung = fits[0] if fits else K - 1
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


def run_budget_encoder(pkg, ctx, w, h, qualities, frames, plan, device_entropy, budget_i, budget_p, call=True, quality=None):
    """`call` False: pfv_encoder_set_iframe_budget is never called"""
    buf = io.BytesIO()
    enc = pkg.Encoder(buf, w, h, 30, quality, ctx, device_entropy=device_entropy, qualities=qualities)
    rungs = []
    try:
        if call:
            enc.set_iframe_budget(budget_i)
        if budget_p:
            enc.set_rate(budget_p)
        for f, kind in zip(frames, plan):
            vf = pkg.VideoFrame.from_packed(w, h, f)
            enc.encode_iframe(vf) if kind == "I" else enc.encode_pframe(vf)
            rungs.append(enc.rung)
        enc.finish()
    finally:
        enc.close()
    return buf.getvalue(), rungs


def budget_clip(w, h):
    """motion_clip with its second i-frame replaced by noise: the two i-frames of BUDGET_PLAN have very different sizes"""
    frames = lc.motion_clip(w, h, 71, len(BUDGET_PLAN))
    frames[3] = content(w, h, "noise", seed=5)
    return frames


def check_budget(pkg, ctx, oracle, device_entropy, w=50, h=38):
    frames = budget_clip(w, h)
    K = len(LADDER)
    s0, s3 = (expected(oracle, w, h, LADDER, frames[t])[0].astype(np.int64) for t in (0, 3))
    assert (np.diff(s0) < 0).all() and (np.diff(s3) < 0).all() and (s3 > s0).all()     # the second i-frame is the larger one at every rung: it lands on another rung
    model = LadderModel(oracle, w, h, LADDER)
    model.iframe(0, frames[0], 2)
    bp = int(1.25 * len(model.payload_p(*model.pframe(0, frames[1], 2), 2)))            # as ladder_cases.rate_budget
    # budgets from the model's sizes of frame 0: rung 0 (with room, and exactly), a middle rung exactly and one byte short of it, the last rung exactly,
    # none fits; and one that frame 3 meets exactly at rung 1
    budgets = [int(s0[0]) + 100, int(s0[0]), int(s0[2]), int(s0[2]) - 1, int(s0[K - 1]), int(s0[K - 1]) - 1, int(s3[1])]
    first_rungs = set()
    for bi in budgets:
        want, rungs = model_budget_run(oracle, w, h, LADDER, frames, BUDGET_PLAN, bi, bp)
        data, got = run_budget_encoder(pkg, ctx, w, h, LADDER, frames, BUDGET_PLAN, device_entropy, bi, bp)
        assert got == rungs, (bi, got, rungs)
        assert data == want, (bi, len(data), len(want))
        first_rungs.add((rungs[0], bi < s0[rungs[0]]))
    print(f"i-frame budgets {budgets}: (rung of frame 0, over budget) {sorted(first_rungs)}")
    assert {(0, False), (2, False), (3, False), (K - 1, False), (K - 1, True)} <= first_rungs
    # budget 0: today's encoder byte for byte, whether or not the call is made; the rung moves by set_rate alone
    want, rungs = model_budget_run(oracle, w, h, LADDER, frames, BUDGET_PLAN, 0, bp, start_rung=0)
    for call in (True, False):
        data, got = run_budget_encoder(pkg, ctx, w, h, LADDER, frames, BUDGET_PLAN, device_entropy, 0, bp, call=call)
        assert got == rungs and data == want


def check_budget_equal_sizes(pkg, ctx, oracle, device_entropy):
    """flat 16x16: 40 bytes at every rung -- a budget of 40 takes rung 0 (the scan starts at the finest), 39 the coarsest"""
    w, h = 16, 16
    f = content(w, h, "flat")
    sizes = expected(oracle, w, h, LADDER, f)[0]
    assert (sizes == 40).all()
    for bi, rung in ((40, 0), (39, len(LADDER) - 1)):
        want, rungs = model_budget_run(oracle, w, h, LADDER, [f, f], "IP", bi, 0)
        data, got = run_budget_encoder(pkg, ctx, w, h, LADDER, [f, f], "IP", device_entropy, bi, 0)
        assert got == rungs == [rung, rung] and data == want


# ------------------------------------------------------------------ check 6: arguments
def check_arguments(pkg, ctx, oracle, w=50, h=38):
    L, lib = pkg._lib, ctx._lib
    BAD = L.PFV_ERR_BAD_ARG
    P = ctypes.c_void_p
    frame = content(w, h, "texture", seed=9)
    vf = pkg.VideoFrame.from_packed(w, h, frame)
    bufs = DevBufs(ctx)
    s = pkg.EncoderSession(ctx, w, h, 4, 1)                            # one rung: one size
    try:
        frames_dev, sizes_dev = bufs.put(frame), bufs.put(np.zeros(1, np.uint32))
        host = np.zeros(1, np.uint32)
        assert lib.pfv_enc_probe_iframe_dev(None, P(frames_dev), P(sizes_dev), None) == BAD
        assert lib.pfv_enc_probe_iframe_dev(s.handle, None, P(sizes_dev), None) == BAD
        assert lib.pfv_enc_probe_iframe_dev(s.handle, P(frames_dev), None, None) == BAD
        assert lib.pfv_enc_probe_iframe(None, frame.ctypes.data_as(P), host.ctypes.data_as(P)) == BAD
        assert lib.pfv_enc_probe_iframe(s.handle, None, host.ctypes.data_as(P)) == BAD
        assert lib.pfv_enc_probe_iframe(s.handle, frame.ctypes.data_as(P), None) == BAD
        want = expected(oracle, w, h, [4], frame)[0]
        got = s.probe_iframe(frame)
        assert got.shape == (1, 1) and np.array_equal(got[0], want)
        s.probe_iframe_dev(frames_dev, sizes_dev)                      # usable after every refused call
        ctx.download(host, sizes_dev)
        assert np.array_equal(host, want)
    finally:
        s.close()
        bufs.close()
    y, u, v = (pl.pixels.ctypes.data_as(P) for pl in (vf.plane_y, vf.plane_u, vf.plane_v))
    e = pkg.Encoder(io.BytesIO(), w, h, 30, None, ctx, qualities=[1, 4, 9])
    try:
        out = np.zeros(3, np.uint32)
        assert lib.pfv_encoder_set_iframe_budget(None, 1) == BAD
        assert lib.pfv_encoder_probe_iframe(None, y, u, v, out.ctypes.data_as(P)) == BAD
        assert lib.pfv_encoder_probe_iframe(e.handle, None, u, v, out.ctypes.data_as(P)) == BAD
        assert lib.pfv_encoder_probe_iframe(e.handle, y, u, v, None) == BAD
        assert np.array_equal(e.probe_iframe(vf), expected(oracle, w, h, [1, 4, 9], frame)[0]) and e.rung == 0
    finally:
        e.close()
    # a one-rung encoder under any budget chooses rung 0 and writes today's bytes
    frames = lc.motion_clip(w, h, 73, 2)
    plain, _ = run_budget_encoder(pkg, ctx, w, h, None, frames, "IP", True, 0, 0, call=False, quality=4)
    for bi in (1, 10 ** 6):
        data, rungs = run_budget_encoder(pkg, ctx, w, h, None, frames, "IP", True, bi, 0, quality=4)
        assert data == plain and rungs == [0, 0]
    e = pkg.Encoder(io.BytesIO(), w, h, 30, None, ctx, qualities=[4], iframe_budget=1)
    try:
        e.encode_iframe(vf)
        assert e.rung == 0 and e.n_rungs == 1
    finally:
        e.close()


# ------------------------------------------------------------------ check 7: the C++ mirror
def build_cpp(lib_path, exe):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "probe_budget.cpp"), "-o", exe, lib_path, "-Wl,-rpath," + os.path.dirname(lib_path)], check=True)


def check_cpp(oracle, exe, tmp_path, w=50, h=38):
    """tests/cpp/probe_budget.cpp (pfv::Encoder::probe_iframe, set_iframe_budget, set_rate) on the budget clip: the model's sizes, rungs and bytes"""
    frames = budget_clip(w, h)
    s0 = expected(oracle, w, h, LADDER, frames[0])[0]
    model = LadderModel(oracle, w, h, LADDER)
    model.iframe(0, frames[0], 2)
    bp = int(1.25 * len(model.payload_p(*model.pframe(0, frames[1], 2), 2)))
    bi = int(s0[2])
    want, rungs = model_budget_run(oracle, w, h, LADDER, frames, BUDGET_PLAN, bi, bp)
    yuv, out = str(tmp_path / "budget.yuv"), str(tmp_path / "budget.pfv")
    np.concatenate(frames).tofile(yuv)
    r = subprocess.run([exe, str(w), str(h), ",".join(str(q) for q in LADDER), str(bi), str(bp), "3", yuv, out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(frames) + 1
    for f, line in zip(frames, lines):
        assert [int(x) for x in line.split()[1:]] == expected(oracle, w, h, LADDER, f)[0].tolist()
    assert [int(x) for x in lines[-1].split()[1:]] == rungs and rungs[0] == 2
    assert open(out, "rb").read() == want
