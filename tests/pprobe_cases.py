"""Shared checks of the p-frame size probe (pfv_enc_probe_pframe*, pfv_encoder_probe_pframe), pfv_encoder's hard p-frame budget
(pfv_encoder_set_pframe_probe) and its automatic frame type (pfv_encoder_encode_frame, pfv_encoder_set_gop; include/pfv_hip_ext.h, "p-frame size
probe"), driven on the CPU emulator by tests/test_emu_pprobe.py and on a real MI355X by tests/test_gpu_pprobe.py at the same small shapes.

Every expectation comes from the oracles, never from the code under test: the size of a frame at rung r is the length of the payload that the
oracle's serialiser writes for what the ladder model's p-frame encoder produces on a COPY of its prev planes,
len(LadderModel.payload_p(*copy.pframe(k, frame, r), r)); the counts are pfv_oracle_entropy_np.histogram over the coded macroblocks, the sum of
coeff_size over their non-zero values, the coded macroblocks, the macroblocks with a non-zero vector and 2 header bits per macroblock + 14 per
non-zero vector.  I-frame sizes are probe_cases.expected.  Everything is compared for equality."""
import copy
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest

import ladder_cases as lc
import pfv_oracle_entropy_np as enp
import probe_cases as pc
from ladder_cases import LADDER, DevBufs, LadderModel, frame_bytes
from probe_cases import FULL_LADDER, SENTINEL, content, options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (w, h, n_streams).  16x16: one macroblock per plane, no room to move; 18x34: partial edge macroblocks; 130x18: two strips in a row;
# 34x82: six macroblock rows = two stacked tiles, chroma 17x41; 50x38 x 3: stream indexing
SHAPES = [(16, 16, 1), (18, 34, 1), (130, 18, 1), (34, 82, 1), (50, 38, 3)]
INTERIOR_SHAPES = lc.INTERIOR_SHAPES                     # the p-frame probes search their strips without bounds tests: interior_mbs below
INTERIOR_CASES = [(400, 80, 1, False), (400, 80, 1, True), (544, 96, 2, False)]                  # (w, h, n_streams, integer transform)
INTERIOR_IDS = ["400x80x1-f32", "400x80x1-i32", "544x96x2-f32"]
NSTATS = 20
CODED, MOVED, HDR = 17, 18, 19
CONTENT_KINDS = ["checker", "gradient", "noise", "texture"]
FRAME_NAMES = ["same", "pan1", "pan4"] + CONTENT_KINDS
NOTHING_CODED_BYTES = {(50, 38): 24, (16, 16): 20}       # 20 macroblocks: (152 + 40 + 7) >> 3; 3 macroblocks: (152 + 6 + 7) >> 3


# ------------------------------------------------------------------ states and frames
def clips(w, h, n):
    """seed 61 as in the probe's table of cases; at 34x82 that clip's own first frame finds a non-zero vector against its reconstruction at every
    rung, so no (frame, rung) pair is left with nothing coded and nothing moved -- seed 63 there (the content changes, check_inputs_cover does not)"""
    seed = 63 if (w, h) == (34, 82) else 61
    return [lc.motion_clip(w, h, seed + k, 7) for k in range(n)]


def state_frames(w, h, n, state):
    """the frames probed in state 0 (behind clip[0] as an i-frame at rung 1) and state 1 (behind clip[1] as a p-frame at rung 2 on top of that):
    [7][n, frame_bytes] -- the frame the state was made from, the clip one step on, four steps on (vector components of 4 and 8), and four
    contents of probe_cases"""
    cl = clips(w, h, n)
    sets = [np.stack([cl[k][state + d] for k in range(n)]) for d in (0, 1, 4)]
    sets += [np.stack([content(w, h, kind, seed=k + 3 * state) for k in range(n)]) for kind in CONTENT_KINDS]
    return sets


def model_in_state(oracle, w, h, qualities, n, state):
    """ladder rungs 1 and 2 are named by index: both ladders of the tests have them"""
    model = LadderModel(oracle, w, h, qualities, n)
    cl = clips(w, h, n)
    for k in range(n):
        model.iframe(k, cl[k][0], 1)
        if state:
            model.pframe(k, cl[k][1], 2)
    return model


def pframe_facts(model, k, frame):
    """what the model's p-frame of `frame` in stream k looks like at every rung, prev untouched -> (sizes [R], stats [R, 20], has [R][tb],
    mv [R][tb, 2])"""
    sizes, stats, hass, mvs = [], [], [], []
    for r in range(len(model.qualities)):
        m = copy.copy(model)
        m.prev = [list(p) for p in model.prev]                 # pframe() replaces prev[k]: a copy of the lists is a copy of the state
        mv, has, coef = m.pframe(k, frame, r)
        mv2 = np.asarray(mv).reshape(-1, 2)
        moved = int((mv2 != 0).any(axis=1).sum())
        sizes.append(len(model.payload_p(mv, has, coef, r)))
        coded = np.asarray(coef, np.int16).reshape(-1, 256)[np.asarray(has).astype(bool)]
        stats.append(list(enp.histogram(coef, has)) + [pc.coeff_sizes_sum(coded), int(np.asarray(has).sum()), moved, 2 * model.tb + 14 * moved])
        hass.append(np.asarray(has).astype(bool))
        mvs.append(mv2)
    return np.array(sizes, np.uint32), np.array(stats, np.uint32), hass, mvs


_FACTS = {}


def facts(oracle, w, h, qualities, n, state, sets=None):
    """per frame set of state_frames (all, or those named by `sets`: None elsewhere): (sizes [n, R], stats [n, R, 20], has [n][R], mv [n][R]);
    computed once per (shape, ladder, state)"""
    key = (w, h, tuple(qualities), n, state, None if sets is None else tuple(sets))
    if key not in _FACTS:
        model = model_in_state(oracle, w, h, qualities, n, state)
        out = []
        for t, frames in enumerate(state_frames(w, h, n, state)):
            if sets is not None and t not in sets:
                out.append(None)
                continue
            per = [pframe_facts(model, k, frames[k]) for k in range(n)]
            out.append((np.stack([p[0] for p in per]), np.stack([p[1] for p in per]), [p[2] for p in per], [p[3] for p in per]))
        _FACTS[key] = out
    return _FACTS[key]


# ------------------------------------------------------------------ check 1: what the inputs exercise (the oracle alone)
def check_inputs_cover(oracle, w, h, n):
    all_coded = some_coded = none_coded = big_vector = still = skipped_moved = i_both = 0
    for state in (0, 1):
        fsets = state_frames(w, h, n, state)
        for (sizes, stats, hass, mvs), frames in zip(facts(oracle, w, h, LADDER, n, state), fsets):
            for k in range(n):
                isizes = pc.expected(oracle, w, h, LADDER, frames[k])[0]
                le = isizes.astype(np.int64) <= sizes[k].astype(np.int64)
                i_both += int(le.any() and not le.all())                  # a rung where the i-frame is not larger and one where it is, on ONE frame
                for r in range(len(LADDER)):
                    has, mv = hass[k][r], mvs[k][r]
                    nz = (mv != 0).any(axis=1)
                    all_coded += int(has.all())
                    some_coded += int(has.any() and not has.all())
                    none_coded += int(not has.any())
                    big_vector += int((np.abs(mv) >= 4).any())
                    still += int(not has.any() and not nz.any())
                    skipped_moved += int((~has & nz).any())
    print(f"p-probe inputs {w}x{h}x{n}: (frame, rung) pairs all coded {all_coded}, some {some_coded}, none {none_coded}, |mv| >= 4 {big_vector}, "
          f"nothing coded and nothing moved {still}, skipped with a vector {skipped_moved}; frames with the i-frame not larger at one rung and larger at another {i_both}")
    assert all_coded and some_coded and none_coded and still
    # 16x16: every padded plane is exactly one macroblock, so the only candidate inside the plane (src/common.rs:171, :182) is (0, 0): no vector
    assert (big_vector and skipped_moved) or (w, h) == (16, 16)
    assert i_both


def interior_mbs(pw, ph):
    """the macroblocks (row-major indices in a padded plane of pw x ph) of the strips that penc_search searches without bounds tests.  Its rule,
    restated: a strip is 8 macroblocks of one macroblock row from x0 = 128 sx, y0 = 16 by; it is interior when x0 >= 16, x0 + 8 * 16 + 16 <= pw,
    y0 >= 16 and y0 + 32 <= ph"""
    bw, bh = pw // 16, ph // 16
    out = []
    for by in range(bh):
        for sx in range((bw + 7) // 8):
            x0, y0 = 128 * sx, 16 * by
            if x0 >= 16 and x0 + 8 * 16 + 16 <= pw and y0 >= 16 and y0 + 32 <= ph:
                out += [by * bw + 8 * sx + m for m in range(8)]
    return out


def frame_interior_mbs(w, h):
    """per plane: interior_mbs as indices into the frame's macroblock list (the planes' lists one behind the other)"""
    out, off = [], 0
    for pw, ph in lc.plane_dims(w, h):
        pw, ph = lc.pad16(pw), lc.pad16(ph)
        out.append(np.array(interior_mbs(pw, ph), np.int64) + off)
        off += (pw // 16) * (ph // 16)
    return out


def check_interior_inputs(oracle, w, h, n, sets=None):
    """of the MODEL alone, for a shape of INTERIOR_SHAPES: interior strips exist (in luma; at 544x96 in both chroma planes too), and over the
    frame sets probed their macroblocks hold, at some rung, a vector with an odd component, one with a component of 4 or more, a zero vector, a
    coded and a skipped macroblock -- in every plane that has interior strips, so that no plane's unchecked search is compared on zeros alone"""
    per_plane = frame_interior_mbs(w, h)
    assert [len(x) for x in per_plane] == {(400, 80): [48, 0, 0], (544, 96): [96, 8, 8]}[(w, h)]
    # the smallest plane with an interior strip, and one step less either way
    assert interior_mbs(272, 48) == list(range(17 + 8, 17 + 16)) and not interior_mbs(256, 48) and not interior_mbs(272, 32)
    for p, idx in enumerate(per_plane):
        if not len(idx):
            continue
        odd = big = zero = coded = skipped = 0
        for state in (0, 1):
            for got in facts(oracle, w, h, LADDER, n, state, sets):
                if got is None:
                    continue
                for k in range(n):
                    for r in range(len(LADDER)):
                        has, mv = got[2][k][r][idx], got[3][k][r][idx].astype(np.int64)
                        odd += int((mv & 1).any(axis=1).sum())
                        big += int((np.abs(mv) >= 4).any(axis=1).sum())
                        zero += int((mv == 0).all(axis=1).sum())
                        coded += int(has.sum())
                        skipped += int((~has).sum())
        print(f"p-probe interior inputs {w}x{h}x{n} plane {p}: {len(idx)} interior macroblocks; over frames and rungs: odd vectors {odd}, |component| >= 4 {big}, "
              f"zero vectors {zero}, coded {coded}, skipped {skipped}")
        assert odd and big and zero and coded and skipped, (w, h, p)


# ------------------------------------------------------------------ check 2: the session probe
class PProbeRig(lc.SessionRig):
    """a SessionRig (encode buffers, entropy stage) with device buffers for the probe's frames (`stride` bytes apart), sizes and counts"""

    def __init__(self, pkg, ctx, w, h, qualities, n, stride=0):
        super().__init__(pkg, ctx, w, h, qualities, n)
        self.R, self.fb, self.stride = len(qualities), frame_bytes(w, h), stride or frame_bytes(w, h)
        self.probe_dev = self.bufs.put(np.zeros(n * self.stride, np.uint8))
        self.sizes_dev = self.bufs.put(np.zeros((n, self.R), np.uint32))
        self.stats_dev = self.bufs.put(np.zeros((n, self.R, NSTATS), np.uint32))

    def to_state(self, state):
        cl = clips(self.w, self.h, self.n)
        self.step(np.stack([c[0] for c in cl]), False, 1)
        if state:
            self.step(np.stack([c[1] for c in cl]), True, 2)

    def upload(self, frames):
        buf = np.full((self.n, self.stride), 0xA5, np.uint8)
        buf[:, :self.fb] = frames
        self.ctx.upload(self.probe_dev, buf)
        self.ctx.upload(self.sizes_dev, np.full((self.n, self.R), SENTINEL, np.uint32))
        self.ctx.upload(self.stats_dev, np.full((self.n, self.R, NSTATS), SENTINEL, np.uint32))

    def fetch(self):
        sizes, stats = np.zeros((self.n, self.R), np.uint32), np.zeros((self.n, self.R, NSTATS), np.uint32)
        self.ctx.download(sizes, self.sizes_dev)
        self.ctx.download(stats, self.stats_dev)
        return sizes, stats

    def probe(self, frames, stats=True):
        self.upload(frames)
        self.enc.probe_pframe_dev(self.probe_dev, self.sizes_dev, self.stats_dev if stats else 0)
        return self.fetch()


def check_session_probe(pkg, ctx, oracle, w, h, n, int_transform=False, qualities=LADDER, sets=None):
    """real session calls make the states: i-frame at rung 1, probe, p-frame at rung 2, probe again.  Sizes and all 20 counts of every frame
    (or of the frame sets named by `sets`, which include 1) at every rung; once without the counts (stats_dev = NULL); the host-buffer form agrees"""
    if tuple(qualities) == tuple(LADDER):
        check_inputs_cover(oracle, w, h, n)
        if (w, h, n) in INTERIOR_SHAPES:
            check_interior_inputs(oracle, w, h, n, sets)
    with options(pkg, ctx, None, int_transform):
        rig = PProbeRig(pkg, ctx, w, h, qualities, n)
    try:
        for state in (0, 1):
            if state == 0:
                rig.step(np.stack([c[0] for c in clips(w, h, n)]), False, 1)
            else:
                rig.step(np.stack([c[1] for c in clips(w, h, n)]), True, 2)
            fsets = state_frames(w, h, n, state)
            want = facts(oracle, w, h, qualities, n, state, sets)
            for t, frames in enumerate(fsets):
                if want[t] is None:
                    continue
                want_sizes, want_stats = want[t][0], want[t][1]
                sizes, stats = rig.probe(frames)
                assert np.array_equal(stats, want_stats), (state, FRAME_NAMES[t], np.argwhere(stats != want_stats)[:4].tolist())
                assert np.array_equal(sizes, want_sizes), (state, FRAME_NAMES[t], sizes.tolist(), want_sizes.tolist())
                if state == 0 and t == 0 and (w, h) in NOTHING_CODED_BYTES and tuple(qualities) == tuple(LADDER):
                    # the closed form of an all-skipped frame, by name: no coded macroblock and no vector at the coarsest rung in the model, and
                    # the DEVICE's size there is (152 + header bits + 7) >> 3 with an all-zero histogram
                    r = len(LADDER) - 1
                    assert not want[t][2][0][r].any() and not want[t][3][0][r].any()
                    assert int(sizes[0][r]) == NOTHING_CODED_BYTES[(w, h)] == (152 + int(stats[0][r][HDR]) + 7) >> 3 and not stats[0][r][:17].any()
            sizes, stats = rig.probe(fsets[1], stats=False)
            assert np.array_equal(sizes, want[1][0]) and (stats == SENTINEL).all()
            assert np.array_equal(rig.enc.probe_pframe(fsets[1]), want[1][0])
            assert rig.enc.rung == 1 + state
    finally:
        rig.close()


# ------------------------------------------------------------------ check 3: no side effects
def check_no_side_effects(pkg, ctx, oracle, w=50, h=38, n=3):
    """i-frame at rung 1, then a p-frame at rung 3: prev_frame, the rung and every output of the p-frame are the model's whether or not probes of
    OTHER frames (device form and host-buffer form) run in between"""
    cl = clips(w, h, n)
    other, want_other = state_frames(w, h, n, 0)[5], facts(oracle, w, h, LADDER, n, 0)[5]
    outs = []
    for with_probe in (False, True):
        rig = PProbeRig(pkg, ctx, w, h, LADDER, n)
        try:
            rig.step(np.stack([c[0] for c in cl]), False, 1)
            if with_probe:
                before = rig.enc.prev_frame()
                ptr_before = [ctx._lib.pfv_enc_prev_frame_dev(rig.enc.handle, k) for k in range(n)]
                sizes, stats = rig.probe(other)
                assert np.array_equal(sizes, want_other[0]) and np.array_equal(stats, want_other[1])
                assert np.array_equal(rig.enc.probe_pframe(other), want_other[0])
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


# ------------------------------------------------------------------ check 4: the probe is what the encoder writes
def check_probe_is_what_the_encoder_writes(pkg, ctx, oracle, device_entropy, w=50, h=38):
    """pfv_encoder: behind the same i-frame, the probed size of rung r == packet_bytes - 5 of the p-frame then encoded at rung r == the model's"""
    base = clips(w, h, 1)[0][0]
    fsets, want = state_frames(w, h, 1, 0), facts(oracle, w, h, LADDER, 1, 0)
    enc = pkg.Encoder(io.BytesIO(), w, h, 30, None, ctx, device_entropy=device_entropy, frame_report=True, qualities=LADDER)
    try:
        for t in (1, 2, 3):                                             # pan1, pan4, checker
            vf = pkg.VideoFrame.from_packed(w, h, fsets[t][0])
            for r in range(len(LADDER)):
                enc.set_rung(1)
                enc.encode_iframe(pkg.VideoFrame.from_packed(w, h, base))
                sizes = enc.probe_pframe(vf)
                assert np.array_equal(sizes, want[t][0][0]), (t, r, sizes.tolist(), want[t][0][0].tolist())
                assert enc.rung == 1
                enc.set_rung(r)
                enc.encode_pframe(vf)
                assert enc.rung == r and enc.last_report.packet_bytes - 5 == int(sizes[r])
    finally:
        enc.close()


# ------------------------------------------------------------------ check 5: window, frame stride, graph
def check_window_stride(pkg, ctx, oracle, w=50, h=38, n=3):
    """window (1, 2) with the frames frame_bytes + 48 apart: slots 1 and 2 exact, the entries of slot 0 left at the sentinel"""
    rig = PProbeRig(pkg, ctx, w, h, LADDER, n, stride=frame_bytes(w, h) + 48)
    try:
        rig.to_state(1)
        rig.enc.set_frame_stride(rig.stride)
        rig.enc.set_window(1, 2)
        fsets, want = state_frames(w, h, n, 1), facts(oracle, w, h, LADDER, n, 1)
        for t in (1, 4):
            sizes, stats = rig.probe(fsets[t])
            assert (sizes[0] == SENTINEL).all() and (stats[0] == SENTINEL).all()
            assert np.array_equal(sizes[1:], want[t][0][1:]) and np.array_equal(stats[1:], want[t][1][1:])
        with pytest.raises(pkg.PfvError) as e:                          # the host-buffer form works on all slots, packed, like pfv_enc_pframe
            rig.enc.probe_pframe(fsets[1])
        assert e.value.code == pkg._lib.PFV_ERR_STATE
        rig.enc.set_window(0, n)                                        # ... and the whole session again, still strided
        sizes, stats = rig.probe(fsets[4])
        assert np.array_equal(sizes, want[4][0]) and np.array_equal(stats, want[4][1])
    finally:
        rig.close()


def unbounded_search(block, ref, bx, by):
    """the reference's search (steps 8, 4, 2, 1 around the best so far; the centre first, then row by row, strict <) WITHOUT its bounds test, on
    the plane as the kernels' window holds it: 16-column chunks and rows beyond the plane repeat the last ones inside -> (dx, dy)"""
    ph, pw = ref.shape
    rows = np.clip(np.arange(-16, ph + 16), 0, ph - 1)
    cols = np.concatenate([np.arange(16), np.arange(pw), np.arange(pw - 16, pw)])
    ext, block = ref[rows][:, cols].astype(np.int64), block.astype(np.int64)

    def err(x, y):
        return int(((ext[by + 16 + y:by + 32 + y, bx + 16 + x:bx + 32 + x] - block) ** 2).sum())
    cx = cy = 0
    best = err(0, 0)
    for s in (8, 4, 2, 1):
        e, _, x, y = min((err(cx + dx * s, cy + dy * s), 3 * dy + dx, cx + dx * s, cy + dy * s) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy)
        if e < best:
            best, cx, cy = e, x, y
    return cx, cy


def check_strip_on_the_right_border(pkg, ctx, oracle, w=256, h=48, rig_class=None):
    """256x48: the luma strip at x0 = 128, y0 = 16 ends ON the right border (x0 + 8 * 16 == pw): it misses penc_search's rule by the 16 of its
    right term alone and keeps its bounds tests.  No other shape of the suite has such a strip (pw a multiple of 128, >= 256).  Of the MODEL first:
    under the pan the search without bounds tests answers otherwise for a macroblock of that strip, its match lying beyond the border.  Then the
    probe's sizes and counts (`rig_class`: PProbeRig or one derived from it, for the other two p-frame probe kernels)"""
    frames = [state_frames(w, h, 1, 0)[t] for t in (1, 2)]                                             # pan1, pan4
    want = facts(oracle, w, h, LADDER, 1, 0, (1, 2))
    ref = model_in_state(oracle, w, h, LADDER, 1, 0).prev[0][0]
    # no interior strip as it is; 16 px wider, that one strip would be
    assert 8 * 16 + 8 * 16 == ref.shape[1] == w and not interior_mbs(w, h) and interior_mbs(w + 16, h) == [(w + 16) // 16 + 8 + m for m in range(8)]
    differs = 0
    for f, t in zip(frames, (1, 2)):
        src = lc.split(f[0], w, h)[0]
        for i in range(w // 16 + 1, 2 * (w // 16)):              # the middle macroblock row; no vector of the last column can point right
            bx, by = i % (w // 16) * 16, i // (w // 16) * 16
            same = unbounded_search(src[by:by + 16, bx:bx + 16], ref, bx, by) == tuple(int(v) for v in want[t][3][0][0][i])
            assert same or bx == w - 16, (t, i)                  # 16 px and more from every border the helper IS the model: no candidate leaves the plane
            differs += int(not same)
    print(f"p-probe {w}x{h}: frames whose last macroblock of the strip on the right border the search without bounds tests answers otherwise: {differs} of 2")
    assert differs
    rig = (rig_class or PProbeRig)(pkg, ctx, w, h, LADDER, 1)
    try:
        rig.to_state(0)
        for f, t in zip(frames, (1, 2)):
            sizes, stats = rig.probe(f)[:2]
            assert np.array_equal(stats, want[t][1]) and np.array_equal(sizes, want[t][0]), FRAME_NAMES[t]
    finally:
        rig.close()


def check_graph(pkg, ctx, oracle, w=50, h=38, n=3):
    """the launch pair recorded once and replayed on changing frame contents: every replay exact (it finds the accumulator as k_pprobe_sizes left
    it: a row not cleared would show in the next replay's counts); a session that has never probed cannot start inside a recording"""
    rig = PProbeRig(pkg, ctx, w, h, LADDER, n)
    fresh = pkg.EncoderSession(ctx, w, h, None, n, qualities=LADDER)
    graph = pkg.Graph(ctx)
    try:
        rig.to_state(0)
        fsets, want = state_frames(w, h, n, 0), facts(oracle, w, h, LADDER, n, 0)
        sizes, stats = rig.probe(fsets[1])                              # the unrecorded call (it makes the accumulator)
        assert np.array_equal(sizes, want[1][0]) and np.array_equal(stats, want[1][1])
        with graph:
            rig.enc.probe_pframe_dev(rig.probe_dev, rig.sizes_dev, rig.stats_dev)
            with pytest.raises(pkg.PfvError) as e:
                fresh.probe_pframe_dev(rig.probe_dev, rig.sizes_dev)
            assert e.value.code == pkg._lib.PFV_ERR_STATE and "before pfv_graph_begin" in str(e.value)
        for t in (5, 0, 5, 2):
            rig.upload(fsets[t])
            graph.launch()
            sizes, stats = rig.fetch()
            assert np.array_equal(stats, want[t][1]) and np.array_equal(sizes, want[t][0]), FRAME_NAMES[t]
    finally:
        graph.close()
        fresh.close()
        rig.close()


# ------------------------------------------------------------------ the encoder's rules on the model
class EncoderModel:
    """pfv_encoder's state on the ladder model: the current rung, the budgets, the frames since the last i-frame"""

    def __init__(self, oracle, w, h, qualities, rung=0, budget_p=0, budget_i=0, pprobe=False, gop=0):
        self.o, self.w, self.h, self.q = oracle, w, h, list(qualities)
        self.model = LadderModel(oracle, w, h, qualities)
        self.sb = self.model.builder()
        self.K, self.rung, self.last_rung = len(qualities), rung, rung
        self.budget_p, self.budget_i, self.pprobe, self.gop = budget_p, budget_i, pprobe, gop
        self.n_written = self.since_i = 0
        self.shown, self.psizes = [], []

    def fit(self, sizes, budget):
        fits = [r for r in range(self.K) if int(sizes[r]) <= budget]
        return fits[0] if fits else self.K - 1

    def hard(self):
        return self.pprobe and self.budget_p and self.K > 1

    def iframe(self, f):
        if self.budget_i and self.K > 1:
            self.rung = self.fit(pc.expected(self.o, self.w, self.h, self.q, f)[0], self.budget_i)
        self.sb.iframe(self.model.iframe(0, f, self.rung), self.model.qidx(self.rung, False))
        self.last_rung, self.since_i = self.rung, 0
        self.n_written += 1
        self.shown.append(self.model.shown(0))
        return 1

    def pframe(self, f, rung_settled=False):
        if self.hard() and not rung_settled:
            sizes = pframe_facts(self.model, 0, f)[0]
            self.psizes.append(sizes)
            self.rung = self.fit(sizes, self.budget_p)
        mv, has, coef = self.model.pframe(0, f, self.rung)
        self.sb.pframe(mv, has, coef, self.model.qidx(self.rung, True))
        n = len(self.sb.parts[-1]) - 5
        self.last_rung = self.rung
        self.since_i += 1
        self.n_written += 1
        if self.budget_p and not self.pprobe:                          # pfv_encoder_set_rate's soft rule
            if n > self.budget_p:
                self.rung = min(self.rung + 1, self.K - 1)
            elif 2 * n <= self.budget_p:
                self.rung = max(self.rung - 1, 0)
        self.shown.append(self.model.shown(0))
        return 2

    def drop(self):
        self.sb.drop()
        self.since_i += 1
        self.n_written += 1
        self.shown.append(None)
        return 3

    def frame(self, f):
        """the five rules of pfv_encoder_encode_frame -> (type, why)"""
        if self.n_written == 0 or (self.gop > 0 and self.since_i >= self.gop):
            return self.iframe(f), "forced"
        psize, stats, _, _ = pframe_facts(self.model, 0, f)
        rp = self.fit(psize, self.budget_p) if self.hard() else self.rung
        if stats[rp][CODED] == 0 and stats[rp][MOVED] == 0:
            return self.drop(), "still"
        isize = pc.expected(self.o, self.w, self.h, self.q, f)[0]
        if int(isize[rp]) <= int(psize[rp]):
            return self.iframe(f), "size"
        self.rung = rp
        return self.pframe(f, rung_settled=True), "p"


def run_encoder(pkg, ctx, w, h, frames, plan, device_entropy, qualities=None, quality=None, rung=None, budget_p=0, budget_i=0, pprobe=None, gop=None,
                set_rungs=None):
    """plan: per frame 'I' | 'P' | 'A' (encode_frame); set_rungs: {frame index: rung set before it} -> (stream bytes, rung after every frame,
    type of every frame)"""
    buf = io.BytesIO()
    enc = pkg.Encoder(buf, w, h, 30, quality, ctx, device_entropy=device_entropy, qualities=qualities, frame_report=True)
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
        for t, (f, kind) in enumerate(zip(frames, plan)):
            vf = pkg.VideoFrame.from_packed(w, h, f)
            if set_rungs and t in set_rungs:
                enc.set_rung(set_rungs[t])
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


# ------------------------------------------------------------------ check 6: the hard p-frame budget
def model_hard_run(oracle, w, h, frames, budget_p, start_rung=2):
    em = EncoderModel(oracle, w, h, lc.RATE_LADDER, rung=start_rung, budget_p=budget_p, pprobe=True)
    rungs = []
    for t, f in enumerate(frames):
        em.iframe(f) if t == 0 else em.pframe(f)
        rungs.append(em.last_rung)
    return em.sb.bytes(), rungs, em.psizes


_HARD = {}


def hard_budget(oracle, w, h, frames):
    """a budget from the model's own sizes: the candidates are the sizes along the run at a generous budget, ascending; the first one under which
    the run uses at least three rungs and meets a frame that fits no rung"""
    if (w, h) not in _HARD:
        _, _, psizes = model_hard_run(oracle, w, h, frames, 10 ** 9)
        for bp in sorted({int(v) for s in psizes for v in s}):
            want, rungs, sizes = model_hard_run(oracle, w, h, frames, bp)
            if len(set(rungs[1:])) >= 3 and any((s.astype(np.int64) > bp).all() for s in sizes):
                _HARD[(w, h)] = (bp, want, rungs, sizes)
                break
    return _HARD[(w, h)]


def check_hard_budget(pkg, ctx, oracle, device_entropy, w=50, h=38):
    frames = lc.rate_clip(w, h)
    K = len(lc.RATE_LADDER)
    bp, want, rungs, sizes = hard_budget(oracle, w, h, frames)
    print(f"hard p-frame budget {bp}: rungs {rungs}, model sizes {[s.tolist() for s in sizes]}")
    assert len(set(rungs[1:])) >= 3 and any((s.astype(np.int64) > bp).all() for s in sizes)              # of the MODEL first
    assert all(rungs[t + 1] == (K - 1 if (s.astype(np.int64) > bp).all() else int(np.argmax(s.astype(np.int64) <= bp))) for t, s in enumerate(sizes))
    plan = "I" + "P" * (len(frames) - 1)
    data, got, _ = run_encoder(pkg, ctx, w, h, frames, plan, device_entropy, qualities=lc.RATE_LADDER, rung=2, budget_p=bp, pprobe=True)
    assert got == rungs, (got, rungs)
    assert data == want
    # the probe off (never switched, and switched off again): pfv_encoder_set_rate's soft rule, byte for byte
    soft, soft_rungs, _ = lc.model_rate_run(oracle, w, h, frames[:8], 2, bp)
    for pprobe in (None, False):
        data, got, _ = run_encoder(pkg, ctx, w, h, frames[:8], plan[:8], device_entropy, qualities=lc.RATE_LADDER, rung=2, budget_p=bp, pprobe=pprobe)
        assert got == soft_rungs and data == soft
    # one rung: nothing to choose, today's bytes
    plain, _, _ = run_encoder(pkg, ctx, w, h, frames[:4], plan[:4], device_entropy, quality=5)
    data, got, _ = run_encoder(pkg, ctx, w, h, frames[:4], plan[:4], device_entropy, qualities=[5], budget_p=bp, pprobe=True)
    assert data == plain and got == [0] * 4


# ------------------------------------------------------------------ check 7: the automatic frame type
def auto_clip(w, h):
    """from the frames of the session checks: the clip's first frame twice (nothing to code at the coarse rungs), the pan, a checkerboard (cheaper
    as an i-frame), the pan again for more than max_interval frames, its last frame twice"""
    cl = clips(w, h, 1)[0]
    return [cl[0], cl[0], cl[1], cl[2], content(w, h, "checker", seed=0), cl[3], cl[4], cl[5], cl[6], cl[6], cl[5], cl[4], cl[3]]


AUTO_GOP = 6
AUTO_SET_RUNGS = {1: 3}      # the caller moves to rung 3 behind the first frame (an i-frame at rung 1): there the repeated frame codes nothing


def model_auto_run(oracle, w, h, frames, rung, budget_p=0, pprobe=False, budget_i=0, set_rungs=None):
    em = EncoderModel(oracle, w, h, LADDER, rung=rung, budget_p=budget_p, pprobe=pprobe, budget_i=budget_i, gop=AUTO_GOP)
    types, whys, rungs = [], [], []
    for i, f in enumerate(frames):
        if set_rungs and i in set_rungs:
            em.rung = set_rungs[i]
        t, why = em.frame(f)
        types.append(t); whys.append(why); rungs.append(em.last_rung)
    return em, types, whys, rungs


def check_auto(pkg, ctx, oracle, device_entropy, w=50, h=38):
    frames = auto_clip(w, h)
    em, types, whys, rungs = model_auto_run(oracle, w, h, frames, 1, set_rungs=AUTO_SET_RUNGS)
    print(f"auto frame types {types} ({whys}), rungs {rungs}")
    assert whys[0] == "forced" and "forced" in whys[1:] and "size" in whys and "p" in whys and "still" in whys            # of the MODEL first
    k = whys.index("still")
    assert whys[k + 1] == "p", "a p-frame follows the drop: it predicts from the reference the drop left alone"
    data, got_rungs, got_types = run_encoder(pkg, ctx, w, h, frames, "A" * len(frames), device_entropy, qualities=LADDER, rung=1, gop=AUTO_GOP,
                                             set_rungs=AUTO_SET_RUNGS)
    assert got_types == types and got_rungs == rungs, (got_types, types, got_rungs, rungs)
    assert data == em.sb.bytes()
    got, ofr = lc.decode_both(pkg, ctx, oracle, data)
    assert len(ofr) == len(frames)
    for t, (s, o) in enumerate(zip(em.shown, ofr)):
        if s is not None:
            assert o is not None and np.array_equal(o, s), t
    shown = [o for o in ofr if o is not None]
    assert len(got) == len(shown) and all(np.array_equal(a, b) for a, b in zip(got, shown))
    # with the hard budget and the i-frame budget on: rp is the budget's choice, an i-frame's rung the i-frame budget's
    bp = int(facts(oracle, w, h, LADDER, 1, 0)[1][0][0][2])           # the pan behind the first frame, rung 2
    bi = int(pc.expected(oracle, w, h, LADDER, frames[0])[0][1])
    em, types, whys, rungs = model_auto_run(oracle, w, h, frames, 3, budget_p=bp, pprobe=True, budget_i=bi)
    print(f"auto frame types under budgets p {bp}, i {bi}: {types} ({whys}), rungs {rungs}")
    assert len(set(rungs)) >= 2 and 2 in types
    data, got_rungs, got_types = run_encoder(pkg, ctx, w, h, frames, "A" * len(frames), device_entropy, qualities=LADDER, rung=3, gop=AUTO_GOP,
                                             budget_p=bp, budget_i=bi, pprobe=True)
    assert got_types == types and got_rungs == rungs, (got_types, types, got_rungs, rungs)
    assert data == em.sb.bytes()


# ------------------------------------------------------------------ check 8: arguments and states
def check_arguments(pkg, ctx, oracle, w=50, h=38):
    L, lib = pkg._lib, ctx._lib
    BAD, STATE = L.PFV_ERR_BAD_ARG, L.PFV_ERR_STATE
    P = ctypes.c_void_p
    frame = clips(w, h, 1)[0][1]
    vf = pkg.VideoFrame.from_packed(w, h, frame)
    bufs = DevBufs(ctx)
    s = pkg.EncoderSession(ctx, w, h, 4, 1)                            # one rung: one size
    try:
        frames_dev, sizes_dev = bufs.put(frame), bufs.put(np.zeros(1, np.uint32))
        host = np.zeros(1, np.uint32)
        assert lib.pfv_enc_probe_pframe_dev(None, P(frames_dev), P(sizes_dev), None) == BAD
        assert lib.pfv_enc_probe_pframe_dev(s.handle, None, P(sizes_dev), None) == BAD
        assert lib.pfv_enc_probe_pframe_dev(s.handle, P(frames_dev), None, None) == BAD
        assert lib.pfv_enc_probe_pframe(None, frame.ctypes.data_as(P), host.ctypes.data_as(P)) == BAD
        assert lib.pfv_enc_probe_pframe(s.handle, None, host.ctypes.data_as(P)) == BAD
        assert lib.pfv_enc_probe_pframe(s.handle, frame.ctypes.data_as(P), None) == BAD
        model = LadderModel(oracle, w, h, [4])                         # against the blank reference of a new session
        want = pframe_facts(model, 0, frame)[0]
        got = s.probe_pframe(frame)
        assert got.shape == (1, 1) and np.array_equal(got[0], want)
        s.probe_pframe_dev(frames_dev, sizes_dev)                      # usable after every refused call
        ctx.download(host, sizes_dev)
        assert np.array_equal(host, want)
    finally:
        s.close()
        bufs.close()
    y, u, v = (pl.pixels.ctypes.data_as(P) for pl in (vf.plane_y, vf.plane_u, vf.plane_v))
    buf = io.BytesIO()
    e = pkg.Encoder(buf, w, h, 30, None, ctx, qualities=[1, 4, 9])
    try:
        out, typ = np.zeros(3, np.uint32), ctypes.c_int(0)
        assert lib.pfv_encoder_probe_pframe(None, y, u, v, out.ctypes.data_as(P)) == BAD
        assert lib.pfv_encoder_probe_pframe(e.handle, None, u, v, out.ctypes.data_as(P)) == BAD
        assert lib.pfv_encoder_probe_pframe(e.handle, y, u, v, None) == BAD
        assert lib.pfv_encoder_set_pframe_probe(None, 1) == BAD and lib.pfv_encoder_set_gop(None, 1) == BAD
        assert lib.pfv_encoder_set_gop(e.handle, -1) == BAD
        assert lib.pfv_encoder_encode_frame(None, y, u, v, ctypes.byref(typ)) == BAD
        assert lib.pfv_encoder_encode_frame(e.handle, y, None, v, ctypes.byref(typ)) == BAD
        model = LadderModel(oracle, w, h, [1, 4, 9])
        assert np.array_equal(e.probe_pframe(vf), pframe_facts(model, 0, frame)[0]) and e.rung == 0
        assert lib.pfv_encoder_encode_frame(e.handle, y, u, v, None) == 0                               # type_out may be NULL; the first frame is an i-frame
        e._flush()
        sb = model.builder()
        sb.iframe(model.iframe(0, frame, 0), model.qidx(0, False))
        assert buf.getvalue() == sb.bytes()[:len(buf.getvalue())] and len(buf.getvalue()) == len(sb.bytes()) - 5     # all but the EOF packet
        e.finish()
        with pytest.raises(pkg.PfvError) as err:                       # a finished encoder
            e.probe_pframe(vf)
        assert err.value.code == STATE
        assert lib.pfv_encoder_encode_frame(e.handle, y, u, v, ctypes.byref(typ)) == STATE
    finally:
        e.close()


def build_poison(exe):
    """tests/cpp/pprobe_poison.cpp against a build of the library sources on the CPU emulator with tests/cpp/poison_seam.h force-included in
    front of them (kept next to the emulator library and rebuilt when a source is newer, as conftest.build_emulator does)"""
    csrc, emu = os.path.join(ROOT, "pretty-fast-video_amd", "csrc"), os.path.join(ROOT, "tests", "hipemu")
    seam, lib = os.path.join(ROOT, "tests", "cpp", "poison_seam.h"), os.path.join(emu, "libpfv_emu_seam.so")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc)] + [seam, os.path.join(emu, "hipemu.cpp"), os.path.join(emu, "hip", "hip_runtime.h"),
                                                               *[os.path.join(ROOT, "include", x) for x in ("pfv_hip.h", "pfv_hip_core.h", "pfv_hip_ext.h")]]
    if not (os.path.exists(lib) and all(os.path.getmtime(x) <= os.path.getmtime(lib) for x in srcs)):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-I", emu, "-include", seam, "-x", "c++",
                        os.path.join(csrc, "pfv_capi.hip"), os.path.join(emu, "hipemu.cpp"), "-o", lib], check=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "pprobe_poison.cpp"), "-o", exe, lib, "-Wl,-rpath," + emu], check=True)


def check_poisoned(oracle, exe, tmp_path, device_entropy, w=50, h=38):
    """a p-frame fails behind its encode kernel (the seam fails the payload-size download): the probe and encode_pframe return PFV_ERR_STATE and
    nothing is written; encode_frame then writes an I-FRAME of the same frame on the given entropy path, and the frame behind it is probed and
    typed by the rules again -- return codes, probed sizes, types and stream bytes against the model"""
    STATE = -9                                                         # PFV_ERR_STATE, include/pfv_hip_core.h
    frames = clips(w, h, 1)[0][:3]
    em = EncoderModel(oracle, w, h, LADDER, rung=1)
    em.iframe(frames[0])
    em.iframe(frames[1])                                               # the failed p-frame left no packet; the recovery is an i-frame at the same rung
    probed = pframe_facts(em.model, 0, frames[2])[0].tolist()
    last_type = em.frame(frames[2])[0]
    yuv, out = str(tmp_path / "poison.yuv"), str(tmp_path / "poison.pfv")
    np.concatenate(frames).tofile(yuv)
    r = subprocess.run([exe, str(w), str(h), ",".join(str(q) for q in LADDER), "1" if device_entropy else "0", yuv, out],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert [ln[0] for ln in lines] == ["failed", "poisoned", "type", "sizes", "type"]
    assert int(lines[0][1]) < 0
    assert [int(x) for x in lines[1][1:]] == [STATE, STATE, 0]
    assert int(lines[2][1]) == 1
    assert [int(x) for x in lines[3][1:]] == probed
    assert int(lines[4][1]) == last_type == 2
    assert open(out, "rb").read() == em.sb.bytes()


# ------------------------------------------------------------------ check 9: the C++ mirror
def build_cpp(lib_path, exe):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "pprobe_auto.cpp"), "-o", exe, lib_path, "-Wl,-rpath," + os.path.dirname(lib_path)], check=True)


def check_cpp(oracle, exe, tmp_path, w=50, h=38):
    """tests/cpp/pprobe_auto.cpp (pfv::Encoder::probe_pframe, set_pframe_probe, set_gop, encode_frame) over the auto clip under both budgets: the
    model's probed sizes, types, rungs and bytes"""
    frames = auto_clip(w, h)
    bp = int(facts(oracle, w, h, LADDER, 1, 0)[1][0][0][2])
    bi = int(pc.expected(oracle, w, h, LADDER, frames[0])[0][1])
    em = EncoderModel(oracle, w, h, LADDER, rung=3, budget_p=bp, pprobe=True, budget_i=bi, gop=AUTO_GOP)
    types, rungs, probed = [], [], []
    for f in frames:
        probed.append(pframe_facts(em.model, 0, f)[0].tolist())
        types.append(em.frame(f)[0])
        rungs.append(em.last_rung)
    yuv, out = str(tmp_path / "auto.yuv"), str(tmp_path / "auto.pfv")
    np.concatenate(frames).tofile(yuv)
    r = subprocess.run([exe, str(w), str(h), ",".join(str(q) for q in LADDER), "3", str(bi), str(bp), str(AUTO_GOP), yuv, out],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(frames) + 2
    for want, line in zip(probed, lines):
        assert [int(x) for x in line.split()[1:]] == want
    assert [int(x) for x in lines[-2].split()[1:]] == types and [int(x) for x in lines[-1].split()[1:]] == rungs
    assert open(out, "rb").read() == em.sb.bytes()
