"""The decoders' guarded float inverse (PFV_OPT_DEC_TRANSFORM, csrc/pfv_kernels.hip: dec_float_guard): one case list for the emulator
(tests/test_emu_dec_float.py) and the GPU (tests/test_gpu_dec_float.py).

Every case is a short frame sequence on 144 x 48 -- luma 9 x 3 macroblocks (a full strip of 8 and a strip of one per row), chroma 72 x 24
padded to 80 x 32 (5 x 2: a partial strip, and under the 16-lane mapping a wavefront of four and a wavefront of one) -- decoded by
  * a session under PFV_DEC_TRANSFORM_AUTO, with path statistics on,
  * a session under PFV_DEC_TRANSFORM_INT,
  * the oracle decoder,
and after every frame the three framebuffers must agree byte for byte AND the AUTO session's count of integer-path wavefronts must equal
the number predicted here from the coefficients, the tables and the library's own bound pfv_dec_float_guard(): a wavefront (8 macroblocks
of a strip, or 4 under the 16-lane mapping) runs in i32 iff one of its coded macroblocks holds a dequantised value v = i32(c * SCALE * q)
with |v| above the bound."""
import numpy as np

import pfv_oracle_np as onp
from oracle_bind import OracleDecoder
from qtable_cases import planes

W, H = 144, 48
SCALE = onp.DCT_SCALE_FACTOR.astype(np.int64)       # dct_decode indexes SCALE and q by the zigzag position (src/dct.rs:78-82)
MAPPINGS = (("lanes8", "PFV_LANES_PER_MB_8", 8), ("lanes16", "PFV_LANES_PER_MB_16", 4))     # (id, option value, macroblocks per wavefront)
FORMS = ("dense", "lists")
TOTAL = sum(n for _, _, _, n in planes(W, H))       # 27 + 10 + 10 macroblocks


def wrap32(x):
    return (np.asarray(x, dtype=np.int64) + (1 << 31)) % (1 << 32) - (1 << 31)


def dequantised(coef, q):
    """coef [n, 256] i16, q [64] -> v [n, 4, 64]: what the kernels look at (wmul24(c, deq), deq = SCALE * q < 2^23)"""
    return wrap32(coef.reshape(-1, 4, 64).astype(np.int64) * wrap32(SCALE * q.astype(np.int64)))


def predict(coef, has, tables, qidx, group, bound):
    """(integer-path wavefronts, wavefronts) of one decode launch"""
    n_int = n_all = 0
    for (pw, ph, mb0, cnt), qi in zip(planes(W, H), qidx):
        bw, bh = pw // 16, ph // 16
        big = (np.abs(dequantised(coef[mb0:mb0 + cnt], tables[qi])) > bound).any(axis=(1, 2)) & (has[mb0:mb0 + cnt] != 0)
        for by in range(bh):
            for g0 in range(0, bw, group):
                n_int += int(big[by * bw + g0:by * bw + min(g0 + group, bw)].any())
                n_all += 1
    return n_int, n_all


# ------------------------------------------------------------------------------------------------------------------ inputs
def flat_tables(q=16):
    return np.full((4, 64), q, dtype=np.int32)


def zero_motion():
    return np.zeros((TOTAL, 2), dtype=np.int8)


def all_coded():
    return np.ones(TOTAL, dtype=np.uint8)


def quiet_coefs(seed, amp=40):
    """coefficients whose dequantised values stay far below any bound with the flat tables: |v| <= 40 * 43 * 16"""
    return np.random.default_rng(seed).integers(-amp, amp + 1, (TOTAL, 256)).astype(np.int16)


def factor_at(target):
    """(zigzag position z, q, c) with SCALE[z] * q * c == target, q a legal table entry, c an i16"""
    for z in range(64):
        s = int(SCALE[z])
        if target % s:
            continue
        rest = target // s
        for q in range(1, 65536):
            if rest % q == 0 and rest // q <= 32767:
                return z, q, rest // q
    raise AssertionError(f"{target} has no SCALE * q * c form")


def at_the_bound(bound, over):
    """cases (a) / (b): quiet content, and in ONE luma macroblock of the full strip of row 1 (+value) and in ONE chroma macroblock (-value,
    other subblock) a coefficient whose dequantised value is exactly bound (+ 1 when `over`).  Two wavefronts hold one under either mapping."""
    za, qa, ca = factor_at(bound)
    zb, qb, cb = factor_at(bound + 1)
    assert za != zb
    tables = flat_tables()
    tables[:, za] = qa
    tables[:, zb] = qb
    z, c = (zb, cb) if over else (za, ca)
    coef = quiet_coefs(11)
    coef[:, [za, 64 + za, 128 + za, 192 + za, zb, 64 + zb, 128 + zb, 192 + zb]] = 0      # the two special positions are quiet elsewhere
    (_, _, y0, _), (_, _, u0, _), _ = planes(W, H)
    coef[y0 + 9 + 2, z] = c                    # luma row 1, macroblock 2 (wavefront: strip 0 of row 1 / its first half), subblock 0
    coef[u0 + 5 + 4, 192 + z] = -c             # U row 1, macroblock 4 (the strip's tail / the one-macroblock wavefront), subblock 3
    v = dequantised(coef, tables[0])
    assert np.abs(v).max() == bound + (1 if over else 0) and (np.abs(v) >= bound).sum() == 2
    has = all_coded()
    return tables, [("i", coef, (0, 1, 1)), ("p", zero_motion(), has, coef, (2, 3, 3))]


def int16_extremes(quality):
    """case (c): +-32767 at every position under the quality's own tables"""
    tables = np.stack(onp.qtables(quality)[:4]).astype(np.int32)
    rng = np.random.default_rng(quality)
    coef = np.where(rng.integers(0, 2, (TOTAL, 256)) == 1, 32767, -32767).astype(np.int16)
    coef[3] = 32767
    coef[4] = -32768
    return tables, [("i", coef, (0, 1, 1)), ("p", zero_motion(), all_coded(), coef, (2, 3, 3))]


def wrapping_product(bound):
    """case (d): a table entry and a coefficient whose product leaves i32 and lands INSIDE the bound: the guard passes, the float path runs,
    and it must run on the wrapped value"""
    best = None
    for z in range(64):
        s = int(SCALE[z])
        for c in (32767, 32766, -32767, -32768):
            q0 = (1 << 32) // (abs(c) * s)
            for q in range(max(1, q0 - 2), min(65535, q0 + 3) + 1):
                exact = c * s * q
                v = int(wrap32(exact))
                if abs(exact) >= (1 << 31) and bound // 2 < abs(v) <= bound and (best is None or abs(v) > abs(best[3])):
                    best = (z, q, c, v)
    assert best is not None
    z, q, c, v = best
    tables = flat_tables()
    tables[:, z] = q
    coef = quiet_coefs(13)
    coef[:, [z, 64 + z, 128 + z, 192 + z]] = 0
    coef[::3, z] = c
    coef[1::3, 128 + z] = c
    assert np.abs(dequantised(coef, tables[0])).max() == abs(v) <= bound
    assert np.abs(coef.reshape(-1, 4, 64).astype(np.int64) * SCALE * tables[0]).max() >= (1 << 31)
    return tables, [("i", coef, (0, 1, 1)), ("p", zero_motion(), all_coded(), coef, (2, 3, 3))]


def moving_frames(seed, n):
    """smooth content that moves, with some noise: ordinary pictures"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for t in range(n):
        y = 128 + 90 * np.sin((xx + 3 * t) / 9.0) * np.cos((yy - 2 * t) / 7.0) + rng.normal(0, 6, (H, W))
        u = 128 + 60 * np.sin((xx[::2, ::2] + 2 * t) / 13.0) + rng.normal(0, 3, (H // 2, W // 2))
        v = 128 + 60 * np.cos((yy[::2, ::2] + t) / 11.0) + rng.normal(0, 3, (H // 2, W // 2))
        out.append(np.concatenate([np.clip(p, 0, 255).astype(np.uint8).reshape(-1) for p in (y, u, v)]))
    return out


def encoder_output(oracle, quality, seed=3):
    """case (e): what the (oracle) encoder makes of three ordinary frames: i, p, p"""
    tables = np.stack(onp.qtables(quality)[:4]).astype(np.int32)
    enc = oracle.encoder(W, H, quality)
    frames = moving_frames(seed + quality, 3)
    seq = [("i", enc.encode_iframe(frames[0]).reshape(TOTAL, 256), (0, 1, 1))]
    for f in frames[1:]:
        mv, has, coef = enc.encode_pframe(f)
        seq.append(("p", mv.reshape(TOTAL, 2), has.reshape(TOTAL), coef.reshape(TOTAL, 256), (2, 3, 3)))
    return tables, seq


def edge_vectors(oracle):
    """a p-frame whose vectors put patches on every edge of every plane: each macroblock points at the nearest-to-reach left, right, top
    or bottom edge (or a corner), as far as an i8 vector goes"""
    tables, seq = encoder_output(oracle, 5)
    kind, _, has, coef, qidx = seq[1]
    mv = np.zeros((TOTAL, 2), dtype=np.int8)
    touched = set()
    for pi, (pw, ph, mb0, cnt) in enumerate(planes(W, H)):
        bw = pw // 16
        for k in range(cnt):
            x, y = (k % bw) * 16, (k // bw) * 16
            want_x = (0, pw - 16, x, x, 0, pw - 16)[k % 6]
            want_y = (y, y, 0, ph - 16, ph - 16, 0)[k % 6]
            mx, my = int(np.clip(want_x - x, -128, 127)), int(np.clip(want_y - y, -128, 127))
            mv[mb0 + k] = (mx, my)
            for name, hit in (("left", x + mx == 0), ("right", x + mx == pw - 16), ("top", y + my == 0), ("bottom", y + my == ph - 16)):
                if hit:
                    touched.add((pi, name))
    assert len(touched) == 12, touched
    return tables, [seq[0], (kind, mv, np.ones(TOTAL, dtype=np.uint8), coef, qidx)]


def mixed_skips(bound):
    """a p-frame with skipped and coded macroblocks inside one wavefront, one wavefront without any coded macroblock, and -- dense form --
    hostile values in the coefficients of skipped macroblocks, which nobody may read: they must neither reach the picture nor fail the guard.
    One coded macroblock is over the bound, so that the count is not trivially zero."""
    tables = flat_tables()
    z, q, c = factor_at(bound + 1)
    tables[:, z] = q
    coef = quiet_coefs(17)
    coef[:, [z, 64 + z, 128 + z, 192 + z]] = 0
    has = np.zeros(TOTAL, dtype=np.uint8)
    (_, _, y0, _), (_, _, u0, _), (_, _, v0, _) = planes(W, H)
    has[y0:y0 + 9:2] = 1                       # luma row 0: coded, skipped, coded, ... inside the strip
    has[y0 + 18:y0 + 27] = 1                   # luma row 2: all coded; row 1: nothing coded (two wavefronts that transform nothing)
    has[u0 + 1] = has[u0 + 7] = 1
    has[v0:v0 + 10] = 1
    has[v0 + 2] = 0
    coef[has == 0] = 32767                     # hostile, unread
    coef[y0 + 1, 5] = -32768
    coef[y0 + 18 + 6, 64 + z] = c              # coded and over the bound: luma row 2, strip 0 / its second half
    i_coef = quiet_coefs(19)
    return tables, [("i", i_coef, (0, 1, 1)), ("p", zero_motion(), has, coef, (2, 3, 3)), ("p", zero_motion(), has[::-1].copy(), coef, (2, 3, 3))]


CASES = ("at_bound", "over_bound", "extremes_q0", "extremes_q10", "wrapping_product", "encoder_q0", "encoder_q5", "encoder_q10", "edge_vectors",
         "mixed_skips")


def build(name, oracle, bound):
    if name == "at_bound":
        return at_the_bound(bound, False)
    if name == "over_bound":
        return at_the_bound(bound, True)
    if name.startswith("extremes_q"):
        return int16_extremes(int(name[10:]))
    if name == "wrapping_product":
        return wrapping_product(bound)
    if name.startswith("encoder_q"):
        return encoder_output(oracle, int(name[9:]))
    if name == "edge_vectors":
        return edge_vectors(oracle)
    assert name == "mixed_skips"
    return mixed_skips(bound)


# what a case must predict, beside whatever the formula says: (a) no wavefront, (b) exactly the two that hold the value, per frame
EXPECT_INT_PER_FRAME = {"at_bound": 0, "over_bound": 2, "wrapping_product": 0, "encoder_q5": 0}


# ------------------------------------------------------------------------------------------------------------------ the check
def run_case(pkg, ctx, oracle, name, mapping, form):
    L = pkg._lib
    _, lanes_opt, group = mapping
    bound = int(ctx._lib.pfv_dec_float_guard())
    tables, seq = build(name, oracle, bound)
    before = {o: ctx.get_option(o) for o in (L.PFV_OPT_LANE_MAPPING, L.PFV_OPT_DEC_TRANSFORM)}
    assert before[L.PFV_OPT_DEC_TRANSFORM] == L.PFV_DEC_TRANSFORM_AUTO      # the default
    try:
        ctx.set_option(L.PFV_OPT_LANE_MAPPING, getattr(L, lanes_opt))
        auto = pkg.DecoderSession(ctx, W, H, tables, 1)
        ctx.set_option(L.PFV_OPT_DEC_TRANSFORM, L.PFV_DEC_TRANSFORM_INT)
        plain = pkg.DecoderSession(ctx, W, H, tables, 1)
    finally:
        for o, v in before.items():
            ctx.set_option(o, v)
    odec = OracleDecoder(oracle, W, H, tables)
    auto.enable_path_stats()
    plain.enable_path_stats()
    want_int = want_all = 0
    try:
        for t, fr in enumerate(seq):
            if fr[0] == "i":
                _, coef, qidx = fr
                has = all_coded()
                for d in (auto, plain):
                    if form == "lists":
                        d.decode_iframe_lists(*d.coef_lists(coef[None]), qidx=qidx)
                    else:
                        d.decode_iframe(coef[None], qidx)
                odec.decode_iframe(coef, qidx)
            else:
                _, mv, has, coef, qidx = fr
                for d in (auto, plain):
                    if form == "lists":
                        d.decode_pframe_lists(mv[None], has[None], *d.coef_lists(coef[None], has[None]), qidx=qidx)
                    else:
                        d.decode_pframe(mv[None], has[None], coef, qidx)
                odec.decode_pframe(mv, has, coef, qidx)
            n_int, n_all = predict(coef, has, tables, qidx, group, bound)
            if name in EXPECT_INT_PER_FRAME:
                assert n_int == EXPECT_INT_PER_FRAME[name], (name, t, n_int)
            want_int += n_int
            want_all += n_all
            fb = auto.framebuffer()[0]
            assert np.array_equal(fb, odec.framebuffer()), (name, mapping[0], form, t, "AUTO differs from the oracle")
            assert np.array_equal(fb, plain.framebuffer()[0]), (name, mapping[0], form, t, "AUTO differs from INT")
            assert auto.path_stats() == (want_int, want_all), (name, mapping[0], form, t, auto.path_stats(), (want_int, want_all))
        assert plain.path_stats() == (0, want_all)          # the integer kernels have no guard to fail
        if name == "mixed_skips":
            assert 0 < want_int < want_all
        if name.startswith("extremes"):
            assert want_int > 0
    finally:
        auto.close()
        plain.close()
