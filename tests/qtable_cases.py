"""Q-table sets and per-plane q-table indices, shared by the GPU tests (tests/test_gpu_qtables.py) and their emulator twins
(tests/test_emu_qtables.py).

A .pfv header carries any number of u16 tables (src/dec.rs:89-111) and every packet names one per plane by a u8 (payload bytes 16-18,
src/dec.rs:244-246, 346-348).  The product's encoders only write four tables and (0,1,1) / (2,3,3), so everything else the format allows
is driven here: streams written from parts (tests/pfv_stream_builder.py) through Decoder, GopDecoder and BatchDecoder against the oracle's
stream decoder call by call, and the decoder session's entry points on hostile tables and coefficients against the oracle's decoder.

The hostile inputs mix four classes of macroblocks, and every check asserts what its own inputs are, with the numpy restatement of the
reference (oracle/pfv_oracle_np.py):
  C1 (the wrap matters)      the "wide" i32 rule changes the decoded output in >= 1/4 of the subblocks of the wrapping classes;
  C2 (not saturated)         in wrap-to-residue blocks >= 1/2 of the output pixels lie strictly inside (0, 255);
  C3 (the selection matters) decoding a plane with any other table index used in the same frame changes its output.
"""
from __future__ import annotations

import contextlib

import numpy as np
import pytest

import pfv_oracle_np as onp
import stream_cases as sc
from oracle_bind import OracleDecoder, OracleEncoder, OracleStreamDecoder, pad16
from pfv_stream_builder import MAX_COEF, StreamBuilder

WRAPPING = ("wrap", "residue", "transform")
SCALE_ZZ = onp.DCT_SCALE_FACTOR.astype(np.int64)          # dct_decode indexes SCALE and q by zigzag position (src/dct.rs:78-82)


@contextlib.contextmanager
def np_rule(name, value):
    old = onp.RULES[name]
    onp.RULES[name] = value
    try:
        yield
    finally:
        onp.RULES[name] = old


def planes(w, h):
    """[(padded width, padded height, first macroblock, macroblock count)] for Y, U, V"""
    out, mb0 = [], 0
    for pw, ph in ((pad16(w), pad16(h)), (pad16(w // 2), pad16(h // 2)), (pad16(w // 2), pad16(h // 2))):
        n = (pw // 16) * (ph // 16)
        out.append((pw, ph, mb0, n))
        mb0 += n
    return out


def split_padded(frame, w, h):
    """padded Y|U|V frame -> three 2-D planes"""
    out, off = [], 0
    for pw, ph, _, _ in planes(w, h):
        out.append(np.asarray(frame[off:off + pw * ph]).reshape(ph, pw))
        off += pw * ph
    return out


def crop(frame, w, h):
    """the retframe (src/dec.rs:195-197) of a padded frame"""
    y, u, v = split_padded(frame, w, h)
    return np.concatenate([y[:h, :w].reshape(-1), u[:h // 2, :w // 2].reshape(-1), v[:h // 2, :w // 2].reshape(-1)])


# ------------------------------------------------------------------------------------------------------------------ tables
RESIDUE_POS = (0, 4, 32, 36)          # the zigzag positions whose SCALE is 32 (a power of two): with q = 2^14 or 2^15 a product wraps to 0


def hostile_tables(rng, n, low=0, high=65535):
    """n tables of 64 entries uniform in [low, high].  The full range [0, 65535] also gets, in every table, a 0 and a 65535 entry, a DC
    entry of 2^14 or 2^15 (and the same at the other RESIDUE_POS now and then): 4096 * 32 * 2^15 = 2^32 == 0, the wrap-to-residue class;
    and four AC entries in [1, 8], where small coefficients keep a wrap-to-residue block textured without saturating it"""
    t = rng.integers(low, high + 1, (n, 64))
    if (low, high) == (0, 65535):
        free = [z for z in range(64) if z not in RESIDUE_POS]
        for k in range(n):
            pick = rng.choice(free, 6, replace=False)
            t[k, pick[0]], t[k, pick[1]] = 0, 65535
            t[k, pick[2:]] = rng.integers(1, 9, 4)
            t[k, 0] = rng.choice([1 << 14, 1 << 15])
            for z in RESIDUE_POS[1:]:
                if rng.random() < 0.5:
                    t[k, z] = rng.choice([1 << 14, 1 << 15])
    return t.astype(np.int64)


def residue_coefs(q, cmax):
    """per zigzag position: the coefficient in [1, cmax] whose dequantised product c * SCALE * q is == 0 mod 2^32 (0 where there is none)"""
    c = np.arange(1, cmax + 1, dtype=np.int64)
    out = np.zeros(64, np.int64)
    for z in range(64):
        if q[z] > 0:
            hit = np.flatnonzero(onp._wrap(c * SCALE_ZZ[z] * int(q[z])) == 0)
            if hit.size:
                out[z] = c[hit[0]]
    return out


def transform_coefs(q, cmax):
    """per zigzag position: the largest coefficient whose dequantised product stays inside i32 (the butterfly sums of a block of them do not)"""
    prod = SCALE_ZZ * np.maximum(q.astype(np.int64), 1)
    return np.minimum(cmax, (2 ** 31 - 1) // prod)


class ClassedCoefs:
    """coefficients of one frame, one class per macroblock (see the module docstring); a table set without a position that wraps to 0 (tables
    away from the full range) gets no wrap-to-residue macroblocks"""

    def __init__(self, rng, w, h, tables, qidx, cmax):
        nb = sum(p[3] for p in planes(w, h))
        self.coef = np.zeros((nb, 256), np.int64)
        self.cls = np.empty(nb, dtype=object)
        for p, (_, _, mb0, n) in enumerate(planes(w, h)):
            q = tables[qidx[p]]
            rc = residue_coefs(q, cmax)
            zero = np.flatnonzero(rc)                                     # products that wrap to 0
            small = np.flatnonzero((q >= 1) & (q <= 8))                   # products that stay small
            kinds = ["typical", "wrap", "transform"] + (["residue"] if zero.size and 0 in zero else [])
            tc = transform_coefs(q, cmax)
            order = rng.permutation(np.arange(n) % len(kinds))            # every class in every plane of 4 or more macroblocks, "typical" in all
            kind = np.array(kinds, dtype=object)[order]
            self.cls[mb0:mb0 + n] = kind
            sign = np.where(rng.random((n, 4, 1)) < 0.5, 1, -1)
            # typical: low-frequency-heavy, low magnitude, like quantised DCT output in zigzag order
            typ = rng.integers(-12, 13, (n, 4, 64)) * (rng.random((n, 4, 64)) < 0.6 * np.exp(-np.arange(64) / 6.0))
            # wrap: 25 % dense, anywhere in the range (cmax 32767: all of int16, beyond what a stream can carry)
            wrp = rng.integers(-32768 if cmax == 32767 else -cmax, cmax + 1, (n, 4, 64)) * (rng.random((n, 4, 64)) < 0.25)
            # residue: the DC (and at times the other positions that can) wraps to 0; small values where q is small
            res = np.zeros((n, 4, 64), np.int64)
            for z in zero:
                on = np.ones((n, 4), bool) if z == 0 else rng.random((n, 4)) < 0.5
                res[:, :, z] = rc[z] * on * np.where(rng.random((n, 4)) < 0.5, 1, -1)
            res[:, :, small] = rng.integers(-3, 4, (n, 4, small.size))
            # transform: every product inside i32, their sums are not
            trf = np.broadcast_to(tc[None, None, :] * sign[:, :1, :], (n, 4, 64))
            pick = {"typical": typ, "wrap": wrp, "residue": res, "transform": trf}
            blk = np.zeros((n, 4, 64), np.int64)
            for k in kinds:
                sel = kind == k
                blk[sel] = pick[k][sel]
            self.coef[mb0:mb0 + n] = blk.reshape(n, 256)
        self.coef = self.coef.astype(np.int16)


# ------------------------------------------------------------------------------------------------------------------ numpy restatement
def np_mb_out(coef, q, ref=None, mv=None, has=None, bw=None):
    """one plane's macroblocks [n,16,16] as the reference decodes them: decode_plane_into (i-frame) or decode_plane_delta (p-frame,
    src/common.rs:254-285) against the padded reference plane `ref`; returns (output, the residual's own decode before the prediction)"""
    dec = onp.decode_blocks(np.asarray(coef), np.asarray(q, dtype=np.int64))
    if ref is None:
        return dec, dec
    n = dec.shape[0]
    i = np.arange(n)
    sx = (i % bw) * 16 + mv[:, 0].astype(np.int64)
    sy = (i // bw) * 16 + mv[:, 1].astype(np.int64)
    prev = ref[(sy[:, None] + np.arange(16))[:, :, None], (sx[:, None] + np.arange(16))[:, None, :]].astype(np.int64)
    out = np.clip(prev + (dec.astype(np.int64) - 128) * 2, 0, 255)
    return np.where(has.astype(bool)[:, None, None], out, prev).astype(np.uint8), dec


def check_conditions(w, h, tables, qidx, coef, cls=None, ref_frame=None, mv=None, has=None, want_frame=None):
    """C1-C3 on one frame of one stream (cls None: typical content, C3 only).  ref_frame: the padded frame a p-frame predicts from.  Also
    holds the numpy restatement to the oracle's frame (want_frame), so that the conditions speak about what the C oracle computes.
    Returns the measured shares."""
    stats = {}
    refs = split_padded(ref_frame, w, h) if ref_frame is not None else [None] * 3
    used = sorted(set(int(x) for x in qidx))
    diff_sub, n_sub, inside, n_res = 0, 0, 0, 0
    outs = []
    for p, (pw, ph, mb0, n) in enumerate(planes(w, h)):
        sl = slice(mb0, mb0 + n)
        args = dict(ref=refs[p], mv=None if mv is None else mv[sl], has=None if has is None else has[sl], bw=pw // 16)
        out, res_dec = np_mb_out(coef[sl], tables[qidx[p]], **args)
        outs.append(onp._scatter(out, pw // 16, ph // 16).reshape(-1))
        coded = np.ones(n, bool) if has is None else has[sl].astype(bool)
        for j in used:                                                               # C3
            if j != qidx[p]:
                other = np_mb_out(coef[sl], tables[j], **args)[0]
                assert not np.array_equal(out, other), f"C3: plane {p} decodes alike with table {j} and with its own {qidx[p]}"
        if cls is None:
            continue
        with np_rule("i32", "wide"):
            wide = np_mb_out(coef[sl], tables[qidx[p]], **args)[0]
        wr = np.isin(cls[sl], WRAPPING) & coded
        d = (out != wide).reshape(n, 2, 8, 2, 8).any(axis=(2, 4))
        diff_sub += int(d[wr].sum())
        n_sub += 4 * int(wr.sum())
        res = (cls[sl] == "residue") & coded
        inside += int(((res_dec[res] > 0) & (res_dec[res] < 255)).sum())     # p-frames: the residual's decode, before the prediction is added
        n_res += 256 * int(res.sum())
    if want_frame is not None:
        assert np.array_equal(np.concatenate(outs), want_frame), "the numpy restatement and the C oracle decode this frame differently"
    if cls is not None:
        stats["c1"] = diff_sub / max(n_sub, 1)
        stats["c2"] = inside / n_res if n_res else None
        assert n_sub > 0 and stats["c1"] >= 0.25, f"C1: the i32 wrap changes only {stats['c1']:.2f} of the wrapping subblocks"
        assert n_res == 0 or stats["c2"] >= 0.5, f"C2: only {stats['c2']:.2f} of the wrap-to-residue pixels are inside (0, 255)"
    return stats


def legal_motion(rng, w, h, n_extreme=0.2):
    """random legal motion vectors over the whole i8 range (the reference only checks that the block stays inside the padded reference
    plane, src/common.rs:258-259); a share of them at the extremes, so that every plane sees blocks read at all four of its edges"""
    mv = []
    for pw, ph, _, n in planes(w, h):
        i = np.arange(n)
        bx, by = (i % (pw // 16)) * 16, (i // (pw // 16)) * 16
        lox, hix = np.maximum(-128, -bx), np.minimum(127, pw - 16 - bx)
        loy, hiy = np.maximum(-128, -by), np.minimum(127, ph - 16 - by)
        mx = lox + (rng.random(n) * (hix - lox + 1)).astype(np.int64)
        my = loy + (rng.random(n) * (hiy - loy + 1)).astype(np.int64)
        e = rng.random(n)
        mx = np.where(e < n_extreme / 2, lox, np.where(e > 1 - n_extreme / 2, hix, mx))
        e = rng.random(n)
        my = np.where(e < n_extreme / 2, loy, np.where(e > 1 - n_extreme / 2, hiy, my))
        # one block of the plane reads each edge for sure
        mx[0], my[0] = lox[0], loy[0]
        mx[n - 1], my[n - 1] = hix[n - 1], hiy[n - 1]
        mv.append(np.stack([mx, my], axis=1))
    mv = np.concatenate(mv)
    assert mv.min() >= -128 and mv.max() <= 127
    return mv.astype(np.int8)


def distinct_qidx(rng, n_tables, prev=None):
    """three distinct indices (U != V, Y apart from both), different from the previous frame's"""
    while True:
        q = tuple(int(x) for x in rng.choice(n_tables, 3, replace=False))
        if q != prev:
            return q


# ------------------------------------------------------------------------------------------------------------------ stream-level
def quality_tables(q):
    il, ic, pl, pc_, _ = onp.qtables(q)
    return [np.asarray(t, np.int64) for t in (il, ic, pl, pc_)]


def table_set(name, rng):
    """the header's tables for a stream case"""
    if name == "one":
        return np.stack([quality_tables(5)[0]])
    if name == "perm4":                      # four distinct tables (quality 5's inter tables are flat: take quality 2's inter_c instead)
        t = quality_tables(5)
        return np.stack([t[0], t[1], t[2], quality_tables(2)[3]])
    if name == "hostile7":
        return hostile_tables(rng, 7)
    if name in ("t256", "t300"):
        return rng.integers(1, 400, (256 if name == "t256" else 300, 64)).astype(np.int64)
    if name == "none":
        return np.zeros((0, 64), np.int64)
    raise ValueError(name)


def stream_qidx(name, n_tables, k, ptype, rng):
    """the indices of the k-th coded packet of a stream case"""
    if name == "one":
        return (0, 0, 0)
    if name == "perm4":                      # Y on a chroma table, U != V, changing from packet to packet
        seq = [(1, 0, 2), (3, 2, 0), (2, 3, 1), (0, 1, 3), (3, 0, 1), (1, 3, 2)]
        return seq[k % len(seq)]
    if name == "t256":                       # index 255 in use
        seq = [(255, 17, 200), (254, 255, 3), (0, 128, 255)]
        return seq[k % len(seq)]
    if name == "t300":                       # only the first 256 can be named
        seq = [(255, 0, 99), (7, 255, 254)]
        return seq[k % len(seq)]
    return distinct_qidx(rng, n_tables)


def coded_content(oracle, pkg, w, h, pattern, seed, hostile_every=0, rng=None):
    """coefficients / vectors / flags per coded packet of `pattern` ('I' / 'P' / 'D'): the oracle encoder's output on the synthetic pan at
    quality 5, every plane of every p-frame with at least one coded macroblock; hostile_every > 0: one macroblock in that many gets
    coefficients anywhere in the stream's range (+-16383)"""
    enc = OracleEncoder(oracle, w, h, 5)
    st = pkg.SyntheticStream(w, h, seed=seed)
    out, t = [], 0
    for c in pattern:
        if c == "D":
            out.append(None)
            continue
        f = st.frame(t)
        t += 1
        if c == "I":
            coef, mv, has = enc.encode_iframe(f), None, None
        else:
            mv, has, coef = enc.encode_pframe(f)
            has = has.copy()
            for _, _, mb0, n in planes(w, h):
                b = mb0 + int(rng.integers(0, n))
                has[b] = 1
                coef[b, :64] = 0
                coef[b, :6] = rng.integers(-20, 21, 6) | 1
        if hostile_every:
            pick = rng.random(coef.shape[0]) < 1.0 / hostile_every
            coef[pick] = rng.integers(-MAX_COEF, MAX_COEF + 1, (int(pick.sum()), 256)) * (rng.random((int(pick.sum()), 256)) < 0.25)
        out.append([c, coef.astype(np.int16), mv, has])
    return out


def _with_residue_blocks(coef, has, w, h, tables, q, k):
    """on hostile tables, coefficients made for a quality table saturate whatever the table: one coded macroblock per plane becomes a
    wrap-to-residue block of the plane's own table (DC * SCALE * q == 0 mod 2^32, small values where q is small), whose output the
    table decides"""
    coef, has = coef.copy(), None if has is None else has.copy()
    rng = np.random.default_rng(k)
    for p, (_, _, mb0, n) in enumerate(planes(w, h)):
        t = tables[q[p]]
        rc = residue_coefs(t, MAX_COEF)
        if not rc[0]:
            continue
        b = mb0 + int(rng.integers(0, n))
        blk = np.zeros((4, 64), np.int64)
        blk[:, 0] = rc[0] * np.where(rng.random(4) < 0.5, 1, -1)
        small = np.flatnonzero((t >= 1) & (t <= 8))
        blk[:, small] = rng.integers(-3, 4, (4, small.size))
        coef[b] = blk.reshape(256)
        if has is not None:
            has[b] = 1
    return coef, has


def build_stream(oracle, w, h, tables, content, qidx_of):
    """content from coded_content; qidx_of(k, ptype) -> the indices of the k-th coded packet.  Returns (bytes, [qidx per packet or None])"""
    nb = sum(p[3] for p in planes(w, h))
    b = StreamBuilder(oracle, w, h, 30, tables, nb)
    used, k = [], 0
    for item in content:
        if item is None:
            b.drop()
            used.append(None)
            continue
        c, coef, mv, has = item
        q = qidx_of(k, c)
        k += 1
        if max(q) < len(tables):
            coef, has = _with_residue_blocks(coef, has, w, h, tables, q, k)
        item[1:] = [coef, mv, has]
        (b.iframe(coef, q) if c == "I" else b.pframe(mv, has, coef, q))
        used.append(q)
    return b.bytes(), used


def check_stream_inputs(w, h, tables, content, used):
    """C3 on every coded packet of a built stream: the plane outputs differ between any two indices the packet uses (p-frames: on the
    coded macroblocks' residual decode, the part of the output the table reaches)"""
    for item, q in zip(content, used):
        if item is None or q is None or max(q) >= len(tables):
            continue
        c, coef, mv, has = item
        for p, (_, _, mb0, n) in enumerate(planes(w, h)):
            sl = slice(mb0, mb0 + n)
            sel = np.ones(n, bool) if has is None else has[sl].astype(bool)
            mine = onp.decode_blocks(coef[sl][sel], tables[q[p]])
            for j in set(q) - {q[p]}:
                assert not np.array_equal(mine, onp.decode_blocks(coef[sl][sel], tables[j])), (q, p, j)


def outcomes_equal(got, want, what):
    assert [x[0] for x in got] == [x[0] for x in want], (what, [x[0] for x in got], [x[0] for x in want])
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"{what}: call {k} gives {a[0]}{a[1:] if a[0] != 'frame' else ''}, the oracle {b[0]}{b[1:] if b[0] != 'frame' else ''}"


def check_decoders_on(pkg, ctx, oracle, data, decoders, gop_shapes):
    """every decoder object on `data`, call by call against the oracle's stream decoder; returns the oracle's outcomes"""
    want = sc._outcomes_oracle(oracle, data)
    for ent, la in decoders:
        got = sc._outcomes(lambda: pkg.Decoder(data, ctx, lookahead=la, entropy=ent), pkg)
        outcomes_equal(got, want, f"Decoder(entropy={ent}, lookahead={la})")
    for k, (mg, ml) in enumerate(gop_shapes):
        for ent in ("host", "device"):
            got = sc._outcomes(lambda: pkg.GopDecoder(data, ctx, max_gops=mg, max_gop_frames=ml, threads=1 + k % 2, entropy=ent), pkg)
            outcomes_equal(got, want, f"GopDecoder(max_gops={mg}, max_gop_frames={ml}, entropy={ent})")
    return want


DECODERS_ALL = (("host", 0), ("host", None), ("device", 0), ("device", None), ("auto", 0), ("auto", None))
GOP_SHAPES = ((4, 4), (3, 4), (2, 2), (8, 15))


def payload_sizes(data):
    """lengths of the coded packets of a .pfv stream"""
    pos = 20 + 128 * int.from_bytes(data[18:20], "little")
    out = []
    while pos + 5 <= len(data):
        t, n = data[pos], int.from_bytes(data[pos + 1:pos + 5], "little")
        if t in (1, 2) and n:
            out.append(n)
        pos += 5 + n
    return out


def check_stream_case(pkg, ctx, oracle, w, h, name, pattern, seed=1, decoders=DECODERS_ALL, gop_shapes=GOP_SHAPES, hostile_every=0,
                      return_sizes=False):
    """one table set with its index pattern: build, check the inputs (C3), then every decoder against the oracle.  Returns the outcome
    kinds, or (return_sizes) the payload sizes -- and then every payload of 64 KiB or more must have taken the device entropy stage's road
    under `auto`"""
    rng = np.random.default_rng(seed)
    tables = table_set(name, rng)
    content = coded_content(oracle, pkg, w, h, pattern, seed, hostile_every, rng)
    data, used = build_stream(oracle, w, h, tables, content, lambda k, t: stream_qidx(name, len(tables), k, t, rng))
    check_stream_inputs(w, h, tables, content, used)
    want = check_decoders_on(pkg, ctx, oracle, data, decoders, gop_shapes)
    if not return_sizes:
        return [x[0] for x in want]
    sizes = payload_sizes(data)
    dec = pkg.Decoder(data, ctx, lookahead=0, entropy="auto")
    while dec.advance_frame(lambda fr: None):
        pass
    counts = dec.entropy_counts()
    dec.close()
    assert counts["packets_read_on_device"] + counts["packets_left_to_host_parser"] == sum(n >= 64 << 10 for n in sizes), (counts, sizes)
    return sizes


def check_zero_tables(pkg, ctx, oracle, w=64, h=48, decoders=DECODERS_ALL, gop_shapes=GOP_SHAPES):
    """a header with no q-table: the reference opens it (Decoder::new, src/dec.rs:89-111); drop frames and EOF as usual, a coded packet fails
    on its index (the reference panics, the oracle reports FormatError) -- on that call, not at open"""
    rng = np.random.default_rng(3)
    nb = sum(p[3] for p in planes(w, h))
    b = StreamBuilder(oracle, w, h, 30, np.zeros((0, 64)), nb)
    b.drop(); b.drop()
    kinds = check_decoders_on(pkg, ctx, oracle, b.bytes(), decoders, gop_shapes)
    assert [k[0] for k in kinds] == ["none", "none", "none", "eof"], kinds      # the call that meets EOF delivers nothing
    content = coded_content(oracle, pkg, w, h, "DIP", 3, rng=rng)
    data, _ = build_stream(oracle, w, h, np.zeros((0, 64)), content, lambda k, t: (0, 0, 0))
    kinds = check_decoders_on(pkg, ctx, oracle, data, decoders, gop_shapes)
    assert [k[0] for k in kinds] == ["none", "err"] and kinds[1][1] == pkg._lib.PFV_ERR_FORMAT, kinds
    # BatchDecoder: opens, drop steps, the coded step fails with FORMAT
    bd = pkg.BatchDecoder([data, data], ctx, threads=1)
    assert bd.advance_frames() is None
    with pytest.raises(pkg.DecodeError) as e:
        bd.advance_frames()
    assert e.value.code == pkg._lib.PFV_ERR_FORMAT
    bd.close()


def check_out_of_range_index(pkg, ctx, oracle, w=64, h=48, decoders=DECODERS_ALL, gop_shapes=GOP_SHAPES):
    """4 tables, the third packet names table 4: FORMAT on that packet, the frames before it delivered"""
    rng = np.random.default_rng(4)
    tables = table_set("perm4", rng)
    content = coded_content(oracle, pkg, w, h, "IPPIP", 4, rng=rng)
    data, _ = build_stream(oracle, w, h, tables, content, lambda k, t: (0, 4, 1) if k == 2 else stream_qidx("perm4", 4, k, t, rng))
    kinds = check_decoders_on(pkg, ctx, oracle, data, decoders, gop_shapes)
    assert [k[0] for k in kinds] == ["frame", "frame", "err"] and kinds[2][1] == pkg._lib.PFV_ERR_FORMAT, kinds


def check_gop_variation(pkg, ctx, oracle, w, h, seed=5, gop_shapes=GOP_SHAPES, modes=("host", "device")):
    """index combinations that vary from GOP to GOP, so that one GOP-decoder step holds several (type, qidx) combinations: GOPs 0 and 2 alike
    and GOP 1 different (a non-contiguous run of slots), leading p-frames (an i- and a p-packet at the same position of a step), a GOP whose
    p-frames change indices mid-way, drop frames"""
    rng = np.random.default_rng(seed)
    tables = hostile_tables(rng, 6, 1, 3000)
    pattern = "PPIPPPIPPPIPPDPIPP"
    #         gop: -1 -1 | 0 0 0 0 | 1 1 1 1 | 2 2 2 D 2 | 3 3 3
    content = coded_content(oracle, pkg, w, h, pattern, seed, rng=rng)
    A_i, A_p, B_i, B_p, C_p = (0, 1, 2), (3, 4, 5), (5, 0, 1), (2, 3, 4), (1, 5, 0)
    coded = [c for c in pattern if c != "D"]
    gop_of, g = [], -1
    for c in coded:
        g += c == "I"
        gop_of.append(g)
    pos_in_gop = [sum(1 for j in range(k) if gop_of[j] == gop_of[k]) for k in range(len(coded))]

    def qidx_of(k, t):
        gg = gop_of[k]
        if gg == -1:
            return B_p                              # leading p-frames: as GOP 1's p-frames
        if gg in (0, 2):
            return A_i if t == "I" else A_p
        if gg == 1:
            return B_i if t == "I" else B_p
        return A_i if t == "I" else (C_p if pos_in_gop[k] >= 2 else A_p)
    data, used = build_stream(oracle, w, h, tables, content, qidx_of)
    check_stream_inputs(w, h, tables, content, used)
    want = sc._outcomes_oracle(oracle, data)
    assert [x[0] for x in want].count("frame") == len(coded)
    for k, (mg, ml) in enumerate(gop_shapes):
        for ent in modes:
            got = sc._outcomes(lambda: pkg.GopDecoder(data, ctx, max_gops=mg, max_gop_frames=ml, threads=1 + k % 2, entropy=ent), pkg)
            outcomes_equal(got, want, f"GopDecoder(max_gops={mg}, max_gop_frames={ml}, entropy={ent})")
    got = sc._outcomes(lambda: pkg.Decoder(data, ctx, lookahead=0, entropy="host"), pkg)
    outcomes_equal(got, want, "Decoder")
    return len(coded)


def check_batch_decoder_qidx(pkg, ctx, oracle, w, h, n_streams=3, seed=6, modes=("host", "device")):
    """BatchDecoder: streams that share a header and indices (hostile tables, indices changing per step, U != V) give the oracle's frames
    stream by stream; streams whose indices differ within a step fail that step with PFV_ERR_FORMAT (a documented restriction of the
    object, pfv_batch_objects.hip), after delivering the steps before it"""
    rng = np.random.default_rng(seed)
    tables = hostile_tables(rng, 7)
    pattern = "IPPDPIPP"
    qseq = [distinct_qidx(rng, 7) for _ in range(len(pattern))]
    datas, contents = [], []
    for s in range(n_streams):
        content = coded_content(oracle, pkg, w, h, pattern, seed + 11 * s, hostile_every=6, rng=rng)
        d, used = build_stream(oracle, w, h, tables, content, lambda k, t: qseq[k])
        check_stream_inputs(w, h, tables, content, used)
        datas.append(d)
        contents.append(content)
    for mode in modes:
        odecs = [OracleStreamDecoder(oracle, d) for d in datas]
        bd = pkg.BatchDecoder(datas, ctx, threads=2, entropy=mode)
        steps = 0
        while True:
            fr = bd.advance_frames()
            if fr is False:
                break
            for s in range(n_streams):
                rc, want = odecs[s].advance_frame()
                assert rc == 1
                if fr is None:
                    assert want is None
                else:
                    assert np.array_equal(fr[s], want), f"BatchDecoder ({mode}): step {steps} stream {s} differs from the oracle"
            steps += 1
        assert steps == len(pattern)
        bd.close()
    # the last stream's indices differ from the others' at its fourth coded packet
    content = coded_content(oracle, pkg, w, h, pattern, seed + 99, rng=rng)
    odd, _ = build_stream(oracle, w, h, tables, content, lambda k, t: qseq[k] if k != 3 else qseq[k][::-1])
    for mode in modes:
        bd = pkg.BatchDecoder(datas[:-1] + [odd], ctx, threads=2, entropy=mode)
        for _ in range(4):                                                 # I P P D: delivered
            assert bd.advance_frames() is not False
        with pytest.raises(pkg.DecodeError) as e:
            bd.advance_frames()
        assert e.value.code == pkg._lib.PFV_ERR_FORMAT
        bd.close()


# ------------------------------------------------------------------------------------------------------------------ session-level
def _schedule(S):
    """(type, entry point, window or None, output form) per frame: every entry point with both frame types, a window on a sub-range of
    slots (the frame after it is an i-frame: a slot left out keeps no usable framebuffer, pfv_hip_ext.h), fused (16-byte aligned stride)
    and separate (misaligned stride) crops"""
    win = (1, S - 1) if S > 1 else None
    return [("I", "dense", None, "packed"), ("P", "sparse", None, "packed"), ("P", "lists", None, "packed"), ("P", "dev", None, "aligned"),
            ("I", "sparse", None, "packed"), ("P", "dense", None, "packed"), ("P", "dev", win, "misaligned"), ("I", "lists", None, "packed"),
            ("P", "lists", None, "packed"), ("P", "dev", None, "misaligned"), ("I", "dev", win, "aligned")]


def check_session_hostile(pkg, ctx, oracle, w, h, n_streams, n_tables, seed, schedule=None, cmax=32767, table_range=(0, 65535)):
    """DecoderSession with n_tables hostile tables and another qidx per frame, on coefficients of the four classes over the full int16 range
    (beyond what a stream can carry), mixed has_coef, random legal motion vectors with some at the extremes: after every frame the framebuffer
    and the cropped frames against the oracle's decoder, stream by stream.  Returns the measured condition shares."""
    rng = np.random.default_rng(seed)
    S = n_streams
    tables = hostile_tables(rng, n_tables, *table_range)
    dec = pkg.DecoderSession(ctx, w, h, tables, S)
    odecs = [OracleDecoder(oracle, w, h, tables) for _ in range(S)]
    nb, fb, pfb = dec.total_blocks, dec.frame_bytes, dec.padded_frame_bytes
    stride_a = (fb + 15) // 16 * 16 + 16
    stride_m = stride_a + 8
    d_out = ctx.alloc(S * stride_m + 64)
    d_coef, d_mv, d_has = ctx.alloc(S * nb * 512), ctx.alloc(S * nb * 2), ctx.alloc(S * nb)
    valid = [True] * S                                  # slot has a usable framebuffer (the reference's new_padded counts as one)
    prev_q, shares = None, []
    for t, (ptype, entry, win, outform) in enumerate(schedule or _schedule(S)):
        first, count = win if win else (0, S)
        qidx = distinct_qidx(rng, n_tables, prev_q)
        prev_q = qidx
        coefs = [ClassedCoefs(rng, w, h, tables, qidx, cmax) for _ in range(S)]
        coef = np.stack([c.coef for c in coefs])
        mv = np.stack([legal_motion(rng, w, h) for _ in range(S)])
        has = (rng.random((S, nb)) < 0.7).astype(np.uint8)
        for s in range(S):                                  # every plane codes one macroblock of each class it has (C1-C3 need them coded)
            for _, _, mb0, n in planes(w, h):
                for kind in ("typical", *WRAPPING):
                    at = np.flatnonzero(coefs[s].cls[mb0:mb0 + n] == kind)
                    if at.size:
                        has[s, mb0 + int(at[0])] = 1
        if ptype == "P":
            assert all(valid[first:first + count]), "schedule: a p-frame on a slot without a framebuffer"
        # what the oracle computes, and the conditions on this frame's inputs
        before = [odecs[s].framebuffer() for s in range(S)]
        for s in range(first, first + count):
            (odecs[s].decode_iframe(coef[s], qidx) if ptype == "I" else odecs[s].decode_pframe(mv[s], has[s], coef[s], qidx))
        want = [odecs[s].framebuffer() for s in range(S)]
        for s in range(first, first + count):
            shares.append(check_conditions(w, h, tables, qidx, coef[s], coefs[s].cls, None if ptype == "I" else before[s],
                                           None if ptype == "I" else mv[s], None if ptype == "I" else has[s], want[s]))
        # the product
        ctx.upload(d_out, np.full(S * stride_m + 64, 0xA5, np.uint8))
        stride = {"packed": fb, "aligned": stride_a, "misaligned": stride_m}[outform]
        if outform == "packed":
            dec.set_output_dev(d_out)
        else:
            dec.set_output_strided_dev(d_out, stride)
        if win:
            dec.set_window(first, count)
        if entry == "dense":
            (dec.decode_iframe(coef, qidx) if ptype == "I" else dec.decode_pframe(mv, has, coef, qidx))
        elif entry == "sparse":
            flat = coef.reshape(-1)
            idx = np.flatnonzero(flat).astype(np.uint32)
            (dec.decode_iframe_sparse(idx, flat[idx], qidx) if ptype == "I" else dec.decode_pframe_sparse(mv, has, idx, flat[idx], qidx))
        elif entry == "lists":
            if ptype == "I":
                dec.decode_iframe_lists(*dec.coef_lists(coef), qidx=qidx)
            else:
                dec.decode_pframe_lists(mv, has, *dec.coef_lists(coef, has), qidx=qidx)
        else:
            ctx.upload(d_coef, coef)
            if ptype == "I":
                dec.decode_iframe_dev(d_coef, qidx)
            else:
                ctx.upload(d_mv, mv)
                ctx.upload(d_has, has)
                dec.decode_pframe_dev(d_mv, d_has, d_coef, qidx)
        dec.check()
        if win:
            dec.set_window(0, S)
            for s in range(S):
                if not first <= s < first + count:
                    valid[s] = False
        if ptype == "I":
            for s in range(first, first + count):
                valid[s] = True
        got = dec.framebuffer()
        out = np.empty(S * stride_m + 64, np.uint8)
        ctx.download(out, d_out)
        for s in range(first, first + count):
            assert np.array_equal(got[s], want[s]), f"frame {t} ({ptype}, {entry}, qidx {qidx}) stream {s}: framebuffer differs from the oracle's"
            assert np.array_equal(out[s * stride:s * stride + fb], crop(want[s], w, h)), \
                f"frame {t} ({ptype}, {entry}, {outform} output) stream {s}: cropped frame differs from the oracle's"
        for s in range(S):
            if not first <= s < first + count:
                assert (out[s * stride:s * stride + fb] == 0xA5).all(), f"frame {t}: slot {s} outside the window was written"
        assert (out[(S - 1) * stride + fb:] == 0xA5).all(), f"frame {t}: written past the last slot"
    dec.set_output_dev(None)
    for p in (d_out, d_coef, d_mv, d_has):
        ctx.free(p)
    dec.close()
    if table_range == (0, 65535):
        assert all(x["c2"] is not None for x in shares), "a frame without wrap-to-residue blocks"
    c2 = [x["c2"] for x in shares if x["c2"] is not None]
    return {"c1_min": min(x["c1"] for x in shares), "c2_min": min(c2) if c2 else None, "frames": len(shares)}


def check_plane_ops_zero_entries(pkg, ctx, oracle, sizes=((48, 32), (100, 60)), seed=9):
    """the plane-level decode operators take q entries of 0 (the reference's decode only multiplies, src/dct.rs:75-86); the encode operators
    still refuse them (they divide).  Hostile coefficients of the four classes against the oracle."""
    rng = np.random.default_rng(seed)
    n = 0
    for (w, h) in sizes:
        bw, bh = pad16(w) // 16, pad16(h) // 16
        for k in range(3):
            q = hostile_tables(rng, 1)[0]
            q[rng.choice([z for z in range(64) if z not in RESIDUE_POS and q[z] > 8], 8, replace=False)] = 0
            assert (q == 0).sum() >= 8
            tabs = np.stack([q, q, q])
            cc = ClassedCoefs(rng, bw * 16, bh * 16, tabs, (0, 1, 2), 32767)
            coef = cc.coef[:bw * bh]
            cls = cc.cls[:bw * bh]
            # C1 / C2 on the plane (its macroblocks are the Y plane of a (bw*16, bh*16) frame)
            out = onp.decode_blocks(coef, q)
            with np_rule("i32", "wide"):
                wide = onp.decode_blocks(coef, q)
            wr = np.isin(cls, WRAPPING)
            assert (out != wide).reshape(-1, 2, 8, 2, 8).any(axis=(2, 4))[wr].mean() >= 0.25
            res = cls == "residue"
            assert res.sum() > 0 and ((out[res] > 0) & (out[res] < 255)).mean() >= 0.5
            want = oracle.decode_plane(coef, bw, bh, q)
            assert np.array_equal(onp._scatter(out, bw, bh), want)
            got = pkg.VideoPlane.decode_plane(pkg.EncodedIPlane(bw * 16, bh * 16, bw, bh, coef), q, ctx).image()
            assert np.array_equal(got, want), (w, h, k, "decode_plane with zero q entries")
            ref = rng.integers(0, 256, (bh * 16, bw * 16), dtype=np.uint8)
            mv = legal_motion(rng, bw * 16, bh * 16)[:bw * bh]          # the Y plane of a (bw*16, bh*16) frame
            has = (rng.random(bw * bh) < 0.7).astype(np.uint8)
            wantp = oracle.decode_plane_delta(mv, has, coef, bw, bh, q, ref)
            src = pkg.EncodedPPlane(bw * 16, bh * 16, bw, bh, mv, has, coef)
            refp = pkg.VideoPlane.from_slice(bw * 16, bh * 16, ref)
            assert np.array_equal(pkg.VideoPlane.decode_plane_delta(src, refp, q, ctx).image(), wantp), (w, h, k, "decode_plane_delta")
            target = pkg.VideoPlane.from_slice(bw * 16, bh * 16, ref)
            pkg.VideoPlane.decode_plane_delta_into(src, target, q, ctx)
            assert np.array_equal(target.image(), wantp), (w, h, k, "decode_plane_delta_into")
            n += 1
        px = rng.integers(0, 256, (h, w), dtype=np.uint8)
        with pytest.raises(pkg.PfvError) as e:
            pkg.VideoPlane.from_slice(w, h, px).encode_plane(q, 0, ctx)
        assert e.value.code == pkg._lib.PFV_ERR_BAD_ARG
    return n
