"""Crafted coefficient / vector / flag buffers for the encoder's entropy stage on the device (csrc/pfv_entropy_kernels.hip: k_ent_scan /
_codes / _init / _pack / _gather) and for the host coder (csrc/pfv_host.hip: serialize_iframe / serialize_pframe), shared by the emulator
tests (test_emulated_kernels.py: test_emu_ent_*), the GPU tests (test_gpu_ent.py) and the CPU test of the host coder (test_ent_host.py).

The stage writes every .pfv byte of the GOP, batch and stream encoders, and random or video-like content never reaches its seams: the
longest symbol such content makes is 23 bits, so the third payload word of a symbol (ent_or_bits), value bits shifted past bit 31 and
code pairs past 20 bits had never run against a reference.  Every case here starts from RUN LISTS (zeros in front, coeff_size, value), as
entd_cases.Runs does for the decoder, and turns them into the buffers an encoder would hand to the stage.  The truth of every case is
the numpy restatement (oracle/pfv_oracle_entropy_np.py: iframe_payload / pframe_payload) AND the C oracle (pfvo_serialize_iframe /
pfvo_serialize_pframe), byte for byte.  Before anything is compared a case proves ON THE RESTATEMENT ALONE (layout() below) that it reaches
the seam it is named after: a case that stops reaching its seam fails instead of passing silently.

Two facts keep a histogram exact: an unused macroblock of an i-frame costs 17 (15, 0) fillers, so histogram-exact i-frames tile EVERY
macroblock with value runs; and a macroblock that does not end on a value at coefficient 255 adds a closing (rest, 0) to bins 0 and rest,
so the exact cases end every macroblock on a value."""
from __future__ import annotations

import ctypes
import functools

import numpy as np

import pfv_oracle_entropy_np as E
from entd_cases import TABLE_SKEW

HEAD_BITS = 152                     # 16 table bytes + 3 q-table indices
GROUP_MBS = 64                      # macroblocks per workgroup of k_ent_scan / k_ent_pack (kEntThreads / 4)
STEP = 256                          # symbol words per step of k_ent_pack (kEntThreads)
WIN_BITS = 2048 * 32                # k_ent_pack's LDS window, production build (PFV_ENT_WIN_WORDS)
WIN_BITS_SMALL = 64 * 32            # the variant build of test_emu_ent_small_window
OVERSIZE = (16384, -16384, 32767, -32768, -16385)


def total_blocks(w, h):
    c = lambda x: (x + 15) // 16
    return c(w) * c(h) + 2 * c((w + 1) // 2) * c((h + 1) // 2)


# geometries by macroblock count: 3, 16, 20 (one group); 191 / 192 / 193 (total_blocks % 64 = 63 / 0 / 1: the last group one macroblock short,
# whole, ONE macroblock)
GEOM = {3: (16, 16), 16: (128, 16), 20: (64, 48), 191: (272, 112), 192: (512, 64)}
GEOM[193] = next((w, h) for h in range(16, 400, 16) for w in range(16, 1200, 16) if total_blocks(w, h) == 193)
assert all(total_blocks(*g) == n for n, g in GEOM.items())


def value_of(size, rng, sign=None):
    """a value whose coeff_size (bit length + 1, src/rle.rs:23-24) is `size`"""
    assert 2 <= size <= 15
    mag = int(rng.integers(1 << (size - 2), 1 << (size - 1)))
    neg = bool(rng.integers(0, 2)) if sign is None else sign < 0
    return -mag if neg else mag


def mb_from_runs(runs, rng=None):
    """one macroblock from (zeros in front, coeff_size, value or None) -- zeros in front may be any count: the fillers are the coder's business.
    What is left behind the last value is the closing run."""
    out = np.zeros(256, np.int16)
    idx = 0
    for z, s, v in runs:
        idx += z
        assert idx < 256, "a run list is at most one macroblock"
        v = value_of(s, rng) if v is None else v
        assert v != 0 and E.coeff_size(v) == s, (s, v)
        out[idx] = v
        idx += 1
    return out


class Frame:
    """what one pack call reads: coef [S][nb][256], and for a p-frame mv [S][nb][2] and has [S][nb].  expect: "ok" (bytes == the oracles'),
    "format" (PFV_ERR_FORMAT), "nomem" (PFV_ERR_NOMEM)"""

    def __init__(self, ptype, coef, mv=None, has=None, expect="ok", note=""):
        self.ptype = ptype
        self.coef = np.ascontiguousarray(coef, np.int16)
        S, nb, _ = self.coef.shape
        self.mv = np.zeros((S, nb, 2), np.int8) if mv is None else np.ascontiguousarray(mv, np.int8)
        self.has = np.ones((S, nb), np.uint8) if has is None else np.ascontiguousarray(has, np.uint8)
        assert self.mv.shape == (S, nb, 2) and self.has.shape == (S, nb)
        self.expect, self.note = expect, note
        self._truth = None

    @property
    def S(self):
        return self.coef.shape[0]

    @property
    def nb(self):
        return self.coef.shape[1]

    def truth(self):
        """the restatement's payloads, one per stream (computed once, shared by every test of the session)"""
        if self._truth is None:
            self._truth = [E.iframe_payload(self.coef[s]) if self.ptype == 1 else E.pframe_payload(self.mv[s], self.has[s], self.coef[s])
                           for s in range(self.S)]
        return self._truth


class Case:
    def __init__(self, name, nb, frames, cap=0, fetch_all=False, large=False):
        self.name, self.nb, self.frames, self.cap, self.fetch_all, self.large = name, nb, frames, cap, fetch_all, large
        self.w, self.h = GEOM[nb]
        assert all(f.nb == nb and f.S == frames[0].S for f in frames) and frames[0].S <= 32
        self.S = frames[0].S


# ------------------------------------------------------------------------------------------------ the restatement's view of a payload
class Layout:
    """where the restatement puts every symbol of one stream's payload, in the units k_ent_pack works in: a SYMBOL is one word of the group's
    list -- a value run or a closing run with the fillers in front of it.  bit: first bit of the run's code pair (behind its fillers);
    length: code pair + value bits; start / span: the same with the fillers"""

    def __init__(self, ptype, coef, mv, has):
        nb = coef.shape[0]
        blocks = E._runs(coef, has if ptype == 2 else None)
        self.table, self.vals, self.lens = E._tree_for(blocks, None)
        lens = self.lens
        hdr = np.zeros(nb, np.int64)
        if ptype == 2:
            hdr[:] = np.where((np.asarray(mv) != 0).any(axis=1), 16, 2)
        self.hdr_base = [HEAD_BITS + int(hdr[:g].sum()) for g in range(0, nb, GROUP_MBS)]
        self.hdr_bits = [int(hdr[g:g + GROUP_MBS].sum()) for g in range(0, nb, GROUP_MBS)]
        bit = HEAD_BITS + int(hdr.sum())
        self.sym_start = bit
        n_groups = (nb + GROUP_MBS - 1) // GROUP_MBS
        self.groups = [[] for _ in range(n_groups)]          # per group: (start, span, bit, length, z, s)
        for b, seq in enumerate(blocks):
            g = b // GROUP_MBS
            if seq is None:
                continue
            start = bit
            for k, (z, s, _) in enumerate(seq):
                n = lens[z] + lens[s] + s
                if (z, s) == (15, 0) and k + 1 < len(seq):    # a filler: part of the next run's word
                    bit += n
                    continue
                self.groups[g].append((start, bit + n - start, bit, n, z, s))
                bit += n
                start = bit
        self.end_bit = bit
        self.n_bytes = (bit + 7) // 8
        self.symbols = [x for grp in self.groups for x in grp]

    def n_words(self):
        return [len(g) for g in self.groups]

    def straddles(self):
        """symbols whose bits reach a third payload word: (bit & 31, length)"""
        return [(b & 31, n) for _, _, b, n, _, _ in self.symbols if (b & 31) + n > 64]

    def window_events(self, win_bits):
        """k_ent_pack's window, restated from its description alone: per group the symbols go 256 at a time; a step that would run past
        the window re-anchors it at the running offset; a symbol that still does not fit goes to memory.  Counts of: steps that fill the
        window to its last bit, steps one bit over, re-anchorings, symbols on the memory path and those among them that reach a third word"""
        ev = dict(exact=0, one_over=0, anchors=0, mem=0, mem_straddles=0, fit_last_bit=0)
        for g, grp in enumerate(self.groups):
            if not grp:
                continue
            running = grp[0][0] & 31
            for k in range(0, len(grp), STEP):
                step = grp[k:k + STEP]
                total = sum(x[1] for x in step)
                ev["exact"] += running + total == win_bits
                ev["one_over"] += running + total == win_bits + 1
                if running + total > win_bits:
                    ev["anchors"] += 1
                    running &= 31
                off = running
                for start, span, bit, n, _, _ in step:
                    if off + span > win_bits:
                        ev["mem"] += 1
                        ev["mem_straddles"] += (bit & 31) + n > 64
                    ev["fit_last_bit"] += off + span == win_bits
                    off += span
                running += total
        return ev


def layouts(frame):
    return [Layout(frame.ptype, frame.coef[s], frame.mv[s], frame.has[s]) for s in range(frame.S)]


def worst_step_bits():
    """the most bits one step of k_ent_pack (256 symbols of one group) can take: every symbol costs at least its own coefficient and 15 more
    per filler, a group has 64 x 256 coefficients, a code is at most 15 bits (16 leaves): F fillers of 30 bits, 256 runs of 30 + 15"""
    fillers = (GROUP_MBS * 256 - STEP) // 15
    return fillers * 30 + STEP * 45


assert worst_step_bits() + 31 <= WIN_BITS, "the production window can be overrun by one step: the memory path is reachable"


# ------------------------------------------------------------------------------------------------ long_symbols
def _exact_histogram_mbs(hist, nb, reserved, rng):
    """macroblocks (lists of (z, s) pairs) whose runs count exactly `hist`: every macroblock is tiled to its 256th coefficient by value runs
    (no filler, no closing run).  reserved: pairs the caller wants in the first macroblocks, taken out of the budget; those macroblocks are
    filled up with runs of one coefficient (no zero in front)"""
    H = [int(x) for x in hist]
    n_pairs, odd = divmod(sum(H), 2)
    assert not odd and H[15] == H[14]
    # which bins stand in front (zeros) and which behind (sizes): 0 and 1 are never a size, 15 would be a filler in front, 14 pairs with 15
    z_side = [0] * 16
    z_side[0], z_side[1], z_side[14] = H[0], H[1], H[14]
    extra = n_pairs - sum(z_side)
    need = nb * 256 - n_pairs - sum(k * z_side[k] for k in range(16))      # zeros the extra runs have to bring
    assert extra >= 0 and need >= 2 * extra, (extra, need)
    up = need - 2 * extra                                                 # runs of 3 zeros instead of 2 until the coefficients are used up
    assert extra <= H[2] and up <= min(extra, H[3]), "the histogram does not tile this many macroblocks"
    z_side[2], z_side[3] = extra - up, up
    zs = [k for k in range(16) for _ in range(z_side[k]) if k != 14]
    ss = [k for k in range(16) for _ in range(H[k] - z_side[k]) if k != 15]
    assert len(zs) == len(ss) and min(ss) >= 2
    rng.shuffle(ss)
    pairs = list(zip(zs, ss)) + [(14, 15)] * H[14]
    for p in (p for r in reserved for p in r):
        pairs.remove(p)
    mbs = [list(r) for r in reserved] + [[] for _ in range(nb - len(reserved))]
    room = [256 - sum(z + 1 for z, _ in m) for m in mbs]
    ones = [p for p in pairs if p[0] == 0]
    for i in range(len(reserved)):
        mbs[i] += [ones.pop() for _ in range(room[i])]
        room[i] = 0
    for p in sorted((p for p in pairs if p[0] > 0), key=lambda p: -p[0]):   # first fit, largest first; the single coefficients level out
        i = next(i for i in range(nb) if room[i] >= p[0] + 1)
        mbs[i].append(p)
        room[i] -= p[0] + 1
    for i in range(nb):
        mbs[i] += [ones.pop() for _ in range(room[i])]
    assert not ones and all(sum(z + 1 for z, _ in m) == 256 for m in mbs)
    return mbs


LONG_VALUES = (8192, -8192, 16383, -16383, 12345, -12345)


@functools.lru_cache(None)
def long_symbols():
    """Histogram 3 x entd_cases.TABLE_SKEW, exactly, so the table IS TABLE_SKEW: codes of 2 .. 13 bits, symbols 14 and 15 at 13 bits each.  Each
    stream holds three runs (14, 15, v): 13 + 13 + 15 = 41 bits, the deepest a 16-symbol table of bytes allows (depth reached: 41; pairs
    of 26 bits), v over both signs of 8192, 12345 and 16383.  Stream k puts k runs of 7 bits in front of the first of them, so its bit phase
    takes every value 0 .. 31 over the 32 streams of the launch; the p-frame form moves the symbol section behind 2- and 16-bit block headers.
    The other two follow k % 13 runs of 7 bits at the head of macroblock 1, symbols 242 .. 255 of the group's list: the end of k_ent_pack's first
    step, which the 64-word window of the variant build sends to memory (ent_or_bits_mem)."""
    nb, S = 16, 32
    rng = np.random.default_rng(41)
    hist = [3 * t for t in TABLE_SKEW]
    front = [[(0, 2)] * 31 + [(14, 15)], [(0, 2)] * 12 + [(14, 15)] * 2]
    mbs = _exact_histogram_mbs(hist, nb, front, rng)
    rest = [mbs[i][len(front[i]):] for i in (0, 1)]
    assert len(mbs[0]) == 242
    coef = np.zeros((S, nb, 256), np.int16)
    for s in range(S):
        r = np.random.default_rng([41, s])
        tail = [(0, 2)] * (31 - s) + rest[0]
        head = [[(0, 2)] * s + [(14, 15)] + [tail[i] for i in r.permutation(len(tail))],
                [(0, 2)] * (s % 13) + [(14, 15)] * 2 + [(0, 2)] * (12 - s % 13) + [rest[1][i] for i in r.permutation(len(rest[1]))]]
        n_long = 0
        for b in range(nb):
            seq = head[b] if b < 2 else [mbs[b][i] for i in r.permutation(len(mbs[b]))]
            runs = []
            for z, sz in seq:
                v = None
                if sz == 15:
                    v = LONG_VALUES[(s + n_long) % 6]
                    n_long += 1
                runs.append((z, sz, v))
            coef[s, b] = mb_from_runs(runs, r)
    mv = np.zeros((S, nb, 2), np.int8)
    mv[:, [1, 5, 9]] = (2, -1)                                 # 16 x 2 + 3 x 14 header bits: the symbol section starts 10 bits further into a word
    fi = Frame(1, coef)
    fp = Frame(2, coef, mv=mv)
    _, want_lens = E.tree_codes(TABLE_SKEW)
    for f in (fi, fp):
        ls = layouts(f)
        hits, shifts, phases = 0, set(), set()
        for s, l in enumerate(ls):
            assert l.table.tolist() == list(TABLE_SKEW) and l.lens == want_lens, "the histogram must give TABLE_SKEW exactly"
            longest = max(n for _, _, _, n, _, _ in l.symbols)
            assert longest == 41 >= 34, longest
            assert max(l.lens[z] + l.lens[sz] for _, _, _, _, z, sz in l.symbols) == 26
            st = l.straddles()
            hits += len(st)
            shifts |= {sh for sh, _ in st}
            phases.add(next(b & 31 for _, _, b, n, _, _ in l.groups[0] if n == 41))
            vb_past_31 = [1 for _, _, b, n, z, sz in l.symbols if l.lens[z] + l.lens[sz] + sz > 32]
            assert vb_past_31
        assert phases == set(range(32)), "the first long symbol takes every bit phase over the 32 streams"
        assert hits >= 8 and len(shifts) >= 2, (hits, shifts)
    vals = {int(v) for v in coef[np.abs(coef.astype(np.int32)) >= 8192]}
    assert vals == set(LONG_VALUES)
    return Case("long_symbols", nb, [fi, fp], fetch_all=True)


# ------------------------------------------------------------------------------------------------ degenerate_tables
def _grid_mb(z, sizes, rng):
    """values at z, 2z + 1, ..., 255 (z in {3, 7, 15}: the macroblock ends on a value): runs (z, size) only"""
    assert 256 % (z + 1) == 0
    n = 256 // (z + 1)
    return mb_from_runs([(z, int(sizes[i % len(sizes)]), None) for i in range(n)], rng)


@functools.lru_cache(None)
def degenerate_tables():
    """One stream per table: runs (z, z) for z = 3, 7, 15 -- ONE symbol, a single 255 in the table, a zero-length code, payloads of bare 3- / 7- /
    15-bit values; two symbols with equal counts ((3, 5) runs) and unequal ones ((3, 3) and (3, 7) runs; dense +-1: (0, 2)), one bit each.  As an
    i-frame, and as a p-frame with skipped macroblocks and non-zero vectors (a skipped macroblock keeps its coefficients: they must not count)."""
    nb, S = 20, 6
    rng = np.random.default_rng(7)
    coef = np.zeros((S, nb, 256), np.int16)
    for b in range(nb):
        coef[0, b] = _grid_mb(3, [3], rng)
        coef[1, b] = _grid_mb(7, [7], rng)
        coef[2, b] = _grid_mb(15, [15], rng)
        coef[3, b] = _grid_mb(3, [5], rng)
        coef[4, b] = _grid_mb(3, [3, 3, 7], rng)
        coef[5, b] = rng.choice(np.array([-1, 1], np.int16), 256)
    has = (rng.random((S, nb)) < 0.6).astype(np.uint8)
    has[:, [0, nb - 1]] = [[1, 0], [0, 1], [1, 1], [0, 0], [1, 0], [0, 1]]
    mv = rng.integers(-9, 10, (S, nb, 2)).astype(np.int8)
    mv[:, ::3] = 0
    fi, fp = Frame(1, coef), Frame(2, coef, mv=mv, has=has)
    for f in (fi, fp):
        for s, l in enumerate(layouts(f)):
            present = [k for k in range(16) if l.table[k]]
            if s < 3:
                z = (3, 7, 15)[s]
                assert present == [z] and l.table[z] == 255 and l.lens[z] == 0, "one symbol, zero-length code"
                assert all(n == z for _, _, _, n, _, _ in l.symbols) and l.end_bit == l.sym_start + z * len(l.symbols)
            else:
                assert len(present) == 2 and all(l.lens[k] == 1 for k in present), "two symbols, one bit each"
            assert l.symbols
    return Case("degenerate_tables", nb, [fi, fp], fetch_all=True)


# ------------------------------------------------------------------------------------------------ typical content
def typical(rng, nb, scale=40):
    """low-frequency-heavy, like quantised DCT output in zigzag order"""
    keep = rng.random((nb, 256)) < (0.6 * np.exp(-(np.arange(256) % 64) / 6.0))[None, :]
    return (rng.integers(-scale, scale + 1, (nb, 256)) * keep).astype(np.int16)


def _words_mbs(n, rng):
    """macroblocks whose symbol lists hold exactly n words together: dense ones (256 words, no closing run), one with values on coefficients
    1 .. 255 (255 words) or a lone value on coefficient 255 (1 word)"""
    out = []
    while n >= 256:
        out.append(mb_from_runs([(0, 2 + int(rng.integers(0, 5)), None) for _ in range(256)], rng))
        n -= 256
    if n == 255:
        out.append(mb_from_runs([(1, 3, None)] + [(0, 2, None)] * 254, rng))
    elif n == 1:
        out.append(mb_from_runs([(255, 4, None)], rng))
    else:
        assert n == 0
    return out


WORDS = (0, 1, 255, 256, 257, 512, 513)


@functools.lru_cache(None)
def group_seams(nb):
    """nb in {192, 193, 191}: total_blocks % 64 = 0, 1, 63 (the last group whole, ONE macroblock, one short: ent_stage_rows' 8-byte read of the
    flags against its partial path).  Stream s < 7: group s % 3 holds exactly WORDS[s] symbol words (the prefetch j + 256 < n_list and the
    wave_syms offsets), the other groups typical content; stream 0's middle group is skipped whole between coded ones (n_syms == 0); the first
    and the last macroblock of every group are skipped in the odd streams and coded in the even ones.  The same buffers as an i-frame."""
    S = 8
    rng = np.random.default_rng(nb)
    n_groups = (nb + GROUP_MBS - 1) // GROUP_MBS
    coef = np.stack([typical(rng, nb) for _ in range(S)])
    has = (rng.random((S, nb)) < 0.6).astype(np.uint8)
    firsts = np.arange(0, nb, GROUP_MBS)
    lasts = np.minimum(firsts + GROUP_MBS, nb) - 1
    for s in range(S):
        has[s, firsts] = has[s, lasts] = 1 - s % 2
    exact = {}
    for s, n in enumerate(WORDS):
        g = s % 3 if n else 1                                # (no words: the skipped group is the MIDDLE one)
        if g == n_groups - 1 and nb - firsts[g] < 3:
            g = 0                                             # the one-macroblock group cannot hold 513 words
        lo, hi = firsts[g], lasts[g] + 1
        mbs = _words_mbs(n, rng)
        has[s, lo:hi] = 0
        pick = lo + rng.permutation(hi - lo)[:len(mbs)]
        for b, m in zip(sorted(pick), mbs):
            coef[s, b], has[s, b] = m, 1
        exact[s] = (g, n)
    fp = Frame(2, coef, mv=np.where(rng.random((S, nb, 1)) < 0.3, rng.integers(-15, 16, (S, nb, 2)), 0), has=has)
    fi = Frame(1, coef)
    ls = layouts(fp)
    for s, (g, n) in exact.items():
        assert ls[s].n_words()[g] == n, (s, g, n, ls[s].n_words())
    assert ls[0].n_words()[1] == 0 and ls[0].n_words()[0] > 0 and ls[0].n_words()[2] > 0, "a skipped group between coded ones"
    assert nb % 64 in (0, 1, 63) and n_groups >= 3
    assert {int(has[s, 0]) for s in range(S)} == {0, 1}
    return Case(f"group_seams_{nb}", nb, [fp, fi])


# ------------------------------------------------------------------------------------------------ runs
@functools.lru_cache(None)
def runs():
    """380 macroblocks over 19 streams: a lone value on every coefficient 0 .. 255 (every run length in front, 0 .. 16 fillers; every closing run,
    none included), an empty macroblock (17 fillers), and for each of the 15 sets of non-empty subblocks eight placements: values on the first
    coefficient of each, on the last, on both, and random ones (ent_prev_last: the run in front of a value crosses 0 .. 3 empty subblocks)."""
    nb, S = 20, 19
    rng = np.random.default_rng(255)
    mbs = [mb_from_runs([(p, 2 + p % 14, None)], rng) for p in range(256)]
    for pattern in range(1, 16):
        live = [q for q in range(4) if pattern >> q & 1]
        for k in range(8):
            m = np.zeros(256, np.int16)
            for q in live:
                pos = ([0], [63], [0, 63])[k] if k < 3 else sorted(set(rng.integers(0, 64, 1 + k % 3).tolist()))
                for p in pos:
                    m[64 * q + p] = value_of(2 + int(rng.integers(0, 14)), rng)
            mbs.append(m)
    mbs += [np.zeros(256, np.int16)] * (nb * S - len(mbs))
    assert len(mbs) == nb * S
    order = rng.permutation(len(mbs))
    coef = np.stack([mbs[i] for i in order]).reshape(S, nb, 256)
    has = np.ones((S, nb), np.uint8)
    has[:, 7] = 0
    fi, fp = Frame(1, coef), Frame(2, coef, has=has)
    lead, close, fill, patterns = set(), set(), set(), set()
    for m in coef.reshape(-1, 256):
        nz = np.flatnonzero(m)
        patterns.add(sum(1 << q for q in range(4) if m[64 * q:64 * q + 64].any()))
        gaps = np.diff(np.concatenate([[-1], nz, [256]])) - 1
        lead |= set(gaps[:-1].tolist())
        close.add(int(gaps[-1]))
        fill |= {(int(g) - 1) // 15 if g > 15 else 0 for g in gaps}
    assert set(range(256)) <= lead and set(range(257)) <= close
    assert fill == set(range(18)) and patterns == set(range(16))
    return Case("runs", nb, [fi, fp])


# ------------------------------------------------------------------------------------------------ headers
MV_EDGES = (-64, 63, 64, -65, 127, -128)


@functools.lru_cache(None)
def headers():
    """P-frames of 193 macroblocks (groups of 64, 64, 64 and 1).  A block header is 2 or 16 bits and the headers start at bit 152, so a group's
    hdr_base is even: stream k < 16 has k moving macroblocks in group 0, which puts hdr_base & 31 of group 1 on (24 + 14 k) % 32 -- every even
    value 0 .. 30 (the odd ones cannot occur).  Stream 16: all 64 macroblocks of group 1 move (1 024 header bits from an odd word offset, the
    kEntHdrWords bound).  Stream 17: the vector components -64, 63 and -- outside the 7 bits the packet has room for -- 64, -65, 127, -128: the
    stage and the oracle keep the low 7 bits."""
    nb, S = 193, 18
    rng = np.random.default_rng(16)
    coef = np.stack([typical(rng, nb, 12) for _ in range(S)])
    has = (rng.random((S, nb)) < 0.4).astype(np.uint8)
    mv = np.zeros((S, nb, 2), np.int8)
    for k in range(16):
        pick = rng.permutation(64)[:k]
        mv[k, pick] = rng.integers(1, 16, (k, 2)) * rng.choice([-1, 1], (k, 2))
        mv[k, 64:] = np.where(rng.random((nb - 64, 1)) < 0.2, rng.integers(-15, 16, (nb - 64, 2)), 0)
    mv[16, 3] = (0, -1)
    mv[16, 64:128] = rng.integers(1, 16, (64, 2))
    mv[16, 64, 0], mv[16, 127, 1] = -64, 63
    edge = [(a, b) for a in MV_EDGES for b in (0,) + MV_EDGES]
    mv[17, 10:10 + len(edge)] = edge
    mv[17, 192] = (127, -128)
    f = Frame(2, coef, mv=mv, has=has)
    ls = layouts(f)
    assert {ls[k].hdr_base[1] & 31 for k in range(16)} == set(range(0, 32, 2))
    assert ls[16].hdr_bits[1] == 64 * 16 and ls[16].hdr_base[1] & 31
    assert set(MV_EDGES) <= set(mv[17].reshape(-1).tolist())
    return Case("headers", nb, [f])


# ------------------------------------------------------------------------------------------------ oversize
@functools.lru_cache(None)
def oversize():
    """193 macroblocks (a last group of one).  Each of 16384, -16384, 32767, -32768, -16385 needs 16 or 17 size bits (the reference indexes its
    histogram out of range, src/rle.rs:44): PFV_ERR_FORMAT, with the value in lane 0 of a wavefront (macroblock 16, coefficient 5), in lane 63
    (macroblock 15, coefficient 200) and in the last, partial group (macroblock 192), as i-frames and p-frames alternately; a good frame follows
    every error.  Last: all five values inside macroblocks a p-frame skips -- nothing to report, the oracle's payload."""
    nb, S = 193, 1
    rng = np.random.default_rng(15)
    base = typical(rng, nb)[None]
    has = (rng.random((S, nb)) < 0.7).astype(np.uint8)
    has[0, [15, 16, 192]] = 1
    mv = np.where(rng.random((S, nb, 1)) < 0.3, rng.integers(-15, 16, (S, nb, 2)), 0)
    good = {1: Frame(1, base), 2: Frame(2, base, mv=mv, has=has)}
    frames = []
    k = 0
    assert (4 * 16 + 5 // 64) % 64 == 0 and (4 * 15 + 200 // 64) % 64 == 63 and 192 // GROUP_MBS == 3
    for v in OVERSIZE:
        for b, i in ((16, 5), (15, 200), (192, 77)):          # subblock index 64 = lane 0 of wavefront 1; 63 = lane 63 of wavefront 0
            ptype = 1 + k % 2
            k += 1
            c = base.copy()
            c[0, b, i] = v
            assert E.coeff_size(v) > 15
            frames.append(Frame(ptype, c, mv=mv, has=has, expect="format", note=f"{v} in macroblock {b}"))
            frames.append(good[ptype])
    c = base.copy()
    h = has.copy()
    for n, v in enumerate(OVERSIZE):
        b = (0, 15, 16, 100, 192)[n]
        c[0, b, (0, 255, 64, 128, 3)[n]] = v
        h[0, b] = 0
    hidden = Frame(2, c, mv=mv, has=h, note="oversize values in skipped macroblocks")
    assert len(hidden.truth()[0]) > 19
    frames.append(hidden)
    return Case("oversize", nb, frames)


# ------------------------------------------------------------------------------------------------ capacity
@functools.lru_cache(None)
def capacity():
    """Three i-frames of 3 macroblocks from one family (k values in front): payloads of n, n + 1 and fewer than n bytes with n a multiple of 16.
    The stage is enabled with a capacity of n - 5: it rounds up to n.  n bytes pack, n + 1 report PFV_ERR_NOMEM, the smaller frame packs behind it."""
    nb = 3
    rng = np.random.default_rng(3)
    full = typical(rng, nb, 300)
    full[full == 0] = 1
    sizes = {}
    for k in range(40, nb * 256):
        c = full.copy().reshape(-1)
        c[k:] = 0
        n = len(E.iframe_payload(c.reshape(nb, 256)))
        sizes.setdefault(n, c.reshape(1, nb, 256))
        if n % 16 == 1 and n - 1 in sizes and n > 64:
            break
    else:
        raise AssertionError("no pair of payloads of 16 m and 16 m + 1 bytes in the family")
    n -= 1
    smaller = max(m for m in sizes if m < n)
    frames = [Frame(1, sizes[n]), Frame(1, sizes[n + 1], expect="nomem"), Frame(1, sizes[smaller]), Frame(1, sizes[n])]
    assert [len(f.truth()[0]) for f in frames] == [n, n + 1, smaller, n] and n % 16 == 0
    return Case("capacity", nb, frames, cap=n - 5)


# ------------------------------------------------------------------------------------------------ code_chunks
@functools.lru_cache(None)
def code_chunks(w, h):
    """2048 x 1360 (16 384 macroblocks: exactly 256 groups, one pass of k_ent_codes' loop over the groups) and 2048 x 1376 (258 groups: a second pass
    of two groups); one typical p-frame stream each"""
    nb = total_blocks(w, h)
    GEOM[nb] = (w, h)
    rng = np.random.default_rng(w + h)
    coef = typical(rng, nb, 20)[None]
    has = (rng.random((1, nb)) < 0.5).astype(np.uint8)
    has[0, -1] = 1
    mv = np.where(rng.random((1, nb, 1)) < 0.3, rng.integers(-15, 16, (1, nb, 2)), 0)
    n_groups = (nb + GROUP_MBS - 1) // GROUP_MBS
    assert n_groups == (256 if h == 1360 else 258)
    return Case(f"code_chunks_{w}x{h}", nb, [Frame(2, coef, mv=mv, has=has)], large=True)


# ------------------------------------------------------------------------------------------------ window (variant build)
@functools.lru_cache(None)
def window():
    """For the 64-word window of the variant build (2 048 bits).  Runs (3, 3) and (3, 6) only: two symbols, 5 and 8 bits per run.  The i-frame's
    symbols start at bit 152 (24 into a word): 8 runs of 5 bits and 248 of 8 in the first step fill the window to its last bit -- running + total
    == 2 048, no re-anchoring, the last symbol ends on the window's last bit.  The p-frame starts them at bit 310 (22 into a word) and its first step
    takes 7 runs of 5 bits and 249 of 8: 2 049, one bit over -- its last symbol alone takes the memory path.  Dense 15-bit values (a third frame) make single steps larger than the window: the
    memory path.  In the production build (2 048 words) no step can overflow the window: ent_cases.worst_step_bits() = 43 770 bits, from the
    coefficients a group has to spend on fillers, against 65 536."""
    nb = 16
    rng = np.random.default_rng(64)

    def frame(n8_first):
        sizes = [6] * n8_first + [3] * (256 - n8_first)
        c = np.zeros((1, nb, 256), np.int16)
        for b in range(nb):
            s4 = sizes[64 * b:64 * b + 64] if b < 4 else rng.choice([3, 6], 64).tolist()
            c[0, b] = _grid_mb(3, s4, rng)
        return c
    fi = Frame(1, frame(248))
    mv = np.zeros((1, nb, 2), np.int8)
    mv[0, 3:12] = (1, -2)                                      # 16 x 2 + 9 x 14 = 158 header bits: the symbols start at bit 310 = 9 * 32 + 22
    fp = Frame(2, frame(249), mv=mv)
    dense = rng.integers(8192, 16384, (1, nb, 256)) * rng.choice([-1, 1], (1, nb, 256))
    fd = Frame(1, dense)
    ei, ep, ed = (layouts(f)[0].window_events(WIN_BITS_SMALL) for f in (fi, fp, fd))
    assert layouts(fi)[0].sym_start & 31 == 24 and layouts(fp)[0].sym_start & 31 == 22
    assert ei["exact"] >= 1 and ei["fit_last_bit"] >= 1 and ei["mem"] == 0, ei
    assert ep["one_over"] >= 1 and ep["mem"] == 1, ep       # (the step is the group's first: re-anchoring gains nothing, its last symbol goes to memory)
    assert ed["mem"] > 100, ed
    for f in (fi, fp, fd):
        assert layouts(f)[0].window_events(WIN_BITS)["mem"] == 0
    return Case("window", nb, [fi, fp, fd])


def window_seams_of(case):
    """(symbols on the memory path, those of them that reach a third word) of a case in the variant build"""
    ev = [l.window_events(WIN_BITS_SMALL) for f in case.frames if f.expect == "ok" for l in layouts(f)]
    return sum(e["mem"] for e in ev), sum(e["mem_straddles"] for e in ev)


# ------------------------------------------------------------------------------------------------ running a case
CASES = {"long_symbols": long_symbols, "degenerate_tables": degenerate_tables, "group_seams_192": functools.partial(group_seams, 192),
         "group_seams_193": functools.partial(group_seams, 193), "group_seams_191": functools.partial(group_seams, 191), "runs": runs,
         "headers": headers, "oversize": oversize, "capacity": capacity}
LARGE = {"code_chunks_256_groups": functools.partial(code_chunks, 2048, 1360), "code_chunks_258_groups": functools.partial(code_chunks, 2048, 1376)}
WINDOW = {"window": window, "long_symbols": long_symbols, "degenerate_tables": degenerate_tables}


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _oracle_lib(oracle):
    L = oracle.L
    L.pfvo_serialize_iframe.restype = ctypes.c_size_t
    L.pfvo_serialize_iframe.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t]
    L.pfvo_serialize_pframe.restype = ctypes.c_size_t
    L.pfvo_serialize_pframe.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t]
    return L


def oracle_payload(oracle, frame, s):
    """the C oracle's payload of stream s"""
    L = _oracle_lib(oracle)
    nb = frame.nb
    ref = np.zeros(152 // 8 + nb * 2 + nb * 256 * 6 + 64, np.uint8)
    if frame.ptype == 2:
        n = L.pfvo_serialize_pframe(_p(frame.mv[s]), _p(frame.has[s]), _p(frame.coef[s]), nb, _p(ref), ref.size)
    else:
        n = L.pfvo_serialize_iframe(_p(frame.coef[s]), nb, _p(ref), ref.size)
    return ref[:n].tobytes()


def _same(got, want, what):
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        n = min(a.size, b.size)
        bad = np.flatnonzero(a[:n] != b[:n])
        raise AssertionError(f"{what}: {a.size} bytes against {b.size}, first difference at byte {int(bad[0]) if bad.size else n}")


def check_truths(oracle, case):
    """the two oracles agree on every good frame of the case (the restatement's word is then the truth of the other checks)"""
    for k, f in enumerate(case.frames):
        if f.expect == "format":
            continue
        for s in range(f.S):
            _same(oracle_payload(oracle, f, s), f.truth()[s], f"{case.name} frame {k} stream {s}: C oracle against the restatement")


def check_device(pkg, ctx, oracle, case, truth="both"):
    """every frame of the case through EncoderSession.pack_*_dev / payload_sizes / payload (and payloads(): k_ent_gather) on `ctx`.
    truth: "both", or "c" (the large cases: the C oracle, and the restatement's histogram and table)"""
    lib = ctx._lib
    assert int(pkg._lib.load().pfv_total_blocks(case.w, case.h)) == case.nb
    enc = pkg.EncoderSession(ctx, case.w, case.h, 5, case.S)
    enc.enable_entropy(case.cap)
    nb, S = case.nb, case.S
    assert enc.total_blocks == nb
    if case.cap:
        assert int(lib.pfv_enc_payload_capacity(enc.handle)) == (case.cap + 15) // 16 * 16
    d_coef, d_mv, d_has = ctx.alloc(S * nb * 512), ctx.alloc(S * nb * 2), ctx.alloc(S * nb)
    checked = 0
    try:
        if truth == "both":
            check_truths(oracle, case)
        for k, f in enumerate(case.frames):
            what = f"{case.name} frame {k} ({'ip'[f.ptype - 1]}-frame{', ' + f.note if f.note else ''})"
            ctx.upload(d_coef, f.coef)
            if f.ptype == 2:
                ctx.upload(d_mv, f.mv); ctx.upload(d_has, f.has)
                enc.pack_pframe_dev(d_mv, d_has, d_coef)
            else:
                enc.pack_iframe_dev(d_coef)
            if f.expect != "ok":
                code = pkg._lib.PFV_ERR_FORMAT if f.expect == "format" else pkg._lib.PFV_ERR_NOMEM
                try:
                    enc.payload_sizes()
                except pkg.PfvError as e:
                    assert e.code == code, (what, e.code, code)
                else:
                    raise AssertionError(f"{what}: no error reported, {f.expect} expected")
                checked += 1
                continue
            sizes = enc.payload_sizes()
            if truth == "both":
                want = f.truth()
            else:
                want = [oracle_payload(oracle, f, s) for s in range(S)]
                for s in range(S):
                    table = E.normalise(E.histogram(f.coef[s], f.has[s] if f.ptype == 2 else None))
                    assert list(want[s][:16]) == table.tolist(), f"{what}: the C oracle's table against the restatement's"
            for s in range(S):
                assert int(sizes[s]) == len(want[s]), (what, s, int(sizes[s]), len(want[s]))
                _same(enc.payload(s, len(want[s])), want[s], f"{what} stream {s}: device stage against the oracle")
                checked += 1
            if case.fetch_all:
                out = np.full(sum((len(x) + 15) // 16 * 16 for x in want), 0xA5, np.uint8)
                sizes2, offs = enc.payloads(out)
                assert sizes2.tolist() == [len(x) for x in want] and all(int(o) % 16 == 0 for o in offs)
                for s in range(S):
                    _same(out[int(offs[s]):int(offs[s]) + int(sizes2[s])].tobytes(), want[s], f"{what} stream {s}: pfv_enc_payloads_fetch")
    finally:
        for p in (d_coef, d_mv, d_has):
            ctx.free(p)
        enc.close()
    return checked


def check_host(pkg, lib, oracle, case):
    """the host coder: pfv_serialize_*_payload == the restatement's bytes, and pfv_parse_*_payload / pfv_parse_payload_sparse read the buffers back
    (a skipped macroblock's coefficients as zeros, a vector component as its low 7 bits, sign-extended)"""
    nb = case.nb
    cap = 19 + nb * 2 + nb * 256 * 6 + 64
    checked = 0
    for k, f in enumerate(case.frames):
        for s in range(f.S):
            what = f"{case.name} frame {k} stream {s}"
            out = np.zeros(cap, np.uint8)
            if f.ptype == 2:
                n = lib.pfv_serialize_pframe_payload(_p(f.mv[s]), _p(f.has[s]), _p(f.coef[s]), nb, _p(out), cap)
            else:
                n = lib.pfv_serialize_iframe_payload(_p(f.coef[s]), nb, _p(out), cap)
            if f.expect == "format":
                assert n == 0, f"{what}: an oversize coefficient must be refused"
                continue
            payload = out[:n].copy()
            _same(payload.tobytes(), f.truth()[s], f"{what}: host coder against the restatement")
            want = f.coef[s] * f.has[s][:, None].astype(np.int16) if f.ptype == 2 else f.coef[s]
            want_mv = (((f.mv[s].astype(np.int16) + 64) & 127) - 64).astype(np.int8)
            got, q = np.full((nb, 256), 77, np.int16), np.zeros(3, np.uint8)
            omv, ohas = np.zeros((nb, 2), np.int8), np.zeros(nb, np.uint8)
            if f.ptype == 2:
                rc = lib.pfv_parse_pframe_payload(_p(payload), payload.size, nb, 4, _p(omv), _p(ohas), _p(got), _p(q))
            else:
                rc = lib.pfv_parse_iframe_payload(_p(payload), payload.size, nb, 4, _p(got), _p(q))
            assert rc == 0 and np.array_equal(got, want), f"{what}: the parser does not give the buffers back (rc {rc})"
            if f.ptype == 2:
                assert np.array_equal(omv, want_mv) and np.array_equal(ohas, f.has[s]), what
            idx, val, cnt = np.zeros(nb * 256, np.uint32), np.zeros(nb * 256, np.int16), ctypes.c_size_t()
            rc = lib.pfv_parse_payload_sparse(int(f.ptype == 2), _p(payload), payload.size, nb, 4, _p(omv), _p(ohas), _p(idx), _p(val),
                                              idx.size, ctypes.byref(cnt), _p(q))
            dense = np.zeros(nb * 256, np.int16)
            dense[idx[:cnt.value]] = val[:cnt.value]
            assert rc == 0 and np.array_equal(dense.reshape(nb, 256), want), f"{what}: the sparse parser (rc {rc})"
            checked += 1
    return checked
