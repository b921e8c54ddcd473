"""Crafted payloads for the decoder's entropy stage on the device (csrc/pfv_entdec_kernels.hip: k_entd_sync / _fix / _verify / _prefix / _emit,
k_hdr_*), shared by the emulator tests (test_emulated_kernels.py: test_emu_entd_*) and the GPU tests (test_gpu_entd.py).

k_entd_emit decides for every packet whether the host parser would have accepted the payload and produced the same array; what it is not
sure of goes to the host parser (kEdIrregular).  A wrong "sure" is silent, so every accept / reject rule gets a payload built for it here --
from RUN LISTS (num_zeroes, coeff_size, value), not from coefficients: most of these payloads no encoder writes.  The truth of every case
is the oracle's decoder (oracle/pfv_oracle_entropy.c, a restatement of src/dec.rs:226-417), call by call to the end of the stream and
beyond an error; the payloads are written with the numpy restatement's BitWriter / tree_codes / packet / stream_header.

A case stream is three packets: a valid i-frame, the crafted packet, a valid p-frame (what follows a rejected packet is checked too: the
framebuffer behind a failed or host-parsed packet is the oracle's).  A case is REGULAR (every packet must be read on the device) or
IRREGULAR (k_entd_emit must mark the crafted packet: left_irregular >= 1, nothing unsettled)."""
from __future__ import annotations

import numpy as np

import pfv_oracle_entropy_np as E

ORG = 152                           # first bit behind the table and the q indices: the lanes are counted from here (EdPacket::org)
LANE = 256                          # payload bits per lane, default shape (kEdSubBits)
SEAMS = (32, None, 1024)            # 32-bit lanes: 240 x 32 = 7 680 bits per workgroup, seams and k_entd_fix inside small payloads
# every one of the 16 symbols has a code (a table of fewer than two symbols never reaches the device reader)
TABLE_FLAT = (200, 180, 160, 140, 120, 100, 90, 80, 70, 60, 50, 40, 30, 20, 10, 5)      # code lengths 3 .. 7
TABLE_SKEW = (255, 255, 255, 233, 144, 89, 55, 34, 21, 13, 8, 5, 3, 2, 1, 1)            # 2 .. 13: symbols 13 / 14 / 15 take 12 / 13 / 13 bits
QIDX = {1: (0, 1, 1), 2: (2, 3, 3)}


def codes(table):
    vals, lens = E.tree_codes(table)
    assert all(lens), "every symbol needs a code"
    return vals, lens


assert codes(TABLE_FLAT)[1] == [3, 3, 3, 3, 4, 4, 4, 4, 4, 4, 5, 5, 5, 6, 7, 7]
assert codes(TABLE_SKEW)[1] == [2, 2, 3, 3, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 13]


def smallest(s):
    return -(1 << (s - 1))


def largest(s):
    return (1 << (s - 1)) - 1


class Runs:
    """one run stream (a coded p-frame macroblock: 256 coefficients; an i-frame: all of them) with the bookkeeping a case needs: the bit the
    next run starts at and the coefficient it starts at"""

    def __init__(self, lens, bit, limit, rng):
        self.lens, self.bit, self.limit, self.rng = lens, int(bit), int(limit), rng
        self.idx = 0
        self.runs = []

    def bits_of(self, z, s):
        return self.lens[z] + self.lens[s] + s

    def add(self, z, s, v=0):
        self.runs.append((int(z), int(s), int(v)))
        self.bit += self.bits_of(z, s)
        self.idx += z + (1 if s else 0)
        return self

    def random_value(self, s):
        return int(self.rng.integers(smallest(s), largest(s) + 1))

    def skip_bits_to(self, target):
        """value runs without zeros in front (one coefficient each) so that the next run starts exactly at bit `target`"""
        gap = int(target) - self.bit
        assert gap >= 0
        coins = {}
        for s in range(1, 16):
            coins.setdefault(self.bits_of(0, s), s)
        best = [None] * (gap + 1)          # best[g]: (runs, last coin) of the fewest runs that take g bits
        best[0] = (0, 0)
        for g in range(1, gap + 1):
            for c in coins:
                if c <= g and best[g - c] is not None and (best[g] is None or best[g - c][0] + 1 < best[g][0]):
                    best[g] = (best[g - c][0] + 1, c)
        assert best[gap] is not None, f"no run sequence takes exactly {gap} bits"
        while gap:
            c = best[gap][1]
            self.add(0, coins[c], self.random_value(coins[c]))
            gap -= c
        assert self.bit == target and self.idx < self.limit - 64, "the crafted run must fit behind the runs in front of it"
        return self

    def to_index(self, index):
        """(15, 0) fillers and one shorter run of zeros up to coefficient `index`"""
        assert self.idx <= index <= self.limit
        while index - self.idx > 15:
            self.add(15, 0)
        if index > self.idx:
            self.add(index - self.idx, 0)
        return self

    def close(self, p_value=0.5, max_size=6, upto=None):
        """ordinary runs up to exactly coefficient `upto` (default: the stream's last)"""
        upto = self.limit if upto is None else upto
        while self.idx < upto:
            rem = upto - self.idx
            if self.rng.random() < p_value:
                s = int(self.rng.integers(1, max_size + 1))
                self.add(int(self.rng.integers(0, min(15, rem - 1) + 1)), s, self.random_value(s))
            else:
                self.add(int(self.rng.integers(1, min(15, rem) + 1)), 0)
        return self


class Payload:
    """table, q indices, block headers (p-frames), run streams; bytes(): padded to whole bytes with zeros or ones, cut or extended by whole bytes"""

    def __init__(self, table, ptype, total_blocks, rng, mv=None, has=None):
        self.table, self.ptype, self.tb, self.rng = tuple(table), ptype, int(total_blocks), rng
        self.vals, self.lens = codes(table)
        self.w = E.BitWriter()
        self.nbits = 0
        for t in self.table:
            self.put(8, t)
        for q in QIDX[ptype]:
            self.put(8, q)
        assert self.nbits == ORG
        self.streams = []
        if ptype == 2:
            self.has = np.ones(self.tb, bool) if has is None else np.asarray(has, bool)
            mv = np.zeros((self.tb, 2), np.int64) if mv is None else np.asarray(mv, np.int64)
            for b in range(self.tb):
                moving = bool(mv[b, 0] or mv[b, 1])
                self.put(1, int(moving))
                self.put(1, int(self.has[b]))
                if moving:
                    self.w.write_signed(7, int(mv[b, 0])); self.w.write_signed(7, int(mv[b, 1]))
                    self.nbits += 14
        self.bit0 = self.nbits

    def put(self, n, v):
        self.w.write(n, v)
        self.nbits += n

    @property
    def end_bit(self):
        return self.streams[-1].bit if self.streams else self.bit0

    def stream(self):
        """the next run stream: the next coded macroblock of a p-frame, THE stream of an i-frame"""
        assert self.ptype == 2 or not self.streams
        r = Runs(self.lens, self.end_bit, 256 if self.ptype == 2 else self.tb * 256, self.rng)
        self.streams.append(r)
        return r

    def n_streams(self):
        return int(self.has.sum()) if self.ptype == 2 else 1

    def fill(self, **kw):
        """ordinary run streams for whatever the case has not written itself"""
        if self.streams and self.streams[-1].idx < self.streams[-1].limit:
            self.streams[-1].close(**kw)
        while len(self.streams) < self.n_streams():
            self.stream().close(**kw)
        return self

    def bytes(self, pad=0, cut=0, extend=b""):
        for r in self.streams:
            for z, s, v in r.runs:
                self.put(self.lens[z], self.vals[z])
                self.put(self.lens[s], self.vals[s])
                if s:
                    self.w.write_signed(s, v)
                    self.nbits += s
        assert self.nbits == self.end_bit
        self.pad_bits = -self.nbits % 8
        if pad and self.pad_bits:
            self.put(self.pad_bits, (1 << self.pad_bits) - 1)
        out = self.w.bytes()
        assert len(out) == (self.end_bit + 7) // 8
        return (out[:len(out) - cut] if cut else out) + bytes(extend)


def with_end_residue(make, residue, tries=400):
    """make(seed) -> Payload; the first seed whose run streams end on a bit that is `residue` modulo 8"""
    for seed in range(tries):
        p = make(seed)
        if p.end_bit % 8 == residue:
            return p
    raise AssertionError(f"no seed in {tries} ends on residue {residue}")


class Case:
    def __init__(self, name, ptype, payload, regular, oracle_accepts=True, why=""):
        self.name, self.ptype, self.payload, self.regular, self.oracle_accepts, self.why = name, ptype, payload, regular, oracle_accepts, why


def build_cases(tb, large=False):
    """every crafted packet for a frame of `tb` macroblocks.  large: only the noise-like pair whose payloads span several workgroups"""
    cases = []
    _, LS = codes(TABLE_SKEW)
    first_last = np.zeros(tb, bool)
    first_last[[0, tb - 1]] = True

    def reg(name, ptype, payload):
        cases.append(Case(name, ptype, payload, True))

    def irr(name, ptype, payload, accepts, why):
        cases.append(Case(name, ptype, payload, False, accepts, why))

    def rng_of(name, seed=0):
        return np.random.default_rng([sum(name.encode()), len(name), seed])

    if large:
        for ptype in (1, 2):
            p = Payload(TABLE_FLAT, ptype, tb, rng_of("large", ptype)).fill(p_value=0.7, max_size=9)
            data = p.bytes()
            assert len(data) > 240 * LANE // 8, "the payload must span two workgroups at the default lane size"
            reg(f"large_{'ip'[ptype - 1]}", ptype, data)
        return cases

    # ---- regular: last run of the last macroblock ends on the payload's last bit (0 pad bits); 1 .. 7 pad bits of ones
    for pad in range(8):
        p = with_end_residue(lambda seed: Payload(TABLE_FLAT, 2, tb, rng_of("pad", seed)).fill(), -pad % 8)
        data = p.bytes(pad=1)
        assert p.pad_bits == pad and (pad == 0 or data[-1] >> (8 - pad) == (1 << pad) - 1)
        reg(f"pad{pad}_ones", 2, data)
    # ---- regular: the fields of one run straddle a lane limit (org + 256; it is a limit of the 32-bit lanes too): first code, second code, value
    z, s = 13, 12                                     # 12 + 11 code bits, 12 value bits
    for what, before in (("code1", 6), ("code2", LS[z] + 5), ("value", LS[z] + LS[s] + 6)):
        p = Payload(TABLE_SKEW, 2, tb, rng_of(what))
        r = p.stream().skip_bits_to(ORG + LANE - before)
        assert r.bit < ORG + LANE < r.bit + r.bits_of(z, s)
        r.add(z, s, smallest(s) + 5)
        reg(f"straddle_{what}", 2, p.fill().bytes())
    # ---- regular: ed_run's windows.  used + coeff_size = 32 and 33 (the value just fits / needs the re-window), each with the value's top
    # bit set and clear; a first code of 12 and of 13 bits (the first re-window) in front of a long second code and a 15-bit value
    p = Payload(TABLE_SKEW, 2, tb, rng_of("windows"))
    r = p.stream()
    for z, s in ((5, 15), (12, 11), (6, 15), (13, 11), (10, 12), (11, 12)):
        assert LS[z] <= 12 and LS[z] + LS[s] + s == (32 if (z, s) in ((5, 15), (12, 11), (10, 12)) else 33)
        r.add(z, s, smallest(s)).add(z, s, largest(s)).add(z, s, smallest(s) + 1)
    r.close()
    r = p.stream()
    for z in (13, 14, 15, 13, 15):
        assert LS[z] == (12 if z == 13 else 13) and LS[15] == 13
        r.add(z, 15, smallest(15) + z).add(z, 15, largest(15) - z)
    r.close()
    reg("windows", 2, p.fill().bytes())
    # ---- regular: values of every size at both ends of its range, both tables
    for tname, table in (("flat", TABLE_FLAT), ("skew", TABLE_SKEW)):
        p = Payload(table, 2, tb, rng_of("sizes"))
        r = p.stream()
        for s in range(1, 16):
            r.add(s % 3, s, smallest(s)).add(0, s, largest(s))
        r.close()
        reg(f"sizes_{tname}", 2, p.fill().bytes())
    # ---- regular, i-frame (one run stream): (15, 0) fillers across macroblock boundaries -- crossing one, ending exactly on one, a value on
    # a macroblock's last and first coefficient, a macroblock without any value; the closing run overshoots the frame without a value
    # (accepted by the reference: the loop of src/dec.rs:261 just ends)
    for name, over in (("fillers_i", 0), ("overshoot_i_no_value", 9)):
        p = Payload(TABLE_FLAT, 1, tb, rng_of(name))
        r = p.stream()
        r.close(upto=250).add(15, 0)                              # 250 -> 265: crosses 256
        r.close(upto=512 - 15).add(15, 0)                         # ends exactly on 512
        r.close(upto=767 - 3).add(3, 4, -7)                       # a value on coefficient 767, the next run starts macroblock 3
        r.close(upto=1019).add(5, 3, 3)                           # a value on coefficient 1024: zeros cross, the value opens macroblock 4
        r.close(upto=1270).to_index(1550)                         # macroblock 5 (1280 .. 1535) holds no value
        r.close(upto=r.limit - 20).to_index(r.limit - 6)
        r.add(6 + over, 0)
        reg(name, 1, p.bytes())
    # ---- regular: only the first / the last / the first and the last macroblock coded
    for name, which in (("coded_first", [0]), ("coded_last", [tb - 1]), ("coded_first_last", [0, tb - 1])):
        has = np.zeros(tb, bool)
        has[which] = True
        reg(name, 2, Payload(TABLE_FLAT, 2, tb, rng_of(name), has=has).fill().bytes())
    # ---- regular: a coded macroblock without any value (17 fillers and one zero), between ordinary ones
    p = Payload(TABLE_FLAT, 2, tb, rng_of("no_value"))
    p.stream().close()
    p.stream().to_index(255).add(1, 0)
    p.stream().to_index(256)                                      # 17 x (15, 0), then (1, 0) again: the same by to_index
    reg("no_value_mb", 2, p.fill().bytes())
    # ---- regular: pairs of codes of 12 and of 13 bits together, the second code's top bit set (the pair table of k_entd_sync ends at 12;
    # k_entd_emit has none: both must agree)
    for total, pairs in ((12, ((10, 2), (11, 0))), (13, ((11, 2), (12, 0)))):
        p = Payload(TABLE_SKEW, 2, tb, rng_of("pairs", total), has=first_last | (np.arange(tb) % 3 == 1))
        for k in range(p.n_streams()):
            r = p.stream()
            while r.idx + 14 < 256:
                zz, ss = pairs[int(p.rng.integers(0, 2))] if k % 2 == 0 else pairs[0]
                assert LS[zz] + LS[ss] == total and (p.vals[ss] >> (LS[ss] - 1)) & 1
                r.add(zz, ss, r.random_value(ss) if ss else 0)
            r.close()
        reg(f"pairs{total}", 2, p.bytes())
    p = Payload(TABLE_FLAT, 2, tb, rng_of("pairs_flat"))
    for k in range(p.n_streams()):
        r = p.stream()
        while r.idx + 16 < 256:
            zz, ss = ((13, 14), (14, 13), (15, 13), (10, 14), (13, 13))[int(p.rng.integers(0, 5))]
            r.add(zz, ss, r.random_value(ss))
        r.close()
    reg("pairs_flat", 2, p.bytes())
    # ---- regular: bytes behind the last coefficient (the reference stops reading, src/dec.rs:261, :382)
    reg("trailing_p", 2, Payload(TABLE_FLAT, 2, tb, rng_of("trailing_p")).fill().bytes(extend=b"\xff\x00\xa5\xff\xff\x3c\xff"))
    reg("trailing_i", 1, Payload(TABLE_FLAT, 1, tb, rng_of("trailing_i")).fill().bytes(extend=b"\xff" * 40))

    # ---- irregular, p-frame: a macroblock closed exactly on coefficient 256 by a run that carries a value (the reference indexes
    # block_coeff[256]); runs that overshoot to 257 and to 270 (the furthest a run can reach: 255 + 15), with and without a value -- without,
    # the reference just leaves its loop and accepts
    for name, at, zeros, size, accepts in (("close256_value", 250, 6, 3, False), ("over257_value", 250, 7, 3, False), ("over257", 250, 7, 0, True),
                                           ("over270_value", 255, 15, 2, False), ("over270", 255, 15, 0, True)):
        # in the second macroblock, ordinary ones behind it -- and as the payload's very last run: the lanes behind a miscounted run start one
        # coefficient off and mark the packet themselves, so only there does the rule stand alone
        for where in ("early", "last"):
            p = Payload(TABLE_FLAT, 2, tb, rng_of(name))
            while len(p.streams) < (1 if where == "early" else p.n_streams() - 1):
                p.stream().close()
            r = p.stream().close(upto=at - 1).add(0, 2, 1)       # a value on coefficient at - 1: the run below starts at `at`
            assert r.idx == at
            r.add(zeros, size, 1 if size else 0)
            r.limit = r.idx                                       # (the stream is over as far as the builder is concerned)
            irr(f"p_{name}_{where}", 2, p.fill().bytes(), accepts, "a p-frame macroblock's runs must end exactly on its 256th coefficient, without a value")
    # ---- irregular, i-frame: the frame's closing run carries a value -- exactly on the last coefficient's successor, and well beyond it
    for name, zeros in (("close_value", 6), ("beyond_value", 15)):
        p = Payload(TABLE_FLAT, 1, tb, rng_of(name))
        r = p.stream()
        r.close(upto=r.limit - 6)
        r.add(zeros, 4, -3)
        r.limit = r.idx
        irr(f"i_{name}", 1, p.bytes(), False, "a value behind the last coefficient")
    # ---- irregular: the last run's value ends 1, 7, 8 and 9 bits behind the payload.  The missing bits are zeros in the uncut payload: the
    # device stages zeros there and would read the right value
    for ptype in (2, 1):
        for missing in (1, 7, 8, 9):
            def make(seed, ptype=ptype):
                p = Payload(TABLE_FLAT, ptype, tb, rng_of("past", seed))
                if ptype == 2:
                    while len(p.streams) < p.n_streams() - 1:
                        p.stream().close()
                r = p.stream()
                r.close(upto=r.limit - 1).add(0, 12, 1)           # 12 value bits, the upper 11 of them zeros
                return p
            p = with_end_residue(make, missing % 8)
            data = p.bytes(cut=(missing + 7) // 8)
            assert p.end_bit - 8 * len(data) == missing
            irr(f"{'ip'[ptype - 1]}_past{missing}", ptype, data, False, "a field that runs past the payload")
    # ---- irregular: the payload ends on a run boundary (and a byte boundary) before the last coefficient: one macroblock short, one run short
    for name in ("mb_short", "run_short"):
        def make(seed, name=name):
            p = Payload(TABLE_FLAT, 2, tb, rng_of(name, seed))
            while len(p.streams) < p.n_streams() - 1:
                p.stream().close()
            if name == "run_short":
                r = p.stream()
                r.close(upto=240)
                r.limit = r.idx                                   # the closing runs are missing
            return p
        irr(f"p_{name}", 2, with_end_residue(make, 0).bytes(), False, "the payload ends before the last coefficient")
    def make_i(seed):
        p = Payload(TABLE_FLAT, 1, tb, rng_of("i_short", seed))
        r = p.stream()
        r.close(upto=r.limit - 300)
        r.limit = r.idx
        return p
    irr("i_mb_short", 1, with_end_residue(make_i, 0).bytes(), False, "the payload ends before the last coefficient")
    # ---- irregular: an empty run region -- the block headers (2 bits per macroblock, 14 more with a vector) end on the payload's last bit,
    # macroblocks are coded
    n_vec = next(k for k in range(5) if (ORG + 2 * tb + 14 * k) % 8 == 0)
    mv = np.zeros((tb, 2), np.int64)
    mv[[5, 6, 9, 10][:n_vec]] = (1, -1)                           # interior luma macroblocks of the 64 x 48 frame
    p = Payload(TABLE_FLAT, 2, tb, rng_of("empty"), mv=mv)
    data = p.bytes()
    assert p.bit0 == 8 * len(data)
    irr("p_empty_run_region", 2, data, False, "coded macroblocks and no bit behind the block headers")
    return cases


def frame_packets(tb, mover, seed=1):
    """the valid packets around the crafted one: an i-frame, and a p-frame with skipped macroblocks and one legal vector (on `mover`, an
    interior luma macroblock)"""
    rng = np.random.default_rng(seed)
    first = Payload(TABLE_FLAT, 1, tb, rng).fill(p_value=0.4, max_size=7).bytes()
    mv = np.zeros((tb, 2), np.int64)
    mv[mover] = (1, -1)
    third = Payload(TABLE_FLAT, 2, tb, rng, mv=mv, has=np.arange(tb) % 3 != 1).fill(p_value=0.4, max_size=5).bytes()
    return first, third


def case_stream(pkg, w, h, case, around, quality=5):
    tabs = pkg.qtables_from_quality(quality)
    head = E.stream_header(w, h, 30, np.stack([np.asarray(tabs[k], np.int64).reshape(64) for k in range(4)]))
    return head + E.packet(E.PKT_IFRAME, around[0]) + E.packet(case.ptype, case.payload) + E.packet(E.PKT_PFRAME, around[1]) + E.packet(E.PKT_EOF)


def outcomes_oracle(oracle, data, n_calls=8):
    """as stream_cases._outcomes_oracle, but beyond an error: the oracle's decoder has consumed the failed packet and left its framebuffer alone
    (as the reference does: the payload is read before it is parsed, src/dec.rs:191-193, :205-207)"""
    from oracle_bind import OracleStreamDecoder
    odec = OracleStreamDecoder(oracle, data)
    assert odec.h
    out = []
    for _ in range(n_calls):
        rc, fr = odec.advance_frame()
        if rc < 0:
            out.append(("err", rc))
            continue
        out.append(("frame", fr.tobytes()) if fr is not None else ("none",))
        if rc == 0:
            out.append(("eof",))
            break
    return out


def outcomes_of(pkg, dec, stats, n_calls=8):
    """one entry per advance_frame call, beyond errors; the object's statistics, read before it is closed"""
    out = []
    try:
        for _ in range(n_calls):
            got = []
            try:
                more = dec.advance_frame(lambda fr: got.append(fr.packed()))
            except pkg.PfvError as e:
                out.append(("err", e.code))
                continue
            out.append(("frame", got[0].tobytes()) if got else ("none",))
            if not more:
                out.append(("eof",))
                break
        return out, dict(stats())
    finally:
        dec.close()


def _kinds(o):
    return [x if x[0] == "err" else x[0] for x in o]


ROUTE = ("packets_read_on_device", "packets_left_to_host_parser", "left_unsettled", "left_irregular")


def check_case(pkg, ctx, oracle, w, h, case, around, shapes=(None, SEAMS), others=True):
    """one case through every decoder object; returns the GOP-batched decoder's route at the first shape"""
    data = case_stream(pkg, w, h, case, around)
    want = outcomes_oracle(oracle, data)
    kinds = _kinds(want)
    # the oracle takes the case as intended: three frames, or the crafted packet fails and the third decodes behind it
    assert kinds[0] == "frame" and kinds[2] == "frame" and kinds[3:] == ["none", "eof"], (case.name, kinds)
    assert (kinds[1] == "frame") == case.oracle_accepts, (case.name, kinds)
    assert case.oracle_accepts or not case.regular
    routes = []
    for shape in shapes:
        dec = pkg.GopDecoder(data, ctx, max_gops=2, max_gop_frames=4, threads=1, entropy="device", entropy_shape=shape)
        got, stats = outcomes_of(pkg, dec, dec.stats)
        what = f"{case.name}, lanes {shape}"
        assert _kinds(got) == kinds, (what, _kinds(got), kinds)
        assert got == want, f"{what}: pfv_gop_decoder with the payloads read on the device delivers other frames than the oracle's"
        route = {k: stats[k] for k in ROUTE}
        if case.regular:
            assert route == dict(zip(ROUTE, (3, 0, 0, 0))), f"{what}: a regular payload left the device: {route}"
        else:
            assert route["left_irregular"] >= 1 and route["left_unsettled"] == 0, f"{what} ({case.why}): not marked by k_entd_emit: {route}"
        routes.append(route)
    if not others:
        return routes[0]
    dec = pkg.GopDecoder(data, ctx, max_gops=2, max_gop_frames=4, threads=1, entropy="host")
    got, stats = outcomes_of(pkg, dec, dec.stats)
    assert got == want, f"{case.name}: pfv_gop_decoder (host parser)"
    assert stats["packets_read_on_device"] == 0
    dec = pkg.Decoder(data, ctx, lookahead=0, entropy="device")
    got, counts = outcomes_of(pkg, dec, dec.entropy_counts)
    assert got == want, f"{case.name}: pfv_decoder with the payloads read on the device"
    if case.regular:
        assert counts == {"packets_read_on_device": 3, "packets_left_to_host_parser": 0}, (case.name, counts)
    else:
        assert counts["packets_read_on_device"] <= 2, (case.name, counts)
    # two copies through pfv_batch_decoder, to its first error
    bd = pkg.BatchDecoder([data, data], ctx, threads=1, entropy="device")
    try:
        for k, x in enumerate(want):
            if x[0] == "eof":
                break
            if x[0] == "err":
                try:
                    bd.advance_frames()
                except pkg.PfvError as e:
                    assert e.code == x[1], (case.name, k, e.code, x[1])
                    break
                raise AssertionError(f"{case.name}: pfv_batch_decoder accepts packet {k}, the oracle reports {x[1]}")
            fr = bd.advance_frames()
            if x[0] == "none":
                assert fr is False, (case.name, k)
                break
            assert fr is not False and fr is not None and fr[0].tobytes() == x[1] and fr[1].tobytes() == x[1], f"{case.name}: pfv_batch_decoder, step {k}"
        bcounts = bd.entropy_counts()
    finally:
        bd.close()
    if case.regular:
        assert bcounts == {"packets_read_on_device": 6, "packets_left_to_host_parser": 0}, (case.name, bcounts)
    return routes[0]


def check_cases(pkg, ctx, oracle, w=64, h=48, large=False, only=None, **kw):
    """every case of build_cases at w x h; returns {name: route}"""
    tb = int(pkg._lib.load().pfv_total_blocks(w, h))
    around = frame_packets(tb, (w + 15) // 16 + 1)
    out = {}
    for case in build_cases(tb, large=large):
        if only is None or only(case):
            out[case.name] = check_case(pkg, ctx, oracle, w, h, case, around, **kw)
    return out


N_REGULAR, N_IRREGULAR = 25, 24


def check_regular(pkg, ctx, oracle):
    out = check_cases(pkg, ctx, oracle, only=lambda c: c.regular)
    assert len(out) == N_REGULAR, sorted(out)
    return out


def check_irregular(pkg, ctx, oracle):
    out = check_cases(pkg, ctx, oracle, only=lambda c: not c.regular)
    assert len(out) == N_IRREGULAR, sorted(out)
    return out


def check_large(pkg, ctx, oracle, w=320, h=240):
    """noise-like run lists at 320 x 240: an i-frame and a p-frame payload of more than 240 x 256 bits each, so that a seam between two
    workgroups of k_entd_sync / k_entd_emit lies inside them at the default lane size too"""
    out = check_cases(pkg, ctx, oracle, w, h, large=True, others=False)
    assert sorted(out) == ["large_i", "large_p"]
    return out
