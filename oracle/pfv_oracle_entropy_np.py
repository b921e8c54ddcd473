"""numpy restatement of the pfv-rs entropy / container layer -- the SECOND oracle of RLE, the Huffman table and tree, the
LSB-first bit packing, the i- and p-frame payloads and the stream container.

TEST INFRASTRUCTURE ONLY, like oracle/pfv_oracle_np.py.  It is written from the reference sources alone (paths relative to the
reference root) so that the C oracle (oracle/pfv_oracle_entropy.c) and the product's three implementations -- the host
serialisers, the device entropy stage and the device entropy decoder -- are checked against a reading that shares nothing with
them.  The committed vectors of tests/golden/entropy_vectors.npz come from here (tests/golden/make_entropy_vectors.py), cross-
checked with the C oracle before they are written.

Integer widths follow a release build of the reference (no overflow checks): oracle/ENTROPY_WIDTHS.md lists every expression.
The bit I/O lives in the bitstream-io crate (LittleEndian): write(n, v) appends the low n bits of v, least significant first;
write_signed(n, v) appends the n-bit two's complement of v the same way; byte_align pads the last byte with zero bits.
"""
from __future__ import annotations

import numpy as np

MAGIC = b"PFVIDEO\0"          # src/common.rs:1
VERSION = 211                 # src/common.rs:2
PKT_EOF, PKT_IFRAME, PKT_PFRAME = 0, 1, 2     # src/enc.rs:221-235, :323-327, :474-478

# Mutation switches, one per rule the entropy layer can get wrong.  The defaults ARE the reference's rules; the only user of any
# other value is tests/test_mutation_sensitivity.py, which flips one at a time and checks that the committed entropy vectors
# notice (or, for the three rules that cannot be observed, that they do not).
DEFAULT_RULES = {
    "sort": "stable",             # src/huffman.rs:81     sort_by on descending freq is stable: ties keep symbol order ("ties_desc")
    "insert": "lt",               # src/huffman.rs:61-69  new node goes before the first strictly smaller entry ("le": first <=)
    "children": "left_last",      # src/huffman.rs:84-88  left = the last entry popped, right = the one before it ("swapped")
    "bit_order": "lsb",           # src/huffman.rs:30-32, :204-217  first branch in bit 0 of the code ("msb": first branch on top)
    "filler": "gt15",             # src/rle.rs:18, :31    (15, 0) fillers while run > 15 ("ge15")
    "trailing": "emit",           # src/rle.rs:36-38      a block's trailing zero run is its own symbol pair ("drop")
    "min1": "clamp",              # src/rle.rs:57         .max(1): a present symbol never gets table byte 0 ("none")
    "table_i32": "wrap",          # src/rle.rs:57         x * 255 is an i32 product and wraps past 8 421 504 ("wide")
    "signed_field": "twos",       # src/enc.rs:312, :463    write_signed: two's complement ("sign_mag")
    "one_symbol": "zero_len",     # src/huffman.rs:99-102, :205-208  a one-leaf tree gives its symbol a 0-bit code ("one_bit")
    "pair_order": "zeroes_first", # src/enc.rs:306-311    num_zeroes code, then coeff_size code ("size_first")
    "pf_header": "mvec_first",    # src/enc.rs:414-422    has_mvec bit, has_coef bit, then the vector ("coded_first")
    # unobservable (tests/test_mutation_sensitivity.py ENTROPY_INVISIBLE asserts they change nothing):
    "u8_cast": "wrap",            # src/rle.rs:57         `as u8` of the quotient ("saturate")
    "code_shift": "u32",          # src/huffman.rs:31     (bit as u32) << len in u32 ("wide")
    "freq": "u32",                # src/huffman.rs:86     Node.freq sums in u32 ("wide")
}
RULES = dict(DEFAULT_RULES)

_M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ src/rle.rs
def coeff_size(v: int) -> int:
    """src/rle.rs:23-24: bit length of |v| (as u16) plus one; 0 is never asked for"""
    return (abs(int(v)) & 0xFFFF).bit_length() + 1


def rle_encode(data) -> list:
    """src/rle.rs:9-39 over one macroblock's coefficients: a list of (num_zeroes, coeff_size, coeff)"""
    out = []
    run = 0
    limit = 15 if RULES["filler"] == "gt15" else 14          # `run > 15` vs `run >= 15`
    for v in np.asarray(data).tolist():
        if v == 0:
            run += 1
            continue
        while run > limit:
            out.append((15, 0, 0))
            run -= 15
        out.append((run, coeff_size(v), v))
        run = 0
    while run > limit:
        out.append((15, 0, 0))
        run -= 15
    if run > 0 and RULES["trailing"] == "emit":
        out.append((run, 0, 0))
    return out


def update_table(table: list, seq: list) -> None:
    """src/rle.rs:41-47: both fields of every pair count; a size of 16 or more would index past the 16 bins (a panic)"""
    for z, s, _ in seq:
        if s > 15:
            raise ValueError(f"coefficient needs {s} size bits: the reference indexes its histogram out of range")
        table[z] += 1
        table[s] += 1


def histogram(coef, has=None) -> np.ndarray:
    """the histogram that rle_encode + update_table build over a frame's coded macroblocks, array-at-a-time (for frames far
    too large for the per-symbol restatement above; the tests hold the two to each other on small frames)"""
    c = np.asarray(coef, np.int16).reshape(-1, 256)
    if has is not None:
        c = c[np.asarray(has).astype(bool)]
    hist = np.zeros(16, np.int64)
    if c.shape[0] == 0:
        return hist
    nzb, nzi = np.nonzero(c)
    mag = np.abs(c[nzb, nzi].astype(np.int64)) & 0xFFFF
    size = np.zeros(mag.shape, np.int64)
    m = mag.copy()
    while np.any(m):
        size += m > 0
        m >>= 1
    size += 1
    if np.any(size > 15):
        raise ValueError("coefficient needs 16 size bits")
    # run in front of every non-zero value: distance to the previous non-zero value of the same block (or the block start)
    prev = np.full(nzi.shape, -1, np.int64)
    same = np.zeros(nzi.shape, bool)
    same[1:] = nzb[1:] == nzb[:-1]
    prev[1:][same[1:]] = nzi[:-1][same[1:]]
    run = nzi - prev - 1
    # the run after the last non-zero value of every block (a block without any is one run of 256)
    last = np.full(c.shape[0], -1, np.int64)
    last[nzb] = nzi                                         # nzi ascends within a block: the last write wins
    tail = 255 - last
    per = 15 if RULES["filler"] == "gt15" else 14

    def fillers(r):
        return np.where(r > per, (r - per + 14) // 15, 0)

    n_fill = int(fillers(run).sum() + fillers(tail).sum())
    hist[15] += n_fill
    hist[0] += n_fill
    np.add.at(hist, run - 15 * fillers(run), 1)
    np.add.at(hist, size, 1)
    rest = tail - 15 * fillers(tail)
    if RULES["trailing"] == "emit":
        np.add.at(hist, rest[rest > 0], 1)
        hist[0] += int((rest > 0).sum())
    return hist


def normalise(hist) -> np.ndarray:
    """src/rle.rs:49-63 for an array of histograms (..., 16) of i32 bins >= 0: the u8 table.  In a release build x * 255 is an
    i32 product that wraps; `/` is i32 division truncating toward zero; .max(1); `as u8`."""
    h = np.asarray(hist, np.int64)
    mx = h.max(axis=-1, keepdims=True)
    prod = h * 255
    if RULES["table_i32"] == "wrap":
        prod = ((prod + (1 << 31)) & _M32) - (1 << 31)
    q = np.sign(prod) * (np.abs(prod) // np.maximum(mx, 1))      # truncating division (the divisor is positive)
    if RULES["min1"] == "clamp":
        q = np.maximum(q, 1)
    q = (q & 0xFF) if RULES["u8_cast"] == "wrap" else np.clip(q, 0, 255)
    return np.where(h > 0, q, 0).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ src/huffman.rs
class _Node:
    __slots__ = ("freq", "ch", "left", "right")

    def __init__(self, freq, ch=None, left=None, right=None):
        self.freq, self.ch, self.left, self.right = freq, ch, left, right


def tree_codes(table):
    """HuffmanTree::from_table (src/huffman.rs:71-119) + assign_codes (:204-217): (val[16], len[16]) per symbol; an absent
    symbol has (0, 0)"""
    table = [int(t) for t in np.asarray(table).reshape(16)]
    p = [_Node(fr, ch) for ch, fr in enumerate(table) if fr > 0]
    if RULES["sort"] == "stable":
        p.sort(key=lambda n: -n.freq)
    else:
        p.sort(key=lambda n: (-n.freq, -n.ch))
    while len(p) > 1:
        a = p.pop()
        b = p.pop()
        f = a.freq + b.freq
        if RULES["freq"] == "u32":
            f &= _M32
        c = _Node(f, None, a, b) if RULES["children"] == "left_last" else _Node(f, None, b, a)
        pos = len(p)
        for i, x in enumerate(p):
            if (c.freq > x.freq) if RULES["insert"] == "lt" else (c.freq >= x.freq):
                pos = i
                break
        p.insert(pos, c)
    vals, lens = [0] * 16, [0] * 16
    if not p:
        return vals, lens
    root = p[0]
    if root.ch is not None and RULES["one_symbol"] == "one_bit":
        vals[root.ch], lens[root.ch] = 0, 1
        return vals, lens

    stack = [(root, 0, 0)]
    while stack:
        n, v, ln = stack.pop()
        if n.ch is not None:
            vals[n.ch], lens[n.ch] = v, ln
            continue
        for node, bit in ((n.right, 1), (n.left, 0)):          # Code::append (:30-32): the new bit goes above the ones before
            if node is not None:
                nv = v | (bit << ln)
                stack.append((node, nv & _M32 if RULES["code_shift"] == "u32" else nv, ln + 1))
    if RULES["bit_order"] == "msb":
        vals = [int(format(v, f"0{ln}b")[::-1], 2) if ln else 0 for v, ln in zip(vals, lens)]
    return vals, lens


def huffman_from_histogram(hist):
    """rle_create_huffman (src/rle.rs:49-66): (table, code values, code lengths)"""
    t = normalise(np.asarray(hist, np.int64).reshape(16))
    v, ln = tree_codes(t)
    return t, np.array(v, np.uint32), np.array(ln, np.uint8)


# ------------------------------------------------------------------------------------------------ bit writer
class BitWriter:
    """bitstream-io BitWriter<_, LittleEndian>: fields are collected, then packed least significant bit first"""

    def __init__(self):
        self.vals, self.lens = [], []

    def write(self, n: int, v: int) -> None:
        if n:
            self.vals.append(int(v) & ((1 << n) - 1))
            self.lens.append(n)

    def write_signed(self, n: int, v: int) -> None:
        if RULES["signed_field"] == "twos":
            self.write(n, int(v) & ((1 << n) - 1))
        else:
            self.write(n, (abs(int(v)) & ((1 << (n - 1)) - 1)) | ((1 << (n - 1)) if v < 0 else 0))

    def bytes(self) -> bytes:
        """byte_align + the finished buffer"""
        if not self.vals:
            return b""
        v = np.array(self.vals, np.uint64)
        ln = np.array(self.lens, np.int64)
        k = np.arange(int(ln.max()), dtype=np.uint64)
        bits = ((v[:, None] >> k[None, :]) & np.uint64(1)).astype(np.uint8)
        bits = bits[np.arange(k.size)[None, :] < ln[:, None]]      # row-major: field after field, low bit first
        return np.packbits(bits, bitorder="little").tobytes()


# ------------------------------------------------------------------------------------------------ src/enc.rs payloads
def _runs(coef, has):
    c = np.asarray(coef, np.int16).reshape(-1, 256)
    return [rle_encode(c[b]) if has is None or has[b] else None for b in range(c.shape[0])]


def _tree_for(blocks, table):
    hist = [0] * 16
    for seq in blocks:
        if seq is not None:
            update_table(hist, seq)
    if table is None:
        table = normalise(np.array(hist, np.int64))
    else:
        table = np.asarray(table, np.uint8).reshape(16)
        used = {s for seq in blocks if seq for z, sz, _ in seq for s in (z, sz)}
        if any(table[s] == 0 for s in used):
            raise ValueError("the table override leaves a symbol the payload needs without a code")
    vals, lens = tree_codes(table)
    return table, vals, lens


def _emit_blocks(w: BitWriter, blocks, vals, lens) -> None:
    """src/enc.rs:301-318 (i-frame), :454-466 (p-frame)"""
    for seq in blocks:
        if seq is None:
            continue
        for z, s, c in seq:
            first, second = (z, s) if RULES["pair_order"] == "zeroes_first" else (s, z)
            w.write(lens[first], vals[first])
            w.write(lens[second], vals[second])
            if s > 0:
                w.write_signed(s, c)


def iframe_payload(coef, table=None) -> bytes:
    """write_iframe_packet's payload (src/enc.rs:237-320): coef[total_blocks][256] (Y, then U, then V macroblocks, four
    subblocks of 64 each).  table: an optional 16-byte table to code with instead of the normalised histogram's."""
    blocks = _runs(coef, None)
    table, vals, lens = _tree_for(blocks, table)
    w = BitWriter()
    for t in table:
        w.write(8, int(t))                                          # :289-292
    for q in (0, 1, 1):
        w.write(8, q)                                               # :296-298
    _emit_blocks(w, blocks, vals, lens)
    return w.bytes()


def pframe_payload(mv, has, coef, table=None) -> bytes:
    """write_pframe_packet's payload (src/enc.rs:332-470): mv[total_blocks][2], has[total_blocks], coef[total_blocks][256]"""
    mv = np.asarray(mv, np.int64).reshape(-1, 2)
    has = np.asarray(has).astype(bool)
    blocks = _runs(coef, has)
    table, vals, lens = _tree_for(blocks, table)
    w = BitWriter()
    for t in table:
        w.write(8, int(t))                                          # :402-405
    for q in (2, 3, 3):
        w.write(8, q)                                               # :409-411
    for b in range(mv.shape[0]):                                    # block headers, every block (:414-451)
        moving = bool(mv[b, 0] != 0 or mv[b, 1] != 0)
        flags = (moving, has[b]) if RULES["pf_header"] == "mvec_first" else (has[b], moving)
        w.write(1, int(flags[0]))
        w.write(1, int(flags[1]))
        if moving:
            w.write_signed(7, int(mv[b, 0]))
            w.write_signed(7, int(mv[b, 1]))
    _emit_blocks(w, blocks, vals, lens)
    return w.bytes()


# ------------------------------------------------------------------------------------------------ src/enc.rs container
def _le(v: int, n: int) -> bytes:
    return (int(v) & ((1 << (8 * n)) - 1)).to_bytes(n, "little")


def stream_header(width: int, height: int, framerate: int, qtables) -> bytes:
    """write_header (src/enc.rs:190-219): magic, u32 version, u16 width / height / framerate (`as u16`), u16 table count 4, then
    intra luma, intra chroma, inter luma, inter chroma, 64 u16 each"""
    q = np.asarray(qtables, np.int64).reshape(4, 64)
    return MAGIC + _le(VERSION, 4) + _le(width, 2) + _le(height, 2) + _le(framerate, 2) + _le(4, 2) + b"".join(_le(v, 2) for v in q.reshape(-1))


def packet(kind: int, payload: bytes = b"") -> bytes:
    """u8 packet type + u32 payload length + payload (src/enc.rs:221-235, :323-327, :474-478); EOF and drop frames are empty"""
    return _le(kind, 1) + _le(len(payload), 4) + bytes(payload)
