"""The entropy layer against its second reading (oracle/pfv_oracle_entropy_np.py), CPU only.

The numpy restatement reproduces the committed entropy vectors and the reference's own entropy vector; it, the C oracle and the
product's host serialisers agree byte for byte on random payloads; the product's two table + code builders (the host
serialisers' normalise_histogram + HuffmanTree, and the device entropy stage's ent_build_codes_wave on the CPU emulator) equal
the restatement through pfv_selfcheck_huffman (csrc/pfv_selfcheck.h), at histograms whose bins wrap x * 255 in i32; and the host
serialiser writes the right table for whole frames whose most frequent bin lands exactly on the wrap points."""
import ctypes

import numpy as np
import pytest

import entropy_recompute as er
from entropy_recompute import ent

P = ctypes.c_void_p


def _p(a):
    return a.ctypes.data_as(P)


def _oracle(oracle):
    L = oracle.L
    L.pfvo_serialize_iframe.restype = L.pfvo_serialize_pframe.restype = ctypes.c_size_t
    L.pfvo_serialize_iframe.argtypes = [P, ctypes.c_int, P, ctypes.c_size_t]
    L.pfvo_serialize_pframe.argtypes = [P, P, P, ctypes.c_int, P, ctypes.c_size_t]
    L.pfvo_huffman_from_histogram.restype = None
    L.pfvo_huffman_from_histogram.argtypes = [P, ctypes.c_int, P, P, P]
    return L


def _product(graft, pkg):
    graft.build_hip()
    __import__("libswitch").reset(pkg)
    return pkg._lib.load()


def selfcheck_huffman(lib, handle, hists, on_device):
    """pfv_selfcheck_huffman (csrc/pfv_selfcheck.h): tables, code values, code lengths of every histogram"""
    fn = lib.pfv_selfcheck_huffman
    fn.restype = ctypes.c_int
    fn.argtypes = [P, P, ctypes.c_int, ctypes.c_int, P, P, P]
    h = np.ascontiguousarray(hists, np.int32).reshape(-1, 16)
    n = h.shape[0]
    t, v, ln = np.zeros((n, 16), np.uint8), np.zeros((n, 16), np.uint32), np.zeros((n, 16), np.uint8)
    rc = fn(handle, _p(h), n, int(on_device), _p(t), _p(v), _p(ln))
    assert rc == 0, rc
    return t, v, ln


def restated(hists):
    rows = [ent.huffman_from_histogram(h) for h in np.asarray(hists).reshape(-1, 16)]
    return tuple(np.stack([r[i] for r in rows]) for i in range(3))


def random_histograms(n, seed):
    """seeded 16-bin histograms: sparse and dense, small and large bins, ties, bins past 8 421 504 and in the window
    [16 843 010, 25 264 513] where x * 255 wraps to a positive i32"""
    rng = np.random.default_rng(seed)
    scale = rng.choice([4, 256, 65536, 8_421_504, 2**31 - 1], n)
    h = (rng.random((n, 16)) * scale[:, None]).astype(np.int64)
    h[rng.random((n, 16)) < rng.random((n, 1))] = 0                       # holes, densities 0 .. 1
    tie = rng.random(n) < 0.3                                               # copy one bin onto another
    a, b = rng.integers(0, 16, n), rng.integers(0, 16, n)
    h[tie, a[tie]] = h[tie, b[tie]]
    win = rng.random(n) < 0.15                                              # the positive-wrap window
    h[win, rng.integers(0, 16, n)[win]] = rng.integers(16_843_010, 25_264_514, int(win.sum()))
    wrap = rng.random(n) < 0.15                                             # just past the first wrap
    h[wrap, rng.integers(0, 16, n)[wrap]] = rng.integers(8_421_505, 12_500_000, int(wrap.sum()))
    return np.clip(h, 0, 2**31 - 1).astype(np.int32)


@pytest.fixture(scope="module")
def vectors():
    return er.load()


def test_restatement_reproduces_committed_vectors(vectors):
    assert ent.RULES == ent.DEFAULT_RULES
    assert er.diff(vectors, er.recompute(vectors)) == []
    assert len(vectors["hist"]) >= 30 and len(er.payload_cases(vectors)) >= 8


def test_restatement_worked_wrap_table():
    """the worked rows of oracle/ENTROPY_WIDTHS.md: (bin, largest bin) -> table byte"""
    for x, mx, want in ((8_421_504, None, 255), (8_421_505, None, 1), (12_311_503, None, 1), (20_000_000, None, 40),
                        (17_000_000, 20_000_000, 2), (4_000_000, 20_000_000, 51)):
        h = np.zeros(16, np.int64)
        h[0] = x
        h[1] = mx or 0
        assert ent.normalise(h)[0] == want, (x, mx)


def test_restatement_reference_entropy_vector():
    """src/lib.rs:98: [10,0,0,5,3,0,0,0,0,-10] as one run stream -- the bytes tests/test_entropy.py pins for the C oracle"""
    seq = ent.rle_encode(np.array([10, 0, 0, 5, 3, 0, 0, 0, 0, -10], np.int16))
    hist = [0] * 16
    ent.update_table(hist, seq)
    t, v, ln = ent.huffman_from_histogram(hist)
    w = ent.BitWriter()
    for z, s, c in seq:
        w.write(int(ln[z]), int(v[z]))
        w.write(int(ln[s]), int(v[s]))
        if s:
            w.write_signed(s, c)
    assert list(w.bytes()) == [171, 88, 141, 165, 5]
    assert t.tolist()[:6] == [255, 0, 127, 127, 255, 255]


def test_array_histogram_equals_the_run_restatement():
    rng = np.random.default_rng(7)
    for k in range(40):
        nb = int(rng.integers(1, 9))
        d = rng.random()
        coef = (rng.integers(-16383, 16384, (nb, 256)) * (rng.random((nb, 256)) < d ** 2)).astype(np.int16)
        has = rng.random(nb) < 0.7
        hist = [0] * 16
        for b in range(nb):
            if has[b]:
                ent.update_table(hist, ent.rle_encode(coef[b]))
        assert ent.histogram(coef, has).tolist() == hist


def test_random_payloads_restatement_oracle_and_product_agree(graft, pkg, oracle):
    """a few hundred seeded coefficient sets, densities 0 .. 1, i- and p-frames: three implementations, one byte string"""
    lib = _product(graft, pkg)
    L = _oracle(oracle)
    rng = np.random.default_rng(2026)
    n_cases = 0
    for k in range(300):
        nb = int(rng.integers(1, 7))
        d = [0.0, 1.0, rng.random() ** 3, rng.random()][k % 4]
        amp = int(rng.choice([1, 3, 100, 16383]))
        coef = (rng.integers(-amp, amp + 1, (nb, 256)) * (rng.random((nb, 256)) < d)).astype(np.int16)
        cap = nb * 256 * 4 + 64
        a, b = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
        if k % 2:
            mv = rng.integers(-16, 17, (nb, 2)).astype(np.int8)
            mv[rng.random(nb) < 0.4] = 0
            has = (rng.random(nb) < rng.random()).astype(np.uint8)
            want = ent.pframe_payload(mv, has, coef)
            na = lib.pfv_serialize_pframe_payload(_p(mv), _p(has), _p(coef), nb, _p(a), cap)
            no = L.pfvo_serialize_pframe(_p(mv), _p(has), _p(coef), nb, _p(b), cap)
        else:
            want = ent.iframe_payload(coef)
            na = lib.pfv_serialize_iframe_payload(_p(coef), nb, _p(a), cap)
            no = L.pfvo_serialize_iframe(_p(coef), nb, _p(b), cap)
        assert na == no == len(want), k
        assert a[:na].tobytes() == want and b[:no].tobytes() == want, k
        n_cases += 1
    assert n_cases == 300


def test_selfcheck_huffman_host_equals_restatement(graft, pkg, vectors, oracle):
    """the host serialisers' builder on every crafted histogram and 20 000 seeded random ones (the C oracle too)"""
    lib = _product(graft, pkg)
    L = _oracle(oracle)
    hists = np.concatenate([vectors["hist"], random_histograms(20_000, 11)])
    assert (hists > 8_421_504).any(axis=1).sum() > 1000
    assert ((hists >= 16_843_010) & (hists <= 25_264_513)).any(axis=1).sum() > 1000
    want = restated(hists)
    got = selfcheck_huffman(lib, None, hists, on_device=0)
    for name, g, w in zip(er.OUTPUTS, got, want):
        bad = np.nonzero((g != w).any(axis=1))[0]
        assert bad.size == 0, f"{name}: {bad.size} histograms differ, first {hists[bad[0]].tolist()}: {g[bad[0]].tolist()} vs {w[bad[0]].tolist()}"
    n = hists.shape[0]
    t, v, ln = np.zeros((n, 16), np.uint8), np.zeros((n, 16), np.uint32), np.zeros((n, 16), np.uint8)
    h = np.ascontiguousarray(hists)
    L.pfvo_huffman_from_histogram(_p(h), n, _p(t), _p(v), _p(ln))
    assert np.array_equal(t, want[0]) and np.array_equal(v, want[1]) and np.array_equal(ln, want[2])


def test_selfcheck_huffman_device_builder_on_emulator(emu_ctx, vectors):
    """the device entropy stage's builder (ent_build_codes_wave) on the CPU emulator, every crafted histogram"""
    got = selfcheck_huffman(emu_ctx._lib, emu_ctx.handle, vectors["hist"], on_device=1)
    for name, g in zip(er.OUTPUTS, got):
        bad = np.nonzero((g != vectors[name]).any(axis=1))[0]
        assert bad.size == 0, f"{name}: {[str(vectors['hist_names'][i]) for i in bad]}"


def frame_with_bin0(target):
    """i-frame coefficients whose run histogram has bin 0 == target and bin 0 the largest: dense macroblocks of +-1 (256 x (0, 2)
    each) and at most two partial ones (k leading +-1, then a zero tail: k + fillers + 1 in bin 0)"""
    def g(k):
        return k + (255 - k) // 15 + 1
    n, rem = divmod(target, 256)
    parts = []
    if rem:
        if rem >= 18:
            parts = [next(k for k in range(256) if g(k) == rem)]
        else:
            n -= 1
            k1 = next(k for k in range(256) if g(k) == 128)
            parts = [k1, next(k for k in range(256) if g(k) == rem + 256 - 128)]
    coef = np.ones((n + len(parts), 256), np.int16)
    coef[1::2] = -1
    for i, k in enumerate(parts):
        coef[n + i, k:] = 0
    return coef


@pytest.mark.parametrize("target,byte0", [(8_421_504, 255), (8_421_505, 1), (12_311_503, 1), (20_000_000, 40)])
def test_host_serialiser_full_frame_at_the_wrap(graft, pkg, oracle, target, byte0):
    """whole frames (up to 78 k macroblocks) whose bin 0 sits on the wrap points: table bytes == restatement, payload == oracle"""
    lib = _product(graft, pkg)
    L = _oracle(oracle)
    coef = frame_with_bin0(target)
    hist = ent.histogram(coef)
    assert hist[0] == target and hist.max() == target
    table = ent.normalise(hist)
    assert table[0] == byte0
    nb = coef.shape[0]
    cap = nb * 256 + (1 << 16)
    a, b = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
    na = lib.pfv_serialize_iframe_payload(_p(coef), nb, _p(a), cap)
    no = L.pfvo_serialize_iframe(_p(coef), nb, _p(b), cap)
    assert 19 < na <= cap
    assert a[:16].tolist() == table.tolist()
    assert na == no and np.array_equal(a[:na], b[:no])
