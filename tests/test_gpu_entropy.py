"""The device entropy stage and the device entropy decoder against the numpy restatement of the entropy layer
(oracle/pfv_oracle_entropy_np.py) and the C oracle, on an MI355X: the table + code builder over a million histograms, whole 4K and 8K
frames whose largest bins wrap x * 255 in i32, one 4K noise frame end to end, and streams coded with tables whose codes run deep
past the decoder's 12-bit lookup (ed_long_code)."""

import numpy as np
import pytest

import entropy_recompute as er
import stream_cases as sc
from entropy_recompute import ent
from oracle_bind import OracleStreamEncoder
from test_entropy_restatement import _oracle, _p, random_histograms, selfcheck_huffman

pytestmark = pytest.mark.gpu


def coefficients_with_bins(nb, bin0, bin2=None):
    """[nb, 256] i-frame coefficients whose run histogram has bin 0 == bin0 (the largest) and, when given, bin 2 == bin2: dense
    macroblocks, one partial one (k leading values, then zeros: k + fillers + 1 in bin 0) and all-zero ones (18 each).  Every value
    has no zero in front of it (bin 0); +-1 count in bin 2, +-2 in bin 3 (all +-1 when bin2 is None)."""
    def g(k):
        return k + ((255 - k) // 15 + 1 if k < 256 else 0)
    t = bin0 - 18 * (nb - 1)
    dense = (t - 18) // 238
    r = t - 238 * dense
    assert 0 <= dense < nb and 18 <= r <= 256
    k_part = next(k for k in range(257) if g(k) == r)
    mask = np.zeros((nb, 256), bool)
    mask[:dense] = True
    mask[dense, :k_part] = True
    n_values = int(mask.sum())
    vals = np.ones(n_values, np.int16)
    if bin2 is not None:
        assert bin2 <= n_values
        vals[bin2:] = 2
    vals[1::2] *= -1
    coef = np.zeros((nb, 256), np.int16)
    coef[mask] = vals
    return coef


def test_gpu_selfcheck_huffman_million_histograms(gpu_ctx, graft, pkg):
    """ent_build_codes_wave on the device: tables == the restatement's formula, codes == the host builder (which the CPU suite holds
    to the restatement), over the crafted histograms and 10^6 seeded random ones"""
    v = er.load()
    got = selfcheck_huffman(gpu_ctx._lib, gpu_ctx.handle, v["hist"], on_device=1)
    for name, g in zip(er.OUTPUTS, got):
        bad = np.nonzero((g != v[name]).any(axis=1))[0]
        assert bad.size == 0, f"{name}: {[str(v['hist_names'][i]) for i in bad]}"
    hists = random_histograms(1_000_000, 12)
    t, cv, cl = selfcheck_huffman(gpu_ctx._lib, gpu_ctx.handle, hists, on_device=1)
    want_t = ent.normalise(hists)
    bad = np.nonzero((t != want_t).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} tables differ; first {hists[bad[0]].tolist()}: {t[bad[0]].tolist()} vs {want_t[bad[0]].tolist()}"
    ht, hv, hl = selfcheck_huffman(gpu_ctx._lib, None, hists, on_device=0)
    assert np.array_equal(ht, want_t)
    bad = np.nonzero((cv != hv).any(axis=1) | (cl != hl).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} code sets differ; first table {t[bad[0]].tolist()}"
    assert ((hists > 8_421_504).any(axis=1)).sum() > 100_000


@pytest.mark.parametrize("w,h,bin0,bin2,byte0,byte2", [
    (3840, 2160, 8_421_505, None, 1, None),
    (3840, 2160, 12_311_503, None, 1, None),
    (7680, 4320, 20_000_000, 17_000_000, 40, 2),
])
def test_gpu_device_entropy_stage_at_the_wrap(gpu_ctx, pkg, oracle, w, h, bin0, bin2, byte0, byte2):
    """EncoderSession.pack_iframe_dev on whole frames whose bin 0 wraps x * 255: payload == the fixed oracle's, table == the worked
    rows of oracle/ENTROPY_WIDTHS.md, and the default payload capacity holds it"""
    ctx = gpu_ctx
    L = _oracle(oracle)
    enc = pkg.EncoderSession(ctx, w, h, 5, 1)
    enc.enable_entropy()
    nb = enc.total_blocks
    coef = coefficients_with_bins(nb, bin0, bin2)
    hist = ent.histogram(coef)
    assert hist[0] == bin0 and hist.max() == bin0 and (bin2 is None or hist[2] == bin2)
    table = ent.normalise(hist)
    assert table[0] == byte0 and (byte2 is None or table[2] == byte2)
    d_coef = ctx.alloc(nb * 512)
    ctx.upload(d_coef, coef)
    enc.pack_iframe_dev(d_coef)
    n = int(enc.payload_sizes()[0])
    cap = int(ctx._lib.pfv_payload_worst_case(w, h))
    assert 19 < n <= cap
    ref = np.zeros(cap + 64, np.uint8)
    no = L.pfvo_serialize_iframe(_p(coef), nb, _p(ref), ref.size)
    assert no == n
    got = np.frombuffer(enc.payload(0, n), np.uint8)
    assert got[:16].tolist() == table.tolist()
    if not np.array_equal(got, ref[:n]):
        raise AssertionError(f"payload differs at byte {int(np.flatnonzero(got != ref[:n])[0])} of {n}")


def _decode_all(pkg, ctx, oracle, data, n_packets):
    """GopDecoder and BatchDecoder with the device entropy reader forced: every frame == the oracle decoder's; their counters"""
    want = sc._outcomes_oracle(oracle, data)
    assert [x[0] for x in want].count("frame") == n_packets
    dec = pkg.GopDecoder(data, ctx, max_gops=2, max_gop_frames=4, threads=2, entropy="device")
    got = []
    while True:
        fr = []
        more = dec.advance_frame(lambda f: fr.append(f.packed().tobytes()))
        got.append(("frame", fr[0]) if fr else ("none",))
        if not more:
            got.append(("eof",))
            break
    stats = dec.stats()
    dec.close()
    assert got == want, "pfv_gop_decoder (device entropy): frames differ from the oracle's"
    frames = [x[1] for x in want if x[0] == "frame"]
    bdec = pkg.BatchDecoder([data], ctx, threads=2, entropy="device")
    k = 0
    while True:
        fr = bdec.advance_frames()
        if fr is False:
            break
        assert fr[0].tobytes() == frames[k], f"pfv_batch_decoder: frame {k} differs from the oracle's"
        k += 1
    counts = bdec.entropy_counts()
    bdec.close()
    assert k == n_packets
    return stats, counts


def test_gpu_end_to_end_4k_noise_quality0(gpu_ctx, pkg, oracle):
    """one 3840x2160 uniform-noise i-frame at quality 0: both encoder forms write the fixed oracle's bytes; the packet's table is the
    restatement's from the oracle's coefficients (bin 0 wraps: byte 0 == 1); both decoders read it on the device"""
    ctx = gpu_ctx
    w, h = 3840, 2160
    rng = np.random.default_rng(4096)
    frame = rng.integers(0, 256, w * h * 3 // 2).astype(np.uint8)
    coef = oracle.encoder(w, h, 0, threads=8).encode_iframe(frame)
    hist = ent.histogram(coef)
    table = ent.normalise(hist)
    assert hist[0] > 8_421_504 and table[0] == 1, (hist.tolist(), table.tolist())
    oenc = OracleStreamEncoder(oracle, w, h, 30, 0, threads=8)
    oenc.encode_iframe(frame)
    oenc.finish()
    want = oenc.bytes()
    head = 20 + 4 * 128
    assert want[head] == 1 and list(want[head + 5:head + 21]) == table.tolist()
    for dev in (True, False):
        data, _ = sc.encode_pattern(pkg, ctx, oracle, w, h, 0, "I", lambda buf: pkg.Encoder(buf, w, h, 30, 0, ctx, device_entropy=dev),
                                    lambda t: frame, with_oracle=False)
        assert data == want, f"Encoder(device_entropy={dev}): the stream differs from the oracle's"
    stats, counts = _decode_all(pkg, ctx, oracle, want, 1)
    assert stats["packets_read_on_device"] == 1 and counts["packets_read_on_device"] == 1, (stats, counts)


def _long_code_tables():
    """(name, 16-byte table, deepest code wanted): tables whose most frequent symbol has a long code, Fibonacci-like weights that
    drive codes as deep as 16 weights <= 255 allow, two-symbol tables"""
    fib = [1, 1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 255, 255]
    return [
        ("one_then_255s", [1] + [255] * 15, 4),
        ("fib", fib, 13),
        ("fib_reversed", fib[::-1], 13),
        ("fib_interleaved", [fib[(k * 7) % 16] for k in range(16)], 13),
        ("two_symbols", [255, 0, 1] + [0] * 13, 1),
        ("two_symbols_equal", [7, 0, 7] + [0] * 13, 1),
    ]


def _stream(pkg, w, h, packets):
    tabs = pkg.qtables_from_quality(5)
    data = ent.stream_header(w, h, 30, np.stack([np.asarray(tabs[k]) for k in range(4)]))
    return data + b"".join(ent.packet(t, p) for t, p in packets) + ent.packet(ent.PKT_EOF)


@pytest.mark.parametrize("name,table,depth", _long_code_tables(), ids=[t[0] for t in _long_code_tables()])
def test_gpu_long_code_tables_decode_on_device(gpu_ctx, pkg, oracle, name, table, depth):
    """streams coded (by the restatement's table override) with deep or two-symbol trees, decoded with the device entropy reader
    forced: frames == the oracle decoder's, and every packet was read on the device (none left to the host parser)"""
    ctx = gpu_ctx
    w, h = 320, 240
    nb = int(pkg._lib.load().pfv_total_blocks(w, h))
    _, lens = ent.tree_codes(table)
    assert max(lens) >= depth
    rng = np.random.default_rng(sum(table))
    present = [k for k in range(16) if table[k]]
    packets = []
    for i, kind in enumerate("IPIP"):
        if present == [0, 2]:                                      # every value +-1 with no zero in front: (0, 2) pairs only
            coef = rng.choice(np.array([-1, 1], np.int16), (nb, 256))
        else:
            coef = np.zeros((nb, 256), np.int16)
            dens = rng.random((nb, 1)) * 0.3
            sizes = rng.integers(1, 15, (nb, 256))
            vals = rng.integers(1 << (sizes - 1), 1 << sizes) * rng.choice([-1, 1], (nb, 256))
            coef[:] = np.where(rng.random((nb, 256)) < dens, vals, 0)
            coef[rng.integers(0, nb, 4)] = 0
        if kind == "I":
            packets.append((ent.PKT_IFRAME, ent.iframe_payload(coef, table=table)))
        else:
            mv = np.zeros((nb, 2), np.int8)                        # (a vector may point off the plane: the decoders reject it)
            has = (rng.random(nb) < 0.7).astype(np.uint8)
            packets.append((ent.PKT_PFRAME, ent.pframe_payload(mv, has, coef, table=table)))
    data = _stream(pkg, w, h, packets)
    stats, counts = _decode_all(pkg, ctx, oracle, data, len(packets))
    assert stats["packets_read_on_device"] == len(packets) and stats["packets_left_to_host_parser"] == 0, (name, stats)
    assert counts["packets_read_on_device"] == len(packets) and counts["packets_left_to_host_parser"] == 0, (name, counts)
