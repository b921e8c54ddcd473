"""Why the decoders may run the inverse transform in f32 below pfv_dec_float_guard() (csrc/pfv_kernels.hip: kDecFloatGuard): with every
dequantised value |v| <= T, every number of the two passes is an integer below 2^23 (or an exact multiple of 1/4 of one), which f32 holds
exactly, so the float butterflies with explicit truncation give the integer oracle's numbers bit for bit.  numpy float32 arithmetic stands
in for the device here; the emulator and GPU tests (tests/decfloat_cases.py) run the kernels themselves."""
import numpy as np

import pfv_oracle_np as onp


def _matrix(signed):
    M = np.zeros((8, 8))
    for k in range(8):
        e = np.zeros(8, dtype=np.int64)
        e[k] = 1 << 20                      # large enough that no division of the 1-D transform truncates
        col = onp.idct(e[None])[0] / float(1 << 20)
        M[:, k] = col if signed else np.abs(col)
    return M


I_ABS, I_SIGNED = _matrix(False), _matrix(True)
R = I_ABS.sum(1).max()
SLACK = 16                                  # what the truncating divisions of one pass can add to an output, generously (at most 5 quotients, < 1 each)


def _guard(pkg, emu_ctx):
    return int(emu_ctx._lib.pfv_dec_float_guard())


F = np.float32


def fidct8_f32(v):
    """csrc/pfv_kernels.hip: fidct8 on the LAST axis, in numpy float32 with explicit truncation toward zero"""
    assert v.dtype == np.float32
    c0, d4, c2, d6, c1, d5, c3, d7 = [v[..., k] for k in range(8)]
    half, quarter = F(0.5), F(0.25)
    c5, c7 = d5 + d6, d5 - d6
    b4, b5, b6, b7 = d4 + c5, d4 - c5, d7 + c7, d7 - c7
    b0, b1 = c0 + c1, c0 - c1
    c2h = np.trunc(c2 * half); c2q = np.trunc(c2h * half); c3h = np.trunc(c3 * half); c3q = np.trunc(c3h * half)
    b4q = np.trunc(b4 * quarter); b4s = np.trunc(b4q * quarter); b5q = np.trunc(b5 * quarter); b5s = np.trunc(b5q * quarter)
    b6q = np.trunc(b6 * quarter); b6s = np.trunc(b6q * quarter); b7q = np.trunc(b7 * quarter); b7s = np.trunc(b7q * quarter)
    b2, b3 = c2 + c2q + c3h, c2h - c3 - c3q
    a4 = b7q + b4 + b4q - b4s
    a7 = b4q - b7 - b7q + b7s
    a5 = b5 - b6 + b6q + b6s
    a6 = b6 + b5 - b5q - b5s
    a0, a1, a2, a3 = b0 + b2, b1 + b3, b1 - b3, b0 - b2
    out = np.stack([a0 + a4, a1 + a5, a2 + a6, a3 + a7, a3 - a7, a2 - a6, a1 - a5, a0 - a4], axis=-1)
    assert out.dtype == np.float32
    return out


def idct2d_f32(m):
    """columns, then rows (src/common.rs:315-316), then t = floor(x / 256): what the float path hands to the reconstruction"""
    x = fidct8_f32(np.swapaxes(fidct8_f32(np.swapaxes(m.astype(np.float32), -1, -2)), -1, -2))
    return x, np.floor(x * F(1.0 / 256.0))


def _same(m):
    want = onp.idct2d(m.astype(np.int64))
    got, t = idct2d_f32(m)
    return np.array_equal(got.astype(np.int64), want) and np.array_equal(t.astype(np.int64), want >> 8)


def test_guard_is_the_largest_bound_of_the_inequality(pkg, emu_ctx):
    T = _guard(pkg, emu_ctx)
    assert R == 121 / 16
    assert R * (R * T + SLACK) + SLACK < 2 ** 23
    assert R * (R * (T + 1) + SLACK) + SLACK >= 2 ** 23


def test_slack_covers_the_truncations(pkg, emu_ctx):
    """|idct(x)| <= R max|x| + SLACK, measured: the largest excess of the truncating transform over the linear one"""
    T = _guard(pkg, emu_ctx)
    rng = np.random.default_rng(1)
    x = rng.integers(-T, T + 1, (200000, 8))
    exact = x @ I_SIGNED.T
    assert np.abs(onp.idct(x) - exact).max() < 5 < SLACK


def test_float32_equals_the_oracle_up_to_the_guard(pkg, emu_ctx):
    T = _guard(pkg, emu_ctx)
    rng = np.random.default_rng(2)
    assert _same(rng.integers(-T, T + 1, (100000, 8, 8)))
    assert _same(rng.integers(-300, 301, (20000, 8, 8)))                    # small values: the truncations matter most
    assert _same(rng.choice(np.array([-T, T]), (20000, 8, 8)))              # |v| = T everywhere, random signs
    # the sign patterns that maximise (and minimise) each of the 64 outputs, all 64 inputs at +-T: the proof's worst case
    s = np.sign(I_SIGNED)
    pats = np.stack([np.outer(s[r], s[c]) for r in range(8) for c in range(8)]).astype(np.int64) * T
    pats = np.concatenate([pats, -pats])
    assert _same(pats)
    peak = np.abs(onp.idct2d(pats)).max()
    assert R * R * T - R * SLACK - SLACK <= peak < 2 ** 23                  # they do reach the bound's neighbourhood


def test_float32_differs_above_the_guard(pkg, emu_ctx):
    """why the guard exists: one subblock not far above the bound whose float32 evaluation is not the integer one"""
    T = _guard(pkg, emu_ctx)
    s = np.sign(I_SIGNED)
    m = (np.outer(s[0], s[0]).astype(np.int64) * (4 * T + 1))[None]       # |v| = 4 T + 1: output (0, 0) needs 26 bits
    want = onp.idct2d(m)
    got, _ = idct2d_f32(m)
    assert np.abs(want).max() >= 2 ** 24
    assert not np.array_equal(got.astype(np.int64), want)
