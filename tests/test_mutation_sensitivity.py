"""Mutation sensitivity of the committed golden vectors ("missing" #1).

Nothing upstream can pin the oracle (the reference's DCT tests only print, src/lib.rs:36-94; its fixtures are Git-LFS stubs; no
Rust toolchain), so the goldens under tests/golden/ are oracle output.  What CAN be shown is that they are not blind: for
every bit-exactness trap of SURVEY.md section 8c, flipping that one rule in the numpy oracle (oracle/pfv_oracle_np.py RULES)
changes at least one committed vector -- so a HIP kernel (or a C oracle) that got the rule wrong could not pass
tests/test_gpu_parity.py::test_golden_vectors / test_trap_vectors.  Two rules are unobservable BY THEOREM, and the test
asserts exactly that, with the argument.
"""
import numpy as np
import pytest

import golden_recompute as gr
from golden_recompute import onp

# (rule, mutated value, reference lines, vectors that must notice -- a non-empty subset is required)
VISIBLE = [
    ("idct_div", "floor", "src/dct.rs:265-274 `/` truncates toward zero", ("ramp_idct", "lib_recon", "pf_rec0")),
    ("quant_div", "floor", "src/dct.rs:95 n / q truncates", ("lib_quant", "pf_c0")),
    ("quant_shift", "trunc", "src/dct.rs:92 >> 16 is an arithmetic shift (floor)", ("lib_quant", "pf_c0")),
    ("pixel_shift", "trunc", "src/common.rs:321 >> 8 is an arithmetic shift", ("lib_recon", "pf_rec0")),
    ("dec_order", "rows_cols", "src/common.rs:315-316 decode = columns then rows", ("lib_recon", "pf_rec0")),
    ("dec_table_index", "raster", "src/dct.rs:78-82 decode tables indexed by zigzag position", ("lib_recon", "pf_rec0")),
    ("i32", "wide", "release-mode i32 wrap-around (SURVEY 8c trap 11)", ("host_rec",)),
    ("u8_cast", "wrap", "src/common.rs:321 clamp before `as u8`", ("host_rec", "q10_intra_c_dec")),
    ("bounds", "exclusive", "src/common.rs:171, :182 `>` (candidate allowed at dim - 16)", ("edge_mv",)),
    ("accept", "le", "src/common.rs:189 strict `<`: first visited wins ties", ("tie_mv",)),
    ("visit", "mx_outer", "src/common.rs:168-179 my outer, mx inner", ("diag_mv",)),
    ("skip", "lt", "src/common.rs:221 `<=` against 576 q^2 (:209)", ("tie_has",)),
    ("resid_div", "floor", "src/common.rs:304 delta / 2 truncates", ("ext_out", "pf_c1")),
    ("quadrants", "tl_bl_tr_br", "src/common.rs:145-149 subblocks TL,TR,BL,BR", ("pf_c0", "pf_rec0")),
    ("pad_clear", "zero", "src/common.rs:352-356 + src/enc.rs:84-90 pad colour 128 for chroma", ("rag_c0",)),
    ("delta_clamp", "wide", "src/common.rs:321 then :100-102 a p-frame's term is a clamped byte before it is doubled (t <= 127)", ("clamp_rec",)),
]

# Unobservable by theorem -- asserted to change NOTHING, here and (for the forward transform) exhaustively in
# tests/test_oracle.py::test_forward_dct_is_exact:
INVISIBLE = [
    ("fdct_div", "floor",
     "src/dct.rs:206-214: every fdct input has 8 zero fraction bits (common.rs:291, :304), so the row pass divides multiples of 256 and "
     "the column pass multiples of 16: no division of the forward transform ever truncates"),
    ("enc_order", "cols_rows",
     "src/common.rs:294-295: for the same reason both forward passes are exact linear maps on different axes; they commute"),
    ("i16_cast", "saturate",
     "src/dct.rs:95: n = (i32) >> 16 lies in [-32768, 32767] and |n / q| <= |n| for q >= 1, so `as i16` never wraps"),
]


@pytest.fixture(scope="module")
def vectors():
    g, t = gr.load()
    return {k: g[k] for k in g.files}, {k: t[k] for k in t.files}


def _recompute(g, t):
    out = gr.recompute_hotpath(g)
    out.update(gr.recompute_traps(t))
    return out


def test_unmutated_numpy_oracle_reproduces_every_golden(vectors):
    g, t = vectors
    assert onp.RULES == onp.DEFAULT_RULES
    got = _recompute(g, t)
    want = {**g, **t}
    assert gr.diff_keys(want, got) == []
    assert len(got) >= 60


@pytest.mark.parametrize("rule,value,where,must", VISIBLE, ids=[v[0] for v in VISIBLE])
def test_golden_vectors_notice_a_flipped_rule(vectors, rule, value, where, must):
    g, t = vectors
    want = {**g, **t}
    onp.RULES[rule] = value
    try:
        changed = gr.diff_keys(want, _recompute(g, t))
    finally:
        onp.RULES.update(onp.DEFAULT_RULES)
    assert changed, f"no committed vector notices {rule}={value} ({where})"
    assert set(must) & set(changed), f"{rule}={value}: expected one of {must} to change, got {changed}"


@pytest.mark.parametrize("rule,value,why", INVISIBLE, ids=[v[0] for v in INVISIBLE])
def test_rules_unobservable_by_theorem(vectors, rule, value, why):
    g, t = vectors
    want = {**g, **t}
    onp.RULES[rule] = value
    try:
        changed = gr.diff_keys(want, _recompute(g, t))
    finally:
        onp.RULES.update(onp.DEFAULT_RULES)
    assert changed == [], f"{rule}={value} was expected to be unobservable ({why}) but changed {changed}"


def test_every_rule_is_covered():
    assert {v[0] for v in VISIBLE} | {v[0] for v in INVISIBLE} == set(onp.DEFAULT_RULES)


# ---------------------------------------------------------------------------------------------------- the entropy layer
# Same idea for the entropy / container layer: the numpy restatement (oracle/pfv_oracle_entropy_np.py RULES) with one rule
# flipped must change at least one committed vector of tests/golden/entropy_vectors.npz (names: `<output>:<histogram>` for the
# crafted histograms, `pay_<case>_bytes` for the payloads).
import entropy_recompute as er                       # noqa: E402
from entropy_recompute import ent                    # noqa: E402

ENTROPY_VISIBLE = [
    ("sort", "ties_desc", "src/huffman.rs:81 stable sort: equal frequencies keep symbol order", ("code_val:all_16_equal", "code_val:tie_at_0")),
    ("insert", "le", "src/huffman.rs:61-69 new node before the first strictly smaller entry", ("code_val:all_16_equal", "code_len:all_16_fib")),
    ("children", "swapped", "src/huffman.rs:84-88 left = last popped", ("code_val:typical_frame",)),
    ("bit_order", "msb", "src/huffman.rs:30-32 first branch in bit 0 (LSB-first codes)", ("code_val:typical_frame",)),
    ("filler", "ge15", "src/rle.rs:18, :31 fillers while run > 15", ("pay_runs_bytes",)),
    ("trailing", "drop", "src/rle.rs:36-38 trailing run emitted", ("pay_all_zero_bytes",)),
    ("min1", "none", "src/rle.rs:57 .max(1)", ("table:min1_floor",)),
    ("table_i32", "wide", "src/rle.rs:57 x * 255 wraps in i32 (release build)", ("table:wrap_8421505", "table:wrap_12311503",
                                                                                      "table:wrap_20000000", "table:wrap_17M_of_20M")),
    ("signed_field", "sign_mag", "src/enc.rs:312, :463 write_signed is two's complement", ("pay_runs_bytes",)),
    ("one_symbol", "one_bit", "src/huffman.rs:99-102, :205-208 a one-leaf tree codes its symbol in 0 bits", ("code_len:one_symbol_0",)),
    ("pair_order", "size_first", "src/enc.rs:306-311 num_zeroes code first, then coeff_size", ("pay_runs_bytes",)),
    ("pf_header", "coded_first", "src/enc.rs:414-422 has_mvec bit, then has_coef bit", ("pay_pmixed_bytes",)),
]

ENTROPY_INVISIBLE = [
    ("u8_cast", "saturate",
     "src/rle.rs:57: q = (x * 255) / max <= 255 without wrap (x <= max); with wrap max > 8 421 504 bounds |q| <= 255, and .max(1) "
     "lifts every negative quotient to 1, so `as u8` never truncates"),
    ("code_shift", "wide",
     "src/huffman.rs:31: 16 leaves make a tree at most 15 deep, so (bit as u32) << len shifts by at most 14"),
    ("freq", "wide",
     "src/huffman.rs:86: every leaf weighs at most 255, so no sum of at most 16 of them comes near 2^32"),
]


@pytest.fixture(scope="module")
def entropy_vectors():
    return er.load()


def test_unmutated_entropy_restatement_reproduces_every_vector(entropy_vectors):
    assert ent.RULES == ent.DEFAULT_RULES
    assert er.diff(entropy_vectors, er.recompute(entropy_vectors)) == []


@pytest.mark.parametrize("rule,value,where,must", ENTROPY_VISIBLE, ids=[v[0] for v in ENTROPY_VISIBLE])
def test_entropy_vectors_notice_a_flipped_rule(entropy_vectors, rule, value, where, must):
    ent.RULES[rule] = value
    try:
        changed = er.diff(entropy_vectors, er.recompute(entropy_vectors))
    finally:
        ent.RULES.update(ent.DEFAULT_RULES)
    assert changed, f"no committed entropy vector notices {rule}={value} ({where})"
    assert set(must) <= set(changed), f"{rule}={value}: expected {must} to change, got {changed}"


@pytest.mark.parametrize("rule,value,why", ENTROPY_INVISIBLE, ids=[v[0] for v in ENTROPY_INVISIBLE])
def test_entropy_rules_unobservable_by_theorem(entropy_vectors, rule, value, why):
    ent.RULES[rule] = value
    try:
        changed = er.diff(entropy_vectors, er.recompute(entropy_vectors))
    finally:
        ent.RULES.update(ent.DEFAULT_RULES)
    assert changed == [], f"{rule}={value} was expected to be unobservable ({why}) but changed {changed}"


def test_every_entropy_rule_is_covered():
    assert {v[0] for v in ENTROPY_VISIBLE} | {v[0] for v in ENTROPY_INVISIBLE} == set(ent.DEFAULT_RULES)
