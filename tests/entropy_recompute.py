"""Recomputes every committed entropy vector (tests/golden/entropy_vectors.npz) from its committed INPUTS with the numpy
restatement of the entropy layer (oracle/pfv_oracle_entropy_np.py).  Used by tests/golden/make_entropy_vectors.py (to produce
the vectors), tests/test_entropy_restatement.py (unmutated restatement == committed vectors) and
tests/test_mutation_sensitivity.py (one entropy rule flipped -> some vector changes).

Layout of the file: `hist` [n, 16] i32 crafted histograms with `hist_names`, and their `table` / `code_val` / `code_len`;
payload cases `pay_<name>_coef` [blocks, 256] i16 (+ `_mv` [blocks, 2] i8 and `_has` [blocks] u8 for p-frames) with the
payload bytes in `pay_<name>_bytes`."""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import pfv_oracle_entropy_np as ent   # noqa: E402

VECTORS = os.path.join(HERE, "golden", "entropy_vectors.npz")
OUTPUTS = ("table", "code_val", "code_len")


def load():
    z = np.load(VECTORS)
    return {k: z[k] for k in z.files}


def payload_cases(v):
    return sorted(k[4:-5] for k in v if k.startswith("pay_") and k.endswith("_coef"))


def recompute(v) -> dict:
    """every output key of the file, recomputed from its inputs under the current ent.RULES"""
    out = {}
    rows = [ent.huffman_from_histogram(h) for h in v["hist"]]
    for i, k in enumerate(OUTPUTS):
        out[k] = np.stack([r[i] for r in rows])
    for name in payload_cases(v):
        coef = v[f"pay_{name}_coef"]
        if f"pay_{name}_has" in v:
            b = ent.pframe_payload(v[f"pay_{name}_mv"], v[f"pay_{name}_has"], coef)
        else:
            b = ent.iframe_payload(coef)
        out[f"pay_{name}_bytes"] = np.frombuffer(b, np.uint8)
    return out


def diff(v, got) -> list:
    """names of the vectors that differ: whole output keys for the payloads, `<output>:<histogram name>` for the crafted rows"""
    changed = []
    names = [str(n) for n in v["hist_names"]]
    for k in OUTPUTS:
        for i, n in enumerate(names):
            if not np.array_equal(v[k][i], got[k][i]):
                changed.append(f"{k}:{n}")
    for k in sorted(got):
        if k.startswith("pay_") and not np.array_equal(v[k], got[k]):
            changed.append(k)
    return changed
