"""The encoder's entropy stage on the device (k_ent_scan / _codes / _init / _pack / _gather) against the numpy restatement of the entropy layer
and the C oracle on an MI355X, on the crafted buffers of tests/ent_cases.py: 41-bit symbols at every bit phase (a symbol's third payload
word), one- and two-symbol tables, group and symbol-list seams, every run length, header phases and vector edges, oversize values, the
payload capacity's edge, and the two 2048-wide geometries with exactly 256 and with 258 groups."""
import pytest

import ent_cases as nc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(nc.CASES))
def test_gpu_ent_cases(gpu_ctx, pkg, oracle, name):
    """EncoderSession.pack_iframe_dev / pack_pframe_dev / payload_sizes / payload (long_symbols and degenerate_tables through payloads() =
    pfv_enc_payloads_fetch = k_ent_gather as well): bytes == the restatement's == the C oracle's, errors as the reference's panics"""
    case = nc.CASES[name]()
    assert nc.check_device(pkg, gpu_ctx, oracle, case) >= len(case.frames)


@pytest.mark.parametrize("name", sorted(nc.LARGE))
def test_gpu_ent_code_chunks(gpu_ctx, pkg, oracle, name):
    """k_ent_codes walks a stream's groups 256 at a time: 2048 x 1360 has exactly 256, 2048 x 1376 has 258"""
    case = nc.LARGE[name]()
    assert nc.check_device(pkg, gpu_ctx, oracle, case) == 1
