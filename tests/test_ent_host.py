"""The host coder (csrc/pfv_host.hip: serialize_iframe / serialize_pframe and the payload parsers), CPU only, on the crafted buffers of
tests/ent_cases.py: bytes == the numpy restatement's (which the same cases hold to the C oracle), and the parsers -- dense and sparse -- give
the buffers back.  Codes past 12 bits (long_symbols: 13) take the parsers' one-at-a-time path."""
import pytest

import ent_cases as nc

ALL = dict(nc.CASES, window=nc.window)


@pytest.mark.parametrize("name", sorted(ALL))
def test_host_coder_on_crafted_buffers(graft, pkg, oracle, name):
    graft.build_hip()
    __import__("libswitch").reset(pkg)
    lib = pkg._lib.load()
    case = ALL[name]()
    nc.check_truths(oracle, case)
    assert nc.check_host(pkg, lib, oracle, case) >= 1
