"""The decoder's entropy stage on the device (k_entd_*, k_hdr_*) on a real MI355X against crafted payloads: the shared cases of
tests/entd_cases.py at the shapes of the emulator twins (tests/test_emulated_kernels.py: test_emu_entd_*).  Every case is an equality with the
oracle's decoder, call by call and beyond an error, plus the route the packets took (read on the device / left to the host parser)."""
import pytest

import entd_cases as ec

pytestmark = pytest.mark.gpu


def test_gpu_entd_regular_payloads(pkg, gpu_ctx, oracle):
    ec.check_regular(pkg, gpu_ctx, oracle)


def test_gpu_entd_irregular_payloads(pkg, gpu_ctx, oracle):
    ec.check_irregular(pkg, gpu_ctx, oracle)


def test_gpu_entd_large_payloads(pkg, gpu_ctx, oracle):
    ec.check_large(pkg, gpu_ctx, oracle)
