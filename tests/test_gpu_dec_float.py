"""The decoders' guarded float inverse on the device: tests/decfloat_cases.py under both lane mappings, with dense coefficients and with
coefficient lists -- byte for byte against the oracle and against PFV_DEC_TRANSFORM_INT, with the count of integer-path wavefronts
predicted on the CPU."""
import pytest

import decfloat_cases as dc


@pytest.mark.gpu
@pytest.mark.parametrize("form", dc.FORMS)
@pytest.mark.parametrize("mapping", dc.MAPPINGS, ids=[m[0] for m in dc.MAPPINGS])
@pytest.mark.parametrize("name", dc.CASES)
def test_gpu_dec_float(pkg, gpu_ctx, oracle, name, mapping, form):
    dc.run_case(pkg, gpu_ctx, oracle, name, mapping, form)
