"""The decoders' guarded float inverse on the CPU emulator build of the kernel sources: tests/decfloat_cases.py under both lane mappings, with
dense coefficients and with coefficient lists."""
import pytest

import decfloat_cases as dc


@pytest.mark.parametrize("form", dc.FORMS)
@pytest.mark.parametrize("mapping", dc.MAPPINGS, ids=[m[0] for m in dc.MAPPINGS])
@pytest.mark.parametrize("name", dc.CASES)
def test_emu_dec_float(pkg, emu_ctx, oracle, name, mapping, form):
    dc.run_case(pkg, emu_ctx, oracle, name, mapping, form)


def test_emu_dec_transform_option(pkg, emu_ctx):
    L = pkg._lib
    assert emu_ctx.get_option(L.PFV_OPT_DEC_TRANSFORM) == L.PFV_DEC_TRANSFORM_AUTO
    emu_ctx.set_option(L.PFV_OPT_DEC_TRANSFORM, L.PFV_DEC_TRANSFORM_INT)
    try:
        assert emu_ctx.get_option(L.PFV_OPT_DEC_TRANSFORM) == L.PFV_DEC_TRANSFORM_INT
        with pytest.raises(pkg.PfvError):
            emu_ctx.set_option(L.PFV_OPT_DEC_TRANSFORM, 2)
    finally:
        emu_ctx.set_option(L.PFV_OPT_DEC_TRANSFORM, L.PFV_DEC_TRANSFORM_AUTO)
    dec = pkg.DecoderSession(emu_ctx, dc.W, dc.H, dc.flat_tables(), 1)
    with pytest.raises(pkg.PfvError):
        dec.path_stats()                     # not enabled
    dec.enable_path_stats()
    assert dec.path_stats() == (0, 0)
    dec.decode_iframe(dc.quiet_coefs(1)[None])
    assert dec.path_stats() == (0, 3 * 3 + 2 * 2 + 2 * 2)      # 16-lane mapping by grid size: luma 3 rows x 3 wavefronts, chroma 2 x 2 each
    dec.enable_path_stats()                  # again: from zero
    assert dec.path_stats() == (0, 0)
    dec.enable_path_stats(False)
    with pytest.raises(pkg.PfvError):
        dec.path_stats()
    dec.close()
