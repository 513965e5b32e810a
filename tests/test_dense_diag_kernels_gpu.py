"""GPU: the two diagonal empirical-Fisher kernels of ``hf_dense.hip`` (``hf_dense_sq_wgrad``, ``hf_dense_sq_colsum``)
through the C ABI against the float64 references of ``dense_diag_refs`` -- no engine, no ``modelprep``.

Shapes and inputs are those of ``dense_refs`` (``test_dense_diag_refs_cpu.py`` shows on the same numbers that an fp32
evaluation is inside the bound and that wrong variants are outside).  Bound of every comparison: ``(L + R) * u * M`` with
``M`` the result itself (every term is non-negative).  Operands sit in NaN-filled buffers (a read outside ``rows x c``
would poison the result), outputs in NaN-filled buffers with 64 guard words; every launch is issued twice and compared
bitwise; everything runs 16-byte aligned and 4 bytes off that grid."""

import pytest
import torch
from tol import within

import dense_diag_refs as ddr
import dense_refs as dr
from guarded import DEV, ERR_ARG, F32, GUARD, NAN, FlatOut, In, P, _ids, st, twice
from pytorchhessianfree_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("shape", dr.SHAPES, ids=_ids)
def test_sq_wgrad(shape, off):
    rows, c_in, c_out = shape
    lib, c = _lib.load(), dr.case(*shape)
    g, x = In(c["g"], off), In(c["x"], off)
    for scale in (1.0, 1.0 / rows):

        def launch():
            out = FlatOut(c_out * c_in, off, front=GUARD)
            rc = lib.hf_dense_sq_wgrad(out.ptr, g.ptr, x.ptr, rows, c_in, c_out, scale, F32, st())
            assert rc == 0, rc
            return out

        out = twice(launch)
        want, M, L = ddr.sq_wgrad(c["g"], c["x"], scale)
        within(dr.ratio(out.val.view(c_out, c_in).cpu().numpy(), want, M, L + ddr.R_SQ_WGRAD), 1.0, note=(shape, off, scale))


@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("shape", dr.SHAPES, ids=_ids)
def test_sq_colsum(shape, off):
    rows, _, c = shape
    lib, cs = _lib.load(), dr.case(*shape)
    g = In(cs["g"], off)
    for scale in (1.0, 1.0 / rows):

        def launch():
            out = FlatOut(c, off, front=GUARD)
            rc = lib.hf_dense_sq_colsum(out.ptr, g.ptr, rows, c, scale, F32, st())
            assert rc == 0, rc
            return out

        out = twice(launch)
        want, M = ddr.sq_colsum(cs["g"], scale)
        within(dr.ratio(out.val.cpu().numpy(), want, M, ddr.R_SQ_COLSUM), 1.0, note=(shape, off, scale))


def test_sq_entry_points_refuse_bad_arguments():
    """One HF_ERR_ARG case per validated field; nothing is launched."""
    lib = _lib.load()
    buf = torch.zeros(4096, device=DEV)
    b, s = P(buf.data_ptr()), st()
    W, C = lib.hf_dense_sq_wgrad, lib.hf_dense_sq_colsum
    for rows, ci, co in ((0, 4, 4), (257, 4, 4), (4, 0, 4), (4, 4, 0), (4, (1 << 20) + 1, 4), (4, 4, (1 << 20) + 1)):
        assert W(b, b, b, rows, ci, co, 1.0, F32, s) == ERR_ARG
    for rows, c in ((0, 4), (257, 4), (4, 0), (4, (1 << 20) + 1)):
        assert C(b, b, rows, c, 1.0, F32, s) == ERR_ARG
    assert W(b, b, b, 4, 4, 4, 1.0, _lib.HF_F64, s) == ERR_ARG and W(b, b, b, 4, 4, 4, NAN, F32, s) == ERR_ARG
    for args in ((None, b, b), (b, None, b), (b, b, None)):
        assert W(*args, 4, 4, 4, 1.0, F32, s) == ERR_ARG
    assert C(b, b, 4, 4, 1.0, _lib.HF_F64, s) == ERR_ARG and C(b, b, 4, 4, NAN, F32, s) == ERR_ARG
    assert C(None, b, 4, 4, 1.0, F32, s) == ERR_ARG and C(b, None, 4, 4, 1.0, F32, s) == ERR_ARG
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0  # nothing ran
