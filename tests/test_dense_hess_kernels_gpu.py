"""GPU: the three kernels of the dense-stack engine's Hessian sweep (``hf_dense_wgrad2``, ``hf_dense_dgrad2_slabs``,
``hf_dense_act_adjoint2`` of ``hf_dense.hip``) through the C ABI against the float64 references of ``dense_hess_refs`` --
no engine, no ``modelprep``.

Inputs come from ``dense_hess_refs.case`` (seeded on the CPU; ``test_dense_hess_refs_cpu.py`` shows on the same numbers
that an fp32 evaluation is inside the bound and that wrong variants are outside).  Bound of every comparison:
``(L + R) * u * M``; ``tol.within`` sees ``value / bound`` against 1.  Operands sit in NaN-filled buffers (a read outside
``rows x c`` would poison the result), outputs in NaN-filled buffers with 64 guard words; every launch is issued twice
and compared bitwise; everything runs 16-byte aligned and 4 bytes off that grid."""

import ctypes

import numpy as np
import pytest
import torch
from tol import within

import dense_hess_refs as hr
import dense_refs as dr
from guarded import DEV, ERR_ARG, F32, NAN, FlatOut, In, P, _ids, pp, st, twice
from pytorchhessianfree_amd import _lib

pytestmark = pytest.mark.gpu


def planned_d(rows, c_in, c_out):
    s_t, s_d = ctypes.c_int(), ctypes.c_int()
    assert _lib.load().hf_dense_plan(rows, c_in, c_out, s_t, s_d) == 0
    return s_d.value


# ---- W2 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("shape", dr.SHAPES, ids=_ids)
def test_wgrad2(shape, off):
    rows, c_in, c_out = shape
    lib, c = _lib.load(), hr.case(*shape)
    ops = [In(c[k], off) for k in ("g", "x", "g1", "t_x")]

    def launch():
        out = FlatOut(c_out * c_in, off)
        rc = lib.hf_dense_wgrad2(out.ptr, *[pp(o) for o in ops], rows, c_in, c_out, c["scale"], F32, st())
        assert rc == 0, rc
        return (out,)

    (out,) = twice(launch)
    want, M, L = hr.wgrad2(c["g"], c["x"], c["g1"], c["t_x"], c["scale"])
    within(dr.ratio(out.val.view(c_out, c_in).cpu().numpy(), want, M, L + hr.R_WGRAD2), 1.0, note=(shape, off))


# ---- D2 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("shape", dr.SHAPES, ids=_ids)
def test_dgrad2_slabs(shape, off):
    rows, c_in, c_out = shape
    lib, c = _lib.load(), hr.case(*shape)
    ops = [In(c[k], off) for k in ("g", "W", "g1", "V")]
    for splits in dr.split_counts(c_out, planned_d(*shape)):
        stride = rows * c_in + (5 if splits > 1 else 0)

        def launch():
            out = FlatOut(rows * c_in, off, splits, stride)
            rc = lib.hf_dense_dgrad2_slabs(out.ptr, *[pp(o) for o in ops], rows, c_in, c_out, splits, stride, F32, st())
            assert rc == 0, rc
            return (out,)

        (out,) = twice(launch)
        want, M, L = hr.dgrad2_slabs(c["g"], c["W"], c["g1"], c["V"], splits)
        within(dr.ratio(out.body.reshape(-1, rows, c_in).cpu().numpy(), want, M, L + dr.R_SLAB), 1.0, note=(shape, off, splits))


# ---- the elementwise pass --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", dr.ACTS)
@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("shape", dr.SHAPES, ids=_ids)
def test_act_adjoint2(shape, off, act):
    rows, _, c = shape
    lib, cs = _lib.load(), hr.case(*shape)
    y, t_y, h = cs["y"][act], cs["t_y"][act], cs["h"]
    nan = np.full((rows, c), np.nan, np.float32)
    for splits in (1, 2, 5):
        for with_b in (True, False):
            slabs = dr.slabs_for((rows, c), splits, seed=2)
            stride = rows * c + (7 if splits > 1 else 0)
            padded = np.full((splits, stride), np.nan, np.float32)
            padded[:, :rows * c] = slabs.reshape(splits, -1)
            s_in, y_in = In(padded, off), In(y, off)
            if act == dr.TANH:
                curv = [(In(t_y, off), In(h, off))]
            else:  # no curvature term: NULL, and NaN buffers that must not be read
                curv = [(None, None), (In(nan, off), In(nan, off))]
            for ty_in, h_in in curv:
                def launch():
                    ga, gb = FlatOut(rows * c, off), (FlatOut(c, off) if with_b else None)
                    rc = lib.hf_dense_act_adjoint2(ga.ptr, pp(gb), s_in.ptr, splits, stride, y_in.ptr, act, pp(ty_in),
                                                   pp(h_in), rows, c, cs["scale"], F32, st())
                    assert rc == 0, rc
                    return ga, gb

                ga, gb = twice(launch)
                want_a, Ma, want_b, Mb = hr.act_adjoint2(slabs, y, act, t_y, h, cs["scale"])
                within(dr.ratio(ga.val.view(rows, c).cpu().numpy(), want_a, Ma, hr.r_act2(splits, act)), 1.0,
                       note=(shape, off, act, splits))
                if with_b:
                    within(dr.ratio(gb.val.cpu().numpy(), want_b, Mb, hr.r_bias2(splits, act)), 1.0,
                           note=(shape, off, act, splits))
                if act != dr.TANH:  # bitwise hf_dense_act_adjoint on the same inputs
                    ga1, gb1 = FlatOut(rows * c, off), (FlatOut(c, off) if with_b else None)
                    assert lib.hf_dense_act_adjoint(ga1.ptr, pp(gb1), s_in.ptr, splits, stride, y_in.ptr, act, rows, c,
                                                    cs["scale"], F32, st()) == 0
                    torch.cuda.synchronize()
                    assert ga.same(ga1) and (gb is None or gb.same(gb1))


# ---- refusals: one HF_ERR_ARG case per validated field, nothing is launched ---------------------------------------
def test_hessian_entry_points_refuse_bad_arguments():
    lib = _lib.load()
    buf = torch.zeros(4096, device=DEV)
    b, s = P(buf.data_ptr()), st()
    W2, D2, J2 = lib.hf_dense_wgrad2, lib.hf_dense_dgrad2_slabs, lib.hf_dense_act_adjoint2
    for rows, ci, co in ((0, 4, 4), (257, 4, 4), (4, 0, 4), (4, 4, 0), (4, (1 << 20) + 1, 4), (4, 4, (1 << 20) + 1)):
        assert W2(b, b, b, b, b, rows, ci, co, 1.0, F32, s) == ERR_ARG
        assert D2(b, b, b, b, b, rows, ci, co, 1, 0, F32, s) == ERR_ARG
    for i in range(5):  # each NULL operand
        args = [b] * 5
        args[i] = None
        assert W2(*args, 4, 4, 4, 1.0, F32, s) == ERR_ARG
        assert D2(*args, 4, 4, 40, 1, 0, F32, s) == ERR_ARG
    assert W2(b, b, b, b, b, 4, 4, 4, 1.0, _lib.HF_F64, s) == ERR_ARG and W2(b, b, b, b, b, 4, 4, 4, NAN, F32, s) == ERR_ARG
    assert D2(b, b, b, b, b, 4, 4, 40, 1, 0, _lib.HF_F64, s) == ERR_ARG
    assert D2(b, b, b, b, b, 4, 4, 40, 0, 0, F32, s) == ERR_ARG      # splits < 1
    assert D2(b, b, b, b, b, 4, 4, 40, 33, 16, F32, s) == ERR_ARG    # splits > 32
    assert D2(b, b, b, b, b, 4, 4, 64, 3, 16, F32, s) == ERR_ARG     # the third split would be empty
    assert D2(b, b, b, b, b, 4, 4, 40, 2, 15, F32, s) == ERR_ARG     # slabs would overlap
    for act in dr.ACTS:
        assert J2(None, b, b, 1, 0, b, act, b, b, 4, 4, 1.0, F32, s) == ERR_ARG   # no output
        assert J2(b, b, None, 1, 0, b, act, b, b, 4, 4, 1.0, F32, s) == ERR_ARG   # no slabs
        assert J2(b, b, b, 0, 0, b, act, b, b, 4, 4, 1.0, F32, s) == ERR_ARG and J2(b, b, b, 33, 16, b, act, b, b, 4, 4, 1.0, F32, s) == ERR_ARG
        assert J2(b, b, b, 2, 15, b, act, b, b, 4, 4, 1.0, F32, s) == ERR_ARG     # slabs overlap
        assert J2(b, b, b, 1, 0, b, act, b, b, 0, 4, 1.0, F32, s) == ERR_ARG and J2(b, b, b, 1, 0, b, act, b, b, 257, 4, 1.0, F32, s) == ERR_ARG
        assert J2(b, b, b, 1, 0, b, act, b, b, 4, 0, 1.0, F32, s) == ERR_ARG
        assert J2(b, b, b, 1, 0, b, act, b, b, 4, 4, NAN, F32, s) == ERR_ARG
        assert J2(b, b, b, 1, 0, b, act, b, b, 4, 4, 1.0, _lib.HF_F64, s) == ERR_ARG
    assert J2(b, b, b, 1, 0, b, 3, b, b, 4, 4, 1.0, F32, s) == ERR_ARG and J2(b, b, b, 1, 0, b, -1, b, b, 4, 4, 1.0, F32, s) == ERR_ARG
    assert J2(b, b, b, 1, 0, None, dr.RELU, b, b, 4, 4, 1.0, F32, s) == ERR_ARG   # relu without y
    assert J2(b, b, b, 1, 0, None, dr.TANH, b, b, 4, 4, 1.0, F32, s) == ERR_ARG   # tanh without y
    assert J2(b, b, b, 1, 0, b, dr.TANH, None, b, 4, 4, 1.0, F32, s) == ERR_ARG   # tanh without t_y
    assert J2(b, b, b, 1, 0, b, dr.TANH, b, None, 4, 4, 1.0, F32, s) == ERR_ARG   # tanh without h
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0  # nothing ran
