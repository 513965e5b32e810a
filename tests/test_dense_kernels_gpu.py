"""GPU: the dense-layer kernels (``hf_dense.hip``) through the C ABI against the float64 references of ``dense_refs``
-- no engine, no ``modelprep``.

Inputs come from ``dense_refs`` (seeded on the CPU; ``test_dense_refs_cpu.py`` shows on the same numbers that an fp32
evaluation is inside the bound and that wrong variants are outside).  Bound of every comparison: ``(L + R) * u * M``;
``tol.within`` sees ``value / bound`` against 1.  Operands sit in NaN-filled buffers (a read outside ``rows x c`` would
poison the result), outputs in NaN-filled buffers with 64 guard words; every launch is issued twice and compared
bitwise; everything runs 16-byte aligned and 4 bytes off that grid."""

import ctypes

import numpy as np
import pytest
import torch
from tol import within

import dense_refs as dr
from guarded import DEV, ERR_ARG, F32, NAN, FlatOut, P, _ids, ip, pp, st, twice
from pytorchhessianfree_amd import _lib

pytestmark = pytest.mark.gpu


def plan(rows, c_in, c_out):
    s_t, s_d = ctypes.c_int(), ctypes.c_int()
    assert _lib.load().hf_dense_plan(rows, c_in, c_out, s_t, s_d) == 0
    return s_t.value, s_d.value


@pytest.mark.parametrize("shape", dr.SHAPES, ids=_ids)
def test_plan_returns_counts_the_split_rule_accepts(shape):
    rows, c_in, c_out = shape
    s_t, s_d = plan(*shape)
    assert dr.split_ok(c_in, s_t) and dr.split_ok(c_out, s_d)


# ---- T ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("shape", dr.SHAPES, ids=_ids)
def test_tangent_slabs(shape, off):
    rows, c_in, c_out = shape
    lib, c = _lib.load(), dr.case(*shape)
    planned = plan(*shape)[0]
    for splits in dr.split_counts(c_in, planned):
        # both terms | first live layer | frozen weight | the forward GEMM (t_x = NULL, V = W)
        combos = [("t_x", "V"), (None, "V"), ("t_x", None), (None, "W")] if splits == planned else [("t_x", "V")]
        for k_tx, k_v in combos:
            t_x, V = (c[k_tx] if k_tx else None), (c[k_v] if k_v else None)
            ops = [ip(t_x, off), ip(c["x"], off), ip(c["W"], off), ip(V, off)]
            stride = rows * c_out + (3 if splits > 1 else 0)

            def launch():
                out = FlatOut(rows * c_out, off, splits, stride)
                rc = lib.hf_dense_tangent_slabs(out.ptr, *[pp(o) for o in ops], rows, c_in, c_out, 0, splits, stride, F32,
                                                st())
                assert rc == 0, rc
                return (out,)

            (out,) = twice(launch)
            want, M, L = dr.tangent_slabs(t_x, c["x"], c["W"], V, splits)
            within(dr.ratio(out.body.reshape(-1, rows, c_out).cpu().numpy(), want, M, L + dr.R_SLAB), 1.0, note=(shape, off, splits, k_tx, k_v))


def test_tangent_slabs_row_pitch():
    """``ld_x``: t_x and x as the first-c_in-columns slices of wider rows (the rest holds NaN)."""
    rows, c_in, c_out, ld = 33, 65, 31, 72
    lib, c = _lib.load(), dr.case(rows, c_in, c_out)
    wide = lambda a: np.concatenate([a, np.full((rows, ld - c_in), np.nan, np.float32)], 1)  # noqa: E731
    ops = [ip(wide(c["t_x"]), 0), ip(wide(c["x"]), 0), ip(c["W"], 0), ip(c["V"], 0)]

    def launch():
        out = FlatOut(rows * c_out, 0, 2, rows * c_out)
        assert lib.hf_dense_tangent_slabs(out.ptr, *[pp(o) for o in ops], rows, c_in, c_out, ld, 2, rows * c_out, F32,
                                          st()) == 0
        return (out,)

    (out,) = twice(launch)
    want, M, L = dr.tangent_slabs(c["t_x"], c["x"], c["W"], c["V"], 2)
    within(dr.ratio(out.body.reshape(-1, rows, c_out).cpu().numpy(), want, M, L + dr.R_SLAB), 1.0)


# ---- D ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("shape", dr.SHAPES, ids=_ids)
def test_dgrad_slabs(shape, off):
    rows, c_in, c_out = shape
    lib, c = _lib.load(), dr.case(*shape)
    ops = [ip(c["g"], off), ip(c["W"], off)]
    for splits in dr.split_counts(c_out, plan(*shape)[1]):
        stride = rows * c_in + (5 if splits > 1 else 0)

        def launch():
            out = FlatOut(rows * c_in, off, splits, stride)
            rc = lib.hf_dense_dgrad_slabs(out.ptr, *[pp(o) for o in ops], rows, c_in, c_out, splits, stride, F32, st())
            assert rc == 0, rc
            return (out,)

        (out,) = twice(launch)
        want, M, L = dr.dgrad_slabs(c["g"], c["W"], splits)
        within(dr.ratio(out.body.reshape(-1, rows, c_in).cpu().numpy(), want, M, L + dr.R_SLAB), 1.0, note=(shape, off, splits))


# ---- W ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("shape", dr.SHAPES, ids=_ids)
def test_wgrad(shape, off):
    rows, c_in, c_out = shape
    lib, c = _lib.load(), dr.case(*shape)
    ops = [ip(c["g"], off), ip(c["x"], off)]

    def launch():
        out = FlatOut(c_out * c_in, off)
        rc = lib.hf_dense_wgrad(out.ptr, *[pp(o) for o in ops], rows, c_in, c_out, c["scale"], F32, st())
        assert rc == 0, rc
        return (out,)

    (out,) = twice(launch)
    want, M, L = dr.wgrad(c["g"], c["x"], c["scale"])
    within(dr.ratio(out.val.view(c_out, c_in).cpu().numpy(), want, M, L + dr.R_WGRAD), 1.0, note=(shape, off))


# ---- the elementwise passes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", dr.ACTS)
@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("shape", dr.SHAPES, ids=_ids)
def test_act_tangent(shape, off, act):
    rows, _, c = shape
    lib, cs = _lib.load(), dr.case(*shape)
    y = cs["y"][act]
    for splits in (1, 2, 5):
        for v_b in (cs["v_b"], None):
            slabs = dr.slabs_for((rows, c), splits)
            stride = rows * c + (7 if splits > 1 else 0)
            padded = np.full((splits, stride), np.nan, np.float32)
            padded[:, :rows * c] = slabs.reshape(splits, -1)
            ops = [ip(padded, off), ip(v_b, off), ip(y, off) if not (act == dr.IDENTITY and v_b is None) else None]

            def launch():
                out = FlatOut(rows * c, off)
                rc = lib.hf_dense_act_tangent(out.ptr, pp(ops[0]), splits, stride, pp(ops[1]), pp(ops[2]), act, rows, c,
                                              F32, st())
                assert rc == 0, rc
                return (out,)

            (out,) = twice(launch)
            want, M = dr.act_tangent(slabs, v_b, y, act)
            within(dr.ratio(out.val.view(rows, c).cpu().numpy(), want, M, dr.r_act(splits, v_b is not None, act)), 1.0,
                   note=(shape, off, act, splits))


@pytest.mark.parametrize("act", dr.ACTS)
@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("shape", dr.SHAPES, ids=_ids)
def test_act_adjoint(shape, off, act):
    rows, _, c = shape
    lib, cs = _lib.load(), dr.case(*shape)
    y = cs["y"][act]
    for splits in (1, 2, 5):
        for with_b in (True, False):
            slabs = dr.slabs_for((rows, c), splits, seed=2)
            stride = rows * c + (7 if splits > 1 else 0)
            padded = np.full((splits, stride), np.nan, np.float32)
            padded[:, :rows * c] = slabs.reshape(splits, -1)
            ops = [ip(padded, off), ip(y, off)]

            def launch():
                ga, gb = FlatOut(rows * c, off), (FlatOut(c, off) if with_b else None)
                rc = lib.hf_dense_act_adjoint(ga.ptr, pp(gb), pp(ops[0]), splits, stride, pp(ops[1]), act, rows, c,
                                              cs["scale"], F32, st())
                assert rc == 0, rc
                return ga, gb

            ga, gb = twice(launch)
            want_a, Ma, want_b, Mb = dr.act_adjoint(slabs, y, act, cs["scale"])
            within(dr.ratio(ga.val.view(rows, c).cpu().numpy(), want_a, Ma, dr.r_act(splits, False, act)), 1.0,
                   note=(shape, off, act, splits))
            if with_b:
                within(dr.ratio(gb.val.cpu().numpy(), want_b, Mb, dr.r_bias(splits, act)), 1.0, note=(shape, off, act, splits))


# ---- refusals: one HF_ERR_ARG case per validated field, nothing is launched ---------------------------------------
def test_dense_entry_points_refuses_bad_arguments():
    lib = _lib.load()
    buf = torch.zeros(4096, device=DEV)
    b, s = P(buf.data_ptr()), st()
    s_t, s_d = ctypes.c_int(), ctypes.c_int()
    for rows, ci, co in ((0, 4, 4), (257, 4, 4), (4, 0, 4), (4, 4, 0), (4, (1 << 20) + 1, 4), (4, 4, (1 << 20) + 1)):
        assert lib.hf_dense_plan(rows, ci, co, s_t, s_d) == ERR_ARG
        assert lib.hf_dense_tangent_slabs(b, b, b, b, b, rows, ci, co, 0, 1, 0, F32, s) == ERR_ARG
        assert lib.hf_dense_dgrad_slabs(b, b, b, rows, ci, co, 1, 0, F32, s) == ERR_ARG
        assert lib.hf_dense_wgrad(b, b, b, rows, ci, co, 1.0, F32, s) == ERR_ARG
    assert lib.hf_dense_plan(4, 4, 4, None, s_d) == ERR_ARG and lib.hf_dense_plan(4, 4, 4, s_t, None) == ERR_ARG
    T = lib.hf_dense_tangent_slabs
    assert T(b, b, b, b, b, 4, 40, 4, 0, 1, 0, _lib.HF_F64, s) == ERR_ARG      # dtype
    assert T(None, b, b, b, b, 4, 40, 4, 0, 1, 0, F32, s) == ERR_ARG            # no output
    assert T(b, None, b, b, None, 4, 40, 4, 0, 1, 0, F32, s) == ERR_ARG         # neither term
    assert T(b, b, b, None, b, 4, 40, 4, 0, 1, 0, F32, s) == ERR_ARG            # t_x without W
    assert T(b, b, None, b, b, 4, 40, 4, 0, 1, 0, F32, s) == ERR_ARG            # V without x
    assert T(b, b, b, b, b, 4, 40, 4, 39, 1, 0, F32, s) == ERR_ARG              # row pitch below c_in
    assert T(b, b, b, b, b, 4, 40, 4, 0, 0, 0, F32, s) == ERR_ARG               # splits < 1
    assert T(b, b, b, b, b, 4, 40, 4, 0, 33, 16, F32, s) == ERR_ARG             # splits > 32
    assert T(b, b, b, b, b, 4, 64, 4, 0, 3, 16, F32, s) == ERR_ARG              # the third split would be empty
    assert T(b, b, b, b, b, 4, 40, 4, 0, 2, 15, F32, s) == ERR_ARG              # slabs would overlap
    D = lib.hf_dense_dgrad_slabs
    assert D(b, b, b, 4, 4, 40, 1, 0, _lib.HF_F64, s) == ERR_ARG
    for args in ((None, b, b), (b, None, b), (b, b, None)):
        assert D(*args, 4, 4, 40, 1, 0, F32, s) == ERR_ARG
    assert D(b, b, b, 4, 4, 40, 0, 0, F32, s) == ERR_ARG and D(b, b, b, 4, 4, 64, 3, 16, F32, s) == ERR_ARG
    assert D(b, b, b, 4, 4, 40, 2, 15, F32, s) == ERR_ARG
    W = lib.hf_dense_wgrad
    assert W(b, b, b, 4, 4, 4, 1.0, _lib.HF_F64, s) == ERR_ARG and W(b, b, b, 4, 4, 4, NAN, F32, s) == ERR_ARG
    for args in ((None, b, b), (b, None, b), (b, b, None)):
        assert W(*args, 4, 4, 4, 1.0, F32, s) == ERR_ARG
    A = lib.hf_dense_act_tangent
    assert A(None, b, 1, 0, b, b, 1, 4, 4, F32, s) == ERR_ARG and A(b, None, 1, 0, b, b, 1, 4, 4, F32, s) == ERR_ARG
    assert A(b, b, 0, 0, b, b, 1, 4, 4, F32, s) == ERR_ARG and A(b, b, 33, 16, b, b, 1, 4, 4, F32, s) == ERR_ARG
    assert A(b, b, 2, 15, b, b, 1, 4, 4, F32, s) == ERR_ARG                      # slabs overlap
    assert A(b, b, 1, 0, b, b, 3, 4, 4, F32, s) == ERR_ARG and A(b, b, 1, 0, b, b, -1, 4, 4, F32, s) == ERR_ARG
    assert A(b, b, 1, 0, b, None, 2, 4, 4, F32, s) == ERR_ARG                    # tanh without y
    assert A(b, b, 1, 0, b, b, 1, 0, 4, F32, s) == ERR_ARG and A(b, b, 1, 0, b, b, 1, 257, 4, F32, s) == ERR_ARG
    assert A(b, b, 1, 0, b, b, 1, 4, 0, F32, s) == ERR_ARG and A(b, b, 1, 0, b, b, 1, 4, 4, _lib.HF_F64, s) == ERR_ARG
    J = lib.hf_dense_act_adjoint
    assert J(None, b, b, 1, 0, b, 1, 4, 4, 1.0, F32, s) == ERR_ARG and J(b, b, None, 1, 0, b, 1, 4, 4, 1.0, F32, s) == ERR_ARG
    assert J(b, b, b, 0, 0, b, 1, 4, 4, 1.0, F32, s) == ERR_ARG and J(b, b, b, 2, 15, b, 1, 4, 4, 1.0, F32, s) == ERR_ARG
    assert J(b, b, b, 1, 0, b, 3, 4, 4, 1.0, F32, s) == ERR_ARG and J(b, b, b, 1, 0, None, 1, 4, 4, 1.0, F32, s) == ERR_ARG
    assert J(b, b, b, 1, 0, b, 1, 257, 4, 1.0, F32, s) == ERR_ARG and J(b, b, b, 1, 0, b, 1, 4, 0, 1.0, F32, s) == ERR_ARG
    assert J(b, b, b, 1, 0, b, 1, 4, 4, NAN, F32, s) == ERR_ARG and J(b, b, b, 1, 0, b, 1, 4, 4, 1.0, _lib.HF_F64, s) == ERR_ARG
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0  # nothing ran
