"""GPU: the tall-batch dense kernels (``hf_dense_tall.hip``, 257 .. 8192 rows) through the C ABI against float64 numpy
references written inline from the formulas of ``include/hf_pcg.h``.  Bound of every comparison: ``(L + R) * 2**-24 * M`` (``L``
the reduction length of one entry, ``R`` the later roundings the header spells out, ``M`` the formula on absolute values).
NaN-filled operands, guarded outputs, every launch twice (bitwise); shapes: the smallest that cross each edge of the tile."""

import ctypes

import numpy as np
import pytest
import torch
from tol import within

from guarded import DEV, ERR_ARG, F32, FlatOut, P, _ids, ip, pp, st, twice
from pytorchhessianfree_amd import _lib

pytestmark = pytest.mark.gpu
U, BK, SCALE = 2.0 ** -24, 16, 0.37
SHAPES = [(257, 4, 4), (257, 37, 5), (300, 130, 129), (385, 17, 260), (129 + 256, 33, 31)]
cases = pytest.mark.parametrize("shape,off", [(s, o) for s in SHAPES for o in (0, 1)], ids=_ids)  # off: floats off the 16-byte grid
kper = lambda n, s: -(-(-(-n // s)) // BK) * BK                              # noqa: E731  (the header's split rule)
split_ok = lambda n, s: 1 <= s <= 32 and (s - 1) * kper(n, s) < n            # noqa: E731


def plan(rows, c_in, c_out):
    c = [ctypes.c_int() for _ in range(4)]
    assert _lib.load().hf_dense_tall_plan(rows, c_in, c_out, *c) == 0
    return [v.value for v in c]


def counts(n, planned):
    assert split_ok(n, planned)  # then: 1, the planned count and the largest the split rule accepts
    return sorted({1, planned, max(s for s in range(1, 33) if split_ok(n, s))})


def ratio(got, want, M, R):
    """max error / bound (printed); where the bound is zero the entry must be exact."""
    err, bound = abs(got.double().cpu().numpy().reshape(want.shape) - want), R * U * M
    assert np.isfinite(err).all() and not ((bound == 0) & (err > 0)).any()
    r = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"ratio {r:.4f}")
    return r


def case(rows, c_in, c_out):
    g = np.random.default_rng(7 * rows + 3 * c_in + c_out)
    f = lambda *sh, s=1.0: (s * g.standard_normal(sh)).astype(np.float32)  # noqa: E731
    return dict(t_x=f(rows, c_in), x=f(rows, c_in), W=f(c_out, c_in, s=c_in ** -0.5), V=f(c_out, c_in, s=c_in ** -0.5),
                g=f(rows, c_out), g2=f(rows, c_out), y=np.tanh(f(rows, c_out)), t_y=f(rows, c_out), h=f(rows, c_out))


def gemm_slabs(pairs, n, splits, left=lambda a: a, right=lambda b: b.T):
    out, mag = [], []  # per split the sum over the pairs of left(a)[.., ks] right(b)[ks, ..] in float64; its magnitude sum
    for lo in range(0, n, kper(n, splits)):
        hi = min(lo + kper(n, splits), n)
        terms = [(left(np.float64(a))[:, lo:hi], right(np.float64(b))[lo:hi]) for a, b in pairs]
        out.append(sum(a @ b for a, b in terms))
        mag.append(sum(abs(a) @ abs(b) for a, b in terms))
    return np.stack(out), np.stack(mag)


def run_slabs(entry, ops, tail, numel, splits, off):
    stride = numel + (3 if splits > 1 else 0)

    def launch():
        out = FlatOut(numel, off, splits, stride)
        assert entry(out.ptr, *[pp(o) for o in ops], *tail, splits, stride, F32, st()) == 0
        return (out,)

    return twice(launch)[0].body


@cases
def test_tangent_slabs(shape, off):
    rows, c_in, c_out = shape
    lib, c, planned = _lib.load(), case(*shape), plan(*shape)[0]
    assert lib.hf_dense_tangent_slabs(*[P(8)] * 5, rows, c_in, c_out, 0, 1, 0, F32, st()) == ERR_ARG  # the skinny range
    for splits in counts(c_in, planned):
        # both terms | t_x only | V only | the forward GEMM (t_x = NULL, V = W) | both terms at a row pitch > c_in
        combos = [("t_x", "V", 0), ("t_x", None, 0), (None, "V", 0), (None, "W", 0), ("t_x", "V", c_in + 3)]
        for k_tx, k_v, ld in combos if splits == planned else combos[:1]:
            wide = lambda a: np.concatenate([a, np.full((rows, ld - c_in), np.nan, np.float32)], 1) if ld else a  # noqa: E731
            ops = [ip(wide(c[k_tx]), off) if k_tx else None, ip(wide(c["x"]), off), ip(c["W"], off), ip(c[k_v], off) if k_v else None]
            got = run_slabs(lib.hf_dense_tall_tangent_slabs, ops, (rows, c_in, c_out, ld), rows * c_out, splits, off)
            pairs = ([(c["t_x"], c["W"])] if k_tx else []) + ([(c["x"], c[k_v])] if k_v else [])
            want, M = gemm_slabs(pairs, c_in, splits)
            within(ratio(got, want, M, len(pairs) * min(kper(c_in, splits), c_in)), 1.0, note=(shape, off, splits, k_tx, k_v, ld))


@cases
def test_dgrad_slabs(shape, off):
    rows, c_in, c_out = shape
    lib, c = _lib.load(), case(*shape)
    for splits in counts(c_out, plan(*shape)[1]):
        for two in (False, True):
            ops = [ip(c["g"], off), ip(c["W"], off), ip(c["g2"], off) if two else None, ip(c["V"], off) if two else None]
            got = run_slabs(lib.hf_dense_tall_dgrad_slabs, ops, (rows, c_in, c_out), rows * c_in, splits, off)
            pairs = [(c["g"], c["W"])] + ([(c["g2"], c["V"])] if two else [])
            want, M = gemm_slabs(pairs, c_out, splits, right=lambda b: b)
            within(ratio(got, want, M, len(pairs) * min(kper(c_out, splits), c_out)), 1.0, note=(shape, off, splits, two))


@pytest.mark.parametrize("mode", (0, 1, 2))  # plain | squared operands | two pairs
@cases
def test_wgrad(shape, off, mode):
    rows, c_in, c_out = shape
    lib, c = _lib.load(), case(*shape)
    ops = [ip(c["g"], off), ip(c["x"], off), ip(c["g2"], off) if mode == 2 else None, ip(c["t_x"], off) if mode == 2 else None]
    sq = (lambda a: a * a) if mode == 1 else (lambda a: a)
    pairs, sc = [(sq(np.float64(c["g"])), sq(np.float64(c["x"])))] + ([(c["g2"], c["t_x"])] if mode == 2 else []), float(np.float32(SCALE))
    for splits in counts(rows, plan(*shape)[2]):
        ws = torch.full((splits * c_out * c_in + 1,), float("nan"), device=DEV)

        def launch():
            out = FlatOut(c_out * c_in, off)
            assert lib.hf_dense_tall_wgrad(out.ptr, P(ws.data_ptr() + 4 * off) if splits > 1 else None, *[pp(o) for o in ops],
                                           rows, c_in, c_out, mode, SCALE, splits, F32, st()) == 0
            return (out,)

        got = twice(launch)[0].val
        want, M = gemm_slabs(pairs, rows, splits, left=lambda a: a.T, right=lambda b: b)
        # R: the slab additions, `scale`, two squarings per product (mode 1), the join of the two chains (mode 2)
        R = (splits - 1) + 1 + (2 if mode == 1 else 0) + (1 if mode == 2 else 0)
        within(ratio(got, sc * want.sum(0), sc * M.sum(0), min(kper(rows, splits), rows) + R), 1.0, note=(shape, off, mode, splits))


@pytest.mark.parametrize("curv", (False, True))
@cases
def test_act_adjoint_and_sq_colsum(shape, off, curv):
    (rows, _, c), lib, cs = shape, _lib.load(), case(*shape)
    act, y, blocks = (2 if curv else 1), np.float64(cs["y"]), plan(*shape)[3]
    ws, sc = torch.full((blocks * c,), float("nan"), dtype=torch.float64, device=DEV), float(np.float32(SCALE))
    for splits in (1, 3):
        slabs = np.random.default_rng(splits).standard_normal((splits, rows * c)).astype(np.float32)
        stride = rows * c + (7 if splits > 1 else 0)
        padded = np.pad(slabs, ((0, 0), (0, stride - rows * c)), constant_values=np.nan)
        ops = [ip(padded, off), ip(cs["y"], off), ip(cs["t_y"], off) if curv else None, ip(cs["h"], off) if curv else None]

        def launch():
            ga, gb = FlatOut(rows * c, off), FlatOut(c, off)
            assert lib.hf_dense_tall_act_adjoint(ga.ptr, gb.ptr, P(ws.data_ptr()), pp(ops[0]), splits, stride, pp(ops[1]), act,
                                                 pp(ops[2]), pp(ops[3]), rows, c, SCALE, F32, st()) == 0
            return ga, gb

        ga, gb = twice(launch)
        s, m = np.float64(slabs).sum(0).reshape(rows, c), abs(np.float64(slabs)).sum(0).reshape(rows, c)
        if curv:  # tanh: (1 - y*y) s - 2 y t_y h
            want = s * (1 - y * y) - 2 * y * np.float64(cs["t_y"]) * np.float64(cs["h"])
            M = m * (1 + y * y) + abs(2 * y * np.float64(cs["t_y"]) * np.float64(cs["h"]))
        else:     # relu on y = tanh(.): the mask y > 0
            want, M = s * (y > 0), m * (y > 0)
        R = (splits - 1) + (5 if curv else 0) or 1  # slab additions; tanh: y*y, 1 - ., s * ., the product with t_y, the fmaf
        within(ratio(ga.val, want, M, R), 1.0, note=(shape, off, curv, splits))
        # the column sums: fp64 accumulation (counted as one rounding), the rounding to fp32, `scale`
        within(ratio(gb.val, sc * want.sum(0), sc * M.sum(0), R + 3), 1.0, note=(shape, off, curv, splits))
    g_in, want = ip(cs["g"], off), sc * (np.float64(cs["g"]) ** 2).sum(0)

    def launch_sq():
        out = FlatOut(c, off)
        assert lib.hf_dense_tall_sq_colsum(out.ptr, P(ws.data_ptr()), g_in.ptr, rows, c, SCALE, F32, st()) == 0
        return (out,)

    within(ratio(twice(launch_sq)[0].val, want, want, 3), 1.0, note=(shape, off))


def test_tall_entry_points_refuse_bad_arguments():
    lib = _lib.load()
    buf = torch.zeros(1 << 16, device=DEV)
    b, s, ints = P(buf.data_ptr()), st(), [ctypes.c_int() for _ in range(4)]
    T, D, Wg = lib.hf_dense_tall_tangent_slabs, lib.hf_dense_tall_dgrad_slabs, lib.hf_dense_tall_wgrad
    A, S = lib.hf_dense_tall_act_adjoint, lib.hf_dense_tall_sq_colsum
    for rows in (256, 8193):  # the row range, at every entry point
        assert lib.hf_dense_tall_plan(rows, 4, 4, *ints) == ERR_ARG
        assert T(b, b, b, b, b, rows, 4, 4, 0, 1, 0, F32, s) == ERR_ARG and D(b, b, b, b, b, rows, 4, 4, 1, 0, F32, s) == ERR_ARG
        assert Wg(b, b, b, b, b, b, rows, 4, 4, 0, 1.0, 1, F32, s) == ERR_ARG and S(b, b, b, rows, 4, 1.0, F32, s) == ERR_ARG
        assert lib.hf_dense_tall_act_forward(b, b, 1, 0, b, 1, rows, 4, F32, s) == ERR_ARG
        assert lib.hf_dense_tall_act_tangent(b, b, 1, 0, b, b, 1, rows, 4, F32, s) == A(b, b, b, b, 1, 0, b, 1, b, b, rows, 4, 1.0, F32, s) == ERR_ARG
    assert T(None, b, b, b, b, 300, 40, 4, 0, 1, 0, F32, s) == ERR_ARG and T(b, None, b, b, None, 300, 40, 4, 0, 1, 0, F32, s) == ERR_ARG  # NULL operands:
    assert T(b, b, b, None, b, 300, 40, 4, 0, 1, 0, F32, s) == ERR_ARG and D(b, None, b, None, None, 300, 4, 40, 1, 0, F32, s) == ERR_ARG
    assert D(b, b, b, None, b, 300, 4, 40, 1, 0, F32, s) == ERR_ARG and Wg(b, b, b, b, b, None, 300, 4, 4, 2, 1.0, 1, F32, s) == ERR_ARG
    assert Wg(b, None, b, b, None, None, 300, 4, 4, 0, 1.0, 2, F32, s) == ERR_ARG and S(b, None, b, 300, 4, 1.0, F32, s) == ERR_ARG
    assert A(b, b, None, b, 1, 0, b, 1, None, None, 300, 4, 1.0, F32, s) == ERR_ARG
    assert T(b, b, b, b, b, 300, 32, 4, 0, 3, 1200, F32, s) == ERR_ARG and D(b, b, b, None, None, 300, 4, 32, 3, 1200, F32, s) == ERR_ARG  # bad splits
    assert Wg(b, b, b, b, None, None, 300, 4, 4, 0, 1.0, 20, F32, s) == ERR_ARG and T(b, b, b, b, b, 300, 40, 4, 0, 2, 1199, F32, s) == ERR_ARG
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0  # nothing ran
