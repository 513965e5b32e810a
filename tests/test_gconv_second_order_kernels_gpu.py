"""GPU: two-term backward and squared sum of hf_gconv.hip against float64 autograd of ``F.conv2d(..., groups=G)`` (CPU), in
guarded buffers, every launch twice.  Rounding bound: ``gamma_K * sum |a_i b_i|`` with K TWICE the products of a sum (the
matrix unit may round a product and its addition separately)."""

import numpy as np
import pytest
import torch

from guarded import ERR_ARG, F32, FlatOut, In, P, U32, _ids, st, twice
from pytorchhessianfree_amd import _lib

pytestmark = pytest.mark.gpu

GEOMETRIES = [  # (n, h, w, G, cg_in, cg_out, (r, s), stride, pad): the twelve of test_gconv_kernels_gpu.py, by value
    (1, 1, 1, 2, 4, 4, (1, 1), (1, 1), (0, 0)), (2, 5, 7, 2, 4, 4, (3, 3), (1, 1), (1, 1)),
    (2, 9, 6, 3, 4, 8, (3, 3), (2, 2), (1, 1)), (2, 6, 6, 3, 8, 4, (3, 3), (1, 1), (0, 0)),
    (1, 2, 2, 2, 4, 4, (3, 3), (1, 1), (1, 1)), (2, 6, 10, 17, 4, 4, (3, 1), (1, 1), (1, 0)),      # small map; second span
    (2, 8, 8, 6, 12, 12, (3, 3), (2, 1), (1, 1)), (1, 9, 9, 2, 16, 16, (5, 5), (1, 1), (2, 2)),   # straddling; two passes
    (1, 4, 4, 2, 64, 64, (3, 3), (1, 1), (1, 1)), (1, 9, 9, 2, 4, 4, (7, 7), (1, 1), (3, 3)),     # width 64; 49 taps
    (2, 9, 9, 16, 4, 4, (3, 3), (2, 2), (1, 1)), (34, 9, 9, 2, 4, 4, (3, 3), (1, 1), (1, 1)),     # 4-row tiles; 46 slabs
]
dims = lambda g: (*g[:3], g[3] * g[4], g[3] * g[5], g[3], *g[6], *g[7], *g[8])  # noqa: E731
nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().float().numpy()  # noqa: E731
grads = lambda geo, x, W, ga: torch.autograd.functional.vjp(  # noqa: E731  (float64 data and weight gradient of ``ga``)
    lambda a, b: torch.nn.functional.conv2d(a, b, None, geo[7], geo[8], 1, geo[3]), (x, W), ga)[1]


def operands(geo, integer, seed=0):  # x, t_x [n, C_in, h, w], W, V [C_out, cg_in, r, s], g', g [n, C_out, oh, ow]
    n, h, w, G, ci, co, (r, s), stride, pad = geo
    g = torch.Generator().manual_seed(seed)
    o = ((h + 2 * pad[0] - r) // stride[0] + 1, (w + 2 * pad[1] - s) // stride[1] + 1)
    draw = (lambda sh: torch.randint(-4, 5, sh, generator=g)) if integer else (lambda sh: torch.randn(sh, generator=g))
    return [draw(sh).double() for sh in [(n, G * ci, h, w)] * 2 + [(G * co, ci, r, s)] * 2 + [(n, G * co, *o)] * 2]


def acts(t_x, x, c, two_pitch, off):  # (pointer of t_x, of x, pitch, buffers): dense maps, or halves of one [t_x | x]
    ins = [In(np.concatenate([nhwc(t_x), nhwc(x)], -1), off)] if two_pitch else [In(nhwc(t), off) for t in (t_x, x)]
    return ins[0].ptr, P(ins[0].ptr.value + 4 * c) if two_pitch else ins[1].ptr, (2 if two_pitch else 1) * c, ins


def backward2(geo, ops, two_pitch=False, off=0):  # -> dx, the slabs' sum, D(g', W) + D(g, V), W(x, g') + W(t_x, g)
    (x, t_x, W, V, gt, g), sw = ops, _lib.load().hf_gconv2d_nhwc_plan(*dims(geo))
    (d1, w1), (d2, w2) = grads(geo, x, W, gt), grads(geo, t_x, V, g)
    ptx, px, ld, keep = acts(t_x, x, geo[3] * geo[4], two_pitch, off)
    gti, gi, wi, vi = In(nhwc(gt), off), In(nhwc(g), off), In(W.float().numpy(), off), In(V.float().numpy(), off)

    def launch():
        dx = FlatOut(x.numel(), off=off, shape=tuple(x.permute(0, 2, 3, 1).shape))
        gw = FlatOut(W.numel(), off=off, slabs=sw, stride=W.numel() + 20)
        assert _lib.load().hf_gconv2d_nhwc_backward2_slabs(dx.ptr, gw.ptr, gti.ptr, gi.ptr, px, ptx, ld, wi.ptr, vi.ptr,
                                                           *dims(geo), sw, gw.stride, F32, st()) == 0
        return dx, gw
    dx, gw = twice(launch)
    return dx.val.cpu().double().permute(0, 3, 1, 2), gw.body.cpu().double().sum(0).view(W.shape), d1 + d2, w1 + w2


@pytest.mark.parametrize("two_pitch, off", [(False, 0), (True, 0), (False, 1), (True, 1)])  # (pitch c / 2c, aligned or not)
@pytest.mark.parametrize("geo", GEOMETRIES, ids=_ids)
def test_two_term_backward_exact_on_integers(geo, two_pitch, off):
    dx, gw, rdx, rgw = backward2(geo, operands(geo, integer=True), two_pitch, off)
    assert torch.equal(dx, rdx) and torch.equal(gw, rgw)


@pytest.mark.parametrize("geo", [GEOMETRIES[6], GEOMETRIES[8], GEOMETRIES[11]], ids=_ids)
def test_two_term_backward_rounding_bound_on_normal_data(geo):
    ops = operands(geo, integer=False, seed=1)
    res, mag = backward2(geo, ops), backward2(geo, [t.abs() for t in ops])  # (mag: the same sums over the magnitudes)
    ks = (2 * 2 * geo[6][0] * geo[6][1] * geo[5], 2 * 2 * geo[0] * ops[4].shape[2] * ops[4].shape[3])  # (dx, gw; two terms)
    pairs = [((res[i] - res[i + 2]).abs(), k * U32 / (1 - k * U32) * mag[i + 2]) for i, k in enumerate(ks)]
    print(f"{geo}: dx, gw at", " ".join(f"{float((e / b).nan_to_num(0.0).max()):.3f}" for e, b in pairs), "of the bound")
    assert all(bool((e <= b).all()) for e, b in pairs)


@pytest.mark.parametrize("pre", [1.0, 2.0])
@pytest.mark.parametrize("geo", GEOMETRIES + [(3, 4, 4, 2, 64, 64, (3, 3), (1, 1), (1, 1))], ids=_ids)  # (+ 3 x 3 passes)
def test_squared_sum_exact_on_integers(geo, pre):
    (x, t_x, W, _, ga, _), n, c = operands(geo, integer=True), geo[0], geo[3] * geo[4]
    ref = sum((pre * grads(geo, x[i:i + 1], W, ga[i:i + 1])[1]) ** 2 for i in range(n))
    assert float(ref.max()) < 2 ** 24  # (so every partial sum is an fp32 integer)
    lib = _lib.load()  # the planned count; ONE split, x a half of [t_x | x] off the 16-byte grid; the plan for 3 workgroups
    for splits, wide in {(lib.hf_gconv2d_nhwc_sqsum_plan(*dims(geo), t), t == 1) for t in (0, 1, 3)}:
        (_, px, ld, keep), gi = acts(t_x, x, c, wide, int(wide)), In(nhwc(ga), int(wide))

        def launch():
            out = FlatOut(W.numel(), off=int(wide), slabs=splits, stride=W.numel() + 20)
            assert lib.hf_gconv2d_nhwc_sqsum_slabs(out.ptr, gi.ptr, px, ld, *dims(geo), pre, splits, out.stride, F32,
                                                   st()) == 0
            return out
        assert torch.equal(twice(launch).body.cpu().double().sum(0).view(W.shape), ref), splits


@pytest.mark.parametrize("case", ["NULL operand", "splits off the plan", "non-finite pre", "width 6"])
def test_refused_arguments_launch_nothing(case):
    lib, geo = _lib.load(), (1, 6, 6, 2, 6, 4, (3, 3), (1, 1), (1, 1)) if case == "width 6" else GEOMETRIES[1]
    n, numel = geo[0], geo[3] * geo[5] * geo[4] * geo[6][0] * geo[6][1]
    buf, dx, gw = In(np.ones(2048, np.float32), 0), FlatOut(n * geo[1] * geo[2] * geo[3] * geo[4]), FlatOut(numel, slabs=3)
    sw, sq = max(1, lib.hf_gconv2d_nhwc_plan(*dims(geo))), max(1, lib.hf_gconv2d_nhwc_sqsum_plan(*dims(geo), 0))
    bad, pre = case == "splits off the plan", float("inf") if case == "non-finite pre" else 1.0
    for null in range(8) if case == "NULL operand" else [None]:
        ptrs = [None if i == null else b.ptr for i, b in enumerate([dx, gw] + [buf] * 6)]
        if case != "non-finite pre":  # (the two-term backward has no such argument)
            assert lib.hf_gconv2d_nhwc_backward2_slabs(*ptrs[:6], 0, *ptrs[6:], *dims(geo), sw + bad, numel, F32,
                                                       st()) == ERR_ARG
        if null is None or 1 <= null <= 3:  # (out, ga, x)
            assert lib.hf_gconv2d_nhwc_sqsum_slabs(*ptrs[1:4], 0, *dims(geo), pre, n + 1 if bad else sq, numel, F32,
                                                   st()) == ERR_ARG
    torch.cuda.synchronize()
    assert dx.pristine() and gw.pristine()
