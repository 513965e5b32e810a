"""GPU: the grouped kernels (hf_gconv.hip) against ``F.conv2d(..., groups=G)`` and its autograd in float64 (CPU), in
guarded buffers, every launch twice.  Integer data: exact (a wrong lane map of the 4x4x1 MFMA cannot pass).  Normal data:
``|got - ref| <= gamma_K * sum |a_i b_i|`` with K TWICE the products of the sum (the matrix unit may round a product and
its addition separately)."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from guarded import ERR_ARG, F32, FlatOut, In, P, U32, _ids, st, twice
from pytorchhessianfree_amd import _lib

pytestmark = pytest.mark.gpu

GEOMETRIES = [  # (n, h, w, G, cg_in, cg_out, (r, s), stride, pad)
    (1, 1, 1, 2, 4, 4, (1, 1), (1, 1), (0, 0)),
    (2, 5, 7, 2, 4, 4, (3, 3), (1, 1), (1, 1)),
    (2, 9, 6, 3, 4, 8, (3, 3), (2, 2), (1, 1)),     # two output quads per group, exact-division taps
    (2, 6, 6, 3, 8, 4, (3, 3), (1, 1), (0, 0)),     # cg_in wider than cg_out, no padding
    (1, 2, 2, 2, 4, 4, (3, 3), (1, 1), (1, 1)),     # a map smaller than the kernel
    (2, 6, 10, 17, 4, 4, (3, 1), (1, 1), (1, 0)),   # C_out = 68: a second span, one quad wide
    (2, 8, 8, 6, 12, 12, (3, 3), (2, 1), (1, 1)),   # group 5 straddles the 64-channel span; per-axis stride
    (1, 9, 9, 2, 16, 16, (5, 5), (1, 1), (2, 2)),   # 25 taps: two weight-gradient passes of 50 slots
    (1, 4, 4, 2, 64, 64, (3, 3), (1, 1), (1, 1)),   # the widest group: chunks of 20 channels, three passes
    (1, 9, 9, 2, 4, 4, (7, 7), (1, 1), (3, 3)),     # 49 taps
    (2, 9, 9, 16, 4, 4, (3, 3), (2, 2), (1, 1)),    # 16 groups per span at stride 2: 4-row tiles
    (34, 9, 9, 2, 4, 4, (3, 3), (1, 1), (1, 1)),    # 2 x 2 tiles per sample: 136 units in 46 slabs of 3, the last of 1
]
FORMS = [(False, True), (True, True), (False, True), (True, False)]  # (t_x * W, x * V): the first one is V = W, the forward
nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().float().numpy()  # noqa: E731


def dims(geo):
    n, h, w, G, ci, co, (r, s), stride, pad = geo
    return n, h, w, G * ci, G * co, G, r, s, *stride, *pad


def operands(geo, integer, seed=0):
    """x, t_x [n, C_in, h, w], W, V [C_out, cg_in, r, s], ga [n, C_out, oh, ow] in float64 (float32 draws, widened)."""
    n, h, w, G, ci, co, (r, s), stride, pad = geo
    g = torch.Generator().manual_seed(seed)
    oh, ow = (h + 2 * pad[0] - r) // stride[0] + 1, (w + 2 * pad[1] - s) // stride[1] + 1
    draw = (lambda sh: torch.randint(-4, 5, sh, generator=g)) if integer else (lambda sh: torch.randn(sh, generator=g))
    shapes = [(n, G * ci, h, w), (n, G * ci, h, w), (G * co, ci, r, s), (G * co, ci, r, s), (n, G * co, oh, ow)]
    return [draw(sh).double() for sh in shapes]


def acts(t_x, x, c, two_pitch, off):
    """(pointer of t_x, of x, pixel pitch, the buffers): dense maps, or the halves of one [t_x | x] buffer (absent: NaN)."""
    if not two_pitch:
        ins = [None if t is None else In(nhwc(t), off) for t in (t_x, x)]
        return *(None if i is None else i.ptr for i in ins), c, ins
    shape = nhwc(x if t_x is None else t_x).shape
    cat = In(np.concatenate([np.full(shape, np.nan, np.float32) if t is None else nhwc(t) for t in (t_x, x)], -1), off)
    return None if t_x is None else cat.ptr, None if x is None else P(cat.ptr.value + 4 * c), 2 * c, [cat]


def tangent(geo, t_x, x, W, V, two_pitch=True, off=0):
    """The launch (twice) and the float64 value of ``conv(t_x, W) + conv(x, V)``; an absent term is None."""
    G, stride, pad = geo[3], geo[7], geo[8]
    ref = sum(F.conv2d(a, m, None, stride, pad, 1, G) for a, m in ((t_x, W), (x, V)) if a is not None and m is not None)
    ptx, px, ld, keep = acts(t_x if W is not None else None, x if V is not None else None, G * geo[4], two_pitch, off)
    wi, vi = (None if m is None else In(m.float().numpy(), off) for m in (W, V))

    def launch():
        out = FlatOut(ref.numel(), off=off, shape=tuple(ref.permute(0, 2, 3, 1).shape))
        assert _lib.load().hf_gconv2d_nhwc_tangent(out.ptr, ptx, px, ld, None if wi is None else wi.ptr,
                                                   None if vi is None else vi.ptr, *dims(geo), F32, st()) == 0
        return out
    return twice(launch).val.cpu().double().permute(0, 3, 1, 2), ref


def backward(geo, x, W, ga, two_pitch=False, off=0, with_dx=True):
    """The launch (twice): (dx or None, the slabs summed in float64), and their float64 values by autograd."""
    G, stride, pad = geo[3], geo[7], geo[8]
    x64, w64 = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    rdx, rgw = torch.autograd.grad(F.conv2d(x64, w64, None, stride, pad, 1, G), (x64, w64), ga)
    _, px, ld, keep = acts(None, x, G * geo[4], two_pitch, off)
    gi, wi, sw = In(nhwc(ga), off), In(W.float().numpy(), off), _lib.load().hf_gconv2d_nhwc_plan(*dims(geo))

    def launch():
        dx = FlatOut(x.numel(), off=off, shape=tuple(x.permute(0, 2, 3, 1).shape)) if with_dx else None
        gw = FlatOut(W.numel(), off=off, slabs=sw, stride=W.numel() + 20)
        assert _lib.load().hf_gconv2d_nhwc_backward_slabs(None if dx is None else dx.ptr, gw.ptr, gi.ptr, px, ld,
                                                          wi.ptr if with_dx else None, *dims(geo), sw, gw.stride, F32,
                                                          st()) == 0
        return dx, gw
    dx, gw = twice(launch)
    got_dx = None if dx is None else dx.val.cpu().double().permute(0, 3, 1, 2)
    return got_dx, gw.body.cpu().double().sum(0).view(W.shape), rdx, rgw


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "elementwise"])
@pytest.mark.parametrize("two_pitch", [False, True], ids=["pitch-c", "pitch-2c"])
@pytest.mark.parametrize("geo", GEOMETRIES, ids=_ids)
def test_exact_on_integers(geo, two_pitch, off):
    x, t_x, W, V, ga = operands(geo, integer=True)
    for i, (has_t, has_v) in enumerate(FORMS):
        got, ref = tangent(geo, t_x if has_t else None, x, W if has_t else None, (W if i == 0 else V) if has_v else None,
                           two_pitch, off)
        assert torch.equal(got, ref), i
    for with_dx in (True, False):
        dx, gw, rdx, rgw = backward(geo, x, W, ga, two_pitch, off, with_dx)
        assert torch.equal(gw, rgw) and (dx is None or torch.equal(dx, rdx)), with_dx


@pytest.mark.parametrize("geo", [GEOMETRIES[6], GEOMETRIES[8], GEOMETRIES[11]], ids=_ids)
def test_rounding_bound_on_normal_data(geo):
    n, h, w, G, ci, co, (r, s), stride, pad = geo
    gamma = lambda k: k * U32 / (1 - k * U32)  # noqa: E731
    ops = operands(geo, integer=False, seed=1)
    (x, t_x, W, V, ga), (ax, at, aw, av, ag) = ops, [t.abs() for t in ops]
    pairs = []  # (error, bound) per output
    for has_t, has_v in ((True, True), (False, True), (True, False)):
        k = 2 * r * s * ci * (has_t + has_v)
        got, ref = tangent(geo, t_x if has_t else None, x, W if has_t else None, V if has_v else None)
        _, scale = tangent(geo, at if has_t else None, ax, aw if has_t else None, av if has_v else None)
        pairs.append(((got - ref).abs(), gamma(k) * scale))
    dx, gw, rdx, rgw = backward(geo, x, W, ga)
    _, _, sdx, sgw = backward(geo, ax, aw, ag)  # (the same sums over the operands' magnitudes)
    pairs += [((dx - rdx).abs(), gamma(2 * r * s * co) * sdx), ((gw - rgw).abs(), gamma(2 * n * ga[0, 0].numel()) * sgw)]
    print(f"{geo}: tangent (both, x * V, t_x * W), dx, gw at",
          " ".join(f"{float((e / b).nan_to_num(0.0).max()):.3f}" for e, b in pairs), "of the bound")
    assert all(bool((e <= b).all()) for e, b in pairs)


@pytest.mark.parametrize("case", ["width 6", "width 68", "C_in off G * cg_in", "50 taps", "both terms NULL",
                                  "splits_w off the plan"])
def test_refused_arguments_launch_nothing(case):
    lib = _lib.load()
    assert lib.hf_gconv2d_nhwc_plan(*dims(GEOMETRIES[-1])) == 46  # (the many-slab geometry: 45 slabs of 3 units, one of 1)
    d = {"width 6": dims((1, 6, 6, 2, 6, 4, (3, 3), (1, 1), (1, 1))), "width 68": dims((1, 6, 6, 2, 4, 68, (3, 3), (1, 1), (1, 1))),
         "C_in off G * cg_in": (2, 5, 7, 9, 8, 2, 3, 3, 1, 1, 1, 1),
         "50 taps": dims((1, 12, 12, 2, 4, 4, (5, 10), (1, 1), (0, 0)))}.get(case, dims(GEOMETRIES[1]))
    n, h, w, c_in, c_out, G, r, s = d[:8]
    buf = In(np.ones(n * h * w * max(c_in, c_out) * 2 + c_out * c_in * r * s, np.float32), 0)
    out, gw = FlatOut(n * h * w * max(c_in, c_out)), FlatOut(c_out * c_in * r * s, slabs=3)
    t_x, v = (None, None) if case == "both terms NULL" else (buf.ptr, buf.ptr)
    sw = lib.hf_gconv2d_nhwc_plan(*d)
    assert sw == (2 if d == dims(GEOMETRIES[1]) else ERR_ARG)
    if case != "splits_w off the plan":
        assert lib.hf_gconv2d_nhwc_tangent(out.ptr, t_x, buf.ptr, 0, buf.ptr, v, *d, F32, st()) == ERR_ARG
    if case != "both terms NULL":
        assert lib.hf_gconv2d_nhwc_backward_slabs(out.ptr, gw.ptr, buf.ptr, buf.ptr, 0, buf.ptr, *d, max(sw, 0) + 1,
                                                  c_out * c_in * r * s, F32, st()) == ERR_ARG
    torch.cuda.synchronize()
    assert out.pristine() and gw.pristine()
