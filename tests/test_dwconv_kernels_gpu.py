"""GPU: the depthwise kernels (hf_dwconv.hip) against ``F.conv2d(..., groups=c)`` and its autograd in float64 (CPU), in
guarded buffers, every launch twice.  Integer data: exact.  Normal data: ``|got - ref| <= gamma_K * sum |a_i b_i|``."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from guarded import ERR_ARG, F32, FlatOut, In, P, U32, _ids, st, twice
from pytorchhessianfree_amd import _lib

pytestmark = pytest.mark.gpu

CB, TILE = 32, 8  # hf_dwconv.hip: most channels per workgroup, tile edge
GEOMETRIES = [  # (n, h, w, c, (r, s), stride, pad)
    (1, 1, 1, 4, (1, 1), (1, 1), (0, 0)),
    (2, 5, 7, 4, (3, 3), (1, 1), (1, 1)),
    (2, 9, 6, 12, (3, 3), (2, 2), (1, 1)),
    (1, 2, 2, 8, (3, 3), (1, 1), (1, 1)),      # a map smaller than the kernel
    (2, 6, 6, 8, (3, 3), (1, 1), (0, 0)),
    (2, 6, 10, 8, (3, 1), (1, 1), (1, 0)),
    (3, 8, 8, CB + 4, (3, 3), (2, 1), (1, 1)),  # two channel blocks, the second one quad wide
    (2, 11, 11, 8, (5, 5), (1, 1), (2, 2)),
    (1, 9, 9, 4, (7, 7), (1, 1), (3, 3)),
    (34, TILE + 1, TILE + 1, 4, (3, 3), (1, 1), (1, 1)),  # 2 x 2 tiles per sample: 136 units in 46 slabs of 3, the last of 1
]
FORMS = [(False, True, True), (True, True, True), (False, False, True), (True, True, False)]  # (t_x, W, V): forward (V = W) ..
dims = lambda g: (*g[:4], *g[4], *g[5], *g[6])  # noqa: E731  (n, h, w, c, r, s, stride_h, stride_w, pad_h, pad_w)
nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().float().numpy()  # noqa: E731


def operands(geo, integer, seed=0):
    """x, t_x [n, c, h, w], W, V [c, 1, r, s], ga [n, c, oh, ow] in float64 (float32 draws, widened)."""
    n, h, w, c, (r, s), stride, pad = geo
    g = torch.Generator().manual_seed(seed)
    oh, ow = (h + 2 * pad[0] - r) // stride[0] + 1, (w + 2 * pad[1] - s) // stride[1] + 1
    draw = (lambda sh: torch.randint(-4, 5, sh, generator=g)) if integer else (lambda sh: torch.randn(sh, generator=g))
    return [draw(sh).double() for sh in [(n, c, h, w), (n, c, h, w), (c, 1, r, s), (c, 1, r, s), (n, c, oh, ow)]]


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
    c, stride, pad = geo[3], geo[5], geo[6]
    ref = sum(F.conv2d(a, m, None, stride, pad, 1, c) for a, m in ((t_x, W), (x, V)) if a is not None and m is not None)
    ptx, px, ld, keep = acts(t_x if W is not None else None, x if V is not None else None, c, two_pitch, off)
    wi, vi = (None if m is None else In(m.float().numpy(), off) for m in (W, V))

    def launch():
        out = FlatOut(ref.numel(), off=off, shape=tuple(ref.permute(0, 2, 3, 1).shape))
        assert _lib.load().hf_dwconv2d_nhwc_tangent(out.ptr, ptx, px, ld, None if wi is None else wi.ptr,
                                                    None if vi is None else vi.ptr, *dims(geo), F32, st()) == 0
        return out
    return twice(launch).val.cpu().double().permute(0, 3, 1, 2), ref


def backward(geo, x, W, ga, two_pitch=False, off=0, with_dx=True):
    """The launch (twice): (dx or None, the slabs summed in float64), and their float64 values by autograd."""
    n, h, w, c, (r, s), stride, pad = geo
    x64, w64 = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    rdx, rgw = torch.autograd.grad(F.conv2d(x64, w64, None, stride, pad, 1, c), (x64, w64), ga)
    _, px, ld, keep = acts(None, x, c, two_pitch, off)
    gi, wi, sw = In(nhwc(ga), off), In(W.float().numpy(), off), _lib.load().hf_dwconv2d_nhwc_plan(*dims(geo))

    def launch():
        dx = FlatOut(x.numel(), off=off, shape=tuple(x.permute(0, 2, 3, 1).shape)) if with_dx else None
        gw = FlatOut(c * r * s, off=off, slabs=sw, stride=c * r * s + 20)
        assert _lib.load().hf_dwconv2d_nhwc_backward_slabs(None if dx is None else dx.ptr, gw.ptr, gi.ptr, px, ld,
                                                           wi.ptr if with_dx else None, *dims(geo), sw, gw.stride, F32,
                                                           st()) == 0
        return dx, gw
    dx, gw = twice(launch)
    got_dx = None if dx is None else dx.val.cpu().double().permute(0, 3, 1, 2)
    return got_dx, gw.body.cpu().double().sum(0).view(c, 1, r, s), rdx, rgw


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "elementwise"])
@pytest.mark.parametrize("two_pitch", [False, True], ids=["pitch-c", "pitch-2c"])
@pytest.mark.parametrize("geo", GEOMETRIES, ids=_ids)
def test_exact_on_integers(geo, two_pitch, off):
    x, t_x, W, V, ga = operands(geo, integer=True)
    for i, (has_t, has_w, has_v) in enumerate(FORMS):
        got, ref = tangent(geo, t_x if has_t else None, x, W if has_w and has_t else None,
                           (W if i == 0 else V) if has_v else None, two_pitch, off)
        assert torch.equal(got, ref), i
    for with_dx in (True, False):
        dx, gw, rdx, rgw = backward(geo, x, W, ga, two_pitch, off, with_dx)
        assert torch.equal(gw, rgw) and (dx is None or torch.equal(dx, rdx)), with_dx


@pytest.mark.parametrize("geo", [GEOMETRIES[2], GEOMETRIES[8], GEOMETRIES[9]], ids=_ids)
def test_rounding_bound_on_normal_data(geo):
    n, h, w, c, (r, s), stride, pad = geo
    gamma = lambda k: k * U32 / (1 - k * U32)  # noqa: E731
    ops = operands(geo, integer=False, seed=1)
    (x, t_x, W, V, ga), (ax, at, aw, av, ag) = ops, [t.abs() for t in ops]
    for has_t, has_v, k in ((True, True, 2 * r * s), (False, True, r * s), (True, False, r * s)):
        got, ref = tangent(geo, t_x if has_t else None, x, W if has_t else None, V if has_v else None)
        _, scale = tangent(geo, at if has_t else None, ax, aw if has_t else None, av if has_v else None)
        assert bool(((got - ref).abs() <= gamma(k) * scale).all())
    dx, gw, rdx, rgw = backward(geo, x, W, ga)
    _, _, sdx, sgw = backward(geo, ax, aw, ag)  # (the same sums over the operands' magnitudes)
    k_w = n * ga.shape[2] * ga.shape[3]
    print(f"{geo}: dx {float(((dx - rdx).abs() / (gamma(r * s) * sdx)).max()):.3f}, "
          f"gw {float(((gw - rgw).abs() / (gamma(k_w) * sgw)).max()):.3f} of the bound")
    assert bool(((dx - rdx).abs() <= gamma(r * s) * sdx).all()) and bool(((gw - rgw).abs() <= gamma(k_w) * sgw).all())


@pytest.mark.parametrize("case", ["c % 4", "50 taps", "both terms NULL", "splits_w off the plan"])
def test_refused_arguments_launch_nothing(case):
    lib = _lib.load()
    assert lib.hf_dwconv2d_nhwc_plan(*dims(GEOMETRIES[-1])) == 46  # (the many-slab geometry: 45 slabs of 3 units, one of 1)
    geo = {"c % 4": (1, 6, 6, 6, (3, 3), (1, 1), (1, 1)), "50 taps": (1, 12, 12, 4, (5, 10), (1, 1), (0, 0))}.get(
        case, GEOMETRIES[1])
    n, h, w, c, (r, s), stride, pad = geo
    buf = In(np.ones(n * h * w * c * 2 + c * r * s, np.float32), 0)
    out, gw = FlatOut(n * h * w * c), FlatOut(c * r * s, slabs=3)
    t_x, v = (None, None) if case == "both terms NULL" else (buf.ptr, buf.ptr)
    sw = lib.hf_dwconv2d_nhwc_plan(*dims(geo))
    assert sw == (2 if geo is GEOMETRIES[1] else ERR_ARG)
    if case != "splits_w off the plan":
        assert lib.hf_dwconv2d_nhwc_tangent(out.ptr, t_x, buf.ptr, 0, buf.ptr, v, *dims(geo), F32, st()) == ERR_ARG
    if case != "both terms NULL":
        assert lib.hf_dwconv2d_nhwc_backward_slabs(out.ptr, gw.ptr, buf.ptr, buf.ptr, 0, buf.ptr, *dims(geo), max(sw, 0) + 1,
                                                   c * r * s, F32, st()) == ERR_ARG
    torch.cuda.synchronize()
    assert out.pristine() and gw.pristine()
