"""GPU: ``hf_gn_split_adjoint2_sums`` + ``hf_gn_split_act_adjoint2`` through the C ABI against ``gn2_refs.adjoint2``; guarded
outputs, the launch pair twice with equal bits; E[t], E[xh t] from the table ``hf_gn_split_tangent_sums`` leaves for the same t.

Bound, counted from the kernel file's chain: per element the pair does ``hf_gn_act_adjoint2``'s roundings in its order; only a
mean's source differs -- a lane's fp32 chain runs over its PART (``L = chain(part_pixels, cg)``), all behind it (lanes, waves,
parts) is fp64 with ONE rounding, T1 and Tx included.  So ``gn2_refs.r_adjoint2`` holds term by term with the part's ``L`` and
``Lr = row_chain(part_pixels, span)``; a sample's part rows are added here in float64: no rounding, the parts' bounds add."""

import pytest
import torch

import gn2_refs
import gn_refs
import guarded as gd
from layer_refs import ratio
from pytorchhessianfree_amd import _lib

pytestmark = pytest.mark.gpu
EPS = float(torch.tensor(1e-5))
# (n, h, w, c, groups, slabs), test_gn_split_kernels_gpu.py's: just over the limit at cg = 4 | 65 channel quads per pixel | two
# groups in one span, three slabs | odd pixel count, a short last part | cg = 1024.  Forms: linear and relu (a mask) with both
# vectors and every row table; bare: a mask, v_gamma = v_conv_bias = NULL, no row table
SHAPES = [(1, 64, 65, 4, 1, 1), (1, 8, 8, 260, 1, 1), (2, 40, 40, 24, 2, 3), (2, 33, 33, 64, 1, 2), (1, 5, 5, 2048, 2, 1)]
CASES = [(s, f) for s in SHAPES for f in ("linear", "relu")] + [(SHAPES[2], "bare")]


@pytest.mark.parametrize("shape, form", CASES, ids=gd._ids)
def test_adjoint2_against_float64(shape, form):
    n, h, w, c, groups, splits = shape
    hw, rows, cg, lib, relu, full = h * w, n * h * w, c // groups, _lib.load(), form != "linear", form != "bare"
    span, parts, pp = _lib.gn_split_plan(n, hw, c, groups)
    assert parts >= 2 and pp * span <= 16384
    gen = torch.Generator().manual_seed(13 * c + splits + len(form))
    rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    a, gamma, gy2, ta, g = rnd(1, n, hw, c), rnd(c), rnd(splits, n, hw, c), rnd(splits, n, hw, c), rnd(n, hw, c)
    v_cb, vg = (rnd(c), rnd(c)) if full else (None, None)
    fw = gn_refs.forward(a, None, gamma, rnd(c), EPS, groups, relu)  # statistics, map and mask as given, rounded to fp32
    a32, mean32, rstd32, y32 = fw.s.float(), fw.mean.float(), fw.rstd.float(), (fw.y.float() if relu else None)
    if relu:
        g = torch.where(y32 > 0, g, torch.zeros_like(g))
    stride = rows * c + gd.SLAB_GAP
    gy2_d, ta_d = (gd.slabs_dev(t.reshape(splits, -1), stride) for t in (gy2, ta))
    a_d, g_d, mean_d, rstd_d, y_d = (gd.dv(t) for t in (a32, g, mean32, rstd32, y32))
    gamma_i, vcb_i, vg_i = (gd.ip(None if t is None else t.numpy(), off) for t, off in ((gamma, 1), (v_cb, 3), (vg, 5)))
    given = (gd.p(a_d), gd.p(g_d), gd.p(mean_d), gd.p(rstd_d), gamma_i.ptr, gd.pp(vg_i))
    dims = (n, hw, c, groups, gd.F32, gd.st())
    t_tab, raw = gd.FlatOut(n * groups * parts * 2, dtype=torch.float64), gd.RowOut(rows, c)  # (the raw map is not used)
    assert lib.hf_gn_split_tangent_sums(raw.ptr, 0, t_tab.ptr, gd.p(ta_d), splits, stride, gd.pp(vcb_i), given[0], *given[2:4], *dims) == 0

    def launch():  # (g' goes to ga2's own buffer, which the apply launch rewrites in place)
        ga2, t_map, tab = gd.RowOut(rows, c), gd.RowOut(rows, c), gd.FlatOut(n * groups * parts * 5, dtype=torch.float64)
        gw, gb, gcb = (gd.FlatOut(n * parts * c) if full else None for _ in range(3))
        assert lib.hf_gn_split_adjoint2_sums(ga2.ptr, t_map.ptr, tab.ptr, gd.optr(gw), gd.optr(gb), gd.p(gy2_d), splits,
                                             stride, gd.p(ta_d), splits, stride, gd.pp(vcb_i), t_tab.ptr, *given, gd.p(y_d),
                                             *dims) == 0
        assert lib.hf_gn_split_act_adjoint2(ga2.ptr, gd.optr(gcb), ga2.ptr, t_map.ptr, tab.ptr, t_tab.ptr, *given, *dims) == 0
        return ga2, t_map, tab, gw, gb, gcb

    ga2, _, _, *tables = gd.twice(launch)
    ref = gn2_refs.adjoint2(gy2, ta, v_cb, a32, g, mean32, rstd32, gamma, vg, y32, groups)
    R = gn2_refs.r_adjoint2(splits, gn_refs.chain(pp, cg), gn_refs.row_chain(pp, span))
    assert ratio(ga2.val, ref.ga.reshape(rows, c), ref.Mga.reshape(rows, c), R.ga) <= 1 and t_tab.untouched()
    for got, k in zip(tables, ("gw", "gb", "gcb")):  # the sample's part rows added in float64
        assert got is None or ratio(got.val.view(n, parts, c).double().sum(1), getattr(ref, k), getattr(ref, "M" + k),
                                    getattr(R, k)) <= 1, k


def test_a_group_wider_than_the_lds_is_refused_and_nothing_is_written():
    n, hw, c, groups, lib = 1, 1, 16388, 1, _lib.load()  # cg: one quad over 16 384 floats in a single pixel
    ins = torch.zeros(c, device=gd.DEV), torch.ones(c, device=gd.DEV)
    m, v = (gd.p(t) for t in ins)
    outs = [gd.RowOut(1, c) for _ in range(5)] + [gd.FlatOut(5, dtype=torch.float64), gd.FlatOut(2, dtype=torch.float64)]
    ga2, t_map, gw, gb, gcb, tab, t_tab = (o.ptr for o in outs)
    dims = (n, hw, c, groups, gd.F32, gd.st())
    assert lib.hf_gn_split_adjoint2_sums(ga2, t_map, tab, gw, gb, m, 1, 0, m, 1, 0, v, t_tab, m, m, v, v, v, v, m, *dims) == gd.ERR_ARG
    assert lib.hf_gn_split_act_adjoint2(ga2, gcb, ga2, t_map, tab, t_tab, m, m, v, v, v, v, *dims) == gd.ERR_ARG
    torch.cuda.synchronize()
    assert all(o.pristine() for o in outs)
