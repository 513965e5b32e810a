"""GPU: ``hf_gn_act_adjoint2`` through the C ABI against ``gn2_refs.py`` within the bound counted from the kernel file's chain;
guarded outputs, every launch twice with equal bits.  Linear form: ``v_conv_bias`` / ``v_gamma`` given, convolution-bias rows,
per-channel operands on odd 4-byte offsets; ReLU form: a mask, neither of the two vectors, no convolution-bias rows."""

import pytest
import torch

import gn2_refs
import gn_refs
import guarded as gd
from layer_refs import ratio
from pytorchhessianfree_amd import _lib

pytestmark = pytest.mark.gpu
EPS = float(torch.tensor(1e-5))
# (n, h, w, c, groups, splits), the layouts of test_gn_kernels_gpu.py: two teams, 15 pixels | one-wave teams, three slabs | 16
# groups per span, a partial last span | one group of exactly 16 384 floats: both blocks at the LDS limit | one pixel
SHAPES = [(2, 3, 5, 8, 2, 1), (3, 4, 4, 24, 3, 3), (2, 7, 7, 72, 18, 2), (1, 8, 8, 256, 1, 1), (2, 1, 1, 16, 4, 1)]


@pytest.mark.parametrize("relu", [0, 1], ids=["linear", "relu"])
@pytest.mark.parametrize("shape", SHAPES, ids=gd._ids)
def test_adjoint2_against_float64(shape, relu):
    n, h, w, c, groups, splits = shape
    hw, rows, cg, lib = h * w, n * h * w, c // groups, _lib.load()
    gen = torch.Generator().manual_seed(11 * c + splits + relu)
    rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    a, gamma, gy2, ta, g = rnd(1, n, hw, c), rnd(c), rnd(splits, n, hw, c), rnd(splits, n, hw, c), rnd(n, hw, c)
    v_cb, vg = (None, None) if relu else (rnd(c), rnd(c))
    fw = gn_refs.forward(a, None, gamma, rnd(c), EPS, groups, relu)  # statistics, map and mask as given, rounded to fp32
    a32, mean32, rstd32, y32 = fw.s.float(), fw.mean.float(), fw.rstd.float(), (fw.y.float() if relu else None)
    if relu:
        g = torch.where(y32 > 0, g, torch.zeros_like(g))
    stride = rows * c + gd.SLAB_GAP
    gy2_d, ta_d = (gd.slabs_dev(t.reshape(splits, -1), stride) for t in (gy2, ta))
    a_d, g_d, mean_d, rstd_d, y_d = (gd.dv(t) for t in (a32, g, mean32, rstd32, y32))
    gamma_i, vcb_i, vg_i = (gd.ip(None if t is None else t.numpy(), off) for t, off in ((gamma, 1), (v_cb, 3), (vg, 5)))

    def launch():
        out = gd.RowOut(rows, c), gd.FlatOut(n * c), gd.FlatOut(n * c), None if relu else gd.FlatOut(n * c)
        assert lib.hf_gn_act_adjoint2(*(gd.optr(o) for o in out), gd.p(gy2_d), splits, stride, gd.p(ta_d), splits, stride,
                                      gd.pp(vcb_i), gd.p(a_d), gd.p(g_d), gd.p(mean_d), gd.p(rstd_d), gamma_i.ptr,
                                      gd.pp(vg_i), gd.p(y_d), n, hw, c, groups, gd.F32, gd.st()) == 0
        return out

    ga, *tables = gd.twice(launch)
    ref = gn2_refs.adjoint2(gy2, ta, v_cb, a32, g, mean32, rstd32, gamma, vg, y32, groups)
    R = gn2_refs.r_adjoint2(splits, gn_refs.chain(hw, cg), gn_refs.row_chain(hw, _lib.gn_plan(n, hw, c, groups)))
    assert ratio(ga.val, ref.ga.reshape(rows, c), ref.Mga.reshape(rows, c), R.ga) <= 1
    for got, k in zip(tables, ("gw", "gb", "gcb")):
        assert got is None or ratio(got.val.view(n, c), getattr(ref, k), getattr(ref, "M" + k), getattr(R, k)) <= 1


def test_a_block_over_the_lds_limit_is_refused_and_nothing_is_written():
    n, hw, c, groups, lib = 1, 64, 260, 1, _lib.load()  # one quad over 16 384 floats
    m, v = torch.zeros(hw * c, device=gd.DEV), torch.ones(c, device=gd.DEV)
    outs = [gd.RowOut(hw, c)] + [gd.FlatOut(n * c) for _ in range(3)]
    assert lib.hf_gn_act_adjoint2(*(o.ptr for o in outs), gd.p(m), 1, 0, gd.p(m), 1, 0, gd.p(v), gd.p(m), gd.p(m), gd.p(v),
                                  gd.p(v), gd.p(v), gd.p(v), gd.p(m), n, hw, c, groups, gd.F32, gd.st()) == gd.ERR_ARG
    torch.cuda.synchronize()
    assert all(o.pristine() for o in outs)
