"""GPU: the GroupNorm kernels of ``hf_gn.hip`` through the C ABI against the float64 references of ``gn_refs.py``, each
within the bound counted from the kernel file's arithmetic chains (derived, not measured); guarded outputs, every launch
twice with the same bits.  Per shape two forms -- without ReLU: convolution bias and its tangent, the operand's first
half, no ``v_beta``, no ``g``; with ReLU: one constant (sample, group) block (``rstd = 1/sqrt(eps)``), the second half, no
``v_gamma``, no convolution-bias rows."""

import pytest
import torch

import gn_refs
import guarded as gd
from layer_refs import ratio
from pytorchhessianfree_amd import _lib

pytestmark = pytest.mark.gpu
EPS = float(torch.tensor(1e-5))  # (exact in fp32: the kernel and the reference see the same number)
# (n, h, w, c, groups, splits): smallest, 15 pixels | cg = 8, three slabs | cg = 4, many groups per workgroup, a partial last
# span | one group of exactly 16 384 floats | one pixel
SHAPES = [(2, 3, 5, 8, 2, 1), (3, 4, 4, 24, 3, 3), (2, 7, 7, 72, 18, 2), (1, 8, 8, 256, 1, 1), (2, 1, 1, 16, 4, 1)]


def _half(rows, c, half):
    """Half ``half`` of a [rows, 2c] operand; the other half and the guards must stay untouched."""
    return gd.FlatOut(c, off=half * c, slabs=rows, stride=2 * c)


@pytest.mark.parametrize("relu", [0, 1], ids=["linear", "relu"])
@pytest.mark.parametrize("shape", SHAPES, ids=gd._ids)
def test_kernels_against_float64(shape, relu):
    n, h, w, c, groups, splits = shape
    hw, rows, cg, lib = h * w, n * h * w, c // groups, _lib.load()
    span = _lib.gn_plan(n, hw, c, groups)
    assert span % cg == 0 and cg <= span <= c and hw * span <= 16384
    L, Lr = gn_refs.chain(hw, cg), gn_refs.row_chain(hw, span)
    gen = torch.Generator().manual_seed(7 * c + splits + relu)
    rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    a, ta, gy = rnd(splits, n, hw, c), rnd(splits, n, hw, c), rnd(splits, n, hw, c)
    gamma, beta, vg, vb = rnd(c), rnd(c), (None if relu else rnd(c)), (rnd(c) if relu else None)
    cb, v_cb = (None, None) if relu else (rnd(c), rnd(c))
    if relu:  # the last sample's first group is constant (exactly, whatever the split order)
        a[:, -1, :, :cg] = 0
        a[0, -1, :, :cg] = 3.25
    stride = rows * c + gd.SLAB_GAP
    dslabs = lambda t: gd.slabs_dev(t.reshape(splits, -1), stride)  # noqa: E731
    a_d, ta_d, gy_d = dslabs(a), dslabs(ta), dslabs(gy)
    gamma_d, beta_d, cb_d, vcb_d, vg_d, vb_d = (gd.dv(t) for t in (gamma, beta, cb, v_cb, vg, vb))
    dims = (n, hw, c, groups, gd.F32, gd.st())

    def fwd():
        out = gd.RowOut(rows, c), _half(rows, c, relu), gd.RowOut(rows, c), gd.FlatOut(n * groups), gd.FlatOut(n * groups)
        y, y2, a_out, mean, rstd = out
        assert lib.hf_gn_forward(y.ptr, y2.ptr, 2 * c, a_out.ptr, mean.ptr, rstd.ptr, gd.p(a_d), splits, stride, gd.p(cb_d),
                                 gd.p(gamma_d), gd.p(beta_d), EPS, relu, *dims) == 0
        return out

    y, y2, a_out, mean, rstd = gd.twice(fwd)
    fw, R = gn_refs.forward(a, cb, gamma, beta, EPS, groups, relu), gn_refs.r_forward(splits, cb is not None, L)
    flat = lambda t: t.reshape(rows, c)  # noqa: E731
    assert ratio(a_out.val, flat(fw.s), flat(fw.Ms), R.s) <= 1
    assert ratio(mean.val, fw.mean.reshape(-1), fw.Mmean.reshape(-1), R.mean) <= 1
    assert ratio(rstd.val, fw.rstd.reshape(-1), fw.Mrstd.reshape(-1), R.rstd) <= 1
    assert ratio(y.val, flat(fw.y), flat(fw.My), R.y) <= 1 and gd.bits_equal(y.val, y2.body)
    if relu:
        assert float(rstd.val[(n - 1) * groups]) == float((1.0 / torch.tensor(EPS, dtype=torch.float64).sqrt()).float())

    # ---- tangent and adjoint: statistics, map and mask as given (the references' values, rounded to fp32) --------------
    a32, mean32, rstd32, y32 = fw.s.float(), fw.mean.float(), fw.rstd.float(), (fw.y.float() if relu else None)
    a32_d, mean_d, rstd_d, y_d = (gd.dv(t) for t in (a32, mean32, rstd32, y32))

    def tan():
        out = _half(rows, c, relu)
        assert lib.hf_gn_act_tangent(out.ptr, 2 * c, gd.p(ta_d), splits, stride, gd.p(vcb_d), gd.p(a32_d), gd.p(mean_d),
                                     gd.p(rstd_d), gd.p(gamma_d), gd.p(vg_d), gd.p(vb_d), gd.p(y_d), *dims) == 0
        return out

    want, M = gn_refs.tangent(ta, v_cb, a32, mean32, rstd32, gamma, vg, vb, y32, groups)
    assert ratio(gd.twice(tan).body, flat(want), flat(M), gn_refs.r_tangent(splits, v_cb is not None, L)) <= 1

    def adj():
        out = (gd.RowOut(rows, c), gd.RowOut(rows, c) if relu else None, gd.FlatOut(n * c), gd.FlatOut(n * c),
               None if relu else gd.FlatOut(n * c))
        assert lib.hf_gn_act_adjoint(*(gd.optr(o) for o in out), gd.p(gy_d), splits, stride, gd.p(a32_d), gd.p(mean_d),
                                     gd.p(rstd_d), gd.p(gamma_d), gd.p(y_d), *dims) == 0
        return out

    ga, g, gw, gb, gcb = gd.twice(adj)
    ad, R = gn_refs.adjoint(gy, a32, mean32, rstd32, gamma, y32, groups), gn_refs.r_adjoint(splits, L, Lr)
    assert ratio(ga.val, flat(ad.ga), flat(ad.Mga), R.ga) <= 1
    assert g is None or ratio(g.val, flat(ad.g), flat(ad.Mg), R.g) <= 1
    for got, name in ((gw, "gw"), (gb, "gb"), (gcb, "gcb")):  # per sample, and after summation over the samples
        if got is not None:
            t, wanted, Mt, r = got.val.view(n, c), getattr(ad, name), getattr(ad, "M" + name), getattr(R, name)
            assert ratio(t, wanted, Mt, r) <= 1 and ratio(t.double().sum(0), wanted.sum(0), Mt.sum(0), r) <= 1

    def sq():  # the squared rows of diag_ef, from the tables the adjoint launch left
        out = gd.FlatOut(c, off=1), gd.FlatOut(c, off=2), None if gcb is None else gd.FlatOut(c, off=3)
        assert lib.hf_gn_rows_sqsum(out[0].ptr, gw.ptr, out[1].ptr, gb.ptr, gd.optr(out[2]), gd.optr(gcb), float(n), n, c,
                                    gd.F32, gd.st()) == 0
        return out

    for got, table in zip(gd.twice(sq), (gw, gb, gcb)):
        if got is not None:
            assert ratio(got.val, *gn_refs.rows_sqsum(table.val.view(n, c), float(n)), 4) <= 1


def test_a_block_over_the_lds_limit_is_refused_and_nothing_is_written():
    n, hw, c, groups = 1, 64, 260, 1  # one quad over 16 384 floats
    lib, rows = _lib.load(), 64
    with pytest.raises(_lib.Refused):
        _lib.gn_plan(n, hw, c, groups)
    ins = [torch.zeros(rows * c, device=gd.DEV) for _ in range(2)] + [torch.ones(c, device=gd.DEV) for _ in range(3)]
    a, y_in, gamma, mean, rstd = (gd.p(t) for t in ins)
    outs = [gd.RowOut(rows, c) for _ in range(5)] + [gd.FlatOut(n * c) for _ in range(5)]
    o = [x.ptr for x in outs]
    dims = (n, hw, c, groups, gd.F32, gd.st())
    assert lib.hf_gn_forward(o[0], o[1], c, o[2], o[5], o[6], a, 1, 0, None, gamma, gamma, EPS, 1, *dims) == gd.ERR_ARG
    assert lib.hf_gn_act_tangent(o[3], 0, a, 1, 0, None, a, mean, rstd, gamma, gamma, gamma, y_in, *dims) == gd.ERR_ARG
    assert lib.hf_gn_act_adjoint(o[4], o[0], o[7], o[8], o[9], a, 1, 0, a, mean, rstd, gamma, y_in, *dims) == gd.ERR_ARG
    torch.cuda.synchronize()
    assert all(x.pristine() for x in outs)
