"""GPU: the split GroupNorm kernels of ``hf_gn.hip`` (a reduce and an apply launch per direction) through the C ABI against
the float64 references of ``gn_refs.py`` -- the twin of ``test_gn_kernels_gpu.py``, on blocks beyond one workgroup's LDS.
Guarded outputs, every launch pair twice with the same bits; the same two operand forms per shape.

Bounds, counted from the kernel file's "Split family" chains (derived, not measured).  The longest fp32 chain is a PART's:
``L = chain(part_pixels, cg)`` in a group reduction, ``Lr = row_chain(part_pixels, span)`` down the pixels; the
combination over the parts is fp64 and adds no rounding.  With ``r_s = splits - 1 [+ 1]``:
  mean   r_s + L + 1                               (as one launch: the chain, then one rounding)
  rstd   (2 (r_s + 1) + 1 + L) + 2 (r_s + L + 1)   within the parts: d = s - c_i (c_i is a number both launches know exactly:
                                                   it adds no error), the square, the chain | between the parts: the
                                                   square of S_i / n_i - m, each r_s + L, + m's
  y      rstd + 3
  tangent, ga, g, rows: ``gn_refs.r_tangent`` / ``r_adjoint`` with the part's L and Lr (the same chains per element)
  squared rows   6: the row's rounding and t (each twice through the square), the square, the store
The test prints the largest ratio seen per quantity."""

import pytest
import torch

import gn_refs
import guarded as gd
from layer_refs import ratio
from pytorchhessianfree_amd import _lib

pytestmark = pytest.mark.gpu
EPS = float(torch.tensor(1e-5))  # (exact in fp32: the kernel and the reference see the same number)
# (n, h, w, c, groups, splits): one pixel over the limit at cg = 4, a ragged last part | 65 channel quads per pixel | two
# groups in one span, three slabs | GroupNorm(1, 64), odd pixel count, many parts | cg = 1024, parts capped by 25 pixels
SHAPES = [(1, 64, 65, 4, 1, 1), (1, 8, 8, 260, 1, 1), (2, 40, 40, 24, 2, 3), (2, 33, 33, 64, 1, 2), (1, 5, 5, 2048, 2, 1)]
_worst = {}  # the largest ratio seen per quantity (printed; a single rounding, as a_out's, comes close to 1 by itself)


def _r(name, *a):
    _worst[name] = max(_worst.get(name, 0.0), v := ratio(*a))
    return v


_half = lambda rows, c, half: gd.FlatOut(c, off=half * c, slabs=rows, stride=2 * c)  # noqa: E731  (a half of [rows, 2c])


@pytest.mark.parametrize("relu", [0, 1], ids=["linear", "relu"])
@pytest.mark.parametrize("shape", SHAPES, ids=gd._ids)
def test_kernels_against_float64(shape, relu):
    n, h, w, c, groups, splits = shape
    hw, rows, cg, lib = h * w, n * h * w, c // groups, _lib.load()
    span, parts, pp = _lib.gn_split_plan(n, hw, c, groups)
    assert pp * span <= 16384 and parts == -(-hw // pp) >= 2 and span % cg == 0 and cg <= span <= c
    L, Lr = gn_refs.chain(pp, cg), gn_refs.row_chain(pp, span)
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
    tab = lambda: gd.FlatOut(n * groups * parts * 2, dtype=torch.float64)  # noqa: E731

    def fwd():
        out = (gd.RowOut(rows, c), _half(rows, c, relu), gd.RowOut(rows, c), gd.FlatOut(n * groups), gd.FlatOut(n * groups),
               tab())
        y, y2, a_out, mean, rstd, t = out
        assert lib.hf_gn_split_stats(a_out.ptr, t.ptr, gd.p(a_d), splits, stride, gd.p(cb_d), *dims) == 0
        assert lib.hf_gn_split_forward(y.ptr, y2.ptr, 2 * c, mean.ptr, rstd.ptr, a_out.ptr, t.ptr, gd.p(gamma_d),
                                       gd.p(beta_d), EPS, relu, *dims) == 0
        return out

    y, y2, a_out, mean, rstd, _ = gd.twice(fwd)
    fw, r_s = gn_refs.forward(a, cb, gamma, beta, EPS, groups, relu), splits - 1 + int(cb is not None)
    r_rstd = (2 * (r_s + 1) + 1 + L) + 2 * (r_s + L + 1)
    flat = lambda t: t.reshape(rows, c)  # noqa: E731
    assert _r("a_out", a_out.val, flat(fw.s), flat(fw.Ms), r_s) <= 1
    assert _r("mean", mean.val, fw.mean.reshape(-1), fw.Mmean.reshape(-1), r_s + L + 1) <= 1
    assert _r("rstd", rstd.val, fw.rstd.reshape(-1), fw.Mrstd.reshape(-1), r_rstd) <= 1
    assert _r("y", y.val, flat(fw.y), flat(fw.My), r_rstd + 3) <= 1 and gd.bits_equal(y.val, y2.body)
    if relu:
        assert float(rstd.val[(n - 1) * groups]) == float((1.0 / torch.tensor(EPS, dtype=torch.float64).sqrt()).float())

    # ---- tangent and adjoint: statistics, map and mask as given (the references' values, rounded to fp32) --------------
    a32, mean32, rstd32, y32 = fw.s.float(), fw.mean.float(), fw.rstd.float(), (fw.y.float() if relu else None)
    a32_d, mean_d, rstd_d, y_d = (gd.dv(t) for t in (a32, mean32, rstd32, y32))

    def tan():
        out, t = _half(rows, c, relu), tab()
        assert lib.hf_gn_split_tangent_sums(out.ptr, 2 * c, t.ptr, gd.p(ta_d), splits, stride, gd.p(vcb_d), gd.p(a32_d),
                                            gd.p(mean_d), gd.p(rstd_d), *dims) == 0
        assert lib.hf_gn_split_act_tangent(out.ptr, 2 * c, t.ptr, gd.p(a32_d), gd.p(mean_d), gd.p(rstd_d), gd.p(gamma_d),
                                           gd.p(vg_d), gd.p(vb_d), gd.p(y_d), *dims) == 0
        return out, t

    want, M = gn_refs.tangent(ta, v_cb, a32, mean32, rstd32, gamma, vg, vb, y32, groups)
    assert _r("tangent", gd.twice(tan)[0].body, flat(want), flat(M), gn_refs.r_tangent(splits, v_cb is not None, L)) <= 1

    def adj():  # (without ReLU no separate g: the masked cotangent goes to ga, which the apply launch rewrites in place)
        out = (gd.RowOut(rows, c), gd.RowOut(rows, c) if relu else None, gd.FlatOut(n * parts * c),
               gd.FlatOut(n * parts * c), None if relu else gd.FlatOut(n * parts * c), tab())
        ga, g, gw, gb, gcb, t = out
        g_ptr = (g or ga).ptr
        assert lib.hf_gn_split_adjoint_sums(g_ptr, t.ptr, gw.ptr, gb.ptr, gd.p(gy_d), splits, stride, gd.p(a32_d),
                                            gd.p(mean_d), gd.p(rstd_d), gd.p(gamma_d), gd.p(y_d), *dims) == 0
        assert lib.hf_gn_split_act_adjoint(ga.ptr, gd.optr(gcb), g_ptr, t.ptr, gd.p(a32_d), gd.p(mean_d), gd.p(rstd_d),
                                           gd.p(gamma_d), *dims) == 0
        return out

    ga, g, gw, gb, gcb, _ = gd.twice(adj)
    ad, R = gn_refs.adjoint(gy, a32, mean32, rstd32, gamma, y32, groups), gn_refs.r_adjoint(splits, L, Lr)
    assert _r("ga", ga.val, flat(ad.ga), flat(ad.Mga), R.ga) <= 1
    assert g is None or _r("g", g.val, flat(ad.g), flat(ad.Mg), R.g) <= 1
    for got, name in ((gw, "gw"), (gb, "gb"), (gcb, "gcb")):  # the parts added per sample, and then over the samples
        if got is not None:
            t, wanted, Mt, r = got.val.view(n, parts, c).double().sum(1), getattr(ad, name), getattr(ad, "M" + name), getattr(R, name)
            assert _r(name, t, wanted, Mt, r) <= 1 and _r(name, t.sum(0), wanted.sum(0), Mt.sum(0), r) <= 1

    def sq():  # the squared rows of diag_ef, from the tables the adjoint launches left
        out = gd.FlatOut(c, off=1), gd.FlatOut(c, off=2), None if gcb is None else gd.FlatOut(c, off=3)
        assert lib.hf_gn_split_rows_sqsum(out[0].ptr, gw.ptr, out[1].ptr, gb.ptr, gd.optr(out[2]), gd.optr(gcb), float(n),
                                          n, parts, c, gd.F32, gd.st()) == 0
        return out

    for got, table in zip(gd.twice(sq), (gw, gb, gcb)):
        if got is not None:
            want = ((float(n) * table.val.view(n, parts, c).double().sum(1)) ** 2).sum(0)
            assert _r("sqsum", got.val, want, want, 6) <= 1
    print("largest ratios so far:", " ".join(f"{k} {v:.3f}" for k, v in _worst.items()))


def test_a_group_wider_than_the_lds_is_refused_and_nothing_is_written():
    n, hw, c, groups = 1, 1, 16388, 1  # one quad over 16 384 floats in a single pixel
    with pytest.raises(_lib.Refused):
        _lib.gn_split_plan(n, hw, c, groups)
    ins = [torch.zeros(c, device=gd.DEV) for _ in range(2)] + [torch.ones(c, device=gd.DEV) for _ in range(3)]
    a, y_in, gamma, mean, rstd = (gd.p(t) for t in ins)
    outs = [gd.RowOut(1, c) for _ in range(10)] + [gd.FlatOut(2, dtype=torch.float64) for _ in range(3)]
    o, lib = [x.ptr for x in outs], _lib.load()
    dims, E = (n, hw, c, groups, gd.F32, gd.st()), gd.ERR_ARG
    assert lib.hf_gn_split_stats(o[0], o[10], a, 1, 0, None, *dims) == E
    assert lib.hf_gn_split_forward(o[1], o[2], c, o[3], o[4], a, o[10], gamma, gamma, EPS, 1, *dims) == E
    assert lib.hf_gn_split_tangent_sums(o[5], 0, o[11], a, 1, 0, None, a, mean, rstd, *dims) == E
    assert lib.hf_gn_split_act_tangent(o[5], 0, o[11], a, mean, rstd, gamma, gamma, gamma, y_in, *dims) == E
    assert lib.hf_gn_split_adjoint_sums(o[6], o[12], o[7], o[8], a, 1, 0, a, mean, rstd, gamma, y_in, *dims) == E
    assert lib.hf_gn_split_act_adjoint(o[6], o[9], o[6], o[12], a, mean, rstd, gamma, *dims) == E
    torch.cuda.synchronize()
    assert all(x.pristine() for x in outs)
