"""CPU: the float64 references of ``layer_refs`` are anchored to something independent (autograd, ``F.batch_norm``,
ATen's max-pool), and the error bound the kernel tests use is shown to be HONEST (an fp32 evaluation of the header's
formula, in the documented order, lies inside it on the very inputs the GPU tests use) and to DISCRIMINATE (wrong
variants of that evaluation -- a slab dropped, ``mask_src >= 0``, the neighbouring channel's statistics, the second
cotangent added behind the mask, a count off by one -- each violate it)."""

from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layer_refs as L
from layer_refs import U32

dt = torch.float64


def _r(gen, *s):
    return torch.randn(*s, generator=gen, dtype=dt)


# ---------------------------------------------------------------------------------------------------------------
# anchors
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True])
def test_eval_batchnorm_references_match_autograd(relu):
    gen = torch.Generator().manual_seed(1)
    n, c, hw, eps = 6, 5, 7, 1e-5
    x = _r(gen, n, hw, c).requires_grad_()
    rm, rv = _r(gen, c), _r(gen, c).abs() + 0.3
    w, b = _r(gen, c).requires_grad_(), _r(gen, c).requires_grad_()
    res = _r(gen, n, hw, c).requires_grad_()
    rstd = (rv + eps).rsqrt()
    z = F.batch_norm(x.permute(0, 2, 1), rm, rv, w, b, False, 0.0, eps).permute(0, 2, 1) + res
    y = torch.relu(z) if relu else z
    # forward: q = w, r = b, add = res
    got, _ = L.chan_affine(None, x, rm, rstd, None, w, b, res, None, relu_self=relu)
    assert float((got - y).abs().max()) < 1e-13
    fw = L.bn_forward(x.detach()[None], rm, rstd, w, b, res, relu)
    assert float((fw.y - y).abs().max()) < 1e-13 and torch.equal(fw.s, x.detach())
    # adjoint: two cotangents, the mask source is the layer's own output
    gy, gy2 = _r(gen, 2, n, hw, c), _r(gen, 1, n, hw, c)
    gx, gw, gb, gres = torch.autograd.grad(y, (x, w, b, res), gy.sum(0) + gy2.sum(0))
    bw = L.chan_affine_bwd(gy, gy2, x, rm, rstd, w, y if relu else None)
    for got, want in ((bw.gx, gx), (bw.g, gres)):
        assert float((got - want.reshape(-1, c)).abs().max()) < 1e-13
    assert float((bw.col(bw.gwe) - gw).abs().max()) < 1e-12 and float((bw.col(bw.g) - gb).abs().max()) < 1e-12
    pre = L.bn_adjoint_pre(gy, gy2, y if relu else None, w, rstd)
    assert float((pre.ga - gx.reshape(-1, c)).abs().max()) < 1e-13 and torch.equal(pre.g, bw.g)
    # tangent of the map (a = tangent of x, q = tangent of w, r = tangent of b, add = tangent of res, masked by y)
    tx, tw, tb, tr = _r(gen, n, hw, c), _r(gen, c), _r(gen, c), _r(gen, n, hw, c)
    _, jvp = torch.func.jvp(
        lambda x_, w_, b_, r_: (lambda z_: torch.relu(z_) if relu else z_)(
            F.batch_norm(x_.permute(0, 2, 1), rm, rv, w_, b_, False, 0.0, eps).permute(0, 2, 1) + r_),
        (x.detach(), w.detach(), b.detach(), res.detach()), (tx, tw, tb, tr))
    got, _ = L.chan_affine(tx[None], x, rm, rstd, w, tw, tb, tr, y if relu else None)
    assert float((got - jvp).abs().max()) < 1e-13


def test_train_batchnorm_tangent_reference_matches_jvp():
    gen = torch.Generator().manual_seed(2)
    rows, c, eps = 29, 6, 1e-5
    a, w, b = _r(gen, rows, c) * 2 + 0.5, _r(gen, c), _r(gen, c)
    t, vq, vr, add = _r(gen, 3, rows, c), _r(gen, c), _r(gen, c), _r(gen, rows, c)

    def f(a_, w_, b_):
        return F.batch_norm(a_.t()[None], None, None, w_, b_, True, 0.0, eps)[0].t()

    z, jvp = torch.func.jvp(f, (a, w, b), (t.sum(0), vq, vr))
    mean, rstd = a.mean(0), (a.var(0, unbiased=False) + eps).rsqrt()
    # the reduction launch's partial rows (gx = NULL form of hf_chan_affine_bwd_ex), 4 row shares
    red = L.chan_affine_bwd(t, None, a, mean, rstd, None, None)
    px = torch.stack([red.col(red.gwe, lo, hi) for lo, hi in L.row_shares(rows, 4)])
    p1 = torch.stack([red.col(red.g, lo, hi) for lo, hi in L.row_shares(rows, 4)])
    got, _ = L.chan_affine_train(t, a, mean, rstd, w, px, p1, vq, vr, float(rows), add, z)
    want = torch.where(z > 0, jvp + add, torch.zeros_like(jvp))
    assert float((got - want).abs().max()) < 1e-12
    # the adjoint's use (vq = vr = NULL): the same operator is self-adjoint on the xhat part
    gy = _r(gen, 1, rows, c)
    (ga,) = torch.autograd.grad(f(a.requires_grad_(), w, b), a, gy[0])
    red = L.chan_affine_bwd(gy, None, a.detach(), mean, rstd, None, None)
    got, _ = L.chan_affine_train(gy, a.detach(), mean, rstd, w, red.col(red.gwe)[None], red.col(red.g)[None], None,
                                 None, float(rows), None, None)
    assert float((got - ga).abs().max()) < 1e-12


@pytest.mark.parametrize("rows,c,sp", [(37, 8, 1), (32, 12, 3)])
def test_train_hessian_references_match_double_backward(rows, c, sp):
    pr = L.train_hessian_problem(rows, c, sp)
    xh, r, m = pr.xh, pr.r, float(rows)
    cf = L.train_hessian_coeffs(*(e.sum(0, keepdim=True) for e in (pr.dg_z * xh, pr.dg_z, r * pr.g_z * pr.da,
                                                                     pr.da * xh, pr.da)),
                                pr.gg, pr.gb, pr.gam, pr.dgam, r, m)
    got = cf.coef[0] * pr.ga + cf.coef[1] * pr.g_z + cf.coef[2] * pr.dg_z + cf.coef[3] * pr.da + cf.coef[4] * xh + \
        cf.coef[5]
    assert float((got - pr.want_a).abs().max()) < 1e-11
    dgg = (pr.dg_z * xh).sum(0) + (r * pr.g_z * pr.da).sum(0) + cf.corr
    assert float((dgg - pr.want_g).abs().max()) < 1e-11 and float((pr.dg_z.sum(0) - pr.want_b).abs().max()) < 1e-11
    assert bool((cf.Mcoef >= cf.coef.abs() * (1 - 1e-12)).all()) and bool((cf.Mcorr >= cf.corr.abs() * (1 - 1e-12)).all())
    out, M = L.train_hessian_apply(pr.ga, pr.g_z, pr.dg_z, pr.t, pr.a, pr.a.double().mean(0), r, cf.coef)
    assert float((out - pr.want_a).abs().max()) < 1e-11 and bool((M >= out.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("geom", L.POOL_GEOMS, ids=str)
def test_maxpool_reference_matches_aten(geom):
    n, c, h, w, kh, kw, sh, sw, ph, pw = geom
    x = L.maxpool_input(geom)
    val, idx = L.maxpool_forward(x, kh, kw, sh, sw, ph, pw)
    want, widx = F.max_pool2d(x, (kh, kw), (sh, sw), (ph, pw), return_indices=True)
    assert torch.equal(idx, widx) and torch.equal(torch.nan_to_num(val, nan=7.0), torch.nan_to_num(want, nan=7.0))
    assert bool(torch.isnan(val).any()) and bool(torch.isinf(x).any())
    # ties are frequent: many windows hold their maximum more than once
    cols = F.unfold(torch.nan_to_num(x, nan=-1e30, neginf=-1e30), (kh, kw), 1, (ph, pw), (sh, sw))
    cols = cols.view(n, c, kh * kw, -1)
    assert int(((cols == cols.max(2, keepdim=True).values).sum(2) > 1).sum()) > cols.shape[-1] * n * c // 20


@pytest.mark.parametrize("n,hw,k", L.HEAD_SHAPES)
def test_head_references_match_autograd_hvp(n, hw, k):
    gen = torch.Generator().manual_seed(n + hw + k)
    feat, v = _r(gen, n, hw, k).requires_grad_(), _r(gen, n, hw, k)
    target = torch.randint(0, k, (n,), generator=gen)
    logits = feat.mean(1)
    (g,) = torch.autograd.grad(F.cross_entropy(logits, target), feat, create_graph=True)
    (hv,) = torch.autograd.grad((g * v).sum(), feat)
    p = torch.softmax(logits.detach(), 1)
    ref = L.pool_ce_head(v, p, 1.0 / n)
    assert float((ref.g - hv).abs().max()) < 1e-14 and float((ref.jv - v.mean(1)).abs().max()) < 1e-14
    out, _ = L.softmax_ce_hvp(p, v.mean(1), 1.0 / n)
    assert float((out[:, None, :] / hw - hv).abs().max()) < 1e-14
    if L.LD_OK:
        out_ld, _ = L.softmax_ce_hvp(p, v.mean(1), 1.0 / n, ld=True)
        assert float(np.abs(out_ld - out.numpy()).max()) < 1e-15


def test_conv_references_are_autograd():
    gen = torch.Generator().manual_seed(5)
    x, w, gy = _r(gen, 2, 4, 5, 5), _r(gen, 8, 4, 3, 3), _r(gen, 2, 8, 3, 3)
    y, gx, gw = L.conv_refs(x, w, gy, (2, 2), (1, 1))
    assert torch.equal(y, F.conv2d(x, w, None, 2, 1))
    eps = 1e-6
    d = _r(gen, *x.shape)
    num = ((F.conv2d(x + eps * d, w, None, 2, 1) - F.conv2d(x - eps * d, w, None, 2, 1)) * gy).sum() / (2 * eps)
    assert abs(float(num - (gx * d).sum())) < 1e-6 * float(gx.abs().sum())


def test_planner_never_asks_for_an_empty_row_share():
    """``engine/buffers.py`` ends its choice with ``rb = ceil(rows / per)``; ``hf_chan_affine_bwd_ex`` then gives
    every workgroup ``ceil(rows / rb)`` rows and refuses counts whose last share would start behind the end."""
    for rows in list(range(1, 300)) + [1568, 6272, 32768]:
        for per in {1, 2, 3, 5, 8, 21, 64, 100, rows}:
            rb = -(-rows // per)
            assert L.share_ok(rows, rb), (rows, per, rb)
    assert not L.share_ok(37, 63) and L.share_ok(37, 37) and not L.share_ok(5, 4)


# ---------------------------------------------------------------------------------------------------------------
# fp32 evaluations of the header's formulas (torch on the CPU rounds every operation to fp32), with wrong variants
# ---------------------------------------------------------------------------------------------------------------
def _ssum(a, mut=""):
    n = a.shape[0] - (1 if mut == "drop_slab" else 0)
    s = a[0].clone()
    for i in range(1, n):
        s = s + a[i]
    return s if not (mut == "drop_slab" and a.shape[0] == 1) else s * 0


def _nb(v, mut):
    return v.roll(1) if (mut == "neighbour" and v is not None) else v


def _keep(mask, mut):
    return mask >= 0 if mut == "mask_ge" else mask > 0


def emu_chan_affine(a, x, mean, rstd, w, q, r, add, mask, relu_self, mut=""):
    mean, rstd = _nb(mean, mut), _nb(rstd, mut)
    acc = None
    if a is not None:
        acc = _ssum(a, mut) * ((w if w is not None else 1.0) * (rstd if rstd is not None else 1.0))
    if q is not None:
        t = ((x - mean) * rstd) * q
        acc = t if acc is None else acc + t
    for term in (r, add):
        if term is not None:
            acc = term.expand_as(add if add is not None else mask).clone() if acc is None else acc + term
    if relu_self:
        return torch.relu(acc)
    return torch.where(_keep(mask, mut), acc, torch.zeros_like(acc)) if mask is not None else acc


def emu_bwd(gy, gy2, x, mean, rstd, w, mask, mut=""):
    mean, rstd = _nb(mean, mut), _nb(rstd, mut)
    g = _ssum(gy, mut)
    h = _ssum(gy2) if gy2 is not None else None
    if mut == "gy2_after_mask" and h is not None and mask is not None:
        g = torch.where(mask > 0, g, torch.zeros_like(g)) + h
    else:
        if h is not None:
            g = g + h
        if mask is not None:
            g = torch.where(_keep(mask, mut), g, torch.zeros_like(g))
    gx = g * ((w if w is not None else 1.0) * (rstd if rstd is not None else 1.0))
    gwe = None
    if x is not None:
        xh = (x - (mean if mean is not None else 0.0)) * (rstd if rstd is not None else 1.0)
        gwe = g.double() * xh.double()
    return g, gx, gwe


def emu_bn_forward(a, mean, rstd, w, b, res, relu, mut=""):
    mean, rstd = _nb(mean, mut), _nb(rstd, mut)
    t = _ssum(a, mut)
    if rstd is not None:
        t = ((t - mean) * rstd) * w
    if b is not None:
        t = t + b
    if mut == "res_after_relu":
        return torch.relu(t) + res
    if res is not None:
        t = t + res
    return torch.relu(t) if relu else t


def emu_train(a, x, mean, rstd, w, px, p1, vq, vr, count, add, mask, mut=""):
    if mut == "count":
        count = count - 1.0
    inv = torch.tensor(1.0 / count, dtype=torch.float32)
    k = w * rstd * inv
    q = (vq if vq is not None else 0.0) - k * px.double().sum(0).float()
    r = (vr if vr is not None else 0.0) - k * p1.double().sum(0).float()
    return emu_chan_affine(a, x, mean, rstd, w, q, r, add, mask, 0, mut)


def emu_hessian_apply(ga1, gz1, gz2, t, a, mean, rstd, coef, mut=""):
    k = coef.roll(1, 1) if mut == "neighbour" else coef
    if mut == "swap":
        k = coef[[0, 2, 1, 3, 4, 5]]
    xh = (a - mean) * rstd
    return ((k[0] * ga1 + k[1] * gz1) + (k[2] * gz2 + k[3] * _ssum(t, mut))) + (k[4] * xh + k[5])


def emu_softmax(p, v, scale, mut=""):
    pv = p.double() * v.double()
    if mut == "drop_col":
        pv = torch.cat([pv[:, :pv.shape[1] // 2], pv[:, pv.shape[1] // 2 + 1:]], 1)  # (one term of the dot product lost)
    d = pv.sum(1, keepdim=True).to(p.dtype)
    if mut == "neighbour":
        d = d.roll(1, 0)
    if mut == "no_centre":
        d = d * 0
    sc = torch.tensor(scale * (1.5 if mut == "scale" else 1.0), dtype=p.dtype)
    return sc * (p * (v - d))


def emu_pool_head(t, p, scale, mut=""):
    hw = t.shape[1]
    s = t[:, 0].clone()
    for i in range(1, hw - (1 if mut == "drop_pixel" else 0)):
        s = s + t[:, i]
    jv = s / torch.tensor(float(hw + (1 if mut == "count" else 0)), dtype=torch.float32)
    pp = p.roll(1, 1) if mut == "neighbour" else p
    d = (pp.double() * jv.double()).sum(1, keepdim=True).float()
    h = (torch.tensor(scale, dtype=torch.float32) * (pp * (jv - d))) / float(hw)
    return jv, h[:, None, :].expand_as(t)


def _col_ratio(elem64, want_e, M_e, R):
    """fp64 column sum of an fp32-rounded term, stored with one rounding, against the float64 reference"""
    return L.ratio(elem64.sum(0).float(), want_e.sum(0), M_e.sum(0), R)


CASES = L.eval_cases()


@pytest.mark.parametrize("shape,slabs,i", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_fp32_evaluation_of_the_eval_forms_is_inside_the_bound(shape, slabs, i):
    """chan_affine, chan_affine_bwd, bn_adjoint_pre, bn_forward on the GPU tests' inputs."""
    (rows, c), (s1, s2) = shape, slabs
    o = L.eval_inputs(rows, c, s1, s2)
    v = L.AFFINE_VARIANTS[i % len(L.AFFINE_VARIANTS)]
    drop = tuple(d for d in v.drop if not (d == "a" and s1 > 1))
    a, x, mean, rstd, w, q, r, add, mask = L.pick(o, ("a", "x", "mean", "rstd", "w", "q", "r", "add", "mask"), drop)
    want, M = L.chan_affine(a, x, mean, rstd, w, q, r, add, mask, v.relu_self)
    R = L.r_chan_affine(s1, a is not None, q is not None, r is not None, add is not None)
    got = emu_chan_affine(a, x, mean, rstd, w, q, r, add, mask if mask is not None else None, v.relu_self)
    assert L.ratio(got, want, M, R) <= 1.0
    if not v.relu_self and mask is not None:
        assert bool((got[~(mask > 0)] == 0).all())

    bv = L.BWD_VARIANTS[i % len(L.BWD_VARIANTS)]
    x, mean, rstd, w, mask = L.pick(o, ("x", "mean", "rstd", "w", "mask"), bv.drop)
    ref = L.chan_affine_bwd(o.a, o.b, x, mean, rstd, w, mask)
    g, gx, gwe = emu_bwd(o.a, o.b, x, mean, rstd, w, mask)
    assert L.ratio(g, ref.g, ref.Mg, L.r_bwd_g(s1, s2)) <= 1.0
    assert L.ratio(gx, ref.gx, ref.Mgx, L.r_bwd_gx(s1, s2)) <= 1.0
    assert _col_ratio(g.double(), ref.g, ref.Mg, L.r_bwd_gb(s1, s2)) <= 1.0
    if gwe is not None:
        assert _col_ratio(gwe, ref.gwe, ref.Mgwe, L.r_bwd_gw(s1, s2)) <= 1.0

    fw = L.bn_forward(o.a, o.mean, o.rstd, o.w, o.r, o.add, 1)
    assert L.ratio(emu_bn_forward(o.a, o.mean, o.rstd, o.w, o.r, o.add, 1), fw.y, fw.My,
                   L.r_bn_forward(s1, True, True, True)) <= 1.0


MUT_CASES = [((200, 96), (3, 1)), ((37, 12), (9, 2)), ((130, 260), (2, 17)), ((3, 20), (8, 1))]


@pytest.mark.parametrize("shape,slabs", MUT_CASES, ids=str)
def test_wrong_variants_of_the_eval_forms_violate_the_bound(shape, slabs):
    (rows, c), (s1, s2) = shape, slabs
    o = L.eval_inputs(rows, c, s1, s2)
    want, M = L.chan_affine(o.a, o.x, o.mean, o.rstd, o.w, o.q, o.r, o.add, o.mask)
    R = L.r_chan_affine(s1, True, True, True, True)
    for mut in ("drop_slab", "mask_ge", "neighbour"):
        got = emu_chan_affine(o.a, o.x, o.mean, o.rstd, o.w, o.q, o.r, o.add, o.mask, 0, mut)
        assert L.ratio(got, want, M, R) > 1.0, mut
    ref = L.chan_affine_bwd(o.a, o.b, o.x, o.mean, o.rstd, o.w, o.mask)
    for mut in ("drop_slab", "mask_ge", "neighbour", "gy2_after_mask"):
        g, gx, gwe = emu_bwd(o.a, o.b, o.x, o.mean, o.rstd, o.w, o.mask, mut)
        worst = max(L.ratio(g, ref.g, ref.Mg, L.r_bwd_g(s1, s2)), L.ratio(gx, ref.gx, ref.Mgx, L.r_bwd_gx(s1, s2)),
                    _col_ratio(gwe, ref.gwe, ref.Mgwe, L.r_bwd_gw(s1, s2)),
                    _col_ratio(g.double(), ref.g, ref.Mg, L.r_bwd_gb(s1, s2)))
        assert worst > 1.0, mut
        if mut != "neighbour":  # (the elementwise adjoint pre-pass reads no statistics but rstd)
            pre = L.bn_adjoint_pre(o.a, o.b, o.mask, o.w, o.rstd)
            assert L.ratio(g, pre.g, pre.Mg, L.r_bwd_g(s1, s2)) > 1.0, mut
    # a row attributed to the neighbouring share cancels in the total but not in the single partial rows
    g, _, gwe = emu_bwd(o.a, o.b, o.x, o.mean, o.rstd, o.w, o.mask)
    (lo, hi) = L.row_shares(rows, 2)[0]
    assert bool((o.mask[hi] > 0).any())  # (the misplaced row carries something)
    assert L.ratio(g.double()[lo:hi + 1].sum(0).float(), ref.col(ref.g, lo, hi), ref.col(ref.Mg, lo, hi),
                   L.r_bwd_gb(s1, s2)) > 1.0
    fw = L.bn_forward(o.a, o.mean, o.rstd, o.w, o.r, o.add, 1)
    for mut in ("drop_slab", "neighbour", "res_after_relu"):
        got = emu_bn_forward(o.a, o.mean, o.rstd, o.w, o.r, o.add, 1, mut)
        assert L.ratio(got, fw.y, fw.My, L.r_bn_forward(s1, True, True, True)) > 1.0, mut


@pytest.mark.parametrize("rows,c,splits,nparts", L.TRAIN_CASES)
def test_fp32_evaluation_of_the_train_forms_and_its_wrong_variants(rows, c, splits, nparts):
    o = L.train_inputs(rows, c, splits, nparts)
    want, M = L.chan_affine_train(o.a, o.x, o.mean, o.rstd, o.w, o.px, o.p1, o.q, o.r, float(rows), o.add, o.mask)
    R = L.r_chan_affine_train(splits, True)
    args = (o.a, o.x, o.mean, o.rstd, o.w, o.px, o.p1, o.q, o.r, float(rows), o.add, o.mask)
    assert L.ratio(emu_train(*args), want, M, R) <= 1.0
    for mut in ("count", "mask_ge", "neighbour") + (("drop_slab",) if splits > 1 else ()):
        assert L.ratio(emu_train(*args, mut=mut), want, M, R) > 1.0, mut


@pytest.mark.parametrize("rows,c,sp", [(37, 8, 1), (128, 256, 3), (1568, 64, 9), (32, 12, 3)])
def test_fp32_evaluation_of_the_train_hessian_apply_and_its_wrong_variants(rows, c, sp):
    pr = L.train_hessian_problem(rows, c, sp)
    gen = L.gen_of("coef", rows, c)
    coef = L.randn(gen, 6, c)
    ops = (pr.ga.float(), pr.g_z.float(), pr.dg_z.float(), pr.t, pr.a, pr.mean, pr.rstd, coef)
    want, M = L.train_hessian_apply(*ops)
    R = L.r_train_hessian_apply(sp)
    assert L.ratio(emu_hessian_apply(*ops), want, M, R) <= 1.0
    for mut in ("neighbour", "swap") + (("drop_slab",) if sp > 1 else ("neighbour",)):
        assert L.ratio(emu_hessian_apply(*ops, mut=mut), want, M, R) > 1.0, mut


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("rows", [1, 33])
@pytest.mark.parametrize("cols", [1, 10, 257, 1000])
def test_fp32_evaluation_of_the_softmax_hessian_and_its_wrong_variants(dtype, rows, cols):
    f64 = dtype == torch.float64
    if f64 and not L.LD_OK:
        pytest.skip("numpy.longdouble is no wider than float64 on this machine")
    p, v = L.softmax_inputs(rows, cols, dtype)
    want, M = L.softmax_ce_hvp(p, v, 1.0 / rows, ld=f64)
    R, u = L.r_softmax_ce_hvp(cols, f64), (L.U64 if f64 else U32)
    assert L.ratio(emu_softmax(p, v, 1.0 / rows), want, M, R, u) <= 1.0
    # (one column: p = 1 and the result is identically zero, whatever the scale)
    muts = ("no_centre",) + (("scale", "drop_col") if cols > 1 else ()) + (("neighbour",) if rows > 1 else ())
    for mut in muts:
        assert L.ratio(emu_softmax(p, v, 1.0 / rows, mut), want, M, R, u) > 1.0, mut


@pytest.mark.parametrize("n,hw,k", L.HEAD_SHAPES)
def test_fp32_evaluation_of_the_pool_head_and_its_wrong_variants(n, hw, k):
    t, p = L.head_inputs(n, hw, k)
    ref = L.pool_ce_head(t, p, 1.0 / n)
    rj, rg = L.r_pool_ce_head(hw)
    jv, g = emu_pool_head(t, p, 1.0 / n)
    assert L.ratio(jv, ref.jv, ref.Mjv, rj) <= 1.0 and L.ratio(g, ref.g, ref.Mg, rg) <= 1.0
    for mut in ("count", "neighbour") + (("drop_pixel",) if hw > 1 else ()):
        jv, g = emu_pool_head(t, p, 1.0 / n, mut)
        assert max(L.ratio(jv, ref.jv, ref.Mjv, rj), L.ratio(g, ref.g, ref.Mg, rg)) > 1.0, mut


@pytest.mark.skipif(not L.LD_OK, reason="numpy.longdouble is no wider than float64 on this machine")
def test_longdouble_references_agree_with_float64_ones():
    o = L.eval_inputs(37, 12, 9, 2, dtype=torch.float64)
    w64, M = L.chan_affine(o.a, o.x, o.mean, o.rstd, o.w, o.q, o.r, o.add, o.mask)
    wld, Mld = L.chan_affine(o.a, o.x, o.mean, o.rstd, o.w, o.q, o.r, o.add, o.mask, ld=True)
    assert L.ratio(w64, wld, Mld, L.r_chan_affine(9, True, True, True, True), L.U64) <= 1.0
    b64, bld = L.chan_affine_bwd(o.a, o.b, o.x, o.mean, o.rstd, o.w, o.mask), \
        L.chan_affine_bwd(o.a, o.b, o.x, o.mean, o.rstd, o.w, o.mask, ld=True)
    assert L.ratio(b64.gx, bld.gx, bld.Mgx, L.r_bwd_gx(9, 2), L.U64) <= 1.0


# ---------------------------------------------------------------------------------------------------------------
# train-mode BatchNorm forward (hf_bn_stats_rows, hf_bn_forward_train) and the linear head (hf_linear_ce_head)
# ---------------------------------------------------------------------------------------------------------------
f32, f64 = np.float32, np.float64


@pytest.mark.parametrize("relu,res", [(0, 0), (1, 1), (0, 1)])
def test_train_batchnorm_forward_reference_matches_batch_norm(relu, res):
    """``bn_stats`` + ``bn_forward_train`` = ``F.batch_norm(training=True)`` in float64, the moved running statistics
    (unbiased variance) included, with residual and ReLU."""
    gen = torch.Generator().manual_seed(11 + relu)
    rows, c, splits, rb = 29, 8, 3, 4
    a = torch.randn(splits, rows, c, generator=gen)
    w, b, rm = (torch.randn(c, generator=gen) for _ in range(3))
    rv, r_ = torch.randn(c, generator=gen).abs() + 0.5, (torch.randn(rows, c, generator=gen) if res else None)
    st = L.bn_stats(a, rb)
    assert torch.equal(st.s, (a[0] + a[1]) + a[2])
    ref = L.bn_forward_train(st.s, torch.from_numpy(st.part.astype(f64)), rows, 1e-5, 0.1, w, b, r_, relu, rm, rv)
    rm64, rv64 = rm.double().clone(), rv.double().clone()
    want = F.batch_norm(st.s.double().t()[None], rm64, rv64, w.double(), b.double(), True, 0.1, 1e-5)[0].t()
    if res:
        want = want + r_.double()
    want = torch.relu(want) if relu else want
    s64 = st.s.double()
    for got, exp in ((ref.y, want), (ref.rm, rm64), (ref.rv, rv64), (ref.mean, s64.mean(0)),
                     (ref.rstd, (s64.var(0, unbiased=False) + 1e-5).rsqrt())):
        assert float(np.abs(got.astype(f64) - exp.numpy()).max()) < 1e-12
    assert float(np.abs((st.part[:, 0].sum(0) / rows).astype(f64) - s64.mean(0).numpy()).max()) < 1e-14


@pytest.mark.parametrize("rows,features,classes,bias", [(5, 8, 3, 1), (9, 12, 7, 0)])
def test_linear_head_reference_matches_autograd(rows, features, classes, bias):
    """``linear_ce_head`` = J^T H_L J v of ``cross_entropy(linear(feat))`` with respect to (feat, weight, bias), each
    factor by float64 autograd: J v by forward mode, H_L by double backward through the loss, J^T by a vjp.  (The
    full Hessian of the composition adds the terms of the bilinear map's own second derivative; the engine adds those
    outside this kernel.)  The per-workgroup slabs add up to the weight and bias gradients."""
    gen = torch.Generator().manual_seed(rows + classes)
    feat, w = _r(gen, rows, features).requires_grad_(), _r(gen, classes, features).requires_grad_()
    b = _r(gen, classes).requires_grad_()
    t_feat, v_w, v_b = _r(gen, rows, features), _r(gen, classes, features), _r(gen, classes)
    if not bias:
        v_b = v_b * 0
    target = torch.randint(0, classes, (rows,), generator=gen)
    logits = F.linear(feat, w, b)
    _, jv = torch.func.jvp(F.linear, (feat.detach(), w.detach(), b.detach()), (t_feat, v_w, v_b))
    z = logits.detach().requires_grad_()
    (gz,) = torch.autograd.grad(F.cross_entropy(z, target), z, create_graph=True)
    (hjv,) = torch.autograd.grad((gz * jv).sum(), z)
    g_feat, g_w, g_b = torch.autograd.grad(logits, (feat, w, b), hjv)
    ref = L.linear_ce_head(t_feat, feat.detach(), w.detach(), v_w, v_b if bias else None,
                           torch.softmax(logits.detach(), 1), 1.0 / rows)
    assert ref.g_w.shape[0] == -(-rows // 4)
    for got, want in ((ref.jv, jv), (ref.h, hjv), (ref.g_feat, g_feat), (ref.g_w.sum(0), g_w), (ref.g_b.sum(0), g_b)):
        assert float((got - want).abs().max()) < 1e-13
    for M, v in ((ref.Mjv, ref.jv), (ref.Mh, ref.h), (ref.Mg_feat, ref.g_feat), (ref.Mg_w, ref.g_w), (ref.Mg_b, ref.g_b)):
        assert bool((M >= v.abs() * (1 - 1e-12)).all())


def emu_bn_stats(a, row_blocks, mut=""):
    """fp32 slab additions in split order, then per share sequential fp64 sums of s and s*s (as one thread would)."""
    s = L.f32_slab_sum(a, a.shape[0] - 1 if mut == "drop_slab" else None).numpy()
    acc_t = f32 if mut == "f32_acc" else f64
    shares = L.row_shares(s.shape[0], row_blocks)
    if mut == "neighbour_row":   # the first row of share 1 is added to share 0
        (l0, h0), (l1, h1) = shares[0], shares[1]
        shares = [(l0, h0 + 1), (l1 + 1, h1)] + shares[2:]
    part = np.zeros((row_blocks, 2, s.shape[1]), f64)
    for i, (lo, hi) in enumerate(shares):
        a1, a2 = np.zeros(s.shape[1], acc_t), np.zeros(s.shape[1], acc_t)
        for r in range(lo, hi):
            v = s[r].astype(acc_t)
            a1 = a1 + v
            a2 = a2 + ((s[r] * s[r]).astype(acc_t) if mut == "sq_after_round" else v * v)
        part[i, 0], part[i, 1] = a1, a2
    return torch.from_numpy(s), part


def _stats_muts(rows, c, splits, rb):
    """the wrong variants that are not the identity on this case"""
    per = -(-rows // rb)
    return ("f32_acc", "sq_after_round") + (("drop_slab",) if splits > 1 else ()) + \
        (("neighbour_row",) if rb > 1 and rows > per else ())


STATS = L.stats_cases()
_ids = lambda v: str(v).replace(" ", "")  # noqa: E731


@pytest.mark.parametrize("rows,c,splits,rb,form", STATS, ids=_ids)
def test_fp32_evaluation_of_the_batch_statistics_and_its_wrong_variants(rows, c, splits, rb, form):
    a = L.stats_inputs(rows, c, splits)
    ref = L.bn_stats(a, rb)
    s, part = emu_bn_stats(a, rb)
    assert torch.equal(s, ref.s) and bool((s[:, 0] == L.CONST_VALUE).all())
    assert L.ratio_rows(part, ref.part, ref.Mpart, ref.R) <= 1.0
    for i, (lo, hi) in enumerate(L.row_shares(rows, rb)):
        if lo >= hi:
            assert not ref.part[i].any() and not ref.Mpart[i].any()   # an empty share: exact zeros, bound zero
    for mut in _stats_muts(rows, c, splits, rb):
        s, part = emu_bn_stats(a, rb, mut)
        assert L.ratio_rows(part, ref.part, ref.Mpart, ref.R) > 1.0, mut
        assert torch.equal(s, ref.s) == (mut != "drop_slab")   # (a_out is compared bitwise)
    if rb > 1 and rows > -(-rows // rb):  # the misplaced row cancels in the total: only the single rows show it
        _, part = emu_bn_stats(a, rb, "neighbour_row")
        tot, Mt = ref.part.sum(0), ref.Mpart.sum(0)
        assert L.ratio(part.sum(0), tot, Mt, rows) <= 1.0


def emu_bn_forward_train(o, count, eps, momentum, b, res, relu, rm, rv, mut=""):
    """The kernel's arithmetic in numpy: partial rows added in fp64, mean / var / rstd in fp64 with eps and momentum
    rounded to fp32 first, one rounding to fp32 each, then y in fp32."""
    part = o.part.numpy()
    if mut == "drop_part":
        part = part[1:]
    if mut == "f32_sums":
        S = part.astype(f32)[0].copy()
        for i in range(1, part.shape[0]):
            S = S + part.astype(f32)[i]
        S = S.astype(f64)
    else:
        S = np.zeros_like(part[0])
        for i in range(part.shape[0]):
            S = S + part[i]
    count = f64(count)
    m = S[0] / count
    var = np.maximum(S[1] / count - m * m, 0.0)
    e = 0.0 if mut == "no_eps" else f64(f32(eps))
    unb = var * count / (count - 1.0) if count > 1.0 else var
    with np.errstate(divide="ignore"):
        mf, rf = m.astype(f32), (1.0 / np.sqrt((unb if mut == "unbiased_rstd" else var) + e)).astype(f32)
    out = NS(mean=mf, rstd=rf, rm=None, rv=None)
    if momentum is not None and momentum >= 0 and rm is not None:
        mo = f64(f32(momentum))
        k_old, k_new = (mo, 1.0 - mo) if mut == "swap_momentum" else (1.0 - mo, mo)
        out.rm = (k_old * rm.numpy().astype(f64) + k_new * mf.astype(f64)).astype(f32)
        out.rv = (k_old * rv.numpy().astype(f64) + k_new * (var if mut == "biased_running" else unb)).astype(f32)
    with np.errstate(invalid="ignore"):  # (no_eps: 0 * inf in the constant channel)
        t = ((o.s.numpy() - mf) * rf) * o.w.numpy()
    if b is not None:
        t = t + b.numpy()
    if mut == "res_after_relu":
        t = np.maximum(t, f32(0)) + res.numpy()
    else:
        if res is not None:
            t = t + res.numpy()
        if relu:
            t = np.maximum(t, f32(0))
    assert t.dtype == f32
    out.y = t
    return out


def fwd_worst(got, ref, R):
    """worst value/bound per result of the forward (the GPU test asserts each on its own)"""
    w = {"mean": L.ratio(got.mean, ref.mean, L.mixed(ref.Mmean, R.mean[0], ref.Mmean, R.mean[1]), 1),
         "rstd": L.ratio(got.rstd, ref.rstd, L.mixed(ref.Mrstd, R.rstd[0], ref.Mrstd64, R.rstd[1]), 1),
         "y": L.ratio(got.y, ref.y, L.mixed(ref.My, R.y[0], ref.My64, R.y[1]), 1)}
    if got.rm is not None:
        w["rm"] = L.ratio(got.rm, ref.rm, L.mixed(ref.Mrm, R.rm[0], ref.Mrm, R.rm[1]), 1)
        w["rv"] = L.ratio(got.rv, ref.rv, L.mixed(ref.Mrv, R.rv[0], ref.Mrv64, R.rv[1]), 1)
    return w


def _fwd_muts(rows, nparts, f):
    moved = f.stat == "move"
    return ("no_eps", "f32_sums") + (("unbiased_rstd",) if rows > 1 else ()) + \
        (("biased_running",) if moved and rows > 1 else ()) + (("swap_momentum",) if moved else ()) + \
        (("drop_part",) if nparts > 1 else ()) + (("res_after_relu",) if f.relu and f.res != "none" else ())


FWD = L.fwd_cases()


@pytest.mark.parametrize("rows,c,nparts,i", FWD, ids=_ids)
def test_fp32_evaluation_of_the_train_forward_and_its_wrong_variants(rows, c, nparts, i):
    o, f = L.train_fwd_inputs(rows, c, nparts), L.fwd_form(i)
    b, res = (o.b if f.b else None), (o.res if f.res != "none" else None)
    mom = L.BN_MOMENTUM if f.stat != "neg" else -1.0
    rm, rv = (o.rm, o.rv) if f.stat != "null" else (None, None)
    args = (float(rows), L.BN_EPS, mom, b, res, f.relu, rm, rv)
    ref = L.bn_forward_train(o.s, o.part, float(rows), L.BN_EPS, mom, o.w, b, res, f.relu, rm, rv)
    R = L.r_bn_forward_train(nparts, f.b, res is not None)
    got = emu_bn_forward_train(o, *args)
    worst = fwd_worst(got, ref, R)
    assert max(worst.values()) <= 1.0, worst
    assert (f.stat == "move") == ("rm" in worst)
    # the constant channel: var clamps to 0, a - mean is exactly 0 and y is exactly b + res
    assert float(ref.var[0]) == 0.0 and float(got.mean[0]) == L.CONST_VALUE
    exact = f32(b[0].item() if f.b else 0.0) + (res[:, 0].numpy() if res is not None else np.zeros(rows, f32))
    assert np.array_equal(got.y[:, 0], np.maximum(exact, 0) if f.relu else exact)
    for mut in _fwd_muts(rows, nparts, f):
        w = fwd_worst(emu_bn_forward_train(o, *args, mut=mut), ref, R)
        assert max(w.values()) > 1.0, (mut, w)
    # and the fault must show in the result it belongs to
    if rows > 1 and f.stat == "move":
        assert fwd_worst(emu_bn_forward_train(o, *args, mut="biased_running"), ref, R)["rv"] > 1.0
        assert fwd_worst(emu_bn_forward_train(o, *args, mut="swap_momentum"), ref, R)["rm"] > 1.0
    if rows > 1:
        assert fwd_worst(emu_bn_forward_train(o, *args, mut="f32_sums"), ref, R)["rstd"] > 1.0


def _fma(a, b, c):
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def emu_linear_head(o, mut=""):
    """k_linear_ce_head in numpy, thread by thread: lane l of a row's wave holds the float4 chunks l, l + 64, ...; two
    interleaved fma chains, their sum, a six-step butterfly, the bias; <p, Jv> in fp64; h; g_feat by sequential fmas
    over the classes; the slabs from the workgroup's four rows (zeros for rows past the end)."""
    rows, F_, K = o.rows, o.features, o.classes
    ch = L.head_chunks(F_)
    pad = 256 * ch - F_

    def lanes(t):  # [n, F] -> [n, CH, 64, 4]
        return np.pad(t.numpy(), ((0, 0), (0, pad))).reshape(t.shape[0], ch, 64, 4)

    W, V = (o.v_w, o.w) if mut == "swap_w" else (o.w, o.v_w)
    tf, ff, w4, v4 = lanes(o.t_feat)[:, None], lanes(o.feat)[:, None], lanes(W)[None], lanes(V)[None]
    p0 = p1 = np.zeros((rows, K, 64), f32)
    for u in range(ch):
        p0, p1 = _fma(tf[:, :, u, :, 0], w4[:, :, u, :, 0], p0), _fma(tf[:, :, u, :, 1], w4[:, :, u, :, 1], p1)
        p0, p1 = _fma(tf[:, :, u, :, 2], w4[:, :, u, :, 2], p0), _fma(tf[:, :, u, :, 3], w4[:, :, u, :, 3], p1)
        p0, p1 = _fma(ff[:, :, u, :, 0], v4[:, :, u, :, 0], p0), _fma(ff[:, :, u, :, 1], v4[:, :, u, :, 1], p1)
        p0, p1 = _fma(ff[:, :, u, :, 2], v4[:, :, u, :, 2], p0), _fma(ff[:, :, u, :, 3], v4[:, :, u, :, 3], p1)
    part = p0 + p1
    for off in (32, 16, 8, 4, 2, 1):
        part = part + part[..., np.arange(64) ^ off]
    jv = part[..., 0]
    if o.v_b is not None and mut != "no_bias":
        jv = jv + o.v_b.numpy()
    p = o.p.numpy()
    pj = p.astype(f64) * jv.astype(f64)
    if mut == "drop_class":
        pj = np.delete(pj, K // 2, 1)
    d = pj.sum(1, keepdims=True).astype(f32)
    sc = f32(1.0 if mut == "no_scale" else o.scale)
    h = sc * (p * (jv - d))
    assert h.dtype == f32
    wn = W.numpy()
    gf = np.zeros((rows, F_), f32)
    for k in range(K):
        gf = _fma(h[:, k:k + 1], wn[k][None], gf)
    groups = -(-rows // 4)
    hp = np.zeros((groups * 4, K), f32)
    fp = np.zeros((groups * 4, F_), f32)
    hp[:rows], fp[:rows] = h, o.feat.numpy()
    if mut == "tail_fill":   # the last workgroup's missing rows filled with the row before them
        for r in range(rows, groups * 4):
            hp[r], fp[r] = hp[r - 1], fp[r - 1]
    if mut == "neighbour_slab":  # row 4 is credited to workgroup 0, row 3 to workgroup 1
        hp[[3, 4]], fp[[3, 4]] = hp[[4, 3]], fp[[4, 3]]
    hg, fg = hp.reshape(groups, 4, K), fp.reshape(groups, 4, F_)
    gw, gb = np.zeros((groups, K, F_), f32), np.zeros((groups, K), f32)
    for r in range(4):
        gw = _fma(hg[:, r, :, None], fg[:, r, None, :], gw)
        gb = gb + hg[:, r]
    return NS(jv=jv, h=h, g_feat=gf, g_w=gw, g_b=gb)


def head_worst(got, ref, R):
    w = {k: L.ratio(torch.from_numpy(getattr(got, k)), getattr(ref, k), getattr(ref, "M" + k), getattr(R, k))
         for k in ("g_feat", "g_w", "g_b")}
    w["sum_w"] = L.ratio(torch.from_numpy(got.g_w.astype(f64).sum(0)), ref.g_w.sum(0), ref.Mg_w.sum(0), R.g_w)
    w["sum_b"] = L.ratio(torch.from_numpy(got.g_b.astype(f64).sum(0)), ref.g_b.sum(0), ref.Mg_b.sum(0), R.g_b)
    return w


def _head_muts(rows, features, classes, bias):
    if classes == 1:  # p = 1: Jv - <p, Jv> = 0 exactly, every output is zero whatever else is wrong
        return ()
    return ("drop_class", "swap_w") + (("no_bias",) if bias else ()) + (("no_scale",) if rows > 1 else ()) + \
        (("neighbour_slab",) if rows > 4 else ()) + (("tail_fill",) if rows % 4 else ())


@pytest.mark.parametrize("rows,features,classes,bias", L.LIN_HEAD_CASES, ids=_ids)
def test_fp32_evaluation_of_the_linear_head_and_its_wrong_variants(rows, features, classes, bias):
    o = L.linear_head_inputs(rows, features, classes, bias)
    ref = L.linear_ce_head(o.t_feat, o.feat, o.w, o.v_w, o.v_b, o.p, o.scale)
    R = L.r_linear_ce_head(features, classes, bias)
    got = emu_linear_head(o)
    assert L.ratio(torch.from_numpy(got.jv), ref.jv, ref.Mjv, R.jv) <= 1.0
    assert L.ratio(torch.from_numpy(got.h), ref.h, ref.Mh, R.h) <= 1.0
    worst = head_worst(got, ref, R)
    assert max(worst.values()) <= 1.0, worst
    if classes == 1:
        assert not got.h.any() and not got.g_feat.any() and not got.g_w.any() and not got.g_b.any()
    for mut in _head_muts(rows, features, classes, bias):
        w = head_worst(emu_linear_head(o, mut), ref, R)
        assert max(w.values()) > 1.0, (mut, w)
        if mut in ("neighbour_slab", "tail_fill"):
            assert w["g_w"] > 1.0 and w["g_b"] > 1.0, (mut, w)
    if rows > 4:  # a row in the neighbouring slab cancels in the sum of the slabs: only the single slabs show it
        w = head_worst(emu_linear_head(o, "neighbour_slab"), ref, R)
        assert w["sum_w"] <= 1.0 and w["sum_b"] <= 1.0 and w["g_feat"] <= 1.0


def test_case_tables_reach_every_branch_of_the_three_kernels():
    """Mirrors of the kernels' thread maps (``layer_refs.stats_map`` / ``fwd_map`` / ``head_map``) on the case tables."""
    sm = [(L.stats_map(r, c, s, rb), r, c, s, rb, L.STATS_FORMS[f]) for r, c, s, rb, f in STATS]
    assert {m.quads for m, *_ in sm} == {1, 3, 24, 64, 256}
    assert {m.idle for m, *_ in sm} == {0, 1, 16}              # c = 12: 85 row groups of 3 quads; c = 96: 10 of 24
    assert {m.RP for m, *_ in sm} >= {256, 1}
    for c in (4, 12, 96, 256):  # (c = 4 takes 256 rows per pass: no table row has more)
        assert any(m.short for m, r, c_, *_ in sm if c_ == c)
        assert c == 4 or any(m.several_passes for m, r, c_, *_ in sm if c_ == c)
    assert any(m.several_passes for m, r, c_, *_ in sm if c_ == 1024)
    assert all(any(m.empty for m, r, c_, *_ in sm if c_ == c) for c in (4, 12, 96, 256, 1024))
    assert {s for _, _, _, s, _, _ in sm} == set(L.STATS_SPLITS)
    assert {(m.slab_passes, m.partial_batch) for m, *_ in sm} >= {(0, False), (1, True), (1, False), (2, False), (3, True),
                                                                  (5, True)}
    for s in L.STATS_SPLITS:
        forms = [f for _, _, _, s_, _, f in sm if s_ == s]
        assert {f.a_out for f in forms} == {0, 1} and {f.gap for f in forms} == {0, 1} and {f.tail for f in forms} == {0, 1}
    for c in (4, 12, 96, 256, 1024):
        assert {f.a_out for _, _, c_, _, _, f in sm if c_ == c} == {0, 1}

    fm = [(L.fwd_map(r, c, n), r, c, n, L.fwd_form(i)) for r, c, n, i in FWD]
    assert {m.lanes for m, *_ in fm} == {4, 12, 64, 96, 256} and {m.G for m, *_ in fm} == {64, 21, 4, 2, 1}
    assert {m.col_passes for m, *_ in fm} == {1, 4} and {m.idle for m, *_ in fm} == {0, 4, 64}
    for c in L.FWD_C:  # nparts on both sides of one 4*G batch, and nparts == 1, for every c
        mine = [(m, n) for m, _, c_, n, _ in fm if c_ == c]
        assert {m.batches > 1 for m, _ in mine} == {False, True} and any(n == 1 for _, n in mine)
        assert any(n == 257 for _, n in mine) and any(m.partial for m, _ in mine)
    assert any(m.have_false and m.wgs > 1 for m, *_ in fm) and any(m.have_false and m.wgs == 1 for m, *_ in fm)
    assert any(not m.have_false for m, *_ in fm) and any(m.groups_without_rows for m, *_ in fm)
    forms = [f for *_, f in fm]
    assert {f.out for f in forms} == set(L.FWD_OUT) and {f.res for f in forms} == set(L.FWD_RES)
    assert {f.stat for f in forms} == set(L.FWD_STAT) and {f.b for f in forms} == {True, False}
    assert {f.relu for f in forms} == {0, 1} and any(r == 1 for _, r, *_ in fm)
    assert {(f.out, f.res) for f in forms} >= {("y2", "strided"), ("y", "none"), ("both", "dense")}
    assert any(f.relu and f.res != "none" for f in forms) and any(f.stat == "move" and not f.b for f in forms)

    hm = [(L.head_map(r, f, k), r, f, k, b) for r, f, k, b in L.LIN_HEAD_CASES]
    assert {m.CH for m, *_ in hm} == {1, 2} and any(m.CH == 2 and m.last_chunk_lanes == 1 for m, *_ in hm)
    assert any(m.CH == 2 and m.last_chunk_lanes == 64 for m, *_ in hm) and any(m.CH == 1 and m.last_chunk_lanes == 1 for m, *_ in hm)
    assert any(m.all_lanes_hold_a_class and m.clamped for m, *_ in hm)
    assert {m.clamped for m, *_ in hm} >= {0, 1, 4} and any(k == 1 for _, _, _, k, _ in hm)      # 5 | 6 = 5 + 1 | 4, 64 = 65 - 1
    assert {m.last_rows for m, *_ in hm} == {1, 2, 3, 4} and any(m.groups > 1 and m.last_rows < 4 for m, *_ in hm)
    assert sorted(m.lds for m, *_ in hm)[-2:] == [61648, 64384] and all(m.lds <= 65536 for m, *_ in hm)
    assert all(L.head_shape_ok_ref(r, f, k) for _, r, f, k, _ in hm) and {b for *_, b in hm} == {0, 1}
    for r, f, k in ((1, 124, 64), (1, 512, 14), (0, 4, 1), (4097, 4, 1), (1, 4, 65), (1, 2, 1), (1, 6, 1), (1, 516, 1)):
        assert not L.head_shape_ok_ref(r, f, k)
