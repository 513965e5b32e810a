"""CPU: the float64 references of ``layer_refs`` are anchored to something independent (autograd, ``F.batch_norm``,
ATen's max-pool), and the error bound the kernel tests use is shown to be HONEST (an fp32 evaluation of the header's
formula, in the documented order, lies inside it on the very inputs the GPU tests use) and to DISCRIMINATE (wrong
variants of that evaluation -- a slab dropped, ``mask_src >= 0``, the neighbouring channel's statistics, the second
cotangent added behind the mask, a count off by one -- each violate it)."""

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
