"""High-precision references of the curvature engine's LAYER kernels (``hf_bn.hip`` / ``hf_head.hip``), written from
the formulas in ``include/hf_pcg.h``, and the error bounds the kernel tests hold them to.  Plain module, no GPU.

Every reference takes the operands as given (fp32 inputs are converted exactly), computes in float64 -- or in
``numpy.longdouble`` with ``ld=True``, for the kernels' HF_F64 instantiations -- and returns, next to each result, its
per-element MAGNITUDE SUM ``M``: the same formula with every term replaced by its absolute value.  The bound of a
comparison is the standard forward bound ``R * u * M`` (``u`` = 2**-24 resp. 2**-53, ``R`` = the number of roundings
on the longest path to the element, counted from the header's formula by the ``r_*`` functions below).

Layout convention: the channel is the LAST axis of every activation-shaped operand (NHWC rows; an NCHW test permutes),
per-channel vectors are 1-D, slab operands carry the slab index as their FIRST axis and are summed here.

The second half of the module generates the kernel tests' inputs on the CPU from seeds, so that the CPU tests of the
references (``test_layer_refs_cpu.py``) and the GPU tests of the kernels (``test_layer_kernels_gpu.py``) see the same
numbers."""

from types import SimpleNamespace as NS

import numpy as np
import torch

U32, U64 = 2.0 ** -24, 2.0 ** -53
LD_EPS = float(np.finfo(np.longdouble).eps)
LD_OK = LD_EPS < 2.0 ** -60  # a longdouble that is no better than float64 cannot referee the HF_F64 kernels


# ---- small array helpers (torch float64 or numpy longdouble) ---------------------------------------------------
def up(t, ld=False):
    if t is None:
        return None
    if ld:
        return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).astype(np.longdouble)
    return t.detach().double()


def _where(m, t):
    if isinstance(t, np.ndarray):
        return np.where(m, t, np.zeros_like(t))
    return torch.where(m, t, torch.zeros_like(t))


def ratio(got, want, M, R, u=U32):
    """max over the elements of |got - want| / (R*u*M); where the bound is zero the element must be exact."""
    ld = isinstance(want, np.ndarray)
    got = up(got, ld)
    if ld:
        err, bound = np.abs(got - want), R * np.longdouble(u) * np.broadcast_to(M, want.shape)
        bad = (bound == 0) & (err > 0)
        if not np.isfinite(err).all() or bad.any():
            return float("inf")
        nz = bound > 0
        return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
    want = want.to(got.device)
    err, bound = (got - want).abs(), (R * u * M.to(got.device)).expand_as(want)
    if not bool(torch.isfinite(err).all()) or bool(((bound == 0) & (err > 0)).any()):
        return float("inf")
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0


def slab_sum(a):
    return a.sum(0), abs(a).sum(0)


# ---- eval-mode BatchNorm forms -----------------------------------------------------------------------------------
def chan_affine(a, x, mean, rstd, w, q, r, add, mask_src, relu_self=False, ld=False):
    """hf_chan_affine / _ex / _pair:  t = a*(w*rstd) + xhat*q + r + add,  xhat = (x - mean)*rstd;
    out = relu_self ? max(t, 0) : mask_src ? (mask_src > 0 ? t : 0) : t.   ``a``: [slabs, ..., c] or None."""
    a, x, mean, rstd, w, q, r, add, mask_src = (up(t, ld) for t in (a, x, mean, rstd, w, q, r, add, mask_src))
    like = next(v for v in (a[0] if a is not None else None, x, add, mask_src) if v is not None)
    t = M = like * 0
    if a is not None:
        s, ms = slab_sum(a)
        scale = (w if w is not None else 1) * (rstd if rstd is not None else 1)
        t, M = s * scale, ms * abs(scale)
    if q is not None:
        t, M = t + ((x - mean) * rstd) * q, M + ((abs(x) + abs(mean)) * abs(rstd)) * abs(q)
    for term in (r, add):
        if term is not None:
            t, M = t + term, M + abs(term)
    if relu_self:
        t = _where(t > 0, t)
    elif mask_src is not None:
        keep = mask_src > 0
        t, M = _where(keep, t), _where(keep, M)
    return t, M


def r_chan_affine(splits, has_a, has_q, has_r, has_add):
    """Roundings on the longest path: slab additions, w*rstd and a*(.) for the a term | (x-mean), *rstd, *q for the
    xhat term; one addition joins the two, one more each for r and add."""
    pa = (splits - 1) + 2 if has_a else 0
    pq = 3 if has_q else 0
    return max(pa, pq, 0) + (1 if has_a and has_q else 0) + int(has_r) + int(has_add) or 1


def chan_affine_bwd(gy, gy2, x, mean, rstd, w, mask_src, ld=False):
    """hf_chan_affine_bwd / _ex / _pair:  g = mask(gy + gy2) (both [slabs, rows.., c]); gx = g*(w*rstd), gres = g,
    gw = sum g*xhat, gb = sum g.  Returns the ELEMENTWISE fields flattened to [rows, c] (g, gx, gwe = g*xhat and their
    magnitude sums); ``col(field, lo, hi)`` sums a row share."""
    gy, gy2, x, mean, rstd, w, mask_src = (up(t, ld) for t in (gy, gy2, x, mean, rstd, w, mask_src))
    g, Mg = slab_sum(gy)
    if gy2 is not None:
        h, mh = slab_sum(gy2)
        g, Mg = g + h, Mg + mh
    if mask_src is not None:
        keep = mask_src > 0
        g, Mg = _where(keep, g), _where(keep, Mg)
    c = g.shape[-1]
    scale = (w if w is not None else 1) * (rstd if rstd is not None else 1)
    out = NS(g=g.reshape(-1, c), Mg=Mg.reshape(-1, c))
    out.gx, out.Mgx = (g * scale).reshape(-1, c), (Mg * abs(scale)).reshape(-1, c)
    if x is not None:
        rs = rstd if rstd is not None else 1
        mu = mean if mean is not None else 0
        out.gwe = (g * ((x - mu) * rs)).reshape(-1, c)
        out.Mgwe = (Mg * ((abs(x) + abs(mu)) * abs(rs))).reshape(-1, c)
    out.col = lambda f, lo=0, hi=None: f[lo:hi].sum(0)
    return out


def r_bwd_g(s1, s2):
    """g: the slab additions of the longer cotangent + the addition of the two."""
    return max(max(s1, s2 or 1) - 1 + (1 if s2 else 0), 1)


def r_bwd_gx(s1, s2):
    return r_bwd_g(s1, s2) + 2  # w*rstd, g*(.)


def r_bwd_gw(s1, s2):
    """Column sums are accumulated in fp64 and rounded once per partial row: the fp32 roundings inside one term
    (g, and xhat = (x-mean)*rstd rounded to fp32 before the product) + the store."""
    return r_bwd_g(s1, s2) + 2 + 1


def r_bwd_gb(s1, s2):
    return r_bwd_g(s1, s2) + 1


def bn_forward(a, mean, rstd, w, b, res, relu, ld=False):
    """hf_bn_forward: s = sum of slabs; t = rstd ? ((s-mean)*rstd)*w : s; + b; + res; y = relu ? max(t,0) : t."""
    a, mean, rstd, w, b, res = (up(t, ld) for t in (a, mean, rstd, w, b, res))
    s, ms = slab_sum(a)
    t, M = s, ms
    if rstd is not None:
        t, M = ((s - mean) * rstd) * w, ((ms + abs(mean)) * abs(rstd)) * abs(w)
    for term in (b, res):
        if term is not None:
            t, M = t + term, M + abs(term)
    if relu:
        t = _where(t > 0, t)
    return NS(s=s, Ms=ms, y=t, My=M)


def r_bn_forward(splits, has_rstd, has_b, has_res):
    return max((splits - 1) + (3 if has_rstd else 0) + int(has_b) + int(has_res), 1)


def bn_adjoint_pre(gy_a, gy_b, mask_src, w, rstd, ld=False):
    """hf_bn_adjoint_pre: g = mask(sum gy_a + sum gy_b); ga = g * (w*rstd)."""
    b = chan_affine_bwd(gy_a, gy_b, None, None, rstd, w, mask_src, ld)
    return NS(g=b.g, Mg=b.Mg, ga=b.gx, Mga=b.Mgx)


# ---- train-mode BatchNorm ---------------------------------------------------------------------------------------
def chan_affine_train(a, x, mean, rstd, w, part_x, part_1, vq, vr, count, add, mask_src):
    """hf_chan_affine_train / _pair:  q = vq - w*rstd*S_x/count, r = vr - w*rstd*S_1/count (S_*: the column sums of
    the partial rows), out = mask(sum(a)*(w*rstd) + xhat*q + r + add)."""
    a, x, mean, rstd, w, part_x, part_1, vq, vr, add, mask_src = (
        up(t) for t in (a, x, mean, rstd, w, part_x, part_1, vq, vr, add, mask_src))
    k = w * rstd / count
    q, Mq = -k * part_x.sum(0), abs(k) * part_x.abs().sum(0)
    r, Mr = -k * part_1.sum(0), abs(k) * part_1.abs().sum(0)
    if vq is not None:
        q, Mq = q + vq, Mq + vq.abs()
    if vr is not None:
        r, Mr = r + vr, Mr + vr.abs()
    s, ms = slab_sum(a)
    t = s * (w * rstd) + ((x - mean) * rstd) * q + r
    M = ms * (w * rstd).abs() + ((x.abs() + mean.abs()) * rstd.abs()) * Mq + Mr
    if add is not None:
        t, M = t + add, M + add.abs()
    if mask_src is not None:
        keep = mask_src > 0
        t, M = _where(keep, t), _where(keep, M)
    return t, M


def r_chan_affine_train(splits, has_add):
    """q / r: 1/count rounded to fp32, w*rstd, *(1/count), the fp64 column sum rounded to fp32, k*S, the subtraction
    = 6, then *xhat; the a term: slab additions + w*rstd + a*(.); then the additions of the two terms, r and add."""
    return max(6 + 1, (splits - 1) + 2) + 2 + int(has_add)


def train_hessian_closed_form(s_gx, s_g, s_ga, S1, Sx, g_gam, g_bet, gam, dgam, r, m, mag=False):
    """The closed forms behind hf_bn_train_hessian_coeffs (header: "Hessian product ... through a TRAIN-mode
    BatchNorm"): from the five row sums, the first-order parameter gradients and the per-channel vectors the six
    coefficients of  g_a' = c0 g_a + c1 g_z + c2 g_z' + c3 a' + c4 xhat + c5,  the closed-form share ``corr`` of
    g_gamma' and g_gamma' = dgg itself.  ``mag=True``: the magnitude sums (absolute values, every sign positive)."""
    sg = 1.0
    if mag:
        s_gx, s_g, s_ga, S1, Sx, g_gam, g_bet, gam, dgam, r = (
            abs(t) for t in (s_gx, s_g, s_ga, S1, Sx, g_gam, g_bet, gam, dgam, r))
        sg = -1.0
    corr = -sg * r * (S1 * g_bet + Sx * g_gam)
    dgg = s_gx + s_ga + corr
    mG, m2, mGx = (dgam * g_bet + gam * s_g) / m, (dgam * g_gam + gam * dgg) / m, gam * g_gam / m
    c = (-sg * r * Sx, r * dgam, r * gam, -sg * r * r * mGx, r * r * mGx * Sx - sg * r * m2,
         -sg * r * mG + r * r * mGx * S1)
    return c, corr, dgg


def train_hessian_coeffs(sum_gx2, sum_g2, sum_ga, sum_tx, sum_t1, g_gamma1, g_beta1, gamma, v_gamma, rstd, count):
    """hf_bn_train_hessian_coeffs: partial rows [nparts, c] -> (coef [6, c], gw_corr [c]) and their magnitude sums."""
    f = [up(t) for t in (sum_gx2, sum_g2, sum_ga, sum_tx, sum_t1, g_gamma1, g_beta1, gamma, v_gamma, rstd)]
    out = []
    for mag in (False, True):
        red = (lambda t: t.abs().sum(0)) if mag else (lambda t: t.sum(0))
        s_gx, s_g, s_ga, s_tx, s_t1 = (red(t) for t in f[:5])
        c, corr, _ = train_hessian_closed_form(s_gx, s_g, s_ga, s_t1 / count, s_tx / count, f[5], f[6], f[7], f[8],
                                               f[9], count, mag=mag)
        out += [torch.stack(c), corr]
    return NS(coef=out[0], corr=out[1], Mcoef=out[2], Mcorr=out[3])


def train_hessian_apply(ga1, gz1, gz2, t, a, mean, rstd, coef, Mcoef=None):
    """hf_bn_train_hessian_apply: out = c0 ga1 + c1 gz1 + c2 gz2 + c3 sum(t) + c4 xhat + c5."""
    ga1, gz1, gz2, t, a, mean, rstd, coef = (up(v) for v in (ga1, gz1, gz2, t, a, mean, rstd, coef))
    Mc = coef.abs() if Mcoef is None else Mcoef
    ts, mts = slab_sum(t)
    xh, mxh = (a - mean) * rstd, (a.abs() + mean.abs()) * rstd.abs()
    out = coef[0] * ga1 + coef[1] * gz1 + coef[2] * gz2 + coef[3] * ts + coef[4] * xh + coef[5]
    M = Mc[0] * ga1.abs() + Mc[1] * gz1.abs() + Mc[2] * gz2.abs() + Mc[3] * mts + Mc[4] * mxh + Mc[5]
    return out, M


def r_train_hessian_apply(splits):
    """k3 * (slab sum) is the longest product: slab additions + the product, then three levels of additions
    ((k0 ga + k1 gz) + (k2 gz' + k3 t)) + (k4 xhat + k5); xhat's own path (2 + 1 + 2) is never longer."""
    return max((splits - 1) + 1 + 2, 5)


# ---- heads and pooling ------------------------------------------------------------------------------------------
def maxpool_forward(x, kh, kw, sh, sw, ph, pw):
    """hf_maxpool_forward_nhwc, literally: the first maximum of the window in scan order, NaN wins; returns
    (values, flat positions y*w + x), both [n, c, oh, ow]."""
    n, c, h, w = x.shape
    oh, ow = (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1
    val = torch.full((n, c, oh, ow), float("-inf"), dtype=x.dtype)
    idx = torch.zeros((n, c, oh, ow), dtype=torch.int64)
    for oy in range(oh):
        for ox in range(ow):
            y0, x0 = max(oy * sh - ph, 0), max(ox * sw - pw, 0)
            y1, x1 = min(oy * sh - ph + kh, h), min(ox * sw - pw + kw, w)
            best = torch.full((n, c), float("-inf"), dtype=x.dtype)
            bi = torch.full((n, c), y0 * w + x0, dtype=torch.int64)
            for yy in range(y0, y1):
                for xx in range(x0, x1):
                    v = x[:, :, yy, xx]
                    take = (v > best) | torch.isnan(v)
                    best = torch.where(take, v, best)
                    bi = torch.where(take, torch.full_like(bi, yy * w + xx), bi)
            val[:, :, oy, ox], idx[:, :, oy, ox] = best, bi
    return val, idx


def softmax_ce_hvp(p, v, scale, ld=False):
    """hf_softmax_ce_hvp: out = scale * p * (v - <p, v>) row-wise."""
    p, v = up(p, ld), up(v, ld)
    d, md = (p * v).sum(-1)[..., None], abs(p * v).sum(-1)[..., None]
    return scale * (p * (v - d)), abs(scale) * (abs(p) * (abs(v) + md))


def r_softmax_ce_hvp(cols, f64):
    """fp32: the dot product is accumulated in fp64 and rounded once, `scale` is rounded to fp32, then v - d,
    p*(.), scale*(.).  fp64: the dot product's products and additions round in the working precision (any order:
    `cols` roundings), `scale` is exact."""
    return (cols + 3) if f64 else 5


def pool_ce_head(t, p, scale):
    """hf_pool_ce_head: Jv = mean_hw t [n, hw, k]; h = scale * p * (Jv - <p, Jv>); g[n, hw, k] = h / hw."""
    t, p = up(t), up(p)
    hw = t.shape[1]
    jv, mjv = t.sum(1) / hw, t.abs().sum(1) / hw
    d, md = (p * jv).sum(-1, keepdim=True), (p.abs() * mjv).sum(-1, keepdim=True)
    h, mh = scale * (p * (jv - d)) / hw, abs(scale) * (p.abs() * (mjv + md)) / hw
    return NS(jv=jv, Mjv=mjv, g=h[:, None, :].expand_as(t), Mg=mh[:, None, :].expand_as(t))


def r_pool_ce_head(hw):
    """Jv: hw - 1 additions and the division = hw; then the fp64 dot product rounded once, `scale` rounded to
    fp32, Jv - d, p*(.), scale*(.), / hw."""
    return hw, hw + 6


def conv_refs(x, w, gy, stride, padding):
    """float64 convolution, data gradient and weight gradient (NCHW tensors)."""
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = torch.nn.functional.conv2d(x64, w64, None, stride, padding)
    gx, gw = torch.autograd.grad(y, (x64, w64), gy.double())
    return y.detach(), gx, gw


# =================================================================================================================
# Inputs of the kernel tests: generated on the CPU from a seed (the CPU tests of the bounds use the same numbers)
# =================================================================================================================
def gen_of(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + (hash(k) if not isinstance(k, str) else sum(map(ord, k)))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def randn(gen, *shape, dtype=torch.float32):
    return torch.randn(*shape, generator=gen, dtype=dtype)


def rstd_like(gen, c, dtype=torch.float32):
    """positive, spread over 0.1 ... 10"""
    return (10.0 ** (torch.rand(c, generator=gen, dtype=torch.float64) * 2 - 1)).to(dtype)


def mask_like(gen, *shape, dtype=torch.float32):
    """negative values, exact +0.0, exact -0.0 and positive values; at least 5 % exact zeros"""
    m = torch.randn(*shape, generator=gen, dtype=dtype)
    u = torch.rand(*shape, generator=gen)
    m[u < 0.04] = 0.0
    m[(u >= 0.04) & (u < 0.08)] = -0.0
    flat = m.view(-1)
    k = max(2, -(-flat.numel() // 10))  # (tiny tensors: every tenth element by construction)
    flat[0:k:2] = 0.0
    flat[1:k:2] = -0.0
    if flat.numel() > k + 1:
        flat[k], flat[k + 1] = -0.75, 0.5
    zeros = int((flat == 0).sum())
    assert zeros * 20 >= flat.numel() and bool((torch.signbit(flat) & (flat == 0)).any())
    return m


EVAL_SHAPES = [(1568, 64), (32, 512), (200, 96), (37, 12), (5, 4), (130, 260), (64, 1024), (3, 20)]
# Up to 17 slabs a 16-deep batch loop (which starts at slab 1) makes one pass.  18 is the first count with a second
# pass, 33 fills two passes exactly, 34 adds a third with one live load; the 8-deep loops end on a partial batch at 18
# and 34.
SLAB_COUNTS_ONE_PASS = [(1, None), (1, 1), (3, 1), (8, 1), (9, 2), (1, 9), (2, 17), (17, 17)]
SLAB_COUNTS_MORE_PASSES = [(18, 1), (1, 18), (34, 33)]
SLAB_COUNTS = SLAB_COUNTS_ONE_PASS + SLAB_COUNTS_MORE_PASSES


def eval_cases():
    """(shape, slab counts, i) of the eval-mode forms; i numbers the cases and picks each one's variant.  The counts
    with more than one 16-deep pass come last, so that the cases before them keep their numbers."""
    pairs = [(sh, sl) for sh in EVAL_SHAPES for sl in SLAB_COUNTS_ONE_PASS] + \
            [(sh, sl) for sh in EVAL_SHAPES for sl in SLAB_COUNTS_MORE_PASSES]
    return [(sh, sl, i) for i, (sh, sl) in enumerate(pairs)]


def eval_inputs(rows, c, s1, s2, dtype=torch.float32, tag="eval"):
    """Operands of the eval-mode forms on [rows, c]: two slab sets (the second is None for s2 = None), x, mask source,
    residual, and the per-channel vectors."""
    gen = gen_of(tag, rows, c, s1, s2 or 0, str(dtype))
    o = NS(rows=rows, c=c, s1=s1, s2=s2)
    o.a = randn(gen, s1, rows, c, dtype=dtype)
    o.b = randn(gen, s2, rows, c, dtype=dtype) if s2 else None
    o.x = randn(gen, rows, c, dtype=dtype) * 2 + 0.5
    o.mask = mask_like(gen, rows, c, dtype=dtype)
    o.add = randn(gen, rows, c, dtype=dtype)
    o.mean, o.w, o.q, o.r = (randn(gen, c, dtype=dtype) for _ in range(4))
    o.rstd = rstd_like(gen, c, dtype)
    return o


def row_block_choices(rows, c):
    """{1, 2, 7, 63, rows} + one count that leaves the last share short + one whose shares are smaller than the
    BLOCK / (c/4) rows a workgroup takes per pass.  ``share_ok`` tells which the library accepts."""
    rp = max(256 // (c // 4), 1)
    out = [1, 2, 7, 63, rows]
    short = next((rb for rb in range(3, rows) if rows % rb and (rb - 1) * -(-rows // rb) < rows), None)
    small = next((rb for rb in range(2, rows + 1) if -(-rows // rb) < rp and (rb - 1) * -(-rows // rb) < rows), None)
    for rb in (short, small):
        if rb is not None:
            out.append(rb)
    seen, uniq = set(), []
    for rb in out:
        if rb not in seen and rb >= 1:
            seen.add(rb)
            uniq.append(rb)
    return uniq


def share_ok(rows, row_blocks):
    """No empty workgroup: the last of ``row_blocks`` shares of ceil(rows / row_blocks) rows still starts inside."""
    return (row_blocks - 1) * -(-rows // row_blocks) < rows


def row_shares(rows, row_blocks):
    per = -(-rows // row_blocks)
    return [(i * per, min((i + 1) * per, rows)) for i in range(row_blocks)]


def train_hessian_problem(rows, c, t_splits, seed=0):
    """The float64 problem of ``test_train_mode_batchnorm_hessian_closed_forms`` on fp32 data: z = gamma*xhat + beta,
    y = relu(z), loss = sum(y*wl) + sum(y**3)/3; the first-order cotangents, the tangent sweep's quantities, the
    second-order cotangent and -- by float64 double backward -- the wanted tangent of the adjoint."""
    dt = torch.float64
    gen = gen_of("hess", rows, c, t_splits, seed)
    eps = 1e-5
    a32 = randn(gen, rows, c) * 2 + 0.5
    gam32, bet32, dgam32, dbet32 = (randn(gen, c) for _ in range(4))
    wl = randn(gen, rows, c, dtype=dt)
    t32 = randn(gen, t_splits, rows, c)          # the tangent convolution's slabs: a' is their sum
    mean32 = a32.double().mean(0).float()
    rstd32 = (a32.double().var(0, unbiased=False) + eps).rsqrt().float()
    a = a32.double().requires_grad_()
    gam, bet = gam32.double().requires_grad_(), bet32.double().requires_grad_()
    mu = a.mean(0)
    r = (((a - mu) ** 2).mean(0) + eps).rsqrt()
    xh = (a - mu) * r
    z = gam * xh + bet
    y = torch.relu(z)
    loss = (y * wl).sum() + (y ** 3).sum() / 3
    ga, gg, gb = torch.autograd.grad(loss, (a, gam, bet), create_graph=True)
    da, dgam, dbet = t32.double().sum(0), dgam32.double(), dbet32.double()
    want_a, want_g, want_b = torch.autograd.grad((ga * da).sum() + (gg * dgam).sum() + (gb * dbet).sum(), (a, gam, bet))
    with torch.no_grad():
        mask = (z > 0).to(dt)
        g_z = mask * (wl + y ** 2)
        S1, Sx = da.mean(0), (da * xh).mean(0)
        dxh = r * (da - S1 - xh * Sx)
        dy = mask * (dgam * xh + gam * dxh + dbet)
        dg_z = mask * (2 * y * dy)
    return NS(rows=rows, c=c, a=a32, mean=mean32, rstd=rstd32, gam=gam32, dgam=dgam32, t=t32, xh=xh.detach(),
              r=r.detach(), ga=ga.detach(), g_z=g_z, dg_z=dg_z, da=da, gg=gg.detach(), gb=gb.detach(),
              want_a=want_a, want_g=want_g, want_b=want_b)


def partial_rows(elem, nparts):
    """[rows, c] float64 -> the fp32 partial rows [nparts, c] a reduction launch with ``nparts`` row shares leaves
    (shares past the end are empty: zeros)."""
    rows = elem.shape[0]
    per = -(-rows // nparts)
    out = torch.zeros(nparts, elem.shape[1], dtype=torch.float64)
    for i in range(nparts):
        if i * per < rows:
            out[i] = elem[i * per:(i + 1) * per].sum(0)
    return out.float()


POOL_GEOMS = [(32, 64, 14, 14, 3, 3, 2, 2, 1, 1), (3, 8, 9, 7, 2, 2, 2, 2, 0, 0), (2, 12, 10, 10, 3, 3, 1, 1, 1, 1),
              (2, 4, 7, 7, 3, 3, 3, 3, 1, 1), (1, 4, 5, 5, 3, 3, 2, 2, 1, 1), (2, 8, 9, 11, 3, 2, 2, 1, 1, 0)]


def maxpool_input(geom):
    """Multiples of 0.25 (frequent ties), some -inf, and NaNs placed so that no window holds two of them."""
    n, c, h, w, kh, kw = geom[:6]
    gen = gen_of("pool", *geom)
    x = (torch.randn(n, c, h, w, generator=gen) * 4).round() / 4
    x[torch.rand(n, c, h, w, generator=gen) < 0.05] = float("-inf")
    nan = torch.zeros(n, c, h, w, dtype=torch.bool)
    oy, ox = int(torch.randint(0, kh, (1,), generator=gen)), int(torch.randint(0, kw, (1,), generator=gen))
    nan[:, :, oy::2 * kh, ox::2 * kw] = torch.rand(n, c, len(range(oy, h, 2 * kh)), len(range(ox, w, 2 * kw)),
                                                   generator=gen) < 0.5
    x[nan] = float("nan")
    return x


HEAD_SHAPES = [(32, 36, 10), (5, 1, 3), (7, 64, 100), (1, 49, 10), (130, 4, 12)]


def head_inputs(n, hw, k):
    gen = gen_of("head", n, hw, k)
    t = randn(gen, n, hw, k)
    p = torch.softmax(randn(gen, n, k) * 2, 1)
    return t, p


def softmax_inputs(rows, cols, dtype):
    gen = gen_of("smx", rows, cols, str(dtype))
    p = torch.softmax(randn(gen, rows, cols, dtype=torch.float64) * 2, 1)
    if cols > 1:  # one row with one entry ~ 1 and the rest ~ 1e-8
        p[0] = 1e-8
        p[0, cols // 2] = 1.0 - 1e-8 * (cols - 1)
    return p.to(dtype), randn(gen, rows, cols, dtype=dtype)


LAYOUT_SHAPES = [(3, 8, 5, 4), (2, 6, 3, 3), (4, 16, 1, 1), (1, 4, 2, 7), (2, 3, 9, 9), (64, 5, 3, 3), (2, 32, 17, 17)]


# Which optional operands a case leaves out (every NULL combination the header documents appears at least once), and
# the leading dimension of its output / residual buffers (0 = dense, else a multiple of c plus a remainder).
AFFINE_VARIANTS = [
    NS(drop=(), relu_self=0, ld=(0, 0)),
    NS(drop=("q",), relu_self=0, ld=(2, 0)),                      # no xhat term: x / mean are not read
    NS(drop=("q", "rstd"), relu_self=0, ld=(2, 4)),               # rstd == NULL: convolution + bias layer
    NS(drop=("w",), relu_self=0, ld=(0, 0)),
    NS(drop=("a",), relu_self=0, ld=(2, 0)),                      # (single-slab cases only)
    NS(drop=("r", "add"), relu_self=0, ld=(2, 4)),
    NS(drop=("mask",), relu_self=0, ld=(0, 0)),
    NS(drop=(), relu_self=1, ld=(2, 0)),                          # forward form: its own ReLU, mask_src ignored
    NS(drop=("a", "q", "x", "mean"), relu_self=0, ld=(2, 4)),     # r + add alone
]
BWD_VARIANTS = [
    NS(drop=()),
    NS(drop=("gx",)),                                             # reduction-only form (+ gres)
    NS(drop=("gw", "x", "mean")),                                 # gw == NULL allows x == NULL
    NS(drop=("gw", "gx", "gres", "x", "mean", "rstd", "w")),      # gb alone: a convolution layer's bias gradient
    NS(drop=("mask",)),
    NS(drop=("w",)),
    NS(drop=("gres", "gb")),
    NS(drop=("gw", "x", "mean", "rstd")),                         # no BatchNorm: gx = g * w
]


def pick(o, names, drop):
    return [None if n in drop else getattr(o, n) for n in names]


# (rows, c, splits, nparts): c in {4, 12, 96, 1024} x nparts in {1, 7, 64, 257} (both sides of HF_FCS_BATCH * G partial
# rows per pass), splits in {1, 8, 9}; then 18 and 34 slabs: a second and a third 16-deep pass
TRAIN_CASES = [(64, 4, 1, 1), (37, 4, 8, 7), (50, 4, 9, 64), (40, 4, 8, 257),
               (37, 12, 8, 1), (33, 12, 9, 7), (200, 12, 1, 64), (64, 12, 9, 257),
               (200, 96, 9, 1), (130, 96, 1, 7), (64, 96, 8, 64), (37, 96, 9, 257),
               (32, 1024, 8, 1), (5, 1024, 9, 7), (16, 1024, 1, 64), (32, 1024, 8, 257),
               (37, 12, 18, 7), (32, 1024, 34, 64)]


def train_inputs(rows, c, splits, nparts):
    """Operands of hf_chan_affine_train: those of the eval forms + the reduction launch's partial rows."""
    o = eval_inputs(rows, c, splits, None, tag="train")
    gen = gen_of("trainparts", rows, c, splits, nparts)
    o.px, o.p1 = randn(gen, nparts, c) * 3, randn(gen, nparts, c) * 3
    return o


# =================================================================================================================
# Train-mode BatchNorm forward (hf_bn_stats_rows, hf_bn_forward_train) and the linear head (hf_linear_ce_head)
# =================================================================================================================
# These references run in numpy.longdouble where the kernels run in fp64 (their bounds are stated in U64: a float64
# reference would err as much as the kernel).  REF64 scales an fp64 rounding count for the reference's own roundings:
# 1 + 2**-11 with an 80-bit longdouble, 2 where longdouble is float64.
LDT = np.longdouble
REF64 = 1.0 + (LD_EPS / 2) / U64


def mixed(M, R, M64, R64):
    """``R*U32*M + R64*U64*M64`` as the M of a comparison with R = 1, u = U32: a result with fp32 roundings on values
    of magnitude M AND fp64 roundings on (larger, cancelling) values of magnitude M64."""
    return R * M + (R64 * REF64 * U64 / U32) * M64


def _ld(t):
    return None if t is None else (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).astype(LDT)


def f32_slab_sum(a, upto=None):
    """The split-order fp32 sum of the slabs [splits, ...]: bitwise what every slab loop of the library leaves."""
    a = a.numpy()
    s = a[0].copy()
    for i in range(1, a.shape[0] if upto is None else upto):
        s = s + a[i]
    return torch.from_numpy(s)


def bn_stats(a_slabs, row_blocks):
    """hf_bn_stats_rows: s = split-order fp32 sum of the slabs [splits, rows, c] (bitwise); part[i] = (sum s, sum s*s)
    over share i of ceil(rows / row_blocks) rows -- exact sums (the square of an fp32 value is exact in fp64), an empty
    share gives zeros.  Unit U64; ``R[i]`` = the rows of share i (its fp64 additions, at least 1)."""
    s = f32_slab_sum(a_slabs)
    sl = _ld(s)
    c = s.shape[-1]
    part, M, R = np.zeros((row_blocks, 2, c), LDT), np.zeros((row_blocks, 2, c), LDT), np.ones(row_blocks)
    for i, (lo, hi) in enumerate(row_shares(s.shape[0], row_blocks)):
        if lo < hi:
            blk = sl[lo:hi]
            part[i, 0], part[i, 1] = blk.sum(0), (blk * blk).sum(0)
            M[i, 0], M[i, 1] = np.abs(blk).sum(0), part[i, 1]
            R[i] = hi - lo
    return NS(s=s, part=part, Mpart=M, R=R)


def ratio_rows(got, want, M, R, u=U64):
    """``ratio`` with one R per leading index (partial rows of shares of different lengths)."""
    return max(ratio(got[i], want[i], M[i], float(R[i]), u) for i in range(len(R)))


def bn_forward_train(s, part, count, eps, momentum, w, b, res, relu, run_mean, run_var):
    """hf_bn_forward_train on the partial rows AS GIVEN (float64 [nparts, 2, c]) and the summed activation s [rows, c]:
    mean = S1/count, var = max(S2/count - mean^2, 0), rstd = 1/sqrt(var + eps) (eps exact),
    running <- (1 - momentum) running + momentum * {mean, var * count/(count - 1)} (count == 1: var), and
    y = act(((s - mean)*rstd)*w + b + res).  Every result with its fp32 magnitude M and, where fp64 roundings act on
    larger cancelling values, M64 (see ``r_bn_forward_train`` / ``mixed``)."""
    p_, sl, w, b, res, rm, rv = (_ld(t) for t in (part, s, w, b, res, run_mean, run_var))
    count, eps = LDT(count), LDT(eps)
    S1, S2 = p_[:, 0].sum(0), p_[:, 1].sum(0)
    Mm, E2 = np.abs(p_[:, 0]).sum(0) / count, np.abs(p_[:, 1]).sum(0) / count
    mean = S1 / count
    var = np.maximum(S2 / count - mean * mean, 0)
    Mvar = E2 + Mm * Mm + eps
    rstd = 1 / np.sqrt(var + eps)
    drstd = rstd ** 3 / 2                       # |d rstd / d var|
    o = NS(mean=mean, Mmean=Mm, var=var, rstd=rstd, Mrstd=rstd + drstd * eps, Mrstd64=rstd + drstd * Mvar)
    if momentum is not None and momentum >= 0 and rm is not None:
        mo = LDT(momentum)
        k = count / (count - 1) if count > 1 else LDT(1)
        both = abs(1 - mo) + abs(mo)
        o.rm, o.Mrm = (1 - mo) * rm + mo * mean, both * np.abs(rm) + abs(mo) * Mm
        o.rv, o.Mrv = (1 - mo) * rv + mo * var * k, both * np.abs(rv) + abs(mo) * var * k
        o.Mrv64 = o.Mrv + abs(mo) * k * Mvar
    t = ((sl - mean) * rstd) * w
    spread = (np.abs(sl) + Mm) * np.abs(w)
    M, M64 = spread * rstd, spread * o.Mrstd64
    for term in (b, res):
        if term is not None:
            t, M = t + term, M + np.abs(term)
    o.y, o.My, o.My64 = (np.where(t > 0, t, 0) if relu else t), M, M64
    return o


def r_bn_forward_train(nparts, has_b, has_res):
    """(R, R64) per result, from the kernel's order.  fp64 (unit U64): nparts - 1 additions per sum, /count; the
    variance E[a^2] - mean^2 carries the mean's roundings twice (2*nparts), the product, the subtraction, + eps, sqrt,
    1/x: 2*nparts + 5; the running variance further *count, /(count-1), two products and the addition.  fp32:
      mean   -- its store;                       rstd -- eps rounded to fp32 and the store (one each on the two
      terms of Mrstd = rstd + |d rstd/d var| eps);
      running mean -- momentum rounded to fp32, the ROUNDED mean, the store;   running var -- momentum, the store;
      y      -- mean's and rstd's stores, eps (half a rounding of rstd, counted as one), a - mean, *rstd, *w, + b, + res."""
    return NS(mean=(1, nparts), rstd=(1, 2 * nparts + 5), rm=(3, nparts + 3), rv=(2, 2 * nparts + 10),
              y=(6 + int(has_b) + int(has_res), 2 * nparts + 5))


HEAD_ROWS, HEAD_KB = 4, 5        # rows per workgroup / classes per pass of k_linear_ce_head


def linear_ce_head(t_feat, feat, w, v_w, v_b, p, scale):
    """hf_linear_ce_head:  Jv = t_feat W^T + feat V_W^T + v_b;  h = scale * p * (Jv - <p, Jv>);  g_feat = h W;
    per workgroup g (rows 4g .. 4g+3, those past the end contribute nothing):  g_w[g] = h^T feat, g_b[g] = sum h."""
    t_feat, feat, w, v_w, v_b, p = (up(t) for t in (t_feat, feat, w, v_w, v_b, p))
    jv, M = t_feat @ w.t() + feat @ v_w.t(), t_feat.abs() @ w.abs().t() + feat.abs() @ v_w.abs().t()
    if v_b is not None:
        jv, M = jv + v_b, M + v_b.abs()
    d, Md = (p * jv).sum(1, keepdim=True), (p.abs() * M).sum(1, keepdim=True)
    h, Mh = scale * (p * (jv - d)), abs(scale) * (p.abs() * (M + Md))
    rows, groups = h.shape[0], -(-h.shape[0] // HEAD_ROWS)
    sl = [slice(HEAD_ROWS * g, min(HEAD_ROWS * (g + 1), rows)) for g in range(groups)]
    return NS(jv=jv, Mjv=M, h=h, Mh=Mh, g_feat=h @ w, Mg_feat=Mh @ w.abs(),
              g_w=torch.stack([h[q].t() @ feat[q] for q in sl]), Mg_w=torch.stack([Mh[q].t() @ feat[q].abs() for q in sl]),
              g_b=torch.stack([h[q].sum(0) for q in sl]), Mg_b=torch.stack([Mh[q].sum(0) for q in sl]))


def head_chunks(features):
    """template parameter CH of k_linear_ce_head: float4 chunks per lane"""
    return -(-(features // 4) // 64)


def r_linear_ce_head(features, classes, has_bias):
    """Jv: each lane runs two interleaved fma chains over its CH chunks (4 fmas per chain and chunk), adds the two, six
    shuffle additions, the bias.  h: + the fp64 dot product rounded once (its six fp64 additions: 6 U64), `scale`
    rounded to fp32, Jv - d, p*(.), scale*(.).  g_feat: `classes` sequential fmas; a g_w slab: four fmas; a g_b slab:
    three additions (the first is 0 + h)."""
    jv = 4 * head_chunks(features) + 1 + 6 + int(has_bias)
    h = jv + 5 + 6 * U64 / U32
    return NS(jv=jv, h=h, g_feat=h + classes, g_w=h + HEAD_ROWS, g_b=h + HEAD_ROWS - 1)


def head_shape_ok_ref(rows, features, classes):
    """The entry point's shape rule, from the header: what the host's predicate and the library must both say."""
    lds = (2 * classes * features + HEAD_ROWS * features + HEAD_ROWS * classes) * 4
    return 1 <= rows <= 4096 and 1 <= classes <= 64 and 4 <= features <= 512 and features % 4 == 0 and lds <= 65536


# ---- thread-map mirrors (what the branch-coverage test asserts the tables reach) ----------------------------------
BLOCK = 256


def stats_map(rows, c, splits, row_blocks):
    """k_bn_stats_rows: quads, rows per pass RP, idle threads, shares shorter than a pass / empty, and whether the
    8-deep slab loop ends on a partial batch (and in which pass)."""
    quads = c // 4
    rp = BLOCK // quads
    sh = [hi - lo for lo, hi in row_shares(rows, row_blocks)]
    passes = -(-(splits - 1) // 8)
    return NS(quads=quads, RP=rp, idle=BLOCK - rp * quads, short=any(0 < n < rp for n in sh),
              empty=any(n <= 0 for n in sh), several_passes=any(n > rp for n in sh), slab_passes=passes,
              partial_batch=(splits - 1) % 8 != 0)


def fwd_map(rows, c, nparts):
    """k_bn_forward_train: prologue lanes, row groups G, column passes, whether nparts exceeds one 4*G batch or leaves
    it partial, idle prologue threads, and whether the last workgroup has threads without a quad."""
    lanes = min(c, BLOCK)
    G = BLOCK // lanes
    quads = rows * c // 4
    return NS(lanes=lanes, G=G, col_passes=-(-c // lanes), batches=-(-nparts // (4 * G)), partial=nparts % (4 * G) != 0,
              groups_without_rows=nparts < G, idle=BLOCK - G * lanes, wgs=-(-quads // BLOCK), have_false=quads % BLOCK != 0)


def head_map(rows, features, classes):
    """k_linear_ce_head: CH, live lanes of the last chunk, KB passes and the clamped surplus of the last one, rows of
    the last workgroup, LDS bytes."""
    f4 = features // 4
    ch = head_chunks(features)
    return NS(CH=ch, last_chunk_lanes=f4 - 64 * (ch - 1), passes=-(-classes // HEAD_KB), clamped=-classes % HEAD_KB,
              all_lanes_hold_a_class=classes == 64, last_rows=rows - HEAD_ROWS * ((rows - 1) // HEAD_ROWS),
              groups=-(-rows // HEAD_ROWS),
              lds=(2 * classes * features + HEAD_ROWS * features + HEAD_ROWS * classes) * 4)


# ---- inputs -------------------------------------------------------------------------------------------------------
CONST_VALUE = 3.25               # the constant channel (exact in fp32; its sums and squares are exact in fp64)
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def train_fwd_activation(gen, rows, c):
    """[rows, c] fp32: channel 0 constant, channel 1 mean ~ 100 / std ~ 0.1 (|mean|/std ~ 1e3), channel 2 std ~ 0.003
    (variance of the order of eps), the others offset ~ N(0, 1), scale 0.1 ... 10."""
    off = randn(gen, c, dtype=torch.float64)
    sc = 10.0 ** (torch.rand(c, generator=gen, dtype=torch.float64) * 2 - 1)
    off[0], sc[0] = CONST_VALUE, 0.0
    if c > 1:
        off[1], sc[1] = 100.0, 0.1
    if c > 2:
        off[2], sc[2] = 0.5, 0.003
    return (off + sc * randn(gen, rows, c, dtype=torch.float64)).float()


def stats_inputs(rows, c, splits):
    """Slabs [splits, rows, c] whose split-order sum has the channels of ``train_fwd_activation``: slabs 1.. are
    random (channel 0: the constants 0.25 k, so that every partial sum is exact), slab 0 holds the rest."""
    gen = gen_of("bnstats", rows, c, splits)
    target = train_fwd_activation(gen, rows, c)
    a = randn(gen, splits, rows, c)
    for k in range(1, splits):
        a[k, :, 0] = 0.25 * k
    a[0] = (target.double() - a[1:].double().sum(0)).float()
    return a


def share_sums(s, nparts):
    """float64 [nparts, 2, c]: the exact share sums of s and s*s, rounded once (the forward kernel's input)."""
    a = torch.zeros(1, *s.shape)
    a[0] = s
    return torch.from_numpy(bn_stats(a, nparts).part.astype(np.float64))


def train_fwd_inputs(rows, c, nparts):
    gen = gen_of("bnfwd", rows, c, nparts)
    o = NS(rows=rows, c=c, nparts=nparts, s=train_fwd_activation(gen, rows, c))
    o.part = share_sums(o.s, nparts)
    o.w, o.b, o.rm = (randn(gen, c) for _ in range(3))
    o.rv = randn(gen, c).abs() + 0.5
    o.res = randn(gen, rows, c)
    return o


# (c, rows) of the statistics kernel; row_blocks from row_block_choices + one count with empty last shares
STATS_SHAPES = [(c, r) for c in (4, 12, 96, 256) for r in (3, 37, 200)] + [(1024, 5)]
STATS_SPLITS = [1, 3, 8, 9, 17, 18, 34]
# a_out given | NULL;  slab stride dense | larger, NaN in the gap;  a whole NaN slab behind the last
STATS_FORMS = [NS(a_out=1, gap=0, tail=0), NS(a_out=0, gap=0, tail=1), NS(a_out=1, gap=1, tail=0),
               NS(a_out=0, gap=1, tail=1), NS(a_out=1, gap=1, tail=1)]


def stats_cases():
    """(rows, c, splits, row_blocks, form index): every row_blocks choice of every shape, splits and forms cycling
    (5 forms, 7 split counts, 6 to 8 choices: coprime cycles, every split count meets every form)."""
    out, i = [], 0
    for c, rows in STATS_SHAPES:
        for rb in row_block_choices(rows, c) + [rows + 2]:
            out.append((rows, c, STATS_SPLITS[i % 7], rb, i % 5))
            i += 1
    return out


FWD_C = [4, 12, 64, 96, 256, 1024]
FWD_NPARTS = [1, 3, 7, 64, 257]
# which of y / y2 (y2_ld = 2c);  residual: none | dense | res_ld = 2c;  b;  relu;  statistics: moved | momentum < 0 | NULL
FWD_OUT, FWD_RES, FWD_STAT = ("y", "y2", "both"), ("none", "dense", "strided"), ("move", "neg", "null")


def fwd_form(i):
    return NS(out=FWD_OUT[i % 3], res=FWD_RES[(i // 3 + i) % 3], b=i % 4 != 3, relu=(i // 2) % 2,
              stat=FWD_STAT[(i // 5 + i) % 3])


def fwd_cases():
    """(rows, c, nparts, i): c x nparts, rows cycling through sizes with and without a partial last workgroup (c = 1024:
    3 and 5 rows); i picks the argument form.  Last: rows = count = 1."""
    out = []
    for ci, c in enumerate(FWD_C):
        for pi, nparts in enumerate(FWD_NPARTS):
            i = len(out)
            rows = (5, 3)[pi % 2] if c == 1024 else (37, 3, 200, 50, 130)[(ci + pi) % 5]
            out.append((rows, c, nparts, i))
    return out + [(1, 12, 1, 0), (1, 1024, 3, 8)]


LIN_HEAD_CASES = [(1, 4, 1, 1), (5, 64, 3, 0), (7, 260, 11, 1), (16, 256, 10, 1), (32, 512, 10, 1), (130, 64, 12, 0),
                  (9, 120, 64, 1), (6, 512, 13, 1), (4, 8, 5, 1), (3, 8, 6, 0)]


def linear_head_inputs(rows, features, classes, bias):
    gen = gen_of("linhead", rows, features, classes, bias)
    o = NS(rows=rows, features=features, classes=classes, scale=1.0 / rows)
    o.t_feat, o.feat = randn(gen, rows, features), randn(gen, rows, features)
    o.w, o.v_w = randn(gen, classes, features), randn(gen, classes, features)
    o.v_b = randn(gen, classes) if bias else None
    p = torch.softmax(randn(gen, rows, classes, dtype=torch.float64) * 2, 1)
    if classes > 1:  # one row with one entry ~ 1 and the rest ~ 1e-8 (as softmax_inputs; not the first row, whose loss
        p[rows // 2] = 1e-8  # from a slab must show)
        p[rows // 2, classes // 2] = 1.0 - 1e-8 * (classes - 1)
    o.p = p.float()
    return o
