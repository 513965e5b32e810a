"""float64 references of the pooled TRAIN-mode BatchNorm unit's kernels (``hf_pool_bn_act_tangent_train_nhwc`` /
``hf_pool_bn_act_adjoint_reduce_nhwc``, include/hf_pcg.h) and the seeded operands of their tests.

Both are compositions of references that exist: the tangent is ``layer_refs.chan_affine_train`` (the dense train-mode
tangent, unmasked) gathered at the windows' positions and masked by the pooled map; the reduction pass is
``pool_bn_act_refs.adjoint`` without its ``ga``; the whole two-pass adjoint is that followed by ``chan_affine_train`` on
``g`` and the partial rows.  ``test_pool_bn_train_refs_cpu.py`` anchors them to autograd through
``max_pool2d(relu(batch_norm(a, training=True)))``.

Layouts are the kernels': NHWC, ``idx`` int [n, oh, ow, c] holding the flat position ``y*w + x`` of the window's maximum;
partial rows [nparts, c]."""

import torch

import layer_refs as L
import pool_act_refs as R
import pool_bn_act_refs as B

EPS = 1e-5
# (kernel, stride, padding), (h, w): overlapping 3/2 windows on 5x5 -> 2x2 (row / column 2 in two windows each, the
# centre in four); 2/2 windows on 6x4 -> 3x2 (every pixel in exactly one).  A pixel that is no window's maximum gets no
# cotangent and is never read by the tangent: most pixels of both.
GEOMS = [((3, 2, 0), (5, 5)), ((2, 2, 0), (6, 4))]
AXIS_GEOMS = R.AXIS_GEOMS  # per-axis windows, ((kh, kw), (sh, sw), (ph, pw)), (h, w): every function below takes pairs
BLOCK, FCS_BATCH = 256, 8  # hf_common.h; HF_FCS_BATCH of hf_bn.hip


def nparts_choices(c):
    """1, 3 and one count above what the prologue keeps in flight per pass (HF_FCS_BATCH x row groups)."""
    return (1, 3, FCS_BATCH * (BLOCK // (c // 4)) + 5)


def batch_stats(a, dtype=torch.float32):
    """(mean, rstd) over (n, h, w) of ``a`` [n,h,w,c], biased variance: computed in float64, rounded to ``dtype``."""
    a = a.double()
    var, mean = torch.var_mean(a, dim=(0, 1, 2), unbiased=False)
    return mean.to(dtype), torch.rsqrt(var + EPS).to(dtype)


def partial_rows(total, nparts, gen):
    """``nparts`` rows that add up to ``total`` [c] (float64) up to rounding, all of its sign: positive random shares."""
    share = torch.rand(nparts, 1, generator=gen, dtype=torch.float64) + 0.1
    return (share / share.sum()) * total.double()[None]


def case(n, c, h, w, k, s, p, splits, gy_splits, nparts, tag=""):
    """Seeded standard-normal operands: ``pool_bn_act_refs.case`` with ``mean`` / ``rstd`` the batch statistics of ``a``
    (fp32), a positive scale, a shift that masks a share of the windows, and -- fp32 -- the partial rows of the tangent's
    sums  S_x = sum_rows xhat*T,  S_1 = sum_rows T  (T: the sum of the slabs), as ``nparts`` positive shares."""
    o = B.case(n, c, h, w, k, s, p, splits, gy_splits, exact=False, tag=f"train{tag}")
    gen = torch.Generator().manual_seed(R._seed("pool-bn-train", n, c, h, w, k, s, p, splits, gy_splits, nparts, tag))
    o["mean"], o["rstd"] = batch_stats(o["a"])
    o["b"] = -0.6 + 0.5 * torch.randn(c, generator=gen)
    T = o["slabs"].double().sum(0)
    o["count"] = float(n * h * w)
    o["S_x"], o["S_1"] = (B.xhat(o) * T).sum((0, 1, 2)), T.sum((0, 1, 2))
    o["part_x"] = partial_rows(o["S_x"], nparts, gen).float()
    o["part_1"] = partial_rows(o["S_1"], nparts, gen).float()
    return o


def dense_tangent(o, v_w, v_b, part_x=None, part_1=None):
    """``hf_chan_affine_train``'s unmasked dense output (t, M), float64 [n,h,w,c]."""
    return L.chan_affine_train(o["slabs"], o["a"], o["mean"], o["rstd"], o["w"], o["part_x"] if part_x is None else part_x,
                               o["part_1"] if part_1 is None else part_1, v_w, v_b, o["count"], None, None)


def gather_mask(t, idx, y_pool, relu):
    """t [n,h,w,c] at ``idx`` [n,oh,ow,c], zero where the pooled map is not positive (with ``relu``)."""
    n, h, w, c = t.shape
    _, oh, ow, _ = idx.shape
    out = torch.gather(t.reshape(n, h * w, c), 1, idx.reshape(n, oh * ow, c).long()).reshape(n, oh, ow, c)
    return torch.where(y_pool > 0, out, torch.zeros_like(out)) if relu else out


def tangent(o, v_w, v_b, idx, y_pool, relu, part_x=None, part_1=None):
    """out[n,oy,ox,c] = m * (T[p]*(w*rstd) + xhat[p]*q + r),  p = idx,  q = v_w - k*S_x,  r = v_b - k*S_1,
    k = w*rstd/count; float64 (out, M)."""
    t, M = dense_tangent(o, v_w, v_b, part_x, part_1)
    return gather_mask(t, idx, y_pool, relu), gather_mask(M, idx, y_pool, relu)


def adjoint_reduce(o, idx, y_pool, relu, h, w, k, s, p, row_blocks):
    """Pass 1: ``pool_bn_act_refs.adjoint``'s g / gw / gb (and their magnitudes); its ga is not part of this form."""
    r = B.adjoint(o, idx, y_pool, relu, h, w, k, s, p, row_blocks)
    r.pop("ga")
    return r


def adjoint(o, idx, y_pool, relu, h, w, k, s, p, row_blocks, drop_x=False, drop_1=False):
    """Both passes: g_a = (w*rstd) * (g - mean(g) - xhat * mean(g*xhat)), as ``hf_chan_affine_train`` forms it from g and
    the partial rows of pass 1.  ``drop_*``: without that correction (what the eval formula would give)."""
    r = adjoint_reduce(o, idx, y_pool, relu, h, w, k, s, p, row_blocks)
    gw, gb = r["gw"] * (0.0 if drop_x else 1.0), r["gb"] * (0.0 if drop_1 else 1.0)
    ga, Mga = L.chan_affine_train(r["g"][None], o["a"], o["mean"], o["rstd"], o["w"], gw, gb, None, None, o["count"], None,
                                  None)
    r.update(ga=ga, Mga=Mga)
    return r
