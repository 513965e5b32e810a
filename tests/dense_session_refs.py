"""Numpy references of the dense-stack session's two kernels (``hf_dense_act_forward``, ``hf_dense_loss_head`` of
``hf_dense.hip``) in the rounding order ``include/hf_pcg.h`` states: every fp32 operation is one numpy float32 operation,
every fp64 accumulation a float64 one (numpy adds pairwise where the kernels use a fixed tree: the two differ by parts
in 1e16, far below the one rounding to fp32 that follows).  ``expf`` / ``tanhf`` are numpy's float32 ones, so results
that pass through them agree with the kernels to rounding, not to the bit; everything else does to the bit.

No torch, no GPU: ``test_dense_session_refs_cpu.py`` checks these against float64, the GPU tests use them."""

import numpy as np

IDENTITY, RELU, TANH = 0, 1, 2
CE, MSE = 0, 1
F32 = np.float32
U32 = 2.0 ** -24


def slab_sum(slabs, b=None):
    """slab 0, then slabs 1 .. n-1 in split order, then the bias: one fp32 rounding per addition."""
    slabs = np.asarray(slabs, dtype=F32)
    s = slabs[0].copy()
    for k in range(1, slabs.shape[0]):
        s = (s + slabs[k]).astype(F32)
    if b is not None:
        s = (s + np.asarray(b, dtype=F32)[None, :]).astype(F32)
    return s


def act_forward(slabs, b, act):
    """``hf_dense_act_forward``: ``act(sum of slabs + b)``; relu is ``s <= 0 ? +0 : s`` (a NaN stays a NaN)."""
    s = slab_sum(slabs, b)
    if act == RELU:
        return np.where(s <= 0, F32(0.0), s).astype(F32)
    if act == TANH:
        return np.tanh(s).astype(F32)
    return s


def ce_head(logits, targets, scale_g, scale_ps, reduction):
    """``hf_dense_loss_head``, kind 0.  Returns ``(p, dl, dl_ps, loss, flag)``."""
    x = np.asarray(logits, dtype=F32)
    t = np.asarray(targets, dtype=np.int64)
    rows, c = x.shape
    m = x.max(1, keepdims=True)
    e = np.exp((x - m).astype(F32)).astype(F32)
    S = e.astype(np.float64).sum(1)
    p = (e / S.astype(F32)[:, None]).astype(F32)
    ok = (t >= 0) & (t < c)
    onehot = np.zeros_like(p)
    onehot[np.nonzero(ok)[0], t[ok]] = 1.0
    d = (p - onehot).astype(F32)
    dl = (d * F32(scale_g)).astype(F32)
    dl_ps = (d * F32(scale_ps)).astype(F32)
    x_t = x[np.arange(rows), np.where(ok, t, 0)].astype(np.float64)
    terms = np.where(ok, np.log(S) - (x_t - m[:, 0].astype(np.float64)), 0.0)
    total = 0.0
    for v in terms:  # rows in ascending order
        total += float(v)
    coef = 1.0 / rows if reduction == "mean" else 1.0
    return p, dl, dl_ps, F32(total * coef), int((~ok).any())


def mse_head(out, targets, scale_g, scale_ps, reduction):
    """``hf_dense_loss_head``, kind 1.  Returns ``(dl, dl_ps, loss, flag)``."""
    x, t = np.asarray(out, dtype=F32), np.asarray(targets, dtype=F32)
    d = (x - t).astype(F32)
    dl = (d * F32(scale_g)).astype(F32)
    dl_ps = (d * F32(scale_ps)).astype(F32)
    d64 = d.astype(np.float64)
    coef = 1.0 / d.size if reduction == "mean" else 1.0
    return dl, dl_ps, F32(F32((d64 * d64).sum()) * F32(coef)), 0


def loss_scales(kind, rows, c, reduction):
    """``(scale_g, scale_ps, coef)`` of a plain loss: ``d loss / d logits = d * scale_g``, the per-sample cotangent
    ``d * scale_ps`` (a ``mean`` loss carries 1/N, ``loss(model(x_i), t_i)`` does not), ``loss = coef * sum``."""
    mean = reduction == "mean"
    if kind == CE:
        g, coef = (1.0 / rows if mean else 1.0), (1.0 / rows if mean else 1.0)
    else:
        g, coef = (2.0 / (rows * c) if mean else 2.0), (1.0 / (rows * c) if mean else 1.0)
    return g, g * (rows if mean else 1.0), coef


def logits_case(rows, c, seed=0, scale=3.0, offset=0.0):
    """fp32 logits of spread ``scale`` (+ ``offset``) and class indices, from a seed."""
    g = np.random.default_rng(100003 * seed + 1009 * rows + c)
    x = (scale * g.standard_normal((rows, c)) + offset).astype(F32)
    return x, g.integers(0, c, size=rows).astype(np.int64)


def mse_case(rows, c, seed=0):
    g = np.random.default_rng(200003 * seed + 1013 * rows + c)
    return g.standard_normal((rows, c)).astype(F32), g.standard_normal((rows, c)).astype(F32)
