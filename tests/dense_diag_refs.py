"""Float64 references of the two diagonal empirical-Fisher kernels of ``hf_dense.hip`` (``hf_dense_sq_wgrad``,
``hf_dense_sq_colsum``), written from the formulas in ``include/hf_pcg.h``, with the bounds the kernel tests hold them to,
and the whole-stack diagonal built from them.  Plain module, no GPU; conventions of ``dense_refs.py``.

Every term of either sum is non-negative, so the magnitude sum ``M`` of ``dense_refs`` is the result itself and the
forward bound ``(L + R) * u * M`` is an ENTRYWISE RELATIVE one, ``u = 2**-24``:

* ``sq_wgrad``: ``L = rows`` (an fp32 sum of ``rows`` products, fused or not), ``R = 3``: the squaring of ``g_a``, the
  squaring of ``x`` (one rounding each, relative, so they pass to every term) and the multiplication by ``scale``.
* ``sq_colsum``: ``L = 0`` -- the squares of fp32 numbers are exact in fp64 and the fp64 sum of ``rows <= 256`` of them
  errs by ``rows * 2**-53``, counted as one fp32 rounding (far more than it is) --, then the rounding to fp32 and the
  multiplication by ``scale``: ``R = 3``."""

import numpy as np

import dense_refs as dr

R_SQ_WGRAD = 3
R_SQ_COLSUM = 3


def sq_wgrad(g, x, scale):
    """hf_dense_sq_wgrad: ``scale * (g*g)^T (x*x)`` with ``scale`` rounded to fp32.  Returns (result, M, L)."""
    g, x, sc = dr.f64(g), dr.f64(x), float(np.float32(scale))
    out = sc * ((g * g).T @ (x * x))
    return out, out, g.shape[0]


def sq_colsum(g, scale):
    """hf_dense_sq_colsum: ``scale * column sums of g*g`` with ``scale`` rounded to fp32.  Returns (result, M)."""
    g, sc = dr.f64(g), float(np.float32(scale))
    out = sc * (g * g).sum(0)
    return out, out


def stack_diag(layers, x, g_logits, scale):
    """The engine's sweep in float64.  ``layers``: ``[(W, b or None, act, (w_trainable, b_trainable)), ...]`` in forward
    order; ``x`` the batch; ``g_logits`` the PER-SAMPLE cotangents at the network output; ``scale`` 1/N or 1.  Returns
    the concatenated diagonal over the trainable parameters in ``model.parameters()`` order (weight, then bias)."""
    xs, cur = [], dr.f64(x)
    for W, b, act, _ in layers:
        xs.append(cur)
        pre = cur @ dr.f64(W).T + (0.0 if b is None else dr.f64(b)[None, :])
        cur = {dr.IDENTITY: pre, dr.RELU: np.maximum(pre, 0.0), dr.TANH: np.tanh(pre)}[act]
        xs.append(cur)
    pieces, slab = [], dr.f64(g_logits)[None]
    for k in range(len(layers) - 1, -1, -1):
        W, b, act, (tw, tb) = layers[k]
        ga, _, _, _ = dr.act_adjoint(slab, xs[2 * k + 1], act, 1.0)
        here = []
        if tw:
            here.append(sq_wgrad(ga, xs[2 * k], scale)[0].reshape(-1))
        if b is not None and tb:
            here.append(sq_colsum(ga, scale)[0])
        pieces = here + pieces
        slab, _, _ = dr.dgrad_slabs(ga, W, 1)
    return np.concatenate(pieces) if pieces else np.zeros(0)
