"""Diagonal empirical-Fisher preconditioner (reference
``hessianfree/preconditioners.py:11-159``, Martens' recipe
``M^-1 x = (diag + lambda)^-0.75 * x``).

Differences in mechanism, not in result:

* ``diag_to_preconditioner`` returns a :class:`DiagonalPreconditioner` whose
  power is evaluated ONCE by the ``hf_precond_build`` kernel (the reference
  re-evaluates ``(diag+damping)**-exponent`` inside every CG iteration,
  preconditioners.py:124-125) and whose multiply is fused into the PCG kernels;
* ``diag_EF_autograd`` accumulates ``g_i**2`` with the multi-tensor
  ``hf_pack(mode=1)`` kernel straight from autograd's per-parameter outputs
  (no ``torch.cat`` of every per-sample gradient, preconditioners.py:98);
* ``diag_EF_backpack`` keeps its name for drop-in compatibility but does not
  need BackPACK: the per-sample gradients come from one batched
  ``torch.func.vmap(grad)`` pass.  Like BackPACK's version it only sees the part
  of the loss that flows through ``loss_function(model(x), t)``.  For a prepared
  MLP with ``HF_DENSE_ENGINE=1`` no per-sample gradient is formed at all: the
  dense-stack engine's ``diag_ef`` (own kernels, one adjoint sweep) answers.
"""

import torch

from . import _lib
from .cg import DiagonalPreconditioner
from .curvature import flatten_into


def _check_reduction(reduction):
    if reduction not in ["sum", "mean"]:
        raise ValueError(f"reduction {reduction} is not supported.")


def _accumulate_squares(diag, grads, params):
    """diag += concat(grads)**2"""
    if diag.is_cuda:
        dense = [torch.zeros_like(p) if g is None else g.detach() for g, p in zip(grads, params)]
        _lib.pack(diag, dense, scale=1.0, mode=1)
    else:
        diag += flatten_into(grads, params) ** 2
    return diag


def diag_EF_autograd(model, loss_function, inputs, targets, reduction):
    """``sum_i g_i^2`` (``sum``) or ``(1/N) sum_i g_i^2`` (``mean``) with one backward
    pass per sample (preconditioners.py:63-105)."""
    _check_reduction(reduction)
    params = [p for p in model.parameters() if p.requires_grad]
    n = sum(p.numel() for p in params)
    diag = torch.zeros(n, dtype=params[0].dtype, device=params[0].device)
    for x_i, t_i in zip(inputs, targets):
        loss_i = loss_function(model(x_i), t_i)
        g_i = torch.autograd.grad(loss_i, params, retain_graph=False, allow_unused=True)
        _accumulate_squares(diag, g_i, params)
    if reduction == "mean":
        diag = diag / inputs.shape[0]
    return diag


def diag_EF_backpack(model, loss_function, inputs, targets, reduction, why=None):
    """Same quantity from ONE batched per-sample-gradient pass (the role BackPACK's
    ``SumGradSquared`` plays in preconditioners.py:11-60).  A prepared MLP with ``HF_DENSE_ENGINE=1``
    takes the dense-stack engine's closed form instead (``engine.dense.diag_ef_of``: one adjoint sweep,
    no per-sample gradient); ``why`` (a list) receives the reason whenever it does not."""
    _check_reduction(reduction)
    from .engine.dense import diag_ef_of

    diag = diag_ef_of(model, loss_function, inputs, targets, reduction, why=why)
    if diag is not None:
        return diag
    return _diag_EF_vmap(model, loss_function, inputs, targets, reduction)


def _diag_EF_vmap(model, loss_function, inputs, targets, reduction):
    """``diag_EF_backpack`` by ``torch.func.vmap(grad)``: materialises the per-sample gradients."""
    from torch.func import functional_call, grad, vmap

    names, params = [], []
    for name, p in model.named_parameters():
        if p.requires_grad:
            names.append(name)
            params.append(p)
    frozen = {k: v for k, v in model.named_parameters() if not v.requires_grad}
    buffers = dict(model.named_buffers())

    def sample_loss(train, x, t):
        state = {**frozen, **buffers, **dict(zip(names, train))}
        out = functional_call(model, state, (x.unsqueeze(0),))
        return loss_function(out, t.unsqueeze(0))

    try:
        per_sample = vmap(grad(sample_loss), in_dims=(None, 0, 0))(tuple(params), inputs, targets)
    except Exception:  # op without a batching rule: fall back to the loop
        return diag_EF_autograd(model, loss_function, inputs, targets, reduction)
    squares = [torch.einsum("b...,b...->...", g, g) for g in per_sample]
    scale = 1.0 / inputs.shape[0] if reduction == "mean" else 1.0
    return flatten_into(squares, params, scale=scale)


def diag_to_preconditioner(diag_vec, damping, exponent=0.75):
    """Callable computing ``(diag_vec + damping)^-exponent * x``
    (preconditioners.py:108-127)."""
    return DiagonalPreconditioner(diag_vec, damping, exponent)


def diag_EF_preconditioner(model, loss_function, inputs, targets, reduction, damping,
                           exponent=None, use_backpack=True):
    """preconditioners.py:130-159."""
    fn = diag_EF_backpack if use_backpack else diag_EF_autograd
    diag = fn(model, loss_function, inputs, targets, reduction)
    if exponent is None:
        return diag_to_preconditioner(diag, damping)
    return diag_to_preconditioner(diag, damping, exponent)
