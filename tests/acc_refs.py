"""The float64 reference of ``HessianFree.acc_step()``'s accumulated quantities: plain autograd on the CPU, written from
the definition (reference optimizer.py:608-684: ``result += eval_mb`` per chunk) and without any of the session's code.

Per data list the accumulation of a per-chunk quantity ``q_k`` is ``sum_k N_k q_k / sum_k N_k`` (``mean``) or
``sum_k q_k`` (``sum``), one term per OCCURRENCE of a chunk in its list.  The loss function is called as the user wrote
it -- a regulariser included, so under ``sum`` it counts once per occurrence."""

import torch


def _params(model):
    return [p for p in model.parameters() if p.requires_grad]


def _flat(ts):
    return torch.cat([t.reshape(-1) for t in ts])


def _split(v, params):
    out, o = [], 0
    for p in params:
        out.append(v[o:o + p.numel()].reshape(p.shape))
        o += p.numel()
    return out


def _f64(x, t):
    return x.detach().cpu().double(), (t.detach().cpu().double() if t.is_floating_point() else t.detach().cpu())


def loss_hessian(outputs, targets, reduction):
    """``d^2 loss / d outputs^2`` in closed form, per sample ``[N, C, C]`` (the loss couples no two samples): softmax
    cross-entropy (class-index targets) ``diag(p) - p p^T``, squared error (float targets) ``2 I``; ``mean`` divides by
    what the loss divides by -- ``N`` resp. ``N * C``."""
    n, c = outputs.shape
    if targets.is_floating_point():
        h = 2.0 * torch.eye(c, dtype=outputs.dtype).expand(n, c, c)
        return h / (n * c) if reduction == "mean" else h
    p = torch.softmax(outputs.detach(), 1)
    h = torch.diag_embed(p) - p[:, :, None] * p[:, None, :]
    return h / n if reduction == "mean" else h


def jvp(outputs, params, vs):
    """``(d outputs / d params) v`` by double backward: the derivative of ``u -> J^T u`` with respect to ``u``."""
    u = torch.zeros_like(outputs, requires_grad=True)
    jtu = torch.autograd.grad(outputs, params, grad_outputs=u, create_graph=True, allow_unused=True)
    pairs = [(g, v) for g, v in zip(jtu, vs) if g is not None]
    (out,) = torch.autograd.grad([g for g, _ in pairs], u, grad_outputs=[v for _, v in pairs])
    return out.detach()


def ggn_product(outputs, targets, params, vs, reduction):
    """``J^T H_L J v``, flat.  A regulariser adds nothing: it does not depend on the outputs."""
    hjv = torch.einsum("nij,nj->ni", loss_hessian(outputs, targets, reduction), jvp(outputs, params, vs))
    g = torch.autograd.grad(outputs, params, grad_outputs=hjv, retain_graph=True, allow_unused=True)
    return _flat([torch.zeros_like(p) if x is None else x for x, p in zip(g, params)]).detach()


def hessian_product(loss, params, vs):
    """``(d^2 loss / d params^2) v`` by double backward, flat."""
    g = torch.autograd.grad(loss, params, create_graph=True, allow_unused=True)
    dot = sum((x * v).sum() for x, v in zip(g, vs) if x is not None)
    h = torch.autograd.grad(dot, params, allow_unused=True)
    return _flat([torch.zeros_like(p) if x is None else x for x, p in zip(h, params)]).detach()


def _accumulated(datalist, reduction, q):
    total, count = 0.0, 0
    for x, t in datalist:
        x, t = _f64(x, t)
        n = t.shape[0]
        total = total + (n * q(x, t) if reduction == "mean" else q(x, t))
        count += n
    return total / count if reduction == "mean" else total


def accumulate(model64, lossf, loss_dl, grad_dl, mvp_dl, reduction, curvature, v, trial_delta=None):
    """``dict(loss=, grad=, product=, trial_loss=)`` in float64 (``trial_loss``: ``None`` without ``trial_delta``):
    the loss list's loss, the gradient list's gradient, the curvature list's product ``curvature`` ("ggn" or "hessian")
    with the flat vector ``v``, and the loss list's loss at ``theta + trial_delta``.  ``model64``: a float64 copy of the
    stock model (its mode is left alone: a train-mode BatchNorm normalises every chunk with that chunk's statistics);
    ``lossf``: the loss function as the user wrote it, on ``model64`` where it reads parameters."""
    assert reduction in ("mean", "sum") and curvature in ("ggn", "hessian")
    params = _params(model64)
    assert all(p.dtype == torch.float64 for p in params)
    vs = _split(v.detach().cpu().double(), params)

    def loss_of(x, t):
        with torch.no_grad():
            return lossf(model64(x), t).detach()

    def grad_of(x, t):
        g = torch.autograd.grad(lossf(model64(x), t), params, allow_unused=True)
        return _flat([torch.zeros_like(p) if y is None else y for y, p in zip(g, params)])

    def product_of(x, t):
        out = model64(x)
        if curvature == "hessian":
            return hessian_product(lossf(out, t), params, vs)
        return ggn_product(out, t, params, vs, reduction)

    res = dict(loss=float(_accumulated(loss_dl, reduction, loss_of)), grad=_accumulated(grad_dl, reduction, grad_of),
               product=_accumulated(mvp_dl, reduction, product_of), trial_loss=None)
    if trial_delta is not None:
        saved = [p.detach().clone() for p in params]
        with torch.no_grad():
            for p, d in zip(params, _split(trial_delta.detach().cpu().double(), params)):
                p.add_(d)
        try:
            res["trial_loss"] = float(_accumulated(loss_dl, reduction, loss_of))
        finally:
            with torch.no_grad():
                for p, s in zip(params, saved):
                    p.copy_(s)
    return res
