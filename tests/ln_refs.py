"""float64 references of the LayerNorm kernels (``hf_ln.hip``), written from the formulas in ``include/hf_pcg.h``, in the
convention of ``gn_refs.py``: next to each result its magnitude map ``M`` (the same computation on absolute values,
first-order through the statistics), and ``r_*``: the roundings on the longest path, read off the arithmetic chains in
the kernel file's header.  The bound of a comparison is ``layer_refs.ratio(got, want, M, R) <= 1``.

Layout: activations [rows, c], slabs [S, rows, c], ``rstd`` [rows], per-column vectors [c].  Plain module."""

from types import SimpleNamespace as NS

import torch

from layer_refs import up

RELU, TANH = 1, 2
E = lambda t: t.mean(1, keepdim=True)  # noqa: E731
# terms of a lane's fp32 chain: its quads of the row, 64 lanes per row up to 1024 features, 256 beyond
chain = lambda c: -(-(-(-c // 4)) // (64 if c <= 1024 else 256))  # noqa: E731
# a | mu: + chain + its one rounding | d = a - mu | var: 2 r_d (a square) + product + chain | rstd: one rounding, counted by
# M's ``+ rstd`` | xh: the product | y: * gamma, + beta (tanhf itself: 2 ulp = 4 u of |y|, below any R here)
r_rstd = lambda splits, has_b, L: 2 * (splits - 1 + int(has_b) + L + 2) + 1 + L  # noqa: E731
r_forward = lambda splits, has_b, L: NS(rstd=r_rstd(splits, has_b, L), xh=r_rstd(splits, has_b, L) + 1,  # noqa: E731
                                        y=r_rstd(splits, has_b, L) + 3)
# t | E[xh t]: product 1, chain, 1 | xh * it 1 | the difference 1 | * rstd 1 | * gamma 1 | + v_gamma xh 1 | + v_beta 1 | tanh:
# the factor 2, the product 1
r_tangent = lambda splits, has_vb, L, act: splits - 1 + int(has_vb) + L + 8 + 3 * (act == TANH)  # noqa: E731
# s: the slabs (tanh: + 3) | q = gamma s 1 | E[q xh]: product 1, chain, 1 | xh * it 1 | the difference 1 | * rstd 1
r_adjoint = lambda splits, L, act: NS(s=splits - 1 + 3 * (act == TANH), ga=splits - 1 + 3 * (act == TANH) + L + 6)  # noqa: E731


def _slabs(a, extra):
    s, M = a.sum(0), a.abs().sum(0)
    return (s, M) if extra is None else (s + extra, M + extra.abs())


def _act_apply(s, Ms, y, act):
    """``hf_dense_act.h::act_apply``: ``s * act'(y)``; tanh's factor ``1 - y*y`` is formed in fp32 (magnitude 1 + y*y)."""
    if act == RELU:
        return torch.where(y > 0, s, torch.zeros_like(s)), torch.where(y > 0, Ms, torch.zeros_like(Ms))
    return (s * (1 - y * y), Ms * (1 + y * y)) if act == TANH else (s, Ms)


def _centred(t, Mt, xh, rs):
    """``rstd * (t - E[t] - xh * E[xh t])`` and its magnitude."""
    return rs * (t - E(t) - xh * E(xh * t)), rs * (Mt + E(Mt) + xh.abs() * E(xh.abs() * Mt))


def forward(a, b, gamma, beta, eps, act):
    a, b, gamma, beta = (up(t) for t in (a, b, gamma, beta))
    s, Ms = _slabs(a, b)
    d, Md = s - E(s), Ms + E(Ms)
    rstd = (E(d * d) + eps) ** -0.5
    Mrstd = 0.5 * rstd ** 3 * E(Md * Md) + rstd
    xh, Mxh = d * rstd, Md * rstd + d.abs() * Mrstd
    y, My = xh * gamma + beta, Mxh * gamma.abs() + beta.abs()
    if act == RELU:
        y = y.clamp_min(0)
    if act == TANH:
        y = torch.tanh(y)
        My = (1 - y * y) * My + y.abs()
    return NS(rstd=rstd[:, 0], Mrstd=Mrstd[:, 0], xh=xh, Mxh=Mxh, y=y, My=My)


def tangent(ta, vb, xh, rstd, gamma, vg, vbeta, y, act):
    ta, vb, xh, rstd, gamma, vg, vbeta, y = (up(t) for t in (ta, vb, xh, rstd, gamma, vg, vbeta, y))
    tx, Mtx = _centred(*_slabs(ta, vb), xh, rstd[:, None])
    r, M = gamma * tx, gamma.abs() * Mtx
    if vg is not None:
        r, M = r + vg * xh, M + vg.abs() * xh.abs()
    if vbeta is not None:
        r, M = r + vbeta, M + vbeta.abs()
    return _act_apply(r, M, y, act)


def adjoint(gy, xh, rstd, gamma, y, act):
    gy, xh, rstd, gamma, y = (up(t) for t in (gy, xh, rstd, gamma, y))
    s, Ms = _act_apply(*_slabs(gy, None), y, act)
    ga, Mga = _centred(gamma * s, gamma.abs() * Ms, xh, rstd[:, None])
    return NS(s=s, Ms=Ms, ga=ga, Mga=Mga)


def param_sums(s, xh, ga, scale, squared):
    """``(o_gamma, o_beta, o_b)`` of the operands as given, each with its magnitude; ``scale`` exact in fp32.  R = 4: the
    product s * xh, the rounding of the fp64 sum, the scale (squared: 5, the product counts twice)."""
    terms = [t * t if squared else t for t in (up(s) * up(xh), up(s), up(ga))]
    return [(scale * t.sum(0), abs(scale) * t.abs().sum(0)) for t in terms]
