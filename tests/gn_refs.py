"""float64 references of the GroupNorm kernels (``hf_gn.hip``), written from the formulas in ``include/hf_pcg.h``, in the
convention of ``layer_refs.py``: next to each result its magnitude map ``M`` (the same computation on absolute values,
first-order through the statistics), and ``r_*``: the roundings on the longest path, read off the arithmetic chains in
the kernel file's header.  The bound of a comparison is ``layer_refs.ratio(got, want, M, R) <= 1``.

Layout: activations [n, hw, c], slabs [S, n, hw, c], statistics [n, groups], per-channel vectors [c].  Plain module."""

from types import SimpleNamespace as NS

import torch

from layer_refs import up


def E(t, groups):
    """The mean over each (sample, group) block, broadcast back to [n, hw, c]."""
    n, hw, c = t.shape
    m = t.reshape(n, hw, groups, c // groups).mean(dim=(1, 3), keepdim=True)
    return m.expand(n, hw, groups, c // groups).reshape(n, hw, c)


stat = lambda t, groups: t[:, 0, ::t.shape[2] // groups]  # noqa: E731  ([n, hw, c] constant per block -> [n, groups])
spread = lambda s, c: s.repeat_interleave(c // s.shape[1], dim=1)[:, None, :]  # noqa: E731  ([n, groups] -> [n, 1, c])
# terms of a lane's fp32 chain, at most: in a group reduction (a team has at least 64 lanes), and down the pixels in the
# row reduction of a workgroup that owns ``span`` channels
chain = lambda hw, cg: -(-hw * cg // 256)  # noqa: E731
row_chain = lambda hw, span: -(-hw // (256 // min(span // 4, 256)))  # noqa: E731


def _slabs(a, extra):
    s, M = a.sum(0), a.abs().sum(0)
    return (s, M) if extra is None else (s + extra, M + extra.abs())


def _xhat(a, mean, rstd):
    mu, rs = spread(mean, a.shape[2]), spread(rstd, a.shape[2])
    return (a - mu) * rs, (a.abs() + mu.abs()) * rs, rs


def _masked(mask, *ts):
    return ts if mask is None else tuple(torch.where(mask > 0, t, torch.zeros_like(t)) for t in ts)


def forward(a, cbias, gamma, beta, eps, groups, relu):
    a, cbias, gamma, beta = (up(t) for t in (a, cbias, gamma, beta))
    s, Ms = _slabs(a, cbias)
    mu, Mmu = E(s, groups), E(Ms, groups)
    d, Md = s - mu, Ms + Mmu
    var, Mvar = E(d * d, groups), E(Md * Md, groups)
    rstd = (var + eps) ** -0.5
    Mrstd = 0.5 * rstd ** 3 * Mvar + rstd
    y, My = d * rstd * gamma + beta, (Md * rstd + d.abs() * Mrstd) * gamma.abs() + beta.abs()
    if relu:
        y = y.clamp_min(0)
    return NS(s=s, Ms=Ms, mean=stat(mu, groups), Mmean=stat(Mmu, groups), rstd=stat(rstd, groups),
              Mrstd=stat(Mrstd, groups), y=y, My=My)


def r_forward(splits, has_cbias, L):
    """s | mean: + chain + its one rounding | d = s - mean | var: 2 r_d (a square) + product + chain | rstd: one rounding,
    counted by M's ``+ rstd`` | y: xhat, * gamma, + beta."""
    r_s = splits - 1 + int(has_cbias)
    r_mean = r_s + L + 1
    r_var = 2 * (r_mean + 1) + 1 + L
    return NS(s=r_s, mean=r_mean, rstd=r_var, y=r_var + 3)


def tangent(ta, v_cb, a, mean, rstd, gamma, vg, vb, mask, groups):
    ta, v_cb, a, mean, rstd, gamma, vg, vb, mask = (up(t) for t in (ta, v_cb, a, mean, rstd, gamma, vg, vb, mask))
    t, Mt = _slabs(ta, v_cb)
    xh, Mxh, rs = _xhat(a, mean, rstd)
    r = gamma * rs * (t - E(t, groups) - xh * E(xh * t, groups))
    M = gamma.abs() * rs * (Mt + E(Mt, groups) + Mxh * E(Mxh * Mt, groups))
    if vg is not None:
        r, M = r + vg * xh, M + vg.abs() * Mxh
    if vb is not None:
        r, M = r + vb, M + vb.abs()
    return _masked(mask, r, M)


def r_tangent(splits, has_vcb, L):
    """t | E[xhat t]: xhat 2, product 1, chain, 1 | xhat * it: 2 + 1 | the difference 1 | gamma*rstd and the product 2 |
    + v_gamma xhat 1 | + v_beta 1."""
    return (splits - 1 + int(has_vcb)) + L + 12


def adjoint(gy, a, mean, rstd, gamma, mask, groups):
    gy, a, mean, rstd, gamma, mask = (up(t) for t in (gy, a, mean, rstd, gamma, mask))
    g, Mg = _masked(mask, *_slabs(gy, None))
    xh, Mxh, rs = _xhat(a, mean, rstd)
    p, Mp = gamma * g, gamma.abs() * Mg
    ga = rs * (p - E(p, groups) - xh * E(p * xh, groups))
    Mga = rs * (Mp + E(Mp, groups) + Mxh * E(Mp * Mxh, groups))
    return NS(g=g, Mg=Mg, ga=ga, Mga=Mga, gb=g.sum(1), Mgb=Mg.sum(1), gw=(g * xh).sum(1), Mgw=(Mg * Mxh).sum(1),
              gcb=ga.sum(1), Mgcb=Mga.sum(1))


def r_adjoint(splits, L, Lr):
    """g | ga: p 1, E[p xhat]: + xhat 2 + product 1 + chain + 1, xhat * it 2 + 1, the difference 1, * rstd 1 | the rows:
    the element's roundings + the chain down the pixels + the store."""
    r_g = splits - 1
    r_ga = r_g + L + 10
    return NS(g=r_g, ga=r_ga, gb=r_g + Lr + 1, gw=r_g + 3 + Lr + 1, gcb=r_ga + Lr + 1)


def rows_sqsum(rows, pre):
    """out[c] = sum_n (pre * rows[n, c])^2 and its magnitude (itself); R = 4: t (twice through the square), the square,
    the store (the sum itself is fp64)."""
    out = ((pre * up(rows)) ** 2).sum(0)
    return out, out
