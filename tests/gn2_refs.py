"""float64 reference of ``hf_gn_act_adjoint2`` (the tangent of the GroupNorm adjoint; formulas: ``include/hf_pcg.h``) in
``gn_refs.py``'s convention: next to each result its magnitude map ``M``; ``r_adjoint2``: the roundings on the longest path,
from the arithmetic chain in ``hf_gn.hip``'s header.  ``g``: the first-order masked cotangent, a map as given."""

from types import SimpleNamespace as NS

from gn_refs import E, _masked, _slabs, _xhat
from layer_refs import up


def adjoint2(gy2, ta, v_cb, a, g, mean, rstd, gamma, vg, mask, groups):
    gy2, ta, v_cb, a, g, mean, rstd, gamma, vg, mask = (up(x) for x in (gy2, ta, v_cb, a, g, mean, rstd, gamma, vg, mask))
    Eg = lambda z: E(z, groups)  # noqa: E731
    (gp, Mgp), (t, Mt), (xh, Mxh, rs) = _masked(mask, *_slabs(gy2, None)), _slabs(ta, v_cb), _xhat(a, mean, rstd)
    p, Mp, pp, Mpp = gamma * g, (gamma * g).abs(), gamma * gp, gamma.abs() * Mgp
    if vg is not None:
        pp, Mpp = pp + vg * g, Mpp + (vg * g).abs()
    Tx, MTx, Px, MPx = Eg(xh * t), Eg(Mxh * Mt), Eg(p * xh), Eg(Mp * Mxh)
    tau, Mtau = t - Eg(t) - xh * Tx, Mt + Eg(Mt) + Mxh * MTx
    ga, Mga = rs * (p - Eg(p) - xh * Px), rs * (Mp + Eg(Mp) + Mxh * MPx)
    Qs, MQs = Eg(pp * xh) + rs * Eg(p * tau), Eg(Mpp * Mxh) + rs * Eg(Mp * Mtau)
    ga2 = rs * (pp - Eg(pp) - xh * Qs - rs * tau * Px) - rs * Tx * ga
    Mga2 = rs * (Mpp + Eg(Mpp) + Mxh * MQs + rs * Mtau * MPx) + rs * MTx * Mga
    return NS(ga=ga2, Mga=Mga2, gb=gp.sum(1), Mgb=Mgp.sum(1), gw=(gp * xh + g * rs * tau).sum(1),
              Mgw=(Mgp * Mxh + g.abs() * rs * Mtau).sum(1), gcb=ga2.sum(1), Mgcb=Mga2.sum(1))


def r_adjoint2(splits, L, Lr):
    """Both slab operands in ``splits`` slabs; ``v_conv_bias`` and ``v_gamma`` counted as given (the longest path).  A sum or
    difference: the larger count of its terms + 1; a product: both counts + 1; a mean: + the chain + its one rounding."""
    r_g, r_t, xh = splits - 1, splits, 2
    r_pp = r_g + 2                                          # gamma g' (1) + v_gamma g (the sum: 1)
    T1, Tx, Px = r_t + L + 1, r_t + xh + 1 + L + 1, 1 + xh + 1 + L + 1
    tau = max(T1 + 1, xh + Tx + 1) + 1                      # (t - T1) - xh * Tx
    Qt = (1 + tau + 1) + L + 1 + 1                          # rstd * E[p tau]
    Qs = max(r_pp + xh + 1 + L + 1, Qt) + 1                 # Qx + Qt
    rt, ga = tau + 1, L + 10                                # rstd * tau;  ga as in gn_refs.r_adjoint
    inner = max(max(r_pp + L + 1 + 1, xh + Qs + 1) + 1, rt + Px + 1) + 1
    r_ga2 = max(inner + 1, (Tx + 1) + ga + 1) + 1           # rstd * inner - rT * ga
    return NS(ga=r_ga2, gb=r_g + Lr + 1, gw=max(r_g + xh + 1, rt + 1) + 1 + Lr + 1, gcb=r_ga2 + Lr + 1)
