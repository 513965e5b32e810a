"""CPU: the closed form of ``gn2_refs.adjoint2`` against ``torch.autograd``: the jvp of the first-order GroupNorm adjoint
(statistics as functions of ``a``) along ``(t, g', v_gamma)``, both in float64 -- the anchor of the kernel test's reference."""

import pytest
import torch
from torch.autograd.functional import jvp

import gn2_refs
import gn_refs
from layer_refs import U64, ratio

EPS = 1e-5


@pytest.mark.parametrize("n, hw, c, groups", [(3, 6, 24, 3), (2, 1, 16, 4)], ids=str)
def test_closed_form_is_autograds_jvp_of_the_adjoint(n, hw, c, groups):
    gen = torch.Generator().manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)  # noqa: E731
    a, g, gp, t, gamma, vg = rnd(n, hw, c), rnd(n, hw, c), rnd(n, hw, c), rnd(n, hw, c), rnd(c), rnd(c)
    Eg = lambda z: gn_refs.E(z, groups)  # noqa: E731

    def adjoint(a, g, gamma):
        d = a - Eg(a)
        rs = (Eg(d * d) + EPS) ** -0.5
        xh, p = d * rs, gamma * g
        ga = rs * (p - Eg(p) - xh * Eg(p * xh))
        return ga, (g * xh).sum(1), g.sum(1), ga.sum(1)

    want = jvp(adjoint, (a, g, gamma), (t, gp, vg))[1]
    fw = gn_refs.forward(a[None], None, gamma, 0 * gamma, EPS, groups, relu=False)
    got = gn2_refs.adjoint2(gp[None], t[None], None, a, g, fw.mean, fw.rstd, gamma, vg, None, groups)
    # the same float64 quantity by two routes of about R roundings each (torch sums pairwise: chains of log2(terms))
    R = gn2_refs.r_adjoint2(1, max(1, (hw * c // groups - 1).bit_length()), max(1, (hw - 1).bit_length()))
    worst = [ratio(w, getattr(got, k), getattr(got, "M" + k), 2 * getattr(R, k), U64)
             for w, k in zip(want, ("ga", "gw", "gb", "gcb"))]
    print("closed form vs autograd jvp, largest |diff| / (2 R 2^-53 M):", worst)
    assert max(worst) <= 1
