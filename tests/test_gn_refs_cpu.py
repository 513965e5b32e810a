"""CPU: the three formulas of ``gn_refs.py`` against ``torch.autograd`` (forward, jvp and vjp of ``F.group_norm`` + ReLU in
float64) at one shape -- the anchor of the references the GroupNorm kernel tests use."""

import torch
import torch.nn.functional as F
from torch.autograd.functional import jvp, vjp

import gn_refs

N, HW, C, G, EPS = 3, 6, 24, 3, 1e-5


def test_references_are_autograds_group_norm():
    gen = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)  # noqa: E731
    a, gamma, beta, cb = rnd(2, N, HW, C), rnd(C), rnd(C), rnd(C)
    nchw = lambda t: t.permute(0, 2, 1)  # noqa: E731  ([n, hw, c] -> [n, c, hw])
    f = lambda x, w, b: F.relu(F.group_norm(nchw(x), G, w, b, EPS))  # noqa: E731
    x = a.sum(0) + cb
    fw = gn_refs.forward(a, cb, gamma, beta, EPS, G, relu=True)
    assert torch.allclose(nchw(fw.y), f(x, gamma, beta), rtol=0, atol=1e-12)
    t_a, v_cb, vg, vb = rnd(2, N, HW, C), rnd(C), rnd(C), rnd(C)
    want = jvp(f, (x, gamma, beta), (t_a.sum(0) + v_cb, vg, vb))[1]
    got, _ = gn_refs.tangent(t_a, v_cb, x, fw.mean, fw.rstd, gamma, vg, vb, fw.y, G)
    assert torch.allclose(nchw(got), want, rtol=0, atol=1e-12)
    gy = rnd(2, N, HW, C)
    gx, gw, gb = vjp(f, (x, gamma, beta), nchw(gy.sum(0)))[1]
    ad = gn_refs.adjoint(gy, x, fw.mean, fw.rstd, gamma, fw.y, G)
    assert torch.allclose(ad.ga, gx, rtol=0, atol=1e-12)
    assert torch.allclose(ad.gw.sum(0), gw, rtol=0, atol=1e-12) and torch.allclose(ad.gb.sum(0), gb, rtol=0, atol=1e-12)
    assert torch.allclose(ad.gcb.sum(0), gx.sum((0, 1)), rtol=0, atol=1e-12)
    assert torch.equal(gn_refs.rows_sqsum(ad.gw, 3.0)[0], ((3.0 * ad.gw) ** 2).sum(0))
