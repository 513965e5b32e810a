"""CPU: the float64 references of ``pool_bn_act_refs`` against ``torch.autograd.functional``'s ``jvp`` / ``vjp`` of
``max_pool2d(relu(batch_norm_eval(a)))`` with respect to ``a``, ``w`` and ``b`` -- and, for the dyadic operands of the GPU
kernel tests, that every reference value is an fp32 number (the GPU tests then compare bitwise)."""

import pytest
import torch

import pool_bn_act_refs as B

CASES = [((3, 2, 0), (5, 7), 4, 1), ((2, 2, 0), (4, 4), 12, 0), ((3, 2, 1), (5, 7), 3, 1), ((3, 3, 1), (3, 3), 6, 1),
         ((2, 1, 0), (4, 4), 4, 0)]


def _unit(o, k, s, p, relu):
    """The unit as a float64 function of (a, w, b), NCHW inside."""
    mean, rstd = o["mean"].double(), o["rstd"].double()

    def f(a, w, b):
        z = ((a - mean) * rstd) * w + b
        z = torch.relu(z) if relu else z
        return torch.nn.functional.max_pool2d(z.permute(0, 3, 1, 2), k, s, p).permute(0, 2, 3, 1)
    return f


AXIS_CASES = [(geom, hw, c, relu) for geom, hw in B.AXIS_GEOMS for c in (4, 3) for relu in (0, 1)]


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("geom, hw, c, relu", CASES + AXIS_CASES)
def test_references_equal_autograd(geom, hw, c, relu, exact):
    (k, s, p), (h, w), n = geom, hw, 2
    o = B.case(n, c, h, w, k, s, p, 2, 3, exact=exact)
    y_pool, idx = B.forward(o, k, s, p, relu)
    f = _unit(o, k, s, p, relu)
    prim = (o["a"].double(), o["w"].double(), o["b"].double())
    t_a = o["slabs"].double().sum(0)
    _, jv = torch.autograd.functional.jvp(f, prim, (t_a, o["v_w"].double(), o["v_b"].double()))
    want, M = B.tangent(o, o["v_w"], o["v_b"], idx, y_pool, relu)
    assert float((want - jv).abs().max()) <= 1e-12 * float(M.max())
    # (frozen scale / shift: the terms drop out)
    _, jv0 = torch.autograd.functional.jvp(f, prim, (t_a, torch.zeros(c, dtype=torch.float64),
                                                     torch.zeros(c, dtype=torch.float64)))
    want0, _ = B.tangent(o, None, None, idx, y_pool, relu)
    assert float((want0 - jv0).abs().max()) <= 1e-12 * float(M.max())
    rb = 3
    r = B.adjoint(o, idx, y_pool, relu, h, w, k, s, p, rb)
    _, (ga, gw, gb) = torch.autograd.functional.vjp(f, prim, o["gy"].double().sum(0))
    scale = max(1.0, float(r["M"].max()))
    assert float((r["ga"] - ga).abs().max()) <= 1e-12 * scale * 4
    assert float((r["gb"].sum(0) - gb).abs().max()) <= 1e-12 * float(r["Mb"].sum(0).max() + 1)
    assert float((r["gw"].sum(0) - gw).abs().max()) <= 1e-12 * float(r["Mw"].sum(0).max() + 1)
    # g is the cotangent of the BatchNorm's output: ga without the scale
    assert torch.equal(r["ga"], r["g"] * (o["w"].double() * o["rstd"].double()))


def test_dyadic_references_are_fp32_numbers():
    """On the GPU tests' dyadic operands the float64 references round to themselves in fp32 -- tangent, g, ga, gw, gb, at
    the largest split counts and share sizes those tests use -- so a bitwise comparison asks for the exact result."""
    def fp32(t):
        return torch.equal(t.float().double(), t)

    for (k, s, p), (h, w) in [(g, m) for g in B.GEOMS for m in B.MAPS] + B.AXIS_GEOMS:
        for relu in (0, 1):
            o = B.case(2, 4, h, w, k, s, p, 9, 9)
            y_pool, idx = B.forward(o, k, s, p, relu)
            assert fp32(B.tangent(o, o["v_w"], o["v_b"], idx, y_pool, relu)[0])
            r = B.adjoint(o, idx, y_pool, relu, h, w, k, s, p, 1)
            assert all(fp32(r[name]) for name in ("g", "ga", "gw", "gb"))
    for c in (258, 1028):  # the wide cases of the row-sum kernel: n = 1, shares of up to 16 rows
        o = B.case(1, c, 4, 4, 2, 2, 0, 1, 2)
        y_pool, idx = B.forward(o, 2, 2, 0, 1)
        r = B.adjoint(o, idx, y_pool, 1, 4, 4, 2, 2, 0, 1)
        assert all(fp32(r[name]) for name in ("g", "ga", "gw", "gb"))


def test_the_cases_mask_windows():
    masked = 0
    for (k, s, p) in B.GEOMS:
        for (h, w) in B.MAPS:
            o = B.case(2, 4, h, w, k, s, p, 1, 1)
            y_pool, _ = B.forward(o, k, s, p, 1)
            masked += bool((y_pool <= 0).any()) and bool((y_pool > 0).any())
    assert masked >= 8


@pytest.mark.parametrize("geom, hw, c, relu", AXIS_CASES)
def test_per_axis_cases_tell_an_exchanged_window_apart(geom, hw, c, relu):
    """Every output of the adjoint -- g, ga and both sum rows -- computed with (kh, kw), (sh, sw) or (ph, pw) exchanged in
    the window predicate alone differs from the right one (without the ReLU as well: the pooled no-ReLU unit)."""
    (k, s, p), (h, w) = geom, hw
    o = B.case(2, c, h, w, k, s, p, 1, 2)
    y_pool, idx = B.forward(o, k, s, p, relu)
    r = B.adjoint(o, idx, y_pool, relu, h, w, k, s, p, 1)
    assert B.R.exchanges(geom)
    for name, (k2, s2, p2) in B.R.exchanges(geom):
        r2 = B.adjoint(o, idx, y_pool, relu, h, w, k2, s2, p2, 1)
        for out in ("g", "ga", "gw", "gb"):
            assert not torch.equal(r2[out], r[out]), (name, out)


def test_the_per_axis_cases_mask_windows():
    for (k, s, p), (h, w) in B.AXIS_GEOMS:
        for c in (4, 3):
            o = B.case(2, c, h, w, k, s, p, 1, 1)
            y_pool, _ = B.forward(o, k, s, p, 1)
            assert bool((y_pool <= 0).any()) and bool((y_pool > 0).any())
