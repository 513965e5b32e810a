"""CPU: the float64 references of ``pool_bn_train_refs`` against autograd through
``max_pool2d(relu(batch_norm(a, training=True)))`` -- ``torch.func.jvp`` for the tangent, ``vjp`` for the two-pass adjoint
(the reduction pass composed with ``layer_refs.chan_affine_train``) -- and that they DISCRIMINATE: without either
batch-statistics correction (the eval formula) the outputs of the GPU test's inputs move by far more than its bound."""

import pytest
import torch

import layer_refs as L
import pool_bn_train_refs as T

B = T.B
CASES = [(geom, hw, c, relu) for geom, hw in T.GEOMS for c in (8, 12) for relu in (0, 1)]
AXIS_CASES = [(geom, hw, c, relu) for geom, hw in T.AXIS_GEOMS for c in (4, 3) for relu in (0, 1)]


def _exact(o):
    """The case with float64 statistics and exact float64 sums as ONE partial row: what autograd computes."""
    o = dict(o)
    o["mean"], o["rstd"] = T.batch_stats(o["a"], torch.float64)
    t_a = o["slabs"].double().sum(0)
    o["part_x"], o["part_1"] = (B.xhat(o) * t_a).sum((0, 1, 2))[None], t_a.sum((0, 1, 2))[None]
    return o, t_a


def _unit(k, s, p, relu):
    def f(a, w, b):
        z = torch.nn.functional.batch_norm(a.permute(0, 3, 1, 2), None, None, w, b, True, 0.0, T.EPS)
        z = torch.relu(z) if relu else z
        return torch.nn.functional.max_pool2d(z, k, s, p).permute(0, 2, 3, 1)
    return f


@pytest.mark.parametrize("geom, hw, c, relu", CASES + AXIS_CASES)
def test_references_equal_autograd(geom, hw, c, relu):
    (k, s, p), (h, w), n = geom, hw, 2
    o, t_a = _exact(T.case(n, c, h, w, k, s, p, 3, 3, 3))
    y_pool, idx = B.forward(o, k, s, p, relu)
    f = _unit(k, s, p, relu)
    prim = (o["a"].double(), o["w"].double(), o["b"].double())
    zero = torch.zeros(c, dtype=torch.float64)
    for v_w, v_b in ((o["v_w"], o["v_b"]), (None, o["v_b"]), (o["v_w"], None)):
        tang = (t_a, zero if v_w is None else v_w.double(), zero if v_b is None else v_b.double())
        y, jv = torch.func.jvp(f, prim, tang)
        assert torch.equal(y > 0, y_pool > 0) or not relu
        want, M = T.tangent(o, v_w, v_b, idx, y_pool, relu)
        assert float((want - jv).abs().max()) <= 1e-11 * float(M.max())
    rb = 3
    r = T.adjoint(o, idx, y_pool, relu, h, w, k, s, p, rb)
    _, pull = torch.func.vjp(f, *prim)
    ga, gw, gb = pull(o["gy"].double().sum(0))
    assert float((r["ga"] - ga).abs().max()) <= 1e-11 * float(r["Mga"].max())
    assert float((r["gb"].sum(0) - gb).abs().max()) <= 1e-11 * float(r["Mb"].sum(0).max() + 1)
    assert float((r["gw"].sum(0) - gw).abs().max()) <= 1e-11 * float(r["Mw"].sum(0).max() + 1)


def test_the_cases_mask_windows_and_leave_windows():
    for (k, s, p), (h, w) in T.GEOMS:
        for c in (8, 12):
            o = T.case(2, c, h, w, k, s, p, 1, 1, 1)
            y_pool, _ = B.forward(o, k, s, p, 1)
            assert bool((y_pool <= 0).any()) and bool((y_pool > 0).any())


@pytest.mark.parametrize("geom, hw", T.GEOMS)
@pytest.mark.parametrize("c", [8, 12])
def test_references_discriminate_the_batch_statistics_corrections(geom, hw, c):
    """On the GPU test's inputs: dropping the S_x or the S_1 correction of the tangent, or either mean of the adjoint's
    second pass, moves some output by more than 1000 times the bound the GPU test allows that element."""
    (k, s, p), (h, w), n, splits = geom, hw, 2, 3
    o = T.case(n, c, h, w, k, s, p, splits, 3, 3)
    y_pool, idx = B.forward(o, k, s, p, 1)
    want, M = T.tangent(o, o["v_w"], o["v_b"], idx, y_pool, 1)
    bound = L.r_chan_affine_train(splits, False) * L.U32 * M
    zx, z1 = torch.zeros_like(o["part_x"]), torch.zeros_like(o["part_1"])
    for name, kw in (("S_x", dict(part_x=zx)), ("S_1", dict(part_1=z1))):
        moved, _ = T.tangent(o, o["v_w"], o["v_b"], idx, y_pool, 1, **kw)
        ratio = float(((moved - want).abs() / bound.clamp_min(1e-300))[bound > 0].max())
        print(f"tangent without {name}: {ratio:.3g} x the bound")
        assert ratio > 1000
    r = T.adjoint(o, idx, y_pool, 1, h, w, k, s, p, 3)
    bound = L.r_chan_affine_train(1, False) * L.U32 * r["Mga"]
    for name, kw in (("mean(g*xhat)", dict(drop_x=True)), ("mean(g)", dict(drop_1=True))):
        moved = T.adjoint(o, idx, y_pool, 1, h, w, k, s, p, 3, **kw)["ga"]
        ratio = float(((moved - r["ga"]).abs() / bound.clamp_min(1e-300))[bound > 0].max())
        print(f"adjoint without {name}: {ratio:.3g} x the bound")
        assert ratio > 1000


@pytest.mark.parametrize("geom, hw, c, relu", AXIS_CASES)
def test_per_axis_cases_tell_an_exchanged_window_apart(geom, hw, c, relu):
    """The reduction pass (g and both sum rows) and the two-pass ga with (kh, kw), (sh, sw) or (ph, pw) exchanged in the
    window predicate alone move some element by more than 1000 times the bound the GPU test allows it."""
    (k, s, p), (h, w) = geom, hw
    o = T.case(2, c, h, w, k, s, p, 1, 3, 1)
    y_pool, idx = B.forward(o, k, s, p, relu)
    r = T.adjoint(o, idx, y_pool, relu, h, w, k, s, p, 3)
    R_ = 3 * r["windows"] + 2
    bounds = dict(g=R_ * L.U32 * r["M"], gb=R_ * L.U32 * r["Mb"], gw=(R_ + 4) * L.U32 * r["Mw"],
                  ga=L.r_chan_affine_train(1, False) * L.U32 * r["Mga"])
    assert T.R.exchanges(geom)
    for name, (k2, s2, p2) in T.R.exchanges(geom):
        r2 = T.adjoint(o, idx, y_pool, relu, h, w, k2, s2, p2, 3)
        for out, bound in bounds.items():
            ratio = float(((r2[out] - r[out]).abs() / bound.clamp_min(1e-300))[bound > 0].max())
            assert ratio > 1000, (name, out, ratio)
