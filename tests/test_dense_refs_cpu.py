"""CPU: the float64 references of the dense-layer kernels (``dense_refs.py``) are the derivatives autograd takes of a
``Linear`` + activation; an fp32 evaluation of the header's formulas stays inside the forward bounds on the GPU tests'
own inputs; the wrong variants a kernel could plausibly compute fall outside them."""

import numpy as np
import pytest
import torch

import dense_refs as dr

ACTS = (dr.IDENTITY, dr.RELU, dr.TANH)
_ACT_MOD = {dr.IDENTITY: torch.nn.Identity, dr.RELU: torch.nn.ReLU, dr.TANH: torch.nn.Tanh}


def _f32(a):
    return np.asarray(a, dtype=np.float32)


# ---- fp32 evaluations of the header's formulas (separately rounded steps) ------------------------------------------
def tangent32(c, splits, with_tx=True, with_v=True):
    c_in = c["W"].shape[1]
    out = []
    for lo, hi in dr.split_ranges(c_in, splits):
        s = np.zeros((c["x"].shape[0], c["W"].shape[0]), np.float32)
        if with_tx:
            s = s + c["t_x"][:, lo:hi] @ c["W"][:, lo:hi].T
        if with_v:
            s = s + c["x"][:, lo:hi] @ c["V"][:, lo:hi].T
        out.append(_f32(s))
    return np.stack(out)


def act32(s, y, act):
    if act == dr.RELU:
        return np.where(y > 0, s, np.float32(0))
    if act == dr.TANH:
        return _f32(s * _f32(np.float32(1) - _f32(y * y)))
    return s


def slabsum32(slabs):
    s = slabs[0]
    for k in range(1, len(slabs)):
        s = _f32(s + slabs[k])
    return s


def act_tangent32(slabs, v_b, y, act):
    s = slabsum32(slabs)
    if v_b is not None:
        s = _f32(s + v_b[None, :])
    return act32(s, y, act)


def act_adjoint32(slabs, y, act, scale):
    ga = act32(slabsum32(slabs), y, act)
    return ga, _f32(_f32(ga.astype(np.float64).sum(0)) * np.float32(scale))


# ---- anchoring: the references ARE the derivatives of Linear + activation -----------------------------------------
@pytest.mark.parametrize("act", ACTS)
def test_references_are_autograd_derivatives_of_linear_plus_activation(act):
    rows, c_in, c_out = 5, 7, 4
    c = dr.case(rows, c_in, c_out, seed=3)
    t = lambda k: torch.tensor(c[k], dtype=torch.float64)  # noqa: E731
    x, W, b = t("x"), t("W"), t("v_b") * 0.5
    fn = lambda x_, W_, b_: _ACT_MOD[act]()(x_ @ W_.T + b_)  # noqa: E731
    y = fn(x, W, b)
    _, jv = torch.autograd.functional.jvp(fn, (x, W, b), (t("t_x"), t("V"), t("v_b")))
    for splits in (1, 1 + (c_in > dr.KSTEP)):
        slabs, _, _ = dr.tangent_slabs(c["t_x"], c["x"], c["W"], c["V"], splits)
        got, _ = dr.act_tangent(slabs, c["v_b"], y.numpy(), act)
        assert np.abs(got - jv.numpy()).max() < 1e-12
    gy = t("g")
    _, (gx, gW, gb) = torch.autograd.functional.vjp(fn, (x, W, b), gy)
    ga, _, g_b, _ = dr.act_adjoint(c["g"][None], y.numpy(), act, 1.0)
    assert np.abs(g_b - gb.numpy()).max() < 1e-12
    gw, _, _ = dr.wgrad(ga, c["x"], 1.0)
    assert np.abs(gw - gW.numpy()).max() < 1e-12
    d, _, _ = dr.dgrad_slabs(ga, c["W"], 1)
    assert np.abs(d.sum(0) - gx.numpy()).max() < 1e-12
    # the forward GEMM is the tangent kernel with t_x = NULL, V = W
    fwd, _, _ = dr.tangent_slabs(None, c["x"], c["W"], c["W"], 1)
    assert np.abs(fwd[0] - (x @ W.T).numpy()).max() < 1e-12


def test_split_rule_matches_the_header():
    assert dr.split_ok(1, 1) and not dr.split_ok(1, 2) and not dr.split_ok(64, 3) and dr.split_ok(65, 3)
    assert dr.split_ok(1024, 32) and not dr.split_ok(1 << 20, 33) and not dr.split_ok(10, 0)
    for length in (1, 31, 32, 33, 260, 3072):
        for s in range(1, dr.MAX_SPLITS + 1):
            if dr.split_ok(length, s):
                rng = dr.split_ranges(length, s)
                assert rng[0][0] == 0 and rng[-1][1] == length and all(lo < hi for lo, hi in rng)
                assert all(a[1] == b[0] for a, b in zip(rng, rng[1:])) and all(lo % dr.KSTEP == 0 for lo, _ in rng)


# ---- fp32 evaluations stay inside the bounds on the GPU tests' inputs; wrong variants do not ---------------------------
@pytest.mark.parametrize("shape", dr.SHAPES)
def test_fp32_gemms_stay_inside_the_bound_and_wrong_variants_do_not(shape):
    rows, c_in, c_out = shape
    c = dr.case(*shape)
    for splits in dr.split_counts(c_in, 1):
        want, M, L = dr.tangent_slabs(c["t_x"], c["x"], c["W"], c["V"], splits)
        assert dr.ratio(tangent32(c, splits), want, M, L + dr.R_SLAB) < 1
        # the V term dropped
        assert dr.ratio(tangent32(c, splits, with_v=False), want, M, L + dr.R_SLAB) > 1
    for splits in dr.split_counts(c_out, 1):
        want, M, L = dr.dgrad_slabs(c["g"], c["W"], splits)
        got = np.stack([_f32(c["g"][:, lo:hi] @ c["W"][lo:hi]) for lo, hi in dr.split_ranges(c_out, splits)])
        assert dr.ratio(got, want, M, L + dr.R_SLAB) < 1
    want, M, L = dr.wgrad(c["g"], c["x"], c["scale"])
    got = _f32(_f32(c["g"].T @ c["x"]) * np.float32(c["scale"]))
    assert dr.ratio(got, want, M, L + dr.R_WGRAD) < 1
    # scale applied twice
    assert dr.ratio(_f32(got * np.float32(c["scale"])), want, M, L + dr.R_WGRAD) > 1


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", dr.SHAPES)
def test_fp32_elementwise_passes_stay_inside_the_bound_and_wrong_variants_do_not(shape, act):
    rows, _, c = shape
    cs = dr.case(*shape)
    y, v_b = cs["y"][act], cs["v_b"]
    for splits in (1, 2, 5):
        slabs = dr.slabs_for((rows, c), splits)
        want, M = dr.act_tangent(slabs, v_b, y, act)
        R = dr.r_act(splits, True, act)
        assert dr.ratio(act_tangent32(slabs, v_b, y, act), want, M, R) < 1
        ga, Ma, gb, Mb = dr.act_adjoint(slabs, y, act, cs["scale"])
        got_a, got_b = act_adjoint32(slabs, y, act, cs["scale"])
        assert dr.ratio(got_a, ga, Ma, dr.r_act(splits, False, act)) < 1
        assert dr.ratio(got_b, gb, Mb, dr.r_bias(splits, act)) < 1
        # scale applied twice to the bias gradient
        assert dr.ratio(_f32(got_b * np.float32(cs["scale"])), gb, Mb, dr.r_bias(splits, act)) > 1
        if splits > 1:  # a slab dropped
            assert dr.ratio(act_tangent32(slabs[:-1], v_b, y, act), want, M, R) > 1
        if c > 1:  # the neighbouring column's bias
            assert dr.ratio(act_tangent32(slabs, np.roll(v_b, 1), y, act), want, M, R) > 1
    slabs = dr.slabs_for((rows, c), 2)
    want, M = dr.act_tangent(slabs, v_b, y, act)
    if act == dr.RELU and (y == 0).any():  # the mask y >= 0 lets the clipped entries through
        wrong = np.where(y >= 0, _f32(slabsum32(slabs) + v_b[None, :]), np.float32(0))
        assert dr.ratio(wrong, want, M, dr.r_act(2, True, act)) > 1
    if act == dr.TANH:  # 1 - y instead of 1 - y*y
        wrong = _f32(_f32(slabsum32(slabs) + v_b[None, :]) * _f32(np.float32(1) - y))
        assert dr.ratio(wrong, want, M, dr.r_act(2, True, act)) > 1
