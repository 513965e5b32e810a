"""CPU: the float64 references of the diagonal empirical-Fisher kernels (``dense_diag_refs.py``), chained over a stack,
ARE ``sum_i g_i^2`` of a per-sample autograd loop in float64; an fp32 evaluation of the header's formulas stays inside the
bounds on the GPU tests' own inputs; the wrong variants a kernel could plausibly compute fall outside them."""

import numpy as np
import pytest
import torch

import dense_diag_refs as ddr
import dense_refs as dr
from pytorchhessianfree_amd import testproblems as tp

_ACT = {torch.nn.ReLU: dr.RELU, torch.nn.Tanh: dr.TANH}


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def _layers(model):
    """``stack_diag``'s description of a ``Linear [ReLU | Tanh] ...`` model."""
    leaves = [m for m in model.modules() if not list(m.children())]
    out = []
    for i, m in enumerate(leaves):
        if isinstance(m, torch.nn.Linear):
            act = _ACT.get(type(leaves[i + 1]), dr.IDENTITY) if i + 1 < len(leaves) else dr.IDENTITY
            b = None if m.bias is None else m.bias.detach().numpy()
            out.append((m.weight.detach().numpy(), b, act,
                        (m.weight.requires_grad, m.bias is not None and m.bias.requires_grad)))
    return out


def _loop64(model, lossf, x, t):
    """sum_i g_i^2 by one backward pass per sample, float64 (the reference's diag_EF_autograd, unscaled)."""
    params = [p for p in model.parameters() if p.requires_grad]
    diag = torch.zeros(sum(p.numel() for p in params), dtype=torch.float64)
    for i in range(x.shape[0]):
        g = torch.autograd.grad(lossf(model(x[i:i + 1]), t[i:i + 1]), params)
        diag += torch.cat([q.reshape(-1) for q in g]) ** 2
    return diag.numpy()


def _tanh_ce():
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(11, 6), torch.nn.Tanh(), torch.nn.Linear(6, 5, bias=False), torch.nn.Tanh(),
                              torch.nn.Linear(5, 4))
    gen = torch.Generator().manual_seed(1)
    return net, (torch.rand(9, 11, generator=gen), torch.randint(0, 4, (9,), generator=gen)), torch.nn.CrossEntropyLoss


@pytest.mark.parametrize("problem", ["small_nn", "small_nn_all", "tanh_ce"])
@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_references_are_the_per_sample_loop_in_float64(problem, reduction):
    if problem == "tanh_ce":
        model, (x, t), loss_cls = _tanh_ce()
    else:
        model, (x, t), _ = tp.small_nn(batch_size=7, freeze_layer1=problem == "small_nn")
        loss_cls = torch.nn.MSELoss
    model, x = model.double(), x.double()
    t = t.double() if t.dtype.is_floating_point else t
    lossf = loss_cls(reduction=reduction)
    n = x.shape[0]
    want = _loop64(model, lossf, x, t) * (1.0 / n if reduction == "mean" else 1.0)
    # the engine's cotangents: d loss / d outputs of the WHOLE batch, times N for a `mean` loss
    out = model(x)
    (dl,) = torch.autograd.grad(lossf(out, t), out)
    g = dl.numpy() * (n if reduction == "mean" else 1.0)
    got = ddr.stack_diag(_layers(model), x.numpy(), g, 1.0 / n if reduction == "mean" else 1.0)  # (frozen: no entries)
    assert got.shape == want.shape
    # (scale goes through fp32 in the references, as in the kernels: 1/7 and 1/9 are not fp32 numbers)
    assert np.abs(got - want).max() <= 2.0 ** -23 * np.abs(want).max()


def sq_wgrad32(g, x, scale):
    g2, x2 = _f32(g * g), _f32(x * x)
    return _f32(_f32(g2.T @ x2) * np.float32(scale))


def sq_colsum32(g, scale):
    g64 = g.astype(np.float64)
    return _f32(_f32((g64 * g64).sum(0)) * np.float32(scale))


@pytest.mark.parametrize("shape", dr.SHAPES)
def test_fp32_evaluations_stay_inside_the_bound_and_wrong_variants_do_not(shape):
    rows, c_in, c_out = shape
    c = dr.case(*shape)
    g, x = c["g"], c["x"]
    for scale in (1.0, 1.0 / rows):
        want, M, L = ddr.sq_wgrad(g, x, scale)
        assert dr.ratio(sq_wgrad32(g, x, scale), want, M, L + ddr.R_SQ_WGRAD) < 1
        want_b, Mb = ddr.sq_colsum(g, scale)
        assert dr.ratio(sq_colsum32(g, scale), want_b, Mb, ddr.R_SQ_COLSUM) < 1
        # x left unsquared
        assert dr.ratio(_f32(_f32(_f32(g * g).T @ x) * np.float32(scale)), want, M, L + ddr.R_SQ_WGRAD) > 1
        # g_a left unsquared in the column sum
        assert dr.ratio(_f32(_f32(g.astype(np.float64).sum(0)) * np.float32(scale)), want_b, Mb, ddr.R_SQ_COLSUM) > 1
        if rows > 1:  # the last row dropped (an odd row count's tail)
            assert dr.ratio(sq_wgrad32(g[:-1], x[:-1], scale), want, M, L + ddr.R_SQ_WGRAD) > 1
            assert dr.ratio(sq_colsum32(g[:-1], scale), want_b, Mb, ddr.R_SQ_COLSUM) > 1
            # scale applied twice
            if scale != 1.0:
                assert dr.ratio(_f32(sq_wgrad32(g, x, scale) * np.float32(scale)), want, M, L + ddr.R_SQ_WGRAD) > 1
