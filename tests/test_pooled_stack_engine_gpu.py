"""GPU: plain conv stacks with ``MaxPool2d`` layers on the plain-stack engine (``engine/plain.py``: a pooled unit's bias /
ReLU / pool is ONE launch per sweep direction, ``hf_pool_act_tangent_nhwc`` / ``hf_pool_act_adjoint_nhwc``), on
``testproblems.convpool_small`` -- the im2col'd first layer pooled (3x3 / stride 2, overlapping windows, 12x12 -> 5x5),
a second pooled layer (2x2 / stride 2 on the odd 5x5 map), an unpooled last layer.

Reference sides (``stack_harness.py``): float64 autograd of the STOCK model on the engine's own ReLU and pooling decisions
(replayed, and bounded: a replayed decision may differ from the float64 model's own only within rounding of a tie), and
the fixture the real reference wrote (``tests/golden/convnet_convpool.npz``, ``make_golden_convpool.py``).  Bounds are the
ones ``test_engine_gpu.py`` states for All-CNN-C: 1e-6 (GGN) and 2e-6 (Hessian, gradient, logits, diagonal) against
float64, 1e-5 against the reference's fp32 results."""

import pytest
import torch
from tol import within

from helpers import RefTrace, compare_trace
from pytorchhessianfree_amd import testproblems as tp
from pytorchhessianfree_amd.engine import PlainStackEngine
from stack_harness import (DEV, _Net, check_point, declined_net, engine, float64_twin, grad64, product64, record_launches,
                           rel, run_steps)

pytestmark = pytest.mark.gpu
N_ALL = 844  # parameters of convpool_small


@pytest.mark.parametrize("batch", [2, 5])
@pytest.mark.parametrize("hessian", [False, True], ids=["ggn", "hessian"])
def test_products_gradient_logits_and_diagonal_match_float64_and_the_reference(batch, hessian):
    """``curvature.ggn_operator`` / ``hessian_operator`` of the prepared pooled stack IS a ``PlainStackEngine`` (without
    the pooled-layer support it is the autograd operator: this is the assertion that fails on the parent commit)."""
    op, model, (x, t), lossf, cpu_params = engine(tp.convpool_small, batch, hessian)
    assert isinstance(op, PlainStackEngine) and op.hessian == hessian
    assert [u.pool for u in op.units] == [(3, 3, 2, 2, 0, 0), (2, 2, 2, 2, 0, 0), None]
    assert op.units[0].im2col and op.n == N_ALL
    check_point(op, tp.convpool_small, batch, x, lossf, cpu_params, ("convpool", f"b{batch}"), f"b{batch}")


@pytest.mark.parametrize("batch", [2, 5])
def test_batched_diagonal_matches_float64_and_the_reference(batch, monkeypatch):
    """``HF_DIAG_EF_BATCHED=1``: one squared-sum launch per layer on the same cotangents."""
    monkeypatch.setenv("HF_DIAG_EF_BATCHED", "1")
    op, model, (x, t), lossf, _ = engine(tp.convpool_small, batch)
    assert isinstance(op, PlainStackEngine) and op._diag_batched
    ref = RefTrace("convpool", f"b{batch}")
    got_d = op.diag_ef("mean").clone()
    within(ref.vec_err64("diag", got_d), 2e-6)
    within(ref.vec_err("diag", got_d), 1e-5)
    assert torch.equal(op.diag_ef("mean"), got_d)


def test_a_pooled_layer_costs_four_launches_per_product(monkeypatch):
    """The launches of one GGN product, counted as ``test_dense_launch_order_gpu.py`` does (a proxy around the library):
    per layer the tangent convolution, ONE bias / ReLU (/ pool) tangent launch, ONE adjoint launch, the convolution's
    gradients -- 4, pooled or not; the stem's max-pool launches and, for the pooled units, ``hf_chan_affine_ex`` do not
    appear."""
    names = record_launches(monkeypatch)
    op, *_ = engine(tp.convpool_small, 2)
    assert isinstance(op, PlainStackEngine) and names
    v = torch.randn(op.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(6))
    del names[:]
    op.local(v)
    torch.cuda.synchronize()
    got = list(names)
    once = {"hf_pool_ce_head", "hf_pack_ex", "hf_bn_sums_multi", "hf_unpack_tangent_ex", "hf_unpack_weights"}
    per_layer = [n for n in got if n not in once]
    assert len(per_layer) == 4 * len(op.units), got
    assert got.count("hf_pool_act_tangent_nhwc") == 2 and got.count("hf_pool_act_adjoint_nhwc") == 2, got
    assert got.count("hf_chan_affine_ex") == 1, got  # (the unpooled last layer's)
    assert "hf_maxpool_tangent_nhwc" not in got and "hf_maxpool_adjoint_nhwc" not in got, got
    assert all(got.count(n) <= 1 for n in once), got
    # the sequence: tangent sweep in layer order, head, adjoint sweep in reverse
    order = [n for n in got if n.startswith(("hf_pool_act", "hf_chan_affine", "hf_bn_adjoint", "hf_pool_ce"))]
    assert order[:3] == ["hf_pool_act_tangent_nhwc", "hf_pool_act_tangent_nhwc", "hf_chan_affine_ex"], order
    assert order[3] == "hf_pool_ce_head" and order[-2:] == ["hf_pool_act_adjoint_nhwc"] * 2, order


def test_three_default_steps_through_the_session_match_the_reference_trace():
    """``HessianFree(graph_matvec=True).step()`` on the pooled stack runs on the persistent session (own forward pass with
    the pool launches, loss head, gradient sweep, graphed products); the three-step trace against the real reference's at
    the bounds of the All-CNN-C trace (``compare_trace``'s defaults)."""
    seeds = (21, 22, 23)  # (make_golden_convpool.STEP_SEEDS: the reference's fp32 and float64 traces agree there)
    opt, finals, _, ref = run_steps(tp.convpool_small, seeds, 2, ("convpool", "steps"), graph_matvec=True)
    assert opt._session is not None and opt._session.steps == 3
    assert isinstance(opt._session.engine, PlainStackEngine)
    compare_trace(opt.state, finals, ref)


def _freeze_first(model):
    conv = next(m for m in model.modules() if isinstance(m, torch.nn.Conv2d))
    for p in conv.parameters():
        p.requires_grad_(False)


@pytest.mark.parametrize("hessian", [False, True], ids=["ggn", "hessian"])
def test_frozen_first_convolution(hessian):
    """The pooled first layer frozen: dead for both sweeps (its pooled map is a constant input of the second layer, which
    needs no data gradient); the product on the trainable subset against float64, the frozen tensors untouched."""
    op, model, (x, t), lossf, _ = engine(tp.convpool_small, 2, hessian, prep=_freeze_first)
    assert isinstance(op, PlainStackEngine) and op.dead_units == 1 and op.n == N_ALL - (8 * 27 + 8)
    conv = next(m for m in model.modules() if isinstance(m, torch.nn.Conv2d))
    before = [p.detach().clone() for p in conv.parameters()]
    v = torch.randn(op.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(8))
    got = op(v).clone()
    assert torch.equal(op(v), got)
    p64, out64, loss64, _ = float64_twin(tp.convpool_small, 2, op, prep=_freeze_first)
    within(rel(got, product64(p64, out64, loss64, v, hessian)), 2e-6 if hessian else 1e-6)
    within(rel(op.gradient(), grad64(loss64, p64)), 2e-6)
    op.diag_ef("mean")
    assert all(torch.equal(a, b.detach()) and b.grad is None for a, b in zip(before, conv.parameters()))


def _declined_variants():
    C, R, P, A, G = torch.nn.Conv2d, torch.nn.ReLU, torch.nn.MaxPool2d, torch.nn.AvgPool2d, torch.nn.AdaptiveAvgPool2d
    return {
        "pool_before_gap": (lambda: _Net([C(3, 8, 3, 1, 1), R(), C(8, 4, 1), P(2, 2), G(1)]), "MaxPool2d behind conv1"),
        "relu_behind_pool": (lambda: _Net([C(3, 8, 3, 1, 1), P(2, 2), R(), C(8, 4, 1), G(1)]), "ReLU behind the MaxPool2d"),
        "avgpool": (lambda: _Net([C(3, 8, 3, 1, 1), R(), A(2, 2), C(8, 4, 1), G(1)]), "AvgPool2d"),
        "ceil_mode": (lambda: _Net([C(3, 8, 3, 1, 1), R(), P(3, 2, ceil_mode=True), C(8, 4, 1), G(1)]),
                      "MaxPool2d behind conv0"),
        "dilation": (lambda: _Net([C(3, 8, 3, 1, 1), R(), P(2, 2, dilation=2), C(8, 4, 1), G(1)]), "MaxPool2d behind conv0"),
        "detour": (lambda: _Net([C(3, 8, 3, 1, 1), R(), P(2, 2), C(8, 4, 1), G(1)], detour=True), "MaxPool2d behind conv0"),
    }


@pytest.mark.parametrize("name", sorted(_declined_variants()))
def test_declined_variants_keep_the_autograd_path_and_say_why(name):
    declined_net(*_declined_variants()[name])
