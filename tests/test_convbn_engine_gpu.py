"""GPU: plain conv stacks with eval-mode ``BatchNorm2d`` units on the plain-stack engine (``engine/plain.py``: an unpooled
BatchNorm unit runs on the shared BatchNorm launches, a pooled one's BatchNorm / ReLU / pool is ONE launch per sweep
direction, ``hf_pool_bn_act_tangent_nhwc`` / ``hf_pool_bn_act_adjoint_nhwc``), on ``testproblems.convbn_small`` -- the
im2col'd first unit pooled (3x3 / stride 2, 12x12 -> 5x5), an unpooled BatchNorm unit, a pooled one without a ReLU (2x2 /
stride 2 on the odd 5x5 map), a 1x1 bias layer -- and ``testproblems.convbn_fc_small`` (two pooled BatchNorm units in front
of a ``Flatten, Linear, ReLU, Linear`` tail).  The BatchNorm state is seeded (``testproblems.seed_batchnorm``).

Reference sides (``stack_harness.py``): float64 autograd of the STOCK model on the engine's own ReLU and pooling
decisions, and the fixture the real reference wrote (``tests/golden/convnet_convbn.npz``, ``make_golden_convbn.py``).
Bounds are the project's: 1e-6 (GGN) and 2e-6 (Hessian, gradient, logits, diagonal) against float64, 1e-5 against the
reference's fp32 results."""

import pytest
import torch
from tol import within

from helpers import RefTrace, compare_trace
from pytorchhessianfree_amd import curvature, modelprep
from pytorchhessianfree_amd import testproblems as tp
from pytorchhessianfree_amd.engine import FusedGGNEngine, PlainStackEngine
from stack_harness import (DEV, _Net, check_point, declined_net, diag64, engine, float64_twin, grad64, product64,
                           record_launches, rel, run_steps)

pytestmark = pytest.mark.gpu
N_SMALL, N_FC = 1764, 1694  # parameters of convbn_small / convbn_fc_small
# (make_golden_convbn.NETS: the reference's fp32 and float64 traces agree on these data seeds)
STEPS = {"small": (tp.convbn_small, (41, 42, 43), 2), "fc": (tp.convbn_fc_small, (61, 62, 63), 5)}
POOL_T, POOL_A = "hf_pool_bn_act_tangent_nhwc", "hf_pool_bn_act_adjoint_nhwc"


@pytest.mark.parametrize("batch", [2, 5])
@pytest.mark.parametrize("hessian", [False, True], ids=["ggn", "hessian"])
def test_convbn_small_is_a_plain_stack_engine_and_matches_float64_and_the_reference(batch, hessian):
    """``curvature.ggn_operator`` / ``hessian_operator`` of prepared ``convbn_small`` IS a ``PlainStackEngine`` (without
    the BatchNorm units it is the autograd operator, "unsupported layer BatchNorm2d": this is the assertion that fails on
    the parent commit)."""
    op, model, (x, t), lossf, cpu_params = engine(tp.convbn_small, batch, hessian)
    assert isinstance(op, PlainStackEngine) and op.hessian == hessian
    assert [u.pool for u in op.units] == [(3, 3, 2, 2, 0, 0), None, (2, 2, 2, 2, 0, 0), None]
    assert [type(u.bn).__name__ for u in op.units] == ["BatchNorm2d"] * 3 + ["NoneType"]
    assert [u.relu for u in op.units] == [True, True, False, False]
    assert op.units[0].im2col and op.n == N_SMALL and not op.classifier
    check_point(op, tp.convbn_small, batch, x, lossf, cpu_params, ("convbn", f"small/b{batch}"), f"small-b{batch}")


@pytest.mark.parametrize("batch", [2, 5])
def test_convbn_fc_small_runs_the_tail_behind_pooled_batchnorm_units(batch):
    op, model, (x, t), lossf, cpu_params = engine(tp.convbn_fc_small, batch)
    assert isinstance(op, PlainStackEngine) and not op.hessian
    assert [u.pool for u in op.units] == [(3, 3, 2, 2, 0, 0), (2, 2, 2, 2, 0, 0)] and op.n == N_FC
    assert all(isinstance(u.bn, torch.nn.BatchNorm2d) and u.relu for u in op.units)
    assert [(u.c_in, u.c_out, u.act) for u in op.classifier] == [(32, 20, 1), (20, 10, 0)]
    check_point(op, tp.convbn_fc_small, batch, x, lossf, cpu_params, ("convbn", f"fc/b{batch}"), f"fc-b{batch}")


def test_hessian_products_through_the_tail_stay_refused():
    op, *_ = engine(tp.convbn_fc_small, 2, hessian=True)
    assert type(op) is curvature.HessianOperator
    model, (x, t), lossf = tp.convbn_fc_small(batch_size=2, device=DEV)
    modelprep.prepare_model(model, channels_last=True)
    out, why = model(x), []
    assert FusedGGNEngine.try_build(lossf(out, t), out, list(model.parameters()), hessian=True, why=why) is None
    assert any("Hessian products through a classifier tail are not covered" in w for w in why), why


@pytest.mark.parametrize("family, batch", [("small", 2), ("small", 5), ("fc", 5)])
def test_batched_diagonal_matches_float64_and_the_reference(family, batch, monkeypatch):
    """``HF_DIAG_EF_BATCHED=1``: one squared-sum launch per layer on the same cotangents (a BatchNorm unit's: its stored
    unscaled ``g``)."""
    monkeypatch.setenv("HF_DIAG_EF_BATCHED", "1")
    make = STEPS[family][0]
    op, model, (x, t), lossf, _ = engine(make, batch)
    assert isinstance(op, PlainStackEngine) and op._diag_batched
    got_d = op.diag_ef("mean").clone()
    p64, out64, _loss64, t64 = float64_twin(make, batch, op)
    within(rel(got_d, diag64(lossf, p64, out64, t64, batch, op.n)), 2e-6)
    ref = RefTrace("convbn", f"{family}/b{batch}")
    within(ref.vec_err64("diag", got_d), 2e-6)
    within(ref.vec_err("diag", got_d), 1e-5)
    assert torch.equal(op.diag_ef("mean"), got_d)


@pytest.mark.parametrize("defer", ["1", "0"], ids=["deferred", "fused"])
def test_a_pooled_batchnorm_unit_costs_four_launches_per_product(defer, monkeypatch):
    """The launches of one GGN product, counted through a proxy around the library: per unit the tangent convolution, ONE
    BatchNorm / bias (/ ReLU / pool) tangent launch, ONE adjoint launch, the convolution's gradients -- 4, pooled or not,
    BatchNorm or bias -- and the head's one.  The first unit's map is large enough for its sums to leave the chain
    (``HF_BN_SUMS_DEFER``, the default): one ``hf_bn_sums_multi`` launch in front of the gather; switched off, none."""
    monkeypatch.setenv("HF_BN_SUMS_DEFER", defer)
    names = record_launches(monkeypatch)
    op, *_ = engine(tp.convbn_small, 2)
    assert isinstance(op, PlainStackEngine) and names
    assert [u.defer for u in op.units] == [defer == "1", False, False, False]
    v = torch.randn(op.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(6))
    del names[:]
    op.local(v)
    torch.cuda.synchronize()
    got = list(names)
    once = {"hf_pool_ce_head", "hf_pack_ex", "hf_bn_sums_multi", "hf_unpack_tangent_ex", "hf_unpack_weights"}
    per_unit = [n for n in got if n not in once]
    assert len(per_unit) == 4 * len(op.units), got
    assert got.count("hf_pool_ce_head") == 1 and got.count("hf_pack_ex") == 1, got
    assert got.count("hf_bn_sums_multi") == (1 if defer == "1" else 0), got
    assert got.count(POOL_T) == 2 and got.count(POOL_A) == 2, got
    assert "hf_pool_act_tangent_nhwc" not in got and "hf_pool_act_adjoint_nhwc" not in got, got
    assert got.count("hf_chan_affine_ex") == 2, got  # (the unpooled BatchNorm unit's and the bias layer's tangents)
    assert "hf_maxpool_tangent_nhwc" not in got and "hf_maxpool_adjoint_nhwc" not in got, got
    # the sequence: tangent sweep in layer order, head, adjoint sweep in reverse
    order = [n for n in got if n.startswith(("hf_pool_", "hf_chan_affine", "hf_bn_adjoint"))]
    assert order[:5] == [POOL_T, "hf_chan_affine_ex", POOL_T, "hf_chan_affine_ex", "hf_pool_ce_head"], order
    assert order[5:] == ["hf_chan_affine_bwd_ex", POOL_A, "hf_chan_affine_bwd_ex", POOL_A], order


def _freeze_first_unit(model):
    mods = list(model.net)
    for m in mods[:2]:  # the first convolution and its BatchNorm
        for p in m.parameters():
            p.requires_grad_(False)


def _freeze_scales(model):
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.requires_grad_(False)


@pytest.mark.parametrize("hessian", [False, True], ids=["ggn", "hessian"])
@pytest.mark.parametrize("prep", [_freeze_first_unit, _freeze_scales], ids=["first_unit", "scales"])
def test_frozen_parameters(prep, hessian):
    """The pooled first unit frozen (convolution, scale and shift: dead for both sweeps), and every BatchNorm's scale
    frozen (no ``v_w`` term, no scale sums; the shifts stay trainable): products, gradient and diagonal on the trainable
    subset against float64, the frozen tensors untouched."""
    op, model, (x, t), lossf, _ = engine(tp.convbn_small, 2, hessian, prep=prep)
    assert isinstance(op, PlainStackEngine)
    if prep is _freeze_first_unit:
        assert op.dead_units == 1 and op.n == N_SMALL - (8 * 27 + 16)
    else:
        assert op.dead_units == 0 and op.n == N_SMALL - 28 and all(u.pg is None for u in op.units)
    frozen = [p for p in model.parameters() if not p.requires_grad]
    before = [p.detach().clone() for p in frozen]
    v = torch.randn(op.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(8))
    got = op(v).clone()
    assert torch.equal(op(v), got)
    p64, out64, loss64, t64 = float64_twin(tp.convbn_small, 2, op, prep=prep)
    within(rel(got, product64(p64, out64, loss64, v, hessian)), 2e-6 if hessian else 1e-6)
    within(rel(op.gradient(), grad64(loss64, p64)), 2e-6)
    within(rel(op.diag_ef("mean"), diag64(lossf, p64, out64, t64, 2, op.n)), 2e-6)
    assert all(torch.equal(a, b.detach()) and b.grad is None for a, b in zip(before, frozen))


@pytest.mark.parametrize("family", sorted(STEPS))
def test_three_default_steps_through_the_session_match_the_reference_trace(family):
    """``HessianFree(graph_matvec=True).step()`` runs on the persistent session (own forward pass with the BatchNorm and
    pool launches, loss head, gradient sweep, graphed products); the three-step trace against the real reference's at
    ``compare_trace``'s defaults."""
    make, seeds, batch = STEPS[family]
    opt, finals, _, ref = run_steps(make, seeds, batch, ("convbn", f"{family}/steps"), graph_matvec=True)
    assert opt._session is not None and opt._session.steps == 3
    assert isinstance(opt._session.engine, PlainStackEngine)
    compare_trace(opt.state, finals, ref)


def _declined_variants():
    C, B, R, P, G = torch.nn.Conv2d, torch.nn.BatchNorm2d, torch.nn.ReLU, torch.nn.MaxPool2d, torch.nn.AdaptiveAvgPool2d
    nb = dict(bias=False)
    return {
        "conv_bias": (lambda: _Net([C(3, 8, 3, 1, 1), B(8), R(), C(8, 4, 1), G(1)]),
                      "a convolution bias in front of a BatchNorm2d is not covered"),
        "bn_behind_relu": (lambda: _Net([C(3, 8, 3, 1, 1, **nb), R(), B(8), C(8, 4, 1), G(1)]),
                           "a BatchNorm must directly follow a convolution"),
        "bn_behind_pool": (lambda: _Net([C(3, 8, 3, 1, 1, **nb), P(2, 2), B(8), C(8, 4, 1), G(1)]),
                           "a BatchNorm must directly follow a convolution"),
        "bn_first": (lambda: _Net([B(3), C(3, 8, 3, 1, 1), R(), C(8, 4, 1), G(1)]),
                     "a BatchNorm must directly follow a convolution"),
        "not_affine": (lambda: _Net([C(3, 8, 3, 1, 1, **nb), B(8, affine=False), R(), C(8, 4, 1), G(1)]),
                       "has no fused eval record"),
        "no_running_stats": (lambda: _Net([C(3, 8, 3, 1, 1, **nb), B(8, track_running_stats=False), R(), C(8, 4, 1), G(1)]),
                             "has no fused eval record"),
    }


@pytest.mark.parametrize("name", sorted(_declined_variants()))
def test_declined_variants_keep_the_autograd_path_and_say_why(name):
    build, reason = _declined_variants()[name]
    declined_net(lambda: tp.seed_batchnorm(build()), reason)
