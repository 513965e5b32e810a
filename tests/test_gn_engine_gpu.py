"""GPU: ``testproblems.gn_small`` on the plain-stack engine (GroupNorm units on hf_gn.hip) against float64 autograd of the
stock model on the engine's own decisions (``stack_harness``); and the declines, which name their unit."""

import pytest
import torch
from torch import nn

import pytorchhessianfree_amd as hf
import stack_harness as sh
from pytorchhessianfree_amd import modelprep, testproblems
from pytorchhessianfree_amd.engine import PlainStackEngine
from tol import within

pytestmark = pytest.mark.gpu

BATCH, MAKE = 3, testproblems.gn_small
_freeze = lambda model: model.net[4].weight.requires_grad_(False)  # noqa: E731  (the second unit's scale: v_gamma = NULL)


@pytest.fixture(autouse=True)
def _opt_in(monkeypatch):
    monkeypatch.setenv("HF_GN_ENGINE", "1")  # (GroupNorm units are opt-in)


@pytest.mark.parametrize("batched", ["0", "1"], ids=["per-sample", "batched"])
def test_eval_point_against_float64(batched, monkeypatch):
    monkeypatch.setenv("HF_DIAG_EF_BATCHED", batched)  # (diag_ef's two routes)
    op, model, (x, t), lossf, cpu_params = sh.engine(MAKE, BATCH)
    assert type(op) is PlainStackEngine, type(op)
    assert [u.gn is not None for u in op.units] == [True, True, True, False] and op.units[1].pcb is not None
    sh.check_point(op, MAKE, BATCH, x, lossf, cpu_params, None, "gn_small")
    names = sh.record_launches(monkeypatch)
    op(torch.ones(op.n, device=sh.DEV))
    # 4 launches per GroupNorm unit and product: tangent convolution, hf_gn_act_tangent, hf_gn_act_adjoint, D + W gradient
    assert names.count("hf_gn_act_tangent") == names.count("hf_gn_act_adjoint") == 3, names
    assert sum(x.startswith(("hf_chan", "hf_bn")) for x in names) == 2, names  # (the bias unit's own two)
    assert len(names) <= 4 * len(op.units) + 3, names  # (+ the scatter of v_W, the head, the gather)


def test_frozen_scale_against_float64():
    op, model, (x, t), lossf, _ = sh.engine(MAKE, BATCH, prep=_freeze)
    assert type(op) is PlainStackEngine and op.units[1].pg is None
    v = torch.randn(op.n, generator=torch.Generator().manual_seed(74)).to(sh.DEV)
    p64, out64, loss64, _ = sh.float64_twin(MAKE, BATCH, op, prep=_freeze)
    within(sh.rel(op(v), sh.product64(p64, out64, loss64, v)), 1e-6)
    within(sh.rel(op.gradient(), sh.grad64(loss64, p64)), 2e-6)


def test_step_takes_the_session():
    model, (x, t), lossf = MAKE(batch_size=BATCH, device=sh.DEV)
    modelprep.prepare_model(model, channels_last=True)
    opt = hf.HessianFree(model.parameters(), cg_max_iter=5, graph_matvec=True)
    opt.step(lambda: (lambda out: (lossf(out, t), out))(model(x)))
    assert opt.path_report()["step"]["path"] == "session", opt.path_report()


_net = lambda *gn, c=8: lambda: sh._Net([nn.Conv2d(3, c, 3, 1, 1), *gn, nn.Conv2d(c, 4, 1),  # noqa: E731
                                         nn.AdaptiveAvgPool2d(1)])


@pytest.mark.parametrize("build, reason, unset", [
    (_net(nn.GroupNorm(2, 8), nn.ReLU()), "conv0: GroupNorm(2, 8): GroupNorm units are opt-in (HF_GN_ENGINE=1)", True),
    (_net(nn.GroupNorm(2, 8, affine=False)), "conv0: GroupNorm(2, 8): affine=False is not covered", False),
    (_net(nn.GroupNorm(4, 8)), "conv0: GroupNorm(4, 8): 2 channels per group (the kernels take multiples of 4)", False),
    (_net(nn.GroupNorm(1, 260), c=260), "conv0: GroupNorm(1, 260): a block of h*w*span = 64 * 260 = 16640 floats (one "
     "workgroup's LDS holds 16384)", False),
    (_net(nn.GroupNorm(2, 8), nn.ReLU(), nn.MaxPool2d(2)), "MaxPool2d behind conv0: a pool behind a GroupNorm unit is not "
     "covered", False),
], ids=["switch-unset", "not-affine", "width-2", "lds-limit", "max-pool"])
def test_declined_stacks(build, reason, unset, monkeypatch):
    if unset:
        monkeypatch.delenv("HF_GN_ENGINE")
    sh.declined_net(build, reason)


def test_declined_hessian_and_process_group():
    model, (x, t), lossf = MAKE(batch_size=BATCH, device=sh.DEV)
    modelprep.prepare_model(model, channels_last=True)
    sh.declined(model, x, t, lossf, "conv0: GroupNorm(2, 8): Hessian products through a GroupNorm unit", hessian=True)
    params, out, why = list(model.parameters()), model(x), []
    assert PlainStackEngine.try_build(lossf(out, t), out, params, why=why, group=object()) is None
    assert any("conv0: GroupNorm(2, 8): data parallelism is not covered for a GroupNorm unit" in w for w in why), why
