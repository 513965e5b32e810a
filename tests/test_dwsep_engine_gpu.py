"""GPU: ``testproblems.dwsep_small`` on the plain-stack engine (depthwise units on hf_dwconv.hip) against float64 autograd
of the stock model on the engine's own decisions (``stack_harness``); and the declines, which name their unit."""

import functools

import pytest
import torch
from torch import nn

import pytorchhessianfree_amd as hf
import stack_harness as sh
from pytorchhessianfree_amd import modelprep, testproblems
from pytorchhessianfree_amd.engine import PlainStackEngine
from tol import within

pytestmark = pytest.mark.gpu

BATCH = 3
BIAS, BN = testproblems.dwsep_small, functools.partial(testproblems.dwsep_small, bn=True)
_freeze = lambda model: model.net[2].weight.requires_grad_(False)  # noqa: E731  (the first depthwise unit: V = NULL)


@pytest.fixture(autouse=True)
def _opt_in(monkeypatch):
    monkeypatch.setenv("HF_DW_ENGINE", "1")  # (depthwise units are opt-in until their speed is measured)


@pytest.mark.parametrize("make", [BIAS, BN], ids=["bias", "bn-eval"])
def test_eval_point_against_float64(make):
    op, model, (x, t), lossf, cpu_params = sh.engine(make, BATCH)
    assert type(op) is PlainStackEngine, type(op)
    assert [u.depthwise for u in op.units] == [False, True, False, True, False, False]
    sh.check_point(op, make, BATCH, x, lossf, cpu_params, None, "dwsep_small")


@pytest.mark.parametrize("make, train, prep", [(BN, True, None), (BIAS, False, _freeze)], ids=["bn-train", "frozen-dw-weight"])
def test_product_and_gradient_against_float64(make, train, prep):
    op, model, (x, t), lossf, _ = sh.engine(make, BATCH, train=train, prep=prep)
    assert type(op) is PlainStackEngine and op.train_bn == train and (op.units[1].pw is None) == (prep is not None)
    v = torch.randn(op.n, generator=torch.Generator().manual_seed(74)).to(sh.DEV)
    p64, out64, loss64, _ = sh.float64_twin(make, BATCH, op, prep=prep, train=train)
    within(sh.rel(op(v), sh.product64(p64, out64, loss64, v)), 1e-6)
    if op.loss_spec is not None:  # (a train-mode engine has a gradient where its own forward pass reproduces the model's)
        within(sh.rel(op.gradient(), sh.grad64(loss64, p64)), 2e-6)


def test_step_takes_the_session():
    model, (x, t), lossf = BIAS(batch_size=BATCH, device=sh.DEV)
    modelprep.prepare_model(model, channels_last=True)
    opt = hf.HessianFree(model.parameters(), cg_max_iter=5, graph_matvec=True)
    opt.step(lambda: (lambda out: (lossf(out, t), out))(model(x)))
    assert opt.path_report()["step"]["path"] == "session", opt.path_report()


_net = lambda dw, cin=8: lambda: sh._Net([nn.Conv2d(3, cin, 3, 1, 1), nn.ReLU(), dw,  # noqa: E731
                                          nn.Conv2d(dw.out_channels, 4, 1), nn.AdaptiveAvgPool2d(1)])


@pytest.mark.parametrize("build, reason", [
    (_net(nn.Conv2d(8, 16, 3, 1, 1, groups=8)), "no depth multiplier"),
    (_net(nn.Conv2d(8, 8, 3, 1, 1, groups=2)), "only depthwise"),
    (_net(nn.Conv2d(6, 6, 3, 1, 1, groups=6), cin=6), "depthwise over 6 channels"),
    (_net(nn.Conv2d(8, 8, (5, 10), 1, (2, 5), groups=8)), "depthwise with 50 taps"),
], ids=["depth-multiplier", "other-groups", "c%4", "50-taps"])
def test_declined_stacks(build, reason):
    sh.declined_net(build, reason)


def test_declined_first_layer_hessian_and_process_group():
    torch.manual_seed(0)  # a depthwise FIRST layer (4 input channels: a 3-channel one would be declined for c % 4)
    model = sh._Net([nn.Conv2d(4, 4, 3, 1, 1, groups=4), nn.ReLU(), nn.Conv2d(4, 4, 1), nn.AdaptiveAvgPool2d(1)]).eval()
    model, x, t = model.to(sh.DEV), torch.rand(2, 4, 8, 8).to(sh.DEV), torch.tensor([0, 3]).to(sh.DEV)
    modelprep.prepare_model(model, channels_last=True)
    sh.declined(model, x, t, nn.CrossEntropyLoss(), "depthwise first layer")
    model, (x, t), lossf = BIAS(batch_size=BATCH, device=sh.DEV)
    modelprep.prepare_model(model, channels_last=True)
    sh.declined(model, x, t, lossf, "Hessian products through a depthwise convolution", hessian=True)
    params, out, why = list(model.parameters()), model(x), []
    assert PlainStackEngine.try_build(lossf(out, t), out, params, why=why, group=object()) is None
    assert any("data parallelism is not covered for a depthwise convolution" in w for w in why), why
