"""GPU: ``testproblems.group_small`` on the plain-stack engine (grouped units on hf_gconv.hip) against float64 autograd of
the stock model on the engine's own decisions (``stack_harness``); and the declines, which name their unit."""

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
BIAS, BN = testproblems.group_small, functools.partial(testproblems.group_small, bn=True)
_freeze = lambda model: model.net[2].weight.requires_grad_(False)  # noqa: E731  (the first grouped unit: V = NULL)


@pytest.fixture(autouse=True)
def _opt_in(monkeypatch):
    monkeypatch.setenv("HF_GROUP_ENGINE", "1")  # (grouped units are opt-in: their speed is not measured)


@pytest.mark.parametrize("make", [BIAS, BN], ids=["bias", "bn-eval"])
def test_eval_point_against_float64(make):
    op, model, (x, t), lossf, cpu_params = sh.engine(make, BATCH)
    assert type(op) is PlainStackEngine, type(op)
    assert [u.grouped for u in op.units] == [False, True, False, True, False]
    sh.check_point(op, make, BATCH, x, lossf, cpu_params, None, "group_small")


@pytest.mark.parametrize("make, train, prep", [(BN, True, None), (BIAS, False, _freeze)], ids=["bn-train", "frozen-g-weight"])
def test_product_and_gradient_against_float64(make, train, prep):
    op, model, (x, t), lossf, _ = sh.engine(make, BATCH, train=train, prep=prep)
    assert type(op) is PlainStackEngine and op.train_bn == train and (op.units[1].pw is None) == (prep is not None)
    v = torch.randn(op.n, generator=torch.Generator().manual_seed(74)).to(sh.DEV)
    p64, out64, loss64, _ = sh.float64_twin(make, BATCH, op, prep=prep, train=train)
    e_prod = sh.rel(op(v), sh.product64(p64, out64, loss64, v))
    print(f"group_small product: rel err {e_prod:.3e}")
    within(e_prod, 1e-6)
    if op.loss_spec is not None:  # (a train-mode engine has a gradient where its own forward pass reproduces the model's)
        e_grad = sh.rel(op.gradient(), sh.grad64(loss64, p64))
        print(f"group_small gradient: rel err {e_grad:.3e}")
        within(e_grad, 2e-6)


def test_step_takes_the_session():
    model, (x, t), lossf = BIAS(batch_size=BATCH, device=sh.DEV)
    modelprep.prepare_model(model, channels_last=True)
    opt = hf.HessianFree(model.parameters(), cg_max_iter=5, graph_matvec=True)
    opt.step(lambda: (lambda out: (lossf(out, t), out))(model(x)))
    assert opt.path_report()["step"]["path"] == "session", opt.path_report()


_net = lambda g, cin=8: lambda: sh._Net([nn.Conv2d(3, cin, 3, 1, 1), nn.ReLU(), g,  # noqa: E731
                                         nn.Conv2d(g.out_channels, 4, 1), nn.AdaptiveAvgPool2d(1)])


@pytest.mark.parametrize("build, reason, unset", [
    (_net(nn.Conv2d(8, 8, 3, 1, 1, groups=2)), "conv 1: groups = 2 with 8 -> 8 channels: only depthwise convolutions (groups = "
     "in_channels = out_channels) are covered, no depth multiplier; other grouped layers are opt-in (HF_GROUP_ENGINE=1)", True),
    (_net(nn.Conv2d(12, 8, 3, 1, 1, groups=2), cin=12), "conv 1: groups = 2 with 12 -> 8 channels: 6 -> 4 channels per group",
     False),
    (_net(nn.Conv2d(8, 16, 3, 1, 1, groups=8)), "conv 1: groups = 8 with 8 -> 16 channels: only depthwise", False),
], ids=["switch-unset", "width-6", "depth-multiplier"])
def test_declined_stacks(build, reason, unset, monkeypatch):
    if unset:
        monkeypatch.delenv("HF_GROUP_ENGINE")
    sh.declined_net(build, reason)


def test_declined_first_layer_hessian_and_process_group():
    torch.manual_seed(0)  # a grouped FIRST layer (8 input channels in 2 groups)
    model = sh._Net([nn.Conv2d(8, 8, 3, 1, 1, groups=2), nn.ReLU(), nn.Conv2d(8, 4, 1), nn.AdaptiveAvgPool2d(1)]).eval()
    model, x, t = model.to(sh.DEV), torch.rand(2, 8, 8, 8).to(sh.DEV), torch.tensor([0, 3]).to(sh.DEV)
    modelprep.prepare_model(model, channels_last=True)
    sh.declined(model, x, t, nn.CrossEntropyLoss(), "conv 0: a grouped first layer")
    model, (x, t), lossf = BIAS(batch_size=BATCH, device=sh.DEV)
    modelprep.prepare_model(model, channels_last=True)
    sh.declined(model, x, t, lossf, "conv 1: Hessian products through a grouped convolution", hessian=True)
    params, out, why = list(model.parameters()), model(x), []
    assert PlainStackEngine.try_build(lossf(out, t), out, params, why=why, group=object()) is None
    assert any("conv 1: data parallelism is not covered for a grouped convolution" in w for w in why), why
