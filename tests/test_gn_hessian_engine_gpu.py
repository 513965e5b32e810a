"""GPU: GroupNorm stacks as Hessian engines (``HF_GN_ENGINE=1 HF_GN_HESSIAN=1``; the second-order half of a GroupNorm unit is
``hf_gn_act_adjoint2``) against float64 autograd of the stock model on the engine's own decisions (``stack_harness``)."""

import pytest
import torch
from torch import nn

import stack_harness as sh
from pytorchhessianfree_amd import modelprep, testproblems
from pytorchhessianfree_amd.engine import PlainStackEngine
from tol import within

pytestmark = pytest.mark.gpu

BATCH, MAKE = 3, testproblems.gn_small
_freeze = lambda model: model.net[4].weight.requires_grad_(False)  # noqa: E731  (the second unit's scale: v_gamma = NULL)


def _dw_gn(batch_size, device, **kw):
    """A GroupNorm behind a depthwise convolution (with a bias): the one-launch two-term backward reads ``u.gah``."""
    torch.manual_seed(0)
    model = sh._Net([nn.Conv2d(3, 8, 3, 1, 1), nn.ReLU(), nn.Conv2d(8, 8, 3, 1, 1, groups=8), nn.GroupNorm(2, 8), nn.ReLU(),
                     nn.Conv2d(8, 4, 1), nn.AdaptiveAvgPool2d(1)]).eval()
    gen = torch.Generator().manual_seed(1)
    x, t = torch.rand(batch_size, 3, 8, 8, generator=gen), torch.randint(0, 4, (batch_size,), generator=gen)
    return model.to(device), (x.to(device), t.to(device)), nn.CrossEntropyLoss()


@pytest.fixture(autouse=True)
def _opt_in(monkeypatch):
    for name in ("HF_GN_ENGINE", "HF_GN_HESSIAN", "HF_DW_ENGINE", "HF_DW_HESSIAN"):
        monkeypatch.setenv(name, "1")


@pytest.mark.parametrize("make, prep, gn_units", [(MAKE, None, 3), (MAKE, _freeze, 3), (_dw_gn, None, 1)],
                         ids=["gn_small", "frozen-scale", "depthwise"])
def test_hessian_products_against_float64(make, prep, gn_units, monkeypatch):
    op, model, (x, t), lossf, _ = sh.engine(make, BATCH, hessian=True, prep=prep)
    assert type(op) is PlainStackEngine and op.hessian, type(op)  # (without HF_GN_HESSIAN: the autograd operator)
    assert sum(u.gn is not None for u in op.units) == gn_units and any(u.in_place for u in op.units) == (make is _dw_gn)
    v = torch.randn(op.n, generator=torch.Generator().manual_seed(74)).to(sh.DEV)
    got = op(v).clone()
    assert torch.equal(op(v), got)
    p64, out64, loss64, _ = sh.float64_twin(make, BATCH, op, prep=prep)
    errs = sh.rel(got, sh.product64(p64, out64, loss64, v, hessian=True)), sh.rel(op.gradient(), sh.grad64(loss64, p64))
    print("GroupNorm Hessian product, gradient: rel err %.3e, %.3e" % errs)
    within(max(errs), 2e-6)
    assert torch.equal(op(v), got)  # (untouched by the gradient sweep)
    names = sh.record_launches(monkeypatch)
    op(v)  # ONE second-order launch per GroupNorm unit, the first-order adjoint's not at all
    assert names.count("hf_gn_act_adjoint2") == gn_units and names.count("hf_gn_act_adjoint") == 0, names


def test_without_the_switch_hessian_products_are_declined(monkeypatch):
    monkeypatch.delenv("HF_GN_HESSIAN")
    model, (x, t), lossf = MAKE(batch_size=BATCH, device=sh.DEV)
    modelprep.prepare_model(model, channels_last=True)
    sh.declined(model, x, t, lossf, "conv0: GroupNorm(2, 8): Hessian products through a GroupNorm unit are not covered "
                "(opt-in on top of HF_GN_ENGINE=1: HF_GN_HESSIAN=1)", hessian=True)
