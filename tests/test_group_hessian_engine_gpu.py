"""GPU: ``group_small`` as a Hessian engine and under the batched ``diag_ef`` against float64 (``stack_harness``)."""

import pytest
import torch

import stack_harness as sh
from pytorchhessianfree_amd import modelprep, testproblems
from pytorchhessianfree_amd.engine import PlainStackEngine
from tol import within

pytestmark = pytest.mark.gpu

BATCH, BIAS, BN = 3, testproblems.group_small, lambda **kw: testproblems.group_small(bn=True, **kw)
_freeze = lambda model: model.net[2].weight.requires_grad_(False)  # noqa: E731  (the first grouped unit: V = NULL)


@pytest.fixture(autouse=True)
def _opt_in(monkeypatch):
    monkeypatch.setenv("HF_GROUP_ENGINE", "1")
    monkeypatch.setenv("HF_GROUP_HESSIAN", "1")


@pytest.mark.parametrize("make, train, prep", [(BIAS, 0, None), (BN, 0, None), (BN, 1, None), (BIAS, 0, _freeze)],
                         ids=["bias", "bn-eval", "bn-train", "frozen-g-weight"])
def test_hessian_products_against_float64(make, train, prep, monkeypatch):
    op, model, (x, t), lossf, _ = sh.engine(make, BATCH, hessian=True, train=train, prep=prep)
    assert type(op) is PlainStackEngine and op.hessian, type(op)  # (without HF_GROUP_HESSIAN: the autograd operator)
    v = torch.randn(op.n, generator=torch.Generator().manual_seed(74)).to(sh.DEV)
    got = op(v).clone()
    assert torch.equal(op(v), got)
    p64, out64, loss64, _ = sh.float64_twin(make, BATCH, op, prep=prep, train=train)
    errs = sh.rel(got, sh.product64(p64, out64, loss64, v, hessian=True)), sh.rel(op.gradient(), sh.grad64(loss64, p64))
    print("group_small Hessian product, gradient: rel err %.3e, %.3e" % errs)
    within(max(errs), 2e-6)
    names = sh.record_launches(monkeypatch)
    op(v)  # one two-term launch per grouped unit with a trainable weight and a tangent-carrying input
    assert names.count("hf_gconv2d_nhwc_backward2_slabs") == sum(u.two_term for u in op.units) == (1 if prep else 2), names


@pytest.mark.parametrize("make", [BIAS, BN], ids=["bias", "bn-eval"])
def test_batched_diag_ef_against_float64(make, monkeypatch):
    monkeypatch.setenv("HF_DIAG_EF_BATCHED", "1")
    op, model, (x, t), lossf, _ = sh.engine(make, BATCH)
    assert type(op) is PlainStackEngine and op.diag_batched_declined is None
    p64, out64, loss64, t64 = sh.float64_twin(make, BATCH, op)
    names = sh.record_launches(monkeypatch)
    within(sh.rel(op.diag_ef("mean"), sh.diag64(lossf, p64, out64, t64, BATCH, op.n)), 2e-6)
    assert names.count("hf_gconv2d_nhwc_sqsum_slabs") == sum(u.grouped and u.pw is not None for u in op.units) == 2


def test_without_the_switch_hessian_products_are_declined(monkeypatch):
    monkeypatch.delenv("HF_GROUP_HESSIAN")
    model, (x, t), lossf = BIAS(batch_size=BATCH, device=sh.DEV)
    modelprep.prepare_model(model, channels_last=True)
    sh.declined(model, x, t, lossf, "conv 1: Hessian products through a grouped convolution are not covered (opt-in on top "
                "of HF_GROUP_ENGINE=1: HF_GROUP_HESSIAN=1)", hessian=True)
