"""GPU: plain stacks with split GroupNorm units as Hessian engines (``HF_GN_ENGINE=1 HF_GN_SPLIT=1 HF_GN_HESSIAN=1``: a split
unit's second-order half is ``hf_gn_split_adjoint2_sums`` + ``hf_gn_split_act_adjoint2``) against float64 autograd of the stock
model on the engine's own decisions (``stack_harness``), within the one-launch units' 2e-6 (``test_gn_hessian_engine_gpu.py``)."""

import pytest
import torch
from torch import nn

import pytorchhessianfree_amd as hf
import stack_harness as sh
from pytorchhessianfree_amd import modelprep
from pytorchhessianfree_amd.engine import PlainStackEngine
from tol import within

pytestmark = pytest.mark.gpu

# test_gn_split_engine_gpu.py's nets, restated: (layers, input size, batch, which GroupNorm units are split).  (a) 16 640 floats,
# ReLU.  (b) GroupNorm(1, 8) at 48x48 = 18 432 floats: split; GroupNorm(2, 8) = 9 216: hf_gn_act_adjoint2 in the same engine
LAYERS = {"a": (lambda: [nn.Conv2d(3, 260, 3, 1, 1), nn.GroupNorm(1, 260), nn.ReLU(), nn.Conv2d(260, 4, 1),
                         nn.AdaptiveAvgPool2d(1)], 8, 3, [True]),
          "b": (lambda: [nn.Conv2d(3, 8, 3, 1, 1), nn.GroupNorm(1, 8), nn.Conv2d(8, 8, 3, 1, 1), nn.GroupNorm(2, 8), nn.ReLU(),
                         nn.Conv2d(8, 4, 1), nn.AdaptiveAvgPool2d(1)], 48, 2, [True, False])}
_freeze = lambda model: model.net[1].weight.requires_grad_(False)  # noqa: E731  (the split unit's scale: v_gamma = NULL)


def _make(net):
    def make(batch_size, device="cpu", data_seed=None):
        torch.manual_seed(0)
        model = sh._Net(LAYERS[net][0]()).eval()
        gen = torch.Generator().manual_seed(1000)
        with torch.no_grad():
            for m in (m for m in model.modules() if isinstance(m, nn.GroupNorm)):
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=gen))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=gen))
        gen, size = torch.Generator().manual_seed(1 if data_seed is None else data_seed), LAYERS[net][1]
        x, t = torch.rand(batch_size, 3, size, size, generator=gen), torch.randint(0, 4, (batch_size,), generator=gen)
        return model.to(device), (x.to(device), t.to(device)), nn.CrossEntropyLoss()
    return make


@pytest.fixture(autouse=True)
def _opt_in(monkeypatch):
    for name in ("HF_GN_ENGINE", "HF_GN_SPLIT", "HF_GN_HESSIAN"):
        monkeypatch.setenv(name, "1")


@pytest.mark.parametrize("net, prep", [("a", None), ("b", None), ("b", _freeze)], ids=["a", "b", "b-frozen-scale"])
def test_hessian_products_against_float64(net, prep, monkeypatch):
    make, batch, split = _make(net), LAYERS[net][2], LAYERS[net][3]
    op, model, (x, t), lossf, _ = sh.engine(make, batch, hessian=True, prep=prep)
    assert type(op) is PlainStackEngine and op.hessian and (op.units[0].pg is None) == (prep is not None), type(op)
    assert [u.gn_parts >= 2 for u in op.units if u.gn is not None] == split
    v = torch.randn(op.n, generator=torch.Generator().manual_seed(74)).to(sh.DEV)
    got = op(v).clone()
    p64, out64, loss64, _ = sh.float64_twin(make, batch, op, prep=prep)
    within(sh.rel(got, sh.product64(p64, out64, loss64, v, hessian=True)), 2e-6)
    within(sh.rel(op.gradient(), sh.grad64(loss64, p64)), 2e-6)
    names = sh.record_launches(monkeypatch)
    assert torch.equal(op(v), got)  # (repeatable, and untouched by the gradient sweep)
    # a reduce and an apply launch per split unit, ONE launch per unit within the limit, no first-order adjoint
    assert [names.count(f"hf_gn_{x}") for x in ("split_adjoint2_sums", "split_act_adjoint2", "act_adjoint2", "split_adjoint_sums",
                                                "act_adjoint")] == [sum(split)] * 2 + [len(split) - sum(split), 0, 0], names


def test_hessian_step_takes_the_session():
    model, (x, t), lossf = _make("a")(batch_size=3, device=sh.DEV)
    modelprep.prepare_model(model, channels_last=True)
    opt = hf.HessianFree(model.parameters(), cg_max_iter=5, curvature_opt="hessian", graph_matvec=True)
    opt.step(lambda: (lambda out: (lossf(out, t), out))(model(x)))
    assert opt.path_report()["step"]["path"] == "session" and opt._session.engine.hessian, opt.path_report()
