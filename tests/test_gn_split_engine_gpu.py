"""GPU: plain stacks whose GroupNorm blocks exceed one workgroup's LDS on the plain-stack engine (the split kernels of
hf_gn.hip, ``HF_GN_SPLIT=1`` on top of ``HF_GN_ENGINE=1``) against float64 autograd of the stock model on the engine's own
decisions (``stack_harness``); and the declines, which name their unit."""

import pytest
import torch
from torch import nn

import pytorchhessianfree_amd as hf
import stack_harness as sh
from pytorchhessianfree_amd import modelprep
from pytorchhessianfree_amd.engine import PlainStackEngine
from tol import within

pytestmark = pytest.mark.gpu

# (a) GroupNorm(1, 260) on 8x8: 16 640 floats, ReLU.  (b) 48x48: GroupNorm(1, 8) = 18 432 floats -- split, no ReLU, behind
# a biased convolution -- and GroupNorm(2, 8) = 9 216 floats, which stays on the one-launch kernels in the same engine
LAYERS = {"a": (lambda: [nn.Conv2d(3, 260, 3, 1, 1), nn.GroupNorm(1, 260), nn.ReLU(), nn.Conv2d(260, 4, 1),
                         nn.AdaptiveAvgPool2d(1)], 8, 3, [True]),
          "b": (lambda: [nn.Conv2d(3, 8, 3, 1, 1), nn.GroupNorm(1, 8), nn.Conv2d(8, 8, 3, 1, 1), nn.GroupNorm(2, 8), nn.ReLU(),
                         nn.Conv2d(8, 4, 1), nn.AdaptiveAvgPool2d(1)], 48, 2, [True, False])}
SPLIT_NAMES = ("hf_gn_split_tangent_sums", "hf_gn_split_act_tangent", "hf_gn_split_adjoint_sums", "hf_gn_split_act_adjoint")


def _make(net):
    layers, size, _, _ = LAYERS[net]

    def make(batch_size, device="cpu", data_seed=None):
        torch.manual_seed(0)
        model = sh._Net(layers()).eval()
        gen = torch.Generator().manual_seed(1000)
        with torch.no_grad():
            for m in model.modules():
                if isinstance(m, nn.GroupNorm):
                    m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=gen))
                    m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=gen))
        gen = torch.Generator().manual_seed(1 if data_seed is None else data_seed)
        x, t = torch.rand(batch_size, 3, size, size, generator=gen), torch.randint(0, 4, (batch_size,), generator=gen)
        return model.to(device), (x.to(device), t.to(device)), nn.CrossEntropyLoss()
    return make


@pytest.fixture(autouse=True)
def _opt_in(monkeypatch):
    monkeypatch.setenv("HF_GN_ENGINE", "1")
    monkeypatch.setenv("HF_GN_SPLIT", "1")


@pytest.mark.parametrize("batched", ["0", "1"], ids=["per-sample", "batched"])
@pytest.mark.parametrize("net", ["a", "b"])
def test_eval_point_against_float64(net, batched, monkeypatch):
    monkeypatch.setenv("HF_DIAG_EF_BATCHED", batched)  # (diag_ef's two routes)
    make, batch, split = _make(net), LAYERS[net][2], LAYERS[net][3]
    op, model, (x, t), lossf, cpu_params = sh.engine(make, batch)
    assert type(op) is PlainStackEngine, type(op)
    assert [u.gn_parts >= 2 for u in op.units if u.gn is not None] == split and op.units[0].pcb is not None
    sh.check_point(op, make, batch, x, lossf, cpu_params, None, f"gn_split_{net}")
    names = sh.record_launches(monkeypatch)
    op(torch.ones(op.n, device=sh.DEV))
    # a split unit: tangent convolution, 2, 2, D + W gradient; the one-launch unit of (b) keeps its own two
    assert [names.count(x) for x in SPLIT_NAMES] == [sum(split)] * 4, names
    assert names.count("hf_gn_act_tangent") == names.count("hf_gn_act_adjoint") == len(split) - sum(split), names
    assert len(names) <= 4 * len(op.units) + 2 * sum(split) + 3, names  # (+ the scatter of v_W, the head, the gather)


def test_frozen_scale_against_float64():
    make = _make("b")
    freeze = lambda model: model.net[1].weight.requires_grad_(False)  # noqa: E731  (the split unit's scale: v_gamma = NULL)
    op, model, (x, t), lossf, _ = sh.engine(make, 2, prep=freeze)
    assert type(op) is PlainStackEngine and op.units[0].pg is None and op.units[0].gn_parts >= 2
    v = torch.randn(op.n, generator=torch.Generator().manual_seed(74)).to(sh.DEV)
    p64, out64, loss64, _ = sh.float64_twin(make, 2, op, prep=freeze)
    within(sh.rel(op(v), sh.product64(p64, out64, loss64, v)), 1e-6)
    within(sh.rel(op.gradient(), sh.grad64(loss64, p64)), 2e-6)


def test_step_takes_the_session():
    model, (x, t), lossf = _make("a")(batch_size=3, device=sh.DEV)
    modelprep.prepare_model(model, channels_last=True)
    opt = hf.HessianFree(model.parameters(), cg_max_iter=5, graph_matvec=True)
    opt.step(lambda: (lambda out: (lossf(out, t), out))(model(x)))
    assert opt.path_report()["step"]["path"] == "session", opt.path_report()


@pytest.mark.parametrize("reason, unset, hessian", [
    ("conv0: GroupNorm(1, 260): a block of h*w*span = 64 * 260 = 16640 floats (one workgroup's LDS holds 16384)", True, False),
    ("conv0: GroupNorm(1, 260): Hessian products through a split GroupNorm unit are not covered", False, True),
], ids=["switch-unset", "hessian"])
def test_declined(reason, unset, hessian, monkeypatch):
    if unset:
        monkeypatch.delenv("HF_GN_SPLIT")
    model, (x, t), lossf = _make("a")(batch_size=3, device=sh.DEV)
    modelprep.prepare_model(model, channels_last=True)
    sh.declined(model, x, t, lossf, reason, hessian=hessian)
