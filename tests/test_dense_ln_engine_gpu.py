"""GPU: LayerNorm layers on the dense-stack engine (``HF_DENSE_ENGINE=1 HF_DENSE_LN=1``; the kernels of ``hf_ln.hip``) -- GGN
products, ``gradient()`` and ``diag_ef`` of prepared MLPs against float64 evaluations of the STOCK model, each at ``3 x`` the
distance the stock fp32 evaluation of the same quantity (``curvature.GGNOperator``, autograd's gradient,
``diag_EF_autograd``) keeps from float64, measured in the test; ``step()`` on the engine; what it declines."""

import copy
import warnings

import pytest
import torch
from tol import within
from torch import nn

import pytorchhessianfree_amd as hf
from pytorchhessianfree_amd import curvature, modelprep, preconditioners
from pytorchhessianfree_amd.engine import FusedGGNEngine
from pytorchhessianfree_amd.engine.dense import DenseStackEngine

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _switches_on(monkeypatch):
    monkeypatch.setenv("HF_DENSE_ENGINE", "1")
    monkeypatch.setenv("HF_DENSE_LN", "1")


trainable = lambda model: [p for p in model.parameters() if p.requires_grad]  # noqa: E731
flat = lambda ts: torch.cat([t.reshape(-1) for t in ts])  # noqa: E731
# max-norm distance relative to max |b| (b: the float64 result)
dist = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))  # noqa: E731


def net(kind, affine=True):
    """(model, x, t, loss function): ``small`` -- ReLU and Tanh, cross-entropy, batch 9; ``wide`` -- a 1030-feature row (the
    workgroup form), MSE, batch 3; ``frozen`` -- ``small`` with a dead first layer and the second LayerNorm's scale frozen."""
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(1)
    if kind == "wide":
        model = nn.Sequential(nn.Linear(16, 1030), nn.LayerNorm(1030), nn.Tanh(), nn.Linear(1030, 4))
        x, t, lossf = torch.rand(3, 16, generator=gen), torch.rand(3, 4, generator=gen), nn.MSELoss()
    else:
        model = nn.Sequential(nn.Linear(20, 12), nn.LayerNorm(12, elementwise_affine=affine), nn.ReLU(), nn.Linear(12, 6),
                              nn.LayerNorm(6), nn.Tanh(), nn.Linear(6, 5))
        x, t, lossf = torch.rand(9, 20, generator=gen), torch.randint(0, 5, (9,), generator=gen), nn.CrossEntropyLoss()
    with torch.no_grad():  # (scales and shifts away from their initial 1 and 0)
        for m in model.modules():
            if isinstance(m, nn.LayerNorm) and m.elementwise_affine:
                m.weight.add_(0.3 * torch.randn(m.weight.shape, generator=gen))
                m.bias.add_(0.3 * torch.randn(m.bias.shape, generator=gen))
    if kind == "frozen":
        for p in (*model[0].parameters(), *model[1].parameters(), model[4].weight):
            p.requires_grad = False
    return model.to(DEV), x.to(DEV), t.to(DEV), lossf


def build(model, x, t, lossf, why=None, **kw):
    out = model(x)
    return FusedGGNEngine.try_build(lossf(out, t), out, trainable(model), why=why, **kw)


@pytest.mark.parametrize("kind", ["small", "wide", "frozen"])
def test_products_gradient_and_diag_ef_against_float64(kind):
    """``HF_DENSE_LN=1`` (set for every test of this file): the model is taken, and every served quantity is right."""
    model, x, t, lossf = net(kind)
    v = torch.randn(sum(p.numel() for p in trainable(model)), device=DEV,
                    generator=torch.Generator(device=DEV).manual_seed(5))
    m64 = copy.deepcopy(model).double()
    x64, t64 = x.double(), (t.double() if t.dtype.is_floating_point else t)
    o64, stock = m64(x64), copy.deepcopy(model)
    o32 = stock(x)
    want = {"product": curvature.GGNOperator(lossf(o64, t64), o64, trainable(m64))(v.double()).clone(),
            "gradient": flat(torch.autograd.grad(lossf(o64, t64), trainable(m64))),
            "diag_ef": preconditioners.diag_EF_autograd(m64, lossf, x64, t64, "mean")}
    fp32 = {"product": curvature.GGNOperator(lossf(o32, t), o32, trainable(stock))(v).clone(),
            "gradient": flat(torch.autograd.grad(lossf(o32, t), trainable(stock))),
            "diag_ef": preconditioners.diag_EF_autograd(stock, lossf, x, t, "mean")}
    modelprep.prepare_model(model)
    why = []
    eng = build(model, x, t, lossf, why)
    assert isinstance(eng, DenseStackEngine) and eng.has_ln, why
    assert eng.dead_layers == (1 if kind == "frozen" else 0)
    got = {"product": eng(v).clone(), "gradient": eng.gradient(torch.empty_like(v)), "diag_ef": eng.diag_ef("mean")}
    for name in got:
        d_eng, d_own = dist(got[name], want[name]), dist(fp32[name], want[name])
        print(f"{kind} {name}: engine {d_eng:.3e}  stock fp32 {d_own:.3e}")
        within(d_eng, 3.0 * d_own, note=(kind, name))
    assert torch.equal(got["product"].view(torch.int32), eng(v).view(torch.int32))  # two products: the same bits


def test_step_runs_on_the_dense_stack_engine():
    model, x, t, lossf = net("small")
    modelprep.prepare_model(model)
    opt = hf.HessianFree(model.parameters(), graph_matvec=True, cg_max_iter=5)

    def forward():
        o = model(x)
        return lossf(o, t), o

    before = float(forward()[0].detach())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        after = float(opt.step(forward))
    rep = opt.path_report()["step"]
    assert rep["path"] == "engine-graphed" and "dense-stack engine has no session yet" in rep["declined"], rep
    assert after < before


def test_declines_name_their_reason(monkeypatch):
    def reason(model, x, t, lossf, **kw):
        modelprep.prepare_model(model, channels_last=any(isinstance(m, nn.Conv2d) for m in model.modules()))
        why = []
        assert build(model, x, t, lossf, why, **kw) is None
        return " | ".join(why)

    monkeypatch.setenv("HF_DENSE_HESSIAN", "1")
    assert "Hessian products through a LayerNorm layer are not covered" in reason(*net("small"), hessian=True)
    assert "without elementwise_affine" in reason(*net("small", affine=False))
    monkeypatch.setenv("HF_DENSE_TALL", "1")
    model, _, _, lossf = net("small")
    gen = torch.Generator().manual_seed(2)
    xb, tb = torch.rand(300, 20, generator=gen).to(DEV), torch.randint(0, 5, (300,), generator=gen).to(DEV)
    assert "LayerNorm layers are not covered on the tall chain" in reason(model, xb, tb, lossf)
    torch.manual_seed(0)
    conv = nn.Sequential(nn.Conv2d(3, 4, 3), nn.ReLU(), nn.Flatten(), nn.Linear(64, 8), nn.LayerNorm(8), nn.ReLU(),
                         nn.Linear(8, 5)).to(DEV)
    xc, tc = torch.rand(2, 3, 6, 6, generator=gen).to(DEV), torch.randint(0, 5, (2,), generator=gen).to(DEV)
    assert "unsupported layer LayerNorm in the classifier tail" in reason(conv, xc, tc, lossf)
    monkeypatch.delenv("HF_DENSE_LN")
    why = reason(*net("small"))
    assert "LayerNorm layers are opt-in: HF_DENSE_LN=1" in why, why
