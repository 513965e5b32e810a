"""GPU: the dense-stack engine on TALL batches (``HF_DENSE_ENGINE=1`` + ``HF_DENSE_TALL=1``, ``hf_dense_tall.hip``) at batch
300.  GGN / Hessian (``HF_DENSE_HESSIAN=1``) products and the gradient sit within ``3 x`` the distance fp32 autograd keeps from
float64 autograd of the STOCK model (the rule of ``test_dense_engine_gpu.py`` / ``test_dense_hess_engine_gpu.py``), ``diag_ef``
within ``3 x`` that of fp32 ``diag_EF_autograd`` ``+ 4 u`` (``test_dense_diag_engine_gpu.py``); graph capture; path report."""

import copy

import pytest
import torch
from tol import within

import pytorchhessianfree_amd as hf
from pytorchhessianfree_amd import curvature, modelprep, preconditioners
from pytorchhessianfree_amd import testproblems as tp
from pytorchhessianfree_amd.engine import FusedGGNEngine
from pytorchhessianfree_amd.engine.dense import DenseStackEngine

pytestmark = pytest.mark.gpu
DEV, ROWS, U32 = "cuda", 300, 2.0 ** -24


@pytest.fixture(autouse=True)
def _tall_on(monkeypatch):
    for name in ("HF_DENSE_ENGINE", "HF_DENSE_TALL", "HF_DENSE_HESSIAN"):
        monkeypatch.setenv(name, "1")


def _net(widths, acts, ce, seed):
    """``Linear [activation]`` per entry of ``acts``, data and targets at batch ROWS, all from one seed."""
    gen = torch.manual_seed(seed)
    layers = [m for i, a in enumerate(acts) for m in [torch.nn.Linear(widths[i], widths[i + 1])] + ([a()] if a else [])]
    x = torch.randn(ROWS, widths[0], generator=gen)
    t = torch.randint(0, widths[-1], (ROWS,), generator=gen) if ce else torch.randn(ROWS, widths[-1], generator=gen)
    return torch.nn.Sequential(*layers).to(DEV), (x.to(DEV), t.to(DEV)), torch.nn.CrossEntropyLoss() if ce else torch.nn.MSELoss()


PROBLEMS = {"mwe_mlp": lambda: tp.mwe_mlp(batch_size=ROWS, device=DEV),
            "tanh_ce": lambda: _net((130, 64, 48, 10), (torch.nn.Tanh, torch.nn.Tanh, None), True, 0),
            "mixed_mse": lambda: _net((37, 40, 33, 20, 6), (torch.nn.Tanh, torch.nn.ReLU, torch.nn.Tanh, None), False, 2)}


def trainable(model):
    return [p for p in model.parameters() if p.requires_grad]


def dist(a, b):
    b = b.double()
    return float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-300))


def references(model, x, t, lossf, v, dtype):
    """(GGN product, Hessian product, gradient) of the stock model by the autograd operators in ``dtype``."""
    m = copy.deepcopy(model).to(dtype)
    out = m(x.to(dtype))
    loss = lossf(out, t.to(dtype) if t.dtype.is_floating_point else t)
    ggn = curvature.GGNOperator(loss, out, trainable(m))(v.to(dtype)).clone()
    grad = torch.cat([g.reshape(-1) for g in torch.autograd.grad(loss, trainable(m), retain_graph=True)])
    return ggn, curvature.HessianOperator(loss, trainable(m))(v.to(dtype)).clone(), grad


def engine(model, x, t, lossf, hessian=False):
    out, why = model(x), []
    eng = FusedGGNEngine.try_build(lossf(out, t), out, trainable(model), hessian=hessian, why=why)
    assert isinstance(eng, DenseStackEngine) and eng.chain.tall and eng.rows == ROWS, why
    return eng


def _vector(model, seed=5):
    n = sum(p.numel() for p in trainable(model))
    return torch.randn(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def _check(model, x, t, lossf, note):
    v = _vector(model)
    r32, r64 = references(model, x, t, lossf, v, torch.float32), references(model, x, t, lossf, v, torch.float64)
    modelprep.prepare_model(model)
    ggn, hes = engine(model, x, t, lossf)(v).clone(), engine(model, x, t, lossf, hessian=True)
    got = (ggn, hes(v).clone(), hes.gradient(torch.empty_like(v)))
    for name, g, a, b in zip(("ggn", "hessian", "gradient"), got, r32, r64):
        print(f"{note} {name}: engine {dist(g, b):.3e}  autograd {dist(a, b):.3e}")
        within(dist(g, b), 3.0 * dist(a, b), note=(note, name))
    return hes, v, got[1]


@pytest.mark.parametrize("frozen", (0, 1))  # 1: the first layer frozen, a dead prefix
@pytest.mark.parametrize("problem", sorted(PROBLEMS))
def test_products_gradient_and_diag_ef_against_float64(problem, frozen):
    model, (x, t), lossf = PROBLEMS[problem]()
    for p in list(model[0].parameters())[:2 * frozen]:
        p.requires_grad = False
    t64 = t.double() if t.dtype.is_floating_point else t
    d64 = preconditioners.diag_EF_autograd(copy.deepcopy(model).double(), lossf, x.double(), t64, "mean")
    d32 = preconditioners.diag_EF_autograd(copy.deepcopy(model), lossf, x, t, "mean")
    hes, v, got = _check(model, x, t, lossf, (problem, frozen))
    diag = hes.diag_ef("mean")  # against diag_EF_autograd in float64, fp32 diag_EF_autograd as the yardstick
    print(f"{problem} {frozen} diag_ef: engine {dist(diag, d64):.3e}  diag_EF_autograd {dist(d32, d64):.3e}")
    within(dist(diag, d64), 3.0 * dist(d32, d64) + 4.0 * U32, note=(problem, frozen))
    assert hes.dead_layers == frozen and hes.layers[frozen].first_live and hes.layers[frozen].dslabs is None
    assert torch.equal(hes(v).view(torch.int32), got.view(torch.int32)), "two products of one vector differ"


def test_captured_product_replays_to_the_eager_bits():
    model, (x, t), lossf = PROBLEMS["tanh_ce"]()
    eng, v = engine(modelprep.prepare_model(model), x, t, lossf, hessian=True), _vector(model, 9)
    eager, out = eng.local(v).clone(), torch.empty_like(v)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.local(v, out=out)
    for seed in (9, 10, 11):  # (several replays, on new vectors too)
        v.copy_(_vector(model, seed))
        want = eng.local(v).clone() if seed != 9 else eager
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)), seed


def _step_report(monkeypatch, **env):
    for k, val in env.items():
        monkeypatch.setenv(k, val) if val is not None else monkeypatch.delenv(k)
    model, (x, t), lossf = tp.mwe_mlp(batch_size=ROWS, device=DEV)
    modelprep.prepare_model(model)
    opt = hf.HessianFree(model.parameters(), graph_matvec=True, cg_max_iter=2)
    opt.step(lambda: (lambda o: (lossf(o, t), o))(model(x)))  # forward(): (loss, outputs)
    return opt.path_report()["step"]


@pytest.mark.filterwarnings("ignore:HessianFree")  # (the slower-path warning is what the reports below are about)
def test_step_reports_the_engine_the_switch_and_the_session_limit(monkeypatch):
    rep = _step_report(monkeypatch)
    assert rep["path"] == "engine-graphed" and "no session yet" in rep["declined"], rep
    rep = _step_report(monkeypatch, HF_DENSE_SESSION="1")  # the session stays at 256 rows; products still on the engine
    assert rep["path"] == "engine-graphed" and "DenseStackEngine" in rep["declined"], rep
    assert "up to 256 rows" in rep["declined"] and "batch 300" in rep["declined"], rep
    rep = _step_report(monkeypatch, HF_DENSE_SESSION="0", HF_DENSE_TALL=None)
    assert rep["path"] == "autograd-graphed", rep
    assert "batch 300 > 256 rows" in rep["declined"] and "HF_DENSE_TALL" in rep["declined"], rep
