"""GPU: the diagonal empirical-Fisher preconditioner on the dense-stack engine (``DenseStackEngine.diag_ef``,
``engine.dense.diag_ef_of``, ``preconditioners.diag_EF_backpack``) against a per-sample float64 loop on the STOCK model,
the reference's stored vectors and ``diag_EF_autograd``; frozen patterns; repeatability and graph capture; the public
route; what falls through to the ``vmap`` code and why.

Distances are max-norm relative to the largest float64 entry (``dist`` of ``test_dense_engine_gpu.py``).  Bound of the
engine's distance to float64: ``3 x max(distance of diag_EF_autograd in fp32 on the stock model, distance of the
reference's stored vector where there is one) + 4 u`` -- the factor 3 over the other fp32 evaluations is the project's
rule for dense products; ``4 u`` (``u = 2**-24``) covers the four final roundings ANY fp32 evaluation has (two squares,
their product, the 1/N): on 48-entry vectors the alternatives can land within one ulp by luck.  Both distances are
measured here; nothing is taken from the engine.  Every comparison prints its triple as one JSON line.

The engine is opt-in (``HF_DENSE_ENGINE=1``): every test sets the switch."""

import copy
import json
import warnings

import pytest
import torch
from helpers import T, small_nn
from tol import within

import pytorchhessianfree_amd as hf
from pytorchhessianfree_amd import modelprep, preconditioners
from pytorchhessianfree_amd import testproblems as tp
from pytorchhessianfree_amd.engine.dense import DenseStackEngine, diag_ef_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
U32 = 2.0 ** -24
KEYS = ["smallnn_s0_mean", "smallnn_s0_sum", "smallnn_s1_mean", "smallnn_s1_sum", "smallnn_s42_mean", "smallnn_s42_sum"]


@pytest.fixture(autouse=True)
def _dense_engine_on(monkeypatch):
    monkeypatch.setenv("HF_DENSE_ENGINE", "1")


def trainable(model):
    return [p for p in model.parameters() if p.requires_grad]


def dist(a, b):
    """max-norm distance relative to max |b| (b: the float64 diagonal)."""
    b = b.double()
    return float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-300))


def loop64(model, lossf, x, t, reduction):
    """The per-sample loop on a ``.double()`` copy of the stock model: the float64 truth."""
    m64 = copy.deepcopy(model).double()
    params = trainable(m64)
    x64 = x.double()
    t64 = t.double() if t.dtype.is_floating_point else t
    diag = torch.zeros(sum(p.numel() for p in params), dtype=torch.float64, device=x.device)
    for i in range(x.shape[0]):
        g = torch.autograd.grad(lossf(m64(x64[i]), t64[i]), params)
        diag += torch.cat([q.reshape(-1) for q in g]) ** 2
    return diag / x.shape[0] if reduction == "mean" else diag


def engine_for(model, lossf, x, t):
    out = model(x)
    why = []
    eng = DenseStackEngine.try_build(lossf(out, t), out, trainable(model), why=why)
    assert isinstance(eng, DenseStackEngine), why
    return eng


def diagonals(model, lossf, x, t, reduction):
    """(engine diagonal, engine, diag_EF_autograd of the stock fp32 model, float64 loop of the stock model).  ``model`` is
    prepared here, after the stock evaluations."""
    d64 = loop64(model, lossf, x, t, reduction)
    d32 = preconditioners.diag_EF_autograd(copy.deepcopy(model), lossf, x, t, reduction).clone()
    modelprep.prepare_model(model)
    eng = engine_for(model, lossf, x, t)
    return eng.diag_ef(reduction).clone(), eng, d32, d64


def check(case, got, d32, d64, ref=None):
    d_eng, d_own = dist(got, d64), dist(d32, d64)
    d_ref = None if ref is None else dist(ref, d64)
    bound = 3.0 * max(d_own, d_ref or 0.0) + 4.0 * U32
    print("diag-ef triple " + json.dumps({"case": case, "engine": d_eng, "diag_EF_autograd": d_own, "reference": d_ref,
                                          "bound": bound}))
    within(d_eng, bound, note=case)
    return bound


# ---- (a) the reference's own test problem and its stored vectors -------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 16])
@pytest.mark.parametrize("key", KEYS)
def test_small_nn_diagonal_against_float64_and_the_reference(golden, key, rows):
    g = golden("curvature.npz")
    model = small_nn(g, key, device=DEV)  # (layer 1 frozen, as tests/test_utils.py:39-43)
    x, t = T(g[key + "/inputs"], DEV)[:rows], T(g[key + "/targets"], DEV)[:rows]
    reduction = key.rsplit("_", 1)[1]
    lossf = torch.nn.MSELoss(reduction=reduction)
    got, eng, d32, d64 = diagonals(model, lossf, x, t, reduction)
    # the dead prefix is skipped and the first live layer issues no data gradient
    assert eng.dead_layers == 1 and eng.layers[1].first_live and eng.layers[1].dslabs is None and eng.rows == rows
    assert got.numel() == eng.n == 48
    ref = T(g[f"{key}/diagEF_n{rows}"], DEV)
    bound = check(f"{key}/n{rows}", got, d32, d64, ref)
    within(dist(got, ref), bound + dist(ref, d64), note=key)  # (the reference sits that far from float64 itself)


# ---- (b) frozen patterns ---------------------------------------------------------------------------------------------
def _freeze(model, pattern):
    lins = [m for m in model.modules() if isinstance(m, torch.nn.Linear)]
    frozen = {"none": [], "first_weight": [lins[0].weight], "middle_bias": [lins[1].bias],
              "last_layer": [lins[-1].weight, lins[-1].bias]}[pattern]
    for p in frozen:
        p.requires_grad = False


@pytest.mark.parametrize("pattern", ["none", "first_weight", "middle_bias", "last_layer"])
def test_frozen_patterns_have_exactly_the_trainable_entries(pattern):
    model, (x, t), lossf = tp.small_nn(device=DEV, freeze_layer1=False)
    _freeze(model, pattern)
    n = sum(p.numel() for p in trainable(model))
    got, eng, d32, d64 = diagonals(model, lossf, x, t, "mean")
    assert eng.dead_layers == 0 and eng.n == n and got.numel() == n == d64.numel()
    check(f"small_nn/{pattern}", got, d32, d64)


# ---- (c) tanh / cross-entropy and the bias-free MSE example ----------------------------------------------------------------
def _tanh_net(reduction="mean"):
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(3072, 64), torch.nn.Tanh(), torch.nn.Linear(64, 48), torch.nn.Tanh(),
                              torch.nn.Linear(48, 100))
    gen = torch.Generator().manual_seed(1)
    x, t = torch.rand(17, 3072, generator=gen), torch.randint(0, 100, (17,), generator=gen)
    return net.to(DEV), (x.to(DEV), t.to(DEV)), torch.nn.CrossEntropyLoss(reduction=reduction)


@pytest.mark.parametrize("problem,reduction", [("mwe_mlp", "mean"), ("tanh_ce", "mean"), ("tanh_ce", "sum")])
def test_diagonal_against_float64_and_diag_ef_autograd(problem, reduction):
    model, (x, t), lossf = tp.mwe_mlp(device=DEV) if problem == "mwe_mlp" else _tanh_net(reduction)
    got, eng, d32, d64 = diagonals(model, lossf, x, t, reduction)
    assert eng.dead_layers == 0 and (eng._ce is None) == (problem == "mwe_mlp")
    check(f"{problem}/{reduction}", got, d32, d64)


# ---- (d) repeatability, graph capture, the guard ---------------------------------------------------------------------------
def test_two_calls_and_a_graph_replay_are_bitwise_equal():
    model, (x, t), lossf = _tanh_net()
    modelprep.prepare_model(model)
    eng = engine_for(model, lossf, x, t)
    a = eng.diag_ef("mean").clone()
    out = torch.full((eng.n,), float("nan"), device=DEV)
    assert eng.diag_ef("mean", out=out) is out
    assert torch.equal(a.view(torch.int32), out.view(torch.int32))
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    eng.diag_ef("mean", out=out)
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before  # (no allocation once the buffers exist)
    static = torch.full((eng.n,), float("nan"), device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.diag_ef("mean", out=static)
    static.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), static.view(torch.int32))


def test_a_reduction_other_than_the_losss_own_raises():
    model, (x, t), lossf = tp.mwe_mlp(device=DEV)
    modelprep.prepare_model(model)
    eng = engine_for(model, lossf, x, t)
    with pytest.raises(RuntimeError, match="reduction differs"):
        eng.diag_ef("sum")
    with pytest.raises(ValueError):
        eng.diag_ef("max")
    # (the public route keeps answering such a call as before: the vmap construction)
    why = []
    got = preconditioners.diag_EF_backpack(model, lossf, x, t, "sum", why=why)
    assert any("differs from the requested one" in w for w in why), why
    assert _same(got, preconditioners._diag_EF_vmap(model, lossf, x, t, "sum"))


# ---- (e) the public route ------------------------------------------------------------------------------------------------
def test_diag_ef_backpack_returns_the_engines_vector():
    model, (x, t), lossf = _tanh_net()
    modelprep.prepare_model(model)
    want = engine_for(model, lossf, x, t).diag_ef("mean").clone()
    why = []
    got = preconditioners.diag_EF_backpack(model, lossf, x, t, "mean", why=why)
    assert not why, why
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(hf.diag_EF_preconditioner(model, lossf, x, t, "mean", 0.5).diag.view(torch.int32),
                       want.view(torch.int32))


def test_get_preconditioner_and_a_preconditioned_step_run_on_the_engine():
    """``(d + lam)^-0.75`` moves by ``0.75 * delta / (d + lam)`` (relative) when ``d`` moves by ``delta``: an ENTRYWISE
    relative bound ``b`` on ``d`` gives at most ``0.75 b`` for ``d, lam > 0``; the max-norm bound ``B * max d`` used here
    gives ``0.75 * B * max d / (d_j + lam)`` at entry ``j``.  To that comes what the fp32 power and multiplication of
    ``DiagonalPreconditioner`` themselves add, measured on the float64 diagonal rounded to fp32 (factor 3, plus one
    ``u`` for that rounding)."""
    model, (x, t), lossf = _tanh_net()
    d64 = loop64(model, lossf, x, t, "mean")
    d32 = preconditioners.diag_EF_autograd(copy.deepcopy(model), lossf, x, t, "mean")
    B = 3.0 * dist(d32, d64) + 4.0 * U32
    modelprep.prepare_model(model)
    opt = hf.HessianFree(model.parameters(), graph_matvec=True)
    lam = opt.param_groups[0]["damping"]
    assert lam > 0
    M = opt.get_preconditioner(model, lossf, x, t, "mean")
    within(dist(M.diag, d64), B)
    v = torch.randn(d64.numel(), device=DEV, generator=torch.Generator(device=DEV).manual_seed(8))
    want = preconditioners.diag_to_preconditioner(d64.cpu(), lam)(v.double().cpu()).to(DEV)
    rel = lambda a: (a.double() - want).abs() / want.abs().clamp_min(1e-300)  # noqa: E731
    own = float(rel(preconditioners.diag_to_preconditioner(d64.float(), lam)(v)).max())
    allowed = 0.75 * B * d64.max() / (d64 + lam) + 3.0 * own + U32
    within(float((rel(M(v)) / allowed).max()), 1.0)

    def forward():
        o = model(x)
        return lossf(o, t), o

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        final = opt.step(forward, M_func=M)
    rep = opt.path_report()["step"]
    assert rep["path"] == "engine-graphed", rep
    assert final <= opt.state["init_losses"][-1]


# ---- (f) what falls through, bitwise equal to the vmap construction, and why ------------------------------------------------
def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_falls_through_with_the_switch_unset(monkeypatch):
    monkeypatch.delenv("HF_DENSE_ENGINE")
    model, (x, t), lossf = tp.mwe_mlp(device=DEV)
    modelprep.prepare_model(model)
    why = []
    assert diag_ef_of(model, lossf, x, t, "mean", why=why) is None
    assert any("set HF_DENSE_ENGINE=1" in w for w in why), why
    got = preconditioners.diag_EF_backpack(model, lossf, x, t, "mean")
    assert _same(got, preconditioners._diag_EF_vmap(model, lossf, x, t, "mean"))


def test_falls_through_for_a_stock_model_a_sigmoid_net_and_batch_300():
    lossf = torch.nn.MSELoss()
    stock, (x, t), _ = tp.mwe_mlp(device=DEV)
    torch.manual_seed(0)
    sig = torch.nn.Sequential(torch.nn.Linear(10, 10), torch.nn.Sigmoid(), torch.nn.Linear(10, 10)).to(DEV)
    modelprep.prepare_model(sig)
    big, (xb, tb), _ = tp.mwe_mlp(batch_size=300, device=DEV)
    modelprep.prepare_model(big)
    for model, xs, ts, reason in ((stock, x, t, "not a prepared one"), (sig, x, t, "unsupported layer Sigmoid"),
                                  (big, xb, tb, "batch 300 > 256 rows")):
        why = []
        got = preconditioners.diag_EF_backpack(model, lossf, xs, ts, "mean", why=why)
        assert any(reason in w for w in why), (reason, why)
        assert _same(got, preconditioners._diag_EF_vmap(model, lossf, xs, ts, "mean")), reason
        # (and the vmap construction is the per-sample loop's quantity)
        loop = preconditioners.diag_EF_autograd(model, lossf, xs, ts, "mean")
        within(float((got - loop).abs().max() / loop.abs().max()), 1e-5, note=reason)


def test_a_loss_the_engine_does_not_read_falls_through():
    model, (x, t), _ = tp.mwe_mlp(device=DEV)
    modelprep.prepare_model(model)
    lossf = torch.nn.L1Loss()
    why = []
    got = preconditioners.diag_EF_backpack(model, lossf, x, t, "mean", why=why)
    assert any("neither a plain softmax cross-entropy nor a mean-squared error" in w for w in why), why
    assert _same(got, preconditioners._diag_EF_vmap(model, lossf, x, t, "mean"))
