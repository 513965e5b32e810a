"""GPU: the dense-stack engine's session mode (``engine/dense.py`` with ``HF_DENSE_SESSION=1``) and
``HessianFree.step()`` on a persistent session of it: first build against float64 of the STOCK model; a new batch / moved
parameters against an engine freshly built there (bitwise); the session's graphs against the eager calls (bitwise);
``step()`` against the prepared twin without the switch (``engine-graphed``); what declines the session.

Bounds.  Against float64: ``3 x`` the distance another fp32 evaluation of the same quantity (fp32 autograd of the stock
model) keeps from float64, both measured here; every such comparison asserts that the reference distance is not zero.
A scalar (a loss value) is one number that fp32 rounds correctly as often as not, so loss values are compared as the
vector of their relative errors over the problems / trial points of a test.  The session's own thresholds (loss 1e-5,
logits 1e-4) are the optimizer's.

Every test sets ``HF_DENSE_ENGINE=1`` and ``HF_DENSE_SESSION=1`` unless it is about the switch."""

import copy
import warnings

import pytest
import torch
from tol import within

import pytorchhessianfree_amd as hf
from pytorchhessianfree_amd import modelprep, preconditioners
from pytorchhessianfree_amd import testproblems as tp
from pytorchhessianfree_amd.engine import FusedGGNEngine, _Unsupported
from pytorchhessianfree_amd.engine.dense import DenseStackEngine
from pytorchhessianfree_amd.session import EngineSession
from pytorchhessianfree_amd.utils import ParameterArena

pytestmark = pytest.mark.gpu
DEV = "cuda"
FROZEN = ["none", "first_layer", "first_weight", "middle_bias", "last_layer"]


@pytest.fixture(autouse=True)
def _dense_session_on(monkeypatch):
    monkeypatch.setenv("HF_DENSE_ENGINE", "1")
    monkeypatch.setenv("HF_DENSE_SESSION", "1")


def trainable(model):
    return [p for p in model.parameters() if p.requires_grad]


def dist(a, b):
    """max-norm distance relative to max |b| (b: the float64 result)."""
    b = b.double()
    return float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-300))


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def _tanh_net():
    """The net of ``test_dense_engine_gpu.py``: 3072-64-48-100, tanh, cross-entropy, 17 rows."""
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(3072, 64), torch.nn.Tanh(), torch.nn.Linear(64, 48), torch.nn.Tanh(),
                              torch.nn.Linear(48, 100))
    gen = torch.Generator().manual_seed(1)
    x, t = torch.rand(17, 3072, generator=gen), torch.randint(0, 100, (17,), generator=gen)
    return net.to(DEV), (x.to(DEV), t.to(DEV)), torch.nn.CrossEntropyLoss()


def _freeze(model, pattern):
    lins = [m for m in model.modules() if isinstance(m, torch.nn.Linear)]
    frozen = {"none": [], "first_layer": [lins[0].weight, lins[0].bias], "first_weight": [lins[0].weight],
              "middle_bias": [lins[1].bias], "last_layer": [lins[-1].weight, lins[-1].bias]}[pattern]
    for p in frozen:
        p.requires_grad = False
    return frozen


def problem(name):
    """(stock model, (x, t), loss function) of ``mwe_mlp``, ``tanh_ce`` or ``small_nn/<frozen pattern>``."""
    if name == "mwe_mlp":
        return tp.mwe_mlp(device=DEV)
    if name == "tanh_ce":
        return _tanh_net()
    model, data, lossf = tp.small_nn(device=DEV, freeze_layer1=False)
    _freeze(model, name.split("/")[1])
    return model, data, lossf


PROBLEMS = ["mwe_mlp", "tanh_ce"] + ["small_nn/" + p for p in FROZEN]


def other_batch(x, t, seed=3):
    gen = torch.Generator().manual_seed(seed)
    x2 = torch.rand(x.shape, generator=gen).to(DEV) if float(x.min()) >= 0 else torch.randn(x.shape, generator=gen).to(DEV)
    if t.dtype.is_floating_point:
        return x2, torch.randn(t.shape, generator=gen).to(DEV)
    return x2, torch.randint(0, int(t.max()) + 1, t.shape, generator=gen).to(DEV)


def build(model, x, t, lossf, weight=1.0, hessian=False):
    """The session-capable engine of a PREPARED model on ``(x, t)``."""
    out = model(x)
    why = []
    eng = FusedGGNEngine.try_build(lossf(out, t), out, trainable(model), weight=weight, hessian=hessian, why=why,
                                   need_session=True)
    assert isinstance(eng, DenseStackEngine) and eng.loss_spec is not None and eng.supports_session, why
    return eng


def stock_eval(model, x, t, lossf, dtype, weight=1.0):
    """(logits, loss, weight * gradient) of a copy of the STOCK model in ``dtype``."""
    m = copy.deepcopy(model).to(dtype)
    out = m(x.to(dtype))
    loss = lossf(out, t.to(dtype) if t.dtype.is_floating_point else t)
    g = torch.cat([q.reshape(-1) for q in torch.autograd.grad(loss, trainable(m))]) * weight
    return out.detach(), loss.detach(), g


def state(eng, v):
    """Everything a step reads off the engine at its current point: logits, loss, gradient, one product, diagonal."""
    grad = torch.full((eng.n,), float("nan"), device=DEV)
    eng.gradient(grad)
    return dict(logits=eng.logits.clone(), loss=eng.loss_buf.clone(), grad=grad, prod=eng(v).clone(),
                diag=eng.diag_ef(eng.loss_spec["reduction"]).clone(), bad=eng.bad_targets.clone())


def assert_same_state(a, b, note):
    for k in a:
        assert same(a[k], b[k]), (note, k)


# ---- first build -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight", [1.0, 0.375])
@pytest.mark.parametrize("name", PROBLEMS)
def test_first_build_logits_and_gradient_against_float64(name, weight):
    model, (x, t), lossf = problem(name)
    o64, _, g64 = stock_eval(model, x, t, lossf, torch.float64, weight)
    o32, _, g32 = stock_eval(model, x, t, lossf, torch.float32, weight)
    modelprep.prepare_model(model)
    eng = build(model, x, t, lossf, weight=weight)
    assert eng.outputs is None and all(getattr(m, "_hf_io", None) is None for m in model.modules())  # records dropped
    assert int(eng.bad_targets) == 0 and eng.weight == weight
    grad = torch.full((eng.n,), float("nan"), device=DEV)
    assert eng.gradient(grad) is grad
    for what, got, r32, w64 in (("logits", eng.logits, o32, o64), ("gradient", grad, g32, g64)):
        d_got, d_ref = dist(got, w64), dist(r32, w64)
        print(f"{name} w={weight} {what}: engine {d_got:.3e}  fp32 autograd {d_ref:.3e}")
        assert d_ref > 0.0, what
        within(d_got, 3.0 * d_ref, strict=False, note=(name, weight, what))


def test_first_build_loss_values_against_float64():
    """``loss_buf`` of every problem: the relative errors as one vector."""
    got, ref = [], []
    for name in PROBLEMS:
        model, (x, t), lossf = problem(name)
        l64 = float(stock_eval(model, x, t, lossf, torch.float64)[1])
        l32 = float(stock_eval(model, x, t, lossf, torch.float32)[1])
        modelprep.prepare_model(model)
        eng = build(model, x, t, lossf)
        got.append(abs(float(eng.loss_buf.double()) - l64) / abs(l64))
        ref.append(abs(l32 - l64) / abs(l64))
    print(f"first-build losses: engine {max(got):.3e}  fp32 autograd {max(ref):.3e}")
    assert max(ref) > 0.0
    within(max(got), 3.0 * max(ref), strict=False, note=(got, ref))


# ---- a new batch, moved parameters: bitwise a fresh engine -------------------------------------------------------------
@pytest.mark.parametrize("name", PROBLEMS)
def test_new_batch_equals_a_fresh_engine(name):
    model, (x, t), lossf = problem(name)
    modelprep.prepare_model(model)
    x2, t2 = other_batch(x, t)
    v = torch.randn(sum(p.numel() for p in trainable(model)), device=DEV,
                    generator=torch.Generator(device=DEV).manual_seed(5))
    eng = build(model, x, t, lossf)
    state(eng, v)  # (everything has run once on the first batch: a stale buffer would show below)
    with torch.no_grad():
        eng.set_batch(x2, t2)
        eng.forward_own(refresh=True)
    a = state(eng, v)
    b = state(build(model, x2, t2, lossf), v)
    assert_same_state(a, b, name)
    with pytest.raises(RuntimeError, match="input shape changed"):
        eng.set_batch(x2[:-1] if x2.shape[0] > 1 else torch.cat([x2, x2]))


@pytest.mark.parametrize("name", ["tanh_ce", "small_nn/first_weight", "small_nn/first_layer", "small_nn/middle_bias"])
def test_parameters_moved_in_place_equal_a_fresh_engine(name):
    """The optimizer's arena moves the trainable parameters in place; a frozen weight is written in place too (the
    kernels read it where it is: there is no copy that could be stale)."""
    model, (x, t), lossf = problem(name)
    frozen = [p for p in model.parameters() if not p.requires_grad]
    modelprep.prepare_model(model)
    arena = ParameterArena(model.parameters())
    v = torch.randn(arena.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(6))
    eng = build(model, x, t, lossf)
    assert eng._flat_params is not None and eng._flat_params.data_ptr() == arena.theta.data_ptr()
    state(eng, v)
    step = 0.05 * torch.randn(arena.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
    arena.write(arena.snapshot(), step, 0.5)
    with torch.no_grad():
        for p in frozen:
            p.mul_(1.01).add_(0.003)
        eng.refresh_weights(transposed=True)  # (no-ops: nothing to forget)
        eng.refresh_frozen()
        eng.forward_own(refresh=True)
    a = state(eng, v)
    b = state(build(model, x, t, lossf), v)
    assert_same_state(a, b, name)


# ---- the session's graphs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mwe_mlp", "tanh_ce", "small_nn/first_weight"])
def test_session_graphs_replay_the_eager_calls_bitwise_and_trial_losses_against_float64(name):
    model, (x, t), lossf = problem(name)
    stock = copy.deepcopy(model)
    modelprep.prepare_model(model)
    arena = ParameterArena(model.parameters())
    out = model(x)
    why = []
    sess = EngineSession.try_create(lossf(out, t), out, trainable(model), why=why)
    assert sess is not None, why
    eng = sess.engine
    assert isinstance(eng, DenseStackEngine)
    red = eng.loss_spec["reduction"]
    v = torch.randn(arena.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(8))
    nan = float("nan")
    with torch.no_grad():
        eng.forward_own(refresh=True)
        want = state(eng, v)
        for buf in (eng.logits, eng.loss_buf, eng._h_last, eng._g_ef):
            buf.fill_(nan)
        sess.g_fwd.replay()
        assert same(eng.logits, want["logits"]) and same(eng.loss_buf, want["loss"])
        sess.grad_buffer.fill_(nan)
        assert same(sess.gradient(), want["grad"])
        sess.input_buffer.copy_(v)
        sess.output_buffer.fill_(nan)
        sess.graph.replay()
        assert same(sess.output_buffer, want["prod"])
        assert same(sess.diag_ef(red), want["diag"]) and same(sess.diag_ef(red), want["diag"])
    # trial points theta0 + alpha * s: one arena write and one replay each; the losses in ONE read-back
    base = arena.snapshot()
    s = 0.1 * torch.randn(arena.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9))
    alphas = [1.0, 0.5, 0.25, -0.3]
    l32, l64 = [], []
    for k, alpha in enumerate(alphas):
        arena.write(base, s, alpha)
        sess.forward_loss(k)
        stock.load_state_dict({k2: v2.detach().clone() for k2, v2 in model.state_dict().items()})
        l64.append(float(stock_eval(stock, x, t, lossf, torch.float64)[1]))
        l32.append(float(stock_eval(stock, x, t, lossf, torch.float32)[1]))
    got = sess.losses[:len(alphas)].double().tolist()
    e_got = max(abs(a - b) / abs(b) for a, b in zip(got, l64))
    e_ref = max(abs(a - b) / abs(b) for a, b in zip(l32, l64))
    print(f"{name} trial losses: session {e_got:.3e}  fp32 stock model {e_ref:.3e}")
    assert e_ref > 0.0
    within(e_got, 3.0 * e_ref, strict=False, note=(name, got, l32, l64))


# ---- step() ---------------------------------------------------------------------------------------------------------------
def _steps(name, n_steps=3, **opts):
    model, (x, t), lossf = problem(name)
    modelprep.prepare_model(model)
    opt = hf.HessianFree(model.parameters(), graph_matvec=True, **opts)

    def forward():
        o = model(x)
        return lossf(o, t), o

    finals, msgs = [], []
    for _ in range(n_steps):
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            finals.append(opt.step(forward))
        msgs += [str(w.message) for w in rec]
    return opt, finals, msgs, (model, x, t, lossf, forward)


def _compare_with_twin(a, fa, b, fb):
    """As ``test_dense_engine_gpu.py`` compares its twins: everything discrete up to the first differing back-tracking
    pick, the losses within its bounds."""
    n_steps = len(fa)
    same_upto = n_steps
    for i, (p, q) in enumerate(zip(a.state["best_cg_iters"], b.state["best_cg_iters"])):
        if int(p) != int(q):
            same_upto = i
            break
    for key in ("learning_rates", "dampings", "cg_reasons"):
        assert list(a.state[key])[:same_upto] == list(b.state[key])[:same_upto], (key, a.state[key], b.state[key])
    for i in range(min(same_upto + 1, n_steps)):
        p, q = a.state["init_losses"][i], b.state["init_losses"][i]
        within(abs(p - q), (1e-5 if i == 0 else 3e-5) * abs(q), strict=False,
               note=(a.state["init_losses"], b.state["init_losses"]))
        within(abs(fa[i] - fb[i]), (1e-4 if i == 0 else 5e-4) * abs(fb[i]), strict=False, note=(fa, fb))


@pytest.mark.parametrize("name", ["mwe_mlp", "tanh_ce"])
def test_three_steps_run_on_the_session_and_equal_the_twin_without_the_switch(name, monkeypatch):
    a, fa, msgs, _ = _steps(name)
    assert a.path_report()["step"]["path"] == "session", a.path_report()["step"]
    assert not [m for m in msgs if "slower path" in m], msgs
    assert a._session is not None and a._session.steps == 3 and isinstance(a._session.engine, DenseStackEngine)
    monkeypatch.delenv("HF_DENSE_SESSION")
    b, fb, _, _ = _steps(name)
    assert b.path_report()["step"]["path"] == "engine-graphed", b.path_report()["step"]
    _compare_with_twin(a, fa, b, fb)


def test_hessian_steps_run_on_the_session_and_equal_the_twin_without_the_switch(monkeypatch):
    """``mwe_mlp`` only, both twins on the dense engine's own Hessian products (no capture of autograd double backward
    anywhere in this file)."""
    monkeypatch.setenv("HF_DENSE_HESSIAN", "1")
    a, fa, msgs, _ = _steps("mwe_mlp", curvature_opt="hessian")
    assert a.path_report()["step"]["path"] == "session", a.path_report()["step"]
    assert not [m for m in msgs if "slower path" in m], msgs
    assert a._session.steps == 3 and a._session.engine.hessian
    monkeypatch.delenv("HF_DENSE_SESSION")
    b, fb, _, _ = _steps("mwe_mlp", curvature_opt="hessian")
    assert b.path_report()["step"]["path"] == "engine-graphed", b.path_report()["step"]
    _compare_with_twin(a, fa, b, fb)


def test_hessian_engine_on_a_new_batch_equals_a_fresh_engine(monkeypatch):
    """The tanh / cross-entropy net in Hessian mode, engine level only: after ``set_batch`` and a new forward pass,
    ``gradient()`` followed by a product is bitwise a fresh engine's."""
    monkeypatch.setenv("HF_DENSE_HESSIAN", "1")
    model, (x, t), lossf = _tanh_net()
    modelprep.prepare_model(model)
    x2, t2 = other_batch(x, t)
    v = torch.randn(sum(p.numel() for p in trainable(model)), device=DEV,
                    generator=torch.Generator(device=DEV).manual_seed(10))
    eng = build(model, x, t, lossf, hessian=True)
    assert eng.hessian
    state(eng, v)
    with torch.no_grad():
        eng.set_batch(x2, t2)
        eng.forward_own(refresh=True)
    a = state(eng, v)
    b = state(build(model, x2, t2, lossf, hessian=True), v)
    assert_same_state(a, b, "tanh_ce hessian")


def test_session_is_reverified_and_rebuilt_when_a_layer_is_swapped(monkeypatch):
    monkeypatch.setenv("HF_SESSION_VERIFY", "1")
    a, _, msgs, (model, x, t, lossf, forward) = _steps("tanh_ce", n_steps=2)
    assert a.path_report()["step"]["path"] == "session" and a._session.steps == 2, (a.path_report()["step"], msgs)
    first = a._session
    before = first.engine.layer_signature()
    model[2] = copy.copy(model[2])  # another module object on the same parameters (its forward hook travels along)
    assert first.engine.layer_signature() != before
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a.step(forward)
    assert a.path_report()["step"]["path"] == "session", a.path_report()["step"]
    assert a._session is not first and a._session.steps == 1


def test_get_preconditioner_returns_the_sessions_diagonal():
    a, _, _, (model, x, t, lossf, forward) = _steps("tanh_ce", n_steps=1)
    assert a.path_report()["step"]["path"] == "session"
    M = a.get_preconditioner(model, lossf, x, t, "mean")
    eng = a._session.engine
    assert same(M.diag, eng.diag_ef("mean"))  # (the engine stands at the batch and parameters of that call)
    stock = _tanh_net()[0]
    stock.load_state_dict({k: v.detach().clone() for k, v in model.state_dict().items()})
    d32 = preconditioners.diag_EF_autograd(copy.deepcopy(stock), lossf, x, t, "mean")
    m64 = copy.deepcopy(stock).double()  # (the per-sample loop in float64: the truth)
    d64 = torch.zeros(eng.n, dtype=torch.float64, device=DEV)
    for i in range(x.shape[0]):
        g = torch.autograd.grad(lossf(m64(x[i].double()), t[i]), trainable(m64))
        d64 += torch.cat([q.reshape(-1) for q in g]) ** 2
    d64 /= x.shape[0]
    d_got, d_ref = dist(M.diag, d64), dist(d32, d64)
    print(f"get_preconditioner: session {d_got:.3e}  diag_EF_autograd fp32 {d_ref:.3e}")
    assert d_ref > 0.0
    within(d_got, 3.0 * d_ref, strict=False)


# ---- the switch, and what declines the session ---------------------------------------------------------------------------
def test_switch_and_declines(monkeypatch):
    """``HF_DENSE_SESSION``: without it the decline names it next to the old sentence; with it a regularised loss, a
    process group and ``acc_step`` decline with their reasons and the call completes on the next path."""
    monkeypatch.delenv("HF_DENSE_SESSION")
    a, _, _, _ = _steps("mwe_mlp", n_steps=1, cg_max_iter=2)
    rep = a.path_report()["step"]
    assert rep["path"] == "engine-graphed", rep
    assert "the dense-stack engine has no session yet" in rep["declined"] and "HF_DENSE_SESSION=1" in rep["declined"], rep
    monkeypatch.setenv("HF_DENSE_SESSION", "1")
    # a regularised loss
    model, (x, t), lossf = _tanh_net()
    modelprep.prepare_model(model)
    reg = tp.l2_regularized(lossf, model)
    opt = hf.HessianFree(model.parameters(), graph_matvec=True, cg_max_iter=2)

    def forward():
        o = model(x)
        return reg(o, t), o

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        opt.step(forward)
    rep = opt.path_report()["step"]
    assert rep["path"] == "engine-graphed" and "no quadratic regulariser" in rep["declined"], rep
    # data parallelism
    out = model(x)
    why = []
    assert EngineSession.try_create(lossf(out, t), out, trainable(model), group=object(), why=why) is None
    assert any("DenseStackEngine: data parallelism is not implemented" in w for w in why), why
    eng = build(model, x, t, lossf)
    # (one process only: the two-phase product's entry points do not exist on this kind, and the constructor -- above,
    # and here directly -- refuses a group before anything is laid out)
    for name in ("phase_split", "local_phase_a", "local_phase_b"):
        assert not hasattr(eng, name), name
    assert not eng.supports_two_phase and eng.group is None
    with pytest.raises(_Unsupported, match="data parallelism is not implemented for dense stacks"):
        DenseStackEngine(model, lossf(out, t), out, trainable(model), 1.0, object())
    from pytorchhessianfree_amd.session import ChunkedEngineOperator

    with pytest.raises(TypeError, match="needs the fused curvature engine"):
        ChunkedEngineOperator(lambda: eng)
    # acc_step (asked of the kind: no dense engine is built for it)
    opt = hf.HessianFree(model.parameters(), graph_matvec=True, cg_max_iter=2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        opt.acc_step(model, lossf, [(x, t)], reduction="mean")
    rep = opt.path_report()["acc_step"]
    assert rep["path"] != "acc-session" and "the dense-stack engine serves step() sessions only" in rep["declined"], rep
