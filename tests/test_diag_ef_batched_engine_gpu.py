"""GPU: ``engine.diag_ef`` of the conv-unit engines with ``HF_DIAG_EF_BATCHED=1`` -- per unit ONE squared-sum convolution
(``hf_conv2d_nhwc_sqsum_slabs``) and ONE squared channel sum (``hf_chan_sqsum``) on the whole batch, ONE gather -- against
the per-sample autograd loop of ``test_engine_diag_ef_matches_per_sample_autograd`` on the same model, at that test's own
bound (1e-5 max-norm relative, through ``tol.within``; the switch-off sweep is measured at the same site so that the
tolerance log shows both).  The nets are those of ``engine_nets``: ``wide`` (batch 16, maps 8x8 -> 4x4 -> 2x2 -> 1x1: the
per-sample and the squared-operand form, the stem's im2col, a downsample unit), with frozen scales / shifts, as a Hessian
engine (cotangents in ``ga1`` / ``g1``), and the conv + bias stack of the plain-stack engine (no head)."""

import warnings

import pytest
import torch
from torch import nn

import engine_nets as en
import pytorchhessianfree_amd as hf
from pytorchhessianfree_amd import _lib, modelprep
from pytorchhessianfree_amd import testproblems as tp
from pytorchhessianfree_amd.engine import FusedGGNEngine, PlainStackEngine
from tol import within

pytestmark = pytest.mark.gpu
DEV = en.DEV
SWITCH = "HF_DIAG_EF_BATCHED"
NEW = ("hf_conv2d_nhwc_sqsum_slabs", "hf_chan_sqsum")
KINDS = ["wide", "wide_frozen", "wide_hessian", "stack"]


def make(kind, reduction="mean", batch=None):
    """``(engine, model, x, t, loss function)`` of one of the nets of ``engine_nets`` (its seeds, statistics and freezing
    patterns), with the loss's reduction and the batch size as asked."""
    if kind == "stack":
        torch.manual_seed(7)
        model, classes, shape = en.SmallConvStack(), 12, (batch or 4, 3, 8, 8)
    else:
        spec = en.NETS["wide"]
        torch.manual_seed(5)
        model, classes, shape = en.SmallResNet(spec["ch"], spec["blocks"]), 10, (batch or spec["batch"], 1, 8, 8)
        with torch.no_grad():
            for m in model.modules():
                if isinstance(m, nn.BatchNorm2d):
                    m.running_mean.uniform_(-0.2, 0.2)
                    m.running_var.uniform_(0.7, 1.4)
                    m.weight.uniform_(0.6, 1.3)
                    m.bias.uniform_(-0.2, 0.2)
                    m.eps = 0.1
        en._freeze(model, "scale_shift" if kind == "wide_frozen" else "plain")
    model.eval()
    x, t = torch.randn(*shape).to(DEV), torch.randint(0, classes, (shape[0],)).to(DEV)
    model = model.to(DEV)
    modelprep.prepare_model(model, channels_last=True)
    params = [p for p in model.parameters() if p.requires_grad]
    lossf = nn.CrossEntropyLoss(reduction=reduction)
    out = model(x)
    why = []
    eng = FusedGGNEngine.try_build(lossf(out, t), out, params, hessian=kind == "wide_hessian", why=why)
    assert isinstance(eng, PlainStackEngine if kind == "stack" else FusedGGNEngine), why
    assert eng.hessian == (kind == "wide_hessian")
    return eng, model, x, t, lossf


def per_sample_autograd(model, x, t, lossf, reduction):
    """The reference's loop (preconditioners.py:91-99) on batches of ONE sample."""
    params = [p for p in model.parameters() if p.requires_grad]
    want = None
    for i in range(x.shape[0]):
        g_i = torch.autograd.grad(lossf(model(x[i:i + 1]), t[i:i + 1]), params)
        sq = torch.cat([g.reshape(-1) for g in g_i]) ** 2
        want = sq if want is None else want + sq
    return want / x.shape[0] if reduction == "mean" else want


class Names:
    """``_lib.load`` proxy (as the launch-sequence test's): the names of the ``hf_*`` entry points that are called."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in _lib.SIGNATURES:
            return fn

        def call(*args):
            self.names.append(name)
            return fn(*args)

        return call


def recorded_names(monkeypatch, eng, reduction="mean"):
    rec = Names(_lib.load())
    with monkeypatch.context() as m:
        m.setattr(_lib, "load", lambda: rec)
        eng.diag_ef(reduction)
        torch.cuda.synchronize()
    return rec.names


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("kind", KINDS)
def test_batched_diag_ef_matches_per_sample_autograd(kind, reduction, monkeypatch):
    monkeypatch.setenv("HF_ENGINE_VERIFY", "never")
    results = {}
    for switch in ("0", "1"):
        monkeypatch.setenv(SWITCH, switch)
        eng, model, x, t, lossf = make(kind, reduction)
        assert eng._diag_batched == (switch == "1")
        got = eng.diag_ef(reduction).clone()
        want = per_sample_autograd(model, x, t, lossf, reduction)
        assert float(want.abs().max()) > 0
        # (one site for both routes: the tolerance log then holds the worse of the two, the printed line each of them)
        err = float((got - want).abs().max() / want.abs().max())
        print("diag_ef %s %s switch=%s: max-norm relative error %.3e" % (kind, reduction, switch, err))
        within(err, 1e-5)
        results[switch] = (eng, got)
    eng, got = results["1"]
    assert torch.equal(eng.diag_ef(reduction), got)  # bitwise repeatable
    out = torch.empty_like(got)
    assert eng.diag_ef(reduction, out=out) is out and torch.equal(out, got)
    # the products of the same engine are untouched by the sweep's buffers
    v = torch.randn(eng.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    a = eng(v).clone()
    eng.diag_ef(reduction)
    assert torch.equal(eng(v), a)
    # every unit contributes: the two routes agree entry by entry (each is within 1e-5 of the same reference, so
    # within 2e-5 of the other by the triangle inequality) and no entry is left at zero by one route alone
    within(float((got - results["0"][1]).abs().max() / got.abs().max()), 2e-5)
    assert bool(((got != 0) == (results["0"][1] != 0)).all())


@pytest.mark.parametrize("kind", KINDS)
def test_batched_sweep_is_one_gather_and_a_batch_independent_number_of_launches(kind, monkeypatch):
    monkeypatch.setenv("HF_ENGINE_VERIFY", "never")
    monkeypatch.setenv(SWITCH, "1")
    counts = {}
    for batch in (4, 8) if kind == "stack" else (8, 16):
        eng = make(kind, batch=batch)[0]
        eng.diag_ef("mean")  # (first use: buffers)
        names = recorded_names(monkeypatch, eng)
        # ``gradient()`` runs exactly as ever, its own gather of the gradient included; behind it: exactly ONE gather
        sweep = recorded_names_of_gradient(monkeypatch, eng)
        assert sweep.count("hf_pack_ex") == 1 and names[:len(sweep)] == sweep
        tail = names[len(sweep):]
        assert tail.count("hf_pack_ex") == 1
        assert tail[-1] == "hf_pack_ex" and set(tail[:-1]) <= set(NEW)
        live = [u for u in eng.units if not u.dead]
        assert tail.count(NEW[0]) == sum(u.pw is not None for u in live)
        assert tail.count(NEW[1]) == sum(u.pg is not None or u.pb is not None for u in live)
        # (the adjoint sweep in front is today's: whether a block's two adjoints share a launch depends on the maps' sizes,
        # so ITS count may move with the batch; what this sweep adds behind it must not)
        counts[batch] = len(tail)
    assert len(set(counts.values())) == 1, counts


def recorded_names_of_gradient(monkeypatch, eng):
    """The adjoint sweep alone, as ``diag_ef`` runs it (without the tagged L2 term)."""
    rec = Names(_lib.load())
    with monkeypatch.context() as m:
        m.setattr(_lib, "load", lambda: rec)
        eng.gradient()
        torch.cuda.synchronize()
    return rec.names


def test_without_the_switch_no_new_entry_point_is_called(monkeypatch):
    """``HF_DIAG_EF_BATCHED`` is opt-in: unset (and at "0") the sweep is the per-sample one -- one squaring gather per
    sample, neither new entry point; at "1" both are called and the per-sample launches are gone."""
    monkeypatch.setenv("HF_ENGINE_VERIFY", "never")
    for value, batched in ((None, False), ("0", False), ("1", True)):
        if value is None:
            monkeypatch.delenv(SWITCH, raising=False)
        else:
            monkeypatch.setenv(SWITCH, value)
        eng = make("wide")[0]
        assert eng._diag_batched == batched
        eng.diag_ef("mean")  # (first use: the planner's answers, buffers)
        names = recorded_names(monkeypatch, eng)
        assert all((name in names) == batched for name in NEW), (value, sorted(set(names)))
        n = eng.x_in.shape[0]
        sweep = recorded_names_of_gradient(monkeypatch, eng)
        assert names[:len(sweep)] == sweep
        assert names[len(sweep):].count("hf_pack_ex") == (1 if batched else n)
    # read once, when the engine is built: the environment of a later call does not matter
    monkeypatch.setenv(SWITCH, "0")
    assert all(name in recorded_names(monkeypatch, eng) for name in NEW)


def test_train_mode_engine_still_refuses_before_any_launch(monkeypatch):
    monkeypatch.setenv("HF_ENGINE_VERIFY", "never")
    monkeypatch.setenv(SWITCH, "1")
    eng = en.build("wide", train=True)
    rec = Names(_lib.load())
    with monkeypatch.context() as m:
        m.setattr(_lib, "load", lambda: rec)
        with pytest.raises(RuntimeError, match="eval-mode BatchNorm"):
            eng.diag_ef("mean")
    assert rec.names == []


def test_get_preconditioner_on_the_session_with_the_batched_sweep(monkeypatch):
    """Mirror of ``test_get_preconditioner_uses_the_sessions_engine_from_the_second_step`` under the switch: All-CNN-C at
    batch 8 with the tagged L2 term; the session captures whatever the engine issues."""
    monkeypatch.setenv(SWITCH, "1")
    model, (x, t), lossf0 = tp.allcnnc_cifar100(batch_size=8, device=DEV, data_seed=4)
    lossf = tp.l2_regularized(lossf0, model, 5e-4)
    modelprep.prepare_model(model, channels_last=True)
    opt = hf.HessianFree(model.parameters(), curvature_opt="hessian", graph_matvec=True, cg_max_iter=5)

    def forward():
        o = model(x)
        return lossf(o, t), o

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        M0 = opt.get_preconditioner(model, lossf, x, t, "mean", use_backpack=False)   # no session yet
        opt.step(forward, M_func=M0)
        assert opt._session is not None and opt._session.engine._diag_batched
        M1 = opt.get_preconditioner(model, lossf, x, t, "mean", use_backpack=False)   # the engine's sweep, captured
        first = M1.diag.clone()
        want = hf.diag_EF_autograd(model, lossf, x, t, "mean")
        within(float((first - want).abs().max() / want.abs().max()), 1e-5)
        M2 = opt.get_preconditioner(model, lossf, x, t, "mean", use_backpack=False)   # a replay
        assert torch.equal(M2.diag, first)
        final = opt.step(forward, M_func=M2)
        assert final <= opt.state["init_losses"][-1]
