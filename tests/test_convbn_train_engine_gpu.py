"""GPU: plain conv stacks with TRAIN-mode ``BatchNorm2d`` units on the plain-stack engine (``engine/plain.py``) -- batch
statistics in the forward pass, in the tangent (``S_x`` / ``S_1`` over all rows: an unpooled unit on the shared train-mode
launches, a pooled one on ``hf_pool_bn_act_tangent_train_nhwc``) and in the two-pass adjoint
(``hf_pool_bn_act_adjoint_reduce_nhwc``, then ``hf_chan_affine_train``) --, on ``testproblems.convbn_small`` /
``convbn_fc_small`` after ``model.train()``.

Reference sides: float64 autograd of the STOCK train-mode model on the engine's own ReLU and pooling decisions (the replay
of ``stack_harness.py``), and the fixture the real reference wrote in train mode
(``tests/golden/convnet_convbn_train.npz``, ``make_golden_convbn_train.py``).

The float64 bounds are 3x the worst figure of this package's STOCK fp32 autograd operator (``curvature.GGNOperator`` /
``HessianOperator`` through the stock layers, ``torch.autograd.grad``, the model's own output) against the same float64
twin on the same replayed decisions, over every case of the product and mixed-mode tests below -- the rule
``BOUND_TAIL`` was set by; ``scripts/convbn_train_errors.py`` measures both sides, ``profiles/r30_convbn_train.jsonl``
holds the figures.  Fixture comparisons use the fixture's own fp32-vs-float64 envelope (``RefTrace.envelope``)."""

import warnings

import pytest
import torch
from tol import within

import pytorchhessianfree_amd as hf
from helpers import RefTrace, compare_trace
from pytorchhessianfree_amd import curvature, modelprep
from pytorchhessianfree_amd import testproblems as tp
from pytorchhessianfree_amd.engine import FusedGGNEngine, PlainStackEngine
from stack_harness import DEV, _Net, declined, engine, float64_twin, grad64, product64, record_launches, rel, run_steps

pytestmark = pytest.mark.gpu
N_SMALL, N_FC = 1764, 1694
# 3x the worst stock_fp32 figure per quantity of profiles/r30_convbn_train.jsonl, one significant digit, rounded up
# (stock: ggn 1.31e-6, hessian 9.9e-7, grad 5.2e-7, logits 5.8e-7, loss 7.9e-8; the engine's own worst figures there:
# 1.31e-6, 8.1e-7, 5.0e-7, 4.8e-7, 5.4e-8)
BOUND = {"ggn": 4e-6, "hessian": 3e-6, "grad": 2e-6, "logits": 2e-6, "loss": 3e-7}
STEPS = {"small": (tp.convbn_small, 2), "fc": (tp.convbn_fc_small, 5)}
T_TRAIN, A_REDUCE = "hf_pool_bn_act_tangent_train_nhwc", "hf_pool_bn_act_adjoint_reduce_nhwc"


def _bns(model):
    return [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]


def _one_eval(model):
    _bns(model)[1].eval()  # (the unpooled unit's, inside a train-mode model)


def _one_train(model):
    model.eval()
    _bns(model)[2].train()  # (the pooled unit's without a ReLU, inside an eval-mode model)


def _one_train_first(model):
    model.eval()
    _bns(model)[0].train()  # (the im2col'd, pooled first unit's)


def _freeze_scales(model):
    for m in _bns(model):
        m.weight.requires_grad_(False)


def _freeze_first_unit(model):
    for m in list(model.net)[:2]:  # the first convolution and its BatchNorm
        for p in m.parameters():
            p.requires_grad_(False)


# every (family, batch, hessian, prep) the float64 bounds were measured on: items 1 and 3
POINTS = ([("small", b, h, None) for b in (2, 5) for h in (False, True)] + [("fc", b, False, None) for b in (2, 5)])
MIXED = [("small", 2, h, prep) for prep in (_one_eval, _one_train, _one_train_first, _freeze_scales, _freeze_first_unit)
         for h in (False, True)]


def _engine(family, batch, hessian=False, prep=None):
    """``model.train()`` first, ``prep`` then (the float64 twin of ``measure`` in the same modes)."""
    return engine(STEPS[family][0], batch, hessian, prep, train=True)


def measure(family, batch, hessian, prep, stock=False):
    """The distances to the float64 twin (on the ENGINE's decisions) of the engine -- or, ``stock``, of this package's
    autograd operator through the stock layers, ``torch.autograd.grad`` and the model's own output: ``{quantity: error}``,
    and the engine."""
    op, model, (x, t), lossf, _ = _engine(family, batch, hessian, prep)
    assert isinstance(op, PlainStackEngine)
    v = torch.randn(op.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(8))
    p64, out64, loss64, _ = float64_twin(STEPS[family][0], batch, op, prep, train=True)
    want, want_grad = product64(p64, out64, loss64, v, hessian), grad64(loss64, p64)
    if stock:
        params = [p for p in model.parameters() if p.requires_grad]
        out = model(x)
        loss = lossf(out, t)
        got = (curvature.HessianOperator(loss, params) if hessian else curvature.GGNOperator(loss, out, params))(v)
        grad = torch.cat([g.reshape(-1) for g in torch.autograd.grad(loss, params, retain_graph=True)])
        logits, lossv = out.detach(), float(loss.detach())
    else:
        got, grad, logits, lossv = op(v).clone(), op.gradient().clone(), op.logits, float(op.loss_buf)
    l64 = float(loss64.detach())
    return {"hessian" if hessian else "ggn": rel(got, want), "grad": rel(grad, want_grad),
            "logits": rel(logits, out64.detach()), "loss": abs(lossv - l64) / abs(l64)}, op


def _check_float64(family, batch, hessian, prep):
    errs, op = measure(family, batch, hessian, prep)
    print(f"{family}-b{batch}-{'hessian' if hessian else 'ggn'}-{getattr(prep, '__name__', None)}: "
          + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    for k, e in errs.items():
        within(e, BOUND[k], note=k)
    return op


def _check_fixture(op, family, batch, hessian, x, cpu_params):
    ref = RefTrace("convbn_train", f"{family}/b{batch}")
    ref.check_inputs(cpu_params, x.cpu())
    kind = "hessian" if hessian else "ggn"
    rp = RefTrace("convbn_train", f"{family}/b{batch}/{kind}")
    v = rp.probe().to(DEV)
    got = op(v).clone()
    for _ in range(3):
        assert torch.equal(op(v), got)  # bitwise repeatable over 4 calls
    u = torch.randn(op.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    gu = op(u).clone()
    a, b = float(u.double() @ got.double()), float(v.double() @ gu.double())
    within(abs(a - b), 1e-5 * abs(a), strict=False)  # symmetric operator
    print(f"  product vs the reference's float64 {rp.vec_err64('', got):.2e}, fp32 {rp.vec_err('', got):.2e} "
          f"(its own fp32 error {rp.own_err(''):.2e})")
    within(rp.vec_err64("", got), BOUND[kind])
    within(rp.vec_err("", got), rp.envelope("", BOUND[kind]))
    grad = op.gradient().clone()
    within(ref.vec_err64("grad", grad), BOUND["grad"])
    within(ref.vec_err("grad", grad), ref.envelope("grad", BOUND["grad"]))
    within(rel(op.logits.cpu(), torch.from_numpy(ref.array("logits_f64"))), BOUND["logits"])
    own = rel(torch.from_numpy(ref.array("logits")), torch.from_numpy(ref.array("logits_f64")))
    within(rel(op.logits.cpu(), torch.from_numpy(ref.array("logits"))), BOUND["logits"] + 3 * own)
    l64 = ref.scalar("loss_f64")
    within(abs(float(op.loss_buf) - l64), BOUND["loss"] * abs(l64), strict=False)
    within(abs(float(op.loss_buf) - ref.scalar("loss")), BOUND["loss"] * abs(l64) + 3 * abs(ref.scalar("loss") - l64),
           strict=False)
    assert torch.equal(op(v), got)  # (the products are untouched by the first-order sweep)


@pytest.mark.parametrize("batch", [2, 5])
@pytest.mark.parametrize("hessian", [False, True], ids=["ggn", "hessian"])
def test_train_mode_convbn_small_is_a_plain_stack_engine_and_matches_float64_and_the_reference(batch, hessian):
    """After ``model.train()`` the operator of prepared ``convbn_small`` IS a ``PlainStackEngine`` with batch statistics in
    its sweeps and an own forward pass (on the parent commit it is the autograd operator, "the model must be in eval
    mode": this is the assertion that fails there)."""
    op, model, (x, t), lossf, cpu_params = _engine("small", batch, hessian)
    assert isinstance(op, PlainStackEngine) and op.hessian == hessian
    assert op.train_bn and op.train_own and all(u.train for u in op.units if u.bn is not None)
    assert [u.pool for u in op.units] == [(3, 3, 2, 2, 0, 0), None, (2, 2, 2, 2, 0, 0), None]
    assert [u.train for u in op.units] == [True, True, True, False] and op.n == N_SMALL and not op.classifier
    assert not any(u.defer or u.split for u in op.units if u.train)
    _check_fixture(op, "small", batch, hessian, x, cpu_params)
    _check_float64("small", batch, hessian, None)


@pytest.mark.parametrize("batch", [2, 5])
def test_train_mode_convbn_fc_small_runs_the_tail_behind_pooled_train_units(batch):
    op, model, (x, t), lossf, cpu_params = _engine("fc", batch)
    assert isinstance(op, PlainStackEngine) and not op.hessian and op.train_bn and op.train_own
    assert [u.pool for u in op.units] == [(3, 3, 2, 2, 0, 0), (2, 2, 2, 2, 0, 0)] and op.n == N_FC
    assert all(u.train and u.relu for u in op.units) and len(op.classifier) == 2
    _check_fixture(op, "fc", batch, False, x, cpu_params)
    _check_float64("fc", batch, False, None)


def test_hessian_products_through_the_tail_stay_refused_in_train_mode():
    op, *_ = _engine("fc", 2, hessian=True)
    assert type(op) is curvature.HessianOperator


def test_launches_per_ggn_product(monkeypatch):
    """One GGN product of train-mode ``convbn_small`` through a proxy around the library.  A pooled train unit: the
    tangent convolution (with the sums in its epilogue, or one reduction launch behind it), ONE
    ``hf_pool_bn_act_tangent_train_nhwc``; ONE ``hf_pool_bn_act_adjoint_reduce_nhwc``, ONE ``hf_chan_affine_train``, the
    convolution's gradients -- 5 or 6, as an unpooled train unit; the bias unit 4 as before.  None of the eval-mode pooled
    launches, none of the stem's max-pool launches."""
    names = record_launches(monkeypatch)
    op, *_ = _engine("small", 2)
    assert isinstance(op, PlainStackEngine) and op.train_bn and names
    v = torch.randn(op.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(6))
    del names[:]
    op.local(v)
    torch.cuda.synchronize()
    got = list(names)
    once = {"hf_pool_ce_head", "hf_pack_ex", "hf_unpack_tangent_ex", "hf_unpack_weights"}
    assert got.count("hf_pool_ce_head") == 1 and got.count("hf_pack_ex") == 1 and "hf_bn_sums_multi" not in got, got
    per_unit = [n for n in got if n not in once]
    bn_units = [u for u in op.units if u.train]
    epilogue = sum(bool(u.tsum) for u in bn_units)
    assert [u.tsum for u in op.units] == [False, True, True, False]  # (the im2col'd first unit has no epilogue form)
    assert len(per_unit) == 6 * len(bn_units) - epilogue + 4, got
    assert got.count(T_TRAIN) == 2 and got.count(A_REDUCE) == 2, got
    for eval_name in ("hf_pool_bn_act_tangent_nhwc", "hf_pool_bn_act_adjoint_nhwc", "hf_pool_act_tangent_nhwc",
                      "hf_pool_act_adjoint_nhwc", "hf_maxpool_tangent_nhwc", "hf_maxpool_adjoint_nhwc"):
        assert eval_name not in got, got
    # the sequence: tangent sweep in layer order (the first unit's sums by a reduction launch), head, adjoint in reverse
    order = [n for n in got if n.startswith(("hf_pool_", "hf_chan_affine", "hf_bn_adjoint"))]
    assert order[:6] == ["hf_chan_affine_bwd_ex", T_TRAIN, "hf_chan_affine_train", T_TRAIN, "hf_chan_affine_ex",
                         "hf_pool_ce_head"], order
    assert order[6:] == ["hf_chan_affine_bwd_ex", A_REDUCE, "hf_chan_affine_train", "hf_chan_affine_bwd_ex",
                         "hf_chan_affine_train", A_REDUCE, "hf_chan_affine_train"], order


@pytest.mark.parametrize("hessian", [False, True], ids=["ggn", "hessian"])
@pytest.mark.parametrize("prep", [_one_eval, _one_train, _one_train_first, _freeze_scales, _freeze_first_unit],
                         ids=lambda f: f.__name__.strip("_"))
def test_mixed_modes_and_frozen_parameters(prep, hessian):
    """One BatchNorm in eval mode inside a train-mode model, one in train mode inside an eval-mode model (the pooled unit
    without a ReLU; the im2col'd first unit), every scale frozen, the first unit frozen (dead for both sweeps; its forward
    pass still takes batch statistics): products, gradient, logits and loss against float64, the frozen tensors untouched."""
    assert ("small", 2, hessian, prep) in MIXED
    op, model, (x, t), lossf, _ = _engine("small", 2, hessian, prep)
    assert isinstance(op, PlainStackEngine) and op.train_bn and op.train_own
    want_train = {_one_eval: [True, False, True, False], _one_train: [False, False, True, False],
                  _one_train_first: [True, False, False, False]}.get(prep, [True, True, True, False])
    assert [u.train for u in op.units] == want_train
    if prep is _freeze_first_unit:
        assert op.dead_units == 1 and op.n == N_SMALL - (8 * 27 + 16)
    if prep is _freeze_scales:
        assert op.n == N_SMALL - 28 and all(u.pg is None for u in op.units)
    frozen = [p for p in model.parameters() if not p.requires_grad]
    before = [p.detach().clone() for p in frozen]
    v = torch.randn(op.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(8))
    got = op(v).clone()
    assert torch.equal(op(v), got)
    op.gradient()
    assert all(torch.equal(a, b.detach()) and b.grad is None for a, b in zip(before, frozen))
    _check_float64("small", 2, hessian, prep)


def _run_steps(family, session):
    make, batch = STEPS[family]
    fixture = ("convbn_train", f"{family}/steps")
    seeds = [int(s) for s in RefTrace(*fixture).array("seeds")]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return run_steps(make, seeds, batch, fixture, train=True, session=session, graph_matvec=True)


@pytest.mark.parametrize("family", sorted(STEPS))
def test_three_default_steps_through_the_session_match_the_reference_trace_and_the_autograd_path(family):
    """``HessianFree(graph_matvec=True).step()`` in train mode runs on the persistent session (own forward pass with batch
    statistics, running statistics moved per forward evaluation); the three-step trace against the real reference's at
    ``compare_trace``'s defaults, and against a twin on this package's autograd path (``_session_off``): same discrete
    trace, the running statistics and ``num_batches_tracked`` of every BatchNorm after the steps."""
    a, fa, ma, ref = _run_steps(family, session=True)
    assert a._session is not None and a._session.steps == 3
    eng = a._session.engine
    assert isinstance(eng, PlainStackEngine) and eng.train_bn and eng.train_own
    compare_trace(a.state, fa, ref)
    b, fb, mb, _ = _run_steps(family, session=False)
    assert b._session is None
    compare_trace(b.state, fb, ref)
    # the running statistics move on both paths, once per forward evaluation (the session evaluates the points the
    # reference evaluates; its trial values are cached per step, so the two counts need not be equal) and stay finite:
    # what the train-mode ResNet test of test_session_gpu.py asks.  The movement itself is held to the stock layers'
    # in test_own_forward_moves_the_running_statistics_as_the_stock_layers_do
    for x, y in zip(_bns(ma), _bns(mb)):
        print(f"  num_batches_tracked session {int(x.num_batches_tracked)} autograd path {int(y.num_batches_tracked)}, "
              f"running_mean {rel(x.running_mean, y.running_mean):.1e} running_var {rel(x.running_var, y.running_var):.1e}")
        for m in (x, y):
            assert int(m.num_batches_tracked) > 3 and float(m.running_mean.abs().max()) > 0
            assert bool(torch.isfinite(m.running_var).all()) and float(m.running_var.min()) > 0


@pytest.mark.parametrize("family", sorted(STEPS))
def test_own_forward_moves_the_running_statistics_as_the_stock_layers_do(family):
    """One ``forward_own(update_running=True)`` against one forward pass of the stock train-mode layers from the same
    state: ``running_mean`` 1e-6, ``running_var`` 5e-6 (the bounds of the residual kind's one-pass statistics,
    test_engine_gpu.py), ``num_batches_tracked`` + 1; ``update_running=False`` leaves all three alone."""
    op, model, (x, t), lossf, _ = _engine(family, 5)
    assert isinstance(op, PlainStackEngine) and op.train_own
    bns = _bns(model)
    state = lambda: [(m.running_mean.clone(), m.running_var.clone(), m.num_batches_tracked.clone()) for m in bns]  # noqa: E731
    saved = state()
    with torch.no_grad():
        model(x)
    stock = state()
    for m, (rm, rv, nb) in zip(bns, saved):
        m.running_mean.copy_(rm), m.running_var.copy_(rv), m.num_batches_tracked.copy_(nb)
    op.forward_own(update_running=False)
    assert all(torch.equal(a, b) for now, was in zip(state(), saved) for a, b in zip(now, was))
    op.forward_own(update_running=True)
    for m, (rm, rv, nb), (_, _, nb0) in zip(bns, stock, saved):
        within(rel(m.running_mean, rm), 1e-6)
        within(rel(m.running_var, rv), 5e-6)
        assert int(m.num_batches_tracked) == int(nb) == int(nb0) + 1


def test_an_active_dropout_keeps_the_autograd_path_and_is_named():
    C, B, R, D, G = torch.nn.Conv2d, torch.nn.BatchNorm2d, torch.nn.ReLU, torch.nn.Dropout, torch.nn.AdaptiveAvgPool2d
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(1)
    x, t = torch.rand(2, 3, 8, 8, generator=gen).to(DEV), torch.randint(0, 4, (2,), generator=gen).to(DEV)
    build = lambda p: tp.seed_batchnorm(_Net([C(3, 8, 3, 1, 1, bias=False), B(8), R(), D(p), C(8, 4, 1), G(1)])).train()  # noqa: E731
    lossf = torch.nn.CrossEntropyLoss()
    model = build(0.5).to(DEV)
    modelprep.prepare_model(model, channels_last=True)
    declined(model, x, t, lossf, "Dropout(p=0.5) behind conv0 is active")
    # p = 0, or the module in eval mode inside the train-mode model: skipped as before
    for variant in (build(0.0), build(0.5)):
        for m in variant.modules():
            if isinstance(m, D) and m.p > 0:
                m.eval()
        variant = variant.to(DEV)
        modelprep.prepare_model(variant, channels_last=True)
        out = variant(x)
        op = curvature.ggn_operator(lossf(out, t), out, list(variant.parameters()))
        assert isinstance(op, PlainStackEngine) and op.train_bn
        # (what a session compares per step: switching the skipped Dropout on is another network)
        sig = op.layer_signature()
        drop = next(m for m in variant.modules() if isinstance(m, D))
        drop.train()
        assert (op.layer_signature() != sig) == (drop.p > 0)


def test_allcnnc_in_train_mode_names_its_dropout():
    model, (x, t), lossf = tp.allcnnc_cifar100(batch_size=2, device=DEV)
    model.train()
    modelprep.prepare_model(model, channels_last=True)
    out, why = model(x), []
    assert FusedGGNEngine.try_build(lossf(out, t), out, [p for p in model.parameters() if p.requires_grad], why=why) is None
    assert any("Dropout(p=0.2) in front of the first convolution is active" in w for w in why), why


def test_train_mode_under_a_process_group_is_declined():
    model, (x, t), lossf = tp.convbn_small(batch_size=2, device=DEV)
    model.train()
    modelprep.prepare_model(model, channels_last=True)
    out, why = model(x), []
    group = object()  # (the layout only asks whether there is one)
    assert FusedGGNEngine.try_build(lossf(out, t), out, list(model.parameters()), group=group, why=why) is None
    assert any("conv0: train-mode BatchNorm under data parallelism: batch statistics couple the samples of a shard" in w
               for w in why), why


def test_preconditioner_and_diag_ef_on_a_train_mode_engine(monkeypatch):
    """``engine.diag_ef`` stays refused with batch statistics (the samples interact); ``get_preconditioner`` with a
    train-mode session leaves the engine alone and hands the call to the autograd construction, as for a train-mode
    ResNet, and returns what that answers (the reference's own per-sample loop feeds unbatched samples, which
    ``BatchNorm2d`` refuses: not this package's to widen -- the construction is stood in for here)."""
    from pytorchhessianfree_amd import optimizer_session as hfopt

    op, model, (x, t), lossf, _ = _engine("small", 2)
    assert isinstance(op, PlainStackEngine) and op.train_bn
    with pytest.raises(RuntimeError, match="eval-mode BatchNorm"):
        op.diag_ef("mean")
    opt = hf.HessianFree(model.parameters(), graph_matvec=True)

    def forward():
        out = model(x)
        return lossf(out, t), out

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        opt.step(forward)
        assert opt._session is not None and opt._session.engine.train_bn
        calls, answer = [], object()
        monkeypatch.setattr(hfopt, "diag_EF_preconditioner", lambda *a, **k: calls.append(k) or answer)
        monkeypatch.setattr(type(opt._session.engine), "diag_ef",
                            lambda *a, **k: pytest.fail("engine.diag_ef on a train-mode engine"))
        M = opt.get_preconditioner(model, lossf, x, t, "mean", use_backpack=False)
    assert M is answer and len(calls) == 1 and calls[0]["use_backpack"] is False
