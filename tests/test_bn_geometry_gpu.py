"""GPU: BatchNorm units of ``PlainStackEngine`` (``Conv2d(bias=False) BatchNorm2d [ReLU] [MaxPool2d]``; pooled ones on
``hf_pool_bn_act_*_nhwc``, ``hf_pool_bn_act_tangent_train_nhwc`` and ``hf_pool_bn_act_adjoint_reduce_nhwc``), in eval and in
train mode, on the cases of ``geometry_nets.BN_STACKS`` against the float64 reference of the STOCK model, on the engine's own
ReLU decisions and pool positions (the units' masks, then the tail's; ``u.pidx``; replayed under ``geometry_nets.MAX_FLIPS``
/ ``MARGIN``), tensor by tensor: ``max|got_T - want_T| / max|want_T|`` for every parameter tensor ``T``, exactly zero where
the reference is exactly zero (``geometry_nets.per_tensor_errors``).

What the cases reach that ``convbn_small`` / ``convbn_fc_small`` (square 12x12 inputs, square windows, equal strides, pool
padding 0, whole-vector max-norm) do not stands in ``geometry_nets.BN_GEOMETRY``: ``h != w``, ``kh != kw``, ``sh != sw``,
``ph != pw`` behind a BatchNorm, a padded pool window behind a BatchNorm without ReLU, dead kernel taps, 60 and 40 row blocks
in the pooled adjoint, one-row / one-column / 1x1 maps, batch statistics over 15 rows, a first unit that is not im2col'd,
pooled BatchNorm units in front of a classifier tail.

Every case is prepared with ``modelprep.prepare_model(channels_last=True)`` and built through ``curvature.ggn_operator`` /
``hessian_operator``, once per (case, mode, curvature); a decline fails with the reasons.

Bounds (``BOUND_BN``).  Not taken from the engine: per quantity 3x the worst distance of STOCK fp32 autograd on the GPU
(``geometry_nets.stock_fp32_errors``) from the same float64 reference in the same per-tensor measure over the BatchNorm-stack
cases, rounded up to one significant digit -- the policy of ``test_engine_geometry_gpu.BOUND`` and
``test_tail_geometry_gpu.BOUND_TAIL``, kept apart from them.  The running statistics: 3x the stock fp32 train-mode forward
pass's distance from the same float64 pass.  Both series, stock fp32 and the engine's own figures per case, quantity and
tensor, stand in ``profiles/r31_bn_geometry.jsonl``."""

import copy
import hashlib

import geometry_nets as gn
import pytest
import torch
from tol import within
from torch import nn

import pytorchhessianfree_amd as hf
from pytorchhessianfree_amd import curvature, modelprep
from pytorchhessianfree_amd.engine import PlainStackEngine
from pytorchhessianfree_amd.session import EngineSession

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEEDS = (11, 12)  # (of the vectors the products are taken of)

# quantity: 3 x (worst figure of the series "stock_fp32" in profiles/r31_bn_geometry.jsonl over the cases), rounded up to
# one significant digit -- ``scripts/engine_geometry_errors.py --cases bn`` writes that file and prints these lines
BOUND_BN = {
    "logits": 2e-6,          # 3.44e-7 (bn_wide_rows)
    "loss": 2e-7,            # 5.12e-8 (bn_row_map)
    "gradient": 2e-6,        # 3.85e-7 (bn_wide_rows)
    "ggn": 2e-6,             # 4.47e-7 (bn_tail_rect)
    "hessian": 2e-6,         # 5.48e-7 (bn_wide_rows)
    "diag_ef": 2e-6,         # 4.08e-7 (bn_rect_pooled)
    "logits_train": 2e-6,    # 4.32e-7 (bn_wide_rows)
    "loss_train": 2e-7,      # 4.18e-8 (bn_tail_rect)
    "gradient_train": 4e-6,  # 1.13e-6 (bn_wide_rows)
    "ggn_train": 5e-6,       # 1.57e-6 (bn_wide_rows)
    "hessian_train": 6e-6,   # 1.95e-6 (bn_wide_rows)
    "running": 4e-7,         # 1.19e-7 (bn_wide_rows)
}
TAIL_REFUSAL = "Hessian products through a classifier tail are not covered"


def _modes(case):
    return [False, True] if case in gn.BN_TRAIN_CASES else [False]


CASE_MODES = [(case, train) for case in gn.BN_CASES for train in _modes(case)]
HESSIAN_MODES = [(case, train) for case, train in CASE_MODES if case in gn.BN_HESSIAN_CASES]
MODE_IDS = lambda v: ("train" if v else "eval") if isinstance(v, bool) else str(v)  # noqa: E731


def _q(quantity, train):
    return quantity + ("_train" if train else "")


def _bns(model):
    return [m for m in model.modules() if isinstance(m, nn.BatchNorm2d)]


# ---- mixed modes and frozen structure (on bn_rect_pooled): prep, train mode, entries left, dead units ----------------
def _one_eval(model):
    _bns(model)[1].eval()  # (the pooled unit's without a ReLU, inside a train-mode model)


def _freeze_scale_and_shift(model):
    _bns(model)[0].weight.requires_grad_(False)  # (the nullable gw of the pooled unit with a ReLU ...)
    _bns(model)[1].bias.requires_grad_(False)    # (... and the nullable gb of the pooled unit without one)


def _freeze_first_unit(model):
    for m in list(model.net)[:2]:  # the first convolution and its BatchNorm
        for p in m.parameters():
            p.requires_grad_(False)


MIXED_CASE, N_RECT = "bn_rect_pooled", 2852
MIXED = {
    "one_eval": (_one_eval, True, N_RECT, 0),
    "frozen_scale_and_shift_eval": (_freeze_scale_and_shift, False, N_RECT - 8 - 12, 0),
    "frozen_scale_and_shift_train": (_freeze_scale_and_shift, True, N_RECT - 8 - 12, 0),
    "frozen_first_unit_eval": (_freeze_first_unit, False, N_RECT - (8 * 9 + 16), 1),
    "frozen_first_unit_train": (_freeze_first_unit, True, N_RECT - (8 * 9 + 16), 1),
}


def _build(case, train=False, hessian=False, prep=None):
    """The engine of ``case`` through the package's entry point: ``(op, stock model on the CPU, batches, gpu model)``.
    ``prep(stock)`` after the mode is set (the reference copies the same modes and frozen flags)."""
    stock, batches = gn.make(case, train)
    if prep is not None:
        prep(stock)
    x, t = batches[0]
    model = copy.deepcopy(stock).to(DEV)
    modelprep.prepare_model(model, channels_last=True)
    params = [p for p in model.parameters() if p.requires_grad]
    out = model(x.to(DEV))
    why = []
    make = curvature.hessian_operator if hessian else curvature.ggn_operator
    op = make(nn.functional.cross_entropy(out, t.to(DEV)), out, params, why=why)
    assert type(op) is PlainStackEngine, (type(op).__name__, why)
    any_train = any(m.training for m in _bns(stock))
    assert op.hessian == hessian and op.train_bn == any_train and (op.train_own or not any_train)
    assert bool(op.classifier) == (case == "bn_tail_rect")
    return op, stock, batches, model


_ENGINES, _REFS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_engines():
    """The engines and references the tests of this file share live as long as the file's tests run, no longer."""
    yield
    _ENGINES.clear()
    _REFS.clear()
    torch.cuda.empty_cache()


def _engine(case, train=False, hessian=False):
    key = (case, train, hessian)
    if key not in _ENGINES:  # (built once per case, mode and curvature, shared by the tests, left at its own forward pass)
        _ENGINES[key] = _build(case, train, hessian)
    return _ENGINES[key]


def _decisions(op):
    """The engine's ReLU masks in call order (the units' at full resolution, then the tail's) and its pool positions
    (``[n, c, oh, ow]``, int64: ``geometry_nets.pool_positions``' form)."""
    masks = [(u.y > 0).cpu() for u in op.units if u.relu] + [(u.y > 0).cpu() for u in op.classifier if u.act == 1]
    pools = [u.pidx.permute(0, 3, 1, 2).long().cpu().contiguous() for u in op.units if u.pool is not None]
    return masks, pools


def _reference(key, stock, batch, op):
    """The float64 reference on the decisions ``op`` took (computed once per set of decisions)."""
    masks, pools = _decisions(op)
    digest = hashlib.sha1(b"".join(m.contiguous().numpy().tobytes() for m in masks + pools)).hexdigest()
    key = (key, digest)
    if key not in _REFS:
        _REFS[key] = gn.Reference(stock, *batch, masks=masks, pools=pools)
    return _REFS[key]


def _assert(quantity, errs):
    worst = max(errs, key=errs.get)
    print(f"[bn geometry] {quantity}: worst {errs[worst]:.2e} at {worst} (bound {BOUND_BN[quantity]})")
    for name, e in errs.items():
        within(e, BOUND_BN[quantity], note=(quantity, name, errs))


def _logits_error(op, ref):
    return float((op.logits.cpu().double() - ref.logits).abs().max() / ref.logits.abs().max())


# ---- what each test measures (also what scripts/engine_geometry_errors.py records) -----------------------------------
def forward_errors(case, train=False):
    """Logits and loss behind the engine's own forward pass; train mode: that pass moves the running statistics, from
    the state the stock model was made in, as ONE train-mode pass of the float64 model moves them."""
    op, stock, batches, model = _engine(case, train)
    if train:
        for mine, fresh in zip(_bns(model), _bns(stock)):
            for k in ("running_mean", "running_var", "num_batches_tracked"):
                getattr(mine, k).copy_(getattr(fresh, k))
    op.forward_own(update_running=True)
    ref = _reference((case, train, 0), stock, batches[0], op)
    res = {_q("logits", train): {"logits": _logits_error(op, ref)},
           _q("loss", train): {"loss": gn.scalar_error(op.loss_buf, ref.loss())}}
    if train:
        res["running"] = gn.running_errors(model, ref)  # (num_batches_tracked: equal, asserted there)
        assert len(res["running"]) == 2 * len(_bns(stock)) > 0
    return res


def gradient_errors(case, train=False):
    op, stock, batches, _ = _engine(case, train)
    ref = _reference((case, train, 0), stock, batches[0], op)
    return {_q("gradient", train): gn.per_tensor_errors(op.gradient(), ref.gradient(), gn.named_sizes(stock))}


def _product_errors(op, stock, ref):
    sizes = gn.named_sizes(stock)
    assert op.n == sum(k for _, k in sizes)
    worst, got = {}, []
    for seed in SEEDS:
        v = gn.probe(op.n, seed, DEV)
        g = op(v).clone()
        for _ in range(3):
            assert torch.equal(op(v), g)  # bitwise repeatable: four calls
        want = ref.hessian(v) if op.hessian else ref.ggn(v)
        for name, e in gn.per_tensor_errors(g, want, sizes).items():
            worst[name] = max(worst.get(name, 0.0), e)
        got.append((v, g))
    # a symmetric operator: <u, G v> == <v, G u>
    (u, gu), (v, gv) = got
    a, b = float(u.double() @ gv.double()), float(v.double() @ gu.double())
    within(abs(a - b), 1e-5 * abs(a), strict=False)
    return worst


def product_errors(case, hessian=False, train=False):
    op, stock, batches, _ = _engine(case, train, hessian)
    ref = _reference((case, train, 0), stock, batches[0], op)
    return {_q("hessian" if hessian else "ggn", train): _product_errors(op, stock, ref)}


def diag_errors(case):
    """Diagonal empirical Fisher (eval mode) at the first batch; then a second batch through ``set_batch`` and the
    engine's OWN forward pass (not the recorded one): loss, logits, gradient, diagonal again."""
    op, stock, batches, _ = _build(case)
    sizes = gn.named_sizes(stock)
    res = {"diag_ef": {}, "gradient": {}, "loss": {}, "logits": {}}
    for which, (x, t) in enumerate(batches):
        if which:
            op.set_batch(x.to(DEV), t.to(DEV))
            op.forward_own()
        ref = _reference((case, False, which), stock, (x, t), op)
        d = op.diag_ef("mean").clone()
        assert torch.equal(op.diag_ef("mean"), d)  # repeatable
        for name, e in gn.per_tensor_errors(d, ref.diag_ef(), sizes).items():
            res["diag_ef"][f"batch{which}/{name}"] = e
        if which:
            for name, e in gn.per_tensor_errors(op.gradient(), ref.gradient(), sizes).items():
                res["gradient"][f"batch{which}/{name}"] = e
            res["loss"]["batch1/loss"] = gn.scalar_error(op.loss_buf, ref.loss())
            res["logits"]["batch1/logits"] = _logits_error(op, ref)
    res["batched"] = bool(op._diag_batched)
    return res


def mixed_errors(name, hessian=False):
    """``bn_rect_pooled`` under ``MIXED[name]``: ``{quantity: errors}`` of product, gradient, logits and loss, with the
    structure asserted and the frozen tensors untouched."""
    prep, train, n, dead = MIXED[name]
    op, stock, batches, model = _build(MIXED_CASE, train, hessian, prep)
    sizes = gn.named_sizes(stock)
    assert op.n == n == sum(k for _, k in sizes) and op.dead_units == dead
    if prep is _one_eval:
        assert [u.train for u in op.units] == [True, False, True, False]
    else:
        assert op.frozen_any and [u.train for u in op.units] == [train, train, train, False]
    if prep is _freeze_scale_and_shift:
        assert op.units[0].pg is None and op.units[0].pb is not None
        assert op.units[1].pb is None and op.units[1].pg is not None
    frozen = [p for p in model.parameters() if not p.requires_grad]
    before = [p.detach().clone() for p in frozen]
    assert bool(frozen) == (prep is not _one_eval)
    ref = _reference((MIXED_CASE, name), stock, batches[0], op)
    res = {_q("hessian" if hessian else "ggn", train): _product_errors(op, stock, ref),
           _q("gradient", train): gn.per_tensor_errors(op.gradient(), ref.gradient(), sizes)}
    op.forward_own(update_running=False)
    res[_q("logits", train)] = {"logits": _logits_error(op, ref)}
    res[_q("loss", train)] = {"loss": gn.scalar_error(op.loss_buf, ref.loss())}
    assert all(torch.equal(a, b.detach()) and b.grad is None for a, b in zip(before, frozen))
    return res


# ---- the tests -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case, train", CASE_MODES, ids=MODE_IDS)
def test_engine_layout_is_the_bn_cases_table(case, train):
    """Per unit: maps, pool ``(kh, kw, sh, sw, ph, pw)``, pooled map, row blocks, live taps, im2col and mode are what
    ``geometry_nets.BN_GEOMETRY`` writes out.  How the unit's sums are scheduled is printed, not asserted."""
    op, stock, batches, model = _engine(case, train)
    lit = gn.BN_GEOMETRY[case]
    names = {m: n for n, m in model.named_modules()}
    for u in op.units:
        print(f"[bn geometry] {case} {'train' if train else 'eval'} {u.name}: " + ", ".join(
            f"{k} {getattr(u, k, None)}" for k in ("epi", "tsum", "defer", "split")))
    first = lit["convs"][0][0]  # (an im2col'd unit reads no taps: its dead ones are zero columns of the im2col)
    got = [(names[u.conv], tuple(u.x.shape[2:]), tuple(u.a.shape[2:]), 0 if u.im2col else u.live, u.rb, u.pool,
            None if u.pool is None else tuple(u.yp.shape[2:])) for u in op.units]
    assert got == [(name, hw, ohw, 0 if (lit["im2col"] and name == first) else mask, rb, pool, pooled)
                   for name, hw, ohw, mask, rb, pool, pooled in lit["convs"]]
    assert [u.im2col for u in op.units] == [lit["im2col"]] + [False] * (len(op.units) - 1)
    assert [u.train for u in op.units] == [train and u.bn is not None for u in op.units]
    assert [u.bn is not None for u in op.units] == [isinstance(stock.net[int(name.split(".")[1]) + 1], nn.BatchNorm2d)
                                                    for name, *_ in lit["convs"]]
    assert op.n == lit["n"] and op.dead_units == 0
    for u in op.units:
        if u.pool is not None:  # (what ``_pool_dims`` hands the pooled launches)
            n, h, w, oh, ow, c = op._pool_dims(u)
            assert (h, w) == tuple(u.a.shape[2:]) and (oh, ow) == tuple(u.yp.shape[2:]) and c == u.conv.out_channels
            assert n == batches[0][0].shape[0] and tuple(u.pidx.shape) == (n, oh, ow, c)


@pytest.mark.parametrize("case, train", CASE_MODES, ids=MODE_IDS)
def test_forward_pass_matches_float64(case, train):
    errs = forward_errors(case, train)
    for quantity, e in errs.items():
        _assert(quantity, e)


@pytest.mark.parametrize("case, train", CASE_MODES, ids=MODE_IDS)
def test_gradient_matches_float64_per_tensor(case, train):
    quantity = _q("gradient", train)
    _assert(quantity, gradient_errors(case, train)[quantity])


@pytest.mark.parametrize("case, train", CASE_MODES, ids=MODE_IDS)
def test_ggn_product_matches_float64_per_tensor(case, train):
    quantity = _q("ggn", train)
    _assert(quantity, product_errors(case, train=train)[quantity])


@pytest.mark.parametrize("case, train", HESSIAN_MODES, ids=MODE_IDS)
def test_hessian_product_matches_float64_per_tensor(case, train):
    quantity = _q("hessian", train)
    _assert(quantity, product_errors(case, hessian=True, train=train)[quantity])


@pytest.mark.parametrize("train", [False, True], ids=MODE_IDS)
def test_hessian_products_through_the_tail_stay_refused(train):
    stock, batches = gn.make("bn_tail_rect", train)
    x, t = batches[0]
    model = copy.deepcopy(stock).to(DEV)
    modelprep.prepare_model(model, channels_last=True)
    out, why = model(x.to(DEV)), []
    op = curvature.hessian_operator(nn.functional.cross_entropy(out, t.to(DEV)), out, list(model.parameters()), why=why)
    assert type(op) is curvature.HessianOperator, type(op).__name__
    assert any("PlainStackEngine" in line and TAIL_REFUSAL in line for line in why), why


@pytest.mark.parametrize("batched", [False, True], ids=["per_sample", "batched"])
@pytest.mark.parametrize("case", gn.BN_CASES)
def test_diagonal_fisher_and_a_second_batch_match_float64_per_tensor(case, batched, monkeypatch):
    monkeypatch.setenv("HF_DIAG_EF_BATCHED", "1" if batched else "0")
    errs = diag_errors(case)
    assert errs.pop("batched") == batched
    for quantity in ("diag_ef", "gradient", "loss", "logits"):
        _assert(quantity, errs[quantity])


@pytest.mark.parametrize("hessian", [False, True], ids=["ggn", "hessian"])
@pytest.mark.parametrize("name", sorted(MIXED))
def test_mixed_modes_and_frozen_parameters_match_float64_per_tensor(name, hessian):
    """``bn_rect_pooled`` with (a) the pooled unit without a ReLU in eval mode inside a train-mode model, (b) the scale of
    the first unit and the shift of the second frozen (the nullable ``gw`` / ``gb`` of the pooled launches), (c) the
    first unit frozen (dead for both sweeps; in train mode its forward pass still takes batch statistics)."""
    for quantity, errs in mixed_errors(name, hessian).items():
        _assert(quantity, errs)


def _session(case, train):
    stock, batches = gn.make(case, train)
    x, t = batches[0]
    model = copy.deepcopy(stock).to(DEV)
    modelprep.prepare_model(model, channels_last=True)
    opt = hf.HessianFree(model.parameters(), graph_matvec=True)
    opt._ensure_arena()
    out = model(x.to(DEV))
    why = []
    sess = EngineSession.try_create(nn.functional.cross_entropy(out, t.to(DEV)), out, opt._params_list, why=why)
    assert sess is not None and type(sess.engine) is PlainStackEngine and sess.engine.train_bn == train, why
    return sess, opt, model


@pytest.mark.parametrize("case, train", gn.BN_CAPTURED_CASES, ids=MODE_IDS)
def test_captured_replay_is_bitwise_the_eager_product(case, train):
    """The product as the session replays it (one hipGraph over the engine's static buffers) against the eager launches."""
    sess, opt, model = _session(case, train)
    eng = sess.engine
    assert [u.rb for u in eng.units] == [rb for *_, rb, _, _ in gn.BN_GEOMETRY[case]["convs"]]
    for seed in SEEDS:
        v = gn.probe(eng.n, seed, DEV)
        eager = eng.local(v).clone()
        assert torch.equal(sess.local(v), eager)
        assert torch.equal(sess(v), eager)
        assert torch.equal(eng.local(v), eager)
    assert bool(eager.abs().max() > 0)
