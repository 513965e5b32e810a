"""GPU: the curvature engines (``FusedGGNEngine``, ``PlainStackEngine``) on the non-square and degenerate geometries of
``geometry_nets.py`` against the float64 reference of the STOCK model, on the engine's own ReLU decisions (replayed under
``geometry_nets.MAX_FLIPS`` / ``MARGIN``), tensor by tensor: ``max|got_T - want_T| / max|want_T|`` for every parameter
tensor ``T``, exactly zero where the reference is exactly zero (``geometry_nets.per_tensor_errors``).

Every case is prepared with ``modelprep.prepare_model(channels_last=True)`` and built through ``curvature.ggn_operator`` /
``curvature.hessian_operator``; a decline (the engine's first-use check included: it swaps in the autograd operator) fails
with the reasons.  One test per case and quantity: forward pass, gradient, GGN product, Hessian product, train-mode
BatchNorm, diagonal empirical Fisher (per-sample and batched launches; then a second batch through ``set_batch``),
compact layout, captured replay.

Bounds (``BOUND``).  Not taken from the engine: per quantity 3x the worst distance of STOCK fp32 autograd on the GPU -- the
unprepared model, ``GGNOperator``, ``HessianOperator``, per-sample gradients; ``geometry_nets.stock_fp32_errors`` -- from
the same float64 reference in the same per-tensor measure over all cases, rounded up to one significant digit (the
project's 3x policy; the yardstick of the Bottleneck test).  Both series, stock fp32 and the engine's own figures per
case, quantity and tensor, stand in ``profiles/r26_engine_geometry.jsonl``."""

import copy
import hashlib

import geometry_nets as gn
import pack_refs as pr
import pytest
import torch
from tol import within
from torch import nn

import pytorchhessianfree_amd as hf
from pytorchhessianfree_amd import curvature, modelprep
from pytorchhessianfree_amd.engine import FusedGGNEngine, PlainStackEngine
from pytorchhessianfree_amd.session import EngineSession

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEEDS = (11, 12)  # (of the vectors the products are taken of)

# quantity: 3 x (worst figure of the series "stock_fp32" in profiles/r26_engine_geometry.jsonl over the cases), rounded up
# to one significant digit -- ``scripts/engine_geometry_errors.py`` writes that file and prints these lines
BOUND = {
    "logits": 5e-7,         # 1.50e-7 (wide_rows)
    "loss": 5e-7,           # 1.42e-7 (plain_quads_in)
    "gradient": 2e-6,       # 5.38e-7 (nonsquare_odd)
    "ggn": 4e-6,            # 1.06e-6 (col_map)
    "hessian": 2e-6,        # 5.64e-7 (asym_stride)
    "ggn_train": 2e-5,      # 3.64e-6 (wide_rows)
    "hessian_train": 7e-6,  # 2.22e-6 (wide_rows)
    "diag_ef": 3e-6,        # 7.65e-7 (batch_one)
}


def _kind(case):
    return PlainStackEngine if case in gn.STACKS else FusedGGNEngine


def _build(case, train=False, hessian=False):
    """The engine of ``case`` through the package's entry point: ``(op, stock model on the CPU, batches, gpu model)``."""
    stock, batches = gn.make(case, train)
    x, t = batches[0]
    model = copy.deepcopy(stock).to(DEV)
    modelprep.prepare_model(model, channels_last=True)
    params = [p for p in model.parameters() if p.requires_grad]
    out = model(x.to(DEV))
    why = []
    make = curvature.hessian_operator if hessian else curvature.ggn_operator
    op = make(nn.functional.cross_entropy(out, t.to(DEV)), out, params, why=why)
    assert type(op) is _kind(case), (type(op).__name__, why)
    assert op.hessian == hessian and op.train_bn == train
    return op, stock, batches, model


_ENGINES, _REFS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_engines():
    """The engines and references the tests of this file share live as long as the file's tests run, no longer."""
    yield
    _ENGINES.clear()
    _REFS.clear()
    torch.cuda.empty_cache()


def _ggn_engine(case):
    if case not in _ENGINES:  # (built once per case, shared by the forward / gradient / product tests, left unchanged)
        _ENGINES[case] = _build(case)
    return _ENGINES[case]


def _masks(op):
    return [(u.y > 0).cpu() for u in op.units if u.relu]


def _reference(case, stock, batch, op, train=False, which=0):
    """The float64 reference on the decisions ``op`` took (computed once per set of decisions)."""
    masks = _masks(op)
    digest = hashlib.sha1(b"".join(m.contiguous().numpy().tobytes() for m in masks)).hexdigest()
    key = (case, train, which, digest)
    if key not in _REFS:
        _REFS[key] = gn.Reference(stock, *batch, masks=masks)
    return _REFS[key]


def _assert(quantity, errs):
    worst = max(errs, key=errs.get)
    print(f"[geometry] {quantity}: worst {errs[worst]:.2e} at {worst} (bound {BOUND[quantity]})")
    for name, e in errs.items():
        within(e, BOUND[quantity], note=(quantity, name, errs))


# ---- what each test measures (also what scripts/engine_geometry_errors.py records) -------------------
def forward_errors(case):
    op, stock, batches, _ = _ggn_engine(case)
    op.forward_own()
    ref = _reference(case, stock, batches[0], op)
    logits = float((op.logits.cpu().double() - ref.logits).abs().max() / ref.logits.abs().max())
    return {"logits": {"logits": logits}, "loss": {"loss": gn.scalar_error(op.loss_buf, ref.loss())}}


def gradient_errors(case):
    op, stock, batches, _ = _ggn_engine(case)
    ref = _reference(case, stock, batches[0], op)
    return {"gradient": gn.per_tensor_errors(op.gradient(), ref.gradient(), gn.named_sizes(stock))}


def product_errors(case, hessian=False, train=False):
    op, stock, batches, _ = _build(case, train, hessian) if (hessian or train) else _ggn_engine(case)
    ref = _reference(case, stock, batches[0], op, train)
    sizes = gn.named_sizes(stock)
    assert op.n == sum(k for _, k in sizes)
    worst, got = {}, []
    for seed in SEEDS:
        v = gn.probe(op.n, seed, DEV)
        g = op(v).clone()
        for _ in range(3):
            assert torch.equal(op(v), g)  # bitwise repeatable
        want = ref.hessian(v) if hessian else ref.ggn(v)
        for name, e in gn.per_tensor_errors(g, want, sizes).items():
            worst[name] = max(worst.get(name, 0.0), e)
        got.append((v, g))
    # a symmetric operator: <u, G v> == <v, G u>
    (u, gu), (v, gv) = got
    a, b = float(u.double() @ gv.double()), float(v.double() @ gu.double())
    within(abs(a - b), 1e-5 * abs(a), strict=False)
    return {("hessian" if hessian else "ggn") + ("_train" if train else ""): worst}


def diag_errors(case):
    """Diagonal empirical Fisher at the first batch; then a second batch through ``set_batch`` and the engine's OWN
    forward pass (not the recorded one): loss, gradient, diagonal again."""
    op, stock, batches, _ = _build(case)
    sizes = gn.named_sizes(stock)
    res = {"diag_ef": {}, "gradient": {}, "loss": {}, "logits": {}}
    for which, (x, t) in enumerate(batches):
        if which:
            op.set_batch(x.to(DEV), t.to(DEV))
            op.forward_own()
        ref = _reference(case, stock, (x, t), op, which=which)
        d = op.diag_ef("mean").clone()
        assert torch.equal(op.diag_ef("mean"), d)  # repeatable
        for name, e in gn.per_tensor_errors(d, ref.diag_ef(), sizes).items():
            res["diag_ef"][f"batch{which}/{name}"] = e
        if which:
            for name, e in gn.per_tensor_errors(op.gradient(), ref.gradient(), sizes).items():
                res["gradient"][f"batch{which}/{name}"] = e
            res["loss"]["batch1/loss"] = gn.scalar_error(op.loss_buf, ref.loss())
            res["logits"]["batch1/logits"] = float((op.logits.cpu().double() - ref.logits).abs().max()
                                                   / ref.logits.abs().max())
    res["batched"] = bool(op._diag_batched)
    return res


# ---- the tests -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gn.CASES)
def test_engine_geometry_is_the_float64_cases_table(case):
    """The engine's units see the maps, live-tap masks and row-block counts ``geometry_nets.GEOMETRY`` writes out."""
    op, stock, batches, model = _ggn_engine(case)
    names = {m: n for n, m in model.named_modules()}
    got = {names[u.conv]: (tuple(u.x.shape[2:]), tuple(u.a.shape[2:]), 0 if u.im2col else u.live, u.rb) for u in op.units}
    assert got == {name: (hw, ohw, mask, rb) for name, hw, ohw, mask, rb in gn.GEOMETRY[case]}
    assert op.units[0].im2col == (case != "plain_quads_in")
    last = gn.GEOMETRY[case][-1][2]
    assert op._head_hw == last[0] * last[1]
    if case == "batch_one":  # the head reads the last unit's 1x1 map in place
        assert op._head_hw == 1 and op.feat.data_ptr() == op.tail.y.data_ptr()
    if case == "asym_stride":
        assert op.units[0].cols_pad.shape[2] == 28 and op.units[0].jcols == 27
    if case == "stem7":
        assert op.units[0].jcols == 147


@pytest.mark.parametrize("case", gn.CASES)
def test_forward_pass_matches_float64(case):
    errs = forward_errors(case)
    _assert("logits", errs["logits"])
    _assert("loss", errs["loss"])


@pytest.mark.parametrize("case", gn.CASES)
def test_gradient_matches_float64_per_tensor(case):
    _assert("gradient", gradient_errors(case)["gradient"])


@pytest.mark.parametrize("case", gn.CASES)
def test_ggn_product_matches_float64_per_tensor(case):
    _assert("ggn", product_errors(case)["ggn"])


@pytest.mark.parametrize("case", gn.CASES)
def test_hessian_product_matches_float64_per_tensor(case):
    _assert("hessian", product_errors(case, hessian=True)["hessian"])


@pytest.mark.parametrize("hessian", [False, True], ids=["ggn", "hessian"])
@pytest.mark.parametrize("case", gn.TRAIN_CASES)
def test_train_mode_batchnorm_product_matches_float64_per_tensor(case, hessian):
    quantity = ("hessian" if hessian else "ggn") + "_train"
    _assert(quantity, product_errors(case, hessian=hessian, train=True)[quantity])


@pytest.mark.parametrize("batched", [False, True], ids=["per_sample", "batched"])
@pytest.mark.parametrize("case", gn.CASES)
def test_diagonal_fisher_and_a_second_batch_match_float64_per_tensor(case, batched, monkeypatch):
    monkeypatch.setenv("HF_DIAG_EF_BATCHED", "1" if batched else "0")
    errs = diag_errors(case)
    assert errs.pop("batched") == batched
    for quantity in ("diag_ef", "gradient", "loss", "logits"):
        _assert(quantity, errs[quantity])


def _session(case):
    stock, batches = gn.make(case)
    x, t = batches[0]
    model = copy.deepcopy(stock).to(DEV)
    modelprep.prepare_model(model, channels_last=True)
    opt = hf.HessianFree(model.parameters(), graph_matvec=True)
    opt._ensure_arena()
    out = model(x.to(DEV))
    why = []
    sess = EngineSession.try_create(nn.functional.cross_entropy(out, t.to(DEV)), out, opt._params_list, why=why)
    assert sess is not None and type(sess.engine) is _kind(case), why
    return sess, opt, model


@pytest.mark.parametrize("case", gn.COMPACT_CASES)
def test_compact_product_is_bitwise_the_gathered_full_product(case):
    """``local_compact(gather(v)) == gather(local(v))`` bit for bit, eager and as the session's captured graph;
    ``n_live`` is what the masks of ``geometry_nets.GEOMETRY`` leave."""
    sess, opt, model = _session(case)
    eng, c = sess.engine, sess.compact
    assert c is not None, sess.compact_decline
    mods = dict(model.named_modules())
    dead = sum(mods[name].weight.numel() // 9 * (9 - bin(mask).count("1"))
               for name, _, _, mask, _ in gn.GEOMETRY[case] if mask)
    assert dead > 0 and c.n_live == eng.n - dead
    assert sorted(c.layout["nl"].values()) == sorted(bin(m).count("1") for *_, m, _ in gn.GEOMETRY[case] if m)
    idx = torch.from_numpy(pr.live_index(c.layout["table"])).to(DEV)
    is_dead = torch.ones(eng.n, dtype=torch.bool, device=DEV)
    is_dead[idx] = False
    assert int(is_dead.sum()) == dead
    v = gn.probe(eng.n, SEEDS[0], DEV)
    full = eng.local(v).clone()
    assert not full[is_dead].any() and bool(full[idx].abs().max() > 0)
    vc = c.gather(v)
    assert torch.equal(vc, v[idx])
    out = torch.empty(c.n_live, dtype=torch.float32, device=DEV)
    eng.local_compact(vc, out)
    assert torch.equal(out, c.gather(full)) and torch.equal(out, full[idx])
    assert torch.equal(c(vc), out)              # the captured compact product
    assert torch.equal(sess.local(v), full)      # ... and the captured full one, both graphs intact
    assert torch.equal(eng.local(v), full)


@pytest.mark.parametrize("case", gn.CAPTURED_CASES)
def test_captured_replay_is_bitwise_the_eager_product(case):
    """The product as the session replays it (one hipGraph over the engine's static buffers) against the eager launches."""
    sess, opt, model = _session(case)
    eng = sess.engine
    for seed in SEEDS:
        v = gn.probe(eng.n, seed, DEV)
        eager = eng.local(v).clone()
        assert torch.equal(sess.local(v), eager)
        assert torch.equal(sess(v), eager)
        assert torch.equal(eng.local(v), eager)
    assert bool(eager.abs().max() > 0)
