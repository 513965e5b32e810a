"""GPU: the classifier tail of ``PlainStackEngine`` (``nn.Flatten``, ``hf_flatten_nhwc_rows`` / ``hf_unflatten_slabs_nhwc``,
the dense kernels on slices of the flat vector) on the tail cases of ``geometry_nets.py`` against the float64 reference of
the STOCK model, on the engine's own ReLU decisions and pool positions (the units' masks, then the tail's; ``u.pidx``;
replayed under ``geometry_nets.MAX_FLIPS`` / ``MARGIN``), tensor by tensor: ``max|got_T - want_T| / max|want_T|`` for every
parameter tensor ``T``, exactly zero where the reference is exactly zero (``geometry_nets.per_tensor_errors``).

What the cases reach that ``convfc_small`` / ``convfc_flat`` do not stands in ``geometry_nets.TAIL_GEOMETRY``: data-gradient
slabs that are really summed (``sD > 1``), operands at offsets 1 and 2 mod 4 of the flat vector with row pitches that are no
multiple of 4, two flatten tiles with a partial last one both ways, a 1x1 and a pooled non-square last map, a last unit
without ReLU, batch 1 and 256, a bias-free ``Linear``, frozen tail tensors, a ``Dropout`` leaf in the tail.

Every case is prepared with ``modelprep.prepare_model(channels_last=True)`` and built through ``curvature.ggn_operator``; a
decline fails with the reasons.

Bounds (``BOUND_TAIL``).  Not taken from the engine: per quantity 3x the worst distance of STOCK fp32 autograd on the GPU
(``geometry_nets.stock_fp32_errors``) from the same float64 reference in the same per-tensor measure over the tail cases,
rounded up to one significant digit -- the policy of ``test_engine_geometry_gpu.BOUND``, kept apart from it.  Both series,
stock fp32 and the engine's own figures per case, quantity and tensor, stand in ``profiles/r28_tail_geometry.jsonl``."""

import copy
import hashlib
import warnings

import geometry_nets as gn
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

# quantity: 3 x (worst figure of the series "stock_fp32" in profiles/r28_tail_geometry.jsonl over the tail cases), rounded
# up to one significant digit -- ``scripts/engine_geometry_errors.py --cases tail`` writes that file and prints these lines
BOUND_TAIL = {
    "logits": 5e-7,    # 1.61e-7 (tail_rows_256)
    "loss": 4e-7,      # 1.12e-7 (tail_pixel)
    "gradient": 2e-6,  # 4.52e-7 (tail_rows_256)
    "ggn": 3e-6,       # 7.31e-7 (tail_wide_first)
    "diag_ef": 2e-6,   # 3.63e-7 (tail_rows_256)
}


# ---- frozen structure (on tail_rect_pooled): what is frozen, entries left, dead units at the input end ---------------
def _linears(model):
    return [m for m in model.modules() if isinstance(m, nn.Linear)]


def _freeze_first_tail_bias(model):
    _linears(model)[0].bias.requires_grad_(False)


def _freeze_last_linear(model):
    for p in _linears(model)[-1].parameters():
        p.requires_grad_(False)


def _freeze_conv0_and_first_tail_weight(model):
    for p in next(m for m in model.modules() if isinstance(m, nn.Conv2d)).parameters():
        p.requires_grad_(False)
    _linears(model)[0].weight.requires_grad_(False)


FROZEN = {
    "first_tail_bias": (_freeze_first_tail_bias, 2211 - 21, 0),
    "last_linear": (_freeze_last_linear, 2211 - (21 * 7 + 7), 0),
    "conv0_and_first_tail_weight": (_freeze_conv0_and_first_tail_weight, 2211 - (8 * 27 + 8) - 72 * 21, 1),
}
FROZEN_CASE = "tail_rect_pooled"


def _build(case, prep=None):
    """The engine of ``case`` through the package's entry point: ``(op, stock model on the CPU, batches, gpu model)``."""
    stock, batches = gn.make(case)
    if prep is not None:
        prep(stock)
    x, t = batches[0]
    model = copy.deepcopy(stock).to(DEV)
    modelprep.prepare_model(model, channels_last=True)
    params = [p for p in model.parameters() if p.requires_grad]
    out = model(x.to(DEV))
    why = []
    op = curvature.ggn_operator(nn.functional.cross_entropy(out, t.to(DEV)), out, params, why=why)
    assert type(op) is PlainStackEngine, (type(op).__name__, why)
    assert not op.hessian and not op.train_bn and op.classifier
    return op, stock, batches, model


_ENGINES, _REFS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_engines():
    """The engines and references the tests of this file share live as long as the file's tests run, no longer."""
    yield
    _ENGINES.clear()
    _REFS.clear()
    torch.cuda.empty_cache()


def _engine(case):
    if case not in _ENGINES:  # (built once per case, shared by the layout / forward / gradient / product tests)
        _ENGINES[case] = _build(case)
    return _ENGINES[case]


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
    print(f"[tail geometry] {quantity}: worst {errs[worst]:.2e} at {worst} (bound {BOUND_TAIL[quantity]})")
    for name, e in errs.items():
        within(e, BOUND_TAIL[quantity], note=(quantity, name, errs))


def _logits_error(op, ref):
    return float((op.logits.cpu().double() - ref.logits).abs().max() / ref.logits.abs().max())


# ---- what each test measures (also what scripts/engine_geometry_errors.py records) -----------------------------------
def forward_errors(case):
    op, stock, batches, _ = _engine(case)
    op.forward_own()
    ref = _reference((case, 0), stock, batches[0], op)
    return {"logits": {"logits": _logits_error(op, ref)}, "loss": {"loss": gn.scalar_error(op.loss_buf, ref.loss())}}


def gradient_errors(case):
    op, stock, batches, _ = _engine(case)
    ref = _reference((case, 0), stock, batches[0], op)
    return {"gradient": gn.per_tensor_errors(op.gradient(), ref.gradient(), gn.named_sizes(stock))}


def _product_errors(op, stock, ref):
    sizes = gn.named_sizes(stock)
    assert op.n == sum(k for _, k in sizes)
    worst, got = {}, []
    for seed in SEEDS:
        v = gn.probe(op.n, seed, DEV)
        g = op(v).clone()
        for _ in range(3):
            assert torch.equal(op(v), g)  # bitwise repeatable
        for name, e in gn.per_tensor_errors(g, ref.ggn(v), sizes).items():
            worst[name] = max(worst.get(name, 0.0), e)
        got.append((v, g))
    # a symmetric operator: <u, G v> == <v, G u>
    (u, gu), (v, gv) = got
    a, b = float(u.double() @ gv.double()), float(v.double() @ gu.double())
    within(abs(a - b), 1e-5 * abs(a), strict=False)
    return worst


def product_errors(case):
    op, stock, batches, _ = _engine(case)
    return {"ggn": _product_errors(op, stock, _reference((case, 0), stock, batches[0], op))}


def diag_errors(case):
    """Diagonal empirical Fisher at the first batch; then a second batch through ``set_batch`` and the engine's OWN
    forward pass (not the recorded one): loss, logits, gradient, diagonal again."""
    op, stock, batches, _ = _build(case)
    sizes = gn.named_sizes(stock)
    res = {"diag_ef": {}, "gradient": {}, "loss": {}, "logits": {}}
    for which, (x, t) in enumerate(batches):
        if which:
            op.set_batch(x.to(DEV), t.to(DEV))
            op.forward_own()
        ref = _reference((case, which), stock, (x, t), op)
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


# ---- the tests -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gn.TAIL_CASES)
def test_engine_layout_is_the_tail_cases_table(case):
    """The engine's units, pools, tail layers (split counts, offsets in the flat vector) and last-map dims are what
    ``geometry_nets.TAIL_GEOMETRY`` writes out."""
    op, stock, batches, model = _engine(case)
    lit = gn.TAIL_GEOMETRY[case]
    names = {m: n for n, m in model.named_modules()}
    got = {names[u.conv]: (tuple(u.x.shape[2:]), tuple(u.a.shape[2:]), 0 if u.im2col else u.live, u.rb) for u in op.units}
    first = lit["convs"][0][0]  # (an im2col'd unit reads no taps: its dead ones are zero columns of the im2col)
    im2col = case != "tail_pixel"
    assert got == {name: (hw, ohw, 0 if (im2col and name == first) else mask, rb)
                   for name, hw, ohw, mask, rb in lit["convs"]}
    assert [u.im2col for u in op.units] == [im2col] + [False] * (len(op.units) - 1)
    assert [u.pool for u in op.units] == lit["pools"]
    assert [(u.c_in, u.c_out, u.sT, u.sD, op._offs[u.pw], None if u.pb is None else op._offs[u.pb])
            for u in op.classifier] == lit["linears"]
    assert [u.act for u in op.classifier] == [1] * (len(op.classifier) - 1) + [0]
    assert op._tail_dims == lit["last"] and op.n == lit["n"] and op.dead_units == 0
    assert op.units[-1].relu == (case != "tail_pixel")
    # the slabs the adjoint sweep sums are as many as planned, each a whole [rows, c_in] map
    rows = lit["last"][0]
    assert [tuple(u.dslabs.shape) for u in op.classifier] == [(sd, rows * ci) for ci, _, _, sd, _, _ in lit["linears"]]
    assert [tuple(u.tslabs.shape) for u in op.classifier] == [(st, rows * co) for _, co, st, _, _, _ in lit["linears"]]


@pytest.mark.parametrize("case", gn.TAIL_CASES)
def test_forward_pass_matches_float64(case):
    errs = forward_errors(case)
    _assert("logits", errs["logits"])
    _assert("loss", errs["loss"])


@pytest.mark.parametrize("case", gn.TAIL_CASES)
def test_gradient_matches_float64_per_tensor(case):
    _assert("gradient", gradient_errors(case)["gradient"])


@pytest.mark.parametrize("case", gn.TAIL_CASES)
def test_ggn_product_matches_float64_per_tensor(case):
    _assert("ggn", product_errors(case)["ggn"])


@pytest.mark.parametrize("batched", [False, True], ids=["per_sample", "batched"])
@pytest.mark.parametrize("case", gn.TAIL_CASES)
def test_diagonal_fisher_and_a_second_batch_match_float64_per_tensor(case, batched, monkeypatch):
    monkeypatch.setenv("HF_DIAG_EF_BATCHED", "1" if batched else "0")
    errs = diag_errors(case)
    assert errs.pop("batched") == batched
    for quantity in ("diag_ef", "gradient", "loss", "logits"):
        _assert(quantity, errs[quantity])


@pytest.mark.parametrize("name", sorted(FROZEN))
def test_frozen_tail_structure_matches_float64_per_tensor(name):
    """``tail_rect_pooled`` with (a) the first tail bias frozen (its weight trainable), (b) the last Linear wholly
    frozen, (c) conv0 and the first tail weight frozen: product, gradient and diagonal per tensor on the trainable
    subset, the frozen tensors untouched."""
    prep, n, dead = FROZEN[name]
    op, stock, batches, model = _build(FROZEN_CASE, prep)
    sizes = gn.named_sizes(stock)
    assert op.n == n == sum(k for _, k in sizes) and op.dead_units == dead and op.frozen_any
    frozen = [p for p in model.parameters() if not p.requires_grad]
    before = [p.detach().clone() for p in frozen]
    assert frozen
    ref = _reference((FROZEN_CASE, name), stock, batches[0], op)
    _assert("ggn", _product_errors(op, stock, ref))
    _assert("gradient", gn.per_tensor_errors(op.gradient(), ref.gradient(), sizes))
    _assert("diag_ef", gn.per_tensor_errors(op.diag_ef("mean"), ref.diag_ef(), sizes))
    op.forward_own()
    _assert("logits", {"logits": _logits_error(op, ref)})
    _assert("loss", {"loss": gn.scalar_error(op.loss_buf, ref.loss())})
    assert all(torch.equal(a, b.detach()) and b.grad is None for a, b in zip(before, frozen))


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
    assert sess is not None and type(sess.engine) is PlainStackEngine and sess.engine.classifier, why
    return sess, opt, model


@pytest.mark.parametrize("case", gn.TAIL_CAPTURED_CASES)
def test_captured_replay_is_bitwise_the_eager_product(case):
    """The product as the session replays it (one hipGraph over the engine's static buffers; the tail's weights are
    read in place in the optimizer's flat vector, at the offsets of the table) against the eager launches."""
    sess, opt, model = _session(case)
    eng = sess.engine
    assert [op_off for *_, op_off, _ in gn.TAIL_GEOMETRY[case]["linears"]] == [eng._offs[u.pw] for u in eng.classifier]
    for seed in SEEDS:
        v = gn.probe(eng.n, seed, DEV)
        eager = eng.local(v).clone()
        assert torch.equal(sess.local(v), eager)
        assert torch.equal(sess(v), eager)
        assert torch.equal(eng.local(v), eager)
    assert bool(eager.abs().max() > 0)


# ---- a last map the flatten kernels do not take: declined by the layout, not by a kernel -----------------------------
class _SixChannels(nn.Module):
    """``Conv(3, 6) ReLU Flatten Linear``: the unit is im2col'd (3 input channels), so nothing checked its 6 output
    channels before ``hf_flatten_nhwc_rows`` met them."""

    def __init__(self, h, w):
        super().__init__()
        self.net = nn.Sequential(nn.Conv2d(3, 6, 3, 1, 1), nn.ReLU(), nn.Flatten(), nn.Linear(6 * h * w, 4))

    def forward(self, x):
        return self.net(x)


def test_a_last_map_of_six_channels_is_declined_with_the_channel_count():
    torch.manual_seed(gn.SEED)
    h, w = 4, 5
    model = _SixChannels(h, w).eval().to(DEV)
    x, t = torch.randn(2, 3, h, w).to(DEV), torch.randint(0, 4, (2,)).to(DEV)
    modelprep.prepare_model(model, channels_last=True)
    params = [p for p in model.parameters() if p.requires_grad]
    reason = "the last map has 6 channels"
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = model(x)
        why = []
        op = curvature.ggn_operator(nn.functional.cross_entropy(out, t), out, params, why=why)
        assert type(op) is curvature.GGNOperator, type(op).__name__
        assert any("PlainStackEngine" in line and reason in line for line in why), why
        assert not any("refused" in line for line in why), why
        out = model(x)
        why = []
        assert FusedGGNEngine.try_build(nn.functional.cross_entropy(out, t), out, params, why=why) is None
        assert any("PlainStackEngine" in line and reason in line for line in why), why
    # (a kernel's refusal warns: the layout declines before any launch)
    assert not [str(w.message) for w in caught if "fused curvature engine" in str(w.message)]
    opt = hf.HessianFree(params, cg_max_iter=3)

    def forward():
        o = model(x)
        return nn.functional.cross_entropy(o, t), o

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        opt.step(forward)
    rep = opt.path_report()["step"]
    assert rep["path"] == "eager" and reason in rep["declined"], rep
