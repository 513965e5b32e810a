"""GPU: conv stacks that end in ``Flatten`` + ``Linear`` layers on the plain-stack engine (``engine/plain.py``: the last
unit writes a ``[t_x | x]`` NHWC operand, ``hf_flatten_nhwc_rows`` / ``hf_unflatten_slabs_nhwc`` cross the boundary, the
tail runs on the skinny GEMMs of hf_dense.hip), on ``testproblems.convfc_small`` (two pooled units, the last one pooled,
``Linear(32->20) ReLU Linear(20->10)``) and ``testproblems.convfc_flat`` (one unpooled im2col'd unit on a 6x5 map,
``Linear(240->10)``).

Reference sides: float64 autograd of the STOCK model on the engine's own ReLU and pooling decisions (replayed as in
``test_pooled_stack_engine_gpu.py``, the tail's ReLU masks included, and bounded: a replayed decision may differ from the
float64 model's own only within rounding of a tie), and the fixture the real reference wrote
(``tests/golden/convnet_convfc.npz``, ``make_golden_convfc.py``).  Bounds are the project's (``test_engine_gpu.py``):
1e-6 (GGN) and 2e-6 (gradient, logits, loss, diagonal) against float64, 1e-5 against the reference's fp32 results."""

import types
import warnings

import pytest
import torch
from tol import within

import pytorchhessianfree_amd as hf
from helpers import RefTrace, compare_trace
from pytorchhessianfree_amd import _lib, curvature, modelprep
from pytorchhessianfree_amd import testproblems as tp
from pytorchhessianfree_amd.engine import FusedGGNEngine, PlainStackEngine

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_SMALL, N_FLAT = 1678, 2634  # parameters of convfc_small / convfc_flat
STEP_SEEDS, STEP_BATCH = (31, 32, 33), 5  # (make_golden_convfc: the reference's fp32 and float64 traces agree there)


def _engine(batch, prep=None, make=tp.convfc_small, hessian=False, lossf=None, onehot=False):
    model, (x, t), lossf0 = make(batch_size=batch, device="cpu")
    lossf = lossf0 if lossf is None else lossf
    if prep is not None:
        prep(model)
    cpu_params = [p.detach().clone() for p in model.parameters() if p.requires_grad]
    if onehot:
        t = torch.nn.functional.one_hot(t, 10).to(torch.float32)
    model, x, t = model.to(DEV), x.to(DEV), t.to(DEV)
    modelprep.prepare_model(model, channels_last=True)
    params = [p for p in model.parameters() if p.requires_grad]
    out = model(x)
    make_op = curvature.hessian_operator if hessian else curvature.ggn_operator
    op = make_op(lossf(out, t), out, params)
    return op, model, (x, t), lossf, cpu_params


def _decisions(op):
    """The engine's ReLU masks in call order (the units' at full resolution, then the tail's) and pool positions
    ([n, c, oh, ow], int64)."""
    masks = [(u.y > 0) for u in op.units if u.relu] + [(u.y > 0) for u in op.classifier if u.act == 1]
    pools = [u.pidx.permute(0, 3, 1, 2).long() for u in op.units if u.pool is not None]
    return masks, pools


def _replay(model, masks, pools, margin=1e-5):
    """Make every ``nn.ReLU`` / ``nn.MaxPool2d`` call of the float64 ``model`` take the given decisions (in call order),
    and bound what is replayed: a ReLU decision may differ from the model's own only where its input lies within
    ``margin`` x the layer's max-norm of zero, a pool position only where the value there is within the same distance
    of the window's own maximum.  (A condition on the float64 model, not a tolerance.)"""
    rc, pc = [0], [0]

    def relu_forward(self, inp):
        m = masks[rc[0]]
        rc[0] += 1
        diff = (inp > 0) != m
        if bool(diff.any()):
            within(float(inp[diff].abs().max() / inp.abs().max()), margin, note="replayed ReLU decision far from zero")
        return inp * m.to(inp.dtype)

    def pool_forward(self, inp):
        idx = pools[pc[0]]
        pc[0] += 1
        own = torch.nn.functional.max_pool2d(inp, self.kernel_size, self.stride, self.padding)
        got = inp.flatten(2).gather(2, idx.flatten(2)).view_as(own)
        within(float((own - got).detach().abs().max() / inp.detach().abs().max().clamp_min(1e-30)), margin,
               note="replayed pool position far from the window's maximum")
        return got

    for mod in model.modules():
        if isinstance(mod, torch.nn.ReLU):
            mod.forward = types.MethodType(relu_forward, mod)
        elif isinstance(mod, torch.nn.MaxPool2d):
            mod.forward = types.MethodType(pool_forward, mod)


def _float64(batch, op, prep=None, make=tp.convfc_small):
    """The float64 twin on the engine's decisions: (params, out, loss, t)."""
    model, (x, t), lossf = make(batch_size=batch, device=DEV)
    if prep is not None:
        prep(model)
    model, x = model.double(), x.double()
    _replay(model, *_decisions(op))
    params = [p for p in model.parameters() if p.requires_grad]
    out = model(x)
    return params, out, lossf(out, t), t


def _rel(got, want):
    return float((got.double() - want.double()).abs().max() / want.double().abs().max())


def _diag64(lossf, p64, out64, t64, batch, n):
    """Per-sample float64 gradients on the same decisions (eval mode: the samples do not interact)."""
    want = torch.zeros(n, dtype=torch.float64, device=DEV)
    for i in range(batch):
        g_i = torch.autograd.grad(lossf(out64[i:i + 1], t64[i:i + 1]), p64, retain_graph=True)
        want += torch.cat([g.reshape(-1) for g in g_i]) ** 2
    return want / batch


CASES = {"small-b2": (tp.convfc_small, 2), "small-b5": (tp.convfc_small, 5), "flat-b3": (tp.convfc_flat, 3)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_products_gradient_logits_and_diagonal_match_float64_and_the_reference(case):
    """``curvature.ggn_operator`` of the prepared model IS a ``PlainStackEngine`` (without the tail it is the autograd
    operator, "unsupported layer Flatten": this is the assertion that fails on the parent commit)."""
    make, batch = CASES[case]
    op, model, (x, t), lossf, cpu_params = _engine(batch, make=make)
    assert isinstance(op, PlainStackEngine) and not op.hessian
    if make is tp.convfc_small:
        assert [u.pool for u in op.units] == [(3, 3, 2, 2, 0, 0), (2, 2, 2, 2, 0, 0)] and op.n == N_SMALL
        assert [(u.c_in, u.c_out, u.act) for u in op.classifier] == [(32, 20, 1), (20, 10, 0)]
        assert op._tail_dims == (batch, 4, 8)
    else:
        assert [u.pool for u in op.units] == [None] and op.n == N_FLAT
        assert [(u.c_in, u.c_out, u.act) for u in op.classifier] == [(240, 10, 0)]
        assert op._tail_dims == (batch, 30, 8)
    assert op.units[0].im2col
    ref = rp = None
    if make is tp.convfc_small:
        ref, rp = RefTrace("convfc", f"b{batch}"), RefTrace("convfc", f"b{batch}/ggn")
        ref.check_inputs(cpu_params, x.cpu())
        v = rp.probe().to(DEV)
    else:
        v = torch.randn(op.n, generator=torch.Generator().manual_seed(74)).to(DEV)
    got = op(v).clone()
    for _ in range(3):
        assert torch.equal(op(v), got)  # bitwise repeatable (4 calls)
    p64, out64, loss64, t64 = _float64(batch, op, make=make)
    want = curvature.GGNOperator(loss64, out64, p64)(v.double())
    e = _rel(got, want)
    print(f"{case}: ggn vs float64 {e:.2e}")
    within(e, 1e-6)
    if rp is not None:  # the reference's own results: its float64 twin and its fp32 product
        within(rp.vec_err64("", got), 1e-6)
        within(rp.vec_err("", got), 1e-5)
    # symmetric operator
    u = torch.randn(op.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    gu = op(u).clone()
    a, b = float(u.double() @ got.double()), float(v.double() @ gu.double())
    within(abs(a - b), 1e-5 * abs(a), strict=False)
    # gradient, logits, loss
    grad64 = torch.cat([g.reshape(-1) for g in torch.autograd.grad(loss64, p64, retain_graph=True)])
    grad = op.gradient().clone()
    e = _rel(grad, grad64)
    print(f"{case}: gradient vs float64 {e:.2e}")
    within(e, 2e-6)
    e = _rel(op.logits, out64.detach())
    print(f"{case}: logits vs float64 {e:.2e}")
    within(e, 2e-6)
    within(abs(float(op.loss_buf) - float(loss64.detach())), 2e-6 * abs(float(loss64.detach())), strict=False)
    if ref is not None:
        within(ref.vec_err64("grad", grad), 2e-6)
        within(ref.vec_err("grad", grad), 1e-5)
        within(_rel(op.logits.cpu(), torch.from_numpy(ref.array("logits"))), 1e-5)
        within(abs(float(op.loss_buf) - ref.scalar("loss")), 1e-5 * abs(ref.scalar("loss")), strict=False)
    # diagonal empirical Fisher
    want_d = _diag64(lossf, p64, out64, t64, batch, op.n)
    got_d = op.diag_ef("mean").clone()
    e = _rel(got_d, want_d)
    print(f"{case}: diag_ef vs float64 {e:.2e}")
    within(e, 2e-6)
    if ref is not None:
        within(ref.vec_err64("diag", got_d), 2e-6)
        within(ref.vec_err("diag", got_d), 1e-5)
    assert torch.equal(op.diag_ef("mean"), got_d)
    assert torch.equal(op(v), got)  # (the products are untouched by the first-order sweeps)


@pytest.mark.parametrize("case", sorted(CASES))
def test_batched_diagonal_matches_float64_and_the_reference(case, monkeypatch):
    """``HF_DIAG_EF_BATCHED=1``: one squared-sum launch per conv layer; the tail's entries by the same dense launches."""
    monkeypatch.setenv("HF_DIAG_EF_BATCHED", "1")
    make, batch = CASES[case]
    op, model, (x, t), lossf, _ = _engine(batch, make=make)
    assert isinstance(op, PlainStackEngine) and op._diag_batched
    got_d = op.diag_ef("mean").clone()
    p64, out64, _loss64, t64 = _float64(batch, op, make=make)
    within(_rel(got_d, _diag64(lossf, p64, out64, t64, batch, op.n)), 2e-6)
    if make is tp.convfc_small:
        ref = RefTrace("convfc", f"b{batch}")
        within(ref.vec_err64("diag", got_d), 2e-6)
        within(ref.vec_err("diag", got_d), 1e-5)
    assert torch.equal(op.diag_ef("mean"), got_d)


class _Recorder:
    """Forwards every attribute to the real library; a call of an ``hf_*`` function appends its name to ``names``."""

    def __init__(self, lib, names):
        self._lib, self._names = lib, names

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("hf_"):
            return fn

        def call(*args):
            self._names.append(name)
            return fn(*args)

        return call


def test_the_launches_of_one_product(monkeypatch):
    """One GGN product of ``convfc_small``, counted through a proxy around the library: 4 launches per conv unit as
    without a tail; the tail adds one flatten, per layer 2 tangent and 3 adjoint launches, the loss Hessian and one
    unflatten; one gather takes the tail's gradients with the units'."""
    names = []
    proxy = _Recorder(_lib.load(), names)
    monkeypatch.setattr(_lib, "load", lambda: proxy)
    op, *_ = _engine(2)
    assert isinstance(op, PlainStackEngine) and names
    v = torch.randn(op.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(6))
    del names[:]
    op.local(v)
    torch.cuda.synchronize()
    got = list(names)
    once = {"hf_pack_ex", "hf_bn_sums_multi", "hf_unpack_tangent_ex", "hf_unpack_weights"}
    assert all(got.count(n) <= 1 for n in once) and got.count("hf_pack_ex") == 1, got
    tail = ["hf_flatten_nhwc_rows"] + ["hf_dense_tangent_slabs", "hf_dense_act_tangent"] * 2 + ["hf_softmax_ce_hvp"] \
        + ["hf_dense_act_adjoint", "hf_dense_wgrad", "hf_dense_dgrad_slabs"] * 2 + ["hf_unflatten_slabs_nhwc"]
    seq = [n for n in got if n.startswith(("hf_dense", "hf_flatten", "hf_unflatten", "hf_softmax"))]
    assert seq == tail, seq
    rest = [n for n in got if n not in once and n not in tail]
    assert len(rest) == 4 * len(op.units), got
    assert got.count("hf_pool_act_tangent_nhwc") == 2 and got.count("hf_pool_act_adjoint_nhwc") == 2, got
    assert "hf_pool_ce_head" not in got
    # the tail stands between the sweeps: behind the last unit's tangent, in front of its adjoint
    i0, i1 = got.index("hf_flatten_nhwc_rows"), got.index("hf_unflatten_slabs_nhwc")
    assert got.index("hf_pool_act_tangent_nhwc", 1) < i0 < i1 < got.index("hf_pool_act_adjoint_nhwc")


def _convs(model):
    return [m for m in model.modules() if isinstance(m, torch.nn.Conv2d)]


def _freeze_first_conv(model):
    for p in _convs(model)[0].parameters():
        p.requires_grad_(False)


def _freeze_convs(model):
    for conv in _convs(model):
        for p in conv.parameters():
            p.requires_grad_(False)


def _freeze_first_tail_weight(model):
    next(m for m in model.modules() if isinstance(m, torch.nn.Linear)).weight.requires_grad_(False)


@pytest.mark.parametrize("prep,n,dead", [(_freeze_first_conv, N_SMALL - (8 * 27 + 8), 1),
                                         (_freeze_first_tail_weight, N_SMALL - 32 * 20, 0)],
                         ids=["conv0", "tail_weight"])
def test_frozen_parameters_match_float64(prep, n, dead):
    """Conv unit 0 frozen: a dead prefix.  The first tail layer's weight frozen: its GEMM reads no slice of the vector
    (``V = NULL``), the gather has no entry for it, its bias stays trainable.  Products, gradient and diagonal on the
    trainable subset against float64; the frozen tensors untouched."""
    op, model, (x, t), lossf, _ = _engine(2, prep=prep)
    assert isinstance(op, PlainStackEngine) and op.dead_units == dead and op.n == n
    frozen = [p for p in model.parameters() if not p.requires_grad]
    before = [p.detach().clone() for p in frozen]
    v = torch.randn(op.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(8))
    got = op(v).clone()
    assert torch.equal(op(v), got)
    p64, out64, loss64, t64 = _float64(2, op, prep=prep)
    within(_rel(got, curvature.GGNOperator(loss64, out64, p64)(v.double())), 1e-6)
    grad64 = torch.cat([g.reshape(-1) for g in torch.autograd.grad(loss64, p64, retain_graph=True)])
    within(_rel(op.gradient(), grad64), 2e-6)
    within(_rel(op.diag_ef("mean"), _diag64(lossf, p64, out64, t64, 2, op.n)), 2e-6)
    assert all(torch.equal(a, b.detach()) and b.grad is None for a, b in zip(before, frozen))


class _Tail(torch.nn.Module):
    """``ConvFCSmall``'s conv part with another tail."""

    def __init__(self, tail):
        super().__init__()
        C, R, P = torch.nn.Conv2d, torch.nn.ReLU, torch.nn.MaxPool2d
        self.net = torch.nn.Sequential(C(3, 8, 3, 1, 1), R(), P(3, 2), C(8, 8, 3, 1, 1), R(), P(2, 2), torch.nn.Flatten(),
                                       *tail)

    def forward(self, x):
        return self.net(x)


def _tanh_tail(batch_size, device):
    torch.manual_seed(0)
    model = _Tail([torch.nn.Linear(32, 20), torch.nn.Tanh(), torch.nn.Linear(20, 10)]).eval()
    _, data, lossf = tp.convfc_small(batch_size=batch_size, device=device)
    return model.to(device), data, lossf


def _inplace_tail(batch_size, device):
    torch.manual_seed(0)
    model = _Tail([torch.nn.Linear(32, 20), torch.nn.ReLU(inplace=True), torch.nn.Linear(20, 10)]).eval()
    _, data, lossf = tp.convfc_small(batch_size=batch_size, device=device)
    return model.to(device), data, lossf


DECLINED = {
    "tanh": (dict(batch=2, make=_tanh_tail), "unsupported layer Tanh in the classifier tail"),
    "inplace_relu": (dict(batch=2, make=_inplace_tail), "tail linear 0: followed by an in-place ReLU"),
    "batch_257": (dict(batch=257, make=tp.convfc_flat), "Linear tail: batch 257 > 256 rows"),
    "hessian": (dict(batch=2, hessian=True), "Hessian products through a classifier tail are not covered"),
    "mse": (dict(batch=2, lossf=torch.nn.MSELoss(), onehot=True), "needs a plain softmax cross-entropy loss"),
    "frozen_convs": (dict(batch=2, prep=_freeze_convs), "every convolution in front of the classifier tail is frozen"),
}


@pytest.mark.parametrize("name", sorted(DECLINED))
def test_declined_variants_keep_the_autograd_path_and_say_why(name):
    kw, reason = DECLINED[name]
    hessian = kw.get("hessian", False)
    op, model, (x, t), lossf, _ = _engine(**kw)
    assert type(op) is (curvature.HessianOperator if hessian else curvature.GGNOperator)
    params = [p for p in model.parameters() if p.requires_grad]
    out = model(x)
    why = []
    assert FusedGGNEngine.try_build(lossf(out, t), out, params, why=why, hessian=hessian) is None
    assert any("PlainStackEngine" in w and reason in w for w in why), why
    opt = hf.HessianFree(params, cg_max_iter=3, curvature_opt="hessian" if hessian else "ggn")

    def forward():
        o = model(x)
        return lossf(o, t), o

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        opt.step(forward)
    rep = opt.path_report()["step"]
    assert rep["path"] == "eager" and reason in rep["declined"], rep


def _steps(run):
    """Three default steps on fresh batches of the fixture's trace; ``run(opt, model, lossf, x, t)`` makes one."""
    ref = RefTrace("convfc", "steps")
    model, _, lossf = tp.convfc_small(batch_size=STEP_BATCH, device="cpu", data_seed=STEP_SEEDS[0])
    ref.check_inputs([p for p in model.parameters() if p.requires_grad])
    model = model.to(DEV)
    modelprep.prepare_model(model, channels_last=True)
    opt = hf.HessianFree(model.parameters(), graph_matvec=True)
    finals = []
    for i in range(3):
        _, (x, t), _ = tp.convfc_small(batch_size=STEP_BATCH, device="cpu", data_seed=STEP_SEEDS[i])
        ref.check_inputs(x=x, step=i)
        finals.append(run(opt, model, lossf, x.to(DEV), t.to(DEV)))
    return opt, finals, ref


def test_three_default_steps_through_the_session_match_the_reference_trace():
    """``HessianFree(graph_matvec=True).step()`` runs on the persistent session (own forward pass through the flatten
    launch and the tail's GEMMs, loss head, gradient sweep, graphed products); the three-step trace against the real
    reference's at ``compare_trace``'s defaults."""
    def run(opt, model, lossf, x, t):
        def forward():
            out = model(x)
            return lossf(out, t), out

        final = opt.step(forward)
        assert opt.path_report()["step"]["path"] == "session", opt.path_report()
        return final

    opt, finals, ref = _steps(run)
    assert opt._session is not None and opt._session.steps == 3
    assert isinstance(opt._session.engine, PlainStackEngine) and opt._session.engine.classifier
    compare_trace(opt.state, finals, ref)


def test_acc_step_on_two_chunks_equals_step_on_the_whole_batch():
    """One ``acc_step`` on chunks [2, 3] takes the accumulated session (one engine per chunk) and makes the update
    ``step()`` makes on the concatenated batch: final loss and parameters to 1e-5."""
    results = []
    for acc in (False, True):
        model, (x, t), lossf = tp.convfc_small(batch_size=STEP_BATCH, device="cpu", data_seed=STEP_SEEDS[0])
        start = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).to(DEV)
        model, x, t = model.to(DEV), x.to(DEV), t.to(DEV)
        modelprep.prepare_model(model, channels_last=True)
        opt = hf.HessianFree(model.parameters(), graph_matvec=True)
        if acc:
            chunks = [(x[:2].contiguous(), t[:2].contiguous()), (x[2:].contiguous(), t[2:].contiguous())]
            final = opt.acc_step(model, lossf, chunks, reduction="mean")
            rep = opt.path_report()["acc_step"]
            assert rep["path"] == "acc-session" and rep["declined"] is None, rep
        else:
            def forward():
                out = model(x)
                return lossf(out, t), out

            final = opt.step(forward)
            assert opt.path_report()["step"]["path"] == "session", opt.path_report()
        results.append((float(final), torch.cat([p.detach().reshape(-1) for p in model.parameters()]).clone()))
    (f_step, p_step), (f_acc, p_acc) = results
    assert _rel(p_step, start) > 1e-3  # (both calls moved the parameters)
    print(f"acc vs step: final {abs(f_acc - f_step) / abs(f_step):.2e}  parameters {_rel(p_acc, p_step):.2e}")
    within(abs(f_acc - f_step), 1e-5 * abs(f_step), strict=False)
    within(_rel(p_acc, p_step), 1e-5)
