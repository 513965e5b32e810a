"""GPU: plain conv stacks with ``MaxPool2d`` layers on the plain-stack engine (``engine/plain.py``: a pooled unit's bias /
ReLU / pool is ONE launch per sweep direction, ``hf_pool_act_tangent_nhwc`` / ``hf_pool_act_adjoint_nhwc``), on
``testproblems.convpool_small`` -- the im2col'd first layer pooled (3x3 / stride 2, overlapping windows, 12x12 -> 5x5),
a second pooled layer (2x2 / stride 2 on the odd 5x5 map), an unpooled last layer.

Reference sides: float64 autograd of the STOCK model on the engine's own ReLU and pooling decisions (replayed, and
bounded: a replayed decision may differ from the float64 model's own only within rounding of a tie), and the fixture the
real reference wrote (``tests/golden/convnet_convpool.npz``, ``make_golden_convpool.py``).  Bounds are the ones
``test_engine_gpu.py`` states for All-CNN-C: 1e-6 (GGN) and 2e-6 (Hessian, gradient, logits, diagonal) against float64,
1e-5 against the reference's fp32 results."""

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
N_ALL = 844  # parameters of convpool_small


def _engine(batch, hessian=False, prep=None, make=tp.convpool_small):
    model, (x, t), lossf = make(batch_size=batch, device="cpu")
    if prep is not None:
        prep(model)
    cpu_params = [p.detach().clone() for p in model.parameters() if p.requires_grad]
    model, x, t = model.to(DEV), x.to(DEV), t.to(DEV)
    modelprep.prepare_model(model, channels_last=True)
    params = [p for p in model.parameters() if p.requires_grad]
    out = model(x)
    make_op = curvature.hessian_operator if hessian else curvature.ggn_operator
    op = make_op(lossf(out, t), out, params)
    return op, model, (x, t), lossf, cpu_params


def _decisions(op):
    """The engine's ReLU masks (full resolution, in layer order) and pool positions ([n, c, oh, ow], int64)."""
    masks = [(u.y > 0) for u in op.units if u.relu]
    pools = [u.pidx.permute(0, 3, 1, 2).long() for u in op.units if u.pool is not None]
    return masks, pools


def _replay(model, masks, pools, margin=1e-5):
    """Make every ``nn.ReLU`` / ``nn.MaxPool2d`` call of the float64 ``model`` take the given decisions (in call order),
    and bound what is replayed: a ReLU decision may differ from the model's own only where its input lies within
    ``margin`` x the layer's max-norm of zero, a pool position only where the value there is within the same distance
    of the window's own maximum."""
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

    def rewind():
        rc[0], pc[0] = 0, 0
    return rewind


def _float64(batch, op, prep=None, make=tp.convpool_small):
    """The float64 twin on the engine's decisions: (params, out, loss, x, t, lossf)."""
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


@pytest.mark.parametrize("batch", [2, 5])
@pytest.mark.parametrize("hessian", [False, True], ids=["ggn", "hessian"])
def test_products_gradient_logits_and_diagonal_match_float64_and_the_reference(batch, hessian):
    """``curvature.ggn_operator`` / ``hessian_operator`` of the prepared pooled stack IS a ``PlainStackEngine`` (without
    the pooled-layer support it is the autograd operator: this is the assertion that fails on the parent commit)."""
    op, model, (x, t), lossf, cpu_params = _engine(batch, hessian)
    assert isinstance(op, PlainStackEngine) and op.hessian == hessian
    assert [u.pool for u in op.units] == [(3, 3, 2, 2, 0, 0), (2, 2, 2, 2, 0, 0), None]
    assert op.units[0].im2col and op.n == N_ALL
    ref = RefTrace("convpool", f"b{batch}")
    ref.check_inputs(cpu_params, x.cpu())
    rp = RefTrace("convpool", f"b{batch}/" + ("hessian" if hessian else "ggn"))
    v = rp.probe().to(DEV)
    got = op(v).clone()
    for _ in range(3):
        assert torch.equal(op(v), got)  # bitwise repeatable
    p64, out64, loss64, t64 = _float64(batch, op)
    want = (curvature.HessianOperator(loss64, p64) if hessian else curvature.GGNOperator(loss64, out64, p64))(v.double())
    tight = 2e-6 if hessian else 1e-6
    within(_rel(got, want), tight)  # (1.4e-7 measured: no need to weigh it against stock fp32 autograd's own distance)
    # the reference's own results: its float64 twin and its fp32 product
    within(rp.vec_err64("", got), tight)
    within(rp.vec_err("", got), 1e-5)
    # symmetric operator
    u = torch.randn(op.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    gu = op(u).clone()
    a, b = float(u.double() @ got.double()), float(v.double() @ gu.double())
    within(abs(a - b), 1e-5 * abs(a), strict=False)
    # gradient, logits, loss
    grad64 = torch.cat([g.reshape(-1) for g in torch.autograd.grad(loss64, p64, retain_graph=True)])
    grad = op.gradient().clone()
    within(_rel(grad, grad64), 2e-6)
    within(ref.vec_err64("grad", grad), 2e-6)
    within(ref.vec_err("grad", grad), 1e-5)
    within(_rel(op.logits, out64.detach()), 2e-6)
    want_logits = torch.from_numpy(ref.array("logits"))
    within(_rel(op.logits.cpu(), want_logits), 1e-5)
    within(abs(float(op.loss_buf) - float(loss64)), 2e-6 * abs(float(loss64)), strict=False)
    within(abs(float(op.loss_buf) - ref.scalar("loss")), 1e-5 * abs(ref.scalar("loss")), strict=False)
    # diagonal empirical Fisher: per-sample float64 gradients on the same decisions (eval mode: the samples do not
    # interact, so the gradient of sample i's loss through the batch's pass IS its per-sample gradient)
    want_d = torch.zeros(op.n, dtype=torch.float64, device=DEV)
    for i in range(batch):
        g_i = torch.autograd.grad(lossf(out64[i:i + 1], t64[i:i + 1]), p64, retain_graph=True)
        want_d += torch.cat([g.reshape(-1) for g in g_i]) ** 2
    want_d /= batch
    got_d = op.diag_ef("mean").clone()
    within(_rel(got_d, want_d), 2e-6)
    within(ref.vec_err64("diag", got_d), 2e-6)
    within(ref.vec_err("diag", got_d), 1e-5)
    assert torch.equal(op.diag_ef("mean"), got_d)
    assert torch.equal(op(v), got)  # (the products are untouched by the first-order sweeps)


@pytest.mark.parametrize("batch", [2, 5])
def test_batched_diagonal_matches_float64_and_the_reference(batch, monkeypatch):
    """``HF_DIAG_EF_BATCHED=1``: one squared-sum launch per layer on the same cotangents."""
    monkeypatch.setenv("HF_DIAG_EF_BATCHED", "1")
    op, model, (x, t), lossf, _ = _engine(batch)
    assert isinstance(op, PlainStackEngine) and op._diag_batched
    ref = RefTrace("convpool", f"b{batch}")
    got_d = op.diag_ef("mean").clone()
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


def test_a_pooled_layer_costs_four_launches_per_product(monkeypatch):
    """The launches of one GGN product, counted as ``test_dense_launch_order_gpu.py`` does (a proxy around the library):
    per layer the tangent convolution, ONE bias / ReLU (/ pool) tangent launch, ONE adjoint launch, the convolution's
    gradients -- 4, pooled or not; the stem's max-pool launches and, for the pooled units, ``hf_chan_affine_ex`` do not
    appear."""
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
    once = {"hf_pool_ce_head", "hf_pack_ex", "hf_bn_sums_multi", "hf_unpack_tangent_ex", "hf_unpack_weights"}
    per_layer = [n for n in got if n not in once]
    assert len(per_layer) == 4 * len(op.units), got
    assert got.count("hf_pool_act_tangent_nhwc") == 2 and got.count("hf_pool_act_adjoint_nhwc") == 2, got
    assert got.count("hf_chan_affine_ex") == 1, got  # (the unpooled last layer's)
    assert "hf_maxpool_tangent_nhwc" not in got and "hf_maxpool_adjoint_nhwc" not in got, got
    assert all(got.count(n) <= 1 for n in once), got
    # the sequence: tangent sweep in layer order, head, adjoint sweep in reverse
    order = [n for n in got if n.startswith(("hf_pool_act", "hf_chan_affine", "hf_bn_adjoint", "hf_pool_ce"))]
    assert order[:3] == ["hf_pool_act_tangent_nhwc", "hf_pool_act_tangent_nhwc", "hf_chan_affine_ex"], order
    assert order[3] == "hf_pool_ce_head" and order[-2:] == ["hf_pool_act_adjoint_nhwc"] * 2, order


def test_three_default_steps_through_the_session_match_the_reference_trace():
    """``HessianFree(graph_matvec=True).step()`` on the pooled stack runs on the persistent session (own forward pass with
    the pool launches, loss head, gradient sweep, graphed products); the three-step trace against the real reference's at
    the bounds of the All-CNN-C trace (``compare_trace``'s defaults)."""
    ref = RefTrace("convpool", "steps")
    seeds = (21, 22, 23)  # (make_golden_convpool.STEP_SEEDS: the reference's fp32 and float64 traces agree there)
    model, _, lossf = tp.convpool_small(batch_size=2, device="cpu", data_seed=seeds[0])
    ref.check_inputs([p for p in model.parameters() if p.requires_grad])
    model = model.to(DEV)
    modelprep.prepare_model(model, channels_last=True)
    opt = hf.HessianFree(model.parameters(), graph_matvec=True)
    finals = []
    for i in range(3):
        _, (x, t), _ = tp.convpool_small(batch_size=2, device="cpu", data_seed=seeds[i])
        ref.check_inputs(x=x, step=i)
        x, t = x.to(DEV), t.to(DEV)

        def forward():
            out = model(x)
            return lossf(out, t), out

        finals.append(opt.step(forward))
        assert opt.path_report()["step"]["path"] == "session", opt.path_report()
    assert opt._session is not None and opt._session.steps == 3
    assert isinstance(opt._session.engine, PlainStackEngine)
    compare_trace(opt.state, finals, ref)


def _freeze_first(model):
    conv = next(m for m in model.modules() if isinstance(m, torch.nn.Conv2d))
    for p in conv.parameters():
        p.requires_grad_(False)


@pytest.mark.parametrize("hessian", [False, True], ids=["ggn", "hessian"])
def test_frozen_first_convolution(hessian):
    """The pooled first layer frozen: dead for both sweeps (its pooled map is a constant input of the second layer, which
    needs no data gradient); the product on the trainable subset against float64, the frozen tensors untouched."""
    op, model, (x, t), lossf, _ = _engine(2, hessian, prep=_freeze_first)
    assert isinstance(op, PlainStackEngine) and op.dead_units == 1 and op.n == N_ALL - (8 * 27 + 8)
    conv = next(m for m in model.modules() if isinstance(m, torch.nn.Conv2d))
    before = [p.detach().clone() for p in conv.parameters()]
    v = torch.randn(op.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(8))
    got = op(v).clone()
    assert torch.equal(op(v), got)
    p64, out64, loss64, _ = _float64(2, op, prep=_freeze_first)
    want = (curvature.HessianOperator(loss64, p64) if hessian else curvature.GGNOperator(loss64, out64, p64))(v.double())
    within(_rel(got, want), 2e-6 if hessian else 1e-6)
    grad64 = torch.cat([g.reshape(-1) for g in torch.autograd.grad(loss64, p64)])
    within(_rel(op.gradient(), grad64), 2e-6)
    op.diag_ef("mean")
    assert all(torch.equal(a, b.detach()) and b.grad is None for a, b in zip(before, conv.parameters()))


class _Net(torch.nn.Module):
    def __init__(self, layers, detour=False):
        super().__init__()
        self.net, self.detour = torch.nn.Sequential(*layers), detour

    def forward(self, x):
        if self.detour:  # the pool reads a COPY of the unit's output: its record is not the unit's
            x = self.net[1](self.net[0](x)) * 1.0
            return torch.flatten(self.net[2:](x), -3)
        return torch.flatten(self.net(x), -3)


def _declined_variants():
    C, R, P, A, G = torch.nn.Conv2d, torch.nn.ReLU, torch.nn.MaxPool2d, torch.nn.AvgPool2d, torch.nn.AdaptiveAvgPool2d
    return {
        "pool_before_gap": (lambda: _Net([C(3, 8, 3, 1, 1), R(), C(8, 4, 1), P(2, 2), G(1)]), "MaxPool2d behind conv1"),
        "relu_behind_pool": (lambda: _Net([C(3, 8, 3, 1, 1), P(2, 2), R(), C(8, 4, 1), G(1)]), "ReLU behind the MaxPool2d"),
        "avgpool": (lambda: _Net([C(3, 8, 3, 1, 1), R(), A(2, 2), C(8, 4, 1), G(1)]), "AvgPool2d"),
        "ceil_mode": (lambda: _Net([C(3, 8, 3, 1, 1), R(), P(3, 2, ceil_mode=True), C(8, 4, 1), G(1)]),
                      "MaxPool2d behind conv0"),
        "dilation": (lambda: _Net([C(3, 8, 3, 1, 1), R(), P(2, 2, dilation=2), C(8, 4, 1), G(1)]), "MaxPool2d behind conv0"),
        "detour": (lambda: _Net([C(3, 8, 3, 1, 1), R(), P(2, 2), C(8, 4, 1), G(1)], detour=True), "MaxPool2d behind conv0"),
    }


@pytest.mark.parametrize("name", sorted(_declined_variants()))
def test_declined_variants_keep_the_autograd_path_and_say_why(name):
    build, reason = _declined_variants()[name]
    torch.manual_seed(0)
    model = build().eval()
    gen = torch.Generator().manual_seed(1)
    x, t = torch.rand(2, 3, 8, 8, generator=gen), torch.randint(0, 4, (2,), generator=gen)
    import copy

    m64 = copy.deepcopy(model).double().to(DEV)
    model, x, t = model.to(DEV), x.to(DEV), t.to(DEV)
    modelprep.prepare_model(model, channels_last=True)
    lossf = torch.nn.CrossEntropyLoss()
    params = list(model.parameters())
    out = model(x)
    why = []
    assert FusedGGNEngine.try_build(lossf(out, t), out, params, why=why) is None
    assert any(reason in w for w in why), why
    out = model(x)
    op = curvature.ggn_operator(lossf(out, t), out, params)
    assert type(op) is curvature.GGNOperator
    v = torch.randn(op.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    out64 = m64(x.double())
    want = curvature.GGNOperator(lossf(out64, t), out64, list(m64.parameters()))(v.double())
    within(_rel(op(v), want), 1e-6)
    opt = hf.HessianFree(model.parameters(), cg_max_iter=3)

    def forward():
        o = model(x)
        return lossf(o, t), o

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        opt.step(forward)
    rep = opt.path_report()["step"]
    assert rep["path"] == "eager" and reason in rep["declined"], rep
