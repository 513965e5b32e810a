"""GPU: conv stacks that end in ``Flatten`` + ``Linear`` layers on the plain-stack engine (``engine/plain.py``: the last
unit writes a ``[t_x | x]`` NHWC operand, ``hf_flatten_nhwc_rows`` / ``hf_unflatten_slabs_nhwc`` cross the boundary, the
tail runs on the skinny GEMMs of hf_dense.hip), on ``testproblems.convfc_small`` (two pooled units, the last one pooled,
``Linear(32->20) ReLU Linear(20->10)``) and ``testproblems.convfc_flat`` (one unpooled im2col'd unit on a 6x5 map,
``Linear(240->10)``).

Reference sides (``stack_harness.py``): float64 autograd of the STOCK model on the engine's own ReLU and pooling decisions
(replayed, the tail's ReLU masks included, and bounded: a replayed decision may differ from the float64 model's own only
within rounding of a tie), and the fixture the real reference wrote (``tests/golden/convnet_convfc.npz``,
``make_golden_convfc.py``).  Bounds are the project's (``test_engine_gpu.py``): 1e-6 (GGN) and 2e-6 (gradient, logits,
loss, diagonal) against float64, 1e-5 against the reference's fp32 results."""

import pytest
import torch
from tol import within

import pytorchhessianfree_amd as hf
from helpers import RefTrace, compare_trace
from pytorchhessianfree_amd import curvature, modelprep
from pytorchhessianfree_amd import testproblems as tp
from pytorchhessianfree_amd.engine import PlainStackEngine
from stack_harness import (DEV, check_point, declined, diag64, engine, float64_twin, grad64, product64, record_launches,
                           rel, run_steps)

pytestmark = pytest.mark.gpu
N_SMALL, N_FLAT = 1678, 2634  # parameters of convfc_small / convfc_flat
STEP_SEEDS, STEP_BATCH = (31, 32, 33), 5  # (make_golden_convfc: the reference's fp32 and float64 traces agree there)

CASES = {"small-b2": (tp.convfc_small, 2), "small-b5": (tp.convfc_small, 5), "flat-b3": (tp.convfc_flat, 3)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_products_gradient_logits_and_diagonal_match_float64_and_the_reference(case):
    """``curvature.ggn_operator`` of the prepared model IS a ``PlainStackEngine`` (without the tail it is the autograd
    operator, "unsupported layer Flatten": this is the assertion that fails on the parent commit).  ``convfc_flat`` has
    no fixture: float64 alone."""
    make, batch = CASES[case]
    op, model, (x, t), lossf, cpu_params = engine(make, batch)
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
    fixture = ("convfc", f"b{batch}") if make is tp.convfc_small else None
    check_point(op, make, batch, x, lossf, cpu_params, fixture, case)


@pytest.mark.parametrize("case", sorted(CASES))
def test_batched_diagonal_matches_float64_and_the_reference(case, monkeypatch):
    """``HF_DIAG_EF_BATCHED=1``: one squared-sum launch per conv layer; the tail's entries by the same dense launches."""
    monkeypatch.setenv("HF_DIAG_EF_BATCHED", "1")
    make, batch = CASES[case]
    op, model, (x, t), lossf, _ = engine(make, batch)
    assert isinstance(op, PlainStackEngine) and op._diag_batched
    got_d = op.diag_ef("mean").clone()
    p64, out64, _loss64, t64 = float64_twin(make, batch, op)
    within(rel(got_d, diag64(lossf, p64, out64, t64, batch, op.n)), 2e-6)
    if make is tp.convfc_small:
        ref = RefTrace("convfc", f"b{batch}")
        within(ref.vec_err64("diag", got_d), 2e-6)
        within(ref.vec_err("diag", got_d), 1e-5)
    assert torch.equal(op.diag_ef("mean"), got_d)


def test_the_launches_of_one_product(monkeypatch):
    """One GGN product of ``convfc_small``, counted through a proxy around the library: 4 launches per conv unit as
    without a tail; the tail adds one flatten, per layer 2 tangent and 3 adjoint launches, the loss Hessian and one
    unflatten; one gather takes the tail's gradients with the units'."""
    names = record_launches(monkeypatch)
    op, *_ = engine(tp.convfc_small, 2)
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
    op, model, (x, t), lossf, _ = engine(tp.convfc_small, 2, prep=prep)
    assert isinstance(op, PlainStackEngine) and op.dead_units == dead and op.n == n
    frozen = [p for p in model.parameters() if not p.requires_grad]
    before = [p.detach().clone() for p in frozen]
    v = torch.randn(op.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(8))
    got = op(v).clone()
    assert torch.equal(op(v), got)
    p64, out64, loss64, t64 = float64_twin(tp.convfc_small, 2, op, prep=prep)
    within(rel(got, product64(p64, out64, loss64, v)), 1e-6)
    within(rel(op.gradient(), grad64(loss64, p64)), 2e-6)
    within(rel(op.diag_ef("mean"), diag64(lossf, p64, out64, t64, 2, op.n)), 2e-6)
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
    op, model, (x, t), lossf, _ = engine(**{"make": tp.convfc_small, **kw})
    assert type(op) is (curvature.HessianOperator if hessian else curvature.GGNOperator)
    declined(model, x, t, lossf, reason, hessian=hessian, who="PlainStackEngine")


def test_three_default_steps_through_the_session_match_the_reference_trace():
    """``HessianFree(graph_matvec=True).step()`` runs on the persistent session (own forward pass through the flatten
    launch and the tail's GEMMs, loss head, gradient sweep, graphed products); the three-step trace against the real
    reference's at ``compare_trace``'s defaults."""
    opt, finals, _, ref = run_steps(tp.convfc_small, STEP_SEEDS, STEP_BATCH, ("convfc", "steps"), graph_matvec=True)
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
    assert rel(p_step, start) > 1e-3  # (both calls moved the parameters)
    print(f"acc vs step: final {abs(f_acc - f_step) / abs(f_step):.2e}  parameters {rel(p_acc, p_step):.2e}")
    within(abs(f_acc - f_step), 1e-5 * abs(f_step), strict=False)
    within(rel(p_acc, p_step), 1e-5)
