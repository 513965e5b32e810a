"""GPU: ``HessianFree.acc_step()`` on the fused engine (``acc_session.AccumulatedSession``) -- loss, gradient and every
curvature product accumulated over lists of data chunks (reference ``/root/reference/hessianfree/optimizer.py:
519-606, :608-684, :767-814``), one engine per chunk, the chunks' sweeps on parallel branches of ONE product
graph inside ``cg()``'s iteration graph, trial losses as graph replays.

Oracles: (1) the reference's own statement of chunk additivity (``/root/reference/tests/test_optimizer_acc.py:
116-175``: accumulated == whole batch, ``1e-4``) against this package's ``step`` on the whole batch, and (2) the
CPU path -- stock model, torch autograd, generic accumulation, host logic with ``oracle.pcg`` (the reference's PCG
restated, pinned bit for bit by tests/golden/make_golden.py).  Tolerances are stated at the assertions."""

import warnings

import pytest
import torch
from tol import within

import pytorchhessianfree_amd as hf
from pytorchhessianfree_amd import modelprep
from pytorchhessianfree_amd import testproblems as tp

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEEDS = tp.RESNET18_B32_SEPARATED_SEEDS


def _flat(opt):
    return torch.cat([p.detach().reshape(-1) for p in opt._params_list])


def _chunks(x, t, sizes):
    out, o = [], 0
    for n in sizes:
        out.append((x[o:o + n].contiguous(), t[o:o + n].contiguous()))
        o += n
    return out


def _resnet_runs(kind, steps, sizes=(16, 16), **kw):
    """``kind``: "step" (whole batch through the session) or "acc" (chunks through the accumulated session)."""
    model, _, lossf = tp.resnet18_mnist(batch_size=32, device=DEV, data_seed=SEEDS[0])
    modelprep.prepare_model(model, channels_last=True)
    opt = hf.HessianFree(model.parameters(), graph_matvec=True, **kw)
    finals = []
    for i in range(steps):
        _, (x, t), _ = tp.resnet18_mnist(batch_size=32, device=DEV, data_seed=SEEDS[i])

        def forward():
            out = model(x)
            return lossf(out, t), out

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if kind == "step":
                finals.append(opt.step(forward))
            else:
                finals.append(opt.acc_step(model, lossf, _chunks(x, t, sizes), reduction="mean"))
    return opt, finals


def _same_trace(a, fa, b, fb, loss_tol=1e-5, final_tol=1e-4, iters=2):
    sa, sb = a.state, b.state
    for x, y in zip(sa["init_losses"], sb["init_losses"]):
        assert abs(x - y) <= loss_tol * abs(y)
    assert sa["cg_reasons"] == sb["cg_reasons"]
    assert sa["learning_rates"] == sb["learning_rates"]
    assert sa["dampings"] == sb["dampings"]
    for x, y in zip(sa["num_cg_iters"], sb["num_cg_iters"]):
        assert abs(x - y) <= iters
    for x, y in zip(fa, fb):
        assert abs(x - y) <= final_tol * abs(y)


def test_acc_step_on_engine_equals_step_on_whole_batch_and_is_repeatable():
    """ResNet-18 (config 2), eval-mode BatchNorm: ``acc_step`` on chunks [16, 16] equals ``step`` on the 32-sample
    batch -- the reference's own bar for this equivalence is 1e-4 (test_optimizer_acc.py:175).  Two steps on
    fresh batches; stated tolerance: initial losses 1e-5, learning rates / damping schedule / reasons identical,
    iteration counts +-2, final losses 1e-4, parameters after the first step 1e-4 of their max-norm.  The
    accumulated session serves both steps, and a second run of the same two calls is BITWISE equal."""
    acc, fa = _resnet_runs("acc", 2)
    sess = acc._acc_session
    # (eval-mode BatchNorm couples no samples and both chunks carry the weight 1 / 32 per sample: ONE engine on the
    # concatenated chunks -- acc_session.AccumulatedSession._merge_groups)
    assert sess is not None and sess.steps == 2 and len(sess.engines) == 1 and sess.groups == [[0, 1]]
    assert "engine" in sess.mode and "ONE batch" in sess.mode
    whole, fw = _resnet_runs("step", 2)
    assert whole._session is not None
    _same_trace(acc, fa, whole, fw)
    again, fa2 = _resnet_runs("acc", 2)
    assert fa2 == fa and torch.equal(_flat(again), _flat(acc))
    assert again.state["num_cg_iters"] == acc.state["num_cg_iters"]
    # ... and the reference's own ``acc_step`` on the same chunks (golden ``acc_16_16``), same tolerances
    from helpers import RefTrace, compare_trace

    ref = RefTrace("resnet18", "acc_16_16")
    compare_trace(acc.state, fa, ref)


def test_acc_step_on_engine_matches_reference_trace_with_ragged_chunks():
    """Chunks of unequal sizes [20, 12] (weights N_k / sum N, optimizer.py:677-684): two ``acc_step`` calls against
    the reference's own ``acc_step`` on the stock CPU model (golden ``acc_20_12``, cg_max_iter = 6).  Tolerances as
    above, except the SECOND step's final loss: it starts from parameters that differ like any two fp32 runs, and
    back-tracking / the line search pick between nearly tied candidates (measured: 2.22254 on the GPU -- the lower
    loss -- against 2.22289 / 2.22332 on CPUs, 3.5e-4): 1e-3."""
    from helpers import RefTrace, compare_trace

    ref = RefTrace("resnet18", "acc_20_12")
    acc, fa = _resnet_runs("acc", 2, sizes=(20, 12), cg_max_iter=6)
    assert acc._acc_session is not None and acc._acc_session.chunk_shapes[0][0] == 20
    assert acc._acc_session.shapes[0][0] == 32 and acc._acc_session.merged
    within(abs(fa[0] - ref.finals[0]), 1e-4 * abs(ref.finals[0]), strict=False)
    compare_trace(acc.state, fa, ref, final_tol=(1e-4, 1e-3))


def test_acc_product_gradient_and_loss_equal_generic_accumulation():
    """The session's accumulated loss / gradient / product against the generic ``_acc_*`` accumulation (autograd
    operators per chunk) on the same lists, with DISTINCT loss / gradient / curvature lists (README.md:147-150 of
    the reference): 1e-6 / 2e-6 / 2e-6 (max-norm relative), and the product is bitwise repeatable."""
    model, _, lossf = tp.resnet18_mnist(batch_size=32, device=DEV, data_seed=SEEDS[0])
    modelprep.prepare_model(model, channels_last=True)
    opt = hf.HessianFree(model.parameters(), graph_matvec=True)
    data = [tp.resnet18_mnist(batch_size=32, device=DEV, data_seed=SEEDS[i])[1] for i in range(3)]
    loss_dl = _chunks(*data[0], (16, 16))
    grad_dl = _chunks(*data[1], (12, 20))
    mvp_dl = _chunks(*data[2], (8, 8))  # (a smaller curvature batch: 16 of the 32 samples)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        forward, grad, mvp, sess = opt.acc_linearise(model, lossf, loss_dl, grad_dl, mvp_dl, "mean")
    # (six chunks, three lists: the two chunks of a list carry one per-sample weight and run as one batch -- three
    # engines of 32 / 32 / 16 samples on parallel graph branches)
    assert sess is not None and grad is None and mvp is None and len(sess.engines) == 3
    assert sess.groups == [[0, 1], [2, 3], [4, 5]] and [sh[0] for sh in sess.shapes] == [32, 32, 16]
    want_loss = float(opt._acc_loss(model, lossf, loss_dl, "mean"))
    within(abs(sess.base_loss - want_loss), 1e-6 * abs(want_loss), strict=False)
    want_grad = opt._acc_grad(model, lossf, grad_dl, "mean")
    got_grad = sess.gradient()
    within(float((got_grad - want_grad).abs().max() / want_grad.abs().max()), 2e-6)
    v = torch.randn(sess.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    want = opt._acc_mvp(model, lossf, mvp_dl, "ggn", "mean", v)
    got = sess(v).clone()
    within(float((got - want).abs().max() / want.abs().max()), 2e-6)
    assert torch.equal(sess(v), got)


def test_acc_step_allcnnc_hessian_with_l2_on_engine_equals_step():
    """BASELINE configs[3]'s model through ``acc_step``: All-CNN-C, Hessian curvature, tagged L2 term, chunks
    [16, 16] against ``step`` on the whole batch (both on the plain-stack engine): same tolerances."""
    runs = []
    for kind in ("acc", "step"):
        model, (x, t), lossf = tp.allcnnc_cifar100(batch_size=32, device=DEV, data_seed=7)
        lossf = tp.l2_regularized(lossf, model, 5e-4)
        modelprep.prepare_model(model, channels_last=True)
        opt = hf.HessianFree(model.parameters(), curvature_opt="hessian", graph_matvec=True, cg_max_iter=30)

        def forward():
            out = model(x)
            return lossf(out, t), out

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if kind == "acc":
                final = opt.acc_step(model, lossf, _chunks(x, t, (16, 16)), reduction="mean")
                assert opt._acc_session is not None and opt._acc_session.hessian
            else:
                final = opt.step(forward)
                assert opt._session is not None and opt._session.engine.hessian
        runs.append((opt, [final]))
    _same_trace(*runs[0], *runs[1])


def test_acc_step_falls_back_for_models_the_engine_does_not_cover():
    """An MLP with an MSE loss (the reference's own acc tests): no engine, the generic accumulation runs."""
    model, (x, t), lossf = tp.small_nn(device=DEV)
    opt = hf.HessianFree(model.parameters(), graph_matvec=True, cg_max_iter=5)
    with pytest.warns(UserWarning, match=r"graph_matvec=True\)\.acc_step\(\) runs on the slower path 'eager'.*not a prepared one"):
        opt.acc_step(model, lossf, _chunks(x, t, (16, 16)), reduction="mean")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        opt.acc_step(model, lossf, _chunks(x, t, (16, 16)), reduction="mean")
    assert not [w for w in rec if "slower path" in str(w.message)]  # (once per optimizer)
    assert opt._acc_session is None
    rep = opt.path_report()["acc_step"]
    assert rep["path"] == "eager" and "refused twice" in rep["declined"]
    # a prepared ResNet: another loss, a reduction the loss function does not have, chunks of different image size
    net, (xr, tr), ce = tp.resnet18_mnist(batch_size=8, device=DEV, data_seed=SEEDS[0])
    modelprep.prepare_model(net, channels_last=True)
    cases = [
        (torch.nn.CrossEntropyLoss(label_smoothing=0.1), "mean", _chunks(xr, tr, (4, 4)), "not a plain softmax cross-entropy"),
        (ce, "sum", _chunks(xr, tr, (4, 4)), "reduces by 'mean', acc_step was asked for reduction='sum'"),
        (ce, "mean", [(xr[:4].contiguous(), tr[:4].contiguous()),
                      (xr[4:, :, :20, :20].contiguous(), tr[4:].contiguous())], "differ in more than their batch size"),
    ]
    for lossf_c, reduction, chunks, text in cases:
        opt = hf.HessianFree(net.parameters(), graph_matvec=True, cg_max_iter=2)
        with pytest.warns(UserWarning, match=r"acc_step\(\) runs on the slower path"):
            opt.acc_step(net, lossf_c, chunks, reduction=reduction)
        assert text in opt.path_report()["acc_step"]["declined"], opt.path_report()
    opt = hf.HessianFree(net.parameters(), graph_matvec=True, cg_max_iter=2)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        opt.acc_step(net, ce, _chunks(xr, tr, (4, 4)), reduction="mean")
    assert not [w for w in rec if "slower path" in str(w.message)]
    assert opt.path_report()["acc_step"]["path"] == "acc-session" and opt.path_report()["acc_step"]["declined"] is None


def test_acc_step_train_mode_batchnorm_session_equals_generic_accumulation(monkeypatch):
    """TRAIN-mode BatchNorm through ``acc_step`` (the reference accumulates over chunks with the model as it is,
    optimizer.py:600-700: every chunk is normalised with ITS batch statistics): the accumulated session -- one
    train-mode engine per chunk, the chunks' sweeps in sequence (they move the same running statistics), loss /
    gradient / trial losses as replays -- against this package's generic accumulation (``HF_ACC_SESSION=0``: autograd
    operators per chunk) on the same model, chunks [16, 16], two calls on fresh batches.  Tolerances as for the
    train-mode session of ``step`` (tests/test_session_gpu.py): initial losses 1e-5 / 1e-3, first final loss 5e-4,
    the damping schedule identical, iteration counts +-2, every call reduces its batch's loss; the accumulated
    product against the generic accumulated product at the same point 2e-3 (two fp32 train-mode forward passes of
    this 20-layer net: DESIGN.md section 5), bitwise repeatable."""
    def run(session):
        monkeypatch.setenv("HF_ACC_SESSION", "1" if session else "0")
        model, _, lossf = tp.resnet18_mnist(batch_size=32, device=DEV, data_seed=SEEDS[0])
        model.train()
        modelprep.prepare_model(model, channels_last=True)
        opt = hf.HessianFree(model.parameters(), graph_matvec=True)
        finals = []
        for i in range(2):
            _, (x, t), _ = tp.resnet18_mnist(batch_size=32, device=DEV, data_seed=SEEDS[i])
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                finals.append(opt.acc_step(model, lossf, _chunks(x, t, (16, 16)), reduction="mean"))
        return opt, finals, model, lossf

    a, fa, model, lossf = run(True)
    sess = a._acc_session
    assert sess is not None and sess.train_bn and len(sess.engines) == 2 and sess.steps == 2
    assert all(e.train_bn and all(u.train for u in e.units) for e in sess.engines)
    b, fb, _, _ = run(False)
    assert b._acc_session is None
    ia, ib = a.state["init_losses"], b.state["init_losses"]
    assert abs(ia[0] - ib[0]) <= 1e-5 * abs(ib[0]) and abs(ia[1] - ib[1]) <= 1e-3 * abs(ib[1])
    within(abs(fa[0] - fb[0]), 5e-4 * abs(fb[0]), strict=False)
    assert a.state["dampings"] == b.state["dampings"]
    for x, y in zip(a.state["num_cg_iters"], b.state["num_cg_iters"]):
        within(abs(x - y), 2, strict=False)
    for f, i0 in zip(fa, ia):
        assert f < i0
    # the accumulated product of the session against the generic accumulation at the session's current point
    monkeypatch.setenv("HF_ACC_SESSION", "1")
    _, (x, t), _ = tp.resnet18_mnist(batch_size=32, device=DEV, data_seed=SEEDS[2])
    chunks = _chunks(x, t, (16, 16))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, _, _, s2 = a.acc_linearise(model, lossf, chunks, chunks, chunks, "mean")
    assert s2 is sess
    v = torch.randn(sess.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    got = sess(v).clone()
    assert torch.equal(sess(v), got)
    want = a._acc_mvp(model, lossf, chunks, "ggn", "mean", v)
    within(float((got - want).abs().max() / want.abs().max()), 2e-3)


def test_acc_step_train_mode_hessian_session_equals_generic_accumulation(monkeypatch):
    """``curvature_opt="hessian"`` with TRAIN-mode BatchNorm through ``acc_step``: one Hessian engine per chunk (the
    batch statistics' second-order terms by ``hf_bn_train_hessian_*``; every chunk normalised with ITS statistics, as
    the reference's accumulation does, optimizer.py:600-700) against this package's generic accumulation
    (``HF_ACC_SESSION=0``: ``curvature.HessianOperator`` per chunk), chunks [8, 8], one call: initial loss 1e-5, final
    loss 1e-3, same damping schedule and termination reason, iteration counts +-2; the accumulated product against
    the generic accumulated product at the same point 1e-4, bitwise repeatable.  (The product is taken right after
    ``acc_linearise``, which hands the gradient to ``step`` unevaluated: the session refreshes the first-order cotangents
    a Hessian product reads by itself.)"""
    def run(session):
        monkeypatch.setenv("HF_ACC_SESSION", "1" if session else "0")
        model, (x, t), lossf = tp.resnet18_mnist(batch_size=16, device=DEV, data_seed=5)
        model.train()
        modelprep.prepare_model(model, channels_last=True)
        opt = hf.HessianFree(model.parameters(), curvature_opt="hessian", graph_matvec=True, cg_max_iter=20)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            final = opt.acc_step(model, lossf, _chunks(x, t, (8, 8)), reduction="mean")
        return opt, final, model, lossf, (x, t)

    a, fa, model, lossf, (x, t) = run(True)
    sess = a._acc_session
    assert sess is not None and sess.train_bn and len(sess.engines) == 2
    assert all(e.hessian and e.train_bn for e in sess.engines)
    b, fb, _, _, _ = run(False)
    assert b._acc_session is None
    within(abs(a.state["init_losses"][0] - b.state["init_losses"][0]), 1e-5 * abs(b.state["init_losses"][0]), strict=False)
    assert a.state["dampings"] == b.state["dampings"] and a.state["cg_reasons"] == b.state["cg_reasons"]
    within(abs(a.state["num_cg_iters"][0] - b.state["num_cg_iters"][0]), 2, strict=False)
    within(abs(fa - fb), 1e-3 * abs(fb), strict=False)
    assert fa < a.state["init_losses"][0]
    monkeypatch.setenv("HF_ACC_SESSION", "1")
    chunks = _chunks(x, t, (8, 8))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, _, _, s2 = a.acc_linearise(model, lossf, chunks, chunks, chunks, "mean")
    assert s2 is sess
    v = torch.randn(sess.n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    got = sess(v).clone()
    assert torch.equal(sess(v), got)
    want = a._acc_mvp(model, lossf, chunks, "hessian", "mean", v)
    within(float((got - want).abs().max() / want.abs().max()), 1e-4)  # (9.8e-6 measured)


def test_acc_step_with_mse_loss_on_engine_equals_step_on_whole_batch():
    """``acc_step`` under the loss of the reference's own acc tests (``nn.MSELoss``, tests/test_optimizer_acc.py:47-60)
    on the engine: chunks [20, 12] of float targets merge into one engine batch and equal ``step`` on the 32-sample
    batch (the reference's bar for this equivalence: 1e-4, test_optimizer_acc.py:175); reduction ``sum`` likewise."""
    for reduction in ("mean", "sum"):
        runs = []
        for kind in ("acc", "step"):
            model, (x, t), _ = tp.resnet18_mnist_mse(batch_size=32, device=DEV, data_seed=SEEDS[0])
            lossf = torch.nn.MSELoss(reduction=reduction)
            modelprep.prepare_model(model, channels_last=True)
            opt = hf.HessianFree(model.parameters(), graph_matvec=True, cg_max_iter=10)

            def forward():
                out = model(x)
                return lossf(out, t), out

            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                if kind == "acc":
                    final = opt.acc_step(model, lossf, _chunks(x, t, (20, 12)), reduction=reduction)
                    sess = opt._acc_session
                    assert sess is not None and sess.merged and sess.engines[0].loss_spec["kind"] == "mse"
                else:
                    final = opt.step(forward)
                    assert opt._session is not None
            runs.append((opt, [final]))
        _same_trace(*runs[0], *runs[1])


def test_acc_step_with_mse_loss_matches_reference_trace_with_ragged_chunks():
    """``acc_step`` under ``nn.MSELoss`` on ragged chunks [20, 12] against the REAL reference's ``acc_step`` on the
    stock CPU model (golden ``convnet_resnet18_mse.npz``, ``acc_20_12``, cg_max_iter = 6): the chunks merge into one
    engine batch; the tolerances of the cross-entropy trace."""
    from helpers import RefTrace, compare_trace

    ref = RefTrace("resnet18_mse", "acc_20_12")
    model, _, lossf = tp.resnet18_mnist_mse(batch_size=32, device="cpu", data_seed=SEEDS[0])
    ref.check_inputs([p for p in model.parameters() if p.requires_grad])
    model = model.to(DEV)
    modelprep.prepare_model(model, channels_last=True)
    opt = hf.HessianFree(model.parameters(), graph_matvec=True, cg_max_iter=6)
    finals = []
    for i in range(2):
        _, (x, t), _ = tp.resnet18_mnist_mse(batch_size=32, device="cpu", data_seed=SEEDS[i])
        ref.check_inputs(x=x, step=i)
        x, t = x.to(DEV), t.to(DEV)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            finals.append(opt.acc_step(model, lossf, _chunks(x, t, (20, 12)), reduction="mean"))
    sess = opt._acc_session
    assert sess is not None and sess.merged and sess.steps == 2 and sess.engines[0].loss_spec["kind"] == "mse"
    compare_trace(opt.state, finals, ref, final_tol=(1e-4, 1e-3))


def test_acc_step_with_frozen_layers_matches_reference_whole_batch_step():
    """``acc_step`` on a model with frozen layers (stem + layer1): chunks [16, 16] merge into one engine batch on the
    trainable subset; the accumulated step equals the REAL reference's whole-batch ``step`` on the frozen model (golden
    ``convnet_resnet18_frozen.npz``, ``steps``; the reference states accumulated == whole batch to 1e-4,
    tests/test_optimizer_acc.py:116-175) -- two steps, the tolerances of the unfrozen trace."""
    from helpers import RefTrace, compare_trace

    ref = RefTrace("resnet18_frozen", "steps")
    model, _, lossf = tp.resnet18_mnist(batch_size=32, device="cpu", data_seed=SEEDS[0])
    tp.freeze_stem_and_layer1(model)
    ref.check_inputs([p for p in model.parameters() if p.requires_grad])
    model = model.to(DEV)
    modelprep.prepare_model(model, channels_last=True)
    opt = hf.HessianFree(model.parameters(), graph_matvec=True)
    finals = []
    for i in range(2):
        _, (x, t), _ = tp.resnet18_mnist(batch_size=32, device="cpu", data_seed=SEEDS[i])
        ref.check_inputs(x=x, step=i)
        x, t = x.to(DEV), t.to(DEV)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            finals.append(opt.acc_step(model, lossf, _chunks(x, t, (16, 16)), reduction="mean"))
    sess = opt._acc_session
    assert sess is not None and sess.merged and sess.steps == 2 and sess.engines[0].frozen_any
    assert sess.engines[0].dead_blocks == 2 and sess.n == 11024138
    compare_trace(opt.state, finals, ref, steps=2)
