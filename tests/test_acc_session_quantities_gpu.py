"""GPU: the QUANTITIES the accumulated session (``acc_session.AccumulatedSession``) hands to ``acc_step`` -- loss, gradient,
curvature product and trial loss -- against the float64 reference of tests/acc_refs.py (plain autograd on the CPU, stock
model, the loss function called once per chunk occurrence), for every list structure the session plans differently:
merged chunks, ragged chunks, a chunk listed twice, three distinct lists, overlapping lists, a one-chunk gradient list
with a trailing engine, each under ``mean`` and ``sum``.  The cases and their data are tests/acc_cases.py's; their input
conditions (ReLU margins, the regulariser's share, unequal weights) are asserted in tests/test_acc_refs_cpu.py.

Per case: the session exists and has the expected structure; the four quantities match the reference in max-norm
relative error; a product is bitwise repeatable, and the product taken BEFORE ``gradient()`` (a Hessian session then
refreshes its first-order cotangents itself) is bitwise the one taken after it.

Structures (acc_cases.STRUCTURES).  S5 (loss a b | gradient a b | curvature a) has both engines in its loss list, so its
trial points replay the step's forward graph; the structure whose trial points replay a smaller graph of their own while
the lists overlap is S7 (loss a | gradient a b | curvature a b), added to the issue's six; S4's trial graph is its own too.
No case was declined by the engine at these sizes.

Bounds.  Eval mode: 1e-5 for all four quantities, the package's engine-against-oracle bound
(test_resnet18_engine_product_matches_cpu_oracle_at_batch_32); every defect the matrix is built to catch is at least
1 % (test_acc_refs_cpu.py).  Train-mode BatchNorm: this package's generic fp32 accumulation (``_acc_loss`` / ``_acc_grad``
/ ``_acc_mvp``: autograd per chunk) is measured against the same float64 reference on the same case, and the session may
be 4x as far away (two independent fp32 forward passes), never held to less than 1e-5.  Measured values per case and
quantity: profiles/r24_acc_quantities.jsonl (each test prints its line, marked ``ACCQ``, before it asserts)."""

import json
import warnings

import acc_cases as ac
import acc_refs
import engine_nets as en
import pytest
import torch

import pytorchhessianfree_amd as hf

pytestmark = pytest.mark.gpu
DEV = "cuda"
EVAL_BOUND = 1e-5
QUANTITIES = ("loss", "grad", "product", "trial_loss")


def _rel(got, want):
    got = torch.as_tensor(got, dtype=torch.float64).cpu()
    want = torch.as_tensor(want, dtype=torch.float64)
    return float((got - want).abs().max() / want.abs().max())


def _to_dev(data):
    return {k: (x.to(DEV), t.to(DEV)) for k, (x, t) in data.items()}


def _set_params(params, flat):
    o = 0
    with torch.no_grad():
        for p in params:
            p.copy_(flat[o:o + p.numel()].reshape(p.shape))
            o += p.numel()


def _linearise(opt, model, lossf, lists, reduction):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, grad, mvp, sess = opt.acc_linearise(model, lossf, *lists, reduction)
    assert sess is not None and grad is None and mvp is None, opt.path_report()["acc_step"]
    return sess


def _expect_structure(sess, case):
    if case.train:
        distinct = len(ac.STRUCTURES[case.structure][0])
        groups = [[k] for k in range(distinct)]
    else:
        groups = ac.EVAL_GROUPS[case.structure]
    assert sess.groups == groups
    assert len(sess.engines) == len(groups)
    assert sess.merged == any(len(g) > 1 for g in groups)
    assert sess.parallel == (len(groups) > 1 and not case.train)
    assert sess.train_bn == case.train
    assert sess.hessian == (case.curvature == "hessian") and all(e.hessian == sess.hessian for e in sess.engines)
    # (trial points: the loss list's engines only -- a graph of its own where that is not every engine)
    assert (sess.g_fwd is not sess.g_fwd_all) == (case.structure in ("S4", "S7"))
    if case.net == "plain":
        from pytorchhessianfree_amd.engine import PlainStackEngine

        assert all(isinstance(e, PlainStackEngine) for e in sess.engines)


def _session_quantities(sess, opt, v, delta):
    """``(loss, gradient, product, trial loss)`` of the session at its current data, the repeatability checks on the way;
    the parameters are back at their values afterwards.  Also the fp32 trial point and its float64 step."""
    got = {"loss": sess.base_loss}
    before = sess(v).clone()  # (before gradient(): a Hessian session replays its first-order sweep itself)
    got["grad"] = sess.gradient().clone()
    got["product"] = sess(v).clone()
    assert torch.equal(got["product"], before)
    assert torch.equal(sess(v), got["product"])
    params = opt._params_list
    theta = torch.cat([p.detach().reshape(-1) for p in params]).clone()
    new, delta64 = ac.trial_point(params, delta)
    _set_params(params, new.to(DEV))
    try:
        got["trial_loss"] = float(sess.forward_loss(1))
    finally:
        _set_params(params, theta)
    return got, new, delta64


def _generic_quantities(opt, model, lossf, lists, case, v, new):
    """The same four by this package's generic fp32 accumulation (autograd per chunk)."""
    params = opt._params_list
    theta = torch.cat([p.detach().reshape(-1) for p in params]).clone()
    out = {"loss": float(opt._acc_loss(model, lossf, lists[0], case.reduction)),
           "grad": opt._acc_grad(model, lossf, lists[1], case.reduction).clone(),
           "product": opt._acc_mvp(model, lossf, lists[2], case.curvature, case.reduction, v).clone()}
    _set_params(params, new.to(DEV))
    try:
        out["trial_loss"] = float(opt._acc_loss(model, lossf, lists[0], case.reduction))
    finally:
        _set_params(params, theta)
    return out


def _check(name, sess, opt, model, twin, lossf, lossf64, case, data, gdata):
    """Session against reference on one data set; prints the figures, then asserts."""
    v, delta = ac.vectors(sess.n)
    assert sess.n == sum(p.numel() for p in twin.parameters() if p.requires_grad)
    glists = ac.lists(case, gdata)
    got, new, delta64 = _session_quantities(sess, opt, v.to(DEV), delta)
    want = acc_refs.accumulate(twin, lossf64, *ac.lists(case, data), case.reduction, case.curvature, v, delta64)
    errs = {q: _rel(got[q], want[q]) for q in QUANTITIES}
    record = {"case": name, "engines": len(sess.engines), "groups": sess.groups, "session": errs}
    bounds = dict.fromkeys(QUANTITIES, EVAL_BOUND)
    if case.train:
        generic = _generic_quantities(opt, model, lossf, glists, case, v.to(DEV), new)
        record["generic"] = {q: _rel(generic[q], want[q]) for q in QUANTITIES}
        bounds = {q: max(4.0 * record["generic"][q], EVAL_BOUND) for q in QUANTITIES}
    record["bounds"] = bounds
    print("ACCQ " + json.dumps(record))
    for q in QUANTITIES:
        assert errs[q] < bounds[q], (name, q, errs[q], bounds[q])


def _setup(case):
    _, twin, model = en.three_forms(case.net, train=case.train)
    lossf, lossf64 = ac.loss_function(case, model), ac.loss_function(case, twin)
    opt = hf.HessianFree(model.parameters(), curvature_opt=case.curvature, graph_matvec=True)
    return twin, model, lossf, lossf64, opt


@pytest.mark.parametrize("case", ac.CASES, ids=ac.case_id)
def test_session_quantities_match_float64_reference(case):
    twin, model, lossf, lossf64, opt = _setup(case)
    data = ac.chunks(case)
    gdata = _to_dev(data)
    sess = _linearise(opt, model, lossf, ac.lists(case, gdata), case.reduction)
    _expect_structure(sess, case)
    _check(ac.case_id(case), sess, opt, model, twin, lossf, lossf64, case, data, gdata)


def test_session_is_reused_on_fresh_data_and_rebuilt_when_the_model_changes_mode_float64_reference():
    """S1, ``mean``, GGN: a second call with fresh data of the same shapes gets the SAME session, which matches the
    reference on the new data; after ``model.train()`` a new session is built, one engine per chunk, and matches the
    train-mode reference within the train-mode bound."""
    case = ac.Case("resnet", False, "S1", "mean", "ggn", "ce")
    twin, model, lossf, lossf64, opt = _setup(case)
    first = _linearise(opt, model, lossf, ac.lists(case, _to_dev(ac.chunks(case))), case.reduction)
    _expect_structure(first, case)
    data = ac.chunks(case, seed=ac.REUSE_SEED)
    gdata = _to_dev(data)
    sess = _linearise(opt, model, lossf, ac.lists(case, gdata), case.reduction)
    assert sess is first and sess.steps == 2
    _check("reuse-fresh-data", sess, opt, model, twin, lossf, lossf64, case, data, gdata)
    model.train()
    twin.train()
    case = case._replace(train=True)
    sess = _linearise(opt, model, lossf, ac.lists(case, gdata), case.reduction)
    assert sess is not first and sess.steps == 1
    _expect_structure(sess, case)
    _check("reuse-then-train-mode", sess, opt, model, twin, lossf, lossf64, case, data, gdata)
