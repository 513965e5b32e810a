"""CPU: the float64 reference of the accumulated quantities (tests/acc_refs.py) anchored against what it must equal by
definition, and the input conditions of every case of tests/test_acc_session_quantities_gpu.py, asserted here so that
the GPU test can rely on them.  Errors are max-norm relative; the 1e-12 bounds are float64 rounding of sums of a few
thousand terms (1e-16 each) with room for cancellation."""

import acc_cases as ac
import acc_refs
import engine_nets as en
import pytest
import torch
from torch import nn

from pytorchhessianfree_amd import testproblems as tp


def _rel(got, want):
    got, want = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(want, dtype=torch.float64)
    return float((got - want).abs().max() / want.abs().max())


def _data(sizes, classes=10, channels=1, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, channels, 8, 8, generator=g), torch.randint(0, classes, (n,), generator=g)) for n in sizes]


def _whole(dl):
    return [(torch.cat([x for x, _ in dl]), torch.cat([t for _, t in dl]))]


def _both(twin, lossf, dl, reduction, v):
    out = {}
    for curv in ("ggn", "hessian"):
        res = acc_refs.accumulate(twin, lossf, dl, dl, dl, reduction, curv, v)
        out.update(loss=res["loss"], grad=res["grad"])
        out[curv] = res["product"]
    return out


def _weight_mask(model):
    """1 on the flat vector's entries that ``testproblems.l2_regularized`` regularises (everything but the biases)."""
    return torch.cat([torch.full((p.numel(),), float("bias" not in name), dtype=torch.float64)
                      for name, p in model.named_parameters() if p.requires_grad])


def test_mean_accumulation_over_ragged_chunks_equals_the_whole_batch():
    """Eval mode couples no samples: the ``mean`` accumulation over chunks [5, 3] is the whole batch of 8, for loss,
    gradient, GGN and Hessian product: 1e-12."""
    _, twin, _ = en.three_forms("resnet", prepared=False)
    dl = _data((5, 3))
    n = sum(p.numel() for p in twin.parameters())
    v, _ = ac.vectors(n)
    lossf = nn.CrossEntropyLoss()
    acc, whole = _both(twin, lossf, dl, "mean", v), _both(twin, lossf, _whole(dl), "mean", v)
    for key in ("loss", "grad", "ggn", "hessian"):
        assert _rel(acc[key], whole[key]) < 1e-12, key


@pytest.mark.parametrize("names", ["ab", "aab"])
def test_sum_accumulation_counts_the_regulariser_once_per_chunk_occurrence(names):
    """``sum`` with ``l2_regularized`` over K chunk occurrences: the user's loss function is called once per occurrence,
    so the accumulation exceeds the whole batch by exactly ``(K-1) R``, ``(K-1) l2 theta_w`` and, for the Hessian
    product, ``(K-1) l2 v_w`` (nothing for the GGN): 1e-12.  This is what the session must compute."""
    _, twin, _ = en.three_forms("resnet", prepared=False)
    a, b = _data((5, 3))
    dl = [dict(a=a, b=b)[letter] for letter in names]
    k = len(dl)
    n = sum(p.numel() for p in twin.parameters())
    v, _ = ac.vectors(n)
    lossf = tp.l2_regularized(nn.CrossEntropyLoss(reduction="sum"), twin, ac.L2)
    acc, whole = _both(twin, lossf, dl, "sum", v), _both(twin, lossf, _whole(dl), "sum", v)
    mask = _weight_mask(twin)
    theta = torch.cat([p.detach().reshape(-1) for p in twin.parameters()])
    reg = 0.5 * ac.L2 * float((mask * theta * theta).sum())
    assert reg > 0
    assert abs(acc["loss"] - whole["loss"] - (k - 1) * reg) < 1e-12 * abs(acc["loss"])
    assert _rel(acc["grad"] - whole["grad"], (k - 1) * ac.L2 * mask * theta) < 1e-12 * k
    assert _rel(acc["hessian"] - whole["hessian"], (k - 1) * ac.L2 * mask * v.double()) < 1e-12 * k
    assert _rel(acc["ggn"], whole["ggn"]) < 1e-12


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("loss", ["ce", "mse"])
def test_ggn_by_double_backward_equals_the_materialised_jacobian(loss, reduction):
    """``J^T H_L J v`` of the reference against the explicit product with the Jacobian of ``SmallConvStack``'s 48 outputs
    (4 samples, one backward pass per output) and autograd's own Hessian of the loss with respect to the outputs: 1e-12;
    and against ``oracle.backpack_restated`` (loss Hessian by double backward): 1e-12."""
    from oracle import backpack_restated as bp

    _, twin, _ = en.three_forms("plain", prepared=False)
    ((x, t),) = _data((4,), classes=12, channels=3)
    x = x.double()
    t = torch.randn(4, 12, dtype=torch.float64, generator=torch.Generator().manual_seed(2)) if loss == "mse" else t
    lossf = nn.MSELoss(reduction=reduction) if loss == "mse" else nn.CrossEntropyLoss(reduction=reduction)
    params = list(twin.parameters())
    n = sum(p.numel() for p in params)
    v, _ = ac.vectors(n)
    got = acc_refs.accumulate(twin, lossf, [(x, t)], [(x, t)], [(x, t)], reduction, "ggn", v)["product"]
    out = twin(x)
    jac = torch.stack([torch.cat([g.reshape(-1) for g in torch.autograd.grad(o, params, retain_graph=True)])
                       for o in out.reshape(-1)])
    free = out.detach().clone().requires_grad_(True)
    h = torch.autograd.functional.hessian(lambda o: lossf(o, t), free).reshape(out.numel(), out.numel())
    want = jac.t() @ (h @ (jac @ v.double()))
    assert _rel(got, want) < 1e-12
    vs = acc_refs._split(v.double(), params)
    oracle = torch.cat([g.reshape(-1) for g in bp.ggn_vector_product_from_plist(lossf(out, t), out, params, vs)])
    assert _rel(got, oracle) < 1e-12


def test_train_mode_batchnorm_chunks_are_normalised_with_their_own_statistics():
    """Train-mode BatchNorm: the accumulation over [4, 4] is NOT the whole batch of 8 -- the reference runs the model as
    it is, chunk by chunk (more than 1e-3 apart in every quantity)."""
    _, twin, _ = en.three_forms("resnet", train=True, prepared=False)
    dl = _data((4, 4))
    n = sum(p.numel() for p in twin.parameters())
    v, _ = ac.vectors(n)
    lossf = nn.CrossEntropyLoss()
    acc, whole = _both(twin, lossf, dl, "mean", v), _both(twin, lossf, _whole(dl), "mean", v)
    for key in ("loss", "grad", "ggn", "hessian"):
        assert _rel(acc[key], whole[key]) > 1e-3, key


def test_the_matrix_holds_every_case_the_issue_lists():
    ids = [ac.case_id(c) for c in ac.CASES]
    assert len(set(ids)) == len(ids) == 14 + 8 + 12 + 6 + 4 + 5
    assert ac.Case("resnet", False, "S6", "sum", "hessian", "ce") in ac.CASES
    assert ac.Case("plain", False, "S3", "sum", "hessian", "ce_l2") in ac.CASES
    assert ac.Case("resnet", True, "S1", "mean", "hessian", "ce") in ac.CASES


@pytest.mark.parametrize("case", ac.CASES, ids=ac.case_id)
def test_case_inputs_can_show_what_the_case_is_for(case):
    """Per case of the GPU matrix: (1) no ReLU input of the float64 model within 1e-5 of zero, on any chunk, at the
    linearisation point and at the trial point -- fp32 cannot flip one; (2) ``sum`` with the regulariser: the ``(K-1)``
    term of each list is at least 1 % of the max-norm of the loss, of the gradient and of the Hessian product -- the
    1e-5 bound sees a miscounted regulariser a thousand times over; (3) weighted structures: the smallest chunk weight
    of the named list is at least 10 % off the uniform weight; (4) the trial point's loss is another loss, by more than
    1e-3."""
    _, twin, _ = en.three_forms(case.net, train=case.train, prepared=False)
    data = ac.chunks(case)
    params = [p for p in twin.parameters() if p.requires_grad]
    n = sum(p.numel() for p in params)
    v, delta = ac.vectors(n)
    _, delta64 = ac.trial_point(params, delta)
    margins = [tp.relu_margin(twin, x.double()) for x, _ in data.values()]
    with torch.no_grad():
        for p, d in zip(params, acc_refs._split(delta64, params)):
            p.add_(d)
    margins += [tp.relu_margin(twin, x.double()) for x, _ in data.values()]
    with torch.no_grad():
        for p, d in zip(params, acc_refs._split(delta64, params)):
            p.sub_(d)
    assert min(margins) > 1e-5, margins
    sizes, names = ac.STRUCTURES[case.structure]
    lossf = ac.loss_function(case, twin)
    ref = acc_refs.accumulate(twin, lossf, *ac.lists(case, data), case.reduction, case.curvature, v, delta64)
    assert abs(ref["trial_loss"] - ref["loss"]) > 1e-3 * abs(ref["loss"])  # (a hundred times the GPU test's bound)
    if case.structure in ac.WEIGHTED:
        role = names[ac.WEIGHTED[case.structure]]
        total = sum(sizes[letter] for letter in role)
        weights = [sum(sizes[x] for x in role if x == letter) / total for letter in dict.fromkeys(role)]
        assert min(weights) <= 0.9 / len(weights), weights
    if case.loss == "ce_l2" and case.reduction == "sum":
        mask = _weight_mask(twin)
        theta = torch.cat([p.detach().reshape(-1) for p in params])
        reg = 0.5 * ac.L2 * float((mask * theta * theta).sum())
        k = [len(role) for role in names]
        assert min(k) >= 2
        assert (k[0] - 1) * reg >= 0.01 * abs(ref["loss"])
        assert (k[1] - 1) * ac.L2 * float((mask * theta).abs().max()) >= 0.01 * float(ref["grad"].abs().max())
        if case.curvature == "hessian":
            assert (k[2] - 1) * ac.L2 * float((mask * v.double()).abs().max()) >= 0.01 * float(ref["product"].abs().max())


@pytest.mark.parametrize("train", [False, True])
def test_reuse_data_keeps_the_relu_margin_in_both_modes(train):
    """The fresh S1 data of the GPU reuse test (``acc_cases.REUSE_SEED``), on the eval-mode and on the train-mode model."""
    case = ac.Case("resnet", train, "S1", "mean", "ggn", "ce")
    _, twin, _ = en.three_forms("resnet", train=train, prepared=False)
    params = list(twin.parameters())
    _, delta = ac.vectors(sum(p.numel() for p in params))
    _, delta64 = ac.trial_point(params, delta)
    data = ac.chunks(case, seed=ac.REUSE_SEED)
    margins = [tp.relu_margin(twin, x.double()) for x, _ in data.values()]
    with torch.no_grad():
        for p, d in zip(params, acc_refs._split(delta64, params)):
            p.add_(d)
    margins += [tp.relu_margin(twin, x.double()) for x, _ in data.values()]
    assert min(margins) > 1e-5, margins
