"""The cases of the accumulated session's value tests -- list structures, nets, losses, data -- shared by the test that
checks the cases' input conditions without a GPU (tests/test_acc_refs_cpu.py) and the one that runs them on the session
(tests/test_acc_session_quantities_gpu.py).

List structures on 8x8 inputs: per structure the chunk sizes by letter (a letter is ONE pair of tensors) and the loss /
gradient / curvature list.  S1-S6 are the issue's; S7 is the one in which the trial points' forward graph differs from
the step's while the lists overlap (its loss list is a proper subset of the engines)."""

from collections import namedtuple

import torch
from torch import nn

from pytorchhessianfree_amd import testproblems as tp

STRUCTURES = {
    "S1": (dict(a=4, b=4), ("ab", "ab", "ab")),
    "S2": (dict(a=5, b=3), ("ab", "ab", "ab")),
    "S3": (dict(a=4, b=4), ("aab", "ab", "ab")),
    "S4": (dict(a=4, b=4, c=3, d=5, e=2, f=2), ("ab", "cd", "ef")),
    "S5": (dict(a=4, b=4), ("ab", "ab", "a")),
    "S6": (dict(a=4, b=4), ("ab", "a", "b")),
    "S7": (dict(a=4, b=4), ("a", "ab", "ab")),
}
# what the session makes of them for a model that couples no samples: groups of distinct chunks (numbered in order of
# first appearance over the three lists), one engine per group
EVAL_GROUPS = {"S1": [[0, 1]], "S2": [[0, 1]], "S3": [[0], [1]], "S4": [[0, 1], [2, 3], [4, 5]], "S5": [[0], [1]],
               "S6": [[0], [1]], "S7": [[0], [1]]}
WEIGHTED = {"S2": 0, "S3": 0, "S4": 1}  # (structure: a list whose chunks carry unequal weights under ``mean``)
# (5e-2 leaves the regulariser's (K-1) share of the plain stack's gradient at 0.5 %: four times that, test_acc_refs_cpu.py)
L2 = 0.2
CLASSES = {"resnet": 10, "plain": 12}
CHANNELS = {"resnet": 1, "plain": 3}

Case = namedtuple("Case", "net train structure reduction curvature loss")


def _matrix():
    both = ("mean", "sum")
    cases = [Case("resnet", False, s, r, "ggn", "ce") for s in STRUCTURES for r in both]
    cases += [Case("resnet", False, s, r, "hessian", "ce") for s in ("S1", "S4", "S5", "S6") for r in both]
    cases += [Case("resnet", False, s, r, c, "ce_l2") for c in ("ggn", "hessian") for s in ("S1", "S2", "S3") for r in both]
    cases += [Case("plain", False, s, r, "hessian", "ce_l2") for s in ("S1", "S2", "S3") for r in both]
    cases += [Case("resnet", False, s, r, "ggn", "mse") for s in ("S2", "S4") for r in both]
    cases += [Case("resnet", True, s, r, "ggn", "ce") for s in ("S1", "S3") for r in both]
    cases += [Case("resnet", True, "S1", "mean", "hessian", "ce")]
    return cases


CASES = _matrix()


def case_id(c):
    return "-".join([c.net, "train" if c.train else "eval", c.structure, c.reduction, c.curvature, c.loss])


# Data seeds.  A case's data must keep every ReLU input of the float64 model further than 1e-5 from zero, on every chunk
# and at the trial point (test_acc_refs_cpu.py asserts it): seed 0 unless listed here.
SEEDS = {("resnet", False, "S1", "ce"): 7, ("resnet", False, "S3", "ce"): 7, ("resnet", False, "S4", "ce"): 30,
         ("resnet", False, "S5", "ce"): 7, ("resnet", False, "S6", "ce"): 7, ("resnet", False, "S7", "ce"): 7,
         ("resnet", False, "S1", "ce_l2"): 7, ("resnet", False, "S3", "ce_l2"): 7, ("plain", False, "S1", "ce_l2"): 12,
         ("plain", False, "S3", "ce_l2"): 12, ("resnet", False, "S2", "mse"): 5, ("resnet", False, "S4", "mse"): 34}
REUSE_SEED = 18  # (the fresh S1 data of the reuse test: holds the margin in eval and in train mode)


def data_seed(c):
    return SEEDS.get((c.net, c.train, c.structure, c.loss), 0)


def chunks(c, seed=None, device="cpu"):
    """``{letter: (inputs, targets)}`` of a case: normal inputs ``[n, C, 8, 8]``, class indices or (``mse``) normal float
    targets ``[n, 10]``."""
    g = torch.Generator().manual_seed(1000 + (data_seed(c) if seed is None else seed))
    out = {}
    for letter, n in STRUCTURES[c.structure][0].items():
        x = torch.randn(n, CHANNELS[c.net], 8, 8, generator=g)
        if c.loss == "mse":
            t = torch.randn(n, CLASSES[c.net], generator=g)
        else:
            t = torch.randint(0, CLASSES[c.net], (n,), generator=g)
        out[letter] = (x.to(device), t.to(device))
    return out


def lists(c, data):
    """The three data lists over the SAME tensor pairs (the session tells chunks apart by identity)."""
    return tuple([data[letter] for letter in names] for names in STRUCTURES[c.structure][1])


def loss_function(c, model):
    base = nn.MSELoss(reduction=c.reduction) if c.loss == "mse" else nn.CrossEntropyLoss(reduction=c.reduction)
    return tp.l2_regularized(base, model, L2) if c.loss == "ce_l2" else base


def vectors(n, seed=3):
    """The product's vector and the trial step, fp32 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g), 0.02 * torch.randn(n, generator=g)


def trial_point(params, delta):
    """``theta + delta`` rounded as fp32 rounds it, per parameter, and the float64 difference to ``theta`` that a
    float64 model must add to land on exactly that point."""
    theta = torch.cat([p.detach().reshape(-1).cpu().float() for p in params])
    new = theta + delta
    return new, new.double() - theta.double()
