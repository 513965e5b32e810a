"""GPU: the launch sequence of the dense-stack engine (``engine/dense.py``) -- which ``hf_*`` entry points one call of
``local(v)``, ``gradient(out)``, ``gradient()``, ``diag_ef("mean")`` and ``forward_own()`` issues, in which order.  The
products are captured into hipGraphs: the sequence IS the graph, and the docstring's "5 launches per hidden layer" / "at
most 4 launches per live layer" are read off it.

``_lib.load`` is replaced by a function that returns a proxy around the real library; the proxy forwards every call and
notes the name of every ``hf_*`` function called (``stack_harness.record_launches``).  Recording starts after the engine
is built.

Nets (``engine_nets.net_and_loss``): ``Linear(7,5) ReLU Linear(5,5) Tanh Linear(5,3)``, 3 rows, seeded on the CPU, a mean cross-entropy unless stated:
A all trainable; B layer 0 frozen (dead, layer 1 is the first live one); C layer 1's weight frozen, its bias trainable;
D layer 0's weight frozen, its bias trainable (the first live layer carries only a bias tangent); E net A with a mean
MSE.  Each as a GGN engine, a Hessian engine (``HF_DENSE_HESSIAN=1``) and a GGN engine in session mode
(``HF_DENSE_SESSION=1``).

The expected sequences below are written per layer (``|`` between layers, the tangent sweep in layer order, the adjoint
sweeps in reverse) from two rules.  Tangent sweep, per live layer: ``hf_dense_tangent_slabs`` unless the layer has neither
an input tangent nor a trainable weight, then ``hf_dense_act_tangent``; after the last layer ``hf_softmax_ce_hvp`` for a
cross-entropy.  Adjoint sweep, per live layer: the activation adjoint (``gradient()`` of a Hessian engine first keeps
``h_l`` of a tanh layer by an identity ``hf_dense_act_adjoint``; a Hessian product takes ``hf_dense_act_adjoint2`` on a tanh
layer), the weight output where the weight is trainable (``hf_dense_wgrad2`` in a Hessian product where the layer has an
input tangent; ``hf_dense_sq_wgrad`` in ``diag_ef``; none in ``gradient()`` without ``out``), in ``diag_ef`` the bias output
``hf_dense_sq_colsum`` where the bias is trainable, and the data gradient unless the layer is the first live one
(``hf_dense_dgrad2_slabs`` in a Hessian product where the weight is trainable)."""

import pytest
import torch

from engine_nets import DEV, DENSE_FROZEN as FROZEN, net_and_loss
from pytorchhessianfree_amd.engine import FusedGGNEngine
from pytorchhessianfree_amd.engine.dense import DenseStackEngine
from stack_harness import record_launches

pytestmark = pytest.mark.gpu

SHORT = {"T": "hf_dense_tangent_slabs", "AT": "hf_dense_act_tangent", "ce": "hf_softmax_ce_hvp",
         "aa": "hf_dense_act_adjoint", "aa2": "hf_dense_act_adjoint2", "w": "hf_dense_wgrad", "w2": "hf_dense_wgrad2",
         "d": "hf_dense_dgrad_slabs", "d2": "hf_dense_dgrad2_slabs", "sqw": "hf_dense_sq_wgrad",
         "sqc": "hf_dense_sq_colsum", "af": "hf_dense_act_forward", "lh": "hf_dense_loss_head"}

# local: the product of a GGN / a Hessian engine; grad_out, grad: gradient(out) / gradient() of a Hessian engine (keeps
# h_l of the tanh layer) and of a session-mode GGN engine; diag, forward: the same for every kind (session mode appends
# the loss head to forward)
_A = dict(local_ggn="T AT | T AT | T AT | ce | aa w d | aa w d | aa w",
          local_hessian="T AT | T AT | T AT | ce | aa w2 d2 | aa2 w2 d2 | aa w",
          grad_out_hessian="aa w d | aa aa w d | aa w", grad_hessian="aa d | aa aa d | aa",
          grad_out_ggn="aa w d | aa w d | aa w", grad_ggn="aa d | aa d | aa",
          diag="aa sqw sqc d | aa sqw sqc d | aa sqw sqc", forward="T af | T af | T af")
EXPECTED = {
    "A": _A,
    "B": dict(local_ggn="T AT | T AT | ce | aa w d | aa w",
              local_hessian="T AT | T AT | ce | aa w2 d2 | aa2 w",
              grad_out_hessian="aa w d | aa aa w", grad_hessian="aa d | aa aa",
              grad_out_ggn="aa w d | aa w", grad_ggn="aa d | aa",
              diag="aa sqw sqc d | aa sqw sqc", forward="T af | T af | T af"),
    "C": dict(local_ggn="T AT | T AT | T AT | ce | aa w d | aa d | aa w",
              local_hessian="T AT | T AT | T AT | ce | aa w2 d2 | aa2 d | aa w",
              grad_out_hessian="aa w d | aa aa d | aa w", grad_hessian="aa d | aa aa d | aa",
              grad_out_ggn="aa w d | aa d | aa w", grad_ggn="aa d | aa d | aa",
              diag="aa sqw sqc d | aa sqc d | aa sqw sqc", forward="T af | T af | T af"),
    "D": dict(local_ggn="AT | T AT | T AT | ce | aa w d | aa w d | aa",
              local_hessian="AT | T AT | T AT | ce | aa w2 d2 | aa2 w2 d2 | aa",
              grad_out_hessian="aa w d | aa aa w d | aa", grad_hessian="aa d | aa aa d | aa",
              grad_out_ggn="aa w d | aa w d | aa", grad_ggn="aa d | aa d | aa",
              diag="aa sqw sqc d | aa sqw sqc d | aa sqc", forward="T af | T af | T af"),
    "E": dict(_A, local_ggn="T AT | T AT | T AT | aa w d | aa w d | aa w",
              local_hessian="T AT | T AT | T AT | aa w2 d2 | aa2 w2 d2 | aa w"),
}


def layers_of(text):
    """The per-layer groups of an expected sequence, as lists of entry point names."""
    return [[SHORT[k] for k in group.split()] for group in text.split("|")]


def names_of(text):
    return [name for group in layers_of(text) for name in group]


def build(net, kind, monkeypatch):
    """(engine, the list its launches are recorded in) of net ``net`` as a ``ggn`` / ``hessian`` / ``session`` engine."""
    monkeypatch.setenv("HF_DENSE_ENGINE", "1")
    monkeypatch.setenv("HF_DENSE_HESSIAN", "1" if kind == "hessian" else "0")
    monkeypatch.setenv("HF_DENSE_SESSION", "1" if kind == "session" else "0")
    names = record_launches(monkeypatch)
    model, out, loss = net_and_loss(net)
    why = []
    eng = FusedGGNEngine.try_build(loss, out, [p for p in model.parameters() if p.requires_grad],
                                   hessian=kind == "hessian", why=why, need_session=kind == "session")
    assert isinstance(eng, DenseStackEngine) and eng.hessian == (kind == "hessian"), why
    assert (eng.loss_spec is not None) == (kind == "session"), why
    assert names, "the engine was built without a call through the proxy"
    del names[:]  # recording starts here
    return eng, names


def recorded(names, call):
    del names[:]
    call()
    return list(names)


def launch_counts(net, mode):
    """The two counts of the engine's docstring, on the sequences pinned above: a hidden live layer (all trainable, not
    the first live one) contributes exactly 5 names to a product, no layer more; ``diag_ef`` at most 4 per live layer."""
    groups, diag = layers_of(EXPECTED[net]["local_" + mode]), layers_of(EXPECTED[net]["diag"])
    live = len(diag)
    assert len(groups) == 2 * live + (0 if net == "E" else 1)
    tangent, adjoint = groups[:live], groups[-live:][::-1]  # both in layer order now
    per_layer = [len(t) + len(a) for t, a in zip(tangent, adjoint)]
    assert max(per_layer) <= 5
    if not FROZEN[net]:
        assert per_layer[1] == 5  # Linear(5,5) Tanh between two live layers
    assert max(len(g) for g in diag) <= 4


@pytest.mark.parametrize("kind", ["ggn", "hessian", "session"])
@pytest.mark.parametrize("net", sorted(EXPECTED))
def test_launch_sequence(net, kind, monkeypatch):
    eng, names = build(net, kind, monkeypatch)
    want = EXPECTED[net]
    v = torch.randn(eng.n, generator=torch.Generator().manual_seed(2)).to(DEV)
    out = torch.empty(eng.n, device=DEV)
    mode = "hessian" if kind == "hessian" else "ggn"
    assert recorded(names, lambda: eng.local(v)) == names_of(want["local_" + mode])
    if kind == "ggn":  # (no first-order sweep on a GGN engine outside session mode: nothing is launched)
        del names[:]
        with pytest.raises(RuntimeError):
            eng.gradient(out)
        assert names == []
    else:
        assert recorded(names, lambda: eng.gradient(out)) == names_of(want["grad_out_" + mode])
        assert recorded(names, lambda: eng.gradient()) == names_of(want["grad_" + mode])
    assert recorded(names, lambda: eng.diag_ef("mean")) == names_of(want["diag"])
    forward = want["forward"] + (" | lh" if kind == "session" else "")
    assert recorded(names, eng.forward_own) == names_of(forward)
    torch.cuda.synchronize()
    launch_counts(net, mode)
