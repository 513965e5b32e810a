"""CPU: the replay of ``stack_harness.py`` itself -- the float64-on-given-decisions reference every plain-stack product,
gradient and diagonal is held to -- on the smallest problems (``convpool_small``, ``convfc_small``, eval-mode
``convbn_small``; batch 2, float64), and its launch recorder on a stand-in library.

The model's OWN decisions (ReLU masks ``inp > 0``, pool positions of ``max_pool2d(..., return_indices=True)``) replayed
reproduce output and gradient exactly and are all consumed; a decision far from a tie fails with the bound's note; one
within rounding of a tie passes."""

import copy

import pytest
import torch

from pytorchhessianfree_amd import testproblems as tp
from stack_harness import LaunchRecorder, replay

PROBLEMS = {"convpool_small": (tp.convpool_small, 2), "convfc_small": (tp.convfc_small, 3),
            "convbn_small": (tp.convbn_small, 2)}  # constructor, ReLU calls per pass (convfc_small: the tail's included)
MARGIN = 1e-5  # (``replay``'s default)


def _problem(name):
    model, (x, t), lossf = PROBLEMS[name][0](batch_size=2, device="cpu")
    return model.double(), x.double(), t, lossf


def _own_decisions(model, x):
    """(masks, pools, relu inputs, pool inputs) of one pass of the stock float64 ``model``, in call order."""
    masks, pools, relu_in, pool_in = [], [], [], []

    def relu_hook(mod, args):
        relu_in.append(args[0].detach().clone())
        masks.append(args[0].detach() > 0)

    def pool_hook(mod, args):
        pool_in.append(args[0].detach().clone())
        pools.append(torch.nn.functional.max_pool2d(args[0].detach(), mod.kernel_size, mod.stride, mod.padding,
                                                    return_indices=True)[1])

    hooks = [m.register_forward_pre_hook(relu_hook if isinstance(m, torch.nn.ReLU) else pool_hook)
             for m in model.modules() if isinstance(m, (torch.nn.ReLU, torch.nn.MaxPool2d))]
    with torch.no_grad():
        model(x)
    for h in hooks:
        h.remove()
    return masks, pools, relu_in, pool_in


def _grads(model, x, t, lossf):
    out = model(x)
    return out.detach(), torch.autograd.grad(lossf(out, t), [p for p in model.parameters() if p.requires_grad])


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_own_decisions_reproduce_output_and_gradient_and_are_all_consumed(name):
    model, x, t, lossf = _problem(name)
    masks, pools, _, _ = _own_decisions(model, x)
    assert (len(masks), len(pools)) == (PROBLEMS[name][1], 2)
    want_out, want_grads = _grads(model, x, t, lossf)
    twin = copy.deepcopy(model)
    rewind = replay(twin, masks, pools)
    got_out, got_grads = _grads(twin, x, t, lossf)
    assert torch.equal(got_out, want_out)
    assert len(got_grads) == len(want_grads) and all(torch.equal(a, b) for a, b in zip(got_grads, want_grads))
    assert rewind() == (len(masks), 2)  # both lists were walked to their ends (the tail's ReLU of convfc_small too)
    assert rewind() == (0, 0)
    with torch.no_grad():  # (and from the start again)
        assert torch.equal(twin(x), want_out)
    assert rewind() == (len(masks), 2)


def _note(excinfo):
    return excinfo.value.args[0][3]  # (``tol.within``: (site, value, bound, note))


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_a_far_relu_flip_fails(name):
    model, x, _, _ = _problem(name)
    masks, pools, relu_in, _ = _own_decisions(model, x)
    at = relu_in[0].abs().flatten().argmax()  # the first ReLU's entry farthest from zero
    masks[0].view(-1)[at] ^= True
    replay(model, masks, pools)
    with pytest.raises(AssertionError) as excinfo, torch.no_grad():
        model(x)
    assert _note(excinfo) == "replayed ReLU decision far from zero"


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_a_far_pool_move_fails(name):
    model, x, _, _ = _problem(name)
    masks, pools, _, pool_in = _own_decisions(model, x)
    inp, mod = pool_in[0], next(m for m in model.modules() if isinstance(m, torch.nn.MaxPool2d))
    k, s = mod.kernel_size, mod.stride
    windows = inp.unfold(2, k, s).unfold(3, k, s).flatten(4)  # [n, c, oh, ow, k*k]
    assert windows.shape[:4] == pools[0].shape and mod.padding == 0
    spread = windows.max(-1).values - windows.min(-1).values
    n, c, i, j = (int(a) for a in torch.unravel_index(spread.argmax(), spread.shape))
    assert float(spread[n, c, i, j]) > MARGIN * float(inp.abs().max())  # the precondition: no tie in this window
    low = int(windows[n, c, i, j].argmin())
    pools[0][n, c, i, j] = (i * s + low // k) * inp.shape[3] + j * s + low % k
    assert inp[n, c].flatten()[pools[0][n, c, i, j]] == windows[n, c, i, j].min()
    replay(model, masks, pools)
    with pytest.raises(AssertionError) as excinfo, torch.no_grad():
        model(x)
    assert _note(excinfo) == "replayed pool position far from the window's maximum"


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_a_tie_sized_relu_flip_passes(name):
    """One input of the first ReLU set to 1e-7 x the layer's max-norm (by a hook in front of it), its decision flipped:
    inside the margin, the pass goes through and drops that entry."""
    model, x, _, _ = _problem(name)
    first = next(m for m in model.modules() if isinstance(m, torch.nn.ReLU))

    def nudge(mod, args):
        inp = args[0].clone()
        inp.view(-1)[0] = 1e-7 * inp.abs().max()
        return (inp,)

    first.register_forward_pre_hook(nudge)
    masks, pools, relu_in, _ = _own_decisions(model, x)
    assert bool(masks[0].view(-1)[0])  # (``_own_decisions`` hooked behind ``nudge``: it saw the nudged input)
    assert 0 < float(relu_in[0].view(-1)[0] / relu_in[0].abs().max()) < MARGIN
    masks[0].view(-1)[0] = False
    rewind = replay(model, masks, pools)
    with torch.no_grad():
        assert torch.isfinite(model(x)).all()
    assert rewind() == (len(masks), 2)


def test_launch_recorder_records_and_forwards_hf_calls_only():
    class Lib:
        other = "not a launch"

        def hf_x(self, *args):
            return ("ran", args)

    names = []
    proxy = LaunchRecorder(Lib(), names)
    assert proxy.hf_x(1, "two") == ("ran", (1, "two")) and names == ["hf_x"]
    assert proxy.other == "not a launch" and names == ["hf_x"]
    assert proxy.hf_x() == ("ran", ()) and names == ["hf_x", "hf_x"]
    with pytest.raises(AttributeError):
        proxy.hf_missing
