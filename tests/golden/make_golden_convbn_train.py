"""Golden traces of the REAL reference on the small plain stacks with BatchNorm units in TRAIN mode
(``testproblems.convbn_small`` / ``convbn_fc_small`` after ``model.train()``: batch statistics in the forward pass and in
every derivative) -- the reference side of ``tests/test_convbn_train_engine_gpu.py``.

Run where the reference is available (see ``make_golden.py``)::

    python tests/golden/make_golden_convbn_train.py

Built on ``make_golden_convbn.py``'s layout and the helpers of ``make_golden_convnets.py``: per net (keys ``small/...``
and ``fc/...``) the reference's ``_Gv`` (and, for ``convbn_small``, ``_Hv``) on seeded vectors, the gradient, the loss and
the logits -- each also from the same code in float64 (``.../f64``) -- at batch 2 and batch 5, and a three-step ``step()``
trace with default settings.  No ``diag``: the reference's per-sample loop evaluates one sample at a time, which in train
mode is another function (statistics of a batch of one).  The running statistics are not stored: they depend on how many
points a run evaluates.

The step traces' data seeds are SEARCHED (``CANDIDATES``, in order): the first triple on which the reference's own fp32
and float64 runs take the same discrete decisions is stored, with the triple itself (``<net>/steps/seeds``).
"""

import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_convbn as cb  # noqa: E402  (registers the BackPACK restatement, imports the reference)
from pytorchhessianfree_amd import testproblems as tp  # noqa: E402
from torch.nn.utils.convert_parameters import parameters_to_vector  # noqa: E402

gc, mg, RefHF = cb.gc, cb.mg, cb.RefHF
CANDIDATES = [(s, s + 1, s + 2) for s in range(141, 201, 3)]
NETS = {"small": (tp.convbn_small, True, 2), "fc": (tp.convbn_fc_small, False, 5)}


def _train(make):
    def make_train(**kw):
        model, data, lossf = make(**kw)
        return model.train(), data, lossf
    return make_train


def put_point(store, key, make, batch, hessian):
    """Gradient, loss, logits and one GGN (and Hessian) product at the seeded batch, train mode.  (Every forward pass
    moves the running statistics, which nothing stored here reads.)"""
    model, (x, t), lossf = make(batch_size=batch, device="cpu")
    assert model.training
    params = [p for p in model.parameters() if p.requires_grad]
    idx = gc.put_index(store, key, params)
    store[key + "/init_sha1"] = np.array(gc.sha(gc.flat(params)))
    m64, l64, x64 = gc.double_twin(model, lambda m: lossf, x)
    assert m64.training
    out = model(x)
    loss = lossf(out, t)
    p64 = [p for p in m64.parameters() if p.requires_grad]
    out64 = m64(x64)
    loss64 = l64(out64, t)
    store[key + "/inputs_sha1"] = np.array(gc.sha(x))
    store[key + "/targets"] = gc.npy(t)
    store[key + "/logits"] = gc.npy(out)
    store[key + "/logits_f64"] = out64.detach().numpy()
    store[key + "/loss"] = np.array(float(loss.detach()))
    store[key + "/loss_f64"] = np.array(float(loss64.detach()))
    gc.put_vec(store, key + "/grad", parameters_to_vector(torch.autograd.grad(loss, params, retain_graph=True)), idx)
    gc.put_vec(store, key + "/grad/f64", parameters_to_vector(torch.autograd.grad(loss64, p64, retain_graph=True)), idx)
    n = sum(p.numel() for p in params)
    gc.put_product(store, key + "/ggn", lambda v: RefHF._Gv(loss, out, params, v).detach(), n, idx, seed=171 + batch,
                   B64=lambda v: RefHF._Gv(loss64, out64, p64, v).detach())
    if hessian:
        gc.put_product(store, key + "/hessian", lambda v: RefHF._Hv(loss, params, v).detach(), n, idx, seed=173 + batch,
                       B64=lambda v: RefHF._Hv(loss64, p64, v).detach())


def put_steps(store, key, make, batch):
    for seeds in CANDIDATES:
        trial = {}
        try:
            cb.put_steps(trial, key, make, seeds, batch)
        except AssertionError as exc:
            print(f"{key}: seeds {seeds} rejected ({str(exc)[:120]})", flush=True)
            continue
        trial[key + "/seeds"] = np.array(seeds)
        for k, v in trial.items():
            store.setdefault(k, v)  # (the index sample may be there already)
        print(f"{key}: seeds {seeds}", flush=True)
        return
    raise SystemExit(f"{key}: no candidate seeds on which the reference's fp32 and float64 runs agree")


def make_convbn_train():
    store = {}
    for name, (make, hessian, step_batch) in NETS.items():
        make = _train(make)
        for batch in (2, 5):
            put_point(store, f"{name}/b{batch}", make, batch, hessian)
        put_steps(store, f"{name}/steps", make, step_batch)
    mg.save("convnet_convbn_train.npz", store)


if __name__ == "__main__":
    torch.set_num_threads(gc.THREADS)
    t0 = time.time()
    make_convbn_train()
    print(f"convbn_train: {time.time() - t0:.0f} s", flush=True)
