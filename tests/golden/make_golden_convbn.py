"""Golden traces of the REAL reference on the small plain stacks with eval-mode BatchNorm units
(``testproblems.convbn_small``: conv - BN - ReLU - max-pool, conv - BN - ReLU, conv - BN - max-pool, a 1x1 convolution,
global average pooling; ``testproblems.convbn_fc_small``: two pooled conv - BN - ReLU units and a ``Flatten, Linear, ReLU,
Linear`` tail) -- the reference side of ``tests/test_convbn_engine_gpu.py``.

Run where the reference is available (see ``make_golden.py``)::

    python tests/golden/make_golden_convbn.py

Built on the helpers of ``make_golden.py`` / ``make_golden_convnets.py`` (which import the reference behind the
BackPACK restatement), as ``make_golden_convpool.py`` / ``make_golden_convfc.py`` are: per net (keys ``small/...`` and
``fc/...``) the reference's ``_Gv`` (and, for ``convbn_small``, ``_Hv``) on seeded vectors, the gradient, the loss, the
logits and ``diag_EF_autograd`` -- each also from the same code in float64 (``.../f64``) -- at batch 2 and batch 5, and a
three-step ``step()`` trace with default settings (losses, damping, CG iterations, termination reasons).  Arrays, digests
and reason strings only; the 1764- / 1694-entry vectors are stored whole (the index sample covers them).
"""

import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_convnets as gc  # noqa: E402  (registers the BackPACK restatement, imports the reference)
from hessianfree.preconditioners import diag_EF_autograd  # noqa: E402
from pytorchhessianfree_amd import testproblems as tp  # noqa: E402
from torch.nn.utils.convert_parameters import parameters_to_vector  # noqa: E402

mg, RefHF = gc.mg, gc.RefHF
# Data seeds of the step traces: batches on which the reference's own fp32 and float64 runs take the same discrete
# decisions (termination reasons, learning rates, damping schedule) -- checked below before anything is stored.  (On seeds
# (51, 52, 53) the tail net's two runs part at the first step: best CG iterate 7 against 3.)
NETS = {"small": (tp.convbn_small, True, (41, 42, 43), 2), "fc": (tp.convbn_fc_small, False, (61, 62, 63), 5)}


def put_point(store, key, make, batch, hessian):
    """Gradient, loss, logits, diagonal empirical Fisher and one GGN (and Hessian) product at the seeded batch."""
    model, (x, t), lossf = make(batch_size=batch, device="cpu")
    params = [p for p in model.parameters() if p.requires_grad]
    idx = gc.put_index(store, key, params)
    out = model(x)
    loss = lossf(out, t)
    m64, l64, x64 = gc.double_twin(model, lambda m: lossf, x)
    p64 = [p for p in m64.parameters() if p.requires_grad]
    out64 = m64(x64)
    loss64 = l64(out64, t)
    store[key + "/init_sha1"] = np.array(gc.sha(gc.flat(params)))
    store[key + "/inputs_sha1"] = np.array(gc.sha(x))
    store[key + "/targets"] = gc.npy(t)
    store[key + "/logits"] = gc.npy(out)
    store[key + "/logits_f64"] = out64.detach().numpy()
    store[key + "/loss"] = np.array(float(loss.detach()))
    store[key + "/loss_f64"] = np.array(float(loss64.detach()))
    gc.put_vec(store, key + "/grad", parameters_to_vector(torch.autograd.grad(loss, params, retain_graph=True)), idx)
    gc.put_vec(store, key + "/grad/f64", parameters_to_vector(torch.autograd.grad(loss64, p64, retain_graph=True)), idx)
    gc.put_vec(store, key + "/diag", diag_EF_autograd(model, lossf, x, t, "mean"), idx)
    gc.put_vec(store, key + "/diag/f64", diag_EF_autograd(m64, l64, x64, t, "mean"), idx)
    n = sum(p.numel() for p in params)
    gc.put_product(store, key + "/ggn", lambda v: RefHF._Gv(loss, out, params, v).detach(), n, idx, seed=71 + batch,
                   B64=lambda v: RefHF._Gv(loss64, out64, p64, v).detach())
    if hessian:
        gc.put_product(store, key + "/hessian", lambda v: RefHF._Hv(loss, params, v).detach(), n, idx, seed=73 + batch,
                       B64=lambda v: RefHF._Hv(loss64, p64, v).detach())


def _double(make):
    def make64(**kw):
        model, (x, t), lossf = make(**kw)
        return model.double(), (x.double(), t), lossf
    return make64


def put_steps(store, key, make, seeds, batch):
    """The three-step trace, and the same from the reference's code in float64: its discrete entries must be the fp32
    run's, or the fp32 trace is nothing to hold another fp32 implementation to (choose other seeds)."""
    gc.run_steps(store, key, make, seeds, 3, mk=dict(batch_size=batch))
    twin = {}
    gc.run_steps(twin, key, _double(make), seeds, 3, mk=dict(batch_size=batch))
    for name in ("cg_reasons", "learning_rates", "dampings"):
        a, b = store[f"{key}/state/{name}"].tolist(), twin[f"{key}/state/{name}"].tolist()
        assert a == b, (name, a, b)
    it32, it64 = store[f"{key}/state/num_cg_iters"].tolist(), twin[f"{key}/state/num_cg_iters"].tolist()
    assert all(abs(a - b) <= 1 for a, b in zip(it32, it64)), (it32, it64)
    for a, b in zip(store[f"{key}/state/init_losses"].tolist(), twin[f"{key}/state/init_losses"].tolist()):
        assert abs(a - b) <= 1e-5 * abs(b), (a, b)
    for a, b in zip(store[f"{key}/final_losses"].tolist(), twin[f"{key}/final_losses"].tolist()):
        assert abs(a - b) <= 1e-4 * abs(b), (a, b)


def make_convbn():
    store = {}
    for name, (make, hessian, step_seeds, step_batch) in NETS.items():
        for batch in (2, 5):
            put_point(store, f"{name}/b{batch}", make, batch, hessian)
        put_steps(store, f"{name}/steps", make, step_seeds, step_batch)
    mg.save("convnet_convbn.npz", store)


if __name__ == "__main__":
    torch.set_num_threads(gc.THREADS)
    t0 = time.time()
    make_convbn()
    print(f"convbn: {time.time() - t0:.0f} s", flush=True)
