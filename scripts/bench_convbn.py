"""GGN products per second of VGG-11-BN for 32x32 inputs (``testproblems.vgg11bn_cifar10``, ``--batch`` 32 / 128) as
hipGraph replays with a device synchronise: the plain-stack engine (eval-mode BatchNorm units; the pooled ones on
``hf_pool_bn_act_*_nhwc``) against the path such a model took before the engine accepted BatchNorm units -- autograd sweeps
over the prepared model, captured (``HF_ENGINE=0`` selects it).  ``--bn train``: the model in train mode (batch statistics
in both routes; the pooled units on ``hf_pool_bn_act_tangent_train_nhwc`` / ``hf_pool_bn_act_adjoint_reduce_nhwc``); the
engine's record also counts the library launches of one product.
``--reps`` repetitions of at least ``--seconds`` each, the two operators alternating; one JSON line per operator to
``--out`` (appended as soon as it is known), with every repetition's rate and the spread (max - min)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import pytorchhessianfree_amd as hf
from pytorchhessianfree_amd import curvature, modelprep
from pytorchhessianfree_amd import testproblems as tp


class _Counter:
    """Forwards every attribute to the real library and counts the calls of its launching entry points."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("hf_"):
            return fn

        def call(*args):
            self.names.append(name)
            return fn(*args)

        return call


def launches_per_product(op, v):
    """Library launches of one eager product of the engine ``op`` (plan queries and table builders left out)."""
    from pytorchhessianfree_amd import _lib

    real = _lib.load
    counter = _Counter(real())
    _lib.load = lambda: counter
    try:
        op.local(v)
        torch.cuda.synchronize()
    finally:
        _lib.load = real
    return len([n for n in counter.names if not n.endswith(("_plan", "_table", "_slabs_count"))])


def graphed(engine, batch, dev="cuda", train=False):
    model, (x, t), lossf = tp.vgg11bn_cifar10(batch_size=batch, device=dev)
    if train:
        model.train()
    modelprep.prepare_model(model, channels_last=True)
    params = [p for p in model.parameters() if p.requires_grad]

    def builder():
        out = model(x)
        return curvature.ggn_operator(lossf(out, t), out, params)

    old = os.environ.get("HF_ENGINE")
    os.environ["HF_ENGINE"] = "1" if engine else "0"
    try:
        op = curvature.maybe_graphed(builder, params=params)
    finally:
        if old is None:
            del os.environ["HF_ENGINE"]
        else:
            os.environ["HF_ENGINE"] = old
    assert isinstance(op, curvature.GraphedOperator), "the product was not captured"
    assert ("engine" in op.op.mode) == engine, op.op.mode
    return op


def rate(op, seconds):
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(20):
            op.replay_local()
        torch.cuda.synchronize()
        n += 20
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return n / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--bn", default="eval", choices=["eval", "train"])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    train = args.bn == "train"
    hf.configure()

    def emit(rec):
        print(json.dumps(rec), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(json.dumps(rec) + "\n")

    base = dict(workload="vgg11bn_cifar10", bn=args.bn, batch=args.batch, unit="GGN products/s (hipGraph replay + device sync)",
                device=torch.cuda.get_device_name(0))
    eng = graphed(True, args.batch, train=train)
    assert bool(getattr(eng.op, "train_bn", False)) == train
    v = torch.randn(eng.n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    eng.input_buffer.copy_(v)
    rate(eng, 0.2)
    first = [rate(eng, args.seconds)]
    emit(dict(base, operator="engine-graphed", mode=eng.op.mode, first_rep=first[0]))
    ref = graphed(False, args.batch, train=train)
    ref.input_buffer.copy_(v)
    rate(ref, 0.2)
    eng.replay_local()
    ref.replay_local()
    torch.cuda.synchronize()
    a, b = eng.output_buffer.double(), ref.output_buffer.double()
    agree = float((a - b).abs().max() / b.abs().max())
    rates = {"engine-graphed": [], "autograd-graphed": []}
    for _ in range(args.reps):
        rates["engine-graphed"].append(rate(eng, args.seconds))
        rates["autograd-graphed"].append(rate(ref, args.seconds))
    launches = {"engine-graphed": launches_per_product(eng.op, v)}
    for name, op in (("engine-graphed", eng), ("autograd-graphed", ref)):
        r = rates[name]
        emit(dict(base, operator=name, mode=op.op.mode, rates=r, median=sorted(r)[len(r) // 2], spread=max(r) - min(r),
                  products_agree_rel=agree, launches_per_product=launches.get(name)))


if __name__ == "__main__":
    main()
