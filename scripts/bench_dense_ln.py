"""GGN products per second of the 25.5 M-parameter MLP's widths with a LayerNorm behind every hidden ``Linear``
(``testproblems.mlp_layernorm``: 3072-4096-3072-100, Tanh, cross-entropy, ``--batch`` 64 / 256) as hipGraph replays with a
device synchronise: the dense-stack engine with its LayerNorm layers on the row-resident kernels of hf_ln.hip
(``HF_DENSE_ENGINE=1 HF_DENSE_LN=1``) against the path such a model takes without the switch -- autograd sweeps over the
prepared model, captured.  ``--reps`` repetitions (default 9) of at least ``--seconds`` each, the two operators alternating
on one device; one JSON line per operator to ``--out`` with every repetition's rate, the median and the spread
(max - min); the engine's record also counts the library launches of one product (``profiles/dense_ln.jsonl``)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import pytorchhessianfree_amd as hf
from bench_convbn import launches_per_product, rate
from pytorchhessianfree_amd import curvature, modelprep
from pytorchhessianfree_amd import testproblems as tp


def graphed(engine, batch, dev="cuda"):
    model, (x, t), lossf = tp.mlp_layernorm(batch_size=batch, device=dev)
    modelprep.prepare_model(model)
    params = [p for p in model.parameters() if p.requires_grad]

    def builder():
        out = model(x)
        return curvature.ggn_operator(lossf(out, t), out, params)

    switches = ("HF_DENSE_ENGINE", "HF_DENSE_LN")
    os.environ.update({name: "1" if engine else "0" for name in switches})
    try:
        op = curvature.maybe_graphed(builder, params=params)
    finally:
        for name in switches:
            del os.environ[name]
    assert isinstance(op, curvature.GraphedOperator), "the product was not captured"
    assert ("engine" in op.op.mode) == engine, op.op.mode
    return op


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    hf.configure()

    def emit(rec):
        print(json.dumps(rec), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(json.dumps(rec) + "\n")

    base = dict(workload="mlp_layernorm", batch=args.batch, unit="GGN products/s (hipGraph replay + device sync)",
                device=torch.cuda.get_device_name(0))
    eng, ref = (graphed(e, args.batch) for e in (True, False))
    v = torch.randn(eng.n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    for op in (eng, ref):
        op.input_buffer.copy_(v)
        rate(op, 0.2)
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
