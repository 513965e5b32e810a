"""GGN (or, ``--curvature hessian``, Hessian) products per second of All-CNN-C with ``GroupNorm(8, .)`` behind every convolution but the last (32x32 inputs, 100
classes, ``--batch`` 32 / 128) as hipGraph replays with a device synchronise: the plain-stack engine with its GroupNorm
units on the one-launch kernels of hf_gn.hip (``HF_GN_ENGINE=1``) against the path such a model takes without the switch
-- autograd sweeps over the prepared model, captured (``--curvature hessian``: ``HF_GN_ENGINE=1 HF_GN_HESSIAN=1`` against the
captured autograd ``HessianOperator``).  ``--reps`` repetitions (default 9) of at least ``--seconds`` each,
the two operators alternating on one device; one JSON line per operator to ``--out`` with every repetition's rate, the
median and the spread (max - min); the engine's record also counts the library launches of one product.

``--groups 1``: ``GroupNorm(1, .)`` instead -- every unit at 32x32 and 16x16 is then beyond one workgroup's LDS and takes
the split kernels (``HF_GN_ENGINE=1 HF_GN_SPLIT=1``; with ``--curvature hessian`` also ``HF_GN_HESSIAN=1``), against the
captured autograd operator the same model runs on without the switches; the record counts the split units
(``profiles/gn_split.jsonl``, ``profiles/gn_split_hessian.jsonl``)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from torch import nn

import pytorchhessianfree_amd as hf
from bench_convbn import launches_per_product, rate
from pytorchhessianfree_amd import curvature, modelprep


class AllCNNCGN(nn.Module):
    def __init__(self, num_classes=100, groups=8):
        super().__init__()

        def c(i, o, k, s=1, p=0):
            return [nn.Conv2d(i, o, k, s, p, bias=False), nn.GroupNorm(groups, o), nn.ReLU()]

        self.net = nn.Sequential(
            *c(3, 96, 3, 1, 1), *c(96, 96, 3, 1, 1), *c(96, 96, 3, 2, 1),
            *c(96, 192, 3, 1, 1), *c(192, 192, 3, 1, 1), *c(192, 192, 3, 2, 1),
            *c(192, 192, 3, 1, 0), *c(192, 192, 1), nn.Conv2d(192, num_classes, 1), nn.ReLU(),
            nn.AdaptiveAvgPool2d((1, 1)),
        )

    def forward(self, x):
        return torch.flatten(self.net(x), -3)


def graphed(engine, batch, dev="cuda", hessian=False, groups=8):
    torch.manual_seed(0)
    model = AllCNNCGN(groups=groups).eval().to(dev)
    gen = torch.Generator().manual_seed(0)
    x, t = torch.rand(batch, 3, 32, 32, generator=gen).to(dev), torch.randint(0, 100, (batch,), generator=gen).to(dev)
    lossf = nn.CrossEntropyLoss()
    modelprep.prepare_model(model, channels_last=True)
    params = [p for p in model.parameters() if p.requires_grad]

    def builder():
        out = model(x)
        if hessian:
            return curvature.hessian_operator(lossf(out, t), out, params)
        return curvature.ggn_operator(lossf(out, t), out, params)

    switches = ("HF_GN_ENGINE", "HF_GN_SPLIT") + (("HF_GN_HESSIAN",) if hessian else ())
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
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default="")
    ap.add_argument("--curvature", choices=("ggn", "hessian"), default="ggn")
    ap.add_argument("--groups", type=int, default=8, help="groups of every GroupNorm (1: blocks beyond the LDS, split units)")
    args = ap.parse_args()
    hf.configure()

    def emit(rec):
        print(json.dumps(rec), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(json.dumps(rec) + "\n")

    hessian = args.curvature == "hessian"
    kind = "Hessian" if hessian else "GGN"
    base = dict(workload=f"allcnnc_groupnorm{args.groups}", batch=args.batch, unit=f"{kind} products/s (hipGraph replay + device sync)",
                device=torch.cuda.get_device_name(0))
    eng, ref = (graphed(e, args.batch, hessian=hessian, groups=args.groups) for e in (True, False))
    split_units = sum(bool(u.gn_parts) for u in eng.op.units)
    if split_units:
        base["split_units"] = split_units
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
