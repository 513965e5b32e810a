#!/usr/bin/env python
"""Matvecs/s of the GGN product of the 25.5 M-parameter MLP (3072-4096-3072-100, Tanh, cross-entropy, batch 64:
the 1-GPU leg of BASELINE.json configs[4] as ``tests/test_optimizer_gpu.py::_mlp25m`` builds it) inside ``cg()``:

    python scripts/bench_dense_engine.py --prepared 1     # the dense-stack engine, hipGraph-replayed
    python scripts/bench_dense_engine.py --prepared 0     # the autograd sweeps, hipGraph-replayed

The operator is the one ``HessianFree(graph_matvec=True).step()`` hands to ``cg()`` (``HessianFree.linearise``); the
timed region is ``--reps`` repetitions of ``--steps`` solves of ``--iters`` iterations (``tol = 0``: every solve runs
all of them), each repetition timed on its own after ``--warmup`` untimed solves.  Prints one JSON line."""

import argparse
import json
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pytorchhessianfree_amd as hf  # noqa: E402
from pytorchhessianfree_amd import modelprep  # noqa: E402


def mlp25m(device):
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(3072, 4096), torch.nn.Tanh(), torch.nn.Linear(4096, 3072), torch.nn.Tanh(),
                              torch.nn.Linear(3072, 100))
    g = torch.Generator().manual_seed(1)
    x, t = torch.rand(64, 3072, generator=g), torch.randint(0, 100, (64,), generator=g)
    return net.to(device), x.to(device), t.to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prepared", type=int, default=1)
    ap.add_argument("--iters", type=int, default=250)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--damping", type=float, default=1.0)
    args = ap.parse_args()
    dev = torch.device("cuda")
    model, x, t = mlp25m(dev)
    if args.prepared:
        os.environ["HF_DENSE_ENGINE"] = "1"  # (the engine is opt-in until this script's figures stand in DESIGN.md)
        modelprep.prepare_model(model)
    lossf = torch.nn.CrossEntropyLoss()
    opt = hf.HessianFree(model.parameters(), graph_matvec=True)
    opt._session_off = True  # (neither leg has a persistent session for this model: measure the per-step operator)

    def forward():
        o = model(x)
        return lossf(o, t), o

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        op, grad, loss, _ = opt.linearise(forward)
    A = hf.DampedCurvature(op, args.damping)
    b = -grad

    def solve():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return hf.cg(A, b, max_iter=args.iters, tol=0.0, martens_conv_crit=False, store_x_at_iters=[0])

    for _ in range(args.warmup):
        solve()
    rates, iters_done = [], None
    for _ in range(args.reps):
        calls0 = op.calls
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _s in range(args.steps):
            xs, _, reason = solve()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rates.append((op.calls - calls0) / dt)
        iters_done = len(xs) - 1
    n = sum(p.numel() for p in model.parameters())
    floor_us = 4 * 4 * n / 6.3e12 * 1e6  # the 4 N-word traffic floor at 6.3 TB/s
    mid = sorted(rates)[len(rates) // 2]
    print(json.dumps({
        "bench": "dense_engine_mlp25m", "prepared": bool(args.prepared), "path": opt.path_report()["step"]["path"],
        "mode": getattr(op, "mode", ""), "n": n, "batch": 64, "iters": args.iters, "iters_done": iters_done,
        "steps": args.steps, "reps": args.reps, "matvecs_per_s": [round(r, 1) for r in rates],
        "median_matvecs_per_s": round(mid, 1), "spread": round(max(rates) - min(rates), 1),
        "us_per_matvec_incl_pcg": round(1e6 / mid, 1), "floor_us_4n_words": round(floor_us, 1), "initial_loss": loss,
        "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
