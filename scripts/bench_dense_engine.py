#!/usr/bin/env python
"""Matvecs/s of the GGN (``--curvature hessian``: the Hessian) product of the 25.5 M-parameter MLP (3072-4096-3072-100, Tanh, cross-entropy, batch 64:
the 1-GPU leg of BASELINE.json configs[4] as ``tests/test_optimizer_gpu.py::_mlp25m`` builds it) inside ``cg()``:

    python scripts/bench_dense_engine.py --prepared 1     # the dense-stack engine, hipGraph-replayed
    python scripts/bench_dense_engine.py --prepared 0     # the autograd sweeps, hipGraph-replayed
    python scripts/bench_dense_engine.py --curvature hessian --prepared 1   # forward over reverse on the engine
    python scripts/bench_dense_engine.py --curvature hessian --prepared 0   # autograd double backward, hipGraph-replayed

The operator is the one ``HessianFree(graph_matvec=True).step()`` hands to ``cg()`` (``HessianFree.linearise``); the
timed region is ``--reps`` repetitions of ``--steps`` solves of ``--iters`` iterations (``tol = 0``: every solve runs
all of them), each repetition timed on its own after ``--warmup`` untimed solves.  Prints one JSON line.

    python scripts/bench_dense_engine.py --diag-ef        # the diagonal empirical-Fisher preconditioner instead

``--diag-ef``: wall time per call (after ``--warmup`` untimed calls) and ``torch.cuda.max_memory_allocated`` of the
diagonal of the same model and batch by ``diag_EF_backpack`` with ``HF_DENSE_ENGINE=1`` on the prepared model (the
dense-stack engine's sweep), ``diag_EF_backpack`` with the switch unset (the ``vmap`` per-sample gradients) and
``diag_EF_autograd`` (one backward pass per sample) -- ``--reps`` JSON lines each, one child process per route so that
no route sees another's cached blocks in its peak.

    python scripts/bench_dense_engine.py --step-ms --session 1    # step() on the dense-stack engine's persistent session
    python scripts/bench_dense_engine.py --step-ms --session 0    # step() as engine-graphed (the engine rebuilt per step)

``--step-ms``: wall time per COMPLETE default ``HessianFree(graph_matvec=True).step()`` of the prepared model, a fresh
batch per step: ``--reps`` repetitions of ``--steps`` steps, each repetition timed on its own after ``--warmup`` untimed
repetitions; one process per leg.  With ``--session 1`` (``HF_DENSE_SESSION=1``) also the number of kernel launches of one
replay of the session's forward graph."""

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


DIAG_ROUTES = ("backpack_engine", "backpack_vmap", "autograd")


def diag_ef_route(route, warmup, reps):
    """``reps`` JSON lines for one route of the diagonal empirical Fisher (this process runs nothing else)."""
    dev = torch.device("cuda")
    model, x, t = mlp25m(dev)
    if route == "backpack_engine":
        os.environ["HF_DENSE_ENGINE"] = "1"
    else:
        os.environ.pop("HF_DENSE_ENGINE", None)
    if route == "backpack_engine":  # (the other two routes run the stock model, as before this engine existed)
        modelprep.prepare_model(model)
    lossf = torch.nn.CrossEntropyLoss()
    fn = hf.diag_EF_autograd if route == "autograd" else hf.diag_EF_backpack
    why = []
    if route != "autograd":
        from pytorchhessianfree_amd.engine.dense import diag_ef_of

        on_engine = diag_ef_of(model, lossf, x, t, "mean", why=why) is not None
        assert on_engine == (route == "backpack_engine"), why

    def call():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return fn(model, lossf, x, t, "mean")

    for _ in range(warmup):
        call()
    n = sum(p.numel() for p in model.parameters())
    sweep_ms = None
    if route == "backpack_engine":  # the sweep alone on ONE engine (a call of the public route builds its own)
        from pytorchhessianfree_amd.engine.dense import DenseStackEngine

        o = model(x)
        eng = DenseStackEngine.try_build(lossf(o, t), o, list(model.parameters()))
        out = eng.diag_ef("mean")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            eng.diag_ef("mean", out=out)
        torch.cuda.synchronize()
        sweep_ms = round(1e3 * (time.perf_counter() - t0) / 20, 3)
        del eng, out, o
    for rep in range(reps):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        d = call()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(json.dumps({
            "bench": "dense_diag_ef_mlp25m", "route": route, "rep": rep, "n": n, "batch": int(x.shape[0]),
            "ms_per_call": round(1e3 * dt, 3), "max_memory_allocated_mb": round(torch.cuda.max_memory_allocated() / 2**20, 1),
            "allocated_before_mb": round(base / 2**20, 1), "engine_sweep_alone_ms": sweep_ms, "diag_max": float(d.max()), "declined": why,
            "device": torch.cuda.get_device_name(0)}), flush=True)
        del d


def diag_ef_bench(args):
    import subprocess

    for route in DIAG_ROUTES:
        subprocess.run([sys.executable, os.path.abspath(__file__), "--diag-ef-route", route, "--warmup", str(args.warmup),
                        "--reps", str(args.reps)], check=True)


def step_ms(args):
    """One JSON line: ms per complete step() of the prepared 25.5 M-parameter MLP, with or without the session."""
    os.environ["HF_DENSE_ENGINE"] = "1"
    if args.session:
        os.environ["HF_DENSE_SESSION"] = "1"
    else:
        os.environ.pop("HF_DENSE_SESSION", None)
    if args.curvature == "hessian":
        os.environ["HF_DENSE_HESSIAN"] = "1"
    dev = torch.device("cuda")
    model, x, t = mlp25m(dev)
    modelprep.prepare_model(model)
    lossf = torch.nn.CrossEntropyLoss()
    opt = hf.HessianFree(model.parameters(), curvature_opt=args.curvature, graph_matvec=True)
    gen = torch.Generator(device=dev).manual_seed(2)
    batch = {}

    def forward():
        o = model(batch["x"])
        return lossf(o, batch["t"]), o

    def steps():
        finals = []
        for _ in range(args.steps):
            batch["x"] = torch.rand(x.shape, device=dev, generator=gen)
            batch["t"] = torch.randint(0, 100, t.shape, device=dev, generator=gen)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                finals.append(opt.step(forward))
        return finals

    for _ in range(args.warmup):
        steps()
    ms, paths = [], set()
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        finals = steps()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / args.steps)
        paths.add(opt.path_report()["step"]["path"])
    fwd_launches = None
    sess = getattr(opt, "_session", None)
    if sess is not None:  # every entry point of the forward pass is one launch, the loss head two
        from pytorchhessianfree_amd import _lib

        calls, check = [], _lib.check
        _lib.check = lambda rc, what: (calls.append(what), check(rc, what))[1]
        try:
            with torch.no_grad():
                sess.engine.forward_own(refresh=True)
        finally:
            _lib.check = check
        torch.cuda.synchronize()
        fwd_launches = len(calls) + calls.count("hf_dense_loss_head")
    mid = sorted(ms)[len(ms) // 2]
    print(json.dumps({
        "bench": "dense_step_ms_mlp25m", "curvature": args.curvature, "session_switch": bool(args.session),
        "path": sorted(paths), "declined": opt.path_report()["step"]["declined"],
        "n": sum(p.numel() for p in model.parameters()), "batch": int(x.shape[0]), "steps": args.steps,
        "warmup": args.warmup, "reps": args.reps, "step_ms": [round(v, 2) for v in ms], "median_step_ms": round(mid, 2),
        "spread_ms": round(max(ms) - min(ms), 2), "g_fwd_launches": fwd_launches, "final_loss": finals[-1],
        "session_steps": getattr(sess, "steps", None), "device": torch.cuda.get_device_name(0)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step-ms", action="store_true")
    ap.add_argument("--session", type=int, default=1)
    ap.add_argument("--diag-ef", action="store_true")
    ap.add_argument("--diag-ef-route", choices=DIAG_ROUTES, default=None)
    ap.add_argument("--prepared", type=int, default=1)
    ap.add_argument("--curvature", choices=("ggn", "hessian"), default="ggn")
    ap.add_argument("--iters", type=int, default=250)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--damping", type=float, default=1.0)
    args = ap.parse_args()
    if args.diag_ef_route:
        return diag_ef_route(args.diag_ef_route, args.warmup, args.reps)
    if args.diag_ef:
        return diag_ef_bench(args)
    if args.step_ms:
        return step_ms(args)
    dev = torch.device("cuda")
    model, x, t = mlp25m(dev)
    if args.prepared:
        os.environ["HF_DENSE_ENGINE"] = "1"  # (the engine is opt-in until this script's figures stand in DESIGN.md)
        os.environ["HF_DENSE_HESSIAN"] = "1"
        modelprep.prepare_model(model)
    lossf = torch.nn.CrossEntropyLoss()
    opt = hf.HessianFree(model.parameters(), curvature_opt=args.curvature, graph_matvec=True)
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
    # the traffic floor at 6.3 TB/s: GGN 4 N words (W, V read twice); Hessian 5 N (W, V read twice, the gradient written)
    words = 5 if args.curvature == "hessian" else 4
    floor_us = 4 * words * n / 6.3e12 * 1e6
    mid = sorted(rates)[len(rates) // 2]
    print(json.dumps({
        "bench": "dense_engine_mlp25m", "curvature": args.curvature, "prepared": bool(args.prepared), "path": opt.path_report()["step"]["path"],
        "mode": getattr(op, "mode", ""), "n": n, "batch": 64, "iters": args.iters, "iters_done": iters_done,
        "steps": args.steps, "reps": args.reps, "matvecs_per_s": [round(r, 1) for r in rates],
        "median_matvecs_per_s": round(mid, 1), "spread": round(max(rates) - min(rates), 1),
        "us_per_matvec_incl_pcg": round(1e6 / mid, 1), f"floor_us_{words}n_words": round(floor_us, 1), "initial_loss": loss,
        "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
