#!/usr/bin/env python
"""Wall time of ``session.diag_ef`` (the diagonal empirical Fisher of the conv-unit engines as ONE graph replay, what
``HessianFree.get_preconditioner`` calls from the second step on) with ``HF_DIAG_EF_BATCHED`` off -- per-sample
weight-gradient launches and one squaring gather per sample -- and on -- one squared-sum launch per layer and one gather:

    python scripts/bench_diag_ef.py [--out profiles/<round>_diag_ef_batched.jsonl]

Configurations: ResNet-18 on MNIST shapes at batch 32, All-CNN-C (CIFAR-100 shapes) at batch 32 and at batch 128.  One
child process per (configuration, switch), the two switches ALTERNATING, ``--rounds`` times over, so that both routes see
the same state of the machine.  A child builds the model, takes one ``step()`` (which leaves the persistent session at that
batch), warms the replay up ``--warmup`` times and times ``--reps`` (>= 5) replays, each with its final synchronisation;
it prints one JSON line: the replays' times, their median and spread, and the number of ``hf_*`` calls of one eager sweep
(that the two routes agree is the tests' business).  The parent appends the lines to ``--out`` and prints, per
configuration, the ratio of the medians (off / on).

    python scripts/bench_diag_ef.py --split-sweep allcnnc_b128 [--out ...]

``--split-sweep``: per layer of the configuration's engine, the time of ONE ``hf_conv2d_nhwc_sqsum_slabs`` launch on the
engine's own operands (HIP events around 20 launches, median of ``--reps`` such measurements) at the planned number of
sample splits and at forced ones -- what the planner's workgroup target was chosen from."""

import argparse
import json
import os
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"resnet18_b32": ("resnet18_mnist", 32), "allcnnc_b32": ("allcnnc_cifar100", 32),
           "allcnnc_b128": ("allcnnc_cifar100", 128)}
SWITCH = "HF_DIAG_EF_BATCHED"


def child(config, warmup, reps):
    import torch

    import pytorchhessianfree_amd as hf
    from pytorchhessianfree_amd import _lib, modelprep
    from pytorchhessianfree_amd import testproblems as tp

    problem, batch = CONFIGS[config]
    model, (x, t), lossf = getattr(tp, problem)(batch_size=batch, device="cuda")
    modelprep.prepare_model(model, channels_last=True)
    opt = hf.HessianFree(model.parameters(), graph_matvec=True, cg_max_iter=2)

    def forward():
        o = model(x)
        return lossf(o, t), o

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        opt.step(forward)
    sess = opt._session
    assert sess is not None, opt.path_report()
    eng = sess.engine
    assert eng._diag_batched == (os.environ.get(SWITCH, "0") == "1")
    reduction = eng.loss_spec["reduction"]

    class Count:
        def __init__(self, lib):
            self.lib, self.n = lib, 0

        def __getattr__(self, name):
            fn = getattr(self.lib, name)
            if name not in _lib.SIGNATURES:
                return fn

            def call(*args):
                self.n += 1
                return fn(*args)

            return call

    for _ in range(warmup):
        d = sess.diag_ef(reduction)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d = sess.diag_ef(reduction)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    counter, real = Count(_lib.load()), _lib.load
    _lib.load = lambda: counter
    try:
        with torch.no_grad():
            eng.diag_ef(reduction)
        torch.cuda.synchronize()
    finally:
        _lib.load = real
    mid = sorted(ms)[len(ms) // 2]
    print(json.dumps({
        "bench": "diag_ef_batched", "config": config, "batched": eng._diag_batched, "engine": type(eng).__name__,
        "n": eng.n, "batch": batch, "warmup": warmup, "reps": reps, "ms": [round(v, 3) for v in ms],
        "median_ms": round(mid, 3), "spread_ms": round(max(ms) - min(ms), 3), "hf_calls_per_sweep": counter.n,
        "diag_max": float(d.max()), "device": torch.cuda.get_device_name(0)}), flush=True)


def split_sweep(config, reps, out):
    import torch

    import pytorchhessianfree_amd as hf
    from pytorchhessianfree_amd import _lib, modelprep
    from pytorchhessianfree_amd import testproblems as tp

    os.environ[SWITCH] = "1"
    problem, batch = CONFIGS[config]
    model, (x, t), lossf = getattr(tp, problem)(batch_size=batch, device="cuda")
    modelprep.prepare_model(model, channels_last=True)
    opt = hf.HessianFree(model.parameters(), graph_matvec=True, cg_max_iter=2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        opt.step(lambda: (lambda o: (lossf(o, t), o))(model(x)))
    eng = opt._session.engine
    eng.diag_ef(eng.loss_spec["reduction"])  # (cotangents and the sweep's geometry)
    for u in eng.units:
        if u.dead or u.pw is None:
            continue
        n, h, w, c, k, r, s, st, pd = u.geo1
        act, ga = (u.cols_pad if u.im2col else u.x), (u.ga1 if eng.hessian else u.ga)
        counts = sorted({u.sW1} | {sp for sp in (1, 2, 4, 8, 16, 32, 64, 128) if sp <= n and -(-n // sp) * (sp - 1) < n})
        for sp in counts:
            buf = torch.zeros((sp, u.conv.weight.numel()), device="cuda")

            def launch():
                _lib.conv2d_nhwc_sqsum_slabs(buf, act, ga, n, h, w, c, k, r, s, st, pd, sp, pre=float(n),
                                             out_c=u.jcols if u.im2col else 0)

            launch()
            us = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _i in range(20):
                    launch()
                e1.record()
                torch.cuda.synchronize()
                us.append(1e3 * e0.elapsed_time(e1) / 20)
            row = {"bench": "sqsum_split_sweep", "config": config, "unit": u.name, "geometry": [n, h, w, c, k, r, s, st[0], pd[0]],
                   "splits": sp, "planned": sp == u.sW1, "us_per_launch": round(sorted(us)[len(us) // 2], 2),
                   "spread_us": round(max(us) - min(us), 2), "device": torch.cuda.get_device_name(0)}
            print(json.dumps(row), flush=True)
            if out:
                with open(out, "a") as fh:
                    fh.write(json.dumps(row) + "\n")
    for u in eng.units:  # the squared channel sums at the engine's number of sample shares
        if u.dead or (u.pg is None and u.pb is None):
            continue
        n, k, hw = u.a.shape[0], u.a.shape[1], u.a.shape[2] * u.a.shape[3]
        bn = u.bn is not None and u.pg is not None
        g = (u.g1 if eng.hessian else u.g) if u.bn is not None else (u.ga1 if eng.hessian else u.ga)

        def launch():
            _lib.chan_sqsum(g, n, k, hw, u.rb1, pre=float(n), gw2=u.gws if bn else None,
                            gb2=u.gbs if u.pb is not None else None, x=u.a if bn else None,
                            mean=u.mean if bn else None, rstd=u.rstd if bn else None)

        launch()
        us = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _i in range(20):
                launch()
            e1.record()
            torch.cuda.synchronize()
            us.append(1e3 * e0.elapsed_time(e1) / 20)
        row = {"bench": "chan_sqsum", "config": config, "unit": u.name, "geometry": [n, hw, k], "row_blocks": u.rb1,
               "with_xhat": bn, "us_per_launch": round(sorted(us)[len(us) // 2], 2), "spread_us": round(max(us) - min(us), 2),
               "device": torch.cuda.get_device_name(0)}
        print(json.dumps(row), flush=True)
        if out:
            with open(out, "a") as fh:
                fh.write(json.dumps(row) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--split-sweep", choices=sorted(CONFIGS), default=None)
    ap.add_argument("--child", choices=sorted(CONFIGS), default=None)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if args.split_sweep:
        return split_sweep(args.split_sweep, args.reps, args.out)
    if args.child:
        return child(args.child, args.warmup, args.reps)
    rows = []
    for config in args.configs.split(","):
        for rnd in range(args.rounds):
            for switch in ("0", "1"):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", config, "--warmup",
                                    str(args.warmup), "--reps", str(args.reps)], env=dict(os.environ, **{SWITCH: switch}),
                                   capture_output=True, text=True, timeout=600)
                if p.returncode != 0:
                    sys.stderr.write(p.stderr[-3000:])
                    sys.exit("%s with %s=%s failed (exit status %d)" % (config, SWITCH, switch, p.returncode))
                row = json.loads(p.stdout.strip().splitlines()[-1])
                row["round"] = rnd
                rows.append(row)
                print(json.dumps(row), flush=True)
                if args.out:
                    with open(args.out, "a") as fh:
                        fh.write(json.dumps(row) + "\n")
    for config in args.configs.split(","):
        med = {b: sorted(r["median_ms"] for r in rows if r["config"] == config and r["batched"] == b) for b in (False, True)}
        off, on = (m[len(m) // 2] for m in (med[False], med[True]))
        print("%s: off %.3f ms (%s), on %.3f ms (%s), off / on = %.2f" % (config, off, med[False], on, med[True], off / on))


if __name__ == "__main__":
    main()
