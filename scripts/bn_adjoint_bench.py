"""Micro-benchmark: the eval-mode BatchNorm adjoint as ONE fused launch (k_bn_adjoint_rows / _pair: elementwise part +
per-channel sums, what the adjoint chain ran up to ABI 20) against the elementwise launch alone (k_bn_adjoint_v4 / _pair)
and the one launch that takes all the units' sums afterwards (k_bn_sums_multi).

The operands are not hard-coded: the script builds the bench's engine with the deferral switched off, records every
``hf_chan_affine_bwd_ex`` (row_blocks > 1) / ``hf_chan_affine_bwd_pair`` call of one GGN product -- pointers, slab counts
and strides, row blocks, as the engine issues them -- and replays each one, and its elementwise twin on the same operands,
as a hipGraph of ``REP`` back-to-back launches timed with device events.

    python scripts/bn_adjoint_bench.py [--workload resnet18] [--out profiles/r20_bn_adjoint_split_kernels.jsonl]
"""
import argparse
import ctypes
import json
import os
import sys

os.environ["HF_BN_SUMS_DEFER"] = "0"  # the engine under the recorder issues the fused launches
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import pytorchhessianfree_amd as hf  # noqa: E402
from pytorchhessianfree_amd import _lib, curvature, modelprep  # noqa: E402
from pytorchhessianfree_amd import testproblems as tp  # noqa: E402

REP, REPLAYS, ROUNDS = 20, 50, 5
# hf_chan_affine_bwd_ex's arguments as include/hf_pcg.h declares them.  The recorder sees the call positionally: a change of
# that signature must stop this script, not shift a field under another name
BWD_EX = ("gx", "gw", "gb", "gres", "gy", "gy_splits", "gy_slab", "gy2", "gy2_splits", "gy2_slab", "x", "mean", "rstd", "w",
          "mask_src", "n", "c", "hw", "channels_last", "row_blocks", "dtype", "stream")
assert len(BWD_EX) == len(_lib.SIGNATURES["hf_chan_affine_bwd_ex"][1]), "hf_chan_affine_bwd_ex changed: update BWD_EX"


class Recorder:
    """Wraps the ctypes library and keeps the arguments of the row-major BatchNorm adjoint launches."""

    def __init__(self, lib):
        self._lib, self.calls, self.on = lib, [], False

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in ("hf_chan_affine_bwd_ex", "hf_chan_affine_bwd_pair"):
            return fn

        def call(*a):
            if self.on:
                if name == "hf_chan_affine_bwd_pair":
                    src = ctypes.cast(a[0], ctypes.POINTER(_lib.BnAdjointProblem * 2)).contents
                    arr = (_lib.BnAdjointProblem * 2)()
                    ctypes.memmove(arr, src, ctypes.sizeof(arr))
                    self.calls.append(("pair", arr))
                else:
                    assert len(a) == len(BWD_EX), (len(a), len(BWD_EX))
                    if a[BWD_EX.index("row_blocks")] > 1:
                        self.calls.append(("one", a[:-1]))
            return fn(*a)

        return call


def timed(fn):
    """Mean us per launch: a graph of REP launches, REPLAYS replays between two device events; best of ROUNDS."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REP):
            fn()
    g.replay()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPLAYS):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / (REPLAYS * REP))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="resnet18", choices=["resnet18", "allcnnc", "resnet50"])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    hf.configure()
    dev = torch.device("cuda")
    if args.workload == "resnet18":
        model, (x, t), lossf = tp.resnet18_mnist(batch_size=32, device="cuda", data_seed=tp.RESNET18_B32_SEPARATED_SEEDS[0])
    elif args.workload == "allcnnc":
        model, (x, t), lossf = tp.allcnnc_cifar100(batch_size=32, device="cuda")
    else:
        model, (x, t), lossf = tp.resnet50_small_images(batch_size=32, device="cuda")
    modelprep.prepare_model(model, channels_last=True)
    params = [p for p in model.parameters() if p.requires_grad]
    out = model(x)
    eng = curvature.ggn_operator(lossf(out, t), out, params)
    assert "engine" in eng.mode, "the engine did not take this model"
    v, res = torch.randn(eng.n, device=dev), torch.empty(eng.n, device=dev)
    for _ in range(3):
        eng.local(v, out=res)
    torch.cuda.synchronize()
    lib = _lib.load()
    rec = Recorder(lib)
    _lib._lib = rec
    rec.on = True
    eng.local(v, out=res)
    rec.on = False
    _lib._lib = lib
    torch.cuda.synchronize()

    def stream():
        return _lib.current_stream_ptr(dev)

    keep, lines, table = [], [], []

    def spare(rows, c):  # where the engine stores no g today, the elementwise launch must
        keep.append(torch.empty(rows * c, device=dev))
        return keep[-1].data_ptr()

    def sums_entry(gw, gb, g, xp, mean, rstd, rows, c, rb):
        if not (gw or gb):
            return
        q = _lib.BnSumsProblem()
        q.gw, q.gb, q.g, q.x, q.mean, q.rstd, q.rows, q.c, q.row_blocks = gw, gb, g, xp, mean, rstd, rows, c, rb
        table.append(q)

    for kind, a in rec.calls:
        if kind == "one":
            (gx, gw, gb, gres, gy, s1, l1, gy2, s2, l2, xp, mean, rstd, w, mask, n, c, hw, _cl, rb, dt) = a
            rows = n * hw
            g = gres or spare(rows, c)
            line = {"launch": "single", "rows": [rows], "c": [c], "slabs": [[s1, s2 if gy2 else None]], "rb": [rb]}
            line["fused_us"] = timed(lambda: _lib.check(lib.hf_chan_affine_bwd_ex(*a, stream()), "fused"))
            line["elementwise_us"] = timed(lambda: _lib.check(lib.hf_bn_adjoint_v4(
                g, gx, gy, s1, l1, gy2, s2, l2, mask, w, rstd, rows, c, dt, stream()), "elementwise"))
            sums_entry(gw, gb, g, xp, mean, rstd, rows, c, rb)
        else:
            arr2 = (_lib.BnAdjointProblem * 2)()
            ctypes.memmove(arr2, a, ctypes.sizeof(arr2))
            for q in arr2:
                if not q.gres:
                    q.gres = spare(q.n * q.hw, q.c)
                sums_entry(q.gw, q.gb, q.gres, q.x, q.mean, q.rstd, q.n * q.hw, q.c, q.row_blocks)
            line = {"launch": "pair", "rows": [q.n * q.hw for q in a], "c": [q.c for q in a],
                    "slabs": [[q.gy_splits, q.gy2_splits if q.gy2 else None] for q in a],
                    "rb": [q.row_blocks for q in a]}
            line["fused_us"] = timed(lambda: _lib.check(lib.hf_chan_affine_bwd_pair(
                ctypes.cast(a, _lib.c_void_p), _lib.HF_F32, stream()), "fused pair"))
            line["elementwise_us"] = timed(lambda: _lib.check(lib.hf_bn_adjoint_v4_pair(
                ctypes.cast(arr2, _lib.c_void_p), _lib.HF_F32, stream()), "elementwise pair"))
        line["saved_us"] = line["fused_us"] - line["elementwise_us"]
        lines.append(line)
    # the sums of every recorded unit in one launch (HF_BN_SUMS_MAX problems per launch)
    flush = {"launch": "sums_multi", "problems": len(table)}
    if table:
        tab = (_lib.BnSumsProblem * len(table))(*table)
        blocks = lib.hf_bn_sums_table(ctypes.cast(tab, _lib.c_void_p), len(table))
        assert blocks > 0, blocks
        tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)

        def run():
            for lo in range(0, len(table), _lib.BN_SUMS_MAX):
                _lib.check(lib.hf_bn_sums_multi(tab_dev.data_ptr(), ctypes.cast(tab, _lib.c_void_p), len(table), lo,
                                                min(_lib.BN_SUMS_MAX, len(table) - lo), _lib.HF_F32, stream()),
                           "hf_bn_sums_multi")

        flush["workgroups"], flush["us"] = int(blocks), timed(run)
    n_l = max(1, len(lines))
    summary = {"workload": args.workload, "launches_per_product": len(lines),
               "fused_us_sum": sum(ln["fused_us"] for ln in lines),
               "elementwise_us_sum": sum(ln["elementwise_us"] for ln in lines),
               "mean_saved_us_per_launch": sum(ln["saved_us"] for ln in lines) / n_l,
               "sums_multi_us": flush.get("us"),
               "net_saved_us_per_product": sum(ln["saved_us"] for ln in lines) - (flush.get("us") or 0.0)}
    rnd = lambda d: {k: (round(val, 3) if isinstance(val, float) else val) for k, val in d.items()}  # noqa: E731
    text = "\n".join(json.dumps(rnd(d)) for d in lines + [flush, summary])
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
