"""The compact curvature product alone, as a hipGraph: microseconds per replay.

Builds the headline workload's engine (ResNet-18 on 28x28 inputs, batch 32, eval-mode BatchNorm; the set-up of
scripts/engine_product_driver.py, the model prepared by the passes bench.py runs), captures ONE product between
vectors in the compact layout (``engine.local_compact``: what the PCG iteration graph clones) and replays it
``--replays`` times between two events, ``--reps`` times over.  Prints one JSON line.  ``HF_PCG_LIB`` selects a
variant library (``csrc/build.py::build(out=..., extra_flags=...)``).

    python scripts/product_replay_bench.py [--replays 500] [--reps 5] [--tag NAME]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import torch

import pytorchhessianfree_amd as hf
from pytorchhessianfree_amd import _lib, curvature, modelprep
from pytorchhessianfree_amd import testproblems as tp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    hf.configure()
    dev = "cuda"
    model, (x, t), lossf = tp.resnet18_mnist(batch_size=32, seed=0, device=dev,
                                             data_seed=tp.RESNET18_B32_SEPARATED_SEEDS[0])
    # bench.py build_operator(channels_last=1)
    modelprep.fuse_eval_batchnorm(model)
    modelprep.fuse_conv_tangent(model, channels_last=True)
    modelprep.fuse_residual_blocks(model)
    modelprep.fuse_bn_relu(model)
    modelprep.skip_identity_pools(model)
    modelprep._install_engine_hooks(model)
    params = [p for p in model.parameters() if p.requires_grad]
    out = model(x)
    eng = curvature.ggn_operator(lossf(out, t), out, params)
    assert "engine" in eng.mode, "the engine did not take this model"
    lay = eng.compact_layout()
    assert lay is not None, "no compact layout"
    n_live = lay["n_live"]
    vc = torch.randn(n_live, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    res = torch.empty(n_live, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(3):
            eng.local_compact(vc, res)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = res.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        eng.local_compact(vc, res)
    for _ in range(20):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(res, eager), "the replayed product differs from the eager one"
    us = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.replays):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        us.append(1e3 * e0.elapsed_time(e1) / args.replays)
    print(json.dumps({"what": "compact product, hipGraph replay", "tag": args.tag,
                      "lib": os.path.basename(_lib.LIB_PATH), "n_live": n_live, "n": eng.n,
                      "replays": args.replays, "us_per_product": [round(u, 2) for u in us],
                      "min_us": round(min(us), 2), "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
