"""Stock fp32 autograd and the conv engines against the float64 reference on the cases of ``tests/geometry_nets.py``: one
JSON line per (series, case, quantity) with the error of every parameter tensor -- the record the bounds of
``tests/test_engine_geometry_gpu.py`` are taken from (3x the worst ``stock_fp32`` figure per quantity, one significant
digit, rounded up; the last lines printed list them).

    python scripts/engine_geometry_errors.py --out profiles/rNN_engine_geometry.jsonl
    python scripts/engine_geometry_errors.py --cases tail --out profiles/rNN_tail_geometry.jsonl
    python scripts/engine_geometry_errors.py --cases bn --out profiles/rNN_bn_geometry.jsonl

``--cases tail``: the classifier-tail cases (``geometry_nets.TAIL_CASES``) and the measures of
``tests/test_tail_geometry_gpu.py`` -- the record of its ``BOUND_TAIL`` (GGN products only: no Hessian, no train mode).

``--cases bn``: the BatchNorm plain stacks (``geometry_nets.BN_CASES``) and the measures of
``tests/test_bn_geometry_gpu.py`` -- the record of its ``BOUND_BN``: every quantity in eval and in train mode (``*_train``),
the running statistics one train-mode forward pass moves (``running``), the mixed-mode and frozen variants.

A case the engine gets wrong is recorded (``"failed"``) and the run goes on; any other error ends it."""

import argparse
import json
import math
import os
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import pytorchhessianfree_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--series", default="all", choices=["all", "stock_fp32", "engine"])
    ap.add_argument("--cases", default="geometry", choices=["geometry", "tail", "bn"])
    args = ap.parse_args()
    pytorchhessianfree_amd.configure()  # (as tests/conftest.py: the accurate MIOpen solvers for the stock side)
    import geometry_nets as gn
    if args.cases == "bn":
        return main_bn(args, gn)
    if args.cases == "tail":
        import test_tail_geometry_gpu as tests
    else:
        import test_engine_geometry_gpu as tests
    tail = args.cases == "tail"
    cases = gn.TAIL_CASES if tail else gn.CASES

    run, worst = recorder(args.out)

    def stock_train(case):
        res = gn.stock_fp32_errors(case, "cuda", train=True)
        return {"ggn_train": res["ggn"], "hessian_train": res["hessian"]}

    def stock(case):
        res = gn.stock_fp32_errors(case, "cuda")
        if tail:
            del res["hessian"]  # (the engine makes no Hessian products through a classifier tail: no bound to take)
        return res

    for case in cases if args.series in ("all", "stock_fp32") else []:
        run("stock_fp32", case, "stock", lambda: stock(case))
        if case in gn.TRAIN_CASES:
            run("stock_fp32", case, "stock_train", lambda: stock_train(case))
    for case in cases if args.series in ("all", "engine") else []:
        run("engine", case, "forward", lambda: tests.forward_errors(case))
        run("engine", case, "gradient", lambda: tests.gradient_errors(case))
        run("engine", case, "ggn", lambda: tests.product_errors(case))
        if not tail:
            run("engine", case, "hessian", lambda: tests.product_errors(case, hessian=True))
        if case in gn.TRAIN_CASES:
            run("engine", case, "ggn_train", lambda: tests.product_errors(case, train=True))
            run("engine", case, "hessian_train", lambda: tests.product_errors(case, hessian=True, train=True))
        for batched, prefix in (("0", "per_sample/"), ("1", "batched/")):
            os.environ["HF_DIAG_EF_BATCHED"] = batched  # (read when the engine is built)
            run("engine", case, "diag_ef", lambda: tests.diag_errors(case), prefix=prefix)
        os.environ.pop("HF_DIAG_EF_BATCHED")
    print_bounds(worst)


def recorder(path):
    """``run(series, case, what, fn, prefix="", label="")`` writes one line per quantity of ``fn()``'s result to ``path``
    (``label``: what the line's quantity is called there, the bound's name unchanged); ``worst``: per quantity the worst
    ``stock_fp32`` figure and its case."""
    fh = open(path, "w")
    worst = {}

    def emit(series, case, quantity, errs, **kw):
        top = max(errs.values()) if errs else None
        fh.write(json.dumps({"series": series, "case": case, "quantity": quantity, "worst": top, "errors": errs, **kw}) + "\n")
        fh.flush()
        print(series, case, quantity, "failed" if top is None else f"{top:.2e}", flush=True)
        if series == "stock_fp32" and top is not None and top > worst.get(quantity, (0.0, None))[0]:
            worst[quantity] = (top, case)

    def run(series, case, what, fn, prefix="", **kw):
        t0 = time.time()
        try:
            res = fn()
        except AssertionError:
            emit(series, case, what, {}, failed=traceback.format_exc()[-1500:].replace(ROOT + os.sep, ""), **kw)
            return
        for quantity, errs in res.items():
            if isinstance(errs, dict):
                emit(series, case, prefix + quantity, errs, seconds=round(time.time() - t0, 2), **kw)

    return run, worst


def print_bounds(worst):
    torch.cuda.synchronize()
    for quantity, (top, case) in worst.items():
        e = math.floor(math.log10(3 * top))
        print(f"bound {quantity}: 3 x {top:.3e} ({case}) -> {math.ceil(3 * top / 10 ** e - 1e-9)}e{e}")


def main_bn(args, gn):
    import test_bn_geometry_gpu as tests
    run, worst = recorder(args.out)

    def stock(case, train):
        res = gn.stock_fp32_errors(case, "cuda", train=train)
        return {(k + "_train" if train and k != "running" else k): v for k, v in res.items()}

    modes = {case: ([False, True] if case in gn.BN_TRAIN_CASES else [False]) for case in gn.BN_CASES}
    for case in gn.BN_CASES if args.series in ("all", "stock_fp32") else []:
        for train in modes[case]:
            run("stock_fp32", case, "stock_train" if train else "stock", lambda: stock(case, train))
    for case in gn.BN_CASES if args.series in ("all", "engine") else []:
        for train in modes[case]:
            run("engine", case, "forward", lambda: tests.forward_errors(case, train))
            run("engine", case, "gradient", lambda: tests.gradient_errors(case, train))
            run("engine", case, "ggn", lambda: tests.product_errors(case, train=train))
            if case in gn.BN_HESSIAN_CASES:
                run("engine", case, "hessian", lambda: tests.product_errors(case, hessian=True, train=train))
        for batched, prefix in (("0", "per_sample/"), ("1", "batched/")):
            os.environ["HF_DIAG_EF_BATCHED"] = batched  # (read when the engine is built)
            run("engine", case, "diag_ef", lambda: tests.diag_errors(case), prefix=prefix)
        os.environ.pop("HF_DIAG_EF_BATCHED")
    for name in sorted(tests.MIXED) if args.series in ("all", "engine") else []:
        for hessian in (False, True):
            run("engine", tests.MIXED_CASE, name, lambda: tests.mixed_errors(name, hessian), variant=name)
    print_bounds(worst)


if __name__ == "__main__":
    main()
