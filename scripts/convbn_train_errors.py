"""Stock fp32 autograd and the plain-stack engine against the float64 twin on the train-mode cases of
``tests/test_convbn_train_engine_gpu.py`` (``POINTS`` and ``MIXED``: every case of its product and mixed-mode tests), both
on the ENGINE's replayed ReLU and pooling decisions: one JSON line per (series, case) with the error of every quantity --
the record that file's ``BOUND`` is taken from (3x the worst ``stock_fp32`` figure per quantity, one significant digit,
rounded up; the last lines printed list them).

    python scripts/convbn_train_errors.py --out profiles/rNN_convbn_train.jsonl
"""

import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import pytorchhessianfree_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    pytorchhessianfree_amd.configure()  # (as tests/conftest.py: the accurate MIOpen solvers for the stock side)
    import test_convbn_train_engine_gpu as tests

    worst = {"stock_fp32": {}, "engine": {}}
    with open(args.out, "a") as fh:
        for family, batch, hessian, prep in tests.POINTS + tests.MIXED:
            case = f"{family}-b{batch}-{'hessian' if hessian else 'ggn'}" + (f"-{prep.__name__.strip('_')}" if prep else "")
            for series, stock in (("stock_fp32", True), ("engine", False)):
                errs, _op = tests.measure(family, batch, hessian, prep, stock=stock)
                fh.write(json.dumps({"record": "float64_error", "series": series, "case": case, "errors": errs,
                                     "device": torch.cuda.get_device_name(0)}) + "\n")
                fh.flush()
                print(series, case, {k: f"{e:.2e}" for k, e in errs.items()}, flush=True)
                for k, e in errs.items():
                    if e > worst[series].get(k, (0.0, None))[0]:
                        worst[series][k] = (e, case)
        for series in worst:
            for k, (e, case) in sorted(worst[series].items()):
                line = {"record": "worst", "series": series, "quantity": k, "worst": e, "case": case}
                if series == "stock_fp32":
                    mag = 10.0 ** math.floor(math.log10(3 * e))
                    line["bound_3x"] = math.ceil(3 * e / mag - 1e-9) * mag
                fh.write(json.dumps(line) + "\n")
                print(line, flush=True)


if __name__ == "__main__":
    main()
