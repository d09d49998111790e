#!/usr/bin/env python3
"""qpal_hessian_accum against the two torch ways of accumulating a proxy Hessian, on the same data, in one process.

Per width n in {4096, 14336}, 4096 fp16 rows per call:
  kernel   HessianAccumulator.add(X)                  fp16 MFMA products, fp32 partial sums of <= 256 rows, fp64 accumulation,
                                                      lower-triangle tiles only
  fp64     H.add_(X.double().T @ X.double())          the customary way: the accumulator's own precision class
  fp32     H32.addmm_(X.float().T, X.float())         recorded beside them (an fp32 accumulator over all rows)
Every call is timed with device events; the three take turns inside each of `--calls` rounds after `--warmup` untimed rounds, so
that clock and neighbours hit all three alike.  The conversions of X are part of the torch calls, as they are for a user.
Writes profiles/hessian_bench.json.  Needs a GPU: there is nothing to measure without one.

    python perf/hessian_bench.py [--n 4096 14336] [--rows 4096] [--calls 20] [--warmup 3] [--out profiles/hessian_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import qpalette_amd as qp

F16_PEAK = 2.5e15   # dense f16 matrix peak of the part, FLOP/s


def measure(n, rows, calls, warmup, dev):
    X = (torch.randn(rows, n, device=dev, generator=torch.Generator(device=dev).manual_seed(n)) * 1.5).half()
    acc = qp.HessianAccumulator(n, dev)
    H64 = torch.zeros(n, n, dtype=torch.float64, device=dev)
    H32 = torch.zeros(n, n, dtype=torch.float32, device=dev)
    ways = {"kernel": lambda: acc.add(X),
            "fp64": lambda: H64.add_(X.double().T @ X.double()),
            "fp32": lambda: H32.addmm_(X.float().T, X.float())}
    ms = {k: [] for k in ways}
    for r in range(warmup + calls):
        for name, fn in ways.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= warmup:
                ms[name].append(a.elapsed_time(b))
    # the three accumulators saw the same rows the same number of times
    L = torch.tril(acc.S)
    ref = torch.tril(H64)
    rel = float((L - ref).norm() / ref.norm())
    rel32 = float((torch.tril(H32).double() - ref).norm() / ref.norm())
    rec = {"n": n, "rows_per_call": rows, "calls": calls, "warmup": warmup}
    for name, v in ms.items():
        rec[f"{name}_ms_median"], rec[f"{name}_ms_min"] = statistics.median(v), min(v)
    flops = rows * n * (n + 128)
    rec["kernel_flops_counted"] = flops
    rec["kernel_TFLOPs"] = flops / (rec["kernel_ms_median"] * 1e-3) / 1e12
    rec["kernel_share_of_f16_peak"] = rec["kernel_TFLOPs"] * 1e12 / F16_PEAK
    rec["speedup_over_fp64"] = rec["fp64_ms_median"] / rec["kernel_ms_median"]
    rec["speedup_over_fp32"] = rec["fp32_ms_median"] / rec["kernel_ms_median"]
    rec["kernel_vs_fp64_rel_frobenius_lower"] = rel
    rec["fp32_vs_fp64_rel_frobenius_lower"] = rel32
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[4096, 14336])
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hessian_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("hessian_bench.py needs a GPU")
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(dev), "f16_peak_TFLOPs": F16_PEAK / 1e12, "results": []}
    for n in args.n:
        rec = measure(n, args.rows, args.calls, args.warmup, dev)
        out["results"].append(rec)
        print(f"n={n}: kernel {rec['kernel_ms_median']:.3f} ms ({rec['kernel_TFLOPs']:.0f} TFLOP/s, "
              f"{100 * rec['kernel_share_of_f16_peak']:.1f} % of f16 peak)  fp64 {rec['fp64_ms_median']:.3f} ms  "
              f"fp32 {rec['fp32_ms_median']:.3f} ms  -> {rec['speedup_over_fp64']:.1f}x fp64, {rec['speedup_over_fp32']:.2f}x fp32")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
