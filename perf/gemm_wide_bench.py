"""Per projection group: ONE wide launch (qpal_tcq_gemm_wide) at n rows against two 128-row passes of the lockstep
launch (multi_gemv on row slices, what Prefill(chunk=128) runs), event-timed, the two alternated inside one call.

    python perf/gemm_wide_bench.py [--n 256] [--reps 30] [--out profiles/gemm_wide.json]

--lut BITS VEC (repeatable): the Llama-3.1-8B groups with ldlq_<VEC>_<BITS> layers instead — ONE qpal_lut_gemm_wide launch (DESIGN.md
§43) against multi_gemv on slices of the codec's fused batch (128 rows, 64 under a 128 KiB codebook image), what wide_gemm ran for
these layers before; --passes P measures every group P times in the one call (the spread of a repeated pair).

    python perf/gemm_wide_bench.py --lut 4 1 --lut 8 2 --passes 2 --out profiles/lut_gemm_wide.json
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import qpalette_amd as qp  # noqa: E402

# (name, quantizer, k, [m of every layer of the group])
GROUPS = [
    ("8b q|k|v", "tcomb_6_7_0.5_none_0.9", 4096, [4096, 1024, 1024]), ("8b o", "tcomb_6_7_0.5_none_0.9", 4096, [4096]),
    ("8b up|gate", "tcomb_6_7_0.5_none_0.9", 4096, [14336, 14336]), ("8b down", "tcomb_6_7_0.5_none_0.9", 14336, [4096]),
    ("70b q|k|v", "tcq_3_none_0.9", 8192, [8192, 1024, 1024]), ("70b o", "tcq_3_none_0.9", 8192, [8192]),
    ("70b up|gate", "tcq_3_none_0.9", 8192, [28672, 28672]), ("70b down", "tcq_3_none_0.9", 28672, [8192]),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lut", type=int, nargs=2, action="append", metavar=("BITS", "VEC"))
    ap.add_argument("--passes", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    dev, n = torch.device("cuda", 0), args.n
    rows = []
    groups = GROUPS if not args.lut else [(name, f"ldlq_{vec}_{bits}_none_1.0", k, ms) for bits, vec in args.lut for name, _, k, ms in GROUPS[:4]]
    for name, qstr, k, ms in groups * args.passes:
        layers = [qp.make_linear_from_info(qstr, qp.mem_op.dummy_linear_info(k, m, qstr, seed=i, codebook_seed=1)).to(dev)
                  for i, m in enumerate(ms)]
        if not args.lut:
            qp.share_codebooks(layers)
        x = (torch.randn(n, k, device=dev) * 0.5).half()
        wide = [torch.zeros(n, m, dtype=torch.float32, device=dev) for m in ms]
        two = [torch.zeros(n, m, dtype=torch.float32, device=dev) for m in ms]
        # (the launch itself, not wide_gemm: that sends the classes measured slower here to the sliced path)
        step = min(128, min(l.max_fused_batch for l in layers))
        two_streams = isinstance(layers[0], qp.CombtLinearTCQ)
        if args.lut:
            ljobs = [(l.qweight, l.lut, l.out_features) for l in layers]
            run_wide = lambda: qp.ops.lut_gemm_wide(ljobs, x, layers[0].lut_bits, layers[0].vec_sz, outs=wide)
        else:
            jobs = [(l.trellis1, l.trellis2, l.tlut, l.out_features) if two_streams else (l.trellis, None, l.tlut, l.out_features) for l in layers]
            kv1, kv2 = tuple(layers[0].KV) if two_streams else (layers[0].KV, 0)
            run_wide = lambda: qp.ops.tcq_gemm_wide(jobs, x, 9, kv1, kv2, outs=wide)
        run_two = lambda: [qp.multi_gemv(layers, x[r:r + step], outs=[t[r:r + step] for t in two]) for r in range(0, n, step)]
        for _ in range(3):
            run_wide(), run_two()
        torch.cuda.synchronize()
        diff = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(wide, two))
        t = {"wide": [], "two": []}
        for _ in range(args.reps):
            for key, fn in (("wide", run_wide), ("two", run_two)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                t[key].append(e0.elapsed_time(e1) * 1e3)
        med = {key: sorted(v)[len(v) // 2] for key, v in t.items()}
        rows.append({"group": name, "quantizer": qstr, "k": k, "m": ms, "n": n, "us_wide": med["wide"], "us_two_128_row_passes": med["two"],
                     "slice_rows": step,
                     "us_wide_min": min(t["wide"]), "us_two_min": min(t["two"]), "speedup": med["two"] / med["wide"], "max_rel_diff": diff})
        print(json.dumps(rows[-1]), flush=True)
        del layers, x, wide, two
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"what": "one wide launch vs passes over slices of slice_rows rows (us_two_128_row_passes) per projection group (median of event times, alternated)",
                       "device": torch.cuda.get_device_name(0), "groups": rows}, f, indent=1)


if __name__ == "__main__":
    main()
