#!/usr/bin/env python3
"""Whole-layer quantisation cost on one GPU (qpalette_amd.quantize_layer).

    python perf/layer_quant_bench.py [--out profiles/layer_quant_bench.json] [--kernel-stats STATS_CSV]
    rocprofv3 --kernel-trace --stats -d DIR -o lq --output-format csv -- python perf/layer_quant_bench.py --rotate-only

1. rotate_f32 (qpal_hadamard_f32, csrc/hadamard_f32.hip) on 4096 x 4096, 4096 x 14336 and 14336 x 14336 (in place): time per launch
   from HIP events (median of 20 after 3 warm-up launches), bytes moved (rows * n * 8) per second and the share of the 8 TB/s HBM
   peak.  --kernel-stats: the kernel time of the same launches as rocprofv3 --kernel-trace --stats measured them, from a run of
   its own (--rotate-only), merged into the record.
2. quantize_linear's phases for the Llama-3.1-8B linear shapes (out x in: 4096 x 4096, 1024 x 4096, 14336 x 4096,
   4096 x 14336) with tcomb_5_6_0.5_hess_0.9 and tcq_6_hess_0.9 on a synthetic SPD H: preprocess (rotation of W and H, Wscale),
   LDL (block LDL of HRr), LDLQ + Viterbi (the column-block loop), pack (host-side trellis packing), each timed on its own
   (wall clock, synchronised), and the whole quantize_linear call.
"""
import argparse
import csv
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qpalette_amd as qp  # noqa: E402
from qpalette_amd import hadamard as had  # noqa: E402
from qpalette_amd import packers, quantize  # noqa: E402
from qpalette_amd import quantize_layer as ql  # noqa: E402

HBM_PEAK_GBS = 8000.0
ROT_SHAPES = [(4096, 4096), (4096, 14336), (14336, 14336)]
LAYERS = [(4096, 4096), (1024, 4096), (14336, 4096), (4096, 14336)]
QSTRS = ["tcomb_5_6_0.5_hess_0.9", "tcq_6_hess_0.9"]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def rotate_figures(reps=20):
    out = []
    for rows, n in ROT_SHAPES:
        x = torch.randn(rows, n, device="cuda")
        hadK, K = had.get_hadK(n, transpose=True)
        su = torch.where(torch.rand(n, device="cuda") > 0.5, 1.0, -1.0)
        for _ in range(3):
            had.rotate_f32(x, hadK=hadK, K=K, su=su, out=x)
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            had.rotate_f32(x, hadK=hadK, K=K, su=su, out=x)
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        ms = sorted(ts)[len(ts) // 2]
        nbytes = rows * n * 8
        out.append({"rows": rows, "n": n, "K": K, "in_place": True, "bytes": nbytes, "event_ms_median": ms,
                    "event_GBps": nbytes / ms / 1e6, "event_share_of_hbm_peak": nbytes / ms / 1e6 / HBM_PEAK_GBS})
        del x
    return out


def merge_kernel_stats(rot, path):
    """Kernel time of had_f32_kernel from a rocprofv3 --stats CSV of a --rotate-only run: (3 + 20) launches per shape in ROT_SHAPES
    order; the stats give per-kernel-instantiation averages, so shapes that share an instantiation are not separable: report the
    instantiations as measured."""
    rows = [r for r in csv.DictReader(open(path)) if "had_f32_kernel" in r["Name"]]
    return [{"kernel": r["Name"], "calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3,
             "min_us": float(r.get("MinNs", 0) or 0) / 1e3, "max_us": float(r.get("MaxNs", 0) or 0) / 1e3} for r in rows]


def spd(k, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.randn(2 * k, k, generator=g, device="cuda", dtype=torch.float64)
    X *= torch.linspace(0.2, 2.0, k, dtype=torch.float64, device="cuda")
    return X.T @ X / (2 * k) + 1e-2 * torch.eye(k, dtype=torch.float64, device="cuda")


def tlut9():
    g = torch.Generator().manual_seed(9)
    t = torch.randn(512, 2, generator=g)
    return (t / t.std(unbiased=False) * 0.9682458365518543).half()


def layer_figures():
    out = []
    tlut = tlut9()
    lut_rms = ql.tcq_lut_rms(tlut)
    tl = tlut.cuda()
    for m, k in LAYERS:
        H = spd(k)
        W = (torch.randn(m, k, device="cuda") * 0.02).half()
        SU = ql.random_signs(k, device="cuda")
        for qstr in QSTRS:
            q = ql.parse_quantizer_str(qstr)
            rec = {"out": m, "in": k, "quantizer_str": qstr}
            rec["preprocess_s"], (Wr, _, HRr, _, _) = wall(lambda: ql.incoherent_preprocess(W, H, SU=SU, lut_rms=lut_rms))
            rec["ldl_s"], L = wall(lambda: quantize.block_ldl(HRr, 16))
            L.fill_diagonal_(0)
            W64 = Wr.to(torch.float64)
            if q["kind"] == "tcq":
                rec["ldlq_viterbi_s"], (_, Q) = wall(lambda: quantize._ldlq(W64, L, tl, q["KV"], 128))
                rec["pack_s"], _ = wall(lambda: packers.pack_trellis(Q.cpu(), m, k, q["KV"]))
            else:
                kv1, kv2 = q["KV"]
                p0 = k // 2
                rec["ldlq_viterbi_s"], (_, Q) = wall(lambda: quantize._ldlq(W64, L, tl, kv1, 128, kv_at=lambda r0: kv1 if r0 < p0 else kv2))
                rec["pack_s"], _ = wall(lambda: (packers.pack_trellis(Q[:, :p0 // 2].cpu().contiguous(), m, p0, kv1),
                                                 packers.pack_trellis(Q[:, p0 // 2:].cpu().contiguous(), m, k - p0, kv2)))
            del W64, L, HRr, Wr, Q
            rec["quantize_linear_s"], (_, info) = wall(lambda: ql.quantize_linear(W, qstr, H=H, SU=SU, codebooks={9: tlut}))
            rec["err"] = info["err"]
            print(json.dumps(rec), flush=True)
            out.append(rec)
        del H, W
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layer_quant_bench.json"))
    ap.add_argument("--rotate-only", action="store_true", help="only the rotation launches (the rocprofv3 run); writes nothing")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 kernel_stats.csv of a --rotate-only run")
    args = ap.parse_args()
    assert torch.cuda.is_available()
    rot = rotate_figures()
    print(json.dumps(rot), flush=True)
    if args.rotate_only:
        return
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_GBps": HBM_PEAK_GBS, "rotate_f32": rot}
    if args.kernel_stats:
        res["rotate_f32_rocprofv3"] = merge_kernel_stats(rot, args.kernel_stats)
    res["quantize_linear"] = layer_figures()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
