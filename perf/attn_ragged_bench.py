#!/usr/bin/env python3
"""Ragged prefill attention alone (qpalette_amd.ragged_prefill_attention, csrc/attn_ragged.hip): ONE launch on R = 128 rows cut
evenly into S segments of S sequences against S sequential prefill_attention launches on the same data, kernel time in us.

The times are the kernels' own: the script starts a child of itself under `rocprofv3 --kernel-trace --stats` (a fresh process, the
program behind `--`), the child runs every case in a fixed order, and the parent cuts the trace's attention dispatches, in start
order, by that schedule.  Per case: sequence b holds context - T_s positions and takes T_s = 128 / S new rows (the launch reads
`context` keys per sequence); `us_ragged` is the mean over --iters launches, `us_sequential` the mean over --iters passes of the SUM
of the S one-sequence launches.  Paged cases scatter the same caches into page pools (pages in a seeded random order) and compare
paged_ragged_prefill_attention with S paged_prefill_attention launches.

    python perf/attn_ragged_bench.py [--S 1 8 64] [--context 1024 4096] [--kv fp16 fp8] [--paged 16] [--heads 32 8 128] [--iters 10]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

R, WARM = 128, 2


def cases(args):
    return [(kv, ps, L, S) for kv in args.kv for ps in [0] + args.paged for L in args.context for S in args.S]


def child(args):
    import torch

    import qpalette_amd as qp
    from paged import random_table, scatter
    dev = torch.device("cuda", 0)
    nq, nkv, hd = args.heads
    inv_freq = 1.0 / (500000.0 ** (torch.arange(0, hd, 2, device=dev).float() / hd))
    gen = torch.Generator(device=dev).manual_seed(1)
    qkv = torch.randn(R, (nq + 2 * nkv) * hd, device=dev, generator=gen)
    q, k, v = qkv.split([nq * hd, nkv * hd, nkv * hd], dim=1)
    out = torch.empty(R, nq * hd, dtype=torch.float16, device=dev)
    for kv, ps, L, S in cases(args):
        T = R // S
        kc = (torch.randn(S, nkv, L, hd, device=dev, generator=gen) * 0.5).half()
        vc = (torch.randn(S, nkv, L, hd, device=dev, generator=gen) * 0.5).half()
        if kv == "fp8":
            kc, vc = kc.to(torch.float8_e4m3fn), vc.to(torch.float8_e4m3fn)
        seq = torch.arange(S, dtype=torch.int32, device=dev)
        row0 = torch.arange(0, R + 1, T, dtype=torch.int32, device=dev)
        pos0 = torch.full((S,), L - T, dtype=torch.int64, device=dev)
        pos1 = pos0[:1].clone()
        ws_r = qp.ragged_workspace(R, S, nq, nkv, hd, L, dev)
        ws_p = qp.prefill_workspace(T, nq, nkv, hd, L, dev)
        if ps:
            table = random_table(S, L // ps, S * (L // ps), L + ps + S, dev)
            kp, vp = scatter(kc, table, ps, S * (L // ps)), scatter(vc, table, ps, S * (L // ps))
            ragged = lambda: qp.paged_ragged_prefill_attention(q, k, v, kp, vp, table, seq, row0, pos0, inv_freq, out=out, ws=ws_r)
            one = lambda b: qp.paged_prefill_attention(q[b * T:(b + 1) * T], k[b * T:(b + 1) * T], v[b * T:(b + 1) * T], kp, vp, table[b],
                                                       pos1, inv_freq, out=out[b * T:(b + 1) * T], ws=ws_p)
        else:
            ragged = lambda: qp.ragged_prefill_attention(q, k, v, kc, vc, seq, row0, pos0, inv_freq, out=out, ws=ws_r)
            one = lambda b: qp.prefill_attention(q[b * T:(b + 1) * T], k[b * T:(b + 1) * T], v[b * T:(b + 1) * T], kc[b], vc[b], pos1,
                                                 inv_freq, out=out[b * T:(b + 1) * T], ws=ws_p)
        for _ in range(WARM + args.iters):
            ragged()
        for _ in range(WARM + args.iters):
            for b in range(S):
                one(b)
        torch.cuda.synchronize()
        del kc, vc


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, nargs="+", default=[1, 8, 64], help="segments (divisors of 128)")
    ap.add_argument("--context", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--kv", nargs="+", default=["fp16", "fp8"], choices=["fp16", "fp8"])
    ap.add_argument("--paged", type=int, nargs="*", default=[16], metavar="PAGE_SIZE")
    ap.add_argument("--heads", type=int, nargs=3, default=[32, 8, 128], metavar=("NQ", "NKV", "HD"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if any(R % s for s in args.S):
        raise SystemExit("--S: divisors of 128")
    if args.child:
        return child(args)
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "ragged", "--output-format", "csv", "--", sys.executable,
               os.path.abspath(__file__), "--child"] + [a for a in (argv if argv is not None else sys.argv[1:])]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=900)
        traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if len(traces) != 1:
            raise SystemExit(f"expected one kernel trace, found {traces}")
        with open(traces[0]) as f:
            rows = [r for r in csv.DictReader(f) if "attn_prefill_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3 for r in rows]
    res, at = [], 0
    for kv, ps, L, S in cases(args):
        n_r, n_s = WARM + args.iters, (WARM + args.iters) * S
        rag, seqn = us[at + WARM:at + n_r], us[at + n_r + WARM * S:at + n_r + n_s]
        at += n_r + n_s
        res.append({"kv": kv, "paged": ps, "context": L, "S": S, "rows_per_segment": R // S, "us_ragged": sum(rag) / len(rag),
                    "us_sequential": sum(seqn) / args.iters, "launches_sequential": S})
    if at != len(us):
        raise SystemExit(f"the trace holds {len(us)} attention dispatches, the schedule {at}")
    print(json.dumps({"what": "one ragged prefill launch (R = 128 rows, S segments) vs S one-sequence launches, kernel us (rocprofv3)",
                      "heads": args.heads, "iters": args.iters, "rows": res}))


if __name__ == "__main__":
    main()
