#!/usr/bin/env python3
"""Prefill attention alone (qpalette_amd.prefill_attention, csrc/attn_prefill.hip): time per launch next to its FLOP count
4 nq hd sum_t (pos0 + t + 1), and torch SDPA on the same (already rotated) q and cache under a causal mask in the same call.
Event timing here; for the kernel time proper run it under `rocprofv3 --kernel-trace --stats -- python perf/attn_prefill_bench.py`.

--kv fp8: float8_e4m3fn caches; torch SDPA then runs on their fp16 image.

--paged PAGE_SIZE ...: per row also the same cache scattered into page pools (pages in a seeded random order) through
qpalette_amd.paged_prefill_attention, once per page size ("us_paged"), and the contiguous launch a second time
("us_prefill_attention_again": the spread the paged times are read against).

--window W: per row also the launch with window=W on the same cache ("us_window"; "keys_window": the keys its rows
attend to, sum_t min(pos0 + t + 1, W), next to "keys": sum_t (pos0 + t + 1)), then the plain launch again ("us_prefill_attention_again").

--softcap CAP / --sinks: per row also the launch with softcap=CAP ("us_cap"), with sinks of N(0, 1) per head
("us_sinks") and with both ("us_cap_sinks"), then the plain launch again ("us_prefill_attention_again").

    python perf/attn_prefill_bench.py [--softcap CAP] [--sinks] [--T 128] [--pos0 0 1920 3968] [--context 4096] [--heads 32 8 128] [--iters 50] [--kv fp16|fp8]
                                      [--paged 16 64] [--window W]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import qpalette_amd as qp
from paged import random_table, scatter


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=128)
    ap.add_argument("--pos0", type=int, nargs="+", default=[0, 1920, 3968])
    ap.add_argument("--context", type=int, default=4096)
    ap.add_argument("--heads", type=int, nargs=3, default=[32, 8, 128], metavar=("NQ", "NKV", "HD"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--kv", default="fp16", choices=["fp16", "fp8"], help="KV-cache element format")
    ap.add_argument("--paged", type=int, nargs="*", default=[], metavar="PAGE_SIZE", help="also time paged launches of these page sizes")
    ap.add_argument("--window", type=int, default=None, metavar="W", help="also time the launch with this sliding window")
    ap.add_argument("--softcap", type=float, default=None, metavar="CAP", help="also time the launch with this logit soft cap")
    ap.add_argument("--sinks", action="store_true", help="also time the launch with per-head sinks")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    dev = torch.device("cuda", 0)
    (nq, nkv, hd), T, L = args.heads, args.T, args.context
    gen = torch.Generator(device=dev).manual_seed(1)
    qkv = torch.randn(T, (nq + 2 * nkv) * hd, device=dev, generator=gen)
    q, k, v = qkv.split([nq * hd, nkv * hd, nkv * hd], dim=1)
    kc = (torch.randn(nkv, L, hd, device=dev, generator=gen) * 0.5).half()
    vc = (torch.randn(nkv, L, hd, device=dev, generator=gen) * 0.5).half()
    if args.kv == "fp8":
        kc, vc = kc.to(torch.float8_e4m3fn), vc.to(torch.float8_e4m3fn)
    inv_freq = 1.0 / (500000.0 ** (torch.arange(0, hd, 2, device=dev).float() / hd))
    ws = qp.prefill_workspace(T, nq, nkv, hd, L, dev)
    out = torch.empty(T, nq * hd, dtype=torch.float16, device=dev)

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.iters * 1e3  # us

    rows = []
    for pos0 in args.pos0:
        pos_t = torch.tensor([pos0], dtype=torch.long, device=dev)
        us = timed(lambda: qp.prefill_attention(q, k, v, kc, vc, pos_t, inv_freq, out=out, ws=ws))
        n = pos0 + T
        q16 = torch.randn(1, nq, T, hd, device=dev, generator=gen).half()
        kk = kc[None, :, :n].half().repeat_interleave(nq // nkv, dim=1)
        vv = vc[None, :, :n].half().repeat_interleave(nq // nkv, dim=1)
        mask = torch.arange(n, device=dev)[None, :] <= (pos0 + torch.arange(T, device=dev))[:, None]
        us_sdpa = timed(lambda: torch.nn.functional.scaled_dot_product_attention(q16, kk, vv, attn_mask=mask))
        flop = 4 * nq * hd * sum(pos0 + t + 1 for t in range(T))
        rows.append({"T": T, "pos0": pos0, "kv": args.kv, "flop": flop, "us_prefill_attention": us, "tflops": flop / us * 1e-6,
                     "us_torch_sdpa_causal_mask": us_sdpa})
        if args.softcap is not None or args.sinks:
            sinks = torch.randn(nq, generator=torch.Generator().manual_seed(9)).to(dev) if args.sinks else None
            mods = ([("cap", dict(softcap=args.softcap))] if args.softcap is not None else []) + ([("sinks", dict(sinks=sinks))] if args.sinks else [])
            if len(mods) == 2:
                mods.append(("cap_sinks", dict(softcap=args.softcap, sinks=sinks)))
            for name, kw in mods:
                rows[-1]["us_" + name] = timed(lambda: qp.prefill_attention(q, k, v, kc, vc, pos_t, inv_freq, out=out, ws=ws, **kw))
            if not args.paged and not args.window:
                rows[-1]["us_prefill_attention_again"] = timed(lambda: qp.prefill_attention(q, k, v, kc, vc, pos_t, inv_freq, out=out, ws=ws))
        if args.window:
            rows[-1].update({"window": args.window, "keys": sum(pos0 + t + 1 for t in range(T)),
                             "keys_window": sum(min(pos0 + t + 1, args.window) for t in range(T)),
                             "us_window": timed(lambda: qp.prefill_attention(q, k, v, kc, vc, pos_t, inv_freq, out=out, ws=ws, window=args.window))})
            if not args.paged:
                rows[-1]["us_prefill_attention_again"] = timed(lambda: qp.prefill_attention(q, k, v, kc, vc, pos_t, inv_freq, out=out, ws=ws))
        if args.paged:
            rows[-1]["us_paged"] = {}
            for ps in args.paged:
                table = random_table(1, L // ps, L // ps, L + ps, dev)
                kp, vp = scatter(kc[None], table, ps, L // ps), scatter(vc[None], table, ps, L // ps)
                rows[-1]["us_paged"][str(ps)] = timed(
                    lambda: qp.paged_prefill_attention(q, k, v, kp, vp, table[0], pos_t, inv_freq, out=out, ws=ws))
            rows[-1]["us_prefill_attention_again"] = timed(lambda: qp.prefill_attention(q, k, v, kc, vc, pos_t, inv_freq, out=out, ws=ws))
    print(json.dumps({"what": "prefill attention launch (event timing) vs torch SDPA on the same shapes", "heads": args.heads,
                      "context": L, "rows": rows}))


if __name__ == "__main__":
    main()
