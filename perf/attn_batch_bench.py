#!/usr/bin/env python3
"""Batched decode attention alone (qpalette_amd.decode_attention, csrc/attn_batch.hip): time per launch and achieved KV bytes/s.

Llama-3 8B heads (32 query / 8 kv heads, hd 128) unless told otherwise.  Positions are ragged and seeded (uniform over the cache)
or, with --full, every sequence at max_len - 1.  The bytes are the K and V rows the launch has to read, sum_b (pos[b] + 1) rows of
nkv * hd elements each (2 bytes with --kv fp16, 1 with --kv fp8: float8_e4m3fn caches), not B * max_len.
Back-to-back launches timed with events; under `rocprofv3 --kernel-trace --stats` the kernel's own time comes from the trace (the
two formats run different kernel instantiations; with both named, every row runs fp16 first, then fp8, 10 + iters launches each).

--paged PAGE_SIZE ...: after the contiguous launch of a row, the same caches scattered into page pools (pages handed out in a seeded
random order) through qpalette_amd.paged_decode_attention, once per page size, then the contiguous launch AGAIN (its two timings are
the spread the paged ones are read against).  "pool_bytes": what the pools of a cache that backs only the positions in
use would take (sum_b ceil((pos[b] + 1) / page_size) pages), against "cache_bytes".

--paged PAGE --shared-prefix P ...: the B slots share the pages of a P-position prefix and have 1 .. 256 seeded positions of
their own each (max_len = P + 512; --context and --full are not used).  On ONE pair of pools, --repeats times in turn: the plain
paged launch, then the shared pair (qpalette_amd.shared_prefix_decode_attention), 10 + iters launches each.  Under
`rocprofv3 --kernel-trace` perf/shared_prefix_trace.py turns the trace of this call into per-block medians.

--window W (0: context / 4 of every row): behind the contiguous launch of a row, the same launch with window=W on the
same caches and positions: "us_per_launch_events_window" next to "kv_rows_window" = sum_b min(pos[b] + 1, W), the rows it has to read.

--softcap CAP / --sinks: behind the contiguous launch of a row, the same launch with softcap=CAP
("us_per_launch_events_cap"), with sinks of N(0, 1) per head ("..._sinks") and with both ("..._cap_sinks"), then the plain launch
again ("us_per_launch_events_again": the spread the three are read against).  Under `rocprofv3 --kernel-trace --stats` the plain and
the modified launches are two kernel names (attn_rope_batch_kernel<..., false, false> and <..., true, true>).

    python perf/attn_batch_bench.py [--softcap CAP] [--sinks] [--batch 8 64] [--context 1024 4096] [--iters 200] [--full] [--kv fp16 fp8] [--paged 16 64]
                                    [--shared-prefix 4096 1024] [--repeats 5] [--window W]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import qpalette_amd as qp
from paged import random_table, scatter


def shared_rows(args, dev, inv_freq):
    """the plain paged launch and the shared pair in turn on the same pools, per (prefix, batch, format)"""
    nq, nkv, hd, ps = args.nq, args.nkv, args.hd, args.paged[0]
    rows = []
    for P in args.shared_prefix:
        for B in args.batch:
            L = P + 512
            mp, shared_pages = L // ps, P // ps
            own = mp - shared_pages
            num_pages = shared_pages + B * own
            g = torch.Generator().manual_seed(B * 7 + P)
            pos_h = P + torch.randint(1, 257, (B,), generator=g)
            perm = torch.randperm(num_pages, generator=g).to(torch.int32)
            table = torch.empty(B, mp, dtype=torch.int32)
            table[:, :shared_pages] = perm[:shared_pages]
            table[:, shared_pages:] = perm[shared_pages:].view(B, own)
            table, pos = table.to(dev), pos_h.to(dev)
            qkv = torch.randn(B, (nq + 2 * nkv) * hd, device=dev)
            q, k, v = qkv.split([nq * hd, nkv * hd, nkv * hd], dim=1)
            out = torch.empty(B, nq * hd, dtype=torch.float16, device=dev)
            i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)  # noqa: E731
            px = qp.SharedPrefix(i32([0] * B), i32([0]), i32([P]))
            ws_plain = qp.attention_workspace(B, nq, nkv, hd, L, dev)
            ws_shared = qp.shared_prefix_workspace(B, 1, nq, nkv, hd, L, dev)
            for kv in args.kv:
                dtype = torch.float16 if kv == "fp16" else torch.float8_e4m3fn
                kp, vp = (torch.randn(num_pages, nkv, ps, hd, device=dev).half().to(dtype) for _ in range(2))
                plain = lambda: qp.paged_decode_attention(q, k, v, kp, vp, table, pos, inv_freq, out=out, ws=ws_plain)  # noqa: E731
                shared = lambda: qp.shared_prefix_decode_attention(q, k, v, kp, vp, table, pos, inv_freq, px, out=out, ws=ws_shared)  # noqa: E731
                us = {"plain": [], "shared": []}
                for _ in range(args.repeats):
                    for name, launch in (("plain", plain), ("shared", shared)):
                        for _ in range(10):
                            launch()
                        torch.cuda.synchronize()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(args.iters):
                            launch()
                        e1.record()
                        torch.cuda.synchronize()
                        us[name].append(e0.elapsed_time(e1) * 1e3 / args.iters)
                esz = kp.element_size()
                rows.append({"batch": B, "prefix": P, "max_len": L, "page_size": ps, "kv": kv, "iters": args.iters, "repeats": args.repeats,
                             "kv_rows_plain": int((pos_h + 1).sum()), "kv_rows_shared": int(P + (pos_h + 1 - P).sum()),
                             "kv_MB_plain": int((pos_h + 1).sum()) * nkv * hd * 2 * esz / 1e6,
                             "us_per_launch_events_plain": us["plain"], "us_per_launch_events_shared_pair": us["shared"],
                             "workspace_bytes_plain": 0 if ws_plain is None else ws_plain.numel() * 4,
                             "workspace_bytes_shared": ws_shared.numel() * 4})
                del kp, vp
            torch.cuda.empty_cache()
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--context", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--nq", type=int, default=32)
    ap.add_argument("--nkv", type=int, default=8)
    ap.add_argument("--hd", type=int, default=128)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--full", action="store_true", help="every sequence at the last position of its cache")
    ap.add_argument("--kv", nargs="+", default=["fp16"], choices=["fp16", "fp8"], help="KV-cache element format(s), in this order per row")
    ap.add_argument("--paged", type=int, nargs="*", default=[], metavar="PAGE_SIZE", help="also time paged launches of these page sizes")
    ap.add_argument("--shared-prefix", type=int, nargs="*", default=[], metavar="P",
                    help="with --paged PAGE: slots that share a P-position prefix, the plain launch against the shared pair")
    ap.add_argument("--repeats", type=int, default=5, help="--shared-prefix: timed blocks of each launch, in turn")
    ap.add_argument("--window", type=int, default=None, metavar="W", help="also time the launch with this sliding window (0: context / 4)")
    ap.add_argument("--softcap", type=float, default=None, metavar="CAP", help="also time the launch with this logit soft cap")
    ap.add_argument("--sinks", action="store_true", help="also time the launch with per-head sinks")
    args = ap.parse_args(argv)
    if args.shared_prefix and (len(args.paged) != 1 or any(P % args.paged[0] or P < args.paged[0] for P in args.shared_prefix)):
        raise SystemExit("--shared-prefix: with ONE --paged PAGE, prefixes that are multiples of it")
    dev = torch.device("cuda", 0)
    nq, nkv, hd = args.nq, args.nkv, args.hd
    inv_freq = 1.0 / (500000.0 ** (torch.arange(0, hd, 2, device=dev).float() / hd))
    if args.shared_prefix:
        print(json.dumps({"what": "paged decode attention of slots that share a prefix: the plain launch and the shared pair in turn",
                          "nq": nq, "nkv": nkv, "hd": hd, "rows": shared_rows(args, dev, inv_freq)}))
        return
    rows = []
    for L in args.context:
        for B in args.batch:
            g = torch.Generator().manual_seed(B * 7 + L)
            pos_h = torch.full((B,), L - 1, dtype=torch.long) if args.full else torch.randint(0, L, (B,), generator=g)
            pos = pos_h.to(dev)
            qkv = torch.randn(B, (nq + 2 * nkv) * hd, device=dev)
            q, k, v = qkv.split([nq * hd, nkv * hd, nkv * hd], dim=1)
            kc16 = torch.randn(B, nkv, L, hd, device=dev).half()
            vc16 = torch.randn(B, nkv, L, hd, device=dev).half()
            out = torch.empty(B, nq * hd, dtype=torch.float16, device=dev)
            ws = qp.attention_workspace(B, nq, nkv, hd, L, dev)
            for kv in args.kv:
                kc, vc = (kc16, vc16) if kv == "fp16" else (kc16.to(torch.float8_e4m3fn), vc16.to(torch.float8_e4m3fn))
                kv_rows = int((pos_h + 1).sum())
                nbytes = kv_rows * nkv * hd * 2 * kc.element_size()
                for ps in [0] + args.paged + ([0] if args.paged else []):  # 0: contiguous (again at the end: the spread)
                    if ps:
                        table = random_table(B, L // ps, B * (L // ps), B + L + ps, dev)
                        kp, vp = scatter(kc, table, ps, B * (L // ps)), scatter(vc, table, ps, B * (L // ps))
                        launch = lambda: qp.paged_decode_attention(q, k, v, kp, vp, table, pos, inv_freq, out=out, ws=ws)  # noqa: E731
                    else:
                        launch = lambda: qp.decode_attention(q, k, v, kc, vc, pos, inv_freq, out=out, ws=ws)  # noqa: E731
                    def timed(launch):
                        for _ in range(10):
                            launch()
                        torch.cuda.synchronize()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(args.iters):
                            launch()
                        e1.record()
                        torch.cuda.synchronize()
                        return e0.elapsed_time(e1) * 1e3 / args.iters

                    us = timed(launch)
                    row = {"batch": B, "context": L, "kv": kv, "full": args.full, "kv_rows": kv_rows, "kv_MB": nbytes / 1e6,
                           "us_per_launch_events": us, "TBps_events": nbytes / (us * 1e-6) / 1e12,
                           "workspace_bytes": 0 if ws is None else ws.numel() * 4,
                           "cache_bytes": 2 * qp.attention.kv_cache_bytes(B, nkv, L, hd, kc.dtype)}
                    if args.window is not None and not ps:
                        W = args.window or L // 4
                        rows_w = int(torch.clamp(pos_h + 1, max=W).sum())
                        us_w = timed(lambda: qp.decode_attention(q, k, v, kc, vc, pos, inv_freq, out=out, ws=ws, window=W))
                        row.update({"window": W, "kv_rows_window": rows_w, "kv_MB_window": rows_w * nkv * hd * 2 * kc.element_size() / 1e6,
                                    "us_per_launch_events_window": us_w})
                    if (args.softcap is not None or args.sinks) and not ps:
                        sinks = torch.randn(nq, generator=torch.Generator().manual_seed(9)).to(dev) if args.sinks else None
                        mods = ([("cap", dict(softcap=args.softcap))] if args.softcap is not None else []) + ([("sinks", dict(sinks=sinks))] if args.sinks else [])
                        if len(mods) == 2:
                            mods.append(("cap_sinks", dict(softcap=args.softcap, sinks=sinks)))
                        for name, kw in mods:
                            row["us_per_launch_events_" + name] = timed(lambda: qp.decode_attention(q, k, v, kc, vc, pos, inv_freq, out=out, ws=ws, **kw))
                        row["us_per_launch_events_again"] = timed(launch)
                    if args.paged:
                        row["paged"] = ps
                    if ps:
                        pages = int(((pos_h + ps) // ps).sum())
                        row["pool_bytes"] = 2 * qp.attention.kv_cache_bytes(pages, nkv, ps, hd, kc.dtype)
                        del kp, vp, table
                    rows.append(row)
                del kc, vc
            del kc16, vc16
            torch.cuda.empty_cache()
    print(json.dumps({"what": "batched decode attention, one launch", "nq": nq, "nkv": nkv, "hd": hd, "rows": rows}))


if __name__ == "__main__":
    main()
