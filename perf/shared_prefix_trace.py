#!/usr/bin/env python3
"""Per-block kernel medians of `perf/attn_batch_bench.py --paged PAGE --shared-prefix P ...` run under `rocprofv3 --kernel-trace
--output-format csv`: the call times, per row and --repeats times in turn, a block of 10 + iters plain paged
launches and a block of 10 + iters shared pairs (prefix kernel + suffix kernel).  Per block: the median over its last `iters`
launches (the pair: the sum of its two kernels).  Per row: the plain medians, their spread (max - min), the shared medians, and
whether the WORST shared median beats the BEST plain median by more than that spread.

    python perf/shared_prefix_trace.py <kernel_trace.csv> <bench.json>  >  profiles/shared_prefix.json
"""
import csv
import json
import statistics
import sys


def kind(name):
    if "attn_prefix_kernel" in name:
        return "prefix"
    if "attn_rope_batch_kernel" in name:
        return "suffix" if name.split("attn_rope_batch_kernel<")[1].split(">")[0].replace(" ", "").endswith("true") else "plain"
    return None


def main():
    trace, bench = sys.argv[1], json.loads(open(sys.argv[2]).read().strip().split("\n")[-1])
    ev = []
    for r in csv.DictReader(open(trace)):
        k = kind(r["Kernel_Name"])
        if k:
            ev.append((int(r["Start_Timestamp"]), k, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    ev.sort()
    blocks = []  # (plain | shared, [per-launch us], [prefix us], [suffix us])
    for _, k, us in ev:
        side = "plain" if k == "plain" else "shared"
        if not blocks or blocks[-1][0] != side:
            blocks.append((side, [], [], []))
        b = blocks[-1]
        if k == "plain":
            b[1].append(us)
        elif k == "prefix":
            b[2].append(us)
        else:
            b[3].append(us)
            b[1].append(b[2][-1] + us)
    it = iter(blocks)
    med = lambda xs, n: statistics.median(xs[-n:])  # noqa: E731
    for row in bench["rows"]:
        n, res = row["iters"], {"plain": [], "shared": [], "prefix": [], "suffix": []}
        for _ in range(row["repeats"]):
            for side in ("plain", "shared"):
                b = next(it)
                assert b[0] == side and len(b[1]) == 10 + n, (b[0], side, len(b[1]))
                res[side].append(round(med(b[1], n), 2))
                if side == "shared":
                    res["prefix"].append(round(med(b[2], n), 2))
                    res["suffix"].append(round(med(b[3], n), 2))
        spread = max(res["plain"]) - min(res["plain"])
        row.update({"us_kernel_plain_medians": res["plain"], "us_kernel_shared_pair_medians": res["shared"],
                    "us_kernel_prefix_medians": res["prefix"], "us_kernel_suffix_medians": res["suffix"],
                    "plain_spread_us": round(spread, 2),
                    "shared_beats_plain_by_more_than_the_spread": max(res["shared"]) < min(res["plain"]) - spread})
    bench["method"] = "rocprofv3 --kernel-trace, median of the last `iters` launches of every block"
    print(json.dumps(bench, indent=1))


if __name__ == "__main__":
    main()
