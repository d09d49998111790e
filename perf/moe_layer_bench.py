"""One sparse layer under a HIP graph: the six launches of MoEMLP.run at batch 1 and 8, next to an IncoherentMLP of
intermediate width top_k * I at the same codec, which reads the same weight bytes at batch 1.

    python perf/moe_layer_bench.py [--shape mixtral | qwen3-30b-a3b] [--batch 1 8] [--no-dense] [--quantizer tcq_6_none_0.9]

Random packed experts, one codebook.  Prints one JSON line per measurement: median (min, max) microseconds of 30 replays, the experts
the routing read and the routed bytes per second over the whole layer.  For per-kernel times run it alone under a kernel trace:
`rocprofv3 --kernel-trace --stats -- python perf/moe_layer_bench.py --shape qwen3-30b-a3b --batch 1 --no-dense`."""
import argparse
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__  # noqa: E402,F401
import qpalette_amd as qp  # noqa: E402

SHAPES = {"mixtral": (4096, 14336, 8, 2), "qwen3-30b-a3b": (2048, 768, 128, 8)}   # H, I, E, top_k


def wrapped(k, m, qstr, seed, su):
    il = qp.IncoherentLinear(k, m, k, m, use_linear=False)
    il.linear = qp.make_linear_from_info(qstr, qp.mem_op.dummy_linear_info(k, m, qstr, seed=seed, codebook_seed=3))
    il.SU.data.copy_(su)
    il.rot_info = "skip_r"
    il.apply_rot_info()
    return il.cuda()


def timed(fn, iters=30):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(5):
        g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="+", default=sorted(SHAPES), choices=sorted(SHAPES))
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--quantizer", default="tcq_6_none_0.9")
    ap.add_argument("--no-dense", action="store_true")
    args = ap.parse_args(argv)
    q = args.quantizer
    kv = sum(qp.mem_op.get_quant_info(q)["KV"]) / 2 if "tcomb" in q else qp.mem_op.get_quant_info(q)["KV"]
    for name in args.shape:
        H, I, E, K = SHAPES[name]
        su_h, su_i = torch.ones(H, dtype=torch.float16), torch.ones(I, dtype=torch.float16)
        experts = [(wrapped(H, I, q, 3 * e, su_h), wrapped(H, I, q, 3 * e + 1, su_h), wrapped(I, H, q, 3 * e + 2, su_i)) for e in range(E)]
        layer = qp.MoEMLP.from_experts((torch.randn(E, H) * 4 / H ** 0.5).half().cuda(), experts, K)
        for B in args.batch:
            h, w = torch.randn(B, H, device="cuda"), torch.ones(H, dtype=torch.float16, device="cuda")
            out, ws = torch.zeros_like(h), layer.workspace(B)
            med, lo, hi = timed(lambda: layer.run(h, (1e-5, w), out, False, ws=ws))
            read = len(set(ws.sel.cpu().numpy().ravel().tolist()))
            print(json.dumps(dict(shape=name, B=B, quantizer=q, moe_us=med, moe_us_min=lo, moe_us_max=hi, ngroups=int(ws.ngroups[0]),
                                  experts_read=read, routed_GBps=read * 3 * H * I * kv / 16 / med / 1e3)), flush=True)
        del layer, experts
        torch.cuda.empty_cache()
        if args.no_dense:
            continue
        Id = K * I
        cfg = types.SimpleNamespace(hidden_size=H, intermediate_size=Id, hidden_act="silu")

        def info(k, m, s):
            return {"quant_info": qp.mem_op.get_quant_info(q), "in_features": k, "out_features": m, "dtype": torch.float16, "bias": None,
                    "linear_info": qp.mem_op.dummy_linear_info(k, m, q, seed=s, codebook_seed=3), "SU": torch.ones(k, dtype=torch.float16),
                    "Wscale": torch.ones(m, dtype=torch.float16)}
        mlp = qp.IncoherentMLP.gen_layer_from_info(cfg, info(H, Id, 1), info(H, Id, 2), info(Id, H, 3)).cuda()
        for B in args.batch:
            x = torch.randn(B, H, device="cuda").half()
            med, lo, hi = timed(lambda: mlp(x))
            print(json.dumps(dict(shape=name, B=B, quantizer=q, dense_us=med, dense_us_min=lo, dense_us_max=hi, dense_I=Id)), flush=True)
        del mlp
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
