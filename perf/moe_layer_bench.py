"""One sparse layer under a HIP graph: the six launches of MoEMLP.run at batch 1 and 8, next to an IncoherentMLP of
intermediate width top_k * I at the same codec, which reads the same weight bytes at batch 1.

    python perf/moe_layer_bench.py [--shape mixtral | qwen3-30b-a3b] [--batch 1 8] [--no-dense] [--quantizer tcq_6_none_0.9]
                                   [--moe-router mixtral | qwen2 | deepseek_v2 | deepseek_v3] [--moe-shared IS] [--route]

--moe-router sets the router's fields (moe.router_preset), --moe-shared IS adds a shared expert of intermediate width
IS (gated for qwen2): the layer is then timed with it, without it, and next to a separate IncoherentMLP of width IS.  --route times
qpal_moe_route_ex against qpal_moe_route at the same shapes in the same call, and nothing else.

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


def dense_mlp(H, Id, q, seed=0):
    cfg = types.SimpleNamespace(hidden_size=H, intermediate_size=Id, hidden_act="silu")

    def info(k, m, s):
        return {"quant_info": qp.mem_op.get_quant_info(q), "in_features": k, "out_features": m, "dtype": torch.float16, "bias": None,
                "linear_info": qp.mem_op.dummy_linear_info(k, m, q, seed=s, codebook_seed=3), "SU": torch.ones(k, dtype=torch.float16),
                "Wscale": torch.ones(m, dtype=torch.float16)}
    return qp.IncoherentMLP.gen_layer_from_info(cfg, info(H, Id, seed + 1), info(H, Id, seed + 2), info(Id, H, seed + 3)).cuda()


def router_kwargs(name, E, K, H, gated=None):
    """moe.router_preset's fields with random tensors where the family has them: a select bias for deepseek_v3, a shared gate for qwen2"""
    kw = qp.moe.router_preset(name, E, K)
    if name == "deepseek_v3":
        kw["select_bias"] = (0.1 * torch.randn(E)).cuda()
    if name == "qwen2" if gated is None else gated:
        kw["shared_gate"] = (torch.randn(H) / H ** 0.5).half().cuda()
    return kw


ROUTE_SHAPES = ((2048, 128, 8, 1, 1), (7168, 256, 8, 8, 4))   # H, E, top_k, n_group, topk_group


def route_bench():
    """qpal_moe_route_ex (sigmoid, a select bias, "top2" groups where the shape has them, a shared gate) against qpal_moe_route"""
    for H, E, K, G, tg in ROUTE_SHAPES:
        rw = (torch.randn(E, H) / H ** 0.5).half().cuda()
        router = qp.moe.Router("sigmoid", (0.1 * torch.randn(E)).cuda(), G, tg, "top2", True, 2.5, (torch.randn(H) / H ** 0.5).half().cuda())
        for n in (1, 8, 128):
            h, w = torch.randn(n, H, device="cuda"), torch.ones(H, dtype=torch.float16, device="cuda")
            ws = qp.moe.moe_workspace(n, E, K, H, 32, "cuda", shared_I=32)
            old = timed(lambda: qp.moe.route(h, (1e-5, w), rw, None, K, True, ws))
            new = timed(lambda: qp.moe.route(h, (1e-5, w), rw, None, K, True, ws, router=router))
            print(json.dumps(dict(route=(n, H, E, K, G, tg), route_us=old[0], route_us_min=old[1], route_us_max=old[2], route_ex_us=new[0],
                                  route_ex_us_min=new[1], route_ex_us_max=new[2])), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="+", default=sorted(SHAPES), choices=sorted(SHAPES))
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--quantizer", default="tcq_6_none_0.9")
    ap.add_argument("--no-dense", action="store_true")
    ap.add_argument("--moe-router", default="mixtral", choices=qp.moe.ROUTER_PRESETS)
    ap.add_argument("--moe-shared", type=int, default=0, metavar="IS")
    ap.add_argument("--route", action="store_true")
    args = ap.parse_args(argv)
    if args.route:
        return route_bench()
    q = args.quantizer
    kv = sum(qp.mem_op.get_quant_info(q)["KV"]) / 2 if "tcomb" in q else qp.mem_op.get_quant_info(q)["KV"]
    for name in args.shape:
        H, I, E, K = SHAPES[name]
        su_h, su_i = torch.ones(H, dtype=torch.float16), torch.ones(I, dtype=torch.float16)
        experts = [(wrapped(H, I, q, 3 * e, su_h), wrapped(H, I, q, 3 * e + 1, su_h), wrapped(I, H, q, 3 * e + 2, su_i)) for e in range(E)]
        amp = 1.0 if args.moe_router == "deepseek_v3" else 4.0   # (4 / sqrt(H) saturates a sigmoid)
        router_w = (torch.randn(E, H) * amp / H ** 0.5).half().cuda()
        rkw = router_kwargs(args.moe_router, E, K, H, gated=None if args.moe_shared else False)
        shared = dense_mlp(H, args.moe_shared, q, seed=1000) if args.moe_shared else None
        layer = qp.MoEMLP.from_experts(router_w, experts, K, shared=shared, **rkw)
        bare = qp.MoEMLP.from_experts(router_w, experts, K, **{k: v for k, v in rkw.items() if k != "shared_gate"}) if shared is not None else None
        for B in args.batch:
            h, w = torch.randn(B, H, device="cuda"), torch.ones(H, dtype=torch.float16, device="cuda")
            out, ws = torch.zeros_like(h), layer.workspace(B)
            med, lo, hi = timed(lambda: layer.run(h, (1e-5, w), out, False, ws=ws))
            read = len(set(ws.sel.cpu().numpy().ravel().tolist()))
            res = dict(shape=name, B=B, quantizer=q, router=args.moe_router, shared_I=args.moe_shared, launches=layer.launches(B), moe_us=med,
                       moe_us_min=lo, moe_us_max=hi, ngroups=int(ws.ngroups[0]), experts_read=read,
                       routed_GBps=read * 3 * H * I * kv / 16 / med / 1e3)
            if shared is not None:   # the same layer without its shared expert, and that expert as a dense MLP of its own
                ws2, x = bare.workspace(B), h.half()
                res["moe_without_shared_us"], res["shared_alone_us"] = timed(lambda: bare.run(h, (1e-5, w), out, False, ws=ws2))[0], timed(lambda: shared(x))[0]
            print(json.dumps(res), flush=True)
        del layer, experts, bare, shared
        torch.cuda.empty_cache()
        if args.no_dense:
            continue
        Id = K * I
        mlp = dense_mlp(H, Id, q)
        for B in args.batch:
            x = torch.randn(B, H, device="cuda").half()
            med, lo, hi = timed(lambda: mlp(x))
            print(json.dumps(dict(shape=name, B=B, quantizer=q, dense_us=med, dense_us_min=lo, dense_us_max=hi, dense_I=Id)), flush=True)
        del mlp
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
