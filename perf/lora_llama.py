#!/usr/bin/env python3
"""What low-rank adapters cost a decode step: DecodeStep under graph replay, same model, same B, one call.

The model is perf/decode_llama.py's (random layers of this package's modules), the adapters are random matrices on all seven
linears of every layer.  Per B:

  ms_plain    the step without a bank (B = 1: the fused batch-1 step)
  ms_no_epi   B = 1 only: the step without a bank and with swiglu_epilogue=False — the GEMV launches a step with a bank runs
  per (rank, distinct adapters d):
  ms_idle     a bank whose slots are all -1: four launches per layer that read row_adapter and leave
  ms_lora     slot b runs adapter b % d  (d = 1: every slot the same adapter; d = 8: eight different ones, B >= 8 only)

Every figure comes from the same process on the same device: only ratios inside one output file mean anything.

    python perf/lora_llama.py [--model 3_8b] [--batch 1 8 64] [--rank 16 64] [--adapters 1 8] [--context 1024] [--replays 32] [--out F]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

import qpalette_amd as qp
from decode_llama import build_model, time_graph


def random_adapter(m, rank, gen, dev):
    """{f"{layer}_{linear}": (A [rank, k], B [m, rank])} on every linear, generated on the device"""
    H, I, kv = m.cfg.hidden_size, m.cfg.intermediate_size, m.cfg.num_key_value_heads * m.cfg.head_dim
    shapes = {"self_attn.q_proj": (H, H), "self_attn.k_proj": (H, kv), "self_attn.v_proj": (H, kv), "self_attn.o_proj": (H, H),
              "mlp.up_proj": (H, I), "mlp.gate_proj": (H, I), "mlp.down_proj": (I, H)}
    return {f"{i}_{lin}": (torch.randn(rank, k, device=dev, generator=gen) / k ** 0.5, torch.randn(n, rank, device=dev, generator=gen) * 0.02)
            for i in range(len(m.layers)) for lin, (k, n) in shapes.items()}


def main(argv=None, quiet=False):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="3_8b", choices=sorted(qp.mem_op.LAYER_INFO))
    ap.add_argument("--quantizer", default="tcomb_6_7_0.5_none_0.9")
    ap.add_argument("--qdict", default=None)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--rank", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--adapters", type=int, nargs="+", default=[1, 8], help="distinct adapters among the slots")
    ap.add_argument("--context", type=int, default=1024)
    ap.add_argument("--replays", type=int, default=32)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    dev = torch.device("cuda", 0)
    m = build_model(args.model, args.quantizer, args.qdict, args.layers, args.vocab, dev)
    nkv, hd, nl = m.cfg.num_key_value_heads, m.cfg.head_dim, len(m.layers)
    n0 = args.context // 2
    results = []
    for B in args.batch:
        cg = torch.Generator(device=dev).manual_seed(args.seed)
        kc = [(torch.randn(B, nkv, args.context, hd, device=dev, generator=cg) * 0.5).half() for _ in range(nl)]
        vc = [(torch.randn(B, nkv, args.context, hd, device=dev, generator=cg) * 0.5).half() for _ in range(nl)]
        tok = torch.randint(0, args.vocab, (B,), generator=torch.Generator().manual_seed(args.seed + B)).to(dev)
        pos = torch.full((B,), n0 - 1, dtype=torch.long, device=dev)
        out_tok = torch.zeros(B, dtype=torch.long, device=dev)

        def timed(**kw):
            ds = qp.DecodeStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, tok, pos, out_tok, **kw)
            return time_graph(ds, args.replays, dev), ds.launches_per_token

        ms_plain, launches_plain = timed()
        res = {"batch": B, "ms_plain": ms_plain, "launches_plain": launches_plain, "runs": []}
        if B == 1:
            res["ms_no_epi"], res["launches_no_epi"] = timed(swiglu_epilogue=False)
        for rank in args.rank:
            for d in args.adapters:
                if d > B and d > 1:
                    continue
                bank = qp.LoraBank(m.layers, n_adapters=d, rank=rank, B_slots=B, device=dev)
                for a in range(d):
                    bank.load(a, random_adapter(m, rank, cg, dev), alpha=2.0 * rank)
                ms_idle, launches = timed(adapters=bank)
                for b in range(B):
                    bank.set(b, b % d)
                ms_lora, _ = timed(adapters=bank)
                run = {"rank": rank, "distinct_adapters": d, "ms_idle": ms_idle, "ms_lora": ms_lora, "launches": launches,
                       "bank_MiB": bank.bytes() / 2 ** 20, "lora_over_plain": ms_lora / ms_plain, "idle_over_plain": ms_idle / ms_plain,
                       "us_per_lora_launch": (ms_lora - res.get("ms_no_epi", ms_plain)) * 1e3 / (4 * nl),
                       "us_per_idle_launch": (ms_idle - res.get("ms_no_epi", ms_plain)) * 1e3 / (4 * nl)}
                res["runs"].append(run)
                if not quiet:
                    print(json.dumps({"batch": B, "ms_plain": ms_plain, **run}), file=sys.stderr, flush=True)
                del bank
                torch.cuda.empty_cache()
        results.append(res)
        del kc, vc
        torch.cuda.empty_cache()
    out = {"what": "DecodeStep with a LoraBank against the step without one, ms per graph replay, one process",
           "model": args.model, "layers": nl, "quantizer": args.qdict or args.quantizer, "context": args.context, "position": n0 - 1,
           "replays": args.replays, "results": results}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    if not quiet:
        print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
