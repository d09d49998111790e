#!/usr/bin/env python3
"""Speculative decode step against the plain decode step, same model, same B, both under graph replay.

The model is perf/decode_llama.py's (random layers of this package's modules).  Every slot holds a random history of --context / 2
tokens whose cache rows are random; the last token is pending.  Per (B, draft):

  ms_spec     one SpeculativeStep: spec_draft, the layers on B * (draft + 1) rows, lm_head logits + one draw per row, spec_accept
  ms_decode   one DecodeStep of the same B at the same positions (B = 1: the fused batch-1 step, the fastest this library has)
  break_even  ms_spec / ms_decode: the tokens per step and slot a speculative step must emit to be worth its time
  n_out       the mean tokens per slot it did emit in a step (every replay is the same step: read after the timed loop)

A random model repeats nothing, so prompt lookup proposes nothing and the step degenerates to one row per slot.  --accept M feeds the
caller's drafts instead: a sequential run of the same step first yields each slot's next `draft` tokens, and the timed step is given
those with draft M replaced by another token — exactly M drafts are accepted (n_acc is reported), all draft + 1 rows are computed.
The state is put back in front of every replay, so every replay is the same step.

    python perf/spec_llama.py [--model 3_8b] [--batch 1 4 8] [--draft 2 4 7] [--accept M] [--context 1024] [--replays 32] [--out F]
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


def main(argv=None, quiet=False):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="3_8b", choices=sorted(qp.mem_op.LAYER_INFO))
    ap.add_argument("--quantizer", default="tcomb_6_7_0.5_none_0.9")
    ap.add_argument("--qdict", default=None)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--draft", type=int, nargs="+", default=[2, 4, 7])
    ap.add_argument("--accept", type=int, default=None, metavar="M",
                    help="feed drafts of which exactly M are accepted (clamped to the draft length); default: prompt lookup")
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
        g = torch.Generator().manual_seed(args.seed + B)
        cg = torch.Generator(device=dev).manual_seed(args.seed)
        kc = [(torch.randn(B, nkv, args.context, hd, device=dev, generator=cg) * 0.5).half() for _ in range(nl)]
        vc = [(torch.randn(B, nkv, args.context, hd, device=dev, generator=cg) * 0.5).half() for _ in range(nl)]
        hist = torch.randint(0, args.vocab, (B, n0), generator=g)
        # the plain step at the same positions
        tok, pos = hist[:, -1].clone().to(dev), torch.full((B,), n0 - 1, dtype=torch.long, device=dev)
        out_tok = torch.zeros(B, dtype=torch.long, device=dev)
        ds = qp.DecodeStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, tok, pos, out_tok)
        ms_decode = time_graph(ds, args.replays, dev)
        del ds
        ms_generic = ms_decode  # B = 1: also the batch of one run the way every larger batch runs (what the ragged step's layers are)
        if B == 1:
            ds = qp.DecodeStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, tok, pos, out_tok, generic=True)
            ms_generic = time_graph(ds, args.replays, dev)
            del ds
        for K in args.draft:
            ss = qp.SpeculativeStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, draft=K)
            for b in range(B):
                ss.begin(b, hist[b].tolist())
            start = ss.n_tok.clone()
            ext = ext_n = None
            accept = None if args.accept is None else min(args.accept, K)
            if accept is not None:
                for _ in range(K):  # a sequential run: at least one token per slot and step
                    ss()
                nxt = ss.hist[:, n0:n0 + K].to(torch.int64)
                if accept < K:
                    nxt[:, accept] = (nxt[:, accept] + 1) % args.vocab
                ext, ext_n = nxt.contiguous(), torch.full((B,), K, dtype=torch.int32, device=dev)
            # the state is put back in front of every replay, so every replay is the same step: its n_out / n_acc are read after
            # the timed loop, and the captured graph holds the step alone
            def step():
                ss(ext, ext_n) if ext is not None else ss()

            def reset(i):
                ss.n_tok.copy_(start)

            ss.n_tok.copy_(start)
            ms_spec = time_graph(step, args.replays, dev, reset)
            n_out, n_acc = ss.n_out.double().mean().item(), ss.n_acc.double().mean().item()
            res = {"batch": B, "draft": K, "rows": ss.rows, "accept": accept, "ms_spec": ms_spec, "ms_decode": ms_decode,
                   "ms_decode_generic": ms_generic, "break_even_generic": ms_spec / ms_generic,
                   "break_even": ms_spec / ms_decode, "meets_ratio_below_draft_plus_1": ms_spec / ms_decode < K + 1,
                   "n_out_mean": n_out, "n_acc_mean": n_acc,
                   "tokens_per_s_spec": B * n_out / ms_spec * 1e3, "tokens_per_s_decode": B / ms_decode * 1e3}
            results.append(res)
            if not quiet:
                print(json.dumps(res), file=sys.stderr, flush=True)
            del ss
        del kc, vc
        torch.cuda.empty_cache()
    out = {"what": "speculative step against the decode step of the same B, ms per graph replay", "model": args.model, "layers": nl,
           "quantizer": args.qdict or args.quantizer, "context": args.context, "history": n0, "replays": args.replays,
           "accept": args.accept, "results": results}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    if not quiet:
        print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
