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

--tree N [N ...] --width W [W ...] --right J [J ...]: the TREE step, SpeculativeStep(tree=N), against the chain step of the same row
count min(128, B (N + 1)) in the same call.  A sequential pre-run yields each slot's next tokens; the tree has N // W levels (at most
15) of W siblings under the previous level's sibling J, and sibling J (1-based; 0: none) carries the pre-run's token of its level.
The chain step is fed the pre-run's tokens themselves (every draft accepted).  --repeats times, alternating: chain, tree, chain, ...;
per step the list of ms per replay, and n_out / n_acc of the last replay.
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


def tree_against_chain(args, m, kc, vc, hist, B, N, W, J, n0, dev, ms_decode):
    """one (B, N, W, J) of --tree: the chain step and the tree step at the same row count, timed alternately"""
    K = min(15, N)
    D, R = min(15, N // W), min(128, B * (N + 1))
    model = (m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq)
    chain, tree = qp.SpeculativeStep(*model, draft=K, rows=R), qp.SpeculativeStep(*model, tree=N, rows=R)
    for ss in (chain, tree):
        for b in range(B):
            ss.begin(b, hist[b].tolist())
    start = tree.n_tok.clone()
    for _ in range(K):  # the sequential pre-run (a random model repeats nothing: prompt lookup proposes nothing, one token per step)
        tree()
    nxt = tree.hist[:, n0:n0 + K].to(torch.int64).contiguous()
    ext_n = torch.full((B,), K, dtype=torch.int32, device=dev)
    tok, par = torch.zeros(B, N, dtype=torch.int32, device=dev), torch.zeros(B, N, dtype=torch.int32, device=dev)
    for l in range(D):  # level l: W siblings under the previous level's sibling J (none right: the first)
        for w in range(W):
            tok[:, l * W + w] = nxt[:, l] if w == J - 1 else (nxt[:, l] + 1 + w) % args.vocab
            par[:, l * W + w] = 0 if l == 0 else (l - 1) * W + max(J, 1)
    tree_n = torch.full((B,), D * W, dtype=torch.int32, device=dev)
    steps = {"chain": (chain, lambda: chain(nxt, ext_n)), "tree": (tree, lambda: tree(ext_tok=tok, ext_par=par, ext_n=tree_n))}
    ms = {"chain": [], "tree": []}
    for _ in range(args.repeats):
        for name, (ss, fn) in steps.items():
            ss.n_tok.copy_(start)
            ms[name].append(time_graph(fn, args.replays, dev, lambda i, ss=ss: ss.n_tok.copy_(start)))
    res = {"batch": B, "tree": N, "width": W, "right": J, "levels": D, "rows": R, "ms_chain": ms["chain"], "ms_tree": ms["tree"],
           "ms_decode": ms_decode, "tree_over_chain": min(ms["tree"]) / min(ms["chain"]),
           "chain_spread": (max(ms["chain"]) - min(ms["chain"])) / min(ms["chain"])}
    for name, (ss, _) in steps.items():
        res[f"n_out_{name}"], res[f"n_acc_{name}"] = ss.n_out.double().mean().item(), ss.n_acc.double().mean().item()
    return res


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
    ap.add_argument("--tree", type=int, nargs="+", default=None, metavar="N", help="time the tree step of N nodes per slot against the chain step")
    ap.add_argument("--width", type=int, nargs="+", default=[2], help="--tree: siblings per level")
    ap.add_argument("--right", type=int, nargs="+", default=[1], help="--tree: the sibling (1-based) that carries the sequential token; 0: none")
    ap.add_argument("--repeats", type=int, default=3, help="--tree: alternating repeats of (chain, tree)")
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
        for N, W, J in ((N, W, J) for N in args.tree or [] for W in args.width for J in args.right if J <= W):
            results.append(tree_against_chain(args, m, kc, vc, hist, B, N, W, J, n0, dev, ms_decode))
            if not quiet:
                print(json.dumps(results[-1]), file=sys.stderr, flush=True)
        for K in ([] if args.tree else args.draft):
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
