#!/usr/bin/env python3
"""Scoring token sequences with a Llama-shaped model: qpalette_amd.decoder.Score against the ways log-probabilities could be had
before it.

The model is perf/decode_llama.py's (build_model: same random layers, same --model / --layers / --quantizer / --qdict / --vocab),
with per-layer KV caches [slots][nkv][context][hd] holding random rows.  For every --tokens N, in ONE call:

  * Score: the N tokens into slot --slot in chunks of --chunk rows, each chunk followed by qpal_lm_head_logits on all of its rows
    and qpal_token_logprob against the tokens that follow them -> N - 1 log-probabilities;
  * torch glue at q_len = N (the reference, never Score itself): the Incoherent* modules with torch rotary embedding, a StaticKV
    cache and SDPA under a causal mask; its fp16 final-norm state times lm_head.float(), then log-softmax in fp64 on the host;
  * the EXISTING pair: token-by-token DecodeStep(generic=True, sampler=...) logits through sampling.reference_logprob, against the
    torch-glue log-probs.  Its two distances (max |d logprob|, |d mean nll|) are the yardstick for Score's.

--ppl W N adds qpalette_amd.perplexity over W windows of N tokens against the same three.  Timing (unless --no-time): Score,
Prefill on the same tokens (what the scoring tail adds) and the torch path (glue + fp16 lm_head + log_softmax + gather on the
device), each captured in a graph and replayed; and the tail of one chunk on its own (lm_head logits, log-prob) as a share of a
one-chunk Score.

    python perf/score_llama.py [--model 3_8b] [--tokens 128 512 2048] [--context 4096] [--ppl 3 64] [--json profiles/score.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import qpalette_amd as qp
from decode_llama import StaticKV, build_model, time_graph


def main(argv=None, quiet=False):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="3_8b", choices=sorted(qp.mem_op.LAYER_INFO))
    ap.add_argument("--quantizer", default="tcomb_6_7_0.5_none_0.9")
    ap.add_argument("--qdict", default=None, help="perf/qdicts/<name>.json (figure1c, figure1d) instead of --quantizer")
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--tokens", type=int, nargs="+", default=[128], help="one sequence length or a list (each >= 2)")
    ap.add_argument("--context", type=int, default=4096, help="static KV-cache length")
    ap.add_argument("--chunk", type=int, default=128)
    ap.add_argument("--slots", type=int, default=1, help="sequences the caches hold")
    ap.add_argument("--slot", type=int, default=0, help="the slot the sequence goes into")
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--ppl", type=int, nargs=2, default=None, metavar=("W", "N"), help="perplexity over W windows of N tokens")
    ap.add_argument("--iters", type=int, default=5, help="timed replays of each path")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--no-time", action="store_true", help="checks only")
    ap.add_argument("--no-existing-paths", action="store_true", help="skip the eager token-by-token DecodeStep(generic=True) yardstick")
    ap.add_argument("--json", default=None, help="also write the result to this file")
    ap.add_argument("--progress", action="store_true", help="one line per phase on stderr")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    longest = max(args.tokens + ([args.ppl[1]] if args.ppl else []))
    if args.context % 4 or longest + 1 > args.context or min(args.tokens) < 2:
        raise SystemExit("--context: a multiple of 4, above every --tokens; --tokens: at least 2")
    if not 0 <= args.slot < args.slots:
        raise SystemExit("--slot must name one of --slots")
    dev = torch.device("cuda", 0)

    def note(*a):
        if args.progress:
            print(*a, file=sys.stderr, flush=True)

    m = build_model(args.model, args.quantizer, args.qdict, args.layers, args.vocab, dev)
    note("model built")
    cfg, layers, embed, lm_head, norm, inv_freq = m.cfg, m.layers, m.embed, m.lm_head, m.norm, m.inv_freq
    H, nkv, head_dim, nlayers = cfg.hidden_size, cfg.num_key_value_heads, cfg.head_dim, len(layers)
    B, slot, ctx, vocab = args.slots, args.slot, args.context, args.vocab
    ar = torch.arange(ctx, device=dev)
    cg = torch.Generator(device=dev).manual_seed(args.seed)
    kc = [(torch.randn(B, nkv, ctx, head_dim, device=dev, generator=cg) * 0.5).half() for _ in range(nlayers)]
    vc = [(torch.randn(B, nkv, ctx, head_dim, device=dev, generator=cg) * 0.5).half() for _ in range(nlayers)]
    sc = qp.Score(layers, embed, norm, lm_head, kc, vc, inv_freq, chunk=args.chunk)
    pf = qp.Prefill(layers, embed, norm, lm_head, kc, vc, inv_freq, chunk=args.chunk)
    ref = StaticKV(nlayers, nkv, head_dim, ctx, dev)       # the torch-glue path's cache
    one = StaticKV(nlayers, nkv, head_dim, ctx, dev)       # the token-by-token path's cache
    tok1 = torch.zeros(1, dtype=torch.long, device=dev)
    pos1 = torch.zeros(1, dtype=torch.long, device=dev)
    out1 = torch.zeros(1, dtype=torch.long, device=dev)
    smp1 = qp.Sampler(1, vocab, dev, temperature=0.0)
    generic1 = qp.DecodeStep(layers, embed, norm, lm_head, one.k, one.v, inv_freq, tok1, pos1, out1, generic=True, sampler=smp1)
    lm_head32 = lm_head.float()

    def glue(tokens, pos):
        """the torch-glue step on len(tokens) rows at positions pos: the residual stream [1, n, H] it leaves"""
        n = tokens.shape[0]
        h = embed[tokens].view(1, n, H)
        ang = pos.float()[:, None] * inv_freq[None, :]
        emb = torch.cat((ang, ang), dim=-1)[None]                       # [1, n, head_dim]
        rope = (emb.cos().half(), emb.sin().half())
        mask = torch.where(ar[None, :] <= pos[:, None], 0.0, float("-inf")).half().view(1, 1, n, -1)
        for layer in layers:
            h = layer(h, rope, mask, ref, pos, glue=True)
        return h

    def glue_logprobs(tokens):
        """fp64 [N - 1] on the host: log-softmax of fp16 norm(h) @ lm_head.float() at the next tokens, 128 rows at a time"""
        N = tokens.shape[0]
        state = norm(glue(tokens, torch.arange(N, device=dev))[0])     # fp16 [N, H]
        nxt = tokens[1:].cpu()
        out = []
        for c in range(0, N - 1, 128):
            n = min(128, N - 1 - c)
            logits = (state[c:c + n].float() @ lm_head32.T).cpu().double()
            out.append(torch.log_softmax(logits, dim=-1).gather(1, nxt[c:c + n, None])[:, 0])
        return torch.cat(out).numpy()

    def token_by_token_logprobs(tokens):
        """fp64 [N - 1]: the batch-of-one generic decode step's logits at every position through reference_logprob"""
        N = tokens.shape[0]
        nxt = tokens.cpu().tolist()
        out = np.zeros(N - 1)
        for i in range(N - 1):
            tok1.copy_(tokens[i:i + 1])
            pos1.fill_(i)
            generic1()
            out[i] = qp.reference_logprob(smp1.logits[0].cpu().numpy(), nxt[i + 1])[0]
        return out

    def distances(a, b):
        return {"max_abs_diff_logprob": float(np.abs(a - b).max()), "abs_diff_mean_nll": float(abs(a.mean() - b.mean()))}

    def run(N):
        g = torch.Generator().manual_seed(args.seed + N)
        tokens = torch.randint(0, vocab, (N,), generator=g).to(dev)
        ref_lp = glue_logprobs(tokens)
        note(N, "torch glue done")
        kc0 = [t.clone() for t in kc]
        vc0 = [t.clone() for t in vc]
        lp_dev = sc(tokens, slot=slot, pos0=0)
        torch.cuda.synchronize()
        lp = lp_dev.double().cpu().numpy()
        others = [b for b in range(B) if b != slot]
        untouched = all(torch.equal(t[others].view(torch.int16), t0[others].view(torch.int16)) for t, t0 in zip(kc + vc, kc0 + vc0))
        del kc0, vc0
        note(N, "score done")
        check = {"positions": int(lp.shape[0]), "finite": bool(np.isfinite(lp).all() and np.isfinite(ref_lp).all()),
                 "score_vs_torch_glue": distances(lp, ref_lp), "existing_paths": None, "score_vs_token_by_token": None,
                 "mean_nll_score": float(-lp.mean()), "mean_nll_torch_glue": float(-ref_lp.mean()), "other_slots_untouched": untouched,
                 "mean_rank": float(sc.rank.float().mean())}
        if not args.no_existing_paths:
            tbt = token_by_token_logprobs(tokens)
            check["existing_paths"] = distances(tbt, ref_lp)
            check["score_vs_token_by_token"] = distances(lp, tbt)
            note(N, "token by token done")
        res = {"tokens": N, "check": check, "ms_score": None, "ms_prefill": None, "ms_torch": None}
        if not args.no_time:
            pos = torch.arange(N, device=dev)

            def torch_path():
                logits = norm(glue(tokens, pos)[0]) @ lm_head.T
                return torch.log_softmax(logits[:-1].float(), dim=-1).gather(1, tokens[1:, None])

            ms_sc = time_graph(lambda: sc(tokens, slot=slot, pos0=0), args.iters, dev)
            note(N, "score ms", ms_sc)
            ms_pf = time_graph(lambda: pf(tokens, slot=slot, pos0=0), args.iters, dev)
            note(N, "prefill ms", ms_pf)
            ms_t = time_graph(torch_path, args.iters, dev)
            note(N, "torch ms", ms_t)
            res.update({"ms_score": ms_sc, "tokens_per_s_score": N / ms_sc * 1e3, "ms_prefill": ms_pf, "tokens_per_s_prefill": N / ms_pf * 1e3,
                        "ms_torch": ms_t, "tokens_per_s_torch": N / ms_t * 1e3, "score_over_prefill": ms_sc / ms_pf,
                        "torch_over_score": ms_t / ms_sc})
        return res

    def run_ppl(W, N):
        g = torch.Generator().manual_seed(args.seed + 1000 * W + N)
        windows = torch.randint(0, vocab, (W, N), generator=g).to(dev)
        lp_out = torch.zeros(W, N - 1, device=dev)
        ppl, avg = qp.perplexity(sc, windows, slot=slot, out=lp_out)   # (a second run of the layers would differ in the last bits)
        lps = list(lp_out.double().cpu().numpy())
        host_avg = float(np.mean([-x.mean() for x in lps]))
        glue_avg = float(np.mean([-glue_logprobs(windows[w]).mean() for w in range(W)]))
        out = {"windows": W, "tokens": N, "ppl": ppl, "avg_loss": avg, "ppl_from_logprobs_on_host": float(np.exp(host_avg)),
               "ppl_torch_glue": float(np.exp(glue_avg)), "avg_loss_torch_glue": glue_avg, "existing_paths_abs_diff_mean_nll": None}
        if not args.no_existing_paths:
            tbt_avg = float(np.mean([-token_by_token_logprobs(windows[w]).mean() for w in range(W)]))
            out["existing_paths_abs_diff_mean_nll"] = abs(tbt_avg - glue_avg)
        return out

    def tail_share():
        """one chunk's tail on its own: lm_head logits of `chunk` rows and the log-prob launch, against a one-chunk Score"""
        n = args.chunk
        h32 = torch.randn(n, H, device=dev, generator=cg)
        tokens = torch.randint(0, vocab, (n + 1,), device=dev, generator=cg)
        logits = torch.zeros(n, vocab, device=dev)
        lp = torch.zeros(n, device=dev)
        rank = torch.zeros(n, dtype=torch.int32, device=dev)
        ms_lm = time_graph(lambda: qp.lm_head_logits(h32, norm.weight, norm.eps, lm_head, out=logits), 4 * args.iters, dev)
        ms_lp = time_graph(lambda: qp.token_logprobs(logits, tokens[1:], out=lp, rank=rank), 4 * args.iters, dev)
        ms_chunk = time_graph(lambda: sc(tokens[:n], slot=slot, pos0=0), args.iters, dev)
        return {"rows": n, "ms_lm_head_logits": ms_lm, "ms_token_logprob": ms_lp, "ms_one_chunk_score": ms_chunk,
                "tail_share_of_chunk": (ms_lm + ms_lp) / ms_chunk}

    out = {"what": "scoring: Score (chunked, lm_head logits + token log-prob per chunk) vs torch glue at q_len = N + fp64 log-softmax",
           "model": args.model, "layers": nlayers, "quantizer": args.qdict or args.quantizer, "context": ctx, "chunk": args.chunk,
           "vocab": vocab, "slots": B, "slot": slot, "device": torch.cuda.get_device_name(0), "runs": [run(N) for N in args.tokens],
           "perplexity": run_ppl(*args.ppl) if args.ppl else None, "tail": None if args.no_time else tail_share()}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    if not quiet:
        print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
