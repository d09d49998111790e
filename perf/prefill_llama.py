#!/usr/bin/env python3
"""Prompt prefill of a Llama-shaped model: qpalette_amd.decoder.Prefill against the two ways a prompt could be taken before it.

The model is perf/decode_llama.py's (build_model: same random layers, same --model / --layers / --quantizer / --qdict / --vocab),
with per-layer KV caches [slots][nkv][context][hd] holding random rows.  For every --prompt N, in ONE call:

  * Prefill: the prompt into slot --slot in chunks of --chunk rows (per layer and chunk: RMSNorm + rotation, q|k|v multi_gemv,
    prefill_attention, o_proj, up|gate, SwiGLU rotation, down_proj), captured in a graph and replayed;
  * token by token: the same prompt through a captured batch-1 DecodeStep, one replay per token;
  * torch glue at q_len = N: the Incoherent* modules (DecoderLayer.forward(..., glue=True)) with torch rotary embedding, a StaticKV
    cache and SDPA under a causal mask.

Checks (max |diff| of the last row's final-norm state): Prefill vs torch glue; the two EXISTING paths against each other
(token-by-token DecodeStep(generic=True) vs torch glue: the yardstick for the first figure); the slots Prefill must not touch;
and one batched DecodeStep continuing the prefilled slot against the torch-glue continuation.

    python perf/prefill_llama.py [--model 3_8b] [--prompt 16 128 512 2048] [--context 4096] [--slots 1] [--slot 0] [--no-time]

--ragged S N: instead of the above, S prompts of N tokens (S * N <= 128) into slots 0 .. S - 1 from empty contexts, in the same call
through ONE RaggedStep (one 128-row step, ragged_prefill_attention) and through S Prefill calls, both captured in a
graph and replayed: ms of each, and whether the S next tokens agree.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

import qpalette_amd as qp
from decode_llama import WARMUP, StaticKV, build_model, time_graph


def main(argv=None, quiet=False):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="3_8b", choices=sorted(qp.mem_op.LAYER_INFO))
    ap.add_argument("--quantizer", default="tcomb_6_7_0.5_none_0.9")
    ap.add_argument("--qdict", default=None, help="perf/qdicts/<name>.json (figure1c, figure1d) instead of --quantizer")
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--prompt", type=int, nargs="+", default=[128], help="one prompt length or a list")
    ap.add_argument("--context", type=int, default=4096, help="static KV-cache length")
    ap.add_argument("--chunk", type=int, default=128)
    ap.add_argument("--slots", type=int, default=1, help="sequences the caches hold (B of a DecodeStep over them)")
    ap.add_argument("--slot", type=int, default=0, help="the slot the prompt goes into; the last slot, if another, is inactive")
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--iters", type=int, default=5, help="timed replays of Prefill and of the torch-glue step")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--no-time", action="store_true", help="checks only")
    ap.add_argument("--ragged", type=int, nargs=2, default=None, metavar=("S", "N"), help="S prompts of N tokens: RaggedStep vs S Prefill calls")
    ap.add_argument("--no-existing-paths", action="store_true", help="skip the eager token-by-token DecodeStep(generic=True) check")
    ap.add_argument("--progress", action="store_true", help="one line per phase on stderr")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    if args.context % 4 or max(args.prompt) + 1 > args.context:
        raise SystemExit("--context: a multiple of 4, above every --prompt")
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
    B, slot, ctx = args.slots, args.slot, args.context
    if args.ragged:
        S, N = args.ragged
        if S < 1 or N < 1 or S * N > 128 or N > ctx:
            raise SystemExit("--ragged S N: S * N <= 128 rows, N inside --context")
        kc = [torch.zeros(S, nkv, ctx, head_dim, dtype=torch.float16, device=dev) for _ in range(nlayers)]
        vc = [torch.zeros(S, nkv, ctx, head_dim, dtype=torch.float16, device=dev) for _ in range(nlayers)]
        rs = qp.RaggedStep(layers, embed, norm, lm_head, kc, vc, inv_freq, rows=128, segments=S)
        pf = qp.Prefill(layers, embed, norm, lm_head, kc, vc, inv_freq, chunk=args.chunk)
        g = torch.Generator().manual_seed(args.seed)
        prompts = [torch.randint(0, args.vocab, (N,), generator=g).to(dev) for _ in range(S)]
        packed = rs.pack([(b, prompts[b], 0) for b in range(S)])
        toks_r = rs(*packed).tolist()
        toks_p = [int(pf(prompts[b], slot=b, pos0=0)) for b in range(S)]
        out = {"what": "S prompts of N tokens: one RaggedStep vs S Prefill calls (graph replays, same call)", "model": args.model,
               "layers": nlayers, "quantizer": args.qdict or args.quantizer, "context": ctx, "S": S, "N": N,
               "next_tokens_agree": toks_r == toks_p, "ms_ragged_step": None, "ms_prefill_calls": None}
        if not args.no_time:
            out["ms_ragged_step"] = time_graph(lambda: rs(*packed), args.iters, dev)
            out["ms_prefill_calls"] = time_graph(lambda: [pf(prompts[b], slot=b, pos0=0) for b in range(S)], args.iters, dev)
        if not quiet:
            print(json.dumps(out))
        return out
    ar = torch.arange(ctx, device=dev)
    cg = torch.Generator(device=dev).manual_seed(args.seed)
    kc = [(torch.randn(B, nkv, ctx, head_dim, device=dev, generator=cg) * 0.5).half() for _ in range(nlayers)]
    vc = [(torch.randn(B, nkv, ctx, head_dim, device=dev, generator=cg) * 0.5).half() for _ in range(nlayers)]
    pf = qp.Prefill(layers, embed, norm, lm_head, kc, vc, inv_freq, chunk=args.chunk)
    ref = StaticKV(nlayers, nkv, head_dim, ctx, dev)       # the torch-glue path's cache
    one = StaticKV(nlayers, nkv, head_dim, ctx, dev)       # the token-by-token paths' cache
    tok1 = torch.zeros(1, dtype=torch.long, device=dev)
    pos1 = torch.zeros(1, dtype=torch.long, device=dev)
    out1 = torch.zeros(1, dtype=torch.long, device=dev)
    generic1 = qp.DecodeStep(layers, embed, norm, lm_head, one.k, one.v, inv_freq, tok1, pos1, out1, generic=True)
    fast1 = generic1
    if qp.decoder.fusable(layers):
        fast1 = qp.DecodeStep(layers, embed, norm, lm_head, one.k, one.v, inv_freq, tok1, pos1, out1)

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

    def run(N):
        g = torch.Generator().manual_seed(args.seed + N)
        tokens = torch.randint(0, args.vocab, (N,), generator=g).to(dev)
        pos = torch.arange(N, device=dev)
        bound = lambda r: 2.0 ** -7 * max(1.0, float(r.abs().max()))
        # ---- torch glue at q_len = N
        ref_h = norm(glue(tokens, pos)[:, -1]).float()
        # ---- Prefill into `slot`; every other slot keeps its bytes
        kc0 = [t.clone() for t in kc]
        vc0 = [t.clone() for t in vc]
        next_tok = pf(tokens, slot=slot, pos0=0).clone()
        got_h = pf.hidden().float()
        others = [b for b in range(B) if b != slot]
        untouched = all(torch.equal(t[others].view(torch.int16), t0[others].view(torch.int16)) for t, t0 in zip(kc + vc, kc0 + vc0))
        del kc0, vc0
        # ---- the two existing paths against each other: token by token through DecodeStep(generic=True)
        note(N, "prefill done")
        tbt_h = None
        if not args.no_existing_paths:
            for i in range(N):
                tok1.copy_(tokens[i:i + 1])
                pos1.fill_(i)
                generic1()
            tbt_h = generic1.hidden().float()
        note(N, "checks done")
        check = {"max_abs_diff_final_norm": float((got_h - ref_h).abs().max()), "max_abs_ref": float(ref_h.abs().max()),
                 "bound": bound(ref_h), "finite": bool(torch.isfinite(got_h).all()),
                 "existing_paths_max_abs_diff": None if tbt_h is None else float((tbt_h - ref_h).abs().max()),
                 "prefill_vs_token_by_token": None if tbt_h is None else float((got_h - tbt_h).abs().max()),
                 "other_slots_untouched": untouched, "next_token": int(next_tok),
                 "next_token_token_by_token": None if tbt_h is None else int(out1)}
        # ---- one batched DecodeStep continues the prefilled slot (the last slot, if another, inactive; the rest at position 5)
        tokB = torch.randint(0, args.vocab, (B,), generator=g).to(dev)
        posB = torch.full((B,), 5, dtype=torch.long, device=dev)
        if B > 1 and slot != B - 1:
            posB[B - 1] = -1
        tokB[slot] = next_tok[0]
        posB[slot] = N
        outB = torch.zeros(B, dtype=torch.long, device=dev)
        cont = qp.DecodeStep(layers, embed, norm, lm_head, kc, vc, inv_freq, tokB, posB, outB, generic=True)
        cont()
        cont_h = cont.hidden()[slot].float()
        cont_ref = norm(glue(next_tok, torch.full((1,), N, dtype=torch.long, device=dev))[:, -1]).float().view(-1)
        check["continuation"] = {"max_abs_diff_final_norm": float((cont_h - cont_ref).abs().max()), "bound": bound(cont_ref),
                                 "max_abs_ref": float(cont_ref.abs().max()), "finite": bool(torch.isfinite(cont_h).all())}
        del cont
        res = {"prompt": N, "check": check, "ms_prefill": None, "ms_token_by_token": None, "ms_torch_glue": None}
        if not args.no_time:
            def feed(i):
                j = max(0, i - WARMUP) % N
                tok1.copy_(tokens[j:j + 1])
                pos1.fill_(j)
            ms_pf = time_graph(lambda: pf(tokens, slot=slot, pos0=0), args.iters, dev)
            note(N, "prefill ms", ms_pf)
            ms_tbt = time_graph(fast1, N, dev, feed) * N
            note(N, "token by token ms", ms_tbt)
            ms_glue = time_graph(lambda: glue(tokens, pos), args.iters, dev)
            note(N, "torch glue ms", ms_glue)
            res.update({"ms_prefill": ms_pf, "prompt_tokens_per_s_prefill": N / ms_pf * 1e3,
                        "ms_token_by_token": ms_tbt, "prompt_tokens_per_s_token_by_token": N / ms_tbt * 1e3,
                        "ms_torch_glue": ms_glue, "prompt_tokens_per_s_torch_glue": N / ms_glue * 1e3,
                        "prefill_vs_token_by_token_speedup": ms_tbt / ms_pf})
        return res

    out = {"what": "prompt prefill: Prefill (chunked, prefill_attention) vs token-by-token DecodeStep vs torch glue at q_len = N",
           "model": args.model, "layers": nlayers, "quantizer": args.qdict or args.quantizer, "context": ctx, "chunk": args.chunk,
           "slots": B, "slot": slot, "prompts": [run(N) for N in args.prompt]}
    if not quiet:
        print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
