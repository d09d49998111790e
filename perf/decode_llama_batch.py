#!/usr/bin/env python3
"""Whole-model decode step of a Llama-shaped model at batch B: B concurrent sequences, one token each per step.

The model is perf/decode_llama.py's (same random layers from this package's modules, same --model / --layers / --quantizer /
--qdict / --vocab), with per-layer KV caches [B][nkv][context][hd].  The B sequences sit at ragged, seeded positions; with
--inactive N the last N slots carry pos = -1 (free slots of a continuous-batching server: they cost nothing and change nothing).
One step at batch B (qpalette_amd.decoder.DecodeStep; a batch of one runs the same way here, generic=True):

  1. RMSNorm + sign flip + Hadamard rotation of the fp32 residual stream [B, H] (hadamard.rotate(..., rms=...): one launch)
  2. q|k|v through multi_gemv (fp32 out [B, nq*hd + 2*nkv*hd])
  3. rotary embedding + KV append + attention of every sequence: ONE launch (attention.decode_attention)
  4. o_proj's rotation, then multi_gemv(accumulate=True) into the residual stream
  5. gate|up, the SwiGLU rotation (IN_SWIGLU_F32), down_proj with accumulate=True
  6. final norm, lm_head and argmax as torch ops

The step is captured in a graph and replayed (positions advance on the device between replays).  Next to it: the same graph with
the four projection groups alone (linears-only), and a torch-glue step at the same B built from the Incoherent* modules (torch
rotary embedding, a per-sequence cache write, SDPA with a per-sequence mask), whose final normalised hidden state is the check.

--sample adds the sampled step (DecodeStep(sampler=...): qpal_lm_head_logits + qpal_sample in the torch tail's place) at temperature
0.6 / top-k 5 (the setting of the decode loop this was modelled on) and 0.8 / top-p 0.95, timed in the same call as the greedy step.

--process (with --sample) also times each sampled step with a logits.LogitProcessor: repetition 1.3, presence 0.5,
frequency 0.3, a mask that allows every second token and 64 bias entries in every slot — observe + process, two more launches —
next to the same step without one, in the same call.

--grammar (with --sample) also times each sampled step with a grammar.GrammarBank: every slot follows a number
pattern on a synthetic vocabulary (perf/sampling_kernels.py's) — mask + advance, two more launches — next to the same step without
one, in the same call.

--stop (with --sample) also times each sampled step with a stop.StopBank: a stop set of eight strings, eos as the stop
id and no budget in every slot, `qpal_stop_advance` as the step's last launch — the step then moves tok / pos itself, so its replays
run with NOTHING between them — next to the same step followed by the `tok.copy_(out_tok); pos += 1` this driver issues between
replays today, timed before and behind it in the same call.  Both figures and their difference go to profiles/stop.json.

--kv fp8 keeps the caches as torch.float8_e4m3fn.  The torch-glue reference then keeps fp16 caches of its own that
hold e4m3 values only: `BatchKV.update` stores a new row through the round trip clamp(-448, 448) -> float8_e4m3fn -> half and the
step attends to the round-tripped cache, as the kernels do.  The check also reports how far the fp16-cache step lies from that
reference (what the format itself moves; not a gate).

--paged PAGE_SIZE --shared-prefix P: also the step on pools in which all B slots share the pages of a P-position prefix and have 1 ..
256 seeded positions of their own each, timed both ways in the same call — DecodeStep(block_table=...) and DecodeStep(block_table=...,
shared_prefix=...) —, the plain step again behind them, and how far the two steps' final hidden states lie apart.

    python perf/decode_llama_batch.py [--model 3_8b] [--batch 1 8 16 32 64] [--context 1024] [--tokens 64] [--inactive 0] [--sample]
                                      [--process] [--grammar] [--stop] [--kv fp16|fp8] [--paged PAGE_SIZE] [--shared-prefix P] [--window W]
                                      [--softcap CAP] [--sinks]
                                      [--qkv-bias] [--qk-norm] [--geglu] [--post-norms] [--logit-cap CAP]

--qkv-bias / --qk-norm / --geglu / --post-norms / --logit-cap time the step with each block variant of DESIGN.md §34 on the random
model (random bias, norm weights 1 + 0.3 N(0, 1)), each on its own, all given ones together, and the plain step again: "blocks" in
the result, with every step's launches_per_token.
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
from paged import random_table, scatter


class BatchKV:
    """Per-sequence static caches [B][nkv][max_len][hd] with the `update` the attention module calls: row pos[b] of sequence b
    (a sequence whose position lies outside the cache keeps its cache as it is).  kv8: new rows are stored as the fp16 image of
    their e4m3fn bytes (the stored value of an 8-bit cache)."""

    def __init__(self, k, v, kv8=False):
        self.k, self.v, self.kv8 = k, v, kv8

    def update(self, k, v, layer_idx, kwargs):
        pos = kwargs["cache_position"]
        kc, vc = self.k[layer_idx], self.v[layer_idx]
        B, L = kc.shape[0], kc.shape[2]
        live = ((pos >= 0) & (pos < L)).view(B, 1, 1)
        idx = pos.clamp(0, L - 1)
        rows = torch.arange(B, device=kc.device)
        if self.kv8:
            k, v = e4m3_round_trip(k), e4m3_round_trip(v)
        kc[rows, :, idx] = torch.where(live, k[:, :, 0], kc[rows, :, idx])
        vc[rows, :, idx] = torch.where(live, v[:, :, 0], vc[rows, :, idx])
        return kc, vc


def e4m3_round_trip(x):
    """the fp16 image of x stored as OCP e4m3fn: clamp to the format's range, round to nearest even, back to fp16 (exact)"""
    return x.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).half()


def sparse_layers(layers, E, top_k, inter, qstr, dev, seed=5, router="mixtral", shared_inter=0):
    """the model's layers with every MLP replaced by a MoEMLP of E random experts of intermediate width `inter` (the attention
    modules and norms are the dense model's own): random packed weights of quantizer `qstr`, one codebook, one SU per rotation.
    router: a moe.router_preset name (random select bias / shared gate where the family has one); shared_inter: the width of a
    shared expert with sign vectors of its own (0: none)"""
    import math
    H = layers[0].self_attn.hidden_size
    g = torch.Generator().manual_seed(seed)

    def wrapped(k, m, s, su):
        il = qp.IncoherentLinear(k, m, k, m, use_linear=False)
        il.linear = qp.make_linear_from_info(qstr, qp.mem_op.dummy_linear_info(k, m, qstr, seed=s, codebook_seed=777))
        il.SU.data.copy_(su)
        il.Wscale.data.fill_(1.0 / math.sqrt(k))
        il.rot_info = "skip_r"
        il.apply_rot_info()
        return il.to(dev)

    out = torch.nn.ModuleList()
    for i, l in enumerate(layers):
        su_h, su_i = ((torch.randint(0, 2, (n,), generator=g) * 2 - 1).half() for n in (H, inter))
        experts = [(wrapped(H, inter, 3 * (i * E + e), su_h), wrapped(H, inter, 3 * (i * E + e) + 1, su_h),
                    wrapped(inter, H, 3 * (i * E + e) + 2, su_i)) for e in range(E)]
        layer = torch.nn.Module()
        layer.self_attn, layer.input_layernorm, layer.post_attention_layernorm = l.self_attn, l.input_layernorm, l.post_attention_layernorm
        kw = qp.moe.router_preset(router, E, top_k)
        if router == "deepseek_v3":
            kw["select_bias"] = (0.1 * torch.randn(E, generator=g)).to(dev)
        if shared_inter:
            su_s, su_d = ((torch.randint(0, 2, (n,), generator=g) * 2 - 1).half() for n in (H, shared_inter))
            s0 = 3 * (len(layers) * E + i)
            up, gt, dn = wrapped(H, shared_inter, s0, su_s), wrapped(H, shared_inter, s0 + 1, su_s), wrapped(shared_inter, H, s0 + 2, su_d)
            mlp = qp.IncoherentMLP(H, shared_inter, "silu")
            mlp.up_proj, mlp.gate_proj, mlp.down_proj = up.linear, gt.linear, dn.linear
            mlp = mlp.to(dev)
            mlp.SU_ug.data.copy_(up.SU), mlp.SU_dp.data.copy_(dn.SU)
            mlp.Wscale_ug.data.copy_(torch.cat([up.Wscale, gt.Wscale])), mlp.Wscale_dp.data.copy_(dn.Wscale)
            mlp.scale = up.scale
            kw["shared"] = mlp
            if router == "qwen2":
                kw["shared_gate"] = (torch.randn(H, generator=g) / math.sqrt(H)).half().to(dev)
        amp = 1.0 if router == "deepseek_v3" else 4.0   # (4 / sqrt(H) saturates a sigmoid)
        layer.mlp = qp.MoEMLP.from_experts((torch.randn(E, H, generator=g) * amp / math.sqrt(H)).half().to(dev), experts, top_k, **kw)
        out.append(layer)
    return out


def main(argv=None, quiet=False):
    ap = argparse.ArgumentParser()
    ap.add_argument("--moe-router", default="mixtral", choices=qp.moe.ROUTER_PRESETS,
                    help="with --moe: the router of the sparse layers (moe.router_preset; DESIGN.md §36)")
    ap.add_argument("--moe-shared", type=int, default=0, metavar="IS",
                    help="with --moe: a shared expert of intermediate width IS in every sparse layer (gated for qwen2)")
    ap.add_argument("--model", default="3_8b", choices=sorted(qp.mem_op.LAYER_INFO))
    ap.add_argument("--quantizer", default="tcomb_6_7_0.5_none_0.9")
    ap.add_argument("--qdict", default=None, help="perf/qdicts/<name>.json (figure1c, figure1d) instead of --quantizer")
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--batch", type=int, nargs="+", default=[8], help="one B or a list")
    ap.add_argument("--context", type=int, default=1024, help="static KV-cache length of every sequence")
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--inactive", type=int, default=0, help="slots with pos = -1")
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--seed", type=int, default=7, help="seed of the ragged positions")
    ap.add_argument("--no-torch-glue", action="store_true", help="skip the torch-glue step (its timing and the check)")
    ap.add_argument("--sample", action="store_true", help="also time the step with a sampler (0.6 / top-k 5 and 0.8 / top-p 0.95)")
    ap.add_argument("--process", action="store_true", help="with --sample: also time the sampled step with a logit processor")
    ap.add_argument("--grammar", action="store_true", help="with --sample: also time the sampled step with a grammar in every slot")
    ap.add_argument("--stop", action="store_true",
                    help="with --sample: also time the sampled step with a stop bank that ends it, against the step + the host's feed")
    ap.add_argument("--kv", default="fp16", choices=["fp16", "fp8"], help="KV-cache element format (fp8: OCP e4m3fn, no scales)")
    ap.add_argument("--paged", type=int, default=0, metavar="PAGE_SIZE",
                    help="also time the step on a paged cache of this page size (pages in a seeded random order; DESIGN.md §17)")
    ap.add_argument("--shared-prefix", type=int, default=0, metavar="P",
                    help="with --paged: also time the step both ways on pools whose slots share a P-position prefix (DESIGN.md §26)")
    ap.add_argument("--window", type=int, default=0, metavar="W",
                    help="also time the step with this sliding window in every layer (DecodeStep(window=W), DESIGN.md §31)")
    ap.add_argument("--softcap", type=float, default=None, metavar="CAP",
                    help="also time the step with this logit soft cap in every layer (DecodeStep(softcap=CAP), DESIGN.md §32)")
    ap.add_argument("--sinks", action="store_true", help="also time the step with per-head sinks in every layer (DecodeStep(sinks=...))")
    # the block variants: each one given is timed on its own next to the plain step, then all given ones together
    ap.add_argument("--qkv-bias", action="store_true", help="also time the step with a random q|k|v bias (DecodeStep(qkv_bias=...))")
    ap.add_argument("--qk-norm", action="store_true", help="also time the step with per-head QK-norm (DecodeStep(qk_norm=...))")
    ap.add_argument("--geglu", action="store_true", help="also time the step with mlp_act='gelu_tanh'")
    ap.add_argument("--post-norms", action="store_true", help="also time the step with sandwich post-norms (DecodeStep(post_norms=...))")
    ap.add_argument("--logit-cap", type=float, default=None, metavar="CAP",
                    help="also time the step with this final-logit soft cap (DecodeStep(logit_cap=CAP); it launches behind a sampler's "
                         "lm_head only: the step is timed with a greedy sampler, against the plain step with that sampler)")
    ap.add_argument("--moe", type=int, nargs=3, default=None, metavar=("E", "TOP_K", "I"),
                    help="also time the step on the same model with every MLP a MoEMLP of E random experts of intermediate width I, "
                         "TOP_K of them per token (DESIGN.md §35; --quantizer must be a tcq_* / tcomb_*_0.5 string with KV <= 8)")
    args = ap.parse_args(argv)
    kv8 = args.kv == "fp8"
    if args.shared_prefix and (not args.paged or args.shared_prefix % args.paged or args.shared_prefix < args.paged
                               or args.context < args.shared_prefix + 256 + args.tokens + 16):
        raise SystemExit("--shared-prefix: with --paged, a multiple of the page size, and --context >= P + 256 + --tokens + 16")
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    if args.grammar and not args.sample:
        raise SystemExit("--grammar: the grammar masks a sampler's logits, add --sample")
    if args.stop and not args.sample:
        raise SystemExit("--stop: timed next to the sampled step, add --sample")
    if args.process and not args.sample:
        raise SystemExit("--process: the processor works on a sampler's logits, add --sample")
    if args.context % 4 or args.context < args.tokens + 16:
        raise SystemExit("--context: a multiple of 4, at least --tokens + 16")
    if args.paged and (args.paged not in qp.attention.PAGE_SIZES or args.context % args.paged):
        raise SystemExit(f"--paged: one of {qp.attention.PAGE_SIZES} that divides --context")
    dev = torch.device("cuda", 0)
    m = build_model(args.model, args.quantizer, args.qdict, args.layers, args.vocab, dev)
    cfg, layers, embed, lm_head, norm, inv_freq = m.cfg, m.layers, m.embed, m.lm_head, m.norm, m.inv_freq
    H, I, nkv, head_dim, nlayers = cfg.hidden_size, cfg.intermediate_size, cfg.num_key_value_heads, cfg.head_dim, len(layers)
    moe_layers = (sparse_layers(layers, *args.moe, args.quantizer, dev, router=args.moe_router, shared_inter=args.moe_shared)
                  if args.moe else None)

    def run_batch(B):
        nact = B - args.inactive
        if nact < 1:
            raise SystemExit("--inactive must leave at least one active sequence")
        # ragged, seeded start positions; the timed replays advance every active one by one position per step
        g = torch.Generator().manual_seed(args.seed + B)
        top = args.context - args.tokens - 9
        base = torch.randint(0, top + 1, (B,), generator=g)
        base[0] = 0
        if B > 1:
            base[1] = top
        base[nact:] = -1
        pos0 = base.to(dev)
        inc = (pos0 >= 0).long()
        pos = pos0.clone()
        tok = torch.randint(0, args.vocab, (B,), generator=g).to(dev)
        out_tok = torch.zeros(B, dtype=torch.long, device=dev)
        cg = torch.Generator(device=dev).manual_seed(args.seed)
        kc = [(torch.randn(B, nkv, args.context, head_dim, device=dev, generator=cg) * 0.5).half() for _ in range(nlayers)]
        vc = [(torch.randn(B, nkv, args.context, head_dim, device=dev, generator=cg) * 0.5).half() for _ in range(nlayers)]
        kc_ref, vc_ref = kc, vc  # the torch-glue step's caches: the kernel step's own, or (fp8) an fp16 image of them
        if kv8:
            kc = [t.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn) for t in kc]
            vc = [t.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn) for t in vc]
            kc_ref, vc_ref = [t.half() for t in kc], [t.half() for t in vc]
        # generic: the B = 1 row runs the way every other row runs (rotation launches, decode_attention, torch tail)
        kernel_step = qp.DecodeStep(layers, embed, norm, lm_head, kc, vc, inv_freq, tok, pos, out_tok, generic=True)
        xh16 = torch.zeros(B, H, dtype=torch.float16, device=dev)      # linears-only: fixed rotated inputs
        xi16 = torch.zeros(B, I, dtype=torch.float16, device=dev)

        def linears_only():
            """the four projection groups of every layer alone, into the step's buffers"""
            h32, qkv32, ug32 = kernel_step.h32, kernel_step.qkv32, kernel_step.ug32
            h32.copy_(embed[tok])
            for layer in layers:
                att, mlp = layer.self_attn, layer.mlp
                proj, wsc, _ = att._qkv_layout()
                ugl, ugw = qp.decoder.ug_layout(mlp)
                qp.multi_gemv(proj, xh16, outs=list(qkv32.split([l.out_features for l in proj], dim=1)), wscales=wsc, oscale=att.scale)
                qp.multi_gemv([att.o_proj], xh16, outs=[h32], wscales=[att.Wscale_o], oscale=att.scale, accumulate=True)
                qp.multi_gemv(ugl, xh16, outs=list(ug32.split([l.out_features for l in ugl], dim=1)), wscales=ugw, oscale=mlp.scale)
                qp.multi_gemv([mlp.down_proj], xi16, outs=[h32], wscales=[mlp.Wscale_dp], oscale=mlp.scale, accumulate=True)

        # torch-glue reference at the same B: the Incoherent* modules, torch rope, per-sequence cache rows, SDPA with a mask per sequence
        ref_cache = BatchKV(kc_ref, vc_ref, kv8)
        ar = torch.arange(args.context, device=dev)

        def torch_step():
            h = embed[tok].view(B, 1, H)
            ang = pos.clamp(min=0).float()[:, None] * inv_freq[None, :]
            emb = torch.cat((ang, ang), dim=-1)[:, None]                  # [B, 1, head_dim]
            rope = (emb.cos().half(), emb.sin().half())
            # an inactive slot attends to row 0 only (finite, never compared)
            mask = torch.where(ar[None, :] <= pos.clamp(min=0)[:, None], 0.0, float("-inf")).half().view(B, 1, 1, -1)
            for layer in layers:
                h = layer(h, rope, mask, ref_cache, pos, glue=True)
            hn = norm(h.view(B, H))
            out_tok.copy_((hn @ lm_head.T).argmax(-1))
            return hn

        def feed(i):
            """next token at the next position of every active sequence"""
            tok.copy_(out_tok)
            torch.add(pos0, inc, alpha=i, out=pos)

        def timed(fn, before=feed):
            ms = time_graph(fn, args.tokens, dev, before)
            pos.copy_(pos0)
            return ms  # per step

        check = None
        if not args.no_torch_glue:
            # both steps from the same cache contents, tokens and positions
            kc0 = [t.clone() for t in kc]
            vc0 = [t.clone() for t in vc]
            pos.copy_(pos0)
            if kv8:  # the fp16-cache step from the same (dequantised) contents, before the reference step writes its rows
                kc16, vc16 = [t.clone() for t in kc_ref], [t.clone() for t in vc_ref]
            ref_h = torch_step().float()
            for t, t0 in zip(kc + vc, kc0 + vc0):
                t.copy_(t0)
            del kc0, vc0
            kernel_step()
            got_h = kernel_step.hidden().float()
            act = pos0 >= 0
            d = (ref_h[act] - got_h[act]).abs()
            check = {"max_abs_diff_final_norm": float(d.max()), "max_abs_ref": float(ref_h[act].abs().max()),
                     "finite": bool(torch.isfinite(got_h[act]).all())}
            if kv8:
                step16 = qp.DecodeStep(layers, embed, norm, lm_head, kc16, vc16, inv_freq, tok, pos, torch.zeros_like(out_tok), generic=True)
                step16()
                check["fp16_cache_max_abs_diff_final_norm"] = float((ref_h[act] - step16.hidden().float()[act]).abs().max())
                del step16, kc16, vc16
        ms_step = timed(kernel_step)
        paged = None
        if args.paged:
            # the same cache contents behind a block table; "pool_bytes": pools that back only the positions the run reaches
            ps, mp = args.paged, args.context // args.paged
            table = random_table(B, mp, B * mp, args.seed + B, dev)
            kp, vp = [scatter(t, table, ps, B * mp) for t in kc], [scatter(t, table, ps, B * mp) for t in vc]
            pstep = qp.DecodeStep(layers, embed, norm, lm_head, kp, vp, inv_freq, tok, pos, out_tok, generic=True, block_table=table)
            pages = int(((base[:nact] + args.tokens + ps) // ps).sum())
            paged = {"page_size": ps, "ms_step": timed(pstep), "ms_step_contiguous_again": timed(kernel_step),
                     "pool_bytes": 2 * nlayers * qp.attention.kv_cache_bytes(pages, nkv, ps, head_dim, kc[0].dtype)}
            del pstep, kp, vp, table
        windowed = None
        if args.window:
            # the same caches, tokens and positions with a window in every layer, then the plain step again (the spread)
            wstep = qp.DecodeStep(layers, embed, norm, lm_head, kc, vc, inv_freq, tok, pos, out_tok, generic=True, window=args.window)
            windowed = {"window": args.window, "ms_step": timed(wstep), "ms_step_plain_again": timed(kernel_step),
                        "kv_rows_attended_first_step": int(torch.clamp(pos0[pos0 >= 0] + 1, max=args.window).sum())}
            del wstep
        scored = None
        if args.softcap is not None or args.sinks:
            # the same caches, tokens and positions with the score modifiers in every layer, then the plain step again (the spread)
            sinks = torch.randn(nlayers, cfg.num_attention_heads, generator=torch.Generator().manual_seed(9)).to(embed.device) if args.sinks else None
            sstep = qp.DecodeStep(layers, embed, norm, lm_head, kc, vc, inv_freq, tok, pos, out_tok, generic=True, softcap=args.softcap, sinks=sinks)
            scored = {"softcap": args.softcap, "sinks": bool(args.sinks), "ms_step": timed(sstep), "ms_step_plain_again": timed(kernel_step)}
            del sstep
        blocks = None
        bg = torch.Generator().manual_seed(11)
        variants = {}
        if args.qkv_bias:
            variants["qkv_bias"] = dict(qkv_bias=torch.randn(nlayers, H + 2 * nkv * head_dim, generator=bg).to(dev))
        if args.qk_norm:
            variants["qk_norm"] = dict(qk_norm=(1e-6, (1.0 + 0.3 * torch.randn(nlayers, 2, head_dim, generator=bg)).to(dev)))
        if args.geglu:
            variants["geglu"] = dict(mlp_act="gelu_tanh")
        if args.post_norms:
            variants["post_norms"] = dict(post_norms=(1e-6, (1.0 + 0.3 * torch.randn(nlayers, 2, H, generator=bg)).to(dev)))
        if args.logit_cap is not None:
            variants["logit_cap"] = dict(logit_cap=args.logit_cap, sampler=qp.Sampler(B, args.vocab, dev, temperature=0.0))
        if variants:
            # the same caches, tokens and positions with each variant, then the plain step again (the spread)
            def variant_step(kw):
                st = qp.DecodeStep(layers, embed, norm, lm_head, kc, vc, inv_freq, tok, pos, out_tok, generic=True, **kw)
                return {"ms_step": timed(st), "launches_per_token": st.launches_per_token}
            blocks = {name: variant_step(kw) for name, kw in variants.items()}
            if "logit_cap" in variants:
                blocks["sampler_alone"] = variant_step(dict(sampler=variants["logit_cap"]["sampler"]))
            if len(variants) > 1:
                blocks["all"] = variant_step({k: v for kw in variants.values() for k, v in kw.items()})
            blocks["plain_again"] = {"ms_step": timed(kernel_step), "launches_per_token": kernel_step.launches_per_token}
        moe = None
        if moe_layers is not None:  # the same attention, caches, tokens and positions with sparse MLPs, then the dense step again
            mstep = qp.DecodeStep(moe_layers, embed, norm, lm_head, kc, vc, inv_freq, tok, pos, out_tok, generic=True)
            moe = {"experts": args.moe[0], "top_k": args.moe[1], "expert_intermediate": args.moe[2], "router": args.moe_router,
                   "shared_intermediate": args.moe_shared, "ms_step": timed(mstep),
                   "launches_per_token": mstep.launches_per_token, "ms_step_dense_again": timed(kernel_step),
                   "launches_per_token_dense": kernel_step.launches_per_token}
            del mstep
        shared = None
        if args.shared_prefix:
            P, ps, mp = args.shared_prefix, args.paged, args.context // args.paged
            own = mp - P // ps
            num_pages = P // ps + B * own
            gs = torch.Generator().manual_seed(args.seed + B + 1)
            spos0 = P + torch.randint(1, 257, (B,), generator=gs)
            spos0[nact:] = -1
            perm = torch.randperm(num_pages, generator=gs).to(torch.int32)
            table = torch.empty(B, mp, dtype=torch.int32)
            table[:, :P // ps] = perm[:P // ps]
            table[:, P // ps:] = perm[P // ps:].view(B, own)
            table, spos0 = table.to(dev), spos0.to(dev)
            sinc, spos = (spos0 >= 0).long(), spos0.clone()
            mk = lambda: [(torch.randn(num_pages, nkv, ps, head_dim, device=dev, generator=cg) * 0.5).half().to(kc[0].dtype)  # noqa: E731
                          for _ in range(nlayers)]
            kp, vp = mk(), mk()
            i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)  # noqa: E731
            px = qp.SharedPrefix(i32([0] * B), i32([0]), i32([P]))
            steps = [qp.DecodeStep(layers, embed, norm, lm_head, kp, vp, inv_freq, tok, spos, out_tok, generic=True, block_table=table,
                                   shared_prefix=sp) for sp in (None, px)]

            def sfeed(i):
                tok.copy_(out_tok)
                torch.add(spos0, sinc, alpha=i, out=spos)

            def stimed(fn):
                ms = time_graph(fn, args.tokens, dev, sfeed)
                spos.copy_(spos0)
                return ms

            hs = []
            for st in steps:  # (both append the same rows at the same places: the second starts from what the first started from)
                st()
                hs.append(st.hidden().float()[:nact])
            ms = [stimed(steps[0]), stimed(steps[1]), stimed(steps[0]), stimed(steps[1])]
            shared = {"prefix": P, "page_size": ps, "ms_step_plain": [ms[0], ms[2]], "ms_step_shared": [ms[1], ms[3]],
                      "launches_per_token": [st.launches_per_token for st in steps],
                      "max_abs_diff_final_norm": float((hs[0] - hs[1]).abs().max()), "max_abs_ref": float(hs[0].abs().max()),
                      "kv_rows_plain": int((spos0[:nact] + 1).sum()), "kv_rows_shared": int(P + (spos0[:nact] + 1 - P).sum())}
            del steps, kp, vp, table, px
        ms_lin = timed(linears_only, None)
        ms_torch = None if args.no_torch_glue else timed(torch_step)
        sampled = None
        if args.sample:
            # the same layers with the native tail: lm_head logits of all B rows + one draw per active row (two launches)
            sampled = []
            for temperature, top_k, top_p in ((0.6, 5, 1.0), (0.8, 0, 0.95)):
                smp = qp.Sampler(B, args.vocab, dev, temperature=temperature, top_k=top_k, top_p=top_p, seed=list(range(B)))
                sstep = qp.DecodeStep(layers, embed, norm, lm_head, kc, vc, inv_freq, tok, pos, out_tok, generic=True, sampler=smp)
                ms = timed(sstep)
                sampled.append({"temperature": temperature, "top_k": top_k, "top_p": top_p, "ms_step": ms, "ms_minus_greedy": ms - ms_step,
                                "tokens_per_s": nact / ms * 1e3})
                if args.process:
                    # every stage on in every slot; the step without a processor is timed again behind it (the spread of the call)
                    proc = qp.LogitProcessor(B, args.vocab, dev)
                    half = torch.arange(0, args.vocab, 2)
                    for b in range(B):
                        proc.set(b, repetition=1.3, presence=0.5, frequency=0.3)
                        proc.set_mask(b, half)
                        proc.set_bias(b, {int(i): 1.0 for i in half[:proc.bias_slots]})
                    pstep = qp.DecodeStep(layers, embed, norm, lm_head, kc, vc, inv_freq, tok, pos, out_tok, generic=True, sampler=smp,
                                          processor=proc)
                    ms_p, ms_again = timed(pstep), timed(sstep)
                    sampled[-1].update({"ms_step_processor": ms_p, "ms_step_again": ms_again, "ms_processor_minus_plain": ms_p - 0.5 * (ms + ms_again),
                                        "launches_per_token": [sstep.launches_per_token, pstep.launches_per_token]})
                    del pstep, proc
                if args.grammar:
                    # a number in every slot; the step without a bank is timed again behind it (the spread of the call)
                    from sampling_kernels import NUMBER, synthetic_table
                    bank = qp.GrammarBank(B, synthetic_table(args.vocab), dev, grammars=1, max_states=8)
                    bank.load(0, NUMBER)
                    for b in range(B):
                        bank.set(b, 0)
                    gstep = qp.DecodeStep(layers, embed, norm, lm_head, kc, vc, inv_freq, tok, pos, out_tok, generic=True, sampler=smp,
                                          grammar=bank)
                    ms_g, ms_again = timed(gstep), timed(sstep)
                    sampled[-1].update({"ms_step_grammar": ms_g, "ms_step_again_behind_grammar": ms_again,
                                        "ms_grammar_minus_plain": ms_g - 0.5 * (ms + ms_again),
                                        "grammar_launches_per_token": [sstep.launches_per_token, gstep.launches_per_token],
                                        "grammar_slots_alive_at_the_end": int((bank.state >= 0).sum())})
                    del gstep, bank
                if args.stop:
                    # strings over the vocabulary's bytes that end in a byte no token has: every token is walked, none matches
                    from sampling_kernels import synthetic_table
                    bank = qp.StopBank(B, synthetic_table(args.vocab), dev, sets=1, max_states=64, cap=512)
                    bank.load(0, [b"ab01\n", b"12.-\n", b"xx  \n", b"0.5 \n", b"a-b \n\n", b"\n\n", b"</answer>", b"###"])
                    for b in range(B):
                        bank.set(b, stop=0)
                        bank.reset(b)
                    tstep = qp.DecodeStep(layers, embed, norm, lm_head, kc, vc, inv_freq, tok, pos, out_tok, generic=True, sampler=smp,
                                          stop=bank)

                    def rewind(i):
                        """the step feeds itself: only the first replay is told where to start (the eager run and the capture moved on)"""
                        if i == 0:
                            pos.copy_(pos0)

                    ms_t, ms_again = timed(tstep, rewind), timed(sstep)
                    sampled[-1].update({"ms_step_stop": ms_t, "ms_step_again_behind_stop": ms_again,
                                        "ms_stop_minus_plain_with_host_feed": ms_t - 0.5 * (ms + ms_again),
                                        "stop_launches_per_token": [sstep.launches_per_token, tstep.launches_per_token],
                                        "stop_slots_running_at_the_end": int((bank.reason == 0).sum()),
                                        "stop_tokens_judged_per_slot": bank.n_gen.tolist()})
                    del tstep, bank
                del sstep, smp
        res = {"batch": B, "active": nact, "ms_step": ms_step, "tokens_per_s": nact / ms_step * 1e3,
               "ms_linears_only": ms_lin, "ms_torch_glue": ms_torch,
               "tokens_per_s_torch_glue": None if ms_torch is None else nact / ms_torch * 1e3,
               "kv_rows_attended_first_step": int((pos0[pos0 >= 0] + 1).sum()), "check": check, "kv": args.kv,
               "kv_cache_bytes": 2 * nlayers * qp.attention.kv_cache_bytes(B, nkv, args.context, head_dim, kc[0].dtype)}
        if sampled is not None:
            res["sampled"] = sampled
        if paged is not None:
            res["paged"] = paged
        if windowed is not None:
            res["window"] = windowed
        if scored is not None:
            res["score_mods"] = scored
        if blocks is not None:
            res["blocks"] = blocks
        if shared is not None:
            res["shared_prefix"] = shared
        if moe is not None:
            res["moe"] = moe
        del kc, vc, kc_ref, vc_ref, ref_cache, kernel_step
        torch.cuda.empty_cache()
        return res

    results = [run_batch(B) for B in args.batch]
    out = {"what": "decode step at batch B: quantized projections + batched attention (one launch per layer) + rotations",
           "model": args.model, "layers": nlayers, "quantizer": args.qdict or args.quantizer, "context": args.context,
           "tokens": args.tokens, "inactive": args.inactive, "batches": results}
    if args.stop:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        with open(os.path.join(root, "profiles", "stop.json"), "w") as f:
            json.dump({"what": "DecodeStep(stop=bank), whose last launch judges the token and moves tok / pos, against the same sampled "
                               "step followed by the host's tok.copy_(out_tok); pos += 1 (DESIGN.md §33), one MI355X, one call",
                       "command": "python perf/decode_llama_batch.py " + " ".join(sys.argv[1:] if argv is None else argv),
                       "result": out}, f, indent=1)
            f.write("\n")
    if args.qkv_bias or args.qk_norm or args.geglu or args.post_norms or args.logit_cap is not None:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        with open(os.path.join(root, "profiles", "blocks.json"), "w") as f:
            json.dump({"what": "DecodeStep with the block variants of DESIGN.md §34, each on its own, all together, and the plain step "
                               "again, one MI355X, one call",
                       "command": "python perf/decode_llama_batch.py " + " ".join(sys.argv[1:] if argv is None else argv),
                       "result": out}, f, indent=1)
            f.write("\n")
    if not quiet:
        print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
