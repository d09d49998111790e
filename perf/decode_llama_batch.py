#!/usr/bin/env python3
"""Whole-model decode step of a Llama-shaped model at batch B: B concurrent sequences, one token each per step.

The model is perf/decode_llama.py's (same random layers from this package's modules, same --model / --layers / --quantizer /
--qdict / --vocab), with per-layer KV caches [B][nkv][context][hd].  The B sequences sit at ragged, seeded positions; with
--inactive N the last N slots carry pos = -1 (free slots of a continuous-batching server: they cost nothing and change nothing).
One step at batch B:

  1. RMSNorm + sign flip + Hadamard rotation of the fp32 residual stream [B, H] (hadamard.rotate(..., rms=...): one launch)
  2. q|k|v through multi_gemv (fp32 out [B, nq*hd + 2*nkv*hd])
  3. rotary embedding + KV append + attention of every sequence: ONE launch (attention.decode_attention)
  4. o_proj's rotation, then multi_gemv(accumulate=True) into the residual stream
  5. gate|up, the SwiGLU rotation (IN_SWIGLU_F32), down_proj with accumulate=True
  6. final norm, lm_head and argmax as torch ops

The step is captured in a graph and replayed (positions advance on the device between replays).  Next to it: the same graph with
the four projection groups alone (linears-only), and a torch-glue step at the same B built from the Incoherent* modules (torch
rotary embedding, a per-sequence cache write, SDPA with a per-sequence mask), whose final normalised hidden state is the check.

    python perf/decode_llama_batch.py [--model 3_8b] [--batch 1 8 16 32 64] [--context 1024] [--tokens 64] [--inactive 0]
"""
import argparse
import json
import math
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import torch.nn as nn

import qpalette_amd as qp
from decode_llama import LINEARS, DecoderLayer, RMSNorm  # noqa: F401  (LINEARS: the projection names the layers are built from)


class BatchKV:
    """Per-sequence static caches [B][nkv][max_len][hd] with the `update` the attention module calls: row pos[b] of sequence b
    (a sequence whose position lies outside the cache keeps its cache as it is)."""

    def __init__(self, k, v):
        self.k, self.v = k, v

    def update(self, k, v, layer_idx, kwargs):
        pos = kwargs["cache_position"]
        kc, vc = self.k[layer_idx], self.v[layer_idx]
        B, L = kc.shape[0], kc.shape[2]
        live = ((pos >= 0) & (pos < L)).view(B, 1, 1)
        idx = pos.clamp(0, L - 1)
        rows = torch.arange(B, device=kc.device)
        kc[rows, :, idx] = torch.where(live, k[:, :, 0], kc[rows, :, idx])
        vc[rows, :, idx] = torch.where(live, v[:, :, 0], vc[rows, :, idx])
        return kc, vc


def main(argv=None, quiet=False):
    ap = argparse.ArgumentParser()
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
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    if args.context % 4 or args.context < args.tokens + 16:
        raise SystemExit("--context: a multiple of 4, at least --tokens + 16")
    dev = torch.device("cuda", 0)
    li = qp.mem_op.get_layer_info(args.model)
    H, I = li["mlp.gate_proj"]["in_features"], li["mlp.gate_proj"]["out_features"]
    kv_out = li["self_attn.k_proj"]["out_features"]
    head_dim = 128
    cfg = types.SimpleNamespace(hidden_size=H, intermediate_size=I, hidden_act="silu", num_attention_heads=H // head_dim,
                                num_key_value_heads=kv_out // head_dim, head_dim=head_dim, attention_dropout=0.0)
    nq, nkv = cfg.num_attention_heads, cfg.num_key_value_heads
    nlayers = args.layers or li["nlayers"]
    qdict, merge_info = None, None
    if args.qdict:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "qdicts", args.qdict + ".json")) as f:
            data = json.load(f)
        qdict, merge_info = data["qdict"], data["merge_info"]

    def qof(layer, key):
        if qdict is None:
            return args.quantizer, False
        q, simt = qdict[f"{layer}_{key}"]
        return q, simt == "1"

    gen = torch.Generator(device=dev).manual_seed(1234)
    layers = nn.ModuleList([DecoderLayer(cfg, args.model, i, qof, set(merge_info[i]) if merge_info else set(), dev, gen)
                            for i in range(nlayers)])
    qp.share_codebooks([m for m in layers.modules() if hasattr(m, "tlut") or hasattr(m, "lut")])
    embed = (torch.randn(args.vocab, H, device=dev, generator=gen) * 0.5).half()
    lm_head = (torch.randn(args.vocab, H, device=dev, generator=gen) * 0.02).half()
    norm = RMSNorm(H).to(dev)
    inv_freq = 1.0 / (500000.0 ** (torch.arange(0, head_dim, 2, device=dev).float() / head_dim))
    eps = layers[0].input_layernorm.eps
    had = qp.hadamard
    hk_hidden, K_hidden = had.get_hadK(H)
    hk_hidden = None if hk_hidden is None else hk_hidden.T.contiguous().half().to(dev)

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
        ws = qp.attention_workspace(B, nq, nkv, head_dim, args.context, dev)
        h32 = torch.zeros(B, H, dtype=torch.float32, device=dev)
        qkv32 = torch.zeros(B, H + 2 * kv_out, dtype=torch.float32, device=dev)
        a16 = torch.zeros(B, H, dtype=torch.float16, device=dev)
        ug32 = torch.zeros(B, 2 * I, dtype=torch.float32, device=dev)
        xh16 = torch.zeros(B, H, dtype=torch.float16, device=dev)      # linears-only: fixed rotated inputs
        xi16 = torch.zeros(B, I, dtype=torch.float16, device=dev)
        want_hidden = [False]

        def ug_layout(mlp):
            inter = mlp.intermediate_size
            if mlp.merge_ug:
                return [mlp.ug_proj], [mlp.Wscale_ug]
            return [mlp.up_proj, mlp.gate_proj], [mlp.Wscale_ug[:inter], mlp.Wscale_ug[inter:]]

        def layer_step(idx, layer, glue):
            att, mlp = layer.self_attn, layer.mlp
            proj, wsc, blocks = att._qkv_layout()
            outs = list(qkv32.split([l.out_features for l in proj], dim=1))
            ugl, ugw = ug_layout(mlp)
            ug_outs = list(ug32.split([l.out_features for l in ugl], dim=1))
            if not glue:
                qp.multi_gemv(proj, xh16, outs=outs, wscales=wsc, oscale=att.scale)
                qp.multi_gemv([att.o_proj], xh16, outs=[h32], wscales=[att.Wscale_o], oscale=att.scale, accumulate=True)
                qp.multi_gemv(ugl, xh16, outs=ug_outs, wscales=ugw, oscale=mlp.scale)
                qp.multi_gemv([mlp.down_proj], xi16, outs=[h32], wscales=[mlp.Wscale_dp], oscale=mlp.scale, accumulate=True)
                return
            xr = had.rotate(h32, hadK=hk_hidden, K=K_hidden, su=att.SU_qkv, post_scale=1.0 / att.scale, in_mode=had.IN_F32,
                            rms=(eps, layer.input_layernorm.weight))
            qp.multi_gemv(proj, xr, outs=outs, wscales=wsc, oscale=att.scale)
            parts = dict(zip([b[0] for b in blocks], qkv32.split([b[1] for b in blocks], dim=1)))
            qp.decode_attention(parts["q"], parts["k"], parts["v"], kc[idx], vc[idx], pos, inv_freq,
                                scale=1.0 / math.sqrt(head_dim), out=a16, ws=ws)
            xr = had.rotate(a16, hadK=hk_hidden, K=K_hidden, su=att.SU_o, post_scale=1.0 / att.scale)
            qp.multi_gemv([att.o_proj], xr, outs=[h32], wscales=[att.Wscale_o], oscale=att.scale, accumulate=True)
            xr = had.rotate(h32, hadK=hk_hidden, K=K_hidden, su=mlp.SU_ug, post_scale=1.0 / mlp.scale, in_mode=had.IN_F32,
                            rms=(eps, layer.post_attention_layernorm.weight))
            qp.multi_gemv(ugl, xr, outs=ug_outs, wscales=ugw, oscale=mlp.scale)
            xr = had.rotate(ug32, hadK=mlp.had_left_dp_T, K=mlp.inter_K, su=mlp.SU_dp, post_scale=1.0 / mlp.scale,
                            in_mode=had.IN_SWIGLU_F32)
            qp.multi_gemv([mlp.down_proj], xr, outs=[h32], wscales=[mlp.Wscale_dp], oscale=mlp.scale, accumulate=True)

        def kernel_step(glue=True):
            h32.copy_(embed[tok])
            for idx, layer in enumerate(layers):
                layer_step(idx, layer, glue)
            if not glue:
                return None
            hn = norm(h32.half())
            out_tok.copy_((hn @ lm_head.T).argmax(-1))
            return hn if want_hidden[0] else None

        # torch-glue reference at the same B: the Incoherent* modules, torch rope, per-sequence cache rows, SDPA with a mask per sequence
        ref_cache = BatchKV(kc, vc)
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

        def timed(fn, feed):
            s = torch.cuda.Stream(dev)
            with torch.cuda.stream(s):
                fn()
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=s):
                    fn()

                def one(i):
                    if feed:                                   # next token at the next position of every active sequence
                        tok.copy_(out_tok)
                        torch.add(pos0, inc, alpha=i, out=pos)
                    graph.replay()
                for i in range(8):
                    one(i)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(args.tokens):
                    one(8 + i)
                e1.record()
                torch.cuda.synchronize()
            pos.copy_(pos0)
            return e0.elapsed_time(e1) / args.tokens  # ms per step

        check = None
        if not args.no_torch_glue:
            # both steps from the same cache contents, tokens and positions
            kc0 = [t.clone() for t in kc]
            vc0 = [t.clone() for t in vc]
            pos.copy_(pos0)
            ref_h = torch_step().float()
            for t, t0 in zip(kc + vc, kc0 + vc0):
                t.copy_(t0)
            del kc0, vc0
            want_hidden[0] = True
            got_h = kernel_step().float()
            want_hidden[0] = False
            act = pos0 >= 0
            d = (ref_h[act] - got_h[act]).abs()
            check = {"max_abs_diff_final_norm": float(d.max()), "max_abs_ref": float(ref_h[act].abs().max()),
                     "finite": bool(torch.isfinite(got_h[act]).all())}
        ms_step = timed(kernel_step, True)
        ms_lin = timed(lambda: kernel_step(False), False)
        ms_torch = None if args.no_torch_glue else timed(torch_step, True)
        res = {"batch": B, "active": nact, "ms_step": ms_step, "tokens_per_s": nact / ms_step * 1e3,
               "ms_linears_only": ms_lin, "ms_torch_glue": ms_torch,
               "tokens_per_s_torch_glue": None if ms_torch is None else nact / ms_torch * 1e3,
               "kv_rows_attended_first_step": int((pos0[pos0 >= 0] + 1).sum()), "check": check}
        del kc, vc, ref_cache
        torch.cuda.empty_cache()
        return res

    results = [run_batch(B) for B in args.batch]
    out = {"what": "decode step at batch B: quantized projections + batched attention (one launch per layer) + rotations",
           "model": args.model, "layers": nlayers, "quantizer": args.qdict or args.quantizer, "context": args.context,
           "tokens": args.tokens, "inactive": args.inactive, "batches": results}
    if not quiet:
        print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
