#!/usr/bin/env python3
"""End-to-end decode loop of a Llama-shaped model built from THIS package's modules.

Counterpart of the reference's eval/measure_latency.py (HF model + StaticCache + CUDA graphs): every decoder layer is
``IncoherentSdpaAttention`` + ``IncoherentMLP`` (qpalette_amd, dummy packed weights of the reference's shapes: quantizer
string per linear or a published qdict with its merge_info), with a static KV cache, rotary embedding, RMSNorm, residuals,
embedding and an fp16 lm_head.  One decode step is captured in a HIP graph and replayed.

What is NOT this package's work and is left as plain torch ops (the reference gets them fused by torch.compile, which is
Triton and therefore not used here): RMSNorm, rotary embedding, KV-cache update, SDPA, residual adds, argmax — a few
hundred small launches per token.  The script reports the whole-step rate and, next to it, the rate of the quantized
projections alone (same graph without the glue), so the two are not confused.

Third figure: the same step on this library's own glue, `qpalette_amd.DecodeStep` (q-palette_amd/decoder.py), on the same caches,
token and position; the modular step above is the reference its final normalised hidden state is checked against.

    python perf/decode_llama.py [--quantizer tcomb_6_7_0.5_none_0.9 | --qdict figure1d] [--context 1024] [--tokens 64]
"""
import argparse
import json
import math
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn

import qpalette_amd as qp

LINEARS = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj",
           "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]


class RMSNorm(nn.Module):
    def __init__(self, n, eps=1e-5):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(n, dtype=torch.float16), requires_grad=False)
        self.eps = eps

    def forward(self, x):
        return torch.nn.functional.rms_norm(x, (x.shape[-1],), self.weight, self.eps)  # one launch


class StaticKV:
    """Fixed-size key/value cache with the `update(k, v, layer_idx, kwargs)` method the attention module calls."""

    def __init__(self, nlayers, kv_heads, head_dim, max_len, device):
        shape = (1, kv_heads, max_len, head_dim)
        self.k = [torch.zeros(shape, dtype=torch.float16, device=device) for _ in range(nlayers)]
        self.v = [torch.zeros(shape, dtype=torch.float16, device=device) for _ in range(nlayers)]

    def update(self, k, v, layer_idx, kwargs):
        pos = kwargs["cache_position"]
        self.k[layer_idx].index_copy_(2, pos, k)
        self.v[layer_idx].index_copy_(2, pos, v)
        return self.k[layer_idx], self.v[layer_idx]


def _info(model_key, layer, key, qstr, device, gen):
    li = qp.mem_op.get_layer_info(model_key)[key]
    k, m = li["in_features"], li["out_features"]
    return {"quant_info": qp.mem_op.get_quant_info(qstr), "in_features": k, "out_features": m, "dtype": torch.float16,
            "bias": None,
            "linear_info": qp.mem_op.dummy_linear_info(k, m, qstr, seed=layer * 16 + LINEARS.index(key), device=device,
                                                       codebook_seed=777),
            "SU": (torch.randint(0, 2, (k,), device=device, generator=gen) * 2 - 1).half(),
            # small output scales keep the random model's residual stream finite in fp16 over 32 layers
            "Wscale": (0.001 + 0.001 * torch.rand(m, device=device, generator=gen)).half()}


class DecoderLayer(nn.Module):
    def __init__(self, cfg, model_key, layer, qof, merges, device, gen):
        super().__init__()
        inf = {key: _info(model_key, layer, key, *qof(layer, key)[:1], device, gen) for key in LINEARS}
        simt = {key: qof(layer, key)[1] for key in LINEARS}
        q, k, v, o, g, u, d = LINEARS
        self.self_attn = qp.IncoherentSdpaAttention.gen_layer_from_info(
            cfg, layer, inf[q], inf[k], inf[v], inf[o], merge_qk="merge_qk" in merges, merge_qv="merge_qv" in merges,
            merge_kv="merge_kv" in merges, merge_qkv="merge_qkv" in merges, use_simt_q=simt[q], use_simt_k=simt[k],
            use_simt_v=simt[v], use_simt_o=simt[o]).to(device)
        self.mlp = qp.IncoherentMLP.gen_layer_from_info(cfg, inf[u], inf[g], inf[d], merge_ug="merge_ug" in merges,
                                                        use_simt_u=simt[u], use_simt_g=simt[g], use_simt_d=simt[d]).to(device)
        self.input_layernorm = RMSNorm(cfg.hidden_size).to(device)
        self.post_attention_layernorm = RMSNorm(cfg.hidden_size).to(device)

    def forward(self, h, rope, mask, cache, pos, glue=True):
        if not glue:  # the quantized projections alone: q|k|v, o, up|gate (+SwiGLU rotation), down
            q, _, _ = self.self_attn.compute_qkv(h)
            self.self_attn.compute_o(q)
            self.mlp(h)
            return h
        a, _, _ = self.self_attn(self.input_layernorm(h), attention_mask=mask, past_key_value=cache, cache_position=pos,
                                 position_embeddings=rope)
        h = h + a
        return h + self.mlp(self.post_attention_layernorm(h))


def build_model(model, quantizer, qdict_name, nlayers, vocab, dev):
    """The random Llama-shaped model both decode scripts run: cfg, layers (every one or the first `nlayers`; --quantizer on every
    linear or the published perf/qdicts/<qdict_name>.json with its merge_info), embed, lm_head, the final norm, inv_freq."""
    li = qp.mem_op.get_layer_info(model)
    H, I = li["mlp.gate_proj"]["in_features"], li["mlp.gate_proj"]["out_features"]
    head_dim = 128
    cfg = types.SimpleNamespace(hidden_size=H, intermediate_size=I, hidden_act="silu", num_attention_heads=H // head_dim,
                                num_key_value_heads=li["self_attn.k_proj"]["out_features"] // head_dim, head_dim=head_dim,
                                attention_dropout=0.0)
    qdict, merge_info = None, None
    if qdict_name:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "qdicts", qdict_name + ".json")) as f:
            data = json.load(f)
        qdict, merge_info = data["qdict"], data["merge_info"]

    def qof(layer, key):
        if qdict is None:
            return quantizer, False
        q, simt = qdict[f"{layer}_{key}"]
        return q, simt == "1"

    gen = torch.Generator(device=dev).manual_seed(1234)
    layers = nn.ModuleList([DecoderLayer(cfg, model, i, qof, set(merge_info[i]) if merge_info else set(), dev, gen)
                            for i in range(nlayers or li["nlayers"])])
    qp.share_codebooks([m for m in layers.modules() if hasattr(m, "tlut") or hasattr(m, "lut")])
    embed = (torch.randn(vocab, H, device=dev, generator=gen) * 0.5).half()
    lm_head = (torch.randn(vocab, H, device=dev, generator=gen) * 0.02).half()
    inv_freq = 1.0 / (500000.0 ** (torch.arange(0, head_dim, 2, device=dev).float() / head_dim))
    return types.SimpleNamespace(cfg=cfg, layers=layers, embed=embed, lm_head=lm_head, norm=RMSNorm(H).to(dev), inv_freq=inv_freq)


WARMUP = 8


def time_graph(fn, replays, dev, before=None):
    """ms per replay of `replays` replays of fn() captured in a graph, after one eager run and WARMUP untimed replays.  The loop that
    is timed is the loop that is warmed up: `before(i)` (i counts the replays from the first untimed one) runs in front of every
    replay — a decode loop copies the sampled token in and sets the position there, two tiny launches whose FIRST use loads their
    code objects (~28 ms that round 3 had inside the timed region: 284 tok/s at 20 tokens against 472 at 64).
    Timed with events on the replay stream around the whole loop, the host loop runs ahead of the GPU."""
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            fn()

        def run(lo, hi):
            for i in range(lo, hi):
                if before is not None:
                    before(i)
                g.replay()
        run(0, WARMUP)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(WARMUP, WARMUP + replays)
        e1.record()
        torch.cuda.synchronize()
    return e0.elapsed_time(e1) / replays


def main(argv=None, quiet=False):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="3_8b", choices=sorted(qp.mem_op.LAYER_INFO))
    ap.add_argument("--quantizer", default="tcomb_6_7_0.5_none_0.9")
    ap.add_argument("--qdict", default=None, help="perf/qdicts/<name>.json (figure1c, figure1d) instead of --quantizer")
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--context", type=int, default=1024, help="static KV-cache length attended over")
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--start-pos", type=int, default=8, help="position of the first timed token (the cache below it is attended over)")
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--no-fused", action="store_true", help="skip the fused-glue step (third figure)")
    ap.add_argument("--no-swiglu-epilogue", action="store_true", help="fused step: up|gate as fp32 outputs + SwiGLU inside the rotation launch")
    ap.add_argument("--torch-lm-head", action="store_true", help="fused step: final norm, lm_head and argmax as torch ops (hipBLASLt GEMV)")
    ap.add_argument("--no-split-attention", action="store_true", help="one workgroup per query head at every context length")
    ap.add_argument("--no-modular", action="store_true", help="time the fused-glue step only (profiling)")
    ap.add_argument("--no-k28-fusion", action="store_true", help="fused step: down_proj's 28 x 512 rotation as a launch of its own (round 2)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    dev = torch.device("cuda", 0)
    m = build_model(args.model, args.quantizer, args.qdict, args.layers, args.vocab, dev)
    cfg, layers, embed, lm_head, norm, inv_freq = m.cfg, m.layers, m.embed, m.lm_head, m.norm, m.inv_freq
    H, nlayers = cfg.hidden_size, len(layers)
    cache = StaticKV(nlayers, cfg.num_key_value_heads, cfg.head_dim, args.context, dev)
    tok = torch.zeros(1, dtype=torch.long, device=dev)
    pos = torch.zeros(1, dtype=torch.long, device=dev)
    out_tok = torch.zeros(1, dtype=torch.long, device=dev)
    ar = torch.arange(args.context, device=dev)

    def step(glue=True):
        h = embed[tok].view(1, 1, H)
        rope = mask = None
        if glue:
            ang = pos.float()[:, None] * inv_freq[None, :]
            emb = torch.cat((ang, ang), dim=-1)[None]                       # [1, 1, head_dim]
            rope = (emb.cos().half(), emb.sin().half())
            mask = torch.where(ar <= pos, 0.0, float("-inf")).half().view(1, 1, 1, -1)
        for layer in layers:
            h = layer(h, rope, mask, cache, pos, glue=glue)
        if glue:
            logits = norm(h).view(1, H) @ lm_head.T
            out_tok.copy_(logits.argmax(-1))
        return h

    def feed(i):
        """the next step consumes the sampled token at the next position; the timed tokens start at --start-pos like the untimed ones"""
        tok.copy_(out_tok)
        pos.fill_(min(args.context - 1, args.start_pos + (i if i < WARMUP else i - WARMUP)))

    def timed(fn, before=feed):
        return time_graph(fn, args.tokens, dev, before) * 1e-3  # seconds per token

    # ---- fused glue (MI355X decoder block, qpalette_amd.decoder): 5 / 6 / 9 launches per layer instead of ~41
    fused = None
    if not args.no_fused and qp.decoder.fusable(layers):
        fused = qp.DecodeStep(layers, embed, norm, lm_head, cache.k, cache.v, inv_freq, tok, pos, out_tok,
                              swiglu_epilogue=not args.no_swiglu_epilogue, k28_fusion=not args.no_k28_fusion,
                              native_lm_head=not args.torch_lm_head, split_attention=not args.no_split_attention)

    # the fused step computes what the modular step computes (fp32 residual stream instead of fp16: small differences)
    check = None
    if fused and not args.no_modular:
        tok.zero_()
        pos.fill_(3)
        ref_h = norm(step(True).view(1, 1, H)).float()
        tok.zero_()
        pos.fill_(3)
        fused()
        got_h = fused.hidden().float()  # an extra torch norm, not timed
        check = {"max_abs_diff_final_norm": float((ref_h - got_h).abs().max()), "max_abs_ref": float(ref_h.abs().max())}
    if args.no_modular:
        if not fused:
            raise SystemExit("--no-modular: this configuration has no fused-glue step")
        t_fused = timed(fused)
        if not quiet:
            print(json.dumps({"model": args.model, "layers": nlayers, "quantizer": args.qdict or args.quantizer, "context": args.context,
                              "tokens_per_s_fused_glue": 1.0 / t_fused, "ms_fused_glue": t_fused * 1e3}))
        return {"ms_whole_step": None, "ms_fused_glue": t_fused * 1e3, "check": None, "launches_per_token": fused.launches_per_token}
    t_full = timed(step)
    t_proj = timed(lambda: step(False), None)
    t_fused = timed(fused) if fused else None
    finite = bool(torch.isfinite(step(True)).all())
    packed = sum(t.numel() * t.element_size() for m in layers.modules() for name in ("trellis", "trellis1", "trellis2", "qweight")
                 if (t := getattr(m, name, None)) is not None)
    print(json.dumps({
        "what": "decode step of a Llama-shaped model: incoherent quantized projections (this package) + torch glue",
        "model": args.model, "layers": nlayers, "quantizer": args.qdict or args.quantizer, "context": args.context,
        "tokens_per_s_whole_step": 1.0 / t_full, "ms_whole_step": t_full * 1e3,
        "tokens_per_s_projections_only": 1.0 / t_proj, "ms_projections_only": t_proj * 1e3,
        "glue_ms": (t_full - t_proj) * 1e3, "packed_weight_GB": packed / 1e9, "lm_head_GB": lm_head.numel() * 2 / 1e9,
        "tokens_per_s_fused_glue": (1.0 / t_fused) if t_fused else None, "ms_fused_glue": t_fused * 1e3 if t_fused else None,
        "fused_vs_modular": check, "finite": finite}))
    return {"ms_whole_step": t_full * 1e3, "ms_fused_glue": t_fused * 1e3 if t_fused else None, "check": check}


if __name__ == "__main__":
    main()
