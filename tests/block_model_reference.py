"""model_reference.build's small model as a Qwen- or a Gemma-shaped model: a float64 forward with the block variants,
the same forward with the formats' rounding points, and seeded defects.  Written from model_reference's importable pieces (_rms_norm,
_rope, _attend, Lin, build_spec, build, e_h, e_l, tolerance, decidable): model_reference._forward is one function and cannot be
patched for the post-norms.  The new operations round to fp32 in the emulation; everything else rounds as forward_emulated does.

  "qwen"   qkv_bias ~ N(0, 1) times the projections' own RMS (q, k: QK_RMS, v: V_RMS); qk_norm with weights 1 + 0.3 N(0, 1).
  "gemma"  qk_norm; mlp_act = "gelu_tanh"; post_norms with weights 1 + 0.3 N(0, 1); logit_cap = CAP_RMS = 4 times the RMS of the
           uncapped logits (see below); a per-layer inv_freq (bases 10000 / 500000 / 10000); embed pre-scaled by fp16(sqrt(H)) and rounded to fp16;
           in layer 1 a soft cap of 4 on the scores and a window of 8; attn_scale 0.2 on every layer (a step has one).

    var = variant("gemma", spec.ref)                  # the variant's tensors, float64 on the model's device
    ref = forward(spec.ref, var, toks)                # .stream[slot] [layers, N, H], .logits, .logprob
    emu = forward(spec.ref, var, toks, emu=True)
    kw, embed, inv_freq = step_arguments(var, dev)    # the keyword arguments of a step class, its embed table and rotary table

The cap's magnitude.  At twice the logits' RMS the cap squeezes the top of every row — the largest of 1024 logits lies near 3.2 RMS,
where the slope of cap tanh(l / cap) is sech^2(1.6) = 0.15 — so the top-two gap shrinks sixfold while the tolerance does not, and 26 to
45 % of the rows of every token set tried (seeds 41 .. 60) are undecidable.  At 4 times the RMS the first seeds meet the cap of 10 %
(decode 41: 8 %, prefill 42: 9 %), and dropping the cap still moves the logits 102 times the tolerance.

Seeded defects (mutate=(name, layer); float64 forward only) and how far each moves the last layer's stream or the logits, in units of
the tolerance, on the decode token set of test_block_model.py (measured on the CPU by test_the_seeded_defects_leave_the_tolerance,
which prints them; the magnitudes above were chosen so that every factor is above 4):
  qwen:  bias_dropped, bias_behind_rope, qk_norm_behind_rope
  gemma: qk_norm_behind_rope, post_norm_after_add, gelu_is_silu, cap_dropped, rope_row_of_layer0, embed_unscaled
  gemma with adapters: post_norm_before_lora"""
import math
import types

import torch

import attn_reference as ar
import model_reference as mr
import score_reference as sr
from model_reference import f16, f32

DEFECTS = {"qwen": ("bias_dropped", "bias_behind_rope", "qk_norm_behind_rope"),
           "gemma": ("qk_norm_behind_rope", "post_norm_after_add", "gelu_is_silu", "cap_dropped", "rope_row_of_layer0", "embed_unscaled")}
LORA_DEFECTS = ("post_norm_before_lora",)
QK_EPS, POST_EPS = 1e-6, 1e-6
GELU_C0, GELU_C1 = 0.7978845608, 0.044715
CAP_RMS = 4.0
GEMMA_SOFTCAP, GEMMA_WINDOW, GEMMA_SCALE, GEMMA_BASES = 4.0, 8, 0.2, (10000.0, 500000.0, 10000.0)


def gelu_tanh(g):
    return 0.5 * g * (1.0 + torch.tanh(GELU_C0 * (g + GELU_C1 * g * g * g)))


def variant(kind, model, seed=7):
    """the variant's tensors for the float64 model `model` (3 layers), float64 on its device; every draw from a host generator"""
    geo, dev, L = model.geo, model.embed.device, len(model.layers)
    H, nq, nkv, hd = geo["H"], geo["nq"], geo["nkv"], geo["hd"]
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    v = types.SimpleNamespace(kind=kind, bias=None, qk=None, gelu=False, post=None, cap=None, embed=model.embed,
                              inv_freq=model.inv_freq[None, :].expand(L, -1).contiguous(), per_layer_rope=False,
                              softcap=[None] * L, window=[None] * L, scale=None)
    # both kinds norm q and k: weights 1 + 0.3 N(0, 1), rounded to the fp32 the steps hold
    v.qk = (QK_EPS, (1.0 + 0.3 * rnd(L, 2, hd)).float().double().to(dev))
    if kind == "qwen":
        rms = torch.cat((torch.full((nq * hd,), mr.QK_RMS), torch.full((nkv * hd,), mr.QK_RMS), torch.full((nkv * hd,), mr.V_RMS))).double()
        v.bias = (rnd(L, (nq + 2 * nkv) * hd) * rms).float().double().to(dev)
        return v
    assert kind == "gemma"
    v.gelu = True
    v.post = (POST_EPS, (1.0 + 0.3 * rnd(L, 2, H)).float().double().to(dev))
    v.inv_freq = torch.stack([1.0 / (GEMMA_BASES[i % 3] ** (torch.arange(0, hd, 2).float() / hd)) for i in range(L)]).to(dev)
    v.per_layer_rope = True
    # Gemma: the embedding row times fp16(sqrt(H)), rounded to the activation dtype
    v.embed = (model.embed * float(torch.tensor(math.sqrt(H)).half())).half().double()
    v.softcap, v.window, v.scale = [None, GEMMA_SOFTCAP, None][:L], [None, GEMMA_WINDOW, None][:L], GEMMA_SCALE
    # the cap: CAP_RMS times the RMS of the uncapped logits on the calibration tokens, two significant digits
    out = forward(model, v, [t.to(dev) for t in mr.calibration_tokens(model.lm_head.shape[0], 0)])
    rms = float(torch.cat(out.logits).pow(2).mean().sqrt())
    v.cap = float(f"{CAP_RMS * rms:.2g}")
    return v


def step_arguments(v, dev):
    """(keyword arguments of a step class, the embed table fp16, inv_freq fp32 [hd / 2] or [layers, hd / 2]) of a variant, on dev"""
    kw = {}
    if v.bias is not None:
        kw["qkv_bias"] = v.bias.float().to(dev).contiguous()
    if v.qk is not None:
        kw["qk_norm"] = (v.qk[0], v.qk[1].float().to(dev).contiguous())
    if v.gelu:
        kw["mlp_act"] = "gelu_tanh"
    if v.post is not None:
        kw["post_norms"] = (v.post[0], v.post[1].float().to(dev).contiguous())
    if v.cap is not None:
        kw["logit_cap"] = v.cap
    if any(c is not None for c in v.softcap):
        kw["softcap"] = list(v.softcap)
    if any(w is not None for w in v.window):
        kw["window"] = list(v.window)
    if v.scale is not None:
        kw["attn_scale"] = v.scale
    return kw, v.embed.half().to(dev), (v.inv_freq.float().to(dev).contiguous() if v.per_layer_rope else v.inv_freq[0].float().to(dev).contiguous())


def _head_norm(x, heads, hd, w, eps):
    """per-head RMSNorm of x [n, heads * hd] (or [n, heads, hd]) with the weight w [hd]"""
    shape = x.shape
    x = x.reshape(x.shape[0], heads, hd)
    return (x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * w).reshape(shape)


def _attend(q, Kc, Vc, pos, scale, window, cap):
    """model_reference._attend with the layer's window, soft cap and scale (Hugging Face's form: cap the scaled scores, then mask)"""
    if window is None and cap is None:
        return mr._attend(q, Kc, Vc, pos, scale)
    n, nq, hd = q.shape
    nkv = Kc.shape[0]
    top = int(pos.max()) + 1
    j = torch.arange(top, device=q.device)
    valid = j[None, :] <= pos[:, None]
    if window is not None:
        valid = valid & (j[None, :] >= (pos - (window - 1))[:, None])
    s = torch.einsum("rgpd,gjd->rgpj", q.reshape(n, nkv, nq // nkv, hd), Kc[:, :top]) * scale
    if cap is not None:
        s = cap * torch.tanh(s / cap)
    p = torch.softmax(s.masked_fill(~valid[:, None, None, :], float("-inf")), dim=-1)
    return torch.einsum("rgpj,gjd->rgpd", p, Vc[:, :top]).reshape(n, nq * hd)


def forward(model, var, tokens_per_slot, emu=False, chunk=16, prefill=False, kv_dtype=None, lora=None, mutate=None, context=None):
    """model_reference.forward_fp64 (emu: forward_emulated) of the model with the variant's blocks, in Hugging Face's order: q | k | v,
    their adapter update, bias, per-head QK-norm, rotary embedding (layer i: row i of the table), attention, o_proj, its adapter
    update, post-norm + add, up | gate, their update, activation, down_proj, its update, post-norm + add; final norm, lm_head, cap.
    mutate = (name, layer) seeds one defect (float64 forward only)."""
    geo, dev = model.geo, model.embed.device
    H, nq, nkv, hd = geo["H"], geo["nq"], geo["nkv"], geo["hd"]
    B, L = len(tokens_per_slot), len(model.layers)
    scale = 1.0 / math.sqrt(hd) if var.scale is None else var.scale
    mname, mlayer = mutate if mutate else (None, None)
    assert mname is None or (not emu and mname in DEFECTS["qwen"] + DEFECTS["gemma"] + LORA_DEFECTS), mname
    r32 = f32 if emu else (lambda t: t)     # the rounding of the new operations: fp32 rows
    toks = [torch.as_tensor(t, dtype=torch.long, device=dev).reshape(-1) for t in tokens_per_slot]
    ctx = context or max(1, max(int(t.shape[0]) for t in toks))
    embed = model.embed if mname == "embed_unscaled" else var.embed
    h = [r32(embed.to(dev)[t]) for t in toks]
    out = mr.Out()
    out.stream = [[] for _ in range(B)]

    def cache_image(t):
        if kv_dtype == ar.F8:
            return ar.to_cache(t.float(), ar.F8).float().double()
        return f16(t) if emu else t

    def delta(i, name, b, xin):
        """(alpha / r) B (A xin) of slot b's adapter on linear `name` of layer i, or 0"""
        a = -1 if lora is None else lora["slot_adapter"][b]
        if a < 0:
            return 0.0
        w, alpha = lora["adapters"][a]
        A, Bm = (t.to(dev).double() for t in w[f"{i}_{mr.KEYS[name]}"])
        return (alpha / A.shape[0]) * (xin @ A.T) @ Bm.T

    def apply(lin, x):
        """W_eff x; in the emulation the rotated input is rounded to fp16 (twice, around the 1 / scale) in front of W^"""
        if not emu:
            return x @ lin.eff().T
        xr = f16(f16(mr.rot(x * lin.su, lin.hadk)) / mr.SCALE)
        return f32((xr @ lin.What.T) * (lin.wscale * mr.SCALE))

    def post(i, which, hb, y, lora_delta, mut):
        """the sublayer's output y (without its adapter's update lora_delta) into the stream"""
        if var.post is None:
            return r32(hb + (y + lora_delta))
        eps, w = var.post
        if mut == "post_norm_after_add":
            s = hb + (y + lora_delta)
            return s * torch.rsqrt((s * s).mean(-1, keepdim=True) + eps) * w[i, which]
        if mut == "post_norm_before_lora":
            return hb + y * torch.rsqrt((y * y).mean(-1, keepdim=True) + eps) * w[i, which] + lora_delta
        y = r32(y + lora_delta)
        return r32(hb + y * torch.rsqrt((y * y).mean(-1, keepdim=True) + eps) * w[i, which])

    for i, layer in enumerate(model.layers):
        mut = mname if mlayer == i else None
        inv_f = var.inv_freq[0 if mut == "rope_row_of_layer0" else i]
        Kc = [torch.zeros(nkv, ctx, hd, dtype=torch.float64, device=dev) for _ in range(B)]
        Vc = [torch.zeros(nkv, ctx, hd, dtype=torch.float64, device=dev) for _ in range(B)]
        for b in range(B):
            N = toks[b].shape[0]
            if N == 0:
                out.stream[b].append(h[b])
                continue
            # ---- attention
            x = mr._rms_norm(h[b], layer["ln1"], model.eps_layer, emu)
            q, k, v = (apply(layer[name], x) + delta(i, name, b, x) for name in ("q", "k", "v"))
            if emu and lora is not None:
                q, k, v = f32(q), f32(k), f32(v)
            bq = bk = bv = None
            if var.bias is not None and mut != "bias_dropped":
                bq, bk, bv = var.bias[i].split([nq * hd, nkv * hd, nkv * hd])
                v = r32(v + bv)
                if mut != "bias_behind_rope":
                    q, k = r32(q + bq), r32(k + bk)
            qk_late = var.qk is not None and mut == "qk_norm_behind_rope"
            if var.qk is not None and not qk_late:
                q, k = r32(_head_norm(q, nq, hd, var.qk[1][i, 0], var.qk[0])), r32(_head_norm(k, nkv, hd, var.qk[1][i, 1], var.qk[0]))
            a = torch.zeros(N, H, dtype=torch.float64, device=dev)
            for c0 in range(0, N, chunk):
                n = min(chunk, N - c0)
                pos = torch.arange(c0, c0 + n, device=dev)
                rows = slice(c0, c0 + n)
                qi, ki, vi = q[rows].reshape(n, nq, hd), k[rows].reshape(n, nkv, hd), v[rows].reshape(n, nkv, hd)
                if emu:
                    qr, kr = ar.rope_f16(qi.float(), pos[:, None], inv_f).double(), ar.rope_f16(ki.float(), pos[:, None], inv_f).double()
                else:
                    qr, kr = mr._rope(qi, pos, inv_f), mr._rope(ki, pos, inv_f)
                    if mut == "bias_behind_rope":
                        qr, kr = qr + bq.reshape(nq, hd), kr + bk.reshape(nkv, hd)
                    if qk_late:
                        qr, kr = _head_norm(qr, nq, hd, var.qk[1][i, 0], var.qk[0]), _head_norm(kr, nkv, hd, var.qk[1][i, 1], var.qk[0])
                Kc[b][:, pos] = cache_image(kr).transpose(0, 1)
                Vc[b][:, pos] = cache_image(vi).transpose(0, 1)
                if emu:
                    fmt = ar.F8 if kv_dtype == ar.F8 else ar.F16
                    Kf, Vf = (t.to(fmt) if fmt == ar.F16 else t.float().to(fmt) for t in (Kc[b], Vc[b]))
                    a[rows] = sr.emulate(qr.reshape(n, H).half(), Kf, Vf, pos.tolist(), var.window[i], nq, nkv, hd, scale,
                                         2.0 ** -11 if prefill else 0.0, var.softcap[i], None).double()
                else:
                    a[rows] = _attend(qr, Kc[b], Vc[b], pos, scale, var.window[i], var.softcap[i])
            hb = post(i, 0, h[b], apply(layer["o"], a), delta(i, "o", b, a), mut)
            # ---- MLP
            x = mr._rms_norm(hb, layer["ln2"], model.eps_layer, emu)
            u, g = apply(layer["up"], x) + delta(i, "up", b, x), apply(layer["gate"], x) + delta(i, "gate", b, x)
            if var.gelu and mut != "gelu_is_silu":
                act = r32(gelu_tanh(g) * u)        # fp32 rows; the adapter's "down" update reads them as they are
                xin = f16(act) if emu else act     # the rotation takes them to fp16 on the way in
            else:
                act = torch.nn.functional.silu(g) * u
                act = xin = f16(act) if emu else act   # (as model_reference: fp16 silu(gate) * up)
            h[b] = post(i, 1, hb, apply(layer["down"], xin), delta(i, "down", b, act), mut)
            out.stream[b].append(h[b])
    cap = None if mname == "cap_dropped" else var.cap
    for b in range(B):
        out.stream[b] = torch.stack(out.stream[b])
        xn = mr._rms_norm(h[b], model.norm_w, model.eps_final, emu, two=True)
        lg = xn @ model.lm_head.T
        lg = f32(lg) if emu else lg
        if cap is not None:
            lg = r32(cap * torch.tanh(lg / cap))
        out.normed.append(xn)
        out.logits.append(lg)
        out.logprob.append(torch.log_softmax(lg, dim=-1))
    return out


def plain(model):
    """the variant with nothing in it: forward(model, plain(model), ...) is model_reference.forward_fp64 (a CPU test compares them)"""
    L = len(model.layers)
    return types.SimpleNamespace(kind="llama", bias=None, qk=None, gelu=False, post=None, cap=None, embed=model.embed,
                                 inv_freq=model.inv_freq[None, :].expand(L, -1).contiguous(), per_layer_rope=False,
                                 softcap=[None] * L, window=[None] * L, scale=None)
