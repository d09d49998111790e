"""A small Llama-shaped model in which every weight counts, a float64 forward of it that shares no code with decoder.py, the same
forward with the formats' rounding points, and seeded defects.  Used by test_model_exact.py; device-agnostic: the
CPU part of that file runs everything here on the host, the GPU part runs the float64 forward as torch ops on the device.

The model (build_spec / build): every RMSNorm weight 1 + 0.3 N(0, 1), two different eps, random +-1 SU per wrapper, Wscale random
per output row times a per-projection constant that a calibration pass of the float64 forward sets so that every sublayer adds
CAL_RATIO of the stream's RMS, another codec on each of the seven linears.  Effective weights: W_eff = diag(Wscale) W^ R diag(SU),
W^ the CPU oracle's decode of the packed weights, R the normalised Hadamard rotation in the convention of oracle/incoherent.py.

    spec = build_spec("S", "mixed")                       # CPU: infos, norms, embedding, the float64 model spec.ref
    m = build("S", "mixed", (), 3, VOCAB, 0, dev)         # the modules of the same model on the device (m.ref: float64 on dev)
    out = forward_fp64(m.ref, [tokens of slot 0, ...])    # out.stream[slot] [layers, N, H], .normed, .logits, .logprob [N, ...]
    emu = forward_emulated(m.ref, [...], prefill=True)    # the same with fp16 / fp32 rounding points"""
import math
import types

import numpy as np
import torch

import attn_reference as ar

LINEARS = ("q", "k", "v", "o", "gate", "up", "down")
KEYS = {"q": "self_attn.q_proj", "k": "self_attn.k_proj", "v": "self_attn.v_proj", "o": "self_attn.o_proj",
        "gate": "mlp.gate_proj", "up": "mlp.up_proj", "down": "mlp.down_proj"}
GEOMETRY = {"S": dict(H=512, nq=8, nkv=2, hd=64, I=1792), "S1": dict(H=512, nq=4, nkv=4, hd=128, I=1792),
            "F": dict(H=2048, nq=32, nkv=8, hd=64, I=14336), "F8": dict(H=2048, nq=32, nkv=8, hd=64, I=8192)}
QUANTIZERS = {
    # seven codecs on seven linears; o and down add into the stream, so they are column-split / single-stream TCQ or VQ layers
    "mixed": dict(q="tcq_6", k="tcq_3", v="ldlq_2_8", o="tcomb_3_4_0.5", gate="ldlq_1_4", up="ldlq_2_6", down="tcomb_6_7_0.5"),
    "tcomb": {n: "tcomb_6_7_0.5" for n in LINEARS},
    # q, k, v of one codec and up, gate of one codec: what a merge (and the interleaved up|gate layer of the batch-1 step) needs
    "merge": dict(q="tcq_3", k="tcq_3", v="tcq_3", o="tcomb_3_4_0.5", gate="ldlq_2_8", up="ldlq_2_8", down="tcq_6"),
    "fused": dict(q="tcq_6", k="tcq_3", v="ldlq_2_8", o="tcomb_3_4_0.5", gate="tcomb_6_7_0.5", up="tcomb_6_7_0.5", down="tcq_6"),
}
VOCAB, NLAYERS, SCALE = 1024, 3, 64.0
EPS_LAYER, EPS_FINAL, EMBED_MS = 1e-3, 1e-2, 1e-2
CAL_RATIO = 0.6          # sublayer RMS / stream RMS the calibration aims at, inside the [0.3, 1.0] the CPU test asserts
QK_RMS, V_RMS, UG_RMS = 1.25, 1.0, 1.0   # RMS of q, k | v | up, gate entries the calibration aims at (scores: sd of about 1.5)
DEFECTS = ("norm_w_swap", "final_norm_w_of_layer", "final_eps_of_layer", "no_eps", "wscale_qkv_as_q_k_v", "su_ug_is_su_qkv",
           "rope_pos_plus_1_on_k", "rope_interleaved", "cache_of_next_slot", "lost_key", "row_sees_next", "chunk_pos0_minus_1",
           "up_gate_swapped", "hadK_transposed", "o_proj_replaces_stream", "lora_of_next_slot", "lora_reads_unnormed_x",
           "lora_down_reads_plain_up_gate")


def f16(t):
    return t.to(torch.float16).double()


def f32(t):
    return t.float().double()


# ------------------------------------------------------------------------------------------------------------------- rotation
def wht(a):
    """unnormalised Walsh-Hadamard transform (Sylvester order) of the last axis"""
    n = a.shape[-1]
    lead, h = a.shape[:-1], 1
    while h < n:
        a = a.reshape(*lead, n // (2 * h), 2, h)
        a = torch.stack((a[..., 0, :] + a[..., 1, :], a[..., 0, :] - a[..., 1, :]), dim=-2)
        h *= 2
    return a.reshape(*lead, n)


def hadk_of(n, dev="cpu"):
    """the K x K factor of width n as the incoherent wrappers pass it to the rotation (had_left_T), float64, or None"""
    from qpalette_amd import hadamard as had
    hk, K = had.get_hadK(n)
    return None if hk is None else hk.T.contiguous().double().to(dev)


def rot(a, hadk):
    """(hadK (x) H_P) a / sqrt(n) of every row, a viewed as [K][P]: oracle/incoherent.py's had_blocks at hd = n"""
    n = a.shape[-1]
    K = 1 if hadk is None else hadk.shape[0]
    t = wht(a.reshape(*a.shape[:-1], K, n // K)) * float(n) ** -0.5
    if K > 1:
        t = torch.einsum("ji,...ic->...jc", hadk, t)
    return t.reshape(a.shape)


def rot_swapped(a, hadk):
    """the factors of rot in the other order, (H_P (x) hadK) / sqrt(n), a viewed as [P][K]: the seeded defect hadK_transposed (the
    28 x 28 Paley factor is symmetric, so transposing the factor alone changes nothing)"""
    if hadk is None:
        return rot(a, None)
    K, n = hadk.shape[0], a.shape[-1]
    t = a.reshape(*a.shape[:-1], n // K, K).transpose(-1, -2).reshape(a.shape)
    t = rot(t, hadk).reshape(*a.shape[:-1], K, n // K).transpose(-1, -2)
    return t.reshape(a.shape)


def rot_T(a, hadk):
    """the transpose of rot as a matrix: (hadK^T (x) H_P) / sqrt(n)"""
    return rot(a, None if hadk is None else hadk.T.contiguous())


# ---------------------------------------------------------------------------------------------------------------------- model
class Lin:
    """one linear of the float64 model: raw decoded weights What [m, k], signs su [k], Wscale [m], the rotation's K x K factor"""

    def __init__(self, What, su, wscale, hadk):
        self.What, self.su, self.wscale, self.hadk = What, su, wscale, hadk
        self._eff = None

    def eff(self, su=None, wscale=None, hadk_T=False):
        """W_eff = diag(Wscale) W^ R diag(SU) [m, k]; the arguments replace a factor (seeded defects)"""
        plain = su is None and wscale is None and not hadk_T
        if plain and self._eff is not None:
            return self._eff
        # rows of W^ R (rot_swapped is symmetric up to its factor's transpose, and that factor is symmetric where the defect is used)
        WR = rot_swapped(self.What, self.hadk) if hadk_T else rot_T(self.What, self.hadk)
        W = (self.wscale if wscale is None else wscale)[:, None] * WR * (self.su if su is None else su)[None, :]
        if plain:
            self._eff = W
        return W

    def to(self, dev):
        return Lin(self.What.to(dev), self.su.to(dev), self.wscale.to(dev), None if self.hadk is None else self.hadk.to(dev))


class Model64:
    """the float64 model: layers [{name: Lin, "ln1", "ln2"}], embed, lm_head, norm_w, inv_freq (fp32), the geometry, both eps"""

    def __init__(self, geo, layers, embed, lm_head, norm_w, inv_freq, eps_layer, eps_final):
        self.geo, self.layers, self.embed, self.lm_head, self.norm_w, self.inv_freq = geo, layers, embed, lm_head, norm_w, inv_freq
        self.eps_layer, self.eps_final = eps_layer, eps_final

    def to(self, dev):
        layers = [{k: v.to(dev) for k, v in l.items()} for l in self.layers]
        return Model64(self.geo, layers, self.embed.to(dev), self.lm_head.to(dev), self.norm_w.to(dev), self.inv_freq.to(dev),
                       self.eps_layer, self.eps_final)


class RMSNorm(torch.nn.Module):
    """what the step classes read of a norm: weight (fp16), eps, and the call hidden() makes"""

    def __init__(self, weight, eps):
        super().__init__()
        self.weight = torch.nn.Parameter(weight.clone(), requires_grad=False)
        self.eps = eps

    def forward(self, x):
        return torch.nn.functional.rms_norm(x, (x.shape[-1],), self.weight, self.eps)


def oracle_weight(qstr, info, m, k):
    """fp16 [m, k]: the CPU oracle's decode of one linear's packed weights"""
    from oracle import oracle
    if "tcomb" in qstr:
        return oracle.tcq_dequant(info["trellis1"].numpy(), info["tlut"].numpy(), m, k, info["tlut_bits"], info["KV"][0],
                                  c2=info["trellis2"].numpy(), KV2=info["KV"][1], split=2)
    if "tcq" in qstr:
        return oracle.tcq_dequant(info["trellis"].numpy(), info["tlut"].numpy(), m, k, info["tlut_bits"], info["KV"])
    return oracle.lut_tc_dequant(info["qweight"].numpy(), info["lut"].numpy(), m, k, info["lut_bits"], info["vec_sz"])


def _decode(qstr, info, m, k, dev):
    """W^ in float64 on dev: the oracle on the host; on a GPU, for the wide geometries, the layer's own get_weight(), which
    test_gpu_parity.py pins bit for bit to the oracle"""
    if torch.device(dev).type == "cuda" and m * k > (1 << 22):
        import qpalette_amd as qp
        return qp.make_linear_from_info(qstr, info).to(dev).get_weight().double()
    return torch.from_numpy(oracle_weight(qstr, info, m, k).astype(np.float64)).to(dev)


def calibration_tokens(vocab, seed, slots=4, n=24):
    g = torch.Generator().manual_seed(1000 + seed)
    return [torch.randint(0, vocab, (n,), generator=g) for _ in range(slots)]


def build_spec(geometry, quantizers, nlayers=NLAYERS, vocab=VOCAB, seed=0, device="cpu", eps_layer=EPS_LAYER, eps_final=EPS_FINAL):
    """Everything of the model that needs no module: the per-linear info dicts (quant_info, linear_info, SU, Wscale), the norms'
    weights, embed / lm_head (fp16), inv_freq, and spec.ref, the float64 model on `device`.  Every draw comes from host generators
    seeded by (seed, layer, linear): the same model on every machine.  Wscale's per-projection constants come from one float64
    pass over calibration_tokens (forward_fp64(calibrate=True)), layer after layer, then Wscale is rounded to fp16 as the modules
    hold it."""
    import qpalette_amd as qp
    geo = dict(GEOMETRY[geometry]) if isinstance(geometry, str) else dict(geometry)
    qz = QUANTIZERS[quantizers] if isinstance(quantizers, str) else dict(quantizers)
    H, I, kv = geo["H"], geo["I"], geo["nkv"] * geo["hd"]
    assert geo["nq"] * geo["hd"] == H
    shapes = {"q": (H, H), "k": (H, kv), "v": (H, kv), "o": (H, H), "gate": (H, I), "up": (H, I), "down": (I, H)}
    rng = np.random.default_rng(seed)

    def norm_w():
        return torch.from_numpy((1.0 + 0.3 * rng.standard_normal(H)).astype(np.float16))

    def signs(n):
        return torch.from_numpy((rng.integers(0, 2, n) * 2 - 1).astype(np.float16))

    infos, layers64, ln = [], [], []
    hadks = {H: hadk_of(H, device), I: hadk_of(I, device)}
    for i in range(nlayers):
        su = {"qkv": signs(H), "o": signs(H), "ug": signs(H), "down": signs(I)}
        group = {"q": "qkv", "k": "qkv", "v": "qkv", "o": "o", "gate": "ug", "up": "ug", "down": "down"}
        inf, l64 = {}, {}
        for j, name in enumerate(LINEARS):
            k, m = shapes[name]
            li = qp.mem_op.dummy_linear_info(k, m, qz[name], seed=seed * 1000 + i * 16 + j, device="cpu", codebook_seed=777)
            row = torch.from_numpy(rng.uniform(0.5, 1.5, m))
            inf[name] = {"quant_info": qp.mem_op.get_quant_info(qz[name]), "in_features": k, "out_features": m, "dtype": torch.float16,
                         "bias": None, "linear_info": li, "SU": su[group[name]], "Wscale": None, "_row": row}
            l64[name] = Lin(_decode(qz[name], li, m, k, device), su[group[name]].double().to(device), row.to(device), hadks[k])
        w1, w2 = norm_w(), norm_w()
        ln.append((w1, w2))
        l64["ln1"], l64["ln2"] = w1.double().to(device), w2.double().to(device)
        infos.append(inf)
        layers64.append(l64)
    final_w = norm_w()
    embed = torch.from_numpy((rng.standard_normal((vocab, H)) * math.sqrt(EMBED_MS)).astype(np.float16))
    lm_head = torch.from_numpy((rng.standard_normal((vocab, H)) * 0.05).astype(np.float16))
    inv_freq = 1.0 / (500000.0 ** (torch.arange(0, geo["hd"], 2).float() / geo["hd"]))
    ref = Model64(geo, layers64, embed.double().to(device), lm_head.double().to(device), final_w.double().to(device),
                  inv_freq.to(device), eps_layer, eps_final)
    forward_fp64(ref, [t.to(device) for t in calibration_tokens(vocab, seed)], calibrate=True)
    for inf, l64 in zip(infos, layers64):
        for name in LINEARS:
            inf[name]["Wscale"] = l64[name].wscale.cpu().to(torch.float16)
            assert bool((inf[name]["Wscale"].float() > 2.0 ** -14).all()), "a Wscale fell into the fp16 subnormals"
            l64[name].wscale, l64[name]._eff = inf[name]["Wscale"].double().to(device), None
            del inf[name]["_row"]
    return types.SimpleNamespace(geo=geo, quantizers=qz, infos=infos, ln=ln, final_w=final_w, embed=embed, lm_head=lm_head,
                                 inv_freq=inv_freq, eps_layer=eps_layer, eps_final=eps_final, ref=ref, vocab=vocab, seed=seed)


def build(geometry, quantizers, merges, nlayers, vocab, seed, device, spec=None):
    """The modules of build_spec's model on `device`, as the namespace perf/decode_llama.build_model returns (cfg, layers, embed,
    lm_head, norm, inv_freq), plus infos (the per-linear dicts, unmerged), spec and ref (the float64 model on `device`).  merges:
    any of "merge_qkv", "merge_qk", "merge_kv", "merge_qv", "merge_ug"."""
    import qpalette_amd as qp
    spec = build_spec(geometry, quantizers, nlayers, vocab, seed, device) if spec is None else spec
    geo, merges = spec.geo, set(merges)
    cfg = types.SimpleNamespace(hidden_size=geo["H"], intermediate_size=geo["I"], hidden_act="silu", num_attention_heads=geo["nq"],
                                num_key_value_heads=geo["nkv"], head_dim=geo["hd"], attention_dropout=0.0)
    layers = torch.nn.ModuleList()
    for i, (inf, (w1, w2)) in enumerate(zip(spec.infos, spec.ln)):
        layer = torch.nn.Module()
        layer.self_attn = qp.IncoherentSdpaAttention.gen_layer_from_info(
            cfg, i, inf["q"], inf["k"], inf["v"], inf["o"], merge_qk="merge_qk" in merges, merge_qv="merge_qv" in merges,
            merge_kv="merge_kv" in merges, merge_qkv="merge_qkv" in merges)
        layer.mlp = qp.IncoherentMLP.gen_layer_from_info(cfg, inf["up"], inf["gate"], inf["down"], merge_ug="merge_ug" in merges)
        layer.input_layernorm, layer.post_attention_layernorm = RMSNorm(w1, spec.eps_layer), RMSNorm(w2, spec.eps_layer)
        layers.append(layer.to(device))
    qp.share_codebooks([m for m in layers.modules() if hasattr(m, "tlut") or hasattr(m, "lut")])
    ref = spec.ref if spec.ref.embed.device == torch.device(device) else spec.ref.to(device)
    return types.SimpleNamespace(cfg=cfg, layers=layers, embed=spec.embed.to(device), lm_head=spec.lm_head.to(device),
                                 norm=RMSNorm(spec.final_w, spec.eps_final).to(device), inv_freq=spec.inv_freq.to(device),
                                 infos=spec.infos, spec=spec, ref=ref)


# -------------------------------------------------------------------------------------------------------------------- forward
class Out:
    """per slot: stream [layers, N, H] (the residual stream after every layer), normed [N, H], logits / logprob [N, vocab];
    ratios [layers, 2]: RMS(sublayer output) / RMS(stream it is added to) over all rows, attention then MLP"""

    def __init__(self):
        self.stream, self.normed, self.logits, self.logprob, self.ratios = [], [], [], [], None


def _rms_norm(h, w, eps, emu, two=False):
    """RMSNorm in float64; emu: glue_reference's rounding rules, norm_one_rounding for the norm fused in front of a projection,
    norm_two_roundings for the final norm (restated in torch so that they run on the device; a CPU test compares them)"""
    inv = torch.rsqrt((h * h).mean(-1, keepdim=True) + eps)
    if not emu:
        return h * inv * w
    return f16(f16(h * inv) * w) if two else f16(h * inv * w)   # glue_reference: the final norm rounds twice, the fused one once


def _rope(x, pos, inv_freq, interleaved=False):
    """x [n, heads, hd] float64 at positions pos [n]: the angle is the fp32 product float(pos) * inv_freq[i]; half-split pairs (i,
    i + hd / 2), or (seeded defect) interleaved pairs (2 i, 2 i + 1)"""
    ang = (pos.float()[:, None] * inv_freq[None, :]).double()
    c, s = ang.cos()[:, None, :], ang.sin()[:, None, :]
    if interleaved:
        x1, x2 = x[..., 0::2], x[..., 1::2]
        return torch.stack((x1 * c - x2 * s, x2 * c + x1 * s), dim=-1).flatten(-2)
    half = x.shape[-1] // 2
    x1, x2 = x[..., :half], x[..., half:]
    return torch.cat((x1 * c - x2 * s, x2 * c + x1 * s), dim=-1)


def _attend(q, Kc, Vc, pos, scale, see_next=False, lose_prev=False):
    """q [n, nq, hd] float64 at positions pos; Kc / Vc [nkv, L, hd] float64; row r attends causally to keys 0 .. pos[r]"""
    n, nq, hd = q.shape
    nkv = Kc.shape[0]
    top = int(pos.max()) + (2 if see_next else 1)
    top = min(top, Kc.shape[1])
    j = torch.arange(top, device=q.device)
    valid = j[None, :] <= (pos + (1 if see_next else 0))[:, None]
    if lose_prev:
        valid = valid & (j[None, :] != (pos - 1)[:, None])
    qg = q.reshape(n, nkv, nq // nkv, hd)
    s = torch.einsum("rgpd,gjd->rgpj", qg, Kc[:, :top]) * scale
    p = torch.softmax(s.masked_fill(~valid[:, None, None, :], float("-inf")), dim=-1)
    return torch.einsum("rgpj,gjd->rgpd", p, Vc[:, :top]).reshape(n, nq * hd)


def _forward(model, tokens_per_slot, emu, chunk, prefill, kv_dtype, lora, mutate, calibrate, context):
    geo, dev = model.geo, model.embed.device
    H, nq, nkv, hd = geo["H"], geo["nq"], geo["nkv"], geo["hd"]
    kvw, B, L = nkv * hd, len(tokens_per_slot), len(model.layers)
    scale = 1.0 / math.sqrt(hd)
    mname, mlayer = mutate if mutate else (None, None)
    if mname is not None and mname not in DEFECTS:
        raise ValueError(mname)
    toks = [torch.as_tensor(t, dtype=torch.long, device=dev).reshape(-1) for t in tokens_per_slot]
    ctx = context or max(1, max(int(t.shape[0]) for t in toks))
    h = [model.embed[t] for t in toks]
    if emu:
        h = [f32(x) for x in h]
    out = Out()
    out.stream = [[] for _ in range(B)]
    ratios = torch.zeros(L, 2, dtype=torch.float64)

    def cache_image(t):
        """what the cache holds of float64 rows t: the rows themselves; the fp16 image in the emulation; fp16 then e4m3 for kv_dtype"""
        if kv_dtype == ar.F8:
            return ar.to_cache(t.float(), ar.F8).float().double()
        return f16(t) if emu else t

    def adapter_of(b, mut):
        if lora is None:
            return -1
        sa = lora["slot_adapter"]
        return sa[(b + 1) % B] if mut == "lora_of_next_slot" else sa[b]

    def delta(i, name, b, xin, mut):
        """(alpha / r) B (A xin) of slot b's adapter on linear `name` of layer i, or 0"""
        a = adapter_of(b, mut)
        if a < 0:
            return 0.0
        w, alpha = lora["adapters"][a]
        A, Bm = (t.to(dev).double() for t in w[f"{i}_{KEYS[name]}"])
        return (alpha / A.shape[0]) * (xin @ A.T) @ Bm.T

    def apply(lin, x, **kw):
        """W_eff x; in the emulation the rotated input is rounded to fp16 (twice, around the 1 / scale) in front of W^"""
        if not emu:
            return x @ lin.eff(**kw).T
        su = kw.get("su", None)
        xr = (rot_swapped if kw.get("hadk_T") else rot)(x * (lin.su if su is None else su), lin.hadk)
        xr = f16(f16(xr) / SCALE)
        ws = kw.get("wscale", None)
        return f32((xr @ lin.What.T) * ((lin.wscale if ws is None else ws) * SCALE))

    for i, layer in enumerate(model.layers):
        mut = mname if mlayer == i else None
        eps = 0.0 if mut == "no_eps" else model.eps_layer
        Kc = [torch.zeros(nkv, ctx, hd, dtype=torch.float64, device=dev) for _ in range(B)]
        Vc = [torch.zeros(nkv, ctx, hd, dtype=torch.float64, device=dev) for _ in range(B)]
        sq = torch.zeros(4, dtype=torch.float64)
        # ---- attention
        att_out = []
        if mut == "cache_of_next_slot":   # every slot's K / V of this layer first: a slot then attends over its neighbour's real rows
            for b in range(B):
                N = toks[b].shape[0]
                if N:
                    x, pos = _rms_norm(h[b], layer["ln1"], eps, emu), torch.arange(N, device=dev)
                    k, v = (apply(layer[name], x) + delta(i, name, b, x, mut) for name in ("k", "v"))
                    Kc[b][:, pos] = cache_image(_rope(k.reshape(N, nkv, hd), pos, model.inv_freq)).transpose(0, 1)
                    Vc[b][:, pos] = cache_image(v.reshape(N, nkv, hd)).transpose(0, 1)
        for b in range(B):
            N = toks[b].shape[0]
            if N == 0:
                att_out.append(h[b])
                continue
            x = _rms_norm(h[b], layer["ln1"], eps, emu)
            xl = h[b] if mut == "lora_reads_unnormed_x" else x
            ws = {}
            if mut == "wscale_qkv_as_q_k_v":   # Wscale stored q | v | k (merge_qv), read as q | k | v
                cat = torch.cat((layer["q"].wscale, layer["v"].wscale, layer["k"].wscale))
                ws = {"q": cat[:H], "k": cat[H:H + kvw], "v": cat[H + kvw:]}
            if calibrate and b == 0:
                for name, want in (("q", QK_RMS), ("k", QK_RMS), ("v", V_RMS)):
                    y = apply(layer[name], x)
                    layer[name].wscale, layer[name]._eff = layer[name].wscale * (want / float(y.pow(2).mean().sqrt())), None
            q, k, v = (apply(layer[name], x, wscale=ws.get(name)) + delta(i, name, b, xl, mut) for name in ("q", "k", "v"))
            a = torch.zeros(N, H, dtype=torch.float64, device=dev)
            src = (b + 1) % B if mut == "cache_of_next_slot" else b
            for c0 in range(0, N, chunk):
                n = min(chunk, N - c0)
                pos = torch.arange(c0, c0 + n, device=dev)
                if mut == "chunk_pos0_minus_1" and c0 > 0:
                    pos = pos - 1
                rows = slice(c0, c0 + n)
                qi, ki, vi = q[rows].reshape(n, nq, hd), k[rows].reshape(n, nkv, hd), v[rows].reshape(n, nkv, hd)
                kpos = pos + 1 if mut == "rope_pos_plus_1_on_k" else pos
                if emu:
                    qr = ar.rope_f16(qi.float(), pos[:, None], model.inv_freq).double()
                    kr = ar.rope_f16(ki.float(), kpos[:, None], model.inv_freq).double()
                else:
                    qr = _rope(qi, pos, model.inv_freq, mut == "rope_interleaved")
                    kr = _rope(ki, kpos, model.inv_freq, mut == "rope_interleaved")
                Kc[b][:, pos] = cache_image(kr).transpose(0, 1)
                Vc[b][:, pos] = cache_image(vi).transpose(0, 1)
                if emu:
                    fmt = ar.F8 if kv_dtype == ar.F8 else ar.F16
                    a[rows] = ar.emulate(qr.reshape(n, H).half(), Kc[src].to(fmt) if fmt == ar.F16 else Kc[src].float().to(fmt),
                                         Vc[src].to(fmt) if fmt == ar.F16 else Vc[src].float().to(fmt), (pos + 1).tolist(), nq, nkv, hd,
                                         scale, 2.0 ** -11 if prefill else 0.0).double()
                else:
                    a[rows] = _attend(qr, Kc[src], Vc[src], pos, scale, see_next=mut == "row_sees_next", lose_prev=mut == "lost_key")
            y = apply(layer["o"], a)
            if calibrate:
                f = CAL_RATIO * float(h[b].pow(2).mean().sqrt()) / float(y.pow(2).mean().sqrt()) if b == 0 else 1.0
                layer["o"].wscale, layer["o"]._eff, y = layer["o"].wscale * f, None, y * f
            y = y + delta(i, "o", b, a, mut)
            sq[0] += float(y.pow(2).sum())
            sq[1] += float(h[b].pow(2).sum())
            att_out.append(y if mut == "o_proj_replaces_stream" else (f32(h[b] + y) if emu else h[b] + y))
        h = att_out
        # ---- MLP
        for b in range(B):
            if toks[b].shape[0] == 0:
                out.stream[b].append(h[b])
                continue
            x = _rms_norm(h[b], layer["ln1"] if mut == "norm_w_swap" else layer["ln2"], eps, emu)
            xl = h[b] if mut == "lora_reads_unnormed_x" else x
            su = model.layers[i]["q"].su if mut == "su_ug_is_su_qkv" else None
            if calibrate and b == 0:
                for name in ("up", "gate"):
                    y = apply(layer[name], x)
                    layer[name].wscale, layer[name]._eff = layer[name].wscale * (UG_RMS / float(y.pow(2).mean().sqrt())), None
            u0, g0 = apply(layer["up"], x, su=su), apply(layer["gate"], x, su=su)
            u, g = u0 + delta(i, "up", b, xl, mut), g0 + delta(i, "gate", b, xl, mut)
            if mut == "up_gate_swapped":
                u, g = g, u
                u0, g0 = g0, u0
            act = torch.nn.functional.silu(g) * u
            if emu:
                act = f16(act)
            y = apply(layer["down"], act, hadk_T=mut == "hadK_transposed")
            if calibrate:
                f = CAL_RATIO * float(h[b].pow(2).mean().sqrt()) / float(y.pow(2).mean().sqrt()) if b == 0 else 1.0
                layer["down"].wscale, layer["down"]._eff, y = layer["down"].wscale * f, None, y * f
            plain = torch.nn.functional.silu(g0) * u0 if mut == "lora_down_reads_plain_up_gate" else act
            y = y + delta(i, "down", b, plain, mut)
            sq[2] += float(y.pow(2).sum())
            sq[3] += float(h[b].pow(2).sum())
            h[b] = f32(h[b] + y) if emu else h[b] + y
            out.stream[b].append(h[b])
        ratios[i, 0], ratios[i, 1] = math.sqrt(sq[0] / max(sq[1], 1e-300)), math.sqrt(sq[2] / max(sq[3], 1e-300))
    out.ratios = ratios
    final_w = model.layers[mlayer]["ln1"] if mname == "final_norm_w_of_layer" else model.norm_w
    final_eps = model.eps_layer if mname == "final_eps_of_layer" else model.eps_final
    for b in range(B):
        out.stream[b] = torch.stack(out.stream[b])
        xn = _rms_norm(h[b], final_w, final_eps, emu, two=True)
        lg = xn @ model.lm_head.T
        lg = f32(lg) if emu else lg
        out.normed.append(xn)
        out.logits.append(lg)
        out.logprob.append(torch.log_softmax(lg, dim=-1))
    return out


def forward_fp64(model, tokens_per_slot, chunk=16, kv_dtype=None, lora=None, mutate=None, calibrate=False, context=None):
    """A plain Llama forward in float64: slot b's tokens stand at positions 0 .. N_b - 1 (an empty list: an inactive slot), go through
    the layers in chunks of `chunk` rows, each chunk appended to the slot's own float64 K / V and attended causally.  kv_dtype =
    torch.float8_e4m3fn: the cache holds the e4m3 image (fp16 first) of the rotated keys and the values.  lora = {"adapters":
    {id: (weights, alpha)}, "slot_adapter": [...]} in test_lora.py's raw form.  mutate = (name, layer): one of DEFECTS in one layer
    (the final-norm defects take the layer whose weight / eps they borrow).  calibrate: set the model's Wscale constants on the
    way (build_spec)."""
    return _forward(model, tokens_per_slot, False, chunk, False, kv_dtype, lora, mutate, calibrate, context)


def forward_emulated(model, tokens_per_slot, chunk=16, prefill=False, kv_dtype=None, lora=None, context=None):
    """forward_fp64 with the formats' rounding points: the fused norm's one fp16 rounding, fp16 after the rotation and after its
    1 / scale, attn_reference.rope_f16, fp16 (or e4m3) cache rows, attn_reference.emulate (fp16 output; prefill: fp16 softmax
    weights, U_PREFILL), fp16 silu(gate) up, the final norm's two roundings, fp32 stream and logits.  Says how far a correct
    implementation in these formats lies from the exact model; nothing else."""
    return _forward(model, tokens_per_slot, True, chunk, prefill, kv_dtype, lora, None, False, context)


# -------------------------------------------------------------------------------------------------------------------- measure
KAPPA, TEETH = 4.0, 4.0


def e_h(got, ref):
    """per row: ||h_got - h_ref||_2 / ||h_ref||_2"""
    return (got.double() - ref).norm(dim=-1) / ref.norm(dim=-1)


def e_l(got, ref):
    """per row: max |logit_got - logit_ref| / rms(logit_ref)"""
    return (got.double() - ref).abs().amax(-1) / ref.pow(2).mean(-1).sqrt()


def tolerance(emu_err):
    """kappa times the emulation's own distance per row, floored at the median over the rows of the case"""
    return KAPPA * torch.maximum(emu_err, emu_err.median())


def top2_gap(logits):
    t = logits.topk(2, dim=-1).values
    return t[:, 0] - t[:, 1]


def decidable(ref_logits, tol_l):
    """rows whose top-two gap exceeds twice the row's logit tolerance (tol_l is relative to the row's rms)"""
    return top2_gap(ref_logits) > 2.0 * tol_l * ref_logits.pow(2).mean(-1).sqrt()
