"""Calibration: proxy Hessians of every linear layer's inputs, and the whole-model quantisation driver.

  reference_hessian(xs)            the contract of the accumulation in numpy fp64: (S = sum x x^T, s = sum x, ct = rows)
  HessianAccumulator(n, device)    S and s on the GPU, fed by qpal_hessian_accum (csrc/hessian.hip): fp16 rows in, fp64 sums;
                                   .hessian() = S / ct, .state() / .save() = the file load_hessian reads
  DenseModel / random_dense_model  a Llama-shaped fp16 model as plain tensors
  collect_hessians(model, windows) layer by layer over all windows: the inputs of q|k|v, o, up|gate and down into four accumulators;
                                   dense matmuls and norms are torch, attention is prefill_attention (the runtime's rotary
                                   convention and causal rule)
  dense_logprobs(model, windows)   the same forward to the log-probability of every next token (what a quantised model is
                                   compared with)
  quantize_model(model, quantizer, hess_dir, quant_dir)
                                   the seven quantize_linear calls per layer, then the layers as DecodeStep / Prefill / Score take them
"""
import os
import types

import numpy as np
import torch
import torch.nn as nn

from . import _native
from .attention import prefill_attention, prefill_workspace
from .linear import IncoherentMLP, IncoherentSdpaAttention
from .quantize_layer import layer_file_path, load_hessian, parse_quantizer_str, quantize_linear, random_signs

QpalError = _native.QpalError

LINEARS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj",
           "mlp.up_proj", "mlp.gate_proj", "mlp.down_proj")
HESSIAN_KEYS = ("qkv", "o", "up", "down")
# linear -> (the Hessian file of its input, its sign group: q / k / v share one SU, up / gate share one)
GROUP = {"self_attn.q_proj": ("qkv", 0), "self_attn.k_proj": ("qkv", 0), "self_attn.v_proj": ("qkv", 0), "self_attn.o_proj": ("o", 1),
         "mlp.up_proj": ("up", 2), "mlp.gate_proj": ("up", 2), "mlp.down_proj": ("down", 3)}


def reference_hessian(xs):
    """xs: fp16 arrays [rows_i, n] -> (S fp64 [n, n] = sum of x x^T over all rows, s fp64 [n] = sum of x, ct = the number of rows)."""
    S = s = None
    ct = 0
    for x in xs:
        x = np.asarray(x)
        if x.dtype != np.float16 or x.ndim != 2:
            raise ValueError("reference_hessian takes fp16 [rows, n] arrays")
        x64 = x.astype(np.float64)
        S = x64.T @ x64 if S is None else S + x64.T @ x64
        s = x64.sum(0) if s is None else s + x64.sum(0)
        ct += x.shape[0]
    return S, s, ct


class HessianAccumulator:
    """S = sum x x^T (fp64 [n, n], lower-triangle tiles only) and s = sum x (fp64 [n]) over every row given to add()."""

    def __init__(self, n, device):
        n = int(n)
        if n < 64 or n > 32768 or n % 64:
            raise QpalError(f"HessianAccumulator: n must be a multiple of 64 in 64 .. 32768, got {n}")
        self.n, self.ct, self.device = n, 0, torch.device(device)
        self.S = torch.zeros(n, n, dtype=torch.float64, device=self.device)
        self.s = torch.zeros(n, dtype=torch.float64, device=self.device)

    @classmethod
    def from_sums(cls, S, s, ct):
        """An accumulator holding the sums (S, s, ct) of reference_hessian (numpy or torch; S's lower triangle is what counts)."""
        S, s = torch.as_tensor(S, dtype=torch.float64), torch.as_tensor(s, dtype=torch.float64)
        self = cls.__new__(cls)
        self.n, self.ct, self.device, self.S, self.s = S.shape[0], int(ct), S.device, S, s
        return self

    def add(self, X):
        """X fp16 [..., n] on the accumulator's GPU, any leading shape; a 2-D view whose rows are contiguous and 16-byte aligned is
        read where it lies (row stride >= n).  One launch, no synchronisation."""
        if X.dtype != torch.float16 or X.dim() < 1 or X.shape[-1] != self.n or X.device != self.device or not X.is_cuda:
            raise QpalError(f"HessianAccumulator.add: X must be fp16 [..., {self.n}] on {self.device}")
        if X.dim() != 2:
            X = X.reshape(-1, self.n)
        rows = X.shape[0]
        if rows == 0:
            return self
        if X.stride(1) != 1 or (rows > 1 and (X.stride(0) < self.n or X.stride(0) % 8)) or X.data_ptr() % 16:
            X = X.contiguous()
            if X.data_ptr() % 16:
                X = X.clone()
        ld = X.stride(0) if rows > 1 else self.n
        with torch.cuda.device(self.device):
            rc = _native.lib().qpal_hessian_accum(self.S.data_ptr(), self.s.data_ptr(), X.data_ptr(), ld, rows, self.n,
                                                  torch.cuda.current_stream(self.device).cuda_stream)
        _native.check(rc, "qpal_hessian_accum")
        self.ct += rows
        return self

    def hessian(self):
        """S / ct, fp64 [n, n] on the accumulator's device: the lower triangle mirrored, H == H.T exactly."""
        if self.ct < 1:
            raise QpalError("HessianAccumulator: no rows yet")
        L = torch.tril(self.S)
        L += torch.tril(self.S, -1).T
        return L / self.ct

    def state(self):
        """{"flatH", "mu", "n", "ct"} (CPU tensors), the reference's Hessian file: mu = s / ct and flatH the lower triangle of
        S / ct - mu mu^T row by row (torch.tril_indices); load_hessian gives back the regularised S / ct."""
        H, mu = self.hessian(), self.s / self.ct
        H -= mu[:, None] * mu[None, :]
        idx = torch.tril_indices(self.n, self.n, device=H.device)
        return {"flatH": H[idx[0], idx[1]].cpu(), "mu": mu.cpu(), "n": self.n, "ct": self.ct}

    def save(self, path):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        torch.save(self.state(), path)
        return path


# ------------------------------------------------------------------------------------------------------------ dense model


class RMSNorm(nn.Module):
    """weight fp16 [n] and eps: what the step classes read off a norm; forward in fp32"""

    def __init__(self, weight, eps):
        super().__init__()
        self.weight = nn.Parameter(weight, requires_grad=False)
        self.eps = float(eps)

    def forward(self, x):
        x32 = x.float()
        return (x32 * torch.rsqrt(x32.square().mean(-1, keepdim=True) + self.eps) * self.weight.float()).to(x.dtype)


class DenseLayer:
    """the seven [out, in] fp16 weights of a decoder layer and its two norms"""

    def __init__(self, q, k, v, o, gate, up, down, input_layernorm, post_attention_layernorm):
        self.q, self.k, self.v, self.o, self.gate, self.up, self.down = q, k, v, o, gate, up, down
        self.input_layernorm, self.post_attention_layernorm = input_layernorm, post_attention_layernorm

    def weight(self, key):
        return getattr(self, key.split(".")[1].split("_")[0])


class DenseModel:
    """cfg (hidden_size, intermediate_size, num_attention_heads, num_key_value_heads, head_dim, hidden_act = silu), embed fp16
    [vocab, hidden], layers (DenseLayer), norm (RMSNorm), lm_head fp16 [vocab, hidden], inv_freq fp32 [head_dim / 2]."""

    def __init__(self, cfg, embed, layers, norm, lm_head, inv_freq):
        self.cfg, self.embed, self.layers, self.norm, self.lm_head, self.inv_freq = cfg, embed, layers, norm, lm_head, inv_freq


def random_dense_model(hidden, inter, nq, nkv, nlayers, vocab, seed=0, device="cuda", eps=1e-5, rope_theta=500000.0):
    """A random model of that shape: weights N(0, 1 / in), norm weights around 1, a residual stream of order 1."""
    dev = torch.device(device)
    if hidden % nq or nq % nkv:
        raise QpalError("random_dense_model: hidden % nq and nq % nkv must be 0")
    hd = hidden // nq
    g = torch.Generator().manual_seed(seed)

    def w(m, k, gain=1.0):
        return (torch.randn(m, k, generator=g) * (gain / k ** 0.5)).half().to(dev)

    def norm():
        return RMSNorm((1.0 + 0.1 * torch.randn(hidden, generator=g)).half().to(dev), eps)

    cfg = types.SimpleNamespace(hidden_size=hidden, intermediate_size=inter, hidden_act="silu", num_attention_heads=nq,
                                num_key_value_heads=nkv, head_dim=hd, attention_dropout=0.0)
    embed = torch.randn(vocab, hidden, generator=g).half().to(dev)
    layers = [DenseLayer(w(hidden, hidden), w(nkv * hd, hidden), w(nkv * hd, hidden), w(hidden, hidden, 0.5), w(inter, hidden),
                         w(inter, hidden), w(hidden, inter, 0.5), norm(), norm()) for _ in range(nlayers)]
    inv_freq = (1.0 / (rope_theta ** (torch.arange(0, hd, 2).float() / hd))).to(dev)
    return DenseModel(cfg, embed, layers, norm(), w(vocab, hidden), inv_freq)


def _check_windows(model, windows):
    if windows.dtype != torch.int64 or windows.dim() != 2 or windows.device != model.embed.device:
        raise QpalError(f"windows must be int64 [W, N] on {model.embed.device}")
    return windows.shape


def _forward(model, windows, rows_per_call, on_layer=None, on_input=None):
    """The dense forward of all windows, layer by layer, the hidden states of every window on the GPU in fp16.  Blocks of whole
    windows (about rows_per_call rows) go through a layer at a time; on_input(layer, key, X fp16 [rows, n]) sees what the layer's
    projections read, on_layer(layer) runs when a layer is through.  Returns the hidden states fp16 [W * N, hidden]."""
    W, N = _check_windows(model, windows)
    cfg, dev = model.cfg, model.embed.device
    nq, nkv, hd = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
    h = model.embed[windows.reshape(-1)]
    kc = torch.zeros(nkv, N, hd, dtype=torch.float16, device=dev)  # one slot of N positions, rewritten by every window
    vc = torch.zeros_like(kc)
    ws = prefill_workspace(min(128, N), nq, nkv, hd, N, dev)
    pos0 = torch.zeros(1, dtype=torch.int64, device=dev)
    per = max(1, int(rows_per_call) // N) * N
    for li, L in enumerate(model.layers):
        wqkv, wug = torch.cat([L.q, L.k, L.v], 0), torch.cat([L.gate, L.up], 0)
        for r0 in range(0, W * N, per):
            hb = h[r0:r0 + per]
            x = L.input_layernorm(hb)
            if on_input:
                on_input(li, "qkv", x)
            qkv = (x @ wqkv.T).float()
            q, k, v = qkv.split([nq * hd, nkv * hd, nkv * hd], dim=1)
            a = torch.empty(hb.shape[0], nq * hd, dtype=torch.float16, device=dev)
            for w0 in range(0, hb.shape[0], N):
                for c0 in range(0, N, 128):
                    rows = slice(w0 + c0, w0 + min(c0 + 128, N))
                    pos0.fill_(c0)
                    prefill_attention(q[rows], k[rows], v[rows], kc, vc, pos0, model.inv_freq, out=a[rows], ws=ws)
            if on_input:
                on_input(li, "o", a)
            hb = (hb.float() + (a @ L.o.T).float()).half()
            x = L.post_attention_layernorm(hb)
            if on_input:
                on_input(li, "up", x)
            gu = x @ wug.T
            act = (torch.nn.functional.silu(gu[:, :cfg.intermediate_size].float()) * gu[:, cfg.intermediate_size:].float()).half()
            if on_input:
                on_input(li, "down", act)
            h[r0:r0 + per] = (hb.float() + (act @ L.down.T).float()).half()
        if on_layer:
            on_layer(li)
    return h


def hessian_file_path(hess_dir, layer, key):
    """{hess_dir}/{layer}_{qkv|o|up|down}.pt"""
    return os.path.join(hess_dir, f"{layer}_{key}.pt")


def collect_hessians(model, windows, hess_dir=None, rows_per_call=4096):
    """The four proxy Hessians of every layer of `model` over the token windows int64 [W, N]: `qkv` from RMSNorm(h) * w_in (fp16),
    `o` from the attention output, `up` from RMSNorm(h') * w_post, `down` from silu(gate) * up (fp16).  An add() takes at most
    rows_per_call rows (whole windows where a window fits).  Returns {(layer, key): HessianAccumulator}; with hess_dir the files
    {hess_dir}/{layer}_{key}.pt are written layer by layer, one layer's accumulators live at a time, and the dictionary holds the
    paths."""
    cfg, dev = model.cfg, model.embed.device
    width = {"qkv": cfg.hidden_size, "o": cfg.num_attention_heads * cfg.head_dim, "up": cfg.hidden_size, "down": cfg.intermediate_size}
    out, acc = {}, {}
    step = max(1, int(rows_per_call))

    def on_input(li, key, X):
        a = acc.get(key)
        if a is None:
            a = acc[key] = HessianAccumulator(width[key], dev)
        for r0 in range(0, X.shape[0], step):
            a.add(X[r0:r0 + step])

    def on_layer(li):
        for key in HESSIAN_KEYS:
            out[(li, key)] = acc[key] if hess_dir is None else acc[key].save(hessian_file_path(hess_dir, li, key))
        acc.clear()

    _forward(model, windows, rows_per_call, on_layer, on_input)
    return out


def dense_logprobs(model, windows, rows_per_call=4096, top1=False):
    """fp32 [W, N - 1]: log p(windows[w, t + 1] | windows[w, :t + 1]) of the dense forward collect_hessians runs; with top1 also the
    most likely next token after every one of the N rows, int64 [W, N]."""
    W, N = _check_windows(model, windows)
    h = _forward(model, windows, rows_per_call).view(W, N, -1)
    out = torch.empty(W, N - 1, dtype=torch.float32, device=h.device)
    best = torch.empty(W, N, dtype=torch.int64, device=h.device)
    for w in range(W):
        logits = (model.norm(h[w]) @ model.lm_head.T).float()
        best[w] = logits.argmax(-1)
        out[w] = torch.log_softmax(logits[:-1], -1).gather(1, windows[w, 1:, None])[:, 0]
    return (out, best) if top1 else out


# ----------------------------------------------------------------------------------------------------------------- driver


class QuantizedLayer(nn.Module):
    """self_attn (IncoherentSdpaAttention), mlp (IncoherentMLP) and the two norms: a layer as the step classes take it"""

    def __init__(self, self_attn, mlp, input_layernorm, post_attention_layernorm):
        super().__init__()
        self.self_attn, self.mlp = self_attn, mlp
        self.input_layernorm, self.post_attention_layernorm = input_layernorm, post_attention_layernorm


def layer_signs(seed, layer, key, n, device="cpu"):
    """The SU of linear `key` of `layer` under quantize_model(seed=seed): random_signs from a generator seeded by (seed, layer,
    sign group), so q / k / v get one vector and up / gate get one."""
    g = torch.Generator().manual_seed((int(seed) * 1000003 + int(layer)) * 4 + GROUP[key][1])
    return random_signs(n, generator=g, device=device)


def quantize_model(model, quantizer, hess_dir, quant_dir, codebooks=None, lut_cache=None, seed=0):
    """Quantise every linear of a DenseModel and load the result: per layer seven quantize_linear calls (left_only, SU =
    layer_signs, H = load_hessian of the layer's Hessian file where the string says `hess`, save_path = layer_file_path), then
    IncoherentSdpaAttention / IncoherentMLP.gen_layer_from_quantizer_str_and_key on the files, nothing merged.  quantizer: one
    string, or {f"{layer}_{linear}": string} over LINEARS.  Returns the list of layers DecodeStep / Prefill / Score take (with
    model.embed, model.norm, model.lm_head, model.inv_freq); returned.infos holds the seven quant_info dictionaries per layer."""
    dev = model.embed.device
    layers, infos = [], []
    for li, L in enumerate(model.layers):
        qs = {key: quantizer if isinstance(quantizer, str) else quantizer[f"{li}_{key}"] for key in LINEARS}
        hess, info = {}, {}
        for key in LINEARS:
            W = L.weight(key)
            H = None
            if parse_quantizer_str(qs[key])["use_hess"]:
                hkey = GROUP[key][0]
                if hkey not in hess:
                    hess = {hkey: load_hessian(hessian_file_path(hess_dir, li, hkey))}  # (one at a time: n = 14336 is 1.6 GB)
                H = hess[hkey]
            _, info[key] = quantize_linear(W, qs[key], H=H, SU=layer_signs(seed, li, key, W.shape[1]), SV=torch.ones(W.shape[0]),
                                           left_only=True, codebooks=codebooks, lut_cache=lut_cache,
                                           save_path=layer_file_path(quant_dir, qs[key], li, key))
        q, k, v, o, u, g, d = LINEARS
        attn = IncoherentSdpaAttention.gen_layer_from_quantizer_str_and_key(
            model.cfg, li, quant_dir, qs[q], qs[k], qs[v], qs[o], f"{li}_{q}", f"{li}_{k}", f"{li}_{v}", f"{li}_{o}")
        mlp = IncoherentMLP.gen_layer_from_quantizer_str_and_key(model.cfg, quant_dir, qs[u], qs[g], qs[d], f"{li}_{u}", f"{li}_{g}",
                                                                 f"{li}_{d}")
        layers.append(QuantizedLayer(attn, mlp, L.input_layernorm, L.post_attention_layernorm).to(dev))
        infos.append(info)
    layers = nn.ModuleList(layers)
    layers.infos = infos
    return layers
