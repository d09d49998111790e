"""Low-rank adapters on the quantised base: out += B[a] (A[a] xin), a per ROW, one launch per projection group.

  reference_lora(out, x, in_mode, rms, A, B, blk_off, blk_m, row_adapter)
                         the contract of qpal_lora_apply (include/qpal.h) in numpy fp64 on the stored fp16 / fp32 values; CPU only
  lora_apply(...)        the launch (csrc/lora.hip) on device tensors, same arguments
  LoraBank(layers, n_adapters, rank, B_slots, device)
                         per layer and projection group (q|k|v, o, up|gate, down) the packed A / B of every adapter, and
                         slot_adapter int32 [B_slots] on the device (-1: the slot has no adapter) — what the step classes of
                         decoder.py take as `adapters=`;  load / unload an adapter, set a slot's adapter
  load_peft_adapter(path)  a Hugging Face PEFT directory -> (weights, alpha) as LoraBank.load takes them

A weight delta cannot be folded into packed trellis or codebook codes, so the update is a launch of its own behind each group's
GEMV.  It reads the activations that ARE in memory — the fp32 residual stream, the fp16 attention output, the fp32 up | gate — and
applies the group's input transform (RMSNorm, SwiGLU) itself; A sees un-rotated activations, nothing is folded into it.
"""
import collections
import ctypes
import json
import os
import re

import numpy as np
import torch

from . import _native
from .hadamard import IN_F16, IN_F32, IN_SWIGLU_F32

QpalError = _native.QpalError

MAX_ROWS, MAX_RANK, MAX_K, MAX_BLOCKS = 128, 64, 32768, 3
# projection group -> its linears, in the order of the group's blocks of A and B
GROUPS = {"qkv": ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"), "o": ("self_attn.o_proj",),
          "ug": ("mlp.up_proj", "mlp.gate_proj"), "down": ("mlp.down_proj",)}
LINEARS = tuple(l for g in GROUPS.values() for l in g)

Group = collections.namedtuple("Group", "A B blk_off blk_m k")


def _xin(x, in_mode, rms):
    """fp64 [rows, k]: the rows' inputs under in_mode"""
    x = np.asarray(x)
    want = np.float16 if in_mode == IN_F16 else np.float32
    if in_mode not in (IN_F16, IN_F32, IN_SWIGLU_F32) or x.dtype != want or x.ndim != 2:
        raise ValueError("reference_lora: x must be fp16 [rows, k] (IN_F16), fp32 [rows, k] (IN_F32) or fp32 [rows, 2k] (IN_SWIGLU_F32)")
    x64 = x.astype(np.float64)
    if in_mode == IN_SWIGLU_F32:
        if rms is not None:
            raise ValueError("reference_lora: rms needs IN_F32")
        k = x.shape[1] // 2
        up, gate = x64[:, :k], x64[:, k:]
        return gate / (1.0 + np.exp(-gate)) * up
    if rms is not None:
        if in_mode != IN_F32:
            raise ValueError("reference_lora: rms needs IN_F32")
        eps, w = rms
        x64 = x64 / np.sqrt((x64 * x64).mean(axis=1, keepdims=True) + float(np.float32(eps)))
        if w is not None:
            w = np.asarray(w)
            if w.dtype != np.float16 or w.shape != (x.shape[1],):
                raise ValueError("reference_lora: the rms weight must be fp16 [k]")
            x64 = x64 * w.astype(np.float64)[None, :]
    return x64


def reference_lora(out, x, in_mode, rms, A, B, blk_off, blk_m, row_adapter, return_scale=False):
    """The contract of qpal_lora_apply in fp64.  out fp32 [rows, ld_out]; x as in_mode says; rms None or (eps, w fp16 [k] or None);
    A fp16 [N, P R, k]; B fp16 [N, sum blk_m, R] (alpha / r already folded in); blk_off / blk_m: P ints; row_adapter ints [rows].
    Returns out + the update as fp64 [rows, ld_out]: rows whose adapter is outside [0, N) and columns outside the blocks are out's
    own values.  return_scale: also S fp64 [rows, ld_out], S[i][off_p + j] = sum_r |B_jr| sum_l |A_rl xin_l| (0 where nothing is
    added) — what the launch's error bound is stated in."""
    out, A, B = np.asarray(out), np.asarray(A), np.asarray(B)
    if out.dtype != np.float32 or out.ndim != 2 or A.dtype != np.float16 or B.dtype != np.float16 or A.ndim != 3 or B.ndim != 3:
        raise ValueError("reference_lora: out fp32 [rows, ld_out], A fp16 [N, P R, k], B fp16 [N, M, R]")
    xin = _xin(x, in_mode, rms)
    N, R, P = A.shape[0], B.shape[2], len(blk_m)
    if A.shape[1] != P * R or A.shape[2] != xin.shape[1] or B.shape[0] != N or B.shape[1] != sum(blk_m) or len(blk_off) != P:
        raise ValueError("reference_lora: A, B and the blocks do not fit each other")
    res, scale = out.astype(np.float64), np.zeros(out.shape, dtype=np.float64)
    A64, B64, ra = A.astype(np.float64), B.astype(np.float64), np.asarray(row_adapter).reshape(-1)
    if ra.shape[0] != out.shape[0] or xin.shape[0] != out.shape[0]:
        raise ValueError("reference_lora: out, x and row_adapter must have the same rows")
    for a in range(N):
        rows = np.nonzero(ra == a)[0]  # (the rows of one adapter at a time: the sums of a row do not depend on the others)
        if rows.size == 0:
            continue
        t = xin[rows] @ A64[a].T
        tabs = np.abs(xin[rows]) @ np.abs(A64[a]).T if return_scale else None  # sum_l |A_rl xin_l| = sum_l |A_rl| |xin_l|
        boff = 0
        for p in range(P):
            Bp, cols = B64[a, boff:boff + blk_m[p]], slice(blk_off[p], blk_off[p] + blk_m[p])
            res[rows, cols] += t[:, p * R:(p + 1) * R] @ Bp.T
            if return_scale:
                scale[rows, cols] = tabs[:, p * R:(p + 1) * R] @ np.abs(Bp).T
            boff += blk_m[p]
    return (res, scale) if return_scale else res


def _ints(name, v, P):
    v = [int(e) for e in v]
    if len(v) != P:
        raise QpalError(f"lora_apply: {name} must hold {P} ints, got {len(v)}")
    return v


def lora_apply(out, x, in_mode, rms, A, B, blk_off, blk_m, row_adapter):
    """One launch of qpal_lora_apply: out[i] += B[a] (A[a] xin[i]), a = row_adapter[i], for the rows with an adapter.
    out fp32 [rows, >= the blocks' columns] (rows contiguous, any row stride); x fp16 [rows, k] (IN_F16), fp32 [rows, k] (IN_F32;
    rms = (eps, fp16 weight [k] or None) normalises the row first) or fp32 [rows, 2k] = up | gate (IN_SWIGLU_F32); A fp16 [N, P R, k];
    B fp16 [N, sum blk_m, R]; blk_off / blk_m: P <= 3 ints; row_adapter int32 [rows] on the device.  No synchronisation."""
    dev = out.device
    if not out.is_cuda:
        raise QpalError("qpalette_amd has no CPU implementation: lora_apply() needs device tensors (reference_lora is the contract)")
    if out.dtype != torch.float32 or out.dim() != 2 or out.stride(1) != 1 or (out.shape[0] > 1 and out.stride(0) < out.shape[1]):
        raise QpalError("lora_apply: out must be fp32 [rows, columns] with contiguous rows")
    rows = out.shape[0]
    ld_out = out.stride(0) if rows > 1 else out.shape[1]
    if not 1 <= rows <= MAX_ROWS:
        raise QpalError(f"lora_apply: out has {rows} rows, the launch takes 1 .. {MAX_ROWS}")
    if in_mode not in (IN_F16, IN_F32, IN_SWIGLU_F32):
        raise QpalError(f"lora_apply: in_mode must be IN_F16, IN_F32 or IN_SWIGLU_F32, got {in_mode}")
    if (A.dtype != torch.float16 or A.dim() != 3 or not A.is_contiguous() or A.device != dev or A.data_ptr() % 16):
        raise QpalError(f"lora_apply: A must be a contiguous 16-byte aligned fp16 [N, P R, k] tensor on {dev}")
    if (B.dtype != torch.float16 or B.dim() != 3 or not B.is_contiguous() or B.device != dev or B.data_ptr() % 16
            or B.shape[0] != A.shape[0]):
        raise QpalError(f"lora_apply: B must be a contiguous 16-byte aligned fp16 [N = {A.shape[0]}, sum blk_m, R] tensor on {dev}")
    N, k, R = A.shape[0], A.shape[2], B.shape[2]
    P = len(blk_m)
    if not 1 <= P <= MAX_BLOCKS:
        raise QpalError(f"lora_apply: blk_m must name 1 .. {MAX_BLOCKS} blocks, got {P}")
    blk_off, blk_m = _ints("blk_off", blk_off, P), _ints("blk_m", blk_m, P)
    if R % 8 or not 8 <= R <= MAX_RANK or A.shape[1] != P * R:
        raise QpalError(f"lora_apply: the rank (B's last dimension) must be a multiple of 8 in 8 .. {MAX_RANK} and A [N, {P} R, k], "
                        f"got R = {R}, A {list(A.shape)}")
    if k % 64 or not 64 <= k <= MAX_K:
        raise QpalError(f"lora_apply: k (A's last dimension) must be a multiple of 64 in 64 .. {MAX_K}, got {k}")
    if any(m < 16 or m % 16 for m in blk_m) or sum(blk_m) != B.shape[1]:
        raise QpalError(f"lora_apply: blk_m must be multiples of 16 that add up to B's {B.shape[1]} rows, got {blk_m}")
    spans = sorted(zip(blk_off, blk_m))
    if spans[0][0] < 0 or any(o + m > o2 for (o, m), (o2, _) in zip(spans, spans[1:])) or spans[-1][0] + spans[-1][1] > out.shape[1]:
        raise QpalError(f"lora_apply: blk_off must place disjoint blocks inside out's {out.shape[1]} columns, got {blk_off} / {blk_m}")
    want, width = (torch.float16, k) if in_mode == IN_F16 else (torch.float32, k if in_mode == IN_F32 else 2 * k)
    if x.dtype != want or tuple(x.shape) != (rows, width) or not x.is_contiguous() or x.device != dev or x.data_ptr() % 16:
        raise QpalError(f"lora_apply: x must be a contiguous 16-byte aligned {want} [{rows}, {width}] tensor on {dev}")
    eps, w = -1.0, None
    if rms is not None:
        if in_mode != IN_F32:
            raise QpalError("lora_apply: rms needs in_mode IN_F32")
        eps, w = float(rms[0]), rms[1]
        if not eps >= 0.0:
            raise QpalError(f"lora_apply: the rms eps must be >= 0, got {eps}")
        if w is not None and (w.dtype != torch.float16 or w.numel() != k or not w.is_contiguous() or w.device != dev or w.data_ptr() % 16):
            raise QpalError(f"lora_apply: the rms weight must be a contiguous 16-byte aligned fp16 vector of {k} elements on {dev}")
    if (row_adapter.dtype != torch.int32 or tuple(row_adapter.shape) != (rows,) or not row_adapter.is_contiguous()
            or row_adapter.device != dev):
        raise QpalError(f"lora_apply: row_adapter must be a contiguous int32 [{rows}] tensor on {dev}")
    arr = ctypes.c_int * P
    with torch.cuda.device(dev):
        rc = _native.lib().qpal_lora_apply(out.data_ptr(), ld_out, x.data_ptr(), in_mode, eps, w.data_ptr() if w is not None else None,
                                           A.data_ptr(), B.data_ptr(), arr(*blk_off), arr(*blk_m), P, row_adapter.data_ptr(), rows, k,
                                           R, N, torch.cuda.current_stream(dev).cuda_stream)
    _native.check(rc, "qpal_lora_apply")
    return out


class LoraBank:
    """The adapters a step can apply.  layers: the modules the step classes take (self_attn: IncoherentSdpaAttention, mlp:
    IncoherentMLP) — only their shapes and `_qkv_layout()` are read; n_adapters: N, the adapter ids are 0 .. N - 1; rank: R, a
    multiple of 8 up to 64 (adapters of lower rank are zero-padded); B_slots: the sequences of the caches; device: a GPU, or "cpu"
    (packing only: nothing launches from a CPU bank).

    Per layer i and group g in ("qkv", "o", "ug", "down"), bank.group(i, g) is (A fp16 [N, P R, k], B fp16 [N, sum blk_m, R],
    blk_off, blk_m, k): the blocks of "qkv" are q, k, v at the columns `_qkv_layout()` gives them in the step's q|k|v buffer (merged
    or not), those of "ug" up, gate at 0 and intermediate_size.  bank.slot_adapter int32 [B_slots], all -1 at first.

    Between replays of a captured step `set` changes what a slot runs with; `load` / `unload` rewrite the tensors the captured
    launches read, in place (stream-ordered copies: not inside a capture)."""

    def __init__(self, layers, n_adapters, rank, B_slots, device):
        N, R, S = int(n_adapters), int(rank), int(B_slots)
        if N < 1 or S < 1 or R % 8 or not 8 <= R <= MAX_RANK:
            raise QpalError(f"LoraBank: n_adapters and B_slots must be >= 1 and rank a multiple of 8 in 8 .. {MAX_RANK}, "
                            f"got {n_adapters}, {B_slots}, {rank}")
        self.n_adapters, self.rank, self.slots, self.device = N, R, S, torch.device(device)
        self.slot_adapter = torch.full((S,), -1, dtype=torch.int32, device=self.device)
        self.groups = []
        for i, layer in enumerate(layers):
            att, mlp = layer.self_attn, layer.mlp
            H, kv, inter = att.hidden_size, att.kv_out, mlp.intermediate_size
            at, off = {}, 0
            for name, width in att._qkv_layout()[2]:
                at[name] = off
                off += width
            shapes = {"qkv": (H, [at["q"], at["k"], at["v"]], [H, kv, kv]), "o": (H, [0], [H]),
                      "ug": (H, [0, inter], [inter, inter]), "down": (inter, [0], [H])}
            g = {}
            for name, (k, blk_off, blk_m) in shapes.items():
                if k % 64 or k > MAX_K or any(m % 16 for m in blk_m):
                    raise QpalError(f"LoraBank: layer {i} {name}: k = {k} must be a multiple of 64 up to {MAX_K}, widths {blk_m} of 16")
                g[name] = Group(torch.zeros(N, len(blk_m) * R, k, dtype=torch.float16, device=self.device),
                                torch.zeros(N, sum(blk_m), R, dtype=torch.float16, device=self.device), blk_off, blk_m, k)
            self.groups.append(g)

    def group(self, layer, name):
        return self.groups[layer][name]

    def _check_id(self, who, adapter_id):
        if not 0 <= int(adapter_id) < self.n_adapters:
            raise QpalError(f"LoraBank.{who}: adapter_id {adapter_id} outside 0 .. {self.n_adapters - 1}")
        return int(adapter_id)

    def load(self, adapter_id, weights, alpha):
        """weights: {f"{layer}_{linear}": (A [r, k], B [m, r])} over any subset of LINEARS ("self_attn.q_proj" ... "mlp.down_proj")
        and layers, numpy or torch, any float dtype, r <= rank.  The adapter's delta of that linear is (alpha / r) B A.  Packing:
        A rounded to fp16 into rows p R .. p R + r - 1 of the group's A (the rest zero); B times alpha / r in fp32, rounded to
        fp16 ONCE, into columns 0 .. r - 1 of the block's rows of B.  A linear the dictionary does not name is zero rows of both.
        Whatever the adapter held before is replaced."""
        a = self._check_id("load", adapter_id)
        known = {f"{i}_{lin}" for i in range(len(self.groups)) for lin in LINEARS}
        for key in weights:
            if key not in known:
                raise QpalError(f"LoraBank.load: {key!r} names no linear of these {len(self.groups)} layers "
                                f"(keys are '<layer>_<linear>', linear in {LINEARS})")
        staged = []
        for i, g in enumerate(self.groups):
            for name, linears in GROUPS.items():
                grp = g[name]
                A = torch.zeros(grp.A.shape[1:], dtype=torch.float16)
                B = torch.zeros(grp.B.shape[1:], dtype=torch.float16)
                boff = 0
                for p, lin in enumerate(linears):
                    m = grp.blk_m[p]
                    if f"{i}_{lin}" in weights:
                        wa, wb = (torch.as_tensor(w).detach().cpu() for w in weights[f"{i}_{lin}"])
                        r = wa.shape[0] if wa.dim() == 2 else -1
                        if not 1 <= r <= self.rank or tuple(wa.shape) != (r, grp.k) or tuple(wb.shape) != (m, r):
                            raise QpalError(f"LoraBank.load: {i}_{lin}: A must be [r <= {self.rank}, {grp.k}] and B [{m}, r], got "
                                            f"{list(wa.shape)} and {list(wb.shape)}")
                        A[p * self.rank:p * self.rank + r] = wa.to(torch.float16)
                        B[boff:boff + m, :r] = (wb.to(torch.float32) * torch.tensor(float(alpha) / r, dtype=torch.float32)).to(torch.float16)
                    boff += m
                staged.append((grp, A, B))
        for grp, A, B in staged:  # (nothing is written before every entry has passed its checks)
            grp.A[a].copy_(A)
            grp.B[a].copy_(B)

    def unload(self, adapter_id):
        """zeroes the adapter's A and B: rows that still name it get an update of exactly 0"""
        a = self._check_id("unload", adapter_id)
        for g in self.groups:
            for grp in g.values():
                grp.A[a].zero_()
                grp.B[a].zero_()

    def set(self, slot, adapter_id):
        """slot `slot` runs with adapter `adapter_id` (-1: none) from the next step, or replay of a captured step, on: one 4-byte
        host-to-device write, outside any capture"""
        if not 0 <= int(slot) < self.slots:
            raise QpalError(f"LoraBank.set: slot {slot} outside the bank's {self.slots} slots")
        if int(adapter_id) != -1:
            self._check_id("set", adapter_id)
        self.slot_adapter[int(slot):int(slot) + 1].copy_(torch.tensor([int(adapter_id)], dtype=torch.int32))

    def bytes(self):
        """the size of the bank's tensors"""
        return self.slot_adapter.numel() * 4 + sum(grp.A.numel() * 2 + grp.B.numel() * 2 for g in self.groups for grp in g.values())


_PEFT_KEY = re.compile(r"(?:^|\.)layers\.(\d+)\.(self_attn|mlp)\.([a-z]+_proj)\.lora_([AB])(?:\.[A-Za-z0-9_]+)?\.weight$")


def load_peft_adapter(path):
    """A Hugging Face PEFT LoRA directory -> (weights, alpha): adapter_config.json (r, lora_alpha, target_modules) and
    adapter_model.safetensors, whose keys look like '...layers.{i}.self_attn.q_proj.lora_A.weight'.  weights is
    {f"{layer}_{linear}": (A [r, k], B [m, r])} as stored (LoraBank.load folds alpha / r in).  What this library does not apply
    raises QpalError naming the key: use_dora, use_rslora, modules_to_save, rank_pattern / alpha_pattern, bias terms, targets
    outside the seven linears of a layer."""
    from safetensors.torch import load_file
    with open(os.path.join(path, "adapter_config.json")) as f:
        cfg = json.load(f)
    for key in ("use_dora", "use_rslora", "modules_to_save", "rank_pattern", "alpha_pattern"):
        if cfg.get(key):
            raise QpalError(f"load_peft_adapter: {key} = {cfg[key]!r} is not supported")
    if cfg.get("bias", "none") != "none":
        raise QpalError(f"load_peft_adapter: bias = {cfg['bias']!r} is not supported (no bias terms)")
    if cfg.get("peft_type", "LORA") != "LORA":
        raise QpalError(f"load_peft_adapter: peft_type = {cfg['peft_type']!r} is not supported")
    for key in ("r", "lora_alpha", "target_modules"):
        if key not in cfg:
            raise QpalError(f"load_peft_adapter: adapter_config.json has no {key}")
    targets = cfg["target_modules"]
    names = {lin.split(".")[1] for lin in LINEARS}
    if isinstance(targets, str) or any(t.split(".")[-1] not in names for t in targets):
        raise QpalError(f"load_peft_adapter: target_modules = {targets!r}: only lists of {sorted(names)} are supported")
    r, parts = int(cfg["r"]), {}
    for key, t in load_file(os.path.join(path, "adapter_model.safetensors")).items():
        mt = _PEFT_KEY.search(key)
        lin = f"{mt.group(2)}.{mt.group(3)}" if mt else None
        if lin not in LINEARS:
            raise QpalError(f"load_peft_adapter: tensor {key!r} is not a LoRA matrix of one of {LINEARS}")
        parts.setdefault(f"{int(mt.group(1))}_{lin}", {})[mt.group(4)] = (key, t)
    weights = {}
    for name, ab in parts.items():
        if set(ab) != {"A", "B"}:
            raise QpalError(f"load_peft_adapter: {name} has lora_{'A' if 'A' in ab else 'B'} only ({next(iter(ab.values()))[0]!r})")
        (ka, A), (kb, B) = ab["A"], ab["B"]
        if A.dim() != 2 or B.dim() != 2 or A.shape[0] != r or B.shape[1] != r:
            raise QpalError(f"load_peft_adapter: {ka!r} / {kb!r}: shapes {list(A.shape)} / {list(B.shape)} do not have r = {r}")
        weights[name] = (A, B)
    return weights, float(cfg["lora_alpha"])
