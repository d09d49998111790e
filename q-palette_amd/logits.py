"""Logit processors on the device: token masks, a sparse logit bias and repetition / presence / frequency penalties, applied to the
logits between ``qpal_lm_head_logits`` and ``qpal_sample`` (C-ABI ``qpal_logit_process`` / ``qpal_logit_observe``,
csrc/logit_proc.hip).

    proc = LogitProcessor(B, vocab, device)                       # per-slot state on the device, neutral
    proc.set(3, repetition=1.3, presence=0.5, frequency=0.3)      # one slot (a new request)
    proc.set_mask(3, allowed_ids)                                 # only these tokens may be drawn; None: no mask
    proc.set_bias(3, {17: 4.0, 2: -100.0})                        # a sparse logit bias; None: no bias
    observe(proc, tok, slot=slots, active=pos)                    # count[slot[r]][tok[r]] += 1
    process(smp.logits, proc, row_slot, ctr)                      # in place; then sample(smp.logits, smp, ctr)

``decoder.DecodeStep / Prefill / SpeculativeStep(..., processor=proc)`` put the two launches into their tails: a step counts the
tokens it feeds, then processes, then draws.  A captured step reads the state when it runs: the setters between replays change the
next draw.

The operation is specified exactly (include/qpal.h); ``reference_process`` restates it in numpy fp32, operation for operation, and
the kernel is held to it bit for bit.  It is fp32 and not fp64 for that reason.  CPU only, no torch.cuda, no library call.
"""
import math

import numpy as np

MAX_ROWS, MAX_EXTRA, MAX_BIAS, MAX_OBSERVE = 128, 15, 1024, 2048


def reference_process(logits, row_slot, ctr, count, repetition, presence, frequency, mask, mask_on, bias_id, bias_val, bias_n,
                      tokens=None, row0=None, out=None, vocab=None):
    """The contract of qpal_logit_process.  logits fp32 [rows, >= vocab] (vocab defaults to the width), row_slot int [rows], ctr int
    [rows]; the state: count int [slots, >= vocab], repetition / presence / frequency fp32 [slots], mask uint32 (or int32, the same
    bits) [slots, >= ceil(vocab / 32)], mask_on int [slots], bias_id int [slots, bias_slots], bias_val fp32 [slots, bias_slots],
    bias_n int [slots]; tokens int [rows] with row0 int [slots + 1]: a speculative step's rows, whose extras count.  Returns a copy
    of `out` (default: of logits) with the active rows' first vocab columns written."""
    lin = np.asarray(logits, dtype=np.float32)
    rows = lin.shape[0]
    vocab = lin.shape[1] if vocab is None else int(vocab)
    res = lin.copy() if out is None else np.array(out, dtype=np.float32)
    count = np.asarray(count)
    slots = count.shape[0]
    mask = np.ascontiguousarray(mask).view(np.uint32)
    bias_id, bias_val = np.asarray(bias_id), np.asarray(bias_val, dtype=np.float32)
    idx = np.arange(vocab)
    for r in range(rows):
        b = int(row_slot[r])
        if int(ctr[r]) < 0 or not 0 <= b < slots:
            continue
        c = count[b, :vocab].astype(np.int64)
        if tokens is not None:
            first = int(row0[b])
            if first < 0 or not 0 <= r - first <= MAX_EXTRA:
                continue
            for t in np.asarray(tokens)[first + 1:r + 1]:
                if 0 <= int(t) < vocab:
                    c[int(t)] += 1
        l = lin[r, :vocab].copy()
        rep, pres, freq = np.float32(repetition[b]), np.float32(presence[b]), np.float32(frequency[b])
        hit = (c > 0) & ~np.isnan(l)
        with np.errstate(all="ignore"):
            x = l[hit]
            x = np.where(x > 0, x / rep, x * rep).astype(np.float32)       # every operation on np.float32: rounded once
            f = (freq * c[hit].astype(np.float32)).astype(np.float32)
            s = (pres + f).astype(np.float32)
            l[hit] = (x - s).astype(np.float32)
        if int(mask_on[b]) != 0:
            allowed = (mask[b, idx >> 5] >> (idx & 31).astype(np.uint32)) & np.uint32(1)
            l[allowed == 0] = -np.inf
        n = bias_id.shape[1] if bias_id.ndim == 2 else 0
        for j in range(max(0, min(int(bias_n[b]), n)) if n else 0):
            i = int(bias_id[b, j])
            if 0 <= i < vocab and not np.isnan(l[i]):
                with np.errstate(all="ignore"):
                    l[i] = np.float32(l[i]) + np.float32(bias_val[b, j])
        res[r, :vocab] = l
    return res


def reference_observe(count, slot, tokens, active=None, vocab=None):
    """The contract of qpal_logit_observe: a copy of count int32 [slots, >= vocab] with count[slot[r]][tokens[r]] += 1 for the rows
    that count.  slot: an int per row, or one int for all rows."""
    res = np.array(count, dtype=np.int32)
    vocab = res.shape[1] if vocab is None else int(vocab)
    tokens = np.asarray(tokens, dtype=np.int64).reshape(-1)
    slot = np.broadcast_to(np.asarray(slot, dtype=np.int64), tokens.shape)
    ok = (slot >= 0) & (slot < res.shape[0]) & (tokens >= 0) & (tokens < vocab)
    if active is not None:
        ok &= np.asarray(active, dtype=np.int64).reshape(-1) >= 0
    np.add.at(res, (slot[ok], tokens[ok]), 1)
    return res


def mask_bits(allowed_ids, vocab):
    """uint32 [ceil(vocab / 32)]: bit i & 31 of word i >> 5 set for every id in allowed_ids (ids outside [0, vocab): ValueError)"""
    ids = np.asarray(list(allowed_ids) if not hasattr(allowed_ids, "__array__") else allowed_ids, dtype=np.int64).reshape(-1)
    if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= vocab):
        raise ValueError(f"mask_bits: token ids must be in 0 .. {vocab - 1}")
    bits = np.zeros((vocab + 31) // 32, dtype=np.uint32)
    np.bitwise_or.at(bits, ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
    return bits


# ---------------------------------------------------------------------------------------------------------------- GPU side

def _torch():
    import torch
    return torch


class LogitProcessor:
    """The logit processors' state of B slots on the device (what qpal_logit_process reads; include/qpal.h):

        count       int32 [B, vocab]        how often each token has been counted for the slot — B * vocab * 4 bytes: 66 MB at B = 128
                                            and vocab 128 256 (0.5 MB per slot)
        repetition, presence, frequency     fp32 [B]; neutral: 1, 0, 0
        mask        int32 [B, ceil(vocab / 32)] (the bits of a uint32: bit i & 31 of word i >> 5 set = token i allowed), mask_on int32 [B]
        bias_id     int32 [B, bias_slots], bias_val fp32 [B, bias_slots], bias_n int32 [B]: a sparse bias per slot

    A new processor is neutral: a step with it computes bit for bit what the step computes without one.  count_prompt: the steps
    count prompt tokens as well as generated ones (False: generated tokens only).  The setters are plain device writes between
    replays of a captured step, not part of one."""

    def __init__(self, B, vocab, device, bias_slots=64, count_prompt=True):
        torch = _torch()
        from ._native import QpalError
        if not 1 <= int(B) <= MAX_ROWS or not 1 <= int(vocab) <= 1 << 30 or not 0 <= int(bias_slots) <= MAX_BIAS:
            raise QpalError(f"LogitProcessor: B in 1 .. {MAX_ROWS}, vocab in 1 .. 2^30 and bias_slots in 0 .. {MAX_BIAS}, got {B}, "
                            f"{vocab}, {bias_slots}")
        self.B, self.vocab, self.device, self.bias_slots = int(B), int(vocab), torch.device(device), int(bias_slots)
        self.count_prompt = bool(count_prompt)
        z = lambda *shape, dtype=torch.int32: torch.zeros(*shape, dtype=dtype, device=self.device)
        self.count = z(self.B, self.vocab)
        self.repetition = torch.ones(self.B, dtype=torch.float32, device=self.device)
        self.presence, self.frequency = z(self.B, dtype=torch.float32), z(self.B, dtype=torch.float32)
        self.mask, self.mask_on = z(self.B, (self.vocab + 31) // 32), z(self.B)
        self.bias_id, self.bias_val = z(self.B, self.bias_slots), z(self.B, self.bias_slots, dtype=torch.float32)
        self.bias_n = z(self.B)

    def _slot(self, who, slot):
        from ._native import QpalError
        if not 0 <= int(slot) < self.B:
            raise QpalError(f"LogitProcessor.{who}: slot {slot} outside 0 .. {self.B - 1}")
        return int(slot)

    def set(self, slot, repetition=None, presence=None, frequency=None):
        """write one slot's penalties (those given): repetition > 0, all finite"""
        from ._native import QpalError
        slot = self._slot("set", slot)
        for name, v in (("repetition", repetition), ("presence", presence), ("frequency", frequency)):
            if v is not None and (not math.isfinite(float(v)) or (name == "repetition" and float(v) <= 0)):
                raise QpalError(f"LogitProcessor.set: {name} must be finite{' and > 0' if name == 'repetition' else ''}, got {v}")
        for t, v in ((self.repetition, repetition), (self.presence, presence), (self.frequency, frequency)):
            if v is not None:
                t[slot] = float(v)

    def set_mask(self, slot, allowed=None, bits=None):
        """only the token ids in `allowed` (any sequence or array of ints) may be drawn in this slot — or `bits`, the mask itself:
        ceil(vocab / 32) words, uint32 or int32 (numpy or torch); neither: the slot has no mask"""
        torch = _torch()
        from ._native import QpalError
        slot = self._slot("set_mask", slot)
        if allowed is None and bits is None:
            self.mask_on[slot] = 0
            return
        if allowed is not None and bits is not None:
            raise QpalError("LogitProcessor.set_mask: allowed ids or bits, not both")
        if bits is None:
            try:
                words = mask_bits(allowed.cpu().numpy() if isinstance(allowed, torch.Tensor) else allowed, self.vocab)
            except ValueError as e:
                raise QpalError(f"LogitProcessor.set_mask: {e}") from None
        else:
            words = bits.cpu().numpy() if isinstance(bits, torch.Tensor) else np.asarray(bits)
            if words.dtype not in (np.uint32, np.int32) or words.shape != (self.mask.shape[1],):
                raise QpalError(f"LogitProcessor.set_mask: bits must be uint32 or int32 [{self.mask.shape[1]}]")
        self.mask[slot] = torch.from_numpy(np.ascontiguousarray(words).view(np.int32).copy()).to(self.device)
        self.mask_on[slot] = 1

    def set_bias(self, slot, bias=None):
        """the slot's logit bias {token id: value} (at most bias_slots entries, distinct ids in [0, vocab), finite values); None or
        empty: no bias"""
        torch = _torch()
        from ._native import QpalError
        slot = self._slot("set_bias", slot)
        items = [] if bias is None else [(int(i), float(v)) for i, v in (bias.items() if hasattr(bias, "items") else bias)]
        if len(items) > self.bias_slots:
            raise QpalError(f"LogitProcessor.set_bias: {len(items)} entries, built for bias_slots = {self.bias_slots}")
        if len({i for i, _ in items}) != len(items):
            raise QpalError("LogitProcessor.set_bias: a token id is named twice")
        for i, v in items:
            if not 0 <= i < self.vocab or not math.isfinite(v):
                raise QpalError(f"LogitProcessor.set_bias: ids in 0 .. {self.vocab - 1} and finite values, got {i}: {v}")
        if items:
            self.bias_id[slot, :len(items)] = torch.tensor([i for i, _ in items], dtype=torch.int32).to(self.device)
            self.bias_val[slot, :len(items)] = torch.tensor([v for _, v in items], dtype=torch.float32).to(self.device)
        self.bias_n[slot] = len(items)

    def reset(self, slot):
        """the slot's counts back to zero (a new request); parameters, mask and bias stay"""
        self.count[self._slot("reset", slot)].zero_()

    def count_tokens(self, slot, tokens):
        """count `tokens` (ints, or an int64 tensor) for the slot: qpal_logit_observe in chunks of 2048 rows"""
        torch = _torch()
        slot = self._slot("count_tokens", slot)
        toks = torch.as_tensor(tokens, dtype=torch.int64).reshape(-1).to(self.device)
        for c in range(0, toks.shape[0], MAX_OBSERVE):
            observe(self, toks[c:c + MAX_OBSERVE], slot=slot)


def _arr(t, name, dtype, shape, dev, who):
    from ._native import QpalError
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != dev:
        raise QpalError(f"{who}: {name} must be a contiguous {dtype} {list(shape)} tensor on {dev}")
    return t.data_ptr()


def _state(proc, who):
    torch = _torch()
    from ._native import QpalError
    if not isinstance(proc, LogitProcessor):
        raise QpalError(f"{who}: proc must be a LogitProcessor")
    B, dev, f32, i32 = proc.B, proc.device, torch.float32, torch.int32
    return [_arr(proc.count, "count", i32, (B, proc.vocab), dev, who), proc.vocab,
            _arr(proc.repetition, "repetition", f32, (B,), dev, who), _arr(proc.presence, "presence", f32, (B,), dev, who),
            _arr(proc.frequency, "frequency", f32, (B,), dev, who),
            _arr(proc.mask, "mask", i32, (B, (proc.vocab + 31) // 32), dev, who), (proc.vocab + 31) // 32,
            _arr(proc.mask_on, "mask_on", i32, (B,), dev, who),
            _arr(proc.bias_id, "bias_id", i32, (B, proc.bias_slots), dev, who) if proc.bias_slots else None,
            _arr(proc.bias_val, "bias_val", f32, (B, proc.bias_slots), dev, who) if proc.bias_slots else None,
            _arr(proc.bias_n, "bias_n", i32, (B,), dev, who) if proc.bias_slots else None, proc.bias_slots]


def process(logits, proc, row_slot, ctr, out=None, tokens=None, row0=None, vocab=None):
    """Apply proc's state to logits fp32 [rows, >= vocab] (contiguous rows, 1 .. 128 of them; vocab defaults to proc.vocab): row r
    with slot row_slot[r] (int32 [rows]) and counter ctr[r] (int64 [rows]; < 0: inactive, the row is not written).  out: None — in
    place — or another fp32 [rows, >= vocab] tensor.  tokens int64 [rows] with row0 int32 [B + 1] (spec_draft's): a speculative
    step's rows, whose guessed tokens count for the rows behind them.  One launch on the current stream; no host read.  Returns out."""
    torch = _torch()
    from . import _native
    who, QpalError = "logits.process", _native.QpalError
    if logits.dtype != torch.float32 or not logits.is_cuda or logits.dim() != 2 or logits.stride(1) != 1:
        raise QpalError(f"{who}: logits must be an fp32 device tensor [rows, vocab] with contiguous rows")
    st = _state(proc, who)
    rows, dev = logits.shape[0], logits.device
    vocab = proc.vocab if vocab is None else int(vocab)
    ld = logits.stride(0) if rows > 1 else logits.shape[1]
    if not 1 <= rows <= MAX_ROWS or vocab != proc.vocab or vocab > logits.shape[1] or ld < vocab or dev != proc.device:
        raise QpalError(f"{who}: 1 .. {MAX_ROWS} rows of {proc.vocab} logits on {proc.device}, got {list(logits.shape)} on {dev}")
    if out is None:
        out = logits
    elif (out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != rows or out.shape[1] < vocab or out.stride(1) != 1
          or out.device != dev or (rows > 1 and out.stride(0) < vocab)):
        raise QpalError(f"{who}: out must be fp32 [{rows}, >= {vocab}] with contiguous rows on {dev}")
    ld_out = out.stride(0) if rows > 1 else out.shape[1]
    rs, cp = _arr(row_slot, "row_slot", torch.int32, (rows,), dev, who), _arr(ctr, "ctr", torch.int64, (rows,), dev, who)
    if (tokens is None) != (row0 is None):
        raise QpalError(f"{who}: tokens and row0 go together")
    ext = [None, None]
    if tokens is not None:
        ext = [_arr(tokens, "tokens", torch.int64, (rows,), dev, who), _arr(row0, "row0", torch.int32, (proc.B + 1,), dev, who)]
    with torch.cuda.device(dev):
        rc = _native.lib().qpal_logit_process(logits.data_ptr(), ld, out.data_ptr(), ld_out, rows, vocab, rs, cp, proc.B, *st, *ext,
                                              torch.cuda.current_stream(dev).cuda_stream)
    _native.check(rc, "qpal_logit_process")
    return out


def observe(proc, tokens, slot, active=None):
    """proc.count[slot[r]][tokens[r]] += 1 for the rows of tokens int64 [n], 1 <= n <= 2048.  slot: an int32 [n] tensor, or one int
    for all rows.  Skipped: rows with a slot outside the processor's, active[r] < 0 (active: an optional int64 [n], a decode step's
    positions) or a token outside [0, vocab).  One launch on the current stream; no host read."""
    torch = _torch()
    from . import _native
    who, QpalError = "logits.observe", _native.QpalError
    st = _state(proc, who)
    dev = proc.device
    if tokens.dim() != 1 or not 1 <= tokens.shape[0] <= MAX_OBSERVE:
        raise QpalError(f"{who}: tokens must be int64 [n] with 1 <= n <= {MAX_OBSERVE}")
    n = tokens.shape[0]
    tp = _arr(tokens, "tokens", torch.int64, (n,), dev, who)
    if isinstance(slot, torch.Tensor):
        sp, s0 = _arr(slot, "slot", torch.int32, (n,), dev, who), 0
    else:
        sp, s0 = None, int(slot)
        if not 0 <= s0 < proc.B:
            raise QpalError(f"{who}: slot {slot} outside 0 .. {proc.B - 1}")
    ap = None if active is None else _arr(active, "active", torch.int64, (n,), dev, who)
    if not tokens.is_cuda:
        raise QpalError(f"{who}: the state must live on a GPU, got {dev}")
    with torch.cuda.device(dev):
        rc = _native.lib().qpal_logit_observe(st[0], proc.vocab, proc.B, proc.vocab, sp, s0, tp, ap, n,
                                              torch.cuda.current_stream(dev).cuda_stream)
    _native.check(rc, "qpal_logit_observe")
