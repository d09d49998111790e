"""Speculative decoding, the two ends of a step (C-ABI ``qpal_spec_draft`` / ``qpal_spec_accept``, csrc/spec.hip).

A step feeds, per slot, the pending token and up to K guessed tokens as one segment of a ragged step, draws at EVERY row the token the
model would have drawn at that position (the draw is a function of seed, position, logits and parameters: §14.1), and keeps the
guesses that equal the draws.  The emitted stream is token for token what one-token-at-a-time sampling emits on the same logits.

    spec_draft(hist, n_tok, limit, K, gram, max_len, tokens, seq, row0, pos0, row_slot, row_ctr, n_draft)   # state -> step inputs
    ... the ragged step on `tokens`, one draw per row with ctr = row_ctr -> drawn ...
    spec_accept(tokens, drawn, seq, row0, hist, n_tok, limit, eos, out_tok, n_out, n_acc)                  # draws -> state

``decoder.SpeculativeStep`` is the whole step.  ``reference_spec_draft`` / ``reference_spec_accept`` restate the two contracts in
plain numpy: they are the specification the kernels are held to, bit for bit (CPU only, no torch, no library call).
"""
import numpy as np

MAX_SLOTS, MAX_DRAFT, MAX_GRAM, MAX_ROWS = 128, 15, 8, 128


def _active(n, lim, max_len, ld_hist):
    return 1 <= n < lim and n <= max_len and n <= ld_hist


def lookup(h, gmin, gmax):
    """prompt lookup on the known tokens h [n]: the index the drafts start at, or None.  For g = gmax down to gmin with g < n: the
    largest j with j + g < n and h[j : j + g] == h[n - g :]; the first g that has one gives j + g."""
    h = np.asarray(h)
    n = h.shape[0]
    for g in range(gmax, gmin - 1, -1):
        if g >= n:
            continue
        # windows h[j : j + g] for j = 0 .. n - g - 1 (j + g < n), each against the suffix
        hits = np.nonzero((np.lib.stride_tricks.sliding_window_view(h[:n - 1], g) == h[n - g:]).all(axis=1))[0]
        if hits.size:
            return int(hits[-1]) + g
    return None


def reference_spec_draft(hist, n_tok, limit, K, gmin, gmax, R, max_len, ext_draft=None, ext_n=None):
    """The contract of qpal_spec_draft.  hist int [B, ld_hist], n_tok / limit int [B]; ext_draft int [B, K] and ext_n int [B], or
    None: prompt lookup.  Returns a dict of numpy arrays: tokens int64 [R], seq int32 [B], row0 int32 [B + 1], pos0 int64 [B],
    row_slot int32 [R], row_ctr int64 [R], n_draft int32 [B]."""
    hist = np.asarray(hist)
    B, ld = hist.shape
    if not (1 <= B <= MAX_SLOTS and 0 <= K <= MAX_DRAFT and 1 <= gmin <= gmax <= MAX_GRAM and B <= R <= MAX_ROWS and max_len >= 1):
        raise ValueError("reference_spec_draft: B, K, gram, R or max_len outside the contract")
    n_tok, limit = [int(v) for v in n_tok], [int(v) for v in limit]
    act = [_active(n_tok[b], limit[b], max_len, ld) for b in range(B)]
    drafts = []
    for b in range(B):
        d = []
        if act[b]:
            n = n_tok[b]
            d_max = max(0, min(K, limit[b] - n - 1, max_len - n))
            if ext_draft is not None:
                for t in list(np.asarray(ext_draft)[b][:max(0, min(int(ext_n[b]), d_max))]):
                    if not 0 <= int(t) < 2 ** 30:
                        break
                    d.append(int(t))
            elif d_max > 0:
                at = lookup(hist[b, :n], gmin, gmax)
                if at is not None:
                    d = [int(t) for t in hist[b, at:min(at + d_max, n)]]
        drafts.append(d)
    out = dict(tokens=np.zeros(R, np.int64), seq=np.full(B, -1, np.int32), row0=np.zeros(B + 1, np.int32), pos0=np.zeros(B, np.int64),
               row_slot=np.full(R, -1, np.int32), row_ctr=np.full(R, -1, np.int64), n_draft=np.zeros(B, np.int32))
    at = 0
    for b in range(B):
        out["pos0"][b] = n_tok[b] - 1
        if act[b]:
            later = sum(act[b + 1:])                      # every active slot keeps its one row
            d = drafts[b][:max(0, R - at - 1 - later)]    # drafts are cut where R is full
            rows = [int(hist[b, n_tok[b] - 1])] + d
            out["tokens"][at:at + len(rows)] = rows
            out["row_slot"][at:at + len(rows)] = b
            out["row_ctr"][at:at + len(rows)] = n_tok[b] - 1 + np.arange(len(rows))
            out["seq"][b], out["n_draft"][b] = b, len(d)
            at += len(rows)
        out["row0"][b + 1] = at
    return out


def reference_spec_accept(tokens, drawn, seq, row0, hist, n_tok, limit, eos, K, out_tok=None):
    """The contract of qpal_spec_accept.  Returns a dict: hist, n_tok, limit (the advanced state, copies), out_tok int64 [B, K + 1]
    (a copy of `out_tok` where given, else zeros, with the emitted tokens written), n_out int32 [B], n_acc int32 [B]."""
    tokens, drawn = np.asarray(tokens, np.int64), np.asarray(drawn, np.int64)
    hist = np.array(hist, dtype=np.int32)
    B, ld = hist.shape
    R = tokens.shape[0]
    n_tok, limit = np.array(n_tok, dtype=np.int64), np.array(limit, dtype=np.int64)
    out = np.zeros((B, K + 1), np.int64) if out_tok is None else np.array(out_tok, dtype=np.int64)
    n_out, n_acc = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        r, T = int(row0[b]), int(row0[b + 1]) - int(row0[b])
        n, lim = int(n_tok[b]), int(limit[b])
        if not (int(seq[b]) == b and 1 <= T <= K + 1 and r >= 0 and r + T <= R and 1 <= n < lim):
            continue
        m = 0
        while m < T - 1 and tokens[r + m + 1] == drawn[r + m]:
            m += 1
        emitted = [int(t) for t in drawn[r:r + m + 1]][:lim - n]
        stop = int(eos[b])
        if stop >= 0 and stop in emitted:
            emitted = emitted[:emitted.index(stop) + 1]
            limit[b] = n + len(emitted)
        for i, t in enumerate(emitted):
            out[b, i] = t
            if n + i < ld:
                hist[b, n + i] = t
        n_tok[b] = n + len(emitted)
        n_out[b], n_acc[b] = len(emitted), m
    return dict(hist=hist, n_tok=n_tok, limit=limit, out_tok=out, n_out=n_out, n_acc=n_acc)


# ---------------------------------------------------------------------------------------------------------------- GPU side

def _torch():
    import torch
    return torch


def _arr(t, name, dtype, shape, dev, who):
    from ._native import QpalError
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise QpalError(f"{who}: {name} must be a contiguous {dtype} {list(shape)} tensor")
    if t.device != dev:
        raise QpalError(f"{who}: {name} must be on {dev}")
    return t.data_ptr()


def _state(who, hist, n_tok, limit):
    torch = _torch()
    from ._native import QpalError
    if hist.dtype != torch.int32 or hist.dim() != 2 or not hist.is_contiguous() or hist.shape[1] < 1:
        raise QpalError(f"{who}: hist must be a contiguous int32 [B, ld_hist] tensor")
    B, dev = hist.shape[0], hist.device
    if not 1 <= B <= MAX_SLOTS:
        raise QpalError(f"{who}: 1 .. {MAX_SLOTS} slots, got {B}")
    return B, dev, [_arr(n_tok, "n_tok", torch.int64, (B,), dev, who), _arr(limit, "limit", torch.int64, (B,), dev, who)]


def spec_draft(hist, n_tok, limit, K, gram, max_len, tokens, seq, row0, pos0, row_slot, row_ctr, n_draft, ext_draft=None, ext_n=None):
    """One ragged step's inputs from the state (the contract: include/qpal.h, reference_spec_draft).  hist int32 [B, ld_hist], n_tok /
    limit int64 [B]; K the draft length 0 .. 15, gram = (gmin, gmax) within 1 .. 8, max_len the cache's positions.  Written: tokens
    int64 [R] (B <= R <= 128), seq int32 [B], row0 int32 [B + 1], pos0 int64 [B], row_slot int32 [R], row_ctr int64 [R], n_draft
    int32 [B].  ext_draft int64 [B, K] with ext_n int32 [B]: the caller's drafts instead of prompt lookup.  Everything is a device
    tensor the host never reads; two launches on the current stream."""
    torch = _torch()
    from . import _native
    who, QpalError = "spec_draft", _native.QpalError
    B, dev, st = _state(who, hist, n_tok, limit)
    K, (gmin, gmax), max_len = int(K), (int(gram[0]), int(gram[1])), int(max_len)
    if not 0 <= K <= MAX_DRAFT or not 1 <= gmin <= gmax <= MAX_GRAM or max_len < 1:
        raise QpalError(f"{who}: K must be in 0 .. {MAX_DRAFT}, 1 <= gmin <= gmax <= {MAX_GRAM} and max_len >= 1, got {K}, {gram}, {max_len}")
    if tokens.dim() != 1 or not B <= tokens.shape[0] <= MAX_ROWS:
        raise QpalError(f"{who}: tokens must be int64 [R] with {B} <= R <= {MAX_ROWS}")
    R = tokens.shape[0]
    outs = [_arr(tokens, "tokens", torch.int64, (R,), dev, who), _arr(seq, "seq", torch.int32, (B,), dev, who),
            _arr(row0, "row0", torch.int32, (B + 1,), dev, who), _arr(pos0, "pos0", torch.int64, (B,), dev, who),
            _arr(row_slot, "row_slot", torch.int32, (R,), dev, who), _arr(row_ctr, "row_ctr", torch.int64, (R,), dev, who),
            _arr(n_draft, "n_draft", torch.int32, (B,), dev, who)]
    ext = [None, None]
    if ext_draft is not None:
        if ext_n is None:
            raise QpalError(f"{who}: ext_draft needs ext_n")
        ext = [_arr(ext_draft, "ext_draft", torch.int64, (B, K), dev, who), _arr(ext_n, "ext_n", torch.int32, (B,), dev, who)]
    if not hist.is_cuda:
        raise QpalError(f"{who}: the state must live on a GPU, got {dev}")
    with torch.cuda.device(dev):
        rc = _native.lib().qpal_spec_draft(hist.data_ptr(), hist.shape[1], *st, *ext, B, K, gmin, gmax, R, max_len, *outs,
                                           torch.cuda.current_stream(dev).cuda_stream)
    _native.check(rc, "qpal_spec_draft")


def spec_accept(tokens, drawn, seq, row0, hist, n_tok, limit, eos, out_tok, n_out, n_acc):
    """The draws of every row -> the emitted tokens and the advanced state (the contract: include/qpal.h, reference_spec_accept).
    tokens / seq / row0 as spec_draft wrote them, drawn int64 [R]; hist, n_tok, limit are updated in place, eos int64 [B] (-1: none).
    Written: out_tok int64 [B, K + 1] (entries past n_out keep what they held), n_out int32 [B], n_acc int32 [B].  One launch on the
    current stream; the host reads nothing."""
    torch = _torch()
    from . import _native
    who, QpalError = "spec_accept", _native.QpalError
    B, dev, st = _state(who, hist, n_tok, limit)
    if out_tok.dim() != 2 or not 1 <= out_tok.shape[1] <= MAX_DRAFT + 1:
        raise QpalError(f"{who}: out_tok must be int64 [{B}, K + 1] with K in 0 .. {MAX_DRAFT}")
    K = out_tok.shape[1] - 1
    if tokens.dim() != 1 or not B <= tokens.shape[0] <= MAX_ROWS:
        raise QpalError(f"{who}: tokens must be int64 [R] with {B} <= R <= {MAX_ROWS}")
    R = tokens.shape[0]
    ins = [_arr(tokens, "tokens", torch.int64, (R,), dev, who), _arr(drawn, "drawn", torch.int64, (R,), dev, who),
           _arr(seq, "seq", torch.int32, (B,), dev, who), _arr(row0, "row0", torch.int32, (B + 1,), dev, who)]
    eos_p = _arr(eos, "eos", torch.int64, (B,), dev, who)
    outs = [_arr(out_tok, "out_tok", torch.int64, (B, K + 1), dev, who), _arr(n_out, "n_out", torch.int32, (B,), dev, who),
            _arr(n_acc, "n_acc", torch.int32, (B,), dev, who)]
    if not hist.is_cuda:
        raise QpalError(f"{who}: the state must live on a GPU, got {dev}")
    with torch.cuda.device(dev):
        rc = _native.lib().qpal_spec_accept(*ins, hist.data_ptr(), hist.shape[1], *st, eos_p, B, K, R, *outs,
                                            torch.cuda.current_stream(dev).cuda_stream)
    _native.check(rc, "qpal_spec_accept")
