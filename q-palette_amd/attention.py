"""Decode attention of B concurrent sequences (C-ABI ``qpal_attn_rope_decode_batch``, csrc/attn_batch.hip).

One launch per layer and step: rotary embedding of every sequence's new q and k, k and v appended to that sequence's static
KV cache at ``pos[b]``, and attention over its positions ``0 .. pos[b]``.  A sequence whose position lies outside the cache
(``pos[b] = -1`` for a free slot, for example) is inactive: its cache and its output row are left as they were.

    ws = attention_workspace(B, nq, nkv, hd, max_len, device)      # once, shared by every layer
    out = decode_attention(q, k, v, kcache, vcache, pos, inv_freq, ws=ws)

Prompt prefill of ONE sequence (``qpal_attn_rope_prefill``, csrc/attn_prefill.hip): T <= 128 new tokens at positions ``pos0 ..
pos0 + T - 1`` in one launch, appended to that sequence's cache, every row attending causally to everything before it.

    ws = prefill_workspace(128, nq, nkv, hd, max_len, device)      # once, shared by every layer and every shorter chunk
    out = prefill_attention(q, k, v, kcache[b], vcache[b], pos0, inv_freq, ws=ws)

Both take the caches in one of two element formats and dispatch on their dtype: ``torch.float16``, or ``torch.float8_e4m3fn`` (OCP
e4m3, one byte per element, no scales: ``qpal_attn_rope_decode_batch_kv8`` / ``qpal_attn_rope_prefill_kv8``).  A
new row is stored as ``h.float().clamp(-448, 448).to(torch.float8_e4m3fn)`` of the fp16 row ``h`` the fp16 path writes and takes
part in its own launch at that stored value; stored bytes are converted exactly to fp16.  The workspaces serve both formats.

Paged caches (``qpal_attn_rope_decode_batch_paged`` / ``qpal_attn_rope_prefill_paged``): per-layer pools
``[num_pages, nkv, page_size, hd]`` and one int32 block table ``[B, max_pages]`` (``paging.PagedKVCache`` owns both); position n of
sequence b lives in page ``block_table[b, n // page_size]``.  ``max_pages * page_size`` takes the place of max_len everywhere,
the workspaces of that max_len serve the paged launches, and the result is bit for bit the contiguous launch's on the gathered cache.

    out = paged_decode_attention(q, k, v, kpool, vpool, block_table, pos, inv_freq, ws=ws)
    out = paged_prefill_attention(q, k, v, kpool, vpool, block_table[b], pos0, inv_freq, ws=ws)

Slots of a paged cache that share the pages of a common prefix (``PagedKVCache.fork``) read it once per group
(``qpal_attn_rope_decode_batch_shared``, csrc/attn_prefix.hip):

    ws = shared_prefix_workspace(B, cache.prefix.G, nq, nkv, hd, max_len, device)
    out = shared_prefix_decode_attention(q, k, v, kpool, vpool, block_table, pos, inv_freq, cache.prefix, ws=ws)

Ragged prefill (``qpal_attn_rope_prefill_ragged`` / ``_paged``, csrc/attn_ragged.hip): up to 128 rows of SEVERAL
sequences in one launch — prompt chunks and decode tokens side by side — cut into segments that three device tensors describe.

    ws = ragged_workspace(128, S, nq, nkv, hd, max_len, device)
    out = ragged_prefill_attention(q, k, v, kcache, vcache, seq, row0, pos0, inv_freq, ws=ws)
    out = paged_ragged_prefill_attention(q, k, v, kpool, vpool, block_table, seq, row0, pos0, inv_freq, ws=ws)

Sliding window (``qpal_attn_rope_decode_batch_window`` / ``_prefill_window`` / ``_prefill_ragged_window``): every launch
above except the shared-prefix one takes ``window=W``: the row at position p attends to keys ``window_floor(p, W) .. p``, W keys
with its own (Hugging Face's ``sliding_window``); ``None`` is no window.  Rotary embedding, append, the inactive and fit rules and
the stored bytes do not change; nothing below the floor is read, so those rows may hold anything and a paged cache may give their
pages back (``PagedKVCache.trim(slot, window_floor(pos, W))``).  ``W >= max_len`` is bit for bit the launch without a window.  The
workspaces above serve the windowed launches as they are.

Score modifiers (``qpal_attn_rope_decode_batch_score`` / ``_prefill_score`` / ``_prefill_ragged_score``): the same
launches take ``softcap=c`` (a finite float > 0: every scaled score s becomes c * tanh(s / c) in front of the mask and the softmax,
Gemma-2's ``attn_logit_softcapping``) and ``sinks=t`` (fp32 [nq] on the cache's device: one learned logit per query head that joins
the softmax denominator and nothing else, gpt-oss's sinks; read on the device at every launch).  ``None`` for both is the launch
as it was, bit for bit; ``sinks`` of -inf is bit for bit the launch without sinks.  With or without ``window``; not on the
shared-prefix launch.  Nothing else changes: stored bytes, rules and workspaces are the plain launches'.
"""
import math

import torch

from . import _native
from ._native import QpalError


def _window(window, who):
    """the window argument of a launch: None, or an int >= 1"""
    if window is None:
        return None
    if isinstance(window, bool) or not isinstance(window, int) or window < 1:
        raise QpalError(f"{who}: window must be None or an int >= 1, got {window!r}")
    return window


def _score_mods(softcap, sinks, who):
    """the softcap / sinks arguments of a launch: (None, None), or (softcap as a float or None, sinks or None); the tensor's shape
    and device are checked by _score_args, where nq is known"""
    if softcap is not None:
        if isinstance(softcap, bool) or not isinstance(softcap, (int, float)) or not math.isfinite(softcap) or not softcap > 0:
            raise QpalError(f"{who}: softcap must be None or a finite float > 0, got {softcap!r}")
        softcap = float(softcap)
        if not math.isfinite(torch.tensor(softcap, dtype=torch.float32).item()):
            raise QpalError(f"{who}: softcap must be finite in fp32, got {softcap!r}")
    if sinks is not None and not isinstance(sinks, torch.Tensor):
        raise QpalError(f"{who}: sinks must be None or an fp32 [nq] tensor, got {type(sinks).__name__}")
    return softcap, sinks


def _score_args(who, mods, nq, dev):
    """the two arguments of a _score entry point behind window: softcap (0: none) and the sinks' address (None: none)"""
    softcap, sinks = mods
    if sinks is not None:
        if sinks.dtype != torch.float32 or sinks.shape != (nq,) or sinks.device != dev or not sinks.is_contiguous():
            raise QpalError(f"{who}: sinks must be a contiguous float32 [{nq}] tensor on {dev}, got {sinks.dtype} "
                            f"{list(sinks.shape)} on {sinks.device}")
        if sinks.data_ptr() % 4:
            raise QpalError(f"{who}: sinks must be 4-byte aligned")
    return (0.0 if softcap is None else softcap, None if sinks is None else sinks.data_ptr())


def window_floor(pos, window):
    """lo(pos) = max(0, pos - window + 1): the first key the row at position pos attends to under ``window`` (None: 0).  pos: an int,
    a numpy array or a torch tensor; the result has its kind.  Inactive positions (pos < 0) give 0."""
    w = _window(window, "window_floor")
    if isinstance(pos, torch.Tensor):
        return torch.zeros_like(pos) if w is None else (pos - (w - 1)).clamp(min=0)
    if isinstance(pos, int):
        return 0 if w is None else max(0, pos - w + 1)
    import numpy as np

    pos = np.asarray(pos)
    return np.zeros_like(pos) if w is None else np.maximum(pos - (w - 1), 0)


def attention_workspace(B, nq, nkv, hd, max_len, device):
    """The zero-filled workspace ``decode_attention`` needs for up to B sequences and caches of up to max_len positions (same nq,
    nkv, hd), or None where no launch of that shape needs one.  Keep it across launches: the kernel leaves it as it found it."""
    return _workspace("qpal_attn_batch_ws_bytes", device, B, nq, nkv, hd, max_len)


def _workspace(sizer, device, *shape):
    """the zero-filled workspace of the launches whose bytes `sizer` gives for `shape`, or None where none of them needs one"""
    n = getattr(_native.lib(), sizer)(*(int(x) for x in shape))
    return torch.zeros((n + 3) // 4, dtype=torch.float32, device=device) if n > 0 else None


_CACHE_ENTRY = {torch.float16: "", torch.float8_e4m3fn: "_kv8"}  # cache dtype -> suffix of the C entry point


def kv_cache_bytes(B, nkv, max_len, hd, dtype=torch.float16):
    """Bytes of ONE cache tensor [B, nkv, max_len, hd] (k or v of one layer) in the element format `dtype`."""
    if dtype not in _CACHE_ENTRY:
        raise QpalError(f"kv_cache_bytes: a KV cache is torch.float16 or torch.float8_e4m3fn, got {dtype}")
    return int(B) * int(nkv) * int(max_len) * int(hd) * torch.empty(0, dtype=dtype).element_size()


def _cache_dtype(kcache, vcache, who):
    if kcache.dtype != vcache.dtype:
        raise QpalError(f"{who}: kcache and vcache must share one dtype, got {kcache.dtype} and {vcache.dtype}")
    if kcache.dtype not in _CACHE_ENTRY:
        raise QpalError(f"{who}: the caches' dtype must be torch.float16 or torch.float8_e4m3fn, got {kcache.dtype}")


def _cache_entry(kcache, vcache, who):
    """the caches' common element format as the suffix of the entry point; everything the library would not check for itself"""
    _cache_dtype(kcache, vcache, who)
    for name, t in (("kcache", kcache), ("vcache", vcache)):
        if not t.is_cuda or not t.is_contiguous():
            raise QpalError(f"{who}: {name} must be a contiguous device tensor, got one on {t.device}")
        if t.data_ptr() % 16:
            raise QpalError(f"{who}: {name} must be 16-byte aligned")
    return _CACHE_ENTRY[kcache.dtype]


def _rows(t, name, B, width, who):
    if t.dtype != torch.float32 or not t.is_cuda:
        raise QpalError(f"{who}: {name} must be an fp32 device tensor, got {t.dtype} on {t.device}")
    if t.dim() != 2 or t.shape[0] != B or t.shape[1] != width:
        raise QpalError(f"{who}: {name} must have shape [{B}, {width}], got {list(t.shape)}")
    if t.stride(1) != 1:
        raise QpalError(f"{who}: {name} rows must be contiguous")
    return t.stride(0) if B > 1 else width


def decode_attention(q, k, v, kcache, vcache, pos, inv_freq, scale=None, out=None, ws=None, window=None, softcap=None, sinks=None):
    """q fp32 [B, nq*hd], k / v fp32 [B, nkv*hd] (rows may be strided: column slices of one q|k|v output with a common row
    stride); kcache / vcache [B, nkv, max_len, hd] contiguous, 16-byte aligned, updated in place at row pos[b]; pos int64
    [B] on the device; inv_freq fp32 [hd/2].  Returns out fp16 [B, nq*hd] (``out`` if given: rows of an inactive sequence keep
    what they held).  scale defaults to 1/sqrt(hd).  Launches on the current stream.

    The caches' dtype selects the kernel: torch.float16 -> qpal_attn_rope_decode_batch; torch.float8_e4m3fn ->
    qpal_attn_rope_decode_batch_kv8 (the new row is stored as h.float().clamp(-448, 448).to(torch.float8_e4m3fn) of the fp16 row h
    and attended to at that value).  Caches of two different dtypes, or of any other dtype, raise QpalError before the library is
    reached.  One attention_workspace serves both formats.

    window=W (an int >= 1): sequence b attends to positions window_floor(pos[b], W) .. pos[b] only (qpal_attn_rope_decode_batch_window);
    cache rows below that floor are not read and may hold anything.  The attention_workspace of max_len serves it.

    softcap=c / sinks=t (the module's "Score modifiers", qpal_attn_rope_decode_batch_score): the capped scores, the new position's
    included, and one sink logit per query head in the denominator; the stored rows and the workspace do not change."""
    window, mods = _window(window, "decode_attention"), _score_mods(softcap, sinks, "decode_attention")
    if kcache.dim() != 4 or kcache.shape != vcache.shape:
        raise QpalError("decode_attention: kcache / vcache must both have shape [B, nkv, max_len, hd]")
    B, nkv, max_len, hd = kcache.shape
    entry = "qpal_attn_rope_decode_batch" + _cache_entry(kcache, vcache, "decode_attention")
    return _decode("decode_attention", entry, q, k, v, kcache, vcache, pos, inv_freq, scale, out, ws, B, nkv, max_len, hd, None,
                   window=window, mods=mods)


def _window_args(paged, empty, kcache, rows, max_len, scale, window):
    """the arguments of a _window entry point between inv_freq and ws: the paged arguments (`empty`: their stand-in for a contiguous
    cache, a null table), kv_fmt, the rows' shape, max_len (paged: ignored), scale, window"""
    head = empty + (_KV_FMT[kcache.dtype],) if paged is None else paged
    return head + rows + (max_len if paged is None else 0, scale, window)


def _decode(who, entry, q, k, v, kcache, vcache, pos, inv_freq, scale, out, ws, B, nkv, max_len, hd, paged, groups=None, window=None,
            mods=(None, None)):
    """the checks and the launch the decode entry points share; paged: None, or the arguments that take max_len's place; groups: None,
    or the G of a shared-prefix launch (its workspace is shared_prefix_workspace's); window: None, or the W of the _window entry
    point, which then takes `entry`'s place; mods: (softcap, sinks) — with either, the _score entry point takes it"""
    def pos_check():
        if pos.dtype != torch.int64 or pos.shape != (B,) or pos.device != kcache.device or not pos.is_contiguous():
            raise QpalError(f"{who}: pos must be a contiguous int64 [{B}] tensor on {kcache.device}")

    _, nq, ld, out, ld_out = _qkv_rows(who, q, k, v, kcache, inv_freq, out, nkv, hd, pos_check, B)
    score = None if mods[0] is None and mods[1] is None else _score_args(who, mods, nq, kcache.device)  # (before the library)
    lib = _native.lib()
    if groups is None:
        need, maker = lib.qpal_attn_batch_ws_bytes(B, nq, nkv, hd, max_len), "attention_workspace"
    else:
        need, maker = lib.qpal_attn_prefix_ws_bytes(B, groups, nq, nkv, hd, max_len), "shared_prefix_workspace"
    ws_ptr, ws_bytes = _launch_ws(who, need, ws, kcache, maker)
    scale = 1.0 / math.sqrt(hd) if scale is None else float(scale)
    if score is not None:
        entry = "qpal_attn_rope_decode_batch_score"
        shape = (_window_args(paged, (None, 0, 0, 0, 0), kcache, (B, nq, nkv, hd), max_len, scale, window or 0)
                 + score)
    elif window is None:
        shape = ((B, nq, nkv, hd, max_len) if paged is None else paged + (B, nq, nkv, hd)) + (scale,)
    else:
        entry, shape = "qpal_attn_rope_decode_batch_window", _window_args(paged, (None, 0, 0, 0, 0), kcache, (B, nq, nkv, hd), max_len, scale, window)
    with torch.cuda.device(kcache.device):
        rc = getattr(lib, entry)(
            q.data_ptr(), k.data_ptr(), v.data_ptr(), ld, kcache.data_ptr(), vcache.data_ptr(), out.data_ptr(), ld_out,
            pos.data_ptr(), inv_freq.data_ptr(), *shape,
            ws_ptr, ws_bytes, torch.cuda.current_stream(kcache.device).cuda_stream)
    _native.check(rc, entry)
    return out


def prefill_workspace(T, nq, nkv, hd, max_len, device):
    """The zero-filled workspace ``prefill_attention`` needs for chunks of up to T rows and a cache of up to max_len positions
    (same nq, nkv, hd), or None where no launch of that shape needs one.  Keep it across launches: the kernel leaves it as it
    found it."""
    return _workspace("qpal_attn_prefill_ws_bytes", device, T, nq, nkv, hd, max_len)


def prefill_attention(q, k, v, kcache, vcache, pos0, inv_freq, scale=None, out=None, ws=None, window=None, softcap=None, sinks=None):
    """q fp32 [T, nq*hd], k / v fp32 [T, nkv*hd], 1 <= T <= 128: row t is the token at position pos0 + t (rows may be strided:
    column slices of one q|k|v output with a common row stride); kcache / vcache [nkv, max_len, hd] of ONE sequence,
    contiguous, 16-byte aligned (``kcache[b]`` of the batched layout), updated in place at rows pos0 .. pos0 + T - 1; pos0 int64
    [1] on the device; inv_freq fp32 [hd/2].  Returns out fp16 [T, nq*hd] (``out`` if given): row t attends to positions 0 ..
    pos0 + t.  pos0 < 0 or pos0 + T > max_len: nothing is written, neither cache nor out.  scale defaults to 1/sqrt(hd).
    Launches on the current stream.

    The caches' dtype selects the kernel: torch.float16 -> qpal_attn_rope_prefill; torch.float8_e4m3fn -> qpal_attn_rope_prefill_kv8
    (new rows are stored as h.float().clamp(-448, 448).to(torch.float8_e4m3fn) of the fp16 rows h and attended to at that value: the
    cache ends up byte for byte as decode_attention would have filled it token by token).  Caches of two different dtypes, or of any
    other dtype, raise QpalError before the library is reached.  One prefill_workspace serves both formats.

    window=W (an int >= 1): row t attends to positions window_floor(pos0 + t, W) .. pos0 + t only (qpal_attn_rope_prefill_window); the
    cache ends up byte for byte as without a window, rows below window_floor(pos0, W) are not read and may hold anything.  The
    prefill_workspace of max_len serves it.

    softcap=c / sinks=t (the module's "Score modifiers", qpal_attn_rope_prefill_score): every row's scores capped, one sink logit
    per query head in every row's denominator; the cache ends up byte for byte as without them."""
    who = "prefill_attention"
    window, mods = _window(window, who), _score_mods(softcap, sinks, who)
    if kcache.dim() != 3 or kcache.shape != vcache.shape:
        raise QpalError(f"{who}: kcache / vcache must both have shape [nkv, max_len, hd]")
    nkv, max_len, hd = kcache.shape
    entry = "qpal_attn_rope_prefill" + _cache_entry(kcache, vcache, who)
    return _prefill(who, entry, q, k, v, kcache, vcache, pos0, inv_freq, scale, out, ws, nkv, max_len, hd, None, window=window,
                    mods=mods)


def _qkv_rows(who, q, k, v, kcache, inv_freq, out, nkv, hd, pos_check=None, B=None):
    """the checks of q / k / v / inv_freq / out every attention launch shares — B: the rows of a decode launch, None: the 1 .. 128
    rows of a prefill launch — with the launch's own position check, where it has one, in its place among them; returns (T, nq,
    ld_qkv, out, ld_out)"""
    if B is not None:
        if q.dim() != 2 or q.shape[0] != B or q.shape[1] % hd:
            raise QpalError(f"{who}: q must have shape [{B}, nq*{hd}], got {list(q.shape)}")
    elif q.dim() != 2 or not 1 <= q.shape[0] <= 128 or q.shape[1] % hd:
        raise QpalError(f"{who}: q must have shape [T, nq*{hd}] with 1 <= T <= 128, got {list(q.shape)}")
    T, nq = q.shape[0], q.shape[1] // hd
    ld = _rows(q, "q", T, nq * hd, who)
    for name, t in (("k", k), ("v", v)):
        if _rows(t, name, T, nkv * hd, who) != ld and T > 1:
            raise QpalError(f"{who}: q, k and v must share one row stride")
    if pos_check is not None:
        pos_check()
    if inv_freq.dtype != torch.float32 or inv_freq.numel() != hd // 2 or inv_freq.device != kcache.device or not inv_freq.is_contiguous():
        raise QpalError(f"{who}: inv_freq must be a contiguous fp32 [{hd // 2}] tensor on {kcache.device}")
    if any(t.device != kcache.device for t in (q, k, v)):
        raise QpalError(f"{who}: every tensor must be on the caches' device")
    if out is None:
        out = torch.empty(T, nq * hd, dtype=torch.float16, device=kcache.device)
    elif out.dtype != torch.float16 or out.dim() != 2 or out.shape != (T, nq * hd) or out.stride(1) != 1 or out.device != kcache.device:
        raise QpalError(f"{who}: out must be fp16 [{T}, {nq * hd}] with contiguous rows on {kcache.device}")
    return T, nq, ld, out, out.stride(0) if T > 1 else nq * hd


def _launch_ws(who, need, ws, kcache, maker):
    """(pointer, bytes) of the workspace a launch that needs `need` bytes is given"""
    if need <= 0:
        return None, 0
    if ws is None:
        raise QpalError(f"{who}: this shape needs a workspace ({maker}(...))")
    if ws.device != kcache.device or ws.numel() * ws.element_size() < need or not ws.is_contiguous():
        raise QpalError(f"{who}: ws must be a contiguous device buffer of >= {need} bytes on {kcache.device}")
    return ws.data_ptr(), ws.numel() * ws.element_size()


def _prefill(who, entry, q, k, v, kcache, vcache, pos0, inv_freq, scale, out, ws, nkv, max_len, hd, paged, window=None,
             mods=(None, None)):
    """the checks and the launch both prefill entry points share; paged: None, or the arguments that take max_len's place; window:
    None, or the W of the _window entry point, which then takes `entry`'s place; mods: (softcap, sinks) — with either, the _score
    entry point takes it"""
    def pos_check():
        if pos0.dtype != torch.int64 or pos0.numel() != 1 or pos0.device != kcache.device:
            raise QpalError(f"{who}: pos0 must be an int64 tensor of one element on {kcache.device}")

    T, nq, ld, out, ld_out = _qkv_rows(who, q, k, v, kcache, inv_freq, out, nkv, hd, pos_check)
    score = None if mods[0] is None and mods[1] is None else _score_args(who, mods, nq, kcache.device)  # (before the library)
    lib = _native.lib()
    ws_ptr, ws_bytes = _launch_ws(who, lib.qpal_attn_prefill_ws_bytes(T, nq, nkv, hd, max_len), ws, kcache, "prefill_workspace")
    scale = 1.0 / math.sqrt(hd) if scale is None else float(scale)
    if score is not None:
        entry = "qpal_attn_rope_prefill_score"
        shape = (_window_args(paged, (None, 0, 0, 0), kcache, (T, nq, nkv, hd), max_len, scale, window or 0)
                 + score)
    elif window is None:
        shape = ((T, nq, nkv, hd, max_len) if paged is None else paged + (T, nq, nkv, hd)) + (scale,)
    else:
        entry, shape = "qpal_attn_rope_prefill_window", _window_args(paged, (None, 0, 0, 0), kcache, (T, nq, nkv, hd), max_len, scale, window)
    with torch.cuda.device(kcache.device):
        rc = getattr(lib, entry)(
            q.data_ptr(), k.data_ptr(), v.data_ptr(), ld, kcache.data_ptr(), vcache.data_ptr(), out.data_ptr(), ld_out,
            pos0.data_ptr(), inv_freq.data_ptr(), *shape,
            ws_ptr, ws_bytes, torch.cuda.current_stream(kcache.device).cuda_stream)
    _native.check(rc, entry)
    return out


PAGE_SIZES = (16, 32, 64, 128, 256)
_KV_FMT = {torch.float16: 0, torch.float8_e4m3fn: 1}  # pool dtype -> kv_fmt of the paged entry points


def _pools(kpool, vpool, table, who):
    """the checks of the pools and the block table the library would not make for itself; returns (num_pages, nkv, page_size, hd)"""
    if kpool.dim() != 4 or kpool.shape != vpool.shape:
        raise QpalError(f"{who}: kpool / vpool must both have shape [num_pages, nkv, page_size, hd]")
    _cache_dtype(kpool, vpool, who)
    num_pages, nkv, page_size, hd = kpool.shape
    if page_size not in PAGE_SIZES:
        raise QpalError(f"{who}: page_size must be one of {PAGE_SIZES}, got {page_size}")
    if table.dtype != torch.int32:
        raise QpalError(f"{who}: the block table must be int32, got {table.dtype}")
    if table.device != kpool.device:
        raise QpalError(f"{who}: the block table must be on the pools' device {kpool.device}, got {table.device}")
    if table.stride(-1) != 1:
        raise QpalError(f"{who}: the block table's rows must be contiguous")
    _cache_entry(kpool, vpool, who)
    return num_pages, nkv, page_size, hd


def _pools_2d(kpool, vpool, block_table, who):
    """_pools, then the checks of a block table [B, max_pages]; returns (B, nkv, max_len, hd, the launch arguments that take max_len's
    place)"""
    num_pages, nkv, page_size, hd = _pools(kpool, vpool, block_table, who)
    if block_table.dim() != 2 or block_table.shape[1] < 1:
        raise QpalError(f"{who}: block_table must have shape [B, max_pages >= 1], got {list(block_table.shape)}")
    B, max_pages = block_table.shape
    ld_table = block_table.stride(0) if B > 1 else max_pages
    if ld_table < max_pages:
        raise QpalError(f"{who}: the block table's row stride must be at least max_pages")
    return B, nkv, max_pages * page_size, hd, (block_table.data_ptr(), ld_table, num_pages, page_size, max_pages, _KV_FMT[kpool.dtype])


def paged_decode_attention(q, k, v, kpool, vpool, block_table, pos, inv_freq, scale=None, out=None, ws=None, window=None, softcap=None,
                           sinks=None):
    """decode_attention on a paged cache: kpool / vpool [num_pages, nkv, page_size, hd] (fp16 or float8_e4m3fn, contiguous, 16-byte
    aligned, page_size in {16, 32, 64, 128, 256}), block_table int32 [B, max_pages] on the device with contiguous rows (a row
    stride >= max_pages): entry j of row b is the page of positions j * page_size .. of sequence b.  Everything else, and every
    rule, is decode_attention's with max_len = max_pages * page_size (ws: attention_workspace of that max_len); the result is bit
    for bit that launch's on the gathered cache.  Only entries that cover positions 0 .. pos[b] are read.  An entry in use outside
    [0, num_pages) (an unreserved -1): reads go to page 0, the new row is dropped, that sequence's out row is unspecified.

    window=W: decode_attention's window; only entries that cover window_floor(pos[b], W) .. pos[b] are read, so the entries of pages
    wholly below the floor may be -1 (PagedKVCache.trim).  softcap / sinks: decode_attention's."""
    who = "paged_decode_attention"
    window, mods = _window(window, who), _score_mods(softcap, sinks, who)
    B, nkv, max_len, hd, paged = _pools_2d(kpool, vpool, block_table, who)
    return _decode(who, "qpal_attn_rope_decode_batch_paged", q, k, v, kpool, vpool, pos, inv_freq, scale, out, ws, B, nkv, max_len, hd,
                   paged, window=window, mods=mods)


MAX_GROUPS = 16  # groups of one shared-prefix launch


def reference_shared_rows(row_group, grp_slot, grp_len, pos, page_size, max_len):
    """The membership rule of the shared-prefix launch (csrc/attn_prefix.h: shared_prefix_len) restated in numpy.  row_group [B],
    grp_slot / grp_len [G], pos [B] as integer arrays.  Returns (group, length) as int64 [B]: slot b is served as a member of
    group[b] with length[b] > 0 shared positions, or group[b] = -1 and length[b] = 0 where it is an ordinary slot."""
    import numpy as np

    row_group, pos = np.asarray(row_group, dtype=np.int64).reshape(-1), np.asarray(pos, dtype=np.int64).reshape(-1)
    grp_slot, grp_len = np.asarray(grp_slot, dtype=np.int64).reshape(-1), np.asarray(grp_len, dtype=np.int64).reshape(-1)
    B, G = row_group.shape[0], grp_slot.shape[0]
    in_range = (row_group >= 0) & (row_group < G)
    g = np.where(in_range, row_group, 0)
    gs, gl = (grp_slot[g], grp_len[g]) if G else (np.full(B, -1), np.zeros(B, dtype=np.int64))
    member = in_range & (gs >= 0) & (gs < B) & (gl > 0) & (gl % int(page_size) == 0) & (gl <= pos) & (pos >= 0) & (pos < int(max_len))
    return np.where(member, row_group, -1), np.where(member, gl, 0)


def _prefix_tensors(prefix, B, dev, who):
    """the checks of the three tensors that describe sharing; returns the launch arguments behind the paged ones"""
    rg, gs, gl = (getattr(prefix, n, None) for n in ("row_group", "grp_slot", "grp_len"))
    if any(not isinstance(t, torch.Tensor) for t in (rg, gs, gl)):
        raise QpalError(f"{who}: prefix must carry the tensors row_group, grp_slot and grp_len (paging.SharedPrefix)")
    for name, t in (("row_group", rg), ("grp_slot", gs), ("grp_len", gl)):
        if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
            raise QpalError(f"{who}: {name} must be a contiguous int32 vector, got {t.dtype} {list(t.shape)}")
        if t.device != dev:
            raise QpalError(f"{who}: {name} must be on the pools' device {dev}, got {t.device}")
    G = gs.shape[0]
    if rg.shape[0] != B:
        raise QpalError(f"{who}: row_group must have shape [{B}], got {list(rg.shape)}")
    if not 1 <= G <= MAX_GROUPS or gl.shape[0] != G:
        raise QpalError(f"{who}: grp_slot and grp_len must both have shape [G] with 1 <= G <= {MAX_GROUPS}, got {list(gs.shape)} and "
                        f"{list(gl.shape)}")
    return (rg.data_ptr(), gs.data_ptr(), gl.data_ptr(), G), G


def shared_prefix_workspace(B, G, nq, nkv, hd, max_len, device):
    """The zero-filled workspace ``shared_prefix_decode_attention`` needs for up to B slots in up to G groups on a paged cache of
    max_len = max_pages * page_size positions (same nq, nkv, hd).  It contains the plain launch's workspace; keep it across
    launches and layers: both launches leave their tickets at zero."""
    ws = _workspace("qpal_attn_prefix_ws_bytes", device, B, G, nq, nkv, hd, max_len)
    if ws is None:
        raise QpalError(f"shared_prefix_workspace: no shared-prefix launch of shape B={B}, G={G}, nq={nq}, nkv={nkv}, hd={hd}, "
                        f"max_len={max_len}")
    return ws


def shared_prefix_decode_attention(q, k, v, kpool, vpool, block_table, pos, inv_freq, prefix, scale=None, out=None, ws=None,
                                   window=None, softcap=None, sinks=None):
    """paged_decode_attention for slots that share the pages of a common prefix (``qpal_attn_rope_decode_batch_shared``, DESIGN.md
    §26).  prefix: a paging.SharedPrefix (``cache.prefix``) — row_group int32 [B], grp_slot / grp_len int32 [G] on the pools'
    device, read by the launches and never by the host.  A slot that reference_shared_rows() makes a member reads its group's first
    grp_len positions through table row grp_slot, once per group, and the rest through its own row; every other slot, the appended
    rows and the pools are bit for bit paged_decode_attention's.  Two launches on the current stream.  ws:
    shared_prefix_workspace(B, G, ...), always needed.  window: anything but None raises QpalError — the shared-prefix launches have
    no window.  softcap / sinks: the same — no score modifiers there either."""
    who = "shared_prefix_decode_attention"
    if window is not None:
        raise QpalError(f"{who}: no sliding window in the shared-prefix launches (window must be None)")
    if softcap is not None or sinks is not None:
        raise QpalError(f"{who}: no soft cap and no sinks in the shared-prefix launches (softcap and sinks must be None)")
    if block_table.dim() != 2:
        raise QpalError(f"{who}: block_table must have shape [B, max_pages >= 1], got {list(block_table.shape)}")
    tensors, G = _prefix_tensors(prefix, block_table.shape[0], kpool.device, who)  # (first: these checks need no device)
    B, nkv, max_len, hd, paged = _pools_2d(kpool, vpool, block_table, who)
    return _decode(who, "qpal_attn_rope_decode_batch_shared", q, k, v, kpool, vpool, pos, inv_freq, scale, out, ws, B, nkv, max_len, hd,
                   paged + tensors, groups=G)


def paged_prefill_attention(q, k, v, kpool, vpool, block_row, pos0, inv_freq, scale=None, out=None, ws=None, window=None, softcap=None,
                            sinks=None):
    """prefill_attention on a paged cache: the pools of paged_decode_attention and block_row int32 [max_pages], the block-table row
    of the ONE sequence (``block_table[b]``).  Every rule is prefill_attention's with max_len = max_pages * page_size (ws:
    prefill_workspace of that max_len); bit for bit that launch's result on the gathered cache, and the pools end up byte for byte
    as paged_decode_attention would have filled them token by token.  Only entries that cover positions 0 .. pos0 + T - 1 are read;
    the guard on entries outside [0, num_pages) is paged_decode_attention's.  window=W: prefill_attention's window; entries of pages
    wholly below window_floor(pos0, W) may be -1.  softcap / sinks: prefill_attention's."""
    who = "paged_prefill_attention"
    window, mods = _window(window, who), _score_mods(softcap, sinks, who)
    num_pages, nkv, page_size, hd = _pools(kpool, vpool, block_row, who)
    if block_row.dim() != 1 or block_row.shape[0] < 1:
        raise QpalError(f"{who}: block_row must have shape [max_pages >= 1], got {list(block_row.shape)}")
    max_pages = block_row.shape[0]
    paged = (block_row.data_ptr(), num_pages, page_size, max_pages, _KV_FMT[kpool.dtype])
    return _prefill(who, "qpal_attn_rope_prefill_paged", q, k, v, kpool, vpool, pos0, inv_freq, scale, out, ws, nkv,
                    max_pages * page_size, hd, paged, window=window, mods=mods)


def ragged_workspace(R, S, nq, nkv, hd, max_len, device):
    """The zero-filled workspace ``ragged_prefill_attention`` needs for launches of up to R rows in up to S segments on caches of
    up to max_len positions (same nq, nkv, hd), or None where no launch of that shape needs one (max_len < 512).  Keep it across
    launches: every launch leaves its tickets at zero, and they sit at a fixed offset, so launches of fewer rows, fewer segments
    or a shorter cache may share it in any order.  It is laid out for ragged launches: a prefill_workspace does not stand in."""
    return _workspace("qpal_attn_ragged_ws_bytes", device, R, S, nq, nkv, hd, max_len)


def _segments(who, seq, row0, pos0, dev):
    """the checks of the three segment descriptors; returns S"""
    if seq.dtype != torch.int32 or seq.dim() != 1 or not 1 <= seq.shape[0] <= 128 or not seq.is_contiguous():
        raise QpalError(f"{who}: seq must be a contiguous int32 [S] tensor with 1 <= S <= 128, got {seq.dtype} {list(seq.shape)}")
    S = seq.shape[0]
    if row0.dtype != torch.int32 or row0.shape != (S + 1,) or not row0.is_contiguous():
        raise QpalError(f"{who}: row0 must be a contiguous int32 [{S + 1}] tensor, got {row0.dtype} {list(row0.shape)}")
    if pos0.dtype != torch.int64 or pos0.shape != (S,) or not pos0.is_contiguous():
        raise QpalError(f"{who}: pos0 must be a contiguous int64 [{S}] tensor, got {pos0.dtype} {list(pos0.shape)}")
    for name, t in (("seq", seq), ("row0", row0), ("pos0", pos0)):
        if t.device != dev:
            raise QpalError(f"{who}: {name} must be on the caches' device {dev}, got {t.device}")
    return S


def _ragged(who, entry, q, k, v, kcache, vcache, seq, row0, pos0, S, inv_freq, scale, out, ws, B, nkv, max_len, hd, head, tail,
            window=None, mods=(None, None)):
    """the checks (behind _segments, which gave S) and the launch both ragged entry points share; head / tail: the arguments in
    front of and behind (R, S, B, nq, nkv, hd); window: None, or the W of the _window entry point, which then takes `entry`'s place
    (tail empty: a paged launch, head its paged arguments); mods: (softcap, sinks) — with either, the _score entry point takes it"""
    R, nq, ld, out, ld_out = _qkv_rows(who, q, k, v, kcache, inv_freq, out, nkv, hd)
    score = None if mods[0] is None and mods[1] is None else _score_args(who, mods, nq, kcache.device)  # (before the library)
    lib = _native.lib()
    ws_ptr, ws_bytes = _launch_ws(who, lib.qpal_attn_ragged_ws_bytes(R, S, nq, nkv, hd, max_len), ws, kcache, "ragged_workspace")
    scale = 1.0 / math.sqrt(hd) if scale is None else float(scale)
    if score is not None:
        entry = "qpal_attn_rope_prefill_ragged_score"
        shape = (_window_args(head if not tail else None, (None, 0, 0, 0, 0), kcache, (R, S, B, nq, nkv, hd), max_len, scale, window or 0)
                 + score)
    elif window is None:
        shape = tuple(head) + (R, S, B, nq, nkv, hd) + tuple(tail) + (scale,)
    else:
        entry = "qpal_attn_rope_prefill_ragged_window"
        shape = _window_args(head if not tail else None, (None, 0, 0, 0, 0), kcache, (R, S, B, nq, nkv, hd), max_len, scale, window)
    with torch.cuda.device(kcache.device):
        rc = getattr(lib, entry)(
            q.data_ptr(), k.data_ptr(), v.data_ptr(), ld, kcache.data_ptr(), vcache.data_ptr(), out.data_ptr(), ld_out,
            seq.data_ptr(), row0.data_ptr(), pos0.data_ptr(), inv_freq.data_ptr(), *shape,
            ws_ptr, ws_bytes, torch.cuda.current_stream(kcache.device).cuda_stream)
    _native.check(rc, entry)
    return out


def ragged_prefill_attention(q, k, v, kcache, vcache, seq, row0, pos0, inv_freq, scale=None, out=None, ws=None, window=None,
                             softcap=None, sinks=None):
    """prefill_attention for rows of SEVERAL sequences in one launch (``qpal_attn_rope_prefill_ragged``).  q fp32 [R,
    nq*hd], k / v fp32 [R, nkv*hd], 1 <= R <= 128 (strided rows as for prefill_attention); kcache / vcache [B, nkv, max_len, hd],
    fp16 or float8_e4m3fn, contiguous, 16-byte aligned.  The rows are cut into S <= 128 segments described ON THE DEVICE (never read
    by the host: a captured launch can be replayed while they change): seq int32 [S], row0 int32 [S + 1] (cumulative, row0[0] = 0),
    pos0 int64 [S] — segment s is rows row0[s] .. row0[s + 1] - 1, the tokens of sequence seq[s] at positions pos0[s] ...  Per
    segment the launch does what prefill_attention does for those rows on kcache[seq[s]]: rotary embedding, append, causal
    attention over that sequence only.  A decode token is a segment of one row.

    A segment with no rows, row0[s + 1] > R, seq[s] outside [0, B), pos0[s] < 0 or pos0[s] + rows > max_len is inactive: no cache
    byte and no out byte is written for it; out rows of no active segment keep what they held.  Two active segments naming one
    sequence: the caller's error, that sequence's result is unspecified.  ws: ragged_workspace(R, S, ...).

    window=W: per segment prefill_attention's window (qpal_attn_rope_prefill_ragged_window): bit for bit the one-sequence windowed
    launch wherever the unwindowed pair is; rows below window_floor(pos0[s], W) of a segment's sequence are not read.

    softcap=c / sinks=t (qpal_attn_rope_prefill_ragged_score): per segment prefill_attention's, bit for bit that launch's."""
    who = "ragged_prefill_attention"
    window, mods = _window(window, who), _score_mods(softcap, sinks, who)
    if kcache.dim() != 4 or kcache.shape != vcache.shape:
        raise QpalError(f"{who}: kcache / vcache must both have shape [B, nkv, max_len, hd]")
    B, nkv, max_len, hd = kcache.shape
    S = _segments(who, seq, row0, pos0, kcache.device)  # (first: these checks need no device)
    _cache_entry(kcache, vcache, who)
    return _ragged(who, "qpal_attn_rope_prefill_ragged", q, k, v, kcache, vcache, seq, row0, pos0, S, inv_freq, scale, out, ws, B,
                   nkv, max_len, hd, (_KV_FMT[kcache.dtype],), (max_len,), window=window, mods=mods)


def paged_ragged_prefill_attention(q, k, v, kpool, vpool, block_table, seq, row0, pos0, inv_freq, scale=None, out=None, ws=None,
                                   window=None, softcap=None, sinks=None):
    """ragged_prefill_attention on a paged cache (``qpal_attn_rope_prefill_ragged_paged``): the pools and the block table int32 [B,
    max_pages] of paged_decode_attention; segment s uses row seq[s] of the table.  Every rule is ragged_prefill_attention's with
    max_len = max_pages * page_size (ws: ragged_workspace of that max_len); bit for bit that launch's result on the gathered cache.
    Only entries that cover positions 0 .. pos0[s] + rows - 1 of an active segment are read; the guard on entries outside [0,
    num_pages) is paged_decode_attention's.  window=W: ragged_prefill_attention's window; entries of pages wholly below a segment's
    window_floor(pos0[s], W) may be -1.  softcap / sinks: ragged_prefill_attention's."""
    who = "paged_ragged_prefill_attention"
    window, mods = _window(window, who), _score_mods(softcap, sinks, who)
    S = _segments(who, seq, row0, pos0, kpool.device)
    B, nkv, max_len, hd, head = _pools_2d(kpool, vpool, block_table, who)
    return _ragged(who, "qpal_attn_rope_prefill_ragged_paged", q, k, v, kpool, vpool, seq, row0, pos0, S, inv_freq, scale, out, ws, B,
                   nkv, max_len, hd, head, (), window=window, mods=mods)
