"""Sampling the next token on the GPU: the batched lm_head (C-ABI ``qpal_lm_head_logits``, csrc/lm_head_batch.hip) and the
temperature / top-k / top-p / seeded draw (``qpal_sample``, csrc/sample.hip), one launch each for up to 128 rows.

    smp = Sampler(B, vocab, device, temperature=0.6, top_k=5, seed=1234)   # per-slot parameters on the device
    smp.set(3, temperature=0.8, top_k=0, top_p=0.95, seed=7)               # one slot (a new request)
    lm_head_logits(h32, norm.weight, norm.eps, lm_head, out=smp.logits)
    tok = sample(smp.logits, smp, ctr)                                     # ctr int64 [B]: the position; < 0: row inactive

``decoder.DecodeStep(..., sampler=smp)`` and ``decoder.Prefill(..., sampler=smp)`` end in these two launches.

    lp = token_logprobs(smp.logits, tok)      # fp32 [B]: log softmax(logits)[tok], one launch (``qpal_token_logprob``, csrc/logprob.hip)

``Sampler(..., logprobs=True)`` makes that the third launch of the tail (``smp.logprob``); ``decoder.Score`` runs it on every row of
a prompt.  ``reference_logprob`` is its contract in numpy fp64.

    ids, lp = top_logprobs(smp.logits, 5)     # int32 / fp32 [B, 5]: the 5 likeliest tokens per row, one launch (``qpal_top_logprob``)

``Sampler(..., top_logprobs=n)`` makes that one more launch of the tail (``smp.top_id``, ``smp.top_logprob``), ``decoder.Score(...,
top_logprobs=n)`` runs it on every row; ``reference_top_logprobs`` is its contract.

``Sampler(..., min_p=0.05)`` (or top_a=, typical_p=, or truncation=True) adds the three truncation filters: the draw is then
``qpal_sample_trunc``, still one launch; ``truncation_mask`` is the set it keeps.

The draw is specified exactly (include/qpal.h); ``reference_draw`` restates it in numpy fp64 with its own Philox.
It is the specification the tests hold the kernel to: CPU only, no torch.cuda, no library call.
"""
import numpy as np

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32(counter, key):
    """Philox4x32-10.  counter: uint32 [..., 4], key: uint32 [..., 2] (broadcast against each other) -> uint32 [..., 4]"""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]  # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & _MASK]
        k = [(k[0] + np.uint64(_W0)) & _MASK, (k[1] + np.uint64(_W1)) & _MASK]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def race_scores(z, seed, ctr):
    """s[i] = z[i] - ln(-ln u_i) in fp64, u_i from Philox word i & 3 of counter (i >> 2, 0, ctr_lo, ctr_hi), key (seed_lo, seed_hi).
    ctr: an int or an int array [n] -> s [vocab] or [n, vocab]"""
    z = np.asarray(z, dtype=np.float64)
    vocab = z.shape[0]
    ctr_a = np.atleast_1d(np.asarray(ctr, dtype=np.int64)).astype(np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    groups = np.arange((vocab + 3) // 4, dtype=np.uint64)
    counter = np.zeros((ctr_a.shape[0], groups.shape[0], 4), dtype=np.uint64)
    counter[..., 0] = groups[None, :]
    counter[..., 2] = (ctr_a & _MASK)[:, None]
    counter[..., 3] = (ctr_a >> np.uint64(32))[:, None]
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    x = philox4x32(counter, key).reshape(ctr_a.shape[0], -1)[:, :vocab]
    u = ((x >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    with np.errstate(invalid="ignore"):
        s = z[None, :] - np.log(-np.log(u))
    return s[0] if np.ndim(ctr) == 0 else s


def topk_mask(l, top_k):
    """step 3 on l (fp32 values, NaN already -inf): {i : l[i] >= the k-th largest value}; top_k <= 0 or >= vocab: all"""
    top_k = int(top_k)
    if top_k <= 0 or top_k >= l.shape[0]:
        return np.ones(l.shape[0], dtype=bool)
    return l >= np.partition(l, l.shape[0] - top_k)[l.shape[0] - top_k]


def probabilities(l, temperature, kmask):
    """p (fp64) of step 4 over the set kmask; 0 outside it.  All -inf: zeros."""
    z = np.where(kmask, l.astype(np.float64) / float(temperature), -np.inf)
    zmax = z.max()
    if not np.isfinite(zmax):
        return np.zeros_like(z) if zmax < 0 else (z == zmax) / float((z == zmax).sum())
    w = np.exp(z - zmax)
    return w / w.sum()


def nucleus_mask(p, kmask, top_p):
    """step 4: {i in K : p[i] >= tau}, tau the largest value among the p's with sum{p[j] : p[j] >= tau} >= top_p"""
    top_p = float(top_p)
    if top_p >= 1.0 or top_p <= 0.0 or not p.any():
        return kmask.copy()
    vals, inv = np.unique(p[kmask], return_inverse=True)       # ascending
    mass = np.bincount(inv, weights=p[kmask], minlength=vals.shape[0])
    cum = np.cumsum(mass[::-1])                                  # mass of {p >= vals[::-1][j]}
    j = int(np.searchsorted(cum, top_p, side="left"))
    tau = vals[::-1][min(j, vals.shape[0] - 1)]
    return kmask & (p >= tau)


def truncation_mask(l, T, nmask, min_p=0.0, top_a=0.0, typical_p=1.0, fallback=True, tol_d=0.0):
    """step 4a (qpal_sample_trunc) on l (fp32 values, NaN already -inf) at temperature T > 0: R = N ∩ A ∩ B ∩ C for the
    nucleus nmask, all three judged on the one q = the tempered distribution renormalised over N.  min_p > 0: A = {w >= min(min_p,
    1)}, w = exp(z - zmax); top_a > 0: B = {w >= top_a / S}, S = sum of w over N; 0 < typical_p < 1: C = {d <= delta}, d = |(zmax -
    z) - c|, c = sum of q (zmax - z), delta the smallest value among the d's with sum{q[j] : d[j] <= delta} >= typical_p (ties at
    delta all kept).  An empty R is the one token argmax l over N, lowest id (fallback=False: the empty set, for tests that build
    inner sets).  tol_d: C = {d <= delta + tol_d}, for tests that build inner (< 0) and outer (> 0) sets.  +inf logits share the
    mass equally and have d = 0; no logit above -inf in N: N itself."""
    nmask = np.asarray(nmask, dtype=bool)
    min_p, top_a, typical_p = float(min_p), float(top_a), float(typical_p)
    on_t = 0.0 < typical_p < 1.0
    if not (min_p > 0.0 or top_a > 0.0 or on_t):
        return nmask.copy()
    z = np.where(nmask, l.astype(np.float64) / float(T), -np.inf)
    zmax = z.max()
    if zmax == -np.inf:
        return nmask.copy()
    with np.errstate(invalid="ignore"):
        gap = np.where(z == zmax, 0.0, zmax - z)  # inf - inf: a copy of a +inf maximum is at gap 0
    w = np.where(nmask, np.exp(-gap), 0.0)
    S = w.sum()
    keep = nmask.copy()
    if min_p > 0.0:
        keep &= w >= min(min_p, 1.0)
    if top_a > 0.0:
        keep &= w >= top_a / S
    if on_t:
        q = w / S
        c = float((q[w > 0] * gap[w > 0]).sum())
        d = np.abs(gap - c)
        vals, inv = np.unique(d[nmask], return_inverse=True)  # ascending
        cum = np.cumsum(np.bincount(inv, weights=q[nmask], minlength=vals.shape[0]))  # mass of {d <= vals[j]}
        j = int(np.searchsorted(cum, typical_p, side="left"))
        delta = vals[min(j, vals.shape[0] - 1)]
        keep &= d <= delta + float(tol_d)
    if fallback and not keep.any():
        keep[int(np.argmax(np.where(nmask, l, -np.inf)))] = True
    return keep


def clean_logits(logits_row):
    """fp32 logits as the kernel sees them, NaN -> -inf (a NaN logit is never kept)"""
    l = np.asarray(logits_row, dtype=np.float32).copy()
    l[np.isnan(l)] = -np.inf
    return l


def reference_draw(logits_row, temperature, top_k, top_p, seed, ctr, min_p=0.0, top_a=0.0, typical_p=1.0):
    """The contract of qpal_sample for one row, in fp64, and with min_p / top_a / typical_p that of qpal_sample_trunc (step 4a:
    truncation_mask on the nucleus).  temperature / top_p and the three are rounded to fp32 first (what the kernel is given).
    ctr: an int -> the token (None for ctr < 0: the row is inactive), or an int array of non-negative counters -> tokens."""
    if np.ndim(ctr) == 0 and int(ctr) < 0:
        return None
    l = clean_logits(logits_row)
    T, P = float(np.float32(temperature)), float(np.float32(top_p))
    scalar = np.ndim(ctr) == 0
    if not T > 0.0 or int(top_k) == 1:
        tok = int(np.argmax(l)) if np.isfinite(l.max()) or l.max() > 0 else 0
        return tok if scalar else np.full(np.shape(ctr), tok, dtype=np.int64)
    kmask = topk_mask(l, top_k)
    kept = nucleus_mask(probabilities(l, T, kmask), kmask, P)
    kept = truncation_mask(l, T, kept, float(np.float32(min_p)), float(np.float32(top_a)), float(np.float32(typical_p)))
    z = l.astype(np.float64) / T
    s = np.atleast_2d(race_scores(z, seed, ctr))
    s = np.where(kept[None, :] & (z[None, :] > -np.inf), s, -np.inf)
    tok = np.where(s.max(axis=1) > -np.inf, s.argmax(axis=1), 0).astype(np.int64)
    return int(tok[0]) if scalar else tok


def reference_logprob(logits_row, token):
    """The contract of qpal_token_logprob for one row, in fp64 on clean_logits(row): (logprob, lse, rank) as Python floats and an
    int, or None for an inactive row (token < 0 or >= vocab).  Plain softmax of the raw logits (temperature 1, no filter); rank =
    #{i : l[i] > l[token]} on the fp32 values.  No logit above -inf: (-inf, -inf, 0); +inf logits share the mass equally."""
    l = clean_logits(logits_row)
    token = int(token)
    if not 0 <= token < l.shape[0]:
        return None
    lt, lmax = float(l[token]), float(l.max())
    rank = int((l > l[token]).sum())
    if lmax == -np.inf:
        return -np.inf, -np.inf, 0
    if lmax == np.inf:
        return (-float(np.log((l == lmax).sum())) if lt == lmax else -np.inf), np.inf, rank
    lse = lmax + float(np.log(np.exp(l.astype(np.float64) - lmax).sum()))
    return (lt - lse if lt > -np.inf else -np.inf), lse, rank


def reference_top_logprobs(logits_row, n):
    """The contract of qpal_top_logprob for one row, in fp64 on clean_logits(row): (ids int32 [n], logprob float64 [n], lse).  The
    tokens by value descending (fp32 values: -0 and +0 tie; NaN is -inf), equal values by ascending id; entry j < min(n, vocab) is
    the j-th of them with reference_logprob's value for it, the rest are id -1, logprob -inf."""
    l = clean_logits(logits_row)
    n = int(n)
    order = np.argsort(-l.astype(np.float64), kind="stable")[:n]  # stable: equal values keep their ascending ids
    ids, logprob = np.full(n, -1, dtype=np.int32), np.full(n, -np.inf, dtype=np.float64)
    ids[:order.shape[0]] = order
    logprob[:order.shape[0]] = [reference_logprob(l, t)[0] for t in order]
    return ids, logprob, reference_logprob(l, 0)[1]


# ---------------------------------------------------------------------------------------------------------------- GPU side

def _torch():
    import torch
    return torch


def lm_head_logits(h32, norm_weight, eps, lm_head, out=None):
    """logits fp32 [rows, vocab] = lm_head @ fp16(fp16(RMSNorm(h32)) * norm_weight) per row; norm_weight None: weight 1, as in the
    other norm entry points; eps <= 0: no norm at all, x = fp16(h32), and norm_weight is ignored.
    h32 fp32 [rows, k] (rows may be strided), 1 <= rows <= 128, k a multiple of 512 up to 8192; lm_head fp16 [vocab, k] contiguous,
    16-byte aligned; out: fp32 [rows, >= vocab columns] with contiguous rows (columns past vocab are left alone).  Launches on the
    current stream."""
    torch = _torch()
    from . import _native
    who, QpalError = "lm_head_logits", _native.QpalError
    if h32.dtype != torch.float32 or not h32.is_cuda or h32.dim() != 2 or h32.stride(1) != 1:
        raise QpalError(f"{who}: h32 must be an fp32 device tensor [rows, k] with contiguous rows")
    rows, k = h32.shape
    if not 1 <= rows <= 128 or k % 512 or not 512 <= k <= 8192:
        raise QpalError(f"{who}: rows must be in 1 .. 128 and k a multiple of 512 up to 8192, got {list(h32.shape)}")
    if lm_head.dtype != torch.float16 or lm_head.dim() != 2 or lm_head.shape[1] != k or not lm_head.is_contiguous() or lm_head.device != h32.device:
        raise QpalError(f"{who}: lm_head must be a contiguous fp16 [vocab, {k}] tensor on {h32.device}")
    vocab = lm_head.shape[0]
    ld_h = h32.stride(0) if rows > 1 else k
    if lm_head.data_ptr() % 16 or h32.data_ptr() % 16 or ld_h % 4:
        raise QpalError(f"{who}: lm_head and h32 must be 16-byte aligned, the row stride of h32 a multiple of 4")
    w = None
    eps = float(eps) if eps > 0 else 0.0
    if norm_weight is not None and eps > 0:
        w = norm_weight
        if w.dtype != torch.float16 or w.shape != (k,) or not w.is_contiguous() or w.device != h32.device or w.data_ptr() % 8:
            raise QpalError(f"{who}: norm_weight must be a contiguous 8-byte aligned fp16 [{k}] tensor on {h32.device}")
    if out is None:
        out = torch.empty(rows, vocab, dtype=torch.float32, device=h32.device)
    elif (out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != rows or out.shape[1] < vocab or out.stride(1) != 1
          or out.device != h32.device or (rows > 1 and out.stride(0) < vocab)):
        raise QpalError(f"{who}: out must be fp32 [{rows}, >= {vocab}] with contiguous rows on {h32.device}")
    ld_out = out.stride(0) if rows > 1 else out.shape[1]
    with torch.cuda.device(h32.device):
        rc = _native.lib().qpal_lm_head_logits(h32.data_ptr(), ld_h, w.data_ptr() if w is not None else None, eps,
                                               lm_head.data_ptr(), out.data_ptr(), ld_out, rows, vocab, k,
                                               torch.cuda.current_stream(h32.device).cuda_stream)
    _native.check(rc, "qpal_lm_head_logits")
    return out


TRUNCATION = ("min_p", "top_a", "typical_p")  # the per-slot vectors of a truncating Sampler, in qpal_sample_trunc's order


def _param(t, name, dtype, rows, dev, who):
    from ._native import QpalError
    if t.dtype != dtype or t.shape != (rows,) or t.device != dev or not t.is_contiguous():
        raise QpalError(f"{who}: {name} must be a contiguous {dtype} [{rows}] tensor on {dev}")
    return t.data_ptr()


def sample(logits, params, ctr, out=None, vocab=None):
    """token int64 [rows]: one draw per row of logits fp32 [rows, >= vocab] (contiguous rows; vocab defaults to the width) with
    params.temperature / top_k / top_p / seed ([rows] device tensors: a Sampler, or a view of one) and the counter ctr int64 [rows]
    (the position; < 0: the row is inactive and out[row] keeps what it held).  params built with the truncation filters (min_p /
    top_a / typical_p are tensors, not None): ``qpal_sample_trunc`` with them; otherwise ``qpal_sample``.  Launches on the current
    stream; no host read."""
    torch = _torch()
    from . import _native
    who, QpalError = "sample", _native.QpalError
    if logits.dtype != torch.float32 or not logits.is_cuda or logits.dim() != 2 or logits.stride(1) != 1:
        raise QpalError(f"{who}: logits must be an fp32 device tensor [rows, vocab] with contiguous rows")
    rows, dev = logits.shape[0], logits.device
    vocab = logits.shape[1] if vocab is None else int(vocab)
    ld = logits.stride(0) if rows > 1 else logits.shape[1]
    if not 1 <= rows <= 128 or not 1 <= vocab <= logits.shape[1] or ld < vocab:
        raise QpalError(f"{who}: rows must be in 1 .. 128 and 1 <= vocab <= the row width, got {list(logits.shape)}, vocab {vocab}")
    ptrs = [_param(params.temperature, "temperature", torch.float32, rows, dev, who), _param(params.top_k, "top_k", torch.int32, rows, dev, who),
            _param(params.top_p, "top_p", torch.float32, rows, dev, who), _param(params.seed, "seed", torch.int64, rows, dev, who),
            _param(ctr, "ctr", torch.int64, rows, dev, who)]
    if out is None:
        out = torch.zeros(rows, dtype=torch.int64, device=dev)
    else:
        _param(out, "out", torch.int64, rows, dev, who)
    if getattr(params, "min_p", None) is None:
        with torch.cuda.device(dev):
            rc = _native.lib().qpal_sample(logits.data_ptr(), ld, rows, vocab, *ptrs, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        _native.check(rc, "qpal_sample")
        return out
    trunc = [_param(getattr(params, name), name, torch.float32, rows, dev, who) for name in TRUNCATION]
    with torch.cuda.device(dev):
        rc = _native.lib().qpal_sample_trunc(logits.data_ptr(), ld, rows, vocab, *ptrs[:3], *trunc, *ptrs[3:], out.data_ptr(),
                                             torch.cuda.current_stream(dev).cuda_stream)
    _native.check(rc, "qpal_sample_trunc")
    return out


def token_logprobs(logits, tokens, out=None, lse=None, rank=None, vocab=None, active=None):
    """logprob fp32 [rows]: log softmax(logits[row, :vocab])[tokens[row]] per row of logits fp32 [rows, >= vocab] (contiguous rows;
    vocab defaults to the width), tokens int64 [rows].  A row whose token is < 0 or >= vocab, or whose active[row] < 0 (active: an
    optional int64 [rows], a decode step's positions), is inactive: its entries of out / lse / rank keep what they held.  lse fp32
    [rows] and rank int32 [rows], where given, receive the row's log-sum-exp and #{i : l[i] > l[token]}.  Launches on the current
    stream; no host read."""
    torch = _torch()
    from . import _native
    who, QpalError = "token_logprobs", _native.QpalError
    if logits.dtype != torch.float32 or not logits.is_cuda or logits.dim() != 2 or logits.stride(1) != 1:
        raise QpalError(f"{who}: logits must be an fp32 device tensor [rows, vocab] with contiguous rows")
    rows, dev = logits.shape[0], logits.device
    vocab = logits.shape[1] if vocab is None else int(vocab)
    ld = logits.stride(0) if rows > 1 else logits.shape[1]
    if not 1 <= rows <= 128 or not 1 <= vocab <= logits.shape[1] or ld < vocab:
        raise QpalError(f"{who}: rows must be in 1 .. 128 and 1 <= vocab <= the row width, got {list(logits.shape)}, vocab {vocab}")
    tok_p = _param(tokens, "tokens", torch.int64, rows, dev, who)
    if out is None:
        out = torch.zeros(rows, dtype=torch.float32, device=dev)
    ptrs = [_param(out, "out", torch.float32, rows, dev, who),
            None if lse is None else _param(lse, "lse", torch.float32, rows, dev, who),
            None if rank is None else _param(rank, "rank", torch.int32, rows, dev, who),
            None if active is None else _param(active, "active", torch.int64, rows, dev, who)]
    with torch.cuda.device(dev):
        rc = _native.lib().qpal_token_logprob(logits.data_ptr(), ld, rows, vocab, tok_p, *ptrs, torch.cuda.current_stream(dev).cuda_stream)
    _native.check(rc, "qpal_token_logprob")
    return out


def top_logprobs(logits, n, ids=None, logprob=None, lse=None, vocab=None, active=None):
    """(ids int32 [rows, n], logprob fp32 [rows, n]): the n <= 64 likeliest tokens of every row of logits fp32 [rows, >= vocab]
    (contiguous rows; vocab defaults to the width) and their log-probabilities under the plain softmax of the row, likeliest first,
    equal values by ascending id; entries past the vocabulary are id -1, logprob -inf.  Every value is bitwise what token_logprobs
    gives for that token on the same row.  A row whose active[row] < 0 (active: an optional int64 [rows], a decode step's positions)
    keeps what its entries held.  lse fp32 [rows], where given, receives the row's log-sum-exp.  ids / logprob: contiguous [rows, n]
    tensors to write into.  Launches on the current stream (``qpal_top_logprob``, csrc/top_logprob.hip); no host read."""
    torch = _torch()
    from . import _native
    who, QpalError = "top_logprobs", _native.QpalError
    if logits.dtype != torch.float32 or not logits.is_cuda or logits.dim() != 2 or logits.stride(1) != 1:
        raise QpalError(f"{who}: logits must be an fp32 device tensor [rows, vocab] with contiguous rows")
    rows, dev, n = logits.shape[0], logits.device, int(n)
    vocab = logits.shape[1] if vocab is None else int(vocab)
    ld = logits.stride(0) if rows > 1 else logits.shape[1]
    if not 1 <= rows <= 128 or not 1 <= vocab <= logits.shape[1] or ld < vocab:
        raise QpalError(f"{who}: rows must be in 1 .. 128 and 1 <= vocab <= the row width, got {list(logits.shape)}, vocab {vocab}")
    if not 1 <= n <= 64:
        raise QpalError(f"{who}: n must be in 1 .. 64, got {n}")
    if ids is None:
        ids = torch.full((rows, n), -1, dtype=torch.int32, device=dev)
    if logprob is None:
        logprob = torch.full((rows, n), float("-inf"), dtype=torch.float32, device=dev)
    for t, name, dtype in ((ids, "ids", torch.int32), (logprob, "logprob", torch.float32)):
        if t.dtype != dtype or t.shape != (rows, n) or t.device != dev or not t.is_contiguous():
            raise QpalError(f"{who}: {name} must be a contiguous {dtype} [{rows}, {n}] tensor on {dev}")
    ptrs = [None if lse is None else _param(lse, "lse", torch.float32, rows, dev, who),
            None if active is None else _param(active, "active", torch.int64, rows, dev, who)]
    with torch.cuda.device(dev):
        rc = _native.lib().qpal_top_logprob(logits.data_ptr(), ld, rows, vocab, n, ids.data_ptr(), logprob.data_ptr(), *ptrs,
                                            torch.cuda.current_stream(dev).cuda_stream)
    _native.check(rc, "qpal_top_logprob")
    return ids, logprob


class Sampler:
    """Per-slot sampling parameters of B sequences, on the device: temperature fp32, top_k int32, top_p fp32, seed int64, each [B],
    and the logits buffer fp32 [B, vocab] the step's lm_head writes.  Scalars broadcast; sequences of B values are taken per slot.
    temperature <= 0 or top_k == 1: greedy; top_k <= 0: no top-k; top_p >= 1 or <= 0: no top-p.  A captured step reads the tensors
    when it runs: ``set`` between replays changes the next draw.  logprobs=True: the sampler also owns logprob fp32 [B], and a step
    with this sampler writes the log-probability of each token it draws there (plain softmax of the logits, whatever the filter:
    token_logprobs; one more launch); otherwise logprob is None.  top_logprobs=n (1 .. 64): the sampler also owns top_id int32 [B, n]
    and top_logprob fp32 [B, n], and a step with this sampler writes the n likeliest tokens of each row that drew and their
    log-probabilities there (top_logprobs, under the same plain softmax of the logits the draw saw; one more launch); 0 or unset:
    both are None.  min_p / top_a / typical_p (min_p <= 0, top_a <= 0, typical_p <= 0 or >= 1: that filter off): given
    a non-neutral value, or with truncation=True, the sampler also owns min_p / top_a / typical_p fp32 [B] and draws with
    ``qpal_sample_trunc``; otherwise the three are None and every launch is the plain sampler's."""

    def __init__(self, B, vocab, device, temperature=1.0, top_k=0, top_p=1.0, seed=0, logprobs=False, top_logprobs=0, min_p=0.0,
                 top_a=0.0, typical_p=1.0, truncation=False):
        torch = _torch()
        from ._native import QpalError
        if not 1 <= int(B) <= 128 or int(vocab) < 1:
            raise QpalError(f"Sampler: B must be in 1 .. 128 and vocab >= 1, got {B}, {vocab}")
        self.B, self.vocab, self.device = int(B), int(vocab), torch.device(device)

        def full(v, dtype):
            t = torch.as_tensor(v, dtype=dtype).reshape(-1)
            if t.numel() not in (1, self.B):
                raise QpalError(f"Sampler: a scalar or {self.B} values, got {t.numel()}")
            return t.expand(self.B).contiguous().to(self.device)

        self.temperature, self.top_k = full(temperature, torch.float32), full(top_k, torch.int32)
        self.top_p, self.seed = full(top_p, torch.float32), full(seed, torch.int64)
        self.logits = torch.zeros(self.B, self.vocab, dtype=torch.float32, device=self.device)
        self.logprob = torch.zeros(self.B, dtype=torch.float32, device=self.device) if logprobs else None
        n = int(top_logprobs or 0)
        if not 0 <= n <= 64:
            raise QpalError(f"Sampler: top_logprobs must be in 0 .. 64, got {top_logprobs}")
        self.top_id = torch.full((self.B, n), -1, dtype=torch.int32, device=self.device) if n else None
        self.top_logprob = torch.full((self.B, n), float("-inf"), dtype=torch.float32, device=self.device) if n else None
        given = [torch.as_tensor(v, dtype=torch.float32).reshape(-1) for v in (min_p, top_a, typical_p)]
        neutral = bool((given[0] <= 0).all()) and bool((given[1] <= 0).all()) and bool(((given[2] <= 0) | (given[2] >= 1)).all())
        if truncation or not neutral:
            self.min_p, self.top_a, self.typical_p = (full(v, torch.float32) for v in given)
        else:
            self.min_p = self.top_a = self.typical_p = None

    def set(self, slot, temperature=None, top_k=None, top_p=None, seed=None, min_p=None, top_a=None, typical_p=None):
        """write one slot's parameters (those given); min_p / top_a / typical_p only on a sampler built with them"""
        from ._native import QpalError
        if not 0 <= int(slot) < self.B:
            raise QpalError(f"Sampler.set: slot {slot} outside 0 .. {self.B - 1}")
        if self.min_p is None and not (min_p is None and top_a is None and typical_p is None):
            raise QpalError("Sampler.set: min_p / top_a / typical_p need a sampler built with them (a non-neutral value, or truncation=True)")
        for t, v in ((self.temperature, temperature), (self.top_k, top_k), (self.top_p, top_p), (self.seed, seed), (self.min_p, min_p),
                     (self.top_a, top_a), (self.typical_p, typical_p)):
            if v is not None:
                t[int(slot)] = v

    def slot(self, slot):
        """a one-row view of slot `slot` (what Prefill draws with): same storage"""
        v = object.__new__(Sampler)
        v.B, v.vocab, v.device = 1, self.vocab, self.device
        s = slice(int(slot), int(slot) + 1)
        v.temperature, v.top_k, v.top_p, v.seed, v.logits = self.temperature[s], self.top_k[s], self.top_p[s], self.seed[s], self.logits[s]
        v.logprob = None if self.logprob is None else self.logprob[s]
        v.top_id = None if self.top_id is None else self.top_id[s]
        v.top_logprob = None if self.top_logprob is None else self.top_logprob[s]
        v.min_p, v.top_a, v.typical_p = (None if self.min_p is None else getattr(self, name)[s] for name in TRUNCATION)
        return v
