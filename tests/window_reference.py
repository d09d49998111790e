"""Sliding-window attention references, on top of tests/attn_reference.py: the float64 result, the emulation and the
bound of a row with a window, the census expectation, seeded window defects, and inputs whose dynamic range lies INSIDE the window.
Used by test_window_contract.py (CPU), test_window.py and test_window_model.py (GPU); device-agnostic.

The contract: with window W >= 1 the row at position p attends to keys lo(p) .. p, lo(p) = max(0, p - W + 1).  The windowed float64
result of that row IS attn_reference.attention_fp64 on the slice K[:, lo:p + 1], V[:, lo:p + 1] with p + 1 - lo keys (sliced(), which
serves emulate() and the terms of the bound the same way).  masked() computes the same thing for many rows at once with a mask over
one shared key range — what the GPU tests call, and what carries the seeded defects; test_window_contract.py pins it to sliced().

kappa of bound(): attn_reference.KAPPA = 8 was measured at 512 keys and more.  With few keys the weight term shrinks (A and Smax are
those of a handful of keys) while the fp32 rounding of the quotient does not, so the ratio |fp32 quotient - ref| / ((u_p + 2^-23 (1 +
Smax)) A), taken in front of the output rounding, is larger.  Measured on the CPU over every windowed case the GPU tests use
(both cache formats, every head shape; elements whose weight term lies below the bound's absolute floor 2^-24 are left out — a
window of a few e4m3 values that are all zero or subnormal — the whole tolerance checks them.  Decode: every case of
test_window.py::test_decode_families_within_the_bound.  Prefill: EVERY row of every case of test_window.py::PF_CASES;
test_window_contract.py::test_emulation_sits_inside_the_windowed_bound re-measures the decode column in full and the prefill
column on the first, middle and last row of every case, where it reaches 0.79, and prints both):

  family      u_p = 0 (decode)   u_p = 2^-11 (prefill, ragged)
  peaked           1.232              1.385
  ramp_up          3.571              0.877
  ramp_down        4.201              0.891
  offset           3.221              0.842
  needle           0.000              0.820

By the §23 rule kappa is four times the worst, rounded up to a power of two, per u_p: 4 x 4.201 = 16.8 -> 32 for decode, 4 x 1.385 =
5.54 -> 8 for prefill and ragged.  The emulation stays at or below 0.77 of the whole tolerance.  The kernels' own ratios never set it."""
import math

import torch

import attn_reference as ar

U_PREFILL = 2.0 ** -11
KAPPA = {False: 32.0, True: 8.0}  # keyed by u_p > 0: decode keeps fp32 weights, prefill / ragged round them to fp16


def lo(p, W):
    """the first key of the row at position p: max(0, p - W + 1); W None: 0"""
    return 0 if W is None else max(0, int(p) - int(W) + 1)


def sliced(fn, q16, K, V, pos, W, *args, **kw):
    """fn = attn_reference.attention_fp64 or emulate, row by row on the row's own slice of the cache: the definition.  Returns the
    per-row results concatenated (attention_fp64: the triple ref, A, Smax)."""
    outs = []
    for r, p in enumerate(pos):
        l = lo(p, W)
        outs.append(fn(q16[r:r + 1], K[:, l:p + 1], V[:, l:p + 1], [p + 1 - l], *args, **kw))
    if isinstance(outs[0], tuple):
        return tuple(torch.cat(t) for t in zip(*outs))
    return torch.cat(outs)


DEFECTS = ("wide", "narrow", "tile", "first_row_lo", "last_chunk_only", "shift")


def admitted(pos, W, j0, j1, dev, mutate=None):
    """bool [R, j1 - j0]: which keys j0 .. j1 - 1 each row attends to.  mutate seeds one window defect:
      ("wide",) one key too wide: admits lo - 1; ("narrow",) one key too narrow: drops lo; ("tile", g) the lower mask at tile
      granularity: admits down to the multiple of g at or below lo; ("first_row_lo",) every row takes lo of the FIRST row;
      ("last_chunk_only", c) chunks of c keys counted from the multiple of 32 at or below the first row's lo, the lower edge
      applied in the last one only: every earlier chunk admits all of its keys from that multiple on; ("shift", s) the whole window
      moved down by s keys."""
    p = torch.as_tensor(pos, dtype=torch.long, device=dev).view(-1, 1)
    j = torch.arange(j0, j1, device=dev).view(1, -1)
    low = (p - (W - 1)).clamp(min=0) if W is not None else torch.zeros_like(p)
    kind = mutate[0] if mutate else None
    top = p
    if kind == "wide":
        low = (low - 1).clamp(min=0)
    elif kind == "narrow":
        low = torch.minimum(low + 1, p)
    elif kind == "tile":
        low = low // mutate[1] * mutate[1]
    elif kind == "first_row_lo":
        low = low[:1].expand_as(low)
    elif kind == "shift":
        low, top = (low - mutate[1]).clamp(min=0), p - mutate[1]
    elif kind == "last_chunk_only":
        base = low[0, 0] // 32 * 32
        last = base + (p.max() - base) // mutate[1] * mutate[1]  # the first key of the last chunk of the launch's keys
        return (j <= p) & ((j >= low) | ((j < last) & (j >= base)))
    elif kind is not None:
        raise ValueError(kind)
    return (j >= low) & (j <= top)


def masked(q16, K, V, pos, W, nq, nkv, hd, scale, mutate=None):
    """(ref, A, Smax) of attn_reference.attention_fp64 for rows at positions pos under window W, all rows at once: float64 over the
    keys from the lowest admitted one to the highest, the rest masked.  No cache row outside that range is touched (they may hold
    NaN).  With mutate (admitted()): ref is the defective result, A and Smax stay those of the correct computation."""
    dev, R = q16.device, q16.shape[0]
    ok = admitted(pos, W, 0, int(max(pos)) + 1, dev)
    bad = admitted(pos, W, 0, int(max(pos)) + 1, dev, mutate) if mutate else ok
    cols = (ok | bad).any(0).nonzero().view(-1)
    j0, j1 = int(cols.min()), int(cols.max()) + 1
    ok, bad = ok[:, j0:j1], bad[:, j0:j1]
    q = q16.view(R, nkv, nq // nkv, hd).float().double()
    Kd, Vd = K[:, j0:j1].float().double(), V[:, j0:j1].float().double()

    def soft(valid):
        s = (torch.einsum("rgpd,gjd->rgpj", q, Kd) * scale).masked_fill(~valid[:, None, None, :], float("-inf"))
        return torch.softmax(s, dim=-1)

    p = soft(ok)
    ref = torch.einsum("rgpj,gjd->rgpd", p, Vd).reshape(R, nq * hd)
    A = torch.einsum("rgpj,gjd->rgpd", p, Vd.abs()).reshape(R, nq * hd)
    Smax = (torch.einsum("rgpd,gjd->rgpj", q.abs(), Kd.abs()) * scale).masked_fill(~ok[:, None, None, :], 0.0).amax(-1).reshape(R, nq)
    if mutate:
        ref = torch.einsum("rgpj,gjd->rgpd", soft(bad), Vd).reshape(R, nq * hd)
    return ref, A, Smax


def bound(ref, A, Smax, u_p):
    """attn_reference.bound with this file's kappa: 2^-11 |ref| + 2^-24 + kappa (u_p + 2^-23 (1 + Smax)) A"""
    return 2.0 ** -11 * ref.abs() + 2.0 ** -24 + KAPPA[u_p > 0] * ar.weight_term(A, Smax, u_p)


def census_expected(pos, W, nq, hd, dev):
    """out[r, h, d] = #{lo <= j <= pos[r] : j = d (mod hd)} / (pos[r] + 1 - lo) as float64 [R, nq * hd] and its tolerance, one fp16 ulp
    (attn_reference.census_expected's reasoning: exact counts, one fp32 division, one fp16 rounding)"""
    n = torch.as_tensor([p + 1 for p in pos], dtype=torch.long, device=dev).view(-1, 1)
    l = torch.as_tensor([lo(p, W) for p in pos], dtype=torch.long, device=dev).view(-1, 1)
    d = torch.arange(hd, device=dev)[None, :]
    below = lambda x: (x - d + hd - 1).clamp(min=0) // hd  # noqa: E731  #{0 <= j < x : j = d (mod hd)}
    exp = ((below(n) - below(l)).double() / (n - l).double()).repeat(1, nq)
    return exp, ar.fp16_ulp(exp)


def window_cache(family, q16, nq, nkv, hd, L, first, n, scale, seed, needle_at=None):
    """fp32 targets (K, V) [nkv, L, hd] whose keys first .. n - 1 are attn_reference.build_cache's family over n - first keys (the
    ramps rise / fall across the WINDOW, the needle's margin is over the window's keys), N(0, 0.5) elsewhere.  needle_at: absolute."""
    K, V = ar.build_cache("base", q16, nq, nkv, hd, L, n, scale, seed + 50)
    if family == "needle":
        at = needle_at - first
        if 0 <= at < n - first:
            Kw, Vw = ar.build_cache("needle", q16, nq, nkv, hd, n - first, n - first, scale, seed, needle_at=at)
        else:
            # a needle OUTSIDE the window (below first: it must not be seen), as strong as one inside would be
            Kn, Vn = ar.build_cache("needle", q16, nq, nkv, hd, n - first, n - first, scale, seed, needle_at=0)
            K[:, needle_at], V[:, needle_at] = Kn[:, 0], Vn[:, 0]
            Kw, Vw = ar.build_cache("base", q16, nq, nkv, hd, n - first, n - first, scale, seed)
    else:
        Kw, Vw = ar.build_cache(family, q16, nq, nkv, hd, n - first, n - first, scale, seed)
    K[:, first:n], V[:, first:n] = Kw, Vw
    return K, V
