"""Attention score modifiers restated in float64, on top of tests/attn_reference.py and tests/window_reference.py:
the logit soft cap and the per-head sinks, the emulation written from the number formats, the bound with its measured kappa, the
census expectation with a sink, seeded defects, and the list of cases the GPU tests run (the CPU contract test measures kappa on
exactly those).  Used by test_attn_score_contract.py (CPU), test_attn_score.py and test_attn_score_model.py (GPU); device-agnostic.

The contract.  For a row with scaled scores s_j = scale * q.k_j over its admitted keys (causal, and windowed: window_reference.admitted):
  cap > 0:   s_j <- cap * tanh(s_j / cap), behind scale, in front of the mask and the maximum, the row's own new key included;
  sink[h]:   out = sum_j e^(s_j - M) v_j / (sum_j e^(s_j - M) + e^(sink[h] - M)), M = max(max_j s_j, sink[h]) — the sink is not
             capped, has no value row and enters once per row.
score_fp64() writes that as Hugging Face does — cap the scores, concatenate the sink as one more column, softmax, drop the column —
which is NOT the kernels' stable form (a rescale of the keys' sums where the row is finished): the two are independent.

The bound is §23's with the cap's term: 2^-11 |ref| + 2^-24 + kappa (u_p + 2^-23 (1 + Smax + cap)) A.  The cap is a contraction
(|d/ds cap tanh(s / cap)| <= 1), so a score's rounding error from before the cap carries over at most as it is; the fp32 tanh, 1 - 2
/ (exp(2x) + 1), adds an absolute error of a few 2^-24, times cap in the score.  A = sum_j p_j |v_jd| with the p that includes the
sink's share: what a relative error of the weights can move.  Smax is the uncapped sum_d |q_d k_jd| * scale.

kappa is not fixed in advance: measured on the CPU as the worst |fp32 quotient - ref| / ((u_p + 2^-23 (1 + Smax + cap)) A) of
emulate() over every case of measure() — each family x cap in {None, 8, 50} x sinks in {None, N(0, 2), near the row maximum, 40 above
every row's maximum, 40 below} x with and without a window x the three head shapes x both cache formats; every row of the decode launches and of the
prefill and ragged ones (`python tests/score_reference.py` prints this table; test_attn_score_contract.py re-measures the decode
column in full and the other on the first, middle and last row of every sequence).  Elements whose weight term lies below the
bound's absolute floor 2^-24 are left out, as in §31.4 (a sink 40 above every score leaves |out| < 1e-15: the floor is their whole
tolerance):

  family      u_p = 0 (decode)   u_p = 2^-11 (prefill, ragged)
  peaked           0.717              1.041
  ramp_up          1.629              0.877
  ramp_down        0.920              0.871
  offset           1.794              0.922
  needle           1.000              0.071

By the §23 rule kappa is four times the worst, rounded up to a power of two, per u_p: 4 x 1.794 = 7.18 -> 8 for decode, 4 x 1.041 =
4.16 -> 8 for prefill and ragged.  The rounded emulation stays at or below 0.90 of the whole tolerance.  The kernels' own ratios are
printed by the GPU tests and never set it."""
import math

import torch

import attn_reference as ar
import window_reference as wr

U_PREFILL = wr.U_PREFILL
KAPPA = {False: 8.0, True: 8.0}  # keyed by u_p > 0


def tanh_f32(s, cap):
    """cap * tanh(s / cap) in fp32 in the form the kernels use: x = s * (1 / cap) clamped to +-15, 1 - 2 / (exp(2 x) + 1)"""
    s = s.float()
    x = (s * torch.tensor(1.0 / cap, dtype=torch.float32)).clamp(-15.0, 15.0)
    return torch.tensor(cap, dtype=torch.float32) * (1.0 - 2.0 / (torch.exp(2.0 * x) + 1.0))


def _setup(q16, K, V, pos, W, nq, nkv, hd):
    dev, R = q16.device, q16.shape[0]
    ok = wr.admitted(pos, W, 0, int(max(pos)) + 1, dev)
    cols = ok.any(0).nonzero().view(-1)
    j0, j1 = int(cols.min()), int(cols.max()) + 1
    return R, nq // nkv, j0, j1, ok[:, j0:j1][:, None, None, :]


def score_fp64(q16, K, V, pos, W, nq, nkv, hd, scale, cap=None, sinks=None, mutate=None):
    """(ref, A, Smax) for rows at positions pos of ONE sequence (K / V [nkv, L, hd], the new rows in place) under window W, soft cap
    `cap` and sinks fp32 [nq] (None: none): a masked float64 softmax over the capped scores with the sink concatenated as a column
    and dropped behind the softmax.  A = sum_j p_j |v_jd| with that p, Smax the uncapped max_j sum_d |q_d k_jd| * scale.
    mutate seeds one defect into ref (A, Smax stay the correct computation's):
      ("cap_dropped",); ("cap_before_scale",) cap tanh(q.k / cap) * scale; ("cap_not_on_new",) the row's own key keeps its raw score;
      ("cap_on_sink",); ("sink_dropped",); ("sink_times", n) the sink counted n (an int or one per row) times: once per chunk or
      tile; ("sink_value_row",) the sink's weight times the row's own v added to the output; ("sink_head", "div_rep" | "plus1")
      head h takes the sink of head h // rep or h + 1; ("sink_before_merge", c) the sink's term taken relative to the maximum of
      the row's LAST chunk of c keys instead of the row's maximum."""
    R, rep, j0, j1, ok = _setup(q16, K, V, pos, W, nq, nkv, hd)
    dev = q16.device
    q = q16.view(R, nkv, rep, hd).float().double()
    Kd, Vd = K[:, j0:j1].float().double(), V[:, j0:j1].float().double()
    raw = torch.einsum("rgpd,gjd->rgpj", q, Kd)
    capf = (lambda x: x) if cap is None else (lambda x: cap * torch.tanh(x / cap))
    s = raw * scale
    sk = None if sinks is None else sinks.double().view(1, nkv, rep, 1).expand(R, nkv, rep, 1)

    def soft(sc, sink):
        sm = sc.masked_fill(~ok, float("-inf"))
        if sink is None:
            return torch.softmax(sm, dim=-1), None
        p = torch.softmax(torch.cat((sm, sink), dim=-1), dim=-1)
        return p[..., :-1], p[..., -1:]

    p, p_sink = soft(capf(s), sk)
    ref = torch.einsum("rgpj,gjd->rgpd", p, Vd).reshape(R, nq * hd)
    A = torch.einsum("rgpj,gjd->rgpd", p, Vd.abs()).reshape(R, nq * hd)
    Smax = (torch.einsum("rgpd,gjd->rgpj", q.abs(), Kd.abs()) * scale).masked_fill(~ok, 0.0).amax(-1).reshape(R, nq)
    if mutate is None:
        return ref, A, Smax
    kind, arg = mutate[0], (mutate[1] if len(mutate) > 1 else None)
    own = (torch.arange(j0, j1, device=dev)[None, :] == torch.as_tensor(pos, device=dev)[:, None])[:, None, None, :]
    sc2, sk2 = capf(s), sk
    if kind == "cap_dropped":
        sc2 = s
    elif kind == "cap_before_scale":
        sc2 = capf(raw) * scale
    elif kind == "cap_not_on_new":
        sc2 = torch.where(own, s, sc2)
    elif kind == "cap_on_sink":
        sk2 = capf(sk)
    elif kind == "sink_dropped":
        sk2 = None
    elif kind == "sink_times":
        n = torch.as_tensor(arg, dtype=torch.float64, device=dev).expand(R) if not isinstance(arg, int) else torch.full((R,), float(arg), device=dev, dtype=torch.float64)
        sk2 = sk + torch.log(n).view(R, 1, 1, 1)
    elif kind == "sink_head":
        h = torch.arange(nq, device=dev)
        sk2 = sinks.double()[h // rep if arg == "div_rep" else (h + 1) % nq].view(1, nkv, rep, 1).expand(R, nkv, rep, 1)
    elif kind == "sink_before_merge":
        sm = sc2.masked_fill(~ok, float("-inf"))
        last = (torch.as_tensor(pos, device=dev) - j0) // arg * arg  # the first key (relative) of the chunk that holds the row's own
        in_last = (torch.arange(j1 - j0, device=dev)[None, :] >= last[:, None])[:, None, None, :]
        m_last = sm.masked_fill(~in_last, float("-inf")).amax(-1, keepdim=True)
        M = torch.maximum(sm.amax(-1, keepdim=True), sk)
        sk2 = sk + (M - m_last)
    elif kind != "sink_value_row":
        raise ValueError(kind)
    p2, p2_sink = soft(sc2, sk2)
    out = torch.einsum("rgpj,gjd->rgpd", p2, Vd)
    if kind == "sink_value_row":
        out = out + p2_sink * torch.einsum("rgpj,gjd->rgpd", own.expand_as(p2).double(), Vd)
    return out.reshape(R, nq * hd), A, Smax


def row_max(q16, K, V, pos, W, nq, nkv, hd, scale, cap=None):
    """float64 [R, nq]: the maximum of every row's (capped) admitted scores — what a sink is placed above or below"""
    R, rep, j0, j1, ok = _setup(q16, K, V, pos, W, nq, nkv, hd)
    s = torch.einsum("rgpd,gjd->rgpj", q16.view(R, nkv, rep, hd).float().double(), K[:, j0:j1].float().double()) * scale
    if cap is not None:
        s = cap * torch.tanh(s / cap)
    return s.masked_fill(~ok, float("-inf")).amax(-1).reshape(R, nq)


def row_lse(q16, K, V, pos, W, nq, nkv, hd, scale, cap=None):
    """float64 [R, nq]: log sum_j e^(s_j) over every row's (capped) admitted scores — a sink at this value takes half the row"""
    R, rep, j0, j1, ok = _setup(q16, K, V, pos, W, nq, nkv, hd)
    s = torch.einsum("rgpd,gjd->rgpj", q16.view(R, nkv, rep, hd).float().double(), K[:, j0:j1].float().double()) * scale
    if cap is not None:
        s = cap * torch.tanh(s / cap)
    return torch.logsumexp(s.masked_fill(~ok, float("-inf")), dim=-1).reshape(R, nq)


def by_rows(fn, q16, K, V, pos, W, *args, **kw):
    """fn = score_fp64 row by row, each row on its own (the definition the batched form is pinned to)"""
    outs = [fn(q16[r:r + 1], K, V, [p], W, *args, **kw) for r, p in enumerate(pos)]
    return tuple(torch.cat(t) for t in zip(*outs))


def emulate(q16, K, V, pos, W, nq, nkv, hd, scale, u_p, cap=None, sinks=None, rounded=True):
    """The arithmetic bound() describes, written from the formats alone: fp32 scores from fp16 factors, the fp32 tanh form, fp32 exp
    and accumulation; for u_p > 0 the weights rounded to fp16 in 32-key tiles (cut on multiples of 32 of the key index) under a
    running maximum, as attn_reference.emulate; the sink added once at the end, to sums that are relative to the keys' maximum; one
    fp16 rounding of the output (rounded=False: the fp32 quotient in front of it)."""
    R, rep, j0, j1, ok = _setup(q16, K, V, pos, W, nq, nkv, hd)
    dev = q16.device
    t0 = j0 // 32 * 32
    q, Kf, Vf = q16.view(R, nkv, rep, hd).float(), K[:, t0:j1].float(), V[:, t0:j1].float()
    ok = torch.nn.functional.pad(ok, (j0 - t0, 0), value=False)
    s = torch.einsum("rgpd,gjd->rgpj", q, Kf) * torch.tensor(scale, dtype=torch.float32)
    if cap is not None:
        s = tanh_f32(s, cap)
    s = s.masked_fill(~ok, float("-inf"))
    Vf = torch.nan_to_num(Vf.masked_fill(~ok.any(0).any(0).any(0)[None, :, None], 0.0))  # (rows no row admits may hold NaN)
    if u_p == 0:
        m = s.amax(-1)
        e = torch.exp(s - m[..., None])
        l, o = e.sum(-1), torch.einsum("rgpj,gjd->rgpd", e, Vf)
    else:
        m = torch.full(s.shape[:-1], -3.0e38, device=dev)
        l = torch.zeros_like(m)
        o = torch.zeros(*m.shape, hd, device=dev)
        for c0 in range(0, j1 - t0, 32):
            st = s[..., c0:c0 + 32]
            m_new = torch.maximum(m, st.amax(-1))
            alpha = torch.exp(m - m_new)
            ph = torch.exp(st - m_new[..., None]).half().float()
            l = l * alpha + ph.sum(-1)
            o = o * alpha[..., None] + torch.einsum("rgpj,gjd->rgpd", ph, Vf[:, c0:c0 + 32])
            m = m_new
    if sinks is not None:
        sk = sinks.float().view(1, nkv, rep).expand_as(m)
        M = torch.maximum(m, sk)
        f = torch.exp(m - M)
        l, o = l * f + torch.exp(sk - M), o * f[..., None]
    o = (o / l[..., None]).reshape(R, nq * hd)
    return o.half() if rounded else o


def weight_term(A, Smax, u_p, cap=None):
    """(u_p + 2^-23 (1 + Smax + cap)) A: what kappa multiplies in bound()"""
    hd = A.shape[-1] // Smax.shape[-1]
    return (u_p + 2.0 ** -23 * (1.0 + Smax.repeat_interleave(hd, dim=-1) + (cap or 0.0))) * A


def bound(ref, A, Smax, u_p, cap=None):
    """2^-11 |ref| + 2^-24 + kappa (u_p + 2^-23 (1 + Smax + cap)) A"""
    return 2.0 ** -11 * ref.abs() + 2.0 ** -24 + KAPPA[u_p > 0] * weight_term(A, Smax, u_p, cap)


def unstable_sink_term(row_maximum, sinks):
    """fp32 e^(sink - max_j s_j), the sink's term when M is taken WITHOUT the sink: what overflows"""
    return torch.exp(sinks.float()[None, :] - row_maximum.float())


def census_expected(pos, W, nq, hd, dev, sink_count=1):
    """the census with sink = 0: every score is 0 and so is the sink, every weight is 1 / (n + sink_count); out[r, h, d] = #{lo <= j <=
    pos[r] : j = d (mod hd)} / (n + 1), n = pos[r] + 1 - lo, and its tolerance, one fp16 ulp (window_reference.census_expected's
    reasoning: exact counts, M = 0 = every score, every rescale exp(0) = 1, one fp32 division, one fp16 rounding).  sink_count: what
    a defect would count (0: dropped, the number of chunks or tiles: once per each)."""
    n = torch.as_tensor([p + 1 for p in pos], dtype=torch.long, device=dev).view(-1, 1)
    l = torch.as_tensor([wr.lo(p, W) for p in pos], dtype=torch.long, device=dev).view(-1, 1)
    d = torch.arange(hd, device=dev)[None, :]
    below = lambda x: (x - d + hd - 1).clamp(min=0) // hd  # noqa: E731
    extra = torch.as_tensor(sink_count, dtype=torch.float64, device=dev).view(-1, 1) if not isinstance(sink_count, int) else float(sink_count)
    exp = ((below(n) - below(l)).double() / ((n - l).double() + extra)).repeat(1, nq)
    return exp, ar.fp16_ulp(exp)


# ------------------------------------------------------------------------------------------- the cases of the GPU tests

SHAPES = [(8, 1, 64), (4, 2, 256), (8, 2, 128)]  # gpt-oss's rep 8, Gemma-2's hd 256, and (8, 2, 128)
DTYPES = [ar.F16, ar.F8]
CAPS = (None, 8.0, 50.0)
SINK_KINDS = (None, "normal", "near", "above", "below")  # near: beyond what §32 asks for — a sink that competes with the top keys
DECODE_L, DECODE_POS, DECODE_W = 2048, (40, 2047), (None, 700)     # max_len >= 512: the split launch; one chunk at 40, a merge at 2047
PREFILL_L, PREFILL_ROWS, PREFILL_W = 1024, ((17, 900), (33, 0)), (None, 600)  # (T, pos0): a merged launch and a one-chunk one
RAGGED_ROWS, RAGGED_POS0 = (5, 17, 40), (0, 31, 900)                # three segments of unequal length on the prefill cache


def sequences(kind):
    """the sequences of a launch of `kind`: (T, pos0) each — decode: one new row per sequence"""
    if kind == "decode":
        return [(1, p) for p in DECODE_POS]
    return list(PREFILL_ROWS) if kind == "prefill" else list(zip(RAGGED_ROWS, RAGGED_POS0))


def launch_shape(kind):
    """(L, the windows, u_p) of the launches of `kind`; prefill launches its sequences one by one, the others in one launch"""
    return (DECODE_L, DECODE_W, 0.0) if kind == "decode" else (PREFILL_L, PREFILL_W, U_PREFILL)


def needle_at(pos0, W):
    """the needle of a sequence: the middle of its first row's window"""
    l = wr.lo(pos0, W)
    return l + (pos0 - l) // 2


def make_sinks(kind, row_maxima, nq, seed=11):
    """fp32 [nq] on row_maxima's device.  normal: N(0, 2) per head; near: the median row maximum + N(0, 1) per head (the sink weighs
    about as much as the row's best key); above / below: 40 above the largest / below the smallest row maximum of the launch, per
    head (row_maxima: float64 [rows of the whole launch, nq])"""
    dev = row_maxima.device
    if kind is None:
        return None
    if kind == "normal":
        return (2.0 * torch.randn(nq, generator=torch.Generator().manual_seed(seed))).to(dev)
    if kind == "near":
        return (row_maxima.median(0).values + torch.randn(nq, generator=torch.Generator().manual_seed(seed + 1)).to(dev)).float()
    if kind == "above":
        return (row_maxima.amax(0) + 40.0).float()
    if kind == "below":
        return (row_maxima.amin(0) - 40.0).float()
    raise ValueError(kind)


def share(raw, ref, A, Smax, u_p, cap):
    """kappa's share of an fp32 quotient `raw`: |raw - ref| / weight term where that term is at least the bound's floor 2^-24"""
    wt = weight_term(A, Smax, u_p, cap)
    r = ((raw.double() - ref).abs() / wt)[wt >= 2.0 ** -24]
    return float(r.max()) if r.numel() else 0.0


def measure(make_case, kinds=("decode", "prefill", "ragged"), rows_of=None, families=ar.FAMILIES):
    """the table of the header: worst share per (family, u_p > 0) and the worst err / whole tolerance of the rounded emulation, over
    cases().  make_case(family, shape, L, dtype, pos, W, needle_at) -> (q16, K, V) builds a sequence; rows_of(T) -> the rows
    measured (None: all)."""
    worst, whole = {}, 0.0
    for kind in kinds:
        L, windows, u_p = launch_shape(kind)
        for shape in SHAPES:
            nq, nkv, hd = shape
            scale = 1.0 / math.sqrt(hd)
            for dtype in DTYPES:
                for family in families:
                    for W in windows:
                        seqs = []
                        for T, pos0 in sequences(kind):
                            pos = list(range(pos0, pos0 + T))
                            seqs.append((pos,) + tuple(make_case(family, shape, L, dtype, pos, W, needle_at(pos0, W) if family == "needle" else None)))
                        groups = [[s] for s in seqs] if kind == "prefill" else [seqs]  # the rows that share one sinks vector
                        for cap in CAPS:
                            for group in groups:
                                rm = torch.cat([row_max(q16, K, V, pos, W, nq, nkv, hd, scale, cap) for pos, q16, K, V in group])
                                for sk in SINK_KINDS:
                                    sinks = make_sinks(sk, rm, nq)
                                    for pos, q16, K, V in group:
                                        sel = list(range(len(pos))) if rows_of is None else rows_of(len(pos))
                                        qs, ps = q16[sel], [pos[i] for i in sel]
                                        ref, A, Smax = score_fp64(qs, K, V, ps, W, nq, nkv, hd, scale, cap, sinks)
                                        raw = emulate(qs, K, V, ps, W, nq, nkv, hd, scale, u_p, cap, sinks, rounded=False)
                                        emu = raw.half().double()  # (the emulation's own last step)
                                        key = (family, u_p > 0)
                                        worst[key] = max(worst.get(key, 0.0), share(raw, ref, A, Smax, u_p, cap))
                                        whole = max(whole, float(((emu - ref).abs() / bound(ref, A, Smax, u_p, cap)).max()))
    return worst, whole


def print_table(worst, whole):
    print("score-modifier emulation err / weight term at kappa = 1, worst per family:")
    print("  family      u_p = 0 (decode)   u_p = 2^-11 (prefill, ragged)")
    for family in ar.FAMILIES:
        print(f"  {family:10s} {worst.get((family, False), float('nan')):10.3f} {worst.get((family, True), float('nan')):18.3f}")
    print(f"worst err / whole tolerance: {whole:.3f}")


if __name__ == "__main__":
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from test_window_contract import _case

    print_table(*measure(lambda family, shape, L, dtype, pos, W, at: _case(family, shape, L, dtype, pos, W, needle_at=at)))
