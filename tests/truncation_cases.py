"""What tests/test_truncation_spec.py (CPU) and tests/test_truncation.py (GPU) share: the inputs of the contract test of
qpal_sample_trunc, the sandwich a draw is judged by, and an fp32 emulation of the kernel's arithmetic.

The sandwich is that of tests/test_sampling.py with step 4a added.  A draw is judged on the logits the kernel was given:
  * the token is in the top-k set (exact) and in the OUTER set; it wins the race against the INNER set within delta;
  * outer / inner = sampling.truncation_mask on nucleus(top_p +- EPS) with min_p (1 -+ EPS), top_a (1 -+ EPS), typical_p +- EPS and d
    compared with delta_t +- tol_d.  Where the two nuclei differ the kernel's N is one of them, and the draw passes if it passes
    under either.  An empty inner set allows the fallback token (argmax l over N) as well;
  * EPS = 2^-16 and delta are tests/test_sampling.py's.  min-p compares ONE weight w = expf((l - lmax) / T) with min_p: the
    relative error of one summand, < 2^-17.  top-a compares it with top_a / S, S exact in its summands (2^-40 fixed point, truncation
    <= 2^-23) and rounded to fp32 once, the quotient once: < 2^-17 + 2^-22 < EPS.  typical-p's mass target is top-p's;
  * tol_d = 2^-18 max(16, max|l| / T).  The kernel computes d = |g - c| in fp32 with g = (lmax - l) / T (two roundings on a magnitude
    <= 2 max|l| / T), c = fp32(M / S) (one rounding; M and S exact in their summands, M / S in fp64) and the subtraction (one): four
    roundings, <= 4 * 2^-24 * 2 max|l| / T = 2^-21 max|l| / T, times eight.  What the summands' own error (relative e_i <= (2 g_i + 2)
    2^-24 each) moves c by is sum q_i e_i |g_i - c| <= 2^-23 E[(g + 1) |g - c|], below 2^-17 for every row here (E[...] < 64): inside
    the factor eight's room (tol_d >= 2^-14)."""
import functools

import numpy as np

from qpalette_amd import sampling

EPS = 2.0 ** -16

# (temperature, top_k, top_p, min_p, top_a, typical_p) by row type
TRUNC_TYPES = [
    (1.0, 0, 1.0, 0.05, 0.0, 1.0),    # min-p
    (0.8, 0, 1.0, 0.0, 0.2, 1.0),     # top-a
    (1.0, 0, 1.0, 0.0, 0.0, 0.9),     # typical-p, wide
    (0.7, 0, 1.0, 0.0, 0.0, 0.2),     # typical-p, narrow
    (0.7, 50, 0.9, 0.1, 0.0, 0.95),   # top-k + top-p + min-p + typical-p
    (0.8, 0, 0.95, 0.0, 0.0, 1.0),    # neutral
    (0.0, 0, 1.0, 0.05, 0.2, 0.9),    # greedy
    "inactive",
]
SHAPES = [(vocab, rows, sigma) for vocab in (128256, 1000, 33) for rows in (1, 128) for sigma in (1.0, 2.5)]
COUNTERS = 3


@functools.lru_cache(maxsize=None)
def contract_case(case):
    """(logits fp32 [rows, vocab], types [rows], seeds [rows], ctr int64 [COUNTERS, rows]) of SHAPES[case]: numpy, seeded, so that
    the CPU test and the GPU test see the very same inputs"""
    vocab, rows, sigma = SHAPES[case]
    rng = np.random.default_rng(5000 + case)
    logits = (rng.standard_normal((rows, vocab)) * sigma).astype(np.float32)
    types = [TRUNC_TYPES[(r + case) % len(TRUNC_TYPES)] for r in range(rows)]
    seeds = [91 * (case + 1) + 1000003 * r for r in range(rows)]
    ctr = np.array([[-1 if t == "inactive" else rep * 4099 + 17 * r + (1 << 33) * (r % 3 == 2) for r, t in enumerate(types)]
                    for rep in range(COUNTERS)], dtype=np.int64)
    return logits, types, seeds, ctr


def sampler_for(qp, types, seeds, vocab, dev):
    neutral = (1.0, 0, 1.0, 0.0, 0.0, 1.0)
    cols = list(zip(*[neutral if t == "inactive" else t for t in types]))
    return qp.Sampler(len(types), vocab, dev, temperature=cols[0], top_k=cols[1], top_p=cols[2], min_p=cols[3], top_a=cols[4],
                      typical_p=cols[5], seed=seeds, truncation=True)


def contract_check(l, t, seed, ctr, tok):
    """asserts the sandwich of the module docstring for one draw with parameters t = (T, top_k, top_p, min_p, top_a, typical_p);
    returns whether tok is reference_draw's exact winner"""
    T, top_k, top_p, min_p, top_a, typ = t
    vocab = l.shape[0]
    assert 0 <= tok < vocab
    want = sampling.reference_draw(l, T, top_k, top_p, seed, ctr, min_p=min_p, top_a=top_a, typical_p=typ)
    T32, P32 = float(np.float32(T)), float(np.float32(top_p))
    mp, ta, ty = float(np.float32(min_p)), float(np.float32(top_a)), float(np.float32(typ))
    if not T32 > 0 or top_k == 1:
        assert tok == want, ("greedy", tok, want)
        return True
    lc = sampling.clean_logits(l)
    kmask = sampling.topk_mask(lc, top_k)
    assert kmask[tok], ("outside the top-k set", tok, top_k)
    z = lc.astype(np.float64) / T32
    s = sampling.race_scores(z, seed, ctr)
    fin = np.isfinite(lc)
    scale = max(16.0, float(np.abs(lc[fin]).max()) / T32 if fin.any() else 0.0)
    delta, tol_d = 2.0 ** -18 * scale, 2.0 ** -18 * scale
    nuclei = [kmask]
    if 0.0 < P32 < 1.0:
        p = sampling.probabilities(lc, T32, kmask)
        nuclei = [sampling.nucleus_mask(p, kmask, P32 + EPS), sampling.nucleus_mask(p, kmask, P32 - EPS)]
        assert nuclei[0][tok], ("outside nucleus(top_p + eps)", tok, float(p[tok]))
        if np.array_equal(*nuclei):
            nuclei = nuclei[:1]
    why = None
    for n_out, n_in in [(nuclei[0], nuclei[-1])] + [(n, n) for n in nuclei[1:]]:
        ty_out, ty_in = (min(ty + EPS, 1.0 - 2.0 ** -30), max(ty - EPS, 2.0 ** -30)) if 0.0 < ty < 1.0 else (ty, ty)
        outer = sampling.truncation_mask(lc, T32, n_out, mp * (1 - EPS), ta * (1 - EPS), ty_out, fallback=False, tol_d=tol_d)
        inner = sampling.truncation_mask(lc, T32, n_in, mp * (1 + EPS), ta * (1 + EPS), ty_in, fallback=False, tol_d=-tol_d)
        if not inner.any():
            outer = outer.copy()
            outer[int(np.argmax(np.where(n_out, lc, -np.inf)))] = True
        sel = inner & (z > -np.inf)
        best = s[sel].max() if sel.any() else -np.inf
        if not outer[tok]:
            why = ("outside the outer set", tok, want)
        elif not s[tok] >= best - delta:
            why = ("lost the race", tok, want, float(s[tok]), float(best), delta)
        else:
            return tok == want
    raise AssertionError(why)


# ------------------------------------------------------------------------------------------------ the kernel's arithmetic in fp32

F = np.float32
_TWO40 = F(2.0 ** 40)


def _fixed(w32):
    """a weight in [0, 1] as 2^-40 fixed point, truncated: the kernel's (unsigned long long)(w * 2^40f)"""
    return (w32 * _TWO40).astype(np.float64).astype(np.uint64)  # fp32 times a power of two is exact; the cast truncates


def _mass_select_desc(vals, mass, frac):
    """the largest value K with mass{vals >= K} >= floor(frac * total) (clamped to [1, total]); None with no mass"""
    total = int(mass.sum())
    if total == 0:
        return None
    tgt = min(max(int(np.float64(frac) * np.float64(total)), 1), total)
    order = np.argsort(-vals, kind="stable")
    v = vals[order]
    cum = np.cumsum(mass[order].astype(object))  # Python ints: exact
    first = np.flatnonzero(np.r_[True, v[1:] != v[:-1]])
    last = np.r_[first[1:] - 1, len(v) - 1]
    j = next(i for i in range(len(last)) if cum[last[i]] >= tgt)
    return v[first[j]]


def _uniforms(vocab, seed, ctr):
    """u fp32 [vocab] of step 5: ((x >> 9) + 0.5) 2^-23, x = word i & 3 of Philox(counter (i >> 2, 0, ctr_lo, ctr_hi), key seed)"""
    seed, ctr = int(seed) & 0xFFFFFFFFFFFFFFFF, int(ctr) & 0xFFFFFFFFFFFFFFFF
    counter = np.zeros(((vocab + 3) // 4, 4), dtype=np.uint32)
    counter[:, 0] = np.arange(counter.shape[0], dtype=np.uint32)
    counter[:, 2], counter[:, 3] = ctr & 0xFFFFFFFF, ctr >> 32
    x = sampling.philox4x32(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)).reshape(-1)[:vocab]
    return ((x >> np.uint32(9)).astype(F) + F(0.5)) * F(2.0 ** -23)


def emulate_fp32(l, t, seed, ctrs):
    """tokens int64 [len(ctrs)]: csrc/sample.hip's arithmetic for one row in numpy float32 — w, the gaps, d and the race scores in
    fp32, the masses truncated to 2^-40 and summed as integers, M / S in fp64 rounded to fp32 — with numpy's exp / log in the place of
    the device's (both within a few ulp)."""
    T, top_k, top_p, min_p, top_a, typ = t
    T, top_p, min_p, top_a, typ = F(T), F(top_p), F(min_p), F(top_a), F(typ)
    ctrs = np.asarray(ctrs, dtype=np.int64)
    lc = sampling.clean_logits(l)
    if not T > 0 or top_k == 1:
        tok = int(np.argmax(lc)) if lc.max() > -np.inf else 0
        return np.full(ctrs.shape, tok, dtype=np.int64)
    keep = sampling.topk_mask(lc, top_k) & ~np.isnan(np.asarray(l, dtype=np.float32))
    mx = lc.max()
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        g = ((mx - lc) / T).astype(F)
        g = np.where(np.isnan(g), np.where(lc == mx, F(0), F(np.inf)), g).astype(F)
        w = np.exp(-g).astype(F)
        wf = _fixed(w)
        if 0 < top_p < 1 and mx > -np.inf:
            idx = np.flatnonzero(keep & (wf > 0))
            K = _mass_select_desc(lc[idx], wf[idx], top_p)
            if K is not None:
                keep &= lc >= K
        trunc = (min_p > 0 or top_a > 0 or 0 < typ < 1) and mx > -np.inf
        final = keep.copy()
        if trunc:
            wmin = min(min_p, F(1)) if min_p > 0 else F(0)
            idx = np.flatnonzero(keep & (wf > 0))
            S = int(wf[idx].astype(object).sum())
            M = int(_fixed((w[idx] * g[idx]).astype(F)).astype(object).sum())
            if top_a > 0:
                wmin = max(wmin, F(top_a / F(np.float64(S) * 2.0 ** -40)))
            final &= w >= wmin
            if 0 < typ < 1:
                cen = F(np.float64(M) / np.float64(S))
                d = np.abs((g - cen).astype(F))
                dsel = _mass_select_desc(-d[idx].astype(np.float64), wf[idx], typ)
                final &= d <= F(-dsel)
            if not final.any():
                final[int(np.flatnonzero(keep & (lc == mx))[0])] = True
        z = (lc / T).astype(F)
        out = np.zeros(ctrs.shape, dtype=np.int64)
        for i, c in enumerate(ctrs):
            s = (z - np.log(-np.log(_uniforms(lc.shape[0], seed, c)))).astype(F)
            s = np.where(final & (z > -np.inf), s, -np.inf)
            out[i] = int(np.argmax(s)) if s.max() > -np.inf else 0
    return out
