"""The contract of qpal_sample_trunc without a GPU (include/qpal.h): sampling.truncation_mask and the min_p / top_a /
typical_p keywords of sampling.reference_draw are the specification tests/test_truncation.py holds the kernel to.  Here: the
symbols, the neutral defaults, the mask against an independent restatement, its properties, the distribution a draw samples
(chi-square), the argument errors as return codes, and an fp32 emulation of the kernel's arithmetic on the very inputs of the GPU
contract test."""
import math
import os

import numpy as np
import pytest

import qpalette_amd as qp
from qpalette_amd import sampling
from test_sampling_spec import _chi2_sf
from truncation_cases import COUNTERS, SHAPES, contract_case, contract_check, emulate_fp32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_SHAPE, E_NULL, E_ALIGN = -1, -3, -4


def test_symbols_and_exports():
    lib = qp._native.lib()
    assert "qpal_sample_trunc" in qp._native.exported_symbols() and hasattr(lib, "qpal_sample_trunc")
    assert len(qp._native._SIGNATURES["qpal_sample_trunc"]) == 14
    with open(os.path.join(ROOT, "include", "qpal.h")) as f:
        assert "int qpal_sample_trunc(" in f.read()
    assert callable(qp.truncation_mask) and qp.truncation_mask is sampling.truncation_mask
    assert sampling.TRUNCATION == ("min_p", "top_a", "typical_p")
    s = qp.Sampler(2, 10, "cpu", min_p=0.1)
    assert s.min_p.tolist() == pytest.approx([0.1, 0.1]) and s.top_a.tolist() == [0.0, 0.0] and s.typical_p.tolist() == [1.0, 1.0]


def _mixed_rows(n_per, seed):
    """(l, T, top_k, top_p) over vocab {33, 1000} x sigma {1, 2.5, 6} with mixed T / k / p"""
    rng = np.random.default_rng(seed)
    settings = [(1.0, 0, 1.0), (0.6, 5, 1.0), (0.8, 0, 0.95), (0.7, 50, 0.9), (1.3, 20, 0.5), (0.0, 0, 1.0), (0.9, 1, 1.0)]
    for vocab in (33, 1000):
        for sigma in (1.0, 2.5, 6.0):
            for i in range(n_per):
                yield ((rng.standard_normal(vocab) * sigma).astype(np.float32),) + settings[i % len(settings)]


def test_neutral_keywords_change_nothing():
    """336 rows: reference_draw with neutral keywords (the defaults; min_p / top_a <= 0; typical_p >= 1 or <= 0) = without them"""
    n = 0
    neutrals = [dict(min_p=0.0, top_a=0.0, typical_p=1.0), dict(min_p=-1.0, top_a=-0.5, typical_p=0.0), dict(typical_p=1.5)]
    for i, (l, T, k, p) in enumerate(_mixed_rows(56, 1)):
        ctr = np.arange(4) + 5 * i
        want = sampling.reference_draw(l, T, k, p, 17 + i, ctr)
        assert np.array_equal(sampling.reference_draw(l, T, k, p, 17 + i, ctr, **neutrals[i % 3]), want)
        assert sampling.reference_draw(l, T, k, p, 17 + i, int(ctr[1]), **neutrals[i % 3]) == int(want[1])
        n += 1
    assert n >= 300
    all_ = np.ones(33, dtype=bool)
    assert sampling.truncation_mask(np.zeros(33, np.float32), 1.0, all_).all()


def _restated(l, T, nmask, min_p, top_a, typ, rel=1e-9):
    """(R as a list of bools, near): step 4a of include/qpal.h restated with a full sort, a running sum and explicit loops.  near:
    some q or d (or the running mass) lies within `rel` relative of its threshold without being equal to it."""
    ids = [i for i in range(len(l)) if nmask[i]]
    z = {i: float(l[i]) / T for i in ids}
    zmax = max(z.values())
    w = {i: math.exp(z[i] - zmax) for i in ids}
    S = math.fsum(w.values())
    q = {i: w[i] / S for i in ids}
    qmax = max(q.values())
    keep, near = {i: True for i in ids}, False
    for on, thr in ((min_p > 0, min(min_p, 1.0) * qmax), (top_a > 0, top_a * qmax * qmax)):
        if on:
            for i in ids:
                near |= q[i] != thr and abs(q[i] - thr) <= rel * thr
                if q[i] < thr:
                    keep[i] = False
    if 0.0 < typ < 1.0:
        H = -math.fsum(q[i] * math.log(q[i]) for i in ids if q[i] > 0)
        d = {i: abs(-math.log(q[i]) - H) if q[i] > 0 else math.inf for i in ids}
        order = sorted(ids, key=lambda i: d[i])
        run, delta = 0.0, d[order[-1]]
        for pos, i in enumerate(order):
            run += q[i]
            last_of_ties = pos + 1 == len(order) or d[order[pos + 1]] != d[i]
            if last_of_ties:
                near |= abs(run - typ) <= rel * typ
                if run >= typ:
                    delta = d[i]
                    break
        for i in ids:
            near |= d[i] != delta and abs(d[i] - delta) <= rel * max(delta, 1e-300)
            if d[i] > delta:
                keep[i] = False
    if not any(keep.values()):
        best = max(ids, key=lambda i: (float(l[i]), -i))
        keep[best] = True
    return [bool(nmask[i]) and keep.get(i, False) for i in range(len(l))], near


def test_truncation_mask_is_the_restatement():
    """each filter alone and the three together, on the whole row, a top-k set and a nucleus: equal masks wherever no q or d lies
    within 1e-9 relative of its threshold; such inputs are at most 1 % (printed).  The restatement measures d as |-ln q - H|, the
    mask as |(zmax - z) - c|: equal up to rounding, which is what the 1e-9 is for."""
    rng = np.random.default_rng(77)
    settings = [(0.05, 0.0, 1.0), (0.3, 0.0, 1.0), (0.0, 0.2, 1.0), (0.0, 1.5, 1.0), (0.0, 0.0, 0.9), (0.0, 0.0, 0.2), (0.0, 0.0, 0.5),
                (0.1, 0.2, 0.95), (0.02, 0.05, 0.6)]
    total = near_n = 0
    for vocab, sigma in ((33, 1.0), (33, 2.5), (200, 1.0), (200, 6.0)):
        for rep in range(12):
            l = (rng.standard_normal(vocab) * sigma).astype(np.float32)
            if rep % 3 == 0:
                l[[3, 11, 20]] = l[5]  # exact ties
            T = (1.0, 0.7, 1.4)[rep % 3]
            kmask = sampling.topk_mask(l, (0, 10, 0)[rep % 3])
            nmask = sampling.nucleus_mask(sampling.probabilities(l, T, kmask), kmask, (1.0, 1.0, 0.9)[rep % 3])
            for mp, ta, ty in settings:
                want, near = _restated(l, T, nmask, mp, ta, ty)
                total += 1
                if near:
                    near_n += 1
                    continue
                got = sampling.truncation_mask(l, T, nmask, mp, ta, ty)
                assert got.tolist() == want, (vocab, sigma, rep, mp, ta, ty)
    print(f"{total} inputs, {near_n} within 1e-9 of a threshold ({100.0 * near_n / total:.2f} %)")
    assert total >= 400 and near_n <= 0.01 * total


def test_properties_of_the_kept_set():
    rng = np.random.default_rng(5)
    for vocab, sigma, T in ((33, 1.0, 1.0), (1000, 2.5, 0.8), (1000, 6.0, 1.2), (257, 1.0, 0.5)):
        l = (rng.standard_normal(vocab) * sigma).astype(np.float32)
        all_ = np.ones(vocab, dtype=bool)
        top = int(np.argmax(l))
        mask = lambda **kw: sampling.truncation_mask(l, T, all_, **kw)
        prev = None
        for ty in (0.01, 0.1, 0.3, 0.5, 0.7, 0.9, 0.99, 0.999999):  # R grows with typical_p
            m = mask(typical_p=ty)
            assert m.any() and (prev is None or (m | ~prev).all())
            prev = m
        for name in ("min_p", "top_a"):  # R shrinks with min_p and with top_a, and is never empty
            prev = all_
            for x in (1e-6, 1e-3, 0.05, 0.3, 0.9, 1.0, 3.0, 1e6):
                m = mask(**{name: x})
                assert m.any() and (prev | ~m).all(), (name, x)
                assert name != "min_p" or m[top]  # the argmax is in A for every min_p (values above 1 read as 1)
                prev = m
        l2 = l.copy()
        l2[[1, vocab - 1]] = l.max()
        ties = l2 == l2.max()
        assert np.array_equal(sampling.truncation_mask(l2, T, all_, min_p=1.0), ties)  # min_p = 1: exactly the ties of the maximum
        assert np.array_equal(sampling.truncation_mask(l2, T, all_, min_p=7.0), ties)
        # typical_p -> 0+: exactly the argmin of d
        z = l.astype(np.float64) / T
        w = np.exp(z - z.max())
        q = w / w.sum()
        d = np.abs((z.max() - z) - (q * (z.max() - z)).sum())
        assert np.array_equal(mask(typical_p=1e-12), d == d.min())
        # every combination keeps something inside N
        N = sampling.topk_mask(l, 7)
        for kw in (dict(min_p=0.9, typical_p=0.05), dict(top_a=50.0), dict(min_p=1.0, top_a=2.0, typical_p=0.01)):
            m = sampling.truncation_mask(l, T, N, **kw)
            assert m.any() and (N | ~m).all()
    flat = np.full(50, 1.25, dtype=np.float32)  # all-equal logits keep everything
    for kw in (dict(min_p=1.0), dict(top_a=1.0), dict(typical_p=0.01), dict(min_p=0.5, top_a=0.5, typical_p=0.5)):
        assert sampling.truncation_mask(flat, 0.7, np.ones(50, dtype=bool), **kw).all()


def test_the_empty_intersection_is_the_argmax():
    """one token at 0.4, sixty at 0.01: -ln q of the likeliest token is far below the entropy, so typical_p = 0.5 keeps only small
    tokens, min_p = 0.5 only the likeliest: the intersection is empty and R is the argmax over N (lowest id on ties)"""
    p = np.array([0.01] * 30 + [0.4] + [0.01] * 30)
    l = np.log(p).astype(np.float32)
    all_ = np.ones(61, dtype=bool)
    C = sampling.truncation_mask(l, 1.0, all_, typical_p=0.5)
    A = sampling.truncation_mask(l, 1.0, all_, min_p=0.5)
    assert not C[30] and C.sum() == 60 and A.tolist() == [i == 30 for i in range(61)]
    assert not sampling.truncation_mask(l, 1.0, all_, min_p=0.5, typical_p=0.5, fallback=False).any()
    assert sampling.truncation_mask(l, 1.0, all_, min_p=0.5, typical_p=0.5).tolist() == [i == 30 for i in range(61)]
    assert (sampling.reference_draw(l, 1.0, 0, 1.0, 3, np.arange(50), min_p=0.5, typical_p=0.5) == 30).all()
    l = np.log(np.array([0.002] * 400)).astype(np.float32)
    l[[12, 300]] = np.float32(np.log(0.1))  # a tie of the maximum (q 0.1 each, d 3.1; the others d 0.8): the lowest id
    assert sampling.truncation_mask(l, 1.0, np.ones(400, dtype=bool), min_p=0.9, typical_p=0.3).tolist() == [i == 12 for i in range(400)]
    # degenerate rows follow sampling.probabilities
    inf = np.array([0.0, np.inf, -1.0, np.inf, np.nan], dtype=np.float32)
    lc = sampling.clean_logits(inf)
    for kw in (dict(min_p=0.3), dict(top_a=0.5), dict(typical_p=0.4), dict(min_p=0.3, top_a=0.5, typical_p=0.4)):
        assert sampling.truncation_mask(lc, 1.0, np.ones(5, dtype=bool), **kw).tolist() == [False, True, False, True, False]
        assert sampling.reference_draw(inf, 1.0, 0, 1.0, 1, 0, **kw) == 1
        assert sampling.reference_draw(np.full(8, -np.inf), 0.7, 0, 1.0, 1, 0, **kw) == 0
        assert sampling.reference_draw(np.full(8, np.nan), 0.7, 3, 0.9, 1, 0, **kw) == 0


def test_the_contract_samples_the_truncated_distribution():
    """vocab 33, a fixed logit row, 20 000 draws with ctr = 0 .. 19 999 per filter setting: chi-square of the counts against q
    renormalised over R (cells with expectation < 5 pooled), p > 1e-4; no draw outside R"""
    vocab, n = 33, 20000
    l = (np.random.default_rng(2025).standard_normal(vocab) * 1.5).astype(np.float32)
    cases = [(1.5, 0, 1.0, dict(min_p=0.05)), (1.2, 0, 1.0, dict(top_a=0.1)), (1.5, 0, 1.0, dict(typical_p=0.5)),
             (1.5, 20, 0.95, dict(min_p=0.02, top_a=0.05, typical_p=0.9))]  # 17, 11, 14 (without the likeliest token) and 13 of 17 kept
    for (T, top_k, top_p, kw), seed in zip(cases, (201, 202, 203, 204)):
        toks = sampling.reference_draw(l, T, top_k, top_p, seed, np.arange(n), **kw)
        lc = sampling.clean_logits(l)
        kmask = sampling.topk_mask(lc, top_k)
        N = sampling.nucleus_mask(sampling.probabilities(lc, np.float32(T), kmask), kmask, float(np.float32(top_p)))
        R = sampling.truncation_mask(lc, float(np.float32(T)), N, **{k: float(np.float32(v)) for k, v in kw.items()})
        assert R[toks].all(), "a draw outside the kept set"
        assert 1 < R.sum() < N.sum(), "the setting must cut something and leave a choice"
        exp = sampling.probabilities(lc, np.float32(T), R) * n
        obs = np.bincount(toks, minlength=vocab).astype(np.float64)
        cells = R & (exp >= 5)
        o, e = list(obs[cells]), list(exp[cells])
        pooled = R & ~cells
        if pooled.any():
            o.append(obs[pooled].sum())
            e.append(exp[pooled].sum())
        o, e = np.array(o), np.array(e)
        stat = float(((o - e) ** 2 / e).sum())
        pval = _chi2_sf(stat, len(o) - 1) if len(o) > 1 else 1.0
        print(kw, "kept", int(R.sum()), "of", int(N.sum()), "cells", len(o), "chi2", round(stat, 2), "p", round(pval, 4))
        assert pval > 1e-4, (kw, stat, pval)


def _trunc_call(lib, logits=64, ld=1024, rows=8, vocab=1000, t=64, tk=64, tp=64, mp=64, ta=64, ty=64, seed=64, ctr=64, tok=64):
    return lib.qpal_sample_trunc(logits, ld, rows, vocab, t, tk, tp, mp, ta, ty, seed, ctr, tok, None)


def test_argument_errors_without_a_gpu():
    """host checks, returned before anything touches a device: the small integers below are never dereferenced"""
    lib = qp._native.lib()
    for kw in ({"logits": None}, {"t": None}, {"tk": None}, {"tp": None}, {"seed": None}, {"ctr": None}, {"tok": None}):
        assert _trunc_call(lib, **kw) == E_NULL, kw
        assert _trunc_call(lib, mp=None, ta=None, ty=None, **kw) == E_NULL, kw
    for kw in ({"rows": 0}, {"rows": 129}, {"vocab": 0}, {"ld": 999}):
        assert _trunc_call(lib, **kw) == E_SHAPE, kw
        assert _trunc_call(lib, mp=None, ta=None, ty=None, **kw) == E_SHAPE, kw  # all three filter pointers NULL is accepted so far
    for kw in ({"logits": 66}, {"t": 66}, {"seed": 68}, {"ctr": 68}, {"tok": 68}, {"mp": 66}, {"ta": 66}, {"ty": 66}):
        assert _trunc_call(lib, **kw) == E_ALIGN, kw
    E = qp._native.QpalError
    plain = qp.Sampler(4, 100, "cpu", temperature=0.6, min_p=0.0, top_a=-1.0, typical_p=1.0)
    assert plain.min_p is None and plain.top_a is None and plain.typical_p is None and plain.slot(1).min_p is None
    for kw in (dict(min_p=0.1), dict(top_a=0.1), dict(typical_p=0.5)):
        with pytest.raises(E):
            plain.set(1, **kw)
    plain.set(1, temperature=0.5)
    for s in (qp.Sampler(4, 100, "cpu", truncation=True), qp.Sampler(4, 100, "cpu", typical_p=[1.0, 0.9, 1.0, 1.0])):
        s.set(2, min_p=0.25, typical_p=0.5)
        assert s.min_p.tolist() == [0.0, 0.0, 0.25, 0.0] and s.typical_p[2] == 0.5 and s.top_a.dtype == s.min_p.dtype
        v = s.slot(2)
        assert v.min_p.data_ptr() == s.min_p[2:3].data_ptr() and v.typical_p.shape == (1,)


def test_fp32_emulation_of_the_kernel_on_the_gpu_tests_inputs():
    """truncation_cases.emulate_fp32 — w, d and the scores in numpy float32, masses truncated to 2^-40 — on every draw of the GPU
    contract test: each passes the sandwich, and at most 0.25 % differ from the fp64 contract's winner (the GPU test's cap is 1 %).
    Measured: 0 of 2034."""
    draws = differ = 0
    for case in range(len(SHAPES)):
        logits, types, seeds, ctr = contract_case(case)
        for r, t in enumerate(types):
            if t == "inactive":
                continue
            got = emulate_fp32(logits[r], t, seeds[r], ctr[:, r])
            for i in range(COUNTERS):
                differ += not contract_check(logits[r], t, seeds[r], int(ctr[i, r]), int(got[i]))
                draws += 1
    print(f"draws {draws}, differing from the fp64 winner {differ} ({100.0 * differ / draws:.3f} %)")
    assert draws >= 1500 and differ <= 0.0025 * draws
