"""The sampling contract without a GPU: sampling.reference_draw (numpy fp64, its own Philox4x32-10) is the specification the
kernel tests (tests/test_sampling.py) hold qpal_sample to.  Here: the generator's known answers, the top-k set against the
arithmetic of the decode loop this project was modelled on, the distribution the draw samples (chi-square), and the argument
errors of the two new entry points as return codes."""
import math
import os

import numpy as np
import torch

import qpalette_amd as qp
from qpalette_amd import sampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_SHAPE, E_NULL, E_ALIGN = -1, -3, -4


def test_symbols_and_exports():
    lib = qp._native.lib()
    for name in ("qpal_lm_head_logits", "qpal_sample"):
        assert name in qp._native.exported_symbols() and hasattr(lib, name)
    with open(os.path.join(ROOT, "include", "qpal.h")) as f:
        hdr = f.read()
    assert "qpal_lm_head_logits(" in hdr and "qpal_sample(" in hdr
    assert callable(qp.lm_head_logits) and callable(qp.sample) and callable(qp.reference_draw) and callable(qp.Sampler)


def test_philox_known_answers():
    """Philox4x32-10 known answers (the Random123 test vectors)"""
    cases = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
             ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
             ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in cases:
        out = sampling.philox4x32(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))
        assert " ".join(f"{int(v):08x}" for v in out) == want
    # vectorised over counters = one at a time
    ctrs = np.array([c[0] for c in cases], dtype=np.uint32)
    one = sampling.philox4x32(ctrs, np.array(cases[2][1], dtype=np.uint32))
    assert np.array_equal(one[1], sampling.philox4x32(ctrs[1], np.array(cases[2][1], dtype=np.uint32)))


def test_race_uses_word_i_and_3_of_counter_i_shift_2():
    """s[i] = z[i] - ln(-ln u), u = ((x >> 9) + 0.5) 2^-23, x = word i & 3 of Philox(counter (i >> 2, 0, ctr_lo, ctr_hi), key seed)"""
    seed, ctr, vocab = (0x299F31D0 << 32) | 0xA4093822, (5 << 32) | 77, 11
    s = sampling.race_scores(np.zeros(vocab), seed, ctr)
    for i in (0, 3, 6, 10):
        x = sampling.philox4x32(np.array([i >> 2, 0, 77, 5], dtype=np.uint32), np.array([0xA4093822, 0x299F31D0], dtype=np.uint32))[i & 3]
        u = ((int(x) >> 9) + 0.5) * 2.0 ** -23
        assert 0.0 < u < 1.0 and s[i] == -math.log(-math.log(u))
    # a vector of counters = one at a time; a negative counter is an inactive row
    many = sampling.race_scores(np.zeros(vocab), seed, np.array([3, ctr]))
    assert np.array_equal(many[1], s)
    assert sampling.reference_draw(np.zeros(vocab), 1.0, 0, 1.0, seed, -1) is None


def _reference_loop_kept(logits, temperature, top_k):
    """logits_to_probs(...) > 0 of the decode loop this was modelled on: logits / T, pivot = the k-th of topk, logits < pivot -> -inf,
    softmax (fp64 here, so that no kept probability underflows)"""
    l = torch.from_numpy(logits).double() / max(temperature, 1e-5)
    v, _ = torch.topk(l, min(top_k, l.shape[-1]))
    l = torch.where(l < v[-1], -float("inf"), l)
    return (torch.softmax(l, dim=-1) > 0).numpy()


def test_topk_set_is_the_reference_loops():
    rng = np.random.default_rng(3)
    for vocab, k, T in ((64, 5, 0.6), (1000, 5, 0.6), (1000, 50, 1.3), (33, 40, 0.6), (128, 1, 0.6), (4096, 7, 0.25)):
        l = rng.standard_normal(vocab).astype(np.float32)
        if k > 1:  # ties at the pivot: copies of the k-th largest value
            kth = np.sort(l)[::-1][min(k, vocab) - 1]
            l[[1, vocab // 2, vocab - 1]] = kth
        want = _reference_loop_kept(l, T, k)
        got = sampling.topk_mask(sampling.clean_logits(l), k if k < vocab else 0)
        assert np.array_equal(got, want), (vocab, k)
        if k > 1:
            assert got.sum() >= min(k, vocab) and (k >= vocab or got.sum() > k)
        # and the draw stays inside it
        toks = sampling.reference_draw(l, T, k, 1.0, 11, np.arange(200))
        assert want[toks].all()
        if k == 1:
            assert (toks == int(np.argmax(l))).all()


def test_top_p_is_a_threshold_set():
    p = np.array([0.4, 0.2, 0.2, 0.1, 0.05, 0.05])
    l = np.log(p).astype(np.float32)
    all_ = np.ones(6, dtype=bool)
    pr = sampling.probabilities(l, 1.0, all_)
    assert np.allclose(pr, p, atol=1e-7)
    assert sampling.nucleus_mask(pr, all_, 0.3).tolist() == [True, False, False, False, False, False]
    assert sampling.nucleus_mask(pr, all_, 0.5).tolist() == [True, True, True, False, False, False]   # ties stay together
    assert sampling.nucleus_mask(pr, all_, 0.85).tolist() == [True, True, True, True, False, False]
    assert sampling.nucleus_mask(pr, all_, 1.0).all() and sampling.nucleus_mask(pr, all_, 0.0).all()
    k3 = sampling.topk_mask(l, 3)
    assert sampling.nucleus_mask(sampling.probabilities(l, 1.0, k3), k3, 0.6).tolist() == [True, True, True, False, False, False]
    # degenerate rows give a valid token
    assert sampling.reference_draw(np.full(8, np.nan), 0.7, 3, 0.9, 1, 0) == 0
    assert sampling.reference_draw(np.full(8, -np.inf), 0.7, 0, 1.0, 1, 0) == 0
    assert sampling.reference_draw(np.full(8, -np.inf), 0.0, 0, 1.0, 1, 0) == 0


def _chi2_sf(x, dof):
    """upper tail of the chi-square distribution: Q(dof / 2, x / 2), series / continued fraction (Numerical Recipes gammq)"""
    a, x = dof / 2.0, x / 2.0
    if x <= 0:
        return 1.0
    lg = math.lgamma(a)
    if x < a + 1.0:
        ap, s, d = a, 1.0 / a, 1.0 / a
        for _ in range(10000):
            ap += 1.0
            d *= x / ap
            s += d
            if abs(d) < abs(s) * 1e-15:
                break
        return 1.0 - s * math.exp(-x + a * math.log(x) - lg)
    b, c, d = x + 1.0 - a, 1e300, 1.0 / (x + 1.0 - a)
    h = d
    for i in range(1, 10000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        d = 1e-300 if abs(d) < 1e-300 else d
        c = b + an / c
        c = 1e-300 if abs(c) < 1e-300 else c
        d = 1.0 / d
        de = d * c
        h *= de
        if abs(de - 1.0) < 1e-15:
            break
    return math.exp(-x + a * math.log(x) - lg) * h


def test_chi2_helper():
    assert abs(_chi2_sf(3.841458820694124, 1) - 0.05) < 1e-9 and abs(_chi2_sf(18.307038053275146, 10) - 0.05) < 1e-9
    assert abs(_chi2_sf(100.0, 63) - 0.0020758) < 1e-5


def test_the_contract_samples_the_kept_sets_distribution():
    """vocab 64, a fixed logit row, T = 0.7, 20 000 draws with ctr = 0 .. 19 999 per filter setting: chi-square of the counts against
    the fp64 probabilities of the kept set (cells with expectation < 5 pooled), p > 1e-4; no draw outside the kept set.
    p-values with these seeds (101 .. 104): (0, 1): 0.058  (5, 1): 0.992  (0, 0.9): 0.215  (20, 0.8): 0.876"""
    vocab, T, n = 64, 0.7, 20000
    l = (np.random.default_rng(2024).standard_normal(vocab) * 1.5).astype(np.float32)
    for (top_k, top_p), seed in zip(((0, 1.0), (5, 1.0), (0, 0.9), (20, 0.8)), (101, 102, 103, 104)):
        toks = sampling.reference_draw(l, T, top_k, top_p, seed, np.arange(n))
        lc = sampling.clean_logits(l)
        kmask = sampling.topk_mask(lc, top_k)
        kept = sampling.nucleus_mask(sampling.probabilities(lc, np.float32(T), kmask), kmask, float(np.float32(top_p)))
        assert kept[toks].all(), "a draw outside the kept set"
        assert kept.sum() == {(0, 1.0): 64, (5, 1.0): 5}.get((top_k, top_p), kept.sum())
        p = sampling.probabilities(lc, np.float32(T), kept)
        exp = p * n
        obs = np.bincount(toks, minlength=vocab).astype(np.float64)
        cells = kept & (exp >= 5)
        o, e = list(obs[cells]), list(exp[cells])
        pooled = kept & ~cells
        if pooled.any():
            o.append(obs[pooled].sum())
            e.append(exp[pooled].sum())
        o, e = np.array(o), np.array(e)
        stat = float(((o - e) ** 2 / e).sum())
        pval = _chi2_sf(stat, len(o) - 1) if len(o) > 1 else 1.0
        print((top_k, top_p), "kept", int(kept.sum()), "cells", len(o), "chi2", round(stat, 2), "p", round(pval, 4))
        assert pval > 1e-4, (top_k, top_p, stat, pval)


def _logits_call(lib, h=64, ld_h=4096, w_ln=64, eps=1e-5, w=64, out=64, ld_out=1024, rows=8, vocab=1000, k=4096):
    return lib.qpal_lm_head_logits(h, ld_h, w_ln, eps, w, out, ld_out, rows, vocab, k, None)


def _sample_call(lib, logits=64, ld=1024, rows=8, vocab=1000, t=64, tk=64, tp=64, seed=64, ctr=64, tok=64):
    return lib.qpal_sample(logits, ld, rows, vocab, t, tk, tp, seed, ctr, tok, None)


def test_argument_errors_without_a_gpu():
    """host checks, returned before anything touches a device: the small integers below are never dereferenced"""
    lib = qp._native.lib()
    for kw in ({"h": None}, {"w": None}, {"out": None}):
        assert _logits_call(lib, **kw) == E_NULL, kw
    for kw in ({"rows": 0}, {"rows": 129}, {"k": 1000}, {"k": 0}, {"k": 8704}, {"ld_out": 999}, {"ld_h": 4092}, {"vocab": 0}):
        assert _logits_call(lib, **kw) == E_SHAPE, kw
    for kw in ({"w": 64 + 8}, {"w": 66}, {"h": 68}, {"ld_h": 4098}, {"out": 66}, {"w_ln": 66}):
        assert _logits_call(lib, **kw) == E_ALIGN, kw
    for kw in ({"logits": None}, {"t": None}, {"tk": None}, {"tp": None}, {"seed": None}, {"ctr": None}, {"tok": None}):
        assert _sample_call(lib, **kw) == E_NULL, kw
    for kw in ({"rows": 0}, {"rows": 129}, {"vocab": 0}, {"ld": 999}):
        assert _sample_call(lib, **kw) == E_SHAPE, kw
    for kw in ({"logits": 66}, {"t": 66}, {"seed": 68}, {"ctr": 68}, {"tok": 68}):
        assert _sample_call(lib, **kw) == E_ALIGN, kw


def test_wrappers_check_before_the_library():
    z = torch.zeros
    E = qp._native.QpalError
    import pytest
    with pytest.raises(E):
        qp.lm_head_logits(z(4, 4096), None, 0.0, z(100, 4096, dtype=torch.float16))           # not on a device
    with pytest.raises(E):
        qp.sample(z(4, 100), None, z(4, dtype=torch.int64))
    with pytest.raises(E):
        qp.Sampler(0, 100, "cpu")
    with pytest.raises(E):
        qp.Sampler(129, 100, "cpu")
    s = qp.Sampler(4, 100, "cpu", temperature=0.6, top_k=[1, 2, 3, 4], seed=9)
    assert s.temperature.dtype == torch.float32 and s.top_k.tolist() == [1, 2, 3, 4] and s.seed.tolist() == [9] * 4
    assert s.top_p.tolist() == [1.0] * 4 and s.logits.shape == (4, 100) and s.logits.dtype == torch.float32
    s.set(2, temperature=0.0, top_p=0.5, seed=-3)
    assert s.temperature[2] == 0 and s.top_p[2] == 0.5 and s.seed[2] == -3 and s.top_k[2] == 3
    v = s.slot(2)
    assert v.B == 1 and v.seed.data_ptr() == s.seed[2:3].data_ptr() and v.logits.shape == (1, 100)
    with pytest.raises(E):
        s.set(4, seed=1)
