"""The top-N log-probability contract without a GPU: sampling.reference_top_logprobs (numpy fp64) is the specification the kernel
tests (tests/test_top_logprobs.py) hold qpal_top_logprob to.  Here: the reference against a brute-force double loop,
its properties on the degenerate rows, the argument errors of the entry point as return codes, the wrappers' checks, and that a
Sampler without top_logprobs is what it was."""
import math
import os
import types

import numpy as np
import pytest
import torch

import qpalette_amd as qp
from qpalette_amd import sampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_SHAPE, E_NULL, E_ALIGN = -1, -3, -4
PAIRS = [(1000, 64), (33, 64), (1, 4), (4099, 20)]
KINDS = ["plain", "constant", "mostly_nan", "all_neg_inf", "three_pos_inf", "threshold_ties", "signed_zeros"]


def make_row(kind, vocab, n, rng):
    """one row of N(0, 3^2) logits with the case `kind` planted"""
    l = (rng.standard_normal(vocab) * 3.0).astype(np.float32)
    if kind == "constant":
        l[:] = np.float32(1.25)
    elif kind == "mostly_nan":        # a handful of finite logits, NaN elsewhere, -inf scattered among them
        keep = rng.choice(vocab, size=min(vocab, 3), replace=False)
        dead = np.full(vocab, np.nan, dtype=np.float32)
        dead[::7] = -np.inf
        dead[keep] = l[keep]
        l = dead
    elif kind == "all_neg_inf":
        l[:] = -np.inf
    elif kind == "three_pos_inf":
        l[rng.choice(vocab, size=min(vocab, 3), replace=False)] = np.inf
    elif kind == "threshold_ties":    # the n-th value has more holders than slots are left for it
        m = min(n, vocab)
        order = np.argsort(-l, kind="stable")
        v = l[order[max(m - 2, 0)]]
        l[order[max(m - 2, 0):m + 5]] = v
        l[[0, vocab - 1, vocab // 2]] = v
    elif kind == "signed_zeros":
        l[:] = np.where(np.arange(vocab) % 2 == 0, np.float32(0.0), np.float32(-0.0))
        l[1::5] = np.float32(-1.0)
    return l


def brute_force(row, n):
    """the order of the contract by a double loop: token i stands before token k if its value is larger, or equal with i < k"""
    l = sampling.clean_logits(row)
    V = l.shape[0]
    before = [sum(1 for i in range(V) if l[i] > l[k] or (l[i] == l[k] and i < k)) for k in range(V)]
    ids = np.full(n, -1, dtype=np.int32)
    for k in range(V):
        if before[k] < n:
            ids[before[k]] = k
    return ids


def test_symbols_and_exports():
    lib = qp._native.lib()
    assert "qpal_top_logprob" in qp._native.exported_symbols() and hasattr(lib, "qpal_top_logprob")
    with open(os.path.join(ROOT, "include", "qpal.h")) as f:
        assert "qpal_top_logprob(" in f.read()
    assert qp.top_logprobs is sampling.top_logprobs and qp.reference_top_logprobs is sampling.reference_top_logprobs


@pytest.mark.parametrize("vocab,n", [(33, 64), (1, 4), (200, 7), (64, 64)])
@pytest.mark.parametrize("kind", KINDS)
def test_reference_against_a_double_loop(kind, vocab, n):
    rng = np.random.default_rng(vocab * 100 + n)
    row = make_row(kind, vocab, n, rng)
    ids, lp, lse = sampling.reference_top_logprobs(row, n)
    assert ids.dtype == np.int32 and ids.shape == (n,) and lp.dtype == np.float64 and lp.shape == (n,)
    assert np.array_equal(ids, brute_force(row, n))
    for j in range(min(n, vocab)):
        want = sampling.reference_logprob(row, ids[j])
        assert lp[j] == want[0] and lse == want[1]


@pytest.mark.parametrize("vocab,n", PAIRS)
@pytest.mark.parametrize("kind", KINDS)
def test_reference_properties(kind, vocab, n):
    rng = np.random.default_rng(vocab + n)
    row = make_row(kind, vocab, n, rng)
    l = sampling.clean_logits(row)
    ids, lp, lse = sampling.reference_top_logprobs(row, n)
    m = min(n, vocab)
    # padding: -1 and -inf past the vocabulary
    assert np.all(ids[m:] == -1) and np.all(lp[m:] == -np.inf)
    assert np.all(ids[:m] >= 0) and np.all(ids[:m] < vocab) and len(set(ids[:m].tolist())) == m
    # strict order by (value descending, id ascending), on fp32 VALUES: -0 == +0
    for j in range(m - 1):
        a, b = l[ids[j]], l[ids[j + 1]]
        assert a > b or (a == b and ids[j] < ids[j + 1]), (j, a, b, ids[j], ids[j + 1])
    # nothing outside the list stands before its last entry
    last = l[ids[m - 1]]
    outside = np.ones(vocab, dtype=bool)
    outside[ids[:m]] = False
    assert not np.any(l[outside] > last) and not np.any((l[outside] == last) & (np.arange(vocab)[outside] < ids[m - 1]))
    # the greedy consequence: the first entry is the sampler's greedy token, degenerate rows included
    assert ids[0] == sampling.reference_draw(row, 0.0, 0, 1.0, 0, 0)
    # every listed token has at most j tokens strictly above it, and its figure is reference_logprob's
    for j in range(m):
        want = sampling.reference_logprob(row, ids[j])
        assert want[2] <= j and lp[j] == want[0] and (lse == want[1])
    fin = np.isfinite(lp)
    assert float(np.exp(lp[fin]).sum()) <= 1.0 + 1e-12
    if kind == "all_neg_inf":
        assert ids[:m].tolist() == list(range(m)) and np.all(lp == -np.inf) and lse == -np.inf
    if kind == "constant":
        assert ids[:m].tolist() == list(range(m)) and np.allclose(lp[:m], -math.log(vocab), atol=1e-12)
    if kind == "three_pos_inf":
        k = int(np.isposinf(l).sum())
        assert lse == np.inf and np.allclose(lp[:min(k, m)], -math.log(k)) and np.all(lp[k:] == -np.inf)
        assert ids[:min(k, m)].tolist() == np.flatnonzero(np.isposinf(l))[:m].tolist()
    if kind == "signed_zeros":
        zeros, rest = [i for i in range(vocab) if l[i] == 0], [i for i in range(vocab) if l[i] != 0]
        assert ids[:m].tolist() == (zeros + rest)[:m]                              # +0 and -0 interleaved: by id alone
    if kind == "mostly_nan" and vocab > 3:
        assert np.all(np.isfinite(lp[:3])) and np.all(lp[3:m] == -np.inf)
        dead = [i for i in range(vocab) if not np.isfinite(l[i])]
        assert ids[3:m].tolist() == dead[:m - 3]                                    # NaN and -inf tie: by id alone


def _call(lib, logits=64, ld=1024, rows=8, vocab=1000, n=5, ids=64, lp=64, lse=64, active=None):
    return lib.qpal_top_logprob(logits, ld, rows, vocab, n, ids, lp, lse, active, None)


def test_argument_errors_without_a_gpu():
    """host checks, returned before anything touches a device: the small integers below are never dereferenced"""
    lib = qp._native.lib()
    for kw in ({"logits": None}, {"ids": None}, {"lp": None}):
        assert _call(lib, **kw) == E_NULL, kw
    for kw in ({"rows": 0}, {"rows": 129}, {"vocab": 0}, {"ld": 999}, {"vocab": -5}, {"n": 0}, {"n": 65}, {"n": -1}):
        assert _call(lib, **kw) == E_SHAPE, kw
    for kw in ({"logits": 66}, {"ids": 66}, {"lp": 66}, {"lse": 66}, {"active": 68}):
        assert _call(lib, **kw) == E_ALIGN, kw
    assert _call(lib, lse=None, active=None, rows=0) == E_SHAPE   # null lse / active are accepted


def test_wrapper_checks_before_the_library():
    z, E = torch.zeros, qp._native.QpalError
    with pytest.raises(E):
        qp.top_logprobs(z(4, 100), 5)                              # not on a device
    with pytest.raises(E):
        qp.top_logprobs(z(4, 100, dtype=torch.float16), 5)         # wrong dtype
    with pytest.raises(E):
        qp.top_logprobs(z(100), 5)                                 # not [rows, vocab]
    with pytest.raises(E):
        qp.Sampler(4, 100, "cpu", top_logprobs=65)
    with pytest.raises(E):
        qp.Sampler(4, 100, "cpu", top_logprobs=-1)


def test_a_sampler_without_top_logprobs_is_what_it_was():
    s = qp.Sampler(4, 100, "cpu", temperature=0.6, top_k=5, seed=9, logprobs=True)
    assert s.top_id is None and s.top_logprob is None and s.slot(2).top_id is None and s.slot(2).top_logprob is None
    assert qp.Sampler(4, 100, "cpu", top_logprobs=0).top_id is None
    s2 = qp.Sampler(4, 100, "cpu", logprobs=True, top_logprobs=5)
    assert s2.top_id.shape == (4, 5) and s2.top_id.dtype == torch.int32 and s2.top_id.is_contiguous()
    assert s2.top_logprob.shape == (4, 5) and s2.top_logprob.dtype == torch.float32 and s2.top_logprob.is_contiguous()
    v = s2.slot(2)
    assert v.top_id.data_ptr() == s2.top_id[2:3].data_ptr() and v.top_id.shape == (1, 5)
    assert v.top_logprob.data_ptr() == s2.top_logprob[2:3].data_ptr() and v.top_logprob.shape == (1, 5)
    for name in ("temperature", "top_k", "top_p", "seed", "logits", "logprob"):
        assert getattr(s2, name).shape == getattr(s, name).shape and getattr(s2, name).dtype == getattr(s, name).dtype
    # launches_per_token is arithmetic on the step's configuration: the top-N launch is one more, with or without logprobs
    prop = qp.DecodeStep.launches_per_token.fget
    s3 = qp.Sampler(4, 100, "cpu", top_logprobs=64)
    for rot, ug_il, per_layer in ((True, [(None, None, True)], 5), (False, None, 9)):
        step = types.SimpleNamespace(rot_in_gemv=rot, ug_il=ug_il, layers=[0] * 32, sampler=s)
        assert prop(step) == 32 * per_layer + 3
        step.sampler = s2
        assert prop(step) == 32 * per_layer + 4
        step.sampler = s3
        assert prop(step) == 32 * per_layer + 3
