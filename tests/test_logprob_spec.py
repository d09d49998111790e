"""The log-probability contract without a GPU: sampling.reference_logprob (numpy fp64) is the specification the kernel tests
(tests/test_score.py) hold qpal_token_logprob to.  Here: its known answers, the argument errors of the entry point as return
codes, the wrappers' checks, and that a Sampler without logprobs is what it was."""
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


def test_symbols_and_exports():
    lib = qp._native.lib()
    assert "qpal_token_logprob" in qp._native.exported_symbols() and hasattr(lib, "qpal_token_logprob")
    with open(os.path.join(ROOT, "include", "qpal.h")) as f:
        assert "qpal_token_logprob(" in f.read()
    assert callable(qp.token_logprobs) and callable(qp.reference_logprob) and callable(qp.perplexity)
    assert issubclass(qp.Score, qp.Prefill) and qp.Score is qp.decoder.Score
    assert qp.token_logprobs is sampling.token_logprobs and qp.reference_logprob is sampling.reference_logprob


def _call(lib, logits=64, ld=1024, rows=8, vocab=1000, tok=64, lp=64, lse=64, rank=64, active=None):
    return lib.qpal_token_logprob(logits, ld, rows, vocab, tok, lp, lse, rank, active, None)


def test_argument_errors_without_a_gpu():
    """host checks, returned before anything touches a device: the small integers below are never dereferenced"""
    lib = qp._native.lib()
    for kw in ({"logits": None}, {"tok": None}, {"lp": None}):
        assert _call(lib, **kw) == E_NULL, kw
    for kw in ({"rows": 0}, {"rows": 129}, {"vocab": 0}, {"ld": 999}, {"vocab": -5}):
        assert _call(lib, **kw) == E_SHAPE, kw
    for kw in ({"logits": 66}, {"tok": 68}, {"lp": 66}, {"lse": 66}, {"rank": 66}, {"active": 68}):
        assert _call(lib, **kw) == E_ALIGN, kw
    # null lse / rank / active are accepted: with them only the shape is left to object to
    assert _call(lib, lse=None, rank=None, active=None, rows=0) == E_SHAPE


def test_wrappers_check_before_the_library():
    z, E = torch.zeros, qp._native.QpalError
    tok = z(4, dtype=torch.int64)
    with pytest.raises(E):
        qp.token_logprobs(z(4, 100), tok)                              # not on a device
    with pytest.raises(E):
        qp.token_logprobs(z(4, 100, dtype=torch.float16), tok)         # wrong dtype
    with pytest.raises(E):
        qp.token_logprobs(z(100), tok)                                 # not [rows, vocab]
    # past the logits checks only with a device tensor; the token / output checks are _param's, shown on it directly
    for bad in (z(4, dtype=torch.int32), z(5, dtype=torch.int64), z(4, 1, dtype=torch.int64), z(8, dtype=torch.int64)[::2]):
        with pytest.raises(E):
            sampling._param(bad, "tokens", torch.int64, 4, torch.device("cpu"), "token_logprobs")
    assert sampling._param(tok, "tokens", torch.int64, 4, torch.device("cpu"), "token_logprobs") == tok.data_ptr()


def test_reference_known_answers():
    ref = sampling.reference_logprob
    # a uniform row of V logits c: -ln V, lse c + ln V, rank 0
    for V, c in ((1, 3.5), (7, 0.0), (1000, -12.25), (128256, 80.0)):
        lp, lse, rank = ref(np.full(V, c, dtype=np.float32), V // 2)
        assert abs(lp + math.log(V)) < 1e-12 and abs(lse - (c + math.log(V))) < 1e-12 and rank == 0
    # two points by hand: l = (0, ln 3) -> p = (1/4, 3/4)
    row = np.array([0.0, math.log(3.0)], dtype=np.float32)
    l1 = float(row[1])
    lse = math.log(1.0 + math.exp(l1))
    assert ref(row, 0) == pytest.approx((-lse, lse, 1), abs=1e-15)
    assert ref(row, 1) == pytest.approx((l1 - lse, lse, 0), abs=1e-15)
    assert abs(math.exp(ref(row, 0)[0]) - 0.25) < 1e-7
    # the result does not move with a common offset beyond fp32's rounding of the inputs (offsets exact in fp32 here)
    base = np.array([0.5, -1.25, 3.0, 2.0], dtype=np.float32)
    for off in (80.0, -80.0):
        a, b = ref(base, 2), ref(base + np.float32(off), 2)
        assert abs(a[0] - b[0]) < 1e-12 and abs(a[1] + off - b[1]) < 1e-12 and a[2] == b[2] == 0
    # token out of range: the row is inactive
    assert ref(base, -1) is None and ref(base, 4) is None and ref(base, 1 << 40) is None


def test_reference_nan_and_infinities():
    ref = sampling.reference_logprob
    ninf, nan = -np.inf, np.nan
    row = np.array([1.0, nan, 2.0, ninf, 2.0], dtype=np.float32)
    lse = math.log(math.exp(1.0) + 2.0 * math.exp(2.0))
    assert ref(row, 0) == pytest.approx((1.0 - lse, lse, 2), abs=1e-15)
    assert ref(row, 2) == pytest.approx((2.0 - lse, lse, 0), abs=1e-15)      # a tie with the target is not above it
    assert ref(row, 1) == (ninf, pytest.approx(lse, abs=1e-15), 3)             # a NaN logit is read as -inf
    assert ref(row, 3) == (ninf, pytest.approx(lse, abs=1e-15), 3)
    for dead in (np.full(6, ninf, dtype=np.float32), np.full(6, nan, dtype=np.float32)):
        assert ref(dead, 2) == (ninf, ninf, 0)                                   # a row without a finite logit
    top = np.array([0.0, np.inf, 5.0, np.inf], dtype=np.float32)
    assert ref(top, 1) == (pytest.approx(-math.log(2.0)), np.inf, 0) and ref(top, 2) == (ninf, np.inf, 2)


def test_reference_probabilities_sum_to_one():
    rng = np.random.default_rng(15)
    for V, sigma in ((33, 1.0), (1000, 3.0), (4096, 6.0)):
        row = (rng.standard_normal(V) * sigma).astype(np.float32)
        row[5] = np.nan
        out = [sampling.reference_logprob(row, t) for t in range(V)]
        assert abs(sum(math.exp(o[0]) for o in out) - 1.0) < 1e-12
        assert len({o[1] for o in out}) == 1
        order = np.argsort(-sampling.clean_logits(row), kind="stable")
        assert [out[t][2] for t in order[:20]] == list(range(20))              # distinct values: the rank is the sorted position
        # and the probabilities are those of the sampler's own reference at temperature 1 without a filter
        p = sampling.probabilities(sampling.clean_logits(row), 1.0, np.ones(V, dtype=bool))
        assert np.allclose([math.exp(o[0]) for o in out], p, rtol=1e-12, atol=0)


def test_a_sampler_without_logprobs_is_what_it_was():
    s = qp.Sampler(4, 100, "cpu", temperature=0.6, top_k=5, seed=9)
    assert s.logprob is None and s.slot(2).logprob is None
    s2 = qp.Sampler(4, 100, "cpu", logprobs=True)
    assert s2.logprob.shape == (4,) and s2.logprob.dtype == torch.float32
    assert s2.slot(2).logprob.data_ptr() == s2.logprob[2:3].data_ptr() and s2.slot(2).logprob.shape == (1,)
    for name in ("temperature", "top_k", "top_p", "seed", "logits"):
        assert getattr(s2, name).shape == getattr(s, name).shape and getattr(s2, name).dtype == getattr(s, name).dtype
    # launches_per_token is arithmetic on the step's configuration: evaluate the property on stand-ins for the three tails
    prop = qp.DecodeStep.launches_per_token.fget
    for rot, ug_il, per_layer in ((True, [(None, None, True)], 5), (True, [(None, None, False)], 6), (False, None, 9)):
        step = types.SimpleNamespace(rot_in_gemv=rot, ug_il=ug_il, layers=[0] * 32, sampler=None)
        assert prop(step) == 32 * per_layer + 1
        step.sampler = s
        assert prop(step) == 32 * per_layer + 2
        step.sampler = s2
        assert prop(step) == 32 * per_layer + 3
