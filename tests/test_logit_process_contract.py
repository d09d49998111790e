"""Logit processors without a GPU: the numpy reference on hand-made rows, the C-ABI's argument errors as return codes,
the host setters' checks, and the losslessness argument of §22.3 run as a test on a toy model — speculative steps with penalties,
a mask and a bias emit the stream sequential decoding emits.  The kernel tests (tests/test_logit_process.py) hold
qpal_logit_process / qpal_logit_observe to these references bit for bit."""
import os

import numpy as np
import pytest
import torch

import qpalette_amd as qp
from qpalette_amd import logits as lg
from qpalette_amd import sampling
from qpalette_amd import speculative as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_SHAPE, E_PARAM, E_NULL, E_ALIGN = -1, -2, -3, -4
F32 = np.float32


def _state(slots, vocab, bias_slots=4):
    """a neutral state in numpy, as a dict of reference_process's keyword arguments"""
    return dict(count=np.zeros((slots, vocab), np.int32), repetition=np.ones(slots, F32), presence=np.zeros(slots, F32),
                frequency=np.zeros(slots, F32), mask=np.zeros((slots, (vocab + 31) // 32), np.uint32), mask_on=np.zeros(slots, np.int32),
                bias_id=np.zeros((slots, bias_slots), np.int32), bias_val=np.zeros((slots, bias_slots), F32),
                bias_n=np.zeros(slots, np.int32))


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- the reference

def test_repetition_divides_positive_and_multiplies_negative_logits():
    st = _state(1, 8)
    st["repetition"][0] = 1.3
    st["count"][0, [1, 2]] = 1
    l = np.array([[2.0, 2.0, -2.0, -2.0, 0.5, 0.0, 1.0, -1.0]], F32)
    out = lg.reference_process(l, [0], [5], **st)
    want = l.copy()
    want[0, 1] = F32(2.0) / F32(1.3)
    want[0, 2] = F32(-2.0) * F32(1.3)
    assert out.dtype == F32 and np.array_equal(_bits(out), _bits(want))
    assert out[0, 1] < 2.0 and out[0, 2] < -2.0, "both are pushed down"
    # a counted zero logit is not positive: multiplied, it stays zero
    st["count"][0, 5] = 2
    assert lg.reference_process(l, [0], [5], **st)[0, 5] == 0.0


def test_presence_and_frequency_with_count_three():
    st = _state(2, 8)
    st["presence"][1], st["frequency"][1] = 0.25, 0.5
    st["count"][1, 3], st["count"][1, 4] = 3, 1
    l = np.array([[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]], F32)
    out = lg.reference_process(l, [1], [0], **st)
    assert out[0].tolist() == [1.0, 1.0, 1.0, 1.0 - (0.25 + 0.5 * 3.0), 1.0 - (0.25 + 0.5), 1.0, 1.0, 1.0]
    # one rounding per operation, in the contract's order: (l / rep) - (presence + frequency * float(c)), all in fp32
    st["repetition"][1], st["presence"][1], st["frequency"][1] = 1.3, 0.1, 0.3
    l[0, 3] = 0.7
    out = lg.reference_process(l, [1], [0], **st)
    want = F32(F32(0.7) / F32(1.3)) - F32(F32(0.1) + F32(F32(0.3) * F32(3.0)))
    assert _bits(out[0, 3]) == _bits(F32(want))


def test_a_masked_token_with_a_bias_stays_minus_infinity():
    st = _state(1, 40)
    st["mask"][0] = lg.mask_bits([0, 5, 31, 32, 39], 40)
    st["mask_on"][0] = 1
    st["bias_id"][0, :3], st["bias_val"][0, :3], st["bias_n"][0] = [5, 6, 39], [4.0, 4.0, -1.5], 3
    l = np.arange(40, dtype=F32)[None, :] / 8
    out = lg.reference_process(l, [0], [0], **st)
    allowed = np.zeros(40, bool)
    allowed[[0, 5, 31, 32, 39]] = True
    assert np.all(np.isneginf(out[0, ~allowed])), "token 6 is masked: its bias must not bring it back"
    assert out[0, 5] == l[0, 5] + 4.0 and out[0, 39] == l[0, 39] - 1.5 and out[0, 0] == l[0, 0] and out[0, 32] == l[0, 32]
    # mask_on = 0: the mask is ignored, the bias is not
    st["mask_on"][0] = 0
    out = lg.reference_process(l, [0], [0], **st)
    assert out[0, 6] == l[0, 6] + 4.0 and out[0, 7] == l[0, 7]
    # bias_n cuts the list; an id outside the vocabulary is skipped
    st["bias_n"][0], st["bias_id"][0, 0] = 2, 40
    out = lg.reference_process(l, [0], [0], **st)
    assert out[0, 5] == l[0, 5] and out[0, 6] == l[0, 6] + 4.0 and out[0, 39] == l[0, 39]
    assert lg.mask_bits([33], 34).tolist() == [0, 2] and lg.mask_bits([], 33).tolist() == [0, 0]
    with pytest.raises(ValueError):
        lg.mask_bits([34], 34)


def test_extras_of_a_speculative_row_count_as_if_emitted():
    """slot 1's segment is rows 2 .. 5: pending token 9, guesses 4, 4, 6.  Token 4 has count 1 already: row 4 sees it three times."""
    st = _state(2, 12)
    st["presence"][1], st["frequency"][1] = 0.5, 1.0
    st["count"][1, 4] = 1
    tokens = np.array([3, 4, 9, 4, 4, 6, 0, 0], np.int64)
    row0 = np.array([0, 2, 6], np.int32)
    row_slot = np.array([0, 0, 1, 1, 1, 1, -1, -1], np.int32)
    ctr = np.array([7, 8, 20, 21, 22, 23, -1, -1], np.int64)
    l = np.full((8, 12), 2.0, F32)
    sent = np.full((8, 12), -77.0, F32)
    out = lg.reference_process(l, row_slot, ctr, tokens=tokens, row0=row0, out=sent, **st)
    assert out[2].tolist() == [2.0] * 4 + [2.0 - 1.5] + [2.0] * 7                       # no extras: the stored count alone
    assert out[3, 4] == 2.0 - 2.5 and out[4, 4] == 2.0 - 3.5 and out[4, 6] == 2.0       # one, then two extras equal to token 4
    assert out[5, 4] == 2.0 - 3.5 and out[5, 6] == 2.0 - 1.5 and out[5, 9] == 2.0       # the pending token 9 is no extra
    assert np.array_equal(out[0], l[0]) and np.array_equal(out[1], l[1])                # slot 0 is neutral, its extras change nothing
    assert np.all(out[6:] == -77.0), "rows of no slot are not written"
    # a row that is no row of its slot's segment (more than 15 in front of it, or in front of the segment) is inactive
    out = lg.reference_process(l, np.array([1] * 8, np.int32), np.zeros(8, np.int64), tokens=tokens, row0=np.array([0, 3, 6], np.int32),
                               out=sent, **st)
    assert np.all(out[:3] == -77.0) and np.all(out[3:, 1] == 2.0) and out[7, 0] == 2.0 - 2.5   # (rows 6, 7 are zeros: extras too)


def test_neutral_parameters_return_the_input_bits():
    st = _state(3, 37)
    st["count"][:] = np.random.default_rng(0).integers(0, 4, size=(3, 37))
    l = np.random.default_rng(1).normal(0, 2.5, size=(3, 37)).astype(F32)
    l[0, 3], l[1, 5], l[2, 7], l[0, 9], l[1, 11] = np.nan, -np.inf, np.inf, -0.0, 1e-42  # a denormal too
    out = lg.reference_process(l, [0, 1, 2], [0, 0, 0], **st)
    assert np.array_equal(_bits(out), _bits(l))
    # non-neutral parameters leave the tokens that were never counted alone, bit for bit, and a NaN wherever it is
    st["repetition"][:], st["presence"][:], st["frequency"][:] = 1.3, 0.5, 0.3
    out = lg.reference_process(l, [0, 1, 2], [0, 0, 0], **st)
    keep = (st["count"] == 0) | np.isnan(l)
    assert np.array_equal(_bits(out)[keep], _bits(l)[keep]) and not np.array_equal(_bits(out)[~keep], _bits(l)[~keep])
    assert out[1, 5] == -np.inf and out[2, 7] == np.inf


def test_inactive_rows_and_columns_past_vocab_are_left_alone():
    st = _state(2, 10)
    st["presence"][:] = 1.0
    st["count"][:] = 1
    l = np.ones((4, 12), F32)
    out = lg.reference_process(l, [0, 1, -1, 2], [3, -1, 3, 3], vocab=10, **st)
    assert np.all(out[0, :10] == 0.0) and np.all(out[0, 10:] == 1.0), "columns vocab .. ld are not written"
    assert np.all(out[1:] == 1.0), "ctr < 0, slot < 0 and slot >= slots: not written"


def test_reference_observe_counts_repeats_and_skips_what_does_not_count():
    c = lg.reference_observe(np.zeros((2, 5), np.int32), [0, 0, 1, 1, 2, -1, 0, 0], [3, 3, 3, 5, 1, 1, -1, 4], active=[0, 7, 0, 0, 0, 0, 0, -1])
    assert c.tolist() == [[0, 0, 0, 2, 0], [0, 0, 0, 1, 0]] and c.dtype == np.int32
    assert lg.reference_observe(np.zeros((2, 5), np.int32), 1, [4, 4, 0]).tolist() == [[0] * 5, [1, 0, 0, 0, 2]]


# ---------------------------------------------------------------------------------------------------- losslessness on a toy model

def _toy(seed, V):
    table = np.random.default_rng(seed).normal(0, 2.5, size=(V, V, V, V)).astype(F32)
    return lambda ctx: table[ctx[-3], ctx[-2], ctx[-1]]


def _toy_state(V, B):
    """slot 0: repetition; slot 1: presence + frequency; slot 2: a mask and a bias on two allowed tokens; slot 3: neutral"""
    st = _state(B, V)
    st["repetition"][0] = 1.3
    st["presence"][1], st["frequency"][1] = 0.5, 0.05
    st["mask"][2], st["mask_on"][2] = lg.mask_bits([0, 2, 3, 5, 6], V), 1
    st["bias_id"][2, :2], st["bias_val"][2, :2], st["bias_n"][2] = [2, 5], [1.0, 1.0], 2
    return st


@pytest.mark.parametrize("mode", ["greedy", "seeded"])
@pytest.mark.parametrize("K", [1, 4])
def test_the_speculative_stream_with_processors_is_the_sequential_stream(K, mode):
    """test_spec_contract's toy loop with logits: the next token's logits are a fixed function of the last three tokens over a
    vocabulary of 7, processed with the slot's state and drawn greedily or with a seed.  Sequential: one token at a time, every fed
    token counted.  Speculative: draft -> reference_process with the segment's extras -> one draw per row -> accept -> the emitted
    tokens counted.  Token for token the same stream, and the same counts at the end."""
    V, B, new, ld = 7, 4, 120, 160
    toy = _toy(5, V)
    rng = np.random.default_rng(6)
    prompts = [[int(t) for t in rng.integers(0, V, size=n)] for n in (3, 4, 9, 17)]
    T, seeds = (0.0, [0] * B) if mode == "greedy" else (0.6, [11, 12, 13, 14])

    def draw(l, b, ctr):
        return int(sampling.reference_draw(l, T, 0, 1.0, seeds[b], int(ctr)))

    # ---- sequential: feed s[n - 1] at counter n - 1 with the counts of s[0 .. n)
    want, st = [], _toy_state(V, B)
    for b, p in enumerate(prompts):
        s = list(p)
        st["count"][b] = np.bincount(s, minlength=V)
        for _ in range(new):
            l = lg.reference_process(toy(s)[None, :], [b], [len(s) - 1], **st)
            s.append(draw(l[0], b, len(s) - 1))
            st["count"][b, s[-1]] += 1
        want.append(s[len(p):])
    want_count = st["count"].copy()
    allowed = {0, 2, 3, 5, 6}
    assert set(want[2]) <= allowed and not set(want[3]) <= allowed, "the mask binds in slot 2 and only there"

    # ---- speculative
    st = _toy_state(V, B)
    hist = np.zeros((B, ld), np.int32)
    for b, p in enumerate(prompts):
        hist[b, :len(p)] = p
        st["count"][b] = np.bincount(p, minlength=V)   # begin: reset, then count the known tokens, the pending one included
    n_tok, limit, eos = np.array([len(p) for p in prompts]), np.array([len(p) + new for p in prompts]), np.full(B, -1)
    R = min(128, B * (K + 1)) - (1 if K == 4 else 0)
    got, best, steps, penalised_extra = [[] for _ in range(B)], 0, 0, 0
    while (n_tok < limit).any():
        d = sp.reference_spec_draft(hist, n_tok, limit, K, 2, 4, R, max_len=ld)
        raw = np.zeros((R, V), F32)
        for r in range(R):
            b = int(d["row_slot"][r])
            if b >= 0:
                raw[r] = toy(list(hist[b, :n_tok[b]]) + list(d["tokens"][d["row0"][b] + 1:r + 1]))
        l = lg.reference_process(raw, d["row_slot"], d["row_ctr"], tokens=d["tokens"], row0=d["row0"], **st)
        plain = lg.reference_process(raw, d["row_slot"], d["row_ctr"], **st)
        penalised_extra += int((_bits(l) != _bits(plain)).any())
        drawn = np.zeros(R, np.int64)
        for r in range(R):
            if d["row_slot"][r] >= 0:
                drawn[r] = draw(l[r], int(d["row_slot"][r]), d["row_ctr"][r])
        a = sp.reference_spec_accept(d["tokens"], drawn, d["seq"], d["row0"], hist, n_tok, limit, eos, K)
        for b in range(B):
            out = a["out_tok"][b, :a["n_out"][b]].tolist()
            got[b] += out
            st["count"] = lg.reference_observe(st["count"], b, out) if out else st["count"]
        hist, n_tok, limit = a["hist"], a["n_tok"], a["limit"]
        best, steps = max(best, int(a["n_acc"].max())), steps + 1
        assert steps <= new
    assert got == want
    assert np.array_equal(st["count"], want_count)
    assert all(np.array_equal(st["count"][b], np.bincount(hist[b, :n_tok[b]], minlength=V)) for b in range(B)), "the invariant of §22.3"
    assert best >= min(K, 2) and steps < new, "no step accepted two drafts: the test shows nothing"
    assert penalised_extra > 0, "no extra ever changed a logit: the test shows nothing"


# ---------------------------------------------------------------------------------------------------------------- the C-ABI

@pytest.fixture(scope="module")
def lib():
    return qp._native.lib()


def test_logit_symbols_are_exported(lib):
    for name in ("qpal_logit_process", "qpal_logit_observe"):
        assert name in qp._native.exported_symbols() and hasattr(lib, name)
    for f in (qp.LogitProcessor, qp.reference_process, lg.process, lg.observe, lg.reference_observe):
        assert callable(f)
    with open(os.path.join(ROOT, "include", "qpal.h")) as f:
        hdr = f.read()
    assert "qpal_logit_process(" in hdr and "qpal_logit_observe(" in hdr


_PROC = dict(logits=1024, ld=4096, out=1 << 20, ld_out=4096, rows=4, vocab=4096, row_slot=16, ctr=16, slots=4, count=16, ld_count=4096,
             repetition=16, presence=16, frequency=16, mask=16, ld_mask=128, mask_on=16, bias_id=16, bias_val=16, bias_n=16, bias_slots=8,
             tokens=None, row0=None)
_OBS = dict(count=16, ld_count=4096, slots=4, vocab=4096, slot=16, slot0=0, tokens=16, active=16, n=8)


def _c_process(lib, **kw):
    return lib.qpal_logit_process(*{**_PROC, **kw}.values(), None)


def _c_observe(lib, **kw):
    return lib.qpal_logit_observe(*{**_OBS, **kw}.values(), None)


def test_logit_argument_errors_without_a_gpu(lib):
    """every argument error is returned before any stream work: the pointers below are never dereferenced"""
    for name in ("logits", "out", "row_slot", "ctr", "count", "repetition", "presence", "frequency", "mask", "mask_on", "bias_id", "bias_val",
                 "bias_n"):
        assert _c_process(lib, **{name: None}) == E_NULL, name
    assert _c_process(lib, tokens=16) == E_NULL and _c_process(lib, row0=16) == E_NULL, "tokens and row0 go together"
    for kw in ({"rows": 0}, {"rows": 129}, {"vocab": 0}, {"vocab": (1 << 30) + 1, "ld": 1 << 31, "ld_out": 1 << 31, "ld_count": 1 << 31,
                                                           "ld_mask": 1 << 26}, {"slots": 0}, {"slots": 129}, {"ld": 4095},
               {"ld_out": 4095}, {"ld_count": 4095}, {"ld_mask": 127}, {"bias_slots": -1}, {"bias_slots": 1025}):
        assert _c_process(lib, **kw) == E_SHAPE, kw
    for kw in ({"logits": 1026}, {"out": (1 << 20) + 1}, {"row_slot": 18}, {"ctr": 20}, {"count": 18}, {"repetition": 17}, {"presence": 18},
               {"frequency": 19}, {"mask": 18}, {"mask_on": 17}, {"bias_id": 18}, {"bias_val": 18}, {"bias_n": 17},
               {"tokens": 20, "row0": 16}, {"tokens": 16, "row0": 18}):
        assert _c_process(lib, **kw) == E_ALIGN, kw
    # in place is out == logits with one stride; rows that overlap in any other way would give a word two writers
    assert _c_process(lib, out=1024, ld_out=8192) == E_PARAM and _c_process(lib, out=1024 + 4096) == E_PARAM
    for name in ("count", "tokens"):
        assert _c_observe(lib, **{name: None}) == E_NULL, name
    for kw in ({"n": 0}, {"n": 2049}, {"vocab": 0}, {"slots": 0}, {"slots": 129}, {"ld_count": 4095}, {"slot": None, "slot0": 4},
               {"slot": None, "slot0": -1}):
        assert _c_observe(lib, **kw) == E_SHAPE, kw
    for kw in ({"count": 18}, {"slot": 18}, {"tokens": 20}, {"active": 20}):
        assert _c_observe(lib, **kw) == E_ALIGN, kw


# ---------------------------------------------------------------------------------------------------------------- the host side

def test_logit_processor_state_and_setters_reject_bad_input():
    E = qp._native.QpalError
    p = qp.LogitProcessor(3, 70, "cpu", bias_slots=4)
    assert p.count.shape == (3, 70) and p.count.dtype == torch.int32 and p.mask.shape == (3, 3) and p.bias_id.shape == (3, 4)
    assert p.repetition.tolist() == [1.0] * 3 and p.presence.tolist() == [0.0] * 3 and p.frequency.tolist() == [0.0] * 3
    assert p.mask_on.tolist() == [0] * 3 and p.bias_n.tolist() == [0] * 3 and p.count_prompt
    for kw in ({"repetition": 0.0}, {"repetition": -1.0}, {"repetition": float("inf")}, {"presence": float("nan")},
               {"frequency": float("-inf")}):
        with pytest.raises(E, match="finite"):
            p.set(1, **kw)
    with pytest.raises(E, match="slot"):
        p.set(3, presence=1.0)
    assert p.repetition.tolist() == [1.0] * 3, "a rejected call writes nothing"
    p.set(1, repetition=1.3, frequency=0.5)
    assert p.repetition[1] == np.float32(1.3) and p.frequency[1] == 0.5 and p.presence[1] == 0.0
    for bias, what in (({1: 1.0, 2: 1.0, 3: 1.0, 4: 1.0, 5: 1.0}, "entries"), ([(1, 1.0), (1, 2.0)], "twice"), ({70: 1.0}, "ids in"),
                       ({-1: 1.0}, "ids in"), ({1: float("nan")}, "finite"), ({1: float("inf")}, "finite")):
        with pytest.raises(E, match=what):
            p.set_bias(0, bias)
    assert int(p.bias_n[0]) == 0
    p.set_bias(0, {69: -2.0, 0: 4.0})
    assert int(p.bias_n[0]) == 2 and p.bias_id[0, :2].tolist() == [69, 0] and p.bias_val[0, :2].tolist() == [-2.0, 4.0]
    p.set_bias(0, None)
    assert int(p.bias_n[0]) == 0
    with pytest.raises(E, match="token ids"):
        p.set_mask(2, [70])
    with pytest.raises(E, match="bits"):
        p.set_mask(2, bits=np.zeros(2, np.uint32))
    p.set_mask(2, [0, 33, 69])
    assert int(p.mask_on[2]) == 1 and p.mask[2].tolist() == [1, 2, 32]
    p.set_mask(2, bits=np.array([0x80000000, 0, 0], np.uint32))
    assert p.mask[2].numpy().view(np.uint32).tolist() == [0x80000000, 0, 0]
    p.set_mask(2, None)
    assert int(p.mask_on[2]) == 0
    p.count[1, 5] = 3
    p.reset(1)
    assert int(p.count.sum()) == 0
    for kw in ({"B": 0}, {"B": 129}, {"vocab": 0}, {"bias_slots": 1025}):
        with pytest.raises(E):
            qp.LogitProcessor(**{**dict(B=2, vocab=8, device="cpu"), **kw})


class _Dummy:
    pass


def test_steps_check_the_processor_before_anything_else():
    """the processor's shape is checked against the step's slots / vocabulary, and a step without a logits tail refuses one"""
    check = qp.decoder._Rows._check_processor
    E = qp._native.QpalError
    embed, lm_head = torch.zeros(16, 8), torch.zeros(16, 8)
    p = qp.LogitProcessor(4, 16, "cpu")
    assert check("X", None, 4, embed, lm_head, False) is None and check("X", p, 4, embed, lm_head, True) is p
    with pytest.raises(E, match="sampler"):
        check("X", p, 4, embed, lm_head, False)
    for bad in (qp.LogitProcessor(3, 16, "cpu"), qp.LogitProcessor(4, 17, "cpu"), _Dummy()):
        with pytest.raises(E, match="LogitProcessor of 4 slots of 16"):
            check("X", bad, 4, embed, lm_head, True)
