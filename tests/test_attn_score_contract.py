"""CPU checks of the score-modifier contract: tests/score_reference.py is what it says it is — the batched float64
form is the row-by-row definition, no modifiers give attention_fp64, its kappa comes from the emulation over the cases the GPU
tests use — every seeded defect of the soft cap and the sinks lands >= 4x outside the tolerance at those sizes (the one that cannot
is named and covered another way), the census with sink = 0 sees a sink dropped or counted per chunk, every new QpalError is raised
before the library is reached, and the new entry points' return codes."""
import math

import numpy as np
import pytest
import torch

import attn_reference as ar
import qpalette_amd as qp
import score_reference as sr
import window_reference as wr
from attn_reference import F8, F16
from qpalette_amd._native import QpalError
from test_attn_exact import TEETH, _id
from test_window_contract import _case

CPU = torch.device("cpu")
DEC = ("decode", 2048, [2047], 0.0)        # the merged row of the GPU tests' decode launch
DEC40 = ("decode", 2048, [40], 0.0)        # its one-chunk row
PRE = ("prefill", 1024, list(range(900, 917)), sr.U_PREFILL)


def _seq(family, shape, L, dtype, pos, W, at=None):
    return _case(family, shape, L, dtype, pos, W, needle_at=at)


# ------------------------------------------------------------------------------------------------------------ the reference

@pytest.mark.parametrize("W", [None, 5, 100])
@pytest.mark.parametrize("cap,sk", [(None, "normal"), (8.0, None), (8.0, "near"), (50.0, "above")])
def test_batched_reference_is_the_row_by_row_definition(W, cap, sk):
    shape = nq, nkv, hd = (8, 2, 64)
    pos = list(range(90, 123))
    q16, K, V = _seq("peaked", shape, 128, F16, pos, W)
    scale = 1.0 / math.sqrt(hd)
    sinks = sr.make_sinks(sk, sr.row_max(q16, K, V, pos, W, nq, nkv, hd, scale, cap), nq)
    many = sr.score_fp64(q16, K, V, pos, W, nq, nkv, hd, scale, cap, sinks)
    for a, b in zip(many, sr.by_rows(sr.score_fp64, q16, K, V, pos, W, nq, nkv, hd, scale, cap, sinks)):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("W", [None, 33])
def test_no_cap_and_a_sink_of_minus_infinity_reproduce_attention_fp64(W):
    shape = nq, nkv, hd = (8, 2, 64)
    pos = list(range(100, 120))
    q16, K, V = _seq("ramp_up", shape, 128, F8, pos, W)
    scale = 1.0 / math.sqrt(hd)
    want = wr.sliced(ar.attention_fp64, q16, K, V, pos, W, nq, nkv, hd, scale)
    for sinks in (None, torch.full((nq,), float("-inf"))):
        for a, b in zip(sr.score_fp64(q16, K, V, pos, W, nq, nkv, hd, scale, None, sinks), want):
            assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    # and the emulation is attn_reference's where that one applies (no window: tiles from key 0)
    if W is None:
        for u_p in (0.0, sr.U_PREFILL):
            a = sr.emulate(q16, K, V, pos, None, nq, nkv, hd, scale, u_p, None, torch.full((nq,), float("-inf")), rounded=False)
            b = ar.emulate(q16, K, V, [p + 1 for p in pos], nq, nkv, hd, scale, u_p, rounded=False)
            assert torch.equal(a, b)


def test_the_fp32_tanh_form_is_within_a_few_ulp_of_one_and_saturates_cleanly():
    s = torch.cat((torch.linspace(-400.0, 400.0, 200001), torch.tensor([0.0, 1e-8, -1e-8, 3.0e38, -3.0e38, float("inf"), float("-inf")])))
    for cap in (2.0, 8.0, 50.0):
        got = sr.tanh_f32(s, cap).double()
        want = cap * torch.tanh(s.double() / cap)
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) <= cap
        assert float((got - want).abs().max()) <= 4 * 2.0 ** -24 * cap  # the absolute error the bound's cap term stands for


def test_census_expectation_with_a_sink_is_the_references():
    nq, nkv, hd = 2, 2, 64
    K, V = ar.census_cache(nkv, 600, hd, F16, CPU)
    q16 = torch.ones(40, nq * hd, dtype=F16)
    zero = torch.zeros(nq)
    for W in (None, 1, 5, 64, 300):
        pos = list(range(540, 580))
        exp, tol = sr.census_expected(pos, W, nq, hd, CPU)
        got = sr.score_fp64(q16, K, V, pos, W, nq, nkv, hd, 0.125, None, zero)[0]
        assert bool(((got - exp).abs() <= tol).all()), W
        assert bool(((sr.score_fp64(q16, K, V, pos, W, nq, nkv, hd, 0.125, 8.0, zero)[0] - exp).abs() <= tol).all()), W  # tanh(0) = 0


# -------------------------------------------------------------------------------------------------------------------- kappa

def test_emulation_sits_inside_the_bound():
    """kappa per u_p: four times the worst ratio of the emulation over the cases of the GPU tests, rounded up to a power of two
    (score_reference.KAPPA; the full table is in that file's header and DESIGN.md §32).  Decode in full; prefill and ragged on the
    first, middle and last row of every sequence."""
    worst, whole = sr.measure(lambda family, shape, L, dtype, pos, W, at: _seq(family, shape, L, dtype, pos, W, at),
                              rows_of=lambda T: sorted({0, T // 2, T - 1}))
    sr.print_table(worst, whole)
    assert whole <= 1.0
    for pre in (False, True):
        top = max(r for (f, u), r in worst.items() if u == pre)
        assert 4.0 * top <= sr.KAPPA[pre] < 16.0 * top, (pre, top, sr.KAPPA[pre])


# -------------------------------------------------------------------------------------------------------------------- teeth

def _excess(case, family, shape, cap, sk, mutate, dtype=F16, W=None):
    """how far outside the tolerance a seeded defect lands on a case of the GPU tests' sizes: max |defective - ref| / bound"""
    _, L, pos, u_p = case
    nq, nkv, hd = shape
    scale = 1.0 / math.sqrt(hd)
    q16, K, V = _seq(family, shape, L, dtype, pos, W)
    sinks = sr.make_sinks(sk, sr.row_max(q16, K, V, pos, W, nq, nkv, hd, scale, cap), nq)
    ref, A, Smax = sr.score_fp64(q16, K, V, pos, W, nq, nkv, hd, scale, cap, sinks)
    bad = sr.score_fp64(q16, K, V, pos, W, nq, nkv, hd, scale, cap, sinks, mutate=mutate)[0]
    return float(((bad - ref).abs() / sr.bound(ref, A, Smax, u_p, cap)).max())


# inputs on which the cap has teeth: peaked (score sd ~6) with cap 2 / 8, the ramps (range ~60) with cap 8 / 50, offset (scores near
# 2048 * scale) with cap 50, where tanh saturates
CAP_INPUTS = [("peaked", 2.0), ("peaked", 8.0), ("ramp_up", 8.0), ("ramp_up", 50.0), ("ramp_down", 8.0), ("ramp_down", 50.0), ("offset", 50.0)]


@pytest.mark.parametrize("shape", sr.SHAPES, ids=_id)
@pytest.mark.parametrize("case", [DEC, DEC40, PRE], ids=lambda c: f"{c[0]}{c[2][0]}")
def test_cap_defects_have_teeth(case, shape):
    for family, cap in CAP_INPUTS:
        assert _excess(case, family, shape, cap, None, ("cap_dropped",)) >= TEETH, (family, cap)
        if family != "offset":  # (offset: every raw q.k is far into the saturation with or without scale — both forms give ~cap)
            assert _excess(case, family, shape, cap, None, ("cap_before_scale",)) >= TEETH, (family, cap)
        if family in ("ramp_up", "offset"):  # (where the row's own key is among the best: under ramp_down it is the worst of all, and
            # under peaked it is wherever chance puts it — its weight is nothing either way)
            assert _excess(case, family, shape, cap, None, ("cap_not_on_new",)) >= TEETH, (family, cap)
    # (a sink near the capped maximum of ~50 is squashed to 50 tanh(1) = 38: with cap 2 or 8 under peaked scores the sink weighs too
    # little for that to show everywhere)
    assert _excess(case, "ramp_up", shape, 50.0, "near", ("cap_on_sink",)) >= TEETH


def decode_chunks(B, nkv, L, rel):
    """chunks a decode row with rel + 1 keys is cut into by a launch of B sequences on caches of L >= 512 positions whose scores fit
    one LDS chunk (csrc/attn_batch.hip: batch_geometry and the kernel's cld), and the chunk length"""
    want = min(-(-256 // (B * nkv)), 64)
    c = (-(-L // want) + 63) // 64 * 64
    ns = -(-L // c)
    cld = c
    if ns > 1:
        cld = min(max(((rel + ns) // ns + 63) // 64 * 64, 128), c)
    return rel // cld + 1, cld


def test_decode_chunks_of_the_gpu_cases():
    """B = 3 on 2048 positions: 32 chunks of 64 positions, so position 40 is finished by its only chunk and 2047 by a merge of 32;
    under a window of 700 the launch is sized for 700 positions: 11 chunks of 64"""
    for nkv in (1, 2):
        assert decode_chunks(3, nkv, 2048, 2047) == (32, 64) and decode_chunks(3, nkv, 2048, 40) == (1, 64)
        assert decode_chunks(3, nkv, 2048, 63)[0] == 1 and decode_chunks(3, nkv, 2048, 64)[0] == 2 and decode_chunks(3, nkv, 2048, 511)[0] == 8
        assert decode_chunks(3, nkv, 700, 699) == (11, 64)


@pytest.mark.parametrize("shape", sr.SHAPES, ids=_id)
@pytest.mark.parametrize("case", [DEC, DEC40, PRE], ids=lambda c: f"{c[0]}{c[2][0]}")
def test_sink_defects_have_teeth(case, shape):
    """with a sink that competes with the row's best keys ("near"); N(0, 2) sinks under scores of standard deviation 6 weigh nothing,
    and 40 above / below leave nothing to see (the output is 0, or the sink is)"""
    kind, L, pos, _ = case
    nkv = shape[1]
    if kind == "decode":
        chunks, clen = decode_chunks(3, nkv, L, pos[0])
        counts = [chunks] if chunks > 1 else []
        counts.append(-(-(pos[0] + 1) // 32))  # once per 32-key tile
    else:
        counts, clen = [-(-(pos[0] + 1) // 128), -(-(pos[0] + 1) // 32)], 128  # chunks of kPfMinChunk keys, tiles
    defects = [("sink_dropped",), ("sink_value_row",), ("sink_head", "div_rep"), ("sink_head", "plus1"), ("sink_before_merge", clen)]
    defects += [("sink_times", n) for n in counts]
    for family, cap in (("peaked", None), ("ramp_down", None), ("ramp_up", 50.0)):
        for mutate in defects:
            if mutate[0] == "sink_before_merge" and family != "ramp_down":
                continue  # (visible where the last chunk's maximum lies below the row's: scores that fall towards the new key)
            assert _excess(case, family, shape, cap, "near", mutate) >= TEETH, (family, cap, mutate)
    # a sink 40 above everything: dropping it is the whole output
    assert _excess(case, "peaked", shape, None, "above", ("sink_dropped",)) >= 1e4


def test_a_maximum_taken_without_the_sink_overflows_in_fp32_and_the_stable_form_does_not():
    """The defect 'M taken without the sink' cannot be made visible in the OUTPUT: e^(sink - max s) overflows to inf at sink - max s >=
    89, the quotient is then num / inf = 0, and the true result is below 1e-38 there; short of the overflow the two forms are the
    same number.  What it does show is inf in the denominator (and NaN wherever that term is normalised, inf / inf): covered here,
    and on the GPU by the needle test with a sink far above every score (no inf or NaN may come out)."""
    shape = nq, nkv, hd = (8, 1, 64)
    kind, L, pos, u_p = DEC
    scale = 1.0 / math.sqrt(hd)
    q16, K, V = _seq("peaked", shape, L, F16, pos, None)
    rm = sr.row_max(q16, K, V, pos, None, nq, nkv, hd, scale)
    for gap in (90.0, 200.0, 3000.0):
        sinks = (rm.amax(0) + gap).float()
        term = sr.unstable_sink_term(rm, sinks)
        assert bool(torch.isinf(term).all()) and bool(torch.isnan(term / (1.0 + term)).all())
        for u in (0.0, sr.U_PREFILL):
            out = sr.emulate(q16, K, V, pos, None, nq, nkv, hd, scale, u, None, sinks, rounded=False)
            assert bool(torch.isfinite(out).all()) and float(out.abs().max()) < 1e-30
            ref, A, Smax = sr.score_fp64(q16, K, V, pos, None, nq, nkv, hd, scale, None, sinks)
            assert bool(((out.double() - ref).abs() <= sr.bound(ref, A, Smax, u)).all())


@pytest.mark.parametrize("hd", [64, 128, 256])
def test_census_catches_a_sink_dropped_or_counted_per_chunk(hd):
    """the GPU census: sink = 0 under K = 0, so the row's weight is 1 / (n + 1); a dropped sink gives 1 / n, one per chunk 1 / (n +
    chunks) or per tile — at least 4 ulp away at every position and window of the GPU test, but for the dropped sink on rows of
    512 keys and more"""
    nq = 2
    for W in (None, 1, 5, 64, 300):
        for p in (0, 1, 63, 64, 127, 128, 511, 512, 2047):
            n = p + 1 - wr.lo(p, W)
            chunks = decode_chunks(3, 1, 2048, p - wr.lo(p, W))[0] if (W is None or W >= 512) else 1
            exp, tol = sr.census_expected([p], W, nq, hd, CPU)
            wrong = [0] + ([chunks] if chunks > 1 else []) + ([-(-n // 32)] if n > 32 else [])
            for count in wrong:
                bad = sr.census_expected([p], W, nq, hd, CPU, sink_count=count)[0]
                seen = float(((bad - exp).abs() / tol).max())
                if count > 0 or n <= 256:
                    assert seen >= TEETH, (W, p, count, seen)
                else:  # (a dropped sink under more keys: 1 / n against 1 / (n + 1) shrinks to one ulp at 2048 — the short rows see it)
                    assert seen > 0.0, (W, p, count, seen)


# -------------------------------------------------------------------------------------------------------- the whole model

def test_the_models_modifiers_bite(monkeypatch):
    """the cap, the sinks and the scale test_attn_score_model.py runs its two-layer model with: dropping the caps, the sinks or the
    scale each moves the last layer's stream at least 4 tolerances (model_reference.tolerance of the patched emulation) in every slot"""
    import model_reference as mr
    import test_attn_score_model as tm
    from test_window_model import CHUNK, NL, _tokens

    spec = mr.build_spec("S", "mixed", NL, mr.VOCAB, 0)
    toks, sinks = _tokens(), tm.model_sinks(CPU)
    for prefill in (False, True):
        ref, emu = tm.refs(monkeypatch, spec.ref, toks, CPU, prefill, sinks=sinks)
        for name, mods in (("caps", dict(sinks=sinks, caps=(None, None))), ("sinks", dict(sinks=None)), ("scale", dict(sinks=sinks, scale=0.125))):
            bad = tm.refs(monkeypatch, spec.ref, toks, CPU, prefill, **mods)[0]
            seen = [float((mr.e_h(bad.stream[b][-1], ref.stream[b][-1]) / mr.tolerance(mr.e_h(emu.stream[b][-1], ref.stream[b][-1]))).max())
                    for b in range(len(toks))]
            print(f"{name} dropped, prefill={prefill}: the stream moves {min(seen):.0f} .. {max(seen):.0f} tolerances")
            assert min(seen) >= TEETH, (name, prefill, seen)


# ------------------------------------------------------------------------------------------------- errors and return codes

def test_every_new_error_is_raised_before_the_library_is_reached(monkeypatch):
    def no_lib():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(qp._native, "lib", no_lib)
    x = None
    launches = [lambda **kw: qp.decode_attention(x, x, x, x, x, x, x, **kw),
                lambda **kw: qp.prefill_attention(x, x, x, x, x, x, x, **kw),
                lambda **kw: qp.paged_decode_attention(x, x, x, x, x, x, x, x, **kw),
                lambda **kw: qp.paged_prefill_attention(x, x, x, x, x, x, x, x, **kw),
                lambda **kw: qp.ragged_prefill_attention(x, x, x, x, x, x, x, x, x, **kw),
                lambda **kw: qp.paged_ragged_prefill_attention(x, x, x, x, x, x, x, x, x, x, **kw)]
    for launch in launches:
        for bad in (0, 0.0, -1, -1.0, float("nan"), float("inf"), 1e39, True, "8"):
            with pytest.raises(QpalError, match="softcap"):
                launch(softcap=bad)
        for bad in ([0.0] * 8, 1.0, np.zeros(8, dtype=np.float32)):
            with pytest.raises(QpalError, match="sinks"):
                launch(sinks=bad)
    for kw in ({"softcap": 8.0}, {"sinks": torch.zeros(8)}):
        with pytest.raises(QpalError, match="shared-prefix"):
            qp.shared_prefix_decode_attention(x, x, x, x, x, x, x, x, x, **kw)
    # the tensor's checks, where nq is known: dtype, length, layout, alignment
    dev = torch.device("cpu")
    for bad in (torch.zeros(8, dtype=torch.float64), torch.zeros(8, dtype=torch.float16), torch.zeros(7), torch.zeros(9), torch.zeros(1, 8),
                torch.zeros(16)[::2]):
        with pytest.raises(QpalError, match="sinks"):
            qp.attention._score_args("decode_attention", (None, bad), 8, dev)
    with pytest.raises(QpalError, match="sinks"):
        qp.attention._score_args("decode_attention", (None, torch.zeros(8, device="meta")), 8, dev)
    # (torch makes no fp32 tensor off a 4-byte boundary; the C entry points' QPAL_E_ALIGN is checked below, in front of any launch)
    assert qp.attention._score_args("x", (None, None), 8, dev) == (0.0, None) and qp.attention._score_args("x", (8, None), 8, dev)[0] == 8
    # the step classes
    class _L:
        class self_attn:
            num_heads = 8
    layers = [_L, _L]
    check = qp.decoder._Rows._check_score
    assert check("Prefill", None, None, layers, dev) == ([None, None], None)
    assert check("Prefill", 8, None, layers, dev)[0] == [8.0, 8.0] and check("Prefill", (None, 50.0), None, layers, dev)[0] == [None, 50.0]
    for bad in (0, -1.0, float("nan"), float("inf"), (8.0,), (8.0, 8.0, 8.0), (8.0, -1.0), "8", [None]):
        with pytest.raises(QpalError, match="softcap"):
            check("Prefill", bad, None, layers, dev)
    ok = torch.zeros(2, 8)
    assert check("Prefill", None, ok, layers, dev)[1] is ok
    for bad in (torch.zeros(8), torch.zeros(2, 7), torch.zeros(3, 8), torch.zeros(2, 8, dtype=torch.float64), torch.zeros(2, 16)[:, ::2], [0.0] * 16):
        with pytest.raises(QpalError, match="sinks"):
            check("Prefill", None, bad, layers, dev)
    tok = torch.zeros(2, dtype=torch.int64)
    for kw in ({"softcap": 8.0}, {"sinks": ok}):
        with pytest.raises(QpalError, match="shared_prefix with softcap"):
            qp.DecodeStep([x, x], x, x, x, x, x, x, tok, tok, tok, block_table=torch.zeros(2, 4, dtype=torch.int32), shared_prefix=object(), **kw)


def test_score_entry_points_return_codes():
    lib = qp._native.lib()
    buf = np.zeros(1 << 16, dtype=np.uint8)
    p = buf.ctypes.data
    assert p % 4 == 0
    dec = lambda q, table, window, cap, sinks, L=128, fmt=0: lib.qpal_attn_rope_decode_batch_score(  # noqa: E731
        q, p, p, 512, p, p, p, 512, p, p, table, 8, 4, 16, 8, fmt, 1, 8, 8, 64, L, 0.125, window, cap, sinks, None, 0, None)
    pre = lambda q, row, window, cap, sinks, L=128, fmt=0: lib.qpal_attn_rope_prefill_score(  # noqa: E731
        q, p, p, 512, p, p, p, 512, p, p, row, 4, 16, 8, fmt, 1, 8, 8, 64, L, 0.125, window, cap, sinks, None, 0, None)
    rag = lambda q, table, window, cap, sinks, L=128, fmt=0: lib.qpal_attn_rope_prefill_ragged_score(  # noqa: E731
        q, p, p, 512, p, p, p, 512, p, p, p, p, table, 8, 4, 16, 8, fmt, 1, 1, 1, 8, 8, 64, L, 0.125, window, cap, sinks, None, 0, None)
    for fn in (dec, pre, rag):
        for table in (None, p):
            assert fn(None, table, 4, 8.0, p) == -3 and fn(None, table, -1, -1.0, p) == -3  # a null pointer: QPAL_E_NULL, first
            for cap in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):             # a bad cap: QPAL_E_PARAM, before any other check
                assert fn(p, table, 4, cap, None) == -2 and fn(p, table, 0, cap, p, L=130, fmt=7) == -2
            assert fn(p, table, -1, 8.0, None) == -2 and fn(p, table, -1, 0.0, None) == -2    # and the window's
            for cap, sinks in ((8.0, None), (0.0, p), (8.0, p), (0.0, None)):
                assert fn(p, table, 4, cap, sinks, fmt=2) == -1                               # then the siblings' checks
                assert fn(p, table, 0, cap, sinks, fmt=2) == -1
            assert fn(p, table, 0, 0.0, p + 2) == -4 and fn(p, table, 4, 8.0, p + 1) == -4    # sinks off a 4-byte boundary: QPAL_E_ALIGN
        for cap, sinks in ((8.0, None), (0.0, p), (0.0, None)):
            assert fn(p, None, 4, cap, sinks, L=130) == -1 and fn(p, None, 0, cap, sinks, L=130) == -1  # max_len % 4 (contiguous)
