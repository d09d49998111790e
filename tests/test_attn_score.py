"""Attention score modifiers on the GPU: softcap= and sinks= on batched decode, prefill and ragged prefill, fp16 and
e4m3 caches, contiguous and paged, with and without a window, against tests/score_reference.py — the census with a sink of 0 (the
output counts the keys AND the sink: a sink dropped or counted once per chunk shows), the input families inside the float64 bound,
needles under a cap and under a sink far above every score, and the bit-for-bit rules of the contract: a sink of -inf is the launch
without sinks, no modifiers is the existing entry point, paged = contiguous, a ragged segment = the one-sequence launch, the stored
bytes do not change."""
import pytest
import torch

import attn_reference as ar
import qpalette_amd as qp
import score_reference as sr
import window_reference as wr
from attn_reference import F8, F16
from qpalette_amd._native import QpalError
from test_attn_exact import _id, _qkv, _rotated_q, _stack
from test_window import WProblem, _bits, _nan_mask, _page_out

SHAPES, DTYPES = sr.SHAPES, sr.DTYPES
_WORST = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _report(kernels, family, worst, what):
    key = (kernels, family)
    _WORST[key] = max(_WORST.get(key, 0.0), worst)
    print(f"{kernels} {family} {what}: worst err/tol = {worst:.3f} (so far over {kernels} {family}: {_WORST[key]:.3f})")
    assert worst <= 1.0, (kernels, family, what, worst)


def _ratio(out, exp, tol):
    return float(torch.nan_to_num((out.double() - exp).abs() / tol, nan=float("inf")).max())


# ------------------------------------------------------------------------------------------------------------------ launches

def _decode(dev, shape, L, probs, W, cap=None, sinks=None, pos=None, **kw):
    """decode_attention on one-row problems, each a sequence of its own (fresh copies of their caches): out and the caches behind it"""
    nq, nkv, hd = shape
    B = len(probs)
    kc, vc = _stack([p.kc for p in probs]), _stack([p.vc for p in probs])
    q, k, v = _qkv(*(torch.cat([getattr(p, a) for p in probs]) for a in ("q32", "k32", "v32")))
    pos_t = torch.tensor([p.pos0 for p in probs] if pos is None else pos, dtype=torch.long, device=dev)
    out = torch.full((B, nq * hd), float("nan"), dtype=F16, device=dev)
    qp.decode_attention(q, k, v, kc, vc, pos_t, probs[0].inv, out=out, ws=qp.attention_workspace(B, nq, nkv, hd, L, dev), window=W,
                        softcap=cap, sinks=sinks, **kw)
    torch.cuda.synchronize()
    return out, kc, vc


def _prefill(prob, W, cap=None, sinks=None):
    """prefill_attention on a fresh copy of the problem's cache"""
    nq, nkv, hd = prob.shape
    kc, vc = prob.kc.clone(), prob.vc.clone()
    out = torch.full((prob.T, nq * hd), float("nan"), dtype=F16, device=prob.dev)
    pos_t = torch.tensor([prob.pos0], dtype=torch.long, device=prob.dev)
    qp.prefill_attention(*_qkv(prob.q32, prob.k32, prob.v32), kc, vc, pos_t, prob.inv, out=out,
                         ws=qp.prefill_workspace(prob.T, nq, nkv, hd, prob.L, prob.dev), window=W, softcap=cap, sinks=sinks)
    torch.cuda.synchronize()
    return out, kc, vc


def _ragged(dev, shape, L, probs, W, cap=None, sinks=None):
    """ragged_prefill_attention: segment s is problem s, in slot (s + 1) % S; returns the per-segment outputs and the caches [S, ...]"""
    nq, nkv, hd = shape
    S = len(probs)
    slots = [(s + 1) % S for s in range(S)]
    order = sorted(range(S), key=lambda s: slots[s])
    kc, vc = _stack([probs[s].kc for s in order]), _stack([probs[s].vc for s in order])
    q, k, v = _qkv(*(torch.cat([getattr(p, a) for p in probs]) for a in ("q32", "k32", "v32")))
    row0 = [0]
    for p in probs:
        row0.append(row0[-1] + p.T)
    R = row0[-1]
    out = torch.full((R, nq * hd), float("nan"), dtype=F16, device=dev)
    qp.ragged_prefill_attention(q, k, v, kc, vc, torch.tensor(slots, dtype=torch.int32, device=dev),
                                torch.tensor(row0, dtype=torch.int32, device=dev),
                                torch.tensor([p.pos0 for p in probs], dtype=torch.int64, device=dev), probs[0].inv, out=out,
                                ws=qp.ragged_workspace(R, S, nq, nkv, hd, L, dev), window=W, softcap=cap, sinks=sinks)
    torch.cuda.synchronize()
    return [out[row0[s]:row0[s + 1]] for s in range(S)], [kc[slots[s]] for s in range(S)], [vc[slots[s]] for s in range(S)]


def _run(kind, dev, shape, L, probs, W, cap=None, sinks=None):
    """the launches of `kind` over its sequences: per sequence (out, kc, vc) as the launch left them"""
    if kind == "decode":
        out, kc, vc = _decode(dev, shape, L, probs, W, cap, sinks)
        return [(out[b:b + 1], kc[b], vc[b]) for b in range(len(probs))]
    if kind == "prefill":
        return [_prefill(p, W, cap, sinks) for p in probs]
    return list(zip(*_ragged(dev, shape, L, probs, W, cap, sinks)))


def _problems(kind, dev, shape, dtype, family, W, seed=700, nan_below=True):
    L = sr.launch_shape(kind)[0]
    return [WProblem(dev, shape, L, dtype, family, pos0, T, W, seed + i, needle_at=sr.needle_at(pos0, W) if family == "needle" else None,
                     nan_below=nan_below) for i, (T, pos0) in enumerate(sr.sequences(kind))]


def _row_maxima(probs, filled, W, cap):
    nq, nkv, hd = probs[0].shape
    return torch.cat([sr.row_max(p.q16, kc, vc, p.pos, W, nq, nkv, hd, p.scale, cap) for p, (_, kc, vc) in zip(probs, filled)])


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# -------------------------------------------------------------------------------------------------------------------- census

CENSUS_POS = [0, 1, 63, 64, 127, 128, 511, 512, 2047]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_decode_census_with_a_sink_of_zero(dev, shape, dtype):
    """K = 0, V[j] = e_(j mod hd), sink = 0: out = count_d / (n + 1).  2048 rows: the split launch (position 0 .. 63: one chunk,
    beyond: a merge of up to 32), B = 3 with one inactive slot; without a window and under windows of 1, 5, 64 and 300 keys, with
    NaN in every row below the floor.  A sink per chunk would give n + chunks, a dropped one n.  A cap changes nothing: tanh(0) = 0."""
    nq, nkv, hd = shape
    L, B = 2048, 3
    K1, V1 = ar.census_cache(nkv, L, hd, dtype, dev)
    ws = qp.attention_workspace(B, nq, nkv, hd, L, dev)
    inv = ar.inv_freq(hd, dev)
    q = ar.query_targets(B, nq, nkv, hd, 3, dev)
    k = torch.zeros(B, nkv * hd, device=dev)
    j = torch.arange(L, device=dev)[None, :]
    zero = torch.zeros(nq, device=dev)
    for W, cap in ((None, None), (1, None), (5, 8.0), (64, None), (300, 50.0), (None, 8.0)):
        outs, positions = [], []
        for i in range(0, len(CENSUS_POS), 2):
            pos = [CENSUS_POS[i], -1] + CENSUS_POS[i + 1:i + 2]  # (the middle slot is inactive)
            pos += [-1] * (B - len(pos))
            pos_t = torch.tensor(pos, dtype=torch.long, device=dev)
            kc, vc = _stack([K1] * B), _stack([V1] * B)
            low = qp.window_floor(pos_t, W)
            mask = ((j < low[:, None]) | (j == pos_t[:, None])) & (pos_t >= 0)[:, None]
            _nan_mask(kc, mask)
            _nan_mask(vc, mask)
            out = torch.full((B, nq * hd), float("nan"), dtype=F16, device=dev)
            qp.decode_attention(*_qkv(q, k, ar.census_new_v(pos_t, nkv, hd, dev)), kc, vc, pos_t, inv, out=out, ws=ws, window=W, softcap=cap,
                                sinks=zero)
            act = pos_t >= 0
            assert bool(torch.isnan(out[~act]).all())  # an inactive slot's row is not written
            outs.append(out[act])
            positions += [p for p in pos if p >= 0]
        exp, tol = sr.census_expected(positions, W, nq, hd, dev)
        _report("decode_attention", "census", _ratio(torch.cat(outs), exp, tol), f"{_id(shape)} {_id(dtype)} L={L} B={B} W={W} cap={cap}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_prefill_and_ragged_census_with_a_sink_of_zero(dev, shape, dtype):
    """T in {1, 17, 128} at pos0 in {0, 31, 500} on a 1024-row cache (one chunk, and merged chunks from 500 on), then the three as
    segments of unequal length of one ragged launch; with and without a window"""
    nq, nkv, hd = shape
    L = 1024
    zero = torch.zeros(nq, device=dev)
    for W in (None, 64):
        for T in (1, 17, 128):
            for pos0 in (0, 31, 500):
                prob = WProblem(dev, shape, L, dtype, "census", pos0, T, W, 0)
                exp, tol = sr.census_expected(prob.pos, W, nq, hd, dev)
                _report("prefill_attention", "census", _ratio(_prefill(prob, W, None, zero)[0], exp, tol),
                        f"{_id(shape)} {_id(dtype)} T={T} pos0={pos0} W={W}")
        probs = [WProblem(dev, shape, L, dtype, "census", pos0, T, W, 0) for T, pos0 in ((1, 0), (17, 31), (100, 500))]
        outs = _ragged(dev, shape, L, probs, W, 8.0, zero)[0]
        for p, out in zip(probs, outs):
            exp, tol = sr.census_expected(p.pos, W, nq, hd, dev)
            _report("ragged_prefill_attention", "census", _ratio(out, exp, tol), f"{_id(shape)} {_id(dtype)} T={p.T} pos0={p.pos0} W={W}")


# ------------------------------------------------------------------------------------------------------------------ families

@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
@pytest.mark.parametrize("kind", ["decode", "prefill", "ragged"])
def test_families_within_the_bound(dev, kind, shape, dtype):
    """score_reference.measure()'s cases: every family x cap x sinks x with and without a window, NaN below every floor.  The plain
    launch fills the caches the float64 reference reads (the stored bytes do not depend on the modifiers: asserted for every one)."""
    nq, nkv, hd = shape
    L, windows, u_p = sr.launch_shape(kind)
    worst = {}
    for family in ar.FAMILIES:
        for W in windows:
            probs = _problems(kind, dev, shape, dtype, family, W)
            filled = _run(kind, dev, shape, L, probs, W)
            groups = [[i] for i in range(len(probs))] if kind == "prefill" else [list(range(len(probs)))]
            for cap in sr.CAPS:
                for group in groups:
                    rm = _row_maxima([probs[i] for i in group], [filled[i] for i in group], W, cap)
                    for sk in sr.SINK_KINDS:
                        sinks = sr.make_sinks(sk, rm, nq)
                        got = _run(kind, dev, shape, L, [probs[i] for i in group], W, cap, sinks)
                        for i, (out, kc, vc) in zip(group, got):
                            assert _same((kc, vc), filled[i][1:]), (family, W, cap, sk)
                            ref, A, Smax = sr.score_fp64(probs[i].q16, kc, vc, probs[i].pos, W, nq, nkv, hd, probs[i].scale, cap, sinks)
                            r = _ratio(out, ref, sr.bound(ref, A, Smax, u_p, cap))
                            worst[family] = max(worst.get(family, 0.0), r)
                            assert r <= 1.0, (kind, family, W, cap, sk, i, r)
                            if sk == "above":
                                assert float(out.float().abs().max()) <= 2.0 ** -24  # 40 above every score: the row is (fp16) zero
    for family, r in worst.items():
        _report(f"{kind}_attention", family, r, f"{_id(shape)} {_id(dtype)}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
@pytest.mark.parametrize("kind", ["decode", "prefill", "ragged"])
def test_needles_under_a_cap_and_under_a_dominant_sink(dev, kind, shape, dtype):
    """cap = 8: a needle 30 above the rest is squashed to within 8 of it — its weight follows the float64 reference and is not 1
    (the uncapped launch returns the needle's v).  A sink 30, 90 and 3000 above every score: the output is within the bound of ~0
    with no inf and no NaN (a maximum taken without the sink overflows from 89 on)."""
    nq, nkv, hd = shape
    L, windows, u_p = sr.launch_shape(kind)
    for W in windows:
        probs = _problems(kind, dev, shape, dtype, "needle", W)
        plain = _run(kind, dev, shape, L, probs, W)
        capped = _run(kind, dev, shape, L, probs, W, 8.0, None)
        for p, (o0, kc, vc), (o8, _, _) in zip(probs, plain, capped):
            at = sr.needle_at(p.pos0, W)
            v_needle = vc[:, at].float().repeat_interleave(nq // nkv, dim=0).reshape(1, nq * hd)
            assert float((o0.float() - v_needle).abs().max()) <= 2.0 ** -6  # uncapped: weight 1 (to fp16)
            ref, A, Smax = sr.score_fp64(p.q16, kc, vc, p.pos, W, nq, nkv, hd, p.scale, 8.0, None)
            assert _ratio(o8, ref, sr.bound(ref, A, Smax, u_p, 8.0)) <= 1.0
            if len(p.pos) + p.pos0 - wr.lo(p.pos0, W) > 64:  # (among more than a few keys the squashed needle no longer dominates)
                assert float((ref - v_needle.double()).abs().max()) > 0.25 and float((o8.float() - v_needle).abs().max()) > 0.25
        rm = _row_maxima(probs, plain, W, None)
        for gap in (30.0, 90.0, 3000.0):
            sinks = (rm.amax(0) + gap).float()
            for p, (out, kc, vc) in zip(probs, _run(kind, dev, shape, L, probs, W, None, sinks)):
                assert bool(torch.isfinite(out).all())
                ref, A, Smax = sr.score_fp64(p.q16, kc, vc, p.pos, W, nq, nkv, hd, p.scale, None, sinks)
                assert _ratio(out, ref, sr.bound(ref, A, Smax, u_p)) <= 1.0 and float(out.float().abs().max()) <= 2.0 ** -20, gap


# --------------------------------------------------------------------------------------------------------- bit-for-bit rules

@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
@pytest.mark.parametrize("kind", ["decode", "prefill", "ragged"])
def test_a_sink_of_minus_infinity_is_the_launch_without_sinks(dev, kind, shape, dtype):
    """outputs and cache bytes, every family, with and without a window, under a cap of 8 and of 50: both sides run the new
    instantiation, as the contract says.  Without a cap the other side is the EXISTING instantiation (softcap=None, sinks=None is the
    existing entry point), another piece of compiled code: the cache bytes are still equal, and both outputs lie inside the bound
    of the one float64 result (they are bit for bit equal on every shape here but the (8, 2, 128) prefill body, where a score that
    differs in its last bit rounds an fp16 weight the other way)."""
    nq, nkv, hd = shape
    L, windows, u_p = sr.launch_shape(kind)
    none = torch.full((nq,), float("-inf"), device=dev)
    for family in ar.FAMILIES:
        for W in windows:
            probs = _problems(kind, dev, shape, dtype, family, W)
            for cap in (8.0, 50.0, None):
                a, b = _run(kind, dev, shape, L, probs, W, cap, None), _run(kind, dev, shape, L, probs, W, cap, none)
                for x, y in zip(a, b):
                    assert not bool(torch.isnan(x[0]).any()) and _same(x[1:], y[1:]), (family, W, cap)
                    if cap is not None:
                        assert torch.equal(_bits(x[0]), _bits(y[0])), (family, W, cap)
                if cap is None:
                    for p, x, y in zip(probs, a, b):
                        ref, A, Smax = sr.score_fp64(p.q16, x[1], x[2], p.pos, W, nq, nkv, hd, p.scale)
                        tol = sr.bound(ref, A, Smax, u_p)
                        assert _ratio(x[0], ref, tol) <= 1.0 and _ratio(y[0], ref, tol) <= 1.0, (family, W)


def _raw_call(entry, args, dev):
    with torch.cuda.device(dev):
        rc = getattr(qp._native.lib(), entry)(*args, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, (entry, rc)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_no_modifiers_is_the_existing_entry_point(dev, shape, dtype):
    """softcap=None, sinks=None: the Python launches are the calls without the keywords, and the _score entry points with softcap
    = 0 and sinks = NULL launch what the existing ones launch — bit for bit, outputs and caches, with and without a window"""
    nq, nkv, hd = shape
    fmt = 0 if dtype == F16 else 1
    for W in (None, 300):
        # decode
        L = sr.DECODE_L
        probs = _problems("decode", dev, shape, dtype, "peaked", W)
        want = _decode(dev, shape, L, probs, W)
        B = len(probs)
        kc, vc = _stack([p.kc for p in probs]), _stack([p.vc for p in probs])
        q, k, v = _qkv(*(torch.cat([getattr(p, a) for p in probs]) for a in ("q32", "k32", "v32")))
        pos_t = torch.tensor([p.pos0 for p in probs], dtype=torch.long, device=dev)
        out = torch.full((B, nq * hd), float("nan"), dtype=F16, device=dev)
        ws = qp.attention_workspace(B, nq, nkv, hd, L, dev)
        _raw_call("qpal_attn_rope_decode_batch_score",
                  (q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), out.stride(0),
                   pos_t.data_ptr(), probs[0].inv.data_ptr(), None, 0, 0, 0, 0, fmt, B, nq, nkv, hd, L, probs[0].scale, W or 0, 0.0, None,
                   ws.data_ptr(), ws.numel() * 4), dev)
        assert not bool(torch.isnan(out).any()) and _same((out, kc, vc), want), W
        # prefill
        L = sr.PREFILL_L
        for p in _problems("prefill", dev, shape, dtype, "peaked", W):
            want = _prefill(p, W)
            kc, vc = p.kc.clone(), p.vc.clone()
            q, k, v = _qkv(p.q32, p.k32, p.v32)
            out = torch.full((p.T, nq * hd), float("nan"), dtype=F16, device=dev)
            pos_t = torch.tensor([p.pos0], dtype=torch.long, device=dev)
            ws = qp.prefill_workspace(p.T, nq, nkv, hd, L, dev)
            _raw_call("qpal_attn_rope_prefill_score",
                      (q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), out.stride(0),
                       pos_t.data_ptr(), p.inv.data_ptr(), None, 0, 0, 0, fmt, p.T, nq, nkv, hd, L, p.scale, W or 0, 0.0, None,
                       None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel() * 4), dev)
            assert not bool(torch.isnan(out).any()) and _same((out, kc, vc), want), (W, p.T)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_storage_and_segments_carry_over(dev, shape, dtype):
    """with both modifiers, with and without a window: paged (page 16) = contiguous on the gathered cache, a ragged segment = the
    one-sequence launch, and the cache after a modified prefill = the cache after the plain one — all bit for bit"""
    nq, nkv, hd = shape
    cap = 8.0
    for W in (None, 600):
        # prefill: the stored bytes, then paged = contiguous
        L = sr.PREFILL_L
        probs = _problems("ragged", dev, shape, dtype, "peaked", W, nan_below=False)
        plain = _run("prefill", dev, shape, L, probs, W)
        rm = _row_maxima(probs, plain, W, cap)
        sinks = sr.make_sinks("near", rm, nq)
        mod = _run("prefill", dev, shape, L, probs, W, cap, sinks)
        for p, a, b in zip(probs, plain, mod):
            assert _same(a[1:], b[1:]) and not torch.equal(_bits(a[0]), _bits(b[0])) and not bool(torch.isnan(b[0]).any())
            cache = qp.PagedKVCache(1, L // 16, nkv, 16, hd, 1, L // 16, dtype=dtype, device=dev)
            _page_out(cache, (p.kc[None], p.vc[None]), dev)
            out = torch.full((p.T, nq * hd), float("nan"), dtype=F16, device=dev)
            qp.paged_prefill_attention(*_qkv(p.q32, p.k32, p.v32), cache.kpool[0], cache.vpool[0], cache.table[0],
                                       torch.tensor([p.pos0], dtype=torch.long, device=dev), p.inv, out=out,
                                       ws=qp.prefill_workspace(p.T, nq, nkv, hd, L, dev), window=W, softcap=cap, sinks=sinks)
            torch.cuda.synchronize()
            assert torch.equal(_bits(out), _bits(b[0]))
            for n in p.pos:
                pg = cache.pages_of(0)[n // 16]
                assert torch.equal(_bits(cache.kpool[0][pg, :, n % 16]), _bits(b[1][:, n])) and torch.equal(_bits(cache.vpool[0][pg, :, n % 16]), _bits(b[2][:, n]))
        # a ragged segment = the one-sequence launch (and its paged form = the contiguous one)
        outs, kcs, vcs = _ragged(dev, shape, L, probs, W, cap, sinks)
        for s, b in enumerate(mod):
            assert _same((outs[s], kcs[s], vcs[s]), b), s
        S = len(probs)
        slots = [(s + 1) % S for s in range(S)]
        order = sorted(range(S), key=lambda s: slots[s])
        cache = qp.PagedKVCache(1, S * L // 16, nkv, 16, hd, S, L // 16, dtype=dtype, device=dev)
        _page_out(cache, (_stack([probs[s].kc for s in order]), _stack([probs[s].vc for s in order])), dev)
        q, k, v = _qkv(*(torch.cat([getattr(p, a) for p in probs]) for a in ("q32", "k32", "v32")))
        row0 = [0]
        for p in probs:
            row0.append(row0[-1] + p.T)
        out = torch.full((row0[-1], nq * hd), float("nan"), dtype=F16, device=dev)
        qp.paged_ragged_prefill_attention(q, k, v, cache.kpool[0], cache.vpool[0], cache.table, torch.tensor(slots, dtype=torch.int32, device=dev),
                                          torch.tensor(row0, dtype=torch.int32, device=dev),
                                          torch.tensor([p.pos0 for p in probs], dtype=torch.int64, device=dev), probs[0].inv, out=out,
                                          ws=qp.ragged_workspace(row0[-1], S, nq, nkv, hd, L, dev), window=W, softcap=cap, sinks=sinks)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(torch.cat(outs)))
        # decode: paged = contiguous
        L = sr.DECODE_L
        probs = _problems("decode", dev, shape, dtype, "peaked", W, nan_below=False)
        plain = _decode(dev, shape, L, probs, W)
        rm = _row_maxima(probs, [(None, plain[1][b], plain[2][b]) for b in range(len(probs))], W, cap)
        sinks = sr.make_sinks("near", rm, nq)
        want = _decode(dev, shape, L, probs, W, cap, sinks)
        assert _same(want[1:], plain[1:]) and not torch.equal(_bits(want[0]), _bits(plain[0]))
        B = len(probs)
        cache = qp.PagedKVCache(1, B * L // 16, nkv, 16, hd, B, L // 16, dtype=dtype, device=dev)
        _page_out(cache, (_stack([p.kc for p in probs]), _stack([p.vc for p in probs])), dev)
        q, k, v = _qkv(*(torch.cat([getattr(p, a) for p in probs]) for a in ("q32", "k32", "v32")))
        out = torch.full((B, nq * hd), float("nan"), dtype=F16, device=dev)
        qp.paged_decode_attention(q, k, v, cache.kpool[0], cache.vpool[0], cache.table, torch.tensor([p.pos0 for p in probs], dtype=torch.long, device=dev),
                                  probs[0].inv, out=out, ws=qp.attention_workspace(B, nq, nkv, hd, L, dev), window=W, softcap=cap, sinks=sinks)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(want[0]))
        for b, p in enumerate(probs):
            pg = cache.pages_of(b)[p.pos0 // 16]
            assert torch.equal(_bits(cache.kpool[0][pg, :, p.pos0 % 16]), _bits(want[1][b, :, p.pos0]))


# ------------------------------------------------------------------------------------------------------------------ heads

@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
@pytest.mark.parametrize("kind", ["decode", "prefill", "ragged"])
def test_heads_do_not_cross(dev, kind, shape, dtype):
    """identical q in every query head, sinks h - nq / 2 around the rows' log-sum-exp (where a sink takes about half a row): head h's
    output follows ITS sink — inside the bound of the reference, and at least four tolerances away from the result with head h //
    rep's or head h + 1's sink"""
    nq, nkv, hd = shape
    L, windows, u_p = sr.launch_shape(kind)
    for W in windows:
        probs = _problems(kind, dev, shape, dtype, "base", W)
        for p in probs:
            pos = torch.arange(p.pos0, p.pos0 + p.T, device=dev)
            tgt = ar.query_targets(p.T, nq, nkv, hd, 900, dev).view(p.T, nq, hd)
            tgt = tgt[:, :1].expand(p.T, nq, hd).contiguous()
            p.q32 = ar.unrope(tgt, pos[:, None], p.inv).reshape(p.T, nq * hd)
            p.q16 = _rotated_q(p.q32, p.pos, shape, dev)
            assert torch.equal(p.q16.view(p.T, nq, hd)[:, 0], p.q16.view(p.T, nq, hd)[:, nq - 1])
        filled = _run(kind, dev, shape, L, probs, W)
        lse = [sr.row_lse(p.q16, kc, vc, p.pos, W, nq, nkv, hd, p.scale) for p, (_, kc, vc) in zip(probs, filled)]
        groups = [[i] for i in range(len(probs))] if kind == "prefill" else [list(range(len(probs)))]  # the rows of one launch
        got = {}
        for group in groups:
            sinks = (float(torch.cat([lse[i] for i in group]).median()) + torch.arange(nq, device=dev) - nq / 2).float()
            for i, res in zip(group, _run(kind, dev, shape, L, [probs[i] for i in group], W, None, sinks)):
                got[i] = (sinks, res)
        seen = {"div_rep": 0.0, "plus1": 0.0}
        for i, p in enumerate(probs):
            sinks, (out, kc, vc) = got[i]
            ref, A, Smax = sr.score_fp64(p.q16, kc, vc, p.pos, W, nq, nkv, hd, p.scale, None, sinks)
            tol = sr.bound(ref, A, Smax, u_p)
            assert _ratio(out, ref, tol) <= 1.0
            for how in ("div_rep", "plus1"):
                bad = sr.score_fp64(p.q16, kc, vc, p.pos, W, nq, nkv, hd, p.scale, None, sinks, mutate=("sink_head", how))[0]
                seen[how] = max(seen[how], _ratio(out, bad, tol))
        assert min(seen.values()) >= 4.0, seen  # (over the launches of the case: a row far from the median weighs its sink little)


# ----------------------------------------------------------------------------------------------------------------- errors

@pytest.mark.gpu
def test_errors_are_raised_before_any_launch(dev):
    shape = nq, nkv, hd = (8, 2, 128)
    L = 256
    p = WProblem(dev, shape, L, F16, "peaked", 100, 1, None, 1, nan_below=False)
    kc0, vc0 = p.kc.clone(), p.vc.clone()
    pos_t = torch.tensor([100], dtype=torch.long, device=dev)
    good = torch.zeros(nq, device=dev)
    bad_sinks = [torch.zeros(nq, dtype=torch.float64, device=dev), torch.zeros(nq, dtype=F16, device=dev), torch.zeros(nq - 1, device=dev),
                 torch.zeros(nq + 1, device=dev), torch.zeros(1, nq, device=dev), torch.zeros(nq), torch.zeros(2 * nq, device=dev)[::2], [0.0] * nq]
    bad_caps = [-1.0, 0.0, float("nan"), float("inf"), float("-inf"), "8", True]

    def launches(out, kw):
        q, k, v = _qkv(p.q32, p.k32, p.v32)
        kc, vc = p.kc[None], p.vc[None]
        one = torch.tensor([0], dtype=torch.int32, device=dev)
        row0 = torch.tensor([0, 1], dtype=torch.int32, device=dev)
        yield lambda: qp.decode_attention(q, k, v, kc, vc, pos_t, p.inv, out=out, **kw)
        yield lambda: qp.prefill_attention(q, k, v, p.kc, p.vc, pos_t, p.inv, out=out, **kw)
        yield lambda: qp.ragged_prefill_attention(q, k, v, kc, vc, one, row0, pos_t, p.inv, out=out, **kw)
        pool_k, pool_v = p.kc.view(nkv, L // 16, 16, hd).transpose(0, 1).contiguous(), p.vc.view(nkv, L // 16, 16, hd).transpose(0, 1).contiguous()
        table = torch.arange(L // 16, dtype=torch.int32, device=dev)[None]
        yield lambda: qp.paged_decode_attention(q, k, v, pool_k, pool_v, table, pos_t, p.inv, out=out, **kw)
        yield lambda: qp.paged_prefill_attention(q, k, v, pool_k, pool_v, table[0], pos_t, p.inv, out=out, **kw)
        yield lambda: qp.paged_ragged_prefill_attention(q, k, v, pool_k, pool_v, table, one, row0, pos_t, p.inv, out=out, **kw)

    for kws, match in (([{"softcap": c} for c in bad_caps] + [{"softcap": c, "sinks": good} for c in bad_caps], "softcap"),
                       ([{"sinks": s} for s in bad_sinks] + [{"sinks": s, "softcap": 8.0} for s in bad_sinks], "sinks")):
        for kw in kws:
            out = torch.full((1, nq * hd), float("nan"), dtype=F16, device=dev)
            for launch in launches(out, kw):
                with pytest.raises(QpalError, match=match):
                    launch()
            torch.cuda.synchronize()
            assert bool(torch.isnan(out).all()) and torch.equal(_bits(p.kc), _bits(kc0)) and torch.equal(_bits(p.vc), _bits(vc0))
    # the shared-prefix launch has neither
    cache = qp.PagedKVCache(1, 2 * L // 16, nkv, 16, hd, 2, L // 16, dtype=F16, device=dev, min_len=32, min_members=2)
    cache.reserve(0, 101)
    cache.fork(0, 1, 64)
    cache.reserve(1, 101)
    q2, k2, v2 = _qkv(p.q32.repeat(2, 1), p.k32.repeat(2, 1), p.v32.repeat(2, 1))
    pos2 = torch.tensor([100, 100], dtype=torch.long, device=dev)
    for kw in ({"softcap": 8.0}, {"sinks": good}, {"softcap": 8.0, "sinks": good}):
        out = torch.full((2, nq * hd), float("nan"), dtype=F16, device=dev)
        with pytest.raises(QpalError, match="shared-prefix"):
            qp.shared_prefix_decode_attention(q2, k2, v2, cache.kpool[0], cache.vpool[0], cache.table, pos2, p.inv, cache.prefix, out=out,
                                              **kw)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())
