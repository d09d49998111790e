"""qpal_sample_trunc on the GPU — min-p, top-a and typical-p in the draw — and the step classes with a truncating
sampler.  A draw is judged on the logits the kernel was given by the sandwich of tests/truncation_cases.py (its docstring has the
derivations of EPS, delta and tol_d); the inputs of the contract test are the ones tests/test_truncation_spec.py runs its fp32
emulation of the kernel on."""
import numpy as np
import pytest
import torch

import test_spec as ts
from qpalette_amd import sampling
from test_sampling import TYPES, _make_sampler, _model
from test_spec import dev, model, prompts  # noqa: F401  (fixtures)
from truncation_cases import COUNTERS, SHAPES, contract_case, contract_check, sampler_for

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def qp():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import qpalette_amd
    qpalette_amd._native.lib()
    return qpalette_amd


def test_draws_against_the_contract(qp):
    """vocab {128256, 1000, 33} x rows {1, 128} x logits N(0, 1), N(0, 2.5^2), three counters each, per-row mixed parameters in ONE
    launch: min-p 0.05, top-a 0.2, typical-p 0.9, typical-p 0.2, top-k 50 + top-p 0.9 + min-p 0.1 + typical-p 0.95, a neutral row, a
    greedy row, an inactive row.  Every draw passes the sandwich; at most 1 % differ from reference_draw's exact winner."""
    d = torch.device("cuda", 0)
    draws = exact = 0
    for case, (vocab, rows, sigma) in enumerate(SHAPES):
        logits, types, seeds, ctrs = contract_case(case)
        smp = sampler_for(qp, types, seeds, vocab, d)
        smp.logits.copy_(torch.from_numpy(logits))
        for rep in range(COUNTERS):
            out = torch.full((rows,), -7, dtype=torch.int64, device=d)
            qp.sample(smp.logits, smp, torch.from_numpy(ctrs[rep]).to(d), out=out)
            toks = out.cpu().tolist()
            for r, t in enumerate(types):
                if t == "inactive":
                    assert toks[r] == -7, "an inactive row's token must keep its sentinel"
                    continue
                exact += bool(contract_check(logits[r], t, seeds[r], int(ctrs[rep, r]), toks[r]))
                draws += 1
    print(f"draws {draws}, exact winner {exact}, differing {draws - exact} ({100.0 * (draws - exact) / draws:.3f} %)")
    assert draws >= 1500
    assert draws - exact <= 0.01 * draws


@pytest.mark.parametrize("vocab", [128256, 33])
@pytest.mark.parametrize("rows", [1, 128])
def test_neutral_rows_equal_qpal_sample(qp, rows, vocab):
    """every row type of tests/test_sampling.py: qpal_sample_trunc with null filter pointers, with all three vectors neutral and
    with one vector given (the other two null) returns qpal_sample's tokens"""
    d = torch.device("cuda", 0)
    lib, stream = qp._native.lib(), torch.cuda.current_stream(d).cuda_stream
    for offset in range(len(TYPES) if rows == 1 else 1):
        smp, types = _make_sampler(qp, rows, vocab, d, offset=offset, seed0=31 * offset + 5)
        smp.logits.copy_(torch.randn(rows, vocab, device=d, generator=torch.Generator(device=d).manual_seed(vocab + offset)) * 2.0)
        ctr = torch.tensor([-1 if t == "inactive" else 11 + 7 * r for r, t in enumerate(types)], dtype=torch.int64, device=d)
        want = torch.full((rows,), -7, dtype=torch.int64, device=d)
        qp.sample(smp.logits, smp, ctr, out=want)
        tr = qp.Sampler(rows, vocab, d, truncation=True)
        assert tr.min_p is not None and smp.min_p is None
        tr.typical_p.copy_(torch.tensor([(1.0, 0.0, 1.5, -1.0)[r % 4] for r in range(rows)]))
        tr.min_p.copy_(torch.tensor([(0.0, -1.0)[r % 2] for r in range(rows)]))
        for name in ("temperature", "top_k", "top_p", "seed"):
            getattr(tr, name).copy_(getattr(smp, name))
        got = torch.full((rows,), -7, dtype=torch.int64, device=d)
        qp.sample(smp.logits, tr, ctr, out=got)
        assert torch.equal(got, want), (offset, got.tolist(), want.tolist())
        ld = smp.logits.stride(0) if rows > 1 else vocab
        for filt in ((None, None, None), (None, tr.top_a.data_ptr(), None)):
            raw = torch.full((rows,), -7, dtype=torch.int64, device=d)
            rc = lib.qpal_sample_trunc(smp.logits.data_ptr(), ld, rows, vocab, smp.temperature.data_ptr(), smp.top_k.data_ptr(),
                                       smp.top_p.data_ptr(), *filt, smp.seed.data_ptr(), ctr.data_ptr(), raw.data_ptr(), stream)
            assert rc == 0 and torch.equal(raw, want), (offset, filt)


# (T, top_k, top_p, min_p, top_a, typical_p) of the degenerate-row tests
FILTERS = [(1.0, 0, 1.0, 0.3, 0.0, 1.0), (0.8, 0, 1.0, 0.0, 0.5, 1.0), (1.0, 0, 1.0, 0.0, 0.0, 0.4), (0.7, 50, 0.9, 0.1, 0.2, 0.6)]


def _exact_kept(l, t):
    T, top_k, top_p, min_p, top_a, typ = (float(np.float32(x)) if i != 1 else x for i, x in enumerate(t))
    lc = sampling.clean_logits(l)
    kmask = sampling.topk_mask(lc, top_k)
    N = sampling.nucleus_mask(sampling.probabilities(lc, T, kmask), kmask, top_p)
    return sampling.truncation_mask(lc, T, N, min_p, top_a, typ)


@pytest.mark.parametrize("case", ["neg_inf", "nan", "pos_inf", "one_finite", "all_equal"])
def test_degenerate_rows_satisfy_the_contract_exactly(qp, case):
    """one row per filter setting: the token is reference_draw's (all -inf / NaN: 0; +inf entries: the lowest of them; one finite
    logit: it), or with all-equal logits a token of the exact kept set (everything) that passes the sandwich; a fifth, inactive row
    keeps its sentinel"""
    d = torch.device("cuda", 0)
    vocab = 5000
    l = torch.randn(5, vocab, generator=torch.Generator().manual_seed(3))
    if case == "neg_inf":
        l[:] = float("-inf")
    elif case == "nan":
        l[:] = float("nan")
    elif case == "pos_inf":
        l[:, [4000, 77, 1234]] = float("inf")
        l[:, 9] = float("nan")
    elif case == "one_finite":
        l[:] = float("-inf")
        l[:, 4321] = -3.5
    else:
        l[:] = 0.75
    types = FILTERS + [FILTERS[0]]
    smp = sampler_for(qp, types, [3, 4, 5, 6, 7], vocab, d)
    ln = l.numpy()
    seen = set()
    for c in range(4):
        ctr = torch.tensor([c, c + 10, c + 20, c + 30, -1], dtype=torch.int64, device=d)
        out = torch.full((5,), -7, dtype=torch.int64, device=d)
        qp.sample(l.to(d), smp, ctr, out=out)
        toks = out.cpu().tolist()
        assert toks[4] == -7
        for r, t in enumerate(FILTERS):
            want = sampling.reference_draw(ln[r], t[0], t[1], t[2], 3 + r, int(ctr[r]), min_p=t[3], top_a=t[4], typical_p=t[5])
            if case == "all_equal":
                kept = _exact_kept(ln[r], t)
                assert kept.all() and 0 <= toks[r] < vocab
                contract_check(ln[r], t, 3 + r, int(ctr[r]), toks[r])
                seen.add(toks[r])
            else:
                assert toks[r] == want == {"neg_inf": 0, "nan": 0, "pos_inf": 77, "one_finite": 4321}[case], (r, toks[r], want)
    assert case != "all_equal" or len(seen) > 4


def test_exact_ties_at_delta(qp):
    """three levels: one token at 3, twelve at 1 (ids spread over the row), the rest at -12.  All tokens of a level share d, so
    typical-p keeps whole levels: q = 0.381 for the top token, 0.0516 for each of the twelve, c = 1.24, so d = 0.76 for the twelve, 1.24
    for the top token, 13.8 for the rest.  With typical_p = 0.3 delta falls on the twelve and all twelve are kept and nothing else;
    the masses of the level sets (0.619, 0.9999) are far from 0.3, so the kernel's set is the exact one.  min-p 0.1 on the same row
    keeps the thirteen (w = 1 and 0.135)."""
    d = torch.device("cuda", 0)
    vocab = 1000
    l = torch.full((2, vocab), -12.0)
    ties = [5, 64, 65, 130, 255, 256, 511, 700, 701, 888, 998, 999]
    l[:, ties] = 1.0
    l[:, 400] = 3.0
    types = [(1.0, 0, 1.0, 0.0, 0.0, 0.3), (1.0, 0, 1.0, 0.1, 0.0, 1.0)]
    kept = [_exact_kept(l[r].numpy(), types[r]) for r in range(2)]
    assert np.flatnonzero(kept[0]).tolist() == ties and np.flatnonzero(kept[1]).tolist() == sorted(ties + [400])
    smp = sampler_for(qp, types, [21, 22], vocab, d)
    seen = [set(), set()]
    for c in range(48):
        ctr = torch.full((2,), c, dtype=torch.int64, device=d)
        toks = qp.sample(l.to(d), smp, ctr).cpu().tolist()
        for r in range(2):
            assert kept[r][toks[r]], (r, c, toks[r])
            contract_check(l[r].numpy(), types[r], 21 + r, c, toks[r])
            seen[r].add(toks[r])
    assert len(seen[0]) >= 6 and 400 in seen[1] and len(seen[1]) >= 4


def test_a_draw_depends_on_seed_counter_logits_and_parameters_only(qp):
    """a row alone and the same row as row 77 of 128: the same token; two launches bitwise equal; another min_p in row 3 changes
    nothing of any other row"""
    d = torch.device("cuda", 0)
    vocab = 128256
    big = torch.randn(128, vocab, device=d, generator=torch.Generator(device=d).manual_seed(9)) * 1.5
    for t in ((1.0, 0, 1.0, 0.05, 0.0, 1.0), (0.8, 0, 1.0, 0.0, 0.2, 1.0), (0.9, 0, 1.0, 0.0, 0.0, 0.6), (0.7, 50, 0.9, 0.1, 0.1, 0.9)):
        smp = qp.Sampler(128, vocab, d, temperature=1.0, seed=list(range(128)), min_p=0.02, typical_p=0.95)
        smp.set(77, temperature=t[0], top_k=t[1], top_p=t[2], min_p=t[3], top_a=t[4], typical_p=t[5], seed=424242)
        ctr = torch.arange(128, dtype=torch.int64, device=d)
        ctr[77] = 12345
        a = qp.sample(big, smp, ctr)
        b = qp.sample(big, smp, ctr)
        one = sampler_for(qp, [t], [424242], vocab, d)
        c = qp.sample(big[77:78].clone(), one, ctr[77:78].clone())
        smp.set(3, min_p=0.9)
        e = qp.sample(big, smp, ctr)
        torch.cuda.synchronize()
        assert torch.equal(a, b)
        assert int(a[77]) == int(c[0])
        keep = torch.arange(128, device=d) != 3
        assert torch.equal(a[keep], e[keep])
        contract_check(big[77].cpu().numpy(), t, 424242, 12345, int(a[77]))


# ---------------------------------------------------------------------------------------------------------------- the steps

STEP_TYPES = [(1.0, 0, 1.0, 0.05, 0.0, 1.0), (0.8, 0, 1.0, 0.0, 0.2, 0.9), (0.7, 50, 0.9, 0.1, 0.0, 0.95), (1.2, 0, 1.0, 0.0, 0.0, 0.5)]


def _decode_state(m, B, d, seed):
    g = torch.Generator(device=d).manual_seed(seed)
    kc = [(torch.randn(B, 8, 512, 128, device=d, generator=g) * 0.5).half() for _ in m.layers]
    vc = [(torch.randn(B, 8, 512, 128, device=d, generator=g) * 0.5).half() for _ in m.layers]
    tok = torch.randint(0, 4096, (B,), device=d, generator=g)
    pos = torch.tensor([10, 3, 100, 250][:B], dtype=torch.int64, device=d)
    return kc, vc, tok, pos


def _check_rows(logits, types, seeds, ctrs, toks):
    torch.cuda.synchronize()
    lg = logits.cpu().numpy()
    for r, t in enumerate(types):
        if int(ctrs[r]) >= 0:
            contract_check(lg[r], t, int(seeds[r]), int(ctrs[r]), int(toks[r]))


@pytest.mark.parametrize("B", [1, 4])
def test_decode_step_with_a_truncating_sampler(qp, B):
    """DecodeStep(sampler=a truncating Sampler): the same launch count as with a plain sampler; every out_tok[b] passes the sandwich
    on sampler.logits[b] with ctr = pos[b] (slot 1 of 4 inactive)"""
    d = torch.device("cuda", 0)
    m = _model(d)
    types = STEP_TYPES[:B]
    seeds = [11 + b for b in range(B)]
    smp = sampler_for(qp, types, seeds, 4096, d)
    kc, vc, tok, pos = _decode_state(m, B, d, 5)
    if B > 1:
        pos[1] = -1
    out = torch.full((B,), -7, dtype=torch.int64, device=d)
    st = qp.DecodeStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, tok, pos, out, sampler=smp)
    plain = qp.DecodeStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, tok, pos, out.clone(), sampler=qp.Sampler(B, 4096, d))
    assert st.launches_per_token == plain.launches_per_token
    for _ in range(2):
        st()
        _check_rows(smp.logits, types, seeds, pos.tolist(), out.tolist())
        assert B == 1 or int(out[1]) == -7
        tok.copy_(torch.where(pos >= 0, out, tok))
        pos += (pos >= 0).long()


def test_prefill_with_a_truncating_sampler(qp):
    d = torch.device("cuda", 0)
    m = _model(d)
    B, slot, N = 3, 1, 37
    kc = [torch.zeros(B, 8, 512, 128, dtype=torch.float16, device=d) for _ in m.layers]
    vc = [torch.zeros(B, 8, 512, 128, dtype=torch.float16, device=d) for _ in m.layers]
    types, seeds = STEP_TYPES[:B], [1, 2, 3]
    smp = sampler_for(qp, types, seeds, 4096, d)
    pf = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, chunk=128, sampler=smp)
    toks = torch.randint(0, 4096, (N,), device=d, generator=torch.Generator(device=d).manual_seed(N))
    out = pf(toks, slot=slot, pos0=4)
    torch.cuda.synchronize()
    contract_check(smp.logits[slot].cpu().numpy(), types[slot], seeds[slot], 4 + N - 1, int(out[0]))


def test_ragged_step_draws_with_the_slots_gathered_parameters(qp):
    """four segments in the order of slots 3, 0, 2, 1: rs.draw holds the slots' min_p / top_a / typical_p per SEGMENT, and each
    segment's token passes the sandwich on rs.draw.logits[s] with its slot's parameters and seed and its last position"""
    d = torch.device("cuda", 0)
    m, nb = _model(d), 4
    kc = [torch.zeros(nb, 8, 512, 128, dtype=torch.float16, device=d) for _ in m.layers]
    vc = [t.clone() for t in kc]
    seeds = [11, 12, 13, 14]
    smp = sampler_for(qp, STEP_TYPES, seeds, 4096, d)
    rs = qp.RaggedStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, rows=128, segments=4, sampler=smp)
    assert rs.draw.min_p is not None
    plain = qp.RaggedStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, rows=128, segments=4, sampler=qp.Sampler(nb, 4096, d))
    assert plain.draw.min_p is None
    g = torch.Generator().manual_seed(21)
    items = [(3, torch.randint(0, 4096, (30,), generator=g).to(d), 0), (0, torch.randint(0, 4096, (7,), generator=g).to(d), 0),
             (2, torch.randint(0, 4096, (50,), generator=g).to(d), 0), (1, torch.randint(0, 4096, (41,), generator=g).to(d), 0)]
    got = rs(*rs.pack(items)).clone()
    order = [it[0] for it in items]
    for name in sampling.TRUNCATION:
        assert torch.equal(getattr(rs.draw, name), getattr(smp, name)[order])
    _check_rows(rs.draw.logits, [STEP_TYPES[s] for s in order], [seeds[s] for s in order], rs.ctr.tolist(), got.tolist())


def test_set_between_replays_of_a_captured_decode_step(qp):
    """a captured DecodeStep at B = 4, T = 1.5: replayed twice on the same state it draws the same tokens; set(slot, min_p=1) — only
    the likeliest token is left — makes that slot's next draw its argmax and leaves every other slot's token as it was"""
    d = torch.device("cuda", 0)
    m, B = _model(d), 4
    smp = qp.Sampler(B, 4096, d, temperature=1.5, seed=[5, 6, 7, 8], min_p=0.001, typical_p=0.99)
    kc, vc, tok, pos = _decode_state(m, B, d, 8)
    out = torch.full((B,), -7, dtype=torch.int64, device=d)
    st = qp.DecodeStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, tok, pos, out, sampler=smp)
    s = torch.cuda.Stream(d)
    with torch.cuda.stream(s):
        st()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            st()
        g.replay()
        first = out.clone()
        g.replay()
        assert torch.equal(out, first)
        top = smp.logits.argmax(dim=1)
        moved = [b for b in range(B) if int(first[b]) != int(top[b])]
        assert moved, "at T = 1.5 some slot must draw another token than its argmax"
        b = moved[0]
        smp.set(b, min_p=1.0)
        g.replay()
        torch.cuda.synchronize()
    assert int(out[b]) == int(top[b]) != int(first[b])
    keep = torch.arange(B, device=d) != b
    assert torch.equal(out[keep], first[keep])


# ---- the speculative step: losslessness with the truncation filters on (a draw depends on (seed, ctr, logits,
# parameters) only, so verifying a drafted token by drawing at its row is drawing it one token at a time)

SPEC_PARAMS = {
    "seeded": dict(temperature=[0.7, 1.0, 0.0, 1.3], top_k=[40, 0, 5, 0], top_p=[0.9, 0.95, 1.0, 1.0], seed=[11, 12, 13, 14],
                   min_p=[0.05, 0.0, 0.1, 0.02], typical_p=[1.0, 0.9, 0.5, 0.8]),
    "greedy": dict(temperature=0.0, min_p=[0.05, 0.0, 0.1, 0.02], typical_p=[1.0, 0.9, 0.5, 0.8]),
}


def _trunc_scores(l, params, slot, ctr):
    """ts._scores with step 4a: the race scores of (slot, ctr) on the logits l, -inf outside R; greedy: l"""
    get = lambda name, default: np.broadcast_to(params.get(name, default), ts.NB)[slot]
    l = sampling.clean_logits(l)
    T, k, p = float(np.float32(get("temperature", 1.0))), int(get("top_k", 0)), float(np.float32(get("top_p", 1.0)))
    if not T > 0.0 or k == 1:
        return l.astype(np.float64)
    kmask = sampling.topk_mask(l, k)
    N = sampling.nucleus_mask(sampling.probabilities(l, T, kmask), kmask, p)
    R = sampling.truncation_mask(l, T, N, float(np.float32(get("min_p", 0.0))), 0.0, float(np.float32(get("typical_p", 1.0))))
    return np.where(R, sampling.race_scores(l.astype(np.float64) / T, int(get("seed", 0)), int(ctr)), -np.inf)


@pytest.mark.parametrize("mode", ["greedy", "seeded"])
def test_speculative_step_emits_the_one_token_stream(qp, dev, model, prompts, mode):  # noqa: F811
    """tests/test_spec.py's model, prompts and near-tie rule, min-p and typical-p set per slot: the yardstick is Prefill + one-token
    DecodeStep(generic=True) with the truncating sampler; SpeculativeStep with prompt-lookup drafts and with the right drafts given
    emits the same 24 tokens per slot"""
    params, NB, NEW = SPEC_PARAMS[mode], ts.NB, ts.NEW
    m = model
    kc, vc = ts._caches(m, dev, ts.F16)
    smp = qp.Sampler(NB, ts.VOCAB, dev, **params)
    pf = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, chunk=128, sampler=smp)
    tok = torch.zeros(NB, dtype=torch.long, device=dev)
    want, logits = [[] for _ in range(NB)], [[] for _ in range(NB)]
    for b, p in enumerate(prompts):
        tok[b] = pf(p, slot=b, pos0=0)[0]
        logits[b].append(smp.logits[b].cpu().numpy().copy())
        want[b].append(int(tok[b]))
    pos = torch.tensor([p.shape[0] for p in prompts], dtype=torch.long, device=dev)
    out = torch.zeros(NB, dtype=torch.long, device=dev)
    step = qp.DecodeStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, tok, pos, out, generic=True, sampler=smp)
    for _ in range(NEW - 1):
        step()
        lg = smp.logits.cpu().numpy()
        for b in range(NB):
            want[b].append(int(out[b]))
            logits[b].append(lg[b].copy())
        tok.copy_(out)
        pos += 1
    for way in ("a", "b"):
        kr, vr = ts._caches(m, dev, ts.F16)
        pf2 = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kr, vr, m.inv_freq, chunk=128)
        ss = qp.SpeculativeStep(m.layers, m.embed, m.norm, m.lm_head, kr, vr, m.inv_freq, draft=ts.DRAFT, gram=(2, 4),
                                sampler=qp.Sampler(NB, ts.VOCAB, dev, **params))
        assert ss.draw.min_p is not None and ss.draw.typical_p.shape == (ss.rows,)
        for b, p in enumerate(prompts):
            pf2(p[:-1], slot=b, pos0=0)
            ss.begin(b, p.tolist(), limit=p.shape[0] + NEW)
        got, records = ts._generate(ss, dev, want, way)
        behind = 0
        for b in range(NB):
            assert len(got[b]) == NEW
            diff = [i for i in range(NEW) if got[b][i] != want[b][i]]
            if diff:
                i = diff[0]
                s = _trunc_scores(logits[b][i], params, b, prompts[b].shape[0] - 1 + i)
                gap, thr = abs(float(s[want[b][i]] - s[got[b][i]])), 2 * ts._bound(logits[b][i])
                print(f"{mode} {way} slot {b} token {i}: {got[b][i]} for {want[b][i]}, score gap {gap:.4g}, excuse threshold {thr:.4g}")
                assert gap < thr, f"slot {b} token {i}: {got[b][i]} for {want[b][i]} is no near tie ({gap} >= {thr})"
                behind += NEW - i
        assert behind <= 0.05 * NB * NEW, f"{behind} of {NB * NEW} tokens lie behind an excused near tie"
        print(f"{mode} {way}: {len(records)} steps for {NEW} tokens per slot, {behind} tokens behind a near tie")
