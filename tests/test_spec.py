"""Speculative decoding on the GPU (csrc/spec.hip, qpalette_amd.spec_draft / spec_accept, decoder.SpeculativeStep).

Kernels: every output of qpal_spec_draft / qpal_spec_accept bit for bit the numpy references (tests/test_spec_contract.py holds those
to hand-made cases), two launches bitwise equal.  Whole model: SpeculativeStep emits the stream sequential DecodeStep sampling emits,
with prompt lookup, with the caller's drafts right, partly right and all wrong, greedy and seeded, on fp16 contiguous caches and on
paged e4m3 pools; a captured step replayed to the end, and a new sequence begun between replays.

Near ties: the two paths compute a row's logits in launches of different row counts; §13's whole-model bound allows 2^-7 max(1, max
|l|) between them.  A first difference in a slot's stream is excused only if, in the yardstick's logits of that step, the race scores
(greedy: the logits) of the two tokens differ by less than twice that bound; the slot's comparison ends there, and at most 5 % of a
run's tokens may lie behind an excuse."""
import os
import sys

import numpy as np
import pytest
import torch

import qpalette_amd as qp
from qpalette_amd import sampling
from qpalette_amd import speculative as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, F8 = torch.float16, torch.float8_e4m3fn


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


# ---------------------------------------------------------------------------------------------------------------- kernels

DRAFT_OUT = (("tokens", torch.int64, "R"), ("seq", torch.int32, "B"), ("row0", torch.int32, "B1"), ("pos0", torch.int64, "B"),
             ("row_slot", torch.int32, "R"), ("row_ctr", torch.int64, "R"), ("n_draft", torch.int32, "B"))


def _gpu_draft(dev, hist, n_tok, limit, K, gram, R, max_len, ext=None, ext_n=None, fill=-77):
    """the kernel on a numpy state; every output starts as `fill`, so a word the launch leaves alone shows"""
    B = hist.shape[0]
    sizes = {"R": R, "B": B, "B1": B + 1}
    out = {name: torch.full((sizes[n],), fill, dtype=dt, device=dev) for name, dt, n in DRAFT_OUT}
    kw = {}
    if ext is not None:
        kw = dict(ext_draft=torch.as_tensor(ext, dtype=torch.int64).to(dev).contiguous(), ext_n=torch.as_tensor(ext_n, dtype=torch.int32).to(dev))
    qp.spec_draft(torch.as_tensor(hist).to(dev), torch.as_tensor(n_tok, dtype=torch.int64).to(dev),
                  torch.as_tensor(limit, dtype=torch.int64).to(dev), K, gram, max_len, **out, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(got, ref, what):
    for k, v in ref.items():
        assert got[k].dtype == v.dtype and np.array_equal(got[k], v), (what, k, got[k][:24], v[:24])


LD, MAX_LEN = 5003, 5002  # ld_hist is no multiple of 4: the rows of slots 1, 2, 3 (mod 4) are not 16-byte aligned
LENGTHS = [5000, 40, 5002, 1, 4999, 41, 3, 4098, 7, 1029, 0, 4997]  # 5002 = max_len; 1: no gram fits; 0: never begun


def _state(B, seed, lengths=LENGTHS):
    rng = np.random.default_rng(seed)
    hist = rng.integers(0, 5, size=(B, LD)).astype(np.int32)
    n_tok = np.array([lengths[b % len(lengths)] for b in range(B)], np.int64)
    limit = n_tok + 100
    limit[6::7] = n_tok[6::7]          # at the limit: inactive (B = 128; at B = 5 the aligned slot 4, 4999 tokens, stays active)
    limit[3::11] = n_tok[3::11] + 2    # one draft at most
    return hist, n_tok, limit


@pytest.mark.gpu
@pytest.mark.parametrize("full", [False, True], ids=["R=B", "R=128"])
@pytest.mark.parametrize("K", [0, 4, 15])
@pytest.mark.parametrize("B", [1, 5, 128])
def test_draft_kernel_is_the_reference(dev, B, K, full):
    """histories of 3, 40 and 5000 tokens (and more) over a vocabulary of 5: many matches at many offsets; 5000 tokens cross the
    per-thread loop and the 16-byte tail; slots at n_tok = max_len, at their limit and with one token"""
    R = 128 if full else B
    gram = (1, 8) if K == 15 else (2, 4)
    cases = [[n] for n in (3, 40, 5000)] if B == 1 else [LENGTHS]
    for i, lengths in enumerate(cases):
        hist, n_tok, limit = _state(B, seed=100 * B + K + i, lengths=lengths)
        ref = sp.reference_spec_draft(hist, n_tok, limit, K, gram[0], gram[1], R, MAX_LEN)
        got = _gpu_draft(dev, hist, n_tok, limit, K, gram, R, MAX_LEN)
        _same(got, ref, (B, K, R, lengths[0]))
        again = _gpu_draft(dev, hist, n_tok, limit, K, gram, R, MAX_LEN, fill=12345)
        _same(again, got, "two launches on one state")
        if K and B > 1 and full:
            assert int(ref["n_draft"].max()) > 0, "no slot drafted: the case shows too little"


@pytest.mark.gpu
@pytest.mark.parametrize("gram", [(1, 1), (3, 3), (4, 8), (8, 8)], ids=str)
def test_draft_kernel_every_gram_range(dev, gram):
    """a vocabulary of 2: grams up to 8 match, the longest wins; every length 1 .. 70 so every alignment of the look-back window"""
    B, K = 70, 6
    rng = np.random.default_rng(gram[0] + 10 * gram[1])
    hist = rng.integers(0, 2, size=(B, 75)).astype(np.int32)
    n_tok = np.arange(1, B + 1)
    limit = n_tok + 9
    ref = sp.reference_spec_draft(hist, n_tok, limit, K, gram[0], gram[1], 128, 75)
    _same(_gpu_draft(dev, hist, n_tok, limit, K, gram, 128, 75), ref, gram)
    assert int(ref["n_draft"].max()) > 0


@pytest.mark.gpu
def test_draft_kernel_external_drafts(dev):
    B, K, R = 5, 4, 14
    hist, n_tok, limit = _state(B, seed=3)
    n_tok[2], limit[2] = 3, 103
    limit[1], limit[4] = n_tok[1] + 3, n_tok[4] + 100  # slot 1: d_max = 2; slot 3 (n_tok = 1, limit 3): d_max = 1
    ext = np.array([[11, 12, 13, 14], [21, 22, 23, 24], [31, -1, 33, 34], [41, 42, 43, 2 ** 30], [51, 52, 53, 54]])
    for ext_n in ([4, 4, 4, 4, 4], [0, 9, 1, -3, 2]):
        ref = sp.reference_spec_draft(hist, n_tok, limit, K, 2, 4, R, MAX_LEN, ext_draft=ext, ext_n=ext_n)
        _same(_gpu_draft(dev, hist, n_tok, limit, K, (2, 4), R, MAX_LEN, ext=ext, ext_n=ext_n), ref, ext_n)
    assert ref["n_draft"].tolist() == [0, 2, 1, 0, 2]


@pytest.mark.gpu
@pytest.mark.parametrize("K", [0, 4, 15])
@pytest.mark.parametrize("B", [1, 5, 128])
def test_accept_kernel_is_the_reference(dev, B, K):
    """random draws that accept none, some or all drafts, stop tokens and tight limits; out_tok entries past n_out keep a sentinel"""
    R, ld = 128, 64
    rng = np.random.default_rng(7 * B + K)
    hist = rng.integers(0, 5, size=(B, ld)).astype(np.int32)
    n_tok = rng.integers(0, ld - 10, size=B)           # some 0: inactive; room for K + 1 below ld except where it is tight
    if B == 128:
        n_tok[rng.random(B) < 0.7] = 0                  # (so that the 128 rows have room for drafts)
    n_tok[B // 2] = ld - 2                              # emitted tokens cross the end of the history
    limit = n_tok + rng.integers(0, 2 * K + 4, size=B)  # some at the limit (inactive), some cut the emitted tokens
    eos = np.where(rng.random(B) < 0.5, rng.integers(0, 5, size=B), -1)
    d = sp.reference_spec_draft(hist, n_tok, limit, K, 1, 4, R, 1 << 20, ext_draft=rng.integers(0, 5, size=(B, K)), ext_n=np.full(B, K))
    drawn = rng.integers(0, 5, size=R)
    keep = rng.random(R) < 0.8
    drawn[:-1] = np.where(keep[:-1], d["tokens"][1:], drawn[:-1])  # row r's draw mostly equals the next row's draft
    out0 = np.full((B, K + 1), -9, np.int64)
    ref = sp.reference_spec_accept(d["tokens"], drawn, d["seq"], d["row0"], hist, n_tok, limit, eos, K, out_tok=out0)
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt).to(dev).contiguous()
    st = dict(hist=t(hist, torch.int32), n_tok=t(n_tok, torch.int64), limit=t(limit, torch.int64))
    out = dict(out_tok=t(out0, torch.int64), n_out=t(np.full(B, -9), torch.int32), n_acc=t(np.full(B, -9), torch.int32))
    qp.spec_accept(t(d["tokens"], torch.int64), t(drawn, torch.int64), t(d["seq"], torch.int32), t(d["row0"], torch.int32),
                   eos=t(eos, torch.int64), **st, **out)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in {**st, **out}.items()}
    _same(got, ref, (B, K))
    # a second launch on a copy of the same state: bitwise the first
    st2 = dict(hist=t(hist, torch.int32), n_tok=t(n_tok, torch.int64), limit=t(limit, torch.int64))
    out2 = dict(out_tok=t(out0, torch.int64), n_out=t(np.full(B, 5), torch.int32), n_acc=t(np.full(B, 5), torch.int32))
    qp.spec_accept(t(d["tokens"], torch.int64), t(drawn, torch.int64), t(d["seq"], torch.int32), t(d["row0"], torch.int32),
                   eos=t(eos, torch.int64), **st2, **out2)
    torch.cuda.synchronize()
    _same({k: v.cpu().numpy() for k, v in {**st2, **out2}.items()}, got, "two launches on one state")
    if B > 1 and K:
        assert int(ref["n_acc"].max()) >= 2
    if B == 128:
        assert int((ref["limit"] != limit).sum()) > 0 and int((ref["n_out"] == 0).sum()) > 0  # stop tokens were hit, slots inactive


# -------------------------------------------------------------------------------------------------------- whole model

NB, L, PS, NEW, DRAFT, VOCAB = 4, 512, 64, 24, 4, 4096
PROMPT_LENGTHS = (5, 17, 40, 64)
# Recorded on an MI355X with these seeds: the yardsticks' smallest winner / runner-up gap, in units of the excuse threshold, is 0.228
# (fp16 greedy), 0.271 (fp16 mixed), 0.235 (e4m3 greedy), 0.283 (e4m3 mixed).  Below 1, so an excuse can occur and the 5 % budget of
# _judge is what binds; of the prompt seeds 31 .. 60 none has every gap above 1, and 31 has the largest least gap (the others: 0.000
# .. 0.215), which is why it stays.  In the recorded run no excuse was taken: all 16 comparisons are equal token for token.
PROMPT_SEED = 31
MIXED = dict(temperature=[0.7, 1.0, 0.0, 1.3], top_k=[40, 0, 5, 3], top_p=[0.9, 0.95, 1.0, 1.0], seed=[11, 12, 13, 14])
GREEDY = dict(temperature=0.0)


@pytest.fixture(scope="module")
def model(dev):
    sys.path.insert(0, os.path.join(ROOT, "perf"))
    from decode_llama import build_model
    return build_model("3_8b", "tcomb_6_7_0.5_none_0.9", None, 2, VOCAB, dev)


@pytest.fixture(scope="module")
def prompts(dev):
    g = torch.Generator().manual_seed(PROMPT_SEED)
    return [torch.randint(0, VOCAB, (n,), generator=g).to(dev) for n in PROMPT_LENGTHS]


def _caches(m, dev, dtype):
    nkv, hd = m.cfg.num_key_value_heads, m.cfg.head_dim
    mk = lambda: torch.zeros(NB, nkv, L, hd, dtype=torch.uint8 if dtype == F8 else F16, device=dev).view(dtype)
    return [mk() for _ in m.layers], [mk() for _ in m.layers]


def _scores(l, params, slot, ctr):
    """the race scores the draw of (slot, ctr) maximises on the logits l: reference_draw's, -inf outside the kept set; greedy: l"""
    l = sampling.clean_logits(l)
    T = float(np.float32(np.broadcast_to(params.get("temperature", 1.0), NB)[slot]))
    k = int(np.broadcast_to(params.get("top_k", 0), NB)[slot])
    p = float(np.float32(np.broadcast_to(params.get("top_p", 1.0), NB)[slot]))
    seed = int(np.broadcast_to(params.get("seed", 0), NB)[slot])
    if not T > 0.0 or k == 1:
        return l.astype(np.float64)
    kmask = sampling.topk_mask(l, k)
    kept = sampling.nucleus_mask(sampling.probabilities(l, T, kmask), kmask, p)
    return np.where(kept, sampling.race_scores(l.astype(np.float64) / T, seed, int(ctr)), -np.inf)


def _bound(l):
    return 2.0 ** -7 * max(1.0, float(np.abs(l[np.isfinite(l)]).max()))


_YARD = {}


def _yardstick(dev, m, prompts, dtype, mode):
    """sequential generation, one token per slot and step: Prefill draws the first new token, DecodeStep(generic=True) the rest.
    Returns (streams [NB][NEW], logits [NB][NEW][VOCAB]); computed once per (cache format, sampling mode) and left unchanged."""
    key = (dtype, mode)
    if key in _YARD:
        return _YARD[key]
    params = MIXED if mode == "mixed" else GREEDY
    kc, vc = _caches(m, dev, dtype)
    smp = qp.Sampler(NB, VOCAB, dev, **params)
    pf = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, chunk=128, sampler=smp)
    tok = torch.zeros(NB, dtype=torch.long, device=dev)
    streams, logits = [[] for _ in range(NB)], [[] for _ in range(NB)]
    for b, p in enumerate(prompts):
        tok[b] = pf(p, slot=b, pos0=0)[0]
        logits[b].append(smp.logits[b].cpu().numpy().copy())
    pos = torch.tensor([p.shape[0] for p in prompts], dtype=torch.long, device=dev)
    out = torch.zeros(NB, dtype=torch.long, device=dev)
    ds = qp.DecodeStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, tok, pos, out, generic=True, sampler=smp)
    for b in range(NB):
        streams[b].append(int(tok[b]))
    for _ in range(NEW - 1):
        ds()
        lg = smp.logits.cpu().numpy()
        for b in range(NB):
            streams[b].append(int(out[b]))
            logits[b].append(lg[b].copy())
        tok.copy_(out)
        pos += 1
    # the smallest gap between the winner and the runner-up of any draw, in units of the excuse threshold (twice the bound)
    gap = np.inf
    for b in range(NB):
        for i in range(NEW):
            s = np.sort(_scores(logits[b][i], params, b, prompts[b].shape[0] - 1 + i))
            assert int(np.argmax(_scores(logits[b][i], params, b, prompts[b].shape[0] - 1 + i))) == streams[b][i]
            gap = min(gap, float(s[-1] - s[-2]) / (2 * _bound(logits[b][i])))
    print(f"yardstick {dtype} {mode}: smallest winner / runner-up gap = {gap:.3f} x the excuse threshold")
    _YARD[key] = (streams, logits, gap)
    return _YARD[key]


def _spec_step(m, dev, prompts, dtype, paged, mode):
    """a SpeculativeStep on fresh caches of its own, prompts[b][:-1] prefilled into slot b"""
    params = MIXED if mode == "mixed" else GREEDY
    nkv, hd, nl = m.cfg.num_key_value_heads, m.cfg.head_dim, len(m.layers)
    table = cache = None
    if paged:
        cache = qp.PagedKVCache(nl, 2 * NB * (L // PS), nkv, PS, hd, NB, L // PS, dtype=dtype, device=dev)
        for n in (64, 128):  # page by page, slot after slot: no slot's pages are consecutive; 128 >= every limit
            for slot in range(NB):
                cache.reserve(slot, n)
        kr, vr, table = cache.kpool, cache.vpool, cache.table
    else:
        kr, vr = _caches(m, dev, dtype)
    pf = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kr, vr, m.inv_freq, chunk=128, block_table=table)
    smp = qp.Sampler(NB, VOCAB, dev, **params) if mode == "mixed" else None
    ss = qp.SpeculativeStep(m.layers, m.embed, m.norm, m.lm_head, kr, vr, m.inv_freq, draft=DRAFT, gram=(2, 4), sampler=smp,
                            block_table=table)
    assert ss.rows == NB * (DRAFT + 1) and ss.context == L and ss.history == L

    def begin(slot, prompt):
        pf(prompt[:-1], slot=slot, pos0=0)
        ss.begin(slot, prompt.tolist(), limit=prompt.shape[0] + NEW)
    for b, p in enumerate(prompts):
        begin(b, p)
    return ss, begin


def _ext(dev, want, done, way):
    """the caller's drafts of one step from the yardstick's streams: the next DRAFT tokens of every slot; way c: draft 2 replaced by
    another token, way d: every draft replaced"""
    ext = torch.zeros(NB, DRAFT, dtype=torch.int64)
    for b in range(NB):
        nxt = want[b][done[b]:done[b] + DRAFT]
        ext[b, :len(nxt)] = torch.tensor(nxt, dtype=torch.int64)
    if way == "c":
        ext[:, 2] = (ext[:, 2] + 1) % VOCAB
    if way == "d":
        ext = (ext + 1) % VOCAB
    return ext.to(dev), torch.full((NB,), DRAFT, dtype=torch.int32, device=dev)


def _generate(ss, dev, want, way, step=None, slots=range(NB)):
    """steps until every slot is at its limit.  Returns (streams, records): per step and slot (tokens emitted before it, n_draft,
    n_acc, n_out).  step: what runs one step in ss()'s place (a graph replay)."""
    got, records = [[] for _ in range(NB)], []
    ext = ext_n = None
    if way != "a":
        ext, ext_n = _ext(dev, want, [0] * NB, way)
    for _ in range(NEW + 1):
        if not bool((ss.n_tok < ss.limit).any()):
            break
        if way != "a":
            e, _ = _ext(dev, want, [len(g) for g in got], way)
            ext.copy_(e)
        (step or (lambda: ss(ext, ext_n) if way != "a" else ss()))()
        out, n_out, n_acc, n_draft = ss.out_tok.cpu(), ss.n_out.cpu(), ss.n_acc.cpu(), ss.n_draft.cpu()
        rec = {}
        for b in slots:
            if int(n_out[b]):
                rec[b] = (len(got[b]), int(n_draft[b]), int(n_acc[b]), int(n_out[b]))
                got[b] += out[b, :int(n_out[b])].tolist()
        records.append(rec)
    assert not bool((ss.n_tok < ss.limit).any()), "a slot did not reach its limit"
    return got, records


def _judge(got, records, want, logits, prompts, params, way):
    """the stream against the yardstick's under the near-tie rule, then the expectations of the way on the steps before any excuse"""
    upto, behind = [NEW] * NB, 0
    for b in range(NB):
        assert len(got[b]) == NEW, (b, len(got[b]))
        diff = [i for i in range(NEW) if got[b][i] != want[b][i]]
        if diff:
            i = diff[0]
            s = _scores(logits[b][i], params, b, prompts[b].shape[0] - 1 + i)
            gap, thr = abs(float(s[want[b][i]] - s[got[b][i]])), 2 * _bound(logits[b][i])
            print(f"slot {b} token {i}: {got[b][i]} for {want[b][i]}, score gap {gap:.4g}, excuse threshold {thr:.4g}")
            assert gap < thr, f"slot {b} token {i}: {got[b][i]} for {want[b][i]} is no near tie ({gap} >= {thr})"
            upto[b], behind = i, behind + NEW - i
    assert behind <= 0.05 * NB * NEW, f"{behind} of {NB * NEW} tokens lie behind an excused near tie"
    acc = drafts = 0
    for rec in records:
        for b, (done, n_draft, n_acc, n_out) in rec.items():
            if done + n_out > upto[b]:
                continue
            acc, drafts = acc + n_acc, drafts + n_draft
            if way != "a":
                assert n_draft == min(DRAFT, NEW - done - 1), (b, done, n_draft)
            if way == "b":
                assert n_acc == n_draft and n_out == n_draft + 1, (b, done, n_draft, n_acc, n_out)
            if way == "c":
                assert n_acc == min(2, n_draft) and n_out == n_acc + 1, (b, done, n_draft, n_acc, n_out)
            if way == "d":
                assert n_acc == 0 and n_out == 1, (b, done, n_draft, n_acc, n_out)
    return acc, drafts


@pytest.mark.gpu
@pytest.mark.parametrize("way", ["a", "b", "c", "d"], ids=["lookup", "right", "third-wrong", "all-wrong"])
@pytest.mark.parametrize("mode", ["greedy", "mixed"])
@pytest.mark.parametrize("kind", ["fp16", "paged-fp8"])
def test_speculative_step_emits_the_sequential_stream(dev, model, prompts, kind, mode, way):
    """2 layers of 3_8b, vocab 4096, context 512, 4 slots, prompts of 5 / 17 / 40 / 64 tokens, 24 new tokens per slot, draft 4.
    _yardstick prints each yardstick's smallest winner / runner-up gap in units of the excuse threshold (see PROMPT_SEED)."""
    dtype, paged = (F8, True) if kind == "paged-fp8" else (F16, False)
    want, logits, _ = _yardstick(dev, model, prompts, dtype, mode)
    ss, _ = _spec_step(model, dev, prompts, dtype, paged, mode)
    got, records = _generate(ss, dev, want, way)
    acc, drafts = _judge(got, records, want, logits, prompts, MIXED if mode == "mixed" else GREEDY, way)
    print(f"{kind} {mode} {way}: {len(records)} steps for {NEW} tokens per slot, {acc} of {drafts} drafts accepted")
    if way == "b":
        assert len(records) == -(-NEW // (DRAFT + 1))  # 5 tokens per step and slot: 5 steps
    for b, p in enumerate(prompts):  # the state holds the whole sequence
        n = p.shape[0]
        assert int(ss.n_tok[b]) == n + NEW and ss.hist[b, :n + NEW].tolist() == p.tolist() + got[b]


@pytest.mark.gpu
def test_speculative_step_logprobs(dev, model, prompts):
    """a sampler with logprobs=True: the third return value holds, for every emitted token, token_logprobs' figure on its row"""
    ss, _ = _spec_step(model, dev, prompts, F16, False, "greedy")
    smp = qp.Sampler(NB, VOCAB, dev, logprobs=True, **MIXED)
    ss2 = qp.SpeculativeStep(model.layers, model.embed, model.norm, model.lm_head, ss.kcache, ss.vcache, model.inv_freq, draft=DRAFT,
                             sampler=smp)
    for b, p in enumerate(prompts):
        ss2.begin(b, p.tolist(), limit=p.shape[0] + NEW)
    out_tok, n_out, lp = ss2()
    rows = qp.token_logprobs(ss2.draw.logits, ss2.drawn, active=ss2.row_ctr)
    for b in range(NB):
        r, n = int(ss2.row0[b]), int(n_out[b])
        assert n >= 1 and torch.equal(lp[b, :n], rows[r:r + n]) and bool((lp[b, :n] <= 0).all()) and bool(torch.isfinite(lp[b, :n]).all())
        assert torch.equal(out_tok[b, :n], ss2.drawn[r:r + n])


@pytest.mark.gpu
def test_a_captured_step_replayed_to_the_end_and_a_new_sequence_between_replays(dev, model, prompts):
    """one captured ss(): replayed until every slot is at its limit, the stream is the eager stream; then a new sequence is begun in
    slot 1 and the same graph generates it, without recapture"""
    eager, begin_e = _spec_step(model, dev, prompts, F16, False, "greedy")
    want, _ = _generate(eager, dev, None, "a")
    ss, begin = _spec_step(model, dev, prompts, F16, False, "greedy")
    state = (ss.n_tok.clone(), ss.limit.clone())
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        ss.n_tok.zero_()  # the warm-up runs on a state without sequences: no row, no cache byte, no token
        ss()
        torch.cuda.synchronize()
        assert int(ss.n_out.sum()) == 0 and int(ss.row0[-1]) == 0
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            ss()
        ss.n_tok.copy_(state[0])
        got, records = _generate(ss, dev, None, "a", step=g.replay)
        assert got == want and len(records) <= NEW
        new = torch.randint(0, VOCAB, (23,), generator=torch.Generator().manual_seed(77)).to(dev)
        begin_e(1, new)
        want2, _ = _generate(eager, dev, None, "a", slots=[1])
        begin(1, new)
        got2, _ = _generate(ss, dev, None, "a", step=g.replay, slots=[1])
        torch.cuda.synchronize()
    assert len(got2[1]) == NEW and got2 == want2
    assert ss.hist[1, :23 + NEW].tolist() == new.tolist() + got2[1]
