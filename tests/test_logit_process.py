"""Logit processors on the GPU (csrc/logit_proc.hip, qpalette_amd.logits, the `processor=` of the step classes).

Kernels: qpal_logit_process bit for bit logits.reference_process (tests/test_logit_process_contract.py holds that to hand-made rows),
in place and out of place, on 16-byte aligned rows and on rows that are not, two launches bitwise equal; qpal_logit_observe equal to
np.add.at.  Whole model (tests/test_spec.py's model, prompts, generation loop and near-tie rule, loaded from that file): a neutral
processor changes no bit of DecodeStep, Prefill and SpeculativeStep; with a different processor in every slot the mask is never
left, the counts are the histogram of the tokens, and SpeculativeStep emits the stream of sequential Prefill + DecodeStep sampling;
captured steps obey set_mask / set between replays."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import qpalette_amd as qp
from qpalette_amd import logits as lg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- kernels

def _random_state(rng, slots, vocab, bias_slots):
    """per-slot mixed parameters: every fourth slot neutral, repetition above and below 1, masks on odd slots, bias_n cycling through
    0, 1, bias_slots; counts mostly zero, some up to 5"""
    st = dict(count=(rng.integers(0, 6, size=(slots, vocab)) * (rng.random((slots, vocab)) < 0.3)).astype(np.int32),
              repetition=np.ones(slots, F32), presence=np.zeros(slots, F32), frequency=np.zeros(slots, F32),
              mask=rng.integers(0, 2 ** 32, size=(slots, (vocab + 31) // 32), dtype=np.uint64).astype(np.uint32),
              mask_on=np.zeros(slots, np.int32), bias_id=np.zeros((slots, bias_slots), np.int32),
              bias_val=rng.normal(0, 4, size=(slots, bias_slots)).astype(F32), bias_n=np.zeros(slots, np.int32))
    for b in range(slots):
        if b % 4 != 3:
            st["repetition"][b] = (1.3, 0.8, 1.0)[b % 3]
            st["presence"][b], st["frequency"][b] = ((0.5, 0.3), (0.0, 0.7), (0.25, 0.0))[(b // 3) % 3]
        st["mask_on"][b] = b % 2
        st["bias_id"][b] = rng.choice(vocab, size=bias_slots, replace=False)
        st["bias_n"][b] = (bias_slots, 0, 1)[b % 3]
    return st


def _processor(dev, st, vocab, bias_slots):
    p = qp.LogitProcessor(st["count"].shape[0], vocab, dev, bias_slots=bias_slots)
    for name in ("count", "repetition", "presence", "frequency", "mask_on", "bias_id", "bias_val", "bias_n"):
        getattr(p, name).copy_(torch.from_numpy(st[name]))
    p.mask.copy_(torch.from_numpy(st["mask"].view(np.int32)))
    return p


def _random_logits(rng, rows, vocab, ld):
    """N(0, 2.5^2) with a few -inf and NaN entries; columns vocab .. ld hold a sentinel"""
    l = np.full((rows, ld), -77.0, F32)
    l[:, :vocab] = rng.normal(0, 2.5, size=(rows, vocab))
    for r in range(rows):
        l[r, rng.integers(0, vocab, size=3)] = (-np.inf, np.nan, -np.inf)
    return l


def _segments(rows):
    """rows cut into segments of 16, 1, 5, 9, 16, 3, ... rows (0 .. 15 extras) and one slot without rows: (row_slot, row0, slots)"""
    row0, at, lengths = [0], 0, (16, 1, 5, 9, 16, 3)
    while at < rows:
        if len(row0) == 3:
            row0.append(at)  # slot 2 has no rows
        at = min(rows, at + lengths[(len(row0) - 1) % len(lengths)])
        row0.append(at)
    slots = len(row0) - 1
    row_slot = np.zeros(rows, np.int32)
    for b in range(slots):
        row_slot[row0[b]:row0[b + 1]] = b
    return row_slot, np.array(row0, np.int32), slots


CASES = [(1, 33), (5, 33), (128, 33), (1, 1000), (5, 1000), (128, 1000), (5, 4099), (128, 4099), (2, 128256)]


@pytest.mark.gpu
@pytest.mark.parametrize("spec", [False, True], ids=["rows", "segments"])
@pytest.mark.parametrize("wide", [False, True], ids=["ld=vocab", "ld>vocab"])
@pytest.mark.parametrize("rows,vocab", CASES)
def test_process_kernel_is_the_reference(dev, rows, vocab, wide, spec):
    """vocab 33: one full mask word and one bit; 4099 with ld = vocab: rows that are not 16-byte aligned (single loads); ld > vocab (a
    multiple of 4): aligned logits rows, the row's last group by single loads, sentinel columns kept; 128 256: 32 tiles per row.
    Out of place into a sentinel-filled buffer (inactive rows and the columns past vocab keep it), twice (bitwise equal), then in place."""
    rng = np.random.default_rng(1000 * rows + vocab + 7 * wide + spec)
    ld = (vocab + 3) // 4 * 4 + 4 if wide else vocab
    bias_slots = 8 if vocab < 100 else 64
    l = _random_logits(rng, rows, vocab, ld)
    if spec:
        row_slot, row0, slots = _segments(rows)
        # guesses from a handful of tokens, so that extras repeat and meet counted tokens; some are no token of the vocabulary
        tokens = rng.choice(np.concatenate([rng.integers(0, vocab, size=6), [vocab, 2 ** 30 - 1]]), size=rows).astype(np.int64)
        ctr = np.arange(rows, dtype=np.int64) + 100
        if rows > 3:
            ctr[2] = -1                                                 # an inactive row inside a segment
        kw = dict(tokens=tokens, row0=row0)
    else:
        slots = 1 if rows == 1 else 6
        row_slot = rng.integers(0, slots, size=rows).astype(np.int32)  # several rows share a slot
        ctr = rng.integers(0, 1 << 40, size=rows)
        if rows > 3:
            row_slot[1], ctr[3] = -1, -1                                # inactive rows keep the sentinel
        if rows > 5:
            row_slot[9] = slots
        kw = {}
    st = _random_state(rng, slots, vocab, bias_slots)
    sent = np.full((rows, ld), 55.0, F32)
    ref = lg.reference_process(l, row_slot, ctr, out=sent, vocab=vocab, **st, **kw)
    proc = _processor(dev, st, vocab, bias_slots)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    gkw = {k: t(v) for k, v in kw.items()}
    lin, outs = t(l), []
    for _ in range(2):
        out = t(sent)
        assert lg.process(lin, proc, t(row_slot), t(ctr), out=out, **gkw) is out
        outs.append(out.cpu().numpy())
    assert np.array_equal(_bits(lin.cpu().numpy()), _bits(l)), "out of place: the input is not written"
    bad = np.argwhere(_bits(outs[0]) != _bits(ref))
    assert bad.shape[0] == 0, (bad[:5], [(outs[0][r, i], ref[r, i], l[r, i]) for r, i in bad[:5]])
    assert np.array_equal(_bits(outs[1]), _bits(outs[0])), "two launches on one state"
    ref_in = lg.reference_process(l, row_slot, ctr, vocab=vocab, **st, **kw)  # in place: inactive rows keep their logits
    assert lg.process(lin, proc, t(row_slot), t(ctr), **gkw) is lin
    assert np.array_equal(_bits(lin.cpu().numpy()), _bits(ref_in))
    # the case shows what it is meant to show
    act = (row_slot >= 0) & (row_slot < slots) & (ctr >= 0)
    assert np.all(ref[~act] == 55.0) and np.all(ref[:, vocab:] == 55.0) and np.isnan(ref[act]).any() and np.isneginf(ref[act]).any()
    if rows > 3:
        assert (~act).any() and (_bits(ref[act][:, :vocab]) != _bits(l[act][:, :vocab])).any()
    if spec and rows >= 5:
        plain = lg.reference_process(l, row_slot, ctr, out=sent, vocab=vocab, **st)
        assert (_bits(plain) != _bits(ref)).any(), "no extra changed a logit"


@pytest.mark.gpu
def test_process_kernel_neutral_state_keeps_every_bit(dev):
    rows, vocab = 5, 4099
    rng = np.random.default_rng(3)
    l = _random_logits(rng, rows, vocab, vocab)
    proc = qp.LogitProcessor(rows, vocab, dev)
    proc.count.copy_(torch.from_numpy(rng.integers(0, 3, size=(rows, vocab)).astype(np.int32)))
    lin = torch.from_numpy(l).to(dev)
    lg.process(lin, proc, torch.arange(rows, dtype=torch.int32, device=dev), torch.zeros(rows, dtype=torch.int64, device=dev))
    assert np.array_equal(_bits(lin.cpu().numpy()), _bits(l))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 128, 2048])
def test_observe_kernel_is_add_at(dev, n):
    """repeated (slot, token) pairs (tokens from a range of 9), tokens outside the vocabulary, slots outside the processor's and
    inactive rows; then one slot for all rows"""
    slots, vocab = 5, 1000
    rng = np.random.default_rng(n)
    tokens = rng.integers(-2, 9, size=n) * 111               # -222, -111: outside; 0 .. 888
    tokens[rng.random(n) < 0.05] = vocab                     # the first id past the vocabulary
    slot = rng.integers(-1, slots + 1, size=n).astype(np.int32)
    active = np.where(rng.random(n) < 0.2, -1, rng.integers(0, 1 << 40, size=n))
    if n == 1:
        tokens[0], slot[0], active[0] = 888, slots - 1, 0
    start = rng.integers(0, 3, size=(slots, vocab)).astype(np.int32)
    ref = lg.reference_observe(start, slot, tokens, active=active)
    proc = qp.LogitProcessor(slots, vocab, dev)
    proc.count.copy_(torch.from_numpy(start))
    t = lambda a, dt: torch.as_tensor(a, dtype=dt).to(dev)
    lg.observe(proc, t(tokens, torch.int64), t(slot, torch.int32), active=t(active, torch.int64))
    assert np.array_equal(proc.count.cpu().numpy(), ref)
    if n > 1:
        assert int((ref - start).max()) >= 2 and int((ref - start).sum()) < n, "no pair repeated, or nothing was skipped"
    ref2 = lg.reference_observe(ref, 3, tokens)
    lg.observe(proc, t(tokens, torch.int64), 3)
    assert np.array_equal(proc.count.cpu().numpy(), ref2)
    proc.count_tokens(1, [5, 5, 999])
    ref2[1, 5] += 2
    ref2[1, 999] += 1
    assert np.array_equal(proc.count.cpu().numpy(), ref2)


# -------------------------------------------------------------------------------------------------------- whole model

def _load_spec_tests():
    """tests/test_spec.py as a module: its model, prompts, generation loop and near-tie rule are this file's too"""
    spec = importlib.util.spec_from_file_location("_spec_tests_for_logit_process", os.path.join(ROOT, "tests", "test_spec.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ts = _load_spec_tests()
NB, L, NEW, DRAFT, VOCAB, F16 = ts.NB, ts.L, ts.NEW, ts.DRAFT, ts.VOCAB, ts.F16
# Recorded on an MI355X with prompt seed 31 (tests/test_spec.py's default): the yardsticks' smallest winner / runner-up gap on the
# PROCESSED logits, in units of the excuse threshold, is 0.228 (greedy) and 0.270 (mixed).  Below 1, so an excuse can occur and the
# 5 % budget of _judge is what binds; in the recorded run no excuse was taken — all four comparisons are equal token for token — so
# the default seed stays and that file's search over the seeds 31 .. 60 was not needed.
PROMPT_SEED = ts.PROMPT_SEED
ALLOWED = np.sort(np.random.default_rng(22).choice(VOCAB, size=256, replace=False))  # slot 2's mask
BIASED = (int(ALLOWED[3]), int(ALLOWED[200]))                                        # + 4 on two allowed tokens


@pytest.fixture(scope="module")
def model(dev):
    sys.path.insert(0, os.path.join(ROOT, "perf"))
    from decode_llama import build_model
    return build_model("3_8b", "tcomb_6_7_0.5_none_0.9", None, 2, VOCAB, dev)


@pytest.fixture(scope="module")
def prompts(dev):
    g = torch.Generator().manual_seed(PROMPT_SEED)
    return [torch.randint(0, VOCAB, (n,), generator=g).to(dev) for n in ts.PROMPT_LENGTHS]


def _configured(dev, neutral=False):
    """slot 0: repetition 1.3; slot 1: presence 0.5, frequency 0.3; slot 2: a mask of 256 ids and + 4 on two of them; slot 3: neutral"""
    proc = qp.LogitProcessor(NB, VOCAB, dev)
    if not neutral:
        proc.set(0, repetition=1.3)
        proc.set(1, presence=0.5, frequency=0.3)
        proc.set_mask(2, ALLOWED)
        proc.set_bias(2, {BIASED[0]: 4.0, BIASED[1]: 4.0})
    return proc


def _params(mode):
    return ts.MIXED if mode == "mixed" else ts.GREEDY


def _sequential(dev, m, prompts, mode, proc, chunk=128):
    """Prefill draws the first new token, DecodeStep(generic=True) the rest (test_spec's yardstick, with a processor or None).
    Returns (streams, logits as the sampler held them after each draw, the sampler)."""
    kc, vc = ts._caches(m, dev, F16)
    smp = qp.Sampler(NB, VOCAB, dev, **_params(mode))
    pf = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, chunk=chunk, sampler=smp, processor=proc)
    tok = torch.zeros(NB, dtype=torch.long, device=dev)
    streams, logits = [[] for _ in range(NB)], [[] for _ in range(NB)]
    for b, p in enumerate(prompts):
        tok[b] = pf(p, slot=b, pos0=0)[0]
        logits[b].append(smp.logits[b].cpu().numpy().copy())
        streams[b].append(int(tok[b]))
    pos = torch.tensor([p.shape[0] for p in prompts], dtype=torch.long, device=dev)
    out = torch.zeros(NB, dtype=torch.long, device=dev)
    ds = qp.DecodeStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, tok, pos, out, generic=True, sampler=smp, processor=proc)
    assert ds.launches_per_token == 9 * len(m.layers) + 2 + (2 if proc is not None else 0)
    for _ in range(NEW - 1):
        ds()
        lgts = smp.logits.cpu().numpy()
        for b in range(NB):
            streams[b].append(int(out[b]))
            logits[b].append(lgts[b].copy())
        tok.copy_(out)
        pos += 1
    return streams, logits, smp


_YARD = {}


def _yardstick(dev, m, prompts, mode):
    """the sequential streams under the configured processor, once per sampling mode; prints the smallest winner / runner-up gap of
    any draw on the processed logits, in units of the excuse threshold, as tests/test_spec.py does"""
    if mode not in _YARD:
        proc = _configured(dev)
        streams, logits, _ = _sequential(dev, m, prompts, mode, proc)
        gap = np.inf
        for b in range(NB):
            for i in range(NEW):
                s = ts._scores(logits[b][i], _params(mode), b, prompts[b].shape[0] - 1 + i)
                assert int(np.argmax(s)) == streams[b][i]
                s = np.sort(s)
                gap = min(gap, float(s[-1] - s[-2]) / (2 * ts._bound(logits[b][i])))
        print(f"yardstick with processors, {mode}, prompt seed {PROMPT_SEED}: smallest winner / runner-up gap = {gap:.3f} x the excuse threshold")
        _YARD[mode] = (streams, logits, proc.count.cpu().numpy())
    return _YARD[mode]


def _spec_step(m, dev, prompts, mode, proc):
    """tests/test_spec.py's _spec_step on fp16 caches, with a processor: prompts[b][:-1] prefilled (no processor: begin counts)"""
    kr, vr = ts._caches(m, dev, F16)
    pf = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kr, vr, m.inv_freq, chunk=128)
    smp = qp.Sampler(NB, VOCAB, dev, **_params(mode)) if mode == "mixed" else None
    ss = qp.SpeculativeStep(m.layers, m.embed, m.norm, m.lm_head, kr, vr, m.inv_freq, draft=DRAFT, gram=(2, 4), sampler=smp, processor=proc)
    for b, p in enumerate(prompts):
        pf(p[:-1], slot=b, pos0=0)
        ss.begin(b, p.tolist(), limit=p.shape[0] + NEW)
    return ss


@pytest.mark.gpu
def test_a_neutral_processor_changes_no_bit(dev, model, prompts, monkeypatch):
    """(a) Prefill, DecodeStep and SpeculativeStep with a fresh LogitProcessor.  The batched projections accumulate with float atomics
    (DESIGN.md §15.4): two runs of one step agree to rounding only, with or without a processor, so "the same step without one" is
    the same run — the logits the lm_head wrote against what the process launch left in their place, bit for bit, and the step's
    tokens against a draw from a copy of the unprocessed logits.  (Prompts in chunks of 16 rows: counted chunk by chunk.)"""
    calls, real = [], lg.process

    def spy(logits, proc, row_slot, ctr, **kw):
        before = logits.clone()
        real(logits, proc, row_slot, ctr, **kw)
        calls.append((before, logits.clone(), ctr.clone()))
        return logits
    monkeypatch.setattr(lg, "process", spy)
    proc = _configured(dev, neutral=True)
    streams, _, smp = _sequential(dev, model, prompts, "mixed", proc, chunk=16)
    assert len(calls) == NB + NEW - 1, "one process launch per Prefill call and per DecodeStep"
    for i, (before, after, ctr) in enumerate(calls):
        assert torch.equal(before.view(torch.int32), after.view(torch.int32)), i
        if i < NB:   # Prefill of slot i: one row
            assert qp.sample(before, smp.slot(i), ctr).tolist() == [streams[i][0]]
        else:
            assert qp.sample(before, smp, ctr).tolist() == [streams[b][i - NB + 1] for b in range(NB)]
    assert int(proc.count.sum()) == sum(p.shape[0] for p in prompts) + NB * (NEW - 1), "a neutral processor still counts what is fed"
    del calls[:]
    ss = _spec_step(model, dev, prompts, "mixed", _configured(dev, neutral=True))
    got, records = ts._generate(ss, dev, None, "a")
    assert len(calls) == len(records) and all(len(g) == NEW for g in got)
    assert all(torch.equal(before.view(torch.int32), after.view(torch.int32)) for before, after, _ in calls)
    before, _, ctr = calls[-1]   # ss.draw still holds the last step's gathered parameters
    assert torch.equal(qp.sample(before, ss.draw, ctr, out=ss.drawn.clone()), ss.drawn)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["greedy", "mixed"])
def test_sequential_generation_with_processors(dev, model, prompts, mode):
    """(b), the yardstick itself: no token of slot 2 outside its mask, the counts are the histogram of what was fed — the prompt and
    every emitted token but the last, which no step has fed yet — and the processors changed the streams"""
    streams, logits, count = _yardstick(dev, model, prompts, mode)
    assert set(streams[2]) <= set(ALLOWED.tolist())
    for b, p in enumerate(prompts):
        assert np.array_equal(count[b], np.bincount(p.tolist() + streams[b][:-1], minlength=VOCAB)), b
    assert all(np.all(np.isneginf(l[np.setdiff1d(np.arange(VOCAB), ALLOWED)])) for l in logits[2])
    plain, _, _ = _sequential(dev, model, prompts, mode, None)
    assert not set(plain[2]) <= set(ALLOWED.tolist()) and plain[:3] != streams[:3], "the processors bind"


@pytest.mark.gpu
@pytest.mark.parametrize("way", ["a", "c"], ids=["lookup", "third-wrong"])
@pytest.mark.parametrize("mode", ["greedy", "mixed"])
def test_speculative_step_with_processors_emits_the_sequential_stream(dev, model, prompts, mode, way):
    """(b) tests/test_spec.py's comparison and near-tie rule (_judge: excuse threshold and the 5 % cap as they are there), the scores
    taken from the PROCESSED logits the yardstick's sampler held.  No token any step emits for slot 2 lies outside its mask.  At the
    end: count[b] = the histogram of prompt + emitted tokens, exactly."""
    want, logits, _ = _yardstick(dev, model, prompts, mode)
    proc = _configured(dev)
    ss = _spec_step(model, dev, prompts, mode, proc)
    got, records = ts._generate(ss, dev, want, way)
    assert set(got[2]) <= set(ALLOWED.tolist()), "every token any step emitted for slot 2 lies in its mask"
    acc, drafts = ts._judge(got, records, want, logits, prompts, _params(mode), way)
    print(f"processors {mode} {way}: {len(records)} steps for {NEW} tokens per slot, {acc} of {drafts} drafts accepted")
    count = proc.count.cpu().numpy()
    for b, p in enumerate(prompts):
        n = p.shape[0]
        assert int(ss.n_tok[b]) == n + NEW and ss.hist[b, :n + NEW].tolist() == p.tolist() + got[b]
        assert np.array_equal(count[b], np.bincount(p.tolist() + got[b], minlength=VOCAB)), b


@pytest.mark.gpu
def test_captured_steps_obey_the_processor_between_replays(dev, model, prompts):
    """(c) one captured DecodeStep and one captured SpeculativeStep; set_mask / set between replays change the next draw"""
    kc, vc = ts._caches(model, dev, F16)
    smp, proc = qp.Sampler(NB, VOCAB, dev, temperature=0.0), qp.LogitProcessor(NB, VOCAB, dev)
    tok = torch.tensor([5, 6, 7, 8], dtype=torch.long, device=dev)
    pos, out = torch.zeros(NB, dtype=torch.long, device=dev), torch.zeros(NB, dtype=torch.long, device=dev)
    ds = qp.DecodeStep(model.layers, model.embed, model.norm, model.lm_head, kc, vc, model.inv_freq, tok, pos, out, generic=True,
                       sampler=smp, processor=proc)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        ds()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            ds()
        g.replay()
        torch.cuda.synchronize()
        free = out.tolist()
        only = (free[0] + 1) % VOCAB
        proc.set_mask(0, [only])
        proc.set(1, presence=1e4)       # whatever slot 1 has counted is out of reach
        proc.count[1, free[1]] += 1     # ... its favourite among them
        proc.set_bias(3, {(free[3] + 7) % VOCAB: 1e4})
        g.replay()
        torch.cuda.synchronize()
        now = out.tolist()
        assert now[0] == only and now[1] != free[1] and int(proc.count[1, now[1]]) == 0 and now[2] == free[2]
        assert now[3] == (free[3] + 7) % VOCAB
        assert int(proc.count[2, 7]) == 3, "the warm-up and two replays each counted the fed token"
        proc.set_mask(0, None)
        proc.set(1, presence=0.0)
        proc.set_bias(3, None)
        g.replay()
        torch.cuda.synchronize()
        assert out.tolist() == free

        # ---- the speculative step: a mask of one token in slot 1, from the second replay on
        proc2 = qp.LogitProcessor(NB, VOCAB, dev)
        ss = _spec_step(model, dev, prompts, "greedy", proc2)
        state = ss.n_tok.clone()
        ss.n_tok.zero_()  # warm-up and capture on a state without sequences
        ss()
        torch.cuda.synchronize()
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2, stream=s):
            ss()
        ss.n_tok.copy_(state)
        g2.replay()
        torch.cuda.synchronize()
        first = [ss.out_tok[b, :int(ss.n_out[b])].tolist() for b in range(NB)]
        assert all(len(f) >= 1 for f in first)
        proc2.set_mask(1, [1234])
        proc2.set(2, repetition=1.3, presence=1e4)
        seen = set(prompts[2].tolist()) | set(first[2])
        for _ in range(3):
            g2.replay()
            torch.cuda.synchronize()
            assert set(ss.out_tok[1, :int(ss.n_out[1])].tolist()) == {1234}
            new = ss.out_tok[2, :int(ss.n_out[2])].tolist()
            assert len(new) >= 1 and not set(new) & seen and len(set(new)) == len(new), "slot 2 may repeat nothing"
            seen |= set(new)
        for b, p in enumerate(prompts):
            n = int(ss.n_tok[b])
            assert np.array_equal(proc2.count[b].cpu().numpy(), np.bincount(ss.hist[b, :n].cpu().numpy(), minlength=VOCAB))


@pytest.mark.gpu
def test_steps_refuse_a_processor_they_cannot_serve(dev, model):
    kc, vc = ts._caches(model, dev, F16)
    m, E = model, qp._native.QpalError
    proc = qp.LogitProcessor(NB, VOCAB, dev)
    with pytest.raises(E, match="no processor on a ragged step"):
        qp.RaggedStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, sampler=qp.Sampler(NB, VOCAB, dev), processor=proc)
    with pytest.raises(E, match="give the step a sampler"):
        qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, processor=proc)
    with pytest.raises(E, match="LogitProcessor of 4 slots"):
        qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, sampler=qp.Sampler(NB, VOCAB, dev),
                   processor=qp.LogitProcessor(NB + 1, VOCAB, dev))
