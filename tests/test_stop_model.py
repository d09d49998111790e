"""`stop=` on the whole-model steps, on the small model of tests/model_reference.py.

(a) DecodeStep(stop=bank), captured and replayed n times with no host access, leaves in the bank the record of a host-driven loop of
    the plain step that applies stop.reference_stop_advance between steps: every field, greedy (argmax tail) and seeded, at B = 1 (the
    batch-1 step) and B = 3; one slot ends by a stop id, one by a stop string that spans two tokens, one by max_tokens, and the cache
    rows of a finished slot past its end_pos keep the bytes of a snapshot.
(b) SpeculativeStep(stop=bank) at draft 4 emits the stream of DecodeStep(stop=bank) and ends with its reason and text_len.  Three slots
    run free; the fourth follows a grammar that admits one token at a time, with a periodic prompt, so that prompt lookup drafts
    across its stop string (checked with reference_spec_draft) and the stop falls inside an accepted run.
(c) With a bank built with min_tokens=True no stop id is drawn before the bound, on both steps.
(d) launches_per_token: unchanged without stop=, + 1 with it, + 2 with the mask."""
import functools

import numpy as np
import pytest
import torch

import model_reference as mr
from qpalette_amd import stop as sp
from qpalette_amd.grammar import TokenTable
from qpalette_amd.speculative import reference_spec_draft

gpu = pytest.mark.gpu
CTX, NL, P, N, SENTINEL = 64, 2, 12, 14, 7.0
SEEDED = dict(temperature=[0.7, 1.0, 0.9, 1.3], top_k=[40, 0, 5, 3], top_p=[0.9, 0.95, 1.0, 1.0], seed=[11, 12, 13, 14])


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _model.cache_clear()


@functools.lru_cache(maxsize=None)
def _model():
    return mr.build("S", "mixed", (), NL, mr.VOCAB, 0, torch.device("cuda", 0))


def _table():
    """tokens 0 .. 63 are the single bytes "0" .. "o"; every other token has two bytes, of ranges no single-byte token uses"""
    toks = [bytes([48 + t]) if t < 64 else bytes([0x80 + (t >> 5), 0xA0 + (t & 31)]) for t in range(mr.VOCAB)]
    return TokenTable(toks, eos=mr.VOCAB - 1)


TABLE = _table()
FORCED_PROMPT = [0, 1, 2] * (P // 3)      # "012012..": the grammar below makes the model go on like this
FORCED_PATTERN, FORCED_STOP = "(012){20}", b"12"


def _bytes(tokens):
    return b"".join(TABLE.token(int(t)) for t in tokens)


def _prompts(B):
    g = torch.Generator().manual_seed(31)
    return [torch.randint(64, mr.VOCAB, (P,), generator=g) for _ in range(B)]


def _sampler(qp, dev, B, mode):
    if mode == "argmax":
        return None
    if mode == "greedy":
        return qp.Sampler(B, mr.VOCAB, dev, temperature=0.0)
    return qp.Sampler(B, mr.VOCAB, dev, **{k: v[:B] for k, v in SEEDED.items()})


class _Rig:
    """fresh caches filled with a sentinel, the prompts' first P - 1 tokens prefilled, the last one pending in tok / pos"""

    def __init__(self, qp, m, dev, prompts):
        B = len(prompts)
        nkv, hd = m.cfg.num_key_value_heads, m.cfg.head_dim
        self.kc = [torch.full((B, nkv, CTX, hd), SENTINEL, dtype=torch.float16, device=dev) for _ in m.layers]
        self.vc = [torch.full((B, nkv, CTX, hd), SENTINEL, dtype=torch.float16, device=dev) for _ in m.layers]
        self.args = (m.layers, m.embed, m.norm, m.lm_head, self.kc, self.vc, m.inv_freq)
        pf = qp.Prefill(*self.args, chunk=16)
        for b, p in enumerate(prompts):
            pf(p[:-1].to(dev), slot=b, pos0=0)
        self.tok0 = torch.tensor([int(p[-1]) for p in prompts], dtype=torch.long, device=dev)
        self.pos0 = torch.full((B,), P - 1, dtype=torch.long, device=dev)
        self.tok, self.pos = self.tok0.clone(), self.pos0.clone()
        self.out = torch.zeros(B, dtype=torch.long, device=dev)

    def untouched_rows(self, slot, first):
        """True if the cache rows of `slot` from position `first` on still hold the sentinel, in every layer"""
        return all(bool((c[slot, :, first:] == SENTINEL).all()) for c in self.kc + self.vc)


def _free_streams(qp, m, dev, prompts, mode, n=N, grammar=None):
    """the plain step driven from the host for n tokens, nothing stopping it: the streams the criteria are chosen from"""
    rig = _Rig(qp, m, dev, prompts)
    step = qp.DecodeStep(*rig.args, rig.tok, rig.pos, rig.out, sampler=_sampler(qp, dev, len(prompts), mode), grammar=grammar)
    streams = [[] for _ in prompts]
    for _ in range(n):
        step()
        for b, t in enumerate(rig.out.tolist()):
            streams[b].append(t)
        rig.tok.copy_(rig.out)
        rig.pos += 1
    return streams


def _criteria(streams, which):
    """per slot (stop strings or None, stop ids, max_tokens) of kind which[b]: 0 a stop id, 1 a stop string that spans two tokens, 2
    max_tokens, 3 the forced slot's string — chosen from the free streams so that every slot finishes inside the run"""
    crit = []
    for s, kind in zip(streams, which):
        if kind == 0:
            crit.append((None, (s[4], s[9]), 0))
        elif kind == 1:
            crit.append(([TABLE.token(s[3])[-1:] + TABLE.token(s[4]), b"never"], (), 0))
        elif kind == 2:
            crit.append((None, (), 6))
        else:
            crit.append(([FORCED_STOP], (), 0))
    return crit


def _bank(qp, dev, crit, **kw):
    bank = qp.StopBank(len(crit), TABLE, dev, sets=len(crit), max_states=32, cap=N + 4, **kw)
    for b, (strings, ids, max_tokens) in enumerate(crit):
        if strings is not None:
            bank.load(b, strings)
        bank.set(b, stop=None if strings is None else b, stop_ids=ids, max_tokens=max_tokens)
        bank.reset(b)
    return bank


def _host_loop(qp, m, dev, prompts, mode, bank, n=N):
    """the yardstick of (a): the PLAIN step, the host applying the contract between steps; returns (state, tok, pos, rig)"""
    rig = _Rig(qp, m, dev, prompts)
    step = qp.DecodeStep(*rig.args, rig.tok, rig.pos, rig.out, sampler=_sampler(qp, dev, len(prompts), mode))
    st, sets = bank.state(), list(bank.stops)
    tok, pos = rig.tok.cpu().numpy(), rig.pos.cpu().numpy()
    for _ in range(n):
        step()
        st, tok, pos = sp.reference_stop_advance(sets, TABLE, st, rig.out.cpu().numpy(), CTX, tok=tok, pos=pos)
        rig.tok.copy_(torch.from_numpy(tok))
        rig.pos.copy_(torch.from_numpy(pos))
    return st, tok, pos, rig


def _replayed(qp, m, dev, prompts, mode, bank, n=N):
    """DecodeStep(stop=bank) captured once and replayed n times; nothing is read before the last replay has run"""
    rig = _Rig(qp, m, dev, prompts)
    step = qp.DecodeStep(*rig.args, rig.tok, rig.pos, rig.out, sampler=_sampler(qp, dev, len(prompts), mode), stop=bank)
    torch.cuda.synchronize()       # the prefill and the bank's setters ran on the default stream
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        rig.pos.fill_(-1)          # the warm-up and the capture run on inactive slots: no cache byte, no record
        step()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            step()
        rig.tok.copy_(rig.tok0)
        rig.pos.copy_(rig.pos0)
        for _ in range(n):
            g.replay()
        torch.cuda.synchronize()
    return step, rig


@gpu
@pytest.mark.parametrize("mode", ["argmax", "seeded"])
@pytest.mark.parametrize("B", [1, 3])
def test_replayed_decode_step_leaves_the_host_loops_record(dev, B, mode):
    import qpalette_amd as qp
    m, prompts = _model(), _prompts(B)
    streams = _free_streams(qp, m, dev, prompts, mode)
    for which in ([[0, 1, 2]] if B == 3 else [[0], [1], [2]]):
        crit = _criteria(streams, which)
        ref, tok, pos, _ = _host_loop(qp, m, dev, prompts, mode, _bank(qp, dev, crit))
        bank = _bank(qp, dev, crit)
        before = bank.state()
        step, rig = _replayed(qp, m, dev, prompts, mode, bank)
        assert step.batch1 == (B == 1)
        got = bank.state()
        assert not ref.equal(got), (which, ref.equal(got), got.out, ref.out, got.reason, ref.reason)
        assert rig.tok.tolist() == tok.tolist() and rig.pos.tolist() == pos.tolist() == [-1] * B
        assert ref.reason.tolist() == [k + 1 for k in which], "every slot ends by the criterion it was given"
        assert int(ref.n_gen.max()) < N - 2, "the replays go on after the last slot has finished"
        assert before.equal(got) and "out" in before.equal(got)
        for b, kind in enumerate(which):
            n = int(ref.n_gen[b])
            assert ref.out[b, :n].tolist() == streams[b][:n], "a stopped stream is a prefix of the free one"
            assert int(ref.end_pos[b]) == P - 1 + n
            assert rig.untouched_rows(b, P - 1 + n) and not rig.untouched_rows(b, P - 2 + n), (b, n)
            res = bank.result(b)
            assert res["tokens"] == streams[b][:n] and res["reason"] == sp.REASONS[kind + 1] and res["end_pos"] == P - 1 + n
            if kind == 0:
                assert res["tokens"][-1] in crit[b][1] and res["text"] == _bytes(streams[b][:n - 1]) and res["stop"] is None
            if kind == 1:
                assert res["stop"] == crit[b][0][0] and n >= 2
                text = _bytes(streams[b][:n])
                assert text.endswith(res["stop"]) and res["text"] == text[:-len(res["stop"])]
                assert len(TABLE.token(streams[b][n - 1])) < len(res["stop"]), "the match spans two tokens"
            if kind == 2:
                assert n == 6 and res["text"] == _bytes(streams[b][:n])


def _speculative(qp, m, dev, prompts, mode, bank, grammar=None):
    """SpeculativeStep(stop=bank) at draft 4 until every slot has finished; returns (streams, per step (n_out, n_acc) lists)"""
    rig = _Rig(qp, m, dev, prompts)
    ss = qp.SpeculativeStep(*rig.args, draft=4, gram=(2, 4), sampler=_sampler(qp, dev, len(prompts), mode), grammar=grammar, stop=bank)
    for b, p in enumerate(prompts):
        ss.begin(b, p.tolist(), limit=CTX)
    got, steps = [[] for _ in prompts], []
    for _ in range(N + 2):
        if not bool((ss.n_tok < ss.limit).any()):
            break
        out, n_out = ss()[:2]
        n_out = n_out.tolist()
        steps.append((n_out, ss.n_acc.tolist()))
        for b in range(len(prompts)):
            got[b] += out[b, :n_out[b]].tolist()
    assert not bool((ss.n_tok < ss.limit).any()), "a slot did not finish"
    return got, steps, ss


@gpu
@pytest.mark.parametrize("mode", ["greedy", "seeded"])
def test_speculative_step_stops_where_the_decode_step_stops(dev, mode):
    import qpalette_amd as qp
    m = _model()
    prompts = _prompts(3) + [torch.tensor(FORCED_PROMPT)]
    which = [0, 1, 2, 3]

    def grammar():
        bank = qp.GrammarBank(4, TABLE, dev, grammars=1, max_states=64)
        bank.load(0, FORCED_PATTERN)
        bank.set(3, 0)
        return bank

    # on the CPU: prompt lookup drafts across the forced slot's stop string
    d = reference_spec_draft(np.array([FORCED_PROMPT + [0] * (CTX - P)]), [P], [CTX], 4, 2, 4, 5, CTX)
    drafts = d["tokens"][1:1 + int(d["n_draft"][0])].tolist()
    assert drafts == [0, 1, 2] and FORCED_STOP in _bytes(drafts) and all(len(TABLE.token(t)) == 1 for t in drafts)
    streams = _free_streams(qp, m, dev, prompts, mode, grammar=grammar())
    assert streams[3][:6] == [0, 1, 2, 0, 1, 2], "the grammar admits one token at a time"
    crit = _criteria(streams, which)
    # (a)'s step, driven from the host
    bank = _bank(qp, dev, crit)
    rig = _Rig(qp, m, dev, prompts)
    step = qp.DecodeStep(*rig.args, rig.tok, rig.pos, rig.out, sampler=_sampler(qp, dev, 4, mode), grammar=grammar(), stop=bank)
    for _ in range(N):
        step()
    want = bank.state()
    assert want.reason.tolist() == [1, 2, 3, 2] and rig.pos.tolist() == [-1] * 4
    # the speculative step
    bank2 = _bank(qp, dev, crit)
    got, steps, ss = _speculative(qp, m, dev, prompts, mode, bank2, grammar=grammar())
    have = bank2.state()
    for b in range(4):
        n = int(want.n_gen[b])
        assert got[b] == want.out[b, :n].tolist() == have.out[b, :n].tolist(), (b, got[b], want.out[b, :n])
    for name in ("n_gen", "reason", "text_len", "gen_bytes", "hit", "end_pos", "ac_state"):
        assert np.array_equal(getattr(have, name), getattr(want, name)), name
    assert ss.n_tok.tolist() == ss.limit.tolist() == [P + int(n) for n in want.n_gen]
    # the forced slot: its first step accepts the drafts "0", "1", "2" and the stop string ends at the third emitted token
    (n_out, n_acc) = steps[0]
    assert n_acc[3] == 3 and n_out[3] == 3 and got[3] == [0, 1, 2], "the run of 4 is cut behind the accepted draft that ends the match"
    assert bank2.result(3)["stop"] == FORCED_STOP and bank2.result(3)["text"] == b"0"
    assert int(ss.grammar.state[3]) == int(step.grammar.state[3]), "the grammar saw the cut run"


@gpu
def test_no_stop_id_before_min_tokens(dev):
    import qpalette_amd as qp
    m, prompts, mode = _model(), _prompts(3), "seeded"
    streams = _free_streams(qp, m, dev, prompts, mode)
    bound = [5, 3, 0]

    def bank():
        bk = qp.StopBank(3, TABLE, dev, sets=1, max_states=8, cap=N + 4, min_tokens=True)
        for b in range(3):   # the ids the free stream draws first: without the mask slot b would stop at once
            bk.set(b, stop_ids=streams[b][:3], min_tokens=bound[b], max_tokens=10)
            bk.reset(b)
        return bk

    bk = bank()
    step, rig = _replayed(qp, m, dev, prompts, mode, bk)
    st = bk.state()
    for b in range(3):
        n, ids = int(st.n_gen[b]), set(streams[b][:3])
        assert n >= max(bound[b], 1) and not ids & set(st.out[b, :bound[b]].tolist()), (b, st.out[b, :n], ids)
        assert st.reason[b] in (sp.STOP_ID, sp.MAX_TOKENS) and (st.reason[b] != sp.STOP_ID or int(st.out[b, n - 1]) in ids)
    assert st.n_gen[2] == 1 and st.reason[2] == sp.STOP_ID and st.out[2, 0] == streams[2][0], "no bound: the first token stops the slot"
    assert st.out[0, 0] != streams[0][0], "the mask changed the first draw of a slot whose first free token is a stop id"
    # the speculative step: the same record (row j of a segment is masked as the j-th token from now)
    bk2 = bank()
    got, _, _ = _speculative(qp, m, dev, prompts, mode, bk2)
    st2 = bk2.state()
    for name in ("n_gen", "reason", "out", "text_len"):
        assert np.array_equal(getattr(st2, name), getattr(st, name)), (name, getattr(st2, name), getattr(st, name))


@gpu
def test_launch_counts(dev):
    import qpalette_amd as qp
    m = _model()
    rig = _Rig(qp, m, dev, _prompts(3))
    smp = qp.Sampler(3, mr.VOCAB, dev, temperature=0.0)
    plain_bank = qp.StopBank(3, TABLE, dev, sets=1, max_states=8, cap=8)
    mask_bank = qp.StopBank(3, TABLE, dev, sets=1, max_states=8, cap=8, min_tokens=True)
    mk = lambda **kw: qp.DecodeStep(*rig.args, rig.tok, rig.pos, rig.out, **kw)   # noqa: E731
    per_layer = 9   # H = 512: a rotation launch in front of q|k|v, o and up|gate
    assert mk().launches_per_token == per_layer * NL + 1 and mk(sampler=smp).launches_per_token == per_layer * NL + 2
    assert mk(stop=plain_bank).launches_per_token == mk().launches_per_token + 1
    assert mk(sampler=smp, stop=plain_bank).launches_per_token == mk(sampler=smp).launches_per_token + 1
    assert mk(sampler=smp, stop=mask_bank).launches_per_token == mk(sampler=smp).launches_per_token + 2
    QpalError = qp._native.QpalError
    with pytest.raises(QpalError, match="min_tokens mask"):
        mk(stop=mask_bank)
    with pytest.raises(QpalError, match="StopBank of 3 slots"):
        mk(stop=qp.StopBank(2, TABLE, dev))
    with pytest.raises(QpalError, match="no stop bank on a ragged step"):
        qp.RaggedStep(*rig.args, rows=16, segments=3, stop=plain_bank)
    for cls in (qp.Prefill, qp.Score):
        with pytest.raises(TypeError):
            cls(*rig.args, stop=plain_bank)
    # the launches themselves: a step with stop= issues the plain step's C-ABI calls and qpal_stop_advance behind them
    calls = []
    lib = qp._native.lib()

    class Spy:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if not name.startswith("qpal_") or name.endswith("_bytes"):
                return fn

            def call(*a):
                calls.append(name)
                return fn(*a)
            return call

    rig.pos.fill_(-1)
    orig = qp._native.lib
    qp._native.lib = lambda: Spy()
    try:
        mk(sampler=smp)()
        plain, calls = calls, []
        mk(sampler=smp, stop=mask_bank)()
    finally:
        qp._native.lib = orig
    assert calls[-1] == "qpal_stop_advance" and calls.count("qpal_stop_mask") == 1
    assert calls.index("qpal_stop_mask") == calls.index("qpal_sample") - 1
    assert [c for c in calls if not c.startswith("qpal_stop_")] == plain
    torch.cuda.synchronize()
