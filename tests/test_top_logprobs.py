"""qpal_top_logprob on the GPU, the sampled tails with top_logprobs, and decoder.Score(top_logprobs=n).

The kernel is judged on the logits it was given by sampling.reference_top_logprobs (numpy fp64), no case excluded:
  * ids exact;
  * finite log-probs and lse within delta = 2^-15 + 2^-22 * max|l| of the fp64 value — the bound tests/test_score.py derives for
    this arithmetic (the same maximum, exp-sum and fp64 combine); infinite values are matched exactly;
  * every listed value bitwise equal to token_logprobs (the existing kernel) for that token on the same buffer.
The layers of a step are not bitwise reproducible from run to run (the batched projections accumulate with float atomics), so two
runs of a step are compared through the logits each of them left: what the tail computes is a function of those."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from qpalette_amd import sampling

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_spec():
    """tests/test_top_logprobs_spec.py as a module: its planted rows are this file's too"""
    spec = importlib.util.spec_from_file_location("_top_logprobs_spec_rows", os.path.join(ROOT, "tests", "test_top_logprobs_spec.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ts = _load_spec()
KINDS = ts.KINDS


@pytest.fixture(scope="module")
def qp():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import qpalette_amd
    qpalette_amd._native.lib()
    return qpalette_amd


@pytest.fixture(scope="module")
def model(qp):
    sys.path.insert(0, os.path.join(ROOT, "perf"))
    from decode_llama import build_model
    return build_model("3_8b", "tcomb_6_7_0.5_none_0.9", None, 2, 4096, torch.device("cuda", 0))


def delta_of(row):
    l = sampling.clean_logits(row)
    fin = np.isfinite(l)
    return 2.0 ** -15 + 2.0 ** -22 * (float(np.abs(l[fin]).max()) if fin.any() else 0.0)


def bits(t):
    return t.contiguous().view(torch.int32)


def check_lists(row, n, ids, lp, lse, what):
    """one row's lists against reference_top_logprobs; returns the worst error as a share of delta"""
    want_ids, want_lp, want_lse = sampling.reference_top_logprobs(row, n)
    assert np.array_equal(np.asarray(ids), want_ids), (what, np.asarray(ids).tolist(), want_ids.tolist())
    d, worst = delta_of(row), 0.0
    pairs = [(f"logprob[{j}]", lp[j], want_lp[j]) for j in range(n)] + ([] if lse is None else [("lse", lse, want_lse)])
    for name, got, ref in pairs:
        if np.isinf(ref):
            assert got == ref, (what, name, got, ref)
        else:
            assert np.isfinite(got) and abs(float(got) - ref) <= d, (what, name, float(got), ref, abs(float(got) - ref), d)
            worst = max(worst, abs(float(got) - ref) / d)
    return worst


def padded(host, dev, pad=3):
    """the rows in a buffer of vocab + pad columns (rows after the first are not 16-byte aligned); the padding holds 1e30: a kernel
    that read it would list it"""
    rows, vocab = host.shape
    buf = torch.full((rows, vocab + pad), 1e30, dtype=torch.float32, device=dev)
    buf[:, :vocab] = torch.from_numpy(host).to(dev)
    return buf


def launch(qp, buf, n, vocab, lse=True, active=None):
    rows, dev = buf.shape[0], buf.device
    ids = torch.full((rows, n), -7, dtype=torch.int32, device=dev)
    lp = torch.full((rows, n), 777.0, device=dev)
    ls = torch.full((rows,), 777.0, device=dev) if lse else None
    got = qp.top_logprobs(buf, n, ids=ids, logprob=lp, lse=ls, vocab=vocab, active=active)
    assert got[0] is ids and got[1] is lp
    return ids, lp, ls


def greedy(qp, buf, vocab):
    rows, dev = buf.shape[0], buf.device
    smp = qp.Sampler(rows, vocab, dev, temperature=0.0)
    return qp.sample(buf, smp, torch.zeros(rows, dtype=torch.int64, device=dev), vocab=vocab)


def yardstick_bitwise(qp, buf, vocab, ids, lp, lse, rows=None):
    """token_logprobs on the same buffer for every listed id: its logprob and lse equal the lists' bit for bit"""
    n, dev = ids.shape[1], buf.device
    for j in range(min(n, vocab)):
        t_lp = torch.full((buf.shape[0],), 555.0, device=dev)
        t_lse = torch.full((buf.shape[0],), 555.0, device=dev)
        qp.token_logprobs(buf, ids[:, j].long().contiguous(), out=t_lp, lse=t_lse, vocab=vocab)
        sel = slice(None) if rows is None else rows
        assert torch.equal(bits(t_lp[sel]), bits(lp[sel, j])), ("logprob", j)
        assert torch.equal(bits(t_lse[sel]), bits(lse[sel])), ("lse", j)


@pytest.mark.parametrize("rows,vocab,n", [(1, 128256, 20), (128, 32000, 5), (65, 1000, 64), (17, 33, 64), (3, 1, 4), (5, 4099, 20)])
def test_kernel_against_its_specification(qp, rows, vocab, n):
    """logits N(0, 3^2) in a padded buffer, the planted cases of KINDS on consecutive rows (launches with the cases shifted until every
    kind has been seen): ids exact, values within delta, bitwise token_logprobs' figures, two launches bitwise equal, a null lse
    changes nothing else, the first entry is the greedy draw"""
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(rows * 1000 + vocab)
    worst, seen = 0.0, set()
    for shift in range(0, len(KINDS), min(rows, len(KINDS))):
        kinds = [KINDS[(r + shift) % len(KINDS)] for r in range(rows)]
        seen.update(kinds)
        host = np.stack([ts.make_row(kind, vocab, n, rng) for kind in kinds])
        buf = padded(host, dev)
        ids, lp, lse = launch(qp, buf, n, vocab)
        ids2, lp2, lse2 = launch(qp, buf, n, vocab)
        ids3, lp3, _ = launch(qp, buf, n, vocab, lse=False)
        tok = greedy(qp, buf, vocab)
        yardstick_bitwise(qp, buf, vocab, ids, lp, lse)
        torch.cuda.synchronize()
        assert torch.equal(ids, ids2) and torch.equal(bits(lp), bits(lp2)) and torch.equal(bits(lse), bits(lse2))
        assert torch.equal(ids, ids3) and torch.equal(bits(lp), bits(lp3))
        assert torch.equal(ids[:, 0].long(), tok), "the first entry is the greedy token"
        assert bool((buf[:, vocab:] == 1e30).all())
        ids_h, lp_h, lse_h = ids.cpu().numpy(), lp.cpu().numpy(), lse.cpu().numpy()
        for r, kind in enumerate(kinds):
            worst = max(worst, check_lists(host[r], n, ids_h[r], lp_h[r], lse_h[r], (rows, vocab, n, r, kind)))
    assert seen == set(KINDS)
    print(f"rows {rows} vocab {vocab} n {n}: worst error {worst:.4f} of delta")


def test_threshold_ties_across_the_workgroup(qp):
    """the threshold value held by tokens of different lanes, waves and strides of 1024 groups: the lowest ids win"""
    dev = torch.device("cuda", 0)
    vocab, n = 128256, 8
    rng = np.random.default_rng(27)
    held = [3, 4 * 1024 + 1, 4 * 1024 * 5 + 2, 4 * 1024 * 5 + 3, 4 * 64 + 0, 4 * 64 * 7 + 1, 70000, 100001, vocab - 1]
    host = (rng.standard_normal((6, vocab)) * 3.0).astype(np.float32).clip(-20.0, 20.0)
    host[0, held] = 30.0                       # three above the ties: five slots for nine holders
    host[0, [9, 50000, 128000]] = [40.0, 41.0, 39.0]
    host[1, held] = 30.0                       # the ties are the maximum: every slot is theirs
    host[2, :] = -2.5                          # a constant row
    late = [120001, 120002, 124095, 124096, 126000, 127777, 128000, 128100, 128254, vocab - 1]
    host[3, late] = 30.0                       # holders in the last groups only: the compaction runs to the end of the row
    host[3, [0, 1, 2]] = 35.0
    host[4, :] = np.nan                        # NaN and -inf tie with each other
    host[4, 5::3] = -np.inf
    host[4, [77, 99999]] = [1.0, 2.0]
    host[5, held] = 30.0                       # exactly as many holders as slots: no compaction
    host[5, held[n:]] = 0.0
    buf = padded(host, dev)
    ids, lp, lse = launch(qp, buf, n, vocab)
    yardstick_bitwise(qp, buf, vocab, ids, lp, lse)
    ids64, lp64, lse64 = launch(qp, buf, 64, vocab)
    torch.cuda.synchronize()
    ids_h, lp_h, lse_h = ids.cpu().numpy(), lp.cpu().numpy(), lse.cpu().numpy()
    assert ids_h[0].tolist() == [50000, 9, 128000] + sorted(held)[:5]
    assert ids_h[1].tolist() == sorted(held)[:8]
    assert ids_h[2].tolist() == list(range(8)) and ids64[2].cpu().tolist() == list(range(64))
    assert ids_h[3].tolist() == [0, 1, 2] + late[:5]
    assert ids_h[4].tolist() == [99999, 77, 0, 1, 2, 3, 4, 5]
    assert ids_h[5].tolist() == sorted(held)[:8]
    for r in range(6):
        check_lists(host[r], n, ids_h[r], lp_h[r], lse_h[r], ("ties", r))
        check_lists(host[r], 64, ids64[r].cpu().numpy(), lp64[r].cpu().numpy(), float(lse64[r]), ("ties, n = 64", r))


def test_active_vector_and_row_independence(qp):
    """active[row] < 0 leaves the row's three outputs alone; row 77 of a 128-row launch equals the same row launched alone, bitwise;
    the first entries are the greedy draws of the planted batch"""
    dev = torch.device("cuda", 0)
    rows, vocab, n = 128, 128256, 20
    rng = np.random.default_rng(4)
    host = (rng.standard_normal((rows, vocab)) * 3.0).astype(np.float32)
    for r in range(rows):
        if KINDS[r % len(KINDS)] != "plain":
            host[r] = ts.make_row(KINDS[r % len(KINDS)], vocab, n, rng)
    buf = torch.from_numpy(host).to(dev)
    active = torch.arange(rows, dtype=torch.int64, device=dev) - 5  # rows 0 .. 4 inactive
    ids, lp, lse = launch(qp, buf, n, vocab, active=active)
    full_ids, _, _ = launch(qp, buf, n, vocab)
    one = launch(qp, buf[77:78].clone(), n, vocab)
    tok = greedy(qp, buf, vocab)
    torch.cuda.synchronize()
    assert bool((ids[:5] == -7).all()) and bool((lp[:5] == 777.0).all()) and bool((lse[:5] == 777.0).all())
    assert bool((ids[5:] >= 0).all()) and bool((lp[5:] <= 0).all()) and torch.equal(ids[5:], full_ids[5:])
    assert torch.equal(one[0], ids[77:78]) and torch.equal(bits(one[1]), bits(lp[77:78])) and torch.equal(bits(one[2]), bits(lse[77:78]))
    assert torch.equal(full_ids[:, 0].long(), tok)
    for r in (5, 6, 77, 127):
        check_lists(host[r], n, ids[r].cpu().numpy(), lp[r].cpu().numpy(), float(lse[r]), ("row", r))


def test_errors_before_any_launch(qp):
    dev, E = torch.device("cuda", 0), qp._native.QpalError
    buf = torch.zeros(4, 100, device=dev)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    for n in (0, 65, -1):
        with pytest.raises(E):
            qp.top_logprobs(buf, n)
    for kw in (dict(ids=f32(4, 5)), dict(ids=i32(4, 6)), dict(ids=i32(5, 5)), dict(ids=i32(4, 5).cpu()), dict(ids=i32(4, 10)[:, ::2]),
               dict(logprob=i32(4, 5)), dict(logprob=f32(4, 4)), dict(logprob=f32(20)), dict(logprob=f32(4, 5).cpu()),
               dict(lse=f32(5)), dict(lse=i32(4)), dict(active=i32(4)), dict(vocab=101), dict(vocab=0)):
        with pytest.raises(E):
            qp.top_logprobs(buf, 5, **kw)
    with pytest.raises(E):
        qp.top_logprobs(torch.zeros(129, 100, device=dev), 5)
    ids, lp = qp.top_logprobs(buf, 5)
    torch.cuda.synchronize()
    assert ids.shape == (4, 5) and ids.dtype == torch.int32 and lp.shape == (4, 5) and lp.dtype == torch.float32
    assert ids.cpu().tolist() == [list(range(5))] * 4


# ---------------------------------------------------------------------------------------------------------------- the steps

def _state(m, B, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    kc = [(torch.randn(B, 8, 512, 128, device=dev, generator=g) * 0.5).half() for _ in m.layers]
    vc = [(torch.randn(B, 8, 512, 128, device=dev, generator=g) * 0.5).half() for _ in m.layers]
    tok = torch.randint(0, 4096, (B,), device=dev, generator=g)
    pos = torch.tensor([10, 3, 100, 0, 250, 77, 31, 400][:B], dtype=torch.int64, device=dev)
    if B > 1:
        pos[5] = -1  # a free slot
    return kc, vc, tok, pos


TYPES = [(0.6, 5, 1.0), (1.0, 0, 1.0), (0.8, 0, 0.95), (0.7, 50, 0.9), (0.0, 0, 1.0), (1.0, 0, 1.0), (0.9, 5000, 1.0), (0.6, 5, 0.9)]


def _decode_step(qp, m, B, dev, top, **kw):
    t = TYPES[:B]
    smp = qp.Sampler(B, 4096, dev, temperature=[x[0] for x in t], top_k=[x[1] for x in t], top_p=[x[2] for x in t],
                     seed=[11 + b for b in range(B)], logprobs=True, top_logprobs=top)
    kc, vc, tok, pos = _state(m, B, dev, 5)
    out = torch.full((B,), -7, dtype=torch.int64, device=dev)
    step = qp.DecodeStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, tok, pos, out, sampler=smp, **kw)
    return step, smp, tok, pos, out


def _check_tail(qp, smp, pos, out, n, what):
    """the sampler's lists against the reference on a copy of smp.logits; the drawn token's entry is smp.logprob bitwise; a free
    slot keeps its sentinels; and the three outputs are bitwise the launches alone on these logits.  Returns the listed draws."""
    torch.cuda.synchronize()
    B, dev = smp.B, smp.logits.device
    logits = smp.logits.clone()
    host, toks, ps = logits.cpu().numpy(), out.cpu().tolist(), pos.cpu().tolist()
    ids_h, lp_h = smp.top_id.cpu().numpy(), smp.top_logprob.cpu().numpy()
    listed = 0
    for b in range(B):
        if ps[b] < 0:
            assert (ids_h[b] == -7).all() and (lp_h[b] == 555.0).all() and float(smp.logprob[b]) == 555.0, "a free slot keeps its lists"
            continue
        check_lists(host[b], n, ids_h[b], lp_h[b], None, (what, b))
        if toks[b] in ids_h[b].tolist():
            j = ids_h[b].tolist().index(toks[b])
            assert torch.equal(bits(smp.top_logprob[b, j:j + 1]), bits(smp.logprob[b:b + 1])), (what, b, j)
            listed += 1
    ids, lp, _ = launch(qp, logits, n, logits.shape[1], active=pos)
    alone = qp.token_logprobs(logits, out, out=torch.full((B,), 555.0, device=dev), active=pos)
    drawn = qp.sample(logits, smp, pos, out=torch.full((B,), -7, dtype=torch.int64, device=dev))
    torch.cuda.synchronize()
    act = pos >= 0
    assert torch.equal(ids[act], smp.top_id[act]) and torch.equal(bits(lp[act]), bits(smp.top_logprob[act]))
    assert torch.equal(bits(alone), bits(smp.logprob)) and torch.equal(drawn, out)
    return listed


@pytest.mark.parametrize("B", [1, 8])
def test_decode_step_with_top_logprobs(qp, model, B):
    """Sampler(logprobs=True, top_logprobs=5): the lists are those of smp.logits for the active slots, the free slot keeps its
    sentinels, the drawn token's entry is smp.logprob bitwise; tokens and logprob are those of the step without top_logprobs, which
    has one launch less; a captured step replayed three times agrees with three eager steps"""
    dev, m, n = torch.device("cuda", 0), model, 5
    plain, smp0, _, _, out0 = _decode_step(qp, m, B, dev, 0)
    step, smp, tok, pos, out = _decode_step(qp, m, B, dev, n)
    assert smp0.top_id is None and step.launches_per_token == plain.launches_per_token + 1 and step.batch1 == (B == 1)
    for s in (smp0, smp):
        s.logprob.fill_(555.0)
    smp.top_id.fill_(-7)
    smp.top_logprob.fill_(555.0)
    plain()
    step()
    listed = _check_tail(qp, smp, pos, out, n, ("step", B))
    assert listed >= 1, "no drawn token was listed: the bitwise check did not run"
    # against the step without top_logprobs: the same tokens; the same logprob bit for bit where the two runs of the layers left the
    # same logits, and otherwise within what their difference allows: |d logprob| <= |d l[t]| + |d lse| <= 2 max |d l| (log-sum-exp
    # is 1-Lipschitz in the sup norm), each kernel value within delta of the exact one
    assert torch.equal(out, out0), "top_logprobs must not disturb the draw"
    same = torch.equal(bits(smp.logits), bits(smp0.logits))
    print(f"B {B}: the two steps' logits are {'bitwise equal' if same else 'equal to rounding only'}")
    if same:
        assert torch.equal(bits(smp.logprob), bits(smp0.logprob))
    else:
        for b in range(B):
            dl = float((smp.logits[b] - smp0.logits[b]).abs().max())
            bound = 2.0 * delta_of(smp.logits[b].cpu().numpy()) + 2.0 * dl
            assert abs(float(smp.logprob[b]) - float(smp0.logprob[b])) <= bound, (b, dl, bound)
    # three eager steps, then the same three from a captured graph on the same state
    state = ([t.clone() for t in step.kcache + step.vcache], tok.clone(), pos.clone(), out.clone())

    def advance():
        tok.copy_(torch.where(pos >= 0, out, tok))
        pos.add_((pos >= 0).long())

    eager = []
    for _ in range(3):
        advance()
        step()
        _check_tail(qp, smp, pos, out, n, ("eager", B))
        eager.append((smp.logits.clone(), out.clone(), smp.top_id.clone(), smp.top_logprob.clone()))
    for t, t0 in zip(step.kcache + step.vcache, state[0]):
        t.copy_(t0)
    tok.copy_(state[1]), pos.copy_(state[2]), out.copy_(state[3])
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            step()
        for i in range(3):
            advance()
            g.replay()
            _check_tail(qp, smp, pos, out, n, ("replay", B, i))
            lg, o, ti, tl = eager[i]
            if not torch.equal(o, out):
                break  # (a near-tie drawn the other way on logits that differ in rounding: the streams have parted)
            act = pos >= 0
            if torch.equal(bits(lg), bits(smp.logits)):
                assert torch.equal(ti[act], smp.top_id[act]) and torch.equal(bits(tl[act]), bits(smp.top_logprob[act]))
        else:
            print(f"B {B}: three replays drew the eager steps' tokens")
        torch.cuda.synchronize()


def _model_table(G):
    """a synthetic vocabulary for the model's 4096 ids: the single characters of "ab0123456789.-x" first, then strings of 1 .. 4 of
    them; eos = 2 carries bytes no grammar takes"""
    rng = np.random.default_rng(4096)
    alpha = b"ab0123456789.-x"
    toks = [bytes([c]) for c in alpha]
    while len(toks) < 4096:
        toks.append(bytes(rng.choice(np.frombuffer(alpha, np.uint8), size=rng.integers(1, 5)).tolist()))
    toks[2], toks[-1] = b"</s>", b"0"
    return G.TokenTable(toks, eos=2)


def test_decode_step_with_a_processor_and_a_grammar(qp, model):
    """the lists are those of the processed and masked logits the draw saw"""
    dev, m, n, B = torch.device("cuda", 0), model, 5, 8
    proc = qp.LogitProcessor(B, 4096, dev)
    proc.set_mask(0, allowed=[7, 1000, 4095])               # three tokens allowed: two of the five entries are at -inf, by id
    proc.set_bias(1, {123: 50.0, 4000: 49.0})
    proc.set(2, repetition=1.3, presence=0.5)
    bank = qp.GrammarBank(B, _model_table(qp.grammar), dev, grammars=2, max_states=32)
    bank.load(0, r"-?(0|[1-9]\d*)(\.\d+)?")
    bank.set(3, 0)
    bank.set(1, 0)
    plain, _, _, _, _ = _decode_step(qp, m, B, dev, 0, processor=proc, grammar=bank)
    step, smp, tok, pos, out = _decode_step(qp, m, B, dev, n, processor=proc, grammar=bank)
    assert step.launches_per_token == plain.launches_per_token + 1
    smp.logprob.fill_(555.0)
    smp.top_id.fill_(-7)
    smp.top_logprob.fill_(555.0)
    step()
    _check_tail_masked(qp, smp, pos, out, n)
    ids = smp.top_id.cpu().tolist()
    lp = smp.top_logprob.cpu().numpy()
    assert sorted(ids[0][:3]) == [7, 1000, 4095] and ids[0][3:] == [0, 1] and np.all(lp[0][3:] == -np.inf) and np.all(np.isfinite(lp[0][:3]))
    assert bool(torch.isinf(smp.logits[3]).any()) and bool(torch.isinf(smp.logits[1]).any()), "the grammar has masked its slots"
    allowed = qp.grammar.reference_allow(qp.grammar.compile_regex(r"-?(0|[1-9]\d*)(\.\d+)?"), _model_table(qp.grammar))
    assert all(np.isinf(lp[3][j]) or ((allowed[0][ids[3][j] >> 5] >> (ids[3][j] & 31)) & 1) for j in range(n))


def _check_tail_masked(qp, smp, pos, out, n):
    """_check_tail without the stand-alone draw (with a grammar the step has advanced the automata behind it)"""
    torch.cuda.synchronize()
    host, toks, ps = smp.logits.cpu().numpy(), out.cpu().tolist(), pos.cpu().tolist()
    ids_h, lp_h = smp.top_id.cpu().numpy(), smp.top_logprob.cpu().numpy()
    for b in range(smp.B):
        if ps[b] < 0:
            assert (ids_h[b] == -7).all() and (lp_h[b] == 555.0).all()
            continue
        check_lists(host[b], n, ids_h[b], lp_h[b], None, ("processed", b))
        if toks[b] in ids_h[b].tolist():
            j = ids_h[b].tolist().index(toks[b])
            assert torch.equal(bits(smp.top_logprob[b, j:j + 1]), bits(smp.logprob[b:b + 1]))


def test_prefill_writes_the_slots_row(qp, model):
    dev, m, n = torch.device("cuda", 0), model, 5
    B, slot, N = 3, 1, 129
    kc = [torch.zeros(B, 8, 512, 128, dtype=torch.float16, device=dev) for _ in m.layers]
    vc = [torch.zeros(B, 8, 512, 128, dtype=torch.float16, device=dev) for _ in m.layers]
    smp = qp.Sampler(B, 4096, dev, temperature=[1.0, 0.8, 0.0], top_k=[0, 50, 0], top_p=[1.0, 0.9, 1.0], seed=[1, 2, 3], logprobs=True,
                     top_logprobs=n)
    smp.top_id.fill_(-7)
    smp.top_logprob.fill_(555.0)
    pf = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, sampler=smp)
    toks = torch.randint(0, 4096, (N,), device=dev, generator=torch.Generator(device=dev).manual_seed(N))
    pf(toks, slot=slot, pos0=0)
    torch.cuda.synchronize()
    assert bool((smp.top_id[[0, 2]] == -7).all()) and bool((smp.top_logprob[[0, 2]] == 555.0).all())
    check_lists(smp.logits[slot].cpu().numpy(), n, smp.top_id[slot].cpu().numpy(), smp.top_logprob[slot].cpu().numpy(), None, "prefill")


def test_ragged_step_writes_per_segment(qp, model):
    dev, m, n = torch.device("cuda", 0), model, 5
    B = 4
    kc = [torch.zeros(B, 8, 512, 128, dtype=torch.float16, device=dev) for _ in m.layers]
    vc = [torch.zeros(B, 8, 512, 128, dtype=torch.float16, device=dev) for _ in m.layers]
    smp = qp.Sampler(B, 4096, dev, temperature=[1.0, 0.8, 0.0, 0.6], top_k=[0, 50, 0, 5], seed=[1, 2, 3, 4], logprobs=True, top_logprobs=n)
    rs = qp.RaggedStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, rows=32, segments=4, sampler=smp)
    assert rs.draw.top_id.shape == (4, n) and rs.draw.top_logprob.shape == (4, n)
    rs.draw.top_id.fill_(-7)
    rs.draw.top_logprob.fill_(555.0)
    g = torch.Generator().manual_seed(18)
    items = [(2, torch.randint(0, 4096, (17,), generator=g), 0), (0, torch.randint(0, 4096, (5,), generator=g), 3)]
    out = rs(*rs.pack(items))
    torch.cuda.synchronize()
    for s in range(2):
        check_lists(rs.draw.logits[s].cpu().numpy(), n, rs.draw.top_id[s].cpu().numpy(), rs.draw.top_logprob[s].cpu().numpy(), None, ("segment", s))
        if int(out[s]) in rs.draw.top_id[s].cpu().tolist():
            j = rs.draw.top_id[s].cpu().tolist().index(int(out[s]))
            assert torch.equal(bits(rs.draw.top_logprob[s, j:j + 1]), bits(rs.draw.logprob[s:s + 1]))
    assert bool((rs.draw.top_id[2:] == -7).all()) and bool((rs.draw.top_logprob[2:] == 555.0).all()), "inactive segments keep theirs"


def test_speculative_step_gathers_the_rows_lists(qp, model):
    """out_top_id[b, j], j < n_out[b], is the list of the row that emitted out_tok[b, j]; the return tuple stays as it is"""
    dev, m, n = torch.device("cuda", 0), model, 5
    B, draft = 4, 4
    kc = [torch.zeros(B, 8, 512, 128, dtype=torch.float16, device=dev) for _ in m.layers]
    vc = [torch.zeros(B, 8, 512, 128, dtype=torch.float16, device=dev) for _ in m.layers]
    g = torch.Generator().manual_seed(31)
    prompts = [torch.randint(0, 4096, (k,), generator=g).to(dev) for k in (5, 17, 40)]
    prompts[2][-6:] = prompts[2][10:16]   # a repeated run: prompt lookup has something to draft
    pf = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq)
    smp = qp.Sampler(B, 4096, dev, temperature=[0.7, 1.0, 0.0, 1.3], top_k=[40, 0, 5, 3], seed=[11, 12, 13, 14], top_logprobs=n)
    ss = qp.SpeculativeStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, draft=draft, sampler=smp)
    assert ss.out_top_id.shape == (B, draft + 1, n) and ss.out_top_id.dtype == torch.int32 and ss.out_logprob is None
    assert ss.out_top_logprob.shape == (B, draft + 1, n) and ss.out_top_logprob.dtype == torch.float32
    for b, p in enumerate(prompts):
        pf(p[:-1], slot=b, pos0=0)
        ss.begin(b, p.tolist(), limit=p.shape[0] + 24)
    res = ss()
    assert len(res) == 2
    out_tok, n_out = res
    ids, lp, _ = launch(qp, ss.draw.logits, n, 4096, lse=False, active=ss.row_ctr)
    torch.cuda.synchronize()
    assert int(n_out[3]) == 0
    for b in range(3):
        r, k = int(ss.row0[b]), int(n_out[b])
        assert k >= 1 and torch.equal(out_tok[b, :k], ss.drawn[r:r + k])
        assert torch.equal(ss.out_top_id[b, :k], ids[r:r + k]) and torch.equal(bits(ss.out_top_logprob[b, :k]), bits(lp[r:r + k]))
        for j in range(k):
            check_lists(ss.draw.logits[r + j].cpu().numpy(), n, ss.out_top_id[b, j].cpu().numpy(), ss.out_top_logprob[b, j].cpu().numpy(),
                        None, ("speculative", b, j))


@pytest.mark.parametrize("N", [2, 129, 300])
def test_score_with_top_logprobs(qp, model, N, monkeypatch):
    """sc.top_id / sc.top_logprob [N - 1, 4]: every position's list is the launch on its row of the chunk's logits alone, bitwise,
    and the reference's; lp and rank are what they are without top_logprobs"""
    dev, m, n = torch.device("cuda", 0), model, 4
    g = torch.Generator(device=dev).manual_seed(3)
    kc = [(torch.randn(3, 8, 512, 128, device=dev, generator=g) * 0.5).half() for _ in m.layers]
    vc = [(torch.randn(3, 8, 512, 128, device=dev, generator=g) * 0.5).half() for _ in m.layers]
    sc = qp.Score(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, chunk=128, top_logprobs=n)
    assert qp.Score(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq).top_id is None
    chunks, real = [], sampling.top_logprobs

    def spy(logits, *a, **kw):   # the logits of every chunk, as the launch saw them
        chunks.append(logits.clone())
        return real(logits, *a, **kw)

    monkeypatch.setattr(sampling, "top_logprobs", spy)
    tokens = torch.randint(0, 4096, (N,), device=dev, generator=torch.Generator(device=dev).manual_seed(N))
    lp = sc(tokens, slot=1, pos0=0)
    monkeypatch.setattr(sampling, "top_logprobs", real)
    torch.cuda.synchronize()
    assert sc.top_id.shape == (N - 1, n) and sc.top_id.dtype == torch.int32 and sc.top_logprob.shape == (N - 1, n)
    assert sc.top_logprob.dtype == torch.float32 and lp.shape == (N - 1,) and sc.rank.shape == (N - 1,)
    assert [c.shape[0] for c in chunks] == [min(128, N - c) for c in range(0, N, 128)]
    all_logits = torch.cat(chunks)
    rank = torch.zeros(N - 1, dtype=torch.int32, device=dev)
    for c in range(0, N - 1, 128):
        k = min(128, N - 1 - c)
        alone = qp.token_logprobs(all_logits[c:c + k], tokens[c + 1:c + 1 + k].contiguous(), rank=rank[c:c + k])
        assert torch.equal(bits(alone), bits(lp[c:c + k])), "lp is what it is without top_logprobs"
    assert torch.equal(rank, sc.rank)
    for t in range(N - 1):
        ids, lps, _ = launch(qp, all_logits[t:t + 1], n, 4096, lse=False)
        assert torch.equal(ids[0], sc.top_id[t]) and torch.equal(bits(lps[0]), bits(sc.top_logprob[t])), t
    host = all_logits.cpu().numpy()
    for t in sorted({0, (N - 1) // 2, N - 2}):
        check_lists(host[t], n, sc.top_id[t].cpu().numpy(), sc.top_logprob[t].cpu().numpy(), None, ("score", N, t))
