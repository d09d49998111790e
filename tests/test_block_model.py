"""The five step classes on Qwen- and Gemma-shaped blocks against the float64 forward of block_model_reference.py:
model_reference.build's small model, 3 layers, context 64, as "qwen" (qkv_bias + qk_norm) and as "gemma" (qk_norm, GeGLU, post-norms,
logit cap, per-layer inv_freq, pre-scaled embed, and in one layer a score cap and a window under attn_scale).  Tolerance: §28's,
model_reference.tolerance — 4 x the emulation's own distance from the float64 forward, measured on the reference pair.

CPU: the reference with nothing in it is model_reference's forward; every seeded defect leaves the tolerance (factors printed); the
share of undecidable rows of every token set stays under the cap.  GPU: DecodeStep at B = 4 (one inactive slot) and at B = 1,
Prefill, Score, RaggedStep, SpeculativeStep; a paged e4m3 decode case; a decode case with adapters; a captured step that follows
rows rewritten in place; launches_per_token; every new argument at its default is the step without them, bit for bit."""
import functools
import types

import pytest
import torch

import block_model_reference as bm
import model_reference as mr
from attn_reference import F8
from test_model_exact import LORA_SCALE, UNDECIDABLE_CAP, _bank, _raw_adapters
from test_window_model import _caches, _Decode, _forced, _judge, _reproducible_projections

gpu = pytest.mark.gpu
NL, CHUNK = 3, 16
KINDS = ("qwen", "gemma")
DECODE_LENS = (24, 30, 0, 33)            # B = 4, slot 2 inactive
PREFILL_LENS = (1, 17, 40)
SEEDS = {"decode": 41, "prefill": 42}    # the first seeds, counted up from 41, whose sets meet the cap on undecidable rows (CPU test)
SLOT_ADAPTER = [0, 1, -1, 0]


def _tokens(name):
    g = torch.Generator().manual_seed(SEEDS[name])
    lens = DECODE_LENS if name == "decode" else PREFILL_LENS
    return [torch.randint(0, mr.VOCAB, (n,), generator=g) for n in lens]


@functools.lru_cache(maxsize=None)
def _spec(geometry="S"):
    return mr.build_spec(geometry, "mixed", NL)


@functools.lru_cache(maxsize=None)
def _cpu_pair(kind, name, lora=False):
    spec = _spec()
    var, toks = bm.variant(kind, spec.ref), _tokens(name)
    lo = {"adapters": _raw_adapters(spec, LORA_SCALE, NL), "slot_adapter": SLOT_ADAPTER} if lora else None
    ref = bm.forward(spec.ref, var, toks, chunk=CHUNK, lora=lo)
    emu = bm.forward(spec.ref, var, toks, emu=True, chunk=CHUNK, prefill=name == "prefill", lora=lo)
    return var, toks, lo, ref, emu


def _rows(toks):
    return [(b, p) for b, t in enumerate(toks) for p in range(len(t))]


# ============================================================================================================================= CPU
def test_the_reference_with_nothing_in_it_is_model_reference():
    spec, toks = _spec(), _tokens("decode")
    for emu in (False, True):
        a = bm.forward(spec.ref, bm.plain(spec.ref), toks, emu=emu, chunk=CHUNK)
        b = (mr.forward_emulated if emu else mr.forward_fp64)(spec.ref, toks, chunk=CHUNK)
        for s in (0, 1, 3):
            assert torch.allclose(a.stream[s], b.stream[s], rtol=1e-9, atol=1e-12) and torch.allclose(a.logits[s], b.logits[s], rtol=1e-9, atol=1e-12)


def _factor(ref, emu, bad, rows):
    """how far `bad` lies from ref in units of the tolerance: max over rows of stream and logits"""
    st = lambda o: torch.stack([o.stream[b][-1][p] for b, p in rows])   # noqa: E731
    lg = lambda o: torch.stack([o.logits[b][p] for b, p in rows])        # noqa: E731
    xh = mr.e_h(st(bad), st(ref)) / mr.tolerance(mr.e_h(st(emu), st(ref)))
    xl = mr.e_l(lg(bad), lg(ref)) / mr.tolerance(mr.e_l(lg(emu), lg(ref)))
    return float(torch.maximum(xh, xl).max())


@pytest.mark.parametrize("kind", KINDS)
def test_the_seeded_defects_leave_the_tolerance(kind, capsys):
    spec = _spec()
    var, toks, _, ref, emu = _cpu_pair(kind, "decode")
    rows = _rows(toks)
    assert _factor(ref, emu, emu, rows) <= 0.25 + 1e-9       # the tolerance is 4 x the emulation's distance
    for name in bm.DEFECTS[kind]:
        f = _factor(ref, emu, bm.forward(spec.ref, var, toks, chunk=CHUNK, mutate=(name, 1)), rows)
        with capsys.disabled():
            print(f"\n  {kind} {name}: {f:.1f} x the tolerance")
        assert f > mr.TEETH, (name, f)
    if kind == "gemma":
        var, toks, lo, ref, emu = _cpu_pair(kind, "decode", True)
        f = _factor(ref, emu, bm.forward(spec.ref, var, toks, chunk=CHUNK, lora=lo, mutate=("post_norm_before_lora", 1)), rows)
        with capsys.disabled():
            print(f"\n  {kind} post_norm_before_lora: {f:.1f} x the tolerance")
        assert f > mr.TEETH, f


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(SEEDS))
def test_undecidable_rows_stay_under_the_cap(kind, name):
    var, toks, _, ref, emu = _cpu_pair(kind, name)
    rows = _rows(toks)
    rl, el = torch.stack([ref.logits[b][p] for b, p in rows]), torch.stack([emu.logits[b][p] for b, p in rows])
    dec = mr.decidable(rl, mr.tolerance(mr.e_l(el, rl)))
    assert float((~dec).float().mean()) <= UNDECIDABLE_CAP, (kind, name, int((~dec).sum()), len(rows))


# ============================================================================================================================= GPU
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _world.cache_clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _world(kind, geometry="S"):
    """(modules with the variant's embed / inv_freq in place, variant on the device, step keyword arguments)"""
    d = torch.device("cuda", 0)
    m = mr.build(geometry, "mixed", (), NL, mr.VOCAB, 0, d)
    var = bm.variant(kind, m.ref)
    kw, embed, inv_freq = bm.step_arguments(var, d)
    mm = types.SimpleNamespace(**vars(m))
    mm.embed, mm.inv_freq = embed, inv_freq
    return mm, var, kw


def _refs(mm, var, toks, dev, prefill=False, kv=None, lora=None):
    t = [x.to(dev) for x in toks]
    return (bm.forward(mm.ref, var, t, chunk=CHUNK, kv_dtype=kv, lora=lora),
            bm.forward(mm.ref, var, t, emu=True, chunk=CHUNK, prefill=prefill, kv_dtype=kv, lora=lora))


def _tokens_agree(case, rows, ref, emu, got_tok):
    """greedy tokens on the rows whose top-two gap the tolerance cannot close"""
    rl, el = torch.stack([ref.logits[b][p] for b, p in rows]), torch.stack([emu.logits[b][p] for b, p in rows])
    dec = mr.decidable(rl, mr.tolerance(mr.e_l(el, rl)))   # (the CPU test holds the share of undecidable rows of the whole sets)
    assert torch.equal(got_tok[dec].cpu(), rl.argmax(-1)[dec].cpu()), case


def _decode_case(mm, var, kw, dev, B, toks, kind="fp16", lora=None, bank=None, slots=None):
    ref, emu = _refs(mm, var, toks, dev, kv=F8 if "e4m3" in kind else None, lora=lora)
    sel = toks if slots is None else [toks[b] for b in slots]
    cache, kc, vc, ckw = _caches(mm, kind, dev, B)
    if cache is not None:
        for b, t in enumerate(sel):
            if len(t):
                cache.reserve(b, len(t))
    extra = {} if bank is None else {"adapters": bank}
    run = _Decode(mm, dev, B, kc, vc, **kw, **ckw, **extra)
    plan = _forced(sel)
    run.run(plan)
    picks = [(s, b) for s, row in enumerate(plan) for b, r in enumerate(row) if r is not None]
    rows = [(b if slots is None else slots[b], s) for s, b in picks]
    _judge(f"DecodeStep B={B} {var.kind} {kind}", rows, ref, emu, torch.stack([run.h[s][b] for s, b in picks]),
           torch.stack([run.l[s][b] for s, b in picks]))
    _tokens_agree(f"DecodeStep B={B} {var.kind} {kind}: tokens", rows, ref, emu, torch.stack([run.t[s][b] for s, b in picks]))
    return run


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_decode_steps_agree_with_the_reference(dev, kind):
    """B = 4 with an inactive slot, and the batch-1 step: the fused single-sequence attention kernel behind qkv_prep for "qwen", the
    batched launch at B = 1 for "gemma" (a window and a score cap)"""
    mm, var, kw = _world(kind)
    toks = _tokens("decode")
    run = _decode_case(mm, var, kw, dev, 4, toks)
    block = 1 + (3 if kind == "gemma" else 0)
    assert run.step.launches_per_token == (9 + block) * NL + 2 + (1 if kind == "gemma" else 0)
    b1 = _decode_case(mm, var, kw, dev, 1, toks, slots=[1])
    assert b1.step.batch1 and b1.step.attn_batch == (kind == "gemma") and b1.step.ug_il is None
    assert b1.step.launches_per_token == run.step.launches_per_token


@gpu
def test_decode_step_on_head_dim_128_and_on_a_paged_e4m3_cache(dev):
    mm, var, kw = _world("qwen", "S1")
    _decode_case(mm, var, kw, dev, 4, _tokens("decode"))
    mm, var, kw = _world("gemma")
    _decode_case(mm, var, kw, dev, 4, _tokens("decode"), kind="paged-e4m3")


@gpu
def test_decode_step_with_adapters_keeps_the_order_of_update_prep_and_post_norm(dev):
    mm, var, kw = _world("gemma")
    lo = {"adapters": _raw_adapters(mm.spec, LORA_SCALE, NL), "slot_adapter": SLOT_ADAPTER}
    run = _decode_case(mm, var, kw, dev, 4, _tokens("decode"), lora=lo, bank=_bank(mm, dev, LORA_SCALE, SLOT_ADAPTER))
    assert run.step.launches_per_token == (9 + 4 + 4) * NL + 3


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_prefill_score_and_ragged_agree_with_the_reference(dev, kind):
    import qpalette_amd as qp
    mm, var, kw = _world(kind)
    toks = _tokens("prefill")
    ref, emu = _refs(mm, var, toks, dev, prefill=True)
    _, kc, vc, _ = _caches(mm, "fp16", dev, 3)
    args = (mm.layers, mm.embed, mm.norm, mm.lm_head, kc, vc, mm.inv_freq)
    pf = qp.Prefill(*args, chunk=CHUNK, sampler=qp.Sampler(3, mr.VOCAB, dev, temperature=0.0), **kw)
    hs, ls, ts = [], [], []
    for b, t in enumerate(toks):
        ts.append(pf(t.to(dev), slot=b, pos0=0).clone()[0])
        hs.append(pf.last32[0].clone())
        ls.append(pf.sampler.logits[b].clone())
    torch.cuda.synchronize()
    last = [(b, len(t) - 1) for b, t in enumerate(toks)]
    _judge(f"Prefill {kind}", last, ref, emu, torch.stack(hs), torch.stack(ls))
    _tokens_agree(f"Prefill {kind}: tokens", last, ref, emu, torch.stack(ts))
    # RaggedStep: each slot's last 1 / 5 / 12 tokens onto the prefill of the rest (the caches hold every row already)
    tails = (1, 5, 12)
    rs = qp.RaggedStep(*args, rows=32, segments=3, **kw)
    items = [(b, t[len(t) - n:], len(t) - n) for b, (t, n) in enumerate(zip(toks, tails))]
    out = rs(*rs.pack(items))
    torch.cuda.synchronize()
    rows = [(b, p0 + r) for b, t, p0 in items for r in range(len(t))]
    _judge(f"RaggedStep {kind}: rows", rows, ref, emu, rs.h32[:len(rows)])
    _judge(f"RaggedStep {kind}: segments", last, ref, emu, rs.last32[:3], rs.draw.logits[:3])
    _tokens_agree(f"RaggedStep {kind}: tokens", last, ref, emu, out[:3])
    # Score: log-probabilities under the cap; log_softmax moves by at most twice the largest logit error
    sc = qp.Score(*args, chunk=CHUNK, **kw)
    worst = 0.0
    for b, t in enumerate(toks):
        if len(t) < 2:
            continue
        lp = sc(t.to(dev), slot=b, pos0=0).double()
        want = ref.logprob[b][:-1].gather(1, t[1:].to(dev)[:, None])[:, 0]
        tol_l = mr.tolerance(mr.e_l(emu.logits[b][:-1], ref.logits[b][:-1])) * ref.logits[b][:-1].pow(2).mean(-1).sqrt()
        worst = max(worst, float(((lp - want).abs() / (2.0 * tol_l)).max()))
        if var.cap is not None:
            assert float(sc.logits.abs().max()) <= var.cap
    print(f"Score {kind}: worst err / tol {worst:.3f}")
    assert worst <= 1.0


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_speculative_step_agrees_with_the_reference(dev, kind):
    """draft = 3 with the caller's drafts, which are the sequences' own next tokens: row j of slot b's segment stands at position
    P - 1 + j and is fed the sequence's token there, so every row of the step — stream, logits, and the draw on decidable rows — is
    the float64 forward's row of the teacher-forced sequence, whatever the accept keeps; the first emitted token is row 0's draw.
    Slot 2 is never begun and has no rows."""
    import qpalette_amd as qp
    mm, var, kw = _world(kind)
    P, K = 12, 3
    toks = _tokens("decode")
    ref, emu = _refs(mm, var, toks, dev, prefill=True)
    _, kc, vc, _ = _caches(mm, "fp16", dev, 4)
    args = (mm.layers, mm.embed, mm.norm, mm.lm_head, kc, vc, mm.inv_freq)
    pf = qp.Prefill(*args, chunk=CHUNK, **kw)
    ss = qp.SpeculativeStep(*args, draft=K, sampler=qp.Sampler(4, mr.VOCAB, dev, temperature=0.0), **kw)
    drafts = torch.zeros(4, K, dtype=torch.long)
    for b, t in enumerate(toks):
        if len(t):
            pf(t[:P - 1].to(dev), slot=b, pos0=0)
            ss.begin(b, t[:P].tolist())
            drafts[b] = t[P:P + K]
    out_tok, n_out = ss(drafts.to(dev), torch.full((4,), K, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    row0 = ss.row0.tolist()
    assert row0[3] - row0[2] == 0 and int(n_out[2]) == 0
    live = [b for b, t in enumerate(toks) if len(t)]
    rows = [(b, P - 1 + j) for b in live for j in range(K + 1)]
    at = torch.tensor([row0[b] + j for b in live for j in range(K + 1)], device=dev)
    _judge(f"SpeculativeStep {kind}", rows, ref, emu, ss.h32[at], ss.draw.logits[at])
    _tokens_agree(f"SpeculativeStep {kind}: draws", rows, ref, emu, ss.drawn[at])
    for b in live:
        assert int(n_out[b]) >= 1 and int(out_tok[b, 0]) == int(ss.drawn[row0[b]])
    if var.cap is not None:
        assert float(ss.draw.logits[at].abs().max()) <= var.cap


@gpu
def test_a_captured_decode_step_follows_rows_rewritten_in_place(dev):
    """ONE captured graph of a DecodeStep replayed over a slot's tokens twice: between the passes layer 1's qkv_bias row (qwen) or its
    post_norms rows (gemma) are overwritten in place; each pass agrees with the float64 model that has ITS rows"""
    for kind, field in (("qwen", "bias"), ("gemma", "post")):
        mm, var, kw = _world(kind)
        kw = dict(kw)
        toks = [_tokens("decode")[1]]
        if field == "bias":
            live = kw["qkv_bias"] = kw["qkv_bias"].clone()
        else:
            live = kw["post_norms"][1].clone()
            kw["post_norms"] = (kw["post_norms"][0], live)
        first = live.clone()
        second = first.clone()
        second[1] = first[1].flip(-1) * 1.5
        _, kc, vc, _ = _caches(mm, "fp16", dev, 1)
        run = _Decode(mm, dev, 1, kc, vc, generic=True, **kw)
        run.tok.fill_(int(toks[0][0]))
        run.pos.fill_(0)
        run.step()  # (warm-up outside the capture: position 0 is written again by the first replay)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            run.step()
        passes = []
        for values in (first, second):
            live.copy_(values)
            hs, ls = [], []
            for s, t in enumerate(toks[0].tolist()):
                run.tok.fill_(t)
                run.pos.fill_(s)
                graph.replay()
                torch.cuda.synchronize()
                hs.append(run.step.h32[0].clone())
                ls.append(run.smp.logits[0].clone())
            passes.append((torch.stack(hs), torch.stack(ls)))
            v2 = types.SimpleNamespace(**vars(var))
            if field == "bias":
                v2.bias = values.double()
            else:
                v2.post = (var.post[0], values.double())
            ref, emu = _refs(mm, v2, toks, dev)
            _judge(f"captured DecodeStep {kind}, pass {len(passes)}", [(0, s) for s in range(len(toks[0]))], ref, emu, *passes[-1])
        assert float((passes[0][0].double() - passes[1][0].double()).abs().max()) > 1e-3


@gpu
def test_every_new_argument_at_its_default_is_the_step_without_them(dev, monkeypatch):
    """bit for bit, on projections without float atomics (test_window_model._reproducible_projections), and the same launch count"""
    import qpalette_amd as qp
    mm, _, _ = _world("qwen")
    m = mr.build("S", "mixed", (), NL, mr.VOCAB, 0, dev, spec=mm.spec)
    _reproducible_projections(monkeypatch)
    toks = _tokens("decode")
    defaults = dict(qkv_bias=None, qk_norm=None, mlp_act="silu", post_norms=None, logit_cap=None)
    got = []
    for kw in ({}, defaults):
        _, kc, vc, _ = _caches(m, "fp16", dev, 4)
        run = _Decode(m, dev, 4, kc, vc, **kw)
        run.run(_forced(toks)[:6])
        pf = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, chunk=CHUNK, **kw)
        pf(toks[1].to(dev), slot=2, pos0=0)
        torch.cuda.synchronize()
        got.append((run.step.launches_per_token, torch.stack(run.h), torch.stack(run.l), torch.stack(run.t), pf.last32.clone(), pf.out_tok.clone()))
        assert run.step.y32 is None and run.step.act32 is None and not run.step.rope_per_layer
    assert got[0][0] == got[1][0] == 9 * NL + 2
    for a, b in zip(got[0][1:], got[1][1:]):
        assert torch.equal(a, b)


@gpu
def test_launches_per_token_is_the_configuration_arithmetic_and_bad_arguments_raise(dev):
    import qpalette_amd as qp
    mm, var, kw = _world("gemma")
    E = qp._native.QpalError
    _, kc, vc, _ = _caches(mm, "fp16", dev, 4)
    tok, pos, out = (torch.zeros(4, dtype=torch.long, device=dev) for _ in range(3))
    mk = lambda **k: qp.DecodeStep(mm.layers, mm.embed, mm.norm, mm.lm_head, kc, vc, mm.inv_freq, tok, pos, out, **k)   # noqa: E731
    smp = qp.Sampler(4, mr.VOCAB, dev, temperature=0.0)
    base, L, H, hd = mk().launches_per_token, NL, 512, 64
    bias = torch.zeros(L, 768, device=dev)
    qk, post = (1e-6, torch.ones(L, 2, hd, device=dev)), (1e-6, torch.ones(L, 2, H, device=dev))
    assert base == 9 * L + 1
    assert mk(qkv_bias=bias).launches_per_token == base + L and mk(qk_norm=qk).launches_per_token == base + L
    assert mk(qkv_bias=bias, qk_norm=qk).launches_per_token == base + L            # one launch serves both
    assert mk(post_norms=post).launches_per_token == base + 2 * L and mk(mlp_act="gelu_tanh").launches_per_token == base + L
    assert mk(logit_cap=30.0).launches_per_token == base                           # an argmax tail needs no cap launch
    assert mk(logit_cap=30.0, sampler=smp).launches_per_token == mk(sampler=smp).launches_per_token + 1
    assert mk(qkv_bias=bias, qk_norm=qk, post_norms=post, mlp_act="gelu_tanh", logit_cap=30.0, sampler=smp).launches_per_token == (9 + 4) * L + 3
    for bad in (dict(qkv_bias=bias.half()), dict(qkv_bias=bias[:2]), dict(qkv_bias=bias.cpu()), dict(qkv_bias=bias.t().contiguous().t()),
                dict(qk_norm=qk[1]), dict(qk_norm=(0.0, qk[1])), dict(qk_norm=(1e-6, qk[1][:, :1])), dict(post_norms=(float("nan"), post[1])),
                dict(post_norms=(1e-6, post[1][:, :, :256])), dict(mlp_act="gelu"), dict(logit_cap=0.0), dict(logit_cap=float("inf")),
                dict(logit_cap=True)):
        with pytest.raises(E):
            mk(**bad)
    with pytest.raises(E):   # a per-layer table of the wrong height
        qp.DecodeStep(mm.layers, mm.embed, mm.norm, mm.lm_head, kc, vc, mm.inv_freq[:2], tok, pos, out)
    for cls, extra in ((qp.Prefill, {}), (qp.Score, {}), (qp.RaggedStep, {}), (qp.SpeculativeStep, {})):
        with pytest.raises(E):
            cls(mm.layers, mm.embed, mm.norm, mm.lm_head, kc, vc, mm.inv_freq, mlp_act="relu", **extra)
