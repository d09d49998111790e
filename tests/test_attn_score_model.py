"""Whole-model steps with attention score modifiers against the float64 model of tests/model_reference.py with the
modified attention patched in, the way tests/test_window_model.py patches a window: model_reference._attend and attn_reference.emulate
are replaced by wrappers that apply the soft cap, the sinks, the window and the attention scale of the layer under way (_forward visits
layers, slots and chunks in a fixed order: the index of the call gives the layer).

The model: model_reference.build's small one, 2 layers, with softcap = CAPS per layer, random sinks per layer and head, attn_scale =
ATTN_SCALE (not 1 / sqrt(head_dim) = 0.125) and a window in the first layer only.  CAPS was chosen on the CPU
(test_attn_score_contract.py::test_the_models_modifiers_bite): under ATTN_SCALE the model's scores have a standard deviation of about
2.5 and reach 10 .. 13, so caps of 4 and 6 squash the top of every row; dropping them moves the last layer's stream 112 times the
tolerance and more (measured there: the caps 112 .. 147, the sinks 195 .. 243, the default scale 60 .. 67)."""
import pytest
import torch

import attn_reference as ar
import model_reference as mr
import score_reference as sr
from attn_reference import F8
from test_window_model import CHUNK, NL, _bits, _caches, _Decode, _forced, _judge, _model, _tokens

gpu = pytest.mark.gpu
CAPS = (4.0, 6.0)
ATTN_SCALE = 0.2
WINDOWS = (8, None)
NQ = mr.GEOMETRY["S"]["nq"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def model_sinks(dev, seed=5, shift=0.0):
    """fp32 [NL, nq]: N(0, 2) per layer and head (+ shift)"""
    return (2.0 * torch.randn(NL, NQ, generator=torch.Generator().manual_seed(seed)) + shift).to(dev)


class Modified:
    """the two patches: one window, cap and sinks row per layer, one scale; calls_per_layer = the attention calls _forward makes per
    layer (one per slot with tokens and chunk)"""

    def __init__(self, monkeypatch, toks, windows=WINDOWS, caps=CAPS, sinks=None, scale=ATTN_SCALE, chunk=CHUNK):
        self.windows, self.caps, self.sinks, self.scale = list(windows), list(caps), sinks, scale
        self.per_layer = sum(-(-len(t) // chunk) for t in toks if len(t))
        self.calls = {"attend": 0, "emulate": 0}
        monkeypatch.setattr(mr, "_attend", self.attend)
        monkeypatch.setattr(ar, "emulate", self.emulate)

    def _layer(self, which):
        i = (self.calls[which] // self.per_layer) % len(self.windows)
        self.calls[which] += 1
        return self.windows[i], self.caps[i], None if self.sinks is None else self.sinks[i]

    def attend(self, q, Kc, Vc, pos, scale, see_next=False, lose_prev=False):
        """model_reference._attend with the layer's modifiers, in Hugging Face's form: cap the scores, mask, concatenate the sink
        as a column, softmax, drop the column"""
        w, cap, sk = self._layer("attend")
        n, nq, hd = q.shape
        nkv = Kc.shape[0]
        top = int(pos.max()) + 1
        j = torch.arange(top, device=q.device)
        valid = j[None, :] <= pos[:, None]
        if w is not None:
            valid = valid & (j[None, :] >= (pos - (w - 1))[:, None])
        s = torch.einsum("rgpd,gjd->rgpj", q.reshape(n, nkv, nq // nkv, hd), Kc[:, :top]) * self.scale
        if cap is not None:
            s = cap * torch.tanh(s / cap)
        s = s.masked_fill(~valid[:, None, None, :], float("-inf"))
        if sk is not None:
            s = torch.cat((s, sk.double().to(q.device).view(1, nkv, nq // nkv, 1).expand(n, nkv, nq // nkv, 1)), dim=-1)
        p = torch.softmax(s, dim=-1)[..., :top]
        return torch.einsum("rgpj,gjd->rgpd", p, Vc[:, :top]).reshape(n, nq * hd)

    def emulate(self, q16, K, V, n_keys_per_row, nq, nkv, hd, scale, u_p, rounded=True):
        w, cap, sk = self._layer("emulate")
        pos = [int(n) - 1 for n in n_keys_per_row]
        return sr.emulate(q16, K, V, pos, w, nq, nkv, hd, self.scale, u_p, cap, None if sk is None else sk.to(q16.device), rounded=rounded)


def refs(monkeypatch, model64, toks, dev, prefill, kv=None, **mods):
    """(float64 forward, emulated forward) of the modified model; mods: Modified's keywords"""
    Modified(monkeypatch, toks, **mods)
    t = [x.to(dev) for x in toks]
    ref = mr.forward_fp64(model64, t, chunk=CHUNK, kv_dtype=kv)
    emu = mr.forward_emulated(model64, t, chunk=CHUNK, prefill=prefill, kv_dtype=kv)
    monkeypatch.undo()
    return ref, emu


def _kw(sinks, **over):
    kw = dict(window=WINDOWS, softcap=CAPS, sinks=sinks, attn_scale=ATTN_SCALE)
    kw.update(over)
    return kw


KINDS = ["fp16", "paged-e4m3"]


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_decode_steps_agree_with_the_modified_reference(dev, kind, monkeypatch):
    """DecodeStep at B = 3 and at B = 1 (the batch-1 step: the batched attention at B = 1), every step of every slot"""
    m, toks = _model(), _tokens()[:3]
    sinks = model_sinks(dev)
    ref, emu = refs(monkeypatch, m.ref, toks, dev, False, kv=F8 if "e4m3" in kind else None, sinks=sinks)
    for B, sel in ((3, toks), (1, toks[2:3])):
        cache, kc, vc, kw = _caches(m, kind, dev, B)
        if cache is not None:
            for b, t in enumerate(sel):
                cache.reserve(b, len(t))
        run = _Decode(m, dev, B, kc, vc, **_kw(sinks), **kw)
        assert run.step.attn_batch and run.step.batch1 == (B == 1) and run.step.attn_scale == ATTN_SCALE
        before = run.step.launches_per_token
        plan = _forced(sel)
        run.run(plan)
        picks = [(s, b) for s, row in enumerate(plan) for b, r in enumerate(row) if r is not None]
        rows = [(b if B == 3 else 2, s) for s, b in picks]
        _judge(f"DecodeStep B={B} {kind} score modifiers", rows, ref, emu, torch.stack([run.h[s][b] for s, b in picks]),
               torch.stack([run.l[s][b] for s, b in picks]))
        plain = _Decode(m, dev, B, *_caches(m, kind, dev, B)[1:3], **kw)
        assert plain.step.launches_per_token == before  # the launch count does not change


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_prefill_ragged_and_score_agree_with_the_modified_reference(dev, kind, monkeypatch):
    """Prefill (chunk 16) of every slot, one RaggedStep that takes each slot's last 1 .. 12 tokens onto a Prefill of the rest, and
    Score's log-probabilities of every slot's tokens"""
    import qpalette_amd as qp
    m, toks = _model(), _tokens()
    sinks = model_sinks(dev)
    ref, emu = refs(monkeypatch, m.ref, toks, dev, True, kv=F8 if "e4m3" in kind else None, sinks=sinks)
    cache, kc, vc, kw = _caches(m, kind, dev, 4)
    if cache is not None:
        for b, t in enumerate(toks):
            cache.reserve(b, len(t))
    pf = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, chunk=CHUNK, sampler=qp.Sampler(4, mr.VOCAB, dev, temperature=0.0),
                    **_kw(sinks), **kw)
    hs, ls = [], []
    for b, t in enumerate(toks):
        pf(t.to(dev), slot=b, pos0=0)
        hs.append(pf.last32[0].clone())
        ls.append(pf.sampler.logits[b].clone())
    torch.cuda.synchronize()
    _judge(f"Prefill {kind} score modifiers", [(b, len(t) - 1) for b, t in enumerate(toks)], ref, emu, torch.stack(hs), torch.stack(ls))
    tails = (12, 1, 9, 5)
    rs = qp.RaggedStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, rows=32, segments=4, **_kw(sinks), **kw)
    items = [(b, t[len(t) - n:], len(t) - n) for b, (t, n) in enumerate(zip(toks, tails))]
    rs(*rs.pack(items))
    torch.cuda.synchronize()
    rows = [(b, p0 + r) for b, t, p0 in items for r in range(len(t))]
    _judge(f"RaggedStep {kind} score modifiers: rows", rows, ref, emu, rs.h32[:len(rows)])
    _judge(f"RaggedStep {kind} score modifiers: segments", [(b, len(t) - 1) for b, t in enumerate(toks)], ref, emu, rs.last32[:4], rs.draw.logits[:4])
    # Score: lp[i] = log p(t[i + 1] | t[:i + 1]).  log_softmax moves by at most twice the largest logit error, so the logits'
    # tolerance (relative to the row's rms) carries over with a factor of two
    sc = qp.Score(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, chunk=CHUNK, **_kw(sinks), **kw)
    worst = 0.0
    for b, t in enumerate(toks):
        lp = sc(t.to(dev), slot=b, pos0=0).double()
        nxt = t[1:].to(dev)
        want = ref.logprob[b][:-1].gather(1, nxt[:, None])[:, 0]
        tol_l = mr.tolerance(mr.e_l(emu.logits[b][:-1], ref.logits[b][:-1])) * ref.logits[b][:-1].pow(2).mean(-1).sqrt()
        worst = max(worst, float(((lp - want).abs() / (2.0 * tol_l)).max()))
    print(f"Score {kind} score modifiers: worst err / tol {worst:.3f}")
    assert worst <= 1.0


@gpu
def test_speculative_step_emits_the_modified_decode_steps_stream(dev):
    """greedy: SpeculativeStep with the modifiers emits, token for token, what DecodeStep with them emits from the same prompts"""
    import qpalette_amd as qp
    m, toks = _model(), _tokens()
    sinks = model_sinks(dev)
    P, N = 12, 24
    prompts = [t[:P] for t in toks]
    cache, kc, vc, kw = _caches(m, "fp16", dev, 4)
    pf = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, chunk=CHUNK, **_kw(sinks))
    run = _Decode(m, dev, 4, kc, vc, **_kw(sinks))
    for b in range(4):
        pf(prompts[b][:P - 1].to(dev), slot=b, pos0=0)
    seqs = [p.tolist() for p in prompts]
    for s in range(N - P):
        run.run([[(seqs[b][-1], P - 1 + s) for b in range(4)]])
        for b in range(4):
            seqs[b].append(int(run.t[-1][b]))
    cache, kc, vc, kw = _caches(m, "fp16", dev, 4)
    pf = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, chunk=CHUNK, **_kw(sinks))
    ss = qp.SpeculativeStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, draft=3, gram=(1, 2), **_kw(sinks))
    spec = [p.tolist() for p in prompts]
    for b in range(4):
        pf(prompts[b][:P - 1].to(dev), slot=b, pos0=0)
        ss.begin(b, spec[b], limit=N)
    for _ in range(N):
        out_tok, n_out = ss()
        torch.cuda.synchronize()
        for b in range(4):
            spec[b] += out_tok[b, :int(n_out[b])].tolist()
        if all(len(s) >= N for s in spec):
            break
    assert [s[:N] for s in spec] == [s[:N] for s in seqs]
    # and the modifiers are not idle: the plain model's stream differs
    cache, kc, vc, kw = _caches(m, "fp16", dev, 4)
    pf = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, chunk=CHUNK)
    plain = _Decode(m, dev, 4, kc, vc)
    for b in range(4):
        pf(prompts[b][:P - 1].to(dev), slot=b, pos0=0)
    other = [p.tolist() for p in prompts]
    for s in range(N - P):
        plain.run([[(other[b][-1], P - 1 + s) for b in range(4)]])
        for b in range(4):
            other[b].append(int(plain.t[-1][b]))
    assert other != seqs


@gpu
def test_a_captured_decode_step_follows_sinks_changed_in_place(dev, monkeypatch):
    """ONE captured graph of the batch-1 DecodeStep replayed over a slot's tokens from position 0, twice: between the two passes the
    sinks tensor is overwritten in place.  Each pass agrees with the float64 model that has ITS sinks (the launches read the sinks on
    the device at every replay), and the two passes differ."""
    m, toks = _model(), _tokens()[2:3]
    first, second = model_sinks(dev, seed=5), model_sinks(dev, seed=6, shift=2.0)
    sinks = first.clone()
    _, kc, vc, _ = _caches(m, "fp16", dev, 1)
    run = _Decode(m, dev, 1, kc, vc, **_kw(sinks))
    run.tok.fill_(int(toks[0][0]))
    run.pos.fill_(0)
    run.step()  # (warm-up outside the capture: position 0 is written again by the first replay)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run.step()
    passes = []
    for values in (first, second):
        sinks.copy_(values)
        hs, ls = [], []
        for s, t in enumerate(toks[0].tolist()):
            run.tok.fill_(t)
            run.pos.fill_(s)
            graph.replay()
            torch.cuda.synchronize()
            hs.append(run.step.h32[0].clone())
            ls.append(run.smp.logits[0].clone())
        passes.append((torch.stack(hs), torch.stack(ls)))
        ref, emu = refs(monkeypatch, m.ref, toks, dev, False, sinks=values)
        _judge(f"captured DecodeStep, sinks pass {len(passes)}", [(0, s) for s in range(len(toks[0]))], ref, emu, *passes[-1])
    assert float((passes[0][0].double() - passes[1][0].double()).abs().max()) > 1e-3


@gpu
def test_with_both_modifiers_none_every_class_is_its_parents_launch(dev):
    """softcap=None, sinks=None, attn_scale=None: the attention launch of every layer of all five step classes, on the SAME q | k | v
    rows and caches, is bit for bit the launch of the step built without the keywords (no projection in between: reproducible on
    every run), outputs and caches; the batch-1 step keeps the fused single-sequence kernel, and takes the batched one with either
    modifier"""
    import qpalette_amd as qp
    m = _model()
    H, kvw = m.cfg.hidden_size, m.cfg.num_key_value_heads * m.cfg.head_dim
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)  # noqa: E731
    i64 = lambda x: torch.tensor(x, dtype=torch.int64, device=dev)  # noqa: E731
    got = {}
    for name_kw, kw in (("parent", {}), ("none", dict(softcap=None, sinks=None, attn_scale=None)), ("none-per-layer", dict(softcap=(None, None)))):
        g = torch.Generator(device=dev).manual_seed(11)
        cache, kc, vc, _ = _caches(m, "fp16", dev, 4)
        for c in kc + vc:
            c.copy_(0.5 * torch.randn(c.shape, device=dev, generator=g))
        args = (m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq)
        tok, out_tok = torch.zeros(4, dtype=torch.long, device=dev), torch.zeros(4, dtype=torch.long, device=dev)
        b1 = args[:4] + ([c[:1] for c in kc], [c[:1] for c in vc], m.inv_freq)
        steps = {"decode": qp.DecodeStep(*args, tok, i64([10, 63, 30, -1]), out_tok, **kw),
                 "decode-b1": qp.DecodeStep(*b1, tok[:1], i64([40]), out_tok[:1], **kw),
                 "prefill": qp.Prefill(*args, chunk=CHUNK, **kw), "score": qp.Score(*args, chunk=CHUNK, **kw),
                 "ragged": qp.RaggedStep(*args, rows=32, segments=4, **kw), "spec": qp.SpeculativeStep(*args, draft=3, **kw)}
        assert steps["decode-b1"].batch1 and not steps["decode-b1"].attn_batch
        assert all(s.attn_scale == 0.125 and s.softcap == [None] * NL and s.sinks is None for s in steps.values())
        for name, slot, pos in (("prefill", 1, 7), ("score", 2, 40)):
            steps[name].slot = slot
            steps[name].pos.fill_(pos)
        steps["ragged"].seq, steps["ragged"].row0, steps["ragged"].pos0 = i32([3, 0, -1, 1]), i32([0, 17, 18, 18, 30]), i64([5, 63, 0, 33])
        steps["spec"].seq.copy_(i32([0, 1, 2, -1]))
        steps["spec"].row0.copy_(i32([0, 4, 6, 10, 10]))
        steps["spec"].pos0.copy_(i64([60, 0, 21, 0]))
        res = []
        for name, step in steps.items():
            rows = step.qkv32.shape[0]
            q, k, v = torch.randn(rows, H + 2 * kvw, device=dev, generator=g).split([H, kvw, kvw], dim=1)
            for i in range(NL):
                out = torch.zeros(rows, H, dtype=torch.float16, device=dev)
                step._attention(i, q, k, v, out)
                res.append(out)
        torch.cuda.synchronize()
        got[name_kw] = res + [c.clone() for c in kc + vc]
    for name_kw in ("none", "none-per-layer"):
        assert len(got[name_kw]) == len(got["parent"]) == 6 * NL + 2 * NL
        for i, (a, b) in enumerate(zip(got[name_kw], got["parent"])):
            assert torch.equal(_bits(a), _bits(b)), (name_kw, i)
    _, kc, vc, _ = _caches(m, "fp16", dev, 1)
    for kw in (dict(softcap=8.0), dict(sinks=torch.zeros(NL, NQ, device=dev)), dict(softcap=(None, 8.0))):
        step = qp.DecodeStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, tok[:1], i64([0]), out_tok[:1], **kw)
        assert step.batch1 and step.attn_batch
