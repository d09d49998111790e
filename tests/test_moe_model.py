"""Sparse layers in the step classes (qpalette_amd/decoder.py `_moe`): model_reference's small model (geometry
"S", 3 layers, context 64) with layers 0 and 2 sparse (E = 8, top_k = 2, expert I = 512, tcq_6 up / gate and tcomb_6_7_0.5 down)
and layer 1 dense.  Every sparse layer of every step is held to the float64 contract on the rows it was given: the step's own
stream in front of the layer and behind it are recorded, and the difference must lie within moe_reference.layer_reference's bound
of reference_moe_mlp on each expert's decoded weights, on the rows whose routing is decidable."""
import functools
import types

import numpy as np
import pytest
import torch

import model_reference as mr
import moe_model_reference as mmr
import moe_reference as mref
from test_model_exact import _judge
from test_moe import _layer, decoded
from test_window_model import _caches, _Decode, _forced, _reproducible_projections

pytestmark = pytest.mark.gpu
NL, SPARSE, E, TOP_K, I = 3, (0, 2), 8, 2, 512
UNDECIDABLE_CAP = 0.10


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
def _world(renorm=True):
    import qpalette_amd as qp
    d = torch.device("cuda", 0)
    spec, sparse = mmr.world(renorm)
    m = mr.build("S", "mixed", (), NL, mr.VOCAB, 0, d, spec=spec)
    mm = types.SimpleNamespace(**vars(m))
    mm.layers = torch.nn.ModuleList(list(m.layers))
    mm.sparse = {}
    for i in SPARSE:
        experts, router, su_ug, su_dp = _layer(qp, E=E, H=m.cfg.hidden_size, I=I, seed=100 + i)
        for _, _, down in experts:   # moe_model_reference.world's calibration: a power of two, exact in fp16
            down.Wscale.data.mul_(sparse[i].factor)
        layer = torch.nn.Module()
        layer.self_attn, layer.input_layernorm = m.layers[i].self_attn, m.layers[i].input_layernorm
        layer.post_attention_layernorm = m.layers[i].post_attention_layernorm
        layer.mlp = qp.MoEMLP.from_experts(router, experts, TOP_K, renorm=renorm)
        mm.layers[i] = layer
        assert all(np.array_equal(a, b) for ta, tb in zip(decoded(experts), sparse[i].What) for a, b in zip(ta, tb))   # the CPU twin
        mm.sparse[i] = types.SimpleNamespace(What=sparse[i].What, su_ug=su_ug, su_dp=su_dp, scale=experts[0][0].scale,
                                             router=router.cpu().numpy(), rms_w=layer.post_attention_layernorm.weight.cpu().numpy(),
                                             eps=layer.post_attention_layernorm.eps)
    mm.ref_model, mm.ref_sparse = spec.ref, sparse
    return mm


def _model_refs(mm, name):
    """(tokens, float64 forward, emulation, {(slot, position): routing-decidable}) of a token set of moe_model_reference, on the CPU"""
    seed, lens, prefill = mmr.TOKEN_SETS[name]
    toks = mmr.tokens(seed, lens)
    ref = mmr.forward(mm.ref_model, mm.ref_sparse, toks)
    emu = mmr.forward(mm.ref_model, mm.ref_sparse, toks, emu=True, prefill=prefill)
    return toks, ref, emu, mmr.routing_decidable(ref, emu, toks)


def test_decode_against_the_float64_model(dev):
    """DecodeStep at B = 4 with one inactive slot, and at B = 1: stream, logits and greedy tokens of every routing-decidable row
    against the float64 forward of the model with its sparse layers, within model_reference.tolerance (4 x the emulation's own
    distance); the seeded defects miss that bar by more than TEETH on the CPU (tests/test_moe_contract.py)"""
    mm = _world()
    toks, ref, emu, ok = _model_refs(mm, "decode")
    for B, slots in ((4, None), (1, [1])):
        sel = toks if slots is None else [toks[b] for b in slots]
        _, kc, vc, ckw = _caches(mm, "fp16", dev, B)
        run = _Decode(mm, dev, B, kc, vc, **ckw)
        plan = _forced(sel)
        run.run(plan)
        picks = [(s, b) for s, row in enumerate(plan) for b, r in enumerate(row) if r is not None]
        picks = [(s, b) for s, b in picks if ok[(b if slots is None else slots[b], s)]]
        rows = [(b if slots is None else slots[b], s) for s, b in picks]
        assert len(rows) >= 0.9 * sum(len(t) for t in sel)
        _judge(f"DecodeStep B={B} sparse", rows, ref, emu, torch.stack([run.h[s][b] for s, b in picks]).cpu(),
               torch.stack([run.l[s][b] for s, b in picks]).cpu(), torch.stack([run.t[s][b] for s, b in picks]).cpu(),
               cap=None if slots else 0.10)   # (the cap is the token set's, asserted on the CPU; one slot alone is a part of it)


def test_prefill_and_ragged_against_the_float64_model(dev):
    import qpalette_amd as qp
    mm = _world()
    toks, ref, emu, ok = _model_refs(mm, "prefill")
    _, kc, vc, _ = _caches(mm, "fp16", dev, 3)
    args = (mm.layers, mm.embed, mm.norm, mm.lm_head, kc, vc, mm.inv_freq)
    pf = qp.Prefill(*args, chunk=16, sampler=qp.Sampler(3, mr.VOCAB, dev, temperature=0.0))
    hs, ls, ts = [], [], []
    for b, t in enumerate(toks):
        ts.append(pf(t.to(dev), slot=b, pos0=0).clone()[0])
        hs.append(pf.last32[0].clone())
        ls.append(pf.sampler.logits[b].clone())
    torch.cuda.synchronize()
    keep = [b for b, t in enumerate(toks) if ok[(b, len(t) - 1)]]
    assert len(keep) >= 2
    last = [(b, len(toks[b]) - 1) for b in keep]
    _judge("Prefill sparse", last, ref, emu, torch.stack(hs)[keep].cpu(), torch.stack(ls)[keep].cpu(), torch.stack(ts)[keep].cpu())
    tails = (1, 5, 4)
    rs = qp.RaggedStep(*args, rows=32, segments=3)
    items = [(b, t[len(t) - n:], len(t) - n) for b, (t, n) in enumerate(zip(toks, tails))]
    rs(*rs.pack(items))
    torch.cuda.synchronize()
    rows = [(b, p0 + r) for b, t, p0 in items for r in range(len(t))]
    at = [i for i, r in enumerate(rows) if ok[r]]
    assert len(at) >= 0.8 * len(rows)
    _judge("RaggedStep sparse: rows", [rows[i] for i in at], ref, emu, rs.h32[:len(rows)][at].cpu(), None, None)


def _record(step):
    """every call of step._moe: (layer, the stream rows in front, the layer's output as the step left it, the activity vector)"""
    rec, orig = [], step._moe

    def moe(i, h32):
        before = h32.clone()
        orig(i, h32)
        out = (h32 - before) if step.post_norms is None else step.y32[:h32.shape[0]].clone()
        act = step._moe_active()
        rec.append((i, before, out, None if act is None else act.clone()))
    step._moe = moe
    return rec


def _check(mm, rec, case, renorm=True, min_rows=1):
    """every recorded sparse layer within the layer tolerance (moe_reference.layer_judge: KAPPA x the format emulation's own distance
    from the float64 layer, the bar tests/test_moe_contract.py shows every seeded defect to miss by more than TEETH) on the rows
    whose routing is decidable; at most UNDECIDABLE_CAP of the rows are not"""
    import qpalette_amd as qp
    seen, und, worst = 0, 0, 0.0
    for i, before, out, act in rec:
        sp = mm.sparse[i]
        h = before.cpu().numpy()
        active = None if act is None else act.cpu().numpy()[:h.shape[0]]
        rt = qp.moe.reference_route(h, sp.rms_w, sp.eps, sp.router, None, TOP_K, renorm, active)
        live = np.ones(len(h), dtype=bool) if active is None else active >= 0
        ok = mref.decidable_rows(rt, mref.logit_bounds(rt, sp.router), TOP_K, active) & live
        got = out.cpu().numpy().astype(np.float64)
        assert (got[~live] == 0).all(), (case, i)                         # an idle row is left alone
        if ok.any():
            f, rows = mref.layer_judge(sp.What, sp.su_ug, sp.su_dp, sp.scale, rt, ok, got)
            assert (f <= 1.0).all(), (case, i, rows[f > 1.0].tolist(), float(f.max()))
            worst = max(worst, float(f.max()))
        seen, und = seen + int(live.sum()), und + int((live & ~ok).sum())
    print(f"{case}: {seen} rows in sparse layers, {und} undecidable, max distance / tolerance {worst:.3f}")
    assert seen >= min_rows and und <= UNDECIDABLE_CAP * seen, (case, seen, und)


def _tokens(seed, lens):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, mr.VOCAB, (n,), generator=g) for n in lens]


def test_decode_b4_one_idle_slot_and_launch_count(dev):
    mm = _world()
    toks = _tokens(41, (9, 7, 0, 8))
    _, kc, vc, ckw = _caches(mm, "fp16", dev, 4)
    run = _Decode(mm, dev, 4, kc, vc, **ckw)
    rec = _record(run.step)
    run.run(_forced(toks))
    _check(mm, rec, "DecodeStep B=4", min_rows=40)
    assert run.step.launches_per_token == 9 * NL + (6 - 4) * len(SPARSE) + 2


def test_decode_b1_graph_replays_with_changing_routes(dev, monkeypatch):
    """a captured batch-1 step replays over positions whose routing differs: every replay equals the eager step, bit for bit (the
    dense projections on test_window_model's stand-in without float atomics; the routed launches are the library's and have none)"""
    mm = _world()
    _reproducible_projections(monkeypatch)
    toks = _tokens(43, (10,))[0]
    outs = []
    for graphed in (False, True):
        _, kc, vc, ckw = _caches(mm, "fp16", dev, 1)
        run = _Decode(mm, dev, 1, kc, vc, **ckw)
        assert run.step.batch1
        rec = _record(run.step) if not graphed else None
        hs, sels = [], []
        graph = None
        if graphed:
            run.tok.fill_(int(toks[0])), run.pos.fill_(0)
            run.step()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                run.step()
        for p, t in enumerate(toks.tolist()):
            run.tok.fill_(t), run.pos.fill_(p)
            graph.replay() if graphed else run.step()
            torch.cuda.synchronize()
            hs.append(run.step.h32.clone())
            sels.append(tuple(next(iter(run.step.moe_ws.values())).sel.cpu().numpy().ravel().tolist()))   # (the last sparse layer's)
        outs.append((torch.stack(hs), sels))
        if not graphed:
            _check(mm, rec, "DecodeStep B=1", min_rows=2 * len(toks))
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]
    assert len(set(outs[1][1])) > 1   # the routing did change from token to token
    assert run.step.launches_per_token == (6 if run.step.rot_in_gemv else 9) * NL + (6 - (3 if run.step.rot_in_gemv else 4)) * len(SPARSE) + 2


def test_prefill_ragged_and_paged_e4m3(dev):
    import qpalette_amd as qp
    mm = _world()
    toks = _tokens(42, (21, 16, 5))
    _, kc, vc, _ = _caches(mm, "fp16", dev, 3)
    args = (mm.layers, mm.embed, mm.norm, mm.lm_head, kc, vc, mm.inv_freq)
    pf = qp.Prefill(*args, chunk=16)
    rec = _record(pf)
    for b, t in enumerate(toks):
        pf(t.to(dev), slot=b, pos0=0)
    torch.cuda.synchronize()
    _check(mm, rec, "Prefill", min_rows=2 * 42)
    rs = qp.RaggedStep(*args, rows=32, segments=3)
    rec = _record(rs)
    rs(*rs.pack([(b, t[len(t) - n:], len(t) - n) for b, (t, n) in enumerate(zip(toks, (1, 5, 4)))]))
    torch.cuda.synchronize()
    _check(mm, [(i, b[:10], o[:10], None) for i, b, o, _ in rec], "RaggedStep", min_rows=20)
    sc = qp.Score(*args, chunk=16)
    rec = _record(sc)
    sc(toks[0].to(dev), slot=0, pos0=0)
    torch.cuda.synchronize()
    _check(mm, rec, "Score", min_rows=40)
    # a paged e4m3 decode
    cache, kc, vc, ckw = _caches(mm, "paged-e4m3", dev, 4)
    dt = _tokens(44, (6, 0, 5, 6))
    for b, t in enumerate(dt):
        if len(t):
            cache.reserve(b, len(t))
    run = _Decode(mm, dev, 4, kc, vc, **ckw)
    rec = _record(run.step)
    run.run(_forced(dt))
    _check(mm, rec, "DecodeStep paged e4m3", min_rows=30)


def test_post_norms_and_no_renorm(dev):
    mm = _world()
    H = mm.cfg.hidden_size
    g = torch.Generator().manual_seed(5)
    post = (1e-6, (1 + 0.2 * torch.randn(NL, 2, H, generator=g)).to(dev))
    toks = _tokens(45, (6, 5, 0, 6))
    _, kc, vc, ckw = _caches(mm, "fp16", dev, 4)
    run = _Decode(mm, dev, 4, kc, vc, post_norms=post, **ckw)
    rec = _record(run.step)
    run.run(_forced(toks))
    _check(mm, rec, "DecodeStep post_norms", min_rows=30)
    assert run.step.launches_per_token == (9 + 2) * NL + 2 * len(SPARSE) + 2
    m2 = _world(False)
    _, kc, vc, ckw = _caches(m2, "fp16", dev, 4)
    run = _Decode(m2, dev, 4, kc, vc, **ckw)
    rec = _record(run.step)
    run.run(_forced(toks))
    _check(m2, rec, "DecodeStep renorm=False", renorm=False, min_rows=30)


def test_refused_combinations_raise(dev):
    import qpalette_amd as qp
    mm = _world()
    _, kc, vc, _ = _caches(mm, "fp16", dev, 4)
    tok, pos, out = (torch.zeros(4, dtype=torch.long, device=dev) for _ in range(3))
    args = (mm.layers, mm.embed, mm.norm, mm.lm_head, kc, vc, mm.inv_freq)
    with pytest.raises(qp._native.QpalError, match="gelu_tanh.*MoE"):
        qp.DecodeStep(*args, tok, pos, out, mlp_act="gelu_tanh")
    with pytest.raises(qp._native.QpalError, match="adapters= on a model with MoE layers"):
        qp.DecodeStep(*args, tok, pos, out, adapters=object())
    for cls in (qp.Prefill, qp.Score, qp.RaggedStep, qp.SpeculativeStep):
        with pytest.raises(qp._native.QpalError, match="gelu_tanh.*MoE"):
            cls(*args, mlp_act="gelu_tanh")


def test_speculative_step_emits_the_sequential_tokens(dev):
    """draft = 3.  A greedy DecodeStep first generates K + 1 tokens per slot from the prefilled prompts; those tokens are then the
    caller's drafts of a SpeculativeStep on its own copy of the prefilled caches: it must accept them all and emit the same K + 1
    tokens, wherever the sequential run's own top-two logit gap is not a near-tie (two correct runs through different attention
    launches differ by a few fp16 roundings of the logits: a gap above 2^-6 of the row's logit rms, 32 fp16 roundings, is judged).
    Every sparse layer of the verify step is also held to the layer tolerance.  Slot 2 is never begun."""
    import qpalette_amd as qp
    mm = _world()
    P, K = 12, 3
    toks = _tokens(46, (12, 12, 0, 12))
    live = [b for b, t in enumerate(toks) if len(t)]
    caches = [_caches(mm, "fp16", dev, 4) for _ in range(2)]
    for _, kc, vc, _ in caches:
        pf = qp.Prefill(mm.layers, mm.embed, mm.norm, mm.lm_head, kc, vc, mm.inv_freq, chunk=16)
        for b in live:
            pf(toks[b][:P - 1].to(dev), slot=b, pos0=0)
    # sequential greedy sampling
    _, kc, vc, ckw = caches[0]
    run = _Decode(mm, dev, 4, kc, vc, **ckw)
    seq, near = [], []
    feed = [int(toks[b][P - 1]) if b in live else None for b in range(4)]
    for s in range(K + 1):
        run.run([[None if f is None else (f, P - 1 + s) for f in feed]])
        lg = run.l[-1].double()
        top = lg.topk(2, dim=-1).values
        near.append(((top[:, 0] - top[:, 1]) <= 2.0 ** -6 * lg.pow(2).mean(-1).sqrt()).cpu())
        seq.append(run.t[-1].cpu())
        feed = [int(seq[-1][b]) if b in live else None for b in range(4)]
    seq, near = torch.stack(seq, 1), torch.stack(near, 1)          # [4, K + 1]
    # the verify step with those tokens as drafts
    _, kc, vc, _ = caches[1]
    ss = qp.SpeculativeStep(mm.layers, mm.embed, mm.norm, mm.lm_head, kc, vc, mm.inv_freq, draft=K,
                            sampler=qp.Sampler(4, mr.VOCAB, dev, temperature=0.0))
    for b in live:
        ss.begin(b, toks[b][:P].tolist())
    rec = _record(ss)
    out_tok, n_out = ss(seq[:, :K].to(dev), torch.full((4,), K, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    assert int(n_out[2]) == 0
    judged = 0
    for b in live:
        clear = int((~near[b]).long().cumprod(0).sum())              # tokens in front of the first near-tie
        assert int(n_out[b]) >= min(clear, K + 1) >= 0
        m = min(clear, int(n_out[b]))
        assert out_tok[b, :m].cpu().tolist() == seq[b, :m].tolist(), (b, out_tok[b].tolist(), seq[b].tolist())
        judged += m
    print(f"SpeculativeStep: {judged} emitted tokens equal to the sequential ones")
    assert judged >= 2 * len(live)
    row0 = ss.row0.tolist()
    at = torch.tensor([row0[b] + j for b in live for j in range(K + 1)], device=dev)
    _check(mm, [(i, x[at], o[at], None) for i, x, o, _ in rec], "SpeculativeStep", min_rows=2 * len(at))
