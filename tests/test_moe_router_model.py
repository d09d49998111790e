"""Sparse layers of the second router with shared experts in the step classes (qpalette_amd/decoder.py `_moe`):
model_reference's small model (geometry "S", 3 layers, context 64) with layer 0 a sigmoid router with a select bias, 4 groups of
which 2 are allowed by "top2", and a gated shared expert; layer 1 dense; layer 2 a softmax router with "max" groups, a routed scale
and an ungated shared expert that reads the experts' rotated rows (moe_router_model_reference.ROUTERS).  The steps are judged
against the float64 forward of that model on the routing-decidable rows, within model_reference.tolerance; the seeded defects miss
that bar by more than TEETH on the CPU (tests/test_moe_router_contract.py)."""
import functools
import types

import numpy as np
import pytest
import torch

import model_reference as mr
import moe_router_model_reference as mm
from test_model_exact import _judge
from test_moe import _cuda, _layer, decoded
from test_moe_router import shared_decoded, shared_mlp
from test_window_model import _caches, _Decode, _forced, _reproducible_projections

pytestmark = pytest.mark.gpu
NL, SPARSE, E, TOP_K, I = mm.NL, mm.SPARSE, mm.E, mm.TOP_K, mm.I


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
def _world():
    import qpalette_amd as qp
    d = torch.device("cuda", 0)
    spec, sparse = mm.world()
    m = mr.build("S", "mixed", (), NL, mr.VOCAB, 0, d, spec=spec)
    w = types.SimpleNamespace(**vars(m))
    w.layers = torch.nn.ModuleList(list(m.layers))
    H = m.cfg.hidden_size
    for i in SPARSE:
        scoring, G, tg, gs, renorm, biased, gated, same_su = mm.ROUTERS[i]
        sp = sparse[i]
        experts, router_w, su_ug, su_dp = _layer(qp, E=E, H=H, I=I, seed=100 + i)
        if scoring == "sigmoid":
            router_w = router_w / 4
        shared, _, _ = shared_mlp(qp, H, mm.IS, su_ug=su_ug if same_su else None, seed=900 + i)
        for _, _, down in experts:   # moe_router_model_reference.world's calibration: a power of two, exact in fp16
            down.Wscale.data.mul_(sp.factor)
        shared.Wscale_dp.data.mul_(sp.factor)
        layer = torch.nn.Module()
        layer.self_attn, layer.input_layernorm = m.layers[i].self_attn, m.layers[i].input_layernorm
        layer.post_attention_layernorm = m.layers[i].post_attention_layernorm
        layer.mlp = qp.MoEMLP.from_experts(router_w, experts, TOP_K, renorm=renorm, scoring=scoring, select_bias=_cuda(sp.router.select_bias),
                                           n_group=G, topk_group=tg, group_score=gs, routed_scale=sp.router.routed_scale, shared=shared,
                                           shared_gate=_cuda(sp.router.shared_gate))
        assert layer.mlp.shared_x16 == same_su
        w.layers[i] = layer
        # the CPU twin: the same decoded weights, the same router
        assert all(np.array_equal(a, b) for ta, tb in zip(decoded(experts), sp.world[0]) for a, b in zip(ta, tb))
        assert all(np.array_equal(a, b) for a, b in zip(shared_decoded(shared), sp.world[4]))
        assert np.array_equal(router_w.cpu().numpy(), sp.router_w)
    w.ref_model, w.ref_sparse = spec.ref, sparse
    return w


def _model_refs(w, name):
    """(tokens, float64 forward, emulation, {(slot, position): routing-decidable}) of a token set, on the CPU"""
    seed, lens, prefill = mm.TOKEN_SETS[name]
    toks = mm.tokens(seed, lens)
    ref = mm.forward(w.ref_model, w.ref_sparse, toks)
    emu = mm.forward(w.ref_model, w.ref_sparse, toks, emu=True, prefill=prefill)
    return toks, ref, emu, mm.routing_decidable(ref, emu, toks, w.ref_sparse)


def test_decode_against_the_float64_model(dev):
    """DecodeStep at B = 4 with one idle slot, and at B = 1: stream, logits and greedy tokens of every routing-decidable row; the
    launch count of the step with its two kinds of shared expert (4 and 3 launches more than a plain sparse layer's six)"""
    w = _world()
    toks, ref, emu, ok = _model_refs(w, "decode")
    for B, slots in ((4, None), (1, [0])):   # (slot 0: the set's one routing-undecidable row lies in slot 1)
        sel = toks if slots is None else [toks[b] for b in slots]
        _, kc, vc, ckw = _caches(w, "fp16", dev, B)
        run = _Decode(w, dev, B, kc, vc, **ckw)
        plan = _forced(sel)
        run.run(plan)
        picks = [(s, b) for s, row in enumerate(plan) for b, r in enumerate(row) if r is not None]
        picks = [(s, b) for s, b in picks if ok[(b if slots is None else slots[b], s)]]
        rows = [(b if slots is None else slots[b], s) for s, b in picks]
        assert len(rows) >= 0.9 * sum(len(t) for t in sel)
        _judge(f"DecodeStep B={B} router", rows, ref, emu, torch.stack([run.h[s][b] for s, b in picks]).cpu(),
               torch.stack([run.l[s][b] for s, b in picks]).cpu(), torch.stack([run.t[s][b] for s, b in picks]).cpu(),
               cap=None if slots else 0.10)
        dense = 3 if run.step.rot_in_gemv else 4
        assert [w.layers[i].mlp.launches(B) for i in SPARSE] == [10, 9]
        assert run.step.launches_per_token == ((6 if run.step.rot_in_gemv else 9) * NL + (10 - dense) + (9 - dense) + 2)


def test_prefill_and_ragged_against_the_float64_model(dev):
    import qpalette_amd as qp
    w = _world()
    toks, ref, emu, ok = _model_refs(w, "prefill")
    _, kc, vc, _ = _caches(w, "fp16", dev, 3)
    args = (w.layers, w.embed, w.norm, w.lm_head, kc, vc, w.inv_freq)
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
    _judge("Prefill router", last, ref, emu, torch.stack(hs)[keep].cpu(), torch.stack(ls)[keep].cpu(), torch.stack(ts)[keep].cpu())
    tails = (1, 5, 4)
    rs = qp.RaggedStep(*args, rows=32, segments=3)
    items = [(b, t[len(t) - n:], len(t) - n) for b, (t, n) in enumerate(zip(toks, tails))]
    rs(*rs.pack(items))
    torch.cuda.synchronize()
    rows = [(b, p0 + r) for b, t, p0 in items for r in range(len(t))]
    at = [i for i, r in enumerate(rows) if ok[r]]
    assert len(at) >= 0.8 * len(rows)
    _judge("RaggedStep router: rows", [rows[i] for i in at], ref, emu, rs.h32[:len(rows)][at].cpu(), None, None)


def test_captured_decode_replays_with_changing_routes_and_gates(dev, monkeypatch):
    """a captured batch-1 step replays over 8 positions whose routing and shared gates differ: every replay equals the eager step,
    bit for bit (the dense projections, the shared experts' too, on test_window_model's stand-in without float atomics; the
    routed launches are the library's and have none)"""
    import qpalette_amd as qp
    w = _world()
    _reproducible_projections(monkeypatch)
    monkeypatch.setattr(qp.linear, "multi_gemv", qp.decoder.multi_gemv)   # (moe.py calls linear.multi_gemv for the shared expert)
    toks = mm.tokens(47, (8,))[0]
    outs = []
    for graphed in (False, True):
        _, kc, vc, ckw = _caches(w, "fp16", dev, 1)
        run = _Decode(w, dev, 1, kc, vc, **ckw)
        ws0 = run.step.moe_ws[w.layers[0].mlp.shape_key()]
        assert ws0.sgate is not None
        graph = None
        if graphed:
            run.tok.fill_(int(toks[0])), run.pos.fill_(0)
            run.step()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                run.step()
        hs, sels, gates = [], [], []
        for p, t in enumerate(toks.tolist()):
            run.tok.fill_(t), run.pos.fill_(p)
            graph.replay() if graphed else run.step()
            torch.cuda.synchronize()
            hs.append(run.step.h32.clone())
            sels.append(tuple(ws0.sel.cpu().numpy().ravel().tolist()))   # (one workspace serves both sparse layers: these are the last one's)
            gates.append(float(ws0.sgate[0]))
        outs.append((torch.stack(hs), sels, gates))
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1] and outs[0][2] == outs[1][2]
    assert len(set(outs[1][1])) > 1   # the routing did change from token to token


def test_gated_layer_shared_gates_change_under_replay(dev):
    """the gated layer alone under a graph: the shared gates written by a replay follow the rows (they are no constants of the capture)"""
    w = _world()
    layer = w.layers[0].mlp
    rms = (1e-5, w.layers[0].post_attention_layernorm.weight)
    ws = layer.new_workspace(4)
    g = torch.Generator().manual_seed(3)
    h = torch.randn(4, layer.hidden_size, generator=g).to(dev)
    out = torch.zeros_like(h)
    layer.run(h, rms, out, False, ws=ws)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        layer.run(h, rms, out, False, ws=ws)
    seen = []
    for s in range(3):
        h.copy_(torch.randn(4, layer.hidden_size, generator=g))
        graph.replay()
        torch.cuda.synchronize()
        rt = mm.moe.reference_route_ex(h.cpu().numpy(), rms[1].cpu().numpy(), 1e-5, w.ref_sparse[0].router_w, None, TOP_K, w.ref_sparse[0].router)
        assert np.abs(ws.sgate.cpu().numpy() - rt["sgate"]).max() <= 1e-4
        seen.append(ws.sgate.cpu().numpy().copy())
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


def test_refused_combinations_still_raise(dev):
    import qpalette_amd as qp
    w = _world()
    _, kc, vc, _ = _caches(w, "fp16", dev, 4)
    tok, pos, out = (torch.zeros(4, dtype=torch.long, device=dev) for _ in range(3))
    args = (w.layers, w.embed, w.norm, w.lm_head, kc, vc, w.inv_freq)
    with pytest.raises(qp._native.QpalError, match="gelu_tanh.*MoE"):
        qp.DecodeStep(*args, tok, pos, out, mlp_act="gelu_tanh")
    with pytest.raises(qp._native.QpalError, match="adapters= on a model with MoE layers"):
        qp.DecodeStep(*args, tok, pos, out, adapters=object())
    for cls in (qp.Prefill, qp.Score, qp.RaggedStep, qp.SpeculativeStep):
        with pytest.raises(qp._native.QpalError, match="gelu_tanh.*MoE"):
            cls(*args, mlp_act="gelu_tanh")


def test_speculative_step_accepts_a_greedy_runs_own_tokens(dev):
    """draft = 3, as test_moe_model's: the tokens a greedy DecodeStep generates from the prefilled prompts are the drafts of a
    SpeculativeStep on its own copy of the caches, which must emit them wherever the sequential run's top-two logit gap is no
    near-tie (above 2^-6 of the row's logit rms).  Slot 2 is never begun."""
    import qpalette_amd as qp
    w = _world()
    P, K = 12, 3
    toks = mm.tokens(46, (12, 12, 0, 12))
    live = [b for b, t in enumerate(toks) if len(t)]
    caches = [_caches(w, "fp16", dev, 4) for _ in range(2)]
    for _, kc, vc, _ in caches:
        pf = qp.Prefill(w.layers, w.embed, w.norm, w.lm_head, kc, vc, w.inv_freq, chunk=16)
        for b in live:
            pf(toks[b][:P - 1].to(dev), slot=b, pos0=0)
    _, kc, vc, ckw = caches[0]
    run = _Decode(w, dev, 4, kc, vc, **ckw)
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
    _, kc, vc, _ = caches[1]
    ss = qp.SpeculativeStep(w.layers, w.embed, w.norm, w.lm_head, kc, vc, w.inv_freq, draft=K,
                            sampler=qp.Sampler(4, mr.VOCAB, dev, temperature=0.0))
    for b in live:
        ss.begin(b, toks[b][:P].tolist())
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
