"""The routed skinny GEMM on the GPU (csrc/moe_gemm.hip): qpal_moe_gemm against the CPU oracle's float64 sum at the
run lengths that cross a table entry (8), an MFMA group (16) and the widest chunk (128); a row's bits against the row alone; the guards;
MoEMLP(wide=True) in a layer and in the steps.  Bounds and helpers: tests/test_moe.py, tests/moe_reference.py."""
import numpy as np
import pytest
import torch

import gemv_reference as gref
import model_reference as mr
import moe_reference as mref
from test_model_exact import _judge
from test_moe import E4, GEMV_RTOL_ABS, SENTINEL, _cuda, _experts, _layer, _table, oracle, qp  # noqa: F401 (fixtures)
from test_moe_model import _model_refs, _world
from test_window_model import _caches, _Decode, _forced, _reproducible_projections

pytestmark = pytest.mark.gpu
WAVES = 8   # supertile rows of a workgroup (moe_gemm.hip): m = 32 (WAVES + 1) leaves the last block of rows nearly empty


def _run(qp, projs, x, tlut, table, x_index, P, oscale, width, max_run=128):
    out = torch.full((P + 3, width + 8), SENTINEL, dtype=torch.float32, device="cuda")   # rows and columns nobody may write
    if x_index is not None and x_index.numel() < P + 3:
        x_index = torch.cat([x_index, torch.full((P + 3 - x_index.numel(),), -1, dtype=torch.int32, device="cuda")])
    qp.moe.moe_gemm(out, projs, x, tlut, *table, x_index=x_index, oscale=oscale, max_run=max_run)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _case(qp, oracle, k, m, qstr, nproj, indexed, exact, seed, counts, max_run=128):
    """test_moe._gemv_case with the rows per expert given: 1e-5 sum |w x| against the oracle, EQUAL on exactly summable inputs"""
    n = sum(counts)
    sel = np.repeat(np.arange(E4), counts)[np.random.default_rng(seed).permutation(n)].reshape(n, 1)
    lay = qp.moe.reference_layout(sel, E4)
    made = [_experts(qp, k, m, qstr, seed + 10 * j, exact, cb_seed=seed) for j in range(nproj)]
    projs, tlut = [t[0] for t in made], made[0][3]
    xs = gref.exact_x(n, k, seed) if exact else np.random.default_rng(seed + 1).standard_normal((n, k)).astype(np.float16)
    xi = lay["x_index"][:n]
    x_dev = _cuda(xs if indexed else xs[xi])
    oscale = 2.0 if exact else 3.0
    if exact:
        gref.assert_budget(k, xmax=3.0, scale_max=2.0 * oscale, scale_min=0.5 * oscale)
    got = _run(qp, projs, x_dev, tlut, _table(lay), _cuda(xi.astype(np.int32)) if indexed else None, n, oscale, nproj * m, max_run)
    assert (got[n:] == SENTINEL).all() and (got[:, nproj * m:] == SENTINEL).all()
    experts = sel[lay["order"][:n], 0]
    for j, (_, W, ws, _) in enumerate(made):
        for e in np.unique(experts):
            pos = np.nonzero(experts == e)[0]
            ref, mag = oracle.gemv(W[e], xs[xi[pos]])
            scale = ws[e].astype(np.float64) * oscale
            want, y = ref * scale, got[pos, j * m:(j + 1) * m].astype(np.float64)
            if exact:
                assert np.array_equal(y, want), (j, e, gref.describe_difference(y, want))
            else:
                tol = GEMV_RTOL_ABS * mag * scale + 2.0 ** -22 * np.abs(want) + 1e-30
                assert (np.abs(y - want) <= tol).all(), (j, e, float((np.abs(y - want) / tol).max()))
    return got, projs, x_dev, tlut, lay, xi, oscale


CODECS = ["tcq_2_none_0.9", "tcq_8_none_0.9", "tcomb_3_4_0.5_none_0.9", "tcomb_6_7_0.5_none_0.9"]
# rows per expert: 1, 8, 9, 16, 17, 33 cross the 8-row table entry and the 16-row MFMA group; 128 are one chunk; an expert without rows
RUNS = ((9, 16, 0, 1), (17, 33, 8, 0), (128, 1, 0, 8), (33, 0, 17, 9))


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("qstr", CODECS)
def test_moe_gemm(qp, oracle, qstr, exact):
    """k of one step (128), a partial last step (160, single-stream codecs), split streams of 1.5 steps each (384) and 17 / 18 steps
    (2112); m of one supertile row and of WAVES + 1; one and two projections (two: a block of rows straddles up | gate); x through
    x_index and in place"""
    big = 32 * (WAVES + 1)
    k1 = 384 if "tcomb" in qstr else 160
    for i, (k, m, nproj, indexed) in enumerate(((128, 32, 1, True), (k1, big, 2, True), (384, 32, 2, False), (2112, big, 1, False))):
        _case(qp, oracle, k, m, qstr, nproj, indexed, exact, 100 * CODECS.index(qstr) + i + 1, RUNS[i])


@pytest.mark.parametrize("qstr", ["tcq_5_none_0.9", "tcomb_3_4_0.5_none_0.9"])
def test_a_row_is_independent_of_its_chunk_and_of_max_run(qp, oracle, qstr):
    """a 33-row run: bitwise the same for max_run 16 (cut in chunks of 16, 16, 1), 64 and 128, and for every row launched alone"""
    counts, k, m = (33, 3, 0, 1), 384, 96
    got, projs, x_dev, tlut, lay, xi, oscale = _case(qp, oracle, k, m, qstr, 2, True, False, 77, counts)
    P, xi_dev = len(xi), _cuda(xi.astype(np.int32))
    for max_run in (16, 64):
        again = _run(qp, projs, x_dev, tlut, _table(lay), xi_dev, P, oscale, 2 * m, max_run)
        assert np.array_equal(again.view(np.uint32), got.view(np.uint32)), max_run
    for pos in range(P):
        g = int(np.searchsorted(lay["group_first"], pos, side="right")) - 1
        one = dict(group_expert=lay["group_expert"][g:g + 1], group_first=np.array([pos]), group_count=np.array([1]), ngroups=1)
        alone = _run(qp, projs, x_dev, tlut, _table(one), xi_dev, P, oscale, 2 * m)
        assert np.array_equal(alone[pos].view(np.uint32), got[pos].view(np.uint32)), pos
        assert (np.delete(alone, pos, axis=0) == SENTINEL).all()


def test_moe_gemm_guards(qp, oracle):
    """test_moe_gemv_guards' entries do no work; a second entry that is not contiguous opens a chunk of its own; an x index outside
    the rows reads zeros; other codecs and max_run outside 1 .. 128 are refused"""
    k, m = 128, 32
    proj, W, ws, tlut = _experts(qp, k, m, "tcq_5_none_0.9", 5, False)
    x = _cuda(np.random.default_rng(0).standard_normal((4, k)).astype(np.float16))
    for ge, gf, gc, ng in (([E4], [0], [2], 1), ([-1], [0], [2], 1), ([0], [6], [2], 1), ([0], [0], [9], 1), ([0], [-1], [1], 1),
                           ([0], [0], [1], 0)):
        t = dict(group_expert=np.array(ge), group_first=np.array(gf), group_count=np.array(gc), ngroups=ng)
        assert (_run(qp, [proj], x, tlut, _table(t), None, 4, 1.0, m) == SENTINEL).all(), (ge, gf, gc, ng)

    def want(e, r):
        return oracle.gemv(W[e], x[r:r + 1].cpu().numpy())[0][0] * ws[e].astype(np.float64)
    t = dict(group_expert=np.array([1, 1]), group_first=np.array([0, 3]), group_count=np.array([2, 1]), ngroups=7)   # ngroups > the table
    out = _run(qp, [proj], x, tlut, _table(t), _cuda(np.array([3, 9, 0, 0], dtype=np.int32)), 4, 1.0, m)
    assert (out[2] == SENTINEL).all() and (out[4:] == SENTINEL).all() and (out[:, m:] == SENTINEL).all()
    assert (out[1, :m] == 0).all()                                                     # an x index outside the rows reads zeros
    assert np.allclose(out[0, :m], want(1, 3), rtol=1e-3, atol=1e-3) and np.allclose(out[3, :m], want(1, 0), rtol=1e-3, atol=1e-3)
    lib, buf = qp._native.lib(), torch.zeros(1 << 12, dtype=torch.int32, device="cuda")
    p, P1 = buf.data_ptr(), qp._native.MoeProj

    def call(proj, S=9, max_run=128):
        return lib.qpal_moe_gemm(p, 64, 4, (P1 * 1)(proj), 1, p, 128, 4, None, p, p, p, p, 1, 4, 128, p, S, 1.0, max_run, None)
    assert call(P1(p, None, None, 32, 5, 0, 0)) == 0
    assert call(P1(p, None, None, 32, 5, 0, 0), S=10) == -2 and call(P1(p, None, None, 32, 9, 0, 0)) == -2
    assert call(P1(p, None, None, 32, 5, 0, 0), max_run=0) == -1 and call(P1(p, None, None, 32, 5, 0, 0), max_run=129) == -1
    torch.cuda.synchronize()
    bad = qp.moe.Projection([buf[:576]], None, None, 32, 128, 9, 0, tlut_bits=10)
    with pytest.raises(qp._native.QpalError, match="moe_gemm.*S = 10, KV = 9"):
        qp.moe.moe_gemm(torch.zeros(4, 32, device="cuda"), [bad], torch.zeros(4, 128, dtype=torch.float16, device="cuda"),
                        torch.zeros(1024, 2, dtype=torch.float16, device="cuda"), buf[:1], buf[:1], buf[:1], buf[:1])


@pytest.mark.parametrize("n", [48, 128])
def test_moemlp_wide_forward(qp, n):
    """MoEMLP(wide=True) on moe_reference.cpu_layer's twin: the routing-decidable rows within the layer tolerance (KAPPA = 4)"""
    E, H, I, top_k = 8, 512, 512, 2
    What, su_ug, su_dp, scale, rw, _ = mref.cpu_layer(E, H, I)
    rng = np.random.default_rng(n)
    h, rms_w = rng.standard_normal((n, H)).astype(np.float32), (1 + 0.3 * rng.standard_normal(H)).astype(np.float16)
    rt = qp.moe.reference_route(h, rms_w, mref.EPS, rw, None, top_k, True)
    ok = mref.decidable_rows(rt, mref.logit_bounds(rt, rw), top_k)
    assert (~ok).sum() <= mref.UNDECIDABLE_CAP * n                  # (the reference alone, on the CPU)
    experts, router, _, _ = _layer(qp, E=E, H=H, I=I, seed=100)
    assert np.array_equal(router.cpu().numpy(), rw)
    layer = qp.MoEMLP.from_experts(router, experts, top_k, renorm=True, wide=True)
    assert layer.launches(n) == 6
    got = layer(_cuda(h), (mref.EPS, _cuda(rms_w))).cpu().numpy().astype(np.float64)
    f, rows = mref.layer_judge(What, su_ug, su_dp, scale, rt, ok, got)
    print(f"MoEMLP(wide=True) n = {n}: max distance / tolerance {f.max():.3f}")
    assert (f <= 1.0).all(), rows[f > 1.0].tolist()


def test_steps_with_wide_sparse_layers(qp, monkeypatch):
    """the small sparse model with wide=True: one Prefill and DecodeStep at B = 4 judged as tests/test_moe_model.py judges them;
    the captured B = 4 step replays bit for bit what the eager step computes"""
    dev, mm = torch.device("cuda", 0), _world()
    for l in mm.layers:
        if isinstance(l.mlp, qp.MoEMLP):
            monkeypatch.setattr(l.mlp, "wide", True)   # (the model is shared with tests/test_moe_model.py: restored at teardown)
    toks, ref, emu, ok = _model_refs(mm, "prefill")
    _, kc, vc, _ = _caches(mm, "fp16", dev, 3)
    pf = qp.Prefill(mm.layers, mm.embed, mm.norm, mm.lm_head, kc, vc, mm.inv_freq, chunk=16, sampler=qp.Sampler(3, mr.VOCAB, dev, temperature=0.0))
    hs, ls, ts = [], [], []
    for b, t in enumerate(toks):
        ts.append(pf(t.to(dev), slot=b, pos0=0).clone()[0])
        hs.append(pf.last32[0].clone())
        ls.append(pf.sampler.logits[b].clone())
    keep = [b for b, t in enumerate(toks) if ok[(b, len(t) - 1)]]
    _judge("Prefill sparse wide", [(b, len(toks[b]) - 1) for b in keep], ref, emu, torch.stack(hs)[keep].cpu(), torch.stack(ls)[keep].cpu(),
           torch.stack(ts)[keep].cpu())
    toks, ref, emu, ok = _model_refs(mm, "decode")
    plan = _forced(toks)
    _, kc, vc, ckw = _caches(mm, "fp16", dev, 4)
    run = _Decode(mm, dev, 4, kc, vc, **ckw)
    run.run(plan)
    picks = [(s, b) for s, row in enumerate(plan) for b, r in enumerate(row) if r is not None and ok[(b, s)]]
    _judge("DecodeStep B=4 sparse wide", [(b, s) for s, b in picks], ref, emu, torch.stack([run.h[s][b] for s, b in picks]).cpu(),
           torch.stack([run.l[s][b] for s, b in picks]).cpu(), torch.stack([run.t[s][b] for s, b in picks]).cpu(), cap=0.10)
    _reproducible_projections(monkeypatch)   # (the dense projections without float atomics; the routed launches have none)
    hs = []
    for graphed in (False, True):
        _, kc, vc, ckw = _caches(mm, "fp16", dev, 4)
        run = _Decode(mm, dev, 4, kc, vc, **ckw)
        if graphed:
            run.run(plan[:1])
            run.h.clear()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                run.step()
            step, run.step = run.step, lambda: graph.replay()   # (`step` keeps the buffers the graph names alive)
            run.step.h32 = step.h32
        run.run(plan)
        hs.append(torch.stack(run.h))
    assert torch.equal(hs[0], hs[1])
