"""Draft trees on the GPU: the tree-masked ragged launch, qpal_kv_compact, qpal_spec_tree_draft / _accept against
their numpy contracts, and SpeculativeStep(tree=7) against the sequential stream under tests/test_spec.py's near-tie rule."""
import math

import numpy as np
import pytest
import torch

import attn_reference as ar
import qpalette_amd as qp
import test_spec as ts
from attn_reference import F8, F16
from qpalette_amd import speculative as sp
from test_attn_exact import _rotated_q
from test_spec import dev, model, prompts  # noqa: F401  (fixtures)

L, PAGE = 1024, 16
CHAIN = list(range(-1, 8))                       # parent of row t (row 0: none): 9 rows
STAR = [-1] + [0] * 31                           # 31 children of the root
BINARY = [-1] + [(t - 1) // 2 for t in range(1, 32)]  # 32 rows: crosses a 16-row tile
MIXED = [-1, 0, 0, 1, 1, 3, 2, 5]                # tests/test_spec_tree_contract.py's tree


def _depth_anc(par):
    depth, anc = [0] * len(par), [1] * len(par)
    for t in range(1, len(par)):
        depth[t], anc[t] = depth[par[t]] + 1, anc[par[t]] | (1 << t)
    return depth, anc


def _i32(bits):
    return torch.tensor(np.array(bits, dtype=np.uint32).view(np.int32))


class Caches:
    """B sequences' K and V caches, random everywhere, contiguous or behind a shuffled block table; rows() gathers [B, nkv, L, hd]"""

    def __init__(self, dev, B, nkv, hd, dtype, paged, seed, table=None):
        g = torch.Generator().manual_seed(seed)
        mk = lambda: (0.5 * torch.randn(B, nkv, L, hd, generator=g)).to(dev).to(dtype)
        self.paged, self.B, self.nkv, self.hd = paged, B, nkv, hd
        self.k, self.v = mk(), mk()
        if paged:
            self.table = torch.randperm(B * (L // PAGE), generator=g).to(torch.int32).view(B, L // PAGE).to(dev) if table is None else table
            self.k, self.v = self._scatter(self.k), self._scatter(self.v)

    def _scatter(self, c):
        pool = torch.empty(self.B * (L // PAGE), self.nkv, PAGE, self.hd, dtype=c.dtype, device=c.device)
        pool.view(torch.uint8)[self.table.view(-1).long()] = \
            c.view(self.B, self.nkv, L // PAGE, PAGE, self.hd).permute(0, 2, 1, 3, 4).reshape(pool.shape).view(torch.uint8)
        return pool

    def rows(self, c):
        if not self.paged:
            return c.clone()
        g = c.view(torch.uint8)[self.table.view(-1).long()].view(self.B, L // PAGE, self.nkv, PAGE, -1)
        return g.permute(0, 2, 1, 3, 4).reshape(self.B, self.nkv, L, -1).view(c.dtype)

    def attend(self, q, k, v, seq, row0, pos0, inv, ws, tree=None):
        if self.paged:
            return qp.paged_ragged_prefill_attention(q, k, v, self.k, self.v, self.table, seq, row0, pos0, inv, ws=ws, tree=tree,
                                                     out=torch.full((q.shape[0], q.shape[1]), 7.0, dtype=F16, device=q.device))
        return qp.ragged_prefill_attention(q, k, v, self.k, self.v, seq, row0, pos0, inv, ws=ws, tree=tree,
                                           out=torch.full((q.shape[0], q.shape[1]), 7.0, dtype=F16, device=q.device))


# (name, [(sequence, parents)], inactive: a segment of 33 rows and one with a bad sequence)
TREES = [("chain", [(0, CHAIN)]), ("star", [(1, STAR)]), ("binary", [(2, BINARY)]),
         ("mixed", [(0, MIXED), (9, CHAIN[:4]), (2, BINARY[:12]), (3, [-1] * 33), (1, [-1])])]


@pytest.mark.gpu
@pytest.mark.parametrize("pos0", [0, 37, 600])
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged16"])
@pytest.mark.parametrize("dtype", [F16, F8], ids=["fp16", "e4m3"])
@pytest.mark.parametrize("shape", [(8, 2, 128), (4, 4, 64), (4, 2, 256)], ids=str)  # hd 256: the instantiations nearest the SGPR limit
def test_tree_attention(dev, shape, dtype, paged, pos0):
    """pos0 37 puts a segment's keys across a 32-key tile edge, 600 takes the split path (max_len 1024).  Per tree: the chain is
    bitwise the ragged launch; every row within attn_reference's bound of the float64 softmax over the cache below pos0 and the
    row's root path; every stored row bitwise the one-sequence launch's at position pos0 + depth; inactive segments untouched."""
    nq, nkv, hd = shape
    B, scale, inv = 4, 1.0 / math.sqrt(hd), ar.inv_freq(hd, dev)
    one_k = torch.zeros(nkv, L, hd, dtype=torch.uint8 if dtype == F8 else F16, device=dev).view(dtype)  # the one-sequence launch's caches
    one_v = torch.zeros_like(one_k)
    one_ws = qp.prefill_workspace(1, nq, nkv, hd, L, dev)
    for name, segs in TREES:
        S, R = len(segs), sum(len(p) for _, p in segs)
        g = torch.Generator().manual_seed(len(name) + pos0)
        q, k, v = torch.randn(R, (nq + 2 * nkv) * hd, generator=g).to(dev).split([nq * hd, nkv * hd, nkv * hd], dim=1)  # one row stride
        seq = torch.tensor([b for b, _ in segs], dtype=torch.int32, device=dev)
        row0 = torch.tensor(np.cumsum([0] + [len(p) for _, p in segs]), dtype=torch.int32, device=dev)
        p0 = [pos0 + 3 * s for s in range(S)]
        pos_t = torch.tensor(p0, dtype=torch.long, device=dev)
        da = [_depth_anc(p) if len(p) <= 32 else ([0] * 33, [1] * 33) for _, p in segs]
        depth = torch.tensor(sum((d for d, _ in da), []), dtype=torch.int32, device=dev)
        anc = _i32(sum((a for _, a in da), [])).to(dev)
        ws = qp.ragged_workspace(R, S, nq, nkv, hd, L, dev)
        c = Caches(dev, B, nkv, hd, dtype, paged, seed=pos0 + 1)
        k0, v0 = c.rows(c.k), c.rows(c.v)
        out = c.attend(q, k, v, seq, row0, pos_t, inv, ws, tree=(depth, anc))
        k1, v1 = c.rows(c.k), c.rows(c.v)
        if name == "chain":
            c2 = Caches(dev, B, nkv, hd, dtype, paged, seed=pos0 + 1)
            out2 = c2.attend(q, k, v, seq, row0, pos_t, inv, ws)
            assert torch.equal(out, out2) and torch.equal(c.k.view(torch.uint8), c2.k.view(torch.uint8)) \
                and torch.equal(c.v.view(torch.uint8), c2.v.view(torch.uint8))
        worst, r = 0.0, 0
        for s, (b, par) in enumerate(segs):
            T = len(par)
            if T > 32 or not 0 <= b < B:  # inactive: out rows and cache bytes keep what they held
                assert bool((out[r:r + T] == 7.0).all()), (name, s)
                r += T
                continue
            d, a = da[s]
            q16 = _rotated_q(q[r:r + T], [p0[s] + x for x in d], shape, dev)  # by qpal_rope_kv, at the rows' POSITIONS
            for t in range(T):
                idx = torch.tensor(list(range(p0[s])) + [p0[s] + j for j in range(T) if (a[t] >> j) & 1], device=dev)
                ref, A, Smax = ar.attention_fp64(q16[t:t + 1], k1[b][:, idx], v1[b][:, idx], [idx.numel()], nq, nkv, hd, scale)
                ratio = (out[r + t:r + t + 1].double() - ref).abs() / ar.bound(ref, A, Smax, 2.0 ** -11)
                worst = max(worst, float(torch.nan_to_num(ratio, nan=float("inf")).max()))
                # the stored row: the one-sequence launch of this k / v row alone at position pos0 + depth
                at = torch.tensor([p0[s] + d[t]], dtype=torch.long, device=dev)
                qp.prefill_attention(q[r + t:r + t + 1], k[r + t:r + t + 1], v[r + t:r + t + 1], one_k, one_v, at, inv, ws=one_ws)
                for got, want in ((k1, one_k), (v1, one_v)):
                    assert torch.equal(got[b][:, p0[s] + t].view(torch.uint8), want[:, p0[s] + d[t]].view(torch.uint8)), (name, s, t)
            k0[b][:, p0[s]:p0[s] + T] = k1[b][:, p0[s]:p0[s] + T]  # the only rows that may differ from before
            v0[b][:, p0[s]:p0[s] + T] = v1[b][:, p0[s]:p0[s] + T]
            r += T
        print(f"tree attention {shape} {dtype} paged={paged} pos0={pos0} {name}: worst err / bound = {worst:.3f}")
        assert worst <= 1.0, (name, worst)
        assert torch.equal(k0.view(torch.uint8), k1.view(torch.uint8)) and torch.equal(v0.view(torch.uint8), v1.view(torch.uint8)), name


@pytest.mark.gpu
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged16"])
@pytest.mark.parametrize("dtype", [F16, F8], ids=["fp16", "e4m3"])
def test_kv_compact_is_a_gather(dev, dtype, paged):
    """two layers, four slots: path (0, 2, 3, 5) whose destinations are other moves' sources, the identity, n_acc = 0, and a
    path to the last rows of a tree; bitwise a numpy gather on the rows before the launch, every other byte unchanged"""
    B, nkv, hd = 4, 2, 64
    layers = [Caches(dev, B, nkv, hd, dtype, paged, seed=50)]
    table = layers[0].table if paged else None
    layers.append(Caches(dev, B, nkv, hd, dtype, paged, seed=51, table=table))  # one block table for the step's layers
    paths = [[0, 2, 3, 5], [0, 1, 2, 3], [0, 9, 11], [0, 4, 17, 30, 31]]
    n_acc = [3, 3, 0, 4]
    pos0 = [37, 0, 600, L - 32]
    path = torch.full((B, 16), -1, dtype=torch.int32)
    for b, p in enumerate(paths):
        path[b, :len(p)] = torch.tensor(p, dtype=torch.int32)
    before = [(c.rows(c.k).view(torch.uint8).cpu().numpy(), c.rows(c.v).view(torch.uint8).cpu().numpy()) for c in layers]
    qp.kv_compact(qp.kv_pointer_table([c.k for c in layers]), qp.kv_pointer_table([c.v for c in layers]), layers[0].k,
                  torch.tensor(pos0, dtype=torch.long, device=dev), path.to(dev), torch.tensor(n_acc, dtype=torch.int32, device=dev),
                  block_table=table)
    for c, (bk, bv) in zip(layers, before):
        for got, want in ((c.rows(c.k), bk.copy()), (c.rows(c.v), bv.copy())):
            src = want.copy()
            for b in range(B):
                for kk in range(1, n_acc[b] + 1):
                    want[b, :, pos0[b] + kk] = src[b, :, pos0[b] + paths[b][kk]]
            assert np.array_equal(got.view(torch.uint8).cpu().numpy(), want)
    assert not np.array_equal(before[0][0], layers[0].rows(layers[0].k).view(torch.uint8).cpu().numpy())


def _trees(rng, B, N):
    """random trees in the caller's format with some invalid parents and tokens, so that lists end early"""
    tok = rng.integers(0, 5, size=(B, max(N, 1))).astype(np.int32)[:, :N]
    par = np.array([[rng.integers(0, i + 1) for i in range(N)] for _ in range(B)], dtype=np.int32).reshape(B, N)
    bad = rng.random((B, N)) < 0.03
    par[bad] = np.arange(1, N + 1)[None, :].repeat(B, 0)[bad]  # a node that names itself
    tok[rng.random((B, N)) < 0.02] = -1
    return tok, par, rng.integers(0, N + 3, size=B).astype(np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("full", [False, True], ids=["R=B", "R=128"])
@pytest.mark.parametrize("N", [0, 7, 31])
@pytest.mark.parametrize("B", [1, 5, 128])
def test_tree_draft_and_accept_are_the_references(dev, B, N, full):
    """tests/test_spec.py's state (histories up to 5000 tokens, slots at their limit, at max_len, never begun): the caller's trees
    and the lookup chain, then the accept on draws that mostly follow a child; every output bit for bit the numpy contract"""
    R = 128 if full else B
    rng = np.random.default_rng(1000 * B + 10 * N + full)
    hist, n_tok, limit = ts._state(B, seed=B + N)
    if B == 128:
        n_tok[rng.random(B) < 0.8] = 0  # room for trees in the 128 rows
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt).to(dev).contiguous()
    for ext in (_trees(rng, B, N), None):
        kw = {} if ext is None else dict(ext_tok=ext[0], ext_par=ext[1], ext_n=ext[2])
        ref = sp.reference_spec_tree_draft(hist, n_tok, limit, N, 1, 4, R, ts.MAX_LEN, **kw)
        sizes = {"R": R, "B": B, "B1": B + 1}
        out = {name: torch.full((sizes[n],), -77, dtype=dt, device=dev) for name, dt, n in ts.DRAFT_OUT}
        out.update(depth=torch.full((R,), -77, dtype=torch.int32, device=dev), anc=torch.full((R,), -77, dtype=torch.int32, device=dev))
        qp.spec_tree_draft(t(hist, torch.int32), t(n_tok, torch.int64), t(limit, torch.int64), N, (1, 4), ts.MAX_LEN, **out,
                           **{k: t(v, torch.int32) for k, v in kw.items()})
        got = {k: v.cpu().numpy() for k, v in out.items()}
        got["anc"] = got["anc"].view(np.uint32)
        ts._same(got, ref, (B, N, R, ext is None))
        # the accept: row r's draw mostly equals the token of one of its children
        drawn = rng.integers(0, 5, size=R)
        for r in range(R):
            kids = [j for j in range(r + 1, R) if ref["row_slot"][j] == ref["row_slot"][r] >= 0 and ref["depth"][j] == ref["depth"][r] + 1
                    and (int(ref["anc"][j]) >> (r - ref["row0"][ref["row_slot"][r]])) & 1]
            if kids and rng.random() < 0.8:
                drawn[r] = ref["tokens"][kids[int(rng.integers(len(kids)))]]
        ld = hist.shape[1]
        lim2 = n_tok + rng.integers(0, 12, size=B)
        eos = np.where(rng.random(B) < 0.5, rng.integers(0, 5, size=B), -1)
        out0 = np.full((B, 16), -9, np.int64)
        aref = sp.reference_spec_tree_accept(ref["tokens"], drawn, ref["seq"], ref["row0"], ref["depth"], ref["anc"], hist, n_tok, lim2, eos,
                                             out_tok=out0)
        st = dict(hist=t(hist, torch.int32), n_tok=t(n_tok, torch.int64), limit=t(lim2, torch.int64))
        ao = dict(out_tok=t(out0, torch.int64), n_out=t(np.full(B, -9), torch.int32), n_acc=t(np.full(B, -9), torch.int32),
                  path=t(np.full((B, 16), -9), torch.int32))
        qp.spec_tree_accept(t(ref["tokens"], torch.int64), t(drawn, torch.int64), out["seq"], out["row0"], out["depth"], out["anc"],
                            eos=t(eos, torch.int64), **st, **ao)
        ts._same({k: v.cpu().numpy() for k, v in {**st, **ao}.items()}, aref, (B, N, R, "accept", ld))
        if ext is not None and N == 31 and B == 5 and full:
            assert int(ref["depth"].max()) >= 3 and int(aref["n_acc"].max()) >= 2, "the trees show too little"


# -------------------------------------------------------------------------------------------------------- whole model

TREE, WIDTH, DEPTH = 7, 2, 3  # 7 nodes offered to a step built for 7: three levels of two siblings, one node unused


def _tree_step(m, dev, prompts, dtype, paged, mode):
    """tests/test_spec.py's _spec_step with tree=TREE: fresh caches, prompts[b][:-1] prefilled into slot b"""
    nkv, hd, nl = m.cfg.num_key_value_heads, m.cfg.head_dim, len(m.layers)
    table = None
    if paged:
        cache = qp.PagedKVCache(nl, 2 * ts.NB * (ts.L // ts.PS), nkv, ts.PS, hd, ts.NB, ts.L // ts.PS, dtype=dtype, device=dev)
        for n in (64, 128):  # 128 >= every limit + TREE + 1
            for slot in range(ts.NB):
                cache.reserve(slot, n)
        kr, vr, table = cache.kpool, cache.vpool, cache.table
    else:
        kr, vr = ts._caches(m, dev, dtype)
    pf = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kr, vr, m.inv_freq, chunk=128, block_table=table)
    smp = qp.Sampler(ts.NB, ts.VOCAB, dev, **ts.MIXED) if mode == "mixed" else None
    ss = qp.SpeculativeStep(m.layers, m.embed, m.norm, m.lm_head, kr, vr, m.inv_freq, sampler=smp, block_table=table, tree=TREE)
    assert ss.rows == ts.NB * (TREE + 1) and ss.out_tok.shape == (ts.NB, 16)
    for b, p in enumerate(prompts):
        pf(p[:-1], slot=b, pos0=0)
        ss.begin(b, p.tolist(), limit=p.shape[0] + ts.NEW)
    return ss


def _offer(want, done, right):
    """per slot a tree of DEPTH levels of WIDTH siblings under the previous level's sibling `right` (None: the first, and no sibling
    carries the yardstick's token); sibling `right` carries the yardstick's next token of its level"""
    tok, par = torch.zeros(ts.NB, TREE, dtype=torch.int32), torch.zeros(ts.NB, TREE, dtype=torch.int32)
    for b in range(ts.NB):
        up = 0
        for l in range(DEPTH):
            nxt = want[b][done[b] + l] if done[b] + l < ts.NEW else 0
            for w in range(WIDTH):
                tok[b, l * WIDTH + w] = nxt if w == right else (nxt + 1 + w) % ts.VOCAB
                par[b, l * WIDTH + w] = up
            up = l * WIDTH + 1 + (right or 0)
    return tok, par


@pytest.mark.gpu
@pytest.mark.parametrize("right", [0, 1, None], ids=["first-sibling", "second-sibling", "absent"])
@pytest.mark.parametrize("kind, mode, graph", [("fp16", "greedy", False), ("fp16", "mixed", False), ("paged-fp8", "greedy", False),
                                               ("paged-fp8", "mixed", False), ("fp16", "mixed", True)],
                         ids=["fp16-greedy", "fp16-mixed", "paged-fp8-greedy", "paged-fp8-mixed", "fp16-mixed-graph"])
def test_tree_step_emits_the_sequential_stream(dev, model, prompts, kind, mode, graph, right):
    """tests/test_spec.py's model, prompts, seeds, yardstick and near-tie rule (_judge: a first difference is excused only inside
    twice §13's bound, at most 5 % of the tokens behind an excuse).  Before any excuse, a step whose trees carry the sequential
    token accepts the whole depth the slot's limit leaves — on the second sibling too, where a chain would accept nothing."""
    dtype, paged = (F8, True) if kind == "paged-fp8" else (F16, False)
    want, logits, _ = ts._yardstick(dev, model, prompts, dtype, mode)
    ss = _tree_step(model, dev, prompts, dtype, paged, mode)
    ext_tok, ext_par = (x.to(dev) for x in _offer(want, [0] * ts.NB, right))
    ext_n = torch.full((ts.NB,), DEPTH * WIDTH, dtype=torch.int32, device=dev)
    step = lambda: ss(ext_tok=ext_tok, ext_par=ext_par, ext_n=ext_n)
    if graph:
        state = (ss.n_tok.clone(), ss.hist.clone())
        stream = torch.cuda.Stream(dev)
        with torch.cuda.stream(stream):
            ss.n_tok.zero_()  # the warm-up runs on a state without sequences: no row, no cache byte, no token
            step()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream):
                step()
        torch.cuda.synchronize()
        ss.n_tok.copy_(state[0])
        ss.hist.copy_(state[1])
        step = g.replay
    got, records = [[] for _ in range(ts.NB)], []
    for _ in range(ts.NEW + 1):
        if not bool((ss.n_tok < ss.limit).any()):
            break
        tok, par = _offer(want, [len(x) for x in got], right)
        ext_tok.copy_(tok)
        ext_par.copy_(par)
        step()
        torch.cuda.synchronize()
        out, n_out, n_acc, n_draft = ss.out_tok.cpu(), ss.n_out.cpu(), ss.n_acc.cpu(), ss.n_draft.cpu()
        rec = {}
        for b in range(ts.NB):
            if int(n_out[b]):
                rec[b] = (len(got[b]), int(n_draft[b]), int(n_acc[b]), int(n_out[b]))
                got[b] += out[b, :int(n_out[b])].tolist()
        records.append(rec)
    assert not bool((ss.n_tok < ss.limit).any()), "a slot did not reach its limit"
    params = ts.MIXED if mode == "mixed" else ts.GREEDY
    ts._judge(got, records, want, logits, prompts, params, "a")
    # per slot, up to its first (excused) difference: behind it the offered trees no longer follow the slot's stream
    upto = [next((i for i in range(ts.NEW) if got[b][i] != want[b][i]), ts.NEW) for b in range(ts.NB)]
    for rec in records:
        for b, (done, n_draft, n_acc, n_out) in rec.items():
            if done + n_out <= upto[b]:
                levels = min(DEPTH, ts.NEW - done - 1)
                assert n_draft == WIDTH * levels, (b, done, n_draft)
                assert n_acc == (0 if right is None else levels) and n_out == n_acc + 1, (b, done, n_acc, n_out)
    print(f"{kind} {mode} graph={graph} right={right}: {len(records)} steps for {ts.NEW} tokens per slot, checked up to {upto}")
    for b, p in enumerate(prompts):
        n = p.shape[0]
        assert int(ss.n_tok[b]) == n + ts.NEW and ss.hist[b, :n + ts.NEW].tolist() == p.tolist() + got[b]
