"""Shared-prefix decode attention on the GPU: shared_prefix_decode_attention against paged_decode_attention (bit for
bit wherever the contract says so), the census, the float64 reference with the bound of attn_reference.py at u_p = 2^-11 (the prefix
phase rounds its softmax weights to fp16 in front of the value product, as the prefill kernels do; the suffix phase keeps fp32), the
independence of a row from its group's other rows, and a captured whole-model step on a forked cache."""
import math
import os
import sys

import pytest
import torch

import qpalette_amd as qp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_reference as ar  # noqa: E402

F16, F8 = ar.F16, ar.F8
DTYPES = [F16, F8]
SHAPES = [(8, 2, 128), (4, 4, 64), (8, 1, 64), (4, 1, 256)]  # nq, nkv, hd
PAGES = [16, 64]
U_PREFIX = 2.0 ** -11
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _bits(t):
    return t.view(torch.uint8) if t.dtype == F8 else t.view(torch.int16)


def _qkv(q, k, v):
    """q | k | v as column slices of one buffer: the launches take rows with a common stride"""
    return torch.cat((q, k, v), dim=1).split([q.shape[1], k.shape[1], v.shape[1]], dim=1)


class Forked:
    """B slots' caches [B, nkv, L, hd] behind a block table in which the members of every group (members, length) share the pages
    of their first `length` positions (the first member's content); every other page is a slot's own, in a seeded random order"""

    def __init__(self, kc, vc, ps, groups, seed):
        B, nkv, L, hd = kc.shape
        self.B, self.ps, self.mp, self.groups = B, ps, L // ps, groups
        self.num_pages = B * self.mp + 3
        perm = torch.randperm(self.num_pages, generator=torch.Generator().manual_seed(seed))
        table = perm[:B * self.mp].view(B, self.mp).clone()
        for members, length in groups:
            for m in members[1:]:
                table[m, :length // ps] = table[members[0], :length // ps]
        self.table = table.to(torch.int32).to(kc.device)
        self.pools = []
        for c in (kc, vc):
            pool = torch.zeros((self.num_pages, nkv, ps, hd), dtype=torch.uint8 if c.dtype == F8 else F16, device=c.device).view(c.dtype)
            pages = _bits(c).view(B, nkv, self.mp, ps, hd).transpose(1, 2)
            for b in reversed(range(B)):  # (the first member of a group is the lowest: its content stays)
                _bits(pool)[self.table[b].long()] = pages[b]
            self.pools.append(pool)

    def clone_pools(self):
        return [p.clone() for p in self.pools]

    def gather(self, pool):
        """the pool read through the table: [B, nkv, L, hd] in the pool's dtype"""
        g = _bits(pool)[self.table.long()]  # [B, mp, nkv, ps, hd]
        return g.transpose(1, 2).reshape(self.B, g.shape[2], self.mp * self.ps, g.shape[4]).contiguous().view(pool.dtype)

    def prefix(self, G=None, row_group=None):
        """the SharedPrefix of the groups (first member as grp_slot), padded to G groups of length 0"""
        G = len(self.groups) if G is None else G
        rg, gs, gl = [-1] * self.B, [-1] * G, [0] * G
        for g, (members, length) in enumerate(self.groups):
            gs[g], gl[g] = members[0], length
            for m in members:
                rg[m] = g
        if row_group is not None:
            rg = row_group
        d = self.table.device
        mk = lambda x: torch.tensor(x, dtype=torch.int32, device=d)  # noqa: E731
        return qp.SharedPrefix(mk(rg), mk(gs), mk(gl))


def _random_problem(dev, shape, L, ps, dtype, groups, pos, seed):
    """random caches whose group members share their prefix, the table, the new rows and the two workspaces"""
    nq, nkv, hd = shape
    B = len(pos)
    gen = torch.Generator(device=dev).manual_seed(seed)
    kc, vc = (0.5 * torch.randn(B, nkv, L, hd, device=dev, generator=gen) for _ in range(2))
    for members, length in groups:
        for m in members[1:]:
            kc[m, :, :length], vc[m, :, :length] = kc[members[0], :, :length], vc[members[0], :, :length]
    fk = Forked(ar.to_cache(kc, dtype), ar.to_cache(vc, dtype), ps, groups, seed)
    q, k, v = _qkv(torch.randn(B, nq * hd, device=dev, generator=gen), torch.randn(B, nkv * hd, device=dev, generator=gen),
                   torch.randn(B, nkv * hd, device=dev, generator=gen))
    return fk, (q, k, v), torch.tensor(pos, dtype=torch.long, device=dev)


def _tickets_are_zero(ws, B, G, shape, L):
    """the plain launch's ticket words and the prefix phase's (behind the plain workspace: [nkv][ceil(B rep / 64) + min(G, B)])"""
    nq, nkv, hd = shape
    w = ws.view(torch.int32)
    plain = qp._native.lib().qpal_attn_batch_ws_bytes(B, nq, nkv, hd, L) // 4
    ntile = (B * (nq // nkv) + 63) // 64 + min(G, B)
    ok = int(w[plain:plain + nkv * ntile].abs().max()) == 0
    return ok and (plain == 0 or int(w[:128 * nkv].abs().max()) == 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "fp8"])
@pytest.mark.parametrize("ps", PAGES)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_ordinary_slots_and_appended_rows_are_the_plain_launch(dev, shape, ps, dtype):
    """L = 1024 (the suffix launch splits).  Groups {0, 2, 3} (3 pages) and {4, 5} (1 page); slot 1 ungrouped; guarded out: slot 6
    (its group's length lies above its position), 7 (group id out of range), 8 (its group's grp_slot is out of range), 9 (length
    no page multiple), 10 (length 0), 11 (inactive, in group 0).  (a) row_group all -1: out and both pools are bit for bit
    paged_decode_attention's.  (b) with the groups: the ordinary rows' out and BOTH WHOLE pools (so every appended row, the
    members' too) are bit for bit the plain launch's; the members' out differs from it by less than the float64 bound allows twice
    over (they are checked properly below).  (c) slot 0 in group {0, 2, 3} equals bit for bit slot 0 in group {0, 3}; two runs of
    one launch are bitwise equal; every ticket is zero afterwards."""
    nq, nkv, hd = shape
    L, B, G = 1024, 12, 5
    groups = [([0, 2, 3], 3 * ps), ([4, 5], ps)]
    pos = [3 * ps + 600, 700, 3 * ps, 3 * ps + 17, ps + 1, ps + 520, 3 * ps - 1, 40, 300, 511, 512, -1]
    fk, qkv, pos_t = _random_problem(dev, shape, L, ps, dtype, groups, pos, seed=11)
    inv = ar.inv_freq(hd, dev)
    ws_plain = qp.attention_workspace(B, nq, nkv, hd, L, dev)
    ws = qp.shared_prefix_workspace(B, G, nq, nkv, hd, L, dev)
    rg = [0, -1, 0, 0, 1, 1, 0, 7, 2, 3, 4, 0]
    px = fk.prefix(G, rg)
    px.grp_slot[2:] = torch.tensor([B, 9, 10], dtype=torch.int32)
    px.grp_len[2:] = torch.tensor([ps, ps + 4, 0], dtype=torch.int32)
    members, length = ar_members(px, pos, ps, L)
    assert members == [0, 2, 3, 4, 5] and length[0] == 3 * ps and length[4] == ps

    def run(fn, *extra, **kw):
        kp, vp = fk.clone_pools()
        out = torch.full((B, nq * hd), 3.0, dtype=F16, device=dev)
        fn(*qkv, kp, vp, fk.table, pos_t, inv, *extra, out=out, **kw)
        torch.cuda.synchronize()
        return out, kp, vp

    ref, rk, rv = run(qp.paged_decode_attention, ws=ws_plain)
    none = qp.SharedPrefix(torch.full_like(px.row_group, -1), px.grp_slot, px.grp_len)
    out, kp, vp = run(qp.shared_prefix_decode_attention, none, ws=ws)
    assert torch.equal(_bits(out), _bits(ref)) and torch.equal(_bits(kp), _bits(rk)) and torch.equal(_bits(vp), _bits(rv))
    out, kp, vp = run(qp.shared_prefix_decode_attention, px, ws=ws)
    ordinary = [b for b in range(B) if b not in members]
    assert torch.equal(_bits(out[ordinary]), _bits(ref[ordinary]))
    assert torch.equal(_bits(kp), _bits(rk)) and torch.equal(_bits(vp), _bits(rv))
    assert bool((out[11] == 3.0).all())
    diff = float((out[members].float() - ref[members].float()).abs().max())
    print(f"{shape} page {ps} {dtype}: members' max |shared - plain| = {diff:.3e}")
    # both lie within bound() of one float64 result: |shared - plain| <= 2 (2^-11 |ref| + 2^-24 + kappa (2^-11 + ...) A) with kappa = 8
    # and |ref|, A <= max |v| < 3 for 0.5 N(0, 1) values: < 2 (0.0015 + 0.0118) < 2^-5
    assert diff < 2.0 ** -5
    again, _, _ = run(qp.shared_prefix_decode_attention, px, ws=ws)
    assert torch.equal(_bits(again), _bits(out))
    rg2 = list(rg)
    rg2[2] = -1
    out2, _, _ = run(qp.shared_prefix_decode_attention, fk.prefix(G, rg2), ws=ws)
    assert torch.equal(_bits(out2[0]), _bits(out[0])) and torch.equal(_bits(out2[3]), _bits(out[3]))
    assert torch.equal(_bits(out2[2]), _bits(ref[2]))
    assert _tickets_are_zero(ws, B, G, shape, L)


def ar_members(px, pos, ps, L):
    """the members of a launch by reference_shared_rows: ([slots], {slot: length})"""
    g, n = qp.reference_shared_rows(px.row_group.cpu().numpy(), px.grp_slot.cpu().numpy(), px.grp_len.cpu().numpy(), pos, ps, L)
    return [b for b in range(len(pos)) if g[b] >= 0], {b: int(n[b]) for b in range(len(pos)) if g[b] >= 0}


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "fp8"])
@pytest.mark.parametrize("ps", PAGES)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_census_every_member_counts_pos_plus_one_keys(dev, shape, ps, dtype):
    """K = 0, V[j] = e_{j mod hd}: out counts keys.  B = 17 slots (136 rows at rep 8: group 0 alone has 72, more than one 64-row
    tile of the prefix kernel): group 0 = slots 0 .. 8 (1 page), group 1 = slots 9 .. 14 (3 pages), slot 15 ungrouped, slot 16
    inactive inside group 0; suffixes of 0 (pos == grp_len), 1, 17 and 600 cached positions (max_len 1024: the suffix splits)."""
    nq, nkv, hd = shape
    L, B = 1024, 17
    groups = [(list(range(0, 9)) + [16], ps), (list(range(9, 15)), 3 * ps)]
    suffix = [0, 1, 17, 600]
    pos = [ps + suffix[b % 4] for b in range(9)] + [3 * ps + suffix[b % 4] for b in range(6)] + [333, -1]
    K1, V1 = ar.census_cache(nkv, L, hd, dtype, dev)
    stack = lambda c: torch.stack([c.view(torch.uint8)] * B).view(c.dtype)  # noqa: E731
    fk = Forked(stack(K1), stack(V1), ps, groups, seed=3)
    pos_t = torch.tensor(pos, dtype=torch.long, device=dev)
    kp, vp = fk.clone_pools()
    act = pos_t >= 0
    for b in range(B - 1):  # NaN into the rows this launch writes (a member's lie in its own pages: pos >= grp_len)
        page, off = int(fk.table[b, pos[b] // ps]), pos[b] % ps
        ar.nan_rows(kp[page], slice(off, off + 1))
        ar.nan_rows(vp[page], slice(off, off + 1))
    q = ar.query_targets(B, nq, nkv, hd, 3, dev)
    k = torch.zeros(B, nkv * hd, device=dev)
    out = torch.full((B, nq * hd), float("nan"), dtype=F16, device=dev)
    px = fk.prefix()
    members, _ = ar_members(px, pos, ps, L)
    assert members == list(range(15))
    qp.shared_prefix_decode_attention(*_qkv(q, k, ar.census_new_v(pos_t, nkv, hd, dev)), kp, vp, fk.table, pos_t, ar.inv_freq(hd, dev), px,
                                      out=out, ws=qp.shared_prefix_workspace(B, px.G, nq, nkv, hd, L, dev))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[16]).all())
    exp, tol = ar.census_expected([p + 1 for p in pos[:16]], nq, hd, dev)
    r = torch.nan_to_num((out[act].double() - exp).abs() / tol, nan=float("inf"))
    print(f"shared_prefix census {shape} page {ps} {dtype}: worst err/tol = {float(r.max()):.3f}")
    assert float(r.max()) <= 1.0, r.amax(dim=1)
    assert torch.equal(_bits(fk.gather(vp)), _bits(stack(V1))) and not bool((fk.gather(kp).view(torch.uint8) & 0x7F).any())


def _rotated_q(q32, pos, shape, dev):
    """fp16 q rows after the rotary embedding at `pos`, by qpal_rope_kv on a scratch cache"""
    nq, nkv, hd = shape
    nat = qp._native
    Ls = (max(pos) + 4) // 4 * 4
    kc = torch.zeros(nkv, Ls, hd, dtype=F16, device=dev)
    vc, zero = torch.zeros_like(kc), torch.zeros(nkv * hd, device=dev)
    q16 = torch.zeros(len(pos), nq * hd, dtype=F16, device=dev)
    pos_t, inv, q32 = torch.tensor(pos, dtype=torch.long, device=dev), ar.inv_freq(hd, dev), q32.contiguous()
    for r in range(len(pos)):
        nat.check(nat.lib().qpal_rope_kv(q32[r].data_ptr(), zero.data_ptr(), zero.data_ptr(), q16[r].data_ptr(), kc.data_ptr(), vc.data_ptr(),
                                         pos_t[r:r + 1].data_ptr(), inv.data_ptr(), nq, nkv, hd, Ls,
                                         torch.cuda.current_stream(dev).cuda_stream), "qpal_rope_kv")
    return q16


_WORST = {}


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "fp8"])
@pytest.mark.parametrize("ps", PAGES)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_families_against_float64_within_the_bound(dev, shape, ps, dtype):
    """base + FAMILIES, attention_fp64 on the gathered cache, bound(ref, A, Smax, u_p = 2^-11).  One group of three members whose
    prefix (1040 positions at page 16, 1088 at page 64) crosses the prefix kernel's key chunks, suffixes of 0, 37 and 700 cached
    positions (max_len 2048), and an ungrouped slot on the same cache; the needle once in the prefix and once in the suffix."""
    nq, nkv, hd = shape
    L, P = 2048, 1040 if ps == 16 else 1088
    pos = [P, P + 37, P + 700, P + 300]
    B, groups, scale, inv = 4, [([0, 1, 2], P)], 1.0 / math.sqrt(hd), ar.inv_freq(hd, dev)
    ws = qp.shared_prefix_workspace(B, 1, nq, nkv, hd, L, dev)
    pos_t = torch.tensor(pos, dtype=torch.long, device=dev)
    for family, needle_at in [("base", None)] + [(f, None) for f in ar.FAMILIES if f != "needle"] + [("needle", 700), ("needle", P + 20)]:
        tgt = ar.query_targets(B, nq, nkv, hd, 21, dev, family).view(B, nq, hd)
        q32 = ar.unrope(tgt, pos_t[:, None], inv).reshape(B, nq * hd)
        q16 = _rotated_q(q32, pos, shape, dev)
        K, V = ar.build_cache(family, q16, nq, nkv, hd, L, max(pos) + 1, scale, 28, needle_at=needle_at)
        k32 = torch.stack([ar.unrope(K[:, p], p, inv).reshape(nkv * hd) for p in pos])
        v32 = torch.stack([V[:, p].reshape(nkv * hd) for p in pos])
        Kc, Vc = ar.to_cache(K, dtype), ar.to_cache(V, dtype)
        stack = lambda c: torch.stack([c.view(torch.uint8)] * B).view(c.dtype)  # noqa: E731
        fk = Forked(stack(Kc), stack(Vc), ps, groups, seed=5)
        kp, vp = fk.clone_pools()
        for b in range(B):  # NaN into the rows this launch writes and into everything behind them
            for p in range(pos[b] // ps, fk.mp):
                page, lo = int(fk.table[b, p]), (pos[b] % ps if p == pos[b] // ps else 0)
                ar.nan_rows(kp[page], slice(lo, ps))
                ar.nan_rows(vp[page], slice(lo, ps))
        out = torch.full((B, nq * hd), float("nan"), dtype=F16, device=dev)
        qp.shared_prefix_decode_attention(*_qkv(q32, k32, v32), kp, vp, fk.table, pos_t, inv, fk.prefix(), scale=scale, out=out, ws=ws)
        torch.cuda.synchronize()
        gk, gv = fk.gather(kp), fk.gather(vp)
        worst = 0.0
        for b in range(B):
            exp, A, Smax = ar.attention_fp64(q16[b:b + 1], gk[b], gv[b], [pos[b] + 1], nq, nkv, hd, scale)
            r = (out[b:b + 1].double() - exp).abs() / ar.bound(exp, A, Smax, U_PREFIX)
            worst = max(worst, float(torch.nan_to_num(r, nan=float("inf")).max()))
        key = family
        _WORST[key] = max(_WORST.get(key, 0.0), worst)
        print(f"shared_prefix_decode_attention {family} {shape} page {ps} {dtype} needle={needle_at}: worst err/tol = {worst:.3f} "
              f"(so far over {family}: {_WORST[key]:.3f})")
        assert worst <= 1.0, (family, needle_at, worst)


# -------------------------------------------------------------------------------------------------------- whole model

@pytest.fixture(scope="module")
def model(dev):
    sys.path.insert(0, os.path.join(ROOT, "perf"))
    from decode_llama import build_model
    return build_model("3_8b", "tcomb_6_7_0.5_none_0.9", None, 2, 4096, dev)


def test_captured_step_on_a_forked_cache(dev, model):
    """two layers of 3_8b, vocab 4096, page_size 16, B = 4: a prompt of 40 tokens prefilled into slot 0 and forked into slots 1 and 2
    (a group of 32 shared positions), slot 3 with a prompt of its own.  DecodeStep(shared_prefix=cache.prefix) captured with
    torch.cuda.graph and replayed for 8 steps with positions advanced; after step 3 slot 0 — the slot grp_slot names — is released
    and the group re-pointed to slot 1.  The eager shared_prefix=None step on a second cache built by the same calls gives the same
    tokens, and the final hidden state agrees within the whole-model bound 2^-7 max(1, max |ref|) of perf/decode_llama_batch.py's
    check."""
    m, B, ps, mp = model, 4, 16, 8
    nkv, hd, nl = m.cfg.num_key_value_heads, m.cfg.head_dim, len(m.layers)
    g = torch.Generator().manual_seed(9)
    prompts = [torch.randint(0, 4096, (n,), generator=g).to(dev) for n in (40, 21)]
    caches, firsts = [], []
    for _ in range(2):
        c = qp.PagedKVCache(nl, 4 * mp, nkv, ps, hd, B, mp, device=dev, min_len=ps, min_members=2)
        pf = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, c.kpool, c.vpool, m.inv_freq, chunk=64, block_table=c.table)
        c.reserve(0, 40 + 9)
        c.reserve(3, 21 + 9)
        firsts = [int(pf(prompts[0], slot=0, pos0=0)), int(pf(prompts[1], slot=3, pos0=0))]
        for dst in (1, 2):
            c.fork(0, dst, 40)
            c.reserve(dst, 40 + 9)
        caches.append(c)
    shared, plain = caches
    assert shared.prefix.row_group.tolist() == [0, 0, 0, -1] and shared.prefix.grp_len.tolist()[0] == 32
    assert torch.equal(shared.table, plain.table)
    start_tok = torch.tensor([firsts[0], firsts[0] + 1, firsts[0] + 2, firsts[1]], device=dev) % 4096
    start_pos = torch.tensor([40, 40, 40, 21], dtype=torch.long, device=dev)
    tok_s, pos_s, out_s = start_tok.clone(), start_pos.clone(), torch.zeros(B, dtype=torch.long, device=dev)
    tok_p, pos_p, out_p = start_tok.clone(), start_pos.clone(), torch.zeros(B, dtype=torch.long, device=dev)
    st_p = qp.DecodeStep(m.layers, m.embed, m.norm, m.lm_head, plain.kpool, plain.vpool, m.inv_freq, tok_p, pos_p, out_p,
                         block_table=plain.table)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        st_s = qp.DecodeStep(m.layers, m.embed, m.norm, m.lm_head, shared.kpool, shared.vpool, m.inv_freq, tok_s, pos_s, out_s,
                             block_table=shared.table, shared_prefix=shared.prefix)
        assert st_s.launches_per_token == st_p.launches_per_token + nl
        st_s()  # warm-up (the rows it appends are appended again by the first replay)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            st_s()
        for i in range(8):
            if i == 4:
                for c, pos in ((shared, pos_s), (plain, pos_p)):
                    c.release(0)
                    pos[0] = -1
                assert shared.prefix.grp_slot.tolist()[0] == 1 and shared.prefix.row_group.tolist() == [-1, 0, 0, -1]
            graph.replay()
            st_p()
            torch.cuda.synchronize()
            act = pos_s >= 0
            hs, hp = st_s.hidden()[act].float(), st_p.hidden()[act].float()
            err, top = float((hs - hp).abs().max()), float(hp.abs().max())
            print(f"step {i}: tokens {out_s[act].tolist()} / {out_p[act].tolist()}, hidden max |diff| {err:.3e} (max |ref| {top:.3f})")
            assert out_s[act].tolist() == out_p[act].tolist()
            assert err <= 2.0 ** -7 * max(1.0, top)
            for tok, out, pos in ((tok_s, out_s, pos_s), (tok_p, out_p, pos_p)):
                tok.copy_(torch.where(pos >= 0, out, tok))
                pos.add_((pos >= 0).long())
    torch.cuda.current_stream(dev).wait_stream(s)
