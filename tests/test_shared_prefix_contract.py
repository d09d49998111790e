"""Shared-prefix decode attention without a GPU: the groups PagedKVCache publishes stay true under random
reserve / fork / release, the membership rule as restated in numpy, the C-ABI is exported and declared, and the argument errors."""
import os
import random

import numpy as np
import pytest
import torch

import qpalette_amd as qp
from qpalette_amd._native import QpalError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PS = 16


def _check_invariants(c, model):
    """model: slot -> (pages, shared_upto) kept by the test from the rules PagedKVCache had before it knew of groups"""
    px = c.prefix
    rg, gs, gl = px.row_group.tolist(), px.grp_slot.tolist(), px.grp_len.tolist()
    assert len(rg) == c.B and len(gs) == len(gl) == px.G
    refs = {}
    for slot in range(c.B):
        pages, shared = model[slot]
        assert c.pages_of(slot) == pages and c.shared_upto(slot) == shared
        assert c.table[slot].tolist() == pages + [-1] * (c.max_pages - len(pages))
        for p in pages:
            refs[p] = refs.get(p, 0) + 1
    assert all(c.refcount(p) == refs.get(p, 0) for p in range(c.num_pages)) and c.pages_free == c.num_pages - len(refs)
    for g in range(px.G):
        members = [b for b in range(c.B) if rg[b] == g]
        assert members == sorted(c.members_of(g))
        if not members:
            assert gl[g] == 0 and gs[g] == -1
            continue
        assert len(members) >= 2 and gs[g] in members and c.pages_of(gs[g])  # a live member
        assert gl[g] > 0 and gl[g] % PS == 0 and gl[g] >= c.min_len
        n = gl[g] // PS
        head = c.pages_of(gs[g])[:n]
        assert len(head) == n
        for b in members:
            assert c.pages_of(b)[:n] == head and c.group_of(b) == g
        assert all(c.refcount(p) >= len(members) for p in head)
    assert all(-1 <= x < px.G for x in rg)


@pytest.mark.parametrize("seed", range(6))
def test_random_reserve_fork_release_keep_the_groups_true(seed):
    rnd = random.Random(seed)
    B, mp, G = 10, 12, 3 if seed % 2 else 16  # (G = 3: forks meet a full set of groups)
    c = qp.PagedKVCache(1, 60, 2, PS, 8, B, mp, groups=G, min_len=PS, min_members=2)
    model = {b: ([], 0) for b in range(B)}
    free = list(range(c.num_pages - 1, -1, -1))
    refs = [0] * c.num_pages
    forks = grouped = 0
    for _ in range(400):
        op = rnd.random()
        slot = rnd.randrange(B)
        pages, shared = model[slot]
        if op < 0.35:  # reserve
            n = rnd.randrange(0, mp * PS + 1)
            need = (n + PS - 1) // PS - len(pages)
            if need > len(free):
                with pytest.raises(QpalError):
                    c.reserve(slot, n)
            else:
                c.reserve(slot, n)
                for _ in range(max(need, 0)):
                    p = free.pop()
                    refs[p] = 1
                    pages = pages + [p]
                model[slot] = (pages, shared)
        elif op < 0.6:  # release
            c.release(slot)
            for p in reversed(pages):
                refs[p] -= 1
                if refs[p] == 0:
                    free.append(p)
            model[slot] = ([], 0)
        else:  # fork slot -> dst
            dst = rnd.randrange(B)
            if dst == slot or model[dst][0] or not pages:
                continue
            n = rnd.randrange(0, len(pages) * PS + 1)
            full, part = divmod(n, PS)
            if part and not free:
                continue
            c.fork(slot, dst, n)
            forks += 1
            new = pages[:full]
            for p in new:
                refs[p] += 1
            if part:
                p = free.pop()
                refs[p] = 1
                new = new + [p]
            model[dst] = (new, n)
            grouped += c.group_of(dst) >= 0
        _check_invariants(c, model)
    assert forks > 20 and grouped > 5


def test_fork_rules_of_groups():
    c = qp.PagedKVCache(1, 40, 2, PS, 8, 8, 8, groups=2, min_len=2 * PS, min_members=2)
    c.reserve(0, 100)
    c.fork(0, 1, 31)                      # one whole page: below min_len
    assert c.group_of(1) == -1 and c.prefix.row_group.tolist() == [-1] * 8
    c.fork(0, 2, 70)                      # four whole pages: a group of length 64
    assert c.group_of(0) == c.group_of(2) == 0 and c.prefix.grp_len.tolist() == [64, 0] and c.prefix.grp_slot.tolist() == [0, -1]
    c.fork(0, 3, 63)                      # shorter than the group: ungrouped
    assert c.group_of(3) == -1
    c.fork(2, 4, 64)                      # from another member, the group's length: joins
    assert c.members_of(0) == [0, 2, 4]
    c.reserve(5, 40)
    c.fork(5, 6, 40)
    assert c.members_of(1) == [5, 6] and c.prefix.grp_len.tolist() == [64, 32]
    c.release(1)
    c.reserve(1, 40)
    c.fork(1, 7, 40)                      # both groups are taken: the fork stays ungrouped
    assert c.group_of(7) == -1 and c.group_of(1) == -1
    c.release(0)                          # grp_slot re-points to a survivor
    assert c.prefix.grp_slot.tolist() == [2, 5] and c.prefix.row_group.tolist() == [-1, -1, 0, -1, 0, 1, 1, -1]
    c.release(6)                          # fewer than two members: dissolved
    assert c.members_of(1) == [] and c.prefix.grp_len.tolist() == [64, 0] and c.prefix.row_group.tolist()[5] == -1
    d = qp.PagedKVCache(1, 4, 1, PS, 8, 2, 2)
    assert (d.min_len, d.min_members) == (qp.paging.MIN_SHARED_LEN, qp.paging.MIN_SHARED_MEMBERS) == (2048, 32)
    # a group is published once it has min_members members, and withdrawn when it falls below
    e = qp.PagedKVCache(1, 40, 2, PS, 8, 5, 4, min_len=PS, min_members=3)
    e.reserve(0, 40)
    e.fork(0, 1, 32)
    assert e.group_of(1) == 0 and not e.published(0) and e.prefix.row_group.tolist() == [-1] * 5 and e.prefix.grp_len.tolist()[0] == 0
    e.fork(1, 2, 32)
    assert e.published(0) and e.prefix.row_group.tolist() == [0, 0, 0, -1, -1] and (e.prefix.grp_slot.tolist()[0], e.prefix.grp_len.tolist()[0]) == (0, 32)
    e.release(0)
    assert e.members_of(0) == [1, 2] and e.prefix.row_group.tolist() == [-1] * 5 and e.prefix.grp_slot.tolist()[0] == -1
    with pytest.raises(QpalError):
        qp.PagedKVCache(1, 4, 1, PS, 8, 2, 2, groups=17)


def test_reference_shared_rows_guards():
    ref = qp.reference_shared_rows
    # slot:       member  id<0  id>=G  slot oor  len 0  no multiple  len > pos  inactive -1  inactive max_len  len == pos
    row_group = [0,      -1,   6,     1,        2,     3,           0,         0,           0,               4]
    pos       = [100,    100,  100,   100,      100,   100,         31,        -1,          256,             48]
    grp_slot = [0, 10, 4, 5, 9, -1]
    grp_len = [32, 32, 0, 40, 48, 32]
    g, n = ref(row_group, grp_slot, grp_len, pos, 16, 256)
    assert g.tolist() == [0, -1, -1, -1, -1, -1, -1, -1, -1, 4] and n.tolist() == [32, 0, 0, 0, 0, 0, 0, 0, 0, 48]
    g, n = ref([5, 0], grp_slot, grp_len, [100, 100], 16, 256)  # grp_slot -1; B = 2 puts grp_slot 0 in range, 10 stays out
    assert g.tolist() == [-1, 0] and n.tolist() == [0, 32]
    g, n = ref([0, 0], [0], [64], [64, 63], 32, 128)
    assert g.tolist() == [0, -1] and n.tolist() == [64, 0]
    g, n = ref([0], [0], [64], [70], 128, 256)  # a multiple of 16 is no multiple of this page size
    assert g.tolist() == [-1]
    assert isinstance(g, np.ndarray) and g.dtype == np.int64


def test_symbols_are_exported_bound_and_declared():
    lib = qp._native.lib()
    header = open(os.path.join(ROOT, "include", "qpal.h")).read()
    for name in ("qpal_attn_prefix_ws_bytes", "qpal_attn_rope_decode_batch_shared"):
        assert name in qp._native.exported_symbols() and hasattr(lib, name) and name + "(" in header
    for name in ("shared_prefix_decode_attention", "shared_prefix_workspace", "reference_shared_rows", "SharedPrefix"):
        assert hasattr(qp, name)
    plain = lib.qpal_attn_batch_ws_bytes(64, 32, 8, 128, 8192)
    assert lib.qpal_attn_prefix_ws_bytes(64, 16, 32, 8, 128, 8192) > plain > 0
    assert lib.qpal_attn_prefix_ws_bytes(4, 1, 8, 2, 64, 256) > 0 == lib.qpal_attn_batch_ws_bytes(4, 8, 2, 64, 256)
    for bad in ((64, 0, 32, 8, 128, 8192), (64, 17, 32, 8, 128, 8192), (129, 4, 32, 8, 128, 8192), (4, 4, 32, 8, 96, 8192)):
        assert lib.qpal_attn_prefix_ws_bytes(*bad) == 0


def test_c_entry_argument_errors_follow_the_paged_sibling():
    """null first, then the paged shape, the geometry, the group count, alignment, the workspace"""
    lib = qp._native.lib()

    def call(q=16, tab=16, rg=16, gs=16, gl=16, G=4, B=4, ps=16, hd=128, ws=16, ws_bytes=1 << 30, kpool=4096):
        return lib.qpal_attn_rope_decode_batch_shared(q, 16, 16, 4096, kpool, 4096, 16, 4096, 16, 16, tab, 64, 100, ps, 64, 0, rg, gs, gl, G, B,
                                                      32, 8, hd, 0.1, ws, ws_bytes, None)

    base = lib.qpal_attn_rope_decode_batch_paged(None, 16, 16, 4096, 4096, 4096, 16, 4096, 16, 16, 16, 64, 100, 16, 64, 0, 4, 32, 8, 128, 0.1,
                                                 16, 1 << 30, None)
    E_NULL = base
    assert E_NULL != 0
    assert call(q=None) == call(tab=None) == call(rg=None) == call(gs=None) == call(gl=None) == E_NULL
    E_SHAPE = lib.qpal_attn_rope_decode_batch_paged(16, 16, 16, 4096, 4096, 4096, 16, 4096, 16, 16, 16, 64, 100, 17, 64, 0, 4, 32, 8, 128, 0.1,
                                                    16, 1 << 30, None)
    assert E_SHAPE not in (0, E_NULL)
    assert call(ps=17) == call(hd=96) == call(G=0) == call(G=17) == call(B=129) == call(ws_bytes=64) == E_SHAPE
    E_ALIGN = lib.qpal_attn_rope_decode_batch_paged(16, 16, 16, 4096, 4100, 4096, 16, 4096, 16, 16, 16, 64, 100, 16, 64, 0, 4, 32, 8, 128, 0.1,
                                                    16, 1 << 30, None)
    assert E_ALIGN not in (0, E_NULL, E_SHAPE)
    assert call(kpool=4100) == call(rg=18) == call(gs=18) == call(gl=18) == call(tab=18) == call(ws=18) == E_ALIGN
    assert call(ws=None) == E_NULL
    assert call(ps=17, kpool=4100) == E_SHAPE  # shape in front of alignment


def _cpu_args(B=3, nq=4, nkv=2, hd=64, ps=16, mp=4, G=2):
    pools = [torch.zeros(8, nkv, ps, hd, dtype=torch.float16) for _ in range(2)]
    table = torch.zeros(B, mp, dtype=torch.int32)
    q, k, v = torch.zeros(B, nq * hd), torch.zeros(B, nkv * hd), torch.zeros(B, nkv * hd)
    px = qp.SharedPrefix.empty(B, G)
    return [q, k, v, *pools, table, torch.zeros(B, dtype=torch.long), torch.zeros(hd // 2)], px


def test_python_entry_rejects_bad_prefix_tensors():
    args, px = _cpu_args()
    f = qp.shared_prefix_decode_attention
    mk = lambda **kw: qp.SharedPrefix(kw.get("rg", px.row_group), kw.get("gs", px.grp_slot), kw.get("gl", px.grp_len))  # noqa: E731
    for bad, word in ((mk(rg=px.row_group.long()), "row_group"), (mk(gs=px.grp_slot.float()), "grp_slot"),
                      (mk(gl=px.grp_len.view(1, -1)), "grp_len"), (mk(rg=torch.zeros(4, dtype=torch.int32)), "row_group"),
                      (mk(gs=torch.zeros(3, dtype=torch.int32)), "grp_slot"), (mk(gs=torch.zeros(17, dtype=torch.int32),
                                                                                  gl=torch.zeros(17, dtype=torch.int32)), "1 <= G <= 16"),
                      (mk(gs=torch.zeros(0, dtype=torch.int32), gl=torch.zeros(0, dtype=torch.int32)), "1 <= G <= 16"),
                      (mk(rg=torch.zeros(6, dtype=torch.int32)[::2]), "row_group"), (object(), "row_group"), (None, "row_group")):
        with pytest.raises(QpalError, match=word):
            f(*args, bad)
    if torch.cuda.is_available():  # (a tensor on another device than the pools')
        with pytest.raises(QpalError, match="device"):
            f(*args, qp.SharedPrefix.empty(3, 2, device="cuda:0"))
    with pytest.raises(QpalError, match="block_table"):
        f(*args[:5], args[5][0], *args[6:], px)
    with pytest.raises(QpalError):  # the checks of paged_decode_attention follow: the pools of this machine's host are no device tensors
        f(*args, px)
    bad_table = list(args)
    bad_table[5] = args[5].long()
    with pytest.raises(QpalError, match="int32"):
        f(*bad_table, px)


def test_decode_step_wants_a_block_table_with_a_shared_prefix():
    z = torch.zeros(2, dtype=torch.long)
    with pytest.raises(QpalError, match="shared_prefix"):
        qp.DecodeStep([], None, None, None, [], [], None, z, z, z, shared_prefix=qp.SharedPrefix.empty(2, 1))
