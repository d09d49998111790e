"""Draft trees, the contracts (CPU only): reference_spec_tree_draft / reference_spec_tree_accept on hand-made trees,
the return codes of the four entry points without a device, and the losslessness loop of tests/test_spec_contract.py for trees."""
import numpy as np
import pytest

import qpalette_amd as qp
from qpalette_amd import speculative as sp

E_SHAPE, E_NULL, E_ALIGN = -1, -3, -4


def _draft(n_tok, limit, tok, par, ext_n, N=7, R=32, max_len=64, ld=32):
    B = len(n_tok)
    hist = np.arange(B * ld, dtype=np.int32).reshape(B, ld) % 50 + 100
    return hist, sp.reference_spec_tree_draft(hist, n_tok, limit, N, 2, 4, R, max_len, ext_tok=np.array(tok), ext_par=np.array(par),
                                              ext_n=ext_n)


#           nodes:  1   2   3   4   5   6   7          a root with two children (1, 2), 1 has (3, 4), 3 has 5, 2 has 6, 5 has 7
TOK, PAR = [11, 12, 13, 14, 15, 16, 17], [0, 0, 1, 1, 3, 2, 5]
DEPTH, ANC = [0, 1, 1, 2, 2, 3, 2, 4], [0b1, 0b11, 0b101, 0b1011, 0b10011, 0b101011, 0b1000101, 0b10101011]


@pytest.mark.parametrize("case, tok, par, kw, rows", [
    ("whole", TOK, PAR, {}, 8),
    ("invalid parent", TOK, [0, 0, 1, 4, 3, 2, 5], {}, 4),            # node 4 names itself: the list ends in front of it
    ("bad token", [11, 12, 2 ** 30, 14, 15, 16, 17], PAR, {}, 3),
    ("depth cut", TOK, PAR, {"limit": [10 + 1 + 3]}, 7),                # d_max = 3: node 7 (depth 4) ends the list
    ("ext_n", TOK, PAR, {"ext_n": [5]}, 6),
    ("cache end", TOK, PAR, {"max_len": 14}, 5),                        # slots 9 .. 13 exist: nodes 1 .. 4
    ("budget", TOK, PAR, {"R": 4}, 4),
])
def test_one_slot_tree(case, tok, par, kw, rows):
    limit, ext_n = kw.pop("limit", [40]), kw.pop("ext_n", [7])
    hist, d = _draft([10], limit, [tok], [par], ext_n, **kw)
    assert d["row0"].tolist() == [0, rows] and d["n_draft"].tolist() == [rows - 1] and d["pos0"].tolist() == [9]
    assert d["tokens"][:rows].tolist() == [int(hist[0, 9])] + tok[:rows - 1]
    assert d["depth"][:rows].tolist() == DEPTH[:rows] and d["anc"][:rows].tolist() == ANC[:rows]
    assert d["row_ctr"][:rows].tolist() == [9 + x for x in DEPTH[:rows]] and (d["row_ctr"][rows:] == -1).all()
    assert (d["anc"][rows:] == 0).all() and (d["row_slot"][rows:] == -1).all()


def test_budget_over_slots_and_the_lookup_chain():
    """R = 9 over three active slots and an inactive one: every root row, then nodes in slot order — 5, 1, 0"""
    _, d = _draft([10, 10, 0, 10], [40] * 4, [TOK] * 4, [PAR] * 4, [5, 7, 7, 7], R=9)
    assert d["n_draft"].tolist() == [5, 1, 0, 0] and d["row0"].tolist() == [0, 6, 8, 8, 9] and d["seq"].tolist() == [0, 1, -1, 3]
    assert d["depth"].tolist() == DEPTH[:6] + DEPTH[:2] + [0] and d["anc"].tolist() == ANC[:6] + ANC[:2] + [1]
    # without ext_tok: the chain of reference_spec_draft's lookup, K = min(N, 15)
    hist = np.array([[1, 2, 3, 4, 5, 1, 2, 3] + [0] * 8], np.int32)
    c = sp.reference_spec_draft(hist, [8], [40], 3, 2, 4, 8, 64)
    t = sp.reference_spec_tree_draft(hist, [8], [40], 3, 2, 4, 8, 64)
    assert all(np.array_equal(t[k], c[k]) for k in c) and t["n_draft"][0] == 3
    assert t["depth"].tolist() == [0, 1, 2, 3, 0, 0, 0, 0] and t["anc"].tolist() == [1, 3, 7, 15, 0, 0, 0, 0]
    assert sp.reference_spec_tree_draft(hist, [8], [40], 31, 2, 4, 32, 64)["n_draft"][0] == 5  # the history's end cuts the chain


def _accept(drawn, n=10, limit=40, eos=-1, tok=TOK):
    hist, d = _draft([n], [limit], [tok], [PAR], [7])
    out0 = np.full((1, 16), -7, np.int64)
    a = sp.reference_spec_tree_accept(d["tokens"], drawn + [0] * 24, d["seq"], d["row0"], d["depth"], d["anc"], hist, [n], [limit], [eos],
                                      out_tok=out0)
    return a, a["out_tok"][0, :a["n_out"][0]].tolist(), a["path"][0].tolist()


def test_accept_walks_the_lowest_matching_child():
    #          row:  0   1   2   3   4   5   6   7
    a, out, path = _accept([12, 0, 16, 0, 0, 0, 99, 0])             # root -> node 2 -> node 6 -> nothing
    assert out == [12, 16, 99] and path == [0, 2, 6] + [-1] * 13 and a["n_acc"][0] == 2 and a["n_tok"][0] == 13
    a, out, path = _accept([11, 13, 0, 15, 0, 17, 0, 5])            # the deepest path: 0 1 3 5 7
    assert out == [11, 13, 15, 17, 5] and path[:5] == [0, 1, 3, 5, 7] and a["n_acc"][0] == 4
    a, out, path = _accept([50, 13, 16, 15, 0, 17, 0, 5])           # the root's draw is no child's token
    assert out == [50] and path == [0] + [-1] * 15 and a["n_acc"][0] == 0
    # duplicate sibling tokens: nodes 1 and 2 both carry 11; the lower index wins and ITS draw goes on
    a, out, path = _accept([11, 13, 16, 0, 0, 0, 0, 0], tok=[11, 11, 13, 14, 15, 16, 17])
    assert path[:3] == [0, 1, 3] and out == [11, 13, 0]
    # a token equal to a non-child's (node 6 carries 16, a child of node 2) is no match under node 1
    a, out, path = _accept([11, 16, 0, 0, 0, 0, 0, 0])
    assert path[:3] == [0, 1, -1] and out == [11, 16]


def test_accept_cuts_at_limit_and_eos():
    a, out, path = _accept([11, 13, 0, 15, 0, 17, 0, 5], limit=13)     # three tokens fit (the draft saw d_max = 2: node 5 is cut)
    assert out == [11, 13, 15] and a["n_acc"][0] == 2 and a["n_tok"][0] == 13
    a, out, path = _accept([11, 13, 0, 15, 0, 17, 0, 5], eos=13)
    assert out == [11, 13] and a["n_acc"][0] == 4 and a["limit"][0] == 12 and path[:5] == [0, 1, 3, 5, 7]
    assert a["out_tok"][0, 2:].tolist() == [-7] * 14 and a["hist"][0, 10:12].tolist() == [11, 13]
    a, out, path = _accept([11] * 8, n=10, limit=10)                   # at its limit: nothing counts
    assert a["n_out"][0] == 0 and path == [0] + [-1] * 15


def test_a_chain_is_the_chain_accept():
    rng = np.random.default_rng(3)
    B, K, R, ld = 6, 15, 96, 64
    hist = rng.integers(0, 4, size=(B, ld)).astype(np.int32)
    n_tok, limit, eos = rng.integers(1, 30, size=B), rng.integers(20, 50, size=B), np.array([-1, 2, -1, 1, -1, 3])
    ext = rng.integers(0, 4, size=(B, K))
    par = np.tile(np.arange(K), (B, 1))
    c = sp.reference_spec_draft(hist, n_tok, limit, K, 2, 4, R, 64, ext_draft=ext, ext_n=np.full(B, K))
    t = sp.reference_spec_tree_draft(hist, n_tok, limit, K, 2, 4, R, 64, ext_tok=ext, ext_par=par, ext_n=np.full(B, K))
    assert all(np.array_equal(t[k], c[k]) for k in c)
    drawn = rng.integers(0, 4, size=R)
    drawn[:-1] = np.where(rng.random(R - 1) < 0.8, c["tokens"][1:], drawn[:-1])
    ca = sp.reference_spec_accept(c["tokens"], drawn, c["seq"], c["row0"], hist, n_tok, limit, eos, K)
    ta = sp.reference_spec_tree_accept(t["tokens"], drawn, t["seq"], t["row0"], t["depth"], t["anc"], hist, n_tok, limit, eos)
    assert all(np.array_equal(ta[k], ca[k]) for k in ca) and int(ca["n_acc"].max()) >= 2
    for b in range(B):
        assert ta["path"][b, :ta["n_acc"][b] + 1].tolist() == list(range(ta["n_acc"][b] + 1))


def test_tree_argument_errors_without_a_gpu():
    """every argument error is returned before any stream work: the pointers below are never dereferenced"""
    lib = qp._native.lib()

    def call(fn, names, defaults, **kw):
        return getattr(lib, fn)(*[kw.get(n, d) for n, d in zip(names, defaults)])

    draft = ("qpal_spec_tree_draft", "hist ld n_tok limit ext_tok ext_par ext_n B N gmin gmax R L tokens seq row0 pos0 row_slot row_ctr "
             "n_draft depth anc stream".split(), [16, 64, 16, 16, None, None, None, 4, 7, 2, 4, 20, 64] + [16] * 9 + [None])
    accept = ("qpal_spec_tree_accept", "tokens drawn seq row0 depth anc hist ld n_tok limit eos B R out_tok n_out n_acc path stream".split(),
              [16] * 7 + [64, 16, 16, 16, 4, 20, 16, 16, 16, 16, None])
    attn = ("qpal_attn_rope_prefill_ragged_tree", "q k v ld kc vc out ldo seq row0 pos0 depth anc inv fmt R S B nq nkv hd L scale ws wsb "
            "stream".split(), [16, 16, 16, 1024, 16, 16, 16, 1024, 16, 16, 16, 16, 16, 16, 0, 32, 2, 2, 8, 2, 128, 256, 0.1, None, 0, None])
    paged = ("qpal_attn_rope_prefill_ragged_tree_paged", "q k v ld kc vc out ldo seq row0 pos0 depth anc inv table ldt np ps mp fmt R S B "
             "nq nkv hd scale ws wsb stream".split(),
             [16, 16, 16, 1024, 16, 16, 16, 1024, 16, 16, 16, 16, 16, 16, 16, 16, 64, 16, 16, 0, 32, 2, 2, 8, 2, 128, 0.1, None, 0, None])
    compact = ("qpal_kv_compact", "kp vp layers pos0 path n_acc table ldt np ps mp fmt B nkv hd L stream".split(),
               [16, 16, 2, 16, 16, 16, None, 0, 0, 0, 0, 0, 4, 2, 128, 256, None])
    cases = [
        (draft, E_NULL, [{n: None} for n in "hist n_tok limit tokens seq row0 pos0 row_slot row_ctr n_draft depth anc".split()]
         + [{"ext_tok": 16}, {"ext_tok": 16, "ext_par": 16}]),
        (draft, E_SHAPE, [{"B": 0}, {"N": -1}, {"N": 32}, {"gmin": 0}, {"gmax": 9}, {"R": 3}, {"R": 129}, {"L": 0}, {"ld": 0}]),
        (draft, E_ALIGN, [{"depth": 18}, {"anc": 17}, {"n_tok": 20}, {"ext_tok": 18, "ext_par": 16, "ext_n": 16}]),
        (accept, E_NULL, [{n: None} for n in "tokens drawn seq row0 depth anc hist n_tok limit eos out_tok n_out n_acc path".split()]),
        (accept, E_SHAPE, [{"B": 0}, {"B": 129, "R": 129}, {"R": 3}, {"R": 129}, {"ld": 0}]),
        (accept, E_ALIGN, [{"depth": 18}, {"anc": 18}, {"path": 17}, {"out_tok": 20}]),
        (attn, E_NULL, [{"depth": None}, {"anc": None}, {"q": None}]),
        (attn, E_SHAPE, [{"fmt": 2}, {"S": 0}, {"R": 129}, {"hd": 96}]),
        (attn, E_ALIGN, [{"depth": 18}, {"anc": 17}]),
        (paged, E_NULL, [{"depth": None}, {"anc": None}, {"table": None}]),
        (paged, E_SHAPE, [{"ps": 24}, {"fmt": 2}]),
        (paged, E_ALIGN, [{"depth": 18}, {"anc": 17}]),
        (compact, E_NULL, [{"kp": None}, {"vp": None}, {"pos0": None}, {"path": None}, {"n_acc": None}]),
        (compact, E_SHAPE, [{"layers": 0}, {"B": 0}, {"B": 129}, {"nkv": 0}, {"hd": 96}, {"fmt": 2}, {"L": 6}, {"table": 16, "ps": 24}]),
        (compact, E_ALIGN, [{"kp": 20}, {"pos0": 20}, {"path": 18}, {"n_acc": 17}]),
    ]
    for (fn, names, defaults), code, kws in cases:
        for kw in kws:
            assert call(fn, names, defaults, **kw) == code, (fn, kw)


@pytest.mark.parametrize("right", [0, 1, None], ids=["first-sibling", "second-sibling", "absent"])
def test_the_emitted_stream_is_the_sequential_stream(right):
    """tests/test_spec_contract.py's toy model (the next token is a fixed function of the last three over a vocabulary of 7).  Every
    step offers a tree of width 2 and depth 3 whose sibling `right` carries the sequential token of its level: tree draft -> one toy
    draw per row on the row's ROOT PATH -> tree accept.  Token for token the sequential stream; with a right sibling every step
    accepts the tree's whole depth, where a chain step that holds the wrong sibling first would accept nothing."""
    V, B, new, ld, D, W = 7, 4, 60, 96, 3, 2
    rng = np.random.default_rng(5)
    table = rng.integers(0, V, size=(V, V, V))
    nxt = lambda ctx: int(table[ctx[-3], ctx[-2], ctx[-1]])
    prompts = [list(rng.integers(0, V, size=n)) for n in (3, 4, 9, 17)]
    want = []
    for p in prompts:
        s = list(p)
        for _ in range(new):
            s.append(nxt(s))
        want.append(s[len(p):])
    hist = np.zeros((B, ld), np.int32)
    for b, p in enumerate(prompts):
        hist[b, :len(p)] = p
    n_tok, limit, eos = np.array([len(p) for p in prompts]), np.array([len(p) + new for p in prompts]), np.full(B, -1)
    got, R, N = [[] for _ in range(B)], B * (D * W + 1) - 2, D * W   # 26 rows for 28: the cut at R takes part
    while (n_tok < limit).any():
        tok, par = np.zeros((B, N), np.int32), np.zeros((B, N), np.int32)
        for b in range(B):  # level l: W children of the previous level's right (or first) sibling
            ctx, up = list(hist[b, :n_tok[b]]), 0
            for l in range(D):
                t = nxt(ctx)
                for w in range(W):
                    tok[b, l * W + w] = t if w == right else (t + 1 + w) % V
                    par[b, l * W + w] = up
                up, ctx = l * W + 1 + (right or 0), ctx + [t]
        d = sp.reference_spec_tree_draft(hist, n_tok, limit, N, 2, 4, R, ld, ext_tok=tok, ext_par=par, ext_n=np.full(B, N))
        drawn = np.zeros(R, np.int64)
        for r in range(R):
            b = int(d["row_slot"][r])
            if b >= 0:
                r0 = int(d["row0"][b])
                path = [j for j in range(1, r - r0 + 1) if (int(d["anc"][r]) >> j) & 1]
                drawn[r] = nxt(list(hist[b, :n_tok[b]]) + [int(d["tokens"][r0 + j]) for j in path])
        a = sp.reference_spec_tree_accept(d["tokens"], drawn, d["seq"], d["row0"], d["depth"], d["anc"], hist, n_tok, limit, eos)
        for b in range(B):
            if d["seq"][b] >= 0 and right is not None:  # the whole depth the draft kept for this slot
                assert a["n_acc"][b] == int(d["depth"][d["row0"][b]:d["row0"][b + 1]].max()), (b, a["n_acc"][b])
            if right is None:
                assert a["n_acc"][b] == 0
            got[b] += a["out_tok"][b, :a["n_out"][b]].tolist()
        hist, n_tok, limit = a["hist"], a["n_tok"], a["limit"]
    assert got == want
