"""Speculative decoding without a GPU: the two numpy references on hand-made cases, the losslessness argument run as
a test on a toy model, the C-ABI's argument errors as return codes, and the wrappers' checks in front of the library.  The kernel
tests (tests/test_spec.py) hold qpal_spec_draft / qpal_spec_accept to these references bit for bit."""
import os

import numpy as np
import pytest
import torch

import qpalette_amd as qp
from qpalette_amd import speculative as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_SHAPE, E_NULL, E_ALIGN = -1, -3, -4


def _hist(rows, ld=24):
    h = np.zeros((len(rows), ld), np.int32)
    for b, r in enumerate(rows):
        h[b, :len(r)] = r
    return h, [len(r) for r in rows]


def _draft(rows, K=4, gram=(2, 4), R=None, max_len=64, limit=None, ld=24, **kw):
    h, n = _hist(rows, ld)
    R = len(rows) * (K + 1) if R is None else R
    return sp.reference_spec_draft(h, n, [60] * len(rows) if limit is None else limit, K, gram[0], gram[1], R, max_len, **kw)


# ---------------------------------------------------------------------------------------------------------------- the draft

def test_lookup_matches_at_gmax():
    d = _draft([[1, 2, 3, 4, 5, 9, 1, 2, 3, 4]])
    assert d["tokens"].tolist() == [4, 5, 9, 1, 2] and d["n_draft"].tolist() == [4]
    assert d["seq"].tolist() == [0] and d["row0"].tolist() == [0, 5] and d["pos0"].tolist() == [9]
    assert d["row_slot"].tolist() == [0] * 5 and d["row_ctr"].tolist() == [9, 10, 11, 12, 13]
    assert d["tokens"].dtype == np.int64 and d["seq"].dtype == np.int32 and d["row0"].dtype == np.int32
    assert d["pos0"].dtype == np.int64 and d["row_slot"].dtype == np.int32 and d["row_ctr"].dtype == np.int64


def test_lookup_falls_back_to_a_smaller_gram():
    # [8 2 3 4] and [2 3 4] occur nowhere else; [3 4] does, at 1: the drafts follow it
    d = _draft([[7, 3, 4, 5, 8, 2, 3, 4]])
    assert d["tokens"].tolist() == [4, 5, 8, 2, 3] and d["n_draft"].tolist() == [4]
    # gmin = 3 forbids the 2-gram: a plain decode token
    d = _draft([[7, 3, 4, 5, 8, 2, 3, 4]], gram=(3, 4))
    assert d["tokens"].tolist() == [4, 0, 0, 0, 0] and d["n_draft"].tolist() == [0] and d["row0"].tolist() == [0, 1]
    assert d["row_slot"].tolist() == [0, -1, -1, -1, -1] and d["row_ctr"].tolist() == [7, -1, -1, -1, -1]


def test_the_longest_gram_beats_a_more_recent_shorter_one_and_the_most_recent_occurrence_wins():
    # [5 1 2] occurs at 0 (followed by 7); [1 2] also at 4 (followed by 9), more recent but shorter
    d = _draft([[5, 1, 2, 7, 1, 2, 9, 5, 1, 2]], gram=(2, 3), K=1)
    assert d["tokens"].tolist() == [2, 7]
    # [1 2] at 0, 3: the later one gives the drafts, which then run into the end of the history (3 of K = 4)
    d = _draft([[1, 2, 7, 1, 2, 8, 1, 2]], gram=(2, 2))
    assert d["tokens"].tolist() == [2, 8, 1, 2, 0] and d["n_draft"].tolist() == [3] and d["row0"].tolist() == [0, 4]
    # an overlapping match: [3 3] at 1 ends where the suffix begins; the single draft is the last token itself
    d = _draft([[3, 3, 3, 3]], gram=(2, 2))
    assert d["tokens"].tolist() == [3, 3, 0, 0, 0] and d["n_draft"].tolist() == [1]


def test_no_match_and_short_histories():
    assert _draft([[1, 2, 3, 4, 5, 6]])["n_draft"].tolist() == [0]
    assert _draft([[4]], gram=(1, 4))["tokens"].tolist() == [4, 0, 0, 0, 0]          # n_tok = 1: no g < n
    assert _draft([[4, 4]], gram=(1, 4))["tokens"].tolist() == [4, 4, 0, 0, 0]       # g = 1 at j = 0, one token follows
    assert _draft([[4, 4]], gram=(2, 4))["n_draft"].tolist() == [0]


def test_the_draft_budget():
    rep = [1, 2, 3, 4, 5, 6, 7, 1, 2]  # [1 2] at 0, five drafts on offer
    assert _draft([rep])["n_draft"].tolist() == [4]                                   # K
    assert _draft([rep], limit=[11])["tokens"].tolist() == [2, 3, 0, 0, 0]            # limit - n - 1 = 1
    assert _draft([rep], limit=[10])["n_draft"].tolist() == [0]                       # one token to go: the pending row only
    assert _draft([rep], max_len=11)["tokens"].tolist() == [2, 3, 4, 0, 0]            # max_len - n = 2
    assert _draft([rep], max_len=9)["row0"].tolist() == [0, 1]                        # n_tok = max_len: active, no drafts
    assert _draft([rep], K=0, R=1)["tokens"].tolist() == [2]
    # R: three slots, 3 + 4 drafts in 6 rows: slot 0 keeps 3 (two later slots keep their rows), slot 1 none
    d = _draft([rep, rep, [9]], R=6)
    assert d["row0"].tolist() == [0, 4, 5, 6] and d["n_draft"].tolist() == [3, 0, 0]
    assert d["tokens"].tolist() == [2, 3, 4, 5, 2, 9] and d["row_slot"].tolist() == [0, 0, 0, 0, 1, 2]
    assert d["row_ctr"].tolist() == [8, 9, 10, 11, 8, 0]
    d = _draft([rep, rep, [9]], R=3)
    assert d["row0"].tolist() == [0, 1, 2, 3] and d["tokens"].tolist() == [2, 2, 9]


def test_inactive_slots_have_no_rows():
    rep = [1, 2, 3, 1, 2]
    d = _draft([rep, rep, [], rep, rep], limit=[60, 5, 60, 4, 60], max_len=64, K=2, R=15)
    assert d["seq"].tolist() == [0, -1, -1, -1, 4] and d["row0"].tolist() == [0, 3, 3, 3, 3, 6]
    assert d["pos0"].tolist() == [4, 4, -1, 4, 4] and d["n_draft"].tolist() == [2, 0, 0, 0, 2]
    assert d["tokens"].tolist() == [2, 3, 1, 2, 3, 1] + [0] * 9 and d["row_slot"].tolist() == [0, 0, 0, 4, 4, 4] + [-1] * 9
    assert _draft([rep], max_len=4)["seq"].tolist() == [-1]                           # n_tok > max_len
    assert _draft([rep], ld=5)["seq"].tolist() == [0] and _draft([rep], ld=5)["n_draft"].tolist() == [3]
    h = np.array([rep[:4]], np.int32)                                                 # n_tok > ld_hist
    assert sp.reference_spec_draft(h, [5], [60], 2, 2, 4, 3, 64)["seq"].tolist() == [-1]


def test_external_drafts():
    ext = np.array([[11, 12, 13, 14], [21, 22, -1, 24], [31, 2 ** 30, 33, 34], [41, 42, 43, 44]])
    rows = [[1, 2, 1, 2], [5], [6], [7]]
    d = _draft(rows, ext_draft=ext, ext_n=[3, 4, 4, 0])
    assert d["n_draft"].tolist() == [3, 2, 1, 0] and d["row0"].tolist() == [0, 4, 7, 9, 10]
    assert d["tokens"][:10].tolist() == [2, 11, 12, 13, 5, 21, 22, 6, 31, 7]
    d = _draft(rows, ext_draft=ext, ext_n=[9, -2, 4, 4], limit=[7, 60, 60, 60], max_len=64)
    assert d["n_draft"].tolist() == [2, 0, 1, 4]                                      # d_max = 2 cuts slot 0; ext_n < 0: none


# ---------------------------------------------------------------------------------------------------------------- accept

def _accept(tokens, drawn, row0, n_tok, limit, eos, K=3, seq=None, ld=16, sentinel=-7):
    B = len(n_tok)
    hist = np.full((B, ld), 50, np.int32)
    out0 = np.full((B, K + 1), sentinel, np.int64)
    seq = list(range(B)) if seq is None else seq
    return sp.reference_spec_accept(tokens, drawn, seq, row0, hist, n_tok, limit, eos, K, out_tok=out0)


def test_accept_none_some_all():
    #         slot 0: m = 0        slot 1: m = 2 of 3      slot 2: all 3 + bonus   slot 3: a decode token
    tokens = [10, 11, 12, 13,      20, 21, 22, 23,         30, 31, 32, 33,         40]
    drawn = [99, 12, 13, 14,       21, 22, 77, 24,         31, 32, 33, 34,         41]
    a = _accept(tokens, drawn, [0, 4, 8, 12, 13], [5, 6, 7, 8], [60] * 4, [-1] * 4)
    assert a["n_acc"].tolist() == [0, 2, 3, 0] and a["n_out"].tolist() == [1, 3, 4, 1]
    assert a["out_tok"].tolist() == [[99, -7, -7, -7], [21, 22, 77, -7], [31, 32, 33, 34], [41, -7, -7, -7]]
    assert a["n_tok"].tolist() == [6, 9, 11, 9] and a["limit"].tolist() == [60] * 4
    assert a["hist"][1, 6:9].tolist() == [21, 22, 77] and a["hist"][1, 9] == 50 and a["hist"][2, 7:11].tolist() == [31, 32, 33, 34]
    assert a["n_out"].dtype == np.int32 and a["n_acc"].dtype == np.int32 and a["out_tok"].dtype == np.int64


def test_accept_is_cut_by_limit_and_closed_by_eos():
    tokens = [30, 31, 32, 33] * 3
    drawn = [31, 32, 33, 34] * 3
    a = _accept(tokens, drawn, [0, 4, 8, 12], [7, 7, 7], [9, 60, 60], [-1, 32, 34])
    assert a["n_acc"].tolist() == [3, 3, 3], "n_acc is m before the cut"
    assert a["n_out"].tolist() == [2, 2, 4] and a["n_tok"].tolist() == [9, 9, 11]
    assert a["limit"].tolist() == [9, 9, 11], "an emitted eos closes the slot"
    assert a["out_tok"].tolist() == [[31, 32, -7, -7], [31, 32, -7, -7], [31, 32, 33, 34]]
    assert a["hist"][0, 7:10].tolist() == [31, 32, 50]
    # the eos behind the limit's cut is not emitted: the slot ends by its limit alone
    a = _accept(tokens[:4], drawn[:4], [0, 4], [7], [8], [32])
    assert a["n_out"].tolist() == [1] and a["limit"].tolist() == [8] and a["n_tok"].tolist() == [8]
    # the next draft call sees closed slots as inactive
    d = sp.reference_spec_draft(a["hist"], a["n_tok"], a["limit"], 3, 2, 4, 4, 64)
    assert d["seq"].tolist() == [-1] and d["row0"].tolist() == [0, 0]


def test_accept_leaves_what_does_not_count():
    tokens, drawn = [1, 2, 3, 4, 5, 6], [2, 3, 4, 5, 6, 7]
    for kw in (dict(seq=[-1, 1]), dict(seq=[1, 1]), dict(row0=[0, 0, 6]), dict(row0=[0, 5, 6]), dict(n_tok=[9, 4]), dict(n_tok=[0, 4])):
        args = dict(row0=[0, 3, 6], n_tok=[4, 4], seq=[0, 1])
        args.update(kw)
        a = _accept(tokens, drawn, args["row0"], args["n_tok"], [9, 60], [-1, -1], seq=args["seq"])
        assert a["n_out"][0] == 0 and a["n_acc"][0] == 0 and a["out_tok"][0].tolist() == [-7] * 4, kw
        assert a["n_tok"][0] == args["n_tok"][0] and a["limit"][0] == 9 and (a["hist"][0] == 50).all(), kw
    # a token past the history's end is emitted, not recorded, and the slot is inactive afterwards
    a = _accept(tokens, drawn, [0, 3, 6], [15, 4], [60, 60], [-1, -1])
    assert a["n_out"].tolist() == [3, 3] and a["n_tok"][0] == 18 and a["hist"][0, 15] == 2
    assert sp.reference_spec_draft(a["hist"], a["n_tok"], a["limit"], 3, 2, 4, 8, 64)["seq"].tolist() == [-1, 1]


# ---------------------------------------------------------------------------------------------------- losslessness on a toy model

@pytest.mark.parametrize("K", [1, 4])
def test_the_emitted_stream_is_the_sequential_stream(K):
    """a toy model: the next token is a fixed pseudo-random function of the last three tokens over a vocabulary of 7 (so streams
    repeat and prompt lookup hits).  draft -> one toy draw per row -> accept, for 4 slots: token for token the sequential stream."""
    V, B, new, ld = 7, 4, 120, 160
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
    hist, n_tok = _hist(prompts, ld)
    n_tok, limit, eos = np.array(n_tok), np.array([len(p) + new for p in prompts]), np.full(B, -1)
    R = min(128, B * (K + 1)) - (1 if K == 4 else 0)  # K = 4: 19 rows, so the cut at R takes part
    got, best, steps = [[] for _ in range(B)], 0, 0
    while (n_tok < limit).any():
        d = sp.reference_spec_draft(hist, n_tok, limit, K, 2, 4, R, max_len=ld)
        drawn = np.zeros(R, np.int64)
        for r in range(R):
            b = int(d["row_slot"][r])
            if b < 0:
                continue
            i = r - int(d["row0"][b])
            drawn[r] = nxt(list(hist[b, :n_tok[b]]) + list(d["tokens"][d["row0"][b] + 1:d["row0"][b] + 1 + i]))
        a = sp.reference_spec_accept(d["tokens"], drawn, d["seq"], d["row0"], hist, n_tok, limit, eos, K)
        assert (a["n_acc"] <= d["n_draft"]).all() and (a["n_out"][d["seq"] >= 0] >= 1).all()
        for b in range(B):
            got[b] += a["out_tok"][b, :a["n_out"][b]].tolist()
        hist, n_tok, limit = a["hist"], a["n_tok"], a["limit"]
        best, steps = max(best, int(a["n_acc"].max())), steps + 1
        assert steps <= new
    assert got == want
    assert all(hist[b, :len(p) + new].tolist() == list(p) + want[b] for b, p in enumerate(prompts))
    assert best >= min(K, 2), "no step accepted two drafts: the test shows nothing"
    assert steps < new, "every step emitted one token: the test shows nothing"


# ------------------------------------------------------------------------------------- the two derivations the kernels rest on

def _one_pass_lookup(h, gmin, gmax):
    """csrc/spec.hip's search restated: for every end p + 1 (p in 0 .. n - 2) the length m <= gmax of the common suffix of h[: p + 1]
    and h, and ONE maximum of the key (m, p) over the ends with m >= gmin"""
    n, best = len(h), 0
    for p in range(n - 1):
        m = 0
        while m < gmax and p - m >= 0 and h[p - m] == h[n - 1 - m]:
            m += 1
        if m >= gmin:
            best = max(best, (m << 32) | p)
    return None if best == 0 else (best & 0xFFFFFFFF) + 1


def test_one_pass_lookup_is_the_lookup_by_descending_gram():
    rng = np.random.default_rng(0)
    hits = 0
    for _ in range(3000):
        h = rng.integers(0, int(rng.integers(2, 6)), size=int(rng.integers(1, 60)))
        gmin = int(rng.integers(1, 9))
        gmax = int(rng.integers(gmin, 9))
        want = sp.lookup(h, gmin, gmax)
        assert _one_pass_lookup(h.tolist(), gmin, gmax) == want, (h, gmin, gmax)
        hits += want is not None
    assert 300 < hits < 2700


def test_closed_form_packing_is_the_cut_where_R_is_full():
    """slot b keeps clamp(R - A - D_b, 0, d_b) drafts and starts at row A_b + min(D_b, R - A) (A active slots, A_b of them before b,
    D_b uncut drafts before b): the sequential rule 'every active slot keeps its row, drafts are cut where R is full'"""
    rng = np.random.default_rng(1)
    cuts = 0
    for _ in range(3000):
        B = int(rng.integers(1, 20))
        R = int(rng.integers(B, 40))
        act = rng.random(B) < 0.7
        d = rng.integers(0, 8, size=B) * act
        at, seq = 0, []
        for b in range(B):
            g = min(int(d[b]), max(0, R - at - 1 - int(act[b + 1:].sum()))) if act[b] else 0
            seq.append((at, g))
            at += (1 + g) if act[b] else 0
        E = R - int(act.sum())
        closed = [(int(act[:b].sum()) + min(int(d[:b].sum()), E), min(max(E - int(d[:b].sum()), 0), int(d[b]))) for b in range(B)]
        assert seq == closed, (R, act, d)
        cuts += sum(g for _, g in seq) < int(d.sum())
    assert cuts > 300


# ---------------------------------------------------------------------------------------------------------------- the C-ABI

@pytest.fixture(scope="module")
def lib():
    return qp._native.lib()


def test_spec_symbols_are_exported(lib):
    for name in ("qpal_spec_draft", "qpal_spec_accept"):
        assert name in qp._native.exported_symbols() and hasattr(lib, name)
    for f in (qp.spec_draft, qp.spec_accept, qp.reference_spec_draft, qp.reference_spec_accept, qp.SpeculativeStep):
        assert callable(f)
    assert issubclass(qp.SpeculativeStep, qp.RaggedStep)
    with open(os.path.join(ROOT, "include", "qpal.h")) as f:
        hdr = f.read()
    assert "qpal_spec_draft(" in hdr and "qpal_spec_accept(" in hdr


def _c_draft(lib, hist=16, ld=64, n_tok=16, limit=16, ext=None, ext_n=None, B=4, K=4, gmin=2, gmax=4, R=20, L=64, tokens=16, seq=16,
             row0=16, pos0=16, row_slot=16, row_ctr=16, n_draft=16):
    return lib.qpal_spec_draft(hist, ld, n_tok, limit, ext, ext_n, B, K, gmin, gmax, R, L, tokens, seq, row0, pos0, row_slot, row_ctr,
                               n_draft, None)


def _c_accept(lib, tokens=16, drawn=16, seq=16, row0=16, hist=16, ld=64, n_tok=16, limit=16, eos=16, B=4, K=4, R=20, out_tok=16, n_out=16,
              n_acc=16):
    return lib.qpal_spec_accept(tokens, drawn, seq, row0, hist, ld, n_tok, limit, eos, B, K, R, out_tok, n_out, n_acc, None)


def test_spec_argument_errors_without_a_gpu(lib):
    """every argument error is returned before any stream work: the pointers below are never dereferenced"""
    for name in ("hist", "n_tok", "limit", "tokens", "seq", "row0", "pos0", "row_slot", "row_ctr", "n_draft"):
        assert _c_draft(lib, **{name: None}) == E_NULL, name
    assert _c_draft(lib, ext=16, ext_n=None) == E_NULL
    for kw in ({"B": 0}, {"B": 129, "R": 129}, {"K": -1}, {"K": 16}, {"gmin": 0}, {"gmax": 9}, {"gmin": 4, "gmax": 3}, {"R": 3}, {"R": 129},
               {"L": 0}, {"ld": 0}, {"ld": 1 << 31}):
        assert _c_draft(lib, **kw) == E_SHAPE, kw
    for kw in ({"hist": 18}, {"n_tok": 20}, {"limit": 20}, {"tokens": 20}, {"seq": 18}, {"row0": 17}, {"pos0": 20}, {"row_slot": 18},
               {"row_ctr": 20}, {"n_draft": 17}, {"ext": 20, "ext_n": 16}, {"ext": 16, "ext_n": 18}):
        assert _c_draft(lib, **kw) == E_ALIGN, kw
    for name in ("tokens", "drawn", "seq", "row0", "hist", "n_tok", "limit", "eos", "out_tok", "n_out", "n_acc"):
        assert _c_accept(lib, **{name: None}) == E_NULL, name
    for kw in ({"B": 0}, {"B": 129, "R": 129}, {"K": -1}, {"K": 16}, {"R": 3}, {"R": 129}, {"ld": 0}):
        assert _c_accept(lib, **kw) == E_SHAPE, kw
    for kw in ({"tokens": 20}, {"drawn": 20}, {"seq": 18}, {"row0": 17}, {"hist": 18}, {"n_tok": 20}, {"limit": 20}, {"eos": 20},
               {"out_tok": 20}, {"n_out": 18}, {"n_acc": 17}):
        assert _c_accept(lib, **kw) == E_ALIGN, kw


def test_spec_wrappers_check_their_arguments_before_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(qp._native, "lib", no_library)
    z, i32, i64 = torch.zeros, torch.int32, torch.int64
    B, R, K = 3, 8, 4
    good = dict(hist=z(B, 32, dtype=i32), n_tok=z(B, dtype=i64), limit=z(B, dtype=i64), K=K, gram=(2, 4), max_len=64,
                tokens=z(R, dtype=i64), seq=z(B, dtype=i32), row0=z(B + 1, dtype=i32), pos0=z(B, dtype=i64), row_slot=z(R, dtype=i32),
                row_ctr=z(R, dtype=i64), n_draft=z(B, dtype=i32))
    bad = [({"hist": z(B, 32, dtype=i64)}, "hist"), ({"hist": z(B, 64, dtype=i32)[:, ::2]}, "hist"), ({"hist": z(129, 4, dtype=i32)}, "slots"),
           ({"n_tok": z(B, dtype=i32)}, "n_tok"), ({"limit": z(B + 1, dtype=i64)}, "limit"), ({"K": 16}, "K must"), ({"K": -1}, "K must"),
           ({"gram": (0, 4)}, "gmin"), ({"gram": (3, 2)}, "gmin"), ({"gram": (2, 9)}, "gmin"), ({"max_len": 0}, "max_len"),
           ({"tokens": z(2, dtype=i64)}, "tokens"), ({"tokens": z(129, dtype=i64)}, "tokens"), ({"tokens": z(R, dtype=i32)}, "tokens"),
           ({"seq": z(B, dtype=i64)}, "seq"), ({"row0": z(B, dtype=i32)}, "row0"), ({"pos0": z(B, dtype=i32)}, "pos0"),
           ({"row_slot": z(R - 1, dtype=i32)}, "row_slot"), ({"row_ctr": z(2 * R, dtype=i64)[::2]}, "row_ctr"),
           ({"n_draft": z(B, dtype=i64)}, "n_draft"), ({"n_draft": z(B, dtype=i32, device="meta")}, "n_draft must be on"),
           ({"ext_draft": z(B, K, dtype=i64)}, "ext_n"), ({"ext_draft": z(B, K + 1, dtype=i64), "ext_n": z(B, dtype=i32)}, "ext_draft"),
           ({"ext_draft": z(B, K, dtype=i64), "ext_n": z(B, dtype=i64)}, "ext_n")]
    for kw, what in bad:
        with pytest.raises(qp._native.QpalError, match=what):
            qp.spec_draft(**{**good, **kw})
    with pytest.raises(qp._native.QpalError, match="GPU"):  # good arguments on the host: still before the library
        qp.spec_draft(**good)
    agood = dict(tokens=z(R, dtype=i64), drawn=z(R, dtype=i64), seq=z(B, dtype=i32), row0=z(B + 1, dtype=i32), hist=z(B, 32, dtype=i32),
                 n_tok=z(B, dtype=i64), limit=z(B, dtype=i64), eos=z(B, dtype=i64), out_tok=z(B, K + 1, dtype=i64), n_out=z(B, dtype=i32),
                 n_acc=z(B, dtype=i32))
    abad = [({"drawn": z(R + 1, dtype=i64)}, "drawn"), ({"drawn": z(R, dtype=i32)}, "drawn"), ({"eos": z(B, dtype=i32)}, "eos"),
            ({"out_tok": z(B, 17, dtype=i64)}, "out_tok"), ({"out_tok": z(B + 1, K + 1, dtype=i64)}, "out_tok"),
            ({"out_tok": z(B, K + 1, dtype=i32)}, "out_tok"), ({"n_out": z(B, dtype=i64)}, "n_out"), ({"n_acc": z(1, dtype=i32)}, "n_acc"),
            ({"hist": z(B, 32, dtype=torch.int16)}, "hist"), ({"seq": z(B + 1, dtype=i32)}, "seq"),
            ({"tokens": z(B - 1, dtype=i64)}, "tokens"), ({"limit": z(B, dtype=i64, device="meta")}, "limit must be on")]
    for kw, what in abad:
        with pytest.raises(qp._native.QpalError, match=what):
            qp.spec_accept(**{**agood, **kw})
    with pytest.raises(qp._native.QpalError, match="GPU"):
        qp.spec_accept(**agood)
