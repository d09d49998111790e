"""CPU checks of the sliding-window contract: tests/window_reference.py is what it says it is, its kappa comes from
the emulation over the windowed cases the GPU tests use, every seeded window defect lands >= 4x outside the tolerance at those sizes,
the census is blind to a window shifted by hd keys and the needles close that, PagedKVCache.trim, every new QpalError (raised before
the library is reached) and the new entry points' return codes."""
import math

import numpy as np
import pytest
import torch

import attn_reference as ar
import qpalette_amd as qp
import window_reference as wr
from attn_reference import F8, F16
from qpalette_amd._native import QpalError
from test_attn_exact import DTYPES, SHAPES, TEETH, _cpu_rows, _id
from test_window import PF_CASES, SHORT_W

CPU = torch.device("cpu")
LONG_W = (5, 100, 512, 516, 1000, 2044)


def _case(family, shape, L, dtype, pos, W, seed=5, needle_at=None):
    """(q16, K, V) on the CPU: rows at positions `pos` (consecutive) whose window keys carry `family`, in the cache format"""
    nq, nkv, hd = shape
    q16 = _cpu_rows(family, shape, pos, seed)
    K, V = wr.window_cache(family, q16, nq, nkv, hd, L, wr.lo(pos[0], W), pos[-1] + 1, 1.0 / math.sqrt(hd), seed + 10, needle_at=needle_at)
    return q16, ar.to_cache(K, dtype), ar.to_cache(V, dtype)


# ------------------------------------------------------------------------------------------------------------ the reference

@pytest.mark.parametrize("W", [1, 5, 33, 100, None])
def test_masked_is_the_sliced_definition(W):
    """the many-rows form the GPU tests call against attention_fp64 on each row's own slice K[:, lo:n], V[:, lo:n]"""
    shape = nq, nkv, hd = (8, 2, 64)
    pos = list(range(90, 123))
    q16, K, V = _case("peaked", shape, 128, F16, pos, W)
    scale = 1.0 / math.sqrt(hd)
    for a, b in zip(wr.masked(q16, K, V, pos, W, nq, nkv, hd, scale), wr.sliced(ar.attention_fp64, q16, K, V, pos, W, nq, nkv, hd, scale)):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


def test_lo_and_window_floor_agree():
    pos = np.arange(-1, 300)
    for W in (1, 2, 5, 64, 299, 300, 1000):
        want = np.array([wr.lo(p, W) if p >= 0 else 0 for p in pos])
        assert np.array_equal(qp.window_floor(pos, W), want)
        assert torch.equal(qp.window_floor(torch.from_numpy(pos), W), torch.from_numpy(want))
        assert all(qp.window_floor(int(p), W) == w for p, w in zip(pos, want))
    assert qp.window_floor(7, None) == 0 and not qp.window_floor(pos, None).any() and not bool(qp.window_floor(torch.from_numpy(pos), None).any())


def test_census_expectation_is_the_references():
    nq, nkv, hd = 2, 2, 64
    K, V = ar.census_cache(nkv, 600, hd, F16, CPU)
    q16 = torch.ones(40, nq * hd, dtype=F16)
    for W in (1, 5, 64, 100, 516):
        pos = list(range(540, 580))
        exp, tol = wr.census_expected(pos, W, nq, hd, CPU)
        got = wr.masked(q16, K, V, pos, W, nq, nkv, hd, 0.125)[0]
        assert bool(((got - exp).abs() <= tol).all()), W


# -------------------------------------------------------------------------------------------------------------------- kappa

def _decode_cases():
    """the windowed decode cases of test_window.py::test_decode_families_within_the_bound"""
    for L in (256, 2048):
        for W in (33, 516):
            plain = [p for p in (W - 2, W - 1, W + 7, L // 2, L - 1) if 0 <= p < L]
            for family in ar.FAMILIES:
                if family == "needle":
                    yield from ((family, L, W, p, at) for p in (min(W + 7, L - 1), L - 1) for at in (wr.lo(p, W), p))
                else:
                    yield from ((family, L, W, p, None) for p in plain)


def _ratios(q16, K, V, pos, W, shape, u_p):
    """(err / weight term in front of the output rounding, err / whole bound after it) of the emulation against float64.  The first
    is kappa's share and is taken where the weight term is at least 2^-24, the bound's absolute floor: below it (a window of a
    few e4m3 values that are all zero or subnormal, |out| < 1e-6) the floor is the tolerance, it also covers a softmax weight that
    lands in fp16's subnormals, and the second figure checks those elements."""
    nq, nkv, hd = shape
    scale = 1.0 / math.sqrt(hd)
    ref, A, Smax = wr.sliced(ar.attention_fp64, q16, K, V, pos, W, nq, nkv, hd, scale)
    raw = wr.sliced(ar.emulate, q16, K, V, pos, W, nq, nkv, hd, scale, u_p, rounded=False).double()
    emu = wr.sliced(ar.emulate, q16, K, V, pos, W, nq, nkv, hd, scale, u_p).double()
    wt = ar.weight_term(A, Smax, u_p)
    share = ((raw - ref).abs() / wt)[wt >= 2.0 ** -24]
    return float(share.max()) if share.numel() else 0.0, float(((emu - ref).abs() / wr.bound(ref, A, Smax, u_p)).max())


def test_emulation_sits_inside_the_windowed_bound():
    """kappa per u_p: four times the worst ratio of the emulation over the windowed cases of the GPU tests, rounded up to a power of
    two (window_reference.KAPPA; the table goes into that file's header and DESIGN.md §31)"""
    worst, whole = {}, 0.0
    for i, (family, L, W, p, at) in enumerate(_decode_cases()):
        for shape in SHAPES:
            for dtype in DTYPES:
                r1, r = _ratios(*_case(family, shape, L, dtype, [p], W, needle_at=at), [p], W, shape, 0.0)
                worst[(family, False)] = max(worst.get((family, False), 0.0), r1)
                whole = max(whole, r)
    for shape, T, W, pos0, L, dtype in PF_CASES:
        rows = sorted({0, T // 2, T - 1})
        for family in ar.FAMILIES:
            for t in rows:  # (the emulation is per row: a sample of the chunk's rows)
                at = wr.lo(pos0 + t, W) if family == "needle" else None
                q16, K, V = _case(family, shape, L, dtype, list(range(pos0, pos0 + T)), W, needle_at=at)
                r1, r = _ratios(q16[t:t + 1], K, V, [pos0 + t], W, shape, wr.U_PREFILL)
                worst[(family, True)] = max(worst.get((family, True), 0.0), r1)
                whole = max(whole, r)
    print("windowed emulation err / weight term at kappa = 1, worst per (family, u_p > 0):")
    for key, r1 in sorted(worst.items()):
        print(f"  {key[0]:10s} u_p={'2^-11' if key[1] else '0':6s} {r1:.3f}")
    print(f"worst err / whole tolerance: {whole:.3f}")
    assert whole <= 1.0
    for pre in (False, True):
        top = max(r for (f, u), r in worst.items() if u == pre)
        assert 4.0 * top <= wr.KAPPA[pre] < 16.0 * top, (pre, top, wr.KAPPA[pre])  # the 4x margin holds, and kappa is no looser than the rule gives


# -------------------------------------------------------------------------------------------------------------------- teeth

def _census_excess(pos, W, hd, mutate, L=None):
    nq = nkv = 2
    K, V = ar.census_cache(nkv, (L or max(pos) + 1), hd, F16, CPU)
    q16 = torch.ones(len(pos), nq * hd, dtype=F16)
    exp, tol = wr.census_expected(pos, W, nq, hd, CPU)
    got = wr.masked(q16, K, V, pos, W, nq, nkv, hd, 0.125, mutate=mutate)[0]
    return ((got - exp).abs() / tol).amax(dim=1)


@pytest.mark.parametrize("hd", [64, 128, 256])
def test_census_catches_a_window_one_key_off_and_a_tile_granular_edge(hd):
    for W in sorted(set(SHORT_W) | set(LONG_W)):
        for p in (W + 2, W + 37, W + 1037):  # lo = 3, 38, 1038: off every multiple of 32 and 64
            l = wr.lo(p, W)
            assert l % 32 and l % 64
            cases = [("wide",), ("tile", 32), ("tile", 64)] + ([("narrow",)] if W > 1 else [])
            for mutate in cases:
                worst = float(_census_excess([p], W, hd, mutate)[0])
                assert worst >= TEETH, (W, p, hd, mutate, worst)
    assert float(_census_excess([100], 2048, 64, ("wide",))[0]) == 0.0  # (lo = 0: nothing below to admit)


@pytest.mark.parametrize("shape,T,W,pos0,L,dtype", [c for c in PF_CASES if c[1] > 1 and c[3] >= c[2]][::3], ids=_id)
def test_census_catches_the_first_rows_edge_for_every_row(shape, T, W, pos0, L, dtype):
    """lo taken from the tile's first row: row t admits t keys too many (row 0 none).  Where W and t are both multiples of hd the t
    extra keys add every residue equally and the census cannot see them (the blindness of the test below): rows t = hd, 2 hd."""
    hd = shape[2]
    per_row = _census_excess(list(range(pos0, pos0 + T)), W, hd, ("first_row_lo",), L)
    seen = [float(r) for t, r in enumerate(per_row) if t % hd]
    assert float(per_row[0]) == 0.0 and min(seen) >= TEETH, per_row.tolist()


def test_census_catches_a_window_applied_in_the_last_chunk_only():
    """the split prefill cases (L = 2048, span >= 512, chunks of 128 keys and more): every row whose lo lies above the first chunk
    gains that chunk's keys"""
    for T, W, pos0 in ((128, 516, 1500), (128, 516, 1920), (64, 1000, 1800)):
        for chunk in (128, 256):
            per_row = _census_excess(list(range(pos0, pos0 + T)), W, 64, ("last_chunk_only", chunk), 2048)
            assert float(per_row.max()) >= TEETH and float((per_row >= TEETH).float().mean()) > 0.5, (T, W, pos0, chunk)


def test_census_is_blind_to_a_shift_by_hd_and_the_needles_are_not():
    """a window moved down by exactly hd keys counts the same residues: 0 ulp, against 31 ulp and more for one key too wide or too
    narrow at W <= 2048 and hd 64.  Needles at lo - 1 (must be invisible) and pos (must be seen) see the shift; the needle at lo
    sees the narrow window, the one at lo - 1 the wide one."""
    hd = 64
    for W in (100, 516, 2044):
        p = W + 100
        assert float(_census_excess([p], W, hd, ("shift", hd))[0]) == 0.0
        assert float(_census_excess([p], W, hd, ("wide",))[0]) >= 31.0 and float(_census_excess([p], W, hd, ("narrow",))[0]) >= 31.0
    shape = nq, nkv, _ = (8, 1, 64)
    scale = 1.0 / math.sqrt(hd)
    for W, p in ((100, 200), (516, 1500)):
        l = wr.lo(p, W)
        seen = {}
        for at in (l - 1, l, p):
            q16, K, V = _case("needle", shape, 2048, F16, [p], W, needle_at=at)
            ref, A, Smax = wr.masked(q16, K, V, [p], W, nq, nkv, hd, scale)
            for mutate in (("shift", hd), ("wide",), ("narrow",)):
                got = wr.masked(q16, K, V, [p], W, nq, nkv, hd, scale, mutate=mutate)[0]
                seen[(at - l, mutate[0])] = float(((got - ref).abs() / wr.bound(ref, A, Smax, 0.0)).max())
        assert seen[(-1, "shift")] >= TEETH and seen[(p - l, "shift")] >= TEETH, seen
        assert seen[(-1, "wide")] >= TEETH and seen[(0, "narrow")] >= TEETH, seen


# ----------------------------------------------------------------------------------------------------------------- trim

def _cache(B=3, pages=24, page=16, max_pages=8, **kw):
    return qp.PagedKVCache(2, pages, 2, page, 64, B, max_pages, **kw)


def test_trim_frees_whole_pages_below_and_keeps_the_length():
    c = _cache()
    c.reserve(0, 100)                                   # 7 pages: 0 .. 6
    assert c.pages_of(0) == list(range(7)) and c.pages_free == 17
    c.trim(0, 47)                                       # pages 0, 1 lie wholly below 47; page 2 holds 32 .. 47
    assert c.pages_of(0) == [-1, -1, 2, 3, 4, 5, 6] and c.pages_free == 19 and c.trimmed_upto(0) == 32 and c.pages_held(0) == 5
    assert c.table[0].tolist() == [-1, -1, 2, 3, 4, 5, 6, -1]
    assert c.refcount(0) == 0 and c.refcount(1) == 0 and c.refcount(2) == 1
    before = (c.pages_of(0), c.pages_free)
    c.trim(0, 20), c.trim(0, 47), c.trim(0, 0), c.trim(0, -5)   # smaller or equal: nothing
    assert (c.pages_of(0), c.pages_free) == before
    c.reserve(0, 100)                                   # counts positions from 0: nothing to add, nothing re-backed
    assert (c.pages_of(0), c.pages_free) == before
    c.reserve(0, 128)
    assert c.pages_of(0)[:2] == [-1, -1] and len(c.pages_of(0)) == 8 and c.pages_of(0)[7] in (0, 1) and c.pages_free == 18
    c.trim(0, 10 ** 6)                                  # past the end: everything reserved goes, nothing more
    assert c.pages_held(0) == 0 and c.pages_free == 24 and c.trimmed_upto(0) == 128
    c.release(0)
    assert c.pages_free == 24 and c.pages_of(0) == [] and c.trimmed_upto(0) == 0 and sorted(c._free) == list(range(24))
    c.reserve(0, 16)
    assert c.pages_held(0) == 1 and c.table[0, 0] >= 0
    with pytest.raises(QpalError):
        c.trim(5, 16)


def test_trim_fork_and_groups():
    c = _cache(B=4, pages=32, min_len=32, min_members=2)
    c.reserve(0, 80)
    c.fork(0, 1, 70)                                    # pages 0 .. 3 shared, the partial page copied; a group of 64 positions
    c.fork(0, 2, 70)
    g = c.group_of(0)
    assert g >= 0 and c.members_of(g) == [0, 1, 2] and c.refcount(0) == 3
    c.trim(1, 40)                                       # slot 1 drops its references on pages 0, 1 and leaves the group
    assert c.refcount(0) == 2 and c.refcount(1) == 2 and c.pages_free == 32 - 7 and c.group_of(1) == -1 and c.members_of(g) == [0, 2]
    assert c.prefix.row_group.tolist()[:3] == [g, -1, g]
    with pytest.raises(QpalError):
        c.fork(1, 3, 16)                                # from below a trimmed position
    c.fork(1, 3, 0)                                     # nothing shared: allowed
    c.trim(0, 40)                                       # the group falls below two members and dissolves
    assert c.group_of(0) == -1 and c.group_of(2) == -1 and c.members_of(g) == [] and c.refcount(0) == 1
    c.trim(2, 40)
    assert c.refcount(0) == 0 and c.refcount(1) == 0 and c.pages_free == 32 - 5
    for s in range(4):
        c.release(s)
    assert c.pages_free == 32 and all(c.refcount(p) == 0 for p in range(32))


# ------------------------------------------------------------------------------------------------- errors and return codes

def test_every_new_error_is_raised_before_the_library_is_reached(monkeypatch):
    def no_lib():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(qp._native, "lib", no_lib)
    x = None
    launches = [lambda w: qp.decode_attention(x, x, x, x, x, x, x, window=w),
                lambda w: qp.prefill_attention(x, x, x, x, x, x, x, window=w),
                lambda w: qp.paged_decode_attention(x, x, x, x, x, x, x, x, window=w),
                lambda w: qp.paged_prefill_attention(x, x, x, x, x, x, x, x, window=w),
                lambda w: qp.ragged_prefill_attention(x, x, x, x, x, x, x, x, x, window=w),
                lambda w: qp.paged_ragged_prefill_attention(x, x, x, x, x, x, x, x, x, x, window=w),
                lambda w: qp.window_floor(3, w),
                lambda w: qp.decoder._Rows._check_window("DecodeStep", w, 2),
                lambda w: qp.decoder._Rows._check_window("DecodeStep", (4, w), 2)]
    for launch in launches:
        for bad in (0, -1, 1.5, True, "8"):
            with pytest.raises(QpalError, match="window"):
                launch(bad)
    for w in (1, 4096):
        with pytest.raises(QpalError, match="shared-prefix"):
            qp.shared_prefix_decode_attention(x, x, x, x, x, x, x, x, x, window=w)
    for bad in ((4,), (4, 4, 4), [None], "44"):
        with pytest.raises(QpalError, match="window"):
            qp.decoder._Rows._check_window("Prefill", bad, 2)
    assert qp.decoder._Rows._check_window("Prefill", None, 2) == [None, None]
    assert qp.decoder._Rows._check_window("Prefill", 8, 3) == [8, 8, 8] and qp.decoder._Rows._check_window("Prefill", (None, 8), 2) == [None, 8]
    tok = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(QpalError, match="shared_prefix with window"):
        qp.DecodeStep([x, x], x, x, x, x, x, x, tok, tok, tok, block_table=torch.zeros(2, 4, dtype=torch.int32), shared_prefix=object(),
                      window=(None, 8))


def test_window_entry_points_return_codes():
    lib = qp._native.lib()
    buf = np.zeros(1 << 16, dtype=np.uint8)
    p = buf.ctypes.data
    dec = lambda q, table, window, L=128, fmt=0: lib.qpal_attn_rope_decode_batch_window(  # noqa: E731
        q, p, p, 512, p, p, p, 512, p, p, table, 8, 4, 16, 8, fmt, 1, 8, 8, 64, L, 0.125, window, None, 0, None)
    pre = lambda q, row, window, L=128, fmt=0: lib.qpal_attn_rope_prefill_window(  # noqa: E731
        q, p, p, 512, p, p, p, 512, p, p, row, 4, 16, 8, fmt, 1, 8, 8, 64, L, 0.125, window, None, 0, None)
    rag = lambda q, table, window, L=128, fmt=0: lib.qpal_attn_rope_prefill_ragged_window(  # noqa: E731
        q, p, p, 512, p, p, p, 512, p, p, p, p, table, 8, 4, 16, 8, fmt, 1, 1, 1, 8, 8, 64, L, 0.125, window, None, 0, None)
    for fn in (dec, pre, rag):
        for table in (None, p):
            assert fn(None, table, 4) == -3 and fn(None, table, -1) == -3     # a null pointer: QPAL_E_NULL, first
            assert fn(p, table, -1) == -2 and fn(p, table, -(1 << 40)) == -2  # a bad window: QPAL_E_PARAM, before any other check
            assert fn(p, table, -1, L=130, fmt=7) == -2
            assert fn(p, table, 4, fmt=2) == -1                               # then the siblings' checks
            assert fn(p, table, 0, fmt=2) == -1
        assert fn(p, None, 4, L=130) == -1 and fn(p, None, 0, L=130) == -1    # max_len % 4 (contiguous)
