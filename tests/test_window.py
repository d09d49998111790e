"""Sliding-window attention on the GPU: batched decode, prefill and ragged prefill with window=, fp16 and e4m3
caches, contiguous and paged, against tests/window_reference.py — census (the output counts the keys of the window), input families
inside the float64 bound with needles on both sides of the lower edge, NaN in every cache row below the floor, and the bit-for-bit
rules of the contract: a full-width window is the launch without one (rule 1), the decode launch is the plain launch's arithmetic on
the window's keys (rule 3), paged = contiguous and a ragged segment = the one-sequence launch (rule 4), the append does not change
(rule 5)."""
import math

import pytest
import torch

import attn_reference as ar
import qpalette_amd as qp
import window_reference as wr
from attn_reference import F8, F16
from test_attn_exact import DTYPES, RAGGED_SEGMENTS, SHAPES, _id, _qkv, _ragged_pos0, _rotated_q, _stack

U_PREFILL = wr.U_PREFILL
_WORST = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _report(kernels, family, worst, what):
    key = (kernels, family)
    _WORST[key] = max(_WORST.get(key, 0.0), worst)
    print(f"{kernels} {family} {what}: worst err/tol = {worst:.3f} (so far over {kernels} {family}: {_WORST[key]:.3f})")
    assert worst <= 1.0, (kernels, family, what, worst)


def _bits(t):
    return t.view(torch.uint8) if t.dtype == F8 else t.view(torch.int16)


def _nan_mask(c, mask):
    """NaN into the rows mask [B, L] (or [L]) of caches [B, nkv, L, hd] ([nkv, L, hd]) of either format"""
    m = mask[:, None, :, None] if mask.dim() == 2 else mask[None, :, None]
    if c.dtype == F16:
        c.masked_fill_(m, float("nan"))
    else:
        c.view(torch.uint8).masked_fill_(m, 0x7F)


class WProblem:
    """ONE sequence under window W: T new rows at positions pos0 .. on a cache [nkv, L, hd] whose keys lo(pos0) .. pos0 + T - 1 carry
    `family` (window_reference.window_cache; census: attn_reference's census cache).  NaN in the rows the launch writes, in the rows
    behind them (census keeps its pattern there) and in EVERY row below lo(pos0): nothing there may be read."""

    def __init__(self, dev, shape, L, dtype, family, pos0, T, W, seed, needle_at=None, nan_below=True):
        nq, nkv, hd = shape
        self.shape, self.L, self.family, self.pos0, self.T, self.W, self.dev = shape, L, family, pos0, T, W, dev
        self.scale, self.inv = 1.0 / math.sqrt(hd), ar.inv_freq(hd, dev)
        self.pos = list(range(pos0, pos0 + T))
        self.first = wr.lo(pos0, W)
        pos = torch.arange(pos0, pos0 + T, device=dev)
        if family == "census":
            self.q32 = ar.query_targets(T, nq, nkv, hd, seed, dev)
            self.k32 = torch.zeros(T, nkv * hd, device=dev)
            self.v32 = ar.census_new_v(pos, nkv, hd, dev)
            self.q16 = None
            self.kc, self.vc = ar.census_cache(nkv, L, hd, dtype, dev)
            behind = slice(pos0, pos0 + T)
        else:
            tgt = ar.query_targets(T, nq, nkv, hd, seed, dev, family).view(T, nq, hd)
            self.q32 = ar.unrope(tgt, pos[:, None], self.inv).reshape(T, nq * hd)
            self.q16 = _rotated_q(self.q32, self.pos, shape, dev)
            K, V = wr.window_cache(family, self.q16, nq, nkv, hd, L, self.first, pos0 + T, self.scale, seed + 7, needle_at=needle_at)
            self.k32 = ar.unrope(K[:, pos0:pos0 + T].transpose(0, 1), pos[:, None], self.inv).reshape(T, nkv * hd)
            self.v32 = V[:, pos0:pos0 + T].transpose(0, 1).reshape(T, nkv * hd).contiguous()
            self.kc, self.vc = ar.to_cache(K, dtype), ar.to_cache(V, dtype)
            behind = slice(pos0, L)
        for c in (self.kc, self.vc):
            ar.nan_rows(c, behind)
            if nan_below:
                ar.nan_rows(c, slice(0, self.first))

    def worst(self, out, u_p, kc=None, vc=None):
        nq, nkv, hd = self.shape
        out = out.double()
        if self.family == "census":
            exp, tol = wr.census_expected(self.pos, self.W, nq, hd, self.dev)
        else:
            exp, A, Smax = wr.masked(self.q16, self.kc if kc is None else kc, self.vc if vc is None else vc, self.pos, self.W, nq, nkv, hd,
                                     self.scale)
            tol = wr.bound(exp, A, Smax, u_p)
        return float(torch.nan_to_num((out - exp).abs() / tol, nan=float("inf")).max())


# ------------------------------------------------------------------------------------------------------------- batched decode

def _census_decode(dev, shape, L, dtype, B, positions, W, what):
    """census through decode_attention(window=W): `positions` in launches of B sequences (the last padded with inactive slots); NaN
    in every row below lo(pos[b]) and in the row the launch writes"""
    nq, nkv, hd = shape
    K1, V1 = ar.census_cache(nkv, L, hd, dtype, dev)
    ws = qp.attention_workspace(B, nq, nkv, hd, L, dev)
    inv = ar.inv_freq(hd, dev)
    q = ar.query_targets(B, nq, nkv, hd, 3, dev)
    k = torch.zeros(B, nkv * hd, device=dev)
    j = torch.arange(L, device=dev)[None, :]
    outs = []
    for i in range(0, len(positions), B):
        pos = positions[i:i + B] + [-1] * (i + B - len(positions))
        pos_t = torch.tensor(pos, dtype=torch.long, device=dev)
        kc, vc = _stack([K1] * B), _stack([V1] * B)
        low = qp.window_floor(pos_t, W)
        mask = ((j < low[:, None]) | (j == pos_t[:, None])) & (pos_t >= 0)[:, None]
        _nan_mask(kc, mask)
        _nan_mask(vc, mask)
        out = torch.full((B, nq * hd), float("nan"), dtype=F16, device=dev)
        qp.decode_attention(*_qkv(q, k, ar.census_new_v(pos_t, nkv, hd, dev)), kc, vc, pos_t, inv, out=out, ws=ws, window=W)
        act = pos_t >= 0
        outs.append(out[act])
        # the row at pos was written: v as the census has it, k as +-0; nothing else changed
        ref_v = _stack([V1] * B)
        _nan_mask(ref_v, mask & (j != pos_t[:, None]))
        assert torch.equal(_bits(vc), _bits(ref_v)), what
        sel = (j == pos_t[:, None]) & act[:, None]
        assert not bool((kc.view(torch.uint8).transpose(1, 2)[sel] & 0x7F).any()), what
    exp, tol = wr.census_expected(positions, W, nq, hd, dev)
    r = (torch.cat(outs).double() - exp).abs() / tol
    _report("decode_attention", "census", float(torch.nan_to_num(r, nan=float("inf")).max()), what)


SHORT_W = [1, 2, 5, 16, 33, 64, 100, 128, 255, 256, 300]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_decode_census_short_cache_every_position(dev, shape, dtype):
    for W in SHORT_W:
        _census_decode(dev, shape, 256, dtype, 128, list(range(256)), W, f"{_id(shape)} {_id(dtype)} L=256 B=128 W={W}")


def _long_positions(L, W):
    """W-2 .. W+1, L-1, and every p where p or lo(p) is within 1 of a multiple of 64; at most 120, spread evenly"""
    near = lambda x: x % 64 in (0, 1, 63)  # noqa: E731
    must = sorted({p for p in (W - 2, W - 1, W, W + 1, L - 1) if 0 <= p < L})
    rest = [p for p in range(L) if p not in must and (near(p) or near(wr.lo(p, W)))]
    keep = 120 - len(must)
    if len(rest) > keep:
        rest = [rest[i * len(rest) // keep] for i in range(keep)]
    return sorted(must + rest)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_decode_census_long_cache(dev, shape, dtype):
    L = 2048
    for W in (5, 100, 512, 516, 1000, 2044):
        positions = _long_positions(L, W)
        assert len(positions) <= 120 and {W - 1, W, L - 1} <= set(positions)
        _census_decode(dev, shape, L, dtype, 4, positions, W, f"{_id(shape)} {_id(dtype)} L={L} B=4 W={W}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_decode_census_where_the_lds_forces_the_split(dev, dtype):
    """(64, 8, 128) at W = 3000: one chunk's scores hold 2944 positions, so the window itself is cut in two and merged"""
    L, W = 4096, 3000
    positions = [2942, 2943, 2944, 2945, 2998, 2999, 3000, 3001, 3063, 3064, 3065, 4031, 4032, 4033, 4094, 4095] + list(range(3100, 4000, 57))
    _census_decode(dev, (64, 8, 128), L, dtype, 32, positions[:32], W, f"64x8x128 {_id(dtype)} L={L} B=32 W={W}")


def _decode_launch(dev, shape, L, problems, W, **kw):
    nq, nkv, hd = shape
    B = len(problems)
    kc, vc = _stack([p.kc for p in problems]), _stack([p.vc for p in problems])
    q, k, v = _qkv(*(torch.cat([getattr(p, a) for p in problems]) for a in ("q32", "k32", "v32")))
    pos_t = torch.tensor([p.pos0 for p in problems], dtype=torch.long, device=dev)
    out = torch.full((B, nq * hd), float("nan"), dtype=F16, device=dev)
    qp.decode_attention(q, k, v, kc, vc, pos_t, kw.pop("inv", problems[0].inv), out=out, ws=qp.attention_workspace(B, nq, nkv, hd, L, dev),
                        window=W, **kw)
    torch.cuda.synchronize()
    return out, kc, vc


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("L", [256, 2048])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_decode_families_within_the_bound(dev, shape, L, dtype):
    """every family over the WINDOW's keys; needles at lo - 1 (outside: must not be seen), lo and pos (must be seen)"""
    for W in (33, 516):
        plain = [p for p in (W - 2, W - 1, W + 7, L // 2, L - 1) if 0 <= p < L]
        for family in ar.FAMILIES:
            if family == "needle":
                cases = [(p, at) for p in (min(W + 7, L - 1), L - 1) for at in (wr.lo(p, W) - 1, wr.lo(p, W), p) if at >= 0]
            else:
                cases = [(p, None) for p in plain]
            probs = [WProblem(dev, shape, L, dtype, family, p, 1, W, 100 + i, needle_at=at) for i, (p, at) in enumerate(cases)]
            out, kc, vc = _decode_launch(dev, shape, L, probs, W)
            worst = max(p.worst(out[b:b + 1], 0.0, kc[b], vc[b]) for b, p in enumerate(probs))
            _report("decode_attention", family, worst, f"{_id(shape)} {_id(dtype)} L={L} W={W}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("L", [256, 2048])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_decode_full_width_window_is_the_plain_launch(dev, shape, L, dtype):
    """rule 1: W = L and W = 4 L, bit for bit in the output and the cache bytes"""
    positions = [0, 1, 63, 64, L // 2 - 1, L // 2, L - 2, L - 1]
    probs = [WProblem(dev, shape, L, dtype, "peaked", p, 1, None, 200 + i) for i, p in enumerate(positions)]
    ref = _decode_launch(dev, shape, L, probs, None)
    assert not bool(torch.isnan(ref[0]).any())
    for W in (L, 4 * L):
        got = _decode_launch(dev, shape, L, probs, W)
        for a, b in zip(ref, got):
            assert torch.equal(_bits(a), _bits(b)), (W, _id(shape))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("L,W,pos", [(2048, 512, 1500), (2048, 1024, 2047), (256, 64, 200), (2048, 516, 300), (256, 100, 50)])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_decode_is_the_plain_arithmetic_on_the_window(dev, shape, L, W, pos, dtype):
    """rule 3 with inv_freq = 0 (the rotation is then the exact identity).  pos >= W - 1: bit for bit the PLAIN launch with max_len
    = W at pos' = W - 1 on a cache whose rows 0 .. W - 2 are the rows lo .. pos - 1.  pos + 1 < W < L: bit for bit the plain launch on
    the cache truncated to W rows."""
    nq, nkv, hd = shape
    B = 4
    inv0 = torch.zeros(hd // 2, device=dev)
    probs = [WProblem(dev, shape, L, dtype, "peaked", pos, 1, W, 300 + b) for b in range(B)]
    out_w, kc_w, vc_w = _decode_launch(dev, shape, L, probs, W, inv=inv0)
    lo = wr.lo(pos, W)
    cut = [(p.kc[:, lo:lo + W].contiguous(), p.vc[:, lo:lo + W].contiguous()) for p in probs]
    kc, vc = _stack([c[0] for c in cut]), _stack([c[1] for c in cut])
    q, k, v = _qkv(*(torch.cat([getattr(p, a) for p in probs]) for a in ("q32", "k32", "v32")))
    pos_t = torch.full((B,), pos - lo, dtype=torch.long, device=dev)
    out = torch.full((B, nq * hd), float("nan"), dtype=F16, device=dev)
    qp.decode_attention(q, k, v, kc, vc, pos_t, inv0, out=out, ws=qp.attention_workspace(B, nq, nkv, hd, W, dev))
    torch.cuda.synchronize()
    assert pos - lo == (W - 1 if pos >= W - 1 else pos) and not bool(torch.isnan(out).any())
    assert torch.equal(_bits(out), _bits(out_w))
    assert torch.equal(_bits(kc[:, :, pos - lo]), _bits(kc_w[:, :, pos])) and torch.equal(_bits(vc[:, :, pos - lo]), _bits(vc_w[:, :, pos]))


def _page_out(cache, caches, dev):
    """the contiguous caches [B, nkv, L, hd] (k, v) into the pools of layer 0 of `cache`, every slot fully reserved"""
    B, nkv, L, hd = caches[0].shape
    ps = cache.page_size
    for b in range(B):
        cache.reserve(b, L)
        for j, page in enumerate(cache.pages_of(b)):
            for pool, c in zip((cache.kpool[0], cache.vpool[0]), caches):
                pool[page].view(torch.uint8).copy_(c[b, :, j * ps:(j + 1) * ps].view(torch.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("page", [16, 128])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_decode_paged_is_contiguous_and_survives_trim(dev, shape, page, dtype):
    """rule 4 and rule 2 (paged): the paged launch is bit for bit the contiguous one on the gathered cache; after trim() of every
    slot, with NaN in every freed page and in page 0, the output is bit for bit the output from before"""
    nq, nkv, hd = shape
    L, W = 1024, 200
    positions = [1023, 5, 199, 200, 333, 511, 512, 800]  # (slot 0 holds page 0: its window has left it)
    B = len(positions)
    probs = [WProblem(dev, shape, L, dtype, "peaked", p, 1, W, 400 + i, nan_below=False) for i, p in enumerate(positions)]
    out_c, kc, vc = _decode_launch(dev, shape, L, probs, W)
    cache = qp.PagedKVCache(1, B * L // page, nkv, page, hd, B, L // page, dtype=dtype, device=dev)
    _page_out(cache, (_stack([p.kc for p in probs]), _stack([p.vc for p in probs])), dev)
    q, k, v = _qkv(*(torch.cat([getattr(p, a) for p in probs]) for a in ("q32", "k32", "v32")))
    pos_t = torch.tensor(positions, dtype=torch.long, device=dev)
    ws = qp.attention_workspace(B, nq, nkv, hd, L, dev)

    def launch():
        out = torch.full((B, nq * hd), float("nan"), dtype=F16, device=dev)
        qp.paged_decode_attention(q, k, v, cache.kpool[0], cache.vpool[0], cache.table, pos_t, probs[0].inv, out=out, ws=ws, window=W)
        torch.cuda.synchronize()
        return out

    out_p = launch()
    assert torch.equal(_bits(out_p), _bits(out_c)) and not bool(torch.isnan(out_c).any())
    for b, p in enumerate(positions):  # the appended rows
        pg = cache.pages_of(b)[p // page]
        assert torch.equal(_bits(cache.kpool[0][pg, :, p % page]), _bits(kc[b, :, p])) and torch.equal(_bits(cache.vpool[0][pg, :, p % page]), _bits(vc[b, :, p]))
    free_before = set(cache._free)
    for b, p in enumerate(positions):
        cache.trim(b, qp.window_floor(p, W))
    freed = sorted(set(cache._free) - free_before)
    assert 0 in freed and len(freed) == sum(wr.lo(p, W) // page for p in positions)
    for pool in (cache.kpool[0], cache.vpool[0]):
        for pg in freed:
            ar.nan_rows(pool[pg], slice(0, page))
    assert torch.equal(_bits(launch()), _bits(out_c))


# ---------------------------------------------------------------------------------------------------------- prefill and ragged

PF_T = [1, 16, 17, 64, 128]
PF_W = [1, 5, 32, 33, 64, 100, 129, 516]
PF_L = [128, 512, 2048]


def _prefill_cases():
    """about 40 of the cross product T x W x pos0 x L: every T, W and L, every kind of pos0 (0, W - 1, W, 300, L - T), and the four
    situations the contract names"""
    cases, i = [], 0
    for W in PF_W:
        for kind in ("0", "W-1", "W", "300", "end"):
            L = PF_L[(i + (i // 3)) % 3]
            T = PF_T[i % 5]
            pos0 = {"0": 0, "W-1": W - 1, "W": W, "300": 300, "end": L - T}[kind]
            if pos0 + T > L:
                L = 2048
                pos0 = min(pos0, L - T)
            cases.append((SHAPES[i % 6], T, W, pos0, L, DTYPES[(i // 2) % 2]))
            i += 1
    cases += [((8, 8, 64), 128, 5, 300, 512, F16),      # W < T: the lower edge inside the new rows
              ((32, 8, 128), 64, 64, 64, 128, F8),      # W = T
              ((4, 2, 256), 17, 100, 300, 512, F16),    # the edge inside the cache, off a multiple of 32: lo = 201
              ((8, 1, 128), 128, 516, 1500, 2048, F8),  # a split launch: span >= 512
              ((16, 2, 64), 128, 516, 1920, 2048, F16)]
    return cases


PF_CASES = _prefill_cases()


def test_prefill_sample_covers_what_the_contract_names():
    seen = lambda i: {c[i] for c in PF_CASES}  # noqa: E731
    assert seen(0) == set(SHAPES) and seen(1) == set(PF_T) and seen(2) == set(PF_W) and seen(4) == set(PF_L) and seen(5) == set(DTYPES)
    assert all(p0 >= 0 and p0 + T <= L for _, T, W, p0, L, _ in PF_CASES) and 35 <= len(PF_CASES) <= 50
    assert any(W < T and p0 > 0 for _, T, W, p0, L, _ in PF_CASES) and any(W == T for _, T, W, p0, L, _ in PF_CASES)
    assert any(0 < wr.lo(p0, W) and wr.lo(p0, W) % 32 and wr.lo(p0, W) < p0 for _, T, W, p0, L, _ in PF_CASES)
    assert any(L == 2048 and p0 + T - wr.lo(p0, W) // 32 * 32 >= 512 for _, T, W, p0, L, _ in PF_CASES)
    for kind in (lambda W, T, L: 0, lambda W, T, L: W - 1, lambda W, T, L: W, lambda W, T, L: 300, lambda W, T, L: L - T):
        assert any(p0 == kind(W, T, L) for _, T, W, p0, L, _ in PF_CASES)


def _prefill_launch(prob, W, kc=None, vc=None):
    nq, nkv, hd = prob.shape
    out = torch.full((prob.T, nq * hd), float("nan"), dtype=F16, device=prob.dev)
    pos_t = torch.tensor([prob.pos0], dtype=torch.long, device=prob.dev)
    ws = qp.prefill_workspace(prob.T, nq, nkv, hd, prob.L, prob.dev)
    qp.prefill_attention(*_qkv(prob.q32, prob.k32, prob.v32), prob.kc if kc is None else kc, prob.vc if vc is None else vc, pos_t, prob.inv,
                         out=out, ws=ws, window=W)
    torch.cuda.synchronize()
    return out


def _needles(pos0, T, W):
    """the first and the last row's lo - 1 and lo"""
    ats = {wr.lo(pos0, W) - 1, wr.lo(pos0, W), wr.lo(pos0 + T - 1, W) - 1, wr.lo(pos0 + T - 1, W)}
    return sorted(a for a in ats if a >= 0)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,T,W,pos0,L,dtype", PF_CASES, ids=_id)
def test_prefill_window(dev, shape, T, W, pos0, L, dtype):
    nq, nkv, hd = shape
    what = f"{_id(shape)} {_id(dtype)} T={T} W={W} pos0={pos0} L={L}"
    # census, NaN below the floor
    prob = WProblem(dev, shape, L, dtype, "census", pos0, T, W, 0)
    _report("prefill_attention", "census", prob.worst(_prefill_launch(prob, W), U_PREFILL), what)
    # families, NaN below the floor; needles at the first and the last row's lo - 1 and lo
    for family in ar.FAMILIES:
        for at in (_needles(pos0, T, W) if family == "needle" else [None]):
            prob = WProblem(dev, shape, L, dtype, family, pos0, T, W, 400, needle_at=at)
            _report("prefill_attention", family, prob.worst(_prefill_launch(prob, W), U_PREFILL), f"{what} needle={at}")
    # rule 5: the cache bytes after the windowed launch are those after the unwindowed one; rule 1: a full-width window is that launch
    clean = WProblem(dev, shape, L, dtype, "peaked", pos0, T, W, 401, nan_below=False)
    caches = {}
    outs = {}
    for name, w in (("none", None), ("W", W), ("L", L), ("4L", 4 * L)):
        kc, vc = clean.kc.clone(), clean.vc.clone()
        outs[name] = _prefill_launch(clean, w, kc, vc)
        caches[name] = (kc, vc)
    for name in ("W", "L", "4L"):
        assert torch.equal(_bits(caches[name][0]), _bits(caches["none"][0])) and torch.equal(_bits(caches[name][1]), _bits(caches["none"][1])), name
    assert not bool(torch.isnan(outs["none"]).any())
    assert torch.equal(_bits(outs["L"]), _bits(outs["none"])) and torch.equal(_bits(outs["4L"]), _bits(outs["none"]))
    # rule 4: paged = contiguous (page 16), with the pages wholly below the floor trimmed and filled with NaN
    cache = qp.PagedKVCache(1, L // 16, nkv, 16, hd, 1, L // 16, dtype=dtype, device=dev)
    _page_out(cache, (clean.kc[None], clean.vc[None]), dev)
    cache.trim(0, wr.lo(pos0, W))
    gone = [p for p in range(L // 16) if p not in cache.pages_of(0)]
    for pool in (cache.kpool[0], cache.vpool[0]):
        for pg in gone:
            ar.nan_rows(pool[pg], slice(0, 16))
    out = torch.full((T, nq * hd), float("nan"), dtype=F16, device=dev)
    qp.paged_prefill_attention(*_qkv(clean.q32, clean.k32, clean.v32), cache.kpool[0], cache.vpool[0], cache.table[0],
                               torch.tensor([pos0], dtype=torch.long, device=dev), clean.inv, out=out,
                               ws=qp.prefill_workspace(T, nq, nkv, hd, L, dev), window=W)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(outs["W"]))
    for p in range(pos0, pos0 + T):
        pg = cache.pages_of(0)[p // 16]
        assert torch.equal(_bits(cache.kpool[0][pg, :, p % 16]), _bits(caches["W"][0][:, p]))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("W", [5, 100])
@pytest.mark.parametrize("L", [128, 2048])
@pytest.mark.parametrize("i,rows", list(enumerate(RAGGED_SEGMENTS)), ids=_id)
def test_ragged_segments_are_the_one_sequence_windowed_launch(dev, i, rows, L, W, dtype):
    nq, nkv, hd = shape = SHAPES[(i + (L == 2048) + 3 * (dtype == F8)) % 6]
    S, R = len(rows), sum(rows)
    slots = [(s + i) % S for s in range(S)]
    for family in ("census", "ramp_up"):
        probs = [WProblem(dev, shape, L, dtype, family, _ragged_pos0(t, L, s + i), t, W, 500 + s) if t else None for s, t in enumerate(rows)]
        idle = torch.zeros(nkv, L, hd, device=dev).to(dtype)
        by_slot = {slots[s]: p for s, p in enumerate(probs) if p is not None}
        kc = _stack([by_slot[b].kc if b in by_slot else idle for b in range(S)])
        vc = _stack([by_slot[b].vc if b in by_slot else idle for b in range(S)])
        live = [p for p in probs if p is not None]
        q, k, v = _qkv(*(torch.cat([getattr(p, a) for p in live]) for a in ("q32", "k32", "v32")))
        row0 = [0]
        for t in rows:
            row0.append(row0[-1] + t)
        seq = torch.tensor(slots, dtype=torch.int32, device=dev)
        row0_t = torch.tensor(row0, dtype=torch.int32, device=dev)
        pos0 = torch.tensor([p.pos0 if p is not None else 5 for p in probs], dtype=torch.int64, device=dev)
        out = torch.full((R, nq * hd), float("nan"), dtype=F16, device=dev)
        qp.ragged_prefill_attention(q, k, v, kc, vc, seq, row0_t, pos0, live[0].inv, out=out, ws=qp.ragged_workspace(R, S, nq, nkv, hd, L, dev),
                                    window=W)
        torch.cuda.synchronize()
        worst = 0.0
        for s, p in enumerate(probs):
            if p is None:
                continue
            seg = out[row0[s]:row0[s + 1]]
            worst = max(worst, p.worst(seg, U_PREFILL, kc[slots[s]], vc[slots[s]]))
            one = _prefill_launch(p, W)  # (on the problem's own cache, which the ragged launch's stack copied)
            assert torch.equal(_bits(one), _bits(seg)), (s, family)
            assert torch.equal(_bits(p.kc), _bits(kc[slots[s]])) and torch.equal(_bits(p.vc), _bits(vc[slots[s]]))
        _report("ragged_prefill_attention", family, worst, f"{_id(shape)} {_id(dtype)} segments={rows} L={L} W={W}")
