"""Attention parity that notices a lost key (tests/attn_reference.py; DESIGN.md §23, "attention parity bound").

The four kernel families — batch-1 decode (csrc/decoder_glue.hip), batched decode (csrc/attn_batch.hip), prefill
(csrc/attn_prefill.hip) and ragged prefill (csrc/attn_ragged.hip) — against
  * census: all keys 0, v_j = e_{j mod hd}: the output COUNTS the keys a row attended to, analytic, to one fp16 ulp;
  * peaked / ramp_up / ramp_down / offset / needle inputs against a float64 softmax within a bound derived from the formats.

CPU: the checks have teeth (every seeded defect of attention_fp64(mutate=...) lands >= 4x outside the bound in the family named for
it) and an emulation of the arithmetic sits inside the bound (this is where kappa is set).  GPU: the kernels."""
import math

import pytest
import torch

import attn_reference as ar
import qpalette_amd as qp
from attn_reference import F8, F16

SHAPES = [(8, 8, 64), (16, 2, 64), (8, 1, 128), (32, 8, 128), (4, 2, 256), (4, 1, 256)]  # nq, nkv, hd: rep 1, 8, 8, 4, 2, 4
DTYPES = [F16, F8]
U_PREFILL = 2.0 ** -11  # prefill and ragged round the softmax weights to fp16 in front of the second product; decode keeps fp32
TEETH = 4.0             # a seeded defect must be this many times outside the tolerance


def _id(v):
    if isinstance(v, torch.dtype):
        return "f16" if v == F16 else "e4m3"
    if isinstance(v, (tuple, list)):
        return "x".join(str(x) for x in v)
    return str(v)


# ---------------------------------------------------------------------------------------------------------------- CPU

CPU = torch.device("cpu")


def _cpu_rows(family, shape, pos, seed):
    """rotated fp16 q rows at positions pos, as a device would produce them from unrope()'d targets"""
    nq, nkv, hd = shape
    inv = ar.inv_freq(hd, CPU)
    tgt = ar.query_targets(len(pos), nq, nkv, hd, seed, CPU, family).view(len(pos), nq, hd)
    p = torch.tensor(pos)[:, None]
    return ar.rope_f16(ar.unrope(tgt, p, inv), p, inv).reshape(len(pos), nq * hd)


def _cpu_case(family, shape, n, dtype, seed=5, rows=1, needle_at=None):
    """(q16, K, V, n_keys_per_row): `rows` rows whose last attends to keys 0 .. n - 1 (rows > 1: a causal prefill chunk)"""
    nq, nkv, hd = shape
    pos = list(range(n - rows, n))
    q16 = _cpu_rows(family, shape, pos, seed)
    K, V = ar.build_cache(family, q16, nq, nkv, hd, n, n, 1.0 / math.sqrt(hd), seed + 10, needle_at=needle_at)
    return q16, ar.to_cache(K, dtype), ar.to_cache(V, dtype), [p + 1 for p in pos]


def _excess(family, shape, n, mutate, u_p, needle_at=None, dtype=F16):
    """the worst |mutated - ref| / bound of a seeded defect; inf where the defect gives a non-finite result"""
    nq, nkv, hd = shape
    q16, K, V, nk = _cpu_case(family, shape, n, dtype, needle_at=needle_at)
    scale = 1.0 / math.sqrt(hd)
    ref, A, Smax = ar.attention_fp64(q16, K, V, nk, nq, nkv, hd, scale)
    mut, _, _ = ar.attention_fp64(q16, K, V, nk, nq, nkv, hd, scale, mutate=mutate)
    if not bool(torch.isfinite(mut).all()):
        return float("inf")
    return float(((mut - ref).abs() / ar.bound(ref, A, Smax, u_p)).max())


def _lost_keys(n):
    """position 0, one below a multiple of 64, on a multiple of 64, pos - 1, pos (the new position)"""
    return [0, n // 2 - 1, n // 2, n - 2, n - 1]


@pytest.mark.parametrize("n", [2048, 8192])
@pytest.mark.parametrize("hd", [64, 256])
def test_census_catches_lost_doubled_and_misplaced_keys(n, hd):
    nq, nkv = 2, 2
    K, V = ar.census_cache(nkv, n + 1, hd, F16, CPU)
    exp, tol = ar.census_expected([n], nq, hd, CPU)
    assert bool(((ar.census_fp64(K, V, [n], nq, nkv, hd) - exp).abs() <= tol).all())  # the analytic value is the reference's
    for mutate in [("drop", j) for j in _lost_keys(n)] + [("double", n // 3), ("double", n - 1), ("past_diag",), ("causal_lt",)]:
        got = ar.census_fp64(K, V, [n], nq, nkv, hd, mutate=mutate)
        worst = float(((got - exp).abs() / tol).max())
        print(f"census n={n} hd={hd} {mutate}: {worst:.1f} x tol")
        assert worst >= TEETH, (mutate, worst)
    # prefill rows: row t must count exactly pos0 + t + 1 keys
    T = 17
    rows = list(range(n - T + 1, n + 1))
    exp, tol = ar.census_expected(rows, nq, hd, CPU)
    for mutate in (("causal_lt",), ("past_diag",), ("drop", n - T), ("drop", n - 1)):
        got = ar.census_fp64(K, V, rows, nq, nkv, hd, mutate=mutate)
        per_row = ((got - exp).abs() / tol).amax(dim=1)
        seen = per_row[-1:] if mutate == ("drop", n - 1) else per_row  # (the last key is in the last row only)
        assert float(seen.min()) >= TEETH, (mutate, per_row.tolist())


def test_census_tolerance_is_at_most_a_quarter_of_one_key_up_to_8192():
    """the issue's sizing rule: a lost key moves an element by hd / (n + 1) relative, at least 4 fp16 ulps for hd 64 and n <= 8192"""
    for n in (1, 2, 63, 64, 65, 1000, 8191, 8192):
        exp, tol = ar.census_expected([n], 1, 64, CPU)
        lost, _ = ar.census_expected([max(n - 1, 1)], 1, 64, CPU)
        if n > 1:
            assert float(((exp - lost).abs() / tol).max()) >= TEETH, n


@pytest.mark.parametrize("n", [2048, 32768])
@pytest.mark.parametrize("u_p", [0.0, U_PREFILL])
def test_needle_catches_a_lost_key(n, u_p):
    for j in _lost_keys(n):
        worst = _excess("needle", (8, 1, 128), n, ("drop", j), u_p, needle_at=j)
        print(f"needle n={n} at {j}: {worst:.1f} x bound")
        assert worst >= TEETH, (j, worst)


@pytest.mark.parametrize("n", [2048, 8192])
def test_offset_catches_a_missing_max_subtraction(n):
    for shape in SHAPES:
        assert _excess("offset", shape, n, ("no_max",), U_PREFILL) >= TEETH, shape


@pytest.mark.parametrize("n", [2048, 8192])
def test_ramps_catch_wrong_merge_weights(n):
    for shape in ((8, 1, 128), (4, 2, 256), (8, 8, 64)):
        for family in ("ramp_up", "ramp_down"):
            for chunk in (n // 4, 128):
                worst = _excess(family, shape, n, ("merge_w1", chunk), U_PREFILL)
                assert worst >= TEETH, (family, shape, chunk, worst)
        worst = _excess("ramp_up", shape, n, ("alpha_l_only", 32), U_PREFILL)
        assert worst >= TEETH, (shape, worst)


@pytest.mark.parametrize("n", [2048, 32768])
def test_peaked_catches_the_neighbouring_kv_head(n):
    for shape in ((16, 2, 64), (4, 2, 256)):
        worst = _excess("peaked", shape, n, ("kv_neighbour",), U_PREFILL)
        assert worst >= TEETH, (shape, worst)


def test_families_have_the_dynamic_range_they_are_named_for():
    nq, nkv, hd = shape = (8, 1, 128)
    n, scale = 2048, 1.0 / math.sqrt(128)
    def scores(family, **kw):
        q16, K, V, _ = _cpu_case(family, shape, n, F16, **kw)
        return torch.einsum("hd,jd->hj", q16.view(nq, hd).double(), K[0, :n].double()) * scale
    assert 4.0 < float(scores("peaked").std()) < 9.0
    up, down = scores("ramp_up"), scores("ramp_down")
    assert float((up[:, -64:].mean(1) - up[:, :64].mean(1)).min()) > 25.0  # every head; ~60 on the group's average
    assert float((up[:, -64:].mean(1) - up[:, :64].mean(1)).mean()) > 50.0
    assert float((down[:, :64].mean(1) - down[:, -64:].mean(1)).mean()) > 50.0
    assert float(scores("offset").min()) > 150.0  # exp overflows fp32 above 88.7
    s = scores("needle", needle_at=777)
    rest = torch.cat((s[:, :777], s[:, 778:]), dim=1)
    assert float((s[:, 777] - rest.amax(1)).min()) >= 30.0


EMU = [  # family, shape, n, rows, u_p: every family at both roundoffs, the largest contexts the GPU part uses
    *[(f, s, n, 1, 0.0) for f in ("base",) + ar.FAMILIES for s, n in (((8, 1, 128), 2048), ((16, 2, 64), 8192), ((4, 2, 256), 2048))],
    *[(f, (8, 1, 128), 32768, 1, 0.0) for f in ("peaked", "needle")],
    *[(f, s, n, 33, U_PREFILL) for f in ("base",) + ar.FAMILIES for s, n in (((8, 1, 128), 2048), ((16, 2, 64), 2048), ((4, 2, 256), 512))],
]


def test_emulation_sits_inside_the_bound():
    """kappa: emulate() (fp32 scores, fp32 exp, fp16 weights in 32-key tiles where u_p > 0, fp32 sums, fp16 out) against the float64
    reference on every family and both cache formats.  The output's own fp16 rounding fills the bound's first two terms by
    itself, so kappa's share is measured in front of it: the worst |fp32 quotient - ref| / ((u_p + 2^-23 (1 + Smax)) A), times 4,
    rounded up to a power of two, is attn_reference.KAPPA.  The rounded result must sit inside the whole bound."""
    worst = {}
    for family, shape, n, rows, u_p in EMU:
        nq, nkv, hd = shape
        for dtype in DTYPES:
            q16, K, V, nk = _cpu_case(family, shape, n, dtype, rows=rows, needle_at=n - 2 if family == "needle" else None)
            scale = 1.0 / math.sqrt(hd)
            ref, A, Smax = ar.attention_fp64(q16, K, V, nk, nq, nkv, hd, scale)
            emu = ar.emulate(q16, K, V, nk, nq, nkv, hd, scale, u_p).double()
            raw = ar.emulate(q16, K, V, nk, nq, nkv, hd, scale, u_p, rounded=False).double()
            r1 = float(((raw - ref).abs() / ar.weight_term(A, Smax, u_p)).max())  # in front of the output rounding: kappa's share
            r = float(((emu - ref).abs() / ar.bound(ref, A, Smax, u_p)).max())
            key = (family, u_p > 0)
            worst[key] = max(worst.get(key, 0.0), r1)
            assert r <= 1.0, (family, shape, n, _id(dtype), r)
    print("emulation err / weight term at kappa = 1, worst per (family, u_p > 0):")
    for key, r1 in sorted(worst.items()):
        print(f"  {key[0]:10s} u_p={'2^-11' if key[1] else '0':6s} {r1:.3f}")
    top = max(worst.values())
    assert 4.0 * top <= ar.KAPPA < 16.0 * top, (top, ar.KAPPA)  # the 4x margin holds, and kappa is no looser than the rule gives


# ---------------------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _rope_kv(q32, k32, v32, q16, kc, vc, pos_t, inv, shape):
    """qpal_rope_kv of ONE token: q16 <- rotated q, row pos of the fp16 cache [nkv, L, hd] <- rotated k, v"""
    nq, nkv, hd = shape
    nat = qp._native
    nat.check(nat.lib().qpal_rope_kv(q32.data_ptr(), k32.data_ptr(), v32.data_ptr(), q16.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                                     pos_t.data_ptr(), inv.data_ptr(), nq, nkv, hd, kc.shape[1], _stream(kc)), "qpal_rope_kv")


def _attn_decode(q16, kc, vc, out, pos_t, shape, scale):
    nq, nkv, hd = shape
    nat = qp._native
    nat.check(nat.lib().qpal_attn_decode(q16.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), pos_t.data_ptr(), nq, nkv, hd,
                                         kc.shape[1], scale, _stream(kc)), "qpal_attn_decode")


def _attn_ws(shape, ctx, dev):
    """the split-context workspace of the batch-1 launch, or None where that context has none (below 2048 positions)"""
    n = qp._native.lib().qpal_attn_ws_bytes(*shape, ctx)
    return torch.zeros(n // 4, dtype=torch.float32, device=dev) if n else None


def _attn_rope_decode(q32, k32, v32, kc, vc, out, pos_t, inv, shape, scale, ws):
    nq, nkv, hd = shape
    nat = qp._native
    nat.check(nat.lib().qpal_attn_rope_decode(q32.data_ptr(), k32.data_ptr(), v32.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(),
                                              pos_t.data_ptr(), inv.data_ptr(), nq, nkv, hd, kc.shape[1], scale,
                                              ws.data_ptr() if ws is not None else None, ws.numel() * 4 if ws is not None else 0,
                                              _stream(kc)), "qpal_attn_rope_decode")


def _qkv(q, k, v):
    """q | k | v as column slices of one buffer: the launches take rows with a common stride"""
    return torch.cat((q, k, v), dim=1).split([q.shape[1], k.shape[1], v.shape[1]], dim=1)


def _rotated_q(q32, positions, shape, dev):
    """fp16 q rows after the rotary embedding at `positions`, by qpal_rope_kv on a scratch cache"""
    nq, nkv, hd = shape
    Ls = (max(positions) + 4) // 4 * 4
    kc = torch.zeros(nkv, Ls, hd, dtype=F16, device=dev)
    vc = torch.zeros_like(kc)
    zero = torch.zeros(nkv * hd, device=dev)
    q16 = torch.zeros(len(positions), nq * hd, dtype=F16, device=dev)
    pos_t = torch.tensor(positions, dtype=torch.long, device=dev)
    q32 = q32.contiguous()
    for r in range(len(positions)):
        _rope_kv(q32[r], zero, zero, q16[r], kc, vc, pos_t[r:r + 1], ar.inv_freq(hd, dev), shape)
    return q16


class Problem:
    """ONE sequence: T new rows at positions pos0 .. pos0 + T - 1 on a cache [nkv, L, hd] of `dtype` built for `family`.
    q32 / k32 / v32: the fp32 rows a launch takes (unrope()'d targets: the device's rotary embedding gives the family's q and new
    keys); q16: the rotated q of qpal_rope_kv; kc / vc: the cache, NaN in the rows the launch writes and, except for census, in
    every row behind them (nothing there may matter; census keeps its pattern there so that a key admitted past the diagonal is
    counted).  After the launch, worst() reads the stored rows back: the reference sees what the kernels saw."""

    def __init__(self, dev, shape, L, dtype, family, pos0, T, seed, needle_at=None, cache_seed=None):
        nq, nkv, hd = shape
        self.shape, self.L, self.family, self.pos0, self.T, self.dev = shape, L, family, pos0, T, dev
        self.scale = 1.0 / math.sqrt(hd)
        self.inv = ar.inv_freq(hd, dev)
        self.n = [pos0 + t + 1 for t in range(T)]
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
            self.q16 = _rotated_q(self.q32, pos.tolist(), shape, dev)
            K, V = ar.build_cache(family, self.q16, nq, nkv, hd, L, pos0 + T, self.scale, seed + 7 if cache_seed is None else cache_seed,
                                  needle_at=needle_at)
            self.k32 = ar.unrope(K[:, pos0:pos0 + T].transpose(0, 1), pos[:, None], self.inv).reshape(T, nkv * hd)
            self.v32 = V[:, pos0:pos0 + T].transpose(0, 1).reshape(T, nkv * hd).contiguous()
            self.kc, self.vc = ar.to_cache(K, dtype), ar.to_cache(V, dtype)
            behind = slice(pos0, L)
        ar.nan_rows(self.kc, behind)
        ar.nan_rows(self.vc, behind)

    def renan(self):
        """NaN again into the rows a launch writes (a second launch on the same problem)"""
        ar.nan_rows(self.kc, slice(self.pos0, self.pos0 + self.T))
        ar.nan_rows(self.vc, slice(self.pos0, self.pos0 + self.T))

    def worst(self, out, u_p, kc=None, vc=None):
        """the worst err / tol of the rows `out` [T, nq * hd] of a launch that left the caches kc / vc (default: this problem's)"""
        nq, nkv, hd = self.shape
        out = out.double()
        if self.family == "census":
            exp, tol = ar.census_expected(self.n, nq, hd, self.dev)
        else:
            exp, A, Smax = ar.attention_fp64(self.q16, self.kc if kc is None else kc, self.vc if vc is None else vc, self.n, nq, nkv, hd,
                                             self.scale)
            tol = ar.bound(exp, A, Smax, u_p)
        r = (out - exp).abs() / tol
        return float(torch.nan_to_num(r, nan=float("inf")).max())


_WORST = {}


def _report(kernels, family, worst, what):
    """print the case's worst err / tol and the running worst of its (kernel family, input family) — the figures DESIGN.md records"""
    key = (kernels, family)
    _WORST[key] = max(_WORST.get(key, 0.0), worst)
    print(f"{kernels} {family} {what}: worst err/tol = {worst:.3f} (so far over {kernels} {family}: {_WORST[key]:.3f})")
    assert worst <= 1.0, (kernels, family, what, worst)


# ---- batched decode

def _stack(caches):
    """[B, nkv, L, hd] of B one-sequence caches (through bytes: either format)"""
    return torch.stack([c.view(torch.uint8) for c in caches]).view(caches[0].dtype)


def _decode_launch(dev, shape, L, dtype, problems):
    """decode_attention on B one-row problems (each a sequence of its own): out [B, nq * hd] and the caches as the launch left them"""
    nq, nkv, hd = shape
    B = len(problems)
    kc, vc = _stack([p.kc for p in problems]), _stack([p.vc for p in problems])
    q, k, v = _qkv(*(torch.cat([getattr(p, a) for p in problems]) for a in ("q32", "k32", "v32")))
    pos_t = torch.tensor([p.pos0 for p in problems], dtype=torch.long, device=dev)
    out = torch.full((B, nq * hd), float("nan"), dtype=F16, device=dev)
    qp.decode_attention(q, k, v, kc, vc, pos_t, problems[0].inv, out=out, ws=qp.attention_workspace(B, nq, nkv, hd, L, dev))
    torch.cuda.synchronize()
    return out, kc, vc


def _census_decode(dev, shape, L, dtype, B, positions, what):
    """census through decode_attention: `positions` in launches of B sequences (the last padded with inactive slots, pos = -1)"""
    nq, nkv, hd = shape
    K1, V1 = ar.census_cache(nkv, L, hd, dtype, dev)
    kc, vc = _stack([K1] * B), _stack([V1] * B)
    ws = qp.attention_workspace(B, nq, nkv, hd, L, dev)
    inv = ar.inv_freq(hd, dev)
    q = ar.query_targets(B, nq, nkv, hd, 3, dev)
    k = torch.zeros(B, nkv * hd, device=dev)
    seqs = torch.arange(B, device=dev)
    outs = []
    for i in range(0, len(positions), B):
        pos = positions[i:i + B] + [-1] * (i + B - len(positions))
        pos_t = torch.tensor(pos, dtype=torch.long, device=dev)
        act = pos_t >= 0
        for c in (kc, vc):  # NaN into the rows this launch writes
            (c if dtype == F16 else c.view(torch.uint8))[seqs[act], :, pos_t[act]] = float("nan") if dtype == F16 else 0x7F
        out = torch.full((B, nq * hd), float("nan"), dtype=F16, device=dev)
        qp.decode_attention(*_qkv(q, k, ar.census_new_v(pos_t, nkv, hd, dev)), kc, vc, pos_t, inv, out=out, ws=ws)
        outs.append(out[act])
    torch.cuda.synchronize()
    # every NaN row was written back: v as it was, k as +-0
    assert torch.equal(vc.view(torch.uint8), _stack([V1] * B).view(torch.uint8)) and not bool((kc.view(torch.uint8) & 0x7F).any())
    exp, tol = ar.census_expected([p + 1 for p in positions], nq, hd, dev)
    r = (torch.cat(outs).double() - exp).abs() / tol
    _report("decode_attention", "census", float(torch.nan_to_num(r, nan=float("inf")).max()), what)


def _edges(L, lo=0):
    """every multiple of 64 in [lo, L) with the position in front of it and behind it, and L - 1"""
    return sorted({p for m in range(lo // 64 * 64, L + 1, 64) for p in (m - 1, m, m + 1) if lo <= p < L} | {L - 1})


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_decode_census_short_cache_every_position(dev, shape, dtype):
    _census_decode(dev, shape, 128, dtype, 128, list(range(128)), f"{_id(shape)} {_id(dtype)} L=128 B=128")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("L", [512, 2048])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_decode_census_one_chunk_per_sequence(dev, shape, L, dtype):
    """B = 128: with B * nkv >= 256 workgroups the host asks for no split (nsplit = 1; the kv-head-1 shapes get 2)"""
    _census_decode(dev, shape, L, dtype, 128, _edges(L), f"{_id(shape)} {_id(dtype)} L={L} B=128")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("L", [512, 2048])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_decode_census_split_context_every_position(dev, shape, L, dtype):
    """B = 4: up to 64 chunks per (sequence, kv head) of at least 128 positions, cut in the kernel from each sequence's own
    position — so every position of the cache is a case of its own"""
    _census_decode(dev, shape, L, dtype, 4, list(range(L)), f"{_id(shape)} {_id(dtype)} L={L} B=4")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_decode_census_where_the_lds_forces_the_split(dev, dtype):
    """B = 32, nkv = 8, rep 8, hd 128, 4096 positions: 256 workgroups without a split, but one chunk's scores hold 2944 positions"""
    _census_decode(dev, (64, 8, 128), 4096, dtype, 32, [2942, 2943, 2944, 2945] + _edges(4096, 2946), f"64x8x128 {_id(dtype)} L=4096 B=32")


def _decode_cases(L):
    """(pos, needle_at): position 0, both sides of a chunk edge (the middle of the cache: a multiple of 128 and of every chunk
    length that divides it) and the last; the needle at the new position, in front of it, at position 0 and on both sides of a
    64-key tile edge"""
    plain = [(0, None), (L // 2 - 1, None), (L // 2, None), (L - 1, None)]
    needles = [(0, 0), (L - 1, L - 1), (L - 1, L - 2), (L - 1, 0), (L - 1, 63), (L - 1, 64), (L // 2, L // 2), (L // 2, L // 2 - 1),
               (L // 2 + 1, L // 2)]
    return plain, needles


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("L", [128, 512, 2048])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_decode_families_within_the_bound(dev, shape, L, dtype):
    plain, needles = _decode_cases(L)
    for family in ar.FAMILIES:
        cases = needles if family == "needle" else plain
        probs = [Problem(dev, shape, L, dtype, family, p, 1, 100 + i, needle_at=at) for i, (p, at) in enumerate(cases)]
        out, kc, vc = _decode_launch(dev, shape, L, dtype, probs)
        worst = max(p.worst(out[b:b + 1], 0.0, kc[b], vc[b]) for b, p in enumerate(probs))
        _report("decode_attention", family, worst, f"{_id(shape)} {_id(dtype)} L={L}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_decode_long_cache(dev, dtype):
    """32768 positions, B = 3, one kv head: 64 chunks of up to 512 positions"""
    shape, L = (8, 1, 128), 32768
    for family, cases in (("peaked", [(L - 1, None), (L // 2, None), (2943, None)]),
                          ("needle", [(L - 1, L - 1), (L - 1, 511), (L // 2, L // 2 - 1)])):
        probs = [Problem(dev, shape, L, dtype, family, p, 1, 200 + i, needle_at=at) for i, (p, at) in enumerate(cases)]
        out, kc, vc = _decode_launch(dev, shape, L, dtype, probs)
        worst = max(p.worst(out[b:b + 1], 0.0, kc[b], vc[b]) for b, p in enumerate(probs))
        _report("decode_attention", family, worst, f"{_id(shape)} {_id(dtype)} L={L}")


# ---- batch-1 kernels

B1_POSITIONS = (0, 63, 64, 511, 512, 2047)


def _batch1_outputs(prob, ws):
    """the three batch-1 forms on one one-row problem: qpal_rope_kv + qpal_attn_decode, qpal_attn_rope_decode without and (where
    the context has one) with the split-context workspace"""
    nq, nkv, hd = prob.shape
    pos_t = torch.tensor([prob.pos0], dtype=torch.long, device=prob.dev)
    outs = {}
    out = torch.full((1, nq * hd), float("nan"), dtype=F16, device=prob.dev)
    q16 = torch.zeros(nq * hd, dtype=F16, device=prob.dev)
    _rope_kv(prob.q32[0], prob.k32[0], prob.v32[0], q16, prob.kc, prob.vc, pos_t, prob.inv, prob.shape)
    _attn_decode(q16, prob.kc, prob.vc, out, pos_t, prob.shape, prob.scale)
    outs["rope_kv + attn_decode"] = out
    for name, w in (("attn_rope_decode", None), ("attn_rope_decode split", ws)):
        if name.endswith("split") and ws is None:
            continue
        prob.renan()
        out = torch.full((1, nq * hd), float("nan"), dtype=F16, device=prob.dev)
        _attn_rope_decode(prob.q32[0], prob.k32[0], prob.v32[0], prob.kc, prob.vc, out, pos_t, prob.inv, prob.shape, prob.scale, w)
        outs[name] = out
    torch.cuda.synchronize()
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("ctx", [64, 512, 2048, 8192])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_batch_one_kernels(dev, shape, ctx):
    ws = _attn_ws(shape, ctx, dev)
    assert (ws is not None) == (ctx >= 2048)
    positions = [p for p in B1_POSITIONS if p < ctx - 1] + [ctx - 1]
    worst = {}
    for i, pos in enumerate(positions):
        needle_at = (pos, max(pos - 1, 0), 0, pos // 64 * 64)[i % 4]
        for family in ("census",) + ar.FAMILIES:
            prob = Problem(dev, shape, ctx, F16, family, pos, 1, 300 + i, needle_at=needle_at, cache_seed=299)
            for name, out in _batch1_outputs(prob, ws).items():
                worst[family] = max(worst.get(family, 0.0), prob.worst(out, 0.0))
    for family, w in worst.items():  # (one workspace through every launch: a ticket left behind would spoil the next)
        _report("batch-1", family, w, f"{_id(shape)} ctx={ctx}")


@pytest.mark.gpu
def test_batch_one_kernel_opts_in_to_its_lds_at_every_head_size(dev):
    """qpal_attn_rope_decode WITHOUT a workspace at 16384 positions: the one-workgroup-per-head kernel asks for 4 * (16384 + 18 hd +
    32) bytes of dynamic LDS — 74 880 at hd 128, 70 272 at hd 64, both above the 64 KiB a kernel gets without the opt-in.  Both
    head sizes in one process, in this order: the opt-in belongs to a kernel, and a latch the head sizes share refuses whichever
    comes second."""
    ctx = 16384
    for shape in ((8, 1, 128), (8, 8, 64)):
        nq, nkv, hd = shape
        worst = {}
        for i, pos in enumerate((16383, 8191)):
            for family in ("census", "needle"):
                prob = Problem(dev, shape, ctx, F16, family, pos, 1, 400 + i, needle_at=(pos, pos // 64 * 64)[i])
                pos_t = torch.tensor([pos], dtype=torch.long, device=dev)
                out = torch.full((1, nq * hd), float("nan"), dtype=F16, device=dev)
                _attn_rope_decode(prob.q32[0], prob.k32[0], prob.v32[0], prob.kc, prob.vc, out, pos_t, prob.inv, shape, prob.scale, None)
                torch.cuda.synchronize()  # (the launch returned QPAL_OK: check() raises on anything else)
                worst[family] = max(worst.get(family, 0.0), prob.worst(out, 0.0))
        for family, w in worst.items():
            _report("batch-1", family, w, f"{_id(shape)} ctx={ctx} no workspace")


# ---- prefill

PF_T = [1, 15, 16, 17, 32, 33, 127, 128]
PF_POS0 = [0, 1, 15, 16, 31, 32, 33, 127, 128, 500, 511, 512, "end"]  # "end": max_len - T
PF_L = [128, 512, 2048]


def _prefill_census_cases():
    """a sample of the cross product: every pos0 that fits meets every max_len, and T, head shape and cache format run through their
    values along the way (a T that does not fit behind pos0 makes room for the next that does); then the split form with chunks
    wholly behind an early row's diagonal (T = 128 at the front of a long cache) on every head shape"""
    cases, i = [], 0
    for L in PF_L:
        for p in PF_POS0:
            if p != "end" and p >= L:
                continue
            T = next(t for t in PF_T[i % 8:] + PF_T[:i % 8] if p == "end" or p + t <= L)
            cases.append((SHAPES[i % 6], T, L - T if p == "end" else p, L, DTYPES[(i // 2) % 2]))
            i += 1
    cases += [(shape, 128, (0, 512, 1920)[j % 3], 2048, DTYPES[j % 2]) for j, shape in enumerate(SHAPES)]
    cases += [((32, 8, 128), 128, 0, 512, F16), ((8, 8, 64), 127, 385, 512, F8)]
    # a query tile whose first rows end in front of a 128-key chunk edge that its last rows pass: the chunk behind the edge is
    # empty for the first rows (their partial has sum 0 and takes part in the merge)
    cases += [((8, 8, 64), 33, 127, 2048, F16), ((32, 8, 128), 33, 127, 512, F8), ((4, 2, 256), 17, 505, 2048, F8)]
    return cases


PF_CENSUS = _prefill_census_cases()


def test_prefill_census_sample_covers_every_value():
    seen = lambda i: {c[i] for c in PF_CENSUS}
    assert seen(0) == set(SHAPES) and seen(1) == set(PF_T) and seen(3) == set(PF_L) and seen(4) == set(DTYPES)
    for L in PF_L:
        have = {p0 for _, _, p0, l, _ in PF_CENSUS if l == L}
        assert {p for p in PF_POS0 if p != "end" and p < L} <= have, L
        assert any(p0 + T == L for _, T, p0, l, _ in PF_CENSUS if l == L), L  # "end"
    assert all(p0 >= 0 and p0 + T <= L for _, T, p0, L, _ in PF_CENSUS) and len(PF_CENSUS) <= 50
    # the split form (max_len >= 512, chunks of 128 keys at these sizes) with a chunk edge inside the first query tile's diagonals
    assert sum(L >= 512 and p0 % 128 and p0 // 128 != (p0 + min(T, 16) - 1) // 128 for _, T, p0, L, _ in PF_CENSUS) >= 3


def _prefill_launch(prob):
    nq, nkv, hd = prob.shape
    out = torch.full((prob.T, nq * hd), float("nan"), dtype=F16, device=prob.dev)
    pos_t = torch.tensor([prob.pos0], dtype=torch.long, device=prob.dev)
    ws = qp.prefill_workspace(prob.T, nq, nkv, hd, prob.L, prob.dev)
    qp.prefill_attention(*_qkv(prob.q32, prob.k32, prob.v32), prob.kc, prob.vc, pos_t, prob.inv, out=out, ws=ws)
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape,T,pos0,L,dtype", PF_CENSUS, ids=_id)
def test_prefill_census_row_t_counts_pos0_plus_t_plus_1_keys(dev, shape, T, pos0, L, dtype):
    prob = Problem(dev, shape, L, dtype, "census", pos0, T, 0)
    worst = prob.worst(_prefill_launch(prob), U_PREFILL)
    _report("prefill_attention", "census", worst, f"{_id(shape)} {_id(dtype)} T={T} pos0={pos0} L={L}")


def _chunk_of(i, L):
    """(T, pos0) of the i-th family case: a chunk across a 32-key tile edge, a full one at the end of the cache, a short one"""
    return [(33, 31), (128, L - 128), (17, min(500, L - 17))][i % 3]


def _needle_positions(T, pos0):
    """the last row's diagonal, the key in front of it, the first and the last key of a 32-key tile that rows of the chunk see"""
    last = pos0 + T - 1
    tile = last // 32 * 32
    return [last, max(last - 1, 0), tile, max(tile - 1, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("L", PF_L)
@pytest.mark.parametrize("i,shape", list(enumerate(SHAPES)), ids=_id)
def test_prefill_families_within_the_bound(dev, i, shape, L, dtype):
    T, pos0 = _chunk_of(i + PF_L.index(L), L)
    for family in ar.FAMILIES:
        for at in (_needle_positions(T, pos0) if family == "needle" else [None]):
            prob = Problem(dev, shape, L, dtype, family, pos0, T, 400 + i, needle_at=at)
            worst = prob.worst(_prefill_launch(prob), U_PREFILL)
            _report("prefill_attention", family, worst, f"{_id(shape)} {_id(dtype)} T={T} pos0={pos0} L={L} needle={at}")


# ---- ragged prefill

RAGGED_SEGMENTS = [[1, 1, 1, 1], [17, 1, 16, 30], [128], [5, 0, 3, 120]]  # test_ragged_prefill.py's lists: rows per segment


def _ragged_pos0(rows, L, j):
    """differing first positions: 0, a tile edge, the split threshold, the end of the cache"""
    return [0, 31, min(511, L - rows), L - rows][j % 4] if rows else 5


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("L", [128, 2048])
@pytest.mark.parametrize("i,rows", list(enumerate(RAGGED_SEGMENTS)), ids=_id)
def test_ragged_census_and_families(dev, i, rows, L, dtype):
    nq, nkv, hd = shape = SHAPES[(i + (L == 2048) + 3 * (dtype == F8)) % 6]
    S, R = len(rows), sum(rows)
    slots = [(s + i) % S for s in range(S)]  # segment s is sequence slots[s]
    for family in ("census", "peaked", "ramp_up"):
        probs = [Problem(dev, shape, L, dtype, family, _ragged_pos0(t, L, s + i), t, 500 + s) if t else None for s, t in enumerate(rows)]
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
        ws = qp.ragged_workspace(R, S, nq, nkv, hd, L, dev)
        qp.ragged_prefill_attention(q, k, v, kc, vc, seq, row0_t, pos0, live[0].inv, out=out, ws=ws)
        torch.cuda.synchronize()
        worst = max(p.worst(out[row0[s]:row0[s + 1]], U_PREFILL, kc[slots[s]], vc[slots[s]]) for s, p in enumerate(probs) if p is not None)
        _report("ragged_prefill_attention", family, worst, f"{_id(shape)} {_id(dtype)} segments={rows} L={L}")
