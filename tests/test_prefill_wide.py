"""Wide prefill attention (csrc/attn_prefill_wide.hip): prefill_attention / paged_prefill_attention at 129 .. 256 rows
and Prefill(wide=256, wide_attention=True).

CPU: the two entry points' return codes with made-up pointers; the workspace size is monotone.  GPU: the census (row t counts
exactly pos0 + t + 1 keys), attn_reference's families against attention_fp64 within bound(u_p = 2^-11: P is rounded to fp16 in front
of the second product, as in the 128-row kernel), the cache bytes against two 128-row launches, the fit rule, the whole model."""
import functools
import math

import pytest
import torch

import attn_reference as ar
import model_reference as mr
import qpalette_amd as qp
from attn_reference import F8, F16

gpu = pytest.mark.gpu
E_SHAPE, E_NULL, E_ALIGN = -1, -3, -4
SHAPES = [(32, 8, 128), (16, 2, 64), (8, 8, 64), (4, 2, 128)]  # nq, nkv, hd: rep 4, 8, 1, 2 (hd 256 has no wide launch)
U_P = 2.0 ** -11


# ---------------------------------------------------------------------------------------------------------------- CPU
def _call(q=16, k=16, v=16, ld=4096, kc=4096, vc=4096, out=16, ld_out=4096, pos=16, inv=16, table=None, pages=64, ps=16, mp=64, fmt=0,
          T=256, nq=32, nkv=8, hd=128, L=1024, ws=4096, ws_bytes=1 << 30):
    return qp._native.lib().qpal_attn_rope_prefill_wide(q, k, v, ld, kc, vc, out, ld_out, pos, inv, table, pages, ps, mp, fmt, T, nq, nkv,
                                                        hd, L, 0.1, ws, ws_bytes, None)


def test_return_codes_without_a_gpu():
    """every argument error is a return code in front of any stream work: none of these pointers is ever dereferenced"""
    for name in ("q", "k", "v", "kc", "vc", "out", "pos", "inv", "ws"):
        assert _call(**{name: None}) == E_NULL, name
    for kw in ({"T": 128}, {"T": 257}, {"T": 0}, {"hd": 96}, {"hd": 32}, {"hd": 256, "nq": 16, "nkv": 4}, {"nq": 24}, {"nq": 128},
               {"L": 1022}, {"L": 0}, {"ld": 4095}, {"ld_out": 100}, {"fmt": 2}, {"ws_bytes": 4096}, {"table": 16, "ps": 24},
               {"table": 16, "pages": 0}, {"table": 16, "mp": 0}):
        assert _call(**kw) == E_SHAPE, kw
    for kw in ({"kc": 4096 + 8}, {"vc": 4096 + 2}, {"q": 18}, {"pos": 17}, {"out": 17}, {"ws": 4096 + 4}, {"table": 18}):
        assert _call(**kw) == E_ALIGN, kw


def test_workspace_size_is_monotone_and_covers_the_128_row_launches():
    lib = qp._native.lib()
    ws, narrow = lib.qpal_attn_prefill_wide_ws_bytes, lib.qpal_attn_prefill_ws_bytes
    for nq, nkv, hd in SHAPES + [(64, 8, 128)]:
        for L in (256, 508, 512, 2048, 32768):
            sizes = [ws(T, nq, nkv, hd, L) for T in range(129, 257)]
            assert all(s >= T * nq * hd * 2 and s % 16 == 0 for T, s in zip(range(129, 257), sizes))  # the q scratch at least
            assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] >= narrow(128, nq, nkv, hd, L), (nq, nkv, hd, L)
        for T in (129, 200, 256):
            sizes = [ws(T, nq, nkv, hd, L) for L in range(4, 65536 + 4, 508)]
            assert all(a <= b for a, b in zip(sizes, sizes[1:])), (nq, nkv, hd, T)
    assert ws(128, 32, 8, 128, 4096) == 0 and ws(257, 32, 8, 128, 4096) == 0 and ws(256, 16, 4, 256, 4096) == 0
    for kw in (dict(wide_attention=True), dict(wide=256, wide_attention=1)):
        with pytest.raises(qp._native.QpalError, match="wide_attention must be"):
            qp.Prefill([], torch.zeros(4, 64), None, torch.zeros(4, 64), [], [], None, **kw)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _id(v):
    return ("f16" if v == F16 else "e4m3") if isinstance(v, torch.dtype) else "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _launch(shape, q, k, v, kc, vc, pos0, page=None, out=None, split=False):
    """prefill_attention on the contiguous caches kc / vc [nkv, L, hd], in place; page: through pools whose pages are a permutation
    (paged_prefill_attention) and back.  split: two launches of 128 rows or fewer (the existing entry) in place of the wide one."""
    nq, nkv, hd = shape
    T, L, dev = q.shape[0], kc.shape[1], kc.device
    q, k, v = torch.cat((q, k, v), dim=1).split([q.shape[1], k.shape[1], v.shape[1]], dim=1)  # column slices of one buffer
    out = torch.full((T, nq * hd), float("nan"), dtype=F16, device=dev) if out is None else out
    ws = qp.prefill_workspace(T, nq, nkv, hd, L, dev)
    if page is None:
        attend, caches = qp.prefill_attention, (kc, vc)
    else:
        table = torch.randperm(L // page, generator=torch.Generator().manual_seed(L + page)).int().to(dev)
        to_pool = lambda c: c.view(torch.uint8).view(nkv, L // page, page, -1).transpose(0, 1)[torch.argsort(table)].contiguous().view(c.dtype)
        attend, caches = qp.paged_prefill_attention, (to_pool(kc), to_pool(vc), table)
    for r in ((0, 128) if split else (0,)):
        n = 128 if split else T
        attend(q[r:r + n], k[r:r + n], v[r:r + n], *caches, torch.tensor([pos0 + r], device=dev), ar.inv_freq(hd, dev), out=out[r:r + n], ws=ws)
    if page is not None:
        for c, pool in zip((kc, vc), caches):
            c.view(torch.uint8).copy_(pool.view(torch.uint8)[table.long()].transpose(0, 1).reshape(nkv, L, -1))
    torch.cuda.synchronize()
    assert ws is None or not bool(ws.view(torch.int32)[:nkv * 8].any())  # the tickets are back at zero
    return out


@gpu
@pytest.mark.parametrize("page", [None, 16, 128])
@pytest.mark.parametrize("L,pos0", [(256, 0), (512, 256), (1024, 1), (1024, 63), (1024, 768), (2048, 1000)])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_census_row_t_counts_pos0_plus_t_plus_1_keys(shape, L, pos0, page):
    nq, nkv, hd = shape
    dev = torch.device("cuda", 0)
    for dtype in (F16, F8):
        for T in (129, 160, 193, 255, 256):
            if pos0 + T > L:
                continue
            kc, vc = ar.census_cache(nkv, L, hd, dtype, dev)
            ar.nan_rows(kc, slice(pos0, pos0 + T))  # the rows the launch writes (behind them the census pattern stays: a key
            ar.nan_rows(vc, slice(pos0, pos0 + T))  # admitted past the diagonal is counted)
            pos = torch.arange(pos0, pos0 + T, device=dev)
            out = _launch(shape, ar.query_targets(T, nq, nkv, hd, 0, dev), torch.zeros(T, nkv * hd, device=dev),
                          ar.census_new_v(pos, nkv, hd, dev), kc, vc, pos0, page)
            exp, tol = ar.census_expected((pos + 1).tolist(), nq, hd, dev)
            worst = float(torch.nan_to_num((out.double() - exp).abs() / tol, nan=float("inf")).max())
            print(f"wide census {_id(shape)} {_id(dtype)} T={T} pos0={pos0} L={L} page={page}: worst err/tol = {worst:.3f}")
            assert worst <= 1.0, (dtype, T)


def _rotated_q(q32, pos0, shape, dev):
    """fp16 q rows after the rotary embedding at pos0 + row, by qpal_rope_kv on a scratch cache"""
    nq, nkv, hd = shape
    T, nat = q32.shape[0], qp._native
    kc = torch.zeros(2, nkv, (pos0 + T + 3) // 4 * 4, hd, dtype=F16, device=dev)
    zero, q16 = torch.zeros(nkv * hd, device=dev), torch.zeros(T, nq * hd, dtype=F16, device=dev)
    pos, inv, q32 = torch.arange(pos0, pos0 + T, device=dev), ar.inv_freq(hd, dev), q32.contiguous()
    for r in range(T):
        nat.check(nat.lib().qpal_rope_kv(q32[r].data_ptr(), zero.data_ptr(), zero.data_ptr(), q16[r].data_ptr(), kc[0].data_ptr(),
                                         kc[1].data_ptr(), pos[r:].data_ptr(), inv.data_ptr(), nq, nkv, hd, kc.shape[2],
                                         torch.cuda.current_stream(dev).cuda_stream), "qpal_rope_kv")
    return q16


@gpu
@pytest.mark.parametrize("dtype", [F16, F8], ids=_id)
@pytest.mark.parametrize("L", [256, 2048])
@pytest.mark.parametrize("T", [129, 256])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_families_within_the_bound(shape, T, L, dtype):
    """the chunk at the end of the cache (L = 2048: split chunks); the reference reads the rows the launch stored"""
    nq, nkv, hd = shape
    dev, pos0, scale = torch.device("cuda", 0), L - T, 1.0 / math.sqrt(hd)
    pos, inv = torch.arange(pos0, L, device=dev), ar.inv_freq(hd, dev)
    for family in ar.FAMILIES:
        for at in ((L - 1, (L - 1) // 64 * 64 - 1) if family == "needle" else (None,)):
            tgt = ar.query_targets(T, nq, nkv, hd, 400, dev, family).view(T, nq, hd)
            q32 = ar.unrope(tgt, pos[:, None], inv).reshape(T, nq * hd)
            q16 = _rotated_q(q32, pos0, shape, dev)
            K, V = ar.build_cache(family, q16, nq, nkv, hd, L, L, scale, 407, needle_at=at)
            k32 = ar.unrope(K[:, pos0:].transpose(0, 1), pos[:, None], inv).reshape(T, nkv * hd)
            v32 = V[:, pos0:].transpose(0, 1).reshape(T, nkv * hd).contiguous()
            kc, vc = ar.to_cache(K, dtype), ar.to_cache(V, dtype)
            ar.nan_rows(kc, slice(pos0, L))
            ar.nan_rows(vc, slice(pos0, L))
            out = _launch(shape, q32, k32, v32, kc, vc, pos0)
            ref, A, Smax = ar.attention_fp64(q16, kc, vc, (pos + 1).tolist(), nq, nkv, hd, scale)
            worst = float(torch.nan_to_num((out.double() - ref).abs() / ar.bound(ref, A, Smax, U_P), nan=float("inf")).max())
            print(f"wide {family} {_id(shape)} {_id(dtype)} T={T} L={L} needle={at}: worst err/tol = {worst:.3f}")
            assert worst <= 1.0, (family, at)


def _random_problem(shape, T, L, dtype, dev, seed=3):
    nq, nkv, hd = shape
    gen = torch.Generator(device=dev).manual_seed(seed)
    q, k, v = (torch.randn(T, w * hd, device=dev, generator=gen) for w in (nq, nkv, nkv))
    caches = [ar.to_cache(0.5 * torch.randn(nkv, L, hd, device=dev, generator=gen), dtype) for _ in range(2)]
    return q, k, 3.0 * v, caches


@gpu
@pytest.mark.parametrize("page", [None, 16])
@pytest.mark.parametrize("dtype", [F16, F8], ids=_id)
@pytest.mark.parametrize("T", [129, 256])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_cache_bytes_are_those_of_two_128_row_launches(shape, T, dtype, page):
    dev, L, pos0 = torch.device("cuda", 0), 1024, 515
    q, k, v, before = _random_problem(shape, T, L, dtype, dev)
    wide, two = [c.clone() for c in before], [c.clone() for c in before]
    _launch(shape, q, k, v, *wide, pos0, page)
    _launch(shape, q, k, v, *two, pos0, page, split=True)
    rows = torch.ones(L, dtype=torch.bool, device=dev)
    rows[pos0:pos0 + T] = False
    for w, t, b in zip(wide, two, before):
        assert torch.equal(w.view(torch.uint8), t.view(torch.uint8))
        assert torch.equal(w.view(torch.uint8)[:, rows], b.view(torch.uint8)[:, rows]) and not torch.equal(w.view(torch.uint8), b.view(torch.uint8))


@gpu
@pytest.mark.parametrize("page", [None, 16])
@pytest.mark.parametrize("dtype", [F16, F8], ids=_id)
def test_fit_rule(dtype, page):
    shape, T, L, dev = (16, 2, 64), 200, 1024, torch.device("cuda", 0)
    q, k, v, before = _random_problem(shape, T, L, dtype, dev)
    for pos0 in (L - T + 1, L, -1, L - T):
        caches, out = [c.clone() for c in before], torch.full((T, shape[0] * shape[2]), 7.0, dtype=F16, device=dev)
        _launch(shape, q, k, v, *caches, pos0, page, out=out)
        same = all(torch.equal(c.view(torch.uint8), b.view(torch.uint8)) for c, b in zip(caches, before))
        if pos0 == L - T:
            assert not same and bool(torch.isfinite(out.float()).all()) and not bool((out == 7.0).all(dim=1).any())
        else:
            assert same and bool((out == 7.0).all()), pos0


CTX, LENS = 320, (257, 300)


@functools.lru_cache(maxsize=None)
def _model():
    """two layers of model_reference's small model and its float64 / emulated forward on ONE 300-token prompt (test_gemm_wide.py's)"""
    dev = torch.device("cuda", 0)
    m = mr.build("S", "mixed", (), 2, mr.VOCAB, 0, dev, spec=mr.build_spec("S", "mixed", nlayers=2))
    toks = torch.randint(0, mr.VOCAB, (max(LENS),), generator=torch.Generator().manual_seed(4))
    return m, toks.to(dev), mr.forward_fp64(m.ref, [toks], chunk=64), mr.forward_emulated(m.ref, [toks], chunk=64, prefill=True)


def _prefill(N, **kw):
    m, toks, _, _ = _model()
    nkv, hd = m.cfg.num_key_value_heads, m.cfg.head_dim
    kc = [torch.zeros(2, nkv, CTX, hd, dtype=F16, device=toks.device) for _ in m.layers]
    vc = [t.clone() for t in kc]
    smp = qp.Sampler(2, mr.VOCAB, toks.device, temperature=0.0)
    return qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, sampler=smp, wide=256, **kw), smp, toks[:N], kc, vc


@gpu
@pytest.mark.parametrize("N", LENS)
def test_prefill_wide_attention(N):
    """the last row within model_reference's tolerance of the float64 forward (4 x the emulation's distance); the
    layer-0 caches byte-equal to Prefill(wide=256)'s; N = 300 (chunks of 256 + 44) also captured and replayed three times"""
    _, _, ref, emu = _model()
    pf, smp, toks, kc, vc = _prefill(N, wide_attention=True)
    tok = int(pf(toks, slot=1, pos0=0))
    rows = [n - 1 for n in LENS]
    rh, rl, i = ref.stream[0][-1][rows], ref.logits[0][rows], LENS.index(N)
    xh = float(mr.e_h(pf.last32, rh[i:i + 1]) / mr.tolerance(mr.e_h(emu.stream[0][-1][rows], rh))[i])
    xl = float(mr.e_l(smp.logits[1:2], rl[i:i + 1]) / mr.tolerance(mr.e_l(emu.logits[0][rows], rl))[i])
    print(f"Prefill(wide=256, wide_attention=True) N {N}: err / tol stream {xh:.3f}, logits {xl:.3f}")
    assert xh <= 1.0 and xl <= 1.0
    base, _, _, kc0, vc0 = _prefill(N)
    base(toks, slot=1, pos0=0)
    assert torch.equal(kc[0], kc0[0]) and torch.equal(vc[0], vc0[0]) and bool(kc[0][1, :, :N].float().abs().sum() > 0)
    if N == 300:
        torch.cuda.synchronize()
        s = torch.cuda.Stream(toks.device)
        with torch.cuda.stream(s):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                out = pf(toks, slot=1, pos0=0)
            for _ in range(3):
                out.fill_(-1)
                g.replay()
                torch.cuda.synchronize()
                assert int(out) == tok
