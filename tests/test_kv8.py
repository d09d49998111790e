"""The 8-bit KV cache (OCP e4m3fn): qpal_attn_rope_decode_batch_kv8 (csrc/attn_batch.hip), qpal_attn_rope_prefill_kv8
(csrc/attn_prefill.hip), their dispatch in qpalette_amd.attention and the decoder classes on float8_e4m3fn caches.

CPU: the symbols are exported and bound, every argument error of the fp16 siblings comes back with the same code, the Python layer
rejects mixed and foreign cache dtypes.
GPU: the appended bytes are torch's cast of the fp16 row qpal_rope_kv writes (h.float().clamp(-448, 448).to(float8_e4m3fn)),
saturating and subnormal inputs among them, every other byte unchanged; the output against fp32 torch attention over the
dequantised cache AFTER the launch with the fp16 tests' tolerance (dequantisation is exact, the arithmetic is the fp16 kernel's);
tickets, determinism, graph replay, inactive and independent sequences, the prefill fit rule; a cache filled by one prefill launch
is byte-identical to one filled token by token; the whole model against the torch-glue step on round-tripped caches."""
import math
import os
import sys

import pytest
import torch

import qpalette_amd as qp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_SHAPE, E_NULL, E_ALIGN = -1, -3, -4
F8 = torch.float8_e4m3fn
NAN8 = 0x7F  # the e4m3fn NaN byte


# ---------------------------------------------------------------------------------------------------------------- CPU

@pytest.fixture(scope="module")
def lib():
    return qp._native.lib()


def test_kv8_symbols_are_exported(lib):
    with open(os.path.join(ROOT, "include", "qpal.h")) as f:
        hdr = f.read()
    for name in ("qpal_attn_rope_decode_batch_kv8", "qpal_attn_rope_prefill_kv8"):
        assert name in qp._native.exported_symbols()
        assert hasattr(lib, name) and getattr(lib, name).argtypes == getattr(lib, name[:-4]).argtypes
        assert name + "(" in hdr


def _call(fn, q=16, k=16, v=16, ld=4096, kc=4096, vc=4096, out=16, ld_out=4096, pos=16, inv=16, B=4, nq=32, nkv=8, hd=128,
          L=1024, ws=16, ws_bytes=1 << 30):
    return fn(q, k, v, ld, kc, vc, out, ld_out, pos, inv, B, nq, nkv, hd, L, 0.1, ws, ws_bytes, None)


@pytest.mark.parametrize("name", ["qpal_attn_rope_decode_batch", "qpal_attn_rope_prefill"])
def test_kv8_argument_errors_are_the_fp16_siblings(lib, name):
    """the fp16 tests' list of perturbations (B stands for T in the prefill entry point): the same code from both entry points,
    before any stream work (the pointers are never dereferenced)"""
    f16, f8 = getattr(lib, name), getattr(lib, name + "_kv8")
    cases = [({"q": None}, E_NULL), ({"k": None}, E_NULL), ({"v": None}, E_NULL), ({"kc": None}, E_NULL), ({"vc": None}, E_NULL),
             ({"out": None}, E_NULL), ({"pos": None}, E_NULL), ({"inv": None}, E_NULL), ({"ws": None}, E_NULL)]
    cases += [(kw, E_SHAPE) for kw in ({"hd": 96}, {"hd": 32}, {"nq": 24}, {"nq": 48}, {"nq": 128}, {"B": 0}, {"B": 129}, {"L": 1022},
                                       {"L": 0}, {"hd": 256, "nq": 64}, {"ld": 4095}, {"ld_out": 100}, {"ws_bytes": 4})]
    cases += [(kw, E_ALIGN) for kw in ({"kc": 4096 + 8}, {"vc": 4096 + 2}, {"q": 18}, {"pos": 17}, {"out": 17}, {"ws": 18})]
    for kw, code in cases:
        assert _call(f8, **kw) == code == _call(f16, **kw), kw


def test_python_layer_rejects_mixed_and_foreign_cache_dtypes():
    z = torch.zeros
    dec = dict(q=z(2, 8), k=z(2, 8), v=z(2, 8), pos=z(2, dtype=torch.long), inv_freq=z(4))
    pre = dict(q=z(2, 8), k=z(2, 8), v=z(2, 8), pos0=z(1, dtype=torch.long), inv_freq=z(4))
    for fn, args, shape in ((qp.decode_attention, dec, (2, 1, 8, 8)), (qp.prefill_attention, pre, (1, 8, 8))):
        with pytest.raises(qp._native.QpalError, match="share one dtype"):
            fn(kcache=z(shape).to(F8), vcache=z(shape).half(), **args)
        with pytest.raises(qp._native.QpalError, match="share one dtype"):
            fn(kcache=z(shape).half(), vcache=z(shape).to(F8), **args)
        for dt in (torch.float8_e5m2, torch.bfloat16, torch.uint8):
            with pytest.raises(qp._native.QpalError, match="dtype must be"):
                fn(kcache=z(shape).to(dt), vcache=z(shape).to(dt), **args)
    assert qp.attention.kv_cache_bytes(64, 8, 4096, 128, F8) * 2 == qp.attention.kv_cache_bytes(64, 8, 4096, 128) == 1 << 29
    with pytest.raises(qp._native.QpalError):
        qp.attention.kv_cache_bytes(1, 1, 4, 64, torch.float8_e5m2)


# ---------------------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _inv_freq(hd, dev):
    return 1.0 / (500000.0 ** (torch.arange(0, hd, 2, device=dev).float() / hd))


def _positions(B, L, seed):
    """test_attn_batch.py's rule"""
    special = [p for p in (0, 63, 64, 511, 512, L - 1, 127, 128, 1023, 1024, 2047, 2048) if p < L]
    g = torch.Generator().manual_seed(seed)
    rnd = torch.randint(0, L, (B,), generator=g).tolist()
    return [special[b] if b < len(special) else rnd[b] for b in range(B)]


def _u8(t):
    return t.view(torch.uint8)


def _quant(h):
    """contract point 1: the byte stored for the fp16 value h"""
    return h.float().clamp(-448.0, 448.0).to(F8)


def _extremes(k, v, rows, hd):
    """in `rows` of the fp32 k / v inputs ([rows, nkv * hd], views): dims 0..7 of both rotary halves of kv head 0 times 1e3 (they
    saturate), dims 8..15 times 1e-3 (e4m3 subnormals: below 2^-6)"""
    half = hd // 2
    for r in rows:
        for t in (k, v):
            for base in (0, half):
                t[r, base:base + 8] *= 1e3
                t[r, base + 8:base + 16] *= 1e-3


def _assert_extremes(exp_rows):
    """the compared bytes hold +448, -448 and nonzero subnormals"""
    b = _u8(exp_rows)
    assert bool((b == 0x7E).any()) and bool((b == 0xFE).any()), "no saturated byte among the expected rows"
    assert bool((((b & 0x7F) >= 1) & ((b & 0x7F) <= 7)).any()), "no subnormal byte among the expected rows"


def _setup(dev, B, nq, nkv, hd, L, pos, seed, extreme=()):
    """test_attn_batch.py's _setup with e4m3 caches: a padded row stride, random context, the NaN byte in the rows about to be
    written"""
    gen = torch.Generator(device=dev).manual_seed(seed)
    W = nq * hd + 2 * nkv * hd
    qkv = torch.randn(B, W + 8, device=dev, generator=gen)
    q, k, v = qkv[:, :nq * hd], qkv[:, nq * hd:nq * hd + nkv * hd], qkv[:, nq * hd + nkv * hd:W]
    _extremes(k, v, extreme, hd)
    kc = (torch.randn(B, nkv, L, hd, device=dev, generator=gen) * 0.5).to(F8)
    vc = (torch.randn(B, nkv, L, hd, device=dev, generator=gen) * 0.5).to(F8)
    for b, p in enumerate(pos):
        if 0 <= p < L:
            _u8(kc)[b, :, p] = NAN8
            _u8(vc)[b, :, p] = NAN8
    return q, k, v, kc, vc, torch.tensor(pos, dtype=torch.long, device=dev)


def _rope_kv_rows(q, k, v, positions, inv_freq, nq, nkv, hd, L):
    """qpal_rope_kv on every row alone at its position (into one fp16 scratch cache): the fp16 k / v rows it writes [rows, nkv, hd]
    and the fp16 q after the rotary embedding; rows with a position outside the cache are skipped (zeros)"""
    nat = qp._native
    n, dev = q.shape[0], q.device
    kr = torch.zeros(n, nkv, hd, dtype=torch.float16, device=dev)
    vr = torch.zeros_like(kr)
    q16 = torch.zeros(n, nq * hd, dtype=torch.float16, device=dev)
    ks = torch.zeros(nkv, L, hd, dtype=torch.float16, device=dev)
    vs = torch.zeros_like(ks)
    qc, kk, vv = q.contiguous(), k.contiguous(), v.contiguous()
    pos_t = torch.tensor(positions, dtype=torch.long, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for i, p in enumerate(positions):
        if not 0 <= p < L:
            continue
        nat.check(nat.lib().qpal_rope_kv(qc[i].data_ptr(), kk[i].data_ptr(), vv[i].data_ptr(), q16[i].data_ptr(), ks.data_ptr(),
                                         vs.data_ptr(), pos_t[i:i + 1].data_ptr(), inv_freq.data_ptr(), nq, nkv, hd, L, stream),
                  "qpal_rope_kv")
        kr[i], vr[i] = ks[:, p], vs[:, p]
    return kr, vr, q16


def _decode_reference(q16, kc, vc, pos, nq, nkv, hd):
    """softmax(q k^T / sqrt(hd)) v over 0 .. pos[b] of the dequantised cache, fp32"""
    B, L = kc.shape[0], kc.shape[2]
    out = torch.zeros(B, nq * hd, device=q16.device)
    for b, p in enumerate(pos):
        if not 0 <= p < L:
            continue
        qf = q16[b].view(nq, 1, hd).float()
        kf = kc[b, :, : p + 1].float().repeat_interleave(nq // nkv, dim=0)
        vf = vc[b, :, : p + 1].float().repeat_interleave(nq // nkv, dim=0)
        out[b] = (torch.softmax(qf @ kf.transpose(-1, -2) / math.sqrt(hd), dim=-1) @ vf).view(-1)
    return out


DECODE = [(8, 16, 2, 64, 128), (16, 32, 8, 128, 512), (1, 32, 8, 128, 2048), (64, 32, 8, 128, 2048), (8, 16, 4, 256, 4096),
          (8, 8, 1, 128, 4096)]  # B, nq, nkv, hd, max_len


@pytest.mark.gpu
@pytest.mark.parametrize("B,nq,nkv,hd,L", DECODE)
def test_decode_kv8_appends_torchs_bytes_and_matches_torch(dev, B, nq, nkv, hd, L):
    pos = _positions(B, L, seed=B * 131 + L)
    extreme = sorted({0, B - 1})  # two sequences (one where B = 1)
    q, k, v, kc, vc, pos_t = _setup(dev, B, nq, nkv, hd, L, pos, seed=B + nq + L, extreme=extreme)
    inv_freq = _inv_freq(hd, dev)
    kr, vr, q16 = _rope_kv_rows(q, k, v, pos, inv_freq, nq, nkv, hd, L)
    kc_exp, vc_exp = kc.clone(), vc.clone()
    rows = torch.arange(B, device=dev)
    _u8(kc_exp)[rows, :, pos_t] = _u8(_quant(kr))
    _u8(vc_exp)[rows, :, pos_t] = _u8(_quant(vr))
    _assert_extremes(_quant(kr[extreme]))
    _assert_extremes(_quant(vr[extreme]))
    kc0, vc0 = kc.clone(), vc.clone()
    ws = qp.attention_workspace(B, nq, nkv, hd, L, dev)
    out = qp.decode_attention(q, k, v, kc, vc, pos_t, inv_freq, ws=ws)
    torch.cuda.synchronize()
    # the append: row pos[b] byte for byte torch's cast of qpal_rope_kv's fp16 row, every other byte unchanged
    bad_k, bad_v = int((_u8(kc) != _u8(kc_exp)).sum()), int((_u8(vc) != _u8(vc_exp)).sum())
    assert bad_k == 0 and bad_v == 0, (bad_k, bad_v)
    ref = _decode_reference(q16, kc, vc, pos, nq, nkv, hd)
    err = float((out.float() - ref).abs().max())
    print(f"kv8 decode parity {(B, nq, nkv, hd, L)}: max |diff| = {err:.3e}")
    assert torch.allclose(out.float(), ref, atol=2e-3, rtol=2e-3), err
    if ws is not None:
        assert int(ws[: 128 * nkv].abs().max()) == 0, "tickets must be back at zero after a launch"
    # a second launch on the restored state: bitwise the same
    out2 = qp.decode_attention(q, k, v, kc0, vc0, pos_t, inv_freq, ws=ws)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), out2.view(torch.int16))
    assert torch.equal(_u8(kc0), _u8(kc_exp)) and torch.equal(_u8(vc0), _u8(vc_exp))


@pytest.mark.gpu
@pytest.mark.parametrize("L", [256, 4096])
def test_kv8_inactive_and_independent_sequences(dev, L):
    nq, nkv, hd, B = 32, 8, 128, 6
    pos = [5, -1, L, L - 1, 1 << 40, 300]
    q, k, v, kc, vc, pos_t = _setup(dev, B, nq, nkv, hd, L, pos, seed=L)
    inv_freq = _inv_freq(hd, dev)
    ws = qp.attention_workspace(B, nq, nkv, hd, L, dev)
    kc0, vc0 = kc.clone(), vc.clone()
    out = torch.full((B, nq * hd), 3.0, dtype=torch.float16, device=dev)
    qp.decode_attention(q, k, v, kc, vc, pos_t, inv_freq, out=out, ws=ws)
    torch.cuda.synchronize()
    active = [b for b, p in enumerate(pos) if 0 <= p < L]  # 300 is past the end of the 256 cache: slot 5 is inactive there
    assert set(active) == ({0, 3} if L == 256 else {0, 3, 5})
    for b in range(B):
        if b in active:  # a finite row, the NaN bytes at pos[b] replaced in both caches
            assert bool(torch.isfinite(out[b]).all()) and not bool((out[b] == 3.0).all())
            assert not bool((_u8(kc[b, :, pos[b]]) == NAN8).any()) and not bool((_u8(vc[b, :, pos[b]]) == NAN8).any())
        else:  # inactive: output row and caches untouched
            assert bool((out[b] == 3.0).all())
            assert torch.equal(_u8(kc[b]), _u8(kc0[b])) and torch.equal(_u8(vc[b]), _u8(vc0[b]))
    # changing sequence j's inputs (new q / k / v and its cached rows) leaves every other row bitwise as it was
    j = 3
    gen = torch.Generator(device=dev).manual_seed(L + 1)
    kcj, vcj = kc0.clone(), vc0.clone()
    kcj[j] = (torch.randn(nkv, L, hd, device=dev, generator=gen) * 0.5).to(F8)
    vcj[j] = (torch.randn(nkv, L, hd, device=dev, generator=gen) * 0.5).to(F8)
    qkv2 = torch.cat([q, k, v], dim=1)
    q2, k2, v2 = qkv2.split([nq * hd, nkv * hd, nkv * hd], dim=1)
    q2[j] += 1.0
    k2[j] -= 1.0
    v2[j] *= 2.0
    out2 = torch.full((B, nq * hd), 3.0, dtype=torch.float16, device=dev)
    qp.decode_attention(q2, k2, v2, kcj, vcj, pos_t, inv_freq, out=out2, ws=ws)
    torch.cuda.synchronize()
    others = [b for b in range(B) if b != j]
    assert torch.equal(out[others].view(torch.int16), out2[others].view(torch.int16))
    assert not torch.equal(out[j], out2[j])
    assert torch.equal(_u8(kc[others]), _u8(kcj[others])) and torch.equal(_u8(vc[others]), _u8(vcj[others]))
    if ws is not None:
        assert int(ws[: 128 * nkv].abs().max()) == 0


@pytest.mark.gpu
def test_kv8_graph_replay_with_positions_advanced_on_the_device(dev):
    """test_attn_batch.py's pattern on e4m3 caches: a captured launch replayed with pos advanced on the device equals eager
    launches; two replays are bitwise equal"""
    B, nq, nkv, hd, L = 8, 32, 8, 128, 4096
    pos = _positions(B, L - 4, seed=11)
    pos[5] = -1
    q, k, v, kc, vc, pos_t = _setup(dev, B, nq, nkv, hd, L, pos, seed=12)
    inv_freq = _inv_freq(hd, dev)
    ws = qp.attention_workspace(B, nq, nkv, hd, L, dev)
    inc = (pos_t >= 0).long()
    kc_e, vc_e, pos_e = kc.clone(), vc.clone(), pos_t.clone()
    eager = []
    for _ in range(3):
        o = torch.zeros(B, nq * hd, dtype=torch.float16, device=dev)
        eager.append(qp.decode_attention(q, k, v, kc_e, vc_e, pos_e, inv_freq, out=o, ws=ws))
        pos_e += inc
    torch.cuda.synchronize()  # (one workspace serves launches of ONE stream at a time)
    out = torch.zeros(B, nq * hd, dtype=torch.float16, device=dev)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        kc_w, vc_w = kc.clone(), vc.clone()
        qp.decode_attention(q, k, v, kc_w, vc_w, pos_t, inv_freq, out=out, ws=ws)  # warm-up on scratch caches
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            qp.decode_attention(q, k, v, kc, vc, pos_t, inv_freq, out=out, ws=ws)
        got = []
        for _ in range(3):
            g.replay()
            got.append(out.clone())
            pos_t += inc
        torch.cuda.synchronize()
        pos_t -= inc
        g.replay()  # the last position again: same bytes rewritten, same output
        again = out.clone()
        torch.cuda.synchronize()
    for a, b in zip(eager, got):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert torch.equal(again.view(torch.int16), got[-1].view(torch.int16))
    assert torch.equal(_u8(kc), _u8(kc_e)) and torch.equal(_u8(vc), _u8(vc_e))
    assert int(ws[: 128 * nkv].abs().max()) == 0


# ------------------------------------------------------------------------------------------------------------ prefill

HEADS = [(32, 8, 128), (8, 8, 64), (16, 4, 256)]
TS = [1, 5, 16, 17, 128]
POS0_L = [(0, 256), (37, 256), (500, 2048), (1920, 2048)]  # the 2048 cases are split; T = 17 / 128 from 500 cross 512


def _setup_prefill(dev, T, nq, nkv, hd, L, pos0, seed, extreme=()):
    gen = torch.Generator(device=dev).manual_seed(seed)
    W = nq * hd + 2 * nkv * hd
    qkv = torch.randn(T, W + 8, device=dev, generator=gen)
    q, k, v = qkv[:, :nq * hd], qkv[:, nq * hd:nq * hd + nkv * hd], qkv[:, nq * hd + nkv * hd:W]
    _extremes(k, v, extreme, hd)
    kc = (torch.randn(nkv, L, hd, device=dev, generator=gen) * 0.5).to(F8)
    vc = (torch.randn(nkv, L, hd, device=dev, generator=gen) * 0.5).to(F8)
    if 0 <= pos0 and pos0 + T <= L:
        _u8(kc)[:, pos0:pos0 + T] = NAN8
        _u8(vc)[:, pos0:pos0 + T] = NAN8
    return q, k, v, kc, vc, torch.tensor([pos0], dtype=torch.long, device=dev)


def _prefill_reference(q16, kc, vc, pos0, nq, nkv, hd):
    """row t: softmax(q k^T / sqrt(hd)) v over 0 .. pos0 + t of the dequantised cache (causal), fp32"""
    T, n = q16.shape[0], pos0 + q16.shape[0]
    qf = q16.view(T, nq, hd).float().transpose(0, 1)
    kf = kc[:, :n].float().repeat_interleave(nq // nkv, dim=0)
    vf = vc[:, :n].float().repeat_interleave(nq // nkv, dim=0)
    s = qf @ kf.transpose(-1, -2) / math.sqrt(hd)
    keep = torch.arange(n, device=s.device)[None, :] <= (pos0 + torch.arange(T, device=s.device))[:, None]
    s = s.masked_fill(~keep[None], float("-inf"))
    return (torch.softmax(s, dim=-1) @ vf).transpose(0, 1).reshape(T, nq * hd)


@pytest.mark.gpu
@pytest.mark.parametrize("pos0,L", POS0_L)
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("nq,nkv,hd", HEADS)
def test_prefill_kv8_appends_torchs_bytes_and_matches_torch(dev, nq, nkv, hd, T, pos0, L):
    extreme = sorted({0, T - 1})
    q, k, v, kc, vc, pos_t = _setup_prefill(dev, T, nq, nkv, hd, L, pos0, seed=T + nq + L + pos0, extreme=extreme)
    inv_freq = _inv_freq(hd, dev)
    kr, vr, q16 = _rope_kv_rows(q, k, v, list(range(pos0, pos0 + T)), inv_freq, nq, nkv, hd, L)
    kc_exp, vc_exp = kc.clone(), vc.clone()
    _u8(kc_exp)[:, pos0:pos0 + T] = _u8(_quant(kr)).transpose(0, 1)
    _u8(vc_exp)[:, pos0:pos0 + T] = _u8(_quant(vr)).transpose(0, 1)
    _assert_extremes(_quant(kr[extreme]))
    _assert_extremes(_quant(vr[extreme]))
    kc0, vc0 = kc.clone(), vc.clone()
    ws = qp.prefill_workspace(T, nq, nkv, hd, L, dev)
    out = qp.prefill_attention(q, k, v, kc, vc, pos_t, inv_freq, ws=ws)
    torch.cuda.synchronize()
    bad_k, bad_v = int((_u8(kc) != _u8(kc_exp)).sum()), int((_u8(vc) != _u8(vc_exp)).sum())
    assert bad_k == 0 and bad_v == 0, (bad_k, bad_v)
    ref = _prefill_reference(q16, kc, vc, pos0, nq, nkv, hd)
    err = float((out.float() - ref).abs().max())
    print(f"kv8 prefill parity {(nq, nkv, hd)} T={T} pos0={pos0} L={L}: max |diff| = {err:.3e}")
    assert torch.allclose(out.float(), ref, atol=2e-3, rtol=2e-3), err  # tests/test_prefill.py's tolerance
    if ws is not None:
        assert int(ws[: 8 * nkv].abs().max()) == 0, "tickets must be back at zero after a launch"
    out2 = qp.prefill_attention(q, k, v, kc0, vc0, pos_t, inv_freq, ws=ws)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), out2.view(torch.int16)) and torch.equal(_u8(kc0), _u8(kc_exp))


@pytest.mark.gpu
@pytest.mark.parametrize("L,T", [(256, 16), (2048, 128), (2048, 1)])
def test_prefill_kv8_fit_rule(dev, L, T):
    nq, nkv, hd = 32, 8, 128
    inv_freq = _inv_freq(hd, dev)
    ws = qp.prefill_workspace(T, nq, nkv, hd, L, dev)
    for pos0 in (-1, L - T + 1, 1 << 40):
        q, k, v, kc, vc, pos_t = _setup_prefill(dev, T, nq, nkv, hd, L, pos0, seed=L)
        kc0, vc0 = kc.clone(), vc.clone()
        out = torch.full((T, nq * hd), 3.0, dtype=torch.float16, device=dev)
        qp.prefill_attention(q, k, v, kc, vc, pos_t, inv_freq, out=out, ws=ws)
        torch.cuda.synchronize()
        assert bool((out == 3.0).all()), pos0
        assert torch.equal(_u8(kc), _u8(kc0)) and torch.equal(_u8(vc), _u8(vc0)), pos0
    if ws is not None:
        assert int(ws.abs().max()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("T,pos0,L", [(5, 0, 256), (128, 37, 256), (17, 500, 2048)])
@pytest.mark.parametrize("nq,nkv,hd", HEADS)
def test_one_prefill_launch_equals_token_by_token_decode(dev, nq, nkv, hd, T, pos0, L):
    """contract point 3: a position has one value whichever kernel reads it — the same q|k|v rows as one prefill launch and as T
    decode_attention launches at B = 1 leave byte-identical caches, and the outputs agree within the decode tolerance"""
    q, k, v, kc, vc, pos_t = _setup_prefill(dev, T, nq, nkv, hd, L, pos0, seed=7 * T + L, extreme=[0, T - 1])
    inv_freq = _inv_freq(hd, dev)
    kc1, vc1 = kc.clone()[None], vc.clone()[None]
    out = qp.prefill_attention(q, k, v, kc, vc, pos_t, inv_freq, ws=qp.prefill_workspace(T, nq, nkv, hd, L, dev))
    ws1 = qp.attention_workspace(1, nq, nkv, hd, L, dev)
    out1 = torch.zeros_like(out)
    p1 = pos_t.clone()
    for t in range(T):
        qp.decode_attention(q[t:t + 1], k[t:t + 1], v[t:t + 1], kc1, vc1, p1, inv_freq, out=out1[t:t + 1], ws=ws1)
        p1 += 1
    torch.cuda.synchronize()
    assert torch.equal(_u8(kc), _u8(kc1[0])) and torch.equal(_u8(vc), _u8(vc1[0]))
    err = float((out.float() - out1.float()).abs().max())
    assert torch.allclose(out.float(), out1.float(), atol=2e-3, rtol=2e-3), err


# -------------------------------------------------------------------------------------------------------- whole model

@pytest.mark.gpu
@pytest.mark.parametrize("model", ["3_8b", "3_70b"])
def test_kv8_decode_step_matches_torch_glue_step_on_round_tripped_caches(dev, model):
    """perf/decode_llama_batch.py --kv fp8: the final-norm state of the active sequences against the torch-glue step whose
    BatchKV.update stores new rows through the e4m3 round trip.  Bound: the project's 2^-7 max(1, max |ref|).  Measured on an
    MI355X: 3_8b 0.0039 (max |ref| 3.79; the fp16-cache step against the same reference 0.0039), 3_70b 0.0039 (max |ref| 3.94;
    fp16-cache step 0.0063): inside the bound (~0.030), so it stays."""
    sys.path.insert(0, os.path.join(ROOT, "perf"))
    import decode_llama_batch
    res = decode_llama_batch.main(["--model", model, "--layers", "2", "--batch", "4", "--inactive", "1", "--context", "128",
                                   "--tokens", "4", "--vocab", "4096", "--kv", "fp8"], quiet=True)
    (r,) = res["batches"]
    chk = r["check"]
    print(model, chk)
    assert r["kv"] == "fp8" and r["active"] == 3 and r["ms_step"] > 0
    assert chk is not None and chk["finite"]
    assert chk["max_abs_diff_final_norm"] <= 2.0 ** -7 * max(1.0, chk["max_abs_ref"]), chk


@pytest.fixture(scope="module")
def model(dev):
    sys.path.insert(0, os.path.join(ROOT, "perf"))
    from decode_llama import build_model
    return build_model("3_8b", "tcomb_6_7_0.5_none_0.9", None, 2, 4096, dev)


def _caches(m, B, L, dev, dtype):
    nkv, hd = m.cfg.num_key_value_heads, m.cfg.head_dim
    gen = torch.Generator(device=dev).manual_seed(3)
    mk = lambda: [(torch.randn(B, nkv, L, hd, device=dev, generator=gen) * 0.5).to(dtype) for _ in m.layers]  # noqa: E731
    return mk(), mk()


@pytest.mark.gpu
def test_prefill_then_decode_step_on_kv8_caches(dev, model):
    """Prefill fills one slot of float8_e4m3fn caches and a DecodeStep (batch B, and the batch-1 step with all its GEMV fusions)
    continues on the same caches: finite tokens, no byte of another slot written"""
    m, B, L, N, slot = model, 3, 256, 150, 1
    kc, vc = _caches(m, B, L, dev, F8)
    kc0, vc0 = [t.clone() for t in kc], [t.clone() for t in vc]
    toks = torch.randint(0, 4096, (N,), generator=torch.Generator().manual_seed(5)).to(dev)
    pf = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, chunk=128)
    nxt = pf(toks, slot=slot, pos0=0)
    tok = torch.zeros(B, dtype=torch.long, device=dev)
    tok[slot] = nxt[0]
    pos = torch.tensor([-1, N, -1], dtype=torch.long, device=dev)
    out_tok = torch.full((B,), -7, dtype=torch.long, device=dev)
    step = qp.DecodeStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, tok, pos, out_tok)
    step()
    torch.cuda.synchronize()
    assert 0 <= int(nxt[0]) < 4096 and 0 <= int(out_tok[slot]) < 4096
    assert bool(torch.isfinite(pf.hidden()).all()) and bool(torch.isfinite(step.hidden()[slot]).all())
    others = [b for b in range(B) if b != slot]
    for t, t0 in zip(kc + vc, kc0 + vc0):
        assert torch.equal(_u8(t[others]), _u8(t0[others]))
        assert not torch.equal(_u8(t[slot, :, :N + 1]), _u8(t0[slot, :, :N + 1]))
        assert torch.equal(_u8(t[slot, :, N + 1:]), _u8(t0[slot, :, N + 1:]))
    # the batch-1 step on the slot's caches alone: same launch count as on fp16 caches, a finite token
    k1, v1 = [t[slot:slot + 1].clone() for t in kc], [t[slot:slot + 1].clone() for t in vc]
    tok1, pos1, out1 = out_tok[slot:slot + 1].clone(), torch.tensor([N + 1], device=dev), torch.zeros(1, dtype=torch.long, device=dev)
    s8 = qp.DecodeStep(m.layers, m.embed, m.norm, m.lm_head, k1, v1, m.inv_freq, tok1, pos1, out1)
    s16 = qp.DecodeStep(m.layers, m.embed, m.norm, m.lm_head, [t.half() for t in k1], [t.half() for t in v1], m.inv_freq, tok1, pos1,
                        torch.zeros_like(out1))
    assert s8.batch1 and s8.launches_per_token == s16.launches_per_token
    s8()
    torch.cuda.synchronize()
    assert 0 <= int(out1[0]) < 4096 and bool(torch.isfinite(s8.hidden()).all())
    for t, t0 in zip(k1 + v1, kc + vc):
        assert not torch.equal(_u8(t[0, :, N + 1]), _u8(t0[slot, :, N + 1])) and torch.equal(_u8(t[0, :, :N + 1]), _u8(t0[slot, :, :N + 1]))


@pytest.mark.gpu
def test_score_on_kv8_caches(dev, model):
    """Score on float8_e4m3fn caches: finite log-probs of the right shape.  Their mean distance from the fp16-cache Score of the same
    model and tokens is printed (DESIGN.md §16 records it: mean 2.0e-4, max 9.4e-4 at a mean log-prob of -9.05); it is not a gate."""
    m, B, L, N = model, 2, 256, 200
    toks = torch.randint(0, 4096, (N,), generator=torch.Generator().manual_seed(9)).to(dev)
    lps = {}
    for dtype in (torch.float16, F8):
        kc, vc = _caches(m, B, L, dev, dtype)
        sc = qp.Score(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, chunk=128)
        lps[dtype] = sc(toks, slot=1, pos0=0).clone()
    torch.cuda.synchronize()
    lp8, lp16 = lps[F8], lps[torch.float16]
    assert lp8.shape == (N - 1,) and lp8.dtype == torch.float32
    assert bool(torch.isfinite(lp8).all()) and bool((lp8 <= 0).all())
    print(f"kv8 Score: mean |lp8 - lp16| = {float((lp8 - lp16).abs().mean()):.4e}, max = {float((lp8 - lp16).abs().max()):.4e}, "
          f"mean lp16 = {float(lp16.mean()):.4f}, mean lp8 = {float(lp8.mean()):.4f}")
