"""Batched decode attention (csrc/attn_batch.hip, qpalette_amd.attention) and the whole-model decode step at batch B
(perf/decode_llama_batch.py).

CPU: the C-ABI is exported, the workspace size is consistent, argument errors are return codes.
GPU: parity with a torch fp32 restatement, the cache append is bit for bit qpal_rope_kv's, inactive and independent sequences,
agreement with the batch-1 entry point, graph replay and determinism, and the whole step against the torch-glue step."""
import math
import os
import sys

import pytest
import torch

import qpalette_amd as qp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_SHAPE, E_NULL, E_ALIGN = -1, -3, -4


# ---------------------------------------------------------------------------------------------------------------- CPU

@pytest.fixture(scope="module")
def lib():
    return qp._native.lib()


def test_batch_attention_symbols_are_exported(lib):
    for name in ("qpal_attn_rope_decode_batch", "qpal_attn_batch_ws_bytes"):
        assert name in qp._native.exported_symbols()
        assert hasattr(lib, name)
    assert callable(qp.decode_attention) and callable(qp.attention_workspace)


def test_batch_workspace_size_is_consistent(lib):
    ws = lib.qpal_attn_batch_ws_bytes
    for nq, nkv, hd in [(32, 8, 128), (64, 8, 128), (8, 8, 64), (16, 2, 64), (16, 4, 256), (8, 1, 128)]:
        for L in (4, 128, 508):  # short caches: one chunk per (sequence, kv head), no workspace
            assert all(ws(B, nq, nkv, hd, L) == 0 for B in (1, 8, 128))
        for L in (512, 1024, 2048, 4096, 32768):
            sizes = [ws(B, nq, nkv, hd, L) for B in range(1, 129)]
            assert all(s > 0 and s % 4 == 0 for s in sizes)
            assert all(a <= b for a, b in zip(sizes, sizes[1:])), (nq, nkv, hd, L)  # monotone in B
        for B in (1, 7, 64, 128):
            sizes = [ws(B, nq, nkv, hd, L) for L in range(4, 65536 + 4, 508)]
            assert all(a <= b for a, b in zip(sizes, sizes[1:])), (nq, nkv, hd, B)  # monotone in max_len
    # no workspace for shapes the launch rejects
    assert ws(0, 32, 8, 128, 4096) == 0 and ws(129, 32, 8, 128, 4096) == 0 and ws(4, 24, 8, 128, 4096) == 0
    assert ws(4, 32, 8, 96, 4096) == 0 and ws(4, 32, 8, 128, 4098) == 0 and ws(4, 64, 8, 256, 4096) == 0


def _call(lib, q=16, k=16, v=16, ld=4096, kc=4096, vc=4096, out=16, ld_out=4096, pos=16, inv=16, B=4, nq=32, nkv=8, hd=128,
          L=1024, ws=16, ws_bytes=1 << 30):
    return lib.qpal_attn_rope_decode_batch(q, k, v, ld, kc, vc, out, ld_out, pos, inv, B, nq, nkv, hd, L, 0.1, ws, ws_bytes, None)


def test_batch_attention_argument_errors_without_a_gpu(lib):
    """Every argument error is returned before any stream work (the pointers below are never dereferenced)."""
    for kw in ({"q": None}, {"k": None}, {"v": None}, {"kc": None}, {"vc": None}, {"out": None}, {"pos": None}, {"inv": None}):
        assert _call(lib, **kw) == E_NULL, kw
    assert _call(lib, ws=None) == E_NULL  # 1024 positions: the split form needs its workspace
    for kw in ({"hd": 96}, {"hd": 32}, {"nq": 24}, {"nq": 48}, {"nq": 128}, {"B": 0}, {"B": 129}, {"L": 1022}, {"L": 0},
               {"hd": 256, "nq": 64}, {"ld": 4095}, {"ld_out": 100}, {"ws_bytes": 4}):
        assert _call(lib, **kw) == E_SHAPE, kw
    for kw in ({"kc": 4096 + 8}, {"vc": 4096 + 2}, {"q": 18}, {"pos": 17}, {"out": 17}, {"ws": 18}):
        assert _call(lib, **kw) == E_ALIGN, kw
    with pytest.raises(qp._native.QpalError):  # the Python layer checks before the library is reached
        qp.decode_attention(torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros(2, 1, 8, 8).half(),
                            torch.zeros(2, 1, 8, 8).half(), torch.zeros(2, dtype=torch.long), torch.zeros(4))


# ---------------------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _rotate_half(x):
    x1, x2 = x[..., : x.shape[-1] // 2], x[..., x.shape[-1] // 2:]
    return torch.cat((-x2, x1), dim=-1)


def _inv_freq(hd, dev):
    return 1.0 / (500000.0 ** (torch.arange(0, hd, 2, device=dev).float() / hd))


def _positions(B, L, seed):
    special = [p for p in (0, 63, 64, 511, 512, L - 1, 127, 128, 1023, 1024, 2047, 2048) if p < L]
    g = torch.Generator().manual_seed(seed)
    rnd = torch.randint(0, L, (B,), generator=g).tolist()
    return [special[b] if b < len(special) else rnd[b] for b in range(B)]


def _setup(dev, B, nq, nkv, hd, L, pos, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    W = nq * hd + 2 * nkv * hd
    qkv = torch.randn(B, W + 8, device=dev, generator=gen)  # a padded row stride: q / k / v are column slices
    q, k, v = qkv[:, :nq * hd], qkv[:, nq * hd:nq * hd + nkv * hd], qkv[:, nq * hd + nkv * hd:W]
    kc = (torch.randn(B, nkv, L, hd, device=dev, generator=gen) * 0.5).half()
    vc = (torch.randn(B, nkv, L, hd, device=dev, generator=gen) * 0.5).half()
    for b, p in enumerate(pos):
        if 0 <= p < L:  # whatever the cache holds at the new position must not matter
            kc[b, :, p] = float("nan")
            vc[b, :, p] = float("nan")
    pos_t = torch.tensor(pos, dtype=torch.long, device=dev)
    return q, k, v, kc, vc, pos_t


def _rope_kv_per_sequence(q, k, v, kc, vc, pos, inv_freq, nq, nkv, hd):
    """qpal_rope_kv on every active sequence alone: (expected caches, fp16 q after the rotary embedding)"""
    nat = qp._native
    B, L = kc.shape[0], kc.shape[2]
    kc_ref, vc_ref = kc.clone(), vc.clone()
    q16 = torch.zeros(B, nq * hd, dtype=torch.float16, device=kc.device)
    qc, kk, vv = q.contiguous(), k.contiguous(), v.contiguous()
    stream = torch.cuda.current_stream(kc.device).cuda_stream
    for b in range(B):
        nat.check(nat.lib().qpal_rope_kv(qc[b].data_ptr(), kk[b].data_ptr(), vv[b].data_ptr(), q16[b].data_ptr(), kc_ref[b].data_ptr(),
                                         vc_ref[b].data_ptr(), pos[b:b + 1].data_ptr(), inv_freq.data_ptr(), nq, nkv, hd, L, stream),
                  "qpal_rope_kv")
    return kc_ref, vc_ref, q16


def _attention_reference(q16, kc_ref, vc_ref, pos, nq, nkv, hd):
    """softmax(q k^T / sqrt(hd)) v over 0 .. pos[b] of the fp16 cache, fp32"""
    B, L = kc_ref.shape[0], kc_ref.shape[2]
    out = torch.zeros(B, nq * hd, device=q16.device)
    for b, p in enumerate(pos.tolist()):
        if not 0 <= p < L:
            continue
        qf = q16[b].view(nq, 1, hd).float()
        kf = kc_ref[b, :, : p + 1].float().repeat_interleave(nq // nkv, dim=0)
        vf = vc_ref[b, :, : p + 1].float().repeat_interleave(nq // nkv, dim=0)
        out[b] = (torch.softmax(qf @ kf.transpose(-1, -2) / math.sqrt(hd), dim=-1) @ vf).view(-1)
    return out


def _torch_rope_q(q, pos, inv_freq, nq, hd):
    ang = pos.clamp(min=0).float()[:, None] * inv_freq[None, :]
    emb = torch.cat((ang, ang), dim=-1)[:, None]
    qh = q.half().view(-1, nq, hd)
    return (qh * emb.cos().half() + _rotate_half(qh) * emb.sin().half()).view(-1, nq * hd)


PARITY = [  # B, nq, nkv, hd, max_len
    (1, 32, 8, 128, 2048), (3, 64, 8, 128, 32768), (3, 32, 8, 128, 32768), (8, 8, 8, 64, 2048), (8, 16, 2, 64, 128),
    (64, 32, 8, 128, 2048), (64, 16, 2, 64, 128), (128, 32, 8, 128, 128), (128, 64, 8, 128, 2048), (8, 16, 4, 256, 4096),
    (8, 8, 1, 128, 4096), (16, 32, 8, 128, 512),
]


@pytest.mark.gpu
@pytest.mark.parametrize("B,nq,nkv,hd,L", PARITY)
def test_batch_attention_matches_torch_and_appends_like_rope_kv(dev, B, nq, nkv, hd, L):
    pos = _positions(B, L, seed=B * 131 + L)
    q, k, v, kc, vc, pos_t = _setup(dev, B, nq, nkv, hd, L, pos, seed=B + nq + L)
    inv_freq = _inv_freq(hd, dev)
    kc_ref, vc_ref, q16 = _rope_kv_per_sequence(q, k, v, kc, vc, pos_t, inv_freq, nq, nkv, hd)
    ws = qp.attention_workspace(B, nq, nkv, hd, L, dev)
    out = qp.decode_attention(q, k, v, kc, vc, pos_t, inv_freq, ws=ws)
    torch.cuda.synchronize()
    # the cache append: row pos[b] bit for bit what qpal_rope_kv writes, every other byte unchanged
    assert torch.equal(kc.view(torch.int16), kc_ref.view(torch.int16)) and torch.equal(vc.view(torch.int16), vc_ref.view(torch.int16))
    ref = _attention_reference(q16, kc_ref, vc_ref, pos_t, nq, nkv, hd)
    assert torch.allclose(out.float(), ref, atol=2e-3, rtol=2e-3), float((out.float() - ref).abs().max())
    # the same against q rotated by torch (cos / sin in torch's fp32 instead of the device's: <= 1 fp16 ulp apart)
    ref_t = _attention_reference(_torch_rope_q(q, pos_t, inv_freq, nq, hd), kc_ref, vc_ref, pos_t, nq, nkv, hd)
    assert torch.allclose(out.float(), ref_t, atol=4e-3, rtol=4e-3)
    if ws is not None:
        assert int(ws[: 128 * nkv].abs().max()) == 0, "tickets must be back at zero after a launch"
    # a second launch on the restored state: bitwise the same (fixed merge order, no float atomics)
    for b, p in enumerate(pos):
        kc[b, :, p] = float("nan")
        vc[b, :, p] = float("nan")
    out2 = qp.decode_attention(q, k, v, kc, vc, pos_t, inv_freq, ws=ws)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), out2.view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("B,nq,nkv,hd,L", [(5, 32, 8, 128, 4096), (4, 64, 8, 128, 1024), (3, 8, 8, 64, 256), (4, 16, 4, 256, 2048)])
def test_batch_attention_agrees_with_batch_one(dev, B, nq, nkv, hd, L):
    """every sequence's row equals qpal_attn_rope_decode run on that sequence alone"""
    nat = qp._native
    pos = _positions(B, L, seed=7 * B + L)
    q, k, v, kc, vc, pos_t = _setup(dev, B, nq, nkv, hd, L, pos, seed=3 * B + L)
    inv_freq = _inv_freq(hd, dev)
    kc1, vc1 = kc.clone(), vc.clone()
    out = qp.decode_attention(q, k, v, kc, vc, pos_t, inv_freq, ws=qp.attention_workspace(B, nq, nkv, hd, L, dev))
    wsb = nat.lib().qpal_attn_ws_bytes(nq, nkv, hd, L)
    ws1 = torch.zeros(max(wsb, 4) // 4, device=dev)
    qc, kk, vv = q.contiguous(), k.contiguous(), v.contiguous()
    stream = torch.cuda.current_stream(dev).cuda_stream
    for b in range(B):
        o1 = torch.empty(nq * hd, dtype=torch.float16, device=dev)
        nat.check(nat.lib().qpal_attn_rope_decode(qc[b].data_ptr(), kk[b].data_ptr(), vv[b].data_ptr(), kc1[b].data_ptr(), vc1[b].data_ptr(),
                                                  o1.data_ptr(), pos_t[b:b + 1].data_ptr(), inv_freq.data_ptr(), nq, nkv, hd, L,
                                                  1.0 / math.sqrt(hd), ws1.data_ptr() if wsb else None, wsb, stream), "qpal_attn_rope_decode")
        torch.cuda.synchronize()
        assert torch.allclose(out[b].float(), o1.float(), atol=2e-3, rtol=2e-3), (b, pos[b], float((out[b].float() - o1.float()).abs().max()))
    assert torch.equal(vc, vc1)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [256, 4096])
def test_inactive_and_independent_sequences(dev, L):
    nq, nkv, hd, B = 32, 8, 128, 6
    pos = [5, -1, L, L - 1, 1 << 40, 300]
    q, k, v, kc, vc, pos_t = _setup(dev, B, nq, nkv, hd, L, [p if 0 <= p < L else -1 for p in pos], seed=L)
    pos_t = torch.tensor(pos, dtype=torch.long, device=dev)
    inv_freq = _inv_freq(hd, dev)
    ws = qp.attention_workspace(B, nq, nkv, hd, L, dev)
    kc0, vc0 = kc.clone(), vc.clone()
    out = torch.full((B, nq * hd), 3.0, dtype=torch.float16, device=dev)
    qp.decode_attention(q, k, v, kc, vc, pos_t, inv_freq, out=out, ws=ws)
    torch.cuda.synchronize()
    for b in (1, 2, 4):  # inactive: output row and cache untouched
        assert bool((out[b] == 3.0).all())
        assert torch.equal(kc[b].view(torch.int16), kc0[b].view(torch.int16)) and torch.equal(vc[b].view(torch.int16), vc0[b].view(torch.int16))
    for b in (0, 3, 5):
        assert bool(torch.isfinite(out[b]).all())
    # changing sequence j's inputs (new q / k / v and its cached rows) leaves every other row bitwise as it was
    j = 3
    kcj, vcj = kc0.clone(), vc0.clone()
    kcj[j] = (torch.randn_like(kcj[j].float()) * 0.5).half()
    vcj[j] = (torch.randn_like(vcj[j].float()) * 0.5).half()
    qkv2 = torch.cat([q, k, v], dim=1)  # (q, k, v share one row stride)
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
    assert torch.equal(kc[others].view(torch.int16), kcj[others].view(torch.int16))
    if ws is not None:
        assert int(ws[: 128 * nkv].abs().max()) == 0


@pytest.mark.gpu
def test_graph_replay_with_positions_advanced_on_the_device(dev):
    """a captured launch replayed with pos advanced on the device equals eager launches; two replays are bitwise equal"""
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
        o = torch.zeros(B, nq * hd, dtype=torch.float16, device=dev)  # (row 5, inactive, keeps its zeros)
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
        g.replay()  # the last position again: same cache row rewritten with the same values, same output
        again = out.clone()
        torch.cuda.synchronize()
    for a, b in zip(eager, got):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert torch.equal(again.view(torch.int16), got[-1].view(torch.int16))
    assert torch.equal(kc.view(torch.int16), kc_e.view(torch.int16)) and torch.equal(vc.view(torch.int16), vc_e.view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["3_8b", "3_70b"])
def test_batched_decode_step_matches_torch_glue_step(dev, model):
    sys.path.insert(0, os.path.join(ROOT, "perf"))
    import decode_llama_batch
    res = decode_llama_batch.main(["--model", model, "--layers", "2", "--batch", "4", "--inactive", "1", "--context", "128",
                                   "--tokens", "4", "--vocab", "4096"], quiet=True)
    (r,) = res["batches"]
    chk = r["check"]
    assert r["active"] == 3 and r["ms_step"] > 0 and r["ms_linears_only"] > 0 and r["ms_torch_glue"] > 0
    assert chk is not None and chk["finite"]
    assert chk["max_abs_diff_final_norm"] <= 2.0 ** -7 * max(1.0, chk["max_abs_ref"]), chk
