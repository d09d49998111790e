"""Prompt prefill: the causal chunk attention kernel (csrc/attn_prefill.hip, qpalette_amd.prefill_attention) and the whole-model
decoder.Prefill (driver perf/prefill_llama.py).

CPU: the C-ABI is exported, the workspace size is monotone, argument errors are return codes, the wrapper checks first.
GPU: parity with a torch fp32 restatement and qpal_rope_kv's cache bytes over sampled (shape, T, pos0, max_len); T = 1 against
decode_attention; causality, chunk invariance, out-of-range positions, determinism and graph replay; the whole model against the
torch-glue step at q_len = N and a batched DecodeStep continuing the prefilled slot.  Tolerances are test_attn_batch.py's."""
import math
import os
import sys

import pytest
import torch

import qpalette_amd as qp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_SHAPE, E_NULL, E_ALIGN = -1, -3, -4
SHAPES = [(32, 8, 128), (64, 8, 128), (8, 8, 64), (16, 2, 64), (16, 4, 256), (8, 1, 128)]  # nq, nkv, hd


# ---------------------------------------------------------------------------------------------------------------- CPU

@pytest.fixture(scope="module")
def lib():
    return qp._native.lib()


def test_prefill_symbols_are_exported(lib):
    for name in ("qpal_attn_rope_prefill", "qpal_attn_prefill_ws_bytes"):
        assert name in qp._native.exported_symbols()
        assert hasattr(lib, name)
    assert callable(qp.prefill_attention) and callable(qp.prefill_workspace) and callable(qp.Prefill)
    with open(os.path.join(ROOT, "include", "qpal.h")) as f:
        hdr = f.read()
    assert "qpal_attn_rope_prefill(" in hdr and "qpal_attn_prefill_ws_bytes(" in hdr


def test_prefill_workspace_size_is_monotone(lib):
    ws = lib.qpal_attn_prefill_ws_bytes
    for nq, nkv, hd in SHAPES:
        for L in (4, 128, 508):  # short caches: one chunk per (kv head, query tile), no workspace
            assert all(ws(T, nq, nkv, hd, L) == 0 for T in (1, 16, 128))
        for L in (512, 1024, 2048, 4096, 32768, 65536):
            sizes = [ws(T, nq, nkv, hd, L) for T in range(1, 129)]
            assert all(s > 0 and s % 4 == 0 for s in sizes)
            assert all(a <= b for a, b in zip(sizes, sizes[1:])), (nq, nkv, hd, L)  # monotone in T
        for T in (1, 7, 64, 128):
            sizes = [ws(T, nq, nkv, hd, L) for L in range(4, 65536 + 4, 508)]
            assert all(a <= b for a, b in zip(sizes, sizes[1:])), (nq, nkv, hd, T)  # monotone in max_len
    # no workspace for shapes the launch rejects
    assert ws(0, 32, 8, 128, 4096) == 0 and ws(129, 32, 8, 128, 4096) == 0 and ws(4, 24, 8, 128, 4096) == 0
    assert ws(4, 32, 8, 96, 4096) == 0 and ws(4, 32, 8, 128, 4098) == 0 and ws(4, 64, 8, 256, 4096) == 0


def _call(lib, q=16, k=16, v=16, ld=4096, kc=4096, vc=4096, out=16, ld_out=4096, pos=16, inv=16, B=4, nq=32, nkv=8, hd=128,
          L=1024, ws=16, ws_bytes=1 << 30):
    return lib.qpal_attn_rope_prefill(q, k, v, ld, kc, vc, out, ld_out, pos, inv, B, nq, nkv, hd, L, 0.1, ws, ws_bytes, None)


def test_prefill_argument_errors_without_a_gpu(lib):
    """Every argument error is returned before any stream work (the pointers below are never dereferenced): the batch kernel's
    list of perturbations, B standing for T."""
    for kw in ({"q": None}, {"k": None}, {"v": None}, {"kc": None}, {"vc": None}, {"out": None}, {"pos": None}, {"inv": None}):
        assert _call(lib, **kw) == E_NULL, kw
    assert _call(lib, ws=None) == E_NULL  # 1024 positions: the split form needs its workspace
    for kw in ({"hd": 96}, {"hd": 32}, {"nq": 24}, {"nq": 48}, {"nq": 128}, {"B": 0}, {"B": 129}, {"L": 1022}, {"L": 0},
               {"hd": 256, "nq": 64}, {"ld": 4095}, {"ld_out": 100}, {"ws_bytes": 4}):
        assert _call(lib, **kw) == E_SHAPE, kw
    for kw in ({"kc": 4096 + 8}, {"vc": 4096 + 2}, {"q": 18}, {"pos": 17}, {"out": 17}, {"ws": 18}):
        assert _call(lib, **kw) == E_ALIGN, kw


def test_prefill_wrapper_checks_before_the_library():
    z = torch.zeros
    good = dict(q=z(2, 8), k=z(2, 8), v=z(2, 8), kcache=z(1, 8, 8).half(), vcache=z(1, 8, 8).half(),
                pos0=z(1, dtype=torch.long), inv_freq=z(4))
    for bad in ({"q": z(2, 8).half()}, {"kcache": z(1, 8, 8)}, {"kcache": z(2, 1, 8, 8).half()}, {"q": z(2, 9)}, {"k": z(3, 8)},
                {"pos0": z(1, dtype=torch.int32)}, {"inv_freq": z(5)}, {"q": z(129, 8)}, {}):  # ({}: host tensors)
        with pytest.raises(qp._native.QpalError):
            qp.prefill_attention(**{**good, **bad})


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


def _setup(dev, T, nq, nkv, hd, L, pos0, seed):
    """test_attn_batch.py's _setup for T rows of one sequence: a padded row stride, NaN in the cache rows about to be written,
    random existing context"""
    gen = torch.Generator(device=dev).manual_seed(seed)
    W = nq * hd + 2 * nkv * hd
    qkv = torch.randn(T, W + 8, device=dev, generator=gen)
    q, k, v = qkv[:, :nq * hd], qkv[:, nq * hd:nq * hd + nkv * hd], qkv[:, nq * hd + nkv * hd:W]
    kc = (torch.randn(nkv, L, hd, device=dev, generator=gen) * 0.5).half()
    vc = (torch.randn(nkv, L, hd, device=dev, generator=gen) * 0.5).half()
    if 0 <= pos0 and pos0 + T <= L:
        kc[:, pos0:pos0 + T] = float("nan")
        vc[:, pos0:pos0 + T] = float("nan")
    return q, k, v, kc, vc, torch.tensor([pos0], dtype=torch.long, device=dev)


def _rope_kv_per_position(q, k, v, kc, vc, pos0, inv_freq, nq, nkv, hd):
    """qpal_rope_kv on every row alone: (expected caches, fp16 q after the rotary embedding)"""
    nat = qp._native
    T, L = q.shape[0], kc.shape[1]
    kc_ref, vc_ref = kc.clone(), vc.clone()
    q16 = torch.zeros(T, nq * hd, dtype=torch.float16, device=kc.device)
    qc, kk, vv = q.contiguous(), k.contiguous(), v.contiguous()
    pos = torch.arange(pos0, pos0 + T, dtype=torch.long, device=kc.device)
    stream = torch.cuda.current_stream(kc.device).cuda_stream
    for t in range(T):
        nat.check(nat.lib().qpal_rope_kv(qc[t].data_ptr(), kk[t].data_ptr(), vv[t].data_ptr(), q16[t].data_ptr(), kc_ref.data_ptr(),
                                         vc_ref.data_ptr(), pos[t:t + 1].data_ptr(), inv_freq.data_ptr(), nq, nkv, hd, L, stream),
                  "qpal_rope_kv")
    return kc_ref, vc_ref, q16


def _attention_reference(q16, kc_ref, vc_ref, pos0, nq, nkv, hd):
    """row t: softmax(q k^T / sqrt(hd)) v over 0 .. pos0 + t of the fp16 cache (causal, GQA by repeat_interleave), fp32"""
    T, n = q16.shape[0], pos0 + q16.shape[0]
    qf = q16.view(T, nq, hd).float().transpose(0, 1)                                   # [nq, T, hd]
    kf = kc_ref[:, :n].float().repeat_interleave(nq // nkv, dim=0)                     # [nq, n, hd]
    vf = vc_ref[:, :n].float().repeat_interleave(nq // nkv, dim=0)
    s = qf @ kf.transpose(-1, -2) / math.sqrt(hd)
    keep = torch.arange(n, device=s.device)[None, :] <= (pos0 + torch.arange(T, device=s.device))[:, None]
    s = s.masked_fill(~keep[None], float("-inf"))
    return (torch.softmax(s, dim=-1) @ vf).transpose(0, 1).reshape(T, nq * hd)


def _torch_rope_q(q, pos0, inv_freq, nq, hd):
    pos = torch.arange(pos0, pos0 + q.shape[0], device=q.device)
    ang = pos.float()[:, None] * inv_freq[None, :]
    emb = torch.cat((ang, ang), dim=-1)[:, None]
    qh = q.half().view(-1, nq, hd)
    return (qh * emb.cos().half() + _rotate_half(qh) * emb.sin().half()).view(-1, nq * hd)


TS = [1, 2, 15, 16, 17, 64, 127, 128]
POS0 = [0, 1, 63, 500, "end"]  # "end": max_len - T
LS = [128, 2048, 32768]
# a sample of the cross product: 48 cases in which every shape meets every max_len and every T, pos0 and shape occurs
PARITY = [(SHAPES[i % 6], TS[i % 8], POS0[i % 5], LS[(i // 6) % 3]) for i in range(48)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,T,pos0,L", PARITY)
def test_prefill_attention_matches_torch_and_appends_like_rope_kv(dev, shape, T, pos0, L):
    nq, nkv, hd = shape
    if T > L:
        pytest.skip("T > max_len")
    pos0 = L - T if pos0 == "end" else pos0
    q, k, v, kc, vc, pos_t = _setup(dev, T, nq, nkv, hd, L, pos0, seed=T + nq + L + pos0)
    inv_freq = _inv_freq(hd, dev)
    ws = qp.prefill_workspace(T, nq, nkv, hd, L, dev)
    kc0, vc0 = kc.clone(), vc.clone()
    out = torch.full((T, nq * hd), 3.0, dtype=torch.float16, device=dev)
    qp.prefill_attention(q, k, v, kc, vc, pos_t, inv_freq, out=out, ws=ws)
    torch.cuda.synchronize()
    if pos0 + T > L:  # the sampled rows do not fit this cache: the launch must do nothing
        assert bool((out == 3.0).all())
        assert torch.equal(kc.view(torch.int16), kc0.view(torch.int16)) and torch.equal(vc.view(torch.int16), vc0.view(torch.int16))
        return
    kc_ref, vc_ref, q16 = _rope_kv_per_position(q, k, v, kc0, vc0, pos0, inv_freq, nq, nkv, hd)
    # the cache append: rows pos0 .. pos0 + T - 1 bit for bit what qpal_rope_kv writes, every other byte unchanged
    assert torch.equal(kc.view(torch.int16), kc_ref.view(torch.int16)) and torch.equal(vc.view(torch.int16), vc_ref.view(torch.int16))
    ref = _attention_reference(q16, kc_ref, vc_ref, pos0, nq, nkv, hd)
    err = float((out.float() - ref).abs().max())
    print(f"prefill parity {shape} T={T} pos0={pos0} L={L}: max |diff| = {err:.3e}")
    assert torch.allclose(out.float(), ref, atol=2e-3, rtol=2e-3), err
    # the same against q rotated by torch (cos / sin in torch's fp32 instead of the device's: <= 1 fp16 ulp apart)
    ref_t = _attention_reference(_torch_rope_q(q, pos0, inv_freq, nq, hd), kc_ref, vc_ref, pos0, nq, nkv, hd)
    assert torch.allclose(out.float(), ref_t, atol=4e-3, rtol=4e-3)
    if ws is not None:
        assert int(ws[: 8 * nkv].abs().max()) == 0, "tickets must be back at zero after a launch"
    # a second launch on the restored state: bitwise the same (fixed merge order, no float atomics)
    kc[:, pos0:pos0 + T] = float("nan")
    vc[:, pos0:pos0 + T] = float("nan")
    out2 = qp.prefill_attention(q, k, v, kc, vc, pos_t, inv_freq, ws=ws)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), out2.view(torch.int16))
    assert torch.equal(kc.view(torch.int16), kc_ref.view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("nq,nkv,hd,L,pos0", [(32, 8, 128, 4096, 1000), (64, 8, 128, 1024, 0), (8, 8, 64, 256, 255), (16, 4, 256, 2048, 77)])
def test_one_row_equals_decode_attention(dev, nq, nkv, hd, L, pos0):
    q, k, v, kc, vc, pos_t = _setup(dev, 1, nq, nkv, hd, L, pos0, seed=L + pos0)
    inv_freq = _inv_freq(hd, dev)
    kc1, vc1 = kc.clone()[None], vc.clone()[None]
    out = qp.prefill_attention(q, k, v, kc, vc, pos_t, inv_freq, ws=qp.prefill_workspace(1, nq, nkv, hd, L, dev))
    out1 = qp.decode_attention(q, k, v, kc1, vc1, pos_t, inv_freq, ws=qp.attention_workspace(1, nq, nkv, hd, L, dev))
    torch.cuda.synchronize()
    assert torch.allclose(out.float(), out1.float(), atol=2e-3, rtol=2e-3), float((out.float() - out1.float()).abs().max())
    assert torch.equal(kc.view(torch.int16), kc1[0].view(torch.int16)) and torch.equal(vc.view(torch.int16), vc1[0].view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("nq,nkv,hd,L,T,pos0,t0", [(32, 8, 128, 2048, 128, 300, 70), (16, 2, 64, 128, 40, 5, 17), (8, 1, 128, 4096, 100, 2000, 99),
                                                    (16, 4, 256, 1024, 64, 0, 1)])
def test_causality_is_bitwise(dev, nq, nkv, hd, L, T, pos0, t0):
    """perturbing row t0's q / k / v leaves out[:t0] and the cache rows below pos0 + t0 bitwise unchanged, and changes out[t0]"""
    q, k, v, kc, vc, pos_t = _setup(dev, T, nq, nkv, hd, L, pos0, seed=T + t0)
    inv_freq = _inv_freq(hd, dev)
    ws = qp.prefill_workspace(T, nq, nkv, hd, L, dev)
    kc2, vc2 = kc.clone(), vc.clone()
    out = qp.prefill_attention(q, k, v, kc, vc, pos_t, inv_freq, ws=ws)
    qkv2 = torch.cat([q, k, v], dim=1)
    q2, k2, v2 = qkv2.split([nq * hd, nkv * hd, nkv * hd], dim=1)
    q2[t0] += 1.0
    k2[t0] -= 1.0
    v2[t0] *= 2.0
    out2 = qp.prefill_attention(q2, k2, v2, kc2, vc2, pos_t, inv_freq, ws=ws)
    torch.cuda.synchronize()
    assert torch.equal(out[:t0].view(torch.int16), out2[:t0].view(torch.int16))
    assert not torch.equal(out[t0], out2[t0])
    n = pos0 + t0
    assert torch.equal(kc[:, :n].view(torch.int16), kc2[:, :n].view(torch.int16)) and torch.equal(vc[:, :n].view(torch.int16), vc2[:, :n].view(torch.int16))
    assert not torch.equal(kc[:, n].view(torch.int16), kc2[:, n].view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("nq,nkv,hd,L,pos0", [(32, 8, 128, 2048, 100), (16, 2, 64, 256, 0), (16, 4, 256, 4096, 3000)])
def test_chunk_invariance(dev, nq, nkv, hd, L, pos0):
    """the same 200 rows as 128 + 72 and as 64 + 64 + 72: bitwise equal caches, outputs within the kernel's tolerance"""
    N = 200
    gen = torch.Generator(device=dev).manual_seed(L)
    qkv = torch.randn(N, nq * hd + 2 * nkv * hd, device=dev, generator=gen)
    q, k, v = qkv.split([nq * hd, nkv * hd, nkv * hd], dim=1)
    kc = (torch.randn(nkv, L, hd, device=dev, generator=gen) * 0.5).half()
    vc = (torch.randn(nkv, L, hd, device=dev, generator=gen) * 0.5).half()
    inv_freq = _inv_freq(hd, dev)
    ws = qp.prefill_workspace(128, nq, nkv, hd, L, dev)
    res = []
    for cuts in ((128, 72), (64, 64, 72)):
        kcc, vcc, outs, at = kc.clone(), vc.clone(), [], 0
        for n in cuts:
            p = torch.tensor([pos0 + at], dtype=torch.long, device=dev)
            outs.append(qp.prefill_attention(q[at:at + n], k[at:at + n], v[at:at + n], kcc, vcc, p, inv_freq, ws=ws))
            at += n
        res.append((kcc, vcc, torch.cat(outs)))
    torch.cuda.synchronize()
    (ka, va, oa), (kb, vb, ob) = res
    assert torch.equal(ka.view(torch.int16), kb.view(torch.int16)) and torch.equal(va.view(torch.int16), vb.view(torch.int16))
    assert torch.allclose(oa.float(), ob.float(), atol=2e-3, rtol=2e-3), float((oa.float() - ob.float()).abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("L,T", [(256, 16), (4096, 128), (2048, 1)])
def test_out_of_range_positions_do_nothing(dev, L, T):
    nq, nkv, hd = 32, 8, 128
    inv_freq = _inv_freq(hd, dev)
    ws = qp.prefill_workspace(T, nq, nkv, hd, L, dev)
    for pos0 in (-1, L - T + 1, 1 << 40):
        q, k, v, kc, vc, pos_t = _setup(dev, T, nq, nkv, hd, L, pos0, seed=L)
        kc0, vc0 = kc.clone(), vc.clone()
        out = torch.full((T, nq * hd), 3.0, dtype=torch.float16, device=dev)
        qp.prefill_attention(q, k, v, kc, vc, pos_t, inv_freq, out=out, ws=ws)
        torch.cuda.synchronize()
        assert bool((out == 3.0).all()), pos0
        assert torch.equal(kc.view(torch.int16), kc0.view(torch.int16)) and torch.equal(vc.view(torch.int16), vc0.view(torch.int16)), pos0
    if ws is not None:
        assert int(ws.abs().max()) == 0


@pytest.mark.gpu
def test_graph_replay_with_the_position_advanced_on_the_device(dev):
    """a captured launch replayed with pos0 advanced by T on the device equals the eager sequence bitwise; the workspace's tickets
    are back at zero afterwards"""
    nq, nkv, hd, L, T = 32, 8, 128, 4096, 128
    q, k, v, kc, vc, pos_t = _setup(dev, T, nq, nkv, hd, L, 1000, seed=5)
    inv_freq = _inv_freq(hd, dev)
    ws = qp.prefill_workspace(T, nq, nkv, hd, L, dev)
    kc_e, vc_e, pos_e = kc.clone(), vc.clone(), pos_t.clone()
    eager = []
    for _ in range(3):
        eager.append(qp.prefill_attention(q, k, v, kc_e, vc_e, pos_e, inv_freq, ws=ws))
        pos_e += T
    torch.cuda.synchronize()
    out = torch.zeros(T, nq * hd, dtype=torch.float16, device=dev)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        kc_w, vc_w = kc.clone(), vc.clone()
        qp.prefill_attention(q, k, v, kc_w, vc_w, pos_t, inv_freq, out=out, ws=ws)  # warm-up on scratch caches
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            qp.prefill_attention(q, k, v, kc, vc, pos_t, inv_freq, out=out, ws=ws)
        got = []
        for _ in range(3):
            g.replay()
            got.append(out.clone())
            pos_t += T
        torch.cuda.synchronize()
    for a, b in zip(eager, got):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert torch.equal(kc.view(torch.int16), kc_e.view(torch.int16)) and torch.equal(vc.view(torch.int16), vc_e.view(torch.int16))
    assert int(ws[: 8 * nkv].abs().max()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["3_8b", "3_70b"])
def test_prefill_matches_torch_glue_and_a_decode_step_continues_it(dev, model):
    """Prefill's last-row final-norm state against the torch-glue q_len = N state: max |diff| <= 2^-7 max(1, max |ref|), the bound of
    test_batched_decode_step_matches_torch_glue_step.  Should the two EXISTING paths (token-by-token DecodeStep(generic=True) vs
    torch glue) alone be further apart than that on these inputs, twice their distance is the bound."""
    sys.path.insert(0, os.path.join(ROOT, "perf"))
    import prefill_llama
    res = prefill_llama.main(["--model", model, "--layers", "2", "--vocab", "4096", "--context", "512", "--slots", "3", "--slot", "1",
                              "--prompt", "1", "5", "128", "129", "300", "--no-time"], quiet=True)
    assert [r["prompt"] for r in res["prompts"]] == [1, 5, 128, 129, 300]
    for r in res["prompts"]:
        chk = r["check"]
        print(model, r["prompt"], chk)
        bound = chk["bound"]
        if chk["existing_paths_max_abs_diff"] > bound:
            bound = 2.0 * chk["existing_paths_max_abs_diff"]
        assert chk["finite"] and chk["max_abs_diff_final_norm"] <= bound, chk
        assert chk["other_slots_untouched"], chk
        cont = chk["continuation"]
        assert cont["finite"] and cont["max_abs_diff_final_norm"] <= max(cont["bound"], bound), chk


@pytest.mark.gpu
def test_prefill_rejects_a_prompt_that_does_not_fit(dev):
    sys.path.insert(0, os.path.join(ROOT, "perf"))
    from decode_llama import build_model
    m = build_model("3_8b", "tcomb_6_7_0.5_none_0.9", None, 1, 512, dev)
    kc = [torch.zeros(1, 8, 64, 128, dtype=torch.float16, device=dev)]
    vc = [torch.zeros(1, 8, 64, 128, dtype=torch.float16, device=dev)]
    pf = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, chunk=32)
    toks = torch.zeros(40, dtype=torch.long, device=dev)
    with pytest.raises(qp._native.QpalError):
        pf(toks, slot=0, pos0=25)
    with pytest.raises(qp._native.QpalError):
        pf(toks, slot=1, pos0=0)
    assert pf(toks, slot=0, pos0=24).shape == (1,)
