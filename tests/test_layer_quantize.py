"""Whole-layer quantisation (qpalette_amd.quantize_layer, csrc/hadamard_f32.hip): the fp32 rotation, the incoherence preprocessing,
the comb / combt quantisers and the quantize_linear front end, against the reference's own outputs (tests/golden/combt_ldlq.npz,
written by tests/golden/make_golden_combt.py) and fp64 restatements (oracle/incoherent.py).

Bars: rotate_f32 per-row normwise relative error <= 2e-6 against fp64; preprocessing Wr / Wscale to 1e-5 relative and HRr to 1e-5
of |H|; combt with H = I bit-exact, with an SPD H >= 99 % of the codes and the proxy error within 0.5 % (the TCQ LDLQ criterion);
layer files load back to bit-identical layers."""
import json
import os
import types

import numpy as np
import pytest
import torch

import qpalette_amd as qp
from qpalette_amd import hadamard as had
from qpalette_amd import packers, quantize
from qpalette_amd import quantize_layer as ql
from oracle import incoherent as oi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODECS = [(9, 5, 6), (9, 7, 8), (11, 9, 10)]


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "combt_ldlq.npz"))


def spd_hessian(A):
    """H = A^T A / rows + 1e-2 I in fp64 (as make_golden_combt.py builds it)."""
    Ai = A.astype(np.int64)
    return (Ai.T @ Ai).astype(np.float64) / A.shape[0] + 1e-2 * np.eye(A.shape[1])


def quantlut_sym(tlut16):
    """numpy restatement of the codebook of every trellis state: [65536, 2] fp32 (bitshift.py:71-79)."""
    S = int(tlut16.shape[0]).bit_length() - 1
    s = np.arange(1 << 16, dtype=np.int64)
    h = (s + 1) * s
    lut = tlut16.astype(np.float32)[(h >> (15 - S)) & ((1 << S) - 1)]
    lut[:, 0] *= 1 - ((h >> 15) & 1) * 2
    return lut


def decode_states(Q, tlut16):
    """hatW [m, k] of Qidxs [m, k/2] (state t of tile (tr, tc) at [16 tr + t / 8][8 tc + t % 8], mma element order)."""
    m, k2 = Q.shape
    lut = quantlut_sym(tlut16)
    inv = quantize.INV_PERMUTE.numpy()
    out = np.zeros((m, 2 * k2), dtype=np.float32)
    for tr in range(m // 16):
        for tc in range(k2 // 8):
            st = Q[16 * tr:16 * tr + 16, 8 * tc:8 * tc + 8].reshape(128).astype(np.int64)
            out[16 * tr:16 * tr + 16, 16 * tc:16 * tc + 16] = lut[st].reshape(256)[inv].reshape(16, 16)
    return out


def proxy_err(W, hatW, H):
    dW = W - hatW
    return np.trace(dW @ H @ dW.T) / np.trace(W @ H @ W.T)


def rel_rows(y, ref):
    return np.linalg.norm(y - ref, axis=-1) / np.linalg.norm(ref, axis=-1)


# ---------------------------------------------------------------------------------------------------------- CPU


def test_hadamard_f32_symbol_exported():
    assert "qpal_hadamard_f32" in qp._native.exported_symbols()
    getattr(qp._native.lib(), "qpal_hadamard_f32")


@pytest.mark.parametrize("case,code", [
    (dict(out=0), -3), (dict(inp=0), -3), (dict(K=12, hd=12 * 64, n=12 * 64, hadk=0), -3),
    (dict(K=3, hd=48, n=48), -2), (dict(K=0), -2), (dict(K=260), -2),
    (dict(n=1000), -1), (dict(hd=96, n=96), -1), (dict(hd=8, n=8), -1), (dict(K=12, hd=12 * 8, n=12 * 8), -1),
    (dict(hd=65536, n=65536), -1), (dict(K=172, hd=172 * 256, n=172 * 256), -1), (dict(rows=0), -1),
    (dict(inp=0x1004), -4), (dict(out=0x2008), -4), (dict(su=0x3002), -4), (dict(K=12, hd=12 * 64, n=12 * 64, hadk=0x4001), -4),
])
def test_hadamard_f32_argument_errors(case, code):
    """Every argument error returns before any stream work (fake device pointers: nothing is dereferenced)."""
    a = dict(out=0x2000, inp=0x1000, su=None, hadk=0x4000, rows=2, n=1024, hd=1024, K=1)
    a.update(case)
    rc = qp._native.lib().qpal_hadamard_f32(a["out"] or None, a["inp"] or None, a["su"], a["hadk"] or None, a["rows"], a["n"], a["hd"],
                                            a["K"], 1.0, None)
    assert rc == code


def qdict_strings():
    out = set()
    for name in ("figure1c", "figure1d"):
        with open(os.path.join(ROOT, "perf", "qdicts", f"{name}.json")) as f:
            qd = json.load(f)["qdict"]
        out.update(v[0] for v in qd.values())  # layer key -> [quantizer string, simt flag]
    return sorted(out)


def test_parse_every_published_quantizer_string():
    strs = qdict_strings()
    assert any(s.startswith("tcomb") for s in strs) and any(s.startswith("ldlq") for s in strs)
    for s in strs:
        q = ql.parse_quantizer_str(s)
        assert q["kind"] in ("tcq", "tcomb", "comb", "ldlq")
        assert q["use_hess"] is False and q["scale_override"] == float(s.rsplit("_", 1)[1])
        if q["kind"] == "tcomb":
            assert q["ratio"] == 0.5 and q["KV"][1] == q["KV"][0] + 1
            assert q["tlut_bits"] == (9 if max(q["KV"]) <= 8 else max(q["KV"]) + 1)
    assert ql.parse_quantizer_str("comb_7_8_0.5_none_0.9")["kind"] == "comb"
    assert ql.parse_quantizer_str("tcq_10_hess_0.9")["tlut_bits"] == 11
    assert ql.parse_quantizer_str("ldlq_2_10_hess_0.9") == {"kind": "ldlq", "vec_sz": 2, "lut_bits": 10, "use_hess": True,
                                                            "scale_override": 0.9}
    for bad in ("sq_4_none_0.9", "vq2_8_hess_1.0", "foo_1", "tcq_x_none_0.9", "tcq_6_maybe_0.9"):
        with pytest.raises(qp._native.QpalError):
            ql.parse_quantizer_str(bad)


def test_layer_file_path():
    assert ql.layer_file_path("q", "tcq_6_none_0.9", 3, "mlp.down_proj") == os.path.join("q", "tcq_6_none_0.9", "3_mlp.down_proj.pt")


@pytest.mark.parametrize("with_mu", [False, True])
def test_load_hessian(tmp_path, with_mu):
    rng = np.random.default_rng(5)
    n = 48
    X = rng.standard_normal((200, n))
    Hf = X.T @ X / 200
    r, c = np.tril_indices(n)
    d = {"flatH": torch.from_numpy(Hf[r, c]), "n": n}
    mu = rng.standard_normal(n)
    if with_mu:
        d["mu"] = torch.from_numpy(mu)
    path = tmp_path / "0_qkv.pt"
    torch.save(d, path)
    H = ql.load_hessian(str(path), sigma_reg=0.01).numpy()
    ref = Hf + (np.outer(mu, mu) if with_mu else 0)
    dm = np.diag(ref).mean()
    ref = (ref / dm + 0.01 * np.eye(n)) * dm
    assert H.dtype == np.float64 and H.shape == (n, n)
    np.testing.assert_allclose(H, ref, rtol=1e-13, atol=1e-13)
    assert np.array_equal(H, H.T)


def test_fixture_is_self_consistent(g):
    W = g["W"].astype(np.float64)
    for S, kv1, kv2 in CODECS:
        tlut = g[f"tlut_S{S}"]
        for name in ("eye", "spd"):
            Q, hat = g[f"kv{kv1}_{kv2}_{name}_Qidxs"].astype(np.int32), g[f"kv{kv1}_{kv2}_{name}_hatW"]
            assert Q.shape == (64, 128) and hat.shape == (64, 256)
            assert np.array_equal(decode_states(Q, tlut), hat.astype(np.float32))
            for half, kv in ((Q[:, :64], kv1), (Q[:, 64:], kv2)):
                assert half.max() < 1 << 16
                packers.pack_trellis(torch.from_numpy(np.ascontiguousarray(half)), 64, 128, kv)  # raises unless tail-biting
        # LDLQ with the SPD H does better on its own proxy loss than H = I
        H = spd_hessian(g["A"])
        e_eye = proxy_err(W, g[f"kv{kv1}_{kv2}_eye_hatW"].astype(np.float64), H)
        e_spd = proxy_err(W, g[f"kv{kv1}_{kv2}_spd_hatW"].astype(np.float64), H)
        assert e_spd < e_eye
    for k in (256, 448):
        W = g[f"pre{k}_W"].astype(np.float64)
        su = g[f"pre{k}_SU"].astype(np.float64)
        hadK, K = had.get_hadK(k, transpose=True)
        rot = oi.had_blocks(W * su, k, None if hadK is None else hadK.numpy())
        for path in ("tcq", "vq"):
            Wr, ws = g[f"pre{k}_{path}_Wr"].astype(np.float64), g[f"pre{k}_{path}_Wscale"].astype(np.float64)
            assert rel_rows(Wr * ws[:, None], rot).max() < 1e-5
        assert np.allclose(np.sqrt((g[f"pre{k}_vq_Wr"].astype(np.float64) ** 2).mean(1)), 0.9, rtol=1e-5)  # per-row rms = scale_override


# ---------------------------------------------------------------------------------------------------------- GPU


def cuda(a, dtype=None):
    t = torch.as_tensor(a).cuda()
    return t if dtype is None else t.to(dtype)


ROT_N = [256, 1024, 4096, 5120, 11008, 12288, 14336, 28672]


@pytest.mark.gpu
@pytest.mark.parametrize("n", ROT_N)
@pytest.mark.parametrize("mode", ["plain", "su", "inplace", "post_scale", "blocks"])
def test_rotate_f32_against_fp64(n, mode):
    rng = np.random.default_rng(n)
    rows = 8 if n <= 4096 else 3
    x = rng.standard_normal((rows, n)).astype(np.float32)
    x[0] *= 1e3
    hd = n
    if mode == "blocks":
        hd = {256: 64, 1024: 128, 4096: 128, 5120: 1280, 11008: 5504, 12288: 3072, 14336: 3584, 28672: 7168}[n]
    hadK, K = had.get_hadK(hd, transpose=(n % 2 == 0))
    su = rng.standard_normal(n).astype(np.float32) if mode in ("su", "inplace") else None
    ps = 0.3 if mode == "post_scale" else 1.0
    xt = cuda(x)
    out = xt if mode == "inplace" else None
    y = had.rotate_f32(xt, hd=hd, hadK=hadK, K=K, su=None if su is None else cuda(su), post_scale=ps, out=out)
    torch.cuda.synchronize()
    if mode == "inplace":
        assert y.data_ptr() == xt.data_ptr()
    y = y.cpu().numpy().astype(np.float64)
    xin = x.astype(np.float64) * (su.astype(np.float64) if su is not None else 1.0)
    ref = oi.had_blocks(xin, hd, None if hadK is None else hadK.numpy()) * ps
    assert np.isfinite(y).all()
    assert rel_rows(y, ref).max() <= 2e-6


@pytest.mark.gpu
def test_matmul_hadUt_head_f32_is_the_inverse_rotation():
    x = torch.randn(4, 14336, generator=torch.Generator().manual_seed(1)).cuda()
    y = had.matmul_hadU_head_f32(had.matmul_hadUt_head_f32(x, 14336), 14336)
    assert (y - x).norm() / x.norm() < 2e-6


@pytest.mark.gpu
@pytest.mark.parametrize("k", [256, 448])
def test_preprocess_against_reference(g, k):
    W = cuda(g[f"pre{k}_W"])
    SU = cuda(g[f"pre{k}_SU"], torch.float32)
    A = g["A"] if k == 256 else g[f"pre{k}_A"]
    H = torch.from_numpy(spd_hessian(A))
    lut_rms = ql.tcq_lut_rms(torch.from_numpy(g["tlut_S9"]))
    for path, lr in (("tcq", lut_rms), ("vq", None)):
        Wr, Wscale, HRr, su, sv = ql.incoherent_preprocess(W, H, SU=SU, scale_override=0.9, lut_rms=lr)
        assert Wr.dtype == torch.float32 and Wscale.dtype == torch.float32 and HRr.dtype == torch.float64
        assert torch.equal(su, SU) and torch.equal(sv, torch.ones_like(sv))
        ref_ws = g[f"pre{k}_{path}_Wscale"].astype(np.float64)
        np.testing.assert_allclose(Wscale.cpu().numpy(), ref_ws, rtol=1e-5)
        assert rel_rows(Wr.cpu().numpy().astype(np.float64), g[f"pre{k}_{path}_Wr"].astype(np.float64)).max() < 1e-5
        R = g[f"pre{k}_HRr_rows"].astype(np.float64)
        assert np.abs(HRr[:R.shape[0]].cpu().numpy() - R).max() <= 1e-5 * np.linalg.norm(H.numpy(), 2)


@pytest.mark.gpu
def test_preprocess_two_sided_uses_one_global_scale():
    W = torch.randn(256, 512, generator=torch.Generator().manual_seed(3)).half().cuda()
    Wr, Wscale, _, SU, SV = ql.incoherent_preprocess(W, left_only=False, lut_rms=1.0, scale_override=0.9)
    assert not torch.equal(SV, torch.ones_like(SV))
    assert torch.equal(Wscale, Wscale[:1].expand_as(Wscale))
    # un-rotating both sides gives W back
    back = had.matmul_hadU_head_f32((Wr * Wscale[:, None]).contiguous(), 512) * SU
    back = (had.matmul_hadU_head_f32(back.T.contiguous(), 256) * SV).T
    assert (back - W.float()).norm() / W.float().norm() < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("S,kv1,kv2", CODECS)
def test_combt_against_reference(g, S, kv1, kv2):
    tlut = cuda(g[f"tlut_S{S}"])
    W = cuda(g["W"], torch.float64)
    Hs = torch.from_numpy(spd_hessian(g["A"]))
    for name, H in (("eye", None), ("eye_ldlq", torch.eye(256, dtype=torch.float64)), ("spd", Hs)):
        key = name.split("_")[0]
        t1, t2, hat, info = ql.quantize_combt_weight(W, tlut, (kv1, kv2), (128, 128), H)
        Q = info["Qidxs"].cpu().numpy()
        refQ, refhat = g[f"kv{kv1}_{kv2}_{key}_Qidxs"].astype(np.int32), g[f"kv{kv1}_{kv2}_{key}_hatW"].astype(np.float32)
        if key == "eye":
            assert np.array_equal(Q, refQ), name
            assert np.array_equal(hat.cpu().numpy().view(np.uint32), refhat.view(np.uint32)), name
        else:
            assert (Q == refQ).mean() >= 0.99
            Hn, Wn = Hs.numpy(), g["W"].astype(np.float64)
            e, e_ref = proxy_err(Wn, hat.cpu().numpy().astype(np.float64), Hn), proxy_err(Wn, refhat.astype(np.float64), Hn)
            assert abs(e - e_ref) <= 0.005 * e_ref
            assert info["proxy_err"] == pytest.approx(e, rel=1e-9)
        q = info["Qidxs"].cpu()
        assert torch.equal(t1, packers.pack_trellis(q[:, :64].contiguous(), 64, 128, kv1))
        assert torch.equal(t2, packers.pack_trellis(q[:, 64:].contiguous(), 64, 128, kv2))


@pytest.mark.gpu
def test_combt_quarter_ratio_decodes_to_hatW(g):
    tlut = cuda(g["tlut_S9"])
    W = torch.randn(64, 512, generator=torch.Generator().manual_seed(7)).double().cuda()
    X = torch.randn(1024, 512, generator=torch.Generator().manual_seed(8), dtype=torch.float64)
    H = X.T @ X / 1024 + 1e-2 * torch.eye(512, dtype=torch.float64)
    t1, t2, hat, info = ql.quantize_combt_weight(W, tlut, (5, 6), (128, 384), H)
    assert t1.shape == ((64 // 16) * (128 // 16), 8 * 5) and t2.shape == ((64 // 16) * (384 // 16), 8 * 6)
    layer = ql._comb_module(qp.CombtLinearTCQ, W, tlut, (5, 6), (128, 384), t1, t2, None)
    assert torch.equal(layer.get_weight().float(), hat)
    with pytest.raises(qp._native.QpalError):
        ql.quantize_combt_weight(W, tlut, (5, 6), (64, 448), H)  # in_part[0] not a multiple of buf_cols


@pytest.mark.gpu
def test_comb_is_two_tcq_quantisations(g):
    tlut = cuda(g["tlut_S9"])
    W = torch.randn(96, 256, generator=torch.Generator().manual_seed(9)).double().cuda()
    H = torch.from_numpy(spd_hessian(g["A"]))
    t1, t2, hat, info = ql.quantize_comb_weight(W, tlut, (7, 8), (32, 64), H)
    r1, h1, _ = quantize.quantize_tcq_weight(W[:32], tlut, 7, H)
    r2, h2, _ = quantize.quantize_tcq_weight(W[32:], tlut, 8, H)
    assert torch.equal(t1, r1) and torch.equal(t2, r2)
    assert torch.equal(hat, torch.cat([h1, h2]))
    layer = ql._comb_module(qp.CombLinearTCQ, W, tlut, (7, 8), (32, 64), t1, t2, None)
    assert torch.equal(layer.get_weight().float(), hat)


# ---------------------------------------------------------------------------------------------------------- end to end


def codebooks():
    gz = np.load(os.path.join(ROOT, "tests", "golden", "combt_ldlq.npz"))
    gv = np.load(os.path.join(ROOT, "tests", "golden", "vq_ldlq.npz"))
    # the module keeps the codebook in fp16: hand the quantiser the fp16 values, so its hatW is the module's weight exactly
    return {9: torch.from_numpy(gz["tlut_S9"]), (2, 10): torch.from_numpy(gv["lut_v2_b10"]).half().float()}


def synthetic_hessian(k, seed):
    X = torch.randn(2 * k, k, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).cuda()
    X = X * torch.linspace(0.2, 2.0, k, dtype=torch.float64, device="cuda")
    return X.T @ X / (2 * k) + 1e-2 * torch.eye(k, dtype=torch.float64, device="cuda")


def effective_weight(layer):
    """fp64 [m, k] of what an IncoherentLinear (skip_r) computes: diag(Wscale) W_q (hadK_left (x) H_P)/sqrt(k) diag(SU)."""
    Wq = layer.linear.get_weight().double().cpu().numpy()
    k = Wq.shape[1]
    hadK, K = had.get_hadK(layer.hadU)
    rot = oi.had_blocks(Wq, layer.hadU, None if hadK is None else hadK.numpy())
    return layer.Wscale.double().cpu().numpy()[:, None] * rot * layer.SU.double().cpu().numpy()[None, :k]


def check_err(layer, info, W, lut_rms):
    """quant_info's err equals the error recomputed from the module's weight (in W's scale)."""
    SU = (1.0 / layer.SU.float())
    Wr, Wscale, _, _, _ = ql.incoherent_preprocess(W, SU=SU, scale_override=info["scale_override"], lut_rms=lut_rms)
    ws = Wscale.double()[:, None]
    Ws, hs = Wr.double() * ws, layer.linear.get_weight().double() * ws
    e = ((Ws - hs).pow(2).mean() / Ws.pow(2).mean()).item()
    assert info["err"] == pytest.approx(e, rel=1e-6)


E2E = [(1024, 4096, "tcq_6_hess_0.9"), (1024, 4096, "tcomb_5_6_0.5_hess_0.9"), (1024, 4096, "comb_7_8_0.5_none_0.9"),
       (1024, 4096, "ldlq_2_10_hess_0.9"), (256, 14336, "tcomb_7_8_0.5_hess_0.9")]


@pytest.mark.gpu
@pytest.mark.parametrize("m,k,qstr", E2E)
def test_quantize_linear_end_to_end(tmp_path, m, k, qstr):
    torch.manual_seed(11)
    lin = torch.nn.Linear(k, m, bias=True, dtype=torch.float16).cuda()
    H = synthetic_hessian(k, 12)
    key = "mlp.down_proj" if k == 14336 else "self_attn.o_proj"
    path = ql.layer_file_path(str(tmp_path), qstr, 0, key)
    layer, info = ql.quantize_linear(lin, qstr, H=H, codebooks=codebooks(), save_path=path)
    for kkey in ("quantizer", "use_hess", "err", "orig_err", "scale_override", "time", "rot_info", "quantizer_str"):
        assert kkey in info
    assert ("vec_sz" in info and "lut_bits" in info) if qstr.startswith("ldlq") else "KV" in info
    assert info["quantizer_str"] == qstr and info["rot_info"] == "skip_r" and os.path.exists(path)
    loaded = qp.IncoherentLinear.gen_layer_from_quantizer_str_and_key(None, str(tmp_path), qstr, f"0_{key}",
                                                                      merge_layers=True).cuda()
    # the loaded layer is the returned one: every buffer and the decoded weight bit for bit, and the forward bit for bit at a batch
    # that takes the decode + GEMM route (batch > 256).  (The fused GEMV's split-K float atomics are not bit-reproducible from call
    # to call, so equality of two small-batch forwards would test the GEMV, not the layer file.)
    for name in ("SU", "SV", "Wscale", "bias"):
        assert torch.equal(getattr(loaded, name), getattr(layer, name)), name
    assert (loaded.skip_l, loaded.skip_r) == (layer.skip_l, layer.skip_r) == (False, True)
    assert torch.equal(loaded.linear.get_weight(), layer.linear.get_weight())
    xb = torch.randn(272, k, generator=torch.Generator().manual_seed(14)).half().cuda()
    assert torch.equal(loaded(xb), layer(xb))
    x = torch.randn(4, k, generator=torch.Generator().manual_seed(13)).half().cuda()
    y = layer(x)
    Weff = effective_weight(layer)
    ref = x.double().cpu().numpy() @ Weff.T + lin.bias.detach().double().cpu().numpy()
    assert rel_rows(y.double().cpu().numpy(), ref).max() < 5e-3
    lut_rms = None if qstr.startswith("ldlq") else ql.tcq_lut_rms(codebooks()[9])
    check_err(layer, info, lin.weight, lut_rms)
    # and the layer approximates the original weight
    W = lin.weight.detach().double().cpu().numpy()
    assert ((Weff - W) ** 2).mean() / (W ** 2).mean() < 0.1


@pytest.mark.gpu
def test_incoherent_mlp_round_trip(tmp_path):
    hidden, inter = 1024, 2048
    torch.manual_seed(21)
    up, gate = (torch.nn.Linear(hidden, inter, bias=False, dtype=torch.float16).cuda() for _ in range(2))
    down = torch.nn.Linear(inter, hidden, bias=False, dtype=torch.float16).cuda()
    cbs = codebooks()
    SU = ql.random_signs(hidden, generator=torch.Generator().manual_seed(22), device="cuda")
    Hh, Hi = synthetic_hessian(hidden, 23), synthetic_hessian(inter, 24)
    qs = {"up": "tcomb_5_6_0.5_hess_0.9", "gate": "tcomb_5_6_0.5_hess_0.9", "down": "tcq_6_hess_0.9"}
    layers = {}
    for name, lin, H, su in (("up", up, Hh, SU), ("gate", gate, Hh, SU), ("down", down, Hi, None)):
        layers[name], _ = ql.quantize_linear(lin, qs[name], H=H, SU=su, codebooks=cbs,
                                             save_path=ql.layer_file_path(str(tmp_path), qs[name], 0, f"mlp.{name}_proj"))
    assert torch.equal(layers["up"].SU, layers["gate"].SU)
    cfg = types.SimpleNamespace(hidden_size=hidden, intermediate_size=inter, hidden_act="silu")
    mlp = qp.IncoherentMLP.gen_layer_from_quantizer_str_and_key(cfg, str(tmp_path), qs["up"], qs["gate"], qs["down"], "0_mlp.up_proj",
                                                               "0_mlp.gate_proj", "0_mlp.down_proj").cuda()
    x = torch.randn(2, hidden, generator=torch.Generator().manual_seed(25)).half().cuda()
    y = mlp(x).double().cpu().numpy()
    xd = x.double().cpu().numpy()
    u, gt = xd @ effective_weight(layers["up"]).T, xd @ effective_weight(layers["gate"]).T
    h = gt / (1.0 + np.exp(-gt)) * u
    ref = h @ effective_weight(layers["down"]).T
    assert np.isfinite(y).all()
    assert rel_rows(y, ref).max() < 2e-2


@pytest.mark.gpu
def test_quality_ordering():
    torch.manual_seed(31)
    W = torch.randn(512, 1024, dtype=torch.float16, device="cuda")
    H = synthetic_hessian(1024, 32)
    SU = ql.random_signs(1024, generator=torch.Generator().manual_seed(33), device="cuda")
    cbs = codebooks()
    err = {q: ql.quantize_linear(W, q, H=H, SU=SU, codebooks=cbs)[1]["err"]
           for q in ("tcq_5_hess_0.9", "tcomb_5_6_0.5_hess_0.9", "tcq_6_hess_0.9")}
    assert err["tcq_5_hess_0.9"] > err["tcomb_5_6_0.5_hess_0.9"] > err["tcq_6_hess_0.9"]
    Wn, Hn = W.double().cpu().numpy(), H.cpu().numpy()
    pe = {}
    for q in ("tcq_6_hess_0.9", "tcq_6_none_0.9"):
        layer, _ = ql.quantize_linear(W, q, H=H, SU=SU, codebooks=cbs)
        pe[q] = proxy_err(Wn, effective_weight(layer), Hn)
    assert pe["tcq_6_hess_0.9"] < pe["tcq_6_none_0.9"]


@pytest.mark.gpu
def test_unsupported_strings_and_missing_codebooks():
    W = torch.randn(64, 256, dtype=torch.float16, device="cuda")
    for q in ("sq_4_none_0.9", "vq2_8_none_0.9"):
        with pytest.raises(qp._native.QpalError, match="k-means"):
            ql.quantize_linear(W, q, codebooks=codebooks())
    with pytest.raises(qp._native.QpalError, match="codebook"):
        ql.quantize_linear(W, "tcq_9_none_0.9", codebooks=codebooks())
