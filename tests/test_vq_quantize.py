"""Fixed-codebook VQ / SQ quantiser (qpalette_amd.quantize, csrc/vq_encode.hip): the nearest-codeword LDLQ encoder against the
reference's own outputs (tests/golden/vq_ldlq.npz, written by tests/golden/make_golden_vq.py).

Bars: codes BIT-EXACT for every codec with H = I and with an SPD H (the fixture keeps every decision a margin away from a tie,
so rounding differences of the fp64 feedback cannot flip one); exact ties go to the lowest index; the module's weight is
lut.half()[Qidxs] exactly."""
import os
import re

import numpy as np
import pytest
import torch

import qpalette_amd as qp
from qpalette_amd import quantize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODECS = [(1, b) for b in (2, 4, 6, 8)] + [(2, b) for b in (2, 5, 6, 8, 10, 12)] + [(4, b) for b in (6, 8)]


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "vq_ldlq.npz"))


def spd_hessian(A):
    """H = A^T A / 512 + 1e-2 I in fp64 from the fixture's ternary A (as make_golden_vq.py builds it)."""
    Ai = A.astype(np.int64)
    return (Ai.T @ Ai).astype(np.float64) / A.shape[0] + 1e-2 * np.eye(A.shape[1])


def brute(X, C):
    """Direct-form fp64 nearest codeword, summed over v in order; lowest index on ties (numpy argmin)."""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    out = np.empty(len(X), dtype=np.int64)
    for r0 in range(0, len(X), 4096):
        x = X[r0:r0 + 4096]
        d = (x[:, None, 0] - C[None, :, 0]) ** 2
        for v in range(1, X.shape[1]):
            d = d + (x[:, None, v] - C[None, :, v]) ** 2
        out[r0:r0 + 4096] = d.argmin(axis=1)
    return out


def proxy_err(W, hatW, H):
    dW = W - hatW
    return np.trace(dW @ H @ dW.T) / np.trace(W @ H @ W.T)


# ---------------------------------------------------------------------------------------------------------- CPU


@pytest.mark.parametrize("vec,bits", CODECS)
def test_fixture_is_self_consistent(g, vec, bits):
    lut, W = g[f"lut_v{vec}_b{bits}"], g["W"]
    assert lut.dtype == np.float32 and lut.shape == (1 << bits, vec)
    for name in ("eye", "spd"):
        q = g[f"v{vec}_b{bits}_{name}_Qidxs"]
        assert q.shape == (64, 256 // vec) and int(q.max()) < 1 << bits
    # without feedback every group takes its nearest codeword on its own
    ref = brute(W.reshape(-1, vec), lut).reshape(64, 256 // vec)
    assert np.array_equal(g[f"v{vec}_b{bits}_eye_Qidxs"], ref)
    assert not np.array_equal(g[f"v{vec}_b{bits}_spd_Qidxs"], ref)


@pytest.mark.parametrize("vec", [1, 2, 4])
def test_fixture_ties_go_to_the_lowest_index(g, vec):
    lut, x, q = g[f"tie_v{vec}_lut"], g[f"tie_v{vec}_x"], g[f"tie_v{vec}_Qidxs"].astype(np.int64)
    assert np.array_equal(q, brute(x, lut))
    d = ((x[:, None, :] - lut[None].astype(np.float64)) ** 2).sum(-1)
    assert ((d == d.min(axis=1, keepdims=True)).sum(axis=1) >= 2).all()   # every row ties
    assert len(np.unique(lut, axis=0)) < len(lut)                           # duplicated codewords


def test_vq_symbols_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qpal.h")).read(), flags=re.S)
    lib = qp._native.lib()
    assert re.search(r"\bqpal_vq_encode\s*\(", text) and "qpal_vq_encode" in qp._native.exported_symbols()
    assert hasattr(lib, "qpal_vq_encode")


def test_vq_encode_argument_errors():
    lib = qp._native.lib()
    buf = np.zeros(1 << 12, dtype=np.float64)
    p = buf.ctypes.data
    ok = dict(idx=p, hat=p, w=p, prod=None, lt=None, ld=16, ld_l=0, lut=p, m=4, cols=16, bits=6, vec=2)

    def call(**kw):
        a = {**ok, **kw}
        return lib.qpal_vq_encode(a["idx"], a["hat"], a["w"], a["prod"], a["lt"], a["ld"], a["ld_l"], a["lut"], a["m"], a["cols"],
                                  a["bits"], a["vec"], None)

    # argument errors return before anything touches a device
    for name in ("idx", "w", "lut"):
        assert call(**{name: None}) == -3
    assert call(prod=p) == -3                      # prod without L
    for vec in (0, 3, 8):
        assert call(vec=vec) == -2
    for bits in (0, 13):
        assert call(bits=bits) == -2
    assert call(m=0) == -1
    assert call(cols=15, ld=15) == -1              # cols % vec
    assert call(ld=8) == -1                        # ld < cols
    assert call(ld=17) == -1                       # ld % vec
    assert call(lt=p, ld_l=16, cols=130, ld=130) == -1   # block wider than 128 columns
    assert call(lt=p, ld_l=8) == -1                # ld_l < cols
    assert call(idx=p + 2) == -4
    assert call(w=p + 4) == -4
    assert call(hat=p + 4) == -4
    assert call(lt=p + 4, ld_l=16) == -4
    assert call(prod=p + 4, lt=p, ld_l=16) == -4
    assert call(lut=p + 2) == -4


def test_python_api_rejects_bad_input():
    lut = torch.randn(64, 2)
    with pytest.raises(qp._native.QpalError):
        quantize.vq_nearest(torch.randn(8, 2), lut)                   # CPU tensor
    with pytest.raises(qp._native.QpalError):
        quantize.quantize_vq_weight(torch.randn(16, 32), lut)         # CPU tensor
    with pytest.raises(qp._native.QpalError):
        quantize.vq_nearest(torch.randn(8, 2), torch.randn(48, 2))    # not 2^bits codewords
    with pytest.raises(qp._native.QpalError):
        quantize.vq_nearest(torch.randn(8, 2), torch.randn(64, 3))    # vec 3
    with pytest.raises(qp._native.QpalError):
        quantize.vq_nearest(torch.randn(8, 2), torch.randn(1 << 13, 1))  # 13 bits
    # (vec, bits) the packers do not hold, checked before any device work
    for vec, bits, simt in ((1, 1, False), (1, 9, False), (2, 1, False), (1, 10, True), (2, 2, True), (4, 5, False),
                            (4, 4, True)):
        with pytest.raises(qp._native.QpalError):
            quantize.make_vq_linear(torch.randn(16, 64), torch.randn(1 << bits, vec), simt=simt)


# ---------------------------------------------------------------------------------------------------------- GPU


def _dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("vec,bits", CODECS)
def test_quantize_vq_weight_matches_reference(g, vec, bits):
    dev = _dev()
    lut = torch.from_numpy(g[f"lut_v{vec}_b{bits}"])
    W = torch.from_numpy(g["W"]).to(dev)
    H = torch.from_numpy(spd_hessian(g["A"])).to(dev)
    for name, h in (("eye", None), ("eye", torch.eye(256, dtype=torch.float64, device=dev)), ("spd", H)):
        _, hatW, info = quantize.quantize_vq_weight(W, lut, H=h)
        q = info["Qidxs"].cpu().numpy()
        assert q.dtype == np.int32
        assert np.array_equal(q, g[f"v{vec}_b{bits}_{name}_Qidxs"].astype(np.int32)), f"{name}, H={'given' if h is not None else None}"
        assert np.array_equal(hatW.cpu().numpy(), g[f"lut_v{vec}_b{bits}"][q].reshape(64, 256))


@pytest.mark.gpu
@pytest.mark.parametrize("vec,bits", [(1, 4), (1, 8), (2, 6), (2, 12), (4, 6), (4, 8)])
def test_vq_nearest_exact(g, vec, bits):
    dev = _dev()
    gen = torch.Generator().manual_seed(vec * 16 + bits)
    lut = torch.randn(1 << bits, vec, generator=gen)
    X = torch.cat([torch.randn(5000, vec, generator=gen) * s for s in (1.0, 3.0, 1e-3)]).double()
    hat, idx = quantize.vq_nearest(X.to(dev), lut.to(dev))
    assert hat.dtype == torch.float64 and idx.dtype == torch.int32
    ref = brute(X.numpy(), lut.numpy())
    assert np.array_equal(idx.cpu().numpy(), ref)
    assert np.array_equal(hat.cpu().numpy(), lut.numpy().astype(np.float64)[ref])
    # duplicated rows: the lowest index
    dup = lut.clone()
    dup[(1 << bits) // 2:] = dup[:(1 << bits) // 2]
    _, idx = quantize.vq_nearest(X.to(dev), dup.to(dev))
    assert np.array_equal(idx.cpu().numpy(), brute(X.numpy(), dup.numpy()))
    assert int(idx.max()) < (1 << bits) // 2


@pytest.mark.gpu
@pytest.mark.parametrize("vec", [1, 2, 4])
def test_vq_nearest_ties(g, vec):
    dev = _dev()
    lut, x, q = g[f"tie_v{vec}_lut"], g[f"tie_v{vec}_x"], g[f"tie_v{vec}_Qidxs"].astype(np.int32)
    _, idx = quantize.vq_nearest(torch.from_numpy(x).to(dev), torch.from_numpy(lut).to(dev))
    assert np.array_equal(idx.cpu().numpy(), q)


@pytest.mark.gpu
@pytest.mark.parametrize("vec,bits", [(1, 6), (2, 10), (4, 8)])
def test_vq_nearest_independent_of_batch_and_position(g, vec, bits):
    dev = _dev()
    gen = torch.Generator().manual_seed(bits)
    lut = torch.randn(1 << bits, vec, generator=gen).to(dev)
    probe = torch.randn(64, vec, generator=gen, dtype=torch.float64)
    _, ref = quantize.vq_nearest(probe.to(dev), lut)
    for B in (1, 64, 1000, 70001):
        X = torch.randn(B, vec, generator=gen, dtype=torch.float64)
        pos = torch.randperm(B, generator=gen)[:min(B, 64)]
        X[pos] = probe[:len(pos)]
        _, idx = quantize.vq_nearest(X.to(dev), lut)
        assert torch.equal(idx[pos.to(dev)], ref[:len(pos)]), f"B={B}"
        assert np.array_equal(idx.cpu().numpy(), brute(X.numpy(), lut.cpu().numpy())), f"B={B}"


@pytest.mark.gpu
@pytest.mark.parametrize("vec,bits,simt", [(1, 4, False), (1, 6, False), (2, 6, False), (2, 12, False), (4, 8, True)])
def test_make_vq_linear_round_trip(vec, bits, simt):
    dev = _dev()
    m, k = 256, 1024
    gen = torch.Generator().manual_seed(vec * 16 + bits)
    lut = torch.randn(1 << bits, vec, generator=gen)
    W = torch.randn(m, k, generator=gen).to(dev)
    layer = quantize.make_vq_linear(W, lut)
    assert isinstance(layer, qp.VQLinearPackSIMT if simt else qp.VQLinearPackTensorCore)
    if vec == 1 and bits <= 4:
        assert layer.vq_type == "sq_dup"
    _, _, info = quantize.quantize_vq_weight(W, lut)
    q = info["Qidxs"].cpu()
    Wq = lut.half()[q.long()].reshape(m, k)
    Wg = layer.get_weight()
    assert torch.equal(Wg.cpu().view(torch.int16), Wq.view(torch.int16)), "dequant of the codes must give lut.half()[Qidxs]"
    Wd = Wq.double().numpy()
    outs = {}
    for bs in (1, 16):
        x = torch.randn(bs, k, generator=torch.Generator().manual_seed(bs)).half()
        y = layer(x.to(dev)).float().cpu().numpy()
        outs[bs] = y
        xd = x.double().numpy()
        ref = xd @ Wd.T
        scale = np.abs(xd) @ np.abs(Wd).T
        tol = 1e-5 * scale + 2.0 ** -10 * np.abs(ref) + 1e-3  # smoke()'s bar: fp32 accumulation, fp16 output
        assert np.all(np.abs(y - ref) <= tol), float(np.abs(y - ref).max())
    # the info round trip rebuilds the same layer
    qstr = f"ldlq_{vec}_{bits}_none_1.0"
    layer2 = qp.make_linear_from_info(qstr, layer._info(), use_simt=simt).to(dev)
    assert torch.equal(layer2.get_weight(), Wg)
    for bs in (1, 16):
        x = torch.randn(bs, k, generator=torch.Generator().manual_seed(bs)).half()
        assert np.array_equal(layer2(x.to(dev)).float().cpu().numpy(), outs[bs])


def torch_ldlq_vq(W, L, lut):
    """Pure-torch fp64 restatement of LDLQ_VQ (ldlq.py:16-58) with a direct-form nearest codeword, on W's device."""
    vec = lut.shape[1]
    m, n = W.shape
    C = lut.to(W.device, torch.float64)
    WT = W.T.contiguous()
    hatT = torch.zeros(n, m, dtype=torch.float64, device=W.device)
    prod = torch.zeros(n, m, dtype=torch.float64, device=W.device)
    buf = 128
    for r1 in range(n, 0, -buf):
        r0 = r1 - buf
        bW, bhat, bL = WT[r0:r1], hatT[r0:r1], L[r0:r1]
        for i in reversed(range(buf // vec)):
            a, b = vec * i, vec * (i + 1)
            x = bW[a:b] + bL[b:, r0 + a:r0 + b].T @ (bW[b:] - bhat[b:]) + prod[r0 + a:r0 + b]
            d = ((x.T[:, None, :] - C[None]) ** 2).sum(-1)
            bhat[a:b] = C[d.argmin(dim=1)].T
        prod += bL.T @ (bW - bhat)
    return hatT.T.contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("vec,bits", [(1, 6), (2, 8)])
def test_ldlq_larger_shape(vec, bits):
    dev = _dev()
    m, k = 512, 1024
    gen = torch.Generator().manual_seed(k + bits)
    lut = torch.randn(1 << bits, vec, generator=gen)
    W = torch.randn(m, k, generator=gen, dtype=torch.float64).to(dev)
    A = torch.randint(-1, 2, (2 * k, k), generator=gen, dtype=torch.float64)
    H = (A.T @ A / (2 * k) + 1e-2 * torch.eye(k, dtype=torch.float64)).to(dev)
    _, _, info = quantize.quantize_vq_weight(W, lut, H=H)
    _, _, info0 = quantize.quantize_vq_weight(W, lut)
    L = quantize.block_ldl(H, vec)
    L.fill_diagonal_(0)
    hat_ref = torch_ldlq_vq(W, L, lut)
    dW = W - hat_ref
    ref = (torch.trace(dW @ H @ dW.T) / torch.trace(W @ H @ W.T)).item()
    assert abs(info["proxy_err"] - ref) <= 1e-6 * ref, (info["proxy_err"], ref)
    dW0 = W - torch.from_numpy(lut.numpy()).to(dev).double()[info0["Qidxs"].long()].reshape(m, k)
    p0 = (torch.trace(dW0 @ H @ dW0.T) / torch.trace(W @ H @ W.T)).item()
    assert info["proxy_err"] < p0
