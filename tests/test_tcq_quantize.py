"""TCQ quantiser (qpalette_amd.quantize, csrc/tcq_viterbi.hip): the tail-biting Viterbi encoder and LDLQ against the
reference's own outputs (tests/golden/viterbi.npz, written by tests/golden/make_golden_viterbi.py).

Bars: Viterbi states and reconstruction BIT-EXACT for every (S, KV) and sequence kind; LDLQ with identity H bit-exact;
LDLQ with an SPD H: >= 99 % of the states (the fp64 feedback matmuls may round differently on the GPU), proxy error
within 0.5 % of the reference's."""
import os
import re

import numpy as np
import pytest
import torch

import qpalette_amd as qp
from qpalette_amd import quantize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = [(9, kv) for kv in range(2, 11)] + [(10, 8), (10, 9), (10, 10), (11, 9), (11, 10)]


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "viterbi.npz"))


def codec(g, S, KV):
    """(tlut fp16, x fp32 [32, 256], reference hat fp32 [32, 256], reference states int32 [32, 128]) of one codec."""
    x = np.concatenate([g["x"], g[f"S{S}_KV{KV}_walk"]]).astype(np.float32)
    return g[f"tlut_S{S}"], x, g[f"S{S}_KV{KV}_hat"].astype(np.float32), g[f"S{S}_KV{KV}_states"].astype(np.int32)


def spd_hessian(A):
    """H = A^T A / 512 + 1e-2 I in fp64 from the fixture's ternary A (as make_golden_viterbi.py builds it)."""
    Ai = A.astype(np.int64)
    return (Ai.T @ Ai).astype(np.float64) / A.shape[0] + 1e-2 * np.eye(A.shape[1])


def ldlq_case(g, name):
    """(W fp64, H fp64, reference Qidxs int32, reference hatW fp64) of the LDLQ case `name` (eye / spd)."""
    H = np.eye(256) if name == "eye" else spd_hessian(g["ldlq_A"])
    return (g["ldlq_W"].astype(np.float64), H, g[f"ldlq_{name}_Qidxs"].astype(np.int32),
            g[f"ldlq_{name}_hatW"].astype(np.float64))


def quantlut_sym(tlut16):
    """numpy restatement of the codebook of every trellis state: [65536, 2] fp32 (bitshift.py:71-79)."""
    S = int(tlut16.shape[0]).bit_length() - 1
    s = np.arange(1 << 16, dtype=np.int64)
    h = (s + 1) * s
    lut = tlut16.astype(np.float32)[(h >> (15 - S)) & ((1 << S) - 1)]
    lut[:, 0] *= 1 - ((h >> 15) & 1) * 2
    return lut


def proxy_err(W, hatW, H):
    dW = W - hatW
    return np.trace(dW @ H @ dW.T) / np.trace(W @ H @ W.T)


# ---------------------------------------------------------------------------------------------------------- CPU


@pytest.mark.parametrize("S,KV", COMBOS)
def test_fixture_is_self_consistent(g, S, KV):
    tlut, x, hat, st = codec(g, S, KV)
    assert st.shape == (32, 128) and hat.shape == (32, 256)
    # every reference walk is a tail-biting walk the packer accepts (32 tiles = a 64 x 128 matrix)
    dst = np.zeros((32, 8 * KV), dtype=np.int16)
    s16 = np.ascontiguousarray(st.astype(np.uint16))
    assert qp._native.lib().qpal_pack_tcq_states(dst.ctypes.data, s16.ctypes.data, 64, 128, KV) == 0
    lut = quantlut_sym(tlut)
    assert np.array_equal(lut[st].reshape(32, 256).view(np.uint32), hat.view(np.uint32))
    # a walk's own reconstruction: zero error is reachable.  The two-pass tail-biting search is a heuristic (its overlap comes
    # from an unconstrained pass) and may miss it by a few values when many states share a reconstruction (S9 KV10 does).
    walk = g["kinds"] == "walk"
    assert ((hat[walk] - x[walk]) ** 2).sum(axis=1).max() < 1e-2
    assert (hat[walk] == x[walk]).mean() > 0.99


def test_viterbi_symbols_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qpal.h")).read(), flags=re.S)
    lib = qp._native.lib()
    for s in ("qpal_tcq_viterbi", "qpal_tcq_viterbi_ws_bytes"):
        assert re.search(rf"\b{s}\s*\(", text) and s in qp._native.exported_symbols() and hasattr(lib, s)


def test_viterbi_argument_errors():
    lib = qp._native.lib()
    assert lib.qpal_tcq_viterbi_ws_bytes(1) == 0 and lib.qpal_tcq_viterbi_ws_bytes(11) == 0
    sizes = [lib.qpal_tcq_viterbi_ws_bytes(kv) for kv in range(2, 11)]
    assert all(0 < s < 1 << 28 for s in sizes)
    buf = np.zeros(1 << 16, dtype=np.uint64)
    p = buf.ctypes.data
    ok = dict(states=p, hat=p, x=p, tlut=p, B=4, S=9, KV=6, ws=p)

    def call(**kw):
        a = {**ok, **kw}
        return lib.qpal_tcq_viterbi(a["states"], a["hat"], a["x"], a["tlut"], a["B"], a["S"], a["KV"], a["ws"], None)

    # argument errors return before anything touches a device
    for kv in (1, 11):
        assert call(KV=kv) == -2
    for s in (8, 12):
        assert call(S=s) == -2
    assert call(B=0) == -1
    for name in ("states", "x", "tlut", "ws"):
        assert call(**{name: None}) == -3
    assert call(x=p + 1) == -4
    assert call(states=p + 2) == -4
    assert call(hat=p + 2) == -4
    assert call(ws=p + 4) == -4


# ---------------------------------------------------------------------------------------------------------- GPU


def _dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("S,KV", COMBOS)
def test_viterbi_bit_exact_against_reference(g, S, KV):
    dev = _dev()
    tlut, x, ref_hat, ref_st = codec(g, S, KV)
    hat, st = quantize.tcq_viterbi(torch.from_numpy(x).to(dev), torch.from_numpy(tlut).to(dev), KV)
    st, hat = st.cpu().numpy(), hat.cpu().numpy()
    for kind in np.unique(g["kinds"]):
        sel = g["kinds"] == kind
        assert np.array_equal(st[sel], ref_st[sel]), f"states differ for {kind}"
        assert np.array_equal(hat[sel].view(np.uint32), ref_hat[sel].view(np.uint32)), f"hat differs for {kind}"


@pytest.mark.gpu
@pytest.mark.parametrize("S,KV", [(9, 2), (9, 6), (11, 10)])
def test_viterbi_independent_of_batch_and_position(g, S, KV):
    dev = _dev()
    tlut, x, ref_hat, ref_st = (torch.from_numpy(a) for a in codec(g, S, KV))
    tlut = tlut.to(dev)
    gen = torch.Generator().manual_seed(KV)
    for B in (1, 7, 256, 3000):
        X = torch.randn(B, 256, generator=gen)
        pos = torch.randperm(B, generator=gen)[:min(B, 32)]
        X[pos] = x[:len(pos)]
        hat1, st1 = quantize.tcq_viterbi(X.to(dev), tlut, KV)
        hat2, st2 = quantize.tcq_viterbi(X.to(dev), tlut, KV)
        assert torch.equal(st1, st2) and torch.equal(hat1.view(torch.int32), hat2.view(torch.int32)), f"B={B}: runs differ"
        assert torch.equal(st1[pos].cpu(), ref_st[:len(pos)]), f"B={B}"
        assert torch.equal(hat1[pos].cpu(), ref_hat[:len(pos)]), f"B={B}"


@pytest.mark.gpu
@pytest.mark.parametrize("m,k,S,KV", [(256, 512, 9, 2), (256, 512, 9, 6), (256, 512, 10, 8), (256, 512, 11, 10),
                                      (4096, 4096, 9, 6)])
def test_make_tcq_linear_round_trip(g, m, k, S, KV):
    dev = _dev()
    tlut = torch.from_numpy(g[f"tlut_S{S}"])
    W = torch.randn(m, k, generator=torch.Generator().manual_seed(m + KV)).to(dev)
    trellis, hatW, info = quantize.quantize_tcq_weight(W, tlut, KV)
    assert 0 < info["err"] < 1
    layer = quantize.make_tcq_linear(W, tlut, KV)
    assert isinstance(layer, qp.QTIPLinearTCQ)
    assert torch.equal(layer.trellis.cpu(), trellis)
    Wg = layer.get_weight()
    assert torch.equal(Wg.view(torch.int16), hatW.half().view(torch.int16)), "dequant of the trellis must give hatW"
    # the module's info round trip rebuilds the same layer
    layer2 = qp.QTIPLinearTCQ.gen_layer_from_info(layer._info()).to(dev)
    assert torch.equal(layer2.get_weight(), Wg)
    Wd = hatW.double().cpu().numpy()
    for bs in (1, 16):
        x = torch.randn(bs, k, generator=torch.Generator().manual_seed(bs)).half()
        y = layer(x.to(dev)).float().cpu().numpy()
        xd = x.double().numpy()
        ref = xd @ Wd.T
        scale = np.abs(xd) @ np.abs(Wd).T
        tol = 1e-5 * scale + 2.0 ** -10 * np.abs(ref) + 1e-3  # smoke()'s bar
        assert np.all(np.abs(y - ref) <= tol), float(np.abs(y - ref).max())


@pytest.mark.gpu
def test_ldlq_identity_h_bit_exact(g):
    dev = _dev()
    tlut = torch.from_numpy(g["tlut_S9"])
    Wn, Hn, ref_q, ref_hat = ldlq_case(g, "eye")
    W, H = torch.from_numpy(Wn).to(dev), torch.from_numpy(Hn).to(dev)
    for h in (H, None):
        trellis, hatW, info = quantize.quantize_tcq_weight(W, tlut, 6, H=h)
        assert np.array_equal(info["Qidxs"].cpu().numpy(), ref_q)
        assert np.array_equal(hatW.double().cpu().numpy(), ref_hat)


@pytest.mark.gpu
def test_ldlq_spd_h(g):
    dev = _dev()
    tlut = torch.from_numpy(g["tlut_S9"])
    Wn, Hn, ref_q, ref_hat = ldlq_case(g, "spd")
    W, H = torch.from_numpy(Wn).to(dev), torch.from_numpy(Hn).to(dev)
    _, hatW, info = quantize.quantize_tcq_weight(W, tlut, 6, H=H)
    agree = (info["Qidxs"].cpu().numpy() == ref_q).mean()
    assert agree >= 0.99, agree
    ref = proxy_err(Wn, ref_hat, Hn)
    assert abs(info["proxy_err"] - ref) <= 0.005 * ref, (info["proxy_err"], ref)
    assert abs(proxy_err(Wn, hatW.double().cpu().numpy(), Hn) - info["proxy_err"]) <= 1e-9
    _, hat0, _ = quantize.quantize_tcq_weight(W, tlut, 6)
    assert info["proxy_err"] < proxy_err(Wn, hat0.double().cpu().numpy(), Hn)
