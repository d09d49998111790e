"""qpal_hessian_accum (csrc/hessian.hip) and calibrate.HessianAccumulator against calibrate.reference_hessian.

The gate, for every element the call owns (the 128 x 128 tiles on and below the diagonal):
    |H_ij - S_ij| <= 1.01 * F * 2^-23 * A_ij,   A_ij = sum_r |x_ri| |x_rj|,   F = 256
and the same for colsum with sum_r |x_rj|.  Derived: fp16 x fp16 products are exact in fp32; at most F of them are added in an fp32
accumulator before the partial sum goes to fp64, each addition within 2^-23 relative of a partial sum that |.| bounds by A; the fp64
part is below 1e-12 * A.  Measured on an MI355X: the printed max |err| / A of every case (DESIGN.md §20 quotes the largest)."""
import numpy as np
import pytest
import torch

import qpalette_amd as qp
from qpalette_amd import calibrate

F = 256
BOUND = 1.01 * F * 2.0 ** -23
TILE = qp._native.HESSIAN_TILE
SENTINEL = -7.25


# ---------------------------------------------------------------------------------------------------------- CPU


def test_symbol_exported():
    assert "qpal_hessian_accum" in qp._native.exported_symbols()
    getattr(qp._native.lib(), "qpal_hessian_accum")


@pytest.mark.parametrize("case,code", [
    (dict(n=0), -1), (dict(n=96, ld=96), -1), (dict(n=32832, ld=32832), -1), (dict(rows=-1), -1), (dict(ld=1016), -1),
    (dict(H=0), -3), (dict(X=0), -3),
    (dict(X=0x1008), -4), (dict(ld=1028), -4), (dict(H=0x2004), -4), (dict(colsum=0x3004), -4),
])
def test_argument_errors(case, code):
    """Every argument error returns before any stream work (fake device pointers: nothing is dereferenced)."""
    a = dict(H=0x2000, colsum=0x3000, X=0x1000, ld=1024, rows=5, n=1024)
    a.update(case)
    rc = qp._native.lib().qpal_hessian_accum(a["H"] or None, a["colsum"] or None, a["X"] or None, a["ld"], a["rows"], a["n"], None)
    assert rc == code


def test_zero_rows_launch_nothing():
    """rows = 0 is a success that reaches no stream: with pointers that belong to no device a launch could not return 0"""
    assert qp._native.lib().qpal_hessian_accum(0x2000, 0x3000, 0x1000, 1024, 0, 1024, None) == 0
    assert qp._native.lib().qpal_hessian_accum(0x2000, None, 0x1000, 64, 0, 64, None) == 0


def test_reference_hessian_by_hand():
    a = np.array([[1.0, 2.0], [3.0, -1.0]], dtype=np.float16)
    b = np.array([[0.5, 0.0]], dtype=np.float16)
    S, s, ct = calibrate.reference_hessian([a, b])
    assert ct == 3 and S.dtype == np.float64 and s.dtype == np.float64
    assert np.array_equal(S, np.array([[10.25, -1.0], [-1.0, 5.0]])) and np.array_equal(s, np.array([4.5, 1.0]))
    with pytest.raises(ValueError):
        calibrate.reference_hessian([a.astype(np.float32)])


def test_state_round_trip_through_load_hessian(tmp_path):
    """A state made from (S, s, ct), saved and read back by load_hessian, is the regularised S / ct."""
    n = 48
    x = (np.random.default_rng(3).standard_normal((100, n)) * 2 + 0.5).astype(np.float16)
    S, s, ct = calibrate.reference_hessian([x[:37], x[37:]])
    acc = calibrate.HessianAccumulator.from_sums(np.tril(S), s, ct)   # only the lower triangle is ever formed
    st = acc.state()
    assert set(st) == {"flatH", "mu", "n", "ct"} and st["n"] == n and st["ct"] == 100 and st["flatH"].shape == (n * (n + 1) // 2,)
    Hs = acc.hessian()
    assert torch.equal(Hs, Hs.T) and np.allclose(Hs.numpy(), S / ct, rtol=1e-15, atol=0)
    idx = torch.tril_indices(n, n)
    C = S / ct - np.outer(s / ct, s / ct)
    assert np.allclose(st["flatH"].numpy(), C[idx[0].numpy(), idx[1].numpy()], rtol=1e-12, atol=1e-14)
    path = acc.save(str(tmp_path / "h" / "0_qkv.pt"))
    H = qp.load_hessian(path, sigma_reg=0.01).numpy()
    want = S / ct
    want = want + 0.01 * np.trace(want) / n * np.eye(n)
    assert np.linalg.norm(H - want) <= 1e-12 * np.linalg.norm(want)


# ---------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    qp._native.lib()
    return torch.device("cuda", 0)


def _x(rows, n, seed):
    return (np.random.default_rng(seed).standard_normal((rows, n)) * 1.5).astype(np.float16)


def _owned(n):
    t = np.arange(n) // TILE
    return t[:, None] >= t[None, :]


def _sentinel_H(n, dev):
    H = torch.zeros(n, n, dtype=torch.float64, device=dev)
    H[torch.from_numpy(~_owned(n)).to(dev)] = SENTINEL
    return H


def _accum(H, cs, X, rows=None):
    rows = X.shape[0] if rows is None else rows
    rc = qp._native.lib().qpal_hessian_accum(H.data_ptr(), None if cs is None else cs.data_ptr(), X.data_ptr(), X.stride(0), rows,
                                             H.shape[0], torch.cuda.current_stream(H.device).cuda_stream)
    assert rc == 0
    return H


def _check(H, cs, xs, what, factor=1.0):
    """H, colsum (as started from _sentinel_H / zeros) against reference_hessian(xs): the gate on owned elements, the sentinel on
    the rest, bit for bit; returns the largest |err| / A"""
    n = H.shape[0]
    S, s, _ = calibrate.reference_hessian(xs)
    ax = np.abs(np.concatenate(xs).astype(np.float64))
    A, own = ax.T @ ax, _owned(n)
    Hh = H.cpu().numpy()
    assert np.all(np.isfinite(Hh))
    err = np.abs(Hh - S)
    ratio = float((err[own] / np.maximum(A[own], 1e-300)).max())
    cerr = np.abs(cs.cpu().numpy() - s)
    cratio = float((cerr / np.maximum(ax.sum(0), 1e-300)).max())
    print(f"{what}: max |err| / A = {ratio:.3e} (colsum {cratio:.3e}), bound {factor * BOUND:.3e}")
    assert np.all(err[own] <= factor * BOUND * A[own]), (what, ratio)
    assert np.all(cerr <= factor * BOUND * ax.sum(0)), (what, cratio)
    assert np.array_equal(Hh[~own].view(np.int64), np.full((~own).sum(), SENTINEL).view(np.int64)), "an upper tile was touched"
    return ratio


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 31, 33, 255, 257, 300])
@pytest.mark.parametrize("n", [64, 192, 448, 1024])
def test_kernel_against_reference(dev, n, rows):
    x = _x(rows, n, 1000 * n + rows)
    X = torch.from_numpy(x).to(dev)
    H, cs = _sentinel_H(n, dev), torch.zeros(n, dtype=torch.float64, device=dev)
    _accum(H, cs, X)
    torch.cuda.synchronize()
    _check(H, cs, [x], f"n={n} rows={rows}")
    # an asymmetric spot check of the orientation: the whole diagonal tile is written, H[1][0] is x_1 . x_0
    x64 = x.astype(np.float64)
    assert abs(float(H[1, 0]) - x64[:, 1] @ x64[:, 0]) <= BOUND * (np.abs(x64[:, 1]) @ np.abs(x64[:, 0]))
    assert float(H[0, 1]) == float(H[1, 0])


@pytest.mark.gpu
def test_wide_matrix_offsets_beyond_4_gib(dev):
    """n = 28672 (the 70B down_proj width): byte offsets into H pass 2^32; compared on the device in fp64, tile row by tile row"""
    n, rows = 28672, 33
    X = (torch.randn(rows, n, device=dev, generator=torch.Generator(device=dev).manual_seed(5)) * 1.5).half()
    H = torch.full((n, n), SENTINEL, dtype=torch.float64, device=dev)
    for b in range(n // TILE):
        H[b * TILE:(b + 1) * TILE, :(b + 1) * TILE] = 0
    cs = torch.zeros(n, dtype=torch.float64, device=dev)
    _accum(H, cs, X)
    X64 = X.double()
    A64 = X64.abs()
    worst = 0.0
    for r0 in range(0, n, 2048):
        r1 = r0 + 2048
        own = (torch.arange(r0, r1, device=dev) // TILE)[:, None] >= (torch.arange(n, device=dev) // TILE)[None, :]
        S, A, Hb = X64[:, r0:r1].T @ X64, A64[:, r0:r1].T @ A64, H[r0:r1]
        err = (Hb - S).abs()
        assert bool((err[own] <= BOUND * A[own]).all()), r0
        assert bool((Hb[~own] == SENTINEL).all()), r0
        worst = max(worst, float((err[own] / A[own].clamp_min(1e-300)).max()))
    assert bool(((cs - X64.sum(0)).abs() <= BOUND * A64.sum(0)).all())
    print(f"n={n} rows={rows}: max |err| / A = {worst:.3e}, bound {BOUND:.3e}")


@pytest.mark.gpu
def test_strided_view_equals_contiguous_bit_for_bit(dev):
    n, rows = 448, 300
    wide = torch.from_numpy(_x(rows, n + 64, 7)).to(dev)
    Xv, Xc = wide[:, :n], wide[:, :n].contiguous()
    assert Xv.stride(0) == n + 64
    a, b = calibrate.HessianAccumulator(n, dev).add(Xv), calibrate.HessianAccumulator(n, dev).add(Xc)
    torch.cuda.synchronize()
    assert torch.equal(a.S.view(torch.int64), b.S.view(torch.int64)) and torch.equal(a.s.view(torch.int64), b.s.view(torch.int64))
    assert a.ct == b.ct == rows and bool(a.S.abs().sum() > 0)


@pytest.mark.gpu
def test_split_calls_and_repeatability(dev):
    """add(X[:k]); add(X[k:]) against add(X) within twice the bound; two identical sequences of calls give identical bits"""
    n, rows, k = 192, 300, 77
    x = _x(rows, n, 11)
    X = torch.from_numpy(x).to(dev)
    runs = []
    for _ in range(2):
        H, cs = _sentinel_H(n, dev), torch.zeros(n, dtype=torch.float64, device=dev)
        _accum(H, cs, X[:k])
        _accum(H, cs, X[k:])
        runs.append((H, cs))
    torch.cuda.synchronize()
    _check(runs[0][0], runs[0][1], [x], "split", factor=2.0)
    assert torch.equal(runs[0][0].view(torch.int64), runs[1][0].view(torch.int64))
    assert torch.equal(runs[0][1].view(torch.int64), runs[1][1].view(torch.int64))
    # the accumulator's view of the same: any leading shape, ct, a symmetric hessian()
    acc = calibrate.HessianAccumulator(n, dev).add(X.view(3, 100, n))
    assert acc.ct == rows
    Hm = acc.hessian()
    S, _, _ = calibrate.reference_hessian([x])
    assert torch.equal(Hm, Hm.T) and np.allclose(Hm.cpu().numpy(), S / rows, rtol=1e-4, atol=1e-4)


@pytest.mark.gpu
def test_outlier_column_stays_finite(dev):
    """+-60000 in every row of one column: 3.6e9 per product, an fp16 product or sum would be inf"""
    n, rows = 192, 300
    x = _x(rows, n, 13)
    x[:, 70] = np.where(np.arange(rows) % 3 == 0, -60000.0, 60000.0).astype(np.float16)
    H, cs = _sentinel_H(n, dev), torch.zeros(n, dtype=torch.float64, device=dev)
    _accum(H, cs, torch.from_numpy(x).to(dev))
    torch.cuda.synchronize()
    _check(H, cs, [x], "outlier")
    assert float(H[70, 70]) == pytest.approx(rows * 3.6e9, rel=BOUND)


@pytest.mark.gpu
def test_zero_rows_change_nothing(dev):
    n = 192
    H, cs = _sentinel_H(n, dev), torch.zeros(n, dtype=torch.float64, device=dev)
    H0 = H.clone()
    X = torch.from_numpy(_x(4, n, 17)).to(dev)
    _accum(H, cs, X, rows=0)
    torch.cuda.synchronize()
    assert torch.equal(H.view(torch.int64), H0.view(torch.int64)) and not bool(cs.any())
    assert calibrate.HessianAccumulator(n, dev).add(X[:0]).ct == 0


@pytest.mark.gpu
def test_graph_replay_adds_twice(dev):
    n, rows = 192, 257
    X = torch.from_numpy(_x(rows, n, 19)).to(dev)
    once, cs1 = _sentinel_H(n, dev), torch.zeros(n, dtype=torch.float64, device=dev)
    _accum(once, cs1, X)
    H, cs = torch.zeros(n, n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _accum(H, cs, X)
    H.zero_()
    cs.zero_()
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    own = torch.from_numpy(_owned(n)).to(dev)
    assert torch.equal(H[own], 2 * once[own]) and torch.equal(cs, 2 * cs1) and not bool(H[~own].any())
