#!/usr/bin/env python3
"""Generate tests/golden/vq_ldlq.npz: the reference's own fixed-codebook VQ / SQ quantiser (nearest codeword + LDLQ_VQ), run
on the CPU.

Like make_golden_viterbi.py this reuses make_golden.py's import-time set-up (absent third-party modules stubbed,
``torch.Tensor.cuda`` patched to the identity) and only CALLS the reference's Python; what it writes is data.

    TORCHDYNAMO_DISABLE=1 python tests/golden/make_golden_vq.py     # from the repository root

Reference entry points used (paths relative to the reference checkout):
  lib/codebook/vq_codebook.py  vq_codebook(vec_sz, lut_bits) (loads assets/lut_cache/vq_kmeans_<bits>_<vec>.pt), .quantize
  lib/utils/math_utils.py      block_LDL
  lib/algo/ldlq.py             LDLQ_VQ

Every decision of the reference is checked while it runs: the best and the second-best direct-form fp64 squared distance
differ by at least 1e-9 (1 + |x|^2), so any fp64 implementation must agree with it bit for bit (the reference's cdist is the
matmul form; the two may disagree only closer than that).  The tie cases are the exception, built to tie exactly in the
direct form.

Contents:
  W                   fp32 [64, 256]   rows 0..51 Gaussian, 52..55 zero, 56..59 x4, 60..63 x1e-3 Gaussian
  A                   int8 [512, 256]  H = A^T A / 512 + 1e-2 I (spd_hessian(); the tests rebuild it in fp64)
  lut_v{vec}_b{bits}  fp32 [2^bits, vec]  the codebook: the reference's cached one for vec 1, 2; seeded synthetic for vec 4
  v{vec}_b{bits}_{eye,spd}_Qidxs  uint16 [64, 256 / vec]  LDLQ_VQ's codes with H = I (use_hess=False) and with the SPD H
  tie_v{vec}_lut      fp32 [2^bits, vec]  a codebook with duplicated rows (vec 1: 4 bits, vec 2 and 4: 6 bits)
  tie_v{vec}_x        fp64 [n, vec]    exact midpoints of two nearest codewords, and duplicated codewords themselves
  tie_v{vec}_Qidxs    uint16 [n]       the lowest index of each tie (the direct-form argmin).  The reference agrees on every
                                       duplicated codeword; on a midpoint its matmul-form cdist may round the tie apart
"""
import os
import sys
import types

os.environ.setdefault("TORCHDYNAMO_DISABLE", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402,F401  (sets up the reference import; chdirs into the reference checkout)

# lib/utils/kmeans.py imports these; the fixture never fits a codebook
sys.modules["flash1dkmeans"].kmeans_1d = None
try:
    import sklearn.cluster  # noqa: F401
except ImportError:
    _sk, _skc = types.ModuleType("sklearn"), types.ModuleType("sklearn.cluster")
    _skc.KMeans = None
    _sk.cluster = _skc
    sys.modules["sklearn"], sys.modules["sklearn.cluster"] = _sk, _skc

from lib.codebook.vq_codebook import vq_codebook  # noqa: E402
from lib.utils.math_utils import block_LDL  # noqa: E402
from lib.algo.ldlq import LDLQ_VQ  # noqa: E402

CODECS = [(1, b) for b in (2, 4, 6, 8)] + [(2, b) for b in (2, 5, 6, 8, 10, 12)] + [(4, b) for b in (6, 8)]
TIE_CODECS = [(1, 4), (2, 6), (4, 6)]
M, K = 64, 256
MARGIN = 1e-9


def codebook(vec, bits, tlut=None):
    """A vq_codebook: the reference's constructor for the cached codebooks; for any other codebook an instance of the same class
    whose buffers hold `tlut` (the constructor would fit one with k-means)."""
    if tlut is None:
        return vq_codebook(vec_sz=vec, lut_bits=bits)
    cb = vq_codebook.__new__(vq_codebook)
    torch.nn.Module.__init__(cb)
    cb.idx_dtype, cb.vec_sz, cb.lut_bits = torch.int32, vec, bits
    cb.register_buffer("tlut", tlut)
    cb.register_buffer("lut", tlut.T.contiguous())
    return cb


def direct_dist(X, C):
    """[B, N] direct-form fp64 squared distances, summed over v in order."""
    d = (X[:, None, 0] - C[None, :, 0]) ** 2
    for v in range(1, X.shape[1]):
        d = d + (X[:, None, v] - C[None, :, v]) ** 2
    return d


def checked(cb):
    """Wrap cb.quantize: every decision agrees with the direct form and clears the margin."""
    quantize = cb.quantize
    C = cb.tlut.to(torch.float64)

    def q(X, **kw):
        hat, state = quantize(X, **kw)
        D = direct_dist(X.to(torch.float64), C)
        top2 = D.topk(2, dim=1, largest=False).values
        assert (top2[:, 1] - top2[:, 0] >= MARGIN * (1 + X.to(torch.float64).pow(2).sum(1))).all(), "decision inside the margin"
        assert torch.equal(state, D.argmin(dim=1)), "reference disagrees with the direct form"
        return hat, state

    cb.quantize = q
    return cb


def spd_hessian(A):
    """H = A^T A / 512 + 1e-2 I in fp64: integer products, then one rounding each for / 512 and + 1e-2 (the tests rebuild it)."""
    Ai = A.astype(np.int64)
    return (Ai.T @ Ai).astype(np.float64) / A.shape[0] + 1e-2 * np.eye(A.shape[1])


def make_w(rng):
    W = rng.standard_normal((M, K)).astype(np.float32)
    W[52:56] = 0
    W[56:60] *= 4
    W[60:64] *= np.float32(1e-3)
    return W


def ldlq(W, H, cb):
    L, _ = block_LDL(torch.from_numpy(H), cb.vec_sz)
    diag = torch.arange(H.shape[0])
    L[diag, diag] = 0
    _, Qidxs = LDLQ_VQ(torch.from_numpy(W.astype(np.float64)), L, cb)
    Q = Qidxs.numpy()
    assert Q.min() >= 0 and Q.max() < 1 << cb.lut_bits
    return Q.astype(np.uint16)


def tie_case(rng, tlut):
    """(codebook with n/8 (at most 8) duplicated rows, inputs that tie exactly): the duplicated codewords themselves, and the exact
    midpoints of n/4 (at most 16) codeword pairs that are each other's nearest with no third codeword as close to the midpoint."""
    n, vec = tlut.shape
    ndup, nmid = min(8, n // 8), min(16, n // 4)
    C = tlut.clone()
    src = torch.from_numpy(rng.choice(n // 2, ndup, replace=False))
    dst = torch.from_numpy(n // 2 + rng.choice(n // 2, ndup, replace=False))
    C[dst] = C[src]
    C64 = C.to(torch.float64)
    X, pairs = [C64[src]], set()
    for a in torch.from_numpy(rng.permutation(n)).tolist():
        if len(pairs) == nmid:
            break
        da = direct_dist(C64[a:a + 1], C64)[0]
        da[a] = float("inf")
        b = int(da.argmin())
        if (C64[a] == C64[b]).all() or (min(a, b), max(a, b)) in pairs:
            continue
        mid = (C64[a] + C64[b]) / 2
        d = direct_dist(mid[None], C64)[0]
        if d[a] == d[b] and (d > d[a]).sum() == n - 2:
            X.append(mid[None])
            pairs.add((min(a, b), max(a, b)))
    assert len(pairs) == nmid
    return C, torch.cat(X)


def main():
    rng = np.random.default_rng(20261016)
    W = make_w(rng)
    A = rng.integers(-1, 2, size=(512, K)).astype(np.int8)
    out = {"W": W, "A": A}
    H = {"eye": np.eye(K), "spd": spd_hessian(A)}
    luts = {}
    for vec, bits in CODECS:
        if vec == 4:
            tlut = torch.from_numpy(rng.standard_normal((1 << bits, vec)).astype(np.float32))
            cb = codebook(vec, bits, tlut)
        else:
            cb = codebook(vec, bits)
        assert cb.tlut.dtype == torch.float32 and tuple(cb.tlut.shape) == (1 << bits, vec)
        luts[vec, bits] = cb.tlut
        out[f"lut_v{vec}_b{bits}"] = cb.tlut.numpy()
        checked(cb)
        for name, h in H.items():
            out[f"v{vec}_b{bits}_{name}_Qidxs"] = ldlq(W, h, cb)
        print(f"vq vec={vec} bits={bits} ok", flush=True)
    for vec, bits in TIE_CODECS:
        C, X = tie_case(rng, luts[vec, bits])
        ndup = min(8, C.shape[0] // 8)
        _, state = codebook(vec, bits, C).quantize(X)
        D = direct_dist(X, C.to(torch.float64))
        assert ((D == D.min(dim=1, keepdim=True).values).sum(1) >= 2).all(), "every tie case ties"
        lowest = D.argmin(dim=1)  # CPU torch.argmin: the first of equal minima
        # a duplicated codeword's two distances are the same computation in any form: the reference takes the lower index too.
        # An exact midpoint ties only in the direct form; the reference's matmul-form cdist may round the two apart.
        assert torch.equal(state[:ndup], lowest[:ndup]), "the reference's duplicate goes to the lowest index"
        out[f"tie_v{vec}_lut"], out[f"tie_v{vec}_x"] = C.numpy(), X.numpy()
        out[f"tie_v{vec}_Qidxs"] = lowest.numpy().astype(np.uint16)
        print(f"ties vec={vec} ok ({int((state != lowest).sum())} midpoints rounded apart by the reference's cdist)", flush=True)
    np.savez_compressed(os.path.join(HERE, "vq_ldlq.npz"), **out)


if __name__ == "__main__":
    main()
