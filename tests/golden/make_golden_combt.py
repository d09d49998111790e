#!/usr/bin/env python3
"""Generate tests/golden/combt_ldlq.npz: the reference's own combt LDLQ quantiser and incoherence preprocessing, run on the CPU.

Like make_golden_vq.py this reuses make_golden.py's import-time set-up (absent third-party modules stubbed, ``torch.Tensor.cuda``
patched to the identity) and only CALLS the reference's Python; what it writes is data.

    TORCHDYNAMO_DISABLE=1 python tests/golden/make_golden_combt.py     # from the repository root

Reference entry points used (paths relative to the reference checkout):
  lib/codebook/bitshift.py       bitshift_codebook(L=16, KV, V=2, tlut_bits=S, decode_mode="quantlut_sym", tlut=...)
  lib/utils/math_utils.py        block_LDL
  lib/algo/ldlq.py               LDLQ_combt(..., for_kernel=True)
  lib/quantizer/tcq_quant.py     linear_to_incoherent_for_tcq(..., left_only=True)
  lib/quantizer/vq_quant.py      linear_to_incoherent_for_vq(..., left_only=True)
  lib/utils/matmul_had.py        matmul_hadUt: the reference's pure-torch transform.  Its matmul_hadUt_head goes through the
                                 third-party fast_hadamard_transform (absent); the preprocessing is run with matmul_hadUt_head
                                 replaced by matmul_hadUt on blocks of head_dim in fp32 — the same transform, as
                                 oracle/incoherent.py restates it.  IncoherentLinear (which needs the CUDA extensions) is
                                 replaced by a holder of the buffers the two functions write.

Contents (every value in the narrowest dtype that holds it exactly):
  W                    fp16 [64, 256]      rows 0..55 Gaussian, 56..59 x4, 60..63 x1e-3
  A                    int8 [512, 256]     H = A^T A / 512 + 1e-2 I (spd_hessian(); the tests rebuild it in fp64)
  tlut_S{S}            fp16 [2^S, 2]       the k-means codebook as the reference loads it, rounded to fp16 (the module's tlut)
  kv{a}_{b}_{eye,spd}_Qidxs  uint16 [64, 128]  LDLQ_combt's codes for tcomb (a, b), ratio 0.5, H = I and the SPD H
  kv{a}_{b}_{eye,spd}_hatW   fp16 [64, 256]    its reconstruction (exact in fp16)
and for k in (256, 448 = 28 * 16) (one W, SU and SPD H each; scale_override 0.9):
  pre{k}_W             fp16 [8, k]         the layer weight
  pre{k}_SU            int8 [k]            +-1
  pre448_A             int8 [128, 448]     H = spd_hessian(A) (k = 256: the A above)
  pre{k}_tcq_Wr, pre{k}_tcq_Wscale      fp32  linear_to_incoherent_for_tcq with the S = 9 codebook (Wr = linear.weight, Wscale [8])
  pre{k}_vq_Wr, pre{k}_vq_Wscale        fp32  linear_to_incoherent_for_vq
  pre{k}_HRr_rows      fp32 [16, k]        rows 0..15 of HRr (both paths compute the same; the fixture size).  HRr goes through fp32 in the reference, so fp32 holds it exactly.
"""
import os
import sys
import types

os.environ.setdefault("TORCHDYNAMO_DISABLE", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402  (sets up the reference import; chdirs into the reference checkout)

# lib/utils/kmeans.py (imported by vq_quant) imports these; the fixture never fits a codebook
sys.modules["flash1dkmeans"].kmeans_1d = None
try:
    import sklearn.cluster  # noqa: F401
except ImportError:
    _sk, _skc = types.ModuleType("sklearn"), types.ModuleType("sklearn.cluster")
    _skc.KMeans = None
    _sk.cluster = _skc
    sys.modules["sklearn"], sys.modules["sklearn.cluster"] = _sk, _skc

from lib.utils.math_utils import block_LDL  # noqa: E402
from lib.utils.matmul_had import matmul_hadUt  # noqa: E402
from lib.algo.ldlq import LDLQ_combt  # noqa: E402
from lib.quantizer import tcq_quant, vq_quant  # noqa: E402

CODECS = [(9, 5, 6), (9, 7, 8), (11, 9, 10)]
M, K = 64, 256
PRE = {256: 16, 448: 16}  # k -> rows of HRr stored
MPRE = 8


class _Holder(torch.nn.Module):
    """Stand-in for IncoherentLinear: the buffers linear_to_incoherent_for_* write (fp32, as they construct it)."""

    def __init__(self, in_features, out_features, hadU, hadV, bias, dtype):
        super().__init__()
        self.linear = torch.nn.Linear(in_features, out_features, bias=False, dtype=dtype)
        self.bias = None
        self.SU = torch.ones(in_features, dtype=dtype)
        self.SV = torch.ones(out_features, dtype=dtype)
        self.Wscale = torch.ones(out_features, dtype=dtype)

    def apply_rot_info(self):
        pass


def _hadUt_head(X, head_dim):
    """matmul_hadUt_head with the pure-torch transform: blocks of head_dim, fp32 inside, X's dtype out (matmul_had.py:95-120)."""
    n = X.shape[-1]
    return matmul_hadUt(X.reshape(-1, n // head_dim, head_dim).float()).reshape(X.shape).to(X.dtype)


tcq_quant.IncoherentLinear = vq_quant.IncoherentLinear = _Holder
tcq_quant.matmul_hadUt_head = vq_quant.matmul_hadUt_head = _hadUt_head


def spd_hessian(A):
    """H = A^T A / 512 + 1e-2 I in fp64: integer products, then one rounding each for / 512 and + 1e-2 (the tests rebuild it)."""
    Ai = A.astype(np.int64)
    return (Ai.T @ Ai).astype(np.float64) / A.shape[0] + 1e-2 * np.eye(A.shape[1])


def exact16(t):
    a = t.numpy().astype(np.float16)
    assert np.array_equal(a.astype(t.numpy().dtype), t.numpy()), "value not exact in fp16"
    return a


def exact32(t):
    a = t.numpy().astype(np.float32)
    assert np.array_equal(a.astype(t.numpy().dtype), t.numpy()), "value not exact in fp32"
    return a


def codebook(S, KV, tlut16):
    return mg.bitshift_codebook(L=16, KV=KV, V=2, tlut_bits=S, decode_mode="quantlut_sym", tlut=tlut16.float())


def combt(W, H, cb1, cb2):
    k = H.shape[0]
    L, _ = block_LDL(torch.from_numpy(H), 16)
    diag = torch.arange(k)
    L[diag, diag] = 0
    args = type("Args", (), {"td_x": 16, "td_y": 16, "V": 2})()
    hatW, Qidxs = LDLQ_combt(torch.from_numpy(W.astype(np.float64)), L, cb1, cb2, args, for_kernel=True)
    return Qidxs.numpy().astype(np.uint16), exact16(hatW)


def preprocess(rng, k, cb, out):
    W = rng.standard_normal((MPRE, k)).astype(np.float16)
    SU = np.where(rng.standard_normal(k) > 0, 1, -1).astype(np.int8)
    A = out["A"] if k == K else rng.integers(-1, 2, size=(128, k)).astype(np.int8)
    HR = torch.from_numpy(spd_hessian(A)).unsqueeze(-1)
    lin = torch.nn.Linear(k, MPRE, bias=False, dtype=torch.float16)
    lin.weight.data.copy_(torch.from_numpy(W))
    su = torch.from_numpy(SU.astype(np.float32))
    sv = torch.ones(MPRE)
    out[f"pre{k}_W"], out[f"pre{k}_SU"] = W, SU
    if k != K:
        out[f"pre{k}_A"] = A
    inc, HRr_t = tcq_quant.linear_to_incoherent_for_tcq(lin, cb, HR.clone(), 0.9, SU=su, SV=sv, hadU=k, hadV=MPRE, rot_info="skip_r",
                                                         left_only=True)
    out[f"pre{k}_tcq_Wr"], out[f"pre{k}_tcq_Wscale"] = exact32(inc.linear.weight.data), exact32(inc.Wscale.data)
    inc, HRr_v = vq_quant.linear_to_incoherent_for_vq(lin, HR.clone(), 0.9, SU=su, SV=sv, hadU=k, hadV=MPRE, rot_info="skip_r",
                                                      left_only=True)
    out[f"pre{k}_vq_Wr"], out[f"pre{k}_vq_Wscale"] = exact32(inc.linear.weight.data), exact32(inc.Wscale.data)
    assert torch.equal(HRr_t, HRr_v)
    out[f"pre{k}_HRr_rows"] = exact32(HRr_t[:PRE[k], :, 0])


def main():
    rng = np.random.default_rng(20261017)
    W = rng.standard_normal((M, K)).astype(np.float32)
    W[56:60] *= 4
    W[60:64] *= np.float32(1e-3)
    W = W.astype(np.float16)
    A = rng.integers(-1, 2, size=(512, K)).astype(np.int8)
    out = {"W": W, "A": A}
    H = {"eye": np.eye(K), "spd": spd_hessian(A)}
    for S, kv1, kv2 in CODECS:
        tlut16 = mg.bitshift_codebook(L=16, KV=kv1, V=2, tlut_bits=S, decode_mode="quantlut_sym").tlut.half()
        out[f"tlut_S{S}"] = tlut16.numpy()
        cb1, cb2 = codebook(S, kv1, tlut16), codebook(S, kv2, tlut16)
        for name, h in H.items():
            Q, hat = combt(W, h, cb1, cb2)
            out[f"kv{kv1}_{kv2}_{name}_Qidxs"], out[f"kv{kv1}_{kv2}_{name}_hatW"] = Q, hat
        print(f"combt S={S} KV=({kv1}, {kv2}) ok", flush=True)
    cb = codebook(9, 6, torch.from_numpy(out["tlut_S9"]))
    for k in PRE:
        preprocess(rng, k, cb, out)
        print(f"preprocess k={k} ok", flush=True)
    np.savez_compressed(os.path.join(HERE, "combt_ldlq.npz"), **out)


if __name__ == "__main__":
    main()
