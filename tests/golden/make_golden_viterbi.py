#!/usr/bin/env python3
"""Generate tests/golden/viterbi.npz: the reference's own TCQ encoder (tail-biting Viterbi) and LDLQ, run on the CPU.

Like make_golden.py (whose import-time set-up is reused: absent third-party modules stubbed, ``torch.Tensor.cuda`` patched to
the identity), this only CALLS the reference's Python and writes data: inputs and the reference's outputs.

    TORCHDYNAMO_DISABLE=1 python tests/golden/make_golden_viterbi.py     # from the repository root

Reference entry points used (paths relative to the reference checkout):
  lib/codebook/bitshift.py   bitshift_codebook(L=16, KV, V=2, tlut_bits=S, decode_mode="quantlut_sym", tlut=...).quantize
  lib/utils/math_utils.py    block_LDL
  lib/algo/ldlq.py           LDLQ(..., for_kernel=True)

Contents (every value is stored in the narrowest dtype that holds it exactly):
  kinds               the kind of each of the 32 sequences (KINDS); the first 28 are the same for every codec:
  x                   fp16 [28, 256]   sequences of those kinds (fp16 values: the encoder rounds its input to fp16)
  tlut_S{S}           fp16 [2^S, 2]    the k-means codebook as the reference loads it, rounded to fp16 (QTIPLinearTCQ.tlut)
and for every (S, KV) of tcq.npz:
  S{S}_KV{KV}_walk    fp16 [4, 256]    the reconstructions of 4 random tail-biting walks: sequences 28..31
  S{S}_KV{KV}_hat     fp16 [32, 256]   reference reconstruction of the 32 sequences (exact in fp16)
  S{S}_KV{KV}_states  uint16 [32, 128] reference trellis states
and two LDLQ cases at m = 64, k = 256, S = 9, KV = 6 on one W (ldlq_W fp16 values; codebook tlut_S9): H = I and
H = A^T A / 512 + 1e-2 I with A = ldlq_A (int8 in {-1, 0, 1}, [512, 256]; spd_hessian() rebuilds H deterministically in fp64),
each with the reference's ldlq_{eye,spd}_Qidxs (uint16 [64, 128]) and ldlq_{eye,spd}_hatW (fp16 [64, 256]).
"""
import os
import sys

os.environ.setdefault("TORCHDYNAMO_DISABLE", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402  (sets up the reference import; chdirs into the reference checkout)

from lib.utils.math_utils import block_LDL  # noqa: E402
from lib.algo.ldlq import LDLQ  # noqa: E402

KINDS = ["gauss"] * 16 + ["zero"] * 2 + ["const"] * 2 + ["x4"] * 4 + ["x1e-3"] * 4 + ["walk"] * 4
NSHARED = 28
COMBOS = [(9, kv) for kv in range(2, 11)] + [(10, 8), (10, 9), (10, 10), (11, 9), (11, 10)]


def codebooks(S, KV):
    cb0 = mg.bitshift_codebook(L=16, KV=KV, V=2, tlut_bits=S, decode_mode="quantlut_sym")
    tlut16 = cb0.tlut.half()
    cb = mg.bitshift_codebook(L=16, KV=KV, V=2, tlut_bits=S, decode_mode="quantlut_sym", tlut=tlut16.float())
    return tlut16, cb


def shared_sequences(rng):
    X = np.zeros((NSHARED, 256), dtype=np.float32)
    for i, kind in enumerate(KINDS[:NSHARED]):
        if kind == "gauss":
            X[i] = rng.standard_normal(256)
        elif kind == "const":
            X[i] = 0.5 if i % 2 == 0 else -1.3
        elif kind == "x4":
            X[i] = 4 * rng.standard_normal(256)
        elif kind == "x1e-3":
            X[i] = 1e-3 * rng.standard_normal(256)
    return X.astype(np.float16)


def walk_sequences(rng, cb, KV):
    st = torch.from_numpy(mg.tail_biting_states(rng, len(KINDS) - NSHARED, KV)).to(torch.int32)
    rec = cb.recons(st).permute(1, 2, 0).reshape(len(st), 256)   # element 2t + v = pair v of state t
    return exact16(rec)


def spd_hessian(A):
    """H = A^T A / 512 + 1e-2 I in fp64: integer products, then one rounding each for / 512 and + 1e-2 (the tests rebuild it)."""
    Ai = A.astype(np.int64)
    return (Ai.T @ Ai).astype(np.float64) / A.shape[0] + 1e-2 * np.eye(A.shape[1])


def exact16(t):
    a = t.numpy().astype(np.float16)
    assert np.array_equal(a.astype(t.numpy().dtype), t.numpy()), "value not exact in fp16"
    return a


def gen_ldlq(W, H, cb):
    k = H.shape[0]
    L, _ = block_LDL(torch.from_numpy(H), 16)
    diag = torch.arange(k)
    L[diag, diag] = 0
    args = type("Args", (), {"td_x": 16, "td_y": 16, "V": 2})()
    hatW, Qidxs = LDLQ(torch.from_numpy(W.astype(np.float64)), L, cb, args, for_kernel=True)
    return dict(Qidxs=Qidxs.numpy().astype(np.uint16), hatW=exact16(hatW))


def main():
    rng = np.random.default_rng(20261015)
    out = {"kinds": np.array(KINDS)}
    shared = shared_sequences(rng)
    out["x"] = shared
    for S, KV in COMBOS:
        tlut16, cb = codebooks(S, KV)
        walks = walk_sequences(rng, cb, KV)
        X = np.concatenate([shared, walks])
        hat, states = cb.quantize(torch.from_numpy(X.astype(np.float32)))
        assert f"tlut_S{S}" not in out or np.array_equal(out[f"tlut_S{S}"], tlut16.numpy())
        out[f"tlut_S{S}"] = tlut16.numpy()
        out[f"S{S}_KV{KV}_walk"] = walks
        out[f"S{S}_KV{KV}_hat"] = exact16(hat)
        out[f"S{S}_KV{KV}_states"] = states.numpy().astype(np.uint16)
        print(f"viterbi S={S} KV={KV} ok", flush=True)
    tlut16, cb = codebooks(9, 6)
    W = rng.standard_normal((64, 256)).astype(np.float16)
    A = rng.integers(-1, 2, size=(512, 256)).astype(np.int8)
    out["ldlq_W"], out["ldlq_A"] = W, A
    for name, H in (("eye", np.eye(256)), ("spd", spd_hessian(A))):
        for key, v in gen_ldlq(W, H, cb).items():
            out[f"ldlq_{name}_{key}"] = v
        print(f"ldlq {name} ok", flush=True)
    np.savez_compressed(os.path.join(HERE, "viterbi.npz"), **out)


if __name__ == "__main__":
    main()
