#!/usr/bin/env python3
"""Rate of the VQ / SQ encoder (qpal_vq_encode, csrc/vq_encode.hip) on one GPU, against a pure-torch restatement of the
reference's per-group LDLQ_VQ loop on the same GPU.

    python perf/vq_quant_bench.py [--out profiles/vq_quant_bench.json]

Per (vec, bits) in (1, 6), (1, 8), (2, 6), (2, 10), (2, 12), (4, 8):
  vq_nearest at B = 2^16 and 2^22: seconds and codeword evaluations/s (B x 2^bits);
  wall time of quantize_vq_weight for a 4096 x 4096 and a 14336 x 4096 layer, H = None and an SPD H (block LDL included);
  the torch restatement (LDLQ_VQ's loop: per group a feedback matmul, torch.cdist, argmin) on the 4096 x 4096 layer with the
  same H, whether its codes agree, and the speed-up.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qpalette_amd as qp  # noqa: E402
from qpalette_amd import quantize  # noqa: E402

CODECS = [(1, 6), (1, 8), (2, 6), (2, 10), (2, 12), (4, 8)]


def codebook(vec, bits):
    g = torch.Generator().manual_seed(vec * 16 + bits)
    return torch.randn(1 << bits, vec, generator=g)


def spd(k, dev):
    g = torch.Generator().manual_seed(k)
    A = torch.randint(-1, 2, (2 * k, k), generator=g, dtype=torch.float64).to(dev)
    return A.T @ A / (2 * k) + 1e-2 * torch.eye(k, dtype=torch.float64, device=dev)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def torch_ldlq_vq(W, H, lut, buf_cols=128):
    """LDLQ_VQ (ldlq.py:16-58) as the reference runs it, on the GPU: block LDL, then per vec-group a feedback matmul,
    torch.cdist against the codebook and an argmin (the reference's vq_codebook.quantize)."""
    vec = lut.shape[1]
    m, n = W.shape
    C = lut.to(W.device, torch.float64)
    L = quantize.block_ldl(H, vec)
    L.fill_diagonal_(0)
    WT = W.T.contiguous()
    hatT = torch.zeros(n, m, dtype=torch.float64, device=W.device)
    QT = torch.zeros(n // vec, m, dtype=torch.int64, device=W.device)
    prod = torch.zeros(n, m, dtype=torch.float64, device=W.device)
    for r1 in range(n, 0, -buf_cols):
        r0 = r1 - buf_cols
        bW, bhat, bL = WT[r0:r1], hatT[r0:r1], L[r0:r1]
        for i in reversed(range(buf_cols // vec)):
            a, b = vec * i, vec * (i + 1)
            x = bW[a:b] + bL[b:, r0 + a:r0 + b].T @ (bW[b:] - bhat[b:]) + prod[r0 + a:r0 + b]
            st = torch.cdist(x.T, C).argmin(dim=-1)
            bhat[a:b] = C[st].T
            QT[(r0 + a) // vec] = st
        prod += bL.T @ (bW - bhat)
    return QT.T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    qp._native.lib()
    res = {"device": torch.cuda.get_device_name(0), "rows": []}
    H = {4096: spd(4096, dev)}
    W = torch.randn(4096, 4096, device=dev)
    for h in (None, H[4096]):  # first-call costs (library loads, solver and matmul set-up) stay out of the timings
        quantize.quantize_vq_weight(W, codebook(1, 6).to(dev), H=h)
    for vec, bits in CODECS:
        lut = codebook(vec, bits).to(dev)
        row = {"vec": vec, "bits": bits, "nearest": []}
        for B in (1 << 16, 1 << 22):
            X = torch.randn(B, vec, device=dev, dtype=torch.float64)
            quantize.vq_nearest(X, lut)
            t, _ = wall(lambda: quantize.vq_nearest(X, lut))
            row["nearest"].append({"B": B, "s": t, "codeword_evals_per_s": B * (1 << bits) / t})
        for m, k in ((4096, 4096), (14336, 4096)):
            W = torch.randn(m, k, device=dev)
            for name, h in (("none", None), ("spd", H[k])):
                t, _ = wall(lambda: quantize.quantize_vq_weight(W, lut, H=h))
                row[f"layer_{m}x{k}_{name}_s"] = t
        W = torch.randn(4096, 4096, device=dev, dtype=torch.float64)
        quantize.quantize_vq_weight(W[:, :256], lut, H=H[4096][:256, :256])  # warm the matmul / LDL paths
        t_ours, (_, _, info) = wall(lambda: quantize.quantize_vq_weight(W, lut, H=H[4096]))
        t_torch, q_ref = wall(lambda: torch_ldlq_vq(W, H[4096], lut))
        row["ldlq_4096x4096_spd"] = {"ours_s": t_ours, "torch_s": t_torch, "speedup_vs_torch": t_torch / t_ours,
                                     "codes_agree": float((q_ref == info["Qidxs"].long()).float().mean())}
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
