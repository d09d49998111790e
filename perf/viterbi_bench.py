#!/usr/bin/env python3
"""Rate of the TCQ encoder (qpal_tcq_viterbi, csrc/tcq_viterbi.hip) on one GPU, against a short pure-torch restatement
of the per-step gather / min update on the same GPU.

    python perf/viterbi_bench.py [--out profiles/viterbi_bench.json]

Per KV in (2, 6, 10), codebook S = 9 (KV <= 8) or KV + 1 (the quantiser strings' rule):
  sequences/s and state evaluations/s (2 passes x 128 steps x 65536 states per sequence) at B = 256, 4096, 65536;
  wall time of quantize_tcq_weight(W, tlut, KV) (H = None) for a 4096 x 4096 and a 14336 x 4096 layer;
  the torch restatement at B = 1024 (the same two passes), its sequences/s, and the speed-up of the kernel at B = 4096.
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

EVALS_PER_SEQ = 2 * 128 * 65536


def codebook(S, dev):
    g = torch.Generator().manual_seed(S)
    return torch.randn(1 << S, 2, generator=g).half().to(dev)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def recon_table(tlut):
    """[2, 65536] fp32 reconstruction of every state (quantlut_sym)."""
    S = tlut.shape[0].bit_length() - 1
    s = torch.arange(1 << 16, device=tlut.device, dtype=torch.int64)
    h = (s + 1) * s
    r = tlut.float()[(h >> (15 - S)) & ((1 << S) - 1)].T.contiguous()
    r[0] *= 1 - ((h >> 15) & 1) * 2
    return r


def torch_pass(x, rec, KV, start=None):
    """One Viterbi pass in plain torch over B sequences x [B, 256] (fp32 of fp16): per step gather the 2^KV predecessors of
    every group, min over them, add the new per-state error; then the backtrack.  start: the overlap of the tail-biting pass
    (first state's high bits = last state's low bits) or None."""
    B = x.shape[0]
    G, F = 1 << (16 - KV), 1 << KV
    pred = (torch.arange(G, device=x.device)[:, None] + (torch.arange(F, device=x.device) << (16 - KV))[None, :]).reshape(-1)

    def err(i):
        return (rec[0][None] - x[:, 2 * i, None]).square() + (rec[1][None] - x[:, 2 * i + 1, None]).square()

    cost = err(0)
    if start is not None:
        keep = (torch.arange(1 << 16, device=x.device)[None] >> KV) == start[:, None]
        cost = torch.where(keep, cost, torch.full_like(cost, float("inf")))
    back = []
    for i in range(1, 128):
        best, arg = cost[:, pred].reshape(B, G, F).min(dim=-1)
        back.append(arg.to(torch.int16))
        cost = err(i) + best.repeat_interleave(F, dim=1)
    if start is not None:  # end mask: the last state's low 16 - KV bits are the first state's high ones
        keep = (torch.arange(1 << 16, device=x.device)[None] & (G - 1)) == start[:, None]
        cost = torch.where(keep, cost, torch.full_like(cost, float("inf")))
    s = cost.argmin(dim=-1)
    states = [s]
    for i in range(127, 0, -1):
        g = s >> KV
        s = g + (back[i - 1].gather(1, g[:, None])[:, 0].long() << (16 - KV))
        states.append(s)
    return torch.stack(states[::-1], dim=1)


def torch_viterbi(x16, tlut, KV):
    x = x16.float()
    rec = recon_table(tlut)
    st = torch_pass(torch.roll(x, 128, 1), rec, KV)
    return torch_pass(x, rec, KV, start=st[:, 64] >> KV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--torch-batch", type=int, default=1024)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    qp._native.lib()
    res = {"device": torch.cuda.get_device_name(0), "rows": []}
    for KV in (2, 6, 10):
        S = 9 if KV <= 8 else KV + 1
        tlut = codebook(S, dev)
        row = {"KV": KV, "S": S, "ws_bytes": qp._native.lib().qpal_tcq_viterbi_ws_bytes(KV), "batch": []}
        for B in (256, 4096, 65536):
            X = torch.randn(B, 256, device=dev)
            t = timed(lambda: quantize.tcq_viterbi(X, tlut, KV), 3 if B < 65536 else 1)
            row["batch"].append({"B": B, "s": t, "seq_per_s": B / t, "state_evals_per_s": B * EVALS_PER_SEQ / t})
        for m, k in ((4096, 4096), (14336, 4096)):
            W = torch.randn(m, k, device=dev) * 0.02
            t0 = time.perf_counter()
            quantize.quantize_tcq_weight(W, tlut, KV)
            torch.cuda.synchronize()
            row[f"layer_{m}x{k}_s"] = time.perf_counter() - t0
        Bt = args.torch_batch
        X = torch.randn(Bt, 256, device=dev)
        x16 = X.half()
        st_ref = torch_viterbi(x16, tlut, KV)
        _, st = quantize.tcq_viterbi(X, tlut, KV)
        row["torch_agree"] = float((st_ref == st.long()).float().mean())
        tt = timed(lambda: torch_viterbi(x16, tlut, KV), 1)
        row["torch"] = {"B": Bt, "s": tt, "seq_per_s": Bt / tt, "layer_4096x4096_s_extrapolated": 65536 * tt / Bt}
        ours = next(r for r in row["batch"] if r["B"] == 4096)
        row["speedup_vs_torch"] = ours["seq_per_s"] / row["torch"]["seq_per_s"]
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
