#!/usr/bin/env python3
"""The whole calibration pipeline on one GPU, on a random Llama-shaped model:

    random_dense_model -> collect_hessians -> quantize_model (with and without `hess`) -> Score perplexity of the quantized layers
    and the dense forward's on held-out windows

Prints seconds per stage and, per linear, the proxy error tr(dW H dW^T) / tr(W H W^T) of the `hess` and of the `none` quantisation
(H = the collected S / ct of the linear's input; dW from the loaded layer's effective weight, read off with an identity batch), the
two models' nll next to the dense forward's, and how often the quantized model's most likely token is the dense forward's (on the
rows of each held-out window's last chunk, whose logits Score keeps).  Nothing here is gated: the figures are recorded.
Writes profiles/calibrate_llama.json.

    python perf/calibrate_llama.py [--hidden 2048 --inter 8192 --heads 16 --kv-heads 4 --layers 2 --vocab 4096]
                                   [--windows 16 --tokens 512 --heldout 4] [--quantizer tcq_4] [--out ...]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import qpalette_amd as qp
from qpalette_amd import calibrate
from qpalette_amd import quantize_layer as ql


def tlut(bits, seed=9):
    """a random Gaussian codebook at the rms the trellis quantiser expects (the library ships none)"""
    t = torch.randn(1 << bits, 2, generator=torch.Generator().manual_seed(seed))
    return (t / t.std(unbiased=False) * 0.9682458365518543).half()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def effective_weight(quant_dir, qstr, li, key, dev):
    """fp64 [out, in] of what the saved layer computes: its forward on an identity batch"""
    layer = qp.IncoherentLinear.gen_layer_from_quantizer_str_and_key(None, quant_dir, qstr, f"{li}_{key}", merge_layers=True).to(dev)
    k = layer.in_features
    return layer(torch.eye(k, dtype=torch.float16, device=dev)).double().T


def proxy_errors(model, hess_dir, quant_dir, qstr, dev):
    out = {}
    for li, L in enumerate(model.layers):
        H = {}
        for key in calibrate.LINEARS:
            hkey = calibrate.GROUP[key][0]
            if hkey not in H:
                H = {hkey: ql.load_hessian(calibrate.hessian_file_path(hess_dir, li, hkey), sigma_reg=0.0).to(dev)}
            W = L.weight(key).double()
            dW = W - effective_weight(quant_dir, qstr, li, key, dev)
            out[f"{li}_{key}"] = float(torch.trace(dW @ H[hkey] @ dW.T) / torch.trace(W @ H[hkey] @ W.T))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--inter", type=int, default=8192)
    ap.add_argument("--heads", type=int, default=16)
    ap.add_argument("--kv-heads", type=int, default=4)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--vocab", type=int, default=4096)
    ap.add_argument("--windows", type=int, default=16)
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--heldout", type=int, default=4)
    ap.add_argument("--quantizer", default="tcq_4", help="family and rate; _hess_0.9 / _none_0.9 are appended")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calibrate_llama.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("calibrate_llama.py needs a GPU")
    dev = torch.device("cuda", 0)
    work = tempfile.mkdtemp(prefix="qpal_calib_")
    hess_dir, rec = os.path.join(work, "hess"), {"args": vars(args), "device": torch.cuda.get_device_name(dev), "seconds": {}}
    try:
        rec["seconds"]["random_dense_model"], model = timed(lambda: calibrate.random_dense_model(
            args.hidden, args.inter, args.heads, args.kv_heads, args.layers, args.vocab, seed=0, device=dev))
        g = torch.Generator().manual_seed(1)
        windows = torch.randint(0, args.vocab, (args.windows, args.tokens), generator=g).to(dev)
        held = torch.randint(0, args.vocab, (args.heldout, args.tokens), generator=g).to(dev)
        rec["seconds"]["collect_hessians"], _ = timed(lambda: calibrate.collect_hessians(model, windows, hess_dir=hess_dir))
        rec["calibration_rows"] = args.windows * args.tokens
        cbs = {9: tlut(9)}
        rec["seconds"]["dense_logprobs"], (dense_lp, dense_top1) = timed(lambda: calibrate.dense_logprobs(model, held, top1=True))
        rec["dense_nll"] = -float(dense_lp.double().mean(1).mean())
        cfg = model.cfg
        shape = (1, cfg.num_key_value_heads, args.tokens, cfg.head_dim)
        c0 = (args.tokens - 1) // 128 * 128     # the first row of a window's last chunk
        for mode in ("hess", "none"):
            qstr, quant_dir = f"{args.quantizer}_{mode}_0.9", os.path.join(work, "quant_" + mode)
            rec["seconds"][f"quantize_model_{mode}"], layers = timed(
                lambda: calibrate.quantize_model(model, qstr, hess_dir, quant_dir, codebooks=cbs, seed=0))
            kc = [torch.zeros(shape, dtype=torch.float16, device=dev) for _ in layers]
            vc = [torch.zeros(shape, dtype=torch.float16, device=dev) for _ in layers]
            sc = qp.Score(layers, model.embed, model.norm, model.lm_head, kc, vc, model.inv_freq)
            lp = torch.empty(args.heldout, args.tokens - 1, dtype=torch.float32, device=dev)
            rec["seconds"][f"score_{mode}"], (ppl, nll) = timed(lambda: qp.perplexity(sc, held, out=lp))
            agree = []
            for w in range(args.heldout):
                sc(held[w])
                agree.append((sc.logits.argmax(-1) == dense_top1[w, c0:]).float().mean())
            rec[mode] = {"quantizer": qstr, "nll": nll, "ppl": ppl, "mean_abs_dlogprob_vs_dense": float((lp - dense_lp).abs().mean()),
                         "top1_agreement_with_dense": float(torch.stack(agree).mean()),
                         "proxy_err": proxy_errors(model, hess_dir, quant_dir, qstr, dev)}
            del sc, layers, kc, vc
    finally:
        shutil.rmtree(work, ignore_errors=True)
    for k, v in rec["seconds"].items():
        print(f"{k:28s} {v:8.2f} s")
    print(f"nll: dense {rec['dense_nll']:.4f}  hess {rec['hess']['nll']:.4f}  none {rec['none']['nll']:.4f};  top-1 agreement with "
          f"dense: hess {rec['hess']['top1_agreement_with_dense']:.3f}  none {rec['none']['top1_agreement_with_dense']:.3f}")
    print(f"{'linear':28s} {'proxy err (hess)':>18s} {'proxy err (none)':>18s}")
    for key in rec["hess"]["proxy_err"]:
        print(f"{key:28s} {rec['hess']['proxy_err'][key]:18.5f} {rec['none']['proxy_err'][key]:18.5f}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    return rec


if __name__ == "__main__":
    main()
