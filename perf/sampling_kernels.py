#!/usr/bin/env python3
"""The two kernels of the sampled tail alone: qpal_lm_head_logits and qpal_sample at vocab 128 256 / k 4096 (Llama-3.1-8B), rows 1,
8, 64, 128.  Event-timed here (us per launch over --iters launches after --warmup); run it under
`rocprofv3 --kernel-trace --stats -- python perf/sampling_kernels.py` for the per-kernel figures.  Beside them: the lm_head stream floor
(vocab * k * 2 bytes at the stream rate qpal_calib_stream_read measures in this run) and the torch tail (norm, matmul, argmax).
Also qpal_logit_process in place on the same logits, with a neutral processor and with every stage on (penalties on
counted tokens, a mask, 64 bias entries per slot), beside a qpal_calib_stream_read of the bytes it moves: logits read, logits
written, counts read = 12 bytes per logit.

    python perf/sampling_kernels.py [--vocab 128256] [--k 4096] [--rows 1 8 64 128] [--iters 20] [--warmup 5]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import qpalette_amd as qp


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 8, 64, 128])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    W = (torch.randn(args.vocab, args.k, device=dev, generator=gen) * 0.02).half()
    w_ln = torch.ones(args.k, dtype=torch.float16, device=dev)
    # the stream floor of the lm_head read, measured: one launch that only reads W
    lib = qp._native.lib()
    sink = torch.zeros(4096, dtype=torch.uint8, device=dev)
    srcs, nbytes = (ctypes.c_void_p * 1)(W.data_ptr()), (ctypes.c_long * 1)(W.numel() * 2)
    stream = torch.cuda.current_stream(dev).cuda_stream
    us_stream = timed(lambda: qp._native.check(lib.qpal_calib_stream_read(srcs, nbytes, 1, sink.data_ptr(), 2048, stream), "stream"),
                      args.iters, args.warmup)
    out = {"what": "qpal_lm_head_logits / qpal_sample alone, us per launch (events)", "vocab": args.vocab, "k": args.k,
           "lm_head_bytes": W.numel() * 2, "us_stream_read_of_lm_head": us_stream, "tb_per_s_stream": W.numel() * 2 / us_stream * 1e-6,
           "rows": []}
    for rows in args.rows:
        h = torch.randn(rows, args.k, device=dev, generator=gen)
        ctr = torch.arange(rows, dtype=torch.int64, device=dev)
        tok = torch.zeros(rows, dtype=torch.int64, device=dev)
        res = {"rows": rows}
        smp = qp.Sampler(rows, args.vocab, dev, seed=list(range(rows)))
        res["us_lm_head_logits"] = timed(lambda: qp.lm_head_logits(h, w_ln, 1e-5, W, out=smp.logits), args.iters, args.warmup)
        for name, (t, k, p) in {"greedy": (0.0, 0, 1.0), "t1_no_filter": (1.0, 0, 1.0), "t0.6_k5": (0.6, 5, 1.0),
                                "t0.8_p0.95": (0.8, 0, 0.95), "t0.7_k50_p0.9": (0.7, 50, 0.9)}.items():
            smp.temperature.fill_(t); smp.top_k.fill_(k); smp.top_p.fill_(p)
            res["us_sample_" + name] = timed(lambda: qp.sample(smp.logits, smp, ctr, out=tok), args.iters, args.warmup)
        # the logit processor on these logits, in place; the stream yardstick reads as many bytes as it reads and writes
        slots = torch.arange(rows, dtype=torch.int32, device=dev)
        for name in ("neutral", "all_stages"):
            proc = qp.LogitProcessor(rows, args.vocab, dev)
            if name == "all_stages":
                proc.count.copy_(torch.randint(0, 3, proc.count.shape, device=dev, generator=gen, dtype=torch.int32))
                half = torch.arange(0, args.vocab, 2)
                for b in range(rows):
                    proc.set(b, repetition=1.3, presence=0.5, frequency=0.3)
                    proc.set_mask(b, half)
                    proc.set_bias(b, {int(i): 1.0 for i in half[:proc.bias_slots]})
            res["us_logit_process_" + name] = timed(lambda: qp.logits.process(smp.logits, proc, slots, ctr), args.iters, args.warmup)
            if name == "neutral":
                moved = 3 * rows * args.vocab * 4
                scratch = torch.zeros((moved + 15) // 16 * 4, dtype=torch.int32, device=dev)
                s2, n2 = (ctypes.c_void_p * 1)(scratch.data_ptr()), (ctypes.c_long * 1)(scratch.numel() * 4)
                res["logit_process_bytes"] = moved
                res["us_stream_read_same_bytes"] = timed(
                    lambda: qp._native.check(lib.qpal_calib_stream_read(s2, n2, 1, sink.data_ptr(), 2048, stream), "stream"), args.iters, args.warmup)
                del scratch
            del proc
        norm = lambda: torch.nn.functional.rms_norm(h.half(), (args.k,), w_ln, 1e-5)
        res["us_torch_tail_norm_matmul_argmax"] = timed(lambda: (norm() @ W.T).argmax(-1), args.iters, args.warmup)
        out["rows"].append(res)
        del smp
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
