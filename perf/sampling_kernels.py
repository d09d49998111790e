#!/usr/bin/env python3
"""The two kernels of the sampled tail alone: qpal_lm_head_logits and qpal_sample at vocab 128 256 / k 4096 (Llama-3.1-8B), rows 1,
8, 64, 128.  Event-timed here (us per launch over --iters launches after --warmup); run it under
`rocprofv3 --kernel-trace --stats -- python perf/sampling_kernels.py` for the per-kernel figures.  Beside them: the lm_head stream floor
(vocab * k * 2 bytes at the stream rate qpal_calib_stream_read measures in this run) and the torch tail (norm, matmul, argmax).
Also qpal_logit_process in place on the same logits, with a neutral processor and with every stage on (penalties on
counted tokens, a mask, 64 bias entries per slot), beside a qpal_calib_stream_read of the bytes it moves: logits read, logits
written, counts read = 12 bytes per logit.
--grammar adds the launches of grammar-constrained decoding in the same call: qpal_grammar_mask on the same logits
(every row in the start state of a number pattern) next to the processor launches above, qpal_grammar_rows and qpal_grammar_advance
at 8 slots with drafts of 4 and 15 one-byte tokens (chains of dependent table reads), and GrammarBank.load of a 301-state automaton
(upload, compile launch, the check's read) on a synthetic vocabulary of --vocab tokens.

--top-logprobs N [N ...] adds qpal_top_logprob on the same logits, before any processor has touched them, between
its two yardsticks: qpal_token_logprob (two passes over the row) below and qpal_sample with top_k = N, top_p = 0.9 (eight passes)
above.  The three launches alternate for three rounds; the figures are the medians.

--truncation times the draw alone and nothing else: qpal_sample on every row type of tests/test_sampling.py, and
qpal_sample_trunc with neutral rows, min-p only (--min-p), top-a only (--top-a), typical-p only (--typical-p) and all three behind
top-k 50 / top-p 0.9.  Every figure is us per launch from a captured graph of --iters launches, replayed --rounds times; the
variants alternate within a round (A/B in one process), and median, least and largest round are kept.  --parent-lib PATH loads a
second build of the library (the parent commit's) and times its qpal_sample in the same rounds.

    python perf/sampling_kernels.py [--vocab 128256] [--k 4096] [--rows 1 8 64 128] [--iters 20] [--warmup 5] [--grammar]
                                    [--top-logprobs 5 20 64]
    python perf/sampling_kernels.py --truncation [--rows 1 8 128] [--min-p 0.05] [--top-a 0.2] [--typical-p 0.9] [--rounds 9]
                                    [--parent-lib PATH]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

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


NUMBER = r"-?(0|[1-9]\d*)(\.\d+)?"


def synthetic_table(vocab, seed=0):
    """a grammar.TokenTable of `vocab` made-up tokens: the 16 characters of "ab0123456789.-x " first, then strings of 1 .. 6 of them
    (2 % special tokens without bytes); eos is the last id"""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ab0123456789.-x ", np.uint8)
    lens = rng.integers(1, 7, size=vocab)
    lens[rng.random(vocab) < 0.02] = 0
    off = np.concatenate([[0], np.cumsum(lens)])
    data = alpha[rng.integers(0, len(alpha), size=off[-1])].tobytes()
    toks = [data[off[t]:off[t + 1]] for t in range(vocab)]
    toks[:len(alpha)] = [bytes([c]) for c in alpha][:vocab]
    toks[-1] = b"</s>"
    return qp.TokenTable(toks, eos=vocab - 1)


def grammar_launches(table, dev, iters, warmup):
    """rows / advance at 8 slots and drafts of 4 and 15 one-byte tokens, and the load of a 301-state automaton"""
    B, res = 8, {"slots": 8, "chains": []}
    bank = qp.GrammarBank(B, table, dev, grammars=2, max_states=301)
    bank.load(0, NUMBER)
    one = table.tok_bytes[table.tok_off[:-1].clip(max=table.total - 1)] == ord("1")
    digit = int(np.flatnonzero(one & (np.diff(table.tok_off) == 1))[0])      # the token "1": every draft stays alive
    for K in (4, 15):
        rows = B * (K + 1)
        tokens = torch.full((rows,), digit, dtype=torch.int64, device=dev)
        row0 = torch.arange(0, rows + 1, K + 1, dtype=torch.int32, device=dev)
        row_state = torch.zeros(rows, dtype=torch.int32, device=dev)
        out_tok, n_out = tokens.view(B, K + 1).clone(), torch.full((B,), K + 1, dtype=torch.int32, device=dev)

        def advance():
            bank.state.zero_()   # (a fill launch inside the timing, on both drafts alike: the walk starts at the start)
            qp.grammar_advance(bank, out_tok, n=n_out)
        for b in range(B):
            bank.set(b, 0)
        res["chains"].append({"draft": K, "rows": rows, "tokens_walked_per_slot": [K, K + 1],
                              "dependent_reads_per_token": 3,   # tok_off -> tok_bytes -> trans, each needs the one before
                              "us_grammar_rows": timed(lambda: qp.grammar_rows(bank, tokens, row0, row_state), iters, warmup),
                              "us_grammar_advance_with_state_fill": timed(advance, iters, warmup),
                              "us_state_fill_alone": timed(lambda: bank.state.zero_(), iters, warmup)})
        assert int(row_state.min()) >= 0, "a draft died: the chains are shorter than stated"
    dfa = qp.compile_regex("[ab]{300}")
    ms = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bank.load(1, dfa)        # upload, one compile launch, the check's read (a synchronisation)
        ms.append((time.perf_counter() - t0) * 1e3)
    res["load_301_states"] = {"ms_each": ms, "ms_median": sorted(ms)[2], "allow_bytes_written": 302 * bank.words * 4}
    lib, stream = qp._native.lib(), torch.cuda.current_stream(dev).cuda_stream
    res["load_301_states"]["us_compile_launch_alone"] = timed(lambda: qp._native.check(lib.qpal_grammar_compile(
        bank.trans[1].data_ptr(), bank.accept[1].data_ptr(), 301, *bank._vocab_args(), bank.allow[1].data_ptr(), bank.words, stream),
        "compile"), iters, warmup)
    return res


def top_logprob_launches(smp, ctr, tok, ns, iters, warmup):
    """qpal_top_logprob at every n of ns on smp.logits beside its yardsticks, three alternating rounds each: medians in us"""
    rows, dev, out = smp.B, smp.device, []
    lp = torch.zeros(rows, device=dev)
    for n in ns:
        ids, top = torch.zeros(rows, n, dtype=torch.int32, device=dev), torch.zeros(rows, n, device=dev)
        smp.temperature.fill_(1.0); smp.top_k.fill_(n); smp.top_p.fill_(0.9)
        launches = {"us_top_logprob": lambda: qp.top_logprobs(smp.logits, n, ids=ids, logprob=top, active=ctr),
                    "us_token_logprob": lambda: qp.token_logprobs(smp.logits, tok, out=lp, active=ctr),
                    "us_sample_topk_n_p0.9": lambda: qp.sample(smp.logits, smp, ctr, out=tok)}
        rounds = {name: [] for name in launches}
        for _ in range(3):
            for name, fn in launches.items():
                rounds[name].append(timed(fn, iters, warmup))
        res = {"n": n, "passes": {"us_top_logprob": 4, "us_token_logprob": 2, "us_sample_topk_n_p0.9": 8}}
        res.update({name: sorted(v)[1] for name, v in rounds.items()})
        res["rounds"] = rounds
        out.append(res)
    return out


# (temperature, top_k, top_p) by row type: tests/test_sampling.py::TYPES without the inactive row; top_k -1 stands for vocab + 10
SAMPLE_TYPES = {"greedy": (0.0, 0, 1.0), "t0.6_k5": (0.6, 5, 1.0), "t1_no_filter": (1.0, 0, 1.0), "t0.8_p0.95": (0.8, 0, 0.95),
                "t0.7_k50_p0.9": (0.7, 50, 0.9), "t0.9_k_above_vocab": (0.9, -1, 1.0)}


def truncation_launches(args, dev):
    """the measurement of DESIGN.md §30: graphs of args.iters launches each, replayed in alternation"""
    lib = qp._native.lib()
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(args.parent_lib)
        parent.qpal_sample.argtypes, parent.qpal_sample.restype = qp._native._SIGNATURES["qpal_sample"], ctypes.c_int
    s = torch.cuda.Stream(dev)
    out = {"what": "qpal_sample / qpal_sample_trunc alone, us per launch (graph replays of %d launches, %d alternating rounds)"
                   % (args.iters, args.rounds), "vocab": args.vocab, "parent_lib": args.parent_lib, "rows": []}
    gen = torch.Generator(device=dev).manual_seed(1)
    for rows in args.rows:
        logits = torch.randn(rows, args.vocab, device=dev, generator=gen) * 2.0
        ctr = torch.arange(rows, dtype=torch.int64, device=dev)
        variants = {}   # name -> (graph, passes over the row, the sampler that owns the parameter tensors)

        def capture(name, passes, smp, entry):
            tok = torch.zeros(rows, dtype=torch.int64, device=dev)
            head = [logits.data_ptr(), logits.stride(0) if rows > 1 else args.vocab, rows, args.vocab, smp.temperature.data_ptr(),
                    smp.top_k.data_ptr(), smp.top_p.data_ptr()]
            tail = [smp.seed.data_ptr(), ctr.data_ptr(), tok.data_ptr(), s.cuda_stream]
            trunc = [getattr(smp, n).data_ptr() for n in qp.sampling.TRUNCATION] if entry == "trunc" else []
            fn = {"new": lib.qpal_sample, "parent": parent.qpal_sample if parent else None, "trunc": lib.qpal_sample_trunc}[entry]
            with torch.cuda.stream(s):
                for _ in range(args.warmup):
                    qp._native.check(fn(*head, *trunc, *tail), name)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):
                    for _ in range(args.iters):
                        qp._native.check(fn(*head, *trunc, *tail), name)
            variants[name] = (g, passes, (smp, tok))

        for name, (t, k, p) in SAMPLE_TYPES.items():
            k = args.vocab + 10 if k < 0 else k
            passes = 1 + (3 if 1 < k < args.vocab and t > 0 else 0) + (4 if 0 < p < 1 and t > 0 else 0)
            smp = qp.Sampler(rows, args.vocab, dev, temperature=t, top_k=k, top_p=p, seed=list(range(rows)), truncation=True)
            capture("sample_" + name, passes, smp, "new")
            if parent:
                capture("parent_sample_" + name, passes, smp, "parent")
            capture("trunc_neutral_" + name, passes, smp, "trunc")
        for name, (t, k, p, mp, ta, ty, passes) in {
                "trunc_min_p": (1.0, 0, 1.0, args.min_p, 0.0, 1.0, 2), "trunc_top_a": (1.0, 0, 1.0, 0.0, args.top_a, 1.0, 3),
                "trunc_typical_p": (1.0, 0, 1.0, 0.0, 0.0, args.typical_p, 6),
                "trunc_all_three_k50_p0.9": (0.7, 50, 0.9, args.min_p, args.top_a, args.typical_p, 12)}.items():
            smp = qp.Sampler(rows, args.vocab, dev, temperature=t, top_k=k, top_p=p, min_p=mp, top_a=ta, typical_p=ty,
                             seed=list(range(rows)), truncation=True)
            capture(name, passes, smp, "trunc")
        us = {name: [] for name in variants}
        with torch.cuda.stream(s):
            for _ in range(args.rounds):
                for name, (g, _, _) in variants.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    g.replay()
                    e1.record(s)
                    e1.synchronize()
                    us[name].append(e0.elapsed_time(e1) / args.iters * 1e3)
        res = {"rows": rows, "launches": {}}
        for name, v in us.items():
            v = sorted(v)
            res["launches"][name] = {"passes": variants[name][1], "us_median": v[len(v) // 2], "us_min": v[0], "us_max": v[-1]}
        out["rows"].append(res)
        del variants
    print(json.dumps(out))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 8, 64, 128])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--top-logprobs", type=int, nargs="+", default=[], metavar="N",
                    help="also time qpal_top_logprob with these list lengths between qpal_token_logprob and qpal_sample(top_k = N, top_p = 0.9)")
    ap.add_argument("--grammar", action="store_true", help="also time the grammar launches (mask beside the processor, rows, advance, load)")
    ap.add_argument("--truncation", action="store_true", help="time qpal_sample and qpal_sample_trunc alone (DESIGN.md §30) and nothing else")
    ap.add_argument("--min-p", type=float, default=0.05)
    ap.add_argument("--top-a", type=float, default=0.2)
    ap.add_argument("--typical-p", type=float, default=0.9)
    ap.add_argument("--rounds", type=int, default=9, help="--truncation: alternating rounds of graph replays")
    ap.add_argument("--parent-lib", default=None, help="--truncation: another build of libqpal_hip.so whose qpal_sample is timed beside this one's")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    dev = torch.device("cuda", 0)
    if args.truncation:
        return truncation_launches(args, dev)
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
    table = synthetic_table(args.vocab) if args.grammar else None
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
        if args.top_logprobs:
            res["top_logprobs"] = top_logprob_launches(smp, ctr, tok, args.top_logprobs, args.iters, args.warmup)
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
        if args.grammar:   # every row in the start state of NUMBER: the digits and "-" stay, everything else becomes -inf
            bank = qp.GrammarBank(rows, table, dev, grammars=1, max_states=8)
            bank.load(0, NUMBER)
            for b in range(rows):
                bank.set(b, 0)
            res["us_grammar_mask"] = timed(lambda: qp.grammar_mask(smp.logits, bank, slots, ctr), args.iters, args.warmup)
            res["grammar_mask_tokens_allowed"] = int(torch.isfinite(smp.logits[0]).sum())
            proc = qp.LogitProcessor(rows, args.vocab, dev)
            res["us_logit_process_neutral_again"] = timed(lambda: qp.logits.process(smp.logits, proc, slots, ctr), args.iters, args.warmup)
            del bank, proc
        norm = lambda: torch.nn.functional.rms_norm(h.half(), (args.k,), w_ln, 1e-5)
        res["us_torch_tail_norm_matmul_argmax"] = timed(lambda: (norm() @ W.T).argmax(-1), args.iters, args.warmup)
        out["rows"].append(res)
        del smp
    if args.grammar:
        out["grammar"] = grammar_launches(table, dev, args.iters, args.warmup)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
