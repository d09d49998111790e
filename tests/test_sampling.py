"""qpal_lm_head_logits and qpal_sample on the GPU, and the sampled tail of decoder.DecodeStep / decoder.Prefill.

The logits are held to the bound the project already uses for this product (test_lm_head_argmax_one_launch).  A draw is judged on
the logits the kernel was given, by sampling.reference_draw's fp64 quantities, with no case excluded:
  * the token is in the top-k set (exact: raw fp32 comparisons);
  * with top-p: token in nucleus(top_p + EPS) and s64[token] >= max(s64 over nucleus(top_p - EPS)) - delta; else s64[token] >=
    max(s64 over the top-k set) - delta;
  * EPS = 2^-16.  The kernel's mass sums are EXACT in their summands (2^-40 fixed point in 64-bit integers, truncation <= 2^-23 of
    the total), so what is left is the error of one summand: exp((l - lmax) / T) in fp32 = a subtraction, a division and expf at
    2 ulp on an exponent of magnitude <= 40 where the mass matters: <= (40 * 2 + 2) * 2^-24 < 2^-17 relative.  EPS = 2^-16 is the
    figure derived for a 1024-lane fp32 sum and covers this one;
  * delta = 2^-18 * max(16, max|l| / T): three roundings and two logf at <= 2 ulp on magnitudes <= |z| + 17: <= 2^-21 of that, x 8;
  * cap: over all draws of the test the share whose token differs from reference_draw's exact winner is at most 1 %."""
import os
import sys

import numpy as np
import pytest
import torch

from qpalette_amd import sampling

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -16


@pytest.fixture(scope="module")
def qp():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import qpalette_amd
    qpalette_amd._native.lib()
    return qpalette_amd


def contract_check(l, T, top_k, top_p, seed, ctr, tok):
    """(exact, message): asserts the sandwich of the module docstring for one draw; exact: tok is reference_draw's winner"""
    vocab = l.shape[0]
    assert 0 <= tok < vocab
    want = sampling.reference_draw(l, T, top_k, top_p, seed, ctr)
    T32, P32 = float(np.float32(T)), float(np.float32(top_p))
    if not T32 > 0 or top_k == 1:
        assert tok == want, ("greedy", tok, want)
        return True
    lc = sampling.clean_logits(l)
    kmask = sampling.topk_mask(lc, top_k)
    assert kmask[tok], ("outside the top-k set", tok, top_k)
    z = lc.astype(np.float64) / T32
    s = sampling.race_scores(z, seed, ctr)
    fin = np.isfinite(lc)
    delta = 2.0 ** -18 * max(16.0, float(np.abs(lc[fin]).max()) / T32 if fin.any() else 0.0)
    inner = kmask
    if 0.0 < P32 < 1.0:
        p = sampling.probabilities(lc, T32, kmask)
        outer = sampling.nucleus_mask(p, kmask, P32 + EPS)
        inner = sampling.nucleus_mask(p, kmask, P32 - EPS)
        assert outer[tok], ("outside nucleus(top_p + eps)", tok, float(p[tok]))
    best = s[inner & (z > -np.inf)].max() if (inner & (z > -np.inf)).any() else -np.inf
    assert s[tok] >= best - delta, ("lost the race", tok, want, float(s[tok]), float(best), delta)
    return tok == want


# (temperature, top_k, top_p) by row type; top_k -1 stands for vocab + 10
TYPES = [(0.0, 0, 1.0), (0.6, 5, 1.0), (1.0, 0, 1.0), (0.8, 0, 0.95), (0.7, 50, 0.9), (0.9, -1, 1.0), "inactive"]


@pytest.mark.parametrize("rows,vocab,k,eps", [(1, 128256, 4096, 1e-5), (8, 128256, 4096, 1e-5), (128, 32000, 2048, 0.0),
                                               (65, 1000, 8192, 1e-5), (17, 33, 4096, 1e-5)])
def test_lm_head_logits(qp, rows, vocab, k, eps):
    """against W.float() @ x.float() with atol = 2e-3 max|ref|, rtol = 1e-3; columns vocab .. ld_logits untouched; two launches bitwise
    equal; rows = 1: within the same bound of qpal_lm_head_argmax's logits; strided h at rows = 8"""
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(vocab + rows)
    ld_h = k + 64 if rows == 8 else k
    hbuf = torch.randn(rows, ld_h, device=dev, generator=gen) * 2.0
    h = hbuf[:, :k]
    w_ln = (1.0 + 0.1 * torch.randn(k, device=dev, generator=gen)).half()
    W = (torch.randn(vocab, k, device=dev, generator=gen) * 0.05).half()
    if eps > 0:
        x = (h * torch.rsqrt((h * h).mean(dim=1, keepdim=True) + eps)).half() * w_ln
    else:
        x = h.half()
    ref = x.float() @ W.float().T
    pad = 3
    out = torch.full((rows, vocab + pad), 777.0, device=dev)
    got = qp.lm_head_logits(h, w_ln if eps > 0 else None, eps, W, out=out)
    torch.cuda.synchronize()
    assert got is out
    tol = 2e-3 * float(ref.abs().max())
    err = float((out[:, :vocab] - ref).abs().max())
    print(f"rows {rows} vocab {vocab} k {k}: max |err| {err:.3e}  atol {tol:.3e}  max |ref| {float(ref.abs().max()):.3f}")
    assert torch.allclose(out[:, :vocab], ref, atol=tol, rtol=1e-3)
    assert bool((out[:, vocab:] == 777.0).all())
    out2 = torch.full((rows, vocab + pad), 777.0, device=dev)
    qp.lm_head_logits(h, w_ln if eps > 0 else None, eps, W, out=out2)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32))
    if rows == 1:
        nat = qp._native
        wsb = nat.lib().qpal_lm_head_ws_bytes(vocab)
        ws = torch.zeros(wsb // 4, device=dev)
        lg = torch.empty(vocab, device=dev)
        tok = torch.zeros(1, dtype=torch.long, device=dev)
        nat.check(nat.lib().qpal_lm_head_argmax(h.data_ptr(), w_ln.data_ptr(), eps, W.data_ptr(), lg.data_ptr(), tok.data_ptr(), ws.data_ptr(),
                                                wsb, vocab, k, torch.cuda.current_stream(dev).cuda_stream), "qpal_lm_head_argmax")
        torch.cuda.synchronize()
        assert torch.allclose(out[0, :vocab], lg, atol=tol, rtol=1e-3)


def _make_sampler(qp, rows, vocab, dev, offset, seed0):
    types = [TYPES[(r + offset) % len(TYPES)] for r in range(rows)]
    smp = qp.Sampler(rows, vocab, dev,
                     temperature=[1.0 if t == "inactive" else t[0] for t in types],
                     top_k=[0 if t == "inactive" else (vocab + 10 if t[1] < 0 else t[1]) for t in types],
                     top_p=[1.0 if t == "inactive" else t[2] for t in types],
                     seed=[seed0 + 1000003 * r for r in range(rows)])
    return smp, types


def test_draws_against_the_contract(qp):
    """vocab {128256, 32000, 1000, 33} x rows {1, 8, 128} x logits N(0, 1), N(0, 2.5^2), three counters each: per-row mixed parameters
    in ONE launch (greedy, T 0.6 / k 5, T 1 / no filter, T 0.8 / p 0.95, k 50 with p 0.9, k > vocab, an inactive row)"""
    dev = torch.device("cuda", 0)
    draws = exact = 0
    case = 0
    for vocab in (128256, 32000, 1000, 33):
        for rows in (1, 8, 128):
            for sigma in (1.0, 2.5):
                case += 1
                gen = torch.Generator(device=dev).manual_seed(1000 + case)
                smp, types = _make_sampler(qp, rows, vocab, dev, offset=case, seed0=77 * case)
                smp.logits.copy_(torch.randn(rows, vocab, device=dev, generator=gen) * sigma)
                lcpu = smp.logits.cpu().numpy()
                seeds = smp.seed.cpu().tolist()
                for rep in range(3):
                    ctr = torch.tensor([-1 if t == "inactive" else (rep * 4099 + 17 * r + (1 << 33) * (r % 3 == 2)) for r, t in enumerate(types)],
                                       dtype=torch.int64, device=dev)
                    out = torch.full((rows,), -7, dtype=torch.int64, device=dev)
                    qp.sample(smp.logits, smp, ctr, out=out)
                    torch.cuda.synchronize()
                    toks, ctrs = out.cpu().tolist(), ctr.cpu().tolist()
                    for r, t in enumerate(types):
                        if t == "inactive":
                            assert toks[r] == -7, "an inactive row's token must keep its sentinel"
                            continue
                        k = vocab + 10 if t[1] < 0 else t[1]
                        exact += bool(contract_check(lcpu[r], t[0], k, t[2], seeds[r], ctrs[r], toks[r]))
                        draws += 1
    print(f"draws {draws}, exact winner {exact}, differing {draws - exact} ({100.0 * (draws - exact) / draws:.3f} %)")
    assert draws >= 2000
    assert draws - exact <= 0.01 * draws


def test_exact_ties(qp):
    """copies of the top logit at 7, 500 and vocab - 1: top_k = 1 -> the lowest index; top_k = 2 -> all copies kept, the token one of them"""
    dev = torch.device("cuda", 0)
    for vocab in (128256, 1000):
        l = torch.randn(2, vocab, device=dev, generator=torch.Generator(device=dev).manual_seed(vocab))
        top = float(l.max()) + 0.5
        l[:, [7, 500, vocab - 1]] = top
        smp = qp.Sampler(2, vocab, dev, temperature=0.9, top_k=[1, 2], seed=5)
        seen = set()
        for c in range(24):
            ctr = torch.full((2,), c, dtype=torch.int64, device=dev)
            tok = qp.sample(l, smp, ctr).cpu().tolist()
            assert tok[0] == 7
            assert tok[1] in (7, 500, vocab - 1)
            contract_check(l[1].cpu().numpy(), 0.9, 2, 1.0, 5, c, tok[1])
            seen.add(tok[1])
        assert len(seen) > 1, "three tied tokens, 24 counters: more than one of them must win"


@pytest.mark.parametrize("case", ["nan", "neg_inf"])
def test_degenerate_rows_give_a_valid_token(qp, case):
    dev = torch.device("cuda", 0)
    vocab = 5000
    l = torch.full((4, vocab), float("nan") if case == "nan" else float("-inf"), device=dev)
    smp = qp.Sampler(4, vocab, dev, temperature=[0.0, 0.7, 1.0, 0.8], top_k=[0, 5, 0, 50], top_p=[1.0, 1.0, 0.9, 0.9], seed=3)
    ctr = torch.arange(4, dtype=torch.int64, device=dev)
    for _ in range(2):
        out = torch.full((4,), -7, dtype=torch.int64, device=dev)
        qp.sample(l, smp, ctr, out=out)
        assert out.cpu().tolist() == [0, 0, 0, 0]
    # one NaN among ordinary logits is never drawn
    l2 = torch.randn(4, vocab, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    l2[:, 17] = float("nan")
    tok = qp.sample(l2, smp, ctr).cpu().tolist()
    for r in range(4):
        assert tok[r] != 17
        contract_check(l2[r].cpu().numpy(), float(smp.temperature[r]), int(smp.top_k[r]), float(smp.top_p[r]), 3, r, tok[r])


def test_a_draw_depends_on_seed_counter_and_logits_only(qp):
    """the same (seed, ctr, logits row, parameters) in row 0 of a 1-row launch and in row 77 of a 128-row launch: the same token; two
    launches bitwise equal; another ctr or seed over 64 draws at T = 1: not all equal"""
    dev = torch.device("cuda", 0)
    vocab = 128256
    gen = torch.Generator(device=dev).manual_seed(9)
    big = torch.randn(128, vocab, device=dev, generator=gen) * 1.5
    for T, k, p in ((1.0, 0, 1.0), (0.6, 5, 1.0), (0.8, 50, 0.9)):
        smp = qp.Sampler(128, vocab, dev, temperature=1.0, top_k=0, top_p=1.0, seed=list(range(128)))
        smp.set(77, temperature=T, top_k=k, top_p=p, seed=424242)
        ctr = torch.arange(128, dtype=torch.int64, device=dev)
        ctr[77] = 12345
        a = qp.sample(big, smp, ctr)
        b = qp.sample(big, smp, ctr)
        one = qp.Sampler(1, vocab, dev, temperature=T, top_k=k, top_p=p, seed=424242)
        c = qp.sample(big[77:78].clone(), one, ctr[77:78].clone())
        torch.cuda.synchronize()
        assert torch.equal(a, b)
        assert int(a[77]) == int(c[0])
    one = qp.Sampler(1, vocab, dev, temperature=1.0, seed=1)
    row = big[:1].contiguous()
    by_ctr = {int(qp.sample(row, one, torch.tensor([c], dtype=torch.int64, device=dev))[0]) for c in range(64)}
    by_seed = set()
    for s in range(64):
        one.set(0, seed=s)
        by_seed.add(int(qp.sample(row, one, torch.zeros(1, dtype=torch.int64, device=dev))[0]))
    assert len(by_ctr) > 1 and len(by_seed) > 1


# ---------------------------------------------------------------------------------------------------------------- the step

def _model(dev):
    sys.path.insert(0, os.path.join(ROOT, "perf"))
    from decode_llama import build_model
    return build_model("3_8b", "tcomb_6_7_0.5_none_0.9", None, 2, 4096, dev)


def _state(m, B, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    kc = [(torch.randn(B, 8, 512, 128, device=dev, generator=g) * 0.5).half() for _ in m.layers]
    vc = [(torch.randn(B, 8, 512, 128, device=dev, generator=g) * 0.5).half() for _ in m.layers]
    tok = torch.randint(0, 4096, (B,), device=dev, generator=g)
    pos = torch.tensor([10, 3, 100, 0, 250, 77, 31, 400][:B], dtype=torch.int64, device=dev)
    if B > 1:
        pos[5] = -1  # a free slot
    return kc, vc, tok, pos


def _check_step(smp, types, pos, out_tok, sentinel=None):
    torch.cuda.synchronize()
    logits, toks, ps, seeds = smp.logits.cpu().numpy(), out_tok.cpu().tolist(), pos.cpu().tolist(), smp.seed.cpu().tolist()
    n = 0
    for b, t in enumerate(types):
        if ps[b] < 0:
            if sentinel is not None:
                assert toks[b] == sentinel
            continue
        contract_check(logits[b], t[0], t[1], t[2], seeds[b], ps[b], toks[b])
        n += 1
    return n


@pytest.mark.parametrize("B", [1, 8])
def test_decode_step_with_a_sampler(qp, B):
    """DecodeStep(sampler=...) at B = 1 (the fused step) and B = 8 (one slot inactive), eager and from a captured graph replayed 3 times
    with pos advanced: every out_tok[b] passes the contract on sampler.logits[b] with ctr = pos[b]; top_k = 1 equals the greedy step
    where the top two logits are further apart than the logits bound; sampler=None is untouched"""
    dev = torch.device("cuda", 0)
    m = _model(dev)
    types = [(0.6, 5, 1.0), (1.0, 0, 1.0), (0.8, 0, 0.95), (0.7, 50, 0.9), (0.0, 0, 1.0), (1.0, 0, 1.0), (0.9, 5000, 1.0), (0.6, 5, 0.9)][:B]
    smp = qp.Sampler(B, 4096, dev, temperature=[t[0] for t in types], top_k=[t[1] for t in types], top_p=[t[2] for t in types],
                     seed=[11 + b for b in range(B)])

    def build(sampler, seed=5):
        kc, vc, tok, pos = _state(m, B, dev, seed)
        out = torch.full((B,), -7, dtype=torch.int64, device=dev)
        return qp.DecodeStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, tok, pos, out, sampler=sampler), tok, pos, out

    # the greedy step is what it was: two steps without a sampler on the same state agree bitwise and count the same launches
    g1, _, _, out_g1 = build(None)
    g2, _, _, out_g2 = build(None)
    g1(); g2()
    torch.cuda.synchronize()
    assert g1.launches_per_token == g2.launches_per_token and torch.equal(out_g1, out_g2)
    assert g1.batch1 == (B == 1) and g1.sampler is None
    # eager
    st, tok, pos, out = build(smp)
    assert st.launches_per_token == g1.launches_per_token + 1 and st.batch1 == (B == 1)
    st()
    assert _check_step(smp, types, pos, out, sentinel=-7) == (B if B == 1 else B - 1)
    # top_k = 1 on the same state: the greedy step's tokens where the top two logits are apart by more than the logits bound
    smp1 = qp.Sampler(B, 4096, dev, temperature=0.7, top_k=1, seed=3)
    s1, _, pos1, out1 = build(smp1)
    s1()
    torch.cuda.synchronize()
    top2 = smp1.logits.topk(2, dim=1).values
    bound = 2.0 * (2e-3 + 1e-3) * float(smp1.logits.abs().max())
    for b in range(B):
        if int(pos1[b]) < 0:
            continue
        assert int(out1[b]) == int(smp1.logits[b].argmax())
        if float(top2[b, 0] - top2[b, 1]) > bound:
            assert int(out1[b]) == int(out_g1[b]), (b, int(out1[b]), int(out_g1[b]))
    # captured, replayed with the positions advanced and the drawn tokens fed back
    st, tok, pos, out = build(smp, seed=6)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        st()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            st()
        for _ in range(3):
            g.replay()
            _check_step(smp, types, pos, out)
            tok.copy_(torch.where(pos >= 0, out, tok))
            pos += (pos >= 0).long()
        torch.cuda.synchronize()


@pytest.mark.parametrize("N", [5, 129])
def test_prefill_with_a_sampler(qp, N):
    """Prefill(sampler=...): the token is drawn with the slot's parameters and ctr = pos0 + N - 1 from sampler.logits[slot]"""
    dev = torch.device("cuda", 0)
    m = _model(dev)
    B, slot = 3, 1
    kc = [torch.zeros(B, 8, 512, 128, dtype=torch.float16, device=dev) for _ in m.layers]
    vc = [torch.zeros(B, 8, 512, 128, dtype=torch.float16, device=dev) for _ in m.layers]
    smp = qp.Sampler(B, 4096, dev, temperature=[1.0, 0.8, 0.0], top_k=[0, 50, 0], top_p=[1.0, 0.9, 1.0], seed=[1, 2, 3])
    pf = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, chunk=128, sampler=smp)
    toks = torch.randint(0, 4096, (N,), device=dev, generator=torch.Generator(device=dev).manual_seed(N))
    for pos0 in (0, torch.tensor([7], dtype=torch.int64, device=dev)):
        out = pf(toks, slot=slot, pos0=pos0)
        torch.cuda.synchronize()
        p0 = int(pos0) if not isinstance(pos0, torch.Tensor) else 7
        assert int(pf.ctr[0]) == p0 + N - 1
        contract_check(smp.logits[slot].cpu().numpy(), 0.8, 50, 0.9, 2, p0 + N - 1, int(out[0]))
    with pytest.raises(qp._native.QpalError):
        qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, sampler=qp.Sampler(2, 4096, dev))
