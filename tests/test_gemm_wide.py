"""The wide dequant GEMM (csrc/tcq_gemm_wide.hip): qpal_tcq_gemm_wide's return codes; linear.wide_gemm EQUAL to the
oracle's float64 sum on exactly summable inputs (tests/gemv_reference.py) at every row count where the kernel changes its path; its
fallback for the formats the kernel refuses; and Prefill(wide=256) on a two-layer model against the float64 reference and against
Prefill(chunk=128).

The issue's grid names a layer of 144 output rows.  The packed formats interleave the two 16-row tile rows of a 32-row supertile
row, so a trellis of 144 rows has no packed form (the oracle cannot decode one either) and every entry point takes m % 32 == 0: the
"partial block of supertile rows" case runs at m = 160 (5 of a workgroup's 8 rows), and m = 144 is one of the refused shapes."""
import functools

import numpy as np
import pytest
import torch

import gemv_reference as gx
import model_reference as mr
import qpalette_amd as qp

gpu = pytest.mark.gpu
F16, F8 = torch.float16, torch.float8_e4m3fn


# ------------------------------------------------------------------------------------------------------------- CPU: codes
def test_return_codes_and_wide_argument():
    lib, Job = qp._native.lib(), qp._native.TcqJob
    buf = np.zeros(1 << 16, dtype=np.uint8)
    p = buf.ctypes.data
    assert p % 16 == 0

    def call(n=256, S=9, KV1=6, KV2=0, njobs=1, **kw):
        jobs = (Job * 5)(*[Job(**dict(dict(out=p, c1=p, c2=p, x=p, tlut=p, m=4096, k=4096), **kw)) for _ in range(5)])
        return lib.qpal_tcq_gemm_wide(jobs, njobs, n, S, KV1, KV2, None)

    assert lib.qpal_tcq_gemm_wide(None, 1, 256, 9, 6, 0, None) == -3
    assert call(n=128) == -1 and call(n=257) == -1
    assert call(njobs=0) == -1 and call(njobs=5) == -1
    assert call(m=4104) == -1 and call(m=144) == -1               # m % 16, m % 32
    assert call(k=4160) == -1 and call(k=4224, KV2=7) == -1       # not whole 128-column steps (per stream)
    assert call(S=10, KV1=8) == -2 and call(KV1=9) == -2 and call(KV1=1) == -2 and call(KV2=9) == -2
    assert call(out=None) == -3 and call(c1=None) == -3 and call(x=None) == -3 and call(tlut=None) == -3
    assert call(c2=None, KV2=7) == -3
    assert call(x_had=1) == -2 and call(kv=6) == -2               # no rotation fusion, no per-job codec
    for wide in (128, 257, 0, True, "auto"):
        with pytest.raises(qp._native.QpalError, match="wide must be"):
            qp.Prefill([], torch.zeros(4, 64), None, torch.zeros(4, 64), [], [], None, wide=wide)


# ------------------------------------------------------------------------------------------------------------- GPU: exact
QSTRS = ("tcq_2_none_0.9", "tcq_8_none_0.9", "tcomb_6_7_0.5_none_0.9")
SHAPES = ((128, 256), (160, 256), (4096, 512), (128, 4096))   # one workgroup; 5 of its 8 rows; many blocks; few rows: K split 8 ways
NS = (129, 144, 145, 192, 193, 255, 256)


@functools.lru_cache(maxsize=None)
def _case(qstr, m, k, seed=0):
    """(layer on the GPU, x fp16 [256, k] on the GPU and as numpy, the oracle's W): rows 0 .. n - 1 of x serve every n"""
    gx.assert_budget(k, xmax=gx.amax_for(k))
    info = gx.exact_info(k, m, qstr, seed=m + k + seed, codebook_seed=5)
    x = gx.exact_x(256, k, seed=k)
    return qp.make_linear_from_info(qstr, info).cuda(), torch.from_numpy(x).cuda(), x, gx.oracle_weight(info)


def _wide(layers, x, n, fill=-7.0, rows=256, **kw):
    """wide_gemm on rows 0 .. n - 1 into buffers of `rows` rows filled with a sentinel; returns the whole buffers as numpy"""
    outs = [torch.full((rows, l.out_features), fill, dtype=torch.float32, device="cuda") for l in layers]
    qp.wide_gemm(layers, x[:n], [o[:n] for o in outs], **kw)
    return [o.cpu().numpy() for o in outs]


@gpu
@pytest.mark.parametrize("m,k", SHAPES)
@pytest.mark.parametrize("qstr", QSTRS)
def test_wide_gemm_equals_the_float64_sum(qstr, m, k):
    layer, x, xn, W = _case(qstr, m, k)
    want = gx.expected(W, xn)
    for n in NS:
        (got,) = _wide([layer], x, n)
        assert gx.same(got[:n], want[:n]), (n, gx.describe_difference(got[:n], want[:n]))
        assert (got[n:] == -7.0).all(), f"n {n}: rows past n were written"


@gpu
@pytest.mark.parametrize("variant", ["three_jobs", "scales", "accumulate", "ldo", "accumulate_split"])
def test_wide_gemm_variants(variant):
    n, qstr = 200, QSTRS[2]
    if variant == "three_jobs":   # unequal m, one launch
        cases = [_case(qstr, m, 512, seed=s) for s, m in enumerate((64, 288, 1024))]
        gots = _wide([c[0] for c in cases], cases[0][1], n)
        for got, c in zip(gots, cases):
            want = gx.expected(c[3], c[2])
            assert gx.same(got[:n], want[:n]), gx.describe_difference(got[:n], want[:n])
        return
    m, k = (128, 4096) if variant == "accumulate_split" else (160, 256)
    layer, x, xn, W = _case(qstr, m, k)
    want = gx.expected(W, xn)
    if variant == "scales":
        ws = (2.0 ** np.random.default_rng(1).integers(-2, 3, size=m)).astype(np.float16)
        gx.assert_budget(k, xmax=gx.amax_for(k), scale_max=4 * 0.5, scale_min=0.25 * 0.5)
        (got,) = _wide([layer], x, n, wscales=[torch.from_numpy(ws).cuda()], oscale=0.5)
        want = gx.expected(W, xn, wscale=ws, oscale=0.5)
    elif variant in ("accumulate", "accumulate_split"):
        base = gx.exact_base(256, m, seed=3)
        gx.assert_budget(k, xmax=gx.amax_for(k), base=64.0)
        out = torch.from_numpy(base).cuda()
        qp.wide_gemm([layer], x[:n], [out[:n]], accumulate=True)
        got, want = out.cpu().numpy(), gx.expected(W, xn, base=base)
        assert gx.same(got[n:], base[n:])
    else:                          # a column block of a wider buffer
        wide = torch.full((256, m + 96), -7.0, dtype=torch.float32, device="cuda")
        qp.wide_gemm([layer], x[:n], [wide[:n, 32:32 + m]])
        got = wide[:, 32:32 + m].cpu().numpy()
        assert bool((wide[:, :32] == -7.0).all()) and bool((wide[:, 32 + m:] == -7.0).all()) and bool((wide[n:] == -7.0).all())
    assert gx.same(got[:n], want[:n]), gx.describe_difference(got[:n], want[:n])


@gpu
def test_wide_gemm_falls_back_per_layer():
    """a mixed group at n = 200: the tcq layer takes the wide launch (exact), the ldlq and comb layers run multi_gemv on the two slices
    — bitwise what that call gives"""
    n, k, m = 200, 512, 256
    qstrs = ("ldlq_2_8_none_1.0", "comb_6_7_0.5_none_0.9", "tcq_6_none_0.9")
    infos = [gx.exact_info(k, m, q, seed=20 + i) for i, q in enumerate(qstrs)]
    layers = [qp.make_linear_from_info(q, info).cuda() for q, info in zip(qstrs, infos)]
    x = torch.from_numpy(gx.exact_x(n, k, seed=9)).cuda()
    gots = _wide(layers, x, n, rows=n)
    for layer, got in zip(layers[:2], gots[:2]):
        want = torch.cat([qp.multi_gemv([layer], x[r:r + 128])[0].float() for r in (0, 128)]).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert gx.same(gots[2], gx.expected(gx.oracle_weight(infos[2]), x.cpu().numpy()))


# ------------------------------------------------------------------------------------------------------------- GPU: whole model
CTX, LENS = 320, (129, 256, 257, 300)


@functools.lru_cache(maxsize=None)
def _model():
    """two layers of model_reference's small model, and its float64 / emulated forward on ONE 300-token prompt (causal: row N - 1 of it
    is the last row of the N-token prompt)"""
    dev = torch.device("cuda", 0)
    m = mr.build("S", "mixed", (), 2, mr.VOCAB, 0, dev, spec=mr.build_spec("S", "mixed", nlayers=2))
    toks = torch.randint(0, mr.VOCAB, (max(LENS),), generator=torch.Generator().manual_seed(4))
    return m, toks.to(dev), {kv: (mr.forward_fp64(m.ref, [toks], chunk=64, kv_dtype=kv),
                                   mr.forward_emulated(m.ref, [toks], chunk=64, prefill=True, kv_dtype=kv)) for kv in (None, F8)}


def _prefill(N, kind, **kw):
    """(token, last row of the stream, logits, caches as float, [slot's rows, the rest] masks) of one Prefill call into slot 1 of 2"""
    m, toks, _ = _model()
    dev = toks.device
    nkv, hd = m.cfg.num_key_value_heads, m.cfg.head_dim
    if kind == "paged":
        cache = qp.PagedKVCache(len(m.layers), 2 * (CTX // 16), nkv, 16, hd, 2, CTX // 16, dtype=F16, device=dev)
        cache.reserve(1, N)
        kc, vc, extra = cache.kpool, cache.vpool, dict(block_table=cache.table)
    else:
        dt = F8 if kind == "e4m3" else F16
        kc = [torch.zeros(2, nkv, CTX, hd, dtype=torch.uint8 if dt == F8 else F16, device=dev).view(dt) for _ in m.layers]
        vc, extra = [t.clone() for t in kc], {}
    smp = qp.Sampler(2, mr.VOCAB, dev, temperature=0.0)
    pf = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, sampler=smp, **extra, **kw)
    return pf, smp, toks[:N], kc + vc


@gpu
@pytest.mark.parametrize("N,kind", [(N, "fp16") for N in LENS] + [(257, "paged"), (257, "e4m3")])
def test_prefill_wide(N, kind):
    """Prefill(wide=256): the last row against the float64 forward within model_reference's tolerance (4 x the emulation's distance,
    DESIGN.md §28.3); the token and the caches against Prefill(chunk=128).  fp16 caches agree to the 2e-3 of two runs that round
    differently under float atomics, and bitwise where neither run writes; e4m3 bytes are one of 8 values per octave, so there the
    rows past the prompt and the other slot are compared (bitwise) and the prompt's rows are left to the reference check.

    Measured on an MI355X: err / tol of the stream 0.19 .. 0.33, of the logits 0.20 .. 0.33; the caches differ from chunk=128's as
    chunk=64's do (at most 1.95e-3 at N = 257)."""
    _, _, refs = _model()
    ref, emu = refs[F8 if kind == "e4m3" else None]
    got = {}
    for name, kw in (("wide", dict(wide=256)), ("chunk", dict(chunk=128))):
        pf, smp, toks, caches = _prefill(N, kind, **kw)
        tok = pf(toks, slot=1, pos0=0)
        got[name] = (int(tok), pf.last32[0].clone(), smp.logits[1].clone(), [c.clone() for c in caches])
    rows = [n - 1 for n in LENS]
    rh, rl = ref.stream[0][-1][rows], ref.logits[0][rows]
    tol_h = mr.tolerance(mr.e_h(emu.stream[0][-1][rows], rh))[LENS.index(N)]
    tol_l = mr.tolerance(mr.e_l(emu.logits[0][rows], rl))[LENS.index(N)]
    i = LENS.index(N)
    xh = float(mr.e_h(got["wide"][1][None], rh[i:i + 1]) / tol_h)
    xl = float(mr.e_l(got["wide"][2][None], rl[i:i + 1]) / tol_l)
    print(f"Prefill(wide=256) N {N} {kind}: err / tol stream {xh:.3f}, logits {xl:.3f}")
    assert xh <= 1.0 and xl <= 1.0
    assert got["wide"][0] == got["chunk"][0]
    for a, b in zip(got["wide"][3], got["chunk"][3]):
        if kind == "paged":
            torch.testing.assert_close(a.float(), b.float(), atol=2e-3, rtol=2e-3)
            continue
        assert torch.equal(a[0].view(torch.uint8), b[0].view(torch.uint8)) and torch.equal(a[1, :, N:].view(torch.uint8), b[1, :, N:].view(torch.uint8))
        assert bool(a[1, :, :N].float().abs().sum() > 0)
        if kind == "fp16":
            torch.testing.assert_close(a[1, :, :N].float(), b[1, :, :N].float(), atol=2e-3, rtol=2e-3)


@gpu
def test_prefill_wide_under_graph_capture():
    """N = 300 (chunks of 256 + 44) captured once and replayed three times: the eager call's token every time"""
    pf, _, toks, _ = _prefill(300, "fp16", wide=256)
    want = int(pf(toks, slot=1, pos0=0))
    torch.cuda.synchronize()
    s = torch.cuda.Stream(toks.device)
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = pf(toks, slot=1, pos0=0)
        for _ in range(3):
            out.fill_(-1)
            g.replay()
            torch.cuda.synchronize()
            assert int(out) == want
