"""The wide dequant GEMM of the VQ/SQ layers (csrc/lut_gemm_wide.h): qpal_lut_gemm_wide's return codes;
ops.lut_gemm_wide EQUAL to the oracle's float64 sum on exactly summable inputs (tests/gemv_reference.py) for one codec per decode
path, both row-group counts and the shapes at which the launch changes its path; the job fields; linear.wide_gemm's routing."""
import functools

import numpy as np
import pytest
import torch

import gemv_reference as gx
import qpalette_amd as qp

gpu = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------- CPU: codes
def test_return_codes():
    lib, Job = qp._native.lib(), qp._native.LutJob
    buf = np.zeros(1 << 16, dtype=np.uint8)
    p = buf.ctypes.data
    assert p % 16 == 0

    def call(n=256, bits=8, vec=2, njobs=1, **kw):
        jobs = (Job * 5)(*[Job(**dict(dict(out=p, qweight=p, x=p, lut=p, m=4096, k=4096), **kw)) for _ in range(5)])
        return lib.qpal_lut_gemm_wide(jobs, njobs, n, bits, vec, None)

    assert lib.qpal_lut_gemm_wide(None, 1, 256, 8, 2, None) == -3
    assert call(n=128) == -1 and call(n=257) == -1
    assert call(njobs=0) == -1 and call(njobs=5) == -1
    assert call(m=144) == -1 and call(k=4160) == -1 and call(ldo=4095) == -1
    assert call(bits=9, vec=1) == -2 and call(bits=13, vec=2) == -2
    assert call(m=144, bits=13) == -1 and call(bits=13, out=None) == -2       # shape before codec before NULL
    assert call(out=None) == -3 and call(qweight=None) == -3 and call(x=None) == -3 and call(lut=None) == -3
    assert call(x_had=1) == -2 and call(x_rms_eps=1e-5) == -2 and call(act_out=p) == -2 and call(x_K=28) == -2
    assert call(x=p + 8) == -4 and call(out=p + 2) == -4 and call(wscale=p + 1) == -4


# ------------------------------------------------------------------------------------------------------------- GPU: exact
# one codec per decode path: sq_dup pair table; pair table of 2^12 entries (the 4-copy image); two gathers per pair, 16 words per
# lane; 2 words per lane; 9-bit fields across dword boundaries; the largest vq2 codebook
QSTRS = ("ldlq_1_3_none_1.0", "ldlq_1_6_none_1.0", "ldlq_1_8_none_1.0", "ldlq_2_2_none_1.0", "ldlq_2_9_none_1.0", "ldlq_2_12_none_1.0")
SHAPES = ((160, 128), (32, 384), (128, 4096))   # 5 of a workgroup's 8 rows, one step; one row, three steps; K split 8 ways
NS = (129, 192, 193, 256)                        # 12 and 16 row groups, the last one with one row and full


@functools.lru_cache(maxsize=None)
def _case(qstr, m, k, seed=0):
    """((qweight, lut, m) on the GPU, (bits, vec), x fp16 [256, k] on the GPU and as numpy, the oracle's W)"""
    gx.assert_budget(k, xmax=gx.amax_for(k))
    info = gx.exact_info(k, m, qstr, seed=m + k + seed)
    x = gx.exact_x(256, k, seed=k)
    return ((info["qweight"].cuda(), info["lut"].cuda(), m), (info["lut_bits"], info["vec_sz"]), torch.from_numpy(x).cuda(), x,
            gx.oracle_weight(info))


def _sentinel(n_rows, m, fill=-7.0):
    return torch.full((n_rows, m), fill, dtype=torch.float32, device="cuda")


@gpu
@pytest.mark.parametrize("m,k", SHAPES)
@pytest.mark.parametrize("qstr", QSTRS)
def test_lut_gemm_wide_equals_the_float64_sum(qstr, m, k):
    job, codec, x, xn, W = _case(qstr, m, k)
    want = gx.expected(W, xn)
    for n in NS:
        out = _sentinel(256, m)
        qp.ops.lut_gemm_wide([job], x[:n], *codec, outs=[out[:n]])
        got = out.cpu().numpy()
        assert gx.same(got[:n], want[:n]), (n, gx.describe_difference(got[:n], want[:n]))
        assert (got[n:] == -7.0).all(), f"n {n}: rows past n were written"


@gpu
@pytest.mark.parametrize("variant", ["three_jobs", "accumulate", "accumulate_split", "ldo"])
def test_lut_gemm_wide_job_fields(variant):
    n, qstr = 200, QSTRS[4]
    if variant == "three_jobs":   # unequal m and three codebooks in one launch, per-row and per-launch scales (powers of two)
        k = 384
        cases = [_case(qstr, m, k, seed=s) for s, m in enumerate((64, 288, 32))]
        gx.assert_budget(k, xmax=gx.amax_for(k), scale_max=4 * 0.5, scale_min=0.25 * 0.5)
        ws = [(2.0 ** np.random.default_rng(s).integers(-2, 3, size=c[0][2])).astype(np.float16) for s, c in enumerate(cases)]
        gots = qp.ops.lut_gemm_wide([c[0] for c in cases], cases[0][2][:n], *cases[0][1], wscales=[torch.from_numpy(w).cuda() for w in ws],
                                    oscale=0.5)
        for got, c, w in zip(gots, cases, ws):
            want = gx.expected(c[4], c[3], wscale=w, oscale=0.5)
            assert gx.same(got.cpu().numpy(), want[:n]), gx.describe_difference(got.cpu().numpy(), want[:n])
        return
    m, k = (128, 4096) if variant == "accumulate_split" else (160, 128)
    job, codec, x, xn, W = _case(qstr, m, k)
    want = gx.expected(W, xn)
    if variant == "ldo":           # a column block of a wider buffer
        wide = _sentinel(256, m + 96)
        qp.ops.lut_gemm_wide([job], x[:n], *codec, outs=[wide[:n, 32:32 + m]])
        got = wide[:, 32:32 + m].cpu().numpy()
        assert bool((wide[:, :32] == -7.0).all()) and bool((wide[:, 32 + m:] == -7.0).all()) and bool((wide[n:] == -7.0).all())
    else:
        base = gx.exact_base(256, m, seed=3)
        gx.assert_budget(k, xmax=gx.amax_for(k), base=64.0)
        out = torch.from_numpy(base).cuda()
        qp.ops.lut_gemm_wide([job], x[:n], *codec, outs=[out[:n]], accumulate=True)
        got, want = out.cpu().numpy(), gx.expected(W, xn, base=base)
        assert gx.same(got[n:], base[n:])
    assert gx.same(got[:n], want[:n]), gx.describe_difference(got[:n], want[:n])


@gpu
def test_wide_gemm_routes_lut_layers(monkeypatch):
    """up | gate of one ldlq_2_8 codec at n = 256: ONE lut_gemm_wide launch, the oracle's sum; a SIMT-packed layer in the same call
    keeps the sliced path's bits"""
    n, k, m, qstr = 256, 512, 256, "ldlq_2_8_none_1.0"
    infos = [gx.exact_info(k, m, qstr, seed=30 + i) for i in range(3)]
    layers = [qp.make_linear_from_info(qstr, info).cuda() for info in infos[:2]] + [qp.VQLinearPackSIMT.gen_layer_from_info(infos[2], device="cuda")]
    x = torch.from_numpy(gx.exact_x(n, k, seed=9)).cuda()
    calls, real = [], qp.ops.lut_gemm_wide
    monkeypatch.setattr(qp.ops, "lut_gemm_wide", lambda jobs, x2, *codec, **kw: calls.append((len(jobs), codec)) or real(jobs, x2, *codec, **kw))
    outs = qp.wide_gemm(layers, x, [_sentinel(n, m) for _ in layers])
    assert calls == [(2, (8, 2))]
    for out, info in zip(outs[:2], infos):
        assert gx.same(out.cpu().numpy(), gx.expected(gx.oracle_weight(info), x.cpu().numpy()))
    step = layers[2].max_fused_batch   # (a SIMT packing's fused batch is 8 rows: its slices are that long)
    want = torch.cat([qp.multi_gemv([layers[2]], x[r:r + step])[0].float() for r in range(0, n, step)])
    assert torch.equal(outs[2].view(torch.int32), want.view(torch.int32))
