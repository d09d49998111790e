"""The fused decode + GEMV (csrc/tc_kernels.h), the lockstep skinny GEMM (csrc/tc_gemm.h, tc_gemm16.h) and the SIMT GEMV held to
EQUALITY with the oracle's float64 sum, on inputs that every order of fp32 summation adds without rounding (grid,
budget rule, reference and seeded defects: gemv_reference.py).  The tolerance the other GEMV tests use, 1e-5 * sum |w x|, is wider
than one term of the sum; here one wrong weight, one lost or doubled term, one stale x element changes the expected bits.

CPU part (no marker): the grid is exact in fp16, every case of this file is inside the bit budget, fp32 accumulation gives the
reference's bits in every order tried, every seeded defect changes an output — and the share of those defects that the tolerance
bar passes is printed (test_share_of_defects_the_tolerance_bar_passes; the table of DESIGN.md §29.4).

GPU part (marked gpu): the public paths the tolerance tests use (qp.ops.get_op, layer._gemv, layer(x), qp.multi_gemv), every
output compared by value with gemv_reference.expected, and two calls of every case compared bit for bit.

What stays on the tolerance bar: rotations at k = 2048 and 14336 (k^-1/2 is no power of two: the staged x is rounded), the
RMSNorm-fused staging (a division by a root), the module path above the fused batch (an fp16 GEMM of a library)."""
import numpy as np
import pytest

import gemv_reference as gx

gpu = pytest.mark.gpu

TCQ_COMBOS = [(9, kv) for kv in range(2, 11)] + [(10, 8), (10, 9), (10, 10), (11, 9), (11, 10)]
TCQ_PAIRS = [(9, 2), (9, 3), (9, 5), (9, 6), (9, 7), (9, 9), (10, 8), (10, 9), (11, 9)]   # (S, KV) of the (KV, KV + 1) streams
LUT_CODECS = [("sq", b) for b in range(2, 9)] + [("sq_dup", b) for b in range(2, 5)] + [("vq2", b) for b in range(2, 13)]
CODEC_M, CODEC_K, CODEC_NS = 64, 512, (1, 3, 4, 8, 12, 40)   # 3 | 4: per-wave kernel | lockstep kernel

RUN_QSTRS = ("tcq_6_none_0.9", "tcq_7_none_0.9", "tcomb_6_7_0.5_none_0.9", "ldlq_2_9_none_1.0")
RAGGED = [(32, 64), (32, 32), (96, 160), (160, 96), (32, 4096), (4096, 32), (64, 14336), (2048, 2560), (992, 1056)]
RUN_SHAPES = [(32, 128 * st) for st in (1, 2, 3, 5, 8, 15, 16)] + RAGGED
RUN_NS = (1, 2, 8, 12, 17, 40, 128)

# three of test_gpu_parity.py's pair-mode shapes: 2 x 280 supertile rows (two streams), 2 x 160, 2 x 896 (two shared rows per pair)
PAIR_SHAPES = [("tcomb_6_7_0.5_none_0.9", 8960, 4096), ("tcq_5_none_0.9", 5120, 4096), ("tcq_6_none_0.9", 28672, 2048)]
WIDE = [("tcq_6_none_0.9", 256, 28672), ("tcomb_6_7_0.5_none_0.9", 256, 28672)]
MULTI_MS = [1024, 512, 512, 96, 2048, 32, 544, 256]
MULTI_QSTRS = ("tcq_6_none_0.9", "tcomb_6_7_0.5_none_0.9", "ldlq_2_8_none_1.0")
EPI_K, EPI_BASE, EPI_SCALES, EPI_OSCALE = 1024, 64, (0.5, 1.0, 2.0), 0.5
ROT_K, ROT_ONES, ROT_POSTS = 4096, 5, (1.0, 0.5)
SIMT_SHAPES = [(1, 2, 8199, 2560), (1, 7, 8199, 2560), (2, 3, 8199, 2560), (2, 9, 8199, 6144), (4, 6, 8199, 5120), (4, 12, 8199, 4096),
               (2, 5, 1024, 14336), (4, 8, 4096, 14336), (1, 4, 1023, 4096)]


def _budgets():
    """label -> bit_budget arguments of every case of this file"""
    b = {"every codec, k 512": dict(k=CODEC_K, xmax=gx.amax_for(CODEC_K))}
    for k in sorted({k for _, k in RUN_SHAPES} | {k for _, _, k in PAIR_SHAPES} | {k for _, _, k in WIDE} | {4096, 14336}
                    | {k for _, _, _, k in SIMT_SHAPES}):
        b[f"plain GEMV, k {k}"] = dict(k=k, xmax=gx.amax_for(k))
    b["epilogue, k 1024"] = dict(k=EPI_K, xmax=gx.amax_for(EPI_K), scale_max=max(EPI_SCALES) * EPI_OSCALE,
                                 scale_min=min(EPI_SCALES) * EPI_OSCALE, base=EPI_BASE)
    for post in ROT_POSTS:   # staged x: odd integers up to 5 in units of 2^-6 * post
        b[f"rotation, k 4096, post {post}"] = dict(k=ROT_K, xmax=ROT_ONES * post / 64, grid=gx.GRID_STEP * post / 64)
    return b


BUDGETS = _budgets()


# ===================================================================================================== CPU: the method itself
def test_grid_values_are_exact_in_fp16():
    g = gx.GRID.astype(np.float64)
    assert gx.GRID.dtype == np.float16 and g.size == 256 and len(np.unique(g)) == 256
    assert np.array_equal(g, np.arange(-128, 128) / 32.0) and g.min() == -4.0 and g.max() == 4.0 - 2.0 ** -5
    neg = (-gx.GRID).astype(np.float64)   # the TCQ sign flip: still multiples of the step, still within wmax
    assert np.array_equal(neg * 32, np.rint(neg * 32)) and np.abs(neg).max() == gx.WMAX
    cb = gx.grid_codebook((512, 2), 3).astype(np.float64)
    assert np.isin(cb, g).all()
    # entries coincide at the rate of chance, 1/256 (the price of a wrong gather going unseen, per weight)
    flat = gx.grid_codebook((1 << 14,), 5)
    rate = (flat[:-1] == flat[1:]).mean()
    assert abs(rate - 1 / 256) < 4 * np.sqrt(1 / 256 / flat.size), rate


def test_budgets_of_every_case(capsys):
    with capsys.disabled():
        for label, kw in BUDGETS.items():
            b = gx.bit_budget(**kw)
            print(f"\n[gemv-exact] budget {label}: {b:.0f} = 2^{np.log2(b):.2f}", end="")
            assert b <= gx.BUDGET_MAX, (label, b)
    # the amax rule fits at the widest k of each band, and one more would not fit one column later
    for k in (8192, 16384, 28672):
        assert gx.bit_budget(k, xmax=gx.amax_for(k)) <= gx.BUDGET_MAX < gx.bit_budget(k + 32, xmax=gx.amax_for(k) + 1)
    assert gx.bit_budget(4096, gx.WMAX, 3, gx.GRID_STEP) == 4096 * 4 * 3 * 32


FAMILIES = ("tcq_6_none_0.9", "tcomb_6_7_0.5_none_0.9", "comb_6_7_0.5_none_0.9", "ldlq_1_4_none_1.0", "ldlq_2_8_none_1.0")


@pytest.fixture(scope="module")
def family_cases():
    """(W fp16 [64, 4096], x fp16 [2, 4096], float64 reference) per family, computed once"""
    out = {}
    for i, qstr in enumerate(FAMILIES):
        W = gx.oracle_weight(gx.exact_info(4096, 64, qstr, seed=10 + i))
        x = gx.exact_x(2, 4096, seed=20 + i)
        out[qstr] = (W, x, gx.expected(W, x))
    return out


def _seq_sum32(p):
    """strictly sequential fp32 accumulation over the last axis (np.sum is pairwise; cumsum is not)"""
    return np.cumsum(p.astype(np.float32), axis=-1, dtype=np.float32)[..., -1]


@pytest.mark.parametrize("qstr", FAMILIES)
def test_fp32_accumulation_is_order_independent(family_cases, qstr):
    W, x, ref = family_cases[qstr]
    assert np.isin(W.astype(np.float64), np.append(gx.GRID.astype(np.float64), gx.WMAX)).all()
    p = W.astype(np.float32)[None, :, :] * x.astype(np.float32)[:, None, :]   # [n, m, k]; fp16 x fp16 is exact in fp32
    assert np.array_equal(p.astype(np.float64), W.astype(np.float64)[None] * x.astype(np.float64)[:, None])
    rng = np.random.default_rng(1)
    for _ in range(4):
        assert np.array_equal(_seq_sum32(p[..., rng.permutation(p.shape[-1])]), ref)
    assert np.array_equal(_seq_sum32(np.sort(p, axis=-1)), ref)            # all negative terms first: the largest partial sums
    assert np.array_equal(_seq_sum32(-np.sort(-p, axis=-1)), ref)
    blocks = _seq_sum32(p.reshape(*p.shape[:-1], -1, 32))                   # blocks of 32 (an MFMA chain), then the partials
    assert np.array_equal(_seq_sum32(blocks), ref)
    assert np.array_equal(_seq_sum32(blocks[..., ::-1]), ref)


@pytest.mark.parametrize("qstr", FAMILIES)
def test_every_seeded_defect_changes_an_output(family_cases, qstr):
    W, x, ref = family_cases[qstr]
    for kind in gx.DEFECTS:
        for seed in range(8):
            Wd, xd = gx.seeded_defect(kind, W, x, seed)
            bad = (Wd @ xd.T).T.astype(np.float32)   # (float64 product of exactly summable values, cast without loss)
            assert bad.shape == ref.shape and not np.array_equal(bad, ref), (qstr, kind, seed)
            assert (bad != ref).sum() <= (ref.size if kind in ("stale_x", "replica") else 2), (qstr, kind, seed)


def test_share_of_defects_the_tolerance_bar_passes(capsys):
    """The measurement that justifies this file, printed and not asserted: of all single seeded defects, the share
    whose effect stays within 1e-5 * sum |w x| — on the inputs the tolerance tests use (N(0,1) codebook, N(0,1) x) and, for
    comparison, on this file's inputs.  Under equality the share is 0 by construction (test_every_seeded_defect_changes_an_output)."""
    import qpalette_amd as qp
    from oracle import oracle
    qstr, m = "tcq_6_none_0.9", 64
    with capsys.disabled():
        for k in (4096, 14336, 28672):
            info = qp.mem_op.dummy_linear_info(k, m, qstr, seed=k, device="cpu")
            W = oracle.tcq_dequant(info["trellis"].numpy(), info["tlut"].numpy(), m, k, info["tlut_bits"], info["KV"])
            x = np.random.default_rng(k).standard_normal(k).astype(np.float16)
            sh = gx.shares_under_tolerance(W, x)
            We = gx.oracle_weight(gx.exact_info(k, m, qstr, seed=k))
            she = gx.shares_under_tolerance(We, gx.exact_x(1, k, seed=k))
            for name, s in (("N(0,1) inputs", sh), ("grid inputs", she)):
                print(f"\n[gemv-exact] share passing 1e-5 * sum|wx|, k={k}, {name}: " + ", ".join(f"{d} {100 * s[d]:.1f}%" for d in gx.DEFECTS),
                      end="")
                assert all(0.0 <= v <= 1.0 for v in s.values())


# ===================================================================================================== GPU
@pytest.fixture(scope="module")
def qp():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import qpalette_amd
    qpalette_amd._native.lib()  # fail loudly if the HIP library is missing
    return qpalette_amd


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _x(n, k, seed, amax=None):
    """exact x of a plain GEMV; the budget is asserted before anything is launched"""
    amax = gx.amax_for(k) if amax is None else amax
    gx.assert_budget(k, xmax=amax)
    return gx.exact_x(n, k, seed, amax)


def _np(y):
    return y.detach().cpu().numpy()


def _twice(fn):
    """fn() -> tensor or list of tensors; run twice -> two lists of numpy arrays"""
    import torch
    runs = []
    for _ in range(2):
        ys = fn()
        torch.cuda.synchronize()
        runs.append([_np(y).copy() for y in (ys if isinstance(ys, (list, tuple)) else [ys])])
    return runs


def _bits(a):
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _exact(runs, wants, what):
    first, second = runs
    assert len(first) == len(wants)
    for j, (a, b, want) in enumerate(zip(first, second, wants)):
        a, b = a.reshape(want.shape), b.reshape(want.shape)
        assert gx.same(a, want), f"{what} [output {j}]: {gx.describe_difference(a, want)}"
        assert np.array_equal(_bits(a), _bits(b)), f"{what} [output {j}]: two calls differ: {gx.describe_difference(b, a)}"


def _layers(qp, qstrs, infos, share=True):
    mods = [qp.make_linear_from_info(q, info).cuda() for q, info in zip(qstrs, infos)]
    if share and len(mods) > 1:
        qp.share_codebooks(mods)
    return mods


def _gemv_want(layer, W, x, y):
    """a few-row VQ / SQ layer answers batch <= 8 from its SIMT-order twin: fp16 output, one rounding of the exact sum"""
    return gx.expected(W, x, fp16_out=(y.dtype == np.float16))


# ----------------------------------------------------------------------------------------- every codec, n across the kernel boundary
@gpu
@pytest.mark.parametrize("S,KV", TCQ_COMBOS)
def test_every_tcq_codec(qp, S, KV):
    m, k = CODEC_M, CODEC_K
    info = gx.exact_info(k, m, f"tcq_{KV}_none_0.9", seed=S * 16 + KV, tlut_bits=S)
    W = gx.oracle_weight(info)
    tr, tl = _cuda(info["trellis"].numpy()), _cuda(info["tlut"].numpy())
    for n in CODEC_NS:
        x = _x(n, k, seed=n + KV)
        op = qp.ops.get_op(f"decompress_gemm_tcq_{m}_{n}_{k}_{S}_{KV}")
        xd = _cuda(x)
        _exact(_twice(lambda: op(tr, xd, tl)), [gx.expected(W, x)], f"tcq S {S} KV {KV} n {n}")


@gpu
@pytest.mark.parametrize("S,KV", TCQ_PAIRS)
def test_every_two_stream_codec(qp, S, KV):
    """combt (column halves, the fused two-stream kernel) and comb (row halves) of every (KV, KV + 1) pair"""
    m, k = CODEC_M, CODEC_K
    for kind in ("combt", "comb"):
        qstr = f"{'tcomb' if kind == 'combt' else 'comb'}_{KV}_{KV + 1}_0.5_none_0.9"
        info = gx.exact_info(k, m, qstr, seed=S * 16 + KV + (100 if kind == "comb" else 0), tlut_bits=S)
        W = gx.oracle_weight(info)
        t1, t2, tl = _cuda(info["trellis1"].numpy()), _cuda(info["trellis2"].numpy()), _cuda(info["tlut"].numpy())
        for n in CODEC_NS:
            x = _x(n, k, seed=n + 3 * KV)
            op = qp.ops.get_op(f"decompress_gemm_tcq_{kind}_{m}_{n}_{k}_{S}_{KV}_{KV + 1}")
            xd = _cuda(x)
            _exact(_twice(lambda: op(t1, t2, xd, tl)), [gx.expected(W, x)], f"{kind} S {S} KV {KV} n {n}")


@gpu
@pytest.mark.parametrize("vt,bits", LUT_CODECS)
def test_every_lut_codec(qp, vt, bits):
    m, k = CODEC_M, CODEC_K
    vec = 2 if vt == "vq2" else 1
    info = gx.exact_info(k, m, f"ldlq_{vec}_{bits}_none_1.0", seed=bits * 4 + vec)
    W = gx.oracle_weight(info)
    limit = qp.VQLinearPackTensorCore(k, m, bits, vec).max_fused_batch
    q, lut = _cuda(info["qweight"].numpy()), _cuda(info["lut"].numpy())
    for n in CODEC_NS:
        if n > limit:
            continue
        x = _x(n, k, seed=n + 5 * bits)
        op = qp.ops.get_op(f"decompress_gemm_{m}_{n}_{k}_{bits}_{vt}")
        xd = _cuda(x)
        _exact(_twice(lambda: op(q, xd, lut)), [gx.expected(W, x)], f"{vt} {bits} n {n}")
    x = _x(1, k, seed=bits)   # the op that writes a caller's tensor
    import torch
    out = torch.full((1, m), float("nan"), device="cuda")
    qp.ops.get_op(f"decompress_gemv_{m}_{k}_{bits}_{vt}")(q, _cuda(x), lut, out)
    assert gx.same(_np(out), gx.expected(W, x)), gx.describe_difference(_np(out), gx.expected(W, x))


# ----------------------------------------------------------------------------------------- run lengths, ragged K, every batch range
@gpu
@pytest.mark.parametrize("m,k", RUN_SHAPES)
def test_run_lengths_and_ragged_k(qp, m, k):
    """One supertile row whose K makes a run of 1, 2, 3, 5, 8, 15, 16 waves, and the ragged shapes of test_gpu_parity.py (partial
    steps, more waves than steps, tiny and long K), at batches 1, 2, 8 (per-wave kernel; few-row VQ layers: their SIMT twin) and
    12, 17, 40, 128 (lockstep kernels: 1, 2, 4, 8 groups of 16 batch rows, rows that do not fill a group)."""
    for qstr in RUN_QSTRS:
        if "ldlq_2_9" in qstr and (9 * k) % 64:
            continue   # (the packing has no such shape)
        if "tcomb" in qstr and k % 64:
            continue
        info = gx.exact_info(k, m, qstr, seed=m + k)
        W = gx.oracle_weight(info)
        layer = qp.make_linear_from_info(qstr, info).cuda()
        for n in RUN_NS:
            x = _x(n, k, seed=m * 7 + k + n)
            xd = _cuda(x)
            runs = _twice(lambda: layer._gemv(xd, n))
            _exact(runs, [_gemv_want(layer, W, x, runs[0][0])], f"{qstr} m {m} k {k} n {n}")


# ----------------------------------------------------------------------------------------- shared rows, split K
@gpu
@pytest.mark.parametrize("qstr,m,k", PAIR_SHAPES)
def test_rows_shared_by_two_workgroups(qp, qstr, m, k):
    """Pair mode: two projections onto outputs declared zeroed, the shared rows' halves meeting by atomics — and the plain launch
    of the same layers.  Onto zeros, 0 + a + b: exact in either order."""
    import torch
    infos = [gx.exact_info(k, m, qstr, seed=70 + i, codebook_seed=13) for i in range(2)]
    mods = _layers(qp, [qstr] * 2, infos)
    Ws = [gx.oracle_weight(info) for info in infos]
    for n in (1, 3):
        x = _x(n, k, seed=21 + n)
        xd = _cuda(x)
        wants = [gx.expected(W, x) for W in Ws]
        _exact(_twice(lambda: qp.multi_gemv(mods, xd)), wants, f"{qstr} m {m} n {n} plain")
        zeroed = lambda: qp.multi_gemv(mods, xd, outs=[torch.zeros(n, m, dtype=torch.float32, device="cuda") for _ in mods], outs_zeroed=True)
        _exact(_twice(zeroed), wants, f"{qstr} m {m} n {n} zeroed")


@gpu
def test_split_k_onto_a_prezeroed_output(qp):
    """down_proj (k = 14336, split K: atomics) onto the output that the gate | up launch zeroed, as test_prezero_and_out_zeroed"""
    import torch
    qstr = "tcomb_6_7_0.5_none_0.9"
    gu_infos = [gx.exact_info(4096, 2048, qstr, seed=s, codebook_seed=2) for s in (1, 2)]
    gate, up = _layers(qp, [qstr] * 2, gu_infos)
    info = gx.exact_info(14336, 4096, qstr, seed=3)
    down = qp.make_linear_from_info(qstr, info).cuda()
    W = gx.oracle_weight(info)
    x, xd = _x(1, 4096, seed=1), _x(1, 14336, seed=2)
    want = gx.expected(W, xd)
    outs = []
    for _ in range(2):
        out = torch.full((1, 4096), float("nan"), device="cuda")
        gu = qp.multi_gemv([gate, up], _cuda(x), prezero=out)
        assert torch.count_nonzero(out).item() == 0
        (y,) = qp.multi_gemv([down], _cuda(xd), outs=[out], outs_zeroed=True)
        assert y.data_ptr() == out.data_ptr()
        outs.append([_np(y)] + [_np(g) for g in gu])
    _exact(outs, [want] + [gx.expected(gx.oracle_weight(i), x) for i in gu_infos], "prezero + outs_zeroed")
    assert gx.same(_np(down._gemv(_cuda(xd), 1)), want)


@gpu
@pytest.mark.parametrize("qstr,m,k", WIDE)
def test_widest_k(qp, qstr, m, k):
    info = gx.exact_info(k, m, qstr, seed=5)
    W = gx.oracle_weight(info)
    layer = qp.make_linear_from_info(qstr, info).cuda()
    for n in (1, 16):
        x = _x(n, k, seed=n)
        assert np.abs(x).max() == 1
        xd = _cuda(x)
        _exact(_twice(lambda: layer._gemv(xd, n)), [gx.expected(W, x)], f"{qstr} k {k} n {n}")


# ----------------------------------------------------------------------------------------- multi-job launches
@gpu
@pytest.mark.parametrize("qstr", MULTI_QSTRS)
@pytest.mark.parametrize("njobs", [2, 3, 5, 8])
def test_multi_job_launches_early_and_late_staging(qp, qstr, njobs):
    """2, 3, 5, 8 jobs of unequal row counts in one launch, once with ONE codebook tensor (staged early, from preloaded kernel
    arguments) and once with equal-valued distinct tensors (ordinary staging): both equal the reference, hence each other — at
    every batch, also where the lockstep kernel's K split lets test_early_and_late_staging_agree only use allclose."""
    k, ms = 4096, MULTI_MS[:njobs]
    infos = [gx.exact_info(k, m, qstr, seed=50 + i, codebook_seed=2) for i, m in enumerate(ms)]
    Ws = [gx.oracle_weight(info) for info in infos]
    name = "tlut" if "tlut" in infos[0] else "lut"
    shared = _layers(qp, [qstr] * njobs, infos)
    assert len({getattr(l, name).data_ptr() for l in shared}) == 1
    apart = _layers(qp, [qstr] * njobs, infos, share=False)
    assert len({getattr(l, name).data_ptr() for l in apart}) == njobs
    assert [len(g) for g in qp.linear.launch_groups(shared)] == [njobs]
    for n in (1, 5, 33):
        x = _x(n, k, seed=njobs * 10 + n)
        xd = _cuda(x)
        wants = [gx.expected(W, x) for W in Ws]
        _exact(_twice(lambda: qp.multi_gemv(shared, xd)), wants, f"{qstr} {njobs} jobs n {n} shared codebook")
        _exact(_twice(lambda: qp.multi_gemv(apart, xd)), wants, f"{qstr} {njobs} jobs n {n} distinct codebooks")


@gpu
@pytest.mark.parametrize("kvs,ms", [((3, 6, 8), (4096, 1024, 1024)), ((2, 7), (2048, 1024)), ((8, 9, 10), (512, 256, 256)), ((9, 10), (1024, 32))])
def test_mixed_kv_projections_in_one_launch(qp, kvs, ms):
    """q | k | v of different bit widths: the any-KV kernel (TcqAny instantiations), one codebook image; set-up of
    test_mixed_kv_projections_share_one_launch.  Batch 12 goes out as one launch per codec."""
    k = 4096
    qstrs = [f"tcq_{kv}_none_0.9" for kv in kvs]
    infos = [gx.exact_info(k, m, q, seed=100 + i, codebook_seed=3 if kv <= 8 else 30 + kv) for i, (q, kv, m) in enumerate(zip(qstrs, kvs, ms))]
    mods = _layers(qp, qstrs, infos)
    sizes = sorted(len(g) for g in qp.linear.launch_groups(mods, mixed_kv=True))
    assert sizes == ([len(kvs)] if max(kvs) <= 8 else [1] * len(kvs)), (kvs, sizes)
    Ws = [gx.oracle_weight(info) for info in infos]
    for n in (1, 3, 8, 12):
        x = _x(n, k, seed=n)
        xd = _cuda(x)
        _exact(_twice(lambda: qp.multi_gemv(mods, xd)), [gx.expected(W, x) for W in Ws], f"KV {kvs} n {n}")


@gpu
@pytest.mark.parametrize("qstrs,ms", [(("tcomb_3_4_0.5_none_0.9", "tcq_6_none_0.9", "tcq_3_none_0.9"), (4096, 1024, 1024)),
                                      (("tcomb_6_7_0.5_none_0.9", "tcomb_2_3_0.5_none_0.9"), (2048, 1024)),
                                      (("tcq_5_none_0.9", "tcomb_7_8_0.5_none_0.9", "tcomb_4_5_0.5_none_0.9", "tcq_8_none_0.9"), (512, 2048, 96, 32))])
def test_tcomb_and_tcq_projections_in_one_launch(qp, qstrs, ms):
    """column-split and plain TCQ layers in one any-KV launch (per-job KV and KV2); set-up of
    test_tcomb_and_tcq_projections_share_one_launch"""
    k = 4096
    infos = [gx.exact_info(k, m, q, seed=200 + i, codebook_seed=3) for i, (q, m) in enumerate(zip(qstrs, ms))]
    mods = _layers(qp, qstrs, infos)
    assert [len(g) for g in qp.linear.launch_groups(mods, mixed_kv=True)] == [len(mods)], qstrs
    Ws = [gx.oracle_weight(info) for info in infos]
    for n in (1, 5, 8):
        x = _x(n, k, seed=40 + n)
        xd = _cuda(x)
        _exact(_twice(lambda: qp.multi_gemv(mods, xd)), [gx.expected(W, x) for W in Ws], f"{qstrs} n {n}")


@gpu
def test_batch_slices_of_a_multi_job_launch(qp):
    """q | k | v at a wide batch: every projection twice in the lockstep kernel's launch, once per slice of the batch"""
    k, qstr, ms = 4096, "tcomb_6_7_0.5_none_0.9", (1024, 256, 256)
    infos = [gx.exact_info(k, m, qstr, seed=40 + i, codebook_seed=11) for i, m in enumerate(ms)]
    mods = _layers(qp, [qstr] * 3, infos)
    Ws = [gx.oracle_weight(info) for info in infos]
    for n in (32, 40, 64, 96, 128):
        x = _x(n, k, seed=12 + n)
        xd = _cuda(x)
        _exact(_twice(lambda: qp.multi_gemv(mods, xd)), [gx.expected(W, x) for W in Ws], f"batch slices n {n}")


# ----------------------------------------------------------------------------------------- epilogues
@gpu
@pytest.mark.parametrize("qstr,ms", [("tcq_6_none_0.9", (1024, 256, 256)), ("tcomb_6_7_0.5_none_0.9", (512, 96, 32)), ("ldlq_2_9_none_1.0", (512,))])
def test_epilogue_scales_accumulate_and_strided_out(qp, qstr, ms):
    """out = acc * wscale[row] * oscale, wscale in {0.5, 1, 2}, oscale 0.5: exact scalings; `+=` onto an integer-valued fp32 base;
    outs that are column blocks of a wider buffer whose padding stays untouched (test_gemv_epilogue_scale_and_strided_out).  The
    budget counts the scales and the base."""
    import torch
    k, pad, total = EPI_K, 64, sum(ms)
    infos = [gx.exact_info(k, m, qstr, seed=40 + i, codebook_seed=7) for i, m in enumerate(ms)]
    mods = _layers(qp, [qstr] * len(ms), infos)
    Ws = [gx.oracle_weight(info) for info in infos]
    rng = np.random.default_rng(len(ms))
    ws = [rng.choice(np.array(EPI_SCALES), size=m).astype(np.float16) for m in ms]
    wsd = [_cuda(w) for w in ws]
    gx.assert_budget(**BUDGETS["epilogue, k 1024"])
    cols = np.cumsum((0,) + tuple(ms))
    for n in (1, 33):
        x = gx.exact_x(n, k, seed=n, amax=BUDGETS["epilogue, k 1024"]["xmax"])
        xd = _cuda(x)
        base = gx.exact_base(n, total + pad, seed=n, bmax=EPI_BASE)

        def plain():
            buf = torch.full((n, total + pad), -7.0, dtype=torch.float32, device="cuda")
            qp.multi_gemv(mods, xd, outs=list(buf[:, :total].split(list(ms), dim=1)), wscales=wsd, oscale=EPI_OSCALE)
            return buf

        def accumulate():
            buf = _cuda(base)
            qp.multi_gemv(mods, xd, outs=list(buf[:, :total].split(list(ms), dim=1)), wscales=wsd, oscale=EPI_OSCALE, accumulate=True)
            return buf

        want = np.full((n, total + pad), -7.0, dtype=np.float32)
        want_acc = base.copy()
        for j, (W, w) in enumerate(zip(Ws, ws)):
            blk = slice(cols[j], cols[j + 1])
            want[:, blk] = gx.expected(W, x, wscale=w, oscale=EPI_OSCALE)
            want_acc[:, blk] = gx.expected(W, x, wscale=w, oscale=EPI_OSCALE, base=base[:, blk])
        _exact(_twice(plain), [want], f"{qstr} n {n} scales, strided")
        _exact(_twice(accumulate), [want_acc], f"{qstr} n {n} scales, strided, accumulate")


# ----------------------------------------------------------------------------------------- rotation in the staging
@gpu
@pytest.mark.parametrize("post", ROT_POSTS)
def test_rotation_in_the_staging_k4096(qp, post):
    """x_rot = (su, post) at k = 4096, where k^-1/2 = 2^-6 is an exact scaling: x has five entries of +-1 (an odd count: no
    rotated element is zero), su is random +-1, and the staged vector is H (x su) / 64 * post — odd integers up to 5 in units of
    2^-6 post, computed here in integers.  fp16 x and the fp32 residual stream.  (k = 2048 and 14336 have no dyadic scale: their
    staged x is rounded, and they stay on the tolerance bar of test_incoherent.py / test_glue_exact.py.)"""
    import torch
    k = ROT_K
    gx.assert_budget(**BUDGETS[f"rotation, k 4096, post {post}"])
    rng = np.random.default_rng(int(post * 8))
    x = np.zeros((1, k), dtype=np.float16)
    x[0, rng.choice(k, size=ROT_ONES, replace=False)] = rng.integers(0, 2, ROT_ONES) * 2.0 - 1.0
    su = (rng.integers(0, 2, k) * 2 - 1).astype(np.float16)
    xr = gx.rotated_x(x, su, post)
    assert np.abs(xr).min() > 0 and np.abs(xr).max() <= ROT_ONES * post / 64
    sud = _cuda(su)
    for qstr, ms in (("tcq_4_none_0.9", (512, 256)), ("tcomb_6_7_0.5_none_0.9", (512,)), ("ldlq_2_8_none_1.0", (256, 256, 128))):
        infos = [gx.exact_info(k, m, qstr, seed=60 + i, codebook_seed=9) for i, m in enumerate(ms)]
        mods = _layers(qp, [qstr] * len(ms), infos)
        assert qp.linear.rotation_fusable(mods, 1)
        wants = [gx.expected(gx.oracle_weight(info), xr.astype(np.float16)) for info in infos]
        for xin in (_cuda(x), _cuda(x.astype(np.float32))):
            _exact(_twice(lambda: qp.multi_gemv(mods, xin, x_rot=(sud, post))), wants, f"{qstr} rotation post {post} {xin.dtype}")


# ----------------------------------------------------------------------------------------- SIMT family
@gpu
@pytest.mark.parametrize("vec,bits,m,k", SIMT_SHAPES)
def test_simt_gemv_geometries(qp, vec, bits, m, k):
    """Every launch geometry of the SIMT GEMV (test_gpu_parity.py's shapes; m = 8199: odd, no multiple of 32): fp32 accumulation,
    one rounding: the fp16 output equals float16 of the exact sum."""
    import torch
    rng = np.random.default_rng(bits * 7 + vec + m)
    idx = rng.integers(0, 1 << bits, size=(m, k // vec), dtype=np.int64)
    lut = gx.grid_codebook((1 << bits, vec), seed=bits + vec)
    ti = torch.from_numpy(idx)
    q = qp.packers.pack_qweight_sq_simt(ti, bits) if vec == 1 else qp.packers.pack_qweight_vq_simt(ti, bits, vec)
    W = lut[idx].reshape(m, k)
    qd, ld = q.cuda(), _cuda(lut)
    for n in (1, 2):
        x = _x(n, k, seed=m + n)
        xd = _cuda(x.reshape(n, 1, k))
        if vec == 1:
            call = lambda: qp.ops.get_op("sq_pack_gemm_simt")(xd, qd, ld, bits)
        else:
            call = lambda: qp.ops.get_op(f"vq_pack_gemm_simt_{n}_{vec}_{bits}")(xd, qd, ld)
        runs = _twice(call)
        assert runs[0][0].dtype == np.float16
        _exact(runs, [gx.expected(W, x, fp16_out=True)], f"simt vec {vec} bits {bits} m {m} k {k} n {n}")


@gpu
@pytest.mark.parametrize("qstr", ["ldlq_2_8_none_1.0", "ldlq_1_4_none_1.0"])
def test_few_row_layer_answers_from_its_simt_twin(qp, qstr):
    k, m = 4096, 1024
    info = gx.exact_info(k, m, qstr, seed=7)
    W = gx.oracle_weight(info)
    layer = qp.make_linear_from_info(qstr, info).cuda()
    for n in (1, 2, 8):
        x = _x(n, k, seed=n)
        xd = _cuda(x)
        runs = _twice(lambda: layer._gemv(xd, n))
        assert runs[0][0].dtype == np.float16 and getattr(layer, "_simt_qweight", None) is not None   # the twin answered
        _exact(runs, [gx.expected(W, x, fp16_out=True)], f"{qstr} twin n {n}")
    x = _x(3, k, seed=3)   # and the module's forward: fp32 in -> the same value in fp32
    y = layer(_cuda(x).float())
    assert gx.same(_np(y), gx.expected(W, x, fp16_out=True).astype(np.float32))
