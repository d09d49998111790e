"""Exactly summable inputs for the fused GEMV / skinny GEMM / SIMT GEMV tests (tests/test_gemv_exact.py, the exact pass of
tests/test_gemv_row_finish.py).  No GPU in this module.

The codebook is an input tensor and everything behind the gather is fp16 x fp16 -> fp32.  With every codebook value on a dyadic
grid, every x a small integer and every partial sum inside an fp32 significand, no addition ever rounds: MFMA chains, the LDS row
finish, fp32 atomics between workgroups and the `+=` of the accumulate path give the same bits in every order, and a kernel's
output must EQUAL the float64 reference — one wrong weight, one lost term, one stale x element changes it.

GRID: the fp16 multiples of 2^-5 in [-4, 4): 256 values; the negation the TCQ decode applies to a codebook value stays on the
grid's lattice and within |w| <= 4 (-(-4) = 4 is the one value outside the list; the budget counts it).

Bit budget: sum_k |w_k x_k| <= k * wmax * xmax, in units of grid (the spacing of the products): bit_budget() <= 2^22 is asserted by
every case before it launches anything.  fp32 holds 2^24: two bits stay spare for however the f16 matrix instruction aligns the
products of one instruction before it adds them (not measured in this project).  amax_for(k) is the largest |x| that keeps a plain
GEMV inside: 3 up to k = 8192, 2 up to 16384, 1 above (28672 * 4 * 1 * 32 = 3.67e6 <= 2^22 = 4.19e6)."""
import numpy as np

GRID_STEP = 2.0 ** -5
GRID = (np.arange(-128, 128, dtype=np.float64) * GRID_STEP).astype(np.float16)
WMAX = 4.0
BUDGET_MAX = 2 ** 22


def _oracle():
    from oracle import oracle
    return oracle


# ------------------------------------------------------------------------------------------------------------- inputs
def amax_for(k):
    return 3 if k <= 8192 else (2 if k <= 16384 else 1)


def bit_budget(k, wmax=WMAX, xmax=1.0, grid=GRID_STEP, scale_max=1.0, scale_min=1.0, base=0.0):
    """Largest |partial sum| of a case in units of its smallest representable step: k * wmax * xmax / grid for a plain GEMV.
    grid: the spacing of the products w * x (codebook step times the unit of x).  An epilogue out = acc * wscale * oscale (+ base)
    multiplies the sum by up to scale_max, refines the step by scale_min and adds |base| <= base."""
    return (k * wmax * xmax * scale_max + base) / (grid * scale_min)


def assert_budget(k, **kw):
    b = bit_budget(k, **kw)
    assert b <= BUDGET_MAX, (k, kw, b)
    return b


def grid_codebook(shape, seed):
    """fp16 codebook drawn uniformly (with replacement) from GRID.  Two distinct ENTRIES hold the same value with probability 1/256 —
    chance, no more: that is the probability that a gather of the wrong entry goes unseen, per weight; a wrong gather that touches
    t weights of an output row goes unseen with 256^-t."""
    rng = np.random.default_rng(seed)
    return GRID[rng.integers(0, GRID.size, size=shape)]


def exact_info(k, m, qstr, seed, codebook_seed=None, tlut_bits=None, part=None):
    """qpalette_amd.mem_op.dummy_linear_info (full-range random trellis / codes, CPU tensors) with its codebook (`tlut` / `lut`)
    redrawn from GRID.  codebook_seed: the same codebook in every layer that passes the same value (share_codebooks);
    tlut_bits: a codebook size other than the quantizer string's own (the (S, KV) table of the kernels is wider)."""
    import torch
    from qpalette_amd import mem_op
    info = mem_op.dummy_linear_info(k, m, qstr, seed=seed, device="cpu", part=part)
    name = "tlut" if "tlut" in info else "lut"
    shape = tuple(info[name].shape)
    if tlut_bits is not None:
        assert name == "tlut"
        info["tlut_bits"] = tlut_bits
        shape = (2 ** tlut_bits, 2)
    cb = grid_codebook(shape, 7919 * (seed + 1) + 1 if codebook_seed is None else 104729 * (codebook_seed + 1))
    info[name] = torch.from_numpy(cb.copy())
    return info


def exact_x(n, k, seed, amax=None):
    """fp16 [n, k] of integers in +-1 .. +-amax, no zeros: every column counts in every row."""
    amax = amax_for(k) if amax is None else amax
    rng = np.random.default_rng(seed)
    return (rng.integers(1, amax + 1, size=(n, k)) * (rng.integers(0, 2, size=(n, k)) * 2 - 1)).astype(np.float16)


def exact_base(n, m, seed, bmax=64):
    """fp32 [n, m] of integers in -bmax .. bmax: what the accumulate path adds onto"""
    return np.random.default_rng(seed).integers(-bmax, bmax + 1, size=(n, m)).astype(np.float32)


def oracle_weight(info):
    """fp16 W [m, k] of any linear_info dict, decoded by the CPU oracle"""
    o = _oracle()
    m, k = info["out_features"], info["in_features"]
    if "qweight" in info:
        return o.lut_tc_dequant(info["qweight"].numpy(), info["lut"].numpy(), m, k, info["lut_bits"], info["vec_sz"])
    tl, S = info["tlut"].numpy(), info["tlut_bits"]
    if "trellis" in info:
        return o.tcq_dequant(info["trellis"].numpy(), tl, m, k, S, info["KV"])
    kv1, kv2 = info["KV"]
    if "in_part" in info and tuple(info["in_part"]) != (k // 2, k // 2):
        p = info["in_part"]
        return np.concatenate([o.tcq_dequant(info["trellis1"].numpy(), tl, m, p[0], S, kv1),
                               o.tcq_dequant(info["trellis2"].numpy(), tl, m, p[1], S, kv2)], axis=1)
    return o.tcq_dequant(info["trellis1"].numpy(), tl, m, k, S, kv1, c2=info["trellis2"].numpy(), KV2=kv2,
                         split=2 if "in_part" in info else 1)


# ------------------------------------------------------------------------------------------------------------- the reference
def exact32(ref):
    """float64 -> fp32, asserting that nothing is lost: the reference itself is checked, not only the kernel"""
    r32 = np.asarray(ref, dtype=np.float64).astype(np.float32)
    assert np.array_equal(r32.astype(np.float64), ref), "the float64 reference does not fit fp32: the case is over its budget"
    return r32


def expected(W, x, fp16_out=False, wscale=None, oscale=1.0, base=None):
    """oracle.gemv's float64 sum (times wscale[row] * oscale, plus base), cast to fp32 without loss; fp16_out (SIMT family: fp32
    accumulation, ONE rounding of the result): float16 of it, a single well-defined rounding."""
    ref, mag = _oracle().gemv(np.ascontiguousarray(W, dtype=np.float16), np.ascontiguousarray(x, dtype=np.float16))
    exact32(mag)  # (the sum of magnitudes bounds every partial sum of every order)
    if wscale is not None:
        ref = ref * np.asarray(wscale, dtype=np.float64)[None, :]
    ref = ref * float(oscale)
    if base is not None:
        ref = ref + np.asarray(base, dtype=np.float64)
    r32 = exact32(ref)
    return r32.astype(np.float16) if fp16_out else r32


def same(got, want):
    """Equality by VALUE: -0 equals +0, NaN never matches."""
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def describe_difference(got, want):
    """Where two [n, m] outputs differ: what a failing exact test prints (batch rows, output rows mod 32, the differences in units of
    one grid step), so the pattern can be read off the assertion."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return f"shapes {got.shape} != {want.shape}"
    bad = np.argwhere(~(got == want))
    if not len(bad):
        return "equal"
    d = (got - want)[tuple(bad.T)] / GRID_STEP
    return (f"{len(bad)} of {got.size} differ; batch rows {sorted(set(bad[:, 0].tolist()))[:8]}, output rows {sorted(set(bad[:, 1].tolist()))[:12]}"
            f" (mod 32: {sorted(set((bad[:, 1] % 32).tolist()))[:12]}); differences / 2^-5: {d[:8].tolist()}")


def rotated_x(x, su, post):
    """What x_rot = (su, post) stages at k = 4096 for integer x: H (x * su) / 64 * post, computed in integers (k^-1/2 = 2^-6 and
    post, a power of two, are exact scalings).  float64 [n, k]; exact in fp16 for the sparse x of the rotation cases."""
    from oracle import incoherent as oi
    k = x.shape[-1]
    assert k == 4096
    h = oi.wht(np.asarray(x, dtype=np.float64) * np.asarray(su, dtype=np.float64))
    assert np.array_equal(h, np.rint(h))
    out = h / 64.0 * float(post)
    assert np.array_equal(out.astype(np.float16).astype(np.float64), out)
    return out


# ------------------------------------------------------------------------------------------------------------- seeded defects
DEFECTS = ("neighbour_weight", "dropped_term", "doubled_term", "stale_x", "replica")


def _neighbour(v):
    """the neighbouring grid value (one step up; one step down from the top)"""
    v = np.asarray(v, dtype=np.float64)
    return np.where(v + GRID_STEP < WMAX, v + GRID_STEP, v - GRID_STEP)


def seeded_defect(kind, W, x, seed):
    """(W', x') float64: the oracle's W and x with ONE slip of a kernel seeded into them.
    neighbour_weight: one weight moved to the neighbouring grid value;  dropped_term / doubled_term: one (non-zero) term missing /
    counted twice;  stale_x: one x element replaced by its neighbour's (where they differ);  replica: one codebook value wrong in a
    single replica of a banked codebook image — wrong for the weights whose column index is = r mod 32."""
    rng = np.random.default_rng(seed)
    W, x = np.array(W, dtype=np.float64), np.array(x, dtype=np.float64)
    m, k = W.shape
    if kind == "stale_x":
        b = int(rng.integers(0, x.shape[0]))
        js = np.nonzero(x[b, :-1] != x[b, 1:])[0]
        j = int(js[rng.integers(0, len(js))])
        x[b, j] = x[b, j + 1]
        return W, x
    if kind == "replica":
        r = int(rng.integers(0, 32))
        cols = np.arange(r, k, 32)
        v = W[int(rng.integers(0, m)), int(cols[rng.integers(0, len(cols))])]   # (a value that replica does serve)
        sub = W[:, cols]
        sub[sub == v] = _neighbour(v)
        W[:, cols] = sub
        return W, x
    while True:
        i, j = int(rng.integers(0, m)), int(rng.integers(0, k))
        if W[i, j] != 0.0:
            break
    W[i, j] = {"neighbour_weight": float(_neighbour(W[i, j])), "dropped_term": 0.0, "doubled_term": 2.0 * W[i, j]}[kind]
    return W, x


def shares_under_tolerance(W, x, rtol=1e-5, replicas=256, seed=0):
    """Of every possible seeded defect of each kind (replica: of `replicas` sampled ones), the share whose change of the output
    stays within rtol * sum_k |w_k x_k| on every output it touches, i.e. that a tolerance test of that bar passes.  W, x: what such
    a test runs on (any codebook: the neighbouring value is the next one of W's own sorted values).  One batch row."""
    W, x = np.asarray(W, dtype=np.float64), np.asarray(x, dtype=np.float64).reshape(-1)
    m, k = W.shape
    bar = rtol * (np.abs(W) * np.abs(x)[None, :]).sum(-1)   # [m]
    term = np.abs(W * x[None, :])
    live = W != 0.0
    vals = np.unique(W)
    pos = np.searchsorted(vals, W)
    nb = vals[np.where(pos + 1 < len(vals), pos + 1, pos - 1)]
    out = {"dropped_term": float((term <= bar[:, None])[live].mean()), "doubled_term": float((term <= bar[:, None])[live].mean()),
           "neighbour_weight": float((np.abs((nb - W) * x[None, :]) <= bar[:, None]).mean())}
    dx = np.append(x[1:] - x[:-1], 0.0)
    cand = dx != 0.0
    out["stale_x"] = float((np.abs(W * dx[None, :]) <= bar[:, None]).all(0)[cand].mean())
    rng = np.random.default_rng(seed)
    passed = 0
    for _ in range(replicas):
        r = int(rng.integers(0, 32))
        cols = np.arange(r, k, 32)
        v = W[int(rng.integers(0, m)), int(cols[rng.integers(0, len(cols))])]
        v2 = vals[min(int(np.searchsorted(vals, v)) + 1, len(vals) - 1)] if v != vals[-1] else vals[-2]
        delta = ((W[:, cols] == v) * (v2 - v) * x[None, cols]).sum(-1)
        passed += bool((np.abs(delta) <= bar).all())
    out["replica"] = passed / replicas
    return out
