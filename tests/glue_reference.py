"""Float64 rules, bounds derived from the number formats, CPU emulations and seeded defects for the launches around every projection
of a decode step: the RMSNorm fused into the GEMV staging and into the rotation launch, the final norm + lm_head in
both forms, the SwiGLU epilogue and the residual add.  numpy only; test_glue_exact.py runs the CPU part (the checks have teeth, kappa
comes from the emulation) and holds the kernels to the rules on the GPU.

A `mutate=(name, argument...)` argument seeds ONE defect into a float64 rule; the CPU self-test alone uses it."""
import numpy as np

from oracle.incoherent import f16, left_input, silu, wht

GEMV_RTOL_ABS = 1e-5      # the project's GEMV bar: |y - sum w x| <= 1e-5 * sum |w x| (fp32 accumulation of fp16 products)
INV_REL = 2.0 ** -20      # relative slack of the fp32 1/rms (and of the fp32 product in front of the rounding): DESIGN.md §25.2
SILU_REL = 2.0 ** -20     # relative slack of the fp32 silu in front of its fp16 rounding (§25.4)
RMS_PRE = 2.0 ** -6       # the staging's power-of-two guard scale (csrc/tc_kernels.h kRmsPre, csrc/hadamard.hip)
KAPPA = {False: 8.0, True: 16.0}   # staging bound, keyed by K > 1: twice the worst emulated ratio, rounded up to a power of two
                                   # (§25.3 table; a CPU test derives it again and compares)
RMS_SUPPORTED = 2.0 ** -8  # rows with rms >= this must meet the staging bound; smaller ones are range checks (§25.3)


def ulp16(v):
    """Spacing of fp16 at |v| (2^-24 in the subnormal range and at 0)."""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float16)).astype(np.float64)


def rms_inv(h, eps, mutate=None):
    """(mean(h^2) + eps)^-1/2 per row in float64; eps <= 0: no norm (1)."""
    h = np.asarray(h, dtype=np.float64)
    if not eps > 0:
        return np.ones(h.shape[:-1] + (1,))
    kind = mutate[0] if mutate else None
    k = h.shape[-1]
    ms = (h * h).mean(-1, keepdims=True)
    if kind == "half_rms":      # the sum of squares of half the row, divided by the whole width
        ms = (h[..., : k // 2] ** 2).sum(-1, keepdims=True) / k
    inv = 1.0 / np.sqrt(ms + (0.0 if kind == "no_eps" else eps))
    if kind == "inv_row0":      # every row scaled by row 0's 1/rms
        inv = np.broadcast_to(inv[:1], inv.shape).copy()
    return inv


def _weight(w, k, mutate=None):
    if w is None or (mutate and mutate[0] == "no_weight"):
        return np.ones(k)
    return np.asarray(w, dtype=np.float64)


def norm_two_roundings(h, w, eps, inv_scale=1.0, mutate=None):
    """f16(f16(h * inv) * w): the reference's LlamaRMSNorm (model/llama.py:129-135, `weight * hidden.to(fp16)`) and the rule of both
    lm_head kernels.  inv_scale perturbs inv (the accepted interval of the staged x)."""
    h = np.asarray(h, dtype=np.float64)
    inv = rms_inv(h, eps, mutate) * inv_scale
    return f16(f16(h * inv) * _weight(w, h.shape[-1], mutate))


def norm_one_rounding(h, w, eps):
    """f16(h * inv * w): what the fused per-layer norm (x_rms, qpal_hadamard_rms) aims at."""
    h = np.asarray(h, dtype=np.float64)
    return f16(h * rms_inv(h, eps) * _weight(w, h.shape[-1]))


# ------------------------------------------------------------------------------------------------------------ final norm + lm_head
def staged_x_interval(h, w, eps):
    """(lo, hi, exact): the staged x of the lm_head kernels is accepted iff lo <= x <= hi, ends included: the two-rounding rule at
    inv (1 -+ 2^-20), and the same rule at the exact inv.  Both roundings are monotone, so every fp32 inv within 2^-20 of the exact
    one — and the fp32 rounding of h * inv in front of the fp16 one — lands inside."""
    a, b = norm_two_roundings(h, w, eps, 1.0 - INV_REL), norm_two_roundings(h, w, eps, 1.0 + INV_REL)
    return np.minimum(a, b), np.maximum(a, b), norm_two_roundings(h, w, eps)


def lm_head_rule(h, w, eps, W, mutate=None):
    """-> (x [rows, k], logits [rows, vocab]) in float64: x by the two-rounding rule, logits = x W^T.  Defects: ("drop_col", j) the
    product of column j lost; ("swap_stages", a, b) the x of 256-column stages a and b exchanged under the weights; ("inv_row0",),
    ("no_weight",), ("no_eps",) in the norm."""
    x = norm_two_roundings(h, w, eps, mutate=mutate)
    xm = x
    kind = mutate[0] if mutate else None
    if kind == "drop_col":
        xm = x.copy()
        xm[:, mutate[1]] = 0.0
    elif kind == "swap_stages":
        a, b = mutate[1], mutate[2]
        xm = x.copy()
        xm[:, 256 * a: 256 * a + 256], xm[:, 256 * b: 256 * b + 256] = x[:, 256 * b: 256 * b + 256], x[:, 256 * a: 256 * a + 256]
    return x, xm @ np.asarray(W, dtype=np.float64).T


def logits_bound(x, W):
    """(sum w x, 1e-5 * sum |w x|) in float64 for the kernel's own staged x."""
    Wd, xd = np.asarray(W, dtype=np.float64), np.asarray(x, dtype=np.float64)
    return xd @ Wd.T, GEMV_RTOL_ABS * (np.abs(xd) @ np.abs(Wd).T)


def interval_excess(got, lo, hi, exact):
    """How far outside [lo, hi] in units of the tier's own width max(hi - lo, one fp16 ulp of the rule): 0 inside."""
    got = np.asarray(got, dtype=np.float64)
    return np.maximum(np.maximum(lo - got, got - hi), 0.0) / np.maximum(hi - lo, ulp16(exact))


LM_HEAD_FAMILIES = ("sigma 1", "outlier", "sigma 2^-10", "sigma 2^10", "outlier 2^10", "zero", "mean << eps", "one-hot", "sigma 1 again")


def lm_head_rows(rng, k, rows):
    """The input rows of one lm_head launch, row i of family i % 9 -> h float32 [rows, k]."""
    h = np.zeros((rows, k))
    for i in range(rows):
        fam = LM_HEAD_FAMILIES[i % len(LM_HEAD_FAMILIES)]
        g = rng.standard_normal(k)
        if fam.startswith("sigma 1"):
            h[i] = g
        elif fam == "sigma 2^-10":
            h[i] = g * 2.0 ** -10
        elif fam == "sigma 2^10":
            h[i] = g * 2.0 ** 10
        elif fam.startswith("outlier"):
            s = 2.0 ** 10 if fam.endswith("2^10") else 1.0
            h[i] = g * s
            h[i, rng.integers(k)] = 400.0 * s            # an outlier channel
        elif fam == "mean << eps":
            h[i] = g * 1e-4                              # mean(h^2) = 1e-8
        elif fam == "one-hot":
            h[i, rng.integers(k)] = 3.0
    return h.astype(np.float32)


# ------------------------------------------------------------------------------------------------- RMSNorm + rotation (the staging)
def _rotate(a, hadk, mid=None):
    """(hadK (x) H_P) a / sqrt(k) of every row, a as [K][P]; mid(t) is applied between the factors where K > 1."""
    k = a.shape[-1]
    K = 1 if hadk is None else hadk.shape[0]
    t = wht(a.reshape(a.shape[0], K, k // K)) * float(k) ** -0.5
    if K > 1:
        if mid is not None:
            t = mid(t)
        t = np.einsum("ji,ric->rjc", np.asarray(hadk, dtype=np.float64), t)
    return t.reshape(a.shape)


def staged_rule(x, w, su, eps, post, hadk=None, mutate=None):
    """The kernels' order in float64: a = f16(x w 2^-6) su;  t = H a / sqrt(k) scaled by 64 inv (rounded to fp16 between the factors
    where K > 1);  z = f16(f16(t) post).  Defects: ("zero8", i) inputs i .. i + 7 lost, ("half_rms",), ("su_skip", b) the signs of
    64-block b not applied."""
    x = np.asarray(x, dtype=np.float64)
    k = x.shape[-1]
    kind = mutate[0] if mutate else None
    inv = rms_inv(x, eps, mutate)
    a = f16(x * _weight(w, k) * RMS_PRE)
    s = np.ones(k) if su is None else np.asarray(su, dtype=np.float64).copy()
    if kind == "su_skip":
        s[64 * mutate[1]: 64 * mutate[1] + 64] = 1.0
    a = a * s
    if kind == "zero8":
        a[:, mutate[1]: mutate[1] + 8] = 0.0
    scale = inv[:, :, None] / RMS_PRE if hadk is not None else None
    if hadk is None:
        t = _rotate(a, None) * inv / RMS_PRE
    else:
        t = _rotate(a, hadk, mid=lambda t: f16(t * scale))
    return f16(f16(t) * post)


def staging_target(x, w, su, eps, post, hadk=None):
    """What the fused launches aim at: the reference's pipeline on the one-rounding norm."""
    k = np.asarray(x).shape[-1]
    return left_input(norm_one_rounding(x, w, eps), np.ones(k) if su is None else su, hadk, 1.0 / post)


def kappa(hadk):
    return KAPPA[hadk is not None]


def staging_terms(x, w, eps, post):
    """(y, spread): y = x inv w and spread = sqrt(sum_i delta_i^2 / k) * post per row, delta_i = max(2^-11 |y_i|, 2^-25 * 64 * inv):
    the first rounding, a half ulp relative — or, in the fp16 subnormal range of x w 2^-6, half its fixed step 2^-24 brought back to
    the scale of y — spread over the k inputs of every output by the orthogonal transform."""
    x = np.asarray(x, dtype=np.float64)
    k = x.shape[-1]
    inv = rms_inv(x, eps)
    y = x * inv * _weight(w, k)
    delta = np.maximum(2.0 ** -11 * np.abs(y), 2.0 ** -25 * inv / RMS_PRE)
    return y, np.sqrt((delta * delta).sum(-1, keepdims=True) / k) * post


def staging_ratio(got, x, w, su, eps, post, hadk=None):
    """(|got - target| - ulp16(target)) / spread per element: the kernels must stay below kappa(K)."""
    ref = staging_target(x, w, su, eps, post, hadk)
    _, spread = staging_terms(x, w, eps, post)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (np.abs(np.asarray(got, dtype=np.float64) - ref) - ulp16(ref)) / spread
    return np.where(spread > 0, r, np.where(np.abs(got - ref) <= ulp16(ref), 0.0, np.inf))


def emulate_staging(x, w, su, eps, post, hadk=None, src_f16=False, hilo=True, flush=False):
    """The staging with every rounding point restated from the number formats (not from the kernels' output): fp32 sum of squares,
    fp32 1/rms, fp32 product then fp16 on the way in, an exact transform (fp16 inputs, fp32 accumulators: exact below 2^24 steps of
    the smallest input; what is not is covered by kappa's factor 2), the matrix pipe's fp16 hi + lo split of the 64-point stage
    (hilo), fp32 scaling, two fp16 roundings on the way out.  flush: fp16 subnormal inputs of the matrix pipe read as zero (the
    behaviour the GPU part measures; never part of kappa)."""
    x = np.asarray(x, dtype=np.float32)
    if src_f16:
        x = x.astype(np.float16).astype(np.float32)
    k = x.shape[-1]
    wv = np.ones(k, np.float32) if w is None else np.asarray(w, dtype=np.float16).astype(np.float32)
    ss = (x * x).sum(-1, keepdims=True, dtype=np.float32)
    inv = (np.float32(1.0) / np.sqrt(ss / np.float32(k) + np.float32(eps))).astype(np.float32)
    a = ((x * np.float32(RMS_PRE)) * wv).astype(np.float16)

    def fl(v16):
        return np.where(np.abs(v16.astype(np.float64)) < 2.0 ** -14, 0.0, v16.astype(np.float64)) if flush else v16.astype(np.float64)

    a = fl(a) * (1.0 if su is None else np.asarray(su, dtype=np.float64))
    K = 1 if hadk is None else hadk.shape[0]
    P = k // K
    t = a.reshape(x.shape[0], K, P)
    if hilo and P % 64 == 0:
        d1 = wht(t.reshape(x.shape[0], K, P // 64, 64)) * 0.125          # [R][64] view: the 64-point factor first
        hi = d1.astype(np.float32).astype(np.float16)
        lo = (d1.astype(np.float32) - hi.astype(np.float32)).astype(np.float16)
        d1 = (fl(hi) + fl(lo)) * 8.0
        t = np.swapaxes(wht(np.swapaxes(d1, -1, -2)), -1, -2).reshape(x.shape[0], K, P)
    else:
        t = wht(t)
    pre = np.float32(float(k) ** -0.5)
    mul = (inv * np.float32(1.0 / RMS_PRE)).astype(np.float32)
    if K > 1:
        mid = (t.astype(np.float32) * (pre * mul)[:, :, None]).astype(np.float16)
        t = np.einsum("ji,ric->rjc", np.asarray(hadk, dtype=np.float64), fl(mid)).astype(np.float32).reshape(x.shape)
    else:
        t = ((t.reshape(x.shape).astype(np.float32) * pre).astype(np.float32) * mul).astype(np.float32)
    z = t.astype(np.float16).astype(np.float32) * np.float32(post)
    return z.astype(np.float16).astype(np.float64)


STAGING_SIGMAS = tuple(2.0 ** e for e in (0, -4, 4, -8, 8, -12, 12))


def staging_families():
    fams = []
    for s in STAGING_SIGMAS:
        fams += [("sigma", s), ("outlier", s)]
    return fams + [("constant", 0.75), ("constant", -3.0 * 2.0 ** -7), ("one-hot", 2.5)]


def staging_rows(rng, k, rows=None):
    """The families of §25.3, row i of family i % 17 (rows None: each once) -> (x float32 [rows, k], names, hot): hot[i] is the index
    of a one-hot row's element, -1 elsewhere."""
    fams = staging_families()
    rows = len(fams) if rows is None else rows
    x, names, hot = np.zeros((rows, k)), [], np.full(rows, -1)
    for i in range(rows):
        kind, s = fams[i % len(fams)]
        names.append(f"{kind} {s:g}")
        if kind == "constant":
            x[i] = s
        elif kind == "one-hot":
            hot[i] = int(rng.integers(k))
            x[i, hot[i]] = s
        else:
            x[i] = rng.standard_normal(k) * s
            if kind == "outlier":
                x[i, rng.integers(k)] = 400.0 * s
    return x.astype(np.float32), names, hot


def one_hot_target(k, hot, amp, w, su, eps, post):
    """Analytic: y = e_hot * amp inv w_hot, the transform spreads +-|y| / sqrt(k) over every output."""
    inv = 1.0 / np.sqrt(amp * amp / k + eps)
    y = float(f16(amp * inv * (1.0 if w is None else float(w[hot])))) * (1.0 if su is None else float(su[hot]))
    signs = np.array([1.0 - 2.0 * (bin(i & hot).count("1") & 1) for i in range(k)])
    return f16(f16(signs * y * float(k) ** -0.5) * post)


# ------------------------------------------------------------------------------------------------------------------ SwiGLU epilogue
def swiglu_candidates(u, g, mutate=None):
    """The accepted set of one act_out element as [3, ...]: f16(s * f16(u)) for s in f16(silu64(g') (1 + {-1, 0, 1} 2^-20)), g' =
    f16(g).  Defects: ("silu_up",) silu(u) * g; ("no_gate_factor",) sigmoid(g) * u."""
    u16, g16 = f16(u), f16(g)
    kind = mutate[0] if mutate else None
    if kind == "silu_up":
        u16, g16 = g16, u16
    s = silu(g16)
    if kind == "no_gate_factor":
        s = 1.0 / (1.0 + np.exp(-g16))
    return np.stack([f16(f16(s * (1.0 + d * SILU_REL)) * u16) for d in (-1.0, 0.0, 1.0)])


def swiglu_member(act, u, g):
    c = swiglu_candidates(u, g)
    return (np.asarray(act, dtype=np.float64)[None] == c).any(0)


def swiglu_bound(u, g, du, dg):
    """(ref, tol) for a real up | gate layer: ref = silu(g) u in float64 on the fp32 projections of the plain launch, du / dg their
    GEMV bar (1e-5 osc |x'| @ |W|^T).  Terms: the two fp16 roundings of the product and of silu (1.5 * 2^-10 |ref| covers the product's
    half ulp and the propagated half ulp of f16(u)), the subnormal step, the rounding of f16(g) through silu (|silu'| <= 1.1), and
    the summation-order slack of both projections.  No max|ref| term."""
    u, g = np.asarray(u, dtype=np.float64), np.asarray(g, dtype=np.float64)
    s = silu(g)
    ref = s * u
    tol = 1.5 * 2.0 ** -10 * np.abs(ref) + 2.0 ** -24 + 2.0 ** -10 * np.abs(s * u) + 1.1 * np.abs(u) * dg + np.abs(s) * du
    return ref, tol


# --------------------------------------------------------------------------------------------------------------------- residual add
def accumulate_rule(h, y, mutate=None):
    """fl32(h + y); ("overwrite",): y alone."""
    if mutate and mutate[0] == "overwrite":
        return np.asarray(y, dtype=np.float32)
    return (np.asarray(h, dtype=np.float32) + np.asarray(y, dtype=np.float32)).astype(np.float32)


def accumulate_split_tol(h, y, delta):
    """Split K: partial sums arrive as atomics onto the live output, each add rounds at the magnitude of |h| + |y|."""
    return 2.0 ** -22 * (np.abs(np.asarray(h, dtype=np.float64)) + np.abs(np.asarray(y, dtype=np.float64))) + delta
