"""Float64 rules, bounds derived from the number formats, fp32 emulations and seeded defects for the four launches of
csrc/block_glue.hip: qpal_qkv_prep, qpal_norm_add, qpal_glu_gelu_tanh, qpal_logit_cap.  numpy only; shares no code with
qpalette_amd/blocks.py.  test_block_glue.py runs the CPU part (the emulations stay inside half the bounds, every seeded defect lands
outside them) and holds the kernels to the rules on the GPU.

A `mutate=name` argument seeds ONE defect into a float64 rule; the CPU self-test alone uses it.

The bounds (u = 2^-24, the unit roundoff of fp32; nothing here is fitted to a kernel's output):
  norm      a sum of n positive fp32 terms in ANY order is within (n - 1) u of the exact sum of its terms, and every term, a square,
            carries one rounding: n u on the sum of squares, half of that on its inverse root.  The mean, the + eps, the root and
            the reciprocal get glue_reference.INV_REL = 2^-20.  Then one rounding per product, (x inv) w: 2 u.
            With a bias in front, x + b rounds once (u on the element itself, and at most u more through the sum of squares).
                NORM_REL(n) = n u / 2 + 2^-20 + 4 u            relative to |result|
            norm_add adds the rounding of the final sum h + z, the one term that can fill its bound by itself (a correctly rounded
            sum is off by up to u): it is counted as a whole ulp, + 2 u (|h| + |z|), so that a correctly rounded evaluation keeps
            to HALF the bound, which the CPU test asserts of three emulations.
  tanh      DESIGN.md §32.2: the clamped exp / rcp form is within 4 u of tanh (4 u cap on cap tanh).  Its ARGUMENT is computed in
            fp32 too; an argument t with relative error r moves tanh by at most |t| sech^2(t) r <= 0.448 r.
              logit_cap: t = l * fl(1 / cap), two roundings: 0.9 u, counted as u.  |got - ref| <= 5 u cap + u |ref|.
              GELU:      t = c0 (g + c1 g^3): five roundings and the two literals' own (half a unit each): 6 u, 0.448 * 6 = 2.7 u.
                         TANH_ABS = 4 u + 2.7 u, rounded up to 7 u.  gelu = (0.5 g) (1 + tanh): 0.5 |g| TANH_ABS absolute, plus the
                         roundings of 1 + tanh, of the product and of the product with up: 3 u relative.
                         |got - ref| <= |up| 0.5 |g| 7 u + 3 u |ref|."""
import numpy as np

U = 2.0 ** -24
INV_REL = 2.0 ** -20          # glue_reference.INV_REL, restated (a CPU test compares them)
TANH_FORM_ABS = 4.0 * U
GELU_TANH_ABS = 7.0 * U
GELU_C0, GELU_C1 = 0.7978845608, 0.044715
QKV_DEFECTS = ("bias_q_only", "bias_behind_norm", "q_weight_on_k", "norm_whole_row", "v_normed", "no_eps")
NORM_ADD_DEFECTS = ("norm_of_sum", "no_eps")
GLU_DEFECTS = ("silu", "up_gate_swapped")
CAP_DEFECTS = ("tanh_times_cap",)


def norm_rel(n):
    return n * U / 2.0 + INV_REL + 4.0 * U


# ------------------------------------------------------------------------------------------------------------------------ the rules
def _head_norm(x, heads, hd, w, eps, whole_row=False):
    x = x.reshape(x.shape[0], heads, hd)
    ms = (x * x).mean((-1, -2) if whole_row else -1, keepdims=True)
    with np.errstate(invalid="ignore"):   # (the seeded defect without eps turns a head of zeros into NaN)
        return (x / np.sqrt(ms + eps) * w).reshape(x.shape[0], heads * hd)


def qkv_prep_rule(q, k, v, nq, nkv, hd, bias=None, qw=None, kw=None, eps=0.0, mutate=None):
    """-> (q, k, v) float64: x + b on q, k, v (bias in q | k | v order), then per-head RMSNorm * w on q and k"""
    q, k, v = (np.array(t, dtype=np.float64) for t in (q, k, v))
    assert mutate is None or mutate in QKV_DEFECTS
    b = None if bias is None else np.asarray(bias, dtype=np.float64)
    bq, bk, bv = (None, None, None) if b is None else (b[:nq * hd], b[nq * hd:(nq + nkv) * hd], b[(nq + nkv) * hd:])

    def add_bias(q, k, v):
        if b is None:
            return q, k, v
        return (q + bq, k, v) if mutate == "bias_q_only" else (q + bq, k + bk, v + bv)

    if mutate != "bias_behind_norm":
        q, k, v = add_bias(q, k, v)
    if qw is not None:
        qw, kw = np.asarray(qw, dtype=np.float64), np.asarray(kw, dtype=np.float64)
        e = 0.0 if mutate == "no_eps" else eps
        whole = mutate == "norm_whole_row"
        q = _head_norm(q, nq, hd, qw, e, whole)
        k = _head_norm(k, nkv, hd, qw if mutate == "q_weight_on_k" else kw, e, whole)
        if mutate == "v_normed":
            v = _head_norm(v, nkv, hd, kw, e)
    if mutate == "bias_behind_norm":
        q, k, v = add_bias(q, k, v)
    return q, k, v


def norm_add_rule(h, y, w, eps, mutate=None):
    h, y, w = (np.asarray(t, dtype=np.float64) for t in (h, y, w))
    assert mutate is None or mutate in NORM_ADD_DEFECTS
    e = 0.0 if mutate == "no_eps" else eps
    if mutate == "norm_of_sum":      # the post-norm applied after the add
        s = h + y
        return s / np.sqrt((s * s).mean(-1, keepdims=True) + e) * w
    return h + y / np.sqrt((y * y).mean(-1, keepdims=True) + e) * w


def gelu_tanh(g):
    g = np.asarray(g, dtype=np.float64)
    return 0.5 * g * (1.0 + np.tanh(GELU_C0 * (g + GELU_C1 * g * g * g)))


def glu_rule(ug, mutate=None):
    """up | gate rows [rows, 2 inter] -> gelu_tanh(gate) * up"""
    ug = np.asarray(ug, dtype=np.float64)
    assert mutate is None or mutate in GLU_DEFECTS
    inter = ug.shape[-1] // 2
    u, g = ug[..., :inter], ug[..., inter:]
    if mutate == "up_gate_swapped":
        u, g = g, u
    if mutate == "silu":
        return g / (1.0 + np.exp(-g)) * u
    return gelu_tanh(g) * u


def cap_rule(l, cap, mutate=None):
    l = np.asarray(l, dtype=np.float64)
    assert mutate is None or mutate in CAP_DEFECTS
    return np.tanh(l) * cap if mutate == "tanh_times_cap" else cap * np.tanh(l / cap)


# ----------------------------------------------------------------------------------------------------------------------- the bounds
def qkv_norm_tol(ref, hd):
    return norm_rel(hd) * np.abs(ref)


def norm_add_tol(h, y, w, eps):
    h, y, w = (np.asarray(t, dtype=np.float64) for t in (h, y, w))
    z = y / np.sqrt((y * y).mean(-1, keepdims=True) + eps) * w
    return norm_rel(y.shape[-1]) * np.abs(z) + 2.0 * U * (np.abs(h) + np.abs(z))


def glu_tol(ug):
    ug = np.asarray(ug, dtype=np.float64)
    inter = ug.shape[-1] // 2
    u, g = ug[..., :inter], ug[..., inter:]
    return np.abs(u) * 0.5 * np.abs(g) * GELU_TANH_ABS + 3.0 * U * np.abs(gelu_tanh(g) * u)


def cap_tol(l, cap):
    return (TANH_FORM_ABS + U) * cap + U * np.abs(cap_rule(l, cap))


# ------------------------------------------------------------------------------------------------------------------- fp32 emulations
ORDERS = ("sequential", "reversed", "pairwise")
F = np.float32


def sum32(a, order):
    """the fp32 sum of the last axis of fp32 terms in one of three orders"""
    a = np.asarray(a, dtype=F)
    if order == "sequential":
        return np.cumsum(a, axis=-1, dtype=F)[..., -1]
    if order == "reversed":
        return np.cumsum(a[..., ::-1], axis=-1, dtype=F)[..., -1]
    while a.shape[-1] > 1:
        if a.shape[-1] % 2:
            a = np.concatenate((a, np.zeros(a.shape[:-1] + (1,), F)), axis=-1)
        a = (a[..., 0::2] + a[..., 1::2]).astype(F)
    return a[..., 0]


def _inv32(ss, n, eps):
    return (F(1.0) / np.sqrt((ss / F(n)).astype(F) + F(eps), dtype=F)).astype(F)


def emulate_qkv_prep(q, k, v, nq, nkv, hd, bias, qw, kw, eps, order):
    q, k, v = (np.array(t, dtype=F) for t in (q, k, v))
    if bias is not None:
        b = np.asarray(bias, dtype=F)
        q, k, v = q + b[:nq * hd], k + b[nq * hd:(nq + nkv) * hd], v + b[(nq + nkv) * hd:]
    if qw is not None:
        def norm(x, heads, w):
            x = x.reshape(x.shape[0], heads, hd)
            inv = _inv32(sum32((x * x).astype(F), order), hd, eps)[..., None]
            return ((x * inv).astype(F) * np.asarray(w, dtype=F)).astype(F).reshape(x.shape[0], heads * hd)
        q, k = norm(q, nq, qw), norm(k, nkv, kw)
    return q, k, v


def emulate_norm_add(h, y, w, eps, order):
    h, y, w = (np.asarray(t, dtype=F) for t in (h, y, w))
    inv = _inv32(sum32((y * y).astype(F), order), y.shape[-1], eps)[..., None]
    return (h + ((y * inv).astype(F) * w).astype(F)).astype(F)


def tanh32(x, form):
    """three fp32 statements of tanh: the clamped exp / rcp form of the kernels, the expm1 form, and numpy's own fp32 tanh"""
    x = np.asarray(x, dtype=F)
    if form == "exp_rcp":
        x = np.clip(x, F(-15.0), F(15.0))
        return (F(1.0) - F(2.0) * (F(1.0) / (np.exp(F(2.0) * x, dtype=F) + F(1.0)).astype(F)).astype(F)).astype(F)
    if form == "expm1":
        x = np.clip(x, F(-15.0), F(15.0))
        e = np.expm1(F(2.0) * x, dtype=F)
        return (e / (e + F(2.0)).astype(F)).astype(F)
    return np.tanh(x, dtype=F)


TANH_FORMS = ("exp_rcp", "expm1", "numpy")


def emulate_glu(ug, form):
    ug = np.asarray(ug, dtype=F)
    inter = ug.shape[-1] // 2
    u, g = ug[..., :inter], ug[..., inter:]
    t = (F(GELU_C0) * (g + (F(GELU_C1) * ((g * g).astype(F) * g).astype(F)).astype(F)).astype(F)).astype(F)
    return (((F(0.5) * g).astype(F) * (F(1.0) + tanh32(t, form)).astype(F)).astype(F) * u).astype(F)


def emulate_cap(l, cap, form):
    l = np.asarray(l, dtype=F)
    inv = F(1.0) / F(cap)
    return (F(cap) * tanh32((l * inv).astype(F), form)).astype(F)


# ------------------------------------------------------------------------------------------------------------------ the test inputs
def qkv_case(seed, hd, nq, nkv, rows, pad=24):
    """One fp32 buffer [rows, ld] holding q | v | k (the order merge_qv leaves) with `pad` foreign columns in front, between and
    behind; rows cycle through RMS 1, 1e-4, 1e3; head 1 of q (and head 0 of k) of row 0 is all zero.  -> dict with buf, the column
    offsets, bias, qw, kw, eps.  The bias is of the projections' own scale per row family 1."""
    rng = np.random.default_rng(seed)
    wq, wkv = nq * hd, nkv * hd
    ld = wq + 2 * wkv + 4 * pad
    off = {"q": pad, "v": 2 * pad + wq, "k": 3 * pad + wq + wkv}
    buf = rng.standard_normal((rows, ld))
    scale = np.array([1.0, 1e-4, 1e3])[np.arange(rows) % 3][:, None]
    buf = buf * scale
    buf[0, off["q"] + hd: off["q"] + 2 * hd] = 0.0   # (every shape of the tests has nq >= 2)
    buf[0, off["k"]: off["k"] + hd] = 0.0
    return dict(buf=buf.astype(F), off=off, wq=wq, wkv=wkv, ld=ld,
                bias=rng.standard_normal(wq + 2 * wkv).astype(F),
                qw=(1.0 + 0.3 * rng.standard_normal(hd)).astype(F), kw=(1.0 + 0.3 * rng.standard_normal(hd)).astype(F), eps=1e-6)


def qkv_views(case, buf=None):
    buf = case["buf"] if buf is None else buf
    o = case["off"]
    return buf[:, o["q"]:o["q"] + case["wq"]], buf[:, o["k"]:o["k"] + case["wkv"]], buf[:, o["v"]:o["v"] + case["wkv"]]


def norm_add_case(seed, n, rows):
    rng = np.random.default_rng(seed)
    scale = np.array([1.0, 1e-4, 1e3])[np.arange(rows) % 3][:, None]
    return dict(h=rng.standard_normal((rows, n)).astype(F), y=(rng.standard_normal((rows, n)) * scale).astype(F),
                w=(1.0 + 0.3 * rng.standard_normal(n)).astype(F), eps=1e-6)


def glu_case(seed, inter, rows):
    """up | gate rows; the gate covers +-30 densely around 0 and sparsely outside, with the exact values 0, +-30 present"""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((rows, inter)) * 3.0
    far = rng.random((rows, inter)) < 0.1
    g = np.where(far, rng.uniform(-30.0, 30.0, (rows, inter)), g)
    g[0, :3] = (0.0, 30.0, -30.0)
    return np.concatenate((rng.standard_normal((rows, inter)), g), axis=1).astype(F)


def cap_case(seed, vocab, rows, cap):
    """logits over +-10 cap: a normal bulk of sd cap / 2 and a uniform tail, the ends and 0 present"""
    rng = np.random.default_rng(seed)
    l = rng.standard_normal((rows, vocab)) * (cap / 2.0)
    far = rng.random((rows, vocab)) < 0.1
    l = np.where(far, rng.uniform(-10.0 * cap, 10.0 * cap, (rows, vocab)), l)
    l[0, :3] = (0.0, 10.0 * cap, -10.0 * cap)
    return l.astype(F)
