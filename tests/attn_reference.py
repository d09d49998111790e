"""A float64 attention reference, an error bound derived from the number formats, and input families that make a lost key, a
skipped max subtraction or a wrongly weighted merge visible ("attention parity bound").  Used by test_attn_exact.py;
device-agnostic: the same code runs on the CPU (the self-test of the checks) and on the GPU (parity of the kernels).

Layout everywhere: q16 [R, nq * hd] (the rows after the rotary embedding, fp16), K / V [nkv, L, hd] (ONE sequence's cache, fp16 or
float8_e4m3fn, or fp32 targets a test casts), query head h reads kv head h // (nq // nkv).  Row r attends to keys 0 .. n[r] - 1."""
import functools
import math

import torch

F16, F8 = torch.float16, torch.float8_e4m3fn


def _f64(t):
    return t.float().double()


def _heads(q16, nq, nkv, hd):
    return q16.view(q16.shape[0], nkv, nq // nkv, hd)


def attention_fp64(q16, K, V, n_keys_per_row, nq, nkv, hd, scale, mutate=None):
    """softmax(q k^T * scale) v in float64 over the stored cache values.  Returns (ref, A, Smax): ref and A = sum_j p_j |v_jd| as
    [R, nq * hd], Smax = max_j sum_d |q_d k_jd| * scale as [R, nq].  mutate = (name, argument) seeds one defect into ref (A and
    Smax stay those of the correct computation); the CPU self-test alone uses it:
      ("drop", j) key j lost; ("double", j) key j counted twice; ("causal_lt",) row r stops one key early; ("past_diag",) row r
      admits key n[r]; ("no_max",) fp32 exp without the max subtraction; ("merge_w1", c) chunks of c keys merged with weight 1;
      ("alpha_l_only", t) t-key tiles with a running max, l rescaled by alpha but O not; ("kv_neighbour",) head group g reads kv
      head g + 1."""
    dev, R, rep = q16.device, q16.shape[0], nq // nkv
    n = torch.as_tensor(n_keys_per_row, dtype=torch.long, device=dev).view(R)
    kind = mutate[0] if mutate else None
    arg = mutate[1] if mutate and len(mutate) > 1 else None
    nmax = int(n.max()) + (1 if kind == "past_diag" else 0)
    q = _f64(_heads(q16, nq, nkv, hd))
    Kd, Vd = _f64(K[:, :nmax]), _f64(V[:, :nmax])
    j = torch.arange(nmax, device=dev)

    def scores(Kx):
        return torch.einsum("rgpd,gjd->rgpj", q, Kx) * scale

    def mask(valid):
        return valid[:, None, None, :]

    valid = j[None, :] < n[:, None]
    s = scores(Kd).masked_fill(~mask(valid), float("-inf"))
    p = torch.softmax(s, dim=-1)
    ref = torch.einsum("rgpj,gjd->rgpd", p, Vd).reshape(R, nq * hd)
    A = torch.einsum("rgpj,gjd->rgpd", p, Vd.abs()).reshape(R, nq * hd)
    Smax = (torch.einsum("rgpd,gjd->rgpj", q.abs(), Kd.abs()) * scale).masked_fill(~mask(valid), 0.0).amax(-1).reshape(R, nq)
    if kind is None:
        return ref, A, Smax

    Km, Vm = (Kd.roll(-1, 0), Vd.roll(-1, 0)) if kind == "kv_neighbour" else (Kd, Vd)
    v2 = valid
    if kind == "drop":
        v2 = valid & (j != arg)[None, :]
    elif kind == "causal_lt":
        v2 = j[None, :] < (n - 1)[:, None]
    elif kind == "past_diag":
        v2 = j[None, :] < (n + 1)[:, None]
    sm = scores(Km).masked_fill(~mask(v2), float("-inf"))
    if kind == "double":
        sm[..., arg] += math.log(2.0)
    if kind == "no_max":
        num = den = torch.exp(sm.float())  # fp32, as a kernel would
        Vm = Vm.float()
    elif kind == "merge_w1":
        pad = (-nmax) % arg
        sp = torch.nn.functional.pad(sm, (0, pad), value=float("-inf")).unflatten(-1, (-1, arg))
        w = torch.exp(sp - sp.amax(-1, keepdim=True))  # every chunk relative to its OWN max, then summed as they are
        num = den = torch.nan_to_num(w, nan=0.0).flatten(-2)[..., :nmax]
    elif kind == "alpha_l_only":
        pad = (-nmax) % arg
        sp = torch.nn.functional.pad(sm, (0, pad), value=float("-inf")).unflatten(-1, (-1, arg))
        mrun = torch.cummax(sp.amax(-1), dim=-1).values  # the running max after each tile
        num = torch.exp(sp - mrun[..., None]).flatten(-2)[..., :nmax]  # O keeps every tile at the max it was added under
        den = torch.exp(sm - sm.amax(-1, keepdim=True))
    else:
        num = den = torch.exp(sm - sm.amax(-1, keepdim=True))
    out = torch.einsum("rgpj,gjd->rgpd", num, Vm) / den.sum(-1)[..., None]
    return out.double().reshape(R, nq * hd), A, Smax


# kappa of bound(): four times the worst ratio of emulate() against attention_fp64() over every input family of test_attn_exact.py,
# rounded up to a power of two.  The ratio is |fp32 quotient - ref| / ((u_p + 2^-23 (1 + Smax)) A), taken in front of the output's
# fp16 rounding (that rounding fills the bound's first two terms by itself).  Measured on the CPU, both cache formats, hd 64 /
# 128 / 256, 512 .. 32768 keys (test_emulation_sits_inside_the_bound prints the table):
#
#   family      u_p = 0 (decode)   u_p = 2^-11 (prefill, ragged)
#   base             0.073              0.115
#   peaked           0.918              0.797
#   ramp_up          1.005              0.486
#   ramp_down        0.718              0.414
#   offset           0.309              0.117
#   needle           0.000              0.115
#
# worst 1.005 -> 4 x 1.005 = 4.02 -> kappa = 8.  The kernels' own ratios (printed by every GPU test) never set it.
KAPPA = 8.0


def weight_term(A, Smax, u_p):
    """(u_p + 2^-23 (1 + Smax)) A: what kappa multiplies in bound()"""
    hd = A.shape[-1] // Smax.shape[-1]
    return (u_p + 2.0 ** -23 * (1.0 + Smax.repeat_interleave(hd, dim=-1))) * A


def bound(ref, A, Smax, u_p):
    """|out - ref| allowed per element: the fp16 rounding of the output (2^-11 |ref|, 2^-24 in the subnormals) + kappa (u_p +
    2^-23 (1 + Smax)) A.  u_p: the unit roundoff of the softmax weights in front of the second product (2^-11 where they are rounded
    to fp16: prefill and ragged; 0 where they stay fp32: the decode families).  2^-23 (1 + Smax): a score is a sum of fp32
    products of total magnitude <= Smax, so it carries an absolute error of that order, which exp turns into a relative error
    of the weight; A = sum_j p_j |v_jd| is what a relative error of the weights can move.  kappa: the table above; the derivation
    is in DESIGN.md §23."""
    return 2.0 ** -11 * ref.abs() + 2.0 ** -24 + KAPPA * weight_term(A, Smax, u_p)


def emulate(q16, K, V, n_keys_per_row, nq, nkv, hd, scale, u_p, rounded=True):
    """The arithmetic bound() describes, written from the formats alone (no kernel is consulted): fp32 scores from fp16 factors,
    fp32 exp, fp32 accumulation, one fp16 rounding of the output; for u_p > 0 the weights are rounded to fp16 in 32-key tiles
    under a running max with the alpha rescale.  Returns fp16 [R, nq * hd]; rounded=False: the fp32 quotient in front of the last
    rounding."""
    dev, R = q16.device, q16.shape[0]
    n = torch.as_tensor(n_keys_per_row, dtype=torch.long, device=dev).view(R)
    nmax = int(n.max())
    q, Kf, Vf = _heads(q16, nq, nkv, hd).float(), K[:, :nmax].float(), V[:, :nmax].float()
    valid = (torch.arange(nmax, device=dev)[None, :] < n[:, None])[:, None, None, :]
    s = (torch.einsum("rgpd,gjd->rgpj", q, Kf) * torch.tensor(scale, dtype=torch.float32)).masked_fill(~valid, float("-inf"))
    if u_p == 0:
        e = torch.exp(s - s.amax(-1, keepdim=True))
        o = torch.einsum("rgpj,gjd->rgpd", e, Vf) / e.sum(-1)[..., None]
        o = o.reshape(R, nq * hd)
        return o.half() if rounded else o
    m = torch.full(s.shape[:-1], float("-inf"), device=dev)
    l = torch.zeros_like(m)
    o = torch.zeros(*m.shape, hd, device=dev)
    for t0 in range(0, nmax, 32):
        st = s[..., t0:t0 + 32]
        m_new = torch.maximum(m, st.amax(-1))
        alpha = torch.exp(m - m_new)
        ph = torch.exp(st - m_new[..., None]).half().float()
        l = l * alpha + ph.sum(-1)
        o = o * alpha[..., None] + torch.einsum("rgpj,gjd->rgpd", ph, Vf[:, t0:t0 + 32])
        m = m_new
    o = (o / l[..., None]).reshape(R, nq * hd)
    return o.half() if rounded else o


# ------------------------------------------------------------------------------------------------------------ rotary embedding

def inv_freq(hd, dev):
    return 1.0 / (500000.0 ** (torch.arange(0, hd, 2, device=dev).float() / hd))


def unrope(target, pos, inv_f):
    """fp32 rows [..., hd] whose rotary embedding at position(s) pos is `target` (up to the fp16 rounding of the embedding): the
    inverse rotation, so that a test can ask for a rotated q or a new k of a given shape.  pos: a scalar or a tensor that
    broadcasts against target's leading dimensions."""
    half = target.shape[-1] // 2
    ang = torch.as_tensor(pos, device=target.device).double()[..., None] * inv_f.double()
    c, s = ang.cos(), ang.sin()
    t1, t2 = target[..., :half].double(), target[..., half:].double()
    return torch.cat((t1 * c + t2 * s, t2 * c - t1 * s), dim=-1).float()


def rope_f16(x, pos, inv_f):
    """qpal_rope_kv's rule in torch (cos / sin rounded to fp16, fp16 arithmetic), for the CPU self-test where no device rotates"""
    half = x.shape[-1] // 2
    ang = torch.as_tensor(pos, device=x.device).float()[..., None] * inv_f
    c, s = ang.cos().half(), ang.sin().half()
    x1, x2 = x[..., :half].half(), x[..., half:].half()
    return torch.cat((x1 * c + (-x2) * s, x2 * c + x1 * s), dim=-1)


# -------------------------------------------------------------------------------------------------------------- input families

OFFSET_DIM, OFFSET_Q, OFFSET_K = 3, 32.0, 64.0
FAMILIES = ("peaked", "ramp_up", "ramp_down", "offset", "needle")


@functools.lru_cache(maxsize=8)
def _host_randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _randn(shape, seed, dev):
    """N(0, 1) from a host generator (the same values on any device); a fresh copy every time"""
    return _host_randn(tuple(shape), seed).to(dev, copy=True)


def query_targets(R, nq, nkv, hd, seed, dev, family="base", shared=0.5):
    """The rotated q a test asks for, [R, nq * hd] fp32 ~ N(0, 1) (feed unrope() of it).  shared: the fraction of the variance
    that one common vector per kv head carries through all rows and all query heads of its group, so that a group (and a prefill
    chunk) has a direction for the ramp and needle keys to lie along.  offset: dimension OFFSET_DIM of every head is OFFSET_Q."""
    q = math.sqrt(1.0 - shared) * _randn((R, nkv, nq // nkv, hd), seed, dev)
    q = q + math.sqrt(shared) * _randn((1, nkv, 1, hd), seed + 1, dev)
    if family == "offset":
        q[..., OFFSET_DIM] = OFFSET_Q
    return q.reshape(R, nq * hd)


def _group_direction(q16, nq, nkv, hd):
    """per kv head: the sum of the unit vectors of its rows' and query heads' q, and the least projection of a q on it"""
    q = _f64(_heads(q16, nq, nkv, hd))
    u = (q / q.norm(dim=-1, keepdim=True)).sum(dim=(0, 2))           # [nkv, hd]
    u = u / u.norm(dim=-1, keepdim=True)
    proj = torch.einsum("rgpd,gd->rgp", q, u)
    return u, proj.amin(dim=(0, 2)), proj.mean(dim=(0, 2))           # [nkv, hd], [nkv], [nkv]


def build_cache(family, q16, nq, nkv, hd, L, n, scale, seed, needle_at=None):
    """fp32 targets (K, V) [nkv, L, hd] of one sequence whose keys 0 .. n - 1 are attended to by the rows q16 (a test casts them to
    the cache format; what the reference sees is the cast).  base: 0.5 N(0, 1), the existing tests' recipe.  peaked: keys scaled
    so that the scores have standard deviation ~6.  ramp_up / ramp_down: a component along the group's q direction so that the
    scores rise / fall by ~60 over keys 0 .. n - 1.  offset: dimension OFFSET_DIM of every key is OFFSET_K (with q's OFFSET_Q:
    every score near 2048 * scale).  needle: key needle_at lies along the group's direction, long enough to beat every other
    score of every row by 30, and its v is a pattern of +-1 .. +-4."""
    dev = q16.device
    K = 0.5 * _randn((nkv, L, hd), seed, dev)
    V = 0.5 * _randn((nkv, L, hd), seed + 1, dev)
    if family == "peaked":
        qrms = float(q16.float().pow(2).mean().sqrt())
        K = K * (2.0 * 6.0 / (qrms * math.sqrt(hd) * scale))         # (K is 0.5 N(0, 1): score sd = 0.5 c qrms sqrt(hd) scale)
    elif family in ("ramp_up", "ramp_down"):
        u, _, pmean = _group_direction(q16, nq, nkv, hd)
        t = torch.arange(L, device=dev, dtype=torch.float64) / max(n - 1, 1)
        t = t.clamp(max=1.0) if family == "ramp_up" else (1.0 - t).clamp(min=0.0)
        K = K + (60.0 / (pmean * scale))[:, None, None].float() * t[None, :, None].float() * u[:, None, :].float()
    elif family == "offset":
        K[..., OFFSET_DIM] = OFFSET_K
    elif family == "needle":
        u, pmin, _ = _group_direction(q16, nq, nkv, hd)
        other = (torch.einsum("rgpd,gjd->rgpj", _f64(_heads(q16, nq, nkv, hd)), K[:, :n].double()) * scale).amax(dim=(0, 2, 3))
        assert bool((pmin > 0).all()), "a query head points away from its group's direction: choose another seed"
        # e4m3 keeps 3 mantissa bits: 1.125 covers the cast's shortening of the needle and of its projection
        c = 1.125 * (32.0 + other.clamp(min=0.0)) / (pmin * scale)
        K[:, needle_at] = (c[:, None] * u).float()
        d = torch.arange(hd, device=dev)
        V[:, needle_at] = ((1 + d % 4) * (1 - 2 * (d // 4 % 2))).float()[None, :]
    elif family != "base":
        raise ValueError(family)
    return K, V


def to_cache(t, dtype):
    """the cast of fp32 targets to a cache format (e4m3: saturating, the store rule of the kernels)"""
    return t.half() if dtype == F16 else t.half().float().clamp(-448, 448).to(F8)


def nan_rows(cache, rows):
    """NaN into cache[..., rows, :] of either format (fp16 0x7E00, e4m3fn 0x7F)"""
    if cache.dtype == F16:
        cache[..., rows, :] = float("nan")
    else:
        cache.view(torch.uint8)[..., rows, :] = 0x7F


# --------------------------------------------------------------------------------------------------------------------- census

def census_cache(nkv, L, hd, dtype, dev):
    """K = 0 (every score is exactly 0, before and after the rotary embedding), V[j] = e_{j mod hd}: the output counts keys"""
    K = torch.zeros(nkv, L, hd, device=dev)
    V = torch.zeros(nkv, L, hd, device=dev)
    j = torch.arange(L, device=dev)
    V[:, j, j % hd] = 1.0
    return to_cache(K, dtype), to_cache(V, dtype)


def census_new_v(pos, nkv, hd, dev):
    """the new rows' v, fp32 [len(pos), nkv * hd]: e_{pos mod hd} for every kv head"""
    pos = torch.as_tensor(pos, device=dev).view(-1)
    v = torch.zeros(pos.shape[0], nkv, hd, device=dev)
    v[torch.arange(pos.shape[0], device=dev), :, pos.clamp(min=0) % hd] = 1.0
    return v.reshape(pos.shape[0], nkv * hd)


def census_expected(n_keys_per_row, nq, hd, dev):
    """out[r, h, d] = #{0 <= j < n[r] : j = d (mod hd)} / n[r] as float64 [R, nq * hd], and its tolerance: one fp16 ulp of the
    quotient (counts and n are exact in fp32; one fp32 division, one fp16 rounding; every merge weight is exp(0) = 1)"""
    n = torch.as_tensor(n_keys_per_row, dtype=torch.long, device=dev).view(-1, 1)
    d = torch.arange(hd, device=dev)[None, :]
    count = (n - d + hd - 1).clamp(min=0) // hd
    exp = (count.double() / n.double()).repeat(1, nq)
    return exp, fp16_ulp(exp)


def fp16_ulp(x):
    e = torch.floor(torch.log2(x.abs().clamp(min=2.0 ** -14)))
    return torch.pow(2.0, e - 10.0)


def census_fp64(K, V, n_keys_per_row, nq, nkv, hd, mutate=None):
    """attention_fp64 on a census cache (q is irrelevant: every key is 0): what a seeded defect does to the counts"""
    R = len(n_keys_per_row)
    q16 = torch.ones(R, nq * hd, dtype=F16, device=K.device)
    return attention_fp64(q16, K, V, n_keys_per_row, nq, nkv, hd, 1.0 / math.sqrt(hd), mutate)[0]
