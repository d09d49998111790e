"""Inputs, bounds and a second statement for the tests of the second MoE router and the shared experts (tests/test_moe_router_contract.py
on the CPU, tests/test_moe_router.py on the GPU).  numpy and CPU torch only — no GPU in this module.

The key's error bound, from moe_reference.logit_bounds' d (every fp32 logit within d[r, e] of its float64 value; D = the row's
largest d):
  sigmoid   |sigma'| <= 1 / 4, so the score moves by at most d / 4; its fp32 evaluation (expf within 2 ulp, one addition, one
            division) adds less than SIG_FP32 = 2^-21 of the score.
  softmax   numerator and denominator move by exp(+-D) each: the score by a factor within exp(+-2 D); the fp32 softmax adds
            moe_reference.GATE_FP32 relative.
  key       the score's bound, plus one fp32 rounding of the sum where a select_bias is added.
  group     "max": the largest key bound of the group (|max a' - max a| <= max |a' - a|); "top2": twice that, plus one rounding.
A row is DECIDABLE when every allowed group's score minus its bound lies above every other group's score plus its bound, and,
among the experts of the allowed groups, every chosen key minus its bound lies above every other key plus its bound.
The gates: with the scores of the chosen within eps_i, gate_i = s_i / sum s moves by at most (eps_i + gate_i sum eps) / (sum s -
sum eps) when renormalised (numerator, then denominator), by eps_i when not; the sum of at most 8 terms, the division and the
routed scale add GATE_OPS = 2^-20 relative.  The shared gate is a sigmoid of one more logit: d_s / 4 + SIG_FP32."""
import functools
import itertools

import numpy as np
import torch

import moe_reference as mref
from qpalette_amd import moe

SIG_FP32 = 2.0 ** -21
GATE_OPS = 2.0 ** -20
UNDECIDABLE_CAP = mref.UNDECIDABLE_CAP
EPS = 1e-5
ROUTED_SCALE = 2.5

# (n, H, E, top_k, n_group, topk_group): S = 2 (a lane walks its group), S = 20 (no power of two, groups across the lane-63 / 64
# border, wave reductions), one group (no group limit), and every limit at once
CASES = ((5, 64, 8, 3, 4, 2), (9, 160, 160, 6, 8, 3), (33, 256, 60, 4, 1, 1), (128, 128, 256, 8, 8, 4))
# (scoring, group_score, select_bias, renorm)
VARIANTS = tuple(itertools.product(("softmax", "sigmoid"), ("max", "top2"), (False, True), (False, True)))
# the first seed counted up from 0 that meets UNDECIDABLE_CAP for every variant of the case (test_moe_router_contract.py asserts it)
SEEDS = {CASES[0]: 0, CASES[1]: 0, CASES[2]: 0, CASES[3]: 0}


def inputs(case, seed, scoring, bias):
    """router entries N(0, 1) / sqrt(H) for sigmoid (4 / sqrt(H) would saturate it), 4 / sqrt(H) N(0, 1) for softmax, fp16; rows
    N(0, 1) fp32; RMSNorm weights 1 + 0.3 N(0, 1) fp16; a shared-gate weight N(0, 1) / sqrt(H) fp16; a select_bias of the scores'
    own spread (0.1 N(0, 1) for sigmoid, N(0, 1) / E for softmax); every fourth row (from row 2) inactive"""
    n, H, E, top_k, G, tg = case
    rng = np.random.default_rng(1000 * seed + n + 7 * E)
    amp = 4.0 if scoring == "softmax" else 1.0
    router_w = (amp / np.sqrt(H) * rng.standard_normal((E, H))).astype(np.float16)
    h = rng.standard_normal((n, H)).astype(np.float32)
    rms_w = (1.0 + 0.3 * rng.standard_normal(H)).astype(np.float16)
    shared_gate = (rng.standard_normal(H) / np.sqrt(H)).astype(np.float16)
    sb = ((0.1 if scoring == "sigmoid" else 1.0 / E) * rng.standard_normal(E)).astype(np.float32)
    active = np.arange(n, dtype=np.int64)
    active[2::4] = -1
    return dict(h=h, rms_w=rms_w, router_w=router_w, bias=None, select_bias=sb if bias else None, shared_gate=shared_gate,
                active=active, eps=EPS)


def router_of(case, variant, inp, shared_gate=True):
    scoring, group_score, _, renorm = variant
    return moe.Router(scoring, inp["select_bias"], case[4], case[5], group_score, renorm, ROUTED_SCALE,
                      inp["shared_gate"] if shared_gate else None)


@functools.lru_cache(maxsize=None)
def world(case, variant, seed=None):
    """(inputs, Router, the float64 route, bounds) of one case and variant: computed once, shared by the tests, never changed"""
    inp = inputs(case, SEEDS[case] if seed is None else seed, variant[0], variant[2])
    router = router_of(case, variant, inp)
    rt = moe.reference_route_ex(inp["h"], inp["rms_w"], inp["eps"], inp["router_w"], None, case[3], router, inp["active"])
    return inp, router, rt, bounds(rt, inp["router_w"], router)


def bounds(rt, router_w, router):
    """dict(d [n, E] the logit bounds, score, key [n, E], group [n, G] or None): the module's bounds on the fp32 route's distance
    from the float64 route `rt`"""
    d = mref.logit_bounds(rt, router_w)
    if router.scoring == "sigmoid":
        score = d / 4.0 + SIG_FP32 * rt["score"]
    else:
        score = rt["score"] * (np.expm1(2.0 * d.max(-1, keepdims=True)) + mref.GATE_FP32)
    key = score + (mref.U32 * np.abs(rt["key"]) if router.select_bias is not None else 0.0)
    group = None
    if router.n_group > 1:
        n, E = key.shape
        gmax = key.reshape(n, router.n_group, E // router.n_group).max(-1)
        group = gmax if router.group_score == "max" else 2.0 * gmax + mref.U32 * np.abs(rt["gscore"])
    return dict(d=d, score=score, key=key, group=group)


def decidable_rows(rt, b, top_k, router, active=None):
    """bool [n] by the module's rule (both gaps); inactive rows are decidable (they choose nothing)"""
    n, E = rt["key"].shape
    ok = np.ones(n, dtype=bool)
    for r in range(n):
        if router.n_group > 1 and router.topk_group < router.n_group:
            gs, gb = rt["gscore"][r], b["group"][r]
            best = np.lexsort((np.arange(router.n_group), -gs))[:router.topk_group]
            rest = np.setdiff1d(np.arange(router.n_group), best)
            ok[r] &= (gs[best] - gb[best]).min() > (gs[rest] + gb[rest]).max()
        ids = np.nonzero(rt["allowed"][r])[0]
        if top_k < len(ids):
            k, kb = rt["key"][r], b["key"][r]
            order = ids[np.lexsort((ids, -k[ids]))]
            chosen, rest = order[:top_k], order[top_k:]
            ok[r] &= (k[chosen] - kb[chosen]).min() > (k[rest] + kb[rest]).max()
    if active is not None:
        ok |= np.asarray(active) < 0
    return ok


def gate_tolerance(rt, b, router):
    """[n, top_k]: the module's bound on |gate - float64 gate| (rows whose sel is the contract's)"""
    sel = np.maximum(rt["sel"], 0)
    s = np.take_along_axis(rt["score"], sel, 1)
    eps = np.take_along_axis(b["score"], sel, 1)
    if router.renorm:
        tot, etot = s.sum(-1, keepdims=True), eps.sum(-1, keepdims=True)
        tol = (eps + s / tot * etot) / (tot - etot)
    else:
        tol = eps
    return np.where(rt["sel"] >= 0, tol * router.routed_scale + GATE_OPS * rt["gate"] + 1e-30, 0.0)


def shared_gate_tolerance(rt, shared_gate):
    """[n]: d_s / 4 + SIG_FP32, d_s the logit bound of the shared gate's dot product"""
    w = np.abs(np.asarray(shared_gate, dtype=np.float64))
    return mref.LOGIT_C * len(w) * mref.U32 * (np.abs(rt["xhat"]) @ w) / 4.0 + SIG_FP32


# ------------------------------------------------------------------------------------------------------------- the second statement
def model_card_route(logits, top_k, router):
    """The gates as the model cards write them (DeepSeek-V2 / V3's MoEGate, Qwen2-MoE's block): CPU torch float64, topk and
    masked_fill with -inf.  logits [n, E] float64 -> (sel int64 [n, top_k] ascending, gate [n, top_k])"""
    lg = torch.as_tensor(np.asarray(logits), dtype=torch.float64)
    n, E = lg.shape
    scores = lg.softmax(dim=-1) if router.scoring == "softmax" else lg.sigmoid()
    choice = scores.clone()
    if router.select_bias is not None:
        choice = choice + torch.as_tensor(np.asarray(router.select_bias), dtype=torch.float64)[None]
    if router.n_group > 1:
        grouped = choice.view(n, router.n_group, -1)
        gscore = grouped.max(dim=-1).values if router.group_score == "max" else grouped.topk(2, dim=-1).values.sum(dim=-1)
        gidx = gscore.topk(router.topk_group, dim=-1, sorted=False).indices
        gmask = torch.zeros_like(gscore).scatter_(1, gidx, 1.0)
        emask = gmask.unsqueeze(-1).expand(n, router.n_group, E // router.n_group).reshape(n, E)
        choice = choice.masked_fill(emask == 0, float("-inf"))
    idx = choice.topk(top_k, dim=-1, sorted=False).indices.sort(dim=-1).values
    w = scores.gather(1, idx)
    if router.renorm:
        w = w / w.sum(dim=-1, keepdim=True)
    return idx.numpy(), (w * router.routed_scale).numpy()


# -------------------------------------------------------------------------------------------------------- a whole layer of the router
DEFECTS = ("gate_from_key", "bias_in_the_gate", "group_max_for_top2", "expert_outside_the_groups", "routed_scale_dropped",
           "shared_gate_dropped", "shared_expert_twice")


def mutated_route(rt, router, mutate):
    """a copy of the float64 route `rt` (sel, gate, sgate) with one of DEFECTS' routing defects seeded"""
    sel, gate, sgate = rt["sel"].copy(), rt["gate"].copy(), rt["sgate"].copy()
    live = sel[:, 0] >= 0
    pick = lambda a: np.take_along_axis(a, np.maximum(sel, 0), 1)   # noqa: E731

    def gates(g):
        if router.renorm:
            g = g / g.sum(-1, keepdims=True)
        return np.where(live[:, None], g * router.routed_scale, 0.0)
    if mutate == "gate_from_key":
        gate = gates(pick(rt["key"]))
    elif mutate == "bias_in_the_gate":   # (behind the renormalisation: the finished gate carries the chosen expert's bias)
        sb = pick(np.broadcast_to(np.asarray(router.select_bias, dtype=np.float64), rt["score"].shape))
        gate = np.where(live[:, None], gate + sb * router.routed_scale, 0.0)
    elif mutate == "routed_scale_dropped":
        gate = gate / router.routed_scale
    elif mutate == "shared_gate_dropped":
        sgate = np.where(live, 1.0, 0.0)
    elif mutate in ("group_max_for_top2", "expert_outside_the_groups"):
        n, E = rt["key"].shape
        G, S = router.n_group, E // router.n_group
        for r in np.nonzero(live)[0]:
            if mutate == "group_max_for_top2":
                gs = rt["key"][r].reshape(G, S).max(-1)
                best = np.lexsort((np.arange(G), -gs))[:router.topk_group]
                ids = np.nonzero(np.isin(np.arange(E) // S, best))[0]
            else:
                ids = np.arange(E)   # no mask at all
            sel[r] = np.sort(ids[np.lexsort((ids, -rt["key"][r, ids]))[:sel.shape[1]]])
        gate = gates(np.take_along_axis(rt["score"], np.maximum(sel, 0), 1))
    return dict(rt, sel=sel, gate=gate, sgate=sgate)


def shared_forward(Ws, su_ug, su_dp, scale, rt, emu=False, twice=False):
    """the shared expert's term sgate[r] * Wdown (silu(Wgate x) * (Wup x)) on the rows of `rt`, float64 or (emu) with
    moe_reference.layer_forward's rounding points.  Ws = (up, gate, down): W^ * Wscale * scale of the shared expert"""
    up, gt, dn = Ws
    su_ug, su_dp = np.asarray(su_ug, dtype=np.float64), np.asarray(su_dp, dtype=np.float64)
    f16, f32 = mref.f16, mref.f32

    def apply(W, x, su):
        xr = mref.wht(x * su) / np.sqrt(x.shape[-1])
        xr = f16(f16(xr) / scale) if emu else xr / scale
        return f32(W @ xr) if emu else W @ xr
    out = np.zeros((rt["xhat"].shape[0], dn.shape[0]))
    for r in range(out.shape[0]):
        if rt["sgate"][r] == 0:
            continue
        x = f16(rt["xhat"][r]) if emu else rt["xhat"][r]
        u, g = apply(up, x, su_ug), apply(gt, x, su_ug)
        act = g / (1 + np.exp(-g)) * u
        y = apply(dn, f16(act) if emu else act, su_dp)
        out[r] = rt["sgate"][r] * y * (2.0 if twice else 1.0)
    return out


def layer_forward_ex(What, su_ug, su_dp, scale, Ws, s_su_ug, s_su_dp, s_scale, rt, router=None, emu=False, mutate=None):
    """routed sum (moe_reference.layer_forward on rt's sel and gates) + the shared term; mutate: one of DEFECTS"""
    if mutate is not None and mutate != "shared_expert_twice":
        rt = mutated_route(rt, router, mutate)
    out = mref.layer_forward(What, su_ug, su_dp, scale, rt, emu=emu)
    if Ws is not None:
        sh = shared_forward(Ws, s_su_ug, s_su_dp, s_scale, rt, emu=emu, twice=mutate == "shared_expert_twice")
        out = mref.f32(out + sh) if emu else out + sh
    return out


def layer_judge_ex(world_, rt, ok, got, router=None):
    """(factor per judged row, rows): the distance of `got` from the float64 layer in units of moe_reference.tolerance (KAPPA x the
    emulation's own distance); world_ = (What, su_ug, su_dp, scale, Ws, s_su_ug, s_su_dp, s_scale)"""
    rows = np.nonzero(ok)[0]
    ref = layer_forward_ex(*world_, rt)[rows]
    emu = layer_forward_ex(*world_, rt, emu=True)[rows]
    return mref.e_rows(np.asarray(got)[rows], ref) / mref.tolerance(mref.e_rows(emu, ref)), rows


def cpu_shared(H=512, Is=512, q_ug="tcq_6_none_0.9", q_dp="tcomb_6_7_0.5_none_0.9", seed=900, su_ug=None):
    """the shared expert of the layer tests rebuilt on the CPU from the same seeds (test_moe_router._shared): decoded by the oracle.
    -> (Ws, su_ug, su_dp, scale); su_ug given: the experts' own vector (the shared expert reads their rotated rows)"""
    from qpalette_amd import mem_op
    import gemv_reference as gref
    rng = np.random.default_rng(seed)
    own_ug, su_dp = (rng.integers(0, 2, H) * 2.0 - 1).astype(np.float16), (rng.integers(0, 2, Is) * 2.0 - 1).astype(np.float16)
    trip = []
    for k, m, q, s in ((H, Is, q_ug, seed + 1), (H, Is, q_ug, seed + 2), (Is, H, q_dp, seed + 3)):
        W = gref.oracle_weight(mem_op.dummy_linear_info(k, m, q, seed=s, codebook_seed=3)).astype(np.float64)
        ws = (np.random.default_rng(s).uniform(0.8, 1.2, m) / np.sqrt(k)).astype(np.float16).astype(np.float64)
        trip.append(W * ws[:, None] * 32.0)
    return trip, (own_ug if su_ug is None else su_ug), su_dp, 32.0
