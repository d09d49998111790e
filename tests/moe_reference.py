"""Inputs, bounds and brute-force restatements for the mixture-of-experts tests (tests/test_moe_contract.py on the CPU,
tests/test_moe.py on the GPU).  numpy only — no GPU in this module.

The router's error bound.  The kernel forms xhat in fp32 (the sum of squares as a chain of H / 1024 terms per thread and a fixed
tree, one division and square root, two multiplications: a relative error below (H / 256 + 14) u, u = 2^-24) and every logit as a chain
of H / 64 fused multiply-adds per lane and the wave's tree of 6 additions: |error| <= (H / 64 + 6) u sum |w| |xhat| to first order.
Together (H / 64 + H / 256 + 20) u sum |w x| <= 4 H u sum |w x| for every H >= 8: LOGIT_C = 4 is that round figure, derived from
the order of operations and not fitted to the kernel.

A row is DECIDABLE when the gap between its k-th and (k+1)-th float64 logits exceeds the sum of the two logits' bounds; only such
rows must reproduce the contract's sel.  The gates: with every logit within d of its float64 value a softmax term moves by a
factor within exp(+-2 d) (numerator and denominator by exp(+-d) each), a renormalised gate (a ratio of two such sums) by
exp(+-4 d); the fp32 softmax itself (the argument's rounding at |l - max| <= 64, expf, the sum over E <= 256 terms, the divisions)
adds less than GATE_FP32 = 2^-17 relative."""
import numpy as np

U32 = 2.0 ** -24
LOGIT_C = 4.0
GATE_FP32 = 2.0 ** -17
UNDECIDABLE_CAP = 0.10

# (n, H, E, top_k) of the route tests and the seed of each: the first seed counted up from 0 whose undecidable share is under the cap
# for every (renorm, bias) variant (test_moe_contract.py asserts it)
ROUTE_CASES = ((1, 128, 4, 2), (9, 160, 4, 2), (17, 256, 8, 2), (128, 512, 64, 8))
ROUTE_SEEDS = {(1, 128, 4, 2): 0, (9, 160, 4, 2): 0, (17, 256, 8, 2): 0, (128, 512, 64, 8): 0}
EPS = 1e-5


def route_inputs(n, H, E, top_k, seed, bias):
    """router entries 4 / sqrt(H) * N(0, 1) rounded to fp16; rows N(0, 1) in fp32 (the route normalises them) with RMSNorm weights
    1 + 0.3 N(0, 1) in fp16; every fourth row (from row 2) inactive where n > 1.  -> dict of numpy arrays"""
    rng = np.random.default_rng(1000 * seed + n + 7 * E)
    router_w = (4.0 / np.sqrt(H) * rng.standard_normal((E, H))).astype(np.float16)
    h = rng.standard_normal((n, H)).astype(np.float32)
    rms_w = (1.0 + 0.3 * rng.standard_normal(H)).astype(np.float16)
    b = rng.standard_normal(E).astype(np.float32) if bias else None
    active = np.arange(n, dtype=np.int64)
    if n > 1:
        active[2::4] = -1
    return dict(h=h, rms_w=rms_w, router_w=router_w, bias=b, active=active, eps=EPS)


def logit_bounds(rt, router_w):
    """[n, E]: LOGIT_C * H * 2^-24 * sum_i |w_ei| |xhat_i| for the float64 route `rt`"""
    W = np.abs(np.asarray(router_w, dtype=np.float64))
    H = W.shape[1]
    return LOGIT_C * H * U32 * (np.abs(rt["xhat"]) @ W.T)


def decidable_rows(rt, bounds, top_k, active=None):
    """bool [n]: the gap between the k-th and the (k+1)-th largest float64 logit exceeds the sum of the two logits' bounds (top_k = E:
    every row).  Inactive rows are decidable (they choose nothing)."""
    lg = rt["logits"]
    n, E = lg.shape
    ok = np.ones(n, dtype=bool)
    if top_k < E:
        for r in range(n):
            o = np.lexsort((np.arange(E), -lg[r]))
            a, b = o[top_k - 1], o[top_k]
            ok[r] = lg[r, a] - lg[r, b] > bounds[r, a] + bounds[r, b]
    if active is not None:
        ok |= np.asarray(active) < 0
    return ok


def gate_tolerance(rt, bounds, renorm):
    """[n, top_k]: the module's bound on |gate - float64 gate|"""
    d = bounds.max(-1, keepdims=True)
    rel = np.expm1((4.0 if renorm else 2.0) * d) + GATE_FP32
    return rt["gate"] * rel + 1e-30


def brute_layout(sel, E):
    """reference_layout restated without a sort: position of a pair = the number of routed pairs with a smaller (expert, id)"""
    sel = np.asarray(sel)
    n, top_k = sel.shape
    flat = [int(v) for v in sel.reshape(-1)]
    P = len(flat)
    valid = [i for i in range(P) if 0 <= flat[i] < E]
    inv = [-1] * P
    for i in valid:
        inv[i] = sum(1 for j in valid if (flat[j], j) < (flat[i], i))
    order = [-1] * P
    for i in valid:
        order[inv[i]] = i
    groups = []
    for e in range(E):
        mine = sorted(inv[i] for i in valid if flat[i] == e)
        for c in range(0, len(mine), 8):
            groups.append((e, mine[c], len(mine[c:c + 8])))
    return dict(order=order, inv=inv, x_index=[o // top_k if o >= 0 else -1 for o in order], groups=groups)


def brute_max_groups(n, E, top_k):
    """max over every count vector 0 <= c_e <= n, sum c_e = n top_k of sum ceil(c_e / 8), by a table over (experts used, pairs placed)"""
    P = n * top_k
    best = {0: 0}
    for _ in range(E):
        nxt = {}
        for placed, g in best.items():
            for c in range(0, min(n, P - placed) + 1):
                v = g + (c + 7) // 8
                if nxt.get(placed + c, -1) < v:
                    nxt[placed + c] = v
        best = nxt
    return best[P]


def counts_to_sel(counts, n, top_k):
    """a routing [n, top_k] (ascending ids per row) whose experts hold exactly `counts` pairs (c_e <= n, sum = n top_k): the experts,
    fullest first, are dealt to the rows in turn"""
    slots = []
    for e in sorted(range(len(counts)), key=lambda e: -counts[e]):
        slots += [e] * counts[e]
    assert len(slots) == n * top_k and max(counts) <= n
    rows = [[] for _ in range(n)]
    for i, e in enumerate(slots):
        rows[i % n].append(e)
    assert all(len(set(r)) == top_k for r in rows)
    return np.array([sorted(r) for r in rows], dtype=np.int64)


def worst_counts(n, E, top_k):
    """a count vector that reaches brute_max_groups (the same table, with the argmax kept)"""
    P = n * top_k
    best = {0: (0, [])}
    for _ in range(E):
        nxt = {}
        for placed, (g, cs) in best.items():
            for c in range(0, min(n, P - placed) + 1):
                v = g + (c + 7) // 8
                if placed + c not in nxt or nxt[placed + c][0] < v:
                    nxt[placed + c] = (v, cs + [c])
        best = nxt
    return best[P][1]


# ------------------------------------------------------------------------------------------------------------- a whole sparse layer
R16 = 2.0 ** -11          # one fp16 rounding
GEMV_RTOL_ABS = 1e-5      # the project's GEMV bar, times sum |w x|


def wht(a):
    """unnormalised Walsh-Hadamard transform (Sylvester order) of the last axis, float64"""
    a = np.array(a, dtype=np.float64)
    n, h = a.shape[-1], 1
    while h < n:
        a = a.reshape(*a.shape[:-1], n // (2 * h), 2, h)
        a = np.stack((a[..., 0, :] + a[..., 1, :], a[..., 0, :] - a[..., 1, :]), axis=-2).reshape(*a.shape[:-3], n)
        h *= 2
    return a


def layer_reference(What, su_ug, su_dp, scale, rt, bounds, renorm, active=None):
    """The output of one sparse layer (without the residual) on the rows of the float64 route `rt`, and its bound, on each expert's
    own decoded weights.  What[e] = (up, gate, down) float64: W^ * Wscale * scale; widths are powers of two (the rotation is the
    Walsh-Hadamard transform).  -> (ref [n, H], tol [n, H], ok bool [n]: the rows whose routing is decidable and active).

    The bound, from the formats: the rotated input of a projection is rounded to fp16 twice (relative 2^-11 each) and the GEMV adds
    1e-5 sum |w x|, so a projection is off by at most (2^-10 + 1e-5) |W^| |xr|; silu' <= 1.1 carries the gate's error; up, gate,
    silu and their product are rounded to fp16 (4 * 2^-11 of the activation); the activation's error reaches the output through
    |W_down R diag(SU)|; the gates move by gate_tolerance.  Every term is a worst case (absolute values summed): wide next to a
    typical error, narrow next to a defect — another expert's output is an independent draw of the same spread."""
    n, top_k = rt["sel"].shape
    H, I = What[0][0].shape[1], What[0][0].shape[0]
    su_ug, su_dp = np.asarray(su_ug, dtype=np.float64), np.asarray(su_dp, dtype=np.float64)
    ok = decidable_rows(rt, bounds, top_k, active)
    if active is not None:
        ok &= np.asarray(active) >= 0
    gtol = gate_tolerance(rt, bounds, renorm)
    ref, tol = np.zeros((n, H)), np.zeros((n, H))
    dn_eff = {}
    for r in np.nonzero(ok)[0]:
        xr = wht(rt["xhat"][r] * su_ug) / np.sqrt(H) / scale
        for j in range(top_k):
            e = int(rt["sel"][r, j])
            up, gt, dn = What[e]
            if e not in dn_eff:
                dn_eff[e] = np.abs(wht(dn) / np.sqrt(I) * su_dp[None, :] / scale)   # |dn R diag(SU) / scale|: y = dn_eff act
            u, g = up @ xr, gt @ xr
            du, dg = ((2 * R16 + GEMV_RTOL_ABS) * (np.abs(w) @ np.abs(xr)) for w in (up, gt))
            s = g / (1 + np.exp(-g))
            act = s * u
            dact = 1.1 * dg * np.abs(u) + np.abs(s) * du + 4 * R16 * np.abs(act)
            xa = wht(act * su_dp) / np.sqrt(I) / scale
            y = dn @ xa
            dy = dn_eff[e] @ dact + (2 * R16 + GEMV_RTOL_ABS) * (np.abs(dn) @ np.abs(xa))
            ref[r] += rt["gate"][r, j] * y
            tol[r] += rt["gate"][r, j] * dy + gtol[r, j] * np.abs(y) + 2.0 ** -22 * np.abs(y)
    return ref, tol, ok


# ------------------------------------------------------------------------------------- the layer against its own format emulation
KAPPA, TEETH = 4.0, 4.0   # model_reference's: the tolerance is KAPPA x the emulation's own distance, a defect must land TEETH x outside
DEFECTS = ("gates_not_renormalised", "softmax_over_the_chosen", "top_k_minus_1", "up_gate_swapped_in_one_expert", "expert_of_the_next_row",
           "gate_without_down_wscale", "another_su")


def f16(a):
    return np.asarray(a, dtype=np.float64).astype(np.float16).astype(np.float64)


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def layer_forward(What, su_ug, su_dp, scale, rt, emu=False, mutate=None, wscale_dn=None, other_su=None):
    """The output of one sparse layer (without the residual) on the rows of the float64 route `rt`: float64, or (emu) with the formats'
    rounding points as model_reference.forward_emulated places them — the fused norm's one fp16 rounding, fp16 after the rotation
    and after its 1 / scale, fp32 projections, fp16 silu(gate) up, fp32 output (the router and the gates stay float64: their fp32
    error is far below one fp16 rounding).  What[e] = (up, gate, down): W^ * Wscale * scale.  mutate: one of DEFECTS —
    gates_not_renormalised / softmax_over_the_chosen (the gates of the other `renorm`: rt must carry "p"), top_k_minus_1 (the last
    chosen expert dropped), up_gate_swapped_in_one_expert (the lowest chosen id), expert_of_the_next_row, gate_without_down_wscale
    (wscale_dn[e]: down's Wscale, divided out again), another_su (other_su in place of su_ug)."""
    n, top_k = rt["sel"].shape
    H, I = What[0][0].shape[1], What[0][0].shape[0]
    su_ug = np.asarray(other_su if mutate == "another_su" else su_ug, dtype=np.float64)
    su_dp = np.asarray(su_dp, dtype=np.float64)

    def apply(W, x, su):
        xr = wht(x * su) / np.sqrt(x.shape[-1])
        xr = f16(f16(xr) / scale) if emu else xr / scale
        y = W @ xr
        return f32(y) if emu else y

    sel, gate = rt["sel"], rt["gate"]
    if mutate in ("gates_not_renormalised", "softmax_over_the_chosen"):
        g = np.where(sel >= 0, np.take_along_axis(rt["p"], np.maximum(sel, 0), 1), 0.0)
        gate = g if mutate == "gates_not_renormalised" else g / np.maximum(g.sum(-1, keepdims=True), 1e-300)
    if mutate == "expert_of_the_next_row":
        sel = np.roll(sel, -1, axis=0)
    out = np.zeros((n, H))
    for r in range(n):
        x = f16(rt["xhat"][r]) if emu else rt["xhat"][r]
        for j in range(top_k - 1 if mutate == "top_k_minus_1" else top_k):
            e = int(sel[r, j])
            if e < 0 or rt["sel"][r, j] < 0:
                continue
            up, gt, dn = What[e]
            if mutate == "up_gate_swapped_in_one_expert" and j == 0:
                up, gt = gt, up
            u, g = apply(up, x, su_ug), apply(gt, x, su_ug)
            act = g / (1 + np.exp(-g)) * u
            y = apply(dn, f16(act) if emu else act, su_dp)
            if mutate == "gate_without_down_wscale":
                y = y / np.asarray(wscale_dn[e], dtype=np.float64)
            out[r] += gate[r, j] * y
    return f32(out) if emu else out


def e_rows(got, ref):
    """per row: ||got - ref||_2 / ||ref||_2"""
    return np.linalg.norm(np.asarray(got, dtype=np.float64) - ref, axis=-1) / np.linalg.norm(ref, axis=-1)


def tolerance(emu_err):
    """model_reference.tolerance: KAPPA x the emulation's own distance per row, floored at the median over the rows"""
    return KAPPA * np.maximum(emu_err, np.median(emu_err))


def layer_judge(What, su_ug, su_dp, scale, rt, ok, got):
    """(factor per judged row: the distance of `got` from the float64 layer in units of the tolerance; the rows judged)"""
    rows = np.nonzero(ok)[0]
    ref = layer_forward(What, su_ug, su_dp, scale, rt)[rows]
    emu = layer_forward(What, su_ug, su_dp, scale, rt, emu=True)[rows]
    return e_rows(np.asarray(got)[rows], ref) / tolerance(e_rows(emu, ref)), rows


def cpu_layer(E=8, H=512, I=512, q_ug="tcq_6_none_0.9", q_dp="tcomb_6_7_0.5_none_0.9", seed=100):
    """the sparse layer of the model tests rebuilt on the CPU from the same seeds (test_moe._layer): decoded by the oracle"""
    from qpalette_amd import mem_op
    import gemv_reference as gref
    rng = np.random.default_rng(seed)
    su_ug, su_dp = (rng.integers(0, 2, H) * 2.0 - 1).astype(np.float16), (rng.integers(0, 2, I) * 2.0 - 1).astype(np.float16)
    What, wsc_dn = [], []
    for e in range(E):
        trip = []
        for k, m, q, s in ((H, I, q_ug, 10 * e + 1), (H, I, q_ug, 10 * e + 2), (I, H, q_dp, 10 * e + 3)):
            W = gref.oracle_weight(mem_op.dummy_linear_info(k, m, q, seed=s, codebook_seed=3)).astype(np.float64)
            ws = (np.random.default_rng(s).uniform(0.8, 1.2, m) / np.sqrt(k)).astype(np.float16).astype(np.float64)
            trip.append(W * ws[:, None] * 32.0)
        What.append(trip)
        wsc_dn.append(ws)
    router = (4.0 / np.sqrt(H) * rng.standard_normal((E, H))).astype(np.float16)
    return What, su_ug, su_dp, 32.0, router, wsc_dn
