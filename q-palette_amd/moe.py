"""Mixture-of-experts MLPs on the quantized experts (csrc/moe_route.hip, csrc/moe_gemv.hip).

A layer has n <= 128 rows, E <= 256 experts and 1 <= top_k <= min(8, E): P = n * top_k routed pairs (r, j), pair id r * top_k + j.
Six launches per layer, no host read between them:

  had.rotate (rms)      x16 [n, H]     the RMSNorm + rotation every expert's up | gate shares (ONE SU for the layer)
  route                 sel, gate, order, inv, x_index, the group table, ngroups        (qpal_moe_route)
  moe_gemv up | gate    ug32 [P, 2 I]  row = sorted position, x row through x_index       (qpal_moe_gemv)
  had.rotate (SwiGLU)   act16 [P, I]   the rotation every expert's down shares
  moe_gemv down         y32 [P, H]
  combine               h[r] += sum_j gate[r][j] * y32[inv[r][j]]                           (qpal_moe_combine)

The contract is restated in numpy float64 below (reference_route, reference_layout, reference_moe_mlp), as the other modules keep
theirs; tests/test_moe_contract.py checks the restatement, tests/test_moe.py holds the kernels to it.

The second router and shared experts: a layer built with scoring=, select_bias=, n_group=, topk_group=,
group_score=, routed_scale=, shared= or shared_gate= routes through qpal_moe_route_ex (reference_route_ex), runs its shared expert
(an IncoherentMLP) on the same normed rows with the dense MLP's launches into ws.ys32, and folds it in with the one combine
launch (qpal_moe_combine_shared, reference_combine_shared).  A layer built without them launches exactly the six above."""
import collections
import ctypes
import math

import numpy as np
import torch
import torch.nn as nn

from . import _native as nat
from . import hadamard as had
from . import linear
from .linear.incoherent_linear import IncoherentLinear

MAX_ROWS, MAX_EXPERTS, MAX_TOP_K, GROUP_ROWS, MAX_HIDDEN = 128, 256, 8, 8, 8192


# ------------------------------------------------------------------------------------------------------------------ the contract
def _check_shape(n, E, top_k):
    if not (1 <= n <= MAX_ROWS and 1 <= E <= MAX_EXPERTS and 1 <= top_k <= min(MAX_TOP_K, E)):
        raise nat.QpalError(f"moe: need 1 <= n <= {MAX_ROWS}, 1 <= E <= {MAX_EXPERTS}, 1 <= top_k <= min({MAX_TOP_K}, E); "
                            f"got n = {n}, E = {E}, top_k = {top_k}")


def max_groups(n, E, top_k):
    """The largest ngroups any routing of the shape can give (exactly): max of sum_e ceil(c_e / 8) over 0 <= c_e <= n with
    sum_e c_e = n * top_k (every such count vector is a routing: a row's experts are distinct, so c_e <= n is all it takes).
    N groups over a = min(E, N) experts in use exist iff N <= a G and 8 N - 7 a <= P <= 8 N - t f, where n = 8 G - t and
    f = max(0, N - a (G - 1)) experts must hold G groups (more experts in use only widen the range).  The host-side twin of
    qpal_moe_max_groups; it sizes every grid and workspace."""
    _check_shape(n, E, top_k)
    P, G = n * top_k, (n + 7) // 8
    t = 8 * G - n
    best = 0
    for N in range(1, min(P, E * G) + 1):
        a = min(E, N)
        f = max(0, N - a * (G - 1))
        if N <= a * G and 8 * N - 7 * a <= P <= 8 * N - t * f:
            best = N
    return best


def reference_route(h, rms_w, eps, router_w, router_bias, top_k, renorm, active=None):
    """float64.  -> dict(xhat [n, H], logits [n, E], p [n, E], sel int [n, top_k], gate [n, top_k]).
    xhat = h * rsqrt(mean(h^2) + eps) * rms_w; logits = xhat @ router_w.T (+ bias); p = softmax over all E; the chosen set is the
    top_k largest logits, ties to the lower expert id; sel lists it in ascending expert id; gate = p[sel], divided by its sum when
    renorm.  Rows with active[r] < 0 choose nothing: sel -1, gate 0."""
    h = np.asarray(h, dtype=np.float64)
    W = np.asarray(router_w, dtype=np.float64)
    n, E = h.shape[0], W.shape[0]
    xhat = h / np.sqrt((h * h).mean(-1, keepdims=True) + float(eps))
    if rms_w is not None:
        xhat = xhat * np.asarray(rms_w, dtype=np.float64)
    logits = xhat @ W.T
    if router_bias is not None:
        logits = logits + np.asarray(router_bias, dtype=np.float64)
    z = logits - logits.max(-1, keepdims=True)
    p = np.exp(z)
    p = p / p.sum(-1, keepdims=True)
    sel = np.full((n, top_k), -1, dtype=np.int64)
    gate = np.zeros((n, top_k))
    for r in range(n):
        if active is not None and int(active[r]) < 0:
            continue
        chosen = np.sort(np.lexsort((np.arange(E), -logits[r]))[:top_k])   # by (-logit, id): ties to the lower id
        sel[r] = chosen
        g = p[r, chosen]
        gate[r] = g / g.sum() if renorm else g
    return dict(xhat=xhat, logits=logits, p=p, sel=sel, gate=gate)


Router = collections.namedtuple("Router", "scoring select_bias n_group topk_group group_score renorm routed_scale shared_gate",
                                defaults=("softmax", None, 1, 1, "max", True, 1.0, None))
Router.__doc__ = """The record of the second router: scoring in {"softmax", "sigmoid"}; select_bias fp32 [E] or None; n_group,
topk_group; group_score in {"max", "top2"}; renorm; routed_scale; shared_gate fp16 [H] or None (numpy for the contract, CUDA
tensors for the launches)."""
SCORINGS, GROUP_SCORES = ("softmax", "sigmoid"), ("max", "top2")


def check_router(router, E, top_k):
    """the argument rules of qpal_moe_route_ex, as QpalError before any stream work"""
    if router.scoring not in SCORINGS or router.group_score not in GROUP_SCORES:
        raise nat.QpalError(f"moe: scoring must be one of {SCORINGS} and group_score one of {GROUP_SCORES}, got {router.scoring!r}, "
                            f"{router.group_score!r}")
    G, tg = router.n_group, router.topk_group
    if not (isinstance(G, int) and isinstance(tg, int) and G >= 1 and E % G == 0 and 1 <= tg <= G):
        raise nat.QpalError(f"moe: need E % n_group == 0 and 1 <= topk_group <= n_group; got E = {E}, n_group = {G}, topk_group = {tg}")
    S = E // G
    if tg * S < top_k:
        raise nat.QpalError(f"moe: the allowed groups hold topk_group * S = {tg * S} experts, fewer than top_k = {top_k}")
    if router.group_score == "top2" and S < 2:
        raise nat.QpalError(f"moe: group_score \"top2\" needs groups of at least two experts, got S = {S}")
    rs = router.routed_scale
    if isinstance(rs, bool) or not isinstance(rs, (int, float)) or not math.isfinite(rs) or not rs > 0:
        raise nat.QpalError(f"moe: routed_scale must be finite and > 0, got {rs!r}")


ROUTER_PRESETS = ("mixtral", "qwen2", "deepseek_v2", "deepseek_v3")


def router_preset(name, E, top_k):
    """The router arguments of MoEMLP for a family of checkpoints, without the tensors: mixtral (the first router), qwen2 (softmax,
    gates not renormalised; its shared expert is gated: give shared_gate=), deepseek_v2 (softmax, the best half of the groups by their
    maximum, a routed scale, no renormalisation), deepseek_v3 (sigmoid, a select_bias= to be given, the best half of the groups by
    the sum of their two best, renormalised, scale 2.5).  The groups: the most of 8, 4, 2 that divide E into groups of at least two
    experts and leave top_k experts in the allowed half."""
    if name not in ROUTER_PRESETS:
        raise nat.QpalError(f"moe: router preset {name!r} is none of {ROUTER_PRESETS}")
    G = next((g for g in (8, 4, 2) if E % g == 0 and E // g >= 2 and (g // 2) * (E // g) >= top_k), 1)
    groups = dict(n_group=G, topk_group=max(1, G // 2))
    return {"mixtral": dict(), "qwen2": dict(scoring="softmax", renorm=False),
            "deepseek_v2": dict(scoring="softmax", renorm=False, group_score="max", routed_scale=16.0, **groups),
            "deepseek_v3": dict(scoring="sigmoid", renorm=True, group_score="top2", routed_scale=2.5, **groups)}[name]


def reference_route_ex(h, rms_w, eps, router_w, router_bias, top_k, router, active=None):
    """float64.  -> dict(xhat [n, H], logits, score, key [n, E], gscore [n, n_group] or None, allowed bool [n, E], sel int
    [n, top_k], gate [n, top_k], sgate [n]).
    1. xhat and logits are exactly as in reference_route.  The existing router_bias still adds to the logits.
    2. score = softmax(logits) over all E, or 1 / (1 + exp(-logits)).
    3. key = score + select_bias.  The bias decides who is chosen and never enters a gate.  (An expert whose logit is -inf — the
       kernel's image of a NaN logit too — has key -inf whatever its bias: it is chosen only when nothing else is left.)
    4. With n_group > 1: experts g S .. g S + S - 1, S = E / n_group, form group g.  Its score is the largest key in it ("max") or
       the sum of its two largest ("top2").  The topk_group groups with the largest score are allowed, ties to the lower group id.
       An expert outside them is never chosen.  (The Hugging Face code fills masked keys with 0.0, which differs only when an
       allowed key is negative.)
    5. The chosen set is the top_k largest keys among the allowed experts, ties to the lower expert id.  sel lists it in ascending
       expert id.
    6. gate = score[sel], not key.  It is divided by its sum over the chosen in ascending-id order when renorm, then multiplied by
       routed_scale.
    7. sgate[r] = sigmoid(xhat[r] . shared_gate), or exactly 1.0 without shared_gate.
    8. Rows with active[r] < 0 get sel -1, gate 0 and sgate 0."""
    h = np.asarray(h, dtype=np.float64)
    W = np.asarray(router_w, dtype=np.float64)
    n, E = h.shape[0], W.shape[0]
    _check_shape(n, E, top_k)
    check_router(router, E, top_k)
    xhat = h / np.sqrt((h * h).mean(-1, keepdims=True) + float(eps))
    if rms_w is not None:
        xhat = xhat * np.asarray(rms_w, dtype=np.float64)
    logits = xhat @ W.T
    if router_bias is not None:
        logits = logits + np.asarray(router_bias, dtype=np.float64)
    if router.scoring == "softmax":
        score = np.exp(logits - logits.max(-1, keepdims=True))
        score = score / score.sum(-1, keepdims=True)
    else:
        score = 1.0 / (1.0 + np.exp(-logits))
    key = score if router.select_bias is None else score + np.asarray(router.select_bias, dtype=np.float64)
    key = np.where(np.isneginf(logits), -np.inf, key)
    G = router.n_group
    S = E // G
    allowed = np.ones((n, E), dtype=bool)
    gscore = None
    if G > 1:
        grouped = np.sort(key.reshape(n, G, S), axis=-1)
        gscore = grouped[..., -1] if router.group_score == "max" else grouped[..., -1] + grouped[..., -2]
        for r in range(n):
            best = np.lexsort((np.arange(G), -gscore[r]))[:router.topk_group]
            allowed[r] = np.isin(np.arange(E) // S, best)
    sel = np.full((n, top_k), -1, dtype=np.int64)
    gate = np.zeros((n, top_k))
    sgate = np.ones(n) if router.shared_gate is None else 1.0 / (1.0 + np.exp(-(xhat @ np.asarray(router.shared_gate, dtype=np.float64))))
    for r in range(n):
        if active is not None and int(active[r]) < 0:
            sgate[r] = 0.0
            continue
        ids = np.nonzero(allowed[r])[0]
        chosen = np.sort(ids[np.lexsort((ids, -key[r, ids]))[:top_k]])
        sel[r] = chosen
        g = score[r, chosen]
        if router.renorm:
            den = 0.0
            for v in g:
                den += v
            g = g / den
        gate[r] = g * float(router.routed_scale)
    return dict(xhat=xhat, logits=logits, score=score, key=key, gscore=gscore, allowed=allowed, sel=sel, gate=gate, sgate=sgate)


def reference_layout(sel, E):
    """Pure integer work, exact.  sel int [n, top_k] (-1: no expert) -> dict of int arrays: order [P] (the pair at each sorted
    position, -1 behind the routed pairs), inv [P] (the position of each pair, or -1), x_index [P] (order // top_k, or -1),
    group_expert / group_first / group_count [ngroups] (every expert's run cut into groups of at most 8 consecutive positions, in
    sorted order) and ngroups.  The pairs with 0 <= sel < E are sorted by (expert, pair id), stably."""
    sel = np.asarray(sel, dtype=np.int64)
    n, top_k = sel.shape
    P = n * top_k
    flat = sel.reshape(-1)
    pairs = [i for i in range(P) if 0 <= flat[i] < E]
    pairs.sort(key=lambda i: (int(flat[i]), i))
    order = np.full(P, -1, dtype=np.int64)
    inv = np.full(P, -1, dtype=np.int64)
    order[:len(pairs)] = pairs
    for pos, i in enumerate(pairs):
        inv[i] = pos
    x_index = np.where(order >= 0, order // top_k, -1)
    ge, gf, gc = [], [], []
    pos = 0
    while pos < len(pairs):
        e = int(flat[pairs[pos]])
        run = pos
        while run < len(pairs) and int(flat[pairs[run]]) == e:
            run += 1
        for first in range(pos, run, GROUP_ROWS):
            ge.append(e), gf.append(first), gc.append(min(GROUP_ROWS, run - first))
        pos = run
    return dict(order=order, inv=inv, x_index=x_index, group_expert=np.array(ge, dtype=np.int64),
                group_first=np.array(gf, dtype=np.int64), group_count=np.array(gc, dtype=np.int64), ngroups=len(ge))


def reference_combine(base, y, gate, inv, accumulate):
    """The fp32 contract of qpal_moe_combine in its stated order: out[r] (+)= sum_j gate[r][j] * y[inv[r][j]], every product rounded
    to fp32, the sum built in j order, then added (accumulate) or stored."""
    gate, y = np.asarray(gate, dtype=np.float32), np.asarray(y, dtype=np.float32)
    n, top_k = gate.shape
    inv = np.asarray(inv).reshape(n, top_k)
    out = np.array(base, dtype=np.float32) if accumulate else np.zeros((n, y.shape[1]), dtype=np.float32)
    for r in range(n):
        acc = None
        for j in range(top_k):
            if inv[r, j] >= 0:
                t = (gate[r, j] * y[inv[r, j]]).astype(np.float32)
                acc = t if acc is None else (acc + t).astype(np.float32)
        if acc is not None:
            out[r] = (out[r] + acc).astype(np.float32) if accumulate else acc
    return out


def reference_combine_shared(base, y, gate, inv, ys, sgate, accumulate):
    """The fp32 contract of qpal_moe_combine_shared: the routed sum is built as reference_combine builds it; then
    t = fp32(sgate[r] * ys[r]), one rounding; the row's term is acc + t, or t alone where the row has no routed pair; the term is
    added to base (accumulate) or stored.  A row with sgate[r] == 0 exactly gets no shared term at all, not even 0 * ys: what ys
    holds for an inactive row never reaches the stream."""
    gate, y = np.asarray(gate, dtype=np.float32), np.asarray(y, dtype=np.float32)
    ys, sgate = np.asarray(ys, dtype=np.float32), np.asarray(sgate, dtype=np.float32)
    n, top_k = gate.shape
    inv = np.asarray(inv).reshape(n, top_k)
    out = np.array(base, dtype=np.float32) if accumulate else np.zeros((n, y.shape[1]), dtype=np.float32)
    for r in range(n):
        acc = None
        for j in range(top_k):
            if inv[r, j] >= 0:
                t = (gate[r, j] * y[inv[r, j]]).astype(np.float32)
                acc = t if acc is None else (acc + t).astype(np.float32)
        if sgate[r] != 0:
            t = (sgate[r] * ys[r]).astype(np.float32)
            acc = t if acc is None else (acc + t).astype(np.float32)
        if acc is not None:
            out[r] = (out[r] + acc).astype(np.float32) if accumulate else acc
    return out


def _silu(v):
    return v / (1.0 + np.exp(-v))


def reference_moe_mlp(h, rms_w, eps, router_w, router_bias, top_k, renorm, active, experts):
    """The whole layer in float64: h[r] += sum_j gate[r][j] * Wdown_e (silu(Wgate_e xhat) * (Wup_e xhat)), e = sel[r][j], j ascending.
    experts: per expert (W_up [I, H], W_gate [I, H], W_down [H, I]), the EFFECTIVE weights (W_eff of tests/model_reference.py:
    diag(Wscale) W^ R diag(SU), times the wrapper's scales).  -> (h_out [n, H], the reference_route dict)"""
    rt = reference_route(h, rms_w, eps, router_w, router_bias, top_k, renorm, active)
    out = np.array(h, dtype=np.float64)
    for r in range(out.shape[0]):
        for j in range(top_k):
            e = int(rt["sel"][r, j])
            if e < 0:
                continue
            up, gt, dn = (np.asarray(w, dtype=np.float64) for w in experts[e])
            out[r] += rt["gate"][r, j] * (dn @ (_silu(gt @ rt["xhat"][r]) * (up @ rt["xhat"][r])))
    return out, rt


def reference_moe_mlp_ex(h, rms_w, eps, router_w, router_bias, top_k, router, active, experts, shared=None):
    """The whole layer of the second router in float64: reference_moe_mlp's routed sum with reference_route_ex's sel and gates,
    plus sgate[r] * Wdown_s (silu(Wgate_s xhat) * (Wup_s xhat)) for shared = (W_up [Is, H], W_gate [Is, H], W_down [H, Is]), the
    shared expert's EFFECTIVE weights.  -> (h_out [n, H], the reference_route_ex dict)"""
    rt = reference_route_ex(h, rms_w, eps, router_w, router_bias, top_k, router, active)
    out = np.array(h, dtype=np.float64)
    for r in range(out.shape[0]):
        for j in range(top_k):
            e = int(rt["sel"][r, j])
            if e < 0:
                continue
            up, gt, dn = (np.asarray(w, dtype=np.float64) for w in experts[e])
            out[r] += rt["gate"][r, j] * (dn @ (_silu(gt @ rt["xhat"][r]) * (up @ rt["xhat"][r])))
        if shared is not None and rt["sgate"][r] != 0:
            up, gt, dn = (np.asarray(w, dtype=np.float64) for w in shared)
            out[r] += rt["sgate"][r] * (dn @ (_silu(gt @ rt["xhat"][r]) * (up @ rt["xhat"][r])))
    return out, rt


# ------------------------------------------------------------------------------------------------------------------ the launches
class MoEWorkspace:
    """Every buffer the six launches of one layer write, for up to n rows: allocated once (moe_workspace), reused by every layer
    of a step whose shapes agree.  The ticket word of qpal_moe_route is zero between launches."""

    def __init__(self, n, E, top_k, H, I, dev, shared_I=0):
        """shared_I: the width of the layer's shared expert (0: none).  With one: sgate [n] (the shared gates of the route), sx16
        [n, H] (its rotated input where it cannot take x16), sug32 [n, 2 Is], sact16 [n, Is] and ys32 [n, H] (its output)"""
        _check_shape(n, E, top_k)
        self.n, self.E, self.top_k, self.H, self.I, self.shared_I = n, E, top_k, H, I, shared_I
        self.P, self.max_groups = n * top_k, max_groups(n, E, top_k)
        i32 = dict(dtype=torch.int32, device=dev)
        self.ticket = torch.zeros(4, **i32)
        self.sel = torch.full((n, top_k), -1, **i32)
        self.gate = torch.zeros(n, top_k, dtype=torch.float32, device=dev)
        self.order, self.inv, self.x_index = (torch.full((self.P,), -1, **i32) for _ in range(3))
        self.group_expert = torch.full((self.max_groups,), -1, **i32)
        self.group_first, self.group_count = torch.zeros(self.max_groups, **i32), torch.zeros(self.max_groups, **i32)
        self.ngroups = torch.zeros(1, **i32)
        self.x16 = torch.zeros(n, H, dtype=torch.float16, device=dev)
        self.ug32 = torch.zeros(self.P, 2 * I, dtype=torch.float32, device=dev)
        self.act16 = torch.zeros(self.P, I, dtype=torch.float16, device=dev)
        self.y32 = torch.zeros(self.P, H, dtype=torch.float32, device=dev)
        self.sgate = self.sx16 = self.sug32 = self.sact16 = self.ys32 = None
        if shared_I:
            self.sgate = torch.zeros(n, dtype=torch.float32, device=dev)
            self.sx16 = torch.zeros(n, H, dtype=torch.float16, device=dev)
            self.sug32 = torch.zeros(n, 2 * shared_I, dtype=torch.float32, device=dev)
            self.sact16 = torch.zeros(n, shared_I, dtype=torch.float16, device=dev)
            self.ys32 = torch.zeros(n, H, dtype=torch.float32, device=dev)

    def fits(self, n, E, top_k, H, I, dev):
        return (self.n >= n and (self.E, self.top_k, self.H, self.I) == (E, top_k, H, I) and self.ticket.device == torch.device(dev))

    def rows(self, n):
        """the views of a launch on n <= self.n rows (the group table keeps its full length: max_groups is monotone in n); built
        once per n"""
        if n == self.n:
            return self
        views = self.__dict__.setdefault("_views", {})
        if n not in views:
            views[n] = self._view(n)
        return views[n]

    def _view(self, n):
        v = object.__new__(MoEWorkspace)
        v.__dict__.update({k: t for k, t in self.__dict__.items() if k != "_views"})
        v.n, v.P = n, n * self.top_k
        v.sel, v.gate, v.x16 = self.sel[:n], self.gate[:n], self.x16[:n]
        v.order, v.inv, v.x_index = self.order[:v.P], self.inv[:v.P], self.x_index[:v.P]
        v.ug32, v.act16, v.y32 = self.ug32[:v.P], self.act16[:v.P], self.y32[:v.P]
        if self.shared_I:
            v.sgate, v.sx16, v.sug32, v.sact16, v.ys32 = self.sgate[:n], self.sx16[:n], self.sug32[:n], self.sact16[:n], self.ys32[:n]
        return v


def moe_workspace(n, E, top_k, H, I, dev, shared_I=0):
    return MoEWorkspace(n, E, top_k, H, I, dev, shared_I=shared_I)


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _want(t, name, dtype, shape=None):
    if t is None:
        return
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise nat.QpalError(f"moe: {name} must be a contiguous {dtype} CUDA tensor" + (f" of shape {tuple(shape)}" if shape else "")
                            + f", got {t.dtype} {tuple(t.shape)} on {t.device}")


def route(h32, rms, router_w, router_bias, top_k, renorm, ws, active=None, router=None, sgate_out=None):
    """qpal_moe_route on the rows of h32 (fp32 [n, H], row stride h32.stride(0)): fills ws.sel .. ws.ngroups.  rms = (eps, weight
    fp16 [H] or None); router_w fp16 [E, H]; router_bias fp32 [E] or None; active: int64 [n] (rows with a negative entry choose
    nothing) or None.  router: None launches qpal_moe_route; a Router (CUDA tensors) launches qpal_moe_route_ex — `renorm` is then
    the record's, and the shared gates go to sgate_out (fp32 [n]; default ws.sgate; None: not written, refused with a shared_gate)."""
    n, H = h32.shape
    E = router_w.shape[0]
    eps, w = rms
    if h32.dtype != torch.float32 or not h32.is_cuda or h32.stride(1) != 1:
        raise nat.QpalError("moe.route: h32 must be fp32 CUDA rows")
    _want(router_w, "router_w", torch.float16, (E, H)), _want(router_bias, "router_bias", torch.float32, (E,))
    _want(w, "the RMSNorm weight", torch.float16, (H,)), _want(active, "active", torch.int64, (n,))
    if (ws.n, ws.E, ws.top_k) != (n, E, top_k):
        raise nat.QpalError(f"moe.route: the workspace is for (n, E, top_k) = {(ws.n, ws.E, ws.top_k)}, the call has {(n, E, top_k)}")
    if router is not None:
        check_router(router, E, top_k)
        sgate_out = ws.sgate if sgate_out is None else sgate_out
        _want(router.select_bias, "select_bias", torch.float32, (E,)), _want(router.shared_gate, "shared_gate", torch.float16, (H,))
        _want(sgate_out, "the shared gates' output", torch.float32, (n,))
        if router.shared_gate is not None and sgate_out is None:
            raise nat.QpalError("moe.route: a shared_gate needs somewhere to put its gates (a workspace built with shared_I, or sgate_out=)")
        st = nat.MoeRouter(SCORINGS.index(router.scoring), router.n_group, router.topk_group, GROUP_SCORES.index(router.group_score),
                           1 if router.renorm else 0, float(router.routed_scale), _ptr(router.select_bias), _ptr(router.shared_gate),
                           _ptr(sgate_out))
        with torch.cuda.device_of(h32):
            nat.check(nat.lib().qpal_moe_route_ex(h32.data_ptr(), h32.stride(0), _ptr(w), float(eps), router_w.data_ptr(), _ptr(router_bias),
                                                  _ptr(active), n, H, E, top_k, ws.sel.data_ptr(), ws.gate.data_ptr(),
                                                  ws.order.data_ptr(), ws.inv.data_ptr(), ws.x_index.data_ptr(),
                                                  ws.group_expert.data_ptr(), ws.group_first.data_ptr(), ws.group_count.data_ptr(),
                                                  ws.ngroups.data_ptr(), ws.group_expert.numel(), ws.ticket.data_ptr(),
                                                  ctypes.byref(st), _stream(h32)), "qpal_moe_route_ex")
        return ws
    with torch.cuda.device_of(h32):
        nat.check(nat.lib().qpal_moe_route(h32.data_ptr(), h32.stride(0), _ptr(w), float(eps), router_w.data_ptr(), _ptr(router_bias),
                                           _ptr(active), n, H, E, top_k, 1 if renorm else 0, ws.sel.data_ptr(), ws.gate.data_ptr(),
                                           ws.order.data_ptr(), ws.inv.data_ptr(), ws.x_index.data_ptr(), ws.group_expert.data_ptr(),
                                           ws.group_first.data_ptr(), ws.group_count.data_ptr(), ws.ngroups.data_ptr(),
                                           ws.group_expert.numel(), ws.ticket.data_ptr(), _stream(h32)), "qpal_moe_route")
    return ws


class Projection:
    """One projection kind of a layer's experts as qpal_moe_gemv takes it: device tables of the experts' stream (and second
    stream, Wscale) pointers.  Keeps the tensors it points at alive."""

    def __init__(self, streams1, streams2, wscales, m, k, kv, kv2, tlut_bits=9):
        dev = streams1[0].device
        self.keep = (list(streams1), None if streams2 is None else list(streams2), None if wscales is None else list(wscales))
        self.E, self.m, self.k, self.kv, self.kv2, self.tlut_bits = len(streams1), m, k, kv, kv2, tlut_bits
        kc = k // 2 if streams2 is not None else k
        for ts, v, what, nbytes in ((streams1, kv, "stream", m * kc * kv // 16), (streams2, kv2, "second stream", m * kc * kv2 // 16),
                                    (wscales, 1, "Wscale", 2 * m)):
            for e, t in enumerate(ts or ()):   # the kernel trusts the tables: every pointer must cover what a launch reads
                if not t.is_cuda or t.device != dev or not t.is_contiguous() or t.numel() * t.element_size() != nbytes:
                    raise nat.QpalError(f"moe.Projection: expert {e}'s {what} must be a contiguous tensor of {nbytes} bytes on {dev}")
        if (streams2 is None) != (kv2 == 0) or len(streams2 or streams1) != self.E or len(wscales or streams1) != self.E:
            raise nat.QpalError("moe.Projection: one stream (and Wscale) per expert; a second one exactly when kv2 is given")

        def table(ts):
            return None if ts is None else torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=dev)
        self.c1, self.c2, self.wscale = table(streams1), table(streams2), table(wscales)

    def struct(self, out_col):
        return nat.MoeProj(_ptr(self.c1), _ptr(self.c2), _ptr(self.wscale), self.m, self.kv, self.kv2, out_col)


def moe_gemv(out, projs, x16, tlut, group_expert, group_first, group_count, ngroups, x_index=None, oscale=1.0, out_cols=None):
    """qpal_moe_gemv: for every group g < min(ngroups, len(group_expert)) and every projection in `projs` (one or two Projection
    objects of one k): out[group_first[g] + b][out_col + row] = (W_e x16[xi])[row] * wscale_e[row] * oscale for b < group_count[g],
    e = group_expert[g], xi = x_index[group_first[g] + b] (or the position itself).  out fp32 [P, ldo]; out_cols: the first
    column of each projection (default: one behind the other)."""
    if out.dtype != torch.float32 or not out.is_cuda or out.dim() != 2 or out.stride(1) != 1:
        raise nat.QpalError("moe_gemv: out must be fp32 CUDA rows")
    if x16.dtype != torch.float16 or not x16.is_cuda or x16.dim() != 2 or x16.stride(1) != 1:
        raise nat.QpalError("moe_gemv: x must be fp16 CUDA rows")
    for t, name in ((group_expert, "group_expert"), (group_first, "group_first"), (group_count, "group_count"), (ngroups, "ngroups"),
                    (x_index, "x_index")):
        _want(t, name, torch.int32)
    if not 1 <= len(projs) <= 2 or any(p.k != x16.shape[1] or p.E != projs[0].E for p in projs):
        raise nat.QpalError("moe_gemv: one or two projections of x's width and one expert count")
    for p in projs:
        if p.tlut_bits != 9 or not 2 <= p.kv <= 8 or (p.kv2 and not p.kv2 <= 8):
            raise nat.QpalError(f"moe_gemv: the routed kernel decodes tcq_* and tcomb_* layers with codebooks of 512 pairs (S = 9) and KV 2..8 "
                                f"(S = 9); got S = {p.tlut_bits}, KV = {(p.kv, p.kv2) if p.kv2 else p.kv}")
    if x_index is not None and x_index.numel() < out.shape[0]:
        raise nat.QpalError("moe_gemv: x_index must have an entry for every row of out")
    if not (len(group_expert) == len(group_first) == len(group_count)):
        raise nat.QpalError("moe_gemv: the three columns of the group table differ in length")
    if out_cols is None:
        out_cols = [sum(p.m for p in projs[:i]) for i in range(len(projs))]
    key = (tuple(id(p) for p in projs[1:]), tuple(out_cols))
    cache = projs[0].__dict__.setdefault("_arrays", {})   # the argument structs of a launch are built once
    if key not in cache:
        cache[key] = (nat.MoeProj * len(projs))(*[p.struct(c) for p, c in zip(projs, out_cols)])
    arr = cache[key]
    _want(tlut, "tlut", torch.float16)
    with torch.cuda.device_of(out):
        nat.check(nat.lib().qpal_moe_gemv(out.data_ptr(), out.stride(0), out.shape[0], arr, len(projs), x16.data_ptr(), x16.stride(0),
                                          x16.shape[0], _ptr(x_index), group_expert.data_ptr(), group_first.data_ptr(),
                                          group_count.data_ptr(), ngroups.data_ptr(), len(group_expert), projs[0].E, x16.shape[1],
                                          tlut.data_ptr(), projs[0].tlut_bits, float(oscale), _stream(out)), "qpal_moe_gemv")
    return out


def combine(out, y32, gate, inv, accumulate=True, shared=None):
    """qpal_moe_combine: out[r] (+)= sum_j gate[r][j] * y32[inv[r][j]] (j ascending, fp32); out fp32 [n, H] rows.  shared = (ys32
    fp32 [n, H] rows, sgate fp32 [n]): qpal_moe_combine_shared, + sgate[r] * ys32[r] behind the routed sum."""
    n, top_k = gate.shape
    _want(gate, "gate", torch.float32), _want(inv, "inv", torch.int32), _want(y32, "y", torch.float32)
    if out.dtype != torch.float32 or not out.is_cuda or out.stride(1) != 1 or out.shape != (n, y32.shape[1]) or inv.numel() != n * top_k:
        raise nat.QpalError("moe.combine: out must be fp32 CUDA rows [n, H], inv one entry per pair")
    if shared is not None:
        ys, sgate = shared
        _want(sgate, "sgate", torch.float32, (n,))
        if ys.dtype != torch.float32 or not ys.is_cuda or ys.stride(1) != 1 or ys.shape != out.shape:
            raise nat.QpalError("moe.combine: the shared expert's rows must be fp32 CUDA rows [n, H]")
        with torch.cuda.device_of(out):
            nat.check(nat.lib().qpal_moe_combine_shared(out.data_ptr(), out.stride(0), y32.data_ptr(), y32.stride(0), gate.data_ptr(),
                                                        inv.data_ptr(), ys.data_ptr(), ys.stride(0), sgate.data_ptr(), n, top_k,
                                                        y32.shape[1], y32.shape[0], 1 if accumulate else 0, _stream(out)),
                      "qpal_moe_combine_shared")
        return out
    with torch.cuda.device_of(out):
        nat.check(nat.lib().qpal_moe_combine(out.data_ptr(), out.stride(0), y32.data_ptr(), y32.stride(0), gate.data_ptr(), inv.data_ptr(),
                                             n, top_k, y32.shape[1], y32.shape[0], 1 if accumulate else 0, _stream(out)),
                  "qpal_moe_combine")
    return out


# ------------------------------------------------------------------------------------------------------------------ the module
def _codec(il, who):
    """(class name, KV, KV2, streams) of an expert projection, or a QpalError naming what the routed kernel cannot decode"""
    inner = il.linear
    if isinstance(inner, linear.QTIPLinearTCQ):
        key, streams = ("tcq", inner.KV, 0), (inner.trellis, None)
    elif isinstance(inner, linear.CombtLinearTCQ) and inner.use_comb_kernel:
        key, streams = ("tcomb", inner.KV[0], inner.KV[1]), (inner.trellis1, inner.trellis2)
    else:
        raise nat.QpalError(f"MoEMLP: {who} is a {type(inner).__name__}: the routed kernel decodes tcq_* and tcomb_*_0.5 layers only "
                            "(no comb_*, ldlq_*, SIMT packings or unquantized experts)")
    if inner.tlut_bits != 9 or max(key[1], key[2]) > 8 or key[1] < 2:
        raise nat.QpalError(f"MoEMLP: {who} has S = {inner.tlut_bits}, KV = {inner.KV}: the routed kernel has the codebooks of 512 pairs (S = 9) "
                            "with KV 2..8 only (1 to 4 bits per weight)")
    return key, streams


def _shared_ug(mlp):
    """(layers, their Wscale slices) of a shared expert's up | gate group (decoder.ug_layout)"""
    inter = mlp.intermediate_size
    if mlp.merge_ug:
        return [mlp.ug_proj], [mlp.Wscale_ug]
    return [mlp.up_proj, mlp.gate_proj], [mlp.Wscale_ug[:inter], mlp.Wscale_ug[inter:]]


class MoEMLP(nn.Module):
    """A sparse MLP: fp16 router [E, H] (+ fp32 bias), E experts of (up, gate, down) IncoherentLinear modules that share ONE SU for
    up | gate and ONE for down, left-only rotations, one scale and one codebook.  forward runs the six launches of the module's
    first paragraph on fp32 rows [n, H].

    scoring, select_bias, n_group, topk_group, group_score, routed_scale: the fields of the second router (Router); shared: an
    IncoherentMLP of the layer's hidden width and any intermediate width, in tensor-core-order codecs with a silu activation (it
    carries its own SUs and scale); shared_gate: fp16 [H], the weight of its per-row sigmoid gate (None: the shared expert counts
    in full).  With every one of them at its default the layer is the first router's, launch for launch."""

    def __init__(self, router_w, experts, top_k, renorm=True, router_bias=None, scoring="softmax", select_bias=None, n_group=1,
                 topk_group=1, group_score="max", routed_scale=1.0, shared=None, shared_gate=None):
        super().__init__()
        E = len(experts)
        if router_w.dim() != 2 or router_w.shape[0] != E:
            raise nat.QpalError(f"MoEMLP: router_w must be [E = {E}, H], got {tuple(router_w.shape)}")
        H = router_w.shape[1]
        _check_shape(1, E, top_k)
        if H % 32 or H > MAX_HIDDEN:
            raise nat.QpalError(f"MoEMLP: the hidden width must be a multiple of 32 up to {MAX_HIDDEN}, got {H}")
        ups, gates, downs = ([t[i] for t in experts] for i in range(3))
        for kind, mods in (("up", ups), ("gate", gates), ("down", downs)):
            for e, il in enumerate(mods):
                if not isinstance(il, IncoherentLinear):
                    raise nat.QpalError(f"MoEMLP: expert {e}'s {kind} is a {type(il).__name__}, not an IncoherentLinear")
        dev = ups[0].SU.device
        I = ups[0].out_features
        keys = {}
        for kind, mods, (k, m) in (("up", ups, (H, I)), ("gate", gates, (H, I)), ("down", downs, (I, H))):
            for e, il in enumerate(mods):
                who = f"expert {e}'s {kind}"
                key, _ = _codec(il, who)
                if keys.setdefault(kind, key) != key:
                    raise nat.QpalError(f"MoEMLP: one quantizer string per projection kind: {who} is {key}, expert 0's is {keys[kind]}")
                if (il.in_features, il.out_features) != (k, m):
                    raise nat.QpalError(f"MoEMLP: {who} is [{il.out_features}, {il.in_features}], expected [{m}, {k}]")
                if il.skip_l or not il.skip_r or il.bias is not None:
                    raise nat.QpalError(f"MoEMLP: {who} must be rotated on the left only (rot_info 'skip_r', applied) and have no bias")
                if il.scale != ups[0].scale:
                    raise nat.QpalError(f"MoEMLP: one scale for the layer: {who} has {il.scale}, expert 0's up {ups[0].scale}")
                ref = (ups[0] if kind != "down" else downs[0]).SU
                if il.SU.device != dev or not torch.equal(il.SU, ref):
                    raise nat.QpalError(f"MoEMLP: ONE SU shared by all experts' {'up and gate' if kind != 'down' else 'down'} (one "
                                        f"rotation serves the layer): {who} differs from expert 0's")
        if (keys["up"][2] != 0) != (keys["gate"][2] != 0):
            raise nat.QpalError("MoEMLP: up and gate share a launch: both single-stream (tcq_*) or both column-split (tcomb_*)")
        inners = [il.linear for il in ups + gates + downs]
        if linear.share_codebooks(inners) != 1:
            raise nat.QpalError("MoEMLP: the experts must share ONE codebook (share_codebooks left more than one)")
        self.hidden_size, self.intermediate_size, self.num_experts, self.top_k, self.renorm = H, I, E, top_k, bool(renorm)
        self.scale = float(ups[0].scale)
        self.experts = nn.ModuleList([nn.ModuleList(t) for t in experts])   # keeps every stream and Wscale alive
        self.register_buffer("router_w", router_w.detach().to(dev, torch.float16).contiguous())
        self.register_buffer("router_bias", None if router_bias is None else router_bias.detach().to(dev, torch.float32).contiguous())
        self.register_buffer("SU_ug", ups[0].SU.detach().clone())
        self.register_buffer("SU_dp", downs[0].SU.detach().clone())
        hk, self.hidden_K = had.get_hadK(H)
        ik, self.inter_K = had.get_hadK(I)
        self.register_buffer("had_left_ug_T", None if hk is None else hk.T.contiguous().half().to(dev), persistent=False)
        self.register_buffer("had_left_dp_T", None if ik is None else ik.T.contiguous().half().to(dev), persistent=False)
        self.tlut = inners[0].tlut

        def proj(mods, k, m):
            cs = [_codec(il, "")[1] for il in mods]
            key = _codec(mods[0], "")[0]
            return Projection([c[0] for c in cs], [c[1] for c in cs] if key[2] else None, [il.Wscale for il in mods], m, k, key[1], key[2])
        self.p_up, self.p_gate, self.p_down = proj(ups, H, I), proj(gates, H, I), proj(downs, I, H)
        self._ws = []   # the module's own workspaces (forward without a step): every one handed out stays alive
        # ---- the second router and the shared expert (None, None: the first router's six launches)
        plain = (scoring == "softmax" and select_bias is None and n_group == 1 and topk_group == 1 and group_score == "max"
                 and routed_scale == 1.0 and shared is None and shared_gate is None)
        self.register_buffer("select_bias", None if select_bias is None else select_bias.detach().to(dev, torch.float32).contiguous())
        self.register_buffer("shared_gate", None if shared_gate is None else shared_gate.detach().to(dev, torch.float16).contiguous())
        self.shared = shared
        self.router = None
        self.shared_x16 = False   # the shared expert reads the experts' own rotated rows
        if not plain:
            for t, name, width in ((self.select_bias, "select_bias", E), (self.shared_gate, "shared_gate", H)):
                if t is not None and tuple(t.shape) != (width,):
                    raise nat.QpalError(f"MoEMLP: {name} must be [{width}], got {tuple(t.shape)}")
            if shared_gate is not None and shared is None:
                raise nat.QpalError("MoEMLP: shared_gate= gates a shared expert: give shared= too")
            self.router = Router(scoring, self.select_bias, n_group, topk_group, group_score, bool(renorm), routed_scale, self.shared_gate)
            check_router(self.router, E, top_k)
        if shared is not None:
            self._check_shared(shared, H, dev)
            self.shared_x16 = bool(shared.scale == self.scale and torch.equal(shared.SU_ug.to(dev).float(), self.SU_ug.float()))

    @staticmethod
    def _check_shared(mlp, H, dev):
        from .linear import IncoherentMLP
        from .linear._base import PackedLinearBase
        if not isinstance(mlp, IncoherentMLP) or mlp.hidden_size != H or mlp.hidden_act not in ("silu", "swish"):
            raise nat.QpalError(f"MoEMLP: shared= must be an IncoherentMLP of hidden width {H} with a silu activation")
        for l in _shared_ug(mlp)[0] + [mlp.down_proj]:
            if not isinstance(l, PackedLinearBase) or isinstance(l, linear.VQLinearPackSIMT):
                raise nat.QpalError(f"MoEMLP: the shared expert's projections must be tensor-core-order packed layers (the dense "
                                    f"fused path), got a {type(l).__name__}")
        if mlp.SU_ug.device != torch.device(dev):
            raise nat.QpalError(f"MoEMLP: the shared expert lives on {mlp.SU_ug.device}, the experts on {dev}")

    @staticmethod
    def from_experts(router_w, experts, top_k, renorm=True, router_bias=None, **router):
        """experts: a list of (up, gate, down) IncoherentLinear triples (quantize_experts builds one).  Checks what the launches
        assume — one quantizer string per projection kind, ONE SU for all up and gate, ONE for all down, left-only rotation, one
        scale, one codebook — builds the pointer tables and keeps the modules alive.  **router: scoring=, select_bias=, n_group=,
        topk_group=, group_score=, routed_scale=, shared=, shared_gate= (the class's)."""
        return MoEMLP(router_w, [tuple(t) for t in experts], top_k, renorm=renorm, router_bias=router_bias, **router)

    @property
    def shared_size(self):
        return 0 if self.shared is None else self.shared.intermediate_size

    def shape_key(self):
        return (self.num_experts, self.top_k, self.hidden_size, self.intermediate_size, self.shared_size, self.router_w.device)

    def launches(self, n):
        """kernel launches of run() on n rows: the six routed ones; with a shared expert its rotation (none where it reads the
        experts' rotated rows), its up | gate launch(es), its SwiGLU rotation and its down"""
        if self.shared is None:
            return 6
        return 6 + (0 if self.shared_x16 else 1) + len(linear.launch_groups(_shared_ug(self.shared)[0], n <= 8)) + 2

    def new_workspace(self, n):
        """fresh buffers for up to n rows: a step class takes its own when it is built and keeps them for its lifetime, so a
        captured graph never outlives the memory it names"""
        return moe_workspace(n, self.num_experts, self.top_k, self.hidden_size, self.intermediate_size, self.router_w.device,
                             shared_I=self.shared_size)

    def workspace(self, n):
        """the module's own buffers for up to n rows (forward outside a step).  A larger request allocates a new workspace and KEEPS
        the earlier ones: a graph captured on one of them stays valid."""
        for ws in self._ws:
            if ws.n >= n:
                return ws.rows(n)
        self._ws.append(self.new_workspace(n))
        return self._ws[-1].rows(n)

    def run(self, h32, rms, out, accumulate, active=None, ws=None):
        """the six launches on the rows of h32; the layer's output is added into (accumulate) or written over `out` (fp32 [n, H])"""
        n = h32.shape[0]
        ws = self.workspace(n) if ws is None else ws.rows(n)
        had.rotate(h32, hadK=self.had_left_ug_T, K=self.hidden_K, su=self.SU_ug, post_scale=1.0 / self.scale, rms=rms,
                   in_mode=had.IN_F32, out=ws.x16)
        route(h32, rms, self.router_w, self.router_bias, self.top_k, self.renorm, ws, active=active, router=self.router)
        table = (ws.group_expert, ws.group_first, ws.group_count, ws.ngroups)
        moe_gemv(ws.ug32, [self.p_up, self.p_gate], ws.x16, self.tlut, *table, x_index=ws.x_index, oscale=self.scale)
        had.rotate(ws.ug32, in_mode=had.IN_SWIGLU_F32, hadK=self.had_left_dp_T, K=self.inter_K, su=self.SU_dp,
                   post_scale=1.0 / self.scale, out=ws.act16)
        moe_gemv(ws.y32, [self.p_down], ws.act16, self.tlut, *table, oscale=self.scale)
        if self.shared is None:
            return combine(out, ws.y32, ws.gate, ws.inv, accumulate=accumulate)
        # the shared expert on the same normed rows, every row (an inactive row's result stays out: its gate is 0): the dense MLP's
        # launches, written over ws.ys32
        sh = self.shared
        x16 = ws.x16
        if not self.shared_x16:
            x16 = had.rotate(h32, hadK=self.had_left_ug_T, K=self.hidden_K, su=sh.SU_ug, post_scale=1.0 / sh.scale, rms=rms,
                             in_mode=had.IN_F32, out=ws.sx16)
        ugl, ugw = _shared_ug(sh)
        linear.multi_gemv(ugl, x16, outs=list(ws.sug32.split([l.out_features for l in ugl], dim=1)), wscales=ugw, oscale=sh.scale)
        had.rotate(ws.sug32, in_mode=had.IN_SWIGLU_F32, hadK=sh.had_left_dp_T, K=sh.inter_K, su=sh.SU_dp, post_scale=1.0 / sh.scale,
                   out=ws.sact16)
        linear.multi_gemv([sh.down_proj], ws.sact16, outs=[ws.ys32], wscales=[sh.Wscale_dp], oscale=sh.scale)
        return combine(out, ws.y32, ws.gate, ws.inv, accumulate=accumulate, shared=(ws.ys32, ws.sgate))

    def forward(self, h, rms, active=None):
        """h: fp32 [..., H] rows of the residual stream; rms = (eps, weight fp16 [H] or None), the norm in front of the layer.
        Returns the layer's output (without the residual), fp32, h's shape."""
        h32 = h.reshape(-1, self.hidden_size)
        if h32.dtype != torch.float32 or not h32.is_cuda:
            raise nat.QpalError("MoEMLP: the rows must be fp32 on the GPU (no CPU implementation)")
        out = torch.empty_like(h32)
        return self.run(h32.contiguous(), rms, out, False, active=active).view(h.shape)


def quantize_experts(router_w, ups, gates, downs, quantizer_str, top_k, H_ug=None, H_dp=None, codebooks=None, lut_cache=None,
                     renorm=True, router_bias=None, seed=0, shared=None, **router):
    """Quantise E experts and build their MoEMLP.  ups / gates: E weights [I, H]; downs: E weights [H, I] (CUDA tensors or
    nn.Linear); quantizer_str: one string, or (up, gate, down); H_ug / H_dp: per-expert proxy Hessians ([E] lists, entries may be
    None) or None.  Every expert's up and gate get ONE random sign vector, every down another: the layer's two rotations.
    shared: (up [Is, H], gate [Is, H], down [H, Is]) weights of a shared expert, quantised with quantize_linear like a dense MLP
    (the strings of the experts, or the fourth to sixth of six; sign vectors of its own); **router: the
    second router's arguments and shared_gate=, as MoEMLP takes them."""
    from .quantize_layer import quantize_linear
    E = len(ups)
    qs = (quantizer_str,) * 3 if isinstance(quantizer_str, str) else tuple(quantizer_str)   # (six: the shared expert's behind)
    W0 = ups[0].weight if isinstance(ups[0], nn.Linear) else ups[0]
    I, H = W0.shape
    g = torch.Generator().manual_seed(seed)
    su_ug = (torch.randint(0, 2, (H,), generator=g) * 2 - 1).to(W0.device, torch.float32)
    su_dp = (torch.randint(0, 2, (I,), generator=g) * 2 - 1).to(W0.device, torch.float32)
    H_ug = [None] * E if H_ug is None else H_ug
    H_dp = [None] * E if H_dp is None else H_dp
    kw = dict(left_only=True, codebooks=codebooks, lut_cache=lut_cache)
    experts = []
    for e in range(E):
        up, _ = quantize_linear(ups[e], qs[0], H=H_ug[e], SU=su_ug.clone(), **kw)
        gt, _ = quantize_linear(gates[e], qs[1], H=H_ug[e], SU=su_ug.clone(), **kw)
        dn, _ = quantize_linear(downs[e], qs[2], H=H_dp[e], SU=su_dp.clone(), **kw)
        experts.append((up, gt, dn))
    if shared is not None:
        from .linear import IncoherentMLP
        Ws = shared[0].weight if isinstance(shared[0], nn.Linear) else shared[0]
        Is = Ws.shape[0]
        s_ug = (torch.randint(0, 2, (H,), generator=g) * 2 - 1).to(W0.device, torch.float32)
        s_dp = (torch.randint(0, 2, (Is,), generator=g) * 2 - 1).to(W0.device, torch.float32)
        sq = qs[3:6] if len(qs) >= 6 else qs[:3]
        up, _ = quantize_linear(shared[0], sq[0], SU=s_ug.clone(), **kw)
        gt, _ = quantize_linear(shared[1], sq[1], SU=s_ug.clone(), **kw)
        dn, _ = quantize_linear(shared[2], sq[2], SU=s_dp.clone(), **kw)
        mlp = IncoherentMLP(H, Is, "silu")
        mlp.up_proj, mlp.gate_proj, mlp.down_proj = up.linear, gt.linear, dn.linear
        mlp = mlp.to(W0.device)
        mlp.SU_ug.data.copy_(up.SU), mlp.SU_dp.data.copy_(dn.SU)
        mlp.Wscale_ug.data.copy_(torch.cat([up.Wscale, gt.Wscale], dim=-1)), mlp.Wscale_dp.data.copy_(dn.Wscale)
        mlp.scale = up.scale
        router["shared"] = mlp
    return MoEMLP.from_experts(router_w, experts, top_k, renorm=renorm, router_bias=router_bias, **router)
