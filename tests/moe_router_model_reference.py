"""model_reference's small model with sparse layers of the second router and shared experts: the float64 forward and its emulation
(tests/test_moe_router_model.py, tests/test_moe_router_contract.py).  The dense part is
moe_model_reference.forward's, restated; a sparse layer is moe_router_reference.layer_forward_ex on the rows of the slot.

Layer 0: sigmoid scores, a select bias, 4 groups of which the 2 best by "top2" are allowed, renormalised gates times 2.5, a gated
shared expert with sign vectors of its own (DeepSeek-V3's shape).  Layer 1: dense.  Layer 2: softmax scores, the 2 best of 4 groups
by their maximum, gates not renormalised, times 2.5, an ungated shared expert that reads the experts' rotated rows (DeepSeek-V2's).

A (slot, position) is ROUTING-UNDECIDABLE if in any sparse layer the float64 forward's routing is not decidable by
moe_router_reference.decidable_rows with, as every key's bound, 4 x the emulation's largest deviation of a score on the token set:
absolute for sigmoid scores, relative to the score for softmax ones (their error is a factor), and the group bounds that follow
from it; every later position of its slot is undecidable with it, because its keys and values are read by them."""
import functools
import math
import types

import numpy as np
import torch

import attn_reference as ar
import model_reference as mr
import moe_reference as mref
import moe_router_reference as rr
from moe_model_reference import CAL_RATIO, E, I, NL, SPARSE, TOP_K, tokens  # noqa: F401
from qpalette_amd import moe

DEFECTS = rr.DEFECTS
IS = 512
# layer: (scoring, n_group, topk_group, group_score, renorm, select bias, gated, the shared expert shares SU_ug)
ROUTERS = {0: ("sigmoid", 4, 2, "top2", True, True, True, False), 2: ("softmax", 4, 2, "max", False, False, False, True)}
# name: (seed, tokens per slot, prefill emulation) — the first seeds counted up from 41 whose sets meet both caps on undecidable rows
# (tests/test_moe_router_contract.py asserts it; 41, 42 and 41 .. 51 miss one of them)
TOKEN_SETS = {"decode": (43, (9, 7, 0, 8), False), "prefill": (52, (12, 10, 5), True)}


def forward(model, sparse, tokens_per_slot, emu=False, chunk=16, prefill=False, kv_dtype=None, mutate=None, context=None):
    """moe_model_reference.forward with the sparse layers of the second router.  -> model_reference.Out plus .router {layer: [per
    slot the reference_route_ex dict of its rows]}.  sparse: {layer: namespace(world = moe_router_reference.layer_forward_ex's
    eight, router_w, router)}; mutate = (one of moe_router_reference.DEFECTS, layer)."""
    geo, dev = model.geo, model.embed.device
    H, nq, nkv, hd = geo["H"], geo["nq"], geo["nkv"], geo["hd"]
    B, L = len(tokens_per_slot), len(model.layers)
    scale = 1.0 / math.sqrt(hd)
    f16, f32 = mr.f16, mr.f32
    toks = [torch.as_tensor(t, dtype=torch.long, device=dev).reshape(-1) for t in tokens_per_slot]
    ctx = context or max(1, max(int(t.shape[0]) for t in toks))
    h = [model.embed[t] for t in toks]
    if emu:
        h = [f32(x) for x in h]
    out = mr.Out()
    out.stream, out.router = [[] for _ in range(B)], {i: [None] * B for i in sparse}
    ratios = torch.zeros(L, 2, dtype=torch.float64)

    def cache_image(t):
        if kv_dtype == ar.F8:
            return ar.to_cache(t.float(), ar.F8).float().double()
        return f16(t) if emu else t

    def apply(lin, x):
        if not emu:
            return x @ lin.eff().T
        xr = f16(f16(mr.rot(x * lin.su, lin.hadk)) / mr.SCALE)
        return f32((xr @ lin.What.T) * (lin.wscale * mr.SCALE))

    for i, layer in enumerate(model.layers):
        eps = model.eps_layer
        sq = torch.zeros(4, dtype=torch.float64)
        for b in range(B):
            N = toks[b].shape[0]
            if N == 0:
                continue
            Kc = torch.zeros(nkv, ctx, hd, dtype=torch.float64, device=dev)
            Vc = torch.zeros(nkv, ctx, hd, dtype=torch.float64, device=dev)
            x = mr._rms_norm(h[b], layer["ln1"], eps, emu)
            q, k, v = (apply(layer[name], x) for name in ("q", "k", "v"))
            a = torch.zeros(N, H, dtype=torch.float64, device=dev)
            for c0 in range(0, N, chunk):
                n = min(chunk, N - c0)
                pos = torch.arange(c0, c0 + n, device=dev)
                rows = slice(c0, c0 + n)
                qi, ki, vi = q[rows].reshape(n, nq, hd), k[rows].reshape(n, nkv, hd), v[rows].reshape(n, nkv, hd)
                if emu:
                    qr = ar.rope_f16(qi.float(), pos[:, None], model.inv_freq).double()
                    kr = ar.rope_f16(ki.float(), pos[:, None], model.inv_freq).double()
                else:
                    qr, kr = mr._rope(qi, pos, model.inv_freq), mr._rope(ki, pos, model.inv_freq)
                Kc[:, pos] = cache_image(kr).transpose(0, 1)
                Vc[:, pos] = cache_image(vi).transpose(0, 1)
                if emu:
                    fmt = ar.F8 if kv_dtype == ar.F8 else ar.F16
                    a[rows] = ar.emulate(qr.reshape(n, H).half(), Kc.to(fmt) if fmt == ar.F16 else Kc.float().to(fmt),
                                         Vc.to(fmt) if fmt == ar.F16 else Vc.float().to(fmt), (pos + 1).tolist(), nq, nkv, hd, scale,
                                         2.0 ** -11 if prefill else 0.0).double()
                else:
                    a[rows] = mr._attend(qr, Kc, Vc, pos, scale)
            y = apply(layer["o"], a)
            sq[0] += float(y.pow(2).sum())
            sq[1] += float(h[b].pow(2).sum())
            h[b] = f32(h[b] + y) if emu else h[b] + y
        for b in range(B):
            if toks[b].shape[0] == 0:
                out.stream[b].append(h[b])
                continue
            if i in sparse:
                sp = sparse[i]
                rt = moe.reference_route_ex(h[b].cpu().numpy(), layer["ln2"].cpu().numpy(), eps, sp.router_w, None, TOP_K, sp.router)
                out.router[i][b] = rt
                mut = mutate[0] if mutate and mutate[1] == i else None
                y = rr.layer_forward_ex(*sp.world, rt, router=sp.router, emu=emu, mutate=mut)
                y = torch.from_numpy(y).to(dev)
            else:
                x = mr._rms_norm(h[b], layer["ln2"], eps, emu)
                act = torch.nn.functional.silu(apply(layer["gate"], x)) * apply(layer["up"], x)
                y = apply(layer["down"], f16(act) if emu else act)
            sq[2] += float(y.pow(2).sum())
            sq[3] += float(h[b].pow(2).sum())
            h[b] = f32(h[b] + y) if emu else h[b] + y
            out.stream[b].append(h[b])
        ratios[i, 0], ratios[i, 1] = math.sqrt(sq[0] / max(sq[1], 1e-300)), math.sqrt(sq[2] / max(sq[3], 1e-300))
    out.ratios = ratios
    for b in range(B):
        out.stream[b] = torch.stack(out.stream[b])
        xn = mr._rms_norm(h[b], model.norm_w, model.eps_final, emu, two=True)
        lg = xn @ model.lm_head.T
        lg = f32(lg) if emu else lg
        out.normed.append(xn)
        out.logits.append(lg)
        out.logprob.append(torch.log_softmax(lg, dim=-1))
    return out


@functools.lru_cache(maxsize=None)
def world():
    """(spec of the dense model on the CPU, {layer: sparse layer}): moe_model_reference.world's experts (test_moe._layer(seed = 100 +
    layer)) and the shared expert of moe_router_reference.cpu_shared(seed = 900 + layer); every down's Wscale of a sparse layer,
    the shared expert's too, times a power of two so that the layer carries about CAL_RATIO of the stream it is added to"""
    spec = mr.build_spec("S", "mixed", NL, mr.VOCAB, 0, "cpu")
    sparse = {}
    cal = mr.calibration_tokens(mr.VOCAB, 0)
    H = spec.geo["H"]
    for i in SPARSE:
        scoring, G, tg, gs, renorm, biased, gated, same_su = ROUTERS[i]
        What, su_ug, su_dp, scale, router_w, _ = mref.cpu_layer(E=E, H=H, I=I, seed=100 + i)
        Ws, s_ug, s_dp, s_scale = rr.cpu_shared(H=H, Is=IS, seed=900 + i, su_ug=su_ug if same_su else None)
        rng = np.random.default_rng(700 + i)
        if scoring == "sigmoid":
            router_w = (router_w.astype(np.float64) / 4).astype(np.float16)   # N(0, 1) / sqrt(H): exact in fp16
        sb = (0.1 * rng.standard_normal(E)).astype(np.float32) if biased else None
        sg = (rng.standard_normal(H) / np.sqrt(H)).astype(np.float16) if gated else None
        router = moe.Router(scoring, sb, G, tg, gs, renorm, rr.ROUTED_SCALE, sg)
        sparse[i] = types.SimpleNamespace(world=(What, su_ug, su_dp, scale, Ws, s_ug, s_dp, s_scale), router_w=router_w, router=router,
                                          factor=1.0)
        r = float(forward(spec.ref, sparse, cal).ratios[i, 1])
        f = 2.0 ** round(math.log2(CAL_RATIO / r))
        sparse[i].factor = f
        sparse[i].world = ([[up, gt, dn * f] for up, gt, dn in What], su_ug, su_dp, scale, [Ws[0], Ws[1], Ws[2] * f], s_ug, s_dp, s_scale)
    return spec, sparse


def routing_decidable(ref, emu, toks, sparse):
    """{(slot, position): bool} by the module's rule"""
    ok = {(b, p): True for b, t in enumerate(toks) for p in range(len(t))}
    for i in ref.router:
        router = sparse[i].router
        pairs = [(emu.router[i][b], ref.router[i][b]) for b, t in enumerate(toks) if len(t)]
        if router.scoring == "softmax":
            dev = max(float(np.abs(e["score"] / r["score"] - 1.0).max()) for e, r in pairs)
        else:
            dev = max(float(np.abs(e["score"] - r["score"]).max()) for e, r in pairs)
        for b, t in enumerate(toks):
            if not len(t):
                continue
            rt = ref.router[i][b]
            kb = 4.0 * dev * (rt["score"] if router.scoring == "softmax" else np.ones_like(rt["score"]))
            gmax = kb.reshape(len(t), router.n_group, -1).max(-1)
            good = rr.decidable_rows(rt, dict(key=kb, group=gmax if router.group_score == "max" else 2.0 * gmax), TOP_K, router)
            for p in range(len(t)):
                ok[(b, p)] &= bool(good[p])
    for b, t in enumerate(toks):     # a slot's later positions read the keys and values of an undecidable one
        for p in range(1, len(t)):
            ok[(b, p)] &= ok[(b, p - 1)]
    return ok
