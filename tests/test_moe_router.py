"""The second MoE router and the shared experts on the GPU (csrc/moe_route.hip: qpal_moe_route_ex, qpal_moe_combine_shared; DESIGN.md
§36) against the float64 contract of qpalette_amd/moe.py.  The bounds are derived in tests/moe_router_reference.py;
tests/test_moe_router_contract.py asserts on the CPU that the routed inputs are decidable and that the layer tolerance has teeth."""
import ctypes

import numpy as np
import pytest
import torch

import moe_reference as mref
import moe_router_reference as rr
from test_moe import SENTINEL, _check_layout, _cuda, _i, _layer, _wrapped, decoded

pytestmark = pytest.mark.gpu
PAD = 8


@pytest.fixture(scope="module")
def qp():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import qpalette_amd
    qpalette_amd._native.lib()
    return qpalette_amd


OUTPUTS = ("sel", "gate", "order", "inv", "x_index", "group_expert", "group_first", "group_count", "ngroups", "sgate")


def _fenced_workspace(qp, n, E, top_k, H):
    """a workspace whose route outputs each lie inside a buffer of sentinels: PAD words in front, PAD behind"""
    ws = qp.moe.moe_workspace(n, E, top_k, H, 32, "cuda", shared_I=32)
    fences = {}
    for name in OUTPUTS:
        t = getattr(ws, name)
        buf = torch.full((t.numel() + 2 * PAD,), -77 if t.dtype == torch.int32 else SENTINEL, dtype=t.dtype, device="cuda")
        fences[name] = buf
        setattr(ws, name, buf[PAD:PAD + t.numel()].view(t.shape))
    return ws, fences


def _assert_fences(fences):
    for name, buf in fences.items():
        want = -77 if buf.dtype == torch.int32 else SENTINEL
        assert bool((buf[:PAD] == want).all()) and bool((buf[-PAD:] == want).all()), name


def _router_cuda(qp, router):
    return router._replace(select_bias=_cuda(router.select_bias), shared_gate=_cuda(router.shared_gate))


def _route_ex(qp, inp, router, top_k, n, E, bias=None):
    ws, fences = _fenced_workspace(qp, n, E, top_k, inp["h"].shape[1])
    qp.moe.route(_cuda(inp["h"]), (inp["eps"], _cuda(inp["rms_w"])), _cuda(inp["router_w"]), _cuda(bias), top_k, None, ws,
                 active=_cuda(inp.get("active")), router=_router_cuda(qp, router))
    torch.cuda.synchronize()
    assert int(ws.ticket[0]) == 0   # the ticket is left as it was found
    _assert_fences(fences)
    return ws


# --------------------------------------------------------------------------------------------------------------------- route_ex
@pytest.mark.parametrize("variant", rr.VARIANTS, ids=lambda v: "-".join(str(x) for x in v))
@pytest.mark.parametrize("case", rr.CASES, ids=lambda c: "x".join(str(x) for x in c))
def test_route_ex(qp, case, variant):
    n, H, E, top_k, G, tg = case
    inp, router, rt, b = rr.world(case, variant)
    ok = rr.decidable_rows(rt, b, top_k, router, inp["active"])
    assert 1.0 - ok.mean() <= rr.UNDECIDABLE_CAP
    ws = _route_ex(qp, inp, router, top_k, n, E)
    sel, gate, sgate = _i(ws.sel), ws.gate.cpu().numpy().astype(np.float64), ws.sgate.cpu().numpy().astype(np.float64)
    assert np.array_equal(sel[ok], rt["sel"][ok])
    off = inp["active"] < 0
    assert (sel[off] == -1).all() and (gate[off] == 0).all() and (sgate[off] == 0).all()
    assert (np.diff(sel[~off], axis=1) > 0).all() and (sel[~off] >= 0).all() and (sel[~off] < E).all()   # ascending ids, every row
    err, tol = np.abs(gate - rt["gate"])[ok], rr.gate_tolerance(rt, b, router)[ok]
    serr, stol = np.abs(sgate - rt["sgate"]), rr.shared_gate_tolerance(rt, inp["shared_gate"])
    print(f"gate: max err / tol {(err[tol > 0] / tol[tol > 0]).max():.3f}; shared gate: {(serr / stol).max():.3f}")
    assert (err <= tol).all()
    assert (serr <= stol).all()
    _check_layout(qp, ws, E)
    # without a shared gate the shared expert counts in full: exactly 1.0 on the live rows
    ws = _route_ex(qp, inp, router._replace(shared_gate=None), top_k, n, E)
    assert np.array_equal(ws.sgate.cpu().numpy(), (~off).astype(np.float32))
    assert np.array_equal(_i(ws.sel), sel)


def _tie_inputs(n, H, E, seed=11):
    rng = np.random.default_rng(seed)
    return dict(h=rng.standard_normal((n, H)).astype(np.float32), rms_w=(1 + 0.3 * rng.standard_normal(H)).astype(np.float16),
                router_w=(rng.standard_normal((E, H)) / np.sqrt(H)).astype(np.float16), eps=1e-5, active=np.arange(n, dtype=np.int64))


@pytest.mark.parametrize("scoring", ["softmax", "sigmoid"])
def test_route_ex_tie_rules(qp, scoring):
    """equal router rows give bitwise equal keys: the lower expert id, the lower group id, on both sides of the lane 63 / 64 border"""
    R = qp.moe.Router
    n, H = 9, 160
    # duplicate rows inside one group (S = 4: lane walk): group 0 wins, expert 0 takes the first place, the twins 1 and 3 tie
    inp = _tie_inputs(n, H, 8)
    inp["router_w"][3] = inp["router_w"][1]
    sb = np.array([10, 0, -10, 0, -10, -10, -10, -10], dtype=np.float32)
    ws = _route_ex(qp, inp, R(scoring, sb, 2, 1, "max", True, 1.0, None), 2, n, 8)
    assert (_i(ws.sel) == np.array([0, 1])).all()
    _check_layout(qp, ws, 8)
    # both twins chosen: equal scores, bit for bit, the bias in neither
    sb = np.array([-10, 0, -10, 3, -10, -10, -10, -10], dtype=np.float32)
    ws = _route_ex(qp, inp, R(scoring, sb, 2, 1, "max", False, 2.0, None), 2, n, 8)
    assert (_i(ws.sel) == np.array([1, 3])).all()
    g = ws.gate.cpu().numpy().view(np.uint32)
    assert np.array_equal(g[:, 0], g[:, 1])
    # two groups with identical member rows (S = 2): the lower group, by its maximum and by the sum of its two best
    inp = _tie_inputs(n, H, 8)
    inp["router_w"][4:6] = inp["router_w"][0:2]
    sb = np.array([0, 0, -10, -10, 0, 0, -10, -10], dtype=np.float32)
    for gs in ("max", "top2"):
        ws = _route_ex(qp, inp, R(scoring, sb, 4, 1, gs, True, 1.0, None), 2, n, 8)
        assert (_i(ws.sel) == np.array([0, 1])).all(), gs
    # the same with groups of 64 (wave reductions): group 1 = experts 64 .. 127 repeats group 0
    inp = _tie_inputs(n, H, 128)
    inp["router_w"][64:] = inp["router_w"][:64]
    for gs in ("max", "top2"):
        ws = _route_ex(qp, inp, R(scoring, None, 2, 1, gs, True, 1.0, None), 4, n, 128)
        assert (_i(ws.sel) < 64).all() and (_i(ws.sel) >= 0).all(), gs
    # a duplicate pair on lanes 63 / 64 (registers 0 and 1): expert 5 first, then the twins tie
    inp = _tie_inputs(n, H, 128)
    inp["router_w"][64] = inp["router_w"][63]
    sb = np.full(128, -10, dtype=np.float32)
    sb[5], sb[63], sb[64] = 10, 0, 0
    ws = _route_ex(qp, inp, R(scoring, sb, 1, 1, "max", True, 1.0, None), 2, n, 128)
    assert (_i(ws.sel) == np.array([5, 63])).all()
    ws = _route_ex(qp, inp, R(scoring, sb, 2, 2, "top2", False, 1.0, None), 3, n, 128)
    assert (_i(ws.sel) == np.array([5, 63, 64])).all()
    g = ws.gate.cpu().numpy().view(np.uint32)
    assert np.array_equal(g[:, 1], g[:, 2])
    _check_layout(qp, ws, 128)


def test_route_ex_argument_errors(qp):
    lib, buf = qp._native.lib(), torch.zeros(1 << 14, dtype=torch.int32, device="cuda")
    q = [buf.data_ptr() + 4096 * i for i in range(16)]   # a region of 1024 words for every argument: the two good calls launch
    p = q[0]
    MR = qp._native.MoeRouter

    def call(rt, n=4, H=64, E=8, k=2, mg=16):
        return lib.qpal_moe_route_ex(q[0], H, q[1], 1e-5, q[2], None, None, n, H, E, k, q[3], q[4], q[5], q[6], q[7], q[8], q[9], q[10],
                                     q[11], mg, q[12], None if rt is None else ctypes.byref(rt), None)
    assert call(MR(0, 1, 1, 0, 1, 1.0, None, None, None)) == 0
    assert call(MR(1, 4, 2, 1, 1, 2.5, q[13], q[14], q[15])) == 0
    torch.cuda.synchronize()
    assert int(buf[12 * 1024]) == 0                       # (the ticket is zero again)
    assert call(None) == -3
    assert call(MR(0, 3, 1, 0, 1, 1.0, None, None, None)) == -1                 # E % n_group
    assert call(MR(0, 4, 0, 0, 1, 1.0, None, None, None)) == -1                 # topk_group < 1
    assert call(MR(0, 4, 5, 0, 1, 1.0, None, None, None)) == -1                 # topk_group > n_group
    assert call(MR(0, 4, 1, 0, 1, 1.0, None, None, None), k=3) == -1            # topk_group * S < top_k
    assert call(MR(0, 8, 4, 1, 1, 1.0, None, None, None)) == -1                 # "top2" with S = 1
    assert call(MR(0, 0, 1, 0, 1, 1.0, None, None, None)) == -1
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        assert call(MR(0, 1, 1, 0, 1, scale, None, None, None)) == -2
    assert call(MR(2, 1, 1, 0, 1, 1.0, None, None, None)) == -2 and call(MR(0, 1, 1, 2, 1, 1.0, None, None, None)) == -2
    assert call(MR(0, 1, 1, 0, 1, 1.0, None, p, None)) == -3                    # a shared gate without its output
    assert call(MR(0, 1, 1, 0, 1, 1.0, None, p + 8, p)) == -4 and call(MR(0, 1, 1, 0, 1, 1.0, p + 2, None, None)) == -4
    # the limits of qpal_moe_route stay
    ok = MR(0, 1, 1, 0, 1, 1.0, None, None, None)
    assert call(ok, mg=1) == -1 and call(ok, H=60) == -1 and call(ok, k=9) == -1 and call(ok, n=129, mg=300) == -1
    assert call(ok, E=257, mg=300) == -1 and call(ok, H=8200) == -1
    torch.cuda.synchronize()
    ws = qp.moe.moe_workspace(4, 8, 2, 64, 32, "cuda")
    h, w = torch.zeros(4, 64, device="cuda"), torch.zeros(8, 64, dtype=torch.float16, device="cuda")
    with pytest.raises(qp._native.QpalError, match="n_group"):
        qp.moe.route(h, (1e-5, None), w, None, 2, None, ws, router=qp.moe.Router(n_group=3))
    with pytest.raises(qp._native.QpalError, match="somewhere to put"):
        qp.moe.route(h, (1e-5, None), w, None, 2, None, ws, router=qp.moe.Router(shared_gate=w[0]))


@pytest.mark.parametrize("case", mref.ROUTE_CASES)
def test_route_ex_neutral_is_the_first_router(qp, case):
    """softmax, no select bias, one group, scale 1: qpal_moe_route's sel on every decidable row, and its gates bit for bit"""
    n, H, E, top_k = case
    for bias, renorm in ((False, True), (True, False)):
        inp = mref.route_inputs(n, H, E, top_k, mref.ROUTE_SEEDS[case], bias)
        old = qp.moe.moe_workspace(n, E, top_k, H, 32, "cuda")
        qp.moe.route(_cuda(inp["h"]), (inp["eps"], _cuda(inp["rms_w"])), _cuda(inp["router_w"]), _cuda(inp["bias"]), top_k, renorm, old,
                     active=_cuda(inp["active"]))
        new = _route_ex(qp, inp, qp.moe.Router(renorm=renorm), top_k, n, E, bias=inp["bias"])
        rt = qp.moe.reference_route(inp["h"], inp["rms_w"], inp["eps"], inp["router_w"], inp["bias"], top_k, renorm, inp["active"])
        ok = mref.decidable_rows(rt, mref.logit_bounds(rt, inp["router_w"]), top_k, inp["active"])
        assert np.array_equal(_i(new.sel)[ok], _i(old.sel)[ok])
        same = (_i(new.sel) == _i(old.sel)).all(axis=1)
        assert np.array_equal(new.gate.cpu().numpy().view(np.uint32)[same], old.gate.cpu().numpy().view(np.uint32)[same])


# -------------------------------------------------------------------------------------------------------------- combine_shared
@pytest.mark.parametrize("accumulate", [False, True])
def test_combine_shared(qp, accumulate):
    """bit for bit reference_combine_shared: a row with sgate == 0 whose ys is NaN, rows without a routed pair (with and without
    a shared term), H with a partial last block"""
    rng = np.random.default_rng(9)
    n, top_k, H, E = 9, 2, 200, 4
    sel = np.stack([np.sort(rng.permutation(E)[:top_k]) for _ in range(n)])
    sel[[2, 6]] = -1
    lay = qp.moe.reference_layout(sel, E)
    P = n * top_k
    y = rng.standard_normal((P, H)).astype(np.float32)
    gate = rng.uniform(0.05, 1.0, size=(n, top_k)).astype(np.float32)
    ys = rng.standard_normal((n, H)).astype(np.float32)
    sgate = rng.uniform(0.05, 1.0, size=n).astype(np.float32)
    sgate[[2, 4]] = 0.0          # row 2: no routed pair and no shared term; row 4: routed pairs only
    ys[[2, 4]] = np.nan          # what an inactive slot left behind
    base = rng.standard_normal((n, H)).astype(np.float32)   # row 6: no routed pair, the term is the shared expert's alone
    out = torch.full((n + 2, H + 8), SENTINEL, dtype=torch.float32, device="cuda")
    out[:n, :H] = _cuda(base)
    qp.moe.combine(out[:n, :H], _cuda(y), _cuda(gate), _cuda(lay["inv"].astype(np.int32)), accumulate=accumulate,
                   shared=(_cuda(ys), _cuda(sgate)))
    want = qp.moe.reference_combine_shared(base, y, gate, lay["inv"], ys, sgate, accumulate)
    got = out.cpu().numpy()
    assert np.array_equal(got[:n, :H].view(np.uint32), want.view(np.uint32))
    assert (got[n:] == SENTINEL).all() and (got[:, H:] == SENTINEL).all()
    assert np.array_equal(got[2, :H], base[2] if accumulate else np.zeros(H, dtype=np.float32))
    assert np.isfinite(got[:n, :H]).all()
    lib, p = qp._native.lib(), out.data_ptr()
    assert lib.qpal_moe_combine_shared(p, H, p, H, p, p, None, H, p, n, top_k, H, P, 1, None) == -3
    assert lib.qpal_moe_combine_shared(p, H, p, H, p, p, p, H, None, n, top_k, H, P, 1, None) == -3
    assert lib.qpal_moe_combine_shared(p, H, p, H, p, p, p, H - 1, p, n, top_k, H, P, 1, None) == -1
    assert lib.qpal_moe_combine_shared(p, H, p, H, p, p, p + 2, H, p, n, top_k, H, P, 1, None) == -4
    assert lib.qpal_moe_combine_shared(p, H, p, H, p, p, p, H, p, n, 9, H, P, 1, None) == -1


# ---------------------------------------------------------------------------------------------------------------------- MoEMLP
def shared_mlp(qp, H, Is, su_ug=None, seed=900, q_ug="tcq_6_none_0.9", q_dp="tcomb_6_7_0.5_none_0.9"):
    """the shared expert of moe_router_reference.cpu_shared on the GPU: an IncoherentMLP of three wrapped dummy layers"""
    rng = np.random.default_rng(seed)
    own_ug, su_dp = (rng.integers(0, 2, H) * 2.0 - 1).astype(np.float16), (rng.integers(0, 2, Is) * 2.0 - 1).astype(np.float16)
    su_ug = own_ug if su_ug is None else su_ug
    up, gt, dn = _wrapped(qp, H, Is, q_ug, seed + 1, su_ug), _wrapped(qp, H, Is, q_ug, seed + 2, su_ug), _wrapped(qp, Is, H, q_dp, seed + 3, su_dp)
    mlp = qp.linear.IncoherentMLP(H, Is, "silu")
    mlp.up_proj, mlp.gate_proj, mlp.down_proj = up.linear, gt.linear, dn.linear
    mlp = mlp.cuda()
    mlp.SU_ug.data.copy_(up.SU), mlp.SU_dp.data.copy_(dn.SU)
    mlp.Wscale_ug.data.copy_(torch.cat([up.Wscale, gt.Wscale])), mlp.Wscale_dp.data.copy_(dn.Wscale)
    mlp.scale = up.scale
    qp.linear.share_codebooks([mlp.up_proj, mlp.gate_proj, mlp.down_proj])
    return mlp, su_ug, su_dp


def shared_decoded(mlp):
    ws = (mlp.Wscale_ug[:mlp.intermediate_size], mlp.Wscale_ug[mlp.intermediate_size:], mlp.Wscale_dp)
    return [l.get_weight().double().cpu().numpy() * w.double().cpu().numpy()[:, None] * mlp.scale
            for l, w in zip((mlp.up_proj, mlp.gate_proj, mlp.down_proj), ws)]


LAYER_ROUTERS = {   # name: (Router fields without the tensors, select bias, gated, the shared expert reads the experts' rows)
    "deepseek_v3_gated": (("sigmoid", 4, 2, "top2", True, 2.5), True, True, False),
    "deepseek_v2_ungated": (("softmax", 4, 2, "max", False, 2.5), False, False, True),
}


@pytest.mark.parametrize("name", sorted(LAYER_ROUTERS))
def test_moemlp_forward_with_a_shared_expert(qp, name, monkeypatch):
    """E = 8, H = 512, I = Is = 512: within KAPPA x the emulation's distance of the float64 layer (moe_router_reference.layer_judge_ex)
    on the decidable rows; the shared expert that shares SU_ug and the scale skips its first rotation, counted launch by launch"""
    (scoring, G, tg, gs, renorm, rscale), biased, gated, same_su = LAYER_ROUTERS[name]
    E, H, I, top_k, n = 8, 512, 512, 2, 9
    experts, router_w, su_ug, su_dp = _layer(qp, E=E, H=H, I=I)
    if scoring == "sigmoid":
        router_w = router_w / 4      # (exact in fp16) N(0, 1) / sqrt(H): 4 / sqrt(H) saturates a sigmoid
    mlp, s_ug, s_dp = shared_mlp(qp, H, 512, su_ug=su_ug if same_su else None)
    rng = np.random.default_rng(1)
    h = rng.standard_normal((n, H)).astype(np.float32)
    rms_w = (1 + 0.3 * rng.standard_normal(H)).astype(np.float16)
    sb = (0.1 * rng.standard_normal(E)).astype(np.float32) if biased else None
    sg = (rng.standard_normal(H) / np.sqrt(H)).astype(np.float16) if gated else None
    active = np.arange(n, dtype=np.int64)
    active[4] = -1
    layer = qp.MoEMLP.from_experts(router_w, experts, top_k, renorm=renorm, scoring=scoring, select_bias=_cuda(sb), n_group=G,
                                   topk_group=tg, group_score=gs, routed_scale=rscale, shared=mlp, shared_gate=_cuda(sg))
    assert layer.shared_x16 == same_su and layer.launches(n) == (9 if same_su else 10)
    counts = {"rotate": 0, "multi_gemv": 0, "moe_gemv": 0, "route": 0, "combine": 0}

    def counted(mod, fn):
        real = getattr(mod, fn)

        def wrapper(*a, **kw):
            counts[fn] += 1
            return real(*a, **kw)
        monkeypatch.setattr(mod, fn, wrapper)
    counted(qp.moe.had, "rotate"), counted(qp.moe.linear, "multi_gemv")
    for fn in ("moe_gemv", "route", "combine"):
        counted(qp.moe, fn)
    got = layer(_cuda(h), (1e-5, _cuda(rms_w)), active=_cuda(active)).cpu().numpy().astype(np.float64)
    assert counts == {"rotate": 3 if same_su else 4, "multi_gemv": 2, "moe_gemv": 2, "route": 1, "combine": 1}
    assert sum(counts.values()) == layer.launches(n)
    assert (got[4] == 0).all()
    router = qp.moe.Router(scoring, sb, G, tg, gs, renorm, rscale, sg)
    rw = router_w.cpu().numpy()
    rt = qp.moe.reference_route_ex(h, rms_w, 1e-5, rw, None, top_k, router, active)
    ok = rr.decidable_rows(rt, rr.bounds(rt, rw, router), top_k, router, active) & (active >= 0)
    assert ok.sum() >= 6
    ws = layer.workspace(n)
    assert np.array_equal(_i(ws.sel)[ok], rt["sel"][ok])
    world = (decoded(experts), su_ug, su_dp, experts[0][0].scale, shared_decoded(mlp), s_ug, s_dp, mlp.scale)
    f, rows = rr.layer_judge_ex(world, rt, ok, got)
    print(f"MoEMLP.forward ({name}): max distance / tolerance {f.max():.3f}")
    assert (f <= 1.0).all()


def test_default_moemlp_is_the_old_launches_bit_for_bit(qp):
    """a MoEMLP built with the first router's arguments: no Router record, six launches, and its output bitwise that of
    qpal_moe_route and qpal_moe_combine called directly around the same routed launches"""
    E, H, I, top_k, n = 4, 256, 512, 2, 9
    experts, router_w, su_ug, su_dp = _layer(qp)
    layer = qp.MoEMLP.from_experts(router_w, experts, top_k, renorm=True)
    assert layer.router is None and layer.shared is None and layer.launches(n) == 6
    rng = np.random.default_rng(1)
    h = _cuda(rng.standard_normal((n, H)).astype(np.float32))
    rms = (1e-5, _cuda((1 + 0.3 * rng.standard_normal(H)).astype(np.float16)))
    active = np.arange(n, dtype=np.int64)
    active[4] = -1
    active = _cuda(active)
    got = layer(h, rms, active=active)
    lib, moe, had = qp._native.lib(), qp.moe, qp.hadamard
    ws = moe.moe_workspace(n, E, top_k, H, I, "cuda")
    assert ws.sgate is None and ws.ys32 is None
    had.rotate(h, hadK=layer.had_left_ug_T, K=layer.hidden_K, su=layer.SU_ug, post_scale=1.0 / layer.scale, rms=rms, in_mode=had.IN_F32, out=ws.x16)
    rc = lib.qpal_moe_route(h.data_ptr(), h.stride(0), rms[1].data_ptr(), 1e-5, layer.router_w.data_ptr(), None, active.data_ptr(), n, H, E,
                            top_k, 1, ws.sel.data_ptr(), ws.gate.data_ptr(), ws.order.data_ptr(), ws.inv.data_ptr(), ws.x_index.data_ptr(),
                            ws.group_expert.data_ptr(), ws.group_first.data_ptr(), ws.group_count.data_ptr(), ws.ngroups.data_ptr(),
                            ws.group_expert.numel(), ws.ticket.data_ptr(), None)
    assert rc == 0
    table = (ws.group_expert, ws.group_first, ws.group_count, ws.ngroups)
    moe.moe_gemv(ws.ug32, [layer.p_up, layer.p_gate], ws.x16, layer.tlut, *table, x_index=ws.x_index, oscale=layer.scale)
    had.rotate(ws.ug32, in_mode=had.IN_SWIGLU_F32, hadK=layer.had_left_dp_T, K=layer.inter_K, su=layer.SU_dp, post_scale=1.0 / layer.scale,
               out=ws.act16)
    moe.moe_gemv(ws.y32, [layer.p_down], ws.act16, layer.tlut, *table, oscale=layer.scale)
    out = torch.empty_like(h)
    rc = lib.qpal_moe_combine(out.data_ptr(), out.stride(0), ws.y32.data_ptr(), ws.y32.stride(0), ws.gate.data_ptr(), ws.inv.data_ptr(), n,
                              top_k, H, ws.y32.shape[0], 0, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), out.view(torch.int32))
    mine = layer.workspace(n)
    assert torch.equal(mine.sel, ws.sel) and torch.equal(mine.gate.view(torch.int32), ws.gate.view(torch.int32))


def test_moemlp_refuses(qp):
    experts, router_w, su_ug, su_dp = _layer(qp, E=4, H=128, I=128)
    mlp, _, _ = shared_mlp(qp, 128, 256)
    qp.MoEMLP.from_experts(router_w, experts, 2, shared=mlp)
    with pytest.raises(qp._native.QpalError, match="n_group"):
        qp.MoEMLP.from_experts(router_w, experts, 2, n_group=3)
    with pytest.raises(qp._native.QpalError, match="fewer than top_k"):
        qp.MoEMLP.from_experts(router_w, experts, 2, n_group=4, topk_group=1)
    with pytest.raises(qp._native.QpalError, match="routed_scale"):
        qp.MoEMLP.from_experts(router_w, experts, 2, routed_scale=0.0)
    with pytest.raises(qp._native.QpalError, match="shared_gate= gates a shared expert"):
        qp.MoEMLP.from_experts(router_w, experts, 2, shared_gate=torch.zeros(128))
    with pytest.raises(qp._native.QpalError, match="select_bias must be"):
        qp.MoEMLP.from_experts(router_w, experts, 2, select_bias=torch.zeros(5))
    other, _, _ = shared_mlp(qp, 256, 256)
    with pytest.raises(qp._native.QpalError, match="IncoherentMLP of hidden width 128"):
        qp.MoEMLP.from_experts(router_w, experts, 2, shared=other)


def test_quantize_experts_with_a_shared_expert(qp):
    """quantize_experts(shared=...) quantises the shared expert like a dense MLP (sign vectors of its own) and builds a layer that
    follows the contract on its own decoded weights"""
    E, H, I, Is, top_k, n = 4, 256, 512, 256, 2, 5
    g = torch.Generator().manual_seed(0)
    ups, gates = ([torch.randn(I, H, generator=g).cuda() / 16 for _ in range(E)] for _ in range(2))
    downs = [torch.randn(H, I, generator=g).cuda() / 22 for _ in range(E)]
    shared = (torch.randn(Is, H, generator=g).cuda() / 16, torch.randn(Is, H, generator=g).cuda() / 16, torch.randn(H, Is, generator=g).cuda() / 16)
    router_w = torch.randn(E, H, generator=g).cuda() / 16
    sg = (torch.randn(H, generator=g) / 16).half()
    cb = {9: torch.randn(512, 2, generator=g).half()}
    layer = qp.quantize_experts(router_w, ups, gates, downs, ("tcq_8_none_0.9", "tcq_8_none_0.9", "tcomb_7_8_0.5_none_0.9"), top_k, codebooks=cb,
                                shared=shared, scoring="sigmoid", n_group=2, topk_group=1, group_score="top2", routed_scale=2.0,
                                shared_gate=sg.cuda())
    assert layer.shared.intermediate_size == Is and not layer.shared_x16 and layer.launches(n) == 10
    h = torch.randn(n, H, generator=g).cuda()
    got = layer(h, (1e-5, torch.ones(H, dtype=torch.float16, device="cuda"))).cpu().numpy().astype(np.float64)
    router = qp.moe.Router("sigmoid", None, 2, 1, "top2", True, 2.0, sg.numpy())
    rw = layer.router_w.cpu().numpy()
    rt = qp.moe.reference_route_ex(h.cpu().numpy(), np.ones(H), 1e-5, rw, None, top_k, router)
    ok = rr.decidable_rows(rt, rr.bounds(rt, rw, router), top_k, router)
    assert ok.sum() >= 3
    assert np.array_equal(_i(layer.workspace(n).sel)[ok], rt["sel"][ok])
    sh = layer.shared
    world = (decoded(layer.experts), layer.SU_ug.cpu().numpy(), layer.SU_dp.cpu().numpy(), layer.scale, shared_decoded(sh),
             sh.SU_ug.cpu().numpy(), sh.SU_dp.cpu().numpy(), sh.scale)
    f, _ = rr.layer_judge_ex(world, rt, ok, got)
    print(f"quantize_experts layer with a shared expert: max distance / tolerance {f.max():.3f}")
    assert (f <= 1.0).all()
