"""The mixture-of-experts kernels on the GPU (csrc/moe_route.hip, csrc/moe_gemv.hip), each at the smallest shapes
at which it can still go wrong, against the float64 contract of qpalette_amd/moe.py and the CPU oracle's decode.  The bounds are
derived in tests/moe_reference.py; tests/test_moe_contract.py asserts on the CPU that the routed inputs are decidable."""
import numpy as np
import pytest
import torch

import gemv_reference as gref
import moe_reference as mref

pytestmark = pytest.mark.gpu

GEMV_RTOL_ABS = 1e-5  # times sum |w x|: the project's GEMV bar (tests/test_gpu_parity.py)
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def qp():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import qpalette_amd
    qpalette_amd._native.lib()
    return qpalette_amd


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _i(t):
    return t.cpu().numpy().astype(np.int64)


# ----------------------------------------------------------------------------------------------------------------------- route
def _route(qp, inp, top_k, renorm, n, E):
    ws = qp.moe.moe_workspace(n, E, top_k, inp["h"].shape[1], 32, "cuda")
    qp.moe.route(_cuda(inp["h"]), (inp["eps"], _cuda(inp["rms_w"])), _cuda(inp["router_w"]), _cuda(inp["bias"]), top_k, renorm, ws,
                 active=_cuda(inp["active"]))
    torch.cuda.synchronize()
    assert int(ws.ticket[0]) == 0   # the ticket is left as it was found
    return ws


def _check_layout(qp, ws, E):
    sel = _i(ws.sel)
    lay = qp.moe.reference_layout(sel, E)
    ng = lay["ngroups"]
    assert int(ws.ngroups[0]) == ng
    assert np.array_equal(_i(ws.order), lay["order"]) and np.array_equal(_i(ws.inv), lay["inv"])
    assert np.array_equal(_i(ws.x_index), lay["x_index"])
    for name in ("group_expert", "group_first", "group_count"):
        got = _i(getattr(ws, name))
        assert np.array_equal(got[:ng], lay[name]), name
        assert (got[ng:] == (-1 if name == "group_expert" else 0)).all(), name


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("renorm", [False, True])
@pytest.mark.parametrize("case", mref.ROUTE_CASES)
def test_route(qp, case, renorm, bias):
    n, H, E, top_k = case
    inp = mref.route_inputs(n, H, E, top_k, mref.ROUTE_SEEDS[case], bias)
    rt = qp.moe.reference_route(inp["h"], inp["rms_w"], inp["eps"], inp["router_w"], inp["bias"], top_k, renorm, inp["active"])
    bounds = mref.logit_bounds(rt, inp["router_w"])
    ok = mref.decidable_rows(rt, bounds, top_k, inp["active"])
    assert 1.0 - ok.mean() <= mref.UNDECIDABLE_CAP
    ws = _route(qp, inp, top_k, renorm, n, E)
    sel, gate = _i(ws.sel), ws.gate.cpu().numpy().astype(np.float64)
    assert np.array_equal(sel[ok], rt["sel"][ok])
    off = inp["active"] < 0
    assert (sel[off] == -1).all() and (gate[off] == 0).all()
    assert (np.diff(sel[~off], axis=1) > 0).all() and (sel[~off] >= 0).all() and (sel[~off] < E).all()   # ascending ids, every row
    err, tol = np.abs(gate - rt["gate"])[ok], mref.gate_tolerance(rt, bounds, renorm)[ok]
    print(f"gate: max err / tol {(err / tol).max():.3f}")
    assert (err <= tol).all()
    _check_layout(qp, ws, E)


def test_route_tie_rule(qp):
    """two identical router rows give bitwise equal logits; the lower id is taken when one place is left"""
    rng = np.random.default_rng(11)
    n, H, E = 9, 160, 4
    W = (4.0 / np.sqrt(H) * rng.standard_normal((E, H))).astype(np.float16)
    W[3] = W[1]
    inp = dict(h=rng.standard_normal((n, H)).astype(np.float32), rms_w=(1 + 0.3 * rng.standard_normal(H)).astype(np.float16),
               router_w=W, eps=1e-5, active=np.arange(n, dtype=np.int64))
    # both twins chosen, gates not renormalised: equal logits give equal softmax terms, bit for bit
    inp["bias"] = np.array([-60.0, 0.0, -60.0, 0.0], dtype=np.float32)
    ws = _route(qp, inp, 2, False, n, E)
    assert (_i(ws.sel) == np.array([1, 3])).all()
    g = ws.gate.cpu().numpy().view(np.uint32)
    assert np.array_equal(g[:, 0], g[:, 1])
    # expert 0 takes the first place, the twins tie for the one that is left
    inp["bias"] = np.array([60.0, 0.0, -60.0, 0.0], dtype=np.float32)
    ws = _route(qp, inp, 2, True, n, E)
    assert (_i(ws.sel) == np.array([0, 1])).all()
    _check_layout(qp, ws, E)


def test_route_argument_errors(qp):
    lib, buf = qp._native.lib(), torch.zeros(1 << 14, dtype=torch.int32, device="cuda")
    p = buf.data_ptr()
    args = lambda n, H, E, k, mg: (p, H, p, 1e-5, p, None, None, n, H, E, k, 1, p, p, p, p, p, p, p, p, p, mg, p, None)  # noqa: E731
    assert lib.qpal_moe_route(*args(4, 64, 4, 2, 1)) == -1          # max_groups below the bound
    assert lib.qpal_moe_route(*args(4, 60, 4, 2, 8)) == -1          # H % 8
    assert lib.qpal_moe_route(*args(4, 64, 4, 5, 8)) == -1          # top_k > E
    assert lib.qpal_moe_route(*args(129, 64, 4, 2, 300)) == -1
    a = list(args(4, 64, 4, 2, 8))
    a[0] = None
    assert lib.qpal_moe_route(*a) == -3
    assert lib.qpal_moe_max_groups(128, 64, 8) == qp.moe.max_groups(128, 64, 8) == 184
    assert lib.qpal_moe_max_groups(9, 4, 2) == qp.moe.max_groups(9, 4, 2)
    assert lib.qpal_moe_route_ws_bytes(9, 4, 2) == 16 + 4 * (5 * 18 + 3 * qp.moe.max_groups(9, 4, 2) + 1)


# -------------------------------------------------------------------------------------------------------------------- moe_gemv
E4 = 4
COUNTS = (9, 3, 0, 1)   # rows per expert: a full group of 8 and a second group of one row for expert 0; an expert without rows


def _experts(qp, k, m, qstr, seed, exact, cb_seed=None):
    """E4 random packed experts of one codebook -> (Projection, [W fp16 [m, k]] decoded by the CPU oracle, wscale fp16 [E4, m], tlut)"""
    cb_seed = seed if cb_seed is None else cb_seed
    infos = [gref.exact_info(k, m, qstr, seed + e, codebook_seed=cb_seed) if exact
             else qp.mem_op.dummy_linear_info(k, m, qstr, seed=seed + e, codebook_seed=cb_seed) for e in range(E4)]
    W = [gref.oracle_weight(i) for i in infos]
    rng = np.random.default_rng(seed)
    ws = (2.0 ** rng.integers(-1, 2, size=(E4, m)) if exact else rng.uniform(0.5, 2.0, size=(E4, m))).astype(np.float16)
    two = "trellis1" in infos[0]
    s1 = [(i["trellis1"] if two else i["trellis"]).cuda() for i in infos]
    s2 = [i["trellis2"].cuda() for i in infos] if two else None
    kv = infos[0]["KV"]
    proj = qp.moe.Projection(s1, s2, [_cuda(w) for w in ws], m, k, kv[0] if two else kv, kv[1] if two else 0)
    return proj, W, ws, infos[0]["tlut"].cuda()


def _table(lay):
    return [_cuda(lay[n].astype(np.int32)) for n in ("group_expert", "group_first", "group_count")] + \
           [torch.tensor([lay["ngroups"]], dtype=torch.int32, device="cuda")]


def _run_gemv(qp, projs, x, tlut, table, x_index, P, oscale, width):
    out = torch.full((P + 3, width + 8), SENTINEL, dtype=torch.float32, device="cuda")   # rows and columns nobody may write
    if x_index is not None and x_index.numel() < P + 3:   # (one entry per row of out, as the route's workspace holds them)
        x_index = torch.cat([x_index, torch.full((P + 3 - x_index.numel(),), -1, dtype=torch.int32, device="cuda")])
    qp.moe.moe_gemv(out, projs, x, tlut, *table, x_index=x_index, oscale=oscale)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _gemv_case(qp, oracle, k, m, qstr, nproj, indexed, exact, seed):
    n = sum(COUNTS)
    sel = np.repeat(np.arange(E4), COUNTS)[np.random.default_rng(seed).permutation(n)].reshape(n, 1)
    lay = qp.moe.reference_layout(sel, E4)
    P = n
    made = [_experts(qp, k, m, qstr, seed + 10 * j, exact, cb_seed=seed) for j in range(nproj)]
    projs, tlut = [t[0] for t in made], made[0][3]
    for t in made[1:]:
        assert torch.equal(t[3], tlut)
    xs = gref.exact_x(n, k, seed) if exact else np.random.default_rng(seed + 1).standard_normal((n, k)).astype(np.float16)
    xi = lay["x_index"][:P]
    x_dev = _cuda(xs if indexed else xs[xi])       # identity: the caller has gathered the rows into sorted order
    oscale = 2.0 if exact else 3.0
    if exact:   # Wscale in {1/2, 1, 2}, oscale 2: the sum grows by up to 4, the step shrinks by no less than 1
        gref.assert_budget(k, xmax=3.0, scale_max=2.0 * oscale, scale_min=0.5 * oscale)
    got = _run_gemv(qp, projs, x_dev, tlut, _table(lay), _cuda(xi.astype(np.int32)) if indexed else None, P, oscale, nproj * m)
    assert (got[P:] == SENTINEL).all() and (got[:, nproj * m:] == SENTINEL).all()
    for j, (_, W, ws, _) in enumerate(made):
        for pos in range(P):
            e, r = int(sel[lay["order"][pos], 0]), int(xi[pos])
            ref, mag = oracle.gemv(W[e], xs[r:r + 1])
            scale = ws[e].astype(np.float64) * oscale
            want, y = ref[0] * scale, got[pos, j * m:(j + 1) * m].astype(np.float64)
            if exact:
                assert np.array_equal(y, want), (j, pos, gref.describe_difference(y[None], want[None]))
            else:
                tol = GEMV_RTOL_ABS * mag[0] * scale + 2.0 ** -22 * np.abs(want) + 1e-30
                assert (np.abs(y - want) <= tol).all(), (j, pos, float((np.abs(y - want) / tol).max()))
    return got, projs, x_dev, tlut, lay, xi, oscale


CODECS = ["tcq_2_none_0.9", "tcq_5_none_0.9", "tcq_8_none_0.9", "tcomb_3_4_0.5_none_0.9", "tcomb_6_7_0.5_none_0.9"]


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    return o


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("qstr", CODECS)
def test_moe_gemv(qp, oracle, qstr, exact):
    """every shape of the issue's list: k with a partial last step (160), split streams of 1.5 steps each (384), m of one and of
    three supertile rows, one and two projections, x through x_index and in place"""
    ks = (128, 384) if "tcomb" in qstr else (128, 160, 384)
    seed = 0
    for k in ks:
        for m, nproj, indexed in ((32, 1, True), (96, 2, True), (96, 1, False), (32, 2, False)):
            seed += 1
            _gemv_case(qp, oracle, k, m, qstr, nproj, indexed, exact, 100 * CODECS.index(qstr) + seed)
    # K cut into parts that a row's lead wave sums through LDS (moe_gemv.hip: 2 parts from 8 steps a row, 4 from 16): 8 steps, 16
    # steps, and 17 / 18 steps with a partial last one, where the parts are unequal (4 + 4 + 4 + 5; split: 4 + 5 + 4 + 5, stream 2
    # beginning with part 2).  With 32 + 32 rows and 4 rows a pass the second projection begins inside a workgroup's second pass.
    for k, m, nproj, indexed in ((1024, 32, 2, True), (2048, 32, 1, False), (2112, 32, 2, True)):
        seed += 1
        _gemv_case(qp, oracle, k, m, qstr, nproj, indexed, exact, 100 * CODECS.index(qstr) + seed)


@pytest.mark.parametrize("qstr", ["tcq_5_none_0.9", "tcomb_3_4_0.5_none_0.9"])
def test_moe_gemv_row_is_independent_of_its_group(qp, oracle, qstr):
    """every row's output is bitwise the same when the launch is repeated with only that row's pair present"""
    for k, m in ((384, 96), (2112, 32)):   # one part per row; four unequal parts summed through LDS
        _independent(qp, oracle, qstr, k, m)


def _independent(qp, oracle, qstr, k, m):
    got, projs, x_dev, tlut, lay, xi, oscale = _gemv_case(qp, oracle, k, m, qstr, 2, True, False, 77)
    P = len(xi)
    for pos in range(P):
        g = int(np.searchsorted(lay["group_first"], pos, side="right")) - 1
        one = dict(group_expert=lay["group_expert"][g:g + 1], group_first=np.array([pos]), group_count=np.array([1]), ngroups=1)
        alone = _run_gemv(qp, projs, x_dev, tlut, _table(one), _cuda(xi.astype(np.int32)), P, oscale, 2 * m)
        assert np.array_equal(alone[pos].view(np.uint32), got[pos].view(np.uint32)), pos
        assert (np.delete(alone, pos, axis=0) == SENTINEL).all()


def test_moe_gemv_guards(qp, oracle):
    """an expert id outside [0, E), a group past the output, ngroups above the table: no work, nothing touched"""
    k, m = 128, 32
    proj, W, ws, tlut = _experts(qp, k, m, "tcq_5_none_0.9", 5, False)
    x = _cuda(np.random.default_rng(0).standard_normal((4, k)).astype(np.float16))
    for ge, gf, gc, ng in (([E4], [0], [2], 1), ([-1], [0], [2], 1), ([0], [6], [2], 1), ([0], [0], [9], 1), ([0], [-1], [1], 1),
                           ([0], [0], [1], 0)):
        t = dict(group_expert=np.array(ge), group_first=np.array(gf), group_count=np.array(gc), ngroups=ng)
        assert (_run_gemv(qp, [proj], x, tlut, _table(t), None, 4, 1.0, m) == SENTINEL).all(), (ge, gf, gc, ng)
    t = dict(group_expert=np.array([1]), group_first=np.array([2]), group_count=np.array([2]), ngroups=7)   # ngroups > the table
    out = _run_gemv(qp, [proj], x, tlut, _table(t), _cuda(np.array([3, 3, 9, 0], dtype=np.int32)), 4, 1.0, m)
    assert (out[:2] == SENTINEL).all() and (out[4:] == SENTINEL).all()
    assert (out[2, :m] == 0).all()                                                     # an x index outside the rows reads zeros
    ref, _ = oracle.gemv(W[1], x[0:1].cpu().numpy())
    assert np.allclose(out[3, :m], ref[0] * ws[1].astype(np.float64), rtol=1e-3, atol=1e-3)


def test_moe_gemv_refuses_other_codecs(qp):
    lib, buf = qp._native.lib(), torch.zeros(1 << 12, dtype=torch.int32, device="cuda")
    p = buf.data_ptr()
    P1 = qp._native.MoeProj

    def call(proj, k=128, S=9, nproj=1):
        arr = (P1 * 2)(proj, proj)
        return lib.qpal_moe_gemv(p, 64, 4, arr, nproj, p, k, 4, None, p, p, p, p, 1, 4, k, p, S, 1.0, None)
    assert call(P1(p, None, None, 32, 5, 0, 0)) == 0
    assert call(P1(p, None, None, 32, 5, 0, 0), S=10) == -2 and call(P1(p, None, None, 32, 5, 0, 0), S=11) == -2
    assert call(P1(p, None, None, 32, 9, 0, 0)) == -2 and call(P1(p, None, None, 32, 1, 0, 0)) == -2
    assert call(P1(p, p, None, 32, 5, 7, 0)) == -2                       # kv2 != kv + 1
    assert call(P1(p, None, None, 40, 5, 0, 0)) == -1 and call(P1(p, None, None, 32, 5, 0, 0), k=144) == -1
    assert call(P1(p, p, None, 32, 3, 4, 0), k=160) == -1               # split: k % 64
    assert call(P1(p, None, None, 32, 5, 0, 48)) == -1                   # out_col + m > ldo
    assert call(P1(None, None, None, 32, 5, 0, 0)) == -3
    torch.cuda.synchronize()
    proj = qp.moe.Projection([buf[:576]], None, None, 32, 128, 9, 0, tlut_bits=10)
    with pytest.raises(qp._native.QpalError, match="KV 2..8"):
        qp.moe.moe_gemv(torch.zeros(4, 32, device="cuda"), [proj], torch.zeros(4, 128, dtype=torch.float16, device="cuda"),
                        torch.zeros(1024, 2, dtype=torch.float16, device="cuda"), buf[:1], buf[:1], buf[:1], buf[:1])


# --------------------------------------------------------------------------------------------------------------------- combine
@pytest.mark.parametrize("accumulate", [False, True])
def test_combine(qp, accumulate):
    rng = np.random.default_rng(9)
    n, top_k, H, E = 9, 2, 200, 4
    sel = np.stack([np.sort(rng.permutation(E)[:top_k]) for _ in range(n)])
    sel[[2, 6]] = -1
    lay = qp.moe.reference_layout(sel, E)
    P = n * top_k
    y = rng.standard_normal((P, H)).astype(np.float32)
    gate = rng.uniform(0.05, 1.0, size=(n, top_k)).astype(np.float32)
    base = rng.standard_normal((n, H)).astype(np.float32)
    out = _cuda(base.copy())
    qp.moe.combine(out, _cuda(y), _cuda(gate), _cuda(lay["inv"].astype(np.int32)), accumulate=accumulate)
    want = qp.moe.reference_combine(base, y, gate, lay["inv"], accumulate)
    got = out.cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(got[[2, 6]], base[[2, 6]] if accumulate else np.zeros((2, H), dtype=np.float32))


# ---------------------------------------------------------------------------------------------------------------------- MoEMLP
def _wrapped(qp, k, m, qstr, seed, su, cb_seed=3):
    il = qp.IncoherentLinear(k, m, k, m, use_linear=False)
    il.linear = qp.make_linear_from_info(qstr, qp.mem_op.dummy_linear_info(k, m, qstr, seed=seed, codebook_seed=cb_seed))
    il.SU.data.copy_(torch.from_numpy(su))
    il.Wscale.data.copy_(torch.from_numpy((np.random.default_rng(seed).uniform(0.8, 1.2, m) / np.sqrt(k)).astype(np.float16)))
    il.rot_info = "skip_r"
    il.apply_rot_info()
    return il.cuda()


def _layer(qp, E=4, H=256, I=512, q_ug="tcq_6_none_0.9", q_dp="tcomb_6_7_0.5_none_0.9", seed=0):
    rng = np.random.default_rng(seed)
    su_ug, su_dp = (rng.integers(0, 2, H) * 2.0 - 1).astype(np.float16), (rng.integers(0, 2, I) * 2.0 - 1).astype(np.float16)
    experts = [(_wrapped(qp, H, I, q_ug, 10 * e + 1, su_ug), _wrapped(qp, H, I, q_ug, 10 * e + 2, su_ug), _wrapped(qp, I, H, q_dp, 10 * e + 3, su_dp))
               for e in range(E)]
    router = torch.from_numpy((4.0 / np.sqrt(H) * rng.standard_normal((E, H))).astype(np.float16)).cuda()
    return experts, router, su_ug, su_dp


def decoded(experts):
    """per expert (up, gate, down) float64: W^ * Wscale * scale, the layers' own get_weight()"""
    return [[il.linear.get_weight().double().cpu().numpy() * il.Wscale.double().cpu().numpy()[:, None] * il.scale for il in t] for t in experts]


def test_moemlp_forward(qp):
    """the six launches against the contract on each expert's own decoded weights, within the layer tolerance (KAPPA x the format emulation's distance, moe_reference.layer_judge)"""
    E, H, I, top_k, n = 4, 256, 512, 2, 9
    assert qp.hadamard.get_hadK(H)[1] == 1 and qp.hadamard.get_hadK(I)[1] == 1
    experts, router, su_ug, su_dp = _layer(qp)
    layer = qp.MoEMLP.from_experts(router, experts, top_k, renorm=True)
    rng = np.random.default_rng(1)
    h = rng.standard_normal((n, H)).astype(np.float32)
    rms_w = (1 + 0.3 * rng.standard_normal(H)).astype(np.float16)
    active = np.arange(n, dtype=np.int64)
    active[4] = -1
    got = layer(_cuda(h), (1e-5, _cuda(rms_w)), active=_cuda(active)).cpu().numpy().astype(np.float64)
    assert (got[4] == 0).all()
    What, scale, rw = decoded(experts), experts[0][0].scale, router.cpu().numpy()
    rt = qp.moe.reference_route(h, rms_w, 1e-5, rw, None, top_k, True, active)
    ok = mref.decidable_rows(rt, mref.logit_bounds(rt, rw), top_k, active) & (active >= 0)
    assert ok.sum() >= 6
    f, rows = mref.layer_judge(What, su_ug, su_dp, scale, rt, ok, got)
    print(f"MoEMLP.forward: max distance / tolerance {f.max():.3f}")
    assert (f <= 1.0).all()
    ref = mref.layer_forward(What, su_ug, su_dp, scale, rt)
    # the same through the whole-layer contract and W_eff = diag(Wscale) W^ R diag(SU)
    eff = [[mref.wht(w) / np.sqrt(w.shape[1]) * su.astype(np.float64)[None, :] / scale for w, su in zip(t, (su_ug, su_ug, su_dp))] for t in What]
    full, _ = qp.moe.reference_moe_mlp(h, rms_w, 1e-5, rw, None, top_k, True, active, eff)
    assert np.allclose((full - h)[ok], ref[ok], rtol=1e-9, atol=1e-9)


def test_from_experts_refuses(qp):
    experts, router, su_ug, su_dp = _layer(qp, E=2, H=128, I=128)
    qp.MoEMLP.from_experts(router, experts, 2)
    bad = [list(t) for t in experts]
    bad[1][1] = _wrapped(qp, 128, 128, "tcq_6_none_0.9", 99, -su_ug)
    with pytest.raises(qp._native.QpalError, match="ONE SU"):
        qp.MoEMLP.from_experts(router, bad, 2)
    bad = [list(t) for t in experts]
    bad[1][0] = _wrapped(qp, 128, 128, "tcq_5_none_0.9", 98, su_ug)
    with pytest.raises(qp._native.QpalError, match="one quantizer string per projection kind"):
        qp.MoEMLP.from_experts(router, bad, 2)
    bad = [list(t) for t in experts]
    bad[0][2] = bad[1][2] = _wrapped(qp, 128, 128, "ldlq_2_6_none_1.0", 97, su_dp)
    with pytest.raises(qp._native.QpalError, match="routed kernel decodes"):
        qp.MoEMLP.from_experts(router, bad, 2)
    bad = [list(t) for t in experts]
    bad[0][2] = bad[1][2] = _wrapped(qp, 128, 128, "tcq_9_none_0.9", 96, su_dp)
    with pytest.raises(qp._native.QpalError, match="KV 2..8"):
        qp.MoEMLP.from_experts(router, bad, 2)


def test_quantize_experts_layer(qp):
    """a quantize_experts-built layer passes from_experts' checks and follows reference_moe_mlp on its own decoded weights"""
    E, H, I, top_k, n = 4, 256, 512, 2, 5
    g = torch.Generator().manual_seed(0)
    ups, gates = ([torch.randn(I, H, generator=g).cuda() / 16 for _ in range(E)] for _ in range(2))
    downs = [torch.randn(H, I, generator=g).cuda() / 22 for _ in range(E)]
    router = torch.randn(E, H, generator=g).cuda() * 4 / 16
    cb = {9: torch.randn(512, 2, generator=g).half()}
    layer = qp.quantize_experts(router, ups, gates, downs, ("tcq_8_none_0.9", "tcq_8_none_0.9", "tcomb_7_8_0.5_none_0.9"), top_k, codebooks=cb)
    h = torch.randn(n, H, generator=g).cuda()
    rms_w = torch.ones(H, dtype=torch.float16, device="cuda")
    got = layer(h, (1e-5, rms_w)).cpu().numpy().astype(np.float64)
    rt = qp.moe.reference_route(h.cpu().numpy(), np.ones(H), 1e-5, layer.router_w.cpu().numpy(), None, top_k, True)
    ok = mref.decidable_rows(rt, mref.logit_bounds(rt, layer.router_w.cpu().numpy()), top_k)
    ws = layer.workspace(n)
    assert np.array_equal(_i(ws.sel)[ok], rt["sel"][ok])           # the routing is the contract's
    # on each expert's own decoded weights, its own Wscale and the layer's own sign vectors: within the layer tolerance
    f, _ = mref.layer_judge(decoded(layer.experts), layer.SU_ug.cpu().numpy(), layer.SU_dp.cpu().numpy(), layer.scale, rt, ok, got)
    print(f"quantize_experts layer: max distance / tolerance {f.max():.3f}")
    assert (f <= 1.0).all()
