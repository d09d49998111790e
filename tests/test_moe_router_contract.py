"""The contract of the second MoE router and the shared experts on the CPU (qpalette_amd/moe.py: reference_route_ex,
reference_combine_shared, reference_moe_mlp_ex): against a second statement written the way the model cards write their
gates, against the first router at neutral parameters, the decidability of the inputs the GPU tests route, the teeth of the layer
tolerance, and every argument rule."""
import numpy as np
import pytest

import moe_reference as mref
import moe_router_reference as rr
from qpalette_amd import _native as nat
from qpalette_amd import moe


@pytest.mark.parametrize("case", rr.CASES)
def test_route_ex_is_the_model_cards_gate(case):
    """every (scoring, group_score, bias, renorm): sel and gates equal to the torch statement (topk, masked_fill with -inf) to 1e-12"""
    for variant in rr.VARIANTS:
        inp, router, rt, _ = rr.world(case, variant)
        live = inp["active"] >= 0
        sel, gate = rr.model_card_route(rt["logits"], case[3], router)
        assert np.array_equal(rt["sel"][live], sel[live]), variant
        assert np.abs(rt["gate"][live] - gate[live]).max() <= 1e-12, variant
        assert (rt["sel"][~live] == -1).all() and (rt["gate"][~live] == 0).all() and (rt["sgate"][~live] == 0).all()
        x = rt["xhat"] @ inp["shared_gate"].astype(np.float64)
        assert np.abs(rt["sgate"][live] - 1 / (1 + np.exp(-x[live]))).max() <= 1e-15
        assert np.isin(np.take_along_axis(rt["allowed"], np.maximum(rt["sel"], 0), 1)[live], True).all()


@pytest.mark.parametrize("case", mref.ROUTE_CASES)
def test_neutral_parameters_are_the_first_router(case):
    """softmax, no bias, one group, scale 1: reference_route's sel on every decidable row (and its gates)"""
    n, H, E, top_k = case
    for bias, renorm in ((False, False), (True, True)):
        inp = mref.route_inputs(n, H, E, top_k, mref.ROUTE_SEEDS[case], bias)
        old = moe.reference_route(inp["h"], inp["rms_w"], inp["eps"], inp["router_w"], inp["bias"], top_k, renorm, inp["active"])
        new = moe.reference_route_ex(inp["h"], inp["rms_w"], inp["eps"], inp["router_w"], inp["bias"], top_k, moe.Router(renorm=renorm),
                                     inp["active"])
        ok = mref.decidable_rows(old, mref.logit_bounds(old, inp["router_w"]), top_k, inp["active"])
        assert np.array_equal(new["sel"][ok], old["sel"][ok])
        assert np.abs(new["gate"] - old["gate"])[ok].max() <= 1e-15
        assert (new["sgate"] == (inp["active"] >= 0)).all()     # exactly 1.0 without a shared gate, 0 on an inactive row


@pytest.mark.parametrize("case", rr.CASES)
def test_gpu_route_inputs_are_decidable(case):
    """at most UNDECIDABLE_CAP of the rows of every variant undecidable for the committed seed, which is the first such seed counted
    up from 0; the gate bound stays a small fraction of the gate"""
    def worst(seed):
        shares = []
        for variant in rr.VARIANTS:
            inp, router, rt, b = rr.world(case, variant, seed)
            shares.append(1.0 - rr.decidable_rows(rt, b, case[3], router, inp["active"]).mean())
        return max(shares)
    for seed in range(rr.SEEDS[case]):
        assert worst(seed) > rr.UNDECIDABLE_CAP, seed
    share = worst(rr.SEEDS[case])
    print(f"{case}: worst undecidable share {share:.3f}")
    assert share <= rr.UNDECIDABLE_CAP
    for variant in rr.VARIANTS:
        inp, router, rt, b = rr.world(case, variant, rr.SEEDS[case])
        assert (rr.gate_tolerance(rt, b, router) <= 0.05 * rt["gate"] + 1e-30).all(), variant
        assert (rr.shared_gate_tolerance(rt, inp["shared_gate"]) <= 1e-3).all()


def test_check_router_refuses():
    R = moe.Router
    for bad, E, top_k in ((R(n_group=3), 8, 2),                          # E % n_group
                          (R(n_group=4, topk_group=0), 8, 2), (R(n_group=4, topk_group=5), 8, 2),
                          (R(n_group=4, topk_group=1), 8, 3),            # topk_group * S < top_k
                          (R(n_group=8, topk_group=4, group_score="top2"), 8, 2),   # S = 1
                          (R(routed_scale=0.0), 8, 2), (R(routed_scale=-1.0), 8, 2), (R(routed_scale=float("inf")), 8, 2),
                          (R(routed_scale=float("nan")), 8, 2), (R(scoring="tanh"), 8, 2), (R(group_score="mean"), 8, 2)):
        with pytest.raises(nat.QpalError):
            moe.check_router(bad, E, top_k)
        with pytest.raises(nat.QpalError):
            moe.reference_route_ex(np.ones((1, 8)), None, 1e-5, np.ones((E, 8)), None, top_k, bad)
    moe.check_router(R(n_group=4, topk_group=2, group_score="top2"), 8, 3)
    for n, E, top_k in ((129, 8, 2), (1, 257, 2), (1, 8, 9)):        # the limits stay
        with pytest.raises(nat.QpalError):
            moe.reference_route_ex(np.ones((n, 8)), None, 1e-5, np.ones((E, 8)), None, top_k, R())


def test_group_mask_rules():
    """hand-made keys: ties between groups go to the lower group, ties between experts to the lower id, an expert outside the allowed
    groups is never chosen although its key is the largest left, and the bias never enters a gate"""
    H, E = 8, 8
    W = np.zeros((E, H))
    h = np.ones((1, H))
    sb = np.array([0.5, 0.0, 0.5, 0.0, 0.0, 0.2, 0.4, 0.1])     # sigmoid(0) = 0.5 everywhere: the keys are 0.5 + sb
    r = moe.Router("sigmoid", sb, 4, 2, "max", False, 1.0, None)
    rt = moe.reference_route_ex(h, None, 1e-5, W, None, 3, r)
    # groups (0,1) (2,3) (4,5) (6,7): scores 1.0, 1.0, 0.7, 0.9 -> groups 0 and 1; keys 1.0, .5, 1.0, .5: experts 0, 2 and the tie 1 < 3
    assert rt["sel"].tolist() == [[0, 1, 2]] and np.array_equal(rt["gate"], np.full((1, 3), 0.5))
    r = r._replace(group_score="top2")                           # sums 1.5, 1.5, 1.2, 1.5: the three-way tie goes to groups 0 and 1
    assert moe.reference_route_ex(h, None, 1e-5, W, None, 3, r)["sel"].tolist() == [[0, 1, 2]]
    r = r._replace(topk_group=3, renorm=True, routed_scale=3.0)  # group 3 joins: keys 1.0, 1.0, 0.9 -> experts 0, 2, 6
    rt = moe.reference_route_ex(h, None, 1e-5, W, None, 3, r)
    assert rt["sel"].tolist() == [[0, 2, 6]] and np.allclose(rt["gate"], 1.0, rtol=0, atol=1e-15)


def test_reference_combine_shared():
    rng = np.random.default_rng(3)
    n, top_k, H = 4, 2, 6
    inv = np.array([[0, 1], [-1, -1], [2, 3], [-1, -1]])
    y = rng.standard_normal((4, H)).astype(np.float32)
    gate = rng.uniform(0.1, 1, (n, top_k)).astype(np.float32)
    ys = rng.standard_normal((n, H)).astype(np.float32)
    ys[3] = np.nan
    sgate = np.array([0.5, 0.25, 0.0, 0.0], dtype=np.float32)
    base = rng.standard_normal((n, H)).astype(np.float32)
    plain = moe.reference_combine(base, y, gate, inv, True)
    out = moe.reference_combine_shared(base, y, gate, inv, ys, sgate, True)
    r0 = (gate[0, 0] * y[0]).astype(np.float32) + (gate[0, 1] * y[1]).astype(np.float32)
    assert np.array_equal(out[0], base[0] + (r0 + (sgate[0] * ys[0]).astype(np.float32)))
    assert np.array_equal(out[1], base[1] + (sgate[1] * ys[1]).astype(np.float32))      # no routed pair: the term is t
    assert np.array_equal(out[2], plain[2]) and np.array_equal(out[3], base[3])        # sgate == 0: no shared term, NaN stays out
    over = moe.reference_combine_shared(base, y, gate, inv, ys, sgate, False)
    assert np.array_equal(over[1], (sgate[1] * ys[1]).astype(np.float32)) and (over[3] == 0).all()


def test_reference_moe_mlp_ex_is_the_sum_of_its_parts():
    rng = np.random.default_rng(5)
    n, H, I, E = 4, 16, 8, 4
    experts = [(rng.standard_normal((I, H)), rng.standard_normal((I, H)), rng.standard_normal((H, I))) for _ in range(E)]
    shared = (rng.standard_normal((12, H)), rng.standard_normal((12, H)), rng.standard_normal((H, 12)))
    h, W = rng.standard_normal((n, H)), rng.standard_normal((E, H))
    active = np.array([0, -1, 2, 3])
    router = moe.Router("sigmoid", rng.standard_normal(E) * 0.1, 2, 1, "top2", True, 2.0, rng.standard_normal(H))
    out, rt = moe.reference_moe_mlp_ex(h, None, 1e-5, W, None, 2, router, active, experts, shared)
    assert np.array_equal(out[1], h[1])
    for r in (0, 2, 3):
        x = rt["xhat"][r]
        mlp = lambda t: t[2] @ ((t[1] @ x) / (1 + np.exp(-(t[1] @ x))) * (t[0] @ x))   # noqa: E731
        want = h[r] + sum(rt["gate"][r, j] * mlp(experts[rt["sel"][r, j]]) for j in range(2)) + rt["sgate"][r] * mlp(shared)
        assert np.allclose(out[r], want, rtol=1e-12, atol=1e-12)
    # neutral router, no shared expert: the first router's layer
    a, _ = moe.reference_moe_mlp_ex(h, None, 1e-5, W, None, 2, moe.Router(), active, experts)
    b, _ = moe.reference_moe_mlp(h, None, 1e-5, W, None, 2, True, active, experts)
    assert np.allclose(a, b, rtol=1e-14, atol=1e-14)


# ---------------------------------------------------------------------------------------- the layer tolerance of the GPU tests has teeth
DEFECT_SEED = 41   # the first seed counted up from 41 whose rows meet the cap on routing-undecidable rows (asserted below)


def _defect_world():
    """moe_reference.cpu_layer's experts behind a sigmoid router (its entries / 4: N(0, 1) / sqrt(H)) with a bias, 4 groups of
    which the 2 best by "top2" are allowed, renormalised gates times 2.5, and a gated shared expert with sign vectors of its own"""
    What, su_ug, su_dp, scale, router_w, _ = mref.cpu_layer()
    Ws, s_ug, s_dp, s_scale = rr.cpu_shared()
    rng = np.random.default_rng(DEFECT_SEED)
    h = rng.standard_normal((32, 512)).astype(np.float32)
    rms_w = (1.0 + 0.3 * rng.standard_normal(512)).astype(np.float16)
    router_w = (router_w.astype(np.float64) / 4).astype(np.float16)
    router = moe.Router("sigmoid", (0.1 * rng.standard_normal(8)).astype(np.float32), 4, 2, "top2", True, rr.ROUTED_SCALE,
                        (rng.standard_normal(512) / np.sqrt(512)).astype(np.float16))
    rt = moe.reference_route_ex(h, rms_w, 1e-5, router_w, None, 2, router)
    ok = rr.decidable_rows(rt, rr.bounds(rt, router_w, router), 2, router)
    return (What, su_ug, su_dp, scale, Ws, s_ug, s_dp, s_scale), router, rt, ok


def test_the_seeded_defects_leave_the_layer_tolerance(capsys):
    """every defect of the second router and the shared expert, seeded into the float64 layer, lands more than TEETH x the
    tolerance (KAPPA x the format emulation's own distance) outside in some row; the emulation itself sits at 1 / KAPPA"""
    world, router, rt, ok = _defect_world()
    assert 1.0 - ok.mean() <= rr.UNDECIDABLE_CAP
    emu = rr.layer_forward_ex(*world, rt, emu=True)
    f, rows = rr.layer_judge_ex(world, rt, ok, emu)
    assert f.max() <= 1.0 / mref.KAPPA + 1e-9
    for name in rr.DEFECTS:
        bad = rr.layer_forward_ex(*world, rt, router=router, mutate=name)
        worst = float(rr.layer_judge_ex(world, rt, ok, bad)[0].max())
        with capsys.disabled():
            print(f"\n  {name}: {worst:.1f} x the tolerance")
        assert worst > mref.TEETH, (name, worst)


# ------------------------------------------------------------------------------------------- the whole model with such layers (CPU)
import functools  # noqa: E402

import torch  # noqa: E402

import model_reference as mr  # noqa: E402
import moe_router_model_reference as mm  # noqa: E402


@functools.lru_cache(maxsize=None)
def _model_pair(name):
    spec, sparse = mm.world()
    seed, lens, prefill = mm.TOKEN_SETS[name]
    toks = mm.tokens(seed, lens)
    return spec, sparse, toks, mm.forward(spec.ref, sparse, toks), mm.forward(spec.ref, sparse, toks, emu=True, prefill=prefill)


@pytest.mark.parametrize("name", sorted(mm.TOKEN_SETS))
def test_model_token_sets_meet_both_caps(name):
    """the seeds of the GPU model tests: at most 10 % of a set's rows routing-undecidable (moe_router_model_reference's rule) and at
    most 10 % logit-undecidable (test_model_exact's cap), separately; every sublayer counts, the sparse ones with their shared
    expert too"""
    spec, sparse, toks, ref, emu = _model_pair(name)
    ok = mm.routing_decidable(ref, emu, toks, sparse)
    rows = list(ok)
    rl, el = torch.stack([ref.logits[b][p] for b, p in rows]), torch.stack([emu.logits[b][p] for b, p in rows])
    dec = mr.decidable(rl, mr.tolerance(mr.e_l(el, rl)))
    print(f"{name}: {sum(not v for v in ok.values())} routing-undecidable, {int((~dec).sum())} logit-undecidable of {len(rows)} rows")
    assert sum(not v for v in ok.values()) <= rr.UNDECIDABLE_CAP * len(rows)
    assert int((~dec).sum()) <= rr.UNDECIDABLE_CAP * len(rows)
    assert bool(((ref.ratios >= 0.3) & (ref.ratios <= 1.0)).all()), ref.ratios


def test_the_seeded_defects_leave_the_model_tolerance(capsys):
    """model_reference.tolerance (4 x the emulation's own distance, stream and logits) against every defect of the second router
    and the shared expert, seeded into the layer of the float64 model that can show it: more than TEETH x outside, factors printed"""
    spec, sparse, toks, ref, emu = _model_pair("decode")
    ok = mm.routing_decidable(ref, emu, toks, sparse)
    rows = [r for r, v in ok.items() if v]

    def factor(bad):
        st = lambda o: torch.stack([o.stream[b][-1][p] for b, p in rows])   # noqa: E731
        lg = lambda o: torch.stack([o.logits[b][p] for b, p in rows])        # noqa: E731
        xh = mr.e_h(st(bad), st(ref)) / mr.tolerance(mr.e_h(st(emu), st(ref)))
        xl = mr.e_l(lg(bad), lg(ref)) / mr.tolerance(mr.e_l(lg(emu), lg(ref)))
        return float(torch.maximum(xh, xl).max())
    assert factor(emu) <= 0.25 + 1e-9
    for name in mm.DEFECTS:   # (layer 0 has the bias, the "top2" groups and the gate; layer 2 shows the scale without a renormalisation)
        layer = 2 if name == "routed_scale_dropped" else 0
        f = factor(mm.forward(spec.ref, sparse, toks, mutate=(name, layer)))
        with capsys.disabled():
            print(f"\n  model, layer {layer}, {name}: {f:.1f} x the tolerance")
        assert f > mr.TEETH, (name, f)
