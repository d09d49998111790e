"""The mixture-of-experts contract on the CPU (qpalette_amd/moe.py): reference_layout against a brute-force
restatement, max_groups exact (never exceeded, and reached), and the inputs of the GPU tests (tests/test_moe.py) decidable often
enough for the kernel's sel to be held to the float64 contract."""
import itertools

import numpy as np
import pytest

import moe_reference as mref
from qpalette_amd import moe


def _same_layout(sel, E):
    got, want = moe.reference_layout(sel, E), mref.brute_layout(sel, E)
    assert got["order"].tolist() == want["order"] and got["inv"].tolist() == want["inv"]
    assert got["x_index"].tolist() == want["x_index"]
    groups = list(zip(got["group_expert"].tolist(), got["group_first"].tolist(), got["group_count"].tolist()))
    assert groups == want["groups"] and got["ngroups"] == len(groups)
    n, top_k = np.asarray(sel).shape
    assert got["ngroups"] <= moe.max_groups(n, E, top_k)
    return got


@pytest.mark.parametrize("n,E,top_k", [(1, 4, 2), (5, 4, 2), (9, 4, 2), (17, 8, 2), (12, 6, 1), (7, 5, 5), (128, 64, 8), (33, 3, 3)])
def test_layout_random(n, E, top_k):
    rng = np.random.default_rng(n * 100 + E)
    for trial in range(4 if n < 64 else 1):
        sel = np.stack([np.sort(rng.permutation(E)[:top_k]) for _ in range(n)])
        if trial % 2:
            sel[rng.random(n) < 0.3] = -1   # inactive rows
        _same_layout(sel, E)


def test_layout_adversarial():
    # all rows on one expert: groups 8, 8, ..., remainder
    sel = np.full((19, 1), 2)
    lay = _same_layout(sel, 4)
    assert lay["group_count"].tolist() == [8, 8, 3] and lay["group_expert"].tolist() == [2, 2, 2]
    assert lay["group_first"].tolist() == [0, 8, 16] and lay["order"].tolist() == list(range(19))
    # every pair on a different expert
    sel = np.arange(12).reshape(4, 3)
    lay = _same_layout(sel, 12)
    assert lay["ngroups"] == 12 and set(lay["group_count"].tolist()) == {1}
    # nothing routed
    lay = _same_layout(np.full((3, 2), -1), 4)
    assert lay["ngroups"] == 0 and set(lay["order"].tolist()) == {-1} and set(lay["inv"].tolist()) == {-1}
    # top_k = E: every expert holds every row, in row order
    lay = _same_layout(np.tile(np.arange(4), (9, 1)), 4)
    assert lay["group_count"].tolist() == [8, 1] * 4
    assert lay["x_index"].tolist() == list(range(9)) * 4
    # stability: equal experts keep their pair order; an id outside [0, E) is not routed
    sel = np.array([[1, 3], [1, 7], [0, 1]])
    lay = _same_layout(sel, 4)
    assert lay["order"].tolist() == [4, 0, 2, 5, 1, -1] and lay["inv"].tolist() == [1, 4, 2, -1, 0, 3]


def test_max_groups_is_exact():
    shapes = [(n, E, k) for n in range(1, 20) for E in range(1, 5) for k in range(1, E + 1)] + [(24, 6, 3), (9, 8, 8), (10, 8, 8), (17, 7, 2)]
    for n, E, k in shapes:
        assert moe.max_groups(n, E, k) == mref.brute_max_groups(n, E, k), (n, E, k)
    # reached by a routing, and no routing exceeds it
    for n, E, k in [(9, 4, 2), (17, 8, 2), (10, 8, 8), (24, 6, 3), (128, 64, 8), (1, 4, 2)]:
        if n <= 24:
            counts = mref.worst_counts(n, E, k)
        else:   # 1024 pairs over 64 experts: every count = 1 (mod 8)
            counts = [17] * 56 + [9] * 8
            assert sum(counts) == n * k
        sel = mref.counts_to_sel(counts, n, k)
        assert moe.reference_layout(sel, E)["ngroups"] == moe.max_groups(n, E, k), (n, E, k)
    with pytest.raises(moe.nat.QpalError):
        moe.max_groups(129, 4, 2)
    with pytest.raises(moe.nat.QpalError):
        moe.max_groups(4, 4, 5)


def test_route_contract_tie_rule_and_inactive_rows():
    rng = np.random.default_rng(3)
    W = rng.standard_normal((4, 32))
    W[3] = W[1]
    h = rng.standard_normal((6, 32))
    bias = np.array([50.0, 0.0, -50.0, 0.0])
    active = np.array([0, 1, -1, 3, 4, 5])
    rt = moe.reference_route(h, None, 1e-5, W, bias, 2, True, active)
    assert np.array_equal(rt["logits"][:, 1], rt["logits"][:, 3])
    for r in range(6):
        if active[r] < 0:
            assert rt["sel"][r].tolist() == [-1, -1] and rt["gate"][r].tolist() == [0.0, 0.0]
        else:
            assert rt["sel"][r].tolist() == [0, 1]                    # one place left: the lower id of the tie
            assert abs(rt["gate"][r].sum() - 1.0) < 1e-12
    rt2 = moe.reference_route(h, None, 1e-5, W, bias, 2, False, None)
    assert np.allclose(rt2["gate"], np.take_along_axis(rt2["p"], rt2["sel"], 1)) and (rt2["gate"].sum(-1) <= 1.0 + 1e-12).all()


def test_moe_mlp_contract_is_the_dense_mlp_when_one_expert_takes_all():
    rng = np.random.default_rng(5)
    H, I = 32, 48
    h = rng.standard_normal((3, H))
    experts = [(rng.standard_normal((I, H)), rng.standard_normal((I, H)), rng.standard_normal((H, I)) * 0.1)]
    out, rt = moe.reference_moe_mlp(h, None, 1e-5, rng.standard_normal((1, H)), None, 1, True, None, experts)
    x = rt["xhat"]
    g = x @ experts[0][1].T
    want = h + (g / (1 + np.exp(-g)) * (x @ experts[0][0].T)) @ experts[0][2].T
    assert np.allclose(out, want, rtol=1e-12, atol=1e-12) and np.array_equal(rt["gate"], np.ones((3, 1)))


@pytest.mark.parametrize("case", mref.ROUTE_CASES)
def test_gpu_route_inputs_are_decidable(case):
    """the undecidable share of every input set tests/test_moe.py routes stays under the cap, for the seed fixed per case"""
    n, H, E, top_k = case
    for bias, renorm in itertools.product((False, True), (False, True)):
        inp = mref.route_inputs(n, H, E, top_k, mref.ROUTE_SEEDS[case], bias)
        rt = moe.reference_route(inp["h"], inp["rms_w"], inp["eps"], inp["router_w"], inp["bias"], top_k, renorm, inp["active"])
        ok = mref.decidable_rows(rt, mref.logit_bounds(rt, inp["router_w"]), top_k, inp["active"])
        share = 1.0 - ok.mean()
        print(f"{case} bias={bias}: undecidable share {share:.3f}")
        assert share <= mref.UNDECIDABLE_CAP
        # the gate bound stays a small fraction of the gate: a gate of the wrong expert, or one not renormalised, is far outside
        assert (mref.gate_tolerance(rt, mref.logit_bounds(rt, inp["router_w"]), renorm) <= 0.05 * rt["gate"] + 1e-30).all()


# ---------------------------------------------------------------------------------------- the layer tolerance of the GPU tests has teeth
DEFECT_SEED = 41   # the first seed counted up from 41 whose rows meet the cap on routing-undecidable rows (asserted below)


def _defect_world(renorm):
    What, su_ug, su_dp, scale, router, wsc_dn = mref.cpu_layer()
    rng = np.random.default_rng(DEFECT_SEED)
    h = rng.standard_normal((32, 512)).astype(np.float32)
    rms_w = (1.0 + 0.3 * rng.standard_normal(512)).astype(np.float16)
    rt = moe.reference_route(h, rms_w, 1e-5, router, None, 2, renorm)
    ok = mref.decidable_rows(rt, mref.logit_bounds(rt, router), 2)
    other = (np.random.default_rng(7).integers(0, 2, 512) * 2.0 - 1)
    return What, su_ug, su_dp, scale, rt, ok, wsc_dn, other


def test_the_seeded_defects_leave_the_layer_tolerance(capsys):
    """every defect of the composition, seeded into the float64 layer, lands more than TEETH x the tolerance (KAPPA x the format
    emulation's own distance) outside; the emulation itself sits at 1 / KAPPA"""
    for renorm in (True, False):
        What, su_ug, su_dp, scale, rt, ok, wsc_dn, other = _defect_world(renorm)
        assert 1.0 - ok.mean() <= mref.UNDECIDABLE_CAP
        emu = mref.layer_forward(What, su_ug, su_dp, scale, rt, emu=True)
        f, rows = mref.layer_judge(What, su_ug, su_dp, scale, rt, ok, emu)
        assert f.max() <= 1.0 / mref.KAPPA + 1e-9
        ref = mref.layer_forward(What, su_ug, su_dp, scale, rt)
        with capsys.disabled():
            print(f"\n  renorm={renorm}: emulation's distance per row, median {np.median(mref.e_rows(emu[rows], ref[rows])):.2e}")
        for name in mref.DEFECTS:
            if (name == "gates_not_renormalised") != renorm and name in ("gates_not_renormalised", "softmax_over_the_chosen"):
                if not (name == "softmax_over_the_chosen" and not renorm):
                    continue
            bad = mref.layer_forward(What, su_ug, su_dp, scale, rt, mutate=name, wscale_dn=wsc_dn, other_su=other)
            worst = float(mref.layer_judge(What, su_ug, su_dp, scale, rt, ok, bad)[0].max())
            with capsys.disabled():
                print(f"  renorm={renorm} {name}: {worst:.1f} x the tolerance")
            assert worst > mref.TEETH, (name, worst)


# ------------------------------------------------------------------------------------------- the whole model with sparse layers (CPU)
import functools  # noqa: E402

import torch  # noqa: E402

import model_reference as mr  # noqa: E402
import moe_model_reference as mm  # noqa: E402

MODEL_SETS = mm.TOKEN_SETS


@functools.lru_cache(maxsize=None)
def _model_pair(name, renorm=True):
    spec, sparse = mm.world(renorm)
    seed, lens, prefill = MODEL_SETS[name]
    toks = mm.tokens(seed, lens)
    return spec, sparse, toks, mm.forward(spec.ref, sparse, toks), mm.forward(spec.ref, sparse, toks, emu=True, prefill=prefill)


@pytest.mark.parametrize("name", sorted(MODEL_SETS))
def test_model_token_sets_meet_both_caps(name):
    """the seeds of the GPU model tests: at most 10 % of a set's rows routing-undecidable (moe_model_reference's rule, with its closure
    over the later positions of a slot), and at most 10 % logit-undecidable (test_model_exact's cap), separately"""
    spec, sparse, toks, ref, emu = _model_pair(name)
    ok = mm.routing_decidable(ref, emu, toks)
    rows = list(ok)
    rl, el = torch.stack([ref.logits[b][p] for b, p in rows]), torch.stack([emu.logits[b][p] for b, p in rows])
    dec = mr.decidable(rl, mr.tolerance(mr.e_l(el, rl)))
    print(f"{name}: {sum(not v for v in ok.values())} routing-undecidable, {int((~dec).sum())} logit-undecidable of {len(rows)} rows")
    assert sum(not v for v in ok.values()) <= mref.UNDECIDABLE_CAP * len(rows)
    assert int((~dec).sum()) <= mref.UNDECIDABLE_CAP * len(rows)
    assert bool(((ref.ratios >= 0.3) & (ref.ratios <= 1.0)).all()), ref.ratios     # every sublayer counts, the sparse ones too


def test_the_seeded_defects_leave_the_model_tolerance(capsys):
    """model_reference.tolerance (4 x the emulation's own distance, stream and logits) against every seeded defect of a sparse layer,
    seeded into layer 2 of the float64 model: more than TEETH x outside, factors printed"""
    for renorm in (True, False):
        spec, sparse, toks, ref, emu = _model_pair("decode", renorm)
        ok = mm.routing_decidable(ref, emu, toks)
        rows = [r for r, v in ok.items() if v]

        def factor(bad):
            st = lambda o: torch.stack([o.stream[b][-1][p] for b, p in rows])   # noqa: E731
            lg = lambda o: torch.stack([o.logits[b][p] for b, p in rows])        # noqa: E731
            xh = mr.e_h(st(bad), st(ref)) / mr.tolerance(mr.e_h(st(emu), st(ref)))
            xl = mr.e_l(lg(bad), lg(ref)) / mr.tolerance(mr.e_l(lg(emu), lg(ref)))
            return float(torch.maximum(xh, xl).max())
        assert factor(emu) <= 0.25 + 1e-9
        for name in mm.DEFECTS:
            if name == ("softmax_over_the_chosen" if renorm else "gates_not_renormalised"):
                continue
            f = factor(mm.forward(spec.ref, sparse, toks, mutate=(name, 2)))
            with capsys.disabled():
                print(f"\n  model, renorm={renorm} {name}: {f:.1f} x the tolerance")
            assert f > mr.TEETH, (name, f)
