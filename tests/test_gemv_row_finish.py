"""The row finish of the fused GEMV (csrc/tc_kernels.h, behind the second workgroup barrier): the lead wave of a row sums the
partials of its run of waves — in wave order, the loads of a block of 16 / 8 / 4 / 2 / 1 partials requested together — and writes
the row (plain store, `+=` of the accumulate path, atomics on a row two workgroups share, or the SwiGLU epilogue).

Shapes: the smallest at which the finish can go wrong — ONE supertile row (m = 32) whose K makes a run of every length 1..16 (and
so every combination of blocks), two streams, several rows per workgroup with runs of mixed length, rows shared by two
workgroups, batches 1, 2, 3 and 8, three jobs in one launch, launches of more than one round (the reduction buffer reused), the
rotating kernels' SwiGLU finish.  Every output against the oracle's float64 GEMV under the project's bound
|err| <= 1e-5 * sum |w x| (tests/test_gpu_parity.py), and bit-identical between two calls.

The exact pass: every launch of the file runs a second time (`exact` in its dict) on exactly summable inputs — the codebook redrawn
from the dyadic grid of gemv_reference.py, integer x, integer residuals — and must then EQUAL the float64 sum: no order of the
finish's additions rounds, so the two-call equality holds for `accumulate` on shared rows too.

The planner decides the runs, so every test reads the plan of its launches through qpal_plan_gemv and asserts the run lengths
it is there for; test_census_of_run_lengths asserts that the file as a whole covers 1, 2, 3, 4, 5, 8, 15, 16 and a shared row.

The host reads its geometry knobs (QPAL_FORCE_G, QPAL_FORCE_RG, QPAL_GEMM_MIN_BATCH) ONCE per process (function-local statics of
csrc/qpal_capi.hip), so setting them inside a pytest process that has launched a GEMV before has no effect: the cases that need
a knob run in a fresh child process (this file as a script) that has them in its environment from the start."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gemv_reference as gx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEMV_RTOL_ABS = 1e-5  # times sum |w x|: the project's bound (tests/test_gpu_parity.py)
TCQ, TCOMB = "tcq_6_none_0.9", "tcomb_6_7_0.5_none_0.9"
Z, ACC, ACT = 1, 2, 4  # qpal_plan_gemv job flags: output declared zeroed, accumulate, SwiGLU epilogue


def _launch(layers, k, n=1, mode="plain", runs=(), shared=None, rounds=False, exact=False):
    """One GEMV launch of the file: layers [(qstr, m, seed)], mode plain / zeroed / accumulate; what its plan must show: these run
    lengths among its lead entries, a shared row (or none), more items than workgroups.  exact: on exactly summable inputs."""
    return dict(layers=[list(l) for l in layers], k=k, n=n, mode=mode, runs=list(runs), shared=shared, rounds=rounds, exact=exact)


def _exact_twin(la):
    return dict(la, exact=True)


EXACT_RESIDUAL_MAX = 64  # |integer residual| of the exact pass's accumulate launches


def _one(st, n=1):
    return _launch([(TCQ, 32, 100 + st)], 128 * st, n=n, runs=[st], shared=False)


# in-process launches (the planner's own choice) ...
ONE_ROW = [_one(st) for st in (1, 2, 3, 4, 5, 8, 9, 15, 16)] + [_launch([(TCQ, 32, 132)], 4096, runs=[16], shared=False)]
ONE_ROW_BATCH = [_one(st, n) for st in (3, 5, 16) for n in (2, 3)]
TWO_STREAMS = [_launch([(TCOMB, 32, 140 + i)], k, runs=[16], shared=False) for i, k in enumerate((2048, 4096))]
MULTI_JOB = [_launch([(TCQ, 64, 150), (TCQ, 32, 151), (TCQ, 32, 152)], 2048, n=n, runs=[16], shared=False) for n in (1, 3)]
# ... and the ones that need a knob: (environment, launches) per child process
FORCED = {
    # 7 rows of 16 + 16 steps on two workgroups: three whole rows and half of the fourth, shared, per workgroup — runs of 2, 4 and 6
    "2x7": (dict(QPAL_FORCE_G="2", QPAL_FORCE_RG="7"),
            [_launch([(TCOMB, 224, 160)], 4096, n=n, mode=mode, runs=[2, 4, 6], shared=True)
             for n, mode in ((1, "zeroed"), (3, "zeroed"), (1, "plain"), (1, "accumulate"), (2, "accumulate"))]),
    # three whole rows per workgroup; whole rows under accumulate (left alone the planner shares rows wherever that is free)
    "1x3": (dict(QPAL_FORCE_G="1", QPAL_FORCE_RG="3"),
            [_launch([(TCQ, 96, 170)], 896, n=n, mode=mode, runs=[4], shared=False)
             for n, mode in ((1, "plain"), (3, "plain"), (1, "accumulate"), (2, "accumulate"))]),
    # batch 8 on the per-wave kernel (the host sends batches >= 4 to the lockstep GEMM kernel otherwise), and a layer of 2000 rows
    # at one row per item: 2000 items on 256 workgroups, eight rounds (and 300 rows of three steps: two rounds of runs of 3) — the
    # reduction buffer is reused behind the trailing barrier
    "n8-rounds": (dict(QPAL_GEMM_MIN_BATCH="9", QPAL_FORCE_G="1", QPAL_FORCE_RG="1"),
                  [_one(st, 8) for st in (3, 5, 16)]
                  + [_launch([(TCQ, 64000, 180)], 128, runs=[1], shared=False, rounds=True),
                     _launch([(TCQ, 9600, 181)], 384, n=2, runs=[3], shared=False, rounds=True)]),
}
# every child runs its launches a second time on exact inputs (the same plans)
FORCED = {name: (env, launches + [_exact_twin(la) for la in launches]) for name, (env, launches) in FORCED.items()}


# ---------------------------------------------------------------------------------------------- the plan of a launch
def _native():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_qpal_native_rowfinish", os.path.join(ROOT, "q-palette_amd", "_native.py"))
    nat = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(nat)
    return nat


def _plan_of(lib, la, act=False):
    """(run lengths of the lead entries, any shared row, grid, items) of the launch as the host plans it"""
    rows = [m // 32 for _, m, _ in la["layers"]]
    two = [q.startswith("tcomb") for q, _, _ in la["layers"]]
    st1 = [(la["k"] // 2 if t else la["k"]) // 128 for t in two]
    st2 = [la["k"] // 2 // 128 if t else 0 for t in two]
    flag = (ACT if act else 0) | {"plain": 0, "zeroed": Z, "accumulate": ACC}[la["mode"]]
    nj = len(rows)
    arr = lambda v: (ctypes.c_int * nj)(*v)
    out = (ctypes.c_int * 1024)()
    rc = lib.qpal_plan_gemv(arr(rows), arr(st1), arr(st2), arr([flag] * nj), nj, 16, 1, out, 1024)
    assert rc == 0, rc
    o = list(out)
    M, W = o[6], o[7]
    runs, shared, pos = set(), False, 8
    for c in range(2):
        G = 1 << o[pos]
        for m in range(G if c < o[2] else 0):
            for w in range(W):
                a = o[pos + 2 + 2 * (m * W + w)] & 0xffffffff
                if not (a >> 16) & 1:
                    continue
                shared = shared or bool((a >> 10) & 1)
                if (a >> 9) & 1:
                    runs.add((a >> 11) & 31)
        pos += 2 + 2 * M * W
    return dict(runs=sorted(runs), shared=shared, grid=o[0], items=o[1])


def _check_plan(la, plan):
    assert set(la["runs"]) <= set(plan["runs"]), (la, plan)
    if la["shared"] is not None:
        assert plan["shared"] == la["shared"], (la, plan)
    if la["rounds"]:
        assert plan["items"] > plan["grid"], (la, plan)


def _child(name, plan_only, tmp_path):
    env, launches = FORCED[name]
    spec, res = os.path.join(str(tmp_path), name + ".json"), os.path.join(str(tmp_path), name + ".npz")
    with open(spec, "w") as f:
        json.dump(dict(launches=launches, plan_only=plan_only, out=res), f)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), spec], env=dict(os.environ, PYTHONPATH=ROOT, **env),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    plans = json.loads(r.stdout.strip().splitlines()[-1])
    return plans, (None if plan_only else np.load(res))


# ---------------------------------------------------------------------------------------------- running a launch
def _infos(qp, la):
    if la.get("exact"):  # the same codes, the codebook redrawn from the grid
        return [gx.exact_info(la["k"], m, q, seed=seed, codebook_seed=13) for q, m, seed in la["layers"]]
    return [qp.mem_op.dummy_linear_info(la["k"], m, q, seed=seed, codebook_seed=13, device="cpu") for q, m, seed in la["layers"]]


def _x_and_residuals(la):
    if la.get("exact"):  # integer x, integer residuals; the budget is asserted before anything is launched
        amax = gx.amax_for(la["k"])
        gx.assert_budget(la["k"], xmax=amax, base=EXACT_RESIDUAL_MAX if la["mode"] == "accumulate" else 0.0)
        x = gx.exact_x(la["n"], la["k"], seed=la["k"] * 8 + la["n"], amax=amax)
        res = [gx.exact_base(la["n"], m, seed=seed, bmax=EXACT_RESIDUAL_MAX) for _, m, seed in la["layers"]]
        return x, res
    rng = np.random.default_rng(la["k"] * 8 + la["n"])
    x = rng.standard_normal((la["n"], la["k"])).astype(np.float16)
    res = [rng.standard_normal((la["n"], m)).astype(np.float32) * 4.0 for _, m, _ in la["layers"]]
    return x, res


def _run(qp, la):
    """the launch twice -> per layer (first call, second call), numpy fp32 [n, m]"""
    import torch
    mods = [qp.make_linear_from_info(q, info).cuda() for (q, _, _), info in zip(la["layers"], _infos(qp, la))]
    if len(mods) > 1:
        qp.share_codebooks(mods)
    x, res = _x_and_residuals(la)
    xd = torch.from_numpy(x).cuda()
    got = []
    for _ in range(2):
        if la["mode"] == "accumulate":
            outs = [torch.from_numpy(r).cuda() for r in res]
            qp.multi_gemv(mods, xd, outs=outs, accumulate=True)
        else:
            fill = 0.0 if la["mode"] == "zeroed" else float("nan")
            outs = [torch.full((la["n"], m), fill, dtype=torch.float32, device="cuda") for _, m, _ in la["layers"]]
            qp.multi_gemv(mods, xd, outs=outs, outs_zeroed=la["mode"] == "zeroed")
        torch.cuda.synchronize()
        got.append([o.cpu().numpy() for o in outs])
    return list(zip(*got))


def _oracle_weight(oracle, qstr, info, m, k):
    if "tcomb" in qstr:
        return oracle.tcq_dequant(info["trellis1"].numpy(), info["tlut"].numpy(), m, k, info["tlut_bits"], info["KV"][0],
                                  c2=info["trellis2"].numpy(), KV2=info["KV"][1], split=2)
    return oracle.tcq_dequant(info["trellis"].numpy(), info["tlut"].numpy(), m, k, info["tlut_bits"], info["KV"])


def _check(qp, oracle, la, results):
    """results: per layer (first call, second call).  fp32 accumulation against the oracle's float64 sum; the accumulate path adds
    onto a live fp32 value r: one more rounding of r + y — two where two workgroups add their halves, (r + a) + b — each at most
    2^-24 (|r| + sum |w x|)."""
    x, res = _x_and_residuals(la)
    if la.get("exact"):
        for (q, m, _), info, (y, y2), r in zip(la["layers"], _infos(qp, la), results, res):
            want = gx.expected(_oracle_weight(oracle, q, info, m, la["k"]), x, base=r if la["mode"] == "accumulate" else None)
            assert gx.same(y, want), (la, gx.describe_difference(y, want))
            # nothing rounds, whatever the order: two calls agree on shared rows under accumulate as well
            assert np.array_equal(y.view(np.uint32), y2.view(np.uint32)), (la, "two calls differ", gx.describe_difference(y2, y))
        return
    for (q, m, _), info, (y, y2), r in zip(la["layers"], _infos(qp, la), results, res):
        # (two workgroups adding their halves of a shared row onto a LIVE value, (r + a) + b or (r + b) + a, round differently:
        # only there two calls may differ in the last bit — onto zeros, 0 + a + b, the order does not matter)
        if not (la["mode"] == "accumulate" and la["shared"]):
            assert np.array_equal(y.view(np.uint32), y2.view(np.uint32)), (la, "two calls differ")
        ref, scale = oracle.gemv(_oracle_weight(oracle, q, info, m, la["k"]), x)
        tol = GEMV_RTOL_ABS * scale + 1e-30
        if la["mode"] == "accumulate":
            ref = ref + r.astype(np.float64)
            tol = tol + 2.0 ** -23 * (np.abs(r) + scale)
        err = np.abs(y.astype(np.float64) - ref)
        print(f"{la['layers']} k {la['k']} n {la['n']} {la['mode']}: max err / tol {(err / tol).max():.3f}")
        assert np.all(err <= tol), (la, f"max err {err.max():.3e}, max tol-ratio {(err / tol).max():.2f}")


# ---------------------------------------------------------------------------------------------- tests
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def qp():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import qpalette_amd
    qpalette_amd._native.lib()  # fail loudly if the HIP library is missing
    return qpalette_amd


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    return o


def _in_process(qp, oracle, la):
    _check_plan(la, _plan_of(qp._native.lib(), la))
    for la in (la, _exact_twin(la)):
        _check(qp, oracle, la, _run(qp, la))


@pytest.mark.parametrize("la", ONE_ROW, ids=lambda la: f"k{la['k']}")
def test_one_row_runs_of_every_length(qp, oracle, la):
    _in_process(qp, oracle, la)


@pytest.mark.parametrize("la", ONE_ROW_BATCH, ids=lambda la: f"k{la['k']}-n{la['n']}")
def test_one_row_batches(qp, oracle, la):
    _in_process(qp, oracle, la)


@pytest.mark.parametrize("la", TWO_STREAMS, ids=lambda la: f"k{la['k']}")
def test_run_across_two_streams(qp, oracle, la):
    _in_process(qp, oracle, la)


@pytest.mark.parametrize("la", MULTI_JOB, ids=lambda la: f"n{la['n']}")
def test_three_jobs_one_launch(qp, oracle, la):
    _in_process(qp, oracle, la)


@pytest.mark.parametrize("name", sorted(FORCED))
def test_forced_geometries(qp, oracle, name, tmp_path):
    """Several rows per workgroup with runs of mixed length, rows shared by two workgroups (atomics: zeroed outputs, the memset the
    host adds when they are not, accumulate), whole rows under accumulate, batch 8, launches of eight rounds — in a child process
    that has the host's knobs in its environment."""
    plans, res = _child(name, False, tmp_path)
    for i, (la, plan) in enumerate(zip(FORCED[name][1], plans)):
        _check_plan(la, plan)
        _check(qp, oracle, la, [(res[f"l{i}_j{j}_a"], res[f"l{i}_j{j}_b"]) for j in range(len(la["layers"]))])


def test_swiglu_finish(qp):
    """The rotating kernels' finish (ROT == 1): an interleaved up | gate layer through act_out at k = 2048, driven as
    tests/test_decoder_glue.py does — fp16 silu(gate) * up equal to the two projections' launch (plain finish) + torch SwiGLU on the
    reference's fp16 rounding points within its 1-2 fp16 ulps, and bit-identical between two calls."""
    import torch
    dev = torch.device("cuda", 0)
    k, inter = 2048, 128
    la = _launch([(TCOMB, 2 * inter, 0)], k)
    plan = _plan_of(qp._native.lib(), la, act=True)
    assert not plan["shared"] and plan["runs"], plan
    up = qp.make_linear_from_info(TCOMB, qp.mem_op.dummy_linear_info(k, inter, TCOMB, seed=5, codebook_seed=3)).to(dev)
    gate = qp.make_linear_from_info(TCOMB, qp.mem_op.dummy_linear_info(k, inter, TCOMB, seed=6, codebook_seed=3)).to(dev)
    qp.share_codebooks([up, gate])
    il = qp.linear.interleave_up_gate(up, gate)
    gen = torch.Generator(device=dev).manual_seed(7)
    x = torch.randn(1, k, device=dev, generator=gen).half()
    su = (torch.randint(0, 2, (k,), device=dev, generator=gen) * 2 - 1).half()
    wu = (0.02 + 0.02 * torch.rand(inter, device=dev, generator=gen)).half()
    wg = (0.02 + 0.02 * torch.rand(inter, device=dev, generator=gen)).half()
    scale = 32.0
    u, g = qp.multi_gemv([up, gate], x, wscales=[wu, wg], oscale=scale, x_rot=(su, 1.0 / scale))
    ref = (torch.nn.functional.silu(g.half().float()).half().float() * u.half().float()).half()
    acts = []
    for _ in range(2):
        act = torch.full((1, inter), float("nan"), dtype=torch.float16, device=dev)
        qp.multi_gemv([il], x, wscales=[qp.linear.interleave_rows(wu, wg)], oscale=scale, x_rot=(su, 1.0 / scale), act_out=act)
        torch.cuda.synchronize()
        acts.append(act)
    assert torch.equal(acts[0].view(torch.int16), acts[1].view(torch.int16))
    assert bool(torch.isfinite(acts[0]).all())
    err = (acts[0].float() - ref.float()).abs()
    tol = 2.0 ** -9 * ref.float().abs() + 2.0 ** -9 * float(ref.float().abs().max()) * 2.0 ** -6
    assert bool((err <= tol).all()), float((err / tol).max())


def test_census_of_run_lengths(qp, tmp_path):
    """No case is missed silently: over the plans of every launch of this file, the lead entries' run lengths contain 1, 2, 3, 4,
    5, 8, 15 and 16, some row is shared by two workgroups and some launch has more than one round."""
    lib = qp._native.lib()
    plans = [_plan_of(lib, la) for la in ONE_ROW + ONE_ROW_BATCH + TWO_STREAMS + MULTI_JOB]
    for name in sorted(FORCED):
        plans += _child(name, True, tmp_path)[0]
    runs = set().union(*(p["runs"] for p in plans))
    assert {1, 2, 3, 4, 5, 8, 15, 16} <= runs, sorted(runs)
    assert any(p["shared"] for p in plans)
    assert any(p["items"] > p["grid"] for p in plans)


# ---------------------------------------------------------------------------------------------- the child process
def _main(spec_path):
    with open(spec_path) as f:
        spec = json.load(f)
    if spec["plan_only"]:  # (no torch, no GPU: the planner is host code)
        lib = _native().lib()
        print(json.dumps([_plan_of(lib, la) for la in spec["launches"]]))
        return
    import qpalette_amd as qp
    arrays, plans = {}, []
    for i, la in enumerate(spec["launches"]):
        plans.append(_plan_of(qp._native.lib(), la))
        for j, (a, b) in enumerate(_run(qp, la)):
            arrays[f"l{i}_j{j}_a"], arrays[f"l{i}_j{j}_b"] = a, b
    np.savez(spec["out"], **arrays)
    print(json.dumps(plans))


if __name__ == "__main__":
    _main(sys.argv[1])
