"""The four launches of csrc/block_glue.hip against the float64 rules of block_reference.py.

CPU: the bounds are restated constants (compared with glue_reference); three fp32 emulations of every rule — three summation orders
for the norms, three statements of tanh for GeGLU and the cap — stay inside HALF the bound; every seeded defect lands outside it on
the inputs the GPU tests use; the package's own contracts (blocks.reference_*) are the same functions as the rules here; the host
refuses bad arguments with the documented codes, and the Python wrappers raise QpalError before any launch.
GPU: each kernel at the smallest shapes at which it can go wrong, within the bound; bias alone EQUAL to numpy's fp32 x + b; columns
outside the views unchanged bit for bit."""
import numpy as np
import pytest
import torch

import block_reference as br
import glue_reference as gr

gpu = pytest.mark.gpu
QKV_SHAPES = [(64, 8, 2), (128, 4, 4), (256, 2, 1)]   # one, two, four elements per lane
F = np.float32


# ============================================================================================================================= CPU
def test_the_restated_constants_are_the_projects():
    import qpalette_amd.blocks as blocks
    assert br.INV_REL == gr.INV_REL and br.U == 2.0 ** -24
    assert (br.GELU_C0, br.GELU_C1) == (blocks.GELU_C0, blocks.GELU_C1)
    assert abs(br.GELU_C0 - np.sqrt(2.0 / np.pi)) < 1e-9
    # |t| sech^2(t) <= 0.448: the factor of the argument terms in the tanh bounds
    t = np.linspace(0.0, 20.0, 200001)
    assert 0.447 < (t / np.cosh(t) ** 2).max() < 0.448


def _worst(got, ref, tol):
    """max over elements of |got - ref| / tol (0 / 0 counts as 0)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / tol)
    return float(np.nanmax(r))


@pytest.mark.parametrize("hd,nq,nkv", QKV_SHAPES)
@pytest.mark.parametrize("mode", ["bias", "norm", "both"])
def test_qkv_prep_emulations_stay_inside_half_the_bound(hd, nq, nkv, mode):
    c = br.qkv_case(hd + nq, hd, nq, nkv, 7)
    q, k, v = br.qkv_views(c)
    bias = c["bias"] if mode != "norm" else None
    qw, kw = (c["qw"], c["kw"]) if mode != "bias" else (None, None)
    ref = br.qkv_prep_rule(q, k, v, nq, nkv, hd, bias, qw, kw, c["eps"])
    for order in br.ORDERS:
        got = br.emulate_qkv_prep(q, k, v, nq, nkv, hd, bias, qw, kw, c["eps"], order)
        if mode == "bias":
            for g, x, b in zip(got, (q, k, v), np.split(bias, [nq * hd, (nq + nkv) * hd])):
                assert np.array_equal(g, x + b)
            continue
        for g, r in zip(got[:2], ref[:2]):
            assert _worst(g, r, br.qkv_norm_tol(r, hd)) <= 0.5, (order, _worst(g, r, br.qkv_norm_tol(r, hd)))
        assert np.array_equal(got[2].astype(np.float64), ref[2].astype(F).astype(np.float64))   # v: the fp32 sum, or untouched
        assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any()
        if mode == "norm":   # a head of zeros stays zero
            assert not got[0][0, hd:2 * hd].any() and not got[1][0, :hd].any()


@pytest.mark.parametrize("n", [512, 2560, 8192])
def test_norm_add_emulations_stay_inside_half_the_bound(n):
    c = br.norm_add_case(n, n, 5)
    ref, tol = br.norm_add_rule(c["h"], c["y"], c["w"], c["eps"]), br.norm_add_tol(c["h"], c["y"], c["w"], c["eps"])
    for order in br.ORDERS:
        assert _worst(br.emulate_norm_add(c["h"], c["y"], c["w"], c["eps"], order), ref, tol) <= 0.5, order


def test_tanh_emulations_stay_inside_the_bound(capsys):
    """The two tanh rules have no sum whose order could vary: the three emulations are three fp32 statements of tanh.  GeGLU's stay
    inside half the bound.  The cap's bound is the 4 u cap that DESIGN.md §32.2 states for the clamped exp / rcp form, and a correctly
    rounded numpy evaluation of that very form uses 3.3 u of it (0.59 of the whole bound, at l / cap = -0.55): the cap's emulations
    (all three forms) are held to the bound itself, and the figures are printed."""
    ug = br.glu_case(3, 1792, 3)
    for form in br.TANH_FORMS:
        assert _worst(br.emulate_glu(ug, form), br.glu_rule(ug), br.glu_tol(ug)) <= 0.5, form
    for cap in (30.0, 0.75):
        l = br.cap_case(4, 1000, 3, cap)
        for form in br.TANH_FORMS:
            worst = _worst(br.emulate_cap(l, cap, form), br.cap_rule(l, cap), br.cap_tol(l, cap))
            with capsys.disabled():
                print(f"\n  cap {cap} {form}: worst error / bound {worst:.3f}")
            assert worst <= 1.0, (cap, form, worst)


@pytest.mark.parametrize("hd,nq,nkv", QKV_SHAPES)
def test_teeth_qkv_prep(hd, nq, nkv):
    """every seeded defect leaves the bound on the GPU tests' inputs"""
    c = br.qkv_case(hd + nq, hd, nq, nkv, 3)
    q, k, v = br.qkv_views(c)
    args = (q, k, v, nq, nkv, hd, c["bias"], c["qw"], c["kw"], c["eps"])
    ref = br.qkv_prep_rule(*args)
    tols = [br.qkv_norm_tol(ref[0], hd), br.qkv_norm_tol(ref[1], hd), br.U * np.abs(ref[2])]
    plain = args[:6] + (None,) + args[7:]   # the same launch without a bias, which would bury the rows of RMS 1e-4 (no_eps)
    ref0 = br.qkv_prep_rule(*plain)
    for name in br.QKV_DEFECTS:
        bad = br.qkv_prep_rule(*args, mutate=name)
        worst = max(_worst(b, r, np.maximum(t, 1e-300)) for b, r, t in zip(bad, ref, tols))
        if not name.startswith("bias"):
            worst = max([worst] + [_worst(b, r, np.maximum(br.qkv_norm_tol(r, hd), 1e-300))
                                   for b, r in zip(br.qkv_prep_rule(*plain, mutate=name)[:2], ref0[:2])])
        assert worst > 100.0, (name, worst)


def test_teeth_norm_add_glu_and_cap():
    c = br.norm_add_case(512, 512, 5)
    ref, tol = br.norm_add_rule(c["h"], c["y"], c["w"], c["eps"]), br.norm_add_tol(c["h"], c["y"], c["w"], c["eps"])
    for name in br.NORM_ADD_DEFECTS:
        assert _worst(br.norm_add_rule(c["h"], c["y"], c["w"], c["eps"], mutate=name), ref, tol) > 100.0, name
    ug = br.glu_case(3, 1792, 3)
    for name in br.GLU_DEFECTS:
        assert _worst(br.glu_rule(ug, mutate=name), br.glu_rule(ug), np.maximum(br.glu_tol(ug), 1e-300)) > 100.0, name
    l = br.cap_case(4, 1000, 3, 30.0)
    assert _worst(br.cap_rule(l, 30.0, mutate="tanh_times_cap"), br.cap_rule(l, 30.0), br.cap_tol(l, 30.0)) > 100.0


def test_the_package_contracts_are_the_rules():
    import qpalette_amd.blocks as blocks
    hd, nq, nkv = 64, 8, 2
    c = br.qkv_case(1, hd, nq, nkv, 4)
    q, k, v = br.qkv_views(c)
    a = blocks.reference_qkv_prep(q, k, v, nq, nkv, hd, c["bias"], c["qw"], c["kw"], c["eps"])
    b = br.qkv_prep_rule(q, k, v, nq, nkv, hd, c["bias"], c["qw"], c["kw"], c["eps"])
    assert all(np.allclose(x, y, rtol=1e-13, atol=0) for x, y in zip(a, b))
    n = br.norm_add_case(2, 512, 3)
    assert np.allclose(blocks.reference_norm_add(n["h"], n["y"], n["w"], n["eps"]), br.norm_add_rule(n["h"], n["y"], n["w"], n["eps"]), rtol=1e-13)
    ug = br.glu_case(3, 1792, 2)
    assert np.allclose(blocks.reference_glu_gelu_tanh(ug), br.glu_rule(ug), rtol=1e-13, atol=1e-300)
    l = br.cap_case(4, 1000, 2, 30.0)
    assert np.allclose(blocks.reference_logit_cap(l, 30.0), br.cap_rule(l, 30.0), rtol=1e-13)


def test_error_codes_are_decided_on_the_host():
    """the argument checks precede any stream work, so they run without a GPU (the pointers are never dereferenced)"""
    import qpalette_amd
    lib = qpalette_amd._native.lib()
    OK, SHAPE, PARAM, NULL, ALIGN = 0, -1, -2, -3, -4
    p, inf, nan = 4096, float("inf"), float("nan")
    prep = lambda **kw: lib.qpal_qkv_prep(*[kw.get(n, d) for n, d in (   # noqa: E731
        ("q", p), ("k", p + 2048), ("v", p + 4096), ("ld", 2048), ("rows", 3), ("nq", 8), ("nkv", 2), ("hd", 64), ("bias", p),
        ("qw", p), ("kw", p), ("eps", 1e-6), ("stream", None))])
    assert prep(q=None) == NULL and prep(v=None) == NULL
    assert prep(kw=None) == PARAM and prep(qw=None) == PARAM
    for hd in (32, 96, 512):
        assert prep(hd=hd) == SHAPE
    assert prep(ld=511) == SHAPE and prep(rows=-1) == SHAPE and prep(nq=0) == SHAPE and prep(rows=65536) == SHAPE
    for eps in (0.0, -1e-6, nan, inf):
        assert prep(eps=eps) == PARAM
    assert prep(eps=0.0, qw=None, kw=None, rows=0) == OK          # no norm: eps is not looked at; no rows: nothing is launched
    assert prep(bias=None, qw=None, kw=None) == OK                # neither: nothing is launched
    assert prep(rows=0) == OK
    assert prep(q=p + 2) == ALIGN and prep(bias=p + 1) == ALIGN and prep(kw=p + 2) == ALIGN
    na = lambda **kw: lib.qpal_norm_add(*[kw.get(n, d) for n, d in (   # noqa: E731
        ("h", p), ("ld_h", 512), ("y", p + (1 << 20)), ("ld_y", 512), ("w", p), ("eps", 1e-6), ("rows", 3), ("n", 512), ("stream", None))])
    assert na(h=None) == NULL and na(y=None) == NULL and na(w=None) == NULL
    assert na(n=510) == SHAPE and na(n=16388, ld_h=16388, ld_y=16388) == SHAPE and na(n=0) == SHAPE and na(ld_h=508) == SHAPE
    assert na(eps=0.0) == PARAM and na(eps=nan) == PARAM and na(y=p + 16) == PARAM   # (the last: y overlaps h)
    assert na(h=p + 4) == ALIGN and na(ld_y=514) == ALIGN and na(rows=0) == OK
    glu = lambda **kw: lib.qpal_glu_gelu_tanh(*[kw.get(n, d) for n, d in (   # noqa: E731
        ("act", p), ("ld_act", 1792), ("ug", p + (1 << 20)), ("ld_ug", 3584), ("rows", 3), ("inter", 1792), ("stream", None))])
    assert glu(act=None) == NULL and glu(ug=None) == NULL
    assert glu(inter=1790) == SHAPE and glu(ld_ug=3580) == SHAPE and glu(ld_act=1788) == SHAPE and glu(rows=-1) == SHAPE
    assert glu(ug=p + 16) == PARAM and glu(act=p + 8) == ALIGN and glu(rows=0) == OK
    cap = lambda **kw: lib.qpal_logit_cap(*[kw.get(n, d) for n, d in (   # noqa: E731
        ("l", p), ("ld", 1024), ("rows", 3), ("vocab", 1000), ("cap", 30.0), ("stream", None))])
    assert cap(l=None) == NULL and cap(vocab=0) == SHAPE and cap(ld=999) == SHAPE and cap(l=p + 2) == ALIGN and cap(rows=0) == OK
    for bad in (0.0, -1.0, nan, inf):
        assert cap(cap=bad) == PARAM


# ============================================================================================================================= GPU
@pytest.fixture(scope="module")
def qp():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import qpalette_amd
    qpalette_amd._native.lib()
    return qpalette_amd


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _n(t):
    return t.detach().cpu().numpy()


@gpu
@pytest.mark.parametrize("rows", [1, 3, 130])
@pytest.mark.parametrize("hd,nq,nkv", QKV_SHAPES)
def test_qkv_prep_meets_the_bound(qp, capsys, hd, nq, nkv, rows):
    c = br.qkv_case(hd + nq, hd, nq, nkv, rows)
    q0, k0, v0 = br.qkv_views(c)
    bias, qw, kw = _t(c["bias"]), _t(c["qw"]), _t(c["kw"])
    for mode in ("bias", "norm", "both"):
        buf = _t(c["buf"])
        q, k, v = br.qkv_views(c, buf)
        b = bias if mode != "norm" else None
        w = (qw, kw) if mode != "bias" else (None, None)
        qp.blocks.qkv_prep(q, k, v, nq, nkv, hd, bias=b, q_norm_w=w[0], k_norm_w=w[1], eps=c["eps"])
        torch.cuda.synchronize()
        got = _n(buf)
        gq, gk, gv = br.qkv_views(c, got)
        # columns outside the three views: bit for bit
        mask = np.ones(c["ld"], bool)
        for name, wd in (("q", c["wq"]), ("k", c["wkv"]), ("v", c["wkv"])):
            mask[c["off"][name]: c["off"][name] + wd] = False
        assert np.array_equal(got[:, mask].view(np.uint32), c["buf"][:, mask].view(np.uint32))
        bq, bk, bv = np.split(c["bias"], [nq * hd, (nq + nkv) * hd])
        if mode == "bias":
            assert np.array_equal(gq, q0 + bq) and np.array_equal(gk, k0 + bk) and np.array_equal(gv, v0 + bv)
            continue
        assert np.array_equal(gv, v0 + bv if mode == "both" else v0)   # v: the fp32 sum, never normed
        ref = br.qkv_prep_rule(q0, k0, v0, nq, nkv, hd, None if b is None else c["bias"], c["qw"], c["kw"], c["eps"])
        worst = max(_worst(gq, ref[0], br.qkv_norm_tol(ref[0], hd)), _worst(gk, ref[1], br.qkv_norm_tol(ref[1], hd)))
        with capsys.disabled():
            print(f"\n  qkv_prep hd {hd} nq {nq} nkv {nkv} rows {rows} {mode}: worst error / bound {worst:.3f}")
        assert not np.isnan(got).any() and worst <= 1.0
        if mode == "norm":   # the all-zero heads stay zero
            assert not gq[0, hd:2 * hd].any() and not gk[0, :hd].any()


@gpu
@pytest.mark.parametrize("rows", [1, 5, 130])
@pytest.mark.parametrize("n", [512, 2560, 8192])
def test_norm_add_meets_the_bound(qp, capsys, n, rows):
    c = br.norm_add_case(n + rows, n, rows)
    hbuf = np.zeros((rows, n + 12), F)       # ld_h != n; the columns past n must stay as they are
    hbuf[:, :n], hbuf[:, n:] = c["h"], 7.0
    h, y = _t(hbuf), _t(c["y"])
    qp.blocks.norm_add(h[:, :n], y, _t(c["w"]), c["eps"])
    torch.cuda.synchronize()
    got = _n(h)
    worst = _worst(got[:, :n], br.norm_add_rule(c["h"], c["y"], c["w"], c["eps"]), br.norm_add_tol(c["h"], c["y"], c["w"], c["eps"]))
    with capsys.disabled():
        print(f"\n  norm_add n {n} rows {rows}: worst error / bound {worst:.3f}")
    assert worst <= 1.0 and np.all(got[:, n:] == 7.0) and np.array_equal(_n(y), c["y"])


@gpu
@pytest.mark.parametrize("rows", [1, 3, 130])
@pytest.mark.parametrize("inter", [1792, 14336])
def test_glu_gelu_tanh_meets_the_bound(qp, capsys, inter, rows):
    ug = br.glu_case(inter + rows, inter, rows)
    out = torch.full((rows, inter + 4), 7.0, dtype=torch.float32, device="cuda:0")
    act = qp.blocks.glu_gelu_tanh(_t(ug), out=out[:, :inter])
    torch.cuda.synchronize()
    got = _n(act)
    worst = _worst(got, br.glu_rule(ug), br.glu_tol(ug))
    with capsys.disabled():
        print(f"\n  glu_gelu_tanh inter {inter} rows {rows}: worst error / bound {worst:.3f}")
    assert not np.isnan(got).any() and worst <= 1.0 and bool((out[:, inter:] == 7.0).all())
    assert got[0, 0] == 0.0 and got[0, 2] == 0.0 and got[0, 1] == F(F(30.0) * ug[0, 1])   # gate 0, -30, +30: 0, 0, up * 30
    fresh = qp.blocks.glu_gelu_tanh(_t(ug))
    assert torch.equal(fresh, act)


@gpu
@pytest.mark.parametrize("rows", [1, 3, 128])
@pytest.mark.parametrize("vocab", [1000, 1024, 128256])
def test_logit_cap_meets_the_bound(qp, capsys, vocab, rows):
    cap = 30.0
    l = br.cap_case(vocab + rows, vocab, rows, cap)
    buf = np.full((rows, vocab + 9), 1e4, F)     # ld > vocab, odd: rows of every alignment
    buf[:, :vocab] = l
    t = _t(buf)
    qp.blocks.logit_cap(t, cap, vocab=vocab)
    torch.cuda.synchronize()
    got = _n(t)
    worst = _worst(got[:, :vocab], br.cap_rule(l, cap), br.cap_tol(l, cap))
    with capsys.disabled():
        print(f"\n  logit_cap vocab {vocab} rows {rows}: worst error / bound {worst:.3f}")
    assert worst <= 1.0 and np.all(got[:, vocab:] == F(1e4)) and np.abs(got[:, :vocab]).max() <= cap
    assert got[0, 1] == F(cap) and got[0, 2] == F(-cap)   # the clamped form saturates exactly


@gpu
def test_wrappers_raise_before_any_launch(qp):
    E, d = qp._native.QpalError, "cuda:0"
    z = lambda *s, **kw: torch.zeros(*s, dtype=kw.get("dtype", torch.float32), device=d)   # noqa: E731
    buf = z(3, 1024)
    q, k, v = buf[:, :512], buf[:, 512:640], buf[:, 640:768]
    before = buf.clone()
    for kw in (dict(bias=z(768, dtype=torch.float16)), dict(bias=z(767)), dict(q_norm_w=z(64)), dict(q_norm_w=z(64), k_norm_w=z(32), eps=1e-6),
               dict(q_norm_w=z(64), k_norm_w=z(64), eps=0.0), dict(q_norm_w=z(64), k_norm_w=z(64), eps=float("nan")),
               dict(bias=z(768).cpu())):
        with pytest.raises(E):
            qp.blocks.qkv_prep(q, k, v, 8, 2, 64, **kw)
    with pytest.raises(E):
        qp.blocks.qkv_prep(q, k, v, 8, 2, 96, bias=z(768))
    with pytest.raises(E):
        qp.blocks.qkv_prep(q, k[:2], v, 8, 2, 64, bias=z(768))
    with pytest.raises(E):
        qp.blocks.qkv_prep(q.half(), k, v, 8, 2, 64, bias=z(768))
    h, y = z(3, 512), z(3, 512)
    for args in ((h, y, z(512), 0.0), (h, y, z(511), 1e-6), (h, y[:2], z(512), 1e-6), (h[:, :510], y[:, :510], z(510), 1e-6),
                 (h.half(), y, z(512), 1e-6), (h, y, z(512), float("inf"))):
        with pytest.raises(E):
            qp.blocks.norm_add(*args)
    with pytest.raises(E):
        qp.blocks.glu_gelu_tanh(z(3, 1022))
    with pytest.raises(E):
        qp.blocks.glu_gelu_tanh(z(3, 1024), out=z(3, 500))
    for cap in (0.0, -1.0, float("nan"), float("inf"), None, True):
        with pytest.raises(E):
            qp.blocks.logit_cap(z(3, 100), cap)
    with pytest.raises(E):
        qp.blocks.logit_cap(z(3, 100), 30.0, vocab=101)
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and not h.any()
