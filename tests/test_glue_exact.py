"""The launches around every projection of a decode step, held to float64 rules with bounds derived from the number formats
(rules and bounds: glue_reference.py): RMSNorm fused into the GEMV staging (x_rms + x_rot) and into the rotation
launch (qpal_hadamard_rms), final norm + lm_head (qpal_lm_head_logits, qpal_lm_head_argmax), the SwiGLU epilogue (act_out) and the
residual add (accumulate).

CPU part (no marker): the two norm rules differ by at most one fp16 ulp, kappa of the staging bound comes from an emulation that
restates the rounding points, and every check has teeth — a seeded defect of the float64 rule lands >= 4x outside the bound of the
tier that owns it.  GPU part (marked gpu): the kernels against the rules.  The tiny (rms < 2^-8) and outlier families are range
checks and exempt from the teeth requirement."""
import functools

import numpy as np
import pytest
import torch

import glue_reference as gr
from oracle import incoherent as oi

gpu = pytest.mark.gpu
EPS = 1e-5
QSTRS = ("tcq_4_none_0.9", "tcomb_6_7_0.5_none_0.9", "ldlq_2_8_none_1.0")


def _signs(rng, n):
    return (rng.integers(0, 2, n) * 2 - 1).astype(np.float64)


def _ln_weight(rng, k):
    return (1.0 + 0.1 * rng.standard_normal(k)).astype(np.float16)


def _hadk(k):
    import qpalette_amd as qp
    hk, K = qp.hadamard.get_hadK(k)
    return (None, 1) if K == 1 else (hk.T.contiguous().half(), K)   # as the incoherent wrappers pass it (had_left_T)


def _hadk64(k):
    hk, _ = _hadk(k)
    return None if hk is None else hk.numpy().astype(np.float64)


# =============================================================================================================== CPU: rules, kappa
def test_the_two_norm_rules_differ_by_at_most_one_ulp():
    """f16(f16(h inv) w) (LlamaRMSNorm, both lm_head kernels) against f16(h inv w) (the fused per-layer norm's target)."""
    rng = np.random.default_rng(1)
    for k in (512, 4096):
        x, names, _ = gr.staging_rows(rng, k)
        w = _ln_weight(rng, k)
        for wv in (w, None):
            two, one = gr.norm_two_roundings(x, wv, EPS), gr.norm_one_rounding(x, wv, EPS)
            d = np.abs(two - one) / np.maximum(gr.ulp16(one), gr.ulp16(two))
            assert d.max() <= 1.0, (k, names[int(d.max(-1).argmax())], d.max())
            if wv is None:
                assert d.max() == 0.0
            else:
                assert (d > 0).mean() > 0.05   # and they do differ: the comment in test_decoder_glue.py names which rule is whose


def _emulated_ratios(k, rng):
    """Worst (|emulation - target| - ulp) / spread per family over w / su given or not, fp32 / fp16 source, hi + lo split or not."""
    hadk = _hadk64(k)
    x, names, _ = gr.staging_rows(rng, k)
    worst = np.zeros(len(names))
    for wv in (_ln_weight(rng, k), None):
        for su in (_signs(rng, k), None):
            for hilo in ((True, False) if hadk is None else (False,)):
                for src16 in ((False, True) if k <= 4096 else (False,)):
                    xx = x
                    if src16:
                        xx = np.clip(x, -60000.0, 60000.0).astype(np.float16).astype(np.float32)
                    z = gr.emulate_staging(xx, wv, su, EPS, 1 / 32, hadk, src_f16=src16, hilo=hilo)
                    worst = np.maximum(worst, gr.staging_ratio(z, xx, wv, su, EPS, 1 / 32, hadk).max(-1))
    return names, worst


def test_kappa_comes_from_the_emulation(capsys):
    """kappa = twice the worst emulated ratio, rounded up to a power of two, separately for K = 1 and K > 1 (the fp16 rounding between
    the factors).  The table goes to DESIGN.md §25.3."""
    worst = {False: 0.0, True: 0.0}
    with capsys.disabled():
        for k in (2048, 4096, 8192, 5120, 11008):
            names, r = _emulated_ratios(k, np.random.default_rng(k))
            print(f"\n[glue] emulated staging ratio k={k}: max {r.max():.2f} ({names[int(r.argmax())]}); " +
                  " ".join(f"{v:.2f}" for v in r), end="")
            assert np.isfinite(r).all()
            worst[k in (5120, 11008)] = max(worst[k in (5120, 11008)], float(r.max()))
    for key, val in worst.items():
        assert 2.0 ** np.ceil(np.log2(2.0 * val)) == gr.KAPPA[key], (key, val)


def test_staged_rule_meets_its_bound_and_the_one_hot_row_is_analytic():
    rng = np.random.default_rng(5)
    for k in (2048, 5120):
        hadk = _hadk64(k)
        x, names, hot = gr.staging_rows(rng, k)
        w, su = _ln_weight(rng, k), _signs(rng, k)
        z = gr.staged_rule(x, w, su, EPS, 1 / 32, hadk)
        r = gr.staging_ratio(z, x, w, su, EPS, 1 / 32, hadk)
        assert r.max() <= gr.kappa(hadk) / 2, (k, names[int(r.max(-1).argmax())], r.max())
        if hadk is None:
            i = int(np.nonzero(hot >= 0)[0][0])
            want = gr.one_hot_target(k, hot[i], float(x[i, hot[i]]), w, su, EPS, 1 / 32)
            assert np.all(np.abs(z[i] - want) <= gr.ulp16(want))


def test_lm_head_interval_holds_for_an_fp32_restatement(capsys):
    """fp32 sum of squares, fp32 1/sqrt, fp32 product, two fp16 roundings (numpy float32) land inside the accepted interval on every
    family: the 2^-20 of §25.2 is not tuned to a kernel."""
    rng = np.random.default_rng(7)
    for k in (512, 8192):
        h = gr.lm_head_rows(rng, k, 18)
        w = _ln_weight(rng, k)
        ss = (h * h).sum(-1, keepdims=True, dtype=np.float32)
        inv = (np.float32(1.0) / np.sqrt(ss / np.float32(k) + np.float32(EPS))).astype(np.float32)
        x = ((h * inv).astype(np.float16) * w).astype(np.float16).astype(np.float64)
        lo, hi, exact = gr.staged_x_interval(h, w, EPS)
        assert np.all((lo <= x) & (x <= hi))
        with capsys.disabled():
            print(f"\n[glue] fp32 restatement of the lm_head norm, k={k}: {np.mean(x != exact):.2e} of the elements differ "
                  "from the exact-inv rule", end="")


# ======================================================================================================================= CPU: teeth
def _teeth(ratio, what):
    assert np.max(ratio) >= 4.0, f"{what}: the defect stays within {np.max(ratio):.2f}x the bound"


def test_teeth_lm_head():
    rng = np.random.default_rng(11)
    k, R = 1024, 96
    h = rng.standard_normal((8, k)).astype(np.float32)         # the sigma = 1 family
    w = _ln_weight(rng, k)
    W = (rng.standard_normal((R, k)) * 0.05).astype(np.float16)
    x, _ = gr.lm_head_rule(h, w, EPS, W)
    dot, tol = gr.logits_bound(x, W)
    lo, hi, exact = gr.staged_x_interval(h, w, EPS)
    assert gr.interval_excess(x, lo, hi, exact).max() == 0.0
    for mut in [("drop_col", j) for j in (0, 255, 256, k - 1)] + [("swap_stages", 1, 2)]:   # the random-row tier owns these
        _, lg = gr.lm_head_rule(h, w, EPS, W, mut)
        _teeth(np.abs(lg - dot) / tol, mut)
        assert (np.abs(lg - dot) > 4 * tol).mean() > 0.5, mut   # (a product with a small |w x| is lost unseen in that one logit)
    for mut in (("inv_row0",), ("no_weight",)):                                              # the staged-x tier owns these
        xm, _ = gr.lm_head_rule(h, w, EPS, W, mut)
        ex = gr.interval_excess(xm, lo, hi, exact)
        _teeth(ex[1:], mut)
    small = (rng.standard_normal((1, k)) * 1e-4).astype(np.float32)                          # eps dropped: the mean << eps row
    lo, hi, exact = gr.staged_x_interval(small, w, EPS)
    xm, _ = gr.lm_head_rule(small, w, EPS, W, ("no_eps",))
    _teeth(gr.interval_excess(xm, lo, hi, exact), "no_eps")


@pytest.mark.parametrize("k", [2048, 4096, 5120])
def test_teeth_staging(k):
    rng = np.random.default_rng(k)
    hadk = _hadk64(k)
    x = rng.standard_normal((4, k)).astype(np.float32)
    w, su = _ln_weight(rng, k), _signs(rng, k)
    post = 1 / 32
    assert gr.staging_ratio(gr.staged_rule(x, w, su, EPS, post, hadk), x, w, su, EPS, post, hadk).max() <= gr.kappa(hadk)
    for mut in (("zero8", 0), ("zero8", k // 2 + 8), ("zero8", k - 8), ("half_rms",), ("su_skip", 0), ("su_skip", k // 64 - 1)):
        z = gr.staged_rule(x, w, su, EPS, post, hadk, mutate=mut)
        r = gr.staging_ratio(z, x, w, su, EPS, post, hadk)
        _teeth(r.max(-1).min() / gr.kappa(hadk), (k, mut))   # in every row


def test_teeth_swiglu_and_accumulate():
    rng = np.random.default_rng(13)
    u = rng.standard_normal(4096).astype(np.float32)
    g = rng.standard_normal(4096).astype(np.float32)
    good = gr.swiglu_candidates(u, g)[1]
    assert gr.swiglu_member(good, u, g).all() and np.array_equal(good, oi.swiglu(u, g))
    ref, tol = gr.swiglu_bound(u, g, 1e-5 * np.abs(u), 1e-5 * np.abs(g))
    assert np.all(np.abs(good - ref) <= tol)
    for mut in (("silu_up",), ("no_gate_factor",)):
        bad = gr.swiglu_candidates(u, g, mut)[1]
        dist = np.abs(bad[None] - gr.swiglu_candidates(u, g)).min(0) / gr.ulp16(good)
        assert (dist >= 4).mean() > 0.9, mut              # the exact tier: ulps away from every member of the set
        _teeth(np.abs(bad - ref) / tol, mut)              # the bound tier of the real layers
        assert (np.abs(bad - ref) > 4 * tol).mean() > 0.9, mut
    h = (rng.standard_normal(1024) * 2.0 ** rng.integers(0, 11, 1024)).astype(np.float32)
    y = rng.standard_normal(1024).astype(np.float32)
    assert np.array_equal(gr.accumulate_rule(h, y), h + y)
    over = gr.accumulate_rule(h, y, ("overwrite",)).astype(np.float64)
    want = h.astype(np.float64) + y
    assert (np.abs(over - want) > 4 * gr.accumulate_split_tol(h, y, 1e-5 * np.abs(y) * 8)).mean() > 0.9


# ============================================================================================================================= GPU
@pytest.fixture(scope="module")
def qp():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import qpalette_amd
    qpalette_amd._native.lib()
    return qpalette_amd


def _dev():
    return torch.device("cuda", 0)


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(_dev())


def _n64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def _selection_layer(k, m=None, seed=None):
    """Row r of W is the unit vector e_sel[r] (5-bit scalar codes, lut = {0, 1, ...}, tensor-core packing): y[r] = x'[sel[r]], the
    launch's own staged vector, exactly.  seed None: sel = 0 .. k - 1."""
    import qpalette_amd as qp
    sel = np.arange(k) if seed is None else np.random.default_rng(seed).integers(0, k, m)
    m = sel.size
    idx = torch.zeros((m, k), dtype=torch.int32)
    idx[torch.arange(m), torch.from_numpy(sel)] = 1
    lut = torch.zeros(32, dtype=torch.float16)
    lut[1] = 1.0
    lut[2:] = torch.linspace(-3, 3, 30).half()
    info = {"in_features": k, "out_features": m, "lut_bits": 5, "vec_sz": 1, "bias": None, "dtype": torch.float16,
            "qweight": qp.packers.pack_qweight(idx, 1, 5), "lut": lut.view(32, 1)}
    return qp.VQLinearPackTensorCore.gen_layer_from_info(info).to(_dev()), sel


# ------------------------------------------------------------------------------------------------------------- final norm + lm_head
def _lm_head_W(k, R, nsel, seed):
    """nsel selection rows (W[v] = e_v) followed by R random rows ~ 0.05 N(0, 1)."""
    gen = torch.Generator(device=_dev()).manual_seed(seed)
    W = torch.zeros(nsel + R, k, dtype=torch.float16, device=_dev())
    W[torch.arange(nsel), torch.arange(nsel)] = 1.0
    W[nsel:] = (torch.randn(R, k, device=_dev(), generator=gen) * 0.05).half()
    return W


def _check_lm_head_tiers(logits, h, w, eps, W, nsel, what, capsys):
    """logits fp32 [rows, vocab] of one launch.  Tier 1: the staged x (selection rows) inside the two-rounding interval.  Tier 2: the
    random rows within 1e-5 sum |w x| of the float64 product with the kernel's OWN x.  Returns the share of staged elements that
    differ from the rule at the exact inv."""
    k = W.shape[1]
    xk = logits[:, :nsel]
    lo, hi, exact = gr.staged_x_interval(h, None if w is None else _n64(w), eps)
    lo, hi, exact = lo[:, :nsel], hi[:, :nsel], exact[:, :nsel]
    got = _n64(xk)
    bad = ~((lo <= got) & (got <= hi))
    assert not bad.any(), (f"{what}: {bad.sum()} staged x outside the interval, worst {gr.interval_excess(got, lo, hi, exact).max():.2f} "
                           f"widths, rows {sorted(set(np.nonzero(bad)[0]))[:8]}")
    share = float(np.mean(got != exact))
    if nsel == k:
        xd = xk.double()
        Wr = W[nsel:].double()
        dot, mag = xd @ Wr.T, xd.abs() @ Wr.abs().T
        err = (logits[:, nsel:].double() - dot).abs()
        tol = gr.GEMV_RTOL_ABS * mag
        assert bool((err <= tol).all()), f"{what}: random rows off by {float((err / tol.clamp_min(1e-300)).max()):.2f}x the GEMV bar"
    with capsys.disabled():
        print(f"\n[glue] {what}: {share:.2e} of {got.size} staged x differ from the exact-inv rule", end="")
    return share


# (rows, k, R, eps, weight given, strided h / wide logits): every NBT 1..8 at k = 4096 with full and ragged last tiles, every k once,
# vocab % 256 in {0, 1, 17, 255} (k is a multiple of 256: R % 256), both contract corners (eps > 0 without weight; eps = 0)
LM_LOGITS_CASES = [
    (1, 4096, 256, EPS, True, False), (16, 4096, 257, EPS, True, True), (17, 4096, 17, EPS, None, False), (33, 4096, 255, EPS, True, True),
    (48, 4096, 256, 0.0, None, False), (49, 4096, 257, EPS, True, False), (64, 4096, 17, EPS, True, True), (65, 4096, 255, EPS, None, True),
    (81, 4096, 256, EPS, True, False), (97, 4096, 257, 0.0, True, True), (113, 4096, 17, EPS, True, False), (128, 4096, 255, EPS, True, True),
    (17, 512, 257, EPS, True, True), (33, 1536, 17, EPS, None, False), (128, 8192, 255, EPS, True, True), (1, 8192, 256, EPS, None, False),
]


@gpu
@pytest.mark.parametrize("rows,k,R,eps,wgiven,strided", LM_LOGITS_CASES)
def test_lm_head_logits_two_tiers(qp, capsys, rows, k, R, eps, wgiven, strided):
    rng = np.random.default_rng(rows * 131 + k)
    h = gr.lm_head_rows(rng, k, rows)
    if not eps > 0:
        h = np.clip(h, -60000.0, 60000.0)      # no norm: x = fp16(h), the residual has to fit fp16
    w = _t(_ln_weight(rng, k)) if wgiven else None
    W = _lm_head_W(k, R, k, rows + k)
    vocab = k + R
    hbuf = torch.zeros(rows, k + (64 if strided else 0), device=_dev())
    hbuf[:, :k] = _t(h)
    out = torch.full((rows, vocab + (5 if strided else 0)), -7.0, device=_dev())
    got = qp.sampling.lm_head_logits(hbuf[:, :k], w, eps, W, out=out)
    again = qp.sampling.lm_head_logits(hbuf[:, :k], w, eps, W)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and bool((out[:, vocab:] == -7.0).all())
    logits = out[:, :vocab]
    assert torch.equal(logits, again)                       # one writer per logit: two launches are bitwise equal
    # eps <= 0: no norm and the weight is ignored; eps > 0 without a weight: w = 1
    _check_lm_head_tiers(logits, h, w if eps > 0 else None, eps, W, k,
                         f"lm_head_logits rows={rows} k={k} vocab={vocab} eps={eps} w={wgiven}", capsys)
    zero = [i for i in range(rows) if not h[i].any()]
    assert rows < 6 or zero
    for i in zero:
        assert float(logits[i].abs().max()) == 0.0


@gpu
def test_lm_head_logits_vocab_below_one_workgroup(qp, capsys):
    rows, k, nsel, R = 20, 512, 100, 77
    rng = np.random.default_rng(3)
    h = gr.lm_head_rows(rng, k, rows)
    w = _t(_ln_weight(rng, k))
    W = _lm_head_W(k, R, nsel, 9)
    logits = qp.sampling.lm_head_logits(_t(h), w, EPS, W)
    torch.cuda.synchronize()
    _check_lm_head_tiers(logits, h, w, EPS, W, nsel, "lm_head_logits vocab=177", capsys)
    x = torch.from_numpy(gr.norm_two_roundings(h, _n64(w), EPS)).to(_dev())   # (the whole x is not visible: the rule's x, one ulp of slack)
    Wr = W[nsel:].double()
    err = (logits[:, nsel:].double() - x @ Wr.T).abs()
    slack = torch.from_numpy(gr.ulp16(_n64(x.float()))).to(_dev()) @ Wr.abs().T
    assert bool((err <= gr.GEMV_RTOL_ABS * (x.abs() @ Wr.abs().T) + slack).all())


@gpu
@pytest.mark.parametrize("k", [2048, 4096, 8192])
def test_lm_head_argmax_two_tiers_and_the_token(qp, capsys, k):
    nat = qp._native
    rng = np.random.default_rng(k)
    R = 257
    vocab = k + R
    H = gr.lm_head_rows(rng, k, 9)
    w = _t(_ln_weight(rng, k))
    W = _lm_head_W(k, R, k, k)
    wsb = nat.lib().qpal_lm_head_ws_bytes(vocab)
    ws = torch.zeros(wsb // 4, device=_dev())
    tok = torch.full((1,), -1, dtype=torch.long, device=_dev())
    stream = torch.cuda.current_stream(_dev()).cuda_stream

    def launch(h, wv, eps, Wm, logits):
        toks = []
        for rep in range(2):          # twice: the ticket must be back at zero
            tok.fill_(-1)
            if logits is not None:
                logits.fill_(float("nan"))
            nat.check(nat.lib().qpal_lm_head_argmax(h.data_ptr(), wv.data_ptr() if wv is not None else None, eps, Wm.data_ptr(),
                                                    logits.data_ptr() if logits is not None else None, tok.data_ptr(), ws.data_ptr(), wsb,
                                                    vocab, k, stream), "qpal_lm_head_argmax")
            torch.cuda.synchronize()
            toks.append(int(tok[0]))
        assert toks[0] == toks[1], toks
        return toks[0]

    logits = torch.empty(vocab, device=_dev())
    for i, fam in enumerate(gr.LM_HEAD_FAMILIES):
        for wv, eps in ((w, EPS),) if i else ((w, EPS), (None, EPS), (None, 0.0), (w, 0.0)):
            h = _t(H[i])
            t = launch(h, wv, eps, W, logits)
            _check_lm_head_tiers(logits[None], H[i: i + 1], wv if eps > 0 else None, eps, W, k,
                                 f"lm_head_argmax k={k} {fam} eps={eps} w={wv is not None}", capsys)
            top = float(logits.max())
            assert t == int((logits == top).nonzero()[0, 0]), (fam, t)          # the lowest-index argmax of the kernel's own logits
            assert launch(h, wv, eps, W, None) == t
    # the winner planted (its row scaled by 1.5: exact in fp16) at row 0, in the second row a wave has in flight, in the last
    # workgroup, at vocab - 1; then at all four: equal logits, the lowest index wins
    h = _t(H[0])
    t = launch(h, w, EPS, W, logits)
    assert float(logits[t]) > 0
    grid = min(1024, (vocab + 31) // 32)
    spots = [0, 5 + 16 * grid, (grid - 1) * 16 + 3, vocab - 1]
    assert all(0 <= s < vocab for s in spots) and len(set(spots)) == 4
    for where in [[s] for s in spots] + [spots]:
        W2 = W.clone()
        for s in where:
            W2[s] = W[t] * 1.5
        t2 = launch(h, w, EPS, W2, logits)
        assert all(float(logits[s]) == float(logits[where[0]]) for s in where) and float(logits[where[0]]) > float(logits[t])
        assert t2 == min(where), (where, t2)


# ---------------------------------------------------------------------------------------------------------------- RMSNorm + rotation
def _assert_staging(got, x, names, hot, w, su, eps, post, hadk, what, capsys):
    """Rows with rms >= 2^-8 must meet the bound; smaller ones must be finite, their ratio is printed."""
    assert np.isfinite(got).all(), what
    r = gr.staging_ratio(got, x, w, su, eps, post, hadk).max(-1)
    rms = np.sqrt((x.astype(np.float64) ** 2).mean(-1))
    must = rms >= gr.RMS_SUPPORTED
    kap = gr.kappa(hadk)
    small = {names[i]: round(float(r[i]), 2) for i in range(len(r)) if not must[i]}
    with capsys.disabled():
        print(f"\n[glue] {what}: worst ratio {r[must].max():.2f} of kappa {kap:g} ({names[int(np.where(must, r, -np.inf).argmax())]}); "
              f"rms < 2^-8: {small}", end="")
    assert np.all(r[must] <= kap), f"{what}: {[(names[i], round(float(r[i]), 2)) for i in np.nonzero(must & (r > kap))[0]]}"
    if hadk is None:
        for i in np.nonzero(hot >= 0)[0]:
            want = gr.one_hot_target(x.shape[1], hot[i], float(x[i, hot[i]]), w, su, eps, post)
            _, spread = gr.staging_terms(x[i: i + 1], w, eps, post)
            assert np.all(np.abs(got[i] - want) <= gr.ulp16(want) + kap * spread[0]), what


@gpu
@pytest.mark.parametrize("k", [2048, 4096])
@pytest.mark.parametrize("src", ["fp32", "fp16"])
def test_rmsnorm_in_the_gemv_staging_meets_the_bound(qp, capsys, k, src):
    """The staged vector of the fused launch (x_rms + x_rot), read back through a selection layer, against
    left_input(norm_one_rounding(x)); w and su given or None."""
    sel, _ = _selection_layer(k)
    rng = np.random.default_rng(k + len(src))
    x, names, hot = gr.staging_rows(rng, k)
    if src == "fp16":
        keep = np.abs(x).max(-1) < 60000.0            # what an fp16 residual can hold
        x, names, hot = x[keep].astype(np.float16).astype(np.float32), [n for n, f in zip(names, keep) if f], hot[keep]
    post = 1 / 32
    for wv in (_ln_weight(rng, k), None):
        for su in (_signs(rng, k), None):
            wd = None if wv is None else _t(wv)
            sd = None if su is None else _t(su, torch.float16)
            got = np.zeros_like(x, dtype=np.float64)
            for i in range(x.shape[0]):
                xi = _t(x[i: i + 1]) if src == "fp32" else _t(x[i: i + 1], torch.float16)
                (y,) = qp.multi_gemv([sel], xi, x_rot=(sd, post), x_rms=(EPS, wd))
                got[i] = _n64(y)[0]
            _assert_staging(got, x, names, hot, None if wv is None else wv.astype(np.float64), su, EPS, post, None,
                            f"GEMV staging k={k} {src} w={wv is not None} su={su is not None}", capsys)


@gpu
@pytest.mark.parametrize("k", [2048, 4096])
def test_gemv_staging_without_a_norm_is_the_reference_pipeline(qp, k):
    """eps = 0 on the staging: no x_rms, the fp32 residual rounds to fp16 once and takes the reference's left_input."""
    sel, _ = _selection_layer(k)
    rng = np.random.default_rng(k)
    x = rng.standard_normal((1, k)).astype(np.float32)
    su = _signs(rng, k)
    (y,) = qp.multi_gemv([sel], _t(x), x_rot=(_t(su, torch.float16), 1 / 32))
    (y0,) = qp.multi_gemv([sel], _t(x), x_rot=(_t(su, torch.float16), 1 / 32), x_rms=(0.0, None))
    want = oi.left_input(x, su, None, 32.0)
    assert torch.equal(y, y0)
    assert np.all(np.abs(_n64(y) - want) <= gr.ulp16(want)) and np.mean(_n64(y) == want) > 0.99


@gpu
@pytest.mark.parametrize("qstr", QSTRS)
@pytest.mark.parametrize("k", [2048, 4096])
def test_fused_norm_launch_equals_the_plain_launch_on_its_staged_vector(qp, qstr, k):
    """The other codec instantiations of the same staging code: (x fp32, x_rms, x_rot, wscales, oscale) is bit-equal to the plain
    launch on the staged vector the selection layer reads."""
    sel, _ = _selection_layer(k)
    m = 256
    layer = qp.make_linear_from_info(qstr, qp.mem_op.dummy_linear_info(k, m, qstr, seed=k + 1)).to(_dev())
    rng = np.random.default_rng(k + 2)
    x = _t((rng.standard_normal((1, k)) * 3.0).astype(np.float32))
    w, su = _t(_ln_weight(rng, k)), _t(_signs(rng, k), torch.float16)
    wsc = _t((0.01 + 0.01 * rng.random(m)).astype(np.float16))
    rot, rms = (su, 1 / 64), (EPS, w)
    (z,) = qp.multi_gemv([sel], x, x_rot=rot, x_rms=rms)
    (fused,) = qp.multi_gemv([layer], x, wscales=[wsc], oscale=64.0, x_rot=rot, x_rms=rms)
    (plain,) = qp.multi_gemv([layer], z.half(), wscales=[wsc], oscale=64.0)
    torch.cuda.synchronize()
    assert torch.equal(z, z.half().float()) and float(fused.abs().max()) > 0
    assert torch.equal(fused, plain)


@gpu
@pytest.mark.parametrize("rows", [1, 3, 16, 128])
@pytest.mark.parametrize("n", [2048, 4096, 5120, 8192, 11008])
def test_rmsnorm_inside_the_rotation_launch_meets_the_bound(qp, capsys, n, rows):
    """qpal_hadamard_rms: the general kernel (2048, 4096), K = 20 (5120) and 172 (11008), the split kernel (8192)."""
    had = qp.hadamard
    rng = np.random.default_rng(n + rows)
    x, names, hot = gr.staging_rows(rng, n, rows)
    hk, K = _hadk(n)
    hadk = None if hk is None else hk.numpy().astype(np.float64)
    post = 1 / 32
    both = ((_ln_weight(rng, n), _signs(rng, n)), (None, None))
    one = ((_ln_weight(rng, n), None), (None, _signs(rng, n)))
    for wv, su in both if rows in (3, 128) else one:
        got = had.rotate(_t(x), hadK=None if hk is None else hk.to(_dev()), K=K, su=None if su is None else _t(su, torch.float16),
                         post_scale=post, in_mode=had.IN_F32, rms=(EPS, None if wv is None else _t(wv)))
        torch.cuda.synchronize()
        _assert_staging(_n64(got), x, names, hot, None if wv is None else wv.astype(np.float64), su, EPS, post, hadk,
                        f"hadamard_rms n={n} rows={rows} w={wv is not None} su={su is not None}", capsys)
    with pytest.raises(RuntimeError):      # eps = 0 is no norm: the entry point refuses it (rotate without rms is that launch)
        had.rotate(_t(x), hadK=None if hk is None else hk.to(_dev()), K=K, post_scale=post, in_mode=had.IN_F32, rms=(0.0, None))


# ------------------------------------------------------------------------------------------------------------------- SwiGLU epilogue
@gpu
def test_swiglu_epilogue_is_a_member_of_the_exact_set(qp, capsys):
    """Selection up | gate layer: u, g are staged elements times fp32(oscale * wscale); act_out must be f16(s * f16(u)) for an s in
    f16(silu64(f16(g)) (1 +- 2^-20)); per-row gate scales sweep |g| over 2^-8 .. 2^6 (both saturated ends of the sigmoid)."""
    k, inter = 4096, 1024
    up, selu = _selection_layer(k, inter, 21)
    gate, selg = _selection_layer(k, inter, 22)
    ident, _ = _selection_layer(k)
    qp.share_codebooks([up, gate])
    il = qp.linear.interleave_up_gate(up, gate)
    rng = np.random.default_rng(23)
    x = _t(rng.standard_normal((1, k)).astype(np.float16))
    su = _t(_signs(rng, k), torch.float16)
    wu = np.ones(inter, np.float16)
    wg = (2.0 ** (np.arange(inter) % 15 - 8)).astype(np.float16)
    osc = 1.25
    rot = (su, 1.0)
    (xs,) = qp.multi_gemv([ident], x, x_rot=rot)
    u, g = qp.multi_gemv([up, gate], x, wscales=[_t(wu), _t(wg)], oscale=osc, x_rot=rot)
    act = torch.full((1, inter), float("nan"), dtype=torch.float16, device=_dev())
    ws_il = qp.linear.interleave_rows(_t(wu), _t(wg))
    (none,) = qp.multi_gemv([il], x, wscales=[ws_il], oscale=osc, x_rot=rot, act_out=act)
    sdn = _t(_signs(rng, inter), torch.float16)
    act_s = torch.empty_like(act)
    qp.multi_gemv([il], x, wscales=[ws_il], oscale=osc, x_rot=rot, act_out=act_s, act_su=sdn)
    torch.cuda.synchronize()
    assert none is None
    xs32 = xs.cpu().numpy()[0].astype(np.float32)
    u32 = xs32[selu] * (np.float32(osc) * wu.astype(np.float32))
    g32 = xs32[selg] * (np.float32(osc) * wg.astype(np.float32))
    assert np.array_equal(u.cpu().numpy()[0], u32) and np.array_equal(g.cpu().numpy()[0], g32)   # exact in numpy float32
    ag = np.abs(g32)
    assert ag.min() < 2.0 ** -8 and (g32 < -17).any() and (g32 > 17).any() and ((g32 < -17) & (np.abs(u32) > 0.5)).any()
    a = _n64(act)[0]
    ok = gr.swiglu_member(a, u32, g32)
    with capsys.disabled():
        print(f"\n[glue] SwiGLU exact set: {np.mean(a != gr.swiglu_candidates(u32, g32)[1]):.2e} of {a.size} differ from the centre "
              "of the set", end="")
    assert ok.all(), f"{(~ok).sum()} outside the set, e.g. g = {g32[~ok][:4]}, u = {u32[~ok][:4]}, got {a[~ok][:4]}"
    assert torch.equal(act_s.view(torch.int16), (act.view(torch.int16) ^ ((sdn < 0).to(torch.int16) << 15)))   # sign flips, bit for bit


SWIGLU_REFUSED = set()   # (qstr, inter) the host refuses (QPAL_E_SHAPE from the launch planner): none of the shapes below


@gpu
@pytest.mark.parametrize("qstr,inter", [(q, i) for q in QSTRS for i in (64, 96, 1024)] + [("tcomb_6_7_0.5_none_0.9", 14336)])
def test_swiglu_epilogue_of_real_layers_meets_the_float64_bound(qp, qstr, inter):
    k = 4096
    up = qp.make_linear_from_info(qstr, qp.mem_op.dummy_linear_info(k, inter, qstr, seed=5, codebook_seed=3)).to(_dev())
    gate = qp.make_linear_from_info(qstr, qp.mem_op.dummy_linear_info(k, inter, qstr, seed=6, codebook_seed=3)).to(_dev())
    qp.share_codebooks([up, gate])
    il = qp.linear.interleave_up_gate(up, gate)
    ident, _ = _selection_layer(k)
    gen = torch.Generator(device=_dev()).manual_seed(inter)
    x = torch.randn(1, k, device=_dev(), generator=gen).half()
    su = (torch.randint(0, 2, (k,), device=_dev(), generator=gen) * 2 - 1).half()
    wu = (0.02 + 0.02 * torch.rand(inter, device=_dev(), generator=gen)).half()
    wg = (0.02 + 0.02 * torch.rand(inter, device=_dev(), generator=gen)).half()
    scale = 32.0
    rot = (su, 1.0 / scale)
    act = torch.full((1, inter), float("nan"), dtype=torch.float16, device=_dev())
    try:
        (none,) = qp.multi_gemv([il], x, wscales=[qp.linear.interleave_rows(wu, wg)], oscale=scale, x_rot=rot, act_out=act)
    except RuntimeError:
        assert (qstr, inter) in SWIGLU_REFUSED, "the host refuses a shape this test lists as served"
        return
    assert (qstr, inter) not in SWIGLU_REFUSED and none is None
    u, g = qp.multi_gemv([up, gate], x, wscales=[wu, wg], oscale=scale, x_rot=rot)
    (xs,) = qp.multi_gemv([ident], x, x_rot=rot)
    torch.cuda.synchronize()
    xa = xs.double().abs()
    du = gr.GEMV_RTOL_ABS * scale * wu.double() * (xa @ up.get_weight().double().abs().T)
    dg = gr.GEMV_RTOL_ABS * scale * wg.double() * (xa @ gate.get_weight().double().abs().T)
    ref, tol = gr.swiglu_bound(u.double().cpu().numpy(), g.double().cpu().numpy(), du.cpu().numpy(), dg.cpu().numpy())
    err = np.abs(_n64(act) - ref)
    assert np.isfinite(_n64(act)).all() and np.all(err <= tol), float((err / tol).max())


# ---------------------------------------------------------------------------------------------------------------------- residual add
def _residual(rng, n, m):
    return (rng.standard_normal((n, m)) * 2.0 ** rng.integers(0, 11, (n, m))).astype(np.float32)   # |h| up to 2^10


def _rows_shared(qp, qstr, k, m):
    """What the launch planner does with an accumulating launch of this layer: True if two workgroups share a row (their partial
    sums then arrive as atomics).  An accumulating launch shares rows where a plain one would not: the live output needs no memset."""
    import ctypes
    st = (k // 256, k // 256) if qstr.startswith("tcomb") else (k // 128, 0)
    one = lambda v: (ctypes.c_int * 1)(v)
    out = (ctypes.c_int * 1024)()
    assert qp._native.lib().qpal_plan_gemv(one(m // 32), one(st[0]), one(st[1]), one(2), 1, 16, 1, out, 1024) == 0
    M, W = out[6], out[7]
    return out[8 + 2 * (2 + 2 * M * W) + 3] > 1


@gpu
@pytest.mark.parametrize("qstr", QSTRS)
@pytest.mark.parametrize("m,n", [(8192, 1), (8192, 3), (1024, 1), (1024, 3)])
def test_accumulate_is_one_fp32_add(qp, qstr, m, n):
    """k = 4096.  m = 8192: no row is shared between workgroups, so out = fl32(h + y) BIT FOR BIT, y the same launch without
    accumulate.  m = 1024: the planner gives an accumulating launch two workgroups per row (it needs no memset for that), each adds its
    partial sum onto the live residual: the split-K bound."""
    k = 4096
    shared = _rows_shared(qp, qstr, k, m)
    assert shared == (m == 1024)
    layer = qp.make_linear_from_info(qstr, qp.mem_op.dummy_linear_info(k, m, qstr, seed=2)).to(_dev())
    rng = np.random.default_rng(n)
    x = _t(rng.standard_normal((n, k)).astype(np.float16))
    wsc = _t((0.01 + 0.01 * rng.random(m)).astype(np.float16))
    h = _residual(rng, n, m)
    forms = [dict(wscales=[wsc], oscale=64.0)]
    if n == 1:   # the decoder block's form: rotation (and norm) in the staging
        su = _t(_signs(rng, k), torch.float16)
        forms.append(dict(wscales=[wsc], oscale=64.0, x_rot=(su, 1 / 64)))
        forms.append(dict(wscales=[wsc], oscale=64.0, x_rot=(su, 1 / 64), x_rms=(EPS, _t(_ln_weight(rng, k)))))
    absW = layer.get_weight().double().abs()
    for kw in forms:
        xin = x.float() if "x_rms" in kw else x
        (y,) = qp.multi_gemv([layer], xin, **kw)
        out = _t(h)
        qp.multi_gemv([layer], xin, outs=[out], accumulate=True, **kw)
        torch.cuda.synchronize()
        assert float(y.abs().max()) > 0
        if not shared:
            want = gr.accumulate_rule(h, y.cpu().numpy())
            diff = out.cpu().numpy().view(np.int32) != want.view(np.int32)
            assert not diff.any(), (sorted(kw), int(diff.sum()))
        else:
            xs = xin
            if "x_rot" in kw:
                ident, _ = _selection_layer(k)
                (xs,) = qp.multi_gemv([ident], xin, **{a: b for a, b in kw.items() if a in ("x_rot", "x_rms")})
            delta = (gr.GEMV_RTOL_ABS * 64.0 * wsc.double() * (xs.double().abs() @ absW.T)).cpu().numpy()
            h64, y64 = h.astype(np.float64), y.double().cpu().numpy()
            err = np.abs(out.double().cpu().numpy() - (h64 + y64))
            tol = gr.accumulate_split_tol(h64, y64, delta)
            assert np.all(err <= tol), (sorted(kw), float((err / tol).max()))


@gpu
@pytest.mark.parametrize("qstr,n", [(QSTRS[0], 1), (QSTRS[1], 1), (QSTRS[1], 3), (QSTRS[2], 1)])
def test_accumulate_under_split_k_meets_the_fp32_bound(qp, qstr, n):
    """k = 14336, m = 4096: K is split over workgroups, the partial sums arrive as atomics onto the live residual."""
    k, m = 14336, 4096
    layer = qp.make_linear_from_info(qstr, qp.mem_op.dummy_linear_info(k, m, qstr, seed=5)).to(_dev())
    rng = np.random.default_rng(n + 40)
    x = _t(rng.standard_normal((n, k)).astype(np.float16))
    h = _residual(rng, n, m)
    (y,) = qp.multi_gemv([layer], x)
    out = _t(h)
    qp.multi_gemv([layer], x, outs=[out], accumulate=True)
    torch.cuda.synchronize()
    delta = (gr.GEMV_RTOL_ABS * (x.double().abs() @ layer.get_weight().double().abs().T)).cpu().numpy()
    h64, y64 = h.astype(np.float64), y.double().cpu().numpy()
    err = np.abs(out.double().cpu().numpy() - (h64 + y64))
    tol = gr.accumulate_split_tol(h64, y64, delta)
    assert np.all(err <= tol), float((err / tol).max())
    assert np.abs(out.double().cpu().numpy() - h64).max() > 1.0, "nothing was added"
