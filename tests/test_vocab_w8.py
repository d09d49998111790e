"""8-bit vocabulary tables: qpal_lm_head_w8 against float64 (glue_reference's rule and bounds), bit-exact on exactly
summable inputs, its fused argmax, qpal_embed_rows_w8, the quantizer, the step classes against their fp16 twins, the guards."""
import numpy as np
import pytest
import torch

import glue_reference as gr
import model_reference as mr

pytestmark = pytest.mark.gpu
EPS, F8 = 1e-5, torch.float8_e4m3fn
TIES = ((15, 16), (31, 32), (255, 256))   # across a tile, a wave and a workgroup boundary


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


def _table(qp, rng, vocab, k, nsel=0):
    """nsel selection rows (1.0 at column v, scale 1) then random e4m3 bytes (signs, zeros, subnormals, +-448 for the NaN codes)
    with scales log-uniform over 2^-12 .. 2^4 -> (Table8, float64 values)"""
    b = rng.integers(0, 256, (vocab, k), dtype=np.uint8)
    b[(b & 0x7F) == 0x7F] -= 1
    b[:, ::7] &= 0x87                                  # a seventh of the columns: zeros and subnormals
    s = np.exp2(rng.uniform(-12, 4, vocab)).astype(np.float32)
    b[:nsel], s[:nsel] = 0, 1.0
    b[np.arange(nsel), np.arange(nsel)] = 0x38
    t = qp.sampling.Table8(_t(b).view(F8), _t(s))
    return t, t.dequantize().double().cpu().numpy()


# (rows, k, R, eps, strided): vocab = R without a norm, k selection rows + R with one (the staged x is then visible, §25.2)
LOGITS_CASES = [(1, 512, 33, 0.0, False), (16, 512, 545, 0.0, False), (17, 1536, 545, 0.0, False), (128, 1536, 33, 0.0, False),
                (128, 512, 545, 0.0, False), (8, 512, 545, 0.0, True), (17, 8192, 545, 0.0, False), (17, 512, 33, EPS, True),
                (1, 1536, 33, EPS, False)]


@pytest.mark.parametrize("rows,k,R,eps,strided", LOGITS_CASES)
def test_logits_against_float64(qp, rows, k, R, eps, strided):
    rng = np.random.default_rng(rows * 131 + k + R)
    nsel = k if eps > 0 else 0
    vocab = nsel + R
    h = np.clip(gr.lm_head_rows(rng, k, rows), -60000.0, 60000.0)
    w = _t((1.0 + 0.1 * rng.standard_normal(k)).astype(np.float16)) if eps > 0 else None
    table, W = _table(qp, rng, vocab, k, nsel)
    hbuf = torch.zeros(rows, k + (64 if strided else 0), device=_dev())
    hbuf[:, :k] = _t(h)
    out = torch.full((rows, vocab + (5 if strided else 0)), -7.0, device=_dev())
    qp.sampling.lm_head_logits(hbuf[:, :k], w, eps, table, out=out)
    again = qp.sampling.lm_head_logits(hbuf[:, :k], w, eps, table)
    assert bool((out[:, vocab:] == -7.0).all()) and torch.equal(out[:, :vocab], again)
    got = out[:, :vocab].double().cpu().numpy()
    x = gr.f16(h.astype(np.float64))
    if eps > 0:   # tier 1: the kernel's own staged x inside the two-rounding interval; tier 2 below is then held on that x
        x = got[:, :nsel]
        lo, hi, _ = gr.staged_x_interval(h, w.double().cpu().numpy(), eps)
        assert np.all((lo <= x) & (x <= hi))
    dot, tol = gr.logits_bound(x, W[nsel:])
    assert np.all(np.abs(got[:, nsel:] - dot) <= tol), float((np.abs(got[:, nsel:] - dot) / np.maximum(tol, 1e-300)).max())


@pytest.mark.parametrize("k", [512, 1536])
@pytest.mark.parametrize("vocab", [33, 545])
@pytest.mark.parametrize("rows", [1, 16, 17, 128])
def test_exact_sums_and_the_argmax(qp, rows, vocab, k):
    """weights n / 8 (|n| <= 15), power-of-two scales, integer h, no norm: every partial sum fits fp32, the logits EQUAL the float64
    product; row i < 3 has an exact tie of its maximum at TIES[i]; token = numpy.argmax of the launch's own logits"""
    rng = np.random.default_rng(rows + vocab + k)
    sp = qp.sampling
    h = rng.integers(-8, 9, (rows, k)).astype(np.float32)
    n8 = rng.integers(-15, 16, (vocab, k)).astype(np.float32) / 8
    s = np.exp2(rng.integers(-3, 3, vocab)).astype(np.float32)
    ties = [p for p in TIES[:rows] if p[1] < vocab]
    for i, (a, b) in enumerate(ties):
        n8[a] = n8[b] = np.where(h[i] < 0, -1.875, 1.875)
        s[a] = s[b] = 8.0
    table = sp.Table8(_t(n8).to(F8), _t(s))
    assert torch.equal(table.w8.float().cpu(), torch.from_numpy(n8))
    hd = _t(h)
    active = torch.zeros(rows, dtype=torch.int64, device=_dev())
    active[rows // 2] = -1
    only = sp.lm_head_logits(hd, None, 0.0, table)
    both, tok2 = torch.empty_like(only), torch.full((rows,), -7, dtype=torch.int64, device=_dev())
    tok1, ws = tok2.clone(), sp.lm_head_w8_workspace(rows, vocab, _dev())
    sp.lm_head_argmax(hd, None, 0.0, table, tok1, active=active, ws=ws)
    sp.lm_head_argmax(hd, None, 0.0, table, tok2, active=active, ws=ws, out=both)
    assert torch.equal(only, both) and torch.equal(tok1, tok2) and not bool(ws.any())
    want = h.astype(np.float64) @ (n8.astype(np.float64) * s[:, None]).T
    assert np.array_equal(only.double().cpu().numpy(), want)
    expect = want.argmax(-1)
    assert all(expect[i] == a for i, (a, b) in enumerate(ties))
    expect[rows // 2] = -7
    assert np.array_equal(tok1.cpu().numpy(), expect)


@pytest.mark.parametrize("k", [48, 512])
def test_embedding_rows(qp, k):
    rng = np.random.default_rng(k)
    vocab = 545
    table, _ = _table(qp, rng, vocab, k)
    tokens = _t(np.array([0, vocab - 1, -1, vocab, 7, 256, 7], dtype=np.int64))
    out = torch.full((7, k + 8), -7.0, device=_dev())
    qp.sampling.embed_rows(table, tokens, out)
    ok = ((tokens >= 0) & (tokens < vocab)).cpu()
    t = tokens.cpu().clamp(0, vocab - 1)
    want = torch.where(ok[:, None], table.scale.cpu()[t][:, None] * table.w8.cpu().float()[t], torch.zeros(()))
    assert torch.equal(out[:, :k].cpu(), want) and bool((out[:, k:] == -7.0).all())


def test_quantizer(qp):
    g = torch.Generator().manual_seed(3)
    t = torch.randn(6, 512, generator=g)
    t[torch.arange(5), torch.arange(5) * 9] = 40.0
    t[5] = 0.0
    t = t.half()
    q = qp.sampling.quantize_table(t)
    deq, amax = q.dequantize(), t.float().abs().amax(1)
    assert float(q.scale[5]) == 1.0 and torch.equal(q.scale[:5], amax[:5] / 448.0)
    # half an e4m3 step: 2^-4 relative on a normal element, 2^-10 scale below 2^-6 scale (+ the fp32 division in front of the cast)
    half_step = torch.maximum(t.float().abs() * 2.0 ** -4, q.scale[:, None] * 2.0 ** -10) * (1 + 2.0 ** -20)
    assert bool(((deq - t.float()).abs() <= half_step).all())
    assert bool(((deq.abs().amax(1) - amax).abs() <= amax * 2.0 ** -23).all())


def _pow2_table(qp, t):
    """a Table8 of power-of-two scales near t and its exact fp16 twin"""
    s = torch.exp2(torch.ceil(torch.log2(t.float().abs().amax(1) / 448.0)))
    t8 = qp.sampling.Table8((t.float() / s[:, None]).to(F8), s)
    twin = t8.dequantize().half()
    assert torch.equal(twin.float(), t8.dequantize())
    return t8, twin


# SEED: chosen on the CPU with model_reference's float64 forward on the twin tables — every row of the three plans below has a
# top-two gap of at least 2.4 times the bound of `_agree` there, so the reference alone excuses no row (the cap is 10 %)
STEPS, SEED = 6, 7


def _decode(qp, m, B, embed, lm_head, sampled, graph=False):
    """STEPS teacher-forced steps, the last slot of B > 1 idle -> (logits [STEPS, B, vocab] or None, tokens [STEPS, B])"""
    dev, live = _dev(), max(1, B - 1)
    g = torch.Generator().manual_seed(SEED + B)
    toks = torch.randint(0, mr.VOCAB, (STEPS, B), generator=g)
    kc = [torch.zeros(B, m.cfg.num_key_value_heads, 64, m.cfg.head_dim, dtype=torch.float16, device=dev) for _ in m.layers]
    vc = [t.clone() for t in kc]
    tok, pos = torch.zeros(B, dtype=torch.long, device=dev), torch.full((B,), -1, dtype=torch.long, device=dev)
    out = torch.full((B,), -7, dtype=torch.long, device=dev)
    smp = qp.Sampler(B, mr.VOCAB, dev, temperature=0.0) if sampled else None
    step = qp.DecodeStep(m.layers, embed, m.norm, lm_head, kc, vc, m.inv_freq, tok, pos, out, sampler=smp)
    run, ls, ts = step, [], []
    for s in range(STEPS):
        tok.copy_(toks[s])
        pos[:live] = s
        if graph and s == 1:   # step 0 ran eagerly; the rest replay one captured step
            run = torch.cuda.CUDAGraph()
            with torch.cuda.graph(run):
                step()
        run.replay() if run is not step else step()
        ls.append(smp.logits.clone() if sampled else None)
        ts.append(out.clone())
    assert all(int(t[-1]) == -7 for t in ts) or B == 1
    return (torch.stack(ls) if sampled else None), torch.stack(ts)[:, :live]


@pytest.fixture(scope="module")
def model(qp):
    m = mr.build("S", "mixed", (), mr.NLAYERS, mr.VOCAB, 0, _dev())
    return m, _pow2_table(qp, m.embed), _pow2_table(qp, m.lm_head)


def _agree(l16, t16, l8, t8, cap=0.10):
    """logits within twice test_sampling.py's lm_head bound; tokens equal where the fp16 top-two gap exceeds it; <= 10 % excused"""
    bound = 2.0 * (2e-3 + 1e-3) * float(l16.abs().max())
    assert float((l8 - l16).abs().max()) <= bound
    top2 = l16.topk(2, dim=-1).values
    clear = (top2[..., 0] - top2[..., 1]) > bound
    assert float((~clear).float().mean()) <= cap
    assert torch.equal(t8[clear], t16[clear])
    return bound


def _caches(m, B):
    kc = [torch.zeros(B, m.cfg.num_key_value_heads, 64, m.cfg.head_dim, dtype=torch.float16, device=_dev()) for _ in m.layers]
    return kc, [t.clone() for t in kc]


def test_the_steps_gather_is_bitwise_the_fp16_steps(qp, model):
    """the stream rows directly behind the gather of the step's own `_run_layers` (no layer run): all rows, and a short chunk"""
    m, (e8, e16), _ = model
    toks, got = _t(np.array([0, mr.VOCAB - 1, 5, 5], dtype=np.int64)), []
    for embed in (e16, e8):
        kc, vc = _caches(m, 4)
        st = qp.DecodeStep(m.layers, embed, m.norm, m.lm_head, kc, vc, m.inv_freq, toks, toks.clone(), toks.clone())
        pf = qp.Prefill(m.layers, embed, m.norm, m.lm_head, kc, vc, m.inv_freq, chunk=16)
        st.layers = pf.layers = []
        st.h32.fill_(-7.0), pf.h32.fill_(-7.0)
        got.append((st._run_layers(toks).clone(), pf._run_layers(toks[1:], 3).clone(), pf.h32[3:].clone()))
    assert all(torch.equal(a, b) for a, b in zip(*got))
    assert torch.equal(got[1][0], e16[toks].float()) and torch.equal(got[1][1], e16[toks[1:]].float())
    assert bool((got[1][2] == -7.0).all())


@pytest.mark.parametrize("cls", ["RaggedStep", "SpeculativeStep", "Score"])
def test_the_other_steps_against_the_fp16_twin(qp, model, cls):
    """greedy RaggedStep and SpeculativeStep with a Table8 end in the ONE launch that writes logits and tokens: the tokens EQUAL the
    argmax of the step's own logits, inactive rows keep theirs, and logits / tokens agree with the fp16 twin's as `_agree` says (no
    cap on excused rows here: three and eight rows).  Score: |lp8 - lp16| <= 2 bounds, the logit's own and the log-sum-exp's."""
    m, (e8, e16), (l8, l16) = model
    g = torch.Generator().manual_seed(SEED)
    seqs = [torch.randint(0, mr.VOCAB, (n,), generator=g).to(_dev()) for n in (20, 9, 1)]
    drafts = torch.randint(0, mr.VOCAB, (3, 3), generator=g).to(_dev())
    res = []
    for embed, lm_head in ((e16, l16), (e8, l8)):
        kc, vc = _caches(m, 3)
        args = (m.layers, embed, m.norm, lm_head, kc, vc, m.inv_freq)
        if cls == "RaggedStep":
            st = qp.RaggedStep(*args, rows=32, segments=4)
            st.out_tok.fill_(-7)
            tok = st(*st.pack([(b, s, 0) for b, s in enumerate(seqs)]))
            assert int(tok[3]) == -7
            res.append((st.draw.logits[:3].clone(), tok[:3].clone()))
        elif cls == "SpeculativeStep":
            st = qp.SpeculativeStep(*args, draft=3)
            for b in (0, 1):   # slot 2 has no sequence: no rows
                st.begin(b, seqs[b][:1].tolist())
            st.drawn.fill_(-7)
            st(drafts, torch.full((3,), 3, dtype=torch.int32, device=_dev()))
            live = st.row_ctr >= 0
            assert int(live.sum()) == 8 and bool((st.drawn[~live] == -7).all())
            res.append((st.draw.logits[live].clone(), st.drawn[live].clone()))
        else:
            st = qp.Score(*args, chunk=32)   # (one chunk: st.logits holds every row's)
            lp = st(seqs[0]).clone()
            res.append((st.logits.clone(), lp))
    (la, ta), (lb, tb) = res
    if cls == "Score":
        bound = 2.0 * (2e-3 + 1e-3) * float(la.abs().max())
        assert float((la - lb).abs().max()) <= bound and float((ta - tb).abs().max()) <= 2.0 * bound
        return
    assert torch.equal(tb, lb.argmax(-1))
    _agree(la, ta, lb, tb, cap=1.0)


@pytest.mark.parametrize("B", [1, 4])
def test_decode_step_against_the_fp16_twin(qp, model, B):
    m, (e8, e16), (l8, l16) = model
    ref_l, ref_t = _decode(qp, m, B, e16, l16, True)
    got_l, got_t = _decode(qp, m, B, e8, l8, True)
    _agree(ref_l[:, :got_t.shape[1]], ref_t, got_l[:, :got_t.shape[1]], got_t)
    greedy_l, greedy_t = _decode(qp, m, B, e8, l8, False)
    assert greedy_l is None and torch.equal(greedy_t, got_l[:, :got_t.shape[1]].argmax(-1))
    assert torch.equal(_decode(qp, m, B, e8, l8, False, graph=True)[1], greedy_t)


def test_prefill_against_the_fp16_twin(qp, model):
    m, (e8, e16), (l8, l16) = model
    prompt = torch.randint(0, mr.VOCAB, (20,), generator=torch.Generator().manual_seed(SEED)).to(_dev())
    res = []
    for embed, lm_head in ((e16, l16), (e8, l8), (e8, l8)):   # the third: no sampler, the fused argmax tail
        kc = [torch.zeros(1, m.cfg.num_key_value_heads, 64, m.cfg.head_dim, dtype=torch.float16, device=_dev()) for _ in m.layers]
        smp = qp.Sampler(1, mr.VOCAB, _dev(), temperature=0.0) if len(res) < 2 else None
        pf = qp.Prefill(m.layers, embed, m.norm, lm_head, kc, [t.clone() for t in kc], m.inv_freq, chunk=16, sampler=smp)
        tok = pf(prompt).clone()
        res.append((None if smp is None else smp.logits.clone(), tok))
    _agree(res[0][0], res[0][1], res[1][0], res[1][1])
    assert torch.equal(res[2][1], res[1][0].argmax(-1))


GUARDS = ["dtype", "misaligned", "length", "k a multiple of 512", "rows must be in 1 .. 128", "both outputs", "short workspace"]


@pytest.mark.parametrize("what", GUARDS)
def test_guards(qp, what):
    sp, dev = qp.sampling, _dev()
    w8, s = torch.zeros(64 * 512 + 16, dtype=torch.uint8, device=dev).view(F8), torch.ones(64, device=dev)
    table, h = sp.Table8(w8[:64 * 512].view(64, 512), s), torch.zeros(4, 512, device=dev)
    tok = torch.zeros(4, dtype=torch.int64, device=dev)
    calls = {"dtype": lambda: sp.Table8(torch.zeros(64, 512, dtype=torch.float16, device=dev), s),
             "misaligned": lambda: sp.Table8(w8[8:8 + 64 * 512].view(64, 512), s),
             "length": lambda: sp.Table8(w8[:64 * 512].view(64, 512), s[:63]),
             "k a multiple of 512": lambda: sp.lm_head_logits(torch.zeros(4, 768, device=dev), None, 0.0,
                                                              sp.Table8(w8[:32 * 768].view(32, 768), s[:32])),
             "rows must be in 1 .. 128": lambda: sp.lm_head_logits(torch.zeros(129, 512, device=dev), None, 0.0, table),
             "both outputs": lambda: sp.lm_head_argmax(h, None, 0.0, table, None),
             "short workspace": lambda: sp.lm_head_argmax(h, None, 0.0, table, tok, ws=torch.zeros(8, dtype=torch.int64, device=dev))}
    with pytest.raises(qp._native.QpalError, match=what):
        calls[what]()
