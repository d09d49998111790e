"""calibrate.collect_hessians and calibrate.quantize_model on a small random model.

Model: random_dense_model(hidden=1024, inter=2048, nq=8, nkv=2, nlayers=2, vocab=4096), W = 3 windows of N = 160 tokens: two attention
chunks per window, one of them short.

The collector is held against an independent forward written here in plain torch (its own rotary embedding in qpal_rope_kv's
convention, a causal softmax, fp16 rounding at the four points where a Hessian is taken).  Its activations pass through fp16 matmuls
and the attention kernel, so the tolerance is measured, not derived: the relative Frobenius distance, per Hessian, between that
independent forward run in fp32 and run in fp64; 4 x the largest of them is allowed.  Both figures are printed by the test.

The driver must give layers whose packed buffers, SU and Wscale are, bit for bit, those of seven hand-made quantize_linear calls per
layer with the same signs and load_hessian(file)."""
import math
import os

import pytest
import torch

import qpalette_amd as qp
from qpalette_amd import calibrate
from qpalette_amd import quantize_layer as ql

pytestmark = pytest.mark.gpu
W_, N_ = 3, 160
QSTR = "tcq_6_hess_0.9"


def tlut9():
    """a random Gaussian codebook at the rms the trellis quantiser expects"""
    t = torch.randn(512, 2, generator=torch.Generator().manual_seed(9))
    return (t / t.std(unbiased=False) * 0.9682458365518543).half()


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    qp._native.lib()
    dev = torch.device("cuda", 0)
    model = calibrate.random_dense_model(hidden=1024, inter=2048, nq=8, nkv=2, nlayers=2, vocab=4096, seed=0, device=dev)
    windows = torch.randint(0, 4096, (W_, N_), generator=torch.Generator().manual_seed(1)).to(dev)
    hess_dir = str(tmp_path_factory.mktemp("hess"))
    paths = calibrate.collect_hessians(model, windows, hess_dir=hess_dir)
    return dict(dev=dev, model=model, windows=windows, hess_dir=hess_dir, paths=paths, quant_dir=str(tmp_path_factory.mktemp("quant")))


# ------------------------------------------------------------------------------------------------------------- collector


def _rotate_half(x):
    a, b = x[..., : x.shape[-1] // 2], x[..., x.shape[-1] // 2:]
    return torch.cat((-b, a), dim=-1)


def independent_hessians(model, windows, dt):
    """{(layer, key): X^T X / ct in fp64} of a forward in dtype dt: residual stream, matmuls, rotary embedding and softmax in dt, the
    four Hessian inputs rounded to fp16 (and used at that value), as the collector's are"""
    cfg = model.cfg
    nq, nkv, hd, inter = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim, cfg.intermediate_size
    Wn, N = windows.shape
    out = {}

    def norm(x, m):
        return (x * torch.rsqrt(x.square().mean(-1, keepdim=True) + m.eps) * m.weight.to(dt)).half().to(dt)

    def take(li, key, x):
        x64 = x.reshape(-1, x.shape[-1]).double()
        out[(li, key)] = x64.T @ x64 / x64.shape[0]

    h = model.embed[windows].to(dt)                                                     # [W, N, hidden]
    ang = torch.arange(N, device=h.device).to(dt)[:, None] * model.inv_freq.to(dt)[None, :]
    cos, sin = torch.cat((ang, ang), -1).cos()[None, :, None], torch.cat((ang, ang), -1).sin()[None, :, None]
    keep = torch.ones(N, N, dtype=torch.bool, device=h.device).tril()
    for li, L in enumerate(model.layers):
        x = norm(h, L.input_layernorm)
        take(li, "qkv", x)
        q = (x @ L.q.to(dt).T).view(Wn, N, nq, hd)
        k = (x @ L.k.to(dt).T).view(Wn, N, nkv, hd)
        v = (x @ L.v.to(dt).T).view(Wn, N, nkv, hd)
        q, k = q * cos + _rotate_half(q) * sin, k * cos + _rotate_half(k) * sin
        k, v = k.repeat_interleave(nq // nkv, dim=2), v.repeat_interleave(nq // nkv, dim=2)
        s = torch.einsum("wthd,wshd->whts", q, k) / math.sqrt(hd)
        p = torch.softmax(s.masked_fill(~keep, float("-inf")), -1)
        a = torch.einsum("whts,wshd->wthd", p, v).reshape(Wn, N, nq * hd).half().to(dt)
        take(li, "o", a)
        h = h + a @ L.o.to(dt).T
        x = norm(h, L.post_attention_layernorm)
        take(li, "up", x)
        act = (torch.nn.functional.silu(x @ L.gate.to(dt).T) * (x @ L.up.to(dt).T)).half().to(dt)
        take(li, "down", act)
        h = h + act @ L.down.to(dt).T
    return out


def test_collector_against_an_independent_forward(run):
    """Measured on an MI355X (the test prints both figures per Hessian): the fp32 and the fp64 forward are at most 4.20e-4 apart
    (layer 1 `down`), so 1.68e-3 is allowed; the collector's largest distance from the fp64 forward is 1.05e-3 (layer 1 `down`), its
    smallest 7.5e-6 (layer 0 `qkv`, no attention in front of it)."""
    model, windows = run["model"], run["windows"]
    h32, h64 = independent_hessians(model, windows, torch.float32), independent_hessians(model, windows, torch.float64)
    base = {key: float((h32[key] - h64[key]).norm() / h64[key].norm()) for key in h64}
    tol = 4.0 * max(base.values())
    assert len(run["paths"]) == 8 and set(run["paths"]) == set(h64)
    dist = {}
    for key, path in sorted(run["paths"].items()):
        assert path == os.path.join(run["hess_dir"], f"{key[0]}_{key[1]}.pt") and os.path.exists(path)
        H = ql.load_hessian(path, sigma_reg=0.0).to(windows.device)
        assert torch.equal(H, H.T)
        dist[key] = float((H - h64[key]).norm() / h64[key].norm())
        print(f"{key}: collector vs fp64 forward {dist[key]:.3e}; fp32 vs fp64 forward {base[key]:.3e}")
    print(f"largest fp32-vs-fp64 distance {max(base.values()):.3e}, allowed {tol:.3e}, largest collector distance {max(dist.values()):.3e}")
    assert max(dist.values()) <= tol, (dist, tol)


def test_collector_in_memory_equals_files_and_row_chunking(run):
    """without hess_dir the accumulators come back; the first Hessian (no attention in front of it) does not depend on how rows are
    cut into add() calls beyond the kernel's bound; ct counts every row"""
    model, windows = run["model"], run["windows"]
    accs = calibrate.collect_hessians(model, windows, rows_per_call=96)
    assert set(accs) == set(run["paths"]) and all(a.ct == W_ * N_ for a in accs.values())
    assert accs[(0, "qkv")].n == 1024 and accs[(1, "down")].n == 2048
    # same rows, other cuts: both sums are within the kernel's bound F * 2^-23 * A of the exact one (tests/test_hessian.py)
    H = accs[(0, "qkv")].hessian()
    ref = ql.load_hessian(run["paths"][(0, "qkv")], sigma_reg=0.0).to(H.device)
    ax = model.layers[0].input_layernorm(model.embed[windows.reshape(-1)]).double().abs()
    A = ax.T @ ax / (W_ * N_)
    assert bool(((H - ref).abs() <= (2 * 1.01 * 256 * 2.0 ** -23 + 1e-12) * A).all())


# ----------------------------------------------------------------------------------------------------------------- driver


@pytest.fixture(scope="module")
def quantized(run):
    return calibrate.quantize_model(run["model"], QSTR, run["hess_dir"], run["quant_dir"], codebooks={9: tlut9()}, seed=5)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16) if a.dtype == torch.float16 else a,
                                                                     b.view(torch.int16) if b.dtype == torch.float16 else b)


@pytest.mark.parametrize("li", [0, 1])
def test_driver_equals_seven_hand_made_calls(run, quantized, li):
    model, dev = run["model"], run["dev"]
    L, layer = model.layers[li], quantized[li]
    hand = {}
    for key in calibrate.LINEARS:
        W = L.weight(key)
        H = ql.load_hessian(os.path.join(run["hess_dir"], f"{li}_{calibrate.GROUP[key][0]}.pt"))
        hand[key], _ = ql.quantize_linear(W, QSTR, H=H, SU=calibrate.layer_signs(5, li, key, W.shape[1]), SV=torch.ones(W.shape[0]),
                                          left_only=True, codebooks={9: tlut9()})
        assert os.path.exists(ql.layer_file_path(run["quant_dir"], QSTR, li, key))
    q, k, v, o, u, g, d = (hand[key] for key in calibrate.LINEARS)
    att, mlp = layer.self_attn, layer.mlp
    for mine, ref in ((att.q_proj, q), (att.k_proj, k), (att.v_proj, v), (att.o_proj, o), (mlp.up_proj, u), (mlp.gate_proj, g),
                      (mlp.down_proj, d)):
        assert _same(mine.trellis, ref.linear.trellis) and _same(mine.tlut, ref.linear.tlut)
    assert _same(q.SU, k.SU) and _same(q.SU, v.SU) and _same(u.SU, g.SU) and not _same(q.SU, o.SU)
    assert _same(att.SU_qkv, q.SU) and _same(att.SU_o, o.SU) and _same(mlp.SU_ug, u.SU) and _same(mlp.SU_dp, d.SU)
    assert _same(att.Wscale_qkv, torch.cat([q.Wscale, k.Wscale, v.Wscale])) and _same(att.Wscale_o, o.Wscale)
    assert _same(mlp.Wscale_ug, torch.cat([u.Wscale, g.Wscale])) and _same(mlp.Wscale_dp, d.Wscale)
    assert all(bool((x.SV == 1).all()) for x in hand.values())
    assert layer.input_layernorm.weight is L.input_layernorm.weight and layer.input_layernorm.eps == L.input_layernorm.eps
    assert all(i["use_hess"] and i["quantizer_str"] == QSTR for i in quantized.infos[li].values())


def test_quantizer_dictionary(run, tmp_path):
    """a {layer_linear: string} dictionary: strings without `hess` read no Hessian file (none exists in the empty directory)"""
    model = run["model"]
    qd = {f"{li}_{key}": "tcq_5_none_0.9" if "mlp" in key else "tcq_6_none_0.9" for li in range(2) for key in calibrate.LINEARS}
    layers = calibrate.quantize_model(model, qd, str(tmp_path / "nohess"), str(tmp_path / "q"), codebooks={9: tlut9()})
    assert layers[0].mlp.down_proj.KV == 5 and layers[1].self_attn.q_proj.KV == 6
    with pytest.raises(FileNotFoundError):
        calibrate.quantize_model(model, QSTR, str(tmp_path / "nohess"), str(tmp_path / "q2"), codebooks={9: tlut9()})


def test_score_and_decode_on_the_quantized_layers(run, quantized):
    """Score gives finite log-probabilities for a 160-token window and a DecodeStep continues the slot.  Recorded, not gated: the
    quantized model's nll next to the dense forward's, and top-1 agreement of the two on the window's next tokens."""
    model, dev, windows = run["model"], run["dev"], run["windows"]
    cfg = model.cfg
    shape = (1, cfg.num_key_value_heads, 256, cfg.head_dim)
    kc = [torch.zeros(shape, dtype=torch.float16, device=dev) for _ in quantized]
    vc = [torch.zeros(shape, dtype=torch.float16, device=dev) for _ in quantized]
    sc = qp.Score(quantized, model.embed, model.norm, model.lm_head, kc, vc, model.inv_freq)
    lp = sc(windows[0], slot=0, pos0=0).clone()
    assert lp.shape == (N_ - 1,) and bool(torch.isfinite(lp).all())
    dense = calibrate.dense_logprobs(model, windows[:1])[0]
    assert dense.shape == (N_ - 1,) and bool(torch.isfinite(dense).all())
    print(f"nll quantized {-float(lp.mean()):.4f}, dense {-float(dense.mean()):.4f}; mean |d logprob| {float((lp - dense).abs().mean()):.4f}")
    tok = windows[1, :1].clone()
    pos = torch.tensor([N_], dtype=torch.int64, device=dev)
    out = torch.full((1,), -7, dtype=torch.int64, device=dev)
    before = [t[0, :, N_].clone() for t in kc]
    # (hidden = 1024 is outside the one-launch lm_head + argmax kernel's widths: the tail is the norm module + a matmul)
    qp.DecodeStep(quantized, model.embed, model.norm, model.lm_head, kc, vc, model.inv_freq, tok, pos, out, native_lm_head=False)()
    torch.cuda.synchronize()
    assert 0 <= int(out[0]) < 4096
    assert all(not torch.equal(t[0, :, N_], b) for t, b in zip(kc, before))
