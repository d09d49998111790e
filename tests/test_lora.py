"""Multi-adapter LoRA on the GPU (csrc/lora.hip, qpalette_amd.lora, the step classes' `adapters=`).

Kernel: qpal_lora_apply against reference_lora (numpy fp64 on the stored values; tests/test_lora_spec.py holds that to hand-made
cases).  Per element  |got - ref| <= 2e-5 * sum_r |B_jr| * sum_l |A_rl xin_l| + 2^-23 |ref|:  the project's fp32-sum bar (1e-5 *
sum |w x|, tests/test_gpu_parity.py) once for each of the two chained sums, plus the final fp32 add.  Rows without an adapter and
columns outside the blocks keep their bytes.  Two launches are bitwise equal; a row's bits do not depend on where it stands or on
the other rows.

Whole model: the yardstick is a test-local DecodeStep(generic=True) that runs the parent's GEMVs and adds every delta with torch
fp32 ops from the RAW (A, B, alpha) dictionaries — not from the bank's packed tensors.  The adapters are scaled until, on the
yardstick alone, they move the logits by at least 8 x the bound; then DecodeStep (B = 4, and the batch-1 step), Prefill + decode,
RaggedStep, a captured step with an adapter swapped between replays, Score and SpeculativeStep are held to it within
2^-7 max(1, max |ref|), the bound test_paged_kv.py and test_spec.py use between two routes through the same model."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import qpalette_amd as qp
from qpalette_amd import hadamard as had
from qpalette_amd import sampling
from qpalette_amd.hadamard import IN_F16, IN_F32, IN_SWIGLU_F32

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = qp._native.QpalError


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


# ----------------------------------------------------------------------------------------------------------------- kernel

N_AD, ROWS, RANKS = 3, (1, 5, 16, 17, 128), (8, 16, 64)
MODES = {"4096-f16": (4096, IN_F16, None), "4096-f32-rms-weight": (4096, IN_F32, "weight"), "4096-f32-rms": (4096, IN_F32, "plain"),
         "2048-f32": (2048, IN_F32, None), "14336-swiglu": (14336, IN_SWIGLU_F32, None)}
# (blk_off, blk_m, ld_out): ld_out > sum blk_m in every layout; the first has gaps in front of, between and behind its blocks
BLOCKS = {"q-k-v": ([32, 4096 + 96, 5120 + 112], [4096, 1024, 1024], 6144 + 144), "one": ([16], [4096], 4096 + 48),
          "up-gate": ([0, 14336], [14336, 14336], 2 * 14336 + 16)}
EPS = 1e-5


def _row_adapters(rows):
    """0, 1, 2, -1 and one id out of range (N), mixed; one row: adapter 1"""
    ra = np.array([(1, -1, 0, 2, N_AD, 0, 2, 1, -1)[i % 9] for i in range(rows)], np.int32)
    return ra


def _inputs(k, mode, rms, blk_m, ld_out, seed):
    """the largest case (128 rows, rank 64) of one (k, mode, blocks); smaller ranks and row counts are slices of it"""
    rng = np.random.default_rng(seed)
    P, M = len(blk_m), sum(blk_m)
    A = (rng.standard_normal((N_AD, P * 64, k), dtype=np.float32) / np.sqrt(k)).astype(np.float16)
    B = (rng.standard_normal((N_AD, M, 64), dtype=np.float32) * 0.25).astype(np.float16)
    x = rng.standard_normal((128, 2 * k if mode == IN_SWIGLU_F32 else k), dtype=np.float32) * 1.5
    x = x.astype(np.float16) if mode == IN_F16 else x
    w = (1.0 + 0.25 * rng.standard_normal(k, dtype=np.float32)).astype(np.float16) if rms == "weight" else None
    out = rng.standard_normal((128, ld_out), dtype=np.float32) * 4.0
    return A, B, x, w, out


def _rank_slice(A, B, P, R):
    """rank R of the rank-64 master: rows p 64 .. p 64 + R - 1 of every block of A, columns 0 .. R - 1 of B"""
    idx = np.concatenate([np.arange(p * 64, p * 64 + R) for p in range(P)])
    return np.ascontiguousarray(A[:, idx]), np.ascontiguousarray(B[:, :, :R])


@pytest.mark.parametrize("blocks", list(BLOCKS))
@pytest.mark.parametrize("case", list(MODES))
def test_kernel_is_the_reference(dev, case, blocks):
    """every rows x rank of one (k, mode) x block layout: the reference is computed once per rank on 128 rows (a row's sums do not
    depend on the other rows), the launches of 1, 5, 16, 17 and 128 rows are held to its first rows"""
    k, mode, rms = MODES[case]
    blk_off, blk_m, ld_out = BLOCKS[blocks]
    P = len(blk_m)
    A64m, B64m, x, w, out0 = _inputs(k, mode, rms, blk_m, ld_out, seed=sum(map(ord, case + blocks)))
    ra = _row_adapters(128)
    rms_arg = None if rms is None else (EPS, w)
    x_d, out0_d = torch.from_numpy(x).to(dev), torch.from_numpy(out0).to(dev)
    w_d = None if w is None else torch.from_numpy(w).to(dev)
    inside = np.zeros(ld_out, bool)
    for o, m in zip(blk_off, blk_m):
        inside[o:o + m] = True
    assert not inside.all()
    worst = 0.0
    for R in RANKS:
        A, B = _rank_slice(A64m, B64m, P, R)
        ref, scale = qp.reference_lora(out0, x, mode, rms_arg, A, B, blk_off, blk_m, ra, return_scale=True)
        bound = 2e-5 * scale + 2.0 ** -23 * np.abs(ref)
        A_d, B_d = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)
        for rows in ROWS:
            ra_r = _row_adapters(rows)
            assert np.array_equal(ra_r, ra[:rows])
            out = out0_d[:rows].clone()
            qp.lora_apply(out, x_d[:rows].contiguous(), mode, None if rms is None else (EPS, w_d), A_d, B_d, blk_off, blk_m,
                          torch.from_numpy(ra_r).to(dev))
            got = out.cpu().numpy()
            live = (ra_r >= 0) & (ra_r < N_AD)
            # rows with no adapter, and every column outside the blocks: the bytes of the pre-fill
            assert np.array_equal(got[~live].view(np.uint32), out0[:rows][~live].view(np.uint32)), (R, rows)
            assert np.array_equal(got[:, ~inside].view(np.uint32), out0[:rows][:, ~inside].view(np.uint32)), (R, rows)
            err = np.abs(got.astype(np.float64) - ref[:rows])
            sel = np.ix_(live, inside)
            ratio = float((err[sel] / bound[:rows][sel]).max())
            worst = max(worst, ratio)
            assert np.mean(got[sel] != out0[:rows][sel]) > 0.999, "adapter rows kept their pre-fill: nothing was added"
            assert ratio <= 1.0, (case, blocks, R, rows, ratio)
    print(f"lora {case} {blocks}: largest |got - ref| / bound over ranks {RANKS} x rows {ROWS} = {worst:.4f}")


def _small(dev, mode, seed, rows=17, k=4096, R=16):
    blk_off, blk_m, ld_out = BLOCKS["q-k-v"]
    rms = "weight" if mode == IN_F32 else None
    A, B, x, w, out0 = _inputs(k, mode, rms, blk_m, ld_out, seed)
    A, B = _rank_slice(A, B, 3, R)
    t = lambda a: torch.from_numpy(a).to(dev)
    return t(A), t(B), t(x[:rows].copy()), (None if w is None else (EPS, t(w))), t(out0[:rows].copy()), blk_off, blk_m


@pytest.mark.parametrize("mode", [IN_F16, IN_F32, IN_SWIGLU_F32], ids=["f16", "f32-rms", "swiglu"])
def test_kernel_properties(dev, mode):
    """equal launches give equal bits; a row's bits do not change when it moves to another row index or when the other rows'
    inputs and adapters change (same launch shape); a launch whose rows all have no adapter leaves out byte-equal"""
    A, B, x, rms, out0, blk_off, blk_m = _small(dev, mode, seed=5, k=4096 if mode != IN_SWIGLU_F32 else 2048)
    rows = x.shape[0]
    ra = torch.from_numpy(_row_adapters(rows)).to(dev)
    run = lambda o, xx, rr: qp.lora_apply(o.clone(), xx, mode, rms, A, B, blk_off, blk_m, rr)
    first, again = run(out0, x, ra), run(out0, x, ra)
    assert torch.equal(first.view(torch.int32), again.view(torch.int32))
    assert not torch.equal(first.view(torch.int32), out0.view(torch.int32))
    # row 3 (adapter 2) moves to index 11; the other rows get other inputs, other out values and other adapters
    g = torch.Generator(device=dev).manual_seed(1)
    x2 = (torch.randn(x.shape, device=dev, generator=g) * 2).to(x.dtype)
    out2 = torch.randn(out0.shape, device=dev, generator=g)
    ra2 = torch.roll(ra, 4)
    x2[11], out2[11], ra2[11] = x[3], out0[3], ra[3]
    moved = run(out2, x2, ra2)
    assert int(ra[3]) == 2 and torch.equal(moved[11].view(torch.int32), first[3].view(torch.int32))
    assert not torch.equal(moved[3].view(torch.int32), first[3].view(torch.int32))
    none = run(out0, x, torch.full_like(ra, -1))
    assert torch.equal(none.view(torch.int32), out0.view(torch.int32))
    beyond = run(out0, x, torch.full_like(ra, N_AD))
    assert torch.equal(beyond.view(torch.int32), out0.view(torch.int32))


@pytest.mark.parametrize("k,mode", [(28672, IN_F32), (32768, IN_F16), (8192, IN_SWIGLU_F32), (3072, IN_F32)], ids=str)
def test_kernel_widest_inputs(dev, k, mode):
    """k = 28672 and 32768: the staged row needs more than 64 KiB of LDS (the opt-in path); 8192 and 3072: the other widths the
    kernel must take.  Same bound, 3 rows, rank 8 and 64, one block of 48 columns (a split that is not full)"""
    rms = "weight" if mode == IN_F32 else None
    A64m, B64m, x, w, out0 = _inputs(k, mode, rms, [48], 80, seed=k)
    x, out0, ra = x[:3].copy(), out0[:3].copy(), np.array([2, -1, 0], np.int32)
    for R in (8, 64):
        A, B = _rank_slice(A64m, B64m, 1, R)
        ref, scale = qp.reference_lora(out0, x, mode, None if rms is None else (EPS, w), A, B, [16], [48], ra, return_scale=True)
        t = lambda a: torch.from_numpy(a).to(dev)
        got = qp.lora_apply(t(out0), t(x), mode, None if rms is None else (EPS, t(w)), t(A), t(B), [16], [48], t(ra)).cpu().numpy()
        ratio = np.abs(got - ref)[[0, 2], 16:64] / (2e-5 * scale + 2.0 ** -23 * np.abs(ref))[[0, 2], 16:64]
        print(f"lora k = {k} R = {R}: largest |got - ref| / bound = {float(ratio.max()):.4f}")
        assert float(ratio.max()) <= 1.0
        keep = np.ones(out0.shape, bool)
        keep[[0, 2], 16:64] = False
        assert np.array_equal(got[keep].view(np.uint32), out0[keep].view(np.uint32)) and np.all(got[~keep] != out0[~keep])


def test_kernel_argument_errors(dev):
    """R = 12, k = 100, P = 4, blk_m = 24, a misaligned A: each its code, decided on the host — out keeps its bytes"""
    lib = qp._native.lib()
    rows, k, R, N = 4, 256, 16, 2
    out0 = torch.randn(rows, 256, device=dev)
    out = out0.clone()
    x = torch.randn(rows, k, device=dev)
    A = torch.randn(N * 4 * R * k + 8, device=dev).half()
    B = torch.randn(N * 256 * R, device=dev).half()
    ra = torch.zeros(rows, dtype=torch.int32, device=dev)
    SHAPE, PARAM, NULL, ALIGN = -1, -2, -3, -4

    def call(R=R, k=k, P=2, blk_off=(0, 128), blk_m=(64, 64), A_ptr=None, in_mode=IN_F32, eps=-1.0, rows=rows, ld_out=256, x_ptr=None):
        arr = ctypes.c_int * len(blk_m)
        return lib.qpal_lora_apply(out.data_ptr(), ld_out, x.data_ptr() if x_ptr is None else x_ptr, in_mode, eps, None,
                                   A.data_ptr() if A_ptr is None else A_ptr, B.data_ptr(), arr(*blk_off), arr(*blk_m), P, ra.data_ptr(),
                                   rows, k, R, N, torch.cuda.current_stream(dev).cuda_stream)

    for kw, code in ((dict(R=12), SHAPE), (dict(k=100), SHAPE), (dict(P=4, blk_off=(0, 64, 128, 192), blk_m=(64,) * 4), SHAPE),
                     (dict(blk_m=(64, 24)), SHAPE), (dict(A_ptr=A.data_ptr() + 2), ALIGN), (dict(R=72), SHAPE), (dict(R=0), SHAPE),
                     (dict(rows=129), SHAPE), (dict(rows=0), SHAPE), (dict(k=32768 + 64), SHAPE), (dict(blk_off=(0, 32)), SHAPE),
                     (dict(ld_out=128), SHAPE), (dict(in_mode=3), PARAM), (dict(in_mode=IN_F16, eps=1e-5), PARAM),
                     (dict(A_ptr=0), NULL), (dict(x_ptr=out.data_ptr()), PARAM)):
        assert call(**kw) == code, (kw, code)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), out0.view(torch.int32))
    assert call() == 0
    torch.cuda.synchronize()
    assert not torch.equal(out.view(torch.int32), out0.view(torch.int32))
    # the host wrapper names the argument
    A3, B3 = A[:N * 2 * R * k].view(N, 2 * R, k), B[:N * 128 * R].view(N, 128, R)
    ok = dict(out=out, x=x, in_mode=IN_F32, rms=None, A=A3, B=B3, blk_off=[0, 128], blk_m=[64, 64], row_adapter=ra)
    for change, named in ((dict(B=B[:N * 128 * 12].view(N, 128, 12)), "rank"), (dict(blk_m=[104, 24]), "blk_m"),
                          (dict(blk_off=[0, 32]), "blk_off"), (dict(A=A[1:N * 2 * R * k + 1].view(N, 2 * R, k)), "A must"),
                          (dict(x=x.half()), "x must"), (dict(row_adapter=ra.long()), "row_adapter"), (dict(rms=(1e-5, x[0])), "rms weight"),
                          (dict(in_mode=IN_F16, x=x.half(), rms=(1e-5, None)), "rms needs"), (dict(out=out.half()), "out must")):
        with pytest.raises(E, match=named):
            qp.lora_apply(**{**ok, **change})


# -------------------------------------------------------------------------------------------------------------- whole model

NB, L, VOCAB, PROMPT, NEW = 4, 128, 4096, 40, 8
SLOT_ADAPTER = [0, 1, -1, 0]
RANK = {0: 16, 1: 8}
TOKEN_SEED = 11
LINEARS = qp.lora.LINEARS


@pytest.fixture(scope="module")
def model(dev):
    sys.path.insert(0, os.path.join(ROOT, "perf"))
    from decode_llama import build_model
    return build_model("3_8b", "tcomb_6_7_0.5_none_0.9", None, 2, VOCAB, dev)


def _bound(l):
    l = np.asarray(l)
    return 2.0 ** -7 * max(1.0, float(np.abs(l[np.isfinite(l)]).max()))


def _caches(m, dev, B=NB):
    nkv, hd = m.cfg.num_key_value_heads, m.cfg.head_dim
    mk = lambda: torch.zeros(B, nkv, L, hd, dtype=torch.float16, device=dev)
    return [mk() for _ in m.layers], [mk() for _ in m.layers]


def _raw_adapters(m, scale):
    """{adapter: (weights, alpha)} on all seven linears of both layers, fp32, as a training run would leave them (CPU)"""
    H, I, kv = m.cfg.hidden_size, m.cfg.intermediate_size, m.cfg.num_key_value_heads * m.cfg.head_dim
    shapes = {"self_attn.q_proj": (H, H), "self_attn.k_proj": (H, kv), "self_attn.v_proj": (H, kv), "self_attn.o_proj": (H, H),
              "mlp.up_proj": (H, I), "mlp.gate_proj": (H, I), "mlp.down_proj": (I, H)}
    g = torch.Generator().manual_seed(2024)
    res = {}
    for a, r in RANK.items():
        w = {f"{i}_{lin}": (torch.randn(r, shapes[lin][0], generator=g) / shapes[lin][0] ** 0.5, torch.randn(shapes[lin][1], r, generator=g) * scale)
             for i in range(len(m.layers)) for lin in LINEARS}
        res[a] = (w, 2.0 * r)
    return res


def _bank(m, dev, raw, slot_adapter=SLOT_ADAPTER):
    bank = qp.LoraBank(m.layers, n_adapters=2, rank=16, B_slots=len(slot_adapter), device=dev)
    for a, (w, alpha) in raw.items():
        bank.load(a, w, alpha)
    for s, a in enumerate(slot_adapter):
        bank.set(s, a)
    return bank


class _Yardstick(qp.DecodeStep):
    """DecodeStep(generic=True) without a bank: the parent's GEMV launches, and behind each projection group the deltas of the RAW
    adapters, (alpha / r) B (A xin), added by torch fp32 ops row by row"""

    def __init__(self, m, dev, kc, vc, tok, pos, out, smp, raw, slot_adapter):
        super().__init__(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, tok, pos, out, generic=True, sampler=smp)
        self.raw = {a: ({k: (A.to(dev), B.to(dev)) for k, (A, B) in w.items()}, alpha) for a, (w, alpha) in raw.items()}
        self.slot_adapter = slot_adapter

    def _delta(self, i, lin, xin, out):
        for b, a in enumerate(self.slot_adapter):
            if a >= 0:
                (A, B), alpha = self.raw[a][0][f"{i}_{lin}"], self.raw[a][1]
                out[b] += (alpha / A.shape[0]) * (B @ (A @ xin[b]))

    @staticmethod
    def _normed(h32, eps, w):
        return h32 * torch.rsqrt(h32.square().mean(-1, keepdim=True) + eps) * w.float()

    def _layer(self, i, h32, a16, qkv32, ug32):
        layer = self.layers[i]
        att = layer.self_attn
        proj, wsc, blocks = att._qkv_layout()
        xin = self._normed(h32, self.eps, layer.input_layernorm.weight)
        self._gemv(proj, h32, att.SU_qkv, att.scale, rms=(self.eps, layer.input_layernorm.weight), wscales=wsc,
                   outs=list(qkv32.split([l.out_features for l in proj], dim=1)))
        parts = dict(zip([b[0] for b in blocks], qkv32.split([b[1] for b in blocks], dim=1)))
        for name in "qkv":
            self._delta(i, f"self_attn.{name}_proj", xin, parts[name])
        self._attention(i, parts["q"], parts["k"], parts["v"], a16)
        self._gemv([att.o_proj], a16, att.SU_o, att.scale, wscales=[att.Wscale_o], outs=[h32], accumulate=True)
        self._delta(i, "self_attn.o_proj", a16.float(), h32)
        self._mlp(i, h32, ug32)

    def _mlp(self, i, h32, ug32):
        mlp, w = self.layers[i].mlp, self.layers[i].post_attention_layernorm.weight
        inter = mlp.intermediate_size
        xin = self._normed(h32, self.eps, w)
        ugl, ugw = qp.decoder.ug_layout(mlp)
        self._gemv(ugl, h32, mlp.SU_ug, mlp.scale, rms=(self.eps, w), wscales=ugw, outs=list(ug32.split([l.out_features for l in ugl], dim=1)))
        self._delta(i, "mlp.up_proj", xin, ug32[:, :inter])
        self._delta(i, "mlp.gate_proj", xin, ug32[:, inter:])
        x = had.rotate(ug32, in_mode=IN_SWIGLU_F32, hadK=mlp.had_left_dp_T, K=mlp.inter_K, su=mlp.SU_dp, post_scale=1.0 / mlp.scale)
        qp.multi_gemv([mlp.down_proj], x, outs=[h32], wscales=[mlp.Wscale_dp], oscale=mlp.scale, accumulate=True)
        self._delta(i, "mlp.down_proj", torch.nn.functional.silu(ug32[:, inter:]) * ug32[:, :inter], h32)


def _feed(step, tok, pos, smp, tokens, t0, t1):
    """teacher-forced decode steps t0 .. t1 - 1 (tokens [NB or 1, T]); returns the logits of every step [t1 - t0, B, VOCAB]"""
    res = []
    for t in range(t0, t1):
        tok.copy_(tokens[:, t])
        pos.fill_(t)
        step()
        res.append(smp.logits.cpu().numpy().copy())
    return np.stack(res)


@pytest.fixture(scope="module")
def world(dev, model):
    """tokens [NB, PROMPT + NEW]; the yardstick's logits of every position with the adapters, and without (for the size of the
    adapters' effect); the raw adapters, scaled up until the yardstick alone shows them at 8 x the bound or more.  Computed once."""
    m = model
    tokens = torch.randint(0, VOCAB, (NB, PROMPT + NEW), generator=torch.Generator().manual_seed(TOKEN_SEED)).to(dev)

    def yard(raw, slot_adapter):
        kc, vc = _caches(m, dev)
        tok, pos, out = (torch.zeros(NB, dtype=torch.long, device=dev) for _ in range(3))
        smp = qp.Sampler(NB, VOCAB, dev, temperature=0.0)
        return _feed(_Yardstick(m, dev, kc, vc, tok, pos, out, smp, raw, slot_adapter), tok, pos, smp, tokens, 0, PROMPT + NEW)

    base = yard({}, [-1] * NB)
    for scale in (0.02, 0.08, 0.32, 1.28):
        raw = _raw_adapters(m, scale)
        ref = yard(raw, SLOT_ADAPTER)
        moved = min(float(np.abs(ref[t, b] - base[t, b]).max()) / _bound(ref[t, b]) for t in range(PROMPT + NEW) for b in (0, 1, 3))
        print(f"yardstick: adapter scale {scale}: the adapters move the logits by at least {moved:.1f} x the bound")
        if moved >= 8.0:
            break
    assert moved >= 8.0, "the yardstick does not show the adapters: scale them up"
    assert max(float(np.abs(ref[t, 2] - base[t, 2]).max()) / _bound(base[t, 2]) for t in range(PROMPT + NEW)) <= 1.0
    return dict(tokens=tokens, ref=ref, base=base, raw=raw)


def _agree(got, ref, what):
    """got, ref [..., VOCAB]: every row within its bound; prints the largest share of the bound and whether the bits are equal"""
    got, ref = np.asarray(got).reshape(-1, VOCAB), np.asarray(ref).reshape(-1, VOCAB)
    share = max(float(np.abs(g - r).max()) / _bound(r) for g, r in zip(got, ref))
    print(f"{what}: largest |d logit| = {share:.4f} x the bound; bitwise equal: {np.array_equal(got.view(np.uint32), ref.view(np.uint32))}")
    assert np.isfinite(got).all() and share <= 1.0, (what, share)


def _decode(m, dev, kc, vc, bank, B=NB, **kw):
    tok, pos, out = (torch.zeros(B, dtype=torch.long, device=dev) for _ in range(3))
    smp = qp.Sampler(B, VOCAB, dev, temperature=0.0)
    return qp.DecodeStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, tok, pos, out, sampler=smp, adapters=bank, **kw), tok, pos, smp


def test_decode_step_batch_4(dev, model, world):
    m, T = model, PROMPT + NEW
    bank = _bank(m, dev, world["raw"])
    step, tok, pos, smp = _decode(m, dev, *_caches(m, dev), bank)
    plain, tok0, pos0, smp0 = _decode(m, dev, *_caches(m, dev), None)
    assert step.launches_per_token == plain.launches_per_token + 4 * len(m.layers)
    got = _feed(step, tok, pos, smp, world["tokens"], 0, T)
    _agree(got, world["ref"], "DecodeStep B = 4 against the yardstick")
    # slot 2 has no adapter: the step without a bank
    none = _feed(plain, tok0, pos0, smp0, world["tokens"], 0, T)
    _agree(got[:, 2], none[:, 2], "slot 2 (no adapter) against a step without a bank")
    with pytest.raises(E, match="adapters"):
        _decode(m, dev, *_caches(m, dev), _bank(m, dev, world["raw"], [0, 1]))     # a bank of 2 slots on a step of 4


def test_decode_step_batch_1(dev, model, world):
    """the batch-1 step (GEMV-staged RMSNorm and rotation; up | gate in memory) with adapter 0 against the yardstick's slot 0"""
    m, T = model, PROMPT + NEW
    bank = _bank(m, dev, world["raw"], [0])
    step, tok, pos, smp = _decode(m, dev, *_caches(m, dev, 1), bank, B=1)
    plain = _decode(m, dev, *_caches(m, dev, 1), None, B=1)[0]
    assert step.batch1 and step.rot_in_gemv and step.ug_il is None and plain.ug_il is not None
    assert step.launches_per_token == (6 + 4) * len(m.layers) + 2
    got = _feed(step, tok, pos, smp, world["tokens"][:1], 0, T)
    _agree(got[:, 0], world["ref"][:, 0], "DecodeStep B = 1 against the yardstick's slot 0")


def _prefilled(m, dev, bank, tokens, slots=range(NB), n=PROMPT):
    """fresh caches with tokens[b, :n] prefilled into the slots; returns (kc, vc, the logits of each slot's last prompt row)"""
    kc, vc = _caches(m, dev)
    smp = qp.Sampler(NB, VOCAB, dev, temperature=0.0)
    pf = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, chunk=32, sampler=smp, adapters=bank)
    last = {}
    for b in slots:
        pf(tokens[b, :n], slot=b, pos0=0)
        last[b] = smp.logits[b].cpu().numpy().copy()
    return kc, vc, last


def test_prefill_then_decode(dev, model, world):
    m = model
    bank = _bank(m, dev, world["raw"])
    kc, vc, last = _prefilled(m, dev, bank, world["tokens"])   # 40 tokens in chunks of 32: a full and a short chunk
    _agree(np.stack([last[b] for b in range(NB)]), world["ref"][PROMPT - 1], "Prefill (40 tokens) against the yardstick")
    step, tok, pos, smp = _decode(m, dev, kc, vc, bank)
    got = _feed(step, tok, pos, smp, world["tokens"], PROMPT, PROMPT + NEW)
    _agree(got, world["ref"][PROMPT:], "8 DecodeStep steps after Prefill against the yardstick")


def test_ragged_step(dev, model, world):
    """one step: the 40-row prompt of slot 3 (adapter 0) and one decode token each of slots 1 (adapter 1), 0 (adapter 0) and 2 (none)"""
    m, tokens = model, world["tokens"]
    bank = _bank(m, dev, world["raw"])
    kc, vc, _ = _prefilled(m, dev, bank, tokens, slots=(0, 1, 2))
    rs = qp.RaggedStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, rows=64, segments=6, adapters=bank)
    items = [(3, tokens[3, :PROMPT], 0), (1, tokens[1, PROMPT:PROMPT + 1], PROMPT), (0, tokens[0, PROMPT:PROMPT + 1], PROMPT),
             (2, tokens[2, PROMPT:PROMPT + 1], PROMPT)]
    rs(*rs.pack(items))
    torch.cuda.synchronize()
    assert rs.row_adapter.tolist() == [0] * PROMPT + [1, 0, -1] + [-1] * (64 - PROMPT - 3)
    got = rs.draw.logits.cpu().numpy()
    want = np.stack([world["ref"][PROMPT - 1, 3], world["ref"][PROMPT, 1], world["ref"][PROMPT, 0], world["ref"][PROMPT, 2]])
    _agree(got[:4], want, "RaggedStep (a prompt chunk + three decode tokens) against the yardstick")


def test_captured_step_takes_a_new_adapter_between_replays(dev, model, world):
    m, tokens = model, world["tokens"]
    bank = _bank(m, dev, world["raw"])
    kc, vc, _ = _prefilled(m, dev, bank, tokens)
    step, tok, pos, smp = _decode(m, dev, kc, vc, bank)
    tok.copy_(tokens[:, PROMPT])
    pos.fill_(PROMPT)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        step()  # warm-up (the row it appends is appended again by every replay)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            step()
        g.replay()
        torch.cuda.synchronize()
        first = smp.logits.cpu().numpy().copy()
        bank.set(1, 0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        second = smp.logits.cpu().numpy().copy()
    _agree(first, world["ref"][PROMPT], "captured DecodeStep, first replay, against the yardstick")
    # an eager step built with the new assignment, on the same caches (slot 1's prompt rows were written under adapter 1 in both)
    eager, tok_e, pos_e, smp_e = _decode(m, dev, kc, vc, _bank(m, dev, world["raw"], [0, 0, -1, 0]))
    want = _feed(eager, tok_e, pos_e, smp_e, tokens, PROMPT, PROMPT + 1)[0]
    _agree(second, want, "second replay after bank.set(1, 0) against an eager step built with that assignment")
    moved = float(np.abs(second[1] - first[1]).max()) / _bound(first[1])
    print(f"slot 1 moved by {moved:.1f} x the bound")
    assert moved > 8.0
    for b in (0, 2, 3):
        assert float(np.abs(second[b] - first[b]).max()) <= _bound(first[b])


def test_score_with_an_adapter(dev, model, world):
    """Score's log-probabilities of slot 1's 48 tokens (adapter 1) against reference_logprob of the yardstick's logits.  Logits
    within b = 2^-7 max(1, max |ref|) put a log-probability within 2 b (the token's logit and the log-sum-exp move by at most b
    each); test_score.py's delta for the log-prob kernel itself comes on top."""
    m, tokens = model, world["tokens"]
    bank = _bank(m, dev, world["raw"])
    kc, vc = _caches(m, dev)
    sc = qp.Score(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, chunk=32, adapters=bank)
    for slot in (1, 2):
        lp = sc(tokens[slot], slot=slot, pos0=0).cpu().numpy()
        toks, worst = tokens[slot].tolist(), 0.0
        assert lp.shape == (PROMPT + NEW - 1,)
        for t in range(PROMPT + NEW - 1):
            row = world["ref"][t, slot]
            want = sampling.reference_logprob(row, toks[t + 1])[0]
            tol = 2.0 * _bound(row) + 2.0 ** -15 + 2.0 ** -22 * float(np.abs(row).max())
            worst = max(worst, abs(float(lp[t]) - want) / tol)
        print(f"Score slot {slot}: largest |d logprob| = {worst:.4f} x the tolerance")
        assert worst <= 1.0


# of the prompt seeds 31 .. 50, 36 and 45 leave no position of the yardstick stream within the excuse threshold; 36 has the larger
# least gap (1.35 x the threshold against 1.14; recorded on an MI355X)
SPEC_SEED = 36


def _greedy_stream(m, dev, bank, seed):
    """prompts of 17 and 40 tokens for slots 0 and 1; the stream of DecodeStep(generic=True) with the bank: Prefill of all but the
    last prompt token, then NEW greedy tokens, one per step.  Returns (prompts, tokens [2][NEW], logits [2][NEW], the positions
    whose two largest logits are within twice the bound)"""
    prompts = [torch.randint(0, VOCAB, (n,), generator=torch.Generator().manual_seed(seed + n)).to(dev) for n in (17, 40)]
    kc, vc = _caches(m, dev)
    pf = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, adapters=bank)
    for b, p in enumerate(prompts):
        pf(p[:-1], slot=b, pos0=0)
    step, tok, pos, smp = _decode(m, dev, kc, vc, bank, generic=True)
    tok[:2] = torch.stack([p[-1] for p in prompts])
    pos.fill_(-1)
    pos[:2] = torch.tensor([p.shape[0] - 1 for p in prompts], device=dev)
    want, logits = [[], []], [[], []]
    for _ in range(NEW):
        step()
        lg = smp.logits.cpu().numpy()
        for b in range(2):
            want[b].append(int(step.out_tok[b]))
            logits[b].append(lg[b].copy())
        tok[:2] = step.out_tok[:2]
        pos[:2] += 1
    close = sum(1 for b in range(2) for l in logits[b] if float(np.diff(np.sort(l)[-2:])[0]) < 2 * _bound(l))
    return prompts, want, logits, close


def test_speculative_step_emits_the_decode_stream(dev, model, world):
    """8 greedy tokens of slots 0 (adapter 0) and 1 (adapter 1): SpeculativeStep with the bank against the stream of
    DecodeStep(generic=True) with the same bank, token for token.  A first difference is excused only where the yardstick's two
    largest logits of that step are within twice the bound (test_spec.py's rule); at most one position of the run."""
    m = model
    bank = _bank(m, dev, world["raw"])
    prompts, want, logits, close = _greedy_stream(m, dev, bank, SPEC_SEED)
    print(f"yardstick stream: {close} of {2 * NEW} positions have their two largest logits within twice the bound")
    assert close <= 1, "pick another SPEC_SEED: the yardstick alone must leave at most one position that could be excused"
    kc, vc = _caches(m, dev)
    pf = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, adapters=bank)
    ss = qp.SpeculativeStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, draft=4, gram=(2, 4), adapters=bank)
    for b, p in enumerate(prompts):
        pf(p[:-1], slot=b, pos0=0)
        ss.begin(b, p.tolist(), limit=p.shape[0] + NEW)
    got = [[], []]
    for _ in range(NEW + 1):
        if not bool((ss.n_tok < ss.limit).any()):
            break
        out_tok, n_out = ss()
        for b in range(2):
            got[b] += out_tok[b, :int(n_out[b])].tolist()
    excused = 0
    for b in range(2):
        assert len(got[b]) == NEW, (b, got[b])
        for i in range(NEW):
            if got[b][i] != want[b][i]:
                l = logits[b][i]
                assert abs(float(l[got[b][i]]) - float(l[want[b][i]])) < 2 * _bound(l), (b, i, got[b], want[b])
                excused += 1
                break
    print(f"SpeculativeStep with adapters: {excused} excused position(s); streams equal: {got == want}")
    assert excused <= 1
