"""The LoRA contract and its host side without a GPU (qpalette_amd/lora.py): reference_lora on hand-made cases
against explicit fp64 formulas, LoraBank packing on CPU tensors, load_peft_adapter round trip and rejections."""
import json
import re
import types

import numpy as np
import pytest
import torch

import qpalette_amd as qp
from qpalette_amd.hadamard import IN_F16, IN_F32, IN_SWIGLU_F32

F16 = np.float16


def _case(seed, rows=4, k=64, R=8, blk_m=(32, 16), N=2, ld_out=80, mode=IN_F16):
    rng = np.random.default_rng(seed)
    P, M = len(blk_m), sum(blk_m)
    A = rng.standard_normal((N, P * R, k)).astype(F16)
    B = rng.standard_normal((N, M, R)).astype(F16)
    width = 2 * k if mode == IN_SWIGLU_F32 else k
    x = rng.standard_normal((rows, width)).astype(F16 if mode == IN_F16 else np.float32)
    out = rng.standard_normal((rows, ld_out)).astype(np.float32)
    return out, x, A, B


def _explicit(out, xin, A, B, blk_off, blk_m, row_adapter):
    """element by element, straight from the statement of the contract"""
    res = out.astype(np.float64)
    R = B.shape[2]
    for i, a in enumerate(row_adapter):
        if not 0 <= a < A.shape[0]:
            continue
        boff = 0
        for p, (off, m) in enumerate(zip(blk_off, blk_m)):
            for j in range(m):
                s = 0.0
                for r in range(R):
                    t = float(np.dot(A[a, p * R + r].astype(np.float64), xin[i]))
                    s += float(B[a, boff + j, r]) * t
                res[i, off + j] += s
            boff += m
    return res


def test_rows_without_an_adapter_and_columns_outside_the_blocks_are_untouched():
    out, x, A, B = _case(1)
    blk_off, blk_m = [40, 8], [32, 16]  # columns 0 .. 7, 24 .. 39 and 72 .. 79 belong to no block; ld_out = 80 > 48
    ra = [0, -1, 1, 2]                   # 2 = N: out of range
    got = qp.reference_lora(out, x, IN_F16, None, A, B, blk_off, blk_m, ra)
    assert got.dtype == np.float64 and got.shape == out.shape
    for i in (1, 3):
        assert np.array_equal(got[i], out[i].astype(np.float64))
    inside = np.zeros(80, bool)
    inside[40:72] = inside[8:24] = True
    assert np.array_equal(got[:, ~inside], out[:, ~inside].astype(np.float64))
    assert np.all(got[0, inside] != out[0, inside]) and np.all(got[2, inside] != out[2, inside])
    ref = _explicit(out, x.astype(np.float64), A, B, blk_off, blk_m, ra)
    assert np.allclose(got, ref, rtol=1e-12, atol=1e-12)


def test_a_zero_B_gives_out_back_exactly():
    out, x, A, B = _case(2)
    got, scale = qp.reference_lora(out, x, IN_F16, None, A, np.zeros_like(B), [0, 32], [32, 16], [0, 1, 0, 1], return_scale=True)
    assert np.array_equal(got, out.astype(np.float64)) and not scale.any()


@pytest.mark.parametrize("mode,rms", [(IN_F16, None), (IN_F32, None), (IN_F32, "weight"), (IN_F32, "plain"), (IN_SWIGLU_F32, None)],
                         ids=["f16", "f32", "f32-rms-weight", "f32-rms", "swiglu"])
def test_each_input_mode_against_its_formula(mode, rms):
    out, x, A, B = _case(3, mode=mode)
    k, eps = 64, 1e-5
    w = np.random.default_rng(9).standard_normal(k).astype(F16)
    x64 = x.astype(np.float64)
    if mode == IN_SWIGLU_F32:
        up, gate = x64[:, :k], x64[:, k:]
        xin = gate * (1.0 / (1.0 + np.exp(-gate))) * up
    elif rms:
        xin = x64 / np.sqrt(np.mean(x64 ** 2, axis=1, keepdims=True) + float(np.float32(eps)))
        if rms == "weight":
            xin = xin * w.astype(np.float64)
    else:
        xin = x64
    arg = None if rms is None else (eps, w if rms == "weight" else None)
    ra = [1, 0, -1, 1]
    got, scale = qp.reference_lora(out, x, mode, arg, A, B, [0, 48], [32, 16], ra, return_scale=True)
    ref = _explicit(out, xin, A, B, [0, 48], [32, 16], ra)
    assert np.allclose(got, ref, rtol=1e-12, atol=1e-12)
    # the scale of the bound: sum_r |B_jr| sum_l |A_rl xin_l|
    a, j, R = 1, 5, 8
    want = sum(abs(float(B[a, 32 + j, r])) * np.abs(A[a, R + r].astype(np.float64) * xin[0]).sum() for r in range(R))
    assert np.isclose(scale[0, 48 + j], want, rtol=1e-12) and not scale[2].any() and not scale[:, 32:48].any()


def test_reference_rejects_what_the_contract_does_not_define():
    out, x, A, B = _case(4)
    with pytest.raises(ValueError):
        qp.reference_lora(out, x, IN_F16, (1e-5, None), A, B, [0, 32], [32, 16], [0] * 4)  # a norm on fp16 rows
    with pytest.raises(ValueError):
        qp.reference_lora(out, x, IN_F32, None, A, B, [0, 32], [32, 16], [0] * 4)          # fp16 rows as IN_F32
    with pytest.raises(ValueError):
        qp.reference_lora(out, x, IN_F16, None, A, B, [0, 32], [32, 32], [0] * 4)          # blocks that B does not have


# ------------------------------------------------------------------------------------------------------------ LoraBank on CPU

H, KV, INTER, HD = 256, 64, 512, 64


def _layers(n, **merge):
    cfg = types.SimpleNamespace(hidden_size=H, intermediate_size=INTER, hidden_act="silu", num_attention_heads=H // HD,
                                num_key_value_heads=KV // HD, head_dim=HD, attention_dropout=0.0)
    return [types.SimpleNamespace(self_attn=qp.IncoherentSdpaAttention(cfg, **merge), mlp=qp.IncoherentMLP(H, INTER, "silu"))
            for _ in range(n)]


SHAPES = {"self_attn.q_proj": (H, H), "self_attn.k_proj": (H, KV), "self_attn.v_proj": (H, KV), "self_attn.o_proj": (H, H),
          "mlp.up_proj": (H, INTER), "mlp.gate_proj": (H, INTER), "mlp.down_proj": (INTER, H)}


def _adapter(seed, r, layers=(0, 1), linears=tuple(SHAPES)):
    g = torch.Generator().manual_seed(seed)
    return {f"{i}_{lin}": (torch.randn(r, SHAPES[lin][0], generator=g) * 0.1, torch.randn(SHAPES[lin][1], r, generator=g) * 0.1)
            for i in layers for lin in linears}


def test_bank_packing_rank_padding_scale_and_missing_linears():
    bank = qp.LoraBank(_layers(2), n_adapters=3, rank=16, B_slots=4, device="cpu")
    assert bank.slot_adapter.tolist() == [-1] * 4 and bank.slot_adapter.dtype == torch.int32
    w = _adapter(5, r=8, linears=("self_attn.q_proj", "self_attn.v_proj", "mlp.gate_proj", "mlp.down_proj"))
    del w["1_mlp.down_proj"]
    alpha = 24.0
    bank.load(1, w, alpha)
    R = 16
    for i in range(2):
        g = bank.group(i, "qkv")
        assert tuple(g.A.shape) == (3, 3 * R, H) and tuple(g.B.shape) == (3, H + 2 * KV, R)
        assert g.blk_off == [0, H, H + KV] and g.blk_m == [H, KV, KV] and g.k == H
        A, B = w[f"{i}_self_attn.q_proj"]
        assert torch.equal(g.A[1, :8], A.half()) and not g.A[1, 8:R].any()            # rank 8 of 16: zero rows behind it
        assert torch.equal(g.B[1, :H, :8], (B.float() * torch.tensor(alpha / 8)).half()) and not g.B[1, :H, 8:].any()
        assert not g.A[1, R:2 * R].any() and not g.B[1, H:H + KV].any()               # k_proj is not in the adapter
        A, B = w[f"{i}_self_attn.v_proj"]
        assert torch.equal(g.A[1, 2 * R:2 * R + 8], A.half()) and torch.equal(g.B[1, H + KV:, :8], (B.float() * torch.tensor(3.0)).half())
        assert not g.A[0].any() and not g.A[2].any() and not g.B[0].any() and not g.B[2].any()
        g = bank.group(i, "ug")
        assert g.blk_off == [0, INTER] and g.blk_m == [INTER, INTER]
        assert not g.A[1, :R].any() and not g.B[1, :INTER].any()                      # up_proj missing, gate_proj there
        assert torch.equal(g.A[1, R:R + 8], w[f"{i}_mlp.gate_proj"][0].half())
        assert not bank.group(i, "o").A.any() and not bank.group(i, "o").B.any()
    assert bank.group(0, "down").k == INTER and bank.group(0, "down").A[1, :8].any()
    assert not bank.group(1, "down").A.any()                                          # the key removed above
    want = 4 * 4 + sum(2 * 3 * (len(m) * R * k + sum(m) * R) for k, m in ((H, [H, KV, KV]), (H, [H]), (H, [INTER] * 2), (INTER, [H]))) * 2
    assert bank.bytes() == want
    bank.unload(1)
    assert not any(grp.A.any() or grp.B.any() for g in bank.groups for grp in g.values())


def test_bank_merged_and_unmerged_qkv_land_in_the_same_columns():
    w = _adapter(6, r=16)
    packed = {}
    for name, merge in (("plain", {}), ("qkv", dict(merge_qkv=True)), ("kv", dict(merge_kv=True)), ("qv", dict(merge_qv=True))):
        bank = qp.LoraBank(_layers(2, **merge), n_adapters=1, rank=16, B_slots=1, device="cpu")
        bank.load(0, w, 16.0)
        packed[name] = bank.group(1, "qkv")
    # q|k|v buffers hold q, k, v in this order except with q and v merged (q|v|k): the blocks follow, A and B do not change
    for name in ("qkv", "kv"):
        assert packed[name].blk_off == packed["plain"].blk_off == [0, H, H + KV]
    assert packed["qv"].blk_off == [0, H + KV, H] and packed["qv"].blk_m == [H, KV, KV]
    for name in ("qkv", "kv", "qv"):
        assert torch.equal(packed[name].A, packed["plain"].A) and torch.equal(packed[name].B, packed["plain"].B)
    # through the contract: the update of k lands where the layout keeps k
    x = np.random.default_rng(0).standard_normal((1, H)).astype(np.float32)
    out = np.zeros((1, H + 2 * KV), np.float32)
    res = {n: qp.reference_lora(out, x, IN_F32, None, g.A.numpy(), g.B.numpy(), g.blk_off, g.blk_m, [0]) for n, g in packed.items()}
    assert np.array_equal(res["plain"], res["qkv"])
    assert np.array_equal(res["plain"][:, H:H + KV], res["qv"][:, H + KV:]) and np.array_equal(res["plain"][:, H + KV:], res["qv"][:, H:H + KV])
    A, B = (t.half().double().numpy() for t in w["1_self_attn.k_proj"])
    assert np.allclose(res["plain"][0, H:H + KV], (B * 1.0).astype(F16).astype(np.float64) @ (A @ x[0].astype(np.float64)), rtol=1e-12)


def test_bank_argument_errors():
    layers = _layers(1)
    for kw in (dict(n_adapters=0, rank=16, B_slots=1), dict(n_adapters=1, rank=12, B_slots=1), dict(n_adapters=1, rank=72, B_slots=1),
               dict(n_adapters=1, rank=8, B_slots=0)):
        with pytest.raises(qp._native.QpalError):
            qp.LoraBank(layers, device="cpu", **kw)
    bank = qp.LoraBank(layers, n_adapters=2, rank=8, B_slots=2, device="cpu")
    with pytest.raises(qp._native.QpalError, match="adapter_id"):
        bank.load(2, {}, 1.0)
    with pytest.raises(qp._native.QpalError, match="1_self_attn.q_proj"):
        bank.load(0, _adapter(1, 8, layers=(1,)), 1.0)           # the bank has one layer
    with pytest.raises(qp._native.QpalError, match="0_self_attn.q_proj"):
        bank.load(0, _adapter(1, 16, layers=(0,)), 1.0)          # rank 16 into a bank of rank 8
    assert not bank.group(0, "qkv").A.any()                      # a load that fails writes nothing
    with pytest.raises(qp._native.QpalError, match="slot"):
        bank.set(2, 0)
    with pytest.raises(qp._native.QpalError, match="adapter_id"):
        bank.set(0, 2)
    bank.set(1, 1)
    bank.set(0, 0)
    bank.set(0, -1)
    assert bank.slot_adapter.tolist() == [-1, 1]
    with pytest.raises(qp._native.QpalError, match="device tensors"):
        g = bank.group(0, "o")
        qp.lora_apply(torch.zeros(1, H), torch.zeros(1, H, dtype=torch.float16), IN_F16, None, g.A, g.B, g.blk_off, g.blk_m, bank.slot_adapter[:1])


# ------------------------------------------------------------------------------------------------------------ PEFT directories

def _write_peft(path, weights, r=8, alpha=16, targets=("q_proj", "v_proj", "down_proj"), prefix="base_model.model.model.", **cfg):
    from safetensors.torch import save_file
    tensors = {}
    for key, (A, B) in weights.items():
        layer, lin = key.split("_", 1)
        tensors[f"{prefix}layers.{layer}.{lin}.lora_A.weight"] = A.contiguous()
        tensors[f"{prefix}layers.{layer}.{lin}.lora_B.weight"] = B.contiguous()
    save_file(tensors, str(path / "adapter_model.safetensors"))
    config = dict(peft_type="LORA", r=r, lora_alpha=alpha, target_modules=list(targets), bias="none", use_dora=False,
                  modules_to_save=None, rank_pattern={}, alpha_pattern={}, use_rslora=False)
    config.update(cfg)
    (path / "adapter_config.json").write_text(json.dumps(config))
    return tensors


def test_peft_round_trip(tmp_path):
    w = _adapter(7, r=8, linears=("self_attn.q_proj", "self_attn.v_proj", "mlp.down_proj"))
    _write_peft(tmp_path, w)
    got, alpha = qp.load_peft_adapter(str(tmp_path))
    assert alpha == 16.0 and set(got) == set(w) and len(got) == 6
    for key in w:
        assert torch.equal(got[key][0], w[key][0]) and torch.equal(got[key][1], w[key][1])
    bank = qp.LoraBank(_layers(2), n_adapters=1, rank=8, B_slots=1, device="cpu")
    bank.load(0, got, alpha)
    assert torch.equal(bank.group(1, "down").B[0], (w["1_mlp.down_proj"][1] * torch.tensor(2.0)).half())


@pytest.mark.parametrize("cfg,named", [(dict(use_dora=True), "use_dora"), (dict(modules_to_save=["lm_head"]), "modules_to_save"),
                                       (dict(rank_pattern={"q_proj": 4}), "rank_pattern"), (dict(alpha_pattern={"q_proj": 4}), "alpha_pattern"),
                                       (dict(bias="all"), "bias"), (dict(use_rslora=True), "use_rslora"),
                                       (dict(target_modules=["q_proj", "lm_head"]), "target_modules"),
                                       (dict(target_modules="all-linear"), "target_modules")])
def test_peft_rejections_name_the_key(tmp_path, cfg, named):
    _write_peft(tmp_path, _adapter(8, r=8, layers=(0,), linears=("self_attn.q_proj",)), **cfg)
    with pytest.raises(qp._native.QpalError, match=named):
        qp.load_peft_adapter(str(tmp_path))


def test_peft_rejects_tensors_it_cannot_apply(tmp_path):
    from safetensors.torch import save_file
    w = _adapter(9, r=8, layers=(0,), linears=("self_attn.q_proj",))
    tensors = _write_peft(tmp_path, w)
    for extra in ("base_model.model.model.layers.0.self_attn.q_proj.lora_B.bias", "base_model.model.lm_head.lora_A.weight",
                  "base_model.model.model.embed_tokens.lora_embedding_A"):
        save_file({**tensors, extra: torch.zeros(8, 8)}, str(tmp_path / "adapter_model.safetensors"))
        with pytest.raises(qp._native.QpalError, match=re.escape(extra)):
            qp.load_peft_adapter(str(tmp_path))
    half = {k: v for k, v in tensors.items() if "lora_A" in k}
    save_file(half, str(tmp_path / "adapter_model.safetensors"))
    with pytest.raises(qp._native.QpalError, match="lora_A only"):
        qp.load_peft_adapter(str(tmp_path))
    _write_peft(tmp_path, w, r=4)  # the config's rank is not the tensors'
    with pytest.raises(qp._native.QpalError, match="r = 4"):
        qp.load_peft_adapter(str(tmp_path))
