"""CPU-only checks: the C-ABI library loads and exports every symbol include/qpal.h declares (no compute
calls without a GPU), and the host-side mirror of the reference interface behaves (op-name grammar, fake
tensors, quantizer strings, synthetic layer shapes, layer fusion, sharding)."""
import os
import re

import numpy as np
import pytest
import torch

import qpalette_amd as qp
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "qpal.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(qpal_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    syms = _header_symbols()
    assert {"qpal_tcq_gemv", "qpal_tcq_gemv_multi", "qpal_tcq_dequant", "qpal_lut_tc_gemv", "qpal_lut_tc_gemv_multi",
            "qpal_lut_tc_dequant", "qpal_lut_simt_gemv", "qpal_lut_simt_dequant", "qpal_tc_to_simt",
            "qpal_error_string", "qpal_version"} <= set(syms)
    lib = qp._native.lib()
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/qpal.h but not exported"
    assert set(qp._native.exported_symbols()) == set(syms)
    assert lib.qpal_version() >= 100
    assert lib.qpal_error_string(-1).decode().startswith("unsupported shape")


def test_argument_errors_are_return_codes_not_exits():
    lib = qp._native.lib()
    # null pointers / bad shapes are rejected before anything touches a device
    assert lib.qpal_tcq_gemv(None, None, None, None, None, 4096, 1, 4096, 9, 6, 0, 0, None) == -3
    assert lib.qpal_lut_tc_dequant(None, None, None, 64, 64, 4, 1, None) == -3
    buf = np.zeros(1 << 16, dtype=np.uint8)
    p = buf.ctypes.data
    assert lib.qpal_tcq_gemv(p, p, None, p, p, 4100, 1, 4096, 9, 6, 0, 0, None) == -1   # m % 32
    assert lib.qpal_tcq_gemv(p, p, None, p, p, 4096, 129, 4096, 9, 6, 0, 0, None) == -1  # n > 128
    assert lib.qpal_tcq_gemv(p, p, None, p, p, 4096, 1, 4096, 9, 11, 0, 0, None) == -2  # KV outside the table
    assert lib.qpal_tcq_gemv(p, p, p, p, p, 4096, 1, 4096, 9, 6, 8, 2, None) == -2      # KV2 != KV1 + 1
    assert lib.qpal_lut_tc_gemv(p, p, p, p, 4096, 1, 4096, 9, 1, None) == -2            # sq has bits <= 8
    assert lib.qpal_lut_simt_gemv(p, p, p, p, 64, 1, 4096, 5, 4, None) == -2            # vec 4 needs bits >= 6


def test_op_name_grammar():
    good = ["decompress_gemm_tcq_4096_1_4096_9_6", "decompress_gemm_tcq_1024_7_4096_9_10", "decompress_gemm_tcq_1024_16_4096_9_6",
            "decompress_gemm_tcq_1024_64_4096_9_6", "decompress_gemm_tcq_1024_128_4096_9_6",
            "decompress_gemm_tcq_combt_14336_1_4096_9_6_7", "decompress_gemm_tcq_comb_4096_8_4096_10_9_10",
            "decompress_tcq_9_2", "decompress_tcq_combt_11_9_10", "decompress_gemm_4096_2_4096_4_sq_dup",
            "decompress_gemm_4096_1_4096_8_sq", "decompress_gemm_28672_1_4096_12_vq2", "decompress_gemv_4096_4096_4_sq",
            "decompress_6_sq", "vq_pack_gemm_simt_4_2_8", "vq_pack_dequant_simt_4_12", "sq_pack_gemm_simt"]
    bad = ["decompress_gemm_tcq_4096_1_4096_9_11", "decompress_gemm_tcq_4096_1_4096_10_7", "decompress_tcq_12_9",
           "decompress_gemm_tcq_4100_1_4096_9_6", "decompress_gemm_tcq_4096_129_4096_9_6",
           "decompress_gemm_tcq_combt_4096_1_4096_9_6_8", "decompress_gemm_4096_1_4096_5_sq_dup",
           "decompress_gemm_4096_1_4096_13_vq2", "vq_pack_gemm_simt_1_4_5", "vq_pack_gemm_simt_1_3_8", "nonsense"]
    for name in good:
        assert qp.ops.ensure_op(name), name
        assert getattr(torch.ops.ours_lib, name) is not None
    for name in bad:
        assert not qp.ops.ensure_op(name), name
        with pytest.raises(AttributeError):
            getattr(torch.ops.ours_lib, name)


def test_fake_tensor_shapes_and_dtypes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        c = torch.empty(4096 * 4096 * 6 // 32, dtype=torch.int16, device="cuda")
        x = torch.empty(3, 4096, dtype=torch.float16, device="cuda")
        cb = torch.empty(512, 2, dtype=torch.float16, device="cuda")
        y = qp.ops.get_op("decompress_gemm_tcq_4096_3_4096_9_6")(c, x, cb)
        assert tuple(y.shape) == (3, 4096) and y.dtype == torch.float32
        w = qp.ops.get_op("decompress_tcq_9_6")(c, cb, 4096, 4096)
        assert tuple(w.shape) == (4096, 4096) and w.dtype == torch.float16
        q = torch.empty(4096, 512, dtype=torch.int32, device="cuda")
        lut = torch.empty(16, dtype=torch.float16, device="cuda")
        y = qp.ops.get_op("sq_pack_gemm_simt")(x.reshape(3, 1, 4096), q, lut, 4)
        assert tuple(y.shape) == (3, 1, 4096) and y.dtype == torch.float16


def test_no_cpu_implementation():
    """The product path is the HIP library only: CPU tensors are refused, not silently computed."""
    op = qp.ops.get_op("decompress_gemm_tcq_64_1_64_9_4")
    with pytest.raises((RuntimeError, NotImplementedError)):
        op(torch.zeros(32, 16, dtype=torch.int16), torch.zeros(1, 64), torch.zeros(512, 2, dtype=torch.float16))


def test_quantizer_strings_and_layer_shapes():
    mo = qp.mem_op
    assert mo.get_quant_info("tcq_6_none_0.9")["tlut_bits"] == 9 and mo.get_quant_info("tcq_9_none_0.9")["tlut_bits"] == 10
    assert mo.get_quant_info("tcomb_9_10_0.5_none_0.9")["tlut_bits"] == 11
    assert mo.bits_per_weight("tcomb_6_7_0.5_none_0.9") == 3.25 and mo.bits_per_weight("ldlq_2_12_none_1.0") == 6.0
    weights = sum(v["in_features"] * v["out_features"] for k, v in mo.get_layer_info("3_8b").items() if k != "nlayers")
    assert weights == 218103808
    info = mo.get_dummy_quant_results("3_8b", "mlp.down_proj", "tcomb_6_7_0.5_none_0.9")["linear_info"]
    assert tuple(info["trellis1"].shape) == (4096 // 16 * 7168 // 16, 48) and info["trellis1"].dtype == torch.int16
    assert tuple(info["trellis2"].shape) == (4096 // 16 * 7168 // 16, 56) and tuple(info["tlut"].shape) == (512, 2)
    info = mo.get_dummy_quant_results("3_8b", "self_attn.k_proj", "ldlq_2_9_none_1.0")["linear_info"]
    assert tuple(info["qweight"].shape) == (1024, 9 * 4096 // 64) and tuple(info["lut"].shape) == (512, 2)
    assert qp.linear.linear_class_for("tcomb_6_7_0.5_none_0.9") is qp.CombtLinearTCQ
    assert qp.linear.linear_class_for("comb_6_7_0.5_none_0.9") is qp.CombLinearTCQ
    assert qp.linear.linear_class_for("tcq_6_none_0.9") is qp.QTIPLinearTCQ
    assert qp.linear.linear_class_for("ldlq_1_4_none_1.0", use_simt=True) is qp.VQLinearPackSIMT


def test_modules_round_trip_info_and_merge():
    for qstr, cls in (("tcq_5_none_0.9", qp.QTIPLinearTCQ), ("tcomb_6_7_0.5_none_0.9", qp.CombtLinearTCQ),
                      ("comb_3_4_0.5_none_0.9", qp.CombLinearTCQ), ("ldlq_2_8_none_1.0", qp.VQLinearPackTensorCore)):
        a = qp.mem_op.dummy_linear_info(256, 128, qstr, seed=1)
        layer = cls.gen_layer_from_info(a) if cls is not qp.VQLinearPackTensorCore else cls.gen_layer_from_info(a)
        back = layer._info()
        for key, val in a.items():
            if isinstance(val, torch.Tensor):
                assert torch.equal(back[key], val), key
        if hasattr(cls, "merge_infos") and cls is not qp.CombLinearTCQ:
            b = qp.mem_op.dummy_linear_info(256, 64, qstr, seed=2)
            tab = "lut" if "lut" in a else "tlut"
            b[tab] = a[tab].clone()
            m = cls.merge_infos(a, b)
            assert m["out_features"] == 192
            fused = cls.gen_layer_from_info(m)
            assert fused.out_features == 192


def test_merged_rows_decode_as_concatenation():
    """merge_infos == row concatenation of W (what QKV / up+gate fusion relies on), checked with the oracle."""
    qstr = "tcomb_6_7_0.5_none_0.9"
    a = qp.mem_op.dummy_linear_info(256, 128, qstr, seed=1)
    b = qp.mem_op.dummy_linear_info(256, 64, qstr, seed=2)
    b["tlut"] = a["tlut"].clone()
    m = qp.CombtLinearTCQ.merge_infos(a, b)

    def W(i):
        return oracle.tcq_dequant(i["trellis1"].numpy(), i["tlut"].numpy(), i["out_features"], 256, 9, 6,
                                  c2=i["trellis2"].numpy(), KV2=7, split=2)

    assert np.array_equal(W(m).view(np.uint16), np.concatenate([W(a), W(b)], 0).view(np.uint16))


def test_row_shards_decode_as_row_slices():
    for qstr in ("tcq_6_none_0.9", "tcomb_6_7_0.5_none_0.9", "ldlq_1_4_none_1.0", "ldlq_2_9_none_1.0"):
        k, m = 256, 32 * 7  # 7 supertile rows over 3 ranks -> ragged shards
        info = qp.mem_op.dummy_linear_info(k, m, qstr, seed=3)

        def W(i):
            mm = i["out_features"]
            if "trellis1" in i:
                return oracle.tcq_dequant(i["trellis1"].numpy(), i["tlut"].numpy(), mm, k, 9, 6, c2=i["trellis2"].numpy(),
                                          KV2=7, split=2)
            if "trellis" in i:
                return oracle.tcq_dequant(i["trellis"].numpy(), i["tlut"].numpy(), mm, k, 9, 6)
            return oracle.lut_tc_dequant(i["qweight"].numpy(), i["lut"].numpy(), mm, k, i["lut_bits"], i["vec_sz"])

        full = W(info)
        sizes = qp.shard.shard_rows(m, 3)
        assert sizes == [96, 64, 64] and sum(sizes) == m
        for rank in range(3):
            r0, r1 = qp.shard.shard_bounds(m, 3, rank)
            part = W(qp.shard.shard_linear_info(info, rank, 3))
            assert np.array_equal(part.view(np.uint16), full[r0:r1].view(np.uint16))


def test_module_constructors_register_their_ops_without_the_lazy_hook():
    """Boundary hardening: with the private-API lazy lookup switched off (QPAL_LAZY_OPS=0) every operator a module's forward
    asks for already exists after construction, the reference's calling pattern (getattr(torch.ops.ours_lib, f"...") inside
    forward, lib/linear/tcq_linear.py:64-85) traces through register_fake, and names nobody registered are refused."""
    import subprocess
    import sys
    code = r'''
import os, sys
os.environ["QPAL_LAZY_OPS"] = "0"
sys.path.insert(0, %r)
import torch
import qpalette_amd as qp
assert qp.ops.LAZY_LOOKUP is False
k, m = 256, 128
for qstr in ("tcq_6_none_0.9", "tcomb_6_7_0.5_none_0.9", "comb_6_7_0.5_none_0.9", "ldlq_2_8_none_1.0", "ldlq_1_4_none_1.0"):
    layer = qp.make_linear_from_info(qstr, qp.mem_op.dummy_linear_info(k, m, qstr, seed=1))
    for name in layer.op_names():
        getattr(torch.ops.ours_lib, name)          # plain torch lookup, no hook
try:
    getattr(torch.ops.ours_lib, "decompress_gemm_tcq_64_1_64_9_4")
    raise SystemExit("an unregistered name resolved without the lazy hook")
except AttributeError:
    pass

class RefStyle(torch.nn.Module):                    # the reference's forward, verbatim pattern
    def __init__(self, layer):
        super().__init__()
        self.l = layer
    def forward(self, inp):
        l = self.l
        x = inp.view(-1, l.in_features)
        bs = x.shape[0]
        y = getattr(torch.ops.ours_lib, f"decompress_gemm_tcq_{l.out_features}_{bs}_{l.in_features}_{l.tlut_bits}_{l.KV}")(
            l.trellis, x.to(torch.float16), l.tlut)
        return y.view(*inp.shape[:-1], l.out_features).to(inp.dtype)

from torch._subclasses.fake_tensor import FakeTensorMode
from torch.fx.experimental.proxy_tensor import make_fx
layer = qp.make_linear_from_info("tcq_6_none_0.9", qp.mem_op.dummy_linear_info(k, m, "tcq_6_none_0.9", seed=1))
with FakeTensorMode(allow_non_fake_inputs=True) as mode:
    fl = RefStyle(layer).to("meta")
    x = torch.empty(3, k, dtype=torch.float16, device="cuda")
    tre = torch.empty_like(layer.trellis, device="cuda"); tl = torch.empty(512, 2, dtype=torch.float16, device="cuda")
    def f(tre, x, tl):
        return getattr(torch.ops.ours_lib, f"decompress_gemm_tcq_{m}_3_{k}_9_6")(tre, x, tl)
    gm = make_fx(f)(tre, x, tl)
names = [n.target.__name__ if hasattr(n.target, "__name__") else str(n.target) for n in gm.graph.nodes if n.op == "call_function"]
assert any("decompress_gemm_tcq_128_3_256_9_6" in str(t) for t in names), names
print("ok")
''' % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_mi355x_latency_table_is_loadable_by_the_reference_solver():
    """perf/latency/3_8b_latency_coeffs_mi355x.pt has the reference's format (solve_lat_const.py:113-123,
    219-221: {f"{layer}_{quantizer_str}_{simt}": seconds} + a 0-d tensor 'constant') and its exact key set, so that the
    fusion-aware solver can target MI355X; the solver's latency expression evaluates on the published figure1d result."""
    import json
    lat = torch.load(os.path.join(ROOT, "perf", "latency", "3_8b_latency_coeffs_mi355x.pt"), weights_only=True)
    layers = ["q", "k", "v", "o", "u", "g", "d", "qk", "kv", "qv", "qkv", "ug"]
    quants = ([f"tcq_{kv}_none_0.9" for kv in range(3, 11)] + [f"tcomb_{kv}_{kv + 1}_0.5_none_0.9" for kv in range(3, 10)] +
              [f"ldlq_2_{b}_none_1.0" for b in range(3, 13)] + [f"ldlq_1_{b}_none_1.0" for b in range(2, 9)])
    want = {f"{l}_{q}_False" for l in layers for q in quants} | {f"{l}_{q}_True" for l in layers for q in quants if q.startswith("ldlq")}
    assert set(lat) == want | {"constant"} and len(lat) == 589  # the reference's assets/3_8b_latency_coeffs_4090_cc.pt: 589 keys
    assert all(isinstance(lat[k], float) and 1e-6 < lat[k] < 1e-3 for k in want)
    const = float(lat["constant"].item())                        # exactly how the solver reads it (l.114)
    assert 0.0 < const < 0.05
    with open(os.path.join(ROOT, "perf", "qdicts", "figure1d.json")) as f:
        data = json.load(f)
    short = {"self_attn.q_proj": "q", "self_attn.k_proj": "k", "self_attn.v_proj": "v", "self_attn.o_proj": "o",
             "mlp.up_proj": "u", "mlp.gate_proj": "g", "mlp.down_proj": "d"}
    total = const
    for i, merges in enumerate(data["merge_info"]):
        groups = [[k] for k in short]
        for mg in merges:
            members = [k for k in short if short[k] in mg.split("_")[1]]
            groups = [g for g in groups if g[0] not in members] + [members]
        for g in groups:
            q, simt = data["qdict"][f"{i}_{g[0]}"]
            key = "".join(short[k] for k in g)
            key = {"gu": "ug", "ug": "ug"}.get(key, key)
            total += lat[f"{key}_{q}_{'True' if simt == '1' else 'False'}"]
    assert const < total < const + 0.01  # a decoded token of the published fusion-aware model, by the solver's formula


@pytest.mark.parametrize("cls,part", [("CombLinearTCQ", (128, 128)), ("CombtLinearTCQ", (64, 192))])
def test_batches_above_the_fused_batch_do_not_recurse_on_layers_without_a_multi_job_form(cls, part, monkeypatch):
    """Row-split (comb_*) layers and column-split ones with unequal parts run no multi-job launch; for 128 < bs <= 256 their forward
    goes through multi_gemv's chunked branch, which must run passes of the layer's OWN fused launch (it used to call the
    forward again: RecursionError).  Host dispatch only: _gemv is replaced by a recorder, no kernel runs."""
    layer = getattr(qp, cls)(256, 256, 16, 16, part, 16, (3, 4), 2, 9)
    assert qp.linear._codec_key(layer)[0] == "single" and layer.max_chunked_batch == 256
    calls = []

    def fake_gemv(self, x, bs):
        calls.append(bs)
        assert x.shape[0] == bs <= self.max_fused_batch
        return torch.full((bs, self.out_features), float(len(calls)))

    monkeypatch.setattr(type(layer), "_gemv", fake_gemv)
    for bs, want in ((129, [128, 1]), (200, [128, 72]), (256, [128, 128])):
        calls.clear()
        y = layer(torch.zeros(bs, 256).half())
        assert calls == want and tuple(y.shape) == (bs, 256) and y.dtype == torch.float16
        assert float(y[0, 0]) == 1.0 and float(y[-1, 0]) == 2.0  # rows of pass 1, then rows of pass 2


def test_early_load_registers_are_untouched_until_their_wait():
    """the fused GEMV kernels issue their early-staging loads from inline asm, outside the compiler's wait-count
    bookkeeping, and wait for them by hand — so nothing but the register allocator's choices kept a destination register from being
    copied, reused or spilled in between.  perf/check_early_loads.py disassembles every fused-GEMV code object of THIS build and
    walks the control-flow graph from every such load: this test fails the build that breaks the rule."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_check_early", os.path.join(ROOT, "perf", "check_early_loads.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    build = os.path.join(ROOT, "q-palette_amd", "csrc", "build")
    if not os.path.isdir(build) or not os.path.exists(os.path.join(chk.LLVM, "llvm-objdump")):
        pytest.skip("no object files of this build / no llvm-objdump (the library was built elsewhere)")
    r = chk.run(build)
    assert r["kernels"] >= 150 and r["early_loads"] >= 800, r
    assert r["violations"] == [], "\n".join(r["violations"][:10])
    # kernels that spill AND stage early are covered by the same walk (their scratch stores are instructions like any other);
    # the count is pinned so that a new spilling instantiation is noticed
    assert len(r["early_with_scratch"]) <= 32, r["early_with_scratch"]
    # the checker itself: a copy, a reuse and a spill in front of the wait are caught, a wait that covers the load clears it
    ld = ("global_load_dword", "v10, v2, s[4:5]", 0, None)
    fetch = ("s_load_dwordx8", "s[24:31], s[12:13], s9 offset:0x78", 8, None)
    wait0 = ("s_waitcnt", "vmcnt(0)", 12, None)
    use = ("v_xor_b32_e32", "v11, 0x8000, v10", 16, None)
    end = ("s_endpgm", "", 20, None)
    assert chk.check_kernel("k", [ld, fetch, wait0, use, end]) == (1, [])
    for culprit in (("v_mov_b32_e32", "v12, v10", 4, None), ("v_mov_b32_e32", "v10, v3", 4, None),
                    ("scratch_store_dword", "off, v10, off offset:4", 4, None)):
        n, bad = chk.check_kernel("k", [ld, culprit, fetch, wait0, use, end])
        assert n == 1 and len(bad) == 1 and culprit[0] in bad[0]
    # a counted wait covers the load only once enough younger operations are behind it
    ld2 = ("global_load_dword", "v20, v2, s[4:5]", 2, None)
    wait1 = ("s_waitcnt", "vmcnt(1)", 12, None)
    assert chk.check_kernel("k", [ld, ld2, fetch, wait1, use, end]) == (2, [])            # v10 is the older of two: vmcnt(1) covers it
    n, bad = chk.check_kernel("k", [ld2, ld, fetch, wait1, use, end])
    assert n == 2 and len(bad) == 1                                                      # v10 is the younger: vmcnt(1) does not
    # and a path AROUND the wait is found
    br = ("s_cbranch_scc1", "3", 10, 16)
    n, bad = chk.check_kernel("k", [ld, fetch, br, wait0, use, end])
    assert n == 1 and len(bad) == 1


def _plan(rows, st1, st2, flags, waves=16, shared=1):
    import ctypes
    n = len(rows)
    arr = lambda v: (ctypes.c_int * n)(*v)
    out = (ctypes.c_int * 1024)()
    rc = qp._native.lib().qpal_plan_gemv(arr(rows), arr(st1), arr(st2), arr(flags), n, waves, shared, out, 1024)
    assert rc == 0, rc
    o = list(out)
    M, W = o[6], o[7]
    d = {"grid": o[0], "items": o[1], "ncls": o[2], "items0": o[3], "span": o[4], "mask": o[5], "cls": []}
    pos = 8
    for _ in range(2):
        lg, rg = o[pos], o[pos + 1]
        ents = [[(o[pos + 2 + 2 * (m * W + w)] & 0xffffffff, o[pos + 3 + 2 * (m * W + w)] & 0xffffffff) for w in range(W)] for m in range(M)]
        d["cls"].append({"lg": lg, "rg": rg, "w": ents})
        pos += 2 + 2 * M * W
    d["jobs"] = [dict(cls=o[pos + 4 * j], vrow0=o[pos + 4 * j + 1], end=o[pos + 4 * j + 2], sk=o[pos + 4 * j + 3]) for j in range(n)]
    return d


def _check_plan(d, rows, st1, st2, waves):
    """every step of every live row of every job exactly once; runs of a row are consecutive waves with one lead; <= 2 workgroups
    per row; -> steps of the busiest SIMD"""
    busiest = 0
    for c in range(d["ncls"]):
        pl = d["cls"][c]
        G, rg = 1 << pl["lg"], pl["rg"]
        jobs = [j for j in range(len(rows)) if d["jobs"][j]["cls"] == c]
        s1, s2 = st1[jobs[0]], st2[jobs[0]]
        cover = {}
        owners = {}
        for m in range(G):
            simd = [0, 0, 0, 0]
            w = 0
            while w < waves:
                a, b = pl["w"][m][w]
                if not (a >> 16) & 1:
                    w += 1
                    continue
                assert (a >> 9) & 1, "a run starts with its lead"
                run = (a >> 11) & 31
                assert run >= 1
                for q in range(run):
                    a2, b2 = pl["w"][m][w + q]
                    assert (a2 >> 16) & 1 and (a2 & 255) == (a & 255) and ((a2 >> 9) & 1) == (q == 0)
                    row, stream, s0, ns = a2 & 255, (a2 >> 8) & 1, b2 & 0xffff, b2 >> 16
                    assert ns >= 1 and s0 + ns <= (s2 if stream else s1)
                    for s_ in range(s0, s0 + ns):
                        key = (row, stream, s_)
                        assert key not in cover
                        cover[key] = m
                    owners.setdefault(row, set()).add(m)
                    simd[(w + q) % 4] += ns
                    assert ((a2 >> 10) & 1) == ((a >> 10) & 1)
                w += run
            busiest = max(busiest, max(simd))
        assert len(cover) == rg * (s1 + s2), (len(cover), rg, s1, s2)
        for row, ms in owners.items():
            assert len(ms) <= 2
            shared = any((a >> 10) & 1 for m in range(G) for a, b in pl["w"][m] if (a >> 16) & 1 and (a & 255) == row)
            assert shared == (len(ms) == 2)
        # the jobs' virtual rows tile the class's row space
        pos = 0
        for j in jobs:
            assert d["jobs"][j]["vrow0"] == pos and d["jobs"][j]["end"] >= pos + rows[j]
            if d["span"]:
                assert d["jobs"][j]["end"] == pos + rows[j]
            else:
                assert d["jobs"][j]["end"] % rg == 0
            pos = d["jobs"][j]["end"]
    assert d["items"] == sum((max(d["jobs"][j]["end"] for j in range(len(rows)) if d["jobs"][j]["cls"] == c) + d["cls"][c]["rg"] - 1)
                             // d["cls"][c]["rg"] << d["cls"][c]["lg"] for c in range(d["ncls"]))
    assert d["grid"] == min(d["items"], 256)
    return busiest


def test_gemv_launch_planner_random_sweep():
    """400 seeded random launches (1..4 jobs of 1..2000 supertile rows, 1..448 steps, one or two streams, at most two geometry
    classes, outputs zeroed or not, 16- and 8-wave workgroups) through the planner: every table covers every step of every row
    exactly once, never more than two workgroups per row, and one launch round never plans more items than it may."""
    import random
    rng = random.Random(20261005)
    for case in range(400):
        waves = 16 if rng.random() < 0.8 else 8
        geoms = []
        for _ in range(rng.choice((1, 1, 2))):
            a = rng.choice((1, 2, 3, 5, 8, 16, 32, 56, 64, 112, 224, 448, rng.randint(1, 448)))
            geoms.append((a, rng.choice((0, 0, a))))
        njobs = rng.randint(1, 4)
        rows = [rng.choice((1, 2, 7, 32, 128, 448, 896, rng.randint(1, 2000))) for _ in range(njobs)]
        pick = [rng.randrange(len(geoms)) for _ in range(njobs)]
        s1, s2 = [geoms[g][0] for g in pick], [geoms[g][1] for g in pick]
        flags = [rng.randint(0, 1) for _ in range(njobs)]
        d = _plan(rows, s1, s2, flags, waves=waves)
        try:
            _check_plan(d, rows, s1, s2, waves)
        except AssertionError as e:
            raise AssertionError(f"case {case}: rows {rows} steps {s1} + {s2} flags {flags} waves {waves}: {e}") from e
        for j in range(njobs):
            assert d["jobs"][j]["sk"] in (1, 2) and (flags[j] or d["jobs"][j]["sk"] in (1, 2))


def test_gemv_launch_planner_tables():
    """The host-side launch planner of the fused GEMV (csrc/qpal_capi.hip plan_launch, C-ABI qpal_plan_gemv): its per-wave tables
    cover every step of every row exactly once for the shapes the workloads launch, keep to two workgroups per row, and reach the
    balance the design claims — Llama-8B q|k|v (three jobs, 192 rows of 16 + 16 steps) on 256 workgroups with 6 steps on the
    busiest SIMD (whole rows: 8), gate|up on 256 with 28, o and down split in two."""
    Z = 1  # outputs declared zeroed
    # q | k | v of Llama-3.1-8B, tcomb: three jobs, groups stay inside their job.  (192 rows x 32 steps are exactly 24 steps for each
    # of 256 workgroups, but only as ONE row space of groups of 4 x 3 rows that run across the jobs' boundaries — built and measured
    # in round 5: 6 instead of 8 steps on the busiest SIMD, and the launch 0.13 us SLOWER: it is not bound by its steps.)
    rows, s1, s2 = [128, 32, 32], [16] * 3, [16] * 3
    d = _plan(rows, s1, s2, [Z] * 3)
    assert d["span"] == 0 and d["grid"] == 192 and _check_plan(d, rows, s1, s2, 16) == 8
    # ... one fused q|k|v job of 192 rows does get there: groups of 4 workgroups x 3 rows, 6 steps on the busiest SIMD
    d = _plan([192], [16], [16], [Z])
    assert d["grid"] == 256 and (1 << d["cls"][0]["lg"], d["cls"][0]["rg"]) == (4, 3) and _check_plan(d, [192], [16], [16], 16) == 6
    assert d["jobs"][0]["sk"] == 2
    # ... not zeroed: no shared rows without a large gain (a memset node costs more than two steps)
    d = _plan([192], [16], [16], [0])
    assert _check_plan(d, [192], [16], [16], 16) == 8 and d["jobs"][0]["sk"] == 1 and d["grid"] == 192
    # o_proj, gate | up, down_proj
    for rows, s1, s2, want_grid, want_busy in (([128], [16], [16], 256, 4), ([448, 448], [16, 16], [16, 16], 256, 28),
                                                ([128], [56], [56], 256, 14), ([128], [32], [0], 256, 4), ([448, 448], [32, 32], [0, 0], 256, 28)):
        d = _plan(rows, s1, s2, [Z] * len(rows))
        assert d["grid"] == want_grid, (rows, d["grid"])
        assert _check_plan(d, rows, s1, s2, 16) == want_busy, rows
    # Llama-3.1-70B shapes (k = 8192: 64 steps; down: k = 28672): one round, balanced within a step of the ideal
    for rows, st in (([256, 32, 32], 64), ([256], 64), ([896, 896], 64), ([256], 224)):
        d = _plan(rows, [st] * len(rows), [0] * len(rows), [Z] * len(rows))
        ideal = -(-sum(rows) * st // 1024)
        busy = _check_plan(d, rows, [st] * len(rows), [0] * len(rows), 16)
        assert d["items"] <= 256 and ideal <= busy <= ideal + max(2, ideal // 8) + (2 if len(rows) > 1 else 0), (rows, st, busy, ideal)
    # two geometry classes in one launch (any-KV: single- and two-stream jobs), odd shapes, 8-wave workgroups
    rows, s1, s2 = [128, 32, 32], [32, 16, 32], [0, 16, 0]
    d = _plan(rows, s1, s2, [Z] * 3)
    assert d["ncls"] == 2 and d["mask"] == 0b010
    _check_plan(d, rows, s1, s2, 16)
    for rows, st1_, st2_, waves in (([7], [5], [0], 16), ([3, 1000], [9, 9], [4, 4], 16), ([33], [1], [1], 16), ([64], [32], [32], 8),
                                    ([1], [448], [0], 16), ([2000], [2], [0], 16)):
        d = _plan(rows, st1_, st2_, [Z] * len(rows), waves=waves)
        _check_plan(d, rows, st1_, st2_, waves)
    # the SwiGLU epilogue: whole rows, a power-of-two count per workgroup, the up row's lead marked
    d = _plan([896], [16], [16], [4 | Z])
    pl = d["cls"][0]
    assert pl["lg"] == 0 and pl["rg"] in (2, 4, 8, 16) and all(j["sk"] == 1 for j in d["jobs"])
    leads = [(a & 255, (a >> 17) & 1) for a, b in pl["w"][0] if (a >> 9) & 1]
    assert leads and all(flag == (1 - row % 2) for row, flag in leads)


def test_host_path_trace_matches_the_golden_record(tmp_path):
    """The host side of every fused GEMV / lockstep GEMM launch (csrc/qpal_capi.hip: argument checks, the split per row geometry,
    the planners, the memsets in front of split-K launches) never dereferences a device pointer, so it runs without a GPU:
    tests/capi_trace.hip links qpal_capi.hip, compiled host-only, against recording stubs of the launchers and the memsets and sweeps
    qpal_tcq_gemv, qpal_tcq_gemv_multi, qpal_lut_tc_gemv and qpal_lut_tc_gemv_multi with made-up addresses — every codec, batch
    group, split, job variation and argument error, and a reduced sweep per knob in a process of its own.  Each case's return code
    and the digest of its recorded calls (launcher, integer arguments, every field of the parameter block; memset pointers and
    sizes) must be the golden file's: a host-path change that computes another launch for any case is caught here."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_capi_trace", os.path.join(ROOT, "tests", "golden", "make_golden_capi_trace.py"))
    tr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tr)
    exe = tr.build(str(tmp_path))
    got = tr.run_all(exe)
    want = tr.read_golden()
    assert [name for name, _, _ in tr.RUNS] == list(want), "the golden file's sections are the runs, in order"
    assert len(got["default"]) >= 4000 and all(len(got[name]) >= 700 for name in got)
    report = tr.compare(exe, got, want)
    assert not report, report


# every QPAL_* name the preprocessor may test (or the Makefile may define) in the native sources ...
_QPAL_BUILD_SWITCHES = {
    "QPAL_STAMPS",       # diagnostic build, make STAMPS=1
    "QPAL_HESSIAN_KB",   # hessian.hip: the K block, overridable for its own measurements
    "QPAL_TCQ", "QPAL_LUT", "QPAL_GEMM_NBG",  # X-macro names a unit #defines in front of a table / an instantiation file
}
# ... and every QPAL_* environment variable the library or the package may read
_QPAL_ENV_SWITCHES = {
    "QPAL_FORCE_G", "QPAL_FORCE_RG", "QPAL_SHARE", "QPAL_PAIR", "QPAL_PLAN_LOG", "QPAL_GEMM_MIN_BATCH",  # test hooks (qpal_capi.hip)
    "QPAL_STAMPS_BUF", "QPAL_STAMPS_DUMP",  # the stamp build only (gemv_stamps.h)
    "QPAL_LIB", "QPAL_LAZY_OPS",            # Python: which library, eager op registration
}


def _qpal_switches(text, makefile=False):
    """(names tested by #if / #ifdef / #ifndef / #elif or defined by a -D flag of a Makefile, names read from the environment)"""
    built, env = set(), set()
    for line in text.splitlines():
        if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", line):
            built |= set(re.findall(r"\bQPAL_\w+", line.split("//")[0]))
        if makefile:
            built |= set(re.findall(r"-D(QPAL_\w+)", line.split("#")[0]))
        if re.search(r"\b(getenv|env_int|environ)\b", line):
            env |= set(re.findall(r"""["'](QPAL_\w+)["']""", line))
    return built, env


def test_experiment_switches_stay_out_of_the_product():
    """The fused GEMV's headers once carried a second configuration and a handful of knock-out switches, and the library read eleven
    environment variables nothing used.  They are gone; this keeps the list from growing back: every QPAL_* name a native source tests
    in the preprocessor, and every QPAL_* name the library or the Python package reads from the environment, is spelled out above."""
    csrc = os.path.join(ROOT, "q-palette_amd", "csrc")
    files = [os.path.join(csrc, f) for f in sorted(os.listdir(csrc)) if f.endswith((".h", ".hip", ".inc")) or f == "Makefile"]
    for d, _, names in os.walk(os.path.join(ROOT, "q-palette_amd")):
        files += [os.path.join(d, f) for f in sorted(names) if f.endswith(".py")]
    assert len(files) >= 60 and any(f.endswith("Makefile") for f in files) and any(f.endswith("vq_linear.py") for f in files)
    built, env, bad = set(), set(), []
    for path in files:
        with open(path) as fh:
            b, e = _qpal_switches(fh.read(), makefile=path.endswith("Makefile"))
        built |= b
        env |= e
        bad += [f"{os.path.relpath(path, ROOT)}: {n}" for n in sorted((b - _QPAL_BUILD_SWITCHES) | (e - _QPAL_ENV_SWITCHES))]
    assert not bad, "QPAL_* switches outside the allow-lists:\n" + "\n".join(bad)
    # the scan sees what is there (a scanner that finds nothing would pass anything) ...
    assert {"QPAL_STAMPS", "QPAL_HESSIAN_KB"} <= built and _QPAL_ENV_SWITCHES <= env, (built, env)
    # ... in every form the sources use
    assert _qpal_switches('#if defined(QPAL_A) && !defined(QPAL_B)  // QPAL_C\n  # elif QPAL_D != 0\n#define QPAL_E 1\n#ifndef QPAL_F') == \
        ({"QPAL_A", "QPAL_B", "QPAL_D", "QPAL_F"}, set())
    assert _qpal_switches('x = getenv("QPAL_A") != nullptr; env_int("QPAL_B", env_int("QPAL_C", 1));\n'
                          "os.environ.get('QPAL_D'); os.environ[\"QPAL_E\"]; 'QPAL_F' in os.environ\nQPAL_G = \"QPAL_H\"") == \
        (set(), {"QPAL_A", "QPAL_B", "QPAL_C", "QPAL_D", "QPAL_E", "QPAL_F"})
    assert _qpal_switches('CXXFLAGS += -DQPAL_A $(EXTRA)  # -DQPAL_B', makefile=True) == ({"QPAL_A"}, set())
