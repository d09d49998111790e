"""Ragged prefill: rows of several sequences in one launch (csrc/attn_ragged.hip, qpalette_amd.ragged_prefill_attention /
paged_ragged_prefill_attention) and the whole-model decoder.RaggedStep.

CPU: the C-ABI is exported, the workspace size is monotone, argument errors are return codes, the wrappers check the segment
descriptors first, RaggedStep.pack_host's rules.
GPU: per segment, parity with qpal_rope_kv's cache bytes (e4m3: the §16 store rule of them), a torch fp32 restatement and the
one-sequence prefill_attention launches (bitwise where one chunk serves: max_len 128); isolation of a segment from its neighbours;
inactive segments; paged against contiguous; graph replay with the descriptors rewritten on the device; the whole model against
Prefill and DecodeStep.  Tolerances are tests/test_prefill.py's (atol = rtol = 2e-3; whole model 2^-7 max(1, max |ref|))."""
import math
import os
import sys

import pytest
import torch

import qpalette_amd as qp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_SHAPE, E_NULL, E_ALIGN = -1, -3, -4
F16, F8 = torch.float16, torch.float8_e4m3fn
DTYPES = [F16, F8]
SHAPES = [(8, 2, 64), (8, 1, 128), (4, 4, 128), (4, 2, 256)]  # nq, nkv, hd
B = 4
GARBAGE = 0x7FFFFFF0  # a block-table entry nobody may read


def _bits(t):
    """the tensor's bytes as integers (fp16 -> int16, e4m3 -> uint8)"""
    return t.view(torch.int16) if t.dtype == F16 else t.view(torch.uint8)


# ---------------------------------------------------------------------------------------------------------------- CPU

@pytest.fixture(scope="module")
def lib():
    return qp._native.lib()


def test_ragged_symbols_are_exported(lib):
    for name in ("qpal_attn_rope_prefill_ragged", "qpal_attn_rope_prefill_ragged_paged", "qpal_attn_ragged_ws_bytes"):
        assert name in qp._native.exported_symbols()
        assert hasattr(lib, name)
    for f in (qp.ragged_prefill_attention, qp.paged_ragged_prefill_attention, qp.ragged_workspace, qp.RaggedStep):
        assert callable(f)
    with open(os.path.join(ROOT, "include", "qpal.h")) as f:
        hdr = f.read()
    assert "qpal_attn_rope_prefill_ragged(" in hdr and "qpal_attn_rope_prefill_ragged_paged(" in hdr and "qpal_attn_ragged_ws_bytes(" in hdr


def test_ragged_workspace_size_is_monotone(lib):
    ws = lib.qpal_attn_ragged_ws_bytes
    for nq, nkv, hd in SHAPES + [(32, 8, 128), (64, 8, 128)]:
        for L in (4, 128, 508):  # short caches: one chunk per (kv head, query tile), no workspace
            assert all(ws(R, S, nq, nkv, hd, L) == 0 for R in (1, 16, 128) for S in (1, 16, 128))
        for L in (512, 2048, 4096, 65536):
            for S in (1, 3, 16, 128):
                sizes = [ws(R, S, nq, nkv, hd, L) for R in range(1, 129)]
                assert all(s > 0 and s % 4 == 0 for s in sizes)
                assert all(a <= b for a, b in zip(sizes, sizes[1:])), (nq, nkv, hd, L, S)  # monotone in R
            for R in (1, 7, 64, 128):
                sizes = [ws(R, S, nq, nkv, hd, L) for S in range(1, 129)]
                assert all(a <= b for a, b in zip(sizes, sizes[1:])), (nq, nkv, hd, L, R)  # monotone in S
        for R, S in ((1, 1), (7, 3), (128, 16), (128, 128)):
            sizes = [ws(R, S, nq, nkv, hd, L) for L in range(4, 65536 + 4, 508)]
            assert all(a <= b for a, b in zip(sizes, sizes[1:])), (nq, nkv, hd, R, S)  # monotone in max_len
    # no workspace for shapes the launch rejects
    assert ws(0, 4, 32, 8, 128, 4096) == 0 and ws(129, 4, 32, 8, 128, 4096) == 0 and ws(4, 0, 32, 8, 128, 4096) == 0
    assert ws(4, 129, 32, 8, 128, 4096) == 0 and ws(4, 4, 24, 8, 128, 4096) == 0 and ws(4, 4, 32, 8, 96, 4096) == 0
    assert ws(4, 4, 32, 8, 128, 4098) == 0 and ws(4, 4, 64, 8, 256, 4096) == 0


def _call(lib, paged, q=16, k=16, v=16, ld=4096, kc=4096, vc=4096, out=16, ld_out=4096, seq=16, row0=16, pos=16, inv=16, tab=16,
          ld_tab=64, pages=100, ps=16, mp=64, fmt=0, R=128, S=4, nb=4, nq=32, nkv=8, hd=128, L=1024, ws=16, ws_bytes=1 << 30):
    if paged:
        return lib.qpal_attn_rope_prefill_ragged_paged(q, k, v, ld, kc, vc, out, ld_out, seq, row0, pos, inv, tab, ld_tab, pages, ps, mp,
                                                       fmt, R, S, nb, nq, nkv, hd, 0.1, ws, ws_bytes, None)
    return lib.qpal_attn_rope_prefill_ragged(q, k, v, ld, kc, vc, out, ld_out, seq, row0, pos, inv, fmt, R, S, nb, nq, nkv, hd, L, 0.1, ws,
                                             ws_bytes, None)


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("paged", [False, True])
def test_ragged_argument_errors_without_a_gpu(lib, paged, fmt):
    """Every argument error is returned before any stream work (the pointers below are never dereferenced): the siblings' list of
    perturbations and codes, plus the descriptors, S, B and kv_fmt."""
    call = lambda **kw: _call(lib, paged, **{"fmt": fmt, **kw})
    for kw in ({"q": None}, {"k": None}, {"v": None}, {"kc": None}, {"vc": None}, {"out": None}, {"pos": None}, {"inv": None},
               {"seq": None}, {"row0": None}, {"ws": None}):  # (1024 positions: the split form needs its workspace)
        assert call(**kw) == E_NULL, kw
    for kw in ({"hd": 96}, {"hd": 32}, {"nq": 24}, {"nq": 48}, {"nq": 128}, {"R": 0}, {"R": 129}, {"hd": 256, "nq": 64}, {"ld": 4095},
               {"ld_out": 100}, {"ws_bytes": 4}, {"S": 0}, {"S": 129}, {"S": -1}, {"nb": 0}, {"fmt": 2}, {"fmt": -1}):
        assert call(**kw) == E_SHAPE, kw
    for kw in ({"kc": 4096 + 8}, {"vc": 4096 + 2}, {"q": 18}, {"pos": 17}, {"out": 17}, {"ws": 18}, {"seq": 18}, {"row0": 17}):
        assert call(**kw) == E_ALIGN, kw
    if paged:
        assert call(tab=None) == E_NULL and call(tab=18) == E_ALIGN
        for kw in ({"ps": 24}, {"ps": 8}, {"pages": 0}, {"mp": 0}, {"ld_tab": 63}):
            assert call(**kw) == E_SHAPE, kw
    else:
        assert call(L=1022) == E_SHAPE and call(L=0) == E_SHAPE


def test_ragged_wrappers_check_the_descriptors_before_the_library(monkeypatch):
    """the dtype / length / device / contiguity checks of seq, row0 and pos0 come first and need neither a GPU nor the library"""
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(qp._native, "lib", no_library)
    z = torch.zeros
    i32, i64 = torch.int32, torch.int64
    good = dict(q=z(4, 8), k=z(4, 8), v=z(4, 8), kcache=z(2, 1, 8, 8).half(), vcache=z(2, 1, 8, 8).half(), seq=z(2, dtype=i32),
                row0=z(3, dtype=i32), pos0=z(2, dtype=i64), inv_freq=z(4))
    pgood = dict(good, kpool=z(4, 1, 16, 8).half(), vpool=z(4, 1, 16, 8).half(), block_table=z(2, 2, dtype=i32))
    del pgood["kcache"], pgood["vcache"]
    bad = [({"seq": z(2, dtype=i64)}, "seq"), ({"seq": z(0, dtype=i32)}, "seq"), ({"seq": z(129, dtype=i32), "row0": z(130, dtype=i32),
           "pos0": z(129, dtype=i64)}, "seq"), ({"seq": z(2, 1, dtype=i32)}, "seq"), ({"seq": z(4, dtype=i32)[::2]}, "seq"),
           ({"row0": z(3, dtype=i64)}, "row0"), ({"row0": z(2, dtype=i32)}, "row0"), ({"row0": z(4, dtype=i32)}, "row0"),
           ({"pos0": z(2, dtype=i32)}, "pos0"), ({"pos0": z(3, dtype=i64)}, "pos0"), ({"pos0": z(4, dtype=i64)[::2]}, "pos0"),
           ({"seq": z(2, dtype=i32, device="meta")}, "seq must be on"), ({"row0": z(3, dtype=i32, device="meta")}, "row0 must be on"),
           ({"pos0": z(2, dtype=i64, device="meta")}, "pos0 must be on")]
    for kw, what in bad:
        with pytest.raises(qp._native.QpalError, match=what):
            qp.ragged_prefill_attention(**{**good, **kw})
        with pytest.raises(qp._native.QpalError, match=what):
            qp.paged_ragged_prefill_attention(**{**pgood, **kw})
    # good descriptors: the next check speaks (host caches), still before the library
    with pytest.raises(qp._native.QpalError, match="kcache"):
        qp.ragged_prefill_attention(**good)
    with pytest.raises(qp._native.QpalError, match="shape"):
        qp.ragged_prefill_attention(**{**good, "kcache": z(1, 8, 8).half()})
    with pytest.raises(qp._native.QpalError, match="int32"):
        qp.paged_ragged_prefill_attention(**{**pgood, "block_table": z(2, 2, dtype=i64)})


def test_pack_rules():
    pack = lambda items, rows=16, segments=4, slots=3, context=64: qp.RaggedStep.pack_host(items, rows, segments, slots, context)
    ar = lambda n: torch.arange(1, n + 1)
    tokens, seq, row0, pos0 = pack([(2, ar(5), 0), (0, ar(1), 63), (1, ar(10), 7)])
    assert tokens.tolist() == list(range(1, 6)) + [1] + list(range(1, 11)) and tokens.dtype == torch.int64
    assert seq.tolist() == [2, 0, 1, -1] and seq.dtype == torch.int32
    assert row0.tolist() == [0, 5, 6, 16, 16] and row0.dtype == torch.int32
    assert pos0.tolist() == [0, 63, 7, 0] and pos0.dtype == torch.int64
    assert pack([])[2].tolist() == [0] * 5
    for items in ([(0, ar(2), 0), (0, ar(2), 9)],                       # one slot twice
                  [(0, ar(9), 0), (1, ar(8), 0)],                       # more than `rows` rows
                  [(0, ar(17), 0)],
                  [(0, ar(1), 0), (1, ar(1), 0), (2, ar(1), 0), (3, ar(1), 0), (4, ar(1), 0)],  # more than `segments` items
                  [(3, ar(1), 0)], [(-1, ar(1), 0)],                     # a slot the caches do not have
                  [(0, ar(2), 63)], [(0, ar(1), -1)], [(0, ar(1), 64)],  # an item that does not fit the cache
                  [(0, ar(0), 0)], [(0, ar(2).int(), 0)], [(0, ar(4).view(2, 2), 0)]):
        with pytest.raises(qp._native.QpalError):
            pack(items)


# ---------------------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _inv_freq(hd, dev):
    return 1.0 / (500000.0 ** (torch.arange(0, hd, 2, device=dev).float() / hd))


def _tq(nq, nkv):
    rep = nq // nkv
    return 16 * (1 if rep >= 4 else 4 // rep)


def _ntile(R, S, nq, nkv):
    tq = _tq(nq, nkv)
    return min(R, (R + S * (tq - 1)) // tq)


TICKETS = 128  # ticket words per kv head at the front of a ragged workspace, whatever the launch's R and S


def _e4m3(h):
    """the §16 store rule of fp16 rows h"""
    return h.float().clamp(-448, 448).to(F8)


class Case:
    """R rows of q | k | v (a padded row stride), caches [B, nkv, L, hd] of `dtype` with random context and NaN in the rows the
    active segments will write, and the descriptors of segments (slot, rows, pos0)"""

    def __init__(self, dev, shape, segs, L, dtype, seed, R=None):
        nq, nkv, hd = shape
        self.shape, self.L, self.dtype, self.segs, self.dev = shape, L, dtype, segs, dev
        total = sum(max(t, 0) for _, t, _ in segs)
        self.R = min(128, total + 2) if R is None else R
        gen = torch.Generator(device=dev).manual_seed(seed)
        W = nq * hd + 2 * nkv * hd
        qkv = torch.randn(self.R, W + 8, device=dev, generator=gen)
        self.q, self.k, self.v = qkv[:, :nq * hd], qkv[:, nq * hd:nq * hd + nkv * hd], qkv[:, nq * hd + nkv * hd:W]
        self.kc0 = (torch.randn(B, nkv, L, hd, device=dev, generator=gen) * 0.5).to(dtype)
        self.vc0 = (torch.randn(B, nkv, L, hd, device=dev, generator=gen) * 0.5).to(dtype)
        row0, at = [0], 0
        for slot, t, p0 in segs:
            at += max(t, 0)
            row0.append(at)
            if self.active(slot, t, p0, at):
                for c in (self.kc0, self.vc0):
                    _bits(c)[slot, :, p0:p0 + t] = 0x7E00 if dtype == F16 else 0x7F
        self.row0_list = row0
        self.seq = torch.tensor([s for s, _, _ in segs], dtype=torch.int32, device=dev)
        self.row0 = torch.tensor(row0, dtype=torch.int32, device=dev)
        self.pos0 = torch.tensor([p for _, _, p in segs], dtype=torch.int64, device=dev)
        self.inv_freq = _inv_freq(hd, dev)
        self.ws = qp.ragged_workspace(self.R, len(segs), nq, nkv, hd, L, dev)
        assert (self.ws is None) == (L < 512)

    def active(self, slot, t, p0, end):
        return t > 0 and end <= self.R and 0 <= slot < B and p0 >= 0 and p0 + t <= self.L

    def launch(self, kc, vc, out=None, **kw):
        if out is None:
            out = torch.full((self.R, self.shape[0] * self.shape[2]), 3.0, dtype=torch.float16, device=self.dev)
        a = dict(seq=self.seq, row0=self.row0, pos0=self.pos0)
        a.update(kw)
        return qp.ragged_prefill_attention(self.q, self.k, self.v, kc, vc, a["seq"], a["row0"], a["pos0"], self.inv_freq, out=out, ws=self.ws)

    def tickets_are_zero(self):
        if self.ws is None:
            return True
        return int(self.ws.view(torch.int32)[: TICKETS * self.shape[1]].abs().max()) == 0

    def reference(self):
        """per active segment: the rows qpal_rope_kv writes one by one (e4m3: their stored bytes) -> the expected caches, the torch
        fp32 attention on them, and the one-sequence prefill_attention launch on a copy of the initial caches"""
        nat = qp._native
        nq, nkv, hd = self.shape
        kc_ref, vc_ref = self.kc0.clone(), self.vc0.clone()
        refs = []
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        for s, (slot, t, p0) in enumerate(self.segs):
            r0 = self.row0_list[s]
            if not self.active(slot, t, p0, self.row0_list[s + 1]):
                refs.append(None)
                continue
            qc, kk, vv = self.q[r0:r0 + t].contiguous(), self.k[r0:r0 + t].contiguous(), self.v[r0:r0 + t].contiguous()
            k16 = torch.zeros(nkv, self.L, hd, dtype=F16, device=self.dev)
            v16 = torch.zeros_like(k16)
            q16 = torch.zeros(t, nq * hd, dtype=F16, device=self.dev)
            pos = torch.arange(p0, p0 + t, dtype=torch.long, device=self.dev)
            for i in range(t):
                nat.check(nat.lib().qpal_rope_kv(qc[i].data_ptr(), kk[i].data_ptr(), vv[i].data_ptr(), q16[i].data_ptr(), k16.data_ptr(),
                                                 v16.data_ptr(), pos[i:i + 1].data_ptr(), self.inv_freq.data_ptr(), nq, nkv, hd, self.L,
                                                 stream), "qpal_rope_kv")
            for c, h in ((kc_ref, k16), (vc_ref, v16)):
                _bits(c)[slot, :, p0:p0 + t] = _bits(h[:, p0:p0 + t] if self.dtype == F16 else _e4m3(h[:, p0:p0 + t]))
            # row i: softmax(q k^T / sqrt(hd)) v over 0 .. p0 + i of the resulting cache (causal, GQA by repeat_interleave), fp32
            n = p0 + t
            qf = q16.view(t, nq, hd).float().transpose(0, 1)
            kf = kc_ref[slot, :, :n].float().repeat_interleave(nq // nkv, dim=0)
            vf = vc_ref[slot, :, :n].float().repeat_interleave(nq // nkv, dim=0)
            sc = qf @ kf.transpose(-1, -2) / math.sqrt(hd)
            keep = torch.arange(n, device=self.dev)[None, :] <= (p0 + torch.arange(t, device=self.dev))[:, None]
            ref = (torch.softmax(sc.masked_fill(~keep[None], float("-inf")), dim=-1) @ vf).transpose(0, 1).reshape(t, nq * hd)
            kc1, vc1 = self.kc0[slot].clone(), self.vc0[slot].clone()
            one = qp.prefill_attention(self.q[r0:r0 + t], self.k[r0:r0 + t], self.v[r0:r0 + t], kc1, vc1,
                                       torch.tensor([p0], dtype=torch.long, device=self.dev), self.inv_freq,
                                       ws=qp.prefill_workspace(t, nq, nkv, hd, self.L, self.dev))
            assert torch.equal(_bits(kc1), _bits(kc_ref[slot])) and torch.equal(_bits(vc1), _bits(vc_ref[slot]))
            refs.append((ref, one))
        return kc_ref, vc_ref, refs


def _segments(Ts, L):
    """slots in a permuted order; positions: mid-cache, 0, the cache's end, mid-cache"""
    slots = [2, 0, 3, 1]
    want = [3, 0, L, 40] if L == 128 else [700, 0, L, 1500]
    return [(slots[s], t, max(0, min(want[s], L - t))) for s, t in enumerate(Ts)]


SEGMENT_LISTS = [[1, 1, 1, 1], [17, 1, 16, 30], [128], [5, 0, 3, 120]]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "fp8"])
@pytest.mark.parametrize("L", [128, 2048])
@pytest.mark.parametrize("Ts", SEGMENT_LISTS, ids=lambda t: "-".join(map(str, t)))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ragged_parity(dev, shape, Ts, L, dtype):
    c = Case(dev, shape, _segments(Ts, L), L, dtype, seed=sum(Ts) + shape[0] + shape[2] + L)
    kc, vc = c.kc0.clone(), c.vc0.clone()
    out = c.launch(kc, vc)
    torch.cuda.synchronize()
    kc_ref, vc_ref, refs = c.reference()
    # the cache append: the segments' rows bit for bit qpal_rope_kv's (e4m3: their stored bytes), every other byte unchanged
    assert torch.equal(_bits(kc), _bits(kc_ref)) and torch.equal(_bits(vc), _bits(vc_ref))
    written = torch.zeros(c.R, dtype=torch.bool, device=dev)
    for s, r in enumerate(refs):
        if r is None:
            continue
        ref, one = r
        rows = slice(c.row0_list[s], c.row0_list[s + 1])
        written[rows] = True
        got = out[rows]
        e_ref, e_one = float((got.float() - ref).abs().max()), float((got.float() - one.float()).abs().max())
        print(f"ragged parity {shape} T={Ts} L={L} {dtype} segment {s}: max |diff| torch {e_ref:.3e}, prefill_attention {e_one:.3e}")
        assert torch.allclose(got.float(), ref, atol=2e-3, rtol=2e-3), e_ref
        assert torch.allclose(got.float(), one.float(), atol=2e-3, rtol=2e-3), e_one
        if L == 128:  # one chunk, no workspace: the same arithmetic in the same order
            assert torch.equal(_bits(got), _bits(one)), s
    assert bool(written.any()) and bool((out[~written] == 3.0).all()), "rows of no active segment keep what they held"
    assert c.tickets_are_zero(), "tickets must be back at zero after a launch"
    # a second launch on the restored state: bitwise the same (fixed merge order, no float atomics)
    kc2, vc2 = c.kc0.clone(), c.vc0.clone()
    out2 = c.launch(kc2, vc2)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(kc2), _bits(kc_ref)) and torch.equal(_bits(vc2), _bits(vc_ref))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "fp8"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_a_segment_does_not_depend_on_its_neighbours(dev, shape, dtype):
    """segment 1 alone (the others with no rows) against the same segment among three others: same R, S and max_len = 2048, so the
    same grid and chunks; its out rows and cache rows are bitwise equal, and alone it leaves the other sequences' caches untouched"""
    L = 2048
    c = Case(dev, shape, _segments([17, 33, 16, 30], L), L, dtype, seed=11 + shape[2])
    kc, vc = c.kc0.clone(), c.vc0.clone()
    out = c.launch(kc, vc)
    lo, hi = c.row0_list[1], c.row0_list[2]
    row0_alone = torch.tensor([lo, lo, hi, hi, hi], dtype=torch.int32, device=dev)
    kc1, vc1 = c.kc0.clone(), c.vc0.clone()
    out1 = c.launch(kc1, vc1, row0=row0_alone)
    torch.cuda.synchronize()
    slot = c.segs[1][0]
    assert torch.equal(_bits(out1[lo:hi]), _bits(out[lo:hi]))
    assert bool((out1[:lo] == 3.0).all()) and bool((out1[hi:] == 3.0).all())
    assert torch.equal(_bits(kc1[slot]), _bits(kc[slot])) and torch.equal(_bits(vc1[slot]), _bits(vc[slot]))
    assert not torch.equal(_bits(kc1[slot]), _bits(c.kc0[slot]))
    others = [b for b in range(B) if b != slot]
    assert torch.equal(_bits(kc1[others]), _bits(c.kc0[others])) and torch.equal(_bits(vc1[others]), _bits(c.vc0[others]))
    assert c.tickets_are_zero()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "fp8"])
@pytest.mark.parametrize("L", [128, 2048])
@pytest.mark.parametrize("why", ["pos0 = -1", "pos0 + T > max_len", "seq = B", "row0[s+1] > R"])
def test_an_inactive_segment_touches_nothing(dev, why, L, dtype):
    """one segment made inactive: its out rows (3.0) and its sequence's cache are unchanged, the other segments' out rows and caches
    are bitwise what they are in the launch where it is active"""
    shape = (8, 1, 128)
    segs = _segments([9, 20, 1, 31], L)
    victim = 3 if why == "row0[s+1] > R" else 1
    c = Case(dev, shape, segs, L, dtype, seed=L + len(why), R=sum(t for _, t, _ in segs))
    seq, row0, pos0 = c.seq.clone(), c.row0.clone(), c.pos0.clone()
    if why == "pos0 = -1":
        pos0[victim] = -1
    elif why == "pos0 + T > max_len":
        pos0[victim] = L - segs[victim][1] + 1
    elif why == "seq = B":
        seq[victim] = B
    else:
        row0[victim + 1] = c.R + 1
    kc, vc = c.kc0.clone(), c.vc0.clone()
    out = c.launch(kc, vc, seq=seq, row0=row0, pos0=pos0)
    # the yardstick for the other segments: the launch of the same R, S and max_len (the same grid) in which all four are active
    kc_all, vc_all = c.kc0.clone(), c.vc0.clone()
    out_all = c.launch(kc_all, vc_all)
    torch.cuda.synchronize()
    lo, hi = c.row0_list[victim], c.row0_list[victim + 1]
    slot = segs[victim][0]
    assert bool((out[lo:hi] == 3.0).all()), why
    assert torch.equal(_bits(kc[slot]), _bits(c.kc0[slot])) and torch.equal(_bits(vc[slot]), _bits(c.vc0[slot])), why
    assert not torch.equal(_bits(kc_all[slot]), _bits(c.kc0[slot])) and not bool((out_all[lo:hi] == 3.0).all())
    rest = [r for r in range(c.R) if not lo <= r < hi]
    others = [b for b in range(B) if b != slot]
    assert torch.equal(_bits(out[rest]), _bits(out_all[rest]))
    assert torch.equal(_bits(kc[others]), _bits(kc_all[others])) and torch.equal(_bits(vc[others]), _bits(vc_all[others]))
    assert c.tickets_are_zero()


class Paged:
    """tests/test_paged_kv.py's scatter: contiguous caches [B, nkv, L, hd] into pools of about twice the pages through a seeded
    random permutation; unowned pages hold the NaN pattern"""

    def __init__(self, kc, vc, page_size, seed):
        nb, nkv, L, hd = kc.shape
        self.ps, self.mp, self.B = page_size, L // page_size, nb
        need = nb * self.mp
        self.num_pages = 2 * need + 1
        perm = torch.randperm(self.num_pages, generator=torch.Generator().manual_seed(seed))
        self.table = perm[:need].view(nb, self.mp).to(torch.int32).to(kc.device)
        self.unowned = perm[need:].to(kc.device)
        self.nan = 0x7E00 if kc.dtype == F16 else 0x7F
        pools = []
        for c in (kc, vc):
            pool = torch.empty((self.num_pages, nkv, page_size, hd), dtype=torch.uint8 if c.dtype == F8 else F16, device=c.device).view(c.dtype)
            _bits(pool).fill_(self.nan)
            _bits(pool)[self.table.long()] = _bits(c).view(nb, nkv, self.mp, page_size, hd).transpose(1, 2)
            pools.append(pool)
        self.kpool, self.vpool = pools

    def gather(self, pool):
        g = _bits(pool)[self.table.long()]  # [B, mp, nkv, ps, hd]
        return g.transpose(1, 2).reshape(self.B, g.shape[2], self.mp * self.ps, g.shape[4])

    def launch_table(self, last_pos):
        """every entry past the page of a sequence's last position is garbage (all of a sequence without a segment)"""
        t = self.table.clone()
        for b, p in enumerate(last_pos):
            t[b, (p // self.ps + 1 if p >= 0 else 0):] = GARBAGE
        return t

    def unowned_intact(self):
        return all(bool((_bits(pool)[self.unowned.long()] == self.nan).all()) for pool in (self.kpool, self.vpool))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "fp8"])
@pytest.mark.parametrize("ps", [16, 64])
@pytest.mark.parametrize("L", [128, 2048])
@pytest.mark.parametrize("shape", [(8, 2, 64), (8, 1, 128), (4, 2, 256)], ids=lambda s: "x".join(map(str, s)))
def test_paged_ragged_is_bitwise_the_contiguous_launch(dev, shape, L, ps, dtype):
    c = Case(dev, shape, _segments([17, 1, 16, 30] if ps == 16 else [5, 0, 3, 120], L), L, dtype, seed=L + ps + shape[2])
    kc, vc = c.kc0.clone(), c.vc0.clone()
    ref = c.launch(kc, vc)
    pg = Paged(c.kc0, c.vc0, ps, seed=ps + L)
    last = [-1] * B
    for slot, t, p0 in c.segs:
        if t > 0:
            last[slot] = p0 + t - 1
    out = torch.full_like(ref, 3.0)
    qp.paged_ragged_prefill_attention(c.q, c.k, c.v, pg.kpool, pg.vpool, pg.launch_table(last), c.seq, c.row0, c.pos0, c.inv_freq, out=out,
                                      ws=c.ws)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(ref))
    assert not torch.equal(_bits(kc), _bits(c.kc0)), "the contiguous launch appended nothing"
    assert torch.equal(pg.gather(pg.kpool), _bits(kc)) and torch.equal(pg.gather(pg.vpool), _bits(vc))
    assert pg.unowned_intact() and c.tickets_are_zero()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "fp8"])
def test_graph_replay_with_the_descriptors_rewritten_on_the_device(dev, dtype):
    """one captured launch; between replays one segment grows, another moves to a different slot and position: each replay equals
    an eager launch with the same descriptors, bitwise, caches included"""
    shape, L, R = (8, 1, 128), 2048, 64
    c = Case(dev, shape, [(2, 10, 600), (0, 1, 0), (3, 20, 1000)], L, dtype, seed=3, R=R)
    steps = [([2, 0, 3], [0, 10, 11, 31], [600, 0, 1000]),
             ([2, 1, 3], [0, 25, 26, 46], [610, 77, 1020]),      # segment 0 grows to 25 rows, segment 1 moves to slot 1
             ([3, 1, 0], [0, 25, 27, 64], [1040, 78, 1]),        # slots change hands, the last segment takes the rest of the rows
             ([3, 1, 0], [0, 0, 64, 64], [0, L - 64, 0])]        # one segment of 64 rows up to the cache's end, the others empty
    dt = lambda seq, row0, pos0: (torch.tensor(seq, dtype=torch.int32, device=dev), torch.tensor(row0, dtype=torch.int32, device=dev),
                                  torch.tensor(pos0, dtype=torch.int64, device=dev))
    kc_e, vc_e = c.kc0.clone(), c.vc0.clone()
    eager = []
    for st in steps:
        seq, row0, pos0 = dt(*st)
        eager.append(c.launch(kc_e, vc_e, seq=seq, row0=row0, pos0=pos0).clone())
    torch.cuda.synchronize()
    kc, vc = c.kc0.clone(), c.vc0.clone()
    seq, row0, pos0 = dt(*steps[0])
    out = torch.zeros(R, shape[0] * shape[2], dtype=torch.float16, device=dev)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        c.launch(c.kc0.clone(), c.vc0.clone(), out=out, seq=seq, row0=row0, pos0=pos0)  # warm-up on scratch caches
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            c.launch(kc, vc, out=out, seq=seq, row0=row0, pos0=pos0)
        got = []
        for st in steps:
            for dst, src in zip((seq, row0, pos0), dt(*st)):
                dst.copy_(src)
            out.fill_(3.0)
            g.replay()
            got.append(out.clone())
        torch.cuda.synchronize()
    for a, b in zip(eager, got):
        assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(_bits(kc), _bits(kc_e)) and torch.equal(_bits(vc), _bits(vc_e))
    assert c.tickets_are_zero()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "fp8"])
@pytest.mark.parametrize("shape", [(8, 1, 128), (4, 4, 128)], ids=lambda s: "x".join(map(str, s)))
def test_one_workspace_serves_launches_of_different_R_and_S(dev, shape, dtype):
    """one ragged_workspace(128, 16, ...) under a small launch (R = 16, S = 1: one query tile), a large one (R = 128, S = 16, four
    segments of 32 rows among empty ones: the grid this workspace is sized for), a shorter cache, and the small one again: each is bitwise the launch on a fresh workspace
    of its own shape, out and caches, and every ticket word is zero after each.  (A ticket array laid out by the launch's own ntile
    would put the small launch's partials where the large one looks for zeroed tickets.)"""
    nq, nkv, hd = shape
    L = 2048
    shared = qp.ragged_workspace(128, 16, nq, nkv, hd, L, dev)
    small = Case(dev, shape, [(1, 16, 900)], L, dtype, seed=5, R=16)
    large = Case(dev, shape, [(s // 4, 0 if s % 4 else 32, 300 + 100 * s) for s in range(16)], L, dtype, seed=6, R=128)
    short = Case(dev, shape, _segments([17, 1, 16, 30], 1024), 1024, dtype, seed=7)
    assert _ntile(16, 1, nq, nkv) < _ntile(128, 16, nq, nkv)
    assert shared.numel() >= max(c.ws.numel() for c in (small, large, short))
    for c in (small, large, short, small):
        kc_f, vc_f = c.kc0.clone(), c.vc0.clone()
        out_f = c.launch(kc_f, vc_f)
        fresh = c.ws
        kc_s, vc_s = c.kc0.clone(), c.vc0.clone()
        c.ws = shared
        out_s = c.launch(kc_s, vc_s)
        torch.cuda.synchronize()
        assert not bool((out_f[: c.row0_list[-1]] == 3.0).all()), "the launch on the fresh workspace wrote nothing"
        assert torch.equal(_bits(out_s), _bits(out_f)), (c.R, len(c.segs))
        assert torch.equal(_bits(kc_s), _bits(kc_f)) and torch.equal(_bits(vc_s), _bits(vc_f))
        assert c.tickets_are_zero()
        c.ws = fresh
        assert c.tickets_are_zero()


# -------------------------------------------------------------------------------------------------------- whole model

@pytest.fixture(scope="module")
def model(dev):
    sys.path.insert(0, os.path.join(ROOT, "perf"))
    from decode_llama import build_model
    return build_model("3_8b", "tcomb_6_7_0.5_none_0.9", None, 2, 4096, dev)


def _close(got, ref):
    """the whole-model tests' bound: max |diff| <= 2^-7 max(1, max |ref|)"""
    err, top = float((got.float() - ref.float()).abs().max()), float(ref.float().abs().max())
    return err <= 2.0 ** -7 * max(1.0, top), err, top


@pytest.mark.gpu
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_ragged_step_against_prefill_and_decode_step(dev, model, paged):
    """two layers of 3_8b, vocab 4096, context 512, four slots.  Step 1: prompts of 5 / 40 / 83 tokens (128 rows) in ONE RaggedStep
    against three Prefill calls.  Step 2: slots 2 and 0 decode one token each while slot 3 prefills 60 tokens, against DecodeStep +
    Prefill on the reference caches.  The same next tokens, each last-row final-norm state within 2^-7 max(1, max |ref|)."""
    m, nb, L, ps = model, 4, 512, 64
    nkv, hd, nl = m.cfg.num_key_value_heads, m.cfg.head_dim, len(m.layers)
    kc = [torch.zeros(nb, nkv, L, hd, dtype=F16, device=dev) for _ in range(nl)]  # the reference: contiguous caches
    vc = [t.clone() for t in kc]
    table = None
    if paged:
        cache = qp.PagedKVCache(nl, 2 * nb * (L // ps), nkv, ps, hd, nb, L // ps, device=dev)
        for n in (64, 128):  # page by page, slot after slot: no slot's pages are consecutive
            for slot in range(nb):
                cache.reserve(slot, n)
        kr, vr, table = cache.kpool, cache.vpool, cache.table
    else:
        kr, vr = [t.clone() for t in kc], [t.clone() for t in vc]
    pf = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, chunk=128)
    rs = qp.RaggedStep(m.layers, m.embed, m.norm, m.lm_head, kr, vr, m.inv_freq, rows=128, segments=4, block_table=table)
    assert rs.context == L
    g = torch.Generator().manual_seed(9)
    prompts = {2: torch.randint(0, 4096, (5,), generator=g).to(dev), 0: torch.randint(0, 4096, (40,), generator=g).to(dev),
               1: torch.randint(0, 4096, (83,), generator=g).to(dev)}
    rs.out_tok.fill_(7)
    got = rs(*rs.pack([(slot, toks, 0) for slot, toks in prompts.items()])).clone()
    got_h = rs.hidden().clone()
    nxt = {}
    for s, (slot, toks) in enumerate(prompts.items()):
        want = int(pf(toks, slot=slot, pos0=0))
        ok, err, top = _close(got_h[s], pf.hidden()[0])
        print(f"prompt of {len(toks)} in slot {slot}: tokens {want} / {int(got[s])}, hidden max |diff| {err:.3e} (max |ref| {top:.3f})")
        assert ok and int(got[s]) == want
        nxt[slot] = want
    assert int(got[3]) == 7, "an unused segment keeps its out_tok"
    # ---- a mixed step: two decode tokens and a 60-token prompt
    new = torch.randint(0, 4096, (60,), generator=g).to(dev)
    one = lambda slot: torch.tensor([nxt[slot]], dtype=torch.long, device=dev)
    got = rs(*rs.pack([(2, one(2), 5), (3, new, 0), (0, one(0), 40)])).clone()
    got_h = rs.hidden().clone()
    tok = torch.tensor([nxt[0], 0, nxt[2], 0], dtype=torch.long, device=dev)
    pos = torch.tensor([40, -1, 5, -1], dtype=torch.long, device=dev)
    out = torch.zeros(nb, dtype=torch.long, device=dev)
    ds = qp.DecodeStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, tok, pos, out, generic=True)
    ds()
    ds_h = ds.hidden().clone()
    want3 = int(pf(new, slot=3, pos0=0))
    for s, (slot, want, ref_h) in enumerate(((2, int(out[2]), ds_h[2]), (3, want3, pf.hidden()[0]), (0, int(out[0]), ds_h[0]))):
        ok, err, top = _close(got_h[s], ref_h)
        print(f"mixed step, slot {slot}: tokens {want} / {int(got[s])}, hidden max |diff| {err:.3e} (max |ref| {top:.3f})")
        assert ok and int(got[s]) == want


@pytest.mark.gpu
def test_ragged_step_draws_what_prefill_draws(dev, model):
    """a seeded Sampler with different parameters per slot: the token RaggedStep draws for a segment is the one Prefill draws for
    the same slot and position; with logprobs=True rs.draw.logprob is the log-prob launch's figure for that token and those logits"""
    m, nb, L = model, 4, 512
    nkv, hd, nl = m.cfg.num_key_value_heads, m.cfg.head_dim, len(m.layers)
    kc = [torch.zeros(nb, nkv, L, hd, dtype=F16, device=dev) for _ in range(nl)]
    vc = [t.clone() for t in kc]
    kr, vr = [t.clone() for t in kc], [t.clone() for t in vc]
    mk = lambda: qp.Sampler(nb, 4096, dev, temperature=[0.7, 1.0, 0.0, 1.3], top_k=[40, 0, 5, 3], top_p=[0.9, 0.95, 1.0, 1.0],
                            seed=[11, 12, 13, 14], logprobs=True)
    smp_p, smp_r = mk(), mk()
    pf = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, chunk=128, sampler=smp_p)
    rs = qp.RaggedStep(m.layers, m.embed, m.norm, m.lm_head, kr, vr, m.inv_freq, rows=128, segments=4, sampler=smp_r)
    g = torch.Generator().manual_seed(21)
    items = [(3, torch.randint(0, 4096, (30,), generator=g).to(dev), 0), (0, torch.randint(0, 4096, (7,), generator=g).to(dev), 0),
             (2, torch.randint(0, 4096, (50,), generator=g).to(dev), 0), (1, torch.randint(0, 4096, (41,), generator=g).to(dev), 0)]
    got = rs(*rs.pack(items)).clone()
    assert rs.ctr.tolist() == [29, 6, 49, 40]
    for s, (slot, toks, _) in enumerate(items):
        want = int(pf(toks, slot=slot, pos0=0))
        lp_p, lp_r = float(smp_p.logprob[slot]), float(rs.draw.logprob[s])
        print(f"slot {slot}: drawn {want} / {int(got[s])}, logprob {lp_p:.5f} / {lp_r:.5f}")
        assert int(got[s]) == want and lp_r <= 0.0 and math.isfinite(lp_r)
    assert torch.equal(qp.token_logprobs(rs.draw.logits, got), rs.draw.logprob)
