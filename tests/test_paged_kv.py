"""The paged KV cache: qpal_attn_rope_decode_batch_paged (csrc/attn_batch.hip), qpal_attn_rope_prefill_paged
(csrc/attn_prefill.hip), paged_decode_attention / paged_prefill_attention, paging.PagedKVCache and the decoder classes with a block table.

CPU: the symbols are exported, bound and declared; the contiguous siblings' argument errors come back with the same codes, the
paged-only ones with theirs; the Python layer rejects bad pools and tables; the allocator's rules.
GPU: the contract is bitwise — a paged launch equals the contiguous launch of max_len = max_pages * page_size on the gathered cache,
out rows and appended bytes, in both element formats.  Pages are handed out through a seeded random permutation of a pool twice
the needed size; every page nobody owns holds the NaN pattern and must still hold it afterwards; block-table entries past a
sequence's last position hold garbage.  The guard test allocates the pools as the middle pages of a buffer with one pattern page
on either side, so a wrong address would be seen without ever touching foreign memory."""
import os
import sys

import pytest
import torch

import qpalette_amd as qp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_SHAPE, E_NULL, E_ALIGN = -1, -3, -4
F16, F8 = torch.float16, torch.float8_e4m3fn
DTYPES = [F16, F8]
GARBAGE = 0x7FFFFFF0  # a block-table entry nobody may read


def _bits(t):
    """the tensor's bytes as integers (fp16 -> int16, e4m3 -> uint8)"""
    return t.view(torch.int16) if t.dtype == F16 else t.view(torch.uint8)


def _fill_nan(t):
    """the NaN pattern of an unowned page: fp16 0x7E00, e4m3 0x7F"""
    _bits(t).fill_(0x7E00 if t.dtype == F16 else 0x7F)


# ---------------------------------------------------------------------------------------------------------------- CPU

@pytest.fixture(scope="module")
def lib():
    return qp._native.lib()


def test_paged_symbols_are_exported_bound_and_declared(lib):
    with open(os.path.join(ROOT, "include", "qpal.h")) as f:
        hdr = f.read()
    for name, nargs in (("qpal_attn_rope_decode_batch_paged", 24), ("qpal_attn_rope_prefill_paged", 23)):
        assert name in qp._native.exported_symbols()
        assert hasattr(lib, name) and len(getattr(lib, name).argtypes) == nargs
        assert name + "(" in hdr
    assert qp.paged_decode_attention is qp.attention.paged_decode_attention
    assert qp.paged_prefill_attention is qp.attention.paged_prefill_attention
    assert qp.PagedKVCache is qp.paging.PagedKVCache


def _call(lib, name, q=16, k=16, v=16, ld=4096, kc=4096, vc=4096, out=16, ld_out=4096, pos=16, inv=16, B=4, nq=32, nkv=8, hd=128,
          L=1024, ws=16, ws_bytes=1 << 30, table=16, ld_table=None, num_pages=64, page_size=None, max_pages=None, kv_fmt=0):
    """tests/test_kv8.py's _call on a paged or a contiguous entry point: L becomes (page_size, max_pages) = (64, L / 64) where 64
    divides it (L = 0: no page), else (2, L / 2): a page size outside the set, the shape error an odd length is"""
    if not name.endswith("_paged"):
        return getattr(lib, name)(q, k, v, ld, kc, vc, out, ld_out, pos, inv, B, nq, nkv, hd, L, 0.1, ws, ws_bytes, None)
    if page_size is None:
        page_size = 64 if L % 64 == 0 else 2
    if max_pages is None:
        max_pages = L // page_size if page_size > 0 else 16
    if ld_table is None:
        ld_table = max(max_pages, 1)
    if name == "qpal_attn_rope_decode_batch_paged":
        return lib.qpal_attn_rope_decode_batch_paged(q, k, v, ld, kc, vc, out, ld_out, pos, inv, table, ld_table, num_pages, page_size,
                                                     max_pages, kv_fmt, B, nq, nkv, hd, 0.1, ws, ws_bytes, None)
    return lib.qpal_attn_rope_prefill_paged(q, k, v, ld, kc, vc, out, ld_out, pos, inv, table, num_pages, page_size, max_pages, kv_fmt,
                                            B, nq, nkv, hd, 0.1, ws, ws_bytes, None)


@pytest.mark.parametrize("kv_fmt", [0, 1])
@pytest.mark.parametrize("name", ["qpal_attn_rope_decode_batch", "qpal_attn_rope_prefill"])
def test_paged_argument_errors_are_the_contiguous_siblings(lib, name, kv_fmt):
    """tests/test_kv8.py's list of perturbations: the same code from the contiguous and the paged entry point, before any stream
    work (the pointers are never dereferenced); then the paged-only cases"""
    cases = [({"q": None}, E_NULL), ({"k": None}, E_NULL), ({"v": None}, E_NULL), ({"kc": None}, E_NULL), ({"vc": None}, E_NULL),
             ({"out": None}, E_NULL), ({"pos": None}, E_NULL), ({"inv": None}, E_NULL), ({"ws": None}, E_NULL)]
    cases += [(kw, E_SHAPE) for kw in ({"hd": 96}, {"hd": 32}, {"nq": 24}, {"nq": 48}, {"nq": 128}, {"B": 0}, {"B": 129}, {"L": 1022},
                                       {"L": 0}, {"hd": 256, "nq": 64}, {"ld": 4095}, {"ld_out": 100}, {"ws_bytes": 4})]
    cases += [(kw, E_ALIGN) for kw in ({"kc": 4096 + 8}, {"vc": 4096 + 2}, {"q": 18}, {"pos": 17}, {"out": 17}, {"ws": 18})]
    paged = name + "_paged"
    for kw, code in cases:
        assert _call(lib, paged, kv_fmt=kv_fmt, **kw) == code == _call(lib, name, **kw), kw
    only = [({"page_size": 8}, E_SHAPE), ({"page_size": 48}, E_SHAPE), ({"page_size": 512}, E_SHAPE), ({"page_size": 0}, E_SHAPE),
            ({"num_pages": 0}, E_SHAPE), ({"num_pages": -3}, E_SHAPE), ({"max_pages": 0}, E_SHAPE), ({"max_pages": -1}, E_SHAPE),
            ({"kv_fmt": 2}, E_SHAPE), ({"kv_fmt": -1}, E_SHAPE), ({"table": None}, E_NULL), ({"table": 18}, E_ALIGN)]
    if name.endswith("batch"):
        only.append(({"ld_table": 15}, E_SHAPE))
    for kw, code in only:
        assert _call(lib, paged, **{"kv_fmt": kv_fmt, **kw}) == code, kw


def test_python_layer_rejects_bad_pools_and_tables():
    z, Err = torch.zeros, qp._native.QpalError
    dec = dict(q=z(2, 8), k=z(2, 8), v=z(2, 8), pos=z(2, dtype=torch.long), inv_freq=z(4))
    pre = dict(q=z(2, 8), k=z(2, 8), v=z(2, 8), pos0=z(1, dtype=torch.long), inv_freq=z(4))
    for fn, args, tshape, tkey in ((qp.paged_decode_attention, dec, (2, 4), "block_table"), (qp.paged_prefill_attention, pre, (4,), "block_row")):
        tab = z(tshape, dtype=torch.int32)
        shape = (6, 1, 16, 8)
        with pytest.raises(Err, match="share one dtype"):
            fn(kpool=z(shape).to(F8), vpool=z(shape).half(), **{tkey: tab}, **args)
        with pytest.raises(Err, match="share one dtype"):
            fn(kpool=z(shape).half(), vpool=z(shape).to(F8), **{tkey: tab}, **args)
        for dt in (torch.float8_e5m2, torch.bfloat16, torch.uint8):
            with pytest.raises(Err, match="dtype must be"):
                fn(kpool=z(shape).to(dt), vpool=z(shape).to(dt), **{tkey: tab}, **args)
        for ps in (8, 48, 512):
            with pytest.raises(Err, match="page_size"):
                fn(kpool=z(6, 1, ps, 8).half(), vpool=z(6, 1, ps, 8).half(), **{tkey: tab}, **args)
        pools = dict(kpool=z(shape).half(), vpool=z(shape).half())
        for dt in (torch.int64, torch.int16, torch.float32):
            with pytest.raises(Err, match="int32"):
                fn(**pools, **{tkey: tab.to(dt)}, **args)
        wide = z(tshape[:-1] + (8,), dtype=torch.int32)[..., ::2]  # rows that are not contiguous
        with pytest.raises(Err, match="contiguous"):
            fn(**pools, **{tkey: wide}, **args)
        with pytest.raises(Err, match="device"):
            fn(**pools, **{tkey: tab.to("meta")}, **args)
        with pytest.raises(Err, match="shape"):
            fn(kpool=z(shape).half(), vpool=z(5, 1, 16, 8).half(), **{tkey: tab}, **args)
    with pytest.raises(Err, match="page_size"):
        qp.PagedKVCache(1, 4, 1, 24, 8, 1, 2)
    with pytest.raises(Err):
        qp.PagedKVCache(1, 4, 1, 16, 8, 1, 2, dtype=torch.bfloat16)


def test_allocator_rules():
    Err = qp._native.QpalError
    c = qp.PagedKVCache(2, 10, 2, 16, 8, 3, 4, dtype=F8)
    assert len(c.kpool) == len(c.vpool) == 2 and c.kpool[1].shape == (10, 2, 16, 8) and c.kpool[0].dtype == F8
    assert c.table.dtype == torch.int32 and c.table.shape == (3, 4) and bool((c.table == -1).all())
    assert c.pages_free == 10 and c.max_len == 64
    # bytes(): a pool against a contiguous cache of as many positions, both formats
    assert c.bytes() == qp.attention.kv_cache_bytes(1, 2, 10 * 16, 8, F8) == c.kpool[0].numel()
    assert qp.PagedKVCache(1, 10, 2, 16, 8, 3, 4).bytes() == qp.attention.kv_cache_bytes(10, 2, 16, 8) == 2 * c.bytes()
    # reserve grows only and is idempotent
    c.reserve(0, 17)
    p0 = c.pages_of(0)
    assert len(p0) == 2 and c.pages_free == 8 and c.table[0].tolist() == p0 + [-1, -1]
    c.reserve(0, 17)
    c.reserve(0, 3)
    c.reserve(0, 0)
    assert c.pages_of(0) == p0 and c.pages_free == 8
    c.reserve(0, 33)
    assert c.pages_of(0)[:2] == p0 and len(c.pages_of(0)) == 3 and c.table[0].tolist() == c.pages_of(0) + [-1]
    c.reserve(1, 64)
    assert c.pages_free == 3 and not set(c.pages_of(0)) & set(c.pages_of(1))
    # exhaustion and over-length raise and change nothing
    before = (c.table.clone(), c.pages_free, c.pages_of(2))
    with pytest.raises(Err):
        c.reserve(2, 64)
    with pytest.raises(Err):
        c.reserve(0, 65)
    with pytest.raises(Err):
        c.reserve(3, 1)
    assert torch.equal(c.table, before[0]) and c.pages_free == before[1] and c.pages_of(2) == before[2]
    # release returns exactly the pages taken
    took = set(c.pages_of(1))
    free0 = set(c._free)
    c.release(1)
    assert set(c._free) - free0 == took and c.pages_free == 7 and c.table[1].tolist() == [-1] * 4 and c.pages_of(1) == []
    c.release(1)
    assert c.pages_free == 7
    # fork: whole pages below n_positions are shared (count 2), the partial page is copied in every layer
    for pool in c.kpool + c.vpool:
        pool.view(torch.uint8).copy_(torch.randint(0, 255, pool.shape, dtype=torch.uint8))
    with pytest.raises(Err):
        c.fork(0, 0, 10)
    with pytest.raises(Err):
        c.fork(1, 0, 10)   # dst holds pages
    with pytest.raises(Err):
        c.fork(0, 1, 49)   # src has 48 reserved positions
    c.fork(0, 1, 40)
    s0, s1 = c.pages_of(0), c.pages_of(1)
    assert s1[:2] == s0[:2] and s1[2] != s0[2] and len(s1) == 3 and c.pages_free == 6
    assert [c.refcount(p) for p in s0] == [2, 2, 1] and c.refcount(s1[2]) == 1
    assert c.shared_upto(1) == 40 and c.shared_upto(0) == 0 and c.table[1].tolist() == s1 + [-1]
    for pool in c.kpool + c.vpool:
        assert torch.equal(pool[s1[2]].view(torch.uint8), pool[s0[2]].view(torch.uint8))
    # the shared pages survive the release of either slot
    c.release(0)
    assert [c.refcount(p) for p in s1] == [1, 1, 1] and c.pages_free == 7 and not set(s1) & set(c._free)
    c.fork(1, 2, 32)  # no partial page
    assert c.pages_of(2) == s1[:2] and c.pages_free == 7
    c.release(1)
    assert [c.refcount(p) for p in s1] == [1, 1, 0] and c.pages_free == 8 and not set(s1[:2]) & set(c._free)
    c.release(2)
    assert c.pages_free == 10 and sorted(c._free) == list(range(10)) and bool((c.table == -1).all())


# ---------------------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _inv_freq(hd, dev):
    return 1.0 / (500000.0 ** (torch.arange(0, hd, 2, device=dev).float() / hd))


def _positions(B, L, seed):
    """test_attn_batch.py's rule"""
    special = [p for p in (0, 63, 64, 511, 512, L - 1, 127, 128, 1023, 1024, 2047, 2048) if p < L]
    g = torch.Generator().manual_seed(seed)
    rnd = torch.randint(0, L, (B,), generator=g).tolist()
    return [special[b] if b < len(special) else rnd[b] for b in range(B)]


def _rand_cache(shape, dtype, dev, gen):
    return (torch.randn(shape, device=dev, generator=gen) * 0.5).to(dtype)


def _qkv(rows, nq, nkv, hd, dev, gen):
    """a padded row stride, as the q|k|v GEMV output has"""
    W = nq * hd + 2 * nkv * hd
    qkv = torch.randn(rows, W + 8, device=dev, generator=gen)
    return qkv[:, :nq * hd], qkv[:, nq * hd:nq * hd + nkv * hd], qkv[:, nq * hd + nkv * hd:W]


class Paged:
    """contiguous caches [B, nkv, L, hd] scattered into pools of about twice the pages through a seeded random permutation; the
    pools may be the middle pages of a buffer with one pattern page on either side (guard=True)"""

    def __init__(self, kc, vc, page_size, seed, guard=False):
        B, nkv, L, hd = kc.shape
        self.ps, self.mp, self.B = page_size, L // page_size, B
        need = B * self.mp
        self.num_pages = 2 * need + 1
        g = torch.Generator().manual_seed(seed)
        perm = torch.randperm(self.num_pages, generator=g)
        self.table = perm[:need].view(B, self.mp).to(torch.int32).to(kc.device)
        self.unowned = perm[need:].to(kc.device)
        self.bufs = []
        for c in (kc, vc):
            buf = torch.empty((self.num_pages + (2 if guard else 0), nkv, page_size, hd), dtype=torch.uint8 if c.dtype == F8 else F16,
                              device=c.device).view(c.dtype)
            _fill_nan(buf)
            pool = buf[1:self.num_pages + 1] if guard else buf
            _bits(pool)[self.table.long()] = _bits(c).view(B, nkv, self.mp, page_size, hd).transpose(1, 2)
            self.bufs.append(buf)
        self.kbuf, self.vbuf = self.bufs
        self.kpool, self.vpool = (b[1:self.num_pages + 1] if guard else b for b in self.bufs)

    def gather(self, pool):
        """the pool read through the table: bits [B, nkv, L, hd]"""
        g = _bits(pool)[self.table.long()]  # [B, mp, nkv, ps, hd]
        return g.transpose(1, 2).reshape(self.B, g.shape[2], self.mp * self.ps, g.shape[4])

    def launch_table(self, last_pos):
        """the table a launch gets: every entry past the page of a sequence's last position is garbage (all of an inactive one's)"""
        t = self.table.clone()
        for b, p in enumerate(last_pos):
            used = p // self.ps + 1 if 0 <= p < self.mp * self.ps else 0
            t[b, used:] = GARBAGE
        return t

    def unowned_intact(self):
        for pool in (self.kpool, self.vpool):
            b = _bits(pool)[self.unowned.long()]
            if not bool((b == (0x7E00 if pool.dtype == F16 else 0x7F)).all()):
                return False
        return True


DECODE = [(5, 32, 8, 128, 16, 64), (3, 8, 8, 64, 64, 4), (4, 16, 4, 256, 128, 16), (2, 8, 1, 128, 256, 2)]  # B nq nkv hd page_size max_pages


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "fp8"])
@pytest.mark.parametrize("B,nq,nkv,hd,ps,mp", DECODE)
def test_paged_decode_is_bitwise_the_contiguous_launch(dev, B, nq, nkv, hd, ps, mp, dtype):
    L = ps * mp
    want = _positions(B, L, seed=B * 131 + L) + [ps - 1, ps, L - 1]
    want += _positions(B, L, seed=7)[::-1][: (-len(want)) % B]  # the last group filled up
    inv_freq = _inv_freq(hd, dev)
    ws = qp.attention_workspace(B, nq, nkv, hd, L, dev)
    assert (ws is None) == (L < 512)
    gen = torch.Generator(device=dev).manual_seed(B + nq + L)
    kc0, vc0 = _rand_cache((B, nkv, L, hd), dtype, dev, gen), _rand_cache((B, nkv, L, hd), dtype, dev, gen)
    for gi in range(0, len(want), B):
        pos = want[gi:gi + B]
        pos_t = torch.tensor(pos, dtype=torch.long, device=dev)
        q, k, v = _qkv(B, nq, nkv, hd, dev, gen)
        kc, vc = kc0.clone(), vc0.clone()
        pg = Paged(kc, vc, ps, seed=gi + L)
        ref = qp.decode_attention(q, k, v, kc, vc, pos_t, inv_freq, ws=ws)
        tab = pg.launch_table(pos)
        out = qp.paged_decode_attention(q, k, v, pg.kpool, pg.vpool, tab, pos_t, inv_freq, ws=ws)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(ref)), pos
        assert not torch.equal(_bits(kc), _bits(kc0)), "the contiguous launch appended nothing"
        assert torch.equal(pg.gather(pg.kpool), _bits(kc)) and torch.equal(pg.gather(pg.vpool), _bits(vc)), pos
        assert pg.unowned_intact(), pos
        if ws is not None:
            assert int(ws.view(torch.int32)[: 128 * nkv].abs().max()) == 0, "tickets must be back at zero after a launch"
        # a second launch (the same bytes appended again): equal bits
        out2 = qp.paged_decode_attention(q, k, v, pg.kpool, pg.vpool, tab, pos_t, inv_freq, ws=ws)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out2), _bits(out)) and torch.equal(pg.gather(pg.kpool), _bits(kc))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "fp8"])
@pytest.mark.parametrize("T", [1, 17, 128])
@pytest.mark.parametrize("L", [256, 1024])
@pytest.mark.parametrize("ps", [16, 64])
@pytest.mark.parametrize("nq,nkv,hd", [(32, 8, 128), (8, 8, 64)])
def test_paged_prefill_is_bitwise_the_contiguous_launch(dev, nq, nkv, hd, ps, L, T, dtype):
    inv_freq = _inv_freq(hd, dev)
    ws = qp.prefill_workspace(T, nq, nkv, hd, L, dev)
    gen = torch.Generator(device=dev).manual_seed(T + nq + L + ps)
    kc0, vc0 = _rand_cache((1, nkv, L, hd), dtype, dev, gen), _rand_cache((1, nkv, L, hd), dtype, dev, gen)
    q, k, v = _qkv(T, nq, nkv, hd, dev, gen)
    for pos0 in sorted({0, ps - 1, L - T} | ({300} if 300 + T <= L else set())):
        pos_t = torch.tensor([pos0], dtype=torch.long, device=dev)
        kc, vc = kc0.clone(), vc0.clone()
        pg = Paged(kc, vc, ps, seed=pos0 + T)
        ref = qp.prefill_attention(q, k, v, kc[0], vc[0], pos_t, inv_freq, ws=ws)
        row = pg.launch_table([pos0 + T - 1])[0]
        out = qp.paged_prefill_attention(q, k, v, pg.kpool, pg.vpool, row, pos_t, inv_freq, ws=ws)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(ref)), pos0
        assert not torch.equal(_bits(kc), _bits(kc0))
        assert torch.equal(pg.gather(pg.kpool), _bits(kc)) and torch.equal(pg.gather(pg.vpool), _bits(vc)), pos0
        assert pg.unowned_intact(), pos0
        if ws is not None:
            assert int(ws.view(torch.int32)[: 8 * nkv].abs().max()) == 0, "tickets must be back at zero after a launch"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "fp8"])
@pytest.mark.parametrize("nq,nkv,hd,ps,L,T,pos0", [(32, 8, 128, 16, 1024, 17, 15), (8, 8, 64, 64, 256, 17, 63), (32, 8, 128, 64, 1024, 40, 500)])
def test_one_paged_prefill_launch_fills_the_pools_as_token_by_token_paged_decode(dev, nq, nkv, hd, ps, L, T, pos0, dtype):
    inv_freq = _inv_freq(hd, dev)
    gen = torch.Generator(device=dev).manual_seed(T + L)
    kc, vc = _rand_cache((1, nkv, L, hd), dtype, dev, gen), _rand_cache((1, nkv, L, hd), dtype, dev, gen)
    q, k, v = _qkv(T, nq, nkv, hd, dev, gen)
    pa, pb = Paged(kc, vc, ps, seed=1), Paged(kc, vc, ps, seed=1)
    pos_t = torch.tensor([pos0], dtype=torch.long, device=dev)
    qp.paged_prefill_attention(q, k, v, pa.kpool, pa.vpool, pa.table[0], pos_t, inv_freq, ws=qp.prefill_workspace(T, nq, nkv, hd, L, dev))
    ws1 = qp.attention_workspace(1, nq, nkv, hd, L, dev)
    p1 = pos_t.clone()
    for t in range(T):
        qp.paged_decode_attention(q[t:t + 1], k[t:t + 1], v[t:t + 1], pb.kpool, pb.vpool, pb.table, p1, inv_freq, ws=ws1)
        p1 += 1
    torch.cuda.synchronize()
    assert not torch.equal(pa.gather(pa.kpool), _bits(kc))
    assert torch.equal(_bits(pa.kpool), _bits(pb.kpool)) and torch.equal(_bits(pa.vpool), _bits(pb.vpool))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "fp8"])
def test_inactive_sequences_and_a_prefill_that_does_not_fit_touch_nothing(dev, dtype):
    nq, nkv, hd, ps, mp, B = 32, 8, 128, 16, 64, 4
    L = ps * mp
    inv_freq = _inv_freq(hd, dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    kc, vc = _rand_cache((B, nkv, L, hd), dtype, dev, gen), _rand_cache((B, nkv, L, hd), dtype, dev, gen)
    pg = Paged(kc, vc, ps, seed=2)
    k0, v0 = pg.kpool.clone(), pg.vpool.clone()
    pos = [-1, L, 1 << 40, -(1 << 40)]
    q, k, v = _qkv(B, nq, nkv, hd, dev, gen)
    out = torch.full((B, nq * hd), 3.0, dtype=F16, device=dev)
    ws = qp.attention_workspace(B, nq, nkv, hd, L, dev)
    qp.paged_decode_attention(q, k, v, pg.kpool, pg.vpool, pg.launch_table(pos), torch.tensor(pos, device=dev), inv_freq, out=out, ws=ws)
    T = 17
    q, k, v = _qkv(T, nq, nkv, hd, dev, gen)
    outp = torch.full((T, nq * hd), 3.0, dtype=F16, device=dev)
    wsp = qp.prefill_workspace(T, nq, nkv, hd, L, dev)
    for pos0 in (-1, L - T + 1, 1 << 40):
        qp.paged_prefill_attention(q, k, v, pg.kpool, pg.vpool, pg.launch_table([-1])[0], torch.tensor([pos0], device=dev), inv_freq,
                                   out=outp, ws=wsp)
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((outp == 3.0).all())
    assert int(ws.view(torch.int32).abs().max()) == 0
    assert torch.equal(_bits(pg.kpool), _bits(k0)) and torch.equal(_bits(pg.vpool), _bits(v0))
    assert int(wsp.view(torch.int32).abs().max()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "fp8"])
def test_guard_on_entries_outside_the_pool(dev, dtype):
    """the pools are the middle num_pages pages of buffers with one pattern page on either side: an entry of -1 and an entry of
    num_pages at the page of a sequence's NEW row (both would address a guard page if they were followed) change no byte of the
    guard pages, of the unowned pages or of that sequence's pages, and the other sequences come out bit for bit as with a valid table"""
    nq, nkv, hd, ps, mp, B = 32, 8, 128, 16, 64, 4
    L = ps * mp
    inv_freq = _inv_freq(hd, dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    kc, vc = _rand_cache((B, nkv, L, hd), dtype, dev, gen), _rand_cache((B, nkv, L, hd), dtype, dev, gen)
    pos = [700, 37, 600, 16]
    pos_t = torch.tensor(pos, dtype=torch.long, device=dev)
    q, k, v = _qkv(B, nq, nkv, hd, dev, gen)
    ws = qp.attention_workspace(B, nq, nkv, hd, L, dev)
    good, bad = Paged(kc, vc, ps, seed=9, guard=True), Paged(kc, vc, ps, seed=9, guard=True)
    assert good.kpool.data_ptr() == good.kbuf.data_ptr() + nkv * ps * hd * kc.element_size() and good.kpool.is_contiguous()
    before = (bad.kpool.clone(), bad.vpool.clone())
    out_good = qp.paged_decode_attention(q, k, v, good.kpool, good.vpool, good.launch_table(pos), pos_t, inv_freq, ws=ws)
    tab = bad.launch_table(pos)
    tab[1, pos[1] // ps] = -1
    tab[2, pos[2] // ps] = bad.num_pages
    out_bad = qp.paged_decode_attention(q, k, v, bad.kpool, bad.vpool, tab, pos_t, inv_freq, ws=ws)
    # a prefill whose new rows all lie behind bad entries: nothing is stored
    T = 17
    qt, kt, vt = _qkv(T, nq, nkv, hd, dev, gen)
    row = bad.table[1].clone()
    row[37 // ps:] = -1
    row[(37 + T - 1) // ps] = bad.num_pages
    after_decode = (bad.kpool.clone(), bad.vpool.clone())
    qp.paged_prefill_attention(qt, kt, vt, bad.kpool, bad.vpool, row, torch.tensor([37], device=dev), inv_freq,
                               ws=qp.prefill_workspace(T, nq, nkv, hd, L, dev))
    torch.cuda.synchronize()
    nan = 0x7E00 if dtype == F16 else 0x7F
    for p in (bad, good):
        for buf in (p.kbuf, p.vbuf):
            assert bool((_bits(buf[0]) == nan).all()) and bool((_bits(buf[-1]) == nan).all()), "a guard page was written"
        assert p.unowned_intact()
    for got, mid, old, ref in zip((bad.kpool, bad.vpool), after_decode, before, (good.kpool, good.vpool)):
        assert torch.equal(_bits(got), _bits(mid)), "the guarded prefill stored a row"
        for b in (0, 3):  # valid sequences: the pages they own, bit for bit the valid launch's
            assert torch.equal(_bits(got)[bad.table[b].long()], _bits(ref)[good.table[b].long()])
        for b in (1, 2):  # guarded sequences: their stores were dropped
            assert torch.equal(_bits(got)[bad.table[b].long()], _bits(old)[bad.table[b].long()])
    assert torch.equal(_bits(out_bad[[0, 3]]), _bits(out_good[[0, 3]]))
    assert int(ws.view(torch.int32)[: 128 * nkv].abs().max()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "fp8"])
def test_shared_prefix_fork(dev, dtype):
    """a prompt of 100 tokens prefilled once and forked at 100 (page_size 16: six shared pages, one copied partial page), then 40
    decode steps of both slots with different tokens: every step bitwise that of two unshared slots prefilled separately, the
    shared pages byte-identical before and after"""
    nq, nkv, hd, ps, mp, N, steps = 32, 8, 128, 16, 32, 100, 40
    L = ps * mp
    inv_freq = _inv_freq(hd, dev)
    gen = torch.Generator(device=dev).manual_seed(17)
    shared = qp.PagedKVCache(1, 24, nkv, ps, hd, 2, mp, dtype=dtype, device=dev)
    plain = qp.PagedKVCache(1, 24, nkv, ps, hd, 2, mp, dtype=dtype, device=dev)
    q, k, v = _qkv(N, nq, nkv, hd, dev, gen)
    wsp, ws = qp.prefill_workspace(N, nq, nkv, hd, L, dev), qp.attention_workspace(2, nq, nkv, hd, L, dev)
    zero = torch.zeros(1, dtype=torch.long, device=dev)
    shared.reserve(0, N + steps)
    qp.paged_prefill_attention(q, k, v, shared.kpool[0], shared.vpool[0], shared.table[0], zero, inv_freq, ws=wsp)
    shared.fork(0, 1, N)
    shared.reserve(1, N + steps)
    assert shared.pages_of(1)[:6] == shared.pages_of(0)[:6] and shared.pages_of(1)[6] != shared.pages_of(0)[6]
    assert shared.shared_upto(1) == N and all(shared.refcount(p) == 2 for p in shared.pages_of(0)[:6])
    for slot in (1, 0):
        plain.reserve(slot, N + steps)
        qp.paged_prefill_attention(q, k, v, plain.kpool[0], plain.vpool[0], plain.table[slot], zero, inv_freq, ws=wsp)
    assert not set(plain.pages_of(0)) & set(plain.pages_of(1))
    six = torch.tensor(shared.pages_of(0)[:6], device=dev)
    k6, v6 = shared.kpool[0][six].clone(), shared.vpool[0][six].clone()
    pos = torch.full((2,), N, dtype=torch.long, device=dev)
    for _ in range(steps):
        qs, ks, vs = _qkv(2, nq, nkv, hd, dev, gen)
        a = qp.paged_decode_attention(qs, ks, vs, shared.kpool[0], shared.vpool[0], shared.table, pos, inv_freq, ws=ws)
        b = qp.paged_decode_attention(qs, ks, vs, plain.kpool[0], plain.vpool[0], plain.table, pos, inv_freq, ws=ws)
        assert torch.equal(_bits(a), _bits(b))
        pos += 1
    torch.cuda.synchronize()
    assert torch.equal(_bits(shared.kpool[0][six]), _bits(k6)) and torch.equal(_bits(shared.vpool[0][six]), _bits(v6))
    assert not torch.equal(_bits(a[0]), _bits(a[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "fp8"])
def test_paged_graph_replay_across_a_page_boundary_and_the_split_threshold(dev, dtype):
    """one captured paged launch, pos advanced on the device by an add inside the graph (one stream, no parallel branches), replayed
    from page_size - 2 to page_size + 2 (sequence 0) and from 510 to 514 (sequence 1): each replay equals the captured contiguous
    launch's bit for bit"""
    B, nq, nkv, hd, ps, mp = 2, 32, 8, 128, 64, 16
    L = ps * mp
    inv_freq = _inv_freq(hd, dev)
    gen = torch.Generator(device=dev).manual_seed(23)
    kc, vc = _rand_cache((B, nkv, L, hd), dtype, dev, gen), _rand_cache((B, nkv, L, hd), dtype, dev, gen)
    pg = Paged(kc, vc, ps, seed=4)
    q, k, v = _qkv(B, nq, nkv, hd, dev, gen)
    ws = qp.attention_workspace(B, nq, nkv, hd, L, dev)
    start = torch.tensor([ps - 2, 510], dtype=torch.long, device=dev)
    one = torch.ones(B, dtype=torch.long, device=dev)
    outs = {}
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        for name in ("contiguous", "paged"):
            pos_t = start.clone()
            out = torch.zeros(B, nq * hd, dtype=F16, device=dev)

            def launch():
                if name == "paged":
                    qp.paged_decode_attention(q, k, v, pg.kpool, pg.vpool, pg.table, pos_t, inv_freq, out=out, ws=ws)
                else:
                    qp.decode_attention(q, k, v, kc, vc, pos_t, inv_freq, out=out, ws=ws)
                pos_t.add_(one)

            launch()  # warm-up (the row it appends is appended again by the first replay)
            pos_t.copy_(start)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                launch()
            got = []
            for _ in range(5):
                g.replay()
                got.append(out.clone())
            torch.cuda.synchronize()
            assert pos_t.tolist() == [ps + 3, 515]
            outs[name] = got
    for i, (a, b) in enumerate(zip(outs["contiguous"], outs["paged"])):
        assert torch.equal(_bits(a), _bits(b)), i
    assert not torch.equal(_bits(outs["paged"][0]), _bits(outs["paged"][1]))
    assert torch.equal(pg.gather(pg.kpool), _bits(kc)) and torch.equal(pg.gather(pg.vpool), _bits(vc)) and pg.unowned_intact()
    assert int(ws.view(torch.int32)[: 128 * nkv].abs().max()) == 0


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
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "fp8"])
def test_whole_model_paged_against_contiguous(dev, model, dtype):
    """two layers of 3_8b, vocab 4096, context 512, page_size 64: Prefill of 5 / 129 / 300 tokens into slots 0 / 1 / 2, eight
    DecodeStep steps at B = 3 and Score over the 300 tokens, paged against contiguous caches: the same next tokens, hidden() and the
    log-probs within the whole-model tests' bound 2^-7 max(1, |ref|).  The attention launches are bitwise equal and every other
    launch is the same launch on the same bits; whether the end results are bitwise equal too is printed, not asserted (it rests
    on the linears being reproducible run to run at these batches, which nothing here has established)."""
    m, B, L, ps = model, 3, 512, 64
    nkv, hd, nl = m.cfg.num_key_value_heads, m.cfg.head_dim, len(m.layers)
    kc = [torch.zeros(B, nkv, L, hd, dtype=torch.uint8 if dtype == F8 else F16, device=dev).view(dtype) for _ in range(nl)]
    vc = [t.clone() for t in kc]
    cache = qp.PagedKVCache(nl, 2 * B * (L // ps), nkv, ps, hd, B, L // ps, dtype=dtype, device=dev)
    assert cache.max_len == L
    lens = [5, 129, 300]
    for n in range(ps, max(lens) + 8 + ps, ps):  # page by page, slot after slot: no slot's pages are consecutive
        for slot, N in enumerate(lens):
            cache.reserve(slot, min(n, N + 8))
    assert cache.pages_of(2)[1] != cache.pages_of(2)[0] + 1
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(0, 4096, (N,), generator=g).to(dev) for N in lens]
    pf_c = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, chunk=128)
    pf_p = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, cache.kpool, cache.vpool, m.inv_freq, chunk=128, block_table=cache.table)
    assert pf_p.context == L == pf_c.context
    with pytest.raises(qp._native.QpalError):
        pf_p(prompts[2], slot=0, pos0=L - 299)
    with pytest.raises(qp._native.QpalError):
        pf_p(prompts[0], slot=3, pos0=0)
    tok = torch.zeros(B, dtype=torch.long, device=dev)
    for slot, toks in enumerate(prompts):
        a, b = pf_c(toks, slot=slot, pos0=0).clone(), pf_p(toks, slot=slot, pos0=0).clone()
        ok, err, top = _close(pf_p.hidden(), pf_c.hidden())
        print(f"prefill {len(toks)}: tokens {int(a)} / {int(b)}, hidden max |diff| {err:.3e} (max |ref| {top:.3f})")
        assert ok and int(a) == int(b)
        print("  bitwise equal:", torch.equal(pf_p.hidden(), pf_c.hidden()))
        tok[slot] = a[0]
    pos = torch.tensor(lens, dtype=torch.long, device=dev)
    tok_p, pos_p = tok.clone(), pos.clone()
    out_c, out_p = torch.zeros_like(tok), torch.zeros_like(tok)
    st_c = qp.DecodeStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, tok, pos, out_c)
    st_p = qp.DecodeStep(m.layers, m.embed, m.norm, m.lm_head, cache.kpool, cache.vpool, m.inv_freq, tok_p, pos_p, out_p,
                         block_table=cache.table)
    assert st_p.context == L and st_p.launches_per_token == st_c.launches_per_token
    for i in range(8):
        st_c()
        st_p()
        ok, err, top = _close(st_p.hidden(), st_c.hidden())
        print(f"step {i}: tokens {out_c.tolist()} / {out_p.tolist()}, hidden max |diff| {err:.3e} (max |ref| {top:.3f})")
        assert ok and out_c.tolist() == out_p.tolist()
        print("  bitwise equal:", torch.equal(st_p.hidden(), st_c.hidden()))
        for t, o, p in ((tok, out_c, pos), (tok_p, out_p, pos_p)):
            t.copy_(o)
            p += 1
    sc_c = qp.Score(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, chunk=128)
    sc_p = qp.Score(m.layers, m.embed, m.norm, m.lm_head, cache.kpool, cache.vpool, m.inv_freq, chunk=128, block_table=cache.table)
    lp_c, lp_p = sc_c(prompts[2], slot=2, pos0=0).clone(), sc_p(prompts[2], slot=2, pos0=0).clone()
    ok, err, top = _close(lp_p, lp_c)
    print(f"score: log-prob max |diff| {err:.3e} (max |ref| {top:.3f})")
    assert ok and lp_p.shape == (299,)
    print("  bitwise equal:", torch.equal(lp_p, lp_c), torch.equal(sc_p.rank, sc_c.rank))
    # a paged batch of one takes the batched attention launch and keeps the batch-1 GEMV fusions
    one = qp.PagedKVCache(nl, 8, nkv, ps, hd, 1, L // ps, dtype=dtype, device=dev)
    one.reserve(0, 1)
    t1, p1, o1 = torch.zeros(1, dtype=torch.long, device=dev), torch.zeros(1, dtype=torch.long, device=dev), torch.zeros(1, dtype=torch.long, device=dev)
    s1 = qp.DecodeStep(m.layers, m.embed, m.norm, m.lm_head, one.kpool, one.vpool, m.inv_freq, t1, p1, o1, block_table=one.table)
    assert s1.batch1 and s1.attn_batch
    s1()
    torch.cuda.synchronize()
    assert 0 <= int(o1[0]) < 4096 and bool(torch.isfinite(s1.hidden()).all())
