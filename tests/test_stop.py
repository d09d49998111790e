"""Stop conditions on the GPU (csrc/stop.hip, qpalette_amd.stop): qpal_stop_advance in both modes and qpal_stop_mask bit
for bit the numpy contracts (tests/test_stop_contract.py holds those to brute force and to hand-made cases) on random banks, a second
launch on the result of the first, tokens longer than what the wave stages, and the error codes and wrapper checks."""
import ctypes

import numpy as np
import pytest
import torch

import qpalette_amd as qp
from qpalette_amd import stop as sp
from qpalette_amd.grammar import TokenTable

VOCAB, MAX_LEN = 300, 64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _vocabulary():
    """300 tokens of 0 .. 9 bytes over "abc" (matches are common), with a few bytes from anywhere; eos is the last id"""
    rng = np.random.default_rng(300)
    toks = []
    for t in range(VOCAB):
        raw = bytearray(b"abc"[v] for v in rng.integers(0, 3, size=int(rng.integers(0, 10))))
        if raw and rng.random() < 0.1:
            raw[int(rng.integers(0, len(raw)))] = int(rng.integers(0, 256))
        toks.append(bytes(raw))
    toks[VOCAB - 1] = b"<eos>"
    return TokenTable(toks, eos=VOCAB - 1)


TABLE = _vocabulary()


def _sets():
    """set 0: one 1-byte string; set 1: 64 strings of 4 .. 7 bytes over "abc" (nested and overlapping by construction)"""
    rng = np.random.default_rng(64)
    many = set()
    while len(many) < 64:
        many.add(bytes(b"abc"[v] for v in rng.integers(0, 3, size=int(rng.integers(4, 8)))))
    return [sp.compile_stops([b"\x07"]), sp.compile_stops(sorted(many))]


SETS = _sets()


def _bank(dev, B, cap=6, **kw):
    bank = qp.StopBank(B, TABLE, dev, sets=3, max_states=max(s.trans.shape[0] for s in SETS) + 3, cap=cap, **kw)
    for i, ss in enumerate(SETS):
        bank.load(i, ss)
    return bank


def _random_state(rng, B, cap=6, id_slots=16):
    st = sp.StopState(B, cap=cap, id_slots=id_slots)
    st.set_id[:] = rng.choice([-1, 0, 1, 1, 1, 2, 7], size=B)          # 2: a set that is not loaded; 7: outside the bank
    S = np.array([SETS[g].trans.shape[0] if 0 <= g < 2 else 1 for g in st.set_id])
    st.ac_state[:] = rng.integers(0, S)
    st.ac_state[rng.random(B) < 0.1] = rng.choice([-3, 60000])          # read as the start
    st.stop_ids[:] = rng.integers(0, 12, size=st.stop_ids.shape)        # the tokens below are drawn from 0 .. 39: hits are common
    st.stop_ids[rng.random(st.stop_ids.shape) < 0.1] = -1
    st.n_ids[:] = rng.choice([0, 1, 2, id_slots, id_slots + 3, -1], size=B)
    st.n_gen[:] = rng.integers(0, 9, size=B)
    st.max_tokens[:] = rng.choice([0, 0, 3, 6, 9], size=B)
    st.min_tokens[:] = rng.choice([0, 0, 2, 5, 8], size=B)
    st.gen_bytes[:] = rng.integers(0, 1 << 40, size=B)
    st.out[:] = rng.integers(0, VOCAB, size=st.out.shape)
    for name in ("reason", "hit"):                                      # what a launch must leave alone shows
        getattr(st, name)[:] = rng.integers(0, 5, size=B)
    for name in ("text_len", "end_pos"):
        getattr(st, name)[:] = rng.integers(0, 99, size=B)
    return st


def _tokens(rng, shape):
    t = rng.integers(0, 40, size=shape).astype(np.int64)
    t[rng.random(shape) < 0.05] = rng.choice([-1, VOCAB, VOCAB + 5, 1 << 40])   # foreign ids: no bytes
    t[rng.random(shape) < 0.05] = VOCAB - 1
    return t


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same(bank, ref, what):
    got = bank.state()
    bad = ref.equal(got)
    assert not bad, (what, bad, {n: (getattr(got, n)[:8], getattr(ref, n)[:8]) for n in bad})


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, 128])
def test_advance_decode_mode_is_the_reference(dev, B):
    """every criterion on random slots, inactive slots (pos outside the cache), slots at the last position, and a second launch on
    the result of the first: the contract applied twice"""
    rng = np.random.default_rng(B)
    bank = _bank(dev, B)
    sets = list(SETS) + [None]
    seen = set()
    for rep in range(4):
        st = _random_state(rng, B)
        bank.put(st)
        tok = rng.integers(0, VOCAB, size=B).astype(np.int64)
        pos = rng.choice([-1, 0, 5, MAX_LEN - 2, MAX_LEN - 1, MAX_LEN, 1 << 35], size=B, p=[.1, .3, .3, .1, .1, .05, .05]).astype(np.int64)
        d_tok, d_pos = _t(tok, dev), _t(pos, dev)
        for launch in range(2):
            new = _tokens(rng, B)
            was = pos
            st, tok, pos = sp.reference_stop_advance(sets, TABLE, st, new, MAX_LEN, tok=tok, pos=pos)
            seen |= set(st.reason[(was >= 0) & (was < MAX_LEN) & (pos < 0)].tolist())
            sp.stop_advance(bank, _t(new, dev), MAX_LEN, tok=d_tok, pos=d_pos)
            _same(bank, st, (rep, launch))
            assert np.array_equal(d_tok.cpu().numpy(), tok) and np.array_equal(d_pos.cpu().numpy(), pos), (rep, launch)
    assert seen == {1, 2, 3, 4} or B < 128, f"at B = 128 every reason occurs, got {seen}"


@pytest.mark.gpu
@pytest.mark.parametrize("B,width", [(1, 1), (3, 5), (128, 16), (3, 16), (128, 5)])
def test_advance_speculative_mode_is_the_reference(dev, B, width):
    """the in-place n_out / n_tok / limit, n_out == 0, n_out outside 0 .. width, and a second launch on the result of the first"""
    rng = np.random.default_rng(100 * B + width)
    bank = _bank(dev, B)
    sets = list(SETS) + [None]
    cuts = 0
    for rep in range(4):
        st = _random_state(rng, B)
        bank.put(st)
        n_tok = rng.integers(20, MAX_LEN + 4, size=B).astype(np.int64)
        limit = n_tok + rng.integers(0, 9, size=B)
        d_tok, d_lim = _t(n_tok, dev), _t(limit, dev)
        for launch in range(2):
            new = _tokens(rng, (B, width))
            n_out = rng.integers(0, width + 1, size=B).astype(np.int32)
            n_out[rng.random(B) < 0.05] = rng.choice([-2, width + 3])
            d_out = _t(n_out, dev)
            st, r_out, n_tok, limit = sp.reference_stop_advance(sets, TABLE, st, new, MAX_LEN, n_out=n_out, n_tok=n_tok, limit=limit)
            sp.stop_advance(bank, _t(new, dev), MAX_LEN, n_out=d_out, n_tok=d_tok, limit=d_lim)
            _same(bank, st, (rep, launch))
            assert np.array_equal(d_out.cpu().numpy(), r_out), (rep, launch)
            assert np.array_equal(d_tok.cpu().numpy(), n_tok) and np.array_equal(d_lim.cpu().numpy(), limit), (rep, launch)
            cuts += int(((r_out != n_out) & (n_out <= width)).sum())
    assert cuts > 0 or B * width < 15, "a run is cut before its end somewhere"


@pytest.mark.gpu
def test_advance_walks_tokens_longer_than_the_stage(dev):
    """a token of 200 bytes: the bytes behind the first 64 are read where they lie; the match sits at byte 150 of the token and, in
    the second slot, across the boundary between a long token and a short one"""
    long_a = b"x" * 149 + b"Q" + b"y" * 50
    long_b = b"z" * 199 + b"h"
    table = TokenTable([long_a, long_b, b"alt", b"<eos>"], eos=3)
    ss = sp.compile_stops([b"xQ", b"zhalt"])
    bank = qp.StopBank(2, table, dev, sets=1, max_states=16, cap=4)
    bank.load(0, ss)
    for b in range(2):
        bank.set(b, stop=0)
    st = bank.state()
    n_tok, limit = torch.tensor([12, 12], device=dev), torch.tensor([40, 40], device=dev)
    n_out = torch.tensor([2, 2], dtype=torch.int32, device=dev)
    toks = np.array([[0, 2], [1, 2]], np.int64)
    ref, r_out, r_tok, r_lim = sp.reference_stop_advance([ss], table, st, toks, 64, n_out=[2, 2], n_tok=[12, 12], limit=[40, 40])
    assert ref.reason.tolist() == [2, 2] and ref.text_len.tolist() == [148, 198] and r_out.tolist() == [1, 2]
    sp.stop_advance(bank, _t(toks, dev), 64, n_out=n_out, n_tok=n_tok, limit=limit)
    _same(bank, ref, "long tokens")
    assert n_out.tolist() == [1, 2] and n_tok.tolist() == r_tok.tolist() and limit.tolist() == r_lim.tolist()
    res = bank.result(1)
    assert res["reason"] == "stop_string" and res["stop"] == b"zhalt" and res["text"] == b"z" * 198 and res["tokens"] == [1, 2]
    assert bank.result(0)["stop"] == b"xQ" and bank.result(0)["text"] == b"x" * 148


@pytest.mark.gpu
@pytest.mark.parametrize("rows,spec", [(1, False), (3, False), (128, False), (5, True), (128, True)])
def test_mask_is_the_reference(dev, rows, spec):
    rng = np.random.default_rng(rows + spec)
    B = rows if not spec else max(1, rows // 3)
    bank = _bank(dev, B)
    st = _random_state(rng, B)
    st.stop_ids[rng.random(st.stop_ids.shape) < 0.1] = VOCAB + 2     # no token: skipped
    bank.put(st)
    logits = rng.standard_normal((rows, VOCAB + 4)).astype(np.float32)
    ctr = rng.integers(0, 50, size=rows).astype(np.int64)
    ctr[rng.random(rows) < 0.2] = -1
    if spec:
        lens = rng.multinomial(rows - B, np.ones(B) / B) + 1 if rows >= B else np.ones(B, int)
        lens[rng.random(B) < 0.2] = 0
        row0 = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        row_slot = np.full(rows, -1, np.int32)
        for b in range(B):
            row_slot[row0[b]:min(row0[b + 1], rows)] = b
        row0 = np.minimum(row0, rows).astype(np.int32)
        if B > 1:
            row0[1] = -1 if rng.random() < 0.5 else row0[1]           # a segment that is none
    else:
        row0, row_slot = None, np.arange(rows, dtype=np.int32)
        row_slot[rng.random(rows) < 0.1] = rng.choice([-1, B])
    ref = sp.reference_stop_mask(logits, st, row_slot, ctr, row0=row0, vocab=VOCAB)
    d = _t(logits, dev)
    out = sp.stop_mask(d, bank, _t(row_slot, dev), _t(ctr, dev), row0=None if row0 is None else _t(row0, dev))
    assert out is d and np.array_equal(d.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    assert np.isinf(ref).any() and not np.isinf(ref[:, VOCAB:]).any() or rows < 100
    before = bank.state()
    sp.stop_mask(d, bank, _t(row_slot, dev), _t(ctr, dev), row0=None if row0 is None else _t(row0, dev))
    assert np.array_equal(d.cpu().numpy().view(np.uint32), ref.view(np.uint32)) and not before.equal(bank.state())


@pytest.mark.gpu
def test_error_codes_and_wrapper_checks(dev):
    lib, QpalError = qp._native.lib(), qp._native.QpalError
    bank = _bank(dev, 3)
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64, device=dev)   # noqa: E731
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)   # noqa: E731
    tokens, tok, pos, n_out = i64(3, 4), i64(3), i64(3), i32(3)
    voc = [bank.tok_off.data_ptr(), bank.tok_bytes.data_ptr(), VOCAB, TABLE.total]

    def adv(struct=None, voc=voc, slots=3, tokens=tokens.data_ptr(), width=1, n_out=None, n_tok=None, limit=None, tok=tok.data_ptr(),
            pos=pos.data_ptr(), max_len=64):
        return lib.qpal_stop_advance(struct or bank.struct(), *voc, slots, tokens, width, n_out, n_tok, limit, tok, pos, max_len, None)

    assert adv() == 0
    assert adv(width=4, n_out=n_out.data_ptr(), n_tok=tok.data_ptr(), limit=pos.data_ptr(), tok=None, pos=None) == 0
    assert adv(tok=None) == -3 and adv(pos=None) == -3 and adv(tokens=None) == -3
    assert adv(width=4, n_out=n_out.data_ptr(), n_tok=None, limit=pos.data_ptr()) == -3
    assert lib.qpal_stop_advance(None, *voc, 3, tokens.data_ptr(), 1, None, None, None, tok.data_ptr(), pos.data_ptr(), 64, None) == -3
    assert adv(slots=0) == -1 and adv(slots=129) == -1 and adv(max_len=0) == -1 and adv(width=0) == -1
    assert adv(width=17, n_out=n_out.data_ptr(), n_tok=tok.data_ptr(), limit=pos.data_ptr()) == -1
    assert adv(width=2) == -2                                             # decode mode judges one token
    assert adv(tokens=tokens.data_ptr() + 4) == -4 and adv(pos=pos.data_ptr() + 4) == -4
    for name, bad, code in (("sets", 257, -1), ("max_states", 65536, -1), ("id_slots", 17, -1), ("cap", 0, -1), ("hit", None, -3),
                            ("gen_bytes", bank.gen_bytes.data_ptr() + 4, -4), ("out_len", bank.out_len.data_ptr() + 1, -4)):
        s = qp._native.StopBankStruct()
        ctypes.memmove(ctypes.byref(s), ctypes.byref(bank.struct()), ctypes.sizeof(s))
        setattr(s, name, bad)
        assert adv(struct=s) == code, name
    logits, row_slot, ctr = torch.zeros(3, VOCAB, device=dev), i32(3), i64(3)

    def mask(logits=logits.data_ptr(), ld=VOCAB, rows=3, vocab=VOCAB, row_slot=row_slot.data_ptr(), ctr=ctr.data_ptr(), row0=None,
             ids=bank.stop_ids.data_ptr(), id_slots=16, slots=3):
        return lib.qpal_stop_mask(logits, ld, rows, vocab, row_slot, ctr, row0, ids, id_slots, bank.n_ids.data_ptr(),
                                  bank.min_tokens.data_ptr(), bank.n_gen.data_ptr(), slots, None)

    assert mask() == 0
    assert mask(logits=None) == -3 and mask(ctr=None) == -3 and mask(ids=None) == -3
    assert mask(rows=0) == -1 and mask(rows=129) == -1 and mask(ld=VOCAB - 1) == -1 and mask(id_slots=17) == -1 and mask(slots=0) == -1
    assert mask(ctr=ctr.data_ptr() + 4) == -4 and mask(row0=row_slot.data_ptr() + 2) == -4
    torch.cuda.synchronize()
    # ---- the wrappers name the argument
    for kw, name in ((dict(tok=tok.int(), pos=pos), "tok"), (dict(tok=tok, pos=pos[:2]), "pos"), (dict(tok=tok.cpu(), pos=pos), "tok")):
        with pytest.raises(QpalError, match=name):
            sp.stop_advance(bank, tok, 64, **kw)
    with pytest.raises(QpalError, match="tokens"):
        sp.stop_advance(bank, tokens, 64, tok=tok, pos=pos)
    with pytest.raises(QpalError, match="n_out"):
        sp.stop_advance(bank, tokens, 64, n_out=n_out.long(), n_tok=tok, limit=pos)
    with pytest.raises(QpalError, match="decode mode"):
        sp.stop_advance(bank, tok, 64, tok=tok)
    with pytest.raises(QpalError, match="speculative mode"):
        sp.stop_advance(bank, tokens, 64, n_out=n_out, n_tok=tok, limit=pos, pos=pos)
    with pytest.raises(QpalError, match="max_len"):
        sp.stop_advance(bank, tok, 0, tok=tok, pos=pos)
    with pytest.raises(QpalError, match="StopBank"):
        sp.stop_advance(None, tok, 64, tok=tok, pos=pos)
    for args, name in (((logits.half(), bank, row_slot, ctr), "logits"), ((logits, bank, row_slot.long(), ctr), "row_slot"),
                       ((logits, bank, row_slot, ctr[:2]), "ctr"), ((logits[:, :VOCAB - 1], bank, row_slot, ctr), "logits")):
        with pytest.raises(QpalError, match=name):
            sp.stop_mask(*args)
    with pytest.raises(QpalError, match="row0"):
        sp.stop_mask(logits, bank, row_slot, ctr, row0=i32(3))
    # ---- the bank's own checks
    with pytest.raises(QpalError, match="min_tokens"):
        bank.set(0, max_tokens=3, min_tokens=4)
    with pytest.raises(QpalError, match="not loaded"):
        bank.set(0, stop=2)
    with pytest.raises(QpalError, match="stop_ids"):
        bank.set(0, stop_ids=[VOCAB])
    bank.set(1, stop=1)
    with pytest.raises(QpalError, match="in use by slot 1"):
        bank.unload(1)
    with pytest.raises(QpalError, match="max_states"):
        bank.load(2, [b"a" * 2000])
    with pytest.raises(QpalError, match="slot 3"):
        bank.reset(3)
    bank.set(1, stop=None, stop_ids=())
    bank.unload(1)
    assert bank.n_states.tolist()[1] == 0 and bank.n_ids.tolist()[1] == 0
