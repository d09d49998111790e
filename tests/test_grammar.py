"""Grammar-constrained decoding on the GPU (csrc/grammar.hip, qpalette_amd.grammar, the `grammar=` of the step classes).

Kernels: qpal_grammar_compile / rows / mask / advance bit for bit the numpy contracts (tests/test_grammar_contract.py holds those to
hand-made cases and to Python's `re`), two launches bitwise equal.  Whole model (tests/test_spec.py's model, prompts, generation loop
and near-tie rule, loaded from that file as tests/test_logit_process.py does): a bank without a grammar in any slot changes no bit of
DecodeStep, Prefill and SpeculativeStep; with two grammars and a free slot the emitted bytes are at every step a live prefix of the
pattern, a text that ended in eos matches it, the device state is the host walk of the emitted tokens, and SpeculativeStep emits
the stream of sequential Prefill + DecodeStep token for token; a captured DecodeStep follows its grammar over replays."""
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

import qpalette_amd as qp
from qpalette_amd import grammar as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- kernels

_TABLES = {}
SMALL = r"[ab]*(\.[01]+)?"   # 3 states; a token of a's and b's is allowed from the start


def _table(vocab):
    """a vocabulary of `vocab` tokens of 0 .. 40 bytes: a third are strings of a's and b's (what SMALL and [ab]{300} take from most
    states), the others strings over "ab01.-xyz" (mostly refused at some byte), 3 % empty; tokens 0 .. 3 are "a", "b", ".", "0", so
    that every state of the test automata has a token; eos is the last id that has bytes.  Once per vocabulary size."""
    if vocab not in _TABLES:
        rng = np.random.default_rng(vocab)
        good, wide = np.frombuffer(b"ab", np.uint8), np.frombuffer(b"ab01.-xyz", np.uint8)
        lens = np.minimum(40, rng.geometric(0.18, size=vocab))
        lens[rng.random(vocab) < 0.05] = 40
        kind = rng.random(vocab)
        lens[kind < 0.03] = 0
        off = np.concatenate([[0], np.cumsum(lens)])
        is_good = np.repeat(kind < 0.36, lens)
        data = np.where(is_good, good[rng.integers(0, 2, size=off[-1])], wide[rng.integers(0, 9, size=off[-1])]).astype(np.uint8).tobytes()
        toks = [data[off[t]:off[t + 1]] for t in range(vocab)]
        toks[:4] = [b"a", b"b", b".", b"0"]
        toks[vocab - 1] = b"<eos>"
        _TABLES[vocab] = G.TokenTable(toks, eos=vocab - 1)
    return _TABLES[vocab]


_DFAS = {}


def _dfa(pattern):
    if pattern not in _DFAS:
        _DFAS[pattern] = G.compile_regex(pattern)
    return _DFAS[pattern]


COMPILE_CASES = [(v, p) for v in (33, 63, 64, 65, 4099) for p in ("", SMALL, "[ab]{300}")] + [(128256, ""), (128256, SMALL)]


@pytest.mark.gpu
@pytest.mark.parametrize("vocab,pattern", COMPILE_CASES, ids=[f"{v}-{len(p)}" for v, p in COMPILE_CASES])
def test_compile_kernel_is_the_reference(dev, vocab, pattern):
    """vocab 33: one word and one bit; 63 / 64 / 65: the two words of a wave's ballot, full and not; 4099: 17 workgroups, the last
    with one wave of 3 tokens; 128 256 with S <= 8.  "": one state; [ab]{300}: a state index above 255.  Loaded twice: bitwise equal."""
    table, dfa = _table(vocab), _dfa(pattern)
    S = dfa.trans.shape[0]
    ref = G.reference_allow(dfa, table)
    bank = qp.GrammarBank(1, table, dev, grammars=2, max_states=S + 2)
    bank.allow.fill_(0x55555555)       # what the launch does not write shows
    assert bank.allow_bytes == 2 * (S + 3) * ((vocab + 31) // 32) * 4
    for g in range(2):
        bank.load(g, dfa)
    got = bank.allow.cpu().numpy().view(np.uint32)
    bad = np.argwhere(got[0, :S + 1] != ref)
    assert bad.shape[0] == 0, (bad[:5], [(hex(got[0, s, w]), hex(ref[s, w])) for s, w in bad[:5]])
    assert np.array_equal(got[1, :S + 1], got[0, :S + 1]), "two launches"
    assert np.all(got[:, S + 1:] == 0x55555555), "the rows behind the finished state are not written"
    assert bank.n_states.tolist() == [S, S]
    if pattern == SMALL and vocab >= 4099:
        share = float(np.mean([(int(ref[0, t >> 5]) >> (t & 31)) & 1 for t in range(vocab)]))
        assert 0.2 < share < 0.5, f"{share:.2f} of the tokens are allowed from the start: the case is meant to show about a third"
    if pattern == "[ab]{300}":
        assert ref[299].any() and not np.array_equal(ref[299], ref[299 - 256]), "a state index cut to 8 bits would show"


@pytest.mark.gpu
def test_load_refuses_an_automaton_the_vocabulary_cannot_follow(dev):
    table = G.TokenTable([b"a", b"b", b"<eos>"], eos=2)
    bank = qp.GrammarBank(2, table, dev, grammars=2, max_states=16)
    with pytest.raises(qp._native.QpalError, match="no token of the vocabulary continues the text from state 1"):
        bank.load(0, "ac")
    with pytest.raises(qp._native.QpalError, match="not loaded"):
        bank.set(0, 0)
    with pytest.raises(qp._native.QpalError, match="needs 18 states"):
        bank.load(0, "a{17}")
    with pytest.raises(qp._native.QpalError, match="position 1"):
        bank.load(0, "a$")
    bank.load(0, "a+b")
    bank.set(1, 0)
    with pytest.raises(qp._native.QpalError, match="in use by slot 1"):
        bank.unload(0)
    bank.set(1, None)
    bank.unload(0)
    assert bank.n_states.tolist() == [0, 0] and bank.gram.tolist() == [-1, -1]


def _three(dev, vocab, slots, patterns=("(a|b)*abb", SMALL, "")):
    """a bank of `slots` slots with grammars 0 .. 2 loaded (3: not loaded), and the host's copies"""
    table = _table(vocab)
    dfas = [_dfa(p) for p in patterns] + [None]
    bank = qp.GrammarBank(slots, table, dev, grammars=4, max_states=max(d.trans.shape[0] for d in dfas[:3]))
    for g, d in enumerate(dfas[:3]):
        bank.load(g, d)
    return table, dfas, bank


def _random_logits(rng, rows, vocab, ld):
    """N(0, 2.5^2) with a few -inf and NaN entries; columns vocab .. ld hold a sentinel"""
    l = np.full((rows, ld), -77.0, F32)
    l[:, :vocab] = rng.normal(0, 2.5, size=(rows, vocab))
    for r in range(rows):
        l[r, rng.integers(0, vocab, size=3)] = (-np.inf, np.nan, -np.inf)
    return l


CASES = [(1, 33), (5, 33), (128, 33), (1, 1000), (5, 1000), (128, 1000), (5, 4099), (128, 4099), (2, 128256)]


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True], ids=["ld=vocab", "ld>vocab"])
@pytest.mark.parametrize("rows,vocab", CASES)
def test_mask_kernel_is_the_reference(dev, rows, vocab, wide):
    """the row, ld and alignment cases of test_process_kernel_is_the_reference: vocab 33: one full word and one bit; 4099 with ld =
    vocab: rows that are not 16-byte aligned (single stores); ld > vocab (a multiple of 4): aligned rows, sentinel columns kept;
    128 256: 32 tiles per row.  Logits with NaN and -inf.  Skipped rows — ctr < 0, a slot outside the bank, gram = -1 or not
    loaded, a dead row state and one past the finished state — keep every bit.  In place, on two copies (bitwise equal), then
    again on the result (nothing left to change)."""
    rng = np.random.default_rng(1000 * rows + vocab + 7 * wide)
    ld = (vocab + 3) // 4 * 4 + 4 if wide else vocab
    slots = 1 if rows == 1 else 6
    table, dfas, bank = _three(dev, vocab, slots)
    gram = np.array([0] if slots == 1 else [0, 1, -1, 2, 1, 3], np.int32)
    bank.gram.copy_(torch.from_numpy(gram))
    l = _random_logits(rng, rows, vocab, ld)
    row_slot = rng.integers(0, slots, size=rows).astype(np.int32)
    ctr = rng.integers(0, 1 << 40, size=rows)
    row_state = np.zeros(rows, np.int32)
    for r in range(rows):
        d = dfas[gram[row_slot[r]]] if gram[row_slot[r]] >= 0 else None
        S = d.trans.shape[0] if d is not None else 3
        row_state[r] = rng.choice([rng.integers(0, S), S, -1, S + 1, -5], p=[0.6, 0.2, 0.1, 0.05, 0.05])
    if rows > 3:
        row_slot[1], ctr[3] = -1, -1
    if rows > 5:
        row_slot[4] = slots
    if rows == 1:
        row_state[0] = 1
    allows = [None if d is None else G.reference_allow(d, table) for d in dfas]
    ref = G.reference_mask(l, allows, gram, row_state, row_slot, ctr, vocab=vocab)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    args = (t(row_slot), t(ctr))
    outs = []
    for _ in range(2):
        lin = t(l)
        assert G.grammar_mask(lin, bank, *args, row_state=t(row_state)) is lin
        outs.append(lin.cpu().numpy())
    bad = np.argwhere(_bits(outs[0]) != _bits(ref))
    assert bad.shape[0] == 0, (bad[:5], [(outs[0][r, i], ref[r, i], l[r, i]) for r, i in bad[:5]])
    assert np.array_equal(_bits(outs[1]), _bits(outs[0])), "two launches"
    G.grammar_mask(lin, bank, *args, row_state=t(row_state))
    assert np.array_equal(_bits(lin.cpu().numpy()), _bits(ref)), "a second pass over the result"
    # the case shows what it is meant to show
    changed = (_bits(ref) != _bits(l)).any(axis=1)
    assert np.all(ref[:, vocab:] == -77.0) and changed.any()
    if rows > 5:
        assert (~changed).sum() >= 3 and np.isnan(ref[changed]).any()
    if rows == 128:
        g = gram[np.clip(row_slot, 0, slots - 1)]
        S = np.array([dfas[x].trans.shape[0] if x in (0, 1, 2) else 0 for x in g])
        live = (row_slot >= 0) & (row_slot < slots) & (ctr >= 0)
        for what, sel in (("no grammar", g == -1), ("not loaded", g == 3), ("dead", row_state == -1), ("past the end", row_state > S),
                          ("ctr", ctr < 0)):
            assert (sel & ~changed).any() and not (sel & changed).any(), what
        assert (live & (row_state == S) & changed & (g >= 0) & (g < 3)).any(), "a finished row"


@pytest.mark.gpu
def test_mask_kernel_on_the_bank_state_and_a_bank_without_grammars(dev):
    """row_state defaults to bank.state (a decode step: row = slot); a new bank writes nothing"""
    vocab, B = 4099, 6
    table, dfas, bank = _three(dev, vocab, B)
    rng = np.random.default_rng(9)
    l = _random_logits(rng, B, vocab, vocab)
    lin = torch.from_numpy(l).to(dev)
    row_slot, ctr = torch.arange(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int64, device=dev)
    G.grammar_mask(lin, bank, row_slot, ctr)
    assert np.array_equal(_bits(lin.cpu().numpy()), _bits(l)), "no slot has a grammar"
    for b, g in enumerate([0, 1, None, 2, 1, 0]):
        bank.set(b, g)
    bank.state.copy_(torch.tensor([1, 2, 0, 1, 0, -1], dtype=torch.int32))
    gram, state = bank.gram.cpu().numpy(), bank.state.cpu().numpy()
    assert gram.tolist() == [0, 1, -1, 2, 1, 0]
    ref = G.reference_mask(l, [G.reference_allow(d, table) for d in dfas[:3]], gram, state, np.arange(B), np.zeros(B), vocab=vocab)
    G.grammar_mask(lin, bank, row_slot, ctr)
    assert np.array_equal(_bits(lin.cpu().numpy()), _bits(ref))
    assert (_bits(ref) != _bits(l)).any(axis=1).tolist() == [True, True, False, True, True, False]


def _segments(rows):
    """rows cut into segments of 16, 1, 5, 9, 16, 3, ... rows and one slot without rows: (row0, slots)"""
    row0, at, lengths = [0], 0, (16, 1, 5, 9, 16, 3)
    while at < rows:
        if len(row0) == 3:
            row0.append(at)  # slot 2 has no rows
        at = min(rows, at + lengths[(len(row0) - 1) % len(lengths)])
        row0.append(at)
    return np.array(row0, np.int32), len(row0) - 1


def _step_tokens(rng, table, shape, other=0.4):
    """tokens of a handful: "a" and "b", which the automata take, and with probability `other` one of ".", "0", eos (often), the
    empty token, ids outside the vocabulary and any token"""
    empty = int(np.flatnonzero(np.diff(table.tok_off) == 0)[0])
    pool = np.array([0, 1, 2, 3, table.eos, empty, table.vocab, -1, 2 ** 40, int(rng.integers(4, table.vocab - 1))])
    p = np.concatenate([[0.5 * (1 - other)] * 2, other * np.array([.125, .125, .375, .075, .075, .075, .075, .075])])
    return rng.choice(pool, size=shape, p=p).astype(np.int64)


def _random_states(rng, dfas, gram):
    """a state per slot: mostly a state of its automaton — [ab]{300}'s above 255 too —, some finished, dead or out of range"""
    out = np.zeros(len(gram), np.int32)
    for b, g in enumerate(gram):
        S = dfas[g].trans.shape[0] if 0 <= g < 3 else 4
        out[b] = rng.choice([rng.integers(0, S), max(0, S - 1 - rng.integers(0, 40)), S, -1, S + 1], p=[0.45, 0.3, 0.1, 0.1, 0.05])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 20, 128])
def test_rows_kernel_is_the_reference(dev, rows):
    """segments of 1 .. 16 rows and a slot without rows; guesses that die in the middle, ids >= vocab, eos inside a draft, finished
    and dead slots, slots without a grammar or with one that is not loaded; every row is written (the sentinel is gone)"""
    vocab = 1000
    row0, slots = _segments(rows)
    table, dfas, bank = _three(dev, vocab, slots, patterns=("(a|b)*abb", "[ab]{300}", SMALL))
    rng = np.random.default_rng(rows)
    seen = set()
    for trial in range(12):
        gram = rng.choice([0, 1, 2, -1, 3], size=slots, p=[0.3, 0.3, 0.2, 0.1, 0.1]).astype(np.int32)
        state = _random_states(rng, dfas, gram)
        tokens = _step_tokens(rng, table, rows)
        ref = G.reference_rows(dfas, table, gram, state, tokens, row0, rows)
        bank.gram.copy_(torch.from_numpy(gram))
        bank.state.copy_(torch.from_numpy(state))
        outs = []
        for fill in (-77, 12345):
            rs = torch.full((rows,), fill, dtype=torch.int32, device=dev)
            assert G.grammar_rows(bank, torch.from_numpy(tokens).to(dev), torch.from_numpy(row0).to(dev), rs) is rs
            outs.append(rs.cpu().numpy())
        assert np.array_equal(outs[0], ref), (trial, outs[0][:24], ref[:24])
        assert np.array_equal(outs[1], outs[0]) and np.array_equal(bank.state.cpu().numpy(), state), "two launches; the state is read only"
        for b in range(slots):
            seg = ref[row0[b]:row0[b + 1]]
            S = dfas[gram[b]].trans.shape[0] if 0 <= gram[b] < 3 else None
            if S and len(seg) > 2:
                seen |= {"dies inside"} if seg[0] >= 0 and seg[-1] < 0 and seg[1] >= 0 else set()
                seen |= {"finished inside"} if seg[0] < S and (seg[1:] == S).any() else set()
                seen |= {"alive to the end"} if seg[-1] >= 0 else set()
                seen |= {"a state above 255"} if (seg > 255).any() and (np.diff(seg[seg >= 0]) != 0).any() else set()
    if rows == 128:
        assert seen == {"dies inside", "finished inside", "alive to the end", "a state above 255"}, seen


@pytest.mark.gpu
@pytest.mark.parametrize("width", [1, 5, 16])
@pytest.mark.parametrize("B", [1, 7, 128])
def test_advance_kernel_is_the_reference(dev, B, width):
    """n below 0, 0, up to width and above it, and no n; inactive slots; eos, the finished state, dead walks, ids outside the
    vocabulary; then a window of the bank's slots (Prefill's: one slot)"""
    vocab = 1000
    table, dfas, bank = _three(dev, vocab, B, patterns=("(a|b)*abb", "[ab]{300}", SMALL))
    rng = np.random.default_rng(100 * B + width)
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt).to(dev).contiguous()
    moved = 0
    for trial in range(4):
        gram = rng.choice([0, 1, 2, -1, 3], size=B, p=[0.3, 0.3, 0.2, 0.1, 0.1]).astype(np.int32)
        state = _random_states(rng, dfas, gram)
        tokens = _step_tokens(rng, table, (B, width), other=min(0.4, 1.5 / width))
        n = rng.integers(-1, width + 2, size=B).astype(np.int32) if trial % 2 == 0 else None
        active = np.where(rng.random(B) < 0.2, -1, rng.integers(0, 1 << 40, size=B)) if trial < 2 else None
        ref = G.reference_advance(dfas, table, gram, state, tokens, n=n, active=active)
        for _ in range(2):
            bank.gram.copy_(torch.from_numpy(gram))
            bank.state.copy_(torch.from_numpy(state))
            G.grammar_advance(bank, t(tokens, torch.int64), n=None if n is None else t(n, torch.int32),
                              active=None if active is None else t(active, torch.int64))
            assert np.array_equal(bank.state.cpu().numpy(), ref), (trial, bank.state.cpu().numpy()[:16], ref[:16], state[:16])
        moved += int(((ref != state) & (ref >= 0)).sum())
    assert moved >= 1, "no slot walked anywhere: the case shows nothing"
    if B > 1:   # slots 3 .. 4 only, tokens [2]: the others keep their state
        bank.state.copy_(torch.from_numpy(state))
        ref2 = state.copy()
        ref2[3:5] = G.reference_advance(dfas, table, gram[3:5], state[3:5], tokens[3:5, 0])
        G.grammar_advance(bank, t(tokens[3:5, 0], torch.int64), slot0=3)
        assert np.array_equal(bank.state.cpu().numpy(), ref2)


def test_entry_points_return_codes():
    """argument errors are codes decided before any stream work, in logit_proc.hip's style (no GPU is touched: host memory stands in)"""
    lib = qp._native.lib()
    buf = np.zeros(1 << 13, dtype=np.int64)
    p = buf.ctypes.data
    assert lib.qpal_grammar_compile(None, p, 1, p, p, 33, 10, 0, p, 2, None) == -3
    assert lib.qpal_grammar_compile(p, p, 0, p, p, 33, 10, 0, p, 2, None) == -1       # no state
    assert lib.qpal_grammar_compile(p, p, 65535, p, p, 33, 10, 0, p, 2, None) == -1   # 0xFFFF is no state
    assert lib.qpal_grammar_compile(p, p, 1, p, p, 33, 10, 33, p, 2, None) == -1      # eos outside the vocabulary
    assert lib.qpal_grammar_compile(p, p, 1, p, p, 33, 10, 0, p, 1, None) == -1       # ld_allow below the words
    assert lib.qpal_grammar_compile(p + 1, p, 1, p, p, 33, 10, 0, p, 2, None) == -4
    assert lib.qpal_grammar_rows(p, p, p, 1, 4, p, p, 33, 10, 0, p, p, 1, p, None, 1, p, None) == -3
    assert lib.qpal_grammar_rows(p, p, p, 1, 4, p, p, 33, 10, 0, p, p, 1, p, p, 129, p, None) == -1
    assert lib.qpal_grammar_rows(p, p, p, 1, 4, p, p, 33, 10, 0, p, p, 129, p, p, 1, p, None) == -1
    assert lib.qpal_grammar_rows(p, p, p, 1, 4, p, p, 33, 10, 0, p, p, 1, p + 4, p, 1, p, None) == -4   # int64 tokens
    assert lib.qpal_grammar_mask(p, 33, 1, 33, p, p, None, p, 1, p, 1, 4, p, 2, None) == -3
    assert lib.qpal_grammar_mask(p, 32, 1, 33, p, p, p, p, 1, p, 1, 4, p, 2, None) == -1                # ld below vocab
    assert lib.qpal_grammar_mask(p, 33, 1, 33, p, p, p, p, 1, p, 0, 4, p, 2, None) == -1
    assert lib.qpal_grammar_mask(p, 33, 1, 33, p, p + 4, p, p, 1, p, 1, 4, p, 2, None) == -4            # int64 ctr
    assert lib.qpal_grammar_advance(p, p, p, 1, 4, p, p, 33, 10, 0, p, None, 1, p, 1, None, None, None) == -3
    assert lib.qpal_grammar_advance(p, p, p, 1, 4, p, p, 33, 10, 0, p, p, 1, p, 17, None, None, None) == -1
    assert lib.qpal_grammar_advance(p, p, p, 1, 4, p, p, 33, 10, 0, p, p, 1, p, 1, p + 2, None, None) == -4


# -------------------------------------------------------------------------------------------------------- whole model

def _load_spec_tests():
    """tests/test_spec.py as a module: its model, prompts, generation loop and near-tie rule are this file's too"""
    spec = importlib.util.spec_from_file_location("_spec_tests_for_grammar", os.path.join(ROOT, "tests", "test_spec.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ts = _load_spec_tests()
NB, L, NEW, DRAFT, VOCAB, F16 = ts.NB, ts.L, ts.NEW, ts.DRAFT, ts.VOCAB, ts.F16
NUMBER, PAIRS = r"-?(0|[1-9]\d*)(\.\d+)?", r"(ab|ba){3,5}x?"   # unbounded; bounded: after at most 11 bytes only eos is left
SLOT_GRAMMAR = [0, 1, None, 0]                                  # slot 2 runs free


def _model_table():
    """a synthetic vocabulary for the model's 4096 ids: strings of 1 .. 4 bytes over "ab0123456789.-x", 2 % special tokens without
    bytes; the single characters come first, so every state of both grammars has a token; eos = 2 carries bytes no grammar takes"""
    if "model" not in _TABLES:
        rng = np.random.default_rng(4096)
        alpha = b"ab0123456789.-x"
        toks = [bytes([c]) for c in alpha]
        while len(toks) < VOCAB:
            toks.append(b"" if rng.random() < 0.02 else bytes(rng.choice(np.frombuffer(alpha, np.uint8), size=rng.integers(1, 5)).tolist()))
        toks[2], toks[-1] = b"</s>", b"0"     # ("0" was token 2)
        _TABLES["model"] = G.TokenTable(toks, eos=2)
    return _TABLES["model"]


@pytest.fixture(scope="module")
def model(dev):
    sys.path.insert(0, os.path.join(ROOT, "perf"))
    from decode_llama import build_model
    return build_model("3_8b", "tcomb_6_7_0.5_none_0.9", None, 2, VOCAB, dev)


@pytest.fixture(scope="module")
def prompts(dev):
    g = torch.Generator().manual_seed(ts.PROMPT_SEED)
    return [torch.randint(0, VOCAB, (n,), generator=g).to(dev) for n in ts.PROMPT_LENGTHS]


def _configured(dev, neutral=False):
    bank = qp.GrammarBank(NB, _model_table(), dev, grammars=2, max_states=32)
    bank.load(0, NUMBER)
    bank.load(1, PAIRS)
    if not neutral:
        for b, g in enumerate(SLOT_GRAMMAR):
            bank.set(b, g)
    return bank


def _params(mode):
    return ts.MIXED if mode == "mixed" else ts.GREEDY


def _sequential(dev, m, prompts, mode, bank, chunk=128, proc=None):
    """Prefill draws the first new token, DecodeStep(generic=True) the rest (test_spec's yardstick, with a bank or None, and a logit
    processor or None).  Returns (streams, the logits as the sampler held them after each draw, the sampler)."""
    kc, vc = ts._caches(m, dev, F16)
    smp = qp.Sampler(NB, VOCAB, dev, **_params(mode))
    pf = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, chunk=chunk, sampler=smp, grammar=bank, processor=proc)
    tok = torch.zeros(NB, dtype=torch.long, device=dev)
    streams, logits = [[] for _ in range(NB)], [[] for _ in range(NB)]
    for b, p in enumerate(prompts):
        tok[b] = pf(p, slot=b, pos0=0)[0]
        logits[b].append(smp.logits[b].cpu().numpy().copy())
        streams[b].append(int(tok[b]))
    pos = torch.tensor([p.shape[0] for p in prompts], dtype=torch.long, device=dev)
    out = torch.zeros(NB, dtype=torch.long, device=dev)
    ds = qp.DecodeStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, tok, pos, out, generic=True, sampler=smp, grammar=bank,
                       processor=proc)
    assert ds.launches_per_token == 9 * len(m.layers) + 2 + (2 if bank is not None else 0) + (2 if proc is not None else 0)
    for _ in range(NEW - 1):
        ds()
        lgts = smp.logits.cpu().numpy()
        for b in range(NB):
            streams[b].append(int(out[b]))
            logits[b].append(lgts[b].copy())
        tok.copy_(out)
        pos += 1
    return streams, logits, smp


_YARD = {}


def _yardstick(dev, m, prompts, mode):
    """the sequential streams under the configured bank, once per sampling mode: (streams, masked logits, the bank's final state)"""
    if mode not in _YARD:
        bank = _configured(dev)
        streams, logits, _ = _sequential(dev, m, prompts, mode, bank)
        _YARD[mode] = (streams, logits, bank.state.cpu().numpy())
    return _YARD[mode]


def _check_streams(streams, state):
    """every grammar slot's text is at each step a live prefix of its pattern (the host walk never dies), a text that ended in eos
    matches the pattern as Python's `re` reads it, and `state` is the host walk of the emitted tokens"""
    table = _model_table()
    dfas = [G.compile_regex(NUMBER), G.compile_regex(PAIRS)]
    gram = np.array([-1 if g is None else g for g in SLOT_GRAMMAR])
    for b, g in enumerate(SLOT_GRAMMAR):
        if g is None:
            continue
        s, ended = 0, None
        for i, t in enumerate(streams[b]):
            s = G.reference_step(dfas[g], table, s, t)
            assert s != G.DEAD_STATE, f"slot {b}: token {i} = {t} ({table.token(t)!r}) leaves the grammar after {table.text(streams[b][:i])!r}"
            if ended is None:
                assert G.dfa_live_prefix(dfas[g], table.text(streams[b][:i + 1])) is not None
            if t == table.eos and ended is None:
                ended = i
        if ended is not None:
            text = table.text(streams[b][:ended])
            assert re.fullmatch((NUMBER, PAIRS)[g].encode(), text), (b, text)
            assert all(t == table.eos for t in streams[b][ended:]), "behind eos only eos"
    walk = G.reference_advance(dfas, table, gram, np.zeros(NB, np.int32), np.array([s for s in streams]))
    assert np.array_equal(state, walk), (state, walk)


def _one_slot_against(got, want, logits, prompt_len, params, slot):
    """tests/test_spec.py's near-tie rule on one slot's stream: equal, or a first difference that is a near tie in the yardstick's
    logits of that step (the comparison ends there); at most 5 % of the run's tokens may lie behind it"""
    diff = [i for i in range(NEW) if got[i] != want[i]]
    if diff:
        i = diff[0]
        s = ts._scores(logits[i], params, slot, prompt_len - 1 + i)
        gap, thr = abs(float(s[want[i]] - s[got[i]])), 2 * ts._bound(logits[i])
        print(f"slot {slot} token {i}: {got[i]} for {want[i]}, score gap {gap:.4g}, excuse threshold {thr:.4g}")
        assert gap < thr, f"slot {slot} token {i}: {got[i]} for {want[i]} is no near tie ({gap} >= {thr})"
        assert NEW - i <= 0.05 * NB * NEW, f"{NEW - i} of {NB * NEW} tokens lie behind an excused near tie"


@pytest.mark.gpu
def test_a_bank_without_grammars_changes_no_bit(dev, model, prompts, monkeypatch):
    """Prefill, DecodeStep and SpeculativeStep with a bank whose slots all have gram = -1.  Two runs of one step agree to rounding
    only (the batched projections accumulate with float atomics), so "the same step without a bank" is the same run:
    the logits in front of the mask launch against what it left, bit for bit, the step's tokens against a draw from a copy of the
    logits in front of it, and the bank's state untouched."""
    calls, real = [], G.grammar_mask

    def spy(logits, bank, row_slot, ctr, **kw):
        before = logits.clone()
        real(logits, bank, row_slot, ctr, **kw)
        calls.append((before, logits.clone(), ctr.clone()))
        return logits
    monkeypatch.setattr(G, "grammar_mask", spy)
    bank = _configured(dev, neutral=True)
    bank.state.copy_(torch.tensor([0, 3, 1, 2], dtype=torch.int32))
    streams, _, smp = _sequential(dev, model, prompts, "mixed", bank, chunk=16)
    assert len(calls) == NB + NEW - 1, "one mask launch per Prefill call and per DecodeStep"
    for i, (before, after, ctr) in enumerate(calls):
        assert torch.equal(before.view(torch.int32), after.view(torch.int32)), i
        if i < NB:
            assert qp.sample(before, smp.slot(i), ctr).tolist() == [streams[i][0]]
        else:
            assert qp.sample(before, smp, ctr).tolist() == [streams[b][i - NB + 1] for b in range(NB)]
    assert bank.state.tolist() == [0, 3, 1, 2] and bank.gram.tolist() == [-1] * NB
    del calls[:]
    ss = _spec_step(model, dev, prompts, "mixed", bank)
    bank.state.copy_(torch.tensor([0, 3, 1, 2], dtype=torch.int32))   # (begin put them at the start)
    got, records = ts._generate(ss, dev, None, "a")
    assert len(calls) == len(records) and all(len(g) == NEW for g in got)
    assert all(torch.equal(before.view(torch.int32), after.view(torch.int32)) for before, after, _ in calls)
    before, _, ctr = calls[-1]
    assert torch.equal(qp.sample(before, ss.draw, ctr, out=ss.drawn.clone()), ss.drawn)
    assert bank.state.tolist() == [0, 3, 1, 2] and bool((ss._row_state == -1).all())


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["greedy", "mixed"])
def test_sequential_generation_follows_the_grammars(dev, model, prompts, mode):
    """Prefill + DecodeStep with slots 0 and 3 on a number, slot 1 on a bounded pattern and slot 2 free: the free slot emits what a
    step built without a bank emits (near-tie rule), the others stay inside their patterns; the bounded one ends in eos and stays
    there; the masked logits are -inf exactly where the host's table says so"""
    streams, logits, state = _yardstick(dev, model, prompts, mode)
    _check_streams(streams, state)
    plain, plain_logits, _ = ts._yardstick(dev, model, prompts, F16, mode)
    _one_slot_against(streams[2], plain[2], plain_logits[2], prompts[2].shape[0], _params(mode), 2)
    table = _model_table()
    assert table.eos in streams[1] and streams[1][-1] == table.eos, "the bounded pattern has ended"
    assert streams[0] != plain[0] and streams[1] != plain[1] and streams[3] != plain[3], "the grammars bind"
    # the first draw of slot 0: the start state's row of the table
    allow = G.reference_allow(G.compile_regex(NUMBER), table)
    idx = np.arange(VOCAB)
    bit = (allow[0][idx >> 5] >> (idx & 31).astype(np.uint32)) & 1
    assert np.array_equal(np.isneginf(logits[0][0]), bit == 0) and 0 < int(bit.sum()) < VOCAB


def _spec_step(m, dev, prompts, mode, bank, proc=None):
    """tests/test_spec.py's _spec_step on fp16 caches, with a bank and a sampler (greedy: temperature 0): prompts[b][:-1] prefilled.
    No eos is given to begin: a finished slot goes on emitting eos, as the sequential yardstick does."""
    kr, vr = ts._caches(m, dev, F16)
    pf = qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kr, vr, m.inv_freq, chunk=128)
    smp = qp.Sampler(NB, VOCAB, dev, **_params(mode))
    ss = qp.SpeculativeStep(m.layers, m.embed, m.norm, m.lm_head, kr, vr, m.inv_freq, draft=DRAFT, gram=(2, 4), sampler=smp, grammar=bank,
                            processor=proc)
    for b, p in enumerate(prompts):
        pf(p[:-1], slot=b, pos0=0)
        ss.begin(b, p.tolist(), limit=p.shape[0] + NEW)
    return ss


@pytest.mark.gpu
@pytest.mark.parametrize("way", ["a", "c", "d"], ids=["lookup", "third-wrong", "all-wrong"])
@pytest.mark.parametrize("mode", ["greedy", "mixed"])
def test_speculative_step_with_grammars_emits_the_sequential_stream(dev, model, prompts, mode, way):
    """tests/test_spec.py's comparison and near-tie rule (_judge: excuse threshold and the 5 % cap as they are there), the scores
    taken from the MASKED logits the yardstick's sampler held.  Whatever the step emits stays inside the grammars, and the device
    state is the host walk of it."""
    want, logits, _ = _yardstick(dev, model, prompts, mode)
    bank = _configured(dev)
    bank.state.fill_(7)                       # begin puts every slot at the start
    ss = _spec_step(model, dev, prompts, mode, bank)
    assert bank.state.tolist() == [0] * NB
    got, records = ts._generate(ss, dev, want, way)
    _check_streams(got, bank.state.cpu().numpy())
    acc, drafts = ts._judge(got, records, want, logits, prompts, _params(mode), way)
    print(f"grammars {mode} {way}: {len(records)} steps for {NEW} tokens per slot, {acc} of {drafts} drafts accepted")
    if way == "a":
        assert acc > 0, "no draft was accepted: the rows behind the first were never used"


@pytest.mark.gpu
def test_a_grammar_behind_a_logit_processor(dev, model, prompts):
    """process first, mask second, in the sequential steps and in every row of a speculative step: penalties in every slot (a
    repetition penalty on the number slots, presence and frequency on the others), the grammars of the other tests, seeded
    sampling, every third caller's draft wrong — the speculative stream is the sequential one, stays inside the grammars, and the
    processor's counts are the histogram of prompt and emitted tokens"""
    def processor():
        proc = qp.LogitProcessor(NB, VOCAB, dev)
        for b in range(NB):
            proc.set(b, **(dict(repetition=1.3) if SLOT_GRAMMAR[b] == 0 else dict(presence=0.5, frequency=0.3)))
        return proc
    bank = _configured(dev)
    want, logits, _ = _sequential(dev, model, prompts, "mixed", bank, proc=processor())
    _check_streams(want, bank.state.cpu().numpy())
    assert want != _yardstick(dev, model, prompts, "mixed")[0], "the penalties bind"
    bank2, proc2 = _configured(dev), processor()
    ss = _spec_step(model, dev, prompts, "mixed", bank2, proc=proc2)
    got, records = ts._generate(ss, dev, want, "c")
    _check_streams(got, bank2.state.cpu().numpy())
    ts._judge(got, records, want, logits, prompts, ts.MIXED, "c")
    count = proc2.count.cpu().numpy()
    for b, p in enumerate(prompts):
        assert np.array_equal(count[b], np.bincount(p.tolist() + got[b], minlength=VOCAB)), b


@pytest.mark.gpu
def test_a_captured_decode_step_follows_the_grammar_over_replays(dev, model, prompts):
    """one captured DecodeStep with its feedback (tok <- out_tok, pos += 1) inside the graph: replays with no host write in between
    stay inside the grammars; bank.set(slot, other grammar) between replays changes the stream from the
    next draw"""
    table = _model_table()
    dfas = [G.compile_regex(NUMBER), G.compile_regex(PAIRS)]
    assert not set(b"ab") & set(b"-0123456789."), "no token of one grammar continues the other"

    def build():
        kc, vc = ts._caches(model, dev, F16)
        smp, bank = qp.Sampler(NB, VOCAB, dev, temperature=0.0), _configured(dev)
        tok = torch.tensor([5, 6, 7, 8], dtype=torch.long, device=dev)
        pos, out = torch.zeros(NB, dtype=torch.long, device=dev), torch.zeros(NB, dtype=torch.long, device=dev)
        ds = qp.DecodeStep(model.layers, model.embed, model.norm, model.lm_head, kc, vc, model.inv_freq, tok, pos, out, generic=True,
                           sampler=smp, grammar=bank)

        def step():
            ds()
            tok.copy_(out)
            pos.add_(1)
        return bank, tok, pos, out, step

    bank, tok, pos, out, step = build()
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        step()                 # warm-up
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            step()
        pos.zero_()            # a new start: positions, tokens, every slot's state (set puts it at the start)
        tok.copy_(torch.tensor([5, 6, 7, 8]))
        for b, gr in enumerate(SLOT_GRAMMAR):
            bank.set(b, gr)
        got = []
        for i in range(12):
            if i == 8:
                bank.set(0, 1)
            g.replay()
            torch.cuda.synchronize()
            got.append(out.tolist())   # (a host READ; nothing is written between the replays but the set above)
    streams = [[row[b] for row in got] for b in range(NB)]

    def walk(dfa, tokens, s_=0):
        for t in tokens:
            s_ = G.reference_step(dfa, table, s_, t)
        return s_
    for b, gr in ((1, 1), (3, 0)):
        assert walk(dfas[gr], streams[b]) != G.DEAD_STATE and int(bank.state[b]) == walk(dfas[gr], streams[b]), (b, streams[b])
    before = walk(dfas[0], streams[0][:8])
    assert before != G.DEAD_STATE, streams[0]
    assert walk(dfas[1], streams[0][8:]) != G.DEAD_STATE, "from the ninth draw slot 0 follows the other grammar from its start"
    assert int(bank.state[0]) == walk(dfas[1], streams[0][8:]) and walk(dfas[0], streams[0][8:9], before) == G.DEAD_STATE
    assert table.eos in streams[1] and bank.matched(1), "the bounded pattern ended inside the replays"
    assert int(pos[0]) == 12


@pytest.mark.gpu
def test_steps_refuse_a_bank_they_cannot_serve(dev, model):
    kc, vc = ts._caches(model, dev, F16)
    m, E = model, qp._native.QpalError
    table = _model_table()
    bank = qp.GrammarBank(NB, table, dev, grammars=1, max_states=8)
    smp = qp.Sampler(NB, VOCAB, dev)
    tok = torch.zeros(NB, dtype=torch.long, device=dev)
    mk = {"Prefill": lambda **kw: qp.Prefill(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, **kw),
          "DecodeStep": lambda **kw: qp.DecodeStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, tok, tok.clone(), tok.clone(),
                                                   generic=True, **kw),
          "SpeculativeStep": lambda **kw: qp.SpeculativeStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, **kw)}
    small = G.TokenTable([table.token(t) for t in range(VOCAB - 1)], eos=2)
    for who, make in mk.items():
        with pytest.raises(E, match=f"{who}: a grammar masks the logits of a sampler's tail"):
            make(grammar=bank)
        with pytest.raises(E, match=f"{who}: grammar must be a GrammarBank of 4 slots of 4096 tokens"):
            make(sampler=smp, grammar=qp.GrammarBank(NB + 1, table, dev, grammars=1, max_states=8))
        with pytest.raises(E, match="GrammarBank of 4 slots"):
            make(sampler=smp, grammar=qp.GrammarBank(NB, small, dev, grammars=1, max_states=8))
        with pytest.raises(E, match="GrammarBank of 4 slots"):
            make(sampler=smp, grammar=qp.GrammarBank(NB, table, "cpu", grammars=1, max_states=8))
        with pytest.raises(E, match="GrammarBank of 4 slots"):
            make(sampler=smp, grammar=qp.LogitProcessor(NB, VOCAB, dev))
        make(sampler=smp, grammar=bank)
    with pytest.raises(E, match="no grammar on a ragged step"):
        qp.RaggedStep(m.layers, m.embed, m.norm, m.lm_head, kc, vc, m.inv_freq, sampler=smp, grammar=bank)
