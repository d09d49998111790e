"""The host side of grammar-constrained decoding (qpalette_amd.grammar), CPU only: compile_regex against Python's `re`
on bytes patterns, the shape of the automaton (minimal enough to be trimmed: every state reachable and able to accept), the errors,
and the numpy contracts the kernels are held to — reference_allow / _step / _rows / _advance / _mask — on hand-made cases and
against a brute-force walk."""
import itertools
import re

import numpy as np
import pytest

from qpalette_amd import grammar as G
from qpalette_amd.logits import mask_bits

# (pattern, the bytes pattern `re` compiles where it differs, a 6-symbol alphabet); one construct of the subset each
PATTERNS = [
    ("abc", None, b"abcd \n"),                               # literals
    ("ab|cd|a", None, b"abcd|e"),                            # alternation
    ("a*b", None, b"ab*c\n "),                               # star
    ("a+b?", None, b"ab+?c "),                               # plus, optional
    ("(ab)+c", None, b"abc()+"),                             # a capturing group
    ("(?:ab|c)*d", None, b"abcd?:"),                         # a non-capturing group
    ("a{3}", None, b"a{3}b "),                               # {m}
    ("a{2,}b", None, b"ab2,{}"),                             # {m,}
    ("(?:ab){1,3}", None, b"ab13, "),                        # {m,n}
    ("a{0,2}b{0}c", None, b"abc0{}"),                        # zero counts
    (".a.", None, b"a.\nb\x00\xff"),                         # any byte but \n
    ("[abc]+", None, b"abcd[]"),                             # a class
    ("[^ab]c", None, b"abc^\n\xfe"),                         # a negated class
    ("[a-c0-2]*", None, b"ac03b-"),                          # ranges
    ("[]a]+[^]]", None, b"]a[^b\\"),                         # ']' first in a class is a member
    (r"[a\-c]+", None, b"a-cb\\ "),                          # an escaped '-' in a class
    (r"[\d\s]+x", None, b"0 9x\td"),                         # shorthands in a class
    (r"\d+\.\d", None, b"019.d\\"),                          # \d and an escaped metacharacter
    (r"\D\w\W", None, b"a_1 -\xe9"),                         # \D \w \W (ASCII meaning on bytes)
    (r"\s\S", None, b" \t\n\x0bab"),                         # \s \S
    (r"\n\r\t\\", None, b"\n\r\t\\nr"),                      # control escapes and the backslash
    (r"\x41\x00[\x7f-\xff]", None, b"A\x00\x7f\xffx4"),      # \xHH, also as range ends
    (r"(\(|\)|\[|\]|\{|\})+", None, b"()[]{}"),                  # escaped brackets
    (r"\*?\+\?\|\^\$", None, b"*+?|^$"),                     # the other escaped metacharacters
    (r"-?(0|[1-9]\d*)(\.\d+)?", None, b"-0.15a"),            # a number
    ("(a|b)*abb", None, b"abc() "),                          # the textbook subset construction
    ("(|a)b", None, b"ab|() "),                              # an empty branch
    ("é+x", b"(?:\xc3\xa9)+x", b"\xc3\xa9x\xc2e+"),          # a non-ASCII character: its UTF-8 bytes as one group
    ("", None, b"ab \n\x00\xff"),                            # the empty pattern
]


def _strings(alphabet, rng):
    for n in range(6):
        for t in itertools.product(alphabet, repeat=n):
            yield bytes(t)
    lengths = rng.integers(0, 21, size=2000)
    # random strings: mostly from the alphabet (so that long matches occur), some bytes from anywhere
    for n in lengths:
        s = rng.choice(np.frombuffer(alphabet, np.uint8), size=n)
        wild = rng.random(n) < 0.03
        s = np.where(wild, rng.integers(0, 256, size=n), s).astype(np.uint8)
        yield s.tobytes()


@pytest.mark.parametrize("pattern,as_bytes,alphabet", PATTERNS, ids=[repr(p[0]) for p in PATTERNS])
def test_compile_regex_means_what_re_fullmatch_means_on_bytes(pattern, as_bytes, alphabet):
    """every byte string up to length 5 over a 6-symbol alphabet (9331 of them) and 2000 random strings up to length 20"""
    assert len(set(alphabet)) == 6
    dfa = G.compile_regex(pattern)
    ref = re.compile(pattern.encode("ascii") if as_bytes is None else as_bytes)
    rng = np.random.default_rng(len(pattern) + 17)
    n = hits = 0
    for s in _strings(alphabet, rng):
        want = ref.fullmatch(s) is not None
        assert G.dfa_match(dfa, s) == want, (pattern, s, want)
        n, hits = n + 1, hits + want
    assert n == sum(6 ** k for k in range(6)) + 2000 and hits >= 1, "the alphabet never matched: the case shows nothing"
    if pattern:
        assert hits < n


def _reach(trans, starts, forward=True):
    S = trans.shape[0]
    edges = [set(int(x) for x in trans[s] if x != G.DEAD) for s in range(S)]
    if not forward:
        back = [set() for _ in range(S)]
        for s in range(S):
            for t in edges[s]:
                back[t].add(s)
        edges = back
    seen, stack = set(starts), list(starts)
    while stack:
        for t in edges[stack.pop()]:
            if t not in seen:
                seen.add(t)
                stack.append(t)
    return seen


@pytest.mark.parametrize("pattern", [p[0] for p in PATTERNS] + ["[ab]{300}", r"(a|bc|def){2,7}x?"], ids=repr)
def test_the_automaton_is_trimmed_and_well_formed(pattern):
    dfa = G.compile_regex(pattern)
    S = dfa.trans.shape[0]
    assert dfa.trans.dtype == np.uint16 and dfa.trans.shape == (S, 256) and dfa.accept.dtype == np.uint8 and dfa.accept.shape == (S,)
    assert np.all((dfa.trans < S) | (dfa.trans == G.DEAD))
    assert _reach(dfa.trans, [0]) == set(range(S)), "every state is reachable from the start"
    assert _reach(dfa.trans, [s for s in range(S) if dfa.accept[s]], forward=False) == set(range(S)), "every state can accept"
    # minimal: no two states with the same acceptance and the same row (a necessary condition that catches a missing merge)
    rows = {(int(dfa.accept[s]), dfa.trans[s].tobytes()) for s in range(S)}
    assert len(rows) == S


def test_known_sizes():
    assert G.compile_regex("[ab]{300}").trans.shape[0] == 301
    assert G.compile_regex("(a|b)*abb").trans.shape[0] == 4
    assert G.compile_regex("abc|abd").trans.shape[0] == 4      # the common prefix and the common end are shared
    assert G.compile_regex("a|a|a").trans.shape[0] == 2


def test_the_empty_pattern_is_one_accepting_state():
    dfa = G.compile_regex("")
    assert dfa.trans.shape == (1, 256) and np.all(dfa.trans == G.DEAD) and dfa.accept.tolist() == [1]


@pytest.mark.parametrize("pattern,where", [
    ("^a", 0), ("a$", 1), (r"a\b", 1), (r"\Aa", 0), (r"(a)\1", 3), ("(?=a)a", 0), ("(?!a)b", 0), ("(?<=a)b", 0), ("a*?", 2), ("a+?", 2),
    ("a??", 2), ("a{2}?", 4), ("a*+", 2), ("a++", 2), ("(?i)a", 0), ("(?P<n>a)", 0), ("(?#c)a", 0), ("a**", 2), ("*a", 0), ("a|*", 2),
    ("(a", 0), ("a)", 1), ("[a", 0), ("a{", 1), ("a{,3}", 1), ("a{x}", 1), ("a{3,2}", 0), ("[c-a]", None), (r"[a-\d]", None),
    ("[é]", 1), (r"\x4", 0), (r"\q", 0), (r"\0", 0), ("a\\", None), ("[[:alpha:]]", 1), ("}", 0), ("]", 0),
], ids=repr)
def test_what_is_outside_the_subset_raises_and_names_the_position(pattern, where):
    with pytest.raises(ValueError, match="position" if where is None else f"position {where} "):
        G.compile_regex(pattern)


def test_too_many_states_raise():
    with pytest.raises(ValueError, match="301 states, more than max_states = 300"):
        G.compile_regex("[ab]{300}", max_states=300)
    assert G.compile_regex("[ab]{300}", max_states=301).trans.shape[0] == 301
    with pytest.raises(ValueError, match="max_states must be"):
        G.compile_regex("a", max_states=65535)
    with pytest.raises(ValueError, match="matches nothing"):
        G.compile_regex(r"a[^\x00-\xff]")


# ---------------------------------------------------------------------------------------------------------------- the contracts

# tokens:   0 "a"   1 "b"   2 "ab"   3 ""(special)   4 "abb"   5 "c"   6 eos   7 "ba"   8 "bb"
TOKS = [b"a", b"b", b"ab", b"", b"abb", b"c", b"</s>", b"ba", b"bb"]
EOS = 6


def _bits(allow, s, vocab):
    return {t for t in range(vocab) if (int(allow[s, t >> 5]) >> (t & 31)) & 1}


def test_token_table():
    tb = G.TokenTable(TOKS, eos=EOS)
    assert tb.vocab == 9 and tb.eos == 6 and tb.tok_off.dtype == np.int32 and tb.tok_bytes.dtype == np.uint8
    assert tb.tok_off.tolist() == [0, 1, 2, 4, 4, 7, 8, 12, 14, 16] and tb.tok_bytes.tobytes() == b"abababbc</s>babb"
    assert tb.token(4) == b"abb" and tb.token(3) == b"" and tb.text([0, 4, 6, 1]) == b"aabbb"
    for eos in (None, -1, 9):
        with pytest.raises(ValueError, match="eos"):
            G.TokenTable(TOKS, eos=eos)
    only_special = G.TokenTable([b"", b""], eos=1)
    assert only_special.total == 0 and only_special.tok_bytes.shape == (1,)


def test_reference_allow_and_step_by_hand():
    """(a|b)*abb: states 0 (start), 1 (.. a), 2 (.. ab), 3 (.. abb, accepting); 'c' leads nowhere"""
    dfa = G.compile_regex("(a|b)*abb")
    tb = G.TokenTable(TOKS, eos=EOS)
    S = 4
    acc = [s for s in range(S) if dfa.accept[s]]
    assert len(acc) == 1
    allow = G.reference_allow(dfa, tb)
    assert allow.dtype == np.uint32 and allow.shape == (S + 1, 1)
    for s in range(S):
        want = {0, 1, 2, 4, 7, 8} | ({EOS} if s in acc else set())    # never the empty token 3, never "c"
        assert _bits(allow, s, 9) == want, s
    assert _bits(allow, S, 9) == {EOS}, "the finished row: eos only"
    # steps: eos in and outside an accepting state, the finished state, the dead state, ids outside the vocabulary, the empty token
    s_abb = G.reference_step(dfa, tb, 0, 4)
    assert s_abb == acc[0] and G.reference_step(dfa, tb, G.reference_step(dfa, tb, 0, 2), 1) == s_abb
    assert G.reference_step(dfa, tb, s_abb, EOS) == S and G.reference_step(dfa, tb, 0, EOS) == G.DEAD_STATE
    assert G.reference_step(dfa, tb, S, EOS) == S and G.reference_step(dfa, tb, S, 0) == G.DEAD_STATE
    assert G.reference_step(dfa, tb, G.DEAD_STATE, 0) == G.DEAD_STATE and G.reference_step(dfa, tb, G.DEAD_STATE, EOS) == G.DEAD_STATE
    assert G.reference_step(dfa, tb, S + 1, 0) == G.DEAD_STATE and G.reference_step(dfa, tb, -7, 0) == G.DEAD_STATE
    for t in (3, 5, 9, -1, 2 ** 40):
        assert G.reference_step(dfa, tb, 0, t) == G.DEAD_STATE, t
    # the bit and the step agree everywhere
    for s in range(S + 1):
        for t in range(9):
            assert (t in _bits(allow, s, 9)) == (G.reference_step(dfa, tb, s, t) != G.DEAD_STATE), (s, t)


def test_eos_without_bytes_and_with_bytes_that_would_walk():
    """eos is allowed exactly in accepting states: not because its bytes walk ("a" as eos), and although it has none"""
    dfa = G.compile_regex("a+")
    for toks in ([b"a", b"", b"aa"], [b"a", b"a", b"aa"]):      # eos = token 1: no bytes; the bytes "a", which the automaton takes
        tb = G.TokenTable(toks, eos=1)
        allow = G.reference_allow(dfa, tb)
        assert _bits(allow, 0, 3) == {0, 2} and _bits(allow, 1, 3) == {0, 1, 2} and _bits(allow, 2, 3) == {1}
        assert G.reference_step(dfa, tb, 0, 1) == G.DEAD_STATE and G.reference_step(dfa, tb, 1, 1) == 2


def test_reference_allow_against_a_brute_force_walk():
    """a 40-token vocabulary of random strings over "ab.0" (lengths 0 .. 6), three automata, every (state, token) pair by dfa walk"""
    rng = np.random.default_rng(5)
    toks = [bytes(rng.choice(np.frombuffer(b"ab.0", np.uint8), size=rng.integers(0, 7)).tolist()) for _ in range(40)]
    toks[7] = b""
    tb = G.TokenTable(toks, eos=33)
    for pattern in (r"(a|b)*abb", r"[ab0]+(\.0+)?", "[ab]{9}", ""):
        dfa = G.compile_regex(pattern)
        S = dfa.trans.shape[0]
        allow = G.reference_allow(dfa, tb)
        assert allow.shape == (S + 1, 2) and not (allow[:, 1] >> 8).any(), "the bits past the vocabulary are clear"
        for s in range(S + 1):
            want = set()
            for t, by in enumerate(toks):
                if t == 33:
                    ok = s == S or bool(dfa.accept[s])
                elif s == S or not by:
                    ok = False
                else:
                    cur = s
                    for c in by:
                        cur = int(dfa.trans[cur, c]) if cur != G.DEAD else cur
                    ok = cur != G.DEAD
                if ok:
                    want.add(t)
            assert _bits(allow, s, 40) == want, (pattern, s)
            assert np.array_equal(allow[s], mask_bits(sorted(want), 40)), "mask_bits' layout"


def _bank():
    tb = G.TokenTable(TOKS, eos=EOS)
    return tb, [G.compile_regex("(a|b)*abb"), None, G.compile_regex("ab?")]


def test_reference_rows_by_hand():
    """five slots: a draft that stays alive, one that dies in the middle, one with an id >= vocab, a slot without grammar, a slot
    without rows; then eos inside a draft and the finished state"""
    tb, gr = _bank()
    gram = np.array([0, 0, 2, -1, 0, 1, 7])          # slot 5: a grammar id that is not loaded; slot 6: one outside the list
    state = np.array([0, 1, 0, 0, 0, 0, 0])
    #          slot 0: a | ab b c(dead) a      slot 1: b | bb eos eos a  slot 2: a | 99 a   slot 3: a | a   slot 5, 6: a
    tokens = np.array([0, 2, 1, 5, 0, 1, 8, EOS, EOS, 0, 0, 99, 0, 0, 0, 0, 0])
    row0 = np.array([0, 5, 10, 13, 15, 15, 16, 17])
    got = G.reference_rows(gr, tb, gram, state, tokens, row0, 17)
    d0 = gr[0]
    s_a = G.reference_step(d0, tb, 0, 0)
    assert got.dtype == np.int32
    a_ab = G.reference_step(d0, tb, 0, 2)
    a_abb = G.reference_step(d0, tb, a_ab, 1)
    assert got[:5].tolist() == [0, a_ab, a_abb, -1, -1], "the pending token is in the state already; c kills the rows behind it"
    s1b = G.reference_step(d0, tb, 1, 8)
    assert got[5:10].tolist() == [1, s1b, 4, 4, -1] and s1b == a_abb, "eos in an accepting state: finished, eos again, then dead"
    assert got[10:13].tolist() == [0, -1, -1], "an id >= vocab is dead"
    assert got[13:].tolist() == [-1, -1, -1, -1], "no grammar, an id that is not loaded, an id outside the list"
    assert s_a == 1
    # a segment of 17 rows is none; a state outside 0 .. S leaves the rows dead
    assert G.reference_rows(gr, tb, [0], [0], np.zeros(17, np.int64), [0, 17], 17).tolist() == [-1] * 17
    assert G.reference_rows(gr, tb, [0], [5], np.zeros(3, np.int64), [0, 3], 3).tolist() == [-1] * 3
    assert G.reference_rows(gr, tb, [0], [4], np.array([0, EOS, 0]), [0, 3], 3).tolist() == [4, 4, -1], "from the finished state"


def test_reference_advance_by_hand():
    tb, gr = _bank()
    gram = np.array([0, 0, 2, -1, 0, 0])
    state = np.array([0, 0, 0, 3, 2, -1])
    tokens = np.array([[2, 1, EOS], [2, 1, EOS], [0, 1, 1], [5, 5, 5], [1, EOS, EOS], [0, 0, 0]])
    out = G.reference_advance(gr, tb, gram, state, tokens)
    assert out.dtype == np.int32 and out.tolist() == [4, 4, -1, 3, 4, -1]
    n = np.array([2, 0, 2, 3, -5, 99])
    assert G.reference_advance(gr, tb, gram, state, tokens, n=n).tolist() == [3, 0, 2, 3, 2, -1], "n = 0 and n < 0: nothing; n > width: width"
    active = np.array([-1, 5, 0, 0, 0, 0])
    assert G.reference_advance(gr, tb, gram, state, tokens, active=active).tolist() == [0, 4, -1, 3, 4, -1], "an inactive slot keeps its state"
    assert G.reference_advance(gr, tb, [0], [9], [[0]]).tolist() == [-1], "a state outside -1 .. S is dead once it is advanced"
    assert G.reference_advance(gr, tb, [0, 2], [0, 0], np.array([0, 0])).tolist() == [1, 1], "tokens [slots]: width 1"


def test_reference_mask_by_hand():
    tb, gr = _bank()
    allows = [None if d is None else G.reference_allow(d, tb) for d in gr]
    vocab, ld = 9, 12
    rng = np.random.default_rng(0)
    l = rng.normal(size=(8, ld)).astype(np.float32)
    l[0, 5], l[0, 0], l[1, 3] = np.nan, np.nan, -np.inf
    gram = np.array([0, 2, -1, 1])
    #                       row: 0  1  2       3   4  5  6          7
    row_slot = np.array([0, 1, 2, 0, 0, 4, 3, 0])    # row 5: a slot outside; row 6: slot 3's grammar is not loaded
    row_state = np.array([0, 1, 0, -1, 5, 0, 0, 4])  # row 3: dead; row 4: outside 0 .. S = 4; row 7: finished
    ctr = np.array([7, 0, 3, 3, 3, 3, 3, 1 << 40])
    ctr2 = ctr.copy()
    ctr2[1] = -1
    out = G.reference_mask(l, allows, gram, row_state, row_slot, ctr, vocab=vocab)
    bits = lambda a: a.view(np.uint32)
    for r in (2, 3, 4, 5, 6):
        assert np.array_equal(bits(out[r]), bits(l[r])), f"row {r} is skipped and keeps every bit"
    assert np.array_equal(bits(out[:, vocab:]), bits(l[:, vocab:])), "the columns past vocab are kept"
    gone = lambda r: set(np.flatnonzero(np.isneginf(out[r, :vocab]) & ~np.isneginf(l[r, :vocab])).tolist())
    assert gone(0) == {3, 5, EOS} and np.isnan(out[0, 0]), "a disallowed NaN becomes -inf, an allowed one stays"
    assert np.isneginf(out[1, 3]) and gone(1) == {0, 2, 4, 5, 7, 8}, "ab? after 'a': b or eos"
    assert gone(7) == set(range(9)) - {EOS}, "the finished row: eos only"
    keep = ~np.isneginf(out[[0, 1, 7], :vocab])
    assert np.array_equal(bits(out[[0, 1, 7], :vocab][keep]), bits(l[[0, 1, 7], :vocab][keep])), "an allowed logit keeps its bits"
    out2 = G.reference_mask(l, allows, gram, row_state, row_slot, ctr2, vocab=vocab)
    assert np.array_equal(bits(out2[1]), bits(l[1])) and np.array_equal(bits(out2[0]), bits(out[0])), "ctr < 0: inactive"
    assert np.array_equal(bits(G.reference_mask(l, allows, [-1] * 4, row_state, row_slot, ctr, vocab=vocab)), bits(l)), "no grammar anywhere"
