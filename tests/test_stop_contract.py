"""The stop contract on the CPU (numpy only): compile_stops against brute force, the judging rule against a brute-force walk over
random texts cut into tokens in several ways, and hand-made cases of every criterion and of both modes of reference_stop_advance."""
import numpy as np
import pytest

from qpalette_amd import stop as sp
from qpalette_amd.grammar import TokenTable

NESTED = [[b"bc", b"abcd"], [b"aa", b"aaa"], [b"abab", b"bab", b"b"], [b"a", b"b", b"c", b"d"], [b"dcba", b"cb", b"acbd"],
          [b"\x00\xff", b"\xff\xff\x00", b"ab\xff"]]


def _paths(ss):
    """the text of every state: the shortest bytes that reach it"""
    return [sp._path(ss, s) for s in range(ss.trans.shape[0])]


@pytest.mark.parametrize("strings", NESTED)
def test_compile_stops_matches_brute_force(strings):
    ss = sp.compile_stops(strings)
    S = ss.trans.shape[0]
    assert ss.trans.dtype == np.uint16 and ss.out_len.dtype == np.uint16 and ss.trans.shape == (S, 256) and ss.out_len.shape == (S,)
    assert int(ss.trans.max()) < S
    paths = _paths(ss)
    prefixes = {s[:i] for s in strings for i in range(len(s) + 1)}
    assert sorted(paths) == sorted(prefixes) and paths[0] == b""   # the states are the prefixes of the strings
    for s, text in enumerate(paths):
        want = max([len(x) for x in strings if text.endswith(x)], default=0)
        assert int(ss.out_len[s]) == want, (text, want)
        for c in (set(b"abcd\x00\xff") | {17}):   # the next state: the longest suffix of text + c that is a prefix
            nxt = text + bytes([c])
            best = max((nxt[i:] for i in range(len(nxt) + 1) if nxt[i:] in prefixes), key=len)
            assert paths[int(ss.trans[s, c])] == best


def test_compile_stops_errors():
    for bad in ([], [b""], [b"a", b""], [b"x"] * 65, [b"a" * 65536]):
        with pytest.raises(ValueError):
            sp.compile_stops(bad)
    with pytest.raises(ValueError):
        sp.compile_stops([b"abcdefgh"], max_states=8)     # needs 9 states
    assert sp.compile_stops([b"abcdefgh"], max_states=9).trans.shape[0] == 9
    for bad in (0, 65536):
        with pytest.raises(ValueError):
            sp.compile_stops([b"a"], max_states=bad)
    big = sp.compile_stops([bytes([i]) * 1000 for i in range(64)], max_states=65535)
    assert big.trans.shape[0] == 64001 and int(big.out_len.max()) == 1000


# ---------------------------------------------------------------------------------------------------------------- the judging rule

def _first_stop(text, strings):
    """brute force: the first prefix length e at which a stop string is a suffix of text[:e], and the longest such string"""
    for e in range(1, len(text) + 1):
        hits = [s for s in strings if text[:e].endswith(s)]
        if hits:
            return e, max(hits, key=len)
    return None, None


def _run_cut(ss, pieces, width=1):
    """the pieces as the tokens of one slot, `width` per launch in speculative mode (1: decode mode); returns the final state and the
    bytes that had been walked when the slot finished"""
    table = TokenTable(list(pieces) + [b""], eos=len(pieces))   # token i = piece i; the last token is an eos that never comes
    st = sp.StopState(1, cap=4)
    st.set_id[0] = 0
    if width == 1:
        tok, pos = np.zeros(1, np.int64), np.zeros(1, np.int64)
        for i in range(len(pieces)):
            st, tok, pos = sp.reference_stop_advance([ss], table, st, [i], 1 << 20, tok=tok, pos=pos)
            if st.reason[0]:
                assert pos[0] == -1 and st.end_pos[0] == i + 1
                break
            assert pos[0] == i + 1 and tok[0] == i
    else:
        n_tok, limit = np.array([1], np.int64), np.array([1 << 20], np.int64)
        for i in range(0, len(pieces), width):
            m = min(width, len(pieces) - i)
            toks = np.zeros((1, width), np.int64)
            toks[0, :m] = np.arange(i, i + m)
            st, n_out, n_tok2, limit = sp.reference_stop_advance([ss], table, st, toks, 1 << 20, n_out=[m], n_tok=n_tok + m, limit=limit)
            if st.reason[0]:
                assert limit[0] == n_tok2[0] == n_tok[0] + n_out[0] and 1 <= n_out[0] <= m and st.end_pos[0] == n_tok2[0] - 1
                break
            assert n_out[0] == m and n_tok2[0] == n_tok[0] + m
            n_tok = n_tok2
    return st


def _random_cut(rng, text):
    cuts = sorted(rng.choice(len(text) + 1, size=rng.integers(0, len(text) + 2), replace=True).tolist()) if len(text) else []
    edges = [0] + cuts + [len(text)]
    return [text[a:b] for a, b in zip(edges[:-1], edges[1:])]   # (empty pieces included: tokens without bytes)


def test_verdict_depends_on_the_bytes_only():
    rng = np.random.default_rng(5)
    sets = [[b"a"], [b"bc", b"abcd"], [b"aa", b"aaa"], [b"abab", b"bab"], [b"dd", b"cdd", b"a\xffb"], [b"abcabd", b"cab", b"ca"]]
    compiled = [sp.compile_stops(s) for s in sets]
    stopped = 0
    for k in range(2000):
        n = int(rng.integers(0, 21))
        raw = rng.integers(0, 4, size=n)
        text = bytearray(b"abcd"[v] for v in raw)
        for at in rng.integers(0, max(n, 1), size=int(rng.integers(0, 3))):   # a few bytes from anywhere
            if n:
                text[at] = int(rng.integers(0, 256))
        text = bytes(text)
        strings, ss = sets[k % len(sets)], compiled[k % len(sets)]
        e, longest = _first_stop(text, strings)
        stopped += e is not None
        runs = [(_random_cut(rng, text), 1), (_random_cut(rng, text), int(rng.integers(2, 6))), (_random_cut(rng, text), 16),
                ([text[i:i + 1] for i in range(n)], 1)]
        for pieces, width in runs:
            st = _run_cut(ss, pieces, width)
            if e is None:
                assert st.reason[0] == sp.RUNNING and st.gen_bytes[0] == n and st.n_gen[0] == len(pieces), (text, pieces)
                continue
            assert st.reason[0] == sp.STOP_STRING, (text, pieces, strings)
            assert st.gen_bytes[0] == e and st.text_len[0] == e - len(longest), (text, pieces, strings)
            assert sp._path(ss, int(st.hit[0])).endswith(longest) and int(ss.out_len[st.hit[0]]) == len(longest)
    assert 600 < stopped < 1900   # matches are common, and so are texts without one


# ---------------------------------------------------------------------------------------------------------------- hand-made cases

TOKS = [b"ab", b"c", b"", b"<eos>", b"dd", b"abcd", b"x"]   # ids 0 .. 6; eos = 3
TABLE = TokenTable(TOKS, eos=3)
SS = sp.compile_stops([b"bc", b"abcd"])


def _state(B=1, cap=8, **kw):
    st = sp.StopState(B, cap=cap)
    st.stop_ids[:, 0], st.n_ids[:] = 3, 1
    for name, v in kw.items():
        getattr(st, name)[:] = v
    return st


def _decode(st, toks, max_len=100, sets=(SS,), pos0=0):
    tok, pos = np.zeros(len(st.n_gen), np.int64), np.full(len(st.n_gen), pos0, np.int64)
    for t in toks:
        st, tok, pos = sp.reference_stop_advance(list(sets), TABLE, st, np.full(len(tok), t), max_len, tok=tok, pos=pos)
    return st, tok, pos


def test_stop_id_and_min_tokens():
    st, tok, pos = _decode(_state(), [0, 3, 6])
    assert (st.reason[0], st.n_gen[0], st.gen_bytes[0], st.text_len[0], st.end_pos[0], pos[0]) == (sp.STOP_ID, 2, 2, 2, 2, -1)
    assert st.out[0, :3].tolist() == [0, 3, 0] and tok[0] == 0       # the token behind the stop is never judged; tok keeps the last fed
    # inside min_tokens the id is an ordinary token: its bytes are walked and counted
    st, tok, pos = _decode(_state(min_tokens=3), [0, 3, 3, 6])
    assert (st.reason[0], st.n_gen[0], st.gen_bytes[0], st.text_len[0], pos[0]) == (sp.STOP_ID, 3, 7, 7, -1)
    # n_ids = 0: no id stops the slot; an id slot past n_ids is not an id
    st, _, pos = _decode(_state(n_ids=0), [3, 3])
    assert st.reason[0] == sp.RUNNING and pos[0] == 2


def test_exempt_match_is_ignored_for_good():
    # "ab" "c" completes "bc" in token 2, which is exempt (min_tokens 3): the walk goes on and the match never comes back
    st, _, pos = _decode(_state(set_id=0, min_tokens=3), [0, 1, 6, 6])
    assert st.reason[0] == sp.RUNNING and st.gen_bytes[0] == 5 and pos[0] == 4
    # the same text with min_tokens 2: token 2 is not exempt
    st, _, pos = _decode(_state(set_id=0, min_tokens=2), [0, 1, 6])
    assert (st.reason[0], st.text_len[0], st.gen_bytes[0], st.n_gen[0]) == (sp.STOP_STRING, 1, 3, 2)
    assert sp._path(SS, int(st.hit[0])) == b"abc"
    # an exempt token is walked to its end: "abcd" passes "bc" and ends in the state of "abcd", whose match is ignored as well
    st, _, _ = _decode(_state(set_id=0, min_tokens=2), [5])
    assert st.reason[0] == sp.RUNNING and st.gen_bytes[0] == 4 and sp._path(SS, int(st.ac_state[0])) == b"abcd"
    # not exempt: the first match ("bc" at byte 3) wins over the longer one that ends later, and the rest is not walked
    st, _, _ = _decode(_state(set_id=0), [5])
    assert (st.reason[0], st.gen_bytes[0], st.text_len[0]) == (sp.STOP_STRING, 3, 1)


def test_string_wins_over_max_tokens_and_context():
    st, _, _ = _decode(_state(set_id=0, max_tokens=2), [0, 1], max_len=2)
    assert (st.reason[0], st.text_len[0]) == (sp.STOP_STRING, 1)
    st, _, pos = _decode(_state(set_id=0, max_tokens=2), [0, 6], max_len=2)
    assert (st.reason[0], st.text_len[0], st.n_gen[0], pos[0]) == (sp.MAX_TOKENS, 3, 2, -1)
    st, _, pos = _decode(_state(max_tokens=2), [0, 3])
    assert st.reason[0] == sp.STOP_ID


def test_context_rule_and_inactive_slots():
    st, tok, pos = _decode(_state(), [0, 1, 6], max_len=3, pos0=1)   # fed at 1, 2: the second token would be fed at 3
    assert (st.reason[0], st.n_gen[0], st.end_pos[0], pos[0], st.text_len[0]) == (sp.CONTEXT, 2, 3, -1, 3)
    for p in (-1, 3, 1 << 40):                                        # outside the cache: nothing of the slot changes
        st0 = _state()
        st, tok, pos = _decode(st0, [0], max_len=3, pos0=p)
        assert not st.equal(st0) and pos[0] == p and tok[0] == 0


def test_cap_overflow_empty_and_foreign_tokens():
    st, _, pos = _decode(_state(cap=2, set_id=0), [6, 2, 300, -5, 6, 1 << 40])
    assert st.n_gen[0] == 6 and st.out[0].tolist() == [6, 2] and st.gen_bytes[0] == 2 and st.reason[0] == sp.RUNNING and pos[0] == 6
    # an empty or foreign token between "ab" and "c" does not break the match: it has no bytes
    st, _, _ = _decode(_state(set_id=0), [0, 2, 999, 1])
    assert (st.reason[0], st.n_gen[0], st.text_len[0]) == (sp.STOP_STRING, 4, 1)
    # a slot without a set counts bytes and walks nothing; a set id that names no set is no set
    for sid in (-1, 1, 77):
        st, _, _ = _decode(_state(set_id=sid), [0, 1], sets=(SS, None))
        assert st.reason[0] == sp.RUNNING and st.gen_bytes[0] == 3 and st.ac_state[0] == 0


def test_speculative_mode_cuts_the_run():
    toks = np.array([[6, 0, 1, 6, 6]])                      # x ab c x x: "bc" ends in token 2
    for first, n_out, want in ((6, 5, 3), (0, 4, 2), (1, 3, 1)):   # the stop at the end, in the middle, at token 0 of a run
        st = _state(set_id=0)
        lead = [6, 0, 1].index(first) if first != 6 else 0
        run = np.zeros((1, 5), np.int64)
        run[0, :5 - lead] = toks[0, lead:]
        if lead:                                             # the tokens in front of the run came in an earlier step
            st, _, n_tok, _ = sp.reference_stop_advance([SS], TABLE, st, np.array([list(toks[0, :lead]) + [0] * (5 - lead)]), 100,
                                                        n_out=[lead], n_tok=[10 + lead], limit=[50])
            assert st.reason[0] == sp.RUNNING and n_tok[0] == 10 + lead
        st, n, n_tok, limit = sp.reference_stop_advance([SS], TABLE, st, run, 100, n_out=[n_out], n_tok=[10 + lead + n_out], limit=[50])
        assert (st.reason[0], n[0], n_tok[0], limit[0]) == (sp.STOP_STRING, want, 10 + lead + want, 10 + lead + want)
        assert (st.n_gen[0], st.text_len[0], st.gen_bytes[0], st.end_pos[0]) == (3, 2, 4, 10 + lead + want - 1)
        assert st.out[0, :3].tolist() == [6, 0, 1]
    # a run that does not finish leaves n_out / n_tok / limit alone; n_out == 0 skips the slot; n_out is clamped to the width
    st0 = _state(B=3, set_id=0)
    run = np.array([[6, 6, 6], [0, 1, 6], [6, 6, 6]])
    st, n, n_tok, limit = sp.reference_stop_advance([SS], TABLE, st0, run, 100, n_out=[2, 0, 9], n_tok=[12, 7, 20], limit=[50, 7, 60])
    assert n.tolist() == [2, 0, 9] and n_tok.tolist() == [12, 7, 20] and limit.tolist() == [50, 7, 60]
    assert st.n_gen.tolist() == [2, 0, 3] and st.reason.tolist() == [0, 0, 0] and st.gen_bytes.tolist() == [2, 0, 3]
    # the context rule uses n_tok: token j of the run would be fed at n_tok - n_out + j
    st, n, n_tok, limit = sp.reference_stop_advance([SS], TABLE, _state(), np.array([[6, 6, 6]]), 12, n_out=[3], n_tok=[14], limit=[50])
    assert (st.reason[0], n[0], n_tok[0], limit[0], st.end_pos[0]) == (sp.CONTEXT, 2, 13, 13, 12)


def test_stop_mask_contract():
    st = _state(B=3, min_tokens=[0, 2, 5], n_gen=[0, 1, 1])
    st.stop_ids[2, :3], st.n_ids[2] = [3, 6, 400], 3
    logits = np.arange(4 * 8, dtype=np.float32).reshape(4, 8)
    out = sp.reference_stop_mask(logits, st, [0, 1, 2, 2], [5, 5, 5, -1], vocab=7)
    want = logits.copy()
    want[1, 3] = want[2, 3] = want[2, 6] = -np.inf     # slot 0 has no bound, row 3 is inactive, id 400 is no token
    assert np.array_equal(out, want)
    # speculative rows: row j of a segment is the j-th token from now
    row0 = [0, 0, 1, 8]
    out = sp.reference_stop_mask(np.zeros((8, 8), np.float32), st, [1, 2, 2, 2, 2, 2, 2, 2], np.arange(8), row0=row0, vocab=7)
    assert np.isinf(out[:, 3]).tolist() == [True, True, True, True, True, False, False, False]   # slot 2: 1 + j < 5 for j < 4
    assert np.isinf(out[:, 6]).tolist() == [False, True, True, True, True, False, False, False]
