r"""Stop conditions on the device: stop strings, stop token ids, token budgets and the context limit, checked by one small launch at
the end of a step (C-ABI ``qpal_stop_advance`` / ``qpal_stop_mask``, csrc/stop.hip).

    table = grammar.TokenTable(token_bytes, eos=2)                  # the vocabulary's bytes
    bank = StopBank(B, table, device, sets=8, max_states=4096, cap=256)
    bank.load(0, [b"\n\n", b"</answer>"])                           # a stop set: a byte-level Aho-Corasick automaton
    bank.set(3, stop=0, stop_ids=(table.eos,), max_tokens=64)       # slot 3's criteria; stop=None: no strings
    bank.reset(3)                                                    # a new request in slot 3
    step = DecodeStep(..., stop=bank)                                # the LAST launch of the step judges out_tok and moves tok / pos
    for _ in range(n): graph.replay()                                # no host work: finished slots fall out (pos = -1)
    bank.result(3)                                                   # a host read, AFTER the run: tokens, reason, text, the string

A stop string matches on the BYTES of the generated text, across token boundaries: the rule is "the match that ends first, and of
those the longest", so the verdict depends on the bytes only — not on how they are cut into tokens, nor on whether the tokens come
one per step or several per speculative step.  The prompt is not walked and the stop string is not part of the answer.

The contracts are stated exactly (include/qpal.h) and restated here in numpy — ``compile_stops``, ``reference_stop_advance``,
``reference_stop_mask`` — and the kernels are held to them bit for bit.  That part is CPU only: numpy, no torch.cuda, no library call.
"""
from collections import namedtuple

import numpy as np

from .grammar import TokenTable

MAX_SLOTS, MAX_ROWS, MAX_WIDTH, MAX_SETS, MAX_IDS, MAX_STRINGS = 128, 128, 16, 256, 16, 64
MAX_STATES = 65535     # uint16 entries; every value is a state
RUNNING, STOP_ID, STOP_STRING, MAX_TOKENS, CONTEXT = 0, 1, 2, 3, 4
REASONS = ("running", "stop_id", "stop_string", "max_tokens", "context")

StopSet = namedtuple("StopSet", ["trans", "out_len", "strings"])
StopSet.__doc__ = """trans uint16 [S, 256] (every entry a state, failure links resolved), out_len uint16 [S] (the longest stop string
that ends at the state, 0: none), strings: the set's byte strings; state 0 is the start."""


# ---------------------------------------------------------------------------------------------------------------- the automaton

def compile_stops(strings, max_states=4096):
    """The byte-level Aho-Corasick automaton of 1 .. 64 non-empty byte strings, in dense form: the trie of the strings, numbered
    breadth first (bytes in order: the numbering is canonical), with every missing edge replaced by the edge of the longest proper
    suffix that has one.  The state after a text is then the longest suffix of the text that is a prefix of a string, and out_len of
    a state the longest string that is a suffix of it.  ValueError: not 1 .. 64 strings, an empty one, one longer than 65535 bytes,
    or more than max_states (at most 65535) states."""
    if not 1 <= int(max_states) <= MAX_STATES:
        raise ValueError(f"compile_stops: max_states must be in 1 .. {MAX_STATES}, got {max_states}")
    strs = [bytes(s) for s in strings]
    if not 1 <= len(strs) <= MAX_STRINGS:
        raise ValueError(f"compile_stops: a stop set has 1 .. {MAX_STRINGS} strings, got {len(strs)}")
    for s in strs:
        if not 1 <= len(s) <= 65535:
            raise ValueError(f"compile_stops: a stop string has 1 .. 65535 bytes, got {len(s)}")
    # ---- the trie (insertion order), then a breadth-first renumbering
    child, ends = [{}], [0]
    for s in strs:
        at = 0
        for c in s:
            if c not in child[at]:
                if len(child) >= max_states:
                    raise ValueError(f"compile_stops: the set needs more than max_states = {max_states} states")
                child[at][c] = len(child)
                child.append({})
                ends.append(0)
            at = child[at][c]
        ends[at] = len(s)   # (a state's depth: the one string that can end exactly here)
    order, number = [0], {0: 0}
    for at in order:
        for c in sorted(child[at]):
            number[child[at][c]] = len(order)
            order.append(child[at][c])
    S = len(order)
    trans = np.zeros((S, 256), np.uint16)
    out_len = np.zeros(S, np.uint16)
    fail = np.zeros(S, np.int64)
    for k, at in enumerate(order):   # breadth first: a state's failure state is complete before the state is reached
        if k:
            trans[k] = trans[fail[k]]
        out_len[k] = max(ends[at], int(out_len[fail[k]]) if k else 0)
        for c, nxt in child[at].items():
            n = number[nxt]
            fail[n] = trans[fail[k], c] if k else 0   # (read before the edge overwrites the inherited entry)
            trans[k, c] = n
    return StopSet(trans, out_len, tuple(strs))


# ---------------------------------------------------------------------------------------------------------------- contracts

class StopState:
    """The per-slot state of the contract as numpy arrays (what a StopBank holds on the device): set_id, ac_state, n_ids, max_tokens,
    min_tokens, n_gen, reason, hit int32 [B]; stop_ids int32 [B, id_slots]; gen_bytes, text_len, end_pos int64 [B]; out int64 [B, cap]."""

    FIELDS = ("set_id", "ac_state", "stop_ids", "n_ids", "max_tokens", "min_tokens", "n_gen", "gen_bytes", "out", "reason",
              "text_len", "hit", "end_pos")

    def __init__(self, B, cap=64, id_slots=MAX_IDS):
        i32, i64 = np.int32, np.int64
        self.set_id = np.full(B, -1, i32)
        self.stop_ids = np.full((B, id_slots), -1, i32)
        self.out = np.zeros((B, cap), i64)
        for name in ("ac_state", "n_ids", "max_tokens", "min_tokens", "n_gen", "reason", "hit"):
            setattr(self, name, np.zeros(B, i32))
        for name in ("gen_bytes", "text_len", "end_pos"):
            setattr(self, name, np.zeros(B, i64))

    def copy(self):
        new = StopState.__new__(StopState)
        for name in self.FIELDS:
            setattr(new, name, getattr(self, name).copy())
        return new

    def equal(self, other):
        """the names of the fields that differ (empty: bit for bit equal)"""
        return [n for n in self.FIELDS if not np.array_equal(getattr(self, n), np.asarray(getattr(other, n)))]


def _slot_set(sets, st, b):
    g = int(st.set_id[b])
    return sets[g] if 0 <= g < len(sets) else None


def judge(sets, table, st, b, t, next_pos, max_len):
    """The contract of ONE generated token t of slot b, in place on the StopState st: count and record it, stop ids (unless the token
    is exempt: n_gen < min_tokens), else the walk of its bytes through the slot's automaton — the first byte that lands in a state
    with out_len > 0 stops a token that is not exempt —, then max_tokens, then the context: next_pos, the position the token would
    be fed at, must lie below max_len.  Returns the reason (0: the slot goes on).  A slot without a set walks no automaton but still
    counts the bytes; a state or table entry outside the automaton is read as state 0."""
    t = int(t)
    n = int(st.n_gen[b]) + 1
    st.n_gen[b] = n
    if n <= st.out.shape[1]:
        st.out[b, n - 1] = t
    exempt = n < int(st.min_tokens[b])
    ids = st.stop_ids[b, :max(0, min(int(st.n_ids[b]), st.stop_ids.shape[1]))]
    reason = RUNNING
    if not exempt and any(int(i) == t for i in ids):
        reason = STOP_ID
        st.text_len[b] = st.gen_bytes[b]
    elif 0 <= t < table.vocab:
        o0, o1 = int(table.tok_off[t]), int(table.tok_off[t + 1])
        ss = _slot_set(sets, st, b)
        if ss is None:
            st.gen_bytes[b] += max(0, o1 - o0)
        else:
            S = ss.trans.shape[0]
            s = int(st.ac_state[b])
            s = s if 0 <= s < S else 0
            for c in table.tok_bytes[o0:o1]:
                s = int(ss.trans[s, c])
                s = s if s < S else 0
                st.gen_bytes[b] += 1
                if not exempt and ss.out_len[s] > 0:
                    reason = STOP_STRING
                    st.text_len[b] = int(st.gen_bytes[b]) - int(ss.out_len[s])
                    st.hit[b] = s
                    break
            st.ac_state[b] = s
    if reason == RUNNING and int(st.max_tokens[b]) > 0 and n >= int(st.max_tokens[b]):
        reason = MAX_TOKENS
        st.text_len[b] = st.gen_bytes[b]
    if reason == RUNNING and next_pos >= max_len:
        reason = CONTEXT
        st.text_len[b] = st.gen_bytes[b]
    if reason != RUNNING:
        st.reason[b] = reason
    return reason


def reference_stop_advance(sets, table, st, tokens, max_len, tok=None, pos=None, n_out=None, n_tok=None, limit=None):
    """The contract of qpal_stop_advance.  sets: a list of StopSet or None by set id; st: a StopState (not changed).

    Decode mode (tok and pos int [B], tokens int [B]): slot b is judged iff 0 <= pos[b] < max_len, with next_pos = pos[b] + 1.  A
    slot that finished gets end_pos[b] = pos[b] + 1 and pos[b] = -1; one that goes on tok[b] = tokens[b] and pos[b] += 1.
    Returns (state, tok, pos), copies.

    Speculative mode (n_out int [B], n_tok / limit int [B]: qpal_spec_accept's, after the accept; tokens int [B, width]): the first
    n_out[b] (clamped to width; 0: the slot is skipped) tokens are judged in order, token j with next_pos = n_tok[b] - n_out[b] + j.
    At the first one that finishes the slot: n_out[b] = j + 1, n_tok[b] -= old n_out - (j + 1), limit[b] = n_tok[b], end_pos[b] =
    n_tok[b] - 1.  Returns (state, n_out, n_tok, limit), copies."""
    st = st.copy()
    B = len(st.n_gen)
    max_len = int(max_len)
    if n_out is None:
        tokens = np.asarray(tokens, np.int64).reshape(B)
        tok, pos = np.array(tok, dtype=np.int64), np.array(pos, dtype=np.int64)
        for b in range(B):
            p = int(pos[b])
            if not 0 <= p < max_len:
                continue
            if judge(sets, table, st, b, tokens[b], p + 1, max_len) != RUNNING:
                st.end_pos[b] = p + 1
                pos[b] = -1
            else:
                tok[b], pos[b] = tokens[b], p + 1
        return st, tok, pos
    tokens = np.asarray(tokens, np.int64).reshape(B, -1)
    n_out = np.array(n_out, dtype=np.int32)
    n_tok, limit = np.array(n_tok, dtype=np.int64), np.array(limit, dtype=np.int64)
    for b in range(B):
        m = max(0, min(int(n_out[b]), tokens.shape[1]))
        base = int(n_tok[b]) - m
        for j in range(m):
            if judge(sets, table, st, b, tokens[b, j], base + j, max_len) != RUNNING:
                n_out[b] = j + 1
                n_tok[b] = base + j + 1
                limit[b] = n_tok[b]
                st.end_pos[b] = base + j
                break
    return st, n_out, n_tok, limit


def reference_stop_mask(logits, st, row_slot, ctr, row0=None, vocab=None):
    """The contract of qpal_stop_mask: a copy of logits fp32 [rows, >= vocab] in which row r of slot b = row_slot[r], the j-th row of
    its segment (j = r - row0[b]; row0 None: a decode step, j = 0), has -inf at every stop id of the slot that lies in [0, vocab)
    while n_gen[b] + j < min_tokens[b].  No other word differs.  A row is skipped when ctr[r] < 0, when b is outside the slots, or
    (row0 given) when row0[b] < 0 or j is outside 0 .. 15."""
    res = np.array(logits, dtype=np.float32)
    vocab = res.shape[1] if vocab is None else int(vocab)
    B = len(st.n_gen)
    for r in range(res.shape[0]):
        b = int(row_slot[r])
        if int(ctr[r]) < 0 or not 0 <= b < B:
            continue
        j = 0
        if row0 is not None:
            j = r - int(row0[b])
            if int(row0[b]) < 0 or not 0 <= j < MAX_WIDTH:
                continue
        if int(st.n_gen[b]) + j >= int(st.min_tokens[b]):
            continue
        for i in st.stop_ids[b, :max(0, min(int(st.n_ids[b]), st.stop_ids.shape[1]))]:
            if 0 <= int(i) < vocab:
                res[r, int(i)] = -np.inf
    return res


# ---------------------------------------------------------------------------------------------------------------- GPU side

def _torch():
    import torch
    return torch


class StopBank:
    """Up to `sets` stop sets of at most `max_states` states on the device, and the stop criteria and generation record of B slots:

        tok_off int32 [vocab + 1], tok_bytes uint8 [total]     the TokenTable
        trans   int16 [sets, max_states, 256] (the bits of a uint16), out_len int16 [sets, max_states] (likewise), n_states int32 [sets]
        set_id, ac_state, n_ids, max_tokens, min_tokens, n_gen, reason, hit int32 [B]; stop_ids int32 [B, id_slots];
        gen_bytes, text_len, end_pos int64 [B]; out int64 [B, cap]   (the fields of StopState)

    A new bank has no strings, no ids and no budget in any slot: a step with it stops a slot at the context limit only.  The setters
    are plain device writes between replays of a captured step, not part of one.  min_tokens=True: the steps built on the bank issue
    the mask launch that keeps the stop ids from being drawn before a slot's min_tokens (needs a sampler)."""

    def __init__(self, B, table, device, sets=8, max_states=4096, cap=256, id_slots=MAX_IDS, min_tokens=False):
        torch = _torch()
        from ._native import QpalError
        if not isinstance(table, TokenTable):
            raise QpalError("StopBank: table must be a grammar.TokenTable")
        if (not 1 <= int(B) <= MAX_SLOTS or not 1 <= int(sets) <= MAX_SETS or not 1 <= int(max_states) <= MAX_STATES
                or not 1 <= int(id_slots) <= MAX_IDS or int(cap) < 1):
            raise QpalError(f"StopBank: B in 1 .. {MAX_SLOTS}, sets in 1 .. {MAX_SETS}, max_states in 1 .. {MAX_STATES}, id_slots in "
                            f"1 .. {MAX_IDS} and cap >= 1, got {B}, {sets}, {max_states}, {id_slots}, {cap}")
        self.B, self.table, self.device = int(B), table, torch.device(device)
        self.vocab, self.sets, self.max_states, self.cap, self.id_slots = table.vocab, int(sets), int(max_states), int(cap), int(id_slots)
        self.min_tokens_mask = bool(min_tokens)
        dev, i32, i64 = self.device, torch.int32, torch.int64
        self.tok_off = torch.from_numpy(table.tok_off).to(dev)
        self.tok_bytes = torch.from_numpy(table.tok_bytes).to(dev)
        self.trans = torch.zeros(self.sets, self.max_states, 256, dtype=torch.int16, device=dev)
        self.out_len = torch.zeros(self.sets, self.max_states, dtype=torch.int16, device=dev)
        self.n_states = torch.zeros(self.sets, dtype=i32, device=dev)
        self.set_id = torch.full((self.B,), -1, dtype=i32, device=dev)
        self.stop_ids = torch.full((self.B, self.id_slots), -1, dtype=i32, device=dev)
        self.out = torch.zeros(self.B, self.cap, dtype=i64, device=dev)
        for name in ("ac_state", "n_ids", "max_tokens", "min_tokens", "n_gen", "reason", "hit"):
            setattr(self, name, torch.zeros(self.B, dtype=i32, device=dev))
        for name in ("gen_bytes", "text_len", "end_pos"):
            setattr(self, name, torch.zeros(self.B, dtype=i64, device=dev))
        self.stops = [None] * self.sets   # the host copies: what `result` and the callers' checks read
        self._slot_set = [None] * self.B
        self._struct = None

    def _slot(self, who, slot):
        from ._native import QpalError
        if not 0 <= int(slot) < self.B:
            raise QpalError(f"StopBank.{who}: slot {slot} outside 0 .. {self.B - 1}")
        return int(slot)

    def _set(self, who, i):
        from ._native import QpalError
        if not 0 <= int(i) < self.sets:
            raise QpalError(f"StopBank.{who}: stop set {i} outside 0 .. {self.sets - 1}")
        return int(i)

    def struct(self):
        """the qpal_stop_bank of the C-ABI (pointers into the bank's tensors, which live as long as the bank)"""
        from . import _native
        if self._struct is None:
            s = _native.StopBankStruct()
            for name in ("trans", "out_len", "n_states") + StopState.FIELDS:
                setattr(s, name, getattr(self, name).data_ptr())
            s.sets, s.max_states, s.id_slots, s.cap = self.sets, self.max_states, self.id_slots, self.cap
            self._struct = s
        return self._struct

    def load(self, i, strings):
        """stop set i = these byte strings (or a StopSet): compiled on the host and uploaded.  QpalError if the set is too large for
        the bank or a slot still uses i."""
        torch = _torch()
        from ._native import QpalError
        i = self._set("load", i)
        if i in self._slot_set:
            raise QpalError(f"StopBank.load: stop set {i} is in use by slot {self._slot_set.index(i)}: clear it first")
        try:
            ss = strings if isinstance(strings, StopSet) else compile_stops(strings, max_states=self.max_states)
        except ValueError as e:
            raise QpalError(f"StopBank.load: {e}") from None
        trans, out_len = np.ascontiguousarray(ss.trans), np.ascontiguousarray(ss.out_len)
        S = trans.shape[0]
        if (trans.dtype != np.uint16 or trans.shape != (S, 256) or out_len.dtype != np.uint16 or out_len.shape != (S,)
                or not 1 <= S <= self.max_states or int(trans.max()) >= S):
            raise QpalError(f"StopBank.load: trans uint16 [S, 256] with entries below S and out_len uint16 [S], 1 <= S <= "
                            f"{self.max_states}, got {trans.dtype} {list(trans.shape)}, {out_len.dtype} {list(out_len.shape)}")
        self.n_states[i] = 0   # until the tables are there no slot could follow them
        self.trans[i, :S] = torch.from_numpy(trans.view(np.int16)).to(self.device)
        self.out_len[i, :S] = torch.from_numpy(out_len.view(np.int16)).to(self.device)
        self.n_states[i] = S
        self.stops[i] = StopSet(trans, out_len, tuple(ss.strings))
        return self.stops[i]

    def unload(self, i):
        """stop set i is gone; slots using it must have been cleared first"""
        from ._native import QpalError
        i = self._set("unload", i)
        if i in self._slot_set:
            raise QpalError(f"StopBank.unload: stop set {i} is in use by slot {self._slot_set.index(i)}: clear it first")
        self.n_states[i] = 0
        self.stops[i] = None

    def set(self, slot, stop=None, stop_ids=None, max_tokens=0, min_tokens=0):
        """slot's criteria: stop = a loaded set or None (no strings); stop_ids: up to id_slots token ids (default: the table's eos);
        max_tokens: 0 = no bound; min_tokens: the tokens before which nothing but a budget ends the slot.  The automaton state goes
        back to the start; the record is left alone (`reset`)."""
        torch = _torch()
        from ._native import QpalError
        slot = self._slot("set", slot)
        if stop is not None:
            stop = self._set("set", stop)
            if self.stops[stop] is None:
                raise QpalError(f"StopBank.set: stop set {stop} is not loaded")
        ids = [self.table.eos] if stop_ids is None else [int(t) for t in stop_ids]
        if len(ids) > self.id_slots or any(not 0 <= t < self.vocab for t in ids):
            raise QpalError(f"StopBank.set: stop_ids must be at most {self.id_slots} token ids in 0 .. {self.vocab - 1}, got {ids}")
        max_tokens, min_tokens = int(max_tokens), int(min_tokens)
        if max_tokens < 0 or min_tokens < 0 or max(max_tokens, min_tokens) >= 1 << 31 or (max_tokens > 0 and min_tokens > max_tokens):
            raise QpalError(f"StopBank.set: max_tokens >= 0 (0: no bound) and 0 <= min_tokens <= max_tokens, got {max_tokens}, {min_tokens}")
        row = torch.full((self.id_slots,), -1, dtype=torch.int32)
        row[:len(ids)] = torch.tensor(ids, dtype=torch.int32)
        self.stop_ids[slot] = row.to(self.device)
        self.n_ids[slot], self.max_tokens[slot], self.min_tokens[slot] = len(ids), max_tokens, min_tokens
        self.ac_state[slot] = 0
        self.set_id[slot] = -1 if stop is None else stop
        self._slot_set[slot] = stop

    def reset(self, slot):
        """the slot at the start of a new request: nothing generated, the automaton at its start, running; its criteria stay"""
        slot = self._slot("reset", slot)
        for name in ("n_gen", "ac_state", "reason", "hit", "gen_bytes", "text_len", "end_pos"):
            getattr(self, name)[slot] = 0

    def state(self):
        """a host read: the slots' state as a StopState of numpy arrays"""
        st = StopState.__new__(StopState)
        for name in StopState.FIELDS:
            setattr(st, name, getattr(self, name).cpu().numpy())
        return st

    def put(self, st):
        """the slots' state from a StopState (tests and callers that restore a run)"""
        torch = _torch()
        for name in StopState.FIELDS:
            getattr(self, name).copy_(torch.from_numpy(np.ascontiguousarray(getattr(st, name))))

    def result(self, slot):
        """a host read, for AFTER a run of steps: a dict with tokens (the recorded ones, at most cap), n_gen, reason (a name of
        REASONS), text (the answer's bytes: the recorded tokens' bytes cut at text_len — a finishing stop id contributes none;
        complete only if n_gen <= cap), stop (the string that matched, or None) and end_pos."""
        slot = self._slot("result", slot)
        n, reason = int(self.n_gen[slot]), int(self.reason[slot])
        toks = self.out[slot, :min(n, self.cap)].cpu().tolist()
        body = toks[:-1] if reason == STOP_ID and n <= self.cap else toks
        text = b"".join(self.table.token(t) for t in body if 0 <= t < self.vocab)
        stop = None
        if reason != RUNNING:
            text = text[:int(self.text_len[slot])]
        if reason == STOP_STRING:
            ss, hit = self.stops[self._slot_set[slot]], int(self.hit[slot])
            want = int(ss.out_len[hit])
            stop = next(s for s in ss.strings if len(s) == want and _path(ss, hit).endswith(s))
        return dict(tokens=toks, n_gen=n, reason=REASONS[reason] if 0 <= reason < len(REASONS) else reason, text=text, stop=stop,
                    end_pos=int(self.end_pos[slot]))


def _path(ss, state):
    """the bytes that lead from the start to a state of a StopSet along the trie (the shortest text that reaches it)"""
    S = ss.trans.shape[0]
    prev = {0: None}
    queue = [0]
    for s in queue:   # breadth first over all edges: the first visit of a state comes along its trie path
        if s == state:
            break
        for c in range(256):
            n = int(ss.trans[s, c])
            if n not in prev and n < S:
                prev[n] = (s, c)
                queue.append(n)
    out = []
    while prev[state] is not None:
        state, c = prev[state]
        out.append(c)
    return bytes(reversed(out))


def _arr(t, name, dtype, shape, dev, who):
    from ._native import QpalError
    if not hasattr(t, "data_ptr") or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != dev:
        raise QpalError(f"{who}: {name} must be a contiguous {dtype} {list(shape)} tensor on {dev}")
    return t.data_ptr()


def _bank(bank, who):
    from ._native import QpalError
    if not isinstance(bank, StopBank):
        raise QpalError(f"{who}: bank must be a StopBank")
    if bank.device.type != "cuda":
        raise QpalError(f"{who}: the bank must live on a GPU, got {bank.device}")
    return bank


def stop_advance(bank, tokens, max_len, tok=None, pos=None, n_out=None, n_tok=None, limit=None):
    """The launch at the end of a step (the contract: include/qpal.h, reference_stop_advance), on all B slots of the bank.

    Decode mode: tokens int64 [B] (the step's out_tok), tok / pos int64 [B] — a slot with 0 <= pos[b] < max_len is judged; one that
    finished gets pos[b] = -1, one that goes on tok[b] = tokens[b], pos[b] += 1.
    Speculative mode: tokens int64 [B, width <= 16] (spec_accept's out_tok), n_out int32 [B], n_tok / limit int64 [B], all as the
    accept left them; n_out, n_tok and limit are cut in place where a slot finishes inside its run.
    One launch on the current stream; no host read."""
    torch = _torch()
    from . import _native
    who, QpalError = "stop.stop_advance", _native.QpalError
    bank, dev = _bank(bank, who), bank.device
    B = bank.B
    if int(max_len) < 1:
        raise QpalError(f"{who}: max_len must be at least 1, got {max_len}")
    spec = n_out is not None
    if spec:
        if tok is not None or pos is not None or n_tok is None or limit is None:
            raise QpalError(f"{who}: speculative mode takes n_out, n_tok and limit, and neither tok nor pos")
        if not hasattr(tokens, "dim") or tokens.dim() != 2 or not 1 <= tokens.shape[1] <= MAX_WIDTH:
            raise QpalError(f"{who}: tokens must be int64 [{B}, width <= {MAX_WIDTH}] in speculative mode")
        width = tokens.shape[1]
        tp = _arr(tokens, "tokens", torch.int64, (B, width), dev, who)
        ptrs = [_arr(n_out, "n_out", torch.int32, (B,), dev, who), _arr(n_tok, "n_tok", torch.int64, (B,), dev, who),
                _arr(limit, "limit", torch.int64, (B,), dev, who), None, None]
    else:
        if tok is None or pos is None or n_tok is not None or limit is not None:
            raise QpalError(f"{who}: decode mode takes tok and pos, and neither n_tok nor limit")
        width = 1
        tp = _arr(tokens, "tokens", torch.int64, (B,), dev, who)
        ptrs = [None, None, None, _arr(tok, "tok", torch.int64, (B,), dev, who), _arr(pos, "pos", torch.int64, (B,), dev, who)]
    with torch.cuda.device(dev):
        rc = _native.lib().qpal_stop_advance(bank.struct(), bank.tok_off.data_ptr(), bank.tok_bytes.data_ptr(), bank.vocab,
                                             bank.table.total, B, tp, width, *ptrs, int(max_len),
                                             torch.cuda.current_stream(dev).cuda_stream)
    _native.check(rc, "qpal_stop_advance")


def stop_mask(logits, bank, row_slot, ctr, row0=None):
    """In place on logits fp32 [rows, >= bank.vocab] (contiguous rows, 1 .. 128): the min_tokens mask in front of the draw (the
    contract: reference_stop_mask).  row_slot int32 [rows], ctr int64 [rows] (< 0: inactive), row0 int32 [B + 1] for a speculative
    step's segments (None: a decode step, every row the first of its slot).  One launch on the current stream; no host read.
    Returns logits."""
    torch = _torch()
    from . import _native
    who, QpalError = "stop.stop_mask", _native.QpalError
    bank, dev = _bank(bank, who), bank.device
    if (not hasattr(logits, "dim") or logits.dtype != torch.float32 or not logits.is_cuda or logits.dim() != 2
            or logits.stride(1) != 1):
        raise QpalError(f"{who}: logits must be an fp32 device tensor [rows, vocab] with contiguous rows")
    rows, vocab = logits.shape[0], bank.vocab
    ld = logits.stride(0) if rows > 1 else logits.shape[1]
    if not 1 <= rows <= MAX_ROWS or vocab > logits.shape[1] or ld < vocab or logits.device != dev:
        raise QpalError(f"{who}: logits must be 1 .. {MAX_ROWS} rows of {bank.vocab} logits on {dev}, got {list(logits.shape)} on "
                        f"{logits.device}")
    rs, cp = _arr(row_slot, "row_slot", torch.int32, (rows,), dev, who), _arr(ctr, "ctr", torch.int64, (rows,), dev, who)
    r0 = None if row0 is None else _arr(row0, "row0", torch.int32, (bank.B + 1,), dev, who)
    with torch.cuda.device(dev):
        rc = _native.lib().qpal_stop_mask(logits.data_ptr(), ld, rows, vocab, rs, cp, r0, bank.stop_ids.data_ptr(), bank.id_slots,
                                          bank.n_ids.data_ptr(), bank.min_tokens.data_ptr(), bank.n_gen.data_ptr(), bank.B,
                                          torch.cuda.current_stream(dev).cuda_stream)
    _native.check(rc, "qpal_stop_mask")
    return logits
