r"""Grammar-constrained decoding: a byte-level deterministic automaton per slot, compiled from a regular expression on the host,
turned into per-state token bitmasks on the GPU when it is loaded and followed there by three small launches in the steps' tails
(C-ABI ``qpal_grammar_compile / rows / mask / advance``, csrc/grammar.hip).

    dfa = compile_regex(r"-?(0|[1-9]\d*)(\.\d+)?")                # ByteDFA: trans uint16 [S, 256], accept uint8 [S]
    table = TokenTable(token_bytes, eos=2)                          # the vocabulary's bytes
    bank = GrammarBank(B, table, device, grammars=8, max_states=4096)
    bank.load(0, dfa)                                               # upload + compile launch + one read of the table (load time)
    bank.set(3, 0)                                                  # slot 3 follows grammar 0 from its start; None: no grammar
    DecodeStep(..., sampler=smp, grammar=bank)                      # mask in front of the draw, advance behind it: no host read
    bank.matched(3)                                                 # a host read, for callers and tests

The grammar constrains generated tokens only: a prompt is not walked.  Once eos has been emitted the slot is FINISHED and only eos
may follow.  A captured step reads gram / state when it runs: `set` / `reset` between replays change the next draw.

The contracts are stated exactly (include/qpal.h) and restated here in numpy — ``reference_allow``, ``reference_step``,
``reference_rows``, ``reference_mask``, ``reference_advance`` — and the kernels are held to them bit for bit.  That part, and the
regex compiler, is CPU only: numpy, no torch.cuda, no library call.
"""
from collections import namedtuple

import numpy as np

DEAD = 0xFFFF          # trans: no transition
DEAD_STATE = -1        # a slot's state: the text so far can never match
MAX_STATES = 65534     # hard limit of an automaton (uint16 entries, 0xFFFF taken)
MAX_SLOTS, MAX_ROWS, MAX_WIDTH, MAX_GRAMMARS = 128, 128, 16, 1024
_WORK_STATES = 1 << 18  # subset construction and NFA size before minimisation: beyond this the pattern is refused
_MAX_REPEAT = 1 << 16

ByteDFA = namedtuple("ByteDFA", ["trans", "accept"])
ByteDFA.__doc__ = """trans uint16 [S, 256] (DEAD: no transition), accept uint8 [S]; state 0 is the start.  Full-match, minimal, trimmed."""


# ---------------------------------------------------------------------------------------------------------------- regex -> DFA

_ALL = (1 << 256) - 1


def _set(*bytes_):
    m = 0
    for b in bytes_:
        m |= 1 << b
    return m


def _range(lo, hi):
    return ((1 << (hi + 1)) - 1) & ~((1 << lo) - 1)


_DIGIT = _range(0x30, 0x39)
_WORD = _DIGIT | _range(0x41, 0x5A) | _range(0x61, 0x7A) | _set(0x5F)
_SPACE = _set(0x20, 0x09, 0x0A, 0x0D, 0x0C, 0x0B)
_SHORT = {"d": _DIGIT, "D": _ALL & ~_DIGIT, "w": _WORD, "W": _ALL & ~_WORD, "s": _SPACE, "S": _ALL & ~_SPACE}
_CTRL = {"n": 0x0A, "r": 0x0D, "t": 0x09}


class _Parser:
    """pattern -> a tree of ("set", mask) | ("cat", [..]) | ("alt", [..]) | ("rep", node, lo, hi or None) | ("empty",)"""

    def __init__(self, pattern):
        if not isinstance(pattern, str):
            raise ValueError("compile_regex: the pattern must be a str")
        self.p, self.i = pattern, 0

    def fail(self, what, at=None):
        raise ValueError(f"compile_regex: {what} at position {self.i if at is None else at} of {self.p!r}")

    def peek(self):
        return self.p[self.i] if self.i < len(self.p) else ""

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.fail("unbalanced ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.i < len(self.p) and self.peek() not in "|)":
            items.append(self.quantified())
        if not items:
            return ("empty",)
        return items[0] if len(items) == 1 else ("cat", items)

    def quantified(self):
        at = self.i
        c = self.peek()
        if c in "*+?":
            self.fail("nothing to repeat")
        if c == "{":
            self.fail("'{' without an atom in front (write \\{ for the character)")
        node = self.atom()
        c = self.peek()
        lo = hi = None
        if c == "*":
            lo, hi = 0, None
        elif c == "+":
            lo, hi = 1, None
        elif c == "?":
            lo, hi = 0, 1
        elif c == "{":
            lo, hi = self.braces()
        else:
            return node
        if c != "{":
            self.i += 1
        nxt = self.peek()
        if nxt == "?":
            self.fail("lazy quantifiers are not supported")
        if nxt == "+":
            self.fail("possessive quantifiers are not supported")
        if nxt in ("*", "{"):
            self.fail("multiple repeat")
        if hi is not None and hi < lo:
            self.fail("repeat with max below min", at)
        if max(lo, hi or 0) > _MAX_REPEAT:
            self.fail(f"repeat count above {_MAX_REPEAT}", at)
        return ("rep", node, lo, hi)

    def braces(self):
        """{m} {m,} {m,n} at self.i; leaves self.i behind the '}'"""
        end = self.p.find("}", self.i)
        body = self.p[self.i + 1:end] if end > 0 else ""
        parts = body.split(",")
        if end < 0 or len(parts) > 2 or not parts[0].isascii() or not parts[0].isdigit() or (
                len(parts) == 2 and parts[1] != "" and not (parts[1].isascii() and parts[1].isdigit())):
            self.fail("'{' that opens no {m}, {m,} or {m,n} (write \\{ for the character)")
        self.i = end + 1
        lo = int(parts[0])
        if len(parts) == 1:
            return lo, lo
        return lo, (None if parts[1] == "" else int(parts[1]))

    def escape(self):
        """the escape at self.i (behind the backslash): ("set", mask) for a shorthand, else a byte value"""
        c = self.peek()
        if c == "":
            self.fail("a pattern cannot end in a backslash")
        self.i += 1
        if c in _SHORT:
            return ("set", _SHORT[c])
        if c in _CTRL:
            return _CTRL[c]
        if c == "x":
            h = self.p[self.i:self.i + 2]
            if len(h) != 2 or any(d not in "0123456789abcdefABCDEF" for d in h):
                self.fail("\\x needs two hex digits", self.i - 2)
            self.i += 2
            return int(h, 16)
        if c.isascii() and not c.isalnum():   # an escaped metacharacter or other punctuation: itself
            return ord(c)
        self.fail(f"unsupported escape \\{c} (anchors, backreferences and other escapes are not in the subset)", self.i - 2)

    def atom(self):
        at = self.i
        c = self.peek()
        self.i += 1
        if c == "(":
            if self.peek() == "?":
                if self.p[self.i:self.i + 2] != "?:":
                    self.fail("only (?: ) groups are supported (no flags, names or lookaround)", at)
                self.i += 2
            node = self.alt()
            if self.peek() != ")":
                self.fail("missing ')'", at)
            self.i += 1
            return node
        if c == "[":
            return self.klass(at)
        if c == ".":
            return ("set", _ALL & ~_set(0x0A))
        if c == "\\":
            e = self.escape()
            return e if isinstance(e, tuple) else ("set", _set(e))
        if c in "^$":
            self.fail("anchors are not supported (the automaton is a full match)", at)
        if c in "]}":
            self.fail(f"unescaped {c!r} (write \\{c} for the character)", at)
        if ord(c) < 128:
            return ("set", _set(ord(c)))
        return ("cat", [("set", _set(b)) for b in c.encode("utf-8")])  # a non-ASCII character: its UTF-8 bytes as one group

    def klass(self, at):
        negate = self.peek() == "^"
        if negate:
            self.i += 1
        mask, first = 0, True
        while True:
            c = self.peek()
            if c == "":
                self.fail("missing ']'", at)
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            lo = self.class_item()
            if isinstance(lo, tuple):
                mask |= lo[1]
                continue
            if self.peek() == "-" and self.p[self.i + 1:self.i + 2] not in ("]", ""):
                self.i += 1
                hi = self.class_item()
                if isinstance(hi, tuple):
                    self.fail("a class shorthand cannot end a range")
                if hi < lo:
                    self.fail("bad character range")
                mask |= _range(lo, hi)
            else:
                mask |= _set(lo)
        return ("set", (_ALL & ~mask) if negate else mask)

    def class_item(self):
        c = self.peek()
        self.i += 1
        if c == "\\":
            return self.escape()
        if c == "[" and self.peek() == ":":
            self.fail("POSIX classes are not supported", self.i - 1)
        if ord(c) >= 128:
            self.fail("a non-ASCII character inside a class (bytes have no such member; write an alternation)", self.i - 1)
        return ord(c)


class _NFA:
    def __init__(self):
        self.eps, self.edges = [], []   # per state: epsilon targets; (mask, target) pairs

    def new(self):
        if len(self.eps) >= _WORK_STATES:
            raise ValueError(f"compile_regex: the pattern needs more than {_WORK_STATES} working states")
        self.eps.append([])
        self.edges.append([])
        return len(self.eps) - 1

    def build(self, node):
        """(start, end) of a fragment for the tree `node`"""
        kind = node[0]
        if kind == "empty":
            s = self.new()
            return s, s
        if kind == "set":
            s, e = self.new(), self.new()
            self.edges[s].append((node[1], e))
            return s, e
        if kind == "cat":
            s, e = self.build(node[1][0])
            for sub in node[1][1:]:
                s2, e2 = self.build(sub)
                self.eps[e].append(s2)
                e = e2
            return s, e
        if kind == "alt":
            s, e = self.new(), self.new()
            for sub in node[1]:
                s2, e2 = self.build(sub)
                self.eps[s].append(s2)
                self.eps[e2].append(e)
            return s, e
        _, sub, lo, hi = node
        s = e = self.new()
        for _ in range(lo):
            s2, e2 = self.build(sub)
            self.eps[e].append(s2)
            e = e2
        if hi is None:      # a loop behind the required copies
            s2, e2 = self.build(sub)
            hub = self.new()
            self.eps[e].append(hub)
            self.eps[hub].append(s2)
            self.eps[e2].append(hub)
            e = hub
        else:               # hi - lo optional copies, each may leave to the end
            end = self.new()
            for _ in range(hi - lo):
                s2, e2 = self.build(sub)
                self.eps[e].append(end)
                self.eps[e].append(s2)
                e = e2
            self.eps[e].append(end)
            e = end
        return s, e


def _byte_classes(masks):
    """the coarsest partition of 0 .. 255 in which every mask is a union of blocks: (class of each byte [256], one byte per class)"""
    blocks = [_ALL]
    for m in masks:
        nxt = []
        for b in blocks:
            for part in (b & m, b & ~m):
                if part:
                    nxt.append(part)
        blocks = nxt
    cls = np.zeros(256, np.int64)
    reps = []
    for k, b in enumerate(blocks):
        members = [i for i in range(256) if (b >> i) & 1]
        cls[members] = k
        reps.append(members[0])
    return cls, reps


def compile_regex(pattern, max_states=4096):
    """The full-match automaton over BYTES of `pattern`, determinised, minimised and trimmed: every state is reachable from state 0
    and can reach an accepting state, so a byte that leads nowhere useful is DEAD at once.  The subset — literals, the escapes
    \\d \\D \\w \\W \\s \\S \\n \\r \\t \\\\ \\xHH and escaped punctuation, `.` (any byte but \\n), classes with ranges, ( ) and
    (?: ), |, * + ?, {m} {m,} {m,n} — means what Python's `re` gives the same pattern compiled as a bytes pattern with fullmatch.  A
    non-ASCII character outside a class is its UTF-8 bytes as one group.  Anything else — anchors, backreferences, lookaround, lazy
    or possessive quantifiers, flags, named groups — raises ValueError naming the position, as does a pattern that matches nothing
    or whose automaton needs more than max_states (default 4096, at most 65 534) states."""
    if not 1 <= int(max_states) <= MAX_STATES:
        raise ValueError(f"compile_regex: max_states must be in 1 .. {MAX_STATES}, got {max_states}")
    max_states = int(max_states)
    tree = _Parser(pattern).parse()
    nfa = _NFA()
    start, final = nfa.build(tree)
    cls, reps = _byte_classes(sorted({m for es in nfa.edges for m, _ in es}))
    C = len(reps)

    def closure(states):
        seen, stack = set(states), list(states)
        while stack:
            for t in nfa.eps[stack.pop()]:
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        return frozenset(seen)

    # ---- subset construction over the byte classes
    first = closure([start])
    index, order, rows = {first: 0}, [first], []
    while len(rows) < len(order):
        cur = order[len(rows)]
        row = []
        for c in range(C):
            bit = 1 << reps[c]
            to = {t for s in cur for m, t in nfa.edges[s] if m & bit}
            if not to:
                row.append(-1)
                continue
            nxt = closure(to)
            if nxt not in index:
                if len(order) >= _WORK_STATES:
                    raise ValueError(f"compile_regex: {pattern!r} needs more than {_WORK_STATES} states before minimisation")
                index[nxt] = len(order)
                order.append(nxt)
            row.append(index[nxt])
        rows.append(row)
    n = len(order)
    t = np.array(rows, np.int64).reshape(n, C)
    acc = np.array([final in s for s in order], bool)
    # ---- trim: states that reach no accepting state become "no transition" (everything is reachable by construction)
    live = acc.copy()
    while True:
        grown = live | (np.where(t >= 0, live[np.maximum(t, 0)], False)).any(axis=1)
        if np.array_equal(grown, live):
            break
        live = grown
    if not live[0]:
        raise ValueError(f"compile_regex: {pattern!r} matches nothing")
    t = np.where((t >= 0) & live[np.maximum(t, 0)], t, n)      # n: the sink
    t = np.concatenate([t, np.full((1, C), n, np.int64)])
    t[~np.append(live, False)] = n
    # ---- minimise (Moore): refine {accepting, other live, sink / dead} until the blocks' successor blocks agree
    block = np.where(np.append(live, False), np.append(acc, False).astype(np.int64), 2)
    while True:
        sig = np.concatenate([block[:, None], block[t]], axis=1)
        _, new = np.unique(sig, axis=0, return_inverse=True)
        new = new.reshape(-1)
        if len(np.unique(new)) == len(np.unique(block)):
            block = new
            break
        block = new
    sink = int(block[n])
    # ---- renumber breadth first from the start, bytes in order: state 0 is the start, the numbering is canonical
    rep_of = {}
    for s in range(n):
        rep_of.setdefault(int(block[s]), s)
    number, queue = {int(block[0]): 0}, [int(block[0])]
    out_rows = []
    while len(out_rows) < len(queue):
        b = queue[len(out_rows)]
        row = []
        for c in range(C):
            nb = int(block[t[rep_of[b], c]])
            if nb == sink:
                row.append(DEAD)
                continue
            if nb not in number:
                number[nb] = len(queue)
                queue.append(nb)
            row.append(number[nb])
        out_rows.append(row)
    S = len(queue)
    if S > max_states:
        raise ValueError(f"compile_regex: {pattern!r} needs {S} states, more than max_states = {max_states}")
    small = np.array(out_rows, np.uint16).reshape(S, C)
    trans = np.ascontiguousarray(small[:, cls])
    accept = np.array([acc[rep_of[b]] for b in queue], np.uint8)
    return ByteDFA(trans, accept)


def dfa_match(dfa, data):
    """True if the automaton accepts the bytes `data` (the host walk: tests and callers)"""
    s = 0
    for b in bytes(data):
        s = int(dfa.trans[s, b])
        if s == DEAD:
            return False
    return bool(dfa.accept[s])


def dfa_live_prefix(dfa, data):
    """the state after the bytes `data` from the start, or None if no text that begins with them can match"""
    s = 0
    for b in bytes(data):
        s = int(dfa.trans[s, b])
        if s == DEAD:
            return None
    return s


# ---------------------------------------------------------------------------------------------------------------- vocabulary

class TokenTable:
    """The vocabulary's bytes: tok_off int32 [vocab + 1], tok_bytes uint8 [total] (one zero byte where the vocabulary has none, so
    that it can live on a device).  A token with no bytes — a special token — is never allowed by a grammar.  eos: the token id that
    ends a text; a grammar allows it exactly in accepting states, whatever bytes it has."""

    def __init__(self, token_bytes, eos):
        toks = [bytes(t) for t in token_bytes]
        self.vocab = len(toks)
        if not 1 <= self.vocab <= 1 << 30:
            raise ValueError("TokenTable: a vocabulary of 1 .. 2^30 tokens")
        if eos is None or not 0 <= int(eos) < self.vocab:
            raise ValueError(f"TokenTable: eos must be a token id in 0 .. {self.vocab - 1}, got {eos}")
        self.eos = int(eos)
        lens = np.array([len(t) for t in toks], np.int64)
        if int(lens.sum()) >= 1 << 31:
            raise ValueError("TokenTable: the tokens' bytes must stay below 2^31")
        self.tok_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        self.total = int(self.tok_off[-1])
        self.tok_bytes = np.frombuffer(b"".join(toks) or b"\0", dtype=np.uint8).copy()

    def token(self, t):
        return self.tok_bytes[self.tok_off[t]:self.tok_off[t + 1]].tobytes() if self.total else b""

    def text(self, tokens):
        """the bytes of a token sequence, eos left out"""
        return b"".join(self.token(int(t)) for t in tokens if int(t) != self.eos)


# ---------------------------------------------------------------------------------------------------------------- contracts

def reference_step(dfa, table, state, token):
    """The contract of one token: from a state in 0 .. S - 1, eos gives S (FINISHED) if the state accepts, else DEAD_STATE; any other
    token follows its bytes — a token outside [0, vocab), an empty token or a dead walk gives DEAD_STATE.  From S: eos gives S,
    anything else DEAD_STATE.  DEAD_STATE (and any value outside -1 .. S) stays DEAD_STATE."""
    S, s, t = dfa.trans.shape[0], int(state), int(token)
    if s < 0 or s > S:
        return DEAD_STATE
    if s == S:
        return S if t == table.eos else DEAD_STATE
    if t == table.eos:
        return S if dfa.accept[s] else DEAD_STATE
    if not 0 <= t < table.vocab:
        return DEAD_STATE
    o0, o1 = int(table.tok_off[t]), int(table.tok_off[t + 1])
    if o1 <= o0:
        return DEAD_STATE
    for b in table.tok_bytes[o0:o1]:
        s = int(dfa.trans[s, b])
        if s >= S:
            return DEAD_STATE
    return s


def reference_allow(dfa, table):
    """The contract of qpal_grammar_compile: uint32 [S + 1, ceil(vocab / 32)], mask_bits' layout.  Bit t of row s < S is set iff
    token t != eos has at least one byte and walking its bytes from s never meets DEAD; bit eos of row s iff accept[s]; row S, the
    FINISHED state, has the eos bit only."""
    S, V = dfa.trans.shape[0], table.vocab
    lens = np.diff(table.tok_off.astype(np.int64))
    longest = int(lens.max())
    pad = np.zeros((V, max(longest, 1)), np.int64)   # byte p of token t
    for p in range(longest):
        has = lens > p
        pad[has, p] = table.tok_bytes[table.tok_off[:-1][has].astype(np.int64) + p]
    ext = np.concatenate([dfa.trans.astype(np.int64), np.full((1, 256), DEAD, np.int64)])
    ext[ext >= S] = S                                 # row S of ext: the dead sink
    ok = np.zeros((S + 1, V), bool)
    chunk = max(1, (1 << 22) // V)
    for s0 in range(0, S, chunk):
        cur = np.repeat(np.arange(s0, min(S, s0 + chunk))[:, None], V, axis=1)
        for p in range(longest):
            has = lens > p
            cur[:, has] = ext[cur[:, has], pad[has, p][None, :]]
        ok[s0:s0 + cur.shape[0]] = (cur < S) & (lens > 0)[None, :]
    ok[:S, table.eos] = dfa.accept != 0
    ok[S, table.eos] = True
    words = (V + 31) // 32
    bits = np.zeros((S + 1, words * 32), bool)
    bits[:, :V] = ok
    weights = (np.uint64(1) << np.arange(32, dtype=np.uint64))
    return (bits.reshape(S + 1, words, 32).astype(np.uint64) * weights).sum(axis=2).astype(np.uint32)


def _slot_dfa(grammars, gram, b):
    g = int(gram[b])
    return grammars[g] if 0 <= g < len(grammars) else None


def reference_rows(grammars, table, gram, state, tokens, row0, rows):
    """The contract of qpal_grammar_rows.  grammars: a list of ByteDFA or None by grammar id; gram, state int [slots]; tokens int
    [rows] and row0 int [slots + 1]: a speculative step's segments.  Returns row_state int32 [rows]: DEAD_STATE everywhere, except
    that for a slot with a grammar, a segment of 1 .. 16 rows inside [0, rows) and a state in 0 .. S, row first + j holds the state
    after the j guessed tokens in front of it (the pending token at `first` is already in state[b])."""
    out = np.full(int(rows), DEAD_STATE, np.int32)
    for b in range(len(gram)):
        dfa = _slot_dfa(grammars, gram, b)
        first, end = int(row0[b]), int(row0[b + 1])
        if dfa is None or first < 0 or end > rows or not 1 <= end - first <= MAX_WIDTH:
            continue
        s = int(state[b])
        if not 0 <= s <= dfa.trans.shape[0]:
            continue
        out[first] = s
        for r in range(first + 1, end):
            s = reference_step(dfa, table, s, tokens[r])
            if s == DEAD_STATE:
                break
            out[r] = s
    return out


def reference_advance(grammars, table, gram, state, tokens, n=None, active=None):
    """The contract of qpal_grammar_advance: a copy of state int32 [slots] with state[b] = step(.. step(state[b], tokens[b][0]) ..,
    tokens[b][m - 1]), m = n[b] clamped to 0 .. width (n None: width).  A slot without a grammar, with active[b] < 0 or with m = 0
    keeps its state."""
    out = np.array(state, dtype=np.int32)
    tokens = np.asarray(tokens, dtype=np.int64).reshape(len(out), -1)
    for b in range(len(out)):
        dfa = _slot_dfa(grammars, gram, b)
        m = tokens.shape[1] if n is None else max(0, min(tokens.shape[1], int(n[b])))
        if dfa is None or m == 0 or (active is not None and int(active[b]) < 0):
            continue
        s = int(out[b])
        for i in range(m):
            s = reference_step(dfa, table, s, tokens[b, i])
        out[b] = s
    return out


def reference_mask(logits, allows, gram, row_state, row_slot, ctr, vocab=None):
    """The contract of qpal_grammar_mask.  logits fp32 [rows, >= vocab]; allows: a list by grammar id of reference_allow tables (or
    None); gram int [slots]; row_state, row_slot, ctr int [rows].  Returns a copy with, in every row that is active (ctr >= 0), whose
    slot lies in [0, slots) and has a grammar, and whose row state lies in 0 .. S, -inf wherever the state's bit is clear; no other
    bit differs (a skipped row keeps every bit; columns past vocab are kept)."""
    res = np.array(logits, dtype=np.float32)
    vocab = res.shape[1] if vocab is None else int(vocab)
    idx = np.arange(vocab)
    for r in range(res.shape[0]):
        b = int(row_slot[r])
        if int(ctr[r]) < 0 or not 0 <= b < len(gram):
            continue
        g = int(gram[b])
        allow = allows[g] if 0 <= g < len(allows) else None
        s = int(row_state[r])
        if allow is None or not 0 <= s < allow.shape[0]:
            continue
        bit = (np.ascontiguousarray(allow[s]).view(np.uint32)[idx >> 5] >> (idx & 31).astype(np.uint32)) & np.uint32(1)
        res[r, :vocab][bit == 0] = -np.inf
    return res


# ---------------------------------------------------------------------------------------------------------------- GPU side

def _torch():
    import torch
    return torch


class GrammarBank:
    """Up to `grammars` automata of at most `max_states` states on the device, and which of them each of B slots follows:

        tok_off int32 [vocab + 1], tok_bytes uint8 [total]     the TokenTable
        trans   int16 [grammars, max_states, 256] (the bits of a uint16), accept uint8 [grammars, max_states], n_states int32 [grammars]
        allow   int32 [grammars, max_states + 1, ceil(vocab / 32)] (the bits of a uint32): grammars * (max_states + 1) * ceil(vocab
                / 32) * 4 bytes — 526 MB at the defaults (8, 4096) and vocab 128 256; 16 KB per state and grammar.  Size the bank
                for the automata it will hold.
        gram    int32 [B] (-1: no grammar), state int32 [B] (0 .. S - 1; S: finished; -1: dead)

    A new bank has no grammar in any slot: a step with it computes bit for bit what the step computes without one.  The setters are
    plain device writes between replays of a captured step, not part of one."""

    def __init__(self, B, table, device, grammars=8, max_states=4096):
        torch = _torch()
        from ._native import QpalError
        if not isinstance(table, TokenTable):
            raise QpalError("GrammarBank: table must be a TokenTable")
        if not 1 <= int(B) <= MAX_SLOTS or not 1 <= int(grammars) <= MAX_GRAMMARS or not 1 <= int(max_states) <= MAX_STATES:
            raise QpalError(f"GrammarBank: B in 1 .. {MAX_SLOTS}, grammars in 1 .. {MAX_GRAMMARS} and max_states in 1 .. {MAX_STATES}, "
                            f"got {B}, {grammars}, {max_states}")
        self.B, self.table, self.device = int(B), table, torch.device(device)
        self.vocab, self.grammars, self.max_states = table.vocab, int(grammars), int(max_states)
        self.words = (self.vocab + 31) // 32
        self.allow_bytes = self.grammars * (self.max_states + 1) * self.words * 4
        dev = self.device
        self.tok_off = torch.from_numpy(table.tok_off).to(dev)
        self.tok_bytes = torch.from_numpy(table.tok_bytes).to(dev)
        self.trans = torch.full((self.grammars, self.max_states, 256), -1, dtype=torch.int16, device=dev)  # 0xFFFF: no transition
        self.accept = torch.zeros(self.grammars, self.max_states, dtype=torch.uint8, device=dev)
        self.n_states = torch.zeros(self.grammars, dtype=torch.int32, device=dev)
        self.allow = torch.zeros(self.grammars, self.max_states + 1, self.words, dtype=torch.int32, device=dev)
        self.gram = torch.full((self.B,), -1, dtype=torch.int32, device=dev)
        self.state = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.dfas = [None] * self.grammars   # the host copies: what `matched` and the callers' checks read
        self._slot_gram = [None] * self.B

    def _slot(self, who, slot):
        from ._native import QpalError
        if not 0 <= int(slot) < self.B:
            raise QpalError(f"GrammarBank.{who}: slot {slot} outside 0 .. {self.B - 1}")
        return int(slot)

    def _gram(self, who, g):
        from ._native import QpalError
        if not 0 <= int(g) < self.grammars:
            raise QpalError(f"GrammarBank.{who}: grammar {g} outside 0 .. {self.grammars - 1}")
        return int(g)

    def _vocab_args(self):
        return [self.tok_off.data_ptr(), self.tok_bytes.data_ptr(), self.vocab, self.table.total, self.table.eos]

    def _bank_args(self):
        return [self.trans.data_ptr(), self.accept.data_ptr(), self.n_states.data_ptr(), self.grammars, self.max_states]

    def load(self, g, dfa_or_pattern):
        """grammar g = this automaton (a ByteDFA, or a pattern for compile_regex): upload, one compile launch, then ONE read of
        the table — at load time, never in a step.  QpalError if the automaton is too large for the bank, if a slot still uses g,
        or if a state's row is empty: from such a state no token could be drawn (the vocabulary cannot continue the text)."""
        torch = _torch()
        from . import _native
        QpalError = _native.QpalError
        g = self._gram("load", g)
        if g in self._slot_gram:
            raise QpalError(f"GrammarBank.load: grammar {g} is in use by slot {self._slot_gram.index(g)}: clear it first")
        try:
            dfa = dfa_or_pattern if isinstance(dfa_or_pattern, ByteDFA) else compile_regex(dfa_or_pattern, max_states=self.max_states)
        except ValueError as e:
            raise QpalError(f"GrammarBank.load: {e}") from None
        trans, accept = np.ascontiguousarray(dfa.trans), np.ascontiguousarray(dfa.accept)
        S = trans.shape[0]
        if trans.dtype != np.uint16 or trans.shape != (S, 256) or accept.dtype != np.uint8 or accept.shape != (S,) or not 1 <= S <= self.max_states:
            raise QpalError(f"GrammarBank.load: trans uint16 [S, 256] and accept uint8 [S] with 1 <= S <= {self.max_states}, got "
                            f"{trans.dtype} {list(trans.shape)}, {accept.dtype} {list(accept.shape)}")
        self.n_states[g] = 0   # until the table is there no slot could follow it
        self.trans[g, :S] = torch.from_numpy(trans.view(np.int16)).to(self.device)
        self.accept[g, :S] = torch.from_numpy(accept).to(self.device)
        with torch.cuda.device(self.device):
            rc = _native.lib().qpal_grammar_compile(self.trans[g].data_ptr(), self.accept[g].data_ptr(), S, *self._vocab_args(),
                                                    self.allow[g].data_ptr(), self.words,
                                                    torch.cuda.current_stream(self.device).cuda_stream)
        _native.check(rc, "qpal_grammar_compile")
        empty = (self.allow[g, :S + 1] == 0).all(dim=1).nonzero().reshape(-1).tolist()   # the one host read of a load
        if empty:
            self.dfas[g] = None
            raise QpalError(f"GrammarBank.load: no token of the vocabulary continues the text from state {empty[0]} "
                            f"({len(empty)} of {S} states): a row there would have no drawable token")
        self.n_states[g] = S
        self.dfas[g] = ByteDFA(trans, accept)
        return self.dfas[g]

    def unload(self, g):
        """grammar g is gone; slots using it must have been cleared first"""
        from ._native import QpalError
        g = self._gram("unload", g)
        if g in self._slot_gram:
            raise QpalError(f"GrammarBank.unload: grammar {g} is in use by slot {self._slot_gram.index(g)}: clear it first")
        self.n_states[g] = 0
        self.dfas[g] = None

    def set(self, slot, g):
        """slot follows grammar g from its start (state 0); None: the slot has no grammar"""
        from ._native import QpalError
        slot = self._slot("set", slot)
        if g is not None:
            g = self._gram("set", g)
            if self.dfas[g] is None:
                raise QpalError(f"GrammarBank.set: grammar {g} is not loaded")
        self.state[slot] = 0
        self.gram[slot] = -1 if g is None else g
        self._slot_gram[slot] = g

    def reset(self, slot):
        """the slot back in state 0 (a new request); its grammar stays"""
        self.state[self._slot("reset", slot)] = 0

    def matched(self, slot):
        """a host read: True if the slot's emitted text is a whole match so far (an accepting state, or finished by eos)"""
        slot = self._slot("matched", slot)
        g = self._slot_gram[slot]
        if g is None:
            return False
        s, dfa = int(self.state[slot]), self.dfas[g]
        S = dfa.trans.shape[0]
        return s == S or (0 <= s < S and bool(dfa.accept[s]))


def _arr(t, name, dtype, shape, dev, who):
    from ._native import QpalError
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != dev:
        raise QpalError(f"{who}: {name} must be a contiguous {dtype} {list(shape)} tensor on {dev}")
    return t.data_ptr()


def _bank(bank, who):
    from ._native import QpalError
    if not isinstance(bank, GrammarBank):
        raise QpalError(f"{who}: bank must be a GrammarBank")
    if bank.device.type != "cuda":
        raise QpalError(f"{who}: the bank must live on a GPU, got {bank.device}")
    return bank


def _slots(bank, slot0, slots, who):
    """the slots slot0 .. slot0 + slots - 1 of the bank a launch works on (default: all): (slot0, slots)"""
    from ._native import QpalError
    slots = bank.B - slot0 if slots is None else int(slots)
    if not 0 <= int(slot0) < bank.B or not 1 <= slots <= bank.B - slot0:
        raise QpalError(f"{who}: slots {slot0} .. {slot0 + slots - 1} outside the bank's {bank.B}")
    return int(slot0), slots


def grammar_rows(bank, tokens, row0, row_state):
    """row_state int32 [rows] = the automaton state in front of every row of a speculative step's segments (tokens int64 [rows], row0
    int32 [B + 1]: spec_draft's): row first + j of slot b gets the state after the j guessed tokens in front of it, starting from
    bank.state[b]; rows of no segment, of a slot without a grammar or behind a guess the grammar forbids get -1.  One launch on the
    current stream; no host read."""
    torch = _torch()
    from . import _native
    who = "grammar.grammar_rows"
    bank, dev = _bank(bank, who), bank.device
    rows = tokens.shape[0] if tokens.dim() == 1 else 0
    if not 1 <= rows <= MAX_ROWS:
        raise _native.QpalError(f"{who}: tokens must be int64 [rows] with 1 <= rows <= {MAX_ROWS}")
    tp, rp = _arr(tokens, "tokens", torch.int64, (rows,), dev, who), _arr(row0, "row0", torch.int32, (bank.B + 1,), dev, who)
    op = _arr(row_state, "row_state", torch.int32, (rows,), dev, who)
    with torch.cuda.device(dev):
        rc = _native.lib().qpal_grammar_rows(*bank._bank_args(), *bank._vocab_args(), bank.gram.data_ptr(), bank.state.data_ptr(), bank.B,
                                             tp, rp, rows, op, torch.cuda.current_stream(dev).cuda_stream)
    _native.check(rc, "qpal_grammar_rows")
    return row_state


def grammar_mask(logits, bank, row_slot, ctr, row_state=None):
    """In place on logits fp32 [rows, >= bank.vocab] (contiguous rows, 1 .. 128): row r of slot row_slot[r] (int32 [rows]) with counter
    ctr[r] (int64 [rows]; < 0: inactive) gets -inf wherever the grammar of its slot forbids the token in state row_state[r] (int32
    [rows]; default: bank.state — row = slot, rows = B).  A row that is inactive, whose slot is outside the bank or has no grammar,
    or whose state is dead keeps every bit.  One launch on the current stream; no host read.  Returns logits."""
    torch = _torch()
    from . import _native
    who, QpalError = "grammar.grammar_mask", _native.QpalError
    bank, dev = _bank(bank, who), bank.device
    if logits.dtype != torch.float32 or not logits.is_cuda or logits.dim() != 2 or logits.stride(1) != 1:
        raise QpalError(f"{who}: logits must be an fp32 device tensor [rows, vocab] with contiguous rows")
    rows, vocab = logits.shape[0], bank.vocab
    ld = logits.stride(0) if rows > 1 else logits.shape[1]
    if not 1 <= rows <= MAX_ROWS or vocab > logits.shape[1] or ld < vocab or logits.device != dev:
        raise QpalError(f"{who}: 1 .. {MAX_ROWS} rows of {bank.vocab} logits on {dev}, got {list(logits.shape)} on {logits.device}")
    row_state = bank.state if row_state is None else row_state
    rs, cp = _arr(row_slot, "row_slot", torch.int32, (rows,), dev, who), _arr(ctr, "ctr", torch.int64, (rows,), dev, who)
    sp = _arr(row_state, "row_state", torch.int32, (rows,), dev, who)
    with torch.cuda.device(dev):
        rc = _native.lib().qpal_grammar_mask(logits.data_ptr(), ld, rows, vocab, rs, cp, sp, bank.gram.data_ptr(), bank.B,
                                             bank.n_states.data_ptr(), bank.grammars, bank.max_states, bank.allow.data_ptr(), bank.words,
                                             torch.cuda.current_stream(dev).cuda_stream)
    _native.check(rc, "qpal_grammar_mask")
    return logits


def grammar_advance(bank, tokens, n=None, active=None, slot0=0):
    """bank.state[slot0 + b] follows tokens[b, :n[b]] (tokens int64 [slots, width] or [slots], width <= 16; n int32 [slots], default
    all; active int64 [slots], < 0 skips the slot) for the slots slot0 .. slot0 + slots - 1 of the bank.  One launch on the current
    stream; no host read."""
    torch = _torch()
    from . import _native
    who = "grammar.grammar_advance"
    bank, dev = _bank(bank, who), bank.device
    if tokens.dim() not in (1, 2) or not 1 <= (tokens.shape[1] if tokens.dim() == 2 else 1) <= MAX_WIDTH:
        raise _native.QpalError(f"{who}: tokens must be int64 [slots] or [slots, width <= {MAX_WIDTH}]")
    slot0, slots = _slots(bank, slot0, tokens.shape[0], who)
    width = tokens.shape[1] if tokens.dim() == 2 else 1
    tp = _arr(tokens, "tokens", torch.int64, tuple(tokens.shape), dev, who)
    np_ = None if n is None else _arr(n, "n", torch.int32, (slots,), dev, who)
    ap = None if active is None else _arr(active, "active", torch.int64, (slots,), dev, who)
    with torch.cuda.device(dev):
        rc = _native.lib().qpal_grammar_advance(*bank._bank_args(), *bank._vocab_args(), bank.gram[slot0:].data_ptr(),
                                                bank.state[slot0:].data_ptr(), slots, tp, width, np_, ap,
                                                torch.cuda.current_stream(dev).cuda_stream)
    _native.check(rc, "qpal_grammar_advance")
