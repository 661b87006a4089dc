"""Constrained decoding on the host: regular expressions over bytes, and the token automaton the device walks.

No torch here; numpy only. Three layers:

1. ``compile_regex(pattern) -> ByteDFA``: a regular expression over BYTES with full-match semantics, those of Python's ``re`` on a bytes
   pattern (``\\d \\w \\s`` are ASCII, a multi-byte character is several bytes). Dialect: literals and the escapes ``\\d \\w \\s \\D \\W \\S
   \\. \\\\ \\n \\t \\r \\f \\v \\xNN`` (and any escaped punctuation), classes ``[a-z0-9_]`` / ``[^...]``, ``.`` (any byte but ``\\n``),
   ``|``, ``( )``, ``(?: )``, ``? * +``, ``{m}``, ``{m,}``, ``{m,n}``. Anchors, back-references, look-around, flags, named groups and lazy
   or possessive quantifiers are a ValueError that names the construct. Thompson NFA -> subset construction -> trimming (only states
   from which an accepting state is reachable survive) -> Moore minimisation; state 0 is the start.

2. ``TokenFSM``: the DFA lifted to token ids. ``vocab[v]`` is the bytes of id v, or None for ids that never occur inside a grammar
   (special and added tokens); ``vocab_bytes(tokenizer)`` builds the list from a sentencepiece / Llama tokenizer. States are the DFA
   states reachable at token boundaries, state 0 the start. ``trans[s][v]`` is the next state, or -1 where the piece's bytes do not
   survive from s or land in a state from which no sequence of PIECES reaches acceptance: no reachable state is a dead end.
   ``flags[s]``: bit 0 = accepting, bit 1 = final (accepting and no outgoing id). ``from_choices`` builds the same thing from a list of
   id sequences (a trie): multiple choice, and token-level formats such as ``<box_start><loc-i><loc-j><loc-k><loc-l><box_end>``.

3. THE RULE the device runs in the tail of the token step (csrc/decode.hip next_token_kernel<.., FSM>, sx_token_fsm_args), in numpy fp32:

   ``constrain_row(row, fsm, state, eos_id)``: y[v] = -inf where trans[state][v] < 0; y[eos_id] keeps its value iff flags[state] & 1,
   otherwise it is -inf; nothing else changes.
   ``advance(fsm, state, id, eos_id)``: DONE (-2) on EOS; otherwise s' = trans[state][id]; DONE if s' < 0 (only reachable when every
   admissible logit was -inf already); DONE after entering a final state (reported as a stop); else s'.

   A row whose state is DONE (< 0) runs unconstrained; the engines cut the request there.

Out of scope (follow-ups): JSON-schema to regex; context-free grammars; steering the walk so that it completes within the token budget
(a budget that runs out mid-grammar reports ``complete = False``); the verify step of speculative decoding; tensor-parallel ranks;
grammars that admit the image block (the engines ban ``<img>``, ``<img_i>``, ``</img>`` in every grammar they load).
"""
import numpy as np

DONE = -2
ACCEPTING, FINAL = 1, 2
MAX_STATES = 32767            # int16 next states
_MAX_REPEAT = 1000

_DIGIT = frozenset(range(0x30, 0x3A))
_WORD = frozenset(list(range(0x30, 0x3A)) + list(range(0x41, 0x5B)) + list(range(0x61, 0x7B)) + [0x5F])
_SPACE = frozenset(b" \t\n\r\f\v")
_ALL = frozenset(range(256))
_CLASS_ESC = {ord("d"): _DIGIT, ord("w"): _WORD, ord("s"): _SPACE, ord("D"): _ALL - _DIGIT, ord("W"): _ALL - _WORD, ord("S"): _ALL - _SPACE}
_CHAR_ESC = {ord("n"): 10, ord("t"): 9, ord("r"): 13, ord("f"): 12, ord("v"): 11, ord("a"): 7, ord("0"): 0}
_HEX = b"0123456789abcdefABCDEF"


# ---- regular expression -> AST -------------------------------------------------------------------------------------------------------
class _Parser:
    """alt := cat ('|' cat)* ; cat := rep* ; rep := atom quantifier? ; nodes: ('set', frozenset) ('cat', [..]) ('alt', [..])
    ('rep', node, m, n | None)."""

    def __init__(self, pattern):
        self.p = pattern.encode("utf-8") if isinstance(pattern, str) else bytes(pattern)
        self.i = 0

    def err(self, what):
        raise ValueError(f"compile_regex: {what} at byte {self.i} of {self.p!r}")

    def peek(self):
        return self.p[self.i] if self.i < len(self.p) else None

    def parse(self):
        node = self.alt()
        if self.i != len(self.p):
            self.err("unbalanced parenthesis ')'")
        return node

    def alt(self):
        items = [self.cat()]
        while self.peek() == ord("|"):
            self.i += 1
            items.append(self.cat())
        return items[0] if len(items) == 1 else ("alt", items)

    def cat(self):
        items = []
        while self.peek() is not None and self.peek() not in b"|)":
            items.append(self.rep())
        return ("cat", items)

    def quantifier(self):
        """(m, n | None) and the index behind it, or None where no quantifier starts here (a '{' that opens none is a literal)."""
        c = self.peek()
        if c == ord("?"):
            return 0, 1, self.i + 1
        if c == ord("*"):
            return 0, None, self.i + 1
        if c == ord("+"):
            return 1, None, self.i + 1
        if c != ord("{"):
            return None
        j = self.i + 1
        k = j
        while k < len(self.p) and self.p[k] in b"0123456789":
            k += 1
        lo = self.p[j:k]
        if k < len(self.p) and self.p[k] == ord("}"):
            return (int(lo), int(lo), k + 1) if lo else None
        if k < len(self.p) and self.p[k] == ord(","):
            e = k + 1
            while e < len(self.p) and self.p[e] in b"0123456789":
                e += 1
            hi = self.p[k + 1:e]
            if e < len(self.p) and self.p[e] == ord("}") and (lo or hi):
                return int(lo) if lo else 0, int(hi) if hi else None, e + 1
        return None

    def rep(self):
        if self.peek() in b"?*+":
            self.err("nothing to repeat")
        node = self.atom()
        q = self.quantifier()
        if q is None:
            return node
        m, n, self.i = q
        if n is not None and n < m:
            self.err(f"repeat {{{m},{n}}}: min > max")
        if m > _MAX_REPEAT or (n or 0) > _MAX_REPEAT:
            self.err(f"repeat count above {_MAX_REPEAT}")
        if self.peek() == ord("?"):
            self.err("lazy quantifier")
        if self.peek() == ord("+"):
            self.err("possessive quantifier")
        if self.peek() == ord("*") or self.quantifier() is not None:
            self.err("multiple repeat")
        return ("rep", node, m, n)

    def atom(self):
        c = self.p[self.i]
        self.i += 1
        if c == ord("("):
            if self.peek() == ord("?"):
                nxt = self.p[self.i + 1:self.i + 3]
                if nxt[:1] == b":":
                    self.i += 2
                elif nxt[:1] in (b"=", b"!") or nxt in (b"<=", b"<!"):
                    self.err("look-around")
                elif nxt[:1] == b"P" or nxt[:1] == b"<":
                    self.err("named group / named back-reference")
                elif nxt[:1] == b"#":
                    self.err("comment group")
                elif nxt[:1] == b"(":
                    self.err("conditional group")
                elif nxt[:1] == b">":
                    self.err("atomic group")
                else:
                    self.err("inline flags")
            node = self.alt()
            if self.peek() != ord(")"):
                self.err("missing ')'")
            self.i += 1
            return node
        if c == ord("["):
            return ("set", self.char_class())
        if c == ord("."):
            return ("set", _ALL - {10})
        if c == ord("^"):
            self.i -= 1
            self.err("anchor '^'")
        if c == ord("$"):
            self.i -= 1
            self.err("anchor '$'")
        if c == ord("\\"):
            s = self.escape(False)
            return ("set", s if isinstance(s, frozenset) else frozenset([s]))
        return ("set", frozenset([c]))

    def escape(self, in_class):
        """Behind a backslash: a frozenset (class escape) or one byte value."""
        if self.i >= len(self.p):
            self.err("bad escape (end of pattern)")
        c = self.p[self.i]
        self.i += 1
        if c in _CLASS_ESC:
            return _CLASS_ESC[c]
        if c == ord("x"):
            h = self.p[self.i:self.i + 2]
            if len(h) != 2 or h[0] not in _HEX or h[1] not in _HEX:
                self.err("incomplete escape \\x")
            self.i += 2
            return int(h, 16)
        if c == ord("b") and in_class:
            return 8
        if c in b"AZbB":
            self.i -= 2
            self.err(f"anchor '\\{chr(c)}'")
        if c in b"123456789":
            self.i -= 2
            self.err(f"back-reference '\\{chr(c)}'")
        if c in _CHAR_ESC:
            if c == ord("0"):                     # \0, \00, \012: octal
                j = self.i
                while j < len(self.p) and j < self.i + 2 and self.p[j] in b"01234567":
                    j += 1
                v = int(self.p[self.i - 1:j], 8)
                self.i = j
                return v
            return _CHAR_ESC[c]
        if (0x30 <= c <= 0x39) or (0x41 <= c <= 0x5A) or (0x61 <= c <= 0x7A):
            self.i -= 2
            self.err(f"bad escape '\\{chr(c)}'")
        return c

    def char_class(self):
        neg = self.peek() == ord("^")
        if neg:
            self.i += 1
        out, first = set(), True
        while True:
            if self.i >= len(self.p):
                self.err("unterminated character set")
            c = self.p[self.i]
            self.i += 1
            if c == ord("]") and not first:
                break
            first = False
            lo = self.escape(True) if c == ord("\\") else c
            if isinstance(lo, frozenset):
                out |= lo
                continue
            if self.peek() == ord("-") and self.i + 1 < len(self.p) and self.p[self.i + 1] != ord("]"):
                self.i += 1
                c2 = self.p[self.i]
                self.i += 1
                hi = self.escape(True) if c2 == ord("\\") else c2
                if isinstance(hi, frozenset) or hi < lo:
                    self.err("bad character range")
                out |= set(range(lo, hi + 1))
            else:
                out.add(lo)
        return (_ALL - out) if neg else frozenset(out)


# ---- AST -> Thompson NFA -> DFA ------------------------------------------------------------------------------------------------------
class _NFA:
    def __init__(self):
        self.eps, self.sets, self.to = [], [], []         # per state: epsilon targets; at most one (byte set, target) edge

    def new(self):
        self.eps.append([])
        self.sets.append(None)
        self.to.append(-1)
        return len(self.eps) - 1

    def build(self, node):
        """(start, end) of a fresh copy of the node's automaton."""
        kind = node[0]
        if kind == "set":
            a, b = self.new(), self.new()
            self.sets[a], self.to[a] = node[1], b
            return a, b
        if kind == "cat":
            a = b = self.new()
            for sub in node[1]:
                s, e = self.build(sub)
                self.eps[b].append(s)
                b = e
            return a, b
        if kind == "alt":
            a, b = self.new(), self.new()
            for sub in node[1]:
                s, e = self.build(sub)
                self.eps[a].append(s)
                self.eps[e].append(b)
            return a, b
        _, sub, m, n = node
        a = b = self.new()
        for _ in range(m):
            s, e = self.build(sub)
            self.eps[b].append(s)
            b = e
        if n is None:                                     # sub*
            s, e = self.build(sub)
            hub = self.new()
            self.eps[b].append(hub)
            self.eps[hub].append(s)
            self.eps[e].append(hub)
            return a, hub
        end = self.new()
        for _ in range(n - m):                            # (sub (sub (...)?)?)?
            self.eps[b].append(end)
            s, e = self.build(sub)
            self.eps[b].append(s)
            b = e
        self.eps[b].append(end)
        return a, end


class ByteDFA:
    """``table`` int32 [n_states, 256] (-1: no transition), ``accept`` bool [n_states]; state 0 is the start. Trimmed: an accepting state
    is reachable from every state. Minimal (Moore)."""

    def __init__(self, table, accept):
        self.table = np.ascontiguousarray(table, dtype=np.int32)
        self.accept = np.ascontiguousarray(accept, dtype=bool)
        assert self.table.ndim == 2 and self.table.shape[1] == 256 and self.accept.shape == (self.table.shape[0],)

    @property
    def n_states(self):
        return self.table.shape[0]

    def accepts(self, data):
        s = 0
        for b in bytes(data):
            s = int(self.table[s, b])
            if s < 0:
                return False
        return bool(self.accept[s])

    def with_optional_prefix(self, prefix=b" "):
        """The DFA of ``(prefix)?L`` for a one-byte prefix."""
        assert len(prefix) == 1
        p = prefix[0]
        start = ("X",)
        index, order, rows = {start: 0}, [start], []
        k = 0
        while k < len(order):
            cur = order[k]
            k += 1
            row = np.full(256, -1, dtype=np.int32)
            for b in range(256):
                if cur == start:
                    t = {int(self.table[0, b])} | ({0} if b == p else set())
                else:
                    t = {int(self.table[q, b]) for q in cur}
                t = tuple(sorted(q for q in t if q >= 0))
                if not t:
                    continue
                if t not in index:
                    index[t] = len(order)
                    order.append(t)
                row[b] = index[t]
            rows.append(row)
        acc = [bool(self.accept[0]) if s == start else any(self.accept[q] for q in s) for s in order]
        return _trim_minimise(np.stack(rows), np.array(acc, dtype=bool))


def _trim_minimise(table, accept):
    n = table.shape[0]
    # trim: states from which an accepting state is reachable (every state is reachable from the start by construction)
    live = accept.copy()
    while True:
        nxt = live | ((table >= 0) & live[np.maximum(table, 0)]).any(axis=1)
        if (nxt == live).all():
            break
        live = nxt
    if not live[0]:
        raise ValueError("compile_regex: the pattern matches nothing (an empty language)")
    table = np.where((table >= 0) & live[np.maximum(table, 0)], table, -1)
    keep = np.flatnonzero(live)
    remap = np.full(n + 1, -1, dtype=np.int64)
    remap[keep] = np.arange(len(keep))
    table, accept = remap[table[keep]], accept[keep]       # (index -1 reads remap's last entry, -1)
    # reachable from the start (trimming may cut paths), in BFS order so that the numbering is canonical
    order, seen = [0], {0}
    for s in order:
        for t in table[s]:
            t = int(t)
            if t >= 0 and t not in seen:
                seen.add(t)
                order.append(t)
    remap = np.full(table.shape[0] + 1, -1, dtype=np.int64)
    remap[order] = np.arange(len(order))
    table, accept = remap[table[order]], accept[order]
    # Moore: refine {accepting, not} by the classes of the 256 successors until nothing splits
    labels = accept.astype(np.int64)
    while True:
        sig = np.concatenate([labels[:, None], np.where(table >= 0, labels[np.maximum(table, 0)], -1)], axis=1)
        _, new = np.unique(sig, axis=0, return_inverse=True)
        new = new.reshape(-1)
        if len(np.unique(new)) == len(np.unique(labels)):      # (refinement only splits: the same count is the same partition)
            break
        labels = new
    # one representative per class, numbered by first occurrence (state 0 stays the start)
    _, first = np.unique(labels, return_index=True)
    reps = np.sort(first)
    cls = np.full(labels.max() + 1, -1, dtype=np.int64)
    cls[labels[reps]] = np.arange(len(reps))
    t = table[reps]
    out = np.where(t >= 0, cls[labels[np.maximum(t, 0)]], -1)
    return ByteDFA(out, accept[reps])


def compile_regex(pattern):
    """A regular expression over bytes (str patterns are taken as their UTF-8 bytes), full-match semantics -> ByteDFA. See the module
    docstring for the dialect; what lies outside it is a ValueError that names the construct."""
    ast = _Parser(pattern).parse()
    nfa = _NFA()
    start, end = nfa.build(ast)
    n = len(nfa.eps)

    def closure(states):
        stack, seen = list(states), set(states)
        while stack:
            for t in nfa.eps[stack.pop()]:
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        return frozenset(seen)

    masks = np.zeros((n, 256), dtype=bool)
    for s in range(n):
        if nfa.sets[s] is not None:
            masks[s, list(nfa.sets[s])] = True
    s0 = closure([start])
    index, order, rows, memo = {s0: 0}, [s0], [], {}
    k = 0
    while k < len(order):
        cur = order[k]
        k += 1
        src = np.array([s for s in sorted(cur) if nfa.sets[s] is not None], dtype=np.int64)
        row = np.full(256, -1, dtype=np.int32)
        if len(src):
            cols, inv = np.unique(masks[src].T, axis=0, return_inverse=True)       # bytes with the same set of live edges move together
            inv = inv.reshape(-1)
            for j, col in enumerate(cols):
                if not col.any():
                    continue
                key = frozenset(nfa.to[s] for s in src[col])
                if key not in memo:
                    memo[key] = closure(key)
                t = memo[key]
                if t not in index:
                    index[t] = len(order)
                    order.append(t)
                row[inv == j] = index[t]
        rows.append(row)
    return _trim_minimise(np.stack(rows), np.array([end in s for s in order], dtype=bool))


# ---- the token automaton -------------------------------------------------------------------------------------------------------------
def vocab_bytes(tokenizer):
    """One ``bytes`` per id of a sentencepiece / Llama tokenizer, None for added and special tokens: ``▁`` becomes a space, ``<0xNN>``
    that byte. Ids at or above the sentencepiece model's own size (added tokens: ``<img>``, ``<loc-i>``, ...) and every id in
    ``all_special_ids`` are None."""
    n = len(tokenizer)
    sp = getattr(tokenizer, "sp_model", None)
    base = sp.get_piece_size() if sp is not None else getattr(tokenizer, "vocab_size", n)
    special = set(getattr(tokenizer, "all_special_ids", ()) or ())
    added = set((getattr(tokenizer, "get_added_vocab", lambda: {})() or {}).values())
    out = []
    for i in range(n):
        if i >= base or i in special or i in added:
            out.append(None)
            continue
        piece = tokenizer.convert_ids_to_tokens(i)
        if piece is None:
            out.append(None)
        elif len(piece) == 6 and piece.startswith("<0x") and piece.endswith(">"):
            out.append(bytes([int(piece[3:5], 16)]))
        else:
            out.append(piece.replace("▁", " ").encode("utf-8"))
    return out


class TokenFSM:
    """``trans`` int16 [n_states, V] (next state, -1 = banned), ``flags`` int32 [n_states] (bit 0 accepting, bit 1 final); state 0 is the
    start; no reachable state is a dead end."""

    def __init__(self, trans, flags, source=None):
        self.trans = np.ascontiguousarray(trans, dtype=np.int16)
        self.flags = np.ascontiguousarray(flags, dtype=np.int32)
        self.source = source
        assert self.trans.ndim == 2 and self.flags.shape == (self.trans.shape[0],)

    @property
    def n_states(self):
        return self.trans.shape[0]

    @property
    def vocab_size(self):
        return self.trans.shape[1]

    @classmethod
    def from_regex(cls, pattern, vocab, eos_id=None, banned_ids=(), allow_leading_space=False, max_states=MAX_STATES):
        fsm = cls.from_dfa(compile_regex(pattern), vocab, eos_id, banned_ids, allow_leading_space, max_states)
        fsm.source = pattern
        return fsm

    @classmethod
    def from_dfa(cls, dfa, vocab, eos_id=None, banned_ids=(), allow_leading_space=False, max_states=MAX_STATES):
        """Lift a ByteDFA to the ids of ``vocab``. ``eos_id`` and ``banned_ids`` are -1 everywhere (EOS is governed by bit 0 of the
        flags, not by the table), and so are None pieces and empty pieces (an id without bytes would never advance the automaton).
        ``allow_leading_space``: the language becomes ``( )?L`` — a sentencepiece model likes to open a word with ``▁``. Vectorised
        over the vocabulary: all pieces advance one byte position at a time through the DFA table, from every DFA state at once."""
        if allow_leading_space:
            dfa = dfa.with_optional_prefix(b" ")
        V, S = len(vocab), dfa.n_states
        off = set(int(b) for b in banned_ids)
        if eos_id is not None and int(eos_id) >= 0:
            off.add(int(eos_id))
        use = np.array([p is not None and len(p) > 0 and v not in off for v, p in enumerate(vocab)], dtype=bool)
        ids = np.flatnonzero(use)
        L = max((len(vocab[v]) for v in ids), default=0)
        data = np.zeros((len(ids), max(L, 1)), dtype=np.uint8)
        lens = np.zeros(len(ids), dtype=np.int64)
        for k, v in enumerate(ids):
            p = vocab[v]
            data[k, :len(p)] = np.frombuffer(p, dtype=np.uint8)
            lens[k] = len(p)
        # pieces sorted by length: position j only moves the pieces that are longer than j
        srt = np.argsort(-lens, kind="stable")
        data, lens, ids = data[srt], lens[srt], ids[srt]
        tab = np.concatenate([dfa.table, np.full((1, 256), -1, dtype=np.int32)])         # row -1: the dead state stays dead
        cur = np.repeat(np.arange(S, dtype=np.int32)[:, None], len(ids), axis=1)         # [S, pieces]
        for j in range(L):
            m = int((lens > j).sum())
            cur[:, :m] = tab[cur[:, :m], data[None, :m, j]]
        # a DFA state is LIVE when a sequence of pieces reaches acceptance from it (bytes alone do not promise that)
        live = dfa.accept.copy()
        ok = cur >= 0
        while True:
            nxt = live | (ok & live[np.maximum(cur, 0)]).any(axis=1)
            if (nxt == live).all():
                break
            live = nxt
        if not live[0]:
            raise ValueError("TokenFSM: an empty language: no sequence of the vocabulary's pieces is accepted by the grammar")
        cur = np.where(ok & live[np.maximum(cur, 0)], cur, -1)
        # the states reachable at token boundaries, numbered in BFS order from the start
        order, seen = [0], np.zeros(S, dtype=bool)
        seen[0] = True
        k = 0
        while k < len(order):
            t = np.unique(cur[order[k]])
            k += 1
            for q in t[(t >= 0)]:
                if not seen[q]:
                    seen[q] = True
                    order.append(int(q))
        if len(order) > max_states:
            raise ValueError(f"TokenFSM: the grammar needs {len(order)} states, the capacity is {max_states}")
        remap = np.full(S + 1, -1, dtype=np.int64)
        remap[order] = np.arange(len(order))
        trans = np.full((len(order), V), -1, dtype=np.int16)
        trans[:, ids] = remap[cur[order]]
        return cls(trans, cls._flags(trans, dfa.accept[order]))

    @staticmethod
    def _flags(trans, accept):
        accept = np.asarray(accept, dtype=bool)
        final = accept & ~(trans >= 0).any(axis=1)
        return accept.astype(np.int32) * ACCEPTING + final.astype(np.int32) * FINAL

    @classmethod
    def from_choices(cls, id_sequences, vocab_size, eos_id=None, banned_ids=(), max_states=MAX_STATES):
        """A trie over token ids: the accepted language is exactly the listed sequences."""
        seqs = [tuple(int(t) for t in s) for s in id_sequences]
        if not seqs:
            raise ValueError("TokenFSM.from_choices: an empty choice list (an empty language)")
        off = set(int(b) for b in banned_ids)
        if eos_id is not None and int(eos_id) >= 0:
            off.add(int(eos_id))
        for s in seqs:
            for t in s:
                if not 0 <= t < vocab_size:
                    raise ValueError(f"TokenFSM.from_choices: id {t} lies outside the vocabulary of {vocab_size}")
                if t in off:
                    raise ValueError(f"TokenFSM.from_choices: id {t} is banned (banned_ids / eos_id) and cannot occur in a choice")
        nodes, accept = [{}], [False]
        for s in seqs:
            at = 0
            for t in s:
                if t not in nodes[at]:
                    nodes[at][t] = len(nodes)
                    nodes.append({})
                    accept.append(False)
                at = nodes[at][t]
            accept[at] = True
        if len(nodes) > max_states:
            raise ValueError(f"TokenFSM: the grammar needs {len(nodes)} states, the capacity is {max_states}")
        trans = np.full((len(nodes), vocab_size), -1, dtype=np.int16)
        for s, edges in enumerate(nodes):
            for t, to in edges.items():
                trans[s, t] = to
        return cls(trans, cls._flags(trans, accept), source=seqs)

    def allowed(self, state):
        """The ids admissible in ``state`` (EOS is not among them: bit 0 of ``flags[state]`` governs it)."""
        return np.flatnonzero(self.trans[int(state)] >= 0)

    def walk(self, ids):
        """Walk ``ids`` from the start: ``(state, n_consumed, complete)``. The walk ends at the first inadmissible id and right after
        entering a final state; ``complete``: the state reached is accepting and the walk ended there or consumed every id."""
        s, n = 0, 0
        ids = [int(t) for t in ids]
        for t in ids:
            if self.flags[s] & FINAL or not 0 <= t < self.vocab_size or self.trans[s, t] < 0:
                break
            s = int(self.trans[s, t])
            n += 1
        final = bool(self.flags[s] & FINAL)
        return s, n, bool(self.flags[s] & ACCEPTING) and (final or n == len(ids))

    def table(self, n_states, ld_v):
        """The device image: int16 [n_states, ld_v] padded with -1 and int32 [n_states] padded with 0."""
        if self.n_states > n_states:
            raise ValueError(f"TokenFSM.table: the grammar has {self.n_states} states, the capacity is {n_states}")
        if ld_v < self.vocab_size:
            raise ValueError(f"TokenFSM.table: ld_v={ld_v} is below the vocabulary of {self.vocab_size}")
        t = np.full((n_states, ld_v), -1, dtype=np.int16)
        t[:self.n_states, :self.vocab_size] = self.trans
        f = np.zeros(n_states, dtype=np.int32)
        f[:self.n_states] = self.flags
        return t, f


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
def constrain_row(row, fsm, state, eos_id):
    """The masked copy of a logits row (numpy fp32; columns at or above the vocabulary are copied)."""
    y = np.array(row, dtype=np.float32, copy=True)
    V = fsm.vocab_size
    keep_eos = y[eos_id] if eos_id is not None and 0 <= eos_id < V else None
    y[:V][fsm.trans[int(state)] < 0] = -np.inf
    if keep_eos is not None:
        y[eos_id] = keep_eos if fsm.flags[int(state)] & ACCEPTING else -np.inf
    return y


def advance(fsm, state, id, eos_id):
    """The state after the row emitted ``id`` from ``state`` (>= 0), or DONE."""
    id = int(id)
    if eos_id is not None and eos_id >= 0 and id == eos_id:
        return DONE
    if not 0 <= id < fsm.vocab_size:
        return DONE
    s = int(fsm.trans[int(state), id])
    if s < 0 or fsm.flags[s] & FINAL:
        return DONE
    return s
