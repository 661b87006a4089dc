"""Constrained decoding, the host half (seedx_amd.grammar): the byte DFA against Python's ``re``, the token automaton against brute force,
the rule (constrain_row / advance), the device image and the ABI mirror, and every refusal of the model and the engines. No GPU."""
import ctypes
import itertools
import os
import re
import types

import numpy as np
import pytest

from seedx_amd import grammar
from seedx_amd.grammar import DONE, ByteDFA, TokenFSM, advance, compile_regex, constrain_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ALPHABET = b"ab1 .\n"
STRINGS = [bytes(t) for n in range(7) for t in itertools.product(ALPHABET, repeat=n)]

PATTERNS = [
    rb"", rb"a", rb"ab1", rb"a|b", rb"ab|a1|a", rb"ab|abb|ab1", rb"(a|b)*1", rb"(?:ab)+", rb"a?b*1+", rb"a{3}", rb"a{2,}", rb"a{1,3}b",
    rb"(a{2}|b){2,3}", rb"((a|b)(1| ))*", rb"(a(b(1)?)?)?", rb"[ab]+", rb"[^ab]*", rb"[a-b1]{2,4}", rb"[^\n]*\n?", rb".*", rb".+\n.?", rb"a.b",
    rb"\d+", rb"\w*", rb"\s+", rb"\D\W\S", rb"\.+", rb"a\nb|\t|\\", rb"\x61\x20*", rb"[\d\s]+", rb"[^\d.]+", rb"[]a]+", rb"[a\]]*", rb"[.-1]*",
    rb"(a|ab)(1|b1)", rb"(?:a|(?:b|1){2}){1,2} ?", rb"a{,2}b", rb"a{b", rb"-?(0|1[01]*)(\.[01]+)?", rb"(|a)b",
]


@pytest.mark.parametrize("pattern", PATTERNS, ids=[p.decode("latin-1").encode("unicode_escape").decode() or "empty" for p in PATTERNS])
def test_dfa_equals_re_on_every_short_string(pattern):
    dfa = compile_regex(pattern)
    rx = re.compile(pattern)
    for s in STRINGS:
        assert dfa.accepts(s) == (rx.fullmatch(s) is not None), (pattern, s)
    # trimmed: an accepting state is reachable from every state; minimal: no two states agree on acceptance and all 256 successors
    live = dfa.accept.copy()
    for _ in range(dfa.n_states):
        live |= ((dfa.table >= 0) & live[np.maximum(dfa.table, 0)]).any(axis=1)
    assert live.all()
    sig = {(bool(dfa.accept[s]), tuple(dfa.table[s])) for s in range(dfa.n_states)}
    assert len(sig) == dfa.n_states


def test_dfa_is_minimal_on_known_sizes():
    assert compile_regex(rb"(a|b)*abb").n_states == 4
    assert compile_regex(rb"a|a|a").n_states == 2
    assert compile_regex(rb"(ab|ab)*").n_states == 2
    assert compile_regex("é").n_states == 3                  # a multi-byte character is several bytes
    assert compile_regex(rb"[\x00-\xff]*").n_states == 1


UNSUPPORTED = [(rb"^a", "anchor"), (rb"a$", "anchor"), (rb"\bword", "anchor"), (rb"a\Z", "anchor"), (rb"(a)\1", "back-reference"),
               (rb"(?=a)a", "look-around"), (rb"(?<!a)b", "look-around"), (rb"(?!a)b", "look-around"), (rb"a*?", "lazy"), (rb"a+?", "lazy"),
               (rb"a{1,2}?", "lazy"), (rb"a??", "lazy"), (rb"(?P<n>a)", "named group"), (rb"(?i)a", "flags"), (rb"a*+", "possessive"),
               (rb"a**", "multiple repeat"), (rb"(a", "missing"), (rb"a)", "unbalanced"), (rb"[a", "unterminated"), (rb"*a", "nothing to repeat"),
               (rb"\q", "bad escape"), (rb"\x1", "incomplete escape"), (rb"a{3,1}", "min > max"), (rb"[b-a]", "bad character range"),
               (rb"[^\x00-\xff]", "empty language")]


@pytest.mark.parametrize("pattern,what", UNSUPPORTED, ids=[w + "-" + str(i) for i, (_, w) in enumerate(UNSUPPORTED)])
def test_unsupported_constructs_raise_and_name_the_construct(pattern, what):
    with pytest.raises(ValueError, match=what):
        compile_regex(pattern)


# ---- the token automaton ---------------------------------------------------------------------------------------------------------
# 14 ids: multi-byte pieces, pieces that straddle a boundary of the pattern ("b1", "1a"), a <0xNN> byte piece (id 8, the byte "1"),
# a leading-space piece (" a"), two None specials (11, 12), one banned id (13 = "ab": its bytes would fit) and EOS = 12
VOCAB = [b"a", b"b", b"ab", b"b1", b"1a", b"abab", b" a", b" ", b"1", b"11", b"ba", None, None, b"ab"]
EOS, BANNED = 12, (13,)
TOKEN_PATTERNS = [rb"(ab)+1{1,2}", rb"a(b|1)*a", rb"(ab|ba)1?", rb"ab1a|abab"]


def _brute(pattern, lead, max_len=4):
    rx = re.compile((b"(?: )?(?:" + pattern + b")") if lead else pattern)
    usable = [v for v, p in enumerate(VOCAB) if p is not None and v not in BANNED]
    accepted = set()
    for n in range(max_len + 1):
        for seq in itertools.product(usable, repeat=n):
            if rx.fullmatch(b"".join(VOCAB[v] for v in seq)):
                accepted.add(seq)
    return rx, usable, accepted


@pytest.mark.parametrize("lead", [False, True], ids=["plain", "leading-space"])
@pytest.mark.parametrize("pattern", TOKEN_PATTERNS, ids=[p.decode() for p in TOKEN_PATTERNS])
def test_token_fsm_equals_brute_force(pattern, lead):
    fsm = TokenFSM.from_regex(pattern, VOCAB, eos_id=EOS, banned_ids=BANNED, allow_leading_space=lead)
    rx, usable, accepted = _brute(pattern, lead)
    assert fsm.vocab_size == len(VOCAB) and fsm.n_states >= 2
    assert (fsm.trans[:, [11, 12, 13]] == -1).all()           # specials, EOS and the banned id: -1 everywhere
    for n in range(5):
        for seq in itertools.product(range(len(VOCAB)), repeat=n):
            s, used, complete = fsm.walk(seq)
            ok = used == n and bool(fsm.flags[s] & 1)
            assert ok == (tuple(seq) in accepted), (pattern, seq)
            assert complete == (bool(fsm.flags[s] & 1) and (used == n or bool(fsm.flags[s] & 2)))
    # trans >= 0 iff some completion exists: from every reachable state, by the DFA over the bytes consumed so far
    dfa = compile_regex(pattern)
    if lead:
        dfa = dfa.with_optional_prefix(b" ")
    reach = {0: b""}
    todo = [0]
    while todo:
        s = todo.pop()
        for v in fsm.allowed(s):
            t = int(fsm.trans[s, v])
            if t not in reach:
                reach[t] = reach[s] + VOCAB[v]
                todo.append(t)
    assert sorted(reach) == list(range(fsm.n_states))          # every state is reachable at a token boundary

    def completable(prefix, depth=5):
        if rx.fullmatch(prefix):
            return True
        return depth > 0 and any(completable(prefix + VOCAB[v], depth - 1) for v in usable if _dfa_alive(dfa, prefix + VOCAB[v]))

    for s, prefix in reach.items():
        for v in range(len(VOCAB)):
            want = v in usable and _dfa_alive(dfa, prefix + VOCAB[v]) and completable(prefix + VOCAB[v])
            assert (fsm.trans[s, v] >= 0) == want, (pattern, s, v)
        final = bool(fsm.flags[s] & 1) and len(fsm.allowed(s)) == 0
        assert bool(fsm.flags[s] & 2) == final
        assert bool(fsm.flags[s] & 1) == (rx.fullmatch(prefix) is not None)
        assert fsm.flags[s] & 1 or len(fsm.allowed(s)) > 0     # no dead end


def _dfa_alive(dfa, data):
    s = 0
    for b in data:
        s = int(dfa.table[s, b])
        if s < 0:
            return False
    return True


def test_token_level_dead_ends_are_cut():
    """The byte DFA of ab1 is alive after "a", but with no piece that continues it the id must be banned, and with none at all the
    language is empty."""
    fsm = TokenFSM.from_regex(rb"ab1|b", [b"a", b"b", b"1"][:2] + [b"x"])
    assert list(fsm.allowed(0)) == [1] and fsm.n_states == 2 and list(fsm.flags) == [0, 3]
    with pytest.raises(ValueError, match="empty language"):
        TokenFSM.from_regex(rb"ab1", [b"a", b"b", None])
    with pytest.raises(ValueError, match="empty language"):
        TokenFSM.from_regex(rb"a", [b"a"], banned_ids=[0])
    assert TokenFSM.from_regex(rb"a*", [b"a", b""]).trans[0, 1] == -1        # a piece without bytes never advances: banned


def test_from_choices():
    choices = [(3, 4), (3, 4, 5), (3, 6), (7,), (3, 4, 5)]                    # shared prefixes, one a prefix of another, one twice
    fsm = TokenFSM.from_choices(choices, 10, eos_id=9, banned_ids=(8,))
    accepted = {seq for n in range(5) for seq in itertools.product(range(10), repeat=n)
                if (lambda w: w[1] == len(seq) and fsm.flags[w[0]] & 1)(fsm.walk(seq))}
    assert accepted == set(choices)
    s34 = fsm.walk((3, 4))[0]
    assert fsm.flags[s34] == 1 and fsm.flags[fsm.walk((3, 4, 5))[0]] == 3 and fsm.flags[fsm.walk((7,))[0]] == 3 and fsm.flags[0] == 0
    assert fsm.walk((3, 4)) == (s34, 2, True) and fsm.walk((3,))[2] is False and fsm.walk((7, 7)) == (fsm.walk((7,))[0], 1, True)
    assert fsm.walk((3, 4, 2)) == (s34, 2, False)             # an inadmissible id behind an accepting, not final, state
    assert list(fsm.allowed(0)) == [3, 7] and fsm.n_states == 6
    with pytest.raises(ValueError, match="id 10 lies outside the vocabulary of 10"):
        TokenFSM.from_choices([(1, 10)], 10)
    with pytest.raises(ValueError, match="id 8 is banned"):
        TokenFSM.from_choices([(8,)], 10, banned_ids=(8,))
    with pytest.raises(ValueError, match="id 9 is banned"):
        TokenFSM.from_choices([(1, 9)], 10, eos_id=9)
    with pytest.raises(ValueError, match="empty choice list"):
        TokenFSM.from_choices([], 10)
    with pytest.raises(ValueError, match="needs 4 states, the capacity is 3"):
        TokenFSM.from_choices([(1, 2, 3)], 10, max_states=3)


def test_constrain_row_and_advance():
    fsm = TokenFSM.from_choices([(3, 4), (3, 4, 5), (7,)], 10)
    rng = np.random.default_rng(0)
    row = rng.standard_normal(16).astype(np.float32)           # 6 padding columns behind the vocabulary
    s34 = fsm.walk((3, 4))[0]
    for state in range(fsm.n_states):
        for eos in (None, -1, 9, 4):
            y = constrain_row(row, fsm, state, eos)
            assert y.dtype == np.float32 and y.shape == row.shape
            banned = set(np.flatnonzero(fsm.trans[state] < 0))
            if eos is not None and eos >= 0:
                banned.discard(eos)
                if not fsm.flags[state] & 1:
                    banned.add(eos)
            for v in range(16):
                if v in banned:
                    assert y[v] == -np.inf
                else:
                    assert y[v].tobytes() == row[v].tobytes()
    assert constrain_row(row, fsm, s34, 9)[9] == row[9] and constrain_row(row, fsm, 0, 9)[9] == -np.inf     # EOS follows bit 0
    assert constrain_row(row, fsm, s34, 4)[4] == row[4]       # ... whatever the table says about the column
    assert advance(fsm, 0, 3, 9) == fsm.walk((3,))[0] and advance(fsm, fsm.walk((3,))[0], 4, 9) == s34
    assert advance(fsm, s34, 9, 9) == DONE                     # EOS
    assert advance(fsm, s34, 5, 9) == DONE and advance(fsm, 0, 7, 9) == DONE          # entering a final state
    assert advance(fsm, 0, 2, 9) == DONE and advance(fsm, 0, 12, 9) == DONE and advance(fsm, 0, -1, None) == DONE     # inadmissible ids
    assert DONE == -2


def test_table_padding_and_capacity():
    fsm = TokenFSM.from_choices([(3, 4), (7,)], 10)
    t, f = fsm.table(8, 16)
    assert t.dtype == np.int16 and t.shape == (8, 16) and f.dtype == np.int32 and f.shape == (8,)
    assert (t[:fsm.n_states, :10] == fsm.trans).all() and (t[fsm.n_states:] == -1).all() and (t[:, 10:] == -1).all()
    assert (f[:fsm.n_states] == fsm.flags).all() and (f[fsm.n_states:] == 0).all()
    with pytest.raises(ValueError, match="has 4 states, the capacity is 3"):
        fsm.table(3, 16)
    with pytest.raises(ValueError, match="ld_v=8 is below the vocabulary of 10"):
        fsm.table(8, 8)
    with pytest.raises(ValueError, match="needs 7 states, the capacity is 4"):
        TokenFSM.from_regex(rb"a{6}", [b"a"], max_states=4)


def test_large_vocabulary_builds_vectorised():
    """A grammar of a few hundred states against 32 330 pieces: seconds (measured in profiles/grammar.md), checked against the DFA on
    sampled pieces."""
    vocab = synthetic_vocab()
    fsm = TokenFSM.from_regex(r'\{"name": "[a-z ]{1,40}", "count": (0|[1-9][0-9]{0,3}), "ok": (true|false)\}', vocab, eos_id=2,
                              banned_ids=range(32100, 32330), max_states=256)
    assert 50 < fsm.n_states <= 256 and fsm.vocab_size == 32330
    ids = [int(v) for v in fsm.allowed(0)]
    assert ids and all(vocab[v] is not None and b'{"name": "'.startswith(vocab[v]) for v in ids)
    s, n, done = fsm.walk([vocab.index(bytes([c])) for c in b'{"name": "ab c", "count": 120, "ok": true}'])
    assert done and fsm.flags[s] == 3


def synthetic_vocab(n=32330, seed=0):
    """A sentencepiece-like vocabulary: 3 specials, 256 byte pieces, every printable ASCII character, then random lower-case / digit /
    punctuation pieces of 2 .. 8 bytes (half with a leading space); the last 330 ids are added tokens (None)."""
    rng = np.random.default_rng(seed)
    vocab = [None, None, None] + [bytes([b]) for b in range(256)]
    seen = set(vocab[3:])
    alpha = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789 \":,{}.-", dtype=np.uint8)
    while len(vocab) < n - 330:
        k = int(rng.integers(2, 9))
        p = bytes(rng.choice(alpha[:26] if rng.random() < 0.7 else alpha, size=k))
        if rng.random() < 0.5:
            p = b" " + p
        if p not in seen:
            seen.add(p)
            vocab.append(p)
    return vocab + [None] * 330


def test_vocab_bytes_from_a_sentencepiece_like_tokenizer():
    pieces = ["<unk>", "<s>", "</s>", "<0x0A>", "<0xE2>", "▁the", "a", "▁", "é", "<img>", "<loc-0>"]

    class Tok:
        sp_model = types.SimpleNamespace(get_piece_size=lambda: 9)
        all_special_ids = [0, 1, 2]

        def __len__(self):
            return len(pieces)

        def get_added_vocab(self):
            return {"<img>": 9, "<loc-0>": 10}

        def convert_ids_to_tokens(self, i):
            return pieces[i]

    assert grammar.vocab_bytes(Tok()) == [None, None, None, b"\n", b"\xe2", b" the", b"a", b" ", "é".encode(), None, None]


def test_abi():
    """sx_token_fsm_args: header field order == ctypes struct; the two entry points declared, bound and exported (the parsing of
    test_kv_fork_struct_layout_matches_header)."""
    from seedx_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "seedx_hip.h")).read()
    body = re.search(r"typedef struct sx_token_fsm_args \{(.*?)\} sx_token_fsm_args;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip().lstrip("*") for n in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl).split(",")]
    assert names == [f[0] for f in _lib.TokenFsmArgs._fields_]
    assert names == ["table", "state", "trans", "flags", "n_tables", "n_states", "ld_v", "eos_id"]
    assert ctypes.sizeof(_lib.TokenFsmArgs) == 4 * 8 + 4 * 4
    for name in ("sx_next_b_fsm", "sx_next_slots_fsm"):
        assert name in _lib.SIGNATURES and re.search(r"\bint " + name + r"\(", src)
    assert len(_lib.SIGNATURES["sx_next_b_fsm"]) == len(_lib.SIGNATURES["sx_next_b_ctl"]) + 1
    assert len(_lib.SIGNATURES["sx_next_slots_fsm"]) == len(_lib.SIGNATURES["sx_next_slots_ctl"]) + 1
    assert _lib.SIGNATURES["sx_next_b_fsm"][:-2] == _lib.SIGNATURES["sx_next_b_ctl"][:-1]
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, n) for n in ("sx_next_b_fsm", "sx_next_slots_fsm"))
    assert callable(ops.next_b_fsm) and callable(ops.next_slots_fsm)


# ---- refusals: the model and the engines, before anything is touched -----------------------------------------------------------------
def _mini(**kw):
    from oracle import weights
    from seedx_amd.llama import LlamaForCausalLM
    return LlamaForCausalLM(dict(weights.MINI_LLM), max_cache_len=64, **kw)


def test_model_constructor_and_resident_table_refusals():
    off = _mini()
    assert off.max_grammars == 0 and off.memory_footprint().get("grammars", 0) == 0 and off.grammars == []
    assert off.memory_footprint() == _mini(max_grammars=0, grammar_states=7).memory_footprint()
    fsm = TokenFSM.from_choices([(3, 4)], off.V)
    with pytest.raises(ValueError, match="built with max_grammars=0"):
        off.load_grammar("g", fsm)
    with pytest.raises(ValueError, match="built with max_grammars=0"):
        off.slot_state(grammar=True)
    with pytest.raises(ValueError, match="built with max_grammars=0"):
        off.grammar_state()
    for bad in (1, 0, 32768):
        with pytest.raises(ValueError, match=f"grammar_states={bad} must be in 2 .. 32767"):
            _mini(max_grammars=1, grammar_states=bad)
    with pytest.raises(ValueError, match="max_grammars=-1"):
        _mini(max_grammars=-1)
    m = _mini(max_grammars=2, grammar_states=3)
    fp = m.memory_footprint()
    assert fp["grammars"] == 2 * 3 * (m.Vpad * 2 + 4) and fp["total"] == off.memory_footprint()["total"] + fp["grammars"]
    with pytest.raises(ValueError, match="has 4 states, the model was built with grammar_states=3"):
        m.load_grammar("long", TokenFSM.from_choices([(3, 4, 5)], m.V))
    with pytest.raises(ValueError, match="is over 10 ids, the model's vocabulary has 500"):
        m.load_grammar("small", TokenFSM.from_choices([(3,)], 10))
    with pytest.raises(ValueError, match="unknown grammar 'nope'"):
        m.unload_grammar("nope")
    m._grammars["a"] = (0, fsm)                                # (what load_grammar leaves behind, without a device)
    with pytest.raises(ValueError, match="a grammar named 'a' is resident already"):
        m.load_grammar("a", fsm)
    m._grammars["b"] = (1, fsm)
    with pytest.raises(ValueError, match=r"all 2 grammar slots are in use \(\['a', 'b'\]\)"):
        m.load_grammar("c", fsm)
    assert m.grammars == ["a", "b"] and m._grammar_index("b") == 1 and m._grammar_index(None) == -1 and m.grammar("a") is fsm


class _Tok:
    """encode() of the image block only: ids 400 .. 465, as the miniature's tokenizer has them."""
    eos_token_id = 2

    def encode(self, text, add_special_tokens=False):
        return list(range(400, 400 + text.count("<img")  + text.count("</img>")))


def test_engines_refuse_before_touching_anything():
    """A stand-in LLM that has nothing but what the refusals look at: had anything else been touched, an AttributeError would show."""
    from seedx_amd.seed_x import ContinuousLVLM
    good = TokenFSM.from_choices([(3, 4)], 500)
    ok, con = dict(input_ids=[[1, 2]]), dict(input_ids=[[1, 2]], grammar="g")

    def agent(world=1, max_grammars=1, resident=("g",), fsm=good):
        llm = types.SimpleNamespace(comm=types.SimpleNamespace(world=world), V=500, max_grammars=max_grammars, grammars=sorted(resident),
                                    grammar=lambda n: fsm)
        return ContinuousLVLM(llm, None, None)
    for name in ("generate_batch", "generate_inflight"):
        with pytest.raises(ValueError, match="built with.*max_grammars=0"):
            getattr(agent(max_grammars=0), name)(None, [ok, con])
        with pytest.raises(ValueError, match="request 1 names the unknown grammar 'h' \\(resident: \\['g'\\]\\)"):
            getattr(agent(), name)(None, [ok, dict(con, grammar="h")])
        with pytest.raises(ValueError, match="grammar.*on tp=2 tensor-parallel ranks is not built \\(follow-up"):
            getattr(agent(world=2), name)(None, [ok, con])
        with pytest.raises(ValueError, match="request 1 carries a grammar but its prompt ends inside the image block \\(id 401\\).*follow-up"):
            getattr(agent(), name)(_Tok(), [ok, dict(con, input_ids=[[1, 401]])])
        with pytest.raises(ValueError, match="grammar 'g' admits ids of the image block \\(follow-up\\)"):
            getattr(agent(fsm=TokenFSM.from_choices([(3, 465)], 500)), name)(_Tok(), [ok, con])
    with pytest.raises(ValueError, match="request 1 carries a grammar and force_image_at.*follow-up"):
        agent().generate_batch(None, [ok, con], force_image_at=2)
    with pytest.raises(ValueError, match="request 1 carries a grammar and force_image_at.*follow-up"):
        agent().generate_inflight(None, [ok, dict(con, force_image_at=2)])
    spec = agent()
    spec.speculative = True
    with pytest.raises(ValueError, match="grammar.*with agent.speculative is not built \\(follow-up"):
        spec.generate_inflight(None, [ok, con])
    one = agent()
    one.llm.G = 1
    with pytest.raises(ValueError, match="names the unknown grammar 'zz'"):
        one.generate(None, input_ids=[[1, 2]], grammar="zz")
    # no request names a grammar: nothing of the above is looked at
    bare = ContinuousLVLM(object(), None, None)
    assert bare._grammar_names("generate_batch", [ok, ok], [False, False]) == [None, None]
    src = open(os.path.join(ROOT, "seed-x_amd", "llama.py")).read()
    assert "a grammar in the verify step of speculative decoding" in src and "grammars on tp={self.tp}" in src
