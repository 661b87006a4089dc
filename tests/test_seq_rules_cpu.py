"""Stop sequences and no_repeat_ngram_size, host side: the rules the tail kernel is held to (seedx_amd.sampling.ngram_banned /
apply_no_repeat / stop_match), the request keys (SeqParams.from_request), every refusal of the engines, and the C-ABI of the two new
entry points."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from seedx_amd import sampling
from seedx_amd.sampling import SeqParams, apply_no_repeat, ngram_banned, stop_match

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_ngram_banned_against_transformers():
    """The 270-case grid: n in {1, 2, 3, 4, 8} x L in {0, 1, 2, 3, 7, 8, 9, 40, 300} x 6 draws over an alphabet of 5 ids, against
    transformers' NoRepeatNGramLogitsProcessor on one decoder-only sequence."""
    transformers = pytest.importorskip("transformers")
    import torch
    rng = np.random.default_rng(0)
    cases = 0
    for n in (1, 2, 3, 4, 8):
        proc = transformers.NoRepeatNGramLogitsProcessor(n)
        for L in (0, 1, 2, 3, 7, 8, 9, 40, 300):
            for _ in range(6):
                hist = rng.integers(0, 5, size=L).tolist()
                out = proc(torch.tensor(hist, dtype=torch.long).reshape(1, L), torch.zeros(1, 5))
                ref = set(torch.nonzero(out[0] == float("-inf")).reshape(-1).tolist())
                assert ngram_banned(hist, n) == ref, (n, L, hist)
                cases += 1
    assert cases == 270


def test_ngram_banned_by_hand():
    assert ngram_banned([], 1) == set() and ngram_banned([4, 2, 4], 1) == {2, 4}          # n = 1: every id of the history
    assert ngram_banned([1, 2, 3], 0) == set()
    for n in (2, 3, 8):
        same = [7] * 20
        assert ngram_banned(same[:max(0, n - 2)], n) == set()                              # L = n - 2: the tail does not exist yet
        assert ngram_banned(same[:n - 1], n) == set()                                      # L = n - 1: a tail, but no n-gram to repeat
        assert ngram_banned(same[:n], n) == {7}                                            # L = n: the first possible ban (i = 0)
    assert ngram_banned([1, 2, 3, 1, 2], 3) == {3} and ngram_banned([1, 2, 3, 9, 2], 3) == set()
    assert ngram_banned([1, 2, 5, 1, 2, 6, 1, 2], 3) == {5, 6}
    assert ngram_banned([1, 2, 3, 1, 2], 3, vocab=3) == set() and ngram_banned([1, 2, 3, 1, 2], 3, vocab=4) == {3}     # the banned id >= V
    # a placeholder id >= V inside the matching prefix: it bans nothing itself but takes part in the comparison
    assert ngram_banned([900, 2, 3, 900, 2], 3, vocab=500) == {3} and ngram_banned([900, 2, 3, 901, 2], 3, vocab=500) == set()
    assert ngram_banned([-1, 4, -1], 2, vocab=500) == {4}


def test_apply_no_repeat_edits_nothing_else():
    x = (np.random.default_rng(1).normal(size=40) * 3).astype(F32)
    x[5] = F32(-0.0)
    hist = [3, 4, 5, 3, 4, 7, 99, 3, 4]
    y = apply_no_repeat(x, hist, 3)
    assert y.dtype == F32 and y is not x and set(np.nonzero(np.isneginf(y))[0].tolist()) == {5, 7}      # 99 lies outside the row
    keep = np.ones(40, bool)
    keep[[5, 7]] = False
    assert np.array_equal(y.view(np.uint32)[keep], x.view(np.uint32)[keep])
    assert np.array_equal(apply_no_repeat(x, hist, 0).view(np.uint32), x.view(np.uint32))


def test_stop_match():
    gen = [5, 6, 7, 8, 9, 10, 11, 12, 13]
    assert stop_match(gen, [[13]]) == 0 and stop_match(gen, [[12]]) is None                  # length 1
    assert stop_match(gen, [gen[1:]]) == 0 and stop_match(gen, [[0] + gen[2:]]) is None       # length 8
    assert stop_match(gen, [[1], [12, 13], [13]]) == 1                                       # two match at once: the lowest index
    assert stop_match([13], [[12, 13], [13]]) == 1                                           # a stop longer than the generated ids
    assert stop_match([], [[1]]) is None and stop_match(gen, []) is None
    prompt, generated = [1, 2, 3], [4, 5]
    assert stop_match(generated, [[3, 4, 5]]) is None and stop_match(generated, [[4, 5]]) == 0   # prompt tail + generated: no match


def test_seq_params():
    for req in ({}, dict(stop=None), dict(no_repeat_ngram_size=None), dict(no_repeat_ngram_size=0), dict(stop=[]),
                dict(stop=[], no_repeat_ngram_size=0)):
        assert SeqParams.from_request(req) is None
    p = SeqParams.from_request(dict(stop=[5, 6, 7], no_repeat_ngram_size=3, temperature=0.3))
    assert p.stop == ((5, 6, 7),) and p.as_dict() == {"stop": [[5, 6, 7]], "no_repeat_ngram_size": 3}
    assert SeqParams(stop=[[1], (2, 3)]).stop == ((1,), (2, 3)) and SeqParams(no_repeat_ngram_size=8).no_repeat_ngram_size == 8
    assert SeqParams(stop=[[1]] * 4, no_repeat_ngram_size=np.int64(2)).no_repeat_ngram_size == 2
    bad = [(dict(stop="\n\n"), "not strings.*tokenis"), (dict(stop=["a", "b"]), "not strings"), (dict(stop=[[1], "x"]), "not strings"),
           (dict(stop=7), "stop must be a list"), (dict(stop=[[1]] * 5), "5 sequences, at most 4"), (dict(stop=[[]]), "1 .. 8 ids, got 0"),
           (dict(stop=[list(range(9))]), "1 .. 8 ids, got 9"), (dict(stop=[[1, -2]]), "ints >= 0"), (dict(stop=[[1.5]]), "list of int token ids"),
           (dict(stop=[[1], 2]), "list of int token ids"), (dict(stop=[[True]]), "list of int token ids"),
           (dict(no_repeat_ngram_size=9), "0 .. 8"), (dict(no_repeat_ngram_size=-1), "0 .. 8"), (dict(no_repeat_ngram_size=2.0), "0 .. 8"),
           (dict(no_repeat_ngram_size=True), "0 .. 8")]
    for req, msg in bad:
        with pytest.raises(ValueError, match=msg):
            SeqParams.from_request(req)
    with pytest.raises(ValueError, match="stop id 500 lies outside the vocabulary"):
        SeqParams(stop=[[3, 500]]).check_vocab(500)
    assert SeqParams(stop=[[3, 499]]).check_vocab(500).stop == ((3, 499),)


def _stub_agent(world=1):
    from seedx_amd.seed_x import ContinuousLVLM
    llm = types.SimpleNamespace(comm=types.SimpleNamespace(world=world), V=500)
    return ContinuousLVLM(llm, None, None)


def test_engines_refuse_before_touching_anything():
    """Malformed values, agent.speculative, force_image_at on the same request and tp > 1: ValueError from a stand-in LLM that has
    nothing (``object()``) or nothing but ``comm.world`` and ``V`` — nothing else was looked at. Each message names the follow-up."""
    from seedx_amd.seed_x import ContinuousLVLM
    bare = ContinuousLVLM(object(), None, None)
    ok = dict(input_ids=[[1, 2]])
    for call in (bare.generate_batch, bare.generate_inflight):
        with pytest.raises(ValueError, match="not strings"):
            call(None, [ok, dict(ok, stop=["\n\n"])])
        with pytest.raises(ValueError, match="no_repeat_ngram_size must be an int in 0 .. 8"):
            call(None, [ok, dict(ok, no_repeat_ngram_size=12)])
    for rule in (dict(ok, stop=[[5, 6]]), dict(ok, no_repeat_ngram_size=3)):
        with pytest.raises(ValueError, match="request 1 carries stop sequences / no_repeat_ngram_size and force_image_at.*follow-up"):
            bare.generate_batch(None, [ok, rule], force_image_at=2)
        with pytest.raises(ValueError, match="request 1 carries stop sequences / no_repeat_ngram_size and force_image_at.*follow-up"):
            bare.generate_inflight(None, [ok, dict(rule, force_image_at=2)])
    bare.speculative = True
    with pytest.raises(ValueError, match="no_repeat_ngram_size with agent.speculative are not built \\(follow-up"):
        bare.generate_inflight(None, [ok, dict(ok, stop=[[5]])])
    tp = _stub_agent(world=2)
    for call in (tp.generate_batch, tp.generate_inflight):
        with pytest.raises(ValueError, match="no_repeat_ngram_size on tp=2 tensor-parallel ranks are not built \\(follow-up"):
            call(None, [ok, dict(ok, no_repeat_ngram_size=2)])
    one = _stub_agent()
    for call in (one.generate_batch, one.generate_inflight):
        with pytest.raises(ValueError, match="stop id 500 lies outside the vocabulary"):
            call(None, [dict(ok, stop=[[1, 500]])])


def test_generate_takes_the_keys_as_kwargs():
    import inspect
    from seedx_amd.seed_x import ContinuousLVLM
    sig = inspect.signature(ContinuousLVLM.generate)
    assert all(k in sig.parameters for k in sampling.SEQ_KEYS)
    agent = ContinuousLVLM(types.SimpleNamespace(G=1), None, None)
    with pytest.raises(ValueError, match="not strings"):
        agent.generate(None, input_ids=[[1, 2]], stop="\n")


def test_decode_step_refusals_are_spelled_out():
    src = open(os.path.join(ROOT, "seed-x_amd", "llama.py")).read()
    assert "no_repeat_ngram_size in the verify step of speculative" in src and "sequence rules on tp={self.tp}" in src


def test_seq_rule_struct_layout_matches_header():
    """sx_seq_rule_args: header field order == ctypes struct; the two entry points declared, bound and exported, and their argument
    lists are the _fsm entry points' plus one."""
    from seedx_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "seedx_hip.h")).read()
    cname = "sx_seq_rule_args"
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip().lstrip("*") for n in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl).split(",")]
    assert names == [f[0] for f in _lib.SeqRuleArgs._fields_], names
    assert names == ["on", "ngram", "hist", "hist_len", "prompt_len", "n_stop", "stop_len", "stop_ids", "matched", "ld_hist", "reserved"]
    assert ctypes.sizeof(_lib.SeqRuleArgs) == 9 * 8 + 2 * 4
    for name in ("sx_next_b_seq", "sx_next_slots_seq"):
        assert name in _lib.SIGNATURES and re.search(r"\bint " + name + r"\(", src)
    assert _lib.SIGNATURES["sx_next_b_seq"][:-2] == _lib.SIGNATURES["sx_next_b_fsm"][:-1]
    assert _lib.SIGNATURES["sx_next_slots_seq"][:-2] == _lib.SIGNATURES["sx_next_slots_fsm"][:-1]
    # the older structs are what they were: nothing was added to them
    assert ctypes.sizeof(_lib.LogitsCtlArgs) == 11 * 8 + 2 * 4 and ctypes.sizeof(_lib.TokenFsmArgs) == 4 * 8 + 4 * 4
    assert ctypes.sizeof(_lib.SlotStepArgs) == 12 * 8 + 8 * 4
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, n) for n in ("sx_next_b_seq", "sx_next_slots_seq"))
    assert callable(ops.next_b_seq) and callable(ops.next_slots_seq)
