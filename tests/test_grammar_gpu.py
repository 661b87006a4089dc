"""Constrained decoding on the device (sx_next_b_fsm / sx_next_slots_fsm) against the numpy rule of seedx_amd.grammar (constrain_row,
advance): everything here is torch.equal or an exact list. The working rows are compared with the rule bit for bit; ids, counters,
status, n_kept and p_chosen with the EXISTING tails run on the numpy-edited rows — with an image-id list on which the processor rule is
the identity (two ids: the first is never a previous id, the second names a padding column that holds exactly 0.0 in the input) —; the
LP records with sx_token_logprobs of the RAW rows; rows without an automaton with sx_next_b_ctl / sx_next_slots_ctl on the same input."""
import re

import numpy as np
import pytest
import torch

from seedx_amd.grammar import DONE, TokenFSM, advance, constrain_row
from seedx_amd.sampling import ControlParams, count_words
from tests.test_controls_gpu import EOS, NINF, Ctl, _bits, _edited, _sample_params
from tests.test_inflight_gpu import IMG_IDS, KW, _i32, _req
from tests.test_logprobs_gpu import PROMPT, Rec, _agent
from tests.test_models_gpu import StubTokenizer

WIDTHS = [(33, 64), (500, 512), (32330, 32384)]
N_STATES = 32


def _tables(V):
    """Two automata over ids below 33 (EOS = 7 occurs in neither). Table 0: a trie with a one-id state ((11,) -> {12}), an accepting state
    that goes on ((5, 6) -> {9}) and final states; table 1: a trie over random sequences."""
    rng = np.random.default_rng(1)
    t0 = TokenFSM.from_choices([(5, 6), (5, 6, 9), (5, 8), (10,), (11, 12)], V, eos_id=EOS)
    ids = [i for i in range(min(V, 33)) if i != EOS]
    t1 = TokenFSM.from_choices([tuple(int(t) for t in rng.choice(ids, size=int(rng.integers(1, 5)))) for _ in range(6)] + [(3,), (3, 4)], V,
                               eos_id=EOS)
    return [t0, t1]


class Fsm:
    """A grammar state as ops takes it (what llama.GrammarState holds)."""

    def __init__(self, dev, fsms, table, state, ld_v, n_states=N_STATES):
        imgs = [f.table(n_states, ld_v) for f in fsms]
        self.trans = torch.from_numpy(np.stack([t for t, _ in imgs])).to(dev)
        self.flags = torch.from_numpy(np.stack([f for _, f in imgs])).to(dev)
        self.table, self.state = _i32(table, dev), _i32(state, dev)


def _identity_img(V, dev):
    return _i32([V + 2, V + 1], dev)          # V + 2: never a previous id; V + 1: a padding column that holds 0.0


G1 = 24


def _lock_case(V, ld):
    g = torch.Generator().manual_seed(7)
    rng = np.random.default_rng(7)
    logits = torch.randn(G1, ld, generator=g) * 3
    logits[:, V:] = float("nan")
    logits[:, V + 1] = 0.0
    fsms = _tables(V)
    t0, t1 = fsms
    s5, s56, s11 = t0.walk((5,))[0], t0.walk((5, 6))[0], t0.walk((11,))[0]
    s3 = t1.walk((3,))[0]
    #        one-id   EOS is the raw arg-max  accepting: EOS wins  enters final    accepting, goes on
    table = [0,       0,                      0,                   0,              0,     0, 0, 0, 1, 1,  1, 1,  1, 1, 1, 1, -1, 0,    1, -1, 0, 1, 0, 1]
    state = [s11,     0,                      s56,                 s5,             s56,   0, s5, s11, 0, s3, 0, s3, 1, 2, 3, 4, 0, DONE, 0, 5, 0, 2, s5, s3]
    logits[1, EOS] = logits[2, EOS] = 50.0
    logits[1, 5] = 30.0
    logits[3, 8] = 40.0
    logits[9, EOS] = 45.0                                                    # table 1, accepting (3,): EOS
    prev = [40 + r for r in range(G1)]
    tok = [int(t) for t in rng.integers(0, 6, size=G1)]
    counts = np.stack([count_words(V, rng.integers(0, V, size=12), rng.integers(0, min(V, 33), size=int(rng.integers(1, 30)))) for _ in range(G1)])
    P = ControlParams
    params = [None] * G1
    params[4] = P(min_new_tokens=9, logit_bias={9: 1.0})                     # accepting, but min_new_tokens masks EOS: 9 is all that is left
    tok[4] = 2
    logits[4, EOS] = 50.0
    params[5] = P(repetition_penalty=1.4, frequency_penalty=0.3)
    params[6] = P(logit_bias={6: NINF})                                      # controls ban an admissible id
    params[10] = P(presence_penalty=0.6, logit_bias={3: 2.0})
    params[12] = P(repetition_penalty=0.8)
    params[16] = P(repetition_penalty=1.3, logit_bias={2: 1.0})              # controls, table = -1
    params[17] = P(frequency_penalty=0.2)                                    # controls, DONE
    params[22] = P(repetition_penalty=1.2, presence_penalty=0.2, frequency_penalty=0.1, logit_bias={8: -3.0, 6: 0.5})
    return logits, fsms, table, state, prev, tok, counts, params


def _constrained(table, state):
    return [t >= 0 and s >= 0 for t, s in zip(table, state)]


def _final_rows(logits, V, fsms, table, state, counts, params, tok):
    """The rows the id functions see: apply_controls, then constrain_row on the constrained rows."""
    out = _edited(logits, V, counts, params, tok, EOS)
    for r, on in enumerate(_constrained(table, state)):
        if on:
            out[r, :V] = torch.from_numpy(constrain_row(out[r, :V].numpy(), fsms[table[r]], state[r], EOS))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("sampled,lp_n", [(False, None), (True, None), (True, 3)], ids=["greedy", "sampled", "sampled-lp3"])
@pytest.mark.parametrize("V,ld", WIDTHS)
def test_lockstep_form(dev, V, ld, sampled, lp_n):
    from seedx_amd import ops
    logits, fsms, table, state, prev, tok, counts, params = _lock_case(V, ld)
    con = _constrained(table, state)
    final = _final_rows(logits, V, fsms, table, state, counts, params, tok)
    img, rows = _identity_img(V, dev), 8
    step = _i32(tok, dev)

    def launch(fsm_on):
        dl, cur = logits.to(dev), _i32(prev, dev)
        out = torch.full((G1, rows), -1, dtype=torch.int32, device=dev)
        ctl = Ctl(dev, params, counts, ld)
        sp = _sample_params(dev, G1) if sampled else None
        rec = Rec(dev, [int(r % 5 != 4) for r in range(G1)], rows, lp_n) if lp_n is not None else None
        kw = dict(sample=sp, lp=rec, token_index=step, eos_id=EOS, **(dict(n_kept=sp.n_kept, p_chosen=sp.p_chosen) if sampled else {}))
        fs = Fsm(dev, fsms, table, state, ld)
        if fsm_on:
            ops.next_b_fsm(dl, V, img, cur, out, step, ctl, fs, **kw)
        else:
            ops.next_b_ctl(dl, V, img, cur, out, step, ctl, **kw)
        torch.cuda.synchronize()
        return dl, cur, out, ctl, sp, rec, fs
    # ---- the oracle: the parent's tail on the numpy-edited rows
    ref_l, ref_cur = final.to(dev), _i32(prev, dev)
    ref_out = torch.full((G1, rows), -1, dtype=torch.int32, device=dev)
    if sampled:
        rp = _sample_params(dev, G1)
        ops.sample_next_b(ref_l, V, img, ref_cur, ref_out, step, rp, token_index=step, n_kept=rp.n_kept, p_chosen=rp.p_chosen)
    else:
        ops.greedy_next_b(ref_l, V, img, ref_cur, ref_out, step)
    plain = launch(False)
    dl, cur, out, ctl, sp, rec, fs = launch(True)
    emitted = cur.tolist()
    assert torch.equal(cur, ref_cur) and torch.equal(out, ref_out)
    if sampled:
        assert torch.equal(sp.n_kept, rp.n_kept) and torch.equal(_bits(sp.p_chosen), _bits(rp.p_chosen))
        assert (sp.n_kept[:16] > 1).any() and sp.n_kept[0].item() in (1, -1)
    else:
        assert emitted == [int(np.argmax(final[r, :V].numpy())) for r in range(G1)]
        assert emitted[1] == 5 and emitted[2] == EOS and emitted[3] == 8 and emitted[4] == 9 and emitted[9] == EOS
    assert emitted[0] == 12                                                  # the one-id state, greedy or drawn
    for r in range(G1):
        if con[r]:
            assert emitted[r] == EOS or fsms[table[r]].trans[state[r], emitted[r]] >= 0, r
            assert torch.equal(_bits(ctl.work[r, :V].cpu()), _bits(final[r, :V])), r
            assert torch.equal(_bits(dl[r].cpu()), _bits(logits[r])), r      # the logits row stays raw, padding included
        else:                                                                # bit for bit sx_next_b_ctl: logits row, working row
            assert torch.equal(_bits(dl[r]), _bits(plain[0][r])) and torch.equal(_bits(ctl.work[r]), _bits(plain[3].work[r])), r
            assert plain[1][r].item() == emitted[r] and torch.equal(out[r], plain[2][r])
    want_state = [advance(fsms[table[r]], state[r], emitted[r], EOS) if con[r] else state[r] for r in range(G1)]
    assert fs.state.tolist() == want_state and fs.table.tolist() == table
    assert want_state[0] == DONE and want_state[4] == DONE                   # entered a final state
    if not sampled:
        assert want_state[2] == DONE and want_state[3] == DONE and want_state[1] == fsms[0].walk((5,))[0]
    exp = counts.copy()
    for r in range(G1):
        if params[r] is not None:
            exp[r, emitted[r]] += 1
    assert np.array_equal(ctl.counts[:, :V].cpu().numpy(), exp)              # counts grow only on rows with on != 0
    if rec is not None:
        c, ti, tv = ops.token_logprobs(logits.to(dev), V, cur, lp_n)
        for r in range(G1):
            got = (rec.chosen[r, tok[r]], rec.top_ids[r, tok[r]], rec.top[r, tok[r]])
            if r % 5 == 4:
                assert (rec.chosen[r] == -7.0).all() and (rec.top_ids[r] == -9).all()
            else:
                assert torch.equal(_bits(got[0]), _bits(c[r])) and torch.equal(got[1], ti[r]) and torch.equal(_bits(got[2]), _bits(tv[r])), r


G2 = 10


@pytest.mark.gpu
@pytest.mark.parametrize("sampled,lp_n", [(False, None), (True, None), (True, 2)], ids=["greedy", "sampled", "sampled-lp2"])
@pytest.mark.parametrize("V,ld", [(500, 512), (32330, 32384)])
def test_slot_form(dev, V, ld, sampled, lp_n):
    """Ten slots: live constrained (0, 1, 6, 9), parked (2: nothing is written, its state included), live unconstrained (3, and 8 with
    controls), one that stops by entering a final state (4), one that stops on EOS in an accepting state (5), one that stops on its
    budget mid-grammar (7)."""
    from seedx_amd import ops
    g = torch.Generator().manual_seed(21)
    rng = np.random.default_rng(21)
    logits = torch.randn(G2, ld, generator=g) * 3
    logits[:, V:] = float("nan")
    logits[:, V + 1] = 0.0
    fsms = _tables(V)
    t0, t1 = fsms
    s5, s56, s11, s3 = t0.walk((5,))[0], t0.walk((5, 6))[0], t0.walk((11,))[0], t1.walk((3,))[0]
    table = [0, 1, 0, -1, 0, 0, 1, 0, -1, 1]
    state = [0, 0, s5, 0, s11, s56, s3, s5, 0, 2]
    logits[5, EOS] = 60.0
    live = [1, 1, 0, 1, 1, 1, 1, 1, 1, 1]
    stepv = [0, 3, 2, 5, 1, 4, 3, 2, 6, 2]
    n_new = [1, 4, 3, 6, 2, 5, 4, 3, 7, 3]
    max_new = [100, 100, 100, 100, 100, 100, 100, 4, 100, 100]               # slot 7 reaches its budget (s5 -> 6 is accepting, not final)
    logits[7, 6] = 55.0
    force_at = [-1] * G2
    prev = [40 + r for r in range(G2)]
    pos = [20 + r for r in range(G2)]
    counts = np.stack([count_words(V, rng.integers(0, V, size=12), rng.integers(0, 33, size=int(rng.integers(1, 30)))) for _ in range(G2)])
    P = ControlParams
    params = [None, P(repetition_penalty=1.3, frequency_penalty=0.2), P(presence_penalty=0.4), None, P(logit_bias={3: 1.0}), None,
              P(presence_penalty=0.5, min_new_tokens=9), None, P(repetition_penalty=1.5), None]
    con = [bool(l) and c for l, c in zip(live, _constrained(table, state))]
    final = _edited(logits, V, counts, params, stepv, EOS)
    for r in range(G2):
        if con[r]:
            final[r, :V] = torch.from_numpy(constrain_row(final[r, :V].numpy(), fsms[table[r]], state[r], EOS))
    img = _identity_img(V, dev)

    def run(rows_t, mode):
        t = dict(cur=_i32(prev, dev), live=_i32(live, dev), n_new=_i32(n_new, dev), max_new=_i32(max_new, dev), force_at=_i32(force_at, dev),
                 pos=_i32(pos, dev), ctx=_i32([p + 1 for p in pos], dev), step=_i32(stepv, dev))
        out = torch.full((G2, 8), -1, dtype=torch.int32, device=dev)
        status = torch.full((G2, 4), -5, dtype=torch.int32, device=dev)
        sp = _sample_params(dev, G2, seed=9) if sampled else None
        skw = dict(n_kept=sp.n_kept, p_chosen=sp.p_chosen) if sampled else {}
        args = (rows_t, V, img, t["cur"], t["live"], t["n_new"], t["max_new"], t["force_at"], t["pos"], t["ctx"], t["step"], out, status)
        extra = {}
        if mode == "oracle":
            if sampled:
                ops.sample_next_slots(*args, sp, force_id=400, eos_id=EOS, **skw)
            else:
                ops.greedy_next_slots(*args, force_id=400, eos_id=EOS)
        else:
            ctl = Ctl(dev, params, counts, ld)
            rec = Rec(dev, [1] * G2, 8, lp_n) if lp_n is not None else None
            fs = Fsm(dev, fsms, table, state, ld)
            if mode == "fsm":
                ops.next_slots_fsm(*args, ctl, fs, sample=sp, lp=rec, force_id=400, eos_id=EOS, **skw)
            else:
                ops.next_slots_ctl(*args, ctl, sample=sp, lp=rec, force_id=400, eos_id=EOS, **skw)
            extra = dict(ctl=ctl, rec=rec, fs=fs, logits=rows_t)
        torch.cuda.synchronize()
        t.update(out=out, status=status)
        if sampled:
            t.update(n_kept=sp.n_kept, p_chosen=_bits(sp.p_chosen))
        return t, extra
    ref, _ = run(final.to(dev), "oracle")
    plain, pe = run(logits.to(dev), "ctl")
    got, ge = run(logits.to(dev), "fsm")
    emitted = got["cur"].tolist()
    want_state = [advance(fsms[table[r]], state[r], emitted[r], EOS) if con[r] else state[r] for r in range(G2)]
    assert ge["fs"].state.tolist() == want_state and want_state[2] == s5     # the parked slot's state is not written
    for r in range(G2):
        stopped_by_grammar = con[r] and want_state[r] == DONE and emitted[r] != EOS and n_new[r] + 1 < max_new[r]
        for k in ref:
            if stopped_by_grammar and k in ("live", "pos", "ctx", "step", "status"):
                continue
            assert torch.equal(ref[k][r], got[k][r]), (k, r)
        if stopped_by_grammar:                                               # parks itself exactly as on EOS or budget
            n = n_new[r] + 1
            assert [got[k][r].item() for k in ("live", "step", "pos", "ctx")] == [0, -1, -1, 0]
            assert got["status"][r].tolist() == [emitted[r], 0, n, n]
        if not con[r]:                                                       # bit for bit sx_next_slots_ctl
            for k in plain:
                assert torch.equal(plain[k][r], got[k][r]), (k, r)
            assert torch.equal(_bits(ge["logits"][r]), _bits(pe["logits"][r])) and torch.equal(_bits(ge["ctl"].work[r]), _bits(pe["ctl"].work[r]))
        else:
            assert torch.equal(_bits(ge["ctl"].work[r, :V].cpu()), _bits(final[r, :V])), r
            assert torch.equal(_bits(ge["logits"][r].cpu()), _bits(logits[r])), r
    assert emitted[4] == 12 and got["live"][4].item() == 0 and got["status"][4].tolist() == [12, 0, 3, 3]      # entered a final state
    assert got["status"][2].tolist() == [-5] * 4 and (ge["ctl"].work[2] == -123.0).all() and got["cur"][2].item() == prev[2]
    if not sampled:
        assert got["status"][5].tolist() == [EOS, 0, 6, 6] and want_state[5] == DONE                             # EOS in an accepting state
        assert got["status"][7].tolist() == [6, 0, 4, 4] and want_state[7] == s56                                # budget, mid-grammar
    exp = counts.copy()
    for r in range(G2):
        if live[r] and params[r] is not None:
            exp[r, emitted[r]] += 1
    assert np.array_equal(ge["ctl"].counts[:, :V].cpu().numpy(), exp)
    if lp_n is not None:
        c, ti, tv = ops.token_logprobs(logits.to(dev), V, _i32([e if l else 0 for e, l in zip(emitted, live)], dev), lp_n)
        rec = ge["rec"]
        for r in range(G2):
            if not live[r]:
                assert (rec.chosen[r] == -7.0).all()
            else:
                got_r = (rec.chosen[r, stepv[r]], rec.top_ids[r, stepv[r]], rec.top[r, stepv[r]])
                assert torch.equal(_bits(got_r[0]), _bits(c[r])) and torch.equal(got_r[1], ti[r]) and torch.equal(_bits(got_r[2]), _bits(tv[r])), r


@pytest.mark.gpu
def test_refusals_on_the_device_side(dev):
    """The entry points refuse ld_v < vocab and an odd ld_v; a table index or a state outside the resident tables never reaches them: the
    row runs unconstrained (what sx_next_b_ctl does with it) and its state is left alone."""
    from seedx_amd import ops
    V, ld = 33, 64
    logits = torch.randn(2, ld, generator=torch.Generator().manual_seed(0))
    logits[:, V + 1] = 0.0
    fsms = _tables(V)
    args = lambda: (logits.to(dev), V, _identity_img(V, dev), _i32([40, 41], dev), None, _i32([0, 0], dev),
                    Ctl(dev, [None, None], np.zeros((2, V), np.int32), ld))
    for ld_v in (32, 63):
        fs = Fsm(dev, fsms, [0, 1], [0, 0], ld)
        fs.trans = fs.trans[:, :, :ld_v].contiguous()
        with pytest.raises(RuntimeError, match=f"ld_v={ld_v} must be even and >= vocab=33"):
            ops.next_b_fsm(*args(), fs)
    a, b = args(), args()
    fs = Fsm(dev, fsms, [2, 0], [0, N_STATES], ld)                           # table index 2 of 2; state 32 of 32
    ops.next_b_fsm(*a, fs)
    ops.next_b_ctl(*b)
    torch.cuda.synchronize()
    assert torch.equal(a[3], b[3]) and torch.equal(_bits(a[0]), _bits(b[0])) and fs.state.tolist() == [0, N_STATES]


# ---- model -------------------------------------------------------------------------------------------------------------------------
IMG16 = IMG_IDS[:1] + IMG_IDS[1:17] + IMG_IDS[-1:]
INT = rb"-?(0|[1-9][0-9]{0,3})"
WORD = rb"[a-z]{60}"
CHOICES = [(41,), (42,), (13,), (14,)]                                       # "yes", "no", "a", "b"


def _byte_vocab():
    """Bytes for the miniature's 500 ids: 0 .. 2 special, 3 .. 12 the digits, 13 .. 38 a .. z, then punctuation, "yes" / "no", the numbers
    10 .. 99 and random lower-case pieces of 2 or 3 bytes; 398 and above (the patch and image tokens) are added tokens."""
    rng = np.random.default_rng(3)
    vocab = [None] * 3 + [bytes([48 + i]) for i in range(10)] + [bytes([97 + i]) for i in range(26)]
    vocab += [b" ", b"-", b"yes", b"no", b"{", b"}", b'"', b":", b","] + [str(i).encode() for i in range(10, 100)]
    seen = set(vocab)
    while len(vocab) < 398:
        p = bytes(rng.integers(97, 123, size=int(rng.integers(2, 4))).astype(np.uint8))
        if p not in seen:
            seen.add(p)
            vocab.append(p)
    return vocab + [None] * 102


def _grammars(eos=2):
    vocab = _byte_vocab()
    kw = dict(eos_id=eos, banned_ids=IMG_IDS)
    return vocab, {"int": TokenFSM.from_regex(INT, vocab, **kw), "word": TokenFSM.from_regex(WORD, vocab, **kw),
                   "choice": TokenFSM.from_choices(CHOICES, 500, **kw)}


def _slot_run(dev, agent, names, use_graph, steps=12):
    """Three slots of the miniature through prefill + ``steps`` slot steps. ``names``: per-slot grammar names / None, or None for a slot
    state without a GrammarState."""
    from seedx_amd import ops
    llm = agent.llm
    llm.reset()
    P = llm._pack()
    G, rows = 3, 16
    img = _i32(IMG16, dev)
    st = llm.slot_state(force_id=400, eos_id=-1, **(dict(grammar=True) if names is not None else {}))
    out_ids = torch.full((G, rows), -1, dtype=torch.int32, device=dev)
    hid = torch.zeros((G, rows, llm.H), dtype=torch.float32, device=dev)
    prompts = [[1, 10 + g] + [20 + g + i for i in range(3 + g)] for g in range(G)]
    xs = [ops.embedding(_i32(p, dev), P["embed"]) for p in prompts]
    llm._slot_write(P["pos"], range(G), 0)
    llm._slot_write(P["ctx"], range(G), 1)
    logits, _ = llm.forward_embeds_batch(xs, list(range(G)))
    first = _i32([p[-1] for p in prompts], dev)
    if names is not None:
        assert st.controls is not None and st.grammar.table.tolist() == [-1] * G
        st.grammar.set_rows(range(G), names)
        part = st.grammar.gather(range(G))
        zero = torch.zeros(G, dtype=torch.int32, device=dev)
        ops.next_b_fsm(logits.contiguous(), llm.V, img, first, None, zero, st.controls.gather(range(G)), part, token_index=zero)
        st.grammar.scatter(range(G), part)
    else:
        assert st.grammar is None and st.controls is None
        ops.greedy_next_b(logits.contiguous(), llm.V, img, first, None, None)
    P["cur"].copy_(first)
    out_ids[:, 0] = first
    P["step"].fill_(1)
    st.n_new.fill_(1)
    st.max_new.fill_(100)
    st.live.fill_(1)
    for _ in range(steps):
        llm.decode_step(img, out_ids, hid, use_graph=use_graph, slots=st)
    torch.cuda.synchronize()
    res = out_ids.clone(), hid.clone(), st.live.clone(), (st.grammar.state.clone() if names is not None else None)
    llm.reset()
    return res


@pytest.mark.gpu
def test_model_eager_equals_graph_and_resident_table(dev):
    agent = _agent(dev, torch.float16, 3, max_grammars=2, grammar_states=64)
    llm = agent.llm
    vocab, gr = _grammars()
    two = TokenFSM.from_choices([(41, 13, 14), (42, 13)], 500, eos_id=2, banned_ids=IMG_IDS)
    assert llm.load_grammar("word", gr["word"]) == 0 and llm.load_grammar("two", two) == 1 and llm.grammars == ["two", "word"]
    assert llm.memory_footprint()["grammars"] == 2 * 64 * (llm.Vpad * 2 + 4)
    names = ["word", "two", None]
    plain = _slot_run(dev, agent, None, True)
    assert llm._slot_graph is not None and llm._slot_graph_fsm is None and llm._slot_graph_ctl is None
    eager = _slot_run(dev, agent, names, False)
    assert llm._slot_graph_fsm is None
    graph = _slot_run(dev, agent, names, True)
    assert llm._slot_graph_fsm is not None and llm._slot_graph_ctl is None
    for a, b in zip(eager, graph):
        assert torch.equal(a, b)
    ids, hid, live, state = graph
    word = ids[0, :13].tolist()
    assert all(13 <= t < 398 and vocab[t].isalpha() for t in word) and live[0].item() == 1 and state[0].item() == gr["word"].walk(word)[0]
    got = [t for t in ids[1].tolist() if t >= 0]
    assert tuple(got) in ((41, 13, 14), (42, 13)) and live[1].item() == 0 and state[1].item() == DONE     # parked itself on the final state
    assert torch.equal(ids[2], plain[0][2]) and torch.equal(hid[2], plain[1][2])                        # the slot without a grammar
    # ---- unload / reload into the same index, in place
    T = llm._P["grammar"]
    ptr = T["trans"].data_ptr()
    llm.unload_grammar("two")
    assert llm.grammars == ["word"] and (T["trans"][1] == -1).all() and (T["flags"][1] == 0).all()
    assert llm.load_grammar("int", gr["int"]) == 1 and T["trans"].data_ptr() == ptr
    t, f = gr["int"].table(64, llm.Vpad)
    assert torch.equal(T["trans"][1].cpu(), torch.from_numpy(t)) and torch.equal(T["flags"][1].cpu(), torch.from_numpy(f))
    with pytest.raises(ValueError, match="all 2 grammar slots are in use"):
        llm.load_grammar("choice", gr["choice"])
    with pytest.raises(ValueError, match="unknown grammar 'two'"):
        llm.grammar_state(fresh=True).set_rows([0], ["two"])
    with pytest.raises(ValueError, match="a slot state carries its own grammar state"):
        llm.decode_step(None, None, None, slots=llm.slot_state(force_id=400, grammar=True), grammar=llm.grammar_state())
    llm.reset()


# ---- engines -----------------------------------------------------------------------------------------------------------------------
def _check(res, fsm, pattern, vocab, budget, name):
    ids = res["generate_ids"].tolist()
    assert res["grammar"]["name"] == name and 1 <= len(ids) <= budget
    text = b"".join(vocab[t] for t in ids if t != 2)
    if res["grammar"]["complete"]:
        assert re.fullmatch(pattern, text), (ids, text)
    else:
        assert len(ids) == budget, ids
    assert fsm.walk([t for t in ids if t != 2])[1] == len([t for t in ids if t != 2])               # every id was admissible
    return ids


def _loaded_agent(dev, G, gr, **kw):
    agent = _agent(dev, torch.float16, G, max_grammars=3, grammar_states=64, **kw)
    for name, fsm in gr.items():
        agent.llm.load_grammar(name, fsm)
    return agent


@pytest.mark.gpu
def test_engines(dev):
    tok, n = StubTokenizer(), 12
    vocab, gr = _grammars()
    a3, a1 = _loaded_agent(dev, 3, gr), _loaded_agent(dev, 1, gr)
    others = [_req(1, n), _req(2, n)]
    queue = [_req(0, 9), dict(input_ids=[PROMPT], max_new_tokens=n), _req(2, 7), _req(3, 10), _req(4, 6)]
    queue[0].update(do_sample=True, top_p=0.9, seed=11)
    quiet = a3.generate_inflight(tok, queue, **KW)
    assert a3.llm._slot_sample_graph is not None and a3.llm._slot_sample_graph_fsm is None
    assert "state_sampled" in a3._inflight and not any(k.endswith("_fsm") for k in a3._inflight)
    assert all("grammar" not in r for r in quiet)
    for extra in (dict(), dict(do_sample=True, temperature=1.3, top_k=0, top_p=0.95, seed=7)):
        req = dict(input_ids=[PROMPT], grammar="int", **extra)
        batch = a3.generate_batch(tok, [req] + others, max_new_tokens=n, **KW)
        want = _check(batch[0], gr["int"], INT, vocab, n, "int")
        assert batch[0]["grammar"]["complete"] and "grammar" not in batch[1]
        single = a1.generate(tok, input_ids=[PROMPT], max_new_tokens=n, grammar="int", **extra, **KW)
        assert single["generate_ids"].tolist() == want and single["grammar"] == batch[0]["grammar"]
        for at in (1, 3):                                                    # different slots, different neighbours
            busy_q = [dict(q) for q in queue]
            busy_q[at] = dict(req, max_new_tokens=n)
            busy = a3.generate_inflight(tok, busy_q, **KW)
            assert busy[at]["generate_ids"].tolist() == want and busy[at]["grammar"] == batch[0]["grammar"]
            for r in range(5):
                if r != at:                                                  # the unconstrained requests: the queue run without the key
                    assert torch.equal(quiet[r]["generate_ids"], busy[r]["generate_ids"]), r
                    assert torch.equal(quiet[r]["last_hidden_states"], busy[r]["last_hidden_states"]), r
                    assert "grammar" not in busy[r]
    assert a3.llm._graph_fsm is not None and a3.llm._sample_graph_fsm is not None and a3.llm._slot_sample_graph_fsm is not None
    assert any(k.endswith("_fsm") for k in a3._inflight)
    plain = a3.generate_batch(tok, [dict(input_ids=[PROMPT])] + others, max_new_tokens=n, **KW)
    assert "grammar" not in plain[0] and a3.llm._graph is not None
    # ---- a budget that runs out mid-grammar; EOS in an accepting state; a four-way choice
    short = a3.generate_batch(tok, [dict(input_ids=[PROMPT], grammar="word")] + others, max_new_tokens=6, **KW)[0]
    assert _check(short, gr["word"], WORD, vocab, 6, "word") and short["grammar"]["complete"] is False and len(short["generate_ids"]) == 6
    eosq = a3.generate_inflight(tok, [dict(input_ids=[PROMPT], grammar="int", max_new_tokens=n), _req(1, 5)], **dict(KW, eos_token_id=2))
    _check(eosq[0], gr["int"], INT, vocab, n, "int")
    pick = a1.generate(tok, input_ids=[PROMPT], max_new_tokens=n, grammar="choice", **KW)
    scores = a1.score(tok, [dict(input_ids=[PROMPT], continuations=[list(c) for c in CHOICES])])[0]
    best = CHOICES[int(np.argmax([float(s["token_logprobs"][0]) for s in scores]))]
    assert tuple(pick["generate_ids"].tolist()) == best and pick["grammar"] == {"name": "choice", "complete": True}
    four = a3.generate_inflight(tok, [dict(input_ids=[PROMPT], grammar="choice", max_new_tokens=n, do_sample=True, seed=s) for s in range(4)], **KW)
    assert all(tuple(r["generate_ids"].tolist()) in CHOICES and r["grammar"]["complete"] for r in four)


@pytest.mark.gpu
def test_engines_with_logprobs_controls_adapter_and_pages(dev):
    from tests.test_kv_paged_gpu import _adapter
    tok, n = StubTokenizer(), 10
    vocab, gr = _grammars()
    outs = []
    for kw in (dict(), dict(kv_pages=24, kv_page_size=32)):
        agent = _loaded_agent(dev, 3, gr, max_adapters=1, lora_rank=8, **kw)
        agent.llm.load_adapter("a", _adapter(torch.Generator().manual_seed(8)), lora_alpha=32)
        queue = [dict(input_ids=[PROMPT], grammar="int", logprobs=2, max_new_tokens=n),
                 dict(input_ids=[PROMPT], grammar="word", repetition_penalty=1.4, logit_bias={13: NINF}, max_new_tokens=n),
                 dict(input_ids=[PROMPT], grammar="int", adapter="a", max_new_tokens=n), _req(3, 6),
                 dict(input_ids=[PROMPT], grammar="choice", do_sample=True, seed=3, logprobs=1, min_new_tokens=2, max_new_tokens=n)]
        res = agent.generate_inflight(tok, queue, **KW)
        outs.append(res)
        _check(res[0], gr["int"], INT, vocab, n, "int")
        ids = _check(res[1], gr["word"], WORD, vocab, n, "word")
        assert 13 not in ids and res[1]["controls"]["repetition_penalty"] == 1.4
        _check(res[2], gr["int"], INT, vocab, n, "int")
        assert res[2]["adapter"] == "a" and "grammar" not in res[3]
        assert tuple(res[4]["generate_ids"].tolist()) in CHOICES and res[4]["grammar"]["complete"]
        lp = res[0]["logprobs"]
        assert lp["token_ids"].tolist() == res[0]["generate_ids"].tolist() and torch.isfinite(lp["token_logprobs"]).all()
        assert (lp["token_logprobs"] <= lp["top_logprobs"][:, 0]).all()      # the records are of the RAW row: the top id need not be admissible
    for a, b in zip(*outs):                                                  # the paged model: the contiguous model's ids
        assert torch.equal(a["generate_ids"], b["generate_ids"])
