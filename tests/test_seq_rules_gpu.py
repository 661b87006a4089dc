"""Device-side sequence rules (sx_next_b_seq / sx_next_slots_seq) against the numpy rules seedx_amd.sampling.apply_no_repeat /
stop_match: everything here is torch.equal or an exact list. The working rows are compared with the numpy rule bit for bit; ids, out_ids,
counters, status, n_kept and p_chosen with the EXISTING tails run on the numpy-edited rows (the same arg-max / draw code on the same bits);
the LP records with sx_token_logprobs of the RAW rows; the id history, its length and ``matched`` with the host rule. Rows with on = 0 and
parked slots are compared bit for bit with sx_next_b_ctl / sx_next_b_fsm / sx_next_slots_ctl on the same inputs."""
import numpy as np
import pytest
import torch

from seedx_amd.grammar import DONE, advance, constrain_row
from seedx_amd.sampling import ControlParams, SeqParams, apply_no_repeat, count_words, ngram_banned, stop_match
from tests.test_controls_gpu import EOS, NINF, Ctl, _bits, _edited, _sample_params, _zeroed
from tests.test_grammar_gpu import Fsm, _identity_img, _tables
from tests.test_inflight_gpu import IMG_IDS, KW, _i32, _req
from tests.test_logprobs_gpu import PROMPT, Rec, _agent
from tests.test_models_gpu import StubTokenizer

WIDTHS = [(500, 512), (32330, 32384)]
LD_HIST = 2560
SENT = -77                                                                   # what the unused part of a history row holds


class Seq:
    """A sequence-rule state as ops takes it (what llama.SeqRuleState holds), from per-row dicts(on, n, hist, prompt_len, stops)."""

    def __init__(self, dev, rows, ld_hist=LD_HIST):
        G = len(rows)
        hist = np.full((G, ld_hist), SENT, dtype=np.int32)
        for r, d in enumerate(rows):
            hist[r, :len(d["hist"])] = d["hist"]
        self.on = _i32([int(d["on"]) for d in rows], dev)
        self.ngram = _i32([d["n"] for d in rows], dev)
        self.hist = torch.from_numpy(hist).to(dev)
        self.hist_len = _i32([len(d["hist"]) for d in rows], dev)
        self.prompt_len = _i32([d["prompt_len"] for d in rows], dev)
        self.matched = torch.full((G,), -9, dtype=torch.int32, device=dev)
        self.set_stops(dev, [d.get("stops", []) for d in rows])

    def set_stops(self, dev, stops):
        self.n_stop = _i32([len(s) for s in stops], dev)
        self.stop_len = _i32([[len(q) for q in s] + [0] * (4 - len(s)) for s in stops], dev)
        self.stop_ids = _i32([[list(q) + [-1] * (8 - len(q)) for q in s] + [[-1] * 8] * (4 - len(s)) for s in stops], dev)


def _planted(rng, V, L, n):
    """A history over the whole vocabulary in which the tail (n - 1 ids) occurs at three earlier places (so something is banned)."""
    h = rng.integers(0, V, size=L).tolist()
    tail = h[L - n + 1:] if n > 1 else []
    for at in rng.integers(0, L - 2 * n, size=3).tolist():
        h[at:at + n - 1] = tail
    return h


def _lock_case(V, ld, fsm):
    """The rows of the lock-step test: n in {1, 2, 3, 8} x history lengths {0, n-2, n-1, n, 1023, 1024, 1025, 2500} over a 5-id alphabet
    (many matches, many writers per column; the 1024-thread stride runs one, two and three trips), histories over the whole vocabulary,
    a row whose raw arg-max is banned, placeholder ids >= V in the history, on = 0 rows, rows with stops only, a row inside the image
    chain (without ``fsm``), rows that also carry controls and (with ``fsm``) rows that also carry a grammar."""
    rng = np.random.default_rng(11)
    rows = []
    add = lambda n, hist, on=True, **kw: rows.append(dict(dict(on=on, n=n, hist=[int(t) for t in hist], prev=40 + len(rows), ctl=None, table=-1,
                                                               state=DONE), **kw))
    alpha = np.array([3, 4, 5, 6, 8])
    for n in (1, 2, 3, 8):
        for L in sorted({0, max(0, n - 2), n - 1, n, 1023, 1024, 1025, 2500}):
            add(n, alpha[rng.integers(0, 5, size=L)])
        for L in (1025, 2500):
            add(n, _planted(rng, V, L, n))
    grid = len(rows)
    add(2, [9, 0, 10, 9], tag="top")                                         # hist[1] becomes the row's arg-max below
    add(3, [V + 7, 9, 10, V + 7, 9], tag="placeholder_prefix")               # bans 10
    add(2, [9, V + 3, 9], tag="placeholder_banned")                          # would ban V + 3: nothing
    add(2, alpha[rng.integers(0, 5, size=60)], on=False)
    add(1, alpha[rng.integers(0, 5, size=60)], on=False, ctl=ControlParams(repetition_penalty=1.3))
    add(0, rng.integers(0, V, size=30))                                      # stops only: no working row
    add(0, rng.integers(0, V, size=30), ctl=ControlParams(presence_penalty=0.4))
    if fsm:                                                                  # table 0: state 0 admits {5, 10, 11}, the state behind 5 {6, 8}
        t0 = _tables(V)[0]
        add(1, [5, 3], table=0, state=0, tag="fsm_a")                        # 5 is banned: 10 or 11
        add(2, [5, 6, 9, 5], table=0, state=t0.walk((5,))[0], tag="fsm_b")    # 6 would repeat (5, 6): 8 is all that is left
        add(2, alpha[rng.integers(0, 5, size=40)], table=1, state=0, ctl=ControlParams(repetition_penalty=1.5, frequency_penalty=0.2))
        add(0, [1, 2], table=0, state=0)
    else:
        add(1, [432, 5], prev=431, tag="chain")                              # inside the chain: 432 is forced although it is banned
    for r in range(0, grid, 4):
        rows[r]["ctl"] = ControlParams(repetition_penalty=float(rng.uniform(0.6, 1.8)), presence_penalty=float(rng.normal() * 0.4),
                                       frequency_penalty=float(rng.normal() * 0.2), logit_bias={int(alpha[r % 5]): 2.5},
                                       min_new_tokens=int(rng.integers(0, 4)))
    G = len(rows)
    g = torch.Generator().manual_seed(21)
    logits = torch.randn(G, ld, generator=g) * 3
    logits[:, V:] = float("nan")
    logits[:, V + 1] = 0.0
    logits[:grid, alpha.tolist()] += 9.0                                     # the alphabet holds the largest values: the ban decides the id
    for r, d in enumerate(rows):
        d["L"] = len(d["hist"])
        d["prompt_len"] = int(rng.choice([0, d["L"] // 2, d["L"]]))
        if d.get("tag") == "top":
            raw = logits[r, :V].numpy().copy()
            d["hist"][1] = d["top"] = int(np.argmax(raw if fsm else _zeroed(raw, d["prev"])))
    tok = [int(t) for t in rng.integers(0, 6, size=G)]
    counts = np.stack([count_words(V, rng.integers(0, V, size=20), alpha[rng.integers(0, 5, size=int(rng.integers(1, 30)))]) for _ in range(G)])
    return rows, logits, tok, counts


def _final_rows(rows, logits, V, counts, tok, fsms):
    """The rows the id functions see: apply_controls, then apply_no_repeat, then constrain_row."""
    out = _edited(logits, V, counts, [d["ctl"] for d in rows], tok, EOS)
    for r, d in enumerate(rows):
        if d["on"] and d["n"] > 0:
            out[r, :V] = torch.from_numpy(apply_no_repeat(out[r, :V].numpy(), d["hist"], d["n"]))
        if d["table"] >= 0 and d["state"] >= 0:
            out[r, :V] = torch.from_numpy(constrain_row(out[r, :V].numpy(), fsms[d["table"]], d["state"], EOS))
    return out


def _stops_for(rows, emitted):
    """Stop sequences built from the ids the rows emit (stops do not alter ids): none, a hit of length 1, a hit at index 1, the longest
    hit the history allows (8 where it can), a stop that straddles the end of the prompt, two hits at once."""
    for r, d in enumerate(rows):
        e, h, L = emitted[r], d["hist"], d["L"]
        kind = r % 6
        if kind == 1:
            d["stops"] = [[e]]
        elif kind == 2:
            d["stops"] = [[e + 1], [e]]
        elif kind == 3:
            k = min(7, L)
            d["stops"], d["prompt_len"] = [[1, 2], h[L - k:] + [e]], max(0, L - k)
        elif kind == 4 and L >= 2:
            d["stops"], d["prompt_len"] = [h[L - 2:] + [e]], L - 1          # one id of it lies in the prompt: no match
        elif kind == 5 and L >= 1:
            d["stops"], d["prompt_len"] = [[7, 7, 7], h[L - 1:] + [e], [e]], min(d["prompt_len"], L - 1)
        else:
            d["stops"] = []
    return [stop_match(d["hist"][d["prompt_len"]:] + [emitted[r]], d["stops"]) for r, d in enumerate(rows)]


@pytest.mark.gpu
@pytest.mark.parametrize("fsm", [False, True], ids=["ctl", "fsm"])
@pytest.mark.parametrize("sampled,lp_n", [(False, None), (True, None), (False, 2), (True, 8)], ids=["greedy", "sampled", "greedy-lp", "sampled-lp"])
@pytest.mark.parametrize("V,ld", WIDTHS)
def test_lockstep_form(dev, V, ld, sampled, lp_n, fsm):
    from seedx_amd import ops
    rows, logits, tok, counts = _lock_case(V, ld, fsm)
    G = len(rows)
    fsms = _tables(V) if fsm else None
    params = [d["ctl"] for d in rows]
    prev = [d["prev"] for d in rows]
    final = _final_rows(rows, logits, V, counts, tok, fsms)
    img, nrows = (_identity_img(V, dev) if fsm else _i32(IMG_IDS, dev)), 8
    step = _i32(tok, dev)
    want = [int(r % 5 != 4) for r in range(G)]
    # ---- the oracle: the existing tail on the numpy-edited rows
    ref_l, ref_cur = final.to(dev), _i32(prev, dev)
    ref_out = torch.full((G, nrows), -1, dtype=torch.int32, device=dev)
    if sampled:
        rp = _sample_params(dev, G)
        ops.sample_next_b(ref_l, V, img, ref_cur, ref_out, step, rp, token_index=step, n_kept=rp.n_kept, p_chosen=rp.p_chosen)
    else:
        ops.greedy_next_b(ref_l, V, img, ref_cur, ref_out, step)
    emitted = ref_cur.tolist()
    exp_match = _stops_for(rows, emitted)

    def launch(seq_on):
        dl, cur = logits.to(dev), _i32(prev, dev)
        out = torch.full((G, nrows), -1, dtype=torch.int32, device=dev)
        ctl = Ctl(dev, params, counts, ld)
        sp = _sample_params(dev, G) if sampled else None
        rec = Rec(dev, want, nrows, lp_n) if lp_n is not None else None
        kw = dict(sample=sp, lp=rec, token_index=step, eos_id=EOS, **(dict(n_kept=sp.n_kept, p_chosen=sp.p_chosen) if sampled else {}))
        fs = Fsm(dev, fsms, [d["table"] for d in rows], [d["state"] for d in rows], ld) if fsm else None
        sq = Seq(dev, rows)
        if seq_on:
            ops.next_b_seq(dl, V, img, cur, out, step, ctl, sq, fsm=fs, **kw)
        elif fsm:
            ops.next_b_fsm(dl, V, img, cur, out, step, ctl, fs, **kw)
        else:
            ops.next_b_ctl(dl, V, img, cur, out, step, ctl, **kw)
        torch.cuda.synchronize()
        return dl, cur, out, ctl, sp, rec, fs, sq
    plain = launch(False)
    dl, cur, out, ctl, sp, rec, fs, sq = launch(True)
    assert torch.equal(cur, ref_cur) and torch.equal(out, ref_out)
    if sampled:
        assert torch.equal(sp.n_kept, rp.n_kept) and torch.equal(_bits(sp.p_chosen), _bits(rp.p_chosen))
        assert (sp.n_kept > 1).any()
    tags = {d["tag"]: r for r, d in enumerate(rows) if "tag" in d}
    if not sampled:
        assert emitted[tags["top"]] != rows[tags["top"]]["top"]              # the raw arg-max was banned
    assert final[tags["placeholder_prefix"], 10].item() == NINF and not torch.isinf(final[tags["placeholder_banned"], :V]).any()
    if fsm:
        assert emitted[tags["fsm_a"]] in (10, 11) and emitted[tags["fsm_b"]] == 8
    else:
        assert emitted[tags["chain"]] == 432 and final[tags["chain"], 432].item() == NINF
    hist, hist_len, matched = sq.hist.cpu().numpy(), sq.hist_len.tolist(), sq.matched.tolist()
    seen = set()
    for r, d in enumerate(rows):
        edited = d["ctl"] is not None or (d["on"] and d["n"] > 0) or (d["table"] >= 0 and d["state"] >= 0)
        if d["on"]:
            if d["n"] > 0:
                banned = ngram_banned(d["hist"], d["n"], V)
                assert emitted[r] not in banned or d.get("tag") == "chain", r
                seen.add((d["n"], bool(banned)))
            if edited:
                con = d["table"] >= 0 and d["state"] >= 0
                expect = final[r, :V].numpy().copy() if (fsm or con) else _zeroed(final[r, :V].numpy().copy(), d["prev"])
                assert torch.equal(_bits(ctl.work[r, :V].cpu()), _bits(torch.from_numpy(expect))), r
                assert torch.equal(_bits(ctl.work[r, V:].cpu()), _bits(logits[r, V:])), r       # the padding is a copy, never banned
                assert torch.equal(_bits(dl[r].cpu()), _bits(logits[r])), r                      # the logits row stays raw
            else:
                assert (ctl.work[r] == -123.0).all(), r                      # stops only: no working row
            want_hist = np.full(LD_HIST, SENT, dtype=np.int32)
            want_hist[:d["L"]] = d["hist"]
            want_hist[d["L"]] = emitted[r]
            assert hist_len[r] == d["L"] + 1 and np.array_equal(hist[r], want_hist), r
            assert matched[r] == (-1 if exp_match[r] is None else exp_match[r]), r
        else:                                                                # bit for bit the call without the rules; history untouched
            assert torch.equal(_bits(dl[r]), _bits(plain[0][r])) and torch.equal(_bits(ctl.work[r]), _bits(plain[3].work[r])), r
            assert plain[1][r].item() == emitted[r] and torch.equal(out[r], plain[2][r])
            assert hist_len[r] == d["L"] and matched[r] == -9 and np.array_equal(hist[r], plain[7].hist[r].cpu().numpy()), r
    assert seen == {(n, b) for n in (1, 2, 3, 8) for b in (False, True)}     # every n with and without a ban
    got = [m for m, d in zip(matched, rows) if d["on"]]
    assert {-1, 0, 1} <= set(got)
    exp = counts.copy()
    for r in range(G):
        if params[r] is not None:
            exp[r, emitted[r]] += 1
    assert np.array_equal(ctl.counts[:, :V].cpu().numpy(), exp)
    if fsm:
        want_state = [advance(fsms[d["table"]], d["state"], emitted[r], EOS) if d["table"] >= 0 and d["state"] >= 0 else d["state"]
                      for r, d in enumerate(rows)]
        assert fs.state.tolist() == want_state
    if rec is not None:
        c, ti, tv = ops.token_logprobs(logits.to(dev), V, cur, lp_n)
        for r in range(G):
            got = (rec.chosen[r, tok[r]], rec.top_ids[r, tok[r]], rec.top[r, tok[r]])
            if r % 5 == 4:
                assert (rec.chosen[r] == -7.0).all() and (rec.top_ids[r] == -9).all()
            elif rows[r].get("tag") == "chain":
                assert got[0].isnan() and (got[1] == -1).all() and got[2].isnan().all()
            else:
                assert torch.equal(_bits(got[0]), _bits(c[r])) and torch.equal(got[1], ti[r]) and torch.equal(_bits(got[2]), _bits(tv[r])), r


G2 = 11


@pytest.mark.gpu
@pytest.mark.parametrize("V,ld", WIDTHS)
@pytest.mark.parametrize("sampled,lp_n", [(False, None), (True, None), (False, 2), (True, 8)], ids=["greedy", "sampled", "greedy-lp", "sampled-lp"])
def test_slot_form(dev, V, ld, sampled, lp_n):
    """Eleven slots: a stop of length 1 fires (0), a stop of length 8 fires (1), parked (2), live with on = 0 (3), a stop that straddles
    the prompt does not fire (4), an n-gram ban without stops (5), EOS (6), a force_at replacement that completes a stop (7: the FORCED
    id is appended and matched), budget (8), controls + ban + the second stop fires (9), a 1025-id history (10). A slot whose stop fires
    parks exactly like one whose budget ends on that token: every counter and the status row equal the plain slot tail run on the
    numpy-edited rows with that budget. Parked and on = 0 slots are sx_next_slots_ctl bit for bit, their history untouched."""
    from seedx_amd import ops
    rng = np.random.default_rng(6)
    g = torch.Generator().manual_seed(66)
    logits = torch.randn(G2, ld, generator=g) * 3
    logits[:, V:] = float("nan")
    logits[6, EOS] = 60.0
    alpha = np.array([3, 4, 5, 6, 8])
    logits[:, alpha.tolist()] += 9.0
    logits[6, EOS] = 90.0
    P = ControlParams
    params = [None, None, P(repetition_penalty=1.2), None, None, None, None, None, P(frequency_penalty=0.2),
              P(repetition_penalty=1.6, presence_penalty=0.2, logit_bias={8: -2.0}), None]
    small = lambda L: [int(t) for t in alpha[rng.integers(0, 5, size=L)]]
    rows = [dict(on=1, n=0, hist=small(12)), dict(on=1, n=2, hist=small(40)), dict(on=1, n=2, hist=small(20)), dict(on=0, n=2, hist=small(20)),
            dict(on=1, n=0, hist=small(9)), dict(on=1, n=1, hist=small(30)), dict(on=1, n=3, hist=small(50)), dict(on=1, n=2, hist=small(15)),
            dict(on=1, n=8, hist=small(300)), dict(on=1, n=2, hist=small(64)), dict(on=1, n=3, hist=small(1025))]
    for d in rows:
        d["L"], d["prompt_len"] = len(d["hist"]), len(d["hist"]) // 2
    live = [1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1]
    stepv = [0, 3, 2, 5, 1, 4, 3, 2, 6, 2, 7]
    n_new = [1, 4, 3, 6, 2, 5, 4, 3, 7, 3, 8]
    max_new = [100, 100, 100, 100, 100, 100, 100, 100, 8, 100, 100]          # slot 8 reaches its budget
    force_at = [-1, -1, -1, -1, -1, -1, -1, 3, -1, -1, -1]                   # slot 7: the id is replaced by force_id = 400
    prev = [11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21]
    pos = [20 + r for r in range(G2)]
    counts = np.stack([count_words(V, rng.integers(0, V, size=30), alpha[rng.integers(0, 5, size=int(rng.integers(1, 40)))]) for _ in range(G2)])
    final = _edited(logits, V, counts, params, stepv, EOS)
    for r, d in enumerate(rows):
        if live[r] and d["on"] and d["n"] > 0:
            final[r, :V] = torch.from_numpy(apply_no_repeat(final[r, :V].numpy(), d["hist"], d["n"]))
    img = _i32(IMG_IDS, dev)

    def run(rows_t, budgets, ctl, sq, rec):
        t = dict(cur=_i32(prev, dev), live=_i32(live, dev), n_new=_i32(n_new, dev), force_at=_i32(force_at, dev),
                 pos=_i32(pos, dev), ctx=_i32([p + 1 for p in pos], dev), step=_i32(stepv, dev))
        mx = _i32(budgets, dev)
        out = torch.full((G2, 12), -1, dtype=torch.int32, device=dev)
        status = torch.full((G2, 4), -5, dtype=torch.int32, device=dev)
        sp = _sample_params(dev, G2, seed=9) if sampled else None
        skw = dict(n_kept=sp.n_kept, p_chosen=sp.p_chosen) if sampled else {}
        args = (rows_t, V, img, t["cur"], t["live"], t["n_new"], mx, t["force_at"], t["pos"], t["ctx"], t["step"], out, status)
        if sq is not None:
            ops.next_slots_seq(*args, ctl, sq, sample=sp, lp=rec, force_id=400, eos_id=EOS, **skw)
        elif ctl is not None:
            ops.next_slots_ctl(*args, ctl, sample=sp, lp=rec, force_id=400, eos_id=EOS, **skw)
        elif sampled:
            ops.sample_next_slots(*args, sp, force_id=400, eos_id=EOS, **skw)
        else:
            ops.greedy_next_slots(*args, force_id=400, eos_id=EOS)
        torch.cuda.synchronize()
        t.update(out=out, status=status)
        if sampled:
            t.update(n_kept=sp.n_kept, p_chosen=_bits(sp.p_chosen))
        return t
    first = run(final.to(dev), max_new, None, None, None)                    # the ids the slots emit: stops do not alter them
    e = [s[0] for s in first["status"].tolist()]
    assert e[7] == 400
    h = lambda r, k: rows[r]["hist"][rows[r]["L"] - k:]
    rows[0]["stops"] = [[e[0]]]
    rows[1]["stops"], rows[1]["prompt_len"] = [[1, 2, 3], h(1, 7) + [e[1]]], rows[1]["L"] - 7
    rows[2]["stops"] = [[1]]
    rows[3]["stops"] = [[e[3]]]                                              # on = 0: would fire
    rows[4]["stops"], rows[4]["prompt_len"] = [h(4, 2) + [e[4]]], rows[4]["L"] - 1
    rows[5]["stops"] = []
    rows[6]["stops"] = [[1, 2]]
    rows[7]["stops"], rows[7]["prompt_len"] = [h(7, 1) + [400]], rows[7]["L"] - 1
    rows[8]["stops"] = [[e[8] + 1]]
    rows[9]["stops"] = [[499, e[9]], h(9, 3) + [e[9]], [e[9]]]
    rows[9]["prompt_len"] = 0
    rows[10]["stops"] = [[2, e[10] + 1]]
    exp_match = [stop_match(d["hist"][d["prompt_len"]:] + [e[r]], d["stops"]) if live[r] and d["on"] else None for r, d in enumerate(rows)]
    assert exp_match == [0, 1, None, None, None, None, None, 0, None, 1, None]
    budgets = [n_new[r] + 1 if exp_match[r] is not None else max_new[r] for r in range(G2)]
    ref = run(final.to(dev), budgets, None, None, None)
    ctl_only = Ctl(dev, params, counts, ld)
    dl_ctl = logits.to(dev)
    run(dl_ctl, max_new, ctl_only, None, None)
    dl = logits.to(dev)
    ctl, sq = Ctl(dev, params, counts, ld), Seq(dev, rows)
    rec = Rec(dev, [1] * G2, 12, lp_n) if lp_n is not None else None
    got = run(dl, max_new, ctl, sq, rec)
    for k in ref:
        assert torch.equal(ref[k], got[k]), k
    status = got["status"].tolist()
    for r in (0, 1, 7, 9):                                                   # parked by the stop: the values of a slot that met EOS
        assert status[r][1] == 0 and status[r][3] == n_new[r] + 1
        assert [got[k][r].item() for k in ("live", "step", "pos", "ctx")] == [0, -1, -1, 0]
    assert status[6][0] == EOS and status[6][1] == 0 and status[4][1] == 1 and status[5][1] == 1 and status[10][1] == 1 and status[8][1] == 0
    assert status[2] == [-5] * 4
    hist, hist_len, matched = sq.hist.cpu().numpy(), sq.hist_len.tolist(), sq.matched.tolist()
    for r, d in enumerate(rows):
        want_hist = np.full(LD_HIST, SENT, dtype=np.int32)
        want_hist[:d["L"]] = d["hist"]
        if live[r] and d["on"]:
            want_hist[d["L"]] = e[r]
            assert hist_len[r] == d["L"] + 1 and matched[r] == (-1 if exp_match[r] is None else exp_match[r]), r
            if d["n"] > 0:
                assert e[r] not in ngram_banned(d["hist"], d["n"], V), r
                assert torch.equal(_bits(ctl.work[r, :V].cpu()), _bits(torch.from_numpy(_zeroed(final[r, :V].numpy().copy(), prev[r])))), r
                assert torch.equal(_bits(dl[r].cpu()), _bits(logits[r])), r
            elif params[r] is None:
                assert (ctl.work[r] == -123.0).all(), r
        else:                                                                # parked / on = 0: sx_next_slots_ctl bit for bit
            assert hist_len[r] == d["L"] and matched[r] == -9, r
            assert torch.equal(_bits(dl[r]), _bits(dl_ctl[r])) and torch.equal(_bits(ctl.work[r]), _bits(ctl_only.work[r])), r
        assert np.array_equal(hist[r], want_hist), r
    exp = counts.copy()
    for r in range(G2):
        if live[r] and params[r] is not None:
            exp[r, e[r]] += 1
    assert np.array_equal(ctl.counts[:, :V].cpu().numpy(), exp)
    assert torch.equal(_bits(dl[2].cpu()), _bits(logits[2]))                 # parked: the logits row untouched
    if rec is not None:
        c, ti, tv = ops.token_logprobs(logits.to(dev), V, _i32([x if x >= 0 else 0 for x in e], dev), lp_n)
        for r in range(G2):
            got_r = (rec.chosen[r, stepv[r]], rec.top_ids[r, stepv[r]], rec.top[r, stepv[r]])
            if not live[r]:
                assert (rec.chosen[r] == -7.0).all()
            else:
                assert torch.equal(_bits(got_r[0]), _bits(c[r])) and torch.equal(got_r[1], ti[r]) and torch.equal(_bits(got_r[2]), _bits(tv[r])), r


# ---- model -------------------------------------------------------------------------------------------------------------------------
def _has_repeat(ids, n):
    grams = [tuple(ids[i:i + n]) for i in range(len(ids) - n + 1)]
    return len(grams) != len(set(grams))


def _prompts(G):
    return [[1, 10 + g] + [20 + g + i for i in range(3 + g)] for g in range(G)]


def _slot_run(dev, agent, rules, use_graph, steps=11, host_rule=None):
    """Three slots of the miniature through prefill + ``steps`` slot steps. ``rules``: per-slot SeqParams / None, or None for a slot state
    without a SeqRuleState. ``host_rule`` (per-slot n, with ``rules`` None): the plain eager slot step, whose id the HOST replaces by
    the arg-max of the numpy rule on the step's logits before the next step feeds it. Returns (out_ids, hid)."""
    from seedx_amd import ops
    llm = agent.llm
    llm.reset()
    P = llm._pack()
    G, rows = 3, 16
    img = _i32(IMG_IDS[:1] + IMG_IDS[1:17] + IMG_IDS[-1:], dev)
    imgs = img.tolist()
    st = llm.slot_state(force_id=400, eos_id=-1, **(dict(seq_rules=True) if rules is not None else {}))
    out_ids = torch.full((G, rows), -1, dtype=torch.int32, device=dev)
    hid = torch.zeros((G, rows, llm.H), dtype=torch.float32, device=dev)
    prompts = _prompts(G)
    xs = [ops.embedding(_i32(p, dev), P["embed"]) for p in prompts]
    llm._slot_write(P["pos"], range(G), 0)
    llm._slot_write(P["ctx"], range(G), 1)
    logits, _ = llm.forward_embeds_batch(xs, list(range(G)))
    logits = logits.contiguous()
    first = _i32([p[-1] for p in prompts], dev)
    seen = [list(p) for p in prompts]

    def by_rule(row, g):
        y = row[:llm.V].cpu().numpy().copy()
        if host_rule[g]:
            y = apply_no_repeat(y, seen[g], host_rule[g])
        if seen[g][-1] in imgs[:-1]:
            return imgs[imgs.index(seen[g][-1]) + 1]
        y[imgs[1:]] = 0.0
        return int(np.argmax(y))
    if rules is not None:
        qs = st.seq_rules
        assert qs is not None and st.controls is not None and qs.hist.shape == (G, llm.Tmax)
        qs.set_rows(range(G), rules, prompts)
        zero = torch.zeros(G, dtype=torch.int32, device=dev)
        ops.next_b_seq(logits, llm.V, img, first, None, zero, st.controls.gather(range(G)), qs.gather(range(G)), token_index=zero)
        own = [g for g in range(G) if rules[g] is not None]
        qs.append([(g, len(prompts[g])) for g in own], [[first[g].item()] for g in own])
    elif host_rule is not None:
        first = _i32([by_rule(logits[g], g) for g in range(G)], dev)
    else:
        assert st.seq_rules is None
        ops.greedy_next_b(logits, llm.V, img, first, None, None)
    for g in range(G):
        seen[g].append(first[g].item())
    P["cur"].copy_(first)
    out_ids[:, 0] = first
    P["step"].fill_(1)
    st.n_new.fill_(1)
    st.max_new.fill_(100)
    st.live.fill_(1)
    for k in range(steps):
        llm.decode_step(img, out_ids, hid, use_graph=use_graph, slots=st)
        if host_rule is not None:                        # the step's own logits, before its in-place zeroing mattered: same columns
            ids = [by_rule(st.logits[g], g) for g in range(G)]
            P["cur"].copy_(_i32(ids, dev))
            out_ids[:, k + 1] = _i32(ids, dev)
            for g in range(G):
                seen[g].append(ids[g])
    torch.cuda.synchronize()
    res = out_ids.clone(), hid.clone(), (st.seq_rules.hist.clone(), st.seq_rules.hist_len.tolist()) if rules is not None else None
    llm.reset()
    return res


@pytest.mark.gpu
def test_model_eager_equals_graph_equals_host_rule(dev):
    agent = _agent(dev, torch.float16, 3)
    llm = agent.llm
    ns = [1, 0, 2]
    rules = [SeqParams(no_repeat_ngram_size=1), None, SeqParams(no_repeat_ngram_size=2)]
    plain = _slot_run(dev, agent, None, True)
    assert llm._slot_graph is not None and llm._slot_graph_seq is None
    eager = _slot_run(dev, agent, rules, False)
    assert llm._slot_graph_seq is None
    graph = _slot_run(dev, agent, rules, True)
    assert llm._slot_graph_seq is not None and llm._slot_graph_ctl is None
    assert torch.equal(eager[0], graph[0]) and torch.equal(eager[1], graph[1])
    assert torch.equal(eager[2][0], graph[2][0]) and eager[2][1] == graph[2][1]
    host = _slot_run(dev, agent, None, False, host_rule=ns)
    ids = graph[0]
    assert torch.equal(ids, host[0]) and torch.equal(graph[1], host[1])
    assert (ids[:, :12] >= 0).all() and (ids[:, 12:] == -1).all()
    prompts = _prompts(3)
    hist, hist_len = graph[2]
    for g in (0, 2):
        full = prompts[g] + ids[g, :12].tolist()
        assert not _has_repeat(full, ns[g]), g
        assert hist_len[g] == len(full) and hist[g, :len(full)].tolist() == full       # the device's history is prompt + emitted ids
    assert hist_len[1] == 0
    assert torch.equal(ids[1], plain[0][1]) and torch.equal(graph[1][1], plain[1][1])    # the slot without rules: a model without a state
    assert _has_repeat(prompts[0] + plain[0][0, :12].tolist(), 1) and not torch.equal(ids[0], plain[0][0])    # the ban did something


# ---- engines -----------------------------------------------------------------------------------------------------------------------
def _cut(ids, stop):
    for k in range(1, len(ids) + 1):
        if stop_match(ids[:k], [stop]) is not None:
            return ids[:k]
    return ids


@pytest.mark.gpu
def test_engines_stop(dev):
    """Stops do not alter logits: a stopped request's ids are the unstopped run's ids cut after the first match, in the three engines,
    for stops of length 1, 2 and 8 taken from the unstopped run's own output; in flight the freed slot is refilled earlier."""
    tok, n = StubTokenizer(), 16
    a3 = _agent(dev, torch.float16, 3)
    a1 = _agent(dev, torch.float16, 1)
    others = [_req(1, n), _req(2, n)]
    run3 = lambda req: a3.generate_batch(tok, [req] + others, max_new_tokens=n, **KW)
    base3 = run3(dict(input_ids=[PROMPT]))
    b = base3[0]["generate_ids"].tolist()
    assert len(b) == n and "seq_rules" not in base3[0] and a3.llm._graph is not None and a3.llm._graph_seq is None
    assert getattr(a3.llm, "_seq_rule_state", None) is None                 # nobody asked: no state was built
    queue = [dict(input_ids=[PROMPT], max_new_tokens=n), _req(1, 9), _req(2, 7), _req(3, 10), _req(4, 6), _req(5, 8)]
    quiet = a3.generate_inflight(tok, queue, **KW)
    quiet_steps = a3.last_inflight_stats["decode_steps"]
    assert quiet[0]["generate_ids"].tolist() == b and not any(k.endswith("_seq") for k in a3._inflight)
    assert a3.llm._slot_graph is not None and a3.llm._slot_graph_seq is None
    for stop in ([b[4]], b[5:7], b[3:11]):
        want = _cut(b, stop)
        assert len(want) < n and want[-len(stop):] == stop
        batch = run3(dict(input_ids=[PROMPT], stop=[[499, 498], stop]))
        assert batch[0]["generate_ids"].tolist() == want
        assert batch[0]["seq_rules"] == {"stop": [[499, 498], stop], "no_repeat_ngram_size": 0, "matched": 1}
        for r in (1, 2):                                                     # the neighbours: as without the key
            assert torch.equal(batch[r]["generate_ids"], base3[r]["generate_ids"]) and "seq_rules" not in batch[r]
        single = a1.generate(tok, input_ids=[PROMPT], max_new_tokens=n, stop=stop, **KW)
        assert single["generate_ids"].tolist() == want and single["seq_rules"]["matched"] == 0
        busy_q = [dict(q) for q in queue]
        busy_q[0]["stop"] = [stop]
        busy = a3.generate_inflight(tok, busy_q, **KW)
        assert busy[0]["generate_ids"].tolist() == want and busy[0]["seq_rules"]["matched"] == 0
        assert a3.last_inflight_stats["decode_steps"] < quiet_steps         # the slot was freed and refilled earlier
        for r in range(1, len(queue)):
            assert torch.equal(busy[r]["generate_ids"], quiet[r]["generate_ids"]) and "seq_rules" not in busy[r]
    assert a3.llm._graph_seq is not None and a3.llm._slot_graph_seq is not None
    straddle = PROMPT[-1:] + b[:1]                                            # completed by the prompt's tail on the first token: no match
    miss = run3(dict(input_ids=[PROMPT], stop=[straddle]))[0]["generate_ids"].tolist()
    assert miss == _cut(b, straddle) and len(miss) > 1
    assert "seq_rules" not in a1.generate(tok, input_ids=[PROMPT], max_new_tokens=n, **KW)


@pytest.mark.gpu
def test_engines_no_repeat(dev):
    """The ban fires: the run WITHOUT the rule repeats an n-gram (asserted: prompts and n are chosen for it), the run with it differs and
    repeats none, and the three engines give the same ids, greedy and sampled, beside requests without rules, with controls, log-probabilities
    and a grammar-free queue."""
    tok, n = StubTokenizer(), 24
    a3 = _agent(dev, torch.float16, 3)
    a1 = _agent(dev, torch.float16, 1)
    others = [_req(1, n), _req(2, n)]
    for extra, ng in ((dict(), 3), (dict(do_sample=True, temperature=1.0, top_k=3, top_p=1.0, seed=7), 1),
                      (dict(repetition_penalty=1.05, logprobs=2), 2)):
        req = dict(input_ids=[PROMPT], **extra)
        base = a3.generate_batch(tok, [req] + others, max_new_tokens=n, **KW)
        b = base[0]["generate_ids"].tolist()
        assert _has_repeat(PROMPT + b, ng), (extra, b)                        # the precondition: without the rule an n-gram repeats
        ruled = a3.generate_batch(tok, [dict(req, no_repeat_ngram_size=ng)] + others, max_new_tokens=n, **KW)
        w = ruled[0]["generate_ids"].tolist()
        assert w != b and not _has_repeat(PROMPT + w, ng) and ruled[0]["seq_rules"]["no_repeat_ngram_size"] == ng
        assert ruled[0]["seq_rules"]["matched"] is None
        for r in (1, 2):
            assert torch.equal(ruled[r]["generate_ids"], base[r]["generate_ids"])
        single = a1.generate(tok, input_ids=[PROMPT], max_new_tokens=n, no_repeat_ngram_size=ng, **extra, **KW)
        assert single["generate_ids"].tolist() == w
        queue = [_req(0, 9), dict(req, no_repeat_ngram_size=ng, max_new_tokens=n), _req(2, 7), dict(_req(3, 10), no_repeat_ngram_size=2), _req(4, 6)]
        busy = a3.generate_inflight(tok, queue, **KW)
        assert busy[1]["generate_ids"].tolist() == w
        r3 = busy[3]["generate_ids"].tolist()
        assert not _has_repeat(queue[3]["input_ids"][0] + r3, 2)
        if "logprobs" in extra:                                              # the records describe the RAW rows: the ids' own raw log-probs
            lp = ruled[0]["logprobs"]
            assert lp["token_ids"].tolist() == w and busy[1]["logprobs"]["token_ids"].tolist() == w


@pytest.mark.gpu
def test_refusals_on_the_device_side(dev):
    """decode_step refuses a second sequence-rule state beside a slot state's; the entry points refuse null pointers and ld_hist < 1
    (SX_CHECK → RuntimeError); ops refuses the per-row values the device would clamp (ValueError)."""
    from seedx_amd import ops
    agent = _agent(dev, torch.float16, 3)
    llm = agent.llm
    st = llm.slot_state(force_id=400, seq_rules=True)
    with pytest.raises(ValueError, match="a slot state carries its own sequence-rule state"):
        llm.decode_step(None, None, None, slots=st, seq_rules=llm.seq_rule_state())
    llm.reset()
    V, ld = 500, 512
    rows = [dict(on=1, n=2, hist=[3, 4, 3], prompt_len=1, stops=[[4]]), dict(on=1, n=0, hist=[5], prompt_len=1, stops=[])]
    img = _i32(IMG_IDS, dev)

    def call(sq, slots=False):
        logits = torch.zeros((2, ld), device=dev)
        ctl = Ctl(dev, [None, None], np.zeros((2, V), np.int32), ld)
        z = lambda v=0: _i32([v, v], dev)
        if slots:
            ops.next_slots_seq(logits, V, img, z(1), z(1), z(1), z(9), z(-1), z(4), z(5), z(1), None, torch.zeros((2, 4), dtype=torch.int32, device=dev),
                               ctl, sq)
        else:
            ops.next_b_seq(logits, V, img, z(1), None, z(), ctl, sq)
        torch.cuda.synchronize()
    # a pointer, but no room: the struct as ops builds it, with ld_hist = 0
    import ctypes as C
    from seedx_amd import _lib
    logits, cur, step = torch.zeros((2, ld), device=dev), _i32([1, 1], dev), _i32([0, 0], dev)
    ctl = Ctl(dev, [None, None], np.zeros((2, V), np.int32), ld)
    ca, qa = ops._ctl_args(ctl, logits, V, step, -1), ops._seq_args("test", Seq(dev, rows), 2)
    qa.ld_hist = 0
    p = lambda t: t.data_ptr()
    rc = _lib.load().sx_next_b_seq(p(logits), ld, V, p(img), img.numel(), p(cur), p(cur), None, 0, p(step), 2, None, None, C.byref(ca), None,
                                   C.byref(qa), None)
    with pytest.raises(RuntimeError, match=r"sx_next_b_seq: sx_seq_rule_args.ld_hist=0 \(>= 1\)"):
        _lib.check(rc, "sx_next_b_seq")
    for slots in (False, True):
        call(Seq(dev, rows), slots)                                           # the well-formed call passes
        sq = Seq(dev, rows)
        sq.hist = torch.empty((2, 0), dtype=torch.int32, device=dev)
        with pytest.raises(RuntimeError, match="null pointer in sx_seq_rule_args|ld_hist=0"):
            call(sq, slots)
        for field, value, msg in (("ngram", [9, 0], r"ngram\[0\]=9 lies outside 0 .. 8"), ("ngram", [2, -1], r"ngram\[1\]=-1"),
                                  ("n_stop", [5, 0], r"n_stop\[0\]=5 lies outside 0 .. 4"), ("n_stop", [1, -2], r"n_stop\[1\]=-2"),
                                  ("stop_len", [[0, 0, 0, 0], [0] * 4], r"stop_len\[0\]\[0\]=0 lies outside 1 .. 8"),
                                  ("stop_len", [[9, 0, 0, 0], [0] * 4], r"stop_len\[0\]\[0\]=9")):
            sq = Seq(dev, rows)
            setattr(sq, field, _i32(value, dev))
            with pytest.raises(ValueError, match=msg):
                call(sq, slots)


@pytest.mark.gpu
def test_engines_with_a_grammar_on_the_same_request(dev):
    """A request that carries a grammar AND rules: every id is one the automaton admits, no id of prompt + output occurs twice (n = 1), the
    stop taken from that run's own output cuts it, and the lock-step and the in-flight engine agree."""
    from tests.test_grammar_gpu import _grammars, _loaded_agent
    tok, n = StubTokenizer(), 14
    vocab, gr = _grammars()
    a3 = _loaded_agent(dev, 3, {"word": gr["word"]})
    others = [_req(1, n), _req(2, n)]
    req = dict(input_ids=[PROMPT], grammar="word", no_repeat_ngram_size=1)
    free = a3.generate_batch(tok, [dict(input_ids=[PROMPT], grammar="word")] + others, max_new_tokens=n, **KW)
    assert a3.llm._graph_fsm is not None and a3.llm._graph_fsm_seq is None
    ruled = a3.generate_batch(tok, [req] + others, max_new_tokens=n, **KW)
    assert a3.llm._graph_fsm_seq is not None
    w = ruled[0]["generate_ids"].tolist()
    assert len(w) == n and gr["word"].walk(w)[1] == n and not _has_repeat(PROMPT + w, 1)
    assert ruled[0]["grammar"]["name"] == "word" and ruled[0]["seq_rules"]["no_repeat_ngram_size"] == 1
    for r in (1, 2):
        assert torch.equal(ruled[r]["generate_ids"], free[r]["generate_ids"])
    cut = a3.generate_batch(tok, [dict(req, stop=[w[4:6]])] + others, max_new_tokens=n, **KW)[0]
    assert cut["generate_ids"].tolist() == w[:6] and cut["seq_rules"]["matched"] == 0
    queue = [_req(0, 9), dict(req, max_new_tokens=n, stop=[w[4:6]]), _req(2, 7), dict(req, max_new_tokens=n)]
    busy = a3.generate_inflight(tok, queue, **KW)
    assert busy[1]["generate_ids"].tolist() == w[:6] and busy[3]["generate_ids"].tolist() == w
    assert a3.llm._slot_graph_fsm_seq is not None
