"""Prefix reuse of in-flight batching, host side: what a slot's cache holds (PrefixIndex), who may take it (plan_admission, one
hand-built case per rule on 4 slots), the step and token counts (simulate_prefix) and the sx_kv_fork argument struct."""
import os
import re

from seedx_amd.inflight import PrefixIndex, plan_admission, simulate, simulate_prefix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = [1, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60]          # a 12-id prompt; signatures default to the ids


def _index(records, n_slots=4):
    """records: {slot: ids | (ids, sigs)} recorded in ascending slot order under epoch 0."""
    ix = PrefixIndex(n_slots)
    for g in sorted(records):
        rec = records[g]
        ids, sigs = rec if isinstance(rec, tuple) else (rec, rec)
        ix.record(g, ids, sigs, 0)
    return ix


def _reqs(*prompts):
    return [(r, p, p) for r, p in enumerate(prompts)]


def _no_donor_is_overwritten(plan):
    """No donor slot is assigned to a request whose start is smaller than the length forked from that donor."""
    start_of = {g: start for g, _, start, _ in plan}
    for _, _, start, donor in plan:
        if donor is not None and donor in start_of:
            assert start_of[donor] >= start, plan


def test_match_longest_prefix_on_ids_and_signatures():
    ix = _index({0: A, 1: A[:5] + [90, 91], 2: [2, 3, 4]})
    assert ix.match(A[:8] + [70, 71], A[:8] + [70, 71], 0) == [(0, 8), (1, 5)]
    # same ids, another image: rows 3.. carry other signatures, the prefix ends at the first of them
    sig_a = A[:3] + [1000 + i for i in range(9)]
    sig_b = A[:3] + [2000 + i for i in range(9)]
    ix = _index({0: (A, sig_a)})
    assert ix.match(A + [7], sig_a + [7], 0) == [(0, 12)]
    assert ix.match(A + [7], sig_b + [7], 0) == [(0, 3)]
    assert ix.match([9] + A, [9] + A, 0) == []


def test_match_is_capped_below_the_prompt_length():
    ix = _index({0: A + [61, 62]})
    assert ix.match(A, A, 0) == [(0, len(A) - 1)]                  # one token must be forwarded
    assert ix.match(A[:1], A[:1], 0) == []


def test_stale_epoch_never_matches():
    ix = PrefixIndex(4)
    ix.record(0, A, A, 3)
    assert ix.match(A, A, 3) == [(0, 11)] and ix.match(A, A, 4) == []
    ix.restamp(3, 5)                                               # the owner moved the epoch itself: the record moves with it
    assert ix.match(A, A, 5) == [(0, 11)] and ix.match(A, A, 3) == []
    ix.restamp(4, 6)                                               # someone else's epoch: nothing moves
    assert ix.match(A, A, 6) == []
    ix.invalidate(0)
    assert ix.match(A, A, 5) == []


def test_plan_in_place_first():
    ix = _index({0: [2, 3, 4, 5, 6, 7], 2: A})
    plan, deferred = plan_admission(ix, [0, 1, 2, 3], [], _reqs(A[:9] + [80]), min_tokens=4)
    assert plan == [(2, 0, 9, None)] and deferred == []
    # in place takes any length: no copy is paid for it
    plan, _ = plan_admission(_index({2: A}), [0, 1, 2, 3], [], _reqs(A[:2] + [80, 81, 82, 83]), min_tokens=4)
    assert plan == [(2, 0, 2, None)]


def test_plan_short_in_place_ties_take_the_least_recently_used_slot():
    """Every prompt starts with the BOS id: a one-row match with every recorded slot must not cost the youngest record."""
    ix = PrefixIndex(4)
    for g in (2, 0, 3, 1):                                         # last use: slot 2 oldest, then 0, 3, 1
        ix.record(g, [1, 100 + g, 101, 102, 103, 104], [1, 100 + g, 101, 102, 103, 104], 0)
    plan, _ = plan_admission(ix, [0, 1, 2, 3], [], _reqs([1, 5, 6, 7, 8, 9], [1, 15, 16, 17, 18, 19]), min_tokens=4)
    assert plan == [(2, 0, 1, None), (0, 1, 1, None)]
    # a long match is not a tie to break: the slot that holds it wins whatever its stamp
    plan, _ = plan_admission(ix, [0, 1, 2, 3], [], _reqs([1, 101, 101, 102, 103, 77]), min_tokens=4)
    assert plan == [(1, 0, 5, None)]


def test_plan_two_claimants_of_one_free_slot():
    ix = _index({1: A})
    plan, deferred = plan_admission(ix, [0, 1, 2, 3], [], _reqs(A[:8] + [80, 81], A[:8] + [90]), min_tokens=4)
    # request 1 shares 8 rows with request 0 and 8 with slot 1: not MORE than with a slot, so it is not deferred; it forks the 8 rows
    # request 0 keeps in slot 1
    assert plan == [(1, 0, 8, None), (0, 1, 8, 1)] and deferred == []
    _no_donor_is_overwritten(plan)


def test_plan_fork_from_a_live_slot():
    ix = _index({0: A, 1: [2, 3, 4, 5, 6, 7]})
    plan, deferred = plan_admission(ix, [1, 2, 3], [0], _reqs(A[:10] + [80, 81]), min_tokens=4)
    assert plan == [(2, 0, 10, 0)] and deferred == []              # victim: slot 2 was never used, slot 1 holds a record


def test_plan_below_min_tokens():
    ix = _index({0: A})
    plan, _ = plan_admission(ix, [1, 2, 3], [0], _reqs(A[:3] + [80, 81, 82, 83]), min_tokens=4)
    assert plan == [(1, 0, 0, None)]
    stamps = list(ix.stamp)
    plan, _ = plan_admission(ix, [1, 2, 3], [0], _reqs(A[:4] + [80, 81, 82, 83]), min_tokens=4)
    assert plan == [(1, 0, 4, 0)] and ix.stamp == stamps           # the planner only reads the index


def test_plan_never_forks_rows_the_round_overwrites():
    """Slot 1 holds A. Request 0 keeps 6 of its rows in place and rewrites the rest; request 1 matches 10 rows of slot 1."""
    for min_tokens in (4, 6, 7, 10):
        ix = _index({1: A})
        plan, deferred = plan_admission(ix, [0, 1, 2, 3], [], _reqs(A[:6] + [80, 81, 82], A[:10] + [90]), min_tokens=min_tokens)
        _no_donor_is_overwritten(plan)
        assert deferred == [] and plan[0] == (1, 0, 6, None)
        assert plan[1] == ((0, 1, 6, 1) if min_tokens <= 6 else (0, 1, 0, None)), (min_tokens, plan)
    # every free slot but one is a donor-to-be: the victim is the one that is not
    ix = _index({0: A, 1: [2, 3, 4, 5, 6, 7, 8, 9]})
    plan, _ = plan_admission(ix, [0, 1, 2], [3], _reqs(A[:8] + [80], [2, 3, 4, 5, 6, 7] + [81], A[:8] + [82]), min_tokens=4)
    _no_donor_is_overwritten(plan)
    assert plan == [(0, 0, 8, None), (1, 1, 6, None), (2, 2, 8, 0)]


def test_plan_same_round_leader_and_follower():
    ix = PrefixIndex(4)
    same = A[:10]
    plan, deferred = plan_admission(ix, [0, 1, 2, 3], [], _reqs(same, same, [7, 8, 9, 10, 11, 12], same), min_tokens=4)
    assert plan == [(0, 0, 0, None), (1, 2, 0, None)] and deferred == [1, 3]
    ix.record(0, same, same, 0)                                    # the round ran: slot 0 and 1 are live and recorded
    ix.record(1, [7, 8, 9, 10, 11, 12], [7, 8, 9, 10, 11, 12], 0)
    plan, deferred = plan_admission(ix, [2, 3], [0, 1], [(1, same, same), (3, same, same)], min_tokens=4)
    assert plan == [(2, 1, 9, 0), (3, 3, 9, 0)] and deferred == []
    # a short shared head (below min_tokens) defers nobody
    plan, deferred = plan_admission(PrefixIndex(4), [0, 1, 2, 3], [], _reqs(A[:3] + [80, 81], A[:3] + [90, 91]), min_tokens=4)
    assert deferred == [] and plan == [(0, 0, 0, None), (1, 1, 0, None)]


def test_plan_victim_is_least_recently_used():
    ix = PrefixIndex(4)
    for g in (2, 0, 3, 1):                                         # last use: slot 2 oldest, then 0, 3, 1
        ix.record(g, [100 + g] * 6, [100 + g] * 6, 0)
    plan, _ = plan_admission(ix, [0, 1, 2, 3], [], _reqs([5, 6, 7, 8, 9, 10], [15, 16, 17, 18, 19, 20]), min_tokens=4)
    assert [g for g, _, _, _ in plan] == [2, 0] and all(s == 0 and d is None for _, _, s, d in plan)
    plan, _ = plan_admission(PrefixIndex(4), [1, 2, 3], [0], _reqs([5, 6, 7, 8, 9, 10], [15, 16, 17, 18, 19, 20]), min_tokens=4)
    assert [g for g, _, _, _ in plan] == [1, 2]                    # never used: lowest index first


def _shared_queue():
    prompts = []
    for k in range(3):
        prefix = [1] + [100 * (k + 1) + i for i in range(19)]      # 20 ids
        for q in range(4):
            prompts.append(prefix + [900 + 10 * q + i for i in range(3)])
    return prompts


def test_simulate_prefix_on_shared_prefix_prompts():
    prompts = _shared_queue()
    lengths = [5, 9, 3, 7, 2, 6, 6, 4, 8, 1, 5, 3]
    for max_admit in (None, 1, 2):
        got, want = simulate_prefix(prompts, lengths, 4, max_admit=max_admit), simulate(lengths, 4, max_admit=max_admit)
        for k in ("decode_steps", "live_slot_steps", "admissions"):
            assert got[k] == want[k], (max_admit, k, got, want)
        assert got["prefill_tokens"] + got["prefix_hit_tokens"] == sum(len(p) for p in prompts) == 12 * 23
        assert got["prefix_hit_tokens"] > 0 and got["forked_tokens"] <= got["prefix_hit_tokens"]
        assert sorted(got["finish_order"]) == list(range(12))
    got = simulate_prefix(prompts, lengths, 4)
    # round 1 admits the leader of the first group and defers its three followers; they fork 20 rows each in round 2
    assert got["fork_launches"] >= 1 and got["forked_tokens"] >= 60
    assert got["prefill_passes"] > simulate(lengths, 4)["prefill_passes"]
    # a finished slot holds what it generated: the second turn of request 0 finds prompt + answer but the last id
    ix = PrefixIndex(4)
    simulate_prefix(prompts[:1], [4], 4, generated=[[7, 8, 9, 10]], index=ix)
    turn2 = prompts[0] + [7, 8, 9, 10, 11]
    assert ix.match(turn2, turn2, 0)[0] == (0, 23 + 3)
    again = simulate_prefix([turn2], [2], 4, index=ix)
    assert again["prefill_tokens"] == 2 and again["prefix_hit_tokens"] == 26 and again["forked_tokens"] == 0


def test_simulate_prefix_equals_simulate_on_unshared_prompts():
    lengths = [6, 3, 11, 1, 8, 2, 2, 9, 4, 1, 7, 5, 10]
    prompts = [[1000 * (r + 1) + i for i in range(5 + r % 4)] for r in range(len(lengths))]
    got, want = simulate_prefix(prompts, lengths, 4), simulate(lengths, 4)
    for k, v in want.items():
        assert got[k] == v, (k, got, want)
    assert got["prefix_hit_tokens"] == 0 and got["forked_tokens"] == 0 and got["fork_launches"] == 0
    assert got["prefill_tokens"] == sum(len(p) for p in prompts)


def test_kv_fork_struct_layout_matches_header():
    """Field order / count of sx_kv_fork_args mirror the header (the parsing of test_ctypes_struct_layout_matches_header)."""
    from seedx_amd import _lib
    src = open(os.path.join(ROOT, "include", "seedx_hip.h")).read()
    cname = "sx_kv_fork_args"
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        decl = re.sub(r"^(const\s+)?(void|float|double|int32_t|int64_t|uint32_t|uint64_t)\s*\*?", "", decl)
        names += [n.strip().lstrip("*") for n in decl.split(",")]
    assert names == [f[0] for f in _lib.KvForkArgs._fields_], names
    assert "sx_kv_fork" in _lib.SIGNATURES
