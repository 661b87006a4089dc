"""In-flight batching, host side: the slot scheduler on hand-worked cases and the C-ABI of the slot-step kernel (no GPU)."""
import ctypes
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_bounds(lengths, G, stats):
    from seedx_amd.inflight import lockstep_wave_steps
    assert stats["live_slot_steps"] == sum(n - 1 for n in lengths)
    assert stats["decode_steps"] >= math.ceil(stats["live_slot_steps"] / G)
    assert stats["decode_steps"] <= lockstep_wave_steps(lengths, G)
    assert stats["live_slot_steps"] + stats["parked_slot_steps"] == G * stats["decode_steps"]
    assert stats["admissions"] == len(lengths) and sorted(stats["finish_order"]) == list(range(len(lengths)))


def test_mixed_queue_on_four_slots():
    """Budgets [24, 6, 6, 6] x 3 on 4 slots. By hand: r0 decodes in steps 1-23; r1-r3 in 1-5; r4 (24) takes slot 1 for steps 6-28, r5 / r6
    slots 2 / 3 for 6-10; r7 (6) slot 2 for 11-15 and r8 (24) slot 3 for 11-33; r9 slot 2 for 16-20; r10 slot 2 for 21-25; r11 takes
    r0's slot 0 for 24-28. The last step is r8's 33rd; same-step finishes are reported lowest slot first (r11 in slot 0 before r4)."""
    from seedx_amd.inflight import lockstep_wave_steps, simulate
    lengths = [24, 6, 6, 6] * 3
    s = simulate(lengths, 4)
    assert s["decode_steps"] == 33 and s["live_slot_steps"] == 114 and s["parked_slot_steps"] == 4 * 33 - 114
    assert s["finish_order"] == [1, 2, 3, 5, 6, 7, 9, 0, 10, 11, 4, 8]
    assert s["prefill_passes"] == 6              # {r0-r3}, {r4-r6}, {r7, r8}, {r9}, {r10}, {r11}
    assert lockstep_wave_steps(lengths, 4) == 3 * 23 == 69
    assert math.ceil(114 / 4) == 29 <= s["decode_steps"] < 69
    _check_bounds(lengths, 4, s)


def test_request_that_finishes_at_admission_frees_its_slot_in_the_same_pass():
    """Budgets [5, 1, 3] on 2 slots: r1 ends with its prefill token, r2 takes its slot before the first step; r0 needs 4 steps, r2 two."""
    from seedx_amd.inflight import simulate
    s = simulate([5, 1, 3], 2)
    assert s["decode_steps"] == 4 and s["live_slot_steps"] == 6 and s["prefill_passes"] == 2
    assert s["finish_order"] == [1, 2, 0]
    _check_bounds([5, 1, 3], 2, s)


def test_max_admit_one():
    """max_admit = 1: one request per pass. [5, 1, 3] on 2 slots: r0 alone in step 1; r1 admitted and finished in pass 2 (the pass's
    quota is spent, its slot stays free for step 2); r2 decodes in steps 3-4 next to r0's last two. Still 4 steps, 3 prefills."""
    from seedx_amd.inflight import simulate
    s = simulate([5, 1, 3], 2, max_admit=1)
    assert s["decode_steps"] == 4 and s["live_slot_steps"] == 6 and s["prefill_passes"] == 3
    assert s["finish_order"] == [1, 0, 2]
    _check_bounds([5, 1, 3], 2, s)
    # the mixed queue ramps up one slot per step: r1 / r2 / r3 start 1 / 2 / 3 steps late (r3 ends at step 8), from then on every
    # admission waits for a finish exactly as without the limit but three steps later: r8 ends at 36
    lengths = [24, 6, 6, 6] * 3
    s = simulate(lengths, 4, max_admit=1)
    assert s["decode_steps"] == 36 and s["live_slot_steps"] == 114 and s["prefill_passes"] == 12
    _check_bounds(lengths, 4, s)


@pytest.mark.parametrize("lengths,G,max_admit", [([1], 4, None), ([7], 1, None), ([3, 3, 3], 4, None), ([2, 9, 4, 4, 1, 1, 30], 3, 2),
                                                 (list(range(1, 40)), 16, None), ([128] * 16, 16, None), ([5] * 33, 32, 4)])
def test_step_count_bounds(lengths, G, max_admit):
    from seedx_amd.inflight import simulate
    s = simulate(lengths, G, max_admit)
    if max_admit is None:
        _check_bounds(lengths, G, s)
    else:      # a limited pass may leave slots free that lock-step waves would fill: only the lower bound holds
        assert s["decode_steps"] >= math.ceil(s["live_slot_steps"] / G) and s["admissions"] == len(lengths)
    if len(set(lengths)) == 1 and len(lengths) <= G and max_admit is None:
        assert s["decode_steps"] == lengths[0] - 1 and s["parked_slot_steps"] == (G - len(lengths)) * s["decode_steps"]


def test_scheduler_events():
    from seedx_amd.inflight import SlotScheduler
    sch = SlotScheduler(3, 5)
    assert sch.admit() == [(0, 0), (1, 1), (2, 2)] and sch.admit() == [] and sch.live_slots() == [0, 1, 2]
    assert sch.finish(1) == 1 and sch.live_slots() == [0, 2]
    with pytest.raises(AssertionError):
        sch.finish(1)
    sch.new_pass()
    assert sch.admit() == [(1, 3)]
    assert sch.finish(0) == 0 and sch.finish(2) == 2
    sch.new_pass()
    assert sch.admit() == [(0, 4)] and not sch.done
    assert sch.finish(0) == 4 and sch.finish(1) == 3 and sch.done


def test_slot_step_abi_in_sync():
    """sx_slot_step_args: header field order == ctypes struct; sx_greedy_next_slots declared, bound and exported."""
    from seedx_amd import _lib
    src = open(os.path.join(ROOT, "include", "seedx_hip.h")).read()
    body = re.search(r"typedef struct sx_slot_step_args \{(.*?)\} sx_slot_step_args;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            decl = re.sub(r"^(const\s+)?(void|float|int32_t)\s*\*?", "", decl)
            names += [n.strip().lstrip("*") for n in decl.split(",")]
    assert names == [f[0] for f in _lib.SlotStepArgs._fields_]
    assert ctypes.sizeof(_lib.SlotStepArgs) == 12 * 8 + 8 * 4
    assert "sx_greedy_next_slots" in _lib.SIGNATURES
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "sx_greedy_next_slots")


def test_entry_points_exist():
    import inspect

    from seedx_amd.llama import LlamaForCausalLM, SlotState
    from seedx_amd.seed_x import ContinuousLVLM
    sig = inspect.signature(ContinuousLVLM.generate_inflight)
    assert list(sig.parameters)[1:] == ["tokenizer", "requests", "num_img_gen_tokens", "max_new_tokens", "eos_token_id", "max_admit",
                                        "on_result"]
    assert inspect.signature(LlamaForCausalLM.decode_step).parameters["slots"].default is None
    assert inspect.signature(LlamaForCausalLM._decode_step_body).parameters["slots"].default is None
    assert SlotState.IDLE == {"pos": -1, "ctx": 0, "step": -1}
