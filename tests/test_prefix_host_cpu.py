"""Host-memory tier of the prefix cache, host side: HostPrefixStore on stand-in buffers, plan_host_tier through
inflight.simulate_prefix on a hand-computed queue, the engine's refusals before the LLM is touched, and the C-ABI of sx_kv_rows_copy."""
import ctypes
import os
import re

import pytest

from seedx_amd.inflight import PrefixIndex, simulate_prefix, tag_signatures
from seedx_amd.kvstore import HostPrefixStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_KEYS = ("host_spills", "host_spill_tokens", "host_restores", "host_restore_tokens", "host_evictions", "host_bytes_peak")


def _rec(first, n):
    ids = [1] + [first + i for i in range(n - 1)]
    return ids, list(ids)


def test_kvstore_imports_no_gpu_code():
    """The module's only import at module level is inflight.py (host logic, no torch): torch and the kernels come in when a KVMover is
    built."""
    src = open(os.path.join(ROOT, "seed-x_amd", "kvstore.py")).read()
    assert re.findall(r"^(?:import|from)\s+\S+.*$", src, flags=re.M) == ["from .inflight import _common_prefix"]
    assert not re.findall(r"^(?:import|from)\s+(?!collections)\S+", open(os.path.join(ROOT, "seed-x_amd", "inflight.py")).read(), flags=re.M)


def test_match_lengths_cap_and_adapter_tags():
    st = HostPrefixStore(10 ** 6, 4, row_bytes=10)
    ids, sigs = _rec(100, 12)
    e = st.put(ids, sigs)
    assert st.match(ids + [7, 8], sigs + [7, 8]) == (e, 12)                 # the whole entry, two ids to forward
    assert st.match(ids, sigs) == (e, 11)                                   # the same prompt: capped at len - 1
    assert st.match(ids[:5], sigs[:5]) == (e, 4)
    assert st.match(ids[:6] + [999, 5], sigs[:6] + [999, 5]) == (e, 6)
    assert st.match([2, 3, 4], [2, 3, 4]) is None and st.match([1], [1]) is None
    # same ids, another image: the signatures end the match at the first such row
    other = sigs[:3] + ["other image"] * 9
    assert st.match(ids + [7], other + [7]) == (e, 3)
    # rows computed under an adapter never match untagged ones, and the other way round
    assert st.match(ids + [7], tag_signatures(sigs + [7], "lora-a")) is None
    t = st.put(ids, tag_signatures(sigs, "lora-a"))
    assert st.match(ids + [7], tag_signatures(sigs + [7], "lora-a")) == (t, 12)
    assert st.match(ids + [7], tag_signatures(sigs + [7], "lora-b")) is None
    assert st.match(ids + [7], sigs + [7]) == (e, 12)
    # ties: the earliest inserted
    a, b = HostPrefixStore(10 ** 6, 4), None
    first = a.put(*_rec(100, 8))
    a.put(_rec(100, 8)[0][:6] + [55, 56], _rec(100, 8)[1][:6] + [55, 56])
    assert a.match(_rec(100, 8)[0][:6] + [77, 78], _rec(100, 8)[1][:6] + [77, 78]) == (first, 6) and b is None


def test_wants_too_short_covered_over_budget():
    st = HostPrefixStore(200, 8, row_bytes=10)
    ids, sigs = _rec(100, 12)
    assert not st.wants(ids[:7], sigs[:7])                                  # too short
    assert st.wants(ids[:8], sigs[:8])
    assert not st.wants(*_rec(100, 21))                                     # 210 bytes: more than the budget holds
    assert st.wants(*_rec(100, 20))
    st.put(ids, sigs)
    assert not st.wants(ids, sigs) and not st.wants(ids[:9], sigs[:9])      # equal to / a prefix of a stored entry
    assert st.wants(ids + [5], sigs + [5])                                  # longer than it
    assert st.wants(ids[:9] + [5], sigs[:9] + [5])                          # diverges from it


def test_put_replaces_proper_prefixes():
    st = HostPrefixStore(10 ** 6, 4, row_bytes=10)
    ids, sigs = _rec(100, 20)
    short, other = st.put(ids[:10], sigs[:10], buffer="short"), st.put(*_rec(300, 9), buffer="other")
    long = st.put(ids, sigs, buffer="long")
    assert [e.buffer for e in st.entries] == ["other", "long"] and not short.alive and short.buffer is None and other.alive and long.alive
    assert st.evictions == 0 and st.bytes == 290 and st.peak == 290         # a replacement is no eviction; 100 + 90 before, 90 + 200 after
    assert st.match(ids[:10] + [5], sigs[:10] + [5]) == (long, 10)


def test_lru_under_a_budget_for_two_of_three():
    """Three entries of 10 rows, a budget of exactly two. a, b stored; a used (touch); c evicts b, the least recently used, not a, the
    earliest inserted. Then d evicts a (stamps: a 3, c 4). Untouched entries go in insertion order."""
    st = HostPrefixStore(200, 4, row_bytes=10)
    a, b = st.put(*_rec(100, 10), buffer="a"), st.put(*_rec(200, 10), buffer="b")
    assert st.bytes == 200
    st.touch(st.match(*_rec(100, 11))[0])
    c = st.put(*_rec(300, 10), buffer="c")
    assert [e.buffer for e in st.entries] == ["a", "c"] and not b.alive and st.evictions == 1
    d = st.put(*_rec(400, 10), buffer="d")
    assert [e.buffer for e in st.entries] == ["c", "d"] and not a.alive and c.alive and d.alive and st.evictions == 2
    st.put(*_rec(500, 20), buffer="e")                                      # needs the whole budget: both go, c first
    assert [e.buffer for e in st.entries] == ["e"] and st.evictions == 4 and st.bytes == 200 == st.peak
    fresh = HostPrefixStore(200, 4, row_bytes=10)
    x, y = fresh.put(*_rec(100, 10)), fresh.put(*_rec(200, 10))
    fresh.put(*_rec(300, 10))
    assert not x.alive and y.alive


def test_a_hit_waits_for_the_copy_not_for_time():
    class Event:
        waited = 0

        def synchronize(self):
            Event.waited += 1

    st = HostPrefixStore(10 ** 6, 4)
    e = st.put(*_rec(100, 10), buffer="rows", event=Event())
    e.wait()
    e.wait()
    assert Event.waited == 1 and e.event is None


def test_two_equal_call_sequences_give_equal_entry_lists():
    def run():
        st = HostPrefixStore(350, 4, row_bytes=10)
        for k in (1, 2, 3, 1, 4, 2, 5):
            ids, sigs = _rec(100 * k, 8 + k)
            m = st.match(ids + [9], sigs + [9])
            if m is not None and m[1] >= 4:
                st.touch(m[0])
            if st.wants(ids, sigs):
                st.put(ids, sigs)
        return st.describe(), st.evictions, st.peak
    one, two = run(), run()
    assert one == two and one[1] >= 1 and len(one[0]) >= 2


# ---- the simulator ------------------------------------------------------------------------------------------------------------------
A1 = [1] + list(range(100, 121))                                             # conversation A: 22 ids
U = [[1] + list(range(200 + 10 * k, 205 + 10 * k)) for k in range(3)]        # three unrelated prompts of 6 ids
GEN = [[7, 8], [30, 31, 32, 33, 34, 35], [40, 41], [50, 51], [60, 61]]
A2 = A1 + GEN[0] + [90, 91, 92]                                              # A's second turn: 27 ids
QUEUE, LENGTHS = [A1] + U + [A2], [2, 6, 2, 2, 2]


def test_simulate_prefix_with_the_host_tier_on_a_hand_computed_queue():
    """2 slots, min_tokens 8 on both tiers, 100 bytes a row, an ample budget. Lengths 2, 6, 2, 2, 2.
      pass 1  A1 -> slot 0, U1 -> slot 1: 22 + 6 = 28 rows prefilled.
      step 1  A1 finishes; slot 0 holds its 22 prompt rows + 1 fed id = 23 rows.
      pass 2  U2 takes slot 0 in place on the shared BOS row (start 1): the 23-row record keeps 1 row, so it is SPILLED (23 rows,
              2300 bytes); the host match of U2 is that one row: no restore. 5 rows prefilled, 1 hit.
      step 2  U2 finishes: slot 0 holds 6 + 1 = 7 rows, fewer than 8: never spilled.
      pass 3  U3 -> slot 0, start 1: 5 prefilled, 1 hit.        step 3  U3 finishes (7 rows).
      pass 4  A2 -> slot 0, start 1 from the device (BOS). The host entry agrees with A2 on all its 23 rows (A1 + the fed 7): 23 >= 8 and
              23 > 1, so it is RESTORED: start 23, 4 rows prefilled, 23 hit.
      steps 4, 5  A2 finishes, then U1 (live alone in step 5).
    decode_steps 5, live_slot_steps 2 + 2 + 2 + 2 + 1 = 9, parked 1, 4 prefill passes; prefill_tokens 28 + 5 + 5 + 4 = 42,
    prefix_hit_tokens 1 + 1 + 23 = 25 (42 + 25 = the 67 prompt rows), nothing forked; host: 1 spill of 23 rows, 1 restore of 23 rows,
    no eviction, peak 2300 bytes. Without the tier A2 keeps only the BOS row: 64 prefilled, 3 hit."""
    got = simulate_prefix(QUEUE, LENGTHS, 2, min_tokens=8, generated=GEN, host_bytes=10 ** 6, host_min_tokens=8, row_bytes=100)
    want = dict(decode_steps=5, live_slot_steps=9, parked_slot_steps=1, admissions=5, prefill_passes=4, finish_order=[0, 2, 3, 4, 1],
                prefill_tokens=42, prefix_hit_tokens=25, forked_tokens=0, fork_launches=0, host_spills=1, host_spill_tokens=23,
                host_restores=1, host_restore_tokens=23, host_evictions=0, host_bytes_peak=2300)
    assert got == want
    plain = simulate_prefix(QUEUE, LENGTHS, 2, min_tokens=8, generated=GEN)
    assert plain["prefill_tokens"] == 64 and plain["prefix_hit_tokens"] == 3
    # a budget below the record: nothing is spilled, nothing restored, the counters are there and zero
    small = simulate_prefix(QUEUE, LENGTHS, 2, min_tokens=8, generated=GEN, host_bytes=2299, host_min_tokens=8, row_bytes=100)
    assert all(small[k] == 0 for k in HOST_KEYS) and {k: v for k, v in small.items() if k not in HOST_KEYS} == plain
    # a restore threshold above the match: spilled, not restored
    high = simulate_prefix(QUEUE, LENGTHS, 2, min_tokens=8, generated=GEN, host_bytes=10 ** 6, host_min_tokens=24, row_bytes=100)
    assert high["host_spills"] == 0 and high["host_restores"] == 0          # (23 rows < 24: not worth a spill either)


def test_host_bytes_zero_is_todays_dict():
    lengths = [5, 9, 3, 7, 2, 6, 6, 4]
    prompts = [[1] + [100 * (k % 3 + 1) + i for i in range(19)] + [900 + k] for k in range(8)]
    for kw in (dict(), dict(max_admit=2), dict(min_tokens=4, adapters=[None, "a"] * 4)):
        today = simulate_prefix(prompts, lengths, 4, **kw)
        off = simulate_prefix(prompts, lengths, 4, host_bytes=0, host_min_tokens=8, row_bytes=1234, **kw)
        assert off == today and list(off) == list(today) and not set(HOST_KEYS) & set(off)
    assert simulate_prefix(QUEUE, LENGTHS, 2, generated=GEN, host_bytes=0) == simulate_prefix(QUEUE, LENGTHS, 2, generated=GEN)


def test_the_store_outlives_the_device_records():
    """A second call that finds no device record (an outside write moved the epoch: a fresh PrefixIndex here) restores from the store
    the first call left behind."""
    store = HostPrefixStore(10 ** 6, 8, row_bytes=100)
    one = simulate_prefix(QUEUE[:4], LENGTHS[:4], 2, min_tokens=8, generated=GEN[:4], host_store=store)
    assert one["host_spills"] == 1 and one["host_restores"] == 0 and store.bytes == 2300
    two = simulate_prefix([A2], [2], 2, min_tokens=8, index=PrefixIndex(2), host_store=store)
    assert two["host_restores"] == 1 and two["host_restore_tokens"] == 23 and two["prefill_tokens"] == 4
    assert two["host_bytes_peak"] == 2300 and two["host_evictions"] == 0


# ---- the engine's refusals ----------------------------------------------------------------------------------------------------------
def test_engine_refuses_before_touching_the_llm():
    from seedx_amd.seed_x import ContinuousLVLM
    bare = ContinuousLVLM(object(), None, None)
    assert bare.prefix_host_bytes == 0 and bare.prefix_host_min_tokens == ContinuousLVLM.PREFIX_HOST_MIN_TOKENS == 8
    ok = dict(input_ids=[[1, 2]])
    bare.prefix_host_bytes = 1 << 20
    with pytest.raises(ValueError, match="prefix_host_bytes needs agent.prefix_cache"):
        bare.generate_inflight(None, [ok])
    bare.prefix_cache = True
    for bad in (-1, 1.5, True):
        bare.prefix_host_bytes = bad
        with pytest.raises(ValueError, match="prefix_host_bytes must be an int >= 0"):
            bare.generate_inflight(None, [ok])
    bare.prefix_host_bytes, bare.prefix_host_min_tokens = 1 << 20, 0
    with pytest.raises(ValueError, match="prefix_host_min_tokens must be an int >= 1"):
        bare.generate_inflight(None, [ok])
    # off: the call gets as far as it ever did (the stand-in has no ``comm``)
    bare.prefix_host_bytes, bare.prefix_host_min_tokens = 0, 8
    with pytest.raises(AttributeError):
        bare.generate_inflight(None, [ok])


# ---- C-ABI --------------------------------------------------------------------------------------------------------------------------
def _fields(src, cname):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        decl = re.sub(r"^(const\s+)?(void|float|double|int32_t|int64_t|uint32_t|uint64_t|sx_kv_tensor)\s*\*?", "", decl)
        names += [re.sub(r"\[\d+\]$", "", n.strip().lstrip("*")) for n in decl.split(",")]
    return names


def test_kv_rows_struct_layout_matches_header():
    from seedx_amd import _lib
    src = open(os.path.join(ROOT, "include", "seedx_hip.h")).read()
    assert _fields(src, "sx_kv_tensor") == [f[0] for f in _lib.KvTensor._fields_]
    assert _fields(src, "sx_kv_rows_args") == [f[0] for f in _lib.KvRowsArgs._fields_]
    assert ctypes.sizeof(_lib.KvTensor) == 40 and ctypes.sizeof(_lib.KvRowsArgs) == 4 * 40 + 8 * 8 + 8 * 4
    assert "sx_kv_rows_copy" in _lib.SIGNATURES and "sx_kv_rows_job_bytes" in _lib.SIGNATURES


def test_job_bytes_host_rule_is_the_librarys():
    """ops.kv_rows_bytes (stand-in tensors: only shapes are read) against sx_kv_rows_job_bytes, which the entry point itself uses."""
    import torch
    from seedx_amd import _lib, ops
    lib = _lib.load()
    for Tmax in (37, 64):
        caches = [torch.empty((2, 3, 3, Tmax, 128), dtype=torch.uint8, device="meta"), torch.empty((2, 3, 3, Tmax, 64), dtype=torch.float16, device="meta"),
                  torch.empty((2, 3, 3, Tmax), dtype=torch.float32, device="meta")]
        rb = (ctypes.c_int32 * 4)(128, 128, 4, 0)
        for n in (-3, 0, 1, 2, 3, 4, 5, 20, Tmax, Tmax + 9):
            got = ops.kv_rows_bytes(caches, n)
            assert got == lib.sx_kv_rows_job_bytes(rb, 3, 2, 3, Tmax, n) and got % 16 == 0
        assert ops.kv_rows_bytes(caches, 1) == 2 * 3 * (128 + 128 + 16) and ops.kv_rows_bytes(caches, 5) == 2 * 3 * (640 + 640 + 32)
    assert lib.sx_kv_rows_job_bytes(rb, 5, 2, 3, 37, 4) == -1
