"""The paged KV cache's host side, without a GPU: paging.PagePool, inflight.simulate_paged, the constructor's refusals and the
footprint of LlamaForCausalLM(kv_pages=N)."""
import pytest

from oracle import weights


# ---- PagePool --------------------------------------------------------------------------------------------------------------------------
def test_page_pool_reserve_extend_release():
    from seedx_amd.paging import PagePool, pages_for
    pool = PagePool(6, 32, n_slots=3, max_rows=200)
    assert pool.free == 6 and pool.width == pages_for(200, 32) == 7 and pool.pages(0) == []
    assert pool.reserve(0, 33) and pool.pages(0) == [1, 2] and pool.capacity(0) == 64 and pool.free == 4
    assert pool.reserve(0, 33) and pool.reserve(0, 64) and pool.reserve(0, 1) and pool.pages(0) == [1, 2], "idempotent: extend to AT LEAST n_rows"
    assert pool.reserve(1, 32) and pool.pages(1) == [3]
    assert pool.reserve(0, 65) and pool.pages(0) == [1, 2, 4], "an extension keeps the pages already held, in row order"
    assert pool.table_row(0) == [1, 2, 4, 0, 0, 0, 0] and pool.table_row(2) == [0] * 7
    assert pool.free == 2 and pool.used == 4 and pool.peak == 4
    assert pool.release(0) == 3 and pool.pages(0) == [] and pool.free == 5 and pool.release(0) == 0
    assert pool.peak == 4, "the peak stays"
    assert pool.reserve(0, 0) and pool.pages(0) == []


def test_page_pool_exhaustion_grants_nothing():
    from seedx_amd.paging import PagePool
    pool = PagePool(4, 64, n_slots=2, max_rows=1024)
    assert pool.reserve(0, 129) and pool.pages(0) == [1, 2, 3]
    assert not pool.reserve(1, 65), "two pages wanted, one free"
    assert pool.pages(1) == [] and pool.free == 1, "no partial grant"
    assert not pool.reserve(0, 321) and pool.pages(0) == [1, 2, 3] and pool.free == 1, "a failed extension leaves the slot as it was"
    assert pool.reserve(1, 64) and pool.pages(1) == [4] and pool.free == 0
    assert not pool.reserve(1, 65)
    assert not PagePool(100, 32, 1, max_rows=64).reserve(0, 65), "the per-slot ceiling"


def test_page_pool_reuses_freed_pages_lifo_and_never_hands_out_page_zero():
    from seedx_amd.paging import PagePool
    pool = PagePool(5, 128, n_slots=3, max_rows=4096)
    assert pool.reserve(0, 256) and pool.reserve(1, 128) and pool.reserve(2, 129)
    assert (pool.pages(0), pool.pages(1), pool.pages(2)) == ([1, 2], [3], [4, 5]) and pool.free == 0
    pool.release(0)
    assert pool.reserve(1, 300) and pool.pages(1) == [3, 1, 2], "freed pages come back, the slot's first page first"
    pool.release(2)
    pool.release(1)
    assert pool.free == 5
    seen = set()
    for rnd in range(7):                                 # a deterministic churn: every page that is ever handed out lies in 1 .. n_pages
        for g in range(3):
            if (rnd + g) % 3 == 0:
                pool.release(g)
            else:
                pool.reserve(g, 128 * ((rnd + 2 * g) % 3 + 1))
            seen.update(pool.pages(g))
            held = [p for s in range(3) for p in pool.pages(s)]
            assert len(held) == len(set(held)) == pool.used, "a page has one owner"
    assert seen == {1, 2, 3, 4, 5}
    a, b = PagePool(9, 32, 2, 512), PagePool(9, 32, 2, 512)
    for pool in (a, b):
        pool.reserve(0, 100), pool.reserve(1, 40), pool.release(0), pool.reserve(1, 200), pool.reserve(0, 33)
    assert a.pages(0) == b.pages(0) and a.pages(1) == b.pages(1), "deterministic"


def test_page_pool_refuses_bad_geometry():
    from seedx_amd.paging import PagePool
    for ps in (0, 16, 48, 96, 256):
        with pytest.raises(ValueError, match="page_size"):
            PagePool(4, ps, 1, 128)
    with pytest.raises(ValueError):
        PagePool(0, 64, 1, 128)


# ---- simulate_paged --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_admit", [None, 1, 2])
def test_simulate_paged_equals_simulate_on_an_ample_pool(max_admit):
    from seedx_amd.inflight import simulate, simulate_paged
    lengths = [3, 9, 1, 4, 4, 12, 2, 7, 1, 5]
    plens = [5, 70, 33, 64, 1, 200, 31, 32, 90, 17]
    for slots in (1, 3, 4):
        want = simulate(lengths, slots, max_admit)
        got = simulate_paged(plens, lengths, slots, n_pages=1000, page_size=32, max_admit=max_admit)
        assert got.pop("page_waits") == 0 and got.pop("peak_pages") >= 1
        assert got == want


def test_simulate_paged_hand_worked_tight_case():
    """Three slots, pages of 32 rows, a pool of 4 pages; rows reserved = prompt + length:
         r0 30 + 3 = 33 rows → 2 pages, 3 tokens      r1 20 + 5 = 25 → 1 page, 5 tokens
         r2 40 + 30 = 70 → 3 pages, 30 tokens         r3 10 + 2 = 12 → 1 page, 2 tokens
       Worked by hand:
         pass 1: r0 → slot 0 (2 pages), r1 → slot 1 (1 page); r2 wants 3 pages and 1 is free: it waits in front of the free slot 2, and r3,
                 which would fit, does not overtake it                                                          (wait 1)
         step 1: r0, r1 live.   pass 2: r2 still waits (wait 2).   step 2: r0 makes its token 3 and ends: 3 pages free
         pass 3: r2 → slot 0 (3 pages, the pool is full); r3 waits in front of the free slot 2                  (wait 3)
         step 3: r1, r2 live.   pass 4: r3 still waits (wait 4).   step 4: r1 makes its token 5 and ends: 1 page free
         pass 5: r3 → slot 1.   step 5: r2, r3 live; r3 makes its token 2 and ends
         steps 6 .. 31: r2 alone (token 1 at its admission, tokens 2 .. 30 in steps 3 .. 31)
       31 decode steps; live slot steps r0 2 + r1 4 + r2 29 + r3 1; three batched prefills; all 4 pages held at the peak. Unpaged, r2 is
       admitted in pass 1: 29 steps."""
    from seedx_amd.inflight import simulate, simulate_paged
    got = simulate_paged([30, 20, 40, 10], [3, 5, 30, 2], n_slots=3, n_pages=4, page_size=32)
    assert got["finish_order"] == [0, 1, 3, 2]
    assert got["decode_steps"] == 31
    assert got["live_slot_steps"] == 2 + 4 + 29 + 1            # r0: 2 steps, r1: 4, r2: 29, r3: 1
    assert got["parked_slot_steps"] == 3 * 31 - 36
    assert got["admissions"] == 4 and got["prefill_passes"] == 3
    assert got["peak_pages"] == 4
    assert got["page_waits"] == 4
    free = simulate([3, 5, 30, 2], 3)
    assert free["decode_steps"] == 29 and free["finish_order"] == [0, 3, 1, 2], "the unpaged schedule admits r2 at once"
    # budgets beyond the produced length (EOS, or a forced image block left out of ``lengths``) size the reservation
    wide = simulate_paged([30, 20, 40, 10], [3, 5, 30, 2], 3, 4, 32, budgets=[3, 50, 30, 2])     # r1 now holds 3 pages
    assert wide["finish_order"] == [0, 1, 3, 2] and wide["peak_pages"] == 4 and wide["decode_steps"] == 2 + 4 + 29


def test_simulate_paged_refuses_a_request_that_never_fits():
    from seedx_amd.inflight import simulate_paged
    with pytest.raises(ValueError, match="request 1 needs 5 pages"):
        simulate_paged([10, 100], [5, 30], 2, n_pages=4, page_size=32)


# ---- the constructor -------------------------------------------------------------------------------------------------------------------
def _mk(**kw):
    from seedx_amd.llama import LlamaForCausalLM
    return LlamaForCausalLM(dict(weights.MINI_LLM), max_cache_len=1536, max_batch=3, **kw)


@pytest.mark.parametrize("ps", [0, 16, 48, 100, 256])
def test_constructor_refuses_other_page_sizes(ps):
    with pytest.raises(ValueError, match="kv_page_size must be 32, 64 or 128"):
        _mk(kv_pages=8, kv_page_size=ps)


def test_constructor_refusals_name_the_follow_ups():
    with pytest.raises(ValueError, match="kv_pages needs the precise mode"):
        _mk(kv_pages=8, precise=False)
    for fmt in ("fp8_e4m3", "fp8_e4m3_emulated"):
        with pytest.raises(ValueError, match="follow-up: paged row scales"):
            _mk(kv_pages=8, kv_format=fmt)
    with pytest.raises(ValueError, match="follow-up: a page table in the verify kernel"):
        _mk(kv_pages=8, spec_tokens=3)
    with pytest.raises(ValueError, match="head_dim 128"):
        from seedx_amd.llama import LlamaForCausalLM
        LlamaForCausalLM(dict(weights.MINI_LLM, num_attention_heads=4), kv_pages=8)
    with pytest.raises(ValueError, match="kv_pages=-1"):
        _mk(kv_pages=-1)
    off = _mk()                                          # the default: off, any page size ignored
    assert off.kv_pages == 0 and _mk(kv_page_size=48).kv_pages == 0
    with pytest.raises(ValueError, match="kv_pages=0"):
        off.kv_reserve(0, 10)
    for kw in (dict(kv_v16=True), dict(kv_v16=False), dict(weight_format="fp8_e4m3"), dict(weight_format="mxfp4", weight_residency="tiles"),
               dict(max_adapters=2)):
        assert _mk(kv_pages=8, kv_page_size=128, **kw).kv_pages == 8


def test_memory_footprint_reports_the_pool():
    cfg = weights.MINI_LLM
    L, nh, hd = cfg["num_hidden_layers"], cfg["num_attention_heads"], cfg["hidden_size"] // cfg["num_attention_heads"]
    flat = _mk().memory_footprint()
    assert flat["kv_cache"] == L * 3 * nh * 1536 * hd * 8
    for n, ps in ((8, 32), (40, 64), (5, 128)):
        m = _mk(kv_pages=n, kv_page_size=ps)
        fp = m.memory_footprint()
        assert fp["kv_cache"] == L * (n + 1) * nh * ps * hd * (4 + 4), "k and v pools, fp32 until _pack knows the dtype; the null page included"
        assert fp["total"] - fp["kv_cache"] == flat["total"] - flat["kv_cache"]
        m.kv_v16 = True                                  # what _pack decides for an fp16 model
        assert m.memory_footprint()["kv_cache"] == L * (n + 1) * nh * ps * hd * (4 + 2)
