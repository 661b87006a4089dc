"""Slot assignment of in-flight (continuous) batching — host logic only, no GPU and no torch.

``ContinuousLVLM.generate_inflight`` decodes a queue of requests on the G slots of the lock-step decode step. The schedule is:

  * a request with a budget of n tokens gets token 1 from its admission prefill and tokens 2..n from n - 1 decode steps,
  * after every decode step the finished slots are harvested and freed,
  * before the next step the free slots are refilled from the head of the queue, FIFO, lowest slot first — one ADMISSION PASS. A pass
    admits at most ``max_admit`` requests (None: as many as there are free slots) and is made of rounds, each round one batched
    prefill; a request that finishes at its admission (budget 1, or EOS as its first token) frees its slot within the pass, so a
    later round of the same pass may refill it while the pass has quota left,
  * a decode step runs whenever at least one slot is live.

With ``prefix_cache=True`` the engine also remembers what every slot's KV cache holds (``PrefixIndex``) and lets ``plan_admission``
choose the slots of a round: a request whose prompt starts like a slot's record keeps those rows (in place, when the slot is free) or
gets them copied from the donor slot by one sx_kv_fork launch, and prefills only the rest. The requests admitted per pass, hence the
decode-step counts, are those of the plain schedule; ``simulate_prefix`` is ``simulate``'s counterpart with the token counts. Records a
slot is about to lose may be parked in host memory and restored later (kvstore.py: ``simulate_prefix(host_bytes=...)`` counts that too).

On a paged KV cache (``LlamaForCausalLM(kv_pages=N)``) a request is admitted only when the pages for its prompt and budget are free:
``SlotScheduler.admit(fits)`` stops a round at a queue head that does not fit, and ``simulate_paged`` is ``simulate`` with that gate.

``SlotScheduler`` turns finish events into admissions; ``simulate`` drives it with known lengths and counts steps, which is what
the tests compare the engine's ``last_inflight_stats`` with and what tools/bench_inflight.py prints next to its wall clocks. A forced
image block is a host-driven chunk that takes no decode step: give ``simulate`` a request's length minus its chunk tokens.
"""
from collections import deque


class SlotScheduler:
    def __init__(self, n_slots, n_requests, max_admit=None):
        assert n_slots >= 1 and n_requests >= 0 and (max_admit is None or max_admit >= 1)
        self.n_slots, self.max_admit = int(n_slots), max_admit
        self.queue = deque(range(int(n_requests)))
        self.slot_req = [None] * self.n_slots          # request index held by each slot (None: free)
        self.quota = 0
        self.new_pass()

    def new_pass(self):
        """Start an admission pass: resets the pass's quota."""
        self.quota = self.n_slots if self.max_admit is None else int(self.max_admit)

    def admit(self, fits=None):
        """One round of the current pass: [(slot, request)] for the free slots, lowest slot first, queue head first.
        ``fits(slot, request)`` (the paged KV cache: it reserves the request's pages for the slot, or returns False): a queue head that
        does not fit WAITS — the round ends there and nothing overtakes it, so admission stays first in, first out."""
        out = []
        for g in range(self.n_slots):
            if not self.queue or self.quota <= 0:
                break
            if self.slot_req[g] is None:
                if fits is not None and not fits(g, self.queue[0]):
                    break
                self.slot_req[g] = self.queue.popleft()
                self.quota -= 1
                out.append((g, self.slot_req[g]))
        return out

    def candidates(self):
        """The requests the next ``admit()`` would take, in queue order, without taking them (prefix planning: plan_admission)."""
        n = min(sum(r is None for r in self.slot_req), len(self.queue), max(self.quota, 0))
        return [self.queue[i] for i in range(n)]

    def free_slots(self):
        return [g for g, r in enumerate(self.slot_req) if r is None]

    def place(self, slot, request):
        """Admits ``request`` (one of ``candidates()``) into the free ``slot``: what ``admit()`` does, with the slot chosen by the caller."""
        assert self.slot_req[slot] is None and self.quota > 0, f"slot {slot} is not free or the pass has no quota left"
        self.queue.remove(request)
        self.slot_req[slot] = request
        self.quota -= 1

    def finish(self, slot):
        """The request in ``slot`` ended: frees the slot, returns the request index."""
        r = self.slot_req[slot]
        assert r is not None, f"slot {slot} holds no request"
        self.slot_req[slot] = None
        return r

    def live_slots(self):
        return [g for g, r in enumerate(self.slot_req) if r is not None]

    @property
    def done(self):
        return not self.queue and all(r is None for r in self.slot_req)


def simulate(lengths, n_slots, max_admit=None):
    """Step counts of the schedule for requests that produce ``lengths[i]`` tokens (>= 1 each). Returns a dict with decode_steps,
    live_slot_steps, parked_slot_steps, admissions (requests admitted), prefill_passes (batched prefills run) and finish_order."""
    lengths = [int(n) for n in lengths]
    assert all(n >= 1 for n in lengths)
    sch = SlotScheduler(n_slots, len(lengths), max_admit)
    made = {}
    stats = dict(decode_steps=0, live_slot_steps=0, parked_slot_steps=0, admissions=0, prefill_passes=0, finish_order=[])
    while not sch.done:
        sch.new_pass()
        while True:
            adm = sch.admit()
            if not adm:
                break
            stats["admissions"] += len(adm)
            stats["prefill_passes"] += 1
            for g, r in adm:
                made[g] = 1                                   # token 1 comes from the admission prefill
                if made[g] >= lengths[r]:
                    stats["finish_order"].append(sch.finish(g))
        live = sch.live_slots()
        if not live:
            continue
        stats["decode_steps"] += 1
        stats["live_slot_steps"] += len(live)
        stats["parked_slot_steps"] += n_slots - len(live)
        for g in live:
            made[g] += 1
            if made[g] >= lengths[sch.slot_req[g]]:
                stats["finish_order"].append(sch.finish(g))
    return stats


def simulate_paged(prompt_lens, lengths, n_slots, n_pages, page_size, max_admit=None, budgets=None):
    """``simulate`` on a paged KV cache of ``n_pages`` pages of ``page_size`` rows (paging.PagePool): request i is admitted only when
    the pages for its ``prompt_lens[i]`` prompt rows plus its budget are free, and holds them until it finishes; a queue head that does
    not fit waits for a finishing request's pages and nothing overtakes it. ``budgets[i]``: the rows reserved beyond the prompt (the
    request's ``max_new_tokens``); None: ``lengths[i]`` — the two differ for a request that stops early (EOS) or whose ``lengths``
    entry leaves out a forced image chunk's tokens, as for ``simulate``. Returns simulate's dict plus page_waits (admission rounds
    that ended at a queue head that did not fit while a slot was free) and peak_pages (most pages held at once). With an ample pool the
    counts are simulate's. ValueError for a request that can never fit."""
    from .paging import PagePool, pages_for
    lengths = [int(n) for n in lengths]
    budgets = lengths if budgets is None else [int(b) for b in budgets]
    rows = [int(p) + b for p, b in zip(prompt_lens, budgets)]
    assert len(rows) == len(lengths) and all(n >= 1 for n in lengths)
    for i, n in enumerate(rows):
        if pages_for(n, page_size) > n_pages:
            raise ValueError(f"simulate_paged: request {i} needs {pages_for(n, page_size)} pages of {page_size} rows for {n} rows, "
                             f"the pool holds {n_pages}")
    pool = PagePool(n_pages, page_size, n_slots, max(rows))
    sch = SlotScheduler(n_slots, len(lengths), max_admit)
    made = {}
    stats = dict(decode_steps=0, live_slot_steps=0, parked_slot_steps=0, admissions=0, prefill_passes=0, finish_order=[], page_waits=0,
                 peak_pages=0)

    def finish(g):
        stats["finish_order"].append(sch.finish(g))
        pool.release(g)

    while not sch.done:
        sch.new_pass()
        before = stats["admissions"]
        while True:
            adm = sch.admit(lambda g, r: pool.reserve(g, rows[r]))
            if not adm:
                stats["page_waits"] += bool(sch.queue and sch.quota > 0 and sch.free_slots())
                break
            stats["admissions"] += len(adm)
            stats["prefill_passes"] += 1
            for g, r in adm:
                made[g] = 1                                   # token 1 comes from the admission prefill
                if made[g] >= lengths[r]:
                    finish(g)
        live = sch.live_slots()
        assert live or sch.done or stats["admissions"] > before, "a request that fits an empty pool is always admitted"
        if not live:
            continue
        stats["decode_steps"] += 1
        stats["live_slot_steps"] += len(live)
        stats["parked_slot_steps"] += n_slots - len(live)
        for g in live:
            made[g] += 1
            if made[g] >= lengths[sch.slot_req[g]]:
                finish(g)
    stats["peak_pages"] = pool.peak
    return stats


def simulate_spec(lengths, n_slots, emitted, max_admit=None):
    """``simulate`` for the verify step of speculative decoding (agent.speculative): the k-th decode step request i is live in emits
    ``emitted[i][k]`` tokens (>= 1; what the accept rule kept) instead of one; a count that overshoots the request's length is cut there.
    Returns simulate's dict plus emitted_tokens (tokens produced by decode steps)."""
    lengths = [int(n) for n in lengths]
    assert all(n >= 1 for n in lengths) and len(emitted) == len(lengths)
    sch = SlotScheduler(n_slots, len(lengths), max_admit)
    made, k = {}, {}
    stats = dict(decode_steps=0, live_slot_steps=0, parked_slot_steps=0, admissions=0, prefill_passes=0, finish_order=[], emitted_tokens=0)
    while not sch.done:
        sch.new_pass()
        while True:
            adm = sch.admit()
            if not adm:
                break
            stats["admissions"] += len(adm)
            stats["prefill_passes"] += 1
            for g, r in adm:
                made[g], k[g] = 1, 0                          # token 1 comes from the admission prefill
                if made[g] >= lengths[r]:
                    stats["finish_order"].append(sch.finish(g))
        live = sch.live_slots()
        if not live:
            continue
        stats["decode_steps"] += 1
        stats["live_slot_steps"] += len(live)
        stats["parked_slot_steps"] += n_slots - len(live)
        for g in live:
            r = sch.slot_req[g]
            e = int(emitted[r][k[g]])
            assert e >= 1
            e = min(e, lengths[r] - made[g])
            made[g] += e
            k[g] += 1
            stats["emitted_tokens"] += e
            if made[g] >= lengths[r]:
                stats["finish_order"].append(sch.finish(g))
    return stats


def lockstep_wave_steps(lengths, n_slots):
    """Decode steps of the lock-step alternative: FIFO waves of ``n_slots`` requests, every wave as long as its longest member."""
    lengths = [int(n) for n in lengths]
    return sum(max(lengths[i:i + n_slots]) - 1 for i in range(0, len(lengths), n_slots))


# ---- prefix reuse: what a slot's cache holds, and who may take it ------------------------------------------------------------------
def _common_prefix(ids_a, sigs_a, ids_b, sigs_b, cap):
    """Rows [0, p), p <= cap, on which the token ids AND the row signatures agree."""
    m = min(len(ids_a), len(ids_b), cap)
    p = 0
    while p < m and ids_a[p] == ids_b[p] and sigs_a[p] == sigs_b[p]:
        p += 1
    return p


def tag_signatures(sigs, adapter):
    """Row signatures of a request that runs under the LoRA adapter ``adapter``: KV rows depend on the adapter that computed them, so every
    row's signature carries its name — (signature, adapter). Records and prompts then agree on a row only under the same adapter, and a
    prefix is kept or forked only among requests of one adapter. None (the base model) leaves the signatures as they are, so a queue
    without adapters keeps its records; an untagged signature never equals a tagged one."""
    return list(sigs) if adapter is None else [(s, adapter) for s in sigs]


class PrefixIndex:
    """What the KV cache of each of ``n_slots`` slots holds: the token ids of its rows, one opaque hashable signature per row (the
    engine: a fingerprint of the row's input embedding, so that image rows with equal ids and different features differ — tagged with the
    request's LoRA adapter, ``tag_signatures``), the KV epoch
    the record was made under and a last-use stamp from a clock that only moves forward (0: never used)."""

    def __init__(self, n_slots):
        self.n_slots = int(n_slots)
        self.rec = [None] * self.n_slots               # (ids, sigs, epoch) or None
        self.stamp = [0] * self.n_slots
        self.clock = 0

    def touch(self, slot):
        self.clock += 1
        self.stamp[slot] = self.clock

    def record(self, slot, ids, sigs, epoch):
        ids, sigs = list(ids), list(sigs)
        assert len(ids) == len(sigs), "one signature per row"
        self.rec[slot] = (ids, sigs, epoch)
        self.touch(slot)

    def invalidate(self, slot):
        self.rec[slot] = None

    def restamp(self, old_epoch, new_epoch):
        """The owner of the cache moved the epoch from ``old_epoch`` to ``new_epoch`` itself, without touching a recorded row: records
        made under ``old_epoch`` stay valid. Records of any other epoch stay stale."""
        self.rec = [None if r is None else ((r[0], r[1], new_epoch) if r[2] == old_epoch else r) for r in self.rec]

    def match(self, ids, sigs, epoch):
        """[(slot, p)] with p >= 1, longest first (lowest slot on ties): the slot's record agrees with the prompt on ids and signatures of
        rows [0, p). p is capped at len(ids) - 1: at least one token must be forwarded. Records of another epoch never match."""
        out = []
        for g, r in enumerate(self.rec):
            if r is None or r[2] != epoch:
                continue
            p = _common_prefix(r[0], r[1], ids, sigs, len(ids) - 1)
            if p >= 1:
                out.append((g, p))
        return sorted(out, key=lambda t: (-t[1], t[0]))


def plan_admission(index, free_slots, live_slots, requests, min_tokens, epoch=0):
    """One admission round with prefix reuse. ``requests``: [(request, ids, sigs)] in queue order — exactly the requests
    ``SlotScheduler.admit`` would take, so at most len(free_slots). Returns (plan, deferred): plan = [(slot, request, start, donor)] in
    queue order — the request goes to ``slot``, rows [0, start) of its prompt are already there (donor None) or are to be copied from
    slot ``donor`` BEFORE the round's prefill, rows [start, len) are to be prefilled — and ``deferred`` = the requests left for the next
    round of the same pass. The rules:
      * in place first: the longest match in a free slot nobody took yet is taken as it is (any length, no copy; among free slots that
        tie on a match shorter than ``min_tokens`` — every prompt starts with the same BOS id — the least recently used one, so that
        a one-row match does not pick the slot with the youngest record); of two requests that
        want one free slot the earlier gets it,
      * fork otherwise: a match of >= ``min_tokens`` rows in a live slot (rows below a live request's prompt length are never rewritten)
        or in a free slot an earlier request of the round took IN PLACE is copied into another free slot — of the second kind only the
        rows that request keeps (its ``start``), so no donor is handed to a request that overwrites the forked rows,
      * a shorter match is dropped: start 0, no donor,
      * same-round sharing: a request that shares >= ``min_tokens`` rows with an EARLIER request of the round, and more than with any
        slot, is deferred (and so is every request behind one it shares most with); next round it forks from its leader's slot,
      * victims: a request without a slot of its own overwrites the free slot with the oldest last-use stamp, lowest index on ties —
        chosen after every in-place claim, never a slot the round reads from.
    The index is only read: whoever carries the plan out stamps the donors (``index.touch``) and records the slots."""
    free, live = list(free_slots), set(live_slots)
    assert len(requests) <= len(free), "more requests than free slots"
    placed, deferred, seen = [], [], []             # placed: [request, slot | None, start, donor]
    kept = {}                                       # free slot taken in place -> rows it keeps
    for r, ids, sigs in requests:
        ids, sigs = list(ids), list(sigs)
        matches = [(g, p) for g, p in index.match(ids, sigs, epoch) if g in live or g in free]
        # longest first; a free slot before a live one; short ties by last use (equal lengths are all short or all long)
        matches.sort(key=lambda t: (-t[1], t[0] in live, index.stamp[t[0]] if t[1] < min_tokens else 0, t[0]))
        best = matches[0][1] if matches else 0
        shared = max([_common_prefix(i2, s2, ids, sigs, len(ids) - 1) for i2, s2 in seen], default=0)
        seen.append((ids, sigs))
        if shared >= min_tokens and shared > best:
            deferred.append(r)
            continue
        choice = [r, None, 0, None]
        for g, p in matches:
            if g in free and g not in kept and all(c[1] != g for c in placed):
                choice = [r, g, p, None]
                kept[g] = p
                break
            rows = p if g in live else min(p, kept.get(g, 0))
            if rows >= min_tokens:
                choice = [r, None, rows, g]
                break
        placed.append(choice)
    donors = {c[3] for c in placed if c[3] is not None}
    pool = sorted((g for g in free if g not in kept), key=lambda g: (index.stamp[g], g))
    assert not donors & set(pool), "a donor slot must not be overwritten in its own round"
    for c in placed:
        if c[1] is None:
            c[1] = pool.pop(0)
    return [(c[1], c[0], c[2], c[3]) for c in placed], deferred


def simulate_prefix(prompts, lengths, n_slots, max_admit=None, min_tokens=16, sigs=None, generated=None, index=None, adapters=None,
                    host_bytes=0, host_min_tokens=16, row_bytes=1, host_store=None):
    """``simulate`` with prefix reuse: request i has the prompt ids ``prompts[i]`` (row signatures ``sigs[i]``; None: the ids themselves)
    and produces ``lengths[i]`` tokens by decode steps (a forced image chunk's tokens left out, as for ``simulate``). ``generated[i]``
    (optional) are ALL the ids it produced: a finished slot then holds its prompt and every produced id but the last, which later
    turns may match; without it only the prompt. ``index``: a PrefixIndex to start from and leave behind (None: empty). Returns
    ``simulate``'s dict — same decode_steps, live_slot_steps, parked_slot_steps and admissions: only the slots differ — with
    prefill_passes counting the rounds actually run, plus prefill_tokens (rows forwarded at admission), prefix_hit_tokens (rows not
    forwarded), forked_tokens (those of them that were copied) and fork_launches (rounds with at least one copy).
    ``adapters[i]`` (optional): the LoRA adapter request i runs under, or None — its rows' signatures, prompt rows and fed-back rows
    alike, are tagged with it (``tag_signatures``) exactly as the engine tags them.
    ``host_bytes`` > 0 (default 0: nothing changes, no key is added) adds the host-memory tier of kvstore.py with that budget: every
    round runs ``kvstore.plan_host_tier`` behind ``plan_admission`` exactly as the engine does, on a ``HostPrefixStore(host_bytes,
    host_min_tokens, row_bytes)`` without buffers (``row_bytes``: the cache bytes of one token, ``llm.kv_row_bytes``), or on
    ``host_store``, a store to start from and leave behind, as a second call of the engine finds it. The dict then also predicts
    host_spills, host_spill_tokens, host_restores, host_restore_tokens (rows copied back: prefix hits, none of them forked),
    host_evictions and host_bytes_peak (most bytes the store held during the call)."""
    lengths = [int(n) for n in lengths]
    prompts = [list(p) for p in prompts]
    sigs = prompts if sigs is None else [list(s) for s in sigs]
    adapters = [None] * len(prompts) if adapters is None else list(adapters)
    assert len(adapters) == len(prompts)
    sigs = [tag_signatures(s, a) for s, a in zip(sigs, adapters)]
    assert len(prompts) == len(lengths) == len(sigs) and all(n >= 1 for n in lengths)
    sch = SlotScheduler(n_slots, len(lengths), max_admit)
    index = PrefixIndex(n_slots) if index is None else index
    made = {}
    stats = dict(decode_steps=0, live_slot_steps=0, parked_slot_steps=0, admissions=0, prefill_passes=0, finish_order=[],
                 prefill_tokens=0, prefix_hit_tokens=0, forked_tokens=0, fork_launches=0)
    store = host_store
    if host_bytes or store is not None:
        from .kvstore import HostPrefixStore, plan_host_tier
        store = HostPrefixStore(host_bytes, host_min_tokens, row_bytes) if store is None else store
        stats.update(host_spills=0, host_spill_tokens=0, host_restores=0, host_restore_tokens=0, host_evictions=0, host_bytes_peak=0)
        evicted0, store.peak = store.evictions, store.bytes

    def finish(g):
        r = sch.finish(g)
        stats["finish_order"].append(r)
        fed = list(generated[r])[:-1] if generated is not None else []
        index.record(g, prompts[r] + fed, sigs[r] + tag_signatures(fed, adapters[r]), 0)

    while not sch.done:
        sch.new_pass()
        while True:
            cand = sch.candidates()
            if not cand:
                break
            plan, _ = plan_admission(index, sch.free_slots(), sch.live_slots(), [(r, prompts[r], sigs[r]) for r in cand], min_tokens)
            if store is not None:
                plan, spills, restores = plan_host_tier(store, index, plan, {r: (prompts[r], sigs[r]) for r in cand}, 0, store.min_tokens)
                stats["host_spills"] += len(spills)
                stats["host_spill_tokens"] += sum(e.n_rows for _, e in spills)
                stats["host_restores"] += len(restores)
                stats["host_restore_tokens"] += sum(p for _, _, p in restores)
            stats["admissions"] += len(plan)
            stats["prefill_passes"] += 1
            stats["fork_launches"] += any(d is not None for _, _, _, d in plan)
            for g, r, start, donor in plan:
                if donor is not None:
                    index.touch(donor)
            for g, r, start, donor in plan:
                sch.place(g, r)
                index.record(g, prompts[r], sigs[r], 0)
                stats["prefill_tokens"] += len(prompts[r]) - start
                stats["prefix_hit_tokens"] += start
                stats["forked_tokens"] += start if donor is not None else 0
            for g, r, _, _ in plan:
                made[g] = 1
                if made[g] >= lengths[r]:
                    finish(g)
        live = sch.live_slots()
        if not live:
            continue
        stats["decode_steps"] += 1
        stats["live_slot_steps"] += len(live)
        stats["parked_slot_steps"] += n_slots - len(live)
        for g in live:
            made[g] += 1
            if made[g] >= lengths[sch.slot_req[g]]:
                finish(g)
    if store is not None:
        stats["host_evictions"], stats["host_bytes_peak"] = store.evictions - evicted0, store.peak
    return stats
