"""Host-memory tier of the prefix cache: KV rows that a slot is about to lose are parked in pinned host memory and copied back when a
later prompt starts like them.

``agent.prefix_cache`` (inflight.PrefixIndex) remembers what the KV cache of every slot holds, so its memory is as large as the slots: a
free slot is the victim of the next unrelated request and its record is dropped. With ``agent.prefix_host_bytes > 0`` the engine
(``ContinuousLVLM.generate_inflight``) first SPILLS such a record — one sx_kv_rows_copy launch packs the rows of every layer, head and
cache tensor into a device staging buffer, a side stream copies that to a pinned host buffer — and RESTORES it when a prompt matches:
host to device into staging, one unpack launch into the request's slot, and only the rest of the prompt is prefilled.

Nothing here imports the GPU code when the module is imported: ``HostPrefixStore`` and ``plan_host_tier`` are plain host logic, shared by
the engine and by ``inflight.simulate_prefix`` (which runs them with no buffers at all), and ``KVMover`` imports torch and the kernels
when it is built.

Out of scope, refused where a user can reach them: the paged cache (``prefix_cache`` refuses it), tensor-parallel ranks
(generate_inflight is single-rank), spilling a LIVE request (preemption: only free slots are spilled), sharing a store between models
(a store belongs to one pack and is dropped with it), a disk tier and compression beyond the cache's own format (a spilled row is the
cache's bytes).
"""
from .inflight import _common_prefix


class HostEntry:
    """One spilled record: the token ids and row signatures of its ``n_rows`` rows, the (pinned host) ``buffer`` that holds the rows,
    the ``event`` that completes when the device-to-host copy has finished (None: nothing to wait for), its last-use ``stamp`` and its
    insertion ``order``. ``alive`` turns False when the store drops the entry."""
    __slots__ = ("ids", "sigs", "n_rows", "nbytes", "buffer", "event", "stamp", "order", "alive")

    def __init__(self, ids, sigs, nbytes, buffer, event, stamp, order):
        self.ids, self.sigs, self.n_rows, self.nbytes = ids, sigs, len(ids), nbytes
        self.buffer, self.event, self.stamp, self.order, self.alive = buffer, event, stamp, order, True

    def wait(self):
        """Returns once the entry's rows are in its buffer: a hit never depends on how long the copy took."""
        if self.event is not None:
            self.event.synchronize()
            self.event = None


class HostPrefixStore:
    """Spilled prefix records under a byte budget. An entry costs ``n_rows * row_bytes`` bytes (``row_bytes``: the cache bytes of one
    token, ``llm.kv_row_bytes``; a buffer may add up to 15 padding bytes per span, which the budget does not count). Entries are keyed
    by ids AND signatures: a signature carries the embedding fingerprint and the adapter tag (inflight.tag_signatures), so image rows
    with other features, and rows computed under another adapter, never match. Stamps come from a clock that only moves forward;
    nothing depends on time. Host copies are immutable: the store survives ``llm.reset()``, ``kv_epoch`` changes and outside writes."""

    def __init__(self, budget_bytes, min_tokens, row_bytes=1):
        assert budget_bytes >= 0 and min_tokens >= 1 and row_bytes >= 1
        self.budget, self.min_tokens, self.row_bytes = int(budget_bytes), int(min_tokens), int(row_bytes)
        self.entries = []                              # in insertion order
        self.clock = self.order = self.bytes = self.peak = self.evictions = 0

    def nbytes(self, n_rows):
        return int(n_rows) * self.row_bytes

    def touch(self, entry):
        self.clock += 1
        entry.stamp = self.clock

    def match(self, ids, sigs):
        """(entry, p) with p >= 1: the entry that agrees with the prompt on ids and signatures of the most rows [0, p), the earliest
        inserted on ties; p is capped at len(ids) - 1 (at least one token must be forwarded, as for PrefixIndex.match). None: no entry
        agrees on row 0. Reads only: whoever uses the entry stamps it (``touch``)."""
        best = None
        for e in self.entries:
            p = _common_prefix(e.ids, e.sigs, ids, sigs, len(ids) - 1)
            if p >= 1 and (best is None or p > best[1]):
                best = (e, p)
        return best

    def covers(self, ids, sigs):
        """A stored entry holds these rows already: the record is a prefix of the entry, or equal to it."""
        return any(e.n_rows >= len(ids) and _common_prefix(e.ids, e.sigs, ids, sigs, len(ids)) == len(ids) for e in self.entries)

    def wants(self, ids, sigs):
        """Worth a spill: at least ``min_tokens`` rows, not covered by a stored entry, and within the budget on its own."""
        return len(ids) >= self.min_tokens and self.nbytes(len(ids)) <= self.budget and not self.covers(ids, sigs)

    def _drop(self, entry):
        self.entries.remove(entry)
        self.bytes -= entry.nbytes
        entry.alive, entry.buffer = False, None

    def put(self, ids, sigs, buffer=None, event=None):
        """Stores a record (``wants`` it first). Entries that are a proper prefix of it are replaced: the new one holds their rows.
        Then the least recently used entries — oldest stamp, earliest inserted on ties — are evicted until the new one fits;
        ``evictions`` counts those. Returns the entry."""
        ids, sigs = list(ids), list(sigs)
        assert len(ids) == len(sigs) and self.nbytes(len(ids)) <= self.budget, "HostPrefixStore.put: ask wants() first"
        for e in [e for e in self.entries if e.n_rows < len(ids) and _common_prefix(e.ids, e.sigs, ids, sigs, e.n_rows) == e.n_rows]:
            self._drop(e)
        need = self.nbytes(len(ids))
        while self.bytes + need > self.budget:
            self._drop(min(self.entries, key=lambda e: (e.stamp, e.order)))
            self.evictions += 1
        self.clock += 1
        self.order += 1
        entry = HostEntry(ids, sigs, need, buffer, event, self.clock, self.order)
        self.entries.append(entry)
        self.bytes += need
        self.peak = max(self.peak, self.bytes)
        return entry

    def describe(self):
        """[(ids, n_rows, stamp, order)] of the entries, in insertion order (tests: two equal call sequences give equal lists)."""
        return [(tuple(e.ids), e.n_rows, e.stamp, e.order) for e in self.entries]


def plan_host_tier(store, index, plan, prompts, epoch, min_tokens):
    """The host tier's part of one admission round, between ``plan_admission`` and the round's forks: spill, then restore.
    ``plan``: plan_admission's [(slot, request, start, donor)]; ``prompts[request]`` = (ids, sigs).
      * spill: every planned slot whose record of the current ``epoch`` holds more rows than the request keeps there (its ``start``
        where it keeps the slot in place, nothing where it gets a fork) is about to lose rows; the record goes to the store if the
        store ``wants`` it, in plan order (so a later record of the round sees the earlier ones),
      * restore: a planned request whose longest host match has >= ``min_tokens`` rows and more than its ``start`` takes the entry's
        rows [0, p) instead: start = p, no donor. The entry is stamped.
    Returns (plan, spills, restores): the plan with the restored requests rewritten, spills = [(slot, entry)] (an entry a later put of
    the same round evicted again has ``alive`` False: nothing needs copying) and restores = [(slot, entry, p)]. The index is only
    read; the store is updated."""
    spills, restores, out = [], [], []
    for g, _, start, donor in plan:
        rec = index.rec[g]
        if rec is None or rec[2] != epoch:
            continue
        if len(rec[0]) > (start if donor is None else 0) and store.wants(rec[0], rec[1]):
            spills.append((g, store.put(rec[0], rec[1])))
    for g, r, start, donor in plan:
        m = store.match(*prompts[r])
        if m is not None and m[1] >= min_tokens and m[1] > start:
            store.touch(m[0])
            restores.append((g, m[0], m[1]))
            out.append((g, r, m[1], None))
        else:
            out.append((g, r, start, donor))
    return out, spills, restores


class KVMover:
    """The copies behind ``plan_host_tier``, for one pack ``P`` of cache tensors (needs the GPU: torch and the kernels are imported
    here). ``spill`` packs the rows of a round's spilled slots into one of TWO device staging buffers on the current stream — so the
    pack runs before the round's prefill overwrites the rows — and copies them to pinned host buffers on a side stream behind an
    event; a staging buffer is packed into again only after the event of its last copy has completed. ``restore`` copies the entries
    host to device into a third staging buffer and unpacks them, all on the current stream: the suffix prefill depends on it.
    The staging buffers grow to the largest round they served (1 MiB at least) and stay with the mover."""

    def __init__(self, P):
        import torch
        from . import ops
        self.torch, self.ops, self.P = torch, ops, P
        self.device = P["kc"].device
        self.side = torch.cuda.Stream(self.device)
        self.stage, self.busy, self.turn = [None, None], [None, None], 0
        self.back = None

    def _buffer(self, old, nbytes):
        if old is not None and old.numel() >= nbytes:
            return old
        return self.torch.empty(max(nbytes, 1 << 20), dtype=self.torch.uint8, device=self.device)

    def _jobs(self, rows):
        sizes = [self.ops.kv_rows_bytes(self.P, n) for n in rows]
        return sizes, [sum(sizes[:i]) for i in range(len(sizes))]

    def spill(self, spills):
        """spills: [(slot, entry)] of one round. Sets every living entry's buffer and event."""
        torch = self.torch
        spills = [(g, e) for g, e in spills if e.alive]
        if not spills:
            return
        sizes, offs = self._jobs([e.n_rows for _, e in spills])
        i, self.turn = self.turn, self.turn ^ 1
        if self.busy[i] is not None:                     # the buffer's last device-to-host copies have to be done
            self.busy[i].synchronize()
        self.stage[i] = stage = self._buffer(self.stage[i], sum(sizes))
        self.ops.kv_rows_copy(self.P, [(g, e.n_rows, off) for (g, e), off in zip(spills, offs)], stage, 0)
        packed = torch.cuda.Event()
        packed.record()
        done = torch.cuda.Event()
        with torch.cuda.stream(self.side):
            self.side.wait_event(packed)
            for (_, e), size, off in zip(spills, sizes, offs):
                e.buffer = torch.empty(size, dtype=torch.uint8, pin_memory=True)
                e.buffer.copy_(stage[off:off + size], non_blocking=True)
            done.record()
        for _, e in spills:
            e.event = done
        self.busy[i] = done

    def restore(self, restores):
        """restores: [(slot, entry, p)] of one round: rows [0, p) of every entry into its slot."""
        if not restores:
            return
        sizes, offs = self._jobs([p for _, _, p in restores])
        self.back = back = self._buffer(self.back, sum(sizes))
        for (_, e, p), size, off in zip(restores, sizes, offs):
            e.wait()
            if p == e.n_rows:
                back[off:off + size].copy_(e.buffer)
            else:                                        # a shorter prefix of the entry: its spans are the heads of the entry's spans
                self._copy_prefix(back[off:off + size], e, p)
        self.ops.kv_rows_copy(self.P, [(g, p, off) for (g, _, p), off in zip(restores, offs)], back, 1)

    def _copy_prefix(self, dst, entry, p):
        """The job of rows [0, p) out of the buffer of an entry of n > p rows: span by span (both layouts are [tensor][outer][inner])."""
        caches = self.ops._kv_cache_list(self.P)
        spans = caches[0].shape[0] * caches[0].shape[2]
        src_off = dst_off = 0
        for t in caches:
            rb = self.ops._kv_row_bytes(t)
            full, part = (entry.n_rows * rb + 15) // 16 * 16, (p * rb + 15) // 16 * 16
            src = entry.buffer[src_off:src_off + spans * full].view(spans, full)[:, :p * rb]
            dst[dst_off:dst_off + spans * part].view(spans, part)[:, :p * rb].copy_(src)
            src_off, dst_off = src_off + spans * full, dst_off + spans * part
