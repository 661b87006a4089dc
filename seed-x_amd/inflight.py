"""Slot assignment of in-flight (continuous) batching — host logic only, no GPU and no torch.

``ContinuousLVLM.generate_inflight`` decodes a queue of requests on the G slots of the lock-step decode step. The schedule is:

  * a request with a budget of n tokens gets token 1 from its admission prefill and tokens 2..n from n - 1 decode steps,
  * after every decode step the finished slots are harvested and freed,
  * before the next step the free slots are refilled from the head of the queue, FIFO, lowest slot first — one ADMISSION PASS. A pass
    admits at most ``max_admit`` requests (None: as many as there are free slots) and is made of rounds, each round one batched
    prefill; a request that finishes at its admission (budget 1, or EOS as its first token) frees its slot within the pass, so a
    later round of the same pass may refill it while the pass has quota left,
  * a decode step runs whenever at least one slot is live.

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

    def admit(self):
        """One round of the current pass: [(slot, request)] for the free slots, lowest slot first, queue head first."""
        out = []
        for g in range(self.n_slots):
            if not self.queue or self.quota <= 0:
                break
            if self.slot_req[g] is None:
                self.slot_req[g] = self.queue.popleft()
                self.quota -= 1
                out.append((g, self.slot_req[g]))
        return out

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


def lockstep_wave_steps(lengths, n_slots):
    """Decode steps of the lock-step alternative: FIFO waves of ``n_slots`` requests, every wave as long as its longest member."""
    lengths = [int(n) for n in lengths]
    return sum(max(lengths[i:i + n_slots]) - 1 for i in range(0, len(lengths), n_slots))
