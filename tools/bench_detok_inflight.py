"""In-flight batching of the de-tokenizer against lock-step waves, at full SDXL dimensions (synthetic weights, bench.py's adapter
construction without the VAE: latents out), fp16, 1024 x 1024, G slots. ONE process, device-synchronised wall clocks:

  step   : ms per replay of the slot graph (all G slots live) against the lock-step graph of the same build at the same G, --reps
           repeats of --replays replays each, the two graphs alternated (and their order within a repeat too). The lock-step graph is unchanged code, so the spread between
           its own repeats is the yardstick for the difference.
  queue  : --requests requests with steps drawn from 20..50 by default_rng(seed) and guidance from 3..9. (a) generate() in FIFO waves
           of G, every wave run to its longest member's step count at one guidance scale (what a lock-step batch can do);
           (b) generate_inflight: every request its own steps and guidance. Wall time, UNet steps, and the wall ratio next to the ratio
           the step counts predict (inflight.simulate / lockstep_wave_steps). A parked slot still costs its share of every UNet step:
           the parked share of the slot steps is printed.

Prints one JSON line per measurement; --out writes the tables + raw lines as markdown.

    python tools/bench_detok_inflight.py --out profiles/detok_inflight.md
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from seedx_amd.inflight import lockstep_wave_steps, simulate

ap = argparse.ArgumentParser()
ap.add_argument("--slots", type=int, default=8)
ap.add_argument("--requests", type=int, default=32)
ap.add_argument("--reps", type=int, default=8)
ap.add_argument("--replays", type=int, default=10)
ap.add_argument("--queue-reps", type=int, default=1)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--out", default=None)
a = ap.parse_args()
G, MAX_STEPS = a.slots, 128
assert a.reps >= 3 and a.replays <= MAX_STEPS, "at least three repeats; the replays of a repeat are one schedule"
dev = torch.device("cuda:0")
bench.USE_VAE = False
_, _, ad = bench.build_models(dev, torch.float16, need=("adapter",))
rng = np.random.default_rng(a.seed)
LINES = []


def emit(d):
    LINES.append(json.dumps(d))
    print(LINES[-1], flush=True)


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


steps = [int(s) for s in rng.integers(20, 51, a.requests)]
guidance = [float(g) for g in rng.uniform(3.0, 9.0, a.requests).round(2)]
gen = torch.Generator().manual_seed(a.seed)
feats = torch.randn(a.requests, 1, 64, 4096, generator=gen).to(dev)             # what the LLM's output resampler hands over
noise = torch.randn(a.requests, 1, 4, a.size // 8, a.size // 8, generator=gen)
requests = [dict(image_embeds=feats[i], latents=noise[i], num_inference_steps=steps[i], guidance_scale=guidance[i]) for i in range(a.requests)]
size = dict(height=a.size, width=a.size)

# ---- step: slot graph against lock-step graph --------------------------------------------------------------------------------
ad.generate(image_embeds=torch.cat(list(feats[:G])), latents=torch.cat(list(noise[:G])), num_inference_steps=a.replays, guidance_scale=7.5,
            output_type="latent", **size)                                        # captures the lock-step graph at G; a.replays steps
lock = ad._loop
ad.generate_inflight([dict(r, num_inference_steps=1) for r in requests[:G]], slots=G, max_steps=MAX_STEPS, output_type="latent", **size)
slot = ad._slot_loop
# the slot loop gets the lock-step batch's own G requests (same conditioning, noise, a.replays steps, guidance 7.5), so both graphs work
# on the same numbers: kernel time and clocks depend on the data. Every repeat restarts both from the slot loop's state at step 0,
# which is the lock-step loop's (same expressions).
entries = []
for g in range(G):
    pe, pe_neg, pool, pool_neg = ad.get_image_embeds(image_embeds=feats[g], return_negative=True)
    entries.append((g, dict(latents=noise[g], num_steps=a.replays, guidance_scale=7.5, image_guidance_scale=1.5, ehs=torch.cat([pe_neg, pe]),
                            pooled=torch.cat([pool_neg, pool]), tid=ad._time_ids(a.size, a.size, 2), image_latents=None)))
slot.admit(entries, ad.scheduler)
start = {k: slot._state[k].clone() for k in ("lat", "scaled")}
assert all(torch.equal(lock._state[k], slot._state[k]) for k in ("ehs", "pooled", "tid"))


def replay_lock():
    for _ in range(a.replays):
        lock._graph.replay()


def replay_slot():
    for _ in range(a.replays):
        slot._graph.replay()


def restart():
    for loop in (lock, slot):
        for k, v in start.items():
            loop._state[k].copy_(v)
        loop._state["step"].zero_()                                             # all slots live again; the lock-step tables hold a.replays steps


ms = dict(lock=[], slot=[])
for rep in range(a.reps + 1):                                                   # repeat 0 warms both up
    pair = (("lock", replay_lock), ("slot", replay_slot))
    restart()
    for name, fn in (pair if rep % 2 else pair[::-1]):                          # the order alternates: neither graph always runs second
        t, _ = clock(fn)
        if rep:
            ms[name].append(t / a.replays)
    assert torch.equal(lock._state["lat"], slot._state["lat"]), "the two graphs took the same steps on the same data"
slot.park_all()
med = {k: statistics.median(v) for k, v in ms.items()}
spread = max(ms["lock"]) - min(ms["lock"])
emit(dict(what="step", G=G, replays=a.replays, lock_ms=[round(x, 3) for x in ms["lock"]], slot_ms=[round(x, 3) for x in ms["slot"]],
          lock_median_ms=round(med["lock"], 3), slot_median_ms=round(med["slot"], 3), lock_spread_ms=round(spread, 3),
          slot_minus_lock_ms=round(med["slot"] - med["lock"], 3), within_spread=bool(abs(med["slot"] - med["lock"]) <= spread)))

# ---- queue: waves against in-flight ------------------------------------------------------------------------------------------
sim = simulate([s + 1 for s in steps], G)
wave_steps = lockstep_wave_steps([s + 1 for s in steps], G)


def run_waves():
    out = []
    for i in range(0, a.requests, G):
        n = min(G, a.requests - i)
        out.append(ad.generate(image_embeds=torch.cat(list(feats[i:i + n])), latents=torch.cat(list(noise[i:i + n])),
                               num_inference_steps=max(steps[i:i + n]), guidance_scale=7.5, output_type="latent", **size))
    return out


def run_inflight():
    return ad.generate_inflight(requests, slots=G, max_steps=MAX_STEPS, output_type="latent", **size)


wall = dict(waves=[], inflight=[])
for rep in range(a.queue_reps):
    for name, fn in (("waves", run_waves), ("inflight", run_inflight)):
        t, _ = clock(fn)
        wall[name].append(t)
        emit(dict(what="queue", schedule=name, rep=rep, wall_s=round(t / 1e3, 3),
                  unet_steps=wave_steps if name == "waves" else ad.last_inflight_stats["unet_steps"],
                  stats=None if name == "waves" else ad.last_inflight_stats))
st = ad.last_inflight_stats
assert st["unet_steps"] == sim["decode_steps"] and st["graph_captures"] == 1
w, f = min(wall["waves"]), min(wall["inflight"])
wave_max = [a.replays] + [max(steps[i:i + G]) for i in range(0, a.requests, G)]     # the lock-step graph is re-captured when its key changes
wave_captures = sum(x != y for x, y in zip(wave_max, wave_max[1:]))
parked_share = st["parked_slot_steps"] / (st["parked_slot_steps"] + st["live_slot_steps"])
emit(dict(what="queue summary", requests=a.requests, G=G, steps_min=min(steps), steps_max=max(steps), steps_sum=sum(steps),
          waves_s=round(w / 1e3, 3), inflight_s=round(f / 1e3, 3), wall_ratio=round(w / f, 3), wave_unet_steps=wave_steps,
          inflight_unet_steps=st["unet_steps"], step_ratio=round(wave_steps / st["unet_steps"], 3),
          parked_slot_steps=st["parked_slot_steps"], parked_share=round(parked_share, 4), admission_passes=st["admission_passes"],
          graph_captures=st["graph_captures"], wave_graph_captures=wave_captures))

if a.out:
    s, q = json.loads(LINES[0]), json.loads(LINES[-1])
    with open(a.out, "w") as fh:
        fh.write(f"""# In-flight batching of the de-tokenizer: slot step and mixed queue

`python tools/bench_detok_inflight.py --out {a.out}` — MI355X, full SDXL UNet (synthetic weights), fp16, {a.size} x {a.size}, G = {G} slots
(UNet batch {2 * G}), no VAE decode (latents out), one process, device-synchronised wall clocks.

## Slot step against lock-step step

{a.reps} repeats of {a.replays} graph replays each on the same {G} requests ({a.replays} steps, guidance 7.5: both graphs compute the same latents), the two graphs alternated (their order
within a repeat too) after one warm-up repeat of each. The lock-step graph is unchanged
code; its own repeat-to-repeat spread is the yardstick.

| graph | ms per replay, by repeat | median |
|---|---|---|
| lock-step (`_DenoiseLoop`) | {s['lock_ms']} | {s['lock_median_ms']} |
| slot (`_SlotDenoiseLoop`, all {G} slots live) | {s['slot_ms']} | {s['slot_median_ms']} |

Slot minus lock-step: {s['slot_minus_lock_ms']} ms per step; spread of the lock-step repeats (max - min): {s['lock_spread_ms']} ms;
inside that spread: **{s['within_spread']}**.

## Mixed queue

{q['requests']} requests, steps drawn from 20..50 by `default_rng({a.seed})` (min {q['steps_min']}, max {q['steps_max']}, sum {q['steps_sum']}), guidance from 3..9.
Waves: `generate` on FIFO waves of {G}, each run to its longest member's step count at ONE guidance scale (a lock-step batch shares both),
one graph capture whenever the step count differs from the wave before ({q['wave_graph_captures']} here). In flight: `generate_inflight`, every request its own steps and guidance, one
capture ({q['graph_captures']}) for the whole queue. Best of {a.queue_reps} run(s) each; both loops were warmed up by the step measurement above, the waves still re-capture when their step count changes.

| schedule | wall s | UNet steps |
|---|---|---|
| lock-step waves | {q['waves_s']} | {q['wave_unet_steps']} |
| in flight | {q['inflight_s']} | {q['inflight_unet_steps']} |

Wall ratio waves / in flight: **{q['wall_ratio']}x**, next to the simulated step ratio **{q['step_ratio']}x** (`inflight.simulate` /
`lockstep_wave_steps`; the engine's counts equal the simulation's). The wall ratio also holds the admissions ({q['admission_passes']} passes:
conditioning per request and the cross-attention K / V at the full batch shape) and the waves' captures.

Parked slots are not compacted out of the UNet batch: a parked slot still costs its full share of every UNet step. Here
{q['parked_slot_steps']} of {q['parked_slot_steps'] + q['steps_sum']} slot steps ({100 * q['parked_share']:.1f} %) were parked — the drain at the end of the queue,
when fewer than {G} requests are left.

## Raw lines

```
""" + "\n".join(LINES) + "\n```\n")
