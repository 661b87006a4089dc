"""In-flight batching against lock-step waves on the 13B-dimension LLM (synthetic weights, bench.py's LLM phase construction:
16 slots, fp16, default precise mode). ONE process, two workloads, the two schedules alternated --reps times after a warm-up run of
each, device-synchronised wall clocks:

  mixed   : 64 text requests, budgets drawn (seeded) from 16..128. (a) generate_batch in FIFO waves of 16, every wave run to its
            longest member's budget; (b) generate_inflight. Generated tokens / s (the tokens the requests asked for), decode steps,
            admissions, prefill ms, and the wall ratio next to the ratio the step counts predict.
  uniform : 16 requests of budget 128 (the shape the headline runs): ms per token step of both paths, against the spread between
            the repeated lock-step runs of this very call.

Prefill ms come from one extra, instrumented run per schedule (a synchronised clock around every batched prefill); the timed runs
carry no extra synchronisation. Prints one JSON line per run and per summary; --out writes the tables + raw lines as markdown.

    python tools/bench_inflight.py --out profiles/inflight_serving.md
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from seedx_amd.inflight import lockstep_wave_steps, simulate

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--slots", type=int, default=16)
ap.add_argument("--requests", type=int, default=64)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert a.reps >= 3, "alternate the schedules at least three times"
G = bench.BATCH = a.slots
dev = torch.device("cuda:0")
_, agent, _ = bench.build_models(dev, torch.float16, need=("llm",), max_cache_len=1024)
llm, tok = agent.llm, bench.BenchTokenizer()
rng = np.random.default_rng(a.seed)
LINES = []


def emit(d):
    LINES.append(json.dumps(d))
    print(LINES[-1], flush=True)


def make_requests(budgets):
    return [dict(input_ids=[[1] + rng.integers(3, 31000, size=int(rng.integers(16, 49))).tolist()], max_new_tokens=int(b))
            for b in budgets]


class PrefillClock:
    """Synchronised wall clock around llm.forward_embeds_batch (instrumented runs only)."""

    def __init__(self):
        self.ms, self.calls = 0.0, 0

    def __enter__(self):
        inner = self.inner = llm.forward_embeds_batch

        def timed(*args, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = inner(*args, **kw)
            torch.cuda.synchronize()
            self.ms += (time.perf_counter() - t0) * 1e3
            self.calls += 1
            return out
        llm.forward_embeds_batch = timed
        return self

    def __exit__(self, *exc):
        del llm.forward_embeds_batch          # back to the class's method


def run_lockstep(reqs):
    n = 0
    for i in range(0, len(reqs), G):
        wave = reqs[i:i + G]
        plain = [{k: v for k, v in r.items() if k != "max_new_tokens"} for r in wave]
        plain += [plain[-1]] * (G - len(plain))                      # generate_batch wants exactly G requests: pad the last wave
        outs = agent.generate_batch(tok, plain, max_new_tokens=max(r["max_new_tokens"] for r in wave), eos_token_id=None)
        n += sum(min(len(o["generate_ids"]), r["max_new_tokens"]) for o, r in zip(outs, wave))
    return n


def run_inflight(reqs):
    return sum(len(o["generate_ids"]) for o in agent.generate_inflight(tok, reqs, eos_token_id=None))


def wall(fn, reqs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = fn(reqs)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, n


def workload(name, budgets):
    reqs = make_requests(budgets)
    want = int(sum(budgets))
    pred = simulate(budgets, G)
    steps = {"lockstep": lockstep_wave_steps(budgets, G), "inflight": pred["decode_steps"]}
    fns = {"lockstep": run_lockstep, "inflight": run_inflight}
    prefill = {}
    for sched, fn in fns.items():                                    # warm-up = the instrumented run
        with PrefillClock() as pc:
            ms, n = wall(fn, reqs)
        assert n == want, (sched, n, want)
        prefill[sched] = dict(ms=pc.ms, passes=pc.calls)
        emit(dict(workload=name, schedule=sched, run="warmup+prefill-clock", wall_ms=round(ms, 2), prefill_ms=round(pc.ms, 2),
                  prefill_passes=pc.calls))
    assert agent.last_inflight_stats["decode_steps"] == steps["inflight"], (agent.last_inflight_stats, pred)
    walls = {"lockstep": [], "inflight": []}
    for rep in range(a.reps):
        for sched, fn in fns.items():
            ms, n = wall(fn, reqs)
            assert n == want
            walls[sched].append(ms)
            emit(dict(workload=name, schedule=sched, run=rep, wall_ms=round(ms, 2), tokens=n, tokens_per_s=round(n / ms * 1e3, 1),
                      decode_steps=steps[sched]))
    med = {k: float(np.median(v)) for k, v in walls.items()}
    spread = {k: float(max(v) - min(v)) for k, v in walls.items()}
    summary = dict(
        workload=name, summary=True, requests=len(budgets), slots=G, tokens=want, reps=a.reps,
        lockstep=dict(wall_ms=round(med["lockstep"], 2), spread_ms=round(spread["lockstep"], 2), decode_steps=steps["lockstep"],
                      tokens_per_s=round(want / med["lockstep"] * 1e3, 1), prefill_ms=round(prefill["lockstep"]["ms"], 2),
                      prefill_passes=prefill["lockstep"]["passes"], admissions=len(budgets)),
        inflight=dict(wall_ms=round(med["inflight"], 2), spread_ms=round(spread["inflight"], 2), decode_steps=steps["inflight"],
                      tokens_per_s=round(want / med["inflight"] * 1e3, 1), prefill_ms=round(prefill["inflight"]["ms"], 2),
                      prefill_passes=prefill["inflight"]["passes"], admissions=agent.last_inflight_stats["admissions"],
                      live_slot_steps=pred["live_slot_steps"], parked_slot_steps=pred["parked_slot_steps"]),
        wall_ratio=round(med["lockstep"] / med["inflight"], 4), step_ratio=round(steps["lockstep"] / steps["inflight"], 4))
    for k in ("lockstep", "inflight"):      # decode-only view: wall minus the prefills measured in the instrumented run
        summary[k]["ms_per_step_total"] = round(med[k] / steps[k], 4)
        summary[k]["ms_per_step_decode"] = round((med[k] - prefill[k]["ms"]) / steps[k], 4)
    summary["step_spread_ms_lockstep"] = round(spread["lockstep"] / steps["lockstep"], 4)
    emit(summary)
    return summary


mixed = workload("mixed", rng.integers(16, 129, size=a.requests).tolist())
uniform = workload("uniform", [128] * G)

if a.out:
    def row(name, s):
        return (f"| {name} | {s['wall_ms']:.1f} | {s['spread_ms']:.1f} | {s['tokens_per_s']:.0f} | {s['decode_steps']} | {s['admissions']} | "
                f"{s['prefill_passes']} | {s['prefill_ms']:.1f} | {s['ms_per_step_total']:.3f} | {s['ms_per_step_decode']:.3f} |")
    head = ("| schedule | wall ms (median) | spread ms (max - min) | generated tokens / s | decode steps | admissions | prefill passes | "
            "prefill ms | ms / step (wall) | ms / step (wall - prefill) |\n|---|---|---|---|---|---|---|---|---|---|")
    md = [f"# In-flight batching vs lock-step waves (tools/bench_inflight.py, {G} slots, 13B dims, fp16, precise mode)", ""]
    for s, title in ((mixed, f"Mixed workload: {mixed['requests']} text requests, budgets 16..128 (seed {a.seed}), {mixed['tokens']} tokens"),
                     (uniform, f"Uniform workload: {G} requests of budget 128")):
        md += [f"## {title}", "", head, row("lock-step waves (generate_batch)", s["lockstep"]),
               row("in-flight (generate_inflight)", s["inflight"]), "",
               f"Wall ratio lock-step / in-flight: **{s['wall_ratio']:.3f}**; decode-step ratio: **{s['step_ratio']:.3f}**; "
               f"lock-step spread per step: {s['step_spread_ms_lockstep']:.4f} ms ({s['reps']} alternated repeats).", ""]
    md += ["## Raw lines", "", "```"] + LINES + ["```", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(md))
