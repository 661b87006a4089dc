"""Prefix KV reuse of in-flight batching (agent.prefix_cache, ops.kv_fork / sx_kv_fork) on 13B dimensions. Four parts, every shape from
the flags:

  counts    : host only, always computed. The mixed queue of tools/bench_inflight.py (--requests budgets drawn, seeded, from 16..128)
              rebuilt so that groups of --group requests share a --prefix-len token prefix, on --slots slots:
              inflight.simulate_prefix next to inflight.simulate.
  fork      : ops.kv_fork, one slot to another, at the 13B cache dims (L 40, 40 heads, head_dim 128, --tmax rows) for p in --rows, in the
              mixed (fp32 K + 16-bit V), fp32 and FP8 (codes + row scales) formats, against one torch slice ``copy_`` per cache tensor
              over the same bytes: same process, alternated --reps times after a warm-up, device events around --inner calls each.
              GB/s = bytes copied (read once, written once: 2 x) / time.
  crossover : on the model below, a --prompt token prefill into one slot against fork(p) from a slot that holds the prompt + the
              (prompt - p)-token suffix prefill, alternated; the smallest p from which the fork wins.
  workload  : the counts queue on ONE synthetic model of --layers 13B-dim layers (40: the whole LLM; bench.py's construction, --slots
              slots, fp16, default precise mode), agent.prefix_cache True against False, alternated --reps times after an
              instrumented warm-up run of each (a synchronised clock around every batched prefill and fork): wall ms, prefill ms,
              generated tokens / s. The records are dropped before every cached run, so each run starts cold.

Without a GPU only ``counts`` runs and the timing columns read "not measured". Prints one JSON line per run; --out writes markdown.

    python tools/bench_prefix_cache.py --out profiles/prefix_cache.md
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seedx_amd.inflight import simulate, simulate_prefix
from seedx_amd.seed_x import ContinuousLVLM

ap = argparse.ArgumentParser()
ap.add_argument("--parts", default="counts,fork,crossover,workload")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--slots", type=int, default=16)
ap.add_argument("--requests", type=int, default=64)
ap.add_argument("--group", type=int, default=4)
ap.add_argument("--prefix-len", type=int, default=1536)
ap.add_argument("--min-tokens", type=int, default=ContinuousLVLM.PREFIX_MIN_TOKENS)     # the engine's default
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--rows", default="64,256,1536")
ap.add_argument("--tmax", type=int, default=4096)
ap.add_argument("--inner", type=int, default=50)
ap.add_argument("--layers", type=int, default=40)
ap.add_argument("--prompt", type=int, default=256)
ap.add_argument("--cross-rows", default="2,4,8,16,32,64,128")
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert a.reps >= 3, "alternate the two sides at least three times"
parts = set(a.parts.split(","))
LINES = []
NM = "not measured"


def emit(d):
    LINES.append(json.dumps(d))
    print(LINES[-1], flush=True)


def have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


GPU = have_gpu()
rng = np.random.default_rng(a.seed)
budgets = rng.integers(16, 129, size=a.requests).tolist()
prompts = []
for k in range(0, a.requests, a.group):
    prefix = [1] + rng.integers(3, 31000, size=a.prefix_len - 1).tolist()
    for _ in range(min(a.group, a.requests - k)):
        prompts.append(prefix + rng.integers(3, 31000, size=int(rng.integers(16, 49))).tolist())

# ---- counts (host) -----------------------------------------------------------------------------------------------------------------
plain, cached = simulate(budgets, a.slots), simulate_prefix(prompts, budgets, a.slots, min_tokens=a.min_tokens)
plain["prefill_tokens"] = sum(len(p) for p in prompts)
for k in ("decode_steps", "live_slot_steps", "parked_slot_steps", "admissions"):
    assert plain[k] == cached[k], (k, plain[k], cached[k])
emit(dict(part="counts", requests=a.requests, slots=a.slots, group=a.group, prefix_len=a.prefix_len, tokens=int(sum(budgets)),
          uncached={k: plain[k] for k in ("decode_steps", "admissions", "prefill_passes", "prefill_tokens")},
          cached={k: cached[k] for k in ("decode_steps", "admissions", "prefill_passes", "prefill_tokens", "prefix_hit_tokens",
                                         "forked_tokens", "fork_launches")}))

fork_rows, cross, work = [], None, None
if GPU and parts & {"fork", "crossover", "workload"}:
    import torch

    import bench
    from seedx_amd import ops
    from seedx_amd import synthetic as syn
    dev = torch.device("cuda:0")

    def events(fn, n):
        """ms per call of fn over n back-to-back calls between two device events."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    def alternate(fns, n):
        """{name: [ms per call] x reps}: one warm-up of each, then the sides alternated."""
        for fn in fns.values():
            events(fn, 2)
        out = {k: [] for k in fns}
        for _ in range(a.reps):
            for k, fn in fns.items():
                out[k].append(events(fn, n))
        return out

    # ---- fork bandwidth -----------------------------------------------------------------------------------------------------------
    if "fork" in parts:
        L, nh, hd, G, T = 40, 40, 128, 2, a.tmax
        formats = {"mixed (fp32 K + fp16 V)": [(torch.float32, hd), (torch.float16, hd)],
                   "fp32 (K and V)": [(torch.float32, hd), (torch.float32, hd)],
                   "fp8_e4m3 (codes + fp32 row scales)": [(torch.uint8, hd), (torch.uint8, hd), (torch.float32, 0), (torch.float32, 0)]}
        for name, spec in formats.items():
            caches = [torch.zeros((L, G, nh, T) + ((w,) if w else ()), dtype=dt, device=dev) for dt, w in spec]
            for t in caches:
                t[:, 0].view(torch.uint8).random_(0, 120)              # (bytes below 0x78: no NaN pattern in any of the formats)
            row = sum(t.element_size() * (t.shape[4] if t.dim() == 5 else 1) for t in caches)
            for p in [int(v) for v in a.rows.split(",")]:
                nbytes = L * nh * p * row

                def kernel():
                    ops.kv_fork(caches, [(0, 1, p)])

                def loop():
                    for t in caches:
                        t[:, 1, :, :p].copy_(t[:, 0, :, :p])
                ms = alternate({"kv_fork": kernel, "copy_loop": loop}, a.inner)
                assert all(torch.equal(t[:, 1, :, :p], t[:, 0, :, :p]) for t in caches)
                r = dict(part="fork", format=name, rows=p, bytes_copied=nbytes, launches=len(caches))
                for k, v in ms.items():
                    med = float(np.median(v))
                    r[k] = dict(us=round(med * 1e3, 2), spread_us=round((max(v) - min(v)) * 1e3, 2),
                                gbps=round(2 * nbytes / med / 1e6, 1))
                fork_rows.append(r)
                emit(r)
            del caches
            torch.cuda.empty_cache()

    agent = None
    if parts & {"crossover", "workload"}:
        from seedx_amd.llama import LlamaForCausalLM
        from seedx_amd.visual_encoder import Resampler
        cfg = dict(syn.FULL_LLM, num_hidden_layers=a.layers)
        llm = LlamaForCausalLM(cfg, max_cache_len=max(a.prefix_len + 48 + 128 + 64, a.prompt + 64), max_batch=a.slots)
        llm.load_state_dict(syn.llama_state_dict(cfg, dev, torch.float16))
        llm.to(dev, torch.float16)
        P = llm._pack()
        torch.cuda.empty_cache()
        agent = ContinuousLVLM(llm, Resampler(8, llm.H, 32, kv_dim=4096), Resampler(8, 4096, 32, kv_dim=llm.H), add_patch_pos=True,
                               vit_down=True)
        agent.load_state_dict(syn.agent_state_dict(llm.H, 4096, dev, torch.float16))
        agent.eval().to(dev, torch.float16)

    # ---- crossover ----------------------------------------------------------------------------------------------------------------
    if "crossover" in parts:
        x = torch.randn(a.prompt, llm.H, generator=torch.Generator().manual_seed(a.seed)).to(dev) * 0.5
        llm.reset()
        llm.forward_embeds_batch([x], [0])                             # slot 0 holds the prompt: the donor

        def full():
            llm.set_position(1, 0)
            llm.forward_embeds_batch([x], [1])

        def forked(p):
            def fn():
                ops.kv_fork(P, [(0, 1, p)])
                llm.set_position(1, p)
                llm.forward_embeds_batch([x[p:]], [1])
            return fn
        rows = []
        for p in [int(v) for v in a.cross_rows.split(",") if int(v) < a.prompt]:
            ms = alternate({"full": full, "fork": forked(p)}, 5)
            r = dict(part="crossover", layers=a.layers, prompt=a.prompt, rows=p,
                     full_ms=round(float(np.median(ms["full"])), 4), full_spread_ms=round(max(ms["full"]) - min(ms["full"]), 4),
                     fork_ms=round(float(np.median(ms["fork"])), 4), fork_spread_ms=round(max(ms["fork"]) - min(ms["fork"]), 4))
            r["fork_wins"] = max(ms["fork"]) < min(ms["full"])           # every repeat of the fork side below every repeat of the other
            rows.append(r)
            emit(r)
        wins = [r["rows"] for i, r in enumerate(rows) if all(q["fork_wins"] for q in rows[i:])]
        cross = dict(rows=rows, smallest_winning_rows=wins[0] if wins else None)
        emit(dict(part="crossover", summary=True, smallest_winning_rows=cross["smallest_winning_rows"]))

    # ---- workload -----------------------------------------------------------------------------------------------------------------
    if "workload" in parts:
        tok = bench.BenchTokenizer()
        agent.prefix_min_tokens = a.min_tokens
        reqs = [dict(input_ids=[p], max_new_tokens=int(b)) for p, b in zip(prompts, budgets)]
        want = int(sum(budgets))

        class Clock:
            """Synchronised wall clocks around llm.forward_embeds_batch and ops.kv_fork (instrumented runs only)."""

            def __enter__(self):
                self.ms = {"prefill": 0.0, "fork": 0.0}
                self.inner = (llm.forward_embeds_batch, ops.kv_fork)

                def timed(key, inner):
                    def fn(*args, **kw):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        out = inner(*args, **kw)
                        torch.cuda.synchronize()
                        self.ms[key] += (time.perf_counter() - t0) * 1e3
                        return out
                    return fn
                llm.forward_embeds_batch = timed("prefill", self.inner[0])
                ops.kv_fork = timed("fork", self.inner[1])
                return self

            def __exit__(self, *exc):
                del llm.forward_embeds_batch
                ops.kv_fork = self.inner[1]

        def run(on):
            agent.prefix_cache = on
            if agent._inflight is not None:
                agent._inflight["prefix"] = None                       # every run starts without records
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = agent.generate_inflight(tok, reqs, eos_token_id=None)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, [o["generate_ids"].tolist() for o in out]

        sides = {"uncached": False, "cached": True}
        clocks, ids, stats = {}, {}, {}
        for k, on in sides.items():                                    # warm-up = the instrumented run
            with Clock() as c:
                ms, ids[k] = run(on)
            clocks[k], stats[k] = c.ms, dict(agent.last_inflight_stats)
            assert sum(len(i) for i in ids[k]) == want
            emit(dict(part="workload", side=k, run="warmup+clocks", wall_ms=round(ms, 2), prefill_ms=round(c.ms["prefill"], 2),
                      fork_ms=round(c.ms["fork"], 3), stats=stats[k]))
        for k in ("decode_steps", "admissions", "prefill_passes", "prefill_tokens", "prefix_hit_tokens", "forked_tokens", "fork_launches"):
            assert stats["cached"][k] == cached[k], (k, stats["cached"], cached)
        same = sum(x == y for x, y in zip(ids["cached"], ids["uncached"]))
        walls = {k: [] for k in sides}
        for rep in range(a.reps):
            for k, on in sides.items():
                ms, got = run(on)
                walls[k].append(ms)
                emit(dict(part="workload", side=k, run=rep, wall_ms=round(ms, 2), tokens_per_s=round(want / ms * 1e3, 1)))
        work = dict(identical_id_lists=same, requests=a.requests, tokens=want)
        for k in sides:
            med = float(np.median(walls[k]))
            work[k] = dict(wall_ms=round(med, 1), spread_ms=round(max(walls[k]) - min(walls[k]), 1), tokens_per_s=round(want / med * 1e3, 1),
                           prefill_ms=round(clocks[k]["prefill"], 1), fork_ms=round(clocks[k]["fork"], 2))
        work["wall_ratio"] = round(work["uncached"]["wall_ms"] / work["cached"]["wall_ms"], 3)
        emit(dict(part="workload", summary=True, **work))

if a.out:
    md = ["# Prefix KV reuse for in-flight batching (tools/bench_prefix_cache.py)", ""]
    if not GPU:
        md += ["**Timings: not measured.** This file was written without a GPU: it holds only what the schedule counts (host simulation, "
               "`seedx_amd.inflight.simulate_prefix` / `simulate`). `python tools/bench_prefix_cache.py --out profiles/prefix_cache.md` on an "
               "MI355X fills in the fork bandwidth, the crossover and the wall clocks.", ""]
    md += [f"## Counts: {a.requests} text requests in groups of {a.group} sharing a {a.prefix_len}-token prefix, budgets 16..128 "
           f"(seed {a.seed}), {int(sum(budgets))} generated tokens, {a.slots} slots, min_tokens {a.min_tokens}", "",
           "| engine | decode steps | admissions | prefill passes | prefilled tokens | prefix-hit tokens | forked tokens | fork launches | "
           "wall ms (median) | spread ms | prefill ms | fork ms | generated tokens / s |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, key, s in (("`prefix_cache = False`", "uncached", plain), ("`prefix_cache = True`", "cached", cached)):
        w = work[key] if work else None
        md.append(f"| {name} | {s['decode_steps']} | {s['admissions']} | {s['prefill_passes']} | {s['prefill_tokens']} | "
                  f"{s.get('prefix_hit_tokens', 0)} | {s.get('forked_tokens', 0)} | {s.get('fork_launches', 0)} | "
                  + (f"{w['wall_ms']} | {w['spread_ms']} | {w['prefill_ms']} | {w['fork_ms']} | {w['tokens_per_s']} |" if w else
                     f"{NM} | {NM} | {NM} | {NM} | {NM} |"))
    md += [""]
    if work:
        md += [f"Model: {a.layers} layers of 13B dims, synthetic weights, fp16, precise mode. "
               f"Wall ratio uncached / cached: **{work['wall_ratio']}** ({a.reps} alternated repeats after one instrumented warm-up run of each; "
               f"prefill and fork ms come from that instrumented run). {work['identical_id_lists']} of {work['requests']} requests produced "
               "identical ids on both sides (synthetic weights: near-tied logits may flip on the last bits of a reused row).", ""]
    md += ["## Fork bandwidth: `ops.kv_fork` (one `sx_kv_fork` launch per cache tensor) against one torch slice `copy_` per cache tensor", ""]
    if fork_rows:
        md += [f"13B cache dims (L 40, 40 heads, head_dim 128, Tmax {a.tmax}), slot 0 to slot 1, {a.reps} alternated repeats of {a.inner} calls "
               "between device events; GB/s counts every byte read and written.", "",
               "| format | rows p | bytes copied | launches | kv_fork µs | spread µs | kv_fork GB/s | copy_ loop µs | spread µs | copy_ loop GB/s |",
               "|---|---|---|---|---|---|---|---|---|---|"]
        for r in fork_rows:
            k, c = r["kv_fork"], r["copy_loop"]
            md.append(f"| {r['format']} | {r['rows']} | {r['bytes_copied']} | {r['launches']} | {k['us']} | {k['spread_us']} | {k['gbps']} | "
                      f"{c['us']} | {c['spread_us']} | {c['gbps']} |")
        lost = [f"{r['format']} at p = {r['rows']} ({r['kv_fork']['us']} against {r['copy_loop']['us']} µs, {r['kv_fork']['gbps']} against "
                f"{r['copy_loop']['gbps']} GB/s)" for r in fork_rows if r["kv_fork"]["us"] >= r["copy_loop"]["us"]]
        md += ["", ("`ops.kv_fork` loses to the `copy_` loop in: " + "; ".join(lost) + ". It wins in the other rows." if lost else
                    "`ops.kv_fork` beats the `copy_` loop in every row.")]
    else:
        md += [f"Rows {a.rows} in the mixed, fp32 and FP8 formats: {NM}."]
    md += ["", "## Crossover for `prefix_min_tokens`", ""]
    if cross:
        md += [f"{a.layers} layers of 13B dims, {a.slots} slots, a {a.prompt}-token prompt: full prefill against fork(p) + (prompt - p)-token prefill, {a.reps} "
               "alternated repeats of 5 calls. The fork wins at p when every repeat of its side is below every repeat of the other.", "",
               "| rows p | full prefill ms | spread ms | fork + suffix ms | spread ms | fork wins |", "|---|---|---|---|---|---|"]
        md += [f"| {r['rows']} | {r['full_ms']} | {r['full_spread_ms']} | {r['fork_ms']} | {r['fork_spread_ms']} | {'yes' if r['fork_wins'] else 'no'} |"
               for r in cross["rows"]]
        md += ["", f"Smallest p from which the fork wins at every measured p above it: **{cross['smallest_winning_rows']}**. This times one request: "
               "a fork and a shorter prefill against a full prefill in the SAME pass. `prefix_min_tokens` is also the length from which a "
               "request waits one round for a leader of its own round, which costs a batched prefill pass of its own (one more stream of "
               "the weights while the other slots wait); that cost is not in this table. The engine's default is "
               f"{ContinuousLVLM.PREFIX_MIN_TOKENS}: the largest value repeated runs gave (`profiles/prefix_cache_crossover_runs.md`)."]
    else:
        md += [f"{NM}."]
    md += ["", "## Raw lines", "", "```"] + LINES + ["```", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(md))
