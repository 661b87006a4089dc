"""What device-side sampling costs: sx_sample_next_slots against sx_greedy_next_slots in ONE process.

  kernel : G = 16 and 32 rows of the real width (V = 32330, ld = 32384, normal * 4 logits). Every timed sample is a captured graph of
           --launches iterations of [refresh the logits (the in-place edit must not change the work), restore cur, ONE launch of the
           kernel], replayed between two events; the variants (refresh only, greedy, sampled with the reference defaults 0.7 / 50 / 0.5,
           sampled with top_k = 0 / top_p = 0.9 at T = 0.7) are alternated --reps times. us per launch = median over the repeats, less
           the refresh-only graph; spread = max - min over the repeats.
  step   : (--step) the 16-slot token step of tools/bench_inflight.py's uniform workload (13B dimensions, synthetic weights, fp16,
           precise mode, 16 requests of budget 128) through generate_inflight with an all-greedy queue and with a half-sampled queue
           (every other request do_sample, reference defaults), alternated --reps times: ms per token step, and the kernel
           difference as a share of it.

Prints one JSON line per measurement; --out writes the tables + raw lines as markdown.

    python tools/bench_sample_next.py --step --out profiles/sampling.md
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seedx_amd import ops
from seedx_amd.llama import SampleState
from seedx_amd.sampling import SamplingParams

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--launches", type=int, default=50, help="kernel launches per captured graph (one timed sample)")
ap.add_argument("--step", action="store_true", help="also time the 16-slot token step (builds the 13B-dimension LLM)")
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert a.reps >= 3, "alternate the variants at least three times"
dev = torch.device("cuda:0")
V, LD = 32330, 32384
IMG = torch.arange(32100, 32166, dtype=torch.int32, device=dev)       # <img>, 64 image tokens, </img>
VARIANTS = {"refresh only": None, "greedy": "greedy", "sampled 0.7 / 50 / 0.5": (0.7, 50, 0.5), "sampled 0.7 / 0 / 0.9": (0.7, 0, 0.9)}
LINES = []


def emit(d):
    LINES.append(json.dumps(d))
    print(LINES[-1], flush=True)


def kernel_graphs(G):
    """One captured graph per variant: a.launches x [logits refresh, cur restore, launch]."""
    i32 = lambda v: torch.full((G,), v, dtype=torch.int32, device=dev)
    master = torch.from_numpy((np.random.default_rng(0).normal(size=(G, LD)) * 4.0).astype(np.float32)).to(dev)
    graphs = {}
    for name, var in VARIANTS.items():
        logits, cur0, cur = master.clone(), i32(7), i32(7)
        live, n_new, max_new, force_at = i32(1), i32(1), i32(1 << 30), i32(-1)
        pos, ctx, step, status = i32(10), i32(11), i32(1), torch.zeros((G, 4), dtype=torch.int32, device=dev)
        ss = SampleState(G, dev)
        if isinstance(var, tuple):
            ss.set_rows(range(G), [SamplingParams(True, var[0], var[1], var[2], seed=1000 + g) for g in range(G)])

        def body():
            for _ in range(a.launches):
                logits.copy_(master)
                cur.copy_(cur0)
                if var == "greedy":
                    ops.greedy_next_slots(logits, V, IMG, cur, live, n_new, max_new, force_at, pos, ctx, step, None, status)
                elif var is not None:
                    ops.sample_next_slots(logits, V, IMG, cur, live, n_new, max_new, force_at, pos, ctx, step, None, status, ss)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            body()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            body()
        graphs[name] = (g, (logits, cur, live, n_new, max_new, force_at, pos, ctx, step, status, ss, master, cur0))   # keep the buffers alive
    return graphs


def time_kernels(G):
    graphs = kernel_graphs(G)
    for g, _ in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    us = {k: [] for k in graphs}
    for rep in range(a.reps):
        for name, (g, _) in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / a.launches)
    base = float(np.median(us["refresh only"]))
    out = {}
    for name, v in us.items():
        out[name] = dict(us=round(float(np.median(v)) - (base if name != "refresh only" else 0.0), 2), raw_us=round(float(np.median(v)), 2),
                         spread_us=round(float(max(v) - min(v)), 2))
        emit(dict(part="kernel", G=G, variant=name, launches_per_sample=a.launches, reps=a.reps, **out[name]))
    return out


def time_step():
    import bench
    G = bench.BATCH = 16
    _, agent, _ = bench.build_models(dev, torch.float16, need=("llm",), max_cache_len=1024)
    tok, rng = bench.BenchTokenizer(), np.random.default_rng(0)
    reqs = [dict(input_ids=[[1] + rng.integers(3, 31000, size=int(rng.integers(16, 49))).tolist()], max_new_tokens=128) for _ in range(G)]
    queues = {"all greedy": reqs,
              "half sampled": [dict(r, do_sample=True, seed=100 + i) if i % 2 else r for i, r in enumerate(reqs)]}
    ms = {k: [] for k in queues}
    for rep in range(-1, a.reps):                                      # rep -1: warm-up (graph capture) of each queue
        for name, q in queues.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = agent.generate_inflight(tok, q, eos_token_id=None)
            torch.cuda.synchronize()
            assert all(len(o["generate_ids"]) == 128 for o in out)
            if rep >= 0:
                ms[name].append((time.perf_counter() - t0) * 1e3 / 127)
    out = {}
    for name, v in ms.items():
        out[name] = dict(ms_per_step=round(float(np.median(v)), 4), spread_ms=round(float(max(v) - min(v)), 4))
        emit(dict(part="step", slots=G, queue=name, decode_steps=127, reps=a.reps, **out[name]))
    return out


kern = {G: time_kernels(G) for G in (16, 32)}
step = time_step() if a.step else None

if a.out:
    md = ["# Device-side sampling against the greedy kernel (tools/bench_sample_next.py)", "",
          f"V = {V}, ld = {LD}; {a.launches} launches per captured graph, {a.reps} alternated repeats; us per launch = median, less the "
          "refresh-only graph (logits copy + cur restore); spread = max - min over the repeats.", "",
          "| G | kernel | us per launch | spread us | with the refresh, us |", "|---|---|---|---|---|"]
    for G, res in kern.items():
        for name, r in res.items():
            md.append(f"| {G} | {name} | {r['us']:.2f} | {r['spread_us']:.2f} | {r['raw_us']:.2f} |")
    md.append("")
    if step is not None:
        g16 = kern[16]
        step_us = step["all greedy"]["ms_per_step"] * 1e3
        md += ["## 16-slot token step (13B dimensions, fp16, precise mode, 16 requests of budget 128, generate_inflight)", "",
               "| queue | ms per token step | spread ms |", "|---|---|---|"]
        md += [f"| {name} | {r['ms_per_step']:.4f} | {r['spread_ms']:.4f} |" for name, r in step.items()]
        md.append("")
        for name in list(VARIANTS)[2:]:
            d = g16[name]["us"] - g16["greedy"]["us"]
            md.append(f"Kernel difference at G = 16, {name} - greedy: {d:.2f} us = {100 * d / step_us:.3f} % of the all-greedy token step.")
        md.append("")
    else:
        md += ["Token step: not measured in this run (`--step`).", ""]
    md += ["## Raw lines", "", "```"] + LINES + ["```", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(md))
