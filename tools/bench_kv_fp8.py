"""The graph-replayed token step of the 13B-dimension LLM with the default (mixed: k fp32, v fp16) KV cache against the FP8 (e4m3) KV
cache (LlamaForCausalLM(kv_format="fp8_e4m3")): synthetic weights, fp16, precise mode, at (sequences, context) in --configs
(default 16x256 32x256 16x1024 4x1536), with 16-bit decode tiles and with FP8 decode tiles (--tiles).

ONE process: per (config, tile format) the two models are built from the same state dict, their caches are FILLED directly up to the
context (random values / random non-NaN codes and power-of-two row scales: a token step's time depends on the bytes it reads, and a
13B prefill of 16 x 1024 tokens would only spend the time), each captures one token step, then the two are ALTERNATED --reps times,
each turn timing --steps replays between two device events from the same cache position. Reported per model: ms per step (median over
the turns), spread (max - min), KV bytes and decode-tile bytes per step, and TB/s over their sum. No speed threshold: the table says
what the mode gains, or that it gains nothing.

--out FILE replaces the section between the "measured:begin" / "measured:end" marker lines of FILE (appends one if FILE has none,
creates FILE if missing) after every finished config: the static sections of profiles/fp8_kv.md stay.

    python tools/bench_kv_fp8.py --out profiles/fp8_kv.md
    rocprofv3 --kernel-trace --stats -d /tmp/kv8 -- python tools/bench_kv_fp8.py --configs 16x256 --tiles 16bit --only fp8 --reps 1 --steps 8
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seedx_amd import synthetic as syn
from seedx_amd.llama import LlamaForCausalLM

ap = argparse.ArgumentParser()
ap.add_argument("--configs", nargs="+", default=["16x256", "32x256", "16x1024", "4x1536"], help="SEQUENCESxCONTEXT")
ap.add_argument("--tiles", nargs="+", choices=["16bit", "fp8"], default=["16bit", "fp8"], help="decode-tile formats to run")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--layers", type=int, default=None, help="fewer decoder layers than 40 (quick looks; the table says so)")
ap.add_argument("--only", choices=["default", "fp8"], default=None, help="one cache format only (for a profiler run)")
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev, dt = torch.device("cuda:0"), torch.float16
cfg = dict(syn.FULL_LLM)
if a.layers:
    cfg["num_hidden_layers"] = a.layers
sd = syn.llama_state_dict(cfg, dev, dt)
H, L = cfg["hidden_size"], cfg["num_hidden_layers"]
LINES, ROWS = [], []
BEGIN, END = "<!-- measured:begin (tools/bench_kv_fp8.py --out rewrites this section) -->", "<!-- measured:end -->"


def emit(d):
    LINES.append(json.dumps(d))
    print(LINES[-1], flush=True)


class Stepper:
    def __init__(self, G, context, tiles, kv_format):
        self.G, self.context = G, context
        llm = self.llm = LlamaForCausalLM(dict(cfg), max_cache_len=context + a.steps + 8, max_batch=G,
                                          weight_format="fp8_e4m3" if tiles == "fp8" else None, kv_format=kv_format)
        llm.load_state_dict(dict(sd))
        llm.to(dev, dt)
        P = self.P = llm._pack()
        g = torch.Generator(device=dev).manual_seed(1)
        for li in range(L):                           # fill the cache instead of prefilling (module docstring), layer by layer (memory)
            if kv_format == "fp8_e4m3":
                for c, s in ((P["kc"], P["ks"]), (P["vc"], P["vs"])):
                    r = torch.randint(0, 256, c[li].shape, dtype=torch.uint8, device=dev, generator=g)
                    c[li].copy_(torch.where((r & 0x7f) == 0x7f, r & 0xf0, r))                  # no NaN code
                    s[li].copy_(torch.exp2(torch.randint(-9, -6, s[li].shape, device=dev, generator=g).float()))   # |k|, |v| up to ~ 3
            else:
                P["kc"][li].normal_(generator=g)
                P["vc"][li].copy_(torch.randn(P["vc"][li].shape, device=dev, generator=g))
        self.img = torch.arange(31000, 31066, dtype=torch.int32, device=dev)
        self.ids = torch.full((G, a.steps + 2), -1, dtype=torch.int32, device=dev)
        self.hid = torch.zeros((G, a.steps + 2, H), device=dev)
        self.rewind()
        llm.decode_step(self.img, self.ids, self.hid, use_graph=True)          # warm-up + capture + first replay
        torch.cuda.synchronize()
        fp = llm.memory_footprint()
        self.tile_bytes = fp["decode_tiles"]
        per_token = fp["kv_cache"] // (G * llm.Tmax)                            # bytes per cached token and sequence, all layers and heads
        self.kv_bytes = G * (context + a.steps // 2) * per_token
        self.kv_held = fp["kv_cache"]

    def rewind(self):
        P = self.P
        P["pos"].fill_(self.context)
        P["ctx"].fill_(self.context + 1)
        P["step"].zero_()
        P["cur"].copy_(torch.arange(20, 20 + self.G, dtype=torch.int32, device=dev))

    def turn(self):
        self.rewind()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.steps):
            self.llm.decode_step(self.img, self.ids, self.hid, use_graph=True)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps


def write_out():
    if not a.out:
        return
    md = [BEGIN, "## Step times (measured on one MI355X)", "",
          f"13B dims ({L} layers), fp16, precise mode, {a.steps} replays per turn, {a.reps} alternated turns per model, the two cache formats of a "
          "row pair in one process, caches filled with random values up to the context. Bytes per step = the KV cache read at the measured "
          "position + the decode tiles (+ row scales, + the 16-bit lm_head tiles); TB/s is over their sum. Rows this run did not cover are "
          "absent: **Not measured**.", "",
          "| sequences | context | decode tiles | KV cache | ms / step (median) | spread ms (max - min) | KV GB / step | tile GB / step | TB/s | vs default |",
          "|---|---|---|---|---|---|---|---|---|---|"]
    for r in ROWS:
        md.append(f"| {r['G']} | {r['context']} | {r['tiles']} | {r['kv']} | {r['ms_per_step']:.3f} | {r['spread_ms']:.3f} | {r['kv_gb']:.2f} | "
                  f"{r['tile_gb']:.2f} | {r['tb_per_s']:.2f} | {r.get('vs_default', '')} |")
    md += ["", "### Raw lines", "", "```"] + LINES + ["```", END]
    section = "\n".join(md)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    old = open(a.out).read() if os.path.exists(a.out) else "# FP8 (e4m3) KV cache vs the default mixed cache (tools/bench_kv_fp8.py)\n"
    i, j = old.find("<!-- measured:begin"), old.find(END)
    new = old[:i] + section + old[j + len(END):] if 0 <= i < j else old.rstrip("\n") + "\n\n" + section + "\n"
    with open(a.out, "w") as f:
        f.write(new)


for tiles in a.tiles:
    for c in a.configs:
        G, context = (int(x) for x in c.split("x"))
        models = {}
        for name, fmt in (("default", None), ("fp8", "fp8_e4m3")):
            if a.only in (None, name):
                models[name] = Stepper(G, context, tiles, fmt)
        times = {k: [] for k in models}
        for rep in range(a.reps):
            for k, m in models.items():
                times[k].append(m.turn())
                emit(dict(G=G, context=context, tiles=tiles, kv=k, rep=rep, ms_per_step=round(times[k][-1], 4)))
        med = {k: float(np.median(times[k])) for k in models}
        for k, m in models.items():
            row = dict(G=G, context=context, tiles=tiles, kv=k, layers=L, ms_per_step=round(med[k], 4),
                       spread_ms=round(float(max(times[k]) - min(times[k])), 4), reps=a.reps, steps_per_turn=a.steps,
                       kv_gb=round(m.kv_bytes / 1e9, 3), kv_held_gb=round(m.kv_held / 1e9, 3), tile_gb=round(m.tile_bytes / 1e9, 3),
                       tb_per_s=round((m.tile_bytes + m.kv_bytes) / med[k] / 1e9, 3), summary=True)
            if k == "fp8" and "default" in med:
                row["vs_default"] = f"{(med['fp8'] / med['default'] - 1) * 100:+.1f} %"
            emit(row)
            ROWS.append(row)
        del models
        torch.cuda.empty_cache()
        write_out()
