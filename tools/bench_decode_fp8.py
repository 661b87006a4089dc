"""The graph-replayed token step of the 13B-dimension LLM with 16-bit decode tiles against FP8 (e4m3) decode tiles
(LlamaForCausalLM(weight_format="fp8_e4m3")): synthetic weights, fp16, precise mode, G lock-step sequences for G in --G (1, 16, 32).

ONE process for all G: both models are built from the same state dict, but the FP8 model's row-major matrices are its own dequantised
copies, so the two share no weights. At 13B dims budget, on top of the 26-GB state dict, up to 26 GB of row-major weights per model plus
its decode tiles (26 GB / 13 GB), besides the KV caches. Each is prefilled with --context random embeddings per sequence and captures one
token step; then the two are ALTERNATED --reps times, each turn timing --steps replays between
two device events from the same cache position. Reported per model: ms per step (median over the turns), spread (max - min), bytes per step
(decode tiles incl. the 16-bit lm_head tiles + scales, KV cache read at the measured position) and TB/s over those bytes.

--out FILE replaces the section between the "measured:begin" / "measured:end" marker lines of FILE (appends one if FILE has none,
creates FILE if missing): the static sections of profiles/fp8_decode.md (bytes, compiler table) stay.

    python tools/bench_decode_fp8.py --out profiles/fp8_decode.md
    rocprofv3 --kernel-trace --stats -d /tmp/fp8 -- python tools/bench_decode_fp8.py --G 16 --only fp8 --reps 1 --steps 8     # kernel table
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
ap.add_argument("--G", type=int, nargs="+", default=[1, 16, 32])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--context", type=int, default=256)
ap.add_argument("--layers", type=int, default=None, help="fewer decoder layers than 40 (quick looks; the table says so)")
ap.add_argument("--only", choices=["16bit", "fp8"], default=None, help="one model only (for a profiler run)")
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev, dt = torch.device("cuda:0"), torch.float16
cfg = dict(syn.FULL_LLM)
if a.layers:
    cfg["num_hidden_layers"] = a.layers
sd = syn.llama_state_dict(cfg, dev, dt)
H, L = cfg["hidden_size"], cfg["num_hidden_layers"]
LINES = []


def emit(d):
    LINES.append(json.dumps(d))
    print(LINES[-1], flush=True)


class Stepper:
    def __init__(self, G, fmt):
        self.G, self.fmt = G, fmt
        llm = self.llm = LlamaForCausalLM(dict(cfg), max_cache_len=a.context + a.steps + 8, max_batch=G, weight_format=fmt)
        llm.load_state_dict(dict(sd))
        llm.to(dev, dt)
        P = self.P = llm._pack()
        g = torch.Generator(device=dev).manual_seed(1)
        xs = [torch.randn(a.context, H, generator=g, device=dev) * 0.5 for _ in range(G)]
        for i in range(0, G, 8):                      # prefill in groups of 8 sequences (activation memory)
            llm.forward_embeds_batch(xs[i:i + 8], list(range(i, min(G, i + 8))), need_logits=False)
        self.img = torch.arange(31000, 31066, dtype=torch.int32, device=dev)
        self.ids = torch.full((G, a.steps + 2), -1, dtype=torch.int32, device=dev)
        self.hid = torch.zeros((G, a.steps + 2, H), device=dev)
        self.rewind()
        llm.decode_step(self.img, self.ids, self.hid, use_graph=True)          # warm-up + capture + first replay
        torch.cuda.synchronize()
        fp = llm.memory_footprint()
        kv_elem = 4 + (2 if llm.kv_v16 else 4)
        self.tile_bytes = fp["decode_tiles"]
        self.kv_bytes = L * G * llm.nh_l * (a.context + a.steps // 2) * llm.hd * kv_elem

    def rewind(self):
        P = self.P
        P["pos"].fill_(a.context)
        P["ctx"].fill_(a.context + 1)
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


ROWS = []
for G in a.G:
    models = {}
    for name, fmt in (("16bit", None), ("fp8", "fp8_e4m3")):
        if a.only in (None, name):
            models[name] = Stepper(G, fmt)
    if "fp8" in models:
        emit(dict(G=G, weight_quant_report=models["fp8"].llm.weight_quant_report))
    times = {k: [] for k in models}
    for rep in range(a.reps):
        for k, m in models.items():
            times[k].append(m.turn())
            emit(dict(G=G, model=k, rep=rep, ms_per_step=round(times[k][-1], 4)))
    for k, m in models.items():
        med, spread = float(np.median(times[k])), float(max(times[k]) - min(times[k]))
        nbytes = m.tile_bytes + m.kv_bytes
        row = dict(G=G, model=k, layers=L, context=a.context, ms_per_step=round(med, 4), spread_ms=round(spread, 4), reps=a.reps,
                   steps_per_turn=a.steps, tile_gb=round(m.tile_bytes / 1e9, 3), kv_gb=round(m.kv_bytes / 1e9, 3),
                   tb_per_s=round(nbytes / med / 1e9, 3), summary=True)
        emit(row)
        ROWS.append(row)
    if len(models) == 2:
        ids = [m.ids[:, :a.steps].clone() for m in models.values()]
        emit(dict(G=G, ids_equal_fraction=round(float((ids[0] == ids[1]).float().mean()), 4),
                  note="different models (original vs quantised weights): the ids need not agree"))
    del models
    torch.cuda.empty_cache()

if a.out:
    BEGIN, END = "<!-- measured:begin (tools/bench_decode_fp8.py --out rewrites this section) -->", "<!-- measured:end -->"
    md = [BEGIN, "## Step times (measured on one MI355X)", "",
          f"13B dims ({L} layers), fp16, precise mode, {a.context}-token context, {a.steps} replays per turn, {a.reps} alternated turns per model, "
          "one process per row pair. Bytes per step = decode tiles (+ row scales, + the 16-bit lm_head tiles) + the KV cache read at the "
          "measured position; TB/s is over those bytes.", "",
          "| sequences | decode tiles | ms / step (median) | spread ms (max - min) | tile GB / step | KV GB / step | TB/s |", "|---|---|---|---|---|---|---|"]
    for r in ROWS:
        md.append(f"| {r['G']} | {r['model']} | {r['ms_per_step']:.3f} | {r['spread_ms']:.3f} | {r['tile_gb']:.2f} | {r['kv_gb']:.2f} | {r['tb_per_s']:.2f} |")
    md += ["", "### Raw lines", "", "```"] + LINES + ["```", END]
    section = "\n".join(md)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    old = open(a.out).read() if os.path.exists(a.out) else "# FP8 (e4m3) decode tiles vs 16-bit decode tiles (tools/bench_decode_fp8.py)\n"
    i, j = old.find("<!-- measured:begin"), old.find(END)
    new = old[:i] + section + old[j + len(END):] if 0 <= i < j else old.rstrip("\n") + "\n\n" + section + "\n"
    with open(a.out, "w") as f:
        f.write(new)
