"""What LlamaForCausalLM(weight_residency="tiles") saves and costs at 13B dims (synthetic weights, fp16, precise mode), and the rate of
the kernel behind it (sx_dequant_tiles). ONE process, everything that is compared is alternated --reps times.

Kernel section (--kernel, on by default): per format and projection shape (qkv 15360 x 5120, o 5120 x 5120 in 20-row tiles, gate|up
27648 x 5120, down 5120 x 13824 in 20-row tiles) the time of one ops.dequant_tiles launch against torch.Tensor.clone() of the same
[N, K] fp16 matrix: both rotate over enough sources and destinations for 1 GB of output, so no launch finds its lines in the last-level
cache; --launches launches per turn between two device events; us per launch (median over the turns), spread, output GB/s.

Model section (per format in --formats): the default-residency model D and the tiles model T from the same state dict —
  bytes held: torch.cuda.memory_allocated around _pack against memory_footprint()["total"],
  one prefill pass of 8 / 64 / 512 / 2048 rows (one sequence from cache position 0, no logits), D and T alternated,
  the graph-replayed token step of both (expected equal: the same kernels run).
The byte model the prefill delta is held against (nobody had measured it): MXFP4 reads ~0.17 GB and writes ~0.64 GB per layer, ~0.2 ms
at 4 TB/s, ~8 ms per 40-layer pass at every row count.

--out FILE replaces the section between the "measured:begin" / "measured:end" marker lines of FILE (appends one if FILE has none,
creates FILE if missing; rewritten after every section, so a run cut short leaves what it measured). --jsonl FILE receives every raw line.

    python tools/bench_weight_residency.py --out profiles/weight_residency.md
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seedx_amd import ops, quant
from seedx_amd import synthetic as syn
from seedx_amd.llama import LlamaForCausalLM

ap = argparse.ArgumentParser()
ap.add_argument("--formats", nargs="*", default=["mxfp4", "fp8_e4m3"])
ap.add_argument("--rows", type=int, nargs="*", default=[8, 64, 512, 2048])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--G", type=int, default=4)
ap.add_argument("--steps", type=int, default=32, help="token-step replays per turn")
ap.add_argument("--layers", type=int, default=None, help="fewer decoder layers than 40 (quick looks; the tables say so)")
ap.add_argument("--kernel", type=int, default=1, help="0: skip the kernel section")
ap.add_argument("--launches", type=int, default=40)
ap.add_argument("--out", default=None)
ap.add_argument("--jsonl", default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "tools/bench_weight_residency.py measures on the GPU: there is no CPU fall-back"
dev, dt = torch.device("cuda:0"), torch.float16
cfg = dict(syn.FULL_LLM)
if a.layers:
    cfg["num_hidden_layers"] = a.layers
H, L, I = cfg["hidden_size"], cfg["num_hidden_layers"], cfg["intermediate_size"]
LINES, KERNEL, HELD, PREFILL, STEP = [], [], [], [], []
if a.jsonl:
    os.makedirs(os.path.dirname(os.path.abspath(a.jsonl)), exist_ok=True)
    open(a.jsonl, "w").close()


def emit(d):
    LINES.append(json.dumps(d))
    print(LINES[-1], flush=True)
    if a.jsonl:
        with open(a.jsonl, "a") as f:
            f.write(LINES[-1] + "\n")


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n          # ms per call


def write_out():
    if not a.out:
        return
    BEGIN, END = "<!-- measured:begin (tools/bench_weight_residency.py --out rewrites this section) -->", "<!-- measured:end -->"
    md = [BEGIN, "## Bytes held (measured on one MI355X)", ""]
    if HELD:
        md += [f"13B dims ({L} layers), fp16, {a.G} sequences; allocator = torch.cuda.memory_allocated after _pack minus before (it also holds the norm "
               "weights, RoPE tables, the split-K workspace and the loop state, which memory_footprint() does not price).", "",
               "| format | residency | allocator GB | memory_footprint() total GB | weights GB | prefill scratch GB | decode tiles GB | KV cache GB |",
               "|---|---|---|---|---|---|---|---|"]
        for r in HELD:
            md.append(f"| {r['format']} | {r['residency']} | {r['allocated_gb']:.3f} | {r['footprint_gb']:.3f} | {r['weights_gb']:.3f} | "
                      f"{r['scratch_gb']:.3f} | {r['tiles_gb']:.3f} | {r['kv_gb']:.3f} |")
    else:
        md += ["**Not measured.**"]
    md += ["", "## Prefill pass (measured on one MI355X)", ""]
    if PREFILL:
        md += [f"One pass of T rows of one sequence from cache position 0, no logits, {L} layers; default residency (the parent's code path) and "
               f"'tiles' alternated {a.reps} times in one process; ms per pass, median (spread = max - min). The byte model predicts "
               f"about {8.0 * L / 40:.1f} ms per pass for MXFP4 at every T.", "",
               "| format | rows | default ms | spread | tiles ms | spread | delta ms | tiles / default |", "|---|---|---|---|---|---|---|---|"]
        for r in PREFILL:
            md.append(f"| {r['format']} | {r['rows']} | {r['default_ms']:.3f} | {r['default_spread']:.3f} | {r['tiles_ms']:.3f} | {r['tiles_spread']:.3f} | "
                      f"{r['tiles_ms'] - r['default_ms']:+.3f} | {r['tiles_ms'] / r['default_ms']:.3f} |")
    else:
        md += ["**Not measured.**"]
    md += ["", "## Token step (measured on one MI355X)", ""]
    if STEP:
        md += [f"Graph-replayed token step, {a.G} sequences, {a.steps} replays per turn, {a.reps} alternated turns; ms per step, median (spread).", "",
               "| format | default ms | spread | tiles ms | spread |", "|---|---|---|---|---|"]
        for r in STEP:
            md.append(f"| {r['format']} | {r['default_ms']:.4f} | {r['default_spread']:.4f} | {r['tiles_ms']:.4f} | {r['tiles_spread']:.4f} |")
    else:
        md += ["**Not measured.**"]
    md += ["", "## sx_dequant_tiles against clone() (measured on one MI355X)", ""]
    if KERNEL:
        md += [f"fp16 output, {a.launches} launches per turn, {a.reps} alternated turns, sources and destinations rotated over 1 GB of output; us per "
               "launch, median (spread); GB/s over the output bytes. Target: at most 1.10 x clone().", "",
               "| format | projection | N x K | tiles | dequant us | spread | out GB/s | clone us | spread | out GB/s | dequant / clone |",
               "|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in KERNEL:
            md.append(f"| {r['format']} | {r['projection']} | {r['N']} x {r['K']} | {r['layout']} | {r['dequant_us']:.1f} | {r['dequant_spread']:.1f} | "
                      f"{r['out_mb'] / r['dequant_us'] * 1e3:.0f} | {r['clone_us']:.1f} | {r['clone_spread']:.1f} | {r['out_mb'] / r['clone_us'] * 1e3:.0f} | "
                      f"{r['dequant_us'] / r['clone_us']:.3f} |")
    else:
        md += ["**Not measured.**"]
    md += ["", "### Raw lines", "", "```"] + LINES + ["```", END]
    section = "\n".join(md)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    old = open(a.out).read() if os.path.exists(a.out) else "# Weight residency 'tiles': prefill from FP8 / MXFP4 tiles (tools/bench_weight_residency.py)\n"
    i, j = old.find("<!-- measured:begin"), old.find(END)
    new = old[:i] + section + old[j + len(END):] if 0 <= i < j else old.rstrip("\n") + "\n\n" + section + "\n"
    with open(a.out, "w") as f:
        f.write(new)


# ---- the kernel against clone() ---------------------------------------------------------------------------------------------------------
def kernel_section():
    shapes = [("qkv", 3 * H, H, False), ("o", H, H, True), ("gate-up", 2 * I, H, False), ("down", H, I, True)]
    g = torch.Generator(device=dev).manual_seed(3)
    for fmt in a.formats:
        for pname, N, K, t20 in shapes:
            w = (torch.randn(N, K, generator=g, device=dev) * 0.02).to(dt)
            if fmt == "mxfp4":
                c, s = quant.quantize_blocks_mxfp4(w)
                pair = ((ops.pack_decode_tiles20_fp4 if t20 else ops.pack_decode_tiles_fp4)(c), ops.pack_block_scales_fp4(s, rows=20 if t20 else 16))
                key, wq = "w_fp4", quant.dequantize_blocks_mxfp4(c, s, dt)
            else:
                c, s = quant.quantize_rows(w)
                pair = ((ops.pack_decode_tiles20_fp8 if t20 else ops.pack_decode_tiles_fp8)(c), s)
                key, wq = "w_fp8", quant.dequantize_rows(c, s, dt)
            del w, c
            out_bytes = N * K * 2
            n = max(2, math.ceil(1e9 / out_bytes))
            pairs = [pair] + [(pair[0].clone(), pair[1].clone()) for _ in range(n - 1)]
            srcs = [wq] + [wq.clone() for _ in range(n - 1)]
            outs = [torch.empty(N * K, dtype=dt, device=dev) for _ in range(n)]
            ring = [None] * n
            assert torch.equal(ops.dequant_tiles(dtype=dt, out=outs[0], **{key: pairs[0]}), wq)       # what is timed is the exact kernel

            def dq(i):
                ops.dequant_tiles(dtype=dt, out=outs[i % n], **{key: pairs[i % n]})

            def cl(i):
                ring[i % n] = None                    # the allocator hands the freed block back: n destinations rotate, as for dq
                ring[i % n] = srcs[i % n].clone()
            for f in (dq, cl):                        # warm-up: every destination once
                timed(f, n)
            t = {"dq": [], "cl": []}
            for rep in range(a.reps):
                t["dq"].append(timed(dq, a.launches) * 1e3)
                t["cl"].append(timed(cl, a.launches) * 1e3)
            row = dict(format=fmt, projection=pname, N=N, K=K, layout="20-row" if t20 else "16-row", out_mb=round(out_bytes / 1e6, 2),
                       dequant_us=round(float(np.median(t["dq"])), 2), dequant_spread=round(max(t["dq"]) - min(t["dq"]), 2),
                       clone_us=round(float(np.median(t["cl"])), 2), clone_spread=round(max(t["cl"]) - min(t["cl"]), 2), copies=n,
                       launches_per_turn=a.launches, reps=a.reps)
            emit(row)
            KERNEL.append(row)
            del pairs, srcs, outs, ring, pair, wq
            torch.cuda.empty_cache()


if a.kernel:
    kernel_section()
    write_out()

# ---- the two residencies of one model -----------------------------------------------------------------------------------------------------
sd = syn.llama_state_dict(cfg, dev, dt) if a.formats else None
TMAX = max(a.rows + [256]) + a.steps + 8


def build(fmt, res):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(dev)
    llm = LlamaForCausalLM(dict(cfg), max_cache_len=TMAX, max_batch=a.G, weight_format=fmt, weight_residency=res)
    llm.load_state_dict(dict(sd))
    llm.to(dev, dt)
    llm._pack()
    torch.cuda.synchronize()
    fp = llm.memory_footprint()
    row = dict(format=fmt, residency=res or "default", layers=L, G=a.G, Tmax=TMAX, allocated_gb=round((torch.cuda.memory_allocated(dev) - base) / 1e9, 4),
               footprint_gb=round(fp["total"] / 1e9, 4), weights_gb=round(fp["weights"] / 1e9, 4), scratch_gb=round(fp.get("prefill_scratch", 0) / 1e9, 4),
               tiles_gb=round(fp["decode_tiles"] / 1e9, 4), kv_gb=round(fp["kv_cache"] / 1e9, 4))
    emit(row)
    HELD.append(row)
    return llm


def prefill_pass(llm, x):
    llm.set_position(0, 0)
    llm.forward_embeds_batch([x], [0], need_logits=False)


class Stepper:
    def __init__(self, llm):
        self.llm, self.P = llm, llm._pack()
        g = torch.Generator(device=dev).manual_seed(1)
        llm.reset()
        llm.forward_embeds_batch([torch.randn(256, H, generator=g, device=dev) * 0.5 for _ in range(a.G)], list(range(a.G)), need_logits=False)
        self.img = torch.arange(31000, 31066, dtype=torch.int32, device=dev)
        self.ids = torch.full((a.G, a.steps + 2), -1, dtype=torch.int32, device=dev)
        self.hid = torch.zeros((a.G, a.steps + 2, H), device=dev)
        self.rewind()
        llm.decode_step(self.img, self.ids, self.hid, use_graph=True)          # warm-up + capture + first replay
        torch.cuda.synchronize()

    def rewind(self):
        P = self.P
        P["pos"].fill_(256)
        P["ctx"].fill_(257)
        P["step"].zero_()
        P["cur"].copy_(torch.arange(20, 20 + a.G, dtype=torch.int32, device=dev))

    def turn(self):
        self.rewind()
        return timed(lambda i: self.llm.decode_step(self.img, self.ids, self.hid, use_graph=True), a.steps)


for fmt in a.formats:
    models = {"default": build(fmt, None), "tiles": build(fmt, "tiles")}
    write_out()
    g = torch.Generator(device=dev).manual_seed(2)
    for T in a.rows:
        x = torch.randn(T, H, generator=g, device=dev) * 0.5
        n = max(1, min(8, 512 // T))                  # passes per turn: enough work per timing window at the small sizes
        t = {k: [] for k in models}
        for k, m in models.items():                   # warm-up: every shape once per model
            prefill_pass(m, x)
        for rep in range(a.reps):
            for k, m in models.items():
                t[k].append(timed(lambda i, m=m: prefill_pass(m, x), n))
        row = dict(format=fmt, rows=T, layers=L, passes_per_turn=n, reps=a.reps,
                   default_ms=round(float(np.median(t["default"])), 4), default_spread=round(max(t["default"]) - min(t["default"]), 4),
                   tiles_ms=round(float(np.median(t["tiles"])), 4), tiles_spread=round(max(t["tiles"]) - min(t["tiles"]), 4))
        emit(row)
        PREFILL.append(row)
        write_out()
    steppers = {k: Stepper(m) for k, m in models.items()}
    t = {k: [] for k in models}
    for rep in range(a.reps):
        for k, s in steppers.items():
            t[k].append(s.turn())
    row = dict(format=fmt, G=a.G, layers=L, context=256, steps_per_turn=a.steps, reps=a.reps,
               default_ms=round(float(np.median(t["default"])), 4), default_spread=round(max(t["default"]) - min(t["default"]), 4),
               tiles_ms=round(float(np.median(t["tiles"])), 4), tiles_spread=round(max(t["tiles"]) - min(t["tiles"]), 4))
    emit(row)
    STEP.append(row)
    del steppers, models
    torch.cuda.empty_cache()
    write_out()
