"""The graph-replayed token step of the 13B-dimension LLM with 16-bit, FP8 (e4m3) and MXFP4 (e2m1, block-32 scale) decode tiles
(LlamaForCausalLM(weight_format=None | "fp8_e4m3" | "mxfp4")): synthetic weights, fp16, precise mode, G lock-step sequences for G in --G
(1, 16, 32), and the four projection shapes of a layer under the three formats.

ONE process for all G and all formats: the models are built from the same state dict, but the quantised models' row-major matrices are
their own dequantised copies, so they share no weights. At 13B dims budget, on top of the 26-GB state dict, up to 26 GB of row-major weights
per model plus its decode tiles (26 / 13 / 7 GB), besides the KV caches. Each model is prefilled with --context random embeddings per
sequence and captures one token step; then the models are ALTERNATED --reps times, each turn timing --steps replays between two device
events from the same cache position. Reported per model: ms per step (median over the turns), spread (max - min), bytes per step (decode
tiles incl. the 16-bit lm_head tiles + scales, KV cache read at the measured position) and TB/s over those bytes.

Per projection (--proj, on by default): qkv 15360 x 5120, o 5120 x 5120 (20-row tiles), gate-up 27648 x 5120 (GLU), down 5120 x 13824
(20-row tiles, split-K workspace) at 16 two-plane rows, the three formats alternated --reps times; every launch of a turn reads another
copy of the weight (enough copies for 1 GB, so no launch finds its weights in the last-level cache), --proj-launches launches per turn
as ONE captured graph replayed between two device events (launch gaps included, as in the token step). us per launch (median), spread,
weight bytes per launch and TB/s over them.

--out FILE replaces the section between the "measured:begin" / "measured:end" marker lines of FILE (appends one if FILE has none,
creates FILE if missing; written after the projection section and again after every G): the static sections of profiles/fp4_decode.md (bytes, compiler table, cost) stay. --jsonl FILE receives every
raw line as it is produced.

    python tools/bench_decode_fp4.py --out profiles/fp4_decode.md
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
from seedx_amd.llama import LlamaForCausalLM, glu_pack_rows

FORMATS = (("16bit", None), ("fp8", "fp8_e4m3"), ("fp4", "mxfp4"))
ap = argparse.ArgumentParser()
ap.add_argument("--G", type=int, nargs="*", default=[1, 16, 32])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--context", type=int, default=256)
ap.add_argument("--layers", type=int, default=None, help="fewer decoder layers than 40 (quick looks; the table says so)")
ap.add_argument("--only", choices=[n for n, _ in FORMATS], nargs="+", default=None, help="these models only (e.g. for a profiler run)")
ap.add_argument("--proj", type=int, default=1, help="0: skip the per-projection section")
ap.add_argument("--proj-launches", type=int, default=200)
ap.add_argument("--out", default=None)
ap.add_argument("--jsonl", default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "tools/bench_decode_fp4.py measures on the GPU: there is no CPU fall-back"
dev, dt = torch.device("cuda:0"), torch.float16
cfg = dict(syn.FULL_LLM)
if a.layers:
    cfg["num_hidden_layers"] = a.layers
H, L, I = cfg["hidden_size"], cfg["num_hidden_layers"], cfg["intermediate_size"]
LINES = []
if a.jsonl:
    os.makedirs(os.path.dirname(os.path.abspath(a.jsonl)), exist_ok=True)
    open(a.jsonl, "w").close()


def emit(d):
    LINES.append(json.dumps(d))
    print(LINES[-1], flush=True)
    if a.jsonl:
        with open(a.jsonl, "a") as f:
            f.write(LINES[-1] + "\n")


names = [n for n, _ in FORMATS if a.only is None or n in a.only]


# ---- per-projection times ---------------------------------------------------------------------------------------------------------------
def projection_section():
    M = 16
    shapes = [("qkv", 3 * H, H, False, False), ("o", H, H, False, True), ("gate-up", 2 * I, H, True, False), ("down", H, I, False, True)]
    rows = []
    g = torch.Generator(device=dev).manual_seed(3)
    for pname, N, K, glu, t20 in shapes:
        w = (torch.randn(N, K, generator=g, device=dev) * 0.02).to(dt)
        x = ops.split16(torch.randn(M, K, generator=g, device=dev), dt, tiled=True)
        res = None if glu else torch.randn(M, N, generator=g, device=dev)
        ws = torch.zeros(16384 + 8 * 32 * N * 4, dtype=torch.uint8, device=dev)
        kw = dict(residual=res, act="silu" if glu else None, glu=glu, out_dtype=torch.float32, workspace=ws)
        forms = {}
        if "16bit" in names:
            wp = glu_pack_rows(w[: N // 2], w[N // 2:]) if glu else w
            t = ops.pack_decode_tiles20(wp) if t20 else ops.pack_decode_tiles(wp)
            forms["16bit"] = (t.numel() * 2, lambda c, t20=t20: dict(w_tiles20=c) if t20 else dict(w_tiles=c), t)
        if "fp8" in names:
            c8, s8 = quant.quantize_rows(w)
            if glu:
                c8, s8 = glu_pack_rows(c8[: N // 2], c8[N // 2:]), glu_pack_rows(s8[: N // 2, None], s8[N // 2:, None]).reshape(-1).contiguous()
            t = (ops.pack_decode_tiles20_fp8 if t20 else ops.pack_decode_tiles_fp8)(c8)
            forms["fp8"] = (t.numel() + s8.numel() * 4, lambda c, s8=s8: dict(w_fp8=(c, s8)), t)
        if "fp4" in names:
            c4, s4 = quant.quantize_blocks_mxfp4(w)
            if glu:
                c4, s4 = glu_pack_rows(c4[: N // 2], c4[N // 2:]), glu_pack_rows(s4[: N // 2], s4[N // 2:])
            t = (ops.pack_decode_tiles20_fp4 if t20 else ops.pack_decode_tiles_fp4)(c4)
            st = ops.pack_block_scales_fp4(s4.contiguous(), rows=20 if t20 else 16)
            forms["fp4"] = (t.numel() + st.numel(), lambda c, st=st: dict(w_fp4=(c, st)), t)
        copies = {k: [v[2]] + [v[2].clone() for _ in range(max(1, math.ceil(1e9 / v[0])) - 1)] for k, v in forms.items()}
        times, graphs = {k: [] for k in forms}, {}
        for k, v in forms.items():                   # warm-up (every kernel once), then one captured chain of launches per format
            ops.gemv(x, w, **v[1](copies[k][0]), **kw)
            torch.cuda.synchronize()
            graphs[k] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[k]):
                for i in range(a.proj_launches):
                    ops.gemv(x, w, **v[1](copies[k][i % len(copies[k])]), **kw)
            graphs[k].replay()
        torch.cuda.synchronize()
        for rep in range(a.reps):
            for k in forms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graphs[k].replay()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / a.proj_launches)
        for k, v in forms.items():
            med, spread = float(np.median(times[k])), float(max(times[k]) - min(times[k]))
            row = dict(projection=pname, N=N, K=K, M=M, planes=2, layout="20-row" if t20 else "16-row", model=k, us_per_launch=round(med, 2),
                       spread_us=round(spread, 2), weight_mb=round(v[0] / 1e6, 2), copies=len(copies[k]), launches_per_turn=a.proj_launches,
                       reps=a.reps, tb_per_s=round(v[0] / med / 1e6, 3))
            emit(row)
            rows.append(row)
        del copies, forms, graphs
        torch.cuda.empty_cache()
    return rows


ROWS, PROJ = [], []


def write_out():
    if not a.out:
        return
    BEGIN, END = "<!-- measured:begin (tools/bench_decode_fp4.py --out rewrites this section) -->", "<!-- measured:end -->"
    md = [BEGIN, "## Step times (measured on one MI355X)", ""]
    if ROWS:
        md += [f"13B dims ({L} layers), fp16, precise mode, {a.context}-token context, {a.steps} replays per turn, {a.reps} alternated turns per model, "
               "the models of one row group in one process. Bytes per step = decode tiles (+ scales, + the 16-bit lm_head tiles) + the KV cache read "
               "at the measured position; TB/s is over those bytes.", "",
               "| sequences | decode tiles | ms / step (median) | spread ms (max - min) | tile GB / step | KV GB / step | TB/s |", "|---|---|---|---|---|---|---|"]
        for r in sorted(ROWS, key=lambda r: (r['G'], names.index(r['model']))):
            md.append(f"| {r['G']} | {r['model']} | {r['ms_per_step']:.3f} | {r['spread_ms']:.3f} | {r['tile_gb']:.2f} | {r['kv_gb']:.2f} | {r['tb_per_s']:.2f} |")
        want = {(G, n) for G in (1, 16, 32) for n, _ in FORMATS}
        missing = sorted(want - {(r["G"], r["model"]) for r in ROWS})
        if missing or L != 40:
            md += ["", "Not measured: " + (", ".join(f"{n} at {G} sequences" for G, n in missing) if missing else "—")
                   + (f"; the rows above are {L}-layer models, the 40-layer step is not measured" if L != 40 else "") + "."]
    else:
        md += ["**Not measured.**"]
    md += ["", "## Per-projection times (measured on one MI355X)", ""]
    if PROJ:
        md += [f"16 two-plane rows (the 16-sequence step's GEMV), {a.proj_launches} launches per turn replayed as one captured graph, each on another copy of the "
               f"weight (copies for 1 GB), {a.reps} alternated turns per format; weight bytes include the scales.", "",
               "| projection | N x K | tiles | format | us / launch (median) | spread us | weight MB | TB/s |", "|---|---|---|---|---|---|---|---|"]
        for r in PROJ:
            md.append(f"| {r['projection']} | {r['N']} x {r['K']} | {r['layout']} | {r['model']} | {r['us_per_launch']:.2f} | {r['spread_us']:.2f} | "
                      f"{r['weight_mb']:.1f} | {r['tb_per_s']:.2f} |")
    else:
        md += ["**Not measured.**"]
    md += ["", "### Raw lines", "", "```"] + LINES + ["```", END]
    section = "\n".join(md)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    old = open(a.out).read() if os.path.exists(a.out) else "# MXFP4 decode tiles vs FP8 and 16-bit decode tiles (tools/bench_decode_fp4.py)\n"
    i, j = old.find("<!-- measured:begin"), old.find(END)
    new = old[:i] + section + old[j + len(END):] if 0 <= i < j else old.rstrip("\n") + "\n\n" + section + "\n"
    with open(a.out, "w") as f:
        f.write(new)


PROJ += projection_section() if a.proj else []
write_out()

# ---- token step ---------------------------------------------------------------------------------------------------------------------------
sd = syn.llama_state_dict(cfg, dev, dt) if a.G else None


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


for G in a.G:
    models = {name: Stepper(G, fmt) for name, fmt in FORMATS if name in names}
    for name, m in models.items():
        if m.llm.weight_quant_report:
            emit(dict(G=G, model=name, weight_quant_report=m.llm.weight_quant_report))
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
    del models
    torch.cuda.empty_cache()
    write_out()          # after every row group: a run cut short leaves what it measured
