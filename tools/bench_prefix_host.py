"""Host-memory tier of the prefix cache (agent.prefix_host_bytes, ops.kv_rows_copy / sx_kv_rows_copy, kvstore.py) on 13B dimensions.
Three parts, every shape from the flags:

  pack    : ops.kv_rows_copy, rows [0, p) of one slot to a staging buffer and back, at the 13B cache dims (L 40, 40 heads, head_dim 128,
            --tmax rows) for p in --rows, in the mixed (fp32 K + 16-bit V), fp32 and FP8 (codes + row scales) formats, against one torch
            ``index_select`` (gather) / slice ``copy_`` (scatter) per cache tensor over the same bytes: same process, alternated --reps
            times after a warm-up, device events around --inner calls each. GB/s = bytes moved (read once, written once: 2 x) / time.
  copy    : the same bytes between the staging buffer and ONE pinned host buffer, device to host and host to device, device events.
  restore : on the model below, a restore of p rows (pinned host -> staging -> unpack into the slot) against a prefill pass of the same p
            rows (llm.forward_embeds_batch: what a request pays without the tier), alternated; the smallest p from which the restore wins
            at every larger measured p, rounded up to a multiple of 8, is what ``agent.prefix_host_min_tokens`` should default to.

Without a GPU nothing is timed and every table reads "not measured". Prints one JSON line per run; --out writes markdown.

    python tools/bench_prefix_host.py --out profiles/prefix_host.md
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seedx_amd.seed_x import ContinuousLVLM

ap = argparse.ArgumentParser()
ap.add_argument("--parts", default="pack,copy,restore")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--rows", default="64,256,1024,2048")
ap.add_argument("--tmax", type=int, default=2048)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--layers", type=int, default=40)
ap.add_argument("--slots", type=int, default=2)
ap.add_argument("--cross-rows", default="8,16,32,64,256,1024,2048")
ap.add_argument("--seed", type=int, default=0)
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
pack_rows, copy_rows, cross = [], [], None
if GPU:
    import torch

    from seedx_amd import ops
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

    def cell(v, nbytes, factor):
        med = float(np.median(v))
        return dict(us=round(med * 1e3, 2), spread_us=round((max(v) - min(v)) * 1e3, 2), gbps=round(factor * nbytes / med / 1e6, 1))

    if parts & {"pack", "copy"}:
        L, nh, hd, G, T = 40, 40, 128, 2, a.tmax
        formats = {"mixed (fp32 K + fp16 V)": [(torch.float32, hd), (torch.float16, hd)],
                   "fp32 (K and V)": [(torch.float32, hd), (torch.float32, hd)],
                   "fp8_e4m3 (codes + fp32 row scales)": [(torch.uint8, hd), (torch.uint8, hd), (torch.float32, 0), (torch.float32, 0)]}
        for name, spec in formats.items():
            caches = [torch.zeros((L, G, nh, T) + ((w,) if w else ()), dtype=dt, device=dev) for dt, w in spec]
            for t in caches:
                t[:, 0].view(torch.uint8).random_(0, 120)              # (bytes below 0x78: no NaN pattern in any of the formats)
            for p in [int(v) for v in a.rows.split(",") if int(v) <= T]:
                nbytes = ops.kv_rows_bytes(caches, p)
                staging = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                rows = torch.arange(p, device=dev)
                parked = [torch.empty_like(t[:, 0, :, :p]) for t in caches]          # the torch arm's linear buffers

                def pack():
                    ops.kv_rows_copy(caches, [(0, p, 0)], staging, 0)

                def unpack():
                    ops.kv_rows_copy(caches, [(1, p, 0)], staging, 1)

                def gather():
                    for t, b in zip(caches, parked):
                        torch.index_select(t[:, 0], 2, rows, out=b)

                def scatter():
                    for t, b in zip(caches, parked):
                        t[:, 1, :, :p].copy_(b)
                if "pack" in parts:
                    ms = alternate({"pack": pack, "index_select": gather, "unpack": unpack, "copy_": scatter}, a.inner)
                    assert all(torch.equal(t[:, 1, :, :p], t[:, 0, :, :p]) for t in caches)
                    r = dict(part="pack", format=name, rows=p, bytes=nbytes, **{k: cell(v, nbytes, 2) for k, v in ms.items()})
                    pack_rows.append(r)
                    emit(r)
                if "copy" in parts:
                    host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
                    ms = alternate({"d2h": lambda: host.copy_(staging, non_blocking=True),
                                    "h2d": lambda: staging.copy_(host, non_blocking=True)}, max(2, a.inner // 2))
                    r = dict(part="copy", format=name, rows=p, bytes=nbytes, **{k: cell(v, nbytes, 1) for k, v in ms.items()})
                    copy_rows.append(r)
                    emit(r)
                    del host
                del staging, parked
            del caches
            torch.cuda.empty_cache()

    if "restore" in parts:
        from seedx_amd import synthetic as syn
        from seedx_amd.llama import LlamaForCausalLM
        cfg = dict(syn.FULL_LLM, num_hidden_layers=a.layers)
        llm = LlamaForCausalLM(cfg, max_cache_len=a.tmax + 64, max_batch=a.slots)
        llm.load_state_dict(syn.llama_state_dict(cfg, dev, torch.float16))
        llm.to(dev, torch.float16)
        P = llm._pack()
        torch.cuda.empty_cache()
        ps = [int(v) for v in a.cross_rows.split(",") if int(v) <= a.tmax]
        x = torch.randn(max(ps), llm.H, generator=torch.Generator().manual_seed(a.seed)).to(dev) * 0.5
        llm.reset()
        llm.forward_embeds_batch([x], [0])                             # slot 0 holds the rows: what gets spilled
        rows = []
        for p in ps:
            nbytes = ops.kv_rows_bytes(P, p)
            staging = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            ops.kv_rows_copy(P, [(0, p, 0)], staging, 0)
            host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
            host.copy_(staging)

            def prefill():
                llm.set_position(1, 0)
                llm.forward_embeds_batch([x[:p]], [1])

            def restore():
                staging.copy_(host)                                    # as the engine does it: synchronous, on the main stream
                ops.kv_rows_copy(P, [(1, p, 0)], staging, 1)
            ms = alternate({"prefill": prefill, "restore": restore}, 3)
            r = dict(part="restore", layers=a.layers, rows=p, bytes=nbytes, kv_row_bytes=llm.kv_row_bytes,
                     prefill_ms=round(float(np.median(ms["prefill"])), 4), prefill_spread_ms=round(max(ms["prefill"]) - min(ms["prefill"]), 4),
                     restore_ms=round(float(np.median(ms["restore"])), 4), restore_spread_ms=round(max(ms["restore"]) - min(ms["restore"]), 4))
            r["restore_wins"] = max(ms["restore"]) < min(ms["prefill"])      # every repeat of the restore below every repeat of the prefill
            rows.append(r)
            emit(r)
            del staging, host
        wins = [r["rows"] for i, r in enumerate(rows) if all(q["restore_wins"] for q in rows[i:])]
        cross = dict(rows=rows, smallest_winning_rows=wins[0] if wins else None,
                     default=(wins[0] + 7) // 8 * 8 if wins else None)
        emit(dict(part="restore", summary=True, smallest_winning_rows=cross["smallest_winning_rows"], rounded_up_to_8=cross["default"]))

if a.out:
    md = ["# Host-memory tier of the prefix cache (tools/bench_prefix_host.py)", ""]
    if not GPU:
        md += ["**Not measured.** This file was written without a GPU. `python tools/bench_prefix_host.py --out profiles/prefix_host.md` on an "
               "MI355X fills in the pack / unpack bandwidth, the pinned-memory copies and the restore / prefill crossover. Until then "
               f"`agent.prefix_host_min_tokens` defaults to `prefix_min_tokens`' value, {ContinuousLVLM.PREFIX_HOST_MIN_TOKENS}.", ""]
    md += ["## Pack and unpack: `ops.kv_rows_copy` (one `sx_kv_rows_copy` launch for all cache tensors) against one torch call per cache "
           "tensor", ""]
    if pack_rows:
        md += [f"13B cache dims (L 40, 40 heads, head_dim 128, Tmax {a.tmax}), rows [0, p) of one slot, {a.reps} alternated repeats of {a.inner} "
               "calls between device events; GB/s counts every byte read and written. Torch arms: `index_select` of the rows into a linear "
               "buffer (pack) and a slice `copy_` back (unpack), one call per cache tensor.", "",
               "| format | rows p | bytes | pack µs | spread µs | GB/s | index_select µs | spread µs | GB/s | unpack µs | spread µs | GB/s | "
               "copy_ µs | spread µs | GB/s |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in pack_rows:
            md.append(f"| {r['format']} | {r['rows']} | {r['bytes']} | " + " | ".join(
                f"{r[k]['us']} | {r[k]['spread_us']} | {r[k]['gbps']}" for k in ("pack", "index_select", "unpack", "copy_")) + " |")
        lost = [f"{k} in {r['format']} at p = {r['rows']} ({r[k]['us']} against {r[t]['us']} µs)" for r in pack_rows
                for k, t in (("pack", "index_select"), ("unpack", "copy_")) if r[k]["us"] >= r[t]["us"]]
        md += ["", ("`ops.kv_rows_copy` loses to the torch arm in: " + "; ".join(lost) + ". It wins in the other cells." if lost else
                    "`ops.kv_rows_copy` beats the torch arm in every cell.")]
    else:
        md += [f"Rows {a.rows} in the mixed, fp32 and FP8 formats: {NM}."]
    md += ["", "## Copies through pinned host memory", ""]
    if copy_rows:
        md += ["The staging buffer of the rows above to ONE pinned host buffer and back (`copy_(non_blocking=True)` between device events).", "",
               "| format | rows p | bytes | device to host µs | spread µs | GB/s | host to device µs | spread µs | GB/s |", "|---|---|---|---|---|---|---|---|---|"]
        md += [f"| {r['format']} | {r['rows']} | {r['bytes']} | {r['d2h']['us']} | {r['d2h']['spread_us']} | {r['d2h']['gbps']} | {r['h2d']['us']} | "
               f"{r['h2d']['spread_us']} | {r['h2d']['gbps']} |" for r in copy_rows]
    else:
        md += [f"{NM}."]
    md += ["", "## Restore against prefill: the crossover for `prefix_host_min_tokens`", ""]
    if cross:
        md += [f"{a.layers} layers of 13B dims, synthetic weights, fp16, precise mode (mixed cache), {a.slots} slots: a restore of p rows (pinned host "
               "to staging, then unpack into the slot) against a prefill pass of the same p rows (`llm.forward_embeds_batch`), "
               f"{a.reps} alternated repeats of 3 calls. The restore wins at p when every repeat of its side is below every repeat of the other.", "",
               "| rows p | bytes | prefill ms | spread ms | restore ms | spread ms | restore wins |", "|---|---|---|---|---|---|---|"]
        md += [f"| {r['rows']} | {r['bytes']} | {r['prefill_ms']} | {r['prefill_spread_ms']} | {r['restore_ms']} | {r['restore_spread_ms']} | "
               f"{'yes' if r['restore_wins'] else 'no'} |" for r in cross["rows"]]
        md += ["", f"Smallest p from which the restore wins at every measured p above it: **{cross['smallest_winning_rows']}**; rounded up to a "
               f"multiple of 8: **{cross['default']}**. The engine's default of `prefix_host_min_tokens` is "
               f"{ContinuousLVLM.PREFIX_HOST_MIN_TOKENS}. The table times one request alone: a restore also saves the other slots the wait for a "
               "longer prefill pass, and a spill costs a pack and a device-to-host copy on a side stream; neither is in this table."]
    else:
        md += [f"{NM}."]
    md += ["", "## Raw lines", "", "```"] + LINES + ["```", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(md))
