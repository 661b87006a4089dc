"""What unmerged per-request LoRA adapters cost at 13B dims (synthetic weights, fp16, precise mode, 256 keys per slot): the graph-replayed
token step without adapters, the adapter token step with 0 / half / all slots on an adapter and 1 or 4 distinct adapters, a 64-row and a
512-row prefill with and without an adapter, and the bytes of one adapter slot.

    python tools/bench_lora_serving.py --out profiles/lora_serving_measured.md          # this commit
    python tools/bench_lora_serving.py --base-only --label parent                       # in a checkout of the parent commit: the same base
                                                                                        # step and prefill through the same code, no adapters

Every variant of one model is timed in interleaved rounds in one process (--rounds turns of --steps replays each; median and min over the
turns are reported, and the spread of the base step over its turns is the run-to-run spread the other figures are read against). One JSON
line per figure.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from seedx_amd import synthetic as syn  # noqa: E402
from seedx_amd.llama import LlamaForCausalLM  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--slots", type=int, nargs="*", default=[16, 32])
ap.add_argument("--keys", type=int, default=256)
ap.add_argument("--steps", type=int, default=32, help="token-step replays per turn")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--prefill", type=int, nargs="*", default=[64, 512])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--layers", type=int, default=None, help="fewer decoder layers than 40 (quick looks; the output says so)")
ap.add_argument("--base-only", action="store_true", help="no adapters at all (also runs on a commit without the feature)")
ap.add_argument("--label", default="this commit")
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "tools/bench_lora_serving.py measures on the GPU: there is no CPU fall-back"
dev, dt = torch.device("cuda:0"), torch.float16
cfg = dict(syn.FULL_LLM)
if a.layers:
    cfg["num_hidden_layers"] = a.layers
H, L = cfg["hidden_size"], cfg["num_hidden_layers"]
N_AD, ROWS = 4, []


def emit(d):
    d = dict(label=a.label, layers=L, **d)
    ROWS.append(d)
    print(json.dumps(d), flush=True)


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n          # ms per call


sd = syn.llama_state_dict(cfg, dev, dt)
for G in a.slots:
    torch.cuda.empty_cache()
    kw = {} if a.base_only else dict(max_adapters=N_AD)
    llm = LlamaForCausalLM(dict(cfg), max_cache_len=max(a.keys, max(a.prefill)) + a.steps + 8, max_batch=G, **kw)
    llm.load_state_dict(dict(sd))
    llm.to(dev, dt)
    P = llm._pack()
    g = torch.Generator(device=dev).manual_seed(1)
    if not a.base_only:
        # synthetic adapters written straight into the preallocated tables: rank 32, every projection, gammas near 1
        T = P["lora"]
        for d_ in (T["A"], T["B"]):
            for t in d_.values():
                t.copy_((torch.randn(t.shape, generator=g, device=dev) * 0.01).to(dt))
        for k in ("ln1", "ln2", "norm"):
            T[k].mul_(1.0 + 0.05 * torch.randn(T[k].shape, generator=g, device=dev))
        T["scale"].fill_(1.0)
        llm._adapters = {f"a{i}": i for i in range(N_AD)}
        emit(dict(what="bytes per adapter slot", G=G, gb=round(llm.memory_footprint()["adapters"] / N_AD / 1e9, 4)))
    llm.reset()
    llm.forward_embeds_batch([torch.randn(a.keys, H, generator=g, device=dev) * 0.5 for _ in range(G)], list(range(G)), need_logits=False)
    img = torch.arange(31000, 31066, dtype=torch.int32, device=dev)
    ids = torch.full((G, a.steps + 2), -1, dtype=torch.int32, device=dev)
    hid = torch.zeros((G, a.steps + 2, H), device=dev)

    def rewind():
        P["pos"].fill_(a.keys)
        P["ctx"].fill_(a.keys + 1)
        P["step"].zero_()
        P["cur"].copy_(torch.arange(20, 20 + G, dtype=torch.int32, device=dev))

    # (name, slots on an adapter, distinct adapters, adapter step?)
    variants = [("base step", 0, 0, False)]
    if not a.base_only:
        variants += [(f"adapter step, {n_on} of {G} slots on an adapter, {nd} distinct", n_on, nd, True)
                     for n_on in (0, G // 2, G) for nd in (1, 4)]

    def turn(v):
        _, n_on, nd, ad = v
        if not a.base_only:
            llm.set_adapters(range(G), [f"a{i % nd}" if i < n_on else None for i in range(G)])
        rewind()
        step = (lambda: llm.decode_step(img, ids, hid, use_graph=True, adapters=ad)) if not a.base_only else \
            (lambda: llm.decode_step(img, ids, hid, use_graph=True))
        return timed(step, a.steps)
    for v in variants:          # warm-up + capture
        turn(v)
    times = {v[0]: [] for v in variants}
    for _ in range(a.rounds):   # interleaved rounds
        for v in variants:
            times[v[0]].append(turn(v))
    base_med = statistics.median(times["base step"])
    for v in variants:
        ts = times[v[0]]
        emit(dict(what="token step", G=G, keys=a.keys, variant=v[0], ms_median=round(statistics.median(ts), 4), ms_min=round(min(ts), 4),
                  ms_max=round(max(ts), 4), over_base_ms=round(statistics.median(ts) - base_med, 4)))
    if not a.base_only:
        llm.set_adapters(range(G), [None] * G)
    # prefill of one sequence from row 0
    for rows in a.prefill:
        x = torch.randn(rows, H, generator=g, device=dev) * 0.5
        pv = [("no adapter", {})] + ([] if a.base_only else [("one adapter", dict(adapters=["a0"]))])

        def pre(kw2):
            llm.set_position(0, 0)
            llm.forward_embeds_batch([x], [0], need_logits=False, **kw2)
        for _, kw2 in pv:
            pre(kw2)
        pt = {n: [] for n, _ in pv}
        for _ in range(a.rounds):
            for n, kw2 in pv:
                pt[n].append(timed(lambda: pre(kw2), a.reps))
        for n, _ in pv:
            emit(dict(what="prefill", G=G, rows=rows, variant=n, ms_median=round(statistics.median(pt[n]), 3), ms_min=round(min(pt[n]), 3),
                      ms_max=round(max(pt[n]), 3)))
    del llm, P
if a.out:
    md = [f"<!-- tools/bench_lora_serving.py ({a.label}, {L} layers, fp16, {a.keys} keys, {a.steps} replays x {a.rounds} interleaved turns) -->", "",
          "| what | slots | variant | ms median | ms min | ms max | over the base step |", "|---|---|---|---|---|---|---|"]
    for r in ROWS:
        if r["what"] == "bytes per adapter slot":
            md.append(f"| bytes per adapter slot | {r['G']} | | {r['gb']} GB | | | |")
        else:
            what = r["what"] if r["what"] == "token step" else f"prefill, {r['rows']} rows"
            md.append(f"| {what} | {r['G']} | {r['variant']} | {r['ms_median']} | {r['ms_min']} | {r['ms_max']} | {r.get('over_base_ms', '')} |")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(md) + "\n")
