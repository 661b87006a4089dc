"""What the paged KV cache (LlamaForCausalLM(kv_pages=N)) costs and what it saves, at 13B dims (synthetic weights, fp16, precise mode,
the default mixed cache: k fp32, v fp16).

ONE process, six arms alternated --reps times per measurement (the measuring guide: compare versions in the same call):

  unpaged        this commit, kv_pages = 0
  paged32/64/128 this commit, one pool sized for sequences x max_cache_len rows, pages handed out in a scrambled order
  parent, parent2 the PARENT commit's package and library (``--parent DIR``: a built checkout of it, loaded under another module name),
                 twice: the second copy gives the run-to-run spread that "the unpaged step has not moved" is judged against

  token step: the graph-replayed lock-step step at (sequences, keys) in --steps-at, caches filled with random values (a step's time
              depends on the bytes it reads), --steps replays per turn between two device events;
  prefill:    one pass of T rows of one sequence from position 0 (--prefill), no logits, device events around the pass.

Then the memory statement (--memory): the allocator's bytes for a 32-slot model with max_cache_len 4096, contiguous and with a pool
sized for 32 x 512 rows, and a generate_inflight run of mixed-length requests that completes on the pool.

--layers (default 40) builds fewer decoder layers, and the table says so: six resident 40-layer models do not fit one GPU beside
their caches; the per-layer work is the same. --out FILE rewrites the section between the measured:begin / measured:end markers.

    git worktree add /tmp/parent HEAD~1 && bash /tmp/parent/seed-x_amd/csrc/build.sh
    python tools/bench_kv_paged.py --parent /tmp/parent --layers 8 --out profiles/kv_paged.md
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from seedx_amd import synthetic as syn
from seedx_amd.llama import LlamaForCausalLM

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its seed-x_amd/lib/libseedx_hip.so exists)")
ap.add_argument("--steps-at", nargs="+", default=["1x256", "1x1536", "16x256", "16x1536", "32x256", "32x1536"], help="SEQUENCESxKEYS")
ap.add_argument("--prefill", nargs="+", type=int, default=[512, 2048])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=32)
ap.add_argument("--layers", type=int, default=40)
ap.add_argument("--memory", action="store_true", help="the 32-slot allocator record and the generate_inflight run")
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev, dt = torch.device("cuda:0"), torch.float16
cfg = dict(syn.FULL_LLM, num_hidden_layers=a.layers)
H, L = cfg["hidden_size"], a.layers
LINES, TABLES = [], []
BEGIN, END = "<!-- measured:begin (tools/bench_kv_paged.py --out rewrites this section) -->", "<!-- measured:end -->"


def emit(d):
    LINES.append(json.dumps(d))
    print(LINES[-1], flush=True)


def load_parent(tree):
    """The parent commit's package under the name seedx_amd_parent: its own Python, its own libseedx_hip.so (ctypes loads it privately)."""
    real = os.path.join(tree, "seed-x_amd")
    spec = importlib.util.spec_from_file_location("seedx_amd_parent", os.path.join(real, "__init__.py"), submodule_search_locations=[real])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["seedx_amd_parent"] = mod
    spec.loader.exec_module(mod)
    from seedx_amd_parent import _lib, llama
    assert os.path.samefile(os.path.dirname(_lib.LIB_PATH), os.path.join(real, "lib")), _lib.LIB_PATH
    return llama.LlamaForCausalLM


ARMS = [("unpaged", LlamaForCausalLM, 0), ("paged32", LlamaForCausalLM, 32), ("paged64", LlamaForCausalLM, 64), ("paged128", LlamaForCausalLM, 128)]
if a.parent:
    Parent = load_parent(a.parent)
    ARMS += [("parent", Parent, 0), ("parent2", Parent, 0)]
SD = syn.llama_state_dict(cfg, dev, dt)


class Arm:
    def __init__(self, name, cls, ps, G, Tmax):
        self.name, self.G, self.Tmax = name, G, Tmax
        kw = dict(kv_pages=G * (-(-Tmax // ps)), kv_page_size=ps) if ps else {}
        llm = self.llm = cls(dict(cfg), max_cache_len=Tmax, max_batch=G, **kw)
        llm.load_state_dict(dict(SD))
        llm.to(dev, dt)
        P = self.P = llm._pack()
        g = torch.Generator(device=dev).manual_seed(1)
        for li in range(L):                               # fill instead of prefilling: finite random rows everywhere
            P["kc"][li].normal_(generator=g)
            P["vc"][li].copy_(torch.randn(P["vc"][li].shape, device=dev, generator=g))
        if ps:
            P["kc"][:, 0].zero_()                         # the null page stays the null page
            P["vc"][:, 0].zero_()
            order = torch.randperm(llm.kv_pages, generator=torch.Generator().manual_seed(7)).tolist()
            for g_ in range(G):                           # every sequence holds max_cache_len rows, on scattered pages
                assert llm.kv_reserve(g_, Tmax)
            # scramble: every page is held, so any permutation over the entries is a valid table; sequence g's entry i gets a page from
            # a seeded one, as a pool that has served a queue for a while would hand them out
            w = llm._pool.width
            tab = torch.tensor([[order[g_ * w + i] + 1 for i in range(w)] for g_ in range(G)], dtype=torch.int32)
            P["ptab"].copy_(tab)
        self.img = torch.arange(31000, 31066, dtype=torch.int32, device=dev)
        self.ids = torch.full((G, a.steps + 2), -1, dtype=torch.int32, device=dev)
        self.hid = torch.zeros((G, a.steps + 2, H), device=dev)

    def rewind(self, keys):
        P = self.P
        P["pos"].fill_(keys)
        P["ctx"].fill_(keys + 1)
        P["step"].zero_()
        P["cur"].copy_(torch.arange(20, 20 + self.G, dtype=torch.int32, device=dev))

    def step_turn(self, keys):
        self.rewind(keys)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.steps):
            self.llm.decode_step(self.img, self.ids, self.hid, use_graph=True)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps

    def prefill_turn(self, x):
        self.P["pos"].zero_()
        self.P["ctx"].fill_(1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        self.llm.forward_embeds_batch([x], [0], need_logits=False)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)


def table(title, what, rows):
    """rows: {arm: [times]} → one markdown table: median, spread, and the median against the unpaged arm."""
    med = {k: float(np.median(v)) for k, v in rows.items()}
    out = [f"#### {title}", "", f"| arm | {what} (median) | min | max | vs unpaged |", "|---|---|---|---|---|"]
    for k, v in rows.items():
        out.append(f"| {k} | {med[k]:.4f} | {min(v):.4f} | {max(v):.4f} | {med[k] / med['unpaged']:.4f} |")
    if "parent" in med:
        out.append("")
        out.append(f"parent measured twice: {med['parent']:.4f} / {med['parent2']:.4f} ms — a run-to-run spread of "
                   f"{abs(med['parent'] - med['parent2']) / med['parent'] * 100:.2f} %; unpaged against the parent's mean: "
                   f"{(med['unpaged'] / ((med['parent'] + med['parent2']) / 2) - 1) * 100:+.2f} %")
    TABLES.append("\n".join(out))


def write_out():
    if not a.out:
        return
    md = [BEGIN, "## Measured on one MI355X", "",
          f"13B dims with {L} of 40 decoder layers, fp16, precise mode, mixed cache; {a.steps} graph replays per token-step turn, {a.reps} alternated "
          "turns per arm, all arms in one process. Times in ms. What a run did not cover is absent: **not measured**.", ""]
    md += ["\n\n".join(TABLES), "", "### Raw lines", "", "```"] + LINES + ["```", END]
    section = "\n".join(md)
    old = open(a.out).read() if os.path.exists(a.out) else "# Paged KV cache (tools/bench_kv_paged.py)\n"
    i, j = old.find("<!-- measured:begin"), old.find(END)
    new = old[:i] + section + old[j + len(END):] if 0 <= i < j else old.rstrip("\n") + "\n\n" + section + "\n"
    with open(a.out, "w") as f:
        f.write(new)


def measure(arms, what, turn, title, unit):
    for m in arms:                                        # warm-up: capture / first launches of every shape the timed window uses
        turn(m)
    times = {m.name: [] for m in arms}
    for rep in range(a.reps):
        for m in arms:
            times[m.name].append(turn(m))
            emit(dict(what=what, arm=m.name, rep=rep, ms=round(times[m.name][-1], 4)))
    table(title, unit, times)
    write_out()


by_G = {}
for c in a.steps_at:
    G, keys = (int(x) for x in c.split("x"))
    by_G.setdefault(G, []).append(keys)
for G, keys_list in by_G.items():
    Tmax = max(keys_list) + a.steps + 8
    arms = [Arm(n, cls, ps, G, Tmax) for n, cls, ps in ARMS]
    for keys in keys_list:
        measure(arms, f"step {G}x{keys}", lambda m: m.step_turn(keys), f"Token step, {G} sequences x {keys} keys", "ms / step")
    del arms
    torch.cuda.empty_cache()
if a.prefill:
    Tmax = max(a.prefill)
    arms = [Arm(n, cls, ps, 1, Tmax) for n, cls, ps in ARMS]
    gx = torch.Generator(device=dev).manual_seed(3)
    for T in a.prefill:
        x = torch.randn((T, H), device=dev, generator=gx) * 0.5
        measure(arms, f"prefill {T}", lambda m: m.prefill_turn(x), f"Prefill pass, {T} rows of one sequence", "ms / pass")
    del arms
    torch.cuda.empty_cache()

if a.memory:
    # the allocator's bytes for 32 slots x max_cache_len 4096: contiguous, then one pool for 32 x 512 rows; a mixed queue runs on the pool
    import bench
    from seedx_amd.seed_x import ContinuousLVLM
    from seedx_amd.visual_encoder import Resampler
    rec = {}
    for name, kw in (("contiguous", {}), ("pool for 32 x 512 rows", dict(kv_pages=32 * 512 // 64, kv_page_size=64))):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated(dev)
        llm = LlamaForCausalLM(dict(cfg), max_cache_len=4096, max_batch=32, **kw)
        llm.load_state_dict(dict(SD))
        llm.to(dev, dt)
        llm._pack()
        rec[name] = dict(allocated_gb=round((torch.cuda.memory_allocated(dev) - before) / 1e9, 3),
                         kv_cache_gb=round(llm.memory_footprint()["kv_cache"] / 1e9, 3))
        emit(dict(what="memory", model=name, **rec[name]))
        if not kw:
            del llm
    agent = ContinuousLVLM(llm, Resampler(8, H, 32, kv_dim=4096), Resampler(8, 4096, 32, kv_dim=H), add_patch_pos=True, vit_down=True)
    agent.load_state_dict(syn.agent_state_dict(H, 4096, dev, dt))
    agent.eval().to(dev, dt)
    rng = np.random.default_rng(0)
    plens = [int(n) for n in np.concatenate([rng.integers(20, 200, 44), rng.integers(1400, 1600, 4)])]     # short chats + a few 1.5k contexts
    rng.shuffle(plens)
    reqs = [dict(input_ids=[[1] + [int(t) for t in rng.integers(10, 30000, n - 1)]], max_new_tokens=int(rng.integers(16, 96))) for n in plens]
    out = agent.generate_inflight(bench.BenchTokenizer(), reqs, eos_token_id=None)
    st = agent.last_inflight_stats
    longest = max(n + r["max_new_tokens"] for n, r in zip(plens, reqs))
    emit(dict(what="inflight on the pool", requests=len(reqs), longest_request_rows=longest, finished=sum(o is not None for o in out), **st))
    TABLES.append("\n".join([
        "#### 32 slots, max_cache_len 4096: what the allocator holds", "",
        "| model | allocated GB (weights + tiles + cache) | of it KV cache GB |", "|---|---|---|"] +
        [f"| {k} | {v['allocated_gb']} | {v['kv_cache_gb']} |" for k, v in rec.items()] + [
        "", f"generate_inflight on the pool: {len(reqs)} requests (44 prompts of 20 .. 200 rows, 4 of 1400 .. 1600; budgets 16 .. 96; the longest "
        f"request holds {longest} rows, which a contiguous cache of 512 rows per slot refuses) all finished: {st['decode_steps']} decode steps, "
        f"{st['admissions']} admissions, {st['page_waits']} page waits, peak {st['peak_pages']} of {llm.kv_pages} pages."]))
    write_out()
