"""What the device-side logits controls cost, and that a step without them has not moved (profiles/logits_controls.md).

ONE process, arms alternated --reps times per measurement (the measuring guide: compare versions in the same call):

  parent, parent2  the PARENT commit's package and library (``--parent DIR``: a built checkout of it, loaded under another module name),
                   twice: the second copy gives the run-to-run spread that "the uncontrolled tail / step has not moved" is judged against
  plain            this commit, no control state: the tail and the lock-step token step as ever
  ctl              this commit with a control state, EVERY row controlled (repetition, presence and frequency penalties, two bias
                   entries, min_new_tokens; 64 prompt marks and 32 generated ids per row)

  tail:  the in-flight tail alone on fp32 logits [G, 32384] (V = 32330), G = 1 / 16 / 32, every slot live; --launches launches captured
         in one graph per arm, the time of a replay between two device events divided by the launches;
  step:  the graph-replayed lock-step token step at 13B dims with --layers decoder layers, G = 1 / 16 / 32 at --keys keys.

The uncontrolled arm is judged against the spread of the two parent arms; no threshold is fixed. What the controls cost is reported, not
gated. --out FILE rewrites the section between the measured:begin / measured:end markers.

    git worktree add /tmp/parent HEAD~1 && bash /tmp/parent/seed-x_amd/csrc/build.sh
    python tools/bench_controls.py --parent /tmp/parent --out profiles/logits_controls.md
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
from seedx_amd import ops, synthetic as syn
from seedx_amd.llama import ControlState, LlamaForCausalLM
from seedx_amd.sampling import ControlParams

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its seed-x_amd/lib/libseedx_hip.so exists)")
ap.add_argument("--G", nargs="+", type=int, default=[1, 16, 32])
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--launches", type=int, default=64)
ap.add_argument("--steps", type=int, default=32)
ap.add_argument("--layers", type=int, default=4)
ap.add_argument("--keys", type=int, default=256)
ap.add_argument("--no-step", action="store_true")
ap.add_argument("--reverse", action="store_true", help="build and measure the arms in the opposite order (this commit's first)")
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev, dt = torch.device("cuda:0"), torch.float16
V, LD = 32330, 32384
LINES, TABLES = [], []
TAG = "measured-reverse" if a.reverse else "measured"      # each order has a section of its own
BEGIN, END = f"<!-- {TAG}:begin (tools/bench_controls.py --out rewrites this section) -->", f"<!-- {TAG}:end -->"


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
    from seedx_amd_parent import _lib, llama, ops as pops
    assert os.path.samefile(os.path.dirname(_lib.LIB_PATH), os.path.join(real, "lib")), _lib.LIB_PATH
    return pops, llama.LlamaForCausalLM


PARENT = load_parent(a.parent) if a.parent else None
i32 = lambda v, n: torch.full((n,), v, dtype=torch.int32, device=dev)


def control_all(cs):
    """Every row of ``cs`` controlled: all five controls, 64 prompt marks, 32 generated ids."""
    rng = np.random.default_rng(cs.G)
    p = ControlParams(repetition_penalty=1.3, presence_penalty=0.2, frequency_penalty=0.1, logit_bias={17: -float("inf"), 29: 1.5},
                      min_new_tokens=4)
    cs.set_rows(range(cs.G), [p] * cs.G, [rng.integers(0, V, size=64).tolist() for _ in range(cs.G)])
    for g in range(cs.G):
        cs.count([g] * 32, rng.integers(0, V, size=32).tolist())
    return cs


class TailArm:
    """--launches in-flight tails on the same logits in one captured graph; the counters are put back before every replay."""

    def __init__(self, name, G, mod, ctl):
        self.name, self.G = name, G
        rows = a.launches + 2
        self.logits = (torch.randn((G, LD), generator=torch.Generator().manual_seed(G)) * 4).to(dev)
        self.logits[:, 2] = -50.0                               # the controlled arm's EOS column: no slot stops inside a replay
        self.img = torch.arange(31000, 31066, dtype=torch.int32, device=dev)
        self.cur, self.live, self.n_new, self.max_new, self.force_at = i32(7, G), i32(1, G), i32(1, G), i32(1 << 30, G), i32(-1, G)
        self.pos, self.ctx, self.step = i32(10, G), i32(11, G), i32(0, G)
        self.out_ids = torch.full((G, rows), -1, dtype=torch.int32, device=dev)
        self.status = torch.zeros((G, 4), dtype=torch.int32, device=dev)
        self.saved = [(t, t.clone()) for t in (self.cur, self.n_new, self.pos, self.ctx, self.step)]
        args = (self.logits, V, self.img, self.cur, self.live, self.n_new, self.max_new, self.force_at, self.pos, self.ctx, self.step,
                self.out_ids, self.status)
        if not ctl:
            one = lambda: mod.greedy_next_slots(*args)
        else:
            cs = control_all(ControlState(G, V, LD, dev))
            self.saved.append((cs.counts, cs.counts.clone()))
            one = lambda: mod.next_slots_ctl(*args, cs, eos_id=2)
        one()
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with ops.graph_capture(self.graph):
            for _ in range(a.launches):
                one()

    def turn(self):
        for t, v in self.saved:
            t.copy_(v)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        self.graph.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.launches * 1e3          # µs per launch


class StepArm:
    def __init__(self, name, G, llm, ctl):
        self.name, self.G, self.llm = name, G, llm
        self.P = llm._pack()
        self.img = torch.arange(31000, 31066, dtype=torch.int32, device=dev)
        self.ids = torch.full((G, a.steps + 2), -1, dtype=torch.int32, device=dev)
        self.hid = torch.zeros((G, a.steps + 2, llm.H), device=dev)
        self.kw, self.counts0 = {}, None
        if ctl:
            cs = control_all(llm.control_state())
            self.kw, self.counts0 = dict(controls=cs, eos_id=2), cs.counts.clone()

    def turn(self):
        P = self.P
        P["pos"].fill_(a.keys)
        P["ctx"].fill_(a.keys + 1)
        P["step"].zero_()
        P["cur"].copy_(torch.arange(20, 20 + self.G, dtype=torch.int32, device=dev))
        if self.counts0 is not None:
            self.kw["controls"].counts.copy_(self.counts0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.steps):
            self.llm.decode_step(self.img, self.ids, self.hid, use_graph=True, **self.kw)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps * 1e3             # µs per step


def table(title, unit, rows):
    med = {k: float(np.median(v)) for k, v in rows.items()}
    out = [f"#### {title}", "", f"| arm | {unit} (median) | min | max | vs plain |", "|---|---|---|---|---|"]
    for k, v in rows.items():
        out.append(f"| {k} | {med[k]:.2f} | {min(v):.2f} | {max(v):.2f} | {med[k] / med['plain']:.4f} |")
    out.append("")
    if "parent" in med:
        lo, hi = sorted((med["parent"], med["parent2"]))
        inside = lo <= med["plain"] <= hi
        out.append(f"parent measured twice: {med['parent']:.2f} / {med['parent2']:.2f} µs (spread {abs(hi - lo) / lo * 100:.2f} %); plain against "
                   f"the parents' mean: {(med['plain'] / ((lo + hi) / 2) - 1) * 100:+.2f} % — "
                   + ("inside the two parent medians." if inside else
                      f"outside the two parent medians; all parent turns span {min(rows['parent'] + rows['parent2']):.2f} .. "
                      f"{max(rows['parent'] + rows['parent2']):.2f} µs."))
    out.append(f"Controls on every row cost {med['ctl'] - med['plain']:+.2f} µs per {unit.split(' / ')[1]} "
               f"({(med['ctl'] / med['plain'] - 1) * 100:+.2f} %).")
    TABLES.append("\n".join(out))


def write_out():
    if not a.out:
        return
    md = [BEGIN, "## Measured on one MI355X" + (", arms built and measured in reverse order" if a.reverse else ""), "",
          f"All arms of a table in one process, {a.reps} alternated turns per arm. Tail: {a.launches} launches per graph replay, V = {V}. Step: 13B "
          f"dims with {a.layers} of 40 decoder layers, fp16, precise mode, {a.keys} keys, {a.steps} graph replays per turn. Times in µs.", ""]
    md += ["\n\n".join(TABLES), "", "### Raw lines", "", "```"] + LINES + ["```", END]
    section = "\n".join(md)
    old = open(a.out).read() if os.path.exists(a.out) else "# Device-side logits controls (tools/bench_controls.py)\n"
    i, j = old.find(f"<!-- {TAG}:begin"), old.find(END)
    new = old[:i] + section + old[j + len(END):] if 0 <= i < j else old.rstrip("\n") + "\n\n" + section + "\n"
    with open(a.out, "w") as f:
        f.write(new)


def measure(arms, what, title, unit):
    if a.reverse:
        title += " (arms in reverse order)"
    for m in arms:
        m.turn()                                               # warm-up (the step arms capture here)
    times = {m.name: [] for m in arms}
    for rep in range(a.reps):
        for m in arms:
            times[m.name].append(m.turn())
            emit(dict(what=what, arm=m.name, rep=rep, us=round(times[m.name][-1], 3)))
    table(title, unit, times)
    write_out()


for G in a.G:
    specs = [("parent", PARENT[0], False), ("parent2", PARENT[0], False)] if PARENT else []
    specs += [("plain", ops, False), ("ctl", ops, True)]
    arms = [TailArm(n, G, mod, k) for n, mod, k in (specs[::-1] if a.reverse else specs)]
    measure(arms, f"tail G={G}", f"The in-flight tail alone, G = {G}", "µs / launch")
    del arms
if not a.no_step:
    cfg = dict(syn.FULL_LLM, num_hidden_layers=a.layers)
    SD = syn.llama_state_dict(cfg, dev, dt)
    for G in a.G:
        def build(cls):
            llm = cls(dict(cfg), max_cache_len=a.keys + a.steps + 8, max_batch=G)
            llm.load_state_dict(dict(SD))
            llm.to(dev, dt)
            P = llm._pack()
            g = torch.Generator(device=dev).manual_seed(1)
            for li in range(a.layers):                         # fill instead of prefilling: finite random rows everywhere
                P["kc"][li].normal_(generator=g)
                P["vc"][li].copy_(torch.randn(P["vc"][li].shape, device=dev, generator=g))
            return llm
        # one model per arm: each keeps its own captured step
        specs = [("parent", PARENT[1], False), ("parent2", PARENT[1], False)] if PARENT else []
        specs += [("plain", LlamaForCausalLM, False), ("ctl", LlamaForCausalLM, True)]
        arms = [StepArm(n, G, build(cls), k) for n, cls, k in (specs[::-1] if a.reverse else specs)]
        measure(arms, f"step G={G}", f"Token step, {G} sequences x {a.keys} keys, {a.layers} layers", "µs / step")
        del arms
        torch.cuda.empty_cache()
