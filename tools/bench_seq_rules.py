"""What the device-side sequence rules (stop sequences, no_repeat_ngram_size) cost, and that a step without them has not moved
(profiles/seq_rules.md).

ONE process, arms alternated --reps times per measurement (the measuring guide: compare versions in the same call):

  unasked:  the step nobody asked for. The graph-replayed lock-step token step at 13B dims with --layers decoder layers, G = 1 / 16 / 32
            at 256 and 1536 keys, plain and with a control state (every row controlled, as in tools/bench_controls.py), on
              parent, parent2  the PARENT commit's package and library (``--parent DIR``: a built checkout of it, loaded under another
                               module name), twice: the second copy gives the run-to-run spread any other difference is judged against
              this             this commit
            The claim to support is "unchanged within that spread".
  seq:      this commit's _seq step against its _ctl step (same controls on every row), every row carrying no_repeat_ngram_size = 3 and
            four 8-id stop sequences, at history lengths 256 / 1536 / 4096 (random ids over the vocabulary; the history is put back
            before every turn), G = 1 / 16 / 32 at 256 keys; and the in-flight tail alone (--launches launches per graph replay).

No threshold is fixed: what is measured is recorded. --out FILE rewrites the section between the measured:begin / measured:end markers.

    git worktree add /tmp/parent HEAD~1 && bash /tmp/parent/seed-x_amd/csrc/build.sh
    python tools/bench_seq_rules.py --parent /tmp/parent --out profiles/seq_rules.md
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
from seedx_amd.llama import ControlState, LlamaForCausalLM, SeqRuleState
from seedx_amd.sampling import ControlParams, SeqParams

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its seed-x_amd/lib/libseedx_hip.so exists)")
ap.add_argument("--G", nargs="+", type=int, default=[1, 16, 32])
ap.add_argument("--keys", nargs="+", type=int, default=[256, 1536])
ap.add_argument("--hist", nargs="+", type=int, default=[256, 1536, 4096])
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--launches", type=int, default=64)
ap.add_argument("--steps", type=int, default=32)
ap.add_argument("--layers", type=int, default=4)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev, dt = torch.device("cuda:0"), torch.float16
V, LD = 32330, 32384
LINES, TABLES = [], []
BEGIN, END = "<!-- measured:begin (tools/bench_seq_rules.py --out rewrites this section) -->", "<!-- measured:end -->"


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


PARENT = load_parent(a.parent) if a.parent else None
i32 = lambda v, n: torch.full((n,), v, dtype=torch.int32, device=dev)


def control_all(cs):
    """Every row of ``cs`` controlled: all five controls, 64 prompt marks, 32 generated ids (tools/bench_controls.py's)."""
    rng = np.random.default_rng(cs.G)
    p = ControlParams(repetition_penalty=1.3, presence_penalty=0.2, frequency_penalty=0.1, logit_bias={17: -float("inf"), 29: 1.5},
                      min_new_tokens=4)
    cs.set_rows(range(cs.G), [p] * cs.G, [rng.integers(0, V, size=64).tolist() for _ in range(cs.G)])
    for g in range(cs.G):
        cs.count([g] * 32, rng.integers(0, V, size=32).tolist())
    return cs


def rule_all(qs, L):
    """Every row of ``qs`` carries n = 3 and four 8-id stops that never match (id V - 1 closes each; the logits keep it from being
    chosen), over a history of L random ids, all of them counted as generated (the stop match compares all four sequences)."""
    rng = np.random.default_rng(1000 + L)
    p = SeqParams(stop=[[int(t) for t in rng.integers(0, V - 1, size=7)] + [V - 1] for _ in range(4)], no_repeat_ngram_size=3)
    qs.set_rows(range(qs.G), [p] * qs.G, [rng.integers(0, V - 1, size=L).tolist() for _ in range(qs.G)])
    qs.prompt_len.zero_()
    return qs


class TailArm:
    """--launches in-flight tails on the same logits in one captured graph; counters, counts and history length are put back per replay."""

    def __init__(self, name, G, L):
        self.name, self.G = name, G
        rows = a.launches + 2
        self.logits = (torch.randn((G, LD), generator=torch.Generator().manual_seed(G)) * 4).to(dev)
        self.logits[:, 2] = self.logits[:, V - 1] = -50.0       # the EOS column and the stops' last id: no slot stops inside a replay
        self.img = torch.arange(31000, 31066, dtype=torch.int32, device=dev)
        self.cur, self.live, self.n_new, self.max_new, self.force_at = i32(7, G), i32(1, G), i32(1, G), i32(1 << 30, G), i32(-1, G)
        self.pos, self.ctx, self.step = i32(10, G), i32(11, G), i32(0, G)
        self.out_ids = torch.full((G, rows), -1, dtype=torch.int32, device=dev)
        self.status = torch.zeros((G, 4), dtype=torch.int32, device=dev)
        self.saved = [(t, t.clone()) for t in (self.cur, self.n_new, self.pos, self.ctx, self.step)]
        args = (self.logits, V, self.img, self.cur, self.live, self.n_new, self.max_new, self.force_at, self.pos, self.ctx, self.step,
                self.out_ids, self.status)
        cs = control_all(ControlState(G, V, LD, dev))
        self.saved.append((cs.counts, cs.counts.clone()))
        if L is None:
            one = lambda: ops.next_slots_ctl(*args, cs, eos_id=2)
        else:
            qs = rule_all(SeqRuleState(G, V, L + rows, dev), L)
            self.saved.append((qs.hist_len, qs.hist_len.clone()))
            one = lambda: ops.next_slots_seq(*args, cs, qs, eos_id=2)
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
    """The lock-step token step of ``llm`` at ``keys`` keys: plain, with controls (``ctl``) or with controls and rules over a history of
    ``L`` ids. Arms may share a model: every kind of step keeps its own captured graph."""

    def __init__(self, name, G, llm, keys, ctl=False, L=None):
        self.name, self.G, self.llm, self.keys = name, G, llm, keys
        self.P = llm._pack()
        if getattr(llm, "_bench_buf", None) is None:           # one set of buffers per model: they are part of the graph key, and the
            llm._bench_buf = (torch.arange(31000, 31066, dtype=torch.int32, device=dev),      # arms of a model must not evict each
                              torch.full((G, a.steps + 2), -1, dtype=torch.int32, device=dev),   # other's captured step
                              torch.zeros((G, a.steps + 2, llm.H), device=dev))
        self.img, self.ids, self.hid = llm._bench_buf
        self.kw, self.saved = {}, []
        if ctl or L is not None:
            cs = control_all(llm.control_state())
            self.kw = dict(controls=cs, eos_id=2)
            self.saved.append((cs.counts, cs.counts.clone()))
        if L is not None:
            if getattr(llm, "_bench_rules", None) is None:     # ONE state per model (its pointers are part of the graph key): the arms
                top = max(a.hist)                              # differ in the history length they put back before every turn
                llm._bench_rules = rule_all(SeqRuleState(G, V, max(llm.Tmax, top + a.steps + 8), dev), top)
            qs = llm._bench_rules
            self.kw["seq_rules"] = qs
            self.saved.append((qs.hist_len, torch.full_like(qs.hist_len, L)))

    def turn(self):
        P = self.P
        P["pos"].fill_(self.keys)
        P["ctx"].fill_(self.keys + 1)
        P["step"].zero_()
        P["cur"].copy_(torch.arange(20, 20 + self.G, dtype=torch.int32, device=dev))
        for t, v in self.saved:
            t.copy_(v)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.steps):
            self.llm.decode_step(self.img, self.ids, self.hid, use_graph=True, **self.kw)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps * 1e3             # µs per step


def table(title, unit, rows, base):
    med = {k: float(np.median(v)) for k, v in rows.items()}
    out = [f"#### {title}", "", f"| arm | {unit} (median) | min | max | vs {base} |", "|---|---|---|---|---|"]
    for k, v in rows.items():
        out.append(f"| {k} | {med[k]:.2f} | {min(v):.2f} | {max(v):.2f} | {med[k] / med[base]:.4f} |")
    out.append("")
    if "parent" in med:
        lo, hi = sorted((med["parent"], med["parent2"]))
        inside = lo <= med["this"] <= hi
        out.append(f"parent measured twice: {med['parent']:.2f} / {med['parent2']:.2f} µs (spread {abs(hi - lo) / lo * 100:.2f} %); this commit "
                   f"against the parents' mean: {(med['this'] / ((lo + hi) / 2) - 1) * 100:+.2f} % — "
                   + ("inside the two parent medians." if inside else
                      f"outside the two parent medians; all parent turns span {min(rows['parent'] + rows['parent2']):.2f} .. "
                      f"{max(rows['parent'] + rows['parent2']):.2f} µs."))
    for k in med:
        if k.startswith("seq"):
            out.append(f"{k}: {med[k] - med[base]:+.2f} µs per {unit.split(' / ')[1]} ({(med[k] / med[base] - 1) * 100:+.2f} %) against {base}.")
    TABLES.append("\n".join(out))


def write_out():
    if not a.out:
        return
    md = [BEGIN, "## Measured on one MI355X", "",
          f"All arms of a table in one process, {a.reps} alternated turns per arm. Step: 13B dims with {a.layers} of 40 decoder layers, fp16, "
          f"precise mode, {a.steps} graph replays per turn. Tail: {a.launches} launches per graph replay, V = {V}. Times in µs.", ""]
    md += ["\n\n".join(TABLES), "", "### Raw lines", "", "```"] + LINES + ["```", END]
    section = "\n".join(md)
    old = open(a.out).read() if os.path.exists(a.out) else "# Device-side sequence rules (tools/bench_seq_rules.py)\n"
    i, j = old.find("<!-- measured:begin"), old.find(END)
    new = old[:i] + section + old[j + len(END):] if 0 <= i < j else old.rstrip("\n") + "\n\n" + section + "\n"
    with open(a.out, "w") as f:
        f.write(new)


def measure(arms, what, title, unit, base):
    for m in arms:
        m.turn()                                               # warm-up (the step arms capture here)
    times = {m.name: [] for m in arms}
    for rep in range(a.reps):
        for m in arms:
            times[m.name].append(m.turn())
            emit(dict(what=what, arm=m.name, rep=rep, us=round(times[m.name][-1], 3)))
    table(title, unit, times, base)
    write_out()


cfg = dict(syn.FULL_LLM, num_hidden_layers=a.layers)
SD = syn.llama_state_dict(cfg, dev, dt)
for G in a.G:
    def build(cls):
        llm = cls(dict(cfg), max_cache_len=max(a.keys) + a.steps + 8, max_batch=G)
        llm.load_state_dict(dict(SD))
        llm.to(dev, dt)
        P = llm._pack()
        g = torch.Generator(device=dev).manual_seed(1)
        for li in range(a.layers):                             # fill instead of prefilling: finite random rows everywhere
            P["kc"][li].normal_(generator=g)
            P["vc"][li].copy_(torch.randn(P["vc"][li].shape, device=dev, generator=g))
        return llm
    models = ([("parent", build(PARENT)), ("parent2", build(PARENT))] if PARENT else []) + [("this", build(LlamaForCausalLM))]
    for keys in a.keys:
        for ctl in (False, True):
            kind = "_ctl step" if ctl else "plain step"
            measure([StepArm(n, G, m, keys, ctl=ctl) for n, m in models], f"unasked {kind} G={G} keys={keys}",
                    f"The step nobody asked for: {kind}, {G} sequences x {keys} keys", "µs / step", "parent" if PARENT else "this")
    this = models[-1][1]
    measure([StepArm("ctl", G, this, a.keys[0], ctl=True)] + [StepArm(f"seq hist={L}", G, this, a.keys[0], L=L) for L in a.hist],
            f"seq step G={G}", f"_seq step against _ctl step, {G} sequences x {a.keys[0]} keys, n = 3 and four 8-id stops on every row",
            "µs / step", "ctl")
    measure([TailArm("ctl", G, None)] + [TailArm(f"seq hist={L}", G, L) for L in a.hist], f"seq tail G={G}",
            f"The in-flight tail alone, G = {G}: _seq against _ctl", "µs / launch", "ctl")
    del models, this
    torch.cuda.empty_cache()
