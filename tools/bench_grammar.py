"""What constrained decoding costs on the device and on the host (profiles/grammar.md).

ONE process, arms alternated --reps times per measurement (the measuring guide: compare versions in the same call):

  parent, parent2  the PARENT commit's package and library (``--parent DIR``: a built checkout of it, loaded under another module name),
                   twice: the second copy gives the run-to-run spread every difference is judged against
  ctl              this commit's controlled form, as the parent runs it
  fsm_none         this commit's constrained form with NO row constrained (table = -1 everywhere)
  fsm_all          ... with EVERY row constrained (``([a-z]+ )*`` over a synthetic 32 330-piece vocabulary: it never finishes, so no slot
                   stops inside a replay; every launch reads one table row per slot, masks into the working row and advances the state)

  tail:  sx_next_slots_fsm against the parent's sx_next_slots_ctl on fp32 logits [G, 32384] (V = 32330), G = 1 / 16 / 32 slots, every slot
         live, greedy and sampled (temperature 1, top-k 50, top-p 0.9), controls off on every row: --launches launches captured in one graph
         per arm, the time of a replay between two device events divided by the launches;
  step:  the graph-replayed lock-step token step at 13B dims with --layers decoder layers, G = 1 / 16 / 32 at --keys keys, every row
         controlled as in profiles/logits_controls.md, with and without a grammar, against the controlled step of the parent;
  host:  seconds to build TokenFSM.from_regex for an integer, a four-way choice and a small JSON object against the synthetic vocabulary,
         the states of each and the bytes of a loaded table.

Nothing is gated. --out FILE rewrites the section between the measured:begin / measured:end markers.

    git worktree add /tmp/parent HEAD~1 && bash /tmp/parent/seed-x_amd/csrc/build.sh
    python tools/bench_grammar.py --parent /tmp/parent --out profiles/grammar.md
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from seedx_amd import ops, synthetic as syn
from seedx_amd.grammar import TokenFSM
from seedx_amd.llama import ControlState, LlamaForCausalLM, SampleState
from seedx_amd.sampling import ControlParams, SamplingParams

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its seed-x_amd/lib/libseedx_hip.so exists)")
ap.add_argument("--G", nargs="+", type=int, default=[1, 16, 32])
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--launches", type=int, default=64)
ap.add_argument("--steps", type=int, default=32)
ap.add_argument("--layers", type=int, default=4)
ap.add_argument("--keys", type=int, default=256)
ap.add_argument("--no-step", action="store_true")
ap.add_argument("--no-tail", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev, dt = torch.device("cuda:0"), torch.float16
V, LD, EOS = 32330, 32384, 2
LINES, TABLES = [], []
BEGIN, END = "<!-- measured:begin (tools/bench_grammar.py --out rewrites this section) -->", "<!-- measured:end -->"
PATTERNS = {"integer": r"-?(0|[1-9][0-9]{0,8})", "four-way choice": r" ?(A|B|C|D)",
            "JSON object": r'\{"name": "[a-z ]{1,40}", "count": (0|[1-9][0-9]{0,3}), "ok": (true|false)\}'}


def emit(d):
    LINES.append(json.dumps(d))
    print(LINES[-1], flush=True)


def synthetic_vocab(n=V, seed=0):
    """A sentencepiece-like vocabulary: 3 specials, 256 byte pieces, then random lower-case / digit / punctuation pieces of 2 .. 8 bytes
    (half with a leading space); the last 330 ids are added tokens (None)."""
    rng = np.random.default_rng(seed)
    vocab = [None, None, None] + [bytes([b]) for b in range(256)]
    seen = set(vocab[3:])
    alpha = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789 \":,{}.-", dtype=np.uint8)
    while len(vocab) < n - 330:
        k = int(rng.integers(2, 9))
        p = bytes(rng.choice(alpha[:26] if rng.random() < 0.7 else alpha, size=k))
        if rng.random() < 0.5:
            p = b" " + p
        if p not in seen:
            seen.add(p)
            vocab.append(p)
    return vocab + [None] * 330


VOCAB = synthetic_vocab()
BANNED = range(V - 330, V)
LOOP = TokenFSM.from_regex(r"([a-z]+ )*", VOCAB, eos_id=EOS, banned_ids=BANNED)


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


class Fsm:
    """table / state / trans / flags as ops takes them: one resident grammar of LOOP's states."""

    def __init__(self, G, on):
        t, f = LOOP.table(LOOP.n_states, LD)
        self.trans, self.flags = torch.from_numpy(t)[None].contiguous().to(dev), torch.from_numpy(f)[None].contiguous().to(dev)
        self.table, self.state = i32(0 if on else -1, G), i32(0 if on else -2, G)


def control_all(cs):
    """Every row of ``cs`` controlled as in tools/bench_controls.py: all five controls, 64 prompt marks, 32 generated ids."""
    rng = np.random.default_rng(cs.G)
    p = ControlParams(repetition_penalty=1.3, presence_penalty=0.2, frequency_penalty=0.1, logit_bias={17: -float("inf"), 29: 1.5},
                      min_new_tokens=4)
    cs.set_rows(range(cs.G), [p] * cs.G, [rng.integers(0, V, size=64).tolist() for _ in range(cs.G)])
    for g in range(cs.G):
        cs.count([g] * 32, rng.integers(0, V, size=32).tolist())
    return cs


class TailArm:
    """--launches in-flight tails on the same logits in one captured graph; counters and automaton states are put back before a replay."""

    def __init__(self, name, G, mod, fsm, sampled):
        self.name, self.G = name, G
        rows = a.launches + 2
        self.logits = (torch.randn((G, LD), generator=torch.Generator().manual_seed(G)) * 4).to(dev)
        self.logits[:, EOS] = -50.0                             # no slot stops inside a replay
        self.img = torch.arange(31000, 31066, dtype=torch.int32, device=dev)
        self.cur, self.live, self.n_new, self.max_new, self.force_at = i32(7, G), i32(1, G), i32(1, G), i32(1 << 30, G), i32(-1, G)
        self.pos, self.ctx, self.step = i32(10, G), i32(11, G), i32(0, G)
        self.out_ids = torch.full((G, rows), -1, dtype=torch.int32, device=dev)
        self.status = torch.zeros((G, 4), dtype=torch.int32, device=dev)
        self.saved = [(t, t.clone()) for t in (self.cur, self.n_new, self.pos, self.ctx, self.step)]
        args = (self.logits, V, self.img, self.cur, self.live, self.n_new, self.max_new, self.force_at, self.pos, self.ctx, self.step,
                self.out_ids, self.status)
        cs = ControlState(G, V, LD, dev)                        # every row off: what is measured is the automaton
        sp = None
        if sampled:
            sp = SampleState(G, dev)
            sp.set_rows(range(G), [SamplingParams(do_sample=True, temperature=1.0, top_k=50, top_p=0.9, seed=100 + g) for g in range(G)])
        if fsm is None:
            one = lambda: mod.next_slots_ctl(*args, cs, sample=sp, eos_id=EOS)
        else:
            fs = Fsm(G, fsm == "all")
            self.saved.append((fs.state, fs.state.clone()))
            one = lambda: mod.next_slots_fsm(*args, cs, fs, sample=sp, eos_id=EOS)
        self.keep = (cs, sp, one)                               # the captured launches hold raw pointers into these
        one()
        torch.cuda.synchronize()
        assert self.live.all(), "a slot stopped: the arm would measure parked slots"
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
        assert self.live.all(), f"{self.name}: a slot stopped inside the replay (status {self.status.tolist()})"
        return e0.elapsed_time(e1) / a.launches * 1e3          # µs per launch


class StepArm:
    def __init__(self, name, G, llm, fsm):
        self.name, self.G, self.llm = name, G, llm
        self.P = llm._pack()
        self.img = torch.arange(31000, 31066, dtype=torch.int32, device=dev)
        self.ids = torch.full((G, a.steps + 2), -1, dtype=torch.int32, device=dev)
        self.hid = torch.zeros((G, a.steps + 2, llm.H), device=dev)
        cs = control_all(llm.control_state())
        self.kw, self.counts0, self.gs = dict(controls=cs, eos_id=EOS), cs.counts.clone(), None
        if fsm is not None:
            llm.load_grammar("loop", LOOP)
            self.gs = llm.grammar_state()
            self.names = ["loop" if fsm == "all" else None] * G
            self.kw["grammar"] = self.gs

    def turn(self):
        P = self.P
        P["pos"].fill_(a.keys)
        P["ctx"].fill_(a.keys + 1)
        P["step"].zero_()
        P["cur"].copy_(torch.arange(20, 20 + self.G, dtype=torch.int32, device=dev))
        self.kw["controls"].counts.copy_(self.counts0)
        if self.gs is not None:
            self.gs.set_rows(range(self.G), self.names)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.steps):
            self.llm.decode_step(self.img, self.ids, self.hid, use_graph=True, **self.kw)
        e1.record()
        torch.cuda.synchronize()
        if self.gs is not None and self.names[0] is not None:
            assert (self.gs.state >= 0).all(), "a row's automaton finished: the arm would measure unconstrained rows"
        return e0.elapsed_time(e1) / a.steps * 1e3             # µs per step


def table(title, unit, rows, base):
    med = {k: float(np.median(v)) for k, v in rows.items()}
    out = [f"#### {title}", "", f"| arm | {unit} (median) | min | max | vs {base} |", "|---|---|---|---|---|"]
    for k, v in rows.items():
        out.append(f"| {k} | {med[k]:.2f} | {min(v):.2f} | {max(v):.2f} | {med[k] / med[base]:.4f} |")
    out.append("")
    if "parent2" in med:
        lo, hi = sorted((med["parent"], med["parent2"]))
        out.append(f"parent measured twice: {med['parent']:.2f} / {med['parent2']:.2f} µs (spread {abs(hi - lo) / lo * 100:.2f} %); all parent "
                   f"turns span {min(rows['parent'] + rows['parent2']):.2f} .. {max(rows['parent'] + rows['parent2']):.2f} µs.")
    per = unit.split(" / ")[1]
    out.append(f"No row constrained: {med['fsm_none'] - med[base]:+.2f} µs per {per} against {base}; every row constrained: "
               f"{med['fsm_all'] - med[base]:+.2f} µs per {per} ({(med['fsm_all'] / med[base] - 1) * 100:+.2f} %).")
    TABLES.append("\n".join(out))


def write_out():
    if not a.out:
        return
    md = [BEGIN, "## Measured on one MI355X", "",
          f"All arms of a table in one process, {a.reps} alternated turns per arm. Tail: {a.launches} launches per graph replay, V = {V}, ld "
          f"{LD}, controls off. Step: 13B dims with {a.layers} of 40 decoder layers, fp16, precise mode, {a.keys} keys, {a.steps} graph "
          "replays per turn, every row controlled. Times in µs.", ""]
    md += ["\n\n".join(TABLES), "", "### Raw lines", "", "```"] + LINES + ["```", END]
    section = "\n".join(md)
    old = open(a.out).read() if os.path.exists(a.out) else "# Constrained decoding (tools/bench_grammar.py)\n"
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


# ---- host ------------------------------------------------------------------------------------------------------------------------------
rows = ["#### Host: TokenFSM.from_regex against a synthetic vocabulary of 32 330 pieces", "",
        "| grammar | pattern | DFA states | token states | seconds | table bytes (its states) | resident bytes (256 states) |", "|---|---|---|---|---|---|---|"]
for name, pat in PATTERNS.items():
    from seedx_amd.grammar import compile_regex
    t0 = time.perf_counter()
    fsm = TokenFSM.from_regex(pat, VOCAB, eos_id=EOS, banned_ids=BANNED, max_states=256)
    sec = time.perf_counter() - t0
    d = dict(what="host", grammar=name, dfa_states=compile_regex(pat).n_states, states=fsm.n_states, seconds=round(sec, 3),
             table_bytes=fsm.n_states * (LD * 2 + 4), resident_bytes=256 * (LD * 2 + 4))
    emit(d)
    rows.append(f"| {name} | `{pat}` | {d['dfa_states']} | {d['states']} | {sec:.2f} | {d['table_bytes']} | {d['resident_bytes']} |")
TABLES.append("\n".join(rows))
write_out()

# ---- tail ------------------------------------------------------------------------------------------------------------------------------
base = "parent" if PARENT else "ctl"
if not a.no_tail:
    for sampled in (False, True):
        for G in a.G:
            specs = [("parent", PARENT[0], None), ("parent2", PARENT[0], None)] if PARENT else []
            specs += [("ctl", ops, None), ("fsm_none", ops, "none"), ("fsm_all", ops, "all")]
            arms = [TailArm(n, G, mod, k, sampled) for n, mod, k in specs]
            how = "sampled" if sampled else "greedy"
            measure(arms, f"tail {how} G={G}", f"The in-flight tail alone, {how}, {G} slots", "µs / launch", base)
            del arms
# ---- step ------------------------------------------------------------------------------------------------------------------------------
if not a.no_step:
    cfg = dict(syn.FULL_LLM, num_hidden_layers=a.layers)
    SD = syn.llama_state_dict(cfg, dev, dt)
    for G in a.G:
        def build(cls, **kw):
            llm = cls(dict(cfg), max_cache_len=a.keys + a.steps + 8, max_batch=G, **kw)
            llm.load_state_dict(dict(SD))
            llm.to(dev, dt)
            P = llm._pack()
            g = torch.Generator(device=dev).manual_seed(1)
            for li in range(a.layers):                         # fill instead of prefilling: finite random rows everywhere
                P["kc"][li].normal_(generator=g)
                P["vc"][li].copy_(torch.randn(P["vc"][li].shape, device=dev, generator=g))
            return llm
        # one model per arm: each keeps its own captured step
        specs = [("parent", PARENT[1], None), ("parent2", PARENT[1], None)] if PARENT else []
        specs += [("ctl", LlamaForCausalLM, None), ("fsm_none", LlamaForCausalLM, "none"), ("fsm_all", LlamaForCausalLM, "all")]
        arms = [StepArm(n, G, build(cls, **(dict(max_grammars=1, grammar_states=256) if k else {})), k) for n, cls, k in specs]
        measure(arms, f"step G={G}", f"Token step, {G} sequences x {a.keys} keys, {a.layers} layers", "µs / step", base)
        del arms
        torch.cuda.empty_cache()
