"""What a verify step of speculative decoding costs against the plain slot step (LlamaForCausalLM(spec_tokens=K),
decode_step(..., slots=st, spec=True, draft="given")): 13B dimensions, synthetic weights, fp16, precise mode, --keys (256 and 1536) keys
in every slot's cache. ONE process; the models are built one after the other from one state dict. Per key count it records

  * ms per plain slot step at G = 1, 4, 16 sequences (graph replay; the plain step of a spec_tokens model is the step of a model without),
  * ms per verify step at (G, T) = (1, 4), (1, 8), (2, 8), (4, 8), T = K + 1 rows per sequence, no drafts accepted,
  * one layer's attention launches alone: the verify form (T rows) against the T = 1 fused form, same G, same key splits,
  * tokens per second of one sequence at T = 8 with the emitted count held at 1, 2, 4 and 8 per step: the drafts are cut from the
    sequence's own no-draft transcript (e - 1 right ids, then a wrong one), written into the row inputs from a device-side table
    before every replay (two small device copies per step, inside the timed region),
  * the break-even emitted count t_verify / t_plain at the same G.

The cache rows hold random values (no prefill: the step's cost does not depend on what the keys are). Acceptance on real text is NOT
measured here: there is no checkpoint, and random weights say nothing about language.

--out FILE replaces the section between the "measured:begin" / "measured:end" marker lines of FILE (creates FILE if missing).

    python tools/bench_spec_decode.py --out profiles/spec_decode.md
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seedx_amd import ops
from seedx_amd import synthetic as syn
from seedx_amd.llama import LlamaForCausalLM

ap = argparse.ArgumentParser()
ap.add_argument("--keys", type=int, nargs="*", default=[256, 1536])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--steps", type=int, default=48)
ap.add_argument("--layers", type=int, default=None, help="fewer decoder layers than 40 (quick looks; the table says so)")
ap.add_argument("--attn-launches", type=int, default=100)
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "tools/bench_spec_decode.py measures on the GPU: there is no CPU fall-back"
dev, dt = torch.device("cuda:0"), torch.float16
cfg = dict(syn.FULL_LLM)
if a.layers:
    cfg["num_hidden_layers"] = a.layers
H, L = cfg["hidden_size"], cfg["num_hidden_layers"]
TMAX = max(a.keys) + 8 * a.steps + 16
LINES, PLAIN, VERIFY, ATTN, TOKS = [], {}, {}, [], []


def emit(d):
    LINES.append(json.dumps(d))
    print(LINES[-1], flush=True)


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


class Model:
    def __init__(self, G, K):
        self.G, self.K, self.T = G, K, K + 1
        llm = self.llm = LlamaForCausalLM(dict(cfg), max_cache_len=TMAX, max_batch=G, precise=True, spec_tokens=K)
        llm.load_state_dict(dict(sd))
        llm.to(dev, dt)
        P = self.P = llm._pack()
        for li in range(L):                            # random cache rows, layer by layer (no prefill)
            P["kc"][li].normal_()
            P["vc"][li].normal_()
        self.img = torch.arange(31000, 31066, dtype=torch.int32, device=dev)
        rows = 8 * a.steps + 16
        self.ids = torch.full((G, rows), -1, dtype=torch.int32, device=dev)
        self.hid = torch.zeros((G, rows, H), device=dev)
        self.st = llm.slot_state(force_id=-1, eos_id=-1)

    def rewind(self, keys):
        P, st, G = self.P, self.st, self.G
        P["pos"].fill_(keys)
        P["ctx"].fill_(keys + 1)
        P["step"].fill_(1)
        P["cur"].copy_(torch.arange(20, 20 + G, dtype=torch.int32, device=dev))
        st.live.fill_(1)
        st.n_new.fill_(1)
        st.max_new.fill_(1 << 20)
        st.force_at.fill_(-1)
        if self.K:
            P["spec"]["rows"].copy_(P["cur"].repeat_interleave(self.T))
            P["spec"]["n_draft"].zero_()

    def plain(self, keys):
        def turn():
            self.rewind(keys)
            return timed(lambda i: self.llm.decode_step(self.img, self.ids, self.hid, use_graph=True, slots=self.st), a.steps)
        turn()                                          # capture + warm-up
        return [turn() for _ in range(a.reps)]

    def verify(self, keys, table=None):
        """table: (rows [steps, G*T], n_draft [steps, G]) on the device, copied into the step's inputs before every replay"""
        S = self.P["spec"]

        def step(i):
            if table is not None:
                S["rows"].copy_(table[0][i])
                S["n_draft"].copy_(table[1][i])
            self.llm.decode_step(self.img, self.ids, self.hid, use_graph=True, slots=self.st, spec=True, draft="given")

        def turn():
            self.rewind(keys)
            return timed(step, a.steps)
        turn()
        return [turn() for _ in range(a.reps)]

    def attention(self, keys, T):
        """one layer's attention launches (split kernel + combine) alone, as the step issues them: a captured chain of launches"""
        llm, P, G = self.llm, self.P, self.G
        qkv = torch.randn(G * T, 3 * H, device=dev)
        pos = torch.full((G,), keys, dtype=torch.int32, device=dev)
        part = torch.empty((G * T, llm.nh_l, llm.decode_nsplit_f32, llm.hd + 2), dtype=torch.float32, device=dev)
        go = lambda: ops.attention_f32(qkv, P["kc"][0], P["vc"][0], pos, G, T, llm.nh_l, llm.hd, llm.hd ** -0.5, dt, tiled=True,
                                       nsplit=llm.decode_nsplit_f32, scratch=part, rope=(P["cos"], P["sin"]))
        go()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(a.attn_launches):
                go()
        g.replay()
        return [timed(lambda i: g.replay(), 1) * 1e3 / a.attn_launches for _ in range(a.reps)]


def med(v):
    return float(np.median(v))


def write_out():
    if not a.out:
        return
    BEGIN, END = "<!-- measured:begin (tools/bench_spec_decode.py --out rewrites this section) -->", "<!-- measured:end -->"
    md = [BEGIN, "## Step times (measured on one MI355X)", "",
          f"13B dims ({L} layers), fp16, precise mode, synthetic weights, graph replay, {a.steps} steps per turn, median of {a.reps} turns, all in one "
          "process. No draft is accepted in the verify rows of this table (the step's cost does not depend on acceptance).", "",
          "| keys | step | sequences G | rows per sequence T | rows | ms / step | x plain step at the same G (= break-even emitted count) |", "|---|---|---|---|---|---|---|"]
    for keys in a.keys:
        for G in sorted(g for (k, g) in PLAIN if k == keys):
            md.append(f"| {keys} | plain | {G} | 1 | {G} | {PLAIN[keys, G]:.3f} | 1.00 |")
        for (k, G, T) in sorted(VERIFY):
            if k == keys:
                base = PLAIN.get((keys, G))
                md.append(f"| {keys} | verify | {G} | {T} | {G * T} | {VERIFY[k, G, T]:.3f} | " + (f"{VERIFY[k, G, T] / base:.2f}" if base else "plain step not measured") + " |")
    for keys in a.keys:
        v, p16 = VERIFY.get((keys, 1, 8)), PLAIN.get((keys, 16))
        if v is None or p16 is None:
            continue
        line = f"At {keys} keys the (1, 8) verify step takes {v:.3f} ms, the plain 16-sequence step {p16:.3f} ms"
        if v > p16:
            av = next((r["us_per_launch"] for r in ATTN if r["keys"] == keys and r["G"] == 1 and r["T"] == 8), None)
            a16 = next((r["us_per_launch"] for r in ATTN if r["keys"] == keys and r["G"] == 16 and r["T"] == 1), None)
            if av is not None and a16 is not None:
                d_att = (av - a16) * L / 1e3
                who = "the verify attention launch (attn_f32_verify_kernel + combine)" if d_att > 0.5 * (v - p16) else \
                    "not the attention (the launches outside it: the 8-row GEMVs, norms and the step's tail)"
                line += f": {v - p16:.3f} ms more. The attention launches account for {d_att:+.3f} ms of that ({L} layers x ({av:.1f} - {a16:.1f}) us): responsible is {who}"
            else:
                line += f": {v - p16:.3f} ms more (attention launches not measured: no attribution)"
        else:
            line += ": the 8 rows of one sequence cost no more than 16 sequences"
        md += ["", line + "."]
    md += ["", "## The attention launches of one layer", "",
           f"Split kernel + combine as the step issues them (tiled output, the model's key splits), {a.attn_launches} launches per captured graph, median of {a.reps}.", "",
           "| keys | G | T | key splits | us / launch | x the T = 1 launch at the same G |", "|---|---|---|---|---|---|"]
    for r in ATTN:
        base = next((q["us_per_launch"] for q in ATTN if q["keys"] == r["keys"] and q["G"] == r["G"] and q["T"] == 1), None)
        md.append(f"| {r['keys']} | {r['G']} | {r['T']} | {r['nsplit']} | {r['us_per_launch']:.1f} | " + (f"{r['us_per_launch'] / base:.2f}" if base else "-") + " |")
    md += ["", "## Tokens per second of one sequence, emitted count held fixed", "",
           "G = 1, T = 8, draft=\"given\": drafts cut from the sequence's own transcript (e - 1 right ids, then a wrong one), copied into the row inputs "
           "from a device-side table before every replay (inside the timed region). The emitted count is read back after the turn.", "",
           "| keys | emitted per step (asked) | emitted per step (measured) | ms / step | tokens / s | x the plain step's tokens / s |", "|---|---|---|---|---|---|"]
    for r in TOKS:
        md.append(f"| {r['keys']} | {r['asked']} | {r['emitted_per_step']:.2f} | {r['ms_per_step']:.3f} | {r['tokens_per_s']:.0f} | {r['x_plain']:.2f} |")
    md += ["", "Acceptance on real SEED-X text is not measured: there is no checkpoint here, and random weights say nothing about language. The break-even "
           "column says what acceptance has to deliver.", "", "### Raw lines", "", "```"] + LINES + ["```", END]
    section = "\n".join(md)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    old = open(a.out).read() if os.path.exists(a.out) else "# Speculative decoding: the verify step against the plain slot step (tools/bench_spec_decode.py)\n"
    i, j = old.find("<!-- measured:begin"), old.find(END)
    new = old[:i] + section + old[j + len(END):] if 0 <= i < j else old.rstrip("\n") + "\n\n" + section + "\n"
    with open(a.out, "w") as f:
        f.write(new)


sd = syn.llama_state_dict(cfg, dev, dt)
for G, K in ((1, 7), (1, 3), (2, 7), (4, 7), (16, 0)):
    m = Model(G, K)
    for keys in a.keys:
        if K in (0, 7):
            t = m.plain(keys)
            PLAIN[keys, G] = med(t)
            emit(dict(step="plain", keys=keys, G=G, ms_per_step=round(med(t), 4), spread_ms=round(max(t) - min(t), 4)))
        for T in sorted({1, K + 1}):
            t = m.attention(keys, T)
            ATTN.append(dict(keys=keys, G=G, T=T, nsplit=m.llm.decode_nsplit_f32, us_per_launch=round(med(t), 2), spread_us=round(max(t) - min(t), 2)))
            emit(dict(step="attention", **ATTN[-1]))
        if not K:
            continue
        t = m.verify(keys)
        VERIFY[keys, G, K + 1] = med(t)
        emit(dict(step="verify", keys=keys, G=G, T=K + 1, ms_per_step=round(med(t), 4), spread_ms=round(max(t) - min(t), 4)))
        if (G, K) == (1, 7):
            m.rewind(keys)                              # the sequence's own transcript, one token per step
            n_tok = 8 * a.steps + 1
            for _ in range(n_tok - 1):
                m.llm.decode_step(m.img, m.ids, m.hid, use_graph=True, slots=m.st, spec=True, draft="given")
            tr = m.ids[0, :n_tok].clone()
            tr[0] = 20                                   # token 0 is the current token the turn starts from
            for e in (1, 2, 4, 8):
                rows = torch.zeros((a.steps, 8), dtype=torch.int32, device=dev)
                for i in range(a.steps):
                    rows[i, :e] = tr[i * e:i * e + e]                      # cur, then e - 1 right ids
                    rows[i, e:] = (tr[i * e + e] + 1) % 1000                 # a wrong id (and padding)
                nd = torch.full((a.steps, 1), min(e, 7), dtype=torch.int32, device=dev)
                t = m.verify(keys, (rows, nd))
                got = (int(m.st.n_new[0].item()) - 1) / a.steps
                ms = med(t)
                TOKS.append(dict(keys=keys, asked=e, emitted_per_step=got, ms_per_step=round(ms, 4), tokens_per_s=round(got / ms * 1e3, 1),
                                 x_plain=round(got / ms * PLAIN[keys, 1], 3)))
                emit(dict(step="tokens", **TOKS[-1]))
    del m
    torch.cuda.empty_cache()
    write_out()          # after every model: a run cut short leaves what it measured
