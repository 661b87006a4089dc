"""Lossless speculative decoding on the GPU: the verify form of the fused-RoPE fp32 attention against T successive T = 1 launches (bit
for bit), the draft and accept kernels against seedx_amd.spec, the verify token step of LlamaForCausalLM(spec_tokens=K) (oracle drafts
change nothing but the step count; graph replay == eager) and ContinuousLVLM.generate_inflight with ``agent.speculative``."""
import math

import pytest
import torch

from oracle import weights
from tests.test_models_gpu import StubTokenizer, relerr

pytestmark = pytest.mark.gpu

DTS = [torch.float16, torch.bfloat16]
D, TMAX = 128, 1536
IMG_IDS = list(range(400, 466))          # <img>, <img_00000> .. <img_00063>, </img> of the StubTokenizer
VIT = 128
KW = dict(num_img_gen_tokens=16, eos_token_id=None)
_SD = {}
_ATT = {}


def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


# ---- 1. verify attention ---------------------------------------------------------------------------------------------------------------
def _attn_inputs(dev, G, T, H):
    """qkv rows, caches and tables for one geometry, made once (fp32 on the device; every test clones what it lets a kernel write)."""
    key = (G, T, H)
    if key not in _ATT:
        g = torch.Generator().manual_seed(41)
        qkv = (torch.randn(G * T, 3 * H * D, generator=g) * 1.5).to(dev)
        kc = (torch.randn(G, H, TMAX, D, generator=g) * 1.5).to(dev)
        vc = torch.randn(G, H, TMAX, D, generator=g).to(dev)
        inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
        ang = torch.arange(TMAX).float()[:, None] * inv[None]
        _ATT[key] = (qkv, kc, vc, ang.cos().to(dev).contiguous(), ang.sin().to(dev).contiguous())
    return _ATT[key]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("v16", [False, True])
@pytest.mark.parametrize("G,T,H,pos,nsplit", [
    (2, 8, 2, [0, 250], 1),                    # unsplit
    (3, 4, 2, [13, 31, 32], 2),                # rows straddle a multiple of 16 nsplit: the chunk changes inside the launch
    (4, 8, 5, [0, 17, 300, 1499], 6),          # splits that receive no key
    (2, 8, 2, [1532, -1], 4)])                 # rows past the cache; a parked slot
def test_verify_attention_equals_successive_single_row_launches(dev, dt, v16, G, T, H, pos, nsplit):
    """sx_attention_f32 with rope_cos and T > 1 against T successive fused T = 1 calls (call t: row (g, t) at position pos[g] + t, the
    same nsplit / v16 / dtype): torch.equal on the context planes of every in-range row, on the k cache and on the v cache (so every
    other cache row is untouched in both); rows past the cache and parked slots write nothing and stay finite; tiled output == dense."""
    from seedx_amd import ops
    qkv0, kc0, v32, cos, sin = _attn_inputs(dev, G, T, H)
    vc0 = v32.to(dt) if v16 else v32
    scale = 1.0 / math.sqrt(D)
    posd = _i32(pos, dev)
    ka, va = kc0.clone(), vc0.clone()
    ref = torch.zeros((G * T, 2 * H * D), dtype=dt, device=dev)
    for t in range(T):
        rows = qkv0.view(G, T, -1)[:, t].contiguous()
        pt = _i32([p + t if p >= 0 else -1 for p in pos], dev)          # a parked slot stays parked in every call
        y = ops.attention_f32(rows, ka, va, pt, G, 1, H, D, scale, dt, nsplit=nsplit, rope=(cos, sin))
        ref.view(G, T, -1)[:, t] = y
    kb, vb, qb = kc0.clone(), vc0.clone(), qkv0.clone()
    yb = ops.attention_f32(qb, kb, vb, posd, G, T, H, D, scale, dt, nsplit=nsplit, rope=(cos, sin))
    assert torch.equal(qb, qkv0), "the verify form leaves the qkv buffer alone"
    assert torch.isfinite(yb.float()).all()
    inr = torch.tensor([p >= 0 and p + t < TMAX for p in pos for t in range(T)], device=dev)
    assert inr.sum().item() >= 4
    bad = (yb[inr] != ref[inr]).any(dim=1).nonzero().flatten().tolist()
    assert not bad, f"context planes differ in in-range rows {bad} (of {inr.nonzero().flatten().tolist()})"
    assert torch.equal(kb, ka), "k rows"
    assert torch.equal(vb, va), "v rows"
    for gi, p in enumerate(pos):                       # what was written at all: positions pos .. pos + T - 1 inside the cache, nothing else
        m = torch.ones(TMAX, dtype=torch.bool, device=dev)
        if p >= 0:
            m[p:min(p + T, TMAX)] = False
        assert torch.equal(kb[gi][:, m], kc0[gi][:, m]) and torch.equal(vb[gi][:, m], vc0[gi][:, m]), gi
        if p >= 0:
            assert not torch.equal(kb[gi][:, ~m], kc0[gi][:, ~m])
    yt = ops.attention_f32(qkv0.clone(), kc0.clone(), vc0.clone(), posd, G, T, H, D, scale, dt, tiled=True, nsplit=nsplit, rope=(cos, sin))
    assert torch.equal(yt.dense(), yb[:, :H * D].float() + yb[:, H * D:].float())


def test_verify_attention_refuses_the_fp8_cache(dev):
    from seedx_amd import ops
    qkv0, kc0, v32, cos, sin = _attn_inputs(dev, 2, 8, 2)
    with pytest.raises(RuntimeError, match="verify form"):
        ops.attention_f32(qkv0.clone(), kc0.clone(), v32.clone(), _i32([3, 4], dev), 2, 8, 2, D, 0.1, torch.float16, nsplit=2, rope=(cos, sin),
                          kv_emulate=True)


# ---- 2. draft kernel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ngram", [(3, 1), (2, 2), (5, 3)])
def test_draft_kernel_equals_propose_ngram(dev, ngram):
    """Ids from a vocabulary of 4 (matches abound), G = 4, K = 7, lengths 1, 2, 40 and Tmax: the row inputs up to n_draft and n_draft
    itself equal spec.propose_ngram; a second launch has a parked slot and a length past the history."""
    from seedx_amd import ops, spec
    G, K = 4, 7
    T = K + 1
    hist = torch.randint(0, 4, (G, TMAX), generator=torch.Generator().manual_seed(9), dtype=torch.int32)
    hd = hist.to(dev)
    for lengths in ([1, 2, 40, TMAX], [0, 17, TMAX + 1, 333]):
        pos = _i32([L - 1 for L in lengths], dev)
        cur = _i32([int(hist[g, L - 1]) if 1 <= L <= TMAX else 3 for g, L in enumerate(lengths)], dev)
        rows = torch.full((G * T,), -5, dtype=torch.int32, device=dev)
        nd = torch.full((G,), -5, dtype=torch.int32, device=dev)
        ops.spec_draft_ngram(hd, pos, cur, rows, nd, ngram)
        rows, nd = rows.view(G, T).tolist(), nd.tolist()
        for g, L in enumerate(lengths):
            want = spec.propose_ngram(hist[g, :L].tolist(), K, *ngram) if 1 <= L <= TMAX else []
            assert nd[g] == len(want), (g, L, nd[g], want)
            if L >= 1:
                assert rows[g][:1 + len(want)] == [cur[g].item()] + want, (g, L, rows[g], want)
                assert all(0 <= r < 4 for r in rows[g]), "every row input is a valid id"
            else:
                assert rows[g] == [-5] * T, "a parked slot's rows are not touched"


# ---- 3. accept kernel ------------------------------------------------------------------------------------------------------------------
def _accept_case(dev, slots, T, Tmax=64, ld_out=24, eos=7, force_id=401, img=400):
    """One sx_spec_accept launch over hand-made slots against spec.accept: every output array is compared exactly. A slot is a dict
    with cand, draft, n_new, max_new, force_at, pos, live."""
    from seedx_amd import ops, spec
    G = len(slots)
    pad = lambda v, n, x: list(v) + [x] * (n - len(v))
    cand = _i32([c for s in slots for c in pad(s["cand"], T, 3)], dev)
    rows = _i32([c for s in slots for c in [11] + pad(s["draft"], T - 1, 12)], dev)
    n_draft = _i32([len(s["draft"]) for s in slots], dev)
    live = _i32([s.get("live", 1) for s in slots], dev)
    n_new = _i32([s["n_new"] for s in slots], dev)
    max_new = _i32([s["max_new"] for s in slots], dev)
    force_at = _i32([s.get("force_at", -1) for s in slots], dev)
    pos = _i32([s["pos"] if s.get("live", 1) else -1 for s in slots], dev)
    ctx = _i32([s["pos"] + 1 if s.get("live", 1) else 0 for s in slots], dev)
    step = _i32([s["n_new"] if s.get("live", 1) else -1 for s in slots], dev)
    cur = _i32([11] * G, dev)
    out_ids = torch.full((G, ld_out), -1, dtype=torch.int32, device=dev)
    status = torch.full((G, 4), -9, dtype=torch.int32, device=dev)
    hist = torch.full((G, Tmax), -2, dtype=torch.int32, device=dev)
    before = [t.clone() for t in (cur, live, n_new, pos, ctx, step, out_ids, status, hist, rows)]
    ops.spec_accept(cand, rows, n_draft, cur, live, n_new, max_new, force_at, pos, ctx, step, out_ids, status, hist=hist,
                    force_id=force_id, eos_id=eos, img_ids_dev=_i32([img, 401, 402, 465], dev))
    got = [t.tolist() for t in (cur, live, n_new, pos, ctx, step, out_ids, status, hist, rows)]
    counts = []
    for g, s in enumerate(slots):
        want = [t[g].tolist() if t.dim() > 1 else t[g].item() for t in before[:9]]
        w_rows = before[9].view(G, T)[g].tolist()
        if s.get("live", 1):
            em, stopped = spec.accept(s["cand"], s["draft"], s["n_new"], s["max_new"], s.get("force_at", -1), force_id, eos, img)
            n = s["n_new"] + len(em)
            w_out, w_hist = want[6], want[8]
            for t, tok in enumerate(em):
                if s["n_new"] + t < ld_out:
                    w_out[s["n_new"] + t] = tok
                if s["pos"] + 1 + t < Tmax:
                    w_hist[s["pos"] + 1 + t] = tok
            want = [em[-1], 0 if stopped else 1, n, -1 if stopped else s["pos"] + len(em), 0 if stopped else s["pos"] + 1 + len(em),
                    -1 if stopped else n, w_out, [em[-1], 0 if stopped else 1, n, n if stopped else -1], w_hist]
            w_rows[0] = em[-1]
            counts.append(len(em))
        else:
            counts.append(0)
        have = [x[g] for x in got[:9]]
        names = ("cur", "live", "n_new", "pos", "ctx", "step", "out_ids", "status", "hist")
        for nm, h, w in zip(names, have, want):
            assert h == w, (g, nm, h, w, s)
        assert torch.tensor(got[9]).view(G, T)[g].tolist() == w_rows, (g, "rows")
    return counts


def test_accept_kernel_equals_the_python_rule(dev):
    """Crafted candidates and drafts: every emitted count 1 .. 8, EOS mid-run, the budget mid-run, force_at inside the run, <img> inside
    the run, a parked slot, a run that leaves the id log and the history."""
    T = 8
    seq = [20, 21, 22, 23, 24, 25, 26, 27]
    full = dict(n_new=2, max_new=100, pos=9)
    a = [dict(full, cand=seq, draft=seq[:c - 1] + ([99] if c < 8 else [])) for c in (1, 2, 3, 4)]
    b = [dict(full, cand=seq, draft=seq[:c - 1] + ([99] if c < 8 else [])) for c in (5, 6, 7, 8)]
    assert _accept_case(dev, a, T) == [1, 2, 3, 4] and _accept_case(dev, b, T) == [5, 6, 7, 8]
    c = [dict(full, cand=[20, 21, 7, 23, 24, 25, 26, 27], draft=[20, 21, 7, 23, 24, 25, 26]),           # EOS = 7 mid-run
         dict(full, cand=seq, draft=seq[:7], max_new=6),                                                  # budget: 4 more ids
         dict(full, cand=seq, draft=seq[:7], force_at=4),                                                 # force_at inside: 20 21 401
         dict(full, cand=[20, 400, 22, 23, 24, 25, 26, 27], draft=[20, 400, 22, 23, 24, 25, 26])]        # <img> inside the run
    assert _accept_case(dev, c, T) == [3, 4, 3, 2]
    d = [dict(full, cand=seq, draft=seq[:7], live=0),                                                    # parked: nothing read or written
         dict(full, cand=seq, draft=[], n_new=5),                                                        # no draft: the plain slot advance
         dict(full, cand=seq, draft=seq[:7], n_new=20, pos=60),                                          # leaves out_ids (24) and hist (64)
         dict(full, cand=seq, draft=[401] + seq[1:7], force_at=2)]                                       # forced id == the draft: goes on
    assert _accept_case(dev, d, T) == [0, 1, 8, 8]
    assert _accept_case(dev, [dict(full, cand=[5, 6], draft=[5]), dict(full, cand=[5, 6], draft=[4], max_new=3)], 2) == [2, 1]


# ---- 4. / 5. the verify token step -----------------------------------------------------------------------------------------------------
def _llm(dev, dt, G, **kw):
    from seedx_amd.llama import LlamaForCausalLM
    cfg = weights.MINI_LLM
    if "llm" not in _SD:
        _SD["llm"] = weights.llama_sd(cfg)
    m = LlamaForCausalLM(dict(cfg), max_cache_len=128, max_batch=G, precise=True, **kw)
    m.load_state_dict(dict(_SD["llm"]))
    m.eval().to(dev, dtype=dt)
    return m


def _admit(m, st, dev, budget, sampled=()):
    """Prefill G ragged prompts, take the first token, make every slot live. Returns (out_ids, hid, img_ids, prompt lengths)."""
    from seedx_amd import ops
    from seedx_amd.sampling import SamplingParams
    P, G = m._pack(), m.G
    rows = budget + 16
    out_ids = torch.full((G, rows), -1, dtype=torch.int32, device=dev)
    hid = torch.zeros((G, rows, m.H), dtype=torch.float32, device=dev)
    img = _i32(IMG_IDS[:1] + IMG_IDS[1:17] + IMG_IDS[-1:], dev)
    prompts = [[1, 10 + g] + [20 + g + i for i in range(3 + g)] for g in range(G)]
    m.park_slots(range(G), st)
    m._slot_write(P["pos"], range(G), 0)
    m._slot_write(P["ctx"], range(G), 1)
    logits, _ = m.forward_embeds_batch([ops.embedding(_i32(p, dev), P["embed"]) for p in prompts], list(range(G)))
    first = _i32([p[-1] for p in prompts], dev)
    ops.greedy_next_b(logits.contiguous(), m.V, img, first, None, None)
    if st.sampling is not None:
        st.sampling.set_rows(range(G), [SamplingParams(True, 0.9, 20, 0.95, seed=77 + g) if g in sampled else None for g in range(G)])
    P["cur"].copy_(first)
    out_ids[:, 0] = first
    P["step"].fill_(1)
    st.n_new.fill_(1)
    st.max_new.fill_(budget)
    st.force_at.fill_(-1)
    st.live.fill_(1)
    if m.spec_tokens:
        for g, p in enumerate(prompts):
            m.spec_write_history(g, 0, p + [int(first[g])])
        P["spec"]["rows"].view(G, -1)[:, 0] = first
        P["spec"]["n_draft"].zero_()
    return out_ids, hid, img, [len(p) for p in prompts]


def _spec_run(m, dev, budget, drafts=None, sampled=(), use_graph=False):
    """The verify step with draft="given" until every slot has stopped. ``drafts(g, n_new, k)``: the ids slot g feeds behind its
    current token in its k-th step (None: no drafts). Returns ids, hidden states, cache rows below pos, steps and emitted counts."""
    P, G, T = m._pack(), m.G, m.spec_tokens + 1
    st = m.slot_state(force_id=400, eos_id=-1, sampling=bool(sampled))
    out_ids, hid, img, plen = _admit(m, st, dev, budget, sampled)
    S = P["spec"]
    n_new, live, counts, steps = [1] * G, [1] * G, [[] for _ in range(G)], 0
    while any(live):
        rows = S["rows"].view(G, T).clone()
        nd = [0] * G
        for g in range(G):
            d = list(drafts(g, n_new[g], len(counts[g])))[:T - 1] if drafts is not None and live[g] else []
            nd[g] = len(d)
            if d:
                rows[g, 1:1 + len(d)] = _i32(d, dev)
        S["rows"].copy_(rows.view(-1))
        S["n_draft"].copy_(_i32(nd, dev))
        m.decode_step(img, out_ids, hid, use_graph=use_graph, slots=st, spec=True, draft="given")
        steps += 1
        for g, (_, alive, n, _) in enumerate(st.status.tolist()):
            if live[g]:
                counts[g].append(n - n_new[g])
                n_new[g], live[g] = n, alive
        assert steps <= G * budget
    cache = [(P["kc"][:, g, :, :plen[g] + n_new[g] - 1].clone(), P["vc"][:, g, :, :plen[g] + n_new[g] - 1].clone()) for g in range(G)]
    return dict(ids=out_ids.clone(), hid=hid.clone(), n=n_new, cache=cache, steps=steps, counts=counts)


def _oracle_drafts(ids, K, vocab):
    """Drafts cut from a transcript: step k feeds k % (K + 1) correct ids, then one wrong id."""
    def d(g, n_new, k):
        right = [int(x) for x in ids[g][n_new:n_new + k % (K + 1)] if x >= 0]
        nxt = int(ids[g][n_new + len(right)]) if n_new + len(right) < len(ids[g]) else 0
        return right + [(max(nxt, 0) + 1) % vocab]
    return d


def _same_results(a, b, G):
    for g in range(G):
        n = a["n"][g]
        assert b["n"][g] == n
        assert torch.equal(a["ids"][g, :n], b["ids"][g, :n]), (g, a["ids"][g, :n].tolist(), b["ids"][g, :n].tolist())
        assert torch.equal(a["hid"][g, 1:n], b["hid"][g, 1:n]), g
        assert torch.equal(a["cache"][g][0], b["cache"][g][0]) and torch.equal(a["cache"][g][1], b["cache"][g][1]), g


@pytest.mark.parametrize("dt,G,K,sampled", [(torch.float16, 2, 3, ()), (torch.bfloat16, 2, 3, ()), (torch.float16, 4, 7, ()),
                                            (torch.float16, 2, 3, (0, 1)), (torch.float16, 4, 7, (1, 2))])
def test_verify_step_oracle_drafts_change_nothing_but_the_step_count(dev, dt, G, K, sampled):
    """The same model without drafts (A) and with drafts cut from A's transcript — a cycling correct length 0 .. K, then one wrong id
    (B): ids, logged hidden states and the cache rows below pos are torch.equal (both runs launch the same G*T-row GEMVs; the attention
    rows are equal by test 1); B's step count is the simulator's for the emitted counts the drafts promise, and below A's. A against the
    plain slot step of a spec_tokens = 0 model (greedy cases): ids equal, hidden states within 1e-5 relative (the bound
    test_llm_precise_lock_step_batch_above_16 uses between row-block counts). ``sampled``: those slots draw by the seeded rule."""
    from seedx_amd.inflight import simulate_spec
    budget = 22
    m = _llm(dev, dt, G, spec_tokens=K)
    assert m._pack()["spec"]["rows"].numel() == G * (K + 1)
    a = _spec_run(m, dev, budget, None, sampled)
    assert a["steps"] == budget - 1 and all(c == [1] * (budget - 1) for c in a["counts"]) and a["n"] == [budget] * G
    assert (a["ids"][:, :budget] >= 0).all()
    b = _spec_run(m, dev, budget, _oracle_drafts(a["ids"].tolist(), K, m.V), sampled)
    _same_results(a, b, G)
    promised = [[k % (K + 1) + 1 for k in range(64)]] * G
    want = simulate_spec([budget] * G, G, promised)
    assert b["steps"] == want["decode_steps"] < a["steps"], (b["steps"], want["decode_steps"], a["steps"])
    for g in range(G):                                  # the last count of a request is cut at its budget
        assert b["counts"][g][:-1] == promised[g][:len(b["counts"][g]) - 1] and sum(b["counts"][g]) == budget - 1, (g, b["counts"][g])
    print(f"spec step {dt} G={G} K={K} sampled={sampled}: {a['steps']} plain-equivalent steps, {b['steps']} with oracle drafts")
    if sampled:
        return
    # A against the plain slot step of a model built without spec_tokens (greedy rows: a draw may sit on a boundary of its prefix sums,
    # where the 1e-6 between row-block counts could move it)
    p = _llm(dev, dt, G)
    st = p.slot_state(force_id=400, eos_id=-1, sampling=bool(sampled))
    out_ids, hid, img, _ = _admit(p, st, dev, budget, sampled)
    for _ in range(budget - 1):
        p.decode_step(img, out_ids, hid, use_graph=False, slots=st)
    assert st.live.tolist() == [0] * G
    assert torch.equal(out_ids[:, :budget], a["ids"][:, :budget])
    e = relerr(hid[:, 1:budget], a["hid"][:, 1:budget])
    print(f"   verify step without drafts vs the plain slot step: hidden states {e:.2e}")
    assert e < 1e-5


@pytest.mark.parametrize("sampled", [(), (1,)])
def test_verify_step_graph_replay_equals_eager(dev, sampled):
    """Ids and hidden states of the graph-replayed verify step are torch.equal to the eager step's, with oracle drafts; a model with
    spec_tokens still runs (and captures) the plain slot step when the verify step is not asked for."""
    G, K, budget = 2, 3, 14
    m = _llm(dev, torch.float16, G, spec_tokens=K)
    a = _spec_run(m, dev, budget, None, sampled)
    d = _oracle_drafts(a["ids"].tolist(), K, m.V)
    eager = _spec_run(m, dev, budget, d, sampled, use_graph=False)
    graph = _spec_run(m, dev, budget, d, sampled, use_graph=True)
    assert (m._spec_sample_graph if sampled else m._spec_graph) is not None and m._slot_graph is None
    _same_results(eager, graph, G)
    _same_results(a, graph, G)
    assert graph["steps"] == eager["steps"] < a["steps"]
    st = m.slot_state(force_id=400, eos_id=-1, sampling=bool(sampled))
    out_ids, hid, img, _ = _admit(m, st, dev, budget, sampled)
    for _ in range(budget - 1):
        m.decode_step(img, out_ids, hid, use_graph=True, slots=st)
    assert (m._slot_sample_graph if sampled else m._slot_graph) is not None
    assert torch.equal(out_ids[:, :budget], a["ids"][:, :budget])


# ---- 6. the engine ---------------------------------------------------------------------------------------------------------------------
def _agent(dev, dtype, G, **kw):
    from seedx_amd.llama import LlamaForCausalLM
    from seedx_amd.seed_x import ContinuousLVLM
    from seedx_amd.visual_encoder import Resampler
    cfg = weights.MINI_LLM
    if "llm" not in _SD:
        _SD["llm"] = weights.llama_sd(cfg)
    if "agent" not in _SD:
        _SD["agent"] = weights.agent_sd(cfg, VIT, in_grid=4, out_grid=4)
    llm = LlamaForCausalLM(dict(cfg), max_cache_len=512, max_batch=G, precise=True, **kw)
    llm.load_state_dict(dict(_SD["llm"]))
    H = cfg["hidden_size"]
    agent = ContinuousLVLM(llm, Resampler(4, H, 2, kv_dim=VIT), Resampler(4, VIT, 2, kv_dim=H), add_patch_pos=True)
    agent.load_state_dict(_SD["agent"])
    agent.eval().to(dev, dtype=dtype)
    return agent


def test_generate_inflight_speculative_returns_the_same_ids(dev):
    """Five requests on two slots — mixed budgets, one forced image block, one sampled request, prompts that repeat themselves so that
    prompt lookup has something to propose, EOS = an id the plain run is seen to emit: the ids with ``agent.speculative`` are those of
    the same call without it; decode_steps is inflight.simulate_spec's for the emitted counts; once more with prefix_cache."""
    from seedx_amd.inflight import simulate_spec
    agent, tok = _agent(dev, torch.float16, 2, spec_tokens=3), StubTokenizer()
    reqs = []
    for r, b in enumerate([14, 30, 5, 9, 12]):
        ids = [1, 10 + r] + [20 + r, 21 + r, 22 + r] * 3 + [20 + r]
        reqs.append(dict(input_ids=[ids], max_new_tokens=b))
    reqs[1]["force_image_at"] = 2
    reqs[3].update(do_sample=True, temperature=0.9, top_k=30, top_p=0.95, seed=1234)
    solo = agent.generate_inflight(tok, reqs, **KW)
    t0 = solo[0]["generate_ids"].tolist()
    k = max(t0.index(t) for t in set(t0) if t0.index(t) <= 10)
    assert k >= 1, t0
    kw = dict(KW, eos_token_id=t0[k])
    plain = agent.generate_inflight(tok, reqs, **kw)
    assert "spec_steps" not in agent.last_inflight_stats and agent.llm._spec_graph is None
    plain_steps = agent.last_inflight_stats["decode_steps"]
    assert plain[0]["generate_ids"].tolist() == t0[:k + 1] and plain[1]["num_gen_imgs"] == 1
    agent.speculative = True
    for prefix_cache in (False, True):
        agent.prefix_cache = prefix_cache
        got = agent.generate_inflight(tok, reqs, **kw)
        stats = agent.last_inflight_stats
        for r, (a, b) in enumerate(zip(plain, got)):
            assert torch.equal(a["generate_ids"], b["generate_ids"]), (r, a["generate_ids"].tolist(), b["generate_ids"].tolist())
            assert a["num_gen_imgs"] == b["num_gen_imgs"] and a["text"] == b["text"]
            assert b["last_hidden_states"].shape == a["last_hidden_states"].shape
        lengths = [len(x["generate_ids"]) - (17 if x["num_gen_imgs"] else 0) for x in got]      # an image block takes no decode step
        want = simulate_spec(lengths, 2, agent.last_spec_emitted)
        assert stats["decode_steps"] == stats["spec_steps"] == want["decode_steps"], (stats, want)
        assert stats["live_slot_steps"] == want["live_slot_steps"]
        assert stats["spec_emitted_tokens"] == want["emitted_tokens"] == sum(n - 1 for n in lengths)
        assert stats["decode_steps"] <= plain_steps
        print(f"speculative generate_inflight (prefix_cache={prefix_cache}): {stats['decode_steps']} verify steps for "
              f"{stats['spec_emitted_tokens']} tokens ({plain_steps} plain steps)")
    assert agent.llm._spec_sample_graph is not None
