"""Device-side logits controls (sx_next_b_ctl / sx_next_slots_ctl) against the float32 rule seedx_amd.sampling.apply_controls: everything
here is torch.equal or an exact list. The working rows are compared with the numpy rule bit for bit; ids, out_ids, counters, status,
n_kept and p_chosen with the EXISTING tails run on the numpy-edited rows (the same arg-max / draw code on the same bits); the LP
records with sx_token_logprobs of the RAW rows. Inputs are normal-range N(0, 3) logits, for which one IEEE rounding per operation is
all the rule needs. Counts: a controlled row counts the id it emits; a row with on = 0 and a parked slot count nothing (they run the
uncontrolled path and leave the table alone)."""
import numpy as np
import pytest
import torch

from seedx_amd.sampling import ControlParams, apply_controls, count_words
from tests.test_inflight_gpu import IMG_IDS, KW, _i32, _req
from tests.test_logprobs_gpu import PROMPT, Rec, _agent, _same
from tests.test_models_gpu import StubTokenizer
from tests.test_sampling_gpu import Params

EOS = 7
WIDTHS = [(500, 512), (1031, 1088), (32330, 32384)]
NINF = float("-inf")


class Ctl:
    """A control state as ops takes it (what llama.ControlState holds), from per-row ControlParams (None: on = 0) and count words."""

    def __init__(self, dev, params, counts, ld):
        G = len(params)
        on = [p is not None for p in params]
        f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
        self.on = _i32([int(o) for o in on], dev)
        self.counts = torch.zeros((G, ld), dtype=torch.int32, device=dev)
        self.counts[:, :counts.shape[1]] = torch.from_numpy(counts).to(dev)
        self.work = torch.full((G, ld), -123.0, dtype=torch.float32, device=dev)
        self.rep = f32([p.repetition_penalty if o else 1.0 for p, o in zip(params, on)])
        self.rep_inv = f32([p.rep_inv if o else 1.0 for p, o in zip(params, on)])
        self.presence = f32([p.presence_penalty if o else 0.0 for p, o in zip(params, on)])
        self.frequency = f32([p.frequency_penalty if o else 0.0 for p, o in zip(params, on)])
        self.min_new = _i32([p.min_new_tokens if o else 0 for p, o in zip(params, on)], dev)
        ids = [[i for i, _ in p.logit_bias] + [-1] * (16 - len(p.logit_bias)) if o else [-1] * 16 for p, o in zip(params, on)]
        bias = [[b for _, b in p.logit_bias] + [0.0] * (16 - len(p.logit_bias)) if o else [0.0] * 16 for p, o in zip(params, on)]
        self.bias_ids, self.bias = _i32(ids, dev), f32(bias)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _zeroed(row, prev):
    """The image rule's edit of a row (numpy, in place): nothing inside the chain, else the image columns zeroed."""
    if prev not in IMG_IDS[:-1]:
        row[IMG_IDS[1:]] = 0.0
    return row


G1 = 24


def _case(V, ld, seed=0):
    """24 rows: each control alone, all together, a -inf bias on the row's arg-max, min_new masking an EOS that is the arg-max (and one
    past min_new), a chain row, an on = 0 row, controls on image columns, 16 bias entries, and random mixes."""
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(100 + seed)
    logits = torch.randn(G1, ld, generator=g) * 3
    logits[:, V:] = float("nan")
    logits[7, EOS] = logits[8, EOS] = 50.0
    prev = [11 + r for r in range(G1)]
    prev[10] = 431                                                           # inside the chain: 432 is forced whatever the controls say
    tok = [int(t) for t in rng.integers(0, 6, size=G1)]
    tok[7], tok[8] = 2, 5
    counts = np.stack([count_words(V, rng.integers(0, V, size=40), rng.integers(0, min(V, 600), size=int(rng.integers(0, 60)))) for _ in range(G1)])
    counts[12, 401:466] += 3                                                 # counts on image columns: the zeroing overwrites them
    raw = logits[:, :V].numpy()
    top6 = int(np.argmax(_zeroed(raw[6].copy(), prev[6])))
    many = {int(i): float(b) for i, b in zip(rng.choice(V, 16, replace=False), rng.normal(size=16) * 4)}
    P = ControlParams
    params = [P(repetition_penalty=1.3), P(repetition_penalty=0.8), P(presence_penalty=0.5), P(frequency_penalty=0.25),
              P(presence_penalty=-0.3, frequency_penalty=-0.1), P(logit_bias={5: 2.0, 9: -1.5}), P(logit_bias={top6: NINF}),
              P(min_new_tokens=5), P(min_new_tokens=5),
              P(repetition_penalty=1.7, presence_penalty=0.4, frequency_penalty=0.15, logit_bias={3: 1.25, 33: NINF, EOS: 9.0}, min_new_tokens=4),
              P(repetition_penalty=1.7, presence_penalty=0.4, frequency_penalty=0.15, logit_bias={432: NINF, 3: 2.0}, min_new_tokens=4),
              None, P(repetition_penalty=2.0, frequency_penalty=0.5, logit_bias={410: 30.0, 465: NINF}), P(logit_bias=many)]
    while len(params) < G1:
        params.append(P(repetition_penalty=float(rng.uniform(0.5, 2.0)), presence_penalty=float(rng.normal() * 0.5),
                        frequency_penalty=float(rng.normal() * 0.2),
                        logit_bias={int(i): float(rng.normal() * 3) for i in rng.choice(V, int(rng.integers(0, 5)), replace=False)},
                        min_new_tokens=int(rng.integers(0, 6))))
    return logits, prev, tok, counts, params, top6


def _edited(logits, V, counts, params, tok, eos):
    """The rows the id functions see: apply_controls on the controlled rows (before the image rule), the raw row elsewhere."""
    out = logits.clone()
    for r, p in enumerate(params):
        if p is not None:
            out[r, :V] = torch.from_numpy(apply_controls(logits[r, :V].numpy(), counts[r], p, eos_id=eos, token_index=tok[r]))
    return out


def _sample_params(dev, G, seed=3):
    rng = np.random.default_rng(seed)
    do = [int(r % 4 != 1) for r in range(G)]                                # every fourth row greedy
    return Params(dev, do, [float(t) for t in rng.uniform(0.6, 1.4, size=G)], [int(k) for k in rng.choice([0, 5, 50], size=G)],
                  [float(p) for p in rng.uniform(0.3, 1.0, size=G)], [int(s) for s in rng.integers(0, 2 ** 62, size=G)])


@pytest.mark.gpu
@pytest.mark.parametrize("V,ld,sampled,lp_n", [(v, ld, s, n) for (v, ld) in WIDTHS for s, n in ((False, None), (True, None), (True, 3))]
                         + [(500, 512, False, 8), (40000, 40064, False, None)])
def test_lockstep_form(dev, V, ld, sampled, lp_n):
    """One launch over 24 rows. work[:, :V] = apply_controls then the image zeroing; the logits rows of controlled rows are untouched,
    the on = 0 row is zeroed in place as ever; ids / out_ids / n_kept / p_chosen equal the existing tails on the numpy-edited rows; the
    counts grow by one at the emitted id of every controlled row; with ``lp_n`` the records are sx_token_logprobs of the RAW rows."""
    from seedx_amd import ops
    logits, prev, tok, counts, params, top6 = _case(V, ld)
    img, rows = _i32(IMG_IDS, dev), 8
    edited = _edited(logits, V, counts, params, tok, EOS)
    # ---- the reference: the existing tail on the edited rows
    ref_l, ref_cur = edited.to(dev), _i32(prev, dev)
    ref_out = torch.full((G1, rows), -1, dtype=torch.int32, device=dev)
    step = _i32(tok, dev)
    if sampled:
        rp = _sample_params(dev, G1)
        ops.sample_next_b(ref_l, V, img, ref_cur, ref_out, step, rp, token_index=step, n_kept=rp.n_kept, p_chosen=rp.p_chosen)
    else:
        ops.greedy_next_b(ref_l, V, img, ref_cur, ref_out, step)
    # ---- the controlled tail on the raw rows
    dl, cur = logits.to(dev), _i32(prev, dev)
    out = torch.full((G1, rows), -1, dtype=torch.int32, device=dev)
    ctl = Ctl(dev, params, counts, ld)
    sp = _sample_params(dev, G1) if sampled else None
    rec = Rec(dev, [int(r % 5 != 4) for r in range(G1)], rows, lp_n) if lp_n is not None else None
    ops.next_b_ctl(dl, V, img, cur, out, step, ctl, sample=sp, lp=rec, token_index=step, eos_id=EOS,
                   **(dict(n_kept=sp.n_kept, p_chosen=sp.p_chosen) if sampled else {}))
    torch.cuda.synchronize()
    emitted = cur.tolist()
    assert torch.equal(cur, ref_cur) and torch.equal(out, ref_out)
    if sampled:
        assert torch.equal(sp.n_kept, rp.n_kept) and torch.equal(_bits(sp.p_chosen), _bits(rp.p_chosen))
        assert (sp.n_kept > 1).any() and (sp.n_kept == -1).any()             # something was drawn, something was not
    else:
        assert emitted[6] != top6 and emitted[7] != EOS and emitted[8] == EOS
    assert emitted[10] == 432
    on = [p is not None for p in params]
    for r in range(G1):
        want = _zeroed(edited[r, :V].numpy().copy(), prev[r])
        if on[r]:
            assert torch.equal(_bits(ctl.work[r, :V].cpu()), _bits(torch.from_numpy(want))), r
            assert torch.equal(_bits(dl[r].cpu()), _bits(logits[r])), r      # the logits row, padding included: as lm_head wrote it
        else:
            assert torch.equal(_bits(dl[r, :V].cpu()), _bits(torch.from_numpy(want)))     # today's in-place zeroing
            assert (ctl.work[r] == -123.0).all()
    exp_counts = counts.copy()
    for r in range(G1):
        if on[r]:
            exp_counts[r, emitted[r]] += 1
    assert np.array_equal(ctl.counts[:, :V].cpu().numpy(), exp_counts) and (ctl.counts[:, V:] == 0).all()
    assert (ctl.work[12, 401:466] == 0).all() and ctl.work[9, 33].item() == NINF
    if rec is not None:
        c, ti, tv = ops.token_logprobs(logits.to(dev), V, cur, lp_n)
        for r in range(G1):
            got = (rec.chosen[r, tok[r]], rec.top_ids[r, tok[r]], rec.top[r, tok[r]])
            if r % 5 == 4:
                assert (rec.chosen[r] == -7.0).all() and (rec.top_ids[r] == -9).all()
            elif r == 10:
                assert got[0].isnan() and (got[1] == -1).all() and got[2].isnan().all()
            else:
                assert torch.equal(_bits(got[0]), _bits(c[r])) and torch.equal(got[1], ti[r]) and torch.equal(_bits(got[2]), _bits(tv[r])), r


G2 = 10


@pytest.mark.gpu
@pytest.mark.parametrize("V,ld", [(500, 512), (32330, 32384)])
@pytest.mark.parametrize("sampled,lp_n", [(False, None), (True, None), (False, 2), (True, 8)], ids=["greedy", "sampled", "greedy-lp", "sampled-lp"])
def test_slot_form(dev, V, ld, sampled, lp_n):
    """Ten slots: live and controlled, one parked, one live with on = 0, one whose id is replaced by force_id (counted: the FORCED id), one
    that stops on its budget, one that stops on EOS (min_new behind it), one whose EOS is masked. Counters, ids and status equal the plain
    slot tail on the numpy-edited rows; counts = before + 1 at the emitted id of live controlled slots; parked and on = 0 slots leave
    counts and working rows alone; LP records are those of the RAW rows."""
    from seedx_amd import ops
    rng = np.random.default_rng(5)
    g = torch.Generator().manual_seed(55)
    logits = torch.randn(G2, ld, generator=g) * 3
    logits[:, V:] = float("nan")
    logits[6, EOS] = logits[7, EOS] = 60.0
    P = ControlParams
    params = [P(repetition_penalty=1.4, frequency_penalty=0.3), P(presence_penalty=0.7, logit_bias={12: NINF}), P(repetition_penalty=1.2),
              None, P(frequency_penalty=0.2, logit_bias={3: 4.0}), P(repetition_penalty=0.9, min_new_tokens=2), P(min_new_tokens=3),
              P(min_new_tokens=9, presence_penalty=0.1), P(repetition_penalty=1.6, presence_penalty=0.2, frequency_penalty=0.1, logit_bias={8: -2.0}),
              P(logit_bias={20: 1.0})]
    live = [1, 1, 0, 1, 1, 1, 1, 1, 1, 1]
    stepv = [0, 3, 2, 5, 1, 4, 3, 2, 6, 2]
    n_new = [1, 4, 3, 6, 2, 5, 4, 3, 7, 3]
    max_new = [100, 100, 100, 100, 100, 6, 100, 100, 100, 100]               # slot 5 reaches its budget
    force_at = [-1, 4, -1, -1, -1, -1, -1, -1, -1, -1]                       # slot 1: the id is replaced by force_id = 400
    prev = [11, 12, 13, 14, 431, 16, 17, 18, 19, 20]                         # slot 4 is inside the image chain
    pos = [20 + r for r in range(G2)]
    counts = np.stack([count_words(V, rng.integers(0, V, size=30), rng.integers(0, V, size=int(rng.integers(1, 40)))) for _ in range(G2)])
    edited = _edited(logits, V, counts, params, stepv, EOS)
    img = _i32(IMG_IDS, dev)

    def run(rows_t, ctl, rec):
        t = dict(cur=_i32(prev, dev), live=_i32(live, dev), n_new=_i32(n_new, dev), max_new=_i32(max_new, dev), force_at=_i32(force_at, dev),
                 pos=_i32(pos, dev), ctx=_i32([p + 1 for p in pos], dev), step=_i32(stepv, dev))
        out = torch.full((G2, 8), -1, dtype=torch.int32, device=dev)
        status = torch.full((G2, 4), -5, dtype=torch.int32, device=dev)
        sp = _sample_params(dev, G2, seed=9) if sampled else None
        skw = dict(n_kept=sp.n_kept, p_chosen=sp.p_chosen) if sampled else {}
        args = (rows_t, V, img, t["cur"], t["live"], t["n_new"], t["max_new"], t["force_at"], t["pos"], t["ctx"], t["step"], out, status)
        if ctl is not None:
            ops.next_slots_ctl(*args, ctl, sample=sp, lp=rec, force_id=400, eos_id=EOS, **skw)
        elif sampled:
            ops.sample_next_slots(*args, sp, force_id=400, eos_id=EOS, **skw)
        else:
            ops.greedy_next_slots(*args, force_id=400, eos_id=EOS)
        torch.cuda.synchronize()
        t.update(out=out, status=status)
        if sampled:
            t.update(n_kept=sp.n_kept, p_chosen=_bits(sp.p_chosen))
        return t
    ref = run(edited.to(dev), None, None)
    dl = logits.to(dev)
    ctl = Ctl(dev, params, counts, ld)
    rec = Rec(dev, [1] * G2, 8, lp_n) if lp_n is not None else None
    got = run(dl, ctl, rec)
    for k in ref:
        assert torch.equal(ref[k], got[k]), k
    status = got["status"].tolist()
    assert status[2] == [-5] * 4 and status[1][0] == 400 and status[4][0] == 432 and status[5][1] == 0 and status[5][3] == 6
    if not sampled:
        assert status[6][0] == EOS and status[6][1] == 0 and status[7][0] != EOS and status[7][1] == 1
    exp = counts.copy()
    for r in range(G2):
        if live[r] and params[r] is not None:
            exp[r, status[r][0]] += 1                                        # the emitted id, slot 1's forced one included
    assert np.array_equal(ctl.counts[:, :V].cpu().numpy(), exp)
    for r in (2, 3):                                                         # parked / on = 0: no working row
        assert (ctl.work[r] == -123.0).all()
    assert torch.equal(_bits(dl[2].cpu()), _bits(logits[2]))                 # parked: the logits row untouched
    assert torch.equal(_bits(dl[3, :V].cpu()), _bits(torch.from_numpy(_zeroed(logits[3, :V].numpy().copy(), prev[3]))))
    for r in range(G2):
        if live[r] and params[r] is not None:
            assert torch.equal(_bits(dl[r].cpu()), _bits(logits[r])), r
            assert torch.equal(_bits(ctl.work[r, :V].cpu()), _bits(torch.from_numpy(_zeroed(edited[r, :V].numpy().copy(), prev[r])))), r
    if rec is not None:
        emitted = [status[r][0] if live[r] else 0 for r in range(G2)]
        c, ti, tv = ops.token_logprobs(logits.to(dev), V, _i32(emitted, dev), lp_n)
        for r in range(G2):
            got_r = (rec.chosen[r, stepv[r]], rec.top_ids[r, stepv[r]], rec.top[r, stepv[r]])
            if not live[r]:
                assert (rec.chosen[r] == -7.0).all()
            elif r == 4:
                assert got_r[0].isnan() and (got_r[1] == -1).all()
            else:
                assert torch.equal(_bits(got_r[0]), _bits(c[r])) and torch.equal(got_r[1], ti[r]) and torch.equal(_bits(got_r[2]), _bits(tv[r])), r


# ---- model -------------------------------------------------------------------------------------------------------------------------
def _slot_run(dev, agent, controls, use_graph, steps=11):
    """Three slots of the miniature through prefill + ``steps`` slot steps. ``controls``: per-slot ControlParams / None, or None for a
    slot state without a ControlState. Returns (out_ids, hid, counts or None)."""
    from seedx_amd import ops
    llm = agent.llm
    llm.reset()
    P = llm._pack()
    G, rows = 3, 16
    img = _i32(IMG_IDS[:1] + IMG_IDS[1:17] + IMG_IDS[-1:], dev)
    st = llm.slot_state(force_id=400, eos_id=-1, **(dict(controls=True) if controls is not None else {}))
    out_ids = torch.full((G, rows), -1, dtype=torch.int32, device=dev)
    hid = torch.zeros((G, rows, llm.H), dtype=torch.float32, device=dev)
    prompts = [[1, 10 + g] + [20 + g + i for i in range(3 + g)] for g in range(G)]
    xs = [ops.embedding(_i32(p, dev), P["embed"]) for p in prompts]
    llm._slot_write(P["pos"], range(G), 0)
    llm._slot_write(P["ctx"], range(G), 1)
    logits, _ = llm.forward_embeds_batch(xs, list(range(G)))
    first = _i32([p[-1] for p in prompts], dev)
    if controls is not None:
        cs = st.controls
        assert cs is not None and cs.counts.shape == (G, llm.Vpad)
        cs.set_rows(range(G), controls, prompts)
        zero = torch.zeros(G, dtype=torch.int32, device=dev)
        ops.next_b_ctl(logits.contiguous(), llm.V, img, first, None, zero, cs.gather(range(G)), token_index=zero)
        own = [g for g in range(G) if controls[g] is not None]
        cs.count(own, [first[g].item() for g in own])
    else:
        assert st.controls is None
        ops.greedy_next_b(logits.contiguous(), llm.V, img, first, None, None)
    P["cur"].copy_(first)
    out_ids[:, 0] = first
    P["step"].fill_(1)
    st.n_new.fill_(1)
    st.max_new.fill_(100)
    st.live.fill_(1)
    for _ in range(steps):
        llm.decode_step(img, out_ids, hid, use_graph=use_graph, slots=st)
    torch.cuda.synchronize()
    res = out_ids.clone(), hid.clone(), (st.controls.counts.clone() if controls is not None else None)
    llm.reset()
    return res


@pytest.mark.gpu
def test_model_eager_equals_graph_and_counts_are_bincounts(dev):
    agent = _agent(dev, torch.float16, 3)
    llm = agent.llm
    controls = [ControlParams(repetition_penalty=1.5, frequency_penalty=0.3), None, ControlParams(presence_penalty=0.8, logit_bias={30: NINF, 31: 1.0})]
    plain = _slot_run(dev, agent, None, True)
    assert llm._slot_graph is not None and llm._slot_graph_ctl is None
    eager = _slot_run(dev, agent, controls, False)
    assert llm._slot_graph_ctl is None
    graph = _slot_run(dev, agent, controls, True)
    assert llm._slot_graph_ctl is not None
    for a, b in zip(eager, graph):
        assert torch.equal(a, b)
    ids, _, counts = graph
    assert (ids[:, :12] >= 0).all() and (ids[:, 12:] == -1).all()
    for g in (0, 2):
        assert torch.equal(counts[g, :llm.V].cpu() & 0xFFFFFF, torch.bincount(ids[g, :12].cpu().long(), minlength=llm.V).int())
        marked = sorted(torch.nonzero(counts[g] & (1 << 30)).flatten().tolist())
        assert marked == sorted({1, 10 + g} | {20 + g + i for i in range(3 + g)})
    assert (counts[1] == 0).all()                                            # the uncontrolled slot: nothing marked, nothing counted
    assert torch.equal(ids[1], plain[0][1]) and torch.equal(graph[1][1], plain[1][1])     # ... and the ids / states of a model without a state
    assert 30 not in ids[2].tolist()
    assert not torch.equal(ids[0], plain[0][0]) or not torch.equal(ids[2], plain[0][2])   # the controls did something


# ---- engines -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_engines(dev):
    tok, n = StubTokenizer(), 12
    a3 = _agent(dev, torch.float16, 3)
    others = [_req(1, n), _req(2, n)]
    run3 = lambda req, **kw: a3.generate_batch(tok, [req] + others, max_new_tokens=n, **dict(KW, **kw))
    base = run3(dict(input_ids=[PROMPT], logprobs=2))[0]
    b = base["generate_ids"].tolist()
    assert len(b) == n and "controls" not in base and a3.llm._graph_lp is not None and a3.llm._graph_lp_ctl is None
    assert base["logprobs"]["top_ids"][0, 0].item() == b[0]
    runner_up = base["logprobs"]["top_ids"][0, 1].item()
    banned = run3(dict(input_ids=[PROMPT], logit_bias={b[0]: NINF}))[0]
    assert banned["generate_ids"][0].item() == runner_up and banned["controls"]["logit_bias"] == {b[0]: NINF}
    assert a3.llm._graph_ctl is not None
    stop = b.index(b[3]) + 1                                                  # 4 unless the 4th id occurred before
    eos = run3(dict(input_ids=[PROMPT]), eos_token_id=b[3])[0]
    assert eos["generate_ids"].tolist() == b[:stop]
    late = run3(dict(input_ids=[PROMPT], min_new_tokens=10), eos_token_id=b[3])[0]["generate_ids"].tolist()
    assert late[:stop - 1] == b[:stop - 1] and len(late) >= 10 and b[3] not in late[:10]
    # ---- one controlled request through the three engines
    ctl = dict(repetition_penalty=1.3, frequency_penalty=0.2, presence_penalty=0.1, logit_bias={b[0]: NINF, b[1]: -1.0})
    batch = run3(dict(input_ids=[PROMPT], **ctl))[0]
    want = batch["generate_ids"]
    assert want.tolist() != b and batch["controls"]["repetition_penalty"] == 1.3
    a1 = _agent(dev, torch.float16, 1)
    single = a1.generate(tok, input_ids=[PROMPT], max_new_tokens=n, **ctl, **KW)
    assert torch.equal(single["generate_ids"], want) and "controls" in single
    assert "controls" not in a1.generate(tok, input_ids=[PROMPT], max_new_tokens=n, **KW)
    queue = [_req(0, 9), dict(input_ids=[PROMPT], max_new_tokens=n), _req(2, 7), _req(3, 10), _req(4, 6)]
    queue[0].update(do_sample=True, top_p=0.9, seed=11)
    queue[2]["logprobs"] = 2
    quiet = a3.generate_inflight(tok, queue, **KW)
    assert a3.llm._slot_sample_graph_lp is not None and a3.llm._slot_sample_graph_lp_ctl is None
    busy_q = [dict(q) for q in queue]
    busy_q[1].update(ctl)
    busy = a3.generate_inflight(tok, busy_q, **KW)
    assert a3.llm._slot_sample_graph_lp_ctl is not None
    assert torch.equal(busy[1]["generate_ids"], want) and busy[1]["controls"] == batch["controls"]
    for r in (0, 2, 3, 4):
        assert torch.equal(quiet[r]["generate_ids"], busy[r]["generate_ids"]), r
        assert torch.equal(quiet[r]["last_hidden_states"], busy[r]["last_hidden_states"]), r
        assert "controls" not in busy[r]
    assert all(_same(quiet[2]["logprobs"][k].float(), busy[2]["logprobs"][k].float()) for k in ("token_logprobs", "top_ids", "top_logprobs"))
    assert torch.equal(quiet[1]["generate_ids"], torch.tensor(b))


@pytest.mark.gpu
def test_refusals_on_the_device_side(dev):
    """decode_step refuses a second control state beside a slot state's, and ops refuses a working buffer that is not the logits' shape."""
    from seedx_amd import ops
    agent = _agent(dev, torch.float16, 3)
    llm = agent.llm
    st = llm.slot_state(force_id=400, controls=True)
    with pytest.raises(ValueError, match="a slot state carries its own control state"):
        llm.decode_step(None, None, None, slots=st, controls=llm.control_state())
    logits = torch.zeros((2, 512), device=dev)
    ctl = Ctl(dev, [ControlParams(repetition_penalty=1.1)] * 2, np.zeros((2, 500), np.int32), 576)
    with pytest.raises(AssertionError, match="work is fp32"):
        ops.next_b_ctl(logits, 500, _i32(IMG_IDS, dev), _i32([1, 2], dev), None, _i32([0, 0], dev), ctl)
    llm.reset()
