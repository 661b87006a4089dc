"""Token log-probabilities on the GPU: sx_token_logprobs against the fp64 rule (seedx_amd.sampling.token_logprobs), the bits of a record
(any slot, any G, all three entry points), the LP decode tail against the tail without it (everything but the record is torch.equal),
the LP token step of LlamaForCausalLM, ContinuousLVLM with ``"logprobs"`` (lock step and in flight) and ContinuousLVLM.score.

The bound on a value. With m = max x (exact) the device computes lp = (x_v - m) - logf(S), S = sum expf(x_i - m), in fp32 (u = 2^-24):
  * d_i = fl(x_i - m) has error <= u |x_i - m|; expf turns it into a relative error of e_i = exp(d_i) of the same size, and expf itself
    adds <= 2 u relative (under the TU's fast-math flags its argument scaling adds another u |x_i - m|);
  * the sum is 32 sequential + 6 butterfly + 4 tree additions deep: <= 42 u relative on top. The relative error of S is therefore at most
    u (44 + 2 E_p|x - m|) with p the softmax, and E_p|x - m| = log S - H(p) <= ln V <= 10.4: below 65 u;
  * log S inherits that as an absolute error, logf adds <= 2 u log S <= 21 u (1 <= S <= V);
  * the two subtractions add u |x_v - m| / 2 + u |lp| / 2, and |x_v - m| <= |lp| + ln V.
Sum: about u (65 + 21 + 6 + |lp|) = u (92 + |lp|). Asserted: u (96 + |lp|), tighter than the u (128 + 4 |lp|) the feature was specified
with. Measured on an MI355X: at most 0.35 of the asserted bound (3.8e-6 at |lp| ~ 104, the rounding of the last subtraction)."""
import numpy as np
import pytest
import torch

from oracle import weights
from tests.test_inflight_gpu import IMG_IDS, KW, _i32, _req
from tests.test_models_gpu import StubTokenizer

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NEG, IDS = -7.0, -9                              # sentinels of the record buffers


def bound(ref):
    return U * (96 + np.abs(ref))                # the derivation above, rounded up; never wider than the issue's u (128 + 4 |lp|)


def rule(rows, targets, n_top):
    from seedx_amd.sampling import token_logprobs
    return token_logprobs(np.asarray(rows, dtype=np.float32), targets, n_top)


def check_values(dev_vals, ref, what):
    """|device - fp64| within the bound where the rule is finite; -inf and NaN in the same places."""
    got = np.asarray(dev_vals, dtype=np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), what
    err = np.abs(got[fin] - ref[fin]) / bound(ref[fin])
    worst = float(err.max()) if err.size else 0.0
    print(f"{what}: max error / bound = {worst:.3f}, max abs error = {float(np.abs(got[fin] - ref[fin]).max()) if err.size else 0.0:.3e}")
    assert worst <= 1.0, (what, worst)


class Rec:
    """A logprob state as ops takes it (what llama.LogprobState holds), sentinel filled."""

    def __init__(self, dev, want, rows, n_top):
        G = len(want)
        self.n_top, self.want = n_top, _i32(want, dev)
        self.chosen = torch.full((G, rows), NEG, dtype=torch.float32, device=dev)
        self.top_ids = torch.full((G, rows, n_top), IDS, dtype=torch.int32, device=dev)
        self.top = torch.full((G, rows, n_top), NEG, dtype=torch.float32, device=dev)


# ---- kernel against the rule -------------------------------------------------------------------------------------------------------
def _rows(V, R=32, seed=0):
    """R rows of V columns: random, all equal, one column 100 above the rest, ties at the top, -inf columns, magnitudes near 3e4."""
    rng = np.random.default_rng(seed + V)
    x = (rng.normal(size=(R, V)) * 4).astype(np.float32)
    for r in range(R):
        kind = r % 6
        if kind == 1:
            x[r] = np.float32(rng.normal() * 10)
        elif kind == 2:
            x[r, rng.integers(V)] = x[r].max() + 100
        elif kind == 3:
            x[r, rng.integers(V, size=3)] = x[r].max() + 1
        elif kind == 4:
            x[r, rng.random(V) < 0.5] = -np.inf
            x[r, rng.integers(V)] = 1.5                                   # never a row of -inf only
        elif kind == 5:
            x[r] = (3e4 + rng.normal(size=V) * 3).astype(np.float32) * (1 if r % 12 == 5 else -1)
    t = rng.integers(V, size=R)
    for r in range(4, R, 12):                                             # a -inf target
        hit = np.nonzero(np.isinf(x[r]))[0]
        if hit.size:
            t[r] = hit[0]
    return x, t


@pytest.mark.parametrize("V", [1, 5, 63, 1024, 1025, 32330, 32768])
def test_kernel_against_rule(dev, V):
    """rows in {1, 3, 32} x n_top in {0, 3, 8}, ld > vocab with NaN in the padding: ids equal the rule's exactly, values within the bound,
    -inf where the rule has -inf. The fp64 reference is computed once per vocab (a shorter top list is a prefix of a longer one)."""
    from seedx_amd import ops
    x, t = _rows(V)
    ld = V + 13
    host = np.full((32, ld), np.nan, dtype=np.float32)
    host[:, :V] = x
    logits, targets = torch.from_numpy(host).to(dev), _i32(t.tolist(), dev)
    ref_c, ref_i, ref_t = rule(x, t, 8)
    assert (V < 63 or np.isneginf(ref_c).any()) and np.isfinite(ref_c).sum() >= 26
    for R in (1, 3, 32):
        for n in (0, 3, 8):
            chosen, ids, top = ops.token_logprobs(logits[:R], V, targets[:R], n)
            assert np.array_equal(ids.cpu().numpy(), ref_i[:R, :n]), (V, R, n)
            check_values(chosen.cpu().numpy(), ref_c[:R], f"V={V} R={R} n_top={n} chosen")
            if n:
                check_values(top.cpu().numpy(), ref_t[:R, :n], f"V={V} R={R} n_top={n} top")


def test_kernel_nan_row_and_bad_target(dev):
    from seedx_amd import ops
    x = torch.randn(3, 700, device=dev)
    x[1, 650] = float("nan")
    chosen, ids, top = ops.token_logprobs(x, 700, _i32([5, 5, 700], dev), 4)
    assert torch.isnan(chosen[1:]).all() and torch.isfinite(chosen[0]) and ids[1].tolist() == [-1] * 4 and torch.isnan(top[1]).all()
    assert torch.isfinite(top[2]).all() and (ids[2] >= 0).all()                # a target outside the row: only the chosen value is NaN
    chosen, _, _ = ops.token_logprobs(x, 600, _i32([5, 5, 5], dev), 0)        # the NaN column lies past vocab: never read
    assert torch.isfinite(chosen).all()


# ---- the tail --------------------------------------------------------------------------------------------------------------------
G9, OUT_ROWS, VOC = 9, 6, 500


def _tail_inputs(dev):
    g = torch.Generator().manual_seed(21)
    logits = (torch.randn(G9, 512, generator=g) * 3).to(dev)
    logits[:, 401:465] += 6.0
    logits[0, 401:466] += 50.0                    # row 0: the image columns hold the largest raw values
    logits[1, 77] = 40.0
    logits[8] = -3.0 - logits[8].abs()            # row 8: every free column below 0, so a ZEROED image column wins the arg-max
    logits[8, 401:466] = -5.0
    logits[:, VOC:] = float("nan")
    return dict(logits=logits, cur=_i32([11, 12, 400, 431, 13, 14, 15, 16, 17], dev), live=_i32([1, 1, 1, 1, 0, 1, 1, 1, 1], dev),
                want=[1, 1, 1, 1, 1, 0, 1, 1, 1], step=_i32([0, 3, 2, 5, 1, 4, -1, OUT_ROWS, 2], dev),
                n_new=_i32([1, 4, 3, 6, 2, 5, 7, 7, 3], dev), max_new=_i32([100, 100, 100, 100, 100, 100, 100, 100, 4], dev),
                force_at=_i32([-1, 4, -1, -1, -1, -1, -1, -1, -1], dev), pos=_i32([20, 21, 22, 23, 24, 25, 26, 27, 28], dev))


def _sampling(dev):
    from tests.test_sampling_gpu import Params
    return Params(dev, [0, 1, 1, 0, 1, 1, 1, 0, 0], [1.0] * G9, [50] * G9, [0.9] * G9, [g * 131 + 7 for g in range(G9)])


def _run_tail(dev, slots, sampled, lp_n):
    """One launch of the tail on fresh copies of the same inputs; lp_n None: the entry point without the record. Returns every tensor
    the launch may write (and the raw logits)."""
    from seedx_amd import ops
    d = _tail_inputs(dev)
    raw, img = d["logits"].clone(), _i32(IMG_IDS, dev)
    out_ids = torch.full((G9, OUT_ROWS), -1, dtype=torch.int32, device=dev)
    status = torch.full((G9, 4), -5, dtype=torch.int32, device=dev)
    ctx = d["pos"] + 1
    par = _sampling(dev) if sampled else None
    rec = Rec(dev, d["want"], OUT_ROWS, lp_n) if lp_n is not None else None
    skw = dict(n_kept=par.n_kept, p_chosen=par.p_chosen) if sampled else {}
    if slots:
        args = (d["logits"], VOC, img, d["cur"], d["live"], d["n_new"], d["max_new"], d["force_at"], d["pos"], ctx, d["step"], out_ids, status)
        if rec is not None:
            ops.next_slots_lp(*args, rec, par, force_id=400, eos_id=-1, **skw)
        elif sampled:
            ops.sample_next_slots(*args, par, force_id=400, eos_id=-1, **skw)
        else:
            ops.greedy_next_slots(*args, force_id=400, eos_id=-1)
    else:
        tok = d["n_new"].clone()
        if rec is not None:
            ops.next_b_lp(d["logits"], VOC, img, d["cur"], out_ids, d["step"], rec, par, token_index=tok, **skw)
        elif sampled:
            ops.sample_next_b(d["logits"], VOC, img, d["cur"], out_ids, d["step"], par, token_index=tok, **skw)
        else:
            ops.greedy_next_b(d["logits"], VOC, img, d["cur"], out_ids, d["step"])
    torch.cuda.synchronize()
    res = dict(logits=d["logits"][:, :VOC], cur=d["cur"], live=d["live"], n_new=d["n_new"], pos=d["pos"], ctx=ctx, step=d["step"],
               out_ids=out_ids, status=status)
    if sampled:
        res.update(n_kept=par.n_kept, p_chosen=par.p_chosen)
    return res, rec, raw, d


@pytest.mark.parametrize("slots", [False, True], ids=["lockstep", "slots"])
@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_lp_tail_changes_nothing_but_the_record(dev, slots, sampled):
    """LP entry against the entry without it on the same inputs: ids, edited logits, counters, status, n_kept / p_chosen are torch.equal.
    The records: rows inside the image chain NaN / -1; parked rows, want == 0 rows and rows whose step lies outside [0, ld_out) leave
    the sentinel-filled buffers alone; every other record is torch.equal to sx_token_logprobs on the RAW row with the emitted id — so
    row 0 lists its image columns, and row 8's id, a column the rule zeroed, carries its raw value."""
    from seedx_amd import ops
    plain, _, raw, d = _run_tail(dev, slots, sampled, None)
    for n in (0, 3, 8):
        got, rec, _, _ = _run_tail(dev, slots, sampled, n)
        for k in plain:
            assert torch.equal(plain[k], got[k]) or (k == "p_chosen" and torch.equal(plain[k].isnan(), got[k].isnan())), (k, n)
        step0, emitted = _tail_inputs(dev)["step"].tolist(), got["cur"].tolist()
        if slots:
            assert emitted[1] == 400                                           # force_at: the record describes the forced id
        assert emitted[2:4] == [401, 432] and emitted[8] == 401 and not 401 <= emitted[0] <= 465
        records = [g for g in range(G9) if d["want"][g] and 0 <= step0[g] < OUT_ROWS and (not slots or g != 4)]
        assert records == ([0, 1, 2, 3, 8] if slots else [0, 1, 2, 3, 4, 8])
        want_c, want_i, want_t = ops.token_logprobs(raw, VOC, _i32([e if 0 <= e < VOC else 0 for e in emitted], dev), n)
        exp = Rec(dev, d["want"], OUT_ROWS, n)
        for g in records:
            chain = g in (2, 3)
            exp.chosen[g, step0[g]] = float("nan") if chain else want_c[g]
            exp.top_ids[g, step0[g]] = -1 if chain else want_i[g]
            exp.top[g, step0[g]] = float("nan") if chain else want_t[g]
        assert torch.equal(exp.top_ids, rec.top_ids)
        for a, b in ((exp.chosen, rec.chosen), (exp.top, rec.top)):
            assert torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(1.0), b.nan_to_num(1.0)), n
        if n == 8:
            assert all(401 <= i <= 465 for i in rec.top_ids[0, 0].tolist())    # raw: before the rule zeroed them
            assert rec.chosen[0, 0].item() < -30 and abs(rec.chosen[8, 2].item() - want_c[8].item()) == 0
            ref_c, _, _ = rule(raw[:, :VOC].cpu().numpy(), emitted, 0)
            check_values(rec.chosen[8, 2:3].cpu().numpy(), ref_c[8:9], "a zeroed column's raw value")


def test_bits_do_not_depend_on_slot_or_G(dev):
    """One row in slot 0 of 1, and in slots 0 / 5 / 31 of 32 among other rows, through sx_token_logprobs and through the greedy, the
    sampled and the slot LP tail: every record is torch.equal to the G = 1 standalone one (chosen value: for the id each tail emits)."""
    from seedx_amd import ops
    V, ld, n = 32330, 32384, 8
    g = torch.Generator().manual_seed(3)
    row = (torch.randn(ld, generator=g) * 4).to(dev)
    others = (torch.randn(32, ld, generator=g) * 4).to(dev)
    img = _i32(IMG_IDS, dev)

    def alone(target):
        return ops.token_logprobs(row[None].clone(), V, _i32([target], dev), n)
    base = alone(123)
    for slot in (0, 5, 31):
        batch = others.clone()
        batch[slot] = row
        got = ops.token_logprobs(batch, V, _i32([123] * 32, dev), n)
        assert all(torch.equal(a[0], b[slot]) for a, b in zip(base, got))
        for form in ("greedy", "sampled", "slots"):
            lg, cur, step = batch.clone(), _i32([7] * 32, dev), _i32([1] * 32, dev)
            rec = Rec(dev, [1] * 32, 2, n)
            if form == "slots":
                z = lambda v: _i32([v] * 32, dev)
                ops.next_slots_lp(lg, V, img, cur, z(1), z(1), z(99), z(-1), z(4), z(5), step, None, torch.zeros((32, 4), dtype=torch.int32, device=dev), rec)
            else:
                from tests.test_sampling_gpu import Params
                par = Params(dev, [1] * 32, [1.0] * 32, [50] * 32, [0.9] * 32, list(range(32))) if form == "sampled" else None
                ops.next_b_lp(lg, V, img, cur, None, step, rec, par)
            want = alone(cur[slot].item())
            assert torch.equal(rec.chosen[slot, 1], want[0][0]) and torch.equal(rec.top_ids[slot, 1], want[1][0]), (slot, form)
            assert torch.equal(rec.top[slot, 1], want[2][0]) and torch.equal(rec.top[slot, 1], base[2][0]), (slot, form)
            assert (rec.chosen[:, 0] == NEG).all()


# ---- model and engine ------------------------------------------------------------------------------------------------------------
VIT = 128
_SD = {}
PROMPT = [1, 12, 22, 23, 24, 25]


def _agent(dev, dtype, G, **kw):
    from seedx_amd.llama import LlamaForCausalLM
    from seedx_amd.seed_x import ContinuousLVLM
    from seedx_amd.visual_encoder import Resampler
    cfg = weights.MINI_LLM
    if not _SD:
        _SD["llm"], _SD["agent"] = weights.llama_sd(cfg), weights.agent_sd(cfg, VIT, in_grid=4, out_grid=4)
    llm = LlamaForCausalLM(dict(cfg), max_cache_len=512, max_batch=G, **kw)
    llm.load_state_dict(dict(_SD["llm"]))
    H = cfg["hidden_size"]
    agent = ContinuousLVLM(llm, Resampler(4, H, 2, kv_dim=VIT), Resampler(4, VIT, 2, kv_dim=H), add_patch_pos=True)
    agent.load_state_dict(_SD["agent"])
    agent.eval().to(dev, dtype=dtype)
    return agent


def _same(a, b):
    """torch.equal with NaN == NaN"""
    return a.shape == b.shape and torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(3.0), b.nan_to_num(3.0))


def _same_records(a, b):
    return all(_same(a[k].float(), b[k].float()) for k in ("token_ids", "token_logprobs", "top_ids", "top_logprobs"))


MODELS = [(torch.float16, {}), (torch.bfloat16, {}), (torch.float16, dict(kv_pages=12, kv_page_size=32)),
          (torch.float16, dict(kv_format="fp8_e4m3"))]


@pytest.mark.parametrize("dtype,kw", MODELS, ids=["fp16", "bf16", "paged", "fp8kv"])
def test_lockstep_model_records(dev, dtype, kw, monkeypatch):
    """generate_batch, G = 3, a greedy request with an image block, a sampled one and a greedy one that does not ask. Ids and hidden states
    equal the run without "logprobs"; the eager run's records match the fp64 rule on the logits captured just in front of every LP tail
    (NaN / -1 at the forced ids); the graph run equals the eager run bit for bit; the lists are trimmed to each request's N."""
    from seedx_amd import ops
    tok, n = StubTokenizer(), 26
    reqs = [dict(input_ids=[PROMPT]), dict(input_ids=_req(1, n)["input_ids"], do_sample=True, top_p=0.9, seed=5),
            dict(input_ids=_req(2, n)["input_ids"])]
    asked = [dict(reqs[0], logprobs=3), dict(reqs[1], logprobs=1), reqs[2]]
    run = lambda rq: agent.generate_batch(tok, rq, max_new_tokens=n, force_image_at=2, **KW)     # every sequence emits an image block
    agent = _agent(dev, dtype, 3, **kw)
    V = agent.llm.V
    seen = []
    real = ops.next_b_lp

    def spy(logits, vocab, img, cur, out_ids, step, lp, *a, **k):
        seen.append((logits[:, :V].cpu().numpy().copy(), step.tolist()))
        return real(logits, vocab, img, cur, out_ids, step, lp, *a, **k)
    agent.use_graph = False
    plain = run(reqs)
    monkeypatch.setattr(ops, "next_b_lp", spy)
    eager = run(asked)
    monkeypatch.setattr(ops, "next_b_lp", real)
    agent.use_graph = True
    graph = run(asked)
    assert agent.llm._sample_graph_lp is not None and agent.llm._sample_graph is None and agent.llm._graph is None
    for p, e, g in zip(plain, eager, graph):
        assert torch.equal(p["generate_ids"], e["generate_ids"]) and torch.equal(p["last_hidden_states"], e["last_hidden_states"])
        assert torch.equal(p["generate_ids"], g["generate_ids"]) and torch.equal(p["last_hidden_states"], g["last_hidden_states"])
    assert "logprobs" not in eager[2] and "logprobs" not in plain[0]
    for r, N in ((0, 3), (1, 1)):
        assert _same_records(eager[r]["logprobs"], graph[r]["logprobs"])
        lp, ids = eager[r]["logprobs"], eager[r]["generate_ids"]
        assert torch.equal(lp["token_ids"], ids) and lp["top_ids"].shape == (n, N) and lp["token_logprobs"].shape == (n,)
        forced = torch.zeros(n, dtype=torch.bool)
        forced[2:2 + 1 + 17] = True                    # <img> (replaced by the host), <img_0> .. <img_15>, </img>
        assert ids[2:20].tolist() == [400] + list(range(401, 417)) + [465]
        assert torch.equal(lp["token_logprobs"].isnan(), forced) and torch.equal((lp["top_ids"] == -1).all(dim=1), forced)
        rows, tgt, at = [], [], []
        for logits, step in seen:                      # the tails that produced this request's free ids
            if 0 <= step[r] < n and not forced[step[r]]:
                rows.append(logits[r]); tgt.append(int(ids[step[r]])); at.append(step[r])
        assert sorted(at) == [i for i in range(n) if not forced[i]]
        ref_c, ref_i, ref_t = rule(np.stack(rows), tgt, N)
        assert np.array_equal(lp["top_ids"][at].numpy(), ref_i)
        check_values(lp["token_logprobs"][at].numpy(), ref_c, f"model {r} chosen")
        check_values(lp["top_logprobs"][at].numpy(), ref_t, f"model {r} top")
    if kw.get("kv_pages"):
        agent.llm.reset()
        assert agent.llm.kv_pages_free == kw["kv_pages"]


def test_inflight_records_do_not_depend_on_neighbours(dev):
    """Six requests on three slots, four asking (N = 0, 2, 5, 8; one sampled, one with an image block) and two not: every request's
    records equal those of the same request served alone. A queue in which nobody asks takes the plain slot graph; the asking queue the
    LP one."""
    tok = StubTokenizer()
    agent = _agent(dev, torch.float16, 3)
    budgets = [9, 24, 5, 12, 7, 10]
    reqs = [_req(r, b) for r, b in enumerate(budgets)]
    reqs[1]["force_image_at"] = 3
    reqs[3].update(do_sample=True, top_p=0.9, seed=77)
    quiet = agent.generate_inflight(tok, reqs, **KW)
    llm = agent.llm
    assert llm._slot_sample_graph is not None and llm._slot_sample_graph_lp is None and llm._slot_graph_lp is None
    for r, N in ((0, 2), (1, 5), (3, 0), (5, 8)):
        reqs[r]["logprobs"] = N
    busy = agent.generate_inflight(tok, reqs, **KW)
    assert llm._slot_sample_graph_lp is not None
    for r, (q, b) in enumerate(zip(quiet, busy)):
        assert torch.equal(q["generate_ids"], b["generate_ids"]) and torch.equal(q["last_hidden_states"], b["last_hidden_states"])
        assert ("logprobs" in b) == ("logprobs" in reqs[r])
    for r in (0, 1, 3, 5):
        alone = agent.generate_inflight(tok, [reqs[r]], **KW)[0]
        assert torch.equal(alone["generate_ids"], busy[r]["generate_ids"])
        assert _same_records(alone["logprobs"], busy[r]["logprobs"]), r
        lp = busy[r]["logprobs"]
        assert lp["top_ids"].shape == (budgets[r], reqs[r]["logprobs"])
        nan = lp["token_logprobs"].isnan()
        assert nan.tolist() == ([False] * 4 + [True] * 17 + [False] * 3 if r == 1 else [False] * budgets[r]), r
        assert (lp["token_logprobs"][~nan] <= 0).all()
        if reqs[r]["logprobs"]:
            assert (lp["top_logprobs"][~nan][:, 0] >= lp["token_logprobs"][~nan]).all()


# prefill-vs-decode numerics: score() runs the generated ids as ONE chunk through the multi-row pass, the generation produced them one
# token step at a time. Measured maximum |score - record| on the miniature (fp16 / bf16): see profiles/logprobs.md; asserted at 4x.
SCORE_VS_DECODE_MEASURED = {torch.float16: 8.476e-05, torch.bfloat16: 1.955e-05}


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_score_against_forward_and_generation(dev, dtype):
    """score == the rule on the logits of the same two passes through llm.forward (last-row logits of the context; all-row logits of the
    continuation but its last id, continued from the cache), within the kernel bound. And score(prompt, generated ids) against the
    generation's own records: within 4x the measured prefill-vs-decode difference."""
    tok = StubTokenizer()
    agent = _agent(dev, dtype, 1)
    llm = agent.llm
    conts = [[30, 31, 32, 33, 34], [7, 8, 9]]
    got = agent.score(tok, [dict(input_ids=[PROMPT], continuations=conts)], n_top=4)[0]
    for c, rec in zip(conts, got):
        first = llm(input_ids=torch.tensor([PROMPT], device=dev), logits_positions="last")
        rest = llm(input_ids=torch.tensor([c[:-1]], device=dev), past_key_values=first["past_key_values"])
        rows = torch.cat([first["logits"][0], rest["logits"][0]]).cpu().numpy()
        ref_c, ref_i, ref_t = rule(rows, c, 4)
        assert np.array_equal(rec["top_ids"].numpy(), ref_i) and rec["token_logprobs"].dtype == torch.float32
        check_values(rec["token_logprobs"].numpy(), ref_c, "score chosen")
        check_values(rec["top_logprobs"].numpy(), ref_t, "score top")
        assert rec["sum"] == float(rec["token_logprobs"].double().sum())
    gen = agent.generate(tok, input_ids=[PROMPT], max_new_tokens=12, logprobs=0, **KW)
    again = agent.score(tok, [dict(input_ids=[PROMPT], continuations=[gen["generate_ids"].tolist()])])[0][0]
    diff = float((again["token_logprobs"].double() - gen["logprobs"]["token_logprobs"].double()).abs().max())
    print(f"score vs decode records ({dtype}): max |difference| = {diff:.3e}")
    assert diff <= 4 * SCORE_VS_DECODE_MEASURED[dtype]


@pytest.mark.parametrize("kw", [{}, dict(kv_format="fp8_e4m3"), dict(kv_pages=6, kv_page_size=32)], ids=["contiguous", "fp8kv", "paged"])
def test_score_is_order_independent(dev, kw):
    tok = StubTokenizer()
    agent = _agent(dev, torch.float16, 2, **kw)
    a, b = [30, 31, 32, 33, 34, 35], [7, 8, 9]
    req = lambda conts: [dict(input_ids=[PROMPT], continuations=conts)]
    ab, ba = agent.score(tok, req([a, b]), n_top=2)[0], agent.score(tok, req([b, a]), n_top=2)[0]
    only_a, only_b = agent.score(tok, req([a]), n_top=2)[0][0], agent.score(tok, req([b]), n_top=2)[0][0]
    for x, y in ((ab[0], ba[1]), (ab[1], ba[0]), (ab[0], only_a), (ab[1], only_b)):
        assert torch.equal(x["token_logprobs"], y["token_logprobs"]) and x["sum"] == y["sum"]
        assert torch.equal(x["top_ids"], y["top_ids"]) and torch.equal(x["top_logprobs"], y["top_logprobs"])
    assert len(ab[0]["token_logprobs"]) == 6 and torch.isfinite(ab[0]["token_logprobs"]).all() and ab[0]["sum"] < 0
    if kw.get("kv_pages"):
        assert agent.llm.kv_pages_free == kw["kv_pages"]


def test_refusals(dev, monkeypatch):
    from seedx_amd.llama import LogprobState
    tok = StubTokenizer()
    agent = _agent(dev, torch.float16, 2)
    llm = agent.llm
    with pytest.raises(ValueError, match="logprobs must be an int in 0 .. 8"):
        agent.generate_inflight(tok, [dict(input_ids=[PROMPT], logprobs=9)], **KW)
    with pytest.raises(ValueError, match="logprobs must be an int in 0 .. 8"):
        agent.generate_batch(tok, [dict(input_ids=[PROMPT], logprobs=True)] * 2, **KW)
    agent.speculative = True
    with pytest.raises(ValueError, match="agent.speculative is not built \\(follow-up"):
        agent.generate_inflight(tok, [dict(input_ids=[PROMPT], logprobs=1)], **KW)
    agent.speculative = False
    img = _i32(IMG_IDS[:17] + IMG_IDS[-1:], dev)
    out_ids = torch.full((2, 8), -1, dtype=torch.int32, device=dev)
    hid = torch.zeros((2, 8, llm.H), dtype=torch.float32, device=dev)
    st = llm.slot_state(force_id=400, logprobs=2)
    with pytest.raises(ValueError, match="speculative decoding .*follow-up"):
        llm.decode_step(img, out_ids, hid, slots=st, spec=True)
    llm.reset()
    monkeypatch.setattr(llm, "tp", 2)
    with pytest.raises(ValueError, match="tp=2 tensor-parallel ranks are not built \\(follow-up"):
        llm.decode_step(img, out_ids, hid, logprobs=LogprobState(2, 1, dev))
    with pytest.raises(ValueError, match="n_top must be an int in 0 .. 8"):
        LogprobState(2, 9, dev)
