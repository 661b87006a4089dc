"""Seeded sampling on the GPU: the device Philox, the nucleus and the draw of sx_sample_next_b / sx_sample_next_slots against the fp64
statement of the rule (seedx_amd.sampling.reference_next), the greedy identities, the image-token rule, the realised distribution,
replay, and ContinuousLVLM with do_sample (seed-reproducible, first token == the rule on the prefill logits, neighbours do not matter,
graph replay == eager, forced image block)."""
import numpy as np
import pytest
import torch

from tests.test_inflight_gpu import IMG_IDS, KW, _agent, _i32, _kernel_inputs, _req
from tests.test_models_gpu import StubTokenizer, relerr
from tests.test_sampling_cpu import DELTA, PARAM_SETS, boundary_margin

pytestmark = pytest.mark.gpu

SETS = PARAM_SETS + [(0.7, 0, 0.5)]
f32 = lambda v: float(np.float32(v))          # the value the device sees


class Params:
    """Per-row sampling parameters on the device, in the layout ops.sample_next_* takes (what llama.SampleState holds)."""

    def __init__(self, dev, do_sample, temperature, top_k, top_p, seeds):
        G = len(seeds)
        self.do_sample = _i32(do_sample, dev)
        self.temperature = torch.tensor(temperature, dtype=torch.float32, device=dev)
        self.top_k = _i32(top_k, dev)
        self.top_p = torch.tensor(top_p, dtype=torch.float32, device=dev)
        words = np.array([[s & 0xffffffff, s >> 32] for s in seeds], dtype=np.uint32).view(np.int32)
        self.seed = torch.from_numpy(words).to(dev)
        self.n_kept = torch.full((G,), -7, dtype=torch.int32, device=dev)
        self.p_chosen = torch.full((G,), -7.0, dtype=torch.float32, device=dev)


def _sample_b(logits, vocab, img, cur, par, token_index, out_ids=None, step=None):
    from seedx_amd import ops
    ops.sample_next_b(logits, vocab, img, cur, out_ids, step, par, token_index=token_index, n_kept=par.n_kept, p_chosen=par.p_chosen)


# ---- kernel level ------------------------------------------------------------------------------------------------------------------
def test_device_philox(dev):
    """64 rows of 256 equal logits, T = 1, no top-k, top_p = 1: weights are equal and the CDF boundaries multiples of 2^-8, so the id is
    floor(uniform(seed, n) * 256) exactly."""
    from seedx_amd.sampling import uniform
    G, V = 64, 256
    seeds = [0, 1, (1 << 64) - 1, 0x0123456789abcdef, 1 << 32] + [0x9E3779B97F4A7C15 * (g + 1) % (1 << 64) for g in range(G - 5)]
    ns = [0, 1, 2, 3, 119, 65, 1000] * 9 + [7]
    logits = torch.zeros((G, V), dtype=torch.float32, device=dev)
    par = Params(dev, [1] * G, [1.0] * G, [0] * G, [1.0] * G, seeds)
    cur = _i32([5] * G, dev)
    _sample_b(logits, V, _i32([10, 11, 12], dev), cur, par, _i32(ns, dev))
    want = [int(uniform(s, n) * 256) for s, n in zip(seeds, ns)]
    assert cur.tolist() == want
    assert par.n_kept.tolist() == [V] * G and torch.equal(par.p_chosen, torch.full_like(par.p_chosen, 1 / 256))
    assert len(set(want)) > 32


@pytest.mark.parametrize("V,ld,scale", [(500, 512, 3.0), (1031, 1088, 3.0), (32330, 32384, 4.0)])
def test_nucleus_and_draw_against_reference(dev, V, ld, scale):
    """128 rows x 5 parameter sets in ONE launch (row 5 r + s = base row r under set s): n_kept, the id and p_chosen (rel 1e-5) equal
    reference_next in fp64. A row is left out when its outcome is decided within 1e-5 (larger-mass of a kept or first-dropped token
    within 1e-5 of top_p, or u within 1e-5 of a boundary of the reference CDF): at most 10 % of a set's rows."""
    from seedx_amd.sampling import nucleus, uniform
    R = 128
    base = (np.random.default_rng(0).normal(size=(R, V)) * scale).astype(np.float32)
    G = R * len(SETS)
    host = np.zeros((G, ld), dtype=np.float32)
    host[:, :V] = np.repeat(base, len(SETS), axis=0)
    logits = torch.from_numpy(host).to(dev)
    sets = [SETS[g % len(SETS)] for g in range(G)]
    seeds = [(0xD1B54A32D192ED03 * (g + 1)) % (1 << 64) for g in range(G)]
    ns = [(g * 7) % 131 for g in range(G)]
    par = Params(dev, [1] * G, [s[0] for s in sets], [s[1] for s in sets], [s[2] for s in sets], seeds)
    cur = _i32([7] * G, dev)
    _sample_b(logits, V, _i32(IMG_IDS, dev), cur, par, _i32(ns, dev))
    ids, n_kept, p_chosen = cur.tolist(), par.n_kept.tolist(), par.p_chosen.tolist()
    edited = base.copy()
    edited[:, 401:466] = 0.0
    assert torch.equal(logits[:, :V].cpu(), torch.from_numpy(np.repeat(edited, len(SETS), axis=0)))     # the only edit of the rows
    left_out = [0] * len(SETS)
    for g in range(G):
        T, k, p = sets[g]
        kept, probs, larger = nucleus(edited[g // len(SETS)], f32(T), k, f32(p))
        u = uniform(seeds[g], ns[g])
        cdf = np.cumsum(probs)
        edges = np.concatenate([[0.0], cdf[kept]])
        if boundary_margin(larger, kept, f32(p)) < DELTA or np.abs(edges - u).min() < DELTA:
            left_out[g % len(SETS)] += 1
            continue
        want = int(np.nonzero(kept & (cdf > u * cdf[-1]))[0][0])
        assert n_kept[g] == int(kept.sum()), (g, sets[g], n_kept[g], int(kept.sum()))
        assert ids[g] == want, (g, sets[g], ids[g], want, u)
        assert abs(p_chosen[g] - probs[want]) <= 1e-5 * probs[want], (g, sets[g], p_chosen[g], probs[want])
    print("left out per set", left_out)
    assert max(left_out) <= 0.1 * R, left_out


def test_greedy_rows_inside_a_sampled_launch(dev):
    """do_sample = 0 rows of a mixed launch equal sx_greedy_next_b in ids, out_ids and the edited logits (tied maxima included);
    the sampled rows' logits carry the same edit and nothing else."""
    from seedx_amd import ops
    G, rows = 8, 12
    logits, vocab = _kernel_inputs(dev, G)
    logits[1, 37] = logits[1, 300] = 50.0         # tied maxima: the first index wins
    logits[2, 499] = logits[2, 498] = logits[2, 3] = 70.0
    logits[0, 420] = 90.0                         # an image-token column of a free row: zeroed, must not win
    cur0 = _i32([11, 12, 13, 400, 431, 464, 465, 9], dev)
    img, step = _i32(IMG_IDS, dev), _i32([0, 3, 5, 1, 7, 11, 2, 4], dev)
    la, cur_a, out_a = logits.clone(), cur0.clone(), torch.full((G, rows), -1, dtype=torch.int32, device=dev)
    ops.greedy_next_b(la, vocab, img, cur_a, out_a, step)
    do = [0, 0, 0, 0, 1, 0, 1, 1]
    par = Params(dev, do, [0.7] * G, [50] * G, [0.5] * G, list(range(G)))
    lb, cur_b, out_b = logits.clone(), cur0.clone(), torch.full((G, rows), -1, dtype=torch.int32, device=dev)
    _sample_b(lb, vocab, img, cur_b, par, step, out_ids=out_b, step=step)
    assert cur_a.tolist()[:4] == [int(la[0, :vocab].argmax()), 37, 3, 401]
    greedy = [g for g in range(G) if not do[g]]
    assert cur_b[greedy].tolist() == cur_a[greedy].tolist() and torch.equal(out_a[greedy], out_b[greedy])
    assert cur_b.tolist()[4] == 432                                      # sampled, but inside the chain: the next chain id
    assert torch.equal(la, lb)                                           # chain rows untouched, every other row: the image columns only
    assert [par.n_kept.tolist()[g] for g in greedy + [4]] == [-1] * 6 and [par.p_chosen.tolist()[g] for g in greedy + [4]] == [1.0] * 6
    assert all(par.n_kept.tolist()[g] >= 1 and 0 < par.p_chosen.tolist()[g] <= 1 for g in (6, 7))
    assert all(out_b[g, step[g]].item() == cur_b[g].item() for g in range(G))


@pytest.mark.parametrize("V,ld", [(500, 512), (1031, 1088), (32330, 32384)])
def test_top_p_tiny_and_top_k_one_are_the_arg_max(dev, V, ld):
    from seedx_amd import ops
    G = 16
    logits = torch.from_numpy((np.random.default_rng(1).normal(size=(G, ld)) * 3.0).astype(np.float32)).to(dev)
    img, cur0 = _i32(IMG_IDS, dev), _i32([7] * G, dev)
    ref, cur_r = logits.clone(), cur0.clone()
    ops.greedy_next_b(ref, V, img, cur_r, None, None)
    assert ref[:, :V].sort(dim=1, descending=True).values[:, :2].diff(dim=1).max().item() < 0          # rows without ties
    par = Params(dev, [1] * G, [0.7, 1.0] * 8, [0] * 8 + [1] * 8, [1e-6] * 8 + [1.0] * 8, list(range(100, 100 + G)))
    cur = cur0.clone()
    _sample_b(logits, V, img, cur, par, _i32(list(range(G)), dev))
    assert cur.tolist() == cur_r.tolist() and par.n_kept.tolist() == [1] * G and par.p_chosen.tolist() == [1.0] * G
    assert torch.equal(logits, ref)


def test_slots_form_all_greedy_equals_greedy_next_slots(dev):
    """Every output tensor of sx_sample_next_slots with do_sample = 0 everywhere equals sx_greedy_next_slots: an EOS stop, a budget stop,
    a forced id, a chain row and two parked slots included."""
    from seedx_amd import ops
    G, rows, eos = 6, 8, 2
    logits, vocab = _kernel_inputs(dev, G, seed=9)
    logits[0, eos] = logits[4, eos] = 80.0
    logits[2, 77] = 80.0
    img = _i32(IMG_IDS, dev)
    outs = []
    for sampled in (False, True):
        lg = logits.clone()
        cur = _i32([11, 12, 13, -7, 405, -7], dev)
        live, n_new = _i32([1, 1, 1, 0, 1, 0], dev), _i32([3, 4, 2, 12345, 6, 12345], dev)
        max_new, force_at = _i32([100, 5, 100, 1, 100, 1], dev), _i32([-1, -1, 2, 0, -1, 12345], dev)
        pos, ctx, step = _i32([20, 21, 22, 12345, 24, -1], dev), _i32([21, 22, 23, 12345, 25, 0], dev), _i32([3, 4, 2, 12345, 6, -1], dev)
        out_ids = torch.full((G, rows), -9, dtype=torch.int32, device=dev)
        status = torch.full((G, 4), -5, dtype=torch.int32, device=dev)
        if sampled:
            par = Params(dev, [0] * G, [0.7] * G, [50] * G, [0.5] * G, [3] * G)
            ops.sample_next_slots(lg, vocab, img, cur, live, n_new, max_new, force_at, pos, ctx, step, out_ids, status, par,
                                  force_id=400, eos_id=eos, n_kept=par.n_kept, p_chosen=par.p_chosen)
            assert par.n_kept.tolist() == [-1, -1, -1, -7, -1, -7]       # parked slots return before touching anything
        else:
            ops.greedy_next_slots(lg, vocab, img, cur, live, n_new, max_new, force_at, pos, ctx, step, out_ids, status, force_id=400, eos_id=eos)
        outs.append((lg, cur, live, n_new, pos, ctx, step, out_ids, status))
    assert outs[0][2].tolist() == [0, 0, 1, 0, 1, 0] and outs[0][1].tolist()[2] == 400
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("vocab,ld", [(500, 512), (1031, 1088), (32330, 32384)])
def test_slots_form_samples_with_step_as_the_token_index(dev, vocab, ld):
    """Sampled live slots: the id equals sx_sample_next_b's with token_index = step; force_at replaces it after the draw; the stop rule,
    the counters and the status follow the id; a parked slot keeps everything. At every row width of this file: 1031 and 32330 bring
    the float4 row read, its scalar tail and partly filled threads into play."""
    from seedx_amd import ops
    G, rows = 5, 16
    logits = torch.from_numpy((np.random.default_rng(3).normal(size=(G, ld)) * 3.0).astype(np.float32)).to(dev)
    img = _i32(IMG_IDS, dev)
    mk = lambda: Params(dev, [1, 1, 1, 1, 0], [0.7, 1.0, 1.3, 1.0, 1.0], [50, 0, 8, 50, 0], [0.5, 0.9, 1.0, 0.95, 1.0], [5, 6, 7, 8, 9])
    step0, cur0 = [3, 9, 1, 12345, 6], [11, 12, 13, -7, 14]
    pa, cur_a = mk(), _i32(cur0, dev)
    _sample_b(logits.clone(), vocab, img, cur_a, pa, _i32([3, 9, 1, 0, 6], dev))
    want = cur_a.tolist()
    pb, cur = mk(), _i32(cur0, dev)
    live, n_new, max_new = _i32([1, 1, 1, 0, 1], dev), _i32([3, 9, 1, 12345, 6], dev), _i32([100, 10, 100, 1, 100], dev)
    force_at, pos, ctx, step = _i32([-1, -1, 1, 0, -1], dev), _i32([20, 21, 22, -1, 24], dev), _i32([21, 22, 23, 0, 25], dev), _i32(step0, dev)
    out_ids = torch.full((G, rows), -9, dtype=torch.int32, device=dev)
    status = torch.full((G, 4), -5, dtype=torch.int32, device=dev)
    lg = logits.clone()
    ops.sample_next_slots(lg, vocab, img, cur, live, n_new, max_new, force_at, pos, ctx, step, out_ids, status, pb, force_id=400,
                          eos_id=-1, n_kept=pb.n_kept, p_chosen=pb.p_chosen)
    assert cur.tolist() == [want[0], want[1], 400, -7, want[4]]
    assert want[4] == int(lg[4, :vocab].argmax())
    assert live.tolist() == [1, 0, 1, 0, 1] and n_new.tolist() == [4, 10, 2, 12345, 7] and step.tolist() == [4, -1, 2, 12345, 7]
    assert status.tolist() == [[want[0], 1, 4, -1], [want[1], 0, 10, 10], [400, 1, 2, -1], [-5] * 4, [want[4], 1, 7, -1]]
    assert [out_ids[g, s].item() for g, s in ((0, 3), (1, 9), (2, 1), (4, 6))] == [want[0], want[1], 400, want[4]]
    assert torch.equal(lg[3], logits[3]) and pb.n_kept.tolist()[3] == -7
    assert pb.n_kept.tolist()[:3] == pa.n_kept.tolist()[:3] and torch.equal(pb.p_chosen[:3], pa.p_chosen[:3])


def test_image_rule(dev):
    """Inside the chain: the next chain id whatever the parameters, the row untouched. Outside: the image columns are zeroed in place and
    nothing else changes; with text logits >= 20 and top_p = 0.9 no image id comes back."""
    from seedx_amd import ops
    G, V = 64, 500
    rng = np.random.default_rng(4)
    host = (20.0 + np.abs(rng.normal(size=(G, 512))) * 3.0).astype(np.float32)
    host[:, 401:466] = 30.0 + rng.normal(size=(G, 65)).astype(np.float32)           # would win if they were not zeroed
    logits = torch.from_numpy(host).to(dev)
    chain = {0: 400, 1: 401, 2: 431, 3: 464}
    cur0 = [chain.get(g, 465 if g == 4 else 7) for g in range(G)]
    par = Params(dev, [1] * G, [0.7, 1.0, 1.3, 2.0] * 16, [50, 0, 8, 1] * 16, [0.9] * G, list(range(G)))
    cur, img = _i32(cur0, dev), _i32(IMG_IDS, dev)
    ref, cur_r = logits.clone(), _i32(cur0, dev)
    ops.greedy_next_b(ref, V, img, cur_r, None, None)
    _sample_b(logits, V, img, cur, par, _i32([g % 5 for g in range(G)], dev))
    ids = cur.tolist()
    assert ids[:4] == [401, 402, 432, 465] and par.n_kept.tolist()[:4] == [-1] * 4
    assert torch.equal(logits[:4].cpu(), torch.from_numpy(host[:4]))
    assert torch.equal(logits, ref) and (logits[4:, 401:466] == 0).all()
    assert all(not 401 <= i <= 465 for i in ids[4:]), ids
    assert len(set(ids[4:])) > 8


def test_distribution(dev):
    """4096 rows in one launch, seeds 0..4095, probabilities 0.5 / 0.25 / 0.125 / 0.125 (the rest -inf): every count within 5 binomial
    sigma (32 / 27.7 / 21.2). Deterministic. The 0.5 token is an image column: its logit 0.0 is what the in-place rule writes."""
    G, V = 4096, 500
    host = np.full((G, 512), -np.inf, dtype=np.float32)
    host[:, 3], host[:, 250], host[:, 77] = np.log(0.5), np.log(0.25), np.log(0.25)
    host[:, 499] = 5.0                                                   # img_ids[1]: zeroed → logit 0
    logits = torch.from_numpy(host).to(dev)
    par = Params(dev, [1] * G, [1.0] * G, [0] * G, [1.0] * G, list(range(G)))
    cur = _i32([7] * G, dev)
    _sample_b(logits, V, _i32([498, 499], dev), cur, par, _i32([0] * G, dev))
    counts = np.bincount(np.array(cur.tolist()), minlength=V)
    print("counts", counts[[499, 3, 77, 250]])
    assert counts.sum() == G == counts[[499, 3, 77, 250]].sum() and par.n_kept.tolist() == [4] * G
    probs = {499: 0.5, 3: 0.25, 77: 0.125, 250: 0.125}
    host_p = np.exp(np.array([0.0, np.log(0.5), np.log(0.25), np.log(0.25)]))
    assert np.allclose(host_p / host_p.sum(), [0.5, 0.25, 0.125, 0.125])
    for col, p in probs.items():
        assert abs(counts[col] - G * p) <= 5 * np.sqrt(G * p * (1 - p)), (col, counts[col])
    assert np.allclose(sorted(set(par.p_chosen.tolist())), [0.125, 0.25, 0.5], rtol=1e-6)


def test_replay_is_bit_equal(dev):
    """The same launch twice and once inside a captured graph: ids, n_kept and p_chosen are bit-equal."""
    G, V, ld = 40, 1031, 1088
    logits0 = torch.from_numpy((np.random.default_rng(6).normal(size=(G, ld)) * 3.0).astype(np.float32)).to(dev)
    sets = [SETS[g % len(SETS)] for g in range(G)]
    par = Params(dev, [1] * G, [s[0] for s in sets], [s[1] for s in sets], [s[2] for s in sets], [g * 977 + 1 for g in range(G)])
    img, cur0, tok = _i32(IMG_IDS, dev), _i32([7] * G, dev), _i32(list(range(G)), dev)
    logits, cur = logits0.clone(), cur0.clone()

    def launch():
        logits.copy_(logits0)
        cur.copy_(cur0)
        _sample_b(logits, V, img, cur, par, tok)
    got = []
    for _ in range(2):
        launch()
        got.append((cur.clone(), par.n_kept.clone(), par.p_chosen.clone()))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        launch()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    par.n_kept.fill_(-3)
    g.replay()
    torch.cuda.synchronize()
    got.append((cur.clone(), par.n_kept.clone(), par.p_chosen.clone()))
    assert len(set(got[0][0].tolist())) > 4 and (got[0][1] >= 1).all()
    for other in got[1:]:
        for a, b in zip(got[0], other):
            assert torch.equal(a, b)


# ---- model level -------------------------------------------------------------------------------------------------------------------
PROMPT = [1, 12, 22, 23, 24, 25]
IMG16 = [400] + list(range(401, 417)) + [465]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_generate_is_reproducible_per_seed(dev, dtype):
    agent, tok = _agent(dev, dtype, 1), StubTokenizer()
    run = lambda **kw: agent.generate(tok, input_ids=[PROMPT], max_new_tokens=12, do_sample=True, **kw, **KW)
    a, b = run(seed=11), run(seed=11)
    assert torch.equal(a["generate_ids"], b["generate_ids"]) and a["seed"] == 11 and len(a["generate_ids"]) == 12
    assert torch.equal(a["last_hidden_states"], b["last_hidden_states"])
    outs = [run(seed=s, top_k=50, top_p=0.9)["generate_ids"].tolist() for s in (1, 2, 3, 4)]
    print(outs)
    assert any(o != outs[0] for o in outs[1:])
    free = run()                                                          # seed=None: drawn, reported, and reproducible from the report
    assert torch.equal(run(seed=free["seed"])["generate_ids"], free["generate_ids"])
    greedy = agent.generate(tok, input_ids=[PROMPT], max_new_tokens=12, **KW)
    assert "seed" not in greedy and torch.equal(greedy["generate_ids"], agent.generate(tok, input_ids=[PROMPT], max_new_tokens=12, **KW)["generate_ids"])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_first_token_is_the_rule_on_the_prefill_logits(dev, dtype):
    """Token index 0: reference_next on llm.forward's last-position logits (image columns zeroed) with uniform(seed, 0). The seed is the
    first of 1, 2, ... that the 1e-5 exclusion of the kernel tests does not leave out."""
    from seedx_amd.sampling import nucleus, uniform
    agent, tok = _agent(dev, dtype, 1), StubTokenizer()
    T, k, p = 1.0, 50, 0.9
    x = agent.llm(input_ids=torch.tensor([PROMPT], device=dev), logits_positions="last")["logits"][0, 0].float().cpu().numpy().copy()
    x[401:417] = 0.0
    x[465] = 0.0
    kept, probs, larger = nucleus(x, f32(T), k, f32(p))
    cdf = np.cumsum(probs)
    edges = np.concatenate([[0.0], cdf[kept]])
    assert boundary_margin(larger, kept, f32(p)) >= DELTA
    seed = next(s for s in range(1, 9) if np.abs(edges - uniform(s, 0)).min() >= DELTA)
    want = int(np.nonzero(kept & (cdf > uniform(seed, 0) * cdf[-1]))[0][0])
    got = agent.generate(tok, input_ids=[PROMPT], max_new_tokens=1, do_sample=True, temperature=T, top_k=k, top_p=p, seed=seed, **KW)
    assert got["generate_ids"].tolist() == [want], (seed, got["generate_ids"].tolist(), want, int(kept.sum()))
    assert int(kept.sum()) > 1


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_neighbours_do_not_matter(dev, dtype):
    """One sampled request alone (max_batch = 1), at position 2 of a generate_batch of 4, and inside a generate_inflight queue of 9 mixed
    greedy / sampled requests on 4 slots with different budgets: identical ids, hidden states within the like-with-like tolerance of
    tests/test_inflight_gpu.py (precise mode: 2e-4 fp16 / 2e-3 bf16). The greedy requests of the mixed queue equal the all-greedy queue."""
    tok = StubTokenizer()
    smp = dict(do_sample=True, temperature=1.0, top_k=50, top_p=0.9, seed=1234)
    n = 10
    alone = _agent(dev, dtype, 1).generate(tok, input_ids=[PROMPT], max_new_tokens=n, **smp, **KW)
    agent = _agent(dev, dtype, 4)
    others = [dict(input_ids=_req(r, n)["input_ids"]) for r in range(3)]
    wave = [others[0], dict(others[1], do_sample=True, seed=5), dict(input_ids=[PROMPT], **smp), others[2]]
    batch = agent.generate_batch(tok, wave, max_new_tokens=n, **KW)
    budgets = [6, 9, 4, 12, n, 3, 7, 5, 8]
    queue = [_req(r, b) for r, b in enumerate(budgets)]
    queue[4] = dict(input_ids=[PROMPT], max_new_tokens=n, **smp)
    for r, s in ((1, 21), (6, 22), (7, 23)):
        queue[r].update(do_sample=True, top_p=0.9, seed=s)
    busy = agent.generate_inflight(tok, queue, **KW)
    ids = alone["generate_ids"].tolist()
    print("sampled transcript", ids)
    assert len(ids) == n and alone["seed"] == batch[2]["seed"] == busy[4]["seed"] == 1234 and "seed" not in busy[0]
    assert batch[2]["generate_ids"].tolist()[:n] == ids, (batch[2]["generate_ids"].tolist(), ids)
    assert busy[4]["generate_ids"].tolist() == ids, (busy[4]["generate_ids"].tolist(), ids)
    tol = 2e-4 if dtype == torch.float16 else 2e-3
    assert relerr(batch[2]["last_hidden_states"][:n - 1], alone["last_hidden_states"]) < tol
    assert relerr(busy[4]["last_hidden_states"], alone["last_hidden_states"]) < tol
    assert [len(x["generate_ids"]) for x in busy] == budgets
    greedy_queue = [{k: v for k, v in q.items() if k in ("input_ids", "max_new_tokens")} for q in queue]
    plain = agent.generate_inflight(tok, greedy_queue, **KW)
    for r in (0, 2, 3, 5, 8):
        assert torch.equal(busy[r]["generate_ids"], plain[r]["generate_ids"]), r
        assert torch.equal(busy[r]["last_hidden_states"], plain[r]["last_hidden_states"]), r
    assert any(not torch.equal(busy[r]["generate_ids"], plain[r]["generate_ids"]) for r in (1, 4, 6, 7))


def test_sampled_inflight_graph_replay_equals_eager(dev):
    tok = StubTokenizer()
    reqs = [_req(r, b, force_image_at=2 if r == 1 else None) for r, b in enumerate([9, 22, 4, 1, 7])]
    for r, s in ((0, 31), (1, 32), (3, 33), (4, 34)):
        reqs[r].update(do_sample=True, temperature=1.0, top_p=0.9, seed=s)
    out = []
    for use_graph in (False, True):
        agent = _agent(dev, torch.float16, 2)
        agent.use_graph = use_graph
        out.append(agent.generate_inflight(tok, reqs, **KW))
        out.append(agent.generate_inflight(tok, reqs, **KW))      # a second call reuses the buffers (and the captured step)
        assert (agent.llm._slot_sample_graph is not None) == use_graph and agent.llm._slot_graph is None
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert torch.equal(a["generate_ids"], b["generate_ids"]) and torch.equal(a["last_hidden_states"], b["last_hidden_states"])
    assert out[0][1]["num_gen_imgs"] == 1 and [len(x["generate_ids"]) for x in out[0]] == [9, 22, 4, 1, 7]
    assert torch.equal(out[0][1]["img_gen_feat"], out[2][1]["img_gen_feat"])


def test_sampled_request_with_a_forced_image_block(dev):
    agent, tok = _agent(dev, torch.float16, 1), StubTokenizer()
    got = agent.generate(tok, input_ids=[PROMPT], max_new_tokens=30, do_sample=True, top_p=0.9, seed=77, force_image_at=3, **KW)
    ids = got["generate_ids"].tolist()
    assert ids[3:21] == IMG16 and got["num_gen_imgs"] == 1 and got["img_gen_feat"] is not None and len(ids) == 30
    assert got["img_gen_feat"].shape[0] == 1 and torch.isfinite(got["img_gen_feat"].float()).all()
    again = agent.generate(tok, input_ids=[PROMPT], max_new_tokens=30, do_sample=True, top_p=0.9, seed=77, force_image_at=3, **KW)
    assert again["generate_ids"].tolist() == ids
