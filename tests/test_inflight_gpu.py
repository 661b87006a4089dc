"""In-flight batching on the GPU: the fused next-token / stop-rule / slot-advance kernel (sx_greedy_next_slots), the slot mode of the
decode step (a parked slot writes nothing and stays finite on every attention route) and ContinuousLVLM.generate_inflight (neighbours
do not matter, agreement with the lock-step path, EOS on the device, any queue length, graph replay == eager)."""
import pytest
import torch

from oracle import weights
from tests.test_models_gpu import StubTokenizer, relerr

pytestmark = pytest.mark.gpu

VIT = 128
IMG_IDS = list(range(400, 466))          # <img>, <img_00000> .. <img_00063>, </img> of the StubTokenizer
KW = dict(num_img_gen_tokens=16, eos_token_id=None)
_SD = {}


def _agent(dev, dtype, G, precise=None):
    from seedx_amd.llama import LlamaForCausalLM
    from seedx_amd.seed_x import ContinuousLVLM
    from seedx_amd.visual_encoder import Resampler
    cfg = weights.MINI_LLM
    if not _SD:
        _SD["llm"], _SD["agent"] = weights.llama_sd(cfg), weights.agent_sd(cfg, VIT, in_grid=4, out_grid=4)
    llm = LlamaForCausalLM(dict(cfg), max_cache_len=512, max_batch=G, precise=precise)
    llm.load_state_dict(dict(_SD["llm"]))
    H = cfg["hidden_size"]
    agent = ContinuousLVLM(llm, Resampler(4, H, 2, kv_dim=VIT), Resampler(4, VIT, 2, kv_dim=H), add_patch_pos=True)
    agent.load_state_dict(_SD["agent"])
    agent.eval().to(dev, dtype=dtype)
    return agent


def _req(r, budget, force_image_at=None, n_text=None):
    ids = [1, 10 + r] + [20 + r + i for i in range(3 + r % 5 if n_text is None else n_text)]
    d = dict(input_ids=[ids], max_new_tokens=budget)
    if force_image_at is not None:
        d["force_image_at"] = force_image_at
    return d


def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


# ---- kernel level ------------------------------------------------------------------------------------------------------------------
def _kernel_inputs(dev, G, ld=512, vocab=500, seed=5):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(G, ld, generator=g).to(dev)
    logits[:, 401:465] += 6.0                     # image-token columns that the rule must zero before the arg-max
    return logits, vocab


def test_slots_kernel_equals_greedy_next_b_plus_counters(dev):
    """All slots live, no stop: ids, out_ids, counters and the in-place edited logits equal sx_greedy_next_b + three sx_add_i32_n."""
    from seedx_amd import ops
    G, rows = 7, 12
    logits, vocab = _kernel_inputs(dev, G)
    logits[1, 37] = logits[1, 300] = 50.0         # tied maxima: the first index wins
    logits[2, 499] = logits[2, 498] = logits[2, 3] = 70.0
    logits[0, 420] = 90.0                         # an image-token column of a free row: zeroed, must not win
    cur0 = _i32([11, 12, 13, 400, 431, 464, 465], dev)      # rows 3-5 sit inside the forced image chain; 465 (</img>) is free again
    img = _i32(IMG_IDS, dev)
    step0, pos0 = _i32([0, 3, 5, 1, 7, 11, 2], dev), _i32([9, 30, 2, 0, 100, 17, 55], dev)
    # reference: the lock-step tail
    la, cur_a, out_a = logits.clone(), cur0.clone(), torch.full((G, rows), -1, dtype=torch.int32, device=dev)
    step_a, pos_a, ctx_a = step0.clone(), pos0.clone(), pos0 + 1
    ops.greedy_next_b(la, vocab, img, cur_a, out_a, step_a)
    for t in (step_a, pos_a, ctx_a):
        ops.add_i32(t, 1)
    # the fused kernel
    lb, cur_b, out_b = logits.clone(), cur0.clone(), torch.full((G, rows), -1, dtype=torch.int32, device=dev)
    step_b, pos_b, ctx_b = step0.clone(), pos0.clone(), pos0 + 1
    live, n_new, max_new = _i32([1] * G, dev), _i32([1, 2, 3, 4, 5, 6, 7], dev), _i32([1000] * G, dev)
    force_at, status = _i32([-1] * G, dev), torch.full((G, 4), -5, dtype=torch.int32, device=dev)
    ops.greedy_next_slots(lb, vocab, img, cur_b, live, n_new, max_new, force_at, pos_b, ctx_b, step_b, out_b, status, force_id=400, eos_id=-1)
    torch.cuda.synchronize()
    assert cur_a.tolist()[1] == 37 and cur_a.tolist()[2] == 3 and cur_a.tolist()[3:6] == [401, 432, 465]
    for a, b in ((cur_a, cur_b), (out_a, out_b), (step_a, step_b), (pos_a, pos_b), (ctx_a, ctx_b), (la, lb)):
        assert torch.equal(a, b)
    assert live.tolist() == [1] * G and n_new.tolist() == [2, 3, 4, 5, 6, 7, 8]
    assert status.tolist() == [[c, 1, n, -1] for c, n in zip(cur_b.tolist(), n_new.tolist())]
    assert out_b[5, 11].item() == 465 and (out_b == -1).sum().item() == G * rows - G


def test_slots_kernel_stop_rule_and_parked_slots(dev):
    """EOS hit, budget hit and a forced id at force_at; parked slots keep cur, out_ids, counters, status and their logits row bit for bit."""
    from seedx_amd import ops
    G, rows, eos = 6, 8, 2
    logits, vocab = _kernel_inputs(dev, G, seed=9)
    logits[0, eos] = 80.0                         # slot 0 emits EOS
    logits[2, 77] = 80.0                          # slot 2: arg-max 77, replaced by force_id at n_new == force_at
    logits[4, eos] = 80.0                         # slot 4 would emit EOS but sits in the image chain: the chain wins, no stop
    before = logits.clone()
    img = _i32(IMG_IDS, dev)
    cur = _i32([11, 12, 13, -7, 405, -7], dev)                     # -7 / 12345 / -9: sentinels of the parked slots 3 and 5
    live, n_new = _i32([1, 1, 1, 0, 1, 0], dev), _i32([3, 4, 2, 12345, 6, 12345], dev)
    max_new, force_at = _i32([100, 5, 100, 1, 100, 1], dev), _i32([-1, -1, 2, 0, -1, 12345], dev)
    pos, ctx, step = _i32([20, 21, 22, 12345, 24, -1], dev), _i32([21, 22, 23, 12345, 25, 0], dev), _i32([3, 4, 2, 12345, 6, -1], dev)
    out_ids = torch.full((G, rows), -9, dtype=torch.int32, device=dev)
    status = torch.full((G, 4), -5, dtype=torch.int32, device=dev)
    ops.greedy_next_slots(logits, vocab, img, cur, live, n_new, max_new, force_at, pos, ctx, step, out_ids, status, force_id=400, eos_id=eos)
    torch.cuda.synchronize()
    ref = before.clone()
    ref[:, 401:466] = 0.0
    id1 = int(ref[1, :vocab].argmax())
    assert cur.tolist() == [eos, id1, 400, -7, 406, -7]
    assert live.tolist() == [0, 0, 1, 0, 1, 0]
    assert n_new.tolist() == [4, 5, 3, 12345, 7, 12345]
    assert step.tolist() == [-1, -1, 3, 12345, 7, -1] and pos.tolist() == [-1, -1, 23, 12345, 25, -1]
    assert ctx.tolist() == [0, 0, 24, 12345, 26, 0]
    assert status.tolist() == [[eos, 0, 4, 4], [id1, 0, 5, 5], [400, 1, 3, -1], [-5] * 4, [406, 1, 7, -1], [-5] * 4]
    exp_out = torch.full((G, rows), -9, dtype=torch.int32)
    exp_out[0, 3], exp_out[1, 4], exp_out[2, 2], exp_out[4, 6] = eos, id1, 400, 406
    assert torch.equal(out_ids.cpu(), exp_out)
    for g in (3, 5):                              # parked: the logits row is not even zeroed at the image columns
        assert torch.equal(logits[g], before[g])
    assert torch.equal(logits[4], before[4])      # a row inside the chain skips the zeroing too (as sx_greedy_next_b does)
    for g in (0, 1, 2):
        assert torch.equal(logits[g, :vocab], ref[g, :vocab])


# ---- model level -------------------------------------------------------------------------------------------------------------------
ROUTES = ["precise_fused_rope", "precise_rope_launch", "plain_fused_attention", "plain_three_launches"]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("route", ROUTES)
def test_parked_slot_writes_nothing_and_stays_finite(dev, dtype, route, monkeypatch):
    """Slot 0 finishes after two steps. Its KV rows (all layers), out_ids row and hidden-state rows are then filled with sentinels and
    ten more steps run: every sentinel is intact, its logits row is finite in each step, the other slots advance."""
    from seedx_amd import ops
    precise = route.startswith("precise")
    monkeypatch.setenv("SX_LLM_FUSE_ROPE", "0" if route == "precise_rope_launch" else "1")
    agent = _agent(dev, dtype, 4, precise=precise)
    llm = agent.llm
    P = llm._pack()
    assert llm.precise == precise and llm.hd == 128
    if not precise:
        llm.fused_decode_attention = route == "plain_fused_attention"
    G, rows = 4, 40
    img = _i32(IMG_IDS[:1] + IMG_IDS[1:17] + IMG_IDS[-1:], dev)
    st = llm.slot_state(force_id=400, eos_id=-1)
    assert P["pos"].tolist() == [-1] * G and P["ctx"].tolist() == [0] * G and P["step"].tolist() == [-1] * G
    out_ids = torch.full((G, rows), -1, dtype=torch.int32, device=dev)
    hid = torch.zeros((G, rows, llm.H), dtype=torch.float32, device=dev)
    prompts = [[1, 10 + g] + [20 + g + i for i in range(3 + g)] for g in range(G)]
    xs = [ops.embedding(_i32(p, dev), P["embed"]) for p in prompts]
    llm._slot_write(P["pos"], range(G), 0)
    llm._slot_write(P["ctx"], range(G), 1)
    logits, _ = llm.forward_embeds_batch(xs, list(range(G)))
    first = _i32([p[-1] for p in prompts], dev)
    ops.greedy_next_b(logits.contiguous(), llm.V, img, first, None, None)
    P["cur"].copy_(first)
    out_ids[:, 0] = first
    P["step"].fill_(1)
    st.n_new.fill_(1)
    st.max_new.copy_(_i32([3, 30, 30, 30], dev))
    st.live.fill_(1)
    for _ in range(2):
        llm.decode_step(img, out_ids, hid, use_graph=True, slots=st)
    assert st.live.tolist() == [0, 1, 1, 1] and st.status[0].tolist()[1:] == [0, 3, 3]
    assert P["pos"][0].item() == -1 and P["ctx"][0].item() == 0 and P["step"][0].item() == -1
    cur0 = P["cur"][0].item()
    P["kc"][:, 0] = 0.5
    P["vc"][:, 0] = -0.25
    out_ids[0] = -77
    hid[0] = -3.25
    kc0, vc0 = P["kc"][:, 0].clone(), P["vc"][:, 0].clone()
    for i in range(10):
        llm.decode_step(img, out_ids, hid, use_graph=True, slots=st)
        assert torch.isfinite(st.logits).all(), (route, i)
    assert torch.equal(P["kc"][:, 0], kc0) and torch.equal(P["vc"][:, 0], vc0)
    assert torch.equal(out_ids[0], torch.full_like(out_ids[0], -77)) and torch.equal(hid[0], torch.full_like(hid[0], -3.25))
    assert P["cur"][0].item() == cur0 and st.n_new.tolist() == [3, 13, 13, 13] and st.status[0].tolist()[1:] == [0, 3, 3]
    assert P["pos"].tolist() == [-1] + [len(prompts[g]) + 12 for g in (1, 2, 3)]
    assert (out_ids[1:, :13] >= 0).all() and (out_ids[1:, 13:] == -1).all()
    llm.reset()


def _busy_queue(image_at=4):
    """12 requests for 4 slots, budgets [24, 6, 6, 6] x 3; request `image_at` emits a 16-token image block."""
    return [_req(r, b, force_image_at=3 if r == image_at else None) for r, b in enumerate([24, 6, 6, 6] * 3)]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("precise", [False, True])
def test_neighbours_do_not_matter(dev, dtype, precise):
    """max_admit = 1: every prefill is a single-request pass, decode rows are independent — a request's ids and hidden states from a
    busy queue are bit-identical to the same request served alone by the same 4-wide agent."""
    agent, tok = _agent(dev, dtype, 4, precise=precise), StubTokenizer()
    reqs = _busy_queue()
    seen = []
    busy = agent.generate_inflight(tok, reqs, max_admit=1, on_result=lambda i, r: seen.append(i), **KW)
    assert sorted(seen) == list(range(12)) and len(busy) == 12
    assert busy[4]["generate_ids"].tolist()[3:21] == [400] + list(range(401, 417)) + [465] and busy[4]["num_gen_imgs"] == 1
    for r, req in enumerate(reqs):
        alone = agent.generate_inflight(tok, [req], max_admit=1, **KW)[0]
        assert len(busy[r]["generate_ids"]) == req["max_new_tokens"]
        assert torch.equal(busy[r]["generate_ids"], alone["generate_ids"]), r
        assert torch.equal(busy[r]["last_hidden_states"], alone["last_hidden_states"]), r
        assert busy[r]["text"] == alone["text"] and sorted(busy[r]) == sorted(alone)
    assert torch.equal(busy[4]["img_gen_feat"], agent.generate_inflight(tok, [reqs[4]], max_admit=1, **KW)[0]["img_gen_feat"])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("precise", [False, True])
def test_agrees_with_lockstep_waves(dev, dtype, precise):
    """The same 12 requests through generate_batch in waves of 4, every request run to the queue's largest budget (24) and cut to its
    own. generate_batch forces the image block per WAVE, so the four requests of wave 1 all carry it. Precise mode: identical ids over
    each request's own length; hidden states / img_gen_feat within the like-with-like tolerances of tests/test_batched_decode_gpu.py
    (plain 3e-3 fp16 / 2.4e-2 bf16, precise 2e-4 fp16 / 2e-3 bf16). Plain mode follows that file too: random-weight logits can be
    near-ties, so the ids must agree through the image block (21 tokens) where there is one and the states are compared up to the
    first differing id."""
    agent, tok = _agent(dev, dtype, 4, precise=precise), StubTokenizer()
    budgets = [24, 6, 6, 6, 24, 24, 24, 24, 6, 24, 6, 6]
    reqs = [_req(r, b, force_image_at=3 if 4 <= r < 8 else None) for r, b in enumerate(budgets)]
    got = agent.generate_inflight(tok, reqs, **KW)
    assert agent.last_inflight_stats["admissions"] == 12
    tol = (3e-3 if dtype == torch.float16 else 2.4e-2) if not precise else (2e-4 if dtype == torch.float16 else 2e-3)
    for w in range(3):
        wave = [{k: v for k, v in q.items() if k not in ("max_new_tokens", "force_image_at")} for q in reqs[4 * w:4 * w + 4]]
        ref = agent.generate_batch(tok, wave, max_new_tokens=24, force_image_at=3 if w == 1 else None, **KW)
        for i in range(4):
            r, b = 4 * w + i, budgets[4 * w + i]
            a, e = got[r]["generate_ids"].tolist(), ref[i]["generate_ids"].tolist()[:b]
            assert len(a) == b
            n = next((k for k, (u, v) in enumerate(zip(a, e)) if u != v), b)
            print(f"wave {w} request {r}: ids agree over {n} of {b}; hidden relerr",
                  relerr(got[r]["last_hidden_states"][:n - 1], ref[i]["last_hidden_states"][:n - 1]) if n > 1 else None)
            if precise:
                assert a == e, (r, a, e)
            assert n >= (21 if w == 1 else 1), (r, n, a, e)
            if n > 1:
                assert relerr(got[r]["last_hidden_states"][:n - 1], ref[i]["last_hidden_states"][:n - 1]) < tol
            if w == 1:
                assert a[3:21] == [400] + list(range(401, 417)) + [465]
                assert relerr(got[r]["img_gen_feat"], ref[i]["img_gen_feat"]) < tol


def test_eos_stops_a_request_on_the_device(dev):
    """eos_token_id = an id that request 0's solo transcript emits first at step k >= 1: in the busy queue request 0 ends there with the
    EOS as its last id; every request equals its own solo run under the same EOS (neighbours unaffected)."""
    agent, tok = _agent(dev, torch.float16, 4), StubTokenizer()
    reqs = [_req(r, b) for r, b in enumerate([24, 6, 9, 6, 12, 6])]
    solo = agent.generate_inflight(tok, [reqs[0]], **KW)[0]["generate_ids"].tolist()
    print("solo transcript", solo)
    k = max(solo.index(t) for t in set(solo) if solo.index(t) <= 20)
    assert k >= 1, solo
    kw = dict(KW, eos_token_id=solo[k])
    busy = agent.generate_inflight(tok, reqs, max_admit=1, **kw)
    assert busy[0]["generate_ids"].tolist() == solo[:k + 1] and busy[0]["generate_ids"][-1].item() == solo[k]
    assert busy[0]["last_hidden_states"].shape[0] == k
    for r, req in enumerate(reqs):
        alone = agent.generate_inflight(tok, [req], max_admit=1, **kw)[0]
        assert torch.equal(busy[r]["generate_ids"], alone["generate_ids"]), r
        assert torch.equal(busy[r]["last_hidden_states"], alone["last_hidden_states"]), r
        ids = busy[r]["generate_ids"].tolist()
        assert solo[k] not in ids[:-1] and (len(ids) == req["max_new_tokens"] or ids[-1] == solo[k])
    assert agent.last_inflight_stats is not None


def test_fewer_and_more_requests_than_slots(dev):
    """N = 1, G - 1 and 3G + 1 on 4 slots; the engine's step counts are the scheduler's prediction for the realised lengths. On the
    [24, 6, 6, 6] x 3 queue: 33 decode steps against 69 for lock-step waves."""
    from seedx_amd.inflight import lockstep_wave_steps, simulate
    agent, tok = _agent(dev, torch.float16, 4), StubTokenizer()
    for budgets in ([7], [5, 9, 3], [6, 3, 11, 1, 8, 2, 2, 9, 4, 1, 7, 5, 10], [24, 6, 6, 6] * 3):
        res = agent.generate_inflight(tok, [_req(r, b) for r, b in enumerate(budgets)], **KW)
        lengths = [len(x["generate_ids"]) for x in res]
        assert lengths == budgets                                  # no EOS, no image block: every request runs to its budget
        assert all(x["last_hidden_states"].shape == (b - 1, 256) and not x["has_img_output"] for x, b in zip(res, budgets))
        want, stats = simulate(lengths, 4), agent.last_inflight_stats
        for k in ("decode_steps", "live_slot_steps", "parked_slot_steps", "admissions", "prefill_passes"):
            assert stats[k] == want[k], (budgets, k, stats, want)
        assert stats["prefill_tokens"] == sum(len(_req(r, b)["input_ids"][0]) for r, b in enumerate(budgets))
    assert stats["decode_steps"] == 33 < lockstep_wave_steps(budgets, 4) == 69
    limited = agent.generate_inflight(tok, [_req(r, b) for r, b in enumerate([5, 1, 3])], max_admit=1, **KW)
    assert [len(x["generate_ids"]) for x in limited] == [5, 1, 3]
    assert agent.last_inflight_stats["decode_steps"] == simulate([5, 1, 3], 4, 1)["decode_steps"]
    assert agent.llm._pack()["pos"].tolist() == [0] * 4 and agent.llm._pack()["ctx"].tolist() == [1] * 4   # idle values are gone


@pytest.mark.parametrize("precise", [False, True])
def test_graph_replay_equals_eager_slot_step(dev, precise):
    """use_graph False vs True across admissions and finishes (5 requests on 2 slots, one image block): bit-identical."""
    tok = StubTokenizer()
    reqs = [_req(r, b, force_image_at=2 if r == 1 else None) for r, b in enumerate([9, 22, 4, 1, 7])]
    out = []
    for use_graph in (False, True):
        agent = _agent(dev, torch.float16, 2, precise=precise)
        agent.use_graph = use_graph
        out.append(agent.generate_inflight(tok, reqs, **KW))
        out.append(agent.generate_inflight(tok, reqs, **KW))      # a second call reuses the buffers (and the captured step)
        assert (agent.llm._slot_graph is not None) == use_graph
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert torch.equal(a["generate_ids"], b["generate_ids"]) and torch.equal(a["last_hidden_states"], b["last_hidden_states"])
            assert (a["img_gen_feat"] is None) == (b["img_gen_feat"] is None)
            if a["img_gen_feat"] is not None:
                assert torch.equal(a["img_gen_feat"], b["img_gen_feat"])
    assert out[0][1]["num_gen_imgs"] == 1 and [len(x["generate_ids"]) for x in out[0]] == [9, 22, 4, 1, 7]


def test_tensor_parallel_is_refused(dev):
    agent = _agent(dev, torch.float16, 2)

    class TwoRanks:
        world, rank, graph_safe = 2, 0, False
    agent.llm.comm = TwoRanks()
    with pytest.raises(NotImplementedError):
        agent.generate_inflight(StubTokenizer(), [_req(0, 4)], **KW)
