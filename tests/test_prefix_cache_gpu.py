"""Prefix KV reuse of in-flight batching on the GPU: the slot-to-slot fork kernel (sx_kv_fork / ops.kv_fork, byte level and under the
decode step) and ContinuousLVLM.generate_inflight with ``agent.prefix_cache = True`` against the same engine with it off."""
import pytest
import torch

from oracle import weights

pytestmark = pytest.mark.gpu


def relerr(x, ref):
    x, ref = x.float().cpu(), ref.float().cpu()
    return ((x - ref).norm() / ref.norm()).item()


class StubTokenizer:
    """Ids are written as numbers; <img> = 400, <img_00000> .. = 401 .., </img> = 465 (the special tokens the engine asks for)."""
    eos_token_id = 2

    def encode(self, s, add_special_tokens=False):
        import re
        special = {"<img>": 400, "</img>": 465}
        return [special[t] if t in special else 401 + int(t[5:10]) if t.startswith("<img_") else int(t)
                for t in re.findall(r"<img_\d{5}>|<img>|</img>|\S+", s)]

    def decode(self, ids, skip_special_tokens=False):
        return " ".join(str(int(i)) for i in ids)

VIT = 128
KW = dict(num_img_gen_tokens=16, eos_token_id=None)
NCHUNK = 17                               # <img> + 16 forced image tokens: the rows a forced image block feeds in one chunk
_SD = {}


def _llm(dev, G, precise=None, **kw):
    from seedx_amd.llama import LlamaForCausalLM
    cfg = weights.MINI_LLM
    if not _SD:
        _SD["llm"], _SD["agent"] = weights.llama_sd(cfg), weights.agent_sd(cfg, VIT, in_grid=4, out_grid=4)
    llm = LlamaForCausalLM(dict(cfg), max_cache_len=512, max_batch=G, precise=precise, **kw)
    llm.load_state_dict(dict(_SD["llm"]))
    return llm


def _agent(dev, G, precise=None, **kw):
    from seedx_amd.seed_x import ContinuousLVLM
    from seedx_amd.visual_encoder import Resampler
    llm = _llm(dev, G, precise, **kw)
    H = weights.MINI_LLM["hidden_size"]
    agent = ContinuousLVLM(llm, Resampler(4, H, 2, kv_dim=VIT), Resampler(4, VIT, 2, kv_dim=H), add_patch_pos=True)
    agent.load_state_dict(_SD["agent"])
    agent.eval().to(dev, dtype=torch.float16)
    return agent


def _img_req(img, ids, budget, **kw):
    """ids = [1, x] + 16 image rows + text: an 18-token image prefix."""
    mask = torch.zeros(1, len(ids), dtype=torch.bool)
    mask[0, 2:18] = True
    return dict(input_ids=[list(ids)], image_embeds=img, embeds_cmp_mask=torch.tensor([True]), ids_cmp_mask=mask,
                patch_positions=torch.tensor([[0.5, 0.5]]), max_new_tokens=budget, **kw)


def _txt_req(ids, budget, **kw):
    return dict(input_ids=[list(ids)], max_new_tokens=budget, **kw)


def _ids(req):
    return req["input_ids"][0]


# ---- kernel level ------------------------------------------------------------------------------------------------------------------
PAIRS = [(0, 2, 7), (0, 3, 37), (1, 1, 5), (5, 2, 9), (0, 1, 0)]          # the last three are skipped by the kernel
VALID = PAIRS[:2]


def _check_fork(cache, before):
    for s, d, n in VALID:
        assert torch.equal(cache[:, d, :, :n], before[:, s, :, :n]), (s, d, n)
    want = before.clone()
    for s, d, n in VALID:
        want[:, d, :, :n] = before[:, s, :, :n]
    assert torch.equal(cache, want)          # every other byte is what it was: rows >= n, the other slots, the skipped pairs


@pytest.mark.parametrize("row_bytes", [4, 128, 256, 512])
def test_kv_fork_copies_exactly_the_prefix_bytes(dev, row_bytes):
    """[outer 2][G 4][inner 3][Tmax 37][row_bytes] random bytes. Tmax = 37 with 4-byte rows: a head's span starts at h * 148 bytes and
    slots lie 444 bytes apart, so spans start off 16-byte alignment, source and destination disagree modulo 16 and the 148-byte span
    ends on a 4-byte tail — the dword path; the wide rows take the 16-byte path."""
    from seedx_amd import ops
    g = torch.Generator().manual_seed(row_bytes)
    cache = torch.randint(0, 256, (2, 4, 3, 37, row_bytes), generator=g, dtype=torch.uint8).to(dev)
    before = cache.clone()
    assert ops.kv_fork(cache, PAIRS) == 1
    torch.cuda.synchronize()
    _check_fork(cache, before)


@pytest.mark.parametrize("row_bytes,Tmax,inner", [(4, 37, 3), (4, 38, 4), (128, 37, 3)])
def test_kv_fork_strided_outer_and_mixed_alignment(dev, row_bytes, Tmax, inner):
    """Layers [1:3] of a 4-layer tensor (a non-contiguous outer stride: layers 0 and 3 must stay as they are). (4, 38, 4): heads lie 152
    bytes and slots 608 = 38 * 16 bytes apart, so source and destination agree modulo 16 while odd heads start 8 bytes off: such a span
    has a dword head, a vector body and (7 rows = 28 bytes) a dword tail."""
    from seedx_amd import ops
    g = torch.Generator().manual_seed(7 + Tmax)
    full = torch.randint(0, 256, (4, 4, inner, Tmax, row_bytes), generator=g, dtype=torch.uint8).to(dev)
    pairs = [(s, d, min(n, Tmax)) for s, d, n in PAIRS]
    before = full.clone()
    ops.kv_fork(full[1:3], pairs)
    torch.cuda.synchronize()
    want = before.clone()
    for s, d, n in pairs[:2]:
        want[1:3, d, :, :n] = before[1:3, s, :, :n]
    assert torch.equal(full, want)
    assert not torch.equal(full, before)


def test_kv_fork_long_spans_run_every_loop_more_than_once(dev):
    """Spans many times the 16 KB a block moves per turn. [2][5][8][4096][512] bytes, four pairs: 64 spans of up to 2 MB and 64 blocks per
    span, so one turn of the quad loop moves 65536 vectors: 4096 rows (131072 vectors) are exactly two quad turns, 4001 rows (128032) one
    quad turn, a second one for part of the threads and the one-vector remainder loop for the rest, 3500 and 2999 rows one quad turn and
    up to three remainder turns. [2][4][3][4099][4] bytes: an odd Tmax puts the slots 4 bytes apart modulo 16, so the 4000 words of a
    span all take the dword loop, 512 per turn."""
    from seedx_amd import ops
    g = torch.Generator(device=dev).manual_seed(11)
    for shape, pairs in (((2, 5, 8, 4096, 512), [(0, 1, 4001), (0, 2, 4096), (0, 3, 2999), (0, 4, 3500)]),
                         ((2, 4, 3, 4099, 4), [(1, 0, 4000), (1, 3, 4099)])):
        cache = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8, device=dev)
        before = cache.clone()
        ops.kv_fork(cache, pairs)
        torch.cuda.synchronize()
        for s, d, n in pairs:
            before[:, d, :, :n] = before[:, s, :, :n]
        assert torch.equal(cache, before), shape


def test_kv_fork_wrapper_refusals(dev):
    from seedx_amd import ops
    cache = torch.zeros((2, 4, 3, 37, 128), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        ops.kv_fork(cache, [(0, 2, 5), (1, 2, 5)])                 # a slot receives two prefixes
    with pytest.raises(ValueError):
        ops.kv_fork(cache, [(0, 1, 5), (1, 2, 5)])                 # slot 1 is read and written
    with pytest.raises(ValueError):
        ops.kv_fork(cache, [(0, 1, 38)])                           # longer than the cache
    assert ops.kv_fork(cache, []) == 0


@pytest.mark.parametrize("mode", ["precise", "fp8_kv", "plain"])
def test_fork_then_decode_is_bit_exact(dev, mode):
    """A 20-token prompt prefilled into slot 0, its 20 rows forked to slot 2 (codes AND scales under the FP8 cache), slot 2's pos / ctx /
    cur set to slot 0's: one in-flight decode step gives bit-identical logits rows, hidden states and next ids for the two slots (decode
    rows do not depend on their slot), while the parked slots 1 and 3 write nothing."""
    from seedx_amd import ops
    kw = dict(precise=True, kv_format="fp8_e4m3") if mode == "fp8_kv" else dict(precise=(mode == "precise"))
    llm = _llm(dev, 4, **kw)
    llm.eval().to(dev, torch.float16)
    P = llm._pack()
    assert (llm.kv_format == "fp8_e4m3") == (mode == "fp8_kv") and llm.precise == (mode != "plain")
    T = 20
    x = torch.randn(T, llm.H, generator=torch.Generator().manual_seed(3)) * 0.5
    st = llm.slot_state(force_id=400, eos_id=-1)
    llm._slot_write(P["pos"], [0], 0)
    llm._slot_write(P["ctx"], [0], 1)
    logits, _ = llm.forward_embeds_batch([x.to(dev)], [0])
    cur = int(logits[0, :llm.V].argmax().item())
    n_tensors = ops.kv_fork(P, [(0, 2, T)])
    assert n_tensors == (4 if mode == "fp8_kv" else 2)
    for k in ops.KV_CACHE_KEYS:
        if P.get(k) is not None:
            assert torch.equal(P[k][:, 2, :, :T], P[k][:, 0, :, :T]) and bool((P[k][:, 0, :, :T] != 0).any()), k
            assert not bool(P[k][:, 1].any()) and not bool(P[k][:, 3].any()) and not bool(P[k][:, 2, :, T:].any()), k
    two = [0, 2]
    llm._slot_write(P["pos"], two, T)
    llm._slot_write(P["ctx"], two, T + 1)
    llm._slot_write(P["cur"], two, cur)
    llm._slot_write(P["step"], two, 1)
    llm._slot_write(st.n_new, two, 1)
    llm._slot_write(st.max_new, two, 8)
    llm._slot_write(st.live, two, 1)
    img_ids_dev = torch.tensor([400] + list(range(401, 417)) + [465], dtype=torch.int32, device=dev)
    out_ids = torch.full((4, 16), -1, dtype=torch.int32, device=dev)
    hid = torch.zeros((4, 16, llm.H), dtype=torch.float32, device=dev)
    llm.decode_step(img_ids_dev, out_ids, hid, use_graph=False, slots=st)
    torch.cuda.synchronize()
    assert torch.isfinite(st.logits[0]).all() and bool(hid[0, 1].any())
    assert torch.equal(st.logits[0], st.logits[2])
    assert torch.equal(hid[0], hid[2]) and torch.equal(out_ids[0], out_ids[2]) and out_ids[0, 1].item() >= 0
    assert P["pos"].tolist() == [T + 1, -1, T + 1, -1]
    for k in ops.KV_CACHE_KEYS:
        if P.get(k) is not None:
            assert torch.equal(P[k][:, 2], P[k][:, 0]) and not bool(P[k][:, 1].any()) and not bool(P[k][:, 3].any()), k


# ---- engine level ------------------------------------------------------------------------------------------------------------------
def _serve(agent, tok, reqs, prefix, **kw):
    agent.prefix_cache = prefix
    out = agent.generate_inflight(tok, reqs, **dict(KW, **kw))
    return out, dict(agent.last_inflight_stats), list(agent.last_prefill_tokens)


def _queue(dev, plain):
    """10 requests: three questions about one image (18-token image prefix + 4 different ids; request 1 emits an image block), two
    unrelated prompts, the second turns of the three (first prompt + first answer + 3 new ids) and the third turns of two of them. The
    answers come from the uncached engine ``plain`` (greedy: every later run produces them again)."""
    tok = StubTokenizer()
    img = torch.randn(1, 36, VIT, generator=torch.Generator().manual_seed(44)).to(dev)
    head = [1, 30] + [0] * 16
    first = [_img_req(img, head + [31 + 10 * k + i for i in range(4)], b, **f)
             for k, (b, f) in enumerate(((8, {}), (24, dict(force_image_at=3)), (6, {})))]
    other = [_txt_req([1, 70, 71, 72, 73, 74, 75], 5), _txt_req([1, 80, 81, 82, 83, 84, 85, 86, 87], 12)]
    ans1, _, _ = _serve(plain, tok, first, False)
    second = [_img_req(img, _ids(first[k]) + ans1[k]["generate_ids"].tolist() + [50 + k, 51, 52], b) for k, b in enumerate((6, 5, 7))]
    ans2, _, _ = _serve(plain, tok, second, False)
    third = [_img_req(img, _ids(second[k]) + ans2[k]["generate_ids"].tolist() + [60 + k, 61], b) for k, b in ((0, 4), (2, 9))]
    return tok, first + other + second + third


@pytest.mark.parametrize("precise", [False, True])
def test_prefix_cache_engine_equals_uncached_engine(dev, precise):
    """generate_inflight with the prefix cache against the same engine without: identical ids per request, hidden states and image
    features within 1e-3 (the bound of test_cross_turn_kv_reuse_equals_full_reprefill for the same comparison: reused rows were written
    by a pass of another shape), equal step counts, the counters inflight.simulate_prefix predicts from the produced ids, and fewer
    prefilled tokens. The uncached call before and after (the default path) is bit-identical to itself."""
    from seedx_amd.inflight import simulate_prefix
    agent = _agent(dev, 4, precise=precise)
    tok, reqs = _queue(dev, agent)
    assert len(reqs) == 10
    ref, ref_stats, ref_prefill = _serve(agent, tok, reqs, False)
    assert ref_prefill == [len(_ids(q)) for q in reqs] and "prefix_hit_tokens" not in ref_stats and "fork_launches" not in ref_stats
    got, stats, prefill = _serve(agent, tok, reqs, True)
    assert ref[1]["num_gen_imgs"] == 1 and ref[1]["generate_ids"].tolist()[3:21] == [400] + list(range(401, 417)) + [465]
    for r in range(10):
        a, b = got[r], ref[r]
        print(f"request {r}: hidden relerr {relerr(a['last_hidden_states'], b['last_hidden_states']):.2e}")
        assert a["generate_ids"].tolist() == b["generate_ids"].tolist(), r
        assert len(a["generate_ids"]) == reqs[r]["max_new_tokens"]
        assert relerr(a["last_hidden_states"], b["last_hidden_states"]) < 1e-3, r
        assert (a["img_gen_feat"] is None) == (b["img_gen_feat"] is None) and a["text"] == b["text"]
        if b["img_gen_feat"] is not None:
            assert relerr(a["img_gen_feat"], b["img_gen_feat"]) < 1e-3, r
    assert stats["decode_steps"] == ref_stats["decode_steps"]
    generated = [x["generate_ids"].tolist() for x in got]
    lengths = [len(ids) - NCHUNK * ids.count(400) for ids in generated]
    want = simulate_prefix([_ids(q) for q in reqs], lengths, 4, min_tokens=agent.prefix_min_tokens, generated=generated)
    for k in ("decode_steps", "live_slot_steps", "parked_slot_steps", "admissions", "prefill_passes", "prefill_tokens",
              "prefix_hit_tokens", "forked_tokens", "fork_launches"):
        assert stats[k] == want[k], (k, stats, want)
    assert stats["prefill_tokens"] == sum(prefill) < ref_stats["prefill_tokens"] == sum(ref_prefill)
    assert stats["prefill_tokens"] + stats["prefix_hit_tokens"] == sum(ref_prefill)
    assert stats["fork_launches"] >= 1 and stats["forked_tokens"] >= 2 * 18       # the two other questions about the image fork its 18 rows
    # the default path after a cached call: what it was before (ids, states, statistics, prefill lengths)
    again, again_stats, again_prefill = _serve(agent, tok, reqs, False)
    assert again_stats == ref_stats and again_prefill == ref_prefill
    for a, b in zip(again, ref):
        assert torch.equal(a["generate_ids"], b["generate_ids"]) and torch.equal(a["last_hidden_states"], b["last_hidden_states"])
    assert torch.equal(again[1]["img_gen_feat"], ref[1]["img_gen_feat"])


def test_records_survive_a_call_and_die_on_an_outside_write(dev):
    agent, tok = _agent(dev, 4), StubTokenizer()
    reqs = [_txt_req([1, 10 + r] + [20 + 7 * r + i for i in range(5 + r)], 4 + r) for r in range(3)]
    full = [len(_ids(q)) for q in reqs]
    a, _, prefill = _serve(agent, tok, reqs, True)
    assert prefill == full
    b, stats, prefill = _serve(agent, tok, reqs, True)
    assert prefill == [1, 1, 1] and stats["prefix_hit_tokens"] == sum(full) - 3 and stats["forked_tokens"] == 0
    for x, y in zip(a, b):
        assert x["generate_ids"].tolist() == y["generate_ids"].tolist()
        assert relerr(y["last_hidden_states"], x["last_hidden_states"]) < 1e-3
    agent.llm.forward(input_ids=torch.tensor([[1, 2, 3]]))          # someone else writes the cache
    c, stats, prefill = _serve(agent, tok, reqs, True)
    assert prefill == full and stats["prefix_hit_tokens"] == 0
    for x, y in zip(a, c):
        assert x["generate_ids"].tolist() == y["generate_ids"].tolist()
    # generate_batch rewrites the slots too (its own records are another book)
    agent.generate_batch(tok, [{k: v for k, v in q.items() if k != "max_new_tokens"} for q in reqs] + [dict(input_ids=[[1, 5, 6]])],
                         max_new_tokens=3, reuse_cache=True, **KW)
    _, _, prefill = _serve(agent, tok, reqs, True)
    assert prefill == full


def test_a_changed_image_is_not_a_hit(dev):
    """Same ids, other image features: the reusable prefix ends at the first image row (2 tokens)."""
    agent, tok = _agent(dev, 4), StubTokenizer()
    g = torch.Generator().manual_seed(45)
    img_a, img_b = (torch.randn(1, 36, VIT, generator=g).to(dev) for _ in range(2))
    ids = [1, 30] + [0] * 16 + [31, 32, 33, 34]
    _serve(agent, tok, [_img_req(img_a, ids, 5)], True)
    _, stats, prefill = _serve(agent, tok, [_img_req(img_b, ids, 5)], True)
    assert prefill == [len(ids) - 2] and stats["prefix_hit_tokens"] == 2
    _, stats, prefill = _serve(agent, tok, [_img_req(img_b, ids + [35], 5)], True)
    assert prefill == [1] and stats["prefix_hit_tokens"] == len(ids)                 # the same image again: everything but the new id


def test_same_prompt_under_four_seeds(dev):
    """Four copies of one prompt, do_sample with seeds s .. s + 3, in one call: one full prefill, then three 1-token suffixes on rows forked
    from the leader's slot; every request's ids are those of the same request served alone without the cache."""
    agent, tok = _agent(dev, 4, precise=True), StubTokenizer()
    ids = [1, 30] + [40 + i for i in range(20)]
    s0 = 1234
    reqs = [_txt_req(ids, 9, do_sample=True, temperature=0.9, top_k=40, top_p=0.95, seed=s0 + i) for i in range(4)]
    got, stats, prefill = _serve(agent, tok, reqs, True)
    assert stats["prefill_passes"] == 2 and prefill == [len(ids), 1, 1, 1] and stats["prefill_tokens"] == len(ids) + 3
    assert stats["fork_launches"] >= 1 and stats["forked_tokens"] == 3 * (len(ids) - 1)
    assert [x["seed"] for x in got] == [s0 + i for i in range(4)]
    alone = [_serve(agent, tok, [q], False)[0][0] for q in reqs]
    for i in range(4):
        assert got[i]["generate_ids"].tolist() == alone[i]["generate_ids"].tolist(), i
        assert relerr(got[i]["last_hidden_states"], alone[i]["last_hidden_states"]) < 1e-3
    assert len({tuple(x["generate_ids"].tolist()) for x in got}) > 1                  # the seeds do matter
