"""Host-memory tier of the prefix cache on the GPU: the pack / unpack kernel (sx_kv_rows_copy / ops.kv_rows_copy: byte level, and a spill
to pinned host memory and back under the decode step) and ContinuousLVLM.generate_inflight with ``agent.prefix_host_bytes`` against the
same engine without the tier and without the prefix cache."""
import pytest
import torch

from oracle import weights

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
HOST_KEYS = ("host_spills", "host_spill_tokens", "host_restores", "host_restore_tokens", "host_evictions", "host_bytes_peak")


def relerr(x, ref):
    x, ref = x.float().cpu(), ref.float().cpu()
    return ((x - ref).norm() / ref.norm()).item()


# ---- kernel level ------------------------------------------------------------------------------------------------------------------
FORMATS = {"mixed": [(512, torch.float32), (256, torch.float16)],                      # fp32 k, 16-bit v at head_dim 128
           "fp8": [(128, torch.uint8), (128, torch.uint8), (4, torch.float32), (4, torch.float32)]}     # codes and row scales


def _caches(dev, fmt, Tmax, seed, layers=2, G=3, heads=3, fill=None, lo=0):
    """(raw, typed): per cache tensor the bytes [layers][G][heads][Tmax][row_bytes] and the view the engine would hold (row scales 4-D).
    ``lo`` > 0: the tensors are layers [lo, lo + layers) of a tensor two layers larger (a strided outer axis)."""
    g = torch.Generator().manual_seed(seed)
    raw, typed, full = [], [], []
    for rb, dt in FORMATS[fmt]:
        shape = (layers + 2 * lo, G, heads, Tmax, rb)
        t = (torch.randint(0, 256, shape, generator=g, dtype=torch.uint8) if fill is None else torch.full(shape, fill, dtype=torch.uint8)).to(dev)
        full.append(t)
        t = t[lo:lo + layers]
        raw.append(t)
        v = t.view(dt)
        typed.append(v.squeeze(-1) if rb == 4 else v)
    return raw, typed, full


def _layout(raw, jobs, size):
    """The staging buffer built by plain indexing: job (slot, n, offset) = spans [tensor][outer][inner] of n * row_bytes bytes, each
    padded to a multiple of 16; everything else keeps the sentinel."""
    want = torch.full((size,), SENTINEL, dtype=torch.uint8)
    G, Tmax = raw[0].shape[1], raw[0].shape[3]
    for slot, n, off in jobs:
        if not 0 <= slot < G or n <= 0:
            continue
        n = min(n, Tmax)
        for t in raw:
            for o in range(t.shape[0]):
                for h in range(t.shape[2]):
                    span = t[o, slot, h, :n].reshape(-1).cpu()
                    want[off:off + span.numel()] = span
                    off += (span.numel() + 15) // 16 * 16
    return want


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("Tmax", [37, 64])
@pytest.mark.parametrize("fmt", ["mixed", "fp8"])
def test_pack_and_unpack_layout(dev, fmt, Tmax, strided):
    """L 2, G 3, 3 heads. Tmax 37: the 148-byte scale rows of odd heads and slots start 4 or 8 bytes off 16-byte alignment and take the
    dword path, every other span the 16-byte path with (n = 1: 4 bytes) a dword tail. Jobs of 1, Tmax and 20 rows, one skipped for its
    slot and one for n = 0; their offsets lie inside the buffer, so a job that is not skipped would show."""
    from seedx_amd import ops
    raw, typed, full = _caches(dev, fmt, Tmax, 5 + Tmax, lo=1 if strided else 0)
    size = [ops.kv_rows_bytes(typed, n) for n in (1, Tmax, 20)]
    assert size[2] == sum(2 * 3 * ((20 * rb + 15) // 16 * 16) for rb, _ in FORMATS[fmt])
    offs = [16, 16 + size[0] + 32, 16 + size[0] + 32 + size[1]]              # gaps in front, between and behind
    total = offs[2] + size[2] + 48
    jobs = [(0, 1, offs[0]), (2, Tmax, offs[1]), (1, 20, offs[2]), (7, 5, 0), (1, 0, 16)]
    staging = torch.full((total,), SENTINEL, dtype=torch.uint8, device=dev)
    before = [t.clone() for t in full]
    assert ops.kv_rows_copy(typed, jobs, staging, 0) == 1
    torch.cuda.synchronize()
    assert torch.equal(staging.cpu(), _layout(raw, jobs, total))
    assert all(torch.equal(a, b) for a, b in zip(full, before))              # a pack writes no cache byte
    # unpack into other slots of a sentinel-filled cache: exactly those rows change, and they are the source rows
    raw2, typed2, full2 = _caches(dev, fmt, Tmax, 0, fill=SENTINEL, lo=1 if strided else 0)
    moves = [(0, 1), (2, 0), (1, 2)]                                         # source slot -> destination slot, job by job
    back = [(d, n, off) for (_, n, off), (_, d) in zip(jobs[:3], moves)] + [(-1, 5, 0), (0, -2, 16)]
    staged = staging.clone()
    ops.kv_rows_copy(typed2, back, staging, 1)
    torch.cuda.synchronize()
    assert torch.equal(staging, staged)                                      # an unpack writes no staging byte
    for a, f, src in zip(raw2, full2, raw):
        want = torch.full_like(f, SENTINEL)
        lo = 1 if strided else 0
        for (s, n, _), (_, d) in zip(jobs[:3], moves):
            want[lo:lo + 2, d, :, :n] = src[:, s, :, :n]
        assert torch.equal(f, want)
        assert not torch.equal(a, torch.full_like(a, SENTINEL))


@pytest.mark.parametrize("misaligned", [False, True])
def test_long_spans_run_every_loop_more_than_once(dev, misaligned):
    """One job of 1500 rows of 512 bytes (48000 vectors a span) on [4][2][20][1536] x two tensors = 160 spans: 26 blocks per span, so a
    turn of the quad loop moves 4 x 6656 vectors — one turn for every thread, a second one for the first 1408, up to three turns of the
    one-vector loop for the rest. ``misaligned``: the same tensors start 4 bytes off 16-byte alignment, so no span shares the staging
    buffer's alignment and all 192000 words of a span take the dword loop, 6656 per turn."""
    from seedx_amd import ops
    g = torch.Generator(device=dev).manual_seed(12)
    shape, numel = (4, 2, 20, 1536, 512), 4 * 2 * 20 * 1536 * 512
    flat = [torch.randint(0, 256, (numel + 16,), generator=g, dtype=torch.uint8, device=dev) for _ in range(2)]
    lo = 4 if misaligned else 0
    caches = [f[lo:lo + numel].view(shape) for f in flat]
    assert all(c.data_ptr() % 16 == lo for c in caches)
    size = ops.kv_rows_bytes(caches, 1500)
    assert size == 160 * 1500 * 512
    staging = torch.full((size + 64,), SENTINEL, dtype=torch.uint8, device=dev)
    ops.kv_rows_copy(caches, [(1, 1500, 32)], staging, 0)
    for i, c in enumerate(caches):
        part = staging[32 + i * size // 2:32 + (i + 1) * size // 2].view(4, 20, 1500, 512)
        assert torch.equal(part, c[:, 1, :, :1500]), i
    assert bool((staging[:32] == SENTINEL).all()) and bool((staging[32 + size:] == SENTINEL).all())
    before = [f.clone() for f in flat]
    ops.kv_rows_copy(caches, [(0, 1500, 32)], staging, 1)                    # the round trip: slot 1's rows arrive in slot 0
    torch.cuda.synchronize()
    for f, b, c in zip(flat, before, caches):
        assert torch.equal(c[:, 0, :, :1500], c[:, 1, :, :1500])
        want = b[lo:lo + numel].view(shape).clone()
        want[:, 0, :, :1500] = want[:, 1, :, :1500]
        assert torch.equal(c, want) and torch.equal(f[:lo], b[:lo]) and torch.equal(f[lo + numel:], b[lo + numel:])


def test_kv_rows_copy_refusals(dev):
    from seedx_amd import ops
    _, typed, _ = _caches(dev, "fp8", 37, 1)
    size = ops.kv_rows_bytes(typed, 5)
    staging = torch.zeros(4 * size, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="unpacked into twice"):
        ops.kv_rows_copy(typed, [(1, 5, 0), (1, 5, size)], staging, 1)
    assert ops.kv_rows_copy(typed, [(1, 5, 0), (1, 5, size)], staging, 0) == 1           # packing a slot twice is fine
    with pytest.raises(ValueError, match="longer than the cache"):
        ops.kv_rows_copy(typed, [(0, 38, 0)], staging, 0)
    with pytest.raises(ValueError, match="overlap"):
        ops.kv_rows_copy(typed, [(0, 5, 0), (1, 5, size - 16)], staging, 0)
    with pytest.raises(RuntimeError, match="ends at byte"):                              # staging too small for the jobs
        ops.kv_rows_copy(typed, [(0, 5, 0), (1, 5, size)], staging[:2 * size - 16], 0)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        ops.kv_rows_copy(typed, [(0, 5, 8)], staging, 0)
    with pytest.raises(RuntimeError, match="n_tensors=5"):
        ops.kv_rows_copy(typed + typed[:1], [(0, 5, 0)], staging, 0)
    torch.cuda.synchronize()
    assert ops.kv_rows_copy(typed, [], staging, 0) == 0


# ---- under the decode step ---------------------------------------------------------------------------------------------------------
VIT = 128
KW = dict(num_img_gen_tokens=16, eos_token_id=None)
NCHUNK = 17
_SD = {}


def _llm(dev, G, precise=None, **kw):
    from seedx_amd.llama import LlamaForCausalLM
    cfg = weights.MINI_LLM
    if not _SD:
        _SD["llm"], _SD["agent"] = weights.llama_sd(cfg), weights.agent_sd(cfg, VIT, in_grid=4, out_grid=4)
    llm = LlamaForCausalLM(dict(cfg), max_cache_len=512, max_batch=G, precise=precise, **kw)
    llm.load_state_dict(dict(_SD["llm"]))
    return llm


def _prefill_then_step(dev, mode, via_host):
    """A 20-token prompt prefilled into slot 0 of a 4-slot LLM; its rows reach slot 2 by a device fork (the twin) or, ``via_host``, by
    pack -> pinned host memory -> every cache tensor zeroed -> back -> unpack into slots 0 and 2. Then one in-flight decode step of the
    two slots."""
    from seedx_amd import ops
    kw = dict(precise=True, kv_format="fp8_e4m3") if mode == "fp8_kv" else dict(precise=(mode == "precise"))
    llm = _llm(dev, 4, **kw)
    llm.eval().to(dev, torch.float16)
    P = llm._pack()
    caches = [P[k] for k in ops.KV_CACHE_KEYS if P.get(k) is not None]
    assert len(caches) == (4 if mode == "fp8_kv" else 2)
    assert llm.kv_row_bytes == sum(t[:, 0, :, 0].numel() * t.element_size() for t in caches)
    assert llm.memory_footprint()["kv_cache"] == llm.G * llm.Tmax * llm.kv_row_bytes
    T = 20
    x = torch.randn(T, llm.H, generator=torch.Generator().manual_seed(3)) * 0.5
    st = llm.slot_state(force_id=400, eos_id=-1)
    llm._slot_write(P["pos"], [0], 0)
    llm._slot_write(P["ctx"], [0], 1)
    logits, _ = llm.forward_embeds_batch([x.to(dev)], [0])
    cur = int(logits[0, :llm.V].argmax().item())
    if via_host:
        size = ops.kv_rows_bytes(P, T)
        staging = torch.zeros(2 * size, dtype=torch.uint8, device=dev)
        ops.kv_rows_copy(P, [(0, T, 0)], staging, 0)
        host = torch.empty(size, dtype=torch.uint8, pin_memory=True)
        host.copy_(staging[:size])
        assert bool(host.any())
        for t in caches:
            t.zero_()
        staging.zero_()
        staging[:size].copy_(host)
        staging[size:].copy_(host)
        ops.kv_rows_copy(P, [(0, T, 0), (2, T, size)], staging, 1)
    else:
        ops.kv_fork(P, [(0, 2, T)])
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
    return st.logits.clone(), hid, out_ids, [t.clone() for t in caches]


@pytest.mark.parametrize("mode", ["precise", "fp8_kv", "plain"])
def test_spill_overwrite_restore_then_decode_is_bit_exact(dev, mode):
    twin = _prefill_then_step(dev, mode, False)
    got = _prefill_then_step(dev, mode, True)
    for s in (0, 2):
        assert torch.isfinite(got[0][s]).all() and bool(got[1][s, 1].any()) and got[2][s, 1].item() >= 0
        assert torch.equal(got[0][s], twin[0][s]) and torch.equal(got[1][s], twin[1][s]) and torch.equal(got[2][s], twin[2][s]), s
    for a, b in zip(got[3], twin[3]):
        assert not bool(a[:, 1].any()) and not bool(a[:, 3].any())          # the parked slots stay all zero
        assert torch.equal(a[:, 0, :, :21], b[:, 0, :, :21]) and torch.equal(a[:, 2], a[:, 0])


# ---- engine level ------------------------------------------------------------------------------------------------------------------
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


def _agent(dev, G, precise=None, **kw):
    from seedx_amd.seed_x import ContinuousLVLM
    from seedx_amd.visual_encoder import Resampler
    llm = _llm(dev, G, precise, **kw)
    H = weights.MINI_LLM["hidden_size"]
    agent = ContinuousLVLM(llm, Resampler(4, H, 2, kv_dim=VIT), Resampler(4, VIT, 2, kv_dim=H), add_patch_pos=True)
    agent.load_state_dict(_SD["agent"])
    agent.eval().to(dev, dtype=torch.float16)
    return agent


def _img_req(img, ids, budget):
    """ids = [1, x] + 16 image rows + text: an 18-token image prefix."""
    mask = torch.zeros(1, len(ids), dtype=torch.bool)
    mask[0, 2:18] = True
    return dict(input_ids=[list(ids)], image_embeds=img, embeds_cmp_mask=torch.tensor([True]), ids_cmp_mask=mask,
                patch_positions=torch.tensor([[0.5, 0.5]]), max_new_tokens=budget)


def _txt_req(ids, budget):
    return dict(input_ids=[list(ids)], max_new_tokens=budget)


def _ids(req):
    return req["input_ids"][0]


def _serve(agent, tok, reqs, prefix, host_bytes=0, forget=True):
    """One call. ``forget``: the device records of earlier calls are ended first (an outside reset moves the epoch) and their last-use
    stamps go with them, so the call starts like the simulator does, from an empty index."""
    if forget:
        agent.llm.reset()
        if agent._inflight is not None:
            agent._inflight["prefix"] = None
    agent.prefix_cache, agent.prefix_host_bytes, agent.prefix_host_min_tokens = prefix, host_bytes, 8
    out = agent.generate_inflight(tok, reqs, **KW)
    return out, dict(agent.last_inflight_stats), list(agent.last_prefill_tokens)


def _simulated(agent, reqs, got, sigs, **kw):
    from seedx_amd.inflight import simulate_prefix
    generated = [x["generate_ids"].tolist() for x in got]
    lengths = [len(ids) - NCHUNK * ids.count(400) for ids in generated]
    return simulate_prefix([_ids(q) for q in reqs], lengths, agent.llm.G, min_tokens=agent.prefix_min_tokens, generated=generated, sigs=sigs,
                           host_min_tokens=8, row_bytes=agent.llm.kv_row_bytes, **kw)


def _image_sigs(reqs, tags):
    """Row signatures for the simulator: the ids, with the 16 image rows of request i replaced by its image's tag (None: a text prompt)."""
    return [_ids(q) if t is None else _ids(q)[:2] + [t] * 16 + _ids(q)[18:] for q, t in zip(reqs, tags)]


SIM_KEYS = ("decode_steps", "live_slot_steps", "parked_slot_steps", "admissions", "prefill_passes", "prefill_tokens", "prefix_hit_tokens",
            "forked_tokens", "fork_launches") + HOST_KEYS


def _conversation_queue(dev, agent, tok):
    """A1 (18-row image prefix + 4 ids), three unrelated text prompts that overwrite both slots, then A2 = A1 + its answer + 3 ids. The
    answer comes from the uncached engine (greedy: every later run produces it again)."""
    img = torch.randn(1, 36, VIT, generator=torch.Generator().manual_seed(44)).to(dev)
    a1 = _img_req(img, [1, 30] + [0] * 16 + [31, 32, 33, 34], 2)
    other = [_txt_req([1, 70, 71, 72, 73, 74], 6), _txt_req([1, 80, 81, 82, 83, 84], 2), _txt_req([1, 90, 91, 92, 93, 94], 2)]
    ans, _, _ = _serve(agent, tok, [a1], False)
    a2 = _img_req(img, _ids(a1) + ans[0]["generate_ids"].tolist() + [50, 51, 52], 3)
    return [a1] + other + [a2], ["img", None, None, None, "img"]


def _same_results(got, ref, reqs):
    for r, (a, b) in enumerate(zip(got, ref)):
        print(f"request {r}: hidden relerr {relerr(a['last_hidden_states'], b['last_hidden_states']):.2e}")
        assert a["generate_ids"].tolist() == b["generate_ids"].tolist(), r
        assert len(a["generate_ids"]) == reqs[r]["max_new_tokens"]
        assert relerr(a["last_hidden_states"], b["last_hidden_states"]) < 1e-3, r
        assert (a["img_gen_feat"] is None) == (b["img_gen_feat"] is None) and a["text"] == b["text"]
        if b["img_gen_feat"] is not None:
            assert relerr(a["img_gen_feat"], b["img_gen_feat"]) < 1e-3, r


@pytest.mark.parametrize("precise", [False, True])
def test_host_tier_engine_equals_uncached_engine(dev, precise):
    """2 slots. A1's 23 rows (22 prompt rows + the fed id) are spilled when an unrelated prompt takes its slot, and restored for A2 after
    three unrelated prompts went through both slots: identical ids per request, states within 1e-3 of the uncached engine (the bound of
    test_prefix_cache_engine_equals_uncached_engine for this comparison: reused rows were written by a pass of another shape), equal
    decode steps, fewer prefilled tokens than the prefix cache alone manages, and every counter as inflight.simulate_prefix predicts it."""
    agent, tok = _agent(dev, 2, precise=precise), StubTokenizer()
    reqs, tags = _conversation_queue(dev, agent, tok)
    sigs = _image_sigs(reqs, tags)
    ref, ref_stats, ref_prefill = _serve(agent, tok, reqs, False)
    assert ref_prefill == [len(_ids(q)) for q in reqs]
    dev_only, dev_stats, _ = _serve(agent, tok, reqs, True)
    assert not set(HOST_KEYS) & set(dev_stats)
    got, stats, prefill = _serve(agent, tok, reqs, True, host_bytes=1 << 30)
    _same_results(got, ref, reqs)
    _same_results(dev_only, ref, reqs)
    assert stats["decode_steps"] == ref_stats["decode_steps"] == dev_stats["decode_steps"]
    assert stats["host_restores"] >= 1 and stats["host_restore_tokens"] >= 23 and stats["host_spills"] >= 1
    assert stats["prefill_tokens"] == sum(prefill) < dev_stats["prefill_tokens"] < ref_stats["prefill_tokens"]
    assert stats["prefill_tokens"] + stats["prefix_hit_tokens"] == sum(ref_prefill)
    want = _simulated(agent, reqs, got, sigs, host_bytes=1 << 30)
    for k in SIM_KEYS:
        assert stats[k] == want[k], (k, stats, want)
    assert stats["host_bytes_peak"] == stats["host_spill_tokens"] * agent.llm.kv_row_bytes      # nothing evicted, nothing replaced
    want_dev = _simulated(agent, reqs, dev_only, sigs)
    for k in SIM_KEYS[:9]:
        assert dev_stats[k] == want_dev[k], (k, dev_stats, want_dev)


def test_a_shorter_prefix_of_an_entry_is_restored(dev):
    """Another question about A's image after A's slot was overwritten: the 23-row entry agrees with it on the 18 rows of the image
    prefix only, and those 18 rows — the heads of the entry's spans — are restored."""
    agent, tok = _agent(dev, 2), StubTokenizer()
    reqs, tags = _conversation_queue(dev, agent, tok)
    reqs[4] = dict(reqs[0], input_ids=[_ids(reqs[0])[:18] + [41, 42, 43, 44, 45]], ids_cmp_mask=torch.cat(
        [reqs[0]["ids_cmp_mask"], torch.zeros(1, 1, dtype=torch.bool)], 1), max_new_tokens=3)
    ref, ref_stats, _ = _serve(agent, tok, reqs, False)
    got, stats, prefill = _serve(agent, tok, reqs, True, host_bytes=1 << 30)
    _same_results(got, ref, reqs)
    assert stats["host_restores"] == 1 and stats["host_restore_tokens"] == 18 and prefill[4] == 5
    want = _simulated(agent, reqs, got, _image_sigs(reqs, tags), host_bytes=1 << 30)
    for k in SIM_KEYS:
        assert stats[k] == want[k], (k, stats, want)


def test_host_tier_with_speculative_decoding(dev):
    """The conversation queue on an LLM built with spec_tokens = 3 and agent.speculative: the verify step writes draft rows past a slot's
    last token, the records (and so the spilled rows) end where the fed ids end. Ids as without any cache, A2 restored."""
    agent, tok = _agent(dev, 2, precise=True, spec_tokens=3), StubTokenizer()
    reqs, _ = _conversation_queue(dev, agent, tok)
    ref, _, _ = _serve(agent, tok, reqs, False)
    agent.speculative = True
    got, stats, prefill = _serve(agent, tok, reqs, True, host_bytes=1 << 30)
    assert [x["generate_ids"].tolist() for x in got] == [x["generate_ids"].tolist() for x in ref]
    assert stats["spec_steps"] >= 1 and stats["host_restores"] == 1 and stats["host_restore_tokens"] == 23 and prefill[4] == 4


def test_host_tier_under_a_budget_for_one_entry(dev):
    """Two conversations, four unrelated prompts through both slots, then the second turns, on a budget of 24 rows: B's 23-row record
    evicts A's, A2 finds nothing, B2 is restored. Ids as without any cache; the counters are the simulator's."""
    agent, tok = _agent(dev, 2), StubTokenizer()
    g = torch.Generator().manual_seed(46)
    imgs = [torch.randn(1, 36, VIT, generator=g).to(dev) for _ in range(2)]
    first = [_img_req(imgs[k], [1, 30 + 10 * k] + [0] * 16 + [31 + 10 * k + i for i in range(4)], 2) for k in range(2)]
    other = [_txt_req([1] + [70 + 10 * k + i for i in range(5)], 2) for k in range(4)]
    ans, _, _ = _serve(agent, tok, first, False)
    second = [_img_req(imgs[k], _ids(first[k]) + ans[k]["generate_ids"].tolist() + [60 + k, 61, 62], 2) for k in range(2)]
    reqs, tags = first + other + second, ["a", "b", None, None, None, None, "a", "b"]
    ref, ref_stats, _ = _serve(agent, tok, reqs, False)
    budget = 24 * agent.llm.kv_row_bytes
    got, stats, _ = _serve(agent, tok, reqs, True, host_bytes=budget)
    for a, b in zip(got, ref):
        assert a["generate_ids"].tolist() == b["generate_ids"].tolist()
        assert relerr(a["last_hidden_states"], b["last_hidden_states"]) < 1e-3
    assert stats["host_evictions"] >= 1 and stats["host_bytes_peak"] <= budget and stats["decode_steps"] == ref_stats["decode_steps"]
    want = _simulated(agent, reqs, got, _image_sigs(reqs, tags), host_bytes=budget)
    for k in SIM_KEYS:
        assert stats[k] == want[k], (k, stats, want)
    assert want["host_restores"] == 1 and want["host_spills"] == 2


def test_host_entries_survive_reset_and_outside_writes(dev):
    """After a call, llm.reset() from outside ends every device record (the existing behaviour: the next call keeps no row in place);
    the host entry still gives its hit, in a new call."""
    agent, tok = _agent(dev, 2), StubTokenizer()
    reqs, _ = _conversation_queue(dev, agent, tok)
    ref, _, _ = _serve(agent, tok, reqs, False)
    _, stats, _ = _serve(agent, tok, reqs[:4], True, host_bytes=1 << 30)
    assert stats["host_spills"] >= 1 and stats["host_restores"] == 0
    agent.llm.reset()
    agent.llm.forward(input_ids=torch.tensor([[1, 2, 3]]))                   # ... and someone else writes the cache
    got, stats, prefill = _serve(agent, tok, reqs[4:], True, host_bytes=1 << 30, forget=False)
    assert stats["host_restores"] == 1 and stats["host_restore_tokens"] == 23 and stats["forked_tokens"] == 0
    assert stats["prefix_hit_tokens"] == 23 and prefill == [len(_ids(reqs[4])) - 23]       # the hit is the host's alone
    assert got[0]["generate_ids"].tolist() == ref[4]["generate_ids"].tolist()
    assert relerr(got[0]["last_hidden_states"], ref[4]["last_hidden_states"]) < 1e-3
    # without the tier the same call finds nothing
    agent.llm.reset()
    _, stats, prefill = _serve(agent, tok, reqs[4:], True, forget=False)
    assert stats["prefix_hit_tokens"] == 0 and prefill == [len(_ids(reqs[4]))]


def test_default_path_is_untouched_by_a_tiered_call(dev):
    """prefix_host_bytes = 0 before and after a tiered call: bit-identical results, equal statistics, none of the new keys — for the
    call without the prefix cache and for the call with it."""
    agent, tok = _agent(dev, 2), StubTokenizer()
    reqs, _ = _conversation_queue(dev, agent, tok)
    before = [_serve(agent, tok, reqs, prefix) for prefix in (False, True)]
    _, stats, _ = _serve(agent, tok, reqs, True, host_bytes=1 << 30)
    assert stats["host_restores"] >= 1
    after = [_serve(agent, tok, reqs, prefix) for prefix in (False, True)]
    for (a, a_stats, a_prefill), (b, b_stats, b_prefill) in zip(after, before):
        assert a_stats == b_stats and a_prefill == b_prefill and not set(HOST_KEYS) & set(a_stats)
        for x, y in zip(a, b):
            assert torch.equal(x["generate_ids"], y["generate_ids"]) and torch.equal(x["last_hidden_states"], y["last_hidden_states"])
