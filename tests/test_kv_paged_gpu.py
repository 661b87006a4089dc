"""The paged KV cache on the GPU: a paged launch / model / engine is, bit for bit, the contiguous one — only the address of a key row
changes. Kernel level (sx_rope_kv_append_f32_paged, sx_attention_f32 with a page table: the T = 1 split kernel with and without fused
RoPE, the QB = 4 / 8 VALU kernel, the fp32 MFMA kernel) against the same call on contiguous caches through a scrambled page table; model
level (LlamaForCausalLM(kv_pages=N) against its contiguous twin: prefill, token steps, graph replay across a re-reservation, the adapter
step) and ContinuousLVLM.generate_inflight with page-gated admission. Everything is torch.equal or a count."""
import math

import pytest
import torch

from oracle import weights
from tests.test_models_gpu import StubTokenizer

pytestmark = pytest.mark.gpu

DTS = [torch.float16, torch.bfloat16]
D, H, TMAX = 128, 2, 1536
VIT = 128
KW = dict(num_img_gen_tokens=16, eos_token_id=None)
_IN = {}
_SD = {}


def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


# ---- kernel level ----------------------------------------------------------------------------------------------------------------------
def _inputs(dev, G):
    """qkv rows for up to 165 tokens per sequence, contiguous fp32 caches and the RoPE tables, made once per G (tests clone what a kernel
    writes)."""
    if G not in _IN:
        g = torch.Generator().manual_seed(53)
        qkv = (torch.randn(G * 165, 3 * H * D, generator=g) * 1.5).to(dev)
        kc = (torch.randn(G, H, TMAX, D, generator=g) * 1.5).to(dev)
        vc = torch.randn(G, H, TMAX, D, generator=g).to(dev)
        inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
        ang = torch.arange(TMAX).float()[:, None] * inv[None]
        _IN[G] = (qkv, kc, vc, ang.cos().to(dev).contiguous(), ang.sin().to(dev).contiguous())
    return _IN[G]


def _table(G, ps, dev, spare=5):
    """A scrambled, non-monotonic page table that maps every row of every sequence: a seeded permutation of pages 1 .. N over the
    [G, TMAX / ps] entries, ``spare`` pages left to nobody. Returns (table on the device, N)."""
    W = TMAX // ps
    N = G * W + spare
    perm = (torch.randperm(N, generator=torch.Generator().manual_seed(ps + G)) + 1)[:G * W].view(G, W)
    assert (perm[:, 1:] < perm[:, :-1]).any() and (perm[:, 1:] > perm[:, :-1]).any() and perm.min() >= 1
    return perm.to(torch.int32).to(dev).contiguous(), N


SENTINEL = 7.0      # what pages nobody owns hold (finite: the MFMA kernel may read the rows of a tile's own page past the last key)


def _paginate(c, table, N, ps, into=None):
    """The pool [N + 1, H, ps, D] that holds the contiguous cache c [G, H, TMAX, D] behind ``table``: mapped pages take c's rows, page 0 is
    zero, every other page keeps ``into`` (default: the sentinel)."""
    G = c.shape[0]
    pool = torch.full((N + 1, H, ps, D), SENTINEL, dtype=c.dtype, device=c.device) if into is None else into.clone()
    if into is None:
        pool[0].zero_()
    pages = c.view(G, H, TMAX // ps, ps, D).permute(0, 2, 1, 3, 4)          # [G, W, H, ps, D]
    t = table.long()
    m = t > 0
    pool[t[m]] = pages[m]
    return pool


def _gather(pool, table):
    """The contiguous view [G, H, TMAX, D] of a pool through the table."""
    G, W = table.shape
    return pool[table.long()].permute(0, 2, 1, 3, 4).reshape(G, H, W * pool.shape[2], D)


def _twins(dev, G, ps, dt, v16):
    qkv, kc, v32, cos, sin = _inputs(dev, G)
    vc = v32.to(dt) if v16 else v32
    table, N = _table(G, ps, dev)
    return qkv, kc, vc, cos, sin, table, N, _paginate(kc, table, N, ps), _paginate(vc, table, N, ps)


def _same_pools(kp, vp, kc, vc, table, N, ps, what, into=None):
    """The pools hold exactly the contiguous caches behind the table, and every other page — page 0 included — is untouched."""
    if (table > 0).all():
        assert torch.equal(_gather(kp, table), kc) and torch.equal(_gather(vp, table), vc), what + ": rows gathered through the table"
    assert torch.equal(kp, _paginate(kc, table, N, ps, None if into is None else into[0])), what + ": k pool"
    assert torch.equal(vp, _paginate(vc, table, N, ps, None if into is None else into[1])), what + ": v pool"
    assert not kp[0].any() and not vp[0].any(), what + ": the null page"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("v16", [False, True])
@pytest.mark.parametrize("ps", [32, 128])
def test_append_through_the_table_equals_the_contiguous_append(dev, dt, v16, ps):
    """sx_rope_kv_append_f32_paged against sx_rope_kv_append_f32 / _v16 for T = 1, 5 and 40 rows per sequence at positions that straddle
    page edges, a parked slot and rows past the cache: the rotated q rows, the pool gathered through the table and every page nobody
    owns (page 0 included) are torch.equal. Then one table entry is set to 0: the rows that fall there are not written."""
    from seedx_amd import ops
    G = 4
    qkv0, kc0, vc0, cos, sin, table, N, kp0, vp0 = _twins(dev, G, ps, dt, v16)
    for T, pos in ((1, [0, ps - 1, ps, 1535]), (5, [ps - 2, 1499, -1, 1534]), (40, [37, 2 * ps - 40, 1536, 1500])):
        posd = _i32(pos, dev)
        qa, ka, va = qkv0[:G * T].clone(), kc0.clone(), vc0.clone()
        ops.rope_kv_append_f32(qa, ka, va, cos, sin, posd, G, T, H, D, dt)
        qb, kp, vp = qkv0[:G * T].clone(), kp0.clone(), vp0.clone()
        ops.rope_kv_append_f32(qb, kp, vp, cos, sin, posd, G, T, H, D, dt, paged=(table, TMAX))
        assert torch.equal(qa, qb), (T, "rotated q")
        assert not torch.equal(ka, kc0)
        _same_pools(kp, vp, ka, va, table, N, ps, f"T={T}")
    # sequence 0 loses the page of rows [ps, 2 ps): of its 40 rows at position ps - 8 only the first 8 are written
    T, pos = 40, [ps - 8, 0, 5, 9]
    cut = table.clone()
    lost = int(cut[0, 1])
    cut[0, 1] = 0
    qa, ka, va = qkv0[:G * T].clone(), kc0.clone(), vc0.clone()
    ops.rope_kv_append_f32(qa, ka, va, cos, sin, _i32(pos, dev), G, T, H, D, dt)
    qb, kp, vp = qkv0[:G * T].clone(), kp0.clone(), vp0.clone()
    ops.rope_kv_append_f32(qb, kp, vp, cos, sin, _i32(pos, dev), G, T, H, D, dt, paged=(cut, TMAX))
    assert torch.equal(qa, qb)
    _same_pools(kp, vp, ka, va, cut, N, ps, "an entry of 0", into=(kp0, vp0))
    assert torch.equal(kp[lost], kp0[lost]) and torch.equal(vp[lost], vp0[lost]) and not torch.equal(_gather(kp, table)[0], ka[0])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("v16", [False, True])
@pytest.mark.parametrize("ps", [32, 128])
@pytest.mark.parametrize("fused", [True, False])
def test_single_row_decode_equals_the_contiguous_call(dev, dt, v16, ps, fused):
    """The T = 1 step with nsplit 1, 2 and 6, RoPE + append fused into the launch or in a launch of their own, at positions 0,
    page_size - 1, page_size, 1499 and 1535, with a parked slot (-1) and a position >= max_cache_len: the context planes (row-major and
    tiled), the k pool and the v pool are torch.equal to the contiguous call's planes and caches; untouched pages stay untouched."""
    from seedx_amd import ops
    G = 4
    qkv0, kc0, vc0, cos, sin, table, N, kp0, vp0 = _twins(dev, G, ps, dt, v16)
    scale = 1.0 / math.sqrt(D)

    def step(kc, vc, posd, nsplit, tiled, **pg):
        q = qkv0[:G].clone()
        if fused:
            return ops.attention_f32(q, kc, vc, posd, G, 1, H, D, scale, dt, tiled=tiled, nsplit=nsplit, rope=(cos, sin), **pg)
        ops.rope_kv_append_f32(q, kc, vc, cos, sin, posd, G, 1, H, D, dt, **pg)
        return ops.attention_f32(q, kc, vc, posd, G, 1, H, D, scale, dt, tiled=tiled, nsplit=nsplit, **pg)

    for nsplit in (1, 2, 6):
        for pos in ([0, ps - 1, ps, 1499], [1535, -1, TMAX, TMAX + 40]):
            posd = _i32(pos, dev)
            ka, va, kp, vp = kc0.clone(), vc0.clone(), kp0.clone(), vp0.clone()
            ya = step(ka, va, posd, nsplit, False)
            yb = step(kp, vp, posd, nsplit, False, paged=(table, TMAX))
            assert torch.isfinite(ya.float()).all()
            assert torch.equal(ya, yb), (nsplit, pos, (ya != yb).any(dim=1).nonzero().flatten().tolist())
            _same_pools(kp, vp, ka, va, table, N, ps, f"nsplit={nsplit} pos={pos}")
            yt = step(kc0.clone(), vc0.clone(), posd, nsplit, True)
            ytp = step(kp0.clone(), vp0.clone(), posd, nsplit, True, paged=(table, TMAX))
            assert torch.equal(yt.dense(), ytp.dense()) and torch.equal(yt.dense(), ya[:, :H * D].float() + ya[:, H * D:].float()), \
                (nsplit, pos, "tiled planes")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("v16", [False, True])
@pytest.mark.parametrize("ps", [32, 128])
def test_chunks_equal_the_contiguous_call(dev, dt, v16, ps):
    """Chunks of T = 4 and 8 rows (the QB = 4 / 8 VALU kernel) and of 40 and 165 rows (the MFMA kernel; with sx_attention_f32_variant(0)
    the QB = 8 VALU kernel) at pos0 = 0 and at an unaligned pos0 = 37, two sequences at different positions: append + attention through
    the table equal the contiguous calls in the planes and both caches."""
    from seedx_amd import _lib, ops
    G = 2
    qkv0, kc0, vc0, cos, sin, table, N, kp0, vp0 = _twins(dev, G, ps, dt, v16)
    scale = 1.0 / math.sqrt(D)
    lib = _lib.load()
    try:
        for variant in (1, 0):
            _lib.check(lib.sx_attention_f32_variant(variant), "sx_attention_f32_variant")
            for T in (4, 8, 40, 165):
                for p0 in (0, 37):
                    posd = _i32([p0, p0 + 3 * ps + 5], dev)
                    qa, ka, va = qkv0[:G * T].clone(), kc0.clone(), vc0.clone()
                    ops.rope_kv_append_f32(qa, ka, va, cos, sin, posd, G, T, H, D, dt)
                    ya = ops.attention_f32(qa, ka, va, posd, G, T, H, D, scale, dt)
                    qb, kp, vp = qkv0[:G * T].clone(), kp0.clone(), vp0.clone()
                    ops.rope_kv_append_f32(qb, kp, vp, cos, sin, posd, G, T, H, D, dt, paged=(table, TMAX))
                    yb = ops.attention_f32(qb, kp, vp, posd, G, T, H, D, scale, dt, paged=(table, TMAX))
                    assert torch.isfinite(ya.float()).all()
                    assert torch.equal(ya, yb), (variant, T, p0, (ya != yb).any(dim=1).nonzero().flatten().tolist()[:8])
                    _same_pools(kp, vp, ka, va, table, N, ps, f"variant={variant} T={T} pos0={p0}")
    finally:
        _lib.check(lib.sx_attention_f32_variant(1), "sx_attention_f32_variant")


def test_forms_without_a_paged_kernel_refuse_the_table(dev):
    from seedx_amd import ops
    G, ps = 2, 32
    qkv0, kc0, vc0, cos, sin, table, N, kp0, vp0 = _twins(dev, G, ps, torch.float16, False)
    posd = _i32([3, 40], dev)
    with pytest.raises(RuntimeError, match="a page table and the verify form"):
        ops.attention_f32(qkv0[:G * 4].clone(), kp0.clone(), vp0.clone(), posd, G, 4, H, D, 0.1, torch.float16, nsplit=2, rope=(cos, sin),
                          paged=(table, TMAX))
    with pytest.raises(RuntimeError, match="a page table and kv_fp8 exclude each other"):
        ops.attention_f32(qkv0[:G].clone(), kp0.clone(), vp0.clone(), posd, G, 1, H, D, 0.1, torch.float16, rope=(cos, sin), kv_emulate=True,
                          paged=(table, TMAX))
    d64 = torch.zeros((N + 1, H, ps, 64), device=dev)
    with pytest.raises(RuntimeError, match="a page table needs head_dim 128, not 64"):
        ops.attention_f32(torch.zeros((G, 3 * H * 64), device=dev), d64, d64.clone(), posd, G, 1, H, 64, 0.1, torch.float16, paged=(table, TMAX))
    with pytest.raises(RuntimeError, match="head_dim 64"):
        ops.rope_kv_append_f32(torch.zeros((G, 3 * H * 64), device=dev), d64, d64.clone(), cos, sin, posd, G, 1, H, 64, torch.float16,
                               paged=(table, TMAX))


# ---- model level -----------------------------------------------------------------------------------------------------------------------
def _llm(dev, dt, G, **kw):
    from seedx_amd.llama import LlamaForCausalLM
    cfg = weights.MINI_LLM
    if "llm" not in _SD:
        _SD["llm"] = weights.llama_sd(cfg)
    m = LlamaForCausalLM(dict(cfg), max_cache_len=128, max_batch=G, precise=True, **kw)
    m.load_state_dict(dict(_SD["llm"]))
    m.eval().to(dev, dtype=dt)
    return m


LENS = [31, 33, 64]          # ragged prompts around the edges of 32-row pages; 12 token steps cross rows 32 (sequence 0) and 64 (2)
STEPS = 12


def _prompts(dev):
    g = torch.Generator().manual_seed(5)
    return [(torch.randn(t, weights.MINI_LLM["hidden_size"], generator=g) * 0.5).to(dev) for t in LENS]


def _run(m, dev, xs, bufs, use_graph, seqs=None, steps=STEPS):
    """Prefill ``seqs`` (default: all, after a reset, with LENS + 40 rows reserved on a paged model), then token steps of every
    sequence. Returns (prefill logits, ids, hidden states)."""
    P, G = m._pack(), m.G
    img, out_ids, hid = bufs
    if seqs is None:
        m.reset()
        seqs = list(range(G))
        P["step"].zero_()
        out_ids.fill_(-1)
        hid.zero_()
        if m.kv_pages:
            for g in seqs:
                assert m.kv_reserve(g, LENS[g] + 40)
    logits, _ = m.forward_embeds_batch([xs[g] for g in seqs], seqs)
    m._slot_write(P["cur"], seqs, [20 + g for g in seqs])
    for _ in range(steps):
        m.decode_step(img, out_ids, hid, use_graph=use_graph)
    torch.cuda.synchronize()
    return logits.clone(), out_ids.clone(), hid.clone()


@pytest.mark.parametrize("dt", DTS)
def test_paged_model_equals_its_contiguous_twin(dev, dt):
    """G = 3, pages of 32 rows: prefill logits, 12 token steps' ids and hidden states are torch.equal between the paged model and its
    contiguous twin, eager and under graph replay, and so are the cache rows gathered through the table. Then sequence 1 is released,
    reserved again onto DIFFERENT pages and prefilled again while the others go on: the SAME captured graph, replayed, still equals the
    twin — it reads the table from device memory at replay."""
    G = 3
    xs = _prompts(dev)
    flat, paged = _llm(dev, dt, G), _llm(dev, dt, G, kv_pages=16, kv_page_size=32)
    assert paged.kv_pages_free == 16
    assert paged.memory_footprint()["kv_cache"] == sum(paged._P[k].numel() * paged._P[k].element_size() for k in ("kc", "vc")), "the pool"
    assert paged._P["kc"].shape == (paged.L, 17, 2, 32, 128) and paged._P["ptab"].shape == (G, 4) and paged._P["ptab"].dtype == torch.int32
    mk = lambda: (torch.arange(400, 466, dtype=torch.int32, device=dev), torch.full((G, 40), -1, dtype=torch.int32, device=dev),
                  torch.zeros((G, 40, flat.H), device=dev))
    bf, bp = mk(), mk()
    ref = _run(flat, dev, xs, bf, use_graph=False)
    assert (ref[1][:, :STEPS] >= 0).all()
    for use_graph in (False, True):
        got = _run(paged, dev, xs, bp, use_graph)
        for a, b, what in zip(ref, got, ("prefill logits", "ids", "hidden states")):
            assert torch.equal(a, b), (use_graph, what)
        assert paged.kv_pages_free == 16 - sum(-(-(n + 40) // 32) for n in LENS)
    for a, b in zip(ref, _run(flat, dev, xs, bf, use_graph=True)):
        assert torch.equal(a, b)
    Pf, Pp = flat._P, paged._P
    for g, n in enumerate(LENS):
        for li in range(flat.L):
            k, v = paged._kv_gather(li, g, n + STEPS)
            assert torch.equal(k, Pf["kc"][li][g][:, :n + STEPS]) and torch.equal(v, Pf["vc"][li][g][:, :n + STEPS]), (g, li)
    assert not Pp["kc"][:, 0].any() and not Pp["vc"][:, 0].any(), "the null page"
    # sequence 1 moves to other pages; the captured step is not captured again
    graph, before = paged._graph, paged._pool.pages(1)
    paged.kv_release(1)
    assert paged.kv_reserve(0, LENS[0] + 40 + 32), "sequence 0 grows by a page: it takes the first page sequence 1 gave back"
    assert paged.kv_reserve(1, LENS[1] + 40)
    after = paged._pool.pages(1)
    assert after != before and len(after) == len(before) and set(after) != set(before)
    for m in (flat, paged):
        m.set_position(1, 0)
        m._pack()["step"][1] = 0
    ref2 = _run(flat, dev, xs, bf, use_graph=True, seqs=[1], steps=6)
    got2 = _run(paged, dev, xs, bp, use_graph=True, seqs=[1], steps=6)
    assert paged._graph is graph and paged._graph is not None
    for a, b, what in zip(ref2, got2, ("prefill logits", "ids", "hidden states")):
        assert torch.equal(a, b), what
    assert not torch.equal(ref2[1], ref[1])
    paged.reset()
    assert paged.kv_pages_free == 16 and not Pp["ptab"].any()
    with pytest.raises(RuntimeError, match="more pages of 32 rows"):
        big = _llm(dev, dt, G, kv_pages=2, kv_page_size=32)
        big.forward_embeds_batch([xs[2]], [0])           # 64 rows fit, the 65th does not
        big.forward_embeds_batch([xs[0][:1]], [0])


def _adapter(g, r=8, gain=0.05):
    """A PEFT-style LoRA state dict of rank r on the seven projections of every MINI_LLM layer (16-bit values)."""
    cfg = weights.MINI_LLM
    Hh, I = cfg["hidden_size"], cfg["intermediate_size"]
    dims = {"self_attn.q_proj": (Hh, Hh), "self_attn.k_proj": (Hh, Hh), "self_attn.v_proj": (Hh, Hh), "self_attn.o_proj": (Hh, Hh),
            "mlp.gate_proj": (I, Hh), "mlp.up_proj": (I, Hh), "mlp.down_proj": (Hh, I)}
    sd = {}
    for i in range(cfg["num_hidden_layers"]):
        p = f"base_model.model.model.layers.{i}."
        for n, (N, K) in dims.items():
            sd[p + n + ".lora_A.default.weight"] = (torch.randn(r, K, generator=g) / math.sqrt(K)).half().float()
            sd[p + n + ".lora_B.default.weight"] = (gain * torch.randn(N, r, generator=g) / math.sqrt(r)).half().float()
    return sd


def test_adapter_step_paged_equals_unpaged(dev):
    """max_adapters = 1: a prefill and token steps with sequence 1 under an adapter, the others on the base model — the paged model
    equals its contiguous twin, and the adapter moved sequence 1."""
    G = 3
    xs = _prompts(dev)
    ad = _adapter(torch.Generator().manual_seed(8))
    outs = []
    for kw in (dict(), dict(kv_pages=12, kv_page_size=64)):
        m = _llm(dev, torch.float16, G, max_adapters=1, lora_rank=8, **kw)
        m.load_adapter("a", ad, lora_alpha=32)
        P = m._pack()
        m.reset()
        names = [None, "a", None]
        logits, _ = m.forward_embeds_batch(xs, list(range(G)), adapters=names)
        m.set_adapters(range(G), names)
        P["cur"].copy_(_i32([20, 21, 22], dev))
        P["step"].zero_()
        if m.kv_pages:
            for g in range(G):
                assert m.kv_reserve(g, LENS[g] + 8)
        out_ids = torch.full((G, 8), -1, dtype=torch.int32, device=dev)
        hid = torch.zeros((G, 8, m.H), device=dev)
        for _ in range(4):
            m.decode_step(torch.arange(400, 466, dtype=torch.int32, device=dev), out_ids, hid, use_graph=False)
        torch.cuda.synchronize()
        outs.append((logits.clone(), out_ids.clone(), hid.clone()))
        m.set_adapters(range(G), [None] * G)
    for a, b, what in zip(outs[0], outs[1], ("prefill logits", "ids", "hidden states")):
        assert torch.equal(a, b), what
    base = _run(_llm(dev, torch.float16, G), dev, xs, (torch.arange(400, 466, dtype=torch.int32, device=dev),
                torch.full((G, 8), -1, dtype=torch.int32, device=dev), torch.zeros((G, 8, outs[0][2].shape[2]), device=dev)), False, steps=0)
    assert not torch.equal(base[0][1], outs[0][0][1]), "the adapter moved its sequence"


# ---- the engine ------------------------------------------------------------------------------------------------------------------------
def _agent(dev, G, **kw):
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
    Hh = cfg["hidden_size"]
    agent = ContinuousLVLM(llm, Resampler(4, Hh, 2, kv_dim=VIT), Resampler(4, VIT, 2, kv_dim=Hh), add_patch_pos=True)
    agent.load_state_dict(_SD["agent"])
    agent.eval().to(dev, dtype=torch.float16)
    return agent


PLENS = [40, 45, 60, 33, 50, 70]
BUDGETS = [14, 30, 5, 9, 12, 20]     # rows reserved: 54, 75, 65, 42, 62, 90 = 2, 3, 3, 2, 2, 3 pages of 32 rows


def _requests():
    reqs = [dict(input_ids=[[1] + [10 + (7 * r + 3 * i) % 380 for i in range(n - 1)]], max_new_tokens=b)
            for r, (n, b) in enumerate(zip(PLENS, BUDGETS))]
    reqs[1]["force_image_at"] = 2
    reqs[4].update(do_sample=True, temperature=0.9, top_k=30, top_p=0.95, seed=4321)
    return reqs


def test_generate_inflight_admits_by_pages(dev):
    """Six requests on three slots, mixed budgets, one forced image block, one sampled request. (a) an ample pool: ids, hidden states
    and step counts are the unpaged agent's. (b) a pool of 5 pages holds two of the requests at a time (never three: 2 + 2 + 2 > 5):
    every request's ids are those of (a), the step counts are inflight.simulate_paged's, and every page is free afterwards. (c) a
    request larger than the pool raises ValueError and leaves the pool untouched; prefix_cache raises ValueError."""
    from seedx_amd.inflight import simulate_paged
    tok, reqs = StubTokenizer(), _requests()
    flat = _agent(dev, 3)
    want = flat.generate_inflight(tok, reqs, **KW)
    want_stats = dict(flat.last_inflight_stats)
    assert want[1]["num_gen_imgs"] == 1 and [len(x["generate_ids"]) for x in want] == BUDGETS
    ample = _agent(dev, 3, kv_pages=48, kv_page_size=32)
    got = ample.generate_inflight(tok, reqs, **KW)
    stats = dict(ample.last_inflight_stats)
    for r, (a, b) in enumerate(zip(want, got)):
        assert torch.equal(a["generate_ids"], b["generate_ids"]), (r, a["generate_ids"].tolist(), b["generate_ids"].tolist())
        assert torch.equal(a["last_hidden_states"], b["last_hidden_states"]), r
        assert a["text"] == b["text"] and a["num_gen_imgs"] == b["num_gen_imgs"]
    assert stats.pop("page_waits") == 0 and 6 <= stats.pop("peak_pages") <= 9 and stats == want_stats
    assert ample.llm.kv_pages_free == 48
    # (b) five pages
    tight = _agent(dev, 3, kv_pages=5, kv_page_size=32)
    got = tight.generate_inflight(tok, reqs, **KW)
    stats = tight.last_inflight_stats
    for r, (a, b) in enumerate(zip(want, got)):
        assert torch.equal(a["generate_ids"], b["generate_ids"]), (r, a["generate_ids"].tolist(), b["generate_ids"].tolist())
        assert a["text"] == b["text"] and a["num_gen_imgs"] == b["num_gen_imgs"]
    lengths = [len(x["generate_ids"]) - (17 if x["num_gen_imgs"] else 0) for x in got]          # an image block takes no decode step
    sim = simulate_paged(PLENS, lengths, 3, 5, 32, budgets=BUDGETS)
    for k in ("decode_steps", "live_slot_steps", "parked_slot_steps", "admissions", "prefill_passes", "page_waits", "peak_pages"):
        assert stats[k] == sim[k], (k, stats, sim)
    assert stats["page_waits"] > 0 and stats["peak_pages"] == 5 and stats["decode_steps"] > want_stats["decode_steps"]
    assert tight.llm.kv_pages_free == tight.llm.kv_pages == 5 and not tight.llm._P["ptab"].any()
    print(f"paged generate_inflight: {stats['decode_steps']} steps on 5 pages ({want_stats['decode_steps']} unpaged), "
          f"{stats['page_waits']} page waits")
    # (c) never fits: refused before anything is touched
    assert tight.llm.kv_reserve(0, 40)
    held, tab = tight.llm._pool.pages(0), tight.llm._P["ptab"].clone()
    with pytest.raises(ValueError, match="request 2 needs 181 cache rows"):
        tight.generate_inflight(tok, reqs[:2] + [dict(input_ids=[[1] + list(range(10, 170))], max_new_tokens=20)], **KW)
    assert tight.llm._pool.pages(0) == held and torch.equal(tight.llm._P["ptab"], tab) and tight.llm.kv_pages_free == 3
    tight.prefix_cache = True
    with pytest.raises(ValueError, match="follow-up: prefix reuse by sharing pages by reference"):
        tight.generate_inflight(tok, reqs, **KW)
    assert tight.llm._pool.pages(0) == held


def test_generate_batch_reserves_up_front(dev):
    """generate_batch on a paged LLM: every sequence holds prompt + max_new_tokens rows from the start, the results are the unpaged
    agent's, a ``reuse_cache`` turn extends the reservation in place, and a pool that is too small is a RuntimeError naming the shortfall."""
    tok = StubTokenizer()
    reqs = [dict(input_ids=[[1] + [10 + (5 * r + i) % 300 for i in range(n - 1)]]) for r, n in enumerate((30, 47))]
    kw = dict(KW, max_new_tokens=20)
    want = _agent(dev, 2).generate_batch(tok, reqs, **kw)
    agent = _agent(dev, 2, kv_pages=8, kv_page_size=32)
    got = agent.generate_batch(tok, reqs, reuse_cache=True, **kw)
    for a, b in zip(want, got):
        assert torch.equal(a["generate_ids"], b["generate_ids"]) and torch.equal(a["last_hidden_states"], b["last_hidden_states"])
    pool = agent.llm._pool
    assert (pool.pages(0), pool.pages(1)) == ([1, 2], [3, 4, 5]) and agent.llm.kv_pages_free == 3      # 50 and 67 rows
    turn2 = [dict(input_ids=[r["input_ids"][0] + g["generate_ids"][:-1].tolist() + [7, 8, 9]]) for r, g in zip(reqs, got)]
    again = agent.generate_batch(tok, turn2, reuse_cache=True, **kw)
    assert agent.last_prefill_tokens == [3, 3], "the turn prefills only what the cache does not hold"
    assert (pool.pages(0), pool.pages(1)) == ([1, 2, 6], [3, 4, 5]), "52 + 20 rows need a third page; 69 + 20 still fit three"
    fresh = _agent(dev, 2).generate_batch(tok, turn2, **kw)
    for a, b in zip(fresh, again):
        assert torch.equal(a["generate_ids"], b["generate_ids"])
    small = _agent(dev, 2, kv_pages=4, kv_page_size=32)
    with pytest.raises(RuntimeError, match="sequence 1 needs 67 cache rows = 3 more pages of 32 rows, but 2 of the pool's 4 pages are free"):
        small.generate_batch(tok, reqs, **kw)
