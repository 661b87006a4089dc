"""sx_dequant_tiles and LlamaForCausalLM(weight_residency="tiles") on the GPU.

The claim is EXACTNESS twice over: the kernel rebuilds, bit for bit, the row-major 16-bit matrix quant.dequantize_rows /
dequantize_blocks_mxfp4 give (every code * 2^e is representable in fp16 and bf16), and a model that holds the quantised tiles alone —
prefill dequantising one projection at a time into a shared scratch buffer in front of the unchanged GEMM — computes the bits of the same
weight_format at default residency: prefill logits, decode ids, hidden states, serving ids, tensor-parallel logits. What the mode is for
is checked too: the row-major projections are gone from the allocator's books and memory_footprint() prices what is held.
Reference: modeling_llama_xformer.py:204-206, 239, 166-167 (the nn.Linear calls whose weights these are)."""
import ctypes as C

import pytest
import torch

from oracle import weights

pytestmark = pytest.mark.gpu
DTS = [torch.float16, torch.bfloat16]
FMTS = ["mxfp4", "fp8_e4m3"]
# (N, K): one and several 64-k slabs, 16- and 20-row tails (a wave's last, partial group of slabs), more than one row group, more than one
# workgroup along K (1088 = 17 slabs); a shape whose N is no multiple of the layout's rows has no such tiles (the entry point refuses it)
SHAPES = [(64, 256), (160, 320), (1536, 512), (640, 1088)]
SENTINEL_BYTES = 4096
_REF = {}


def _case(dev, fmt, N, K, rows, seed):
    """Random weights through the codec, once per (format, shape, rows): (row-major codes, scales, the tile pair ops.dequant_tiles takes)."""
    from seedx_amd import ops, quant
    key = (fmt, N, K, rows)
    if key not in _REF:
        g = torch.Generator().manual_seed(seed)
        w = (torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-12, 4, (N, 1), generator=g).float())).to(dev, torch.float16)
        if fmt == "mxfp4":
            codes, scale = quant.quantize_blocks_mxfp4(w)
            pair = ((ops.pack_decode_tiles_fp4 if rows == 16 else ops.pack_decode_tiles20_fp4)(codes), ops.pack_block_scales_fp4(scale, rows=rows))
        else:
            codes, scale = quant.quantize_rows(w)
            pair = ((ops.pack_decode_tiles_fp8 if rows == 16 else ops.pack_decode_tiles20_fp8)(codes), scale.clone())
        _REF[key] = (codes, scale, pair)
    return _REF[key]


@pytest.fixture(scope="module", autouse=True)
def _free():
    yield
    _REF.clear()
    torch.cuda.empty_cache()


def _reference(fmt, codes, scale, dt):
    from seedx_amd import quant
    return (quant.dequantize_blocks_mxfp4 if fmt == "mxfp4" else quant.dequantize_rows)(codes, scale, dt)


def _dequant_with_sentinel(fmt, pair, dt, N, K):
    """ops.dequant_tiles into a caller-owned buffer with SENTINEL_BYTES behind the matrix; returns (matrix view, buffer)."""
    from seedx_amd import ops
    buf = torch.full((N * K + SENTINEL_BYTES // 2,), 0x5a5a, dtype=torch.int16, device=pair[0].device).view(dt)
    w = ops.dequant_tiles(dtype=dt, out=buf, **{"w_fp4" if fmt == "mxfp4" else "w_fp8": pair})
    torch.cuda.synchronize()
    assert w.shape == (N, K) and w.dtype == dt and w.data_ptr() == buf.data_ptr() and w.is_contiguous()
    assert bool((buf.view(torch.int16)[N * K:] == 0x5a5a).all()), "bytes behind the matrix were written"
    return w, buf


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("rows", [16, 20])
def test_dequant_tiles_is_exact(dev, dt, fmt, rows):
    from seedx_amd import ops
    done = 0
    for i, (N, K) in enumerate(SHAPES):
        if N % rows:
            continue
        codes, scale, pair = _case(dev, fmt, N, K, rows, 70 + i)
        want = _reference(fmt, codes, scale, dt)
        got, _ = _dequant_with_sentinel(fmt, pair, dt, N, K)
        bad = (got.view(torch.int16) != want.view(torch.int16)).nonzero()
        assert torch.equal(got, want) and bad.numel() == 0, (N, K, rows, bad[:8].tolist())
        # without ``out`` the function allocates the matrix itself: the same bits
        own = ops.dequant_tiles(dtype=dt, **{"w_fp4" if fmt == "mxfp4" else "w_fp8": pair})
        assert own.shape == (N, K) and torch.equal(own, want)
        done += 1
    assert done == (4 if rows == 16 else 2)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("rows", [16, 20])
def test_every_e2m1_code_under_the_extreme_block_exponents(dev, dt, rows):
    """W[n][k] holds code (n + k) % 16 — every k position of a row sees all 16 codes over the rows — under block exponents -13, 0 and 13
    (cycling over rows and blocks): the result must BE decode(code) * 2^e."""
    from seedx_amd import ops, quant
    N, K = 160, 320
    n_i, k_i = torch.arange(N)[:, None], torch.arange(K)[None, :]
    nib = ((n_i + k_i) % 16).to(torch.uint8)
    e = torch.tensor([-13, 0, 13])[(n_i + torch.arange(K // 32)[None, :]) % 3]
    assert all(set(nib[:, k].tolist()) == set(range(16)) for k in range(64)) and set(e.flatten().tolist()) == {-13, 0, 13}
    codes = (nib[:, 0::2] | (nib[:, 1::2] << 4)).to(dev)
    scale = (e + 127).to(torch.uint8).to(dev)
    want32 = quant.decode_table_e2m1()[nib.long()].double() * torch.pow(2.0, e.double()).repeat_interleave(32, dim=1)
    want = _reference("mxfp4", codes, scale, dt)
    assert torch.equal(want.double().cpu(), want32)                                 # the reference holds the exact values
    pair = ((ops.pack_decode_tiles_fp4 if rows == 16 else ops.pack_decode_tiles20_fp4)(codes), ops.pack_block_scales_fp4(scale, rows=rows))
    got, _ = _dequant_with_sentinel("mxfp4", pair, dt, N, K)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (got.view(torch.int16) != want.view(torch.int16)).nonzero()[:8].tolist()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("rows", [16, 20])
def test_every_finite_e4m3_code_under_the_extreme_row_scales(dev, dt, rows):
    """Every row holds all 254 finite e4m3 codes (the NaN codes 0x7f / 0xff, which the quantiser never produces, are replaced by 0), rows
    alternate between the smallest and the largest scale quantize_rows can produce, 2^-15 and 2^7: fp16 subnormals down to 2^-24 and
    values up to 448 * 128 included. Bit-identical to dequantize_rows, which holds the exact products."""
    from seedx_amd import ops, quant
    N, K = 160, 320
    n_i, k_i = torch.arange(N)[:, None], torch.arange(K)[None, :]
    codes = ((7 * n_i + k_i) % 256).to(torch.uint8)
    codes[(codes & 0x7f) == 0x7f] = 0
    assert all(len(set(codes[n].tolist())) == 254 for n in (0, 1, 159))
    s = torch.where(torch.arange(N) % 2 == 0, torch.tensor(quant.S_MIN), torch.tensor(quant.S_MAX))
    scale = torch.pow(2.0, s.float()).to(dev)
    codes = codes.to(dev)
    want = _reference("fp8_e4m3", codes, scale, dt)
    exact = quant.decode_table()[codes.cpu().long()].double() * scale.cpu().double()[:, None]
    assert torch.equal(want.double().cpu(), exact)                                  # no rounding in the reference: every product is representable
    pair = ((ops.pack_decode_tiles_fp8 if rows == 16 else ops.pack_decode_tiles20_fp8)(codes), scale)
    got, _ = _dequant_with_sentinel("fp8_e4m3", pair, dt, N, K)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (got.view(torch.int16) != want.view(torch.int16)).nonzero()[:8].tolist()


def test_entry_point_refusals(dev):
    """SX_ERR_INVALID with a message and nothing launched: a w_dtype that is neither format, layout 0, K % 64 != 0, N no multiple of the
    layout's rows, a missing / misaligned scale pointer, the other format's scale pointer, out_bytes below N * K * 2."""
    from seedx_amd import _lib, ops
    lib = _lib.load()
    N, K = 160, 320
    t8 = torch.zeros(N * K, dtype=torch.uint8, device=dev)
    rs = torch.ones(N + 4, device=dev)
    bs = torch.full((N * K // 32 + 16,), 127, dtype=torch.uint8, device=dev)
    out = torch.full((N * K,), 0x5a5a, dtype=torch.int16, device=dev)

    def call(fmt, **kw):
        a = _lib.DequantTilesArgs()
        a.tiles, a.out, a.out_bytes, a.N, a.K, a.dtype, a.w_layout = t8.data_ptr(), out.data_ptr(), N * K * 2, N, K, _lib.SX_F16, 1
        if fmt == "fp8":
            a.w_dtype, a.w_scale = _lib.SX_FP8_E4M3, rs.data_ptr()
        else:
            a.w_dtype, a.w_block_scale = _lib.SX_FP4_E2M1, bs.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        st = lib.sx_dequant_tiles(C.byref(a), ops._stream())
        return st, lib.sx_last_error().decode()
    bad = [("fp8", dict(w_dtype=0)), ("fp8", dict(w_dtype=7)), ("fp4", dict(w_dtype=_lib.SX_F16)),
           ("fp8", dict(w_layout=0)), ("fp4", dict(w_layout=0)), ("fp8", dict(w_layout=3)),
           ("fp8", dict(K=288)), ("fp4", dict(K=288)),
           ("fp8", dict(N=168)), ("fp4", dict(N=150, w_layout=2)), ("fp8", dict(N=64, w_layout=2)),
           ("fp8", dict(w_scale=None)), ("fp4", dict(w_block_scale=None)),
           ("fp8", dict(w_scale=rs.data_ptr() + 4)), ("fp4", dict(w_block_scale=bs.data_ptr() + 2)),
           ("fp8", dict(w_block_scale=bs.data_ptr())), ("fp4", dict(w_scale=rs.data_ptr())),
           ("fp8", dict(w_scale=None, w_block_scale=bs.data_ptr())), ("fp4", dict(w_block_scale=None, w_scale=rs.data_ptr())),
           ("fp8", dict(out_bytes=N * K * 2 - 1)), ("fp4", dict(out_bytes=0)),
           ("fp8", dict(dtype=_lib.SX_F32)), ("fp8", dict(out=None)), ("fp4", dict(tiles=None))]
    for fmt, kw in bad:
        st, msg = call(fmt, **kw)
        assert st == 1 and "sx_dequant_tiles" in msg, (fmt, kw, st, msg)
    torch.cuda.synchronize()
    assert bool((out == 0x5a5a).all()), "a refused call wrote to out"
    for fmt in ("fp8", "fp4"):                                     # the unmodified arguments are accepted: code 0 everywhere → zeros
        out.fill_(0x5a5a)
        st, msg = call(fmt)
        assert st == 0, msg
        torch.cuda.synchronize()
        assert not out.any()
    # the wrapper refuses a buffer that is too small or of the other dtype before the library is asked
    pair = (torch.zeros((N // 16, K // 64, 16, 64), dtype=torch.uint8, device=dev), torch.ones(N, device=dev))
    with pytest.raises(AssertionError, match="out must be"):
        ops.dequant_tiles(w_fp8=pair, dtype=torch.float16, out=torch.empty(N * K - 1, dtype=torch.float16, device=dev))
    with pytest.raises(AssertionError, match="out must be"):
        ops.dequant_tiles(w_fp8=pair, dtype=torch.float16, out=torch.empty(N * K, dtype=torch.bfloat16, device=dev))
    with pytest.raises(AssertionError, match="exactly one"):
        ops.dequant_tiles(dtype=torch.float16)


def test_gemv_takes_a_weight_without_storage(dev):
    """ops.gemv with a WeightShape beside the tiles == the same call with the dequantised matrix as ``w``; without tiles it refuses."""
    from seedx_amd import ops
    dt, N, K = torch.float16, 1536, 512
    for fmt in FMTS:
        codes, scale, pair = _case(dev, fmt, N, K, 16, 72)
        wq = _reference(fmt, codes, scale, dt)
        xt = ops.split16(torch.randn(8, K, generator=torch.Generator().manual_seed(1)).to(dev), dt, tiled=True)
        kw = {"w_fp4" if fmt == "mxfp4" else "w_fp8": pair}
        a = ops.gemv(xt, wq, out_dtype=torch.float32, **kw)
        b = ops.gemv(xt, ops.WeightShape((N, K), dt), out_dtype=torch.float32, **kw)
        assert torch.equal(a, b)
    with pytest.raises(AssertionError, match="without storage"):
        ops.gemv(xt, ops.WeightShape((N, K), dt), out_dtype=torch.float32)


def _gamma_far_from_one(sd, g):
    for k in sd:
        if "layernorm" in k or k == "model.norm.weight":
            sd[k] = (1.0 + 0.5 * torch.randn(sd[k].shape, generator=g)).abs().clamp_min(0.2)
    return sd


def _prefill_and_decode(llm, dev, xs, cur0, img_ids, steps, use_graph):
    G, H = len(xs), xs[0].shape[1]
    P = llm._pack()
    llm.reset()
    logits, _ = llm.forward_embeds_batch([x.to(dev) for x in xs], list(range(G)))
    P["cur"].copy_(cur0.to(dev))
    P["step"].zero_()
    out_ids = torch.full((G, steps), -1, dtype=torch.int32, device=dev)
    hid = torch.zeros((G, steps, H), device=dev)
    for _ in range(steps):
        llm.decode_step(img_ids, out_ids, hid, use_graph=use_graph)
    torch.cuda.synchronize()
    return logits.clone(), out_ids.clone(), hid.clone()


def _held(P, keys=("wqkv", "wo", "wgu", "wd")):
    """Bytes by memory_footprint()'s categories, from the tensors the packed model holds."""
    nb = lambda t: t.numel() * t.element_size()
    w = nb(P["embed"]) + nb(P["lm_head"]) + (nb(P["w_scratch"]) if "w_scratch" in P else 0) \
        + sum(nb(lw[k].w) for lw in P["layers"] for k in keys if lw[k].w is not None)
    tiles = nb(P["lm_head_t"]) + sum(nb(t) for lw in P["layers"] for k in keys for t in (lw[k].tiles, lw[k].scales))
    assert w - nb(P["embed"]) - nb(P["lm_head"]) - (nb(P["w_scratch"]) if "w_scratch" in P else 0) \
        == sum(lw[k].nbytes_rowmajor for lw in P["layers"] for k in keys)
    assert tiles - nb(P["lm_head_t"]) == sum(lw[k].nbytes_tiles for lw in P["layers"] for k in keys)
    return {"weights": w, "decode_tiles": tiles, "kv_cache": nb(P["kc"]) + nb(P["vc"])}


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("fmt", FMTS)
def test_tiles_residency_equals_the_default_residency(dev, dt, fmt):
    """The miniature of tests/test_fp4_weights_gpu.py: H = 1024, 8 heads, FFN 2816, 3 layers, gammas far from 1; 4 ragged prompts of
    10 / 7 / 13 / 4 rows, 6 decode steps, max_cache_len 64. A = weight_residency="tiles", B = the same weight_format at default residency:
    bit-identical prefill logits, decode ids and hidden states; A's graph replay == A eager; A's projection handles own no storage; the
    allocator holds L * per_layer_16bit - scratch (less 1 MB of rounding) fewer bytes after A's _pack than after B's, and the bytes held
    are memory_footprint()'s."""
    from seedx_amd import ops
    from seedx_amd.llama import LlamaForCausalLM
    H, nh, I, L = 1024, 8, 2816, 3
    cfg = dict(hidden_size=H, intermediate_size=I, num_hidden_layers=L, num_attention_heads=nh, vocab_size=500, rms_norm_eps=1e-5,
               max_position_embeddings=128)
    g = torch.Generator().manual_seed(11)
    sd = {k: v.to(dt).float() for k, v in _gamma_far_from_one(weights.llama_sd(cfg), g).items()}
    G, STEPS = 4, 6
    lens = [10, 7, 13, 4]
    xs = [torch.randn(t, H, generator=g) * 0.5 for t in lens]
    cur0 = torch.arange(20, 20 + G, dtype=torch.int32)
    img_ids = torch.arange(400, 466, dtype=torch.int32, device=dev)
    keys = ("wqkv", "wo", "wgu", "wd")
    per_layer = (3 * H * H + H * H + 2 * I * H + H * I) * 2
    scratch = 2 * I * H * 2

    def build(**kw):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated(dev)
        llm = LlamaForCausalLM(dict(cfg), max_cache_len=64, max_batch=G, kv_v16=False, weight_format=fmt, **kw)
        llm.load_state_dict(dict(sd))
        llm.eval().to(dev, dtype=dt)
        P = llm._pack()
        torch.cuda.synchronize()
        return llm, P, torch.cuda.memory_allocated(dev) - base
    A, P, bytes_a = build(weight_residency="tiles")
    assert A.weight_residency == "tiles" and A.precise and P["rms_fold_precise"] and P["decode_tiled"] and P["precise_tiled"]
    for lw in P["layers"]:
        for k in keys:
            h = lw[k].gemv_kwargs()["w"]                             # what the token step hands ops.gemv as ``w``: no storage
            assert lw[k].w is None and lw[k].nbytes_rowmajor == 0
            assert isinstance(h, ops.WeightShape) and not torch.is_tensor(h) and h.data_ptr() == 0 and h.dtype == dt == lw[k].dtype
            assert lw[k].format == fmt and lw[k].tiles.dtype == torch.uint8             # quantised tiles only: no 16-bit ones
            assert {"w_tiles", "w_tiles20", "w_fp8", "w_fp4"} & set(lw[k].gemv_kwargs()) == {"w_fp4" if fmt == "mxfp4" else "w_fp8"}
    assert tuple(P["layers"][0]["wgu"].shape) == (2 * I, H) and tuple(P["layers"][0]["wd"].shape) == (H, I)
    assert P["w_scratch"].numel() * 2 == scratch and P["w_scratch"].dtype == dt
    fa, held_a = A.memory_footprint(), _held(P)
    assert fa["prefill_scratch"] == scratch and all(held_a[k] == fa[k] for k in held_a), (held_a, fa)
    assert fa["total"] == sum(held_a.values())
    assert A.weight_quant_report["weight_residency"] == "tiles" and A.weight_quant_report["decode_tile_bytes"] == fa["decode_tiles"]
    a_log, a_ids, a_hid = _prefill_and_decode(A, dev, xs, cur0, img_ids, STEPS, use_graph=False)
    g_log, g_ids, g_hid = _prefill_and_decode(A, dev, xs, cur0, img_ids, STEPS, use_graph=True)
    assert torch.equal(g_log, a_log) and torch.equal(g_ids, a_ids) and torch.equal(g_hid, a_hid)          # graph replay == eager
    del A, P, lw, h
    B, PB, bytes_b = build()
    assert B.weight_residency is None and "w_scratch" not in PB and all(torch.is_tensor(PB["layers"][0][k].w) and PB["layers"][0][k].gemv_kwargs()["w"] is PB["layers"][0][k].w for k in keys)
    fb, held_b = B.memory_footprint(), _held(PB)
    assert "prefill_scratch" not in fb and all(held_b[k] == fb[k] for k in held_b), (held_b, fb)
    assert B.weight_quant_report["weight_residency"] is None
    assert fb["total"] - fa["total"] == L * per_layer - scratch
    b_log, b_ids, b_hid = _prefill_and_decode(B, dev, xs, cur0, img_ids, STEPS, use_graph=False)
    del B, PB
    torch.cuda.empty_cache()
    print(f"weight_residency {fmt} {dt}: allocator bytes after _pack tiles {bytes_a} (memory_footprint total {fa['total']}), default "
          f"{bytes_b} (total {fb['total']}); saved {bytes_b - bytes_a}, expected {L * per_layer - scratch}")
    assert bytes_b - bytes_a >= L * per_layer - scratch - (1 << 20), (bytes_a, bytes_b)
    assert torch.equal(a_log, b_log)
    assert torch.equal(a_ids, b_ids) and bool((a_ids >= 0).all())
    assert torch.equal(a_hid, b_hid)


def test_serving_paths_agree_with_the_default_residency(dev):
    """generate_inflight (five requests, one sampled with a seed; a second pass with prefix_cache on) and generate_batch (four) on
    weights.MINI_LLM with weight_format="mxfp4", kv_format="fp8_e4m3": weight_residency="tiles" returns, request by request, the ids of
    the same calls at default residency."""
    from seedx_amd.llama import LlamaForCausalLM
    from seedx_amd.seed_x import ContinuousLVLM
    from seedx_amd.visual_encoder import Resampler
    from tests.test_models_gpu import StubTokenizer
    cfg, VIT = weights.MINI_LLM, 128
    kw = dict(num_img_gen_tokens=16, eos_token_id=None)
    sd = {k: v.half().float() for k, v in weights.llama_sd(cfg).items()}
    Hd = cfg["hidden_size"]
    tok = StubTokenizer()
    budgets = [9, 5, 12, 7, 6]
    reqs = [dict(input_ids=[[1, 10 + r] + [20 + r + i for i in range(3 + r % 5)]], max_new_tokens=b) for r, b in enumerate(budgets)]
    reqs[1].update(do_sample=True, temperature=1.0, top_k=50, top_p=0.9, seed=21)
    strip = lambda q: {k: v for k, v in q.items() if k != "max_new_tokens"}
    out = {}
    for res in ("tiles", None):
        llm = LlamaForCausalLM(dict(cfg), max_cache_len=512, max_batch=4, weight_format="mxfp4", kv_format="fp8_e4m3", weight_residency=res)
        llm.load_state_dict(dict(sd))
        agent = ContinuousLVLM(llm, Resampler(4, Hd, 2, kv_dim=VIT), Resampler(4, VIT, 2, kv_dim=Hd), add_patch_pos=True)
        agent.load_state_dict(weights.agent_sd(cfg, VIT, in_grid=4, out_grid=4))
        agent.eval().to(dev, dtype=torch.float16)
        inflight = agent.generate_inflight(tok, reqs, **kw)
        agent.prefix_cache = True
        first = agent.generate_inflight(tok, reqs, **kw)            # fills the prefix records
        cached = agent.generate_inflight(tok, reqs, **kw)           # the second pass reuses them: suffix prefills of a few rows
        stats = dict(agent.last_inflight_stats)
        agent.prefix_cache = False
        batch = agent.generate_batch(tok, [strip(r) for r in reqs[:4]], max_new_tokens=8, **kw)
        lw = llm._pack()["layers"][0]
        assert llm.weight_residency == res and torch.is_tensor(lw["wqkv"].w) == (res is None) and lw["wqkv"].format == "mxfp4"
        ids = lambda rs: [x["generate_ids"].tolist() for x in rs]
        out[res] = (ids(inflight), ids(first), ids(cached), ids(batch), stats["prefix_hit_tokens"] + stats["forked_tokens"])
        del agent, llm, lw
        torch.cuda.empty_cache()
    assert [len(x) for x in out["tiles"][0]] == budgets
    print(f"prefix rows reused by the third pass: {out['tiles'][4]}")
    assert out["tiles"][4] == out[None][4]                                          # the cached pass reused the same prefix rows
    for i, name in enumerate(("inflight", "inflight, prefix cache on", "inflight, prefix cache hit", "batch")):
        assert out["tiles"][i] == out[None][i], name


def test_tensor_parallel_tiles_residency(dev):
    """Two ranks on one GPU, launched as tests/test_tensor_parallel_gpu.py launches its ranks (virtual ranks: threads of this process
    through parallel.run_virtual_ranks, so one process holds the GPU), with that file's miniature dims: "mxfp4" + "tiles" against the same
    format at default residency — every rank dequantises its own slices into its own scratch buffer; rank 0's logits are identical."""
    from seedx_amd import ops
    from seedx_amd.llama import LlamaForCausalLM
    from seedx_amd.parallel import run_virtual_ranks
    from tests.test_tensor_parallel_gpu import TP_LLM
    dt, cfg = torch.float16, TP_LLM
    sd = weights.llama_sd(cfg)
    xe = torch.randn(1, 21, cfg["hidden_size"], generator=torch.Generator().manual_seed(3)) * 0.5

    def run(comm, res):
        torch.cuda.set_device(dev)
        llm = LlamaForCausalLM(dict(cfg), max_cache_len=64, max_batch=1, comm=comm, weight_format="mxfp4", weight_residency=res)
        llm.load_state_dict(dict(sd))
        llm.eval().to(dev, dt)
        out = llm(inputs_embeds=xe.to(dev))
        torch.cuda.synchronize()
        P = llm._P
        assert isinstance(P["layers"][0]["wd"].gemv_kwargs()["w"], ops.WeightShape) == (res == "tiles") == (P["layers"][0]["wd"].w is None)
        if res == "tiles":       # per-rank slices: gate|up [2 I / 2, H] is the largest
            assert P["w_scratch"].numel() == 2 * (cfg["intermediate_size"] // 2) * cfg["hidden_size"]
            assert tuple(P["layers"][0]["wd"].shape) == (cfg["hidden_size"], cfg["intermediate_size"] // 2)
        return out["logits"][0].float().cpu()
    a = run_virtual_ranks(2, lambda comm: run(comm, "tiles"))
    b = run_virtual_ranks(2, lambda comm: run(comm, None))
    assert a[0].shape[-1] >= cfg["vocab_size"] and bool(torch.isfinite(a[0]).all())
    assert torch.equal(a[0], b[0])
    assert torch.equal(a[1], a[0])                                                  # and the ranks agree
