"""Weight-only FP8 (e4m3) decode tiles on the GPU (sx_gemv w_dtype = SX_FP8_E4M3, LlamaForCausalLM(weight_format="fp8_e4m3")).

The claim under test is EXACTNESS against the 16-bit path on the dequantised weights, not closeness: the codes are converted in registers
without rounding, they feed the same MFMAs against the same x blocks in the same order, and the power-of-two row scale commutes with every
fp32 rounding. So: every code decodes exactly (one-hot x); every kernel variant equals its 16-bit twin bit for bit and the fp64 product of
the dequantised weights at the bound tests/test_precise_gpu.py::test_gemv_two_planes already holds that kernel to (3e-6); the epilogues
(planes out, RMSNorm fold producer and consumer) equal theirs; the FP8 model equals the default precise model loaded with the dequantised
state dict in prefill logits, decode ids and hidden states, and keeps the precise bounds (1e-4 fp16 / 8e-4 bf16, tests/
test_llm_plain16_gpu.py) against the fp32 oracle on the dequantised weights. What the mode costs against the ORIGINAL weights is printed.
Reference: modeling_llama_xformer.py:204-206, 239, 166-167 (the nn.Linear calls the skinny GEMM replaces)."""
import math

import pytest
import torch

from oracle import restated, weights

pytestmark = pytest.mark.gpu
DTS = [torch.float16, torch.bfloat16]
# (N, K, glu, residual, layout) — the shapes of test_gemv_two_planes, each selecting another variant of gemm_skinny_kernel
SHAPES = [(1536, 512, False, False, "t"),        # R = 1
          (5120, 1024, False, True, "t20"),      # 20-row tiles
          (5120, 5120, False, True, "t"),        # R = 2
          (2816, 512, True, False, "t"),         # GLU
          (640, 13824, False, True, "t"),        # split-K
          (15360, 512, False, False, "t"),       # 64-row workgroups
          (27648, 256, True, False, "t")]        # 64-row workgroups, GLU
_W = {}


def relerr(x, ref):
    x, ref = x.double().cpu(), ref.double().cpu()
    return ((x - ref).norm() / ref.norm()).item()


def _plane_rows(t16):
    """The bits a Tiled16 holds, [planes, rows, cols]: the kernels write rows < M only, the padding rows of the last row block are
    whatever the allocator left there and belong to no comparison."""
    nb = t16.t.shape[0] // t16.planes
    d = t16.t.view(t16.planes, nb, t16.cols // 32, 16, 32).permute(0, 1, 3, 2, 4).reshape(t16.planes, nb * 16, t16.cols)
    return d[:, :t16.rows].contiguous().view(torch.int16)


def _quantised(dev, dt, N, K, glu, seed):
    """randn / sqrt(K) weights through the codec, once per (shape, dtype): (dequantised row-major [GLU-packed], 16-bit tiles, 16-bit 20-row
    tiles or None, FP8 tiles, FP8 20-row tiles or None, scales)."""
    from seedx_amd import ops, quant
    from seedx_amd.llama import glu_pack_rows
    key = (dt, N, K, glu)
    if key not in _W:
        g = torch.Generator().manual_seed(seed)
        w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dev, dt)
        codes, scale = quant.quantize_rows(w)
        if glu:
            codes = glu_pack_rows(codes[: N // 2], codes[N // 2:])
            scale = glu_pack_rows(scale[: N // 2, None], scale[N // 2:, None]).reshape(-1).contiguous()
        wq = quant.dequantize_rows(codes, scale, dt)
        assert torch.equal(wq.float().to(dt), wq) and not ((codes & 0x7f) == 0x7f).any()
        t20 = N % 20 == 0 and not glu
        _W[key] = (wq, ops.pack_decode_tiles(wq), ops.pack_decode_tiles20(wq) if t20 else None,
                   ops.pack_decode_tiles_fp8(codes), ops.pack_decode_tiles20_fp8(codes) if t20 else None, scale)
    return _W[key]


@pytest.fixture(scope="module", autouse=True)
def _free_weights():
    yield
    _W.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M", [16, 32])
@pytest.mark.parametrize("layout", ["t", "t20"])
def test_every_code_decodes_exactly(dev, dt, M, layout):
    """W[n][k < 16] runs through all 254 non-NaN codes, the rest are random codes; row scales 2^-15 .. 2^7; x = one-hot rows (k = m) as two
    planes: y[m][n] must BE decode(code[n][m]) * scale[n]."""
    from seedx_amd import ops, quant
    K, N = 256, 512 if layout == "t" else 640
    g = torch.Generator().manual_seed(7)
    valid = torch.tensor([c for c in range(256) if c & 0x7f != 0x7f], dtype=torch.uint8)
    codes = valid[torch.randint(0, 254, (N, K), generator=g)]
    codes[:, :16] = valid[(torch.arange(N)[:, None] * 16 + torch.arange(16)[None, :]) % 254]
    assert set(codes[:, :16].unique().tolist()) == set(valid.tolist())
    codes = codes.to(dev)
    scale = torch.pow(2.0, ((torch.arange(N) % 23) - 15).double()).float().to(dev)
    assert scale.min().item() == 2.0 ** -15 and scale.max().item() == 2.0 ** 7
    wq = quant.dequantize_rows(codes, scale, dt)
    assert torch.equal(wq.float(), quant.decode_table(dev)[codes.long()] * scale[:, None])       # the 16-bit copy holds the same model
    x = torch.zeros(M, K, device=dev)
    x[torch.arange(M), torch.arange(M)] = 1.0
    xt = ops.split16(x, dt, tiled=True)
    tiles = ops.pack_decode_tiles_fp8(codes) if layout == "t" else ops.pack_decode_tiles20_fp8(codes)
    y = ops.gemv(xt, wq, out_dtype=torch.float32, w_fp8=(tiles, scale))
    want = wq.float()[:, :M].T.contiguous()
    bad = (y != want).nonzero()
    assert torch.equal(y, want), (bad[:8].tolist(), [hex(int(codes[n, m])) for m, n in bad[:8].tolist()])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,planes", [(1, 2), (11, 2), (16, 2), (21, 2), (32, 2), (8, 1), (24, 1)])
def test_fp8_gemv_against_fp64_and_its_16bit_twin(dev, dt, M, planes):
    from seedx_amd import ops
    g = torch.Generator().manual_seed(100 + M)
    for i, (N, K, glu, res, layout) in enumerate(SHAPES):
        wq, w_t, w_t20, f8, f8_20, scale = _quantised(dev, dt, N, K, glu, 50 + i)
        x = torch.randn(M, K, generator=g).to(dev)
        r = torch.randn(M, N, generator=g).to(dev) if res else None
        if planes == 2:
            xt = ops.split16(x, dt, tiled=True)
            xr = xt.dense().double()
        else:
            xt = x.to(dt).contiguous()
            xr = xt.double()
        ws = torch.zeros(16384 + 8 * 32 * N * 4, dtype=torch.uint8, device=dev)
        kw = dict(residual=r, act="silu" if glu else None, glu=glu, out_dtype=torch.float32, workspace=ws)
        # the split-K factor follows K, the workgroup count and the layout only (sx_gemv): the same automatic choice on both sides
        y16 = ops.gemv(xt, wq, w_tiles=w_t, w_tiles20=w_t20 if layout == "t20" else None, **kw)
        y8 = ops.gemv(xt, wq, w_fp8=(f8_20 if layout == "t20" else f8, scale), **kw)
        wd = wq.double()
        if glu:       # rows in GLU-packed order: 32-row groups [16 linear | 16 gate]
            wv = wd.view(N // 32, 2, 16, K)
            ref = (xr @ wv[:, 0].reshape(N // 2, K).T) * torch.nn.functional.silu(xr @ wv[:, 1].reshape(N // 2, K).T)
        else:
            ref = xr @ wd.T + (r.double() if res else 0.0)
        e = relerr(y8, ref)
        print(f"fp8 gemv {dt} M={M} planes={planes} {N}x{K} glu={glu} {layout}: vs fp64 {e:.2e}, == 16-bit twin {torch.equal(y8, y16)}")
        assert tuple(y8.shape) == (M, N // 2 if glu else N) and e < 3e-6
        assert torch.equal(y8, y16)
        assert int(ws[:16384].view(torch.int32).abs().sum()) == 0                 # split-K counters left at zero


def test_fp8_gemv_forced_split_k_factors(dev):
    """The forced split-K factors (sx_gemv_tune key 2) on the 20-row tiles and the 16-row tiles: still the bits of the 16-bit twin at the
    same factor. The hook is restored."""
    from seedx_amd import _lib, ops
    dt, M = torch.float16, 16
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)
    try:
        for S in (2, 8):
            _lib.check(lib.sx_gemv_tune(2, S), "sx_gemv_tune")
            for i, (N, K, glu, res, layout) in enumerate(SHAPES[1:3]):
                wq, w_t, w_t20, f8, f8_20, scale = _quantised(dev, dt, N, K, glu, 51 + i)
                xt = ops.split16(torch.randn(M, K, generator=g).to(dev), dt, tiled=True)
                r = torch.randn(M, N, generator=g).to(dev)
                ws = torch.zeros(16384 + 8 * 32 * N * 4, dtype=torch.uint8, device=dev)
                y16 = ops.gemv(xt, wq, w_tiles=w_t, w_tiles20=w_t20 if layout == "t20" else None, residual=r, out_dtype=torch.float32, workspace=ws)
                y8 = ops.gemv(xt, wq, w_fp8=(f8_20 if layout == "t20" else f8, scale), residual=r, out_dtype=torch.float32, workspace=ws)
                assert torch.equal(y8, y16), (S, N, K)
                assert relerr(y8, xt.dense().double() @ wq.double().T + r.double()) < 3e-6
                assert int(ws[:16384].view(torch.int32).abs().sum()) == 0
    finally:
        _lib.check(lib.sx_gemv_tune(2, 0), "sx_gemv_tune")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M", [1, 16, 21])
def test_fp8_epilogues_equal_the_16bit_path(dev, dt, M):
    """The pattern of test_gemv_plane_outputs_and_precise_rmsnorm_fold with FP8 tiles: (a) planes_out from the SiLU-GLU epilogue (two rows
    of different scale per output), (b) emit_norm with norm_gamma (y, x16 planes, sums of squares), (c) a consumer of ssq_in — each
    torch.equal to the 16-bit kernel on the dequantised weights."""
    from seedx_amd import ops
    g = torch.Generator().manual_seed(40 + M)
    K, H, I2 = 512, 5120, 2816
    xt = ops.split16(torch.randn(M, K, generator=g).to(dev), dt, tiled=True)
    # (a)
    wk, wk_t, _, wk_8, _, sk = _quantised(dev, dt, I2, K, True, 61)
    y16 = ops.gemv(xt, wk, act="silu", glu=True, w_tiles=wk_t, y_tiled=True, planes_out=True)
    y8 = ops.gemv(xt, wk, act="silu", glu=True, w_fp8=(wk_8, sk), y_tiled=True, planes_out=True)
    assert y8.planes == y16.planes == 2 and torch.equal(_plane_rows(y8), _plane_rows(y16))        # hi and lo plane, bit for bit
    # (b)
    wo, wo_t, wo_t20, wo_8, wo_820, so = _quantised(dev, dt, H, K, False, 62)
    res = torch.randn(M, H, generator=g).to(dev) * 3.0
    gam = (1.0 + 0.5 * torch.randn(H, generator=g)).abs().clamp_min(0.2).to(dev)
    ws = torch.zeros(16384 + 8 * 32 * H * 4, dtype=torch.uint8, device=dev)
    wq, wq_t, _, wq_8, _, sq = _quantised(dev, dt, 1536, H, False, 63)
    for layout in ("t", "t20"):
        kw = dict(residual=res, out_dtype=torch.float32, emit_norm=True, planes_out=True, norm_gamma=gam, workspace=ws)
        a_y, a_x16, a_ssq = ops.gemv(xt, wo, w_tiles=wo_t, w_tiles20=wo_t20 if layout == "t20" else None, **kw)
        b_y, b_x16, b_ssq = ops.gemv(xt, wo, w_fp8=(wo_820 if layout == "t20" else wo_8, so), **kw)
        rows = 16 * ((M + 15) // 16)
        assert torch.equal(b_y, a_y) and b_x16.planes == a_x16.planes == 2 and torch.equal(_plane_rows(b_x16), _plane_rows(a_x16))
        assert b_ssq.shape == a_ssq.shape == (rows, 256 if layout == "t20" else 320) and torch.equal(b_ssq[:M], a_ssq[:M])
        # (c)
        a_out = ops.gemv(a_x16, wq, w_tiles=wq_t, out_dtype=torch.float32, ssq_in=(a_ssq, H, 1e-5))
        b_out = ops.gemv(b_x16, wq, w_fp8=(wq_8, sq), out_dtype=torch.float32, ssq_in=(b_ssq, H, 1e-5))
        assert torch.equal(b_out, a_out)
        yd = b_y.double()
        ref = (b_x16.dense().double() * torch.rsqrt(yd.pow(2).mean(-1, keepdim=True) + 1e-5)) @ wq.double().T
        assert relerr(b_out, ref) < 2e-6


def test_fp8_needs_tiles_scales_and_the_mfma_path(dev):
    """SX_ERR_INVALID with a message, never a fall-back: row-major W, a missing scale, a shape outside the MFMA path."""
    import ctypes as C
    from seedx_amd import _lib, ops
    lib = _lib.load()
    dt = torch.float16
    x = torch.zeros(8, 512, dtype=dt, device=dev)
    w = torch.zeros(64, 512, dtype=torch.uint8, device=dev)
    sc = torch.ones(64, device=dev)
    y = torch.empty(8, 64, dtype=torch.float32, device=dev)

    def call(**kw):
        a = _lib.GemvArgs()
        a.x, a.W, a.y, a.M, a.N, a.K = x.data_ptr(), w.data_ptr(), y.data_ptr(), 8, 64, 512
        a.dtype, a.out_dtype, a.w_layout, a.w_dtype, a.w_scale = _lib.SX_F16, _lib.SX_F32, 1, _lib.SX_FP8_E4M3, sc.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        st = lib.sx_gemv(C.byref(a), ops._stream())
        return st, lib.sx_last_error().decode()
    assert call()[0] == 0
    for kw in (dict(w_layout=0), dict(w_scale=None), dict(K=192), dict(w_dtype=7), dict(w_dtype=0)):
        st, msg = call(**kw)
        assert st == 1 and "sx_gemv" in msg, (kw, st, msg)
    torch.cuda.synchronize()


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


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H,nh,I,L", [(1024, 8, 2816, 3), (5120, 40, 13824, 2)])
def test_fp8_model_equals_the_default_model_on_dequantised_weights(dev, dt, H, nh, I, L):
    """Geometries and procedure of tests/test_llm_plain16_gpu.py. A = weight_format="fp8_e4m3", B = the default precise model loaded with
    A's dequantised state dict: bit-identical prefill logits, decode ids and hidden states; A inside the precise bounds against the fp32
    oracle on the dequantised weights; graph replay == eager; one run at 20 sequences (four operand blocks per weight fragment)."""
    from seedx_amd import quant
    from seedx_amd.llama import LlamaForCausalLM
    cfg = dict(hidden_size=H, intermediate_size=I, num_hidden_layers=L, num_attention_heads=nh, vocab_size=500, rms_norm_eps=1e-5,
               max_position_embeddings=128)
    g = torch.Generator().manual_seed(11)
    sd = {k: v.to(dt).float() for k, v in _gamma_far_from_one(weights.llama_sd(cfg), g).items()}
    sd_q, _, _ = quant.quantize_llama_state_dict({k: v.to(dev) for k, v in sd.items()}, cfg, dt)
    sd_q = {k: v.float().cpu() for k, v in sd_q.items()}
    G, T0, STEPS = 8, 10, 4
    xs = [torch.randn(T0, H, generator=g) * 0.5 for _ in range(20)]
    cur0 = torch.arange(20, 40, dtype=torch.int32)
    img_ids = torch.arange(400, 466, dtype=torch.int32, device=dev)

    def build(state, n, **kw):
        llm = LlamaForCausalLM(dict(cfg), max_cache_len=64, max_batch=n, kv_v16=False, **kw)
        llm.load_state_dict(dict(state))
        llm.eval().to(dev, dtype=dt)
        return llm
    A = build(sd, G, weight_format="fp8_e4m3")
    P = A._pack()
    assert A.precise and P["rms_fold_precise"] and P["decode_tiled"] and P["precise_tiled"]
    lw = P["layers"][0]
    # one handle per projection: FP8 codes + fp32 row scales, no 16-bit tiles (the step is handed w_fp8 and nothing else)
    assert all(lw[k].format == "fp8_e4m3" and lw[k].tiles.dtype == torch.uint8 and lw[k].scales.dtype == torch.float32
               and {"w_tiles", "w_tiles20", "w_fp8", "w_fp4"} & set(lw[k].gemv_kwargs()) == {"w_fp8"} for k in ("wqkv", "wo", "wgu", "wd"))
    rows = [16, 20, 16, 20] if H == 5120 else [16] * 4
    assert [lw[k].tile_rows for k in ("wqkv", "wo", "wgu", "wd")] == rows == [lw[k].tiles.shape[2] for k in ("wqkv", "wo", "wgu", "wd")]
    held = sum(l[k].nbytes_tiles for l in P["layers"] for k in ("wqkv", "wo", "wgu", "wd")) + P["lm_head_t"].numel() * 2
    assert held == sum(t.numel() * t.element_size() for l in P["layers"] for k in ("wqkv", "wo", "wgu", "wd") for t in (l[k].tiles, l[k].scales)) \
        + P["lm_head_t"].numel() * 2
    assert A.memory_footprint()["decode_tiles"] == held and A.weight_quant_report["decode_tile_bytes"] == held
    # e4m3 rounds a normal value by at most 2^-4 of itself; the subnormal tail (|w| < amax / 2^13) adds < 1e-3 of the row norm
    assert all(0.0 < v < 0.064 for v in A.weight_quant_report["rel_frobenius_error"].values()), A.weight_quant_report
    for k in ("wqkv", "wo", "wd"):                                   # the row-major weights ARE the dequantised model
        name = {"wo": "self_attn.o_proj", "wd": "mlp.down_proj"}.get(k)
        if name:
            assert torch.equal(lw[k].w.float().cpu(), sd_q[f"model.layers.0.{name}.weight"])
    a_log, a_ids, a_hid = _prefill_and_decode(A, dev, xs[:G], cur0[:G], img_ids, STEPS, use_graph=False)
    g_log, g_ids, g_hid = _prefill_and_decode(A, dev, xs[:G], cur0[:G], img_ids, STEPS, use_graph=True)
    assert torch.equal(g_log, a_log) and torch.equal(g_ids, a_ids) and torch.equal(g_hid, a_hid)          # graph replay == eager
    del A, P, lw
    torch.cuda.empty_cache()
    B = build(sd_q, G)
    PB = B._pack()
    assert B.weight_format is None and PB["rms_fold_precise"] and PB["layers"][0]["wqkv"].format is None and "w_tiles" in PB["layers"][0]["wqkv"].gemv_kwargs()
    b_log, b_ids, b_hid = _prefill_and_decode(B, dev, xs[:G], cur0[:G], img_ids, STEPS, use_graph=False)
    del B, PB
    torch.cuda.empty_cache()
    assert torch.equal(a_log, b_log), relerr(a_log, b_log)
    assert torch.equal(a_ids, b_ids) and (a_ids >= 0).all()
    assert torch.equal(a_hid, b_hid), relerr(a_hid, b_hid)
    # one run at 20 sequences: MB = 4 kernels end to end
    A20 = build(sd, 20, weight_format="fp8_e4m3")
    _, ids20, hid20 = _prefill_and_decode(A20, dev, xs, cur0, img_ids, STEPS, use_graph=False)
    del A20
    torch.cuda.empty_cache()
    # the fp32 oracle, teacher-forced on A's tokens: on the dequantised weights (asserted), on the original ones (printed: the mode's cost)
    tol = {torch.float16: 1e-4, torch.bfloat16: 8e-4}[dt]
    emb = sd["model.embed_tokens.weight"]
    worst_q = worst_o = worst_20 = 0.0
    for ids, hid, seqs in ((a_ids.cpu(), a_hid.cpu(), (0, 3, 7)), (ids20.cpu(), hid20.cpu(), (5, 18))):
        for s in seqs:
            fed = [int(cur0[s])] + [int(t) for t in ids[s, :STEPS - 1]]
            x = torch.cat([xs[s], emb[torch.tensor(fed)]], dim=0).unsqueeze(0)
            _, _, hn = restated.llama_forward(sd_q, cfg, x, table_dtype=dt)
            e = relerr(hid[s], hn[0, T0:])
            if len(seqs) == 3:
                worst_q = max(worst_q, e)
                _, _, hn0 = restated.llama_forward(sd, cfg, x, table_dtype=dt)
                worst_o = max(worst_o, relerr(hid[s], hn0[0, T0:]))
            else:
                worst_20 = max(worst_20, e)
    print(f"FP8 weights at model level, H={H} L={L} {dt}: decode hidden states vs oracle on the dequantised weights {worst_q:.2e} "
          f"(20 sequences {worst_20:.2e}), vs oracle on the ORIGINAL weights {worst_o:.2e}")
    assert worst_q < tol and worst_20 < tol


def test_fp8_serving_paths_agree(dev):
    """generate_inflight on a miniature FP8 model — 6 mixed greedy / sampled requests on 4 slots — returns, request by request, the ids
    of generate_batch on the same model (the property tests/test_inflight_gpu.py holds the 16-bit precise model to)."""
    from seedx_amd.llama import LlamaForCausalLM
    from seedx_amd.seed_x import ContinuousLVLM
    from seedx_amd.visual_encoder import Resampler
    from tests.test_models_gpu import StubTokenizer
    cfg, VIT = weights.MINI_LLM, 128
    kw = dict(num_img_gen_tokens=16, eos_token_id=None)
    llm = LlamaForCausalLM(dict(cfg), max_cache_len=512, max_batch=4, weight_format="fp8_e4m3")
    llm.load_state_dict(weights.llama_sd(cfg))
    Hd = cfg["hidden_size"]
    agent = ContinuousLVLM(llm, Resampler(4, Hd, 2, kv_dim=VIT), Resampler(4, VIT, 2, kv_dim=Hd), add_patch_pos=True)
    agent.load_state_dict(weights.agent_sd(cfg, VIT, in_grid=4, out_grid=4))
    agent.eval().to(dev, dtype=torch.float16)
    tok = StubTokenizer()
    budgets = [9, 5, 12, 7, 6, 10]
    reqs = [dict(input_ids=[[1, 10 + r] + [20 + r + i for i in range(3 + r % 5)]], max_new_tokens=b) for r, b in enumerate(budgets)]
    for r, s in ((1, 21), (2, 22), (5, 23)):
        reqs[r].update(do_sample=True, temperature=1.0, top_k=50, top_p=0.9, seed=s)
    got = agent.generate_inflight(tok, reqs, **kw)
    assert llm.weight_format == "fp8_e4m3" and llm._pack()["layers"][0]["wqkv"].format == "fp8_e4m3" and llm._pack()["layers"][0]["wqkv"].tiles.dtype == torch.uint8
    assert [len(x["generate_ids"]) for x in got] == budgets
    strip = lambda q: {k: v for k, v in q.items() if k != "max_new_tokens"}
    for wave in ([0, 1, 2, 3], [4, 5, 0, 1]):
        ref = agent.generate_batch(tok, [strip(reqs[r]) for r in wave], max_new_tokens=12, **kw)
        for i, r in enumerate(wave):
            assert got[r]["generate_ids"].tolist() == ref[i]["generate_ids"].tolist()[:budgets[r]], (r, got[r]["generate_ids"].tolist())
