"""MXFP4 (e2m1 codes, one E8M0 scale per 32-k block) decode tiles on the GPU (sx_gemv w_dtype = SX_FP4_E2M1,
LlamaForCausalLM(weight_format="mxfp4")).

As for the FP8 tiles (tests/test_fp8_weights_gpu.py) the claim under test is EXACTNESS against the 16-bit path on the dequantised weights:
the codes are converted in registers with their block scale (v_cvt_scalef32_pk_{f16,bf16}_fp4: every code * 2^e, e in [-13, 13], is a
normal 16-bit number), they feed the same MFMAs against the same x blocks over the same k-slices, and the epilogue is the 16-bit one. So:
every code at every k position decodes exactly under every block exponent (one-hot x); every kernel variant equals its 16-bit twin bit for
bit and the fp64 product of the dequantised weights at the 16-bit kernel's own bound (3e-6); the epilogues equal theirs; the MXFP4 model
equals the default precise model loaded with the dequantised state dict in prefill logits, decode ids and hidden states. What the mode
costs against the ORIGINAL weights is printed. Reference: modeling_llama_xformer.py:204-206, 239, 166-167 (the nn.Linear calls the skinny
GEMM replaces)."""
import math

import pytest
import torch

from oracle import restated, weights

pytestmark = pytest.mark.gpu
DTS = [torch.float16, torch.bfloat16]
# (N, K, glu, residual, layout) — the shapes of tests/test_fp8_weights_gpu.py, each selecting another variant of gemm_skinny_kernel
SHAPES = [(1536, 512, False, False, "t"),        # R = 1
          (5120, 1024, False, True, "t20"),      # 20-row tiles
          (5120, 5120, False, True, "t"),        # 320 16-row workgroups
          (2816, 512, True, False, "t"),         # GLU (R = 2)
          (640, 13824, False, True, "t"),        # split-K
          (15360, 512, False, False, "t"),       # 64-row workgroups
          (27648, 256, True, False, "t")]        # 64-row workgroups, GLU
_W = {}


def relerr(x, ref):
    x, ref = x.double().cpu(), ref.double().cpu()
    return ((x - ref).norm() / ref.norm()).item()


def _plane_rows(t16):
    """The bits a Tiled16 holds, [planes, rows, cols] (rows < M only: the padding rows belong to no comparison)."""
    nb = t16.t.shape[0] // t16.planes
    d = t16.t.view(t16.planes, nb, t16.cols // 32, 16, 32).permute(0, 1, 3, 2, 4).reshape(t16.planes, nb * 16, t16.cols)
    return d[:, :t16.rows].contiguous().view(torch.int16)


def _tiles4(codes, scale, rows):
    from seedx_amd import ops
    pack = ops.pack_decode_tiles_fp4 if rows == 16 else ops.pack_decode_tiles20_fp4
    return pack(codes.contiguous()), ops.pack_block_scales_fp4(scale.contiguous(), rows=rows)


def _quantised(dev, dt, N, K, glu, seed):
    """randn / sqrt(K) weights through the codec, once per (shape, dtype): (dequantised row-major [GLU-packed], 16-bit tiles, 16-bit 20-row
    tiles or None, MXFP4 (code tiles, scale tiles), the 20-row pair or None)."""
    from seedx_amd import ops, quant
    from seedx_amd.llama import glu_pack_rows
    key = (dt, N, K, glu)
    if key not in _W:
        g = torch.Generator().manual_seed(seed)
        w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dev, dt)
        codes, scale = quant.quantize_blocks_mxfp4(w)
        if glu:
            codes, scale = glu_pack_rows(codes[: N // 2], codes[N // 2:]), glu_pack_rows(scale[: N // 2], scale[N // 2:])
        wq = quant.dequantize_blocks_mxfp4(codes, scale, dt)
        assert torch.equal(wq.float().to(dt), wq)
        t20 = N % 20 == 0 and not glu
        _W[key] = (wq, ops.pack_decode_tiles(wq), ops.pack_decode_tiles20(wq) if t20 else None,
                   _tiles4(codes, scale, 16), _tiles4(codes, scale, 20) if t20 else None)
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
    """W[n][k] holds code (n + k) % 16: every k position of the row — both nibbles of every byte, both 32-k halves, every lane group and
    k-step — sees all 16 codes over the rows, W[n][k < 16] among them; the block exponents cycle -13 .. 13 over rows and blocks. x = one-hot
    rows (row m at k = s M + m, s = 0 .. K / M - 1, one launch each) as two planes: y[m][n] must BE decode(code[n][k]) * 2^e[n][k / 32]."""
    from seedx_amd import ops, quant
    K, N = 256, 512 if layout == "t" else 640
    n_i, k_i = torch.arange(N)[:, None], torch.arange(K)[None, :]
    nib = ((n_i + k_i) % 16).to(torch.uint8)
    assert all(set(nib[:, k].tolist()) == set(range(16)) for k in range(16))
    codes = (nib[:, 0::2] | (nib[:, 1::2] << 4)).to(dev)
    e = (n_i + 5 * torch.arange(K // 32)[None, :]) % 27 - 13
    assert e.min() == -13 and e.max() == 13 and set(e[:, 0].tolist()) == set(range(-13, 14))
    scale = (e + 127).to(torch.uint8).to(dev)
    wq = quant.dequantize_blocks_mxfp4(codes, scale, dt)
    tab = quant.decode_table_e2m1()
    want_all = (tab[nib.long()].double() * torch.pow(2.0, e.double()).repeat_interleave(32, dim=1)).float()
    assert torch.equal(wq.float().cpu(), want_all)                                  # the 16-bit copy holds the same model
    tiles = _tiles4(codes, scale, 16 if layout == "t" else 20)
    for s in range(K // M):
        x = torch.zeros(M, K, device=dev)
        x[torch.arange(M), s * M + torch.arange(M)] = 1.0
        xt = ops.split16(x, dt, tiled=True)
        y = ops.gemv(xt, wq, out_dtype=torch.float32, w_fp4=tiles)
        want = want_all[:, s * M:(s + 1) * M].T.contiguous().to(dev)
        bad = (y != want).nonzero()
        assert torch.equal(y, want), (s, bad[:8].tolist(), [(int(nib[n, s * M + m]), int(e[n, (s * M + m) // 32])) for m, n in bad[:8].tolist()])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,planes", [(1, 2), (11, 2), (16, 2), (21, 2), (32, 2), (8, 1), (24, 1)])
def test_fp4_gemv_against_fp64_and_its_16bit_twin(dev, dt, M, planes):
    from seedx_amd import ops
    g = torch.Generator().manual_seed(100 + M)
    for i, (N, K, glu, res, layout) in enumerate(SHAPES):
        wq, w_t, w_t20, f4, f4_20 = _quantised(dev, dt, N, K, glu, 50 + i)
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
        y4 = ops.gemv(xt, wq, w_fp4=f4_20 if layout == "t20" else f4, **kw)
        wd = wq.double()
        if glu:       # rows in GLU-packed order: 32-row groups [16 linear | 16 gate]
            wv = wd.view(N // 32, 2, 16, K)
            ref = (xr @ wv[:, 0].reshape(N // 2, K).T) * torch.nn.functional.silu(xr @ wv[:, 1].reshape(N // 2, K).T)
        else:
            ref = xr @ wd.T + (r.double() if res else 0.0)
        e = relerr(y4, ref)
        print(f"mxfp4 gemv {dt} M={M} planes={planes} {N}x{K} glu={glu} {layout}: vs fp64 {e:.2e}, == 16-bit twin {torch.equal(y4, y16)}")
        assert tuple(y4.shape) == (M, N // 2 if glu else N) and e < 3e-6
        assert torch.equal(y4, y16)
        assert int(ws[:16384].view(torch.int32).abs().sum()) == 0                 # split-K counters left at zero


def test_fp4_gemv_forced_split_k_factors(dev):
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
                wq, w_t, w_t20, f4, f4_20 = _quantised(dev, dt, N, K, glu, 51 + i)
                xt = ops.split16(torch.randn(M, K, generator=g).to(dev), dt, tiled=True)
                r = torch.randn(M, N, generator=g).to(dev)
                ws = torch.zeros(16384 + 8 * 32 * N * 4, dtype=torch.uint8, device=dev)
                y16 = ops.gemv(xt, wq, w_tiles=w_t, w_tiles20=w_t20 if layout == "t20" else None, residual=r, out_dtype=torch.float32, workspace=ws)
                y4 = ops.gemv(xt, wq, w_fp4=f4_20 if layout == "t20" else f4, residual=r, out_dtype=torch.float32, workspace=ws)
                assert torch.equal(y4, y16), (S, N, K)
                assert relerr(y4, xt.dense().double() @ wq.double().T + r.double()) < 3e-6
                assert int(ws[:16384].view(torch.int32).abs().sum()) == 0
    finally:
        _lib.check(lib.sx_gemv_tune(2, 0), "sx_gemv_tune")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M", [1, 16, 21])
def test_fp4_epilogues_equal_the_16bit_path(dev, dt, M):
    """(a) planes_out from the SiLU-GLU epilogue with a tiled output, (b) emit_norm with norm_gamma (y, x16 planes, sums of squares) on both
    row layouts, (c) a consumer of ssq_in — each torch.equal to the 16-bit kernel on the dequantised weights."""
    from seedx_amd import ops
    g = torch.Generator().manual_seed(40 + M)
    K, H, I2 = 512, 5120, 2816
    xt = ops.split16(torch.randn(M, K, generator=g).to(dev), dt, tiled=True)
    # (a)
    wk, wk_t, _, wk_4, _ = _quantised(dev, dt, I2, K, True, 61)
    y16 = ops.gemv(xt, wk, act="silu", glu=True, w_tiles=wk_t, y_tiled=True, planes_out=True)
    y4 = ops.gemv(xt, wk, act="silu", glu=True, w_fp4=wk_4, y_tiled=True, planes_out=True)
    assert y4.planes == y16.planes == 2 and torch.equal(_plane_rows(y4), _plane_rows(y16))        # hi and lo plane, bit for bit
    # (b)
    wo, wo_t, wo_t20, wo_4, wo_420 = _quantised(dev, dt, H, K, False, 62)
    res = torch.randn(M, H, generator=g).to(dev) * 3.0
    gam = (1.0 + 0.5 * torch.randn(H, generator=g)).abs().clamp_min(0.2).to(dev)
    ws = torch.zeros(16384 + 8 * 32 * H * 4, dtype=torch.uint8, device=dev)
    wq, wq_t, _, wq_4, _ = _quantised(dev, dt, 1536, H, False, 63)
    for layout in ("t", "t20"):
        kw = dict(residual=res, out_dtype=torch.float32, emit_norm=True, planes_out=True, norm_gamma=gam, workspace=ws)
        a_y, a_x16, a_ssq = ops.gemv(xt, wo, w_tiles=wo_t, w_tiles20=wo_t20 if layout == "t20" else None, **kw)
        b_y, b_x16, b_ssq = ops.gemv(xt, wo, w_fp4=wo_420 if layout == "t20" else wo_4, **kw)
        rows = 16 * ((M + 15) // 16)
        assert torch.equal(b_y, a_y) and b_x16.planes == a_x16.planes == 2 and torch.equal(_plane_rows(b_x16), _plane_rows(a_x16))
        assert b_ssq.shape == a_ssq.shape == (rows, 256 if layout == "t20" else 320) and torch.equal(b_ssq[:M], a_ssq[:M])
        # (c)
        a_out = ops.gemv(a_x16, wq, w_tiles=wq_t, out_dtype=torch.float32, ssq_in=(a_ssq, H, 1e-5))
        b_out = ops.gemv(b_x16, wq, w_fp4=wq_4, out_dtype=torch.float32, ssq_in=(b_ssq, H, 1e-5))
        assert torch.equal(b_out, a_out)
        yd = b_y.double()
        ref = (b_x16.dense().double() * torch.rsqrt(yd.pow(2).mean(-1, keepdim=True) + 1e-5)) @ wq.double().T
        assert relerr(b_out, ref) < 2e-6


def test_fp4_needs_tiles_block_scales_and_the_mfma_path(dev):
    """SX_ERR_INVALID with a message, never a fall-back: row-major W, missing block scales, a shape outside the MFMA path, w_scale set."""
    import ctypes as C
    from seedx_amd import _lib, ops
    lib = _lib.load()
    dt = torch.float16
    x = torch.zeros(8, 512, dtype=dt, device=dev)
    w = torch.zeros(64, 256, dtype=torch.uint8, device=dev)
    sc = torch.full((64, 16), 127, dtype=torch.uint8, device=dev)
    rs = torch.ones(64, device=dev)
    y = torch.empty(8, 64, dtype=torch.float32, device=dev)

    def call(**kw):
        a = _lib.GemvArgs()
        a.x, a.W, a.y, a.M, a.N, a.K = x.data_ptr(), w.data_ptr(), y.data_ptr(), 8, 64, 512
        a.dtype, a.out_dtype, a.w_layout, a.w_dtype, a.w_block_scale = _lib.SX_F16, _lib.SX_F32, 1, _lib.SX_FP4_E2M1, sc.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        st = lib.sx_gemv(C.byref(a), ops._stream())
        return st, lib.sx_last_error().decode()
    assert call()[0] == 0
    torch.cuda.synchronize()
    assert not y.any()                                            # code 0 everywhere: the launch ran and wrote zeros
    for kw in (dict(w_layout=0), dict(w_block_scale=None), dict(K=192), dict(w_scale=rs.data_ptr()),
               dict(w_block_scale=sc.data_ptr() + 2), dict(w_dtype=7)):
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
def test_fp4_model_equals_the_default_model_on_dequantised_weights(dev, dt):
    """H = 1024, 8 heads, FFN 2816, 3 layers, gammas far from 1; 4 ragged prompts, 6 decode steps. A = weight_format="mxfp4", B = the default
    precise model loaded with A's dequantised state dict: bit-identical prefill logits, decode ids and hidden states; graph replay ==
    eager. The deviation from the fp32 oracle on the ORIGINAL weights (the mode's cost) and on the dequantised ones is printed.

    Printed on the MI355X — see profiles/fp4_decode.md for the recorded figures."""
    from seedx_amd import quant
    from seedx_amd.llama import LlamaForCausalLM
    H, nh, I, L = 1024, 8, 2816, 3
    cfg = dict(hidden_size=H, intermediate_size=I, num_hidden_layers=L, num_attention_heads=nh, vocab_size=500, rms_norm_eps=1e-5,
               max_position_embeddings=128)
    g = torch.Generator().manual_seed(11)
    sd = {k: v.to(dt).float() for k, v in _gamma_far_from_one(weights.llama_sd(cfg), g).items()}
    sd_q, _, _ = quant.quantize_llama_state_dict({k: v.to(dev) for k, v in sd.items()}, cfg, dt, weight_format="mxfp4")
    sd_q = {k: v.float().cpu() for k, v in sd_q.items()}
    G, STEPS = 4, 6
    lens = [10, 7, 13, 4]
    xs = [torch.randn(t, H, generator=g) * 0.5 for t in lens]
    cur0 = torch.arange(20, 20 + G, dtype=torch.int32)
    img_ids = torch.arange(400, 466, dtype=torch.int32, device=dev)

    def build(state, **kw):
        llm = LlamaForCausalLM(dict(cfg), max_cache_len=64, max_batch=G, kv_v16=False, **kw)
        llm.load_state_dict(dict(state))
        llm.eval().to(dev, dtype=dt)
        return llm
    A = build(sd, weight_format="mxfp4")
    P = A._pack()
    assert A.precise and P["rms_fold_precise"] and P["decode_tiled"] and P["precise_tiled"]
    lw = P["layers"][0]
    # one handle per projection: MXFP4 codes + E8M0 scale tiles, no 16-bit and no FP8 tiles (the step is handed w_fp4 and nothing else)
    assert all(lw[k].format == "mxfp4" and {"w_tiles", "w_tiles20", "w_fp8", "w_fp4"} & set(lw[k].gemv_kwargs()) == {"w_fp4"}
               for k in ("wqkv", "wo", "wgu", "wd"))
    assert all(lw[k].tiles.dtype == lw[k].scales.dtype == torch.uint8 and lw[k].tiles.shape[2] == lw[k].tile_rows == 16 for k in ("wqkv", "wo", "wgu", "wd"))
    held = sum(t.numel() for l in P["layers"] for k in ("wqkv", "wo", "wgu", "wd") for t in (l[k].tiles, l[k].scales)) + P["lm_head_t"].numel() * 2
    assert held == sum(l[k].nbytes_tiles for l in P["layers"] for k in ("wqkv", "wo", "wgu", "wd")) + P["lm_head_t"].numel() * 2
    nk = 3 * H * H + H * H + 2 * I * H + H * I
    assert held == L * (nk // 2 + nk // 32) + A.V_l * H * 2
    assert A.memory_footprint()["decode_tiles"] == held and A.weight_quant_report["decode_tile_bytes"] == held
    rep = A.weight_quant_report
    # round-to-nearest e2m1 with the block maximum in [4, 8): 0.114 on Gaussian rows (tests/test_fp4_weights_cpu.py holds it in [0.10, 0.13])
    assert rep["weight_format"] == "mxfp4" and all(0.10 < v < 0.13 for v in rep["rel_frobenius_error"].values()), rep
    for k, name in (("wo", "self_attn.o_proj"), ("wd", "mlp.down_proj")):      # the row-major weights ARE the dequantised model
        assert torch.equal(lw[k].w.float().cpu(), sd_q[f"model.layers.0.{name}.weight"])
    a_log, a_ids, a_hid = _prefill_and_decode(A, dev, xs, cur0, img_ids, STEPS, use_graph=False)
    g_log, g_ids, g_hid = _prefill_and_decode(A, dev, xs, cur0, img_ids, STEPS, use_graph=True)
    assert torch.equal(g_log, a_log) and torch.equal(g_ids, a_ids) and torch.equal(g_hid, a_hid)          # graph replay == eager
    del A, P, lw
    torch.cuda.empty_cache()
    B = build(sd_q)
    PB = B._pack()
    assert B.weight_format is None and PB["rms_fold_precise"] and PB["layers"][0]["wqkv"].format is None and "w_tiles" in PB["layers"][0]["wqkv"].gemv_kwargs()
    b_log, b_ids, b_hid = _prefill_and_decode(B, dev, xs, cur0, img_ids, STEPS, use_graph=False)
    del B, PB
    torch.cuda.empty_cache()
    assert torch.equal(a_log, b_log), relerr(a_log, b_log)
    assert torch.equal(a_ids, b_ids) and (a_ids >= 0).all()
    assert torch.equal(a_hid, b_hid), relerr(a_hid, b_hid)
    # the fp32 oracle, teacher-forced on A's tokens: printed, on the dequantised weights and on the original ones (the mode's cost)
    emb = sd["model.embed_tokens.weight"]
    worst_q = worst_o = 0.0
    ids, hid = a_ids.cpu(), a_hid.cpu()
    for s in (0, 3):
        fed = [int(cur0[s])] + [int(t) for t in ids[s, :STEPS - 1]]
        x = torch.cat([xs[s], emb[torch.tensor(fed)]], dim=0).unsqueeze(0)
        _, _, hn = restated.llama_forward(sd_q, cfg, x, table_dtype=dt)
        worst_q = max(worst_q, relerr(hid[s], hn[0, lens[s]:]))
        _, _, hn0 = restated.llama_forward(sd, cfg, x, table_dtype=dt)
        worst_o = max(worst_o, relerr(hid[s], hn0[0, lens[s]:]))
    print(f"MXFP4 weights at model level, H={H} L={L} {dt}: decode hidden states vs oracle on the dequantised weights {worst_q:.2e}, "
          f"vs oracle on the ORIGINAL weights {worst_o:.2e}; rel. Frobenius error per projection {rep['rel_frobenius_error']}")


def test_fp4_serving_paths_agree(dev):
    """generate_inflight and generate_batch on a miniature model with weight_format="mxfp4" and kv_format="fp8_e4m3" return, request by
    request, the ids of the same calls on its twin: the default weight format loaded with the dequantised state dict, same KV format."""
    from seedx_amd import quant
    from seedx_amd.llama import LlamaForCausalLM
    from seedx_amd.seed_x import ContinuousLVLM
    from seedx_amd.visual_encoder import Resampler
    from tests.test_models_gpu import StubTokenizer
    cfg, VIT = weights.MINI_LLM, 128
    kw = dict(num_img_gen_tokens=16, eos_token_id=None)
    sd = {k: v.half().float() for k, v in weights.llama_sd(cfg).items()}
    sd_q, _, _ = quant.quantize_llama_state_dict(sd, cfg, torch.float16, weight_format="mxfp4")
    Hd = cfg["hidden_size"]
    tok = StubTokenizer()
    budgets = [9, 5, 12, 7, 6]
    reqs = [dict(input_ids=[[1, 10 + r] + [20 + r + i for i in range(3 + r % 5)]], max_new_tokens=b) for r, b in enumerate(budgets)]
    reqs[1].update(do_sample=True, temperature=1.0, top_k=50, top_p=0.9, seed=21)
    strip = lambda q: {k: v for k, v in q.items() if k != "max_new_tokens"}
    out = {}
    for name, state, fmt in (("fp4", sd, "mxfp4"), ("twin", sd_q, None)):
        llm = LlamaForCausalLM(dict(cfg), max_cache_len=512, max_batch=4, weight_format=fmt, kv_format="fp8_e4m3")
        llm.load_state_dict(dict(state))
        agent = ContinuousLVLM(llm, Resampler(4, Hd, 2, kv_dim=VIT), Resampler(4, VIT, 2, kv_dim=Hd), add_patch_pos=True)
        agent.load_state_dict(weights.agent_sd(cfg, VIT, in_grid=4, out_grid=4))
        agent.eval().to(dev, dtype=torch.float16)
        inflight = agent.generate_inflight(tok, reqs, **kw)
        batch = agent.generate_batch(tok, [strip(r) for r in reqs[:4]], max_new_tokens=8, **kw)
        lw = llm._pack()["layers"][0]
        assert llm.weight_format == fmt and llm.kv_format == "fp8_e4m3" and lw["wqkv"].format == fmt and (("w_fp4" in lw["wqkv"].gemv_kwargs()) == (fmt == "mxfp4"))
        out[name] = ([x["generate_ids"].tolist() for x in inflight], [x["generate_ids"].tolist() for x in batch])
        del agent, llm, lw
        torch.cuda.empty_cache()
    assert [len(x) for x in out["fp4"][0]] == budgets
    assert out["fp4"][0] == out["twin"][0]
    assert out["fp4"][1] == out["twin"][1]
    for r in range(4):                                    # and the two serving paths of the MXFP4 model agree with each other
        n = min(budgets[r], 8)
        assert out["fp4"][0][r][:n] == out["fp4"][1][r][:n], r
