"""Host side of the weight-only FP8 (e4m3) decode mode: the codec (seedx_amd/quant.py) against torch's own float8_e4m3fn, exactness of the
dequantised values in fp16 and bf16, idempotence, the FP8 tile layouts against the index map of include/seedx_hip.h, tensor-parallel
consistency (quantise, then slice == slices of the quantised model), mode selection and memory_footprint(). No GPU."""
import pytest
import torch

from oracle import weights

NAN_CODES = (0x7f, 0xff)


def _not_nan(codes):
    return (codes & 0x7f) != 0x7f


def test_codec_matches_torch_for_every_finite_fp16():
    """All 63 488 finite fp16 values at s = 0: the codes are torch's clamp + float8_e4m3fn cast, bit for bit (-0 included)."""
    from seedx_amd import quant
    v = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.float16)
    v = v[torch.isfinite(v)]
    assert v.numel() == 63488
    got = quant.encode_e4m3(v.float())
    want = v.float().clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(got, want)
    assert _not_nan(got).all()


def test_decode_matches_torch_for_every_code():
    from seedx_amd import quant
    codes = torch.arange(256, dtype=torch.uint8)
    ok = _not_nan(codes)
    assert int(ok.sum()) == 254
    want = codes.view(torch.float8_e4m3fn).float()
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        got = quant.dequantize_rows(codes[ok][None, :], torch.ones(1), dt)[0]
        assert got.dtype == dt and torch.equal(got.float(), want[ok])
    assert torch.isnan(quant.decode_table()[list(NAN_CODES)]).all()


def _rows_spanning_the_clamp_range(dt):
    g = torch.Generator().manual_seed(3)
    K = 192
    amax = [65504.0, 40000.0, 448.0 * 128, 448.0, 447.9, 448.1, 3.0, 1.0, 0.02, 1e-3, 448.0 * 2.0 ** -15, 1e-4, 1e-6, 6e-8]
    rows = [torch.randn(K, generator=g) for _ in amax]
    rows = [r / r.abs().max() * a for r, a in zip(rows, amax)]
    rows += [torch.zeros(K), torch.randn(K, generator=g) * 0.02, torch.rand(K, generator=g) * 1e-5]
    big = torch.finfo(dt).max if dt == torch.float16 else 65504.0            # same clamp bounds for bf16: stay inside fp16's range
    return torch.stack(rows).clamp(-big, big).to(dt)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_random_rows_exact_idempotent_and_nan_free(dt):
    from seedx_amd import quant
    w = _rows_spanning_the_clamp_range(dt)
    codes, scale = quant.quantize_rows(w)
    assert codes.dtype == torch.uint8 and codes.shape == w.shape and scale.dtype == torch.float32 and scale.shape == (w.shape[0],)
    s = torch.log2(scale)
    assert torch.equal(s, s.round()) and s.min() == -15 and s.max() == 7       # powers of two over the whole clamp range
    assert scale[14] == 1.0 and not codes[14].any()                              # the all-zero row: s = 0, codes 0
    assert _not_nan(codes).all()
    x = quant.dequantize_rows(codes, scale, torch.float32)
    for d2 in (torch.float16, torch.bfloat16):                                   # the dequantised model is exact in BOTH 16-bit types
        assert torch.equal(x.to(d2).float(), x)
    c2, s2 = quant.quantize_rows(quant.dequantize_rows(codes, scale, dt))
    assert torch.equal(c2, codes) and torch.equal(s2, scale)
    # rows whose amax / scale fits e4m3: the row maximum uses the top binade and every value is within half a quantum (2^-4 relative)
    inside = (s > -15) & (s < 7) & (w.float().abs().amax(1) > 0)
    top = x[inside].abs().amax(1) / scale[inside]
    assert (top > 224).all() and (top <= 448).all()
    big = w.float().abs() >= (2.0 ** -6) * scale[:, None]
    rel = ((x - w.float()).abs() / w.float().abs().clamp_min(1e-30))[big & inside[:, None]]
    assert rel.max() <= 2.0 ** -4


def test_quantisation_error_on_gaussian_rows():
    """N(0, 0.02^2) rows of K = 5120: the figure the mode costs per projection (2.65 % relative rms)."""
    from seedx_amd import quant
    w = (torch.randn(64, 5120, generator=torch.Generator().manual_seed(0)) * 0.02).half()
    codes, scale = quant.quantize_rows(w)
    e = ((quant.dequantize_rows(codes, scale) - w.float()).norm() / w.float().norm()).item()
    assert 0.024 < e < 0.029, e


def _k_of_byte(t, p):
    """include/seedx_hip.h: byte p = 16 g + 8 h + j of k-slab t holds k = 64 t + 32 h + 8 g + j."""
    g, h, j = p // 16, (p // 8) % 2, p % 8
    return 64 * t + 32 * h + 8 * g + j


@pytest.mark.parametrize("rows", [16, 20])
def test_pack_functions_round_trip_through_the_stated_index_map(rows):
    from seedx_amd import ops
    N, K = 4 * rows * 2, 192
    codes = torch.randint(0, 256, (N, K), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    t = (ops.pack_decode_tiles_fp8 if rows == 16 else ops.pack_decode_tiles20_fp8)(codes)
    assert t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == (N // rows, K // 64, rows, 64)
    back = torch.empty_like(codes)
    kmap = torch.tensor([[_k_of_byte(s, p) for p in range(64)] for s in range(K // 64)])          # [slab][byte] → k
    for grp in range(N // rows):
        for s in range(K // 64):
            back[grp * rows:(grp + 1) * rows, kmap[s]] = t[grp, s]
    assert torch.equal(back, codes)
    # a lane's 16 bytes: row r, lane group g → its eight k-slots of the first 32-k half, then of the second
    r, g, s = 5, 2, 1
    lane = t[1, s, r, 16 * g:16 * g + 16]
    assert torch.equal(lane[:8], codes[rows + r, 64 * s + 8 * g:64 * s + 8 * g + 8])
    assert torch.equal(lane[8:], codes[rows + r, 64 * s + 32 + 8 * g:64 * s + 32 + 8 * g + 8])
    if rows == 20:                                   # rows 16..19 sit behind the 1-KB tile of rows 0..15
        flat = t[1, s].reshape(-1)
        assert torch.equal(flat[1024 + 64 * 2:1024 + 64 * 3], t[1, s, 18])


def test_glu_packed_scales_follow_their_rows():
    from seedx_amd import quant
    from seedx_amd.llama import glu_pack_rows
    g = torch.Generator().manual_seed(2)
    I, K = 64, 128
    up = (torch.randn(I, K, generator=g) * torch.logspace(-3, 1, I)[:, None]).half()
    gate = (torch.randn(I, K, generator=g) * torch.logspace(1, -3, I)[:, None]).half()
    (cu, su), (cg, sg) = quant.quantize_rows(up), quant.quantize_rows(gate)
    codes = glu_pack_rows(cu, cg)
    scale = glu_pack_rows(su[:, None], sg[:, None]).reshape(-1)
    assert su.unique().numel() > 4
    want = glu_pack_rows(quant.dequantize_rows(cu, su), quant.dequantize_rows(cg, sg))
    assert torch.equal(quant.dequantize_rows(codes, scale), want)
    c2, s2 = quant.quantize_rows(glu_pack_rows(up, gate))                      # packing first, quantising second: the same rows
    assert torch.equal(c2, codes) and torch.equal(s2, scale)


def test_tp_slices_of_one_quantised_model():
    """tp = 2, miniature geometry: quantise the full matrices, then llama_tp_shard == the shards of the quantised matrices — codes,
    dequantised weights and scales (row-sharded q / k / v / gate / up slice theirs, column-sharded o / down replicate)."""
    from seedx_amd import quant
    from seedx_amd.parallel import llama_tp_shard
    cfg = dict(weights.MINI_LLM, num_hidden_layers=1)
    nh, hd = cfg["num_attention_heads"], cfg["hidden_size"] // cfg["num_attention_heads"]
    sd = weights.llama_sd(cfg)
    p = "model.layers.0."
    sd_q, codes, scales = quant.quantize_llama_state_dict(sd, cfg, torch.float16)
    assert sorted(codes) == sorted(scales) == sorted(p + n + ".weight" for n in quant.LLAMA_PROJECTIONS)
    for k in ("model.embed_tokens.weight", "lm_head.weight", "model.norm.weight", p + "input_layernorm.weight"):
        assert sd_q[k] is sd[k]                                                # embedding, norms and lm_head stay as they are
    names = {"q": "self_attn.q_proj", "k": "self_attn.k_proj", "v": "self_attn.v_proj", "o": "self_attn.o_proj",
             "gate": "mlp.gate_proj", "up": "mlp.up_proj", "down": "mlp.down_proj"}
    whole = {}
    for rank in range(2):
        w = llama_tp_shard(sd_q, p, rank, 2, nh, hd)
        c = llama_tp_shard(codes, p, rank, 2, nh, hd)
        s = quant.llama_tp_shard_scales(scales, p, rank, 2, nh, hd)
        for k in names:
            assert torch.equal(quant.dequantize_rows(c[k].contiguous(), s[k]), w[k].float()), (rank, k)
            whole.setdefault(k, []).append((c[k], s[k]))
            assert s[k].shape == (w[k].shape[0],)
    for k, name in names.items():
        col = k in ("o", "down")
        full_c = torch.cat([c for c, _ in whole[k]], dim=1 if col else 0)
        assert torch.equal(full_c, codes[p + name + ".weight"])
        if col:
            assert torch.equal(whole[k][0][1], whole[k][1][1]) and torch.equal(whole[k][0][1], scales[p + name + ".weight"])
        else:
            assert torch.equal(torch.cat([s for _, s in whole[k]]), scales[p + name + ".weight"])
        # a rank's row-sharded slice would quantise to the same codes on its own (per-row scales); a column-sharded one would NOT in
        # general (its row maximum may sit in the other rank's columns) — which is why the full matrices are quantised first
        if not col:
            c0, s0 = quant.quantize_rows(llama_tp_shard(sd, p, 0, 2, nh, hd)[k].half())
            assert torch.equal(c0, whole[k][0][0]) and torch.equal(s0, whole[k][0][1])


def test_mode_selection(monkeypatch):
    from seedx_amd.llama import LlamaForCausalLM
    cfg = dict(weights.MINI_LLM)
    monkeypatch.delenv("SX_LLM_WEIGHTS", raising=False)
    monkeypatch.delenv("SX_LLM_PRECISE", raising=False)
    assert LlamaForCausalLM(dict(cfg), max_cache_len=64).weight_format is None
    m = LlamaForCausalLM(dict(cfg), max_cache_len=64, max_batch=4, weight_format="fp8_e4m3")
    assert m.weight_format == "fp8_e4m3" and m.precise and m.weight_quant_report is None
    with pytest.raises(ValueError, match="precise"):
        LlamaForCausalLM(dict(cfg), max_cache_len=64, weight_format="fp8_e4m3", precise=False)
    with pytest.raises(ValueError, match="weight_format"):
        LlamaForCausalLM(dict(cfg), max_cache_len=64, weight_format="int4")
    with pytest.raises(ValueError, match="skinny GEMM"):                       # FFN width 176 per rank is no multiple of 64: no tiled decode path
        LlamaForCausalLM(dict(cfg, intermediate_size=176), max_cache_len=64, weight_format="fp8_e4m3")
    monkeypatch.setenv("SX_LLM_WEIGHTS", "fp8_e4m3")                            # the A/B switch
    assert LlamaForCausalLM(dict(cfg), max_cache_len=64).weight_format == "fp8_e4m3"
    with pytest.raises(ValueError, match="precise"):
        LlamaForCausalLM(dict(cfg), max_cache_len=64, precise=False)
    monkeypatch.setenv("SX_LLM_PRECISE", "0")
    with pytest.raises(ValueError, match="precise"):
        LlamaForCausalLM(dict(cfg), max_cache_len=64)


def test_from_pretrained_carries_the_keyword(tmp_path):
    import json
    from safetensors.torch import save_file
    from seedx_amd.llama import LlamaForCausalLM
    cfg = dict(weights.MINI_LLM, num_hidden_layers=1)
    json.dump(cfg, open(tmp_path / "config.json", "w"))
    save_file({k: v.contiguous() for k, v in weights.llama_sd(cfg).items()}, str(tmp_path / "model.safetensors"))
    m = LlamaForCausalLM.from_pretrained(str(tmp_path), weight_format="fp8_e4m3", max_cache_len=64)
    assert m.weight_format == "fp8_e4m3" and m.precise


def test_footprint_at_13b_dims(monkeypatch):
    """FP8: decode_tiles = one byte per projection weight in exactly ONE layout (o / down: the 20-row tiles, no 16-row copy) + one fp32
    scale per row + the 16-bit lm_head tiles; weights and KV cache unchanged. Default mode: the figures
    test_llm_mode_selection_and_memory_footprint pins, unchanged."""
    from seedx_amd.llama import LlamaForCausalLM
    monkeypatch.delenv("SX_LLM_WEIGHTS", raising=False)
    monkeypatch.delenv("SX_LLM_PRECISE", raising=False)
    monkeypatch.delenv("SX_GEMV_BAL20", raising=False)
    cfg = dict(weights.FULL_LLM)
    H, I, L = 5120, 13824, 40
    d = LlamaForCausalLM(dict(cfg), max_cache_len=1024, max_batch=16)
    q = LlamaForCausalLM(dict(cfg), max_cache_len=1024, max_batch=16, weight_format="fp8_e4m3")
    fd, fq = d.memory_footprint(), q.memory_footprint()
    per_layer = (3 * H * H + H * H + 2 * I * H + H * I) * 2
    assert fd["weights"] == L * per_layer + (32330 + d.V_l) * H * 2 and fd["decode_tiles"] == L * per_layer + d.V_l * H * 2
    assert fd["kv_cache"] == L * 16 * 40 * 1024 * 128 * 8 and fd["total"] == fd["weights"] + fd["decode_tiles"] + fd["kv_cache"]
    # layouts held per layer: wqkv [3H/16][H/64][16][64], wo [H/20][H/64][20][64], wgu [2I/16][H/64][16][64], wd [H/20][I/64][20][64]
    assert q._bal20(H) and not q._bal20(3 * H)
    tile_bytes = (3 * H // 16) * (H // 64) * 16 * 64 + (H // 20) * (H // 64) * 20 * 64 + (2 * I // 16) * (H // 64) * 16 * 64 \
        + (H // 20) * (I // 64) * 20 * 64
    scale_bytes = (3 * H + H + 2 * I + H) * 4
    assert fq["decode_tiles"] == L * (tile_bytes + scale_bytes) + q.V_l * H * 2
    assert fq["weights"] == fd["weights"] and fq["kv_cache"] == fd["kv_cache"]
    assert fq["total"] == fq["weights"] + fq["decode_tiles"] + fq["kv_cache"]
    saved = fd["decode_tiles"] - fq["decode_tiles"]
    assert saved == L * (per_layer // 2 - scale_bytes) and 12.6e9 < saved < 12.8e9           # 25.7 → 13.0 GB of tiles per step
