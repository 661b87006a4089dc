"""Host side of the MXFP4 (e2m1, block-32 E8M0 scale) decode mode: the codec (seedx_amd/quant.py) against a table of the sixteen e2m1
values, exactness of the dequantised values in fp16 and bf16 at both ends of the exponent clamp, idempotence, the error on Gaussian rows,
the MXFP4 code and scale tile layouts against the index map of include/seedx_hip.h, GLU packing and tensor-parallel consistency, mode
selection, memory_footprint(), and the dispatch plan of an MXFP4 launch (sx_gemv_plan) against that of its 16-bit and FP8 twins. No GPU."""
import pytest
import torch

from oracle import weights
from tests import test_gemv_matrix_gpu as gv

MAGS = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
# (N, K, glu, residual, layout): the shapes of tests/test_fp8_weights_gpu.py
SHAPES = [(1536, 512, False, False, "t"), (5120, 1024, False, True, "t20"), (5120, 5120, False, True, "t"), (2816, 512, True, False, "t"),
          (640, 13824, False, True, "t"), (15360, 512, False, False, "t"), (27648, 256, True, False, "t")]


def _nearest_e2m1(v):
    """The nearest e2m1 magnitude code of every |v| (clamped to 6), ties to the even code — by exhaustive comparison in float64."""
    a = v.double().abs().clamp(max=6.0)
    mags = torch.tensor(MAGS, dtype=torch.float64)
    d = (a[:, None] - mags[None, :]).abs()
    best = d.min(dim=1).values
    hit = d == best[:, None]                                   # one or (exact tie) two neighbouring codes
    codes = torch.arange(8)[None, :].expand_as(hit)
    even = hit & (codes % 2 == 0)
    pick = torch.where(hit.sum(1) == 2, even.float().argmax(1), hit.float().argmax(1))
    return pick.to(torch.uint8) | (torch.signbit(v).to(torch.uint8) << 3)


def test_codec_against_a_table_for_every_fp16_value_of_one_block_range():
    """Every fp16 value of magnitude <= 8 (the whole range a block with e = 0 can hold, past the clamp at 6; both signs, -0, subnormals):
    nearest e2m1, ties to even, clamp at 6, the sign kept."""
    from seedx_amd import quant
    v = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.float16)
    v = v[torch.isfinite(v) & (v.abs() <= 8)]
    assert v.numel() == 2 * (0x4800 + 1)
    got = quant.encode_e2m1(v.float())
    assert got.dtype == torch.uint8 and int(got.max()) == 15
    assert torch.equal(got, _nearest_e2m1(v))
    ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 7.0, 100.0, -0.0, -5.0, -0.25])
    assert quant.encode_e2m1(ties).tolist() == [0, 2, 2, 4, 4, 6, 6, 7, 7, 8, 14, 8]


def test_decode_table_all_sixteen_codes():
    from seedx_amd import quant
    tab = quant.decode_table_e2m1()
    assert tab.dtype == torch.float32 and tab.tolist() == MAGS + [-m for m in MAGS]
    assert torch.signbit(tab[8])                                                   # code 8 is -0
    codes = (torch.arange(16, dtype=torch.uint8)[:, None] | (torch.arange(16, dtype=torch.uint8)[None, :] << 4)).reshape(8, 32)
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        got = quant.dequantize_blocks_mxfp4(codes, torch.full((8, 2), 127, dtype=torch.uint8), dt)
        assert got.dtype == dt and got.shape == (8, 64)
        assert torch.equal(got.float().reshape(-1, 2), torch.stack([tab[(codes & 15).long()], tab[(codes >> 4).long()]], -1).reshape(-1, 2))


def _rows_spanning_the_clamp_range(dt):
    g = torch.Generator().manual_seed(3)
    K = 192
    amax = [1e-6, 3e4, 65504.0, 6.0 * 2.0 ** 13, 2.0 ** -14, 5.9, 6.1, 4.0, 3.99, 1.0, 0.02, 1e-3]
    blocks = []
    for a in amax:                      # every 32-k block of a row scaled to its own amax: rows mix exponents
        r = torch.randn(K, generator=g)
        blocks.append(r / r.abs().max() * a)
    rows = torch.stack(blocks)
    def blk(a):
        b = torch.randn(32, generator=g)
        return b / b.abs().max() * a
    mixed = torch.cat([blk(1e-6), blk(65504.0), torch.zeros(32), blk(1.0), blk(1.0), blk(1.0)])   # e = -13 | 13 | all-zero block | -2
    rows = torch.cat([rows, mixed[None, :]])
    return rows.clamp(-65504.0, 65504.0).to(dt)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_random_rows_exact_idempotent_and_normal(dt):
    from seedx_amd import quant
    w = _rows_spanning_the_clamp_range(dt)
    codes, scale = quant.quantize_blocks_mxfp4(w)
    N, K = w.shape
    assert codes.dtype == scale.dtype == torch.uint8 and codes.shape == (N, K // 2) and scale.shape == (N, K // 32)
    e = scale.int() - 127
    assert e.min() == -13 and e.max() == 13 and torch.equal(e, quant.block_exponents(w))
    # blocks of amax 1e-6 sit at the lower clamp end; amax 3e4 gives floor(log2) - 2 = 12, the upper end 13 takes amax >= 2^15 (rows 2, 3)
    assert (e[0] == -13).all() and e[1].max() == 12 and e[2].max() == 13 and e[3].max() == 13
    assert e[-1].tolist() == [-13, 13, 0, -2, -2, -2] and not codes[-1, 32:48].any()  # the all-zero block: e = 0, codes 0
    x = quant.dequantize_blocks_mxfp4(codes, scale, torch.float32)
    for d2 in (torch.float16, torch.bfloat16):                                      # exact in BOTH 16-bit types
        assert torch.equal(x.to(d2).float(), x)
    nz = x[x != 0].abs()
    assert nz.min() >= 2.0 ** -14 and nz.max() <= 6.0 * 2.0 ** 13                   # all normal fp16 numbers
    # idempotent: the dequantised model quantises to itself — same codes (up to the sign of a zero), same values; the scale byte too, except
    # where a whole block flushed to zero (amax 1e-6 at e = -13): that block now IS an all-zero block, e = 0
    c2, s2 = quant.quantize_blocks_mxfp4(quant.dequantize_blocks_mxfp4(codes, scale, dt))
    flushed = x.view(N, K // 32, 32).abs().amax(-1) == 0
    assert flushed[0].all() and torch.equal(c2, codes) and torch.equal(s2[~flushed], scale[~flushed]) and (s2[flushed] == 127).all()
    assert torch.equal(quant.dequantize_blocks_mxfp4(c2, s2, torch.float32), x)
    # inside the clamp the block maximum lands in e2m1's top binade and every value is within half a quantum of the top binade (2^e)
    inside = (e > -13) & (e < 13) & (w.float().abs().view(N, K // 32, 32).amax(-1) > 0)
    top = x.abs().view(N, K // 32, 32).amax(-1) / torch.pow(2.0, e.float())
    assert (top[inside] >= 4).all() and (top[inside] <= 6).all()
    err = (x - w.float()).abs().view(N, K // 32, 32) / torch.pow(2.0, e.float())[..., None]
    small = (w.float().abs().view(N, K // 32, 32) <= 6 * torch.pow(2.0, e.float())[..., None])
    assert err[inside[..., None] & small].max() <= 1.0


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_quantisation_error_on_gaussian_rows(dt):
    """N(0, 0.02^2), 256 x 5120: the figure the mode costs per projection (0.114 relative rms, fp16 and bf16)."""
    from seedx_amd import quant
    w = (torch.randn(256, 5120, generator=torch.Generator().manual_seed(0)) * 0.02).to(dt)
    codes, scale = quant.quantize_blocks_mxfp4(w)
    e = ((quant.dequantize_blocks_mxfp4(codes, scale) - w.float()).norm() / w.float().norm()).item()
    print(f"MXFP4 relative rms error on Gaussian rows, {dt}: {e:.4f}")
    assert 0.10 <= e <= 0.13, e


def _k_of_nibble(t, p, hi):
    """include/seedx_hip.h: byte p = 8 g + 4 h + i of k-slab t holds k = 64 t + 32 h + 8 g + 2 i in its low nibble, k + 1 in the high."""
    g, h, i = p // 8, (p // 4) % 2, p % 4
    return 64 * t + 32 * h + 8 * g + 2 * i + hi


@pytest.mark.parametrize("rows", [16, 20])
def test_pack_functions_round_trip_through_the_stated_index_map(rows):
    from seedx_amd import ops
    N, K = 4 * rows * 2, 192
    g = torch.Generator().manual_seed(1)
    nib = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8)
    codes = nib[:, 0::2] | (nib[:, 1::2] << 4)
    t = (ops.pack_decode_tiles_fp4 if rows == 16 else ops.pack_decode_tiles20_fp4)(codes)
    assert t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == (N // rows, K // 64, rows, 32)
    back = torch.empty_like(nib)
    for hi in (0, 1):
        kmap = torch.tensor([[_k_of_nibble(s, p, hi) for p in range(32)] for s in range(K // 64)])
        for grp in range(N // rows):
            for s in range(K // 64):
                back[grp * rows:(grp + 1) * rows, kmap[s]] = (t[grp, s] >> (4 * hi)) & 15
    assert torch.equal(back, nib)
    # a lane's 8 bytes: row r, lane group g → dword h = its eight k-slots of 32-k half h, nibble j = slot j, all inside block 2 s + h
    r, gq, s = 5, 2, 1
    lane = t[1, s, r, 8 * gq:8 * gq + 8]
    for h in (0, 1):
        slots = torch.stack([lane[4 * h:4 * h + 4] & 15, lane[4 * h:4 * h + 4] >> 4], -1).reshape(-1)
        k0 = 64 * s + 32 * h + 8 * gq
        assert torch.equal(slots, nib[rows + r, k0:k0 + 8]) and k0 // 32 == (k0 + 7) // 32 == 2 * s + h
    if rows == 20:                                   # rows 16..19 sit behind the 512-B tile of rows 0..15
        flat = t[1, s].reshape(-1)
        assert torch.equal(flat[512 + 32 * 2:512 + 32 * 3], t[1, s, 18])
    # scale tiles [N/rows][K/64][rows][2]: byte h of (row, k-step s) = the scale of block 2 s + h
    scale = torch.randint(114, 141, (N, K // 32), generator=g, dtype=torch.uint8)
    st = ops.pack_block_scales_fp4(scale, rows=rows)
    assert st.dtype == torch.uint8 and st.is_contiguous() and tuple(st.shape) == (N // rows, K // 64, rows, 2)
    for grp in range(N // rows):
        for s in range(K // 64):
            assert torch.equal(st[grp, s], scale[grp * rows:(grp + 1) * rows, 2 * s:2 * s + 2])
    if rows == 20:
        assert torch.equal(st[1, 1].reshape(-1)[32 + 2 * 2:32 + 2 * 3], scale[20 + 18, 2:4])


def test_glu_packed_codes_and_scales_follow_their_rows():
    from seedx_amd import quant
    from seedx_amd.llama import glu_pack_rows
    g = torch.Generator().manual_seed(2)
    I, K = 64, 128
    up = (torch.randn(I, K, generator=g) * torch.logspace(-3, 1, I)[:, None]).half()
    gate = (torch.randn(I, K, generator=g) * torch.logspace(1, -3, I)[:, None]).half()
    (cu, su), (cg, sg) = quant.quantize_blocks_mxfp4(up), quant.quantize_blocks_mxfp4(gate)
    codes, scale = glu_pack_rows(cu, cg), glu_pack_rows(su, sg)
    assert su.unique().numel() > 4 and scale.shape == (2 * I, K // 32)
    want = glu_pack_rows(quant.dequantize_blocks_mxfp4(cu, su), quant.dequantize_blocks_mxfp4(cg, sg))
    assert torch.equal(quant.dequantize_blocks_mxfp4(codes, scale), want)
    c2, s2 = quant.quantize_blocks_mxfp4(glu_pack_rows(up, gate))                  # packing first, quantising second: the same rows
    assert torch.equal(c2, codes) and torch.equal(s2, scale)


def test_tp_slices_of_one_quantised_model():
    """tp = 2, miniature geometry (FFN 768: 384 per rank, a whole number of 64-k steps): quantise the full matrices, then slice — codes and
    block scales of every projection dequantise to the llama_tp_shard slices of the dequantised model, and the ranks' slices put together
    are the whole. The miniature FFN of 704 (352 per rank) would cut a k-step of down_proj: refused."""
    from seedx_amd import quant
    from seedx_amd.parallel import llama_tp_shard
    cfg = dict(weights.MINI_LLM, num_hidden_layers=1, intermediate_size=768)
    nh, hd = cfg["num_attention_heads"], cfg["hidden_size"] // cfg["num_attention_heads"]
    sd = weights.llama_sd(cfg)
    p = "model.layers.0."
    sd_q, codes, scales = quant.quantize_llama_state_dict(sd, cfg, torch.float16, weight_format="mxfp4")
    assert sorted(codes) == sorted(scales) == sorted(p + n + ".weight" for n in quant.LLAMA_PROJECTIONS)
    for k in ("model.embed_tokens.weight", "lm_head.weight", "model.norm.weight", p + "input_layernorm.weight"):
        assert sd_q[k] is sd[k]
    for k in codes:
        assert codes[k].shape == (sd[k].shape[0], sd[k].shape[1] // 2) and scales[k].shape == (sd[k].shape[0], sd[k].shape[1] // 32)
        assert torch.equal(quant.dequantize_blocks_mxfp4(codes[k], scales[k]), sd_q[k].float())
        assert not torch.equal(sd_q[k].float(), sd[k].half().float())             # lossy: the model really changed
    names = {"q": "self_attn.q_proj", "k": "self_attn.k_proj", "v": "self_attn.v_proj", "o": "self_attn.o_proj",
             "gate": "mlp.gate_proj", "up": "mlp.up_proj", "down": "mlp.down_proj"}
    whole = {}
    for rank in range(2):
        w = llama_tp_shard(sd_q, p, rank, 2, nh, hd)
        c, s = quant.llama_tp_shard_mxfp4(codes, scales, p, rank, 2, nh, hd)
        for k in names:
            assert c[k].shape == (w[k].shape[0], w[k].shape[1] // 2) and s[k].shape == (w[k].shape[0], w[k].shape[1] // 32)
            assert torch.equal(quant.dequantize_blocks_mxfp4(c[k].contiguous(), s[k].contiguous()), w[k].float()), (rank, k)
            whole.setdefault(k, []).append((c[k], s[k]))
    for k, name in names.items():
        dim = 1 if k in ("o", "down") else 0
        assert torch.equal(torch.cat([c for c, _ in whole[k]], dim=dim), codes[p + name + ".weight"])
        assert torch.equal(torch.cat([s for _, s in whole[k]], dim=dim), scales[p + name + ".weight"])
    cfg704 = dict(weights.MINI_LLM, num_hidden_layers=1)
    _, c704, s704 = quant.quantize_llama_state_dict(weights.llama_sd(cfg704), cfg704, torch.float16, weight_format="mxfp4")
    with pytest.raises(ValueError, match="multiple of 64"):
        quant.llama_tp_shard_mxfp4(c704, s704, p, 0, 2, nh, hd)
    with pytest.raises(AssertionError, match="multiple of 64"):
        quant.quantize_blocks_mxfp4(torch.zeros(16, 96))


def test_mode_selection(monkeypatch):
    from seedx_amd.llama import LlamaForCausalLM
    cfg = dict(weights.MINI_LLM)
    monkeypatch.delenv("SX_LLM_WEIGHTS", raising=False)
    monkeypatch.delenv("SX_LLM_PRECISE", raising=False)
    monkeypatch.delenv("SX_LLM_KV", raising=False)
    assert LlamaForCausalLM(dict(cfg), max_cache_len=64).weight_format is None
    m = LlamaForCausalLM(dict(cfg), max_cache_len=64, max_batch=4, weight_format="mxfp4")
    assert m.weight_format == "mxfp4" and m.precise and m.weight_quant_report is None
    m = LlamaForCausalLM(dict(cfg), max_cache_len=64, max_batch=4, weight_format="mxfp4", kv_format="fp8_e4m3")
    assert m.weight_format == "mxfp4" and m.kv_format == "fp8_e4m3"
    with pytest.raises(ValueError, match="precise"):
        LlamaForCausalLM(dict(cfg), max_cache_len=64, weight_format="mxfp4", precise=False)
    with pytest.raises(ValueError, match="weight_format"):
        LlamaForCausalLM(dict(cfg), max_cache_len=64, weight_format="int4")
    with pytest.raises(ValueError, match="skinny GEMM"):                       # FFN width 176 per rank is no multiple of 64: no tiled decode path
        LlamaForCausalLM(dict(cfg, intermediate_size=176), max_cache_len=64, weight_format="mxfp4")
    monkeypatch.setenv("SX_LLM_WEIGHTS", "mxfp4")                               # the A/B switch
    assert LlamaForCausalLM(dict(cfg), max_cache_len=64).weight_format == "mxfp4"
    with pytest.raises(ValueError, match="precise"):
        LlamaForCausalLM(dict(cfg), max_cache_len=64, precise=False)
    monkeypatch.setenv("SX_LLM_PRECISE", "0")
    with pytest.raises(ValueError, match="precise"):
        LlamaForCausalLM(dict(cfg), max_cache_len=64)
    monkeypatch.setenv("SX_LLM_WEIGHTS", "int4")
    with pytest.raises(ValueError, match="weight_format"):
        LlamaForCausalLM(dict(cfg), max_cache_len=64, precise=True)


def test_from_pretrained_carries_the_keyword(tmp_path):
    import json
    from safetensors.torch import save_file
    from seedx_amd.llama import LlamaForCausalLM
    cfg = dict(weights.MINI_LLM, num_hidden_layers=1)
    json.dump(cfg, open(tmp_path / "config.json", "w"))
    save_file({k: v.contiguous() for k, v in weights.llama_sd(cfg).items()}, str(tmp_path / "model.safetensors"))
    m = LlamaForCausalLM.from_pretrained(str(tmp_path), weight_format="mxfp4", max_cache_len=64)
    assert m.weight_format == "mxfp4" and m.precise


def test_footprint_at_13b_dims(monkeypatch):
    """MXFP4: decode_tiles = L (sum N K / 2 + sum N K / 32) + the 16-bit lm_head tiles, one layout per projection; weights and KV cache
    unchanged. Default mode: the figures test_llm_mode_selection_and_memory_footprint pins, unchanged."""
    from seedx_amd.llama import LlamaForCausalLM
    for v in ("SX_LLM_WEIGHTS", "SX_LLM_PRECISE", "SX_GEMV_BAL20", "SX_LLM_KV"):
        monkeypatch.delenv(v, raising=False)
    cfg = dict(weights.FULL_LLM)
    H, I, L = 5120, 13824, 40
    d = LlamaForCausalLM(dict(cfg), max_cache_len=1024, max_batch=16)
    q = LlamaForCausalLM(dict(cfg), max_cache_len=1024, max_batch=16, weight_format="mxfp4")
    fd, fq = d.memory_footprint(), q.memory_footprint()
    per_layer = (3 * H * H + H * H + 2 * I * H + H * I) * 2
    assert fd["weights"] == L * per_layer + (32330 + d.V_l) * H * 2 and fd["decode_tiles"] == L * per_layer + d.V_l * H * 2
    assert fd["kv_cache"] == L * 16 * 40 * 1024 * 128 * 8 and fd["total"] == fd["weights"] + fd["decode_tiles"] + fd["kv_cache"]
    nk = 3 * H * H + H * H + 2 * I * H + H * I
    assert fq["decode_tiles"] == L * (nk // 2 + nk // 32) + q.V_l * H * 2
    # the layouts held per layer: wqkv [3H/16][H/64][16][32], wo [H/20][H/64][20][32], wgu [2I/16][H/64][16][32], wd [H/20][I/64][20][32]
    assert q._bal20(H) and not q._bal20(3 * H)
    tile_bytes = (3 * H // 16) * (H // 64) * 16 * 32 + (H // 20) * (H // 64) * 20 * 32 + (2 * I // 16) * (H // 64) * 16 * 32 \
        + (H // 20) * (I // 64) * 20 * 32
    scale_bytes = (3 * H // 16) * (H // 64) * 16 * 2 + (H // 20) * (H // 64) * 20 * 2 + (2 * I // 16) * (H // 64) * 16 * 2 \
        + (H // 20) * (I // 64) * 20 * 2
    assert fq["decode_tiles"] == L * (tile_bytes + scale_bytes) + q.V_l * H * 2
    assert fq["weights"] == fd["weights"] and fq["kv_cache"] == fd["kv_cache"]
    assert fq["total"] == fq["weights"] + fq["decode_tiles"] + fq["kv_cache"]
    assert 6.6e9 < fq["decode_tiles"] - q.V_l * H * 2 < 6.9e9                          # 25.4 → 6.7 GB of projection tiles per step
    k = LlamaForCausalLM(dict(cfg), max_cache_len=1024, max_batch=16, weight_format="mxfp4", kv_format="fp8_e4m3").memory_footprint()
    assert k["decode_tiles"] == fq["decode_tiles"] and k["kv_cache"] == L * 16 * 40 * 1024 * (2 * 128 + 8)


# ---- MXFP4 launches share sx_gemv's one dispatch plan ------------------------------------------------------------------------------
def _case(N, K, glu, layout, M, planes, emit_norm=False, **kw):
    return gv.case("", "f16", M=M, N=N, K=K, glu=glu, w_layout=2 if layout == "t20" else 1, x_layout=1 if planes == 2 else 0, planes=planes,
                   out="f32", emit=emit_norm, **kw)


def test_fp4_grid_rule_agrees_with_ssq_parts_and_the_16bit_dispatch():
    """Through sx_gemv_plan (host only, nothing launched): on the seven shapes of the GPU tests and every (M, planes) they use, the
    MXFP4 launch has the workgroup count sx_gemv_ssq_parts reports wherever the RMSNorm fold asks for it, and the 16-bit, FP8 and MXFP4
    launches have one plan — path, grid, split factor and kernel family — which is the hand-written plan_of's."""
    from seedx_amd import _lib
    lib = _lib.load()
    formats = (0, _lib.SX_FP8_E4M3, _lib.SX_FP4_E2M1)

    def plan(c, ws):
        """The one plan of the three weight formats (asserted equal to each other and to plan_of), without the format field."""
        got = [gv.lib_plan(lib, gv.plan_args(c, ws, w_dtype=f)) for f in formats]
        assert all(g is not None for g in got), lib.sx_last_error().decode()
        assert [g[7] for g in got] == list(formats)
        assert got[0][:7] == got[1][:7] == got[2][:7] == gv.plan_of(c, ws) and got[2][0] == 1, (c, ws, got, gv.plan_of(c, ws))
        return list(got[2][1:7])

    seen = set()
    for N, K, glu, res, layout in SHAPES:
        ws = 16384 + 8 * 32 * N * 4
        for M, planes in [(1, 2), (11, 2), (16, 2), (21, 2), (32, 2), (8, 1), (24, 1)]:
            got = plan(_case(N, K, glu, layout, M, planes), ws)
            seen.add(tuple(got[2:]))
            if not glu:           # the fold's producer form (x16_out): never 64-row workgroups, parts as the library reports them
                fold = plan(_case(N, K, glu, layout, M, planes, emit_norm=True), ws)
                assert fold[0] == lib.sx_gemv_ssq_parts(N, 0, 2 if layout == "t20" else 1), (N, layout, fold)
            elif got[2] != 4:
                assert got[0] == lib.sx_gemv_ssq_parts(N, 1, 1)
        assert plan(_case(N, K, glu, layout, 16, 2), 0)[1] == 1                     # no workspace: never split
    assert plan(_case(640, 13824, False, "t", 16, 2), 16384 + 8 * 32 * 640 * 4)[1] == 8     # the split-K shape splits
    assert len(seen) == 12, seen                        # every family of the default tuning (the other two are lab variants)
    # the query takes every format, and refusals reach it too: a 16-bit w_dtype without w_block_scale is accepted and reports format 0,
    # SX_FP4_E2M1 without its block scales is refused
    a = gv.plan_args(gv.case("", "f16", M=8, N=64, K=512, w_layout=1))
    got = gv.lib_plan(lib, a)
    assert got is not None and got[0] == 1 and got[7] == 0, lib.sx_last_error().decode()
    a.w_dtype = _lib.SX_FP4_E2M1
    assert gv.lib_plan(lib, a) is None and "w_block_scale" in lib.sx_last_error().decode()
