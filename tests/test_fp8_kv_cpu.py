"""Host side of the FP8 (e4m3) KV cache (LlamaForCausalLM(kv_format="fp8_e4m3")): the row codec quant.quantize_kv_rows /
dequantize_kv_rows — one power-of-two scale per (token, head) row of 128 values, exponent clamp [-64, 64] — its error bound, value
idempotence and boundary rows; mode selection and refusals; memory_footprint(). No GPU."""
import pytest
import torch

from oracle import weights

D = 128


def _relerr(x, ref):
    return ((x.double() - ref.double()).norm() / ref.double().norm()).item()


def _rows(kind, n=512, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, D, generator=g)
    if kind == "tiny":
        return x * 1e-6
    if kind == "huge":
        return x * 1e9
    if kind == "heavy":
        return x * torch.exp(3 * torch.randn(n, D, generator=g))
    return x


def _check_rule(x):
    """Element-wise |x^ - x| <= 2^-4 |x| + 2^-10 scale (half a quantum of a normal code: 2^-4 of the value's binade; of the subnormal
    range: half of 2^-9 · scale), no NaN code, |code value| <= 448."""
    from seedx_amd import quant
    codes, scale = quant.quantize_kv_rows(x)
    assert codes.dtype == torch.uint8 and codes.shape == x.shape and scale.dtype == torch.float32 and scale.shape == x.shape[:-1]
    assert ((codes & 0x7f) != 0x7f).all()
    val = quant.decode_table()[codes.long()]
    assert val.abs().max() <= 448
    s = torch.log2(scale)
    assert torch.equal(s, s.round()) and s.min() >= -64 and s.max() <= 64                       # powers of two inside the clamp
    xh = quant.dequantize_kv_rows(codes, scale)
    assert torch.equal(xh, val * scale[..., None])
    bound = x.double().abs() * 2.0 ** -4 + scale.double()[..., None] * 2.0 ** -10
    assert ((xh.double() - x.double()).abs() <= bound).all()
    return codes, scale, xh


@pytest.mark.parametrize("kind", ["normal", "tiny", "huge", "heavy"])
def test_codec_rule(kind):
    from seedx_amd import quant
    x = _rows(kind)
    codes, scale, xh = _check_rule(x)
    # the scale is the smallest power of two that brings the row's amax inside +-448 (no clamp binds on these rows)
    amax = x.abs().amax(dim=-1).double()
    assert (amax <= 448 * scale.double()).all() and (amax > 224 * scale.double()).all()
    if kind == "normal":
        e = _relerr(xh, x)
        print(f"FP8 KV codec, N(0,1) rows of 128: relative Frobenius error {e:.4f}")
        assert e < 0.064            # 2^-4 per normal value + the subnormal tail (< 1e-3 of the row norm): test_fp8_weights_gpu.py's bound
    # VALUE idempotence (code idempotence does not hold: a rounded amax can cross the 1.75 boundary and change s for the same values)
    c2, s2 = quant.quantize_kv_rows(xh)
    assert torch.equal(quant.dequantize_kv_rows(c2, s2), xh)
    # leading dims are free: [G, H, T, D] rows give what the flat rows give
    c4, s4 = quant.quantize_kv_rows(x.view(4, 2, -1, D))
    assert torch.equal(c4.view(-1, D), codes) and torch.equal(s4.view(-1), scale)


def test_zero_row_and_boundary_rows():
    from seedx_amd import quant
    z = torch.zeros(3, D)
    z[1, 5] = -0.0
    codes, scale = quant.quantize_kv_rows(z)
    assert torch.equal(scale, torch.ones(3)) and torch.equal(codes & 0x7f, torch.zeros_like(codes)) and codes[1, 5] == 0x80
    assert torch.equal(quant.dequantize_kv_rows(codes, scale), z)
    # amax exactly 448 · 2^s keeps s (code 0x7e = 448); one ulp above takes s + 1 (and rounds to 224 · 2^(s+1) = the same value)
    for s in (-64, -20, -9, 0, 3, 40, 63):
        on = torch.full((1, D), 0.25 * 2.0 ** s)
        on[0, 7] = -448 * 2.0 ** s
        above = on.clone()
        above[0, 7] = torch.nextafter(on[0, 7], torch.tensor(-float("inf")))
        c0, s0 = quant.quantize_kv_rows(on)
        c1, s1 = quant.quantize_kv_rows(above)
        assert s0.item() == 2.0 ** s and c0[0, 7] == 0xfe and s1.item() == 2.0 ** (s + 1) and c1[0, 7] == 0xf6     # -448, -224
        _check_rule(on)
        _check_rule(above)
    # the clamp: rows below 448 · 2^-64 keep s = -64 (codes shrink towards the subnormals), rows above 448 · 2^64 saturate at +-448
    lo = torch.full((1, D), 2.0 ** -70)
    c, sc = quant.quantize_kv_rows(lo)
    assert sc.item() == 2.0 ** -64 and torch.equal(quant.dequantize_kv_rows(c, sc), lo)            # 2^-6 · 2^-64: exact
    hi = torch.full((1, D), 2.0 ** 80)
    c, sc = quant.quantize_kv_rows(hi)
    assert sc.item() == 2.0 ** 64 and (c == 0x7e).all()
    # the weights' rule is untouched by the optional bounds
    w = torch.randn(8, 64) * 1e-4
    assert torch.equal(quant.row_exponents(w), quant.row_exponents(w, quant.S_MIN, quant.S_MAX)) and quant.row_exponents(w).min() >= -15
    assert quant.row_exponents(w, -64, 64).max() < -15


def test_mode_selection_and_refusals(monkeypatch):
    from seedx_amd.llama import LlamaForCausalLM
    cfg = dict(weights.MINI_LLM)                                               # head_dim 128
    for k in ("SX_LLM_KV", "SX_LLM_WEIGHTS", "SX_LLM_PRECISE", "SX_LLM_V16"):
        monkeypatch.delenv(k, raising=False)
    assert LlamaForCausalLM(dict(cfg), max_cache_len=64).kv_format is None
    for fmt in ("fp8_e4m3", "fp8_e4m3_emulated"):
        m = LlamaForCausalLM(dict(cfg), max_cache_len=64, max_batch=4, kv_format=fmt)
        assert m.kv_format == fmt and m.precise and not m.kv_v16 and m.weight_format is None
        assert LlamaForCausalLM(dict(cfg), max_cache_len=64, kv_format=fmt, kv_v16=False).kv_format == fmt
        with pytest.raises(ValueError, match="precise"):
            LlamaForCausalLM(dict(cfg), max_cache_len=64, kv_format=fmt, precise=False)
        with pytest.raises(ValueError, match="head_dim 128"):
            LlamaForCausalLM(dict(cfg, num_attention_heads=4), max_cache_len=64, kv_format=fmt)
        with pytest.raises(ValueError, match="kv_v16"):
            LlamaForCausalLM(dict(cfg), max_cache_len=64, kv_format=fmt, kv_v16=True)
    with pytest.raises(ValueError, match="kv_format"):
        LlamaForCausalLM(dict(cfg), max_cache_len=64, kv_format="int8")
    # independent of the FP8 weight tiles
    m = LlamaForCausalLM(dict(cfg), max_cache_len=64, max_batch=4, kv_format="fp8_e4m3", weight_format="fp8_e4m3")
    assert m.kv_format == "fp8_e4m3" and m.weight_format == "fp8_e4m3"
    # tensor-parallel ranks: a follow-up

    class TwoRanks:
        world, rank, graph_safe = 2, 0, True
    with pytest.raises(NotImplementedError, match="kv_format is single-rank"):
        LlamaForCausalLM(dict(cfg, num_attention_heads=2), max_cache_len=64, comm=TwoRanks(), kv_format="fp8_e4m3")
    monkeypatch.setenv("SX_LLM_KV", "fp8_e4m3")                                 # the A/B switch
    assert LlamaForCausalLM(dict(cfg), max_cache_len=64).kv_format == "fp8_e4m3"
    assert LlamaForCausalLM(dict(cfg), max_cache_len=64, kv_format="fp8_e4m3_emulated").kv_format == "fp8_e4m3_emulated"   # the keyword wins
    with pytest.raises(ValueError, match="precise"):
        LlamaForCausalLM(dict(cfg), max_cache_len=64, precise=False)
    monkeypatch.setenv("SX_LLM_KV", "fp4")
    with pytest.raises(ValueError, match="kv_format"):
        LlamaForCausalLM(dict(cfg), max_cache_len=64)


def test_from_pretrained_carries_the_keyword(tmp_path, monkeypatch):
    import json
    from safetensors.torch import save_file
    from seedx_amd.llama import LlamaForCausalLM
    monkeypatch.delenv("SX_LLM_KV", raising=False)
    cfg = dict(weights.MINI_LLM, num_hidden_layers=1)
    json.dump(cfg, open(tmp_path / "config.json", "w"))
    save_file({k: v.contiguous() for k, v in weights.llama_sd(cfg).items()}, str(tmp_path / "model.safetensors"))
    m = LlamaForCausalLM.from_pretrained(str(tmp_path), kv_format="fp8_e4m3", max_cache_len=64)
    assert m.kv_format == "fp8_e4m3" and m.precise
    assert LlamaForCausalLM.from_pretrained(str(tmp_path), max_cache_len=64).kv_format is None


def test_footprint_at_13b_dims(monkeypatch):
    """kv_cache = L·G·heads·Tmax·(2·128 + 8) B: one byte per k and per v value + two fp32 row scales, 0.344 of the mixed cache's 768 B per
    (layer, head, token); the emulated twin holds (and reports) the all-fp32 cache; weights and decode tiles are untouched."""
    from seedx_amd.llama import LlamaForCausalLM
    for k in ("SX_LLM_KV", "SX_LLM_WEIGHTS", "SX_LLM_PRECISE"):
        monkeypatch.delenv(k, raising=False)
    cfg = dict(weights.FULL_LLM)
    mk = lambda **kw: LlamaForCausalLM(dict(cfg), max_cache_len=1024, max_batch=16, **kw)
    d, q, e = mk(), mk(kv_format="fp8_e4m3"), mk(kv_format="fp8_e4m3_emulated")
    fd, fq, fe = d.memory_footprint(), q.memory_footprint(), e.memory_footprint()
    assert fq["kv_cache"] == 40 * 16 * 40 * 1024 * 264
    assert fe["kv_cache"] == 40 * 16 * 40 * 1024 * 128 * 8 == fd["kv_cache"]      # (the constructor's default figure is the all-fp32 cache too)
    for f in (fq, fe):
        assert f["weights"] == fd["weights"] and f["decode_tiles"] == fd["decode_tiles"]
        assert f["total"] == f["weights"] + f["decode_tiles"] + f["kv_cache"]
    assert abs(fq["kv_cache"] / (40 * 16 * 40 * 1024 * 768) - 0.344) < 5e-4
    both = mk(kv_format="fp8_e4m3", weight_format="fp8_e4m3").memory_footprint()
    assert both["kv_cache"] == fq["kv_cache"] and both["decode_tiles"] < fd["decode_tiles"]
