"""Weight-only FP8 (OCP e4m3fn) codec of the LLM decode step: one power-of-two scale per output row.

Per row n of a 16-bit weight W[N, K]:  s[n] = clamp(ceil(log2(max|W[n, :]| / 448)), -15, 7)  (0 for an all-zero row),
code = e4m3fn(rne(clamp(W · 2^-s, -448, 448))),  scale[n] = 2^s[n]  (fp32).  The NaN codes 0x7f / 0xff are never produced.
Every code · 2^s with s in [-15, 7] is exactly representable in fp16 AND bf16 (smallest: 2^-9 · 2^-15 = 2^-24, the smallest fp16
subnormal; largest: 448 · 2^7 < 65504; three mantissa bits), so the dequantised 16-bit matrix IS the quantised model: prefill runs
the ordinary GEMMs on it, the decode step streams the codes (sx_gemv w_dtype = SX_FP8_E4M3) and computes the same bits.

MXFP4 (OCP microscaling e2m1, weight_format="mxfp4"): a block is 32 consecutive k of one row of W[N, K] (K % 64 == 0), with one
power-of-two scale per block:  e = clamp(floor(log2(amax_block)) - 2, -13, 13)  (0 for an all-zero block; the OCP MX rule: the block
maximum lands in e2m1's top binade [4, 8) and clips at 6), stored as the E8M0 byte e + 127 (the fp32 scale is byte << 23);
code = e2m1(rne(clamp(|w| · 2^-e, 0, 6))) with the sign from signbit, magnitudes {0, .5, 1, 1.5, 2, 3, 4, 6}; two codes share a byte,
the even k in the low nibble. Every code · 2^e with e in [-13, 13] is a NORMAL fp16 number (smallest .5 · 2^-13 = 2^-14, largest
6 · 2^13 < 65504) and one of bf16, so again the dequantised 16-bit matrix IS the quantised model (sx_gemv w_dtype = SX_FP4_E2M1).
Cost on N(0, 0.02^2) rows of K = 5120: 0.114 relative rms (FP8 per row: 0.027); round to nearest only, no calibration.

Everything here is integer / exact fp32 arithmetic in plain torch ops (no float8 cast, no pow / log2 whose last bit could depend on
the device): the same codes on the CPU and on the GPU.
"""
import torch

FP8_MAX = 448.0
S_MIN, S_MAX = -15, 7
LLAMA_PROJECTIONS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj",
                     "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def _pow2(e):
    """2^e as fp32 for an int32 tensor e in [-126, 127], built from the exponent field (exact on every device)."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def _exponent(v):
    """floor(log2 |v|) of a normal fp32 tensor as int32 (zero → -127)."""
    return ((v.contiguous().view(torch.int32) >> 23) & 0xff) - 127


def row_exponents(w, s_min=S_MIN, s_max=S_MAX):
    """s[n] = clamp(ceil(log2(amax[n] / 448)), s_min, s_max) as int32 (the weights' [-15, 7] by default), amax over the LAST dim;
    0 for an all-zero row. No division: with amax = 1.f · 2^E,
    amax <= 448 · 2^s = 1.75 · 2^(8 + s)  ⇔  s >= E - 8 (fraction <= .75) or s >= E - 7 (fraction > .75)."""
    amax = w.detach().abs().amax(dim=-1).to(torch.float32).contiguous()
    bits = amax.view(torch.int32)
    s = _exponent(amax) - 8 + ((bits & 0x7fffff) > 0x600000).to(torch.int32)
    s = s.clamp(s_min, s_max)
    return torch.where(amax == 0, torch.zeros_like(s), s)


def encode_e4m3(v):
    """fp32 tensor → e4m3fn codes (uint8): clamp to ±448, round to nearest even. Bit-identical to
    ``v.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)`` for every finite input, -0 included."""
    v = v.to(torch.float32)
    a = v.abs().clamp(max=FP8_MAX)
    e = _exponent(a).clamp(min=-6)                       # normal codes: 2^e <= a < 2^(e+1), quantum 2^(e-3); subnormal: quantum 2^-9
    y = torch.round(a * _pow2(3 - e))                    # 0 .. 16 in units of the quantum (torch.round = half to even); 16 = next binade
    # code = (e + 6) · 8 + y: subnormals (e = -6) y = 0..7 → codes 0..7, y = 8 → code 8 = 2^-6; normals y = 8 + mantissa; y = 16 carries
    code = (e + 6) * 8 + y.to(torch.int32)
    code = torch.where(a == 0, torch.zeros_like(code), code)
    code = code | (torch.signbit(v).to(torch.int32) << 7)
    return code.to(torch.uint8)


def decode_table(device=None):
    """fp32 [256]: the value of every e4m3fn code (0x7f / 0xff = NaN)."""
    c = torch.arange(256, dtype=torch.int32, device=device)
    e, m = (c >> 3) & 15, (c & 7).to(torch.float32)
    val = torch.where(e == 0, m * 2.0 ** -9, (8.0 + m) * _pow2(e - 10))
    val = torch.where((c & 0x7f) == 0x7f, torch.full_like(val, float("nan")), val)
    return torch.where((c & 0x80) != 0, -val, val)


def quantize_rows(w):
    """16-bit (or fp32) W[N, K] → (codes uint8 [N, K], scale fp32 [N] = 2^s)."""
    assert w.dim() == 2
    s = row_exponents(w)
    codes = encode_e4m3(w.detach().to(torch.float32) * _pow2(-s)[:, None])
    return codes, _pow2(s)


def dequantize_rows(codes, scale, dtype=torch.float32):
    """codes uint8 [N, K], scale fp32 [N] → decode(code) · scale in ``dtype`` (exact in fp16 / bf16 for quantize_rows' scales)."""
    assert codes.dtype == torch.uint8 and codes.dim() == 2 and scale.shape == (codes.shape[0],)
    val = torch.index_select(decode_table(codes.device), 0, codes.reshape(-1).to(torch.int32)).view(codes.shape)
    return (val * scale.to(torch.float32)[:, None]).to(dtype)


# ---- FP8 KV cache (LlamaForCausalLM(kv_format="fp8_e4m3")): the same row rule on fp32 activations ------------------------------
# One row = the head_dim values of one (token, head), k after RoPE or v. The exponent clamp is [-64, 64] instead of the weights'
# [-15, 7]: that clamp makes dequantised WEIGHTS fp16-exact, which means nothing for fp32 activations and would cost precision on rows
# whose amax is below 448 · 2^-15 = 0.014; +-64 keeps every dequantised value, and its product with O(1) operands, a normal fp32.
# The device quantiser (csrc/precise.hip, quant_row8) computes the same codes and scales; non-finite inputs are outside the rule.
KV_S_MIN, KV_S_MAX = -64, 64


def quantize_kv_rows(x):
    """fp32 [..., D] → (codes uint8 [..., D], scale fp32 [...] = 2^s), s = clamp(ceil(log2(amax / 448)), -64, 64), 0 for a zero row."""
    x = x.detach().to(torch.float32)
    s = row_exponents(x, KV_S_MIN, KV_S_MAX)
    return encode_e4m3(x * _pow2(-s)[..., None]), _pow2(s)


def dequantize_kv_rows(codes, scale):
    """codes uint8 [..., D], scale fp32 [...] → decode(code) · scale, fp32 (exact: the scale is a power of two)."""
    assert codes.dtype == torch.uint8 and scale.shape == codes.shape[:-1]
    val = torch.index_select(decode_table(codes.device), 0, codes.reshape(-1).to(torch.int32)).view(codes.shape)
    return val * scale.to(torch.float32)[..., None]


# ---- MXFP4 weights (LlamaForCausalLM(weight_format="mxfp4")): e2m1 codes, one E8M0 scale per 32-k block (module docstring) ---------
FP4_MAX = 6.0
E_MIN, E_MAX = -13, 13
MX_BLOCK = 32


def encode_e2m1(v):
    """fp32 tensor → e2m1 codes 0..15 (uint8, bit 3 = sign): clamp to ±6, round to nearest, ties to the even code, -0 kept."""
    v = v.to(torch.float32)
    a = v.abs().clamp(max=FP4_MAX)
    e = _exponent(a).clamp(min=0)                        # a < 2: quantum .5 (codes 0..3, the subnormal .5 included); [2, 4): 1; [4, 6]: 2
    y = torch.round(a * _pow2(1 - e))                    # 0 .. 4 in units of the quantum (half to even); 4 = next binade
    code = e * 2 + y.to(torch.int32)                     # e = 0: 0, .5, 1, 1.5, (2); e = 1: y = 2..4 → 2, 3, (4); e = 2: y = 2, 3 → 4, 6
    code = code | (torch.signbit(v).to(torch.int32) << 3)
    return code.to(torch.uint8)


def decode_table_e2m1(device=None):
    """fp32 [16]: the value of every e2m1 code."""
    mag = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float32, device=device)
    return torch.cat([mag, -mag])


def block_exponents(w):
    """e[n, b] = clamp(floor(log2(amax of block b of row n)) - 2, -13, 13) as int32, blocks of 32 along the LAST dim; 0 for an all-zero
    block. floor(log2) is the exponent field of the fp32 amax."""
    assert w.shape[-1] % MX_BLOCK == 0
    amax = w.detach().abs().reshape(*w.shape[:-1], w.shape[-1] // MX_BLOCK, MX_BLOCK).amax(dim=-1).to(torch.float32).contiguous()
    e = (_exponent(amax) - 2).clamp(E_MIN, E_MAX)
    return torch.where(amax == 0, torch.zeros_like(e), e)


def quantize_blocks_mxfp4(w):
    """16-bit (or fp32) W[N, K], K % 64 == 0 → (codes uint8 [N, K/2]: byte i of a row = k 2i in the low nibble, k 2i + 1 in the high one;
    scale uint8 [N, K/32]: the E8M0 byte e + 127 of every block)."""
    assert w.dim() == 2 and w.shape[1] % 64 == 0, "MXFP4 blocks: K must be a multiple of 64"
    e = block_exponents(w)
    c = encode_e2m1(w.detach().to(torch.float32) * _pow2(-e).repeat_interleave(MX_BLOCK, dim=1))
    return (c[:, 0::2] | (c[:, 1::2] << 4)).contiguous(), (e + 127).to(torch.uint8)


def dequantize_blocks_mxfp4(codes, scale, dtype=torch.float32):
    """codes uint8 [N, K/2], scale uint8 [N, K/32] → decode(code) · 2^(scale - 127) in ``dtype`` [N, K] (exact in fp16 / bf16 for
    quantize_blocks_mxfp4's exponents)."""
    assert codes.dtype == torch.uint8 and scale.dtype == torch.uint8 and codes.dim() == 2
    assert scale.shape == (codes.shape[0], codes.shape[1] * 2 // MX_BLOCK)
    nib = torch.stack([codes & 15, codes >> 4], dim=-1).reshape(codes.shape[0], -1)
    val = torch.index_select(decode_table_e2m1(codes.device), 0, nib.reshape(-1).to(torch.int32)).view(nib.shape)
    return (val * _pow2(scale.to(torch.int32) - 127).repeat_interleave(MX_BLOCK, dim=1)).to(dtype)


def _codec(weight_format):
    if weight_format == "mxfp4":
        return quantize_blocks_mxfp4, dequantize_blocks_mxfp4
    assert weight_format == "fp8_e4m3", weight_format
    return quantize_rows, dequantize_rows


def quantize_llama_layer(sd, prefix, dtype, device=None, weight_format="fp8_e4m3"):
    """The seven projection matrices of one decoder layer (FULL matrices: after the LoRA merge, before any tensor-parallel slicing) →
    {key: (codes, scale, dequantised weight in ``dtype``)}. The checkpoint value is first rounded to ``dtype`` — what the 16-bit model
    would have held. ``weight_format``: "fp8_e4m3" (row scales) or "mxfp4" (packed codes, block scales)."""
    quantize, dequantize = _codec(weight_format)
    out = {}
    for n in LLAMA_PROJECTIONS:
        k = prefix + n + ".weight"
        w = sd[k].detach().to(device=device, dtype=dtype)
        codes, scale = quantize(w)
        out[k] = (codes, scale, dequantize(codes, scale, dtype))
    return out


def quantize_llama_state_dict(sd, cfg, dtype=torch.float16, weight_format="fp8_e4m3"):
    """→ (state dict with the seven projection matrices of every layer replaced by their dequantised values, {key: codes}, {key: scale}).
    Embedding, norms and lm_head stay as they are. ``cfg``: dict or config object with num_hidden_layers."""
    L = cfg["num_hidden_layers"] if isinstance(cfg, dict) else cfg.num_hidden_layers
    out, codes, scales = dict(sd), {}, {}
    for i in range(L):
        for k, (c, s, w) in quantize_llama_layer(sd, f"model.layers.{i}.", dtype, weight_format=weight_format).items():
            out[k], codes[k], scales[k] = (w.float() if sd[k].dtype == torch.float32 else w), c, s   # (exact either way)
    return out, codes, scales


def llama_tp_shard_scales(scales, layer_prefix, rank, tp, nh, hd):
    """Rank ``rank``'s row scales of one layer, keyed like parallel.llama_tp_shard: the row-sharded q / k / v / gate / up slice theirs,
    the column-sharded o / down keep every row (each rank holds columns of ALL rows) — the ranks hold slices of ONE quantised model."""
    hl = nh // tp * hd
    hs = slice(rank * hl, (rank + 1) * hl)
    p = layer_prefix
    il = scales[p + "mlp.gate_proj.weight"].shape[0] // tp
    isl = slice(rank * il, (rank + 1) * il)
    return {"q": scales[p + "self_attn.q_proj.weight"][hs], "k": scales[p + "self_attn.k_proj.weight"][hs],
            "v": scales[p + "self_attn.v_proj.weight"][hs], "o": scales[p + "self_attn.o_proj.weight"],
            "gate": scales[p + "mlp.gate_proj.weight"][isl], "up": scales[p + "mlp.up_proj.weight"][isl],
            "down": scales[p + "mlp.down_proj.weight"]}


def llama_tp_shard_mxfp4(codes, scales, layer_prefix, rank, tp, nh, hd):
    """Rank ``rank``'s MXFP4 codes and block scales of one layer → ({name: codes}, {name: scales}), keyed like parallel.llama_tp_shard.
    The FULL matrices were quantised; row-sharded q / k / v / gate / up slice rows of both, column-sharded o / down slice BOTH along K
    (codes: K_l / 2 bytes, scales: K_l / 32 blocks) — a per-rank K that is no multiple of 64 would cut a k-step and is refused."""
    assert nh % tp == 0
    hl = nh // tp * hd
    p = layer_prefix
    il = codes[p + "mlp.gate_proj.weight"].shape[0] // tp
    for name, kl in (("heads x head_dim", hl), ("FFN width", il)):
        if kl % 64 != 0:
            raise ValueError(f"MXFP4 tensor-parallel slices: the per-rank {name} {kl} is no multiple of 64 (o / down are sliced along K in "
                             "whole 64-k steps of two 32-k blocks)")
    hs, isl = slice(rank * hl, (rank + 1) * hl), slice(rank * il, (rank + 1) * il)
    cut = lambda d, div: {
        "q": d[p + "self_attn.q_proj.weight"][hs], "k": d[p + "self_attn.k_proj.weight"][hs], "v": d[p + "self_attn.v_proj.weight"][hs],
        "o": d[p + "self_attn.o_proj.weight"][:, rank * hl // div:(rank + 1) * hl // div],
        "gate": d[p + "mlp.gate_proj.weight"][isl], "up": d[p + "mlp.up_proj.weight"][isl],
        "down": d[p + "mlp.down_proj.weight"][:, rank * il // div:(rank + 1) * il // div]}
    return cut(codes, 2), cut(scales, MX_BLOCK)
