"""LlamaForCausalLM(weight_residency="tiles") and sx_dequant_tiles without a GPU: the argument struct against the header, the host
inverses of the decode-tile packers (the references the kernel is tested against), memory_footprint() at 13B dims in closed form, mode
selection and refusals."""
import os
import re

import pytest
import torch

from oracle import weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = ("SX_LLM_WEIGHTS", "SX_LLM_PRECISE", "SX_GEMV_BAL20", "SX_LLM_KV", "SX_LLM_WEIGHT_RESIDENCY")


def test_dequant_tiles_struct_layout_matches_header():
    """Field order / count of sx_dequant_tiles_args mirror the header (the parsing of tests/test_prefix_cache_cpu.py)."""
    from seedx_amd import _lib
    src = open(os.path.join(ROOT, "include", "seedx_hip.h")).read()
    cname = "sx_dequant_tiles_args"
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        decl = re.sub(r"^(const\s+)?(void|float|double|int32_t|int64_t|uint32_t|uint64_t)\s*\*?", "", decl)
        names += [n.strip().lstrip("*") for n in decl.split(",")]
    assert names == [f[0] for f in _lib.DequantTilesArgs._fields_], names
    for want in ("tiles", "w_scale", "w_block_scale", "w_dtype", "w_layout", "N", "K", "dtype", "out", "out_bytes"):
        assert want in names, want
    assert "sx_dequant_tiles" in _lib.SIGNATURES
    assert re.search(r"int sx_dequant_tiles\(const sx_dequant_tiles_args\* args, void\* stream\);", src)


@pytest.mark.parametrize("N,K", [(64, 256), (160, 320)])
@pytest.mark.parametrize("rows", [16, 20])
def test_host_unpackers_invert_the_packers(N, K, rows):
    """unpack_*(pack_*(x)) == x on random codes and scales, both formats, 16- and 20-row tiles. (64, 256) has no 20-row form (64 is no
    multiple of 20): there the 20-row packers must refuse."""
    from seedx_amd import ops
    g = torch.Generator().manual_seed(N + rows)
    c8 = torch.randint(0, 256, (N, K), dtype=torch.uint8, generator=g)
    c4 = torch.randint(0, 256, (N, K // 2), dtype=torch.uint8, generator=g)
    sc = torch.randint(0, 256, (N, K // 32), dtype=torch.uint8, generator=g)
    p8 = ops.pack_decode_tiles_fp8 if rows == 16 else ops.pack_decode_tiles20_fp8
    p4 = ops.pack_decode_tiles_fp4 if rows == 16 else ops.pack_decode_tiles20_fp4
    if N % rows:
        for f, a in ((p8, c8), (p4, c4), (lambda s: ops.pack_block_scales_fp4(s, rows=rows), sc)):
            with pytest.raises(AssertionError):
                f(a)
        return
    t8, t4, ts = p8(c8), p4(c4), ops.pack_block_scales_fp4(sc, rows=rows)
    assert t8.shape == (N // rows, K // 64, rows, 64) and t4.shape == (N // rows, K // 64, rows, 32) and ts.shape == (N // rows, K // 64, rows, 2)
    assert torch.equal(ops.unpack_decode_tiles_fp8(t8), c8)
    assert torch.equal(ops.unpack_decode_tiles_fp4(t4), c4)
    assert torch.equal(ops.unpack_block_scales_fp4(ts), sc)
    # the documented byte order, spelled out on one element each: FP8 byte 16 g + 8 h + j holds k = 32 h + 8 g + j; MXFP4 byte
    # 8 g + 4 h + i holds k = 32 h + 8 g + 2 i (and + 1); scale byte h of (row, k-step t) is block 2 t + h
    n, t, gg, h, j = 21, K // 64 - 1, 3, 1, 5
    assert t8[n // rows, t, n % rows, 16 * gg + 8 * h + j] == c8[n, 64 * t + 32 * h + 8 * gg + j]
    assert t4[n // rows, t, n % rows, 8 * gg + 4 * h + (j & 3)] == c4[n, (64 * t + 32 * h + 8 * gg + 2 * (j & 3)) // 2]
    assert ts[n // rows, t, n % rows, h] == sc[n, 2 * t + h]


def test_weight_shape_handle_owns_no_storage():
    from seedx_amd import ops
    w = ops.WeightShape((48, 256), torch.bfloat16)
    assert tuple(w.shape) == (48, 256) and w.shape[0] == 48 and w.dtype == torch.bfloat16 and w.numel() == 48 * 256
    assert w.is_contiguous() and w.data_ptr() == 0 and not torch.is_tensor(w)


def test_mode_selection_and_refusals(monkeypatch):
    from seedx_amd.llama import LlamaForCausalLM
    cfg = dict(weights.MINI_LLM)
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    assert LlamaForCausalLM(dict(cfg), max_cache_len=64).weight_residency is None
    assert LlamaForCausalLM(dict(cfg), max_cache_len=64, weight_format="mxfp4").weight_residency is None
    for fmt in ("mxfp4", "fp8_e4m3"):
        m = LlamaForCausalLM(dict(cfg), max_cache_len=64, max_batch=4, weight_format=fmt, weight_residency="tiles")
        assert m.weight_residency == "tiles" and m.weight_format == fmt and m.precise
    with pytest.raises(ValueError, match="weight_format"):
        LlamaForCausalLM(dict(cfg), max_cache_len=64, weight_residency="tiles")
    with pytest.raises(ValueError, match="weight_residency"):
        LlamaForCausalLM(dict(cfg), max_cache_len=64, weight_format="mxfp4", weight_residency="rows")
    with pytest.raises(ValueError, match="weight_residency"):
        LlamaForCausalLM(dict(cfg), max_cache_len=64, weight_residency="rows")
    monkeypatch.setenv("SX_LLM_WEIGHT_RESIDENCY", "tiles")                      # the A/B switch
    assert LlamaForCausalLM(dict(cfg), max_cache_len=64, weight_format="fp8_e4m3").weight_residency == "tiles"
    with pytest.raises(ValueError, match="weight_format"):
        LlamaForCausalLM(dict(cfg), max_cache_len=64)
    monkeypatch.setenv("SX_LLM_WEIGHT_RESIDENCY", "rows")
    with pytest.raises(ValueError, match="weight_residency"):
        LlamaForCausalLM(dict(cfg), max_cache_len=64, weight_format="mxfp4")


def test_from_pretrained_carries_the_keyword(tmp_path, monkeypatch):
    import json
    from safetensors.torch import save_file
    from seedx_amd.llama import LlamaForCausalLM
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    cfg = dict(weights.MINI_LLM, num_hidden_layers=1)
    json.dump(cfg, open(tmp_path / "config.json", "w"))
    save_file({k: v.contiguous() for k, v in weights.llama_sd(cfg).items()}, str(tmp_path / "model.safetensors"))
    m = LlamaForCausalLM.from_pretrained(str(tmp_path), weight_format="mxfp4", weight_residency="tiles", max_cache_len=64)
    assert m.weight_format == "mxfp4" and m.weight_residency == "tiles"
    with pytest.raises(ValueError, match="weight_format"):
        LlamaForCausalLM.from_pretrained(str(tmp_path), weight_residency="tiles", max_cache_len=64)


@pytest.mark.parametrize("fmt", ["mxfp4", "fp8_e4m3"])
def test_footprint_at_13b_dims(monkeypatch, fmt):
    """H 5120, I 13824, L 40, V 32330, constructed without packing. "tiles": weights = embedding + lm_head + the 2 * 2 I H scratch buffer
    (gate|up, the largest projection), decode tiles / KV cache as at default residency, total below the default's by exactly
    L * per_layer_16bit - scratch. The default-residency dicts are the ones the earlier tests pin (keys and values)."""
    from seedx_amd.llama import LlamaForCausalLM
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    cfg = dict(weights.FULL_LLM)
    H, I, L, V = 5120, 13824, 40, 32330
    assert (cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"], cfg["vocab_size"]) == (H, I, L, V)
    kw = dict(max_cache_len=1024, max_batch=16)
    d = LlamaForCausalLM(dict(cfg), **kw).memory_footprint()
    q = LlamaForCausalLM(dict(cfg), weight_format=fmt, **kw).memory_footprint()
    tm = LlamaForCausalLM(dict(cfg), weight_format=fmt, weight_residency="tiles", **kw)
    t = tm.memory_footprint()
    nk = 3 * H * H + H * H + 2 * I * H + H * I
    per_layer = nk * 2
    Vl = tm.V_l
    tiles = L * (nk // 2 + nk // 32) if fmt == "mxfp4" else L * (nk + (3 * H + H + 2 * I + H) * 4)
    kv = L * 16 * 40 * 1024 * 128 * 8
    # default residency, with and without a format: the parent's dicts
    assert d == {"weights": L * per_layer + (V + Vl) * H * 2, "decode_tiles": L * per_layer + Vl * H * 2, "kv_cache": kv,
                 "total": 2 * L * per_layer + (V + 2 * Vl) * H * 2 + kv}
    assert q == {"weights": d["weights"], "decode_tiles": tiles + Vl * H * 2, "kv_cache": kv,
                 "total": d["weights"] + tiles + Vl * H * 2 + kv}
    scratch = 2 * 2 * I * H
    assert scratch == 283_115_520
    assert t == {"weights": (V + Vl) * H * 2 + scratch, "prefill_scratch": scratch, "decode_tiles": tiles + Vl * H * 2, "kv_cache": kv,
                 "total": (V + Vl) * H * 2 + scratch + tiles + Vl * H * 2 + kv}
    assert t["total"] == t["weights"] + t["decode_tiles"] + t["kv_cache"]
    assert q["total"] - t["total"] == L * per_layer - scratch
    # tensor parallelism: the scratch buffer is the largest PER-RANK projection
    from seedx_amd.parallel import Comm

    class _Two(Comm):
        def __init__(self):
            self.rank, self.world = 0, 2
    t2 = LlamaForCausalLM(dict(cfg), weight_format=fmt, weight_residency="tiles", comm=_Two(), **kw).memory_footprint()
    assert t2["prefill_scratch"] == scratch // 2
