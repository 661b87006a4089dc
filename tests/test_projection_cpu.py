"""The projection handle of the Llama decoder (seedx_amd.projection.Projection) on CPU tensors: all three weight formats x tile rows
{16, 20} x GLU packing on / off at K = 256, N = 160 (divisible by 32 and by 20; q | k | v of 64 + 48 + 48 rows, gate | up of 80 + 80).
What it holds is the recipe LlamaForCausalLM._pack always used, spelled out here with the packers of ops, the codecs of quant and
glu_pack_rows; its byte counts are memory_footprint()'s closed forms; the keywords it hands ops.gemv name exactly one tile layout."""
import pytest
import torch

from seedx_amd import ops, quant
from seedx_amd.projection import Projection, glu_pack_rows

K, N = 256, 160
FORMATS = [None, "fp8_e4m3", "mxfp4"]
TILE_KEYS = {"w_tiles", "w_tiles20", "w_fp8", "w_fp4"}


def _parts(glu, dt, seed=0):
    """The row slices of one fused projection in ``dt``: (up, gate) for GLU, else (q, k, v)."""
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, K, generator=g) * 0.05).to(dt) for n in ((80, 80) if glu else (64, 48, 48))]


def _quantised(parts, fmt, dt):
    """Per part, as quant.quantize_llama_layer does per matrix: (codes, scales, dequantised matrix in dt)."""
    q, dq = quant._codec(fmt)
    cs = [q(p) for p in parts]
    return [c for c, _ in cs], [s for _, s in cs], [dq(c, s, dt) for c, s in cs]


@pytest.mark.parametrize("glu", [False, True], ids=["qkv", "glu"])
@pytest.mark.parametrize("rows", [16, 20])
@pytest.mark.parametrize("fmt", FORMATS, ids=["16bit", "fp8", "mxfp4"])
@pytest.mark.parametrize("keep", [True, False], ids=["rowmajor", "tiles_only"])
def test_handle_holds_the_pack_recipe(fmt, rows, glu, keep):
    dt = torch.float16
    parts = _parts(glu, dt)
    join = (lambda ts: glu_pack_rows(*ts)) if glu else (lambda ts: torch.cat(ts, dim=0))
    if fmt is None and not keep:                 # only quantised tiles can stand in for the row-major matrix
        with pytest.raises(AssertionError, match="row-major"):
            Projection.build(parts, dt, "cpu", glu=glu, tile_rows=rows, keep_matrix=False)
        return
    if fmt is None:
        h = Projection.build(parts, dt, "cpu", glu=glu, tile_rows=rows)
        w = join(parts).contiguous()
        want_tiles, want_scales = (ops.pack_decode_tiles20 if rows == 20 else ops.pack_decode_tiles)(w), None
        per_weight = 2.0
    else:
        codes, scales, deq = _quantised(parts, fmt, dt)
        h = Projection.build(deq, dt, "cpu", glu=glu, format=fmt, tile_rows=rows, codes=codes, scales=scales, keep_matrix=keep)
        w = join(deq).contiguous()
        c = join(codes).contiguous()
        if fmt == "fp8_e4m3":
            want_tiles = (ops.pack_decode_tiles20_fp8 if rows == 20 else ops.pack_decode_tiles_fp8)(c)
            # one fp32 scale per row, in the row order of the codes: GLU packing moves a scale with its row
            want_scales = glu_pack_rows(scales[0][:, None], scales[1][:, None]).reshape(-1) if glu else torch.cat(scales)
            assert torch.equal(quant.dequantize_rows(ops.unpack_decode_tiles_fp8(h.tiles), h.scales, dt), w)
            per_weight = 1.0 + 4.0 / K
        else:
            want_tiles = (ops.pack_decode_tiles20_fp4 if rows == 20 else ops.pack_decode_tiles_fp4)(c)
            # block-scale rows [N, K/32]: GLU packing moves whole rows of them, then the scale tiles take the code tiles' rows
            want_scales = ops.pack_block_scales_fp4(join(scales).contiguous(), rows=rows)
            assert torch.equal(quant.dequantize_blocks_mxfp4(ops.unpack_decode_tiles_fp4(h.tiles), ops.unpack_block_scales_fp4(h.scales), dt), w)
            per_weight = 0.5 + 1.0 / 32
    # 1. tiles and scales are the recipe's
    assert h.format == fmt and h.tile_rows == rows and tuple(h.shape) == (N, K) and h.dtype == dt
    assert torch.equal(h.tiles, want_tiles) and h.tiles.dtype == want_tiles.dtype and h.tiles.is_contiguous()
    if want_scales is None:
        assert h.scales is None
    else:
        assert torch.equal(h.scales, want_scales) and h.scales.dtype == want_scales.dtype and h.scales.is_contiguous()
    # 2. byte counts: memory_footprint()'s closed forms, 2 / 1 + 4/K / 1/2 + 1/32 bytes per weight
    assert h.nbytes_tiles == int(N * K * per_weight) == N * K * per_weight
    assert h.nbytes_rowmajor == (2 * N * K if keep else 0)
    # 3. what ops.gemv is handed: exactly one tile layout; ``w`` has storage iff the row-major copy is kept
    kw = h.gemv_kwargs("ws", act="silu", y_tiled=True)
    want_key = {None: "w_tiles20" if rows == 20 else "w_tiles", "fp8_e4m3": "w_fp8", "mxfp4": "w_fp4"}[fmt]
    assert TILE_KEYS & set(kw) == {want_key}
    assert kw[want_key] is h.tiles if fmt is None else (kw[want_key][0] is h.tiles and kw[want_key][1] is h.scales)
    assert kw["workspace"] == "ws" and kw["act"] == "silu" and kw["y_tiled"] is True and h.gemv_kwargs()["workspace"] is None
    assert set(kw) == {"w", want_key, "workspace", "act", "y_tiled"}
    assert isinstance(kw["w"], ops.WeightShape) == (not keep) == (h.w is None)
    assert tuple(kw["w"].shape) == (N, K) and kw["w"].dtype == dt
    if keep:
        assert kw["w"] is h.w and torch.equal(h.w, w) and h.matrix() is h.w
    else:
        assert kw["w"].data_ptr() == 0


@pytest.mark.parametrize("fmt", FORMATS, ids=["16bit", "fp8", "mxfp4"])
def test_handle_without_tiles(fmt):
    """tiled=False (the plain flow below 5 sequences, shapes outside the MFMA path): the row-major matrix alone, no tile keyword."""
    parts = _parts(False, torch.bfloat16)
    h = Projection.build(parts, torch.bfloat16, "cpu", format=fmt, tiled=False)
    assert h.format == fmt and h.tiles is None and h.scales is None and h.nbytes_tiles == 0 and h.nbytes_rowmajor == 2 * N * K
    kw = h.gemv_kwargs()
    assert not TILE_KEYS & set(kw) and kw["w"] is h.w and torch.equal(h.w, torch.cat(parts))


@pytest.mark.parametrize("glu", [False, True], ids=["qkv", "glu"])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_gamma_folded_handle_keeps_the_unfolded_matrix(glu, dt):
    """The plain flow's RMSNorm fold: the tiles hold W · diag(gamma), formed in fp32 from the checkpoint's values (here fp32 values that
    are NOT 16-bit numbers) and rounded once; the matrix kept for prefill is the unfolded one."""
    g = torch.Generator().manual_seed(3)
    parts = [p.float() * 1.0009765625 + 1e-4 for p in _parts(glu, torch.float32, seed=4)]
    gamma = (1.0 + 0.5 * torch.randn(K, generator=g)).abs().clamp_min(0.2)
    h = Projection.build(parts, dt, "cpu", glu=glu, tile_gamma=gamma)
    join = (lambda ts: glu_pack_rows(*ts)) if glu else (lambda ts: torch.cat(ts, dim=0))
    folded = join([(p.to(torch.float32) * gamma[None, :]).to(dt) for p in parts]).contiguous()
    unfolded = join([p.to(dt) for p in parts]).contiguous()
    assert torch.equal(h.w, unfolded) and torch.equal(h.tiles, ops.pack_decode_tiles(folded))
    twice = join([(p.to(dt).to(torch.float32) * gamma[None, :]).to(dt) for p in parts])           # rounding the weight first differs
    assert not torch.equal(folded, twice) and not torch.equal(folded, unfolded)
    assert h.nbytes_tiles == h.nbytes_rowmajor == 2 * N * K and "w_tiles" in h.gemv_kwargs()
