"""One weight handle per LLM projection (wqkv, wo, wgu, wd): shape, dtype, format, the ONE decode-tile layout the token step streams
(16- or 20-row tiles, + scales where the format has them) and the row-major matrix prefill reads (None under the tiles residency).
``P["layers"][i][k]`` of LlamaForCausalLM is such a handle; it is also the only place that knows which ops.gemv keyword a layout takes."""
import torch

from . import ops

# format → {tile rows: packer of the row-major matrix (None) / codes (quantised formats)} and the ops.gemv keyword of that layout
PACKERS = {None: {16: ops.pack_decode_tiles, 20: ops.pack_decode_tiles20},
           "fp8_e4m3": {16: ops.pack_decode_tiles_fp8, 20: ops.pack_decode_tiles20_fp8},
           "mxfp4": {16: ops.pack_decode_tiles_fp4, 20: ops.pack_decode_tiles20_fp4}}
GEMV_KEY = {(None, 16): "w_tiles", (None, 20): "w_tiles20", ("fp8_e4m3", 16): "w_fp8", ("fp8_e4m3", 20): "w_fp8",
            ("mxfp4", 16): "w_fp4", ("mxfp4", 20): "w_fp4"}


def glu_pack_rows(lin, gate):
    """[I,K] linear rows and [I,K] gate rows → [2I,K] in 32-row groups [16 linear | 16 gate] (sx_gemm glu contract)."""
    I, K = lin.shape
    assert I % 16 == 0
    return torch.cat([lin.view(I // 16, 16, K), gate.view(I // 16, 16, K)], dim=1).reshape(2 * I, K).contiguous()


def join_rows(parts, glu=False):
    """The rows of a fused projection from its parts: q | k | v concatenated, or (linear, gate) = (up, gate) GLU-packed. One rule for
    matrices, codes, MXFP4 block-scale rows [rows, K/32] and FP8 row scales [rows] (a scale moves with its row)."""
    if parts[0].dim() == 1:
        return join_rows([p[:, None] for p in parts], glu).reshape(-1)
    return glu_pack_rows(*parts) if glu else parts[0] if len(parts) == 1 else torch.cat(list(parts), dim=0)


def _nbytes(t):
    return 0 if t is None else t.numel() * t.element_size()


class Projection:
    def __init__(self, shape, dtype, format=None, tile_rows=16, tiles=None, scales=None, w=None):
        assert format in PACKERS and tile_rows in (16, 20) and (scales is None) == (format is None or tiles is None)
        assert w is not None or (format is not None and tiles is not None), "only quantised tiles can stand in for the row-major matrix"
        self.shape, self.dtype, self.format, self.tile_rows = torch.Size(shape), dtype, format, tile_rows
        self.tiles, self.scales, self.w = tiles, scales, w
        self._w = w if w is not None else ops.WeightShape(shape, dtype)      # what ops.gemv takes as ``w``: the tiles are the only copy

    @classmethod
    def build(cls, parts, dtype, device, glu=False, format=None, tile_rows=16, tiled=True, codes=None, scales=None, tile_gamma=None,
              keep_matrix=True):
        """parts: the row slices of the (dequantised, where quantised) matrix — one matrix, q | k | v, or (up, gate) with ``glu``.
        16-bit: the tiles are packed from the matrix, or, with ``tile_gamma`` (fp32 [K], the plain flow's RMSNorm fold), from
        W · diag(gamma) formed in fp32 from the parts as given and rounded ONCE, while the matrix kept stays unfolded. Quantised:
        ``codes`` / ``scales`` are the parts' codes and row scales (FP8) or block-scale rows (MXFP4), joined by the same rule.
        ``tiled`` False: no tiles (nothing would read them). ``keep_matrix`` False: the tiles residency."""
        w = join_rows([p.detach().to(device, dtype) for p in parts], glu).contiguous()
        t = sc = None
        if tiled and format is None:
            src = w if tile_gamma is None else \
                join_rows([(p.detach().to(device, torch.float32) * tile_gamma[None, :]).to(dtype) for p in parts], glu).contiguous()
            t = PACKERS[None][tile_rows](src)
        elif tiled:
            t = PACKERS[format][tile_rows](join_rows(codes, glu).contiguous())
            sc = join_rows(scales, glu).contiguous()
            sc = ops.pack_block_scales_fp4(sc, rows=tile_rows) if format == "mxfp4" else sc.clone()
        return cls(w.shape, dtype, format, tile_rows, t, sc, w if keep_matrix else None)

    nbytes_tiles = property(lambda self: _nbytes(self.tiles) + _nbytes(self.scales))
    nbytes_rowmajor = property(lambda self: _nbytes(self.w))

    def gemv_kwargs(self, workspace=None, **epilogue_kw):
        """The keyword arguments of the ops.gemv call behind gemv(): ``w`` (the row-major matrix, or an ops.WeightShape where there
        is none) and exactly one of w_tiles / w_tiles20 / w_fp8 / w_fp4 (none without tiles)."""
        kw = dict(w=self._w, workspace=workspace, **epilogue_kw)
        if self.tiles is not None:
            kw[GEMV_KEY[self.format, self.tile_rows]] = self.tiles if self.format is None else (self.tiles, self.scales)
        return kw

    def gemv(self, x, workspace=None, **epilogue_kw):
        return ops.gemv(x, **self.gemv_kwargs(workspace, **epilogue_kw))

    def matrix(self, scratch=None):
        """The row-major matrix; under the tiles residency rebuilt (exactly: sx_dequant_tiles) into ``scratch``."""
        if self.w is not None:
            return self.w
        return ops.dequant_tiles(dtype=self.dtype, out=scratch, **{GEMV_KEY[self.format, self.tile_rows]: (self.tiles, self.scales)})
