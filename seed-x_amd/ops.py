"""Thin torch-tensor wrappers over the C-ABI kernels (include/seedx_hip.h).

PyTorch is used only for device memory and the current HIP stream: every wrapper passes ``data_ptr()``s and
``torch.cuda.current_stream().cuda_stream`` to libseedx_hip.so. There is no eager/CPU fallback — a missing
library or a non-CUDA tensor raises.
"""
import contextlib
import ctypes as C
import gc
import math

import os

import torch

from . import _lib
from ._lib import (SX_A_CONV3X3, SX_A_LINEAR, SX_ACT_GELU, SX_ACT_NONE, SX_ACT_SILU, SX_BF16, SX_F16, SX_F32,
                   AttnArgs, AttnSmallArgs, GemmArgs, GemvArgs, check)

_DT = {torch.float16: SX_F16, torch.bfloat16: SX_BF16, torch.float32: SX_F32}
_TD = {v: k for k, v in _DT.items()}
ACT = {None: SX_ACT_NONE, "none": SX_ACT_NONE, "gelu": SX_ACT_GELU, "silu": SX_ACT_SILU}


def dt_code(dtype):
    return _DT[dtype]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("seedx_amd.ops: tensors must live on the GPU (no CPU fallback)")
    return C.c_void_p(t.data_ptr())


@contextlib.contextmanager
def graph_capture(g):
    """``with torch.cuda.graph(g)`` with Python's cyclic garbage collector out of the way: torch no longer collects when a capture starts,
    and a collection that fires INSIDE one may finalise a dead object that owns GPU resources (an earlier model's captured graph or
    side stream, kept by a reference cycle) — destroying those is not allowed while a stream captures and aborts the process. Collect
    first, keep the collector off until the capture has ended."""
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(g):
            yield
    finally:
        if was:
            gc.enable()


def _f32c(t):
    """fp32 contiguous parameter tensor or None."""
    if t is None:
        return None
    assert t.dtype == torch.float32 and t.is_contiguous(), "expected contiguous fp32 tensor"
    return t


# ---------------------------------------------------------------------------------------------------------
# GEMM family
# ---------------------------------------------------------------------------------------------------------
class GnStats:
    """fp64 GroupNorm statistics [B, groups, 2] of a tensor that a GEMM / conv is about to produce: handed to the PRODUCER
    (``gemm(..., gn=...)`` / ``conv3x3(..., gn=...)``), whose epilogue accumulates them when it runs on a ping-pong tile (then
    ``ready`` is set), and to the CONSUMER ``groupnorm(..., stats=...)``, which then skips its own zero + statistics launches.
    ``buf`` must be zero before the producer runs (slices of one arena zeroed once per forward: ``GnStats.arena``)."""
    __slots__ = ("buf", "groups", "rows", "ready")

    def __init__(self, buf, groups, rows):
        self.buf, self.groups, self.rows, self.ready = buf, int(groups), int(rows), False

    @staticmethod
    def arena(n, B, groups, device):
        """n zeroed [B, groups, 2] fp64 slots with ONE fill launch."""
        return torch.zeros((n, B, groups, 2), dtype=torch.float64, device=device)


class LnRows:
    """A LayerNorm folded into the GEMMs either side of it (sx_gemm_ln): the PRODUCER (``gemm(..., ln_emit=rows)``: fp32 output)
    also writes ``x16`` = its output rounded to the operand dtype and adds the rows' (sum, sum of squares) to ``stats`` [M, 2]
    fp64 (zero beforehand); the CONSUMER (``gemm(rows.x16, w_folded, bias=b_folded, ln_apply=(rows, colsum, eps))``) applies
    (mu, rstd) per row in its epilogue. Both launches must run on ping-pong tiles: ``ln_fold_ok`` says so beforehand."""
    __slots__ = ("x16", "stats")

    def __init__(self, M, C, dtype, device, stats=None):
        self.x16 = torch.empty((M, C), dtype=dtype, device=device)
        self.stats = stats if stats is not None else torch.zeros((M, 2), dtype=torch.float64, device=device)
        assert self.stats.shape == (M, 2) and self.stats.dtype == torch.float64 and self.stats.is_contiguous()


def gemm_tile(M, N, K, glu=False, conv=False):
    """Tile config 0..8 the cost model gives an M x N x K problem (7 / 8 = the 256-row ping-pong tiles); host-only."""
    return int(_lib.load().sx_gemm_pick_tile(int(M), int(N), int(K), 1 if glu else 0, 1 if conv else 0))


def ln_fold_ok(M, C, consumers, producers):
    """True when every GEMM around a LayerNorm of width C over M rows runs on a ping-pong tile. consumers: [(N, glu)] of the
    projections behind the norm (K = C); producers: [K] of the fp32-output projections ahead of it (N = C)."""
    return all(gemm_tile(M, n, C, glu) >= 7 for n, glu in consumers) and all(gemm_tile(M, C, k) >= 7 for k in producers)


def fold_layernorm(w, bias, gamma, beta):
    """(w', colsum, bias') of a projection behind LayerNorm(gamma, beta): w' = w * gamma in w's dtype, colsum[n] = sum_k w'[n, k]
    (of the ROUNDED w': what the MFMA multiplies), bias' = bias + w beta. Per output row, so GLU-packed rows fold as they are."""
    wf = (w.float() * gamma.float()[None, :]).to(w.dtype).contiguous()
    cs = wf.float().sum(dim=1).contiguous()
    b = w.float() @ beta.float()
    if bias is not None:
        b = b + bias.float()
    return wf, cs, b.contiguous()


GN_FUSE = os.environ.get("SX_GN_FUSE", "1") != "0"     # A/B switch (tools/bench_unet_ab.py): 0 = every GroupNorm runs its own statistics pass


def _launch_gemm(lib, args, gn, what):
    if gn is None or not GN_FUSE:
        check(lib.sx_gemm(C.byref(args), _stream()), what)
        return
    assert gn.buf.dtype == torch.float64 and gn.buf.is_contiguous() and args.M % gn.rows == 0 \
        and gn.buf.numel() == (args.M // gn.rows) * gn.groups * 2, "GnStats does not describe this output"
    fused = C.c_int32(0)
    check(lib.sx_gemm_gn(C.byref(args), gn.buf.data_ptr(), gn.groups, gn.rows, C.byref(fused), _stream()), what)
    gn.ready = bool(fused.value)


def gemm(a, w, bias=None, bias2d=None, bias2d_rows=0, residual=None, res_mod=0, act=None, glu=False,
         out_dtype=None, out=None, n_valid=0, ld_bias2d=0, gn=None, ln_emit=None, ln_apply=None, a_planes=1):
    """out[M, N_out] = epilogue(a[M, K] @ w[N, K]^T). a, w: 16-bit contiguous. residual/bias fp32.
    gn: optional GnStats of the output (the next GroupNorm's statistics pass fused into this launch, see GnStats).
    ln_emit / ln_apply: the two sides of a folded LayerNorm (see LnRows).
    a_planes = 2: a is [M, 2K] = [hi | lo], the planes of an fp32-grade activation (split16 / rmsnorm_planes / attention_f32)."""
    lib = _lib.load()
    assert a.dim() == 2 and w.dim() == 2 and a.is_contiguous() and w.is_contiguous()
    assert a.dtype == w.dtype and a.dtype in (torch.float16, torch.bfloat16)
    M, K = a.shape
    N = w.shape[0]
    assert a_planes in (1, 2) and K % a_planes == 0
    K //= a_planes
    assert w.shape[1] == K, f"K mismatch {a.shape} vs {w.shape} (a_planes {a_planes})"
    n_out = N // 2 if glu else N
    n_store = n_valid if n_valid else n_out
    out_dtype = out_dtype or a.dtype
    if out is None:
        out = torch.empty((M, n_store), dtype=out_dtype, device=a.device)
    assert out.dtype == out_dtype and out.stride(-1) == 1 and out.shape[0] == M
    args = GemmArgs()
    args.A, args.W, args.C = a.data_ptr(), w.data_ptr(), out.data_ptr()
    args.bias = _f32c(bias).data_ptr() if bias is not None else None
    if bias2d is not None:
        assert bias2d.dtype == torch.float32 and bias2d.stride(-1) == 1
        args.bias2d = bias2d.data_ptr()
        args.ld_bias2d = ld_bias2d or bias2d.stride(0)
    if residual is not None:
        assert residual.dtype == torch.float32 and residual.stride(-1) == 1
        args.residual = residual.data_ptr()
        args.ldr = residual.stride(0)
    args.M, args.N, args.K = M, N, K
    args.ldc = out.stride(0)
    args.n_valid = n_valid
    args.res_mod = res_mod
    args.bias2d_rows = bias2d_rows
    args.dtype = _DT[a.dtype]
    args.out_dtype = _DT[out_dtype]
    args.act = ACT[act]
    args.glu = 1 if glu else 0
    args.a_mode = SX_A_LINEAR
    args.a_planes = a_planes
    if ln_emit is not None or ln_apply is not None:
        assert gn is None and not (ln_emit is not None and ln_apply is not None)
        la = _lib.GemmLnArgs()
        if ln_emit is not None:
            assert ln_emit.x16.shape == (M, N) and ln_emit.x16.dtype == a.dtype and ln_emit.stats.shape[0] == M
            la.x16_out, la.ld_x16, la.row_stats_out = ln_emit.x16.data_ptr(), ln_emit.x16.stride(0), ln_emit.stats.data_ptr()
        else:
            rows, colsum, eps = ln_apply
            assert rows.stats.shape[0] == M and colsum.dtype == torch.float32 and colsum.numel() == N and colsum.is_contiguous()
            la.row_stats_in, la.colsum, la.dim, la.eps = rows.stats.data_ptr(), colsum.data_ptr(), K, float(eps)
        check(lib.sx_gemm_ln(C.byref(args), C.byref(la), _stream()), "sx_gemm_ln")
        return out
    _launch_gemm(lib, args, gn, "sx_gemm")
    return out


_PHASE_TAPS = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}   # R(parity, phase tap): the 3x3 taps that share a source pixel


def pack_upsample_phases(w, planes=1, dtype=None, rounded=True):
    """Weights of a 3x3 / pad 1 conv over a nearest-2x up-sampled image → the four 2x2 phase filters over the SOURCE image
    (sx_gemm_args.upsample = 2: 16 products per input pixel, not 36). w: [Cout, 9*C] in (ky, kx, c) order. Output pixel (2i + a, 2j + c)
    reads source pixels (i + a - 1 + u, j + c - 1 + v), u, v in {0, 1}; the taps that land on one of them are summed in fp64:
        Wp[2a + c][n][(2u + v) C + ch] = sum_{ky in R(a, u)} sum_{kx in R(c, v)} w[n][ky][kx][ch],   R = _PHASE_TAPS
    and rounded ONCE: planes = 1 → to `dtype` (default w's); planes = 3 (the fp32-grade VAE) → to fp32, then split per tap into the
    bf16 planes [hi | lo | hi] of vae.pack_planes. Returns [4, Cout, 4*planes*C] contiguous (rounded=False: the fp64 sums, planes = 1)."""
    assert w.dim() == 2 and w.shape[1] % 9 == 0 and planes in (1, 3)
    Cout, C = w.shape[0], w.shape[1] // 9
    w9 = w.detach().double().reshape(Cout, 3, 3, C)
    wp = torch.zeros((4, Cout, 2, 2, C), dtype=torch.float64, device=w.device)
    for (a, u), kys in _PHASE_TAPS.items():
        for (c, v), kxs in _PHASE_TAPS.items():
            for ky in kys:
                for kx in kxs:
                    wp[2 * a + c, :, u, v] += w9[:, ky, kx]
    if not rounded:
        assert planes == 1
        return wp.view(4, Cout, 4 * C)
    if planes == 1:
        return wp.to(dtype or w.dtype).view(4, Cout, 4 * C).contiguous()
    s32 = wp.float()
    hi = s32.to(torch.bfloat16)
    lo = (s32 - hi.float()).to(torch.bfloat16)
    return torch.cat([hi, lo, hi], dim=4).view(4, Cout, 12 * C).contiguous()


def upsample_phases_ok(B, H, W):
    """The shape gate of sx_gemm's upsample = 2: a 256-row ping-pong tile must lie inside one output parity."""
    return (B * H * W) % 256 == 0


def conv3x3(x, w, bias=None, bias2d=None, residual=None, stride=1, upsample=False, out_dtype=None, act=None,
            n_valid=0, pad_mode=0, gn=None, w_phases=None, out=None):
    """3x3 / pad 1 convolution as implicit GEMM. x: [B, H, W, Cin] 16-bit NHWC contiguous; w: [Cout, 9*Cin]
    ((ky,kx,cin)-ordered). Returns [B, Hout*Wout, Cout] (NHWC flattened). bias2d: [B, Cout] fp32 per-sample add.
    residual: fp32 [B*Hout*Wout, Cout]. pad_mode 1 = pad only bottom/right (VAE encoder's stride-2 convs).
    w_phases (upsample only): pack_upsample_phases(w) [4, Cout, 4*Cin]. Used when the shape gate holds and the call has neither a
    residual nor fused GroupNorm statistics (upsample_phases_ok; 16 taps per input pixel); every other call runs the 36-tap gather
    from w as before. out: optional [B*Hout*Wout, n_store] contiguous tensor of out_dtype to store into."""
    lib = _lib.load()
    assert x.dim() == 4 and x.is_contiguous()
    B, H, W, Cin = x.shape
    phases = (w_phases is not None and upsample and stride == 1 and pad_mode == 0 and residual is None and gn is None
              and act is None and upsample_phases_ok(B, H, W))
    if phases:
        assert w_phases.dim() == 3 and w_phases.shape[0] == 4 and w_phases.shape[2] == 4 * Cin and w_phases.dtype == x.dtype
        w = w_phases
        Cout, K = w.shape[1], 4 * Cin
    else:
        assert w is not None, "conv3x3: this call needs the 36-tap weight (the phase gate does not hold)"
        Cout, K = w.shape
        assert K == 9 * Cin
    assert w.is_contiguous()
    hv, wv = (2 * H, 2 * W) if upsample else (H, W)
    padsum = 1 if pad_mode else 2
    Hout, Wout = (hv + padsum - 3) // stride + 1, (wv + padsum - 3) // stride + 1
    M = B * Hout * Wout
    out_dtype = out_dtype or x.dtype
    n_store = n_valid if n_valid else Cout
    if out is None:
        out = torch.empty((M, n_store), dtype=out_dtype, device=x.device)
    assert out.shape == (M, n_store) and out.dtype == out_dtype and out.is_contiguous()
    args = GemmArgs()
    args.A, args.W, args.C = x.data_ptr(), w.data_ptr(), out.data_ptr()
    args.bias = _f32c(bias).data_ptr() if bias is not None else None
    args.n_valid = n_valid
    if bias2d is not None:
        assert bias2d.dtype == torch.float32 and bias2d.stride(-1) == 1 and bias2d.shape == (B, Cout)
        args.bias2d = bias2d.data_ptr()
        args.bias2d_rows = Hout * Wout
        args.ld_bias2d = bias2d.stride(0)
    if residual is not None:
        assert residual.dtype == torch.float32 and residual.stride(-1) == 1
        args.residual = residual.data_ptr()
        args.ldr = residual.stride(0)
    args.M, args.N, args.K = M, Cout, K
    args.ldc = n_store
    args.dtype = _DT[x.dtype]
    args.out_dtype = _DT[out_dtype]
    args.act = ACT[act]
    args.a_mode = SX_A_CONV3X3
    args.B, args.Hin, args.Win, args.Cin, args.Hout, args.Wout = B, H, W, Cin, Hout, Wout
    args.stride = stride
    args.upsample = (2 if phases else 1) if upsample else 0
    args.pad_mode = pad_mode
    _launch_gemm(lib, args, gn, "sx_gemm(conv3x3)")
    return out.view(B, Hout * Wout, n_store)


def pack_decode_tiles(w):
    """Row-major [N, K] 16-bit weight → the decode layout [N/16][K/32][16][32] (same shape, other element order): every
    16-row x 32-k MFMA operand tile is 1 KB contiguous and the tiles of a row group follow each other along K, so the skinny
    GEMM's wave-wide loads are whole contiguous kilobytes instead of 64-B pieces of 16 rows 2K bytes apart."""
    N, K = w.shape
    assert N % 16 == 0 and K % 32 == 0
    return w.view(N // 16, 16, K // 32, 32).permute(0, 2, 1, 3).contiguous().view(N, K)


def pack_decode_tiles20(w):
    """Row-major [N, K] 16-bit weight → 20-row decode tiles [N/20][K/32][20][32] (sx_gemv w_layout 2): a 32-k slab of a 20-row
    group is 1280 contiguous bytes = the 1-KB MFMA operand tile of rows 0..15 followed by rows 16..19."""
    N, K = w.shape
    assert N % 20 == 0 and K % 32 == 0
    return w.view(N // 20, 20, K // 32, 32).permute(0, 2, 1, 3).contiguous().view(N, K)


def _fp8_row_order(codes):
    """[..., K] → [..., K/64, 64] with the 64 codes of a k-slab in the skinny GEMM's lane order: byte 16 g + 8 h + j holds
    k = 32 h + 8 g + j (g = 0..3 lane group, h = 0..1 32-k half, j = 0..7) — sx_gemv_args.w_dtype in include/seedx_hip.h."""
    K = codes.shape[-1]
    return codes.reshape(*codes.shape[:-1], K // 64, 2, 4, 8).transpose(-3, -2).reshape(*codes.shape[:-1], K // 64, 64)


def pack_decode_tiles_fp8(codes):
    """Row-major e4m3 codes uint8 [N, K] (quant.quantize_rows) → FP8 decode tiles [N/16][K/64][16][64]: a 64-k slab of 16 rows is one
    contiguous 1-KB tile, ONE 16-B load per lane and k-step (the 16-bit layout of pack_decode_tiles needs two)."""
    N, K = codes.shape
    assert codes.dtype == torch.uint8 and N % 16 == 0 and K % 64 == 0
    return _fp8_row_order(codes).view(N // 16, 16, K // 64, 64).permute(0, 2, 1, 3).contiguous()


def pack_decode_tiles20_fp8(codes):
    """Row-major e4m3 codes uint8 [N, K] → 20-row FP8 decode tiles [N/20][K/64][20][64] (sx_gemv w_layout 2): the 1-KB tile of rows
    0..15, then rows 16..19, per 64-k slab."""
    N, K = codes.shape
    assert codes.dtype == torch.uint8 and N % 20 == 0 and K % 64 == 0
    return _fp8_row_order(codes).view(N // 20, 20, K // 64, 64).permute(0, 2, 1, 3).contiguous()


def _fp4_row_order(codes):
    """Packed e2m1 codes [..., K/2] (byte i = k 2i | k 2i + 1 << 4) → [..., K/64, 32] with the 32 bytes of a k-slab in the skinny GEMM's
    lane order: byte 8 g + 4 h + i holds k = 32 h + 8 g + 2 i (low nibble) and k + 1 (g = 0..3 lane group, h = 0..1 32-k half,
    i = 0..3) — sx_gemv_args.w_block_scale in include/seedx_hip.h."""
    K2 = codes.shape[-1]
    return codes.reshape(*codes.shape[:-1], K2 // 32, 2, 4, 4).transpose(-3, -2).reshape(*codes.shape[:-1], K2 // 32, 32)


def pack_decode_tiles_fp4(codes):
    """Row-major packed e2m1 codes uint8 [N, K/2] (quant.quantize_blocks_mxfp4) → MXFP4 decode tiles [N/16][K/64][16][32]: a 64-k slab
    of 16 rows is one contiguous 512-B tile, ONE 8-B load per lane and k-step (dword h = the lane's eight k-slots of 32-k half h)."""
    N, K2 = codes.shape
    assert codes.dtype == torch.uint8 and N % 16 == 0 and K2 % 32 == 0
    return _fp4_row_order(codes).view(N // 16, 16, K2 // 32, 32).permute(0, 2, 1, 3).contiguous()


def pack_decode_tiles20_fp4(codes):
    """Row-major packed e2m1 codes uint8 [N, K/2] → 20-row MXFP4 decode tiles [N/20][K/64][20][32] (sx_gemv w_layout 2): the 512-B tile
    of rows 0..15, then rows 16..19, per 64-k slab."""
    N, K2 = codes.shape
    assert codes.dtype == torch.uint8 and N % 20 == 0 and K2 % 32 == 0
    return _fp4_row_order(codes).view(N // 20, 20, K2 // 32, 32).permute(0, 2, 1, 3).contiguous()


def pack_block_scales_fp4(scale, rows=16):
    """E8M0 block scales uint8 [N, K/32] (quant.quantize_blocks_mxfp4, rows in the order of the code matrix) → scale tiles
    [N/rows][K/64][rows][2], rows = 16 or 20 like the code tiles they belong to: byte h of (row, k-step t) is the scale of block 2 t + h."""
    N, B = scale.shape
    assert scale.dtype == torch.uint8 and rows in (16, 20) and N % rows == 0 and B % 2 == 0
    return scale.view(N // rows, rows, B // 2, 2).permute(0, 2, 1, 3).contiguous()


def unpack_decode_tiles_fp8(tiles):
    """FP8 decode tiles [N/rows][K/64][rows][64] (rows = 16: pack_decode_tiles_fp8, 20: pack_decode_tiles20_fp8; the shape says which) →
    the row-major e4m3 codes uint8 [N, K]: the host inverse of the packer, the reference sx_dequant_tiles is tested against."""
    assert tiles.dtype == torch.uint8 and tiles.dim() == 4 and tiles.shape[2] in (16, 20) and tiles.shape[3] == 64
    G, T, R, _ = tiles.shape
    rows = tiles.permute(0, 2, 1, 3).reshape(G * R, T, 4, 2, 8)           # byte 16 g + 8 h + j of a slab → [g][h][j]
    return rows.transpose(-3, -2).reshape(G * R, T * 64).contiguous()      # k = 32 h + 8 g + j


def unpack_decode_tiles_fp4(tiles):
    """MXFP4 decode tiles [N/rows][K/64][rows][32] (rows = 16 or 20) → the row-major packed e2m1 codes uint8 [N, K/2] (byte i = k 2i |
    k 2i + 1 << 4): the host inverse of pack_decode_tiles_fp4 / pack_decode_tiles20_fp4."""
    assert tiles.dtype == torch.uint8 and tiles.dim() == 4 and tiles.shape[2] in (16, 20) and tiles.shape[3] == 32
    G, T, R, _ = tiles.shape
    rows = tiles.permute(0, 2, 1, 3).reshape(G * R, T, 4, 2, 4)           # byte 8 g + 4 h + i of a slab → [g][h][i]
    return rows.transpose(-3, -2).reshape(G * R, T * 32).contiguous()      # byte 16 h + 4 g + i of the row's 32 bytes


def unpack_block_scales_fp4(scale_tiles):
    """E8M0 scale tiles [N/rows][K/64][rows][2] (rows = 16 or 20) → the block scales uint8 [N, K/32]: the inverse of pack_block_scales_fp4."""
    assert scale_tiles.dtype == torch.uint8 and scale_tiles.dim() == 4 and scale_tiles.shape[2] in (16, 20) and scale_tiles.shape[3] == 2
    G, T, R, _ = scale_tiles.shape
    return scale_tiles.permute(0, 2, 1, 3).reshape(G * R, T * 2).contiguous()


class WeightShape:
    """Shape and dtype of a weight whose only copy is its quantised decode tiles (LlamaForCausalLM(weight_residency="tiles")): what gemv
    takes as ``w`` beside w_fp8 / w_fp4. It owns no storage — a kernel that would read it is handed a null pointer and refuses."""
    __slots__ = ("shape", "dtype")

    def __init__(self, shape, dtype):
        self.shape, self.dtype = torch.Size(shape), dtype

    def numel(self):
        return self.shape[0] * self.shape[1]

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return 0


def dequant_tiles(w_fp8=None, w_fp4=None, dtype=torch.float16, out=None):
    """The row-major 16-bit [N, K] matrix of a weight held as decode tiles (sx_dequant_tiles; exact: every element is the value
    quant.dequantize_rows / dequantize_blocks_mxfp4 gives in ``dtype``). w_fp8 = (tiles, scale) / w_fp4 = (code_tiles, scale_tiles) as
    for gemv; the tile shape says 16- or 20-row. ``out``: a caller-owned contiguous buffer of ``dtype`` with at least N * K elements (the
    shared prefill scratch of the tiles residency): the matrix is written to its first N * K elements, nothing behind them is touched,
    and the returned tensor is a view of it. The caller orders its uses of ``out``: on ONE stream the GEMM that reads the view finishes
    before the next dequant_tiles overwrites it."""
    assert (w_fp8 is None) != (w_fp4 is None), "dequant_tiles: exactly one of w_fp8 / w_fp4"
    assert dtype in (torch.float16, torch.bfloat16)
    t, sc = w_fp8 if w_fp8 is not None else w_fp4
    rb = 64 if w_fp8 is not None else 32
    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == 4 and t.shape[2] in (16, 20) and t.shape[3] == rb
    N, K = t.shape[0] * t.shape[2], t.shape[1] * 64
    args = _lib.DequantTilesArgs()
    if w_fp8 is not None:
        assert sc.dtype == torch.float32 and sc.is_contiguous() and sc.shape == (N,) and sc.device == t.device
        args.w_dtype, args.w_scale = _lib.SX_FP8_E4M3, sc.data_ptr()
    else:
        assert sc.dtype == torch.uint8 and sc.is_contiguous() and sc.shape == t.shape[:3] + (2,) and sc.device == t.device
        args.w_dtype, args.w_block_scale = _lib.SX_FP4_E2M1, sc.data_ptr()
    if out is None:
        out = torch.empty(N * K, dtype=dtype, device=t.device)
    assert out.dtype == dtype and out.is_contiguous() and out.device == t.device and out.numel() >= N * K, \
        "dequant_tiles: out must be a contiguous buffer of the target dtype with at least N * K elements"
    args.tiles, args.out, args.out_bytes = t.data_ptr(), out.data_ptr(), out.numel() * out.element_size()
    args.w_layout, args.N, args.K, args.dtype = (1 if t.shape[2] == 16 else 2), N, K, _DT[dtype]
    check(_lib.load().sx_dequant_tiles(C.byref(args), _stream()), "sx_dequant_tiles")
    return out.view(-1)[:N * K].view(N, K)


class Tiled16:
    """A [rows <= 32, cols] 16-bit activation of the decode step held as MFMA operand tiles [rows/16][cols/32][16][32] (SX_TILED16
    in include/seedx_hip.h): what the skinny GEMM reads with one contiguous 1-KB load per operand. Rows 16..31 (lock-step batches
    above 16) are a second block of tiles behind the first; rows >= `rows` of the last block are padding."""
    __slots__ = ("t", "rows", "cols", "planes")

    def __init__(self, rows, cols, dtype, device, planes=1):
        """planes = 2: [2 planes][row blocks][cols/32][16][32] — the hi plane's row blocks, then the lo plane's, of an fp32-grade activation
        (sx_gemv x_planes = 2; 17..32 rows = two row blocks per plane, round 6)."""
        assert rows <= 32 and cols % 32 == 0 and planes in (1, 2)
        nb = planes * ((rows + 15) // 16)
        self.t, self.rows, self.cols, self.planes = torch.empty((nb, cols // 32, 16, 32), dtype=dtype, device=device), rows, cols, planes

    @property
    def dtype(self):
        return self.t.dtype

    def dense(self):
        """[rows, cols] row-major copy (tests); planes = 2: fp32 hi + lo."""
        nb = self.t.shape[0]
        d = self.t.permute(0, 2, 1, 3).reshape(nb * 16, self.cols)
        if self.planes == 2:
            half = (nb // 2) * 16
            return d[:self.rows].float() + d[half:half + self.rows].float()
        return d[:self.rows].contiguous()


def _mfma_shape(N, K):
    """The weight shapes sx_gemv's MFMA skinny kernel takes (its tiled operands and 9..32 rows exist on that kernel only)."""
    return K % 64 == 0 and K >= 256 and N % 32 == 0


def gemv(x, w, residual=None, act=None, glu=False, out_dtype=None, w_tiles=None, y_tiled=False, workspace=None,
         emit_norm=False, ssq_in=None, w_tiles20=None, planes_out=False, norm_gamma=None, w_fp8=None, w_fp4=None, addend=None):
    """w_tiles: the same weight in the decode layout (pack_decode_tiles); used instead of w when the MFMA path runs.
    x may be a Tiled16 (then w_tiles is required); y_tiled returns the 16-bit result as a Tiled16 for the next gemv.
    workspace: zero-initialised uint8 scratch enabling split-K over workgroups for shapes that need it (sx_gemv_args.workspace).
    RMSNorm fold (sx_gemv_args.x16_out / row_ssq_*; MFMA path, tiled x): ``emit_norm`` (fp32 residual outputs) → returns
    (y, x16, ssq): y also as 16-bit operand tiles and the rows' sums of squares per workgroup; ``ssq_in`` = (ssq, dim, eps) of
    the producer → the accumulators are scaled by rsqrt(sum(ssq) / dim + eps) (gamma lives in this launch's weights).
    w_tiles20: the weight as 20-row decode tiles (pack_decode_tiles20) instead of w_tiles: one workgroup per 20 rows.
    planes_out (M <= 16): the tiled 16-bit result (y_tiled) or the emit_norm x16 is written as two planes (Tiled16 planes = 2) for a next
    gemv with fp32-grade x; norm_gamma (with emit_norm): x16 = planes of y * gamma — the NEXT RMSNorm's weight on the activation side, so
    the projection behind the norm keeps exact weights and only applies rstd (ssq_in).
    w_fp8 = (tiles, scale): the weight as e4m3 codes in FP8 decode tiles (pack_decode_tiles_fp8 → 16-row, pack_decode_tiles20_fp8 →
    20-row; the shape says which) with its fp32 row scales [N], in the row order of ``w``; replaces w_tiles / w_tiles20. ``w`` (the
    dequantised 16-bit matrix) only gives shape and dtype. MFMA path only: any other shape is an error, never a fall-back.
    w_fp4 = (code_tiles, scale_tiles): the weight as MXFP4 decode tiles (pack_decode_tiles_fp4 / pack_decode_tiles20_fp4; the shape says
    which) with its E8M0 block-scale tiles (pack_block_scales_fp4 with the same rows); replaces w_tiles / w_tiles20 in the same way.
    With w_fp8 / w_fp4, ``w`` may be a WeightShape: shape and dtype without storage (the tiles are the weight's only copy).
    addend = delta or (delta, sel, n_adapters): fp32 [M, N] (columns in the row order of the weight as passed) added to the summed
    accumulators BEFORE activation / GLU / residual (sx_gemv_args.addend: the unmerged LoRA delta of lora_expand); with sel (int32 [M] on
    the device) only the rows whose sel is in [0, n_adapters) take it, every other row keeps the bits of a launch without an addend. MFMA
    path only: an error on the VALU path, never a fall-back."""
    lib = _lib.load()
    xt = isinstance(x, Tiled16)
    assert not isinstance(w, WeightShape) or w_fp8 is not None or w_fp4 is not None, "gemv: a weight without storage needs its FP8 / MXFP4 tiles"
    if xt:
        M, K = x.rows, x.cols
        assert x.dtype == w.dtype and (x.planes == 2 or w_tiles is not None or w_tiles20 is not None or w_fp8 is not None or w_fp4 is not None)
    else:
        assert x.dim() == 2 and x.is_contiguous() and w.is_contiguous() and x.dtype == w.dtype
        M, K = x.shape
    N = w.shape[0]
    n_out = N // 2 if glu else N
    out_dtype = out_dtype or x.dtype
    dev = x.t.device if xt else x.device
    if y_tiled:
        yt = Tiled16(M, n_out, out_dtype, dev, planes=2 if planes_out else 1)
        y = yt.t
    else:
        y = torch.empty((M, n_out), dtype=out_dtype, device=dev)
    args = GemvArgs()
    args.x, args.W, args.y = (x.t if xt else x).data_ptr(), w.data_ptr(), y.data_ptr()
    args.x_layout = 1 if xt else 0
    args.x_planes = x.planes if xt else 1
    if workspace is not None:
        args.workspace, args.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    if residual is not None:
        assert residual.dtype == torch.float32 and residual.is_contiguous() and residual.shape == (M, n_out)
        args.residual = residual.data_ptr()
    args.M, args.N, args.K = M, N, K
    args.dtype, args.out_dtype, args.act, args.glu = _DT[x.dtype], _DT[out_dtype], ACT[act], 1 if glu else 0
    if y_tiled:
        args.out_dtype |= _lib.SX_TILED16
    if planes_out:
        assert y_tiled or emit_norm
        args.out_planes = 1
    if w_tiles is not None and (xt or y_tiled or M >= 5) and _mfma_shape(N, K):
        assert w_tiles.shape == w.shape and w_tiles.dtype == w.dtype and w_tiles.is_contiguous()
        args.W, args.w_layout = w_tiles.data_ptr(), 1
    if w_tiles20 is not None and not glu and (xt or y_tiled or M >= 5) and _mfma_shape(N, K) and N % 20 == 0:
        assert w_tiles20.shape == w.shape and w_tiles20.dtype == w.dtype and w_tiles20.is_contiguous()
        args.W, args.w_layout = w_tiles20.data_ptr(), 2
    if w_fp8 is not None:
        t8, sc = w_fp8
        assert t8.dtype == torch.uint8 and t8.is_contiguous() and t8.dim() == 4 and t8.shape[2] in (16, 20) and t8.shape[3] == 64
        assert t8.shape[0] * t8.shape[2] == N and t8.shape[1] * 64 == K and t8.device == dev, "FP8 tiles do not match the weight's shape"
        assert sc.dtype == torch.float32 and sc.is_contiguous() and sc.shape == (N,) and sc.device == dev
        args.W, args.w_layout = t8.data_ptr(), 1 if t8.shape[2] == 16 else 2
        args.w_dtype, args.w_scale = _lib.SX_FP8_E4M3, sc.data_ptr()
    if w_fp4 is not None:
        assert w_fp8 is None
        t4, sc = w_fp4
        assert t4.dtype == torch.uint8 and t4.is_contiguous() and t4.dim() == 4 and t4.shape[2] in (16, 20) and t4.shape[3] == 32
        assert t4.shape[0] * t4.shape[2] == N and t4.shape[1] * 64 == K and t4.device == dev, "MXFP4 tiles do not match the weight's shape"
        assert sc.dtype == torch.uint8 and sc.is_contiguous() and sc.shape == t4.shape[:3] + (2,) and sc.device == dev
        args.W, args.w_layout = t4.data_ptr(), 1 if t4.shape[2] == 16 else 2
        args.w_dtype, args.w_block_scale = _lib.SX_FP4_E2M1, sc.data_ptr()
    x16 = ssq = None
    if emit_norm:
        assert args.w_layout in (1, 2) and out_dtype == torch.float32 and not glu and not y_tiled
        x16 = Tiled16(M, n_out, w.dtype, dev, planes=2 if planes_out else 1)
        if norm_gamma is not None:
            assert norm_gamma.dtype == torch.float32 and norm_gamma.is_contiguous() and norm_gamma.numel() == n_out
            args.x16_gamma = norm_gamma.data_ptr()
        ssq = torch.empty((16 * ((M + 15) // 16), lib.sx_gemv_ssq_parts(N, 0, args.w_layout)), dtype=torch.float32, device=dev)   # [row][workgroup]
        args.x16_out, args.row_ssq_out = x16.t.data_ptr(), ssq.data_ptr()
    if ssq_in is not None:
        t, dim, eps = ssq_in
        assert args.w_layout == 1 and t.dtype == torch.float32 and t.is_contiguous() and t.shape[0] == 16 * ((M + 15) // 16)
        args.row_ssq_in, args.ssq_in_parts, args.ssq_dim, args.ssq_eps = t.data_ptr(), t.shape[1], int(dim), float(eps)
    if addend is not None:
        d, asel, n_ad = addend if isinstance(addend, tuple) else (addend, None, 0)
        assert d.dtype == torch.float32 and d.is_contiguous() and d.shape == (M, N) and d.device == dev
        args.addend = d.data_ptr()
        if asel is not None:
            assert asel.dtype == torch.int32 and asel.is_contiguous() and asel.numel() >= M and asel.device == dev and n_ad >= 1
            args.addend_sel, args.addend_n = asel.data_ptr(), int(n_ad)
    check(lib.sx_gemv(C.byref(args), _stream()), "sx_gemv")
    out = yt if y_tiled else y
    return (out, x16, ssq) if emit_norm else out


def linear(x, w, **kw):
    """Dispatch M <= 16 rows to the weight-streaming GEMV / skinny GEMM (when the epilogue allows), else the MFMA GEMM."""
    M, K, N = x.shape[0], x.shape[1], w.shape[0]
    # 9..16 rows only exist on the MFMA skinny kernel (K % 64 == 0, K >= 256, N % 32 == 0); other shapes keep the tiled GEMM
    skinny_ok = M <= 8 or _mfma_shape(N, K)
    if M <= 16 and skinny_ok and kw.get("bias") is None and kw.get("bias2d") is None and not kw.get("res_mod") \
            and kw.get("out") is None and not kw.get("n_valid"):
        res = kw.get("residual")
        if res is None or res.is_contiguous():
            return gemv(x, w, residual=res, act=kw.get("act"), glu=kw.get("glu", False), out_dtype=kw.get("out_dtype"),
                        w_tiles=kw.get("w_tiles"))
    kw.pop("w_tiles", None)
    return gemm(x, w, **kw)


# ---------------------------------------------------------------------------------------------------------
# Norms
# ---------------------------------------------------------------------------------------------------------
def layernorm(x, gamma, beta, eps, out_dtype, rms=False, tiled=False):
    """tiled (rows <= 32, 16-bit out): the result as a Tiled16 — the decode step's norms feed skinny GEMMs only."""
    lib = _lib.load()
    assert x.is_contiguous()
    cols = x.shape[-1]
    rows = x.numel() // cols
    if tiled:
        yt = Tiled16(rows, cols, out_dtype, x.device)
        y, code = yt.t, _DT[out_dtype] | _lib.SX_TILED16
    else:
        y, code = torch.empty(x.shape, dtype=out_dtype, device=x.device), _DT[out_dtype]
    check(lib.sx_layernorm(_p(x), _DT[x.dtype], _p(y), code, _p(_f32c(gamma)), _p(_f32c(beta)), rows, cols,
                           float(eps), 1 if rms else 0, _stream()), "sx_layernorm")
    return yt if tiled else y


def rmsnorm(x, gamma, eps, out_dtype, tiled=False):
    return layernorm(x, gamma, None, eps, out_dtype, rms=True, tiled=tiled)


def groupnorm(x, gamma, beta, groups, eps, silu, out_dtype, want_raw=False, x2=None, comm=None, hw_total=None, planes=False,
              stats=None):
    """x: fp32 [B, HW, C] (NHWC). Returns y (16-bit) and optionally a 16-bit raw copy of x.
    stats: GnStats filled by x's producer (``ready``): only the apply pass runs (single rank, no x2).
    planes: True / 3: y (and raw) come out as bf16 [B, HW, 3C] rows [hi | hi | lo] (split_bf16 role "a") instead; 2: as fp16
    [B, HW, 2C] rows [hi | lo] (split16's layout: the operand of a conv whose fp16 weight rows are duplicated per tap).
    x2: optional second fp32 [B, HW, C2] tensor — the op then runs over the channel concatenation [x | x2] (never built).
    comm / hw_total: x holds only this rank's pixel rows of images with hw_total rows (seqpar.py): the fp64 statistics are
    all-reduced over the ranks between the statistics pass and the apply pass."""
    lib = _lib.load()
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 3
    B, HW, C1 = x.shape
    Cc = C1
    if x2 is not None:
        assert x2.dtype == torch.float32 and x2.is_contiguous() and x2.shape[:2] == (B, HW)
        Cc = C1 + x2.shape[2]
    if planes == 2:
        out_dtype, code, cols = torch.float16, _lib.SX_F16X2, 2 * Cc
    elif planes:
        out_dtype, code, cols = torch.bfloat16, _lib.SX_BF16X3, 3 * Cc
    else:
        code, cols = _DT[out_dtype], Cc
    y = torch.empty((B, HW, cols), dtype=out_dtype, device=x.device)
    raw = torch.empty((B, HW, cols), dtype=out_dtype, device=x.device) if want_raw else None
    if stats is not None and stats.ready and x2 is None and (comm is None or comm.world == 1):
        assert stats.groups == groups and stats.rows == HW and stats.buf.numel() == B * groups * 2
        check(lib.sx_groupnorm_sp(_p(x), None, C1, _p(y), _p(raw), code, _p(_f32c(gamma)), _p(_f32c(beta)), _p(stats.buf), B, HW, HW,
                                  Cc, groups, float(eps), 1 if silu else 0, 2, _stream()), "sx_groupnorm_sp(apply, fused statistics)")
        return (y, raw) if want_raw else y
    stats = torch.empty((B, groups, 2), dtype=torch.float64, device=x.device)
    if comm is None or comm.world == 1:
        check(lib.sx_groupnorm2(_p(x), _p(x2), C1, _p(y), _p(raw), code, _p(_f32c(gamma)), _p(_f32c(beta)), _p(stats),
                                B, HW, Cc, groups, float(eps), 1 if silu else 0, _stream()), "sx_groupnorm")
    else:
        args = (_p(x), _p(x2), C1, _p(y), _p(raw), code, _p(_f32c(gamma)), _p(_f32c(beta)), _p(stats), B, HW,
                int(hw_total), Cc, groups, float(eps), 1 if silu else 0)
        check(lib.sx_groupnorm_sp(*args, 1, _stream()), "sx_groupnorm_sp(stats)")
        comm.all_reduce(stats)
        check(lib.sx_groupnorm_sp(*args, 2, _stream()), "sx_groupnorm_sp(apply)")
    return (y, raw) if want_raw else y


def softmax_rows(x, scale, out_dtype):
    """softmax(scale · x) over the last dim; x fp32 [R, C] (row stride free) → 16-bit (or fp32) [R, C]."""
    lib = _lib.load()
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    R, Cc = x.shape
    y = torch.empty((R, Cc), dtype=out_dtype, device=x.device)
    check(lib.sx_softmax_rows(_p(x), x.stride(0), _p(y), y.stride(0), R, Cc, float(scale), _DT[out_dtype], _stream()),
          "sx_softmax_rows")
    return y


# ---------------------------------------------------------------------------------------------------------
# Attention
# ---------------------------------------------------------------------------------------------------------
def _bshd_strides(t):
    assert t.dim() == 4 and t.stride(3) == 1, "expected a [B, S, H, D] view with unit stride on D"
    return t.stride(0), t.stride(1), t.stride(2)


def attention(q, k, v, scale, causal=False, out=None):
    """Flash attention on MFMA. q: [B, Sq, H, D] view, k/v: [B, Skv, H, D] views (any strides that are multiples of 8
    elements, unit D stride). V is read in this natural layout (the kernel transposes fragments with ds_read_b64_tr_b16).
    Returns [B, Sq, H*D] 16-bit."""
    lib = _lib.load()
    B, Sq, H, D = q.shape
    Skv = k.shape[1]
    assert k.shape == (B, Skv, H, D) and v.shape == (B, Skv, H, D) and q.dtype == k.dtype == v.dtype
    if out is None:
        out = torch.empty((B, Sq, H * D), dtype=q.dtype, device=q.device)
    a = AttnArgs()
    a.Q, a.K, a.V, a.O = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    a.B, a.H, a.Sq, a.Skv, a.D = B, H, Sq, Skv, D
    a.q_batch_stride, a.q_row_stride, a.q_head_stride = _bshd_strides(q)
    a.k_batch_stride, a.k_row_stride, a.k_head_stride = _bshd_strides(k)
    a.v_batch_stride, a.v_row_stride, a.v_head_stride = _bshd_strides(v)
    a.o_batch_stride, a.o_row_stride = out.stride(0), out.stride(1)
    a.scale = float(scale)
    a.causal = 1 if causal else 0
    a.dtype = _DT[q.dtype]
    check(lib.sx_attention(C.byref(a), _stream()), "sx_attention")
    return out


def attention_small(q, k, v, scale):
    lib = _lib.load()
    B, Sq, H, D = q.shape
    Skv = k.shape[1]
    out = torch.empty((B, Sq, H * D), dtype=q.dtype, device=q.device)
    a = AttnSmallArgs()
    a.Q, a.K, a.V, a.O = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    a.B, a.H, a.Sq, a.Skv, a.D = B, H, Sq, Skv, D
    a.q_batch_stride, a.q_row_stride, a.q_head_stride = _bshd_strides(q)
    a.k_batch_stride, a.k_row_stride, a.k_head_stride = _bshd_strides(k)
    a.v_batch_stride, a.v_row_stride, a.v_head_stride = _bshd_strides(v)
    a.o_batch_stride, a.o_row_stride = out.stride(0), out.stride(1)
    a.scale = float(scale)
    a.dtype = _DT[q.dtype]
    check(lib.sx_attention_small(C.byref(a), _stream()), "sx_attention_small")
    return out


def attn_decode(q, kcache, vcache, ctx_len_dev, scale, nsplit=8):
    """q: [H, D] 16-bit; caches [H, Tmax, D]; ctx_len_dev: int32 device scalar. Returns [1, H*D]."""
    lib = _lib.load()
    H, D = q.shape
    Tmax = kcache.shape[1]
    out = torch.empty((1, H * D), dtype=q.dtype, device=q.device)
    scratch = torch.empty((H, nsplit, D + 2), dtype=torch.float32, device=q.device)
    check(lib.sx_attn_decode(_p(q), _p(kcache), _p(vcache), _p(out), _p(scratch), _p(ctx_len_dev), H, D, Tmax, nsplit,
                             float(scale), _DT[q.dtype], _stream()), "sx_attn_decode")
    return out


# ---------------------------------------------------------------------------------------------------------
# fp32-grade activations of the Llama decoder (LlamaForCausalLM(precise=True); csrc/precise.hip)
# ---------------------------------------------------------------------------------------------------------
def _planes_out(rows, cols, dtype, device, tiled):
    if tiled:
        t = Tiled16(rows, cols, dtype, device, planes=2)
        return t, t.t, _DT[dtype] | _lib.SX_TILED16
    y = torch.empty((rows, 2 * cols), dtype=dtype, device=device)
    return y, y, _DT[dtype]


def split16(x, dtype, tiled=False):
    """fp32 [rows, cols] → its two 16-bit planes x = hi + lo: [rows, 2*cols] = [hi | lo] (gemm a_planes = 2), or with ``tiled`` a
    two-block Tiled16 (gemv)."""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    rows, cols = x.shape
    ret, buf, code = _planes_out(rows, cols, dtype, x.device, tiled)
    check(_lib.load().sx_split16(_p(x), x.stride(0), _p(buf), rows, cols, code, _stream()), "sx_split16")
    return ret


def rmsnorm_planes(x, gamma, eps, dtype, tiled=False, want_f32=False, want_planes=True):
    """LlamaRMSNorm in fp32 → (planes of y or None, y fp32 or None)."""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous()
    rows, cols = x.shape
    ret = buf = None
    code = _DT[dtype]
    if want_planes:
        ret, buf, code = _planes_out(rows, cols, dtype, x.device, tiled)
    y32 = torch.empty_like(x) if want_f32 else None
    check(_lib.load().sx_rmsnorm_planes(_p(x), _p(_f32c(gamma)), _p(y32), _p(buf), rows, cols, float(eps), code, _stream()),
          "sx_rmsnorm_planes")
    return ret, y32


def rmsnorm_planes_sel(x, gamma, gamma_table, sel, eps, dtype, tiled=False, want_f32=False, want_planes=True):
    """rmsnorm_planes with one gamma per adapter: row m uses gamma_table[sel[m]] (fp32 [n_adapters, cols]) when sel[m] (int32, device) is
    in [0, n_adapters), else ``gamma`` — every row bit-identical to rmsnorm_planes with the gamma it selected (sx_rmsnorm_planes_sel)."""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous()
    rows, cols = x.shape
    assert sel.dtype == torch.int32 and sel.is_contiguous() and sel.numel() >= rows and sel.device == x.device
    n_ad = 0
    if gamma_table is not None:
        assert gamma_table.dtype == torch.float32 and gamma_table.is_contiguous() and gamma_table.dim() == 2 and gamma_table.shape[1] == cols
        n_ad = gamma_table.shape[0]
    ret = buf = None
    code = _DT[dtype]
    if want_planes:
        ret, buf, code = _planes_out(rows, cols, dtype, x.device, tiled)
    y32 = torch.empty_like(x) if want_f32 else None
    check(_lib.load().sx_rmsnorm_planes_sel(_p(x), _p(_f32c(gamma)), _p(gamma_table), _p(sel), n_ad, _p(y32), _p(buf), rows, cols,
                                            float(eps), code, _stream()), "sx_rmsnorm_planes_sel")
    return ret, y32


def lora_shrink(x, A, sel, out=None):
    """t[m, i] = sum_k A[sel[m], i, k] * (hi + lo)[m, k] in fp32 (sx_lora_shrink; the rule: lora.lora_delta_ref). x: the planes of an
    fp32-grade activation — a two-plane Tiled16 (the decode step's x operand, <= 32 rows) or rows [M, 2K] = [hi | lo] (prefill). A: 16-bit
    [n_adapters, S*R, K]; sel: int32 [M] on the device. Rows whose index is outside [0, n_adapters) are base rows: their t is not written."""
    xt = isinstance(x, Tiled16)
    if xt:
        assert x.planes == 2
        M, K, xb, code = x.rows, x.cols, x.t, _DT[x.dtype] | _lib.SX_TILED16
    else:
        assert x.dim() == 2 and x.is_contiguous() and x.shape[1] % 2 == 0
        M, K, xb, code = x.shape[0], x.shape[1] // 2, x, _DT[x.dtype]
    assert A.dim() == 3 and A.is_contiguous() and A.dtype == xb.dtype and A.shape[2] == K and A.device == xb.device
    assert sel.dtype == torch.int32 and sel.is_contiguous() and sel.numel() >= M and sel.device == xb.device
    n_ad, SR = A.shape[0], A.shape[1]
    if out is None:
        out = torch.empty((M, SR), dtype=torch.float32, device=xb.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == (M, SR)
    check(_lib.load().sx_lora_shrink(_p(xb), _p(A), _p(sel), _p(out), M, K, SR, n_ad, code, _stream()), "sx_lora_shrink")
    return out


def lora_expand(t, B, seg, scale, sel, out=None):
    """delta[m, n] = scale[sel[m]] * sum_j B[sel[m], n, j] * t[m, seg[n // 16] * R + j] in fp32 (sx_lora_expand). B: 16-bit
    [n_adapters, N, R], rows in the order of the projection's weight AS PACKED; seg: int32 [N / 16]; scale: fp32 [n_adapters]. Base rows of
    ``out`` (fp32 [M, N]; a fresh buffer is uninitialised) are not written: hand the result to gemv(addend=(delta, sel, n_adapters))."""
    assert t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous()
    assert B.dim() == 3 and B.is_contiguous() and B.dtype in (torch.float16, torch.bfloat16) and B.device == t.device
    n_ad, N, R = B.shape
    M = t.shape[0]
    assert t.shape[1] % R == 0
    S = t.shape[1] // R
    assert seg.dtype == torch.int32 and seg.is_contiguous() and seg.numel() == N // 16 and seg.device == t.device
    assert scale.dtype == torch.float32 and scale.is_contiguous() and scale.numel() == n_ad and scale.device == t.device
    assert sel.dtype == torch.int32 and sel.is_contiguous() and sel.numel() >= M and sel.device == t.device
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=t.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == (M, N)
    check(_lib.load().sx_lora_expand(_p(t), _p(B), _p(seg), _p(scale), _p(sel), _p(out), M, N, R, S, n_ad, _DT[B.dtype], _stream()),
          "sx_lora_expand")
    return out


def _kv_scales_ok(kv_scales, kcache, vcache):
    """The FP8 cache's tensors: codes uint8 [G, H, Tmax, 128] and one fp32 scale per row [G, H, Tmax], k and v laid out alike."""
    ks, vs = kv_scales
    assert kcache.dtype == torch.uint8 and vcache.dtype == torch.uint8 and kcache.shape[3] == 128
    assert ks.dtype == torch.float32 and vs.dtype == torch.float32 and ks.shape == kcache.shape[:3] and vs.shape == ks.shape \
        and ks[0].is_contiguous() and vs.stride() == ks.stride()
    return ks, vs


def _paged_ok(paged, kcache, vcache, G, H, D):
    """The paged cache's tensors: pools [n_pages + 1, H, page size, 128] (k fp32; v fp32 or 16-bit) and ``paged`` = (page table int32
    [G, ceil(Tmax / page size)] on the device, Tmax). Returns (table, Tmax, page shift, n_pages)."""
    table, Tmax = paged
    ps = kcache.shape[2]
    assert kcache.dim() == 4 and kcache.is_contiguous() and vcache.is_contiguous() and vcache.shape == kcache.shape
    assert kcache.shape[0] >= 2 and kcache.shape[1] == H and kcache.shape[3] == D and ps in (32, 64, 128), "pools are [n_pages + 1, H, 32 | 64 | 128, D]"
    assert table.dtype == torch.int32 and table.is_contiguous() and table.device == kcache.device and table.dim() == 2
    assert table.shape[0] >= G and table.shape[1] == (int(Tmax) + ps - 1) // ps, "page table: int32 [G, ceil(Tmax / page size)]"
    return table, int(Tmax), ps.bit_length() - 1, kcache.shape[0] - 1


def rope_kv_append_f32(qkv, kcache, vcache, cos_tab, sin_tab, pos_dev, G, T, H, D, table_dtype, kv_scales=None, kv_emulate=False,
                       paged=None):
    """qkv fp32 [G*T, 3HD] (q rotated in place); caches [G, H, Tmax, D]: k fp32, v fp32 or — the mixed cache — the model's 16-bit dtype
    (= table_dtype); pos_dev int32 [G].
    paged=(page table, Tmax): the paged cache — kcache / vcache are the page pools [n_pages + 1, H, page size, D] and the row of position
    p of sequence g goes to page table[g, p // page size] (entry 0: nothing is written). Row g of the table belongs to pos_dev[g].
    kv_scales=(kscale, vscale) fp32 [G, H, Tmax]: the FP8 cache — kcache / vcache are uint8 e4m3 codes, every appended row is quantised
    with one power-of-two scale (quant.quantize_kv_rows' rule). kv_emulate: fp32 caches receive the dequantised values instead (the
    bit-reference twin of the FP8 cache)."""
    assert qkv.dtype == torch.float32 and qkv.is_contiguous() and qkv.shape == (G * T, 3 * H * D)
    if paged is not None:
        assert kv_scales is None and not kv_emulate, "the paged cache has no FP8 form"
        table, Tmax, shift, n_pages = _paged_ok(paged, kcache, vcache, G, H, D)
        assert kcache.dtype == torch.float32 and vcache.dtype in (torch.float32, table_dtype)
        check(_lib.load().sx_rope_kv_append_f32_paged(_p(qkv), _p(kcache), _p(vcache), 0 if vcache.dtype == torch.float32 else 1, _p(cos_tab),
                                                      _p(sin_tab), _p(pos_dev), _p(table), G, T, H, D, Tmax, shift, n_pages, kcache.stride(0),
                                                      _DT[table_dtype], _stream()), "sx_rope_kv_append_f32_paged")
        return
    assert kcache.dim() == 4 and kcache.shape[0] == G and kcache[0].is_contiguous() and vcache.stride() == kcache.stride()
    if kv_scales is not None or kv_emulate:
        assert not (kv_scales is not None and kv_emulate)
        if kv_emulate:
            assert kcache.dtype == torch.float32 and vcache.dtype == torch.float32
            ks = vs = None
        else:
            ks, vs = _kv_scales_ok(kv_scales, kcache, vcache)
        check(_lib.load().sx_rope_kv_append_f32_q8(_p(qkv), _p(kcache), _p(vcache), _p(ks), _p(vs), _p(cos_tab), _p(sin_tab), _p(pos_dev),
                                                   G, T, H, D, kcache.shape[2], kcache.stride(0), 0 if ks is None else ks.stride(0),
                                                   _DT[table_dtype], 1 if kv_emulate else 0, _stream()), "sx_rope_kv_append_f32_q8")
        return
    assert kcache.dtype == torch.float32 and vcache.dtype in (torch.float32, table_dtype)
    fn = "sx_rope_kv_append_f32" if vcache.dtype == torch.float32 else "sx_rope_kv_append_f32_v16"
    check(getattr(_lib.load(), fn)(_p(qkv), _p(kcache), _p(vcache), _p(cos_tab), _p(sin_tab), _p(pos_dev), G, T, H, D,
                                   kcache.shape[2], kcache.stride(0), _DT[table_dtype], _stream()), fn)


def attention_f32(qkv, kcache, vcache, pos_dev, G, T, H, D, scale, dtype, tiled=False, nsplit=1, scratch=None, rope=None, kv_scales=None,
                  kv_emulate=False, paged=None):
    """Causal fp32 attention of a T-token chunk per sequence over the fp32 cache (row t sees keys 0 .. pos[g] + t); q = the rotated
    head rows at the front of qkv's rows. Returns the planes of the context [G*T, H*D] (see split16).
    rope=(cos, sin) (T == 1, D == 128): qkv holds the UNROTATED q | k | v rows of the new token; the launch rotates q and k, appends k / v
    to the caches at pos[g] and attends — rope_kv_append_f32 + attention_f32 in one launch per layer.
    rope with 2 <= T <= 8 (G*T <= 32) is the VERIFY form of speculative decoding: rows g*T + t at positions pos[g] + t, bit for bit what T
    successive T = 1 calls with the same nsplit give (planes, k rows, v rows); pos[g] < 0 idles the whole slot. No FP8 cache.
    kv_scales=(kscale, vscale): the FP8 cache (uint8 codes + row scales, see rope_kv_append_f32) — the same bits as this call on a cache
    holding the dequantised values. kv_emulate (with rope): fp32 caches, the new token's rows quantised and dequantised on append.
    paged=(page table, Tmax): the paged cache (see rope_kv_append_f32) — the same bits as this call on contiguous caches holding the same
    rows. The library refuses the forms that read no table (D != 128, the FP8 cache, the verify form)."""
    assert qkv.dtype == torch.float32 and qkv.is_contiguous() and qkv.shape[0] == G * T and qkv.shape[1] >= H * D
    a = _lib.AttnF32Args()
    Tmax = kcache.shape[2]
    if paged is not None:
        table, Tmax, a.page_shift, a.n_pages = _paged_ok(paged, kcache, vcache, G, H, D)
        a.page_table, a.page_stride = _p(table), kcache.stride(0)
    else:
        assert kcache.shape[0] == G
    assert kcache.shape[1] == H and kcache.shape[3] == D and vcache.stride() == kcache.stride()
    ret, buf, code = _planes_out(G * T, H * D, dtype, qkv.device, tiled)
    if kv_scales is not None:
        assert not kv_emulate
        ks, vs = _kv_scales_ok(kv_scales, kcache, vcache)
        a.kv_fp8, a.k_scale, a.v_scale, a.scale_seq_stride = 1, _p(ks), _p(vs), ks.stride(0)
    else:
        assert kcache.dtype == torch.float32 and vcache.dtype in ((torch.float32,) if kv_emulate else (torch.float32, dtype))
        a.kv_fp8 = 2 if kv_emulate else 0
    a.q, a.kcache, a.vcache, a.out, a.pos0_dev = _p(qkv), _p(kcache), _p(vcache), _p(buf), _p(pos_dev)
    a.q_row_stride, a.cache_seq_stride = qkv.stride(0), kcache.stride(0)
    a.G, a.T, a.H, a.D, a.Tmax, a.dtype, a.scale, a.causal = G, T, H, D, Tmax, code, float(scale), 1
    a.v16 = 0 if vcache.dtype in (torch.float32, torch.uint8) else 1
    verify = rope is not None and T > 1   # speculative decoding: T = K + 1 rows per sequence, always split + combine (nsplit >= 1)
    if (nsplit > 1 and T == 1) or verify:  # decode step of few sequences: key splits (scratch: fp32 [G*T, H, nsplit, D + 2])
        if scratch is None:
            scratch = torch.empty((G * T, H, nsplit, D + 2), dtype=torch.float32, device=qkv.device)
        assert scratch.dtype == torch.float32 and scratch.numel() >= G * T * H * nsplit * (D + 2)
        a.nsplit, a.scratch = nsplit, _p(scratch)
    if rope is not None:
        assert 1 <= T <= 8 and D == 128 and qkv.shape[1] == 3 * H * D
        cos, sin = rope
        a.rope_cos, a.rope_sin = _p(cos), _p(sin)
        a.k_new, a.v_new = qkv.data_ptr() + 4 * H * D, qkv.data_ptr() + 8 * H * D
    check(_lib.load().sx_attention_f32(C.byref(a), _stream()), "sx_attention_f32")
    return ret


def attention_f32_full(q, k, v, scale, dtype):
    """Non-causal fp32 attention (fp32 FMA arithmetic and softmax): q [B, Sq, H, D], k / v [B, Skv, H, D] fp32 views with unit D stride
    (e.g. slices of one fused projection output). Returns the planes of the context [B*Sq, H*D] (split16's row layout)."""
    B, Sq, H, D = q.shape
    Skv = k.shape[1]
    assert q.dtype == k.dtype == v.dtype == torch.float32 and k.shape == (B, Skv, H, D) and v.shape == k.shape
    assert q.stride(3) == 1 and q.stride(2) == D and q.stride(0) == Sq * q.stride(1), "q rows must be [B*Sq] rows of H*D heads"
    assert k.stride(3) == 1 and v.stride() == k.stride()
    ret, buf, code = _planes_out(B * Sq, H * D, dtype, q.device, False)
    a = _lib.AttnF32Args()
    a.q, a.kcache, a.vcache, a.out, a.pos0_dev = _p(q), _p(k), _p(v), _p(buf), None
    a.q_row_stride, a.cache_seq_stride, a.kv_row_stride, a.kv_head_stride = q.stride(1), k.stride(0), k.stride(1), k.stride(2)
    a.G, a.T, a.H, a.D, a.Tmax, a.dtype, a.scale, a.causal = B, Sq, H, D, Skv, code, float(scale), 0
    check(_lib.load().sx_attention_f32(C.byref(a), _stream()), "sx_attention_f32")
    return ret


def linear_planes(x32, w, w_tiles=None, **kw):
    """epilogue(x32 @ w^T) with x32 fp32 carried as two 16-bit planes: <= 16 rows on the weight-streaming skinny GEMM, else the MFMA GEMM."""
    M, K = x32.shape
    N = w.shape[0]
    if M <= 32 and _mfma_shape(N, K):
        return gemv(split16(x32, w.dtype, tiled=True), w, w_tiles=w_tiles, **kw)
    return gemm(split16(x32, w.dtype), w, a_planes=2, **kw)


# ---------------------------------------------------------------------------------------------------------
# LLM glue
# ---------------------------------------------------------------------------------------------------------
def rope_kv_append(qkv, kcache, vcache, cos_tab, sin_tab, pos0_dev, H, D):
    lib = _lib.load()
    T = qkv.shape[0]
    assert qkv.is_contiguous() and qkv.shape[1] == 3 * H * D
    check(lib.sx_rope_kv_append(_p(qkv), _p(kcache), _p(vcache), _p(cos_tab), _p(sin_tab), _p(pos0_dev), T, H, D,
                                kcache.shape[1], _DT[qkv.dtype], _stream()), "sx_rope_kv_append")


def embedding(ids_i32, table):
    lib = _lib.load()
    T = ids_i32.numel()
    out = torch.empty((T, table.shape[1]), dtype=torch.float32, device=table.device)
    check(lib.sx_embedding(_p(ids_i32), _p(table), _p(out), T, table.shape[1], _DT[table.dtype], _stream()),
          "sx_embedding")
    return out


def scatter_rows(src, rows_i32, dst):
    lib = _lib.load()
    assert src.dtype == torch.float32 and dst.dtype == torch.float32 and src.is_contiguous() and dst.is_contiguous()
    check(lib.sx_scatter_rows(_p(src), _p(rows_i32), _p(dst), src.shape[0], src.shape[1], _stream()),
          "sx_scatter_rows")


def greedy_next(logits, vocab, img_ids_dev, prev_id_dev, next_id_dev, out_ids=None, step_dev=None):
    lib = _lib.load()
    assert logits.dtype == torch.float32
    cap = out_ids.numel() if out_ids is not None else 0          # capacity: the kernel drops writes at step >= cap
    check(lib.sx_greedy_next_b(_p(logits), 0, vocab, _p(img_ids_dev), img_ids_dev.numel(), _p(prev_id_dev),
                               _p(next_id_dev), _p(out_ids), cap, _p(step_dev), 1, _stream()), "sx_greedy_next")


# ---------------------------------------------------------------------------------------------------------
# Elementwise / layout
# ---------------------------------------------------------------------------------------------------------
def cast(x, dtype):
    lib = _lib.load()
    assert x.is_contiguous()
    y = torch.empty(x.shape, dtype=dtype, device=x.device)
    check(lib.sx_cast(_p(x), _DT[x.dtype], _p(y), _DT[dtype], x.numel(), _stream()), "sx_cast")
    return y


# Accounting hint, not behaviour: while > 1, the K of the sx_gemm launches being issued is this many times the algorithmic K
# (the VAE's fp32-grade mode triples K to carry two bf16 planes per operand). bench.py's roofline pass divides by it so that
# "achieved" counts the FLOPs of the fp32 product being emulated, not the MFMA work spent on it.
OPERAND_PLANES = 1


def split_bf16(x, role="a"):
    """fp32 [..., C] → bf16 [..., 3C]: the planes of x = hi + lo laid out [hi | hi | lo] (role "a": rows of a GEMM's A
    operand) or [hi | lo | hi] (role "w": rows of its W operand). One GEMM over K = 3C then yields Ah·Wh + Ah·Wl + Al·Wh
    with fp32 accumulation — 16 mantissa bits per operand (the VAE's fp32-grade mode)."""
    lib = _lib.load()
    assert x.dtype == torch.float32 and x.is_contiguous() and x.shape[-1] % 4 == 0
    Cc = x.shape[-1]
    out = torch.empty(x.shape[:-1] + (3 * Cc,), dtype=torch.bfloat16, device=x.device)
    check(lib.sx_split_bf16(_p(x), _p(out), x.numel() // Cc, Cc, {"a": 0, "w": 1}[role], _stream()), "sx_split_bf16")
    return out


def copy2d(src, dst, dst_col_off=0):
    """dst[:, off:off+cols] = src (fp32 2-D, row strides honoured)."""
    lib = _lib.load()
    assert src.dtype == torch.float32 and dst.dtype == torch.float32 and src.dim() == 2 and dst.dim() == 2
    assert src.stride(1) == 1 and dst.stride(1) == 1
    d = dst[:, dst_col_off:dst_col_off + src.shape[1]]
    check(lib.sx_copy2d_f32(_p(src), src.stride(0), C.c_void_p(d.data_ptr()), dst.stride(0), src.shape[0],
                            src.shape[1], _stream()), "sx_copy2d_f32")


def add(a, b):
    lib = _lib.load()
    assert a.dtype == torch.float32 and b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous()
    y = torch.empty_like(a)
    check(lib.sx_add_f32(_p(a), _p(b), _p(y), a.numel(), _stream()), "sx_add_f32")
    return y


def patchify(img, patch, kpad, dtype):
    lib = _lib.load()
    assert img.dtype == torch.float32 and img.is_contiguous() and img.shape[1] == 3 and img.shape[2] == img.shape[3]
    B, _, S, _ = img.shape
    g = S // patch
    out = torch.empty((B * g * g, kpad), dtype=dtype, device=img.device)
    check(lib.sx_patchify(_p(img), _p(out), B, S, patch, kpad, _DT[dtype], _stream()), "sx_patchify")
    return out


def im2col3x3_small(x, kpad, dtype):
    lib = _lib.load()
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4
    B, H, W, Cin = x.shape
    out = torch.empty((B * H * W, kpad), dtype=dtype, device=x.device)
    check(lib.sx_im2col3x3_small(_p(x), _p(out), B, H, W, Cin, kpad, _DT[dtype], _stream()), "sx_im2col3x3_small")
    return out


def avgpool_tokens(x, k):
    lib = _lib.load()
    assert x.dtype == torch.float32 and x.is_contiguous()
    B, L, D = x.shape
    y = torch.empty((B, L // k, D), dtype=torch.float32, device=x.device)
    check(lib.sx_avgpool_tokens(_p(x), _p(y), B, L, D, k, _stream()), "sx_avgpool_tokens")
    return y


def timestep_embedding(t, dim, dtype, idx_dev=None, n=None):
    lib = _lib.load()
    assert t.dtype == torch.float32
    n = n if n is not None else t.numel()
    out = torch.empty((n, dim), dtype=dtype, device=t.device)
    check(lib.sx_timestep_embedding(_p(t), _p(idx_dev), _p(out), n, dim, _DT[dtype], _stream()),
          "sx_timestep_embedding")
    return out


def nchw_to_nhwc(src, ld=None, dst=None):
    lib = _lib.load()
    B, Cc, H, W = src.shape
    ld = ld or Cc
    if dst is None:
        dst = torch.zeros((B, H * W, ld), dtype=torch.float32, device=src.device)
    check(lib.sx_nchw_to_nhwc(_p(src.contiguous()), _p(dst), ld, B, Cc, H * W, _stream()), "sx_nchw_to_nhwc")
    return dst


def nhwc_to_nchw(src, Cc, H, W):
    lib = _lib.load()
    B = src.shape[0]
    ld = src.shape[-1]
    dst = torch.empty((B, Cc, H, W), dtype=torch.float32, device=src.device)
    check(lib.sx_nhwc_to_nchw(_p(src), ld, _p(dst), B, Cc, H * W, _stream()), "sx_nhwc_to_nchw")
    return dst


def silu_cast(x, dtype):
    lib = _lib.load()
    assert x.dtype == torch.float32 and x.is_contiguous()
    y = torch.empty(x.shape, dtype=dtype, device=x.device)
    check(lib.sx_silu_cast(_p(x), _p(y), _DT[dtype], x.numel(), _stream()), "sx_silu_cast")
    return y


def add_i32(p, delta):
    check(_lib.load().sx_add_i32_n(_p(p), int(delta), p.numel(), _stream()), "sx_add_i32_n")


# ---- lock-step batched decode (G sequences, one token each) ---------------------------------------------------------
def rope_kv_append_b(qkv, kcache, vcache, cos_tab, sin_tab, pos_dev, G, T, H, D):
    """qkv [G*T, 3HD]; kcache/vcache [G, H, Tmax, D]; pos_dev int32 [G]."""
    lib = _lib.load()
    assert qkv.is_contiguous() and qkv.shape == (G * T, 3 * H * D) and kcache.is_contiguous() and kcache.shape[0] == G
    check(lib.sx_rope_kv_append_b(_p(qkv), _p(kcache), _p(vcache), _p(cos_tab), _p(sin_tab), _p(pos_dev), G, T, H, D,
                                  kcache.shape[2], kcache.stride(0), _DT[qkv.dtype], _stream()), "sx_rope_kv_append_b")


def attn_decode_b(q, kcache, vcache, ctx_dev, scale, nsplit=8, out_tiled=False):
    """q [G, H, D] (rows may be strided views into the fused qkv projection); caches [G, H, Tmax, D]; ctx_dev int32 [G].
    Returns [G, H*D] (out_tiled: as a Tiled16 for the o-projection)."""
    lib = _lib.load()
    G, H, D = q.shape
    assert q.stride(2) == 1 and q.stride(1) == D and q.stride(0) % 8 == 0
    code = _DT[q.dtype]
    if out_tiled:
        ot = Tiled16(G, H * D, q.dtype, q.device)
        out, code = ot.t, code | _lib.SX_TILED16
    else:
        out = torch.empty((G, H * D), dtype=q.dtype, device=q.device)
    scratch = torch.empty((G, H, nsplit, D + 2), dtype=torch.float32, device=q.device)
    check(lib.sx_attn_decode_b(_p(q), _p(kcache), _p(vcache), _p(out), _p(scratch), _p(ctx_dev), G, H, D, kcache.shape[2],
                               kcache.stride(0), nsplit, float(scale), code, q.stride(0), _stream()), "sx_attn_decode_b")
    return ot if out_tiled else out


def attn_decode_fused(qkv, kcache, vcache, pos_dev, cos_tab, sin_tab, scale, H, D, counters, nsplit=8, out_tiled=False):
    """RoPE + KV append + split-KV attention + combine for ONE new token of each of G sequences, one launch.
    qkv [G, 3*H*D] (left untouched); caches [G, H, Tmax, D]; pos_dev int32 [G]; counters: zero int32 [>= G*H] (left zero).
    Returns [G, H*D] (out_tiled: as a Tiled16 for the o-projection)."""
    lib = _lib.load()
    G = qkv.shape[0]
    assert qkv.is_contiguous() and qkv.shape[1] == 3 * H * D and counters.dtype == torch.int32 and counters.numel() >= G * H
    code = _DT[qkv.dtype]
    if out_tiled:
        ot = Tiled16(G, H * D, qkv.dtype, qkv.device)
        out, code = ot.t, code | _lib.SX_TILED16
    else:
        out = torch.empty((G, H * D), dtype=qkv.dtype, device=qkv.device)
    scratch = torch.empty((G, H, nsplit, D + 2), dtype=torch.float32, device=qkv.device)
    a = _lib.AttnDecodeArgs()
    a.qkv, a.kcache, a.vcache, a.out, a.scratch, a.counters = _p(qkv), _p(kcache), _p(vcache), _p(out), _p(scratch), _p(counters)
    a.cos_tab, a.sin_tab, a.pos_dev = _p(cos_tab), _p(sin_tab), _p(pos_dev)
    a.G, a.H, a.D, a.Tmax, a.nsplit, a.dtype = G, H, D, kcache.shape[2], nsplit, code
    a.cache_seq_stride, a.scale = kcache.stride(0), float(scale)
    check(lib.sx_attn_decode_fused(C.byref(a), _stream()), "sx_attn_decode_fused")
    return ot if out_tiled else out


def _next_lockstep(logits, vocab, img_ids_dev, cur_dev, out_ids, step_dev, sample=None, lp=None):
    """The lock-step tail of the token step: sx_greedy_next_b, or sx_sample_next_b when ``sample`` (a filled SampleArgs) is given;
    ``lp`` (a logprob state): sx_sample_next_b_lp, whose row capacity is the state's."""
    lib = _lib.load()
    assert logits.dtype == torch.float32 and logits.stride(1) == 1
    ld_out = out_ids.stride(0) if out_ids is not None else 0
    if lp is not None:
        la, ld_out = _logprob_args(lp, logits.shape[0], out_ids)
        assert step_dev is not None, "the LP tail needs step_dev"
    args = (_p(logits), logits.stride(0), vocab, _p(img_ids_dev), img_ids_dev.numel(), _p(cur_dev), _p(cur_dev), _p(out_ids),
            ld_out, _p(step_dev), logits.shape[0])
    if lp is not None:
        check(lib.sx_sample_next_b_lp(*args, C.byref(sample) if sample is not None else None, C.byref(la), _stream()), "sx_sample_next_b_lp")
    elif sample is None:
        check(lib.sx_greedy_next_b(*args, _stream()), "sx_greedy_next_b")
    else:
        check(lib.sx_sample_next_b(*args, C.byref(sample), _stream()), "sx_sample_next_b")


def _slot_step_args(who, logits, vocab, img_ids_dev, cur, live, n_new, max_new, force_at, pos, ctx, step, out_ids, status, force_id,
                    eos_id):
    """sx_slot_step_args from the slot tensors, checked: logits fp32 [G, ld], the rest contiguous int32 on the device."""
    G = logits.shape[0]
    assert logits.dtype == torch.float32 and logits.stride(1) == 1
    for t in (img_ids_dev, cur, live, n_new, max_new, force_at, pos, ctx, step, status) + ((out_ids,) if out_ids is not None else ()):
        assert t.dtype == torch.int32 and t.is_contiguous(), f"{who}: contiguous int32 tensors"
    for t in (cur, live, n_new, max_new, force_at, pos, ctx, step):
        assert t.numel() == G
    assert status.numel() == 4 * G and (out_ids is None or out_ids.shape[0] == G)
    for t in (logits, img_ids_dev, cur, live, n_new, max_new, force_at, pos, ctx, step, status):
        _p(t)                                   # (GPU tensors only: no CPU fallback)
    return _lib.SlotStepArgs(
        logits=logits.data_ptr(), img_ids_dev=img_ids_dev.data_ptr(), cur=cur.data_ptr(), live=live.data_ptr(),
        n_new=n_new.data_ptr(), max_new=max_new.data_ptr(), force_at=force_at.data_ptr(), pos=pos.data_ptr(), ctx=ctx.data_ptr(),
        step=step.data_ptr(), out_ids=out_ids.data_ptr() if out_ids is not None else None, status=status.data_ptr(),
        ld_logits=logits.stride(0), vocab=int(vocab), n_img=img_ids_dev.numel(), ld_out=out_ids.shape[1] if out_ids is not None else 0,
        force_id=int(force_id), eos_id=int(eos_id), G=G, reserved=0)


def greedy_next_b(logits, vocab, img_ids_dev, cur_dev, out_ids, step_dev):
    """logits fp32 [G, ld]; cur_dev int32 [G] (in: previous id, out: next id); out_ids int32 [G, ld_out]; step_dev [G]."""
    _next_lockstep(logits, vocab, img_ids_dev, cur_dev, out_ids, step_dev)


def greedy_next_slots(logits, vocab, img_ids_dev, cur, live, n_new, max_new, force_at, pos, ctx, step, out_ids, status,
                      force_id=-1, eos_id=-1):
    """In-flight batching tail of the token step (sx_greedy_next_slots): logits fp32 [G, ld]; every other tensor int32 [G] on the
    device, out_ids [G, rows] or None, status [G, 4]. Live slots take their next id, advance n_new / step / pos / ctx and park
    themselves when the id is ``eos_id`` or their budget is reached; parked slots are not touched."""
    a = _slot_step_args("greedy_next_slots", logits, vocab, img_ids_dev, cur, live, n_new, max_new, force_at, pos, ctx, step, out_ids,
                        status, force_id, eos_id)
    check(_lib.load().sx_greedy_next_slots(C.byref(a), _stream()), "sx_greedy_next_slots")


def _sample_args(sample, G, token_index=None, n_kept=None, p_chosen=None):
    """sx_sample_args from a sampling state (llama.SampleState or anything with its five [G] device tensors; seed is [G, 2])."""
    i32, f32 = torch.int32, torch.float32
    for t, dt, n in ((sample.do_sample, i32, G), (sample.temperature, f32, G), (sample.top_k, i32, G), (sample.top_p, f32, G),
                     (sample.seed, i32, 2 * G), (token_index, i32, G), (n_kept, i32, G), (p_chosen, f32, G)):
        if t is not None:
            assert t.dtype == dt and t.is_contiguous() and t.numel() == n, "sampling: contiguous [G] tensors (seed int32 [G, 2])"
    d = lambda t: None if t is None else _p(t).value      # (GPU tensors only: no CPU fallback)
    return _lib.SampleArgs(do_sample=d(sample.do_sample), temperature=d(sample.temperature), top_k=d(sample.top_k),
                           top_p=d(sample.top_p), seed=d(sample.seed), token_index=d(token_index), n_kept=d(n_kept),
                           p_chosen=d(p_chosen))


def sample_next_b(logits, vocab, img_ids_dev, cur_dev, out_ids, step_dev, sample, token_index=None, n_kept=None, p_chosen=None):
    """greedy_next_b with the seeded sampling rule (sx_sample_next_b; seedx_amd.sampling states the rule): ``sample`` holds the per-row
    parameters on the device (do_sample / top_k int32 [G], temperature / top_p fp32 [G], seed int32 [G, 2] = low, high word);
    ``token_index`` int32 [G] is the index of the generated token within its request (default: ``step_dev``). Rows with do_sample = 0
    take the greedy id. Optional outputs n_kept int32 [G], p_chosen fp32 [G]."""
    token_index = step_dev if token_index is None else token_index
    assert token_index is not None, "sample_next_b: token_index (or step_dev) is required"
    _next_lockstep(logits, vocab, img_ids_dev, cur_dev, out_ids, step_dev,
                   _sample_args(sample, logits.shape[0], token_index, n_kept, p_chosen))


def sample_next_slots(logits, vocab, img_ids_dev, cur, live, n_new, max_new, force_at, pos, ctx, step, out_ids, status, sample,
                      force_id=-1, eos_id=-1, n_kept=None, p_chosen=None):
    """greedy_next_slots with the seeded sampling rule (sx_sample_next_slots): the token index of slot g is ``step[g]``."""
    a = _slot_step_args("sample_next_slots", logits, vocab, img_ids_dev, cur, live, n_new, max_new, force_at, pos, ctx, step, out_ids,
                        status, force_id, eos_id)
    s = _sample_args(sample, logits.shape[0], None, n_kept, p_chosen)
    check(_lib.load().sx_sample_next_slots(C.byref(a), C.byref(s), _stream()), "sx_sample_next_slots")


def _logprob_args(lp, G, out_ids):
    """(sx_logprob_args, row capacity) from a logprob state (llama.LogprobState or anything with its tensors): ``want`` int32 [G],
    ``chosen`` fp32 [G, rows], ``top_ids`` int32 / ``top`` fp32 [G, rows, n_top] (unused when n_top = 0). ``out_ids`` shares the capacity."""
    n, rows = int(lp.n_top), lp.chosen.shape[1]
    assert 0 <= n <= 8, "logprobs: n_top in 0 .. 8"
    assert lp.want.dtype == torch.int32 and lp.want.is_contiguous() and lp.want.numel() == G
    assert lp.chosen.dtype == torch.float32 and lp.chosen.is_contiguous() and lp.chosen.shape == (G, rows)
    assert out_ids is None or (out_ids.is_contiguous() and out_ids.shape[1] == rows), "logprobs: the buffers share out_ids' row capacity"
    if n:
        assert lp.top_ids.dtype == torch.int32 and lp.top_ids.is_contiguous() and lp.top_ids.shape == (G, rows, n)
        assert lp.top.dtype == torch.float32 and lp.top.is_contiguous() and lp.top.shape == (G, rows, n)
    d = lambda t: _p(t).value                             # (GPU tensors only: no CPU fallback)
    return _lib.LogprobArgs(want=d(lp.want), chosen=d(lp.chosen), top_ids=d(lp.top_ids) if n else None, top=d(lp.top) if n else None,
                            n_top=n, reserved=0), rows


def token_logprobs(logits, vocab, targets, n_top=0):
    """sx_token_logprobs: logits fp32 [rows, ld] (columns >= vocab are never read), targets int32 [rows] → (chosen fp32 [rows],
    top_ids int32 [rows, n_top], top fp32 [rows, n_top]): lp(target) and the n_top largest lp of each RAW row
    (seedx_amd.sampling.token_logprobs states the rule)."""
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1 and 0 <= int(n_top) <= 8
    R = logits.shape[0]
    assert targets.dtype == torch.int32 and targets.is_contiguous() and targets.numel() == R
    chosen = torch.empty(R, dtype=torch.float32, device=logits.device)
    top_ids = torch.empty((R, n_top), dtype=torch.int32, device=logits.device)
    top = torch.empty((R, n_top), dtype=torch.float32, device=logits.device)
    check(_lib.load().sx_token_logprobs(_p(logits), logits.stride(0), int(vocab), _p(targets), _p(chosen), _p(top_ids) if n_top else None,
                                        _p(top) if n_top else None, int(n_top), R, _stream()), "sx_token_logprobs")
    return chosen, top_ids, top


def next_b_lp(logits, vocab, img_ids_dev, cur_dev, out_ids, step_dev, lp, sample=None, token_index=None, n_kept=None, p_chosen=None):
    """greedy_next_b (``sample`` None) or sample_next_b with the record of sx_sample_next_b_lp: rows with ``lp.want`` != 0 store the
    log-probability of their id and the top list at [g, step[g]] of the state's buffers; everything else is the call without ``lp``."""
    if sample is not None:
        token_index = step_dev if token_index is None else token_index
        sample = _sample_args(sample, logits.shape[0], token_index, n_kept, p_chosen)
    _next_lockstep(logits, vocab, img_ids_dev, cur_dev, out_ids, step_dev, sample, lp)


def next_slots_lp(logits, vocab, img_ids_dev, cur, live, n_new, max_new, force_at, pos, ctx, step, out_ids, status, lp, sample=None,
                  force_id=-1, eos_id=-1, n_kept=None, p_chosen=None):
    """greedy_next_slots (``sample`` None) or sample_next_slots with the record of sx_sample_next_slots_lp (next_b_lp's, per live slot)."""
    a = _slot_step_args("next_slots_lp", logits, vocab, img_ids_dev, cur, live, n_new, max_new, force_at, pos, ctx, step, out_ids,
                        status, force_id, eos_id)
    la, a.ld_out = _logprob_args(lp, logits.shape[0], out_ids)
    s = _sample_args(sample, logits.shape[0], None, n_kept, p_chosen) if sample is not None else None
    check(_lib.load().sx_sample_next_slots_lp(C.byref(a), C.byref(s) if s is not None else None, C.byref(la), _stream()),
          "sx_sample_next_slots_lp")


def _ctl_args(ctl, logits, vocab, token_index=None, eos_id=-1):
    """sx_logits_ctl_args from a control state (llama.ControlState or anything with its tensors): ``on`` / ``min_new`` int32 [G],
    ``counts`` int32 [G, ld_counts], ``work`` fp32 [G, ld] with the logits' row stride, ``rep`` / ``rep_inv`` / ``presence`` /
    ``frequency`` fp32 [G], ``bias_ids`` int32 / ``bias`` fp32 [G, 16]."""
    G, i32, f32 = logits.shape[0], torch.int32, torch.float32
    for t, dt, shape in ((ctl.on, i32, (G,)), (ctl.min_new, i32, (G,)), (ctl.rep, f32, (G,)), (ctl.rep_inv, f32, (G,)),
                         (ctl.presence, f32, (G,)), (ctl.frequency, f32, (G,)), (ctl.bias_ids, i32, (G, 16)), (ctl.bias, f32, (G, 16))):
        assert t.dtype == dt and t.is_contiguous() and tuple(t.shape) == shape, "logits controls: contiguous [G] / [G, 16] tensors"
    assert ctl.counts.dtype == i32 and ctl.counts.is_contiguous() and ctl.counts.shape[0] == G and ctl.counts.shape[1] >= vocab
    assert ctl.work.dtype == f32 and ctl.work.is_contiguous() and tuple(ctl.work.shape) == (G, logits.stride(0)) and logits.stride(0) >= vocab, \
        "logits controls: work is fp32 [G, the logits' row stride]"
    assert token_index is None or (token_index.dtype == i32 and token_index.is_contiguous() and token_index.numel() == G)
    d = lambda t: None if t is None else _p(t).value      # (GPU tensors only: no CPU fallback)
    return _lib.LogitsCtlArgs(on=d(ctl.on), counts=d(ctl.counts), work=d(ctl.work), rep=d(ctl.rep), rep_inv=d(ctl.rep_inv),
                              presence=d(ctl.presence), frequency=d(ctl.frequency), min_new=d(ctl.min_new), bias_ids=d(ctl.bias_ids),
                              bias=d(ctl.bias), token_index=d(token_index), ld_counts=ctl.counts.shape[1], eos_id=int(eos_id))


def next_b_ctl(logits, vocab, img_ids_dev, cur_dev, out_ids, step_dev, ctl, sample=None, lp=None, token_index=None, n_kept=None,
               p_chosen=None, eos_id=-1):
    """The lock-step tail with per-request logits controls (sx_next_b_ctl; seedx_amd.sampling.apply_controls states the rule): greedy
    (``sample`` None) or sampled, with or without the LP record (``lp``). Rows with ``ctl.on`` != 0 take their id from the edited copy
    of their row in ``ctl.work`` — the logits row itself stays untouched — and count it in ``ctl.counts``; the others run as without
    ``ctl``. ``token_index`` int32 [G] (default ``step_dev``) is the sampler's and min_new_tokens' index; ``eos_id``: the column that
    min_new_tokens masks (-1: none)."""
    lib = _lib.load()
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    G = logits.shape[0]
    token_index = step_dev if token_index is None else token_index
    assert token_index is not None, "next_b_ctl: token_index (or step_dev) is required"
    ld_out = out_ids.stride(0) if out_ids is not None else 0
    la = None
    if lp is not None:
        la, ld_out = _logprob_args(lp, G, out_ids)
        assert step_dev is not None, "the LP tail needs step_dev"
    sa = _sample_args(sample, G, token_index, n_kept, p_chosen) if sample is not None else None
    ca = _ctl_args(ctl, logits, vocab, token_index, eos_id)
    check(lib.sx_next_b_ctl(_p(logits), logits.stride(0), vocab, _p(img_ids_dev), img_ids_dev.numel(), _p(cur_dev), _p(cur_dev), _p(out_ids),
                            ld_out, _p(step_dev), G, C.byref(sa) if sa is not None else None, C.byref(la) if la is not None else None,
                            C.byref(ca), _stream()), "sx_next_b_ctl")


def next_slots_ctl(logits, vocab, img_ids_dev, cur, live, n_new, max_new, force_at, pos, ctx, step, out_ids, status, ctl, sample=None,
                   lp=None, force_id=-1, eos_id=-1, n_kept=None, p_chosen=None):
    """The in-flight tail with per-request logits controls (sx_next_slots_ctl): greedy_next_slots / sample_next_slots / next_slots_lp
    with next_b_ctl's edit per live slot; the token index is ``step[g]``, the masked column the call's ``eos_id``, and the id counted is
    the one the slot emits (behind the force_at replacement). Parked slots and slots with ``ctl.on`` = 0 are as without ``ctl``."""
    a = _slot_step_args("next_slots_ctl", logits, vocab, img_ids_dev, cur, live, n_new, max_new, force_at, pos, ctx, step, out_ids,
                        status, force_id, eos_id)
    G = logits.shape[0]
    la = None
    if lp is not None:
        la, a.ld_out = _logprob_args(lp, G, out_ids)
    s = _sample_args(sample, G, None, n_kept, p_chosen) if sample is not None else None
    ca = _ctl_args(ctl, logits, vocab, None, eos_id)
    check(_lib.load().sx_next_slots_ctl(C.byref(a), C.byref(s) if s is not None else None, C.byref(la) if la is not None else None,
                                        C.byref(ca), _stream()), "sx_next_slots_ctl")


def _fsm_args(fsm, logits, vocab, eos_id=-1):
    """sx_token_fsm_args from a grammar state (llama.GrammarState or anything with its tensors): ``table`` / ``state`` int32 [G],
    ``trans`` int16 [n_tables, n_states, ld_v] and ``flags`` int32 [n_tables, n_states]. The shapes are checked here, so that the kernel's
    range test of table[g] and state[g] is all that stands between a row and the table."""
    G, i32 = logits.shape[0], torch.int32
    for t in (fsm.table, fsm.state):
        assert t.dtype == i32 and t.is_contiguous() and tuple(t.shape) == (G,), "token automaton: table / state are contiguous int32 [G]"
    tr, fl = fsm.trans, fsm.flags
    assert tr.dtype == torch.int16 and tr.is_contiguous() and tr.dim() == 3, "token automaton: trans is int16 [n_tables, n_states, ld_v]"
    assert fl.dtype == i32 and fl.is_contiguous() and tuple(fl.shape) == tuple(tr.shape[:2]), "token automaton: flags is int32 [n_tables, n_states]"
    # (ld_v even and >= vocab: the entry point refuses anything else)
    return _lib.TokenFsmArgs(table=_p(fsm.table).value, state=_p(fsm.state).value, trans=_p(tr).value, flags=_p(fl).value,
                             n_tables=tr.shape[0], n_states=tr.shape[1], ld_v=tr.shape[2], eos_id=int(eos_id))


def next_b_fsm(logits, vocab, img_ids_dev, cur_dev, out_ids, step_dev, ctl, fsm, sample=None, lp=None, token_index=None, n_kept=None,
               p_chosen=None, eos_id=-1):
    """The lock-step tail with a token automaton per row (sx_next_b_fsm; seedx_amd.grammar states the rule): next_b_ctl, and a row with
    ``fsm.table[g]`` >= 0 and ``fsm.state[g]`` >= 0 takes its id from a working row in ``ctl.work`` (the controlled row, or a plain copy
    with ``ctl.on[g]`` = 0) in which the ids its table row bans are -inf and ``eos_id`` survives only in an accepting state; the image
    rule is skipped for it, and ``fsm.state[g]`` advances on the id it emits (DONE = -2: the row runs unconstrained from then on).
    Every other row is next_b_ctl's, bit for bit. ``eos_id`` serves min_new_tokens and the automaton alike."""
    lib = _lib.load()
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    G = logits.shape[0]
    token_index = step_dev if token_index is None else token_index
    assert token_index is not None, "next_b_fsm: token_index (or step_dev) is required"
    ld_out = out_ids.stride(0) if out_ids is not None else 0
    la = None
    if lp is not None:
        la, ld_out = _logprob_args(lp, G, out_ids)
        assert step_dev is not None, "the LP tail needs step_dev"
    sa = _sample_args(sample, G, token_index, n_kept, p_chosen) if sample is not None else None
    ca = _ctl_args(ctl, logits, vocab, token_index, eos_id)
    fa = _fsm_args(fsm, logits, vocab, eos_id)
    check(lib.sx_next_b_fsm(_p(logits), logits.stride(0), vocab, _p(img_ids_dev), img_ids_dev.numel(), _p(cur_dev), _p(cur_dev), _p(out_ids),
                            ld_out, _p(step_dev), G, C.byref(sa) if sa is not None else None, C.byref(la) if la is not None else None,
                            C.byref(ca), C.byref(fa), _stream()), "sx_next_b_fsm")


def next_slots_fsm(logits, vocab, img_ids_dev, cur, live, n_new, max_new, force_at, pos, ctx, step, out_ids, status, ctl, fsm, sample=None,
                   lp=None, force_id=-1, eos_id=-1, n_kept=None, p_chosen=None):
    """The in-flight tail with a token automaton per slot (sx_next_slots_fsm): next_slots_ctl with next_b_fsm's mask and advance per live
    slot; a slot whose state becomes DONE stops and parks itself exactly as on EOS or budget. Parked slots read and write nothing,
    ``fsm.state`` included; slots with ``fsm.table`` < 0 or ``fsm.state`` < 0 are next_slots_ctl's."""
    a = _slot_step_args("next_slots_fsm", logits, vocab, img_ids_dev, cur, live, n_new, max_new, force_at, pos, ctx, step, out_ids,
                        status, force_id, eos_id)
    G = logits.shape[0]
    la = None
    if lp is not None:
        la, a.ld_out = _logprob_args(lp, G, out_ids)
    s = _sample_args(sample, G, None, n_kept, p_chosen) if sample is not None else None
    ca = _ctl_args(ctl, logits, vocab, None, eos_id)
    fa = _fsm_args(fsm, logits, vocab, -1)
    check(_lib.load().sx_next_slots_fsm(C.byref(a), C.byref(s) if s is not None else None, C.byref(la) if la is not None else None,
                                        C.byref(ca), C.byref(fa), _stream()), "sx_next_slots_fsm")


def _seq_args(who, seq, G):
    """sx_seq_rule_args from a sequence-rule state (llama.SeqRuleState or anything with its tensors): ``on`` / ``ngram`` / ``hist_len`` /
    ``prompt_len`` / ``n_stop`` / ``matched`` int32 [G], ``hist`` int32 [G, ld_hist], ``stop_len`` int32 [G, 4], ``stop_ids`` int32
    [G, 4, 8]. Values the device would clamp are refused here (ValueError): ``ngram`` outside 0 .. 8, ``n_stop`` outside 0 .. 4, a
    ``stop_len`` outside 1 .. 8 among a row's first ``n_stop``. A state that keeps host mirrors (``host_limits()`` → the three as lists)
    is checked on those; any other state is read back from the device, except inside a graph capture, where nothing can be read."""
    i32 = torch.int32
    for t, shape in ((seq.on, (G,)), (seq.ngram, (G,)), (seq.hist_len, (G,)), (seq.prompt_len, (G,)), (seq.n_stop, (G,)),
                     (seq.matched, (G,)), (seq.stop_len, (G, 4)), (seq.stop_ids, (G, 4, 8))):
        assert t.dtype == i32 and t.is_contiguous() and tuple(t.shape) == shape, f"{who}: contiguous int32 [G] / [G, 4] / [G, 4, 8] tensors"
    h = seq.hist
    assert h.dtype == i32 and h.dim() == 2 and h.is_contiguous() and h.shape[0] == G, f"{who}: hist is contiguous int32 [G, ld_hist]"
    lim = seq.host_limits() if hasattr(seq, "host_limits") else None
    if lim is None and not torch.cuda.is_current_stream_capturing():
        lim = (seq.ngram.tolist(), seq.n_stop.tolist(), seq.stop_len.tolist())
    if lim is not None:
        ngram, n_stop, stop_len = lim
        for g in range(G):
            if not 0 <= int(ngram[g]) <= 8:
                raise ValueError(f"{who}: ngram[{g}]={int(ngram[g])} lies outside 0 .. 8")
            if not 0 <= int(n_stop[g]) <= 4:
                raise ValueError(f"{who}: n_stop[{g}]={int(n_stop[g])} lies outside 0 .. 4")
            for j in range(int(n_stop[g])):
                if not 1 <= int(stop_len[g][j]) <= 8:
                    raise ValueError(f"{who}: stop_len[{g}][{j}]={int(stop_len[g][j])} lies outside 1 .. 8")
    d = lambda t: _p(t).value                             # (GPU tensors only: no CPU fallback)
    return _lib.SeqRuleArgs(on=d(seq.on), ngram=d(seq.ngram), hist=d(h), hist_len=d(seq.hist_len),
                            prompt_len=d(seq.prompt_len), n_stop=d(seq.n_stop), stop_len=d(seq.stop_len), stop_ids=d(seq.stop_ids),
                            matched=d(seq.matched), ld_hist=h.shape[1], reserved=0)


def next_b_seq(logits, vocab, img_ids_dev, cur_dev, out_ids, step_dev, ctl, seq, fsm=None, sample=None, lp=None, token_index=None,
               n_kept=None, p_chosen=None, eos_id=-1):
    """The lock-step tail with sequence rules per row (sx_next_b_seq; seedx_amd.sampling states them: apply_no_repeat, stop_match):
    next_b_ctl (``fsm`` None) or next_b_fsm, and a row with ``seq.on[g]`` != 0 has the ids that would repeat an n-gram of its history
    banned in a working row in ``ctl.work`` (behind the controls, ahead of the grammar mask and the image rule), appends the id it emits
    to ``seq.hist`` and reports in ``seq.matched[g]`` the stop sequence its generated ids now end with (-1: none). Every other row is
    next_b_ctl's / next_b_fsm's, bit for bit, and its history is not touched."""
    lib = _lib.load()
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    G = logits.shape[0]
    token_index = step_dev if token_index is None else token_index
    assert token_index is not None, "next_b_seq: token_index (or step_dev) is required"
    ld_out = out_ids.stride(0) if out_ids is not None else 0
    la = None
    if lp is not None:
        la, ld_out = _logprob_args(lp, G, out_ids)
        assert step_dev is not None, "the LP tail needs step_dev"
    sa = _sample_args(sample, G, token_index, n_kept, p_chosen) if sample is not None else None
    ca = _ctl_args(ctl, logits, vocab, token_index, eos_id)
    fa = _fsm_args(fsm, logits, vocab, eos_id) if fsm is not None else None
    qa = _seq_args("next_b_seq", seq, G)
    check(lib.sx_next_b_seq(_p(logits), logits.stride(0), vocab, _p(img_ids_dev), img_ids_dev.numel(), _p(cur_dev), _p(cur_dev), _p(out_ids),
                            ld_out, _p(step_dev), G, C.byref(sa) if sa is not None else None, C.byref(la) if la is not None else None,
                            C.byref(ca), C.byref(fa) if fa is not None else None, C.byref(qa), _stream()), "sx_next_b_seq")


def next_slots_seq(logits, vocab, img_ids_dev, cur, live, n_new, max_new, force_at, pos, ctx, step, out_ids, status, ctl, seq, fsm=None,
                   sample=None, lp=None, force_id=-1, eos_id=-1, n_kept=None, p_chosen=None):
    """The in-flight tail with sequence rules per slot (sx_next_slots_seq): next_slots_ctl / next_slots_fsm with next_b_seq's ban,
    append and stop match per live slot; a slot whose generated ids end with one of its stop sequences stops and parks itself exactly
    as on EOS or budget. Parked slots read and write nothing, their history included; slots with ``seq.on`` = 0 are next_slots_ctl's /
    next_slots_fsm's."""
    a = _slot_step_args("next_slots_seq", logits, vocab, img_ids_dev, cur, live, n_new, max_new, force_at, pos, ctx, step, out_ids,
                        status, force_id, eos_id)
    G = logits.shape[0]
    la = None
    if lp is not None:
        la, a.ld_out = _logprob_args(lp, G, out_ids)
    s = _sample_args(sample, G, None, n_kept, p_chosen) if sample is not None else None
    ca = _ctl_args(ctl, logits, vocab, None, eos_id)
    fa = _fsm_args(fsm, logits, vocab, -1) if fsm is not None else None
    qa = _seq_args("next_slots_seq", seq, G)
    check(_lib.load().sx_next_slots_seq(C.byref(a), C.byref(s) if s is not None else None, C.byref(la) if la is not None else None,
                                        C.byref(ca), C.byref(fa) if fa is not None else None, C.byref(qa), _stream()), "sx_next_slots_seq")


def _i32s(who, *ts):
    for t in ts:
        assert t.dtype == torch.int32 and t.is_contiguous(), f"{who}: contiguous int32 tensors"
        _p(t)                                   # (GPU tensors only: no CPU fallback)


def scatter_rows_spec(src, step_dev, dst, tok_index=None):
    """dst [G, rows, dim] fp32; dst[g, step[g] + t] = src[g*T + t] for the T = src.shape[0] // G rows of every slot (sx_scatter_rows_spec);
    ``tok_index`` int32 [G*T] receives step[g] + t."""
    G, rows, dim = dst.shape
    T = src.shape[0] // G
    assert src.shape == (G * T, dim) and src.is_contiguous() and dst.is_contiguous() and src.dtype == dst.dtype == torch.float32
    assert step_dev.dtype == torch.int32 and step_dev.numel() == G
    assert tok_index is None or (tok_index.dtype == torch.int32 and tok_index.is_contiguous() and tok_index.numel() == G * T)
    check(_lib.load().sx_scatter_rows_spec(_p(src), _p(step_dev), _p(dst), _p(tok_index), G, T, dim, rows, _stream()), "sx_scatter_rows_spec")


def spec_candidates(logits, vocab, img_ids_dev, rows_in, cand, token_index, sample=None):
    """Candidate ids of the G*T rows of a verify step: sx_greedy_next_b, or sx_sample_next_b with ``sample`` (a sampling state whose
    tensors hold one entry per ROW), over logits fp32 [G*T, ld]. Previous id = the row's input ``rows_in``; ``token_index`` int32 [G*T]
    = step[g] + t; ``cand`` int32 [G*T] receives the ids. Nothing else is written (the image columns of the logits rows are zeroed in place)."""
    lib = _lib.load()
    R = logits.shape[0]
    assert logits.dtype == torch.float32 and logits.stride(1) == 1
    _i32s("spec_candidates", img_ids_dev, rows_in, cand, token_index)
    assert rows_in.numel() == R and cand.numel() == R and token_index.numel() == R
    args = (_p(logits), logits.stride(0), vocab, _p(img_ids_dev), img_ids_dev.numel(), _p(rows_in), _p(cand), None, 0, _p(token_index), R)
    if sample is None:
        check(lib.sx_greedy_next_b(*args, _stream()), "sx_greedy_next_b")
    else:
        check(lib.sx_sample_next_b(*args, C.byref(_sample_args(sample, R, token_index)), _stream()), "sx_sample_next_b")


def spec_accept(cand, rows_in, n_draft, cur, live, n_new, max_new, force_at, pos, ctx, step, out_ids, status, hist=None, force_id=-1,
                eos_id=-1, img_ids_dev=None):
    """The accept rule of speculative decoding on the device (sx_spec_accept; seedx_amd.spec.accept states it): per live slot the longest
    run of candidates ``cand`` [G*T] the model itself would have produced given the drafts fed as ``rows_in`` [G*T] (``n_draft`` [G] of
    them per slot), with greedy_next_slots' force_at, id log, counters, stop rule, parking and status; ``hist`` int32 [G, Tmax] receives
    the emitted ids at the cache positions where they will be fed; ``img_ids_dev`` (the token step's list): its first id, <img>, ends a
    run. Row 0 of every live slot in ``rows_in`` becomes the new current token. Parked slots are not touched."""
    G = cur.numel()
    T = cand.numel() // G
    who = "spec_accept"
    _i32s(who, cand, rows_in, n_draft, cur, live, n_new, max_new, force_at, pos, ctx, step, status)
    _i32s(who, *[t for t in (out_ids, hist, img_ids_dev) if t is not None])
    assert cand.numel() == G * T and rows_in.numel() == G * T and status.numel() == 4 * G
    for t in (n_draft, live, n_new, max_new, force_at, pos, ctx, step):
        assert t.numel() == G
    assert (out_ids is None or out_ids.shape[0] == G) and (hist is None or (hist.dim() == 2 and hist.shape[0] == G))
    a = _lib.SpecAcceptArgs(
        cand=cand.data_ptr(), rows_in=rows_in.data_ptr(), n_draft=n_draft.data_ptr(), cur=cur.data_ptr(), live=live.data_ptr(),
        n_new=n_new.data_ptr(), max_new=max_new.data_ptr(), force_at=force_at.data_ptr(), pos=pos.data_ptr(), ctx=ctx.data_ptr(),
        step=step.data_ptr(), out_ids=out_ids.data_ptr() if out_ids is not None else None, status=status.data_ptr(),
        hist=hist.data_ptr() if hist is not None else None, G=G, T=T, ld_out=out_ids.shape[1] if out_ids is not None else 0,
        img_ids_dev=img_ids_dev.data_ptr() if img_ids_dev is not None else None,
        Tmax=hist.shape[1] if hist is not None else 0, force_id=int(force_id), eos_id=int(eos_id))
    check(_lib.load().sx_spec_accept(C.byref(a), _stream()), "sx_spec_accept")


def spec_draft_ngram(hist, pos, cur, rows_out, n_draft, ngram=(3, 1)):
    """The prompt-lookup drafter on the device (sx_spec_draft_ngram; seedx_amd.spec.propose_ngram states the rule): ``hist`` int32
    [G, Tmax] holds the ids by cache position, ``pos`` [G] the position of ``cur`` [G]; writes the next verify step's row inputs
    ``rows_out`` [G*T] (row 0 = cur, then the draft) and ``n_draft`` [G]. ``ngram`` = (longest, shortest) n-gram tried."""
    G, Tmax = hist.shape
    T = rows_out.numel() // G
    _i32s("spec_draft_ngram", hist, pos, cur, rows_out, n_draft)
    assert pos.numel() == G and cur.numel() == G and n_draft.numel() == G and rows_out.numel() == G * T
    a = _lib.SpecDraftArgs(hist=hist.data_ptr(), pos=pos.data_ptr(), cur=cur.data_ptr(), rows_out=rows_out.data_ptr(),
                           n_draft=n_draft.data_ptr(), G=G, T=T, Tmax=Tmax, ngram_max=int(ngram[0]), ngram_min=int(ngram[1]), reserved=0)
    check(_lib.load().sx_spec_draft_ngram(C.byref(a), _stream()), "sx_spec_draft_ngram")


def scatter_rows_step(src, step_dev, dst):
    """dst [G, rows, dim] fp32; dst[g, step[g]] = src[g]."""
    lib = _lib.load()
    G, rows, dim = dst.shape
    assert src.shape == (G, dim) and src.is_contiguous() and dst.is_contiguous()
    check(lib.sx_scatter_rows_step(_p(src), _p(step_dev), _p(dst), G, dim, rows, _stream()), "sx_scatter_rows_step")


def cfg_euler_step(eps, latents, scaled_next, sigmas_dev, step_dev, nb, C_lat, ld_scaled, gs, igs, mode):
    lib = _lib.load()
    n = latents.numel()
    check(lib.sx_cfg_euler_step(_p(eps), _p(latents), _p(scaled_next), _p(sigmas_dev), _p(step_dev), nb, n, C_lat,
                                ld_scaled, float(gs), float(igs), mode, _stream()), "sx_cfg_euler_step")


def cfg_dpmpp2m_step(eps, latents, x0_prev, scaled_next, sigmas_dev, coef_dev, step_dev, nb, C_lat, ld_scaled, gs, igs, mode):
    """cfg_euler_step's buffers plus x0_prev (fp32, the shape of latents: the previous denoised sample, not read on a step whose c is 0)
    and coef_dev [steps, 3] fp32, the (a, b, c) rows of solvers.dpmpp2m_coefficients: one CFG + DPM-Solver++(2M) step."""
    lib = _lib.load()
    n = latents.numel()
    f32 = torch.float32
    assert x0_prev.dtype == f32 and x0_prev.is_contiguous() and x0_prev.numel() == n and latents.dtype == f32 and latents.is_contiguous()
    assert coef_dev.dtype == f32 and coef_dev.is_contiguous() and coef_dev.dim() == 2 and coef_dev.shape[1] == 3
    assert sigmas_dev.dtype == f32 and sigmas_dev.numel() >= coef_dev.shape[0] + 1, "sigmas must hold one more entry than coef has rows"
    check(lib.sx_cfg_dpmpp2m_step(_p(eps), _p(latents), _p(x0_prev), _p(scaled_next), _p(sigmas_dev), _p(coef_dev), _p(step_dev), nb, n,
                                  C_lat, ld_scaled, float(gs), float(igs), mode, _stream()), "sx_cfg_dpmpp2m_step")


# ---- per-slot denoise step (in-flight batching of the de-tokenizer) ----------------------------------------------------
def _slot_vec(t, G, dtype, what):
    assert t.dtype == dtype and t.is_contiguous() and t.numel() == G and t.is_cuda, f"{what}: {dtype} [{G}] on the device"


def cfg_euler_step_slots(eps, latents, scaled_next, sig_tab, step_dev, n_steps_dev, gs_dev, igs_dev, nb, C_lat, ld_scaled, mode):
    """latents [G, HW, C] fp32, eps [nb*G, HW, C], scaled_next [nb*G, HW, ld_scaled] (or None), rows ordered [branch][slot];
    sig_tab [G, ld_sig] fp32; step / n_steps int32 [G]; gs / igs fp32 [G]. Live slots (0 <= step < n_steps) take one CFG + Euler
    step, bit for bit cfg_euler_step's; parked slots are left untouched."""
    lib = _lib.load()
    G = latents.shape[0]
    n_slot = latents.numel() // G
    f32 = torch.float32
    assert latents.dtype == f32 and latents.is_contiguous() and eps.dtype == f32 and eps.is_contiguous()
    assert eps.numel() == nb * G * n_slot, "eps must hold nb * G slots"
    assert sig_tab.dtype == f32 and sig_tab.is_contiguous() and sig_tab.dim() == 2 and sig_tab.shape[0] == G
    if scaled_next is not None:
        assert scaled_next.dtype == f32 and scaled_next.is_contiguous() and scaled_next.numel() == nb * G * (n_slot // C_lat) * ld_scaled
    _slot_vec(step_dev, G, torch.int32, "step"); _slot_vec(n_steps_dev, G, torch.int32, "n_steps")
    _slot_vec(gs_dev, G, f32, "gs"); _slot_vec(igs_dev, G, f32, "igs")
    check(lib.sx_cfg_euler_step_slots(_p(eps), _p(latents), _p(scaled_next), _p(sig_tab), sig_tab.shape[1], _p(step_dev), _p(n_steps_dev),
                                      _p(gs_dev), _p(igs_dev), nb, G, n_slot, C_lat, ld_scaled, mode, _stream()),
          "sx_cfg_euler_step_slots")


def cfg_dpmpp2m_step_slots(eps, latents, x0_prev, scaled_next, sig_tab, coef_tab, step_dev, n_steps_dev, gs_dev, igs_dev, nb, C_lat,
                           ld_scaled, mode):
    """cfg_euler_step_slots's buffers plus x0_prev [G, HW, C] fp32 and coef_tab [G, ld_sig, 3] fp32 (every slot's (a, b, c) rows, zero
    padded). Live slots take one CFG + DPM-Solver++(2M) step, bit for bit cfg_dpmpp2m_step's; parked slots are left untouched."""
    lib = _lib.load()
    G = latents.shape[0]
    n_slot = latents.numel() // G
    f32 = torch.float32
    assert latents.dtype == f32 and latents.is_contiguous() and eps.dtype == f32 and eps.is_contiguous()
    assert x0_prev.dtype == f32 and x0_prev.is_contiguous() and x0_prev.shape == latents.shape
    assert eps.numel() == nb * G * n_slot, "eps must hold nb * G slots"
    assert sig_tab.dtype == f32 and sig_tab.is_contiguous() and sig_tab.dim() == 2 and sig_tab.shape[0] == G
    assert coef_tab.dtype == f32 and coef_tab.is_contiguous() and tuple(coef_tab.shape) == (G, sig_tab.shape[1], 3)
    if scaled_next is not None:
        assert scaled_next.dtype == f32 and scaled_next.is_contiguous() and scaled_next.numel() == nb * G * (n_slot // C_lat) * ld_scaled
    _slot_vec(step_dev, G, torch.int32, "step"); _slot_vec(n_steps_dev, G, torch.int32, "n_steps")
    _slot_vec(gs_dev, G, f32, "gs"); _slot_vec(igs_dev, G, f32, "igs")
    check(lib.sx_cfg_dpmpp2m_step_slots(_p(eps), _p(latents), _p(x0_prev), _p(scaled_next), _p(sig_tab), _p(coef_tab), sig_tab.shape[1],
                                        _p(step_dev), _p(n_steps_dev), _p(gs_dev), _p(igs_dev), nb, G, n_slot, C_lat, ld_scaled, mode,
                                        _stream()), "sx_cfg_dpmpp2m_step_slots")


def timestep_embedding_slots(t_tab, step_dev, nb, dim, dtype):
    """t_tab [G, ld_t] fp32, step int32 [G] → [nb*G, dim]: row k*G + g embeds t_tab[g, step[g]] (t = 0 for a parked slot)."""
    lib = _lib.load()
    assert t_tab.dtype == torch.float32 and t_tab.is_contiguous() and t_tab.dim() == 2
    G = t_tab.shape[0]
    _slot_vec(step_dev, G, torch.int32, "step")
    out = torch.empty((nb * G, dim), dtype=dtype, device=t_tab.device)
    check(lib.sx_timestep_embedding_slots(_p(t_tab), t_tab.shape[1], _p(step_dev), _p(out), G, nb, dim, _DT[dtype], _stream()),
          "sx_timestep_embedding_slots")
    return out


def denoise_advance(step_dev, n_steps_dev):
    """step[g] += 1 for a live slot, -1 once it reaches n_steps[g]; parked slots stay -1."""
    G = step_dev.numel()
    _slot_vec(step_dev, G, torch.int32, "step"); _slot_vec(n_steps_dev, G, torch.int32, "n_steps")
    check(_lib.load().sx_denoise_advance(_p(step_dev), _p(n_steps_dev), G, _stream()), "sx_denoise_advance")


# ---- KV-cache prefix fork (prefix reuse of in-flight batching) --------------------------------------------------------
KV_CACHE_KEYS = ("kc", "vc", "ks", "vs")


def kv_fork(caches, pairs):
    """Copies cache rows [0, n) of slot ``src`` to slot ``dst`` for every (src, dst, n) of ``pairs``, all layers and heads of a cache
    tensor in ONE sx_kv_fork launch. ``caches``: the LLM's pack (its "kc" / "vc" and, under the FP8 format, "ks" / "vs" tensors: one
    launch each), one cache tensor, or a list of them — [L, G, heads, Tmax, hd] of any dtype, or [L, G, heads, Tmax] (row scales);
    the [Tmax, hd] block of a head must be contiguous, the other axes may be strided. The kernel skips a pair whose src or dst is
    outside [0, G), whose src == dst or whose n <= 0 (include/seedx_hip.h); such pairs are passed on and take no part in the checks
    below. The pairs of a launch are not ordered, so among the others a dst that occurs twice, a slot that is both read and written, and
    n > Tmax raise ValueError. Returns the number of launches."""
    if isinstance(caches, dict):
        caches = [caches[k] for k in KV_CACHE_KEYS if caches.get(k) is not None]
    elif isinstance(caches, torch.Tensor):
        caches = [caches]
    pairs = [(int(s), int(d), int(n)) for s, d, n in pairs]
    assert caches, "kv_fork: no cache tensor"
    G, Tmax = caches[0].shape[1], caches[0].shape[3]
    live = [(s, d, n) for s, d, n in pairs if 0 <= s < G and 0 <= d < G and s != d and n > 0]
    dsts = [d for _, d, _ in live]
    if len(set(dsts)) != len(dsts):
        raise ValueError(f"kv_fork: a slot receives two prefixes in one call: {pairs}")
    if set(dsts) & {s for s, _, _ in live}:
        raise ValueError(f"kv_fork: a slot is both read and written in one call: {pairs}")
    if any(n > Tmax for _, _, n in live):
        raise ValueError(f"kv_fork: a prefix is longer than the cache ({Tmax} rows): {pairs}")
    if not pairs:
        return 0
    lib = _lib.load()
    dev = caches[0].device
    tab = torch.tensor(pairs, dtype=torch.int32).t().contiguous().to(dev)               # [3, n_pairs]: src, dst, n
    for t in caches:
        assert t.is_cuda and t.dim() in (4, 5) and t.shape[1] == G and t.shape[3] == Tmax, "kv_fork: caches of one model"
        es, row = t.element_size(), (t.shape[4] if t.dim() == 5 else 1)
        assert t.stride(3) == row and (t.dim() == 4 or t.stride(4) == 1), "kv_fork: a head's [Tmax, hd] block must be contiguous"
        a = _lib.KvForkArgs(_p(t), _p(tab[0]), _p(tab[1]), _p(tab[2]), t.stride(0) * es, t.stride(1) * es, t.stride(2) * es,
                            len(pairs), t.shape[0], G, t.shape[2], Tmax, row * es)
        check(lib.sx_kv_fork(C.byref(a), _stream()), "sx_kv_fork")
    return len(caches)


# ---- KV-cache rows <-> a linear staging buffer (the host-memory tier of the prefix cache) --------------------------------------
def _kv_cache_list(caches):
    if isinstance(caches, dict):
        return [caches[k] for k in KV_CACHE_KEYS if caches.get(k) is not None]
    return [caches] if isinstance(caches, torch.Tensor) else list(caches)


def _kv_row_bytes(t):
    return (t.shape[4] if t.dim() == 5 else 1) * t.element_size()


def kv_rows_bytes(caches, n_rows):
    """Bytes one job of ``n_rows`` rows (clamped to Tmax; 0 for n_rows <= 0) takes in the staging buffer of ``kv_rows_copy``: for every
    cache tensor outer * inner spans of n_rows * row_bytes bytes, each rounded up to a multiple of 16 — the rule of
    sx_kv_rows_job_bytes (include/seedx_hip.h), computed here without the library."""
    caches = _kv_cache_list(caches)
    outer, Tmax, inner = caches[0].shape[0], caches[0].shape[3], caches[0].shape[2]
    n = min(max(int(n_rows), 0), Tmax)
    return sum(outer * inner * ((n * _kv_row_bytes(t) + 15) // 16 * 16) for t in caches)


def kv_rows_copy(caches, jobs, staging, direction):
    """Moves cache rows [0, n) of slot ``slot`` between the caches and the bytes from ``offset`` of ``staging`` (a contiguous uint8 device
    tensor) for every (slot, n, offset) of ``jobs``: every layer and head of ALL cache tensors in ONE sx_kv_rows_copy launch.
    ``direction`` 0 packs (cache -> staging), 1 unpacks (staging -> cache). ``caches`` as for ``kv_fork``: the LLM's pack, one cache
    tensor or a list of at most four. The layout of a job in staging: spans in the order [tensor][outer][inner], each n * row_bytes bytes
    padded up to a multiple of 16 (``kv_rows_bytes`` gives a job's size; padding bytes are never touched). The kernel skips a job whose
    slot is outside [0, G) or whose n <= 0; such jobs are passed on and take no part in the checks below. The jobs of a launch are not
    ordered, so among the others two unpack jobs into one slot, n > Tmax and overlapping staging ranges raise ValueError; the entry
    point refuses (RuntimeError) offsets that are no multiple of 16, a staging buffer too small for the jobs and more than four tensors."""
    caches = _kv_cache_list(caches)
    jobs = [(int(g), int(n), int(off)) for g, n, off in jobs]
    assert caches, "kv_rows_copy: no cache tensor"
    assert direction in (0, 1), "kv_rows_copy: direction is 0 (pack) or 1 (unpack)"
    outer, G, inner, Tmax = caches[0].shape[:4]
    live = [(g, n, off) for g, n, off in jobs if 0 <= g < G and n > 0]
    if any(n > Tmax for _, n, _ in live):
        raise ValueError(f"kv_rows_copy: a job is longer than the cache ({Tmax} rows): {jobs}")
    if direction == 1 and len({g for g, _, _ in live}) != len(live):
        raise ValueError(f"kv_rows_copy: a slot is unpacked into twice in one call: {jobs}")
    end = 0
    for off, n in sorted((off, n) for _, n, off in live):
        if off < end:
            raise ValueError(f"kv_rows_copy: the staging ranges of two jobs overlap: {jobs}")
        end = off + kv_rows_bytes(caches[:4], n)
    if not jobs:
        return 0
    assert staging.is_cuda and staging.dtype == torch.uint8 and staging.dim() == 1 and staging.is_contiguous(), \
        "kv_rows_copy: staging is a contiguous uint8 device tensor"
    lib = _lib.load()
    a = _lib.KvRowsArgs()
    for i, t in enumerate(caches[:4]):
        assert t.is_cuda and t.dim() in (4, 5) and tuple(t.shape[:4]) == (outer, G, inner, Tmax), "kv_rows_copy: caches of one model"
        es, row = t.element_size(), (t.shape[4] if t.dim() == 5 else 1)
        assert t.stride(3) == row and (t.dim() == 4 or t.stride(4) == 1), "kv_rows_copy: a head's [Tmax, hd] block must be contiguous"
        a.tensor[i] = _lib.KvTensor(t.data_ptr(), t.stride(0) * es, t.stride(1) * es, t.stride(2) * es, row * es, 0)
    host32 = torch.tensor([[g for g, _, _ in jobs], [n for _, n, _ in jobs]], dtype=torch.int32)
    host64 = torch.tensor([off for _, _, off in jobs], dtype=torch.int64)
    dev32, dev64 = host32.to(staging.device), host64.to(staging.device)
    a.slot, a.n_rows, a.offset = _p(dev32[0]), _p(dev32[1]), _p(dev64)
    a.host_slot, a.host_n_rows, a.host_offset = host32[0].data_ptr(), host32[1].data_ptr(), host64.data_ptr()
    a.staging, a.staging_bytes = _p(staging), staging.numel()
    a.n_tensors, a.n_jobs, a.outer, a.G, a.inner, a.Tmax, a.direction = len(caches), len(jobs), outer, G, inner, Tmax, direction
    check(lib.sx_kv_rows_copy(C.byref(a), _stream()), "sx_kv_rows_copy")
    return 1
