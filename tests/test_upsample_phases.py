"""The nearest-2x up-sampler convolution from phase-packed weights (sx_gemm_args.upsample = 2, ops.pack_upsample_phases): a 3x3 conv
over an up-sampled image needs 16 distinct products per input pixel, not 36.

CPU: the index algebra of the pack (borders included) in fp64 against conv2d(interpolate(x)), and the three-plane packer.
GPU: the kernel mode against an fp64 evaluation of the phase formula from the SAME rounded packed weights and 16-bit inputs (only the
kernel is judged; tolerance = tests/test_kernels_gpu.py's fp32-output bound, rel-L2 2e-5), every output pixel written, two launches
equal, the fallback to the 36-tap gather bit for bit, and one loose end-to-end comparison with the 36-tap path. The cases name their
tile (sx_gemm_force_tile 7 / 8 = the 256- / 320-wide ping-pong tile), so that every instantiation of gemm_pp.hip's launch_phases runs:
test_every_phase_kernel_has_a_case compares the case table with the source.

End-to-end figures on MI355X, shape (2, 16, 16, 64, 128), fp16, rel-L2 against fp64 conv(interpolate(x)) of the unpacked weights:
see profiles/upsample_phases.md."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

TOL_F32 = 2e-5          # tests/test_kernels_gpu.py TOL[torch.float32], the bound of test_conv3x3's fp32-output case
TOL_16 = {torch.float16: 6e-4, torch.bfloat16: 4e-3}     # the same table's 16-bit output bounds (= output rounding)

# (B, H, W, Cin, Cout, tile): 512 rows per phase = two tiles, one k-tile per tap | H != W, two k-tiles per tap, the 320-wide tile
SHAPES = [(2, 16, 16, 64, 128, 7), (1, 16, 32, 128, 320, 8)]
BN_OF_TILE = {7: 256, 8: 320}


def _rnd(shape, dtype, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale).to(dtype)


def _phase_conv(x_nhwc, wp, bias=None):
    """fp64 evaluation of the phase formula. x: [B, H, W, C]; wp: [4, Cout, 4*C] → [B, 2H, 2W, Cout]:
    y[b, 2i+a, 2j+c, n] = bias[n] + sum_{u,v,ch} wp[2a+c][n][(2u+v) C + ch] x[b, i+a-1+u, j+c-1+v, ch], zero outside the image."""
    B, H, W, C = x_nhwc.shape
    Cout = wp.shape[1]
    xp = F.pad(x_nhwc.double(), (0, 0, 1, 1, 1, 1))                   # index + 1 on both image axes
    w = wp.double().view(4, Cout, 2, 2, C)
    y = torch.zeros(B, 2 * H, 2 * W, Cout, dtype=torch.float64, device=x_nhwc.device)
    for a in (0, 1):
        for c in (0, 1):
            acc = torch.zeros(B, H, W, Cout, dtype=torch.float64, device=x_nhwc.device)
            for u in (0, 1):
                for v in (0, 1):
                    acc += xp[:, a + u:a + u + H, c + v:c + v + W] @ w[2 * a + c, :, u, v].t()
            y[:, a::2, c::2] = acc
    return y if bias is None else y + bias.double()


def _conv_interp(x_nhwc, w_flat, bias=None):
    """fp64 conv2d(interpolate(x, 2, nearest), w, padding=1) → [B, 2H, 2W, Cout]"""
    Cout, C = w_flat.shape[0], x_nhwc.shape[-1]
    x = F.interpolate(x_nhwc.double().permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
    w = w_flat.double().view(Cout, 3, 3, C).permute(0, 3, 1, 2)
    return F.conv2d(x, w, None if bias is None else bias.double(), padding=1).permute(0, 2, 3, 1)


def _rel(x, ref):
    return ((x.double() - ref.double()).norm() / ref.double().norm()).item()


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C,Cout", [(1, 3, 5, 4, 6), (2, 4, 4, 8, 3)])
def test_pack_index_algebra_fp64(B, H, W, C, Cout):
    from seedx_amd import ops
    x = _rnd((B, H, W, C), torch.float64, seed=1)
    w = _rnd((Cout, 9 * C), torch.float64, 0.3, seed=2)
    wp = ops.pack_upsample_phases(w, rounded=False)
    assert wp.shape == (4, Cout, 4 * C) and wp.dtype == torch.float64
    ref = _conv_interp(x, w)
    d = (_phase_conv(x, wp) - ref).abs().max().item()
    print(f"phase formula vs conv(interpolate), fp64, {(B, H, W, C, Cout)}: max abs diff {d:.3e}, max |y| {ref.abs().max().item():.3e}")
    assert d <= 1e-12 * ref.abs().max().item()


def test_pack_rounds_once_and_layout():
    from seedx_amd import ops
    w = _rnd((6, 9 * 8), torch.float32, 0.3, seed=3)
    s64 = ops.pack_upsample_phases(w, rounded=False)
    for dt in (torch.float16, torch.bfloat16):
        wp = ops.pack_upsample_phases(w, dtype=dt)
        assert wp.shape == (4, 6, 32) and wp.dtype == dt and wp.is_contiguous()
        assert torch.equal(wp, s64.to(dt))                                       # one rounding of the fp64 sum
    w16 = w.to(torch.float16)
    assert ops.pack_upsample_phases(w16).dtype == torch.float16                  # default: the weight's own dtype


def test_pack_three_planes():
    """[hi | lo | hi] per tap; hi + lo reproduces the fp32-rounded sum to bf16^2 precision: hi = s (1 + d1), lo = (s - hi)(1 + d2),
    |d| <= 2^-8 (bf16 carries 8 significant bits) → |s - hi - lo| <= 2^-16 |s|."""
    from seedx_amd import ops
    Cout, C = 5, 8
    w = _rnd((Cout, 9 * C), torch.float32, 0.3, seed=4)
    s32 = ops.pack_upsample_phases(w, rounded=False).float().view(4, Cout, 4, C)
    wp = ops.pack_upsample_phases(w, planes=3)
    assert wp.shape == (4, Cout, 12 * C) and wp.dtype == torch.bfloat16 and wp.is_contiguous()
    pl = wp.view(4, Cout, 4, 3, C)
    hi, lo, hi2 = pl[..., 0, :], pl[..., 1, :], pl[..., 2, :]
    assert torch.equal(hi, hi2) and torch.equal(hi, s32.to(torch.bfloat16))
    err = (hi.double() + lo.double() - s32.double()).abs()
    assert bool((err <= 2.0 ** -16 * s32.double().abs()).all())


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
def _run(ops, x, wp, bias, n_valid=0, out_dtype=torch.float32, tile=-1):
    """Two launches of the phase mode into NaN-filled outputs → the first output, after the written-everywhere and repeatability checks.
    tile: 7 / 8 forces the 256- / 320-wide ping-pong tile, -1 leaves the choice to the cost model."""
    from seedx_amd import _lib
    B, H, W, _ = x.shape
    n_store = n_valid or wp.shape[1]
    outs = []
    lib = _lib.load()
    assert lib.sx_gemm_force_tile(tile) == 0
    try:
        for _ in range(2):
            out = torch.full((B * 4 * H * W, n_store), float("nan"), dtype=out_dtype, device=x.device)
            y = ops.conv3x3(x, None, bias=bias, upsample=True, out_dtype=out_dtype, n_valid=n_valid, w_phases=wp, out=out)
            assert y.data_ptr() == out.data_ptr() and y.shape == (B, 4 * H * W, n_store)
            outs.append(out)
    finally:
        lib.sx_gemm_force_tile(-1)
    assert not torch.isnan(outs[0]).any(), "an output pixel was not written"
    assert torch.equal(outs[0], outs[1])
    return outs[0].view(B, 2 * H, 2 * W, n_store)


@pytest.mark.gpu
@pytest.mark.parametrize("out16", [False, True])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B,H,W,Cin,Cout,tile", SHAPES)
def test_phase_mode(dev, dtype, B, H, W, Cin, Cout, tile, out16):
    """fp32 output: the issue's cases at test_conv3x3's fp32 bound. 16-bit output (the kernel's other store form, same operands): the
    output-rounding bound of the same table."""
    from seedx_amd import ops
    assert ops.upsample_phases_ok(B, H, W)
    x = _rnd((B, H, W, Cin), dtype, seed=16).to(dev)
    w = _rnd((Cout, 9 * Cin), dtype, 0.05, seed=17).to(dev)
    bias = _rnd((Cout,), torch.float32, seed=18).to(dev)
    wp = ops.pack_upsample_phases(w)
    got = _run(ops, x, wp, bias, out_dtype=dtype if out16 else torch.float32, tile=tile)
    e = _rel(got, _phase_conv(x, wp, bias))
    print(f"phase mode {dtype} {(B, H, W, Cin, Cout)} tile {tile} {'16-bit' if out16 else 'fp32'} out: rel-L2 vs fp64 phase formula {e:.3e}")
    assert e < (TOL_16[dtype] if out16 else TOL_F32)


def test_every_phase_kernel_has_a_case():
    """gemm_pp.hip's launch_phases instantiates the phase mode per (tile width, fp32 | 16-bit output), for both dtypes; test_phase_mode
    runs each of them (tests/test_gemm_matrix_gpu.py's table stops at launch_t)."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "seed-x_amd", "csrc", "gemm_pp.hip")).read()
    body = src[src.index("static int launch_phases("):src.index("static int launch_t(")]
    assert "launch_one<TT, BNV, SX_A_CONV3X3_PH, O32, SX_ACT_NONE, false>" in body and body.count("launch_one<") == 1
    inst = sorted((int(bn), o32 == "true") for bn, o32 in re.findall(r"PH_CASE\((\d+), (true|false)\);", body))
    assert inst == sorted((BN_OF_TILE[s[5]], o32) for s in SHAPES for o32 in (False, True)), inst


@pytest.mark.gpu
def test_phase_mode_three_plane_layout(dev):
    """The fp32-grade VAE's operands: activations [hi | hi | lo], weights [hi | lo | hi] per tap → Cin = 3 * 64, N below a tile."""
    from seedx_amd import ops
    B, H, W, C, Cout = 1, 16, 16, 64, 64
    x32 = _rnd((B, H, W, C), torch.float32, seed=21)
    hi = x32.to(torch.bfloat16)
    lo = (x32 - hi.float()).to(torch.bfloat16)
    x = torch.cat([hi, hi, lo], dim=-1).contiguous().to(dev)
    w = _rnd((Cout, 9 * C), torch.float32, 0.05, seed=22).to(dev)
    bias = _rnd((Cout,), torch.float32, seed=23).to(dev)
    wp = ops.pack_upsample_phases(w, planes=3)
    assert wp.shape == (4, Cout, 4 * 192)
    got = _run(ops, x, wp, bias)
    e = _rel(got, _phase_conv(x, wp, bias))
    print(f"phase mode, three bf16 planes {(B, H, W, 3 * C, Cout)}: rel-L2 vs fp64 phase formula {e:.3e}")
    assert e < TOL_F32


@pytest.mark.gpu
def test_phase_mode_n_valid(dev):
    from seedx_amd import ops
    B, H, W, Cin, Cout = 1, 16, 16, 64, 16
    x = _rnd((B, H, W, Cin), torch.bfloat16, seed=24).to(dev)
    w = _rnd((Cout, 9 * Cin), torch.bfloat16, 0.05, seed=25).to(dev)
    bias = _rnd((Cout,), torch.float32, seed=26).to(dev)
    wp = ops.pack_upsample_phases(w)
    got = _run(ops, x, wp, bias, n_valid=4)
    e = _rel(got, _phase_conv(x, wp, bias)[..., :4])
    print(f"phase mode n_valid = 4: rel-L2 vs fp64 phase formula {e:.3e}")
    assert got.shape[-1] == 4 and e < TOL_F32


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W", [(2, 16, 16),      # a tile lies inside one sample: the per-sample row joins the bias vector once
                                   (4, 8, 8)])       # 64 pixels per sample: a tile spans four samples, added per row
def test_phase_mode_bias2d(dev, B, H, W):
    """The per-sample add follows the OUTPUT image (bias2d_rows = Hout * Wout), not the (phase, b, i, j) order of the GEMM rows."""
    from seedx_amd import ops
    Cin, Cout = 64, 64
    x = _rnd((B, H, W, Cin), torch.float16, seed=30).to(dev)
    w = _rnd((Cout, 9 * Cin), torch.float16, 0.05, seed=31).to(dev)
    bias = _rnd((Cout,), torch.float32, seed=32).to(dev)
    b2 = _rnd((B, Cout), torch.float32, seed=33).to(dev)
    wp = ops.pack_upsample_phases(w)
    got = ops.conv3x3(x, None, bias=bias, bias2d=b2, upsample=True, out_dtype=torch.float32, w_phases=wp).view(B, 2 * H, 2 * W, Cout)
    e = _rel(got, _phase_conv(x, wp, bias) + b2.double()[:, None, None, :])
    print(f"phase mode with bias2d {(B, H, W, Cin, Cout)}: rel-L2 vs fp64 phase formula {e:.3e}")
    assert e < TOL_F32


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_gate_fails_keeps_36_tap_path(dev, dtype):
    """B*H*W = 120 is no multiple of the tile: the call runs today's gather, bit for bit, whatever phase weights it is handed."""
    from seedx_amd import ops
    B, H, W, Cin, Cout = 1, 10, 12, 64, 64
    assert not ops.upsample_phases_ok(B, H, W)
    x = _rnd((B, H, W, Cin), dtype, seed=27).to(dev)
    w = _rnd((Cout, 9 * Cin), dtype, 0.05, seed=28).to(dev)
    bias = _rnd((Cout,), torch.float32, seed=29).to(dev)
    old = ops.conv3x3(x, w, bias=bias, upsample=True, out_dtype=torch.float32)
    new = ops.conv3x3(x, w, bias=bias, upsample=True, out_dtype=torch.float32, w_phases=ops.pack_upsample_phases(w))
    assert torch.equal(old, new)
    assert _rel(old.view(B, 2 * H, 2 * W, Cout), _conv_interp(x, w, bias)) < TOL_F32


@pytest.mark.gpu
def test_end_to_end_against_unpacked_weights(dev):
    """New mode vs the 36-tap path, both against fp64 conv(interpolate(x)) of the UNPACKED fp16 weights. The phase weights carry one
    more rounding (relative 2^-11 per summed weight), about the size of the activation rounding already present: new <= 2 x old."""
    from seedx_amd import ops
    B, H, W, Cin, Cout = 2, 16, 16, 64, 128
    x32 = _rnd((B, H, W, Cin), torch.float32, seed=16)
    w32 = _rnd((Cout, 9 * Cin), torch.float32, 0.05, seed=17)
    x, w = x32.to(torch.float16).to(dev), w32.to(torch.float16).to(dev)
    ref = _conv_interp(x32.to(dev), w32.to(dev))                   # unrounded operands: both paths carry their operand roundings
    old = ops.conv3x3(x, w, upsample=True, out_dtype=torch.float32).view(B, 2 * H, 2 * W, Cout)
    new = ops.conv3x3(x, w, upsample=True, out_dtype=torch.float32, w_phases=ops.pack_upsample_phases(w)).view(B, 2 * H, 2 * W, Cout)
    e_old, e_new = _rel(old, ref), _rel(new, ref)
    print(f"end to end fp16 {(B, H, W, Cin, Cout)}: rel-L2 vs fp64 conv(interpolate(x)), 36-tap {e_old:.3e}, phase mode {e_new:.3e}")
    assert e_new <= 2 * e_old
