"""The glue kernels between the pinned GEMM / attention / norm kernels: csrc/elementwise.hip, csrc/preproc.hip and the small helpers of
csrc/decode.hip (sx_rope_kv_append(_b), sx_embedding, sx_scatter_rows(_step | _spec)), in the manner of tests/test_attn_norm_matrix_gpu.py
(GBuf, same_bits, stops_on_gpu_fault, _nanbuf and the NaN patterns are imported from the sibling matrix files).

Every case drives the C entry point through _lib, so every stride and leading dimension is free, and checks
  * that nothing outside the logical output is written: outputs live in guard buffers (GBuf; Guard for uint8 / int32 outputs) whose other
    bytes must be bit-unchanged: pad columns C .. ld, the rows in front and behind, rows that a contract drops;
  * that nothing outside a logical input is read: float inputs are views into NaN-filled buffers;
  * that a second identical launch gives the same bits;
  * that no index that reaches a kernel leaves its array: embedding ids, scatter rows, idx_dev and the Euler step index are in range; the
    only out-of-range values are the negative / too-large `step` and `pos` that the kernels' contracts drop.
Every kernel here is a grid-stride loop behind a grid cap (grid_for / gs_grid: 4096 x 256 threads; preproc.hip: 8192 x 256; sx_halo_pack:
65536 x 256); the cases marked `cap=` are large enough for the second trip of the loop (CAP_CASES; tests/test_cpu_suite.py holds them against
the caps parsed from the sources, and the case tables against every hipLaunchKernelGGL of the three files).

EXACT GROUP: bit for bit against torch on the same operands, random normal data (a wrong index cannot coincide with the right value).
EXACT holds the number of differing elements per kernel (0 everywhere, or the test fails).

BOUNDED GROUP: against an fp64 reference computed with torch from the same fp32 / 16-bit operands, element by element. U32 = 2^-24 is the unit
roundoff of fp32 (half an ulp; an instruction documented to 1 ulp counts 2), u16 = 2^-11 (fp16) / 2^-8 (bf16). `rnd(ref, dt)` is the output
rounding u_out |ref|, or half a unit of the smallest subnormal of fp16 (2^-25) where that is larger; for bf16 and fp32 the floor is 2^-126,
the smallest normal (a hardware exp, reciprocal or product may flush below it). WORST collects the worst |diff| / bound per (kernel, type).

1. sx_avgpool_tokens: |got - ref| <= (k + 1) 2^-24 mean_j |x_j|. One sequential fp32 sum of k terms: k - 1 additions (the first is exact),
   each half an ulp of a partial sum <= sum |x|; the rounding of 1 / k and the product: 2. In units of 2^-24 sum |x| / k that is k + 1.

2. sx_silu_cast: |got - ref| <= u16 |ref| + C_SILU (1 + |x|) 2^-24 |ref|, C_SILU = 6, counted on silu_f, x / (1 + __expf(-x)), the form of every
   epilogue: __expf is v_exp_f32 of x * log2(e): the rounding of the constant and of the product are 2^-24 relative on an argument of
   |x| log2(e) each, i.e. |x| 2^-24 relative on the exponential each: 2 |x|. v_exp_f32 (1 ulp): 2; the addition: 1; the division (under
   -ffast-math a 1-ulp reciprocal and a product): 3; an error of the exponential enters the quotient with weight e / (1 + e) <= 1.
   6 + 2 |x| <= 6 (1 + |x|). Planted: +-0, +-1e-4, +-20, +-88, +-89, +-104 and -inf. At -88 silu is -5.3e-37 and at -89 -2.0e-37, normal numbers of
   bf16 above the floor: silu_f gave -0 at both (the reciprocal of 1 + e^88 = 1.7e38 is subnormal and v_rcp_f32 flushes it; __expf(89) is
   inf), which this matrix found at -88; silu_cast_kernel now takes the exponential and the quotient in fp64 and rounds once (inside the
   count above with room). At -104 the fp64 value -7e-44 is below the floor. At -inf torch gives NaN (-inf * 0) and so does the kernel
   (-inf / inf): asserted.

3. sx_l2norm_dim1: |got - ref| <= (T + 4) 2^-24 |ref|. The sum of squares has T products and T - 1 additions of non-negative terms: T 2^-24
   relative at most, which the root halves: T / 2; the root: 2 (1 ulp); max(norm, eps): exact; the division: 1; the remaining T / 2 + 1 is
   slack. A column of zeros and a column of 1e-20 (its squares are fp32 subnormals) both take the eps branch: y = x / eps.

4. sx_rope_kv_append(_b) (rope_kv_append_kernel<F16 | BF16>): the reference rounds cos / sin to the activation type first, as the kernel does,
   then rotates in fp64: |got - ref| <= u16 |ref| + 2 2^-24 (|x1 c| + |x2 s|): one product rounding and the rounding of the fma (or two
   products and the sum: the sum's half ulp is of |ref| <= |x1 c| + |x2 s|). V rows are bit copies. A position outside [0, Tmax) writes no
   cache row and rotates q by table row 0 (cos 1, sin 0: q unchanged, bit for bit).

5. sx_cfg_euler_step. d = sigma_next - sigma (rounded once: 1 relative), gs / igs the guidance scales.
   mode 0 (e = e_u + gs (e_t - e_u); x' = x + e d), M = |e_u| + gs |e_t - e_u|:
       |got - ref| <= C0 2^-24 (|x| + |d| M),  C0 = 6
   the subtraction (1, times gs <= M), gs * (..) + e_u as product and sum (2 of <= M), d (1 of |e d|), e * d + x as product and sum (1 of
   |e d|, 1 of |x'| <= |x| + |d| M): |x| carries 1, |d| M carries 5 (3 where the compiler fuses); 6 covers both.
   mode 1 (x0_b = x - sigma e_b for b = t, i, u; x0 = x0_u + gs (x0_t - x0_i) + igs (x0_i - x0_u); e = (x0 - x) / (-sigma); x' = x + e d),
   S = (1 + igs) |e_u| + (gs + igs) |e_i| + gs |e_t| (so that |e| <= S), A_b = |x| + sigma |e_b| >= |x0_b|:
       |got - ref| <= C1 2^-24 (|x| + sigma S) (1 + |d| / sigma),  C1 = max(4 (1 + gs + igs), 13)
   each x0_b: product and sum, 2 A_b. The differences: 2 (A_t + A_i) inherited + 1 of their own magnitude sigma (|e_t| + |e_i|); times gs
   and the product's rounding; the two sums into x0 add 1 of A_u + gs sigma (..) and 1 of |x0| each. Collected:
   err(x0) <= 2^-24 (4 (1 + gs + igs) |x| + 6 sigma S). x0 - x: + 1 sigma S. The division by -sigma (reciprocal 2, product 1): 3 S, so
   err(e) <= 2^-24 (4 (1 + gs + igs) |x| / sigma + 10 S). x' = x + e d: |d| err(e) + (d: 1, product: 1) |d| S + 1 (|x| + |d| S)
   = 2^-24 (|x| + (|d| / sigma) (4 (1 + gs + igs) |x| + 13 sigma S)). This is where the division cancels: the roundings of x0_b are of |x|,
   not of sigma |e|, and come back divided by sigma, with weight |d| / sigma (1 at the last step, where sigma_next = 0).
   The scaled copy x' rsqrt(sigma_next^2 + 1) is judged against the fp64 product of the reference: the bound above times the factor, plus
   3 2^-24 |ref|: the argument's fma enters at half weight (0.5), v_rsq_f32 (1.5 allowed of its documented 1 ulp = 2), the product (1).
   All 50 steps of euler_tables(50) are walked with fixed random eps per step and the latents carried from launch to launch; the fp64
   reference of every step starts from the kernel's own previous output, so each step is judged alone; a free-running fp64 chain is carried
   beside it and its final distance printed, not asserted (NOTES).

6. sx_timestep_embedding: the reference is fp64 throughout from the fp32 t: f_j = exp(-ln(10000) j / half), cos / sin (t f_j).
       |got - ref| <= u_out |ref| + 4 E32 2^-24 (|t f_j| + 1)
   E32 is the ONE MEASURED yardstick of this file, and it is measured on the op being replaced, not on the kernel: the test computes on the
   CPU E32(dim) = max |restatement32 - ref| / (2^-24 (|t f_j| + 1)) with restatement32 = oracle.restated_unet.timestep_embedding in fp32 on the
   same t and dim (4.6 at dim 256 and 5.2 at dim 320 with torch's CPU kernels). The factor 4 covers the few-ulp exp, product and range
   reduction that a device function may legitimately take where torch's are within 1 ulp.
"""
import ctypes as C
import math
import os
import re
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from tests.test_gemm_matrix_gpu import BF16, DTYPES, F16, NAN16_IN, NAN32_IN, U32, _nanbuf
from tests.test_gemv_matrix_gpu import GBuf, same_bits, stops_on_gpu_fault

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "seed-x_amd", "csrc")

F32 = torch.float32
ALL_DT = {"f32": F32, "f16": F16, "bf16": BF16}
U_OUT = {F16: 2.0 ** -11, BF16: 2.0 ** -8, F32: U32}
FLOOR = {F16: 2.0 ** -25, BF16: 2.0 ** -126, F32: 2.0 ** -126}
C_SILU = 6.0
C0_EULER = 6.0
GS, IGS = 7.5, 1.5                   # the guidance scales of the pipelines; both exact in fp32
WORST = {}                           # (kernel, type) -> worst |diff| / bound          (bounded group)
EXACT = {}                           # (kernel, type) -> differing elements            (exact group)
NOTES = {}
assert (NAN16_IN, NAN32_IN) == (0x7FFF, 0x7FFFFFFF)


def c1_euler(gs, igs):
    return max(4.0 * (1.0 + gs + igs), 13.0)


def rnd(ref, dt):
    return torch.clamp(U_OUT[dt] * ref.abs(), min=FLOOR[dt])


def sx_code(dt):
    return {F16: 0, BF16: 1, F32: 2}[dt]


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def gen_of(cid, dev):
    return torch.Generator(device=dev).manual_seed(zlib.crc32(cid.encode()))


def nan_lead(t, pad=256):
    """t (contiguous order) at the head of a NaN-filled buffer of its dtype."""
    buf = _nanbuf(t.numel() + pad, t.dtype, t.device)
    buf[:t.numel()] = t.reshape(-1)
    return buf


class Guard:
    """GBuf for integer outputs (uint8, int32): `n` elements inside a buffer of a fixed pattern; `allowed` marks what a launch may write."""
    PATTERN = {torch.uint8: 0xA5, torch.int32: -1515870811}

    def __init__(self, n, dtype, dev, before=64, after=512):
        self.n, self.before, self.pat = n, before, self.PATTERN[dtype]
        self.buf = torch.full((before + n + after,), self.pat, dtype=dtype, device=dev)
        self.body = self.buf[before:before + n]
        self.allowed = torch.zeros(self.buf.numel(), dtype=torch.bool, device=dev)

    def allow(self):
        return self.allowed[self.before:self.before + self.n]

    def ptr(self):
        return self.body.data_ptr()

    def check(self, what):
        bad = (self.buf != self.pat) & ~self.allowed
        assert int(bad.sum()) == 0, f"{what}: {int(bad.sum())} elements outside the documented extent were written; first at element " \
                                    f"{int(bad.nonzero()[0, 0]) - self.before} of {self.n}"


def held(key, got, ref, bound, what):
    """Every element within its bound; records and returns the worst ratio."""
    d = (got - ref).abs()
    ratio = d / bound
    worst = float(ratio.max()) if ratio.numel() else 0.0
    WORST[key] = max(WORST.get(key, 0.0), worst)
    if not worst <= 1.0:
        i = int(torch.nan_to_num(ratio, nan=float("inf")).argmax())
        flat = lambda t: t.reshape(-1)[i]
        raise AssertionError(f"{what} [{key}]: {int((~(ratio <= 1.0)).sum())} of {ratio.numel()} elements beyond the fp64 bound; worst at flat index {i}: "
                             f"got {float(flat(got))!r}, ref {float(flat(ref))!r}, |diff| {float(flat(d)):.3e} > bound {float(flat(bound)):.3e}")
    return worst


def exact(key, got, ref, what):
    """Bit for bit; records the number of differing elements."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if got.dtype.is_floating_point:
        ib = {2: torch.int16, 4: torch.int32}[got.element_size()]
        diff = got.contiguous().view(ib) != ref.contiguous().view(ib)
    else:
        diff = got != ref
    n = int(diff.sum())
    EXACT[key] = EXACT.get(key, 0) + n
    assert n == 0, f"{what} [{key}]: {n} of {got.numel()} elements differ; first at flat index {int(diff.reshape(-1).nonzero()[0, 0])}"


def twice(fn, what):
    """fn() launches into fresh buffers and returns the logical outputs (a tensor or a tuple): two launches, the same bits."""
    a, b = fn(), fn()
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    for x, y in zip(a, b):
        if x is None:
            continue
        assert torch.equal(x, y) if not x.dtype.is_floating_point else same_bits(x.contiguous(), y.contiguous()), f"{what}: two identical launches differ"
    return a[0] if len(a) == 1 else a


def ok(st, what):
    from seedx_amd import _lib
    _lib.check(st, what)
    torch.cuda.synchronize()


def lib_():
    from seedx_amd import _lib
    return _lib.load()


# ----------------------------------------------------------------------------------------------------------------------------
# the case tables (pure data: tests/test_cpu_suite.py reads them without a GPU). `cap`: the trip count that must exceed the grid
# ----------------------------------------------------------------------------------------------------------------------------
CAST_N = (1, 3, 4, 5, 1001, 4 * 1048576 + 259)
CAST = [dict(id=f"cast-{s}-{d}-n{n}", s=s, d=d, n=n, cap=n // 4 if n > 4 * 1048576 else 0) for s in ALL_DT for d in ALL_DT for n in CAST_N]
SPLIT = [dict(id=f"split-r{role}-{r}x{c}", role=role, rows=r, cols=c, cap=r * c // 4 if r * c // 4 > 1048576 else 0)
         for role in (0, 1) for r, c in ((1, 4), (7, 12), (3, 1000), (1025, 4100))]
COPY2D = [dict(id=f"copy2d-{r}x{c}", rows=r, cols=c, cap=r * c // 4 if r * c // 4 > 1048576 else 0)
          for r, c in ((5, 4), (5, 64), (5, 1000), (0, 64), (4200, 1000))]
ADD = [dict(id=f"add-n{n}", n=n, cap=n if n > 1048576 else 0) for n in (1, 257, 1048576 + 257)]
PATCHIFY = [dict(id=f"patchify-{dt}-B{B}S{S}P{P}K{K}", dt=dt, B=B, S=S, P=P, Kpad=K, cap=B * (S // P) ** 2 * K if B * (S // P) ** 2 * K > 1048576 else 0)
            for dt in DTYPES for B, S, P, K in ((1, 14, 14, 588), (2, 28, 14, 640), (1, 6, 2, 16), (3, 448, 14, 640))]
IM2COL = [dict(id=f"im2col-{dt}-B{B}H{H}W{W}C{Ci}K{K}", dt=dt, B=B, H=H, W=W, Cin=Ci, Kpad=K, cap=B * H * W * K if B * H * W * K > 1048576 else 0)
          for dt in DTYPES for B, H, W, Ci, K in ((1, 1, 1, 4, 64), (2, 5, 4, 6, 64), (1, 3, 7, 8, 72), (2, 96, 96, 6, 64))]
LAYOUT = [dict(id=f"layout-B{B}C{Cc}HW{HW}", B=B, C=Cc, HW=HW, cap=B * Cc * HW if B * Cc * HW > 1048576 else 0)
          for B, Cc, HW in [(2, Cc, HW) for Cc in (4, 8, 5) for HW in (1, 64, 1000)] + [(2, 8, 70000)]]
HALO = [dict(id=f"halo-B{B}Hl{Hl}W{W}C{Cc}-p{int(p)}n{int(n)}l{l}b{b}", B=B, Hl=Hl, W=W, C=Cc, prev=p, next=n, left=l, bottom=b, cap=0)
        for B, Hl, W in ((1, 1, 1), (2, 3, 5)) for Cc in (8, 24) for p in (False, True) for n in (False, True) for l in (0, 1) for b in (0, 1)]
HALO.append(dict(id="halo-big", B=1, Hl=4095, W=4095, C=8, prev=True, next=True, left=1, bottom=1, cap=4097 * 4096))
ADD_I32 = [dict(id=f"add_i32-n{n}", n=n) for n in (1, 5, 64)]
EMBED = [dict(id=f"embed-{dt}-T{T}-dim{dim}", dt=dt, T=T, dim=dim, cap=T * dim if T * dim > 1048576 else 0)
         for dt in DTYPES for T, dim in ((7, 8), (7, 64), (7, 5120), (210, 5120))]
SCATTER = [dict(id=f"scatter-n{n}-dim{dim}", n=n, dim=dim, R=R, cap=n * dim if n * dim > 1048576 else 0)
           for n, dim, R in ((5, 96, 9), (0, 96, 9), (1, 5120, 3), (300, 4096, 311))]
SCATTER_STEP = [dict(id=f"scatter_step-dim{dim}", dim=dim, rows=4, cap=5 * dim if 5 * dim > 1048576 else 0) for dim in (8, 5120, 250000)]
SCATTER_SPEC = [dict(id=f"scatter_spec-dim{dim}-tok{int(tok)}", dim=dim, rows=6, tok=tok, cap=15 * dim if 15 * dim > 1048576 else 0)
                for dim, tok in ((8, True), (5120, True), (5120, False), (80000, True))]
LUT = [dict(id=f"lut-{corner}", H=37, W=53, Hc=11, Wc=17, corner=corner, cap=0) for corner in ("tl", "tr", "bl", "br")]
LUT.append(dict(id="lut-big", H=1450, W=1450, Hc=1449, Wc=1449, corner="br", cap=1449 * 1449))
TO_U8 = [dict(id="to_u8-ties", H=16, W=64, cap=0), dict(id="to_u8-big", H=1449, W=1449, cap=1449 * 1449)]
RESAMPLE = [dict(id=f"resample-C{Cc}-{Hi}x{Wi}-to-{Ho}x{Wo}-{rs}", C=Cc, Hin=Hi, Win=Wi, Hout=Ho, Wout=Wo, rs=rs,
                 cap=Ho * Wo if Ho * Wo > 2097152 else 0)
            for Cc, Hi, Wi, Ho, Wo, rs in ((1, 9, 13, 9, 7, "bicubic"), (1, 9, 13, 9, 20, "bilinear"), (1, 9, 13, 5, 13, "bicubic"), (1, 9, 13, 21, 13, "bilinear"),
                                           (1, 9, 13, 6, 7, "bicubic"), (3, 9, 13, 9, 7, "bilinear"), (3, 9, 13, 5, 13, "bicubic"), (3, 9, 13, 12, 20, "bicubic"),
                                           (1, 10, 10, 1449, 1449, "bicubic"))]
MARKER = [dict(id=f"marker-T{T}-{v}", T=T, v=v) for T in (1, 255, 256, 257, 4097) for v in ("straddle", "edges", "random")]

AVGPOOL = [dict(id=f"avgpool-k{k}-B{B}L{L}D{D}", k=k, B=B, L=L, D=D) for k in (1, 4, 64) for B, L, D in ((1, 4, 1), (2, 256, 96), (1, 64, 5120)) if L % k == 0]
SILU = [dict(id=f"silu-{dt}-n{n}", dt=dt, n=n, cap=n if n > 1048576 else 0) for dt in DTYPES for n in (1, 1280, 1048576 + 257)]
L2NORM = [dict(id=f"l2norm-B{B}T{T}D{D}", B=B, T=T, D=D) for B, T, D in ((1, 1, 1), (3, 24, 256), (2, 64, 4097), (2, 3, 40))]
ROPE_TMAX = 16


def rope_cases():
    out = []
    T_ = ROPE_TMAX
    for dt in DTYPES:
        for D in (64, 128, 112):
            for G, T, pos, b in ((1, 1, [0], False), (1, 5, [T_ - 2], False), (1, 5, [7], True), (1, 1, [T_ - 1], True),
                                 (3, 1, [7, -1, T_ - 1], True), (3, 5, [0, T_ - 2, -1], True)):
                out.append(dict(id=f"rope-{dt}-D{D}-G{G}T{T}-pos{'_'.join(map(str, pos))}-{'b' if b else 'single'}", dt=dt, D=D, G=G, T=T, H=2, Tmax=T_, pos=pos,
                                b=b, pad=64 if b else 0, cap=0))
        out.append(dict(id=f"rope-{dt}-cap", dt=dt, D=128, G=1, T=600, H=32, Tmax=640, pos=[37], b=True, pad=64, cap=600 * 32 * 64))
    return out


ROPE = rope_cases()
EULER = [dict(id=f"euler-mode{mode}-ld{ld}-{'scaled' if sc else 'noscaled'}", mode=mode, ld=ld, scaled=sc, HW=128, C=4)
         for mode in (0, 1) for ld, sc in ((4, True), (8, True), (4, False))]
TS_T = (0.0, 1.0, 20.5, 448.0, 981.0, 999.0, 1024.0)
TSEMB = [dict(id=f"tsemb-{o}-dim{dim}-{'rows' if idx is None else 'idx' + str(idx)}", o=o, dim=dim, idx=idx)
         for o in ALL_DT for dim in (2, 256, 320) for idx in (None, 0, 3, 6)]

# what each table launches: (kernel name, template arguments as written in the source)
KERNEL_OF = dict(
    CAST=lambda c: {("cast_kernel", "")}, SPLIT=lambda c: {("split_bf16_kernel", "")}, COPY2D=lambda c: {("copy2d_kernel", "")},
    ADD=lambda c: {("add_kernel", "")}, PATCHIFY=lambda c: {("patchify_kernel", c["dt"].upper())}, IM2COL=lambda c: {("im2col3x3_kernel", c["dt"].upper())},
    LAYOUT=lambda c: {("nchw_to_nhwc_kernel", ""), ("nhwc_to_nchw_kernel", "")}, HALO=lambda c: {("halo_pack_kernel", "")},
    ADD_I32=lambda c: {("add_i32_kernel", "")}, EMBED=lambda c: {("embedding_kernel", c["dt"].upper())}, SCATTER=lambda c: {("scatter_rows_kernel", "")} if c["n"] else set(),
    SCATTER_STEP=lambda c: {("scatter_rows_step_kernel", "")}, SCATTER_SPEC=lambda c: {("scatter_rows_spec_kernel", "")},
    LUT=lambda c: {("u8_to_chw_lut_kernel", "")}, TO_U8=lambda c: {("chw_to_u8_image_kernel", "")},
    RESAMPLE=lambda c: ({("resample_h_kernel", str(c["C"]))} if c["Wout"] != c["Win"] else set()) | ({("resample_v_kernel", str(c["C"]))} if c["Hout"] != c["Hin"] else set()),
    MARKER=lambda c: {("marker_mask_kernel", "")}, AVGPOOL=lambda c: {("avgpool_tokens_kernel", "")}, SILU=lambda c: {("silu_cast_kernel", "")},
    L2NORM=lambda c: {("l2norm_dim1_kernel", "")}, ROPE=lambda c: {("rope_kv_append_kernel", c["dt"].upper())}, EULER=lambda c: {("cfg_euler_kernel", "")},
    TSEMB=lambda c: {("timestep_embedding_kernel", "")},
)
TABLES = dict(CAST=CAST, SPLIT=SPLIT, COPY2D=COPY2D, ADD=ADD, PATCHIFY=PATCHIFY, IM2COL=IM2COL, LAYOUT=LAYOUT, HALO=HALO, ADD_I32=ADD_I32, EMBED=EMBED,
              SCATTER=SCATTER, SCATTER_STEP=SCATTER_STEP, SCATTER_SPEC=SCATTER_SPEC, LUT=LUT, TO_U8=TO_U8, RESAMPLE=RESAMPLE, MARKER=MARKER, AVGPOOL=AVGPOOL,
              SILU=SILU, L2NORM=L2NORM, ROPE=ROPE, EULER=EULER, TSEMB=TSEMB)
# which grid cap a table's `cap` counts against
CAP_OF = dict(CAST="elementwise", SPLIT="elementwise", COPY2D="elementwise", ADD="elementwise", PATCHIFY="elementwise", IM2COL="elementwise",
              LAYOUT="elementwise", SILU="silu_cast", HALO="halo_pack", EMBED="decode", SCATTER="decode", SCATTER_STEP="decode", SCATTER_SPEC="decode",
              ROPE="decode", LUT="preproc", TO_U8="preproc", RESAMPLE="preproc")
COVERED_ELSEWHERE = {"profile_marker_kernel": "an empty launch: a named dispatch for the profiler, nothing to compute"}
GLUE_OF_DECODE = ("rope_kv_append_kernel", "embedding_kernel", "scatter_rows_kernel", "scatter_rows_step_kernel", "scatter_rows_spec_kernel")


def reached():
    return {k for name, table in TABLES.items() for c in table for k in KERNEL_OF[name](c)}


def cap_cases():
    """(table, case id, which cap, trip count) of every case that must take the second trip of its grid-stride loop."""
    return [(name, c["id"], CAP_OF[name], c["cap"]) for name, table in TABLES.items() if name in CAP_OF for c in table if c.get("cap")]


def source_kernels():
    """Every (kernel, template arguments) that a hipLaunchKernelGGL of elementwise.hip / preproc.hip launches and those of the glue kernels of
    decode.hip, and the grid caps: threads of grid_for (elementwise.hip, preproc.hip), gs_grid (decode.hip), sx_silu_cast and sx_halo_pack."""
    src = {f: open(os.path.join(CSRC, f + ".hip")).read() for f in ("elementwise", "preproc", "decode")}
    launch = re.compile(r"hipLaunchKernelGGL\(\s*\(?\s*([A-Za-z_0-9:]+)\s*(?:<([^>]*)>)?")
    kernels = set()
    for f in ("elementwise", "preproc", "decode"):
        for name, targs in launch.findall(src[f]):
            name, targs = name.split("::")[-1], (targs or "").strip()
            if f == "decode" and name not in GLUE_OF_DECODE:
                continue
            if targs == "CC":                                  # the SX_RS(CC) macro of sx_resample_u8
                uses = re.findall(r"\{ SX_RS\((\d+)\) \}", src[f])
                assert uses, "sx_resample_u8 no longer expands SX_RS(3) / SX_RS(1)"
                kernels |= {(name, u) for u in uses}
            else:
                kernels.add((name, targs))
    for f in src:
        assert len(launch.findall(src[f])) == src[f].count("hipLaunchKernelGGL("), f"{f}.hip: a launch statement that the pattern does not read"
    cap = {}
    m = re.search(r"inline dim3 grid_for\(int64_t n, int per_thread = 1\) \{.*?if \(blocks > (\d+)\) blocks = \1;", src["elementwise"], re.S)
    cap["elementwise"] = int(m.group(1)) * 256
    m = re.search(r"inline dim3 grid_for\(int64_t n\) \{.*?if \(b > (\d+)\) b = \1;", src["preproc"], re.S)
    cap["preproc"] = int(m.group(1)) * 256
    m = re.search(r"inline dim3 gs_grid\(int64_t n\) \{.*?if \(b > (\d+)\) b = \1;", src["decode"], re.S)
    cap["decode"] = int(m.group(1)) * 256
    m = re.search(r"silu_cast_kernel, dim3\(\(unsigned\)\(\(n \+ 255\) / 256 > (\d+) \? \1 :", src["elementwise"])
    cap["silu_cast"] = int(m.group(1)) * 256
    m = re.search(r"const int grid = \(int\)\(\(total \+ 255\) / 256 < (\d+) \? \(total \+ 255\) / 256 : \1\);", src["elementwise"])
    cap["halo_pack"] = int(m.group(1)) * 256
    assert "grid_for(n, 4)" in src["elementwise"], "CAST's cap counts quads (grid_for(n, 4): one thread per 4 elements)"
    return kernels, cap


# ----------------------------------------------------------------------------------------------------------------------------
# references (torch, any device: tests/test_cpu_suite.py runs them against independent statements on the CPU)
# ----------------------------------------------------------------------------------------------------------------------------
CAST_PLANT = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), 65504.0, 65520.0, -65520.0, 65519.996, 2.0 ** -24, 2.0 ** -25, -2.0 ** -25,
              2.0 ** -25 * (1 + 2.0 ** -10), 3 * 2.0 ** -25, 2.0 ** -149, -2.0 ** -130, 2.0 ** -127, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8),
              -(1 + 3 * 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -20, 3.3895e38, 2.0 ** -133]


def patchify_ref(img, P, Kpad, dtype):
    """[B, 3, S, S] fp32 -> [B G G, Kpad] in dtype: F.unfold's (c, py, px) column order, zeros in 3 P P .. Kpad."""
    cols = Fn.unfold(img, P, stride=P).transpose(1, 2).reshape(-1, 3 * P * P).to(dtype)
    out = torch.zeros(cols.shape[0], Kpad, dtype=dtype, device=img.device)
    out[:, :3 * P * P] = cols
    return out


def im2col_ref(x, Kpad, dtype):
    """[B, H, W, Cin] fp32 -> [B H W, Kpad]: F.unfold(padding=1) reordered from c * 9 + tap to tap * Cin + c."""
    B, H, W, Cin = x.shape
    cols = Fn.unfold(x.permute(0, 3, 1, 2), 3, padding=1).view(B, Cin, 9, H * W).permute(0, 3, 2, 1).reshape(B * H * W, 9 * Cin).to(dtype)
    out = torch.zeros(B * H * W, Kpad, dtype=dtype, device=x.device)
    out[:, :9 * Cin] = cols
    return out


def halo_ref(x, prev, nxt, left, bottom):
    """x [B, Hl, W, C], prev / nxt [B, W, C] or None -> [B, Hl + 1 + bottom, W + left, C] with zero borders."""
    B, Hl, W, Cc = x.shape
    out = torch.zeros(B, Hl + 1 + bottom, W + left, Cc, dtype=x.dtype, device=x.device)
    out[:, 1:Hl + 1, left:] = x
    if prev is not None:
        out[:, 0, left:] = prev
    if bottom and nxt is not None:
        out[:, Hl + 1, left:] = nxt
    return out


def avgpool_ref(x, k):
    """fp64 mean over k consecutive tokens and the bound (k + 1) 2^-24 mean |x|."""
    B, L, D = x.shape
    x64 = x.double().view(B, L // k, k, D)
    return x64.mean(2), torch.clamp((k + 1) * U32 * x64.abs().mean(2), min=FLOOR[F32])


def silu_ref(x, dt):
    x64 = x.double()
    ref = x64 * torch.sigmoid(x64)
    return ref, rnd(ref, dt) + C_SILU * (1.0 + x64.abs()) * U32 * ref.abs()


def l2norm_ref(x, eps):
    x64 = x.double()
    ref = x64 / x64.pow(2).sum(1, keepdim=True).sqrt().clamp_min(float(torch.tensor(eps, dtype=F32)))
    return ref, torch.clamp((x.shape[1] + 4) * U32 * ref.abs(), min=FLOOR[F32])


def rope_tables(Tmax, D, dev):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    ang = torch.arange(Tmax, dtype=torch.float64)[:, None] * inv[None]
    return ang.cos().float().to(dev), ang.sin().float().to(dev)


def rope_ref(x, cos, sin, pos_rows, dt):
    """x [R, H, D] (16 bit), pos_rows [R] (table rows, already clamped to 0 where the position is outside the cache): the rotation in fp64 with the
    tables rounded to dt first; returns (ref, bound)."""
    half = x.shape[-1] // 2
    c = cos.to(dt).double()[pos_rows][:, None, :]
    s = sin.to(dt).double()[pos_rows][:, None, :]
    x1, x2 = x[..., :half].double(), x[..., half:].double()
    ref = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
    mag = torch.cat([(x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()], -1)
    return ref, rnd(ref, dt) + 2.0 * U32 * mag


def euler_ref(mode, x, eps, sigma, sigma_next, gs, igs):
    """One step in fp64 from fp32 operands: x [n], eps [nb, n], the fp32 sigmas as Python floats. Returns (x', bound, x' rsqrt(sigma_next^2 + 1), its
    bound)."""
    x, eps = x.double(), eps.double()
    d = sigma_next - sigma
    if mode == 0:
        eu, et = eps[0], eps[1]
        e = eu + gs * (et - eu)
        bound = C0_EULER * U32 * (x.abs() + abs(d) * (eu.abs() + gs * (et - eu).abs()))
    else:
        et, ei, eu = eps[0], eps[1], eps[2]
        x0t, x0i, x0u = x - sigma * et, x - sigma * ei, x - sigma * eu
        x0 = x0u + gs * (x0t - x0i) + igs * (x0i - x0u)
        e = (x0 - x) / (-sigma)
        S = (1.0 + igs) * eu.abs() + (gs + igs) * ei.abs() + gs * et.abs()
        bound = c1_euler(gs, igs) * U32 * (x.abs() + sigma * S) * (1.0 + abs(d) / sigma)
    xn = x + e * d
    inv = 1.0 / math.sqrt(sigma_next * sigma_next + 1.0)
    bound = torch.clamp(bound, min=FLOOR[F32])
    return xn, bound, xn * inv, bound * inv + 3.0 * U32 * (xn * inv).abs()


def tsemb_ref(t, dim):
    """fp64 throughout from the fp32 t [n]: (ref [n, dim] = [cos | sin], |t f_j| [n, dim])."""
    half = dim // 2
    f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64, device=t.device) / half)
    arg = t.double()[:, None] * f[None]
    return torch.cat([arg.cos(), arg.sin()], -1), torch.cat([arg.abs(), arg.abs()], -1)


def tsemb_e32(dim):
    """The yardstick: how far the fp32 op that the kernel replaces (oracle.restated_unet.timestep_embedding on the CPU) is from fp64 on TS_T, in units
    of 2^-24 (|t f_j| + 1)."""
    from oracle import restated_unet as ru
    t = torch.tensor(TS_T, dtype=F32)
    ref, arg = tsemb_ref(t, dim)
    return float(((ru.timestep_embedding(t, dim).double() - ref).abs() / (U32 * (arg + 1.0))).max())


def tsemb_bound(ref, arg, odt, e32):
    return rnd(ref, odt) + 4.0 * e32 * U32 * (arg + 1.0)


# inputs shared with tools/lab/glue_bound_sharpness.py
def silu_inputs(c, dev):
    x = torch.randn(c["n"], device=dev, generator=gen_of(c["id"], dev)) * 3.0
    plant = torch.tensor([0.0, -0.0, 1e-4, -1e-4, 20.0, -20.0, 88.0, -88.0, 89.0, -89.0, 104.0, -104.0, float("-inf")], device=dev)
    if c["n"] >= plant.numel():
        x[:plant.numel()] = plant
    return x


def l2norm_inputs(c, dev):
    x = torch.randn(c["B"], c["T"], c["D"], device=dev, generator=gen_of(c["id"], dev))
    if c["D"] >= 8:
        x[-1, :, 7] = 0.0
        x[0, :, 3] = 1e-20
    return x


def avgpool_inputs(c, dev):
    return torch.randn(c["B"], c["L"], c["D"], device=dev, generator=gen_of(c["id"], dev))


def rope_inputs(c, dev):
    g = gen_of(c["id"], dev)
    qkv = torch.randn(c["G"] * c["T"], 3 * c["H"], c["D"], device=dev, generator=g).to(DTYPES[c["dt"]])
    cos, sin = rope_tables(c["Tmax"], c["D"], dev)
    return qkv, cos, sin


def rope_rows(c):
    """Per qkv row: (slot, position, position inside the cache)."""
    out = []
    for g in range(c["G"]):
        for t in range(c["T"]):
            p = c["pos"][g] + t
            out.append((g, p, 0 <= p < c["Tmax"]))
    return out


def euler_inputs(c, dev):
    """(sigmas fp32 [51], lat0 [n], eps [50, nb, n]) of the 50-step walk."""
    from oracle import restated_unet as ru
    _, sig, init = ru.euler_tables(50)
    g = gen_of(c["id"], dev)
    n, nb = c["HW"] * c["C"], 2 + c["mode"]
    lat0 = torch.randn(n, device=dev, generator=g) * init
    eps = torch.randn(50, nb, n, device=dev, generator=g)
    return sig, lat0, eps


# ----------------------------------------------------------------------------------------------------------------------------
# exact group
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(s, d) for s in ALL_DT for d in ALL_DT], ids=lambda p: f"{p[0]}-{p[1]}")
@stops_on_gpu_fault
def test_cast_exact(dev, pair):
    """sx_cast, every size of one (source, destination) pair: NaN stays NaN, everything else equals tensor.to(dtype) bit for bit, planted at the head:
    +-0, +-inf, NaN, 65504, 65520 (the tie that rounds to inf in fp16), 2^-24, 2^-25 (an fp16 subnormal tie), fp32 subnormals, bf16 ties both ways."""
    lib = lib_()
    for c in [c for c in CAST if (c["s"], c["d"]) == pair]:
        sdt, ddt, n = ALL_DT[c["s"]], ALL_DT[c["d"]], c["n"]
        x = torch.randn(n, device=dev, generator=gen_of(c["id"], dev)) * 3.0
        plant = torch.tensor(CAST_PLANT, dtype=F32).to(dev)
        k = min(n, plant.numel())
        x[:k] = plant[(n % 7):][:k] if n < plant.numel() else plant
        src = x.to(sdt)
        sb = nan_lead(src)
        ref = src.to(ddt)

        def go():
            ob = GBuf(n, ddt, dev)
            ob.allow()[:] = True
            ok(lib.sx_cast(sb.data_ptr(), sx_code(sdt), ob.ptr(), sx_code(ddt), n, stream()), c["id"])
            ob.check(c["id"])
            return ob.body
        got = twice(go, c["id"])
        nan = ref.isnan()
        assert torch.equal(got.isnan(), nan), f"{c['id']}: NaN did not stay NaN (or appeared)"
        z = torch.zeros((), dtype=ddt, device=dev)
        exact(("cast_kernel", f"{c['s']}->{c['d']}"), torch.where(nan, z, got), torch.where(nan, z, ref), c["id"])


@pytest.mark.parametrize("c", SPLIT, ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_split_bf16_exact(dev, c):
    """hi = bf16(x), lo = bf16(x - hi); rows laid out [hi | hi | lo] (role 0) / [hi | lo | hi] (role 1). Planted: bf16 ties both ways, x - hi of both signs."""
    lib = lib_()
    rows, cols = c["rows"], c["cols"]
    x = torch.randn(rows, cols, device=dev, generator=gen_of(c["id"], dev))
    plant = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -9, 1 + 2.0 ** -7 - 2.0 ** -10, -(1 + 2.0 ** -9), 0.0, 2.0 ** -100], device=dev)
    k = min(cols, plant.numel())
    x[-1, :k] = plant[:k]
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    assert cols < 8 or (bool((x - hi.float() > 0).any()) and bool((x - hi.float() < 0).any()))
    ref = torch.cat([hi, hi, lo] if c["role"] == 0 else [hi, lo, hi], 1)
    xb = nan_lead(x)

    def go():
        ob = GBuf(rows * 3 * cols, BF16, dev)
        ob.allow()[:] = True
        ok(lib.sx_split_bf16(xb.data_ptr(), ob.ptr(), rows, cols, c["role"], stream()), c["id"])
        ob.check(c["id"])
        return ob.body.view(rows, 3 * cols)
    exact(("split_bf16_kernel", f"role{c['role']}"), twice(go, c["id"]), ref, c["id"])


@pytest.mark.parametrize("c", COPY2D, ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_copy2d_exact(dev, c):
    """src_ld > cols and dst_ld > cols at once, both with a column offset of 4; the columns between and behind the copied ones keep the guard."""
    lib = lib_()
    rows, cols = c["rows"], c["cols"]
    sld, dld, soff, doff = cols + 8, cols + 12, 4, 4
    x = torch.randn(rows, cols, device=dev, generator=gen_of(c["id"], dev))
    sb = _nanbuf(rows * sld + 256, F32, dev)
    sb[:rows * sld].view(rows, sld)[:, soff:soff + cols] = x

    def go():
        ob = GBuf(rows * dld, F32, dev)
        ob.allow().view(rows, dld)[:, doff:doff + cols] = True
        ok(lib.sx_copy2d_f32(sb.data_ptr() + 4 * soff, sld, ob.ptr() + 4 * doff, dld, rows, cols, stream()), c["id"])
        ob.check(c["id"])
        return ob.body.view(rows, dld)[:, doff:doff + cols]
    exact(("copy2d_kernel", "f32"), twice(go, c["id"]).contiguous(), x, c["id"])


@pytest.mark.parametrize("c", ADD, ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_add_f32_exact(dev, c):
    lib = lib_()
    n = c["n"]
    g = gen_of(c["id"], dev)
    a, b = torch.randn(n, device=dev, generator=g), torch.randn(n, device=dev, generator=g) * 100.0
    ab, bb = nan_lead(a), nan_lead(b)

    def go():
        ob = GBuf(n, F32, dev)
        ob.allow()[:] = True
        ok(lib.sx_add_f32(ab.data_ptr(), bb.data_ptr(), ob.ptr(), n, stream()), c["id"])
        ob.check(c["id"])
        return ob.body
    exact(("add_kernel", "f32"), twice(go, c["id"]), a + b, c["id"])


@pytest.mark.parametrize("c", PATCHIFY, ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_patchify_exact(dev, c):
    """Against F.unfold; the columns 3 P P .. Kpad are zeros that the kernel writes."""
    lib = lib_()
    dt, B, S, P, Kpad = DTYPES[c["dt"]], c["B"], c["S"], c["P"], c["Kpad"]
    img = torch.randn(B, 3, S, S, device=dev, generator=gen_of(c["id"], dev))
    ib = nan_lead(img)
    n = B * (S // P) ** 2 * Kpad

    def go():
        ob = GBuf(n, dt, dev)
        ob.allow()[:] = True
        ok(lib.sx_patchify(ib.data_ptr(), ob.ptr(), B, S, P, Kpad, sx_code(dt), stream()), c["id"])
        ob.check(c["id"])
        return ob.body.view(-1, Kpad)
    exact(("patchify_kernel", c["dt"]), twice(go, c["id"]), patchify_ref(img, P, Kpad, dt), c["id"])


@pytest.mark.parametrize("c", IM2COL, ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_im2col3x3_exact(dev, c):
    """Against F.unfold(padding=1) reordered to k = (ky 3 + kx) Cin + c; the 1 x 1 image has every tap but the centre outside."""
    lib = lib_()
    dt, B, H, W, Cin, Kpad = DTYPES[c["dt"]], c["B"], c["H"], c["W"], c["Cin"], c["Kpad"]
    x = torch.randn(B, H, W, Cin, device=dev, generator=gen_of(c["id"], dev))
    xb = nan_lead(x)

    def go():
        ob = GBuf(B * H * W * Kpad, dt, dev)
        ob.allow()[:] = True
        ok(lib.sx_im2col3x3_small(xb.data_ptr(), ob.ptr(), B, H, W, Cin, Kpad, sx_code(dt), stream()), c["id"])
        ob.check(c["id"])
        return ob.body.view(-1, Kpad)
    exact(("im2col3x3_kernel", c["dt"]), twice(go, c["id"]), im2col_ref(x, Kpad, dt), c["id"])


@pytest.mark.parametrize("c", LAYOUT, ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_nchw_nhwc_exact(dev, c):
    """NCHW -> NHWC with ld = C + 3 (the pad columns keep the guard), and back from that very buffer: the round trip is the input bit for bit."""
    lib = lib_()
    B, Cc, HW = c["B"], c["C"], c["HW"]
    ld = Cc + 3
    x = torch.randn(B, Cc, HW, device=dev, generator=gen_of(c["id"], dev))
    xb = nan_lead(x)

    def go():
        ob = GBuf(B * HW * ld, F32, dev)
        ob.allow().view(B * HW, ld)[:, :Cc] = True
        ok(lib.sx_nchw_to_nhwc(xb.data_ptr(), ob.ptr(), ld, B, Cc, HW, stream()), c["id"])
        ob.check(c["id"])
        back = GBuf(B * Cc * HW, F32, dev)
        back.allow()[:] = True
        ok(lib.sx_nhwc_to_nchw(ob.ptr(), ld, back.ptr(), B, Cc, HW, stream()), c["id"])
        back.check(c["id"] + " (back)")
        return ob.body.view(B, HW, ld)[:, :, :Cc].contiguous(), back.body.view(B, Cc, HW)
    nhwc, back = twice(go, c["id"])
    exact(("nchw_to_nhwc_kernel", "f32"), nhwc, x.transpose(1, 2).contiguous(), c["id"])
    exact(("nhwc_to_nchw_kernel", "f32"), back, x, c["id"] + " (round trip)")


def run_halo(dev, c):
    lib = lib_()
    B, Hl, W, Cc, left, bottom = c["B"], c["Hl"], c["W"], c["C"], c["left"], c["bottom"]
    g = gen_of(c["id"], dev)
    bits = lambda *shape: torch.randint(-32768, 32768, shape, device=dev, generator=g, dtype=torch.int32).to(torch.int16)
    x = bits(B, Hl, W, Cc)
    prev = bits(B, W, Cc) if c["prev"] else None
    nxt = bits(B, W, Cc) if c["next"] else None
    lead = lambda t: None if t is None else nan_lead(t.view(F16))
    xb, pb, nb = lead(x), lead(prev), lead(nxt)
    rows = Hl + 1 + bottom
    n = B * rows * (W + left) * Cc

    def go():
        ob = GBuf(n, F16, dev)
        ob.allow()[:] = True
        ok(lib.sx_halo_pack(xb.data_ptr(), pb.data_ptr() if pb is not None else None, nb.data_ptr() if nb is not None else None, ob.ptr(), B, Hl, W, Cc, left,
                            bottom, stream()), c["id"])
        ob.check(c["id"])
        return ob.body.view(torch.int16).view(B, rows, W + left, Cc)
    exact(("halo_pack_kernel", "16 bit"), twice(go, c["id"]), halo_ref(x, prev, nxt, left, bottom), c["id"])


@pytest.mark.parametrize("shape", [(1, 1, 1, 8), (1, 1, 1, 24), (2, 3, 5, 8), (2, 3, 5, 24)], ids=lambda s: "B%dHl%dW%dC%d" % s)
@stops_on_gpu_fault
def test_halo_pack_exact(dev, shape):
    """One process, explicit prev / next rows: all 8 combinations of (prev, next, left_col) with bottom 0 / 1; next is ignored without bottom."""
    cases = [c for c in HALO if (c["B"], c["Hl"], c["W"], c["C"]) == shape]
    assert len(cases) == 16
    for c in cases:
        run_halo(dev, c)


@stops_on_gpu_fault
def test_halo_pack_past_the_grid_cap(dev):
    """4097 rows x 4096 columns x one 16-byte piece: 16 781 312 pieces against 65536 x 256 threads (270 MB of output)."""
    run_halo(dev, HALO[-1])


@pytest.mark.parametrize("c", ADD_I32, ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_add_i32_n_exact(dev, c):
    lib = lib_()
    n = c["n"]
    start = torch.randint(-1000, 1000, (n,), device=dev, generator=gen_of(c["id"], dev), dtype=torch.int32)

    def go():
        ob = Guard(n, torch.int32, dev)
        ob.body.copy_(start)
        ob.allow()[:] = True
        ok(lib.sx_add_i32_n(ob.ptr(), -7, n, stream()), c["id"])
        ob.check(c["id"])
        return ob.body
    exact(("add_i32_kernel", "i32"), twice(go, c["id"]), start - 7, c["id"])


@pytest.mark.parametrize("c", EMBED, ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_embedding_exact(dev, c):
    """Repeated ids, the first and the last row of the table; every id is inside the table."""
    lib = lib_()
    dt, T, dim, V = DTYPES[c["dt"]], c["T"], c["dim"], 11
    g = gen_of(c["id"], dev)
    table = torch.randn(V, dim, device=dev, generator=g).to(dt)
    ids = torch.randint(0, V, (T,), device=dev, generator=g, dtype=torch.int32)
    ids[:4] = torch.tensor([0, V - 1, 5, 5], dtype=torch.int32)
    assert 0 <= int(ids.min()) and int(ids.max()) < V
    tb = nan_lead(table)

    def go():
        ob = GBuf(T * dim, F32, dev)
        ob.allow()[:] = True
        ok(lib.sx_embedding(ids.data_ptr(), tb.data_ptr(), ob.ptr(), T, dim, sx_code(dt), stream()), c["id"])
        ob.check(c["id"])
        return ob.body.view(T, dim)
    exact(("embedding_kernel", c["dt"]), twice(go, c["id"]), table[ids.long()].float(), c["id"])


@pytest.mark.parametrize("c", SCATTER, ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_scatter_rows_exact(dev, c):
    """Rows in permuted order; the rows that are not named keep the guard; n = 0 writes nothing."""
    lib = lib_()
    n, dim, R = c["n"], c["dim"], c["R"]
    g = gen_of(c["id"], dev)
    src = torch.randn(max(n, 1), dim, device=dev, generator=g)[:n]
    rows = torch.randperm(R, device=dev, generator=g)[:n].to(torch.int32)
    assert n == 0 or (0 <= int(rows.min()) and int(rows.max()) < R)
    sb = nan_lead(src) if n else _nanbuf(256, F32, dev)
    rb = torch.cat([rows, torch.zeros(8, dtype=torch.int32, device=dev)])        # behind the n rows: valid row numbers too

    def go():
        ob = GBuf(R * dim, F32, dev)
        ob.allow().view(R, dim)[rows.long()] = True
        ok(lib.sx_scatter_rows(sb.data_ptr(), rb.data_ptr(), ob.ptr(), n, dim, stream()), c["id"])
        ob.check(c["id"])
        return ob.body.view(R, dim)[rows.long()]
    exact(("scatter_rows_kernel", "f32"), twice(go, c["id"]), src, c["id"])


@pytest.mark.parametrize("c", SCATTER_STEP, ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_scatter_rows_step_exact(dev, c):
    """step = -1, 0, rows - 1, rows, rows + 3 over 5 slots: the first and the last two are dropped and write nothing."""
    lib = lib_()
    dim, R, G = c["dim"], c["rows"], 5
    steps = [-1, 0, R - 1, R, R + 3]
    src = torch.randn(G, dim, device=dev, generator=gen_of(c["id"], dev))
    sb, st = nan_lead(src), torch.tensor(steps, dtype=torch.int32, device=dev)
    live = [(g, s) for g, s in enumerate(steps) if 0 <= s < R]
    assert live == [(1, 0), (2, R - 1)]

    def go():
        ob = GBuf(G * R * dim, F32, dev)
        for g, s in live:
            ob.allow().view(G, R, dim)[g, s] = True
        ok(lib.sx_scatter_rows_step(sb.data_ptr(), st.data_ptr(), ob.ptr(), G, dim, R, stream()), c["id"])
        ob.check(c["id"])
        return torch.stack([ob.body.view(G, R, dim)[g, s] for g, s in live])
    exact(("scatter_rows_step_kernel", "f32"), twice(go, c["id"]), src[[g for g, _ in live]], c["id"])


@pytest.mark.parametrize("c", SCATTER_SPEC, ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_scatter_rows_spec_exact(dev, c):
    """T = 3 rows per slot, step = -1 (parked: dropped), 0, rows - 2 (step + 2 is past the log: that row alone is dropped), rows - 1, rows + 3.
    tok_index[g T + t] = max(step[g], 0) + t for EVERY row, dropped or not, as include/seedx_hip.h states it."""
    lib = lib_()
    dim, R, G, T = c["dim"], c["rows"], 5, 3
    steps = [-1, 0, R - 2, R - 1, R + 3]
    src = torch.randn(G * T, dim, device=dev, generator=gen_of(c["id"], dev))
    sb, st = nan_lead(src), torch.tensor(steps, dtype=torch.int32, device=dev)
    live = [(g, t, s + t) for g, s in enumerate(steps) for t in range(T) if s >= 0 and s + t < R]
    assert len(live) == 3 + 2 + 1
    tok_ref = torch.tensor([max(s, 0) + t for s in steps for t in range(T)], dtype=torch.int32, device=dev)

    def go():
        ob = GBuf(G * R * dim, F32, dev)
        for g, t, r in live:
            ob.allow().view(G, R, dim)[g, r] = True
        tk = Guard(G * T, torch.int32, dev)
        tk.allow()[:] = c["tok"]
        ok(lib.sx_scatter_rows_spec(sb.data_ptr(), st.data_ptr(), ob.ptr(), tk.ptr() if c["tok"] else None, G, T, dim, R, stream()), c["id"])
        ob.check(c["id"])
        tk.check(c["id"] + " (tok_index)")
        return torch.stack([ob.body.view(G, R, dim)[g, r] for g, t, r in live]), (tk.body if c["tok"] else None)
    got, tok = twice(go, c["id"])
    exact(("scatter_rows_spec_kernel", "f32"), got, src[[g * T + t for g, t, _ in live]], c["id"])
    if c["tok"]:
        exact(("scatter_rows_spec_kernel", "tok_index"), tok, tok_ref, c["id"] + " (tok_index)")


@pytest.mark.parametrize("c", LUT, ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_u8_to_chw_lut_exact(dev, c):
    """Crop boxes at the four corners of a source with src_stride = 3 W + 7, against the table gather."""
    lib = lib_()
    H, W, Hc, Wc = c["H"], c["W"], c["Hc"], c["Wc"]
    stride = 3 * W + 7
    x0 = 0 if c["corner"][1] == "l" else W - Wc
    y0 = 0 if c["corner"][0] == "t" else H - Hc
    g = gen_of(c["id"], dev)
    src = torch.randint(0, 256, (H, stride), device=dev, generator=g, dtype=torch.int32).to(torch.uint8)
    lut = torch.randn(3, 256, device=dev, generator=g)
    lb = nan_lead(lut)
    crop = src[y0:y0 + Hc, 3 * x0:3 * (x0 + Wc)].reshape(Hc, Wc, 3).long()
    ref = torch.stack([lut[ch][crop[..., ch]] for ch in range(3)])

    def go():
        ob = GBuf(3 * Hc * Wc, F32, dev)
        ob.allow()[:] = True
        ok(lib.sx_u8_to_chw_lut(src.data_ptr(), H, W, stride, x0, y0, Hc, Wc, lb.data_ptr(), ob.ptr(), stream()), c["id"])
        ob.check(c["id"])
        return ob.body.view(3, Hc, Wc)
    exact(("u8_to_chw_lut_kernel", "f32"), twice(go, c["id"]), ref, c["id"])


@pytest.mark.parametrize("c", TO_U8, ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_chw_to_u8_image_exact(dev, c):
    """Every tie (k + 0.5) / 255 mapped back through 2 v - 1, with its two fp32 neighbours; values below -1 and above 1; against the torch formula
    (x / 2 + 0.5).clamp(0, 1) * 255 rounded half to even, in fp32."""
    lib = lib_()
    H, W = c["H"], c["W"]
    x = torch.randn(3, H * W, device=dev, generator=gen_of(c["id"], dev)) * 0.8
    v = ((torch.arange(255, dtype=F32) + 0.5) / 255.0) * 2.0 - 1.0
    inf = torch.tensor(float("inf"))
    ties = torch.cat([v, torch.nextafter(v, inf), torch.nextafter(v, -inf), torch.tensor([-1.0, 1.0, -1.5, 1.5, -100.0, 100.0, 0.0, -0.0, 1e-3])]).to(dev)
    for ch in range(3):
        x[ch, ch:ch + ties.numel()] = ties
    ref = ((x / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).t().contiguous()
    xb = nan_lead(x)

    def go():
        ob = Guard(H * W * 3, torch.uint8, dev)
        ob.allow()[:] = True
        ok(lib.sx_chw_to_u8_image(xb.data_ptr(), H, W, ob.ptr(), stream()), c["id"])
        ob.check(c["id"])
        return ob.body.view(H * W, 3)
    exact(("chw_to_u8_image_kernel", "u8"), twice(go, c["id"]), ref, c["id"])


@pytest.mark.parametrize("c", RESAMPLE, ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_resample_u8_exact(dev, c):
    """The C = 1 instantiations, a horizontal-only and a vertical-only pass, both passes, a strided source, and one output above 2 097 152 pixels from a
    10 x 10 source, against oracle.restated_preproc.resample_u8_fixed_point (which tests/test_cpu_suite.py pins to Pillow) on the product's tables."""
    from oracle import restated_preproc as rp
    from seedx_amd import image_ops as io
    lib = lib_()
    Cc, Hin, Win, Hout, Wout = c["C"], c["Hin"], c["Win"], c["Hout"], c["Wout"]
    stride = Win * Cc + 5
    g = gen_of(c["id"], dev)
    src = torch.randint(0, 256, (Hin, stride), device=dev, generator=g, dtype=torch.int32).to(torch.uint8)
    img = src[:, :Win * Cc].reshape(Hin, Win, Cc).cpu().numpy()
    need_h, need_v = Wout != Win, Hout != Hin
    kh = bh = kv = bv = None
    ksh = ksv = y_first = y_rows = 0
    kk_w = bw_ = kk_h = bh_ = None
    if need_h:
        kk_w, bw_, ksh = io.pil_coeffs(Win, Wout, c["rs"])
        kh, bh = torch.from_numpy(kk_w).to(dev), torch.from_numpy(bw_).to(dev)
    if need_v:
        kk_h, bh_, ksv = io.pil_coeffs(Hin, Hout, c["rs"])
        kv, bv = torch.from_numpy(kk_h).to(dev), torch.from_numpy(bh_).to(dev)
        if need_h:
            y_first = int(bh_[0, 0])
            y_rows = int(bh_[-1, 0] + bh_[-1, 1]) - y_first
    assert 0 <= y_first and y_first + y_rows <= Hin
    ref = torch.from_numpy(rp.resample_u8_fixed_point(img, (Wout, Hout), kk_w, bw_, kk_h, bh_)).to(dev)
    p = lambda t: None if t is None else t.data_ptr()

    def go():
        ob = Guard(Hout * Wout * Cc, torch.uint8, dev)
        ob.allow()[:] = True
        tmp = Guard(max(y_rows, 1) * Wout * Cc, torch.uint8, dev)
        tmp.allow()[:] = need_h and need_v
        ok(lib.sx_resample_u8(src.data_ptr(), Hin, Win, Cc, stride, ob.ptr(), Hout, Wout, p(kh), p(bh), ksh, p(kv), p(bv), ksv, y_first, y_rows,
                              tmp.ptr() if need_h and need_v else None, stream()), c["id"])
        ob.check(c["id"])
        tmp.check(c["id"] + " (tmp)")
        return ob.body.view(Hout, Wout, Cc)
    got = twice(go, c["id"])
    for k in KERNEL_OF["RESAMPLE"](c):
        exact((k[0], f"C={k[1]}"), got, ref, c["id"])


def marker_ids(c):
    """int64 ids [T] on the CPU; markers 11 (<img>), 13 (<patch>), 12 (</img>), 14 (</patch>). The kernel gives thread i the chunk
    [i ceil(T / 256), (i + 1) ceil(T / 256)): `straddle` puts an opener on the last id of a chunk and its closer two further on, at every chunk boundary
    that leaves room; `edges` adds an opener at index 0 and a closer at index T - 1."""
    T, v = c["T"], c["v"]
    rng = np.random.default_rng(zlib.crc32(c["id"].encode()))
    if v == "random":
        return torch.from_numpy(rng.choice([11, 12, 13, 14, 1, 2, 3, 4, 5, 6], size=T).astype(np.int64))
    ids = rng.integers(1, 10, size=T).astype(np.int64)
    chunk, last = -(-T // 256), -1
    for b in range(chunk, T - 1, chunk):
        if b - 1 > last and b + 1 < T:
            ids[b - 1], ids[b + 1] = (11, 12) if (b // chunk) % 2 else (13, 14)
            last = b + 1
    if v == "edges":
        ids[0] = 11
        ids[T - 1] = 14 if T > 1 else 11
    return torch.from_numpy(ids)


@pytest.mark.parametrize("T", (1, 255, 256, 257, 4097))
@stops_on_gpu_fault
def test_marker_mask_exact(dev, T):
    from oracle import restated_preproc as rp
    lib = lib_()
    for c in [c for c in MARKER if c["T"] == T]:
        ids = marker_ids(c)
        ref = rp.marker_mask(ids, 11, 12, 13, 14).to(torch.uint8).to(dev)
        assert c["v"] != "straddle" or T < 4 or int(ref.sum()) > 0
        idev = torch.cat([ids, torch.full((64,), 11, dtype=torch.int64)]).to(dev)      # openers behind the ids: reading them would change the pairing

        def go():
            ob = Guard(T, torch.uint8, dev)
            ob.allow()[:] = True
            ok(lib.sx_marker_mask(idev.data_ptr(), T, 11, 13, 12, 14, ob.ptr(), stream()), c["id"])
            ob.check(c["id"])
            return ob.body
        exact(("marker_mask_kernel", "u8"), twice(go, c["id"]), ref, c["id"])


@stops_on_gpu_fault
def test_zero_counts_are_ok_and_write_nothing(dev):
    """Every entry point that takes an element count returns SX_OK for 0 and writes nothing (sx_silu_cast built a grid of 0 blocks before)."""
    lib = lib_()
    f32, i32 = _nanbuf(4096, F32, dev), torch.zeros(64, dtype=torch.int32, device=dev)
    sig = torch.ones(8, device=dev)
    out = GBuf(4096, F32, dev)
    o16 = GBuf(4096, F16, dev)
    o8 = Guard(4096, torch.uint8, dev)
    i64 = torch.zeros(64, dtype=torch.int64, device=dev)
    s = stream()
    calls = {
        "sx_cast": lambda: lib.sx_cast(f32.data_ptr(), 2, o16.ptr(), 0, 0, s),
        "sx_split_bf16": lambda: lib.sx_split_bf16(f32.data_ptr(), o16.ptr(), 0, 8, 0, s),
        "sx_copy2d_f32": lambda: lib.sx_copy2d_f32(f32.data_ptr(), 8, out.ptr(), 8, 0, 8, s),
        "sx_add_f32": lambda: lib.sx_add_f32(f32.data_ptr(), f32.data_ptr(), out.ptr(), 0, s),
        "sx_patchify": lambda: lib.sx_patchify(f32.data_ptr(), o16.ptr(), 0, 4, 2, 16, 0, s),
        "sx_im2col3x3_small": lambda: lib.sx_im2col3x3_small(f32.data_ptr(), o16.ptr(), 0, 2, 2, 4, 64, 0, s),
        "sx_avgpool_tokens": lambda: lib.sx_avgpool_tokens(f32.data_ptr(), out.ptr(), 0, 4, 8, 2, s),
        "sx_timestep_embedding": lambda: lib.sx_timestep_embedding(f32.data_ptr(), None, out.ptr(), 0, 8, 2, s),
        "sx_nchw_to_nhwc": lambda: lib.sx_nchw_to_nhwc(f32.data_ptr(), out.ptr(), 4, 0, 4, 4, s),
        "sx_nhwc_to_nchw": lambda: lib.sx_nhwc_to_nchw(f32.data_ptr(), 4, out.ptr(), 0, 4, 4, s),
        "sx_cfg_euler_step": lambda: lib.sx_cfg_euler_step(f32.data_ptr(), out.ptr(), out.ptr() + 1024, sig.data_ptr(), i32.data_ptr(), 2, 0, 4, 4, GS, IGS, 0, s),
        "sx_silu_cast": lambda: lib.sx_silu_cast(f32.data_ptr(), o16.ptr(), 0, 0, s),
        "sx_embedding": lambda: lib.sx_embedding(i32.data_ptr(), o16.ptr(), out.ptr(), 0, 8, 0, s),
        "sx_scatter_rows": lambda: lib.sx_scatter_rows(f32.data_ptr(), i32.data_ptr(), out.ptr(), 0, 8, s),
        "sx_marker_mask": lambda: lib.sx_marker_mask(i64.data_ptr(), 0, 11, 13, 12, 14, o8.ptr(), s),
    }
    for name, call in calls.items():
        ok(call(), f"{name} with an element count of 0")
        for b in (out, o16, o8):
            b.check(f"{name} with an element count of 0")


# ----------------------------------------------------------------------------------------------------------------------------
# bounded group
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", AVGPOOL, ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_avgpool_tokens_vs_fp64(dev, c):
    lib = lib_()
    B, L, D, k = c["B"], c["L"], c["D"], c["k"]
    x = avgpool_inputs(c, dev)
    ref, bound = avgpool_ref(x, k)
    xb = nan_lead(x)

    def go():
        ob = GBuf(B * (L // k) * D, F32, dev)
        ob.allow()[:] = True
        ok(lib.sx_avgpool_tokens(xb.data_ptr(), ob.ptr(), B, L, D, k, stream()), c["id"])
        ob.check(c["id"])
        return ob.body.view(B, L // k, D)
    got = twice(go, c["id"])
    assert bool(torch.isfinite(got).all())
    held(("avgpool_tokens_kernel", f"k={k}"), got.double(), ref, bound, c["id"])


@pytest.mark.parametrize("c", SILU, ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_silu_cast_vs_fp64(dev, c):
    lib = lib_()
    dt, n = DTYPES[c["dt"]], c["n"]
    x = silu_inputs(c, dev)
    ref, bound = silu_ref(x, dt)
    xb = nan_lead(x)

    def go():
        ob = GBuf(n, dt, dev)
        ob.allow()[:] = True
        ok(lib.sx_silu_cast(xb.data_ptr(), ob.ptr(), sx_code(dt), n, stream()), c["id"])
        ob.check(c["id"])
        return ob.body
    got = twice(go, c["id"])
    minf = x == float("-inf")
    assert bool(ref[minf].isnan().all()) and bool(got[minf].isnan().all()), f"{c['id']}: silu(-inf) is NaN in torch (-inf * 0) and in the kernel (-inf / inf)"
    assert bool(torch.isfinite(got[~minf].float()).all()), f"{c['id']}: non-finite output"
    held(("silu_cast_kernel", c["dt"]), got[~minf].double(), ref[~minf], bound[~minf], c["id"])


@pytest.mark.parametrize("c", L2NORM, ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_l2norm_dim1_vs_fp64(dev, c):
    lib = lib_()
    B, T, D = c["B"], c["T"], c["D"]
    x = l2norm_inputs(c, dev)
    ref, bound = l2norm_ref(x, 1e-12)
    xb = nan_lead(x)

    def go():
        ob = GBuf(B * T * D, F32, dev)
        ob.allow()[:] = True
        ok(lib.sx_l2norm_dim1(xb.data_ptr(), ob.ptr(), B, T, D, 1e-12, stream()), c["id"])
        ob.check(c["id"])
        return ob.body.view(B, T, D)
    got = twice(go, c["id"])
    assert bool(torch.isfinite(got).all())
    if D >= 8:
        assert bool((got[-1, :, 7] == 0).all()) and float(ref[0, 0, 3]) == pytest.approx(1e-20 / float(torch.tensor(1e-12, dtype=F32)), rel=1e-6)
    held(("l2norm_dim1_kernel", "f32"), got.double(), ref, bound, c["id"])


@pytest.mark.parametrize("c", ROPE, ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_rope_kv_append_vs_fp64(dev, c):
    """q rows in place, K rows rotated into the cache, V rows copied bit for bit; cache_seq_stride = H Tmax D + 64 in the batched form; every cache
    row but the appended ones keeps the guard; positions outside [0, Tmax) (Tmax - 2 with T = 5: the last three rows; -1: a parked slot) write no
    cache row and leave q as it is (table row 0: cos 1, sin 0)."""
    lib = lib_()
    dt, G, T, H, D, Tmax = DTYPES[c["dt"]], c["G"], c["T"], c["H"], c["D"], c["Tmax"]
    qkv, cos, sin = rope_inputs(c, dev)
    rows = rope_rows(c)
    assert all(-1 <= p <= Tmax + T for _, p, _ in rows)
    trow = torch.tensor([p if inside else 0 for _, p, inside in rows], device=dev)
    qref, qbound = rope_ref(qkv[:, :H], cos, sin, trow, dt)
    kref, kbound = rope_ref(qkv[:, H:2 * H], cos, sin, trow, dt)
    cb, sb_ = nan_lead(cos), nan_lead(sin)
    pos = torch.tensor(c["pos"], dtype=torch.int32, device=dev)
    sstride = H * Tmax * D + c["pad"]

    def go():
        qb = GBuf(qkv.numel(), dt, dev)
        qb.body.copy_(qkv.reshape(-1))
        qb.allow()[:] = True
        kc, vc = GBuf(G * sstride, dt, dev), GBuf(G * sstride, dt, dev)
        for buf in (kc, vc):
            a = torch.as_strided(buf.allow(), (G, H, Tmax, D), (sstride, Tmax * D, D, 1))
            for g, p, inside in rows:
                if inside:
                    a[g, :, p] = True
        if c["b"]:
            st = lib.sx_rope_kv_append_b(qb.ptr(), kc.ptr(), vc.ptr(), cb.data_ptr(), sb_.data_ptr(), pos.data_ptr(), G, T, H, D, Tmax, sstride, sx_code(dt), stream())
        else:
            st = lib.sx_rope_kv_append(qb.ptr(), kc.ptr(), vc.ptr(), cb.data_ptr(), sb_.data_ptr(), pos.data_ptr(), T, H, D, Tmax, sx_code(dt), stream())
        ok(st, c["id"])
        for buf, what in ((qb, "qkv"), (kc, "K cache"), (vc, "V cache")):
            buf.check(f"{c['id']} ({what})")
        view = lambda buf: torch.as_strided(buf.body, (G, H, Tmax, D), (sstride, Tmax * D, D, 1))
        sel = [(r, g, p) for r, (g, p, inside) in enumerate(rows) if inside]
        kg = torch.stack([view(kc)[g, :, p] for _, g, p in sel]) if sel else None
        vg = torch.stack([view(vc)[g, :, p] for _, g, p in sel]) if sel else None
        return qb.body.view(G * T, 3 * H, D).clone(), kg, vg
    out, kg, vg = twice(go, c["id"])
    assert same_bits(out[:, H:].contiguous(), qkv[:, H:].contiguous()), f"{c['id']}: the K / V part of qkv was changed"
    key = ("rope_kv_append_kernel", c["dt"])
    held(key, out[:, :H].double(), qref, qbound, c["id"] + " (q)")
    outside = [r for r, (_, _, inside) in enumerate(rows) if not inside]
    if outside:
        assert same_bits(out[outside, :H].contiguous(), qkv[outside, :H].contiguous()), f"{c['id']}: q of a row without a cache position was changed"
    live = [r for r, (_, _, inside) in enumerate(rows) if inside]
    if live:
        held(key, kg.double(), kref[live], kbound[live], c["id"] + " (K)")
        exact(("rope_kv_append_kernel", c["dt"] + " V rows"), vg.contiguous(), qkv[live, 2 * H:].contiguous(), c["id"] + " (V)")


@pytest.mark.parametrize("c", EULER, ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_cfg_euler_step_50_steps_vs_fp64(dev, c):
    """All 50 steps of euler_tables(50) (sigma from 13.1 down to 0.041, then sigma_next = 0), the latents carried from launch to launch and every step judged
    against an fp64 step from the kernel's own previous output. The step index walks 0 .. 49 of the 51 sigmas: always inside."""
    lib = lib_()
    mode, ld, HW, Cc = c["mode"], c["ld"], c["HW"], c["C"]
    n, nb = HW * Cc, 2 + mode
    sig, lat0, eps = euler_inputs(c, dev)
    assert sig.numel() == 51 and float(sig[50]) == 0.0 and float(sig[49]) == float(sig[:50].min()) and 0.03 < float(sig[49]) < 0.05 and float(sig[0]) > 13.0
    sigb = nan_lead(sig.to(dev))
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    lat = GBuf(n, F32, dev)
    lat.allow()[:] = True
    lat.body.copy_(lat0)
    free = lat0.double()
    key = ("cfg_euler_kernel", f"mode {mode}")
    worst_step = (0.0, -1)
    for i in range(50):
        s, sn = float(sig[i]), float(sig[i + 1])
        step.fill_(i)
        assert 0 <= i and i + 1 < sig.numel()
        prev = lat.body.clone()
        eb = nan_lead(eps[i])
        ref, bound, sref, sbound = euler_ref(mode, prev, eps[i], s, sn, GS, IGS)
        free = euler_ref(mode, free, eps[i], s, sn, GS, IGS)[0]

        def launch(latbuf):
            sc = None
            if c["scaled"]:
                sc = GBuf(nb * HW * ld, F32, dev)
                sc.allow().view(nb * HW, ld)[:, :Cc] = True
            ok(lib.sx_cfg_euler_step(eb.data_ptr(), latbuf.ptr(), sc.ptr() if sc is not None else None, sigb.data_ptr(), step.data_ptr(), nb, n, Cc, ld, GS, IGS,
                                     mode, stream()), f"{c['id']} step {i}")
            latbuf.check(f"{c['id']} step {i} (latents)")
            if sc is not None:
                sc.check(f"{c['id']} step {i} (scaled copy)")
            return sc.body.view(nb, HW, ld)[:, :, :Cc].reshape(nb, n) if sc is not None else None
        twin = GBuf(n, F32, dev)
        twin.allow()[:] = True
        twin.body.copy_(prev)
        scaled = launch(lat)
        scaled2 = launch(twin)
        assert same_bits(lat.body, twin.body) and (scaled is None or same_bits(scaled, scaled2)), f"{c['id']} step {i}: two identical launches differ"
        assert bool(torch.isfinite(lat.body).all())
        w = held(key, lat.body.double(), ref, bound, f"{c['id']} step {i} (sigma {s:.4f} -> {sn:.4f})")
        worst_step = max(worst_step, (w, i))
        if scaled is not None:
            for k in range(nb):
                held(("cfg_euler_kernel", f"mode {mode} scaled copy"), scaled[k].double(), sref, sbound, f"{c['id']} step {i} (scaled copy {k})")
    drift = float((lat.body.double() - free).abs().max())
    NOTES[f"{c['id']}: free-running fp64 chain after 50 steps"] = (f"max |kernel - fp64| {drift:.3e} (max |latent| {float(free.abs().max()):.3f}); worst single step "
                                                                    f"{worst_step[0]:.3f} of its bound at step {worst_step[1]}")
    print(f"{c['id']}: drift {drift:.3e}, worst step ratio {worst_step[0]:.3f} at step {worst_step[1]}")


E32_CACHE = {}


@pytest.mark.parametrize("dim", (2, 256, 320))
@stops_on_gpu_fault
def test_timestep_embedding_vs_fp64(dev, dim):
    """Every output type and both forms of idx_dev at one dim; t = 0, 1, 20.5, 448, 981, 999, 1024 (the time ids). idx_dev is 0, 3 or 6 of 7."""
    lib = lib_()
    e32 = E32_CACHE.setdefault(dim, tsemb_e32(dim))
    NOTES[f"timestep embedding dim {dim}: E32 (the fp32 op on the CPU against fp64)"] = f"{e32:.3f}"
    t = torch.tensor(TS_T, dtype=F32, device=dev)
    tb = nan_lead(t)
    for c in [c for c in TSEMB if c["dim"] == dim]:
        odt, idx = ALL_DT[c["o"]], c["idx"]
        assert idx is None or 0 <= idx < t.numel()
        n = t.numel() if idx is None else 2
        tt = t if idx is None else t[idx].expand(n)
        ref, arg = tsemb_ref(tt, dim)
        ib = torch.tensor([idx if idx is not None else 0], dtype=torch.int32, device=dev)

        def go():
            ob = GBuf(n * dim, odt, dev)
            ob.allow()[:] = True
            ok(lib.sx_timestep_embedding(tb.data_ptr(), ib.data_ptr() if idx is not None else None, ob.ptr(), n, dim, sx_code(odt), stream()), c["id"])
            ob.check(c["id"])
            return ob.body.view(n, dim)
        got = twice(go, c["id"])
        assert bool(torch.isfinite(got.float()).all())
        held(("timestep_embedding_kernel", f"{c['o']} dim {dim}"), got.double(), ref, tsemb_bound(ref, arg, odt, e32), c["id"])


def test_print_worst_ratio_per_kernel(dev):
    """Not a check of its own: the differing elements of the exact group (0 or the test failed), the worst |diff| / bound of the bounded group per kernel
    and type (run the file as a whole), E32 and the distance of the free-running fp64 Euler chains."""
    for key, n in sorted(EXACT.items(), key=lambda kv: str(kv[0])):
        print(f"differing elements    {str(key):60s} {n}")
    for key, w in sorted(WORST.items(), key=lambda kv: str(kv[0])):
        print(f"worst |diff| / bound  {str(key):60s} {w:.3f}")
    for k in sorted(NOTES):
        print(f"{k}: {NOTES[k]}")
