// Single-token decode path of the Llama-style LLM on gfx950: HBM-bound weight-streaming GEMV, split-KV
// decode attention, RoPE + KV-cache append, embedding gather/scatter and the fused greedy/logits-rule step.
// All loop state (position, current token) lives in DEVICE memory so a whole token step is hipGraph-replayable
// with zero host round trips (the reference syncs ≥45× per token).
#include "sx_common.h"
#include <type_traits>

namespace sxk_decode {

// ---- GEMV: one wave per 2 weight rows (or one GLU pair), 16-B weight loads, x re-read through L1/L2 ----------
struct GemvP {
  const unsigned short* x;
  const unsigned short* W;
  void* y;
  const float* residual;
  int M, N, K, out_dtype, act, glu;
  int packed;   // W is in the decode layout [N/16][K/32][16 rows][32 k] (one MFMA operand tile = 1 KB contiguous)
  int y_tiled;  // y is written as operand tiles [n_out/32][16][32] (16-bit outputs)
  int x_tiled;  // x is in operand tiles [K/32][16 rows][32 k] (one 1-KB tile per MFMA B operand; rows >= M are padding)
  unsigned* ws_cnt;   // split-K: arrival counters [N/16] (zero between launches)
  float* ws_part;     //          partial sums [S][16][N]
  // RMSNorm fold (include/seedx_hip.h sx_gemv_args): producer side x16_out / ssq_out, consumer side ssq_in
  unsigned short* x16_out;
  float* ssq_out;
  const float* ssq_in;
  int ssq_parts;
  float ssq_inv_dim, ssq_eps;
  int planes2;  // MB = 2 kernels with M <= 16: x block 1 is the LO plane of an fp32-grade activation (sx_gemv_args.x_planes = 2) — the two
                // blocks' results are added ahead of the epilogue
  int out_planes;          // the 16-bit tiled output (y_tiled) or x16_out is written as two planes: block 0 = hi, block 1 = lo (rows <= 16)
  const float* x16_gamma;  // x16_out holds o * gamma[col] (the NEXT RMSNorm's gamma applied on the activation side: the weights stay exact)
  const float* w_scale;    // FP8 weight tiles (W8 kernels): fp32 [N], row n of W as passed is e4m3 code * w_scale[n]
  const unsigned char* w_bscale;   // MXFP4 weight tiles (W4 kernels): E8M0 bytes [N/16][K/64][16][2] (20-row tiles: [N/20][K/64][20][2])
  const float* addend;     // MFMA path: fp32 [M][N] (rows of W as passed) added to row m's summed accumulator ahead of activation / GLU / residual
  const int* addend_sel;   // int32 [M] or NULL: row m takes its addend iff NULL or addend_sel[m] in [0, addend_n) (the unmerged LoRA delta, csrc/lora.hip)
  int addend_n;
};

template <typename TT, int MR>
__global__ __launch_bounds__(256) void gemv_kernel(const GemvP p) {
  const int lane = threadIdx.x & 63;
  const int wid = blockIdx.x * 4 + (threadIdx.x >> 6);  // wave id = pair index
  int r0, r1, n_out;
  if (p.glu) {
    // 32-row groups [16 linear | 16 gate]; pair j of group g = rows (32g + j, 32g + 16 + j)
    const int g = wid >> 4, j = wid & 15;
    r0 = g * 32 + j;
    r1 = r0 + 16;
    n_out = g * 16 + j;
  } else {
    r0 = wid * 2;
    r1 = r0 + 1;
    n_out = r0;
  }
  if (r0 >= p.N) return;
  const bool has1 = r1 < p.N;
  const int nch = p.K >> 3;  // 16-B chunks per row
  const u32x4_t* w0 = (const u32x4_t*)(p.W + (size_t)r0 * p.K);
  const u32x4_t* w1 = (const u32x4_t*)(p.W + (size_t)(has1 ? r1 : r0) * p.K);
  float acc0[MR], acc1[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) { acc0[m] = 0.f; acc1[m] = 0.f; }
  for (int c = lane; c < nch; c += 64) {
    const u32x4_t a = __builtin_nontemporal_load(w0 + c);
    const u32x4_t b = __builtin_nontemporal_load(w1 + c);
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      const int mm = m < p.M ? m : p.M - 1;
      const u32x4_t xv = *(const u32x4_t*)(p.x + (size_t)mm * p.K + (size_t)c * 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float x0 = TT::to_f32(xv[e] & 0xffff), x1 = TT::to_f32(xv[e] >> 16);
        if constexpr (MR > 1) {
          // Several activation rows: every row runs the SAME chain of fused multiply-adds, in element order. This file is built with
          // -ffast-math, and the free-form expression below was scheduled row by row (a mix of mul + add, fma and packed forms that
          // differed between the unrolled rows): the same sequence then gave other bits in slot 3 than in slot 0. Rows of a lock-step
          // batch are independent requests (in-flight batching moves a request between slots), so a row's result must not depend on
          // its index.
#pragma clang fp reassociate(off) contract(off)
          acc0[m] = __builtin_fmaf(TT::to_f32(a[e] >> 16), x1, __builtin_fmaf(TT::to_f32(a[e] & 0xffff), x0, acc0[m]));
          acc1[m] = __builtin_fmaf(TT::to_f32(b[e] >> 16), x1, __builtin_fmaf(TT::to_f32(b[e] & 0xffff), x0, acc1[m]));
        } else {
          acc0[m] += TT::to_f32(a[e] & 0xffff) * x0 + TT::to_f32(a[e] >> 16) * x1;
          acc1[m] += TT::to_f32(b[e] & 0xffff) * x0 + TT::to_f32(b[e] >> 16) * x1;
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    acc0[m] = wave_sum(acc0[m]);
    acc1[m] = wave_sum(acc1[m]);
  }
  if (lane == 0) {
    const int ncols = p.glu ? p.N / 2 : p.N;
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      if (m >= p.M) break;
      float v0, v1 = 0.f;
      if (p.glu) {
        v0 = acc0[m] * apply_act(acc1[m], p.act);
      } else {
        v0 = apply_act(acc0[m], p.act);
        v1 = apply_act(acc1[m], p.act);
      }
      const size_t o = (size_t)m * ncols + n_out;
      if (p.residual) {
        v0 += p.residual[o];
        if (!p.glu && has1) v1 += p.residual[o + 1];
      }
      if (p.out_dtype == SX_F32) {
        ((float*)p.y)[o] = v0;
        if (!p.glu && has1) ((float*)p.y)[o + 1] = v1;
      } else {
        unsigned short* yy = (unsigned short*)p.y;
        yy[o] = p.out_dtype == SX_BF16 ? BF16::from_f32(v0) : F16::from_f32(v0);
        if (!p.glu && has1) yy[o + 1] = p.out_dtype == SX_BF16 ? BF16::from_f32(v1) : F16::from_f32(v1);
      }
    }
  }
}

// ---- skinny GEMM for 2..16 activation rows (lock-step batched decode): y[M][N] = x[M][K] · W[N][K]^T on MFMA -----------------
// The VALU GEMV above costs M FMAs per weight element and turns compute-bound at M = 8 (≈2x its M = 1 time). Here the
// weight rows are the 16x16x32 MFMA's row operand and x^T (M padded to 16 columns) its column operand, so any M <= 16
// costs the same and the kernel stays on the HBM roofline. Block = 4 waves = 4-way split of K; a wave owns R 16-row groups
// (R = 2 = exactly one GLU group [16 linear | 16 gate]) and streams 128 contiguous bytes of each row per k-step (two 16-B
// non-temporal loads per lane; each load instruction covers one 64-B half line of 16 rows: lane group g = lane >> 4 reads
// bytes [16g, 16g + 16) of it, which is exactly the MFMA's k-slot layout, no shuffle). 4 k-steps are in flight per wave
// (8-16 KB). Partial sums meet in LDS; wave 0 runs the fused epilogue (act / GLU / fp32 residual / store).
// TAIL (w_layout 2, R = 2): the workgroup owns 20 weight rows — MFMA row block 0 = rows 0..15, block 1 = rows 16..19 (its other
// 12 operand rows read a zero line). N = 5120 is 320 16-row groups on 256 CUs: the 64 CUs that get two of them set the time
// (o-proj 3.4 TB/s); as 256 groups of 20 every CU streams the same bytes and no cross-workgroup reduction is needed.
__device__ const unsigned g_zero_line[16] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};

// the hi plane of an fp16 pair saturates at the largest finite value (csrc/precise.hip split1 does the same): the remainder travels in lo
__device__ __forceinline__ f32x4_t sat_f16(f32x4_t x) {
  return (f32x4_t){__builtin_amdgcn_fmed3f(x[0], -65504.f, 65504.f), __builtin_amdgcn_fmed3f(x[1], -65504.f, 65504.f),
                   __builtin_amdgcn_fmed3f(x[2], -65504.f, 65504.f), __builtin_amdgcn_fmed3f(x[3], -65504.f, 65504.f)};
}
// lo plane of four fp32 values whose hi plane (two packed dwords) is `hi`: rn16(x - float(hi)), same element type
__device__ __forceinline__ u32x2_t lo_plane(f32x4_t x, u32x2_t hi, bool bf16) {
  u32x2_t lo;
  if (bf16) {
    lo[0] = pack2<BF16>(x[0] - BF16::to_f32(hi[0] & 0xffff), x[1] - BF16::to_f32(hi[0] >> 16));
    lo[1] = pack2<BF16>(x[2] - BF16::to_f32(hi[1] & 0xffff), x[3] - BF16::to_f32(hi[1] >> 16));
  } else {
    lo[0] = pack2<F16>(x[0] - F16::to_f32(hi[0] & 0xffff), x[1] - F16::to_f32(hi[0] >> 16));
    lo[1] = pack2<F16>(x[2] - F16::to_f32(hi[1] & 0xffff), x[3] - F16::to_f32(hi[1] >> 16));
  }
  return lo;
}

// Eight e4m3 codes (two dwords = one lane's k-slots of one 32-k half) → the eight 16-bit MFMA operand elements, exactly: every
// non-NaN code is a normal fp16 number (>= 2^-9) and has 3 mantissa bits (bf16 keeps 7). fp16: one packed convert per pair
// (v_cvt_scalef32_pk_f16_fp8 with scale 1); bf16: packed convert to fp32, then one v_perm_b32 keeps the two upper halves.
template <typename TT>
__device__ __forceinline__ typename TT::vec8 fp8x8_to16(unsigned d0, unsigned d1) {
  u32x4_t o;
#if defined(__HIP_DEVICE_COMPILE__)
  if (std::is_same<TT, F16>::value) {
    o[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(d0, 1.0f, false));
    o[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(d0, 1.0f, true));
    o[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(d1, 1.0f, false));
    o[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(d1, 1.0f, true));
  } else {
    const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8(d0, false), b = __builtin_amdgcn_cvt_pk_f32_fp8(d0, true);
    const f32x2_t c = __builtin_amdgcn_cvt_pk_f32_fp8(d1, false), d = __builtin_amdgcn_cvt_pk_f32_fp8(d1, true);
    o[0] = __builtin_amdgcn_perm(__float_as_uint(a[1]), __float_as_uint(a[0]), 0x07060302u);
    o[1] = __builtin_amdgcn_perm(__float_as_uint(b[1]), __float_as_uint(b[0]), 0x07060302u);
    o[2] = __builtin_amdgcn_perm(__float_as_uint(c[1]), __float_as_uint(c[0]), 0x07060302u);
    o[3] = __builtin_amdgcn_perm(__float_as_uint(d[1]), __float_as_uint(d[0]), 0x07060302u);
  }
#endif
  return __builtin_bit_cast(typename TT::vec8, o);
}

// Eight e2m1 codes (one dword = one lane's k-slots of one 32-k half, nibble j = slot j, all in one 32-k block) times that block's scale
// 2^e → the eight 16-bit MFMA operand elements: one packed convert per byte, the scale applied inside it. Exact: every code * 2^e with
// e in [-13, 13] is a normal fp16 number with one mantissa bit (and one of bf16).
template <typename TT>
__device__ __forceinline__ typename TT::vec8 fp4x8_to16(unsigned d, float sc) {
  u32x4_t o;
#if defined(__HIP_DEVICE_COMPILE__)
  if (std::is_same<TT, F16>::value) {
    o[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(d, sc, 0));
    o[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(d, sc, 1));
    o[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(d, sc, 2));
    o[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(d, sc, 3));
  } else {
    o[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 0));
    o[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 1));
    o[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 2));
    o[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 3));
  }
#endif
  return __builtin_bit_cast(typename TT::vec8, o);
}

// MB = 2 (17..32 activation rows, lock-step batch 32): the x operand is two 16-row blocks — tiles [2][K/32][16][32] or rows 16..31 of
// the row-major x — and every weight fragment feeds two MFMAs, so the weights still stream ONCE for all 32 sequences. Outputs, the
// 16-bit tiled output, x16_out and the sums of squares follow the same block structure (row m = 16 b + r).
// W8 (sx_gemv_args.w_dtype = SX_FP8_E4M3, w_layout 1 / 2 only): the weight tiles hold e4m3 codes, a 64-k slab of 16 rows is ONE 1-KB
// tile [16][64] whose rows are ordered so that lane (r, g) finds its eight k-slots of both 32-k halves in one 16-B load (include/
// seedx_hip.h) — half the bytes and half the weight loads per k-step. The codes become 16-bit operand elements in registers (exact,
// fp8x8_to16) in front of the same MFMAs; the fp32 row scale multiplies the summed accumulators once in wave 0's epilogue.
// W4 (w_dtype = SX_FP4_E2M1, w_layout 1 / 2 only): MXFP4 tiles — a 64-k slab of 16 rows is one 512-B tile [16][32 B], lane (r, g) loads
// the 8 bytes at 32 r + 8 g (dword h = its eight k-slots of 32-k half h) and the two E8M0 bytes of (row, k-step) from w_bscale; the same
// 64-k step and the same k-slices per wave as the 16-bit kernel. fp4x8_to16 makes the exact operand code * 2^e in front of the same
// MFMAs, so there is no scale in the epilogue: it is the 16-bit one.
template <typename TT, int R, int NWV, int U, bool TAIL = false, int MB = 1, bool W8 = false, bool W4 = false>
__global__ __launch_bounds__(NWV * 64) void gemm_skinny_kernel(const GemvP p) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef typename TT::vec8 vec8;
  static_assert(!TAIL || R == 2, "the 20-row variant is two MFMA row blocks");
  static_assert(!(W8 && W4), "one weight format");
  __shared__ float red[NWV - 1][R * MB][64][4];   // waves 1 .. NWV-1 hand their partial sums to wave 0 (which keeps its own in registers)
  // the wave index as a SCALAR: everything derived from it (k range, round counts) then lives in SGPRs and the guards below
  // are scalar branches. With a VGPR-derived count the compiler predicates the guarded MFMAs through EXEC instead — and
  // MFMA ignores EXEC: the skipped k-steps' (never loaded) registers were multiplied in (found by tools/lab/gemv_lab).
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int n0 = TAIL ? blockIdx.x * 20 : blockIdx.x * 16 * R;
  const int nks = p.K >> 6;
  const int S = gridDim.y;                                           // split-K workgroups per row group (1 = none)
  const int nsl = NWV * S, sl = blockIdx.y * NWV + wave;             // k slices: split-K workgroups x waves
  const int ks0 = sl * nks / nsl, ks1 = (sl + 1) * nks / nsl;
  // x blocks: RB row blocks of 16 activation rows each, times the operand planes — planes2 (fp32-grade activations, x = hi + lo): blocks
  // 0 .. RB-1 = the hi plane's row blocks, RB .. 2 RB - 1 = the lo plane's (MB = 2: 16 rows; MB = 4, round 6: 17..32 rows)
  const int RB = p.planes2 ? MB / 2 : MB;
  bool mvalid[MB];
#pragma unroll
  for (int b = 0; b < MB; ++b) mvalid[b] = r + 16 * (b % RB) < p.M;
  // row-major x: a load instruction touches 16 rows 2K bytes apart — for K = 5120 that stride is a multiple of 16 cache
  // lines, so all 16 rows (and every wave on the chip, in step) hit the same L2 channel. Tiled x: the same instruction reads
  // one contiguous 1-KB tile, consecutive k-steps are consecutive tiles.
  const unsigned short* xp[MB];
#pragma unroll
  for (int b = 0; b < MB; ++b)
    xp[b] = p.x_tiled ? p.x + (size_t)b * (size_t)p.K * 16 + r * 32 + 8 * g : p.x + (size_t)(mvalid[b] ? r + 16 * b : 0) * p.K + 8 * g;
  const size_t xstep = p.x_tiled ? 1024 : 64, xhalf = p.x_tiled ? 512 : 32;
  // row-major W: a load instruction covers one 64-B half line of 16 rows (row stride 2K bytes). Decode layout: the same
  // instruction covers one contiguous 1-KB operand tile, a wave's k range is one contiguous stream.
  const unsigned short* wp[R];
  constexpr int WD = W8 ? 2 : 1;   // FP8 tiles: every tile stride is half as many 16-bit units (lane offset r * 32 + 8 g units = byte r * 64 + 16 g: the same)
  const size_t kstep = (TAIL ? 1280 : (p.packed ? 1024 : 64)) / WD, khalf = TAIL ? 640 : (p.packed ? 512 : 32);   // elements per 64-wide k-step / to its 2nd half (16-bit tiles)
  size_t kstep_q[R], khalf_q[R];
#pragma unroll
  for (int q = 0; q < R; ++q) {
    kstep_q[q] = kstep; khalf_q[q] = khalf;
    wp[q] = p.packed ? p.W + (size_t)(n0 / 16 + q) * (size_t)(p.K >> 5) * (512 / WD) + r * 32 + 8 * g
                     : p.W + (size_t)(n0 + q * 16 + r) * p.K + 8 * g;
  }
  if (TAIL) {   // [N/20][K/32][20 rows][32 k]: a 32-k slab of the group is 1280 B = rows 0..15 (the 1-KB MFMA tile) + rows 16..19
    wp[0] = p.W + (size_t)blockIdx.x * (size_t)(p.K >> 5) * (640 / WD) + r * 32 + 8 * g;   // (FP8: [N/20][K/64][20][64], rows 16..19 behind the 1-KB tile)
    if (r < 4) wp[R - 1] = wp[0] + 512;
    else { wp[R - 1] = (const unsigned short*)g_zero_line; kstep_q[R - 1] = 0; khalf_q[R - 1] = 0; }   // operand rows 4..15 of block 1 = 0
  }
  // MXFP4 tiles: 512 B (20-row: 640 B) of codes and 32 B (40 B) of scales per 64-k step; lane offset 32 r + 8 g bytes / 2 r bytes
  const unsigned char* sp[R];
  size_t sstep_q[R];
  if constexpr (W4) {
#pragma unroll
    for (int q = 0; q < R; ++q) {
      kstep_q[q] = TAIL ? 320 : 256;
      sstep_q[q] = TAIL ? 40 : 32;
      wp[q] = p.W + (size_t)(n0 / 16 + q) * (size_t)(p.K >> 6) * 256 + r * 16 + 4 * g;
      sp[q] = p.w_bscale + (size_t)(n0 / 16 + q) * (size_t)(p.K >> 6) * 32 + 2 * r;
    }
    if (TAIL) {   // [N/20][K/64][20][32 B]: rows 16..19 behind the 512-B tile; scales [N/20][K/64][20][2] alike
      wp[0] = p.W + (size_t)blockIdx.x * (size_t)(p.K >> 6) * 320 + r * 16 + 4 * g;
      sp[0] = p.w_bscale + (size_t)blockIdx.x * (size_t)(p.K >> 6) * 40 + 2 * r;
      if (r < 4) { wp[R - 1] = wp[0] + 256; sp[R - 1] = sp[0] + 32; }
      else {      // operand rows 4..15 of block 1: code 0 from the zero line, whatever the scale bits (0 * 2^e = 0)
        wp[R - 1] = (const unsigned short*)g_zero_line; kstep_q[R - 1] = 0;
        sp[R - 1] = (const unsigned char*)g_zero_line; sstep_q[R - 1] = 0;
      }
    }
  }
  f32x4_t acc[R][MB];
#pragma unroll
  for (int q = 0; q < R; ++q)
#pragma unroll
    for (int b = 0; b < MB; ++b) acc[q][b] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  // folded RMSNorm, consumer side: rstd of row r from the producer's per-workgroup sums of squares [16][parts]. Done HERE, ahead of
  // the weight stream, by all 256 threads at once: thread (slice = tid >> 4, r) loads its 1/16 of row r's list as independent 16-B
  // loads (a serial chain of 20 dependent L2 round trips per workgroup cost 5.7 us per launch), two shuffles + one LDS hop add the
  // 16 slices in a fixed order: every workgroup computes the same bits.
  __shared__ float ssq_red[NWV][16 * MB];
  float rstd_fold[MB];
#pragma unroll
  for (int b = 0; b < MB; ++b) rstd_fold[b] = 1.f;
  if (p.ssq_in) {
    const int per = p.ssq_parts >> 4;                                   // parts % 64 == 0 (host-checked) → per % 4 == 0
#pragma unroll
    for (int b = 0; b < MB; ++b) {
      if (b >= RB) break;                                               // the lo plane's blocks are the same rows: no list of their own
      const f32x4_t* src = (const f32x4_t*)(p.ssq_in + (size_t)(r + 16 * b) * p.ssq_parts + (size_t)(wave * 4 + g) * per);
      float s0 = 0.f;
#pragma unroll 5
      for (int i = 0; i < (per >> 2); ++i) {
        const f32x4_t t = src[i];
        s0 += (t[0] + t[1]) + (t[2] + t[3]);
      }
      s0 += __shfl_xor(s0, 16, 64);
      s0 += __shfl_xor(s0, 32, 64);
      if (g == 0) ssq_red[wave][r + 16 * b] = s0;
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < MB; ++b) {
      if (b >= RB) break;
      float tot = 0.f;
#pragma unroll
      for (int w = 0; w < NWV; ++w) tot += ssq_red[w][r + 16 * b];
      rstd_fold[b] = __builtin_amdgcn_rsqf(tot * p.ssq_inv_dim + p.ssq_eps);
    }
  }
  // Rounds of U k-steps through TWO register sets: round i+1's loads are issued before round i is consumed, so 1-2 rounds
  // (U..2U KB per row group and wave) are in flight at every moment. The pipelined loop has no branch inside (the waitcnt
  // pass then emits exact vmcnt(N) waits; with a guard inside it falls back to vmcnt(0) before the first MFMA). Last full
  // rounds and the < U remainder are peeled. Measured (tools/lab/gemv_lab, profiles/r3_ab_experiments.md §6): the deeper
  // flight alone changes nothing (+-1 %) — the wide shapes already stream at 6.5-6.9 TB/s net of the 3-4 us launch cost;
  // what moved the numbers was the x layout (L2 channel conflicts) and, for K = 13824, split-K.
  struct Frag16 { u32x4_t wa[U][R], wb[U][R], xa[U][MB], xb[U][MB]; };
  struct Frag4 { u32x2_t wa[U][R]; unsigned short ws[U][R]; u32x4_t xa[U][MB], xb[U][MB]; };   // MXFP4: 8 B of codes + the two E8M0 bytes of (row, k-step)
  typedef std::conditional_t<W4, Frag4, Frag16> Frag;
  auto load_round = [&](Frag& f, int ks, int cnt) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u < cnt) {
        const size_t k = (size_t)(ks + u) * xstep;
#pragma unroll
        for (int q = 0; q < R; ++q) {
          if constexpr (W4) {
            f.wa[u][q] = __builtin_nontemporal_load((const u32x2_t*)(wp[q] + (size_t)(ks + u) * kstep_q[q]));
            f.ws[u][q] = *(const unsigned short*)(sp[q] + (size_t)(ks + u) * sstep_q[q]);
          } else {
            f.wa[u][q] = __builtin_nontemporal_load((const u32x4_t*)(wp[q] + (size_t)(ks + u) * kstep_q[q]));
            if (!W8) f.wb[u][q] = __builtin_nontemporal_load((const u32x4_t*)(wp[q] + (size_t)(ks + u) * kstep_q[q] + khalf_q[q]));
          }
        }
#pragma unroll
        for (int b = 0; b < MB; ++b) {
          f.xa[u][b] = *(const u32x4_t*)(xp[b] + k);
          f.xb[u][b] = *(const u32x4_t*)(xp[b] + k + xhalf);
        }
      }
    }
  };
  auto consume = [&](const Frag& f, int cnt) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u < cnt) {
        // lanes of rows >= M carry row 0's x: their output columns (m >= M) are never stored, and an MFMA output column depends
        // on its own B column only — no select on the loaded registers (a VALU op on them at the top of the round makes the
        // waitcnt pass drain every load in flight)
#pragma unroll
        for (int q = 0; q < R; ++q) {
          // FP8: the conversion is VALU work on loaded registers too — here, for the k-step being consumed, never at the top of the round
          vec8 wa, wb;
          if constexpr (W4) {   // MXFP4: dword h = the eight k-slots of half h, byte h of ws = its block's E8M0 scale (fp32 bits: byte << 23)
            const unsigned sc = f.ws[u][q];
            wa = fp4x8_to16<TT>(f.wa[u][q][0], __uint_as_float((sc & 0xffu) << 23));
            wb = fp4x8_to16<TT>(f.wa[u][q][1], __uint_as_float((sc >> 8) << 23));
          } else {
            wa = W8 ? fp8x8_to16<TT>(f.wa[u][q][0], f.wa[u][q][1]) : __builtin_bit_cast(vec8, f.wa[u][q]);
            wb = W8 ? fp8x8_to16<TT>(f.wa[u][q][2], f.wa[u][q][3]) : __builtin_bit_cast(vec8, f.wb[u][q]);
          }
#pragma unroll
          for (int b = 0; b < MB; ++b) {
            acc[q][b] = TT::mfma16(wa, __builtin_bit_cast(vec8, f.xa[u][b]), acc[q][b]);
            acc[q][b] = TT::mfma16(wb, __builtin_bit_cast(vec8, f.xb[u][b]), acc[q][b]);
          }
        }
      }
    }
  };
  {
    Frag A, B;
    const int full = (ks1 - ks0) / U, rem = (ks1 - ks0) % U;
    int i = 0;
    if (full > 0) {
      load_round(A, ks0, U);
      for (; i + 2 < full; i += 2) {
        // sched_barrier: the machine scheduler otherwise hoists the next round's loads above this round's MFMAs (renaming
        // the registers), which turns the loop back into "issue everything, then wait for everything"
        load_round(B, ks0 + (i + 1) * U, U);
        __builtin_amdgcn_sched_barrier(0);
        consume(A, U);
        __builtin_amdgcn_sched_barrier(0);
        load_round(A, ks0 + (i + 2) * U, U);
        __builtin_amdgcn_sched_barrier(0);
        consume(B, U);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (i + 2 == full) {
        load_round(B, ks0 + (i + 1) * U, U);
        consume(A, U);
        if (rem) load_round(A, ks0 + full * U, rem);
        consume(B, U);
      } else {
        if (rem) load_round(B, ks0 + full * U, rem);
        consume(A, U);
        if (rem) { consume(B, rem); }
      }
      if (i + 2 == full && rem) consume(A, rem);
    } else if (rem) {
      load_round(A, ks0, rem);
      consume(A, rem);
    }
  }
  if (wave != 0) {
#pragma unroll
    for (int q = 0; q < R; ++q)
#pragma unroll
      for (int b = 0; b < MB; ++b)
#pragma unroll
        for (int e = 0; e < 4; ++e) red[wave - 1][q * MB + b][lane][e] = acc[q][b][e];
  }
  __syncthreads();
  if (wave != 0) return;
  // FP8: the lane's four row scales per row group, asked for ahead of the LDS / split-K sums that hide the round trip (the 20-row
  // tail's block 1 is rows 16..19 = lane group 0 only: the others would read past the group, at the last one past N)
  f32x4_t wsc[R];
  if (W8) {
#pragma unroll
    for (int q = 0; q < R; ++q)
      wsc[q] = (TAIL && q == 1 && g != 0) ? (f32x4_t){0.f, 0.f, 0.f, 0.f} : *(const f32x4_t*)(p.w_scale + n0 + q * 16 + 4 * g);
  }
  // lane holds y[m = 16 b + r][n0 + q*16 + 4g + e], e = 0..3; the waves' partial sums are added in wave order (0 + w0 == w0: the same bits as
  // when wave 0 went through LDS too)
  f32x4_t v[R][MB];
#pragma unroll
  for (int q = 0; q < R; ++q)
#pragma unroll
    for (int b = 0; b < MB; ++b)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float t = acc[q][b][e];
#pragma unroll
        for (int w = 0; w + 1 < NWV; ++w) t += red[w][q * MB + b][lane][e];
        v[q][b][e] = t;
      }
  if (S > 1) {
    // split-K: every workgroup publishes its partial [16][16R] block; the LAST one to arrive (per row group) adds the S partials
    // in split order — the result does not depend on which workgroup that is — and runs the epilogue. The counter is left at 0.
#pragma unroll
    for (int q = 0; q < R; ++q)
#pragma unroll
      for (int b = 0; b < MB; ++b)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (!(TAIL && q == 1 && g != 0))
            __hip_atomic_store(p.ws_part + ((size_t)blockIdx.y * (16 * MB) + 16 * b + r) * p.N + n0 + q * 16 + 4 * g + e, v[q][b][e],
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // No cache-wide fence (an agent-scope release / acquire writes back and invalidates the whole per-XCD L2 — measured 4x
    // slower kernels): the partials themselves move as agent-scope (sc1) atomics, which are performed at the device's
    // coherence point, so ordering them against the counter only needs "my stores are acknowledged" before the count and
    // "count seen" before the loads.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    unsigned old = 0;
    if (lane == 0) old = __hip_atomic_fetch_add(p.ws_cnt + blockIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    old = __shfl(old, 0);
    if (old != (unsigned)(S - 1)) return;
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int q = 0; q < R; ++q)
#pragma unroll
      for (int b = 0; b < MB; ++b)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float t = 0.f;
          if (!(TAIL && q == 1 && g != 0))
            for (int sidx = 0; sidx < S; ++sidx)
              t += __hip_atomic_load(p.ws_part + ((size_t)sidx * (16 * MB) + 16 * b + r) * p.N + n0 + q * 16 + 4 * g + e, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
          v[q][b][e] = t;
        }
    if (lane == 0) __hip_atomic_store(p.ws_cnt + blockIdx.x, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (MB >= 2 && p.planes2) {   // hi-plane + lo-plane products of the same rows: row block rb = blocks rb and RB + rb
#pragma unroll
    for (int q = 0; q < R; ++q)
#pragma unroll
      for (int b = 0; b < MB / 2; ++b) v[q][b] += v[q][MB / 2 + b];
  }
  if (W8) {   // code sums → weights: once per output, behind every sum and ahead of rstd / activation / GLU (whose two rows differ in scale)
#pragma unroll
    for (int q = 0; q < R; ++q)
#pragma unroll
      for (int b = 0; b < MB; ++b)
        if (b < RB) v[q][b] *= wsc[q];
  }
  if (p.ssq_in) {
#pragma unroll
    for (int q = 0; q < R; ++q)
#pragma unroll
      for (int b = 0; b < MB; ++b)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (b < RB) v[q][b][e] *= rstd_fold[b];
  }
  if (p.addend) {   // pre-activation addend: behind every sum and scale, ahead of activation / GLU / residual; a row that is switched off keeps its bits
#pragma unroll
    for (int b = 0; b < MB; ++b) {
      if (b >= RB) break;
      const int m = r + 16 * b;
      bool on = mvalid[b];
      if (on && p.addend_sel) {
        const int a = p.addend_sel[m];
        on = a >= 0 && a < p.addend_n;
      }
      if (on) {
#pragma unroll
        for (int q = 0; q < R; ++q)
          if (!(TAIL && q == 1 && g != 0)) v[q][b] += *(const f32x4_t*)(p.addend + (size_t)m * p.N + n0 + q * 16 + 4 * g);
      }
    }
  }
  const int ncols = p.glu ? p.N / 2 : p.N;
  const size_t lo_off = (size_t)ncols * 16 * (size_t)((p.M + 15) >> 4);   // planes out: the lo plane follows the hi plane's row blocks
#pragma unroll
  for (int b = 0; b < MB; ++b) {
    if (b >= RB) break;
    float ssq_l = 0.f;
    const int m = r + 16 * b;                               // activation row; 16-bit tiles: block b of [RB][ncols/32][16][32]
    const size_t tblk = (size_t)b * (size_t)ncols * 16;
#pragma unroll
    for (int q = 0; q < R; ++q) {
      if (!mvalid[b]) break;
      if (TAIL && q == 1 && g != 0) break;           // block 1 holds rows 16..19 only: output columns n0 + 16 .. n0 + 19 (lane group 0)
      f32x4_t o;
      int col;
      if (p.glu) {
        if (2 * q + 1 >= R) break;                       // GLU: row groups (2 q, 2 q + 1) = one packed [16 linear | 16 gate] group
        col = (blockIdx.x * (R / 2) + q) * 16 + 4 * g;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = v[2 * q][b][e] * apply_act(v[(2 * q + 1) % R][b][e], p.act);
      } else {
        col = n0 + q * 16 + 4 * g;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = apply_act(v[q][b][e], p.act);
      }
      const size_t off = (size_t)m * ncols + col;
      if (p.residual) o += *(const f32x4_t*)(p.residual + off);
      if (p.y_tiled) {      // 16-bit operand tiles [ncols/32][16][32] for the next skinny GEMM (x_layout = 1)
        u32x2_t w2;
        if (p.out_dtype == SX_BF16) { w2[0] = pack2<BF16>(o[0], o[1]); w2[1] = pack2<BF16>(o[2], o[3]); }
        else if (p.out_planes) { const f32x4_t oc = sat_f16(o); w2[0] = pack2<F16>(oc[0], oc[1]); w2[1] = pack2<F16>(oc[2], oc[3]); }   // hi saturates, lo carries the rest
        else { w2[0] = pack2<F16>(o[0], o[1]); w2[1] = pack2<F16>(o[2], o[3]); }
        unsigned short* yt = (unsigned short*)p.y + tblk + (size_t)(col >> 5) * 512 + (size_t)r * 32 + (col & 31);
        *(u32x2_t*)yt = w2;
        if (p.out_planes) *(u32x2_t*)(yt + lo_off) = lo_plane(o, w2, p.out_dtype == SX_BF16);   // lo plane = o - hi
      } else if (p.out_dtype == SX_F32) {
        *(f32x4_t*)((float*)p.y + off) = o;
        if (p.x16_out) {     // folded RMSNorm, producer side: the new residual stream also as the next GEMV's 16-bit operand tiles
          f32x4_t og = o;      // precise mode: gamma of the NEXT norm goes onto the activation (weights stay exact), two planes
          if (p.x16_gamma) og = o * *(const f32x4_t*)(p.x16_gamma + col);
          u32x2_t w2;
          if (std::is_same<TT, BF16>::value) { w2[0] = pack2<BF16>(og[0], og[1]); w2[1] = pack2<BF16>(og[2], og[3]); }
          else if (p.out_planes) { const f32x4_t oc = sat_f16(og); w2[0] = pack2<F16>(oc[0], oc[1]); w2[1] = pack2<F16>(oc[2], oc[3]); }
          else { w2[0] = pack2<F16>(og[0], og[1]); w2[1] = pack2<F16>(og[2], og[3]); }
          unsigned short* xt = p.x16_out + tblk + (size_t)(col >> 5) * 512 + (size_t)r * 32 + (col & 31);
          *(u32x2_t*)xt = w2;
          if (p.out_planes) *(u32x2_t*)(xt + lo_off) = lo_plane(og, w2, std::is_same<TT, BF16>::value);
          ssq_l += o[0] * o[0] + o[1] * o[1] + o[2] * o[2] + o[3] * o[3];
        }
      } else {
        u32x2_t w2;
        if (p.out_dtype == SX_BF16) { w2[0] = pack2<BF16>(o[0], o[1]); w2[1] = pack2<BF16>(o[2], o[3]); }
        else { w2[0] = pack2<F16>(o[0], o[1]); w2[1] = pack2<F16>(o[2], o[3]); }
        *(u32x2_t*)((unsigned short*)p.y + off) = w2;
      }
    }
    if (p.ssq_out) {                                     // (whole wave: rows >= M contribute zeros and are never read)
      ssq_l += __shfl_xor(ssq_l, 16, 64);
      ssq_l += __shfl_xor(ssq_l, 32, 64);
      if (g == 0) p.ssq_out[(size_t)m * gridDim.x + blockIdx.x] = ssq_l;      // [16 MB][parts]
    }
  }
#endif
}

// ---- decode attention: grid (H, nsplit); 16-lane groups own one key row per iteration ---------------------------
template <typename TT>
__global__ __launch_bounds__(256) void attn_decode_kernel(const unsigned short* q, const unsigned short* kc,
                                                          const unsigned short* vc, float* scratch,
                                                          const int* ctx_len_dev, int D, int Tmax, int nsplit,
                                                          float scale, long long seq_stride, long long q_stride) {
  __shared__ float red[16][132];  // 16 lane-groups x (D<=128 outputs + m + l)
  const int h = blockIdx.x, sp = blockIdx.y, g = blockIdx.z, H = gridDim.x;
  const int ctx = ctx_len_dev[g];
  q += (size_t)g * q_stride;
  kc += (size_t)g * seq_stride;
  vc += (size_t)g * seq_stride;
  scratch += (size_t)g * H * nsplit * (D + 2);
  const int chunk = (ctx + nsplit - 1) / nsplit;
  const int t0 = sp * chunk, t1 = min(ctx, t0 + chunk);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int grp = wave * 4 + (lane >> 4);  // 0..15
  const int dl = lane & 15;                // 16-B chunk of the head dim (8 elements); D = 128 → 16 chunks
  const bool dvalid = dl * 8 < D;
  float qv[8];
  {
    u32x4_t raw = {0u, 0u, 0u, 0u};
    if (dvalid) raw = *(const u32x4_t*)(q + (size_t)h * D + dl * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      qv[2 * e] = TT::to_f32(raw[e] & 0xffff) * scale;
      qv[2 * e + 1] = TT::to_f32(raw[e] >> 16) * scale;
    }
  }
  float m_run = -INFINITY, l_run = 0.f, o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = 0.f;
  const unsigned short* kh = kc + (size_t)h * Tmax * D;
  const unsigned short* vh = vc + (size_t)h * Tmax * D;
  for (int t = t0 + grp; t < t1; t += 16) {
    u32x4_t kr = {0u, 0u, 0u, 0u}, vr = {0u, 0u, 0u, 0u};
    if (dvalid) {
      kr = *(const u32x4_t*)(kh + (size_t)t * D + dl * 8);
      vr = *(const u32x4_t*)(vh + (size_t)t * D + dl * 8);
    }
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      s += TT::to_f32(kr[e] & 0xffff) * qv[2 * e] + TT::to_f32(kr[e] >> 16) * qv[2 * e + 1];
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    s += __shfl_xor(s, 8, 64);
    const float m_new = fmaxf(m_run, s);
    const float alpha = __expf(m_run - m_new);  // exp(-inf) = 0 on the first key
    const float pr = __expf(s - m_new);
    l_run = l_run * alpha + pr;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o[2 * e] = o[2 * e] * alpha + pr * TT::to_f32(vr[e] & 0xffff);
      o[2 * e + 1] = o[2 * e + 1] * alpha + pr * TT::to_f32(vr[e] >> 16);
    }
    m_run = m_new;
  }
  if (dvalid) {
#pragma unroll
    for (int e = 0; e < 8; ++e) red[grp][dl * 8 + e] = o[e];
  }
  if (dl == 0) {
    red[grp][128] = m_run;
    red[grp][129] = l_run;
  }
  __syncthreads();
  // combine the 16 groups: thread d < D
  const int d = threadIdx.x;
  float* out = scratch + ((size_t)h * nsplit + sp) * (D + 2);
  float mg = -INFINITY;
#pragma unroll
  for (int g = 0; g < 16; ++g) mg = fmaxf(mg, red[g][128]);
  if (d < D) {
    float acc = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const float mgk = red[g][128];
      const float w = (mgk == -INFINITY) ? 0.f : __expf(mgk - mg);
      acc += w * red[g][d];
    }
    out[d] = acc;
  }
  if (d == 0) {
    float lsum = 0.f;
    for (int g = 0; g < 16; ++g) {
      const float mgk = red[g][128];
      lsum += (mgk == -INFINITY) ? 0.f : __expf(mgk - mg) * red[g][129];
    }
    out[D] = mg;
    out[D + 1] = lsum;
  }
}

// ---- fused decode attention: RoPE of the new token + KV append + split-KV attention + combine, ONE launch ------------------------
// The three-kernel form above costs 6 us (rope) + 18 us (attention) + 5.5 us (combine) per layer, two of them launch-latency
// sized. Here every (head, split, sequence) workgroup rotates q itself (128 values), the one 16-lane group whose key index is the
// new position takes K / V of the new token straight from the qkv row (rotating K, writing both into the cache for later
// steps), and the LAST split of a head to arrive (agent-scope partial stores + arrival counter, as in the skinny GEMM's
// split-K) combines the partials in split order. Same arithmetic, same order, same roundings as rope_kv_append_kernel +
// attn_decode_kernel + attn_decode_combine_kernel: bit-identical output and cache contents.
struct AttnDecP {
  const unsigned short* qkv;   // [G][3*H*D]: q | k | v of the new token, un-rotated
  unsigned short* kc;
  unsigned short* vc;
  unsigned short* out;
  float* scratch;              // [G][H][nsplit][D + 2]
  unsigned* counters;          // [G*H], zero between launches
  const float* cos_t;
  const float* sin_t;
  const int* pos_dev;          // [G]
  int H, D, Tmax, nsplit, tiled;
  float scale;
  long long seq_stride;
};

template <typename TT>
__device__ __forceinline__ void rope_chunk(const unsigned short* base, int dl, int D, const float* cos_t, const float* sin_t, int pos,
                                           float* out8) {
  // rotated elements 8dl .. 8dl+7 of a D-wide head vector at `base`, rounded to the activation dtype (rope_kv_append_kernel)
  const int half = D / 2, j0 = dl * 8;
  const bool lo = j0 < half;
  const u32x4_t a = *(const u32x4_t*)(base + j0);
  const u32x4_t b = *(const u32x4_t*)(base + (lo ? j0 + half : j0 - half));
  // the 8 table entries of this chunk are contiguous (half % 8 == 0): two 16-B loads per table
  const size_t tb = (size_t)pos * half + (lo ? j0 : j0 - half);
  const f32x4_t c0 = *(const f32x4_t*)(cos_t + tb), c1 = *(const f32x4_t*)(cos_t + tb + 4);
  const f32x4_t s0 = *(const f32x4_t*)(sin_t + tb), s1 = *(const f32x4_t*)(sin_t + tb + 4);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float c = TT::to_f32(TT::from_f32(e < 4 ? c0[e & 3] : c1[e & 3]));
    const float sn = TT::to_f32(TT::from_f32(e < 4 ? s0[e & 3] : s1[e & 3]));
    const float x = TT::to_f32((e & 1) ? (a[e >> 1] >> 16) : (a[e >> 1] & 0xffff));
    const float y = TT::to_f32((e & 1) ? (b[e >> 1] >> 16) : (b[e >> 1] & 0xffff));
    // first half: x*c - y*s (y = partner in the second half); second half: x*c + y*s (y = partner in the first half)
    out8[e] = TT::to_f32(TT::from_f32(lo ? x * c - y * sn : x * c + y * sn));
  }
}

template <typename TT>
__global__ __launch_bounds__(256) void attn_decode_fused_kernel(const AttnDecP p) {
  __shared__ float red[16][132];
  __shared__ unsigned s_last;
  const int h = blockIdx.x, sp = blockIdx.y, g = blockIdx.z, H = p.H, D = p.D, nsplit = p.nsplit;
  const int pos = p.pos_dev[g];
  const bool pos_ok = pos >= 0 && pos < p.Tmax;
  const int ctx = pos_ok ? pos + 1 : (pos < 0 ? 0 : p.Tmax);   // a position past the cache: attend to the cache only, write nothing
  const unsigned short* row = p.qkv + (size_t)g * 3 * H * D;
  unsigned short* kh = p.kc + (size_t)g * p.seq_stride + (size_t)h * p.Tmax * D;
  unsigned short* vh = p.vc + (size_t)g * p.seq_stride + (size_t)h * p.Tmax * D;
  float* scratch = p.scratch + (size_t)g * H * nsplit * (D + 2);
  const int chunk = (ctx + nsplit - 1) / nsplit;
  const int t0 = sp * chunk, t1 = min(ctx, t0 + chunk);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int grp = wave * 4 + (lane >> 4);
  const int dl = lane & 15;
  const bool dvalid = dl * 8 < D;
  const int rpos = pos_ok ? pos : 0;
  float qv[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) qv[e] = 0.f;
  if (dvalid) {
    rope_chunk<TT>(row + (size_t)h * D, dl, D, p.cos_t, p.sin_t, rpos, qv);
#pragma unroll
    for (int e = 0; e < 8; ++e) qv[e] *= p.scale;
  }
  float m_run = -INFINITY, l_run = 0.f, o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = 0.f;
  for (int t = t0 + grp; t < t1; t += 16) {
    float kf[8], vf[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { kf[e] = 0.f; vf[e] = 0.f; }
    if (dvalid) {
      if (pos_ok && t == pos) {      // the new token: from the qkv row, and into the cache
        rope_chunk<TT>(row + (size_t)(H + h) * D, dl, D, p.cos_t, p.sin_t, pos, kf);
        const u32x4_t vr = *(const u32x4_t*)(row + (size_t)(2 * H + h) * D + dl * 8);
        u32x4_t kw;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          kw[e] = (unsigned)TT::from_f32(kf[2 * e]) | ((unsigned)TT::from_f32(kf[2 * e + 1]) << 16);
          vf[2 * e] = TT::to_f32(vr[e] & 0xffff);
          vf[2 * e + 1] = TT::to_f32(vr[e] >> 16);
        }
        *(u32x4_t*)(kh + (size_t)pos * D + dl * 8) = kw;
        *(u32x4_t*)(vh + (size_t)pos * D + dl * 8) = vr;
      } else {
        const u32x4_t kr = *(const u32x4_t*)(kh + (size_t)t * D + dl * 8);
        const u32x4_t vr = *(const u32x4_t*)(vh + (size_t)t * D + dl * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          kf[2 * e] = TT::to_f32(kr[e] & 0xffff); kf[2 * e + 1] = TT::to_f32(kr[e] >> 16);
          vf[2 * e] = TT::to_f32(vr[e] & 0xffff); vf[2 * e + 1] = TT::to_f32(vr[e] >> 16);
        }
      }
    }
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) s += kf[2 * e] * qv[2 * e] + kf[2 * e + 1] * qv[2 * e + 1];
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    s += __shfl_xor(s, 8, 64);
    const float m_new = fmaxf(m_run, s);
    const float alpha = __expf(m_run - m_new);
    const float pr = __expf(s - m_new);
    l_run = l_run * alpha + pr;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = o[e] * alpha + pr * vf[e];
    m_run = m_new;
  }
  if (dvalid) {
#pragma unroll
    for (int e = 0; e < 8; ++e) red[grp][dl * 8 + e] = o[e];
  }
  if (dl == 0) {
    red[grp][128] = m_run;
    red[grp][129] = l_run;
  }
  __syncthreads();
  const int d = threadIdx.x;
  float* part = scratch + ((size_t)h * nsplit + sp) * (D + 2);
  float mg = -INFINITY;
#pragma unroll
  for (int gg = 0; gg < 16; ++gg) mg = fmaxf(mg, red[gg][128]);
  if (nsplit == 1) {
    // one split per head: this workgroup holds the whole result — no partials in memory, no counter, no second pass. The
    // split's (acc, m, l) go through LDS and the combine's arithmetic runs on them unchanged (same expressions as the split
    // path and the combine below, so the bits are those of the three-launch form)
    __shared__ float fin[132];
    if (d < D) {
      float acc = 0.f;
#pragma unroll
      for (int gg = 0; gg < 16; ++gg) {
        const float mgk = red[gg][128];
        const float w = (mgk == -INFINITY) ? 0.f : __expf(mgk - mg);
        acc += w * red[gg][d];
      }
      fin[d] = acc;
    }
    if (d == 0) {
      float lsum = 0.f;
      for (int gg = 0; gg < 16; ++gg) {
        const float mgk = red[gg][128];
        lsum += (mgk == -INFINITY) ? 0.f : __expf(mgk - mg) * red[gg][129];
      }
      fin[D] = mg;
      fin[D + 1] = lsum;
    }
    __syncthreads();
    if (d >= D) return;
    float mall = -INFINITY;
    mall = fmaxf(mall, fin[D]);
    const float ms = fin[D];
    const float w1 = (ms == -INFINITY) ? 0.f : __expf(ms - mall);
    float a2 = 0.f, l2 = 0.f;
    a2 += w1 * fin[d];
    l2 += w1 * fin[D + 1];
    const int col1 = h * D + d;
    const size_t o1 = p.tiled ? (size_t)(g >> 4) * (size_t)H * D * 16 + (size_t)(col1 >> 5) * 512 + (size_t)(g & 15) * 32 + (col1 & 31)
                              : (size_t)g * H * D + col1;
    p.out[o1] = TT::from_f32(l2 > 0.f ? a2 / l2 : 0.f);
    return;
  }
  if (d < D) {
    float acc = 0.f;
#pragma unroll
    for (int gg = 0; gg < 16; ++gg) {
      const float mgk = red[gg][128];
      const float w = (mgk == -INFINITY) ? 0.f : __expf(mgk - mg);
      acc += w * red[gg][d];
    }
    __hip_atomic_store(part + d, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (d == 0) {
    float lsum = 0.f;
    for (int gg = 0; gg < 16; ++gg) {
      const float mgk = red[gg][128];
      lsum += (mgk == -INFINITY) ? 0.f : __expf(mgk - mg) * red[gg][129];
    }
    __hip_atomic_store(part + D, mg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(part + D + 1, lsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // arrival: every thread's partial stores are acknowledged, then one count per workgroup; the last split combines
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0)
    s_last = __hip_atomic_fetch_add(p.counters + (size_t)g * H + h, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(nsplit - 1);
  __syncthreads();
  if (!s_last) return;
  if (threadIdx.x == 0) __hip_atomic_store(p.counters + (size_t)g * H + h, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (d >= D) return;
  const float* base = scratch + (size_t)h * nsplit * (D + 2);
  float mall = -INFINITY, acc = 0.f, l = 0.f;
  if (nsplit <= 8) {
    // all 3 x nsplit partial loads in flight together (they miss to memory: the partials came from other CUs / XCDs), then the
    // same arithmetic in the same order as the loop below
    float pm[8], pl[8], pa[8];
#pragma unroll
    for (int s2 = 0; s2 < 8; ++s2) {
      const size_t o2 = (size_t)(s2 < nsplit ? s2 : 0) * (D + 2);
      pm[s2] = __hip_atomic_load(base + o2 + D, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      pl[s2] = __hip_atomic_load(base + o2 + D + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      pa[s2] = __hip_atomic_load(base + o2 + d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int s2 = 0; s2 < 8; ++s2)
      if (s2 < nsplit) mall = fmaxf(mall, pm[s2]);
#pragma unroll
    for (int s2 = 0; s2 < 8; ++s2)
      if (s2 < nsplit) {
        const float w = (pm[s2] == -INFINITY) ? 0.f : __expf(pm[s2] - mall);
        acc += w * pa[s2];
        l += w * pl[s2];
      }
  } else {
    for (int s2 = 0; s2 < nsplit; ++s2)
      mall = fmaxf(mall, __hip_atomic_load(base + (size_t)s2 * (D + 2) + D, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    for (int s2 = 0; s2 < nsplit; ++s2) {
      const float ms = __hip_atomic_load(base + (size_t)s2 * (D + 2) + D, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const float w = (ms == -INFINITY) ? 0.f : __expf(ms - mall);
      acc += w * __hip_atomic_load(base + (size_t)s2 * (D + 2) + d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      l += w * __hip_atomic_load(base + (size_t)s2 * (D + 2) + D + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  const int col = h * D + d;
  const size_t oo = p.tiled ? (size_t)(g >> 4) * (size_t)H * D * 16 + (size_t)(col >> 5) * 512 + (size_t)(g & 15) * 32 + (col & 31)
                            : (size_t)g * H * D + col;
  p.out[oo] = TT::from_f32(l > 0.f ? acc / l : 0.f);
}

template <typename TT>
__global__ void attn_decode_combine_kernel(const float* scratch, unsigned short* out, int D, int nsplit, int tiled) {
  const int h = blockIdx.x, d = threadIdx.x, g = blockIdx.y, H = gridDim.x;
  if (d >= D) return;
  scratch += (size_t)g * H * nsplit * (D + 2);
  const float* base = scratch + (size_t)h * nsplit * (D + 2);
  float mg = -INFINITY;
  for (int s = 0; s < nsplit; ++s) mg = fmaxf(mg, base[(size_t)s * (D + 2) + D]);
  float acc = 0.f, l = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float ms = base[(size_t)s * (D + 2) + D];
    const float w = (ms == -INFINITY) ? 0.f : __expf(ms - mg);
    acc += w * base[(size_t)s * (D + 2) + d];
    l += w * base[(size_t)s * (D + 2) + D + 1];
  }
  const int col = h * D + d;                     // of row g in [G][H*D]; SX_TILED16: tile col/32, row g, column col%32
  const size_t o = tiled ? (size_t)(g >> 4) * (size_t)H * D * 16 + (size_t)(col >> 5) * 512 + (size_t)(g & 15) * 32 + (col & 31)
                         : (size_t)g * H * D + col;      // sequences 16..31: a second block of tiles behind the first
  out[o] = TT::from_f32(l > 0.f ? acc / l : 0.f);
}

// ---- RoPE + KV append ----------------------------------------------------------------------------------------------
template <typename TT>
__global__ void rope_kv_append_kernel(unsigned short* qkv, unsigned short* kc, unsigned short* vc, const float* cos_t,
                                      const float* sin_t, const int* pos0_dev, int T, int H, int D, int Tmax, int G,
                                      long long seq_stride) {
  const int half = D / 2;
  const int64_t total = (int64_t)G * T * H * half;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(i % half);
    const int h = (int)((i / half) % H);
    const int r = (int)(i / ((int64_t)half * H));     // row of qkv = g*T + t
    const int g = r / T, t = r - g * T;
    int pos = pos0_dev[g] + t;
    const bool pos_ok = pos >= 0 && pos < Tmax;
    if (!pos_ok) pos = 0;                   // keep the table reads in range; the cache write below is skipped
    // tables are rounded to the activation dtype before use (modeling_llama_xformer.py:128-131)
    const float c = TT::to_f32(TT::from_f32(cos_t[(size_t)pos * half + j]));
    const float s = TT::to_f32(TT::from_f32(sin_t[(size_t)pos * half + j]));
    unsigned short* row = qkv + (size_t)r * 3 * H * D;
    unsigned short* qh = row + (size_t)h * D;
    const unsigned short* kh = row + (size_t)(H + h) * D;
    const unsigned short* vh = row + (size_t)(2 * H + h) * D;
    const float q1 = TT::to_f32(qh[j]), q2 = TT::to_f32(qh[j + half]);
    qh[j] = TT::from_f32(q1 * c - q2 * s);
    qh[j + half] = TT::from_f32(q2 * c + q1 * s);
    const float k1 = TT::to_f32(kh[j]), k2 = TT::to_f32(kh[j + half]);
    if (!pos_ok) continue;                  // device-resident position past the cache: never write outside it
    unsigned short* kd = kc + (size_t)g * seq_stride + ((size_t)h * Tmax + pos) * D;
    unsigned short* vd = vc + (size_t)g * seq_stride + ((size_t)h * Tmax + pos) * D;
    kd[j] = TT::from_f32(k1 * c - k2 * s);
    kd[j + half] = TT::from_f32(k2 * c + k1 * s);
    vd[j] = vh[j];
    vd[j + half] = vh[j + half];
  }
}

template <typename TT>
__global__ void embedding_kernel(const int* ids, const unsigned short* table, float* out, int T, int dim) {
  const int64_t total = (int64_t)T * dim;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int t = (int)(i / dim), d = (int)(i % dim);
    out[i] = TT::to_f32(table[(size_t)ids[t] * dim + d]);
  }
}

__global__ void scatter_rows_kernel(const float* src, const int* rows, float* dst, int n, int dim) {
  const int64_t total = (int64_t)n * dim;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / dim), d = (int)(i % dim);
    dst[(size_t)rows[r] * dim + d] = src[i];
  }
}

// dst[(g*seq_rows + step[g])][:] = src[g][:]  (per-sequence hidden-state log of the lock-step batched decode)
__global__ void scatter_rows_step_kernel(const float* src, const int* step, float* dst, int G, int dim, int seq_rows) {
  const int64_t total = (int64_t)G * dim;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int g = (int)(i / dim), d = (int)(i % dim);
    const int st = step[g];
    if (st < 0 || st >= seq_rows) continue;  // device-resident step past the log: drop the row instead of corrupting HBM
    dst[((size_t)g * seq_rows + st) * dim + d] = src[i];
  }
}

// ---- greedy next token with the AutoImageTokenGenerationProcessor rule (generation.py:19-31) ------------------------
// One workgroup of 1024 threads per logits row; the rule and the first-maximal-index arg-max exist once, for every form of
// next_token_kernel below.
// The rule's prologue: prev in img_ids[:-1] → its index there, so that the caller forces the next id of the chain (scores[next] =
// max + 10 in the reference); else -1, with the image columns of the row zeroed in place (the only edit of the row) and visible to
// every thread. Every thread returns the same value.
__device__ __forceinline__ int image_chain_index(float* logits, const int* img_ids, int n_img, int prev) {
  __shared__ int forced;
  if (threadIdx.x == 0) forced = -1;
  __syncthreads();
  // list.index() returns the FIRST match; ids are unique so max == first
  if ((int)threadIdx.x < n_img - 1 && img_ids[threadIdx.x] == prev) atomicMax(&forced, (int)threadIdx.x);
  __syncthreads();
  if (forced >= 0) return forced;
  if ((int)threadIdx.x < n_img - 1) logits[img_ids[1 + threadIdx.x]] = 0.0f;
  __syncthreads();
  return -1;
}

// first maximal index of the row; every thread returns it
__device__ __forceinline__ int row_argmax(const float* logits, int vocab) {
  __shared__ float smax[16];
  __shared__ int sidx[16];
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = threadIdx.x; i < vocab; i += 1024) {
    const float v = logits[i];
    if (v > best || (v == best && i < bi)) { best = v; bi = i; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  if ((threadIdx.x & 63) == 0) { smax[threadIdx.x >> 6] = best; sidx[threadIdx.x >> 6] = bi; }
  __syncthreads();
  best = smax[0];
  bi = sidx[0];
  for (int w = 1; w < 16; ++w)
    if (smax[w] > best || (smax[w] == best && sidx[w] < bi)) { best = smax[w]; bi = sidx[w]; }
  return bi;
}

__device__ __forceinline__ int greedy_next_id(float* logits, int vocab, const int* img_ids, int n_img, int prev) {
  const int f = image_chain_index(logits, img_ids, n_img, prev);
  return f >= 0 ? img_ids[f + 1] : row_argmax(logits, vocab);
}

// ---- the tail of the token step: next id, and in the in-flight form stop rule + slot advance, one launch ------------------------
// Two forms of one kernel (next_token_kernel; the kernel-statistics files under profiles/ list its ancestors greedy_next_kernel and
// greedy_next_slots_kernel). LOCK-STEP (live == NULL; sx_greedy_next, sx_greedy_next_b, sx_sample_next_b): every row takes its next
// id and stores it; the host-side step advances the counters. IN-FLIGHT (sx_greedy_next_slots, sx_sample_next_slots):
// Slot g of the lock-step decode step is either LIVE (a request occupies it) or PARKED (free: the host has not refilled it yet).
// A parked slot keeps stepping through the GEMVs with the others (the weights stream once for all rows anyway) but must leave no
// trace: its counters hold the idle values
//     step = -1  → scatter_rows_step_kernel and the out_ids guard drop the row,
//     pos  = -1  → the RoPE / append kernels and both fused attention kernels write nothing (pos_ok is false),
//     ctx  =  0  → ctx == pos + 1 as always: the plain attention sees no key (its combine yields 0, not 0 / 0); the fp32 attention
//                  sees no key either (kend = 0: a reused slot's stale rows are never read) and yields 0 as well,
// and this kernel returns for it before it touches anything, the in-place zeroing of its logits row included.
// A live slot takes the next id by the shared rule, stores it, advances its four counters and tests the stop rule (EOS or budget) on
// the device; a slot that stops parks itself here, so the very next replay of the captured step already treats it as idle.
struct TailP {
  float* logits;
  const int* img_ids;
  const int* prev;     // [G] the token just fed; in-flight: cur
  int* next;           // [G] the next token (may alias prev); in-flight: cur
  int* out_ids;
  int* step;           // lock-step: read only, may be NULL without out_ids
  int ld_logits, vocab, n_img, ld_out, G;
  // in-flight form only
  int* live;
  int* n_new;
  const int* max_new;
  const int* force_at;
  int* pos;
  int* ctx;
  int* status;
  int force_id, eos_id;
};

// ---- seeded sampling: temperature → top-k → top-p → draw, one workgroup per row (sx_sample_next_b / sx_sample_next_slots) -------------
// transformers' sample() order (processors, then TemperatureLogitsWarper → TopKLogitsWarper → TopPLogitsWarper) in one launch, without a
// sort and without a workspace. The row is read from memory ONCE into registers in a blocked layout (thread t holds the columns
// [32 t, 32 t + 32): the index-ordered prefix sum of the draw is then one scan over the threads), as
//   key_i = order-preserving 32-bit image of x_i (ordering by x is the ordering by t = x / T since T > 0; padding columns get key 0),
//   w_i   = exp((x_i − max x) / T) in fp32 (= exp(t_i − max t); the rounding error of the exponent is relative to the distance from
//           the maximum, so the tokens that carry mass are the accurate ones),
//   q_i   = w_i · 2^40 as an integer (at least 1 where w_i > 0). Where the fp32 weight itself underflows to 0 (x_i more than about
//           87 T .. 103 T below the maximum: a probability below 2^-126; -inf columns likewise) the mass is 0: such a token is never
//           drawn, and it is neither kept nor counted in n_kept — with top_p = 1 too, where the written rule would keep every finite
//           token. The fp64 statement drops it the same way once (larger mass) / W_k rounds to 1.
// Every sum that decides something is a sum of the q_i in 64-bit integers, hence exact and independent of order, slot, launch and
// replay: the id is a function of the row's values, the four parameters, the seed and the token index alone. Both thresholds come from
// one radix select over the key (12 + 10 + 10 bits, an LDS histogram of integer masses per pass): it returns the smallest key v with
// (mass of the keys above v) < target — with unit masses and target k that is the k-th largest value (ties at it are kept), with the
// masses q and target ⌈top_p · W_k⌉ it is the nucleus threshold τ (kept iff the mass of the strictly larger survivors is below top_p;
// equal values are kept or dropped together). The draw takes u = (Philox4x32-10((n, 0, 0, 0), seed)[0] >> 8) · 2^-24 and returns the
// smallest index of the kept set whose inclusive prefix mass exceeds u · W, again in integers.
typedef unsigned long long smp_u64;
constexpr int SMP_NPT = 32;            // columns per thread: rows of up to 32768 columns stay in registers
constexpr int SMP_MAX_VOCAB = SMP_NPT * 1024;

struct SampleP {
  const int* do_sample;
  const float* temperature;
  const int* top_k;
  const float* top_p;
  const unsigned* seed;
  const int* token_index;
  int* n_kept;
  float* p_chosen;
};

__device__ __forceinline__ unsigned philox4x32_10_first(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c0;
}

__device__ __forceinline__ unsigned smp_key(float x) {
  unsigned u = __float_as_uint(x);
  if (u == 0x80000000u) u = 0u;                            // −0 → +0 on the bits (x + 0.0f is folded away under fast-math): equal values, equal keys
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float smp_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
__device__ __forceinline__ smp_u64 smp_q(float w) {
  const smp_u64 q = (smp_u64)(w * 1099511627776.0f);       // 2^40: exact scaling, truncation below 2^-40
  return (w > 0.f && q == 0) ? 1 : q;
}

// exclusive prefix of v over the threads of the workgroup in thread order, and the total; wsum: 16 LDS entries
__device__ __forceinline__ smp_u64 smp_block_scan(smp_u64 v, smp_u64* wsum, smp_u64& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  smp_u64 inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const smp_u64 n = __shfl_up(inc, o, 64);
    if (lane >= o) inc += n;
  }
  __syncthreads();                                         // the readers of an earlier call are through
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  smp_u64 base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < 16; ++w) {
    const smp_u64 s = wsum[w];
    if (w < wv) base += s;
    tot += s;
  }
  total = tot;
  return base + inc - v;
}

// Radix select (see above) over the elements with key >= lo_key (lo_key >= 1 leaves the padding out). MASS: the masses are q(w), else 1.
// Needs 1 <= target <= total mass of those elements; returns a key that one of them has.
template <bool MASS>
__device__ __forceinline__ unsigned smp_select(const unsigned (&key)[SMP_NPT], const float (&w)[SMP_NPT], unsigned lo_key, smp_u64 target,
                                               smp_u64* hist, smp_u64* wsum, smp_u64* sel) {
  unsigned prefix = 0, himask = 0;
  smp_u64 acc = 0;                                         // mass of the keys above the current bucket
#pragma unroll
  for (int pass = 0; pass < 3; ++pass) {
    const int shift = pass == 0 ? 20 : pass == 1 ? 10 : 0;
    const int nb = pass == 0 ? 4096 : 1024, per = nb / 1024;
    for (int b = threadIdx.x; b < nb; b += 1024) hist[b] = 0;
    if (threadIdx.x == 0) { sel[0] = 0; sel[1] = acc; }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SMP_NPT; ++j)
      if (key[j] >= lo_key && (key[j] & himask) == prefix)
        atomicAdd(&hist[(key[j] >> shift) & (nb - 1)], MASS ? smp_q(w[j]) : (smp_u64)1);    // integer: any arrival order, same sum
    __syncthreads();
    // thread t owns the bins nb − 1 − (t·per + j), highest first: the scan over the threads yields the mass above them
    smp_u64 h[4], mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      h[j] = j < per ? hist[nb - 1 - ((int)threadIdx.x * per + j)] : 0;
      mine += h[j];
    }
    smp_u64 tot;
    smp_u64 above = acc + smp_block_scan(mine, wsum, tot);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < per && above < target && above + h[j] >= target) {        // exactly one bin of one thread
        sel[0] = (smp_u64)(nb - 1 - ((int)threadIdx.x * per + j));
        sel[1] = above;
      }
      above += h[j];
    }
    __syncthreads();
    prefix |= (unsigned)sel[0] << shift;
    acc = sel[1];
    himask |= (unsigned)(nb - 1) << shift;
    __syncthreads();                                       // sel and hist are rewritten by the next pass
  }
  return prefix;
}

// The next id of row g by the rule above; every thread returns it. n: 0-based index of the generated token within its request.
// Greedy rows (do_sample = 0) and rows inside the forced image chain take greedy_next_id's path and value.
// There is ONE copy of this function in the library (next_token_kernel<true> serves the lock-step and the in-flight form), so a
// request draws the same ids in both by construction, whatever -ffast-math makes of the weight arithmetic.
__device__ __forceinline__ int sample_next_id(float* logits, int vocab, const int* img_ids, int n_img, int prev, const SampleP& s,
                                              int g, int n) {
  __shared__ smp_u64 hist[4096];
  __shared__ smp_u64 wsum[16];
  __shared__ smp_u64 sel[2];
  __shared__ unsigned wmax[16];
  __shared__ int chosen;
  __shared__ float chosen_p;
  const int f = image_chain_index(logits, img_ids, n_img, prev);
  if (f >= 0 || s.do_sample[g] == 0) {                      // the next chain id or the arg-max: nothing is drawn (probability 1)
    if (threadIdx.x == 0) {
      if (s.n_kept) s.n_kept[g] = -1;
      if (s.p_chosen) s.p_chosen[g] = 1.0f;
    }
    return f >= 0 ? img_ids[f + 1] : row_argmax(logits, vocab);
  }
  // ---- the row, once ----
  unsigned key[SMP_NPT];
  float w[SMP_NPT];
  const int i0 = (int)threadIdx.x * SMP_NPT;
  const bool vec = (((uintptr_t)logits) & 15) == 0;
#pragma unroll
  for (int j = 0; j < SMP_NPT; j += 4) {
    const int i = i0 + j;
    if (vec && i + 4 <= vocab) {
      const float4 v = *reinterpret_cast<const float4*>(logits + i);
      key[j] = smp_key(v.x); key[j + 1] = smp_key(v.y); key[j + 2] = smp_key(v.z); key[j + 3] = smp_key(v.w);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) key[j + e] = i + e < vocab ? smp_key(logits[i + e]) : 0u;
    }
  }
  unsigned km = 0;
#pragma unroll
  for (int j = 0; j < SMP_NPT; ++j) km = max(km, key[j]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) km = max(km, (unsigned)__shfl_xor((int)km, o, 64));
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = km;
  __syncthreads();
  km = wmax[0];
#pragma unroll
  for (int v = 1; v < 16; ++v) km = max(km, wmax[v]);
  const float xmax = smp_unkey(km);
  const float T = s.temperature[g];
#pragma unroll
  for (int j = 0; j < SMP_NPT; ++j) w[j] = key[j] ? expf((smp_unkey(key[j]) - xmax) / T) : 0.f;
  // ---- top-k: the k-th largest value ----
  const int k = s.top_k[g];
  unsigned kth = 1;
  if (k > 0 && k < vocab) kth = smp_select<false>(key, w, 1u, (smp_u64)k, hist, wsum, sel);
  // ---- top-p over the survivors ----
  smp_u64 part = 0, Wk;
#pragma unroll
  for (int j = 0; j < SMP_NPT; ++j)
    if (key[j] >= kth) part += smp_q(w[j]);
  smp_block_scan(part, wsum, Wk);
  smp_u64 target = (smp_u64)ceil((double)s.top_p[g] * (double)Wk);
  target = target < 1 ? 1 : target > Wk ? Wk : target;
  const unsigned tau = smp_select<true>(key, w, kth, target, hist, wsum, sel);
  // ---- draw: smallest kept index whose inclusive prefix mass exceeds u · W ----
  part = 0;
  smp_u64 cnt = 0, W, nk;
#pragma unroll
  for (int j = 0; j < SMP_NPT; ++j)
    if (key[j] >= tau) { part += smp_q(w[j]); cnt += 1; }
  const smp_u64 base = smp_block_scan(part, wsum, W);
  smp_block_scan(cnt, wsum, nk);
  const smp_u64 m = philox4x32_10_first((unsigned)n, 0u, 0u, 0u, s.seed[2 * g], s.seed[2 * g + 1]) >> 8;
  const smp_u64 thr = m * (W >> 24) + ((m * (W & 0xffffffull)) >> 24);      // ⌊m · W / 2^24⌋; prefix > u · W ⇔ prefix > thr
  if (threadIdx.x == 0) { chosen = 0; chosen_p = 0.f; }
  __syncthreads();
  if (base <= thr && thr < base + part) {                  // exactly one thread: thr < W
    smp_u64 run = base;
    int id = -1;
    smp_u64 qid = 0;
#pragma unroll
    for (int j = 0; j < SMP_NPT; ++j)
      if (key[j] >= tau) {
        const smp_u64 q = smp_q(w[j]);
        run += q;
        if (id < 0 && run > thr) { id = i0 + j; qid = q; }
      }
    chosen = id;
    chosen_p = (float)((double)qid / (double)W);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s.n_kept) s.n_kept[g] = (int)nk;
    if (s.p_chosen) s.p_chosen[g] = chosen_p;
  }
  return chosen;
}

// the lock-step store: ld_out is the row stride of out_ids and doubles as the row capacity (<= 0: no bound — the G = 1 call)
__device__ __forceinline__ void lockstep_store(const TailP& p, int g, int result) {
  p.next[g] = result;
  if (p.out_ids) {
    const int st = p.step[g];
    if (st >= 0 && (p.ld_out <= 0 || st < p.ld_out)) p.out_ids[(size_t)g * p.ld_out + st] = result;
  }
}

// the slot advance of a live slot (thread 0): force_at, the id log, the counters, the stop rule, parking, the status row
// (ALSO: the FSM form's "or the grammar is done" joins the stop rule)
template <bool ALSO = false>
__device__ __forceinline__ void slot_advance(const TailP& p, int g, int result, [[maybe_unused]] bool also_stop = false) {
  int n = p.n_new[g];
  const int fa = p.force_at[g];
  if (fa >= 0 && n == fa) result = p.force_id;      // synthetic weights only: replaced AFTER the full arg-max / draw (no work skipped)
  const int st = p.step[g];
  if (p.out_ids && st >= 0 && st < p.ld_out) p.out_ids[(size_t)g * p.ld_out + st] = result;   // ld_out is the row capacity
  p.next[g] = result;
  n += 1;
  p.n_new[g] = n;
  bool stop = (p.eos_id >= 0 && result == p.eos_id) || n >= p.max_new[g];
  if constexpr (ALSO) stop = stop || also_stop;
  if (stop) {
    p.live[g] = 0;
    p.step[g] = -1;
    p.pos[g] = -1;
    p.ctx[g] = 0;
  } else {
    p.step[g] = st + 1;
    p.pos[g] += 1;
    p.ctx[g] += 1;
  }
  int* q = p.status + 4 * g;
  q[0] = result;
  q[1] = stop ? 0 : 1;
  q[2] = n;
  q[3] = stop ? n : -1;
}

struct NoSampleP {};

// ---- token log-probabilities: lp(v) = x[v] - logsumexp(x) of the RAW row, and the n_top largest (sx_token_logprobs, the LP tail) ------
// seedx_amd.sampling.token_logprobs states the rule in fp64. One workgroup of 1024 threads per row, fp32 throughout, in a layout that
// depends on nothing but vocab: thread t owns the columns t, t + 1024, t + 2048, ...
//   m      = the row maximum (exact), found together with its first index: that pair is also entry 0 of the top list;
//   S      = sum of expf(x - m): every thread adds its columns in ascending order (32 terms at vocab <= 32768), the 64 lanes of a wave
//            combine in a 6-step xor butterfly (both partners add the same two numbers, so every lane holds the same bits), the 16 wave
//            sums combine in a fixed 4-level pairwise tree: 42 additions deep at vocab <= 32768, 32 more per further 32768 columns;
//   lp(v)  = (x[v] - m) - logf(S);
//   top j  = the first maximal index among the columns after entry j - 1 in the order (value descending, index ascending). Every
//            thread keeps the best of its own columns; only the owner of a selected column looks for its next one.
// Reassociation is switched off for this function and it is never inlined: the standalone kernel and the LP tail run the same
// instructions, so the record's bits are a function of (row values, vocab) alone, whatever the slot, G, the launch or graph replay.
// NaN anywhere in the row (or +inf, or a row of -inf only) makes S NaN: the record is NaN with ids -1.
constexpr int LP_MAX_TOP = 8;
constexpr int LP_REG_COLS = 32;             // columns a thread keeps in registers: rows of up to 32768 columns
struct LpScratch {
  float rv[2][16];
  int ri[2][16];
  float ps[16];
  float topv[LP_MAX_TOP];
  int topi[LP_MAX_TOP];
  float m, log_s, raw;
};

__device__ __forceinline__ bool lp_before(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// After it returns (behind a barrier) every thread may read s->m, s->log_s and s->topv / s->topi [0, n_top): the raw values and indices
// of the n_top largest columns, index -1 and value -inf past the end of the row.
// (A template, like token_logprobs_kernel below, only for its place in the code object: templates are emitted where they are first used,
// behind the kernels the library already had, which keep their order and their offsets within .text — profiles/logprobs.md compares them.)
template <int UNUSED = 0>
__device__ __noinline__ void row_logprob_stats(const float* row, int vocab, int n_top, LpScratch* s) {
#pragma clang fp reassociate(off)
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  float pv = INFINITY, m = -INFINITY;       // the entry selected last; nothing yet
  int pi = -1;
  float bv = -INFINITY;                     // this thread's best column after (pv, pi); bi = INT_MAX: none left
  int bi = 0x7fffffff;
  bool scan = true;
  const int passes = n_top > 1 ? n_top : 1;
  // rows of up to 32768 columns are read from memory ONCE: the thread's columns stay in registers for every pass (same values, same
  // order of operations as the loops over memory that longer rows take)
  const bool reg = vocab <= LP_REG_COLS * 1024;
  const int cnt = vocab > t ? (vocab - t + 1023) >> 10 : 0;
  float loc[LP_REG_COLS];
  if (reg) {
#pragma unroll
    for (int j = 0; j < LP_REG_COLS; ++j) loc[j] = j < cnt ? row[t + 1024 * j] : 0.f;
  }
  for (int k = 0; k < passes; ++k) {
    if (scan) {
      bv = -INFINITY;
      bi = 0x7fffffff;
      auto consider = [&](float v, int i) {
        if ((k == 0 || lp_before(pv, pi, v, i)) && lp_before(v, i, bv, bi)) { bv = v; bi = i; }
      };
      if (reg) {
#pragma unroll
        for (int j = 0; j < LP_REG_COLS; ++j)
          if (j < cnt) consider(loc[j], t + 1024 * j);
      } else {
        for (int i = t; i < vocab; i += 1024) consider(row[i], i);
      }
    }
    float rv = bv;
    int ri = bi;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(rv, o, 64);
      const int oi = __shfl_xor(ri, o, 64);
      if (lp_before(ov, oi, rv, ri)) { rv = ov; ri = oi; }
    }
    if (lane == 0) { s->rv[k & 1][wv] = rv; s->ri[k & 1][wv] = ri; }
    __syncthreads();                        // (the buffers alternate: pass k + 2 writes this one again behind pass k + 1's barrier)
    rv = s->rv[k & 1][0];
    ri = s->ri[k & 1][0];
#pragma unroll
    for (int w = 1; w < 16; ++w)
      if (lp_before(s->rv[k & 1][w], s->ri[k & 1][w], rv, ri)) { rv = s->rv[k & 1][w]; ri = s->ri[k & 1][w]; }
    if (k == 0) m = rv;
    const bool none = ri == 0x7fffffff;
    if (t == 0 && k < n_top) { s->topv[k] = none ? -INFINITY : rv; s->topi[k] = none ? -1 : ri; }
    scan = !none && (ri & 1023) == t;       // the owner of the selected column finds its next one
    pv = rv;
    pi = ri;
  }
  float acc = 0.f;
  if (reg) {
#pragma unroll
    for (int j = 0; j < LP_REG_COLS; ++j)
      if (j < cnt) acc += expf(loc[j] - m);
  } else {
    for (int i = t; i < vocab; i += 1024) acc += expf(row[i] - m);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) s->ps[wv] = acc;
  __syncthreads();
  if (t == 0) {
    const float* q = s->ps;
    const float a0 = (q[0] + q[1]) + (q[2] + q[3]), a1 = (q[4] + q[5]) + (q[6] + q[7]);
    const float a2 = (q[8] + q[9]) + (q[10] + q[11]), a3 = (q[12] + q[13]) + (q[14] + q[15]);
    s->m = m;
    s->log_s = logf((a0 + a1) + (a2 + a3));
  }
  __syncthreads();
}

// One record: raw = x[id] of the raw row. Thread 0 stores the chosen value, threads [0, n_top) the top list. ``none``: the model did
// not choose (a row inside the image chain): NaN and ids -1, as for a row that holds NaN.
__device__ __forceinline__ void lp_store(const LpScratch* s, float raw, bool none, float* chosen, int* top_ids, float* top, int n_top) {
#pragma clang fp reassociate(off)
  const float ls = s->log_s, m = s->m;
  const bool bad = none || ls != ls;
  const int t = threadIdx.x;
  if (t == 0 && chosen) *chosen = bad ? NAN : (raw - m) - ls;
  if (t < n_top) {
    if (top_ids) top_ids[t] = bad ? -1 : s->topi[t];
    if (top) top[t] = bad ? NAN : (s->topv[t] - m) - ls;
  }
}

struct LogprobP {
  const int* want;
  float* chosen;
  int* top_ids;
  float* top;
  int n_top;
};
struct NoLogprobP {};

template <int UNUSED = 0>
__global__ __launch_bounds__(1024) void token_logprobs_kernel(const float* logits, int64_t ld, int vocab, const int* targets, float* chosen,
                                                              int* top_ids, float* top, int n_top) {
  __shared__ LpScratch scr;
  const int r = blockIdx.x;
  const float* row = logits + (size_t)r * ld;
  row_logprob_stats(row, vocab, n_top, &scr);
  const int id = targets[r];
  const bool in = id >= 0 && id < vocab;    // a target outside the row: NaN, nothing is read
  lp_store(&scr, in ? row[id] : NAN, false, chosen + r, top_ids ? top_ids + (size_t)r * n_top : nullptr,
           top ? top + (size_t)r * n_top : nullptr, n_top);
}

// SAMPLE: the id by the seeded rule (token index: token_index[g] in the lock-step form, step[g] in the in-flight form), else the
// greedy id; the greedy instantiation holds nothing of the sampler. LP: rows with want[g] != 0 also record the log-probability of the
// id they emit and the n_top largest of the row, at [g][step[g]] under out_ids' guard. The statistics are taken from the raw row BEFORE
// the rule zeroes its image columns, whose raw values the threads that zero them keep; nothing else of the tail changes.
// CTL: per-request logits controls (seedx_amd.sampling.apply_controls states the rule; include/seedx_hip.h sx_logits_ctl_args). A row
// with on[g] != 0 is NOT edited in place: its edited copy goes to work[g][0..ld), the image rule and the id functions run on that copy, and
// the logits row stays what lm_head wrote (so the LP record is of the RAW row, no fix-up). A row with on[g] == 0 and every parked slot take
// the path of the instantiations without CTL, the in-place zeroing included. After the emitted id is known thread 0 of a controlled row
// counts it.
struct CtlP {
  const int* on;
  int* counts;
  float* work;
  const float* rep;
  const float* rep_inv;
  const float* presence;
  const float* frequency;
  const int* min_new;
  const int* bias_ids;
  const float* bias;
  const int* token_index;
  int ld_counts, eos_id;
};
struct NoCtlP {};
constexpr int CTL_MAX_BIAS = 16;

// One IEEE fp32 operation each, as written: this file is built with -ffast-math, under which f * n + a contracts to v_fmac_f32 whatever
// the fp pragmas say; a single-instruction asm statement is opaque to that.
__device__ __forceinline__ float ctl_mul(float a, float b) {
  float d = 0.f;
#if defined(__HIP_DEVICE_COMPILE__)
  asm("v_mul_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
#endif
  return d;
}
__device__ __forceinline__ float ctl_add(float a, float b) {
  float d = 0.f;
#if defined(__HIP_DEVICE_COMPILE__)
  asm("v_add_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
#endif
  return d;
}
__device__ __forceinline__ float ctl_sub(float a, float b) {
  float d = 0.f;
#if defined(__HIP_DEVICE_COMPILE__)
  asm("v_sub_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
#endif
  return d;
}

// Steps 1-4 of the rule for row g: work[0..ld) = the edited row (columns >= vocab are copied). k: the token index. Ends behind a barrier.
__device__ __forceinline__ void ctl_edit_row(const float* row, float* work, const CtlP& c, int g, int vocab, int ld, int eos, int k) {
  const int* cnt = c.counts + (size_t)g * c.ld_counts;
  const float r = c.rep[g], rinv = c.rep_inv[g], a = c.presence[g], f = c.frequency[g];
  const bool rep_on = r != 1.0f;
  for (int i = threadIdx.x; i < ld; i += 1024) {
    float y = row[i];
    if (i < vocab) {
      const int w = cnt[i];
      const int n = w & 0xFFFFFF;
      if (rep_on && ((w & (1 << 30)) || n > 0)) y = y < 0.f ? ctl_mul(y, r) : ctl_mul(y, rinv);
      if (n > 0) y = ctl_sub(y, ctl_add(ctl_mul(f, (float)n), a));
    }
    work[i] = y;
  }
  __syncthreads();
  if (threadIdx.x == 0) {                           // entries in list order (an id named twice takes both), then the EOS mask
    for (int j = 0; j < CTL_MAX_BIAS; ++j) {
      const int id = c.bias_ids[(size_t)g * CTL_MAX_BIAS + j];
      if (id >= 0 && id < vocab) work[id] = ctl_add(work[id], c.bias[(size_t)g * CTL_MAX_BIAS + j]);
    }
    if (eos >= 0 && eos < vocab && k < c.min_new[g]) work[eos] = -INFINITY;
  }
  __syncthreads();
}

// FSM (on the CTL family only: the controls carry the working rows): constrained decoding by a token automaton (seedx_amd.grammar states
// the rule: constrain_row, advance; include/seedx_hip.h sx_token_fsm_args). Row g is constrained when 0 <= table[g] < n_tables and
// 0 <= state[g] < n_states. Such a row always gets a working row (a plain copy when on[g] == 0, the controlled row otherwise), in which
// every id its table row bans becomes -inf and EOS survives only in an accepting state; the image rule is skipped for it (n_img = 0 to
// the id functions: its zeroing would lift banned image columns to 0.0); the arg-max or the draw is the unchanged one; thread 0 advances
// the state on the id the row emits, and in the slot form a state that becomes DONE stops the slot. Every other row: the CTL path.
struct FsmP {
  const int* table;
  int* state;
  const short* trans;
  const int* flags;
  int n_tables, n_states, ld_v, eos_id;
};
struct CtlFsmP : CtlP {           // one kernel argument, so that the argument list of the older instantiations stays what it was
  FsmP f;
};
constexpr int FSM_DONE = -2;

// work[0..ld) = src[0..ld) with the banned columns -inf (src may be work). trow: the state's table row, int16 [ld_v >= vocab], ld_v even
// and the row 4-byte aligned: one dword holds the next states of two neighbouring ids. Ends behind a barrier.
__device__ __forceinline__ void fsm_mask_row(const float* src, float* work, const short* trow, bool accepting, int vocab, int ld, int eos) {
  for (int i = 2 * (int)threadIdx.x; i < ld; i += 2048) {
    const unsigned pair = i < vocab ? *reinterpret_cast<const unsigned*>(trow + i) : 0u;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int col = i + e;
      if (col < ld) {
        float y = src[col];
        if (col < vocab) {
          const bool ban = col == eos ? !accepting : (short)(pair >> (16 * e)) < 0;
          if (ban) y = -INFINITY;
        }
        work[col] = y;
      }
    }
  }
  __syncthreads();
}

// SEQ (on the CTL family only): per-request sequence rules that need the ORDER of the ids a request has seen (seedx_amd.sampling states
// them: ngram_banned / apply_no_repeat / stop_match; include/seedx_hip.h sx_seq_rule_args). hist[g][0 .. hist_len[g]) is the request's
// prompt followed by every id it emitted. A row with on[g] != 0 and ngram[g] = n > 0 gets a working row (the controlled one, or a plain
// copy) in which every id that would complete an n-gram already in the history is -inf, ahead of the grammar mask and the image rule;
// thread 0 appends the id the row emits and tests the stop sequences against the tail of the generated part; in the slot form a match
// stops the slot. A row with on[g] == 0 and every parked slot: the CTL / FSM path, history and matched untouched.
struct SeqP {
  const int* on;
  const int* ngram;
  int* hist;
  int* hist_len;
  const int* prompt_len;
  const int* n_stop;
  const int* stop_len;
  const int* stop_ids;
  int* matched;
  int ld_hist;
};
struct CtlSeqP : CtlP {
  SeqP q;
};
struct CtlFsmSeqP : CtlFsmP {
  SeqP q;
};
constexpr int SEQ_MAX_NGRAM = 8, SEQ_MAX_STOP = 4, SEQ_MAX_STOP_LEN = 8;

// work[0..ld) = src[0..ld) (src may be work) with the columns banned by the history -inf. The tail hist[L-n+1 .. L) is staged once in
// LDS; thread t takes the start positions t, t + 1024, ... of [0, L - n]: neighbouring threads read neighbouring ids. Several threads may
// ban the same column: they store the same value. Ends behind a barrier.
__device__ __forceinline__ void seq_ban_row(const float* src, float* work, const int* hist, int L, int n, int vocab, int ld) {
  __shared__ int tail[SEQ_MAX_NGRAM];
  if (src != work)
    for (int i = threadIdx.x; i < ld; i += 1024) work[i] = src[i];
  if ((int)threadIdx.x < n - 1 && L - n + 1 >= 0) tail[threadIdx.x] = hist[L - n + 1 + threadIdx.x];
  __syncthreads();
  for (int i = threadIdx.x; i <= L - n; i += 1024) {
    bool same = true;
    for (int j = 0; j < n - 1; ++j) same = same && hist[i + j] == tail[j];
    if (same) {
      const int id = hist[i + n - 1];
      if (id >= 0 && id < vocab) work[id] = -INFINITY;
    }
  }
  __syncthreads();
}

// thread 0, once the id the row emits is known: append it (bounded by ld_hist: a full history takes nothing more and matches nothing),
// then the lowest stop sequence the generated ids end with, or -1
__device__ __forceinline__ bool seq_append_match(const SeqP& q, int g, int id) {
  int* hist = q.hist + (size_t)g * q.ld_hist;
  int L = q.hist_len[g];
  int m = -1;
  if (L >= 0 && L < q.ld_hist) {
    hist[L] = id;
    L += 1;
    q.hist_len[g] = L;
    int pl = q.prompt_len[g];
    pl = pl < 0 ? 0 : pl;
    const int gen = L - pl;
    int ns = q.n_stop[g];
    ns = ns < 0 ? 0 : ns > SEQ_MAX_STOP ? SEQ_MAX_STOP : ns;
    for (int j = 0; j < ns && m < 0; ++j) {
      int sl = q.stop_len[(size_t)g * SEQ_MAX_STOP + j];
      sl = sl < 1 ? 1 : sl > SEQ_MAX_STOP_LEN ? SEQ_MAX_STOP_LEN : sl;
      if (sl > gen) continue;
      const int* sid = q.stop_ids + ((size_t)g * SEQ_MAX_STOP + j) * SEQ_MAX_STOP_LEN;
      bool same = true;
      for (int k = 0; k < sl; ++k) same = same && hist[L - sl + k] == sid[k];
      if (same) m = j;
    }
  }
  q.matched[g] = m;
  return m >= 0;
}

template <bool SAMPLE, bool LP = false, bool CTL = false, bool FSM = false, bool SEQ = false>
__global__ __launch_bounds__(1024) void next_token_kernel(const TailP p, const std::conditional_t<SAMPLE, SampleP, NoSampleP> s,
                                                          const std::conditional_t<LP, LogprobP, NoLogprobP> lp,
                                                          const std::conditional_t<SEQ, std::conditional_t<FSM, CtlFsmSeqP, CtlSeqP>,
                                                                                   std::conditional_t<FSM, CtlFsmP, std::conditional_t<CTL, CtlP, NoCtlP>>> c) {
  static_assert(CTL || !FSM, "the FSM form lives on the CTL family: the controls carry the working rows");
  static_assert(CTL || !SEQ, "the SEQ form lives on the CTL family too");
  const int g = blockIdx.x;
  const bool slots = p.live != nullptr;
  if (slots && p.live[g] == 0) return;              // parked (uniform over the workgroup: no barrier is skipped by a part of it)
  float* row = p.logits + (size_t)g * p.ld_logits;
  [[maybe_unused]] float* raw_row = row;            // CTL: what the LP record reads; `row` becomes the working row of a controlled row
  [[maybe_unused]] bool ctl_on = false;
  if constexpr (CTL) {
    ctl_on = c.on[g] != 0;                          // (uniform over the workgroup)
    if (ctl_on) {
      // everything thread 0 rewrites after the id is known is read here, ahead of the barriers
      const int k = slots ? p.step[g] : c.token_index[g];
      float* work = c.work + (size_t)g * p.ld_logits;
      ctl_edit_row(row, work, c, g, p.vocab, p.ld_logits, slots ? p.eos_id : c.eos_id, k);
      row = work;
    }
  }
  [[maybe_unused]] bool seq_on = false;
  if constexpr (SEQ) {
    seq_on = c.q.on[g] != 0;                        // (uniform over the workgroup)
    if (seq_on) {
      int n = c.q.ngram[g], L = c.q.hist_len[g];    // (hist and hist_len are rewritten by thread 0 behind the id functions' barriers)
      n = n < 0 ? 0 : n > SEQ_MAX_NGRAM ? SEQ_MAX_NGRAM : n;
      L = L < 0 ? 0 : L > c.q.ld_hist ? c.q.ld_hist : L;
      if (n > 0) {
        float* work = c.work + (size_t)g * p.ld_logits;
        seq_ban_row(row, work, c.q.hist + (size_t)g * c.q.ld_hist, L, n, p.vocab, p.ld_logits);
        row = work;
      }
    }
  }
  [[maybe_unused]] bool fsm_on = false;
  [[maybe_unused]] const short* trow = nullptr;
  [[maybe_unused]] const int* frow = nullptr;
  if constexpr (FSM) {
    const int tab = c.f.table[g], st = c.f.state[g];    // (uniform; state[g] is rewritten by thread 0 behind the id functions' barriers)
    fsm_on = tab >= 0 && tab < c.f.n_tables && st >= 0 && st < c.f.n_states;
    if (fsm_on) {
      frow = c.f.flags + (size_t)tab * c.f.n_states;
      trow = c.f.trans + ((size_t)tab * c.f.n_states + st) * c.f.ld_v;
      float* work = c.work + (size_t)g * p.ld_logits;
      fsm_mask_row(row, work, trow, (frow[st] & 1) != 0, p.vocab, p.ld_logits, slots ? p.eos_id : c.f.eos_id);
      row = work;
    }
  }
  [[maybe_unused]] bool rec = false;
  [[maybe_unused]] float raw_img = 0.f;
  [[maybe_unused]] int lp_prev = 0, lp_step = 0, lp_forced = -1;
  [[maybe_unused]] LpScratch* scr = nullptr;
  if constexpr (LP) {
    __shared__ LpScratch lp_scr;
    scr = &lp_scr;
    rec = lp.want[g] != 0;                          // (uniform over the workgroup)
    if (rec) {
      // everything thread 0 rewrites after the id is known, read by every thread before the barriers of the statistics
      lp_prev = p.prev[g];
      lp_step = p.step[g];
      if (slots && p.force_at[g] >= 0 && p.n_new[g] == p.force_at[g]) lp_forced = p.force_id;
      row_logprob_stats(raw_row, p.vocab, lp.n_top, scr);
      if ((int)threadIdx.x < p.n_img - 1) raw_img = raw_row[p.img_ids[1 + threadIdx.x]];
    }
  }
  // every thread reads prev[g] and the token index before the first barrier of the id functions; thread 0 stores to next[g] (which
  // may be prev[g]) and step[g] after the last one
  int result;
  if constexpr (FSM) {
    const int n_img = fsm_on ? 0 : p.n_img;             // a constrained row: no chain, no zeroing
    if constexpr (SAMPLE)
      result = sample_next_id(row, p.vocab, p.img_ids, n_img, p.prev[g], s, g, slots ? p.step[g] : s.token_index[g]);
    else
      result = greedy_next_id(row, p.vocab, p.img_ids, n_img, p.prev[g]);
  } else if constexpr (SAMPLE)
    result = sample_next_id(row, p.vocab, p.img_ids, p.n_img, p.prev[g], s, g, slots ? p.step[g] : s.token_index[g]);
  else
    result = greedy_next_id(row, p.vocab, p.img_ids, p.n_img, p.prev[g]);
  if constexpr (LP) {
    if (rec) {
      const int id = lp_forced >= 0 ? lp_forced : result;        // the id slot_advance emits
      if (threadIdx.x == 0) scr->raw = id >= 0 && id < p.vocab ? raw_row[id] : NAN;
      __syncthreads();
      if ((int)threadIdx.x < p.n_img - 1 && p.img_ids[1 + threadIdx.x] == id) scr->raw = raw_img;   // a zeroed column (ids are unique)
      const bool chain = __syncthreads_or((int)threadIdx.x < p.n_img - 1 && p.img_ids[threadIdx.x] == lp_prev);
      if (lp_step >= 0 && lp_step < p.ld_out) {
        const size_t at = (size_t)g * p.ld_out + lp_step;
        lp_store(scr, scr->raw, chain, lp.chosen + at, lp.top_ids ? lp.top_ids + at * lp.n_top : nullptr,
                 lp.top ? lp.top + at * lp.n_top : nullptr, lp.n_top);
      }
    }
  }
  if (threadIdx.x != 0) return;
  if constexpr (CTL) {
    if (ctl_on) {                                   // the id the row EMITS: in the slot form the one behind the force_at replacement
      int id = result;
      if (slots && p.force_at[g] >= 0 && p.n_new[g] == p.force_at[g]) id = p.force_id;
      if (id >= 0 && id < p.vocab) c.counts[(size_t)g * c.ld_counts + id] += 1;
    }
  }
  [[maybe_unused]] bool fsm_stop = false;
  if constexpr (FSM) {
    if (fsm_on) {                                   // advance on the id the row EMITS; DONE: EOS, an inadmissible id, or a final state
      int id = result;
      if (slots && p.force_at[g] >= 0 && p.n_new[g] == p.force_at[g]) id = p.force_id;
      const int eos = slots ? p.eos_id : c.f.eos_id;
      int ns = FSM_DONE;
      if (!(eos >= 0 && id == eos) && id >= 0 && id < p.vocab) {
        const int t = trow[id];
        if (t >= 0 && t < c.f.n_states && !(frow[t] & 2)) ns = t;
      }
      c.f.state[g] = ns;
      fsm_stop = ns < 0;
    }
  }
  if constexpr (SEQ) {
    bool seq_stop = false;
    if (seq_on) {                                   // the id the row EMITS goes to the history, then the stop sequences
      int id = result;
      if (slots && p.force_at[g] >= 0 && p.n_new[g] == p.force_at[g]) id = p.force_id;
      seq_stop = seq_append_match(c.q, g, id);
    }
    if (slots) slot_advance<true>(p, g, result, fsm_stop || seq_stop);
    else lockstep_store(p, g, result);
  } else if constexpr (FSM) {
    if (slots) slot_advance<true>(p, g, result, fsm_stop);
    else lockstep_store(p, g, result);
  } else {
    if (slots) slot_advance(p, g, result);
    else lockstep_store(p, g, result);
  }
}

inline dim3 gs_grid(int64_t n) {
  int64_t b = (n + 255) / 256;
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return dim3((unsigned)b);
}

}  // namespace sxk_decode
using namespace sxk_decode;

#define ST ((hipStream_t)stream)
static int g_skinny_var[4] = {0, 0, 0, 1};   // [3] = 64-row workgroups (R = 4): 0 never, 1 where >= 200 workgroups remain (round 6), 2 wherever legal  // tuning hook (sx_gemv_tune): [2] = split-K factor (0 auto, -1 never, 2 / 4 / 8 forced)
extern "C" int sx_gemv_tune(int key, int value) {
  SX_CHECK((key == 2 && (value == -1 || value == 0 || value == 1 || value == 2 || value == 4 || value == 8)) || (key == 1 && (value == 0 || value == 1 || value == 2)) ||
               (key == 3 && value >= 0 && value <= 2),
           "sx_gemv_tune: key %d value %d", key, value);
  g_skinny_var[key] = value;
  return SX_OK;
}
static int g_force_valu_gemv = 0;   // test hook (sx_gemv_force_valu): compare the two GEMV paths
extern "C" int sx_gemv_force_valu(int on) { g_force_valu_gemv = on; return SX_OK; }   // 1 = VALU only, 2 = MFMA whenever legal

// Row groups of the MFMA path without 64-row workgroups, as always next to x16_out (row_ssq_out has one column per workgroup:
// sx_gemv_ssq_parts): 20-row tiles, else R = 2 row groups per wave for GLU (one packed group) or when that still gives >= 256 blocks
struct SkinnyRows { bool tail20, r2; int gx; };
static SkinnyRows skinny_rows(int N, int glu, int w_layout) {
  const bool tail20 = w_layout == 2;
  const bool r2 = !tail20 && (glu || N / 32 >= 256);
  return {tail20, r2, tail20 ? N / 20 : (r2 ? N / 32 : N / 16)};
}
extern "C" int sx_gemv_ssq_parts(int N, int glu, int w_layout) { return skinny_rows(N, glu, w_layout).gx; }

// The launch of one sx_gemv call, whatever the weight format: path, grid (gx, S) and kernel — the (R, U, TAIL, MB) family of
// gemm_skinny_kernel, or gemv_kernel with MR = R and U = TAIL = MB = 0 on the VALU path. sx_gemv_plan reports these fields.
struct SkinnyPlan { int mfma, gx, S, R, U, TAIL, MB, ws_part_off; };   // ws_part_off: 0 = no split-K workspace, else where its partial sums begin
static SkinnyPlan skinny_plan(const sx_gemv_args* a, bool planes2, bool mfma_ok) {
  SkinnyPlan pl = {0, 0, 1};
  // the decode-tile layout only exists for the MFMA kernel: it overrides the VALU test hook
  pl.mfma = mfma_ok && (a->w_layout || a->x_layout || (a->out_dtype & SX_TILED16) || (g_force_valu_gemv != 1 && (a->M >= 5 || g_force_valu_gemv == 2)));
  if (!pl.mfma) {
    pl.gx = ((a->N + 1) / 2 + 3) / 4;     // a wave per pair of rows, four waves per workgroup
    pl.R = a->M == 1 ? 1 : (a->M == 2 ? 2 : (a->M <= 4 ? 4 : 8));
    return pl;
  }
  const SkinnyRows rows = skinny_rows(a->N, a->glu, a->w_layout);
  // 64-row workgroups (R = 4, one k-step per round): every workgroup re-reads the whole x operand from L2 (64 B x K per 16-row block) —
  // with two planes that traffic is as large as the weight stream itself and its time ADDS to it (tools/bench_skinny_shapes.py:
  // qkv 26 / 32 / 43 us with 1 / 2 / 4 x blocks). Twice the rows per workgroup halve it; only where enough workgroups remain to fill
  // the chip (qkv at 13B: 240, measured faster than 480 32-row ones), and not together with the RMSNorm-fold producer outputs (20-row
  // tiles anyway)
  const bool r4 = rows.r2 && g_skinny_var[3] > 0 && a->N % 64 == 0 && !a->x16_out && (a->N / 64 >= (g_skinny_var[3] == 2 ? 64 : 200));
  pl.gx = r4 ? a->N / 64 : rows.gx;
  // x blocks per weight fragment: 17..32 rows are two, fp32-grade rows (two planes) twice as many
  pl.MB = (a->M > 16 ? 2 : 1) * (planes2 ? 2 : 1);
  // split-K over workgroups when the row groups alone do not fill the chip (N = 5120: 320 workgroups on 256 CUs, the CUs
  // with two of them set the time) AND the kernel is long enough to pay for the second pass (publish, count, re-read: ~4 us
  // at the kernel's tail): tools/lab/gemv_lab — down 5120x13824 36.8 -> 33.0 us with S = 4, o 5120x5120 15.4 -> 17.6 (never)
  if (a->workspace && !(rows.tail20 && g_skinny_var[2] <= 0)) {      // 256 balanced 20-row groups: no split unless forced (lab)
    if (g_skinny_var[2] > 0) pl.S = g_skinny_var[2];
    else if (g_skinny_var[2] == 0 && a->K >= 8192) while (pl.S < 8 && pl.gx * pl.S < 1024 && (a->K / 64) / (2 * pl.S * 4) >= 4) pl.S *= 2;
    const uint64_t cnt_bytes = 16384;    // fixed, so launches of different N can share one workspace (their partial regions
                                         // may overlap — launches are serial — but never reach the counters)
    if (pl.S > 1 && (pl.gx > 4096 || cnt_bytes + (uint64_t)pl.S * 16 * pl.MB * a->N * 4 > a->workspace_bytes)) pl.S = 1;   // too small: no split
    pl.ws_part_off = (int)cnt_bytes;
  }
  // the family: rows per wave, then k-steps per round by what the x blocks leave of the register file
  pl.R = r4 ? 4 : (rows.tail20 || rows.r2 ? 2 : 1);
  pl.TAIL = rows.tail20;
  if (pl.MB == 4) pl.U = pl.R == 1 ? 2 : 1;
  else if (r4) pl.U = pl.MB == 2 ? 1 : 2;
  else if (pl.MB == 1) pl.U = 4;
  else if (g_skinny_var[1] == 1) pl.U = 4;       // lab: 4 k-steps per round (256 VGPRs + AGPR copies, one wave per SIMD)
  else if (rows.tail20) pl.U = g_skinny_var[1] == 2 ? 4 : 2;
  else pl.U = rows.r2 ? 2 : 4;
  return pl;
}

// every gemm_skinny_kernel the library holds: one row per (R, U, TAIL, MB) family, its kernels by [F16, BF16][16-bit, FP8, MXFP4 weights]
typedef void (*SkinnyKernel)(const GemvP);
struct SkinnyRow { int R, U, TAIL, MB; SkinnyKernel k[2][3]; };
#define SX_SK_ROW(R, U, TAIL, MB)                                                                                                        \
  {R, U, TAIL, MB, {{gemm_skinny_kernel<F16, R, 4, U, TAIL, MB, false, false>, gemm_skinny_kernel<F16, R, 4, U, TAIL, MB, true, false>,   \
                     gemm_skinny_kernel<F16, R, 4, U, TAIL, MB, false, true>},                                                         \
                    {gemm_skinny_kernel<BF16, R, 4, U, TAIL, MB, false, false>, gemm_skinny_kernel<BF16, R, 4, U, TAIL, MB, true, false>, \
                     gemm_skinny_kernel<BF16, R, 4, U, TAIL, MB, false, true>}}}
static const SkinnyRow g_skinny_table[] = {
    SX_SK_ROW(1, 4, false, 1), SX_SK_ROW(2, 4, false, 1), SX_SK_ROW(2, 4, true, 1), SX_SK_ROW(4, 2, false, 1),
    SX_SK_ROW(1, 4, false, 2), SX_SK_ROW(2, 2, false, 2), SX_SK_ROW(2, 2, true, 2), SX_SK_ROW(2, 4, false, 2), SX_SK_ROW(2, 4, true, 2),
    SX_SK_ROW(4, 1, false, 2),
    SX_SK_ROW(1, 2, false, 4), SX_SK_ROW(2, 1, false, 4), SX_SK_ROW(2, 1, true, 4), SX_SK_ROW(4, 1, false, 4),
};
#undef SX_SK_ROW
// every gemv_kernel (the VALU path): [F16, BF16][MR = 1, 2, 4, 8]
static const SkinnyKernel g_gemv_table[2][4] = {{gemv_kernel<F16, 1>, gemv_kernel<F16, 2>, gemv_kernel<F16, 4>, gemv_kernel<F16, 8>},
                                                {gemv_kernel<BF16, 1>, gemv_kernel<BF16, 2>, gemv_kernel<BF16, 4>, gemv_kernel<BF16, 8>}};

static int gemv_entry(const sx_gemv_args* a, void* stream, int32_t* plan) {
  SX_CHECK(a && a->x && a->W && a->y, "sx_gemv: null pointer");
  SX_CHECK(a->dtype == SX_F16 || a->dtype == SX_BF16, "sx_gemv: dtype");
  SX_CHECK(a->M >= 1 && a->M <= 32, "sx_gemv: M=%d must be 1..32", a->M);
  SX_CHECK(a->K % 8 == 0 && a->N > 0, "sx_gemv: K %% 8");
  SX_CHECK(!a->glu || a->N % 32 == 0, "sx_gemv: glu needs N %% 32 == 0");
  GemvP p;
  p.x = (const unsigned short*)a->x; p.W = (const unsigned short*)a->W; p.y = a->y; p.residual = a->residual;
  p.M = a->M; p.N = a->N; p.K = a->K; p.out_dtype = a->out_dtype & 0xff; p.act = a->act; p.glu = a->glu;
  p.y_tiled = (a->out_dtype & SX_TILED16) ? 1 : 0;
  SX_CHECK(!p.y_tiled || ((p.out_dtype == SX_F16 || p.out_dtype == SX_BF16) && (a->glu ? a->N / 2 : a->N) % 32 == 0),
           "sx_gemv: SX_TILED16 needs a 16-bit output with n_out %% 32 == 0");
  p.packed = a->w_layout == 1 ? 1 : 0;
  p.ws_cnt = nullptr; p.ws_part = nullptr;
  p.x16_out = (unsigned short*)a->x16_out; p.ssq_out = a->row_ssq_out; p.ssq_in = a->row_ssq_in;
  p.ssq_parts = a->ssq_in_parts; p.ssq_inv_dim = a->ssq_dim > 0 ? 1.0f / (float)a->ssq_dim : 0.f; p.ssq_eps = a->ssq_eps;
  SX_CHECK(!a->row_ssq_in || (a->ssq_in_parts > 0 && a->ssq_in_parts % 64 == 0 && a->ssq_dim > 0 && ((uintptr_t)a->row_ssq_in & 15) == 0),
           "sx_gemv: row_ssq_in needs ssq_in_parts (a multiple of 64), ssq_dim and a 16-B aligned list");
  SX_CHECK((a->x16_out == nullptr) == (a->row_ssq_out == nullptr), "sx_gemv: x16_out and row_ssq_out come together");
  SX_CHECK(!a->x16_out || (p.out_dtype == SX_F32 && !a->glu && a->N % 32 == 0 && !p.y_tiled),
           "sx_gemv: x16_out needs an fp32, non-GLU output with N %% 32 == 0");
  p.x_tiled = a->x_layout;
  SX_CHECK(a->x_layout == 0 || a->x_layout == 1, "sx_gemv: x_layout must be 0 (row-major) or 1 (operand tiles)");
  SX_CHECK(a->x_planes >= 0 && a->x_planes <= 2, "sx_gemv: x_planes=%d", a->x_planes);
  const bool planes2 = a->x_planes == 2;
  p.planes2 = planes2 ? 1 : 0;
  SX_CHECK(!planes2 || a->x_layout == 1, "sx_gemv: x_planes = 2 needs tiled x ([2 planes][row blocks][K/32][16][32])");
  p.out_planes = a->out_planes ? 1 : 0;
  p.x16_gamma = a->x16_gamma;
  SX_CHECK(!p.out_planes || p.y_tiled || a->x16_out, "sx_gemv: out_planes needs a tiled 16-bit output (SX_TILED16 or x16_out)");
  SX_CHECK(!a->x16_gamma || (a->x16_out && (((uintptr_t)a->x16_gamma) & 15) == 0), "sx_gemv: x16_gamma belongs to x16_out (16-B aligned fp32 [N])");
  SX_CHECK(a->w_layout >= 0 && a->w_layout <= 2, "sx_gemv: w_layout must be 0 (row-major), 1 (decode tiles) or 2 (20-row decode tiles)");
  SX_CHECK(a->w_layout != 2 || (!a->glu && a->N % 20 == 0 && a->N % 32 == 0), "sx_gemv: w_layout 2 needs N %% 20 == 0, N %% 32 == 0, no GLU");
  // MI355X (tools/bench_gemv.py, 13B shapes): VALU path 6.5 / 4.7 / 3.0 TB/s at M = 1 / 4 / 8, MFMA path 4.0-4.4 TB/s at any M
  const bool mfma_ok = (a->M >= 2 || planes2) && a->K % 64 == 0 && a->K >= 256 && a->N % 32 == 0;
  // FP8 weight tiles: codes + fp32 row scales, tiled layouts and the MFMA kernel only (the VALU kernel has no FP8 form)
  SX_CHECK(a->w_dtype == 0 || a->w_dtype == SX_FP8_E4M3 || a->w_dtype == SX_FP4_E2M1,
           "sx_gemv: w_dtype must be 0 (the activation dtype), SX_FP8_E4M3 or SX_FP4_E2M1");
  const bool w8 = a->w_dtype == SX_FP8_E4M3;
  SX_CHECK(!w8 || ((a->w_layout == 1 || a->w_layout == 2) && mfma_ok),
           "sx_gemv: SX_FP8_E4M3 weights need w_layout 1 or 2 and the MFMA path (M >= 2, K %% 64 == 0, K >= 256, N %% 32 == 0)");
  SX_CHECK(!w8 || (a->w_scale && ((uintptr_t)a->w_scale & 15) == 0), "sx_gemv: SX_FP8_E4M3 weights need w_scale (16-B aligned fp32 [N])");
  SX_CHECK(w8 || !a->w_scale, "sx_gemv: w_scale belongs to SX_FP8_E4M3 weights");
  p.w_scale = a->w_scale;
  // MXFP4 weight tiles: codes + E8M0 block scales, tiled layouts and the MFMA kernel only, no row scale
  const bool w4 = a->w_dtype == SX_FP4_E2M1;
  SX_CHECK(!w4 || ((a->w_layout == 1 || a->w_layout == 2) && mfma_ok),
           "sx_gemv: SX_FP4_E2M1 weights need w_layout 1 or 2 and the MFMA path (M >= 2, K %% 64 == 0, K >= 256, N %% 32 == 0)");
  SX_CHECK(!w4 || (a->w_block_scale && ((uintptr_t)a->w_block_scale & 15) == 0),
           "sx_gemv: SX_FP4_E2M1 weights need w_block_scale (16-B aligned E8M0 bytes)");
  SX_CHECK(w4 || !a->w_block_scale, "sx_gemv: w_block_scale belongs to SX_FP4_E2M1 weights");
  p.w_bscale = (const unsigned char*)a->w_block_scale;
  // pre-activation addend (the LoRA delta of csrc/lora.hip): MFMA path only
  SX_CHECK(a->addend || !a->addend_sel, "sx_gemv: addend_sel belongs to addend");
  SX_CHECK(!a->addend || (((uintptr_t)a->addend & 15) == 0 && (a->addend_sel ? a->addend_n >= 1 : a->addend_n == 0)),
           "sx_gemv: addend must be 16-B aligned fp32 [M][N]; addend_sel comes with addend_n >= 1 (rows with addend_sel[m] in [0, addend_n) take it)");
  p.addend = a->addend; p.addend_sel = a->addend_sel; p.addend_n = a->addend_n;
  SX_CHECK(!a->w_layout || (mfma_ok && a->K % 64 == 0), "sx_gemv: the decode-tile layout needs M >= 2, K %% 64 == 0, K >= 256, N %% 32 == 0");
  SX_CHECK(!p.y_tiled || mfma_ok, "sx_gemv: a tiled output needs the MFMA path (M >= 2, K %% 64 == 0, K >= 256, N %% 32 == 0)");
  SX_CHECK(!a->x_layout || mfma_ok, "sx_gemv: tiled x needs the MFMA path (M >= 2, K %% 64 == 0, K >= 256, N %% 32 == 0)");
  const SkinnyPlan pl = skinny_plan(a, planes2, mfma_ok);
  if (!pl.mfma) {
    SX_CHECK(a->M <= 8, "sx_gemv: M=%d > 8 needs K %% 64 == 0 and N %% 32 == 0 (MFMA path)", a->M);
    SX_CHECK(p.packed == 0, "sx_gemv: the VALU kernel reads row-major weights only");
    SX_CHECK(!a->x16_out && !a->row_ssq_in, "sx_gemv: the RMSNorm fold exists on the MFMA path only");
    SX_CHECK(!a->addend, "sx_gemv: the pre-activation addend exists on the MFMA path only");
  }
  if (plan) {
    const int32_t out[8] = {pl.mfma, pl.gx, pl.S, pl.R, pl.U, pl.TAIL, pl.MB, a->w_dtype};
    for (int i = 0; i < 8; ++i) plan[i] = out[i];
    return SX_OK;
  }
  SkinnyKernel kernel = nullptr;
  if (pl.mfma) {
    if (pl.ws_part_off) {
      p.ws_cnt = (unsigned*)a->workspace;
      p.ws_part = (float*)((char*)a->workspace + pl.ws_part_off);
    }
    for (const SkinnyRow& row : g_skinny_table)
      if (row.R == pl.R && row.U == pl.U && row.TAIL == pl.TAIL && row.MB == pl.MB) kernel = row.k[a->dtype == SX_BF16][w4 ? 2 : (w8 ? 1 : 0)];
  } else {
    for (int i = 0; i < 4; ++i)
      if (pl.R == 1 << i) kernel = g_gemv_table[a->dtype == SX_BF16][i];
  }
  SX_CHECK(kernel, "sx_gemv: no kernel for path %d, (R, U, TAIL, MB) = (%d, %d, %d, %d)", pl.mfma, pl.R, pl.U, pl.TAIL, pl.MB);
  hipLaunchKernelGGL(kernel, dim3(pl.gx, pl.S), dim3(256), 0, ST, p);
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}

extern "C" int sx_gemv(const sx_gemv_args* a, void* stream) { return gemv_entry(a, stream, nullptr); }
extern "C" int sx_gemv_plan(const sx_gemv_args* a, int32_t* plan) {
  SX_CHECK(plan, "sx_gemv_plan: null pointer");
  return gemv_entry(a, nullptr, plan);
}

extern "C" int sx_attn_decode_b(const void* q, const void* kcache, const void* vcache, void* out, float* scratch,
                                const int32_t* ctx_len_dev, int G, int H, int D, int Tmax, int64_t cache_seq_stride,
                                int nsplit, float scale, int dtype, int64_t q_seq_stride, void* stream) {
  SX_CHECK(q && kcache && vcache && out && scratch && ctx_len_dev, "sx_attn_decode: null pointer");
  SX_CHECK(q_seq_stride == 0 || (q_seq_stride >= (int64_t)H * D && q_seq_stride % 8 == 0), "sx_attn_decode: q_seq_stride");
  SX_CHECK(D % 8 == 0 && D <= 128, "sx_attn_decode: head_dim %d", D);
  SX_CHECK(nsplit >= 1 && nsplit <= 64 && G >= 1, "sx_attn_decode: nsplit/G");
  const int tiled = (dtype & SX_TILED16) ? 1 : 0;   // the OUTPUT as operand tiles [H*D/32][16][32] (q and the caches are as always)
  dtype &= 0xff;
  SX_CHECK(!tiled || (G <= 32 && (H * D) % 32 == 0), "sx_attn_decode: SX_TILED16 needs G <= 32 and H*D %% 32 == 0");
  if (dtype == SX_BF16) {
    hipLaunchKernelGGL(attn_decode_kernel<BF16>, dim3(H, nsplit, G), dim3(256), 0, ST, (const unsigned short*)q,
                       (const unsigned short*)kcache, (const unsigned short*)vcache, scratch, ctx_len_dev, D, Tmax,
                       nsplit, scale, (long long)cache_seq_stride, (long long)(q_seq_stride ? q_seq_stride : (int64_t)H * D));
    hipLaunchKernelGGL(attn_decode_combine_kernel<BF16>, dim3(H, G), dim3(128), 0, ST, scratch, (unsigned short*)out, D,
                       nsplit, tiled);
  } else {
    hipLaunchKernelGGL(attn_decode_kernel<F16>, dim3(H, nsplit, G), dim3(256), 0, ST, (const unsigned short*)q,
                       (const unsigned short*)kcache, (const unsigned short*)vcache, scratch, ctx_len_dev, D, Tmax,
                       nsplit, scale, (long long)cache_seq_stride, (long long)(q_seq_stride ? q_seq_stride : (int64_t)H * D));
    hipLaunchKernelGGL(attn_decode_combine_kernel<F16>, dim3(H, G), dim3(128), 0, ST, scratch, (unsigned short*)out, D,
                       nsplit, tiled);
  }
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}
extern "C" int sx_attn_decode_fused(const sx_attn_decode_args* a, void* stream) {
  SX_CHECK(a && a->qkv && a->kcache && a->vcache && a->out && a->scratch && a->counters && a->cos_tab && a->sin_tab && a->pos_dev,
           "sx_attn_decode_fused: null pointer");
  const int tiled = (a->dtype & SX_TILED16) ? 1 : 0, dt = a->dtype & 0xff;
  SX_CHECK(dt == SX_F16 || dt == SX_BF16, "sx_attn_decode_fused: dtype");
  SX_CHECK(a->D % 16 == 0 && a->D <= 128, "sx_attn_decode_fused: head_dim %d (must be a multiple of 16, <= 128)", a->D);
  SX_CHECK(a->nsplit >= 1 && a->nsplit <= 64 && a->G >= 1 && a->H >= 1, "sx_attn_decode_fused: nsplit/G/H");
  SX_CHECK(!tiled || (a->G <= 32 && (a->H * a->D) % 32 == 0), "sx_attn_decode_fused: SX_TILED16 needs G <= 32 and H*D %% 32 == 0");
  AttnDecP p;
  p.qkv = (const unsigned short*)a->qkv; p.kc = (unsigned short*)a->kcache; p.vc = (unsigned short*)a->vcache;
  p.out = (unsigned short*)a->out; p.scratch = a->scratch; p.counters = (unsigned*)a->counters;
  p.cos_t = a->cos_tab; p.sin_t = a->sin_tab; p.pos_dev = a->pos_dev;
  p.H = a->H; p.D = a->D; p.Tmax = a->Tmax; p.nsplit = a->nsplit; p.tiled = tiled; p.scale = a->scale;
  p.seq_stride = a->cache_seq_stride;
  const dim3 grid(a->H, a->nsplit, a->G);
  if (dt == SX_BF16) hipLaunchKernelGGL(attn_decode_fused_kernel<BF16>, grid, dim3(256), 0, ST, p);
  else hipLaunchKernelGGL(attn_decode_fused_kernel<F16>, grid, dim3(256), 0, ST, p);
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}

extern "C" int sx_attn_decode(const void* q, const void* kcache, const void* vcache, void* out, float* scratch,
                              const int32_t* ctx_len_dev, int H, int D, int Tmax, int nsplit, float scale, int dtype,
                              void* stream) {
  return sx_attn_decode_b(q, kcache, vcache, out, scratch, ctx_len_dev, 1, H, D, Tmax, 0, nsplit, scale, dtype, 0, stream);
}

extern "C" int sx_rope_kv_append_b(void* qkv, void* kcache, void* vcache, const float* cos_tab, const float* sin_tab,
                                   const int32_t* pos0_dev, int G, int T, int H, int D, int Tmax,
                                   int64_t cache_seq_stride, int dtype, void* stream) {
  SX_CHECK(qkv && kcache && vcache && cos_tab && sin_tab && pos0_dev, "sx_rope_kv_append: null pointer");
  SX_CHECK(D % 2 == 0 && G >= 1 && T >= 1, "sx_rope_kv_append: D/G/T");
  const int64_t n = (int64_t)G * T * H * (D / 2);
  if (dtype == SX_BF16)
    hipLaunchKernelGGL(rope_kv_append_kernel<BF16>, gs_grid(n), dim3(256), 0, ST, (unsigned short*)qkv,
                       (unsigned short*)kcache, (unsigned short*)vcache, cos_tab, sin_tab, pos0_dev, T, H, D, Tmax, G,
                       (long long)cache_seq_stride);
  else
    hipLaunchKernelGGL(rope_kv_append_kernel<F16>, gs_grid(n), dim3(256), 0, ST, (unsigned short*)qkv,
                       (unsigned short*)kcache, (unsigned short*)vcache, cos_tab, sin_tab, pos0_dev, T, H, D, Tmax, G,
                       (long long)cache_seq_stride);
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}
extern "C" int sx_rope_kv_append(void* qkv, void* kcache, void* vcache, const float* cos_tab, const float* sin_tab,
                                 const int32_t* pos0_dev, int T, int H, int D, int Tmax, int dtype, void* stream) {
  return sx_rope_kv_append_b(qkv, kcache, vcache, cos_tab, sin_tab, pos0_dev, 1, T, H, D, Tmax, 0, dtype, stream);
}

extern "C" int sx_embedding(const int32_t* ids, const void* table, float* out, int T, int dim, int dtype,
                            void* stream) {
  SX_CHECK(ids && table && out, "sx_embedding: null pointer");
  if (dtype == SX_BF16)
    hipLaunchKernelGGL(embedding_kernel<BF16>, gs_grid((int64_t)T * dim), dim3(256), 0, ST, ids,
                       (const unsigned short*)table, out, T, dim);
  else
    hipLaunchKernelGGL(embedding_kernel<F16>, gs_grid((int64_t)T * dim), dim3(256), 0, ST, ids,
                       (const unsigned short*)table, out, T, dim);
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}

extern "C" int sx_scatter_rows(const float* src, const int32_t* rows, float* dst, int n, int dim, void* stream) {
  SX_CHECK(src && rows && dst, "sx_scatter_rows: null pointer");
  if (n == 0) return SX_OK;
  hipLaunchKernelGGL(scatter_rows_kernel, gs_grid((int64_t)n * dim), dim3(256), 0, ST, src, rows, dst, n, dim);
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}

static int sample_params(const sx_sample_args* s, int vocab, const char* who, SampleP* out) {
  SX_CHECK(s && s->do_sample && s->temperature && s->top_k && s->top_p && s->seed, "%s: null pointer in sx_sample_args", who);
  SX_CHECK(vocab >= 1 && vocab <= SMP_MAX_VOCAB, "%s: vocab=%d (a sampled row holds at most %d columns)", who, vocab, SMP_MAX_VOCAB);
  out->do_sample = s->do_sample; out->temperature = s->temperature; out->top_k = s->top_k; out->top_p = s->top_p;
  out->seed = s->seed; out->token_index = s->token_index; out->n_kept = s->n_kept; out->p_chosen = s->p_chosen;
  return SX_OK;
}

// sx_slot_step_args as the kernel's parameters: prev and next are both cur. A null struct gives null pointers, which the launcher refuses.
static TailP slot_tail(const sx_slot_step_args* a) {
  if (!a) return TailP{};
  return TailP{a->logits, a->img_ids_dev, a->cur, a->cur, a->out_ids, a->step, a->ld_logits, a->vocab, a->n_img, a->ld_out, a->G,
               a->live, a->n_new, a->max_new, a->force_at, a->pos, a->ctx, a->status, a->force_id, a->eos_id};
}

// The one launcher behind the thirteen entry points. slots: the in-flight form (every pointer but out_ids is required, ld_out is the row
// capacity), else the lock-step form. sampled: the entry point takes a sx_sample_args, which must then be there. lp: the LP form
// (sx_sample_next_b_lp / sx_sample_next_slots_lp); NULL launches exactly what the five older entry points always launched. ctl: the
// controlled forms (sx_next_b_ctl / sx_next_slots_ctl), any of the four combinations of sample and lp. fsm: the constrained forms
// (sx_next_b_fsm / sx_next_slots_fsm), on top of ctl. seq: the sequence-rule forms (sx_next_b_seq / sx_next_slots_seq), on top of ctl, with
// or without fsm.
static int launch_next_token(const char* who, const TailP& p, bool slots, const sx_sample_args* sample, bool sampled, void* stream,
                             const sx_logprob_args* lp = nullptr, const sx_logits_ctl_args* ctl = nullptr,
                             const sx_token_fsm_args* fsm = nullptr, const sx_seq_rule_args* seq = nullptr) {
  SX_CHECK(p.logits && p.img_ids && p.prev && p.next, "%s: null pointer", who);
  SX_CHECK(p.n_img >= 2 && p.n_img <= 1024 && p.G >= 1, "%s: n_img=%d G=%d", who, p.n_img, p.G);
  if (slots) {
    SX_CHECK(p.live && p.n_new && p.max_new && p.force_at && p.pos && p.ctx && p.step && p.status, "%s: null pointer", who);
    SX_CHECK(p.vocab >= 1 && p.ld_logits >= p.vocab, "%s: vocab=%d ld_logits=%d", who, p.vocab, p.ld_logits);
    SX_CHECK(!p.out_ids || p.ld_out >= 1, "%s: out_ids needs ld_out >= 1 (the row capacity)", who);
  } else {
    SX_CHECK(!p.out_ids || p.step, "%s: out_ids needs step_dev", who);
    SX_CHECK(!sampled || p.G == 1 || p.ld_logits >= p.vocab, "%s: vocab=%d ld_logits=%d", who, p.vocab, p.ld_logits);
  }
  SampleP s;
  if (sampled) {
    if (int rc = sample_params(sample, p.vocab, who, &s)) return rc;
    SX_CHECK(slots || s.token_index || (ctl && ctl->token_index), "%s: token_index is required", who);
    if (!slots && !s.token_index) s.token_index = ctl->token_index;
  }
  LogprobP l{};
  if (lp) {
    SX_CHECK(lp->want && lp->chosen && p.step, "%s: sx_logprob_args needs want, chosen and step", who);
    SX_CHECK(lp->n_top >= 0 && lp->n_top <= LP_MAX_TOP && (lp->n_top == 0 || (lp->top_ids && lp->top)),
             "%s: n_top=%d (0 .. %d, with top_ids and top)", who, lp->n_top, LP_MAX_TOP);
    SX_CHECK(p.vocab >= 1 && p.vocab <= SMP_MAX_VOCAB && p.ld_logits >= p.vocab && p.ld_out >= 1,
             "%s: vocab=%d (1 .. %d) ld_logits=%d ld_out=%d", who, p.vocab, SMP_MAX_VOCAB, p.ld_logits, p.ld_out);
    l = LogprobP{lp->want, lp->chosen, lp->top_ids, lp->top, lp->n_top};
  }
  if (!ctl && !lp) {        // (first in the source: the two older instantiations keep their place in the code object)
    if (sampled) hipLaunchKernelGGL(next_token_kernel<true>, dim3(p.G), dim3(1024), 0, ST, p, s, NoLogprobP{}, NoCtlP{});
    else hipLaunchKernelGGL(next_token_kernel<false>, dim3(p.G), dim3(1024), 0, ST, p, NoSampleP{}, NoLogprobP{}, NoCtlP{});
  } else if (!ctl) {
    if (sampled) hipLaunchKernelGGL((next_token_kernel<true, true>), dim3(p.G), dim3(1024), 0, ST, p, s, l, NoCtlP{});
    else hipLaunchKernelGGL((next_token_kernel<false, true>), dim3(p.G), dim3(1024), 0, ST, p, NoSampleP{}, l, NoCtlP{});
  } else {
    // the controlled forms: every row's working copy is ld_logits wide, the count words ld_counts; nothing is read past vocab
    SX_CHECK(ctl->on && ctl->counts && ctl->work && ctl->rep && ctl->rep_inv && ctl->presence && ctl->frequency && ctl->min_new &&
                 ctl->bias_ids && ctl->bias, "%s: null pointer in sx_logits_ctl_args", who);
    SX_CHECK(p.vocab >= 1 && p.ld_logits >= p.vocab && ctl->ld_counts >= p.vocab, "%s: vocab=%d ld_logits=%d ld_counts=%d", who, p.vocab,
             p.ld_logits, ctl->ld_counts);
    SX_CHECK(slots || ctl->token_index, "%s: sx_logits_ctl_args.token_index is required in the lock-step form", who);
    SX_CHECK(ctl->eos_id >= -1 && ctl->eos_id < p.vocab, "%s: sx_logits_ctl_args.eos_id=%d", who, ctl->eos_id);
    const CtlP c{ctl->on, ctl->counts, ctl->work, ctl->rep, ctl->rep_inv, ctl->presence, ctl->frequency, ctl->min_new, ctl->bias_ids,
                 ctl->bias, ctl->token_index, ctl->ld_counts, ctl->eos_id};
    CtlFsmP cf;
    if (fsm) {
      // the constrained forms: a table row is ld_v int16 wide and read two ids per dword up to vocab; table[g] and state[g] live on the
      // device and are range-checked by the kernel (a row outside [0, n_tables) x [0, n_states) runs unconstrained)
      SX_CHECK(fsm->table && fsm->state && fsm->trans && fsm->flags, "%s: null pointer in sx_token_fsm_args", who);
      SX_CHECK(fsm->n_tables >= 1 && fsm->n_states >= 1 && fsm->n_states <= 32767, "%s: sx_token_fsm_args n_tables=%d n_states=%d (>= 1, "
               "1 .. 32767)", who, fsm->n_tables, fsm->n_states);
      SX_CHECK(fsm->ld_v >= p.vocab && fsm->ld_v % 2 == 0 && ((uintptr_t)fsm->trans & 3) == 0,
               "%s: sx_token_fsm_args.ld_v=%d must be even and >= vocab=%d, trans 4-byte aligned", who, fsm->ld_v, p.vocab);
      SX_CHECK(fsm->eos_id >= -1 && fsm->eos_id < p.vocab, "%s: sx_token_fsm_args.eos_id=%d", who, fsm->eos_id);
      static_cast<CtlP&>(cf) = c;
      cf.f = FsmP{fsm->table, fsm->state, fsm->trans, fsm->flags, fsm->n_tables, fsm->n_states, fsm->ld_v, fsm->eos_id};
    }
    if (seq) {
      // (the sequence-rule forms are launched at the end, behind every older instantiation)
    } else if (fsm) {
      if (sampled && lp) hipLaunchKernelGGL((next_token_kernel<true, true, true, true>), dim3(p.G), dim3(1024), 0, ST, p, s, l, cf);
      else if (sampled) hipLaunchKernelGGL((next_token_kernel<true, false, true, true>), dim3(p.G), dim3(1024), 0, ST, p, s, NoLogprobP{}, cf);
      else if (lp) hipLaunchKernelGGL((next_token_kernel<false, true, true, true>), dim3(p.G), dim3(1024), 0, ST, p, NoSampleP{}, l, cf);
      else hipLaunchKernelGGL((next_token_kernel<false, false, true, true>), dim3(p.G), dim3(1024), 0, ST, p, NoSampleP{}, NoLogprobP{}, cf);
    } else if (sampled && lp) hipLaunchKernelGGL((next_token_kernel<true, true, true>), dim3(p.G), dim3(1024), 0, ST, p, s, l, c);
    else if (sampled) hipLaunchKernelGGL((next_token_kernel<true, false, true>), dim3(p.G), dim3(1024), 0, ST, p, s, NoLogprobP{}, c);
    else if (lp) hipLaunchKernelGGL((next_token_kernel<false, true, true>), dim3(p.G), dim3(1024), 0, ST, p, NoSampleP{}, l, c);
    else hipLaunchKernelGGL((next_token_kernel<false, false, true>), dim3(p.G), dim3(1024), 0, ST, p, NoSampleP{}, NoLogprobP{}, c);
    if (seq) {
      // the sequence-rule forms: a history row is ld_hist ids wide and never read or written past it; ngram[g], n_stop[g] and
      // stop_len[g][j] live on the device and are clamped by the kernel (a wrong table gives wrong ids, never a wild address)
      SX_CHECK(seq->on && seq->ngram && seq->hist && seq->hist_len && seq->prompt_len && seq->n_stop && seq->stop_len && seq->stop_ids &&
                   seq->matched, "%s: null pointer in sx_seq_rule_args", who);
      SX_CHECK(seq->ld_hist >= 1, "%s: sx_seq_rule_args.ld_hist=%d (>= 1)", who, seq->ld_hist);
      const SeqP q{seq->on, seq->ngram, seq->hist, seq->hist_len, seq->prompt_len, seq->n_stop, seq->stop_len, seq->stop_ids, seq->matched,
                   seq->ld_hist};
      if (fsm) {
        CtlFsmSeqP cq;
        static_cast<CtlFsmP&>(cq) = cf;
        cq.q = q;
        if (sampled && lp) hipLaunchKernelGGL((next_token_kernel<true, true, true, true, true>), dim3(p.G), dim3(1024), 0, ST, p, s, l, cq);
        else if (sampled) hipLaunchKernelGGL((next_token_kernel<true, false, true, true, true>), dim3(p.G), dim3(1024), 0, ST, p, s, NoLogprobP{}, cq);
        else if (lp) hipLaunchKernelGGL((next_token_kernel<false, true, true, true, true>), dim3(p.G), dim3(1024), 0, ST, p, NoSampleP{}, l, cq);
        else hipLaunchKernelGGL((next_token_kernel<false, false, true, true, true>), dim3(p.G), dim3(1024), 0, ST, p, NoSampleP{}, NoLogprobP{}, cq);
      } else {
        CtlSeqP cq;
        static_cast<CtlP&>(cq) = c;
        cq.q = q;
        if (sampled && lp) hipLaunchKernelGGL((next_token_kernel<true, true, true, false, true>), dim3(p.G), dim3(1024), 0, ST, p, s, l, cq);
        else if (sampled) hipLaunchKernelGGL((next_token_kernel<true, false, true, false, true>), dim3(p.G), dim3(1024), 0, ST, p, s, NoLogprobP{}, cq);
        else if (lp) hipLaunchKernelGGL((next_token_kernel<false, true, true, false, true>), dim3(p.G), dim3(1024), 0, ST, p, NoSampleP{}, l, cq);
        else hipLaunchKernelGGL((next_token_kernel<false, false, true, false, true>), dim3(p.G), dim3(1024), 0, ST, p, NoSampleP{}, NoLogprobP{}, cq);
      }
    }
  }
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}

// the lock-step forms never write step_dev (TailP.step is writable for the in-flight form)
extern "C" int sx_greedy_next_b(float* logits, int ld_logits, int vocab, const int32_t* img_ids_dev, int n_img,
                                const int32_t* prev_id_dev, int32_t* next_id_dev, int32_t* out_ids, int ld_out,
                                const int32_t* step_dev, int G, void* stream) {
  return launch_next_token("sx_greedy_next_b", TailP{logits, img_ids_dev, prev_id_dev, next_id_dev, out_ids, const_cast<int32_t*>(step_dev),
                                                     ld_logits, vocab, n_img, ld_out, G}, false, nullptr, false, stream);
}
extern "C" int sx_greedy_next(float* logits, int vocab, const int32_t* img_ids_dev, int n_img,
                              const int32_t* prev_id_dev, int32_t* next_id_dev, int32_t* out_ids,
                              const int32_t* step_dev, void* stream) {
  return sx_greedy_next_b(logits, 0, vocab, img_ids_dev, n_img, prev_id_dev, next_id_dev, out_ids, 0, step_dev, 1, stream);
}
extern "C" int sx_sample_next_b(float* logits, int ld_logits, int vocab, const int32_t* img_ids_dev, int n_img,
                                const int32_t* prev_id_dev, int32_t* next_id_dev, int32_t* out_ids, int ld_out,
                                const int32_t* step_dev, int G, const sx_sample_args* sample, void* stream) {
  return launch_next_token("sx_sample_next_b", TailP{logits, img_ids_dev, prev_id_dev, next_id_dev, out_ids, const_cast<int32_t*>(step_dev),
                                                     ld_logits, vocab, n_img, ld_out, G}, false, sample, true, stream);
}
extern "C" int sx_greedy_next_slots(const sx_slot_step_args* a, void* stream) {
  return launch_next_token("sx_greedy_next_slots", slot_tail(a), true, nullptr, false, stream);
}
extern "C" int sx_sample_next_slots(const sx_slot_step_args* a, const sx_sample_args* sample, void* stream) {
  return launch_next_token("sx_sample_next_slots", slot_tail(a), true, sample, true, stream);
}
extern "C" int sx_sample_next_b_lp(float* logits, int ld_logits, int vocab, const int32_t* img_ids_dev, int n_img,
                                   const int32_t* prev_id_dev, int32_t* next_id_dev, int32_t* out_ids, int ld_out,
                                   const int32_t* step_dev, int G, const sx_sample_args* sample, const sx_logprob_args* lp, void* stream) {
  SX_CHECK(lp, "sx_sample_next_b_lp: null sx_logprob_args");
  return launch_next_token("sx_sample_next_b_lp", TailP{logits, img_ids_dev, prev_id_dev, next_id_dev, out_ids, const_cast<int32_t*>(step_dev),
                                                        ld_logits, vocab, n_img, ld_out, G}, false, sample, sample != nullptr, stream, lp);
}
extern "C" int sx_sample_next_slots_lp(const sx_slot_step_args* a, const sx_sample_args* sample, const sx_logprob_args* lp, void* stream) {
  SX_CHECK(lp, "sx_sample_next_slots_lp: null sx_logprob_args");
  return launch_next_token("sx_sample_next_slots_lp", slot_tail(a), true, sample, sample != nullptr, stream, lp);
}
extern "C" int sx_next_b_ctl(float* logits, int ld_logits, int vocab, const int32_t* img_ids_dev, int n_img,
                             const int32_t* prev_id_dev, int32_t* next_id_dev, int32_t* out_ids, int ld_out,
                             const int32_t* step_dev, int G, const sx_sample_args* sample, const sx_logprob_args* lp,
                             const sx_logits_ctl_args* ctl, void* stream) {
  SX_CHECK(ctl, "sx_next_b_ctl: null sx_logits_ctl_args");
  return launch_next_token("sx_next_b_ctl", TailP{logits, img_ids_dev, prev_id_dev, next_id_dev, out_ids, const_cast<int32_t*>(step_dev),
                                                  ld_logits, vocab, n_img, ld_out, G}, false, sample, sample != nullptr, stream, lp, ctl);
}
extern "C" int sx_next_slots_ctl(const sx_slot_step_args* a, const sx_sample_args* sample, const sx_logprob_args* lp,
                                 const sx_logits_ctl_args* ctl, void* stream) {
  SX_CHECK(ctl, "sx_next_slots_ctl: null sx_logits_ctl_args");
  return launch_next_token("sx_next_slots_ctl", slot_tail(a), true, sample, sample != nullptr, stream, lp, ctl);
}
extern "C" int sx_next_b_fsm(float* logits, int ld_logits, int vocab, const int32_t* img_ids_dev, int n_img,
                             const int32_t* prev_id_dev, int32_t* next_id_dev, int32_t* out_ids, int ld_out,
                             const int32_t* step_dev, int G, const sx_sample_args* sample, const sx_logprob_args* lp,
                             const sx_logits_ctl_args* ctl, const sx_token_fsm_args* fsm, void* stream) {
  SX_CHECK(ctl && fsm, "sx_next_b_fsm: null sx_logits_ctl_args / sx_token_fsm_args");
  return launch_next_token("sx_next_b_fsm", TailP{logits, img_ids_dev, prev_id_dev, next_id_dev, out_ids, const_cast<int32_t*>(step_dev),
                                                  ld_logits, vocab, n_img, ld_out, G}, false, sample, sample != nullptr, stream, lp, ctl, fsm);
}
extern "C" int sx_next_slots_fsm(const sx_slot_step_args* a, const sx_sample_args* sample, const sx_logprob_args* lp,
                                 const sx_logits_ctl_args* ctl, const sx_token_fsm_args* fsm, void* stream) {
  SX_CHECK(ctl && fsm, "sx_next_slots_fsm: null sx_logits_ctl_args / sx_token_fsm_args");
  return launch_next_token("sx_next_slots_fsm", slot_tail(a), true, sample, sample != nullptr, stream, lp, ctl, fsm);
}
extern "C" int sx_next_b_seq(float* logits, int ld_logits, int vocab, const int32_t* img_ids_dev, int n_img,
                             const int32_t* prev_id_dev, int32_t* next_id_dev, int32_t* out_ids, int ld_out,
                             const int32_t* step_dev, int G, const sx_sample_args* sample, const sx_logprob_args* lp,
                             const sx_logits_ctl_args* ctl, const sx_token_fsm_args* fsm, const sx_seq_rule_args* seq, void* stream) {
  SX_CHECK(ctl && seq, "sx_next_b_seq: null sx_logits_ctl_args / sx_seq_rule_args");
  return launch_next_token("sx_next_b_seq", TailP{logits, img_ids_dev, prev_id_dev, next_id_dev, out_ids, const_cast<int32_t*>(step_dev),
                                                  ld_logits, vocab, n_img, ld_out, G}, false, sample, sample != nullptr, stream, lp, ctl, fsm, seq);
}
extern "C" int sx_next_slots_seq(const sx_slot_step_args* a, const sx_sample_args* sample, const sx_logprob_args* lp,
                                 const sx_logits_ctl_args* ctl, const sx_token_fsm_args* fsm, const sx_seq_rule_args* seq, void* stream) {
  SX_CHECK(ctl && seq, "sx_next_slots_seq: null sx_logits_ctl_args / sx_seq_rule_args");
  return launch_next_token("sx_next_slots_seq", slot_tail(a), true, sample, sample != nullptr, stream, lp, ctl, fsm, seq);
}
extern "C" int sx_token_logprobs(const float* logits, int64_t ld, int vocab, const int32_t* targets, float* chosen, int32_t* top_ids,
                                 float* top, int n_top, int rows, void* stream) {
  SX_CHECK(logits && targets && chosen, "sx_token_logprobs: null pointer");
  SX_CHECK(rows >= 1 && vocab >= 1 && ld >= vocab, "sx_token_logprobs: rows=%d vocab=%d ld=%lld", rows, vocab, (long long)ld);
  SX_CHECK(n_top >= 0 && n_top <= LP_MAX_TOP && (n_top == 0 || (top_ids && top)), "sx_token_logprobs: n_top=%d (0 .. %d, with top_ids and top)",
           n_top, LP_MAX_TOP);
  hipLaunchKernelGGL(token_logprobs_kernel<>, dim3(rows), dim3(1024), 0, ST, logits, ld, vocab, targets, chosen, top_ids, top, n_top);
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}

// ---- speculative decoding: the accept rule and the prompt-lookup drafter (include/seedx_hip.h: sx_spec_accept, sx_spec_draft_ngram) ---
// seedx_amd.spec states both rules in Python (accept, propose_ngram); the kernels equal them exactly.
// Accept: thread g walks slot g's T candidates. Everything it does for an emitted id is slot_advance's work for that id (force_at after
// the rule, the id log, the counters, the stop rule, parking, the status row), plus the id history at the cache position where the id
// will be fed; the walk goes on only while the id just emitted is the draft the next row was fed.
__global__ __launch_bounds__(64) void spec_accept_kernel(const sx_spec_accept_args a) {
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= a.G || a.live[g] == 0) return;             // parked: reads and writes nothing
  const int T = a.T, nd = min(max(a.n_draft[g], 0), T - 1);
  const int fa = a.force_at[g], mx = a.max_new[g];
  int n = a.n_new[g], st = a.step[g], ps = a.pos[g], cx = a.ctx[g];
  const int img_id = a.img_ids_dev ? a.img_ids_dev[0] : -1;
  int id = 0;
  bool stop = false;
  for (int t = 0; t < T; ++t) {
    id = a.cand[g * T + t];
    if (fa >= 0 && n == fa) id = a.force_id;
    if (a.out_ids && st >= 0 && st < a.ld_out) a.out_ids[(size_t)g * a.ld_out + st] = id;
    n += 1;
    st += 1;
    ps += 1;
    cx += 1;
    if (a.hist && ps >= 0 && ps < a.Tmax) a.hist[(size_t)g * a.Tmax + ps] = id;
    stop = (a.eos_id >= 0 && id == a.eos_id) || n >= mx;
    if (stop || t >= nd || id != a.rows_in[g * T + t + 1] || id == img_id) break;
  }
  a.cur[g] = id;
  a.rows_in[g * T] = id;                               // row 0 of the next verify step (a drafter rewrites the rows anyway)
  a.n_new[g] = n;
  if (stop) {
    a.live[g] = 0;
    a.step[g] = -1;
    a.pos[g] = -1;
    a.ctx[g] = 0;
  } else {
    a.step[g] = st;
    a.pos[g] = ps;
    a.ctx[g] = cx;
  }
  int* q = a.status + 4 * g;
  q[0] = id;
  q[1] = stop ? 0 : 1;
  q[2] = n;
  q[3] = stop ? n : -1;
}

// Draft: one workgroup per slot. L = pos + 1 known ids (hist[g][0 .. L), cur the last). For n = ngram_max .. ngram_min the threads
// stride over the starts i <= L - 1 - n and keep the largest one whose n ids equal the last n; the first n with a match wins and
// proposes hist[i + n .. min(i + n + K, L)). Rows: row 0 = cur, rows 1 .. n_draft = the draft, the rest cur (any valid id).
__global__ __launch_bounds__(256) void spec_draft_ngram_kernel(const sx_spec_draft_args a) {
  __shared__ int best;
  const int g = blockIdx.x, T = a.T;
  const int L = a.pos[g] + 1;
  int* rows = a.rows_out + (size_t)g * T;
  if (L <= 0 || L > a.Tmax) {                         // parked, or no room in the history: no draft; the row inputs stay valid ids
    if (threadIdx.x == 0) {
      a.n_draft[g] = 0;
      if (L > 0) for (int t = 0; t < T; ++t) rows[t] = a.cur[g];
    }
    return;
  }
  const int* h = a.hist + (size_t)g * a.Tmax;
  int found_n = 0, found_i = -1;
  for (int n = a.ngram_max; n >= a.ngram_min; --n) {  // uniform over the workgroup
    if (threadIdx.x == 0) best = -1;
    __syncthreads();
    int mine = -1;
    for (int i = threadIdx.x; i + n <= L - 1; i += 256) {
      bool eq = true;
      for (int e = 0; e < n; ++e) eq = eq && (h[i + e] == h[L - n + e]);
      if (eq) mine = i;                               // ascending i: the last match of the thread is its largest
    }
    if (mine >= 0) atomicMax(&best, mine);
    __syncthreads();
    const int b = best;
    __syncthreads();                                  // everyone has read best before the next n resets it
    if (b >= 0) { found_n = n; found_i = b; break; }
  }
  if (threadIdx.x != 0) return;
  const int cur = a.cur[g];
  int nd = 0;
  if (found_i >= 0) nd = min(T - 1, L - (found_i + found_n));
  rows[0] = cur;
  for (int t = 1; t < T; ++t) rows[t] = t <= nd ? h[found_i + found_n + t - 1] : cur;
  a.n_draft[g] = nd;
}

// dst[g][step[g] + t][:] = src[g*T + t][:] (the hidden-state log of a verify step: row t of slot g is the state at the input token that
// would be the slot's (step + t)-th), and tok[g*T + t] = max(step[g], 0) + t, the token index its candidate is drawn with
__global__ void scatter_rows_spec_kernel(const float* src, const int* step, float* dst, int* tok, int G, int T, int dim, int seq_rows) {
  const int64_t total = (int64_t)G * T * dim;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / dim), d = (int)(i % dim);
    const int g = r / T, t = r - g * T;
    const int st = step[g];
    if (tok && d == 0) tok[r] = (st < 0 ? 0 : st) + t;
    if (st < 0 || st + t >= seq_rows) continue;      // parked, or past the log: drop the row instead of corrupting HBM
    dst[((size_t)g * seq_rows + st + t) * dim + d] = src[i];
  }
}

extern "C" int sx_scatter_rows_spec(const float* src, const int32_t* step_dev, float* dst, int32_t* tok_index, int G, int T, int dim,
                                    int seq_rows, void* stream) {
  SX_CHECK(src && step_dev && dst && G >= 1 && T >= 1 && dim >= 1 && seq_rows >= 1, "sx_scatter_rows_spec: bad args");
  hipLaunchKernelGGL(scatter_rows_spec_kernel, gs_grid((int64_t)G * T * dim), dim3(256), 0, ST, src, step_dev, dst, tok_index, G, T, dim,
                     seq_rows);
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}

extern "C" int sx_spec_accept(const sx_spec_accept_args* a, void* stream) {
  SX_CHECK(a && a->cand && a->rows_in && a->n_draft && a->cur && a->live && a->n_new && a->max_new && a->force_at && a->pos && a->ctx &&
           a->step && a->status, "sx_spec_accept: null pointer");
  SX_CHECK(a->G >= 1 && a->T >= 1 && a->T <= 8 && (int64_t)a->G * a->T <= 32, "sx_spec_accept: G=%d T=%d (T <= 8, G*T <= 32)", a->G, a->T);
  SX_CHECK(!a->out_ids || a->ld_out >= 1, "sx_spec_accept: out_ids needs ld_out >= 1 (the row capacity)");
  SX_CHECK(!a->hist || a->Tmax >= 1, "sx_spec_accept: hist needs Tmax >= 1");
  hipLaunchKernelGGL(spec_accept_kernel, dim3((a->G + 63) / 64), dim3(64), 0, ST, *a);
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}

extern "C" int sx_spec_draft_ngram(const sx_spec_draft_args* a, void* stream) {
  SX_CHECK(a && a->hist && a->pos && a->cur && a->rows_out && a->n_draft, "sx_spec_draft_ngram: null pointer");
  SX_CHECK(a->G >= 1 && a->T >= 2 && a->T <= 8 && (int64_t)a->G * a->T <= 32 && a->Tmax >= 1, "sx_spec_draft_ngram: G=%d T=%d Tmax=%d (2 <= T <= 8, G*T <= 32)",
           a->G, a->T, a->Tmax);
  SX_CHECK(a->ngram_min >= 1 && a->ngram_max >= a->ngram_min && a->ngram_max <= 16, "sx_spec_draft_ngram: ngram_max=%d ngram_min=%d (1 <= min <= max <= 16)",
           a->ngram_max, a->ngram_min);
  hipLaunchKernelGGL(spec_draft_ngram_kernel, dim3(a->G), dim3(256), 0, ST, *a);
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}

extern "C" int sx_scatter_rows_step(const float* src, const int32_t* step_dev, float* dst, int G, int dim, int seq_rows,
                                    void* stream) {
  SX_CHECK(src && step_dev && dst && G >= 1, "sx_scatter_rows_step: bad args");
  hipLaunchKernelGGL(scatter_rows_step_kernel, gs_grid((int64_t)G * dim), dim3(256), 0, ST, src, step_dev, dst, G, dim,
                     seq_rows);
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}

// ---- KV-cache prefix fork (include/seedx_hip.h: sx_kv_fork) ---------------------------------------------------------------------------
// Block (x, y, z) = (byte chunk, outer * inner, pair). The span of one (pair, outer, inner) is n_rows * row_bytes contiguous bytes in
// both slots. Where source and destination share their alignment modulo 16 the body moves as 16-byte vectors (lane i at base + 16 i: 1 KiB
// per wave instruction, four independent loads per lane ahead of their stores) and only the head / tail words move as dwords; otherwise the whole span moves as
// dwords. The blocks of one span stride over it, so a long prefix spreads over gridDim.x blocks per (pair, outer, inner).
__global__ void __launch_bounds__(256) kv_fork_kernel(sx_kv_fork_args a) {
  const int pair = blockIdx.z;
  const int s = a.src[pair], d = a.dst[pair];
  int n = a.n_rows[pair];
  if (s < 0 || s >= a.G || d < 0 || d >= a.G || s == d || n <= 0) return;          // block-uniform: the skip rules
  n = n > a.Tmax ? a.Tmax : n;
  const int o = blockIdx.y / a.inner, h = blockIdx.y - o * a.inner;
  const int64_t base = (int64_t)o * a.outer_stride + (int64_t)h * a.inner_stride;
  const char* sp = (const char*)a.cache + base + (int64_t)s * a.slot_stride;
  char* dp = (char*)a.cache + base + (int64_t)d * a.slot_stride;
  const int64_t nbytes = (int64_t)n * a.row_bytes;
  int64_t head = nbytes, body = 0;
  if ((((uintptr_t)sp ^ (uintptr_t)dp) & 15) == 0) {
    head = (int64_t)((16 - ((uintptr_t)sp & 15)) & 15);
    head = head < nbytes ? head : nbytes;
    body = (nbytes - head) & ~(int64_t)15;
  }
  const int64_t stride = (int64_t)gridDim.x * 256, t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const uint4* sv = (const uint4*)(sp + head);
  uint4* dv = (uint4*)(dp + head);
  const int64_t nvec = body >> 4;
  int64_t v = t0;
  for (; v + 3 * stride < nvec; v += 4 * stride) {                                  // full quads: four loads issued, then four stores
    const uint4 r0 = sv[v], r1 = sv[v + stride], r2 = sv[v + 2 * stride], r3 = sv[v + 3 * stride];
    dv[v] = r0;
    dv[v + stride] = r1;
    dv[v + 2 * stride] = r2;
    dv[v + 3 * stride] = r3;
  }
  for (; v < nvec; v += stride) dv[v] = sv[v];                                      // the last, partial quad
  const int64_t hw = head >> 2, nw = (nbytes - body) >> 2;                          // head words, then tail words
  for (int64_t w = t0; w < nw; w += stride) {
    const int64_t off = w < hw ? w * 4 : head + body + (w - hw) * 4;
    *(uint32_t*)(dp + off) = *(const uint32_t*)(sp + off);
  }
}

extern "C" int sx_kv_fork(const sx_kv_fork_args* a, void* stream) {
  SX_CHECK(a && a->cache && a->src && a->dst && a->n_rows, "sx_kv_fork: null pointer");
  SX_CHECK(a->n_pairs >= 0 && a->n_pairs <= 65535, "sx_kv_fork: n_pairs=%d must be 0..65535", a->n_pairs);
  SX_CHECK(a->outer >= 1 && a->G >= 1 && a->inner >= 1 && a->Tmax >= 1 && a->row_bytes >= 4, "sx_kv_fork: bad dims");
  SX_CHECK((int64_t)a->outer * a->inner <= 65535, "sx_kv_fork: outer * inner = %lld exceeds 65535", (long long)a->outer * a->inner);
  SX_CHECK(a->row_bytes % 4 == 0 && ((uintptr_t)a->cache & 3) == 0 && a->outer_stride % 4 == 0 && a->slot_stride % 4 == 0 &&
               a->inner_stride % 4 == 0, "sx_kv_fork: cache, strides and row_bytes must be multiples of 4 bytes");
  const int64_t span = (int64_t)a->Tmax * a->row_bytes;
  SX_CHECK(a->inner_stride >= span && a->slot_stride >= (a->inner - 1) * a->inner_stride + span &&
               a->outer_stride >= (a->G - 1) * a->slot_stride + (a->inner - 1) * a->inner_stride + span,
           "sx_kv_fork: strides do not describe [outer][G][inner][Tmax][row_bytes]");
  if (a->n_pairs == 0) return SX_OK;
  // chunks of 16 KB (256 lanes x 4 vectors), as many blocks per span as fill the machine (~4096 in all) and no more than the span has chunks
  const int64_t spans = (int64_t)a->n_pairs * a->outer * a->inner, chunks = (span + 16383) / 16384;
  int64_t gx = (4096 + spans - 1) / spans;
  gx = gx < 1 ? 1 : (gx > chunks ? chunks : gx);
  hipLaunchKernelGGL(kv_fork_kernel, dim3((unsigned)gx, (unsigned)(a->outer * a->inner), (unsigned)a->n_pairs), dim3(256), 0, ST, *a);
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}

// ---- KV-cache rows <-> linear staging (include/seedx_hip.h: sx_kv_rows_copy) ------------------------------------------------------------
// kv_fork_kernel with one side in a staging buffer. Block (x, y, z) = (byte chunk, tensor * outer * inner + outer index * inner + head,
// job). The span of one (job, tensor, outer, inner) is n * row_bytes contiguous bytes on both sides; the staging side starts on a
// multiple of 16 (offsets and span sizes are), so a 16-byte aligned cache span moves as 16-byte vectors (lane i at base + 16 i, four
// independent loads per lane ahead of their stores) with a dword tail, any other span as dwords. The blocks of one span stride over
// it. The small spans of a launch (scale rows: 4 bytes a row beside 128) share gridDim.x with the large ones: their extra blocks find
// no work and leave.
__host__ __device__ __forceinline__ int64_t kv_span_bytes(int64_t n, int32_t row_bytes) { return (n * row_bytes + 15) & ~(int64_t)15; }

__global__ void __launch_bounds__(256) kv_rows_copy_kernel(sx_kv_rows_args a) {
  const int job = blockIdx.z;
  const int g = a.slot[job];
  int n = a.n_rows[job];
  const int64_t off = a.offset[job];
  if (g < 0 || g >= a.G || n <= 0 || off < 0 || (off & 15)) return;                 // block-uniform: the skip rules
  n = n > a.Tmax ? a.Tmax : n;
  const int oi = a.outer * a.inner;
  const int ti = blockIdx.y / oi, s = blockIdx.y - ti * oi;
  const int o = s / a.inner, h = s - o * a.inner;
  int64_t before = 0, total = 0;                                                    // the job's bytes in front of tensor ti, and in all
  sx_kv_tensor t = a.tensor[0];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < a.n_tensors) {
      const int64_t b = (int64_t)oi * kv_span_bytes(n, a.tensor[k].row_bytes);
      before += k < ti ? b : 0;
      total += b;
      if (k == ti) t = a.tensor[k];
    }
  }
  if (off + total > a.staging_bytes) return;                                        // the guard: never beyond the staging buffer
  char* cp = (char*)t.base + (int64_t)o * t.outer_stride + (int64_t)g * t.slot_stride + (int64_t)h * t.inner_stride;
  char* gp = (char*)a.staging + off + before + (int64_t)s * kv_span_bytes(n, t.row_bytes);
  const char* sp = a.direction ? gp : cp;
  char* dp = a.direction ? cp : gp;
  const int64_t nbytes = (int64_t)n * t.row_bytes;
  const int64_t body = ((uintptr_t)cp & 15) == 0 ? nbytes & ~(int64_t)15 : 0;
  const int64_t stride = (int64_t)gridDim.x * 256, t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const uint4* sv = (const uint4*)sp;
  uint4* dv = (uint4*)dp;
  const int64_t nvec = body >> 4;
  int64_t v = t0;
  for (; v + 3 * stride < nvec; v += 4 * stride) {                                  // full quads: four loads issued, then four stores
    const uint4 r0 = sv[v], r1 = sv[v + stride], r2 = sv[v + 2 * stride], r3 = sv[v + 3 * stride];
    dv[v] = r0;
    dv[v + stride] = r1;
    dv[v + 2 * stride] = r2;
    dv[v + 3 * stride] = r3;
  }
  for (; v < nvec; v += stride) dv[v] = sv[v];                                      // the last, partial quad
  const int64_t nw = (nbytes - body) >> 2;                                          // the tail words, or the whole unaligned span
  for (int64_t w = t0; w < nw; w += stride) *(uint32_t*)(dp + body + w * 4) = *(const uint32_t*)(sp + body + w * 4);
}

extern "C" int64_t sx_kv_rows_job_bytes(const int32_t* row_bytes, int n_tensors, int outer, int inner, int Tmax, int n_rows) {
  if (!row_bytes || n_tensors < 1 || n_tensors > 4) return -1;
  const int64_t n = n_rows <= 0 ? 0 : (n_rows > Tmax ? Tmax : n_rows);
  int64_t sum = 0;
  for (int k = 0; k < n_tensors; ++k) sum += (int64_t)outer * inner * kv_span_bytes(n, row_bytes[k]);
  return sum;
}

extern "C" int sx_kv_rows_copy(const sx_kv_rows_args* a, void* stream) {
  SX_CHECK(a && a->slot && a->n_rows && a->offset && a->host_slot && a->host_n_rows && a->host_offset && a->staging,
           "sx_kv_rows_copy: null pointer");
  SX_CHECK(a->n_tensors >= 1 && a->n_tensors <= 4, "sx_kv_rows_copy: n_tensors=%d must be 1..4 (kc, vc, ks, vs)", a->n_tensors);
  SX_CHECK(a->direction == 0 || a->direction == 1, "sx_kv_rows_copy: direction=%d must be 0 (pack) or 1 (unpack)", a->direction);
  SX_CHECK(a->n_jobs >= 0 && a->n_jobs <= 65535, "sx_kv_rows_copy: n_jobs=%d must be 0..65535", a->n_jobs);
  SX_CHECK(a->outer >= 1 && a->G >= 1 && a->inner >= 1 && a->Tmax >= 1, "sx_kv_rows_copy: bad dims");
  SX_CHECK((int64_t)a->n_tensors * a->outer * a->inner <= 65535, "sx_kv_rows_copy: n_tensors * outer * inner = %lld exceeds 65535",
           (long long)a->n_tensors * a->outer * a->inner);
  SX_CHECK(((uintptr_t)a->staging & 15) == 0 && a->staging_bytes >= 0, "sx_kv_rows_copy: staging must be 16-byte aligned");
  int32_t row_bytes[4];
  int64_t max_span = 0;
  for (int k = 0; k < a->n_tensors; ++k) {
    const sx_kv_tensor& t = a->tensor[k];
    SX_CHECK(t.base, "sx_kv_rows_copy: null pointer (tensor %d)", k);
    SX_CHECK(t.row_bytes >= 4 && t.row_bytes % 4 == 0 && ((uintptr_t)t.base & 3) == 0 && t.outer_stride % 4 == 0 && t.slot_stride % 4 == 0 &&
                 t.inner_stride % 4 == 0, "sx_kv_rows_copy: base, strides and row_bytes of tensor %d must be multiples of 4 bytes", k);
    const int64_t span = (int64_t)a->Tmax * t.row_bytes;
    SX_CHECK(t.inner_stride >= span && t.slot_stride >= (a->inner - 1) * t.inner_stride + span &&
                 t.outer_stride >= (a->G - 1) * t.slot_stride + (a->inner - 1) * t.inner_stride + span,
             "sx_kv_rows_copy: the strides of tensor %d do not describe [outer][G][inner][Tmax][row_bytes]", k);
    row_bytes[k] = t.row_bytes;
    max_span = span > max_span ? span : max_span;
  }
  int64_t longest = 0;
  for (int j = 0; j < a->n_jobs; ++j) {                                             // the jobs as the host states them
    const int64_t off = a->host_offset[j];
    SX_CHECK(off >= 0 && off % 16 == 0, "sx_kv_rows_copy: offset[%d]=%lld must be a multiple of 16 (and >= 0)", j, (long long)off);
    if (a->host_slot[j] < 0 || a->host_slot[j] >= a->G || a->host_n_rows[j] <= 0) continue;       // skipped by the kernel
    const int64_t need = sx_kv_rows_job_bytes(row_bytes, a->n_tensors, a->outer, a->inner, a->Tmax, a->host_n_rows[j]);
    SX_CHECK(off + need <= a->staging_bytes, "sx_kv_rows_copy: job %d (slot %d, %d rows) ends at byte %lld of a staging buffer of %lld",
             j, a->host_slot[j], a->host_n_rows[j], (long long)(off + need), (long long)a->staging_bytes);
    const int64_t n = a->host_n_rows[j] > a->Tmax ? a->Tmax : a->host_n_rows[j];
    longest = n > longest ? n : longest;
  }
  if (a->n_jobs == 0 || longest == 0) return SX_OK;
  // kv_fork's sizing: chunks of 16 KB (256 lanes x 4 vectors), as many blocks per span as fill the machine (~4096 in all) and no more
  // than the longest span of the launch has chunks
  const int64_t spans = (int64_t)a->n_jobs * a->n_tensors * a->outer * a->inner;
  int64_t chunks = (max_span / a->Tmax * longest + 16383) / 16384;
  int64_t gx = (4096 + spans - 1) / spans;
  gx = gx < 1 ? 1 : (gx > chunks ? chunks : gx);
  hipLaunchKernelGGL(kv_rows_copy_kernel, dim3((unsigned)gx, (unsigned)(a->n_tensors * a->outer * a->inner), (unsigned)a->n_jobs), dim3(256),
                     0, ST, *a);
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}

// ---- decode tiles → row-major 16-bit matrix (include/seedx_hip.h: sx_dequant_tiles) ---------------------------------------------------
// The skinny GEMM's weight fragment load, run backwards: a wave takes one 64-k slab of a row group per step. The two half-waves own rows
// 0..7 and 8..15 of the 16-row tile: lane (s = lane >> 5, r8 = (lane >> 2) & 7, g = lane & 3) loads what lane (row r8 + 8 s, group g) of
// the MFMA loads — 16 B of FP8 codes at 64 r + 16 g, or 8 B of MXFP4 codes at 32 r + 8 g plus the row's two E8M0 bytes — and converts it
// with the GEMM's own converts to the eight k-slots of 32-k half 0 (A: k = 8 g ..) and of half 1 (B: k = 32 + 8 g ..). Writes are four
// times the reads, so the store side decides the mapping: as loaded, a store instruction would cover 64-B pieces of 16 rows (the four g
// of a row are one half of its 128-B segment). One v_permlane32_swap per dword hands the lower half-wave's B to the upper one and the
// upper's A down: then the first store (A') covers rows 0..7 and the second (B') rows 8..15, each row's whole 128-B segment = 16 B x the
// eight lanes (g, s) — no LDS. Rows 16..19 of a 20-row tile (behind the 16-row tile) are done 32 lanes per slab, lane = (row, 16-B piece):
// an 8-B (MXFP4: 4-B) load per lane, the same whole segments. U slabs per wave are loaded ahead of their converts; consecutive waves take
// consecutive slabs, so a row's segments are written in address order.
struct DequantP {
  const unsigned char* tiles;
  const float* rscale;
  const unsigned char* bscale;
  unsigned short* out;
  int K, nks;
};

// eight e4m3 codes times the row's power-of-two scale → eight 16-bit values: the code → fp32 convert of fp8x8_to16's bf16 path, the scale
// in fp32 (exact: a power of two), one rounding-free convert down (the product has 4 significant bits and lies in the format's range)
template <typename TT>
__device__ __forceinline__ u32x4_t fp8x8_scaled_to16(unsigned d0, unsigned d1, float sc) {
  u32x4_t o = {0u, 0u, 0u, 0u};
#if defined(__HIP_DEVICE_COMPILE__)
  const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8(d0, false), b = __builtin_amdgcn_cvt_pk_f32_fp8(d0, true);
  const f32x2_t c = __builtin_amdgcn_cvt_pk_f32_fp8(d1, false), d = __builtin_amdgcn_cvt_pk_f32_fp8(d1, true);
  o[0] = pack2<TT>(a[0] * sc, a[1] * sc);
  o[1] = pack2<TT>(b[0] * sc, b[1] * sc);
  o[2] = pack2<TT>(c[0] * sc, c[1] * sc);
  o[3] = pack2<TT>(d[0] * sc, d[1] * sc);
#endif
  return o;
}

template <typename TT, bool W4, bool TAIL>
__global__ __launch_bounds__(256) void dequant_tiles_kernel(const DequantP p) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int U = 4;                        // 64-k slabs per wave
  constexpr int ROWS = TAIL ? 20 : 16;
  constexpr int RB = W4 ? 32 : 64;            // bytes of one row in a slab's tile
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int t0 = (blockIdx.y * 4 + wave) * U;
  if (t0 >= p.nks) return;                    // wave-uniform
  const int nu = p.nks - t0 < U ? p.nks - t0 : U;
  const int n0 = blockIdx.x * ROWS;
  const size_t slab0 = (size_t)blockIdx.x * p.nks + t0;            // this wave's first slab: tiles, scale tiles and k are indexed by it
  const unsigned char* tile = p.tiles + slab0 * (ROWS * RB);
  const unsigned char* stile = W4 ? p.bscale + slab0 * (ROWS * 2) : nullptr;
  {
    const int s = lane >> 5, r = ((lane >> 2) & 7) + 8 * s, g = lane & 3;
    u32x4_t w[U];
    unsigned short ws[U];
    float rs = 0.f;
    if constexpr (!W4) rs = p.rscale[n0 + r];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u < nu) {
        const unsigned char* q = tile + (size_t)u * (ROWS * RB) + r * RB + g * (RB / 4);
        if constexpr (W4) {
          const u32x2_t d = *(const u32x2_t*)q;
          w[u] = (u32x4_t){d[0], d[1], 0u, 0u};
          ws[u] = *(const unsigned short*)(stile + (size_t)u * (ROWS * 2) + 2 * r);
        } else {
          w[u] = *(const u32x4_t*)q;
        }
      }
    }
    // first store: row n0 + r8, second: row n0 + 8 + r8; this lane's 16-B piece of the 128-B segment is g + 4 s in both
    unsigned short* o0 = p.out + (size_t)(n0 + (r & 7)) * p.K + (size_t)t0 * 64 + 8 * (g + 4 * s);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u < nu) {
        u32x4_t A, B;
        if constexpr (W4) {
          A = __builtin_bit_cast(u32x4_t, fp4x8_to16<TT>(w[u][0], __uint_as_float(((unsigned)ws[u] & 0xffu) << 23)));
          B = __builtin_bit_cast(u32x4_t, fp4x8_to16<TT>(w[u][1], __uint_as_float(((unsigned)ws[u] >> 8) << 23)));
        } else {
          A = fp8x8_scaled_to16<TT>(w[u][0], w[u][1], rs);
          B = fp8x8_scaled_to16<TT>(w[u][2], w[u][3], rs);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {   // lanes 32..63 of A <-> lanes 0..31 of B
          const auto x = __builtin_amdgcn_permlane32_swap(A[i], B[i], false, false);
          A[i] = x[0];
          B[i] = x[1];
        }
        *(u32x4_t*)(o0 + u * 64) = A;
        *(u32x4_t*)(o0 + (size_t)8 * p.K + u * 64) = B;
      }
    }
  }
  if constexpr (TAIL) {   // rows 16..19: two slabs per pass, lane = (slab u2 + (lane >> 5), row rr, 16-B piece c = 4 h + g)
    const int rr = (lane >> 3) & 3, c = lane & 7, g = c & 3, h = c >> 2;
    float rs = 0.f;
    if constexpr (!W4) rs = p.rscale[n0 + 16 + rr];
#pragma unroll
    for (int u2 = 0; u2 < U; u2 += 2) {
      const int u = u2 + (lane >> 5);
      if (u < nu) {
        const unsigned char* q = tile + (size_t)u * (ROWS * RB) + 16 * RB + rr * RB + g * (RB / 4) + h * (RB / 8);
        u32x4_t v;
        if constexpr (W4) {
          const unsigned sc = stile[(size_t)u * (ROWS * 2) + 32 + 2 * rr + h];
          v = __builtin_bit_cast(u32x4_t, fp4x8_to16<TT>(*(const unsigned*)q, __uint_as_float(sc << 23)));
        } else {
          const u32x2_t d = *(const u32x2_t*)q;
          v = fp8x8_scaled_to16<TT>(d[0], d[1], rs);
        }
        *(u32x4_t*)(p.out + (size_t)(n0 + 16 + rr) * p.K + (size_t)(t0 + u) * 64 + 8 * c) = v;
      }
    }
  }
#endif
}

template <typename TT>
static void dequant_tiles_launch(const DequantP& p, bool w4, bool tail, dim3 grid, void* stream) {
  if (w4) {
    if (tail) hipLaunchKernelGGL((dequant_tiles_kernel<TT, true, true>), grid, dim3(256), 0, ST, p);
    else hipLaunchKernelGGL((dequant_tiles_kernel<TT, true, false>), grid, dim3(256), 0, ST, p);
  } else {
    if (tail) hipLaunchKernelGGL((dequant_tiles_kernel<TT, false, true>), grid, dim3(256), 0, ST, p);
    else hipLaunchKernelGGL((dequant_tiles_kernel<TT, false, false>), grid, dim3(256), 0, ST, p);
  }
}

extern "C" int sx_dequant_tiles(const sx_dequant_tiles_args* a, void* stream) {
  SX_CHECK(a && a->tiles && a->out, "sx_dequant_tiles: null pointer");
  SX_CHECK(a->dtype == SX_F16 || a->dtype == SX_BF16, "sx_dequant_tiles: dtype must be SX_F16 or SX_BF16");
  SX_CHECK(a->w_dtype == SX_FP8_E4M3 || a->w_dtype == SX_FP4_E2M1, "sx_dequant_tiles: w_dtype must be SX_FP8_E4M3 or SX_FP4_E2M1");
  SX_CHECK(a->w_layout == 1 || a->w_layout == 2, "sx_dequant_tiles: w_layout must be 1 (16-row decode tiles) or 2 (20-row decode tiles)");
  const int rows = a->w_layout == 1 ? 16 : 20;
  SX_CHECK(a->N > 0 && a->K > 0 && a->K % 64 == 0 && a->N % rows == 0,
           "sx_dequant_tiles: N=%d K=%d need K %% 64 == 0 and N %% %d == 0 (w_layout %d)", a->N, a->K, rows, a->w_layout);
  SX_CHECK(((uintptr_t)a->tiles & 15) == 0 && ((uintptr_t)a->out & 15) == 0, "sx_dequant_tiles: tiles and out must be 16-B aligned");
  const bool w4 = a->w_dtype == SX_FP4_E2M1;
  if (w4) {
    SX_CHECK(a->w_block_scale && ((uintptr_t)a->w_block_scale & 15) == 0,
             "sx_dequant_tiles: SX_FP4_E2M1 tiles need w_block_scale (16-B aligned E8M0 scale tiles)");
    SX_CHECK(!a->w_scale, "sx_dequant_tiles: w_scale belongs to SX_FP8_E4M3 tiles");
  } else {
    SX_CHECK(a->w_scale && ((uintptr_t)a->w_scale & 15) == 0, "sx_dequant_tiles: SX_FP8_E4M3 tiles need w_scale (16-B aligned fp32 [N])");
    SX_CHECK(!a->w_block_scale, "sx_dequant_tiles: w_block_scale belongs to SX_FP4_E2M1 tiles");
  }
  SX_CHECK(a->out_bytes >= (uint64_t)a->N * (uint64_t)a->K * 2, "sx_dequant_tiles: out_bytes=%llu is less than N * K * 2 = %llu",
           (unsigned long long)a->out_bytes, (unsigned long long)a->N * (unsigned long long)a->K * 2);
  DequantP p;
  p.tiles = (const unsigned char*)a->tiles;
  p.rscale = a->w_scale;
  p.bscale = (const unsigned char*)a->w_block_scale;
  p.out = (unsigned short*)a->out;
  p.K = a->K;
  p.nks = a->K / 64;
  const int gy = (p.nks + 15) / 16;            // 4 waves x 4 slabs per workgroup
  SX_CHECK(gy <= 65535, "sx_dequant_tiles: K=%d is too large", a->K);
  const dim3 grid((unsigned)(a->N / rows), (unsigned)gy);
  if (a->dtype == SX_F16) dequant_tiles_launch<F16>(p, w4, a->w_layout == 2, grid, stream);
  else dequant_tiles_launch<BF16>(p, w4, a->w_layout == 2, grid, stream);
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}
