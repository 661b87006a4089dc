// Per-request LoRA adapters kept UNMERGED beside one resident base model (seedx_amd/lora.py states the rule in fp64): for a projection
// W[N][K], an input row x = hi + lo (two 16-bit planes) and the row's adapter a with A_a[r][K], B_a[N][r] (16-bit) and s_a = alpha / r,
//     t[i]     = sum_k A_a[i][k] * (hi[k] + lo[k])        fp32, t stays fp32            (sx_lora_shrink)
//     delta[n] = s_a * sum_j B_a[n][j] * t[j]             fp32                           (sx_lora_expand)
// and delta enters the projection's epilogue BEFORE activation / GLU / residual (sx_gemv_args.addend on the decode step, sx_gemm's
// bias2d in prefill) — peft's Linear.forward (proj/peft/src/peft/tuners/lora.py:808-825, dropout off) with the intermediate kept in fp32.
// modules_to_save norm weights replace gamma for the adapter's rows only (sx_rmsnorm_planes_sel).
// Every kernel reads the row's adapter index from DEVICE memory (sel[row]; graph-capturable, no host reads), treats an index outside
// [0, n_adapters) as a base row (nothing is read from the adapter tables, nothing is written for it) and has a fixed reduction order that
// involves the row's own data only: a row's result does not depend on its slot, its neighbours, the row count or eager versus replay.
// Compiled WITHOUT -ffast-math (csrc/build.sh), like precise.hip: hi + lo and the fma chains must stay as written.
#include "sx_common.h"
#include "precise_rows.h"

namespace sxk_lora {

struct ShrinkP {
  const unsigned short* x;
  const unsigned short* A;
  const int* sel;
  float* t;
  int K, SR, n_adapters;
  int tiled;   // 0: x rows [M][2K] = [hi | lo]; else the row blocks RB of operand tiles [2][RB][K/32][16][32]
};

// One wave per (row g, 4 consecutive outputs i): the lanes walk K in 8-element chunks (lane, lane + 64, ...) with 16-B loads of the two x
// planes (read once for the 4 outputs) and of the 4 A rows; per lane an fma chain in k order, then the wave butterfly — both fixed.
template <typename TT>
__global__ __launch_bounds__(256) void lora_shrink_kernel(const ShrinkP p) {
  const int g = blockIdx.y, lane = threadIdx.x & 63;
  const int i0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 4;
  const int a = p.sel[g];
  if (a < 0 || a >= p.n_adapters || i0 >= p.SR) return;      // base row: the tables are not touched, t[g] is not written
  const unsigned short* Ar = p.A + ((size_t)a * p.SR + i0) * (size_t)p.K;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int c8 = lane * 8; c8 < p.K; c8 += 512) {
    const unsigned short* xh = p.tiled ? p.x + ((size_t)(g >> 4) * (size_t)(p.K >> 5) + (size_t)(c8 >> 5)) * 512 + (size_t)(g & 15) * 32 + (c8 & 31)
                                       : p.x + (size_t)g * 2 * p.K + c8;
    const u32x4_t h = *(const u32x4_t*)xh;
    const u32x4_t l = *(const u32x4_t*)(xh + (p.tiled ? (size_t)p.K * 16 * (size_t)p.tiled : (size_t)p.K));
    float xs[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {     // hi + lo is exact in fp32 (the planes span at most 23 bits)
      xs[2 * e] = TT::to_f32(h[e] & 0xffff) + TT::to_f32(l[e] & 0xffff);
      xs[2 * e + 1] = TT::to_f32(h[e] >> 16) + TT::to_f32(l[e] >> 16);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const u32x4_t w = *(const u32x4_t*)(Ar + (size_t)j * p.K + c8);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[j] = fmaf(TT::to_f32(w[e] & 0xffff), xs[2 * e], acc[j]);
        acc[j] = fmaf(TT::to_f32(w[e] >> 16), xs[2 * e + 1], acc[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = wave_sum(acc[j]);
  if (lane == 0) *(f32x4_t*)(p.t + (size_t)g * p.SR + i0) = (f32x4_t){acc[0], acc[1], acc[2], acc[3]};
}

struct ExpandP {
  const float* t;
  const unsigned short* B;
  const int* seg;
  const float* scale;
  const int* sel;
  float* delta;
  int N, R, S, n_adapters;
};

#define SX_LORA_MAX_SR 512

// One thread per (row g, output n): the row's t (S * R floats) sits in LDS, the thread reads its B row (R 16-bit values, 16-B loads) and
// runs one fma chain in j order. seg[n / 16] picks the S-segment of t; it is clamped into [0, S), so a bad table cannot read out of bounds.
template <typename TT>
__global__ __launch_bounds__(256) void lora_expand_kernel(const ExpandP p) {
  __shared__ float ts[SX_LORA_MAX_SR];
  const int g = blockIdx.y, tid = threadIdx.x;
  const int a = p.sel[g];
  if (a < 0 || a >= p.n_adapters) return;                    // base row (uniform per workgroup): delta[g] is not written
  const int SR = p.S * p.R;
  for (int i = tid; i < SR; i += 256) ts[i] = p.t[(size_t)g * SR + i];
  __syncthreads();
  const int n = blockIdx.x * 256 + tid;
  if (n >= p.N) return;
  const int s = min(max(p.seg[n >> 4], 0), p.S - 1);
  const unsigned short* b = p.B + ((size_t)a * p.N + n) * (size_t)p.R;
  const float* tr = ts + s * p.R;
  float acc = 0.f;
  for (int j8 = 0; j8 < p.R; j8 += 8) {
    const u32x4_t w = *(const u32x4_t*)(b + j8);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc = fmaf(TT::to_f32(w[e] & 0xffff), tr[j8 + 2 * e], acc);
      acc = fmaf(TT::to_f32(w[e] >> 16), tr[j8 + 2 * e + 1], acc);
    }
  }
  p.delta[(size_t)g * p.N + n] = p.scale[a] * acc;
}

// sx_rmsnorm_planes with the row's gamma picked from a table: the body is the one of rmsnorm_planes_kernel (precise_rows.h).
template <typename TT>
__global__ __launch_bounds__(256) void rmsnorm_planes_sel_kernel(const float* x, const float* gamma, const float* table, const int* sel,
                                                                 int n_adapters, float* y32, unsigned short* out, int cols, float eps, int tiled) {
  __shared__ float red[4];
  const int row = blockIdx.x, a = sel[row];
  const float* gm = (a >= 0 && a < n_adapters) ? table + (size_t)a * cols : gamma;
  sxk_precise::rmsnorm_planes_row<TT>(x, gm, y32, out, cols, eps, tiled, row, red);
}

}  // namespace sxk_lora

using namespace sxk_lora;

#define ST ((hipStream_t)stream)
#define AL16(p) ((((uintptr_t)(p)) & 15) == 0)

extern "C" int sx_lora_shrink(const void* x, const void* A, const int32_t* sel, float* t, int M, int K, int SR, int n_adapters, int dtype,
                              void* stream) {
  SX_CHECK(x && A && sel && t, "sx_lora_shrink: null pointer");
  const int tiled = (dtype & SX_TILED16) ? (M + 15) / 16 : 0, dt = dtype & 0xff;
  SX_CHECK(dt == SX_F16 || dt == SX_BF16, "sx_lora_shrink: dtype");
  SX_CHECK(M >= 1 && M <= 65535 && n_adapters >= 1 && K >= 8 && K % 8 == 0 && SR >= 4 && SR % 4 == 0 && AL16(x) && AL16(A) && AL16(t),
           "sx_lora_shrink: M=%d K=%d S*R=%d n_adapters=%d (K %% 8, S*R %% 4, 16-B aligned pointers)", M, K, SR, n_adapters);
  SX_CHECK(!tiled || (M <= 32 && K % 32 == 0), "sx_lora_shrink: operand tiles hold <= 32 rows of K %% 32 == 0");
  ShrinkP p;
  p.x = (const unsigned short*)x; p.A = (const unsigned short*)A; p.sel = sel; p.t = t;
  p.K = K; p.SR = SR; p.n_adapters = n_adapters; p.tiled = tiled;
  const dim3 grid((SR + 15) / 16, M);
  if (dt == SX_BF16) hipLaunchKernelGGL(lora_shrink_kernel<BF16>, grid, dim3(256), 0, ST, p);
  else hipLaunchKernelGGL(lora_shrink_kernel<F16>, grid, dim3(256), 0, ST, p);
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}

extern "C" int sx_lora_expand(const float* t, const void* B, const int32_t* seg, const float* scale, const int32_t* sel, float* delta, int M,
                              int N, int R, int S, int n_adapters, int dtype, void* stream) {
  SX_CHECK(t && B && seg && scale && sel && delta, "sx_lora_expand: null pointer");
  SX_CHECK(dtype == SX_F16 || dtype == SX_BF16, "sx_lora_expand: dtype");
  SX_CHECK(M >= 1 && M <= 65535 && n_adapters >= 1 && N >= 16 && N % 16 == 0 && R >= 8 && R % 8 == 0 && S >= 1 && S * R <= SX_LORA_MAX_SR &&
               AL16(B),
           "sx_lora_expand: M=%d N=%d R=%d S=%d n_adapters=%d (N %% 16, R %% 8, S*R <= %d, 16-B aligned B)", M, N, R, S, n_adapters,
           SX_LORA_MAX_SR);
  ExpandP p;
  p.t = t; p.B = (const unsigned short*)B; p.seg = seg; p.scale = scale; p.sel = sel; p.delta = delta;
  p.N = N; p.R = R; p.S = S; p.n_adapters = n_adapters;
  const dim3 grid((N + 255) / 256, M);
  if (dtype == SX_BF16) hipLaunchKernelGGL(lora_expand_kernel<BF16>, grid, dim3(256), 0, ST, p);
  else hipLaunchKernelGGL(lora_expand_kernel<F16>, grid, dim3(256), 0, ST, p);
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}

extern "C" int sx_rmsnorm_planes_sel(const float* x, const float* gamma, const float* gamma_table, const int32_t* sel, int n_adapters,
                                     float* y32, void* out16, int rows, int cols, float eps, int dtype, void* stream) {
  SX_CHECK(x && gamma && sel && (y32 || out16), "sx_rmsnorm_planes_sel: null pointer");
  SX_CHECK(n_adapters >= 0 && (n_adapters == 0 || gamma_table), "sx_rmsnorm_planes_sel: n_adapters=%d needs gamma_table", n_adapters);
  const int tiled = (dtype & SX_TILED16) ? (rows + 15) / 16 : 0, dt = dtype & 0xff;
  SX_CHECK(dt == SX_F16 || dt == SX_BF16, "sx_rmsnorm_planes_sel: dtype");
  SX_CHECK(rows >= 1 && cols >= 8 && cols % 8 == 0 && AL16(x) && AL16(gamma) && AL16(gamma_table),
           "sx_rmsnorm_planes_sel: rows=%d cols=%d (cols %% 8, 16-B aligned)", rows, cols);
  SX_CHECK(!tiled || !out16 || (rows <= 32 && cols % 32 == 0), "sx_rmsnorm_planes_sel: operand tiles hold <= 32 rows of cols %% 32 == 0");
  if (dt == SX_BF16)
    hipLaunchKernelGGL(rmsnorm_planes_sel_kernel<BF16>, dim3(rows), dim3(256), 0, ST, x, gamma, gamma_table, sel, n_adapters, y32,
                       (unsigned short*)out16, cols, eps, tiled);
  else
    hipLaunchKernelGGL(rmsnorm_planes_sel_kernel<F16>, dim3(rows), dim3(256), 0, ST, x, gamma, gamma_table, sel, n_adapters, y32,
                       (unsigned short*)out16, cols, eps, tiled);
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}
