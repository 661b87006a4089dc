// Row helpers of the fp32-grade Llama activations shared by csrc/precise.hip and csrc/lora.hip: the hi + lo plane split, the plane
// stores and the body of LlamaRMSNorm. One definition, so that sx_rmsnorm_planes_sel (per-row gamma) runs the very instructions of
// sx_rmsnorm_planes on the gamma it selected. Both translation units are compiled WITHOUT -ffast-math (csrc/build.sh).
#pragma once
#include "sx_common.h"
#include <type_traits>

namespace sxk_precise {

// hi saturates at the largest finite fp16 (a value beyond 65504 would round to inf and make lo = -inf): the remainder then travels in lo, so
// the pair stays exact-ish up to 2 x 65504 — real Llama checkpoints have "massive activation" channels in the thousands, not beyond. bf16 has
// the fp32 exponent range: the clamp never binds there.
template <typename TT>
__device__ __forceinline__ void split1(float x, unsigned short& hi, unsigned short& lo) {
  hi = TT::from_f32(std::is_same<TT, F16>::value ? __builtin_amdgcn_fmed3f(x, -65504.f, 65504.f) : x);
  lo = TT::from_f32(x - TT::to_f32(hi));
}

// 8 consecutive columns c8 .. c8+7 of activation row `row` → the two planes.
//   tiled == 0: out[row][2*cols] = [hi(cols) | lo(cols)]                                   (A operand of sx_gemm, a_planes = 2)
//   tiled == nrb >= 1: operand tiles [2 planes][nrb row blocks][cols/32][16][32], hi plane first, row < 16 nrb (x operand of sx_gemv,
//                      x_planes = 2; nrb = 1: <= 16 rows, nrb = 2 (round 6): 17..32 lock-step sequences)
template <typename TT>
__device__ __forceinline__ void store_planes8(unsigned short* out, int tiled, int row, int cols, int c8, const float* v) {
  u32x4_t h, l;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    unsigned short h0, l0, h1, l1;
    split1<TT>(v[2 * e], h0, l0);
    split1<TT>(v[2 * e + 1], h1, l1);
    h[e] = (unsigned)h0 | ((unsigned)h1 << 16);
    l[e] = (unsigned)l0 | ((unsigned)l1 << 16);
  }
  if (tiled) {
    unsigned short* b = out + ((size_t)(row >> 4) * (size_t)(cols >> 5) + (size_t)(c8 >> 5)) * 512 + (size_t)(row & 15) * 32 + (c8 & 31);
    *(u32x4_t*)b = h;
    *(u32x4_t*)(b + (size_t)cols * 16 * (size_t)tiled) = l;
  } else {
    unsigned short* b = out + (size_t)row * 2 * cols + c8;
    *(u32x4_t*)b = h;
    *(u32x4_t*)(b + cols) = l;
  }
}

// LlamaRMSNorm (modeling_llama_xformer.py:95 → transformers 4.30.2: w * (x * rsqrt(mean(x^2) + eps)), fp32) of ONE row by a 256-thread
// workgroup. Outputs: y32 (fp32, optional: the final norm's hidden states) and / or the two operand planes. `gamma` is the row's own.
template <typename TT>
__device__ __forceinline__ void rmsnorm_planes_row(const float* x, const float* gamma, float* y32, unsigned short* out, int cols, float eps,
                                                   int tiled, int row, float* red) {
  const int tid = threadIdx.x;
  const float* xr = x + (size_t)row * cols;
  float ss = 0.f;
  for (int c8 = tid * 8; c8 < cols; c8 += 2048) {
    const f32x4_t a = *(const f32x4_t*)(xr + c8), b = *(const f32x4_t*)(xr + c8 + 4);
    ss += (a[0] * a[0] + a[1] * a[1]) + (a[2] * a[2] + a[3] * a[3]) + (b[0] * b[0] + b[1] * b[1]) + (b[2] * b[2] + b[3] * b[3]);
  }
  ss = wave_sum(ss);
  if ((tid & 63) == 0) red[tid >> 6] = ss;
  __syncthreads();
  const float tot = (red[0] + red[1]) + (red[2] + red[3]);
  const float rstd = 1.0f / sqrtf(tot / (float)cols + eps);
  for (int c8 = tid * 8; c8 < cols; c8 += 2048) {
    const f32x4_t a = *(const f32x4_t*)(xr + c8), b = *(const f32x4_t*)(xr + c8 + 4);
    const f32x4_t g0 = *(const f32x4_t*)(gamma + c8), g1 = *(const f32x4_t*)(gamma + c8 + 4);
    float v[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = g0[e] * (a[e] * rstd);
      v[4 + e] = g1[e] * (b[e] * rstd);
    }
    if (y32) {
      *(f32x4_t*)(y32 + (size_t)row * cols + c8) = (f32x4_t){v[0], v[1], v[2], v[3]};
      *(f32x4_t*)(y32 + (size_t)row * cols + c8 + 4) = (f32x4_t){v[4], v[5], v[6], v[7]};
    }
    if (out) store_planes8<TT>(out, tiled, row, cols, c8, v);
  }
}

}  // namespace sxk_precise
