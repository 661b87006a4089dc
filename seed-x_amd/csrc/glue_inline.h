// Inline device functions shared by elementwise.hip and denoise_slots.hip: the lock-step kernels (timestep_embedding_kernel,
// cfg_euler_kernel, cfg_dpmpp2m_kernel) and their per-slot forms are compiled from ONE body each, so a slot's result is the lock-step
// kernel's bit for bit.
#pragma once
#include "sx_common.h"

namespace sxk_glue {

__device__ __forceinline__ float ld_as_f32(const void* p, int dt, int64_t i) {
  if (dt == SX_F32) return ((const float*)p)[i];
  const unsigned short u = ((const unsigned short*)p)[i];
  return dt == SX_BF16 ? BF16::to_f32(u) : F16::to_f32(u);
}
__device__ __forceinline__ void st_from_f32(void* p, int dt, int64_t i, float v) {
  if (dt == SX_F32) ((float*)p)[i] = v;
  else ((unsigned short*)p)[i] = dt == SX_BF16 ? BF16::from_f32(v) : F16::from_f32(v);
}

// one (row, frequency) pair of the sinusoidal embedding: shared by the lock-step and the per-slot kernel, so a slot's row is the
// lock-step kernel's row of the same t bit for bit
template <typename LoadT>
__device__ __forceinline__ void timestep_embedding_pair(void* out, int dt, int dim, int half, int r, int j, LoadT load_t) {
  const float f = expf(-9.210340371976184f * (float)j / (float)half);  // ln(10000)
  const float a = load_t() * f;
  st_from_f32(out, dt, (int64_t)r * dim + j, cosf(a));          // flip_sin_to_cos: cos first
  st_from_f32(out, dt, (int64_t)r * dim + half + j, sinf(a));
}

// CFG + Euler update of element i of ONE generation (n elements, NHWC [HW][C]): eps / scaled_next point at the generation's rows of
// branch 0, branch k lies eps_bs elements (eps_bs / C pixel rows) further. Shared by the lock-step and the per-slot kernel.
__device__ __forceinline__ void cfg_euler_elem(const float* eps, float* lat, float* scaled_next, int64_t i, int64_t eps_bs, int nb, int C,
                                               int ld, float gs, float igs, int mode, float sigma, float sigma_next, float inv_next) {
  const float x = lat[i];
  float e;
  if (mode == 0) {
    const float eu = eps[i], et = eps[eps_bs + i];
    e = eu + gs * (et - eu);
  } else {
    const float x0t = x - sigma * eps[i], x0i = x - sigma * eps[eps_bs + i], x0u = x - sigma * eps[2 * eps_bs + i];
    const float x0 = x0u + gs * (x0t - x0i) + igs * (x0i - x0u);
    e = (x0 - x) / (-sigma);
  }
  const float xn = x + e * (sigma_next - sigma);
  lat[i] = xn;
  if (scaled_next) {
    const float sv = xn * inv_next;
    const int64_t hw = i / C;
    const int c = (int)(i - hw * C);
    const int64_t HW = eps_bs / C;
    for (int k = 0; k < nb; ++k) scaled_next[((int64_t)k * HW + hw) * ld + c] = sv;
  }
}

// CFG + DPM-Solver++(2M) update of element i of ONE generation, laid out as cfg_euler_elem's: x0 the guided denoised sample,
// d = x0 + c (x0 - x0_prev), x' = a x + b d, x0_prev <- x0. (a, b, c) is the step's row of the host table (seedx_amd/solvers.py): no
// logarithm or exponential here. c == 0 (step 0, and the step onto sigma_next = 0) is the same in every lane and skips the read of
// x0_prev, so whatever the buffer holds before step 0 is harmless. Shared by the lock-step and the per-slot kernel.
__device__ __forceinline__ void cfg_dpmpp2m_elem(const float* eps, float* lat, float* x0_prev, float* scaled_next, int64_t i,
                                                 int64_t eps_bs, int nb, int C, int ld, float gs, float igs, int mode, float sigma, float a,
                                                 float b, float c, float inv_next) {
  const float x = lat[i];
  float x0;
  if (mode == 0) {
    const float eu = eps[i], et = eps[eps_bs + i];
    const float e = eu + gs * (et - eu);
    x0 = x - sigma * e;
  } else {
    const float x0t = x - sigma * eps[i], x0i = x - sigma * eps[eps_bs + i], x0u = x - sigma * eps[2 * eps_bs + i];
    x0 = x0u + gs * (x0t - x0i) + igs * (x0i - x0u);
  }
  float d = x0;
  if (c != 0.0f) d = x0 + c * (x0 - x0_prev[i]);
  const float xn = a * x + b * d;
  lat[i] = xn;
  x0_prev[i] = x0;
  if (scaled_next) {
    const float sv = xn * inv_next;
    const int64_t hw = i / C;
    const int ch = (int)(i - hw * C);
    const int64_t HW = eps_bs / C;
    for (int k = 0; k < nb; ++k) scaled_next[((int64_t)k * HW + hw) * ld + ch] = sv;
  }
}

}  // namespace sxk_glue
