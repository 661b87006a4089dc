// Per-slot forms of the denoise-step glue kernels (in-flight batching of the de-tokenizer): G generations ("slots") share one captured
// UNet step, rows ordered [branch][slot]; every slot has its own step counter, sigma / timestep table and guidance scales in device
// memory. A slot is LIVE when 0 <= step[g] < n_steps[g], PARKED otherwise (step -1). The arithmetic is glue_inline.h's, shared with
// elementwise.hip's lock-step kernels. The DPM-Solver++(2M) step lives here in both forms, lock-step and per-slot.
#include "sx_common.h"
#include "glue_inline.h"

namespace sxk_denoise_slots {
using namespace sxk_glue;

inline dim3 grid_for(int64_t n) {
  int64_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  return dim3((unsigned)blocks);
}

// rows ordered [branch][slot]: row k*G + g embeds t_tab[g][step[g]]; a slot whose step is outside [0, ld_t) (parked: -1) embeds t = 0
__global__ void timestep_embedding_slots_kernel(const float* t_tab, int ld_t, const int* step_dev, void* out, int G, int nb, int dim,
                                                int dt) {
  const int half = dim / 2;
  const int total = nb * G * half;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int j = i % half, r = i / half;
    const int g = r % G;
    const int step = step_dev[g];
    timestep_embedding_pair(out, dt, dim, half, r, j,
                            [&]() { return (step >= 0 && step < ld_t) ? t_tab[(int64_t)g * ld_t + step] : 0.0f; });
  }
}

// G generations ("slots") of one UNet batch ordered [branch][slot], each with its own step counter, sigma table and guidance scales in
// device memory. blockIdx.y = slot. A slot is live when 0 <= step[g] < n_steps[g]; a parked slot's workgroups leave without a store.
// step and step + 1 are clamped into the table row.
__global__ void cfg_euler_slots_kernel(const float* eps, float* lat, float* scaled_next, const float* sig_tab, int ld_sig,
                                       const int* step_dev, const int* n_steps_dev, const float* gs_dev, const float* igs_dev, int nb,
                                       int G, int64_t n, int C, int ld, int mode) {
  const int g = blockIdx.y;
  const int step = step_dev[g];
  if (step < 0 || step >= n_steps_dev[g]) return;
  const int s0 = step < ld_sig ? step : ld_sig - 1, s1 = step + 1 < ld_sig ? step + 1 : ld_sig - 1;
  const float sigma = sig_tab[(int64_t)g * ld_sig + s0], sigma_next = sig_tab[(int64_t)g * ld_sig + s1];
  const float inv_next = rsqrtf(sigma_next * sigma_next + 1.0f);
  const float gs = gs_dev[g], igs = igs_dev[g];
  const int64_t scaled_slot = n / C * ld;                               // elements of one slot's rows of scaled_next
  const float* eps_g = eps + (int64_t)g * n;
  float* lat_g = lat + (int64_t)g * n;
  float* scaled_g = scaled_next ? scaled_next + (int64_t)g * scaled_slot : nullptr;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    cfg_euler_elem(eps_g, lat_g, scaled_g, i, (int64_t)G * n, nb, C, ld, gs, igs, mode, sigma, sigma_next, inv_next);
}

// The second-order multistep step (DPM-Solver++(2M), seedx_amd/solvers.py), lock-step form: cfg_euler_kernel's layout with the step's
// (a, b, c) read from the host-made table coef [steps][3] and the previous denoised sample kept in x0_prev. The kernel knows no table
// length: a negative step reads row 0, the upper end is the caller's, as for cfg_euler_kernel.
__global__ void cfg_dpmpp2m_kernel(const float* eps, float* lat, float* x0_prev, float* scaled_next, const float* sigmas, const float* coef,
                                   const int* step_dev, int nb, int64_t n, int C, int ld, float gs, float igs, int mode) {
  const int step = *step_dev > 0 ? *step_dev : 0;
  const float sigma = sigmas[step], sigma_next = sigmas[step + 1];
  const float a = coef[3 * (int64_t)step], b = coef[3 * (int64_t)step + 1], c = coef[3 * (int64_t)step + 2];
  const float inv_next = rsqrtf(sigma_next * sigma_next + 1.0f);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    cfg_dpmpp2m_elem(eps, lat, x0_prev, scaled_next, i, n, nb, C, ld, gs, igs, mode, sigma, a, b, c, inv_next);
}

// per-slot form, cfg_euler_slots_kernel's frame: blockIdx.y = slot, a parked slot's workgroups leave without a store (latents, x0_prev
// and scaled_next alike); step and step + 1 are clamped into the slot's table rows (sig_tab [G][ld_sig], coef_tab [G][ld_sig][3])
__global__ void cfg_dpmpp2m_slots_kernel(const float* eps, float* lat, float* x0_prev, float* scaled_next, const float* sig_tab,
                                         const float* coef_tab, int ld_sig, const int* step_dev, const int* n_steps_dev, const float* gs_dev,
                                         const float* igs_dev, int nb, int G, int64_t n, int C, int ld, int mode) {
  const int g = blockIdx.y;
  const int step = step_dev[g];
  if (step < 0 || step >= n_steps_dev[g]) return;
  const int s0 = step < ld_sig ? step : ld_sig - 1, s1 = step + 1 < ld_sig ? step + 1 : ld_sig - 1;
  const float sigma = sig_tab[(int64_t)g * ld_sig + s0], sigma_next = sig_tab[(int64_t)g * ld_sig + s1];
  const float* co = coef_tab + ((int64_t)g * ld_sig + s0) * 3;
  const float a = co[0], b = co[1], c = co[2];
  const float inv_next = rsqrtf(sigma_next * sigma_next + 1.0f);
  const float gs = gs_dev[g], igs = igs_dev[g];
  const int64_t scaled_slot = n / C * ld;                               // elements of one slot's rows of scaled_next
  const float* eps_g = eps + (int64_t)g * n;
  float* lat_g = lat + (int64_t)g * n;
  float* old_g = x0_prev + (int64_t)g * n;
  float* scaled_g = scaled_next ? scaled_next + (int64_t)g * scaled_slot : nullptr;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    cfg_dpmpp2m_elem(eps_g, lat_g, old_g, scaled_g, i, (int64_t)G * n, nb, C, ld, gs, igs, mode, sigma, a, b, c, inv_next);
}

// last node of a slot step: a live slot's counter moves on, and parks itself (-1) at the end of its schedule
__global__ void denoise_advance_kernel(int* step_dev, const int* n_steps_dev, int G) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const int step = step_dev[g];
  const int next = (step >= 0 && step < n_steps_dev[g]) ? step + 1 : -1;
  step_dev[g] = (next >= 0 && next < n_steps_dev[g]) ? next : -1;
}

}  // namespace sxk_denoise_slots
using namespace sxk_denoise_slots;

#define ST ((hipStream_t)stream)

extern "C" int sx_cfg_euler_step_slots(const float* eps, float* latents, float* scaled_next, const float* sig_tab, int ld_sig,
                                       const int32_t* step_dev, const int32_t* n_steps_dev, const float* gs_dev,
                                       const float* igs_dev, int nb, int G, int64_t n_slot, int C, int ld_scaled, int mode,
                                       void* stream) {
  SX_CHECK(eps && latents && sig_tab && step_dev && n_steps_dev && gs_dev && igs_dev, "sx_cfg_euler_step_slots: null pointer");
  SX_CHECK((mode == 0 && nb == 2) || (mode == 1 && nb == 3), "sx_cfg_euler_step_slots: mode/nb mismatch");
  SX_CHECK(C > 0 && n_slot > 0 && n_slot % C == 0 && ld_scaled >= C, "sx_cfg_euler_step_slots: C/ld");
  SX_CHECK(G >= 1 && G <= 65535 && ld_sig >= 2, "sx_cfg_euler_step_slots: G in 1..65535, ld_sig >= 2");
  dim3 grid = grid_for(n_slot);
  grid.y = (unsigned)G;
  hipLaunchKernelGGL(cfg_euler_slots_kernel, grid, dim3(256), 0, ST, eps, latents, scaled_next, sig_tab, ld_sig, step_dev, n_steps_dev,
                     gs_dev, igs_dev, nb, G, n_slot, C, ld_scaled, mode);
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}
extern "C" int sx_cfg_dpmpp2m_step(const float* eps, float* latents, float* x0_prev, float* scaled_next, const float* sigmas_dev,
                                   const float* coef_dev, const int32_t* step_dev, int nb, int64_t n, int C, int ld_scaled, float gs,
                                   float igs, int mode, void* stream) {
  SX_CHECK(eps && latents && x0_prev && sigmas_dev && coef_dev && step_dev, "sx_cfg_dpmpp2m_step: null pointer");
  SX_CHECK((mode == 0 && nb == 2) || (mode == 1 && nb == 3), "sx_cfg_dpmpp2m_step: mode/nb mismatch");
  SX_CHECK(C > 0 && n >= 0 && n % C == 0 && ld_scaled >= C, "sx_cfg_dpmpp2m_step: C/ld");
  if (n == 0) return SX_OK;
  hipLaunchKernelGGL(cfg_dpmpp2m_kernel, grid_for(n), dim3(256), 0, ST, eps, latents, x0_prev, scaled_next, sigmas_dev, coef_dev, step_dev,
                     nb, n, C, ld_scaled, gs, igs, mode);
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}
extern "C" int sx_cfg_dpmpp2m_step_slots(const float* eps, float* latents, float* x0_prev, float* scaled_next, const float* sig_tab,
                                         const float* coef_tab, int ld_sig, const int32_t* step_dev, const int32_t* n_steps_dev,
                                         const float* gs_dev, const float* igs_dev, int nb, int G, int64_t n_slot, int C, int ld_scaled,
                                         int mode, void* stream) {
  SX_CHECK(eps && latents && x0_prev && sig_tab && coef_tab && step_dev && n_steps_dev && gs_dev && igs_dev,
           "sx_cfg_dpmpp2m_step_slots: null pointer");
  SX_CHECK((mode == 0 && nb == 2) || (mode == 1 && nb == 3), "sx_cfg_dpmpp2m_step_slots: mode/nb mismatch");
  SX_CHECK(C > 0 && n_slot > 0 && n_slot % C == 0 && ld_scaled >= C, "sx_cfg_dpmpp2m_step_slots: C/ld");
  SX_CHECK(G >= 1 && G <= 65535 && ld_sig >= 2, "sx_cfg_dpmpp2m_step_slots: G in 1..65535, ld_sig >= 2");
  dim3 grid = grid_for(n_slot);
  grid.y = (unsigned)G;
  hipLaunchKernelGGL(cfg_dpmpp2m_slots_kernel, grid, dim3(256), 0, ST, eps, latents, x0_prev, scaled_next, sig_tab, coef_tab, ld_sig,
                     step_dev, n_steps_dev, gs_dev, igs_dev, nb, G, n_slot, C, ld_scaled, mode);
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}
extern "C" int sx_timestep_embedding_slots(const float* t_tab, int ld_t, const int32_t* step_dev, void* out, int G, int nb, int dim,
                                           int dtype, void* stream) {
  SX_CHECK(t_tab && step_dev && out && dim > 0 && dim % 2 == 0, "sx_timestep_embedding_slots: dim must be even");
  SX_CHECK(G >= 1 && nb >= 1 && ld_t >= 1, "sx_timestep_embedding_slots: G, nb, ld_t >= 1");
  hipLaunchKernelGGL(timestep_embedding_slots_kernel, grid_for((int64_t)nb * G * dim / 2), dim3(256), 0, ST, t_tab, ld_t, step_dev, out,
                     G, nb, dim, dtype);
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}
extern "C" int sx_denoise_advance(int32_t* step_dev, const int32_t* n_steps_dev, int G, void* stream) {
  SX_CHECK(step_dev && n_steps_dev && G >= 1, "sx_denoise_advance: bad args");
  hipLaunchKernelGGL(denoise_advance_kernel, grid_for(G), dim3(256), 0, ST, step_dev, n_steps_dev, G);
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}
