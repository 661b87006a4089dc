// fp32-grade activations for the Llama decoder (LlamaForCausalLM(precise=True)): north_star asks for logits within 1e-3 of the
// reference; at 40 layers one 16-bit rounding per MFMA operand adds up to 2.2e-3 (tools/llm_error_budget.py: RMSNorm output 1.0e-3,
// q / k before and after RoPE 1.2e-3, v, attention output, GLU output 0.3-0.6e-3 each). The weights of a 16-bit checkpoint are exact,
// so only the ACTIVATION side needs more mantissa:
//   * every GEMM A operand travels as two 16-bit planes x = hi + lo (hi = rn16(x), lo = rn16(x - hi)): sx_gemm a_planes = 2 walks
//     K twice over the same weight tiles, sx_gemv x_planes = 2 feeds every weight fragment to two MFMAs — no extra weight bytes;
//   * q, k, v never become 16-bit: the qkv GEMM stores fp32, RoPE runs in fp32 into an fp32 KV cache (rope_kv_f32_kernel), and
//     attention (attn_f32_kernel) is fp32 FMA work — T <= a few hundred keys per head on this path, 1 % of the LLM's FLOPs.
//   * opt-in, lossy: the FP8 (e4m3) KV cache (kv_format="fp8_e4m3") — k after RoPE and v rounded ONCE, at append, to 128 codes + one
//     power-of-two scale per (token, head) row (quant_row8); attention reads the codes and computes, bit for bit, what the fp32 kernels
//     compute on a cache holding the dequantised values (KV8 template arguments below).
// This file holds the kernels that only exist for that mode. It is compiled WITHOUT -ffast-math (csrc/build.sh): x - float(rn16(x))
// and the softmax bookkeeping must not be re-associated.
// Reference being matched: modeling_llama_xformer.py:95 (RMSNorm), :141-149 (RoPE), :204-239 (attention), run by the fp32 oracle.
#include "sx_common.h"
#include "precise_rows.h"   // split1, store_planes8, rmsnorm_planes_row (shared with csrc/lora.hip)
#include <type_traits>

namespace sxk_precise {

template <typename TT>
__global__ __launch_bounds__(256) void split16_kernel(const float* x, long long ldx, unsigned short* out, int rows, int cols, int tiled) {
  const int cpr = cols >> 3;
  const long long total = (long long)rows * cpr;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int row = (int)(i / cpr), c8 = (int)(i - (long long)row * cpr) * 8;
    const float* src = x + (size_t)row * ldx + c8;
    const f32x4_t a = *(const f32x4_t*)src, b = *(const f32x4_t*)(src + 4);
    const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    store_planes8<TT>(out, tiled, row, cols, c8, v);
  }
}

// LlamaRMSNorm (modeling_llama_xformer.py:95 → transformers 4.30.2: w * (x * rsqrt(mean(x^2) + eps)), fp32). One workgroup per row.
// Outputs: y32 (fp32, optional: the final norm's hidden states) and / or the two operand planes.
template <typename TT>
__global__ __launch_bounds__(256) void rmsnorm_planes_kernel(const float* x, const float* gamma, float* y32, unsigned short* out, int cols,
                                                             float eps, int tiled) {
  __shared__ float red[4];
  rmsnorm_planes_row<TT>(x, gamma, y32, out, cols, eps, tiled, blockIdx.x, red);
}

// RoPE (modeling_llama_xformer.py:141-149) of the q and k heads of fp32 qkv rows [G*T][3*H*D] (q rotated in place) + append of the
// rotated k and of v to the fp32 caches [G][H][Tmax][D] at position pos0[g] + t. The tables are rounded to the model dtype first
// (:128-131 casts them to x.dtype), the products stay fp32.
// V16 (round 6, the "mixed" cache): v is appended in the model's 16-bit dtype (vc = 16-bit [G][H][Tmax][D], same ELEMENT strides) —
// k stays fp32: the score noise of a rounded k goes through the softmax (tools/llm_error_budget.py: q / k 1.2e-3 of the 2.2e-3 at 40
// layers, v 0.6e-3), while a rounded v only perturbs the weighted average. Three quarters of the fp32 cache's bytes.
template <typename TT, bool V16>
__global__ void rope_kv_f32_kernel(float* qkv, float* kc, void* vc_, const float* cos_t, const float* sin_t, const int* pos0_dev, int T,
                                   int H, int D, int Tmax, int G, long long seq_stride) {
  const int half = D / 2;
  const int64_t total = (int64_t)G * T * H * half;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(i % half);
    const int h = (int)((i / half) % H);
    const int r = (int)(i / ((int64_t)half * H));
    const int g = r / T, t = r - g * T;
    int pos = pos0_dev[g] + t;
    const bool pos_ok = pos >= 0 && pos < Tmax;
    if (!pos_ok) pos = 0;
    const float c = TT::to_f32(TT::from_f32(cos_t[(size_t)pos * half + j]));
    const float s = TT::to_f32(TT::from_f32(sin_t[(size_t)pos * half + j]));
    float* row = qkv + (size_t)r * 3 * H * D;
    float* qh = row + (size_t)h * D;
    const float* kh = row + (size_t)(H + h) * D;
    const float* vh = row + (size_t)(2 * H + h) * D;
    const float q1 = qh[j], q2 = qh[j + half];
    qh[j] = q1 * c - q2 * s;
    qh[j + half] = q2 * c + q1 * s;
    if (!pos_ok) continue;                  // a device-resident position past the cache never writes outside it
    const float k1 = kh[j], k2 = kh[j + half];
    float* kd = kc + (size_t)g * seq_stride + ((size_t)h * Tmax + pos) * D;
    kd[j] = k1 * c - k2 * s;
    kd[j + half] = k2 * c + k1 * s;
    const size_t vo = (size_t)g * seq_stride + ((size_t)h * Tmax + pos) * D;
    if constexpr (V16) {
      unsigned short* vd = (unsigned short*)vc_ + vo;
      vd[j] = TT::from_f32(vh[j]);
      vd[j + half] = TT::from_f32(vh[j + half]);
    } else {
      float* vd = (float*)vc_ + vo;
      vd[j] = vh[j];
      vd[j + half] = vh[j + half];
    }
  }
}

// rope_kv_f32_kernel on the paged cache (LlamaForCausalLM(kv_pages=N)) — a kernel of its own, its statements copied, so that the contiguous
// kernel above keeps its signature and its code to the instruction: kc / vc are page pools [n_pages + 1][H][page size][D], page_stride
// elements between pages, and ptab int32 [G][ptw] names the page that holds key rows [i << pshift, (i + 1) << pshift) of sequence g. Page 0 is
// the null page: a row whose entry is 0 is not appended (q is still rotated). The entry is clamped to [0, npages]: a wrong table never gives
// a wild address.
template <typename TT, bool V16>
__global__ void rope_kv_f32_paged_kernel(float* qkv, float* kc, void* vc_, const float* cos_t, const float* sin_t, const int* pos0_dev, int T,
                                         int H, int D, int Tmax, int G, long long page_stride, const int* ptab, int pshift, int npages,
                                         int ptw) {
  const int half = D / 2;
  const int64_t total = (int64_t)G * T * H * half;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(i % half);
    const int h = (int)((i / half) % H);
    const int r = (int)(i / ((int64_t)half * H));
    const int g = r / T, t = r - g * T;
    int pos = pos0_dev[g] + t;
    const bool pos_ok = pos >= 0 && pos < Tmax;
    if (!pos_ok) pos = 0;
    const float c = TT::to_f32(TT::from_f32(cos_t[(size_t)pos * half + j]));
    const float s = TT::to_f32(TT::from_f32(sin_t[(size_t)pos * half + j]));
    float* row = qkv + (size_t)r * 3 * H * D;
    float* qh = row + (size_t)h * D;
    const float* kh = row + (size_t)(H + h) * D;
    const float* vh = row + (size_t)(2 * H + h) * D;
    const float q1 = qh[j], q2 = qh[j + half];
    qh[j] = q1 * c - q2 * s;
    qh[j + half] = q2 * c + q1 * s;
    if (!pos_ok) continue;                  // a device-resident position past the cache never writes outside it
    const int pg = min(max(ptab[(size_t)g * ptw + (pos >> pshift)], 0), npages);
    if (pg == 0) continue;                  // no reservation behind this row: nothing is written
    const size_t vo = (size_t)pg * page_stride + (((size_t)h << pshift) + (pos & ((1 << pshift) - 1))) * D;   // the row's place in its page
    const float k1 = kh[j], k2 = kh[j + half];
    float* kd = kc + vo;
    kd[j] = k1 * c - k2 * s;
    kd[j + half] = k2 * c + k1 * s;
    if constexpr (V16) {
      unsigned short* vd = (unsigned short*)vc_ + vo;
      vd[j] = TT::from_f32(vh[j]);
      vd[j + half] = TT::from_f32(vh[j + half]);
    } else {
      float* vd = (float*)vc_ + vo;
      vd[j] = vh[j];
      vd[j + half] = vh[j + half];
    }
  }
}

// ---- FP8 (e4m3fn) KV cache: LlamaForCausalLM(kv_format="fp8_e4m3") -----------------------------------------------------------------
// The ONE quantiser of every append path (quant.py quantize_kv_rows is its host statement). A 16-lane group owns a row of D = 128 values,
// lane dl the dims 8 dl .. 8 dl + 7 (the mapping of attn_f32_kernel's fused RoPE block). Row amax by four xor shuffles; s = ceil(log2(amax
// / 448)) from the float's exponent and mantissa bits, clamped to [-64, 64], 0 for a zero row; x · 2^-s is exact; clamp to +-448;
// v_cvt_pk_fp8_f32 rounds to nearest even (gfx950 FP8 is OCP e4m3fn). Returns the lane's 8 codes and the row's 2^s.
__device__ __forceinline__ void quant_row8(const float (&x)[8], u32x2_t& codes, float& scale) {
  float am = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) am = fmaxf(am, fabsf(x[e]));
  am = fmaxf(am, __shfl_xor(am, 1, 64));
  am = fmaxf(am, __shfl_xor(am, 2, 64));
  am = fmaxf(am, __shfl_xor(am, 4, 64));
  am = fmaxf(am, __shfl_xor(am, 8, 64));
  const unsigned bits = __float_as_uint(am);
  int s = (int)((bits >> 23) & 0xffu) - 127 - 8 + ((bits & 0x7fffffu) > 0x600000u ? 1 : 0);
  s = min(64, max(-64, s));
  if (am == 0.f) s = 0;
  const float inv = __uint_as_float((unsigned)(127 - s) << 23);
  scale = __uint_as_float((unsigned)(127 + s) << 23);
  float y[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) y[e] = __builtin_amdgcn_fmed3f(x[e] * inv, -448.f, 448.f);
#if defined(__HIP_DEVICE_COMPILE__)
  int w0 = 0, w1 = 0;
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], w0, false);
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], w0, true);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], w1, false);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], w1, true);
  codes[0] = (unsigned)w0;
  codes[1] = (unsigned)w1;
#endif
}

// 8 e4m3fn codes → their fp32 values (exact)
__device__ __forceinline__ void decode8(const u32x2_t w, float* f) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
    const auto b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    f[4 * i] = a[0]; f[4 * i + 1] = a[1]; f[4 * i + 2] = b[0]; f[4 * i + 3] = b[1];
  }
#endif
}

// quant_row8, and x REPLACED by the dequantised values decode(code) · 2^s (exact): what the cache will give back, so a value attended to
// from registers equals the one read later
__device__ __forceinline__ void quant_dequant_row8(float (&x)[8], u32x2_t& codes, float& scale) {
  quant_row8(x, codes, scale);
  decode8(codes, x);
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] *= scale;
}

// rope_kv_f32_kernel with the FP8 cache (D = 128): one 16-lane group per (sequence, token, head) row. q is rotated in place; the rotated
// k row and the v row are quantised and appended as codes [G][H][Tmax][128] + one fp32 scale per row [G][H][Tmax] (EMUL: as their
// dequantised fp32 values into fp32 caches, the bit-reference twin). A position outside [0, Tmax) writes nothing.
template <typename TT, bool EMUL>
__global__ __launch_bounds__(256) void rope_kv_q8_kernel(float* qkv, void* kc_, void* vc_, float* ks, float* vs, const float* cos_t,
                                                         const float* sin_t, const int* pos0_dev, int T, int H, int Tmax, int G,
                                                         long long seq_stride, long long sc_seq_stride) {
  constexpr int D = 128, half = 64;
  const long long rows = (long long)G * T * H;
  const int dl = threadIdx.x & 15;
  const long long r_ = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool valid = r_ < rows;                       // uniform over the 16-lane group
  const long long rr = valid ? r_ : rows - 1;
  const int h = (int)(rr % H);
  const long long r = rr / H;                         // qkv row = g*T + t
  const int g = (int)(r / T), t = (int)(r - (long long)g * T);
  const int praw = pos0_dev[g] + t;
  const bool pos_ok = praw >= 0 && praw < Tmax;
  const int pt = pos_ok ? praw : 0;
  const int jb = (dl & 7) * 8;
  float* row = qkv + (size_t)r * 3 * H * D;
  float* qo = row + (size_t)h * D + dl * 8;
  const float* ko = row + (size_t)(H + h) * D + dl * 8;
  const float* vo = row + (size_t)(2 * H + h) * D + dl * 8;
  const f32x4_t q0 = *(const f32x4_t*)qo, q1 = *(const f32x4_t*)(qo + 4);
  const f32x4_t k0 = *(const f32x4_t*)ko, k1 = *(const f32x4_t*)(ko + 4);
  const f32x4_t v0 = *(const f32x4_t*)vo, v1 = *(const f32x4_t*)(vo + 4);
  const float qa[8] = {q0[0], q0[1], q0[2], q0[3], q1[0], q1[1], q1[2], q1[3]};
  const float ka[8] = {k0[0], k0[1], k0[2], k0[3], k1[0], k1[1], k1[2], k1[3]};
  float va[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
  const float sg = (dl < 8) ? -1.0f : 1.0f;           // first half: x1 c - x2 s; second half: x2 c + x1 s
  float qr[8], kr[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float c = TT::to_f32(TT::from_f32(cos_t[(size_t)pt * half + jb + e]));
    const float s = TT::to_f32(TT::from_f32(sin_t[(size_t)pt * half + jb + e]));
    const float qp = __shfl_xor(qa[e], 8, 64), kp = __shfl_xor(ka[e], 8, 64);   // the rotation partner's dims: lane dl ^ 8
    qr[e] = qa[e] * c + sg * (qp * s);
    kr[e] = ka[e] * c + sg * (kp * s);
  }
  u32x2_t kcod, vcod;
  float ksc, vsc;
  quant_dequant_row8(kr, kcod, ksc);
  quant_dequant_row8(va, vcod, vsc);
  if (!valid) return;
  *(f32x4_t*)qo = (f32x4_t){qr[0], qr[1], qr[2], qr[3]};
  *(f32x4_t*)(qo + 4) = (f32x4_t){qr[4], qr[5], qr[6], qr[7]};
  if (!pos_ok) return;                                // a device-resident position past the cache never writes outside it
  const size_t ro = (size_t)g * seq_stride + ((size_t)h * Tmax + praw) * D + dl * 8;
  if constexpr (EMUL) {
    float* kd = (float*)kc_ + ro;
    float* vd = (float*)vc_ + ro;
    *(f32x4_t*)kd = (f32x4_t){kr[0], kr[1], kr[2], kr[3]};
    *(f32x4_t*)(kd + 4) = (f32x4_t){kr[4], kr[5], kr[6], kr[7]};
    *(f32x4_t*)vd = (f32x4_t){va[0], va[1], va[2], va[3]};
    *(f32x4_t*)(vd + 4) = (f32x4_t){va[4], va[5], va[6], va[7]};
  } else {
    *(u32x2_t*)((unsigned char*)kc_ + ro) = kcod;
    *(u32x2_t*)((unsigned char*)vc_ + ro) = vcod;
    if (dl == 0) {
      const size_t so = (size_t)g * sc_seq_stride + (size_t)h * Tmax + praw;
      ks[so] = ksc;
      vs[so] = vsc;
    }
  }
}

// ---- device code shared by attn_f32_kernel and attn_f32_verify_kernel: the verify form must give the bits of T successive fused T = 1
// launches, so the rotation expression, the score, the per-key update and the group / wave merges exist once ---------------------------
// x1 c - x2 s (sg = -1, first half of the head) or x2 c + x1 s (sg = +1): xp is the rotation partner's value
__device__ __forceinline__ float rope_rot(float x, float xp, float c, float s, float sg) { return x * c + sg * (xp * s); }

// rope_rot as attn_f32_kernel<.., QB = 1, DC = 1, ..> compiles it, spelled out: the compiler contracts the expression differently at its two
// uses there, the same way in all its T = 1 instantiations (their gfx950 code: q is v_pk_mul (x c), v_pk_mul (xp s), v_pk_fma (sg, xp s,
// x c); k is v_pk_mul (xp s), v_pk_mul (sg, ·), v_pk_fma (x, c, ·)). A new instantiation is free to contract otherwise, so the verify
// kernel, which owes the T = 1 launch's bits, uses these two.
__device__ __forceinline__ float rope_rot_q_t1(float x, float xp, float c, float s, float sg) { return __builtin_fmaf(sg, xp * s, x * c); }
__device__ __forceinline__ float rope_rot_k_t1(float x, float xp, float c, float s, float sg) { return __builtin_fmaf(x, c, sg * (xp * s)); }

// q · k of one key row: the lane's DW dims in one fma chain, then the 16 lanes of the group by four xor butterflies
template <int DW>
__device__ __forceinline__ float attn_score(const float (&kf)[DW], const float (&qv)[DW]) {
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < DW; ++e) s = fmaf(kf[e], qv[e], s);
  s += __shfl_xor(s, 1, 64);
  s += __shfl_xor(s, 2, 64);
  s += __shfl_xor(s, 4, 64);
  s += __shfl_xor(s, 8, 64);
  return s;
}

// online softmax: one key with score s and value row vf joins the running (max, sum, weighted values) of a query row
template <int DW>
__device__ __forceinline__ void attn_key_update(float s, const float (&vf)[DW], float& m_run, float& l_run, float (&o)[DW]) {
  const float m_new = fmaxf(m_run, s);
  const float alpha = __expf(m_run - m_new);   // exp(-inf) = 0 on the first key
  const float pr = __expf(s - m_new);
  l_run = l_run * alpha + pr;
#pragma unroll
  for (int e = 0; e < DW; ++e) o[e] = fmaf(pr, vf[e], o[e] * alpha);
  m_run = m_new;
}

// the four 16-lane groups of a wave (xor-16 / xor-32 butterflies: the same order in every lane) into red[wave][row]: the values at
// [0, DMAX), the wave's max at [DMAX], its sum at [DMAX + 1]
template <int QB, int DC>
__device__ __forceinline__ void attn_merge_groups(float (&o)[QB][8 * DC], const float (&m_run)[QB], const float (&l_run)[QB],
                                                  float (&red)[4][QB][128 * DC + 4], const bool (&dvalid)[DC], int lane, int wave, int dl) {
  constexpr int DW = 8 * DC, DMAX = 128 * DC;
#pragma unroll
  for (int i = 0; i < QB; ++i) {
    float mw = fmaxf(m_run[i], __shfl_xor(m_run[i], 16, 64));
    mw = fmaxf(mw, __shfl_xor(mw, 32, 64));
    const float sc = (m_run[i] == -INFINITY) ? 0.f : __expf(m_run[i] - mw);
    float lw = l_run[i] * sc;
    lw += __shfl_xor(lw, 16, 64);
    lw += __shfl_xor(lw, 32, 64);
#pragma unroll
    for (int e = 0; e < DW; ++e) {
      float t = o[i][e] * sc;
      t += __shfl_xor(t, 16, 64);
      t += __shfl_xor(t, 32, 64);
      o[i][e] = t;
    }
    if ((lane >> 4) == 0) {
#pragma unroll
      for (int c = 0; c < DC; ++c) {
        if (dvalid[c]) {
#pragma unroll
          for (int e = 0; e < 8; ++e) red[wave][i][c * 128 + dl * 8 + e] = o[i][8 * c + e];
        }
      }
      if (dl == 0) {
        red[wave][i][DMAX] = mw;
        red[wave][i][DMAX + 1] = lw;
      }
    }
  }
}

// the four waves of the workgroup in wave order, for output (row i, dim d): max, weighted value, weighted sum
template <int QB, int DMAX>
__device__ __forceinline__ void attn_merge_waves(const float (&red)[4][QB][DMAX + 4], int i, int d, float& mg, float& acc, float& lsum) {
  mg = -INFINITY;
#pragma unroll
  for (int gg = 0; gg < 4; ++gg) mg = fmaxf(mg, red[gg][i][DMAX]);
  acc = 0.f;
  lsum = 0.f;
#pragma unroll
  for (int gg = 0; gg < 4; ++gg) {
    const float mgk = red[gg][i][DMAX];
    const float w = (mgk == -INFINITY) ? 0.f : __expf(mgk - mg);
    acc = fmaf(w, red[gg][i][d], acc);
    lsum = fmaf(w, red[gg][i][DMAX + 1], lsum);
  }
}

// Causal attention over the fp32 cache, fp32 FMA arithmetic (modeling_llama_xformer.py:204-239: prefill is causal, a q_len == 1 step
// sees the whole cache — both are "row t of the chunk sees keys 0 .. pos0 + t"). Workgroup = (QB query rows of the chunk, head,
// sequence), 16 groups of 16 lanes: a group owns keys grp, grp + 16, ...; a lane owns 8 of the D <= 128 head dims; every key row is
// loaded once for the QB query rows. Online softmax per (group, row), the 16 groups meet in LDS in group order (deterministic).
// Output: the two 16-bit planes of the context rows (the o-projection's A operand), row-major or tiled (store_planes8's layouts,
// one element at a time).
struct AttnF32P {
  const float* q;          // row r = g*T + t at q + r*q_stride, head h at + h*D (already rotated)
  const float* kc;
  const void* vc;          // fp32, or (V16 kernels) the model's 16-bit dtype with the same element strides
  unsigned short* out;
  const int* pos0_dev;     // [G] cache position of the chunk's first token (causal only)
  long long q_stride, seq_stride, row_stride, head_stride;   // K / V element strides: sequence, key row, head
  int T, H, D, Tmax, tiled, causal;
  float scale;
  float* part;             // SPLIT kernels: partial results [G][H][nsplit][D + 2] = (unnormalised sum over the split's keys, running max, sum)
  int nsplit;
  // T = 1 with RoPE fused in (round 6): q is the UNROTATED row of the qkv buffer, knew / vnew the new token's k / v rows (same row stride
  // as q), cos_t / sin_t the [Tmax][D/2] fp32 tables. The workgroup (the split that owns key pos0[g]) rotates q and k, appends k / v to
  // the cache — what rope_kv_f32_kernel does in a launch of its own — and attends over keys 0 .. pos0 - 1 from the cache plus the new
  // key from registers. nullptr = q is rotated and the cache already holds the token.
  const float* cos_t;
  const float* sin_t;
  const float* knew;
  const float* vnew;
  // FP8 cache (KV8 = 1 kernels): kc / vc hold e4m3fn codes with the SAME element strides, ks / vs one fp32 power-of-two scale per key row,
  // [G][H][Tmax] with sequences sc_seq_stride floats apart
  const float* ks;
  const float* vs;
  long long sc_seq_stride;
  // paged cache (PAGED kernels, D = 128): kc / vc are page pools [npages + 1][H][page size][D] — seq_stride is the element stride between
  // PAGES, head_stride = page size * row_stride — and ptab int32 [G][ptw] names the page of key rows [i << pshift, (i + 1) << pshift) of
  // sequence g. Page 0 is the null page (all zeros, never written): what a contiguous kernel reads from rows nobody owns comes from there.
  const int* ptab;
  int pshift, npages, ptw;
};

// element offset of the page behind table entry pi of sequence g; entry and index are clamped, so a wrong table gives wrong numbers, never
// a wild address. Uniform over the workgroup (g, pi are): the lookup is scalar loads and SGPR arithmetic
__device__ __forceinline__ size_t attn_page_off(const AttnF32P& p, int g, int pi) {
  const int pg = p.ptab[(size_t)g * p.ptw + min(max(pi, 0), p.ptw - 1)];
  return (size_t)min(max(pg, 0), p.npages) * (size_t)p.seq_stride;
}

// one key row t of attn_f32_kernel's walk, as text: the contiguous loop below is, token for token, the loop it always was (its code does
// not move when the paged loop changes), and the paged loop runs the same statements on a page. KH_ / VBASE_: where row 0 sits in k / in
// the v cache's elements; VIS_ + i: the last row query i may see
#define SX_ATTN_F32_KEY_ROW(KH_, VBASE_, VIS_)                                                                                  \
    float kf[DW], vf[DW];                                                                                                       \
    float ksc = 1.f;                                                                                                            \
    _Pragma("unroll")                                                                                                           \
    for (int e = 0; e < DW; ++e) { kf[e] = 0.f; vf[e] = 0.f; }                                                                  \
    if constexpr (KV8 == 1) {                                                                                                   \
      const u32x2_t kw = *(const u32x2_t*)(kc8 + (size_t)t * p.row_stride + dl * 8);                                            \
      const u32x2_t vw = *(const u32x2_t*)(vc8 + (size_t)t * p.row_stride + dl * 8);                                            \
      ksc = p.ks[sbase + t];                                                                                                    \
      const float vsc = p.vs[sbase + t];                                                                                        \
      decode8(kw, kf);                                                                                                          \
      decode8(vw, vf);                                                                                                          \
    _Pragma("unroll")                                                                                                           \
      for (int e = 0; e < 8; ++e) vf[e] *= vsc;                                                                                 \
    }                                                                                                                           \
    _Pragma("unroll")                                                                                                           \
    for (int c = 0; c < DC; ++c) {                                                                                              \
      if (KV8 != 1 && dvalid[c]) {                                                                                              \
        const float* kr = (KH_) + (size_t)t * p.row_stride + c * 128 + dl * 8;                                                  \
        const size_t vo = (VBASE_) + (size_t)t * p.row_stride + c * 128 + dl * 8;                                               \
        const f32x4_t k0 = *(const f32x4_t*)kr, k1 = *(const f32x4_t*)(kr + 4);                                                 \
    _Pragma("unroll")                                                                                                           \
        for (int e = 0; e < 4; ++e) { kf[8 * c + e] = k0[e]; kf[8 * c + 4 + e] = k1[e]; }                                       \
        if constexpr (V16) {                                                                                                    \
          const u32x4_t w = *(const u32x4_t*)((const unsigned short*)p.vc + vo);                                                \
    _Pragma("unroll")                                                                                                           \
          for (int e = 0; e < 4; ++e) {                                                                                         \
            vf[8 * c + 2 * e] = TT::to_f32((unsigned short)(w[e] & 0xffffu));                                                   \
            vf[8 * c + 2 * e + 1] = TT::to_f32((unsigned short)(w[e] >> 16));                                                   \
          }                                                                                                                     \
        } else {                                                                                                                \
          const float* vr = (const float*)p.vc + vo;                                                                            \
          const f32x4_t v0 = *(const f32x4_t*)vr, v1 = *(const f32x4_t*)(vr + 4);                                               \
    _Pragma("unroll")                                                                                                           \
          for (int e = 0; e < 4; ++e) { vf[8 * c + e] = v0[e]; vf[8 * c + 4 + e] = v1[e]; }                                     \
        }                                                                                                                       \
      }                                                                                                                         \
    }                                                                                                                           \
    _Pragma("unroll")                                                                                                           \
    for (int i = 0; i < QB; ++i) {                                                                                              \
      float s = attn_score<DW>(kf, qv[i]);                                                                                      \
      if constexpr (KV8 == 1) s *= ksc;                                                                                         \
      if (i < nq && t <= (VIS_) + i) attn_key_update<DW>(s, vf, m_run[i], l_run[i], o[i]);                                      \
    }

// QB query rows per workgroup: 4 for the decode step and short chunks, 8 for prefill (every key row is loaded once per QB rows: the
// K / V re-reads from L2 halve — 1.5k-token prompts, BASELINE config 5). DC = 8-dim chunks per lane: 1 covers D <= 128 (16 lanes x 8),
// 2 covers D <= 256 (lane dl owns dims [8 dl, 8 dl + 8) and [128 + 8 dl, 128 + 8 dl + 8): the LLM-side resamplers' head_dim 160).
// SPLIT (round 6; T = 1, QB = 1): blockIdx.x is a KEY split, not a query block — a decode step of few sequences (BASELINE config 5:
// 4 sequences x 40 heads = 160 workgroups on 256 CUs, each walking 1.5k keys in 94 dependent iterations) is latency-bound, not
// byte-bound; with the keys of a head spread over nsplit workgroups the walk is nsplit times shorter and the chip is full. Every split
// writes (sum of p v, running max, sum of p) to `part`, attn_f32_combine_kernel merges them in split order (deterministic).
// KV8 (the FP8 cache, D = 128): 1 = k and v are e4m3fn codes with one power-of-two scale per key row: 8 code bytes per lane and key row
// each, decoded exactly (v_cvt_pk_f32_fp8). The k scale multiplies the finished score (one multiply per query row instead of eight per key
// row) and the v scale the decoded values: a power of two commutes with every fp32 rounding of the fma chains as long as nothing leaves
// the normal range — the scores and v · 2^s do not (s in [-64, 64]); a probability times 2^s could, so p is never scaled. The result is,
// bit for bit, the KV8 = 0 kernel's on a cache holding the dequantised values. 2 = the bit-reference twin of the fused RoPE form: fp32
// caches, the new token's k / v quantised and dequantised on append. In both, the new token's own key / value (attended to from
// registers) are the dequantised values — the reason vnew is rounded under V16.
// PAGED (the paged cache, D = 128, KV8 = 0): the key walk goes page by page — ONE table lookup per page, uniform over the workgroup — and
// inside a page a group walks its keys grp + 16 i as before (splits start at multiples of 16, pages at multiples of 32: every group sees
// its keys in the same ascending order, so the bits are the contiguous kernel's). The fused append goes through the table too and writes
// nothing where the entry is 0.
template <typename TT, int QB, int DC, bool V16 = false, bool SPLIT = false, int KV8 = 0, bool PAGED = false>
__global__ __launch_bounds__(256) void attn_f32_kernel(const AttnF32P p) {
  constexpr int DW = 8 * DC, DMAX = 128 * DC;
  static_assert(!PAGED || (DC == 1 && KV8 == 0), "the paged cache: head_dim 128, fp32 k");
  static_assert(!SPLIT || (QB == 1 && DC == 1), "key splits: the single-row decode form");
  static_assert(KV8 == 0 || (DC == 1 && !V16), "the FP8 cache: head_dim 128, no 16-bit v");
  static_assert(KV8 != 2 || QB == 1, "KV8 = 2 only differs in the fused RoPE form");
  __shared__ float red[4][QB][DMAX + 4];
  const int q0 = SPLIT ? 0 : blockIdx.x * QB, h = blockIdx.y, g = blockIdx.z, D = p.D;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int grp = wave * 4 + (lane >> 4), dl = lane & 15;
  bool dvalid[DC];
#pragma unroll
  for (int c = 0; c < DC; ++c) dvalid[c] = c * 128 + dl * 8 < D;
  int pos0 = p.causal ? p.pos0_dev[g] : p.Tmax;   // not causal: every row sees all Tmax keys
  const bool parked = pos0 < 0;                   // a parked slot sees no key: its rows are 0, whatever a reused cache still holds
  if (pos0 < 0) pos0 = 0;
  const int nq = min(QB, p.T - q0);
  float qv[QB][DW], o[QB][DW], m_run[QB], l_run[QB];
#pragma unroll
  for (int i = 0; i < QB; ++i) {
    m_run[i] = -INFINITY;
    l_run[i] = 0.f;
#pragma unroll
    for (int e = 0; e < DW; ++e) { qv[i][e] = 0.f; o[i][e] = 0.f; }
#pragma unroll
    for (int c = 0; c < DC; ++c) {
      if (i < nq && dvalid[c]) {
        const float* qr = p.q + (size_t)((size_t)g * p.T + q0 + i) * p.q_stride + (size_t)h * D + c * 128 + dl * 8;
        const f32x4_t a = *(const f32x4_t*)qr, b = *(const f32x4_t*)(qr + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { qv[i][8 * c + e] = a[e] * p.scale; qv[i][8 * c + 4 + e] = b[e] * p.scale; }
      }
    }
  }
  // (KV8 = 1: kh is unused, see kc8; PAGED: the head's offset inside a page, the page's own comes from the table)
  const float* kh = PAGED ? p.kc + (size_t)h * p.head_stride : p.kc + (size_t)g * p.seq_stride + (size_t)h * p.head_stride;
  const size_t vbase = PAGED ? (size_t)h * p.head_stride : (size_t)g * p.seq_stride + (size_t)h * p.head_stride;
  const unsigned char* kc8 = (const unsigned char*)p.kc + vbase;                        // KV8 = 1: codes, same element strides
  const unsigned char* vc8 = (const unsigned char*)p.vc + vbase;
  const size_t sbase = (size_t)g * p.sc_seq_stride + (size_t)h * p.Tmax;                // KV8 = 1: the row scales of this (sequence, head)
  int kend = min(p.Tmax, pos0 + q0 + nq);       // keys 0 .. kend-1 are visible to the block's last row
  int kbeg = 0;
  int chunk = kend;
  if constexpr (SPLIT) {                              // this split's share of the keys: chunks of a multiple of 16 keys
    chunk = ((kend + p.nsplit - 1) / p.nsplit + 15) & ~15;
    kbeg = (int)blockIdx.x * chunk;
    kend = min(kend, kbeg + chunk);
  }
  // ---- RoPE fused into the T = 1 launch (D = 128: lane dl holds dims 8 dl .. 8 dl + 7, its rotation partner lane dl ^ 8 the other half) ----
  bool own_new = false;                               // this workgroup attends to the NEW key (from registers) and appends it
  float knew[8], vnew[8];
  if constexpr (QB == 1 && DC == 1) {
    if (p.cos_t != nullptr) {
      const int praw = p.pos0_dev[g];
      const bool pos_ok = praw >= 0 && praw < p.Tmax;
      const int pt = pos_ok ? praw : 0, half = D >> 1;
      const int jb = (dl & 7) * 8;
      float cs[8], sn[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {                   // tables rounded to the model dtype like the reference's cast (rope_kv_f32_kernel)
        cs[e] = TT::to_f32(TT::from_f32(p.cos_t[(size_t)pt * half + jb + e]));
        sn[e] = TT::to_f32(TT::from_f32(p.sin_t[(size_t)pt * half + jb + e]));
      }
      const size_t rbase = (size_t)g * p.q_stride + (size_t)h * D;
      const float* qo = p.q + rbase + dl * 8;
      const float* qp = p.q + rbase + (dl ^ 8) * 8;
      const float* ko = p.knew + rbase + dl * 8;
      const float* kp = p.knew + rbase + (dl ^ 8) * 8;
      const float* vo = p.vnew + rbase + dl * 8;
      const float sg = (dl < 8) ? -1.0f : 1.0f;       // first half: x1 c - x2 s; second half: x2 c + x1 s
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        qv[0][e] = rope_rot(qo[e], qp[e], cs[e], sn[e], sg) * p.scale;
        knew[e] = rope_rot(ko[e], kp[e], cs[e], sn[e], sg);
        vnew[e] = V16 ? TT::to_f32(TT::from_f32(vo[e])) : vo[e];
      }
      u32x2_t kcod, vcod;
      float ksc, vsc;
      if constexpr (KV8 != 0) {                       // every group holds the whole row: all of them quantise (uniform shuffles)
        quant_dequant_row8(knew, kcod, ksc);
        quant_dequant_row8(vnew, vcod, vsc);
      }
      own_new = pos_ok && (SPLIT ? (praw / chunk == (int)blockIdx.x) : true);
      size_t ao = (size_t)praw * p.row_stride;        // the appended row's offset from (kh, vbase)
      bool held = true;                               // PAGED: a page is reserved behind the row (entry != 0)
      if constexpr (PAGED) {
        const size_t po = attn_page_off(p, g, pt >> p.pshift);
        held = po != 0;
        ao = po + (size_t)(pt & ((1 << p.pshift) - 1)) * p.row_stride;
      }
      if (own_new && grp == 0 && held) {              // append: one 16-lane group covers the 128 dims
        const size_t vo_c = vbase + ao + dl * 8;
        if constexpr (KV8 == 1) {                     // codes: one 8-byte store per lane, one lane stores the two scales
          *(u32x2_t*)(const_cast<unsigned char*>(kc8) + (size_t)praw * p.row_stride + dl * 8) = kcod;
          *(u32x2_t*)(const_cast<unsigned char*>(vc8) + (size_t)praw * p.row_stride + dl * 8) = vcod;
          if (dl == 0) {
            const_cast<float*>(p.ks)[sbase + praw] = ksc;
            const_cast<float*>(p.vs)[sbase + praw] = vsc;
          }
        } else {
          float* kd = const_cast<float*>(kh) + ao + dl * 8;
#pragma unroll
          for (int e = 0; e < 8; ++e) kd[e] = knew[e];
          if constexpr (V16) {
            unsigned short* vd = (unsigned short*)const_cast<void*>(p.vc) + vo_c;
#pragma unroll
            for (int e = 0; e < 8; ++e) vd[e] = TT::from_f32(vo[e]);
          } else {
            float* vd = (float*)const_cast<void*>(p.vc) + vo_c;
#pragma unroll
            for (int e = 0; e < 8; ++e) vd[e] = KV8 == 2 ? vnew[e] : vo[e];     // (KV8 = 2: the dequantised row)
          }
        }
      }
      if (pos_ok) kend = min(kend, praw);             // the cache rows below pos; the new key comes from registers
    }
  }
  if (parked) kend = 0;                               // (stale rows of a reused slot are finite but arbitrary: v = +-max would not stay finite)
  if constexpr (PAGED) {                              // one trip, and ONE table lookup, per page the key range touches
    for (int pi = kbeg >> p.pshift; pi < ((kend + (1 << p.pshift) - 1) >> p.pshift); ++pi) {
      const int pb = pi << p.pshift;                  // the page's first key row; t counts from it
      const size_t po = attn_page_off(p, g, pi);
      const int te = min(kend, pb + (1 << p.pshift)) - pb;
      for (int t = max(kbeg, pb) - pb + grp; t < te; t += 16) {
        SX_ATTN_F32_KEY_ROW(kh + po, vbase + po, pos0 + q0 - pb)
      }
    }
  } else {
  for (int t = kbeg + grp; t < kend; t += 16) {
    SX_ATTN_F32_KEY_ROW(kh, vbase, pos0 + q0)
  }
  }
  if constexpr (QB == 1 && DC == 1) {
    if (own_new && grp == 0) {                        // the new token's own key / value, straight from the registers
      attn_key_update<8>(attn_score<8>(knew, qv[0]), vnew, m_run[0], l_run[0], o[0]);
    }
  }
  // the four 16-lane groups of a wave first (xor-16 / xor-32 butterflies: the same order in every lane), then the four waves through LDS
  // in wave order: deterministic
  attn_merge_groups<QB, DC>(o, m_run, l_run, red, dvalid, lane, wave, dl);
  __syncthreads();
  // thread → (row i, dim d): 256 threads cover QB * DMAX outputs in QB * DMAX / 256 passes
  for (int idx = threadIdx.x; idx < QB * DMAX; idx += 256) {
    const int i = idx / DMAX, d = idx - i * DMAX;
    if (i >= nq || d >= D) continue;
    float mg, acc, lsum;
    attn_merge_waves<QB, DMAX>(red, i, d, mg, acc, lsum);
    if constexpr (SPLIT) {
      float* pr = p.part + ((size_t)((size_t)g * p.H + h) * p.nsplit + blockIdx.x) * (D + 2);
      pr[d] = acc;
      if (d == 0) { pr[D] = mg; pr[D + 1] = lsum; }
      continue;
    }
    const float val = lsum > 0.f ? acc / lsum : 0.f;
    unsigned short hi, lo;
    split1<TT>(val, hi, lo);
    const int cols = p.H * D, col = h * D + d;
    if (p.tiled) {
      const int row = g * p.T + q0 + i;
      unsigned short* b = p.out + ((size_t)(row >> 4) * (size_t)(cols >> 5) + (size_t)(col >> 5)) * 512 + (size_t)(row & 15) * 32 + (col & 31);
      b[0] = hi;
      b[(size_t)cols * 16 * (size_t)p.tiled] = lo;
    } else {
      unsigned short* b = p.out + (size_t)((size_t)g * p.T + q0 + i) * 2 * cols + col;
      b[0] = hi;
      b[cols] = lo;
    }
  }
}

#undef SX_ATTN_F32_KEY_ROW

// merge of the key splits of one (head, sequence): thread d adds the partials in split order
template <typename TT>
__global__ __launch_bounds__(128) void attn_f32_combine_kernel(const AttnF32P p) {
  const int h = blockIdx.x, g = blockIdx.y, d = threadIdx.x, D = p.D;
  if (d >= D) return;
  const float* pr = p.part + (size_t)((size_t)g * p.H + h) * p.nsplit * (D + 2);
  float mg = -INFINITY;
  for (int s = 0; s < p.nsplit; ++s) mg = fmaxf(mg, pr[(size_t)s * (D + 2) + D]);
  float acc = 0.f, lsum = 0.f;
  for (int s = 0; s < p.nsplit; ++s) {
    const float ms = pr[(size_t)s * (D + 2) + D];
    const float w = (ms == -INFINITY) ? 0.f : __expf(ms - mg);
    acc = fmaf(w, pr[(size_t)s * (D + 2) + d], acc);
    lsum = fmaf(w, pr[(size_t)s * (D + 2) + D + 1], lsum);
  }
  const float val = lsum > 0.f ? acc / lsum : 0.f;
  unsigned short hi, lo;
  split1<TT>(val, hi, lo);
  const int cols = p.H * D, col = h * D + d;
  if (p.tiled) {
    unsigned short* b = p.out + ((size_t)(g >> 4) * (size_t)(cols >> 5) + (size_t)(col >> 5)) * 512 + (size_t)(g & 15) * 32 + (col & 31);
    b[0] = hi;
    b[(size_t)cols * 16 * (size_t)p.tiled] = lo;
  } else {
    unsigned short* b = p.out + (size_t)g * 2 * cols + col;
    b[0] = hi;
    b[cols] = lo;
  }
}

// ---- the VERIFY form of the fused-RoPE decode attention (speculative decoding: T = K + 1 rows per sequence, 2 <= T <= 8, D = 128) ------
// Row t of sequence g (qkv row g*T + t) sits at position pos0[g] + t. The launch gives, bit for bit, what T successive fused T = 1 SPLIT
// launches give (call t on row t at position pos0 + t, same nsplit): context partials, appended k rows, appended v rows. Workgroup =
// (key split, head, sequence) as in the T = 1 launch, but it serves all T query rows: every cache key row of the (head, sequence, split)
// is loaded ONCE for the T rows. What each row keeps of its own T = 1 launch:
//   * its own chunk ((kend_t + nsplit - 1) / nsplit + 15) & ~15 with kend_t from pos0 + t + 1, hence its own key range per split — the
//     ranges of two rows differ when the context crosses a multiple of 16 nsplit inside the launch; the key loop walks the union and a
//     row takes a key only inside its own range;
//   * keys go to 16-lane groups by key % 16 (every range starts at a multiple of 16), in ascending order per group: cache keys below
//     pos0 first, then the earlier draft rows' keys pos0 + j (j < t) by group (pos0 + j) % 16, which the T = 1 launches would have
//     found in the cache — here they come from LDS, where group t parked row t's rotated q, k and (rounded under V16) v — and last the
//     row's own key by group 0;
//   * the arithmetic: rope_rot (its two T = 1 contractions), attn_score, attn_key_update, attn_merge_groups, attn_merge_waves above, shared with attn_f32_kernel.
// A parked slot (pos0 < 0) idles ALL its rows like the T = 1 launch idles its one (they read no key row, write no cache row and
// come out as 0); a row at or past Tmax writes no cache row. The partials go to part[G*T][H][nsplit][D + 2]; the combine is
// attn_f32_combine_kernel over G*T rows.
template <typename TT, int TQ, bool V16>
__global__ __launch_bounds__(256) void attn_f32_verify_kernel(const AttnF32P p) {
  constexpr int D = 128;
  __shared__ float red[4][TQ][D + 4];
  __shared__ float qs[TQ][D], kn[TQ][D], vn[TQ][D];
  const int sp = blockIdx.x, h = blockIdx.y, g = blockIdx.z, T = p.T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int grp = wave * 4 + (lane >> 4), dl = lane & 15;
  const bool dvalid[1] = {true};
  const int praw0 = p.pos0_dev[g];
  const bool parked = praw0 < 0;
  const int pos0 = parked ? 0 : praw0;
  const int climit = parked ? 0 : min(pos0, p.Tmax);    // cache rows this launch may read: those below pos0 (parked: none)
  const float* kh = p.kc + (size_t)g * p.seq_stride + (size_t)h * p.head_stride;
  const size_t vbase = (size_t)g * p.seq_stride + (size_t)h * p.head_stride;
  float qv[TQ][8], o[TQ][8], m_run[TQ], l_run[TQ];
  int kb[TQ], ke[TQ];                                   // the row's key range in this split, its own key excluded
  bool own[TQ];                                         // this split attends to the row's own key and appends it
  int lo = p.Tmax, hi = 0;                              // union of the rows' cache ranges
  const int jb = (dl & 7) * 8;
  const float sg = (dl < 8) ? -1.0f : 1.0f;             // first half: x1 c - x2 s; second half: x2 c + x1 s
#pragma unroll
  for (int i = 0; i < TQ; ++i) {
    m_run[i] = -INFINITY;
    l_run[i] = 0.f;
    kb[i] = 0;
    ke[i] = 0;
    own[i] = false;
#pragma unroll
    for (int e = 0; e < 8; ++e) { qv[i][e] = 0.f; o[i][e] = 0.f; }
    if (i < T) {                                        // uniform over the workgroup
      const int pr = pos0 + i;
      const bool pos_ok = !parked && pr < p.Tmax;
      const int kend = parked ? 1 : min(p.Tmax, pr + 1);   // (parked: only keeps chunk > 0; climit = 0 and own = false, no key is walked)
      const int chunk = ((kend + p.nsplit - 1) / p.nsplit + 15) & ~15;
      kb[i] = sp * chunk;
      ke[i] = min(kend, kb[i] + chunk);
      own[i] = pos_ok && (pr / chunk == sp);
      if (pos_ok) ke[i] = min(ke[i], pr);
      const int ce = min(ke[i], climit);
      if (kb[i] < ce) { lo = min(lo, kb[i]); hi = max(hi, ce); }
    }
    if (i < T && grp == i) {                            // group i rotates row i, parks its q / k / v in LDS and, in the owning split, appends k / v
      const int pr = pos0 + i;
      const int pt = (!parked && pr < p.Tmax) ? pr : 0;
      float cs[8], sn[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {                     // tables rounded to the model dtype like the reference's cast (rope_kv_f32_kernel)
        cs[e] = TT::to_f32(TT::from_f32(p.cos_t[(size_t)pt * 64 + jb + e]));
        sn[e] = TT::to_f32(TT::from_f32(p.sin_t[(size_t)pt * 64 + jb + e]));
      }
      const size_t rbase = (size_t)((size_t)g * T + i) * p.q_stride + (size_t)h * D;
      const float* qo = p.q + rbase + dl * 8;
      const float* qp = p.q + rbase + (dl ^ 8) * 8;
      const float* ko = p.knew + rbase + dl * 8;
      const float* kp = p.knew + rbase + (dl ^ 8) * 8;
      const float* vo = p.vnew + rbase + dl * 8;
      float kr[8], vr[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        qs[i][dl * 8 + e] = rope_rot_q_t1(qo[e], qp[e], cs[e], sn[e], sg) * p.scale;
        kr[e] = rope_rot_k_t1(ko[e], kp[e], cs[e], sn[e], sg);
        vr[e] = V16 ? TT::to_f32(TT::from_f32(vo[e])) : vo[e];
      }
      {
#pragma unroll
        for (int e = 0; e < 8; ++e) { kn[i][dl * 8 + e] = kr[e]; vn[i][dl * 8 + e] = vr[e]; }
        if (own[i]) {
          float* kd = const_cast<float*>(kh) + (size_t)pr * p.row_stride + dl * 8;
          const size_t vo_c = vbase + (size_t)pr * p.row_stride + dl * 8;
#pragma unroll
          for (int e = 0; e < 8; ++e) kd[e] = kr[e];
          if constexpr (V16) {
            unsigned short* vd = (unsigned short*)const_cast<void*>(p.vc) + vo_c;
#pragma unroll
            for (int e = 0; e < 8; ++e) vd[e] = TT::from_f32(vo[e]);
          } else {
            float* vd = (float*)const_cast<void*>(p.vc) + vo_c;
#pragma unroll
            for (int e = 0; e < 8; ++e) vd[e] = vo[e];
          }
        }
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < TQ; ++i) {
    if (i < T) {
#pragma unroll
      for (int e = 0; e < 8; ++e) qv[i][e] = qs[i][dl * 8 + e];
    }
  }
  // ---- cache keys below pos0: one load per key row for all T query rows ----
  for (int t = lo + grp; t < hi; t += 16) {             // lo is a multiple of 16; hi <= climit <= Tmax
    float kf[8], vf[8];
    const float* kr = kh + (size_t)t * p.row_stride + dl * 8;
    const size_t vo = vbase + (size_t)t * p.row_stride + dl * 8;
    const f32x4_t k0 = *(const f32x4_t*)kr, k1 = *(const f32x4_t*)(kr + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { kf[e] = k0[e]; kf[4 + e] = k1[e]; }
    if constexpr (V16) {
      const u32x4_t w = *(const u32x4_t*)((const unsigned short*)p.vc + vo);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        vf[2 * e] = TT::to_f32((unsigned short)(w[e] & 0xffffu));
        vf[2 * e + 1] = TT::to_f32((unsigned short)(w[e] >> 16));
      }
    } else {
      const float* vr = (const float*)p.vc + vo;
      const f32x4_t v0 = *(const f32x4_t*)vr, v1 = *(const f32x4_t*)(vr + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { vf[e] = v0[e]; vf[4 + e] = v1[e]; }
    }
#pragma unroll
    for (int i = 0; i < TQ; ++i) {
      const float s = attn_score<8>(kf, qv[i]);
      if (t >= kb[i] && t < min(ke[i], climit)) attn_key_update<8>(s, vf, m_run[i], l_run[i], o[i]);   // uniform over the 16-lane group
    }
  }
  // ---- the earlier draft rows' keys pos0 + j, ascending, by the group the cache walk would have given them ----
#pragma unroll
  for (int j = 0; j < TQ - 1; ++j) {
    const int key = pos0 + j;
    if (j < T - 1 && !parked && key < p.Tmax && (key & 15) == grp) {
      float kf[8], vf[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { kf[e] = kn[j][dl * 8 + e]; vf[e] = vn[j][dl * 8 + e]; }
#pragma unroll
      for (int i = j + 1; i < TQ; ++i) {
        const float s = attn_score<8>(kf, qv[i]);
        if (key >= kb[i] && key < ke[i]) attn_key_update<8>(s, vf, m_run[i], l_run[i], o[i]);
      }
    }
  }
  // ---- every row's own key, last, by group 0 ----
  if (grp == 0) {
#pragma unroll
    for (int i = 0; i < TQ; ++i) {
      if (own[i]) {
        float kf[8], vf[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { kf[e] = kn[i][dl * 8 + e]; vf[e] = vn[i][dl * 8 + e]; }
        attn_key_update<8>(attn_score<8>(kf, qv[i]), vf, m_run[i], l_run[i], o[i]);
      }
    }
  }
  attn_merge_groups<TQ, 1>(o, m_run, l_run, red, dvalid, lane, wave, dl);
  __syncthreads();
  for (int idx = threadIdx.x; idx < TQ * D; idx += 256) {
    const int i = idx / D, d = idx - i * D;
    if (i >= T) continue;
    float mg, acc, lsum;
    attn_merge_waves<TQ, D>(red, i, d, mg, acc, lsum);
    float* pr = p.part + ((size_t)((size_t)((size_t)g * T + i) * p.H + h) * p.nsplit + sp) * (D + 2);
    pr[d] = acc;
    if (d == 0) { pr[D] = mg; pr[D + 1] = lsum; }
  }
}

// ---- the same attention on the matrix pipe, for chunks above 8 tokens (prefill, the forced image chunk) ------------------------------
// v_mfma_f32_32x32x2_f32 multiplies fp32 operands exactly and accumulates in fp32 — the arithmetic of the VALU kernel above at the fp32
// MFMA rate (64 FLOP / clk / SIMD = the whole fp32 vector rate in one instruction stream that leaves the VALU free for the softmax).
// The VALU kernel is O(T^2) FMA work on the vector pipe: 495 us per launch at T = 165 (84 launches per headline step), quadratic from
// there (BASELINE config 5 prefills 1.5k tokens).
//   wave = 32 query rows x all visible keys, flash-style over 32-key tiles; workgroup = 4 waves = 128 query rows of one (head, sequence).
//   S^T[key][q] = K · Q^T: the contraction index is split by LANE HALF, d = 64 (lane >> 5) + step — so a lane's 64 operand values are 256
//     CONTIGUOUS bytes of its own row, for Q (held in registers for the whole pass, pre-scaled) and for the K tile (16-byte loads straight
//     from the cache, no LDS: a wave's tile is its own);
//   softmax per query column: a lane holds 16 of the column's 32 scores, its partner lane ^ 32 the others (one exchange for the max, one
//     for the sum);
//   O^T[d][q] += V^T · P^T: step t contracts the t-th key of each lane half (keys 8 (t >> 2) + 4 half + (t & 3): exactly the S^T rows
//     the half holds, so P feeds the B operand without moving), the A operand is V[key][4 (lane & 31) + block .. ]: one 16-byte (fp32) or
//     8-byte (16-bit v, the mixed cache) load per step; output row index r of block b is head dim 4 r + b, so a lane ends with 16 groups of
//     4 CONSECUTIVE head dims of its query row → 8-byte plane stores.
// D = 128 only (the decoder's head_dim); everything else keeps the VALU kernel.
typedef float f32x16v_t __attribute__((ext_vector_type(16)));
// KV8 (the FP8 cache): the K tile is 64 code bytes of the lane's half row (four 16-byte loads), a V step 4 code bytes; the k scale
// multiplies the key's score row, the v scale the decoded operand (exact, see attn_f32_kernel) — the same bits as the fp32 kernel on the
// dequantised cache.
// PAGED (the paged cache): k0 is a multiple of 32 and a page holds a multiple of 32 rows, so a tile lies in ONE page: one uniform table
// lookup per tile; rows past kend (cancelled by P = 0) come from the tile's own page or the null page, finite either way.
template <typename TT, bool V16, bool KV8 = false, bool PAGED = false>
__global__ __launch_bounds__(256) void attn_f32_mfma_kernel(const AttnF32P p) {
  static_assert(!(PAGED && KV8), "the paged cache has no FP8 form");
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int D = 128;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = blockIdx.y, g = blockIdx.z;
  const int half = lane >> 5, l32 = lane & 31;
  const int q0 = blockIdx.x * 128 + wave * 32;
  if (q0 >= p.T) return;                                       // (no barriers in this kernel)
  int pos0 = p.pos0_dev[g];
  const bool parked = pos0 < 0;                                 // a parked slot sees no key: its rows are 0
  if (pos0 < 0) pos0 = 0;
  const int qi = q0 + l32;                                      // this lane's query row (column of S^T / O^T)
  const bool qok = qi < p.T;
  const int qc = qok ? qi : p.T - 1;
  // Q operand: 64 contiguous floats of the lane's row, pre-scaled
  float qv[64];
  {
    const float* qr = p.q + (size_t)((size_t)g * p.T + qc) * p.q_stride + (size_t)h * D + half * 64;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const f32x4_t a = *(const f32x4_t*)(qr + 4 * e);
      qv[4 * e] = a[0] * p.scale; qv[4 * e + 1] = a[1] * p.scale; qv[4 * e + 2] = a[2] * p.scale; qv[4 * e + 3] = a[3] * p.scale;
    }
  }
  const float* kh = PAGED ? p.kc + (size_t)h * p.head_stride : p.kc + (size_t)g * p.seq_stride + (size_t)h * p.head_stride;
  const size_t vbase = PAGED ? (size_t)h * p.head_stride : (size_t)g * p.seq_stride + (size_t)h * p.head_stride;
  const unsigned char* kc8 = (const unsigned char*)p.kc + vbase;                        // KV8: codes, same element strides
  const unsigned char* vc8 = (const unsigned char*)p.vc + vbase;
  const size_t sbase = (size_t)g * p.sc_seq_stride + (size_t)h * p.Tmax;                // KV8: the row scales of this (sequence, head)
  f32x16v_t o[4];
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int j = 0; j < 16; ++j) o[b][j] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  const int q_last = min(p.T, q0 + 32) - 1;
  const int kend = parked ? 0 : min(p.Tmax, pos0 + q_last + 1); // keys 0 .. kend - 1 are visible to the wave's last row
  const int vis = pos0 + qi;                                    // last key this lane's row may see
  for (int k0 = 0; k0 < kend; k0 += 32) {
    // ---- S^T tile = K[k0 .. k0+31] · Q^T ----
    size_t po = 0;                                               // PAGED: the tile's page (uniform); its rows are (k0 + ..) & pm inside it
    int pm = -1;
    if constexpr (PAGED) {
      po = attn_page_off(p, g, k0 >> p.pshift);
      pm = (1 << p.pshift) - 1;
    }
    const int kr_ = PAGED ? ((k0 + l32) & pm) : min(k0 + l32, p.Tmax - 1);
    const float* kr = kh + po + (size_t)kr_ * p.row_stride + half * 64;
    f32x16v_t sacc;
#pragma unroll
    for (int j = 0; j < 16; ++j) sacc[j] = 0.f;
    if constexpr (KV8) {                                         // decoded four values at a time, right in front of their MFMAs: the tile
      const unsigned char* kr8 = kc8 + (size_t)kr_ * p.row_stride + half * 64;      // lives in 16 registers of codes, not 64 of floats
      u32x4_t kw[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) kw[e] = *(const u32x4_t*)(kr8 + 16 * e);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)kw[e >> 2][e & 3], false);
        const auto b = __builtin_amdgcn_cvt_pk_f32_fp8((int)kw[e >> 2][e & 3], true);
        sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], qv[4 * e], sacc, 0, 0, 0);
        sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], qv[4 * e + 1], sacc, 0, 0, 0);
        sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(b[0], qv[4 * e + 2], sacc, 0, 0, 0);
        sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(b[1], qv[4 * e + 3], sacc, 0, 0, 0);
      }
    } else {
      f32x4_t kq[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) kq[e] = *(const f32x4_t*)(kr + 4 * e);
#pragma unroll
      for (int e = 0; e < 16; ++e)
#pragma unroll
        for (int c = 0; c < 4; ++c) sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(kq[e][c], qv[4 * e + c], sacc, 0, 0, 0);
    }
    if constexpr (KV8) {                                         // score row j belongs to key k0 + 8 (j >> 2) + 4 half + (j & 3)
#pragma unroll
      for (int j = 0; j < 16; ++j) sacc[j] *= p.ks[sbase + min(k0 + (j >> 2) * 8 + half * 4 + (j & 3), p.Tmax - 1)];
    }
    // ---- online softmax of the lane's column (16 local keys + the partner's 16) ----
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int key = k0 + (j >> 2) * 8 + half * 4 + (j & 3);
      sacc[j] = (key <= vis && key < kend) ? sacc[j] : -INFINITY;
      mx = fmaxf(mx, sacc[j]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);
    const float alpha = (m_new == -INFINITY) ? 1.f : __expf(m_run - m_new);      // exp(-inf) = 0 on the first visible tile
    float ls = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float pr = (sacc[j] == -INFINITY) ? 0.f : __expf(sacc[j] - m_new);
      sacc[j] = pr;
      ls += pr;
    }
    ls += __shfl_xor(ls, 32, 64);
    l_run = l_run * alpha + ls;
    m_run = m_new;
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int j = 0; j < 16; ++j) o[b][j] *= alpha;
    // ---- O^T += V^T · P^T ----
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int key = PAGED ? ((k0 + (t >> 2) * 8 + half * 4 + (t & 3)) & pm) : min(k0 + (t >> 2) * 8 + half * 4 + (t & 3), p.Tmax - 1);
      const size_t vo = vbase + po + (size_t)key * p.row_stride + 4 * l32;
      float vv[4];
      if constexpr (KV8) {
        const unsigned w = *(const unsigned*)(vc8 + (size_t)key * p.row_stride + 4 * l32);
        const float vsc = p.vs[sbase + key];
        const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
        const auto b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
        vv[0] = a[0] * vsc; vv[1] = a[1] * vsc; vv[2] = b[0] * vsc; vv[3] = b[1] * vsc;
      } else if constexpr (V16) {
        const u32x2_t w = *(const u32x2_t*)((const unsigned short*)p.vc + vo);
        vv[0] = TT::to_f32((unsigned short)(w[0] & 0xffffu)); vv[1] = TT::to_f32((unsigned short)(w[0] >> 16));
        vv[2] = TT::to_f32((unsigned short)(w[1] & 0xffffu)); vv[3] = TT::to_f32((unsigned short)(w[1] >> 16));
      } else {
        const f32x4_t w = *(const f32x4_t*)((const float*)p.vc + vo);
        vv[0] = w[0]; vv[1] = w[1]; vv[2] = w[2]; vv[3] = w[3];
      }
#pragma unroll
      for (int b = 0; b < 4; ++b) o[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv[b], sacc[t], o[b], 0, 0, 0);
    }
  }
  // ---- normalise, split into planes, store: lane = query row qi, register j of block b = head dim 4 r_j + b ----
  if (!qok) return;
  const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
  const int cols = p.H * D;
  unsigned short* orow = p.out + (size_t)((size_t)g * p.T + qi) * 2 * cols + (size_t)h * D;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int r = (j >> 2) * 8 + half * 4 + (j & 3);
    unsigned short hi[4], lo[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) split1<TT>(o[b][j] * inv, hi[b], lo[b]);
    u32x2_t wh, wl;
    wh[0] = (unsigned)hi[0] | ((unsigned)hi[1] << 16); wh[1] = (unsigned)hi[2] | ((unsigned)hi[3] << 16);
    wl[0] = (unsigned)lo[0] | ((unsigned)lo[1] << 16); wl[1] = (unsigned)lo[2] | ((unsigned)lo[3] << 16);
    *(u32x2_t*)(orow + 4 * r) = wh;
    *(u32x2_t*)(orow + cols + 4 * r) = wl;
  }
#endif
}

static dim3 gs_grid(int64_t n) {
  int64_t b = (n + 255) / 256;
  if (b > 65535 * 4) b = 65535 * 4;
  if (b < 1) b = 1;
  return dim3((unsigned)b);
}

}  // namespace sxk_precise
using namespace sxk_precise;

#define ST ((hipStream_t)stream)

extern "C" int sx_split16(const float* x, int64_t ldx, void* out, int rows, int cols, int dtype, void* stream) {
  SX_CHECK(x && out, "sx_split16: null pointer");
  const int tiled = (dtype & SX_TILED16) ? (rows + 15) / 16 : 0, dt = dtype & 0xff;     // = the tiled layout's row blocks
  SX_CHECK(dt == SX_F16 || dt == SX_BF16, "sx_split16: dtype");
  SX_CHECK(rows >= 1 && cols >= 8 && cols % 8 == 0 && ldx >= cols && ldx % 4 == 0 && (((uintptr_t)x) & 15) == 0 && (((uintptr_t)out) & 15) == 0,
           "sx_split16: rows=%d cols=%d ldx=%lld (cols %% 8, 16-B aligned rows)", rows, cols, (long long)ldx);
  SX_CHECK(!tiled || (rows <= 32 && cols % 32 == 0), "sx_split16: operand tiles hold <= 32 rows of cols %% 32 == 0");
  const int64_t n = (int64_t)rows * (cols / 8);
  if (dt == SX_BF16) hipLaunchKernelGGL(split16_kernel<BF16>, gs_grid(n), dim3(256), 0, ST, x, (long long)ldx, (unsigned short*)out, rows, cols, tiled);
  else hipLaunchKernelGGL(split16_kernel<F16>, gs_grid(n), dim3(256), 0, ST, x, (long long)ldx, (unsigned short*)out, rows, cols, tiled);
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}

extern "C" int sx_rmsnorm_planes(const float* x, const float* gamma, float* y32, void* out16, int rows, int cols, float eps, int dtype,
                                 void* stream) {
  SX_CHECK(x && gamma && (y32 || out16), "sx_rmsnorm_planes: null pointer");
  const int tiled = (dtype & SX_TILED16) ? (rows + 15) / 16 : 0, dt = dtype & 0xff;
  SX_CHECK(dt == SX_F16 || dt == SX_BF16, "sx_rmsnorm_planes: dtype");
  SX_CHECK(rows >= 1 && cols >= 8 && cols % 8 == 0 && (((uintptr_t)x) & 15) == 0 && (((uintptr_t)gamma) & 15) == 0,
           "sx_rmsnorm_planes: rows=%d cols=%d (cols %% 8, 16-B aligned)", rows, cols);
  SX_CHECK(!tiled || !out16 || (rows <= 32 && cols % 32 == 0), "sx_rmsnorm_planes: operand tiles hold <= 32 rows of cols %% 32 == 0");
  if (dt == SX_BF16)
    hipLaunchKernelGGL(rmsnorm_planes_kernel<BF16>, dim3(rows), dim3(256), 0, ST, x, gamma, y32, (unsigned short*)out16, cols, eps, tiled);
  else
    hipLaunchKernelGGL(rmsnorm_planes_kernel<F16>, dim3(rows), dim3(256), 0, ST, x, gamma, y32, (unsigned short*)out16, cols, eps, tiled);
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}

// (page_table == NULL: the contiguous caches, cache_seq_stride between sequences; else the page pools, cache_seq_stride between pages)
static int rope_kv_f32_impl(float* qkv, float* kcache, void* vcache, int v16, const float* cos_tab, const float* sin_tab,
                            const int32_t* pos0_dev, int G, int T, int H, int D, int Tmax, int64_t cache_seq_stride, int table_dtype,
                            void* stream, const int32_t* page_table = nullptr, int page_shift = 0, int n_pages = 0) {
  SX_CHECK(qkv && kcache && vcache && cos_tab && sin_tab && pos0_dev, "sx_rope_kv_append_f32: null pointer");
  SX_CHECK(D % 2 == 0 && G >= 1 && T >= 1 && H >= 1, "sx_rope_kv_append_f32: D/G/T/H");
  SX_CHECK(table_dtype == SX_F16 || table_dtype == SX_BF16, "sx_rope_kv_append_f32: table_dtype");
  const int64_t n = (int64_t)G * T * H * (D / 2);
  const int ptw = page_table ? (Tmax + (1 << page_shift) - 1) >> page_shift : 0;
#define SX_ROPE_GO(TT, V16)                                                                                                            \
  hipLaunchKernelGGL((rope_kv_f32_kernel<TT, V16>), gs_grid(n), dim3(256), 0, ST, qkv, kcache, vcache, cos_tab, sin_tab, pos0_dev, T, H, D, \
                     Tmax, G, (long long)cache_seq_stride)
#define SX_ROPE_PAGED_GO(TT, V16)                                                                                                      \
  hipLaunchKernelGGL((rope_kv_f32_paged_kernel<TT, V16>), gs_grid(n), dim3(256), 0, ST, qkv, kcache, vcache, cos_tab, sin_tab, pos0_dev, T, \
                     H, D, Tmax, G, (long long)cache_seq_stride, page_table, page_shift, n_pages, ptw)
  if (page_table) {
    if (table_dtype == SX_BF16) { if (v16) SX_ROPE_PAGED_GO(BF16, true); else SX_ROPE_PAGED_GO(BF16, false); }
    else { if (v16) SX_ROPE_PAGED_GO(F16, true); else SX_ROPE_PAGED_GO(F16, false); }
  } else
  if (table_dtype == SX_BF16) { if (v16) SX_ROPE_GO(BF16, true); else SX_ROPE_GO(BF16, false); }
  else { if (v16) SX_ROPE_GO(F16, true); else SX_ROPE_GO(F16, false); }
#undef SX_ROPE_GO
#undef SX_ROPE_PAGED_GO
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}

extern "C" int sx_rope_kv_append_f32_paged(float* qkv, float* kpool, void* vpool, int v16, const float* cos_tab, const float* sin_tab,
                                           const int32_t* pos0_dev, const int32_t* page_table, int G, int T, int H, int D, int Tmax,
                                           int page_shift, int n_pages, int64_t page_stride, int table_dtype, void* stream) {
  SX_CHECK(page_table, "sx_rope_kv_append_f32_paged: page_table is NULL (the contiguous cache is sx_rope_kv_append_f32 / _v16)");
  SX_CHECK(page_shift >= 5 && page_shift <= 7, "sx_rope_kv_append_f32_paged: page_shift %d (pages hold 32, 64 or 128 rows)", page_shift);
  SX_CHECK(D == 128, "sx_rope_kv_append_f32_paged: head_dim %d (the paged cache exists for head_dim 128 only)", D);
  SX_CHECK(n_pages >= 1 && Tmax >= 1 && page_stride >= ((int64_t)H << page_shift) * D, "sx_rope_kv_append_f32_paged: n_pages=%d Tmax=%d page_stride=%lld "
           "(pools are [n_pages + 1][H][page size][D])", n_pages, Tmax, (long long)page_stride);
  SX_CHECK(v16 == 0 || v16 == 1, "sx_rope_kv_append_f32_paged: v16");
  return rope_kv_f32_impl(qkv, kpool, vpool, v16, cos_tab, sin_tab, pos0_dev, G, T, H, D, Tmax, page_stride, table_dtype, stream, page_table,
                          page_shift, n_pages);
}

extern "C" int sx_rope_kv_append_f32(float* qkv, float* kcache, float* vcache, const float* cos_tab, const float* sin_tab,
                                     const int32_t* pos0_dev, int G, int T, int H, int D, int Tmax, int64_t cache_seq_stride,
                                     int table_dtype, void* stream) {
  return rope_kv_f32_impl(qkv, kcache, vcache, 0, cos_tab, sin_tab, pos0_dev, G, T, H, D, Tmax, cache_seq_stride, table_dtype, stream);
}

extern "C" int sx_rope_kv_append_f32_v16(float* qkv, float* kcache, void* vcache16, const float* cos_tab, const float* sin_tab,
                                         const int32_t* pos0_dev, int G, int T, int H, int D, int Tmax, int64_t cache_seq_stride,
                                         int table_dtype, void* stream) {
  return rope_kv_f32_impl(qkv, kcache, vcache16, 1, cos_tab, sin_tab, pos0_dev, G, T, H, D, Tmax, cache_seq_stride, table_dtype, stream);
}

extern "C" int sx_rope_kv_append_f32_q8(float* qkv, void* kcodes, void* vcodes, float* kscale, float* vscale, const float* cos_tab,
                                        const float* sin_tab, const int32_t* pos0_dev, int G, int T, int H, int D, int Tmax,
                                        int64_t cache_seq_stride, int64_t scale_seq_stride, int table_dtype, int emulate, void* stream) {
  SX_CHECK(qkv && kcodes && vcodes && cos_tab && sin_tab && pos0_dev, "sx_rope_kv_append_f32_q8: null pointer");
  SX_CHECK(D == 128, "sx_rope_kv_append_f32_q8: head_dim %d (the FP8 KV cache exists for head_dim 128 only)", D);
  SX_CHECK(G >= 1 && T >= 1 && H >= 1 && Tmax >= 1, "sx_rope_kv_append_f32_q8: G/T/H/Tmax");
  SX_CHECK(table_dtype == SX_F16 || table_dtype == SX_BF16, "sx_rope_kv_append_f32_q8: table_dtype");
  SX_CHECK(emulate == 0 || emulate == 1, "sx_rope_kv_append_f32_q8: emulate must be 0 (codes + scales) or 1 (dequantised values into fp32 caches)");
  SX_CHECK(emulate || (kscale && vscale && (((uintptr_t)kscale) & 3) == 0 && (((uintptr_t)vscale) & 3) == 0 && scale_seq_stride >= (int64_t)H * Tmax),
           "sx_rope_kv_append_f32_q8: kscale / vscale (fp32 [G][H][Tmax], scale_seq_stride >= H*Tmax) are missing or misaligned");
  SX_CHECK((((uintptr_t)qkv) & 15) == 0 && (((uintptr_t)kcodes) & 15) == 0 && (((uintptr_t)vcodes) & 15) == 0 && cache_seq_stride % 8 == 0 &&
           cache_seq_stride >= (int64_t)H * Tmax * D, "sx_rope_kv_append_f32_q8: qkv / cache pointers and cache_seq_stride must keep 16-B alignment");
  const int64_t rows = (int64_t)G * T * H;
  const dim3 grid((unsigned)((rows + 15) / 16));
#define SX_ROPE_Q8_GO(TT, EM)                                                                                                          \
  hipLaunchKernelGGL((rope_kv_q8_kernel<TT, EM>), grid, dim3(256), 0, ST, qkv, kcodes, vcodes, kscale, vscale, cos_tab, sin_tab, pos0_dev, T, \
                     H, Tmax, G, (long long)cache_seq_stride, (long long)scale_seq_stride)
  if (table_dtype == SX_BF16) { if (emulate) SX_ROPE_Q8_GO(BF16, true); else SX_ROPE_Q8_GO(BF16, false); }
  else { if (emulate) SX_ROPE_Q8_GO(F16, true); else SX_ROPE_Q8_GO(F16, false); }
#undef SX_ROPE_Q8_GO
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}

// the paged launches of sx_attention_f32: the D = 128 forms of the fp32 / mixed cache, one instantiation each beside the contiguous one
template <typename TT, bool V16>
static void attn_f32_paged_launch(const sx_attn_f32_args* a, const AttnF32P& p, bool mfma, void* stream) {
  if (a->T == 1 && a->nsplit > 1) hipLaunchKernelGGL((attn_f32_kernel<TT, 1, 1, V16, true, 0, true>), dim3(a->nsplit, a->H, a->G), dim3(256), 0, ST, p);
  else if (mfma) hipLaunchKernelGGL((attn_f32_mfma_kernel<TT, V16, false, true>), dim3((a->T + 127) / 128, a->H, a->G), dim3(256), 0, ST, p);
  else if (a->T > 8) hipLaunchKernelGGL((attn_f32_kernel<TT, 8, 1, V16, false, 0, true>), dim3((a->T + 7) / 8, a->H, a->G), dim3(256), 0, ST, p);
  else if (a->T == 1) hipLaunchKernelGGL((attn_f32_kernel<TT, 1, 1, V16, false, 0, true>), dim3(1, a->H, a->G), dim3(256), 0, ST, p);
  else hipLaunchKernelGGL((attn_f32_kernel<TT, 4, 1, V16, false, 0, true>), dim3((a->T + 3) / 4, a->H, a->G), dim3(256), 0, ST, p);
}

static int g_attn_f32_mfma = 1;    // 0: chunks above 8 tokens keep the VALU kernel (A/B and the bit-reference of the tests)
extern "C" int sx_attention_f32_variant(int v) {
  SX_CHECK(v == 0 || v == 1, "sx_attention_f32_variant: 0 (VALU kernels only) or 1 (fp32 MFMA kernel for chunks above 8 tokens)");
  g_attn_f32_mfma = v;
  return SX_OK;
}

extern "C" int sx_attention_f32(const sx_attn_f32_args* a, void* stream) {
  SX_CHECK(a && a->q && a->kcache && a->vcache && a->out && (a->pos0_dev || !a->causal), "sx_attention_f32: null pointer");
  const int tiled = (a->dtype & SX_TILED16) ? (int)(((int64_t)a->G * a->T + 15) / 16) : 0, dt = a->dtype & 0xff;   // row blocks of the tiled output
  SX_CHECK(dt == SX_F16 || dt == SX_BF16, "sx_attention_f32: dtype (of the output planes)");
  SX_CHECK(a->D % 8 == 0 && a->D >= 8 && a->D <= 256, "sx_attention_f32: head_dim %d (multiple of 8, <= 256)", a->D);
  SX_CHECK(a->G >= 1 && a->T >= 1 && a->H >= 1 && a->Tmax >= 1, "sx_attention_f32: G/T/H/Tmax");
  SX_CHECK(a->q_row_stride >= (int64_t)a->H * a->D && a->q_row_stride % 4 == 0 && (((uintptr_t)a->q) & 15) == 0, "sx_attention_f32: q_row_stride");
  SX_CHECK(!tiled || ((int64_t)a->G * a->T <= 32 && (a->H * a->D) % 32 == 0), "sx_attention_f32: operand tiles hold <= 32 rows, H*D %% 32 == 0");
  AttnF32P p;
  p.q = a->q; p.kc = a->kcache; p.out = (unsigned short*)a->out; p.pos0_dev = a->pos0_dev;
  p.q_stride = a->q_row_stride; p.seq_stride = a->cache_seq_stride;
  p.row_stride = a->kv_row_stride > 0 ? a->kv_row_stride : a->D;
  p.head_stride = a->kv_head_stride > 0 ? a->kv_head_stride : (int64_t)a->Tmax * a->D;
  p.vc = a->vcache;
  SX_CHECK(p.row_stride % 4 == 0 && p.head_stride % 4 == 0 && p.seq_stride % 4 == 0 && (((uintptr_t)a->kcache) & 15) == 0 &&
           (((uintptr_t)a->vcache) & 15) == 0, "sx_attention_f32: K / V strides and pointers must keep 16-B alignment");
  p.T = a->T; p.H = a->H; p.D = a->D; p.Tmax = a->Tmax; p.tiled = tiled; p.scale = a->scale; p.causal = a->causal ? 1 : 0;
  p.part = a->scratch; p.nsplit = a->nsplit;
  p.cos_t = a->rope_cos; p.sin_t = a->rope_sin; p.knew = a->k_new; p.vnew = a->v_new;
  p.ks = a->k_scale; p.vs = a->v_scale; p.sc_seq_stride = a->scale_seq_stride;
  p.ptab = a->page_table; p.pshift = a->page_shift; p.npages = a->n_pages; p.ptw = 0;
  if (a->page_table) {
    // the paged cache: kcache / vcache are the page pools; only the D = 128 forms of the fp32 / mixed cache read a table
    SX_CHECK(a->D == 128, "sx_attention_f32: a page table needs head_dim 128, not %d (the paged cache has no other form)", a->D);
    SX_CHECK(a->kv_fp8 == 0, "sx_attention_f32: a page table and kv_fp8 exclude each other (paged row scales are not built)");
    SX_CHECK(!(a->rope_cos && a->T > 1), "sx_attention_f32: a page table and the verify form (rope_cos with T > 1) exclude each other (the verify "
             "kernel reads the contiguous cache only)");
    SX_CHECK(a->causal && a->kv_row_stride <= 0 && a->kv_head_stride <= 0, "sx_attention_f32: a page table is the causal form over the pool layout (no K / V strides)");
    SX_CHECK(a->page_shift >= 5 && a->page_shift <= 7, "sx_attention_f32: page_shift %d (pages hold 32, 64 or 128 rows)", a->page_shift);
    SX_CHECK(a->n_pages >= 1 && a->page_stride >= ((int64_t)a->H << a->page_shift) * a->D && a->page_stride % 8 == 0,
             "sx_attention_f32: n_pages=%d page_stride=%lld (pools are [n_pages + 1][H][page size][D], 16-B aligned pages)", a->n_pages, (long long)a->page_stride);
    p.seq_stride = a->page_stride;
    p.head_stride = ((int64_t)1 << a->page_shift) * p.row_stride;
    p.ptw = (a->Tmax + (1 << a->page_shift) - 1) >> a->page_shift;
  }
  // the FP8 KV cache: 1 = codes + row scales, 2 = fp32 caches with quantise-dequantise on append (only the fused RoPE form appends:
  // without it 2 IS the fp32 call, on a cache that already holds dequantised values)
  SX_CHECK(a->kv_fp8 >= 0 && a->kv_fp8 <= 2, "sx_attention_f32: kv_fp8 must be 0 (off), 1 (e4m3 codes + row scales) or 2 (fp32 caches, quantise-dequantise on append)");
  const int kv8 = (a->kv_fp8 == 2 && !a->rope_cos) ? 0 : a->kv_fp8;
  if (a->kv_fp8) {
    SX_CHECK(a->D == 128, "sx_attention_f32: kv_fp8 needs head_dim 128, not %d", a->D);
    SX_CHECK(!a->v16, "sx_attention_f32: kv_fp8 and v16 exclude each other (the FP8 cache holds k AND v as codes)");
    SX_CHECK(a->causal && a->kv_row_stride <= 0 && a->kv_head_stride <= 0, "sx_attention_f32: kv_fp8 is the causal form over the cache layout (no K / V strides)");
  }
  if (kv8 == 1) {
    SX_CHECK(a->k_scale && a->v_scale && (((uintptr_t)a->k_scale) & 3) == 0 && (((uintptr_t)a->v_scale) & 3) == 0 &&
             a->scale_seq_stride >= (int64_t)a->H * a->Tmax, "sx_attention_f32: kv_fp8 = 1 needs k_scale / v_scale (fp32 [G][H][Tmax], 4-B aligned, scale_seq_stride >= H*Tmax)");
    SX_CHECK(p.seq_stride % 16 == 0, "sx_attention_f32: kv_fp8 = 1 needs cache_seq_stride %% 16 == 0 (16-B aligned code rows)");
  }
  if (a->rope_cos) {
    SX_CHECK(a->T >= 1 && a->T <= 8 && a->causal && a->D == 128 && a->rope_sin && a->k_new && a->v_new && a->kv_row_stride <= 0 + (int64_t)a->D,
             "sx_attention_f32: the fused RoPE form is the causal step of T <= 8 rows per sequence at head_dim 128 over the cache layout (rope_sin, k_new, v_new set)");
    SX_CHECK((((uintptr_t)a->k_new) & 15) == 0 && (((uintptr_t)a->v_new) & 15) == 0, "sx_attention_f32: k_new / v_new alignment");
  }
  if (a->page_table) {
    // split + combine for the T = 1 step of few sequences, else the one launch the contiguous cache would get
    // (in front of the contiguous dispatch below: none of its branches reads a table)
    const bool split = a->T == 1 && a->nsplit > 1;
    const bool mfma = g_attn_f32_mfma && a->T > 8 && !tiled && (((uintptr_t)a->out) & 7) == 0 && a->q_row_stride % 4 == 0;   // (causal, D = 128: checked above)
    SX_CHECK(!a->v16 || (p.row_stride % 8 == 0 && p.seq_stride % 8 == 0), "sx_attention_f32: a 16-bit V pool needs 16-B aligned rows");
    SX_CHECK(!split || (a->scratch && a->nsplit <= 64), "sx_attention_f32: key splits need scratch [G][H][nsplit][D + 2] floats and nsplit <= 64");
    SX_CHECK(a->v16 == 0 || a->v16 == 1, "sx_attention_f32: v16");
    if (dt == SX_BF16) { if (a->v16) attn_f32_paged_launch<BF16, true>(a, p, mfma, stream); else attn_f32_paged_launch<BF16, false>(a, p, mfma, stream); }
    else { if (a->v16) attn_f32_paged_launch<F16, true>(a, p, mfma, stream); else attn_f32_paged_launch<F16, false>(a, p, mfma, stream); }
    SX_HIP_LAUNCH_CHECK();
    if (split) {
      if (dt == SX_BF16) hipLaunchKernelGGL(attn_f32_combine_kernel<BF16>, dim3(a->H, a->G), dim3(128), 0, ST, p);
      else hipLaunchKernelGGL(attn_f32_combine_kernel<F16>, dim3(a->H, a->G), dim3(128), 0, ST, p);
      SX_HIP_LAUNCH_CHECK();
    }
    return SX_OK;
  }
  if (a->rope_cos && a->T > 1) {
    // the verify form: T = K + 1 rows per sequence, key splits + combine over G*T rows (nsplit = 1 included: one split per row)
    SX_CHECK(a->kv_fp8 == 0, "sx_attention_f32: the verify form (rope_cos with T > 1) has no FP8 KV cache");
    SX_CHECK((int64_t)a->G * a->T <= 32, "sx_attention_f32: the verify form carries G*T <= 32 rows, not %lld", (long long)a->G * a->T);
    SX_CHECK(a->scratch && a->nsplit >= 1 && a->nsplit <= 64, "sx_attention_f32: the verify form needs nsplit in 1..64 and scratch [G*T][H][nsplit][D + 2] floats");
    SX_CHECK(a->kv_head_stride <= 0 || a->kv_head_stride >= (int64_t)a->Tmax * p.row_stride, "sx_attention_f32: kv_head_stride");
    SX_CHECK(!a->v16 || (a->v16 == 1 && p.row_stride % 8 == 0 && p.head_stride % 8 == 0 && p.seq_stride % 8 == 0),
             "sx_attention_f32: a 16-bit V cache needs 16-B aligned rows");
    const dim3 grid(a->nsplit, a->H, a->G);
#define SX_VERIFY_GO(TT, TQ, V16) hipLaunchKernelGGL((attn_f32_verify_kernel<TT, TQ, V16>), grid, dim3(256), 0, ST, p)
#define SX_VERIFY_TQ(TT, V16) do { if (a->T <= 4) SX_VERIFY_GO(TT, 4, V16); else SX_VERIFY_GO(TT, 8, V16); } while (0)
    if (dt == SX_BF16) { if (a->v16) SX_VERIFY_TQ(BF16, true); else SX_VERIFY_TQ(BF16, false); }
    else { if (a->v16) SX_VERIFY_TQ(F16, true); else SX_VERIFY_TQ(F16, false); }
#undef SX_VERIFY_TQ
#undef SX_VERIFY_GO
    SX_HIP_LAUNCH_CHECK();
    if (dt == SX_BF16) hipLaunchKernelGGL(attn_f32_combine_kernel<BF16>, dim3(a->H, a->G * a->T), dim3(128), 0, ST, p);
    else hipLaunchKernelGGL(attn_f32_combine_kernel<F16>, dim3(a->H, a->G * a->T), dim3(128), 0, ST, p);
    SX_HIP_LAUNCH_CHECK();
    return SX_OK;
  }
  if (a->T == 1 && a->nsplit > 1) {
    // the decode step of few sequences: key splits + combine (two launches)
    SX_CHECK(a->scratch && a->causal && a->D <= 128 && a->nsplit <= 64 && (!a->v16 || (p.row_stride % 8 == 0 && p.head_stride % 8 == 0 && p.seq_stride % 8 == 0)),
             "sx_attention_f32: key splits need scratch [G][H][nsplit][D + 2] floats, a causal T = 1 call and head_dim <= 128");
    p.vc = a->vcache;
    const dim3 grid(a->nsplit, a->H, a->G);
#define SX_SPLIT_GO(TT, V16) hipLaunchKernelGGL((attn_f32_kernel<TT, 1, 1, V16, true>), grid, dim3(256), 0, ST, p)
#define SX_SPLIT8_GO(TT, KV8) hipLaunchKernelGGL((attn_f32_kernel<TT, 1, 1, false, true, KV8>), grid, dim3(256), 0, ST, p)
    if (kv8) {
      if (dt == SX_BF16) { if (kv8 == 1) SX_SPLIT8_GO(BF16, 1); else SX_SPLIT8_GO(BF16, 2); }
      else { if (kv8 == 1) SX_SPLIT8_GO(F16, 1); else SX_SPLIT8_GO(F16, 2); }
    } else
    if (dt == SX_BF16) { if (a->v16) SX_SPLIT_GO(BF16, true); else SX_SPLIT_GO(BF16, false); }
    else { if (a->v16) SX_SPLIT_GO(F16, true); else SX_SPLIT_GO(F16, false); }
#undef SX_SPLIT_GO
#undef SX_SPLIT8_GO
    SX_HIP_LAUNCH_CHECK();
    if (dt == SX_BF16) hipLaunchKernelGGL(attn_f32_combine_kernel<BF16>, dim3(a->H, a->G), dim3(128), 0, ST, p);
    else hipLaunchKernelGGL(attn_f32_combine_kernel<F16>, dim3(a->H, a->G), dim3(128), 0, ST, p);
    SX_HIP_LAUNCH_CHECK();
    return SX_OK;
  }
  const bool mfma = g_attn_f32_mfma && a->causal && a->T > 8 && a->D == 128 && !tiled && (((uintptr_t)a->out) & 7) == 0 &&
                    p.row_stride % 4 == 0 && a->q_row_stride % 4 == 0;
  if (mfma) {
    p.vc = a->vcache;
    const dim3 grid((a->T + 127) / 128, a->H, a->G);
    if (kv8 == 1) {
      if (dt == SX_BF16) hipLaunchKernelGGL((attn_f32_mfma_kernel<BF16, false, true>), grid, dim3(256), 0, ST, p);
      else hipLaunchKernelGGL((attn_f32_mfma_kernel<F16, false, true>), grid, dim3(256), 0, ST, p);
    } else if (a->v16) {
      SX_CHECK(p.row_stride % 8 == 0 && p.head_stride % 8 == 0 && p.seq_stride % 8 == 0, "sx_attention_f32: 16-bit V rows must be 16-B aligned");
      if (dt == SX_BF16) hipLaunchKernelGGL((attn_f32_mfma_kernel<BF16, true>), grid, dim3(256), 0, ST, p);
      else hipLaunchKernelGGL((attn_f32_mfma_kernel<F16, true>), grid, dim3(256), 0, ST, p);
    } else {
      if (dt == SX_BF16) hipLaunchKernelGGL((attn_f32_mfma_kernel<BF16, false>), grid, dim3(256), 0, ST, p);
      else hipLaunchKernelGGL((attn_f32_mfma_kernel<F16, false>), grid, dim3(256), 0, ST, p);
    }
    SX_HIP_LAUNCH_CHECK();
    return SX_OK;
  }
  if (kv8) {
    // the FP8 cache (1), or the fused RoPE form of its fp32 twin (2: T == 1 by the check above)
#define SX_KV8_GO(TT, QB, KV8) hipLaunchKernelGGL((attn_f32_kernel<TT, QB, 1, false, false, KV8>), dim3((a->T + QB - 1) / QB, a->H, a->G), dim3(256), 0, ST, p)
    if (kv8 == 2) {
      if (dt == SX_BF16) SX_KV8_GO(BF16, 1, 2); else SX_KV8_GO(F16, 1, 2);
    } else if (a->T > 8) {
      if (dt == SX_BF16) SX_KV8_GO(BF16, 8, 1); else SX_KV8_GO(F16, 8, 1);
    } else if (a->T == 1) {
      if (dt == SX_BF16) SX_KV8_GO(BF16, 1, 1); else SX_KV8_GO(F16, 1, 1);
    } else {
      if (dt == SX_BF16) SX_KV8_GO(BF16, 4, 1); else SX_KV8_GO(F16, 4, 1);
    }
#undef SX_KV8_GO
    SX_HIP_LAUNCH_CHECK();
    return SX_OK;
  }
  if (a->v16) {
    // mixed cache: V in the planes' 16-bit dtype (head_dim <= 128: the decoder's; the resamplers' fp32 views keep the fp32 form)
    SX_CHECK(a->v16 == 1 && a->D <= 128 && p.row_stride % 8 == 0 && p.head_stride % 8 == 0 && p.seq_stride % 8 == 0,
             "sx_attention_f32: a 16-bit V cache needs head_dim <= 128 and 16-B aligned rows");
    if (a->T > 8) {
      const dim3 grid((a->T + 7) / 8, a->H, a->G);
      if (dt == SX_BF16) hipLaunchKernelGGL((attn_f32_kernel<BF16, 8, 1, true>), grid, dim3(256), 0, ST, p);
      else hipLaunchKernelGGL((attn_f32_kernel<F16, 8, 1, true>), grid, dim3(256), 0, ST, p);
    } else if (a->T == 1) {       // the decode step: ONE query row per workgroup (QB = 4 computes four rows' dot products per key for one valid row)
      const dim3 grid(1, a->H, a->G);
      if (dt == SX_BF16) hipLaunchKernelGGL((attn_f32_kernel<BF16, 1, 1, true>), grid, dim3(256), 0, ST, p);
      else hipLaunchKernelGGL((attn_f32_kernel<F16, 1, 1, true>), grid, dim3(256), 0, ST, p);
    } else {
      const dim3 grid((a->T + 3) / 4, a->H, a->G);
      if (dt == SX_BF16) hipLaunchKernelGGL((attn_f32_kernel<BF16, 4, 1, true>), grid, dim3(256), 0, ST, p);
      else hipLaunchKernelGGL((attn_f32_kernel<F16, 4, 1, true>), grid, dim3(256), 0, ST, p);
    }
    SX_HIP_LAUNCH_CHECK();
    return SX_OK;
  }
  if (a->D > 128) {             // two 8-dim chunks per lane (the LLM-side resamplers' head_dim 160): 4 rows per workgroup
    const dim3 grid((a->T + 3) / 4, a->H, a->G);
    if (dt == SX_BF16) hipLaunchKernelGGL((attn_f32_kernel<BF16, 4, 2>), grid, dim3(256), 0, ST, p);
    else hipLaunchKernelGGL((attn_f32_kernel<F16, 4, 2>), grid, dim3(256), 0, ST, p);
  } else if (a->T > 8) {
    const dim3 grid((a->T + 7) / 8, a->H, a->G);
    if (dt == SX_BF16) hipLaunchKernelGGL((attn_f32_kernel<BF16, 8, 1>), grid, dim3(256), 0, ST, p);
    else hipLaunchKernelGGL((attn_f32_kernel<F16, 8, 1>), grid, dim3(256), 0, ST, p);
  } else if (a->T == 1) {
    const dim3 grid(1, a->H, a->G);
    if (dt == SX_BF16) hipLaunchKernelGGL((attn_f32_kernel<BF16, 1, 1>), grid, dim3(256), 0, ST, p);
    else hipLaunchKernelGGL((attn_f32_kernel<F16, 1, 1>), grid, dim3(256), 0, ST, p);
  } else {
    const dim3 grid((a->T + 3) / 4, a->H, a->G);
    if (dt == SX_BF16) hipLaunchKernelGGL((attn_f32_kernel<BF16, 4, 1>), grid, dim3(256), 0, ST, p);
    else hipLaunchKernelGGL((attn_f32_kernel<F16, 4, 1>), grid, dim3(256), 0, ST, p);
  }
  SX_HIP_LAUNCH_CHECK();
  return SX_OK;
}
