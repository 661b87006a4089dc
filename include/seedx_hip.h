/*
 * seedx_hip.h — C-ABI of libseedx_hip.so: the hand-written gfx950 (MI355X / CDNA4) kernels behind the
 * SEED-X inference hot path (ViT visual encoder → Llama-style LLM prefill/decode → SDXL-adapter UNet loop).
 *
 * The reference (AILab-CVC/SEED-X) has NO native layer: every op below replaces a stock
 * PyTorch / xformers / diffusers call made from the reference's Python modules. Each entry cites the
 * reference call site (file:line under the reference tree) it stands in for. The Python host in
 * `seed-x_amd/` binds these with ctypes (INTEGRATION.md shows the stub a reference maintainer would add).
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless a name ends in `_host`
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every call only ENQUEUES work
 *   - return value: 0 (SX_OK) on success; non-zero on error, message via sx_last_error()
 *   - 16-bit activations/weights are fp16 or bf16 selected by `dtype`; accumulation is always fp32
 *   - row-major everywhere; weights are [N][K] (torch nn.Linear layout), conv weights [Cout][3][3][Cin]
 */
#ifndef SEEDX_HIP_H
#define SEEDX_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SX_OK 0
#define SX_ERR_INVALID 1
#define SX_ERR_HIP 2

/* element types */
#define SX_F16 0
#define SX_BF16 1
#define SX_F32 2
#define SX_BF16X3 3 /* sx_groupnorm* outputs only: bf16 planes [hi | hi | lo] per row, 3*C columns (see sx_split_bf16) */
#define SX_F16X2 4  /* sx_groupnorm* outputs only: fp16 planes [hi | lo] per row, 2*C columns (sx_split16's row layout): the A operand
                     * of the fp32-grade VAE convs whose weights are exact in fp16 (W duplicated per tap: A.W = Ah.W + Al.W) */
#define SX_FP8_E4M3 5 /* sx_gemv_args.w_dtype only: OCP e4m3fn weight codes (1-4-3, bias 7, no infinities; the NaN codes 0x7f / 0xff never
                       * occur) with one fp32 scale per weight row, W[n][k] = decode(code[n][k]) * w_scale[n] */
#define SX_FP4_E2M1 6 /* sx_gemv_args.w_dtype only: OCP MXFP4 weight codes (e2m1: sign + magnitudes 0, .5, 1, 1.5, 2, 3, 4, 6; two per byte)
                       * with one E8M0 scale byte per block of 32 consecutive k of a row, W[n][k] = decode(code[n][k]) * 2^(byte - 127) */
/* OR-ed into a 16-bit OUTPUT dtype of the decode-step producers (sx_layernorm with rows <= 32, sx_attn_decode_b, sx_gemv):
 * the [rows <= 32][cols] result is written as MFMA operand tiles [rows/16][cols/32][16][32] — what sx_gemv reads with x_layout = 1
 * (tile t = columns 32t .. 32t+31 of all 16 rows, 1 KB contiguous; rows >= `rows` of a tile are not written). */
#define SX_TILED16 0x100

/* epilogue activations */
#define SX_ACT_NONE 0
#define SX_ACT_GELU 1 /* exact erf GELU  == torch.nn.GELU()            (qwen_visual.py:253-255) */
#define SX_ACT_SILU 2 /* x*sigmoid(x)   == ACT2FN["silu"]             (modeling_llama_xformer.py:152-167) */

/* A-operand addressing modes of sx_gemm */
#define SX_A_LINEAR 0  /* A is [M][K] row-major                                                   */
#define SX_A_CONV3X3 1 /* A is an NHWC image, implicit im2col of a 3x3 / pad 1 convolution        */

const char* sx_last_error(void);
int sx_version(void);

/* ------------------------------------------------------------------------------------------------
 * GEMM / implicit-GEMM conv on MFMA:  C[M][N] = epilogue( A[M][K] · W[N][K]^T )
 * replaces: nn.Linear everywhere on the path (qwen_visual.py:176-177,253-255,115;
 *           modeling_llama_xformer.py:160-167,184-187,707; resampler.py:12-15,42-44,237,257-258),
 *           nn.Conv2d 3x3 inside diffusers UNet2DConditionModel [ext] (call site
 *           pipeline_stable_diffusion_xl_t2i_edit.py:915-922), F.interpolate(nearest 2x)+conv and the
 *           stride-2 Downsample2D conv of the same UNet.
 * epilogue order: v = acc; v += bias[n]; v += bias2d[(m / bias2d_rows)][n]; if(glu) v = first*act(second)
 *                 else v = act(v); v += residual[(res_mod? m % res_mod : m)][n_out]; store as out_dtype.
 * glu: W rows are packed in 32-row groups [16 "linear" rows | 16 "gate" rows]; output has N/2 columns.
 * ------------------------------------------------------------------------------------------------ */
typedef struct sx_gemm_args {
  const void* A;         /* 16-bit, LINEAR: [M][K]; CONV3X3: [B][Hin][Win][Cin]                    */
  const void* W;         /* 16-bit, [N][K]   (CONV3X3: K = 9*Cin ordered (ky,kx,cin); upsample = 2: [4][N][4*Cin]) */
  void* C;               /* [M][N_out] of out_dtype, row stride ldc elements                        */
  const float* bias;     /* [N] fp32 or NULL                                                        */
  const float* bias2d;   /* [M / bias2d_rows][N] fp32 or NULL  (per-sample time-embedding add)      */
  const float* residual; /* fp32 [.][N_out] row stride ldr, or NULL                                 */
  int32_t M, N, K;
  int32_t ldc, ldr;
  int32_t n_valid;     /* 0 = all; else only output columns < n_valid are stored (multiple of 4)    */
  int32_t res_mod;     /* 0 = residual row m; >0 = residual row m % res_mod (pos-embed broadcast)    */
  int32_t bias2d_rows; /* rows of C per bias2d row                                                   */
  int32_t dtype;       /* SX_F16 / SX_BF16 : type of A and W                                         */
  int32_t out_dtype;   /* SX_F16 / SX_BF16 / SX_F32                                                  */
  int32_t act;         /* SX_ACT_*                                                                   */
  int32_t glu;         /* 0/1                                                                        */
  int32_t a_mode;      /* SX_A_*                                                                     */
  /* conv geometry (a_mode == SX_A_CONV3X3): M = B*Hout*Wout, K = 9*Cin */
  int32_t B, Hin, Win, Cin, Hout, Wout;
  int32_t stride;   /* 1 or 2 (padding: see pad_mode)                                                */
  int32_t upsample; /* 1 = input is nearest-2x upsampled on the fly (Hout = 2*Hin)
                       2 = the same convolution from PHASE-PACKED weights: output parity (a, c) = phase 2a + c sees only 2 x 2 distinct
                       source pixels, so the 3x3 taps that share one are summed at pack time (16 products per input pixel, not 36):
                         W[2a + c][n][(2u + v) Cin + ch] = sum_{ky in R(a,u)} sum_{kx in R(c,v)} w[n][ky][kx][ch],
                         R(0,0) = {0}, R(0,1) = {1,2}, R(1,0) = {0,1}, R(1,1) = {2}
                         y[b][2i + a][2j + c][n] = bias[n] + sum_{u,v,ch} W[2a + c][n][(2u + v) Cin + ch] x[b][i + a - 1 + u][j + c - 1 + v][ch]
                       K = 4*Cin, M = 4*B*Hin*Win = B*Hout*Wout (GEMM rows run (phase, b, i, j); C is still the [B][Hout][Wout][N] image),
                       stride 1, pad_mode 0, no residual, no fused GroupNorm statistics (sx_gemm_gn fails); bias2d_rows = Hout*Wout.
                       Ping-pong 256-row tiles only: fails unless B*Hin*Win % 256 == 0 (a tile lies inside one phase) — such shapes
                       keep upsample = 1 */
  int32_t ld_bias2d; /* row stride of bias2d in floats (0 = N): lets one GEMM produce every resnet's time add    */
  int32_t pad_mode; /* 0 = zero pad 1 on every side; 1 = pad 0 top/left and 1 bottom/right (diffusers Downsample2D with
                       padding=0 + F.pad(x, (0,1,0,1)): the stride-2 convs of the VAE encoder [ext])                 */
  int32_t a_planes; /* 0 / 1: A is [M][K]. 2 (SX_A_LINEAR only): A is [M][2K] = [hi(K) | lo(K)], the two 16-bit planes of an
                       fp32-grade activation x = hi + lo (sx_split16 / sx_rmsnorm_planes / sx_attention_f32 write them); W stays
                       [N][K] and its k-tiles are walked twice: C = epilogue((hi + lo) W^T), fp32 accumulation, no extra weight
                       bytes. The Llama decoder's precise mode (modeling_llama_xformer.py:204-206,239,166-167,707 at 1e-3 of fp32) */
} sx_gemm_args;
int sx_gemm(const sx_gemm_args* args, void* stream);
/* sx_gemm + the statistics pass of the GroupNorm that reads its output (diffusers ResnetBlock2D.norm2 / Transformer2DModel.norm /
 * conv_norm_out [ext] after conv1 / conv2 / proj_out; call site pipeline_stable_diffusion_xl_t2i_edit.py:915-922), fused into the
 * GEMM epilogue: stats[row / rows_per_sample][column / (N / groups)][2] (fp64, host-zeroed or pre-accumulated) += (sum, sum of
 * squares) of the stored fp32 output. Only the 256-row ping-pong tiles carry it: *fused_host = 1 if this launch accumulated,
 * 0 if the GEMM ran unchanged (then run sx_groupnorm's own statistics pass). */
int sx_gemm_gn(const sx_gemm_args* args, double* stats, int groups, int rows_per_sample, int* fused_host, void* stream);
/* A LayerNorm folded into the GEMMs either side of it (reference: every `norm1/2/3 → to_q / to_k / to_v / ff.net[0]` pair of the SDXL
 * transformer blocks [ext BasicTransformerBlock], called per step from pipeline_stable_diffusion_xl_t2i_edit.py:915-922).
 *   PRODUCER launch (row_stats_out != NULL; plain fp32 output, e.g. the attention out-projection + residual): besides C it stores
 *     x16_out[M][ld_x16] = C rounded to the operand dtype and adds every row's (sum, sum of squares) over this launch's columns to
 *     row_stats_out[M][2] (fp64 atomics; zero beforehand).
 *   CONSUMER launch (row_stats_in != NULL; A = that x16 copy, W = the weight with gamma folded in, bias = b + W beta):
 *     out = epilogue(rstd_m * (A W'^T - mu_m * colsum) + bias), mu / rstd of row m from row_stats_in (complete), colsum[n] = sum_k W'[n][k].
 * Ping-pong 256-row tiles only: fails (SX_ERR_INVALID) for a shape the cost model gives a lock-step tile — sx_gemm_pick_tile(...) >= 7
 * says beforehand; such shapes keep the separate sx_layernorm launch. */
typedef struct sx_gemm_ln_args {
  void* x16_out;               /* producer */
  double* row_stats_out;
  const double* row_stats_in;  /* consumer */
  const float* colsum;
  int32_t ld_x16;
  int32_t dim;                 /* LayerNorm width (= K of the consumer) */
  float eps;
  int32_t reserved;
} sx_gemm_ln_args;
int sx_gemm_ln(const sx_gemm_args* args, const sx_gemm_ln_args* ln, void* stream);
/* tuning/test hook: force tile config 0..8 (lock-step 128x128, 128x80, 64x128, 64x64, 256x256, 256x320, 256x160; ping-pong
 * 256x256, 256x320 — the two-wave-group schedule of csrc/gemm_pp.hip); -1 = automatic (cost model); 100/101 = 2-D XCD
 * partition off/on; 300+g (g = 0..64) = g tile-rows per in-XCD traversal group (300 = default). Any other value fails
 * (SX_ERR_INVALID) and changes nothing. */
int sx_gemm_force_tile(int cfg);
/* tuning hook: `buf` = device buffer of 4 x uint64 per workgroup; following sx_gemm launches store s_memtime stamps
 * {start, first k-tile landed, main loop done, end} per workgroup (tools/gemm_phase_probe.py). NULL switches it off. */
int sx_gemm_debug_stamps(void* buf);
/* host-only query (no launch): tile config 0..8 the cost model picks for an M x N x K problem (glu / conv3x3 flags) */
int sx_gemm_pick_tile(int M, int N, int K, int glu, int conv);

/* 1..32-row GEMV for single-token decode of up to 32 lock-step sequences (HBM-bound weight streaming).
 * replaces: the same nn.Linear calls at q_len == 1 (modeling_llama_xformer.py:204-206,239,166-167,707).
 * y[m][n_out] = epi( x[m][K] · W[N][K]^T ), x 16-bit, y out_dtype, residual fp32. glu packing as above.
 * M <= 4 (or K % 64 != 0 / N % 32 != 0, then M <= 8): one wave per 2 rows, VALU dot products.
 * M >= 5: the weight rows feed a 16x16x32 MFMA against x^T padded to 16 columns (cost independent of M); M = 17..32: two such
 * column blocks per weight fragment — the weights still stream once (tiled operands: [2][K/32][16][32], rows 16..31 in block 1). */
typedef struct sx_gemv_args {
  const void* x;
  const void* W;
  void* y;
  const float* residual;
  int32_t M, N, K;
  int32_t dtype, out_dtype, act, glu;
  int32_t w_layout;    /* 0: W row-major [N][K]. 1: decode tiles [N/16][K/32][16][32] (each 16-row x 32-k MFMA operand tile
                        * is 1 KB contiguous, tiles of a row group follow each other along K): MFMA path only (M >= 2).
                        * 2: 20-row decode tiles [N/20][K/32][20][32] (no GLU, N % 20 == 0): one workgroup per 20 rows — for
                        * N = 5120 that is 256 equal workgroups on the 256 CUs instead of 320 16-row groups (o / down projections) */
  int32_t x_layout;    /* 0: x row-major [M][K]. 1: operand tiles [K/32][16][32] (tile t holds x[0..15][32t .. 32t+31], rows >= M
                        * are padding with ARBITRARY content (uninitialised is fine, NaN bit patterns included): an MFMA output column depends
                        * only on its own operand column and columns >= M are never stored; 16 * K elements in all): MFMA path only */
  void* workspace;     /* optional, MFMA path: device scratch for split-K over workgroups (shapes whose N / 16 row groups do not
                        * fill the chip). Layout: 16 KB of arrival counters, then the partial sums. Must be ZERO when first used
                        * and is left with its counters at zero. A split into S workgroups (S <= 8) needs
                        * bytes >= 16384 + S * 16 * MB * N * 4, MB = the 16-row x blocks per weight fragment: 1 for M <= 16, 2 for
                        * M = 17..32 or x_planes = 2, 4 for both — so 16384 + 8 * 16 * MB * N * 4 allows every split factor (smaller than
                        * the chosen factor needs: no split, nothing past workspace_bytes is touched). One launch at a time per
                        * workspace (launches on one stream are fine). NULL: never split. Results are deterministic either way
                        * (partials are added in split order by the last workgroup to arrive). */
  uint64_t workspace_bytes;
  /* RMSNorm folded into the decode step's skinny GEMMs (MFMA path only; all NULL / 0 = off). LlamaRMSNorm (modeling_llama_xformer.py:95,
   * 286, 301) is y = x * rsqrt(mean(x^2) + eps) * gamma: gamma is folded into the NEXT projection's weights at load time and
   * rsqrt(...) is a per-row scalar, so the norm needs no pass of its own —
   *   producer (a GEMV with an fp32 residual output = the new residual stream x): also stores x as 16-bit operand tiles
   *     [N/32][16][32] (`x16_out`, the next GEMV's x with x_layout = 1) and, per workgroup p, the rows' sums of squares over its own
   *     columns (`row_ssq_out`[16][parts], parts = the launch's workgroups in x = sx_gemv_ssq_parts(N, glu, w_layout); the consumer needs parts % 64 == 0: 320 / 256 for N = 5120);
   *   consumer: multiplies its accumulators by rsqrt(sum_p row_ssq_in[m][p] / ssq_dim + ssq_eps) before activation / GLU / store
   *     (the partials are added in the fixed order p = 0, 1, ...: every workgroup computes the same scale). */
  void* x16_out;
  float* row_ssq_out;
  const float* row_ssq_in;
  int32_t ssq_in_parts, ssq_dim;
  float ssq_eps;
  int32_t x_planes;    /* 0 / 1: x is one 16-bit activation. 2 (x_layout 1, MFMA path at any M >= 1): x holds the two planes of an
                        * fp32-grade activation as operand blocks [2 planes][RB][K/32][16][32], RB = ceil(M / 16) row blocks of 16 rows —
                        * the hi plane's row blocks, then the lo plane's (sx_split16 / sx_rmsnorm_planes / sx_attention_f32 with
                        * SX_TILED16): every weight fragment feeds 2 RB MFMAs (M <= 16: two, M = 17..32, round 6: four) and the lo
                        * products are added to the hi products ahead of the epilogue — the weights stream once, y = epi((hi + lo) W^T) */
  int32_t out_planes;  /* 1: the tiled 16-bit output (SX_TILED16) or x16_out is written as two planes [2][RB][cols/32][16][32]
                        * (hi = rn16(v), lo = rn16(v - hi)): the next sx_gemv's x with x_planes = 2, without a sx_split16 launch */
  const float* x16_gamma; /* optional fp32 [N] with x16_out: x16_out holds o * gamma (the NEXT LlamaRMSNorm's weight applied on the
                        * activation side, so that the next projection keeps its exact checkpoint weights and only scales by rstd from
                        * row_ssq_in — the RMSNorm fold of the precise mode; row_ssq_out is still the sum of squares of o itself) */
  int32_t w_dtype;     /* 0: W has the activation dtype. SX_FP8_E4M3: W holds one-byte e4m3 codes in the FP8 form of w_layout 1 or 2 (MFMA path
                        * only, any other combination is SX_ERR_INVALID):
                        *   w_layout 1: [N/16][K/64][16][64] — a 64-k slab of 16 rows is one 1-KB tile; inside a row the 64 codes are ordered
                        *     so that byte 16 g + 8 h + j holds k = 64 t + 32 h + 8 g + j (g = 0..3, h = 0..1, j = 0..7): lane (row r, group g)
                        *     of the 16x16x32 MFMA finds its eight k-slots of BOTH 32-k halves in the one 16-B load at byte 64 r + 16 g,
                        *   w_layout 2: [N/20][K/64][20][64] — the same 1-KB tile of rows 0..15, then rows 16..19 (256 B) in the same byte order.
                        * The codes are converted to the activation dtype in registers (exact for every code) and feed the same MFMAs as
                        * 16-bit tiles; the products are summed in fp32 exactly as for 16-bit weights of value decode(code). */
  const float* w_scale; /* with SX_FP8_E4M3 (else NULL): fp32 [N], 16-B aligned, in the row order of W as passed (GLU-packed rows: packed
                        * order). Multiplies the summed accumulators of row n once — after the wave, split-K and plane sums, before rstd
                        * (row_ssq_in), activation, GLU, residual and the plane / sum-of-squares outputs. A power-of-two scale commutes with
                        * every fp32 rounding: the result then has the bits of the 16-bit kernel on the weights code * scale. */
  const void* w_block_scale; /* with w_dtype = SX_FP4_E2M1 (else NULL; w_scale must then be NULL): the E8M0 block scales of the MXFP4 form
                        * of w_layout 1 or 2 (MFMA path only; row-major W, a missing or not 16-B aligned scale array, a shape outside the
                        * MFMA path or w_scale set are SX_ERR_INVALID, never a fall-back). The kernel keeps its 64-k step:
                        *   W, w_layout 1: [N/16][K/64][16][32 B] — a 64-k slab of 16 rows is one 512-B tile; byte 8 g + 4 h + i of a row
                        *     holds k = 64 t + 32 h + 8 g + 2 i in its low nibble and k + 1 in its high one (g = 0..3, h = 0..1, i = 0..3):
                        *     lane (row r, group g) of the 16x16x32 MFMA loads the 8 bytes at 32 r + 8 g, dword h = its eight k-slots of
                        *     32-k half h in nibble order, all in ONE 32-k block — one scale per dword,
                        *   W, w_layout 2: [N/20][K/64][20][32 B] — the 512-B tile of rows 0..15, then rows 16..19 (128 B), same byte order,
                        *   w_block_scale, w_layout 1: [N/16][K/64][16][2] bytes, byte h of (row r, k-step t) = the E8M0 byte of block 2 t + h
                        *     of that row (one 2-B load per lane and k-step); w_layout 2: [N/20][K/64][20][2], rows 16..19 behind rows 0..15.
                        * Rows are in the order of W as passed (GLU-packed rows: packed order). Each dword becomes four packed converts
                        * (v_cvt_scalef32_pk_{f16,bf16}_fp4, the block scale applied in the convert: every code * 2^e with e in [-13, 13] is
                        * a normal fp16 / bf16 number, so the operand is exact) in front of the same MFMAs, k-slices and epilogue as the
                        * 16-bit tiles: the result has the bits of the 16-bit kernel on the dequantised weights. No row scale. */
  /* Pre-activation addend (MFMA path only — every w_dtype, w_layout 1 and 2, every x block count and split-K; SX_ERR_INVALID on the
   * VALU path; all NULL / 0 = off, the launch is then exactly the one without these fields). The unmerged LoRA delta of sx_lora_expand:
   * row m's summed accumulator gets addend[m][n] added AFTER the wave, split-K and plane sums, w_scale and rstd (row_ssq_in) and BEFORE
   * activation, GLU and residual — y = epi(acc + addend). A row that does not take its addend keeps the bits of a launch without one,
   * and nothing of addend is read for it. */
  const float* addend;       /* fp32 [M][N], 16-B aligned, columns in the row order of W as passed (GLU-packed rows: packed order)         */
  const int32_t* addend_sel; /* device int32 [M] or NULL. NULL: every row takes its addend; else row m iff addend_sel[m] in [0, addend_n) */
  int32_t addend_n;          /* with addend_sel: the adapter count (>= 1), so that the rows sx_lora_expand left unwritten are skipped; else 0 */
} sx_gemv_args;
/* workgroups in x (= partial rows of row_ssq_out) sx_gemv launches for an M x N x K problem with / without GLU on the MFMA path */
int sx_gemv_ssq_parts(int N, int glu, int w_layout);
int sx_gemv(const sx_gemv_args* args, void* stream);
/* host only, nothing is launched: the launch sx_gemv would make for these args under the current hooks (same checks, same status), for
 * every weight format and both paths — plan[0] = path (0 VALU, 1 MFMA skinny), plan[1] = workgroups in x, plan[2] = split-K factor
 * (grid y), plan[3..6] = the kernel family (R, U, TAIL, MB) of gemm_skinny_kernel (VALU: MR of gemv_kernel, 0, 0, 0), plan[7] = w_dtype
 * as passed */
int sx_gemv_plan(const sx_gemv_args* args, int32_t* plan);
/* test hook: 1 = always take the VALU path (lets the tests compare both), 0 = automatic */
int sx_gemv_force_valu(int on);
/* tuning hook (tools/lab/gemv_lab): key 2 = split-K factor of the MFMA skinny GEMM when a workspace is given:
 * 0 automatic, -1 / 1 never, 2 / 4 / 8 forced; key 1 = 1: the 17..32-row kernels with 4 k-steps per round (default 2) */
int sx_gemv_tune(int key, int value);

/* ------------------------------------------------------------------------------------------------
 * Normalisations (row reductions with wave shuffles, fp32 statistics)
 * ------------------------------------------------------------------------------------------------ */
/* LayerNorm over the last dim. replaces nn.LayerNorm (qwen_visual.py:246,250,361,384,122-123;
 * resampler.py:11,38-39,240) and diffusers BasicTransformerBlock.norm1/2/3 [ext].
 * rms != 0 → LlamaRMSNorm (modeling_llama_xformer.py:95,286,301,595): y = x * rsqrt(mean(x^2)+eps) * gamma */
int sx_layernorm(const void* x, int in_dtype, void* y, int out_dtype, const float* gamma, const float* beta,
                 int rows, int cols, float eps, int rms, void* stream);

/* Row softmax y = softmax(scale * x) over the last dim, fp32 in → 16-bit out (probabilities feed the P·V GEMM) or fp32
 * out (SX_F32, ldy in floats: the fp32-grade VAE mode splits it into bf16 planes).
 * replaces: the softmax inside diffusers Attention [ext] of the VAE decoder's mid block (one 512-wide head over
 * (H/8)·(W/8) pixels — head_dim 512 does not fit the flash kernel, so scores go through sx_gemm; reference call site
 * pipeline_stable_diffusion_xl_t2i_edit.py:973). */
int sx_softmax_rows(const float* x, int64_t ldx, void* y, int64_t ldy, int rows, int cols, float scale, int out_dtype,
                    void* stream);

/* GroupNorm(+SiLU) over NHWC activations x[B][HW][C] (fp32 in). replaces diffusers
 * ResnetBlock2D.norm1/norm2 + nonlinearity, Transformer2DModel.norm, conv_norm_out [ext].
 * stats: scratch fp64 [B][groups][2] (zeroed by the call). y: 16-bit normalised output; SX_F32 is accepted when raw16 is
 * NULL; SX_BF16X3 writes y (and raw16) as [B][HW][3*C] bf16 planes, SX_F16X2 as [B][HW][2*C] fp16 planes: the A operands of the
 * fp32-grade VAE mode.
 * raw16: optional 16-bit un-normalised copy of x (feeds the 1x1 shortcut conv), may be NULL. */
int sx_groupnorm(const float* x, void* y, void* raw16, int out_dtype, const float* gamma, const float* beta,
                 double* stats, int B, int HW, int C, int groups, float eps, int silu, void* stream);
/* same with the input given as the channel concatenation [x | x2] of two NHWC tensors (x: [B][HW][C1], x2: [B][HW][C-C1]):
 * GroupNorm over torch.cat([hidden_states, res_hidden_states], dim=1) of the UNet up blocks (diffusers
 * CrossAttnUpBlock2D / UpBlock2D [ext]) without materialising the concatenation. x2 == NULL: plain sx_groupnorm. */
int sx_groupnorm2(const float* x, const float* x2, int C1, void* y, void* raw16, int out_dtype, const float* gamma,
                  const float* beta, double* stats, int B, int HW, int C, int groups, float eps, int silu, void* stream);
/* tuning hook: key 0 = block count of the GroupNorm statistics pass (0 = chosen by input size, the default) */
int sx_norm_tune(int key, int value);
/* the same split in two calls for pixel-sharded (sequence-parallel) UNet ranks: phase 1 = zero `stats` and accumulate the
 * fp64 sum / sum-of-squares of THIS rank's HW rows per (sample, group); the caller all-reduces `stats` across ranks;
 * phase 2 = normalise this rank's rows with statistics that cover hw_total rows per sample. */
int sx_groupnorm_sp(const float* x, const float* x2, int C1, void* y, void* raw16, int out_dtype, const float* gamma,
                    const float* beta, double* stats, int B, int HW, int hw_total, int C, int groups, float eps, int silu,
                    int phase, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Attention
 * ------------------------------------------------------------------------------------------------ */
/* Flash-style fused attention on MFMA (online softmax in fp32, LDS-staged K / V^T tiles).
 * replaces: bmm→softmax→bmm (qwen_visual.py:204-215), nn.MultiheadAttention core (qwen_visual.py:145),
 *           xformers memory_efficient_attention (modeling_llama_xformer.py:221-238),
 *           torch SDPA in diffusers AttnProcessor2_0 [ext].
 * Q[b][sq][h][D], K[b][skv][h][D], V[b][skv][h][D] addressed with element strides (multiples of 8 elements).
 * O[b][sq][h][D] (o_row_stride = elements between consecutive sq; heads packed at h*D).
 * causal: key j visible to query i iff j <= i + (Skv - Sq)  (bottom-right aligned; prefill and chunked decode).
 * D must be a multiple of 8 and <= 128 (104 is padded to 128 in LDS/registers only). */
typedef struct sx_attn_args {
  const void* Q;
  const void* K;
  const void* V;
  void* O;
  int32_t B, H, Sq, Skv, D, reserved;
  int64_t q_batch_stride, q_row_stride, q_head_stride;
  int64_t k_batch_stride, k_row_stride, k_head_stride;
  int64_t v_batch_stride, v_row_stride, v_head_stride;
  int64_t o_batch_stride, o_row_stride;
  float scale;
  int32_t causal;
  int32_t dtype;
} sx_attn_args;
int sx_attention(const sx_attn_args* args, void* stream);

/* Small generic attention (any D <= 256, VALU, one wave per query row). Used where FLOPs are negligible:
 * Resampler MHA with head_dim 160 (agent_seed_x_i.yaml:2-7), AttentionPool2d (resampler.py:89-116),
 * PerceiverAttention (resampler.py:46-75). V is in natural [b][skv][h][D] layout. */
typedef struct sx_attn_small_args {
  const void* Q;
  const void* K;
  const void* V;
  void* O;
  int32_t B, H, Sq, Skv, D;
  int64_t q_batch_stride, q_row_stride, q_head_stride;
  int64_t k_batch_stride, k_row_stride, k_head_stride;
  int64_t v_batch_stride, v_row_stride, v_head_stride;
  int64_t o_batch_stride, o_row_stride;
  float scale;
  int32_t dtype;
} sx_attn_small_args;
int sx_attention_small(const sx_attn_small_args* args, void* stream);

/* Single-token decode attention over the KV cache (split-KV flash-decoding, HBM-bound).
 * replaces memory_efficient_attention at q_len == 1 (modeling_llama_xformer.py:231-237).
 * q[H][D] 16-bit; kcache/vcache [H][Tmax][D]; ctx_len read from DEVICE memory (graph-replay friendly);
 * scratch: fp32 [H][nsplit][D+2]; out[H*D] 16-bit. */
int sx_attn_decode(const void* q, const void* kcache, const void* vcache, void* out, float* scratch,
                   const int32_t* ctx_len_dev, int H, int D, int Tmax, int nsplit, float scale, int dtype,
                   void* stream);

/* ------------------------------------------------------------------------------------------------
 * LLM glue kernels
 * ------------------------------------------------------------------------------------------------ */
/* RoPE (HF rotate-half, tables rounded to the activation dtype first — modeling_llama_xformer.py:128-149)
 * applied in place to the q part of qkv[T][3*H*D] and written, with v, into the caches at pos0+t.
 * pos0 read from device memory. */
int sx_rope_kv_append(void* qkv, void* kcache, void* vcache, const float* cos_tab, const float* sin_tab,
                      const int32_t* pos0_dev, int T, int H, int D, int Tmax, int dtype, void* stream);
/* out[t][:] = table[ids[t]][:]   (embed_tokens, seed_x.py:158) ; out fp32 */
int sx_embedding(const int32_t* ids, const void* table, float* out, int T, int dim, int dtype, void* stream);
/* dst[rows[i]][:] = src[i][:] fp32 (input_embeds[ids_cmp_mask] = ..., seed_x.py:173) */
int sx_scatter_rows(const float* src, const int32_t* rows, float* dst, int n, int dim, void* stream);
/* Greedy step with the AutoImageTokenGenerationProcessor rule fused (generation.py:19-31):
 * prev = *prev_id_dev; if prev in img_ids[0..n_img-2] → next = img_ids[idx+1] (the "max+10" rule) else
 * logits[img_ids[1..]] = 0.0 (in place, as the reference does) then argmax (first maximal index).
 * Writes next to *next_id_dev (may alias prev_id_dev) and, if out_ids != NULL, to out_ids[*step_dev]. */
int sx_greedy_next(float* logits, int vocab, const int32_t* img_ids_dev, int n_img, const int32_t* prev_id_dev,
                   int32_t* next_id_dev, int32_t* out_ids, const int32_t* step_dev, void* stream);

/* Lock-step batched decode (G independent sequences, one token each): same kernels with a sequence dimension.
 * Caches are [G][H][Tmax][D] (cache_seq_stride elements apart), positions / context lengths / step counters / token ids
 * are per-sequence device arrays, so weights are streamed from HBM once per step for all G sequences. */
int sx_rope_kv_append_b(void* qkv, void* kcache, void* vcache, const float* cos_tab, const float* sin_tab,
                        const int32_t* pos0_dev, int G, int T, int H, int D, int Tmax, int64_t cache_seq_stride, int dtype,
                        void* stream);
/* q_seq_stride: elements between the q rows of consecutive sequences (0 = H * D, contiguous) — 3 * H * D reads q straight out of
 * the fused [G][3 * H * D] qkv projection. dtype may carry SX_TILED16 (the output as operand tiles for the o-projection). */
int sx_attn_decode_b(const void* q, const void* kcache, const void* vcache, void* out, float* scratch,
                     const int32_t* ctx_len_dev, int G, int H, int D, int Tmax, int64_t cache_seq_stride, int nsplit,
                     float scale, int dtype, int64_t q_seq_stride, void* stream);
/* One launch per layer for the lock-step decode step: RoPE of the new token's q and k, K / V append at pos[g], split-KV attention
 * over the pos[g] + 1 visible keys and the combine of the splits. Replaces sx_rope_kv_append_b (T = 1) + sx_attn_decode_b with
 * bit-identical output and cache contents (modeling_llama_xformer.py:204-239 at q_len == 1). q is NOT rotated in place. */
typedef struct sx_attn_decode_args {
  const void* qkv;          /* [G][3*H*D] 16-bit rows q | k | v of the new token (output of the fused qkv projection)      */
  void* kcache;             /* [G][H][Tmax][D], sequences cache_seq_stride elements apart                                   */
  void* vcache;
  void* out;                /* [G][H*D] 16-bit, or operand tiles with dtype | SX_TILED16                                    */
  float* scratch;           /* [G][H][nsplit][D + 2] fp32                                                                   */
  void* counters;           /* uint32 [G*H]: zero when first used, left at zero                                             */
  const float* cos_tab;     /* [Tmax][D/2] fp32                                                                             */
  const float* sin_tab;
  const int32_t* pos_dev;   /* [G] position of the new token; positions outside [0, Tmax) attend to the cache, write nothing */
  int32_t G, H, D, Tmax, nsplit, dtype;
  int64_t cache_seq_stride;
  float scale;
  int32_t reserved;
} sx_attn_decode_args;
int sx_attn_decode_fused(const sx_attn_decode_args* args, void* stream);
int sx_greedy_next_b(float* logits, int ld_logits, int vocab, const int32_t* img_ids_dev, int n_img,
                     const int32_t* prev_id_dev, int32_t* next_id_dev, int32_t* out_ids, int ld_out,
                     const int32_t* step_dev, int G, void* stream);
/* dst[(g*seq_rows + step[g])][:] = src[g][:] fp32 (per-sequence hidden-state log, seed_x.py:196) */
int sx_scatter_rows_step(const float* src, const int32_t* step_dev, float* dst, int G, int dim, int seq_rows, void* stream);
/* p[0..n) += delta */
int sx_add_i32_n(int32_t* p, int delta, int n, void* stream);
/* In-flight batching: next token + stop rule + slot advance of the lock-step decode step in ONE launch. It replaces four nodes of
 * the captured token step (sx_greedy_next_b and three sx_add_i32_n) and moves the stop decision of the greedy loop that the
 * reference drives from seed_x.py:184-189 onto the device; the logits rule is the processor's (generation.py:19-31), the same
 * device function as sx_greedy_next_b. Per slot g (all arrays int32 [G] in device memory):
 *   live[g] == 0 (parked): nothing is read from the logits row and nothing at all is written.
 *   live[g] != 0: id = rule + first-maximal-index arg-max on logits[g]; if n_new[g] == force_at[g] the id is replaced by force_id
 *     AFTER the arg-max (synthetic weights only; force_at -1 = never). id goes to out_ids[g][step[g]] (if 0 <= step[g] < ld_out)
 *     and to cur[g]; n_new, step, pos and ctx advance by one. Stop rule: id == eos_id (eos_id -1 = none) or n_new >= max_new[g]
 *     → live = 0 and the slot is parked: step = -1, pos = -1, ctx = 0. Those are the idle values every kernel of the token step
 *     honours (no cache, log or id store; the attention kernels read no key row for the slot and return 0 for it).
 *   status[g] = { id, live, n_new, n_new at the finish or -1 }: what the host reads once per token step. */
typedef struct sx_slot_step_args {
  float* logits;                /* [G][ld_logits] fp32; the rule zeroes the image-token columns of LIVE rows in place              */
  const int32_t* img_ids_dev;   /* [n_img]: <img>, <img_0> ... <img_{n-1}>, </img>                                                 */
  int32_t* cur;                 /* in: the token just fed, out: the next token                                                     */
  int32_t* live;
  int32_t* n_new;               /* tokens generated so far                                                                         */
  const int32_t* max_new;       /* token budget per slot                                                                           */
  const int32_t* force_at;
  int32_t* pos;                 /* the three counters the other kernels of the step consume                                        */
  int32_t* ctx;
  int32_t* step;
  int32_t* out_ids;             /* [G][ld_out] or NULL                                                                             */
  int32_t* status;              /* [G][4]                                                                                          */
  int32_t ld_logits, vocab, n_img, ld_out, force_id, eos_id, G, reserved;
} sx_slot_step_args;
int sx_greedy_next_slots(const sx_slot_step_args* args, void* stream);
/* Seeded sampling of the next token on the device: what generate() does with do_sample=True (the reference passes do_sample=False at
 * seed_x.py:175-189, one word away), i.e. transformers' sample(): the processor rule first (generation.py:19-31, exactly as
 * sx_greedy_next applies it, the in-place zeroing of the image columns being the only edit of the row), then temperature → top-k →
 * top-p and one draw. Per row g, with x the fp32 logits row:
 *   do_sample[g] == 0, or the previous id inside the image chain: sx_greedy_next_b's id (arg-max / next chain id); nothing is drawn.
 *   else t = x / T; top-k (0 < top_k < vocab, else off) keeps t >= the k-th largest value, ties kept; w = exp(t − max t) over the
 *     survivors, W_k their sum; top-p keeps a token iff the mass of the strictly larger survivors is below top_p · W_k (the
 *     TopPLogitsWarper of transformers 4.30.2 without its sort: the maximum is always kept, equal values are kept or dropped together);
 *     u = (Philox4x32-10(counter (n, 0, 0, 0), key (seed lo, seed hi))[0] >> 8) · 2^-24; the id is the smallest kept index whose
 *     inclusive prefix mass exceeds u · W. n is token_index[g] (sx_sample_next_b) or step[g] (sx_sample_next_slots): the 0-based index
 *     of the generated token within its request.
 * A token whose fp32 weight underflows to 0 (x more than about 87 T below the maximum, or -inf) has mass 0: it is never drawn, not kept
 * and not counted in n_kept, also with top_p = 1. The masses are summed as 2^40-scaled integers, so the id depends on the row's values, the parameters, the seed and n only — not on
 * the slot, the neighbours, the launch or graph replay. One workgroup per row, the row is read once; vocab <= 32768. Every pointer is
 * device memory with one entry per row, read at launch (a captured graph serves any mix of greedy and sampled rows). */
typedef struct sx_sample_args {
  const int32_t* do_sample;     /* 0: greedy row                                                                                   */
  const float* temperature;     /* T > 0                                                                                           */
  const int32_t* top_k;         /* 0 = off                                                                                         */
  const float* top_p;           /* 0 < top_p <= 1                                                                                  */
  const uint32_t* seed;         /* [G][2]: low word, high word of the 64-bit seed                                                  */
  const int32_t* token_index;   /* sx_sample_next_b only (sx_sample_next_slots uses step); may be NULL there                       */
  int32_t* n_kept;              /* optional out: size of the kept set; -1 for greedy rows and rows inside the image chain          */
  float* p_chosen;              /* optional out: probability of the drawn id within the kept set; 1.0 for those rows               */
} sx_sample_args;
/* sx_greedy_next_b's arguments and outputs, with the id by the rule above. */
int sx_sample_next_b(float* logits, int ld_logits, int vocab, const int32_t* img_ids_dev, int n_img,
                     const int32_t* prev_id_dev, int32_t* next_id_dev, int32_t* out_ids, int ld_out,
                     const int32_t* step_dev, int G, const sx_sample_args* sample, void* stream);
/* sx_greedy_next_slots (parking, force_at after the draw, stop rule, counters, status — all unchanged) with the id by the rule above. */
int sx_sample_next_slots(const sx_slot_step_args* args, const sx_sample_args* sample, void* stream);
/* Token log-probabilities (seedx_amd.sampling.token_logprobs states the rule in fp64). For an fp32 logits row x[0..vocab) as lm_head
 * produced it — before the processor rule's in-place zeroing, temperature, top-k and top-p —
 *   lp(v) = (x[v] − m) − log Σ exp(x − m),  m = max x,
 * and the n_top (0 .. 8) largest columns by successive first-maximal-index selection (ties: lowest index first; past the end of the
 * row: id −1, value −inf). One workgroup per row, fp32 ACCUMULATION in a layout fixed by vocab alone: thread t of 1024 adds the columns
 * t, t + 1024, ... in ascending order, the lanes of a wave combine in a xor butterfly, the 16 wave sums in a pairwise tree (42 additions
 * deep at vocab <= 32768); the maximum is exact. The bits of a record are a function of (row values, vocab) only — not of the slot,
 * the neighbours, G, the launch or graph replay — and the same in all three entry points below, which share one non-inlined device
 * function. x[v] = −inf gives −inf; a row holding NaN (or +inf, or nothing but −inf) gives NaN values and ids −1.
 * sx_token_logprobs: teacher-forced rows (scoring). logits [rows][ld], vocab >= 1 of any size (columns >= vocab are never read),
 * targets int32 [rows] (outside [0, vocab): NaN); chosen fp32 [rows]; top_ids int32 / top fp32 [rows][n_top], both NULL iff n_top = 0. */
int sx_token_logprobs(const float* logits, int64_t ld, int vocab, const int32_t* targets, float* chosen, int32_t* top_ids, float* top,
                      int n_top, int rows, void* stream);
/* The LP form of the decode tail: sx_sample_next_b / sx_sample_next_slots (sample == NULL: sx_greedy_next_b / sx_greedy_next_slots) that
 * also record, per row g with want[g] != 0, the log-probability of the id the row EMITS (after force_at replacement) and the top
 * list, at chosen[g][step[g]] and top_ids / top[g][step[g]][0..n_top) under out_ids' guard 0 <= step[g] < ld_out (out_ids itself may be
 * NULL; ld_out >= 1 and step are required). The statistics are taken from the raw row before the rule edits it. A row whose previous id
 * lies inside the image chain records NaN and ids −1: the rule forces its id, the model did not choose. Parked slots and rows with
 * want[g] == 0 record nothing. Everything else — ids, the zeroed columns, counters, stop rule, status, n_kept / p_chosen — is bit for
 * bit the call without the record. vocab <= 32768. */
typedef struct sx_logprob_args {
  const int32_t* want;          /* [G]: 0 = the row records nothing                                                                */
  float* chosen;                /* [G][ld_out]                                                                                     */
  int32_t* top_ids;             /* [G][ld_out][n_top]; NULL iff n_top == 0                                                         */
  float* top;                   /* [G][ld_out][n_top]; NULL iff n_top == 0                                                         */
  int32_t n_top, reserved;
} sx_logprob_args;
int sx_sample_next_b_lp(float* logits, int ld_logits, int vocab, const int32_t* img_ids_dev, int n_img,
                        const int32_t* prev_id_dev, int32_t* next_id_dev, int32_t* out_ids, int ld_out,
                        const int32_t* step_dev, int G, const sx_sample_args* sample, const sx_logprob_args* lp, void* stream);
int sx_sample_next_slots_lp(const sx_slot_step_args* args, const sx_sample_args* sample, const sx_logprob_args* lp, void* stream);
/* Per-request logits controls on the device (seedx_amd.sampling.apply_controls states the rule in numpy fp32, one IEEE rounding per
 * written operation; the kernel runs each as one instruction). Row g with on[g] != 0: with c = counts[g][v] (bit 30: v occurs in the
 * prompt; c & 0xFFFFFF = n, times generated) and k the token index (step[g] in the slot form, token_index[g] in lock-step),
 *   1. rep != 1 and (mark or n > 0):  y = y < 0 ? y * rep : y * rep_inv            (rep_inv = float32(1 / rep), made by the host)
 *   2. n > 0:                         t = frequency * float(n); t = t + presence; y = y - t
 *   3. every bias entry j with 0 <= bias_ids[g][j] < vocab, in list order:  y[id] = y[id] + bias[g][j]     (-inf bans the id)
 *   4. eos_id >= 0 and k < min_new[g]:  y[eos_id] = -inf                 (the slot form takes sx_slot_step_args.eos_id, lock-step eos_id below)
 * then the processor rule, and the arg-max or draw, of the uncontrolled call run on y. The edited row is written to work[g][0..ld_logits)
 * and the rule's zeroing happens THERE: the logits row of a controlled row stays exactly what lm_head wrote, so the LP record is of
 * the raw row. After the emitted id is known (slot form: after the force_at replacement) counts[g][id] += 1 for 0 <= id < vocab.
 * A row with on[g] == 0 and every parked slot: bit for bit the call without controls (in-place zeroing included), nothing counted. */
typedef struct sx_logits_ctl_args {
  const int32_t* on;            /* [G]: 0 = the row runs as without controls                                                       */
  int32_t* counts;              /* [G][ld_counts]: bit 30 = prompt mark, low 24 bits = times generated                             */
  float* work;                  /* [G][ld_logits]: the edited rows (rows with on = 0 are not written)                              */
  const float* rep;             /* [G] repetition penalty, finite > 0 (1 = off)                                                    */
  const float* rep_inv;         /* [G] float32(1 / rep)                                                                            */
  const float* presence;        /* [G]                                                                                             */
  const float* frequency;       /* [G]                                                                                             */
  const int32_t* min_new;       /* [G]                                                                                             */
  const int32_t* bias_ids;      /* [G][16], -1 = empty                                                                             */
  const float* bias;            /* [G][16]                                                                                         */
  const int32_t* token_index;   /* [G], lock-step form only (the slot form uses step); may be NULL there                           */
  int32_t ld_counts, eos_id;    /* eos_id: lock-step form only, -1 = none                                                          */
} sx_logits_ctl_args;
/* sx_sample_next_b_lp's / sx_sample_next_slots_lp's arguments with sample and lp both nullable (greedy, sampled, LP, sampled + LP) and
 * the controls above; ctl is required. vocab of any size for the greedy form without lp; ld_logits >= vocab, ld_counts >= vocab. */
int sx_next_b_ctl(float* logits, int ld_logits, int vocab, const int32_t* img_ids_dev, int n_img,
                  const int32_t* prev_id_dev, int32_t* next_id_dev, int32_t* out_ids, int ld_out,
                  const int32_t* step_dev, int G, const sx_sample_args* sample, const sx_logprob_args* lp,
                  const sx_logits_ctl_args* ctl, void* stream);
int sx_next_slots_ctl(const sx_slot_step_args* args, const sx_sample_args* sample, const sx_logprob_args* lp,
                      const sx_logits_ctl_args* ctl, void* stream);
/* Constrained decoding: a token-level deterministic automaton per grammar, resident on the device as a dense table
 * (seedx_amd.grammar builds it on the host and states the rule in numpy fp32: constrain_row, advance). Row g is CONSTRAINED when
 * 0 <= table[g] < n_tables and 0 <= state[g] < n_states; with T = trans[table[g]][state[g]] and F = flags[table[g]]:
 *   working row: the row gets one in ctl->work whether or not ctl->on[g] is set - with on[g] != 0 steps 1-4 of the controls rule ran
 *                first, as in sx_next_b_ctl; with on[g] == 0 it is a plain copy of the row and nothing is counted;
 *   mask:        y[v] = -inf where T[v] < 0 (v != eos); y[eos] keeps its value iff F[state[g]] & 1, else -inf; nothing else changes
 *                (eos: sx_slot_step_args.eos_id in the slot form, eos_id below in lock-step; -1 = none);
 *   id:          the processor rule (chain forcing, zeroing of the image columns) is SKIPPED for the row - its zeroing would lift banned
 *                image columns from -inf to 0.0, and the host never constrains a row inside the image chain; the arg-max or the seeded
 *                draw then runs on the working row, unchanged. The logits row stays raw: the LP record describes the raw distribution;
 *   advance:     on the id the row emits (slot form: behind the force_at replacement) state[g] = DONE (-2) on EOS, else s' = T[id];
 *                DONE if s' < 0 (reachable only when every admissible logit was -inf already) or s' is final (F[s'] & 2), else s'.
 * In the slot form the stop rule gains "or the new state is DONE": the slot parks itself exactly as on EOS or budget (same idle values,
 * same status row). In the lock-step form the row runs unconstrained from then on; the host cuts the request there.
 * Every other row (table[g] < 0, state[g] < 0, or either out of range): bit for bit sx_next_b_ctl / sx_next_slots_ctl, the in-place
 * zeroing of an uncontrolled row included. A parked slot reads and writes nothing, state included.
 * trans is read two ids per dword: ld_v is even and >= vocab, trans 4-byte aligned; 1 <= n_states <= 32767. */
typedef struct sx_token_fsm_args {
  const int32_t* table;   /* [G]: grammar index of the row, -1 = unconstrained                 */
  int32_t* state;         /* [G]: in/out; < 0 (DONE) = the row runs unconstrained             */
  const int16_t* trans;   /* [n_tables][n_states][ld_v], -1 = banned                          */
  const int32_t* flags;   /* [n_tables][n_states]: bit 0 accepting, bit 1 final               */
  int32_t n_tables, n_states, ld_v, eos_id;   /* eos_id: lock-step form only, -1 = none       */
} sx_token_fsm_args;
int sx_next_b_fsm(float* logits, int ld_logits, int vocab, const int32_t* img_ids_dev, int n_img,
                  const int32_t* prev_id_dev, int32_t* next_id_dev, int32_t* out_ids, int ld_out,
                  const int32_t* step_dev, int G, const sx_sample_args* sample, const sx_logprob_args* lp,
                  const sx_logits_ctl_args* ctl, const sx_token_fsm_args* fsm, void* stream);
int sx_next_slots_fsm(const sx_slot_step_args* args, const sx_sample_args* sample, const sx_logprob_args* lp,
                      const sx_logits_ctl_args* ctl, const sx_token_fsm_args* fsm, void* stream);
/* Sequence rules: stop sequences and no_repeat_ngram_size (seedx_amd.sampling states them in numpy: ngram_banned, apply_no_repeat,
 * stop_match). They need the ORDER of the ids a request has seen: hist[g][0 .. hist_len[g]) holds its prompt ids (image placeholders
 * included) followed by every id it emitted, prompt_len[g] of them the prompt. For a row with on[g] != 0, in this order:
 *   ban:     with n = ngram[g] > 0 and L = hist_len[g] the row gets a working row in ctl->work (the controlled row when ctl->on[g] is
 *            set, a plain copy otherwise) in which, for every i in [0, L - n] with hist[i .. i+n-1) == hist[L-n+1 .. L), column
 *            hist[i+n-1] is -inf (ids outside [0, vocab) ban nothing but take part in the comparison); nothing else changes. The
 *            grammar mask (fsm may be NULL), the processor rule and the arg-max or draw then run as in sx_next_b_fsm / sx_next_b_ctl;
 *            the logits row stays raw, so the LP record describes the raw distribution. Inside the image chain the forced id wins;
 *   append:  the id the row emits (slot form: behind the force_at replacement) goes to hist[g][hist_len[g]] and hist_len[g] += 1;
 *            a history that is full (hist_len[g] == ld_hist) takes nothing more and matches nothing;
 *   stop:    matched[g] = the lowest j < n_stop[g] for which the GENERATED ids (hist[prompt_len[g] .. hist_len[g])) end with
 *            stop_ids[g][j][0 .. stop_len[g][j]), else -1. A stop that would straddle the end of the prompt does not match.
 * In the slot form a match joins the stop rule: the slot parks itself exactly as on EOS or budget (same idle values, same status row);
 * the matched ids stay in the id log. In the lock-step form matched is all that is written; the host cuts the request there.
 * A row with on[g] == 0 and every parked slot: bit for bit sx_next_b_ctl / sx_next_slots_ctl (with fsm: the _fsm entry points), and its
 * history, hist_len and matched are not touched. Per-row values out of range are clamped on the device (ngram to 0 .. 8, n_stop to
 * 0 .. 4, stop_len to 1 .. 8, hist_len to 0 .. ld_hist): a wrong table gives wrong ids, never a wild address. ld_hist >= 1. */
typedef struct sx_seq_rule_args {
  const int32_t* on;            /* [G]: 0 = the row runs as without sequence rules                   */
  const int32_t* ngram;         /* [G]: no_repeat_ngram_size, 0 = off, at most 8                     */
  int32_t* hist;                /* [G][ld_hist]: prompt ids, then the emitted ids                    */
  int32_t* hist_len;            /* [G]: in/out                                                       */
  const int32_t* prompt_len;    /* [G]                                                               */
  const int32_t* n_stop;        /* [G]: 0 .. 4                                                       */
  const int32_t* stop_len;      /* [G][4]: 1 .. 8 for j < n_stop[g]                                  */
  const int32_t* stop_ids;      /* [G][4][8]                                                         */
  int32_t* matched;             /* [G]: out, index of the matched stop sequence or -1                */
  int32_t ld_hist, reserved;
} sx_seq_rule_args;
/* sx_next_b_fsm's / sx_next_slots_fsm's arguments with fsm nullable, and the rules above; ctl and seq are required. */
int sx_next_b_seq(float* logits, int ld_logits, int vocab, const int32_t* img_ids_dev, int n_img,
                  const int32_t* prev_id_dev, int32_t* next_id_dev, int32_t* out_ids, int ld_out,
                  const int32_t* step_dev, int G, const sx_sample_args* sample, const sx_logprob_args* lp,
                  const sx_logits_ctl_args* ctl, const sx_token_fsm_args* fsm, const sx_seq_rule_args* seq, void* stream);
int sx_next_slots_seq(const sx_slot_step_args* args, const sx_sample_args* sample, const sx_logprob_args* lp,
                      const sx_logits_ctl_args* ctl, const sx_token_fsm_args* fsm, const sx_seq_rule_args* seq, void* stream);

/* Speculative decoding (lossless): the token step carries T = K + 1 rows per slot — row g*T is the slot's current token, rows g*T + 1 ..
 * g*T + n_draft[g] K drafted continuations — and sx_greedy_next_b / sx_sample_next_b over the G*T rows (previous id = the row's input,
 * token index = step[g] + t) give every row its candidate id. sx_spec_accept keeps, per LIVE slot, the longest run the model itself
 * would have produced one token at a time (seedx_amd.spec.accept states the rule): for t = 0, 1, ...
 *   id = cand[g*T + t], replaced by force_id if n_new[g] + t == force_at[g] (after the rule, as in sx_greedy_next_slots);
 *   id goes to out_ids[g][step[g] + t] (inside the row capacity ld_out) and to hist[g][pos[g] + 1 + t] (inside Tmax): the cache position
 *     at which it will be fed;
 *   the walk continues to t + 1 only if t < n_draft[g], id == rows_in[g*T + t + 1] (the draft row t + 1 was fed), id != eos_id,
 *     id != img_ids_dev[0] (<img>: the host-driven image chunk takes over; NULL = no such id) and n_new[g] + t + 1 < max_new[g].
 * pos, ctx, step and n_new advance by the emitted count (>= 1), cur[g] = rows_in[g*T] = the last emitted id (row 0 of the next step:
 * a caller that drafts by itself only fills rows 1 .. and n_draft); the stop rule (EOS or budget), the parking
 * values and status[g] = { last id, live, n_new, n_new at the finish or -1 } are sx_greedy_next_slots'. With n_draft = 0 the launch IS
 * that entry's slot advance. A parked slot reads and writes nothing. A rejected draft leaves cache rows at or above the new pos, which
 * no kernel reads before the next steps overwrite them. T <= 8, G*T <= 32; all arrays int32 in device memory. */
typedef struct sx_spec_accept_args {
  const int32_t* cand;          /* [G*T] candidate ids                                                                             */
  int32_t* rows_in;             /* [G*T] the ids the rows were fed; row g*T is rewritten with the last emitted id                  */
  const int32_t* n_draft;       /* [G] drafted rows per slot, 0 .. T - 1                                                           */
  int32_t* cur;
  int32_t* live;
  int32_t* n_new;
  const int32_t* max_new;
  const int32_t* force_at;
  int32_t* pos;
  int32_t* ctx;
  int32_t* step;
  int32_t* out_ids;             /* [G][ld_out] or NULL                                                                             */
  int32_t* status;              /* [G][4]                                                                                          */
  int32_t* hist;                /* [G][Tmax] ids by cache position, or NULL                                                        */
  const int32_t* img_ids_dev;   /* sx_slot_step_args' list (only <img>, its first entry, is read), or NULL                         */
  int32_t G, T, ld_out, Tmax, force_id, eos_id;
} sx_spec_accept_args;
int sx_spec_accept(const sx_spec_accept_args* args, void* stream);
/* The drafter that needs no second model: prompt-lookup n-grams (seedx_amd.spec.propose_ngram states the rule). Per slot g with
 * L = pos[g] + 1 known ids hist[g][0 .. L) (cur[g] is the last): for n = ngram_max down to ngram_min take the LARGEST start i with
 * hist[i .. i+n) == hist[L-n .. L) and i + n <= L - 1; the first n that matches proposes hist[i+n .. min(i+n+K, L)), K = T - 1.
 * Writes the next step's row inputs rows_out[g*T ..]: row 0 = cur[g], rows 1 .. n_draft[g] the draft, the rest cur[g]; no match, a
 * parked slot (pos < 0) or L > Tmax give n_draft[g] = 0. One workgroup per slot. */
typedef struct sx_spec_draft_args {
  const int32_t* hist;          /* [G][Tmax]                                                                                       */
  const int32_t* pos;           /* [G]                                                                                             */
  const int32_t* cur;           /* [G]                                                                                             */
  int32_t* rows_out;            /* [G*T]                                                                                           */
  int32_t* n_draft;             /* [G]                                                                                             */
  int32_t G, T, Tmax, ngram_max, ngram_min, reserved;
} sx_spec_draft_args;
int sx_spec_draft_ngram(const sx_spec_draft_args* args, void* stream);
/* the hidden-state log of a verify step: dst[(g*seq_rows + step[g] + t)][:] = src[g*T + t][:] fp32 (rows of parked slots, step < 0, and
 * rows past seq_rows are dropped); tok_index (optional, int32 [G*T]) receives max(step[g], 0) + t, the candidates' token indices */
int sx_scatter_rows_spec(const float* src, const int32_t* step_dev, float* dst, int32_t* tok_index, int G, int T, int dim,
                         int seq_rows, void* stream);

/* KV-cache prefix fork (prefix reuse of in-flight batching, inflight.py): copies the first rows of one slot's cache to other slots,
 * every layer and head in ONE launch. The cache is addressed as bytes, so one entry serves every cache tensor and format: the fp32 K
 * cache (row_bytes 512 at head_dim 128), the 16-bit caches (256), the FP8 codes (128) and their fp32 row scales (row_bytes 4).
 * For every pair i and every (o < outer, h < inner) the n_rows[i] * row_bytes contiguous bytes at
 *     cache + o * outer_stride + src[i] * slot_stride + h * inner_stride
 * are copied to the same offset of slot dst[i]. A pair is SKIPPED (nothing is written) when src[i] or dst[i] lies outside [0, G),
 * when src[i] == dst[i] or when n_rows[i] <= 0; n_rows[i] above Tmax is CLAMPED to Tmax. The pairs of one launch are not ordered:
 * no slot may be written twice, and no slot may be read and written (ops.kv_fork refuses both). 16-byte accesses wherever the two
 * spans share their alignment modulo 16, 4-byte accesses for the head and tail of such spans and for spans that do not (scale rows;
 * an odd Tmax): cache, the strides and row_bytes must be multiples of 4. outer * inner and n_pairs are at most 65535 each. */
typedef struct sx_kv_fork_args {
  void* cache;             /* bytes, viewed as [outer][G][inner][Tmax][row_bytes]                       */
  const int32_t* src;      /* device [n_pairs] donor slot                                               */
  const int32_t* dst;      /* device [n_pairs] receiving slot                                           */
  const int32_t* n_rows;   /* device [n_pairs] rows [0, n) to copy                                      */
  int64_t outer_stride, slot_stride, inner_stride;   /* bytes                                           */
  int32_t n_pairs, outer, G, inner, Tmax, row_bytes;
} sx_kv_fork_args;
int sx_kv_fork(const sx_kv_fork_args* args, void* stream);

/* KV-cache rows <-> a linear staging buffer (the host-memory tier of the prefix cache, kvstore.py): sx_kv_fork generalised. ONE launch
 * moves the first rows of any number of slots, every layer and head of ALL cache tensors of the model (kc, vc and, under the FP8
 * format, ks, vs), between the caches and a device staging buffer: direction 0 packs (cache -> staging), 1 unpacks (staging -> cache).
 * Every tensor is addressed as bytes, [outer][G][inner][Tmax][row_bytes] as in sx_kv_fork_args; outer, G, inner and Tmax are shared,
 * the base pointer, the three strides and row_bytes are per tensor (passed by value: the kernel reads them from its arguments).
 * Staging layout of job j, from byte offset[j] (a multiple of 16): spans in the order [tensor][outer][inner], the span of tensor t
 * holding n * row_bytes[t] bytes (the rows [0, n) of one head) and taking that size rounded UP to a multiple of 16; the padding bytes
 * are never read or written. sx_kv_rows_job_bytes states the size of a job; host and kernel compute it by this one rule.
 * A job is SKIPPED (nothing is read or written) when slot[j] lies outside [0, G) or n_rows[j] <= 0 — and, as a guard, when its offset
 * is not a multiple of 16 or its bytes would end beyond staging_bytes; n_rows[j] above Tmax is CLAMPED to Tmax. The jobs of a launch
 * are not ordered: no two unpack jobs may name one slot, no two jobs may overlap in staging (ops.kv_rows_copy refuses both).
 * 16-byte accesses wherever the cache span is 16-byte aligned (the staging side always is), 4-byte accesses for the tail of such spans
 * and for whole spans that are not (scale rows under an odd Tmax); vector stores only, no LDS, no atomics.
 * host_slot / host_n_rows / host_offset are the host's copies of the three device arrays: the entry point checks the jobs as the host
 * states them. SX_ERR_INVALID, never a fall-back: a null pointer, n_tensors outside 1..4, an offset that is no multiple of 16, a job
 * that ends beyond staging_bytes, staging not 16-byte aligned, a base / stride / row_bytes that is no multiple of 4, strides that do
 * not describe the view, n_tensors * outer * inner or n_jobs above 65535, direction other than 0 / 1. */
typedef struct sx_kv_tensor {
  void* base;                                        /* bytes, viewed as [outer][G][inner][Tmax][row_bytes]  */
  int64_t outer_stride, slot_stride, inner_stride;   /* bytes                                                */
  int32_t row_bytes, reserved;
} sx_kv_tensor;
typedef struct sx_kv_rows_args {
  sx_kv_tensor tensor[4];
  const int32_t* slot;          /* device [n_jobs]                                                           */
  const int32_t* n_rows;        /* device [n_jobs] rows [0, n) of the slot                                   */
  const int64_t* offset;        /* device [n_jobs] byte offset of the job in staging                         */
  const int32_t* host_slot;     /* host copies of the three arrays                                           */
  const int32_t* host_n_rows;
  const int64_t* host_offset;
  void* staging;                /* device, 16-byte aligned                                                   */
  int64_t staging_bytes;
  int32_t n_tensors, n_jobs, outer, G, inner, Tmax, direction, reserved;
} sx_kv_rows_args;
int sx_kv_rows_copy(const sx_kv_rows_args* args, void* stream);
/* bytes of one job of n_rows rows (clamped to Tmax; 0 for n_rows <= 0): outer * inner * sum over tensors of
 * round_up(n * row_bytes[t], 16); -1 for n_tensors outside 1..4 */
int64_t sx_kv_rows_job_bytes(const int32_t* row_bytes, int n_tensors, int outer, int inner, int Tmax, int n_rows);

/* Decode tiles → the row-major matrix (LlamaForCausalLM(weight_residency="tiles"): the quantised tiles are the only copy of a
 * projection, prefill rebuilds it into a shared scratch buffer in front of its sx_gemm). The exact inverse of the packers of ops.py:
 * out[n][k] (16-bit, `dtype`, row-major [N][K]) = the value the skinny GEMM feeds its MFMAs for weight (n, k) —
 *   SX_FP8_E4M3: decode(code) * w_scale[n] (the power-of-two row scale: the product is exact in fp32 and, for the quantiser's exponents
 *     [-15, 7], exactly representable in fp16 and bf16), tiles [N/16][K/64][16][64] (w_layout 1) or [N/20][K/64][20][64] (w_layout 2),
 *   SX_FP4_E2M1: decode(code) * 2^(E8M0 byte - 127) by the packed converts of sx_gemv (scale bits = byte << 23), tiles
 *     [N/16][K/64][16][32] + scale tiles [N/16][K/64][16][2] (w_layout 1) or the 20-row forms (w_layout 2),
 * byte order inside a 64-k slab as under sx_gemv_args.w_dtype / w_block_scale. Rows are in the order of the tiles (GLU-packed rows stay
 * packed). Every store instruction of a wave covers whole 128-byte row segments. SX_ERR_INVALID, never a fall-back: another w_dtype,
 * w_layout 0, K % 64 != 0, N no multiple of the layout's 16 / 20 rows, a missing or not 16-B aligned scale array, the other format's scale
 * array set, tiles / out not 16-B aligned, out_bytes < N * K * 2. Nothing beyond the first N * K * 2 bytes of out is written. */
typedef struct sx_dequant_tiles_args {
  const void* tiles;          /* the code tiles                                                               */
  const float* w_scale;       /* SX_FP8_E4M3: fp32 [N] row scales (else NULL)                                 */
  const void* w_block_scale;  /* SX_FP4_E2M1: E8M0 scale tiles (else NULL)                                    */
  void* out;                  /* 16-bit [N][K], row-major                                                     */
  uint64_t out_bytes;         /* bytes the caller owns at out (>= N * K * 2)                                  */
  int32_t w_dtype, w_layout, N, K, dtype, reserved;
} sx_dequant_tiles_args;
int sx_dequant_tiles(const sx_dequant_tiles_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Elementwise / layout helpers
 * ------------------------------------------------------------------------------------------------ */
int sx_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, void* stream);
/* fp32 x[rows][cols] → bf16 out[rows][3*cols] holding the planes of x = hi + lo (hi = bf16(x), lo = bf16(x - hi)):
 * role 0 (A operand rows) = [hi | hi | lo], role 1 (W operand rows) = [hi | lo | hi], so that one sx_gemm with K = 3*cols
 * computes Ah·Wh + Ah·Wl + Al·Wh with fp32 accumulation. cols % 4 == 0. Operand preparation of the VAE's fp32-grade mode:
 * stands in for the fp32 VAE the reference's pipeline switches to in upcast_vae()
 * (pipeline_stable_diffusion_xl_t2i_edit.py:509-511, :569-586, :965-977). */
int sx_split_bf16(const float* x, void* out, int64_t rows, int cols, int role, void* stream);

/* ------------------------------------------------------------------------------------------------
 * fp32-grade activations of the Llama decoder (LlamaForCausalLM(precise=True); csrc/precise.hip): a 16-bit checkpoint's weights
 * are exact, so logits within 1e-3 of the fp32 reference at 40 layers only need more mantissa on the ACTIVATION side:
 * GEMM A operands travel as two 16-bit planes x = hi + lo (hi = rn16(x), lo = rn16(x - hi)), q / k / v and the KV cache stay fp32.
 * `dtype` below = SX_F16 / SX_BF16 of the planes; | SX_TILED16 → operand tiles [2 planes][ceil(rows / 16)][cols/32][16][32] (the hi
 * plane's row blocks, then the lo plane's; rows <= 32: the x operand of sx_gemv with x_planes = 2) instead of rows [rows][2*cols] =
 * [hi | lo] (sx_gemm with a_planes = 2).
 * ------------------------------------------------------------------------------------------------ */
/* fp32 x[rows][cols] (row stride ldx) → the two planes. cols % 8 == 0 (tiles: cols % 32 == 0). */
int sx_split16(const float* x, int64_t ldx, void* out, int rows, int cols, int dtype, void* stream);
/* LlamaRMSNorm (modeling_llama_xformer.py:95,286,301,595): y = gamma * (x * rsqrt(mean(x^2) + eps)), all fp32; y32 (fp32 [rows][cols],
 * may be NULL) and / or the planes of y (out16, may be NULL). */
int sx_rmsnorm_planes(const float* x, const float* gamma, float* y32, void* out16, int rows, int cols, float eps, int dtype,
                      void* stream);
/* Per-request LoRA adapters, UNMERGED beside one resident base model (csrc/lora.hip; the rule in fp64: seedx_amd/lora.py). The reference
 * trains LoRA r 32 / alpha 32 on q/k/v/o/gate/up/down with the three norms in modules_to_save (configs/clm_models/llm_seed_x_lora.yaml) and
 * serves it through peft's Linear.forward (proj/peft/src/peft/tuners/lora.py:808-825): y = W x + s B (A x), s = alpha / r. Here the
 * intermediate t = A x stays fp32. Every call reads the adapter index of a row from DEVICE memory (sel; graph-capturable); an index outside
 * [0, n_adapters) makes the row a base row: nothing is read from the tables and nothing is written for it. Fixed reduction order; a row's
 * result depends on the row, its adapter's tables and its sel only — not on the row count, the row's position or its neighbours.
 *
 * sx_lora_shrink: t[m][i] = sum_k A[sel[m]][i][k] * (hi[m][k] + lo[m][k]), i < SR = S * R — S projections that share the x operand (3 for
 *   q|k|v, 2 for gate|up, 1 for o / down) times the rank table R. x: the planes of sx_split16 / sx_rmsnorm_planes* — dtype | SX_TILED16:
 *   operand tiles [2][ceil(M / 16)][K/32][16][32] (M <= 32, K % 32 == 0: what sx_gemv reads with x_planes = 2); else rows [M][2K] =
 *   [hi | lo] (any M <= 65535: prefill). A: 16-bit [n_adapters][SR][K] (an adapter of rank r < R is zero-padded: exact). t: fp32 [M][SR].
 *   K % 8 == 0, SR % 4 == 0, 16-B aligned pointers. */
int sx_lora_shrink(const void* x, const void* A, const int32_t* sel, float* t, int M, int K, int SR, int n_adapters, int dtype,
                   void* stream);
/* sx_lora_expand: delta[m][n] = scale[sel[m]] * sum_j B[sel[m]][n][j] * t[m][seg[n / 16] * R + j], j < R. B: 16-bit [n_adapters][N][R],
 *   rows in the order of W AS PACKED (GLU-packed rows stay packed); seg: device int32 [N/16], the S-segment of t each 16-row group of W
 *   reads (clamped into [0, S)); scale: fp32 [n_adapters] = lora_alpha / r. delta: fp32 [M][N] — sx_gemv_args.addend (with addend_sel =
 *   sel, addend_n = n_adapters) or sx_gemm's bias2d with bias2d_rows = 1. Base rows of delta are NOT written.
 *   N % 16 == 0, R % 8 == 0, S * R <= 512. */
int sx_lora_expand(const float* t, const void* B, const int32_t* seg, const float* scale, const int32_t* sel, float* delta, int M, int N,
                   int R, int S, int n_adapters, int dtype, void* stream);
/* sx_rmsnorm_planes with one gamma per adapter (peft modules_to_save copies of input_layernorm / post_attention_layernorm / model.norm):
 *   row m uses gamma_table[sel[m]] (fp32 [n_adapters][cols]) when sel[m] is in [0, n_adapters), else the base gamma. Every row has the bits
 *   of sx_rmsnorm_planes called with the gamma it selected (one shared body). n_adapters = 0 (gamma_table may be NULL): all base rows. */
int sx_rmsnorm_planes_sel(const float* x, const float* gamma, const float* gamma_table, const int32_t* sel, int n_adapters, float* y32,
                          void* out16, int rows, int cols, float eps, int dtype, void* stream);
/* sx_rope_kv_append_b on fp32 rows and fp32 caches (modeling_llama_xformer.py:141-149,215-220): qkv fp32 [G*T][3*H*D], q rotated in
 * place, rotated k and v appended to kcache / vcache fp32 [G][H][Tmax][D] at pos0[g] + t. The cos / sin tables are rounded to
 * table_dtype first (:128-131 casts them to the activation dtype); positions outside [0, Tmax) write nothing. */
int sx_rope_kv_append_f32(float* qkv, float* kcache, float* vcache, const float* cos_tab, const float* sin_tab,
                          const int32_t* pos0_dev, int G, int T, int H, int D, int Tmax, int64_t cache_seq_stride,
                          int table_dtype, void* stream);
/* the same with the "mixed" cache: k fp32, v appended in table_dtype (16-bit [G][H][Tmax][D], the same element strides): three
 * quarters of the cache bytes; v's rounding only perturbs the softmax-weighted average */
int sx_rope_kv_append_f32_v16(float* qkv, float* kcache, void* vcache16, const float* cos_tab, const float* sin_tab,
                              const int32_t* pos0_dev, int G, int T, int H, int D, int Tmax, int64_t cache_seq_stride,
                              int table_dtype, void* stream);
/* the same two with the paged cache (sx_attn_f32_args.page_table states the layout): kpool / vpool are [n_pages + 1][H][page size][D]
 * (v16 = 1: vpool is 16-bit in table_dtype), pages page_stride elements apart; the row of position pos0[g] + t goes to page
 * page_table[g][pos >> page_shift] (int32 [G][ceil(Tmax / page size)], clamped to [0, n_pages]) at row pos & (page size - 1). A row whose
 * entry is 0 (the null page) and a position outside [0, Tmax) write nothing; q is rotated either way. head_dim 128, page_shift 5..7. */
int sx_rope_kv_append_f32_paged(float* qkv, float* kpool, void* vpool, int v16, const float* cos_tab, const float* sin_tab,
                                const int32_t* pos0_dev, const int32_t* page_table, int G, int T, int H, int D, int Tmax,
                                int page_shift, int n_pages, int64_t page_stride, int table_dtype, void* stream);
/* the same with the FP8 KV cache (LlamaForCausalLM(kv_format="fp8_e4m3"), head_dim 128 only): the rotated k row and the v row of every
 * (token, head) are quantised to OCP e4m3fn codes with ONE power-of-two scale per row — s = clamp(ceil(log2(amax / 448)), -64, 64), 0 for a
 * zero row, code = e4m3fn(rne(clamp(x * 2^-s, +-448))), never a NaN code (seedx_amd.quant.quantize_kv_rows states the rule on the host, bit
 * for bit) — and appended to kcodes / vcodes uint8 [G][H][Tmax][128] (sequences cache_seq_stride BYTES apart) and kscale / vscale fp32
 * [G][H][Tmax] (sequences scale_seq_stride floats apart): 264 B per (head, token) instead of 768. q is rotated in place.
 * emulate = 1, the bit-reference twin: kcodes / vcodes are the FP32 caches of sx_rope_kv_append_f32 (cache_seq_stride in floats) and
 * receive decode(code) * 2^s; the scale pointers are unused (NULL). Positions outside [0, Tmax) write nothing. */
int sx_rope_kv_append_f32_q8(float* qkv, void* kcodes, void* vcodes, float* kscale, float* vscale, const float* cos_tab,
                             const float* sin_tab, const int32_t* pos0_dev, int G, int T, int H, int D, int Tmax,
                             int64_t cache_seq_stride, int64_t scale_seq_stride, int table_dtype, int emulate, void* stream);
/* Causal attention of a T-token chunk per sequence over the fp32 cache, fp32 FMA arithmetic and softmax
 * (modeling_llama_xformer.py:204-239: prefill causal, q_len == 1 sees the whole cache): row t sees keys 0 .. pos0[g] + t.
 * Device-resident positions → graph-capturable for the decode step (T = 1). Output = the planes of the context rows [G*T][H*D].
 * causal = 0: every row sees all Tmax keys (pos0_dev unused) — with the K / V strides below this is also the small fp32 attention of
 * ResamplerXLV2's precise mode (PerceiverAttention / AttentionPool2d, resampler.py:42-87,89-116: fp32 softmax over <= 129 keys). */
typedef struct sx_attn_f32_args {
  const float* q;           /* rotated q: row g*T + t at q + row*q_row_stride, head h at + h*D (e.g. the qkv buffer, stride 3*H*D) */
  const float* kcache;      /* fp32 [G][H][Tmax][D], sequences cache_seq_stride floats apart                                       */
  const void* vcache;       /* fp32, or — v16 = 1 — the "mixed" cache's 16-bit V (the planes' dtype) with the same ELEMENT strides     */
  void* out;                /* planes of [G*T][H*D], layout by dtype (see above)                                                    */
  const int32_t* pos0_dev;  /* [G] cache position of each sequence's first chunk token (causal)                                    */
  int64_t q_row_stride, cache_seq_stride;
  int64_t kv_row_stride;    /* floats between consecutive keys of a head (0 = D)                                                   */
  int64_t kv_head_stride;   /* floats between heads (0 = Tmax*D: the cache layout)                                                  */
  int32_t G, T, H, D, Tmax, dtype;
  float scale;
  int32_t causal;           /* 1: row t sees keys 0 .. pos0[g] + t; 0: all Tmax keys                                               */
  int32_t v16;              /* 0: fp32 V (default); 1: V is 16-bit, in the planes' dtype (head_dim <= 128): the mixed cache          */
  int32_t nsplit;           /* T == 1 only: > 1 spreads the keys of every (head, sequence) over nsplit workgroups + a combine launch   */
  float* scratch;           /* nsplit > 1: fp32 [G][H][nsplit][D + 2] partial results                                                */
  /* T == 1, causal, D == 128 only — RoPE + KV append fused into the step (modeling_llama_xformer.py:141-149,204-244 in ONE launch
   * per layer): rope_cos != NULL means q is the UNROTATED row, k_new / v_new are the new token's rows (row stride q_row_stride: the
   * qkv buffer's + H*D and + 2*H*D), and the launch appends the rotated k and v (rounded when v16) to kcache / vcache at pos0[g] —
   * the two cache pointers are written through in this form. NULL (default) = sx_rope_kv_append_f32* ran before.
   * 2 <= T <= 8 with rope_cos is the VERIFY form of speculative decoding (G*T <= 32, kv_fp8 = 0, nsplit >= 1, scratch fp32
   * [G*T][H][nsplit][D + 2] always): q / k_new / v_new are rows g*T + t, row t sits at position pos0[g] + t. The launch equals, bit
   * for bit, T successive T = 1 calls of this form with the same nsplit, v16 and dtype (call t on row t at position pos0[g] + t) in
   * the context planes, the k rows and the v rows of every row whose position lies in [0, Tmax); every K / V row of a (head,
   * sequence, split) is loaded once for the T query rows. pos0[g] < 0 (a parked slot, here and in every causal form) idles all T rows
   * of the slot: they read no key row, write no cache row and come out as 0, whatever a reused cache still holds; a row at or past
   * Tmax writes no cache row and stays finite. */
  const float* rope_cos;    /* [Tmax][D/2] fp32 (rounded to the planes' dtype inside, like sx_rope_kv_append_f32)                    */
  const float* rope_sin;
  const float* k_new;
  const float* v_new;
  /* FP8 KV cache (head_dim 128, causal, the cache layout; excludes v16). 0 (default, also a zero-initialised struct): off.
   * 1: kcache / vcache hold e4m3fn codes (uint8, the same ELEMENT strides) and k_scale / v_scale one power-of-two fp32 scale per key row
   *    [G][H][Tmax], sequences scale_seq_stride floats apart; the result equals, bit for bit, the fp32 call on a cache holding
   *    decode(code) * scale. In the fused RoPE form the new token's rows are quantised (sx_rope_kv_append_f32_q8's rule) and appended.
   * 2: meaningful in the fused RoPE form only — fp32 caches, the new token's k / v stored (and attended to) as their quantised and
   *    dequantised values: the bit-reference twin of 1. Without rope_cos it is the plain fp32 call. */
  int32_t kv_fp8;
  const float* k_scale;
  const float* v_scale;
  int64_t scale_seq_stride;
  /* Paged cache (LlamaForCausalLM(kv_pages=N); head_dim 128, causal, kv_fp8 = 0, not the verify form — each refused with a message).
   * NULL (default, also a zero-initialised struct): the contiguous addressing above, the very launches of a build without paging.
   * Else kcache / vcache are page POOLS [n_pages + 1][H][page size][D] (page size = 1 << page_shift = 32, 64 or 128 rows; pages
   * page_stride elements apart; v16 as above) and page_table is device int32 [G][ceil(Tmax / page size)]: key row t of sequence g lives
   * in page page_table[g][t >> page_shift] at row t & (page size - 1). cache_seq_stride and the K / V strides are unused. Page 0 is the
   * NULL page — all zeros, never handed out, never written: an entry without a reservation names it, so whatever the contiguous kernels
   * read from rows nobody owns (the MFMA tile's rows past the last visible key) reads finite zeros, and the
   * fused append of a row whose entry is 0 writes nothing. Entries are clamped to [0, n_pages]: a wrong table gives wrong numbers, never
   * a wild address. The table is read at launch (at replay under a captured graph); one lookup per page (VALU kernels) or per 32-key
   * tile (MFMA kernel). Every launch has the bits of the contiguous call on a cache holding the same rows. */
  const int32_t* page_table;
  int32_t page_shift, n_pages;
  int64_t page_stride;
} sx_attn_f32_args;
int sx_attention_f32(const sx_attn_f32_args* args, void* stream);
/* tuning / test hook: 1 (default) = causal chunks above 8 tokens at head_dim 128 run on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32)
 * flash kernel; 0 = the VALU kernels everywhere (the bit-reference of its test, and the A/B) */
int sx_attention_f32_variant(int v);
/* strided 2-D copy of fp32 rows: dst[r][dst_off + c] = src[r][c]  (channel concat of skip connections) */
int sx_copy2d_f32(const float* src, int64_t src_ld, float* dst, int64_t dst_ld, int64_t rows, int cols,
                  void* stream);
/* y = a + b (fp32), n elements */
int sx_add_f32(const float* a, const float* b, float* y, int64_t n, void* stream);
/* ViT patchify: img[B][3][S][S] (fp32) → patches[B*(S/P)^2][Kpad] 16-bit, k = c*P*P + py*P + px, zero padded
 * (conv1 as a GEMM, qwen_visual.py:352,393-396) */
int sx_patchify(const float* img, void* patches, int B, int S, int P, int Kpad, int dtype, void* stream);
/* generic 3x3/pad1 im2col for tiny Cin (UNet conv_in, Cin = 4|8): x[B][H][W][Cin] fp32 → [B*H*W][Kpad] */
int sx_im2col3x3_small(const float* x, void* out, int B, int H, int W, int Cin, int Kpad, int dtype,
                       void* stream);
/* avg_pool1d(k=4,s=4) over tokens: x[B][L][D] → y[B][L/4][D] fp32 (adapter_modules.py:112-115) */
int sx_avgpool_tokens(const float* x, float* y, int B, int L, int D, int k, void* stream);
/* sinusoidal timestep embedding, flip_sin_to_cos=True, shift 0 (diffusers Timesteps [ext]):
 * out[i][:] = [cos(t_i*f_j) | sin(t_i*f_j)], f_j = exp(-ln(10000) * j / half); t_i = t[i], or t[*idx_dev] for every
 * row when idx_dev != NULL (denoise-step counter kept on the device so the step is graph-replayable) */
int sx_timestep_embedding(const float* t, const int32_t* idx_dev, void* out, int n, int dim, int dtype, void* stream);
/* NCHW fp32 ↔ NHWC fp32 for the 4/8-channel latents; ld = channel stride of the NHWC side */
int sx_nchw_to_nhwc(const float* src, float* dst, int ld, int B, int C, int HW, void* stream);
int sx_nhwc_to_nchw(const float* src, int ld, float* dst, int B, int C, int HW, void* stream);
/* *p += delta on the device (step / position counters of graph-replayed loops) */
int sx_add_i32(int32_t* p, int delta, void* stream);
/* profiling hook: one empty dispatch of `profile_marker_kernel` (tools/kstats_step.py cuts a rocprofv3 kernel trace at these) */
int sx_profile_marker(int tag, void* stream);
/* y = silu(x) as 16-bit (ResnetBlock2D.time_emb_proj input: nonlinearity(temb), diffusers [ext]); the exponential and the quotient are
 * taken in fp64 and rounded once, so the result holds down to the smallest normal of the output type; n = 0 is SX_OK, like sx_cast */
int sx_silu_cast(const float* x, void* y, int dtype, int64_t n, void* stream);

/* Fused classifier-free guidance + Euler step on fp32 latents (NHWC [1][HW][C], n = HW*C; eps [nb][HW][C]).
 * mode 0 (t2i, StableDiffusionXLPipeline.__call__ [ext]; order [uncond, text]):
 *     eps = e0 + gs*(e1 - e0);  lat += eps * (sigma_next - sigma)
 * mode 1 (edit, pipeline_stable_diffusion_xl_t2i_edit.py:926-953; order [text, image, uncond]):
 *     x0_k = lat - sigma*e_k;  x0 = x0_u + gs*(x0_t - x0_i) + igs*(x0_i - x0_u);
 *     eps = (x0 - lat)/(-sigma);  lat += eps * (sigma_next - sigma)
 * Also writes the next step's scaled model input: scaled[k][hw][c] = lat_new / sqrt(sigma_next^2 + 1), k < nb,
 * into an NHWC buffer with channel stride ld_scaled (8 for the edit UNet: channels 4..7 hold the image latents).
 * sigmas live on the device (sigmas_dev[step], sigmas_dev[step+1]); step read from *step_dev. */
int sx_cfg_euler_step(const float* eps, float* latents, float* scaled_next, const float* sigmas_dev,
                      const int32_t* step_dev, int nb, int64_t n, int C, int ld_scaled, float gs, float igs, int mode,
                      void* stream);
/* Fused classifier-free guidance + DPM-Solver++(2M) step (Lu et al. 2022, Algorithm 2: second order, multistep, one UNet evaluation per
 * step) on the same buffers and layout as sx_cfg_euler_step, plus x0_prev [HW][C] fp32, the previous step's denoised sample.
 * coef_dev [steps][3] fp32 holds (a, b, c) of every step, computed on the host (seedx_amd/solvers.py: a = sigma'/sigma,
 * b = 1 - e^-h, c = h / (2 h_last); c = 0 on step 0 and on the step onto sigma' = 0, whose row is (0, 1, 0)): the kernel takes no
 * logarithm or exponential.
 *     mode 0: e = e0 + gs*(e1 - e0);  x0 = lat - sigma*e
 *     mode 1: x0_k = lat - sigma*e_k;  x0 = x0_u + gs*(x0_t - x0_i) + igs*(x0_i - x0_u)
 *     d = x0 + c*(x0 - x0_prev);  lat = a*lat + b*d;  x0_prev = x0;  scaled[k][hw][c] = lat / sqrt(sigma_next^2 + 1), k < nb
 * x0_prev is NOT read when c = 0, so it needs no initial value. scaled_next may be NULL; channels C..ld_scaled-1 are never written.
 * step is read from *step_dev; a negative step reads row 0, and the caller keeps step + 1 inside sigmas_dev (the kernel knows no table
 * length, like sx_cfg_euler_step). n = 0 is SX_OK. SX_ERR_INVALID: a null pointer, nb / mode other than (2, 0) or (3, 1), C <= 0,
 * n % C != 0, ld_scaled < C. */
int sx_cfg_dpmpp2m_step(const float* eps, float* latents, float* x0_prev, float* scaled_next, const float* sigmas_dev,
                        const float* coef_dev, const int32_t* step_dev, int nb, int64_t n, int C, int ld_scaled, float gs, float igs,
                        int mode, void* stream);

/* In-flight batching of the denoise loop: G generations ("slots") share ONE captured UNet step, rows ordered [branch][slot], and every
 * slot carries its own step counter, schedule and guidance scales in device memory. Slot g is LIVE when 0 <= step_dev[g] < n_steps_dev[g],
 * PARKED otherwise (the host parks a slot with step -1).
 *
 * sx_cfg_euler_step_slots: sx_cfg_euler_step on every live slot's n_slot = HW*C elements (eps [nb][G][HW][C], latents [G][HW][C],
 * scaled_next [nb][G][HW][ld_scaled]) with sigma = sig_tab[g][step], sigma_next = sig_tab[g][step + 1] (sig_tab [G][ld_sig] fp32; both
 * indices are clamped into [0, ld_sig), so a wrong table gives wrong numbers, never a wild address), gs_dev[g] and igs_dev[g]. The
 * arithmetic is sx_cfg_euler_step's instruction for instruction: a live slot's result equals that kernel's on the slot's rows bit for
 * bit. For a parked slot nothing is written: not its latents, not its rows of any branch of scaled_next. Channels C..ld_scaled-1 of
 * scaled_next are never written. */
int sx_cfg_euler_step_slots(const float* eps, float* latents, float* scaled_next, const float* sig_tab, int ld_sig,
                            const int32_t* step_dev, const int32_t* n_steps_dev, const float* gs_dev, const float* igs_dev, int nb,
                            int G, int64_t n_slot, int C, int ld_scaled, int mode, void* stream);
/* sx_cfg_dpmpp2m_step on every live slot (x0_prev [G][HW][C]; the other buffers as for sx_cfg_euler_step_slots) with the slot's own
 * sigmas sig_tab[g][step], sig_tab[g][step + 1] and coefficients coef_tab[g][step] (coef_tab [G][ld_sig][3] fp32; the indices are
 * clamped into [0, ld_sig)). The arithmetic is sx_cfg_dpmpp2m_step's instruction for instruction: a live slot's latents, x0_prev and
 * scaled_next rows equal that kernel's bit for bit. For a parked slot nothing is written: not its latents, not its x0_prev, not its rows
 * of scaled_next. One launch may hold slots on step 0 (c = 0), mid-way and on their last step (sigma' = 0). The step counters move with
 * sx_denoise_advance, as for the Euler step. */
int sx_cfg_dpmpp2m_step_slots(const float* eps, float* latents, float* x0_prev, float* scaled_next, const float* sig_tab,
                              const float* coef_tab, int ld_sig, const int32_t* step_dev, const int32_t* n_steps_dev,
                              const float* gs_dev, const float* igs_dev, int nb, int G, int64_t n_slot, int C, int ld_scaled, int mode,
                              void* stream);
/* out [nb*G][dim]: row k*G + g = sx_timestep_embedding's row for t = t_tab[g][step_dev[g]] (t_tab [G][ld_t] fp32), bit for bit; a slot
 * whose step is outside [0, ld_t) (a parked slot: -1) embeds t = 0, which is finite */
int sx_timestep_embedding_slots(const float* t_tab, int ld_t, const int32_t* step_dev, void* out, int G, int nb, int dim, int dtype,
                                void* stream);
/* last node of a slot step, in a launch of its own (every workgroup of sx_cfg_euler_step_slots reads the counters): a live slot's step
 * becomes step + 1, or -1 once that reaches n_steps_dev[g] (the slot parks itself); a parked slot's becomes / stays -1 */
int sx_denoise_advance(int32_t* step_dev, const int32_t* n_steps_dev, int G, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Image pre/post-processing: the byte work either side of the dense paths.
 * ------------------------------------------------------------------------------------------------ */
/* Pillow `Image.resize` for 8-bit images (ImagingResample, Resample.c [ext Pillow]), bit exact: separable antialiased
 * convolution in 22-bit fixed point, horizontal pass (→ uint8) then vertical pass (→ uint8).
 * replaces: `image.resize(...)` (default BICUBIC) at src/inference/any_res.py:104,111,183,187 and torchvision
 * `transforms.Resize` on PIL input (BILINEAR) at src/processer/transforms.py:8-14.
 * src: [Hin][Win][C] uint8, row stride src_stride bytes; dst: dense [Hout][Wout][C] uint8. C = 1 | 3.
 * kk_h / bounds_h (kk_v / bounds_v): Pillow's normalize_coeffs_8bpc(precompute_coeffs(...)) tables built by the host:
 * kk[out][ksize] int32, bounds[out][2] = {first input index, count}. A NULL kk_* skips that pass (Pillow does the same
 * when the size along that axis is unchanged). With both passes, `tmp` holds the horizontally resampled rows
 * [y_first, y_first + y_rows) — the rows the vertical pass touches — as dense [y_rows][Wout][C] uint8. */
int sx_resample_u8(const void* src, int Hin, int Win, int C, int64_t src_stride, void* dst, int Hout, int Wout,
                   const int32_t* kk_h, const int32_t* bounds_h, int ksize_h, const int32_t* kk_v,
                   const int32_t* bounds_v, int ksize_v, int y_first, int y_rows, void* tmp, void* stream);
/* crop + ToTensor + Normalize in one gather: dst[c][y][x] = lut3x256[c][src[y0+y][x0+x][c]], dst fp32 [3][Hc][Wc].
 * replaces: `image.crop(box)` (any_res.py:130-134), transforms.ToTensor() and transforms.Normalize(mean, std)
 * (src/processer/transforms.py:16-19). The host builds lut[c][v] = (float32(v)/255 - mean[c]) / std[c] in float32. */
int sx_u8_to_chw_lut(const void* src, int H, int W, int64_t src_stride, int x0, int y0, int Hc, int Wc,
                     const float* lut3x256, float* dst, void* stream);
/* VaeImageProcessor.postprocess(output_type="pil") [ext diffusers] as called at
 * pipeline_stable_diffusion_xl_t2i_edit.py:986: src fp32 [3][H][W] → dst uint8 [H][W][3],
 * u = round_half_even(clamp(x/2 + 0.5, 0, 1) * 255). */
int sx_chw_to_u8_image(const float* src, int H, int W, void* dst, void* stream);
/* ids_cmp_mask of eval_img2text_seed_x_i.py:153-160: mask[i] = 1 strictly between the k-th opening marker (boi | bop)
 * and the k-th closing marker (eoi | eop), pairs formed like zip(boi_indices, eoi_indices). ids: int64 [T]; mask: uint8 [T]. */
int sx_marker_mask(const int64_t* ids, int T, int64_t boi, int64_t bop, int64_t eoi, int64_t eop, void* mask,
                   void* stream);
/* F.normalize(x) with its default dim=1 on x[B][T][D] fp32 (the token axis — ResamplerXLV2(normalize=True),
 * src/models/detokenizer/resampler.py:271-272): y = x / max(||x[b,:,d]||_2, eps). */
int sx_l2norm_dim1(const float* x, float* y, int B, int T, int D, float eps, void* stream);

/* ------------------------------------------------------------------------------------------------
 * One-shot all-reduce / all-gather over peer-mapped device memory (csrc/comm.hip): the tensor-parallel decode step's
 * 20 KB - 320 KB collectives as ONE graph-capturable kernel launch per rank. No reference counterpart (the reference is
 * single-device inference; src/train/dist_utils.py:5-34 is its only collective code): north_star's TP requirement.
 * The payload is cut into chunks of `chunk` floats (SX_ONESHOT_CHUNK unless overridden); one workgroup per chunk runs the
 * whole publish / signal / wait / reduce protocol on its own epoch counter and flag row, all chunks in flight at once.
 * Set-up (once): every rank sx_comm_alloc()s a staging area (2 x cap floats) and a flag array ((cap / chunk) x world x uint32),
 * sx_ipc_export()s both, sends the 64-byte handles to its peers (any transport), sx_ipc_open()s the peers' handles and
 * stores the world pointers in two DEVICE arrays (own buffers at index rank).
 * ------------------------------------------------------------------------------------------------ */
int sx_comm_alloc(void** ptr, uint64_t bytes);          /* zero-initialised device memory that can be exported        */
int sx_comm_free(void* ptr);
int sx_ipc_export(void* ptr, unsigned char* handle64);  /* hipIpcGetMemHandle: 64 opaque bytes                        */
int sx_ipc_open(const unsigned char* handle64, void** ptr);
int sx_ipc_close(void* ptr);
#define SX_ONESHOT_CHUNK 4096 /* floats per workgroup: 16 KB                                                          */
typedef struct sx_oneshot_args {
  void* data;         /* fp32 [n]: all-reduce in place (gather_out == NULL) or the all-gather input                    */
  void* gather_out;   /* fp32 [world][n] or NULL                                                                       */
  const void* stage;  /* DEVICE array of `world` pointers: rank r's staging area                                       */
  const void* flags;  /* DEVICE array of `world` pointers: rank r's flag array                                         */
  void* epoch;        /* this rank's uint32 epoch counters [cap / chunk] (device, zero at start; advanced by the kernel) */
  void* status;       /* uint32 (device): non-zero after a peer failed to arrive within max_spin polls                */
  int32_t n, cap, rank, world;
  uint32_t max_spin;  /* 0 = default (2^22 polls, a few seconds)                                                       */
  int32_t chunk;      /* floats per workgroup, even, divides cap; 0 = SX_ONESHOT_CHUNK. Fixed for the life of the buffers */
  int32_t mode;       /* 0: all-reduce / all-gather among all ranks. 1: NEIGHBOUR exchange (the row-sharded UNet's conv halo rows,
                       * seqpar.py): data = [my last row | my first row] (n floats, n even), gather_out[n] receives [last row of rank - 1 |
                       * first row of rank + 1] (zeros at the ends of the chain); a rank signals and waits for its one or two
                       * neighbours only. Use a communicator of its own for this mode (its epochs must not interleave with mode 0:
                       * a slot is reused once the NEIGHBOURS have moved on) */
  int32_t reserved;
} sx_oneshot_args;
int sx_allreduce_oneshot(const sx_oneshot_args* args, void* stream);

/* Row-sharded 3x3 convolution input (seqpar.with_halo): out[B][Hl + 1 (+1 if bottom)][W + left_col][C] 16-bit = the local slab
 * x[B][Hl][W][C] with the neighbour rows above (prev_row[B][W][C], NULL = zeros: image border) and below (next_row) and, with
 * left_col, a zero column on the left — one launch instead of torch.zeros + three slice copies. C % 8 == 0. */
int sx_halo_pack(const void* x, const void* prev_row, const void* next_row, void* out, int B, int Hl, int W, int C, int left_col,
                 int bottom, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SEEDX_HIP_H */
