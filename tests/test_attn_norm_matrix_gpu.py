"""sx_attention, sx_attention_small, sx_layernorm (LayerNorm / RMSNorm, wave and block kernel), sx_groupnorm2 / sx_groupnorm_sp and
sx_softmax_rows against fp64, element by element, in the manner of tests/test_gemv_matrix_gpu.py (whose GBuf, TiledOut, same_bits and
stops_on_gpu_fault are imported, with the NaN patterns of tests/test_gemm_matrix_gpu.py).

Every case drives the C entry point through _lib, so every stride and leading dimension is free, and checks
  * every output element against an fp64 reference computed with torch on the GPU from the SAME 16-bit / fp32 operands, with the
    bound of its section below;
  * that nothing outside the logical output is written: outputs live in guard buffers (GBuf / TiledOut) whose other bytes must be
    bit-unchanged, while every logical element must be finite;
  * that nothing outside a logical input is read: inputs are views into NaN-filled buffers; columns D .. head stride, rows >= Skv (Sq)
    inside the allocation, columns cols .. ld, rows >= HW and the elements behind every operand hold NaN;
  * that a second identical launch gives the same bits (GroupNorm: the fp64 atomics of the statistics claim order independence).
WORST collects the worst |diff| / bound per (kernel instantiation, dtype); the last test prints it. kernel_of_* restate the dispatch
rules of the host code by hand; tests/test_cpu_suite.py holds the case tables against the instantiations in norm.hip / attn.hip.

Roundings: U32 = 2^-24 (fp32), u16 = 2^-11 (fp16) / 2^-8 (bf16). `rnd(ref, dt)` is the output rounding u_out * |ref|, or half a unit of
the smallest subnormal of fp16 (2^-25) where that is larger: a result below the smallest normal is rounded to the subnormal grid; for
bf16 and fp32 the floor is 2^-126, the smallest normal (a hardware exp2 or multiply may flush below it).

1. sx_attention (attn_kernel<F16 | BF16, 64 | 128>). p = softmax(scale Q K^T) and A_d = sum_j p_j |V_jd| in fp64:
       |got - ref| <= u_out |ref| + 2 u16 A_d + C32 2^-24 A_d
   One u16 is P rounded to the operand type before P.V; the other is the normaliser, which sums the rounded P (so numerator and
   denominator carry the same roundings, each bounded by u16 of its own terms). C32 = 64 collects the fp32 steps, on the square-root
   law that C_ACC * sqrt(K) of the GEMM matrices uses and for exponents of up to E = 16 log2 units (8 / ln 2 = 11.5 for a planted key,
   4.5 sigma at scale 4 / sqrt(D)): the score is D / 16 <= 8 chained MFMA accumulations, 1 ulp of |s| each: sqrt(8) * E * ln 2 = 31;
   the exp2 argument is ONE fma, 1/2 ulp of <= E: E ln 2 / 2 = 5.5; v_exp: 1; O and the normaliser are Skv / 16 <= 44 chained
   accumulations of non-negative weights each (Skv <= 700): 2 * sqrt(44) = 13.3, the alpha rescales (every tile at worst, 11 tiles,
   both): 2 * sqrt(11) = 6.6; reciprocal and product: 2. Sum 60 <= 64. The deferred reference of the D = 64 kernel keeps P <= 2^8: the
   same RELATIVE rounding of P, so no term of its own. (The staircase cases carry |s| of 60 and more log2 units: their fp32 term is
   larger than C32 allows on its own, while 2 u16 is 2^6 (fp16) to 2^9 (bf16) times the whole fp32 term: the sum is what is asserted.)
   Second assert: relative L2 per (batch, head, query) row below 2 TOL = 1.2e-3 (fp16) / 8e-3 (bf16), test_attention_mfma's bounds.
   Planted keys: row i owns key pi(i), K[pi(i)] = q_i * 8 / (scale |q_i|^2) (score exactly 8 before the rounding to the type); pi is
   injective, starts with the edge positions {0, 63, 64, 127, 128, last full tile's last key, Skv-2, Skv-1} and goes on with
   (37 i) mod Skv; causal: pi(i) = i + Skv - Sq, the row's mask edge. With Sq > Skv only the first Skv rows own a key. For D >= 40
   the reference asserts that every planted key weighs >= 0.25 in its row (not for D = 8 / 16: random queries are not nearly
   orthogonal there).

2. sx_attention_small (attn_small_kernel<F16 | BF16>): P stays fp32, so
       |got - ref| <= u_out |ref| + C32s 2^-24 A_d,      C32s = 2 (C_ACC sqrt(D) S1 + 3) + 2 C_ACC sqrt(Skv) + 4
   S1 = max_ij scale sum_d |q_id k_jd| (>= 1; fp64, from the operands): a score is one sequential fp32 sum of D products
   (C_ACC sqrt(D) 2^-24 of sum |q k|, relative on p after the scaling; the scaled q is rounded once: + 1), __expf: 2; twice, for
   numerator and normaliser. The normaliser (Skv / 64 per lane, then 6 butterfly steps) and the P.V sum (Skv sequential) are sums of
   non-negative weights: C_ACC sqrt(Skv) each covers both chains. Reciprocal, product, max subtraction, conversion: 4.

3. sx_layernorm (layernorm_kernel<DT, NV>, layernorm_block_kernel<DT>), two-pass in registers:
       |got - ref| <= u_out |ref| + C 2^-24 (|x_i - mean| + |mean|) rstd |gamma_i| + 2^-24 |beta_i|       (RMS: without the mean terms)
   C = 2 n + 10 with n = ceil(cols / 4 / lanes) + 11 the longest chain of fp32 additions of one reduction (lanes = 64 | 256): one
   addition per quad of the lane (the quad itself is a 2-level tree: + 2), 6 butterfly steps, the block kernel's sum of 4 wave
   results (+ 2), the division (+ 1). Worst case (1 ulp per addition; all terms of the second sum are non-negative, and for
   mean / std >= 1 so are almost all of the first): the mean is off by <= (n + 1) 2^-24 sum|x| / cols <= 2 (n + 1) 2^-24 |mean|; the
   variance by (n + 3) 2^-24 relative, rstd by half of it + 2 (v_rsq) + 2 (eps, division); x - mean: 1; the two products and the
   addition of beta: 3 of |x^ gamma| and the 2^-24 |beta| of the formula. The bound has no term for the error of the mean of a row
   with mean / std ~ 0 (there it is relative to std, not to |mean|): the rows of that kind are built on a grid on which the fp32 row sum
   is exact (antisymmetric values, multiples of 2^-8 (f32, f16) / 2^-4 (bf16) below 8), so their computed mean is exactly 0.

4. sx_groupnorm2 / sx_groupnorm_sp (gn_stats_kernel<TWO>, gn_apply_kernel<TWO>). x^ the normalised value, kappa = (mean^2 + var) / var
   of the element's group:
       |got - ref| <= u_out |ref| + C 2^-24 (|x^ gamma| + |beta|) + Cv n_acc 2^-24 kappa |x^ gamma| / 2
   n_acc = 2 rows_stats + cpg / 2 + 2 is the longest fp32 chain of gn_stats_kernel (a thread adds two values per row to each of its
   sums over the block's rows_stats rows, one thread then adds the group's cpg / 2 channel pairs; + 2: the square and the in-quad
   addition); the blocks meet in fp64, exactly. Cv = 3: the sum of squares is off by n_acc 2^-24 of itself = n_acc 2^-24 kappa var, the
   mean by n_acc 2^-24 sqrt(mean^2 + var), which enters var through 2 |mean| d(mean) <= 2 n_acc 2^-24 kappa var; rstd takes half of
   the relative error of var (the / 2). C = 14: gn_apply_kernel rounds rstd, gamma rstd, mean, mean * (gamma rstd), beta - that,
   x * scale and the final sum: 7 roundings of magnitudes <= |x^ gamma| + 2 |beta| as long as |mean| rstd |gamma| <= |beta|, which the
   data of every case but the conditioning case keeps (|beta| >= 0.5, |gamma| <= 1.5, group mean / std <= 0.3). SiLU: the bound times its
   Lipschitz constant LIP = 1.10 plus C_EP 2^-24 |pre-activation|, as in the GEMM matrices. The formula has no term for
   2^-24 |mean| rstd |gamma| at x^ ~ 0: in the conditioning case (mean / std up to 100) that is 100 2^-24 |gamma|, below the 16-bit
   output rounding of |beta| >= 0.5, so the case asserts the 16-bit outputs and prints the fp32 figure (profiles/attn_norm_matrix.md).

5. sx_softmax_rows (softmax_rows_kernel<F16 | BF16 | BF16, true>):
       |got - ref| <= u_out ref + C 2^-24 (1 + max_c |scale x| log2e) ref,      C = 4 ceil(cols / 1024) + 20
   the row sum: 4 additions per thread and 1024 columns, 6 butterfly steps, 3 for the four waves (all terms positive: 1 ulp each);
   the exponent x * (scale log2e) - m: the rounding of scale log2e and of the product or fma, twice (numerator and every term of the
   sum): 4 ln 2 < 3 per unit of |scale x| log2e; exp2f 2 ulp, twice: 4; reciprocal and product: 2; the rest is slack below the 1 +.
   The rounded maximum m is the same number in numerator and denominator. Row sums of the stored values: |sum - 1| <= cols u_out / 2 + 1e-6.
"""
import ctypes as C
import math
import os
import re
import zlib

import pytest
import torch

from tests.test_gemm_matrix_gpu import BF16, C_ACC, C_EP, DTYPES, F16, LIP, NAN16_IN, NAN32_IN, TOL, U32, _nanbuf
from tests.test_gemv_matrix_gpu import GBuf, TiledOut, same_bits, stops_on_gpu_fault

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORM_HIP = os.path.join(ROOT, "seed-x_amd", "csrc", "norm.hip")
ATTN_HIP = os.path.join(ROOT, "seed-x_amd", "csrc", "attn.hip")

F32 = torch.float32
ALL_DT = {"f16": F16, "bf16": BF16, "f32": F32}
U_OUT = {F16: 2.0 ** -11, BF16: 2.0 ** -8, F32: U32}
FLOOR = {F16: 2.0 ** -25, BF16: 2.0 ** -126, F32: 2.0 ** -126}
C32_ATTN = 64.0
C_GN, CV_GN = 14.0, 3.0
WORST = {}               # (kernel instantiation, dtype) -> worst |diff| / bound
NOTES = {}               # free-form measured figures, printed by the last test
assert (NAN16_IN, NAN32_IN) == (0x7FFF, 0x7FFFFFFF)      # what _nanbuf fills inputs with; GBuf / TiledOut fill outputs with NAN16_GUARD / NAN32_GUARD


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


def held(key, got, ref, bound, what):
    """Every element within its bound; records and returns the worst ratio."""
    d = (got - ref).abs()
    ratio = d / bound
    worst = float(ratio.max())
    WORST[key] = max(WORST.get(key, 0.0), worst)
    if not worst <= 1.0:
        i = int(torch.nan_to_num(ratio, nan=float("inf")).argmax())
        idx = []
        for n in reversed(ratio.shape):
            idx.insert(0, i % n)
            i //= n
        idx = tuple(idx)
        raise AssertionError(f"{what} [{key}]: {int((~(ratio <= 1.0)).sum())} of {ratio.numel()} elements beyond the fp64 bound; worst at {idx}: got "
                             f"{float(got[idx])!r}, ref {float(ref[idx])!r}, |diff| {float(d[idx]):.3e} > bound {float(bound[idx]):.3e}")
    return worst


# ----------------------------------------------------------------------------------------------------------------------------
# 1 / 2. attention
# ----------------------------------------------------------------------------------------------------------------------------
def acase(cid, dt, **kw):
    c = dict(id=cid, dt=dt, small=False, B=1, H=2, Sq=70, Skv=100, D=64, causal=False, layout="plain", data="plant", scale_mul=1.0)
    c.update(kw)
    c["id"] = f"{cid}-{dt}-B{c['B']}H{c['H']}-Sq{c['Sq']}-Skv{c['Skv']}-D{c['D']}{'-causal' if c['causal'] else ''}"
    return c


def kernel_of_attn(c):
    """sx_attention: attn_kernel<TT, DP> with DP = 64 for D <= 64, else 128; sx_attention_small: attn_small_kernel<TT>."""
    tt = c["dt"].upper()
    return ("attn_small_kernel", tt) if c["small"] else ("attn_kernel", tt, 64 if c["D"] <= 64 else 128)


STAIR_SKV = 768          # 12 tiles of 64 keys


def attn_cases():
    out = []
    for dt in DTYPES:
        A = lambda cid, **kw: out.append(acase(cid, dt, **kw))
        for D in (8, 16, 40, 56, 64, 72, 96, 104, 128):
            A("hd", B=1, H=3, Sq=130, Skv=200, D=D)
        for D in (64, 128):
            for Skv in (1, 63, 64, 65, 127, 128, 129, 700):
                A("skv", B=2, H=2, Sq=70, Skv=Skv, D=D)
            for Sq in (1, 31, 32, 33, 127, 128, 129, 300):
                A("sq", B=1, H=2, Sq=Sq, Skv=100, D=D)
            for Sq, Skv in ((1, 1), (1, 65), (64, 229), (129, 129), (200, 333), (300, 300)):
                A("causal", B=1, H=2, Sq=Sq, Skv=Skv, D=D, causal=True)
            A("stair-up", B=1, H=2, Sq=70, Skv=STAIR_SKV, D=D, data="stair_up")
            A("stair-first", B=1, H=2, Sq=70, Skv=STAIR_SKV, D=D, data="stair_first")
            A("scale4", B=2, H=2, Sq=130, Skv=333, D=D, data="randn", scale_mul=4.0)
        A("causal", B=2, H=1, Sq=200, Skv=333, D=104, causal=True)
        # B * H * q_tiles = 1, 7, 9, 24: xcd_remap on grids that are no multiple of 8
        for B, H, Sq in ((1, 1, 70), (1, 1, 7 * 128 - 5), (1, 3, 300), (2, 3, 500)):
            A("grid", B=B, H=H, Sq=Sq, Skv=100, D=64)
        for i, lay in enumerate(("qb0", "bsh3d", "bs3hd", "kvfused", "kvdiff", "opad", "gap")):
            A(f"lay-{lay}", B=3, H=2, Sq=130, Skv=130, D=(64, 104)[i % 2], layout=lay)
            A(f"lay-{lay}", B=3, H=2, Sq=130, Skv=130, D=(128, 40)[i % 2], layout=lay)
        # sx_attention_small
        S = lambda cid, **kw: out.append(acase(cid, dt, small=True, **kw))
        for D in (8, 64, 160, 256):
            S("small-hd", B=1, H=3, Sq=5, Skv=65, D=D)
        for Skv in (1, 63, 64, 65, 1536):
            S("small-skv", B=1, H=2, Sq=3, Skv=Skv, D=64)
        for Sq in (1, 3, 4, 5, 64):
            S("small-sq", B=1, H=3, Sq=Sq, Skv=63, D=64)               # B * H * Sq % 4 = 3, 1, 0, 3, 0
        S("small-lay-qb0", B=3, H=2, Sq=5, Skv=65, D=64, layout="qb0")
        S("small-lay-kvfused", B=2, H=3, Sq=3, Skv=64, D=160, layout="kvfused")
        S("small-lay-gap", B=2, H=1, Sq=5, Skv=65, D=8, layout="gap")
    return out


ATTN = attn_cases()
XR = 3                   # NaN rows behind the last row of every attention operand, inside its allocation


def attn_layout(c):
    """Where Q, K, V and O live: name -> (buffer key, element offset, batch stride, row stride, head stride); buffer sizes in elements."""
    B, H, Sq, Skv, D, lay = c["B"], c["H"], c["Sq"], c["Skv"], c["D"], c["layout"]
    L, size = {}, {}

    def sep(name, S, hs, rs_extra=0, bs_extra=0, bcast=False):
        rs = H * hs + rs_extra
        bs = (S + XR) * rs + bs_extra
        L[name] = (name, 0, 0 if bcast else bs, rs, hs)
        size[name] = (1 if bcast else B) * bs

    if lay in ("bsh3d", "bs3hd"):
        assert Sq == Skv
        hs, rs = (3 * D, 3 * H * D) if lay == "bsh3d" else (D, 3 * H * D)
        step = D if lay == "bsh3d" else H * D
        for i, n in enumerate("QKV"):
            L[n] = ("QKV", i * step, (Sq + XR) * rs, rs, hs)
        size["QKV"] = B * (Sq + XR) * rs
    else:
        if lay == "gap":
            sep("Q", Sq, D + 8)
        else:
            sep("Q", Sq, D, bcast=lay == "qb0")
        if lay == "kvfused":
            rs = 2 * H * D
            L["K"], L["V"] = ("KV", 0, (Skv + XR) * rs, rs, D), ("KV", H * D, (Skv + XR) * rs, rs, D)
            size["KV"] = B * (Skv + XR) * rs
        elif lay == "kvdiff":
            sep("K", Skv, D + 8, 16, 8)
            sep("V", Skv, D, 8, 0)
        elif lay == "gap":
            sep("K", Skv, D + 8, 8, 16)
            sep("V", Skv, D + 16, 0, 8)
        else:
            sep("K", Skv, D)
            sep("V", Skv, D)
    ors = H * D + (8 if lay == "opad" else 0)
    obs = Sq * ors + (16 if lay == "opad" else 0)
    return L, size, ors, obs


def plant_positions(Sq, Skv, causal):
    if causal:
        return list(range(Skv - Sq, Skv))
    edges = [0, 63, 64, 127, 128, (Skv // 64) * 64 - 1, Skv - 2, Skv - 1]
    cand = edges + [(37 * i) % Skv for i in range(Skv)] + list(range(Skv))
    seen, pos = set(), []
    for p in cand:
        if 0 <= p < Skv and p not in seen:
            seen.add(p)
            pos.append(p)
    return pos[:min(Sq, Skv)]


def attn_inputs(c, dev):
    """Logical Q [Bq, H, Sq, D] (Bq = 1 for the broadcast layout), K, V [B, H, Skv, D] in the operand type, the scale, the planted
    positions (or None)."""
    dtype = DTYPES[c["dt"]]
    g = gen_of(c["id"], dev)
    B, H, Sq, Skv, D = c["B"], c["H"], c["Sq"], c["Skv"], c["D"]
    Bq = 1 if c["layout"] == "qb0" else B
    scale = float(torch.tensor(c["scale_mul"] * D ** -0.5, dtype=F32))
    V = torch.randn(B, H, Skv, D, device=dev, generator=g).to(dtype)
    pos = None
    if c["data"] in ("plant", "randn"):
        Q = torch.randn(Bq, H, Sq, D, device=dev, generator=g).to(dtype)
        K = torch.randn(B, H, Skv, D, device=dev, generator=g).to(dtype)
        if c["data"] == "plant":
            pos = plant_positions(Sq, Skv, c["causal"])
            q = Q[:, :, :len(pos)].double()
            K[:, :, torch.tensor(pos, device=dev)] = (q * 8.0 / (scale * q.pow(2).sum(-1, keepdim=True))).to(dtype).expand(B, -1, -1, -1)
    else:
        # scores = a common part c_j (log2 units) + noise: Q = 4 u + noise orthogonal to u, K_j = b_j u + noise, |u| = 1
        tile = torch.arange(Skv, device=dev) // 64
        if c["data"] == "stair_up":      # + 6 per tile over 10 tiles, then - 40 over the last 2
            cj = torch.where(tile < 10, 6.0 * tile, 54.0 - 20.0 * (tile - 9))
        else:                            # the first tile 200 above everything behind it
            cj = torch.where(tile < 1, 200.0, 0.0)
        u = torch.full((D,), D ** -0.5, device=dev)
        qn = torch.randn(Bq, H, Sq, D, device=dev, generator=g)
        qn = qn - (qn @ u)[..., None] * u
        Q = (4.0 * u + qn).to(dtype)
        bj = cj / (4.0 * scale * 1.4426950408889634)
        K = (bj[:, None] * u + 0.5 * torch.randn(B, H, Skv, D, device=dev, generator=g)).to(dtype)
    return Q, K, V, scale, pos


def attn_launch(lib, c, Q, K, V, scale, dev, refused=False):
    """One launch into fresh NaN / guard buffers. Returns (logical output [B, H, Sq, D], guard buffer, inputs); `refused`: the call must
    return an error, and the status comes back in place of the output."""
    from seedx_amd import _lib
    dtype = DTYPES[c["dt"]]
    B, H, Sq, Skv, D = c["B"], c["H"], c["Sq"], c["Skv"], c["D"]
    L, size, ors, obs = attn_layout(c)
    bufs = {k: _nanbuf(n + 256, dtype, dev) for k, n in size.items()}
    for name, t in (("Q", Q), ("K", K), ("V", V)):
        key, off, bs, rs, hs = L[name]
        torch.as_strided(bufs[key], t.shape, (bs, hs, rs, 1), off).copy_(t)
    ob = GBuf(B * obs, dtype, dev)
    torch.as_strided(ob.allowed, (B, Sq, H * D), (obs, ors, 1), ob.before).fill_(True)
    a = _lib.AttnSmallArgs() if c["small"] else _lib.AttnArgs()
    for name in "QKV":
        key, off, bs, rs, hs = L[name]
        assert off % 8 == 0 and bs % 8 == 0 and rs % 8 == 0 and hs % 8 == 0
        setattr(a, name, bufs[key].data_ptr() + 2 * off)
        n = name.lower()
        setattr(a, n + "_batch_stride", bs), setattr(a, n + "_row_stride", rs), setattr(a, n + "_head_stride", hs)
    a.O, a.o_batch_stride, a.o_row_stride = ob.ptr(), obs, ors
    a.B, a.H, a.Sq, a.Skv, a.D = B, H, Sq, Skv, D
    a.scale, a.dtype = scale, sx_code(dtype)
    if c["small"]:
        st = lib.sx_attention_small(C.byref(a), stream())
    else:
        a.causal = int(c["causal"])
        st = lib.sx_attention(C.byref(a), stream())
    torch.cuda.synchronize()
    if refused:
        return st, ob, bufs
    _lib.check(st, f"attention case {c['id']}")
    out = torch.as_strided(ob.buf, (B, H, Sq, D), (obs, D, ors, 1), ob.before)
    return out, ob, bufs


def attn_reference(c, Q, K, V, scale, pos):
    """fp64 reference, A_d, and S1 = max scale sum_d |q k| (for the small kernel's bound)."""
    q, k, v = Q.double(), K.double(), V.double()
    s = scale * (q @ k.transpose(-1, -2))
    Sq, Skv = c["Sq"], c["Skv"]
    if c["causal"]:
        i, j = torch.arange(Sq, device=s.device)[:, None], torch.arange(Skv, device=s.device)[None, :]
        s = s.masked_fill(j > i + (Skv - Sq), float("-inf"))
    p = torch.softmax(s, -1)
    if pos is not None and c["D"] >= 40:
        n = len(pos)
        w = p[:, :, torch.arange(n, device=s.device), torch.tensor(pos, device=s.device)]
        assert float(w.min()) >= 0.25, f"{c['id']}: a planted key weighs only {float(w.min()):.3f} in its row"
    s1 = float((scale * (q.abs() @ k.abs().transpose(-1, -2))).max())
    return p @ v, p @ v.abs(), s1


def attn_bound(c, ref, A, s1):
    dtype = DTYPES[c["dt"]]
    if c["small"]:
        c32 = 2.0 * (C_ACC * math.sqrt(c["D"]) * max(s1, 1.0) + 3.0) + 2.0 * C_ACC * math.sqrt(c["Skv"]) + 4.0
        return rnd(ref, dtype) + c32 * U32 * A
    return rnd(ref, dtype) + 2.0 * U_OUT[dtype] * A + C32_ATTN * U32 * A


def run_attn(c, dev):
    from seedx_amd import _lib
    lib = _lib.load()
    dtype = DTYPES[c["dt"]]
    Q, K, V, scale, pos = attn_inputs(c, dev)
    ref, A, s1 = attn_reference(c, Q, K, V, scale, pos)
    out, ob, _keep = attn_launch(lib, c, Q, K, V, scale, dev)
    ob.check(c["id"] + " (O)")
    assert bool(torch.isfinite(out.float()).all()), f"{c['id']}: non-finite output: an unwritten element or a read outside an operand"
    got = out.double()
    key = kernel_of_attn(c) + (c["dt"],)
    worst = held(key, got, ref, attn_bound(c, ref, A, s1), c["id"])
    rel = (got - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-30)
    assert float(rel.max()) < 2 * TOL[dtype], f"{c['id']}: a row's rel-L2 {float(rel.max()):.3e} >= {2 * TOL[dtype]}"
    out2, ob2, _keep2 = attn_launch(lib, c, Q, K, V, scale, dev)
    ob2.check(c["id"] + " (O, second launch)")
    assert same_bits(out2, out), f"{c['id']}: two identical launches differ"
    print(f"{c['id']}: {key} worst |diff| / bound {worst:.3f}, worst row rel-L2 {float(rel.max()):.2e}")


@pytest.mark.parametrize("c", [c for c in ATTN if not c["small"]], ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_attention_vs_fp64(dev, c):
    run_attn(c, dev)


@pytest.mark.parametrize("c", [c for c in ATTN if c["small"]], ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_attention_small_vs_fp64(dev, c):
    run_attn(c, dev)


@stops_on_gpu_fault
def test_attention_small_refuses_what_it_cannot_hold(dev):
    """Skv = 1537 (> the 1536 scores of a wave's LDS row) and D = 264 (> 256) are refused before any launch: the output keeps its guard bits."""
    from seedx_amd import _lib
    lib = _lib.load()
    for kw in (dict(Skv=1537, D=64), dict(Skv=64, D=264)):
        c = acase("small-refused", "f16", small=True, B=1, H=1, Sq=2, **kw)
        Q, K, V, scale, _ = attn_inputs(c, dev)
        st, ob, _keep = attn_launch(lib, c, Q, K, V, scale, dev, refused=True)
        assert st != 0, f"sx_attention_small took {kw}"
        ob.allowed[:] = False
        ob.check(f"refused {kw}")


# ----------------------------------------------------------------------------------------------------------------------------
# 3. LayerNorm / RMSNorm
# ----------------------------------------------------------------------------------------------------------------------------
LN_NV = (3, 5, 8, 16, 24)
LN_MODES = ("ln", "ln_nobeta", "rms")
LN_WAVE_SHAPES = [(r, cols) for r in (33, 37) for cols in (4, 768, 772, 1280, 1284, 2048, 2052, 4096, 4100, 6144)]
LN_BLOCK_SHAPES = [(r, cols) for r in (1, 16, 17, 32) for cols in (4, 32, 1024, 1028, 5120, 6144)]
LN_TILED_SHAPES = [(r, cols) for r in (1, 15, 16, 17, 32) for cols in (32, 5120)]


def ln_cases():
    out = []
    for rows, cols in LN_WAVE_SHAPES + LN_BLOCK_SHAPES:
        for i_dt in ALL_DT:
            for o_dt in ALL_DT:
                for mode in LN_MODES:
                    out.append(dict(id=f"ln-{rows}x{cols}-{i_dt}-{o_dt}-{mode}", rows=rows, cols=cols, i=i_dt, o=o_dt, mode=mode, tiled=False))
    for rows, cols in LN_TILED_SHAPES:
        for o_dt in DTYPES:
            for k, i_dt in enumerate(ALL_DT):
                out.append(dict(id=f"ln-tiled-{rows}x{cols}-{i_dt}-{o_dt}", rows=rows, cols=cols, i=i_dt, o=o_dt, mode=LN_MODES[k], tiled=True))
    return out


def kernel_of_ln(c):
    """sx_layernorm: rows <= 32 -> layernorm_block_kernel<DT>; else layernorm_kernel<DT, NV> with the smallest NV of (3, 5, 8, 16, 24)
    that holds cols / 4 quads in 64 lanes."""
    dt = "SX_" + c["i"].upper()
    if c["rows"] <= 32:
        return ("layernorm_block_kernel", dt)
    n4 = c["cols"] // 4
    return ("layernorm_kernel", dt, next(nv for nv in LN_NV if n4 <= 64 * nv))


LN = ln_cases()


def ln_rows(rows, cols, in_dt, g, dev):
    """Row r is of kind r % 4: 0 exact zero mean on a grid (see the docstring), 1 mean / std = 1, 2 mean / std = 1000 (16-bit input: 30),
    3 as 1 with another scale; the last row of a matrix of >= 5 rows is zero."""
    grid = 2.0 ** -4 if in_dt == BF16 else 2.0 ** -8
    x = torch.randn(rows, cols, device=dev, generator=g)
    half = (x[:, :cols // 2].clamp(-7.9, 7.9) / grid).round() * grid
    perm = torch.randperm(cols, device=dev, generator=g)
    zero_mean = torch.cat([half, -half], 1)[:, perm]
    kind = torch.arange(rows, device=dev)[:, None] % 4
    big = 1000.0 if in_dt == F32 else 30.0
    x = torch.where(kind == 0, zero_mean, torch.where(kind == 1, x + 1.0, torch.where(kind == 2, x + big, 3.0 * x - 3.0)))
    if rows >= 5:
        x[-1] = 0.0
    return x.to(in_dt)


def ln_launch(lib, c, x, gamma, beta, eps, dev):
    from seedx_amd import _lib
    rows, cols, o_dt = c["rows"], c["cols"], ALL_DT[c["o"]]
    xb, gb = nan_lead(x), nan_lead(gamma, 64)
    bb = nan_lead(beta, 64) if beta is not None else None
    if c["tiled"]:
        yb = TiledOut(1, rows, cols, o_dt, dev)
    else:
        yb = GBuf(rows * cols, o_dt, dev)
        yb.allow()[:] = True
    st = lib.sx_layernorm(xb.data_ptr(), sx_code(x.dtype), yb.ptr(), sx_code(o_dt) | (_lib.SX_TILED16 if c["tiled"] else 0), gb.data_ptr(),
                          bb.data_ptr() if bb is not None else None, rows, cols, eps, int(c["mode"] == "rms"), stream())
    _lib.check(st, c["id"])
    torch.cuda.synchronize()
    y = yb.planes()[0] if c["tiled"] else yb.body.view(rows, cols)
    return y, yb, (xb, gb, bb)


def ln_reference(c, x, gamma, beta, eps):
    cols = c["cols"]
    lanes = 256 if c["rows"] <= 32 else 64
    n = -(-(cols // 4) // lanes) + 11
    Cc = 2.0 * n + 10.0
    x64, g64 = x.double(), gamma.double()
    if c["mode"] == "rms":
        mean = torch.zeros(x.shape[0], 1, dtype=torch.float64, device=x.device)
    else:
        mean = x64.mean(1, keepdim=True)
    d = x64 - mean
    rstd = 1.0 / torch.sqrt(d.pow(2).mean(1, keepdim=True) + eps)
    ref = d * rstd * g64
    err = Cc * U32 * (d.abs() + mean.abs()) * rstd * g64.abs()
    if beta is not None:
        ref = ref + beta.double()
        err = err + U32 * beta.double().abs()
    return ref, err


def run_ln(c, dev):
    from seedx_amd import _lib
    lib = _lib.load()
    i_dt, o_dt = ALL_DT[c["i"]], ALL_DT[c["o"]]
    g = gen_of(f"ln-{c['rows']}x{c['cols']}-{c['i']}", dev)
    x = ln_rows(c["rows"], c["cols"], i_dt, g, dev)
    gamma = (1.0 + 0.3 * torch.randn(c["cols"], device=dev, generator=g))
    beta = 0.5 * torch.randn(c["cols"], device=dev, generator=g) if c["mode"] == "ln" else None
    eps = 1e-6
    ref, err = ln_reference(c, x, gamma, beta, eps)
    y, yb, _keep = ln_launch(lib, c, x, gamma, beta, eps, dev)
    yb.check(c["id"])
    assert bool(torch.isfinite(y.float()).all()), f"{c['id']}: non-finite output"
    worst = held(kernel_of_ln(c) + (c["o"],), y.double(), ref, err + rnd(ref, o_dt), c["id"])
    if c["rows"] >= 5 and c["mode"] != "rms":
        want = torch.zeros(c["cols"], device=dev) if beta is None else beta
        assert torch.equal(y[-1].float(), want.to(o_dt).float()), f"{c['id']}: a zero row must give beta"
    y2, yb2, _keep2 = ln_launch(lib, c, x, gamma, beta, eps, dev)
    yb2.check(c["id"] + " (second launch)")
    assert same_bits(y2, y), f"{c['id']}: two identical launches differ"
    return worst


@pytest.mark.parametrize("shape", LN_WAVE_SHAPES + LN_BLOCK_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@stops_on_gpu_fault
def test_layernorm_vs_fp64(dev, shape):
    """Every input type x output type x {LayerNorm with beta, without beta, RMSNorm} at one shape."""
    worst = max(run_ln(c, dev) for c in LN if (c["rows"], c["cols"]) == shape and not c["tiled"])
    print(f"layernorm {shape}: worst |diff| / bound {worst:.3f}")


@pytest.mark.parametrize("shape", LN_TILED_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@stops_on_gpu_fault
def test_layernorm_tiled16_vs_fp64(dev, shape):
    """SX_TILED16 output of the block kernel: rows >= M of each 16-row block keep their guard bits, the tiles hold the fp64 values."""
    worst = max(run_ln(c, dev) for c in LN if (c["rows"], c["cols"]) == shape and c["tiled"])
    print(f"layernorm tiled {shape}: worst |diff| / bound {worst:.3f}")


@stops_on_gpu_fault
def test_layernorm_refusals(dev):
    from seedx_amd import _lib
    lib = _lib.load()
    T = _lib.SX_TILED16
    for rows, cols, o_code in ((4, 6148, 0), (40, 6148, 0), (4, 30, 0), (40, 1026, 1), (33, 64, T | 0), (16, 64, T | 2), (16, 48, T | 1)):
        x = torch.randn(rows, cols, device=dev)
        gamma = torch.ones(cols + 4, device=dev)
        yb = GBuf(rows * cols * 2, F16, dev)
        st = lib.sx_layernorm(x.data_ptr(), 2, yb.ptr(), o_code, gamma.data_ptr(), None, rows, cols, 1e-6, 0, stream())
        torch.cuda.synchronize()
        assert st != 0, (rows, cols, o_code)
        yb.check(f"refused layernorm {(rows, cols, o_code)}")


# ----------------------------------------------------------------------------------------------------------------------------
# 4. GroupNorm
# ----------------------------------------------------------------------------------------------------------------------------
GN_MAX_C = 3072


def gcase(cid, **kw):
    c = dict(B=2, HW=12, C=320, C1=0, groups=32, out="f16", raw=True, silu=True, tune=0, data="randn")
    c.update(kw)
    c["id"] = f"gn-{cid}-B{c['B']}-HW{c['HW']}-C{c['C']}{'=' + str(c['C1']) + '+' + str(c['C'] - c['C1']) if c['C1'] else ''}-g{c['groups']}-{c['out']}" \
              f"{'-raw' if c['raw'] else ''}{'-silu' if c['silu'] else ''}{'-tune' + str(c['tune']) if c['tune'] else ''}"
    return c


def gn_threads(C_):
    """Threads of gn_stats_kernel: T = 320 / 160 where the C / 4 quads tile them evenly, 128 up to 128 quads, else 256."""
    nq = C_ // 4
    return 320 if nq % 320 == 0 else (160 if nq % 160 == 0 else (128 if nq <= 128 else 256))


def gn_slots(C_):
    return -(-(C_ // 4) // gn_threads(C_))


def gn_rows(c):
    """(rows_per_block of gn_apply_kernel, rows_stats of gn_stats_kernel), as groupnorm_impl sizes them."""
    B, HW, C_ = c["B"], c["HW"], c["C"]
    rpb = max(4, -(-(HW * B) // 2048))
    nblk = c["tune"] or min(2048, max(512, (B * HW * C_ * 4) >> 18))
    return rpb, max(8, -(-(HW * B) // nblk))


def gn_apply_rounds(c):
    """Rounds of gn_apply_kernel's 4-in-flight main loop of thread 0 in a full block."""
    total = min(c["HW"], gn_rows(c)[0]) * (c["C"] // 4)
    return len(range(0, max(total - 768, 0), 1024))


def kernel_of_gn(c):
    return ("gn_stats_kernel", bool(c["C1"])), ("gn_apply_kernel", bool(c["C1"]))


def gn_cases():
    out = []
    outs = ("f16", "bf16", "f32", "bf16x3", "f16x2")
    for i, C_ in enumerate((64, 320, 512, 640, 960, 1024, 1280, 1536, 1920, 2560, 3072)):
        o = outs[i % 5]
        out.append(gcase("C", C=C_, out=o, raw=o != "f32", silu=i % 2 == 0))
    out.append(gcase("groups", C=128, groups=64, out="bf16", silu=False))
    out.append(gcase("groups", C=64, groups=1, out="f32", raw=False))
    for i, HW in enumerate((1, 3, 7, 8, 37, 100)):
        o = outs[i % 5]
        out.append(gcase("HW", HW=HW, out=o, raw=o != "f32", silu=i % 2 == 1))
    out.append(gcase("long", HW=4200, C=64, out="f16"))
    out.append(gcase("long", HW=4200, C=64, out="f32", raw=False, tune=64))
    # at C = 64 a block of 5 rows holds 80 quads: the apply kernel's 4-in-flight loop needs > 768. 5 rows of 768 quads walk it 3 times
    out.append(gcase("long", HW=4200, C=3072, out="f16", raw=False))
    for o in outs:
        for silu in (True, False):
            for raw in ((False,) if o == "f32" else (True, False)):
                out.append(gcase("fmt", HW=37, C=320, out=o, raw=raw, silu=silu))
    for i, (C1, C2) in enumerate(((640, 320), (320, 640), (4, 60), (1280, 1280))):
        o = outs[i % 5]
        out.append(gcase("two", C=C1 + C2, C1=C1, HW=37, out=o, raw=o != "f32", silu=i % 2 == 0))
    return out


GN = gn_cases()
GN_COND = (0.0, 1.0, 30.0, 100.0)


def gn_inputs(c, dev):
    g = gen_of(c["id"], dev)
    B, HW, C_, G = c["B"], c["HW"], c["C"], c["groups"]
    cpg = C_ // G
    x = torch.randn(B, HW, C_, device=dev, generator=g)
    if c["data"] == "randn":
        x = x + 0.2 * torch.randn(B, 1, C_, device=dev, generator=g)
    elif c["data"] == "cond":            # group g: mean / std = GN_COND[g % 4]
        x = x + torch.tensor(GN_COND, device=dev)[(torch.arange(C_, device=dev) // cpg) % 4]
    elif c["data"] == "grid":            # multiples of 2^-5 below 4: every fp32 sum of the statistics is exact
        x = (x.clamp(-3.9, 3.9) * 32).round() / 32
    sign = lambda t: torch.where(t < 0.5, -1.0, 1.0)
    gamma = (0.5 + torch.rand(C_, device=dev, generator=g)) * sign(torch.rand(C_, device=dev, generator=g))
    beta = (0.5 + torch.rand(C_, device=dev, generator=g)) * sign(torch.rand(C_, device=dev, generator=g))
    return x, gamma, beta


def gn_out_type(o):
    return {"f16": (F16, 1), "bf16": (BF16, 1), "f32": (F32, 1), "bf16x3": (BF16, 3), "f16x2": (F16, 2)}[o]


def gn_code(o):
    return {"f16": 0, "bf16": 1, "f32": 2, "bf16x3": 3, "f16x2": 4}[o]


def gn_recombine(t, o, C_):
    """fp64 [.., C] from the stored planes: [hi | hi | lo] (the two hi copies must agree), [hi | lo], or the plain tensor."""
    t = t.double()
    if o == "bf16x3":
        assert torch.equal(t[..., :C_], t[..., C_:2 * C_]), "the two hi planes of SX_BF16X3 differ"
        return t[..., :C_] + t[..., 2 * C_:]
    if o == "f16x2":
        return t[..., :C_] + t[..., C_:]
    return t


def gn_launch(lib, c, x, gamma, beta, dev, eps=1e-5, phase=0, stats=None, hw_total=None):
    """One sx_groupnorm2 (phase 0) or sx_groupnorm_sp (phase 1 / 2) launch; x is [B, HW, C] (split at C1 into two allocations)."""
    from seedx_amd import _lib
    B, HW, C_, G, C1 = x.shape[0], x.shape[1], c["C"], c["groups"], c["C1"]
    odt, planes = gn_out_type(c["out"])
    if C1:
        xb, x2b = nan_lead(x[..., :C1].contiguous()), nan_lead(x[..., C1:].contiguous())
    else:
        xb, x2b = nan_lead(x), None
    gb, bb = nan_lead(gamma, 64), nan_lead(beta, 64)
    sb = torch.full((2 * B * G + 16,), -7.5, dtype=torch.float64, device=dev)
    if stats is not None:
        sb[:2 * B * G] = stats
    yb = GBuf(B * HW * C_ * planes, odt, dev)
    yb.allow()[:] = True
    rb = None
    if c["raw"]:
        rb = GBuf(B * HW * C_ * planes, odt, dev)
        rb.allow()[:] = True
    x2p = x2b.data_ptr() if x2b is not None else None
    rp = rb.ptr() if rb is not None else None
    try:
        if c["tune"]:
            assert lib.sx_norm_tune(0, c["tune"]) == 0
        if phase == 0:
            st = lib.sx_groupnorm2(xb.data_ptr(), x2p, C1, yb.ptr(), rp, gn_code(c["out"]), gb.data_ptr(), bb.data_ptr(), sb.data_ptr(), B, HW, C_, G,
                                   eps, int(c["silu"]), stream())
        else:
            st = lib.sx_groupnorm_sp(xb.data_ptr(), x2p, C1, yb.ptr(), rp, gn_code(c["out"]), gb.data_ptr(), bb.data_ptr(), sb.data_ptr(), B, HW,
                                     hw_total, C_, G, eps, int(c["silu"]), phase, stream())
    finally:
        lib.sx_norm_tune(0, 0)
    _lib.check(st, c["id"])
    torch.cuda.synchronize()
    assert bool((sb[2 * B * G:] == -7.5).all()), f"{c['id']}: written behind the 2 * B * groups statistics"
    if phase == 1:
        for gbuf in (yb, rb):
            if gbuf is not None:
                gbuf.allowed[:] = False
    yb.check(c["id"] + " (y)")
    if rb is not None:
        rb.check(c["id"] + " (raw)")
    y = yb.body.view(B, HW, C_ * planes)
    raw = rb.body.view(B, HW, C_ * planes) if rb is not None else None
    return y, raw, sb[:2 * B * G].clone(), (xb, x2b, gb, bb)


def gn_reference(c, x, gamma, beta, eps=1e-5):
    """fp64 reference [B, HW, C], the bound without the output rounding, and |mean| rstd |gamma| per element (the magnitude of the apply
    kernel's shift, which the bound's formula does not carry)."""
    B, HW, C_, G = x.shape[0], x.shape[1], c["C"], c["groups"]
    cpg = C_ // G
    xg = x.double().view(B, HW, G, cpg)
    mean = xg.mean((1, 3), keepdim=True)
    var = (xg - mean).pow(2).mean((1, 3), keepdim=True)
    xhat = ((xg - mean) / torch.sqrt(var + eps)).view(B, HW, C_)
    kappa = ((mean.pow(2) + var) / var).expand(B, HW, G, cpg).reshape(B, HW, C_)
    n_acc = 2 * gn_rows(c)[1] + cpg // 2 + 2
    xg_ = (xhat * gamma.double()).abs()
    pre = xhat * gamma.double() + beta.double()
    shift = (mean.abs() / torch.sqrt(var + eps)).expand(B, HW, G, cpg).reshape(B, HW, C_) * gamma.double().abs()
    err = C_GN * U32 * (xg_ + beta.double().abs()) + CV_GN * n_acc * U32 * kappa * xg_ / 2
    if c["silu"]:
        return pre * torch.sigmoid(pre), LIP["silu"] * err + C_EP * U32 * pre.abs(), shift
    return pre, err, shift


def gn_check(c, x, y, raw, ref, err, what):
    """The output (planes recombined and held to the fp32-output bound) and the raw copy."""
    C_ = c["C"]
    odt, planes = gn_out_type(c["out"])
    assert bool(torch.isfinite(y.float()).all()), f"{what}: non-finite output"
    got = gn_recombine(y, c["out"], C_)
    rdt = F32 if planes > 1 else odt
    # two planes hold the value to 2^-16 (bf16 hi + lo) / 2^-21 (fp16 hi + lo) relative: the rounding of the lo plane (fp16: or half a unit of
    # the smallest subnormal, 2^-25, where the lo plane falls below the smallest normal)
    extra = {"bf16x3": 2.0 ** -16, "f16x2": 2.0 ** -21}.get(c["out"], 0.0) * ref.abs() + (2.0 ** -25 if c["out"] == "f16x2" else 0.0)
    worst = 0.0
    for k in kernel_of_gn(c):
        worst = held(k + (c["out"],), got, ref, err + rnd(ref, rdt) + extra, what)
    if planes == 1:
        rel = float((got - ref).norm() / ref.norm())
        assert rel < TOL[odt], f"{what}: rel-L2 {rel:.3e} >= {TOL[odt]}"
    if raw is not None:
        assert bool(torch.isfinite(raw.float()).all()), f"{what}: non-finite raw copy"
        r64, x64 = gn_recombine(raw, c["out"], C_), x.double()
        if planes == 1:
            assert same_bits(raw, x.to(odt)), f"{what}: the raw copy is not x rounded to the output type"
        else:
            lim = {"bf16x3": 2.0 ** -16, "f16x2": 2.0 ** -21}[c["out"]] * x64.abs() + (2.0 ** -25 if c["out"] == "f16x2" else 0.0)
            assert bool(((r64 - x64).abs() <= lim).all()), f"{what}: the raw planes do not recombine to x"
    return worst


def run_gn(c, dev):
    from seedx_amd import _lib
    lib = _lib.load()
    x, gamma, beta = gn_inputs(c, dev)
    ref, err, _ = gn_reference(c, x, gamma, beta)
    y, raw, stats, _keep = gn_launch(lib, c, x, gamma, beta, dev)
    worst = gn_check(c, x, y, raw, ref, err, c["id"])
    y2, raw2, stats2, _keep2 = gn_launch(lib, c, x, gamma, beta, dev)
    assert same_bits(stats2, stats), f"{c['id']}: the statistics of two identical launches differ (the fp64 atomics are not order-independent)"
    assert same_bits(y2, y) and (raw is None or same_bits(raw2, raw)), f"{c['id']}: two identical launches differ"
    print(f"{c['id']}: T {gn_threads(c['C'])} x {gn_slots(c['C'])} slots, rows {gn_rows(c)}, worst |diff| / bound {worst:.3f}")
    return worst


@pytest.mark.parametrize("c", GN, ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_groupnorm_vs_fp64(dev, c):
    run_gn(c, dev)


@pytest.mark.parametrize("out", ("f16", "f32"))
@stops_on_gpu_fault
def test_groupnorm_sp_split_rows(dev, out):
    """The rows of every image split 37 | 63: phase 1 on each part, the statistics added on the host in fp64, phase 2 on each part with
    hw_total = 100. The stacked outputs equal the single launch bit for bit and meet the fp64 bound. The data sit on a grid on which every
    fp32 partial sum of the statistics is exact (multiples of 2^-5 below 4: a block adds at most 8 rows x 10 channels), so the sums
    do not depend on where the blocks' row ranges start, which differs between the split and the single launch."""
    from seedx_amd import _lib
    lib = _lib.load()
    c = gcase("sp", HW=100, C=320, out=out, raw=False, silu=True, data="grid")
    x, gamma, beta = gn_inputs(c, dev)
    ref, err, _ = gn_reference(c, x, gamma, beta)
    y, _, stats, _k = gn_launch(lib, c, x, gamma, beta, dev)
    gn_check(c, x, y, None, ref, err, c["id"])
    parts = (x[:, :37].contiguous(), x[:, 37:].contiguous())
    st = [gn_launch(lib, c, p, gamma, beta, dev, phase=1, hw_total=100)[2] for p in parts]
    total = st[0] + st[1]
    assert same_bits(total, stats), "the statistics of the two parts do not add up to those of the single launch"
    ys = [gn_launch(lib, c, p, gamma, beta, dev, phase=2, stats=total, hw_total=100)[0] for p in parts]
    assert same_bits(torch.cat(ys, 1), y), "phase 1 + phase 2 over split rows differ from the single launch"


@pytest.mark.parametrize("out", ("f16", "bf16", "f32"))
@stops_on_gpu_fault
def test_groupnorm_conditioning(dev, out):
    """Groups with mean / std = 0, 1, 30, 100 in one launch (C = 320, HW = 100; the variance is E[x^2] - mean^2 from fp32 partial sums of
    8 rows, met in fp64). Measured on the MI355X (profiles/attn_norm_matrix.md): the 16-bit outputs meet the derived bound at all four
    ratios (worst |diff| / bound 0.99 / 0.99 / 0.93 / 0.89) and stay inside the plain output-rounding TOL at all four: the relative L2
    error of the fp16 output is 2.06e-4 at 0, 1 and 30 and 2.31e-4 at 100 (TOL 6e-4), of the bf16 output 1.7e-3 throughout (TOL 4e-3);
    100 is the largest ratio measured, so the kernel is usable for 16-bit outputs at least up to there and needs no shifted sum.
    The fp32 output meets the bound up to mean / std = 1 (0.11, 0.22) and exceeds the FORMULA at 30 and 100 (1.2, 1.7 bounds) at
    elements with x^ ~ 0: the formula has no term for the 2^-24 |mean| rstd |gamma| of the four roundings of the apply kernel's shift
    (float(mean), mean * scale, beta - that, x * scale). With 4 * 2^-24 |mean| rstd |gamma| added the fp32 output is inside at all four,
    which is asserted; without it the figure is printed. Its relative L2 error is 3.8e-8, 5.8e-8, 8.1e-6 and 9.0e-5: an fp32-grade
    consumer (TOL 2e-5) is served up to mean / std = 30, not at 100."""
    from seedx_amd import _lib
    lib = _lib.load()
    c = gcase("cond", HW=100, C=320, out=out, raw=False, silu=False, data="cond")
    x, gamma, beta = gn_inputs(c, dev)
    ref, err, shift = gn_reference(c, x, gamma, beta)
    y, _, _, _k = gn_launch(lib, c, x, gamma, beta, dev)
    odt = ALL_DT[out]
    got = y.double()
    assert bool(torch.isfinite(got).all())
    bound = err + rnd(ref, odt)
    cls = ((torch.arange(320, device=dev) // 10) % 4)
    for k, ratio in enumerate(GN_COND):
        sel = cls == k
        g_, r_ = got[..., sel], ref[..., sel]
        w = float(((g_ - r_).abs() / bound[..., sel]).max())
        rel = float((g_ - r_).norm() / r_.norm())
        NOTES[f"groupnorm conditioning {out:5s} mean/std {ratio:5.0f}"] = f"worst |diff| / bound {w:.3f}   rel-L2 {rel:.3e}   TOL {TOL[odt]} {'held' if rel < TOL[odt] else 'NOT held'}"
        print(f"conditioning {out} mean/std {ratio}: worst |diff| / bound {w:.3f}, rel-L2 {rel:.3e} (TOL {TOL[odt]})")
        if out != "f32" or ratio <= 1.0:
            assert w <= 1.0, f"mean / std = {ratio}: {w:.2f} bounds"
            key = ("gn_cond", f"mean/std={ratio:.0f}", out)
            WORST[key] = max(WORST.get(key, 0.0), w)
        else:
            w4 = float(((g_ - r_).abs() / (bound + 4.0 * U32 * shift)[..., sel]).max())
            NOTES[f"groupnorm conditioning {out:5s} mean/std {ratio:5.0f} with the shift term"] = f"worst |diff| / bound {w4:.3f}"
            assert w4 <= 1.0, f"mean / std = {ratio}: {w4:.2f} bounds with the shift term"
        if out != "f32" and ratio <= 30.0:
            assert rel < TOL[odt], f"mean / std = {ratio}: rel-L2 {rel:.3e} >= {TOL[odt]}"


# ----------------------------------------------------------------------------------------------------------------------------
# 5. row softmax
# ----------------------------------------------------------------------------------------------------------------------------
SM_SHAPES = ((1, 4), (3, 260), (5, 1024), (2, 1028), (2, 4100), (1, 16384))
SM_DATA = ("randn", "const", "spike", "span")
SM = [dict(id=f"sm-{r}x{cols}-{o}-{d}", rows=r, cols=cols, o=o, data=d) for r, cols in SM_SHAPES for o in ALL_DT for d in SM_DATA]


def kernel_of_sm(c):
    """sx_softmax_rows: softmax_rows_kernel<BF16, true> for an fp32 output, else <BF16> / <F16>."""
    return ("softmax_rows_kernel", "BF16, true" if c["o"] == "f32" else c["o"].upper())


def sm_launch(lib, c, x, scale, dev):
    from seedx_amd import _lib
    rows, cols, odt = c["rows"], c["cols"], ALL_DT[c["o"]]
    ldx, ldy = cols + 8, cols + 4
    xb = _nanbuf(rows * ldx + 256, F32, dev)
    xb[:rows * ldx].view(rows, ldx)[:, :cols] = x
    yb = GBuf(rows * ldy, odt, dev)
    yb.allow().view(rows, ldy)[:, :cols] = True
    st = lib.sx_softmax_rows(xb.data_ptr(), ldx, yb.ptr(), ldy, rows, cols, scale, sx_code(odt), stream())
    _lib.check(st, c["id"])
    torch.cuda.synchronize()
    return yb.body.view(rows, ldy)[:, :cols], yb, xb


def run_sm(c, dev):
    from seedx_amd import _lib
    lib = _lib.load()
    rows, cols, odt = c["rows"], c["cols"], ALL_DT[c["o"]]
    g = gen_of(c["id"], dev)
    scale = float(torch.tensor(0.37, dtype=F32))
    x = torch.randn(rows, cols, device=dev, generator=g) * 3.0
    if c["data"] == "const":
        x = torch.full((rows, cols), 1.7, device=dev)
    elif c["data"] == "spike":           # one entry 200 above the rest (after the scaling): everything else underflows
        x[torch.arange(rows, device=dev), torch.randint(cols, (rows,), device=dev, generator=g)] += 200.0 / scale
    elif c["data"] == "span":            # scale * x over [-300, 300]
        x = (torch.rand(rows, cols, device=dev, generator=g) * 600.0 - 300.0) / scale
        x[:, 0], x[:, -1] = -300.0 / scale, 300.0 / scale
    z = scale * x.double()
    ref = torch.softmax(z, 1)
    Cc = 4.0 * -(-cols // 1024) + 20.0
    bound = rnd(ref, odt) + Cc * U32 * (1.0 + z.abs().max(1, keepdim=True)[0] * 1.4426950408889634) * ref
    y, yb, _keep = sm_launch(lib, c, x, scale, dev)
    yb.check(c["id"])
    assert bool(torch.isfinite(y.float()).all()), f"{c['id']}: non-finite output"
    worst = held(kernel_of_sm(c) + (c["o"],), y.double(), ref, bound, c["id"])
    sums = y.double().sum(1)
    lim = cols * U_OUT[odt] / 2 + 1e-6
    assert float((sums - 1.0).abs().max()) <= lim, f"{c['id']}: a row sums to {float(sums[(sums - 1.0).abs().argmax()])!r}, off by more than {lim:.2e}"
    y2, yb2, _keep2 = sm_launch(lib, c, x, scale, dev)
    yb2.check(c["id"] + " (second launch)")
    assert same_bits(y2.contiguous(), y.contiguous()), f"{c['id']}: two identical launches differ"
    return worst


@pytest.mark.parametrize("shape", SM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@stops_on_gpu_fault
def test_softmax_rows_vs_fp64(dev, shape):
    """Every output type and row content at one shape, ldx = cols + 8 and ldy = cols + 4 (floats for the fp32 output)."""
    worst = max(run_sm(c, dev) for c in SM if (c["rows"], c["cols"]) == shape)
    print(f"softmax_rows {shape}: worst |diff| / bound {worst:.3f}")


@stops_on_gpu_fault
def test_softmax_rows_refusals(dev):
    from seedx_amd import _lib
    lib = _lib.load()
    x = torch.randn(4, 64, device=dev)
    for cols, scale in ((64, 0.0), (64, -1.0), (62, 1.0)):
        yb = GBuf(4 * 64, F16, dev)
        assert lib.sx_softmax_rows(x.data_ptr(), 64, yb.ptr(), 64, 4, cols, scale, 0, stream()) != 0, (cols, scale)
        torch.cuda.synchronize()
        yb.check(f"refused softmax_rows {(cols, scale)}")


# ----------------------------------------------------------------------------------------------------------------------------
# the sources, for tests/test_cpu_suite.py
# ----------------------------------------------------------------------------------------------------------------------------
def source_kernels():
    """Every instantiation that the host code of norm.hip / attn.hip launches, as the keys of kernel_of_*: a set per kernel family."""
    norm, attn = open(NORM_HIP).read(), open(ATTN_HIP).read()
    host = norm[norm.index('extern "C" int sx_layernorm('):]
    nvs = [int(v) for v in re.findall(r"SX_LN_GO\(DT, (\d+)\)", host)]
    dts = re.findall(r"SX_LN_NV\((SX_\w+)\) break;", host)
    assert host.count("layernorm_kernel<") == 1 and "(layernorm_kernel<DT, NV>)" in host
    src = dict(
        ln_wave={("layernorm_kernel", d, nv) for d in dts for nv in nvs},
        ln_block={("layernorm_block_kernel", d) for d in re.findall(r"layernorm_block_kernel<(SX_\w+)>", host)},
        gn_stats={("gn_stats_kernel", t == "true") for t in re.findall(r"gn_stats_kernel<(true|false)>", host)},
        gn_apply={("gn_apply_kernel", t == "true") for t in re.findall(r"gn_apply_kernel<(true|false)>", host)},
        softmax={("softmax_rows_kernel", t) for t in re.findall(r"softmax_rows_kernel<([^>]+)>", host)},
    )
    assert len(nvs) == len(set(nvs)) and len(dts) == len(set(dts))
    assert host.count("layernorm_block_kernel<") == len(src["ln_block"]) and host.count("softmax_rows_kernel<") == len(src["softmax"])
    assert "const int T = (nq % 320 == 0) ? 320 : ((nq % 160 == 0) ? 160 : ((nq <= 128) ? 128 : 256));" in host, "gn_threads restates this line"
    assert "if (rows <= 32) {" in host and "const int dp = a->D <= 64 ? 64 : 128;" in attn, "kernel_of_ln / kernel_of_attn restate these lines"
    ahost = attn[attn.index('extern "C" int sx_attention('):]
    src["attn"] = {("attn_kernel", t, int(dp)) for t, dp in re.findall(r"attn_kernel<(BF16|F16), (\d+)>", ahost)}
    src["attn_small"] = {("attn_small_kernel", t) for t in re.findall(r"attn_small_kernel<(BF16|F16)>", ahost)}
    assert ahost.count("attn_kernel<") == len(src["attn"]) and ahost.count("attn_small_kernel<") == len(src["attn_small"])
    return src


def test_print_worst_ratio_per_instantiation(dev):
    """Not a check of its own: the worst |diff| / bound of the cases above per instantiation and output / operand type (run the file as a
    whole), and the figures of the GroupNorm conditioning case. A 16-bit output sits just below 1 by construction (one correct rounding,
    among thousands of elements one is close to a tie); the fp32 outputs and the attention rows measure the derived constants."""
    for key, w in sorted(WORST.items(), key=lambda kv: str(kv[0])):
        print(f"worst |diff| / bound  {str(key):60s} {w:.3f}")
    for k in sorted(NOTES):
        print(f"{k}: {NOTES[k]}")
    assert all(w <= 1.0 for w in WORST.values())
