"""csrc/precise.hip against fp64, element by element: sx_attention_f32 (every VALU / key-split / verify / MFMA instantiation and the
combine kernel), sx_rope_kv_append_f32 / _v16 / _paged, sx_rmsnorm_planes and sx_split16, in the manner of
tests/test_attn_norm_matrix_gpu.py (GBuf, TiledOut, same_bits, stops_on_gpu_fault, _nanbuf, the NaN patterns, C_ACC and U32 are imported
from the GEMM / GEMV matrices). Every case drives the C entry point through _lib, so every stride is free. kernel_of_* restate the host
dispatch by hand; tests/test_cpu_suite.py holds the case tables against the instantiations parsed from precise.hip (source_kernels).
WORST keeps the worst |diff| / bound per (instantiation, dtype); the last test prints it.

ONE REFERENCE, MANY STORAGE FORMS. `logical` builds the logical rows of a case (q [G][T][H][D], K and V [G][H][Tmax][D], pos0, scale);
`ref_attention` computes in fp64: row t of sequence g sees keys 0 .. min(Tmax, pos0[g] + t + 1) - 1 (not causal: all Tmax keys); it
returns the context, A_d = sum_j p_j |V_jd|, S1 = max_ij scale sum_d |q_id| |k_jd| and the spread E = max_ij (max_j' s_ij' - s_ij) in
nats, all from the STORED operands (V rounded to 16 bits under v16; decode(code) * scale for the e4m3 cache; the fp64 rotation with the
tables rounded to the planes' dtype in the fused RoPE forms; in the KV8 fused forms the appended row as read back from the cache).
`Store` lays the same rows into guarded buffers: contiguous fp32, strided views (kv_row_stride / kv_head_stride / cache_seq_stride
larger than needed), V in 16 bits, e4m3 codes + power-of-two row scales (seedx_amd.quant.quantize_kv_rows), page pools (page_shift
5, 6, 7; the table a non-monotone permutation, page 0 all zeros, entries of unreserved ranges 0, two pages that no entry names).

WHAT A LAUNCH MAY READ. NaN sits in everything the header does not allow a launch to read: behind every operand, columns D .. row
stride, rows Tmax .. head stride, the k / v columns of the qkv buffer in the non-fused forms, the gap between the sequences' caches and
scale rows, pages no table entry names, the tables behind row Tmax, and every cache row above the rows a launch may load. Established
from the code: the VALU kernels (attn_f32_kernel, attn_f32_verify_kernel) load key rows t < kend <= min(Tmax, pos0 + rows of the block)
only, so in their cases every row above the current position holds NaN. The MFMA kernel loads the rest of its last 32-key tile (rows up
to min(Tmax, roundup32(pos0 + T)) - 1; paged: up to roundup32(pos0 + T) - 1 inside the tile's own page, whose rows at or past Tmax exist)
and relies on P = 0 and the -inf select: those rows hold the largest finite value of their storage type with alternating sign (codes:
+-448 with scale 2^64) — what a reused slot may hold — and the output must be finite and inside the bound all the same. A parked slot
(pos0 < 0) reads no key row in any causal form, whatever T, and its rows must come out as 0 (the header used to allow key row 0, which
leaked a reused slot's stale row into the planes). Its cache holds NaN except key row 0, which holds the same stale finite values: NaN
there would NOT show a kernel that still loads the row — a NaN score makes lsum NaN, `lsum > 0.f ? acc / lsum : 0.f` then stores 0, and
the kernels of before the fix pass 72 of the 78 parked cases on NaN but only 21 on the stale values. Every cache, pool and table ends in
>= 40 NaN rows and no position runs further past Tmax than that: no case needs a clamp to stay inside its allocation.

WHAT A LAUNCH MAY WRITE. Row-major planes live in a GBuf, tiled planes in a TiledOut (rows >= G*T of a block are not writable), the
split scratch in a GBuf. Every other buffer is compared bit for bit with its copy from before the launch: the qkv buffer, tables and
positions never change; caches, pools (the null page included) and scale arrays change only at the appended rows of the fused / verify
forms. Appended k is within 2 * 2^-24 (|x c| + |x' s|) of the fp64 rotation, appended v is bit-equal (the 16-bit rounding under v16).
A second identical launch gives the same bits (planes and appended rows).

THE BOUND of every attention output element (hi + lo summed in fp64):
       |got - ref| <= u_pl |ref| + floor + C32 * 2^-24 * A_d
u_pl = 2^-22 (fp16) / 2^-16 (bf16): hi rounds at u16 = 2^-11 / 2^-8 of the value, lo at u16 of what hi left. floor = 2^-25 (fp16: lo lands
on the subnormal grid) / 2^-126 (bf16). C32, in units of 2^-24 (one fp32 rounding), on the laws of sections 1 and 2 of the attn / norm
matrix (a chain of n fp32 additions costs C_ACC sqrt(n) of the sum of magnitudes; an error e of every p_j, relative, costs 2 e A_d: once
in the numerator, once in the normaliser):
       C32 = 2 ((C_ACC sqrt(n_s) + 1 + R) S1 + 2 E + 2) + 2 C_ACC sqrt(n_acc) + 4
  * the score: q * scale is rounded once (+ 1); VALU attn_score: n_s = DW + 4, the lane's 8 (DC = 1) or 16 (DC = 2) chained FMAs and the
    four butterfly additions; MFMA: n_s = 128, 64 chained v_mfma_f32_32x32x2 accumulations, each adding the products of both lane halves.
    An absolute score error e is a relative error e of p. R = 4 in the fused RoPE forms: two roundings each for the rotation of q and of
    the new key (S1 then uses |x c| + |x' s| for them). The e4m3 row scales multiply by powers of two: no term.
  * exp: s - m_new is rounded (<= E 2^-24), the product with log2(e) inside __expf again (<= E 2^-24), v_exp_f32 1 ulp = 2: 2 E + 2.
    alpha = exp(m_run - m_new) of attn_key_update, sc of attn_merge_groups, w of attn_merge_waves / attn_f32_combine_kernel and the MFMA
    kernel's per-tile alpha multiply numerator and normaliser by the SAME float: their own error cancels, their products are counted below.
  * the sums of p_j v_jd and of p_j, each n_acc additions: VALU n_acc = 2 (ceil(n / 16) + T') + 7 + nsplit: one rescale and one FMA per
    key of a group's stride (n visible keys; T' = T draft keys and own keys of the verify form, else 1 for the fused new key), the group
    merge (product, two butterflies), the four FMAs of attn_merge_waves and the nsplit FMAs of attn_f32_combine_kernel; MFMA n_acc = n +
    2 ceil(n / 32): two products per MFMA step, one alpha product per tile, the row sum's xor step.
  * the division (or reciprocal and product), the final comparison of lsum, the conversion: 4.
E comes from the reference and is at most 60 log2 units in every case (asserted). Measured ratios are far below 1 (profiles/
precise_matrix.md): the constant is the worst case of the law, tools/lab/precise_bound_sharpness.py shows what still leaves it.

PLANTED KEYS. Query row i owns key pi(i) with K[pi(i)] = q_i * 8 / (scale |q_i|^2) (score 8), q and the other keys N(0, 1): with at most
1536 keys the random keys sum to about 1536 e^(1/2) = 2500 against e^8 = 2981. Causal: pi is the row's own mask edge pos0 + t (in the
fused forms that is the NEW key: the unrotated row is the inverse rotation of the planted one); a causal row also owns up to two keys
below pos0 (one with the e4m3 cache or more than 700 keys) taken in turn from the edges of the walk: key 0, the last key of a full
16-group stride, the first and last key of every split's chunk, of the first and last 32-key MFMA tile and of every page. Not causal: the
rows own 0, 15, 16, Skv - 2, Skv - 1, then (37 i) mod Skv. The reference asserts that every planted key weighs >= 0.25 in its row for
D >= 40; at D = 8 random queries are not nearly orthogonal and the assertion is skipped (nothing else is).
Other data: `scale4` N(0, 1) at 4 / sqrt(D); `stair` scores rising by 55 log2 units from the first key to the last (every key rescales);
`first` key 0 55 log2 units above the rest.

THE OTHER ENTRY POINTS. sx_rope_kv_append_f32*: rotated q and k within 2 * 2^-24 (|x c| + |x' s|) of fp64 (two products, one addition or
a product and an FMA; tables rounded to table_dtype; a position outside [0, Tmax) rotates q with table row 0 and appends nothing), v
bit-equal (16-bit rounding under v16), k / v columns of qkv bit-unchanged, caches written at the appended rows only. sx_rmsnorm_planes:
|got - ref| <= u |ref| + floor + C 2^-24 |ref|, u = 2^-24 for y32 and u_pl for the planes, C = 2 it + 11 with it = ceil(cols / 2048) the
trips of rmsnorm_planes_row's loop: the sum of squares is it * 4 (the 8-term tree and the addition to ss) + 6 (wave_sum) + 2 (the four
waves) additions of non-negative terms plus the squares (+ 1), 1 ulp each, the mean / eps / sqrt / reciprocal 4 more; rstd takes half of
that; the two products 2; v_sqrt / v_rcp 2 of slack. The planes are, bit for bit, the split of y32. sx_split16 is exact: hi ==
rn16(clamp(x)) (fp16 clamps at +-65504), lo == rn16(x - hi)."""
import ctypes as C
import math
import os
import re
import zlib

import pytest
import torch

from tests.test_gemm_matrix_gpu import BF16, C_ACC, DTYPES, F16, NAN16_IN, NAN32_IN, U32, _nanbuf
from tests.test_gemv_matrix_gpu import GBuf, TiledOut, same_bits, stops_on_gpu_fault

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISE_HIP = os.path.join(ROOT, "seed-x_amd", "csrc", "precise.hip")

F32, F64 = torch.float32, torch.float64
U_PL = {F16: 2.0 ** -22, BF16: 2.0 ** -16}
FLOOR = {F16: 2.0 ** -25, BF16: 2.0 ** -126}
MAXF = {F32: 3.4028234663852886e38, F16: 65504.0, BF16: 3.3895313892515355e38}
LOG2E = 1.4426950408889634
PADROWS = 40             # NaN rows behind every cache / table: more than any position of a case runs past Tmax
WORST = {}               # (kernel instantiation, dtype) -> worst |diff| / bound
assert (NAN16_IN, NAN32_IN) == (0x7FFF, 0x7FFFFFFF)


def sx_code(dt):
    return {F16: 0, BF16: 1}[dt]


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def gen_of(cid, dev):
    return torch.Generator(device=dev).manual_seed(zlib.crc32(cid.encode()))


def nanbuf(n, dtype, dev):
    """_nanbuf, and 0x7f (the e4m3fn NaN code) for uint8"""
    if dtype == torch.uint8:
        return torch.full((n,), 0x7F, dtype=torch.uint8, device=dev)
    return _nanbuf(n, dtype, dev)


def bits(t):
    return t if t.dtype == torch.uint8 else t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def held(keys, got, ref, bound, what):
    d = (got - ref).abs()
    ratio = d / bound
    worst = float(torch.nan_to_num(ratio, nan=float("inf")).max())
    for key in keys:
        WORST[key] = max(WORST.get(key, 0.0), worst)
    if not worst <= 1.0:
        i = int(torch.nan_to_num(ratio, nan=float("inf")).argmax())
        idx = []
        for n in reversed(ratio.shape):
            idx.insert(0, i % n)
            i //= n
        idx = tuple(idx)
        raise AssertionError(f"{what} {keys}: {int((~(ratio <= 1.0)).sum())} of {ratio.numel()} elements beyond the fp64 bound; worst at {idx}: "
                             f"got {float(got[idx])!r}, ref {float(ref[idx])!r}, |diff| {float(d[idx]):.3e} > bound {float(bound[idx]):.3e}")
    return worst


def unchanged(buf, before, allowed, what):
    bad = bits(buf) != bits(before)
    if allowed is not None:
        bad &= ~allowed
    n = int(bad.sum())
    assert n == 0, f"{what}: {n} elements outside the documented extent were written; first at element {int(bad.nonzero()[0, 0])}"


# ----------------------------------------------------------------------------------------------------------------------------
# 1. sx_attention_f32: the cases
# ----------------------------------------------------------------------------------------------------------------------------
def case_name(c, fam, variant):
    store = "paged%d" % c["pshift"] if c["pshift"] else ("kv8" if c["kv8"] == 1 else ("kv8twin" if c["kv8"] == 2 else ("strided" if c["strided"] else "f32")))
    return (f"{fam}-{c['dt']}-G{c['G']}T{c['T']}H{c['H']}D{c['D']}-Tm{c['Tmax']}-" + ("p" + "_".join(str(p) for p in c["pos0"]) if c["causal"] else "nc") +
            f"-{store}{'-v16' if c['v16'] else ''}{'-ns%d' % c['nsplit'] if c['nsplit'] > 1 else ''}{'-rope' if c['rope'] else ''}"
            f"{'-tiled' if c['tiled'] else ''}{'-valu' if not variant else ''}{'-' + c['data'] if c['data'] != 'plant' else ''}")


def acase(fam, dt, **kw):
    c = dict(fam=fam, dt=dt, G=2, T=1, H=2, D=128, Tmax=64, pos0=None, causal=True, v16=False, kv8=0, pshift=0, strided=False, nsplit=1,
             rope=False, tiled=False, variant=1, data="plant", scale_mul=1.0)
    c.update(kw)
    if c["pos0"] is None:
        c["pos0"] = [max(0, c["Tmax"] - c["T"] - 7 * g) for g in range(c["G"])]
    assert len(c["pos0"]) == c["G"]
    c["id"], c["seed"] = case_name(c, fam, c["variant"]), case_name(c, "mfma" if fam == "mfma-twin" else fam, 1)     # a twin runs its MFMA case's data
    return c


def split_chunk(kend, nsplit):
    """attn_f32_kernel: chunk = ((kend + nsplit - 1) / nsplit + 15) & ~15"""
    return ((kend + nsplit - 1) // nsplit + 15) & ~15


def is_verify(c):
    return c["rope"] and c["T"] > 1


def is_mfma(c):
    """the host's `mfma` flag: the variant hook, a causal chunk above 8 rows at head_dim 128, row-major planes (the strides and the output
    pointer of every case are aligned)"""
    return bool(c["variant"]) and c["causal"] and c["T"] > 8 and c["D"] == 128 and not c["tiled"]


def kernel_of_attn(c):
    """The kernels sx_attention_f32 launches for a case, in the order of its branches: the paged launches, the verify form, the key
    splits, the MFMA kernel, the FP8 cache, the mixed cache, DC = 2, then QB by T. ("attn_f32_kernel", TT, QB, DC, V16, SPLIT, KV8, PAGED),
    ("attn_f32_verify_kernel", TT, TQ, V16), ("attn_f32_mfma_kernel", TT, V16, KV8, PAGED), ("attn_f32_combine_kernel", TT)."""
    tt, T, D, v16 = c["dt"].upper(), c["T"], c["D"], bool(c["v16"])
    split = T == 1 and c["nsplit"] > 1
    kv8 = 0 if (c["kv8"] == 2 and not c["rope"]) else c["kv8"]
    qb = 8 if T > 8 else (1 if T == 1 else 4)
    comb = ("attn_f32_combine_kernel", tt)
    if c["pshift"]:
        if split:
            return [("attn_f32_kernel", tt, 1, 1, v16, True, 0, True), comb]
        if is_mfma(c):
            return [("attn_f32_mfma_kernel", tt, v16, False, True)]
        return [("attn_f32_kernel", tt, qb, 1, v16, False, 0, True)]
    if is_verify(c):
        return [("attn_f32_verify_kernel", tt, 4 if T <= 4 else 8, v16), comb]
    if split:
        return [("attn_f32_kernel", tt, 1, 1, v16 and not kv8, True, kv8, False), comb]
    if is_mfma(c):
        return [("attn_f32_mfma_kernel", tt, v16 and kv8 != 1, kv8 == 1, False)]
    if kv8:
        return [("attn_f32_kernel", tt, 1 if kv8 == 2 else qb, 1, False, False, kv8, False)]
    if v16:
        return [("attn_f32_kernel", tt, qb, 1, True, False, 0, False)]
    if D > 128:
        return [("attn_f32_kernel", tt, 4, 2, False, False, 0, False)]
    return [("attn_f32_kernel", tt, qb, 1, False, False, 0, False)]


STORES = (dict(), dict(v16=True), dict(kv8=1), dict(pshift=5), dict(pshift=6), dict(pshift=7), dict(pshift=6, v16=True))
SPLIT_NS = (2, 3, 6, 16, 64)
MFMA_T = (9, 31, 32, 33, 127, 128, 129, 165)
MFMA_POS = (0, 5, 31, 32, 200)
FAMILIES = ("valu-d", "valu-dc2", "valu-t", "valu-pos", "valu-nc", "valu-store", "valu-tiled", "strided", "split", "split-rope", "fused1",
            "verify", "mfma", "mfma-twin", "stale", "scale4", "stair", "first")


def rope_boundary_pos(nsplit, lo):
    """the smallest position >= lo that is the first key of a split's chunk of its own launch (kend = pos + 1): the owning split changes there"""
    for p in range(lo, 4096):
        if p % split_chunk(p + 1, nsplit) == 0:
            return p
    raise AssertionError(nsplit)


def attn_cases():
    out = []
    for dt in DTYPES:
        A = lambda fam, **kw: out.append(acase(fam, dt, **kw))
        # ---- VALU attn_f32_kernel: D (DC = 1), DC = 2, T (QB), pos0, not causal, the storage forms, tiled planes, strides ----
        for D in (8, 64, 104, 120, 128):
            A("valu-d", G=2, T=3, H=3, D=D, Tmax=50, pos0=[20, 47])
            A("valu-d", G=2, T=1, H=3, D=D, Tmax=50, pos0=[33, 49])
        for D in (136, 160, 256):
            A("valu-dc2", G=2, T=5, H=2, D=D, Tmax=40, pos0=[0, 30])
            A("valu-dc2", G=2, T=5, H=2, D=D, Tmax=33, causal=False)
        for T in (1, 2, 3, 4, 5, 8):
            A("valu-t", G=2, T=T, H=2, D=128, Tmax=80, pos0=[17, 40])
            A("valu-t", G=2, T=T, H=1, D=64, Tmax=80, pos0=[17, 40])
        for T in (9, 15, 16, 17):
            A("valu-t", G=2, T=T, H=2, D=128, Tmax=80, pos0=[17, 40], variant=0)
            A("valu-t", G=2, T=T, H=1, D=64, Tmax=80, pos0=[17, 40])
        for T in (1, 5, 12):
            Tm = 72
            for pos in ([0, 15], [16, 17], [Tm - T, Tm - T + 2], [Tm - 1, Tm + 3], [-1, 20], [31, -1]):
                A("valu-pos", G=2, T=T, H=2, D=128, Tmax=Tm, pos0=pos, variant=0)
        for Skv in (1, 15, 16, 17, 129):
            A("valu-nc", G=2, T=5, H=2, D=64, Tmax=Skv, causal=False)
            A("valu-nc", G=1, T=1, H=3, D=128, Tmax=Skv, causal=False)
            A("valu-nc", G=2, T=12, H=1, D=128, Tmax=Skv, causal=False, strided=True)
        for T in (1, 3, 12):
            for st in STORES:
                A("valu-store", G=2, T=T, H=2, D=128, Tmax=150, pos0=[130, 70], variant=0, **st)
            A("valu-store", G=2, T=T, H=2, D=64, Tmax=150, pos0=[130, 70], v16=True)
        for G, T in ((1, 1), (4, 4), (1, 17), (4, 8)):
            A("valu-tiled", G=G, T=T, H=1, D=64, Tmax=60, pos0=[10 + 9 * g for g in range(G)], tiled=True)
            A("valu-tiled", G=G, T=T, H=2, D=128, Tmax=60, pos0=[10 + 9 * g for g in range(G)], tiled=True, v16=G == 4)
        A("valu-tiled", G=4, T=1, H=2, D=128, Tmax=100, pos0=[40, 70, 99, 3], tiled=True, nsplit=3)
        A("valu-tiled", G=4, T=4, H=1, D=128, Tmax=100, pos0=[40, 70, 90, 3], tiled=True, nsplit=2, rope=True)
        for T, D in ((1, 128), (3, 104), (12, 128), (5, 160)):
            A("strided", G=2, T=T, H=2, D=D, Tmax=70, pos0=[50, 21], strided=True, variant=0)
        A("strided", G=2, T=40, H=2, D=128, Tmax=70, pos0=[30, 21], strided=True)
        A("strided", G=2, T=1, H=2, D=128, Tmax=70, pos0=[50, 21], strided=True, nsplit=3)
        # ---- key splits, T = 1: kend = pos0 + 1 around 16 nsplit, all splits but one empty, 1499 keys ----
        main = (dict(), dict(v16=True), dict(kv8=1), dict(pshift=5), dict(pshift=6), dict(pshift=7))
        i = 0
        for ns in SPLIT_NS:
            for kend in (16 * ns - 1, 16 * ns, 16 * ns + 1, 1, 1499):
                Tm = 1536 if kend == 1499 else max(kend + 5, 40)
                for st in (main[0], main[1 + i % 5]):
                    A("split", G=2, T=1, H=2, D=128, Tmax=Tm, pos0=[kend - 1, min(Tm - 1, kend // 2 + 17)], nsplit=ns, **st)
                i += 1
        A("split", G=2, T=1, H=2, D=128, Tmax=99, pos0=[60, 97], nsplit=3, pshift=6, v16=True)
        A("split", G=2, T=1, H=3, D=64, Tmax=99, pos0=[60, 97], nsplit=3)
        A("split", G=3, T=1, H=2, D=128, Tmax=99, pos0=[60, -1, 98], nsplit=6)
        # ---- key splits with fused RoPE: the new key on a chunk boundary, on the first row of a page, at Tmax - 1, at Tmax ----
        for ns in (2, 6):
            pb = rope_boundary_pos(ns, 40 if ns > 2 else 16)
            for st in (dict(), dict(v16=True), dict(kv8=1), dict(kv8=2), dict(pshift=5), dict(pshift=6), dict(pshift=7), dict(pshift=5, v16=True)):
                page = 1 << (st.get("pshift") or 6)
                Tm = 3 * page + 8
                A("split-rope", G=2, T=1, H=2, D=128, Tmax=max(Tm, pb + 9), pos0=[pb, 2 * page], nsplit=ns, rope=True, **st)
                A("split-rope", G=2, T=1, H=2, D=128, Tmax=Tm, pos0=[Tm - 1, Tm], nsplit=ns, rope=True, **st)
        # ---- the fused step without splits ----
        for st in (dict(), dict(v16=True), dict(kv8=1), dict(kv8=2), dict(pshift=5), dict(pshift=6), dict(pshift=7), dict(pshift=7, v16=True)):
            A("fused1", G=3, T=1, H=2, D=128, Tmax=140, pos0=[0, 17, 128], rope=True, **st)
            A("fused1", G=3, T=1, H=2, D=128, Tmax=140, pos0=[-1, 139, 140], rope=True, **st)
        # ---- the verify form: TQ 4 / 8, per-row key ranges ----
        for T in (2, 4, 5, 8):
            for ns in (1, 2, 6):
                edge = 16 * ns * 2
                for v16 in (False, True):
                    A("verify", G=2, T=T, H=2, D=128, Tmax=edge + 40, pos0=[edge - 2, 14], nsplit=ns, rope=True, v16=v16)      # crosses 16 nsplit k / 16
                A("verify", G=3, T=T, H=1, D=128, Tmax=90, pos0=[90 - T + 1, -1, 33], nsplit=ns, rope=True, v16=T == 4)         # last row at Tmax; parked
        A("verify", G=4, T=8, H=2, D=128, Tmax=120, pos0=[0, 95, 112, 47], nsplit=2, rope=True)                               # G*T = 32
        # ---- the MFMA kernel (T > 8, D = 128) and its VALU twin on the same data ----
        mst = (dict(), dict(v16=True), dict(kv8=1), dict(pshift=5), dict(pshift=6), dict(pshift=7), dict(pshift=5, v16=True))
        i = 0
        for T in MFMA_T:
            for k in range(3):
                st = mst[0] if k == 0 else mst[1 + i % 6]
                i += k > 0
                p = MFMA_POS[(MFMA_T.index(T) + 2 * k) % 5]
                Tm = p + T + (9 if k != 1 else -3)                      # k = 1: the chunk runs past Tmax
                for variant in (1, 0):
                    A("mfma" if variant else "mfma-twin", G=2, T=T, H=1 if T > 100 else 2, D=128, Tmax=Tm, pos0=[p, max(0, p - 3)], variant=variant, **st)
        # ---- stale rows behind the last visible key: pos0 + T one key before, on and after a tile edge; a parked slot ----
        for end in (63, 64, 65, 50):
            for st in (dict(), dict(v16=True), dict(kv8=1), dict(pshift=5), dict(pshift=7)):
                A("stale", G=2, T=20, H=2, D=128, Tmax=100, pos0=[end - 20, end - 27], **st)
        for st in (dict(), dict(v16=True), dict(kv8=1), dict(pshift=6)):
            A("stale", G=3, T=20, H=1, D=128, Tmax=100, pos0=[-1, 33, -5], **st)
            A("stale", G=3, T=1, H=2, D=128, Tmax=100, pos0=[-1, 33, -5], **st)
            A("stale", G=3, T=1, H=2, D=128, Tmax=100, pos0=[-1, 33, -5], nsplit=3, **st)
        # ---- scale: 4 / sqrt(D); a staircase (every key rescales); the first key is the maximum — one per kernel family ----
        for fam, kw in (("scale4", dict(data="randn", scale_mul=4.0)), ("stair", dict(data="stair")), ("first", dict(data="first"))):
            A(fam, G=2, T=3, H=2, D=128, Tmax=200, pos0=[190, 77], **kw)                                    # VALU
            A(fam, G=2, T=3, H=2, D=160, Tmax=200, pos0=[190, 77], **kw)                                    # VALU, DC = 2
            A(fam, G=2, T=1, H=2, D=128, Tmax=200, pos0=[199, 77], nsplit=3, **kw)                          # splits + combine
            A(fam, G=2, T=1, H=2, D=128, Tmax=200, pos0=[150, 77], rope=True, **kw)                         # fused
            A(fam, G=2, T=4, H=2, D=128, Tmax=200, pos0=[150, 77], nsplit=2, rope=True, **kw)               # verify
            A(fam, G=2, T=40, H=2, D=128, Tmax=200, pos0=[150, 77], **kw)                                   # MFMA
            A(fam, G=2, T=40, H=2, D=128, Tmax=200, pos0=[150, 77], kv8=1, **kw)
    return out


ATTN = attn_cases()


# ----------------------------------------------------------------------------------------------------------------------------
# the logical rows and the fp64 reference (CPU or GPU: tools/lab/precise_bound_sharpness.py runs them without one)
# ----------------------------------------------------------------------------------------------------------------------------
def rope_tables(Tmax, D, dev):
    j = torch.arange(D // 2, device=dev, dtype=F64)
    ang = torch.arange(Tmax, device=dev, dtype=F64)[:, None] * (10000.0 ** (-2.0 * j / D))[None]
    return ang.cos().float(), ang.sin().float()


def rot64(x, c, s):
    h = x.shape[-1] // 2
    x1, x2 = x[..., :h], x[..., h:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)


def rotmag(x, c, s):
    h = x.shape[-1] // 2
    x1, x2 = x[..., :h].abs(), x[..., h:].abs()
    return torch.cat([x1 * c.abs() + x2 * s.abs(), x2 * c.abs() + x1 * s.abs()], -1)


def invrot64(y, c, s):
    h = y.shape[-1] // 2
    y1, y2, n = y[..., :h], y[..., h:], c * c + s * s
    return torch.cat([(y1 * c + y2 * s) / n, (y2 * c - y1 * s) / n], -1)


def n_visible(c):
    """[G][T]: the keys row t of sequence g sees"""
    G, T, Tmax = c["G"], c["T"], c["Tmax"]
    if not c["causal"]:
        return [[Tmax] * T for _ in range(G)]
    return [[0 if c["pos0"][g] < 0 else min(Tmax, c["pos0"][g] + t + 1) for t in range(T)] for g in range(G)]


def walk_edges(c, g):
    """Key positions at the edges of the kernels' walks, below pos0[g] (visible to every row of the sequence, nobody's mask edge)."""
    p0, T, Tmax = c["pos0"][g], c["T"], c["Tmax"]
    if p0 <= 0:
        return []
    n = min(Tmax, p0 + T)
    E = {0, 16 * (n // 16) - 1, 31, 32, 32 * ((n - 1) // 32) - 1, 32 * ((n - 1) // 32)}
    if c["nsplit"] > 1:
        ch = split_chunk(n, c["nsplit"])
        for k in range(1, c["nsplit"]):
            E |= {ch * k - 1, ch * k}
    if c["pshift"]:
        P = 1 << c["pshift"]
        for k in range(1, n // P + 1):
            E |= {P * k - 1, P * k}
    return sorted(e for e in E if 0 <= e < min(p0, Tmax))


def logical(c, dev):
    """The logical rows of a case. Qe [G][T][H][D], Ke / Ve [G][H][Tmax][D] fp32: the (rotated) q, keys and values the case is about; in the
    fused forms q_raw / k_raw / v_raw [G][T][H][D] are the unrotated rows of the qkv buffer, pt [G][T] the table row of each query row and
    valid [G][T] whether its position lies in [0, Tmax)."""
    from seedx_amd import quant
    dt = DTYPES[c["dt"]]
    G, T, H, D, Tmax = c["G"], c["T"], c["H"], c["D"], c["Tmax"]
    g_ = gen_of(c["seed"], dev)
    scale = float(torch.tensor(c["scale_mul"] * D ** -0.5, dtype=F32))
    rn = lambda *s: torch.randn(*s, device=dev, generator=g_)
    Qe, Ke, Ve = rn(G, T, H, D), rn(G, H, Tmax, D), rn(G, H, Tmax, D)
    planted = []                                                 # (g, t, h, key)
    nvis = n_visible(c)
    if c["data"] == "plant":
        kvec = lambda g, t, h: (Qe[g, t, h].double() * 8.0 / (scale * Qe[g, t, h].double().pow(2).sum())).float()
        if c["causal"]:
            nsec = 1 if (c["kv8"] or max(max(r) for r in nvis) > 700) else 2
            for g in range(G):
                E, taken, k = walk_edges(c, g), set(), 0
                for t in range(T):
                    p = c["pos0"][g] + t
                    for h in range(H):
                        if c["pos0"][g] >= 0 and p < Tmax:
                            Ke[g, h, p] = kvec(g, t, h)
                            planted.append((g, t, h, p))
                        for _ in range(nsec if E else 0):
                            e = E[k % len(E)]
                            k += 1
                            if (h, e) not in taken:
                                taken.add((h, e))
                                Ke[g, h, e] = kvec(g, t, h)
                                planted.append((g, t, h, e))
        else:
            cand, pos = [0, 15, 16, Tmax - 2, Tmax - 1] + [(37 * i) % Tmax for i in range(Tmax)], []
            for p in cand:
                if 0 <= p < Tmax and p not in pos:
                    pos.append(p)
            for t, p in enumerate(pos[:T]):
                for g in range(G):
                    for h in range(H):
                        Ke[g, h, p] = kvec(g, t, h)
                        planted.append((g, t, h, p))
    elif c["data"] in ("stair", "first"):
        # scores = a common part c_j (log2 units) + small noise: Q = 4 u + noise orthogonal to u, K_j = b_j u + noise, |u| = 1
        j = torch.arange(Tmax, device=dev, dtype=F32)
        cj = 55.0 * j / max(Tmax - 1, 1) if c["data"] == "stair" else torch.where(j < 1, 55.0, 0.0)
        u = torch.full((D,), D ** -0.5, device=dev)
        qn = rn(G, T, H, D)
        Qe = 4.0 * u + (qn - (qn @ u)[..., None] * u)
        Ke = (cj / (4.0 * scale * LOG2E))[:, None] * u + 0.02 * rn(G, H, Tmax, D)
    L = dict(scale=scale, planted=planted, nvis=nvis, dt=dt)
    if c["v16"]:
        L["Ve_raw"] = Ve
        Ve = Ve.to(dt).float()
    if c["kv8"]:                                                 # the cache rows hold dequantised values (1: as codes and scales)
        L["kcodes"], L["kscale"] = quant.quantize_kv_rows(Ke)
        L["vcodes"], L["vscale"] = quant.quantize_kv_rows(Ve)
        Ke_q, Ve_q = quant.dequantize_kv_rows(L["kcodes"], L["kscale"]), quant.dequantize_kv_rows(L["vcodes"], L["vscale"])
    if c["rope"]:
        cos, sin = rope_tables(Tmax, D, dev)
        pos = torch.tensor(c["pos0"], device=dev)[:, None] + torch.arange(T, device=dev)[None]
        valid = (pos >= 0) & (pos < Tmax) & (torch.tensor(c["pos0"], device=dev)[:, None] >= 0)
        pt = torch.where(valid, pos, torch.zeros_like(pos))
        c64, s64 = cos[pt].to(dt).double()[:, :, None], sin[pt].to(dt).double()[:, :, None]          # [G][T][1][D/2]
        gi = torch.arange(G, device=dev)[:, None].expand(G, T)
        k_new = Ke[gi, :, pt]                                     # [G][T][H][D]: the key planted at the row's own position
        v_new = (L["Ve_raw"] if c["v16"] else Ve)[gi, :, pt]
        vm = valid[:, :, None, None]
        L.update(cos=cos, sin=sin, pt=pt, valid=valid, c64=c64, s64=s64,
                 q_raw=invrot64(Qe.double(), c64, s64).float(),
                 k_raw=torch.where(vm, invrot64(k_new.double(), c64, s64).float(), rn(G, T, H, D)),
                 v_raw=torch.where(vm, v_new, rn(G, T, H, D)))
    if c["kv8"]:
        Ke, Ve = Ke_q, Ve_q
    L.update(Qe=Qe, Ke=Ke, Ve=Ve)
    return L


def reference_operands(c, L, new_k=None, new_v=None):
    """q64 [G][T][H][D], K64 / V64 [G][H][Tmax][D] and the magnitudes for S1, from the STORED operands. Fused forms: q and the new keys are
    the fp64 rotation of the stored unrotated rows with the rounded tables (new_k / new_v: the appended rows as read back, KV8 forms)."""
    dt = L["dt"]
    if not c["rope"]:
        q64, K64, V64 = L["Qe"].double(), L["Ke"].double(), L["Ve"].double()
        return q64, K64, V64, q64.abs(), K64.abs()
    G, T = c["G"], c["T"]
    q64, qmag = rot64(L["q_raw"].double(), L["c64"], L["s64"]), rotmag(L["q_raw"].double(), L["c64"], L["s64"])
    K64, V64 = L["Ke"].double().clone(), L["Ve"].double().clone()
    kmag = K64.abs()
    kr, km = rot64(L["k_raw"].double(), L["c64"], L["s64"]), rotmag(L["k_raw"].double(), L["c64"], L["s64"])
    vr = L["v_raw"].to(dt).double() if c["v16"] else L["v_raw"].double()
    for g in range(G):
        for t in range(T):
            if bool(L["valid"][g, t]):
                p = int(L["pt"][g, t])
                K64[g, :, p] = kr[g, t] if new_k is None else new_k[g, t].double()
                kmag[g, :, p] = km[g, t] if new_k is None else new_k[g, t].double().abs()
                V64[g, :, p] = vr[g, t] if new_v is None else new_v[g, t].double()
    return q64, K64, V64, qmag, kmag


def ref_attention(c, L, q64, K64, V64, qmag=None, kmag=None, check_planted=True):
    """fp64 context [G][T][H][D], A_d, S1 and the spread E (nats). Rows without a visible key (a parked slot) are 0."""
    G, T, H, D, Tmax = c["G"], c["T"], c["H"], c["D"], c["Tmax"]
    dev = q64.device
    nvis = torch.tensor(L["nvis"], device=dev)                                                   # [G][T]
    hidden = torch.arange(Tmax, device=dev)[None, None, None, :] >= nvis[:, None, :, None]     # [G][1][T][Tmax]
    live = ~hidden.expand(G, H, T, Tmax)
    K64 = torch.where(live.any(2)[..., None], K64, torch.zeros_like(K64))                       # rows nobody sees: NaN / stale in storage
    V64 = torch.where(live.any(2)[..., None], V64, torch.zeros_like(V64))
    qh = q64.permute(0, 2, 1, 3)
    s = (L["scale"] * (qh @ K64.transpose(-1, -2))).masked_fill(~live, float("-inf"))
    m = s.max(-1, keepdim=True)[0]
    e = torch.where(live, torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m))), torch.zeros_like(s))
    p = e / e.sum(-1, keepdim=True).clamp_min(1e-300)
    if check_planted and D >= 40:
        for (g, t, h, key) in L["planted"]:
            if key < L["nvis"][g][t]:
                assert float(p[g, h, t, key]) >= 0.25, f"{c['id']}: the planted key {key} of row {(g, t, h)} weighs only {float(p[g, h, t, key]):.3f}"
    qm = (q64.abs() if qmag is None else qmag).permute(0, 2, 1, 3)
    km = torch.where(live.any(2)[..., None], K64.abs() if kmag is None else kmag, torch.zeros_like(K64))
    s1 = float((L["scale"] * (qm @ km.transpose(-1, -2))).masked_fill(~live, 0.0).max())
    spread = float(torch.where(live, m - s, torch.zeros_like(s)).max()) if bool(live.any()) else 0.0
    assert spread <= 60.0 / LOG2E, f"{c['id']}: scores spread over {spread * LOG2E:.1f} log2 units"
    return (p @ V64).permute(0, 2, 1, 3), (p @ V64.abs()).permute(0, 2, 1, 3), s1, spread


def c32_of(c, s1, spread):
    """C32 of the module docstring for the kernels of a case"""
    n = max(1, max(max(r) for r in n_visible(c)))
    if is_mfma(c):
        n_s, n_acc = 128, n + 2 * -(-n // 32)
    else:
        tq = c["T"] if is_verify(c) else 1
        n_s, n_acc = (16 if c["D"] > 128 else 8) + 4, 2 * (-(-n // 16) + tq) + 7 + max(1, c["nsplit"])
    return 2.0 * ((C_ACC * math.sqrt(n_s) + 1.0 + (4.0 if c["rope"] else 0.0)) * max(s1, 1.0) + 2.0 * spread + 2.0) + 2.0 * C_ACC * math.sqrt(n_acc) + 4.0


def attn_bound(c, ref, A, s1, spread):
    dt = DTYPES[c["dt"]]
    return U_PL[dt] * ref.abs() + FLOOR[dt] + c32_of(c, s1, spread) * U32 * A


# ----------------------------------------------------------------------------------------------------------------------------
# storage
# ----------------------------------------------------------------------------------------------------------------------------
class Store:
    """The buffers of one launch of a case and the argument struct; `before` holds a copy of every read-only or partly writable buffer."""

    def __init__(self, c, L, dev):
        from seedx_amd import _lib
        self.c, self.L, self.dev = c, L, dev
        dt = L["dt"]
        G, T, H, D, Tmax = c["G"], c["T"], c["H"], c["D"], c["Tmax"]
        cols = H * D
        # ---- q (and, fused, k / v) rows of the qkv buffer ----
        self.qs = qs = 3 * cols + (8 if c["strided"] else 0)
        self.qkv = nanbuf(G * T * qs + 256, F32, dev)
        rows = self.qkv[:G * T * qs].view(G, T, qs)
        if c["rope"]:
            rows[..., :cols], rows[..., cols:2 * cols], rows[..., 2 * cols:3 * cols] = (L[k].reshape(G, T, cols) for k in ("q_raw", "k_raw", "v_raw"))
        else:
            rows[..., :cols] = L["Qe"].reshape(G, T, cols)
        # ---- which cache rows hold data (1), stale finite values (2) or NaN (0) ----
        cls = torch.zeros(G, Tmax, dtype=torch.int32)
        self.reserved = []
        for g in range(G):
            p0 = c["pos0"][g]
            if not c["causal"]:
                n = Tmax
            elif p0 < 0:
                n = 0
                cls[g, 0] = 2                                     # a parked slot: stale values in key row 0 (a NaN would be swallowed: docstring)
            else:
                n = min(Tmax, p0) if c["rope"] else min(Tmax, p0 + T)
            cls[g, :n] = 1
            if is_mfma(c) and p0 >= 0:
                cls[g, n:min(Tmax, (n + 31) // 32 * 32)] = 2      # the rest of the MFMA kernel's last 32-key tile
            self.reserved.append(0 if (c["causal"] and p0 < 0) else min(Tmax, p0 + T) if c["causal"] else Tmax)
        self.cls = cls = cls.to(dev)
        # ---- where row (g, h, r) starts ----
        ar = lambda n: torch.arange(n, device=dev, dtype=torch.int64)
        self.ptab = None
        if c["pshift"]:
            P = 1 << c["pshift"]
            self.ptw = ptw = (Tmax + P - 1) // P
            need = [(n + P - 1) // P for n in self.reserved]
            self.n_pages = sum(need) + 2
            order = torch.randperm(self.n_pages, generator=torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))).tolist()
            names = [o + 1 for o in order][:sum(need)]
            if len(names) >= 3 and names == sorted(names):
                names.reverse()
            tab = torch.zeros(G, ptw, dtype=torch.int32)
            for g in range(G):
                for i in range(need[g]):
                    tab[g, i] = names.pop()
            assert int(tab.min()) >= 0 and int(tab.max()) <= self.n_pages
            self.tab = tab = tab.to(dev)
            self.ptab = torch.zeros(G * ptw + 16, dtype=torch.int32, device=dev)
            self.ptab[:G * ptw] = tab.reshape(-1)
            self.page_stride = H * P * D + 16
            self.rs, self.hs, self.seq = D, P * D, 0
            pg = tab.long()[:, ar(Tmax) >> c["pshift"]]                                            # [G][Tmax]
            self.off = pg[:, None, :] * self.page_stride + ar(H)[None, :, None] * (P * D) + (ar(Tmax) & (P - 1))[None, None, :] * D
            self.placed = (pg != 0)[:, None, :].expand(G, H, Tmax)
            nel = (self.n_pages + 1) * self.page_stride
        else:
            self.rs = rs = D + (8 if c["strided"] else 0)
            self.hs = hs = (Tmax + 3) * rs + 16 if c["strided"] else Tmax * rs
            self.seq = seq = H * hs + 32
            self.off = ar(G)[:, None, None] * seq + ar(H)[None, :, None] * hs + ar(Tmax)[None, None, :] * rs
            self.placed = torch.ones(G, H, Tmax, dtype=torch.bool, device=dev)
            nel = G * seq
        self.idx = self.off[..., None] + ar(D)                                                     # [G][H][Tmax][D] element index
        kdt = torch.uint8 if c["kv8"] == 1 else F32
        vdt = torch.uint8 if c["kv8"] == 1 else (dt if c["v16"] else F32)
        self.kbuf, self.vbuf = nanbuf(nel + PADROWS * self.rs + 256, kdt, dev), nanbuf(nel + PADROWS * self.rs + 256, vdt, dev)
        if c["pshift"]:
            self.kbuf[:H * (1 << c["pshift"]) * D] = 0
            self.vbuf[:H * (1 << c["pshift"]) * D] = 0
        sign = torch.where(ar(D) % 2 == 0, 1.0, -1.0)
        live, stale = (cls == 1)[:, None, :, None], (cls == 2)[:, None, :, None]
        for buf, val, cod in ((self.kbuf, L["Ke"], L.get("kcodes")), (self.vbuf, L["Ve"], L.get("vcodes"))):
            if buf.dtype == torch.uint8:
                dense = torch.where(live, cod, torch.where(stale, torch.where(ar(D) % 2 == 0, 0x7E, 0xFE).to(torch.uint8), torch.full_like(cod, 0x7F)))
            else:
                nan = nanbuf(val.numel(), buf.dtype, dev).view(val.shape)
                dense = torch.where(live, val.to(buf.dtype), torch.where(stale, (sign * MAXF[buf.dtype]).to(buf.dtype).expand(val.shape), nan))
            buf[self.idx[self.placed].reshape(-1)] = dense[self.placed].reshape(-1)
            if c["pshift"] and is_mfma(c):
                # the paged MFMA kernel takes the rest of its last tile from the tile's own page, rows at or past Tmax included (they exist in
                # the page; the contiguous kernel clamps to Tmax - 1 instead): stale there as well
                for g in range(G):
                    n = self.reserved[g]
                    for r in range(Tmax, (n + 31) // 32 * 32 if c["pos0"][g] >= 0 else 0):
                        o = int(self.tab[g, r >> c["pshift"]]) * self.page_stride + ar(H)[:, None] * self.hs + (r & ((1 << c["pshift"]) - 1)) * D + ar(D)
                        buf[o.reshape(-1)] = (sign * MAXF[buf.dtype]).to(buf.dtype).repeat(H)
        self.ksc = self.vsc = None
        if c["kv8"] == 1:
            self.scs = H * Tmax + 8
            self.soff = ar(G)[:, None, None] * self.scs + ar(H)[None, :, None] * Tmax + ar(Tmax)[None, None, :]
            self.ksc, self.vsc = nanbuf(G * self.scs + 64, F32, dev), nanbuf(G * self.scs + 64, F32, dev)
            for buf, sc in ((self.ksc, L["kscale"]), (self.vsc, L["vscale"])):
                nan = nanbuf(sc.numel(), F32, dev).view(sc.shape)
                buf[self.soff.reshape(-1)] = torch.where(live[..., 0], sc, torch.where(stale[..., 0], torch.full_like(sc, 2.0 ** 64), nan)).reshape(-1)
        # ---- positions, tables, output, scratch ----
        self.pos = torch.full((G + 8,), -(1 << 20), dtype=torch.int32, device=dev)
        self.pos[:G] = torch.tensor(c["pos0"], dtype=torch.int32)
        self.cos = self.sin = None
        if c["rope"]:
            self.cos, self.sin = nanbuf((Tmax + PADROWS) * (D // 2), F32, dev), nanbuf((Tmax + PADROWS) * (D // 2), F32, dev)
            self.cos[:Tmax * (D // 2)], self.sin[:Tmax * (D // 2)] = L["cos"].reshape(-1), L["sin"].reshape(-1)
        if c["tiled"]:
            self.ob = TiledOut(2, G * T, cols, dt, dev)
        else:
            self.ob = GBuf(G * T * 2 * cols, dt, dev)
            self.ob.allow()[:] = True
        self.sb = None
        if is_verify(c) or (T == 1 and c["nsplit"] > 1):
            self.sb = GBuf(G * T * H * c["nsplit"] * (D + 2), F32, dev)
            self.sb.allow()[:] = True
        # ---- what the launch may write into the caches: the appended rows ----
        self.kallow = torch.zeros(self.kbuf.numel(), dtype=torch.bool, device=dev)
        self.sallow = torch.zeros(self.ksc.numel(), dtype=torch.bool, device=dev) if self.ksc is not None else None
        if c["rope"]:
            for g in range(G):
                for t in range(T):
                    if bool(L["valid"][g, t]):
                        p = int(L["pt"][g, t])
                        self.kallow[self.idx[g, :, p].reshape(-1)] = True
                        if self.sallow is not None:
                            self.sallow[self.soff[g, :, p]] = True
        self.watched = [("qkv", self.qkv, None), ("k cache", self.kbuf, self.kallow), ("v cache", self.vbuf, self.kallow), ("positions", self.pos, None)]
        for name, buf, allow in (("k scales", self.ksc, self.sallow), ("v scales", self.vsc, self.sallow), ("cos", self.cos, None),
                                 ("sin", self.sin, None), ("page table", self.ptab, None)):
            if buf is not None:
                self.watched.append((name, buf, allow))
        self.before = [b.clone() for _, b, _ in self.watched]
        a = self.a = _lib.AttnF32Args()
        a.q, a.kcache, a.vcache, a.out = self.qkv.data_ptr(), self.kbuf.data_ptr(), self.vbuf.data_ptr(), self.ob.ptr()
        a.pos0_dev = self.pos.data_ptr() if c["causal"] else None
        a.q_row_stride, a.cache_seq_stride = qs, self.seq
        a.kv_row_stride, a.kv_head_stride = (self.rs, self.hs) if c["strided"] else (0, 0)
        a.G, a.T, a.H, a.D, a.Tmax = G, T, H, D, Tmax
        a.dtype = sx_code(dt) | (_lib.SX_TILED16 if c["tiled"] else 0)
        a.scale, a.causal, a.v16, a.nsplit = L["scale"], int(c["causal"]), int(c["v16"]), c["nsplit"]
        a.scratch = self.sb.ptr() if self.sb is not None else None
        if c["rope"]:
            a.rope_cos, a.rope_sin = self.cos.data_ptr(), self.sin.data_ptr()
            a.k_new, a.v_new = self.qkv.data_ptr() + 4 * cols, self.qkv.data_ptr() + 8 * cols
        a.kv_fp8 = c["kv8"]
        if c["kv8"] == 1:
            a.k_scale, a.v_scale, a.scale_seq_stride = self.ksc.data_ptr(), self.vsc.data_ptr(), self.scs
        if c["pshift"]:
            a.page_table, a.page_shift, a.n_pages, a.page_stride = self.ptab.data_ptr(), c["pshift"], self.n_pages, self.page_stride
        for ptr in (a.q, a.kcache, a.vcache, a.out):
            assert ptr % 16 == 0

    def launch(self, lib):
        from seedx_amd import _lib
        try:
            assert lib.sx_attention_f32_variant(int(self.c["variant"])) == 0
            st = lib.sx_attention_f32(C.byref(self.a), stream())
        finally:
            lib.sx_attention_f32_variant(1)
        _lib.check(st, self.c["id"])
        torch.cuda.synchronize()
        return self

    def check_writes(self, what):
        self.ob.check(what + " (planes)")
        if self.sb is not None:
            self.sb.check(what + " (scratch)")
        for (name, buf, allow), before in zip(self.watched, self.before):
            unchanged(buf, before, allow, f"{what} ({name})")

    def planes(self):
        """(hi, lo) [G][T][H][D]"""
        c = self.c
        G, T, H, D = c["G"], c["T"], c["H"], c["D"]
        if c["tiled"]:
            hi, lo = self.ob.planes()
        else:
            pl = self.ob.body.view(G * T, 2, H * D)
            hi, lo = pl[:, 0], pl[:, 1]
        return hi.reshape(G, T, H, D), lo.reshape(G, T, H, D)

    def appended(self):
        """The appended k / v rows as the cache holds them after the launch, [G][T][H][D] in the caches' types (KV8 = 1: dequantised
        fp32), and the raw bits read (for the determinism check); rows that append nothing are 0."""
        from seedx_amd import quant
        c, L = self.c, self.L
        G, T, H, D = c["G"], c["T"], c["H"], c["D"]
        k = torch.zeros(G, T, H, D, dtype=self.kbuf.dtype, device=self.dev)
        v = torch.zeros(G, T, H, D, dtype=self.vbuf.dtype, device=self.dev)
        ks = torch.zeros(G, T, H, device=self.dev)
        vs = torch.zeros(G, T, H, device=self.dev)
        for g in range(G):
            for t in range(T):
                if bool(L["valid"][g, t]):
                    p = int(L["pt"][g, t])
                    k[g, t], v[g, t] = self.kbuf[self.idx[g, :, p]], self.vbuf[self.idx[g, :, p]]
                    if c["kv8"] == 1:
                        ks[g, t], vs[g, t] = self.ksc[self.soff[g, :, p]], self.vsc[self.soff[g, :, p]]
        raw = (k, v, ks, vs)
        if c["kv8"] == 1:
            assert not bool(((k & 0x7F) == 0x7F).any() | ((v & 0x7F) == 0x7F).any()), f"{c['id']}: a NaN code was appended"
            k, v = quant.dequantize_kv_rows(k, ks), quant.dequantize_kv_rows(v, vs)
        return k, v, raw


def run_attn(c, dev):
    from seedx_amd import _lib
    lib = _lib.load()
    dt = DTYPES[c["dt"]]
    L = logical(c, dev)
    S = Store(c, L, dev).launch(lib)
    S.check_writes(c["id"])
    hi, lo = S.planes()
    assert bool(torch.isfinite(hi.float()).all() & torch.isfinite(lo.float()).all()), \
        f"{c['id']}: non-finite planes: an unwritten element, a read outside an operand, or a stale row that was not cancelled"
    new_k = new_v = raw = None
    if c["rope"]:
        ak, av, raw = S.appended()
        vm = L["valid"][:, :, None, None]
        assert bool(torch.isfinite(ak.float()).all() & torch.isfinite(av.float()).all()), f"{c['id']}: non-finite appended rows"
        if c["kv8"]:
            new_k, new_v = ak, av                                # the reference attends to the row as read back (the quantiser has its own tests)
        else:
            kr = rot64(L["k_raw"].double(), L["c64"], L["s64"])
            kb = 2.0 * U32 * rotmag(L["k_raw"].double(), L["c64"], L["s64"]) + 2.0 ** -126
            held([("appended k",) + kernel_of_attn(c)[0] + (c["dt"],)], torch.where(vm, ak.double(), kr), kr, kb, c["id"] + " (appended k)")
            want_v = L["v_raw"].to(dt) if c["v16"] else L["v_raw"]
            assert same_bits(torch.where(vm, av, want_v), want_v), f"{c['id']}: the appended v rows are not the {'rounded ' if c['v16'] else ''}v rows"
    q64, K64, V64, qmag, kmag = reference_operands(c, L, new_k, new_v)
    ref, A, s1, spread = ref_attention(c, L, q64, K64, V64, qmag, kmag)
    got = hi.double() + lo.double()
    keys = [k + (c["dt"],) for k in kernel_of_attn(c)]
    worst = held(keys, got, ref, attn_bound(c, ref, A, s1, spread), c["id"])
    S2 = Store(c, L, dev).launch(lib)
    S2.check_writes(c["id"] + " (second launch)")
    hi2, lo2 = S2.planes()
    assert same_bits(hi2, hi) and same_bits(lo2, lo), f"{c['id']}: two identical launches differ"
    if c["rope"]:
        assert all(same_bits(x, y) for x, y in zip(S2.appended()[2], raw)), f"{c['id']}: the appended rows of two identical launches differ"
    print(f"{c['id']}: {keys[0]} worst |diff| / bound {worst:.4f} (C32 {c32_of(c, s1, spread):.0f}, S1 {s1:.1f}, E {spread * LOG2E:.1f} log2)")


@pytest.mark.parametrize("c", ATTN, ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_attention_f32_vs_fp64(dev, c):
    run_attn(c, dev)


@stops_on_gpu_fault
def test_attention_f32_refusals(dev):
    """Every SX_CHECK of sx_attention_f32 that the fp8 / paged / spec tests do not cover returns non-zero and launches nothing: the planes
    and the scratch keep their guard bits. (Every buffer is large enough for the call as if it were taken.)"""
    from seedx_amd import _lib
    lib = _lib.load()
    big = lambda: torch.zeros(1 << 20, device=dev)
    q, k, v = big(), big(), big()
    pos = torch.tensor([5, 7, 9, 0], dtype=torch.int32, device=dev)
    T16 = _lib.SX_TILED16
    base = dict(G=2, T=1, H=2, D=128, Tmax=32, dtype=0, causal=1, v16=0, nsplit=1, kv_row_stride=0, q_row_stride=None, scratch=True)
    for what, kw in (("D % 8", dict(D=12)), ("D > 256", dict(D=264)), ("tiled, 33 rows", dict(G=3, T=11, dtype=T16)),
                     ("tiled, H*D % 32", dict(H=1, D=24, dtype=T16 | 1)), ("kv_row_stride % 4", dict(kv_row_stride=130)),
                     ("q_row_stride % 4", dict(q_row_stride=770)), ("q_row_stride < H*D", dict(q_row_stride=128)),
                     ("v16 with D > 128", dict(D=160, v16=1)), ("v16 rows not 16-B aligned", dict(D=64, v16=1, kv_row_stride=68)),
                     ("splits with D > 128", dict(D=160, nsplit=2)), ("splits without scratch", dict(nsplit=2, scratch=False)),
                     ("nsplit > 64", dict(nsplit=65)), ("dtype", dict(dtype=2))):
        p = dict(base, **kw)
        ob, sb = GBuf(1 << 16, F16, dev), GBuf(1 << 16, F32, dev)
        a = _lib.AttnF32Args()
        a.q, a.kcache, a.vcache, a.out, a.pos0_dev = q.data_ptr(), k.data_ptr(), v.data_ptr(), ob.ptr(), pos.data_ptr()
        a.G, a.T, a.H, a.D, a.Tmax, a.dtype = p["G"], p["T"], p["H"], p["D"], p["Tmax"], p["dtype"]
        a.q_row_stride = p["q_row_stride"] or 3 * p["H"] * p["D"]
        a.cache_seq_stride, a.kv_row_stride = p["H"] * p["Tmax"] * 264, p["kv_row_stride"]
        a.scale, a.causal, a.v16, a.nsplit = 0.1, p["causal"], p["v16"], p["nsplit"]
        a.scratch = sb.ptr() if p["scratch"] else None
        st = lib.sx_attention_f32(C.byref(a), stream())
        torch.cuda.synchronize()
        assert st != 0, f"sx_attention_f32 took {what}: {kw}"
        ob.check(f"refused ({what}): planes")
        sb.check(f"refused ({what}): scratch")
    assert lib.sx_attention_f32_variant(2) != 0 and lib.sx_attention_f32_variant(1) == 0


# ----------------------------------------------------------------------------------------------------------------------------
# 2. sx_rope_kv_append_f32 / _v16 / _paged
# ----------------------------------------------------------------------------------------------------------------------------
ROPE_D = (8, 64, 104, 128, 160, 256)
ROPE_T = (1, 5, 37)
ROPE_TMAX = 64
ROPE_POS = {"zero": lambda T: [0, 3], "cross": lambda T: [ROPE_TMAX - T // 2 - 1, ROPE_TMAX - 1], "past": lambda T: [ROPE_TMAX, ROPE_TMAX + 2],
            "negative": lambda T: [-T, -2]}
ROPE = [dict(id=f"rope-{dt}-D{D}-T{T}-{pos}{'-v16' if v16 else ''}{'-paged%d' % ps if ps else ''}", dt=dt, D=D, T=T, pos=pos, v16=v16, pshift=ps)
        for dt in DTYPES for D in ROPE_D for T in ROPE_T for pos in ROPE_POS for v16 in (False, True) for ps in ((0, 5, 6, 7) if D == 128 else (0,))]


def kernel_of_rope(c):
    """rope_kv_f32_impl: the paged kernel with a page table, else the contiguous one; <TT of table_dtype, V16>"""
    return ("rope_kv_f32_paged_kernel" if c["pshift"] else "rope_kv_f32_kernel", c["dt"].upper(), bool(c["v16"]))


def run_rope(c, dev):
    from seedx_amd import _lib
    lib = _lib.load()
    dt = DTYPES[c["dt"]]
    G, H, D, T, Tmax = 2, 2, c["D"], c["T"], ROPE_TMAX
    cols, half = H * D, D // 2
    g_ = gen_of(c["id"], dev)
    pos0 = ROPE_POS[c["pos"]](T)
    x = torch.randn(G, T, 3, H, D, device=dev, generator=g_)
    qkv = nanbuf(G * T * 3 * cols + 256, F32, dev)
    qkv[:G * T * 3 * cols] = x.reshape(-1)
    cos, sin = rope_tables(Tmax, D, dev)
    cb, sb = nanbuf((Tmax + PADROWS) * half, F32, dev), nanbuf((Tmax + PADROWS) * half, F32, dev)
    cb[:Tmax * half], sb[:Tmax * half] = cos.reshape(-1), sin.reshape(-1)
    pos = torch.tensor(pos0, device=dev)[:, None] + torch.arange(T, device=dev)[None]
    valid = (pos >= 0) & (pos < Tmax)
    pt = torch.where(valid, pos, torch.zeros_like(pos))
    ar = lambda n: torch.arange(n, device=dev, dtype=torch.int64)
    vdt = dt if c["v16"] else F32
    if c["pshift"]:
        P = 1 << c["pshift"]
        ptw = (Tmax + P - 1) // P
        n_pages = G * ptw + 2
        names = [((5 * i + 3) % (G * ptw)) + 1 for i in range(G * ptw)] if (G * ptw) % 5 else list(range(G * ptw, 0, -1))
        tab = torch.tensor(names, dtype=torch.int32).view(G, ptw)
        tab[1, ptw - 1] = 0                                       # no reservation behind the last page of sequence 1: nothing is written there
        tab = tab.to(dev)
        page_stride = H * P * D + 16
        off = tab.long()[:, ar(Tmax) >> c["pshift"]][:, None, :] * page_stride + ar(H)[None, :, None] * (P * D) + (ar(Tmax) & (P - 1))[None, None, :] * D
        heldpg = (tab.long()[:, ar(Tmax) >> c["pshift"]] != 0)
        nel = (n_pages + 1) * page_stride
    else:
        seq = H * Tmax * D + 32
        off = ar(G)[:, None, None] * seq + ar(H)[None, :, None] * (Tmax * D) + ar(Tmax)[None, None, :] * D
        heldpg = torch.ones(G, Tmax, dtype=torch.bool, device=dev)
        nel = G * seq
    kc, vc = GBuf(nel + PADROWS * D, F32, dev, before=64, after=64), GBuf(nel + PADROWS * D, vdt, dev, before=64, after=64)
    writes = valid & heldpg[ar(G)[:, None], pt]                                                    # [G][T]
    for g in range(G):
        for t in range(T):
            if bool(writes[g, t]):
                ix = (off[g, :, int(pt[g, t])][:, None] + ar(D)).reshape(-1)
                kc.allow()[ix] = True
                vc.allow()[ix] = True
    p0 = torch.tensor(pos0 + [0] * 6, dtype=torch.int32, device=dev)
    tcode = sx_code(dt)
    if c["pshift"]:
        st = lib.sx_rope_kv_append_f32_paged(qkv.data_ptr(), kc.ptr(), vc.ptr(), int(c["v16"]), cb.data_ptr(), sb.data_ptr(), p0.data_ptr(),
                                             tab.data_ptr(), G, T, H, D, Tmax, c["pshift"], n_pages, page_stride, tcode, stream())
    elif c["v16"]:
        st = lib.sx_rope_kv_append_f32_v16(qkv.data_ptr(), kc.ptr(), vc.ptr(), cb.data_ptr(), sb.data_ptr(), p0.data_ptr(), G, T, H, D, Tmax, seq, tcode, stream())
    else:
        st = lib.sx_rope_kv_append_f32(qkv.data_ptr(), kc.ptr(), vc.ptr(), cb.data_ptr(), sb.data_ptr(), p0.data_ptr(), G, T, H, D, Tmax, seq, tcode, stream())
    _lib.check(st, c["id"])
    torch.cuda.synchronize()
    kc.check(c["id"] + " (k cache)")
    vc.check(c["id"] + " (v cache)")
    assert bool(torch.isnan(qkv[G * T * 3 * cols:]).all()), f"{c['id']}: written behind the qkv rows"
    y = qkv[:G * T * 3 * cols].view(G, T, 3, H, D)
    assert same_bits(y[:, :, 1:], x[:, :, 1:]), f"{c['id']}: the k / v columns of qkv changed"
    c64, s64 = cos[pt].to(dt).double()[:, :, None], sin[pt].to(dt).double()[:, :, None]
    key = kernel_of_rope(c) + (c["dt"],)
    qr, kr = rot64(x[:, :, 0].double(), c64, s64), rot64(x[:, :, 1].double(), c64, s64)
    worst = held([key], y[:, :, 0].double(), qr, 2.0 * U32 * rotmag(x[:, :, 0].double(), c64, s64) + 2.0 ** -126, c["id"] + " (q)")
    gk, gv = kr.clone(), (x[:, :, 2].to(vdt)).clone()
    for g in range(G):
        for t in range(T):
            if bool(writes[g, t]):
                ix = off[g, :, int(pt[g, t])][:, None] + ar(D)
                gk[g, t], gv[g, t] = kc.body[ix].double(), vc.body[ix]
    worst = max(worst, held([key], gk, kr, 2.0 * U32 * rotmag(x[:, :, 1].double(), c64, s64) + 2.0 ** -126, c["id"] + " (appended k)"))
    assert same_bits(gv, x[:, :, 2].to(vdt)), f"{c['id']}: the appended v rows are not the {'rounded ' if c['v16'] else ''}v rows"
    return worst


@pytest.mark.parametrize("D", ROPE_D)
@pytest.mark.parametrize("dt", list(DTYPES))
@stops_on_gpu_fault
def test_rope_kv_append_vs_fp64(dev, dt, D):
    """Every T, position pattern, fp32 / 16-bit v and (D = 128) page size at one head_dim and table dtype."""
    worst = max(run_rope(c, dev) for c in ROPE if c["dt"] == dt and c["D"] == D)
    print(f"rope_kv_append {dt} D {D}: worst |diff| / bound {worst:.3f}")


# ----------------------------------------------------------------------------------------------------------------------------
# 3. sx_rmsnorm_planes
# ----------------------------------------------------------------------------------------------------------------------------
RMS_COLS = (8, 2040, 2048, 2056, 4104, 5120)
RMS_ROWS = (1, 16, 17, 32)
RMS_MODES = ("y32", "planes", "both")
RMS = [dict(id=f"rms-{dt}-{rows}x{cols}-{mode}{'-tiled' if tiled else ''}", dt=dt, rows=rows, cols=cols, mode=mode, tiled=tiled)
       for dt in DTYPES for cols in RMS_COLS for rows in RMS_ROWS for mode in RMS_MODES for tiled in ((False, True) if cols % 32 == 0 and mode != "y32" else (False,))]


def kernel_of_rms(c):
    return ("rmsnorm_planes_kernel", c["dt"].upper())


def split_ref(x, dt):
    """split1: hi = rn16(clamp(x)) (fp16 only: +-65504), lo = rn16(x - hi), the subtraction in fp32"""
    hi = (x.clamp(-65504.0, 65504.0) if dt == F16 else x).to(dt)
    return hi, (x - hi.float()).to(dt)


def rms_rows(rows, cols, g_, dev):
    """row r is of kind r % 3: N(0, 3^2); one massive channel (3000 among N(0, 1)); N(0, 1) scaled by 2^-20"""
    x = torch.randn(rows, cols, device=dev, generator=g_)
    kind = torch.arange(rows, device=dev)[:, None] % 3
    x = torch.where(kind == 0, 3.0 * x, torch.where(kind == 1, x, x * 2.0 ** -20))
    x[1::3, 5 % cols] = 3000.0
    return x


def run_rms(c, dev):
    from seedx_amd import _lib
    lib = _lib.load()
    dt = DTYPES[c["dt"]]
    rows, cols = c["rows"], c["cols"]
    g_ = gen_of(f"rms-{rows}x{cols}", dev)
    x = rms_rows(rows, cols, g_, dev)
    gamma = 1.0 + 0.1 * torch.randn(cols, device=dev, generator=g_)
    eps = 1e-5
    xb, gb = nanbuf(rows * cols + 256, F32, dev), nanbuf(cols + 64, F32, dev)
    xb[:rows * cols], gb[:cols] = x.reshape(-1), gamma
    yb = pb = None
    if c["mode"] != "planes":
        yb = GBuf(rows * cols, F32, dev)
        yb.allow()[:] = True
    if c["mode"] != "y32":
        if c["tiled"]:
            pb = TiledOut(2, rows, cols, dt, dev)
        else:
            pb = GBuf(rows * 2 * cols, dt, dev)
            pb.allow()[:] = True
    st = lib.sx_rmsnorm_planes(xb.data_ptr(), gb.data_ptr(), yb.ptr() if yb else None, pb.ptr() if pb else None, rows, cols, eps,
                               sx_code(dt) | (_lib.SX_TILED16 if c["tiled"] else 0), stream())
    _lib.check(st, c["id"])
    torch.cuda.synchronize()
    x64 = x.double()
    ref = gamma.double() * (x64 * torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + eps))
    Cc = 2.0 * -(-cols // 2048) + 11.0
    worst, y32 = 0.0, None
    if yb is not None:
        yb.check(c["id"] + " (y32)")
        y32 = yb.body.view(rows, cols)
        worst = held([kernel_of_rms(c) + ("y32",)], y32.double(), ref, (1.0 + Cc) * U32 * ref.abs() + 2.0 ** -126, c["id"] + " (y32)")
    if pb is not None:
        pb.check(c["id"] + " (planes)")
        hi, lo = pb.planes() if c["tiled"] else (pb.body.view(rows, 2, cols)[:, 0], pb.body.view(rows, 2, cols)[:, 1])
        assert bool(torch.isfinite(hi.float()).all() & torch.isfinite(lo.float()).all()), f"{c['id']}: non-finite planes"
        worst = max(worst, held([kernel_of_rms(c) + (c["dt"],)], hi.double() + lo.double(), ref, U_PL[dt] * ref.abs() + FLOOR[dt] + Cc * U32 * ref.abs(),
                                c["id"] + " (planes)"))
        if y32 is not None:
            wh, wl = split_ref(y32, dt)
            assert same_bits(hi.contiguous(), wh) and same_bits(lo.contiguous(), wl), f"{c['id']}: the planes are not the split of y32"
    return worst


@pytest.mark.parametrize("cols", RMS_COLS)
@pytest.mark.parametrize("dt", list(DTYPES))
@stops_on_gpu_fault
def test_rmsnorm_planes_vs_fp64(dev, dt, cols):
    """rows 1, 16, 17, 32 x {y32 only, planes only, both} x {row-major, SX_TILED16 where cols % 32 == 0} at one width."""
    worst = max(run_rms(c, dev) for c in RMS if c["dt"] == dt and c["cols"] == cols)
    print(f"rmsnorm_planes {dt} cols {cols}: worst |diff| / bound {worst:.3f}")


# ----------------------------------------------------------------------------------------------------------------------------
# 4. sx_split16 (exact)
# ----------------------------------------------------------------------------------------------------------------------------
SPLIT_ROWS_TILED = (1, 15, 16, 17, 31, 32)
SPLIT_ROWS_RM = (33, 300)
SPLIT_COLS = (8, 32, 40, 2080)
SPLIT16 = [dict(id=f"split16-{dt}-{rows}x{cols}{'-tiled' if tiled else ''}", dt=dt, rows=rows, cols=cols, tiled=tiled)
           for dt in DTYPES for rows in SPLIT_ROWS_TILED + SPLIT_ROWS_RM for cols in SPLIT_COLS
           for tiled in ((False, True) if rows <= 32 and cols % 32 == 0 else (False,))]
BELOW_65520 = 65519.99609375                                      # the largest fp32 below 65520 = 65504 + half an fp16 ulp
F16_EDGES = (65504.0, -65504.0, BELOW_65520, 65520.0, -65520.0, 131008.0, -131008.0)
SPLIT_SPECIALS = F16_EDGES + (0.0, -0.0, 1.0 + 2.0 ** -20, -(3.0 + 2.0 ** -17), 2.0 ** -30, 2.0 ** -24, 6.0e-8, 2.0 ** 17 - 64.0)


def kernel_of_split16(c):
    return ("split16_kernel", c["dt"].upper())


def run_split16(c, dev):
    from seedx_amd import _lib
    lib = _lib.load()
    dt = DTYPES[c["dt"]]
    rows, cols = c["rows"], c["cols"]
    g_ = gen_of(f"split16-{rows}x{cols}", dev)
    mag = torch.exp2(torch.rand(rows, cols, device=dev, generator=g_) * 46.0 - 30.0)                # 2^-30 .. 2^16, times [1, 2) below
    x = mag * (1.0 + torch.rand(rows, cols, device=dev, generator=g_)) * torch.where(torch.rand(rows, cols, device=dev, generator=g_) < 0.5, -1.0, 1.0)
    sp = torch.tensor(SPLIT_SPECIALS, device=dev)
    flat = x.view(-1)
    at = (torch.arange(len(SPLIT_SPECIALS), device=dev) * 7) % flat.numel() if flat.numel() >= 7 * len(SPLIT_SPECIALS) else torch.arange(min(len(SPLIT_SPECIALS), flat.numel()), device=dev)
    flat[at] = sp[:at.numel()]
    ldx = cols + 8
    xb = nanbuf(rows * ldx + 256, F32, dev)
    xb[:rows * ldx].view(rows, ldx)[:, :cols] = x
    if c["tiled"]:
        pb = TiledOut(2, rows, cols, dt, dev)
    else:
        pb = GBuf(rows * 2 * cols, dt, dev)
        pb.allow()[:] = True
    st = lib.sx_split16(xb.data_ptr(), ldx, pb.ptr(), rows, cols, sx_code(dt) | (_lib.SX_TILED16 if c["tiled"] else 0), stream())
    _lib.check(st, c["id"])
    torch.cuda.synchronize()
    pb.check(c["id"])
    hi, lo = pb.planes() if c["tiled"] else (pb.body.view(rows, 2, cols)[:, 0], pb.body.view(rows, 2, cols)[:, 1])
    wh, wl = split_ref(x, dt)
    assert same_bits(hi.contiguous(), wh), f"{c['id']}: hi != rn16(clamp(x))"
    assert same_bits(lo.contiguous(), wl), f"{c['id']}: lo != rn16(x - hi)"
    # what the bits imply, stated on its own: inside 2 x 65504 the pair is finite and within u_pl of x (fp16 saturation edges included)
    rec = hi.double() + lo.double()
    if dt == F16:                                                 # between the edges a saturated hi leaves lo a 16-bit rounding of its own
        assert bool(torch.isfinite(rec[x.abs() <= 131008.0]).all()), f"{c['id']}: hi + lo is not finite inside 2 x 65504"
        inside = (x.abs() <= 65504.0) | torch.isin(x, sp[:len(F16_EDGES)])
    else:
        inside = torch.ones_like(x, dtype=torch.bool)
    err = (rec - x.double()).abs()[inside]
    assert bool((err <= U_PL[dt] * x.double().abs()[inside] + FLOOR[dt]).all()), f"{c['id']}: hi + lo is not within u_pl of x"
    z = x == 0
    assert bool((hi.float()[z] == 0).all() & (lo.float()[z] == 0).all())
    WORST[kernel_of_split16(c) + (c["dt"],)] = max(WORST.get(kernel_of_split16(c) + (c["dt"],), 0.0), float((err / (U_PL[dt] * x.double().abs()[inside] + FLOOR[dt])).max()))


@pytest.mark.parametrize("rows", SPLIT_ROWS_TILED + SPLIT_ROWS_RM)
@pytest.mark.parametrize("dt", list(DTYPES))
@stops_on_gpu_fault
def test_split16_bits(dev, dt, rows):
    """Every width and layout at one row count, ldx = cols + 8 with NaN in the gap."""
    for c in SPLIT16:
        if c["dt"] == dt and c["rows"] == rows:
            run_split16(c, dev)


# ----------------------------------------------------------------------------------------------------------------------------
# the source, for tests/test_cpu_suite.py
# ----------------------------------------------------------------------------------------------------------------------------
COVERED_ELSEWHERE = {"rope_kv_q8_kernel": "tests/test_fp8_kv_gpu.py"}


def source_kernels():
    """Every instantiation that the host code of precise.hip launches, as the keys of kernel_of_*: a set per kernel. Asserts that every
    hipLaunchKernelGGL of the file is one of the forms parsed here, so a launch added later is not passed over."""
    src = open(PRECISE_HIP).read()
    tf = lambda s: s == "true"
    attn = set()
    for tt, qb, dc, v16 in re.findall(r"hipLaunchKernelGGL\(\(?attn_f32_kernel<(BF16|F16), (\d), (\d)(, true)?>\)?, (?:grid|dim3)", src):
        attn.add(("attn_f32_kernel", tt, int(qb), int(dc), bool(v16), False, 0, False))
    n_explicit = len(attn)
    assert "#define SX_SPLIT_GO(TT, V16) hipLaunchKernelGGL((attn_f32_kernel<TT, 1, 1, V16, true>)" in src
    assert "#define SX_SPLIT8_GO(TT, KV8) hipLaunchKernelGGL((attn_f32_kernel<TT, 1, 1, false, true, KV8>)" in src
    assert "#define SX_KV8_GO(TT, QB, KV8) hipLaunchKernelGGL((attn_f32_kernel<TT, QB, 1, false, false, KV8>)" in src
    for tt, v16 in re.findall(r"SX_SPLIT_GO\((BF16|F16), (true|false)\)", src):
        attn.add(("attn_f32_kernel", tt, 1, 1, tf(v16), True, 0, False))
    for tt, kv8 in re.findall(r"SX_SPLIT8_GO\((BF16|F16), (\d)\)", src):
        attn.add(("attn_f32_kernel", tt, 1, 1, False, True, int(kv8), False))
    for tt, qb, kv8 in re.findall(r"SX_KV8_GO\((BF16|F16), (\d), (\d)\)", src):
        attn.add(("attn_f32_kernel", tt, int(qb), 1, False, False, int(kv8), False))
    paged_calls = {(tt, tf(v16)) for tt, v16 in re.findall(r"attn_f32_paged_launch<(BF16|F16), (true|false)>\(a, p, mfma, stream\)", src)}
    paged_body = re.findall(r"attn_f32_kernel<TT, (\d), 1, V16, (true|false), 0, true>", src)
    for tt, v16 in paged_calls:
        for qb, split in paged_body:
            attn.add(("attn_f32_kernel", tt, int(qb), 1, v16, tf(split), 0, True))
    mfma = {("attn_f32_mfma_kernel", tt, tf(v16), bool(kv8), False) for tt, v16, kv8 in re.findall(r"attn_f32_mfma_kernel<(BF16|F16), (true|false)(, true)?>\)", src)}
    n_mfma_explicit = len(mfma)
    assert src.count("(attn_f32_mfma_kernel<TT, V16, false, true>)") == 1
    mfma |= {("attn_f32_mfma_kernel", tt, v16, False, True) for tt, v16 in paged_calls}
    assert "#define SX_VERIFY_GO(TT, TQ, V16) hipLaunchKernelGGL((attn_f32_verify_kernel<TT, TQ, V16>)" in src
    tqs = [int(t) for t in re.findall(r"SX_VERIFY_GO\(TT, (\d), V16\)", src)]
    verify = {("attn_f32_verify_kernel", tt, tq, tf(v16)) for tt, v16 in re.findall(r"SX_VERIFY_TQ\((BF16|F16), (true|false)\);", src) for tq in tqs}
    combine = {("attn_f32_combine_kernel", tt) for tt in re.findall(r"hipLaunchKernelGGL\(attn_f32_combine_kernel<(BF16|F16)>", src)}
    assert "hipLaunchKernelGGL((rope_kv_f32_kernel<TT, V16>)" in src and "hipLaunchKernelGGL((rope_kv_f32_paged_kernel<TT, V16>)" in src
    rope = {("rope_kv_f32_kernel", tt, tf(v)) for tt, v in re.findall(r"SX_ROPE_GO\((BF16|F16), (true|false)\)", src)}
    rope_paged = {("rope_kv_f32_paged_kernel", tt, tf(v)) for tt, v in re.findall(r"SX_ROPE_PAGED_GO\((BF16|F16), (true|false)\)", src)}
    rms = {("rmsnorm_planes_kernel", tt) for tt in re.findall(r"hipLaunchKernelGGL\(rmsnorm_planes_kernel<(BF16|F16)>", src)}
    split16 = {("split16_kernel", tt) for tt in re.findall(r"hipLaunchKernelGGL\(split16_kernel<(BF16|F16)>", src)}
    # every launch statement of the file is one of: an explicit attn_f32_kernel / mfma launch, the 4 paged kernels + 1 paged mfma of
    # attn_f32_paged_launch, the macro bodies (split, split8, kv8, verify, rope, rope paged, q8), the combine launches, rmsnorm, split16
    n_launch = src.count("hipLaunchKernelGGL(")
    n_combine = len(re.findall(r"hipLaunchKernelGGL\(attn_f32_combine_kernel<", src))
    assert "hipLaunchKernelGGL((rope_kv_q8_kernel<TT, EM>)" in src and set(COVERED_ELSEWHERE) == {"rope_kv_q8_kernel"}
    assert n_launch == n_explicit + n_mfma_explicit + len(paged_body) + 1 + 7 + n_combine + len(rms) + len(split16), \
        f"precise.hip has {n_launch} hipLaunchKernelGGL statements: one of them is not parsed by source_kernels"
    assert "chunk = ((kend + p.nsplit - 1) / p.nsplit + 15) & ~15;" in src, "split_chunk restates this line"
    assert "const bool mfma = g_attn_f32_mfma && a->causal && a->T > 8 && a->D == 128 && !tiled &&" in src, "is_mfma restates this line"
    assert "if (a->T <= 4) SX_VERIFY_GO(TT, 4, V16); else SX_VERIFY_GO(TT, 8, V16);" in src, "kernel_of_attn restates this line"
    assert "for (int c8 = tid * 8; c8 < cols; c8 += 2048)" in open(os.path.join(os.path.dirname(PRECISE_HIP), "precise_rows.h")).read(), "RMS_COLS sit around this stride"
    return dict(attn=attn, mfma=mfma, verify=verify, combine=combine, rope=rope, rope_paged=rope_paged, rms=rms, split16=split16)


def test_print_worst_ratio_per_instantiation(dev):
    """Not a check of its own: the worst |diff| / bound of the cases above per instantiation and dtype (run the file as a whole)."""
    for key, w in sorted(WORST.items(), key=lambda kv: str(kv[0])):
        print(f"worst |diff| / bound  {str(key):90s} {w:.4f}")
    assert all(w <= 1.0 for w in WORST.values())
