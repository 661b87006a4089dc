"""sx_gemv and the decode attention against fp64: every instantiation of gemm_skinny_kernel and gemv_kernel that sx_gemv launches
(csrc/decode.hip g_skinny_table / g_gemv_table), both 16-bit dtypes, 16-bit and FP8 weight tiles, at the k-slice lengths where the peeled rounds
of the skinny kernel differ; and sx_attn_decode_b / sx_attn_decode_fused at the shapes where the split and the group combine differ.

Each GEMV case drives sx_gemv through _lib.GemvArgs directly and checks
  * every output element against an fp64 reference built from the SAME 16-bit operands (FP8: decode(code) * scale), with the bound of
    tests/test_gemm_matrix_gpu.py (`reference` below; the constants U32, C_ACC, C_EP, LIP are that file's own), plus the relative-L2
    TOL as a second assert;
  * the outputs of the RMSNorm fold: x16_out bit for bit as rn16(y * gamma) of the stored fp32 y (one plane or two), row_ssq_out[m][p]
    against the fp64 sum of squares of the stored y over workgroup p's columns;
  * that no read goes past a logical input: x (row-major and tiled), W, w_scale, residual, x16_gamma and row_ssq_in are leading views of
    NaN-filled buffers, and the padding rows of a tiled x (rows >= M of every 16-row block of every plane) hold NaN bits;
  * that nothing outside the documented extent is written: y, x16_out, row_ssq_out and the workspace sit inside guard-filled buffers,
    rows >= M of 16-bit tiled outputs are pre-filled with the guard pattern; extents are rows < M of y and of the tiles,
    16 * ceil(M / 16) rows of row_ssq_out and 16384 + S * 16 * MB * N * 4 bytes of workspace; the counters are zero afterwards;
  * that a second identical launch gives the same bits, that a launch with the rows of x (and of the residual / row_ssq_in) permuted
    gives the same rows permuted bit for bit (a request's result does not depend on its slot), and that an FP8 case equals, bit for
    bit, the 16-bit launch on the dequantised weights at the same split factor.

K values: a wave of the skinny kernel walks len = ks1 - ks0 k-steps (ks = sl * nks / nsl, nks = K / 64, nsl = 4 waves x S splits) as
full = len / U double-buffered rounds plus rem = len % U; the code behind the pipelined loop branches on full in {0, 1, 2, odd >= 3,
even >= 4} and on rem. NKS[U] makes the four waves' (full, rem) cover every such class with every rem in 0 .. U-1 (a wave without any
k-step, full = rem = 0, needs the forced split-K cases); tests/test_cpu_suite.py checks that without a GPU, together with the case
table against the sources.

The hooks sx_gemv_tune / sx_gemv_force_valu are process-global: every launch that sets them restores (1, 0), (2, 0), (3, 1) and
force_valu(0) on its way out, whatever happens in between (Hooks); test_hook_defaults_restored then asks the library itself, with
launches and sx_gemv_plan queries that do not touch the hooks. kernel_of / plan_of restate sx_gemv's dispatch plan by hand and never
ask the library; tests/test_cpu_suite.py holds sx_gemv_plan against them on the CPU, over the case table and a sweep.
"""
import ctypes as C
import math
import os
import re
import zlib

import pytest
import torch

from tests.test_gemm_matrix_gpu import (BF16, C_ACC, C_EP, DTYPES, F16, LIP, NAN16_GUARD, NAN32_GUARD, TOL, U32, _ibits, _nanbuf, _signed,
                                        act64, guarded, half_ulp)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECODE_HIP = os.path.join(ROOT, "seed-x_amd", "csrc", "decode.hip")

# ----------------------------------------------------------------------------------------------------------------------------
# the case table
# ----------------------------------------------------------------------------------------------------------------------------
# (R, U, TAIL, MB) of gemm_skinny_kernel<TT, R, 4, U, TAIL, MB, W8, W4>: the 14 rows of g_skinny_table
FAMILIES = ((1, 4, False, 1), (2, 4, False, 1), (2, 4, True, 1), (4, 2, False, 1),
            (1, 4, False, 2), (2, 2, False, 2), (2, 2, True, 2), (2, 4, False, 2), (2, 4, True, 2), (4, 1, False, 2),
            (1, 2, False, 4), (2, 1, False, 4), (2, 1, True, 4), (4, 1, False, 4))
VALU_MR = (1, 2, 4, 8)
# K / 64 per U: the four waves' lengths cover 1..4 (U = 1), 1..9 (U = 2), 1..19 (U = 4)
NKS = {1: (5, 13), 2: (5, 13, 21, 29, 33), 4: (5, 13, 21, 29, 37, 45, 53, 61, 69, 73)}
FULL_CLASSES = ("0", "1", "2", "odd>=3", "even>=4")
SSQ_DIM, SSQ_EPS = 4096, 1e-5                     # of every row_ssq_in
_DUMMY = C.create_string_buffer(64 + 16)          # plan_args: where the pointers of a host-only query point


def wave_rounds(nks, U, S=1):
    """(full, rem) of every wave of every split-K workgroup: the kernel's own k-slice formula."""
    nsl = 4 * S
    out = []
    for sl in range(nsl):
        ln = (sl + 1) * nks // nsl - sl * nks // nsl
        out.append((ln // U, ln % U))
    return out


def round_class(full, rem):
    return (FULL_CLASSES[full] if full <= 2 else FULL_CLASSES[3 if full % 2 else 4], rem)


def required_classes(U):
    """Every branch behind the pipelined loop: each class of full with each rem in 0 .. U-1, except the wave without k-steps."""
    return {(f, r) for f in FULL_CLASSES for r in range(U)} - {("0", 0)}


def case(cid, dt, **kw):
    c = dict(id=cid, dt=dt, M=5, N=32, K=320, glu=False, act=None, w_layout=0, w8=False, x_layout=0, planes=1, out="f32",
             out_planes=False, res=False, emit=False, gamma=False, ssq_in=False, S=0, var1=0, var3=1, fv=0, ws="full", fam=None)
    c.update(kw)
    return c


def n_blocks(c):
    """MB of the kernel a case runs on the MFMA path: x blocks per weight fragment."""
    return kernel_of(c)[4]


def mfma_ok(c):
    """The shapes the MFMA skinny kernel takes."""
    return (c["M"] >= 2 or c["planes"] == 2) and c["K"] % 64 == 0 and c["K"] >= 256 and c["N"] % 32 == 0


def kernel_of(c):
    """The kernel sx_gemv launches for a case — ('sk', R, U, TAIL, MB, W8) or ('valu', MR) — by the rules of its dispatch (mfma_ok,
    tail20, r2, r4, M > 16, planes2, g_skinny_var[1], g_skinny_var[3]). Written by hand and independent of the library:
    tests/test_cpu_suite.py holds sx_gemv_plan against it."""
    M, N = c["M"], c["N"]
    planes2 = c["planes"] == 2
    if mfma_ok(c) and (c["w_layout"] or c["x_layout"] or c["out"] == "tiled" or (c["fv"] != 1 and (M >= 5 or c["fv"] == 2))):
        tail20 = c["w_layout"] == 2
        r2 = not tail20 and (c["glu"] or N // 32 >= 256)
        r4 = r2 and c["var3"] > 0 and N % 64 == 0 and not c["emit"] and N // 64 >= (64 if c["var3"] == 2 else 200)
        big = M > 16
        if big and planes2 and r4:
            k = (4, 1, False, 4)
        elif big and planes2:
            k = (2, 1, True, 4) if tail20 else ((2, 1, False, 4) if r2 else (1, 2, False, 4))
        elif r4:
            k = (4, 1, False, 2) if (big or planes2) else (4, 2, False, 1)
        elif big or planes2:
            if c["var1"] == 1:
                k = (2, 4, True, 2) if tail20 else ((2, 4, False, 2) if r2 else (1, 4, False, 2))
            elif tail20 and c["var1"] == 2:
                k = (2, 4, True, 2)
            elif tail20:
                k = (2, 2, True, 2)
            else:
                k = (2, 2, False, 2) if r2 else (1, 4, False, 2)
        elif tail20:
            k = (2, 4, True, 1)
        else:
            k = (2, 4, False, 1) if r2 else (1, 4, False, 1)
        return ("sk",) + k + (c["w8"],)
    assert M <= 8 and not c["w_layout"] and not c["w8"] and not c["emit"] and not c["ssq_in"], c["id"]
    return ("valu", 1 if M == 1 else (2 if M == 2 else (4 if M <= 4 else 8)))


def plan_of(c, ws_bytes):
    """The launch of a case with `ws_bytes` of workspace under its hooks (var1, S = hook 2, var3, fv), as sx_gemv_plan reports it:
    (path, gx, S, R | MR, U, TAIL, MB), or None where sx_gemv refuses the case. By hand, like kernel_of, with the automatic split
    (K >= 8192, < 1024 workgroups, four double rounds left per wave, never on 20-row tiles) and the too-small-workspace fallback."""
    M, N, K = c["M"], c["N"], c["K"]
    tiles = c["w8"] or c.get("w4", False)
    mfma_only = c["w_layout"] or c["x_layout"] or c["out"] == "tiled"
    if ((c["glu"] and N % 32) or (c["planes"] == 2 and not c["x_layout"]) or (c["out_planes"] and not (c["out"] == "tiled" or c["emit"]))
            or (c["emit"] and (c["out"] != "f32" or c["glu"] or N % 32)) or (c["gamma"] and not c["emit"])
            or (c["w_layout"] == 2 and (c["glu"] or N % 20 or N % 32)) or ((mfma_only or tiles) and not mfma_ok(c)) or (tiles and not c["w_layout"])):
        return None
    if not (mfma_ok(c) and (mfma_only or (c["fv"] != 1 and (M >= 5 or c["fv"] == 2)))):
        return None if (M > 8 or c["emit"] or c["ssq_in"]) else (0, ((N + 1) // 2 + 3) // 4, 1, kernel_of(c)[1], 0, 0, 0)
    R, U, TAIL, MB = kernel_of(c)[1:5]
    gx = N // 20 if TAIL else N // (16 * R)
    S, forced = 1, c["S"]
    if ws_bytes and not (TAIL and forced <= 0):
        if forced > 0:
            S = forced
        elif forced == 0 and K >= 8192:
            while S < 8 and gx * S < 1024 and (K // 64) // (4 * S * 2) >= 4:
                S *= 2
        if S > 1 and (gx > 4096 or 16384 + S * 16 * MB * N * 4 > ws_bytes):
            S = 1
    return (1, gx, S, R, U, int(TAIL), MB)


def plan_args(c, ws_bytes=0, w_dtype=None):
    """sx_gemv_args of a case with every pointer it needs set to one 16-B aligned dummy address: for host-only sx_gemv_plan queries, and
    the scalar fields of a launch (which replaces the pointers). `w_dtype` overrides the case's weight format."""
    from seedx_amd import _lib
    a, base = _lib.GemvArgs(), (C.addressof(_DUMMY) + 15) & ~15
    a.x = a.W = a.y = base
    a.M, a.N, a.K = c["M"], c["N"], c["K"]
    a.dtype = _lib.SX_F16 if c["dt"] == "f16" else _lib.SX_BF16
    a.out_dtype = {"f32": _lib.SX_F32, "16": a.dtype, "tiled": a.dtype | _lib.SX_TILED16}[c["out"]]
    a.act = {None: _lib.SX_ACT_NONE, "gelu": _lib.SX_ACT_GELU, "silu": _lib.SX_ACT_SILU}[c["act"]]
    a.glu, a.w_layout, a.x_layout, a.x_planes, a.out_planes = int(c["glu"]), c["w_layout"], c["x_layout"], c["planes"], int(c["out_planes"])
    a.w_dtype = (_lib.SX_FP8_E4M3 if c["w8"] else _lib.SX_FP4_E2M1 if c.get("w4") else 0) if w_dtype is None else w_dtype
    if c["ssq_in"]:
        a.ssq_in_parts, a.ssq_dim, a.ssq_eps = 64, SSQ_DIM, SSQ_EPS
    for on, field in ((a.w_dtype == _lib.SX_FP8_E4M3, "w_scale"), (a.w_dtype == _lib.SX_FP4_E2M1, "w_block_scale"), (c["res"], "residual"),
                      (c["gamma"], "x16_gamma"), (c["ssq_in"], "row_ssq_in"), (c["emit"], "x16_out"), (c["emit"], "row_ssq_out"),
                      (ws_bytes, "workspace"), (ws_bytes, "workspace_bytes")):
        if on:
            setattr(a, field, ws_bytes if field == "workspace_bytes" else base)
    return a


def lib_plan(lib, a):
    """sx_gemv_plan's answer for `a` as a tuple of its eight fields, or None where the library refuses the arguments."""
    plan = (C.c_int32 * 8)()
    return tuple(plan) if lib.sx_gemv_plan(C.byref(a), plan) == 0 else None


def source_kernels():
    """The instantiations in the sources: ({(R, U, TAIL, MB)} of g_skinny_table, {(TT, W8, W4)} of its row macro, {MR}, {TT} of
    g_gemv_table). Every gemm_skinny_kernel< / gemv_kernel< of the host section is one of them."""
    src = open(DECODE_HIP).read()
    host = src[src.index("#define ST "):]
    body = host[host.index("#define SX_SK_ROW("):host.index("#undef SX_SK_ROW")]
    macro, table = body[:body.index("g_skinny_table")], body[body.index("g_skinny_table"):]
    rows = re.findall(r"SX_SK_ROW\((\d), (\d), (true|false), (\d)\)", table)
    sk = {(int(r), int(u), t == "true", int(mb)) for r, u, t, mb in rows}
    assert len(rows) == len(sk) == table.count("SX_SK_ROW("), "a family is listed twice, or a row is not of the form (R, U, TAIL, MB)"
    inst = re.findall(r"gemm_skinny_kernel<(BF16|F16), R, 4, U, TAIL, MB, (true|false), (true|false)>", macro)
    assert len(host.split("gemm_skinny_kernel<")) - 1 == len(inst) == len(set(inst))
    sk_tt = {(tt, w8 == "true", w4 == "true") for tt, w8, w4 in inst}
    valu = re.findall(r"gemv_kernel<(BF16|F16), (\d)>", host)
    assert len(host.split("gemv_kernel<")) - 1 == len(valu) == len(set(valu)) == len({t for t, _ in valu}) * len({m for _, m in valu})
    return sk, sk_tt, {int(m) for _, m in valu}, {t for t, _ in valu}


def _skinny(fam, i, nks, dt, w8, tag="", nonglu_wide=False, **kw):
    """Case number i of a family at K = 64 nks: M at and around the block edges, the smallest N that reaches the kernel, and one of
    the epilogue flavours — all cycled with i. M has period 3 (MB = 2: 6, with the plane count); N moves on by one more step every
    third case (period 9; TAIL: period 2), so every block-edge M meets more than one N; the flavours have period 4 or 5."""
    R, U, TAIL, MB = fam
    c = dict(K=64 * nks, w8=w8, fam=fam)
    ni = (i + i // 3) % 3
    if MB == 1:
        c.update(planes=1, M=(5, 15, 16)[i % 3])
    elif MB == 2:
        c.update(dict(planes=2, M=(1, 15, 16)[(i // 2) % 3]) if i % 2 == 0 else dict(planes=1, M=(17, 31, 32)[(i // 2) % 3]))
    else:
        c.update(planes=2, M=(17, 31, 32)[i % 3])
    if TAIL:
        c.update(N=(160, 640)[i % 2], glu=False, w_layout=2)
    elif R == 1:
        c.update(N=(32, 64, 96)[ni], glu=False)
    elif R == 2:
        c.update(dict(N=8192, glu=False) if nonglu_wide else dict(N=(64, 128, 96)[ni], glu=True))
    else:
        c.update(dict(N=4096, glu=True, var3=2) if i % 2 == 0 else dict(N=8192, glu=False, var3=2))
    if not TAIL:
        c["w_layout"] = 1 if w8 else (0, 1)[i % 2]
    c["x_layout"] = 1 if c["planes"] == 2 else (1, 0)[(i // 2) % 2]
    if fam == (2, 4, True, 2):
        c["var1"] = (2, 1)[i % 2]
    elif fam == (2, 4, False, 2):
        c["var1"] = 1
    elif fam == (1, 4, False, 2):
        c["var1"] = (0, 1)[i % 2]
    n_out = c["N"] // 2 if c["glu"] else c["N"]
    if c["glu"]:
        fl = i % 4
        if fl == 0:
            c.update(out="f32", act="silu")
        elif fl == 1:
            c.update(out="16", act="gelu", res=True)
        elif fl == 2:
            c.update(act="silu", out="tiled" if n_out % 32 == 0 else "16", out_planes=n_out % 32 == 0 and i % 8 == 2)
        else:
            c.update(out="f32", act="silu", ssq_in=True, res=True)
    else:
        fl = (0, 1, 2, 4)[i % 4] if R == 4 else i % 5            # the 64-row workgroups have no RMSNorm-fold producer
        if fl == 0:
            c.update(out="f32", res=True)
        elif fl == 1:
            c.update(out="16", act="silu")
        elif fl == 2:
            c.update(out="tiled", out_planes=i % 4 == 2)
        elif fl == 3:
            c.update(out="f32", res=True, emit=True, gamma=i % 2 == 1, out_planes=i % 4 >= 2)
        else:
            c.update(out="f32", act="gelu", ssq_in=True)
    c.update(kw)
    c = case("", dt, **c)
    flav = "-".join(filter(None, [c["out"], c["act"], "glu" if c["glu"] else "", "res" if c["res"] else "", "emit" if c["emit"] else "",
                                  "gamma" if c["gamma"] else "", "op2" if c["out_planes"] else "", "ssqin" if c["ssq_in"] else ""]))
    cid = (f"sk{R}{U}{'T' if TAIL else 'F'}{MB}-{dt}-{'w8' if w8 else 'w16'}-K{c['K']}-M{c['M']}p{c['planes']}-N{c['N']}-wl{c['w_layout']}"
           f"xl{c['x_layout']}-{flav}{tag}")
    c["id"] = cid
    return c


SPLIT_FAMILIES = ((1, 4, False, 1), (2, 4, False, 1), (2, 4, True, 1), (1, 4, False, 2), (2, 2, False, 2), (2, 2, True, 2),
                  (1, 2, False, 4), (2, 1, False, 4), (2, 1, True, 4))
SHORT_WS_FAMILIES = ((1, 4, False, 1), (2, 2, False, 2), (2, 1, False, 4))        # one per MB value


def skinny_cases():
    out = []
    for dt in DTYPES:
        for w8 in (False, True):
            for fam in FAMILIES:
                R, U, TAIL, MB = fam
                ks = NKS[U]
                n = len(ks) * -(-6 // len(ks))                 # at least 6 cases per family: every M of its list, every flavour
                for i in range(n):
                    out.append(_skinny(fam, i, ks[(i + i // len(ks)) % len(ks)], dt, w8))
                if R == 2 and not TAIL:                        # R = 2 without GLU needs N / 32 >= 256: two short K values
                    for i, nks in ((3, 5), (4, 13)):
                        out.append(_skinny(fam, i, nks, dt, w8, nonglu_wide=True))
            # forced split-K at ragged K: nks = 5 with S = 2 leaves waves without any k-step
            j = 0
            for fam in SPLIT_FAMILIES:
                for S, nks in ((2, 5), (8, 21), (2, 13), (8, 5)):
                    out.append(_skinny(fam, j, nks, dt, w8, tag=f"-S{S}", S=S))
                    j += 1
            # a workspace one byte below the host's threshold: no split, nothing written past workspace_bytes
            for j, fam in enumerate(SHORT_WS_FAMILIES):
                out.append(_skinny(fam, 2 * j, 13, dt, w8, tag="-S2-shortws", S=2, ws="short"))
    return out


def valu_cases():
    """gemv_kernel: K % 64 != 0 (8, 264, 520), odd N (the last wave has no second row), GLU at N = 32, every MR with M < MR inside."""
    out = []
    for dt in DTYPES:
        i = 0
        for M in (1, 2, 3, 4, 5, 7, 8):
            for K in (8, 264, 520):
                for N, glu in ((131, False), (1001, False), (32, True)):
                    kw = [dict(out="f32", res=True), dict(out="16", act="silu"), dict(out="f32", act="gelu"), dict(out="16", res=True)][i % 4]
                    if glu:
                        kw["act"] = kw.get("act") or "silu"
                    out.append(case(f"valu-{dt}-M{M}-K{K}-N{N}{'-glu' if glu else ''}-{kw['out']}-{kw.get('act') or 'none'}{'-res' if kw.get('res') else ''}",
                                    dt, M=M, N=N, K=K, glu=glu, **kw))
                    i += 1
    return out


def both_paths_cases():
    """Shapes where the VALU and the MFMA kernel are both legal (2 <= M <= 8, row-major operands, K % 64 == 0, N % 32 == 0)."""
    out = []
    for dt in DTYPES:
        for i, (M, K, N, glu) in enumerate(((2, 256, 96, False), (3, 320, 64, True), (4, 832, 160, False), (5, 320, 128, True),
                                            (7, 832, 96, False), (8, 256, 64, False))):
            kw = [dict(out="f32", res=True), dict(out="16", act="silu")][i % 2]
            if glu:
                kw["act"] = "silu"
            out.append(case(f"both-{dt}-M{M}-K{K}-N{N}{'-glu' if glu else ''}-{kw['out']}", dt, M=M, N=N, K=K, glu=glu, **kw))
    return out


SKINNY = skinny_cases()
VALU = valu_cases()
BOTH = both_paths_cases()
WORST = {}               # (kernel, dtype) -> worst |diff| / bound seen
WORST32 = {}             # the same over the fp32 outputs alone, where the output rounding is 2^-8 or less of the 16-bit one


# ----------------------------------------------------------------------------------------------------------------------------
# buffers
# ----------------------------------------------------------------------------------------------------------------------------
class GBuf:
    """`n` elements inside a buffer filled with the guard NaN pattern (`before` elements in front, `after` behind). `allowed` marks what
    a launch may write; everything else must be bit-unchanged afterwards."""

    def __init__(self, n, dtype, dev, before=64, after=512):
        self.dtype, self.n, self.before = dtype, n, before
        self.bits = NAN16_GUARD if dtype in (F16, BF16) else NAN32_GUARD
        self.buf = _nanbuf(before + n + after, dtype, dev, self.bits)
        self.body = self.buf[before:before + n]
        self.allowed = torch.zeros(self.buf.numel(), dtype=torch.bool, device=dev)

    def allow(self):
        return self.allowed[self.before:self.before + self.n]

    def ptr(self):
        return self.body.data_ptr()

    def check(self, what):
        bad = (self.buf.view(_ibits(self.dtype)) != _signed(self.bits, self.dtype)) & ~self.allowed
        nbad = int(bad.sum())
        assert nbad == 0, f"{what}: {nbad} elements outside the documented extent were written; first at element " \
                          f"{int(bad.nonzero()[0, 0]) - self.before} of {self.n}"


def tile_rows(planes, M, cols, dtype, dev):
    """[M, cols] 16-bit matrices (one per plane) as operand tiles [planes][row blocks][cols/32][16][32] at the head of a NaN-filled
    buffer: the padding rows of every block of every plane and 256 elements behind the tiles hold NaN bits."""
    RB, P = (M + 15) // 16, len(planes)
    n = P * RB * cols * 16
    buf = _nanbuf(n + 256, dtype, dev)
    t = buf[:n].view(P, RB, cols // 32, 16, 32)
    for p, xp in enumerate(planes):
        for b in range(RB):
            rows = xp[16 * b:min(M, 16 * b + 16)]
            t[p, b, :, :rows.shape[0]] = rows.reshape(rows.shape[0], cols // 32, 32).permute(1, 0, 2)
    return buf


class TiledOut(GBuf):
    """A 16-bit tiled output [planes][row blocks][cols/32][16][32] inside a guard buffer, rows >= M of every block pre-filled with the
    guard pattern and not writable."""

    def __init__(self, P, M, cols, dtype, dev):
        self.P, self.M, self.cols, self.RB = P, M, cols, (M + 15) // 16
        super().__init__(P * self.RB * cols * 16, dtype, dev)
        ok = self.allow().view(P, self.RB, cols // 32, 16, 32)
        for b in range(self.RB):
            ok[:, b, :, :min(16, M - 16 * b)] = True

    def planes(self):
        """[planes, M, cols]"""
        t = self.body.view(self.P, self.RB, self.cols // 32, 16, 32).permute(0, 1, 3, 2, 4).reshape(self.P, self.RB * 16, self.cols)
        return t[:, :self.M].contiguous()


class Hooks:
    """The process-global sx_gemv hooks of one launch; always restored to their defaults."""

    def __init__(self, lib, c):
        self.lib, self.c = lib, c

    def __enter__(self):
        c = self.c
        try:
            for key, value in ((1, c["var1"]), (2, c["S"]), (3, c["var3"])):
                assert self.lib.sx_gemv_tune(key, value) == 0, f"sx_gemv_tune({key}, {value}) refused"
            assert self.lib.sx_gemv_force_valu(c["fv"]) == 0
        except BaseException:            # __exit__ does not run when __enter__ raises: a hook set before the failure must not stay
            restore_defaults(self.lib)
            raise

    def __exit__(self, *exc):
        restore_defaults(self.lib)
        return False


def restore_defaults(lib):
    lib.sx_gemv_tune(1, 0)
    lib.sx_gemv_tune(2, 0)
    lib.sx_gemv_tune(3, 1)
    lib.sx_gemv_force_valu(0)


def make_inputs(c, dev):
    """Random operands of a case (logical values; the device buffers with their NaN padding are built per launch)."""
    from seedx_amd import quant
    dtype = DTYPES[c["dt"]]
    gen = torch.Generator(device=dev).manual_seed(zlib.crc32(c["id"].encode()))
    M, N, K = c["M"], c["N"], c["K"]
    n_out = N // 2 if c["glu"] else N
    RB = (M + 15) // 16
    I = dict(dtype=dtype, n_out=n_out, RB=RB)
    x32 = torch.randn(M, K, device=dev, generator=gen)
    hi = x32.to(dtype)
    I["xs"] = [hi, (x32 - hi.float()).to(dtype)] if c["planes"] == 2 else [hi]       # [hi, lo] as sx_split16 writes them
    W = (torch.randn(N, K, device=dev, generator=gen) * K ** -0.5).to(dtype)
    if c["w8"]:
        I["codes"], I["scale"] = quant.quantize_rows(W)
        assert not bool(((I["codes"] & 0x7f) == 0x7f).any())
        I["W64"] = quant.decode_table(dev).double()[I["codes"].long()] * I["scale"].double()[:, None]
        I["W16"] = quant.dequantize_rows(I["codes"], I["scale"], dtype)
        assert torch.equal(I["W16"].double(), I["W64"]), "the 16-bit twin must hold decode(code) * scale exactly"
    else:
        I["W16"], I["W64"] = W, W.double()
    if c["res"]:
        I["res"] = torch.randn(M, n_out, device=dev, generator=gen)
    if c["gamma"]:
        I["gamma"] = (1.0 + 0.5 * torch.randn(N, device=dev, generator=gen)).abs().clamp_min(0.2)
    if c["ssq_in"]:
        I["ssq_dim"], I["ssq_eps"] = SSQ_DIM, SSQ_EPS
        I["ssq"] = (torch.rand(16 * RB, 64, device=dev, generator=gen) * 1.5 + 0.25) * (I["ssq_dim"] / 64.0)
    return I


def _nan_lead(t, pad=256):
    """t (any shape, contiguous order) at the head of a NaN-filled buffer of its dtype."""
    buf = _nanbuf(t.numel() + pad, t.dtype, t.device)
    buf[:t.numel()] = t.reshape(-1)
    return buf


def weight_buffer(c, I, w8, dev):
    from seedx_amd import ops
    if w8:
        tiles = ops.pack_decode_tiles20_fp8(I["codes"]) if c["w_layout"] == 2 else ops.pack_decode_tiles_fp8(I["codes"])
        buf = torch.full((tiles.numel() + 256,), 0x7f, dtype=torch.uint8, device=dev)              # 0x7f: the e4m3 NaN code
        buf[:tiles.numel()] = tiles.reshape(-1)
        return buf
    w = I["W16"]
    w = ops.pack_decode_tiles(w) if c["w_layout"] == 1 else (ops.pack_decode_tiles20(w) if c["w_layout"] == 2 else w)
    return _nan_lead(w)


def ws_extent(c, S):
    return 16384 + S * 16 * n_blocks(c) * c["N"] * 4


def launch(lib, c, I, dev, perm=None, w8=None, ws_S=None, hooks=True):
    """One sx_gemv launch into fresh guard buffers; `perm` permutes the rows of x, residual and row_ssq_in; `w8` overrides the
    case's weight format (the 16-bit twin of an FP8 case); `ws_S` sizes the workspace for another split factor than the forced one; `hooks=False` launches
    without touching the process-global hooks (the case's var1 / S / var3 / fv are then not applied: the library decides with whatever
    is set). Returns the outputs and their guard buffers."""
    from seedx_amd import _lib
    dtype, n_out, RB = I["dtype"], I["n_out"], I["RB"]
    M, N, K = c["M"], c["N"], c["K"]
    w8 = c["w8"] if w8 is None else w8
    rows = (lambda t: t) if perm is None else (lambda t: t[perm].contiguous())
    keep = {}
    a = plan_args(c, w_dtype=_lib.SX_FP8_E4M3 if w8 else 0)          # the scalar fields; every pointer is replaced below
    xs = [rows(xp) for xp in I["xs"]]
    keep["x"] = tile_rows(xs, M, K, dtype, dev) if c["x_layout"] else _nan_lead(xs[0])
    keep["W"] = weight_buffer(c, I, w8, dev)
    a.x, a.W = keep["x"].data_ptr(), keep["W"].data_ptr()
    if w8:
        keep["scale"] = _nan_lead(I["scale"], 64)
        a.w_scale = keep["scale"].data_ptr()
    if c["res"]:
        keep["res"] = _nan_lead(rows(I["res"]))
        a.residual = keep["res"].data_ptr()
    if c["gamma"]:
        keep["gamma"] = _nan_lead(I["gamma"], 64)
        a.x16_gamma = keep["gamma"].data_ptr()
    if c["ssq_in"]:
        ssq = I["ssq"]
        if perm is not None:        # padding rows stay where they are
            ssq = torch.cat([ssq[:M][perm], ssq[M:]])
        keep["ssq_in"] = _nan_lead(ssq)
        a.row_ssq_in = keep["ssq_in"].data_ptr()
    P_out = 2 if c["out_planes"] else 1
    R = dict(guards=[])
    if c["out"] == "tiled":
        yb = TiledOut(P_out, M, n_out, dtype, dev)
    else:
        yb = GBuf(M * n_out, torch.float32 if c["out"] == "f32" else dtype, dev)
        yb.allow()[:] = True
    a.y = yb.ptr()
    R["guards"].append(("y", yb))
    if c["emit"]:
        parts = lib.sx_gemv_ssq_parts(N, 0, c["w_layout"])
        xb = TiledOut(P_out, M, N, dtype, dev)
        sb = GBuf(16 * RB * parts, torch.float32, dev)
        sb.allow()[:] = True
        a.x16_out, a.row_ssq_out = xb.ptr(), sb.ptr()
        R["guards"] += [("x16_out", xb), ("row_ssq_out", sb)]
    on_mfma = kernel_of(c)[0] == "sk"
    if on_mfma and c["ws"] != "none":
        # the workspace inside a guard-filled byte buffer: its documented extent zero (the contract), 0xA5 around it
        S = ws_S or max(c["S"], 1)
        nbytes = ws_extent(c, S) - (1 if c["ws"] == "short" else 0)
        wsb = torch.full((256 + nbytes + 4096,), 0xA5, dtype=torch.uint8, device=dev)
        wsb[256:256 + nbytes] = 0
        a.workspace, a.workspace_bytes = wsb.data_ptr() + 256, nbytes
        keep["ws"] = wsb
        R["ws"], R["ws_bytes"] = wsb, nbytes
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if hooks:
        with Hooks(lib, c):
            st = lib.sx_gemv(C.byref(a), stream)
    else:
        st = lib.sx_gemv(C.byref(a), stream)
    _lib.check(st, f"sx_gemv case {c['id']}")
    torch.cuda.synchronize()
    if c["out"] == "tiled":
        R["y"] = yb.planes()                                    # [planes, M, n_out]
    else:
        R["y"] = yb.body.view(M, n_out)
    if c["emit"]:
        R["x16"] = xb.planes()
        R["ssq"] = sb.body.view(16 * RB, parts)
    R["keep"] = keep
    return R


def check_guards(c, R, what):
    for name, g in R["guards"]:
        g.check(f"{what} ({name})")
    assert bool(torch.isfinite(R["y"].float()).all()), f"{what}: non-finite output: an unwritten element or an unmasked read past an input"
    if c["emit"]:
        assert bool(torch.isfinite(R["x16"].float()).all()) and bool(torch.isfinite(R["ssq"][:c["M"]]).all()), f"{what}: non-finite x16_out / row_ssq_out"
    if "ws" in R:
        ws, nb = R["ws"], R["ws_bytes"]
        S = plan_of(c, nb)[2]              # the forced factor unless the workspace is too small for it (no case splits by itself)
        ext = ws_extent(c, S) if S > 1 else 16384
        assert bool((ws[:256] == 0xA5).all()) and bool((ws[256 + nb:] == 0xA5).all()), f"{what}: written outside workspace_bytes"
        assert int(ws[256:256 + 16384].view(torch.int32).abs().sum()) == 0, f"{what}: arrival counters not left at zero"
        assert int(ws[256 + ext:256 + nb].max() if nb > ext else 0) == 0, \
            f"{what}: workspace written past 16384 + S * 16 * MB * N * 4 bytes (S = {S}, MB = {n_blocks(c)})"
        if S > 1:
            assert int(ws[256 + 16384:256 + ext].max()) != 0, f"{what}: the forced split factor {S} did not split"


# ----------------------------------------------------------------------------------------------------------------------------
# fp64 reference and bound
# ----------------------------------------------------------------------------------------------------------------------------
def reference(c, I):
    """fp64 reference [M, n_out] and per-element bound (without the output rounding). As test_gemm_matrix_gpu.reference:
      |y - ref| <= L * C_ACC * sqrt(K * planes) * 2^-24 * mag + C_EP * 2^-24 * (epilogue magnitudes) + 1/2 ulp_out,
    mag = (|x| |W|^T) summed over both planes (it bounds every partial sum of the wave, LDS, split-K and plane additions, which are all
    fp32 additions of the same products); GLU and the activation as there (GLU: |act(gate)| on the linear half's error, L |linear| on
    the gate's). The residual is added AFTER the activation here (one fp32 addition: 2 * 2^-24 of its operands, as there). With
    row_ssq_in the accumulator is scaled by rstd = rsqrt(sum_p ssq[m][p] / dim + eps): the terms scale with |rstd|, plus
    C_EP * 2^-24 * |rstd * z| for the fp32 sum of the 64 positive partials (<= 2^-24 * (64 / 16 / 4 + 4 + 3) relative, halved by the
    square root), the 1-ulp hardware rsqrt and the multiplication. An FP8 weight is decode(code) * scale with a power-of-two scale: the
    kernel's products are those of the 16-bit twin, scaled exactly."""
    K, M = c["K"], c["M"]
    W64 = I["W64"]
    Wabs = W64.abs()
    z = sum(xp.double() @ W64.t() for xp in I["xs"])
    S = sum(xp.double().abs() @ Wabs.t() for xp in I["xs"])
    pre, err = z, C_ACC * math.sqrt(K * c["planes"]) * U32 * S
    if c["ssq_in"]:
        rstd = 1.0 / torch.sqrt(I["ssq"][:M].double().sum(1, keepdim=True) / I["ssq_dim"] + I["ssq_eps"])
        pre = rstd * z
        err = rstd * err + C_EP * U32 * pre.abs()
    L = LIP[c["act"]]
    if c["glu"]:
        n_out = I["n_out"]
        pv, ev = pre.view(M, -1, 2, 16), err.view(M, -1, 2, 16)
        v, g = pv[:, :, 0].reshape(M, n_out), pv[:, :, 1].reshape(M, n_out)
        e_v, e_g = ev[:, :, 0].reshape(M, n_out), ev[:, :, 1].reshape(M, n_out)
        ag = act64(g, c["act"])
        ref = v * ag
        err = ag.abs() * e_v + v.abs() * (L * e_g + C_EP * U32 * g.abs()) + C_EP * U32 * ref.abs()
    elif c["act"] is not None:
        ref = act64(pre, c["act"])
        err = L * err + C_EP * U32 * pre.abs()
    else:
        ref = pre
    if c["res"]:
        res = I["res"].double()
        ref = ref + res
        err = err + 2 * U32 * (ref.abs() + res.abs())
    return ref, err


def check_against_reference(c, I, R, what):
    """Every element against the fp64 bound; returns the worst |diff| / bound. A two-plane output is hi + lo with
    |lo| <= 1/2 ulp(hi) and an output rounding of half a unit of the 16-bit type at the magnitude of that remainder."""
    dtype = I["dtype"]
    ref, err = reference(c, I)
    y = R["y"]
    if c["out"] == "tiled" and c["out_planes"]:
        hi, lo = y[0].double(), y[1].double()
        # a tie of the hi rounding gives |lo| = exactly half a unit; half_ulp's pow is not exact to the last bit on the device
        over = lo.abs() / half_ulp(hi.abs(), dtype)
        if float(over.max()) > 1.0 + 1e-9:
            r, col = divmod(int(over.argmax()), over.shape[1])
            raise AssertionError(f"{what}: {int((over > 1.0 + 1e-9).sum())} lo-plane elements larger than half a unit of the hi plane; worst at row {r}, "
                                 f"column {col}: hi {float(hi[r, col])!r}, lo {float(lo[r, col])!r}, ref {float(ref[r, col])!r}")
        y64 = hi + lo
        top = torch.maximum(ref.abs() + err, y64.abs())
        rnd, odt = half_ulp(half_ulp(top, dtype), dtype), torch.float32
    else:
        y64 = (y[0] if c["out"] == "tiled" else y).double()
        odt = torch.float32 if c["out"] == "f32" else dtype
        rnd = half_ulp(torch.maximum(ref.abs() + err, y64.abs()), odt)
    bound = err + rnd
    d = (y64 - ref).abs()
    ratio = d / bound
    worst = float(ratio.max())
    if worst > 1.0:
        i = int(ratio.argmax())
        r, col = divmod(i, ratio.shape[1])
        raise AssertionError(f"{what} [{kernel_of(c)}]: {int((ratio > 1.0).sum())} elements beyond the fp64 bound; worst at row {r}, column "
                             f"{col}: got {float(y64[r, col])!r}, ref {float(ref[r, col])!r}, |diff| {float(d[r, col]):.3e} > bound "
                             f"{float(bound[r, col]):.3e}")
    rel = float((y64 - ref).norm() / ref.norm().clamp_min(1e-30))
    assert rel < TOL[odt], f"{what}: rel-L2 {rel:.3e} vs fp64 >= {TOL[odt]}"
    return worst


def check_fold_outputs(c, I, R, what):
    """x16_out bit for bit from the stored fp32 y (rn16(y * gamma); two planes: hi saturates at the largest finite fp16, lo =
    rn16(y * gamma - hi)), row_ssq_out[m][p] against the fp64 sum of squares of the stored y over workgroup p's columns: n fp32
    additions of n rounded squares, (C_ACC sqrt(n) + 1) * 2^-24 of the (positive) sum, plus half a unit of the fp32 result."""
    dtype, M, N = I["dtype"], c["M"], c["N"]
    y = R["y"]
    og = y * I["gamma"][None, :] if c["gamma"] else y
    ib = _ibits(dtype)
    if c["out_planes"]:
        hi = (og.clamp(-65504.0, 65504.0) if dtype == F16 else og).to(dtype)
        lo = (og - hi.float()).to(dtype)
        want = torch.stack([hi, lo])
    else:
        want = og.to(dtype)[None]
    assert torch.equal(R["x16"].view(ib), want.view(ib)), f"{what}: x16_out != rn16(y * gamma) of the stored y"
    parts = R["ssq"].shape[1]
    ncol = N // parts
    want = y.double().pow(2).view(M, parts, ncol).sum(2)
    bound = (C_ACC * math.sqrt(ncol) + 1.0) * U32 * want + half_ulp(want, torch.float32)
    d = (R["ssq"][:M].double() - want).abs()
    assert bool((d <= bound).all()), f"{what}: row_ssq_out off by {float((d / bound).max()):.2f} bounds (parts of {ncol} columns)"


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(_ibits(a.dtype)), b.contiguous().view(_ibits(b.dtype)))


def stops_on_gpu_fault(fn):
    """A GPU fault poisons the process: every later launch fails for the same reason (and keeps hitting a faulted device). End the session at
    the first one instead."""
    import functools

    @functools.wraps(fn)
    def wrapped(*a, **kw):
        try:
            return fn(*a, **kw)
        except RuntimeError as e:
            if any(t in str(e) for t in ("HIP error", "hipError", "illegal memory access", "device-side assert")):
                pytest.exit(f"GPU fault in {fn.__name__}: {e}", returncode=3)
            raise
    return wrapped


def run_case(c, dev, tag=""):
    from seedx_amd import _lib
    lib = _lib.load()
    what = c["id"] + tag
    kern = kernel_of(c)
    assert c["fam"] is None or kern == ("sk",) + c["fam"] + (c["w8"],), (what, kern)
    I = make_inputs(c, dev)
    R = launch(lib, c, I, dev)
    check_guards(c, R, what)
    worst = check_against_reference(c, I, R, what)
    key = (kern, c["dt"])
    WORST[key] = max(WORST.get(key, 0.0), worst)
    if c["out"] == "f32":
        WORST32[key] = max(WORST32.get(key, 0.0), worst)
    print(f"{what}: {kern} worst |diff| / bound {worst:.3f}")
    if c["emit"]:
        check_fold_outputs(c, I, R, what)
    outs = ["y"] + (["x16", "ssq"] if c["emit"] else [])
    M = c["M"]
    live = lambda R2, k: R2[k][:M] if k == "ssq" else R2[k]
    R2 = launch(lib, c, I, dev)
    check_guards(c, R2, what + " (second launch)")
    for k in outs:
        assert same_bits(live(R2, k), live(R, k)), f"{what}: two identical launches differ in {k}"
    if M > 1:
        # the rows rolled by one: no row keeps its slot, rows 0 and 16 change their 16-row block
        perm = ((torch.arange(M) + 1) % M).to(dev)
        assert not torch.equal(perm, torch.arange(M, device=dev))
        Rp = launch(lib, c, I, dev, perm=perm)
        check_guards(c, Rp, what + " (permuted rows)")
        for k in outs:
            a, b = live(Rp, k), live(R, k)
            want = b[:, perm] if a.dim() == 3 else b[perm]
            assert same_bits(a, want), f"{what}: {k} of a request depends on its row (slot) in x"
    if c["w8"]:
        Rt = launch(lib, c, I, dev, w8=False)
        check_guards(c, Rt, what + " (16-bit twin)")
        for k in outs:
            assert same_bits(live(Rt, k), live(R, k)), f"{what}: FP8 {k} != the 16-bit launch on the dequantised weights"
    return R, I


# ----------------------------------------------------------------------------------------------------------------------------
# GEMV tests
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SKINNY, ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_skinny_instantiation(dev, c):
    run_case(c, dev)


@pytest.mark.parametrize("c", VALU, ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_valu_kernel_edges(dev, c):
    assert kernel_of(c)[0] == "valu"
    run_case(c, dev)


@pytest.mark.parametrize("c", BOTH, ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_valu_against_mfma(dev, c):
    """Where both kernels are legal each meets the fp64 bound on the same operands (so they differ by at most both bounds)."""
    cv, cm = dict(c, fv=1), dict(c, fv=2)            # the same id: the operands' seed follows it
    assert kernel_of(cv)[0] == "valu" and kernel_of(cm)[0] == "sk"
    Rv, I = run_case(cv, dev, tag=" (forced VALU)")
    Rm, _ = run_case(cm, dev, tag=" (forced MFMA)")
    ref, err = reference(c, I)
    odt = Rv["y"].dtype
    lim = 2 * err + half_ulp(ref.abs() + err, odt) * 2
    d = (Rv["y"].double() - Rm["y"].double()).abs()
    assert bool((d <= lim).all()), f"{c['id']}: VALU and MFMA results differ by {float((d / lim).max()):.2f} of both bounds"


@stops_on_gpu_fault
def test_split_workspace_threshold_is_per_mb(dev):
    """The workspace cases really sit one byte below the host's own threshold: with that byte the same launch splits."""
    from seedx_amd import _lib
    lib = _lib.load()
    for c in [c for c in SKINNY if c["ws"] == "short" and c["dt"] == "f16" and not c["w8"]]:
        full = dict(c, ws="full")
        I = make_inputs(full, dev)
        R = launch(lib, full, I, dev)
        check_guards(full, R, c["id"] + " (full workspace)")          # asserts that S = 2 did split
        check_against_reference(full, I, R, c["id"] + " (full workspace)")


def _probe_split(lib, dev, K):
    """Does a launch that leaves the hooks alone write split-K partial sums? M = 5, N = 32 on <1, 4, F, 1>, workspace with room for
    every split factor."""
    c = case(f"defaults-split-K{K}", "f16", M=5, N=32, K=K, w_layout=1, x_layout=1)
    R = launch(lib, c, make_inputs(c, dev), dev, ws_S=8, hooks=False)
    return int(R["ws"][256 + 16384:256 + R["ws_bytes"]].max()) != 0


def _probe_path(lib, dev, c, I):
    return launch(lib, c, I, dev, hooks=False)["y"]


# where hooks 3 and 1 change the kernel family: 200 64-row workgroups (R = 4 by default, R = 2 with hook 3 at 0), 64 of them (R = 2 by
# default, R = 4 with hook 3 at 2, as the matrix sets it), and 17 rows on 20-row tiles (U = 2 by default, U = 4 with hook 1 at 1 or 2)
PROBE_R4 = case("defaults-r4", "f16", M=8, N=12800, K=256)
PROBE_R2 = case("defaults-r2", "f16", M=8, N=4096, K=256, glu=True, act="silu")
PROBE_U = case("defaults-u", "f16", M=17, N=640, K=256, w_layout=2)


@stops_on_gpu_fault
def test_hook_defaults_restored(dev):
    """After the matrix above (this test runs behind it) the library itself is asked, by launches that do NOT touch the hooks (every
    other launch of this file sets all four first, which would hide a leaked value):
      * sx_gemv_tune(2, .) is 0: K = 320 with a workspace writes no partial sums (2 / 4 / 8 would), K = 8192 splits by itself
        (-1 and 1 would not);
      * sx_gemv_force_valu is 0: a row-major M = 3 launch gives the VALU kernel's bits (2 would give the MFMA kernel's), M = 5 the
        MFMA kernel's (1 would give the VALU kernel's).
      * sx_gemv_tune(3, .) is 1 and sx_gemv_tune(1, .) is 0. They choose between kernels that give the same bits, the same
        partial-sum layout ([S][16 MB][N]) and the same counters, so no launch can tell their state at a shape this suite affords;
        sx_gemv_plan can, without a launch: N = 12800 without GLU at M = 8 runs R = 4 (200 64-row workgroups; 0 would give R = 2),
        GLU N = 4096 runs R = 2 (2 would give R = 4), 17 rows on 20-row tiles run U = 2 (hook 1 at 1 or 2 would give U = 4).
    The probes are then shown to see a leak: with (2, 8) resp. force_valu(1) / (2), (3, 0), (3, 2), (1, 1) and (1, 2) set on purpose
    they answer the other way."""
    from seedx_amd import _lib
    lib = _lib.load()
    _probe_family = lambda c: lib_plan(lib, plan_args(c))[3:5]          # (R, U) by sx_gemv_plan: nothing launched, no hook touched
    # 1. the probes, before anything in this test sets a hook
    family_r4, family_r2, family_u = (_probe_family(c) for c in (PROBE_R4, PROBE_R2, PROBE_U))
    leaked_split, auto_split = _probe_split(lib, dev, 320), _probe_split(lib, dev, 8192)
    paths = {}
    for M in (3, 5):
        c = case(f"defaults-path-M{M}", "f16", M=M, N=512, K=256)
        I = make_inputs(c, dev)
        paths[M] = (c, I, _probe_path(lib, dev, c, I))
    # 2. what they are compared with: the same launches with the path forced (Hooks restores the defaults after each)
    forced = {M: {fv: launch(lib, dict(c, fv=fv), I, dev)["y"] for fv in (1, 2)} for M, (c, I, _) in paths.items()}
    for M in (3, 5):
        assert not same_bits(forced[M][1], forced[M][2]), "the VALU and the MFMA kernel give the same bits here: the probe cannot tell them apart"
    assert not leaked_split, "a forced split factor is still set: sx_gemv_tune(2, .) > 1 leaked out of a test"
    assert auto_split, "the automatic split-K is switched off: sx_gemv_tune(2, -1 or 1) leaked out of a test"
    assert same_bits(paths[3][2], forced[3][1]), "M = 3 does not run the VALU kernel: sx_gemv_force_valu(2) leaked out of a test"
    assert same_bits(paths[5][2], forced[5][2]), "M = 5 does not run the MFMA kernel: sx_gemv_force_valu(1) leaked out of a test"
    assert family_r4 == (4, 2), f"N = 12800 at M = 8 does not run <4, 4, 2, F, 1> but (R, U) = {family_r4}: sx_gemv_tune(3, 0) leaked out of a test"
    assert family_r2 == (2, 4), f"GLU N = 4096 at M = 8 does not run <2, 4, 4, F, 1> but (R, U) = {family_r2}: sx_gemv_tune(3, 2) leaked out of a test"
    assert family_u == (2, 2), f"17 rows on 20-row tiles do not run <2, 4, 2, T, 2> but (R, U) = {family_u}: sx_gemv_tune(1, .) leaked out of a test"
    # 3. the probes do see a leak
    try:
        assert lib.sx_gemv_tune(2, 8) == 0
        assert _probe_split(lib, dev, 320), "the split probe does not see sx_gemv_tune(2, 8)"
        assert lib.sx_gemv_tune(2, -1) == 0
        assert not _probe_split(lib, dev, 8192), "the split probe does not see sx_gemv_tune(2, -1)"
        assert lib.sx_gemv_tune(2, 0) == 0
        for fv, M in ((1, 5), (2, 3)):
            assert lib.sx_gemv_force_valu(fv) == 0
            c, I, _ = paths[M]
            assert same_bits(_probe_path(lib, dev, c, I), forced[M][fv]), f"the path probe does not see sx_gemv_force_valu({fv})"
        assert lib.sx_gemv_force_valu(0) == 0 and lib.sx_gemv_tune(3, 0) == 0
        assert _probe_family(PROBE_R4) == (2, 4), "the family probe does not see sx_gemv_tune(3, 0)"
        assert lib.sx_gemv_tune(3, 2) == 0
        assert _probe_family(PROBE_R2) == (4, 2), "the family probe does not see sx_gemv_tune(3, 2)"
        assert lib.sx_gemv_tune(3, 1) == 0
        for v in (1, 2):
            assert lib.sx_gemv_tune(1, v) == 0
            assert _probe_family(PROBE_U) == (2, 4), f"the family probe does not see sx_gemv_tune(1, {v})"
    finally:
        restore_defaults(lib)
    assert not _probe_split(lib, dev, 320) and _probe_split(lib, dev, 8192)
    assert [_probe_family(c) for c in (PROBE_R4, PROBE_R2, PROBE_U)] == [(4, 2), (2, 4), (2, 2)]


# ----------------------------------------------------------------------------------------------------------------------------
# decode attention against an fp64 softmax
# ----------------------------------------------------------------------------------------------------------------------------
TMAX = 96
# context lengths of the sequences of a launch: the first 7 are the edges (one key, two, around the 16 key rows of a pass, ctx < nsplit,
# the last slot and the one before); a launch of one sequence takes one of G1_CTX
CTX_POOL = (17, 1, 96, 2, 15, 16, 95, 3, 5, 33, 64, 7, 48, 31, 9, 63, 40, 8, 11, 80)
NSPLITS = (1, 3, 8, 64)
DOMINANT = 8.0           # score of the planted last visible key; the random keys' scores are N(0, 1)


def _rope64(x, pos, cos_t, sin_t, dtype):
    """fp64 rotation of x [G, H, D] at positions pos [G], tables rounded to the activation dtype first (as test_rope_kv_append)."""
    D = x.shape[-1]
    c = torch.cat([cos_t, cos_t], -1)[pos].to(dtype).double()[:, None, :]
    s = torch.cat([sin_t, sin_t], -1)[pos].to(dtype).double()[:, None, :]
    xf = x.double()
    rot = torch.cat([-xf[..., D // 2:], xf[..., :D // 2]], -1)
    return xf * c + rot * s


def _attn64(q, keys, vals, scale):
    """softmax(scale * q K^T) V in fp64 for the heads of one sequence: q [H, D], keys / vals [H, ctx, D]."""
    s = torch.einsum("hnd,hd->hn", keys.double(), q.double()) * scale
    return torch.einsum("hn,hnd->hd", torch.softmax(s, -1), vals.double())


class AttnCase:
    """Inputs of one decode-attention launch: q read out of a fused qkv buffer (q_seq_stride = 3 H D), caches with a padded sequence
    stride whose gaps, like every row at a position >= ctx[g], hold NaN bits; the last visible key of every (sequence, head) carries a
    dominant score, so dropping it (or admitting the NaN row behind it) moves the output row by far more than the tolerance."""

    def __init__(self, dev, dtype, G, H, D, ctx, seed, fused):
        gen = torch.Generator(device=dev).manual_seed(seed)
        self.G, self.H, self.D, self.ctx, self.dtype, self.fused = G, H, D, ctx, dtype, fused
        self.scale = D ** -0.5
        self.stride = H * TMAX * D + 64
        qkv, _ = guarded((G, 3 * H * D), dtype, dev, gen)
        self.qkv = qkv
        q = qkv[:, :H * D].view(G, H, D)
        # the key with the dominant score: a multiple of q (a rotation at one position keeps the dot product, so this holds for the
        # un-rotated k of the fused form too)
        qf = q.float()
        kdom = (qf * (DOMINANT / (self.scale * qf.pow(2).sum(-1, keepdim=True)))).to(dtype)
        self.kc = _nanbuf(G * self.stride + 256, dtype, dev)
        self.vc = _nanbuf(G * self.stride + 256, dtype, dev)
        for g in range(G):
            n = ctx[g] - (1 if fused else 0)            # fused: the last visible key is the new token, its cache row still NaN
            if n <= 0:
                continue
            for buf, last in ((self.kc, kdom[g]), (self.vc, None)):
                v = buf[g * self.stride:g * self.stride + H * TMAX * D].view(H, TMAX, D)
                v[:, :n] = torch.randn(H, n, D, device=dev, generator=gen).to(dtype)
                if last is not None and not fused:
                    v[:, n - 1] = last
        if fused:
            self.qkv.view(G, 3, H, D)[:, 1] = kdom
        inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
        fr = torch.outer(torch.arange(TMAX).float(), inv)
        self.cos, self.sin = fr.cos().to(dev).contiguous(), fr.sin().to(dev).contiguous()
        self.ctx_dev = torch.tensor(ctx, dtype=torch.int32, device=dev)
        self.kc0, self.vc0, self.qkv0 = self.kc.clone(), self.vc.clone(), self.qkv.clone()

    def cache(self, buf, g):
        return buf[g * self.stride:g * self.stride + self.H * TMAX * self.D].view(self.H, TMAX, self.D)

    def reference(self):
        """fp64 output [G, H, D] (zero rows for ctx = 0) and, for the fused form, the rotated K rows [G, H, D] of the new token."""
        G, H, D = self.G, self.H, self.D
        v3 = self.qkv0.view(G, 3, H, D)
        out = torch.zeros(G, H, D, dtype=torch.float64, device=self.qkv.device)
        if self.fused:
            pos = (self.ctx_dev - 1).long()
            q = _rope64(v3[:, 0], pos, self.cos, self.sin, self.dtype).to(self.dtype)
            knew64 = _rope64(v3[:, 1], pos, self.cos, self.sin, self.dtype)
            knew = knew64.to(self.dtype)
        else:
            q, knew64 = v3[:, 0], None
        for g in range(G):
            n = self.ctx[g]
            if n == 0:
                continue
            K, V = self.cache(self.kc0, g)[:, :n].clone(), self.cache(self.vc0, g)[:, :n].clone()
            if self.fused:
                K[:, n - 1], V[:, n - 1] = knew[g], v3[g, 2]
            out[g] = _attn64(q[g], K, V, self.scale)
        return out, knew64


def _check_attn_rows(got, ref, ctx, dtype, what):
    """Per (sequence, head) row: finite, relative L2 against the fp64 softmax below the project's TOL; ctx = 0 gives zeros."""
    assert bool(torch.isfinite(got.float()).all()), f"{what}: non-finite output (a key at a position >= ctx was read?)"
    g64 = got.double()
    for g, n in enumerate(ctx):
        if n == 0:
            assert bool((g64[g] == 0).all()), f"{what}: sequence {g} has no key, its output must be zero"
    num, den = (g64 - ref).norm(dim=-1), ref.norm(dim=-1)
    rel = torch.where(den > 0, num / den.clamp_min(1e-30), num)
    worst = int(rel.argmax())
    assert float(rel.max()) < TOL[dtype], f"{what}: row (sequence {worst // ref.shape[1]}, head {worst % ref.shape[1]}, ctx " \
                                         f"{ctx[worst // ref.shape[1]]}) rel-L2 {float(rel.max()):.3e} vs fp64 >= {TOL[dtype]}"
    return float(rel.max())


def _attn_out(G, H, D, dtype, dev, tiled):
    if tiled:
        return TiledOut(1, G, H * D, dtype, dev)
    ob = GBuf(G * H * D, dtype, dev)
    ob.allow()[:] = True
    return ob


def _attn_result(ob, G, H, D, tiled):
    return (ob.planes()[0] if tiled else ob.body.view(G, H * D)).view(G, H, D)


# the context of a launch of one sequence: one of the edges, rotating with the other parameters. Any four in a row (cyclically) hold one
# of 1, 2 (fewer keys than splits), one of 15, 16, 17 (around the 16 key rows of a pass) and one of 95, 96 (the end of the cache)
G1_CTX = (1, 96, 16, 2, 95, 17, 15)


def _ctx_list(G, j, with_zero):
    if G == 1:
        return [G1_CTX[j % len(G1_CTX)]]
    ctx = list(CTX_POOL[:G])
    if with_zero and G > 7:
        ctx[7] = 0
    return ctx


def _attn_params(Ds, fused):
    """One test per (dtype, D, H, G, nsplit, output layout); a tiled output needs H * D % 32 == 0. j picks the context of a launch
    of one sequence: it moves on by one with (D, H), with the dtype and with (nsplit, layout), so each (nsplit, layout) pair meets at
    least four contexts in a row of G1_CTX."""
    out = []
    for di, dt in enumerate(DTYPES):
        for G in (1, 7, 20):
            for k, (D, H) in enumerate((D, H) for D in Ds for H in (2, 5)):
                for ni, nsplit in enumerate(NSPLITS):
                    for tiled in (False, True):
                        if tiled and (H * D) % 32:
                            continue
                        j = k + di + 2 * ni + tiled
                        ctx = f"ctx{_ctx_list(G, j, not fused)[0]}" if G == 1 else "mixed"
                        out.append(pytest.param(dt, D, H, G, nsplit, tiled, j,
                                                id=f"{dt}-D{D}-H{H}-G{G}-nsplit{nsplit}-{'tiled' if tiled else 'rows'}-{ctx}"))
    for nsplit in NSPLITS:
        for tiled in (False, True):
            one = {_ctx_list(1, p.values[6], False)[0] for p in out if p.values[3:6] == (1, nsplit, tiled)}
            assert one & {1, 2} and one & {15, 16, 17} and one & {95, 96}, (nsplit, tiled, one)
    assert {_ctx_list(1, p.values[6], False)[0] for p in out if p.values[3] == 1} == set(G1_CTX)
    return out


@pytest.mark.parametrize("dt,D,H,G,nsplit,tiled,j", _attn_params((64, 112, 128), fused=False))
@stops_on_gpu_fault
def test_attn_decode_b_vs_fp64(dev, dt, D, H, G, nsplit, tiled, j):
    """sx_attn_decode_b (split kernel + combine kernel), one test per nsplit and output layout."""
    from seedx_amd import _lib
    lib = _lib.load()
    dtype = DTYPES[dt]
    code = _lib.SX_F16 if dtype == F16 else _lib.SX_BF16
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ctx = _ctx_list(G, j, with_zero=True)
    A = AttnCase(dev, dtype, G, H, D, ctx, seed=1000 * D + 100 * H + 10 * G + j, fused=False)
    ref, _ = A.reference()
    ob = _attn_out(G, H, D, dtype, dev, tiled)
    scratch = GBuf(G * H * nsplit * (D + 2), torch.float32, dev)
    scratch.allow()[:] = True
    what = f"attn_decode_b {dt} D{D} H{H} G{G} nsplit{nsplit} {'tiled' if tiled else 'rows'} ctx{ctx}"
    _lib.check(lib.sx_attn_decode_b(A.qkv.data_ptr(), A.kc.data_ptr(), A.vc.data_ptr(), ob.ptr(), scratch.ptr(), A.ctx_dev.data_ptr(),
                                    G, H, D, TMAX, A.stride, nsplit, A.scale, code | (_lib.SX_TILED16 if tiled else 0), 3 * H * D,
                                    stream), what)
    torch.cuda.synchronize()
    ob.check(what + " (out)")
    scratch.check(what + " (scratch)")
    assert same_bits(A.kc, A.kc0) and same_bits(A.vc, A.vc0) and same_bits(A.qkv, A.qkv0), f"{what}: an input was written"
    w = _check_attn_rows(_attn_result(ob, G, H, D, tiled), ref, ctx, dtype, what)
    print(f"{what}: worst row rel-L2 {w:.2e}")


@pytest.mark.parametrize("dt,D,H,G,nsplit,tiled,j", _attn_params((64, 128), fused=True))
@stops_on_gpu_fault
def test_attn_decode_fused_vs_fp64(dev, dt, D, H, G, nsplit, tiled, j):
    """sx_attn_decode_fused, one test per nsplit and output layout: RoPE of the new token, append, attention and combine against the
    same fp64 reference after the fp64 rotation; V rows of the new token bit for bit, K rows at the output-rounding TOL (as
    test_rope_kv_append), every other cache element and the qkv row unchanged, arrival counters zero."""
    from seedx_amd import _lib
    lib = _lib.load()
    dtype = DTYPES[dt]
    code = _lib.SX_F16 if dtype == F16 else _lib.SX_BF16
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ctx = _ctx_list(G, j, with_zero=False)
    A = AttnCase(dev, dtype, G, H, D, ctx, seed=2000 * D + 100 * H + 10 * G + j, fused=True)
    ref, knew64 = A.reference()
    ob = _attn_out(G, H, D, dtype, dev, tiled)
    scratch = GBuf(G * H * nsplit * (D + 2), torch.float32, dev)
    scratch.allow()[:] = True
    cnt = GBuf(G * H, torch.float32, dev)                 # 32-bit counters inside a guard buffer
    cnt.allow()[:] = True
    cnt.body.view(torch.int32).zero_()
    pos = (A.ctx_dev - 1).contiguous()
    a = _lib.AttnDecodeArgs()
    a.qkv, a.kcache, a.vcache, a.out, a.scratch, a.counters = A.qkv.data_ptr(), A.kc.data_ptr(), A.vc.data_ptr(), ob.ptr(), scratch.ptr(), cnt.ptr()
    a.cos_tab, a.sin_tab, a.pos_dev = A.cos.data_ptr(), A.sin.data_ptr(), pos.data_ptr()
    a.G, a.H, a.D, a.Tmax, a.nsplit, a.dtype = G, H, D, TMAX, nsplit, code | (_lib.SX_TILED16 if tiled else 0)
    a.cache_seq_stride, a.scale = A.stride, A.scale
    what = f"attn_decode_fused {dt} D{D} H{H} G{G} nsplit{nsplit} {'tiled' if tiled else 'rows'} ctx{ctx}"
    _lib.check(lib.sx_attn_decode_fused(C.byref(a), stream), what)
    torch.cuda.synchronize()
    ob.check(what + " (out)")
    scratch.check(what + " (scratch)")
    cnt.check(what + " (counters)")
    assert int(cnt.body.view(torch.int32).abs().sum()) == 0, f"{what}: arrival counters not left at zero"
    assert same_bits(A.qkv, A.qkv0), f"{what}: the qkv row was written"
    # the caches: only row pos of every (sequence, head) changed
    ib = _ibits(dtype)
    v3 = A.qkv0.view(G, 3, H, D)
    for g in range(G):
        p = ctx[g] - 1
        for buf, buf0 in ((A.kc, A.kc0), (A.vc, A.vc0)):
            new, old = A.cache(buf, g).clone(), A.cache(buf0, g).clone()
            new[:, p], old[:, p] = 0, 0
            assert torch.equal(new.view(ib), old.view(ib)), f"{what}: cache rows other than the new position changed (sequence {g})"
        assert torch.equal(A.cache(A.vc, g)[:, p].view(ib), v3[g, 2].view(ib)), f"{what}: appended V row (sequence {g})"
        krow = A.cache(A.kc, g)[:, p].double()
        rel = (krow - knew64[g]).norm(dim=-1) / knew64[g].norm(dim=-1)
        assert bool(torch.isfinite(krow).all()) and float(rel.max()) < TOL[dtype], f"{what}: appended K row (sequence {g}) {float(rel.max()):.2e}"
    gap = lambda buf: torch.cat([buf[g * A.stride + H * TMAX * D:(g + 1) * A.stride] for g in range(G)] + [buf[G * A.stride:]])
    assert same_bits(gap(A.kc), gap(A.kc0)) and same_bits(gap(A.vc), gap(A.vc0)), f"{what}: the gaps between sequences were written"
    w = _check_attn_rows(_attn_result(ob, G, H, D, tiled), ref, ctx, dtype, what)
    print(f"{what}: worst row rel-L2 {w:.2e}")


def test_print_worst_ratio_per_instantiation(dev):
    """Not a check of its own: the worst |diff| / bound of the GEMV cases above, per instantiation and dtype (run the file as a whole).
    Over all outputs the figure sits just below 1 by construction: a 16-bit output is rounded once, by up to the bound's 1/2 ulp_out
    term, which is hundreds of times the accumulation terms, and among thousands of elements one comes close to a rounding tie. It
    says that the output is rounded once and correctly, nothing about C_ACC or C_EP. The fp32 column is the one that measures the
    accumulation and epilogue terms against their constants."""
    for (kern, dt), w in sorted(WORST.items(), key=lambda kv: str(kv[0])):
        w32 = WORST32.get((kern, dt))
        print(f"worst |diff| / bound  {str(kern):42s} {dt:5s} all outputs {w:.3f}   fp32 outputs {'  -  ' if w32 is None else format(w32, '.3f')}")
    assert all(w <= 1.0 for w in WORST.values())
