"""sx_gemm against an fp64 reference: every lock-step tile config (gemm.hip launch_cfg 0-6) and every ping-pong specialization
(gemm_pp.hip launch_t on tiles 7 / 8), both operand dtypes, at the edges where tiled kernels go wrong.

Each case drives sx_gemm / sx_gemm_ln through _lib.GemmArgs directly (every runtime branch is reachable: ldc > n_store, a misaligned
C, ld_bias2d > N, ...) and checks
  * the output element by element against an fp64 reference built from the SAME 16-bit operands (bound: see `reference`), plus the
    relative-L2 TOL of test_kernels_gpu.py as a second assert;
  * that nothing outside the logical output changed: C lives in a larger buffer (guard elements before it, extra rows after M, columns
    up to ldc) filled with a NaN bit pattern that must be bit-unchanged afterwards, while every logical element must be finite;
  * that no read goes past a logical input: A, W, the conv input, bias, bias2d and the residual are leading views of larger
    NaN-filled buffers (pad columns of bias2d / residual included), so an unmasked read shows up as a non-finite output;
  * that a second identical launch gives the same bits.
Production shapes (the config-0 UNet step at 32 CFG rows, the ViT-G at 20 / 32 crops, a 1.6-GiB A operand) check a row subset: every
row within 2 of a 256-row tile boundary or of a sample boundary, plus 4096 random rows.

Every test that forces a tile, the XCD partition or gm restores the defaults (-1, 101, 300) in `finally`: that state is process-global.
tests/test_cpu_suite.py::test_gemm_matrix_covers_every_launched_kernel checks (without a GPU) that PP_SPECS / LOCKSTEP_TILES list every
specialization that the sources instantiate.
"""
import ctypes as C
import math
import os
import re
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "seed-x_amd", "csrc")

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = {"f16": F16, "bf16": BF16}
TOL = {torch.float32: 2e-5, torch.float16: 6e-4, torch.bfloat16: 4e-3}      # test_kernels_gpu.py's rel-L2 bounds

# tile config -> (BM, BN, GLU-capable); 0-6 lock-step (gemm.hip kTiles / SX_GEMM_DISPATCH), 7 / 8 ping-pong (gemm_pp.hip)
TILES = {0: (128, 128, True), 1: (128, 80, False), 2: (64, 128, True), 3: (64, 64, True), 4: (256, 256, True),
         5: (256, 320, False), 6: (256, 160, False), 7: (256, 256, True), 8: (256, 320, False)}
LOCKSTEP_TILES = (0, 1, 2, 3, 4, 5, 6)

U32 = 2.0 ** -24           # unit roundoff of the fp32 accumulation
C_ACC = 4.0                # accumulation constant of the bound (error_bound docstring)
C_EP = 8.0                 # fp32 epilogue arithmetic (activation approximations, FMAs), in units of U32 of the operand magnitude
LIP = {None: 1.0, "gelu": 1.13, "silu": 1.10}    # max |GELU'| = 1.1289, max |SiLU'| = 1.0998

# bit patterns: inputs are padded with a quiet NaN, the output guard with another NaN that the kernel never produces
NAN16_IN, NAN16_GUARD = 0x7FFF, 0x7F5A           # NaN as fp16 (exp 31, mantissa != 0) and as bf16 (exp 255, mantissa != 0)
NAN32_IN, NAN32_GUARD = 0x7FFFFFFF, 0x7FA5A5A5


# ----------------------------------------------------------------------------------------------------------------------------
# the case table
# ----------------------------------------------------------------------------------------------------------------------------
def case(cid, dt, tile, mode="lin", **kw):
    c = dict(id=cid, dt=dt, tile=tile, mode=mode, M=0, N=16, K=64, B=1, H=0, W=0, Cin=64, stride=1, pad_mode=0, out="16",
             act=None, glu=False, bias=True, b2=0, b2_extra=0, res=False, ldr_extra=0, res_mod=0, n_valid=0, ldc_extra=0, c_off=0,
             planes=1, ln=None, xcd=None, gm=None, subset=False, sample_rows=0)
    c.update(kw)
    if mode != "lin":
        up = mode == "up"
        hv, wv = (2 * c["H"], 2 * c["W"]) if up else (c["H"], c["W"])
        padsum = 1 if c["pad_mode"] else 2
        c["Hout"], c["Wout"] = (hv + padsum - 3) // c["stride"] + 1, (wv + padsum - 3) // c["stride"] + 1
        c["M"], c["K"] = c["B"] * c["Hout"] * c["Wout"], 9 * c["Cin"]
    return c


def kernel_of(c):
    """The kernel a case runs: ('ls', tile) or ('pp', BN, A mode, fp32 out, act, GLU, LayerNorm role) — names as in launch_t."""
    if c["tile"] in LOCKSTEP_TILES:
        return ("ls", c["tile"])
    am = {"lin": "SX_A_LINEAR", "conv": "SX_A_CONV3X3", "up": "SX_A_CONV3X3_UP"}[c["mode"]]
    act = {None: "SX_ACT_NONE", "gelu": "SX_ACT_GELU", "silu": "SX_ACT_SILU"}[c["act"]]
    return ("pp", TILES[c["tile"]][1], am, c["out"] == "f32", act, c["glu"], {None: 0, "cons": 1, "prod": 2}[c["ln"]])


def source_kernels():
    """Every lock-step config of SX_GEMM_DISPATCH and every ping-pong instantiation of launch_t, parsed from the sources: the table
    below must list each of them."""
    src = open(os.path.join(CSRC, "gemm.hip")).read()
    ls = {}
    for i, m in enumerate(re.finditer(r"(?:case (\d)|default): return launch_cfg<TT, (\d+), (\d+), \d, \d, \d>", src)):
        ls[int(m.group(1)) if m.group(1) else i] = (int(m.group(2)), int(m.group(3)))
    src = open(os.path.join(CSRC, "gemm_pp.hip")).read()
    body = src[src.index("static int launch_t("):src.index("int launch_pp(")]
    pp = []
    for m in re.finditer(r"launch_one<TT, (\d+), (\w+), (true|false), (\w+), (true|false)(?:, (\d))?>", body):
        bn, am, o32, act, glu, ln = m.groups()
        pp.append(("pp", int(bn), am, o32 == "true", act, glu == "true", int(ln or 0)))
    for m in re.finditer(r"PP_CASE\((\d+), (\w+), (true|false), (\w+), (true|false)\)", body):
        bn, am, o32, act, glu = m.groups()
        pp.append(("pp", int(bn), am, o32 == "true", act, glu == "true", 0))
    return ls, pp


def lockstep_cases(dt):
    out = []
    for t in LOCKSTEP_TILES:
        BM, BN, glu_ok = TILES[t]
        L = lambda tag, **kw: out.append(case(f"{tag}-{dt}-t{t}", dt, t, **kw))
        # M exact multiple / K one k-tile / N = 16
        L("exactM-K64-N16", M=2 * BM, N=16, K=64)
        # M = BM*k + 1, N = BN + 16, 26 k-tiles; fp32 out + SiLU + residual (epilogue load) + straddling bias2d, padded row strides
        L("tailM-K1664-silu-res-b2", M=3 * BM + 1, N=BN + 16, K=1664, out="f32", act="silu", res=True, ldr_extra=8, b2=100,
          b2_extra=12)
        # M < BM, N % BN != 0; GELU, residual broadcast (res_mod), ldc % 8 != 0 (narrow stores)
        L("smallM-K128-gelu-resmod-ldc4", M=BM - 5, N=2 * BN + 48, K=128, act="gelu", res=True, res_mod=7, ldr_extra=4, ldc_extra=4)
        # 16-bit residual as initial value, n_valid < N, ldc % 8 == 0 > n_store (wide stores), 25 k-tiles
        L("resinit-nvalid-ldc8-K1600", M=2 * BM - 1, N=2 * BN, K=1600, res=True, n_valid=2 * BN - 20, ldc_extra=12,
          b2=BM, b2_extra=4)
        # long K, fp32 out, residual as initial value with res_mod, no bias
        L("longK-f32-resinit-resmod", M=2 * BM, N=BN - 16 if BN > 16 else 16, K=5760, out="f32", bias=False, res=True, res_mod=BM + 3)
        # a_planes = 2: A = [hi | lo], W walked twice
        L("planes2", M=BM + 3, N=BN + 16, K=192, out="f32", planes=2, res=True, ldr_extra=4)
        if glu_ok:
            L("geglu-nvalid", M=3 * BM + 1, N=2 * BN, K=1664, act="gelu", glu=True, n_valid=BN - 12, ldc_extra=4, res=True)
            L("swiglu-f32-b2", M=BM - 1, N=BN + 32 if (BN + 32) % 32 == 0 else 2 * BN, K=128, act="silu", glu=True, out="f32",
              b2=37, b2_extra=8)
        L("conv9x9-Cin64-b2-res", mode="conv", B=3, H=9, W=9, Cin=64, N=BN + 16, out="f32", b2=81, res=True)
        L("conv17x13-s2", mode="conv", B=3, H=17, W=13, Cin=128, N=BN, stride=2)
        L("conv10x14-s2-pad1", mode="conv", B=4, H=10, W=14, Cin=64, N=48, stride=2, pad_mode=1, out="f32")
        L("up5x7-Cin320", mode="up", B=2, H=5, W=7, Cin=320, N=BN - 16 if BN > 16 else 16, res=True)
    return out


# one row per ping-pong specialization in launch_t (variants 1-3 excluded); each carries its paired edge cases. Keys as kernel_of().
def _pp_lin16(act, glu, bn):
    k = ("pp", bn, "SX_A_LINEAR", False, {None: "SX_ACT_NONE", "gelu": "SX_ACT_GELU", "silu": "SX_ACT_SILU"}[act], glu, 0)
    return k, dict(act=act, glu=glu)


def pp_spec_table():
    specs = []
    for bn in (256, 320):
        for act, glu in ((None, False), ("gelu", False), ("gelu", True), ("silu", True)):
            if glu and bn == 320:
                continue
            k, kw = _pp_lin16(act, glu, bn)
            specs.append((k, dict(mode="lin", out="16", **kw)))
        specs.append((("pp", bn, "SX_A_LINEAR", True, "SX_ACT_NONE", False, 0), dict(mode="lin", out="f32")))
        for mode, am in (("conv", "SX_A_CONV3X3"), ("up", "SX_A_CONV3X3_UP")):
            for o in ("16", "f32"):
                specs.append((("pp", bn, am, o == "f32", "SX_ACT_NONE", False, 0), dict(mode=mode, out=o)))
        specs.append((("pp", bn, "SX_A_LINEAR", True, "SX_ACT_NONE", False, 2), dict(mode="lin", out="f32", ln="prod")))
        specs.append((("pp", bn, "SX_A_LINEAR", False, "SX_ACT_NONE", False, 1), dict(mode="lin", out="16", ln="cons")))
    specs.append((("pp", 256, "SX_A_LINEAR", False, "SX_ACT_GELU", True, 1), dict(mode="lin", out="16", act="gelu", glu=True,
                                                                                      ln="cons")))
    return specs


PP_SPECS = pp_spec_table()


def pp_cases(dt):
    out = []
    for key, s in PP_SPECS:
        bn = key[1]
        t = 7 if bn == 256 else 8
        name = f"pp{bn}-{s['mode']}-{s['out']}-{s.get('act') or 'none'}{'-glu' if s.get('glu') else ''}" + \
               (f"-ln{s['ln']}" if s.get("ln") else "")
        P = lambda tag, **kw: out.append(case(f"{name}-{tag}-{dt}", dt, t, **{**s, **kw}))
        glu = s.get("glu", False)
        if s["mode"] == "lin" and s.get("ln") == "prod":
            P("tailM-res-K1664", M=3 * 256 + 1, N=bn + 16, K=1664, res=True, ldr_extra=4)
            P("smallM-K64", M=200, N=2 * bn - 16, K=64, bias=False)
        elif s["mode"] == "lin" and s.get("ln") == "cons":
            P("tailM-K640", M=513, N=bn + 64 if not glu else 2 * bn, K=640, ldc_extra=8 if not glu else 4)
            P("smallM-K128", M=255, N=32 if glu else 16, K=128, c_off=4)
        elif s["mode"] == "lin":
            n2 = 32 if glu else 16
            nt = 2 * bn + 64 if glu else 3 * bn - 48          # N % BN != 0
            # M = BM*k + 1, N = BN + n2 (GLU: N % 32), 26 k-tiles; residual (initial value or epilogue load) with ldr > n_out,
            # straddling bias2d (100 rows) with ld_bias2d > N, ldc % 8 != 0 (narrow stores)
            P("tailM-K1664-res-b2-ldc4", M=3 * 256 + 1, N=bn + (32 if glu else 16), K=1664, res=True, ldr_extra=8, b2=100,
              b2_extra=12, ldc_extra=4)
            P("smallM-N16-K64", M=255, N=n2, K=64, bias=False)
            # long K, N tail, n_valid < n_out (GLU: ragged against the 32-column wide stores), ldc % 8 == 0 > n_store, res_mod
            nv = (nt // 2 if glu else nt) - 20
            P("longK-Ntail-nvalid-ldc8-resmod", M=512, N=nt, K=5760, n_valid=nv, ldc_extra=4 if nv % 8 == 4 else 8, res=True,
              res_mod=300, b2=512, b2_extra=4)
            # 25 k-tiles (odd count: the k loop runs tile pairs), C misaligned by 8 bytes (narrow stores although ldc % 8 == 0)
            P("oddK-cmisaligned", M=511, N=2 * bn, K=1600, c_off=4, b2=256)
            if s["out"] == "f32":
                P("planes2-resmod", M=3 * 256 - 1, N=bn + 16, K=640, planes=2, res=True, res_mod=77)
        else:
            up = s["mode"] == "up"
            if up:
                P("up5x7-Cin64", B=3, H=5, W=7, Cin=64, N=bn + 16, res=True)
                P("up3x5-Cin640-b2", B=6, H=3, W=5, Cin=640, N=bn - 16, b2=60, b2_extra=8, ldr_extra=4, res=True)
                P("up9x3-Cin320-smallM", B=1, H=9, W=3, Cin=320, N=16, bias=False)
            else:
                P("9x9-Cin64", B=4, H=9, W=9, Cin=64, N=bn + 16)
                P("10x14-Cin320-b2-res", B=3, H=10, W=14, Cin=320, N=bn - 16, b2=140, b2_extra=4, res=True, ldr_extra=4)
                P("17x13-s2", B=5, H=17, W=13, Cin=64, N=2 * bn, stride=2, b2=63)
                P("10x14-s2-pad1", B=9, H=10, W=14, Cin=128, N=bn, stride=2, pad_mode=1, res=True)
                P("6x6-Cin1280", B=8, H=6, W=6, Cin=1280, N=bn + 16, b2=36)
    return out


def traversal_cases():
    """Tile grids of >= 16 tiles that split unevenly over the 8 XCDs, with the 2-D partition off / on and forced gm (last
    traversal group shorter than gm)."""
    out = []
    for dt in ("f16", "bf16"):
        out += [
            case(f"trav-t7-xcd0-{dt}", dt, 7, M=256 * 11 - 3, N=256 * 3 - 16, K=256, res=True, out="f32", xcd=0),
            case(f"trav-t7-gm3-{dt}", dt, 7, M=256 * 11 - 3, N=256 * 3 - 16, K=256, res=True, out="f32", xcd=1, gm=3),
            case(f"trav-t8-gm4-{dt}", dt, 8, M=256 * 5 + 7, N=320 * 5 - 16, K=192, xcd=1, gm=4),
            case(f"trav-t8-conv-gm2-{dt}", dt, 8, mode="conv", B=3, H=33, W=31, Cin=64, N=320 * 3 - 32, xcd=1, gm=2, out="f32"),
            case(f"trav-t3-gm5-{dt}", dt, 3, M=64 * 21 + 5, N=64 * 9 - 16, K=128, xcd=1, gm=5),
            case(f"trav-t3-xcd0-{dt}", dt, 3, M=64 * 21 + 5, N=64 * 9 - 16, K=128, xcd=0),
            case(f"trav-t0-conv-gm3-{dt}", dt, 0, mode="conv", B=2, H=29, W=31, Cin=64, N=400, xcd=1, gm=3),
            case(f"trav-t6-gm6-{dt}", dt, 6, M=256 * 13 + 1, N=160 * 3 - 16, K=128, xcd=1, gm=6),
        ]
    return out


def plan_grid(M, N, K, BM, BN, xcd_2d, gm_force):
    """gemm_common.h plan_grid: (tiles_m, tiles_n, xm, xn, gm, launch grid)."""
    tm, tn = (M + BM - 1) // BM, (N + BN - 1) // BN
    grid, xm, xn, gm = tm * tn, 0, 0, 1
    if grid >= 16 and xcd_2d:
        ab, wb, best = float(M) * K, float(N) * K, 1e300
        for cxm in (1, 2, 4, 8):
            cxn = 8 // cxm
            if cxm > tm or cxn > tn:
                continue
            padded = 8 * ((tm + cxm - 1) // cxm) * ((tn + cxn - 1) // cxn)
            cost = (ab * cxn + wb * cxm) * (1.0 + 4.0 * (padded - grid) / grid)
            if cost < best:
                best, xm, xn = cost, cxm, cxn
        if xm:
            grid = 8 * ((tm + xm - 1) // xm) * ((tn + xn - 1) // xn)
        gm = gm_force if gm_force else 8
    return tm, tn, xm, xn, gm, grid


# ---- production launches ---------------------------------------------------------------------------------------------------
UNET_B = 32                   # CFG rows of the bench's config-0 UNet step
TEMB_LD = 13760               # temb_all row: every resnet's time-embedding add side by side (sum of the resnets' Co)


def production_cases():
    """Each distinct GEMM / conv launch of the config-0 UNet step (SDXL: 128^2 latents, channels 320 / 640 / 1280, transformer
    depths 0 / 2 / 10, LayerNorm folded at this batch) at 32 CFG rows, and of the ViT-G/448 (1024 tokens, width 1664, MLP 8192)
    at 20 and 32 crops. fp16 (the bench dtype), automatic tile choice."""
    B, out = UNET_B, []
    P = lambda cid, **kw: out.append(case("prod-" + cid, "f16", None, subset=True, **kw))
    for hw, c in ((128, 320), (64, 640), (32, 1280)):
        # resnet convs: conv1 + per-sample time add (bias2d rows = H*W, ld = the whole temb row), conv2 + residual
        P(f"conv{hw}-{c}-b2", mode="conv", B=B, H=hw, W=hw, Cin=c, N=c, out="f32", b2=hw * hw, b2_extra=TEMB_LD - c,
          sample_rows=hw * hw)
        P(f"conv{hw}-{c}-res", mode="conv", B=B, H=hw, W=hw, Cin=c, N=c, out="f32", res=True, sample_rows=hw * hw)
    P("down128-320", mode="conv", B=B, H=128, W=128, Cin=320, N=320, stride=2, out="f32", sample_rows=64 * 64)
    P("down64-640", mode="conv", B=B, H=64, W=64, Cin=640, N=640, stride=2, out="f32", sample_rows=32 * 32)
    P("conv64-320to640-b2", mode="conv", B=B, H=64, W=64, Cin=320, N=640, out="f32", b2=4096, b2_extra=TEMB_LD - 640,
      sample_rows=4096)
    P("conv32-640to1280-b2", mode="conv", B=B, H=32, W=32, Cin=640, N=1280, out="f32", b2=1024, b2_extra=TEMB_LD - 1280,
      sample_rows=1024)
    for hw, cin, co in ((32, 2560, 1280), (32, 1920, 1280), (64, 1920, 640), (64, 1280, 640), (64, 960, 640), (128, 960, 320),
                        (128, 640, 320)):   # up-block conv1 over [x | skip]
        P(f"upres{hw}-{cin}to{co}-b2", mode="conv", B=B, H=hw, W=hw, Cin=cin, N=co, out="f32", b2=hw * hw,
          b2_extra=TEMB_LD - co, sample_rows=hw * hw)
        P(f"short{hw}-{cin}to{co}", M=B * hw * hw, N=co, K=cin, out="f32", sample_rows=hw * hw)     # 1x1 shortcut
    P("short64-320to640", M=B * 4096, N=640, K=320, out="f32", sample_rows=4096)
    P("short32-640to1280", M=B * 1024, N=1280, K=640, out="f32", sample_rows=1024)
    P("upconv32-1280", mode="up", B=B, H=32, W=32, Cin=1280, N=1280, out="f32", sample_rows=4096)
    P("upconv64-640", mode="up", B=B, H=64, W=64, Cin=640, N=640, out="f32", sample_rows=16384)
    P("convout128", mode="conv", B=B, H=128, W=128, Cin=320, N=16, n_valid=4, out="f32", sample_rows=16384)
    P("convin128", M=B * 16384, N=320, K=64, out="f32", sample_rows=16384)     # conv_in: im2col (36 -> 64 wide K) + GEMM
    for hw, c in ((64, 640), (32, 1280)):
        M = B * hw * hw
        P(f"pin{c}", M=M, N=c, K=c, out="f32", ln="prod", sample_rows=hw * hw)
        P(f"qkv{c}", M=M, N=3 * c, K=c, ln="cons", bias=True, sample_rows=hw * hw)
        P(f"q2-{c}", M=M, N=c, K=c, ln="cons", sample_rows=hw * hw)
        P(f"out{c}", M=M, N=c, K=c, out="f32", res=True, ln="prod", sample_rows=hw * hw)
        P(f"geglu{c}", M=M, N=8 * c, K=c, act="gelu", glu=True, ln="cons", sample_rows=hw * hw)
        P(f"ff2-{c}", M=M, N=c, K=4 * c, out="f32", res=True, ln="prod", sample_rows=hw * hw)
        P(f"ff2last{c}", M=M, N=c, K=4 * c, res=True, sample_rows=hw * hw)
        P(f"pout{c}", M=M, N=c, K=c, out="f32", res=True, sample_rows=hw * hw)
    P("temb1", M=B, N=1280, K=320, act="silu")
    P("tembw", M=B, N=TEMB_LD, K=1280, out="f32")
    for crops in (20, 32):                          # ViT-G/448
        M = crops * 1024
        P(f"vit{crops}-patch", M=M, N=1664, K=640, out="f32", bias=False, res=True, res_mod=1024, sample_rows=1024)
        P(f"vit{crops}-qkv", M=M, N=4992, K=1664, sample_rows=1024)
        P(f"vit{crops}-out", M=M, N=1664, K=1664, out="f32", res=True, sample_rows=1024)
        P(f"vit{crops}-fc", M=M, N=8192, K=1664, act="gelu", sample_rows=1024)
        P(f"vit{crops}-proj", M=M, N=1664, K=8192, out="f32", res=True, sample_rows=1024)
    # A operand of 1.63 GiB (just under the 2-GiB buffer-descriptor limit): 32-bit offset arithmetic near the top of the range
    for t in (None, 2):
        out.append(case("bigA-" + (f"t{t}" if t is not None else "auto"), "f16", t, M=524288 - 37, N=320, K=1664, subset=True))
    return out


CASES = [c for dt in DTYPES for c in lockstep_cases(dt) + pp_cases(dt)] + traversal_cases()
PROD = production_cases()


# ----------------------------------------------------------------------------------------------------------------------------
# buffers
# ----------------------------------------------------------------------------------------------------------------------------
def _ibits(dtype):
    return torch.int16 if dtype in (F16, BF16) else torch.int32


def _signed(bits, dtype):
    """The bit pattern as the signed integer that torch's int16 / int32 view of dtype holds."""
    nb = 16 if dtype in (F16, BF16) else 32
    return bits - (1 << nb) if bits >= 1 << (nb - 1) else bits


def _nanbuf(n, dtype, dev, bits=None):
    """n elements of dtype, every one a NaN bit pattern."""
    buf = torch.empty(n, dtype=dtype, device=dev)
    if bits is None:
        bits = NAN16_IN if dtype in (F16, BF16) else NAN32_IN
    buf.view(_ibits(dtype)).fill_(_signed(bits, dtype))
    return buf


def guarded(shape, dtype, dev, gen, scale=1.0, ld=None, pad=256):
    """A random tensor of `shape` (rows x cols; ld >= cols = row stride) as a leading view of a NaN-filled buffer: pad columns and
    `pad` trailing elements stay NaN. Returns (view of the logical values, the full row-strided 2-D view or the tensor)."""
    rows = math.prod(shape[:-1])
    cols = shape[-1]
    ld = ld or cols
    buf = _nanbuf(rows * ld + pad, dtype, dev)
    full = buf[:rows * ld].view(rows, ld)
    full[:, :cols] = (torch.randn(rows, cols, device=dev, generator=gen) * scale).to(dtype)
    return full[:, :cols].view(*shape[:-1], cols) if ld == cols else full[:, :cols], full


class OutBuf:
    """C inside a guard buffer: c_off elements before it, 3 extra rows after M, columns up to ldc, 64 elements behind."""
    XROWS, TAIL = 3, 64

    def __init__(self, M, n_store, ldc, c_off, dtype, dev):
        self.M, self.n, self.ldc, self.off, self.dtype = M, n_store, ldc, c_off, dtype
        self.bits = NAN16_GUARD if dtype in (F16, BF16) else NAN32_GUARD
        self.buf = _nanbuf(c_off + (M + self.XROWS) * ldc + self.TAIL, dtype, dev, self.bits)
        self.mat = self.buf[c_off:c_off + M * ldc].view(M, ldc)

    def ptr(self):
        return self.mat.data_ptr()

    def logical(self):
        return self.mat[:, :self.n]

    def untouched(self):
        return bool((self.buf.view(_ibits(self.dtype)) == _signed(self.bits, self.dtype)).all())

    def check_guard(self, what):
        ib, bits = _ibits(self.dtype), _signed(self.bits, self.dtype)
        mask = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        mask[self.off:self.off + self.M * self.ldc].view(self.M, self.ldc)[:, :self.n] = False
        bad = (self.buf.view(ib) != bits) & mask
        nbad = int(bad.sum())
        if nbad:
            i = int(bad.nonzero()[0, 0]) - self.off
            r, col = (i // self.ldc, i % self.ldc) if i >= 0 else (-1, i)
            raise AssertionError(f"{what}: {nbad} elements outside the logical [{self.M}, {self.n}] output (ldc {self.ldc}) were "
                                 f"written; first at row {r}, column {col}")
        lg = self.logical()
        fin = torch.isfinite(lg)
        if not bool(fin.all()):
            r, col = (~fin).nonzero()[0].tolist()
            raise AssertionError(f"{what}: {int((~fin).sum())} non-finite elements inside the output (first at row {r}, column {col}): "
                                 f"an unwritten element or an unmasked read past an input")


# ----------------------------------------------------------------------------------------------------------------------------
# launch
# ----------------------------------------------------------------------------------------------------------------------------
class Forced:
    """sx_gemm_force_tile state of one case; always restored to the defaults (-1, 101, 300)."""

    def __init__(self, lib, c):
        self.lib, self.c = lib, c

    def __enter__(self):
        c = self.c
        if c["tile"] is not None:
            assert self.lib.sx_gemm_force_tile(c["tile"]) == 0
        if c["xcd"] is not None:
            assert self.lib.sx_gemm_force_tile(100 + c["xcd"]) == 0
        if c["gm"] is not None:
            assert self.lib.sx_gemm_force_tile(300 + c["gm"]) == 0

    def __exit__(self, *exc):
        restore_defaults(self.lib)
        return False


def restore_defaults(lib):
    lib.sx_gemm_force_tile(-1)
    lib.sx_gemm_force_tile(101)
    lib.sx_gemm_force_tile(300)


def make_inputs(c, dev):
    """Random operands of a case, each a leading view of a NaN-padded buffer."""
    dtype = DTYPES[c["dt"]]
    gen = torch.Generator(device=dev).manual_seed(zlib.crc32(c["id"].encode()))
    M, N, K = c["M"], c["N"], c["K"]
    n_out = N // 2 if c["glu"] else N
    n_store = c["n_valid"] or n_out
    I = dict(dtype=dtype, n_out=n_out, n_store=n_store)
    if c["mode"] == "lin":
        I["A"], _ = guarded((M, K * c["planes"]), dtype, dev, gen)
        if c["planes"] == 2:       # [hi | lo]: lo ~ 2^-9 of hi, as sx_split16 writes it
            I["A"][:, K:] = (I["A"][:, K:].float() * 2.0 ** -9).to(dtype)
    else:
        I["A"], _ = guarded((c["B"], c["H"], c["W"], c["Cin"]), dtype, dev, gen)
    I["W"], _ = guarded((N, K), dtype, dev, gen, scale=K ** -0.5)
    I["bias"] = guarded((N,), torch.float32, dev, gen, pad=64)[0] if c["bias"] else None
    if c["b2"]:
        nb2 = (M + c["b2"] - 1) // c["b2"]
        I["b2"], I["b2full"] = guarded((nb2, N), torch.float32, dev, gen, ld=N + c["b2_extra"])
    if c["res"]:
        rr = c["res_mod"] or M
        I["res"], I["resfull"] = guarded((rr, n_store), torch.float32, dev, gen, ld=n_store + c["ldr_extra"])
    if c["ln"] == "cons":
        mu = torch.randn(M, device=dev, generator=gen, dtype=torch.float64) * 0.5
        var = torch.rand(M, device=dev, generator=gen, dtype=torch.float64) * 1.5 + 0.5
        I["stats"] = torch.stack([K * mu, K * (var + mu * mu)], dim=1).contiguous()
        I["cs"] = I["W"].float().sum(dim=1).contiguous()       # colsum of the (gamma-folded) 16-bit weight, as ops.fold_layernorm
    return I


def out_buf(c, I, dev):
    odt = {"f32": torch.float32, "16": I["dtype"], "other16": BF16 if I["dtype"] == F16 else F16}[c["out"]]
    return OutBuf(c["M"], I["n_store"], I["n_store"] + c["ldc_extra"], c["c_off"], odt, dev)


def launch(lib, c, I, dev, ob=None):
    """One sx_gemm / sx_gemm_ln launch into fresh guard buffers (or `ob`). Returns (OutBuf, LayerNorm-producer (x16 OutBuf, stats)
    or None)."""
    from seedx_amd import _lib
    dtype = I["dtype"]
    ob = ob or out_buf(c, I, dev)
    ldc = ob.ldc
    a = _lib.GemmArgs()
    a.A, a.W, a.C = I["A"].data_ptr(), I["W"].data_ptr(), ob.ptr()
    a.bias = I["bias"].data_ptr() if I["bias"] is not None else None
    if c["b2"]:
        a.bias2d, a.bias2d_rows, a.ld_bias2d = I["b2full"].data_ptr(), c["b2"], I["b2full"].stride(0)
    if c["res"]:
        a.residual, a.ldr, a.res_mod = I["resfull"].data_ptr(), I["resfull"].stride(0), c["res_mod"]
    a.M, a.N, a.K, a.ldc, a.n_valid = c["M"], c["N"], c["K"], ldc, c["n_valid"]
    a.dtype = _lib.SX_F16 if dtype == F16 else _lib.SX_BF16
    a.out_dtype = {torch.float32: _lib.SX_F32, F16: _lib.SX_F16, BF16: _lib.SX_BF16}[ob.dtype]
    a.act = {None: _lib.SX_ACT_NONE, "gelu": _lib.SX_ACT_GELU, "silu": _lib.SX_ACT_SILU}[c["act"]]
    a.glu = 1 if c["glu"] else 0
    a.a_planes = c["planes"]
    if c["mode"] == "lin":
        a.a_mode = _lib.SX_A_LINEAR
    else:
        a.a_mode = _lib.SX_A_CONV3X3
        a.B, a.Hin, a.Win, a.Cin, a.Hout, a.Wout = c["B"], c["H"], c["W"], c["Cin"], c["Hout"], c["Wout"]
        a.stride, a.upsample, a.pad_mode = c["stride"], 1 if c["mode"] == "up" else 0, c["pad_mode"]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    prod = None
    with Forced(lib, c):
        if c["ln"] is None:
            st = lib.sx_gemm(C.byref(a), stream)
        else:
            la = _lib.GemmLnArgs()
            if c["ln"] == "prod":
                xb = OutBuf(c["M"], c["N"], c["N"] + 8, 0, dtype, dev)
                stats = torch.zeros(c["M"], 2, dtype=torch.float64, device=dev)
                la.x16_out, la.ld_x16, la.row_stats_out = xb.ptr(), xb.ldc, stats.data_ptr()
                prod = (xb, stats)
            else:
                la.row_stats_in, la.colsum, la.dim, la.eps = I["stats"].data_ptr(), I["cs"].data_ptr(), c["K"], 1e-5
            st = lib.sx_gemm_ln(C.byref(a), C.byref(la), stream)
    _lib.check(st, f"sx_gemm case {c['id']}")
    torch.cuda.synchronize()
    return ob, prod


# ----------------------------------------------------------------------------------------------------------------------------
# fp64 reference and bound
# ----------------------------------------------------------------------------------------------------------------------------
def im2col64(c, x, rows):
    """fp64 [len(rows), 9*Cin] implicit-GEMM operand of the conv for the given output rows ((ky, kx, cin) order, zero padding,
    nearest-2x upsampling, stride and pad_mode exactly as the sx_gemm contract)."""
    B, H, W, Cin = x.shape
    up = c["mode"] == "up"
    Hv, Wv = (2 * H, 2 * W) if up else (H, W)
    pad = 0 if c["pad_mode"] else 1
    hw = c["Hout"] * c["Wout"]
    b, rem = rows // hw, rows % hw
    oy, ox = rem // c["Wout"], rem % c["Wout"]
    d = torch.arange(3, device=x.device)
    vy = (oy * c["stride"] - pad)[:, None, None] + d[None, :, None]        # [R, 3 (ky), 1]
    vx = (ox * c["stride"] - pad)[:, None, None] + d[None, None, :]        # [R, 1, 3 (kx)]
    ok = (vy >= 0) & (vy < Hv) & (vx >= 0) & (vx < Wv)                      # [R, 3, 3]
    sy, sx = vy.clamp(0, Hv - 1), vx.clamp(0, Wv - 1)
    if up:
        sy, sx = sy // 2, sx // 2
    flat = (b[:, None, None] * H + sy) * W + sx                             # [R, 3, 3]
    cols = x.reshape(B * H * W, Cin)[flat.reshape(-1)].double().view(len(rows), 9, Cin)
    cols *= ok.reshape(len(rows), 9, 1)
    return cols.reshape(len(rows), 9 * Cin)


def act64(x, act):
    if act == "gelu":
        return 0.5 * x * (1.0 + torch.erf(x * 0.5 ** 0.5))
    if act == "silu":
        return x * torch.sigmoid(x)
    return x


def half_ulp(x, dtype):
    """Half the spacing of dtype at magnitude x (fp64 in, fp64 out; subnormal spacing below the smallest normal)."""
    p, emin = {F16: (11, -14), BF16: (8, -126), torch.float32: (24, -126)}[dtype]
    _, e = torch.frexp(x)
    e = torch.where(x > 0, e.to(torch.int64) - 1, emin).clamp(min=emin)
    return torch.pow(2.0, (e - p).to(torch.float64))


def reference(c, I, rows):
    """fp64 reference and per-element bound of the rows `rows` of the logical output [M, n_store].

    error_bound: the kernel multiplies the same 16-bit operands exactly and accumulates in fp32 (MFMA, then the fp32 epilogue), so
      |y - ref| <= L * C_ACC * sqrt(Kk) * 2^-24 * mag  +  C_EP * 2^-24 * (magnitudes of the epilogue's fp32 operations)  +  1/2 ulp_out,
    where mag = (|A| |W|^T)_mn + |bias_n| + |bias2d_mn| (+ |residual_mn| when it is the accumulators' initial value) bounds every
    partial sum, Kk the summed length (2K with a_planes = 2) and L the activation's Lipschitz constant (GLU: |act(gate)| on the
    linear half's error, L |linear| on the gate's). Rounding errors of a length-n fp32 sum whose partial sums stay below mag are at
    most n * 2^-24 * mag in the worst case and grow like sqrt(n) * 2^-24 * mag for independent roundings (Higham, Accuracy and
    Stability, 2nd ed., §3.1 / §4.2); C_ACC = 4 covers 4 standard deviations of that random walk with room to spare, since the
    partial sums of these random operands stay far below mag. The epilogue term (C_EP = 8) covers the A&S erf approximation of the
    GELU (|error| <= 1.5e-7 ~ 2.5 * 2^-24), rcp / exp of the SiLU and the fused multiply-adds. A LayerNorm consumer multiplies the
    accumulator by rstd and subtracts rstd mu colsum: its terms scale with |rstd| and |rstd mu colsum|. The output rounding is half a
    unit in the last place of the output dtype at max(|ref| + bound, |y|)."""
    dtype, n_out, n_store = I["dtype"], I["n_out"], I["n_store"]
    K = c["K"]
    W64 = I["W"].double()
    Wabs = W64.abs()
    if c["mode"] == "lin":
        a = I["A"][rows].double()
        if c["planes"] == 2:
            z = a[:, :K] @ W64.t() + a[:, K:] @ W64.t()
            S = a[:, :K].abs() @ Wabs.t() + a[:, K:].abs() @ Wabs.t()
        else:
            z, S = a @ W64.t(), a.abs() @ Wabs.t()
    else:
        a = im2col64(c, I["A"], rows)
        z, S = a @ W64.t(), a.abs() @ Wabs.t()
    del a
    Kk = K * c["planes"]
    acc_c = C_ACC * math.sqrt(Kk) * U32
    bias = I["bias"].double()[None, :] if I["bias"] is not None else torch.zeros(1, c["N"], dtype=torch.float64, device=z.device)
    res_init = c["res"] and c["act"] is None and not c["glu"]
    res = None
    if c["res"]:
        rrows = rows % c["res_mod"] if c["res_mod"] else rows
        res = I["res"][rrows].double()                                       # [R, n_store]
    if c["ln"] == "cons":
        st = I["stats"][rows]
        mu = st[:, 0:1] / K
        rstd = 1.0 / torch.sqrt(st[:, 1:2] / K - mu * mu + 1e-5)
        cs = I["cs"].double()[None, :]
        pre = rstd * (z - mu * cs) + bias
        err = rstd * acc_c * S + C_EP * U32 * (rstd * z.abs() + (rstd * mu * cs).abs() + bias.abs())
    else:
        pre = z + bias
        mag = S + bias.abs()
        if c["b2"]:
            b2 = I["b2"][rows // c["b2"]].double()
            pre = pre + b2
            mag = mag + b2.abs()
        if res_init:
            rfull = torch.zeros_like(pre)
            rfull[:, :n_store] = res
            pre = pre + rfull
            mag = mag + rfull.abs()
        err = acc_c * mag
    L = LIP[c["act"]]
    if c["glu"]:
        R = pre.shape[0]
        pv = pre.view(R, -1, 2, 16)
        ev = err.view(R, -1, 2, 16)
        v, g = pv[:, :, 0].reshape(R, n_out), pv[:, :, 1].reshape(R, n_out)
        e_v, e_g = ev[:, :, 0].reshape(R, n_out), ev[:, :, 1].reshape(R, n_out)
        ag = act64(g, c["act"])
        ref = v * ag
        err = ag.abs() * e_v + v.abs() * (L * e_g + C_EP * U32 * g.abs()) + C_EP * U32 * ref.abs()
    elif c["act"] is not None:
        ref = act64(pre, c["act"])
        err = L * err + C_EP * U32 * pre.abs()
    else:
        ref = pre
    ref, err = ref[:, :n_store], err[:, :n_store]
    if c["res"] and not res_init:
        ref = ref + res
        err = err + 2 * U32 * (ref.abs() + res.abs())
    return ref, err


def check_against_reference(c, I, y, rows, what):
    odt = y.dtype
    ref, err = reference(c, I, rows)
    y64 = y[rows].double()
    bound = err + half_ulp(torch.maximum(ref.abs() + err, y64.abs()), odt)
    d = (y64 - ref).abs()
    ratio = d / bound
    worst = int(ratio.argmax())
    r, col = divmod(worst, ratio.shape[1])
    if float(ratio.max()) > 1.0:
        BM, BN, _ = TILES[c["tile"]] if c["tile"] is not None else (256, 256, True)
        ncol = 32 * (col // 16) + col % 16 if c["glu"] else col
        row = int(rows[r])
        nbad = int((ratio > 1.0).sum())
        raise AssertionError(f"{what}: {nbad} elements beyond the fp64 bound; worst at row {row}, column {col} (tile {row // BM}, "
                             f"{ncol // BN} of {BM}x{BN}"
                             f"{'' if c['tile'] is not None else ', automatic tile: coordinates for 256x256'}): got {float(y64[r, col])!r}, "
                             f"ref {float(ref[r, col])!r}, |diff| {float(d[r, col]):.3e} > bound {float(bound[r, col]):.3e}")
    rel = float((y64 - ref).norm() / ref.norm().clamp_min(1e-30))
    assert rel < TOL[odt], f"{what}: rel-L2 {rel:.3e} vs fp64 >= {TOL[odt]}"


def subset_rows(M, sample_rows, dev, seed):
    """Every row within 2 of a 256-row tile boundary or of a sample boundary, the last rows, and 4096 random rows."""
    m = torch.arange(M, device=dev)
    keep = ((m % 256) < 2) | ((m % 256) >= 254) | (m >= M - 2)
    if sample_rows and sample_rows < M:
        keep |= ((m % sample_rows) < 2) | ((m % sample_rows) >= sample_rows - 2)
    g = torch.Generator(device=dev).manual_seed(seed)
    keep[torch.randint(0, M, (4096,), device=dev, generator=g)] = True
    return keep.nonzero().view(-1)


def run_case(c, dev):
    from seedx_amd import _lib
    lib = _lib.load()
    I = make_inputs(c, dev)
    ob, prod = launch(lib, c, I, dev)
    what = c["id"]
    ob.check_guard(what)
    rows = subset_rows(c["M"], c["sample_rows"], dev, 5) if c["subset"] else torch.arange(c["M"], device=dev)
    y = ob.logical()
    check_against_reference(c, I, y, rows, what)
    if prod is not None:                # LayerNorm producer: 16-bit copy of the stored output and its rows' fp64 sums
        xb, stats = prod
        xb.check_guard(what + " (x16 copy)")
        assert torch.equal(xb.logical().view(_ibits(I["dtype"])), y.to(I["dtype"]).view(_ibits(I["dtype"]))), \
            f"{what}: x16 != the stored output rounded to the operand dtype"
        h = y[rows].double()
        ref_st = torch.stack([h.sum(1), (h * h).sum(1)], dim=1)
        assert torch.allclose(stats[rows], ref_st, rtol=3e-6, atol=1e-3), f"{what}: row sums {(stats[rows] - ref_st).abs().max()}"
    ob2, _ = launch(lib, c, I, dev)
    ib = _ibits(y.dtype)
    assert torch.equal(ob2.logical().view(ib), y.view(ib)), f"{what}: two identical launches differ"


# ----------------------------------------------------------------------------------------------------------------------------
# tests
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in CASES if c["tile"] in LOCKSTEP_TILES and not c["id"].startswith("trav")],
                         ids=lambda c: c["id"])
def test_lockstep_tile(dev, c):
    run_case(c, dev)


@pytest.mark.parametrize("c", [c for c in CASES if c["tile"] in (7, 8) and not c["id"].startswith("trav")], ids=lambda c: c["id"])
def test_pingpong_specialization(dev, c):
    run_case(c, dev)


@pytest.mark.parametrize("c", [c for c in CASES if c["id"].startswith("trav")], ids=lambda c: c["id"])
def test_grid_traversal(dev, c):
    BM, BN, _ = TILES[c["tile"]]
    tm, tn, xm, xn, gm, grid = plan_grid(c["M"], c["N"], c["K"], BM, BN, c["xcd"], c["gm"] or 0)
    assert tm * tn >= 16
    if c["xcd"]:
        rms = [(xr + 1) * tm // xm - xr * tm // xm for xr in range(xm)]
        assert grid > tm * tn or len(set(rms)) > 1, "the case must split unevenly over the XCDs"
        assert any(rm % gm for rm in rms), "a traversal group must come out shorter than gm"
    run_case(c, dev)


@pytest.mark.parametrize("c", PROD, ids=lambda c: c["id"])
def test_production_launch(dev, c):
    run_case(c, dev)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("tile,kw", [
    (7, dict(out="f32", act="gelu")),                           # fp32 output carries no activation on the ping-pong tiles
    (8, dict(act="gelu", glu=True, N=640)),                     # GLU needs the 256-wide tile
    (7, dict(mode="conv", B=2, H=9, W=9, act="silu")),          # convs have no activation there
    (8, dict(mode="up", B=2, H=5, W=7, stride=2)),              # upsampling is stride 1 only
    (7, dict(out="other16")),                                   # 16-bit output of the other dtype
], ids=["f32-gelu", "t8-glu", "conv-silu", "up-stride2", "other16"])
def test_forced_pingpong_rejects_unsupported_epilogue(dev, dt, tile, kw):
    """Forcing a ping-pong tile on an epilogue it has no kernel for fails with the library's error and writes nothing (no silent
    fall-back to a lock-step kernel); the same launch on the automatic pick matches the fp64 reference."""
    from seedx_amd import _lib
    lib = _lib.load()
    c = case(f"neg-{dt}-t{tile}-{'-'.join(map(str, kw.values()))}", dt, tile, **{"M": 300, "N": 272, "K": 128, **kw})
    I = make_inputs(c, dev)
    ob = out_buf(c, I, dev)
    with pytest.raises(RuntimeError, match="forced ping-pong tile has no kernel"):
        launch(lib, c, I, dev, ob)
    torch.cuda.synchronize()
    assert ob.untouched(), "a refused launch wrote C"
    c = dict(c, tile=None)
    ob, _ = launch(lib, c, I, dev)
    ob.check_guard(c["id"])
    check_against_reference(c, I, ob.logical(), torch.arange(c["M"], device=dev), c["id"])


def test_defaults_restored_after_forcing(dev):
    """The matrix leaves the process-global tile state at its defaults: the picks test_gemm_tile_picker_host_logic asserts, no
    forced tile (a LayerNorm fold on a lock-step shape still fails loudly, an fp32 GELU launch runs)."""
    from seedx_amd import _lib, ops
    lib = _lib.load()
    assert lib.sx_gemm_pick_tile(32768, 3840, 1280, 0, 0) == 8 and lib.sx_gemm_pick_tile(32768, 10240, 1280, 1, 0) == 7
    assert lib.sx_gemm_pick_tile(262144, 320, 2880, 0, 1) == 8 and lib.sx_gemm_pick_tile(32768, 320, 2880, 0, 1) == 6
    a = torch.randn(2048, 1280, device=dev).to(F16)
    w = torch.randn(1280, 1280, device=dev).to(F16)
    with pytest.raises(RuntimeError, match="ping-pong"):
        ops.gemm(a, w, out_dtype=torch.float32, ln_emit=ops.LnRows(2048, 1280, F16, dev))
    y = ops.gemm(a[:300, :128].contiguous(), w[:272, :128].contiguous(), act="gelu", out_dtype=torch.float32)
    assert bool(torch.isfinite(y).all())
