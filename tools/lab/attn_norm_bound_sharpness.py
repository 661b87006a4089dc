"""Sharpness of the bounds of tests/test_attn_norm_matrix_gpu.py, without a GPU: each bound is fed an fp32 / 16-bit emulation of the
kernel's arithmetic on the CPU (the clean emulation must stay inside) and one mutant (which must leave it):
  * attention: the planted key of every row dropped from P;
  * GroupNorm: the variance from ONE sequential fp32 sum per group (E[x^2] - mean^2 in fp32) at mean / std = 300, against the
    kernel's order (8 rows per thread, the group's channel pairs, then fp64).
Run from the repository root: python tools/lab/attn_norm_bound_sharpness.py (profiles/attn_norm_matrix.md holds its output)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import test_attn_norm_matrix_gpu as m  # noqa: E402

F32 = torch.float32
dev = torch.device("cpu")


def attn_emulation(c, Q, K, V, scale, pos, drop):
    """fp32 scores, exp2 of one fma against the row maximum, P rounded to the operand type, fp32 sums of the rounded P (attn_kernel)."""
    dtype = m.DTYPES[c["dt"]]
    s = Q.float() @ K.float().transpose(-1, -2)
    cl = scale * 1.4426950408889634
    p = torch.exp2(s * cl - s.max(-1, keepdim=True)[0] * cl).to(dtype)
    if drop:
        n = len(pos)
        p[:, :, torch.arange(n), torch.tensor(pos)] = 0
    return ((p.float() @ V.float()) / p.float().sum(-1, keepdim=True)).to(dtype)


def attn_report():
    for dt in m.DTYPES:
        for D, Skv in ((64, 200), (128, 700), (40, 129)):
            c = m.acase("sharp", dt, B=1, H=2, Sq=130, Skv=Skv, D=D)
            Q, K, V, scale, pos = m.attn_inputs(c, dev)
            ref, A, s1 = m.attn_reference(c, Q, K, V, scale, pos)
            bound = m.attn_bound(c, ref, A, s1)
            for drop in (False, True):
                ratio = (attn_emulation(c, Q, K, V, scale, pos, drop).double() - ref).abs() / bound
                rows = ratio[:, :, :len(pos)].amax(-1)
                print(f"attention {dt:5s} D {D:3d} Skv {Skv:3d} {'planted key dropped' if drop else 'clean emulation   '}: worst |diff| / bound "
                      f"{float(ratio.max()):10.3f}, planted rows beyond the bound {int((rows > 1).sum())} of {rows.numel()}")


def gn_emulation(c, x, gamma, beta, one_pass, eps=1e-5):
    B, HW, C, G = x.shape[0], x.shape[1], c["C"], c["groups"]
    cpg = C // G
    if one_pass:
        xs = x.view(B, HW, G, cpg).permute(0, 2, 1, 3).reshape(B, G, HW * cpg)
        s, q = torch.zeros(B, G), torch.zeros(B, G)
        for i in range(xs.shape[2]):
            s, q = s + xs[..., i], q + xs[..., i] * xs[..., i]
        mean = s / (HW * cpg)
        var = (q / (HW * cpg) - mean * mean).clamp_min(0).double()
        mean = mean.double()
    else:
        rs = m.gn_rows(c)[1]
        s, q = torch.zeros(B, G, dtype=torch.float64), torch.zeros(B, G, dtype=torch.float64)
        for r0 in range(0, HW, rs):
            ps, pq = torch.zeros(B, C // 2), torch.zeros(B, C // 2)                # per channel pair, rows in order
            for r in range(r0, min(HW, r0 + rs)):
                v = x[:, r].view(B, C // 2, 2)
                ps, pq = ps + (v[..., 0] + v[..., 1]), pq + (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1])
            gs, gq = torch.zeros(B, G), torch.zeros(B, G)
            for k in range(cpg // 2):                                              # the group's pairs in index order
                gs, gq = gs + ps.view(B, G, cpg // 2)[..., k], gq + pq.view(B, G, cpg // 2)[..., k]
            s, q = s + gs.double(), q + gq.double()
        mean = s / (HW * cpg)
        var = (q / (HW * cpg) - mean * mean).clamp_min(0)
    rstd = (1.0 / torch.sqrt(var + eps)).float()
    sc = gamma.view(G, cpg) * rstd[..., None]                                      # [B, G, cpg]
    sh = beta.view(G, cpg) - mean.float()[..., None] * sc
    return (x.view(B, HW, G, cpg) * sc[:, None] + sh[:, None]).view(B, HW, C)


def gn_report():
    for ratio in (30.0, 300.0):
        c = m.gcase("sharp", B=1, HW=4096, C=320, out="f16", raw=False, silu=False)
        x, gamma, beta = m.gn_inputs(c, dev)
        x = x + ratio
        ref, err, _ = m.gn_reference(c, x, gamma, beta)
        bound = err + m.rnd(ref, torch.float16)
        for one_pass in (False, True):
            y = gn_emulation(c, x, gamma, beta, one_pass).to(torch.float16).double()
            r = (y - ref).abs() / bound
            print(f"groupnorm mean/std {ratio:5.0f} {'one-pass fp32 variance' if one_pass else 'clean emulation       '}: worst |diff| / bound "
                  f"{float(r.max()):10.3f}, elements beyond the bound {int((r > 1).sum())} of {r.numel()}")


if __name__ == "__main__":
    torch.manual_seed(0)
    attn_report()
    gn_report()
