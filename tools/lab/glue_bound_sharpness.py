"""Sharpness of the bounds of the bounded group of tests/test_glue_matrix_gpu.py, without a GPU: an fp32 restatement of each kernel's arithmetic
(torch on the CPU, the operations in the kernel's order, the output rounded to the case's type) runs on the test's own inputs and is held to the
test's own fp64 references and bounds. Printed per case: the worst |diff| / bound.
  * every figure must be below 1: the restatement alone stays inside the bounds;
  * per kernel the figure of at least one case must be above 0.05: the bound is not vacuous.
Run from the repository root: python tools/lab/glue_bound_sharpness.py (profiles/glue_matrix.md holds its output). Exit status 1 if either fails."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import restated_unet as ru  # noqa: E402
from tests import test_glue_matrix_gpu as m  # noqa: E402

F32 = torch.float32
dev = torch.device("cpu")
FIG = {}                 # kernel -> [(case id, worst ratio)]


def note(kernel, cid, got, ref, bound):
    r = float(((got.double() - ref).abs() / bound).max())
    FIG.setdefault(kernel, []).append((cid, r))
    print(f"{kernel:28s} {cid:48s} worst |diff| / bound {r:8.4f}")


def avgpool():
    for c in m.AVGPOOL:
        x = m.avgpool_inputs(c, dev)
        B, L, D, k = c["B"], c["L"], c["D"], c["k"]
        xv = x.view(B, L // k, k, D)
        s = torch.zeros(B, L // k, D)
        for j in range(k):
            s = s + xv[:, :, j]
        ref, bound = m.avgpool_ref(x, k)
        note("avgpool_tokens_kernel", c["id"], s * torch.tensor(1.0 / k, dtype=F32), ref, bound)


def silu():
    for c in m.SILU:
        dt = m.DTYPES[c["dt"]]
        x = m.silu_inputs(c, dev)
        keep = x != float("-inf")
        y = (x.double() / (1.0 + torch.exp(-x.double()))).float().to(dt)          # silu_cast_kernel: exponential and quotient in fp64, rounded to fp32 once
        ref, bound = m.silu_ref(x, dt)
        note("silu_cast_kernel", c["id"], y[keep], ref[keep], bound[keep])


def l2norm():
    for c in m.L2NORM:
        x = m.l2norm_inputs(c, dev)
        ss = torch.zeros(c["B"], c["D"])
        for t in range(c["T"]):
            ss = ss + x[:, t] * x[:, t]
        nrm = torch.maximum(ss.sqrt(), torch.tensor(1e-12, dtype=F32))
        ref, bound = m.l2norm_ref(x, 1e-12)
        note("l2norm_dim1_kernel", c["id"], x / nrm[:, None, :], ref, bound)


def rope():
    for c in m.ROPE:
        dt, H = m.DTYPES[c["dt"]], c["H"]
        qkv, cos, sin = m.rope_inputs(c, dev)
        rows = torch.tensor([p if inside else 0 for _, p, inside in m.rope_rows(c)])
        for part, lo in (("q", 0), ("k", H)):
            x = qkv[:, lo:lo + H]
            half = c["D"] // 2
            cc, ss = cos.to(dt).float()[rows][:, None, :], sin.to(dt).float()[rows][:, None, :]
            x1, x2 = x[..., :half].float(), x[..., half:].float()
            y = torch.cat([x1 * cc - x2 * ss, x2 * cc + x1 * ss], -1).to(dt)
            ref, bound = m.rope_ref(x, cos, sin, rows, dt)
            note("rope_kv_append_kernel", f"{c['id']} ({part})", y, ref, bound)


def euler():
    for c in m.EULER:
        if c["ld"] != 4:
            continue                     # the leading dimension changes no arithmetic
        mode = c["mode"]
        sig, lat, eps = m.euler_inputs(c, dev)
        gs, igs = torch.tensor(m.GS), torch.tensor(m.IGS)
        worst, worst_s = 0.0, 0.0
        for i in range(50):
            s, sn = sig[i], sig[i + 1]
            ref, bound, sref, sbound = m.euler_ref(mode, lat, eps[i], float(s), float(sn), m.GS, m.IGS)
            if mode == 0:
                eu, et = eps[i, 0], eps[i, 1]
                e = eu + gs * (et - eu)
            else:
                x0t, x0i, x0u = lat - s * eps[i, 0], lat - s * eps[i, 1], lat - s * eps[i, 2]
                x0 = x0u + gs * (x0t - x0i) + igs * (x0i - x0u)
                e = (x0 - lat) / (-s)
            lat = lat + e * (sn - s)
            worst = max(worst, float(((lat.double() - ref).abs() / bound).max()))
            if c["scaled"]:
                sv = lat * torch.rsqrt(sn * sn + 1.0)
                worst_s = max(worst_s, float(((sv.double() - sref).abs() / sbound).max()))
        FIG.setdefault(f"cfg_euler_kernel mode {mode}", []).append((c["id"], worst))
        print(f"{'cfg_euler_kernel':28s} {c['id']:48s} worst |diff| / bound {worst:8.4f}   (50 steps; scaled copy {worst_s:.4f})")
        if c["scaled"]:
            FIG.setdefault(f"cfg_euler_kernel mode {mode} scaled copy", []).append((c["id"], worst_s))


def tsemb():
    t = torch.tensor(m.TS_T, dtype=F32)
    for dim in (2, 256, 320):
        e32 = m.tsemb_e32(dim)
        print(f"E32 at dim {dim}: {e32:.3f}")
        ref, arg = m.tsemb_ref(t, dim)
        for o, odt in m.ALL_DT.items():
            note("timestep_embedding_kernel", f"tsemb-{o}-dim{dim}", ru.timestep_embedding(t, dim).to(odt), ref, m.tsemb_bound(ref, arg, odt, e32))


if __name__ == "__main__":
    torch.manual_seed(0)
    for fn in (avgpool, silu, l2norm, rope, euler, tsemb):
        fn()
    bad = [(k, cid, r) for k, v in FIG.items() for cid, r in v if not r < 1.0]
    vacuous = [k for k, v in FIG.items() if not max(r for _, r in v) > 0.05]
    for k, v in FIG.items():
        print(f"{k:44s} largest figure {max(r for _, r in v):.4f}, smallest {min(r for _, r in v):.4f}")
    print("restatements outside their bound:", bad or "none")
    print("kernels without a figure above 0.05:", vacuous or "none")
    sys.exit(1 if bad or vacuous else 0)
