"""Sharpness of the attention bound of tests/test_precise_matrix_gpu.py, without a GPU: a torch fp32 restatement of the two key walks of
csrc/precise.hip is fed the planted cases of every case family —
  * the VALU walk (attn_f32_kernel / attn_f32_verify_kernel): 16 groups per split, group j % 16 takes its keys in ascending order through
    attn_score (the lane's 8 or 16 chained products, four butterfly levels) and attn_key_update, then attn_merge_groups (two butterfly
    levels per wave), attn_merge_waves (four FMAs) and attn_f32_combine_kernel (one FMA per split);
  * the 32-key tile walk (attn_f32_mfma_kernel): 64 chained steps of two products per score, one alpha per tile, 16 steps of two keys
    into O —
and must stay inside the bound, while each of these mutants must leave it in every family:
  * drop: a planted key at an edge of the walk (a tile / split / page edge, key 0, the mask edge) never reaches the softmax;
  * one-more: every causal row sees key pos0 + t + 1 as well;
  * stale: the row behind the last visible key holds FLT_MAX (k with the signs of q: another request's values are arbitrary) and is not
    cancelled;
  * no-lo: only the hi plane is stored;
  * fp16-score: the scores come from one pass of fp16 products accumulated in fp16 (counted where a row sees at least 32 keys: with
    one key the score does not matter, and with a dozen keys whose weight lies on planted keys of EQUAL score the errors cancel).
Printed: the worst |diff| / bound of the clean walk, and for every mutant the worst ratio of the case (what the test sees: it must exceed
1 in every case) with, in brackets, the smallest over the rows the mutant touches of the row's worst ratio (a row that sees one key, or
whose scores all err alike, can stay inside). Run from the repository root: python tools/lab/precise_bound_sharpness.py (profiles/precise_matrix.md
holds its output)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import test_precise_matrix_gpu as m  # noqa: E402

F32 = torch.float32
dev = torch.device("cpu")
INF = float("inf")
MUTANTS = ("clean", "drop", "one-more", "stale", "no-lo", "fp16-score")


def score_valu(k, q):
    """attn_score: lane dl owns dims [8 dl, 8 dl + 8) (and [128 + 8 dl, ..) at DC = 2): one chain per lane, then a 16-lane tree"""
    D = k.shape[-1]
    DC = 2 if D > 128 else 1
    pad = 128 * DC - D
    k, q = torch.nn.functional.pad(k, (0, pad)), torch.nn.functional.pad(q.expand_as(k), (0, pad))
    k, q = k.reshape(*k.shape[:-1], DC, 16, 8), q.reshape(*q.shape[:-1], DC, 16, 8)
    s = torch.zeros(k.shape[:-3] + (16,), dtype=k.dtype)
    for c in range(DC):
        for e in range(8):
            s = k[..., c, :, e] * q[..., c, :, e] + s
    for _ in range(4):
        s = s[..., 0::2] + s[..., 1::2]
    return s[..., 0]


def score_fp16(k, q):
    k, q = k.half(), q.expand_as(k).half()
    s = torch.zeros(k.shape[:-1], dtype=torch.float16)
    for d in range(k.shape[-1]):
        s = s + k[..., d] * q[..., d]
    return s.float()


def score_tile(k, q):
    """64 chained accumulations, each adding the products of both lane halves (d and 64 + d)"""
    q = q.expand_as(k)
    s = torch.zeros(k.shape[:-1], dtype=k.dtype)
    for d in range(64):
        s = s + (k[..., d] * q[..., d] + k[..., 64 + d] * q[..., 64 + d])
    return s


def expd(a, b):
    """exp(a - b) with exp(-inf - anything) = 0"""
    return torch.where(a == -INF, torch.zeros_like(a), torch.exp(a - b))


def valu_walk(qs, K, V, nv, keep, chunk, ns, score):
    R, n, D = K.shape
    rr = torch.arange(R)[:, None]
    parts = []
    for sp in range(ns):
        mx, l, o = torch.full((R, 16), -INF), torch.zeros(R, 16), torch.zeros(R, 16, D)
        base = sp * chunk[:, None] + torch.arange(16)[None]
        end = torch.minimum(nv, (sp + 1) * chunk)[:, None]
        for i in range(int(chunk.max()) // 16):
            j = base + 16 * i
            jc = j.clamp(max=n - 1)
            ok = (j < end) & keep[rr, jc]
            k, v = K[rr, jc], V[rr, jc]
            s = score(k, qs[:, None, :])
            m_new = torch.maximum(mx, s)
            alpha, pr = expd(mx, m_new), torch.exp(s - m_new)
            l = torch.where(ok, l * alpha + pr, l)
            o = torch.where(ok[..., None], pr[..., None] * v + o * alpha[..., None], o)
            mx = torch.where(ok, m_new, mx)
        mw = mx.view(R, 4, 4).max(-1)[0]
        sc = expd(mx, mw.repeat_interleave(4, 1))
        lw = (l * sc).view(R, 4, 4)
        lw = (lw[..., 0] + lw[..., 1]) + (lw[..., 2] + lw[..., 3])
        ow = (o * sc[..., None]).view(R, 4, 4, D)
        ow = (ow[:, :, 0] + ow[:, :, 1]) + (ow[:, :, 2] + ow[:, :, 3])
        mg = mw.max(-1)[0]
        acc, ls = torch.zeros(R, D), torch.zeros(R)
        for w in range(4):
            wg = expd(mw[:, w], mg)
            acc, ls = wg[:, None] * ow[:, w] + acc, wg * lw[:, w] + ls
        parts.append((acc, mg, ls))
    if ns == 1:
        acc, ls = parts[0][0], parts[0][2]
    else:
        mg = torch.stack([p[1] for p in parts]).max(0)[0]
        acc, ls = torch.zeros(R, D), torch.zeros(R)
        for a, ms, l in parts:
            wg = expd(ms, mg)
            acc, ls = wg[:, None] * a + acc, wg * l + ls
    return torch.where(ls[:, None] > 0, acc / ls[:, None], torch.zeros_like(acc))


def tile_walk(qs, K, V, nv, keep, score):
    R, n, D = K.shape
    rr = torch.arange(R)[:, None]
    mx, l, o = torch.full((R,), -INF), torch.zeros(R), torch.zeros(R, D)
    for k0 in range(0, int(nv.max()), 32):
        j = k0 + torch.arange(32)[None].expand(R, 32)
        jc = j.clamp(max=n - 1)
        ok = (j < nv[:, None]) & keep[rr, jc]
        s = torch.where(ok, score(K[rr, jc], qs[:, None, :]), torch.full((R, 32), -INF))
        m_new = torch.maximum(mx, s.max(-1)[0])
        alpha = torch.where(m_new == -INF, torch.ones_like(mx), expd(mx, m_new))
        p = expd(s, m_new[:, None])
        l, mx, o = l * alpha + p.sum(-1), m_new, o * alpha[:, None]
        v = V[rr, jc]
        for t in range(16):
            o = o + (p[:, 2 * t, None] * v[:, 2 * t] + p[:, 2 * t + 1, None] * v[:, 2 * t + 1])
    return torch.where(l[:, None] > 0, o / l[:, None], torch.zeros_like(o))


def planes_sum(val, dt, lo=True):
    hi, lo_ = m.split_ref(val, dt)
    return hi.double() + (lo_.double() if lo else 0.0)


def run_case(c):
    """ratio [G][T][H][D] of every mutant, and the rows each mutant touches"""
    dt = m.DTYPES[c["dt"]]
    G, T, H, D, Tmax = c["G"], c["T"], c["H"], c["D"], c["Tmax"]
    L = m.logical(c, dev)
    q64, K64, V64, qmag, kmag = m.reference_operands(c, L)
    ref, A, s1, spread = m.ref_attention(c, L, q64, K64, V64, qmag, kmag)
    bound = m.attn_bound(c, ref, A, s1, spread)
    R = G * T * H
    gi = torch.arange(G)[:, None, None].expand(G, T, H).reshape(R)
    hi_ = torch.arange(H)[None, None, :].expand(G, T, H).reshape(R)
    qs = (q64.float() * L["scale"]).reshape(R, D)
    nv0 = torch.tensor(L["nvis"])[:, :, None].expand(G, T, H).reshape(R)
    K0 = torch.cat([K64.float(), torch.zeros(G, H, 1, D)], 2)[gi, hi_]          # one spare row: a key behind a full cache
    V0 = torch.cat([V64.float(), torch.zeros(G, H, 1, D)], 2)[gi, hi_]
    ns = c["nsplit"] if (T == 1 or m.is_verify(c)) else 1
    out = {}
    for mut in MUTANTS:
        K, V, nv = K0, V0, nv0
        keep = torch.ones(R, Tmax + 1, dtype=torch.bool)
        touched = nv0 > 0
        if mut == "drop":
            touched = torch.zeros(R, dtype=torch.bool)
            for (g, t, h, key) in L["planted"]:
                r = (g * T + t) * H + h
                if key < L["nvis"][g][t] and not bool(touched[r]) and (key < c["pos0"][g] or not c["causal"] or not m.walk_edges(c, g)):
                    keep[r, key], touched[r] = False, True
        elif mut in ("one-more", "stale"):
            touched = (nv0 > 0) & (nv0 < Tmax) if c["causal"] else torch.zeros(R, dtype=torch.bool)
            nv = torch.where(touched, nv0 + 1, nv0)
            if mut == "stale":
                K, V = K0.clone(), V0.clone()
                sign = torch.where(torch.arange(D) % 2 == 0, 1.0, -1.0) * m.MAXF[F32]
                K[touched, nv0[touched]], V[touched, nv0[touched]] = torch.where(qs[touched] < 0, -1.0, 1.0) * m.MAXF[F32], sign
        chunk = torch.tensor([m.split_chunk(int(x), ns) if ns > 1 else max(16, (int(x) + 15) & ~15) for x in nv])
        score = score_fp16 if mut == "fp16-score" else (score_tile if m.is_mfma(c) else score_valu)
        val = tile_walk(qs, K, V, nv, keep, score) if m.is_mfma(c) else valu_walk(qs, K, V, nv, keep, chunk, ns, score)
        got = planes_sum(val, dt, lo=mut != "no-lo").reshape(G, T, H, D)
        ratio = torch.nan_to_num((got - ref).abs() / bound, nan=INF).reshape(R, D).amax(-1)
        out[mut] = (ratio, touched)
    return out


def report():
    worst, worst_row = {mut: (INF if mut != "clean" else 0.0) for mut in MUTANTS}, {mut: INF for mut in MUTANTS}
    for fam in m.FAMILIES:
        for dt in m.DTYPES:
            cases = [c for c in m.ATTN if c["fam"] == fam and c["dt"] == dt and c["data"] == "plant" and c["D"] >= 40 and c["Tmax"] <= 400]
            for c in cases[:1] + cases[-1:]:
                res = run_case(c)
                line = []
                for mut in MUTANTS:
                    ratio, touched = res[mut]
                    if mut == "clean":
                        v = float(ratio.max())
                        worst[mut] = max(worst[mut], v)
                    elif not bool(touched.any()):
                        line.append(f"{mut} -")
                        continue
                    else:
                        v, lo = float(ratio[touched].max()), float(ratio[touched].min())
                        if mut == "fp16-score" and max(max(r) for r in m.n_visible(c)) < 32:
                            line.append(f"{mut} {v:.3g} (few keys: not counted)")
                            continue
                        worst[mut], worst_row[mut] = min(worst[mut], v), min(worst_row[mut], lo)
                        line.append(f"{mut} {v:.3g} ({lo:.2g})")
                        continue
                    line.append(f"{mut} {v:.3g}")
                print(f"{c['id']:78s} " + "  ".join(line))
    print("over all cases: clean worst |diff| / bound %.3f; smallest worst ratio of a case (of a touched row): " % worst["clean"] +
          ", ".join(f"{mut} {worst[mut]:.3g} ({worst_row[mut]:.2g})" for mut in MUTANTS[1:]))
    assert worst["clean"] <= 1.0 and all(worst[mut] > 1.0 for mut in MUTANTS[1:])


if __name__ == "__main__":
    report()
