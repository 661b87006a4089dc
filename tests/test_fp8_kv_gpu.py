"""The FP8 (e4m3) KV cache on the GPU (LlamaForCausalLM(kv_format="fp8_e4m3"); sx_rope_kv_append_f32_q8, sx_attn_f32_args.kv_fp8).

The claim under test is EXACTNESS, not closeness: a k / v row is rounded once, when it is appended — by the rule quant.quantize_kv_rows
states on the host, which the device quantiser must reproduce bit for bit — and everything after that is the fp32-grade path: attention
on codes + power-of-two row scales equals, bit for bit, the fp32 kernels on a cache holding the dequantised values, and the FP8-cache
model equals its fp32-cache twin (kv_format="fp8_e4m3_emulated") in logits, ids and hidden states. Two independent evaluations of the
same quantised model do NOT agree tightly (a last-bit difference in one k flips a code and moves everything downstream by ~1e-3), so
the tight model-level tests compare two runs of the same kernels; what the mode costs against the unquantised model is printed and
bounded by a fake-quant fp64 restatement computed here. The mode is opt-in and outside the 1e-3 contract.
Reference: modeling_llama_xformer.py:141-149 (RoPE), :204-239 (attention), :215-220 (the cache the codes replace)."""
import ctypes as C
import math

import pytest
import torch

from oracle import restated, weights

pytestmark = pytest.mark.gpu
DTS = [torch.float16, torch.bfloat16]
D = 128


def relerr(x, ref):
    x, ref = x.double().cpu(), ref.double().cpu()
    return ((x - ref).norm() / ref.norm()).item()


def _tables(Tmax, dev, identity=False):
    if identity:                 # cos = 1, sin = 0: the rotation is exact whatever the compiler contracts (x · 1 + (+-0) = x for x != 0)
        return torch.ones(Tmax, D // 2, device=dev), torch.zeros(Tmax, D // 2, device=dev)
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    fr = torch.outer(torch.arange(Tmax).float(), inv)
    return fr.cos().to(dev).contiguous(), fr.sin().to(dev).contiguous()


def _dense(y, cols):
    return y[:, :cols].float() + y[:, cols:].float()


# ---------------------------------------------------------------------------------------------------------
# 4. the device quantiser against the host rule, bit for bit
# ---------------------------------------------------------------------------------------------------------
def _crafted_rows(n, seed, signed_zero):
    """n rows of 128 that hit every decision of the rule, at row exponents s from the clamp's lower end to its upper end: every binade
    of the format, exact ties (m + 1/2) quanta in the normal and the subnormal range, values that round to the -0 code, an all-zero
    row, amax exactly 448 · 2^s (mantissa 1.75: s stays), one ulp above (s + 1) and below, Gaussian and heavy-tailed rows (the latter
    run into the exponent clamp and saturate at +-448). signed_zero: true -0 inputs (v rows only — a rotated k of -0 is -0 + 0 = +0)."""
    g = torch.Generator().manual_seed(seed)
    exps = [-64, -30, -13, -9, -3, 0, 1, 5, 20, 63]
    rows = []
    for i in range(n):
        sc = 2.0 ** exps[(i * 7 + i // 12) % len(exps)]
        top = torch.tensor(448.0 * sc)
        r = torch.zeros(D)
        kind = i % 12
        sign = torch.where(torch.rand(D, generator=g) < 0.5, -1.0, 1.0)
        if kind == 0:                                           # every binade: (1 + u) · 2^e, e = 8 .. -15 (the last ones below the subnormals)
            e = 8 - (torch.arange(D) % 24)
            r = sign * (1 + torch.rand(D, generator=g)) * torch.exp2(e.float()) * sc
            r[0] = top
        elif kind == 1:                                         # exact ties between two normal codes: (8 + m + 1/2) · 2^(e - 3)
            j = torch.arange(112)
            r[:112] = sign[:112] * (8.5 + (j % 8).float()) * torch.exp2((j // 8).float() - 9) * sc      # e = -6 .. 7
            r[127] = -top
        elif kind == 2:                                         # the subnormal range: ties (m + 1/2) · 2^-9 and random values below 2^-6
            r[:8] = (torch.arange(8).float() + 0.5) * 2.0 ** -9 * sc
            r[8:16] = -r[:8]
            r[16:] = sign[16:] * torch.rand(D - 16, generator=g) * 2.0 ** -6 * sc
            r[64] = top
        elif kind == 3:
            pass                                                # all zero
        elif kind in (4, 5, 6):                                 # amax on the boundary, one ulp above, one ulp below
            r = torch.randn(D, generator=g) * 50 * sc
            r[17] = {4: top, 5: torch.nextafter(top, torch.tensor(float("inf"))), 6: torch.nextafter(top, torch.tensor(0.0))}[kind]
            r[90] = -r[17] if i % 2 else r[90]
        elif kind == 7:
            r = torch.randn(D, generator=g) * 100 * sc
        elif kind == 8:                                         # round to the -0 code: below half a subnormal quantum, and the tie itself
            r[:] = -(2.0 ** -11) * sc
            r[1::3] = -(2.0 ** -10) * sc                        # tie between 0 and the first subnormal: to even = 0
            r[2::3] = torch.nextafter(torch.tensor(2.0 ** -10 * sc), torch.tensor(float("inf")))      # just above: code 1
            r[5] = top
        elif kind == 9:
            r = torch.randn(D, generator=g) * torch.exp(3 * torch.randn(D, generator=g)) * sc
        elif kind == 10:
            r[int(torch.randint(0, D, (1,), generator=g))] = -3.0 * sc                                  # the amax alone
        else:
            r = torch.randn(D, generator=g) * sc
            r[::4] = 0.0
            if signed_zero:
                r[::8] = -0.0
        rows.append(r.float())
    return torch.stack(rows)


def _q8_expect(rows):
    from seedx_amd import quant
    codes, scale = quant.quantize_kv_rows(rows)
    assert ((codes & 0x7f) != 0x7f).all()
    return codes, scale


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("G,T,H,pos", [(3, 1, 4, [0, 17, 63]), (2, 37, 2, [0, 20])])
def test_quantiser_equals_the_host_rule(dev, dt, G, T, H, pos):
    """sx_rope_kv_append_f32_q8 with identity tables on crafted rows: codes and scales equal quant.quantize_kv_rows bit for bit, q is
    unchanged, no other cache row or scale is touched; emulate = 1 writes exactly the dequantised values; at T = 1 the fused decode form
    of sx_attention_f32 (kv_fp8 = 1, with and without key splits) appends the same codes and scales."""
    from seedx_amd import ops, quant
    Tmax, n = 64, G * T * H
    g = torch.Generator().manual_seed(40 + T)
    k = _crafted_rows(n, 1, False).view(G * T, H, D)
    v = _crafted_rows(n + 5, 2, True)[5:].view(G * T, H, D)
    q = torch.randn(G * T, H, D, generator=g)
    qkv0 = torch.cat([q, k, v], dim=1).reshape(G * T, 3 * H * D).contiguous().to(dev)
    kcod, kscl = _q8_expect(k)
    vcod, vscl = _q8_expect(v)
    cos, sin = _tables(Tmax, dev, identity=True)
    posd = torch.tensor(pos, dtype=torch.int32, device=dev)

    def fresh():
        return (torch.full((G, H, Tmax, D), 0x55, dtype=torch.uint8, device=dev), torch.full((G, H, Tmax, D), 0x2a, dtype=torch.uint8, device=dev),
                torch.full((G, H, Tmax), 4.0, device=dev), torch.full((G, H, Tmax), 0.5, device=dev))

    def check(kc, vc, ks, vs, what):
        kc, vc, ks, vs = kc.cpu(), vc.cpu(), ks.cpu(), vs.cpu()
        m = torch.ones(G, Tmax, dtype=torch.bool)
        for gi in range(G):
            for t in range(T):
                p, r = pos[gi] + t, gi * T + t
                m[gi, p] = False
                bad = (kc[gi, :, p] != kcod[r]).sum().item() + (vc[gi, :, p] != vcod[r]).sum().item()
                assert bad == 0, f"{what}: {bad} codes of row {r} differ from the host rule"
                assert torch.equal(ks[gi, :, p], kscl[r]) and torch.equal(vs[gi, :, p], vscl[r]), (what, r, ks[gi, :, p], kscl[r])
        for gi in range(G):                                     # every other row and scale is untouched
            assert (kc[gi][:, m[gi]] == 0x55).all() and (vc[gi][:, m[gi]] == 0x2a).all()
            assert (ks[gi][:, m[gi]] == 4.0).all() and (vs[gi][:, m[gi]] == 0.5).all()
    kc, vc, ks, vs = fresh()
    qkv = qkv0.clone()
    ops.rope_kv_append_f32(qkv, kc, vc, cos, sin, posd, G, T, H, D, dt, kv_scales=(ks, vs))
    assert torch.equal(qkv, qkv0), "identity tables: q is rotated onto itself, the k / v rows of qkv are never written"
    check(kc, vc, ks, vs, "sx_rope_kv_append_f32_q8")
    # the twin: fp32 caches receive decode(code) · scale, nothing else
    ke, ve = torch.full((G, H, Tmax, D), 3.0, device=dev), torch.full((G, H, Tmax, D), -3.0, device=dev)
    qkv = qkv0.clone()
    ops.rope_kv_append_f32(qkv, ke, ve, cos, sin, posd, G, T, H, D, dt, kv_emulate=True)
    assert torch.equal(qkv, qkv0)
    kd, vd = quant.dequantize_kv_rows(kc, ks), quant.dequantize_kv_rows(vc, vs)
    for gi in range(G):
        sl = slice(pos[gi], pos[gi] + T)
        assert torch.equal(ke[gi, :, sl], kd[gi, :, sl]) and torch.equal(ve[gi, :, sl], vd[gi, :, sl])
        ke[gi, :, sl], ve[gi, :, sl] = 3.0, -3.0
    assert (ke == 3.0).all() and (ve == -3.0).all()
    if T == 1:
        for nsplit in (1, 3):
            kc, vc, ks, vs = fresh()
            qkv = qkv0.clone()
            ops.attention_f32(qkv, kc, vc, posd, G, 1, H, D, 1.0 / math.sqrt(D), dt, nsplit=nsplit, rope=(cos, sin), kv_scales=(ks, vs))
            assert torch.equal(qkv, qkv0)
            check(kc, vc, ks, vs, f"fused decode form, nsplit {nsplit}")


# ---------------------------------------------------------------------------------------------------------
# 5. append with real tables
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("G,T,H,pos", [(3, 1, 4, [0, 17, 130]), (2, 37, 2, [0, 0])])
def test_append_with_real_tables(dev, dt, G, T, H, pos):
    """Against sx_rope_kv_append_f32 on the same rows: q within 2e-7; dequantise(codes, scale) within half a quantum of that kernel's k
    (+ 1e-6 amax: the two kernels' rotations may contract their fmas differently); v, which is not rotated, bit for bit the host rule;
    emulate = 1 writes exactly dequantise(codes, scale); rows other than the appended ones untouched."""
    from seedx_amd import ops, quant
    Tmax = 256
    g = torch.Generator().manual_seed(41)
    qkv0 = (torch.randn(G * T, 3 * H * D, generator=g) * 1.5).to(dev)
    cos, sin = _tables(Tmax, dev)
    posd = torch.tensor(pos, dtype=torch.int32, device=dev)
    q_ref, k_ref, v_ref = qkv0.clone(), torch.zeros(G, H, Tmax, D, device=dev), torch.zeros(G, H, Tmax, D, device=dev)
    ops.rope_kv_append_f32(q_ref, k_ref, v_ref, cos, sin, posd, G, T, H, D, dt)
    kc = torch.full((G, H, Tmax, D), 0x55, dtype=torch.uint8, device=dev)
    vc = torch.full((G, H, Tmax, D), 0x2a, dtype=torch.uint8, device=dev)
    ks, vs = torch.full((G, H, Tmax), 4.0, device=dev), torch.full((G, H, Tmax), 0.5, device=dev)
    qkv = qkv0.clone()
    ops.rope_kv_append_f32(qkv, kc, vc, cos, sin, posd, G, T, H, D, dt, kv_scales=(ks, vs))
    e_q = relerr(qkv[:, :H * D], q_ref[:, :H * D])
    assert e_q < 2e-7 and torch.equal(qkv[:, H * D:], qkv0[:, H * D:])
    ke, ve = torch.full((G, H, Tmax, D), 3.0, device=dev), torch.full((G, H, Tmax, D), -3.0, device=dev)
    qe = qkv0.clone()
    ops.rope_kv_append_f32(qe, ke, ve, cos, sin, posd, G, T, H, D, dt, kv_emulate=True)
    assert torch.equal(qe, qkv)
    kd, vd = quant.dequantize_kv_rows(kc, ks), quant.dequantize_kv_rows(vc, vs)
    worst = 0.0
    for gi in range(G):
        sl = slice(pos[gi], pos[gi] + T)
        kr = k_ref[gi, :, sl].double()
        bound = kr.abs() * 2.0 ** -4 + ks[gi, :, sl, None].double() * 2.0 ** -10 + 1e-6 * kr.abs().amax(-1, keepdim=True)
        err = (kd[gi, :, sl].double() - kr).abs()
        worst = max(worst, (err / bound).max().item())
        assert (err <= bound).all()
        vrows = qkv0.view(G, T, 3, H, D)[gi, :, 2].permute(1, 0, 2).cpu()                      # [H, T, D]
        vcod, vscl = quant.quantize_kv_rows(vrows)
        assert torch.equal(vc[gi, :, sl].cpu(), vcod) and torch.equal(vs[gi, :, sl].cpu(), vscl)
        assert torch.equal(ke[gi, :, sl], kd[gi, :, sl]) and torch.equal(ve[gi, :, sl], vd[gi, :, sl])
        m = torch.ones(Tmax, dtype=torch.bool, device=dev)
        m[sl] = False
        assert (kc[gi][:, m] == 0x55).all() and (vc[gi][:, m] == 0x2a).all() and (ks[gi][:, m] == 4.0).all() and (vs[gi][:, m] == 0.5).all()
        assert (ke[gi][:, m] == 3.0).all() and (ve[gi][:, m] == -3.0).all()
    print(f"q8 append {dt} G={G} T={T}: q vs the fp32 kernel {e_q:.2e}, worst k error / bound {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------
# 6. attention on codes == attention on the dequantised fp32 cache
# ---------------------------------------------------------------------------------------------------------
def _random_cache(G, H, Tmax, dev, seed):
    """Random non-NaN codes (subnormals and -0 included) and row scales 2^s, s in [-12, 3]; → (kc, vc, ks, vs, k fp32, v fp32)."""
    from seedx_amd import quant
    g = torch.Generator(device=dev).manual_seed(seed)
    out = []
    for _ in range(2):
        c = torch.randint(0, 256, (G, H, Tmax, D), dtype=torch.uint8, device=dev, generator=g)
        c = torch.where((c & 0x7f) == 0x7f, c & 0xf0, c)                                       # 0x7f / 0xff → 0x70 / 0xf0
        c[:, :, ::7, 3] = 0x80                                                                 # -0
        s = torch.exp2(torch.randint(-12, 4, (G, H, Tmax), device=dev, generator=g).float())
        out += [c, s]
    kc, ks, vc, vs = out
    return kc, vc, ks, vs, quant.dequantize_kv_rows(kc, ks), quant.dequantize_kv_rows(vc, vs)


def _attn_ref(q, kc, vc, pos, T, scale):
    """q [G*T, H, D] fp64; caches [G, H, Tmax, D]; row t of sequence g sees keys 0 .. pos[g] + t."""
    G, H = kc.shape[0], kc.shape[1]
    out = torch.zeros(G * T, H, q.shape[-1], dtype=torch.float64)
    for g in range(G):
        for t in range(T):
            n = int(pos[g]) + t + 1
            s = torch.einsum("hd,hkd->hk", q[g * T + t], kc[g, :, :n].double()) * scale
            out[g * T + t] = torch.einsum("hk,hkd->hd", torch.softmax(s, -1), vc[g, :, :n].double())
    return out


ATTN_SHAPES = [(3, 1, 4, [0, 17, 130], 1, 256),           # VALU, T = 1
               (2, 5, 3, [20, 3], 1, 256),                # VALU, QB = 4
               (2, 9, 2, [0, 40], 1, 512), (3, 37, 2, [0, 5, 130], 1, 512), (1, 165, 3, [0], 1, 512), (1, 300, 2, [200], 1, 512),    # MFMA
               (4, 1, 5, [0, 17, 300, 1499], 6, 1536), (3, 1, 2, [5, 31, 32], 2, 1536)]                                              # key splits


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("G,T,H,pos,nsplit,Tmax", ATTN_SHAPES)
def test_attention_on_codes_equals_attention_on_dequantised_cache(dev, dt, G, T, H, pos, nsplit, Tmax):
    """Every route of sx_attention_f32 with kv_fp8 = 1 (VALU QB 1 / 4 / 8, key splits + combine, the fp32 MFMA kernel) gives the BITS of the
    fp32 call on the dequantised cache, row-major and tiled; and the fp32 kernels' fp64 bound holds against fp64 attention over the
    dequantised values. q is scaled so that the scores against the largest keys (|k| up to 448 · 2^3) stay O(1): a softmax that still
    mixes keys."""
    from seedx_amd import _lib, ops
    lib = _lib.load()
    kc, vc, ks, vs, k32, v32 = _random_cache(G, H, Tmax, dev, 50 + T)
    g = torch.Generator().manual_seed(51)
    qkv = (torch.randn(G * T, 3 * H * D, generator=g) * 2e-3).to(dev)
    posd = torch.tensor(pos, dtype=torch.int32, device=dev)
    scale = 1.0 / math.sqrt(D)
    kw = dict(nsplit=nsplit)
    y8 = ops.attention_f32(qkv, kc, vc, posd, G, T, H, D, scale, dt, kv_scales=(ks, vs), **kw)
    y32 = ops.attention_f32(qkv, k32, v32, posd, G, T, H, D, scale, dt, **kw)
    assert torch.equal(y8, y32), f"codes vs dequantised fp32 cache: {relerr(_dense(y8, H * D), _dense(y32, H * D)):.2e}"
    if G * T <= 32 and (H * D) % 32 == 0:                      # the tiled output (at T > 8 this is the VALU QB = 8 kernel: the MFMA one writes rows)
        t8 = ops.attention_f32(qkv, kc, vc, posd, G, T, H, D, scale, dt, tiled=True, kv_scales=(ks, vs), **kw)
        t32 = ops.attention_f32(qkv, k32, v32, posd, G, T, H, D, scale, dt, tiled=True, **kw)
        assert torch.equal(t8.dense(), t32.dense())
        if T <= 8:
            assert torch.equal(t8.dense(), _dense(y8, H * D))
    if 8 < T <= 37:                                            # the VALU QB = 8 kernel on codes (row-major), MFMA switched off
        try:
            assert lib.sx_attention_f32_variant(0) == 0
            v8 = ops.attention_f32(qkv, kc, vc, posd, G, T, H, D, scale, dt, kv_scales=(ks, vs))
            v32_ = ops.attention_f32(qkv, k32, v32, posd, G, T, H, D, scale, dt)
        finally:
            lib.sx_attention_f32_variant(1)
        assert torch.equal(v8, v32_)
    ref = _attn_ref(qkv.cpu().double()[:, :H * D].reshape(G * T, H, D), k32.cpu(), v32.cpu(), pos, T, scale).reshape(G * T, H * D)
    e = relerr(_dense(y8, H * D), ref)
    print(f"attention on FP8 codes {dt} G={G} T={T} H={H} pos={pos} nsplit={nsplit}: bit-equal to the fp32 cache, vs fp64 {e:.2e}")
    assert e < (2e-6 if dt == torch.float16 else 2e-5)


# ---------------------------------------------------------------------------------------------------------
# 7. fused RoPE + append + attention: kv_fp8 = 1 against its fp32 twin kv_fp8 = 2
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("G,H,pos,nsplit", [(4, 5, [0, 17, 300, 1499], 1), (4, 5, [0, 17, 300, 1499], 6), (2, 2, [1535, 1536], 4), (16, 40, None, 1)])
def test_fused_rope_append_attention_equals_the_twin(dev, dt, G, H, pos, nsplit):
    """The decode step's fused form on the FP8 cache against the same launch on an fp32 cache holding the dequantised values with
    quantise-dequantise on append: context planes bit-equal (the new token's own key / value are the DEQUANTISED values in both), the
    appended row's dequantise(codes, scale) equals the twin's fp32 row, every other row and scale untouched, a position at Tmax writes
    nothing."""
    from seedx_amd import ops, quant
    g = torch.Generator().manual_seed(36)
    if pos is None:
        pos = [int(x) for x in torch.randint(0, 400, (G,), generator=g)]
    Tmax = 1536 if max(pos) >= 512 else 512
    kc0, vc0, ks0, vs0, k32, v32 = _random_cache(G, H, Tmax, dev, 60)
    qkv0 = (torch.randn(G, 3 * H * D, generator=g) * 1.5).to(dev)
    qkv0[:, :H * D] *= 2e-3                                   # O(1) scores against the cache's largest keys (see the test above)
    cos, sin = _tables(Tmax, dev)
    posd = torch.tensor(pos, dtype=torch.int32, device=dev)
    scale = 1.0 / math.sqrt(D)
    kc, vc, ks, vs = kc0.clone(), vc0.clone(), ks0.clone(), vs0.clone()
    qa = qkv0.clone()
    ya = ops.attention_f32(qa, kc, vc, posd, G, 1, H, D, scale, dt, nsplit=nsplit, rope=(cos, sin), kv_scales=(ks, vs))
    kb, vb, qb = k32.clone(), v32.clone(), qkv0.clone()
    yb = ops.attention_f32(qb, kb, vb, posd, G, 1, H, D, scale, dt, nsplit=nsplit, rope=(cos, sin), kv_emulate=True)
    assert torch.equal(qa, qkv0) and torch.equal(qb, qkv0), "the fused form leaves the qkv buffer alone"
    assert torch.equal(ya, yb), f"FP8 cache vs its fp32 twin: {relerr(_dense(ya, H * D), _dense(yb, H * D)):.2e}"
    assert torch.equal(quant.dequantize_kv_rows(kc, ks), kb) and torch.equal(quant.dequantize_kv_rows(vc, vs), vb)
    for gi, pp in enumerate(pos):
        m = torch.ones(Tmax, dtype=torch.bool, device=dev)
        if pp < Tmax:
            m[pp] = False
            assert not torch.equal(kb[gi][:, pp], k32[gi][:, pp]) and not torch.equal(vc[gi][:, pp], vc0[gi][:, pp])     # it WAS appended
        assert torch.equal(kc[gi][:, m], kc0[gi][:, m]) and torch.equal(vc[gi][:, m], vc0[gi][:, m])
        assert torch.equal(ks[gi][:, m], ks0[gi][:, m]) and torch.equal(vs[gi][:, m], vs0[gi][:, m])
        assert torch.equal(kb[gi][:, m], k32[gi][:, m]) and torch.equal(vb[gi][:, m], v32[gi][:, m])
    if G <= 16 and (H * D) % 32 == 0:
        yt = ops.attention_f32(qkv0.clone(), kc0.clone(), vc0.clone(), posd, G, 1, H, D, scale, dt, tiled=True, nsplit=nsplit, rope=(cos, sin),
                               kv_scales=(ks0.clone(), vs0.clone()))
        assert torch.equal(yt.dense(), _dense(ya, H * D))


# ---------------------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_what_they_do_not_cover(dev):
    from seedx_amd import _lib
    lib = _lib.load()
    G, H, Tmax = 1, 2, 32
    p = lambda t: C.c_void_p(t.data_ptr())
    z8 = torch.zeros(G, H, Tmax, D, dtype=torch.uint8, device=dev)
    zs = torch.ones(G, H, Tmax, device=dev)
    qkv = torch.zeros(G, 3 * H * D, device=dev)
    out = torch.zeros(G, 2 * H * D, dtype=torch.float16, device=dev)
    pos = torch.zeros(G, dtype=torch.int32, device=dev)
    cos, sin = _tables(Tmax, dev)

    def args(**kw):
        a = _lib.AttnF32Args()
        a.q, a.kcache, a.vcache, a.out, a.pos0_dev = p(qkv), p(z8), p(z8), p(out), p(pos)
        a.q_row_stride, a.cache_seq_stride = 3 * H * D, H * Tmax * D
        a.G, a.T, a.H, a.D, a.Tmax, a.dtype, a.scale, a.causal = G, 1, H, D, Tmax, _lib.SX_F16, 0.1, 1
        a.kv_fp8, a.k_scale, a.v_scale, a.scale_seq_stride = 1, p(zs), p(zs), H * Tmax
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(status, word):
        msg = lib.sx_last_error().decode()
        assert status != 0 and word in msg, (status, msg)
    assert lib.sx_attention_f32(C.byref(args()), None) == 0                                          # the base call is accepted
    refused(lib.sx_attention_f32(C.byref(args(D=64, H=4)), None), "head_dim 128")
    refused(lib.sx_attention_f32(C.byref(args(v16=1)), None), "v16")
    refused(lib.sx_attention_f32(C.byref(args(k_scale=None)), None), "k_scale")
    refused(lib.sx_attention_f32(C.byref(args(v_scale=C.c_void_p(zs.data_ptr() + 2))), None), "k_scale")        # misaligned
    refused(lib.sx_attention_f32(C.byref(args(causal=0)), None), "causal")
    refused(lib.sx_attention_f32(C.byref(args(kv_row_stride=2 * D)), None), "causal")
    refused(lib.sx_attention_f32(C.byref(args(kv_fp8=3)), None), "kv_fp8")
    q8 = lambda **kw: lib.sx_rope_kv_append_f32_q8(p(qkv), p(z8), p(z8), kw.get("ks", p(zs)), p(zs), p(cos), p(sin), p(pos), G, 1,
                                                   kw.get("H", H), kw.get("D", D), Tmax, H * Tmax * D, H * Tmax, _lib.SX_F16,
                                                   kw.get("emulate", 0), None)
    assert q8() == 0
    refused(q8(D=64, H=4), "head_dim 128")
    refused(q8(ks=None), "kscale")
    refused(q8(emulate=2), "emulate")
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------
# 9. - 11. model level
# ---------------------------------------------------------------------------------------------------------
GEOMS = {"mini": dict(weights.MINI_LLM, max_position_embeddings=128),
         "1024x8": dict(hidden_size=1024, intermediate_size=2816, num_hidden_layers=3, num_attention_heads=8, vocab_size=500, rms_norm_eps=1e-5,
                        max_position_embeddings=128)}
G8, T0, STEPS = 8, 10, 4
_RUNS = {}


def _inputs(cfg, dt):
    g = torch.Generator().manual_seed(11)
    sd = {k: v.to(dt).float() for k, v in weights.llama_sd(cfg).items()}
    xs = [torch.randn(T0, cfg["hidden_size"], generator=g) * 0.5 for _ in range(20)]
    return sd, xs, torch.arange(20, 40, dtype=torch.int32)


def _build(dev, dt, cfg, sd, n, **kw):
    from seedx_amd.llama import LlamaForCausalLM
    llm = LlamaForCausalLM(dict(cfg), max_cache_len=64, max_batch=n, **kw)
    llm.load_state_dict(dict(sd))
    return llm.eval().to(dev, dtype=dt)


def _prefill_and_decode(llm, dev, xs, cur0, img_ids, steps, use_graph):
    G, H = len(xs), xs[0].shape[1]
    P = llm._pack()
    llm.reset()
    logits, _ = llm.forward_embeds_batch([x.to(dev) for x in xs], list(range(G)))
    P["cur"].copy_(cur0.to(dev))
    P["step"].zero_()
    out_ids = torch.full((G, steps), -1, dtype=torch.int32, device=dev)
    hid = torch.zeros((G, steps, H), device=dev)
    for _ in range(steps):
        llm.decode_step(img_ids, out_ids, hid, use_graph=use_graph)
    torch.cuda.synchronize()
    return logits.clone(), out_ids.clone(), hid.clone()


def _run_A(dev, dt, geom):
    """The FP8-cache model's eager run on 8 sequences, once per (geometry, dtype): shared by the twin test and the cost test."""
    key = (geom, dt)
    if key not in _RUNS:
        cfg = GEOMS[geom]
        sd, xs, cur0 = _inputs(cfg, dt)
        img_ids = torch.arange(400, 466, dtype=torch.int32, device=dev)
        A = _build(dev, dt, cfg, sd, G8, kv_format="fp8_e4m3")
        _RUNS[key] = (A, _prefill_and_decode(A, dev, xs[:G8], cur0[:G8], img_ids, STEPS, use_graph=False))
    return _RUNS[key]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("geom", list(GEOMS))
def test_fp8_cache_model_equals_its_fp32_twin(dev, dt, geom):
    """A = kv_format="fp8_e4m3", B = "fp8_e4m3_emulated" (all-fp32 caches holding the rounded rows, the existing fp32 attention kernels):
    prefill logits, decode ids and hidden states bit-equal on 8 sequences (10-token prompts, 4 steps) and at 20 sequences; graph replay
    == eager for A; a 31-token `forward` prefill + six cached single-token `forward` calls give bit-equal logits at every step (batch-1
    models: the fused RoPE + append + key-split decode form); A holds uint8 codes and exactly memory_footprint()["kv_cache"] bytes.
    NOT asserted: prefill == prefill + decode within A — the two GEMM paths differ in the last bit, and that flips codes."""
    cfg = GEOMS[geom]
    sd, xs, cur0 = _inputs(cfg, dt)
    img_ids = torch.arange(400, 466, dtype=torch.int32, device=dev)
    A, (a_log, a_ids, a_hid) = _run_A(dev, dt, geom)
    P = A._pack()
    assert A.precise and A.kv_format == "fp8_e4m3" and not A.kv_v16 and P["kc"].dtype == torch.uint8 and P["vc"].dtype == torch.uint8
    assert P["kc"].shape == (cfg["num_hidden_layers"], G8, cfg["num_attention_heads"], 64, D) and P["ks"].shape == P["kc"].shape[:4]
    held = sum(P[k].numel() * P[k].element_size() for k in ("kc", "vc", "ks", "vs"))
    assert held == A.memory_footprint()["kv_cache"] == cfg["num_hidden_layers"] * G8 * cfg["num_attention_heads"] * 64 * 264
    assert not ((P["kc"] & 0x7f) == 0x7f).any() and not ((P["vc"] & 0x7f) == 0x7f).any() and (a_ids >= 0).all()
    assert (P["ks"][:, :, :, :T0 + STEPS] > 0).all() and (P["ks"][:, :, :, T0 + STEPS:] == 0).all()        # written rows carry a scale, the rest never were
    g_log, g_ids, g_hid = _prefill_and_decode(A, dev, xs[:G8], cur0[:G8], img_ids, STEPS, use_graph=True)
    assert torch.equal(g_log, a_log) and torch.equal(g_ids, a_ids) and torch.equal(g_hid, a_hid)          # graph replay == eager
    B = _build(dev, dt, cfg, sd, G8, kv_format="fp8_e4m3_emulated")
    PB = B._pack()
    assert PB["kc"].dtype == torch.float32 and PB["vc"].dtype == torch.float32 and "ks" not in PB and not B.kv_v16
    assert B.memory_footprint()["kv_cache"] == PB["kc"].numel() * 8
    b_log, b_ids, b_hid = _prefill_and_decode(B, dev, xs[:G8], cur0[:G8], img_ids, STEPS, use_graph=False)
    assert torch.equal(a_log, b_log), relerr(a_log, b_log)
    assert torch.equal(a_ids, b_ids)
    assert torch.equal(a_hid, b_hid), relerr(a_hid, b_hid)
    from seedx_amd import quant                                  # the twin's cache IS the dequantised FP8 cache
    assert torch.equal(quant.dequantize_kv_rows(P["kc"], P["ks"]), PB["kc"]) and torch.equal(quant.dequantize_kv_rows(P["vc"], P["vs"]), PB["vc"])
    del B, PB
    # one run at 20 sequences (four operand blocks per weight fragment, another split count)
    r20 = []
    for fmt in ("fp8_e4m3", "fp8_e4m3_emulated"):
        m = _build(dev, dt, cfg, sd, 20, kv_format=fmt)
        r20.append(_prefill_and_decode(m, dev, xs, cur0, img_ids, STEPS, use_graph=False))
        del m
    assert all(torch.equal(x, y) for x, y in zip(*r20))
    # the reference-style entry on batch-1 models: prefill of 31 tokens, then six cached single-token calls
    g = torch.Generator().manual_seed(12)
    emb = torch.randn(1, 37, cfg["hidden_size"], generator=g) * 0.5
    outs = []
    for fmt in ("fp8_e4m3", "fp8_e4m3_emulated"):
        m = _build(dev, dt, cfg, sd, 1, kv_format=fmt)
        o = m(inputs_embeds=emb[:, :31].to(dev))
        seq = [o["logits"].clone()]
        for t in range(31, 37):
            pkv = o["past_key_values"]
            assert pkv[0][0].dtype == torch.float32 and pkv[0][0].shape == (1, cfg["num_attention_heads"], t, D) and pkv[-1][1].shape[2] == t
            o = m(inputs_embeds=emb[:, t:t + 1].to(dev), past_key_values=pkv)
            seq.append(o["logits"].clone())
        outs.append((seq, pkv))
        del m
    for x, y in zip(outs[0][0], outs[1][0]):
        assert torch.equal(x, y), relerr(x, y)
    assert all(torch.equal(a, b) for la, lb in zip(outs[0][1], outs[1][1]) for a, b in zip(la, lb))       # dequantised copies == the twin's views
    torch.cuda.empty_cache()


def _fakequant_forward64(sd, cfg, x, table_dtype):
    """restated.llama_forward in fp64 with the cache's rounding: k after RoPE and v go through quant.quantize_kv_rows (which rounds its
    input to fp32 first, like the cache's producer) and come back dequantised. → final-norm hidden states [1, T, H] fp64."""
    from seedx_amd import quant
    F = torch.nn.functional
    H, nh, L, eps = cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_hidden_layers"], cfg["rms_norm_eps"]
    hd = H // nh
    w = lambda k: sd[k].double()
    norm = lambda x, k: w(k) * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))
    fq = lambda t: quant.dequantize_kv_rows(*quant.quantize_kv_rows(t.float())).double()
    x = x.double()
    T = x.shape[1]
    cos, sin = restated.rope_tables(hd, T)
    cos, sin = cos.to(table_dtype).double()[None, None], sin.to(table_dtype).double()[None, None]
    ii = torch.arange(T)
    causal = ii[None, :] > ii[:, None]
    for i in range(L):
        p = f"model.layers.{i}."
        h = norm(x, p + "input_layernorm.weight")
        q, k, v = (F.linear(h, w(p + f"self_attn.{n}_proj.weight")).view(1, T, nh, hd).transpose(1, 2) for n in "qkv")
        q = q * cos + restated.rotate_half(q) * sin
        k = fq(k * cos + restated.rotate_half(k) * sin)
        v = fq(v)
        s = (q @ k.transpose(-1, -2) / math.sqrt(hd)).masked_fill(causal, float("-inf"))
        o = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(1, T, H)
        x = x + F.linear(o, w(p + "self_attn.o_proj.weight"))
        h = norm(x, p + "post_attention_layernorm.weight")
        x = x + F.linear(F.silu(F.linear(h, w(p + "mlp.gate_proj.weight"))) * F.linear(h, w(p + "mlp.up_proj.weight")), w(p + "mlp.down_proj.weight"))
    return norm(x, "model.norm.weight")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("geom", list(GEOMS))
def test_cost_of_the_mode(dev, dt, geom):
    """What the FP8 cache costs against the UNQUANTISED model, printed, and bounded by a reference computed here: e_A = the relative
    Frobenius distance of A's decode hidden states from restated.llama_forward teacher-forced on A's tokens; e_ref = the same distance
    for an fp64 fake-quant restatement of the decoder. e_A < 1.5 e_ref: two independent evaluations of the quantised model differed by at
    most 0.12 e_ref on the CPU; a wrong scale index or a truncating convert is off by far more. The figures are large on these
    random-weight miniatures (sharp softmaxes) — the mode is opt-in and outside the 1e-3 contract (profiles/fp8_kv.md)."""
    cfg = GEOMS[geom]
    sd, xs, cur0 = _inputs(cfg, dt)
    _, (_, a_ids, a_hid) = _run_A(dev, dt, geom)
    a_ids, a_hid = a_ids.cpu(), a_hid.cpu()
    emb = sd["model.embed_tokens.weight"]
    got, ref, fake = [], [], []
    for s in (0, 3, 7):
        fed = [int(cur0[s])] + [int(t) for t in a_ids[s, :STEPS - 1]]
        x = torch.cat([xs[s], emb[torch.tensor(fed)]], dim=0).unsqueeze(0)
        ref.append(restated.llama_forward(sd, cfg, x, table_dtype=dt)[2][0, T0:])
        fake.append(_fakequant_forward64(sd, cfg, x, dt)[0, T0:])
        got.append(a_hid[s])
    e_A, e_ref = relerr(torch.cat(got), torch.cat(ref)), relerr(torch.cat(fake), torch.cat(ref))
    print(f"FP8 KV cache at model level, {geom} {dt}: decode hidden states vs the unquantised fp32 model e_A = {e_A:.3e}; "
          f"fp64 fake-quant restatement e_ref = {e_ref:.3e}; ratio {e_A / e_ref:.3f}")
    assert e_ref > 1e-3, "the fake-quant reference must actually quantise"
    assert e_A < 1.5 * e_ref


@pytest.mark.parametrize("weight_format", [None, "fp8_e4m3"])
def test_fp8_kv_serving_paths_agree(dev, weight_format):
    """generate_inflight on a miniature FP8-cache model — 6 mixed greedy / sampled requests on 4 slots — returns, request by request, the
    ids of generate_batch on the same model: a request's cache rows depend on its own values only, so slot independence survives the
    quantisation. Alone and together with the FP8 weight tiles."""
    from seedx_amd.llama import LlamaForCausalLM
    from seedx_amd.seed_x import ContinuousLVLM
    from seedx_amd.visual_encoder import Resampler
    from tests.test_models_gpu import StubTokenizer
    cfg, VIT = weights.MINI_LLM, 128
    kw = dict(num_img_gen_tokens=16, eos_token_id=None)
    llm = LlamaForCausalLM(dict(cfg), max_cache_len=512, max_batch=4, kv_format="fp8_e4m3", weight_format=weight_format)
    llm.load_state_dict(weights.llama_sd(cfg))
    Hd = cfg["hidden_size"]
    agent = ContinuousLVLM(llm, Resampler(4, Hd, 2, kv_dim=VIT), Resampler(4, VIT, 2, kv_dim=Hd), add_patch_pos=True)
    agent.load_state_dict(weights.agent_sd(cfg, VIT, in_grid=4, out_grid=4))
    agent.eval().to(dev, dtype=torch.float16)
    tok = StubTokenizer()
    budgets = [9, 5, 12, 7, 6, 10]
    reqs = [dict(input_ids=[[1, 10 + r] + [20 + r + i for i in range(3 + r % 5)]], max_new_tokens=b) for r, b in enumerate(budgets)]
    for r, s in ((1, 21), (2, 22), (5, 23)):
        reqs[r].update(do_sample=True, temperature=1.0, top_k=50, top_p=0.9, seed=s)
    got = agent.generate_inflight(tok, reqs, **kw)
    P = llm._pack()
    assert llm.kv_format == "fp8_e4m3" and P["kc"].dtype == torch.uint8 and llm.weight_format == weight_format
    assert P["layers"][0]["wqkv"].format == weight_format and ("w_fp8" in P["layers"][0]["wqkv"].gemv_kwargs()) == (weight_format is not None)
    assert [len(x["generate_ids"]) for x in got] == budgets
    strip = lambda q: {k: v for k, v in q.items() if k != "max_new_tokens"}
    for wave in ([0, 1, 2, 3], [4, 5, 0, 1]):
        ref = agent.generate_batch(tok, [strip(reqs[r]) for r in wave], max_new_tokens=12, **kw)
        for i, r in enumerate(wave):
            assert got[r]["generate_ids"].tolist() == ref[i]["generate_ids"].tolist()[:budgets[r]], (r, got[r]["generate_ids"].tolist())
