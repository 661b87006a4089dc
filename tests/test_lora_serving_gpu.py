"""Unmerged per-request LoRA adapters on the GPU (csrc/lora.hip, sx_gemv_args.addend): the kernels against the fp64 rule of seedx_amd.lora,
base rows untouched, row independence, the pre-activation addend of the skinny GEMM over every weight format, sx_rmsnorm_planes_sel."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DTS = [torch.float16, torch.bfloat16]
R = 32                                  # the rank table
SEL_PATTERN = [1, 0, -1, 1, 2, 0, 99]   # two adapters, a base row, and two indices outside [0, 2)
N_AD = 2
SENTINEL = -12345.0


def relerr(x, ref):
    x, ref = x.double().cpu(), ref.double().cpu()
    return ((x - ref).norm() / ref.norm()).item()


def _sel(G, dev=None):
    s = torch.tensor([SEL_PATTERN[g % len(SEL_PATTERN)] for g in range(G)], dtype=torch.int32)
    return s if dev is None else s.to(dev)


def _planes(t16):
    """A two-plane Tiled16 → (hi, lo) [rows, cols] in its dtype, on the CPU."""
    nb = t16.t.shape[0] // 2
    d = t16.t.view(2, nb, t16.cols // 32, 16, 32).permute(0, 1, 3, 2, 4).reshape(2, nb * 16, t16.cols)[:, :t16.rows]
    return d[0].cpu(), d[1].cpu()


def _seg(S, N):
    if S == 3:
        return (torch.arange(N // 16) // (N // 48)).to(torch.int32)
    if S == 2:
        return (torch.arange(N // 16) % 2).to(torch.int32)           # GLU-packed rows: 32-row groups [16 linear | 16 gate]
    return torch.zeros(N // 16, dtype=torch.int32)


def _tables(g, dt, K, r, S, N):
    """A [N_AD, S*R, K], B [N_AD, N, R] (rank r zero-padded to R per segment), scale = alpha / r — 16-bit values, on the CPU."""
    A = torch.zeros(N_AD, S, R, K)
    A[:, :, :r] = torch.randn(N_AD, S, r, K, generator=g) / math.sqrt(K)
    B = torch.zeros(N_AD, N, R)
    B[:, :, :r] = torch.randn(N_AD, N, r, generator=g) / math.sqrt(r)
    scale = torch.tensor([32.0 / r, 16.0 / r])
    return A.view(N_AD, S * R, K).to(dt), B.to(dt), scale


CASES = [(K, r, S, N) for K in (256, 704) for r in (8, 32) for (S, N) in ((3, 768), (2, 1408), (1, 256))]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("G", [1, 5, 16, 17, 32])       # 16 | 17: the row-block boundary of the planes
def test_shrink_expand_against_the_fp64_rule(dev, dt, G):
    from seedx_amd import lora, ops
    g = torch.Generator().manual_seed(11 + G)
    sel = _sel(G)
    on = (sel >= 0) & (sel < N_AD)
    worst = 0.0
    for (K, r, S, N) in CASES:
        A, B, scale = _tables(g, dt, K, r, S, N)
        seg = _seg(S, N)
        xt = ops.split16(torch.randn(G, K, generator=g).to(dev), dt, tiled=True)
        hi, lo = _planes(xt)
        t_ref = lora.shrink_ref(hi, lo, A, sel)
        d_ref = lora.expand_ref(t_ref, B, seg, scale, sel)
        t = ops.lora_shrink(xt, A.to(dev), sel.to(dev), out=torch.full((G, S * R), SENTINEL, device=dev))
        d = ops.lora_expand(t, B.to(dev), seg.to(dev), scale.to(dev), sel.to(dev), out=torch.full((G, N), SENTINEL, device=dev))
        et, ed = relerr(t[on.to(dev)], t_ref[on]), relerr(d[on.to(dev)], d_ref[on])
        worst = max(worst, et, ed)
        print(f"lora shrink/expand {dt} G={G} K={K} r={r} S={S} N={N}: t {et:.2e} delta {ed:.2e}")
        assert et < 3e-6 and ed < 3e-6
        # base rows (index -1 or outside the table): nothing written
        assert bool((t[~on.to(dev)] == SENTINEL).all()) and bool((d[~on.to(dev)] == SENTINEL).all())
        # the padded rank columns are exact zeros
        if r < R:
            assert bool((t[on.to(dev)].view(-1, S, R)[:, :, r:] == 0).all())
    print(f"lora shrink/expand {dt} G={G}: worst relative error vs fp64 {worst:.2e}")


@pytest.mark.parametrize("dt", DTS)
def test_shrink_row_major_planes_any_row_count(dev, dt):
    """The prefill form: rows [M][2K] = [hi | lo], M = 37 rows (no multiple of anything)."""
    from seedx_amd import lora, ops
    g = torch.Generator().manual_seed(3)
    M, K, S, N, r = 37, 704, 2, 1408, 8
    A, B, scale = _tables(g, dt, K, r, S, N)
    seg, sel = _seg(S, N), _sel(M)
    on = (sel >= 0) & (sel < N_AD)
    x = torch.randn(M, K, generator=g).to(dev)
    x2 = ops.split16(x, dt)
    d_ref = lora.delta_ref(x2[:, :K].cpu(), x2[:, K:].cpu(), A, B, seg, scale, sel)
    t = ops.lora_shrink(x2, A.to(dev), sel.to(dev))
    d = ops.lora_expand(t, B.to(dev), seg.to(dev), scale.to(dev), sel.to(dev), out=torch.full((M, N), SENTINEL, device=dev))
    e = relerr(d[on.to(dev)], d_ref[on])
    print(f"lora row-major {dt} M={M}: delta vs fp64 {e:.2e}")
    assert e < 3e-6 and bool((d[~on.to(dev)] == SENTINEL).all())
    # the tiled form of the first 32 rows gives the same bits: one arithmetic behind both layouts
    xt = ops.split16(x[:32].contiguous(), dt, tiled=True)
    hi, lo = _planes(xt)
    assert torch.equal(hi, x2[:32, :K].cpu()) and torch.equal(lo, x2[:32, K:].cpu())
    assert torch.equal(ops.lora_shrink(xt, A.to(dev), sel[:32].to(dev))[on[:32].to(dev)], t[:32][on[:32].to(dev)])


@pytest.mark.parametrize("dt", DTS)
def test_rows_are_independent(dev, dt):
    """Permuting the rows permutes the outputs bit for bit; row g of a 32-row launch equals the 1-row launch."""
    from seedx_amd import ops
    g = torch.Generator().manual_seed(5)
    G, K, S, N, r = 32, 704, 3, 768, 32
    A, B, scale = _tables(g, dt, K, r, S, N)
    A, B, scale, seg = A.to(dev), B.to(dev), scale.to(dev), _seg(S, N).to(dev)
    x = torch.randn(G, K, generator=g).to(dev)
    sel = _sel(G, dev)

    def run(xr, s):
        t = ops.lora_shrink(ops.split16(xr.contiguous(), dt, tiled=True), A, s.contiguous(), out=torch.full((xr.shape[0], S * R), SENTINEL, device=dev))
        return t, ops.lora_expand(t, B, seg, scale, s.contiguous(), out=torch.full((xr.shape[0], N), SENTINEL, device=dev))
    t0, d0 = run(x, sel)
    perm = torch.randperm(G, generator=g).to(dev)
    t1, d1 = run(x[perm], sel[perm])
    assert torch.equal(t1, t0[perm]) and torch.equal(d1, d0[perm])
    for row in (0, 3, 16, 31):
        t2, d2 = run(x[row:row + 1], sel[row:row + 1])
        assert torch.equal(t2[0], t0[row]) and torch.equal(d2[0], d0[row]), row


# ---- sx_gemv_args.addend -------------------------------------------------------------------------------------------------------------
def _weights(dev, dt, N, K, fmt, g):
    """(the 16-bit matrix the kernel multiplies by, gemv keyword arguments for layout 1, the same for the 20-row layout or None)"""
    from seedx_amd import ops, quant
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dev, dt)
    t20 = N % 20 == 0
    if fmt == "fp8":
        codes, sc = quant.quantize_rows(w)
        wq = quant.dequantize_rows(codes, sc, dt)
        return wq, dict(w_fp8=(ops.pack_decode_tiles_fp8(codes.contiguous()), sc.contiguous())), \
            dict(w_fp8=(ops.pack_decode_tiles20_fp8(codes.contiguous()), sc.contiguous())) if t20 else None
    if fmt == "mxfp4":
        codes, sc = quant.quantize_blocks_mxfp4(w)
        wq = quant.dequantize_blocks_mxfp4(codes, sc, dt)
        return wq, dict(w_fp4=(ops.pack_decode_tiles_fp4(codes.contiguous()), ops.pack_block_scales_fp4(sc.contiguous(), rows=16))), \
            dict(w_fp4=(ops.pack_decode_tiles20_fp4(codes.contiguous()), ops.pack_block_scales_fp4(sc.contiguous(), rows=20))) if t20 else None
    return w, dict(w_tiles=ops.pack_decode_tiles(w)), dict(w_tiles20=ops.pack_decode_tiles20(w)) if t20 else None


def _glu_ref(acc, N):
    v = acc.view(acc.shape[0], N // 32, 2, 16)
    lin, gate = v[:, :, 0].reshape(acc.shape[0], N // 2), v[:, :, 1].reshape(acc.shape[0], N // 2)
    return lin * torch.nn.functional.silu(gate)


# (N, K, glu, 20-row layout): layout 1 with the residual, the 20-row layout with the residual, layout 1 with the SiLU-GLU epilogue
GEMV_SHAPES = [(768, 256, False, False), (5120, 256, False, True), (1408, 704, True, False)]


@pytest.mark.parametrize("fmt", ["16bit", "fp8", "mxfp4"])
@pytest.mark.parametrize("M", [5, 16, 24])
@pytest.mark.parametrize("planes", [1, 2])               # x blocks per weight fragment: 1 / 2 (one plane), 2 / 4 (two planes)
def test_gemv_addend(dev, fmt, M, planes):
    from seedx_amd import ops
    dt = torch.float16
    g = torch.Generator().manual_seed(100 + M)
    sel = _sel(M, dev)
    on = ((sel >= 0) & (sel < N_AD)).cpu()
    off_all = torch.full((M,), -1, dtype=torch.int32, device=dev)
    for (N, K, glu, t20) in GEMV_SHAPES:
        wq, kw1, kw20 = _weights(dev, dt, N, K, fmt, g)
        wkw = kw20 if t20 else kw1
        x = torch.randn(M, K, generator=g).to(dev)
        if planes == 2:
            xt = ops.split16(x, dt, tiled=True)
            xr = xt.dense().double().cpu()
        else:
            xt = x.to(dt).contiguous()
            xr = xt.double().cpu()
        n_out = N // 2 if glu else N
        res = None if glu else torch.randn(M, n_out, generator=g).to(dev)
        add = torch.randn(M, N, generator=g).to(dev)          # the size of the accumulators themselves (x ~ 1, w ~ 1 / sqrt(K))
        kw = dict(residual=res, act="silu" if glu else None, glu=glu, out_dtype=torch.float32, **wkw)
        base = ops.gemv(xt, wq, **kw)
        # (a) every row switched off: the launch without the fields, bit for bit; the addend (NaN here) is never read into a result
        y_off = ops.gemv(xt, wq, addend=(torch.full_like(add, float("nan")), off_all, N_AD), **kw)
        assert torch.equal(y_off, base), (N, K, glu)
        # (b) mixed rows against fp64 of epilogue(acc + addend)
        y = ops.gemv(xt, wq, addend=(add, sel, N_AD), **kw)
        acc = xr @ wq.double().cpu().T
        acc_on = acc + add.double().cpu() * on[:, None]
        ref = _glu_ref(acc_on, N) if glu else acc_on + res.double().cpu()
        e = relerr(y, ref)
        print(f"gemv addend {fmt} M={M} planes={planes} {N}x{K} glu={glu} t20={t20}: vs fp64 {e:.2e}")
        assert e < 3e-6
        assert torch.equal(y[~on.to(dev)], base[~on.to(dev)])                       # base rows keep their bits
        # addend_sel = NULL: every row takes it
        y_all = ops.gemv(xt, wq, addend=add, **kw)
        ref_all = _glu_ref(acc + add.double().cpu(), N) if glu else acc + add.double().cpu() + res.double().cpu()
        assert relerr(y_all, ref_all) < 3e-6 and torch.equal(y_all[on.to(dev)], y[on.to(dev)])
        if glu:
            # fixture condition, fp64 side: an addend that entered AFTER the activation would miss by far more than 1e-2
            v = acc.view(M, N // 32, 2, 16)
            a = add.double().cpu().view(M, N // 32, 2, 16)
            late = ((v[:, :, 0] + a[:, :, 0]) * (torch.nn.functional.silu(v[:, :, 1]) + a[:, :, 1])).reshape(M, N // 2)
            assert relerr(late, ref_all) > 1e-2


@pytest.mark.parametrize("fmt", ["16bit", "fp8", "mxfp4"])
def test_gemv_addend_forced_split_k(dev, fmt):
    """A forced split-K factor (sx_gemv_tune key 2): the addend enters once, behind the split sums — the same bits as without the split
    wherever the kernel without an addend has them, and inside the bound either way. The hook is restored."""
    from seedx_amd import _lib, ops
    dt, M = torch.float16, 24
    lib = _lib.load()
    g = torch.Generator().manual_seed(9)
    sel = _sel(M, dev)
    on = ((sel >= 0) & (sel < N_AD)).cpu()
    N, K = 768, 1024
    wq, kw1, _ = _weights(dev, dt, N, K, fmt, g)
    xt = ops.split16(torch.randn(M, K, generator=g).to(dev), dt, tiled=True)
    res = torch.randn(M, N, generator=g).to(dev)
    add = torch.randn(M, N, generator=g).to(dev)
    ws = torch.zeros(16384 + 8 * 64 * N * 4, dtype=torch.uint8, device=dev)
    kw = dict(residual=res, out_dtype=torch.float32, workspace=ws, **kw1)
    ref = xt.dense().double().cpu() @ wq.double().cpu().T + add.double().cpu() * on[:, None] + res.double().cpu()
    out = {}
    try:
        for S in (-1, 2, 8):
            _lib.check(lib.sx_gemv_tune(2, S), "sx_gemv_tune")
            out[S] = (ops.gemv(xt, wq, **kw), ops.gemv(xt, wq, addend=(add, sel, N_AD), **kw))
            assert relerr(out[S][1], ref) < 3e-6, S
            assert torch.equal(out[S][1][~on.to(dev)], out[S][0][~on.to(dev)])
            assert int(ws[:16384].view(torch.int32).abs().sum()) == 0               # split-K counters left at zero
    finally:
        _lib.check(lib.sx_gemv_tune(2, 0), "sx_gemv_tune")
    for S in (2, 8):
        if torch.equal(out[S][0], out[-1][0]):
            assert torch.equal(out[S][1], out[-1][1]), S


def test_gemv_addend_is_refused_on_the_valu_path(dev):
    from seedx_amd import ops
    dt = torch.float16
    x = torch.randn(2, 256).to(dev, dt)
    w = torch.randn(64, 256).to(dev, dt)
    ops.gemv(x, w, out_dtype=torch.float32)                                          # the VALU launch itself is fine
    with pytest.raises(RuntimeError, match="addend"):
        ops.gemv(x, w, out_dtype=torch.float32, addend=torch.zeros(2, 64, device=dev))
    with pytest.raises(RuntimeError, match="addend"):
        ops.gemv(x, w, out_dtype=torch.float32, addend=(torch.zeros(2, 64, device=dev), torch.zeros(2, dtype=torch.int32, device=dev), 1))


# ---- sx_rmsnorm_planes_sel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("rows,tiled", [(1, True), (17, True), (32, True), (37, False)])
def test_rmsnorm_planes_sel_rows_equal_rmsnorm_planes(dev, dt, rows, tiled):
    """Every row is bit-identical to sx_rmsnorm_planes with the gamma it selected, in both output layouts and in the fp32 output."""
    from seedx_amd import ops
    g = torch.Generator().manual_seed(rows)
    cols, eps = 704, 1e-5
    x = (torch.randn(rows, cols, generator=g) * 3).to(dev)
    gam = lambda: (1 + 0.5 * torch.randn(cols, generator=g)).abs().clamp_min(0.2).to(dev)
    base, table = gam(), torch.stack([gam(), gam()]).contiguous()
    sel = _sel(rows, dev)
    got_p, got_f = ops.rmsnorm_planes_sel(x, base, table, sel, eps, dt, tiled=tiled, want_f32=True)
    want = [ops.rmsnorm_planes(x, gm, eps, dt, tiled=tiled, want_f32=True) for gm in (base, table[0], table[1])]
    pick = torch.where((sel >= 0) & (sel < N_AD), sel + 1, torch.zeros_like(sel)).cpu().tolist()
    if tiled:
        gp = torch.stack(_planes(got_p))
        wp = [torch.stack(_planes(w[0])) for w in want]
    else:
        gp = got_p.cpu().view(rows, 2, cols).permute(1, 0, 2)
        wp = [w[0].cpu().view(rows, 2, cols).permute(1, 0, 2) for w in want]
    for m in range(rows):
        assert torch.equal(got_f[m], want[pick[m]][1][m]), m
        assert torch.equal(gp[:, m].view(torch.int16), wp[pick[m]][:, m].view(torch.int16)), m
    assert len(set(pick)) == (3 if rows >= 3 else 1)
    # no table at all: every row is a base row
    p0, f0 = ops.rmsnorm_planes_sel(x, base, None, sel, eps, dt, tiled=tiled, want_f32=True)
    assert torch.equal(f0, want[0][1])
    if not tiled:
        assert torch.equal(p0.view(torch.int16), want[0][0].view(torch.int16))


# ---- the model: weights.MINI_LLM (H 256, FFN 704, 3 layers, head_dim 128), 4 slots, two adapters ---------------------------------------
from oracle import restated, weights  # noqa: E402

CFG = dict(weights.MINI_LLM)
G_M, STEPS, LENS = 4, 6, [10, 7, 13, 4]
NAMES = ["r8", None, "r32", "r8"]                # the adapter of each (prompt, slot) pair
_M = {}


def _peft_adapter(g, r, gain):
    """A PEFT-style dict: lora_A / lora_B (rank r) on the seven projections of every layer, the three norms in modules_to_save with gammas
    far from 1. 16-bit values. ``gain`` scales B so that the adapter moves the model (asserted below)."""
    H, I = CFG["hidden_size"], CFG["intermediate_size"]
    dims = {"self_attn.q_proj": (H, H), "self_attn.k_proj": (H, H), "self_attn.v_proj": (H, H), "self_attn.o_proj": (H, H),
            "mlp.gate_proj": (I, H), "mlp.up_proj": (I, H), "mlp.down_proj": (H, I)}
    gam = lambda: (1 + 0.5 * torch.randn(H, generator=g)).abs().clamp_min(0.2).half().float()
    sd = {"base_model.model.model.norm.modules_to_save.default.weight": gam()}
    for i in range(CFG["num_hidden_layers"]):
        p = f"base_model.model.model.layers.{i}."
        for n, (N, K) in dims.items():
            sd[p + n + ".lora_A.default.weight"] = (torch.randn(r, K, generator=g) / math.sqrt(K)).half().float()
            sd[p + n + ".lora_B.default.weight"] = (gain * torch.randn(N, r, generator=g) / math.sqrt(r)).half().float()
        sd[p + "input_layernorm.modules_to_save.default.weight"] = gam()
        sd[p + "post_attention_layernorm.modules_to_save.default.weight"] = gam()
    return sd


def _oracle_sd(base, ad, alpha=32):
    """The fp32 weights W + s B A (NOT rounded back to 16 bits) with the adapter's norms: what the adapter rows are checked against."""
    out = dict(base)
    for k, v in ad.items():
        k = k[len("base_model.model."):]
        if ".lora_A." in k:
            mod = k.split(".lora_A.")[0]
            A, B = v, ad["base_model.model." + mod + ".lora_B.default.weight"]
            out[mod + ".weight"] = base[mod + ".weight"].float() + (alpha / A.shape[0]) * (B.float() @ A.float())
        elif ".modules_to_save." in k:
            out[k.replace(".modules_to_save.default", "")] = v
    return out


def _fixture():
    if "fx" not in _M:
        g = torch.Generator().manual_seed(21)
        base = {k: v.half().float() for k, v in weights.llama_sd(CFG).items()}
        ads = {"r8": _peft_adapter(g, 8, 0.05), "r32": _peft_adapter(g, 32, 0.05)}
        xs = [torch.randn(t, CFG["hidden_size"], generator=g) * 0.5 for t in LENS]
        _M["fx"] = (base, ads, xs, torch.arange(20, 20 + G_M, dtype=torch.int32))
    return _M["fx"]


def _build(dev, state, **kw):
    from seedx_amd.llama import LlamaForCausalLM
    llm = LlamaForCausalLM(dict(CFG), max_cache_len=64, max_batch=G_M, kv_v16=False, **kw)
    llm.load_state_dict(dict(state))
    llm.eval().to(dev, dtype=torch.float16)
    if kw.get("max_adapters"):
        for name, ad in _fixture()[1].items():
            llm.load_adapter(name, ad, lora_alpha=32)
    return llm


def _run(llm, dev, xs, cur0, names, use_graph, order=None):
    """Prefill the prompts (slot i = pair order[i]) under their adapters, then STEPS token steps; results re-ordered by pair."""
    order = list(range(G_M)) if order is None else order
    img_ids = torch.arange(400, 466, dtype=torch.int32, device=dev)
    P = llm._pack()
    llm.reset()
    nm = [names[j] for j in order]
    kw = dict(adapters=nm) if llm.max_adapters else {}
    logits, _ = llm.forward_embeds_batch([xs[j].to(dev) for j in order], list(range(G_M)), **kw)
    if llm.max_adapters:
        llm.set_adapters(range(G_M), nm)
    P["cur"].copy_(cur0[order].to(dev))
    P["step"].zero_()
    out_ids = torch.full((G_M, STEPS), -1, dtype=torch.int32, device=dev)
    hid = torch.zeros((G_M, STEPS, CFG["hidden_size"]), device=dev)
    for _ in range(STEPS):
        llm.decode_step(img_ids, out_ids, hid, use_graph=use_graph)
    torch.cuda.synchronize()
    inv = torch.tensor([order.index(j) for j in range(G_M)], device=dev)
    return logits[inv].clone(), out_ids[inv].clone(), hid[inv].clone()


def _mixed(dev):
    """The mixed batch on the adapter model, eager: computed once, shared by the tests below."""
    if "mixed" not in _M:
        base, ads, xs, cur0 = _fixture()
        _M["llm"] = _build(dev, base, max_adapters=2)
        _M["mixed"] = _run(_M["llm"], dev, xs, cur0, NAMES, use_graph=False)
    return _M["llm"], _M["mixed"]


@pytest.fixture(scope="module", autouse=True)
def _free_models():
    yield
    _M.clear()
    torch.cuda.empty_cache()


def test_model_adapter_rows_against_the_fp32_oracle(dev):
    """Adapter rows against restated.llama_forward on W + s B A in fp32 (not rounded back) with the adapter's norms, teacher-forced: prefill
    logits and decode hidden states inside the project's contract, 1e-3; the adapter-free row against the oracle on the base weights.
    Fixture condition (CPU side): the oracle with the adapter and without it are more than 0.1 apart, so a dropped delta cannot pass.

    Measured on the MI355X (fp16): see profiles/lora_serving.md."""
    base, ads, xs, cur0 = _fixture()
    llm, (logits, ids, hid) = _mixed(dev)
    assert llm.adapters == ["r32", "r8"] and (ids >= 0).all()
    V = CFG["vocab_size"]
    for s in range(G_M):
        osd = _oracle_sd(base, ads[NAMES[s]]) if NAMES[s] else base
        fed = [int(cur0[s])] + [int(t) for t in ids[s, :STEPS - 1].cpu()]
        x = torch.cat([xs[s], base["model.embed_tokens.weight"][torch.tensor(fed)]], dim=0).unsqueeze(0)
        lref, _, hn = restated.llama_forward(osd, CFG, x, table_dtype=torch.float16)
        e_log, e_hid = relerr(logits[s, :V], lref[0, LENS[s] - 1]), relerr(hid[s], hn[0, LENS[s]:])
        print(f"lora model slot {s} adapter {NAMES[s]}: prefill logits vs fp32 oracle {e_log:.2e}, decode hidden states {e_hid:.2e}")
        if NAMES[s]:
            _, _, hn0 = restated.llama_forward(base, CFG, x, table_dtype=torch.float16)
            apart = relerr(hn0[0, LENS[s]:], hn[0, LENS[s]:])
            print(f"    oracle with vs without the adapter: {apart:.2f}")
            assert apart > 0.1
        assert e_log < 1e-3 and e_hid < 1e-3


def test_model_graph_replay_and_slot_permutation(dev):
    """The adapter step replayed from its own captured graph equals the eager step; permuting which slot each (prompt, adapter) pair occupies
    leaves every pair's prefill logits, ids and hidden states bit-identical."""
    base, ads, xs, cur0 = _fixture()
    llm, (logits, ids, hid) = _mixed(dev)
    g_log, g_ids, g_hid = _run(llm, dev, xs, cur0, NAMES, use_graph=True)
    assert llm._graph_ad is not None and llm._graph is None                       # the adapter step's own graph; the base step's is untouched
    assert torch.equal(g_log, logits) and torch.equal(g_ids, ids) and torch.equal(g_hid, hid)
    p_log, p_ids, p_hid = _run(llm, dev, xs, cur0, NAMES, use_graph=True, order=[2, 0, 3, 1])
    assert torch.equal(p_ids, ids) and torch.equal(p_hid, hid)
    assert torch.equal(p_log, logits)


def test_model_base_rows_and_adapter_free_batches(dev, monkeypatch):
    """(a) The adapter-free row of the mixed batch: decode ids and hidden states bit-identical to an adapter-free model built under
    SX_RMS_FOLD=0 (the unfolded arrangement the adapter step runs on). (b) No request names an adapter: a model with adapters loaded is
    bit-identical to the adapter-free default model, fold on, in prefill logits, ids and states — and runs the base step's graph."""
    base, ads, xs, cur0 = _fixture()
    llm, (logits, ids, hid) = _mixed(dev)
    none = [None] * G_M
    n_log, n_ids, n_hid = _run(llm, dev, xs, cur0, none, use_graph=True)
    assert llm._graph is not None
    D = _build(dev, base)
    assert D.max_adapters == 0 and "lora" not in D._pack() and "adapters" not in D.memory_footprint()      # max_adapters=0 allocates nothing
    d_log, d_ids, d_hid = _run(D, dev, xs, cur0, none, use_graph=True)
    assert torch.equal(n_log, d_log) and torch.equal(n_ids, d_ids) and torch.equal(n_hid, d_hid)
    del D
    monkeypatch.setenv("SX_RMS_FOLD", "0")
    U = _build(dev, base)
    assert not U._pack()["rms_fold_precise"]
    u_log, u_ids, u_hid = _run(U, dev, xs, cur0, none, use_graph=False)
    monkeypatch.delenv("SX_RMS_FOLD")
    s = NAMES.index(None)
    assert torch.equal(u_log[s], logits[s])
    assert torch.equal(u_ids[s], ids[s]) and torch.equal(u_hid[s], hid[s])
    # the whole of the base row's KV cache — the prefill rows of the mixed pass (one GEMM over all rows, a zero delta for this row) and
    # the rows the adapter step appended — has the bits of the adapter-free model's, in every layer
    m_log, m_ids, m_hid = _run(llm, dev, xs, cur0, NAMES, use_graph=False)
    assert torch.equal(m_log, logits) and torch.equal(m_hid, hid)
    PU, PL, rows = U._pack(), llm._pack(), LENS[s] + STEPS
    for k in ("kc", "vc"):
        assert PU[k].dtype == PL[k].dtype == torch.float32
        assert torch.equal(PU[k][:, s, :, :rows].contiguous().view(torch.int32), PL[k][:, s, :, :rows].contiguous().view(torch.int32)), k
    for t in range(G_M):                                                           # and the adapter rows really differ from the base model
        if NAMES[t]:
            assert not torch.equal(u_hid[t], hid[t])


def test_model_combined_formats(dev):
    """weight_format="mxfp4" + weight_residency="tiles" + kv_format="fp8_e4m3" with adapters: bit-identical to the default-format twin on
    the dequantised weights with the same adapters (the adapter stays exact in 16 bits over the quantised base)."""
    from seedx_amd import quant
    base, ads, xs, cur0 = _fixture()
    sd_q, _, _ = quant.quantize_llama_state_dict({k: v.to(dev) for k, v in base.items()}, CFG, torch.float16, weight_format="mxfp4")
    sd_q = {k: v.float().cpu() for k, v in sd_q.items()}
    A = _build(dev, base, weight_format="mxfp4", weight_residency="tiles", kv_format="fp8_e4m3", max_adapters=2)
    assert "adapters" in A.memory_footprint()
    a = _run(A, dev, xs, cur0, NAMES, use_graph=True)
    del A
    torch.cuda.empty_cache()
    B = _build(dev, sd_q, kv_format="fp8_e4m3", max_adapters=2)
    b = _run(B, dev, xs, cur0, NAMES, use_graph=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert (a[1] >= 0).all()


def test_model_refusals_and_table_updates(dev):
    """Unknown names, a full table, a rank above the table, unloading an adapter a sequence uses: ValueError, never the base model. Loading
    into the preallocated tables keeps the table pointers (captured graphs stay valid)."""
    base, ads, xs, cur0 = _fixture()
    llm, _ = _mixed(dev)
    llm.set_adapters(range(G_M), [None] * G_M)                                     # (the runs above left their sequences on their adapters)
    ptr = llm._pack()["lora"]["A"]["qkv"].data_ptr()
    with pytest.raises(ValueError, match="unknown adapter"):
        llm.forward_embeds_batch([xs[0].to(dev)], [0], adapters=["nope"])
    with pytest.raises(ValueError, match="adapter slots are in use"):
        llm.load_adapter("third", ads["r8"])
    llm.set_adapters([0], ["r8"])
    with pytest.raises(ValueError, match="in use"):
        llm.unload_adapter("r8")
    with pytest.raises(ValueError, match="in use"):                                # nor may its tables be replaced under a sequence
        llm.load_adapter("r8", ads["r8"])
    llm.set_adapters([0], [None])
    slot = llm._adapters["r8"]
    llm.unload_adapter("r8")
    T, P = llm._pack()["lora"], llm._pack()
    assert not T["A"]["qkv"][:, slot].any() and not T["B"]["d"][:, slot].any() and float(T["scale"][slot]) == 0.0     # a free slot computes
    assert torch.equal(T["norm"][slot], P["norm"]) and torch.equal(T["ln1"][1, slot], P["layers"][1]["ln1"])          # the base model
    with pytest.raises(ValueError, match="unknown adapter"):
        llm.unload_adapter("r8")
    llm.load_adapter("r8", ads["r8"])
    assert llm.adapters == ["r32", "r8"] and llm._pack()["lora"]["A"]["qkv"].data_ptr() == ptr
    from seedx_amd.llama import LlamaForCausalLM
    small = LlamaForCausalLM(dict(CFG), max_cache_len=64, max_batch=G_M, max_adapters=1, lora_rank=16)
    small.load_state_dict(dict(base))
    small.eval().to(dev, dtype=torch.float16)
    with pytest.raises(ValueError, match="exceeds the table rank"):
        small.load_adapter("r32", ads["r32"])
    off = _build(dev, base)
    with pytest.raises(ValueError, match="max_adapters=0"):
        off.load_adapter("r8", ads["r8"])
    with pytest.raises(ValueError, match="max_adapters=0"):
        off.forward_embeds_batch([xs[0].to(dev)], [0], adapters=["r8"])


def test_serving_generate_batch_mixes_adapters(dev):
    """The miniature agent: four requests on four slots mix two adapters, none, and one sampled request. Every request's ids equal those of
    the same request served in another slot beside other neighbours; the adapter moves the ids; results carry 'adapter'; reuse_cache keeps
    the rows of a sequence whose adapter is unchanged and re-prefills one whose adapter changed."""
    from seedx_amd.seed_x import ContinuousLVLM
    from seedx_amd.visual_encoder import Resampler
    from tests.test_models_gpu import StubTokenizer
    base, ads, _, _ = _fixture()
    VIT, Hd = 128, CFG["hidden_size"]
    kw = dict(num_img_gen_tokens=16, eos_token_id=None, max_new_tokens=8)
    llm = _build(dev, base, max_adapters=2)
    agent = ContinuousLVLM(llm, Resampler(4, Hd, 2, kv_dim=VIT), Resampler(4, VIT, 2, kv_dim=Hd), add_patch_pos=True)
    agent.load_state_dict(weights.agent_sd(CFG, VIT, in_grid=4, out_grid=4))
    agent.eval().to(dev, dtype=torch.float16)
    tok = StubTokenizer()
    prompt = lambda r: [[1, 10 + r] + [20 + r + i for i in range(3 + r % 5)]]
    reqs = [dict(input_ids=prompt(0), adapter="r8"), dict(input_ids=prompt(1)), dict(input_ids=prompt(2), adapter="r32"),
            dict(input_ids=prompt(0), adapter="r32", do_sample=True, temperature=1.0, top_k=50, top_p=0.9, seed=21)]
    mixed = agent.generate_batch(tok, reqs, **kw)
    assert [x["adapter"] for x in mixed] == ["r8", None, "r32", "r32"] and all(len(x["generate_ids"]) == 8 for x in mixed)
    ids = [x["generate_ids"].tolist() for x in mixed]
    filler = dict(input_ids=prompt(3))
    for r, q in enumerate(reqs):                                   # another slot, other neighbours: the same ids
        alone = agent.generate_batch(tok, [filler, filler, filler, q] if r != 3 else [q, filler, filler, filler], **kw)
        assert alone[3 if r != 3 else 0]["generate_ids"].tolist() == ids[r], r
    plain = agent.generate_batch(tok, [dict(input_ids=q["input_ids"]) for q in reqs], **kw)
    assert all(x["adapter"] is None for x in plain) and llm._sel_host == [-1] * 4
    assert plain[1]["generate_ids"].tolist() == ids[1]
    assert plain[0]["generate_ids"].tolist() != ids[0] and plain[2]["generate_ids"].tolist() != ids[2]
    # reuse_cache: the KV rows depend on the adapter
    turn = [dict(input_ids=prompt(r), adapter=a) for r, a in enumerate(["r8", None, "r32", "r8"])]
    first = agent.generate_batch(tok, turn, reuse_cache=True, **kw)
    turn2 = [dict(t) for t in turn]
    turn2[0]["adapter"], turn2[1]["adapter"] = "r32", "r8"
    second = agent.generate_batch(tok, turn2, reuse_cache=True, **kw)
    lens = [len(prompt(r)[0]) for r in range(4)]
    assert agent.last_prefill_tokens == [lens[0], lens[1], 1, 1]
    fresh = agent.generate_batch(tok, turn2, **kw)
    assert [x["generate_ids"].tolist() for x in second] == [x["generate_ids"].tolist() for x in fresh]
    assert first[2]["generate_ids"].tolist() == second[2]["generate_ids"].tolist()
    with pytest.raises(ValueError, match="unknown adapter"):
        agent.generate_batch(tok, [dict(input_ids=prompt(0), adapter="nope")] + [filler] * 3, **kw)


def _agent(dev):
    from seedx_amd.seed_x import ContinuousLVLM
    from seedx_amd.visual_encoder import Resampler
    base = _fixture()[0]
    VIT, Hd = 128, CFG["hidden_size"]
    llm = _build(dev, base, max_adapters=2)
    agent = ContinuousLVLM(llm, Resampler(4, Hd, 2, kv_dim=VIT), Resampler(4, VIT, 2, kv_dim=Hd), add_patch_pos=True)
    agent.load_state_dict(weights.agent_sd(CFG, VIT, in_grid=4, out_grid=4))
    agent.eval().to(dev, dtype=torch.float16)
    return agent


def test_serving_inflight_queue_mixes_adapters(dev):
    """Seven requests on four slots mix two adapters, none, and one sampled request. Every request's ids from generate_inflight equal those
    of the same request served alone through the same agent and those of generate_batch; the step counts are inflight.simulate's. With
    prefix_cache the ids are unchanged, two equal prompts under different adapters share nothing and two under the same adapter share as
    before: prefix_hit_tokens and the other counts are what simulate_prefix predicts with adapter-tagged signatures."""
    from seedx_amd.inflight import simulate, simulate_prefix
    from tests.test_models_gpu import StubTokenizer
    agent, tok = _agent(dev), StubTokenizer()
    llm = agent.llm
    kw = dict(num_img_gen_tokens=16, eos_token_id=None)
    A = [[1] + list(range(30, 42))]                                # 13 rows: above prefix_min_tokens (8)
    other = lambda r: [[1, 10 + r] + [20 + r + i for i in range(3 + r % 5)]]
    spec = [(A, "r8", 9), (other(1), None, 5), (A, "r32", 12), (other(3), "r32", 7), (A, "r8", 6), (other(5), None, 6), (other(6), "r8", 8)]
    reqs = [dict(input_ids=p, max_new_tokens=b, **({"adapter": a} if a else {})) for p, a, b in spec]
    reqs[3].update(do_sample=True, temperature=1.0, top_k=50, top_p=0.9, seed=21)
    names, budgets = [a for _, a, _ in spec], [b for _, _, b in spec]
    agent.prefix_cache = False
    got = agent.generate_inflight(tok, reqs, **kw)
    stats = dict(agent.last_inflight_stats)
    ids = [x["generate_ids"].tolist() for x in got]
    assert [x["adapter"] for x in got] == names and [len(i) for i in ids] == budgets
    assert llm._sel_host == [-1] * 4 and llm._pack()["lora"]["sel"].tolist() == [-1] * 4       # every slot parked at -1
    assert llm._slot_graph_ad is not None or llm._slot_sample_graph_ad is not None           # the adapter step ran on the slots path
    want = simulate(budgets, 4)
    for k in ("decode_steps", "live_slot_steps", "parked_slot_steps", "admissions", "prefill_passes"):
        assert stats[k] == want[k], (k, stats, want)
    for r, q in enumerate(reqs):                                   # the same request alone through the same agent
        alone = agent.generate_inflight(tok, [q], **kw)
        assert alone[0]["generate_ids"].tolist() == ids[r] and alone[0]["adapter"] == names[r], r
    strip = lambda q: {k: v for k, v in q.items() if k != "max_new_tokens"}
    for lo_ in (0, 3):                                             # and through generate_batch, four at a time
        batch = agent.generate_batch(tok, [strip(q) for q in reqs[lo_:lo_ + 4]], max_new_tokens=8, **kw)
        for j, x in enumerate(batch):
            n = min(budgets[lo_ + j], 8)
            assert x["generate_ids"].tolist()[:n] == ids[lo_ + j][:n], lo_ + j
    assert ids[0] != ids[2]                                        # one prompt, two adapters: different ids
    assert ids[4] == ids[0][:6]                                    # one prompt, one adapter
    # prefix reuse
    agent.prefix_cache = True
    got_p = agent.generate_inflight(tok, reqs, **kw)
    st_p = dict(agent.last_inflight_stats)
    assert [x["generate_ids"].tolist() for x in got_p] == ids
    prompts = [p[0] for p, _, _ in spec]
    want_p = simulate_prefix(prompts, budgets, 4, min_tokens=agent.prefix_min_tokens, generated=ids, adapters=names)
    for k in ("decode_steps", "live_slot_steps", "parked_slot_steps", "admissions", "prefill_passes", "prefill_tokens", "prefix_hit_tokens",
              "forked_tokens", "fork_launches"):
        assert st_p[k] == want_p[k], (k, st_p, want_p)
    untagged = simulate_prefix(prompts, budgets, 4, min_tokens=agent.prefix_min_tokens, generated=ids)
    print(f"lora prefix reuse: prefix_hit_tokens {st_p['prefix_hit_tokens']} (adapter-tagged prediction {want_p['prefix_hit_tokens']}, "
          f"untagged signatures would share {untagged['prefix_hit_tokens']})")
    assert 12 <= st_p["prefix_hit_tokens"] < untagged["prefix_hit_tokens"]     # request 4 shares A with request 0; request 2 shares nothing
    agent.prefix_cache = False
