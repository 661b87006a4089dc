"""Unmerged LoRA adapters, host side (seedx_amd.lora): the fp64 rule against a plain restatement of peft's forward, the PEFT key parsing
against merge_peft_lora on the same dict, the table layout, and every refusal of the loader. No GPU."""
import math

import pytest
import torch

L, H, I, NH = 2, 64, 96, 2


def _base_sd(g):
    sd = {"model.embed_tokens.weight": torch.randn(40, H, generator=g), "model.norm.weight": torch.ones(H), "lm_head.weight": torch.randn(40, H, generator=g)}
    for i in range(L):
        p = f"model.layers.{i}."
        for n in ("q_proj", "k_proj", "v_proj", "o_proj"):
            sd[p + f"self_attn.{n}.weight"] = torch.randn(H, H, generator=g) / math.sqrt(H)
        sd[p + "mlp.gate_proj.weight"] = torch.randn(I, H, generator=g) / math.sqrt(H)
        sd[p + "mlp.up_proj.weight"] = torch.randn(I, H, generator=g) / math.sqrt(H)
        sd[p + "mlp.down_proj.weight"] = torch.randn(H, I, generator=g) / math.sqrt(I)
        sd[p + "input_layernorm.weight"] = torch.ones(H)
        sd[p + "post_attention_layernorm.weight"] = torch.ones(H)
    return {k: v.half() for k, v in sd.items()}


def _peft_sd(g, r, named=True, norms=True):
    """A PeftModel-style dict: every base key wrapped, lora_A / lora_B on the seven projections, the norms in modules_to_save."""
    from seedx_amd import lora
    base = _base_sd(g)
    out = {}
    ad = ".default" if named else ""
    for k, v in base.items():
        mod = k[:-len(".weight")]
        name = mod.split(".")[-1]
        if name in lora.PROJECTIONS:
            N, K = v.shape
            out[f"base_model.model.{mod}.base_layer.weight"] = v
            out[f"base_model.model.{mod}.lora_A{ad}.weight"] = (torch.randn(r, K, generator=g) / math.sqrt(K)).half()
            out[f"base_model.model.{mod}.lora_B{ad}.weight"] = (torch.randn(N, r, generator=g) / math.sqrt(r)).half()
        elif norms and (name in lora.NORMS or k == "model.norm.weight"):
            out[f"base_model.model.{mod}.original_module.weight"] = v
            out[f"base_model.model.{mod}.modules_to_save.default.weight"] = (1 + 0.5 * torch.randn(H, generator=g)).abs().clamp_min(0.2).half()
        else:
            out["base_model.model." + k] = v
    return base, out


@pytest.mark.parametrize("r,alpha,named", [(8, 32, True), (32, 32, False), (16, 8, True)])
def test_tables_reproduce_the_delta_merge_peft_lora_adds(r, alpha, named):
    from seedx_amd import lora
    from seedx_amd.llama import merge_peft_lora
    g = torch.Generator().manual_seed(r)
    base, psd = _peft_sd(g, r, named)
    merged = merge_peft_lora(psd, lora_alpha=alpha)
    tab = lora.AdapterTables(psd, L, H, I, R=32, lora_alpha=alpha, dtype=torch.float16)
    assert tab.r == r and tab.scale == alpha / r
    for i in range(L):
        for name in lora.PROJECTIONS:
            k = f"model.layers.{i}.{'self_attn' if name in lora.PROJECTIONS[:4] else 'mlp'}.{name}.weight"
            want = (base[k].float() + tab.delta_weight(i, name)).half()          # the merge rounds W + s B A once, to W's dtype
            assert torch.equal(merged[k], want), k
            assert not torch.equal(merged[k], base[k])
        assert torch.equal(tab.ln1[i], merged[f"model.layers.{i}.input_layernorm.weight"].float())
        assert torch.equal(tab.ln2[i], merged[f"model.layers.{i}.post_attention_layernorm.weight"].float())
    assert torch.equal(tab.norm, merged["model.norm.weight"].float())
    # table shapes and the zero padding of the rank
    assert tab.A["qkv"][0].shape == (96, H) and tab.B["gu"][0].shape == (2 * I, 32) and tab.A["d"][0].shape == (32, I)
    if r < 32:
        assert not tab.A["qkv"][0].view(3, 32, H)[:, r:].any() and not tab.B["o"][0][:, r:].any()
    assert tab.nbytes() == L * 2 * 32 * (4 * 2 * H + 3 * (H + I))          # 16-bit, R (K + N) elements per projection


def test_adapter_without_norms_and_with_a_subset_of_projections():
    from seedx_amd import lora
    g = torch.Generator().manual_seed(1)
    _, psd = _peft_sd(g, 8, norms=False)
    psd = {k: v for k, v in psd.items() if "down_proj.lora_" not in k}
    tab = lora.AdapterTables(psd, L, H, I)
    assert tab.norm is None and tab.ln1 == [None] * L and not tab.A["d"][0].any() and not tab.B["d"][1].any() and tab.A["o"][0].any()


def test_refusals():
    from seedx_amd import lora
    g = torch.Generator().manual_seed(2)
    _, psd = _peft_sd(g, 8)
    A = torch.zeros(8, H).half()
    cases = {
        "rank above the table": (dict(psd), dict(R=4), "exceeds the table rank"),
        "lora_embedding": ({**psd, "base_model.model.model.embed_tokens.lora_embedding_A.default": torch.zeros(8, 40)}, {}, "lora_embedding"),
        "lm_head delta": ({**psd, "base_model.model.lm_head.lora_A.default.weight": A, "base_model.model.lm_head.lora_B.default.weight": torch.zeros(40, 8).half()},
                          {}, "embed_tokens / lm_head"),
        "embed_tokens saved": ({**psd, "base_model.model.model.embed_tokens.modules_to_save.default.weight": torch.zeros(40, H)}, {}, "embed_tokens / lm_head"),
        "another target module": ({**psd, "base_model.model.model.layers.0.mlp.act_fn.lora_A.default.weight": A,
                                   "base_model.model.model.layers.0.mlp.act_fn.lora_B.default.weight": torch.zeros(H, 8).half()}, {}, "adapter targets"),
        "half a pair": ({k: v for k, v in psd.items() if "layers.1.self_attn.o_proj.lora_B" not in k}, {}, "only one of"),
        "a layer the model does not have": ({k.replace("layers.1.", "layers.7."): v for k, v in psd.items()}, {}, "adapter targets"),
    }
    for what, (sd, kw, msg) in cases.items():
        with pytest.raises(ValueError, match=msg):
            lora.AdapterTables(sd, L, H, I, **kw)
    mixed = dict(psd)
    mixed["base_model.model.model.layers.0.self_attn.q_proj.lora_A.default.weight"] = torch.zeros(4, H).half()
    mixed["base_model.model.model.layers.0.self_attn.q_proj.lora_B.default.weight"] = torch.zeros(H, 4).half()
    with pytest.raises(ValueError, match="mixes ranks"):
        lora.AdapterTables(mixed, L, H, I)


def test_the_fp64_rule_is_pefts_forward():
    """shrink_ref / expand_ref on planes and packed tables == peft's Linear.forward restated in plain torch (F.linear(x, W) + lora_B(lora_A(x))
    · alpha / r) minus the base product; base rows are undefined (NaN), whatever index marks them."""
    from seedx_amd import lora
    g = torch.Generator().manual_seed(4)
    M, K, N, r, R = 9, 64, 96, 8, 32
    x = torch.randn(M, K, generator=g)
    hi = x.half()
    lo = (x - hi.float()).half()
    W = torch.randn(N, K, generator=g).half()
    ads = [(torch.randn(r, K, generator=g).half(), torch.randn(N, r, generator=g).half(), 32.0), (torch.randn(r, K, generator=g).half(), torch.randn(N, r, generator=g).half(), 16.0)]
    A = torch.zeros(2, R, K, dtype=torch.float16)
    B = torch.zeros(2, N, R, dtype=torch.float16)
    for a, (Aa, Ba, _) in enumerate(ads):
        A[a, :r], B[a, :, :r] = Aa, Ba
    scale = torch.tensor([al / r for _, _, al in ads])
    sel = torch.tensor([0, 1, -1, 1, 2, 0, 99, 0, 1], dtype=torch.int32)
    d = lora.delta_ref(hi, lo, A, B, torch.zeros(N // 16, dtype=torch.int32), scale, sel)
    xs = hi.double() + lo.double()
    for m in range(M):
        a = int(sel[m])
        if 0 <= a < 2:
            want = lora.peft_linear_ref(xs[m:m + 1], W, ads[a][0], ads[a][1], ads[a][2]) - torch.nn.functional.linear(xs[m:m + 1], W.double())
            assert torch.allclose(d[m:m + 1], want, rtol=1e-12, atol=1e-12), m
        else:
            assert torch.isnan(d[m]).all()


def test_segments_follow_the_packed_rows():
    """q | k | v and the GLU-packed gate | up rows read their own R-segment of t: the rule on a packed [2I, R] B table equals the two
    projections computed apart."""
    from seedx_amd import lora
    g = torch.Generator().manual_seed(6)
    R, K = 8, 32
    seg = lora.seg_tables(H, I)
    assert seg["qkv"].tolist() == [0] * 4 + [1] * 4 + [2] * 4 and seg["gu"].tolist() == [0, 1] * (I // 16) and not seg["o"].any() and not seg["d"].any()
    x = torch.randn(3, K, generator=g).half()
    zero = torch.zeros_like(x)
    Au, Ag = torch.randn(R, K, generator=g).half(), torch.randn(R, K, generator=g).half()
    Bu, Bg = torch.randn(I, R, generator=g).half(), torch.randn(I, R, generator=g).half()
    sel = torch.zeros(3, dtype=torch.int32)
    d = lora.delta_ref(x, zero, torch.cat([Au, Ag])[None], lora.glu_pack_rows(Bu, Bg)[None], seg["gu"], torch.tensor([2.0]), sel)
    v = d.view(3, I // 16, 2, 16)
    up, gate = v[:, :, 0].reshape(3, I), v[:, :, 1].reshape(3, I)
    assert torch.allclose(up, 2.0 * (x.double() @ Au.double().T) @ Bu.double().T, rtol=1e-12, atol=1e-12)
    assert torch.allclose(gate, 2.0 * (x.double() @ Ag.double().T) @ Bg.double().T, rtol=1e-12, atol=1e-12)


def test_gemv_args_mirror_ends_with_the_addend_fields():
    """The ctypes mirror of sx_gemv_args: the new fields sit at the END (a zero-initialised struct of the old size prefix is unchanged)."""
    from seedx_amd import _lib
    names = [f[0] for f in _lib.GemvArgs._fields_]
    assert names[-3:] == ["addend", "addend_sel", "addend_n"] and names[-4] == "w_block_scale"
    a = _lib.GemvArgs()
    assert not a.addend and not a.addend_sel and a.addend_n == 0
    for fn in ("sx_lora_shrink", "sx_lora_expand", "sx_rmsnorm_planes_sel"):
        assert fn in _lib.SIGNATURES


def test_constructor_refusals_and_max_adapters_zero():
    """ValueError, never a fall-back: tensor-parallel ranks, the plain 16-bit flow, a model outside the tiled precise path, a rank table
    the kernels do not take. max_adapters=0 (the default) allocates and prices nothing."""
    from oracle import weights
    from seedx_amd.llama import LlamaForCausalLM
    from seedx_amd.parallel import Comm
    cfg = dict(weights.MINI_LLM)

    class _Two(Comm):
        def __init__(self):
            super().__init__()
            self.rank, self.world = 0, 2
    with pytest.raises(ValueError, match="single rank"):
        LlamaForCausalLM(dict(cfg), max_batch=4, comm=_Two(), max_adapters=1)
    with pytest.raises(ValueError, match="precise mode"):
        LlamaForCausalLM(dict(cfg), max_batch=4, precise=False, max_adapters=1)
    small = dict(cfg, hidden_size=192, intermediate_size=704, num_attention_heads=2)          # H < 256: no MFMA skinny GEMM
    with pytest.raises(ValueError, match="tiled precise decode path"):
        LlamaForCausalLM(small, max_batch=4, max_adapters=1)
    for bad in (0, 4, 12, 176):
        with pytest.raises(ValueError, match="lora_rank"):
            LlamaForCausalLM(dict(cfg), max_batch=4, max_adapters=1, lora_rank=bad)
    with pytest.raises(ValueError, match="max_adapters"):
        LlamaForCausalLM(dict(cfg), max_batch=4, max_adapters=-1)
    off = LlamaForCausalLM(dict(cfg), max_batch=4)
    assert off.max_adapters == 0 and off.adapters == [] and "adapters" not in off.memory_footprint()
    with pytest.raises(ValueError, match="max_adapters=0"):
        off.load_adapter("a", {})
    with pytest.raises(ValueError, match="max_adapters=0"):
        off._adapter_index("a")
    assert off._adapter_index(None) == -1
    on = LlamaForCausalLM(dict(cfg), max_batch=4, max_adapters=3, lora_rank=16)
    fp, fp0 = on.memory_footprint(), off.memory_footprint()
    H, I, Lc = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"]
    assert fp["adapters"] == 3 * (Lc * 2 * 16 * (8 * H + 3 * (H + I)) + (2 * Lc + 1) * H * 4 + 4)
    assert fp["total"] == fp0["total"] + fp["adapters"] and {k: v for k, v in fp.items() if k not in ("adapters", "total")} == \
        {k: v for k, v in fp0.items() if k != "total"}
    with pytest.raises(ValueError, match="unknown adapter"):
        on._adapter_index("nope")


def test_prefix_index_with_adapter_tagged_signatures():
    """KV rows depend on the adapter: with the adapter in every row's signature a record matches a prompt only under the same adapter,
    base requests keep their untagged records, and simulate_prefix predicts the sharing with the same tags."""
    from seedx_amd.inflight import PrefixIndex, plan_admission, simulate_prefix, tag_signatures
    ids = [1] + list(range(30, 50))
    assert tag_signatures(ids, None) == ids and tag_signatures(ids[:2], "a") == [(1, "a"), (30, "a")]
    idx = PrefixIndex(4)
    idx.record(0, ids, tag_signatures(ids, "a"), 0)
    idx.record(1, ids, tag_signatures(ids, None), 0)
    assert idx.match(ids, tag_signatures(ids, "a"), 0) == [(0, 20)]
    assert idx.match(ids, tag_signatures(ids, "b"), 0) == []
    assert idx.match(ids, tag_signatures(ids, None), 0) == [(1, 20)]
    # admission: the request under "b" gets no rows and no donor, the one under "a" keeps slot 0 in place
    plan, deferred = plan_admission(idx, [0, 1, 2, 3], [], [("rb", ids, tag_signatures(ids, "b")), ("ra", ids, tag_signatures(ids, "a"))], 8)
    assert not deferred and sorted((r, start, donor) for _, r, start, donor in plan) == [("ra", 20, None), ("rb", 0, None)]
    assert [g for g, r, _, _ in plan if r == "ra"] == [0] and [g for g, r, _, _ in plan if r == "rb"][0] not in (0,)
    # two equal prompts in one round under different adapters are not leader and follower; under one adapter they are
    prompts, lengths = [ids, ids, ids], [4, 4, 4]
    mixed = simulate_prefix(prompts, lengths, 4, min_tokens=8, adapters=["a", "b", None])
    same = simulate_prefix(prompts, lengths, 4, min_tokens=8, adapters=["a", "a", "a"])
    plain = simulate_prefix(prompts, lengths, 4, min_tokens=8)
    assert mixed["prefix_hit_tokens"] == 0 and mixed["prefill_tokens"] == 3 * len(ids)
    assert same["prefix_hit_tokens"] == plain["prefix_hit_tokens"] == 2 * (len(ids) - 1) and same["forked_tokens"] == plain["forked_tokens"]
    # fed-back rows carry the tag too: a second turn under the same adapter matches into them, under another adapter it does not
    index = PrefixIndex(2)
    gen = [[60, 61, 62, 63]]
    simulate_prefix([ids], [4], 2, min_tokens=8, generated=gen, index=index, adapters=["a"])
    turn2 = ids + gen[0][:3] + [70]
    assert index.match(turn2, tag_signatures(turn2, "a"), 0)[0][1] == len(ids) + 3
    assert index.match(turn2, tag_signatures(turn2, "b"), 0) == []
