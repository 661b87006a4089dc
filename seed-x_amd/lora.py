"""Per-request LoRA adapters kept UNMERGED beside one resident base model: the rule in fp64, the PEFT key parsing and the table layout.

The reference freezes LLaMA and trains LoRA modules (configs/clm_models/llm_seed_x_lora.yaml: r 32, lora_alpha 32 on q/k/v/o/gate/up/down,
the three norms in ``modules_to_save``) and serves them through peft's ``Linear.forward`` (proj/peft/src/peft/tuners/lora.py:808-825,
dropout off at inference):  y = W x + s · B (A x),  s = lora_alpha / r.  The kernels of csrc/lora.hip compute, per activation row with
adapter index a (``sel``), for x carried as two 16-bit planes x = hi + lo:

    t[i]     = Σ_k A_a[i][k] · (hi[k] + lo[k])        fp32 accumulation, t stays fp32      (sx_lora_shrink)
    delta[n] = s_a · Σ_j B_a[n][j] · t[j]             fp32                                  (sx_lora_expand)
    y        = epilogue( acc(W, x) · (row scale / rstd) + delta )                           (sx_gemv addend / sx_gemm bias2d)

The delta enters BEFORE activation, GLU and residual. A row whose index is outside [0, n_adapters) is a base row. This module states that
rule on the host in fp64 (what the kernel tests compare against), parses PEFT state dicts (shared with llama.merge_peft_lora) and lays an
adapter out as the tables the kernels read. Pure torch, no GPU.
"""
import torch

PROJECTIONS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
NORMS = ("input_layernorm", "post_attention_layernorm")
_PRE = "base_model.model."


# ---- the rule, fp64 -------------------------------------------------------------------------------------------------------------
def _in_range(sel, n):
    return (sel >= 0) & (sel < n)


def shrink_ref(hi, lo, A, sel):
    """t fp64 [M, S*R]: hi / lo [M, K] (the two planes), A [n_adapters, S*R, K], sel int [M]. Base rows are NaN: nothing defines them."""
    x = hi.double() + lo.double()
    A, sel = A.double(), sel.long()
    t = torch.full((x.shape[0], A.shape[1]), float("nan"), dtype=torch.float64)
    for m in torch.nonzero(_in_range(sel, A.shape[0])).flatten().tolist():
        t[m] = A[sel[m]] @ x[m]
    return t


def expand_ref(t, B, seg, scale, sel):
    """delta fp64 [M, N]: t [M, S*R], B [n_adapters, N, R] (rows in the order of W as packed), seg int [N/16] (the S-segment of t a 16-row
    group of W reads), scale [n_adapters]. Base rows are NaN."""
    B, sel, t = B.double(), sel.long(), t.double()
    n_ad, N, R = B.shape
    col = (seg.long().repeat_interleave(16)[:, None] * R + torch.arange(R)[None, :])         # [N, R] columns of t
    d = torch.full((t.shape[0], N), float("nan"), dtype=torch.float64)
    for m in torch.nonzero(_in_range(sel, n_ad)).flatten().tolist():
        a = sel[m]
        d[m] = float(scale[a]) * (B[a] * t[m][col]).sum(dim=1)
    return d


def delta_ref(hi, lo, A, B, seg, scale, sel):
    """shrink_ref then expand_ref: the pre-activation addend of every row (NaN for base rows)."""
    return expand_ref(shrink_ref(hi, lo, A, sel), B, seg, scale, sel)


def peft_linear_ref(x, W, A, B, lora_alpha):
    """peft's Linear.forward restated in plain torch, fp64 (lora.py:808-825 with dropout off): result = F.linear(x, W);
    result += lora_B(lora_A(x)) * scaling, scaling = lora_alpha / r."""
    x = x.double()
    result = torch.nn.functional.linear(x, W.double())
    result = result + torch.nn.functional.linear(torch.nn.functional.linear(x, A.double()), B.double()) * (float(lora_alpha) / A.shape[0])
    return result


# ---- PEFT state dicts ---------------------------------------------------------------------------------------------------------------
def split_peft_state_dict(sd, adapter="default"):
    """A PeftModel (LoRA) state dict, or a bare adapter file → (plain, lora, saved, embedding):
      plain      the wrapped model's own keys (``base_model.model.`` prefix, ``.original_module.`` / ``.base_layer.`` dropped), with the
                 ``modules_to_save`` copies of ``adapter`` in place of the wrapped module's weight,
      lora       {module path: {"A": lora_A [r, K], "B": lora_B [N, r]}} of ``adapter`` (``X.lora_A.<adapter>.weight`` or, as adapter
                 files are saved, ``X.lora_A.weight``),
      saved      the keys of ``plain`` that came from ``modules_to_save``,
      embedding  the ``lora_embedding_*`` keys met (never used: merging skips them, serving refuses them).
    The one parser behind llama.merge_peft_lora (merge at load) and AdapterTables (serve unmerged)."""
    out, lora, saved, emb = {}, {}, [], []
    for k, v in sd.items():
        k = k[len(_PRE):] if k.startswith(_PRE) else k
        if ".lora_A." in k or ".lora_B." in k:
            mod, rest = k.split(".lora_", 1)
            which, ad = rest.split(".")[0], rest.split(".")[1]
            if ad == adapter or rest.split(".")[1] == "weight":
                lora.setdefault(mod, {})[which] = v
            continue
        if ".lora_embedding_" in k:
            emb.append(k)
            continue
        if ".lora_dropout." in k:
            continue
        if ".modules_to_save." in k:
            mod, rest = k.split(".modules_to_save.", 1)
            if rest.split(".")[0] == adapter:
                out[mod + "." + rest.split(".", 1)[1]] = v
                saved.append(mod + "." + rest.split(".", 1)[1])
            continue
        k = k.replace(".original_module.", ".").replace(".base_layer.", ".")
        out.setdefault(k, v)
    return out, lora, saved, emb


def glu_pack_rows(lin, gate):
    """llama.glu_pack_rows for any trailing width: [I, C] linear rows and gate rows → [2I, C] in 32-row groups [16 linear | 16 gate]."""
    I, Cc = lin.shape
    assert I % 16 == 0
    return torch.cat([lin.reshape(I // 16, 16, Cc), gate.reshape(I // 16, 16, Cc)], dim=1).reshape(2 * I, Cc).contiguous()


def seg_tables(H, I):
    """The S-segment of t each 16-row group of a projection's weight (as packed) reads: q|k|v rows → 0 / 1 / 2, the GLU-packed gate|up
    rows → 0 for a group of up ("linear") rows and 1 for a group of gate rows, o and down → 0. int32 [N / 16] each."""
    assert H % 16 == 0 and I % 16 == 0
    i32 = lambda t: t.to(torch.int32).contiguous()
    return {"qkv": i32(torch.arange(3 * H // 16) // (H // 16)), "o": i32(torch.zeros(H // 16)),
            "gu": i32(torch.arange(2 * I // 16) % 2), "d": i32(torch.zeros(H // 16))}


class AdapterTables:
    """One adapter in the layout the kernels read (single rank), from a PEFT-style state dict. Per layer li, 16-bit ``dtype``:
      A["qkv"][li] [3R, H] (q | k | v), A["o"][li] [R, H], A["gu"][li] [2R, H] (up | gate), A["d"][li] [R, I],
      B["qkv"][li] [3H, R], B["o"][li] [H, R], B["gu"][li] [2I, R] (GLU-packed like the weight), B["d"][li] [H, R],
    zero-padded from the adapter's rank r to the table rank R (exact: the padded products are 0), a projection the adapter does not
    target all zero; ``ln1`` / ``ln2`` [L] and ``norm``: the fp32 modules_to_save gammas or None (the base gamma holds); ``scale`` =
    lora_alpha / r. ValueError on anything the unmerged path does not cover, never a partial load."""

    def __init__(self, sd, L, H, I, R=32, lora_alpha=32, dtype=torch.float16, adapter="default"):
        plain, lora, saved, emb = split_peft_state_dict(sd, adapter)
        if emb:
            raise ValueError(f"adapter carries lora_embedding_* weights ({emb[0]}): embedding deltas are not served unmerged")
        bad = [k for k in list(lora) + saved if "embed_tokens" in k or "lm_head" in k]
        if bad:
            raise ValueError(f"adapter carries embed_tokens / lm_head weights ({bad[0]}): only the seven projections and the norms are served unmerged")
        ranks = set()
        mods = {}
        for mod, ab in lora.items():
            parts = mod.split(".")
            ok = len(parts) == 5 and parts[:2] == ["model", "layers"] and parts[2].isdigit() and int(parts[2]) < L and parts[4] in PROJECTIONS \
                and parts[3] == ("self_attn" if parts[4] in PROJECTIONS[:4] else "mlp")
            if not ok:
                raise ValueError(f"adapter targets {mod}: only {', '.join(PROJECTIONS)} of the decoder layers are served unmerged")
            if "A" not in ab or "B" not in ab:
                raise ValueError(f"adapter: {mod} has only one of lora_A / lora_B")
            if ab["A"].shape[0] != ab["B"].shape[1]:
                raise ValueError(f"adapter: {mod} lora_A {tuple(ab['A'].shape)} and lora_B {tuple(ab['B'].shape)} disagree on the rank")
            ranks.add(int(ab["A"].shape[0]))
            mods[(int(parts[2]), parts[4])] = ab
        if len(ranks) > 1:
            raise ValueError(f"adapter mixes ranks {sorted(ranks)}: one lora_alpha / r scale per adapter")
        self.r = ranks.pop() if ranks else 0
        if self.r > R:
            raise ValueError(f"adapter rank {self.r} exceeds the table rank lora_rank = {R}")
        gam = {}
        for k in saved:
            parts = k.split(".")
            if k == "model.norm.weight":
                gam["norm"] = plain[k]
            elif len(parts) == 5 and parts[:2] == ["model", "layers"] and parts[2].isdigit() and int(parts[2]) < L and parts[3] in NORMS \
                    and parts[4] == "weight":
                gam[(int(parts[2]), parts[3])] = plain[k]
            else:
                raise ValueError(f"adapter saves {k}: only input_layernorm, post_attention_layernorm and model.norm are served per adapter")
        self.R, self.L, self.H, self.I, self.dtype = int(R), L, H, I, dtype
        self.lora_alpha = float(lora_alpha)
        self.scale = self.lora_alpha / self.r if self.r else 0.0
        dims = {"q_proj": (H, H), "k_proj": (H, H), "v_proj": (H, H), "o_proj": (H, H), "gate_proj": (I, H), "up_proj": (I, H), "down_proj": (H, I)}

        def ab(li, name):
            N, K = dims[name]
            A, B = torch.zeros(R, K, dtype=dtype), torch.zeros(N, R, dtype=dtype)
            m = mods.get((li, name))
            if m is not None:
                if tuple(m["A"].shape) != (self.r, K) or tuple(m["B"].shape) != (N, self.r):
                    raise ValueError(f"adapter: layer {li} {name} has lora_A {tuple(m['A'].shape)} / lora_B {tuple(m['B'].shape)}, expected "
                                     f"({self.r}, {K}) / ({N}, {self.r})")
                A[:self.r], B[:, :self.r] = m["A"].detach().to(dtype), m["B"].detach().to(dtype)
            return A, B
        self.A = {k: [] for k in ("qkv", "o", "gu", "d")}
        self.B = {k: [] for k in ("qkv", "o", "gu", "d")}
        for li in range(L):
            (Aq, Bq), (Ak, Bk), (Av, Bv) = ab(li, "q_proj"), ab(li, "k_proj"), ab(li, "v_proj")
            self.A["qkv"].append(torch.cat([Aq, Ak, Av])), self.B["qkv"].append(torch.cat([Bq, Bk, Bv]))
            Ao, Bo = ab(li, "o_proj")
            self.A["o"].append(Ao), self.B["o"].append(Bo)
            (Au, Bu), (Ag, Bg) = ab(li, "up_proj"), ab(li, "gate_proj")
            self.A["gu"].append(torch.cat([Au, Ag])), self.B["gu"].append(glu_pack_rows(Bu, Bg))
            Ad, Bd = ab(li, "down_proj")
            self.A["d"].append(Ad), self.B["d"].append(Bd)
        f32 = lambda t: None if t is None else t.detach().float().contiguous()
        self.ln1 = [f32(gam.get((li, NORMS[0]))) for li in range(L)]
        self.ln2 = [f32(gam.get((li, NORMS[1]))) for li in range(L)]
        self.norm = f32(gam.get("norm"))

    def nbytes(self):
        """Bytes of the 16-bit tables of one adapter slot (what LlamaForCausalLM(max_adapters=n) holds n times, plus the gammas)."""
        return sum(t.numel() * 2 for d in (self.A, self.B) for ts in d.values() for t in ts)

    def delta_weight(self, li, name):
        """s · B A of one projection in fp32 from the TABLES (rounded to the table dtype, unpacked): what merge_peft_lora adds to W."""
        R, H, I = self.R, self.H, self.I
        j = {"q_proj": 0, "k_proj": 1, "v_proj": 2}
        if name in j:
            A, B = self.A["qkv"][li][j[name] * R:(j[name] + 1) * R], self.B["qkv"][li][j[name] * H:(j[name] + 1) * H]
        elif name == "o_proj":
            A, B = self.A["o"][li], self.B["o"][li]
        elif name == "down_proj":
            A, B = self.A["d"][li], self.B["d"][li]
        else:
            s = 0 if name == "up_proj" else 1
            A = self.A["gu"][li][s * R:(s + 1) * R]
            B = self.B["gu"][li].reshape(I // 16, 2, 16, R)[:, s].reshape(I, R)
        return (B.float() @ A.float()) * self.scale
