"""Path C body — SDXL ``UNet2DConditionModel`` (diffusers 0.25.0 [ext]) on the HIP kernels.

The reference never defines the UNet: it instantiates diffusers' class from the SDXL-base config and overwrites
the weights with the adapter checkpoint (eval_seed_x_detokenizer.py:30-42, adapter_modules.py:62-65). This stand-in
accepts the same state-dict key names and call signature used at the reference call sites
(pipeline_stable_diffusion_xl_t2i_edit.py:915-922 ``unet(sample, t, encoder_hidden_states=…, added_cond_kwargs=…,
return_dict=False)[0]``; adapter_modules.py:45 ``.sample``) and the attributes the pipelines read
(``config.{sample_size, addition_time_embed_dim, in_channels}``, ``add_embedding.linear_1.in_features``, ``dtype``).

Layout: activations are NHWC ([B, H*W, C]) end to end, so Transformer2D's permute/reshape is free and every 3x3
conv is an implicit GEMM over (ky,kx,cin)-ordered weights. Residual streams are fp32, MFMA operands 16-bit.
Fusions: GroupNorm+SiLU(+16-bit copy for the 1x1 shortcut), conv+bias+time-embedding add(+residual),
q/k/v fused GEMM, GEGLU epilogue, nearest-2x upsample inside the conv gather, stride-2 downsample conv,
cross-attention K/V of the (step-invariant) conditioning cached across the 50 denoise steps, all time_emb_proj of a
step in one GEMM.
"""
import math
import os
import types

import torch

from . import ops
from .llama import glu_pack_rows

# LayerNorms of the transformer blocks folded into the GEMMs around them (ops.LnRows, sx_gemm_ln) wherever all of those GEMMs run on
# ping-pong tiles (CFG batch >= 16 at 1024 px): - 1.7 % on the 50-step loop, same-process A/B (profiles/r4_ab_experiments.md).
# SX_LN_FOLD=0 keeps the separate sx_layernorm launches (and saves the second copy of the folded weights, 2.5 GB).
LN_FOLD = os.environ.get("SX_LN_FOLD", "1") != "0"

SDXL_BASE_CONFIG = dict(in_channels=4, out_channels=4, block_out_channels=(320, 640, 1280), layers_per_block=2,
                        down_attn=(False, True, True), up_attn=(True, True, False), transformer_layers=(1, 2, 10),
                        heads=(5, 10, 20), cross_attention_dim=2048, addition_time_embed_dim=256, pooled_dim=1280,
                        norm_groups=32, sample_size=128)


class UNetOutput:
    def __init__(self, sample):
        self.sample = sample


class UNet2DConditionModel:
    def __init__(self, comm=None, **cfg):
        """comm (seedx_amd.parallel.Comm) with world > 1: ONE forward is sharded by pixel rows over the ranks of that
        communicator (seqpar.py — weights replicated, K|V all-gather per self-attention, conv halos, GroupNorm statistics
        all-reduce); every rank passes the same full inputs and receives the same full output."""
        from .parallel import Comm
        self.comm = comm or Comm()
        c = dict(SDXL_BASE_CONFIG)
        c.update(cfg)
        self.cfg = c
        self.config = types.SimpleNamespace(sample_size=c.get("sample_size", 128),
                                            addition_time_embed_dim=c["addition_time_embed_dim"],
                                            in_channels=c["in_channels"], out_channels=c["out_channels"])
        ted = c["block_out_channels"][0] * 4
        self.time_embed_dim = ted
        self.add_embedding = types.SimpleNamespace(
            linear_1=types.SimpleNamespace(in_features=6 * c["addition_time_embed_dim"] + c["pooled_dim"]))
        self.device, self.dtype = None, torch.float16
        self._sd, self._P = None, None
        self._ctx_key, self._ctx = None, None
        self._gn_arena, self._gn_next, self._n_gn_slots = None, 0, 64     # fused GroupNorm statistics slots per forward (47 used by SDXL)
        self._on_mark, self._mark_i, self._trace = None, 0, None
        self._ln_ok = {}                                                   # (rows, width) → LayerNorm fold usable (ops.ln_fold_ok)

    @classmethod
    def from_pretrained(cls, path, subfolder=None, **kw):
        """diffusers directory layout: <path>/<subfolder>/{config.json, diffusion_pytorch_model.safetensors}."""
        import json
        import os
        d = os.path.join(path, subfolder) if subfolder else path
        j = json.load(open(os.path.join(d, "config.json")))
        cfg = dict(in_channels=j["in_channels"], out_channels=j["out_channels"],
                   block_out_channels=tuple(j["block_out_channels"]), layers_per_block=j["layers_per_block"],
                   transformer_layers=tuple(j["transformer_layers_per_block"]), heads=tuple(j["attention_head_dim"]),
                   cross_attention_dim=j["cross_attention_dim"], addition_time_embed_dim=j["addition_time_embed_dim"],
                   pooled_dim=j["projection_class_embeddings_input_dim"] - 6 * j["addition_time_embed_dim"],
                   norm_groups=j["norm_num_groups"], sample_size=j["sample_size"],
                   down_attn=tuple("CrossAttn" in t for t in j["down_block_types"]),
                   up_attn=tuple("CrossAttn" in t for t in j["up_block_types"]))
        m = cls(**cfg)
        from safetensors.torch import load_file
        f = os.path.join(d, "diffusion_pytorch_model.safetensors")
        m.load_state_dict(load_file(f))
        return m

    # ---- state dict ------------------------------------------------------------------------------------------
    def expand_conv_in(self, in_channels):
        """conv_in [Co, 4, 3, 3] → [Co, in_channels, 3, 3], new input channels zero (adapter_modules.py:187-198)."""
        if self.cfg["in_channels"] == in_channels:
            return
        if self._sd is None and self._P is not None:
            raise RuntimeError("UNet2DConditionModel: weights already packed; expand conv_in before the first forward")
        if self._sd is not None:
            w = self._sd["conv_in.weight"]
            new = torch.zeros((w.shape[0], in_channels, w.shape[2], w.shape[3]), dtype=w.dtype)
            new[:, :w.shape[1]] = w
            self._sd = dict(self._sd)
            self._sd["conv_in.weight"] = new
        self.cfg["in_channels"] = self.config.in_channels = in_channels
        self._P = None

    def load_state_dict(self, sd, strict=True, prefix="", merge=False):
        if prefix:
            sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
        if merge and self._sd is not None:                      # overlay on the weights already held
            full = dict(self._sd)
            full.update(sd)
            sd = full
        need = ["conv_in.weight", "conv_out.weight", "time_embedding.linear_1.weight", "add_embedding.linear_2.bias",
                "mid_block.resnets.1.conv2.weight", "conv_norm_out.weight"]
        missing = [k for k in need if k not in sd]
        if missing and strict:
            raise KeyError(f"UNet2DConditionModel: missing keys {missing}")
        if "conv_in.weight" in sd and sd["conv_in.weight"].shape[1] != self.cfg["in_channels"]:
            # reference zero-extends conv_in 4→8 channels then loads the checkpoint (adapter_modules.py:187-198)
            self.cfg["in_channels"] = int(sd["conv_in.weight"].shape[1])
            self.config.in_channels = self.cfg["in_channels"]
        self._sd = sd
        self._P = None
        self._ctx_key = None
        return missing, []

    def to(self, device=None, dtype=None):
        old = (self.device, self.dtype)
        if device is not None:
            self.device = torch.device(device)
        if dtype is not None:
            assert dtype in (torch.float16, torch.bfloat16)
            self.dtype = dtype
        if (self.device, self.dtype) != old:
            if self._P is not None and self._sd is None:
                raise RuntimeError("weights were already packed for %s/%s; reload the state dict to move them" % old)
            self._P = None
            self._ctx_key = None
        return self

    def eval(self):
        return self

    def requires_grad_(self, flag=False):
        return self

    # ---- packing ------------------------------------------------------------------------------------------------
    def _pack(self):
        if self._P is not None:
            return self._P
        if self._sd is None:
            raise RuntimeError("UNet2DConditionModel: load_state_dict() first")
        if self.device is None or self.device.type != "cuda":
            raise RuntimeError("UNet2DConditionModel runs on the GPU only")
        sd, dev, dt, c = self._sd, self.device, self.dtype, self.cfg

        def f32(k):
            return sd[k].detach().to(dev, torch.float32).contiguous()

        def lin16(k):
            return sd[k].detach().to(dev, dt).contiguous()

        def conv16(k):  # [Co,Ci,3,3] → [Co, 9*Ci] with (ky,kx,ci) order
            w = sd[k].detach().to(dev, dt)
            return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()

        def resnet(n):
            r = dict(n1=(f32(n + ".norm1.weight"), f32(n + ".norm1.bias")), w1=conv16(n + ".conv1.weight"),
                     b1=f32(n + ".conv1.bias"), n2=(f32(n + ".norm2.weight"), f32(n + ".norm2.bias")),
                     w2=conv16(n + ".conv2.weight"), b2=f32(n + ".conv2.bias"), name=n)
            if n + ".conv_shortcut.weight" in sd:
                w = sd[n + ".conv_shortcut.weight"].detach().to(dev, dt)
                r["ws"] = w.reshape(w.shape[0], w.shape[1]).contiguous()
                r["bs"] = f32(n + ".conv_shortcut.bias")
            self._temb_names.append(n)
            return r

        def transformer(n, layers, heads):
            t = dict(norm=(f32(n + ".norm.weight"), f32(n + ".norm.bias")), pin_w=lin16(n + ".proj_in.weight"),
                     pin_b=f32(n + ".proj_in.bias"), pout_w=lin16(n + ".proj_out.weight"),
                     pout_b=f32(n + ".proj_out.bias"), heads=heads, blocks=[])
            for k in range(layers):
                b = f"{n}.transformer_blocks.{k}"
                ffw = sd[b + ".ff.net.0.proj.weight"].detach().to(dev, dt)
                ffb = sd[b + ".ff.net.0.proj.bias"].detach().to(dev, torch.float32)
                half = ffw.shape[0] // 2
                t["blocks"].append(dict(
                    n1=(f32(b + ".norm1.weight"), f32(b + ".norm1.bias")),
                    wqkv=torch.cat([lin16(b + f".attn1.{q}.weight") for q in ("to_q", "to_k", "to_v")], 0).contiguous(),
                    wo1=lin16(b + ".attn1.to_out.0.weight"), bo1=f32(b + ".attn1.to_out.0.bias"),
                    n2=(f32(b + ".norm2.weight"), f32(b + ".norm2.bias")),
                    wq2=lin16(b + ".attn2.to_q.weight"),
                    wkv2=torch.cat([lin16(b + ".attn2.to_k.weight"), lin16(b + ".attn2.to_v.weight")], 0).contiguous(),
                    wo2=lin16(b + ".attn2.to_out.0.weight"), bo2=f32(b + ".attn2.to_out.0.bias"),
                    n3=(f32(b + ".norm3.weight"), f32(b + ".norm3.bias")),
                    wff1=glu_pack_rows(ffw[:half].contiguous(), ffw[half:].contiguous()),      # hidden * gelu(gate)
                    bff1=glu_pack_rows(ffb[:half].reshape(-1, 1).contiguous(), ffb[half:].reshape(-1, 1).contiguous()).reshape(-1).contiguous(),
                    wff2=lin16(b + ".ff.net.2.weight"), bff2=f32(b + ".ff.net.2.bias")))
            if LN_FOLD:
                # LayerNorm folded into the projections behind it (ops.LnRows): gamma into a second copy of the weight, beta
                # into its bias; used for the shapes whose GEMMs all run on ping-pong tiles (decided per call in _transformer)
                for blk in t["blocks"]:
                    blk["f1"] = ops.fold_layernorm(blk["wqkv"], None, *blk["n1"])
                    blk["f2"] = ops.fold_layernorm(blk["wq2"], None, *blk["n2"])
                    blk["f3"] = ops.fold_layernorm(blk["wff1"], blk["bff1"], *blk["n3"])
            self._xattn.append(t)
            return t

        self._temb_names, self._xattn = [], []
        boc = c["block_out_channels"]
        P = {}
        cin = c["in_channels"]
        self.cin_kpad = (9 * cin + 63) // 64 * 64
        w = sd["conv_in.weight"].detach().to(dev, dt).permute(0, 2, 3, 1).reshape(boc[0], -1)
        wp = torch.zeros(boc[0], self.cin_kpad, dtype=dt, device=dev)
        wp[:, :w.shape[1]] = w
        P["conv_in_w"], P["conv_in_b"] = wp, f32("conv_in.bias")
        P["te1"] = (lin16("time_embedding.linear_1.weight"), f32("time_embedding.linear_1.bias"))
        P["te2"] = (lin16("time_embedding.linear_2.weight"), f32("time_embedding.linear_2.bias"))
        P["ae1"] = (lin16("add_embedding.linear_1.weight"), f32("add_embedding.linear_1.bias"))
        P["ae2"] = (lin16("add_embedding.linear_2.weight"), f32("add_embedding.linear_2.bias"))
        P["down"] = []
        for i, co in enumerate(boc):
            blk = dict(res=[], attn=[], down=None)
            for j in range(c["layers_per_block"]):
                blk["res"].append(resnet(f"down_blocks.{i}.resnets.{j}"))
                if c["down_attn"][i]:
                    blk["attn"].append(transformer(f"down_blocks.{i}.attentions.{j}", c["transformer_layers"][i], c["heads"][i]))
            if i != len(boc) - 1:
                n = f"down_blocks.{i}.downsamplers.0.conv"
                blk["down"] = (conv16(n + ".weight"), f32(n + ".bias"))
            P["down"].append(blk)
        P["mid"] = dict(res=[resnet("mid_block.resnets.0")], attn=[transformer("mid_block.attentions.0", c["transformer_layers"][-1], c["heads"][-1])])
        P["mid"]["res"].append(resnet("mid_block.resnets.1"))
        P["up"] = []
        rh, rl = list(reversed(c["heads"])), list(reversed(c["transformer_layers"]))
        for i in range(len(boc)):
            blk = dict(res=[], attn=[], up=None)
            for j in range(c["layers_per_block"] + 1):
                blk["res"].append(resnet(f"up_blocks.{i}.resnets.{j}"))
                if c["up_attn"][i]:
                    blk["attn"].append(transformer(f"up_blocks.{i}.attentions.{j}", rl[i], rh[i]))
            if i != len(boc) - 1:
                n = f"up_blocks.{i}.upsamplers.0.conv"
                blk["up"] = (conv16(n + ".weight"), f32(n + ".bias"))
                # the same weight as four 2x2 phase filters (16 taps per input pixel): used when the run-time shape passes the gate
                # (ops.conv3x3); the 36-tap copy stays for the other shapes and for the row-sharded forward
                # — summed in fp64 from the checkpoint's own values, rounded once to the operand dtype
                w = sd[n + ".weight"].detach().to(dev)
                blk["up_ph"] = ops.pack_upsample_phases(w.permute(0, 2, 3, 1).reshape(w.shape[0], -1), dtype=dt)
            P["up"].append(blk)
        P["norm_out"] = (f32("conv_norm_out.weight"), f32("conv_norm_out.bias"))
        wo = conv16("conv_out.weight")
        wop = torch.zeros(16, wo.shape[1], dtype=dt, device=dev)
        wop[:wo.shape[0]] = wo
        bo = torch.zeros(16, dtype=torch.float32, device=dev)
        bo[:wo.shape[0]] = f32("conv_out.bias")
        P["conv_out_w"], P["conv_out_b"] = wop, bo
        # every resnet's time_emb_proj in ONE weight: [sum(Co), ted]
        ws = [sd[n + ".time_emb_proj.weight"].detach().to(dev, dt) for n in self._temb_names]
        bs = [sd[n + ".time_emb_proj.bias"].detach().to(dev, torch.float32) for n in self._temb_names]
        P["temb_w"], P["temb_b"] = torch.cat(ws, 0).contiguous(), torch.cat(bs, 0).contiguous()
        off, P["temb_off"] = 0, {}
        for n, w_ in zip(self._temb_names, ws):
            P["temb_off"][n] = (off, w_.shape[0])
            off += w_.shape[0]
        self._P = P
        self._sd = None
        return P

    # ---- building blocks ---------------------------------------------------------------------------------------------
    # ---- pixel-row sharding helpers (identity for a single rank) -----------------------------------------------------
    def _gn(self, x, gb, eps, silu, Hc, Wc, want_raw=False, x2=None, stats=None):
        """GroupNorm of this rank's rows with statistics over the whole image (Hc x Wc global size).
        stats: ops.GnStats accumulated by the GEMM / conv that produced x (skips the zero + statistics launches)."""
        G, dt = self.cfg["norm_groups"], self.dtype
        return ops.groupnorm(x, gb[0], gb[1], G, eps, silu, dt, want_raw=want_raw, x2=x2, comm=self.comm, hw_total=Hc * Wc,
                             stats=stats)

    def _gn_slot(self, B, HW):
        """Next zeroed statistics slot of this forward's arena (None when the forward is row-sharded: the statistics then need
        the cross-rank all-reduce of the unfused path)."""
        if self._gn_arena is None:
            return None
        i = self._gn_next
        self._gn_next += 1
        if i >= self._gn_arena.shape[0]:
            return None
        return ops.GnStats(self._gn_arena[i], self.cfg["norm_groups"], HW)

    def _conv(self, h16, B, Hc, Wc, w, bias=None, bias2d=None, residual=None, stride=1, upsample=False, n_valid=0, gn=None,
              w_phases=None):
        """3x3 conv on this rank's slab. h16: 16-bit [B, Hl*Wc, Cin] (Hl = Hc / tp rows). Returns fp32 [B, Hl'*Wc', Cout].
        With tp > 1 the slab is extended by the neighbours' boundary rows (seqpar.with_halo) so that no output pixel sees a
        wrong zero padding; rows computed from the artificial padding of the halo itself are dropped."""
        tp = self.comm.world
        Cin = h16.shape[-1]
        if tp == 1:
            return ops.conv3x3(h16.view(B, Hc, Wc, Cin), w, bias=bias, bias2d=bias2d, residual=residual, stride=stride,
                               upsample=upsample, out_dtype=torch.float32, n_valid=n_valid, gn=gn, w_phases=w_phases)
        from . import seqpar
        Hl = Hc // tp
        Co = n_valid or w.shape[0]
        if stride == 2:
            # output row y reads input rows 2y-1 .. 2y+1: only the row ABOVE the slab is foreign. The slab gets that row on
            # top and a zero column on the left, and the kernel pads bottom/right only (pad_mode 1): tap (ky, kx) of output
            # (j, x) then lands on padded index (2j + ky, 2x + kx) = image pixel (2y - 1 + ky, 2x - 1 + kx). No waste.
            xin = seqpar.with_halo(h16, self.comm, Hl, Wc, left_col=True, bottom=False)
            out = ops.conv3x3(xin, w, bias=bias, bias2d=bias2d, stride=2, pad_mode=1, out_dtype=torch.float32)
            assert residual is None
            return out.view(B, (Hl // 2) * (Wc // 2), Co)
        xin = seqpar.with_halo(h16, self.comm, Hl, Wc)                          # [B, Hl + 2, Wc, Cin]
        out = ops.conv3x3(xin, w, bias=bias, bias2d=bias2d, upsample=upsample, out_dtype=torch.float32, n_valid=n_valid)
        f = 2 if upsample else 1
        out = out.view(B, f * (Hl + 2), f * Wc, Co)[:, f:f * (Hl + 1)].reshape(B, f * Hl * f * Wc, Co).contiguous()
        if residual is not None:
            out = ops.add(out, residual.reshape(out.shape).contiguous())
        return out

    # ---- building blocks ---------------------------------------------------------------------------------------------
    def _resnet(self, r, x, B, Hc, Wc, temb_all, skip=None, st_in=None):
        """x: fp32 [B, HW, Ci] → fp32 [B, HW, Co]  (diffusers ResnetBlock2D [ext]).
        skip: fp32 [B, HW, Cs] — the block input is torch.cat([x, skip], dim=1) (up blocks); the concatenation is never
        built: norm1 reads both tensors and emits the 16-bit operands of conv1 and of the 1x1 shortcut.
        (HW = this rank's rows of the Hc x Wc image when the forward is row-sharded.)
        st_in: GroupNorm statistics of x accumulated by its producer. Returns (out, statistics of out accumulated by conv2)."""
        Ci = x.shape[-1] + (skip.shape[-1] if skip is not None else 0)
        if "ws" in r:
            h, raw = self._gn(x, r["n1"], 1e-5, True, Hc, Wc, want_raw=True, x2=skip)
        else:
            assert skip is None
            h = self._gn(x, r["n1"], 1e-5, True, Hc, Wc, stats=st_in)
        off, Co = self._P["temb_off"][r["name"]]
        HW = x.shape[1]
        st2 = self._gn_slot(B, HW)
        h = self._conv(h, B, Hc, Wc, r["w1"], bias=r["b1"], bias2d=temb_all[:, off:off + Co], gn=st2)
        h = self._gn(h, r["n2"], 1e-5, True, Hc, Wc, stats=st2)
        if "ws" in r:
            sc = ops.gemm(raw.view(-1, Ci), r["ws"], bias=r["bs"], out_dtype=torch.float32)
        else:
            sc = x.view(-1, Ci)
        st_out = self._gn_slot(B, HW)
        out = self._conv(h, B, Hc, Wc, r["w2"], bias=r["b2"], residual=sc, gn=st_out).view(B, -1, Co)
        self._mark(out)
        return out, st_out

    def _transformer(self, t, x, B, ctx_kv, Hc, Wc, st_in=None):
        """Transformer2DModel with use_linear_projection [ext]. x: fp32 [B, HW, C] (this rank's rows of the Hc x Wc image);
        ctx_kv: list of cached cross-attention K|V tensors [B, L, 2, heads, 64] for this transformer's blocks."""
        dt, heads = self.dtype, t["heads"]
        _, HW, C = x.shape
        hd = C // heads
        scale = hd ** -0.5
        sp = self.comm.world > 1
        h = self._gn(x, t["norm"], 1e-6, False, Hc, Wc, stats=st_in)
        nb = len(t["blocks"])
        M = B * HW
        if LN_FOLD and not sp and "f1" in t["blocks"][0] and self._ln_fold_ok(M, C):
            # every LayerNorm of the blocks rides on its neighbours: the projection ahead of it (proj_in / out-projections / ff2,
            # fp32 residual stream) also emits the 16-bit copy and the rows' sums, the projection behind it applies (mu, rstd)
            arena = torch.zeros((3 * nb, M, 2), dtype=torch.float64, device=x.device)      # one fill launch

            def rows(i):
                return ops.LnRows(M, C, dt, x.device, stats=arena[i])
            ln = rows(0)
            hs = ops.gemm(h.view(-1, C), t["pin_w"], bias=t["pin_b"], out_dtype=torch.float32, ln_emit=ln)
            for k, b in enumerate(t["blocks"]):
                w, cs, bb = b["f1"]
                qkv = ops.gemm(ln.x16, w, bias=bb, ln_apply=(ln, cs, 1e-5)).view(B, HW, 3, heads, hd)
                att = ops.attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], scale)
                ln = rows(3 * k + 1)
                hs = ops.gemm(att.view(-1, C), b["wo1"], bias=b["bo1"], residual=hs, out_dtype=torch.float32, ln_emit=ln)
                self._mark(hs)
                w, cs, bb = b["f2"]
                q = ops.gemm(ln.x16, w, bias=bb, ln_apply=(ln, cs, 1e-5)).view(B, HW, heads, hd)
                kv = ctx_kv[k]
                att = ops.attention(q, kv[:, :, 0], kv[:, :, 1], scale)
                ln = rows(3 * k + 2)
                hs = ops.gemm(att.view(-1, C), b["wo2"], bias=b["bo2"], residual=hs, out_dtype=torch.float32, ln_emit=ln)
                w, cs, bb = b["f3"]
                g = ops.gemm(ln.x16, w, bias=bb, act="gelu", glu=True, ln_apply=(ln, cs, 1e-5))
                if k == nb - 1:
                    hs = ops.gemm(g, b["wff2"], bias=b["bff2"], residual=hs, out_dtype=dt)
                else:
                    ln = rows(3 * k + 3)
                    hs = ops.gemm(g, b["wff2"], bias=b["bff2"], residual=hs, out_dtype=torch.float32, ln_emit=ln)
                self._mark(hs)
            st_out = self._gn_slot(B, HW)
            out = ops.gemm(hs, t["pout_w"], bias=t["pout_b"], residual=x.view(-1, C), out_dtype=torch.float32, gn=st_out)
            return out.view(B, HW, C), st_out
        hs = ops.gemm(h.view(-1, C), t["pin_w"], bias=t["pin_b"], out_dtype=torch.float32)
        for k, b in enumerate(t["blocks"]):
            n = ops.layernorm(hs, b["n1"][0], b["n1"][1], 1e-5, dt)
            if not sp:
                qkv = ops.gemm(n, b["wqkv"]).view(B, HW, 3, heads, hd)
                att = ops.attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], scale)
            else:
                # row-sharded self-attention: the local K | V rows are projected first and their all-gather runs on the
                # communicator's side stream while the Q projection of the local rows is computed
                from . import seqpar
                kv_l = ops.gemm(n, b["wqkv"][C:]).view(B, HW, 2, heads, hd)
                pending = self.comm.all_gather_async(kv_l)
                q = ops.gemm(n, b["wqkv"][:C]).view(B, HW, heads, hd)
                g = pending.wait()                                              # [tp, B, HWl, 2, heads, hd]
                kv = g.permute(1, 0, 2, 3, 4, 5).reshape(B, g.shape[0] * HW, 2, heads, hd).contiguous()
                att = ops.attention(q, kv[:, :, 0], kv[:, :, 1], scale)
            hs = ops.gemm(att.view(-1, C), b["wo1"], bias=b["bo1"], residual=hs, out_dtype=torch.float32)
            self._mark(hs)
            n = ops.layernorm(hs, b["n2"][0], b["n2"][1], 1e-5, dt)
            q = ops.gemm(n, b["wq2"]).view(B, HW, heads, hd)
            kv = ctx_kv[k]
            att = ops.attention(q, kv[:, :, 0], kv[:, :, 1], scale)
            hs = ops.gemm(att.view(-1, C), b["wo2"], bias=b["bo2"], residual=hs, out_dtype=torch.float32)
            n = ops.layernorm(hs, b["n3"][0], b["n3"][1], 1e-5, dt)
            g = ops.gemm(n, b["wff1"], bias=b["bff1"], act="gelu", glu=True)
            last = k == nb - 1
            hs = ops.gemm(g, b["wff2"], bias=b["bff2"], residual=hs, out_dtype=dt if last else torch.float32)
            self._mark(hs)
        st_out = self._gn_slot(B, HW)
        out = ops.gemm(hs, t["pout_w"], bias=t["pout_b"], residual=x.view(-1, C), out_dtype=torch.float32, gn=st_out)
        return out.view(B, HW, C), st_out

    def _ln_fold_ok(self, M, C):
        # cached per (rows, width): the cost model's answer is a pure function of the shape. (sx_gemm_force_tile is a lab / test hook;
        # a caller that forces tiles clears ``_ln_ok`` — tools/bench_unet_ab.py does)
        key = (M, C)
        if key not in self._ln_ok:
            self._ln_ok[key] = ops.ln_fold_ok(M, C, consumers=[(3 * C, False), (C, False), (8 * C, True)], producers=[C, 4 * C])
        return self._ln_ok[key]

    def prepare_context(self, encoder_hidden_states):
        """Cross-attention K/V of every transformer block for this conditioning (constant over the denoise loop)."""
        P = self._pack()
        ehs = encoder_hidden_states
        key = (ehs.data_ptr(), ehs._version, tuple(ehs.shape))
        if self._ctx_key == key:
            return self._ctx
        B, L, ca = ehs.shape
        e16 = ops.cast(ehs.to(self.device).float().contiguous(), self.dtype).view(B * L, ca)
        ctx = []
        for t in self._xattn:
            heads = t["heads"]
            per = []
            for b in t["blocks"]:
                C = b["wq2"].shape[0]
                kv = ops.gemm(e16, b["wkv2"]).view(B, L, 2, heads, C // heads)
                per.append(kv)                                          # K | V of the context (step-invariant)
            ctx.append(per)
        self._ctx_key, self._ctx = key, ctx
        return ctx

    def time_embeddings(self, t_vals, idx_dev, text_embeds, time_ids, B, ts=None):
        """emb = time_embedding(sinusoid(t)) + add_embedding([text_embeds | sinusoid(time_ids)]); returns the fused
        per-resnet time adds [B, sum(Co)] fp32. t_vals: fp32 device tensor of timesteps; idx_dev: optional device int
        index into it (graph-replayable denoise step). ``ts``: the sinusoid [B, block_out_channels[0]] itself, already computed
        (the slot loop: one timestep per slot, ops.timestep_embedding_slots) — t_vals / idx_dev are then not read."""
        P, dt, c = self._P, self.dtype, self.cfg
        boc0 = c["block_out_channels"][0]
        if ts is None:
            ts = ops.timestep_embedding(t_vals, boc0, dt, idx_dev=idx_dev, n=B)
        assert ts.shape == (B, boc0) and ts.dtype == dt
        e = ops.gemm(ts, P["te1"][0], bias=P["te1"][1], act="silu")
        e = ops.gemm(e, P["te2"][0], bias=P["te2"][1], out_dtype=torch.float32)
        tid = ops.timestep_embedding(time_ids.reshape(-1).float().contiguous(), c["addition_time_embed_dim"], torch.float32)
        add = torch.empty((B, self.add_embedding.linear_1.in_features), dtype=torch.float32, device=self.device)
        ops.copy2d(text_embeds.float().contiguous(), add, 0)
        ops.copy2d(tid.view(B, -1), add, text_embeds.shape[1])
        a = ops.gemm(ops.cast(add, dt), P["ae1"][0], bias=P["ae1"][1], act="silu")
        emb = ops.gemm(a, P["ae2"][0], bias=P["ae2"][1], residual=e, out_dtype=torch.float32)
        return ops.gemm(ops.silu_cast(emb, dt), P["temb_w"], bias=P["temb_b"], out_dtype=torch.float32)

    def _mark(self, t=None):
        """Progress mark of the running forward (after every resnet, in the middle and at the end of every transformer layer):
        ``forward_nhwc(on_mark=f)`` calls f(i) at mark i — the denoise loop's staggered kernel chains record their start events there.
        ``self._trace`` (a list, tools/determinism_trace.py): the residual stream at every mark is appended to it."""
        if self._trace is not None and t is not None:
            self._trace.append(t.detach().float().clone())
        if self._on_mark is not None:
            self._mark_i += 1
            self._on_mark(self._mark_i)

    def forward_nhwc(self, x_in, temb_all, ctx, B, H, W, on_mark=None):
        """x_in: fp32 [B, H*W, Cin] NHWC scaled latents → fp32 [B, H*W, 4] noise prediction. With a multi-rank ``comm`` every
        rank passes the full x_in, works on its H/tp pixel rows in between and returns the full (all-gathered) prediction."""
        P, dt, c = self._P, self.dtype, self.cfg
        self._on_mark, self._mark_i = on_mark, 0
        cin = c["in_channels"]
        tp, rank = self.comm.world, self.comm.rank
        if tp > 1:
            from . import seqpar
            assert H % (tp * 4) == 0, f"latent rows {H} must divide by 4 x the sharding degree {tp} (two 2x down-samplings)"
        col = ops.im2col3x3_small(x_in.view(B, H, W, cin), self.cin_kpad, dt)       # conv_in: replicated (36/72-wide K)
        x = ops.gemm(col, P["conv_in_w"], bias=P["conv_in_b"], out_dtype=torch.float32).view(B, H * W, -1)
        if tp > 1:
            x = seqpar.local_rows(x, rank, tp, H, W)
        skips = [(x, H, W)]
        ti = 0
        Hc, Wc = H, W
        # GroupNorm statistics ride on the epilogue of the GEMM / conv that produces each normalised tensor (ops.GnStats): one
        # zeroed fp64 arena per forward, one slot per producer. Not when row-sharded (cross-rank statistics).
        self._gn_arena = ops.GnStats.arena(self._n_gn_slots, B, c["norm_groups"], x.device) if tp == 1 else None
        self._gn_next = 0
        st = None                                                    # statistics of x, if its producer accumulated them
        for blk in P["down"]:
            for j, r in enumerate(blk["res"]):
                x, st = self._resnet(r, x, B, Hc, Wc, temb_all, st_in=st)
                if blk["attn"]:
                    x, st = self._transformer(blk["attn"][j], x, B, ctx[ti], Hc, Wc, st_in=st)
                    ti += 1
                skips.append((x, Hc, Wc))
            if blk["down"] is not None:
                st = self._gn_slot(B, (Hc // 2) * (Wc // 2))
                x = self._conv(ops.cast(x, dt), B, Hc, Wc, blk["down"][0], bias=blk["down"][1], stride=2, gn=st)
                Hc, Wc = Hc // 2, Wc // 2
                skips.append((x, Hc, Wc))
        x, st = self._resnet(P["mid"]["res"][0], x, B, Hc, Wc, temb_all, st_in=st)
        x, st = self._transformer(P["mid"]["attn"][0], x, B, ctx[ti], Hc, Wc, st_in=st)
        ti += 1
        x, st = self._resnet(P["mid"]["res"][1], x, B, Hc, Wc, temb_all, st_in=st)
        for blk in P["up"]:
            for j, r in enumerate(blk["res"]):
                s, _, _ = skips.pop()
                x, st = self._resnet(r, x.contiguous(), B, Hc, Wc, temb_all, skip=s)   # torch.cat([x, skip], dim=1), fused (norm1 over
                if blk["attn"]:                                                        # the concatenation keeps its own statistics pass)
                    x, st = self._transformer(blk["attn"][j], x, B, ctx[ti], Hc, Wc, st_in=st)
                    ti += 1
            if blk["up"] is not None:
                x = self._conv(ops.cast(x, dt), B, Hc, Wc, blk["up"][0], bias=blk["up"][1], upsample=True, w_phases=blk["up_ph"])
                Hc, Wc = Hc * 2, Wc * 2
                st = None
        h = self._gn(x, P["norm_out"], 1e-5, True, Hc, Wc, stats=st)
        self._gn_arena = None
        self._on_mark = None
        nv = 4 if c["out_channels"] == 4 else 0
        out = self._conv(h, B, Hc, Wc, P["conv_out_w"], bias=P["conv_out_b"], n_valid=nv)
        out = out.view(B, -1, out.shape[-1])
        if tp > 1:
            out = seqpar.gather_rows(out, self.comm)
            # a halo exchange / collective that timed out returned WITHOUT its payload (IpcComm's sticky status, also of the
            # neighbour-only child communicator): one 4-byte read-back per forward turns that into an error instead of a wrong image
            if not torch.cuda.is_current_stream_capturing():
                self.comm.check()
        return out

    # ---- diffusers-compatible call ---------------------------------------------------------------------------------------
    def forward(self, sample, timestep, encoder_hidden_states, added_cond_kwargs=None, cross_attention_kwargs=None,
                return_dict=True, **_):
        """NCHW in / NCHW out, like diffusers. Used for parity tests and by callers that drive their own loop; the
        built-in pipelines use the NHWC fast path (forward_nhwc) under a HIP graph."""
        self._pack()
        assert added_cond_kwargs is not None and "text_embeds" in added_cond_kwargs and "time_ids" in added_cond_kwargs
        B, Cin, H, W = sample.shape
        assert Cin == self.cfg["in_channels"]
        dev = self.device
        t = torch.as_tensor(timestep, dtype=torch.float32, device=dev).reshape(-1)
        t = t.expand(B).contiguous() if t.numel() == 1 else t
        temb = self.time_embeddings(t, None, added_cond_kwargs["text_embeds"].to(dev), added_cond_kwargs["time_ids"].to(dev), B)
        ctx = self.prepare_context(encoder_hidden_states.to(dev))
        x = ops.nchw_to_nhwc(sample.to(dev, torch.float32))
        eps = self.forward_nhwc(x, temb, ctx, B, H, W)
        out = ops.nhwc_to_nchw(eps, self.cfg["out_channels"], H, W).to(sample.dtype if sample.dtype != torch.float64 else torch.float32)
        if not return_dict:
            return (out,)
        return UNetOutput(out)

    __call__ = forward
