"""Path B — Llama-style decoder on the HIP kernels (prefill on MFMA, single-token decode on the HBM-bound
GEMV path, device-resident greedy loop captured in a HIP graph, optional lock-step batching of independent sequences).

Mirrors ``src/models/mllm/modeling_llama_xformer.py`` (``LlamaForCausalLM``: ``forward`` :643-746 semantics —
logits, past_key_values, hidden_states with the LAST entry = post-final-norm state :595-599 —,
``get_input_embeddings`` :623) with the reference's state-dict key names. Differences by design:
  * KV cache is pre-allocated [layer][seq][head][Tmax][hd] and appended in place by the fused RoPE kernel, instead of
    ``torch.cat`` every step (:215-220)
  * q/k/v and gate/up projections are fused GEMMs (weights concatenated / GLU-packed at load)
  * the 4 NaN/Inf guards (:702-713) and the per-layer ``attention_mask.sum()`` sync (:236) are dropped: prefill and
    multi-token chunks are causal (bottom-right aligned), q_len == 1 attends to the whole cache — same math
  * the generate loop only produces the last position's logits (``forward`` returns all positions like the reference)
  * ``max_batch`` > 1: G independent sequences (separate KV caches / positions) decode in lock step, so the 25.7 GB of
    weights are streamed from HBM once per step for all G tokens (the reference is batch 1 only, seed_x.py:191)
  * ``precise`` (default on; ``SX_LLM_PRECISE=0`` or ``precise=False`` for the plain 16-bit flow): fp32-grade activations — every GEMM
    A operand travels as two 16-bit planes x = hi + lo (the 16-bit checkpoint weights are exact and stream once), q / k / v, RoPE, the
    K cache and attention stay fp32 (csrc/precise.hip; v is stored in 16 bits in fp16 models: the mixed cache). 40 layers at 13B dims:
    logits 5.6e-4 / 5.9e-4 (prefill / decode; 2.9e-5 with the all-fp32 cache) from the reference evaluated in fp32, asserted at 1e-3 (2.3e-3 without;
    the per-site budget is tools/llm_error_budget.py). Measured cost (profiles/r5_llm_precise_ab.log): + 1.8 % of a
    headline step — the LLM phases themselves + 49 % (462 → 688 ms: prefill 2.3x, token step 6.0 → 7.7 ms at 16 sequences).
    MEMORY: the KV cache is fp32 for K and — round 6, fp16 models — 16-bit for V ("mixed" cache, ``kv_v16``; bf16 models and
    ``kv_v16=False`` keep fp32 V) — L·G·heads·Tmax·hd·(4 + 2 | 4) B = 5.0 | 6.7 GB per sequence at 13B dims with
    Tmax = 4096, 1.26 | 1.68 GB at Tmax = 1024 (pass ``max_cache_len``: the cache is sized from it, 0.63 | 0.84 GB per sequence at 512;
    ``kv_format="fp8_e4m3"``, below, holds 0.43 GB at 1024) — and the decode-tile copy of the
    weights (+ 25.7 GB at 13B) exists for every batch size, not only G >= 5; ``memory_footprint()`` returns the figures before
    anything is allocated, ``_pack`` logs them. The ``past_key_values`` views ``forward`` returns are fp32 in this mode (the reference
    returns the model dtype; they are views of the module's own cache and only meant to be handed back to ``forward``).
    Lock-step batches of 17..32 sequences stay in precise mode (round 6: four operand blocks per weight fragment, 10.9 ms per 32-sequence
    token step); ``SX_LLM_PRECISE32=0`` sends them to the plain 16-bit flow instead (2.0e-3 at 40 layers) — logged once at construction
  * ``kv_format="fp8_e4m3"`` (opt-in, lossy; or ``SX_LLM_KV=fp8_e4m3``; precise mode, head_dim 128, single rank): the KV cache holds OCP
    e4m3fn codes with one power-of-two fp32 scale per (token, head) row of k (after RoPE) and of v — uint8 [L][G][heads][Tmax][128] +
    fp32 [L][G][heads][Tmax], 264 B per (layer, head, token) instead of 768 (0.344 of the mixed cache). A row is rounded ONCE, when it is
    appended (quant.quantize_kv_rows is the rule, csrc/precise.hip quant_row8 the kernel); everything else is the fp32-grade path: the
    model computes, bit for bit, what the fp32-cache kernels compute on a cache holding the dequantised values.
    ``kv_format="fp8_e4m3_emulated"`` is that statement's other half, the bit-reference twin and test hook (in the spirit of
    sx_attention_f32_variant): ordinary all-fp32 caches, every append stores dequantise(quantise(row)), attention runs the existing fp32
    kernels — the same bits, no byte saving. The mode is NOT inside the 1e-3 contract: on the random-weight miniatures (sharp softmaxes)
    logits move 5e-2 to 6e-2 from the unquantised model and 78-95 % of the arg-maxes survive (profiles/fp8_kv.md); the cost on a real
    checkpoint is not known. A last-bit difference in one k can flip a code, so two different evaluation orders of the same prompt
    (one prefill / prefill + decode, other prefill chunkings) agree only to ~1e-3: cross-turn ``reuse_cache=True`` is NOT claimed to
    reproduce the ids of a fresh prefill under this mode. ``past_key_values`` are dequantised fp32 copies. Independent of
    ``weight_format``
  * ``weight_residency="tiles"`` (opt-in; or ``SX_LLM_WEIGHT_RESIDENCY=tiles``; needs a ``weight_format``): the quantised decode tiles are
    the ONLY copy of the seven projections. By default a quantised model still keeps every projection as a row-major 16-bit matrix of
    the dequantised values (25.7 GB at 13B dims) that only prefill reads; in this mode ``_pack`` frees each layer's matrices once its
    tiles are built (peak load-time memory: one layer), and prefill rebuilds one projection at a time into one shared scratch buffer
    (the largest per-rank projection, gate|up: 283 MB at 13B) with sx_dequant_tiles in front of the unchanged GEMM — the same bits as
    the default residency, prefill and decode. The decode step never touches the scratch buffer. CHOOSING: the mode buys the memory
    (more KV slots / a longer ``max_cache_len`` beside the other models, or a smaller part) and pays one extra pass over the layer's
    weights per prefill pass (0.53 / 1.03 B read + 2 B written per weight). Measured at 13B dims (profiles/weight_residency.md): 25.1 GB
    less held; + 4.3 .. 8.2 ms per pass, which is + 5 % of a 2048-row prefill (150 ms) but + 31 .. 35 % of the 8-row suffix prefills
    (14.5 ms) that in-flight batching with prefix reuse lives on; the token step is unchanged.
  * ``kv_pages=N`` (opt-in, exact; ``kv_page_size`` 32 / 64 / 128 rows, default 64; precise mode, head_dim 128, single rank): the paged KV
    cache — per layer ONE pool of N pages [N + 1][heads][page size][128] (k fp32, v fp32 or 16-bit under ``kv_v16``) shared by every
    slot, instead of ``max_cache_len`` rows per slot, and one int32 page table [max_batch][ceil(max_cache_len / page size)] for all
    layers (the same page index names a slot's rows in every layer's pool). ``max_cache_len`` stays the per-slot ceiling (table width,
    RoPE tables, split arithmetic); it no longer sizes the cache. Page 0 is the NULL page: all zeros, never handed out, never written;
    a table entry without a reservation names it, so reads of rows nobody owns hit finite zeros and an append there writes nothing.
    ``kv_reserve(seq, n_rows)`` extends a sequence's pages (paging.PagePool: LIFO free list, deterministic), ``kv_release(seq)``,
    ``reset`` and ``park_slots`` give them back; the host writes table rows only OUTSIDE captured graphs, and the captured token step
    reads the table from device memory at replay. Only the ADDRESS of a key row changes: a paged model computes, bit for bit, what
    the contiguous model computes (tests/test_kv_paged_gpu.py: torch.equal). Prefill and chunk passes reserve what they append;
    whoever drives ``decode_step`` directly reserves the rows its steps will write (the generate* engines reserve prompt +
    ``max_new_tokens`` up front). ``past_key_values`` are gathered copies. Follow-ups, refused with a ValueError today: the paged FP8
    cache (``kv_format``: paged row scales), the verify step of speculative decoding (``spec_tokens``: the verify kernel reads the
    contiguous cache), prefix reuse (``agent.prefix_cache``: sharing pages by reference in place of sx_kv_fork copies),
    tensor-parallel ranks, and preemption or swapping of a live request. Cost and the choice of 64 rows: profiles/kv_paged.md
  * ``comm`` with world > 1: Megatron tensor parallelism (parallel.py) — this rank owns nh/tp heads (their q/k/v rows, KV
    cache and o_proj columns), I/tp FFN rows (gate/up rows, down_proj columns) and Vpad/tp lm_head rows; the fp32
    residual stream is all-reduced after o_proj and down_proj (rank 0's GEMM epilogue adds the residual), the logits are
    all-gathered in front of the replicated greedy rule, so every rank holds identical tokens and loop state
"""
import logging
import math
import os

import torch

from . import ops
from .lora import split_peft_state_dict
from .parallel import Comm, llama_tp_shard
from .projection import Projection, glu_pack_rows  # noqa: F401  (glu_pack_rows: imported from here by tests and tools)


def merge_peft_lora(sd, lora_alpha=32, adapter="default"):
    """A PeftModel (LoRA) checkpoint of the LLM → the plain LlamaForCausalLM state dict, merged at load time — the optional
    configs/clm_models/llm_seed_x_lora.yaml route (peft.LoraConfig r 32, lora_alpha 32 on q/k/v/o/gate/up/down, modules_to_save = the
    norms): W' = W + (lora_B · lora_A) · lora_alpha / r, exactly peft's Linear.merge() / get_delta_weight()
    (proj/peft/src/peft/tuners/lora.py:779-806); `modules_to_save` copies replace the wrapped module's weight. The product is formed
    in fp32 and cast back to W's dtype. Keys without the `base_model.model.` prefix pass through unchanged."""
    out, lora, _, _ = split_peft_state_dict(sd, adapter)      # the parser shared with the unmerged serving path (lora.AdapterTables)
    for mod, ab in lora.items():
        if "A" not in ab or "B" not in ab:
            raise KeyError(f"merge_peft_lora: {mod} has only one of lora_A / lora_B")
        w = out[mod + ".weight"]
        r = ab["A"].shape[0]
        delta = (ab["B"].float() @ ab["A"].float()) * (float(lora_alpha) / r)
        out[mod + ".weight"] = (w.float() + delta.to(w.device)).to(w.dtype)
    return out


class LlamaConfigLite:
    def __init__(self, hidden_size, intermediate_size, num_hidden_layers, num_attention_heads, vocab_size,
                 rms_norm_eps=1e-5, max_position_embeddings=4096, rope_base=10000.0, **_):
        self.hidden_size, self.intermediate_size = hidden_size, intermediate_size
        self.num_hidden_layers, self.num_attention_heads = num_hidden_layers, num_attention_heads
        self.vocab_size, self.rms_norm_eps = vocab_size, rms_norm_eps
        self.max_position_embeddings, self.rope_base = max_position_embeddings, rope_base


class _Embedding:
    """Callable returned by get_input_embeddings(): ids → fp32 embeddings (seed_x.py:158)."""

    def __init__(self, owner):
        self.owner = owner

    def __call__(self, input_ids):
        ids = input_ids.to(device=self.owner.device, dtype=torch.int32).reshape(-1).contiguous()
        e = ops.embedding(ids, self.owner._P["embed"])
        return e.view(*input_ids.shape, -1)


class CausalLMOutputWithPast(dict):
    """Stand-in for transformers.modeling_outputs.CausalLMOutputWithPast (modeling_llama_xformer.py:740-746): fields by
    attribute (``out.logits``), by key (``out["logits"]``) or by position over the non-None fields (``out[0]``)."""

    def __getattr__(self, k):
        try:
            return dict.__getitem__(self, k)
        except KeyError:
            raise AttributeError(k) from None

    def __getitem__(self, k):
        if isinstance(k, (int, slice)):
            return self.to_tuple()[k]
        return dict.__getitem__(self, k)

    def to_tuple(self):
        return tuple(v for v in self.values() if v is not None)


class SlotState:
    """Device-side bookkeeping of the in-flight decode step (``decode_step(..., slots=...)``, sx_greedy_next_slots), one int32 entry
    per slot of the lock-step batch: ``live`` (a request occupies the slot), ``n_new`` (tokens generated so far), ``max_new`` (its
    budget), ``force_at`` (synthetic weights: index of the generated token replaced by ``force_id``, -1 = none) and ``status``
    [G, 4] = (next id, live, n_new, n_new at the finish or -1), the one tensor the host reads per token step. ``eos_id`` -1 = no
    EOS stop. A slot that is not live is PARKED: its counters in the module hold the idle values pos = -1, ctx = 0, step = -1, under
    which no kernel of the token step writes to its KV cache, id log or hidden-state log. ``logits`` is the [G, Vpad] tensor of
    the most recent step (the captured graph's own buffer under replay)."""
    IDLE = {"pos": -1, "ctx": 0, "step": -1}

    def __init__(self, G, device, force_id=-1, eos_id=-1, sampling=False):
        z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=device)
        self.G = G
        self.live, self.n_new, self.max_new, self.status = z(G), z(G), z(G), z(G, 4)
        self.force_at = torch.full((G,), -1, dtype=torch.int32, device=device)
        self.force_id, self.eos_id = int(force_id), int(eos_id)
        self.logits = None
        self.sampling = SampleState(G, device) if sampling else None     # None: the greedy step (sx_greedy_next_slots)
        # int32 [G] adapter table slot per slot, beside pos / ctx / step (the module's P["lora"]["sel"], which the adapter step reads):
        # written at admission (LlamaForCausalLM.set_adapters), -1 for parked slots and slots without an adapter; None: max_adapters = 0
        self.adapter = None
        # a LogprobState (slot_state(logprobs=n_top)): the step ends in the LP tail and has graphs of its own. None: the step as ever
        self.logprobs = None
        # a ControlState (slot_state(controls=True)): the step ends in the controlled tail (sx_next_slots_ctl) and has graphs of its own
        self.controls = None
        # a GrammarState (slot_state(grammar=True)): the step ends in the constrained tail (sx_next_slots_fsm), graphs of its own again
        self.grammar = None
        # a SeqRuleState (slot_state(seq_rules=True)): the step ends in the sequence-rule tail (sx_next_slots_seq), graphs of its own
        self.seq_rules = None

    def key(self):
        return tuple(t.data_ptr() for t in (self.live, self.n_new, self.max_new, self.force_at, self.status)) \
            + (self.force_id, self.eos_id) + (self.sampling.key() if self.sampling is not None else ()) \
            + (self.logprobs.key() if self.logprobs is not None else ()) + (self.controls.key() if self.controls is not None else ()) \
            + (self.grammar.key() if self.grammar is not None else ()) + (self.seq_rules.key() if self.seq_rules is not None else ())


class SampleState:
    """Per-row sampling parameters of the token step on the device (sx_sample_args; seedx_amd.sampling states the rule): ``do_sample`` /
    ``top_k`` int32 [G], ``temperature`` / ``top_p`` fp32 [G], ``seed`` int32 [G, 2] (low word, high word). The kernels read them at
    launch, so a captured step serves any mix of greedy and sampled rows and a row's parameters change without a new capture. A fresh
    state is all greedy. ``n_kept`` / ``p_chosen``: what the most recent launch reported per row (-1 / 1.0 where nothing was drawn)."""

    def __init__(self, G, device):
        self.G, self.device = int(G), device
        self.do_sample = torch.zeros(G, dtype=torch.int32, device=device)
        self.temperature = torch.ones(G, dtype=torch.float32, device=device)
        self.top_k = torch.zeros(G, dtype=torch.int32, device=device)
        self.top_p = torch.ones(G, dtype=torch.float32, device=device)
        self.seed = torch.zeros((G, 2), dtype=torch.int32, device=device)
        self.n_kept = torch.full((G,), -1, dtype=torch.int32, device=device)
        self.p_chosen = torch.ones(G, dtype=torch.float32, device=device)
        # speculative decoding: (a SampleState of G*T rows, T) that holds slot g's parameters in its rows g*T .. g*T + T - 1 — what
        # the candidates of a verify step are drawn with; set_rows keeps it in step. None: no verify step
        self.rows = None

    def key(self):
        return tuple(t.data_ptr() for t in (self.do_sample, self.temperature, self.top_k, self.top_p, self.seed, self.n_kept,
                                            self.p_chosen)) + (self.rows[0].key() if self.rows is not None else ())

    def set_rows(self, rows, params):
        """rows[i] takes params[i] (a sampling.SamplingParams, or None = greedy): five small host → device copies."""
        rows = list(rows)
        if not rows:
            return
        on = [p is not None and p.do_sample for p in params]
        idx = torch.tensor(rows, dtype=torch.int64, device=self.device)
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=self.device)
        f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=self.device)
        s32 = lambda w: w - (1 << 32) if w >= 1 << 31 else w          # the 32-bit pattern as an int32
        self.do_sample.index_copy_(0, idx, i32([int(o) for o in on]))
        self.temperature.index_copy_(0, idx, f32([p.temperature if o else 1.0 for p, o in zip(params, on)]))
        self.top_k.index_copy_(0, idx, i32([p.top_k if o else 0 for p, o in zip(params, on)]))
        self.top_p.index_copy_(0, idx, f32([p.top_p if o else 1.0 for p, o in zip(params, on)]))
        self.seed.index_copy_(0, idx, i32([[s32(p.seed & 0xffffffff), s32(p.seed >> 32)] if o else [0, 0] for p, o in zip(params, on)]))
        if self.rows is not None:
            st, T = self.rows
            st.set_rows([g * T + t for g in rows for t in range(T)], [p for p in params for _ in range(T)])

    def gather(self, rows):
        """A state of len(rows) rows holding copies of the given rows' parameters (the first token of admitted requests)."""
        out = SampleState(len(rows), self.device)
        idx = torch.tensor(list(rows), dtype=torch.int64, device=self.device)
        for k in ("do_sample", "temperature", "top_k", "top_p", "seed"):
            getattr(out, k).copy_(getattr(self, k).index_select(0, idx))
        return out


class LogprobState:
    """Where the LP tail of the token step records (sx_logprob_args; seedx_amd.sampling.token_logprobs states the rule): ``want`` int32
    [G] (0: the row records nothing) and, per row and token index, ``chosen`` fp32 [G, rows] — the log-probability of the emitted id —
    and ``top_ids`` int32 / ``top`` fp32 [G, rows, n_top], the n_top most likely ids of the raw row. ``rows`` is out_ids' row capacity;
    ``bind`` (re)allocates the three buffers for it, NaN / -1 filled. The pointers are part of the captured graph's key."""

    def __init__(self, G, n_top, device, rows=None):
        if isinstance(n_top, bool) or not 0 <= int(n_top) <= 8:
            raise ValueError(f"LogprobState: n_top must be an int in 0 .. 8, got {n_top!r}")
        self.G, self.n_top, self.device = int(G), int(n_top), device
        self.want = torch.zeros(self.G, dtype=torch.int32, device=device)
        self.chosen = self.top_ids = self.top = None
        if rows is not None:
            self.bind(rows)

    def bind(self, rows):
        if self.chosen is None or self.chosen.shape[1] != int(rows):
            self.chosen = torch.full((self.G, int(rows)), float("nan"), dtype=torch.float32, device=self.device)
            self.top_ids = torch.full((self.G, int(rows), self.n_top), -1, dtype=torch.int32, device=self.device)
            self.top = torch.full((self.G, int(rows), self.n_top), float("nan"), dtype=torch.float32, device=self.device)
        return self

    def key(self):
        return ("lp", self.n_top) + tuple(t.data_ptr() for t in (self.want, self.chosen, self.top_ids, self.top))

    def forced(self, g, start, n):
        """Rows [start, start + n) of sequence g hold ids the host forced (an image chunk): NaN / -1, the model did not choose."""
        self.chosen[g, start:start + n] = float("nan")
        self.top_ids[g, start:start + n] = -1
        self.top[g, start:start + n] = float("nan")


class ControlState:
    """Per-row logits controls of the token step on the device (sx_logits_ctl_args; seedx_amd.sampling.apply_controls states the rule):
    ``on`` int32 [G] (0: the row runs as without controls), ``counts`` int32 [G, ld] (bit 30: the id occurs in the prompt; low 24 bits:
    times generated — the tail counts every id a controlled row emits), ``work`` fp32 [G, ld] (the edited rows; the logits rows
    themselves stay raw), ``rep`` / ``rep_inv`` / ``presence`` / ``frequency`` fp32 [G], ``min_new`` int32 [G], ``bias_ids`` int32 /
    ``bias`` fp32 [G, 16] (-1: empty). ``ld`` is the logits' row stride. The kernels read everything at launch, so one captured step
    serves any mix of controlled and uncontrolled rows; the pointers are part of the graph key. A fresh state has every row off."""
    N_BIAS = 16

    def __init__(self, G, V, ld, device):
        assert int(ld) >= int(V) >= 1
        self.G, self.V, self.ld, self.device = int(G), int(V), int(ld), device
        i32, f32 = torch.int32, torch.float32
        self.on = torch.zeros(G, dtype=i32, device=device)
        self.counts = torch.zeros((G, self.ld), dtype=i32, device=device)
        self.work = torch.zeros((G, self.ld), dtype=f32, device=device)
        self.rep = torch.ones(G, dtype=f32, device=device)
        self.rep_inv = torch.ones(G, dtype=f32, device=device)
        self.presence = torch.zeros(G, dtype=f32, device=device)
        self.frequency = torch.zeros(G, dtype=f32, device=device)
        self.min_new = torch.zeros(G, dtype=i32, device=device)
        self.bias_ids = torch.full((G, self.N_BIAS), -1, dtype=i32, device=device)
        self.bias = torch.zeros((G, self.N_BIAS), dtype=f32, device=device)

    def key(self):
        return ("ctl",) + tuple(t.data_ptr() for t in (self.on, self.counts, self.work, self.rep, self.rep_inv, self.presence,
                                                       self.frequency, self.min_new, self.bias_ids, self.bias))

    def set_rows(self, rows, params, prompt_ids=None):
        """rows[i] takes params[i] (a sampling.ControlParams, or None: the row runs without controls) and starts a request: its counts
        are zeroed and the ids of prompt_ids[i] (a sequence of ints; ids outside [0, V) — image placeholders — are skipped) marked."""
        rows = list(rows)
        if not rows:
            return
        idx = torch.tensor(rows, dtype=torch.int64, device=self.device)
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=self.device)
        f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=self.device)
        on = [p is not None for p in params]
        self.on.index_copy_(0, idx, i32([int(o) for o in on]))
        self.rep.index_copy_(0, idx, f32([p.repetition_penalty if o else 1.0 for p, o in zip(params, on)]))
        self.rep_inv.index_copy_(0, idx, f32([p.rep_inv if o else 1.0 for p, o in zip(params, on)]))
        self.presence.index_copy_(0, idx, f32([p.presence_penalty if o else 0.0 for p, o in zip(params, on)]))
        self.frequency.index_copy_(0, idx, f32([p.frequency_penalty if o else 0.0 for p, o in zip(params, on)]))
        self.min_new.index_copy_(0, idx, i32([p.min_new_tokens if o else 0 for p, o in zip(params, on)]))
        ids, bias = [], []
        for p, o in zip(params, on):
            ent = list(p.logit_bias) if o else []
            assert len(ent) <= self.N_BIAS and all(0 <= i < self.V for i, _ in ent), "logit_bias: at most 16 ids inside the vocabulary"
            ids.append([i for i, _ in ent] + [-1] * (self.N_BIAS - len(ent)))
            bias.append([b for _, b in ent] + [0.0] * (self.N_BIAS - len(ent)))
        self.bias_ids.index_copy_(0, idx, i32(ids))
        self.bias.index_copy_(0, idx, f32(bias))
        self.counts.index_fill_(0, idx, 0)
        for i, g in enumerate(rows):
            pid = [] if prompt_ids is None or prompt_ids[i] is None else [int(t) for t in prompt_ids[i]]
            pid = sorted({t for t in pid if 0 <= t < self.V})
            if on[i] and pid:
                self.counts[g].index_fill_(0, torch.tensor(pid, dtype=torch.int64, device=self.device), 1 << 30)

    def gather(self, rows):
        """A state of len(rows) rows holding copies of the given rows (parameters AND counts): what the first token of admitted
        requests, taken from the prefill logits, is chosen with. The copy's tail counts into the copy; ``count`` puts the id into the
        real table."""
        out = ControlState(len(rows), self.V, self.ld, self.device)
        idx = torch.tensor(list(rows), dtype=torch.int64, device=self.device)
        for k in ("on", "counts", "rep", "rep_inv", "presence", "frequency", "min_new", "bias_ids", "bias"):
            getattr(out, k).copy_(getattr(self, k).index_select(0, idx))
        return out

    def count(self, rows, ids):
        """counts[rows[i], ids[i]] += 1: ids the HOST emitted for controlled rows (the first token, a forced image block). Ids outside
        [0, V) leave no trace, as in the tail."""
        pairs = [(int(g), int(t)) for g, t in zip(rows, ids) if 0 <= int(t) < self.V]
        if pairs:
            g = torch.tensor([a for a, _ in pairs], dtype=torch.int64, device=self.device)
            t = torch.tensor([b for _, b in pairs], dtype=torch.int64, device=self.device)
            self.counts.index_put_((g, t), torch.ones(len(pairs), dtype=torch.int32, device=self.device), accumulate=True)


class GrammarState:
    """Per-row state of constrained decoding on the device (sx_token_fsm_args; seedx_amd.grammar states the rule): ``table`` int32 [G]
    (index of the row's grammar in the model's resident table, -1: unconstrained) and ``state`` int32 [G] (the automaton's state; the
    tail advances it on every id a constrained row emits, DONE = -2: the row runs unconstrained). ``trans`` / ``flags`` are the MODEL's
    tables (``llm.load_grammar`` writes them in place), so one captured step serves any mix of grammars; the pointers are part of the
    graph key. A fresh state has every row unconstrained."""

    def __init__(self, owner):
        T = owner._P["grammar"]
        self.owner, self.G, self.device = owner, owner.G, owner.device
        self.trans, self.flags = T["trans"], T["flags"]
        self.table = torch.full((self.G,), -1, dtype=torch.int32, device=self.device)
        self.state = torch.full((self.G,), -2, dtype=torch.int32, device=self.device)

    def key(self):
        return ("fsm",) + tuple(t.data_ptr() for t in (self.table, self.state, self.trans, self.flags))

    def set_rows(self, slots, names):
        """slots[i] starts a request under the resident grammar names[i] (None: unconstrained): its table index, and state 0. An
        unknown name is a ValueError, never an unconstrained row."""
        slots = list(slots)
        idx = [self.owner._grammar_index(n) for n in names]
        self.owner._slot_write(self.table, slots, idx)
        self.owner._slot_write(self.state, slots, [0 if i >= 0 else -2 for i in idx])

    def gather(self, rows):
        """A state of len(rows) rows holding copies of the given rows: what the first token of admitted requests, taken from the
        prefill logits, is chosen with. ``scatter`` puts the advanced states back."""
        out = GrammarState.__new__(GrammarState)
        out.owner, out.G, out.device, out.trans, out.flags = self.owner, len(rows), self.device, self.trans, self.flags
        idx = torch.tensor(list(rows), dtype=torch.int64, device=self.device)
        out.table, out.state = self.table.index_select(0, idx), self.state.index_select(0, idx)
        return out

    def scatter(self, rows, part):
        self.state.index_copy_(0, torch.tensor(list(rows), dtype=torch.int64, device=self.device), part.state)


class SeqRuleState:
    """Per-row sequence rules of the token step on the device (sx_seq_rule_args; seedx_amd.sampling states the rules: apply_no_repeat,
    stop_match): ``on`` int32 [G] (0: the row runs as without rules), ``ngram`` int32 [G] (no_repeat_ngram_size, 0: off), ``hist`` int32
    [G, ld_hist] (the request's prompt ids followed by every id it emitted; the tail appends), ``hist_len`` / ``prompt_len`` int32 [G],
    ``n_stop`` int32 [G], ``stop_len`` int32 [G, 4], ``stop_ids`` int32 [G, 4, 8] and ``matched`` int32 [G] (the stop sequence the
    generated ids end with, -1: none). ``ld_hist`` is at least the model's max_cache_len: no request holds more ids than cache rows.
    The kernels read everything at launch, so one captured step serves any mix of rows; the pointers are part of the graph key. The
    host keeps mirrors of ``ngram`` / ``n_stop`` / ``stop_len`` (``host_limits``: what ops checks without a device read). A fresh state
    has every row off."""

    def __init__(self, G, V, ld_hist, device):
        assert int(G) >= 1 and int(ld_hist) >= 1
        self.G, self.V, self.ld_hist, self.device = int(G), int(V), int(ld_hist), device
        z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=device)
        self.on, self.ngram, self.hist_len, self.prompt_len, self.n_stop = z(G), z(G), z(G), z(G), z(G)
        self.hist, self.stop_len, self.stop_ids = z(G, self.ld_hist), z(G, 4), z(G, 4, 8)
        self.matched = torch.full((self.G,), -1, dtype=torch.int32, device=device)
        self._ngram_h, self._n_stop_h, self._stop_len_h = [0] * self.G, [0] * self.G, [[0] * 4 for _ in range(self.G)]

    def key(self):
        return ("seq",) + tuple(t.data_ptr() for t in (self.on, self.ngram, self.hist, self.hist_len, self.prompt_len, self.n_stop,
                                                       self.stop_len, self.stop_ids, self.matched))

    def host_limits(self):
        return self._ngram_h, self._n_stop_h, self._stop_len_h

    def tensors(self):
        """What a warm-up or capture of the step rewrites (put back by the caller like the counters)."""
        return [self.hist_len, self.matched]             # (an id the step left past hist_len is never read)

    def set_rows(self, rows, params, prompt_ids=None):
        """rows[i] takes params[i] (a sampling.SeqParams, or None: the row runs without rules) and starts a request: its history is
        prompt_ids[i] (a sequence of ints, image placeholders included), hist_len = prompt_len = its length, matched = -1."""
        rows = list(rows)
        if not rows:
            return
        idx = torch.tensor(rows, dtype=torch.int64, device=self.device)
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=self.device)
        on = [p is not None for p in params]
        pids = [[int(t) for t in prompt_ids[i]] if o and prompt_ids is not None and prompt_ids[i] is not None else []
                for i, o in enumerate(on)]
        assert all(len(p) <= self.ld_hist for p in pids), "sequence rules: a prompt longer than the id history"
        ngram = [p.no_repeat_ngram_size if o else 0 for p, o in zip(params, on)]
        stops = [list(p.stop) if o else [] for p, o in zip(params, on)]
        assert all(0 <= n <= 8 for n in ngram) and all(len(s) <= 4 and all(1 <= len(q) <= 8 for q in s) for s in stops)
        slen = [[len(q) for q in s] + [0] * (4 - len(s)) for s in stops]
        sids = [[list(q) + [-1] * (8 - len(q)) for q in s] + [[-1] * 8] * (4 - len(s)) for s in stops]
        self.on.index_copy_(0, idx, i32([int(o) for o in on]))
        self.ngram.index_copy_(0, idx, i32(ngram))
        self.n_stop.index_copy_(0, idx, i32([len(s) for s in stops]))
        self.stop_len.index_copy_(0, idx, i32(slen))
        self.stop_ids.index_copy_(0, idx, i32(sids))
        self.hist_len.index_copy_(0, idx, i32([len(p) for p in pids]))
        self.prompt_len.index_copy_(0, idx, i32([len(p) for p in pids]))
        self.matched.index_fill_(0, idx, -1)
        for g, p, n, s, sl in zip(rows, pids, ngram, stops, slen):
            self._ngram_h[g], self._n_stop_h[g], self._stop_len_h[g] = n, len(s), sl
            if p:
                self.hist[g, :len(p)] = i32(p)

    def gather(self, rows):
        """A state of len(rows) rows holding copies of the given rows (parameters AND history): what the first token of admitted
        requests, taken from the prefill logits, is chosen with. The copy's tail appends to the copy; ``append`` puts the id into the
        real history."""
        rows = list(rows)
        out = SeqRuleState(len(rows), self.V, self.ld_hist, self.device)
        idx = torch.tensor(rows, dtype=torch.int64, device=self.device)
        for k in ("on", "ngram", "hist", "hist_len", "prompt_len", "n_stop", "stop_len", "stop_ids", "matched"):
            getattr(out, k).copy_(getattr(self, k).index_select(0, idx))
        out._ngram_h = [self._ngram_h[g] for g in rows]
        out._n_stop_h = [self._n_stop_h[g] for g in rows]
        out._stop_len_h = [list(self._stop_len_h[g]) for g in rows]
        return out

    def append(self, rows, ids):
        """rows[i] = (g, at): row g's history takes ids[i] (a list of ids) at position ``at`` — its length as the host knows it, prompt
        length + ids emitted so far — and hist_len[g] = at + len(ids[i]). For ids the HOST emitted for rows that carry rules (the first
        token of an admitted request, a forced image block): small writes, no device read."""
        for (g, at), new in zip(rows, ids):
            new = [int(t) for t in new][:max(0, self.ld_hist - int(at))]
            if new:
                self.hist[g, at:at + len(new)] = torch.tensor(new, dtype=torch.int32, device=self.device)
            self.hist_len[g] = int(at) + len(new)


class LlamaForCausalLM:
    KV_FORMATS =(None, "fp8_e4m3", "fp8_e4m3_emulated")
    WEIGHT_FORMATS = (None, "fp8_e4m3", "mxfp4")
    WEIGHT_RESIDENCIES = (None, "tiles")

    def __init__(self, config, max_cache_len=None, max_batch=1, comm=None, precise=None, kv_v16=None, weight_format=None, kv_format=None,
                 weight_residency=None, max_adapters=0, lora_rank=32, spec_tokens=0, kv_pages=0, kv_page_size=64, max_grammars=0,
                 grammar_states=256):
        self.config = config if not isinstance(config, dict) else LlamaConfigLite(**config)
        c = self.config
        self.H, self.nh, self.L = c.hidden_size, c.num_attention_heads, c.num_hidden_layers
        self.hd = self.H // self.nh
        self.I, self.V = c.intermediate_size, c.vocab_size
        self.comm = comm or Comm()
        tp = self.tp = self.comm.world
        self.Vpad = (self.V + 64 * tp - 1) // (64 * tp) * (64 * tp)   # 32330 → 32384: lm_head rows padded with zeros
        assert self.nh % tp == 0 and self.I % (16 * tp) == 0, f"tp={tp} does not divide heads {self.nh} / FFN {self.I}"
        self.nh_l, self.I_l, self.V_l = self.nh // tp, self.I // tp, self.Vpad // tp
        self.H_l = self.nh_l * self.hd
        self.Tmax = max_cache_len or c.max_position_embeddings
        self.G = int(max_batch)
        assert 1 <= self.G <= 32, "lock-step batch is limited to 32 sequences (two 16-row operand blocks of sx_gemv)"
        # fp32-grade activations (module docstring). Up to 16 sequences the skinny GEMM's two operand blocks are the hi and lo planes; 17..32
        # sequences (round 6) run four blocks per weight fragment ([2 planes][2 row blocks], gemm_skinny_kernel<.., MB = 4>): the weights
        # still stream once. SX_LLM_PRECISE32=0 keeps round 5's behaviour (plain 16-bit flow above 16 sequences, logged).
        if precise is None:
            want = os.environ.get("SX_LLM_PRECISE", "1") != "0"
            precise = want and (self.G <= 16 or os.environ.get("SX_LLM_PRECISE32", "1") != "0")
            if want and not precise:      # never a silent change of numerics
                logging.getLogger("seedx_amd").warning(
                    "LlamaForCausalLM(max_batch=%d): more than 16 lock-step sequences run the PLAIN 16-bit flow (one rounding per MFMA "
                    "operand, 16-bit KV cache: logits 2.0e-3 from the fp32 reference at 40 layers, asserted at 3e-3) instead of the precise "
                    "mode (1e-3 contract) because SX_LLM_PRECISE32=0.", self.G)
        self.precise = bool(precise)
        # precise mode's "mixed" KV cache (round 6): k fp32, v in the model's 16-bit dtype — three quarters of the fp32 cache's bytes
        # (the cache is a third of what a token step moves at 1.5k tokens of context). It costs parity where the round-5 mode had a
        # factor 35 to spare: 40-layer logits 2.9e-5 → 5.6e-4 prefill / 5.9e-4 decode in fp16 (profiles/r6_fulldepth.log; asserted at
        # 1e-3). Default: ON for fp16 models, OFF for bf16 (a bf16 v carries 8 mantissa bits: 2.3e-3 on the miniature decoder, outside the
        # contract) — decided in _pack once the dtype is known; ``kv_v16=False`` / ``SX_LLM_V16=0`` keep the all-fp32 cache.
        self._kv_v16_arg = kv_v16
        self.kv_v16 = False
        # weight-only FP8 of the decode step (quant.py; opt-in: ``weight_format="fp8_e4m3"`` or SX_LLM_WEIGHTS=fp8_e4m3): the seven projection
        # matrices of every layer are quantised to e4m3 codes with a power-of-two scale per row; the decode tiles hold the codes (half the
        # bytes of a token step's weight stream), the row-major 16-bit weights hold their exact dequantised values. The 1e-3 contract
        # then holds against the QUANTISED model (bit-identical to the default mode loaded with the dequantised weights); against the
        # original checkpoint the mode costs the quantisation itself (2.7 % per projection on Gaussian rows, llm.weight_quant_report).
        # ``weight_format="mxfp4"`` (SX_LLM_WEIGHTS=mxfp4) is the same contract at four bits: OCP MXFP4 codes (e2m1, two per byte) with one
        # power-of-two E8M0 scale per 32-k block — 0.53 B per weight in the decode tiles, 11.4 % per projection on Gaussian rows
        # (round to nearest, no calibration); same requirements and refusals.
        if weight_format is None:
            weight_format = os.environ.get("SX_LLM_WEIGHTS") or None
        if weight_format not in self.WEIGHT_FORMATS:
            raise ValueError(f"LlamaForCausalLM: weight_format must be None, 'fp8_e4m3' or 'mxfp4', not {weight_format!r}")
        self.weight_format = weight_format
        self.weight_quant_report = None
        if weight_format is not None:
            # only where the raw matrices ARE the decode tiles: the precise mode's RMSNorm fold keeps gamma on the activation side; the
            # plain flow folds gamma into its tiles, which would be a second, different quantisation of the same weights
            if not self.precise:
                raise ValueError(f"LlamaForCausalLM: weight_format={weight_format!r} needs the precise mode (the plain 16-bit flow folds the RMSNorm "
                                 "gamma into its decode tiles: those are not the checkpoint's matrices and would be quantised a second, different time)")
            self._need_tiled_precise(f"weight_format={weight_format!r}", "FP8 / MXFP4 tiles exist for the MFMA skinny GEMM only")
        # residency of the quantised projections (module docstring; opt-in: ``weight_residency="tiles"`` or SX_LLM_WEIGHT_RESIDENCY=tiles):
        # None keeps the row-major 16-bit copy of the dequantised values for prefill, "tiles" holds the decode tiles alone
        if weight_residency is None:
            weight_residency = os.environ.get("SX_LLM_WEIGHT_RESIDENCY") or None
        if weight_residency not in self.WEIGHT_RESIDENCIES:
            raise ValueError(f"LlamaForCausalLM: weight_residency must be None or 'tiles', not {weight_residency!r}")
        if weight_residency is not None and weight_format is None:
            raise ValueError(f"LlamaForCausalLM: weight_residency={weight_residency!r} needs a weight_format ('fp8_e4m3' or 'mxfp4'): only "
                             "quantised decode tiles can stand in for the row-major 16-bit matrices")
        self.weight_residency = weight_residency
        # FP8 (e4m3) KV cache (module docstring; opt-in: ``kv_format="fp8_e4m3"`` or SX_LLM_KV=fp8_e4m3). Never a silent fall-back: a
        # configuration the FP8 kernels do not cover is refused here, like weight_format
        if kv_format is None:
            kv_format = os.environ.get("SX_LLM_KV") or None
        if kv_format not in self.KV_FORMATS:
            raise ValueError(f"LlamaForCausalLM: kv_format must be None, 'fp8_e4m3' or 'fp8_e4m3_emulated', not {kv_format!r}")
        self.kv_format = kv_format
        if kv_format is not None:
            if not self.precise:
                raise ValueError(f"LlamaForCausalLM: kv_format={kv_format!r} needs the precise mode (the FP8 cache is read by the fp32 attention "
                                 "kernels; the plain 16-bit flow's cache has no FP8 form)")
            if self.hd != 128:
                raise ValueError(f"LlamaForCausalLM: kv_format={kv_format!r} needs head_dim 128, not {self.hd} (one 16-lane group quantises a row)")
            if kv_v16:
                raise ValueError(f"LlamaForCausalLM: kv_v16=True and kv_format={kv_format!r} exclude each other (the FP8 cache holds k AND v "
                                 "as codes; its fp32 twin holds both in fp32)")
            if tp > 1:
                raise NotImplementedError("kv_format is single-rank: tensor-parallel ranks are not supported")
        # Decode attention (tools/bench_decode_attention_ab.py, 16 sequences x 40 heads, ms per token of the graph-replayed step):
        # three launches (RoPE + append, split-KV attention, combine) with 8 / 2 / 1 KV splits 6.70 / 6.46 / 6.52; ONE launch
        # (sx_attn_decode_fused, bit-identical) with 8 splits 6.80 — its arrival-counter tail costs more than two graph
        # launches — but with ONE split per head it needs no partials, counter or second pass at all. So: G x heads >= 512
        # workgroups without splitting → fused, 1 split; fewer → three launches with just enough splits for ~1024 workgroups.
        # Both from the GLOBAL head count: tensor-parallel ranks split exactly like one rank (bit-identical per head).
        self.fused_decode_attention = self.G * self.nh >= 512
        self.decode_nsplit = 1 if self.fused_decode_attention else min(8, max(1, -(-1024 // (self.G * self.nh))))
        # precise mode's fp32 decode attention: one workgroup per (head, sequence) walks ALL keys — 4 sequences x 40 heads are 160
        # workgroups of 94 dependent iterations at 1.5k keys (BASELINE config 5: 4 of the token step's 11 ms). Below 512 workgroups the keys
        # of a head are spread over enough splits for ~1024 (+ a combine launch); from the GLOBAL head count, like decode_nsplit.
        self.decode_nsplit_f32 = 1 if self.G * self.nh >= 512 else min(16, max(1, -(-1024 // (self.G * self.nh))))
        # unmerged per-request LoRA adapters (lora.py; opt-in: ``max_adapters`` > 0 preallocates that many table slots of rank
        # ``lora_rank``): the base weights stay as they are — any weight_format / weight_residency / kv_format — and every row of a prefill
        # pass or of the token step may use one of the resident adapters or none. 0: nothing is allocated, the feature is off. Never a
        # fall-back: a configuration the adapter kernels do not cover is refused here
        self.max_adapters, self.lora_rank = int(max_adapters), int(lora_rank)
        if self.max_adapters < 0:
            raise ValueError(f"LlamaForCausalLM: max_adapters={max_adapters} must be >= 0")
        if self.max_adapters:
            if tp > 1:
                raise ValueError("LlamaForCausalLM: max_adapters needs a single rank (the o / down adapters of tensor-parallel ranks are not built)")
            if not self.precise:
                raise ValueError("LlamaForCausalLM: max_adapters needs the precise mode (the adapter kernels read the two-plane operands; the plain "
                                 "16-bit flow has no adapter step)")
            self._need_tiled_precise("max_adapters", "the pre-activation addend exists on the MFMA skinny GEMM only")
            if self.lora_rank < 8 or self.lora_rank % 8 or 3 * self.lora_rank > 512:
                raise ValueError(f"LlamaForCausalLM: lora_rank={lora_rank} must be a multiple of 8 in 8 .. 168")
        # constrained decoding (grammar.py; opt-in: ``max_grammars`` > 0 preallocates that many token automata of up to ``grammar_states``
        # states, int16 [max_grammars][grammar_states][Vpad] + flags): only the tail of the token step changes, so every weight_format,
        # weight_residency, kv_format, kv_pages, adapter, sampling, logprob and control setting keeps working. 0: nothing is allocated,
        # nothing is launched differently
        self.max_grammars, self.grammar_states = int(max_grammars), int(grammar_states)
        self._grammars = {}
        if self.max_grammars < 0:
            raise ValueError(f"LlamaForCausalLM: max_grammars={max_grammars} must be >= 0")
        if self.max_grammars and not 2 <= self.grammar_states <= 32767:
            raise ValueError(f"LlamaForCausalLM: grammar_states={grammar_states} must be in 2 .. 32767 (next states are int16)")
        # lossless speculative decoding (spec.py; opt-in: ``spec_tokens=K`` drafted tokens per sequence and step): the verify step
        # (``decode_step(..., slots=st, spec=True)``) carries K + 1 rows per slot through the skinny GEMMs — the weights stream once
        # whatever the row count — and keeps the longest prefix the model itself would have produced (sx_spec_accept). 0: nothing is
        # allocated, nothing changes. Never a fall-back: what the verify kernels do not cover is refused here
        self.spec_tokens = int(spec_tokens)
        self.spec_ngram = (3, 1)         # (longest, shortest) n-gram of the prompt-lookup drafter (sx_spec_draft_ngram)
        if self.spec_tokens:
            K = self.spec_tokens
            if not 1 <= K <= 7:
                raise ValueError(f"LlamaForCausalLM: spec_tokens={spec_tokens} must be 0 (off) or 1 .. 7 (the verify attention holds 8 rows per sequence)")
            if not self.precise:
                raise ValueError("LlamaForCausalLM: spec_tokens needs the precise mode (the verify form exists for the fp32 decode attention only)")
            self._need_tiled_precise("spec_tokens", "the K + 1 rows per sequence ride on the MFMA skinny GEMM")
            if self.hd != 128:
                raise ValueError(f"LlamaForCausalLM: spec_tokens needs head_dim 128, not {self.hd} (the verify attention is the fused-RoPE form)")
            if tp > 1:
                raise ValueError("LlamaForCausalLM: spec_tokens needs a single rank (tensor-parallel ranks are not supported)")
            if self.G * (K + 1) > 32:
                raise ValueError(f"LlamaForCausalLM: max_batch {self.G} x (spec_tokens {K} + 1) = {self.G * (K + 1)} rows exceed the 32 rows of "
                                 "the skinny GEMM's operand tiles")
            if kv_format is not None:
                raise ValueError(f"LlamaForCausalLM: spec_tokens and kv_format={kv_format!r} exclude each other (the verify attention has no FP8 "
                                 "KV cache form)")
            if self.max_adapters:
                raise ValueError("LlamaForCausalLM: spec_tokens and max_adapters > 0 exclude each other (the adapter token step has no verify form)")
        # paged KV cache (module docstring; opt-in: ``kv_pages=N`` pages of ``kv_page_size`` rows shared by every slot). 0: nothing is
        # allocated and nothing is launched differently. Never a fall-back: what the paged kernels do not cover is refused here
        self.kv_pages, self.kv_page_size = int(kv_pages), int(kv_page_size)
        self._pool = None                # paging.PagePool, made by _pack
        if self.kv_pages < 0:
            raise ValueError(f"LlamaForCausalLM: kv_pages={kv_pages} must be >= 0 (0: the contiguous cache)")
        if self.kv_pages:
            from .paging import PAGE_SIZES
            if self.kv_page_size not in PAGE_SIZES:
                raise ValueError(f"LlamaForCausalLM: kv_page_size must be 32, 64 or 128 (powers of two and multiples of the MFMA prefill "
                                 f"kernel's 32-key tile, so no tile straddles a page), not {kv_page_size!r}")
            if not self.precise:
                raise ValueError("LlamaForCausalLM: kv_pages needs the precise mode (only the fp32 cache kernels read a page table; the plain "
                                 "16-bit flow's cache has no paged form)")
            if self.hd != 128:
                raise ValueError(f"LlamaForCausalLM: kv_pages needs head_dim 128, not {self.hd} (the paged kernels are the head_dim 128 forms)")
            if tp > 1:
                raise ValueError("LlamaForCausalLM: kv_pages needs a single rank (tensor-parallel ranks are a follow-up)")
            if kv_format is not None:
                raise ValueError(f"LlamaForCausalLM: kv_pages and kv_format={kv_format!r} exclude each other for now (follow-up: paged row "
                                 "scales for the FP8 cache)")
            if self.spec_tokens:
                raise ValueError("LlamaForCausalLM: kv_pages and spec_tokens > 0 exclude each other for now (follow-up: a page table in the "
                                 "verify kernel)")
        self._adapters = {}              # name -> table slot
        self._sel_host = [-1] * self.G   # host mirror of P["lora"]["sel"]: the adapter slot of every sequence, -1 = none
        self.device, self.dtype = None, torch.float16
        self._sd, self._P = None, None
        self._drop_graphs()
        self._sample_state = None
        self._control_state = None
        self._grammar_state = self._off_control_state = None
        self.kv_epoch = 0              # bumped whenever the KV cache is reset or written outside generate_batch

    def _kv_name(self):
        """The KV cache's format in words (log line and fit guard)."""
        if not self.precise:
            return "16-bit"
        if self.kv_format == "fp8_e4m3":
            return "FP8 e4m3 codes + fp32 row scales"
        if self.kv_format == "fp8_e4m3_emulated":
            return "fp32 holding FP8-e4m3-rounded rows (the reference twin)"
        return ("k fp32 + v 16-bit" if self.kv_v16 else "fp32") + \
            (f", paged: {self.kv_pages} pages of {self.kv_page_size} rows" if self.kv_pages else "")

    def _kv_kw(self, li, s=slice(None)):
        """What ops.rope_kv_append_f32 / attention_f32 take beyond the caches under ``kv_format``: layer li's row scales of the sequences
        ``s``, or the emulate flag. Paged cache: the page table rows of the sequences ``s`` (and the per-slot ceiling)."""
        if self.kv_pages:
            return {"paged": (self._P["ptab"][s], self.Tmax)}
        if self.kv_format == "fp8_e4m3":
            return {"kv_scales": (self._P["ks"][li][s], self._P["vs"][li][s])}
        if self.kv_format == "fp8_e4m3_emulated":
            return {"kv_emulate": True}
        return {}

    def _precise_tiled_ok(self):
        """Every projection shape of the precise decode step satisfies the MFMA skinny GEMM (_pack's P["precise_tiled"])."""
        return all(k % 64 == 0 and k >= 256 for k in (self.H, self.H_l, self.I_l)) and \
            all(n % 32 == 0 for n in (3 * self.H_l, self.H, 2 * self.I_l, self.V_l))

    def _skinny_shapes_ok(self):
        """precise_tiled and decode_tiled of _pack, from the dims alone (the attention output travels as operand tiles too)."""
        return self._precise_tiled_ok() and self.H_l % 32 == 0

    def _need_tiled_precise(self, what, why):
        """The one refusal of a feature that exists on the MFMA skinny GEMM only (weight_format, max_adapters, spec_tokens)."""
        if not self._skinny_shapes_ok():
            raise ValueError(f"LlamaForCausalLM: {what} needs the tiled precise decode path: hidden / per-rank head and FFN widths that are "
                             f"multiples of 64 and >= 256, output widths that are multiples of 32 (H {self.H}, heads x dim {self.H_l}, "
                             f"FFN {self.I_l}, vocab rows {self.V_l}): {why}")

    def _proj_shapes(self):
        """(N, K) of this rank's four projections."""
        return {"wqkv": (3 * self.H_l, self.H), "wo": (self.H, self.H_l), "wgu": (2 * self.I_l, self.H), "wd": (self.H, self.I_l)}

    def _has_tiles(self, N, K):
        """A weight of this shape gets decode tiles: the batch runs the MFMA skinny GEMM (G >= 5; precise mode: always) and the shape fits it."""
        return (self.G >= 5 or self.precise) and ops._mfma_shape(N, K)

    def _decode_tiled(self):
        """Every decode GEMV has its decode tiles, so its 16-bit inputs travel as operand tiles too (_pack's P["decode_tiled"])."""
        return all(self._has_tiles(N, K) for N, K in self._proj_shapes().values()) and self.H_l % 32 == 0

    def _bal20(self, n_rows):
        """o / down projections run from 20-row decode tiles where that gives 256 equal workgroups (N = 5120): the one rule for the
        16-bit tiles, the FP8 tiles and the workgroup count of the RMSNorm fold, which must agree on the layout (SX_GEMV_BAL20=0: A/B switch)."""
        return (self.G >= 5 or self.precise) and os.environ.get("SX_GEMV_BAL20", "1") != "0" and n_rows % 20 == 0 and n_rows // 20 == 256

    def _drop_graphs(self):
        """No captured token step: the lock-step one, the in-flight one (decode_step(..., slots=...): one per engine lifetime) and the
        sampled forms of the two (a greedy step and a sampled step never share a graph)."""
        self._graph = self._slot_graph = self._sample_graph = self._slot_sample_graph = None
        # the adapter token step (_layers_single_precise(adapters=True)) has four graphs of its own: it never shares one with the steps above
        self._graph_ad = self._slot_graph_ad = self._sample_graph_ad = self._slot_sample_graph_ad = None
        # the verify step of speculative decoding (decode_step(..., spec=True)): graphs of its own, greedy and sampled
        self._spec_graph = self._spec_sample_graph = None
        # a step that ends in the LP tail (a LogprobState) never shares a graph with the eight plain ones above
        for attr in ("_graph", "_slot_graph", "_sample_graph", "_slot_sample_graph"):
            setattr(self, attr + "_lp", None)
            setattr(self, attr + "_lp_ad", None)
            # ... and a step that ends in the controlled tail (a ControlState) has graphs of its own beside each of the sixteen
            for mid in ("", "_ad", "_lp", "_lp_ad"):
                setattr(self, attr + mid + "_ctl", None)
                setattr(self, attr + mid + "_fsm", None)       # ... and so has a step that ends in the constrained tail (a GrammarState)
                setattr(self, attr + mid + "_seq", None)       # ... and one that ends in the sequence-rule tail (a SeqRuleState),
                setattr(self, attr + mid + "_fsm_seq", None)   # without or with a grammar

    def memory_footprint(self):
        """Bytes this module will hold on its GPU once packed (per rank): 16-bit weights, their decode-tile copy (precise mode: always;
        plain flow: from 5 lock-step sequences), and the KV cache (fp32 in precise mode) — sized from ``max_cache_len``."""
        per_layer = (3 * self.H_l * self.H + self.H * self.H_l + 2 * self.I_l * self.H + self.H * self.I_l) * 2
        w = self.L * per_layer + (self.V + self.V_l) * self.H * 2
        tiles = self.L * per_layer + self.V_l * self.H * 2 if (self.G >= 5 or self.precise) else 0
        if self.weight_format == "fp8_e4m3":
            # one byte per weight + one fp32 scale per row, in exactly one layout per projection (o / down: 20-row OR 16-row tiles);
            # lm_head's tiles stay 16-bit. "weights" is unchanged: the row-major matrices hold the dequantised values for prefill
            rows = 3 * self.H_l + self.H + 2 * self.I_l + self.H
            tiles = self.L * (per_layer // 2 + rows * 4) + self.V_l * self.H * 2
        if self.weight_format == "mxfp4":
            # half a byte per weight + one E8M0 byte per 32 weights, one layout per projection; lm_head's tiles stay 16-bit
            tiles = self.L * (per_layer // 4 + per_layer // 64) + self.V_l * self.H * 2
        kv = self.L * self.G * self.nh_l * self.Tmax * self.hd * ((4 + (2 if self.kv_v16 else 4)) if self.precise else 4)
        if self.kv_pages:                       # the pool (null page included), whatever max_batch x max_cache_len would come to
            kv = self.L * (self.kv_pages + 1) * self.nh_l * self.kv_page_size * self.hd * (4 + (2 if self.kv_v16 else 4))
        if self.kv_format == "fp8_e4m3":        # one byte per k and per v value + the two fp32 row scales (the emulated twin: all fp32, above)
            kv = self.L * self.G * self.nh_l * self.Tmax * (2 * self.hd + 8)
        # adapter tables (max_adapters slots): A and B of the seven projections in 16 bits, the three norms' gammas and the scale in fp32
        ad = {"adapters": self.max_adapters * self._adapter_slot_bytes()} if self.max_adapters else {}
        if self.spec_tokens:                    # the verify step's own buffers (_pack: P["spec"])
            ad["spec_decode"] = self._spec_bytes()
        if self.max_grammars:                   # the resident token automata: int16 next states over the padded vocabulary + int32 flags
            ad["grammars"] = self.max_grammars * self.grammar_states * (self.Vpad * 2 + 4)
        if self.weight_residency == "tiles":
            # no row-major projection is held: embedding + lm_head + the one prefill scratch buffer (the largest per-rank projection)
            scratch = self._scratch_elems() * 2
            w = (self.V + self.V_l) * self.H * 2 + scratch
            return {"weights": w, "prefill_scratch": scratch, "decode_tiles": tiles, "kv_cache": kv, **ad,
                    "total": w + tiles + kv + sum(ad.values())}
        return {"weights": w, "decode_tiles": tiles, "kv_cache": kv, **ad, "total": w + tiles + kv + sum(ad.values())}

    @property
    def kv_row_bytes(self):
        """Bytes the contiguous KV cache holds per token of one sequence, over every layer and head of this rank: memory_footprint()'s
        "kv_cache" = G * Tmax * kv_row_bytes (1.2 MB at 13B dims with the mixed cache). What a spilled prefix costs per row in the
        host tier of the prefix cache (kvstore.py). ``kv_v16`` is settled when the weights are packed: read it after ``_pack()``."""
        if self.kv_format == "fp8_e4m3":
            return self.L * self.nh_l * (2 * self.hd + 8)
        return self.L * self.nh_l * self.hd * ((4 + (2 if self.kv_v16 else 4)) if self.precise else 4)

    def _adapter_slot_bytes(self):
        """Bytes of one adapter slot: R (K + N) 16-bit elements per projection (q, k, v, o: H x H; gate, up: I x H; down: H x I), the
        2 L + 1 fp32 gammas and the fp32 scale. 0.25 GB at 13B dims with R = 32."""
        return self.L * 2 * self.lora_rank * (8 * self.H + 3 * (self.H + self.I)) + (2 * self.L + 1) * self.H * 4 + 4

    def _spec_bytes(self):
        """Bytes of the verify step's own buffers: the id history, the row inputs / candidates / token indices, n_draft, the split-K
        workspace of G (K + 1) rows and the verify attention's partials."""
        R = self.G * (self.spec_tokens + 1)
        return (self.G * self.Tmax + 3 * R + self.G) * 4 + self._gemv_ws_bytes(R) + R * self.nh_l * self.decode_nsplit_f32 * (self.hd + 2) * 4

    def _gemv_ws_bytes(self, rows):
        """split-K scratch of the skinny GEMM for ``rows`` rows: counters + 8 partial [16, H] blocks per operand block
        (include/seedx_hip.h: sx_gemv_args.workspace)"""
        return 16384 + 8 * 16 * ((2 if self.precise else 1) * ((rows + 15) // 16)) * self.H * 4

    def _scratch_elems(self):
        """Elements of the tiles residency's prefill scratch buffer: max over the four per-rank projections of N * K (gate|up at 13B)."""
        return max(3 * self.H_l * self.H, self.H * self.H_l, 2 * self.I_l * self.H, self.H * self.I_l)

    # ---- reference-compatible plumbing ---------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, torch_dtype=torch.float16, low_cpu_mem_usage=True, peft_adapter=None, **kw):
        """HF directory (config.json + *.bin / *.safetensors shards), like llm_seed_x_i.yaml:1-3. ``peft_adapter``: optional PEFT LoRA
        adapter directory merged into the weights at load."""
        import glob
        import json
        import os
        cfg = json.load(open(os.path.join(pretrained_model_name_or_path, "config.json")))
        m = cls(LlamaConfigLite(**cfg), **kw)
        sd = {}
        for f in sorted(glob.glob(os.path.join(pretrained_model_name_or_path, "*.safetensors"))):
            from safetensors.torch import load_file
            sd.update(load_file(f))
        for f in sorted(glob.glob(os.path.join(pretrained_model_name_or_path, "pytorch_model*.bin"))):
            sd.update(torch.load(f, map_location="cpu"))
        lora_alpha = 32
        if peft_adapter is not None:
            # a PEFT adapter directory (adapter_config.json + adapter_model.safetensors | .bin), what PeftModel.from_pretrained(model_id)
            # reads in src/models/mllm/peft_models.py:106: merged into the base weights at load (merge_peft_lora)
            acfg = json.load(open(os.path.join(peft_adapter, "adapter_config.json")))
            lora_alpha = acfg.get("lora_alpha", 32)
            fs = os.path.join(peft_adapter, "adapter_model.safetensors")
            if os.path.exists(fs):
                from safetensors.torch import load_file
                ad = load_file(fs)
            else:
                ad = torch.load(os.path.join(peft_adapter, "adapter_model.bin"), map_location="cpu")
            # adapter files name the LoRA matrices `….lora_A.weight` (the adapter name is dropped on save)
            sd = {("base_model.model." + k if not k.startswith("base_model.model.") else k): v for k, v in sd.items()}
            sd.update(ad)
        m.load_state_dict(sd, lora_alpha=lora_alpha)
        m.dtype = torch_dtype
        return m

    def expected_keys(self):
        keys = ["model.embed_tokens.weight", "model.norm.weight", "lm_head.weight"]
        for i in range(self.L):
            p = f"model.layers.{i}."
            keys += [p + f"self_attn.{n}.weight" for n in ("q_proj", "k_proj", "v_proj", "o_proj")]
            keys += [p + f"mlp.{n}.weight" for n in ("gate_proj", "up_proj", "down_proj")]
            keys += [p + "input_layernorm.weight", p + "post_attention_layernorm.weight"]
        return keys

    def load_state_dict(self, sd, strict=True, lora_alpha=32):
        if any(".lora_A." in k for k in sd):                 # a PeftModel checkpoint (llm_seed_x_lora.yaml): merge the adapters at load
            sd = merge_peft_lora(sd, lora_alpha=lora_alpha)
        missing = [k for k in self.expected_keys() if k not in sd]
        if missing and strict:
            raise KeyError(f"LlamaForCausalLM: missing keys {missing[:6]} (+{max(0, len(missing) - 6)})")
        self._sd = sd
        self._P = None
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
        return self

    def eval(self):
        return self

    def get_input_embeddings(self):
        self._pack()
        return _Embedding(self)

    # ---- packing ---------------------------------------------------------------------------------------------------
    def _pack(self):
        if self._P is not None:
            return self._P
        if self._sd is None:
            raise RuntimeError("LlamaForCausalLM: load_state_dict() first")
        if self.device is None or self.device.type != "cuda":
            raise RuntimeError("LlamaForCausalLM runs on the GPU only")
        sd, dev, dt = self._sd, self.device, self.dtype
        want_v16 = self._kv_v16_arg if self._kv_v16_arg is not None else \
            (os.environ.get("SX_LLM_V16", "1") != "0" and dt == torch.float16)
        self.kv_v16 = bool(want_v16) and self.precise and self.hd <= 128 and self.hd % 8 == 0 and self.kv_format is None
        fp = self.memory_footprint()
        free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)   # + the allocator's cached blocks
        logging.getLogger("seedx_amd").info(
            "LlamaForCausalLM._pack (%s, %d sequences, Tmax %d): weights %.1f GB + decode tiles %.1f GB + KV cache %.1f GB (%s)",
            ("precise" if self.precise else "plain 16-bit") + ({"fp8_e4m3": ", FP8 e4m3 decode tiles", "mxfp4": ", MXFP4 decode tiles"}.get(self.weight_format, ""))
            + (", tiles residency: no row-major projections, prefill dequantises into a %.2f GB scratch buffer" % (fp["prefill_scratch"] / 1e9)
               if self.weight_residency == "tiles" else ""), self.G, self.Tmax,
            fp["weights"] / 1e9, fp["decode_tiles"] / 1e9,
            fp["kv_cache"] / 1e9, self._kv_name())
        if fp["total"] > free:
            raise RuntimeError(
                f"LlamaForCausalLM: {fp['total'] / 1e9:.1f} GB needed ({fp['weights'] / 1e9:.1f} weights + {fp['decode_tiles'] / 1e9:.1f} decode "
                f"tiles + {fp['kv_cache'] / 1e9:.1f} KV cache at max_cache_len {self.Tmax}, {self.G} sequences"
                f"{(', ' + self._kv_name() if self.kv_format else ', fp32 (precise mode)') if self.precise else ''}) but {free / 1e9:.1f} GB are free: lower max_cache_len / max_batch"
                + (", or pass precise=False (16-bit cache, no decode tiles below 5 sequences)" if self.precise else ""))
        if self.tp > 1:     # the captured decode step all-reduces [G, H] and all-gathers [G, Vpad/tp] fp32 (see _decode_step_body)
            self.comm.require_capacity(self.G * max(self.H, self.V_l))
        f32 = lambda t: t.detach().to(dev, torch.float32).contiguous()
        w16 = lambda t: t.detach().to(dev, dt).contiguous()
        P = {"embed": w16(sd["model.embed_tokens.weight"]), "norm": f32(sd["model.norm.weight"]), "layers": []}
        r, tp = self.comm.rank, self.tp
        v0, v1 = r * self.V_l, min((r + 1) * self.V_l, self.V)          # this rank's vocab rows (tail rows stay zero)
        lm = torch.zeros(self.V_l, self.H, dtype=dt, device=dev)
        if v1 > v0:
            lm[:v1 - v0] = sd["lm_head.weight"][v0:v1].detach().to(dev, dt)
        P["lm_head"] = lm
        # Second copy of a weight in the decode-tile layout for the lock-step batched decode (G >= 5 rows take the MFMA skinny GEMM, whose
        # wave-wide loads then cover whole contiguous kilobytes: 2.85 → 4.2 TB/s per layer in situ, tools/bench_gemv_layout.py). Costs
        # the weights' size again (25.7 GB of 288 GB at 13B); prefill keeps row-major. (precise mode: every lock-step batch size runs
        # the MFMA skinny GEMM, so the tiles exist from G = 1: 15.1 → 8 ms per token step at G = 4, BASELINE config 5)
        P["lm_head_t"] = ops.pack_decode_tiles(lm) if self._has_tiles(*lm.shape) else None
        P["decode_tiled"] = self._decode_tiled()        # every decode GEMV has its tiles → its 16-bit inputs travel as operand tiles too
        P["precise_tiled"] = self._precise_tiled_ok()   # precise step on the skinny GEMM (operand tiles, two planes): every shape fits its MFMA path
        # RMSNorm folded into the batched decode step (single rank, G >= 5; sx_gemv_args.x16_out / row_ssq_*): the decode tiles
        # of the projections that FOLLOW a norm carry that norm's gamma (W' = W · diag(gamma), product rounded once to 16 bits) —
        # wgu of every layer (post_attention_layernorm) and wqkv of layers >= 1 (input_layernorm; layer 0's input comes from the
        # embedding, not from a GEMV). Prefill keeps the row-major, unfolded weights and the norm kernel.
        # the consumer adds the producer's per-workgroup sums of squares 64 at a time: the o / down launches (N = H) must have a
        # multiple of 64 workgroups (H = 5120: 256 with 20-row tiles, 320 without)
        # (asked from the library, not re-derived here: sx_gemv's own workgroup count for an N = H launch in that weight layout)
        from . import _lib
        parts = _lib.load().sx_gemv_ssq_parts(self.H, 0, 2 if self._bal20(self.H) else 1)
        fold_ok = tp == 1 and parts % 64 == 0 and self.H % 32 == 0 and P["decode_tiled"] and os.environ.get("SX_RMS_FOLD", "1") != "0"
        P["rms_fold"] = fold_ok and self.G >= 5 and not self.precise       # (the precise mode norms in fp32 and folds in its own way:)
        # RMSNorm fold of the precise decode step (the plain fold's conditions): the residual GEMV writes the two planes of
        # x * gamma_next and the rows' sums of squares, the projection behind the norm scales by rstd. gamma sits on the ACTIVATION
        # here: the checkpoint's weights stay exact.
        P["rms_fold_precise"] = fold_ok and self.precise and P["precise_tiled"] and self.I_l % 32 == 0
        # tiled_step: the token step reads decode tiles (``tl`` of _layers_single / _layers_single_precise). Each projection is held in
        # exactly ONE tile layout: N = 5120 output rows are 320 16-row groups on 256 CUs; as 256 groups of 20 rows every CU streams the
        # same bytes (sx_gemv w_layout 2) — o and down at 13B dims where the step is tiled, 16-row tiles elsewhere, none where unread
        fmt, tiled_step = self.weight_format, P["decode_tiled"] and (P["precise_tiled"] or not self.precise)
        if fmt is not None:
            from . import quant
            qerr = {n.split(".")[1]: torch.zeros(2, dtype=torch.float64, device=dev) for n in quant.LLAMA_PROJECTIONS}   # [|W - Wq|^2, |W|^2]
        for i in range(self.L):
            p = f"model.layers.{i}."
            src, codes, scales = sd, None, None
            if fmt is not None:
                # the FULL matrices are quantised (after the LoRA merge, before the tensor-parallel slicing): every rank holds slices of
                # one quantised model. From here on "the weights" are the dequantised values; codes and scales are sliced the same way
                ql = quant.quantize_llama_layer(sd, p, dt, dev, weight_format=fmt)
                for k, (_, _, wq) in ql.items():
                    w0 = sd[k].detach().to(dev, dt).double()
                    qerr[k[len(p):].split(".")[1]] += torch.stack([(w0 - wq.double()).square().sum(), w0.square().sum()])
                cq, sq, src = ({k: v[j] for k, v in ql.items()} for j in range(3))
                if fmt == "mxfp4":     # packed codes and block scales: o / down are sliced along K in both
                    codes, scales = quant.llama_tp_shard_mxfp4(cq, sq, p, r, tp, self.nh, self.hd)
                else:
                    codes, scales = llama_tp_shard(cq, p, r, tp, self.nh, self.hd), quant.llama_tp_shard_scales(sq, p, r, tp, self.nh, self.hd)
                del ql, cq, sq
            sh = llama_tp_shard(src, p, r, tp, self.nh, self.hd)
            lw = dict(ln1=f32(sd[p + "input_layernorm.weight"]), ln2=f32(sd[p + "post_attention_layernorm.weight"]))
            for k, names in (("wqkv", ("q", "k", "v")), ("wo", ("o",)), ("wgu", ("up", "gate")), ("wd", ("down",))):
                N, K = self._proj_shapes()[k]
                pick = lambda d: None if d is None else [d[n] for n in names]
                gamma = {"wgu": lw["ln2"], "wqkv": lw["ln1"] if i > 0 else None}.get(k) if P["rms_fold"] else None
                lw[k] = Projection.build(pick(sh), dt, dev, glu=k == "wgu", format=fmt, codes=pick(codes), scales=pick(scales),
                                         tile_rows=20 if tiled_step and k in ("wo", "wd") and self._bal20(N) else 16,
                                         tiled=self._has_tiles(N, K) and (P["precise_tiled"] or not self.precise), tile_gamma=gamma,
                                         keep_matrix=self.weight_residency != "tiles")
            P["layers"].append(lw)
            del sh, src, codes, scales
        projections = [lw[k] for lw in P["layers"] for k in ("wqkv", "wo", "wgu", "wd")]
        held = sum(pj.nbytes_tiles for pj in projections) + (0 if P["lm_head_t"] is None else 2 * P["lm_head_t"].numel())
        # memory_footprint() prices what is held, nothing else, in every format (where the step is not tiled it prices the tiled one)
        assert held == fp["decode_tiles"] or not tiled_step, (held, fp["decode_tiles"])
        if fmt is not None:
            err = {k: math.sqrt(float(v[0] / v[1])) if float(v[1]) > 0 else 0.0 for k, v in qerr.items()}
            tiles16 = sum(2 * pj.shape.numel() for pj in projections) + 2 * P["lm_head_t"].numel()
            self.weight_quant_report = {"weight_format": fmt, "decode_tile_bytes": held, "decode_tile_bytes_16bit": tiles16,
                                        "rel_frobenius_error": err, "weight_residency": self.weight_residency}
            if self.weight_residency == "tiles":
                # ONE buffer for all four projections of every layer. Prefill runs on one stream: the GEMM on projection k finishes
                # before the dequantisation of projection k + 1 overwrites the buffer (_layers_multi). The decode step never reads it.
                P["w_scratch"] = torch.empty(self._scratch_elems(), dtype=dt, device=dev)
                rowmajor = P["embed"].numel() * 2 + P["lm_head"].numel() * 2 + P["w_scratch"].numel() * 2 + sum(pj.nbytes_rowmajor for pj in projections)
                assert rowmajor == fp["weights"] and P["w_scratch"].numel() * 2 == fp["prefill_scratch"], (rowmajor, fp)
            logging.getLogger("seedx_amd").info(
                "LlamaForCausalLM._pack: %s weight tiles, %.2f GB of decode tiles (16-bit: %.2f GB); relative Frobenius error of the "
                "quantisation against the %s checkpoint: %s", "MXFP4" if fmt == "mxfp4" else "FP8 e4m3", held / 1e9, tiles16 / 1e9,
                str(dt).replace("torch.", ""), ", ".join(f"{k} {v:.4f}" for k, v in err.items()))
        # split-K scratch of the skinny GEMM: counters + 8 partial [16, H] blocks (include/seedx_hip.h: sx_gemv_args.workspace)
        P["gemv_ws"] = torch.zeros(self._gemv_ws_bytes(self.G), dtype=torch.uint8, device=dev) if P["decode_tiled"] else None
        inv = 1.0 / (self.config.rope_base ** (torch.arange(0, self.hd, 2).float() / self.hd))
        fr = torch.outer(torch.arange(self.Tmax).float(), inv)           # [Tmax, hd/2] fp32 (:97-113)
        P["cos"], P["sin"] = fr.cos().to(dev).contiguous(), fr.sin().to(dev).contiguous()
        G = self.G
        if self.kv_format == "fp8_e4m3":
            # codes + one scale per (token, head) row, all zeros: a never-written row decodes to 0 · 0 and no code is NaN, so what the
            # in-flight step reads from parked slots stays finite
            P["kc"] = torch.zeros((self.L, G, self.nh_l, self.Tmax, self.hd), dtype=torch.uint8, device=dev)
            P["vc"] = torch.zeros_like(P["kc"])
            P["ks"] = torch.zeros((self.L, G, self.nh_l, self.Tmax), dtype=torch.float32, device=dev)
            P["vs"] = torch.zeros_like(P["ks"])
            held = sum(P[k].numel() * P[k].element_size() for k in ("kc", "vc", "ks", "vs"))
            assert held == fp["kv_cache"], (held, fp["kv_cache"])          # memory_footprint() prices what is held
        elif self.kv_pages:
            # the page pools, all zeros (page 0 stays so: the null page), and ONE page table for all layers; the table's pointer never
            # changes, its rows are written by kv_reserve / kv_release outside captured graphs
            from .paging import PagePool
            P["kc"] = torch.zeros((self.L, self.kv_pages + 1, self.nh_l, self.kv_page_size, self.hd), dtype=torch.float32, device=dev)
            P["vc"] = torch.zeros_like(P["kc"], dtype=dt) if self.kv_v16 else torch.zeros_like(P["kc"])
            self._pool = PagePool(self.kv_pages, self.kv_page_size, G, self.Tmax)
            P["ptab"] = torch.zeros((G, self._pool.width), dtype=torch.int32, device=dev)
            held = sum(P[k].numel() * P[k].element_size() for k in ("kc", "vc"))
            assert held == fp["kv_cache"], (held, fp["kv_cache"])          # memory_footprint() prices what is held
        else:
            P["kc"] = torch.zeros((self.L, G, self.nh_l, self.Tmax, self.hd), dtype=torch.float32 if self.precise else dt,
                                  device=dev)                                                      # this rank's heads
            P["vc"] = torch.zeros_like(P["kc"], dtype=dt) if self.kv_v16 else torch.zeros_like(P["kc"])
        # device-resident loop state, one entry per sequence
        P["pos"] = torch.zeros(G, dtype=torch.int32, device=dev)         # position of the next input token
        P["ctx"] = torch.ones(G, dtype=torch.int32, device=dev)          # pos + 1 (keys visible to that token)
        P["step"] = torch.zeros(G, dtype=torch.int32, device=dev)        # index into out_ids / hidden buffer
        P["cur"] = torch.zeros(G, dtype=torch.int32, device=dev)         # current input token id
        P["attn_cnt"] = torch.zeros(G * self.nh_l, dtype=torch.int32, device=dev)   # arrival counters of the fused decode attention
        P["attn_f32_part"] = torch.empty((G, self.nh_l, self.decode_nsplit_f32, self.hd + 2), dtype=torch.float32, device=dev) \
            if (self.precise and self.decode_nsplit_f32 > 1) else None
        if self.max_adapters:
            from . import lora
            nA, R, L, H, I = self.max_adapters, self.lora_rank, self.L, self.H, self.I
            z16 = lambda *shape: torch.zeros(shape, dtype=dt, device=dev)
            # [layer][adapter slot] tables; a free slot is all zero with the base gammas: it computes the base model
            T = {"A": {"qkv": z16(L, nA, 3 * R, H), "o": z16(L, nA, R, H), "gu": z16(L, nA, 2 * R, H), "d": z16(L, nA, R, I)},
                 "B": {"qkv": z16(L, nA, 3 * H, R), "o": z16(L, nA, H, R), "gu": z16(L, nA, 2 * I, R), "d": z16(L, nA, H, R)},
                 "ln1": torch.stack([lw["ln1"] for lw in P["layers"]])[:, None].repeat(1, nA, 1).contiguous(),
                 "ln2": torch.stack([lw["ln2"] for lw in P["layers"]])[:, None].repeat(1, nA, 1).contiguous(),
                 "norm": P["norm"][None].repeat(nA, 1).contiguous(),
                 "scale": torch.zeros(nA, dtype=torch.float32, device=dev),
                 "seg": {k: v.to(dev) for k, v in lora.seg_tables(H, I).items()},
                 "sel": torch.full((G,), -1, dtype=torch.int32, device=dev)}      # per-sequence adapter slot, beside pos / ctx / step
            held = sum(t.numel() * t.element_size() for d in (T["A"], T["B"]) for t in d.values()) \
                + sum(T[k].numel() * 4 for k in ("ln1", "ln2", "norm", "scale"))
            assert held == fp["adapters"], (held, fp["adapters"])                 # memory_footprint() prices what is held
            P["lora"] = T
            self._sel_host = [-1] * G
        if self.max_grammars:
            # a free table slot bans everything and accepts nothing; no row points at one (GrammarState.set_rows resolves names)
            T = {"trans": torch.full((self.max_grammars, self.grammar_states, self.Vpad), -1, dtype=torch.int16, device=dev),
                 "flags": torch.zeros((self.max_grammars, self.grammar_states), dtype=torch.int32, device=dev)}
            held = sum(t.numel() * t.element_size() for t in T.values())
            assert held == fp["grammars"], (held, fp["grammars"])                 # memory_footprint() prices what is held
            for a, f in self._grammars.values():                                  # a re-pack keeps the resident grammars
                trans, flags = f.table(self.grammar_states, self.Vpad)
                T["trans"][a].copy_(torch.from_numpy(trans))
                T["flags"][a].copy_(torch.from_numpy(flags))
            P["grammar"] = T
            self._grammar_state = None
        if self.spec_tokens:
            # the verify step's own buffers; the plain step keeps its workspace, scratch and graphs untouched
            R = G * (self.spec_tokens + 1)
            zi = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
            S = {"hist": zi(G, self.Tmax),                 # ids by cache position (prompt ids at admission, emitted ids by sx_spec_accept)
                 "rows": zi(R),                            # the step's row inputs: row g*T = cur, rows g*T + 1 .. = the draft
                 "cand": zi(R), "tok": zi(R),              # candidate id and token index (step[g] + t) of every row
                 "n_draft": zi(G),
                 "gemv_ws": torch.zeros(self._gemv_ws_bytes(R), dtype=torch.uint8, device=dev),
                 "attn_part": torch.empty((R, self.nh_l, self.decode_nsplit_f32, self.hd + 2), dtype=torch.float32, device=dev)}
            held = sum(t.numel() * t.element_size() for t in S.values())
            assert held == fp["spec_decode"], (held, fp["spec_decode"])           # memory_footprint() prices what is held
            S["sample"] = None                             # SampleState of R rows, made with the first sampled slot state
            P["spec"] = S
        self._P = P
        self._sd = None
        self._drop_graphs()
        return P

    # ---- resident grammars (grammar.py) ---------------------------------------------------------------------------------
    @property
    def grammars(self):
        """Names of the resident grammars."""
        return sorted(self._grammars)

    def _grammar_index(self, name):
        """Table slot of a request's grammar: None → -1 (unconstrained); an unknown name is an error, never an unconstrained row."""
        if name is None:
            return -1
        if not self.max_grammars:
            raise ValueError(f"LlamaForCausalLM: grammar {name!r} requested but the model was built with max_grammars=0")
        if name not in self._grammars:
            raise ValueError(f"LlamaForCausalLM: unknown grammar {name!r} (resident: {self.grammars})")
        return self._grammars[name][0]

    def grammar(self, name):
        """The grammar.TokenFSM resident under ``name`` (the engines walk it on the host for ``complete``)."""
        self._grammar_index(name)
        return self._grammars[name][1]

    def load_grammar(self, name, fsm):
        """Make a grammar.TokenFSM resident under ``name``: its table is written IN PLACE into a free slot of the model's table
        (allocated at pack time), so captured token steps stay valid. ValueError for a full table, a duplicate name, a grammar with
        more states than ``grammar_states`` or another vocabulary, or a model built with ``max_grammars=0``."""
        if not self.max_grammars:
            raise ValueError("LlamaForCausalLM.load_grammar: the model was built with max_grammars=0")
        if name in self._grammars:
            raise ValueError(f"LlamaForCausalLM.load_grammar: a grammar named {name!r} is resident already (unload_grammar first)")
        if len(self._grammars) >= self.max_grammars:
            raise ValueError(f"LlamaForCausalLM.load_grammar: all {self.max_grammars} grammar slots are in use ({self.grammars})")
        if fsm.n_states > self.grammar_states:
            raise ValueError(f"LlamaForCausalLM.load_grammar: grammar {name!r} has {fsm.n_states} states, the model was built with "
                             f"grammar_states={self.grammar_states}")
        if fsm.vocab_size != self.V:
            raise ValueError(f"LlamaForCausalLM.load_grammar: grammar {name!r} is over {fsm.vocab_size} ids, the model's vocabulary has {self.V}")
        T = self._pack()["grammar"]
        a = min(set(range(self.max_grammars)) - {i for i, _ in self._grammars.values()})
        trans, flags = fsm.table(self.grammar_states, self.Vpad)
        T["trans"][a].copy_(torch.from_numpy(trans))
        T["flags"][a].copy_(torch.from_numpy(flags))
        self._grammars[name] = (a, fsm)
        return a

    def unload_grammar(self, name):
        """Free ``name``'s table slot (it bans everything and accepts nothing again), in place."""
        a = self._grammar_index(name)
        if a < 0:
            raise ValueError("LlamaForCausalLM.unload_grammar: no grammar named")
        T = self._pack()["grammar"]
        T["trans"][a].fill_(-1)
        T["flags"][a].zero_()
        del self._grammars[name]

    def grammar_state(self, fresh=False):
        """A GrammarState over this model's table. The lock-step step's (``decode_step(..., grammar=...)``) is made once — its pointers
        are part of the captured graph's key; ``fresh``: a new one (a slot state owns its own)."""
        if not self.max_grammars:
            raise ValueError("LlamaForCausalLM.grammar_state: the model was built with max_grammars=0")
        self._pack()
        if fresh:
            return GrammarState(self)
        if getattr(self, "_grammar_state", None) is None:
            self._grammar_state = GrammarState(self)
        return self._grammar_state

    # ---- unmerged LoRA adapters (lora.py) ---------------------------------------------------------------------------------
    @property
    def adapters(self):
        """Names of the resident adapters."""
        return sorted(self._adapters)

    def _adapter_index(self, name):
        """Table slot of a request's adapter: None → -1 (the base model); an unknown name is an error, never the base model."""
        if name is None:
            return -1
        if not self.max_adapters:
            raise ValueError(f"LlamaForCausalLM: adapter {name!r} requested but the model was built with max_adapters=0")
        if name not in self._adapters:
            raise ValueError(f"LlamaForCausalLM: unknown adapter {name!r} (resident: {self.adapters})")
        return self._adapters[name]

    def load_adapter(self, name, source, lora_alpha=None):
        """Make a LoRA adapter resident under ``name``. ``source``: a PEFT directory (adapter_config.json + adapter_model.safetensors |
        .bin) or a state dict with lora_A / lora_B / modules_to_save keys (the key forms merge_peft_lora parses). The tables were
        allocated at pack time and are written IN PLACE: captured token steps stay valid and no other adapter is touched. Loading a
        resident name again replaces it. ValueError (never a partial load or a fall-back) for what lora.AdapterTables refuses, a full
        table, or a model built without ``max_adapters``."""
        from . import lora
        if not self.max_adapters:
            raise ValueError("LlamaForCausalLM.load_adapter: the model was built with max_adapters=0")
        if isinstance(source, (str, os.PathLike)):
            import json
            acfg = json.load(open(os.path.join(source, "adapter_config.json")))
            if lora_alpha is None:
                lora_alpha = acfg.get("lora_alpha", 32)
            fs = os.path.join(source, "adapter_model.safetensors")
            if os.path.exists(fs):
                from safetensors.torch import load_file
                source = load_file(fs)
            else:
                source = torch.load(os.path.join(source, "adapter_model.bin"), map_location="cpu")
        tab = lora.AdapterTables(source, self.L, self.H, self.I, R=self.lora_rank, lora_alpha=32 if lora_alpha is None else lora_alpha,
                                 dtype=self.dtype)
        if name in self._adapters and self._adapters[name] in self._sel_host:
            raise ValueError(f"LlamaForCausalLM.load_adapter: adapter {name!r} is in use by sequence(s) "
                             f"{[g for g, v in enumerate(self._sel_host) if v == self._adapters[name]]}: its tables cannot be replaced under them")
        if name not in self._adapters and len(self._adapters) >= self.max_adapters:
            raise ValueError(f"LlamaForCausalLM.load_adapter: all {self.max_adapters} adapter slots are in use ({self.adapters})")
        P = self._pack()
        T = P["lora"]
        a = self._adapters.get(name)
        if a is None:
            a = min(set(range(self.max_adapters)) - set(self._adapters.values()))
        for li in range(self.L):
            for k in ("qkv", "o", "gu", "d"):
                T["A"][k][li, a].copy_(tab.A[k][li])
                T["B"][k][li, a].copy_(tab.B[k][li])
            T["ln1"][li, a].copy_(tab.ln1[li] if tab.ln1[li] is not None else P["layers"][li]["ln1"])
            T["ln2"][li, a].copy_(tab.ln2[li] if tab.ln2[li] is not None else P["layers"][li]["ln2"])
        T["norm"][a].copy_(tab.norm if tab.norm is not None else P["norm"])
        T["scale"][a] = tab.scale
        self._adapters[name] = a
        return a

    def unload_adapter(self, name):
        """Free ``name``'s table slot: its tables go back to zero and its gammas to the base model's (a free slot computes the base
        model), in place. No sequence may be using it."""
        a = self._adapter_index(name)
        if a < 0:
            raise ValueError("LlamaForCausalLM.unload_adapter: no adapter named")
        users = [g for g, v in enumerate(self._sel_host) if v == a]
        if users:
            raise ValueError(f"LlamaForCausalLM.unload_adapter: adapter {name!r} is in use by sequence(s) {users}")
        P, T = self._pack(), self._P["lora"]
        for k in ("qkv", "o", "gu", "d"):
            T["A"][k][:, a].zero_()
            T["B"][k][:, a].zero_()
        for li in range(self.L):
            T["ln1"][li, a].copy_(P["layers"][li]["ln1"])
            T["ln2"][li, a].copy_(P["layers"][li]["ln2"])
        T["norm"][a].copy_(P["norm"])
        T["scale"][a] = 0.0
        del self._adapters[name]

    def set_adapters(self, seqs, names):
        """Sequence seqs[i] decodes under adapter names[i] (None = the base model) from now on: one small host → device copy into the
        per-sequence adapter index the token step reads (written at admission; a parked slot holds -1)."""
        idx = [self._adapter_index(n) for n in names]
        seqs = list(seqs)
        if not self.max_adapters:
            return
        P = self._pack()
        self._slot_write(P["lora"]["sel"], seqs, idx)
        for g, a in zip(seqs, idx):
            self._sel_host[g] = a

    # ---- paged KV cache (paging.py) -----------------------------------------------------------------------------------------
    @property
    def kv_pages_free(self):
        """Pages of the pool nobody holds (``kv_pages`` on a model that holds no sequence)."""
        if not self.kv_pages:
            raise ValueError("LlamaForCausalLM.kv_pages_free: the model was built with kv_pages=0 (the contiguous cache)")
        self._pack()
        return self._pool.free

    def kv_reserve(self, seq, n_rows):
        """Sequence ``seq`` may hold ``n_rows`` cache rows from now on: its page list is EXTENDED to cover them (idempotent; pages already
        held stay where they are) and its row of the device page table is rewritten — one small host → device copy, never inside a
        captured graph. False: the free pages do not cover it (or n_rows exceeds ``max_cache_len``) and nothing changed."""
        if not self.kv_pages:
            raise ValueError("LlamaForCausalLM.kv_reserve: the model was built with kv_pages=0 (the contiguous cache)")
        P = self._pack()
        had = len(self._pool.pages(seq))
        if not self._pool.reserve(seq, n_rows):
            return False
        if len(self._pool.pages(seq)) != had:
            P["ptab"][seq].copy_(torch.tensor(self._pool.table_row(seq), dtype=torch.int32))
        return True

    def kv_release(self, seq=None):
        """Gives the pages of sequence ``seq`` (None: of every sequence) back to the pool; its table row names the null page again."""
        if not self.kv_pages:
            raise ValueError("LlamaForCausalLM.kv_release: the model was built with kv_pages=0 (the contiguous cache)")
        P = self._pack()
        for g in (range(self.G) if seq is None else [seq]):
            if self._pool.release(g):
                P["ptab"][g].zero_()

    def _kv_need(self, seq, n_rows, what):
        """kv_reserve or a RuntimeError that names the shortfall."""
        if not self.kv_reserve(seq, n_rows):
            pool = self._pool
            raise RuntimeError(f"LlamaForCausalLM: {what}: sequence {seq} needs {n_rows} cache rows = {pool.need(seq, n_rows)} more pages of "
                               f"{pool.page_size} rows, but {pool.free} of the pool's {pool.n_pages} pages are free (per-slot ceiling "
                               f"max_cache_len = {self.Tmax} rows): build the model with more kv_pages or release a sequence")

    def _kv_gather(self, li, seq, n_rows):
        """Contiguous copies [heads, n_rows, hd] of layer li's k and v rows of sequence ``seq`` (plumbing: past_key_values, tests)."""
        P = self._P
        idx = torch.tensor(self._pool.table_row(seq), dtype=torch.int64, device=self.device)
        out = []
        for c in (P["kc"][li], P["vc"][li]):
            rows = c[idx].permute(1, 0, 2, 3).reshape(self.nh_l, -1, self.hd)      # [heads, width * page size, hd]
            out.append(rows[:, :n_rows].contiguous())
        return tuple(out)

    # ---- core passes ---------------------------------------------------------------------------------------------------
    def reset(self, seq=None):
        P = self._pack()
        self.kv_epoch += 1              # invalidates ContinuousLVLM's cross-turn prefix bookkeeping
        if self.kv_pages:
            self.kv_release(seq)
        s = slice(None) if seq is None else slice(seq, seq + 1)
        P["pos"][s] = 0
        P["step"][s] = 0
        P["ctx"][s] = 1                 # invariant: ctx == pos + 1 (keys visible to the token at `pos`)

    def _layers_multi(self, x, Ts, seqs, adapters=None):
        """Ts[i] tokens appended to sequence seqs[i] at its cache position (prefill of several prompts, or the forced
        image-token chunk of several sequences, as ONE pass): every GEMM runs on all sum(Ts) rows at once — the weights
        stream once per pass instead of once per sequence — while RoPE / KV append / causal flash attention stay per
        sequence (batched into single launches when all sequences share T and position). x: fp32 [sum(Ts), H] residual
        stream, rows ordered like seqs. Returns the final residual stream.
        ``adapters`` (table slots, one per sequence, -1 = none; None or all -1: the pass below is untouched): the rows of sequence i
        run under adapter adapters[i] — its gammas in the norms (sx_rmsnorm_planes_sel) and, per projection, the fp32 delta of
        sx_lora_shrink / sx_lora_expand on the row-major planes handed to the unchanged GEMM as ``bias2d`` (one row of it per output
        row), which its epilogue adds before activation / GLU / residual. Rows without an adapter carry a zero delta; each projection
        is one GEMM over all rows, so under weight_residency="tiles" it is dequantised once."""
        P, dt, H, nh, hd = self._P, self.dtype, self.H_l, self.nh_l, self.hd     # local heads under tensor parallelism
        comm, lead = self.comm, self.comm.rank == 0
        pr = self.precise
        n = len(seqs)
        # tiles residency: the tiles are the only copy of a projection: rebuild it (exactly: sx_dequant_tiles) into the shared scratch buffer
        # right in front of its GEMM. Everything here runs on ONE stream, so the GEMM on projection k has finished before the
        # dequantisation of projection k + 1 overwrites the buffer; nothing else reads it (the decode step runs from the tiles).
        wmat = lambda lw, k: lw[k].matrix(P.get("w_scratch"))
        pos_all = P["pos"].tolist()                                              # one host read per pass
        pos0 = [pos_all[g] for g in seqs]
        for T, p0 in zip(Ts, pos0):
            assert p0 + T <= self.Tmax, f"sequence {p0 + T} exceeds the KV cache ({self.Tmax})"
        if self.kv_pages:               # paged cache: the pass holds pages for every row it appends (a no-op where the caller reserved more)
            for g, T, p0 in zip(seqs, Ts, pos0):
                self._kv_need(g, p0 + T, f"a pass of {T} rows at position {p0}")
        uniform = n > 1 and len(set(Ts)) == 1 and len(set(pos0)) == 1 and list(seqs) == list(range(seqs[0], seqs[0] + n))
        offs = [0]
        for T in Ts:
            offs.append(offs[-1] + T)
        M = offs[-1]
        eps = self.config.rms_norm_eps
        scale = 1.0 / math.sqrt(hd)
        g0 = seqs[0]
        lo = None
        if adapters is not None and any(a >= 0 for a in adapters):
            assert pr and self.max_adapters and len(adapters) == n
            lo = P["lora"]
            sel = torch.repeat_interleave(torch.tensor(list(adapters), dtype=torch.int32), torch.tensor(Ts)).to(x.device)   # [M] rows → slot
            zbuf = {}

            def norm(xx, li, k):
                return ops.rmsnorm_planes_sel(xx, lw[k], lo[k][li], sel, eps, dt)[0]

            def delta(hp, li, k):
                """bias2d of projection k for the planes hp: zero for base rows (sx_lora_expand leaves them unwritten)."""
                t = ops.lora_shrink(hp, lo["A"][k][li], sel)
                N_ = lo["B"][k].shape[2]
                if N_ not in zbuf:          # zeroed ONCE per pass and width: the base rows are never written, the adapter rows always
                    zbuf[N_] = torch.zeros((M, N_), dtype=torch.float32, device=x.device)
                return dict(bias2d=ops.lora_expand(t, lo["B"][k][li], lo["seg"][k], lo["scale"], sel, out=zbuf[N_]), bias2d_rows=1)
        else:
            norm = lambda xx, li, k: ops.rmsnorm_planes(xx, lw[k], eps, dt)[0]
            delta = lambda hp, li, k: {}
        for li, lw in enumerate(P["layers"]):
            kc_l, vc_l = P["kc"][li], P["vc"][li]
            if pr:
                # fp32-grade activations: operand planes into a_planes = 2 GEMMs with fp32 outputs, fp32 RoPE / cache / attention
                h = norm(x, li, "ln1")
                qkv = ops.gemm(h, wmat(lw, "wqkv"), a_planes=2, out_dtype=torch.float32, **delta(h, li, "qkv"))    # [M, 3H] fp32
                # (kv_format: the append quantises; the emulated twin's attention is the plain fp32 call on its rounded rows)
                # paged cache: the caches are the layer's whole pools and the sequences' table rows ride in kw["paged"]
                cs = (lambda c, a, b: c) if self.kv_pages else (lambda c, a, b: c[a:b])
                akw = lambda kw: {k: kw[k] for k in ("kv_scales", "paged") if k in kw}   # (attention: the emulated twin is the plain call)
                if uniform:
                    kw = self._kv_kw(li, slice(g0, g0 + n))
                    ops.rope_kv_append_f32(qkv, cs(kc_l, g0, g0 + n), cs(vc_l, g0, g0 + n), P["cos"], P["sin"], P["pos"][g0:g0 + n], n, Ts[0],
                                           nh, hd, dt, **kw)
                    att = ops.attention_f32(qkv, cs(kc_l, g0, g0 + n), cs(vc_l, g0, g0 + n), P["pos"][g0:g0 + n], n, Ts[0], nh, hd, scale, dt,
                                            **akw(kw))
                else:
                    att = torch.empty((M, 2 * H), dtype=dt, device=x.device)
                    for i, g in enumerate(seqs):
                        rows = qkv[offs[i]:offs[i + 1]]
                        kw = self._kv_kw(li, slice(g, g + 1))
                        ops.rope_kv_append_f32(rows, cs(kc_l, g, g + 1), cs(vc_l, g, g + 1), P["cos"], P["sin"], P["pos"][g:g + 1], 1, Ts[i], nh,
                                               hd, dt, **kw)
                        att[offs[i]:offs[i + 1]] = ops.attention_f32(rows, cs(kc_l, g, g + 1), cs(vc_l, g, g + 1), P["pos"][g:g + 1], 1, Ts[i],
                                                                     nh, hd, scale, dt, **akw(kw))
                x = comm.all_reduce(ops.gemm(att, wmat(lw, "wo"), a_planes=2, residual=x if lead else None, out_dtype=torch.float32,
                                             **delta(att, li, "o")))
                h = norm(x, li, "ln2")
                g_ = ops.split16(ops.gemm(h, wmat(lw, "wgu"), a_planes=2, act="silu", glu=True, out_dtype=torch.float32,
                                          **delta(h, li, "gu")), dt)
                x = comm.all_reduce(ops.gemm(g_, wmat(lw, "wd"), a_planes=2, residual=x if lead else None, out_dtype=torch.float32,
                                             **delta(g_, li, "d")))
                continue
            h = ops.rmsnorm(x, lw["ln1"], eps, dt)
            qkv = ops.gemm(h, lw["wqkv"].w)                                           # [M, 3H]
            if uniform:
                T, Tk = Ts[0], pos0[0] + Ts[0]
                ops.rope_kv_append_b(qkv, kc_l[g0:g0 + n], vc_l[g0:g0 + n], P["cos"], P["sin"], P["pos"][g0:g0 + n], n, T,
                                     nh, hd)
                q4 = qkv.view(n, T, 3, nh, hd)[:, :, 0]
                k4 = kc_l[g0:g0 + n, :, :Tk].permute(0, 2, 1, 3)                      # [n, Tk, nh, hd] views of the caches
                v4 = vc_l[g0:g0 + n, :, :Tk].permute(0, 2, 1, 3)
                att = ops.attention(q4, k4, v4, scale, causal=True).view(M, H)
            else:
                att = torch.empty((M, H), dtype=dt, device=x.device)
                for i, g in enumerate(seqs):
                    T, Tk = Ts[i], pos0[i] + Ts[i]
                    rows = qkv[offs[i]:offs[i + 1]]
                    ops.rope_kv_append(rows, kc_l[g], vc_l[g], P["cos"], P["sin"], P["pos"][g:g + 1], nh, hd)
                    q4 = rows.view(1, T, 3, nh, hd)[:, :, 0]
                    k4 = kc_l[g][:, :Tk].permute(1, 0, 2).unsqueeze(0)                # [1, Tk, nh, hd] view of the cache
                    v4 = vc_l[g][:, :Tk].permute(1, 0, 2).unsqueeze(0)
                    ops.attention(q4, k4, v4, scale, causal=True, out=att[offs[i]:offs[i + 1]].view(1, T, H))
            x = comm.all_reduce(ops.gemm(att, lw["wo"].w, residual=x if lead else None, out_dtype=torch.float32))
            h = ops.rmsnorm(x, lw["ln2"], eps, dt)
            g_ = ops.gemm(h, lw["wgu"].w, act="silu", glu=True)                       # silu(gate) * up, [M, I/tp]
            x = comm.all_reduce(ops.gemm(g_, lw["wd"].w, residual=x if lead else None, out_dtype=torch.float32))
        if uniform:
            ops.add_i32(P["pos"][g0:g0 + n], Ts[0])
            ops.add_i32(P["ctx"][g0:g0 + n], Ts[0])
        else:
            for i, g in enumerate(seqs):
                ops.add_i32(P["pos"][g:g + 1], Ts[i])
                ops.add_i32(P["ctx"][g:g + 1], Ts[i])
        return x

    def _layers_single(self, x, slots=None):
        """One token of EVERY sequence (x: fp32 [G, H]) at the device-resident positions: weight-streaming GEMVs with
        M = G rows + split-KV decode attention per sequence. No host reads → graph-capturable. ``slots`` (in-flight batching): the
        positions are advanced per LIVE slot by sx_greedy_next_slots at the end of the step instead of unconditionally here."""
        P, dt, H, nh, hd, G = self._P, self.dtype, self.H_l, self.nh_l, self.hd, self.G
        comm, lead = self.comm, self.comm.rank == 0
        eps = self.config.rms_norm_eps
        scale = 1.0 / math.sqrt(hd)
        # G >= 5 sequences run the MFMA skinny GEMM: its 16-bit inputs then travel as operand tiles (ops.Tiled16) from the
        # kernel that produces them (norm, attention combine, GLU epilogue) — one contiguous 1-KB load per operand instead of
        # 16 rows that all sit on the same L2 channel — and the down projection may split K over workgroups (workspace)
        tl, ws = P["decode_tiled"] and G >= 5, P["gemv_ws"]
        if self.precise:
            return self._layers_single_precise(x, slots)
        # folded RMSNorm: the residual GEMVs (o, down) also emit the new residual stream as 16-bit operand tiles (x16) and its rows'
        # sums of squares (ssq); the projection behind the norm reads x16 with gamma-folded weights and scales by rstd — no norm launch
        fold = tl and P["rms_fold"]
        x16 = ssq = None
        nl = len(P["layers"])
        for li, lw in enumerate(P["layers"]):
            if fold and li > 0:
                qkv = lw["wqkv"].gemv(x16, ssq_in=(ssq, self.H, eps))
            else:
                h = ops.rmsnorm(x, lw["ln1"], eps, dt, tiled=tl)
                qkv = lw["wqkv"].gemv(h)                                             # [G, 3H]
            if self.fused_decode_attention and hd % 16 == 0:
                # RoPE + KV append + split-KV attention + combine as one launch (bit-identical to the three-kernel form below)
                att = ops.attn_decode_fused(qkv, P["kc"][li], P["vc"][li], P["pos"], P["cos"], P["sin"], scale, nh, hd,
                                            P["attn_cnt"], nsplit=self.decode_nsplit, out_tiled=tl)
            else:
                ops.rope_kv_append_b(qkv, P["kc"][li], P["vc"][li], P["cos"], P["sin"], P["pos"], G, 1, nh, hd)
                q = qkv[:, :H].unflatten(1, (nh, hd))                                # strided view into qkv: no copy
                att = ops.attn_decode_b(q, P["kc"][li], P["vc"][li], P["ctx"], scale, nsplit=self.decode_nsplit, out_tiled=tl)
            if fold:
                x, x16, ssq = lw["wo"].gemv(att, ws, residual=x, out_dtype=torch.float32, emit_norm=True)
                g = lw["wgu"].gemv(x16, act="silu", glu=True, y_tiled=True, ssq_in=(ssq, self.H, eps))
                if li + 1 < nl:
                    x, x16, ssq = lw["wd"].gemv(g, ws, residual=x, out_dtype=torch.float32, emit_norm=True)
                else:                        # the final norm needs fp32 states (hidden-state output): its own launch
                    x = lw["wd"].gemv(g, ws, residual=x, out_dtype=torch.float32)
                continue
            x = comm.all_reduce(lw["wo"].gemv(att, ws, residual=x if lead else None, out_dtype=torch.float32))
            h = ops.rmsnorm(x, lw["ln2"], eps, dt, tiled=tl)
            g = lw["wgu"].gemv(h, act="silu", glu=True, y_tiled=tl)
            x = comm.all_reduce(lw["wd"].gemv(g, ws, residual=x if lead else None, out_dtype=torch.float32))
        if slots is None:
            ops.add_i32(P["pos"], 1)
            ops.add_i32(P["ctx"], 1)
        return x

    def _layers_single_precise(self, x, slots=None, adapters=False, spec=False):
        """_layers_single with fp32-grade activations: the x operand of every skinny GEMM is a two-block Tiled16 (hi plane, lo plane;
        sx_gemv x_planes = 2 — each weight fragment feeds two MFMAs, the weights stream once), its outputs are fp32; RoPE, the KV
        cache and attention are fp32 (sx_rope_kv_append_f32, sx_attention_f32 at T = 1). Shapes outside the skinny GEMM's MFMA path
        (miniature test dims) take the a_planes = 2 GEMM instead. No host reads → graph-capturable.
        ``adapters``: the adapter token step — this body on its UNFOLDED arrangement (the branch SX_RMS_FOLD=0 selects) with the per-row
        gammas (sx_rmsnorm_planes_sel) and, in front of each of the four skinny GEMMs, shrink + expand on the x operand it already
        reads; the fp32 delta enters that GEMM's epilogue before activation / GLU / residual (sx_gemv_args.addend). The adapter slot of
        every sequence is read from device memory (P["lora"]["sel"]); a row without an adapter has the bits of the unfolded base step.
        ``spec``: the verify step of speculative decoding — x holds T = spec_tokens + 1 rows per sequence (row g*T + t at position
        pos[g] + t), the attention is the verify form of the fused-RoPE launch, and the split-K workspace and attention partials are
        the ones sized for G*T rows (P["spec"]). Everything else is the same calls on more rows."""
        P, dt, nh, hd, G = self._P, self.dtype, self.nh_l, self.hd, self.G
        T = self.spec_tokens + 1 if spec else 1
        assert not (spec and adapters) and x.shape[0] == G * T
        lo = P["lora"] if adapters else None
        assert lo is None or (P["precise_tiled"] and P["decode_tiled"])
        comm, lead = self.comm, self.comm.rank == 0
        eps, scale = self.config.rms_norm_eps, 1.0 / math.sqrt(hd)
        tl, ws, f32 = P["precise_tiled"], P["gemv_ws"], torch.float32
        part = P["attn_f32_part"]
        if spec:
            ws, part = P["spec"]["gemv_ws"], P["spec"]["attn_part"]

        def delta(xp, li, kk):
            """the adapter step's addend of projection kk for the operand xp (nothing without adapters)"""
            if lo is None:
                return {}
            t = ops.lora_shrink(xp, lo["A"][kk][li], lo["sel"])
            return dict(addend=(ops.lora_expand(t, lo["B"][kk][li], lo["seg"][kk], lo["scale"], lo["sel"]), lo["sel"], self.max_adapters))

        def norm(xx, li, k):
            if lo is None:
                return ops.rmsnorm_planes(xx, lw[k], eps, dt, tiled=tl)[0]
            return ops.rmsnorm_planes_sel(xx, lw[k], lo[k][li], lo["sel"], eps, dt, tiled=tl)[0]

        def lin(xp, lw, k, **kw):
            if tl:
                return lw[k].gemv(xp, ws, out_dtype=f32, **kw)      # (tl: every projection has its decode tiles, built for every G)
            return ops.gemm(xp, lw[k].w, a_planes=2, out_dtype=f32, **kw)
        fold = P["rms_fold_precise"] and lo is None
        fuse_rope = hd == 128 and (spec or os.environ.get("SX_LLM_FUSE_ROPE", "1") != "0")   # (the verify form IS the fused form)
        x16 = ssq = None
        nl = len(P["layers"])
        for li, lw in enumerate(P["layers"]):
            if fold and li > 0:
                qkv = lin(x16, lw, "wqkv", ssq_in=(ssq, self.H, eps))                 # x16 = planes of x * ln1 (written by the down GEMV)
            else:
                h = norm(x, li, "ln1")
                qkv = lin(h, lw, "wqkv", **delta(h, li, "qkv"))                       # [G, 3H] fp32
            kw = self._kv_kw(li)    # kv_format: the row scales of the FP8 cache, or the emulate flag of its fp32 twin; kv_pages: the page table
            if fuse_rope:           # RoPE + KV append inside the attention launch (one graph node per layer instead of two)
                att = ops.attention_f32(qkv, P["kc"][li], P["vc"][li], P["pos"], G, T, nh, hd, scale, dt, tiled=tl,
                                        nsplit=self.decode_nsplit_f32, scratch=part, rope=(P["cos"], P["sin"]), **kw)
            else:
                ops.rope_kv_append_f32(qkv, P["kc"][li], P["vc"][li], P["cos"], P["sin"], P["pos"], G, 1, nh, hd, dt, **kw)
                att = ops.attention_f32(qkv, P["kc"][li], P["vc"][li], P["pos"], G, 1, nh, hd, scale, dt, tiled=tl,
                                        nsplit=self.decode_nsplit_f32, scratch=P["attn_f32_part"],
                                        **{k: kw[k] for k in ("kv_scales", "paged") if k in kw})
            if fold:
                # residual GEMV: fp32 x, the planes of x * gamma of the NEXT norm, the rows' sums of squares; GLU epilogue: planes directly
                x, x16, ssq = lin(att, lw, "wo", residual=x, emit_norm=True, planes_out=True, norm_gamma=lw["ln2"])
                g = lw["wgu"].gemv(x16, act="silu", glu=True, y_tiled=True, planes_out=True, ssq_in=(ssq, self.H, eps))
                if li + 1 < nl:
                    x, x16, ssq = lin(g, lw, "wd", residual=x, emit_norm=True, planes_out=True, norm_gamma=P["layers"][li + 1]["ln1"])
                else:                        # the final norm wants fp32 states: its own launch (rmsnorm_planes in _decode_step_body)
                    x = lin(g, lw, "wd", residual=x)
                continue
            x = comm.all_reduce(lin(att, lw, "wo", residual=x if lead else None, **delta(att, li, "o")))
            h = norm(x, li, "ln2")
            if tl:                           # SiLU-GLU epilogue writes the two planes of its result itself (no sx_split16 launch)
                g = lw["wgu"].gemv(h, act="silu", glu=True, y_tiled=True, planes_out=True, **delta(h, li, "gu"))
            else:
                g = ops.split16(lin(h, lw, "wgu", act="silu", glu=True), dt)
            x = comm.all_reduce(lin(g, lw, "wd", residual=x if lead else None, **delta(g, li, "d")))
        if slots is None:
            ops.add_i32(P["pos"], 1)
            ops.add_i32(P["ctx"], 1)
        return x

    def _final_norm(self, x, sel=None):
        """model.norm (modeling_llama_xformer.py:595) → fp32 hidden states. ``sel`` (int32 per row, device): the rows' adapter slots —
        an adapter's modules_to_save copy of model.norm replaces gamma for its rows."""
        if sel is not None:
            return ops.rmsnorm_planes_sel(x.contiguous(), self._P["norm"], self._P["lora"]["norm"], sel, self.config.rms_norm_eps, self.dtype,
                                          want_f32=True, want_planes=False)[1]
        if self.precise:
            return ops.rmsnorm_planes(x.contiguous(), self._P["norm"], self.config.rms_norm_eps, self.dtype, want_f32=True,
                                      want_planes=False)[1]
        return ops.rmsnorm(x, self._P["norm"], self.config.rms_norm_eps, torch.float32)

    def _lm_head(self, hn_rows):
        """lm_head (:707) on fp32 post-norm rows → fp32 logits [rows, Vpad / tp]."""
        P = self._P
        if self.precise:
            return ops.linear_planes(hn_rows.contiguous(), P["lm_head"], w_tiles=P["lm_head_t"], out_dtype=torch.float32)
        return ops.linear(ops.cast(hn_rows.contiguous(), self.dtype), P["lm_head"], out_dtype=torch.float32)

    def forward_embeds(self, inputs_embeds, need_logits=True, seq=0, adapter=None):
        """inputs_embeds: fp32 [T, H] on the GPU, appended to sequence `seq` at its current cache position.
        Returns (logits fp32 [Vpad] of the LAST position or None, final-norm hidden states fp32 [T, H]).
        ``adapter``: name of a resident LoRA adapter the rows run under (forward_embeds_batch)."""
        if adapter is not None:
            self.kv_epoch += 1          # a write outside generate_batch, as below
            logits, hs = self.forward_embeds_batch([inputs_embeds], [seq], need_logits, adapters=[adapter])
            return (None if logits is None else logits[0]), hs[0]
        P = self._pack()
        self.kv_epoch += 1              # a write outside generate_batch: cached-prefix records no longer describe the cache
        x = inputs_embeds.to(device=self.device, dtype=torch.float32).contiguous()
        T = x.shape[0]
        if T == 1 and self.G == 1:
            if self.kv_pages:           # (the multi-row pass reserves for itself; this one runs the token step's layers)
                self._kv_need(seq, int(P["pos"][seq].item()) + 1, "a one-token pass")
            x = self._layers_single(x)
        else:
            x = self._layers_multi(x, [T], [seq])
        hn = self._final_norm(x)                                                     # :595
        logits = None
        if need_logits:
            logits = self._lm_head(hn[-1:])[0]
            if self.tp > 1:
                logits = self.comm.all_gather(logits).reshape(-1)                     # [tp, V/tp] → [Vpad], vocab order
        return logits, hn

    def forward_embeds_batch(self, xs, seqs, need_logits=True, adapters=None):
        """xs[i]: fp32 [T_i, H] appended to sequence seqs[i]; all sequences in one pass (see _layers_multi).
        Returns (logits fp32 [n, Vpad] of each sequence's LAST position or None, list of final-norm states [T_i, H]).
        ``adapters``: per sequence the name of a resident LoRA adapter or None; the KV rows written depend on it. None, or no name at
        all: exactly the pass without the argument."""
        P = self._pack()
        Ts = [int(x.shape[0]) for x in xs]
        x = torch.cat([x.to(device=self.device, dtype=torch.float32) for x in xs], dim=0).contiguous()   # plumbing
        idx = [self._adapter_index(a) for a in adapters] if adapters is not None else None
        if idx is not None and any(a >= 0 for a in idx):
            assert len(idx) == len(Ts)
            x = self._layers_multi(x, Ts, list(seqs), adapters=idx)
            sel = torch.repeat_interleave(torch.tensor(idx, dtype=torch.int32), torch.tensor(Ts)).to(self.device)
            hn = self._final_norm(x, sel)
        else:
            x = self._layers_multi(x, Ts, list(seqs))
            hn = self._final_norm(x)
        ends = torch.tensor([sum(Ts[:i + 1]) - 1 for i in range(len(Ts))], device=self.device)
        logits = None
        if need_logits:
            logits = self._lm_head(hn[ends])                                           # [n, Vpad / tp]
            if self.tp > 1:
                logits = self.comm.all_gather(logits).permute(1, 0, 2).reshape(len(Ts), self.Vpad).contiguous()
        return logits, list(torch.split(hn, Ts, dim=0))

    def set_position(self, seq, pos):
        """Truncate / rewind sequence `seq`'s KV cache to `pos` tokens (cross-turn prefix reuse)."""
        P = self._pack()
        assert 0 <= pos <= self.Tmax
        P["pos"][seq] = pos
        P["ctx"][seq] = pos + 1

    # reference-style entry (prefill + cached steps through inputs_embeds / input_ids), batch 1
    def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, inputs_embeds=None,
                labels=None, use_cache=True, output_attentions=None, output_hidden_states=None, return_dict=True,
                logits_positions="all"):
        """The reference forward's inference contract (modeling_llama_xformer.py:643-746), batch 1 (sequence 0).
        Returns a ``CausalLMOutputWithPast`` (attribute / key / index access like transformers' ModelOutput) with
          * ``logits`` [1, T, V] fp32 for EVERY position (:707; ``logits_positions="last"`` → [1, 1, V], what the greedy loop needs),
          * ``past_key_values``: per layer (k, v) VIEWS [1, heads, T_total, hd] of the module's pre-allocated cache (:217-220 builds
            them with torch.cat). Passing any non-None value back continues from the internal cache — its length must equal the
            cache position; ``None`` starts a new sequence,
          * ``hidden_states`` (if requested): a tuple of L + 1 entries like the reference's (:580-599) whose LAST entry is the
            post-final-norm state [1, T, H]; the intermediate entries are None (never materialised; the path only reads [-1],
            seed_x.py:98,196).
        ``attention_mask`` is accepted and ignored exactly as far as the reference ignores it (padding is never honoured, :236;
        prefill is causal, a q_len == 1 step sees the whole cache); ``position_ids`` must be the default arange (what
        prepare_inputs_for_generation :759-765 produces for an all-ones mask). Training inputs (``labels``) are out of scope."""
        if labels is not None:
            raise NotImplementedError("LlamaForCausalLM.forward: the loss path (labels) is training-side and not built")
        if attention_mask is not None and not bool(torch.as_tensor(attention_mask).to(torch.bool).all()):
            import warnings       # the reference does the same silently (:236 only asks whether the mask is all zero); say it once
            warnings.warn("LlamaForCausalLM.forward: attention_mask has zeros (padding) — like the reference's xformers path "
                          "(modeling_llama_xformer.py:232-237) padding is NOT masked: every position attends causally", stacklevel=2)
        if output_attentions:
            raise NotImplementedError("LlamaForCausalLM.forward: attention probabilities are never materialised (flash attention)")
        P = self._pack()
        if past_key_values is None:
            self.reset(0)
        else:
            held = int(P["pos"][0].item())
            if isinstance(past_key_values, (tuple, list)) and len(past_key_values) and isinstance(past_key_values[0], (tuple, list)):
                got = int(past_key_values[0][0].shape[2])
                assert got == held, f"past_key_values holds {got} tokens but the module's cache is at position {held}"
        if inputs_embeds is None:
            inputs_embeds = self.get_input_embeddings()(input_ids)
        x = inputs_embeds.reshape(-1, self.H)
        T = x.shape[0]
        if position_ids is not None:
            p0 = int(P["pos"][0].item())
            want = torch.arange(p0, p0 + T)
            assert torch.equal(position_ids.reshape(-1).cpu().long(), want), "only the default (arange) position_ids are supported"
        if logits_positions == "last":
            logits, hn = self.forward_embeds(x, seq=0)
            logits = logits[: self.V].view(1, 1, -1)
        else:
            _, hn = self.forward_embeds(x, need_logits=False, seq=0)
            logits = self._lm_head(hn)                                                                           # [T, Vpad / tp]
            if self.tp > 1:
                logits = self.comm.all_gather(logits).permute(1, 0, 2).reshape(T, self.Vpad)
            logits = logits[:, : self.V].unsqueeze(0)
        Tk = int(P["pos"][0].item())
        if use_cache and self.kv_format == "fp8_e4m3":
            # dequantised fp32 COPIES (plumbing: the contract only hands them back and reads shape[2])
            from . import quant
            tab = quant.decode_table(self.device)
            deq = lambda c, sc: (tab[c[0][:, :Tk].long()] * sc[0][:, :Tk, None]).unsqueeze(0)
            pkv = tuple((deq(P["kc"][li], P["ks"][li]), deq(P["vc"][li], P["vs"][li])) for li in range(self.L))
        elif use_cache and self.kv_pages:
            # gathered COPIES of sequence 0's pages (plumbing, like the FP8 cache's dequantised copies)
            pkv = tuple(tuple(t.unsqueeze(0) for t in self._kv_gather(li, 0, Tk)) for li in range(self.L))
        else:
            pkv = tuple((P["kc"][li][0][:, :Tk].unsqueeze(0), P["vc"][li][0][:, :Tk].unsqueeze(0)) for li in range(self.L)) \
                if use_cache else None
        hs = ((None,) * self.L + (hn.view(1, -1, self.H),)) if output_hidden_states else None
        out = CausalLMOutputWithPast(loss=None, logits=logits, past_key_values=pkv, hidden_states=hs, attentions=None)
        return out if return_dict else out.to_tuple()

    __call__ = forward

    # ---- in-flight batching: slot states ---------------------------------------------------------------------------------
    def slot_state(self, force_id=-1, eos_id=-1, sampling=False, logprobs=None, controls=False, grammar=False, seq_rules=False):
        """A fresh SlotState with EVERY slot parked (the module's pos / ctx / step take the idle values; ``reset()`` undoes that).
        ``sampling``: the state carries a SampleState (``.sampling``, all rows greedy until set) and its token step ends in
        sx_sample_next_slots instead of sx_greedy_next_slots. ``logprobs`` = n_top (0 .. 8): the state carries a LogprobState
        (``.logprobs``, no row recording until ``want`` is set) and its token step ends in sx_sample_next_slots_lp. ``controls``: the
        state carries a ControlState (``.controls``, every row off until set) and its token step ends in sx_next_slots_ctl — greedy,
        sampled, with or without the record. ``grammar``: the state carries a GrammarState (``.grammar``, every row unconstrained until
        set) beside a ControlState (the constrained tail works on the controls' working rows) and its token step ends in
        sx_next_slots_fsm. ``seq_rules``: the state carries a SeqRuleState (``.seq_rules``, every row off until set) beside a
        ControlState (the n-gram ban works on the controls' working rows) and its token step ends in sx_next_slots_seq, with or
        without a grammar."""
        if grammar and not self.max_grammars:
            raise ValueError("LlamaForCausalLM.slot_state: grammar=True on a model built with max_grammars=0")
        if self.tp > 1:
            raise NotImplementedError("in-flight batching (slot states) is single-rank: tensor-parallel ranks are not supported")
        self._pack()
        st = SlotState(self.G, self.device, force_id, eos_id, sampling)
        if logprobs is not None:
            st.logprobs = LogprobState(self.G, logprobs, self.device)
        if controls or grammar or seq_rules:
            st.controls = self.control_state(fresh=True)
        if seq_rules:
            st.seq_rules = self.seq_rule_state(fresh=True)
        if grammar:
            st.grammar = self.grammar_state(fresh=True)
        if sampling and self.spec_tokens:
            T = self.spec_tokens + 1
            st.sampling.rows = (SampleState(self.G * T, self.device), T)
        if self.max_adapters:
            st.adapter = self._P["lora"]["sel"]
        self.park_slots(range(self.G), st)
        return st

    def _slot_write(self, t, slots, values):
        """t[slots[i]] = values[i] (or one value for all) for a device int32 [G] tensor: one small host → device copy."""
        slots = list(slots)
        if not slots:
            return
        vals = [int(values)] * len(slots) if not isinstance(values, (list, tuple)) else [int(v) for v in values]
        idx = torch.tensor(slots, dtype=torch.int64, device=self.device)
        t.index_copy_(0, idx, torch.tensor(vals, dtype=torch.int32, device=self.device))

    def park_slots(self, slots, state):
        """Host-side parking (a slot the device did not park itself: never used, or finished at admission / in an image chunk)."""
        P = self._pack()
        slots = list(slots)
        self.kv_epoch += 1
        self._slot_write(state.live, slots, 0)
        for k, v in SlotState.IDLE.items():
            self._slot_write(P[k], slots, v)
        if self.kv_pages:
            for g in slots:
                self.kv_release(g)
        if self.max_adapters:
            self.set_adapters(slots, [None] * len(slots))

    # ---- device-resident greedy decode step (all sequences in lock step) -----------------------------------------------
    def sample_state(self):
        """The module's SampleState for the lock-step step (``decode_step(..., sampling=...)``), made once: its pointers are part of
        the captured graph's key."""
        self._pack()
        if self._sample_state is None:
            self._sample_state = SampleState(self.G, self.device)
        return self._sample_state

    def control_state(self, fresh=False):
        """A ControlState for this model's logits rows ([G, Vpad] fp32). The lock-step step's (``decode_step(..., controls=...)``) is
        made once — its pointers are part of the captured graph's key; ``fresh``: a new one (a slot state owns its own)."""
        self._pack()
        if fresh:
            return ControlState(self.G, self.V, self.Vpad, self.device)
        if getattr(self, "_control_state", None) is None:
            self._control_state = ControlState(self.G, self.V, self.Vpad, self.device)
        return self._control_state

    def seq_rule_state(self, fresh=False):
        """A SeqRuleState for this model (history rows of max_cache_len ids). The lock-step step's (``decode_step(..., seq_rules=...)``)
        is made once — its pointers are part of the captured graph's key; ``fresh``: a new one (a slot state owns its own)."""
        self._pack()
        if fresh:
            return SeqRuleState(self.G, self.V, self.Tmax, self.device)
        if getattr(self, "_seq_rule_state", None) is None:
            self._seq_rule_state = SeqRuleState(self.G, self.V, self.Tmax, self.device)
        return self._seq_rule_state

    def _off_controls(self):
        """A ControlState with every row off, never set: the working rows of a lock-step grammar step that carries no controls."""
        if getattr(self, "_off_control_state", None) is None:
            self._off_control_state = ControlState(self.G, self.V, self.Vpad, self.device)
        return self._off_control_state

    def _step_tail(self, x, hid_buf, sel=None, tok=None):
        """The end of every token step: final norm → the post-norm fp32 rows into hid_buf (row g at step[g]; verify step: row (g, t) at
        step[g] + t, ``tok`` takes the token indices) → lm_head logits fp32 [rows, Vpad / tp]. ``sel``: the adapter step — the final
        norm picks every row's gamma like the layers' norms; lm_head has no adapter."""
        P, eps, dt, f32 = self._P, self.config.rms_norm_eps, self.dtype, torch.float32
        tl = P["precise_tiled"]
        if not self.precise:
            hn = ops.rmsnorm(x, P["norm"], eps, f32)
        elif sel is not None:
            hp, hn = ops.rmsnorm_planes_sel(x, P["norm"], P["lora"]["norm"], sel, eps, dt, tiled=tl, want_f32=True)
        else:
            hp, hn = ops.rmsnorm_planes(x, P["norm"], eps, dt, tiled=tl, want_f32=True)
        if tok is None:
            ops.scatter_rows_step(hn, P["step"], hid_buf)
        else:
            ops.scatter_rows_spec(hn, P["step"], hid_buf, tok)
        if self.precise and not tl:              # shapes outside the skinny GEMM's MFMA path (miniature test dims)
            return ops.gemm(hp, P["lm_head"], a_planes=2, out_dtype=f32)
        return ops.gemv(hp if self.precise else ops.cast(hn, dt), P["lm_head"], out_dtype=f32, w_tiles=P["lm_head_t"])

    def _replay(self, attr, key, body, snap, slots=None):
        """Replay the token step ``body`` (a callable without arguments) from the graph held in ``self.<attr>`` = (key, graph[, the
        slot step's logits]); captured first where none is held under ``key``: warm-up on a side stream (allocator / lazy module
        load), then capture of one step. Both really run the step: everything it advances — pos / ctx / step / cur and the tensors
        ``snap``; in slot mode it may even finish a slot — is put back after each."""
        held = getattr(self, attr)
        if held is None or held[0] != key:
            saved = [(t, t.clone()) for t in [self._P[k] for k in ("pos", "ctx", "step", "cur")] + snap]
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                body()
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            for t, v in saved:
                t.copy_(v)
            g = torch.cuda.CUDAGraph()
            with ops.graph_capture(g):
                body()
            for t, v in saved:
                t.copy_(v)
            held = (key, g) + ((slots.logits,) if slots is not None else ())
            setattr(self, attr, held)
        if slots is not None:
            slots.logits = held[2]
        held[1].replay()

    def _decode_step_body(self, img_ids_dev, out_ids, hid_buf, slots=None, sampling=None, adapters=False, logprobs=None, controls=None,
                          eos_id=-1, grammar=None, seq_rules=None):
        """cur[G] → embedding → 40 layers → final norm → lm_head → logits rule + argmax → cur[G]. Records the post-norm
        hidden state of each INPUT token at hid_buf[g, step[g]] (what seed_x.py:196 collects) and the new id at
        out_ids[g, step[g]]; then step += 1. Everything stays on the device. ``slots`` (a SlotState): the tail is ONE
        sx_greedy_next_slots launch — next id, stop rule and the advance of pos / ctx / step for the live slots only; parked
        slots ride along through the GEMVs and write nothing."""
        P = self._P
        x = ops.embedding(P["cur"], P["embed"])                                        # [G, H] fp32
        x = self._layers_single_precise(x, slots, adapters=True) if adapters else self._layers_single(x, slots)
        logits = self._step_tail(x, hid_buf, sel=P["lora"]["sel"] if adapters else None)
        if self.tp > 1:
            logits = self.comm.all_gather(logits).permute(1, 0, 2).reshape(self.G, self.Vpad).contiguous()
        # sampled step: same tail, the id by the seeded rule (token index = step[g]); on tensor-parallel ranks every rank draws from the
        # same gathered logits with the same seed and index
        ss = sampling if slots is None else slots.sampling
        sample = {} if ss is None else dict(sample=ss, n_kept=ss.n_kept, p_chosen=ss.p_chosen)
        # LP step: the same tail with the record of the raw row (a LogprobState), greedy or sampled
        lp = logprobs if slots is None else slots.logprobs
        if lp is not None:
            sample["lp"] = lp
        # controlled step: the same tail again, ids from the edited copy of every controlled row (a ControlState)
        ctl = controls if slots is None else slots.controls
        if ctl is not None:
            sample["ctl"] = ctl
        # constrained step: the same tail once more, with a token automaton per row (a GrammarState) on the controls' working rows
        fsm = grammar if slots is None else slots.grammar
        if fsm is not None:
            sample["fsm"] = fsm
        # sequence-rule step: the same tail with the n-gram ban, the id history and the stop match (a SeqRuleState), fsm or not
        seq = seq_rules if slots is None else slots.seq_rules
        if seq is not None:
            sample["seq"] = seq
        if slots is not None:
            tail = ops.next_slots_seq if seq is not None else ops.next_slots_fsm if fsm is not None else ops.next_slots_ctl if ctl is not None else ops.next_slots_lp if lp is not None else ops.sample_next_slots if sample \
                else ops.greedy_next_slots
            tail(logits, self.V, img_ids_dev, P["cur"], slots.live, slots.n_new, slots.max_new, slots.force_at, P["pos"], P["ctx"],
                 P["step"], out_ids, slots.status, force_id=slots.force_id, eos_id=slots.eos_id, **sample)
            slots.logits = logits
            return
        if ctl is not None:
            sample["eos_id"] = eos_id
        tail = ops.next_b_seq if seq is not None else ops.next_b_fsm if fsm is not None else ops.next_b_ctl if ctl is not None else ops.next_b_lp if lp is not None else ops.sample_next_b if sample else ops.greedy_next_b
        tail(logits, self.V, img_ids_dev, P["cur"], out_ids, P["step"], **sample)
        ops.add_i32(P["step"], 1)

    def _spec_step_body(self, img_ids_dev, out_ids, hid_buf, slots, draft):
        """The verify step of speculative decoding, the slot step over G*T rows (T = spec_tokens + 1): [n-gram draft →] embedding of the
        row inputs → the layers with the verify attention → final norm → hidden state of row (g, t) at hid_buf[g, step[g] + t] →
        lm_head → every row's candidate id (the plain step's rule or sampler: previous id = the row's input, token index step[g] + t)
        → sx_spec_accept: the emitted ids to out_ids[g, step[g] ...] and to the id history, the counters advanced by the emitted
        count, stop rule, parking and status as in the plain slot step. No host reads."""
        P, S = self._P, self._P["spec"]
        if draft == "ngram":
            ops.spec_draft_ngram(S["hist"], P["pos"], P["cur"], S["rows"], S["n_draft"], self.spec_ngram)
        x = ops.embedding(S["rows"], P["embed"])                                       # [G*T, H] fp32
        x = self._layers_single_precise(x, slots, spec=True)
        logits = self._step_tail(x, hid_buf, tok=S["tok"])
        ss = slots.sampling
        ops.spec_candidates(logits, self.V, img_ids_dev, S["rows"], S["cand"], S["tok"], sample=None if ss is None else ss.rows[0])
        ops.spec_accept(S["cand"], S["rows"], S["n_draft"], P["cur"], slots.live, slots.n_new, slots.max_new, slots.force_at, P["pos"],
                        P["ctx"], P["step"], out_ids, slots.status, hist=S["hist"], force_id=slots.force_id, eos_id=slots.eos_id,
                        img_ids_dev=img_ids_dev)
        slots.logits = logits

    def spec_write_history(self, slot, start, ids):
        """hist[slot, start : start + len(ids)] = ids: the ids fed (or about to be fed) at those cache positions, for the n-gram drafter.
        Admission writes the prompt's ids (placeholders for image rows) and the first token; a host-driven chunk its block."""
        S = self._pack()["spec"]
        ids = [int(i) for i in ids][:max(0, self.Tmax - int(start))]
        if ids:
            S["hist"][slot, start:start + len(ids)] = torch.tensor(ids, dtype=torch.int32, device=self.device)

    def decode_step(self, img_ids_dev, out_ids, hid_buf, use_graph=True, slots=None, sampling=None, adapters=None, spec=False, draft="ngram",
                    logprobs=None, controls=None, eos_id=-1, grammar=None, seq_rules=None):
        """out_ids: int32 [G, rows]; hid_buf: fp32 [G, rows, H]. ``slots``: a SlotState → the in-flight step (its captured graph is
        kept apart from the lock-step one, so one graph serves an engine's lifetime whatever else runs in between). ``sampling``: a
        SampleState → the lock-step step ends in sx_sample_next_b (token index = step[g]); a slot state brings its own
        (``slots.sampling``). The state's pointers are part of the graph key: a sampled step and a greedy step never share a graph,
        and the parameters are read from device memory at replay.
        ``adapters``: None (default) → the adapter token step runs iff some sequence has an adapter (set_adapters); True / False force
        it. The adapter step has captured graphs of its own; a step in which no sequence has an adapter runs the calls and graphs it
        ran before adapters existed.
        ``logprobs``: a LogprobState → the lock-step step ends in the LP tail (sx_sample_next_b_lp: rows with ``want`` set record the
        log-probability of their id and the top list at [g, step[g]]); a slot state brings its own (``slots.logprobs``,
        sx_sample_next_slots_lp). Only the tail changes, so it works with every weight_format, weight_residency, kv_format, kv_pages,
        adapters and sampling; the step has captured graphs of its own, and a step without a state runs the calls and graphs it always ran.
        ValueError with the verify step (``spec=True``) and on tensor-parallel ranks: follow-ups.
        ``controls``: a ControlState → the lock-step step ends in the controlled tail (sx_next_b_ctl, token index = step[g], ``eos_id``
        the column min_new_tokens masks); a slot state brings its own (``slots.controls``, sx_next_slots_ctl). Again only the tail
        changes, graphs of its own (attribute suffix ``_ctl``), and a step without a state runs the calls and graphs it always ran.
        ValueError with the verify step and on tensor-parallel ranks: follow-ups.
        ``grammar``: a GrammarState → the lock-step step ends in the constrained tail (sx_next_b_fsm; ``eos_id`` is the column that
        survives in accepting states only; without ``controls`` the module's control state with every row off carries the working
        rows); a slot state brings its own (``slots.grammar``, sx_next_slots_fsm). Only the tail changes, graphs of its own (attribute
        suffix ``_fsm``), and a step without a state runs the calls and graphs it always ran. ValueError with the verify step and on
        tensor-parallel ranks: follow-ups.
        ``seq_rules``: a SeqRuleState → the lock-step step ends in the sequence-rule tail (sx_next_b_seq: no_repeat_ngram_size ban, id
        history, stop match; with or without ``controls`` / ``grammar``, the module's control state with every row off carries the
        working rows otherwise); a slot state brings its own (``slots.seq_rules``, sx_next_slots_seq, where a stop match parks the
        slot). Only the tail changes, graphs of its own (attribute suffix ``_seq``), and a step without a state runs the calls and
        graphs it always ran. ValueError with the verify step and on tensor-parallel ranks: follow-ups."""
        P = self._pack()
        seq = seq_rules if slots is None else getattr(slots, "seq_rules", None)
        if slots is not None and seq_rules is not None:
            raise ValueError("LlamaForCausalLM.decode_step: a slot state carries its own sequence-rule state (slot_state(seq_rules=True))")
        if seq is not None:
            if spec:
                raise ValueError("LlamaForCausalLM.decode_step: stop sequences / no_repeat_ngram_size in the verify step of speculative "
                                 "decoding (spec=True with a sequence-rule state) are not built (follow-up: a ban and a stop match per "
                                 "candidate row of the accepted run)")
            if self.tp > 1:
                raise ValueError(f"LlamaForCausalLM.decode_step: sequence rules on tp={self.tp} tensor-parallel ranks are not built "
                                 "(follow-up: every rank would ban, append and match on the gathered logits)")
            assert seq.G == self.G and seq.ld_hist >= self.Tmax
            if slots is None and controls is None:
                controls = self._off_controls()
        fsm = grammar if slots is None else getattr(slots, "grammar", None)
        if slots is not None and grammar is not None:
            raise ValueError("LlamaForCausalLM.decode_step: a slot state carries its own grammar state (slot_state(grammar=True))")
        if fsm is not None:
            if spec:
                raise ValueError("LlamaForCausalLM.decode_step: a grammar in the verify step of speculative decoding (spec=True with a "
                                 "grammar state) is not built (follow-up: automaton states that advance with the accepted run)")
            if self.tp > 1:
                raise ValueError(f"LlamaForCausalLM.decode_step: grammars on tp={self.tp} tensor-parallel ranks are not built "
                                 "(follow-up: every rank would mask and advance on the gathered logits)")
            assert fsm.G == self.G and fsm.trans is P["grammar"]["trans"]
            if slots is None and controls is None:
                controls = self._off_controls()
        ctl = controls if slots is None else getattr(slots, "controls", None)
        if slots is not None and controls is not None:
            raise ValueError("LlamaForCausalLM.decode_step: a slot state carries its own control state (slot_state(controls=True))")
        if ctl is not None:
            if spec:
                raise ValueError("LlamaForCausalLM.decode_step: logits controls in the verify step of speculative decoding (spec=True with "
                                 "a control state) are not built (follow-up: counts that advance with the accepted run)")
            if self.tp > 1:
                raise ValueError(f"LlamaForCausalLM.decode_step: logits controls on tp={self.tp} tensor-parallel ranks are not built "
                                 "(follow-up: every rank would edit and count on the gathered logits)")
            assert ctl.G == self.G and ctl.V == self.V and ctl.ld == self.Vpad
        lp = logprobs if slots is None else getattr(slots, "logprobs", None)
        if lp is not None:
            if slots is not None and logprobs is not None:
                raise ValueError("LlamaForCausalLM.decode_step: a slot state carries its own logprob state (slot_state(logprobs=n_top))")
            if spec:
                raise ValueError("LlamaForCausalLM.decode_step: token log-probabilities from the verify step of speculative decoding "
                                 "(spec=True with a logprob state) are not built (follow-up: records for the G*T candidate rows)")
            if self.tp > 1:
                raise ValueError(f"LlamaForCausalLM.decode_step: token log-probabilities on tp={self.tp} tensor-parallel ranks are not built "
                                 "(follow-up: every rank would record from the gathered logits)")
            assert lp.G == self.G and out_ids.is_contiguous()
            lp.bind(out_ids.shape[1])
        elif logprobs is not None:
            raise ValueError("LlamaForCausalLM.decode_step: a slot state carries its own logprob state (slot_state(logprobs=n_top))")
        if spec:
            # the verify step of speculative decoding (spec_tokens > 0, a slot state): graphs of its own, greedy and sampled; without
            # ``spec`` a model built with spec_tokens runs the plain steps and graphs below. ``draft``: "ngram" → the step starts with
            # sx_spec_draft_ngram over the id history (``self.spec_ngram`` = (longest, shortest) n-gram); "given" → the caller wrote
            # rows 1 .. of P["spec"]["rows"] and P["spec"]["n_draft"] itself (row 0 is kept by sx_spec_accept)
            if not self.spec_tokens or slots is None:
                raise ValueError("LlamaForCausalLM.decode_step(spec=True) needs spec_tokens > 0 and a slot state")
            if draft not in ("ngram", "given"):
                raise ValueError(f"LlamaForCausalLM.decode_step: draft must be 'ngram' or 'given', not {draft!r}")
            assert sampling is None and not adapters and slots.G == self.G and out_ids.is_contiguous() and hid_buf.is_contiguous()
            assert out_ids.shape[0] == self.G and hid_buf.shape[0] == self.G and hid_buf.shape[1] == out_ids.shape[1]
            assert slots.sampling is None or slots.sampling.rows is not None, "a sampled slot state made by slot_state() of this model"
            body = lambda: self._spec_step_body(img_ids_dev, out_ids, hid_buf, slots, draft)
            if not use_graph or not self.comm.graph_safe:
                return body()
            key = (img_ids_dev.data_ptr(), out_ids.data_ptr(), hid_buf.data_ptr(), tuple(out_ids.shape), draft, tuple(self.spec_ngram)) + slots.key()
            return self._replay("_spec_graph" if slots.sampling is None else "_spec_sample_graph", key, body,
                                [P["spec"]["rows"], P["spec"]["n_draft"], slots.live, slots.n_new, slots.status], slots)
        if adapters is None:
            adapters = any(a >= 0 for a in self._sel_host)
        if adapters and not self.max_adapters:
            raise ValueError("LlamaForCausalLM.decode_step: the adapter step needs max_adapters > 0")
        assert out_ids.shape[0] == self.G and hid_buf.shape[0] == self.G and hid_buf.shape[1] == out_ids.shape[1]
        if slots is not None:
            if self.tp > 1:
                raise NotImplementedError("in-flight batching (slot states) is single-rank: tensor-parallel ranks are not supported")
            assert out_ids.is_contiguous() and slots.G == self.G
            assert sampling is None, "a slot state carries its own sampling state (slot_state(sampling=True))"
        assert sampling is None or sampling.G == self.G
        body = lambda: self._decode_step_body(img_ids_dev, out_ids, hid_buf, slots, sampling, adapters, logprobs, controls, eos_id, grammar,
                                              seq_rules)
        if not use_graph or not self.comm.graph_safe:
            return body()
        if slots is None:
            attr = "_graph" if sampling is None else "_sample_graph"
        else:
            attr = "_slot_graph" if slots.sampling is None else "_slot_sample_graph"
        key = (img_ids_dev.data_ptr(), out_ids.data_ptr(), hid_buf.data_ptr(), tuple(out_ids.shape)) \
            + (slots.key() if slots is not None else ()) + (("sample",) + sampling.key() if sampling is not None else ()) \
            + (logprobs.key() if logprobs is not None else ()) + (controls.key() + (int(eos_id),) if controls is not None else ()) \
            + (grammar.key() if grammar is not None else ()) + (seq_rules.key() if seq_rules is not None else ())
        # (the controlled tail counts the id it emits: warm-up and capture run the step, so the counts are put back like the counters)
        # (... and the constrained tail advances the automaton states: put back likewise)
        self._replay(attr + ("_lp" if lp is not None else "") + ("_ad" if adapters else "")
                     + ("_fsm" if fsm is not None else "_ctl" if ctl is not None and seq is None else "") + ("_seq" if seq is not None else ""),
                     key, body,
                     ([slots.live, slots.n_new, slots.status] if slots is not None else []) + ([ctl.counts] if ctl is not None else [])
                     + ([fsm.state] if fsm is not None else []) + (seq.tensors() if seq is not None else []), slots)
