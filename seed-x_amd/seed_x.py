"""ContinuousLVLM.generate on the HIP path (reference ``src/models/mllm/seed_x.py:22-46,130-234``).

Same constructor / ``from_pretrained`` / ``generate`` signature and return dict as the reference. The greedy loop
of HF ``GenerationMixin.generate`` [ext, transformers 4.30.2] plus ``AutoImageTokenGenerationProcessor``
(generation.py:9-31) is restated as a device-resident loop: one hipGraph replay per token, a single small
read-back per token for the EOS / ``<img>`` test (the reference performs ≥45 device→host syncs per token).
When ``<img>`` is emitted the 64 forced ``<img_i>`` tokens are run as ONE 65-token causal chunk on the MFMA path
(identical math, 64× the arithmetic intensity).
``generate_batch`` runs G independent requests in lock step (one weight stream from HBM per token step for all G).
``generate_inflight`` serves a queue of any length on those G slots: the stop rule runs on the device, a finished slot idles
inside the captured step and is refilled from the queue before the next one (inflight.py holds the schedule). With
``agent.prefix_cache = True`` an admitted request keeps, or gets copied from another slot by one sx_kv_fork launch, the cache rows of the
longest prompt prefix some slot already holds, and prefills only the rest; ``agent.prefix_host_bytes > 0`` parks the rows a slot is about
to lose in pinned host memory and copies them back for a later prompt that starts like them (kvstore.py).
"""
import functools

import torch

from . import ops
from .grammar import DONE, advance
from .inflight import PrefixIndex, SlotScheduler, plan_admission, tag_signatures
from .llama import LogprobState
from .sampling import ControlParams, SamplingParams, SeqParams, logprobs_from_request, logprobs_result, stop_match

BOI_TOKEN = '<img>'
EOI_TOKEN = '</img>'
IMG_TOKEN = '<img_{:05d}>'


def _clears_adapters(fn):
    """A serving call leaves no sequence on an adapter, also when it raises midway: the per-sequence adapter index goes back to -1, so a
    later token step without adapters runs the base step and its graph."""
    @functools.wraps(fn)
    def wrapped(self, *args, **kw):
        try:
            return fn(self, *args, **kw)
        finally:
            llm = self.llm
            if getattr(llm, "max_adapters", 0) and llm._P is not None:
                llm.set_adapters(range(llm.G), [None] * llm.G)
    return wrapped


class ContinuousLVLM:
    # default of ``prefix_min_tokens``: the fork / prefill crossover measured on the 40-layer model. Repeated runs put it at 4 or at 8
    # rows (at 4 the gain is below the run-to-run spread): the larger one (profiles/prefix_cache.md, prefix_cache_crossover_runs.md)
    PREFIX_MIN_TOKENS = 8
    PREFIX_HOST_MIN_TOKENS = 8       # default of ``prefix_host_min_tokens`` (profiles/prefix_host.md)

    def __init__(self, llm, input_resampler, output_resampler, lm_loss_scale=1.0, rec_loss_scale=1.0,
                 add_patch_pos=False, vit_down=False, mse=False):
        self.llm = llm
        self.input_resampler = input_resampler
        self.output_resampler = output_resampler
        self.add_patch_pos = add_patch_pos
        self.vit_down = vit_down
        self.patch_pos_embed = None      # host fp32 [4, dim] (seed_x.py:43-45)
        self.device, self.dtype = None, torch.float16
        self.use_graph = True
        self.chunk_forced_image_tokens = True
        self.prefix_cache = False        # generate_inflight: reuse the cache rows of a prompt prefix some slot already holds (opt-in)
        self.prefix_min_tokens = self.PREFIX_MIN_TOKENS   # shortest prefix worth a slot-to-slot copy, or worth waiting one round for
        self.prefix_host_bytes = 0       # generate_inflight: budget of the host-memory tier behind prefix_cache (kvstore.py); 0 = off
        # shortest record worth a spill and shortest host match worth a restore: the restore / prefill crossover measured on the 40-layer
        # model, rounded up to a multiple of 8. The restore wins from the smallest length measured, 8 rows (0.27 against 14.5 ms), on
        # (profiles/prefix_host.md, tools/bench_prefix_host.py)
        self.prefix_host_min_tokens = self.PREFIX_HOST_MIN_TOKENS
        self.speculative = False         # generate_inflight: lossless speculative decoding on an LLM built with spec_tokens > 0 (opt-in)
        self.spec_ngram = (3, 1)         # (longest, shortest) n-gram of its prompt-lookup drafter
        self._conv = {}                  # sequence → (token ids, row fingerprints, LLM cache epoch, adapter name) held by its KV cache
        self._sig_w = {}
        self.last_prefill_tokens = []
        self.last_inflight_stats = None
        self._inflight = None            # buffers + slot state of generate_inflight, kept so that ONE captured step serves every call

    @classmethod
    def from_pretrained(cls, llm, input_resampler, output_resampler, pretrained_model_path=None, **kwargs):
        model = cls(llm=llm, input_resampler=input_resampler, output_resampler=output_resampler, **kwargs)
        if pretrained_model_path is not None:
            ckpt = torch.load(pretrained_model_path, map_location="cpu")   # agent/pytorch_model.bin (:231-233)
            model.load_state_dict(ckpt)
        return model

    def load_state_dict(self, sd, strict=True):
        """Keys: input_resampler.*, output_resampler.*, patch_pos_embed (+ optional llm.* which is ignored here: the
        released checkpoints ship the LLM as a merged HF directory, llm_seed_x_i.yaml)."""
        self.input_resampler.load_state_dict(sd, prefix="input_resampler.", strict=strict)
        self.output_resampler.load_state_dict(sd, prefix="output_resampler.", strict=strict)
        if self.add_patch_pos:
            if "patch_pos_embed" not in sd:
                raise KeyError("ContinuousLVLM: missing key patch_pos_embed")
            self.patch_pos_embed = sd["patch_pos_embed"].detach().float().cpu()
        return [], []

    def to(self, device=None, dtype=None):
        if device is not None:
            self.device = torch.device(device)
        if dtype is not None:
            self.dtype = dtype
        for m in (self.llm, self.input_resampler, self.output_resampler):
            m.to(self.device, self.dtype)
        return self

    def eval(self):
        return self

    # ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _prompt_ids(tokenizer, req):
        """The request's prompt as a list of token ids (host only: what a paged admission sizes its reservation from)."""
        input_ids = req.get("input_ids")
        if req.get("prompt") is not None:
            input_ids = tokenizer(req["prompt"], return_tensors="pt").input_ids
        if isinstance(input_ids, torch.Tensor):
            return input_ids.reshape(-1).tolist()
        return list(input_ids[0]) if len(input_ids) and isinstance(input_ids[0], (list, tuple)) else list(input_ids)

    def _prompt_embeds(self, tokenizer, req):
        """embed_tokens + input resampler + patch-position term + scatter (seed_x.py:154-173) for ONE request."""
        llm = self.llm
        dev, H = llm.device, llm.H
        input_ids = self._prompt_ids(tokenizer, req)
        ids_dev = torch.tensor(input_ids, dtype=torch.int32, device=dev)
        x = ops.embedding(ids_dev, llm._pack()["embed"])                                    # [T, H] fp32 (:158)
        image_embeds = req.get("image_embeds")
        if image_embeds is not None:
            embeds_cmp_mask, ids_cmp_mask = req.get("embeds_cmp_mask"), req.get("ids_cmp_mask")
            assert embeds_cmp_mask is not None and ids_cmp_mask is not None
            lm = self.input_resampler(image_embeds.to(dev))                                 # [n, nq, H] fp32 (:164)
            n, nq, _ = lm.shape
            if self.add_patch_pos:                                                          # :165-171
                patch_positions = req.get("patch_positions")
                assert patch_positions is not None
                pp = patch_positions.detach().float().cpu()
                rel = torch.mm(torch.cat([pp, 1 - pp], dim=-1) / 2, self.patch_pos_embed)   # host glue, [n, H]
                rel = rel.to(dev).unsqueeze(1).expand(n, nq, H).contiguous()
                lm = ops.add(lm.contiguous(), rel)
            sel = torch.nonzero(embeds_cmp_mask.detach().cpu().reshape(-1)).reshape(-1).tolist()
            rows = torch.nonzero(ids_cmp_mask.detach().cpu().reshape(-1)).reshape(-1).to(torch.int32)
            assert rows.numel() == len(sel) * nq, "ids_cmp_mask / embeds_cmp_mask mismatch"
            src = lm if len(sel) == n else lm[torch.tensor(sel, device=dev)]
            ops.scatter_rows(src.reshape(-1, H).contiguous(), rows.to(dev), x)              # :173
        return input_ids, x

    @torch.no_grad()
    def _row_sig(self, x):
        """Per-row fingerprint of prompt embeddings (fp32 [T, H]) used to validate a cached prefix: two independent
        position-weighted sums of the rows' bit patterns (int64 [T, 2]) — a plain sum would not see permuted columns."""
        bits = x.view(torch.int32).to(torch.int64)
        w = self._sig_w.get((x.shape[1], x.device))
        if w is None:
            gen = torch.Generator().manual_seed(0x5EED)
            w = (torch.randint(1, 1 << 20, (x.shape[1], 2), generator=gen, dtype=torch.int64) * 2 + 1).to(x.device)
            self._sig_w[(x.shape[1], x.device)] = w
        return torch.stack([(bits * w[:, 0]).sum(dim=1), (bits * w[:, 1]).sum(dim=1)], dim=1)

    def _reuse_prefix(self, prompts, adapters=None):
        """Cross-turn KV reuse (no reference counterpart: seed_x.py:184-189 re-prefills the whole conversation every turn).
        For sequence g the cache still holds the previous call's prompt + the generated tokens that were fed back. The new
        prompt's longest prefix whose token ids AND embedding rows (image features included) are identical to what produced
        those cache entries is kept; only the rest is prefilled. Returns the prefix length per sequence. KV rows depend on the LoRA
        adapter they were computed under: a sequence whose adapter changed keeps nothing and is prefilled from row 0."""
        starts = []
        for g, (ids, x) in enumerate(prompts):
            prev = self._conv.get(g)
            p = 0
            if prev is not None and prev[2] != self.llm.kv_epoch:
                prev = None                      # the cache was reset / written behind our back (llm.reset, llm.forward, ...)
            if prev is not None and prev[3] != (adapters[g] if adapters is not None else None):
                prev = None                      # the rows were written under another adapter
            if prev is not None:
                old_ids, old_sig = prev[:2]
                m = min(len(old_ids), len(ids) - 1)                                   # >= 1 token must be forwarded
                while p < m and old_ids[p] == ids[p]:
                    p += 1
                if p:
                    same = (self._row_sig(x[:p]) == old_sig[:p]).all(dim=1).to(torch.int32)
                    p = int(torch.cumprod(same, 0).sum().item())
            starts.append(p)
        return starts

    def _remember(self, g, prompt, gen_ids_fed, adapter=None):
        """Records what sequence g's KV cache now holds: the prompt rows and the generated tokens that were fed back."""
        ids, x = prompt
        sig = self._row_sig(x)
        if len(gen_ids_fed):
            P = self.llm._P
            e = ops.embedding(torch.tensor(gen_ids_fed, dtype=torch.int32, device=x.device), P["embed"])
            sig = torch.cat([sig, self._row_sig(e)])
        self._conv[g] = (list(ids) + list(gen_ids_fed), sig, self.llm.kv_epoch, adapter)

    # ---- constrained decoding (grammar.py): what the engines check before anything is touched ------------------------------
    def _grammar_names(self, who, requests, force_flags):
        """The requests' ``"grammar"`` names (None: unconstrained). ValueError for what is not built or not there: tensor-parallel
        ranks, agent.speculative, a model built with max_grammars=0, an unknown name, force_image_at on the same request."""
        llm = self.llm
        names = [req.get("grammar") for req in requests]
        if all(n is None for n in names):
            return names
        world = llm.comm.world if getattr(llm, "comm", None) is not None else 1
        if world > 1:
            raise ValueError(f"{who}: a \"grammar\" on tp={world} tensor-parallel ranks is not built (follow-up: every rank would mask and "
                             "advance on the gathered logits)")
        if who == "generate_inflight" and self.speculative:
            raise ValueError(f"{who}: a \"grammar\" with agent.speculative is not built (follow-up: automaton states that advance with the "
                             "verify step's accepted run); switch agent.speculative off for calls that carry a grammar")
        if not getattr(llm, "max_grammars", 0):
            raise ValueError(f"{who}: a request names the grammar {next(n for n in names if n is not None)!r} but the model was built with "
                             "max_grammars=0 (LlamaForCausalLM(..., max_grammars=N), then llm.load_grammar(name, fsm))")
        for r, n in enumerate(names):
            if n is None:
                continue
            if n not in llm.grammars:
                raise ValueError(f"{who}: request {r} names the unknown grammar {n!r} (resident: {llm.grammars})")
            if force_flags[r]:
                raise ValueError(f"{who}: request {r} carries a grammar and force_image_at: not built (follow-up: the replaced id would "
                                 "have to be an admissible one); drop one of the two")
        return names

    def _grammar_prompts(self, who, tokenizer, requests, names, img_ids):
        """... and what needs the tokenizer: a constrained request may not start inside the image chain (the constrained row skips the
        chain's forcing), and its grammar may not admit the image block."""
        chain = set(img_ids[:-1])
        for r, n in enumerate(names):
            if n is None:
                continue
            last = self._prompt_ids(tokenizer, requests[r])[-1]
            if last in chain:
                raise ValueError(f"{who}: request {r} carries a grammar but its prompt ends inside the image block (id {last}): not built "
                                 "(follow-up: a grammar that starts behind the forced block)")
            fsm = self.llm.grammar(n)
            if (fsm.trans[:, [i for i in img_ids if 0 <= i < fsm.vocab_size]] >= 0).any():
                raise ValueError(f"{who}: grammar {n!r} admits ids of the image block (follow-up); build it with banned_ids = the block "
                                 "(ContinuousLVLM.image_block_ids)")

    # ---- sequence rules (sampling.SeqParams): what the engines check before anything is touched -------------------------------------
    def _seq_params(self, who, requests, force_flags):
        """The requests' SeqParams (``"stop"`` / ``"no_repeat_ngram_size"``; None: the request carries neither). ValueError for malformed
        values and for what is not built: force_image_at on the same request, agent.speculative, tensor-parallel ranks."""
        llm = self.llm
        seqs = [SeqParams.from_request(req) for req in requests]
        if all(q is None for q in seqs):
            return seqs
        for r, q in enumerate(seqs):
            if q is not None and force_flags[r]:
                raise ValueError(f"{who}: request {r} carries stop sequences / no_repeat_ngram_size and force_image_at: not built "
                                 "(follow-up: synthetic-weights pinning beside an id history); drop one of the two")
        if who == "generate_inflight" and self.speculative:
            raise ValueError(f"{who}: stop sequences / no_repeat_ngram_size with agent.speculative are not built (follow-up: a ban and a "
                             "stop match per candidate row of the verify step's accepted run); switch agent.speculative off for calls "
                             "that carry them")
        world = llm.comm.world if getattr(llm, "comm", None) is not None else 1
        if world > 1:
            raise ValueError(f"{who}: stop sequences / no_repeat_ngram_size on tp={world} tensor-parallel ranks are not built (follow-up: "
                             "every rank would ban, append and match on the gathered logits)")
        for q in seqs:
            if q is not None:
                q.check_vocab(llm.V)
        return seqs

    @staticmethod
    def _seq_result(q, matched):
        """A result's ``'seq_rules'`` entry: the values the device used and the index of the stop sequence that ended the request."""
        return dict(q.as_dict(), matched=None if matched is None or int(matched) < 0 else int(matched))

    @classmethod
    def image_block_ids(cls, tokenizer, num_img_gen_tokens=64):
        """The ids of ``<img>``, ``<img_i>`` and ``</img>``: what a grammar's ``banned_ids`` must hold."""
        return cls._special_ids(tokenizer, num_img_gen_tokens, None)[0]

    @staticmethod
    def _grammar_result(fsm, name, generate_ids, eos):
        """``{'name', 'complete'}``: the walk over the generated ids on the host; a trailing EOS is not part of it."""
        ids = [int(t) for t in generate_ids]
        if ids and eos is not None and eos >= 0 and ids[-1] == eos:
            ids = ids[:-1]
        _, used, complete = fsm.walk(ids)
        return {'name': name, 'complete': bool(complete and used == len(ids))}

    @_clears_adapters
    @torch.no_grad()
    def generate_batch(self, tokenizer, requests, num_img_gen_tokens=64, max_new_tokens=120, eos_token_id="auto",
                       force_image_at=None, reuse_cache=False):
        """G = len(requests) = llm.G independent requests decoded in lock step. Each request is a dict with the
        ``generate`` keyword arguments (input_ids | prompt, image_embeds, embeds_cmp_mask, ids_cmp_mask,
        patch_positions). Returns one reference-style result dict per request. A request may also carry ``do_sample``, ``temperature``,
        ``top_k``, ``top_p`` and ``seed`` (sampling.SamplingParams): its tokens — the prefill's first one included, token index 0 —
        are then drawn on the device by the seeded rule of seedx_amd.sampling (sx_sample_next_b) and its result carries ``'seed'``;
        without a sampling request the call runs the greedy path unchanged. Tensor-parallel ranks (each its own process) must be
        given the same explicit ``seed``: ``seed=None`` is refused there (ValueError), since each rank would draw its own.
        ``reuse_cache``: keep each sequence's KV cache across calls and prefill only the part of the new prompt that is not
        already in it (multi-turn conversations; results are identical to a full re-prefill).
        A request may carry ``"adapter": name`` — a LoRA adapter resident on the LLM (``llm.load_adapter``; ValueError for an unknown
        name or an LLM built without ``max_adapters``): its prompt, its forced image chunks and its token steps run under that adapter,
        unmerged, beside requests under other adapters or none; every result carries ``'adapter'``. Without such a request the call
        runs the calls and captured graphs it always ran. ``reuse_cache`` re-prefills a sequence whose adapter changed.
        On a paged KV cache (``LlamaForCausalLM(kv_pages=N)``) every sequence reserves prompt + ``max_new_tokens`` rows up front and a
        ``reuse_cache`` turn extends its reservation; RuntimeError naming the shortfall if the pool is too small.
        A request may carry ``"logprobs": N`` (an int in 0 .. 8; ValueError otherwise, before anything is touched): its result gains
        ``'logprobs'`` = {'token_ids', 'token_logprobs', 'top_ids', 'top_logprobs'}, one record per generated id in generation order —
        the log-probability of the id under the model's RAW distribution (seedx_amd.sampling.token_logprobs: before the image-token
        rule, temperature, top-k and top-p) and the N most likely ids with theirs. The first record comes from the LP lock-step tail on
        the prefill's logits (sx_sample_next_b_lp), the later ones from the LP token step. Ids the model did not choose — the forced image
        ids and ``</img>``, step-wise or as a host-driven chunk, and a ``force_image_at`` replacement — record NaN and top ids -1.
        Without such a request the call runs exactly the path it always ran.
        A request may carry logits controls — ``repetition_penalty``, ``presence_penalty``, ``frequency_penalty``, ``logit_bias``
        ({id: bias}, at most 16, -inf bans the id) and ``min_new_tokens`` (sampling.ControlParams; malformed values are a ValueError
        before anything is touched): they are applied to its logits row on the device inside the tail of the token step, ahead of the
        image-token rule and the arg-max or draw (seedx_amd.sampling.apply_controls states the rule; sx_next_b_ctl), for the prefill's
        first token (index 0) as for every later one, and its result gains ``'controls'``. Log-probabilities stay those of the RAW
        row. Without such a request the call runs the calls and graphs it always ran. ValueError together with ``force_image_at``
        (synthetic-weights pinning: a follow-up) and on tensor-parallel ranks (follow-up: edit and count on the gathered logits).
        A request may carry ``"grammar": name`` — a token automaton resident on the LLM (``llm.load_grammar(name, fsm)``,
        seedx_amd.grammar): its ids are then chosen among those the automaton admits, by a mask applied on the device inside the tail
        of the token step (sx_next_b_fsm: behind the controls, in place of the image-token rule, ahead of the arg-max or draw), for the
        prefill's first token as for every later one; the row is cut at the token on which its walk finishes (a final state, or EOS
        in an accepting one) and its result gains ``'grammar'`` = {'name', 'complete'} — ``complete`` is the host's walk over the
        generated ids (a trailing EOS apart); a budget that runs out mid-grammar gives False. Log-probabilities stay those of the RAW
        row. Without such a request the call runs the calls and graphs it always ran. ValueError, before anything is touched, for a
        model built with max_grammars=0, an unknown name, ``force_image_at`` (follow-up), a prompt that ends inside the image block
        (follow-up), a grammar that admits the image block (follow-up) and tensor-parallel ranks (follow-up).
        A request may carry sequence rules — ``"stop"``: [[ids], ...] (at most 4 sequences of 1 .. 8 token ids; one flat list counts as
        one sequence; strings are refused) and ``"no_repeat_ngram_size"``: n in 0 .. 8 (sampling.SeqParams; malformed values are a
        ValueError before anything is touched). The device keeps the request's id history (prompt ids, then every id it emits) and, inside
        the tail of the token step (sx_next_b_seq: behind the controls, ahead of the grammar mask and the image-token rule), bans every
        id that would repeat an n-gram of it (seedx_amd.sampling.apply_no_repeat, transformers' NoRepeatNGramLogitsProcessor); the row
        is cut at the token on which its generated ids end with a stop sequence (sampling.stop_match; the matched ids stay in the
        result, like the EOS id; a stop sequence that ends on a host-driven image block is tested behind the whole block) and its
        result gains ``'seq_rules'`` = {'stop', 'no_repeat_ngram_size', 'matched'}. Log-probabilities stay those of the RAW row. Without
        such a request the call runs the calls and graphs it always ran. ValueError with ``force_image_at`` (follow-up) and on
        tensor-parallel ranks (follow-up)."""
        llm = self.llm
        gnames = self._grammar_names("generate_batch", requests, [force_image_at is not None] * len(requests))
        constrained = any(n is not None for n in gnames)
        if constrained:
            self._grammar_prompts("generate_batch", tokenizer, requests, gnames, self._special_ids(tokenizer, num_img_gen_tokens, None)[0])
        asks = [logprobs_from_request(req) for req in requests]
        ctls = [ControlParams.from_request(req) for req in requests]
        controlled = any(c is not None for c in ctls)
        if controlled and force_image_at is not None:
            raise ValueError("generate_batch: logits controls together with force_image_at are not built (follow-up: counting the "
                             "replaced id in the lock-step form); drop one of the two")
        seqs = self._seq_params("generate_batch", requests, [force_image_at is not None] * len(requests))
        ruled = any(q is not None for q in seqs)
        params = [SamplingParams.from_request(req, world=llm.comm.world) for req in requests]     # refuses seed=None on tp > 1 ranks
        if controlled:
            if llm.comm.world > 1:
                raise ValueError(f"generate_batch: logits controls on tp={llm.comm.world} tensor-parallel ranks are not built (follow-up: "
                                 "every rank would edit and count on the gathered logits)")
            for c in ctls:
                if c is not None:
                    c.check_vocab(llm.V)
        if any(n is not None for n in asks) and llm.comm.world > 1:
            raise ValueError(f"generate_batch: \"logprobs\" on tp={llm.comm.world} tensor-parallel ranks is not built (follow-up)")
        names = [req.get("adapter") for req in requests]
        for n in names:
            llm._adapter_index(n)                       # unknown name / feature off: ValueError before anything is touched
        dev, H, G = llm.device, llm.H, len(requests)
        P = llm._pack()
        assert G == llm.G, f"the LLM was built for max_batch={llm.G} lock-step sequences, got {G} requests"
        img_ids, boi_id, eoi_id, eos_token_id = self._special_ids(tokenizer, num_img_gen_tokens, eos_token_id)
        img_ids_dev = torch.tensor(img_ids, dtype=torch.int32, device=dev)
        nchunk = num_img_gen_tokens + 1
        rows = 2 * max_new_tokens + nchunk + 8          # finished sequences keep stepping until the slowest one ends
        out_ids = torch.full((G, rows), -1, dtype=torch.int32, device=dev)
        hid = torch.zeros((G, rows, H), dtype=torch.float32, device=dev)                    # row k = state at input new[k-1]

        # ---- prefill every request (ONE batched pass: M = sum of the prompt lengths), first token --------------------
        prompts = [self._prompt_embeds(tokenizer, req) for req in requests]
        ss = None
        if any(p is not None for p in params):          # per-row parameters on the device; greedy rows keep the arg-max
            ss = llm.sample_state()
            ss.set_rows(range(G), params)
        if self._inflight is not None:
            self._inflight["prefix"] = None             # generate_inflight's slot records: this call rewrites the slots
        starts = self._reuse_prefix(prompts, names) if reuse_cache else [0] * G
        if not reuse_cache:
            llm.reset()
            self._conv = {}
        xs, last_ids = [], []
        for g, (input_ids, x) in enumerate(prompts):
            assert len(input_ids) + rows <= llm.Tmax, "KV cache too small for prompt + max_new_tokens"
            if llm.kv_pages:
                # paged cache: prompt + max_new_tokens rows per sequence, up front (the token steps are captured graphs: they reserve
                # nothing); a reuse_cache turn extends what the sequence holds. A sequence that has finished keeps stepping beside the
                # others past its reservation: those appends find no page and write nothing
                llm._kv_need(g, len(input_ids) + max_new_tokens, f"generate_batch, a prompt of {len(input_ids)} rows + max_new_tokens {max_new_tokens}")
            if reuse_cache:
                llm.set_position(g, starts[g])
            xs.append(x[starts[g]:])
            last_ids.append(input_ids[-1])
        P["step"].zero_()
        named = any(n is not None for n in names)
        logits, _ = llm.forward_embeds_batch(xs, list(range(G)), **(dict(adapters=names) if named else {}))
        logits = logits.contiguous()
        if llm.max_adapters:
            llm.set_adapters(range(G), names)           # the per-sequence adapter index the token step reads (-1: none)
        self.last_prefill_tokens = [int(x.shape[0]) for x in xs]
        P["cur"].copy_(torch.tensor(last_ids, dtype=torch.int32))
        lps = None
        if any(n is not None for n in asks):            # the LP tail, here and in every token step; rows that did not ask record nothing
            lps = LogprobState(G, max(n for n in asks if n is not None), dev, rows)
            lps.want.copy_(torch.tensor([int(n is not None) for n in asks], dtype=torch.int32))
        cs, gs, eos_dev = None, None, -1 if eos_token_id is None else int(eos_token_id)
        fsms = [llm.grammar(n) if n is not None else None for n in gnames]
        gstate = [0 if f is not None else DONE for f in fsms]        # host mirror of the automaton states, advanced on the read-back ids
        qs, gen, smatch = None, [[] for _ in range(G)], [None] * G   # host mirror of the generated ids of the rows that carry rules
        if ruled:                                        # the sequence-rule tail, here and in every token step; working rows: the controls'
            cs, qs = llm.control_state(), llm.seq_rule_state()
            cs.set_rows(range(G), ctls, [ids for ids, _ in prompts])
            qs.set_rows(range(G), seqs, [ids for ids, _ in prompts])
            if constrained:
                gs = llm.grammar_state()
                gs.set_rows(range(G), gnames)
            ops.next_b_seq(logits, llm.V, img_ids_dev, P["cur"], out_ids, P["step"], cs, qs, fsm=gs, sample=ss, lp=lps, eos_id=eos_dev)   # token index 0
        elif constrained:                                  # the constrained tail, here and in every token step; its working rows are the controls'
            cs, gs = llm.control_state(), llm.grammar_state()
            cs.set_rows(range(G), ctls, [ids for ids, _ in prompts])
            gs.set_rows(range(G), gnames)
            ops.next_b_fsm(logits, llm.V, img_ids_dev, P["cur"], out_ids, P["step"], cs, gs, sample=ss, lp=lps, eos_id=eos_dev)   # token index 0
        elif controlled:                                   # the controlled tail, here and in every token step; rows without controls run as ever
            cs = llm.control_state()
            cs.set_rows(range(G), ctls, [ids for ids, _ in prompts])
            ops.next_b_ctl(logits, llm.V, img_ids_dev, P["cur"], out_ids, P["step"], cs, sample=ss, lp=lps, eos_id=eos_dev)   # token index 0
        elif lps is not None:
            ops.next_b_lp(logits, llm.V, img_ids_dev, P["cur"], out_ids, P["step"], lps, ss)     # token index 0
        elif ss is not None:
            ops.sample_next_b(logits, llm.V, img_ids_dev, P["cur"], out_ids, P["step"], ss)      # token index 0
        else:
            ops.greedy_next_b(logits, llm.V, img_ids_dev, P["cur"], out_ids, P["step"])
        ops.add_i32(P["step"], 1)
        n_new = [1] * G
        cur = P["cur"].tolist()
        llm.comm.check()

        def force(g):
            # synthetic-weights benchmarking only: random-init weights never emit <img>, so the transcript is pinned by
            # overwriting generated token #force_image_at with <img> AFTER its full forward/lm_head/argmax has run
            # (no work is skipped). Never set with real checkpoints.
            if force_image_at is not None and n_new[g] - 1 == force_image_at:
                P["cur"][g] = boi_id
                out_ids[g, n_new[g] - 1] = boi_id
                cur[g] = boi_id
                if asks[g] is not None:
                    lps.forced(g, n_new[g] - 1, 1)       # the record made there describes the id that was replaced

        def finished(g):
            return n_new[g] >= max_new_tokens or (eos_token_id is not None and cur[g] == eos_token_id) or (fsms[g] is not None and gstate[g] < 0) \
                or smatch[g] is not None

        def walk(g):                                     # the device did the same on the same id (grammar.advance; sampling.stop_match)
            if fsms[g] is not None and gstate[g] >= 0:
                gstate[g] = advance(fsms[g], gstate[g], cur[g], eos_dev)
            if seqs[g] is not None:
                gen[g].append(cur[g])
                smatch[g] = stop_match(gen[g], seqs[g].stop)
        for g in range(G):
            force(g)
            walk(g)
        done = [finished(g) for g in range(G)]
        final_n = [n_new[g] if done[g] else None for g in range(G)]
        # ---- token loop ---------------------------------------------------------------------------------------------
        while not all(done):
            hit = [g for g in range(G) if not done[g] and self.chunk_forced_image_tokens and cur[g] == boi_id
                   and n_new[g] + nchunk <= max_new_tokens]
            if hit:
                self._forced_image_chunk(hit, n_new, img_ids, hid, out_ids, [names[g] for g in hit] if named else None)
                for g in hit:
                    if asks[g] is not None:
                        lps.forced(g, n_new[g], nchunk)
                    if ctls[g] is not None:              # the host emitted these ids: counted like the tail's
                        cs.count([g] * nchunk, img_ids[1:])
                    if seqs[g] is not None:              # ... and go to the id history like the tail's
                        qs.append([(g, len(prompts[g][0]) + n_new[g])], [img_ids[1:]])
                        gen[g] += img_ids[1:]
                        smatch[g] = stop_match(gen[g], seqs[g].stop)
                    n_new[g] += nchunk
                    P["step"][g] = n_new[g]
                    P["cur"][g] = eoi_id
                    cur[g] = eoi_id
                    if finished(g):
                        done[g], final_n[g] = True, n_new[g]
            if all(done):
                break
            llm.decode_step(img_ids_dev, out_ids, hid, use_graph=self.use_graph, sampling=ss,   # one token for every sequence
                            **(dict(logprobs=lps) if lps is not None else {}),
                            **(dict(controls=cs, eos_id=eos_dev) if cs is not None else {}),
                            **(dict(grammar=gs) if gs is not None else {}),
                            **(dict(seq_rules=qs) if qs is not None else {}))
            cur = P["cur"].tolist()                                                          # the only read-back per step
            llm.comm.check()                              # (tensor-parallel only: + 4 bytes) a timed-out collective must not pass
            for g in range(G):
                if done[g]:
                    continue
                n_new[g] += 1
                force(g)
                walk(g)
                if finished(g):
                    done[g], final_n[g] = True, n_new[g]

        results = []
        for g in range(G):
            n = final_n[g]
            generate_ids = out_ids[g, :n].cpu().long()
            if reuse_cache:
                self._remember(g, prompts[g], generate_ids[:n - 1].tolist(), names[g])   # the last new token was never fed
            results.append(self._result(tokenizer, generate_ids, hid[g, 1:n], boi_id, eoi_id, num_img_gen_tokens))
            if params[g] is not None:
                results[-1]['seed'] = params[g].seed
            results[-1]['adapter'] = names[g]
            if asks[g] is not None:
                results[-1]['logprobs'] = logprobs_result(generate_ids, lps.chosen[g, :n].cpu(), lps.top_ids[g, :n].cpu().long(),
                                                          lps.top[g, :n].cpu(), asks[g])
            if ctls[g] is not None:
                results[-1]['controls'] = ctls[g].as_dict()
            if fsms[g] is not None:
                results[-1]['grammar'] = self._grammar_result(fsms[g], gnames[g], generate_ids.tolist(), eos_dev)
            if seqs[g] is not None:
                results[-1]['seq_rules'] = self._seq_result(seqs[g], smatch[g])
        return results

    @staticmethod
    def _special_ids(tokenizer, num_img_gen_tokens, eos_token_id):
        """(img_ids, boi_id, eoi_id, eos): the ids of [<img>, <img_0> …, </img>] (generation.py:15-17), its two ends, and the EOS id
        ("auto" → tokenizer.eos_token_id; None: no EOS stop)."""
        img_ids = tokenizer.encode(''.join([BOI_TOKEN] + [IMG_TOKEN.format(i) for i in range(num_img_gen_tokens)]
                                           + [EOI_TOKEN]), add_special_tokens=False)
        if eos_token_id == "auto":
            eos_token_id = getattr(tokenizer, "eos_token_id", None)
        return img_ids, img_ids[0], img_ids[-1], eos_token_id

    def _forced_image_chunk(self, hit, n_new, img_ids, hid, out_ids, adapters=None):
        """The forced image block of the sequences ``hit`` (their current token is <img>): inputs [<img>, <img_0> … <img_63>] as one
        causal chunk per sequence, all of them in ONE pass; the outputs are forced (generation.py:23-26). Sequence g's hidden states
        and ids [<img_0> …, </img>] go to rows n_new[g] … of ``hid`` / ``out_ids``; the caller advances its counters."""
        llm, dev = self.llm, self.llm.device
        xe = ops.embedding(torch.tensor(img_ids[:-1], dtype=torch.int32, device=dev), llm._P["embed"])
        _, hns = llm.forward_embeds_batch([xe] * len(hit), hit, need_logits=False, **(dict(adapters=adapters) if adapters else {}))
        forced = torch.tensor(img_ids[1:], dtype=torch.int32, device=dev)
        for g, hn in zip(hit, hns):
            hid[g, n_new[g]:n_new[g] + len(img_ids) - 1] = hn                                # plumbing copy
            out_ids[g, n_new[g]:n_new[g] + len(img_ids) - 1] = forced

    def _result(self, tokenizer, generate_ids, last_hidden, boi_id, eoi_id, num_img_gen_tokens):
        """The reference-style result dict of one finished request (seed_x.py:196-234; last_hidden: :196-197)."""
        eoi_indices = torch.where(generate_ids == eoi_id)[0].tolist()                        # :199
        text_mask = torch.ones_like(generate_ids, dtype=torch.bool)
        img_gen_feat = None
        if eoi_indices:
            feats = []
            for e in eoi_indices:
                feats.append(last_hidden[e - num_img_gen_tokens:e])                          # :204
                text_mask[e - num_img_gen_tokens:e] = False
            img_gen_feat = self.output_resampler(torch.stack(feats))                         # :209-210
            img_gen_feat = ops.cast(img_gen_feat.contiguous(), self.dtype)
        text_mask[generate_ids == boi_id] = False
        text = tokenizer.decode(generate_ids[text_mask], skip_special_tokens=False)          # :214-216
        return {'text': text, 'has_img_output': len(eoi_indices) > 0, 'img_gen_feat': img_gen_feat,
                'num_gen_imgs': len(eoi_indices), 'generate_ids': generate_ids, 'last_hidden_states': last_hidden}

    @_clears_adapters
    @torch.no_grad()
    def generate_inflight(self, tokenizer, requests, num_img_gen_tokens=64, max_new_tokens=120, eos_token_id="auto",
                          max_admit=None, on_result=None):
        """In-flight (continuous) batching: any number of requests >= 1 on the llm.G slots of the lock-step decode step. The request
        dicts are generate_batch's; each may carry its own ``max_new_tokens`` and ``force_image_at``. The stop rule (EOS or budget)
        runs on the device at the end of the captured token step (sx_greedy_next_slots): a finished slot parks itself, writes
        nothing while it idles, and is refilled from the queue head before the next step — at most ``max_admit`` requests per
        admission pass (None: every free slot), each round of a pass ONE batched prefill. The host reads one [G, 4] status tensor
        per step. Returns one reference-style result dict per request, in request order; ``on_result(index, result)`` is called as
        each request finishes; ``last_inflight_stats`` holds the step counts (inflight.simulate predicts them from the lengths).
        Requests may carry ``do_sample``, ``temperature``, ``top_k``, ``top_p`` and ``seed`` as in generate_batch: a queue with at least
        one such request runs the sampled token step (sx_sample_next_slots: same stop rule, the parameters are read per slot from
        device memory, greedy requests keep the arg-max); a queue without one runs the greedy step as before. A request's ids depend
        on its own logits, parameters, seed and token indices only — never on its slot or its neighbours.
        A request may carry ``"adapter": name`` as in generate_batch (ValueError for an unknown name): the slot's adapter index
        (``SlotState.adapter``) is written at its admission and goes back to -1 when the slot parks, its prefill, forced chunks and
        token steps run under the adapter, and a queue may mix adapters and none; a step in which no live slot has an adapter is the
        step of a queue without adapters. With ``prefix_cache`` the adapter rides in every row's signature (inflight.tag_signatures):
        prefixes are kept and forked only among requests of the same adapter. Results carry ``'adapter'``.
        Forced image blocks stay host-driven chunks as in generate_batch (the other slots wait). Slots are reused without zeroing:
        keys at or above ``pos`` are never visible. generate_batch's cross-turn records (``reuse_cache``) are cleared by this call.
        Prefix reuse is switched on the engine, like ``use_graph``: ``agent.prefix_cache = True`` (off by default: the call then takes
        the lowest free slot and prefills every prompt from row 0, as ever) and ``agent.prefix_min_tokens``. With it the engine
        remembers what each slot's cache holds — token ids and ``_row_sig`` fingerprints of the prompt rows, image rows included, and of
        the generated tokens that were fed back — across admissions AND across calls. The records are validated by
        ``llm.kv_epoch``: ``llm.forward``, ``forward_embeds``, ``reset`` and ``park_slots`` move it and so end the records, and
        generate_batch drops them itself. ``llm.forward_embeds_batch``, ``decode_step`` and ``set_position`` do NOT move the epoch (the
        engines are built from them): whoever calls those directly between two cached calls must ``llm.reset()`` afterwards. An admitted request
        whose prompt starts like a record keeps those rows where the slot is free, or has them copied from the live or just-claimed
        donor slot (>= ``prefix_min_tokens`` rows; ops.kv_fork: one launch per cache tensor and round, issued before the round's
        prefill), and prefills only its suffix; requests that share a prefix with an earlier request of their own round (one prompt
        under several seeds) wait one round and fork from it (inflight.plan_admission states the rules). Which requests a pass
        admits does not change, so the step counts stay inflight.simulate's; ``last_prefill_tokens`` lists the suffix lengths and
        ``last_inflight_stats`` also counts prefix_hit_tokens, forked_tokens and fork_launches (inflight.simulate_prefix predicts them).
        Reused rows are the rows an earlier pass wrote: results agree with the uncached call like generate_batch's ``reuse_cache``
        (identical ids, states within the prefill-shape rounding).
        The records are only as large as the slots: a free slot is the victim of the next unrelated request. ``agent.prefix_host_bytes
        = N`` > 0 (0, the default: nothing is allocated, launched or counted differently; needs ``prefix_cache``, ValueError otherwise
        and for a negative value, before anything is touched) adds a host-memory tier of N bytes behind them (kvstore.py). Behind
        ``plan_admission`` every round runs spill → restore → fork → suffix prefill: a planned slot whose record holds more rows than
        the request keeps there is SPILLED if the store wants it (>= ``agent.prefix_host_min_tokens`` rows, not covered by a stored
        entry, within the budget) — one sx_kv_rows_copy launch packs the rows of every layer, head and cache tensor into a staging
        buffer on this stream, a side stream copies them to pinned host memory — and a planned request whose longest host match has
        >= ``prefix_host_min_tokens`` rows and more than the device gave it is RESTORED: host → staging → one unpack launch into its
        slot, synchronously, and only the rest is prefilled. Least recently used entries are evicted under the budget; a hit never
        depends on timing (it waits for the entry's copy). The store belongs to this pack (it goes when the pack or the special ids
        change) and survives ``llm.reset()``, ``kv_epoch`` changes and outside writes: host copies are immutable. Works with every
        contiguous cache form (fp32, mixed, 16-bit, FP8 codes + scales), adapters (tagged signatures) and ``agent.speculative``;
        ``last_inflight_stats`` gains host_spills, host_spill_tokens, host_restores, host_restore_tokens, host_evictions and
        host_bytes_peak (inflight.simulate_prefix(host_bytes=...) predicts them). Only free slots are spilled (no preemption).
        Speculative decoding is switched on the engine too: ``agent.speculative = True`` (off by default) with an LLM built with
        ``spec_tokens=K`` runs the verify step (``llm.decode_step(..., spec=True)``) instead of the plain slot step: every live slot
        feeds its current token and up to K ids drafted from its own history by prompt lookup (``agent.spec_ngram``) and keeps the
        longest prefix the model itself would have produced (spec.py), so a step emits 1 .. K + 1 tokens per slot and the ids are those
        of the call without the switch, for greedy and for sampled requests. The engine writes the prompt's ids (and a forced image
        block's) to the LLM's id history at admission and still reads one [G, 4] status per step; ``last_inflight_stats`` gains
        spec_steps and spec_emitted_tokens (inflight.simulate_spec predicts the step count from the per-step emitted counts).
        On a paged KV cache (``LlamaForCausalLM(kv_pages=N)``) a request is admitted only if the pages for its prompt + budget are free
        and holds them until it finishes; otherwise the queue head waits for a finishing slot's pages and nothing overtakes it, so
        admission stays deterministic (with an ample pool it is exactly the admission above). A request that can never fit — more pages
        than the pool has, or more rows than ``max_cache_len`` — raises ValueError before anything is touched.
        ``last_inflight_stats`` gains page_waits and peak_pages (inflight.simulate_paged predicts them and the step counts).
        ``prefix_cache`` raises ValueError there: prefix reuse on pages means sharing pages by reference, a follow-up.
        A request may carry ``"logprobs": N`` as in generate_batch (same result entry, same NaN / -1 convention for forced ids): a queue
        with at least one such request runs the LP token step on a slot state of its own (``want`` is written per slot at admission;
        slots whose request did not ask record nothing), a queue without one takes the states and graphs it always took. A request's
        records depend on its own logits only — never on its slot, its neighbours or the largest N in the queue. With
        ``agent.speculative`` a logprob request raises ValueError (follow-up).
        A request may carry logits controls as in generate_batch (``repetition_penalty``, ``presence_penalty``, ``frequency_penalty``,
        ``logit_bias``, ``min_new_tokens``; its result gains ``'controls'``): a queue with at least one such request runs the
        controlled token step (sx_next_slots_ctl) on a slot state of its own — parameters, prompt marks and zeroed counts are written
        per slot at admission, slots whose request carries none run as ever — and a queue without one takes the states and graphs it
        always took. The ids depend on the request alone, never on its slot or its neighbours. ValueError with ``agent.speculative``
        (follow-up: counts that advance with the accepted run) and with ``force_image_at`` on the same request (follow-up).
        A request may carry ``"grammar": name`` as in generate_batch (its result gains ``'grammar'``): a queue with at least one such
        request runs the constrained token step (sx_next_slots_fsm) on a slot state of its own — table index and state 0 are written
        per slot at admission, the device advances the state, and a slot whose automaton finishes parks itself like one that met EOS
        — and a queue without one takes the states and graphs it always took. The ids depend on the request alone. The refusals are
        generate_batch's, plus ``agent.speculative`` (follow-up).
        A request may carry ``"stop"`` / ``"no_repeat_ngram_size"`` as in generate_batch (its result gains ``'seq_rules'``): a queue with
        at least one such request runs the sequence-rule token step (sx_next_slots_seq) on a slot state of its own — the rules and the
        prompt's ids (image placeholders included) are written per slot at admission, the device appends every id it emits, bans
        the ids that would repeat an n-gram, and a slot whose generated ids end with one of its stop sequences parks itself like one
        that met EOS, so its slot and its pages are free for the next request at once; ``matched`` is read once per finished slot —
        and a queue without one takes the states and graphs it always took. The ids depend on the request alone. ValueError with
        ``agent.speculative`` and with ``force_image_at`` on the same request (follow-ups)."""
        llm = self.llm
        requests = list(requests)
        host_bytes, host_min_tokens = self.prefix_host_bytes, self.prefix_host_min_tokens
        if isinstance(host_bytes, bool) or not isinstance(host_bytes, int) or host_bytes < 0:
            raise ValueError(f"generate_inflight: agent.prefix_host_bytes must be an int >= 0 (0: the host tier is off), got {host_bytes!r}")
        if host_bytes and not self.prefix_cache:
            raise ValueError("generate_inflight: agent.prefix_host_bytes needs agent.prefix_cache = True (the host tier spills and restores "
                             "the records of the prefix cache)")
        if host_bytes and (isinstance(host_min_tokens, bool) or not isinstance(host_min_tokens, int) or host_min_tokens < 1):
            raise ValueError(f"generate_inflight: agent.prefix_host_min_tokens must be an int >= 1, got {host_min_tokens!r}")
        gnames = self._grammar_names("generate_inflight", requests, [req.get("force_image_at") is not None for req in requests])
        constrained = any(n is not None for n in gnames)
        if constrained:
            self._grammar_prompts("generate_inflight", tokenizer, requests, gnames, self._special_ids(tokenizer, num_img_gen_tokens, None)[0])
        asks = [logprobs_from_request(req) for req in requests]
        ctls = [ControlParams.from_request(req) for req in requests]
        controlled = any(c is not None for c in ctls)
        if controlled and self.speculative:
            raise ValueError("generate_inflight: logits controls with agent.speculative are not built (follow-up: counts that advance with "
                             "the verify step's accepted run); switch agent.speculative off for calls that carry controls")
        for r, (c, req) in enumerate(zip(ctls, requests)):
            if c is not None and req.get("force_image_at") is not None:
                raise ValueError(f"generate_inflight: request {r} carries logits controls and force_image_at: not built (follow-up); drop "
                                 "one of the two")
        seqs = self._seq_params("generate_inflight", requests, [req.get("force_image_at") is not None for req in requests])
        ruled = any(q is not None for q in seqs)
        if controlled and llm.comm.world > 1:
            raise ValueError(f"generate_inflight: logits controls on tp={llm.comm.world} tensor-parallel ranks are not built (follow-up)")
        for c in ctls:
            if c is not None:
                c.check_vocab(llm.V)
        if llm.comm.world > 1:
            raise NotImplementedError("generate_inflight is single-rank: tensor-parallel ranks are not supported")
        n_top = max([n for n in asks if n is not None], default=None)
        if n_top is not None and self.speculative:
            raise ValueError("generate_inflight: \"logprobs\" with agent.speculative is not built (follow-up: records from the verify "
                             "step's candidate rows); switch agent.speculative off for calls that ask for log-probabilities")
        prefix_cache, prefix_min_tokens = bool(self.prefix_cache), int(self.prefix_min_tokens)
        paged = bool(llm.kv_pages)
        if paged and prefix_cache:
            raise ValueError("generate_inflight: agent.prefix_cache and a paged KV cache (kv_pages) exclude each other for now (follow-up: "
                             "prefix reuse by sharing pages by reference in place of sx_kv_fork copies)")
        spec = bool(self.speculative) and llm.spec_tokens > 0
        K = llm.spec_tokens if spec else 0            # extra rows a verify step may write past a slot's last token
        requests = list(requests)
        N = len(requests)
        assert N >= 1, "generate_inflight needs at least one request"
        dev, H, G = llm.device, llm.H, llm.G
        P = llm._pack()
        img_ids, boi_id, eoi_id, eos_token_id = self._special_ids(tokenizer, num_img_gen_tokens, eos_token_id)
        eos = -1 if eos_token_id is None else int(eos_token_id)
        fsms = [llm.grammar(n) if n is not None else None for n in gnames]
        nchunk = num_img_gen_tokens + 1
        budget = [int(req.get("max_new_tokens") or max_new_tokens) for req in requests]
        force_at = [-1 if req.get("force_image_at") is None else int(req["force_image_at"]) for req in requests]
        params = [SamplingParams.from_request(req) for req in requests]
        names = [req.get("adapter") for req in requests]
        for nm in names:
            llm._adapter_index(nm)                      # unknown name / feature off: ValueError before anything is touched
        named = any(nm is not None for nm in names)
        sampled = any(p is not None for p in params)
        assert all(b >= 1 for b in budget)
        need = None
        if paged:
            # rows each request reserves at admission: prompt + budget. Sized from the token ids alone, before anything is touched
            from .paging import pages_for
            need = [len(self._prompt_ids(tokenizer, req)) + b for req, b in zip(requests, budget)]
            for r, n in enumerate(need):
                if n > llm.Tmax or pages_for(n, llm.kv_page_size) > llm.kv_pages:
                    raise ValueError(f"generate_inflight: request {r} needs {n} cache rows (prompt + max_new_tokens) = "
                                     f"{pages_for(n, llm.kv_page_size)} pages of {llm.kv_page_size} rows; the pool holds {llm.kv_pages} pages and "
                                     f"a slot at most max_cache_len = {llm.Tmax} rows: it can never be admitted")
        rows = max(budget) + 8 + K
        keep = self._inflight
        if keep is None or keep["key"] != (tuple(img_ids), eos, G, id(P)) or keep["out_ids"].shape[1] < rows:
            same = keep is not None and keep["key"] == (tuple(img_ids), eos, G, id(P))
            keep = self._inflight = dict(
                host=keep.get("host") if same else None,        # the host tier's store belongs to the pack: another pack, another store
                key=(tuple(img_ids), eos, G, id(P)),
                img_ids_dev=torch.tensor(img_ids, dtype=torch.int32, device=dev),
                out_ids=torch.full((G, rows), -1, dtype=torch.int32, device=dev),
                hid=torch.zeros((G, rows, H), dtype=torch.float32, device=dev),              # row k = state at input new[k-1]
                state=None, state_sampled=None,
                prefix=keep["prefix"] if keep is not None and keep["key"] == (tuple(img_ids), eos, G, id(P)) else None)
        index = None
        if prefix_cache:                                 # what each slot's cache holds; lives next to the buffers, across calls
            index = keep["prefix"] = keep["prefix"] or PrefixIndex(G)
        store = mover = None
        if host_bytes:                                   # the host tier: the store and its staging buffers live next to the records
            from .kvstore import HostPrefixStore, KVMover, plan_host_tier
            if keep.get("host") is None:
                keep["host"] = (HostPrefixStore(host_bytes, host_min_tokens, llm.kv_row_bytes), KVMover(P))
            store, mover = keep["host"]
            store.budget, store.min_tokens = host_bytes, host_min_tokens       # (a smaller budget takes effect at the next spill)
            evicted0, store.peak = store.evictions, store.bytes

        def owned(fn, *a):
            # a step of this call that moves kv_epoch without touching a recorded row: the records move with it. A write from outside
            # moves the epoch alone, and the records made under the old one never match again
            e0 = llm.kv_epoch
            out = fn(*a)
            if index is not None:
                index.restamp(e0, llm.kv_epoch)
            return out

        owned(llm.reset)                                 # bumps kv_epoch: the cross-turn records no longer describe the cache
        self._conv = {}
        which = "state_sampled" if sampled else "state"        # two slot states, two captured steps: neither disturbs the other
        if n_top is not None:                                  # ... and one more pair per n_top for the LP step
            which += f"_lp{n_top}"
        if controlled:                                         # ... and one more of each for the controlled step
            which += "_ctl"
        if constrained:                                        # ... and for the constrained step
            which += "_fsm"
        if ruled:                                              # ... and for the sequence-rule step
            which += "_seq"
        if keep.get(which) is None:
            keep[which] = owned(lambda: llm.slot_state(force_id=boi_id, eos_id=eos, sampling=sampled, logprobs=n_top,
                                                       **(dict(controls=True) if controlled else {}),
                                                       **(dict(grammar=True) if constrained else {}),
                                                       **(dict(seq_rules=True) if ruled else {})))
        st, img_ids_dev, out_ids, hid = keep[which], keep["img_ids_dev"], keep["out_ids"], keep["hid"]
        lps = st.logprobs
        cs = st.controls
        gs = st.grammar
        qs = st.seq_rules
        gen, smatch, qlen = [[] for _ in range(G)], [None] * G, [0] * G    # host mirrors of the ruled slots: generated ids, match, prompt rows
        if qs is not None:
            qs.on.zero_()
        gfin = set()                                     # slots whose automaton finished on the prefill's first token
        if gs is not None:
            gs.table.fill_(-1)
            gs.state.fill_(DONE)
        if cs is not None:
            cs.on.zero_()
        if lps is not None:
            lps.bind(out_ids.shape[1]).want.zero_()
        owned(llm.park_slots, range(G), st)
        sched = SlotScheduler(G, N, max_admit)
        results = [None] * N
        n_new, cur = [0] * G, [0] * G                    # host mirrors of the live slots' state
        plen = [0] * G                                   # speculative: prompt rows of the slot's request (cur sits at plen + n_new - 1)
        stats = dict(decode_steps=0, live_slot_steps=0, parked_slot_steps=0, admissions=0, prefill_passes=0, prefill_tokens=0)
        if spec:
            stats.update(spec_steps=0, spec_emitted_tokens=0)
            llm.spec_ngram = (int(self.spec_ngram[0]), int(self.spec_ngram[1]))
            self.last_spec_emitted = [[] for _ in range(N)]      # per request: tokens emitted by each verify step it was live in
        if prefix_cache:
            stats.update(prefix_hit_tokens=0, forked_tokens=0, fork_launches=0)
        if store is not None:
            stats.update(host_spills=0, host_spill_tokens=0, host_restores=0, host_restore_tokens=0, host_evictions=0, host_bytes_peak=0)
        if paged:
            stats.update(page_waits=0, peak_pages=0)
            llm._pool.peak = llm._pool.used             # (0: the reset above released every sequence)
        fits = (lambda g, r: llm.kv_reserve(g, need[r])) if paged else None
        self.last_prefill_tokens = []
        prompts, held = {}, {}                           # prefix_cache: request -> (ids, x, row signatures); slot -> (ids, signatures)

        def sigs_of(x, adapter=None):
            # KV rows depend on the adapter that computed them: its name rides in every row's signature (inflight.tag_signatures)
            return tag_signatures([tuple(s) for s in self._row_sig(x).tolist()], adapter)

        def harvest(g, n):
            r = sched.finish(g)
            if paged:                                    # the request's pages go back to the pool (a slot the host parked gave them back already)
                llm.kv_release(g)
            generate_ids = out_ids[g, :n].cpu().long()
            if index is not None:                        # the slot now holds its prompt and the generated ids that were fed back
                ids, sig = held.pop(g)
                fed = generate_ids[:n - 1].tolist()
                if fed:
                    sig = sig + sigs_of(ops.embedding(torch.tensor(fed, dtype=torch.int32, device=dev), P["embed"]), names[r])
                index.record(g, ids + fed, sig, llm.kv_epoch)
            last_hidden = hid[g, 1:n].clone()                                                # the slot's rows are reused
            results[r] = self._result(tokenizer, generate_ids, last_hidden, boi_id, eoi_id, num_img_gen_tokens)
            if params[r] is not None:
                results[r]['seed'] = params[r].seed
            results[r]['adapter'] = names[r]
            if asks[r] is not None:
                results[r]['logprobs'] = logprobs_result(generate_ids, lps.chosen[g, :n].cpu(), lps.top_ids[g, :n].cpu().long(),
                                                         lps.top[g, :n].cpu(), asks[r])
            if ctls[r] is not None:
                results[r]['controls'] = ctls[r].as_dict()
            if fsms[r] is not None:
                results[r]['grammar'] = self._grammar_result(fsms[r], gnames[r], generate_ids.tolist(), eos)
            if seqs[r] is not None:                      # a slot the device parked on a stop sequence: one read per finished slot
                results[r]['seq_rules'] = self._seq_result(seqs[r], smatch[g] if smatch[g] is not None else qs.matched[g].item())
            gfin.discard(g)
            if on_result is not None:
                on_result(r, results[r])

        def stopped(g):
            return n_new[g] >= budget[sched.slot_req[g]] or (eos >= 0 and cur[g] == eos) or g in gfin or smatch[g] is not None

        def admit_round(adm, starts=None):
            # ONE batched prefill over the admitted slots; token 1 of each comes from it (host-side stop test: not in the graph).
            # ``starts`` (prefix_cache): rows [0, starts[i]) of slot i's prompt are in its cache already, the rest is forwarded
            slots = [g for g, _ in adm]
            xs, last_ids, pids = [], [], []
            for i, (g, r) in enumerate(adm):
                ids, x = prompts.pop(r)[:2] if starts is not None else self._prompt_embeds(tokenizer, requests[r])
                assert len(ids) + budget[r] + K <= llm.Tmax, "KV cache too small for prompt + max_new_tokens (+ spec_tokens draft rows)"
                xs.append(x if starts is None else x[starts[i]:])
                last_ids.append(ids[-1])
                pids.append(ids)
                if spec:                                 # the drafter's history: the prompt's ids by cache position (image rows: placeholders)
                    plen[g] = len(ids)
                    llm.spec_write_history(g, 0, ids)
            llm._slot_write(P["pos"], slots, 0 if starts is None else list(starts))
            llm._slot_write(P["ctx"], slots, 1 if starts is None else [s + 1 for s in starts])
            adn = [names[r] for _, r in adm]
            logits, _ = llm.forward_embeds_batch(xs, slots, **(dict(adapters=adn) if any(nm is not None for nm in adn) else {}))
            if llm.max_adapters:
                llm.set_adapters(slots, adn)             # admission: the slot's adapter index (SlotState.adapter), -1 = none
            if starts is not None:                       # the slots hold their prompts now
                for g in slots:
                    index.record(g, held[g][0], held[g][1], llm.kv_epoch)
            first = torch.tensor(last_ids, dtype=torch.int32, device=dev)
            if sampled:                                  # the slots take their requests' parameters; token index 0 is drawn here
                st.sampling.set_rows(slots, [params[r] for _, r in adm])
            if cs is not None:                           # the slots take their requests' controls: parameters, prompt marks, zero counts
                cs.set_rows(slots, [ctls[r] for _, r in adm], pids)
            part = None
            if gs is not None:                           # the slots take their requests' grammars: table index, state 0
                gs.set_rows(slots, [gnames[r] for _, r in adm])
                part = gs.gather(slots)
            qpart = None
            if qs is not None:                           # the slots take their requests' rules and their prompts' ids
                qs.set_rows(slots, [seqs[r] for _, r in adm], pids)
                qpart = qs.gather(slots)
            if lps is not None:                          # the first record: the LP lock-step tail on the prefill's logits, one row per slot
                wants = [int(asks[r] is not None) for _, r in adm]
                llm._slot_write(lps.want, slots, wants)
                rec = LogprobState(len(slots), n_top, dev, rows=1)
                rec.want.copy_(torch.tensor(wants, dtype=torch.int32))
                zero = torch.zeros(len(slots), dtype=torch.int32, device=dev)
                if qs is not None:                       # ... of the raw row, the id from the row the rules (and a grammar) edited
                    ops.next_b_seq(logits.contiguous(), llm.V, img_ids_dev, first, None, zero, cs.gather(slots), qpart, fsm=part,
                                   sample=st.sampling.gather(slots) if sampled else None, lp=rec, token_index=zero, eos_id=eos)
                elif gs is not None:                     # ... of the raw row, the id from the constrained one
                    ops.next_b_fsm(logits.contiguous(), llm.V, img_ids_dev, first, None, zero, cs.gather(slots), part,
                                   sample=st.sampling.gather(slots) if sampled else None, lp=rec, token_index=zero, eos_id=eos)
                elif cs is not None:                     # ... of the raw row, the id from the controlled one
                    ops.next_b_ctl(logits.contiguous(), llm.V, img_ids_dev, first, None, zero, cs.gather(slots),
                                   sample=st.sampling.gather(slots) if sampled else None, lp=rec, token_index=zero, eos_id=eos)
                else:
                    ops.next_b_lp(logits.contiguous(), llm.V, img_ids_dev, first, None, zero, rec,
                                  st.sampling.gather(slots) if sampled else None, token_index=zero)
                at = torch.tensor(slots, device=dev)
                lps.chosen[at, 0], lps.top_ids[at, 0], lps.top[at, 0] = rec.chosen[:, 0], rec.top_ids[:, 0], rec.top[:, 0]
                for i, (g, r) in enumerate(adm):
                    if force_at[r] == 0 and wants[i]:
                        lps.forced(g, 0, 1)              # (synthetic weights) the id is replaced below: the model did not choose it
            elif qs is not None:                         # token index 0 through sx_next_b_seq, like every later one
                zero = torch.zeros(len(slots), dtype=torch.int32, device=dev)
                ops.next_b_seq(logits.contiguous(), llm.V, img_ids_dev, first, None, zero, cs.gather(slots), qpart, fsm=part,
                               sample=st.sampling.gather(slots) if sampled else None, token_index=zero, eos_id=eos)
            elif gs is not None:                         # token index 0 through sx_next_b_fsm, like every later one
                zero = torch.zeros(len(slots), dtype=torch.int32, device=dev)
                ops.next_b_fsm(logits.contiguous(), llm.V, img_ids_dev, first, None, zero, cs.gather(slots), part,
                               sample=st.sampling.gather(slots) if sampled else None, token_index=zero, eos_id=eos)
            elif cs is not None:                         # token index 0 by the same rule, on a copy of the slots' rows of the state
                zero = torch.zeros(len(slots), dtype=torch.int32, device=dev)
                ops.next_b_ctl(logits.contiguous(), llm.V, img_ids_dev, first, None, zero, cs.gather(slots),
                               sample=st.sampling.gather(slots) if sampled else None, token_index=zero, eos_id=eos)
            elif sampled:
                ops.sample_next_b(logits.contiguous(), llm.V, img_ids_dev, first, None, None, st.sampling.gather(slots),
                                  token_index=torch.zeros(len(slots), dtype=torch.int32, device=dev))
            else:
                ops.greedy_next_b(logits.contiguous(), llm.V, img_ids_dev, first, None, None)
            first = first.tolist()
            if gs is not None:                           # the advanced states go to the slots; an automaton may be done already
                gs.scatter(slots, part)
                gfin.update(g for (g, r), s in zip(adm, part.state.tolist()) if fsms[r] is not None and s < 0)
            llm.comm.check()
            stats["admissions"] += len(adm)
            stats["prefill_passes"] += 1
            stats["prefill_tokens"] += sum(int(x.shape[0]) for x in xs)
            self.last_prefill_tokens += [int(x.shape[0]) for x in xs]
            for i, (g, r) in enumerate(adm):
                cur[g] = boi_id if force_at[r] == 0 else first[i]      # (synthetic weights: the pinned transcript, see generate_batch)
                n_new[g] = 1
                gen[g], smatch[g], qlen[g] = [], None, len(pids[i])
                if seqs[r] is not None:                  # the first id in the real history (the tail above appended to the copy)
                    qs.append([(g, qlen[g])], [[cur[g]]])
                    gen[g] = [cur[g]]
                    smatch[g] = stop_match(gen[g], seqs[r].stop)
            out_ids[torch.tensor(slots, device=dev), 0] = torch.tensor([cur[g] for g in slots], dtype=torch.int32, device=dev)
            llm._slot_write(P["cur"], slots, [cur[g] for g in slots])
            if cs is not None:                           # the first id in the real table (the tail above counted into the copy)
                own = [g for g, r in adm if ctls[r] is not None]
                cs.count(own, [cur[g] for g in own])
            if spec:
                for g in slots:
                    llm.spec_write_history(g, plen[g], [cur[g]])
            llm._slot_write(P["step"], slots, 1)
            llm._slot_write(st.n_new, slots, 1)
            llm._slot_write(st.max_new, slots, [budget[r] for _, r in adm])
            llm._slot_write(st.force_at, slots, [force_at[r] for _, r in adm])
            llm._slot_write(st.live, slots, 1)
            fin = [g for g in slots if stopped(g)]
            if fin:
                owned(llm.park_slots, fin, st)
                for g in fin:
                    harvest(g, n_new[g])

        def admit_round_prefix(cand):
            # plan → (host tier: spill → restore) → fork → suffix prefill. The forks of a round are issued before its prefill: a donor's
            # rows are read as they were; so are the packs of the records the round is about to overwrite
            for r in cand:
                if r not in prompts:                     # (a deferred request keeps its embeddings for the next round)
                    ids, x = self._prompt_embeds(tokenizer, requests[r])
                    prompts[r] = (ids, x, sigs_of(x, names[r]))
            plan, _ = plan_admission(index, sched.free_slots(), sched.live_slots(), [(r, prompts[r][0], prompts[r][2]) for r in cand],
                                     prefix_min_tokens, llm.kv_epoch)
            if store is not None:
                plan, spills, restores = plan_host_tier(store, index, plan, {r: (prompts[r][0], prompts[r][2]) for r in cand},
                                                        llm.kv_epoch, host_min_tokens)
                mover.spill(spills)                      # packed on this stream, ahead of everything that rewrites the rows
                mover.restore(restores)
                stats["host_spills"] += len(spills)
                stats["host_spill_tokens"] += sum(e.n_rows for _, e in spills)
                stats["host_restores"] += len(restores)
                stats["host_restore_tokens"] += sum(p for _, _, p in restores)
            forks =[(d, g, start) for g, _, start, d in plan if d is not None]
            if forks:
                ops.kv_fork(P, forks)
                stats["fork_launches"] += 1
                for d, _, _ in forks:
                    index.touch(d)
            for g, r, start, d in plan:
                sched.place(g, r)
                held[g] = (list(prompts[r][0]), prompts[r][2])
                index.invalidate(g)                      # rows [start, ...) are about to be rewritten: recorded again after the prefill
                stats["prefix_hit_tokens"] += start
                stats["forked_tokens"] += start if d is not None else 0
            admit_round([(g, r) for g, r, _, _ in plan], [start for _, _, start, _ in plan])

        while not sched.done:
            sched.new_pass()
            while True:
                adm = sched.candidates() if prefix_cache else sched.admit(fits)
                if not adm:
                    if paged:                            # the queue head waits for pages although a slot is free
                        stats["page_waits"] += bool(sched.queue and sched.quota > 0 and sched.free_slots())
                    break
                if prefix_cache:
                    admit_round_prefix(adm)
                else:
                    admit_round(adm)
            live = sched.live_slots()
            hit = [g for g in live if self.chunk_forced_image_tokens and cur[g] == boi_id
                   and n_new[g] + nchunk <= budget[sched.slot_req[g]]]
            if hit:
                self._forced_image_chunk(hit, n_new, img_ids, hid, out_ids,                 # the other slots wait, as in generate_batch
                                         [names[sched.slot_req[g]] for g in hit] if named else None)
                for g in hit:
                    if asks[sched.slot_req[g]] is not None:
                        lps.forced(g, n_new[g], nchunk)
                    if ctls[sched.slot_req[g]] is not None:      # the host emitted these ids: counted like the tail's
                        cs.count([g] * nchunk, img_ids[1:])
                    if seqs[sched.slot_req[g]] is not None:      # ... and go to the id history like the tail's
                        qs.append([(g, qlen[g] + n_new[g])], [img_ids[1:]])
                        gen[g] += img_ids[1:]
                        smatch[g] = stop_match(gen[g], seqs[sched.slot_req[g]].stop)
                    if spec:                             # the block's ids at the positions they were fed (</img> is the new current token)
                        llm.spec_write_history(g, plen[g] + n_new[g] - 1, img_ids)
                    n_new[g] += nchunk
                    cur[g] = eoi_id
                if spec:
                    llm._slot_write(P["spec"]["n_draft"], hit, 0)
                llm._slot_write(st.n_new, hit, [n_new[g] for g in hit])
                llm._slot_write(P["step"], hit, [n_new[g] for g in hit])
                llm._slot_write(P["cur"], hit, eoi_id)
                fin = [g for g in hit if stopped(g)]
                if fin:
                    owned(llm.park_slots, fin, st)
                    for g in fin:
                        harvest(g, n_new[g])
                live = sched.live_slots()
            if not live:
                continue
            if spec:                                     # 1 .. K + 1 tokens for every live slot
                llm.decode_step(img_ids_dev, out_ids, hid, use_graph=self.use_graph, slots=st, spec=True, draft="ngram")
            else:
                llm.decode_step(img_ids_dev, out_ids, hid, use_graph=self.use_graph, slots=st)   # one token for every live slot
            status = st.status.tolist()                                                      # the only read-back per step
            llm.comm.check()
            stats["decode_steps"] += 1
            stats["live_slot_steps"] += len(live)
            stats["parked_slot_steps"] += G - len(live)
            gone = []
            if spec:
                stats["spec_steps"] += 1
                for g in live:
                    stats["spec_emitted_tokens"] += status[g][2] - n_new[g]
                    self.last_spec_emitted[sched.slot_req[g]].append(status[g][2] - n_new[g])
            for g in live:
                cur[g], alive, n_new[g], fin_n = status[g]
                if qs is not None and seqs[sched.slot_req[g]] is not None:
                    gen[g].append(cur[g])
                if not alive:
                    harvest(g, fin_n)
                    gone.append(g)
            if gone and named:
                llm.set_adapters(gone, [None] * len(gone))   # the device parked the slot itself: its adapter index goes back to -1
        if paged:
            stats["peak_pages"] = llm._pool.peak
        owned(llm.reset)                                 # pos / ctx / step leave their idle values
        if store is not None:
            stats["host_evictions"], stats["host_bytes_peak"] = store.evictions - evicted0, store.peak
        self.last_inflight_stats = stats
        return results

    @_clears_adapters
    @torch.no_grad()
    def score(self, tokenizer, requests, n_top=0):
        """Likelihood scoring of given continuations (what multiple-choice benchmarks ask). Each request is generate_batch's prompt keys
        (optionally ``"adapter"``) plus ``"continuations"``: a list of non-empty id lists. On sequence 0 the context is prefilled ONCE
        (the logits of its last row score a continuation's first id); each continuation then rewinds the sequence to the end of the
        context (``set_position``) and runs its ids but the last as one chunk with all-row logits, and sx_token_logprobs scores the rows
        (ops.token_logprobs; the raw distribution, as for ``"logprobs"``). Returns, per request, a list with one dict per continuation:
        ``'token_logprobs'`` fp32 [len], ``'sum'`` (their sum, in fp64 on the host) and, with ``n_top`` in 1 .. 8, ``'top_ids'`` /
        ``'top_logprobs'`` [len, n_top]. A continuation's scores do not depend on the others or on their order. Works on contiguous, FP8
        and paged caches (a paged one reserves context + longest continuation and gives the pages back). The LLM's caches are reset
        before and after. Spreading candidates over slots, strings as continuations and prompt log-probabilities are out of scope."""
        llm = self.llm
        if isinstance(n_top, bool) or not isinstance(n_top, int) or not 0 <= n_top <= 8:
            raise ValueError(f"score: n_top must be an int in 0 .. 8, got {n_top!r}")
        if llm.comm.world > 1:
            raise ValueError(f"score on tp={llm.comm.world} tensor-parallel ranks is not built (follow-up)")
        requests = list(requests)
        for r, req in enumerate(requests):
            conts = req.get("continuations")
            if not conts or any(len(c) < 1 for c in conts):
                raise ValueError(f"score: request {r} needs \"continuations\": a non-empty list of non-empty id lists")
            llm._adapter_index(req.get("adapter"))      # unknown name / feature off: ValueError before anything is touched
        dev = llm.device
        P = llm._pack()
        self._conv = {}
        if self._inflight is not None:
            self._inflight["prefix"] = None
        out = []
        try:
            for req in requests:
                conts = [[int(i) for i in c] for c in req["continuations"]]
                name = req.get("adapter")
                kw = dict(adapters=[name]) if name is not None else {}
                llm.reset()
                ids, x = self._prompt_embeds(tokenizer, req)
                need = len(ids) + max(len(c) for c in conts) - 1
                assert need <= llm.Tmax, "KV cache too small for the context + the longest continuation"
                if llm.kv_pages:
                    llm._kv_need(0, need, f"score, a context of {len(ids)} rows + the longest continuation")
                first, _ = llm.forward_embeds_batch([x], [0], **kw)                          # [1, Vpad]: the context's last row
                res = []
                for c in conts:
                    rows = first
                    if len(c) > 1:
                        llm.set_position(0, len(ids))
                        xe = ops.embedding(torch.tensor(c[:-1], dtype=torch.int32, device=dev), P["embed"])
                        _, hs = llm.forward_embeds_batch([xe], [0], need_logits=False, **kw)
                        rows = torch.cat([first, llm._lm_head(hs[0])])                       # plumbing
                    lp, ti, tv = ops.token_logprobs(rows.contiguous(), llm.V, torch.tensor(c, dtype=torch.int32, device=dev), n_top)
                    lp = lp.cpu()
                    rec = {"token_logprobs": lp, "sum": float(lp.double().sum())}
                    if n_top:
                        rec.update(top_ids=ti.cpu().long(), top_logprobs=tv.cpu())
                    res.append(rec)
                out.append(res)
        finally:
            llm.reset()                                  # (a paged cache gets its pages back)
        return out

    @torch.no_grad()
    def generate(self, tokenizer, prompt=None, input_ids=None, image_embeds=None, embeds_cmp_mask=None,
                 ids_cmp_mask=None, logits_processor=None, num_img_gen_tokens=64, temperature=0.7, num_beams=1,
                 max_new_tokens=120, top_p=0.5, dtype=torch.float16, device='cuda', patch_positions=None,
                 eos_token_id="auto", force_image_at=None, reuse_cache=False, do_sample=False, top_k=50, seed=None, adapter=None,
                 logprobs=None, repetition_penalty=None, presence_penalty=None, frequency_penalty=None, logit_bias=None,
                 min_new_tokens=None, grammar=None, stop=None, no_repeat_ngram_size=None):
        """Reference signature (seed_x.py:130-145). Greedy by default (do_sample=False, num_beams=1 — temperature/top_p are inert
        in the reference too, :175-189). ``do_sample=True`` makes ``temperature`` / ``top_p`` live (defaults: the reference's 0.7 /
        0.5) together with ``top_k`` (50, transformers' generation default) and ``seed`` (None: 64 bits from os.urandom): the seeded
        device-side rule of seedx_amd.sampling; the result then carries ``'seed'``. ``eos_token_id``: "auto" →
        tokenizer.eos_token_id; None disables the EOS stop. On tensor-parallel ranks ``do_sample=True`` needs an explicit ``seed``, the
        same on every rank (ValueError otherwise). ``adapter``: name of a LoRA adapter resident on the LLM (``llm.load_adapter``) the
        request runs under, unmerged; the result carries ``'adapter'``. ``logprobs``: N in 0 .. 8 → the result carries ``'logprobs'``
        (generate_batch: per generated id its log-probability under the raw distribution and the N most likely ids).
        ``repetition_penalty`` / ``presence_penalty`` / ``frequency_penalty`` / ``logit_bias`` / ``min_new_tokens``: the device-side
        logits controls of generate_batch (what a reference user passes through ``logits_processor`` / ``generation_config``; a
        host-supplied processor list itself stays refused); the result then carries ``'controls'``. ``grammar``: name of a token
        automaton resident on the LLM (``llm.load_grammar``) that constrains the ids (generate_batch); the result carries ``'grammar'``.
        ``stop`` / ``no_repeat_ngram_size``: the device-side sequence rules of generate_batch (stop sequences as token ids; transformers'
        no_repeat_ngram_size); the result then carries ``'seq_rules'``."""
        assert logits_processor is None, "the AutoImageTokenGenerationProcessor rule is fused on the device"
        assert num_beams == 1
        assert self.llm.G == 1, "this LLM was built for lock-step batches: use generate_batch()"
        req = dict(prompt=prompt, input_ids=input_ids, image_embeds=image_embeds, embeds_cmp_mask=embeds_cmp_mask,
                   ids_cmp_mask=ids_cmp_mask, patch_positions=patch_positions)
        if logprobs is not None:
            req["logprobs"] = logprobs
        if do_sample:
            req.update(do_sample=True, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed)
        if adapter is not None:
            req["adapter"] = adapter
        req.update(repetition_penalty=repetition_penalty, presence_penalty=presence_penalty, frequency_penalty=frequency_penalty,
                   logit_bias=logit_bias, min_new_tokens=min_new_tokens)
        if grammar is not None:
            req["grammar"] = grammar
        req.update(stop=stop, no_repeat_ngram_size=no_repeat_ngram_size)
        return self.generate_batch(tokenizer, [req], num_img_gen_tokens, max_new_tokens, eos_token_id, force_image_at,
                                   reuse_cache)[0]
