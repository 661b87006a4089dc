"""Seeded sampling of the next token, host side: the rule the device kernels implement (sx_sample_next_b / sx_sample_next_slots in
csrc/decode.hip), stated once in plain Python / numpy fp64 so that the kernel, the tests and a user can be held to the same words.

For a logits row x[0..V) — AFTER the image-token rule of generation.py:19-31, which the kernels apply first — and the parameters
(temperature T > 0, top_k >= 0, 0 < top_p <= 1, seed, token index n) the order is transformers' sample(): temperature → top-k → top-p:

  t_i = x_i / T
  top-k (0 < top_k < V, else off): keep t_i >= the k-th largest value (ties at it are all kept, as TopKLogitsWarper does)
  w_i = exp(t_i - max t) over the survivors, W_k their sum
  top-p: keep i iff the mass of the strictly larger survivors is below top_p · W_k. That is TopPLogitsWarper of transformers 4.30.2
         (ascending sort, remove cumsum <= 1 - top_p, keep at least one) without the sort; equal values are kept or dropped together,
         which differs from the warper only on an exact tie at the boundary
  u = (Philox4x32-10(counter (n, 0, 0, 0), key (seed & 0xffffffff, seed >> 32))[0] >> 8) · 2^-24
  id = the smallest kept index whose inclusive prefix mass exceeds u · W (W = mass of the kept set); the last kept index if rounding
       leaves none.

n is the 0-based index of the generated token within its request (0 for the token that comes out of the prefill). Plain Python and
numpy, nothing from the test infrastructure, no GPU: this module is the definition, not a fallback — the product path draws on the
device.
"""
import os

import numpy as np

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32 with ten rounds on plain Python integers: counter (c0, c1, c2, c3), key (k0, k1) → four 32-bit words."""
    c0, c1, c2, c3 = (int(c) & _MASK for c in counter)
    k0, k1 = (int(k) & _MASK for k in key)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & _MASK, p1 & _MASK, ((p0 >> 32) ^ c3 ^ k1) & _MASK, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def uniform(seed, n):
    """The draw of token index n under ``seed``: a multiple of 2^-24 in [0, 1)."""
    seed = int(seed)
    return (philox4x32_10((int(n), 0, 0, 0), (seed & _MASK, seed >> 32))[0] >> 8) * 2.0 ** -24


def reference_next(logits_row, temperature, top_k, top_p, u):
    """Steps 2-6 of the rule in numpy fp64. Returns (id, kept_mask [V] bool, probs [V] fp64: the distribution over the kept set).
    ``larger_mass`` (the quantity compared with top_p) is available from ``nucleus``."""
    kept, probs, _ = nucleus(logits_row, temperature, top_k, top_p)
    cdf = np.cumsum(probs)                                  # index order; zero increments outside the kept set
    hit = np.nonzero(kept & (cdf > u * cdf[-1]))[0]
    idx = int(hit[0]) if hit.size else int(np.nonzero(kept)[0][-1])
    return idx, kept, probs


def nucleus(logits_row, temperature, top_k, top_p):
    """(kept_mask, probs over the kept set, larger_mass): larger_mass[i] = mass of the strictly larger top-k survivors / W_k (inf
    for tokens that top-k removed). Token i is kept iff larger_mass[i] < top_p."""
    x = np.asarray(logits_row, dtype=np.float64).reshape(-1)
    V = x.size
    t = x / float(temperature)
    alive = np.ones(V, dtype=bool)
    if 0 < int(top_k) < V:
        alive = t >= np.partition(t, V - int(top_k))[V - int(top_k)]
    w = np.where(alive, np.exp(t - t.max()), 0.0)
    Wk = w.sum()
    order = np.argsort(-t, kind="stable")                  # descending
    ts, ws = t[order], w[order]
    before = np.concatenate([[0.0], np.cumsum(ws)[:-1]])    # mass ahead of each position in the sorted order
    first = np.concatenate([[True], ts[1:] != ts[:-1]])     # start of each run of equal values
    run_start = np.maximum.accumulate(np.where(first, np.arange(V), 0))
    larger = np.empty(V)
    larger[order] = before[run_start] / Wk
    larger[~alive] = np.inf
    kept = alive & (larger < float(top_p))
    wk = np.where(kept, w, 0.0)
    return kept, wk / wk.sum(), larger


MAX_TOP_LOGPROBS = 8


def token_logprobs(row, targets=None, n_top=0):
    """The log-probability rule the device kernels implement (sx_token_logprobs and the LP decode tail), in numpy fp64. ``row``: the
    RAW fp32 logits row x[0..V) — what lm_head produced, before the image-token rule's in-place zeroing, temperature, top-k and top-p —
    or [R, V] rows; ``targets``: one id per row (None: no chosen value). lp(v) = x[v] - logsumexp(x).
    Returns (chosen [R] fp64 or None, top_ids [R, n_top] int64, top [R, n_top] fp64), without the leading axis for a 1-D row. The top
    list holds the n_top largest x, ties lowest index first; entries past V are id -1, value -inf. x[v] = -inf gives -inf. A row that
    holds NaN (or whose logsumexp is not finite: +inf, nothing but -inf) gives NaN values and top ids -1; a target outside [0, V) NaN."""
    x = np.asarray(row, dtype=np.float64)
    flat = x.ndim == 1
    x = np.atleast_2d(x)
    R, V = x.shape
    n_top = int(n_top)
    assert n_top >= 0
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = x.max(axis=1, keepdims=True)
        lp = (x - m) - np.log(np.exp(x - m).sum(axis=1, keepdims=True))
    bad = np.isnan(lp).any(axis=1)
    lp[bad] = np.nan
    k = min(n_top, V)
    order = np.argsort(-x, axis=1, kind="stable")[:, :k]     # descending value, ascending index among equals
    top_ids = np.full((R, n_top), -1, dtype=np.int64)
    top = np.full((R, n_top), -np.inf)
    top_ids[:, :k] = order
    top[:, :k] = np.take_along_axis(lp, order, axis=1)
    top_ids[bad] = -1
    top[bad] = np.nan
    chosen = None
    if targets is not None:
        t = np.asarray(targets, dtype=np.int64).reshape(R)
        ok = (t >= 0) & (t < V)
        chosen = np.where(ok, lp[np.arange(R), np.where(ok, t, 0)], np.nan)
    if flat:
        return (None if chosen is None else chosen[0]), top_ids[0], top[0]
    return chosen, top_ids, top


def logprobs_from_request(req):
    """The ``"logprobs"`` key of a request dict: None (absent: the request records nothing) or N, an int in 0 .. 8 — the chosen token's
    log-probability and the N most likely alternatives per generated token. Anything else is a ValueError."""
    n = req.get("logprobs")
    if n is None:
        return None
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= int(n) <= MAX_TOP_LOGPROBS:
        raise ValueError(f"logprobs must be an int in 0 .. {MAX_TOP_LOGPROBS} (0: the chosen token only), got {n!r}")
    return int(n)


def logprobs_result(token_ids, chosen, top_ids, top, n):
    """The ``'logprobs'`` entry of a result: one record per generated id in generation order, the top lists trimmed to the request's
    ``n``. chosen [T]; top_ids / top [T, >= n] (or anything when n = 0). Arrays or tensors; what comes in goes out, sliced."""
    T = len(token_ids)
    assert len(chosen) == T and (n == 0 or (top_ids.shape[0] == T and top_ids.shape[1] >= n and top.shape == top_ids.shape))
    if n == 0:
        top_ids, top = top_ids[:T, :0], top[:T, :0]
    return {"token_ids": token_ids, "token_logprobs": chosen, "top_ids": top_ids[:, :n], "top_logprobs": top[:, :n]}


class SamplingParams:
    """How one request picks its tokens. ``do_sample=False`` is the greedy arg-max (the other fields are then inert). Defaults: the
    reference's temperature 0.7 / top_p 0.5 (seed_x.py:130-145) and transformers' generation default top_k 50, which a sampled
    reference run would have used. ``seed=None`` takes 64 bits from os.urandom; the value used is in ``.seed`` either way (single rank
    only: see ``from_request``)."""
    __slots__ = ("do_sample", "temperature", "top_k", "top_p", "seed")

    def __init__(self, do_sample=False, temperature=0.7, top_k=50, top_p=0.5, seed=None):
        temperature, top_p, top_k = float(temperature), float(top_p), int(top_k)
        if not (np.isfinite(temperature) and temperature > 0):
            raise ValueError(f"temperature must be a finite number > 0, got {temperature}")
        if not 0 < top_p <= 1:
            raise ValueError(f"top_p must lie in (0, 1], got {top_p}")
        if top_k < 0:
            raise ValueError(f"top_k must be >= 0 (0 disables it), got {top_k}")
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"seed must lie in [0, 2^64), got {seed}")
        self.do_sample, self.temperature, self.top_k, self.top_p, self.seed = bool(do_sample), temperature, top_k, top_p, seed

    @classmethod
    def from_request(cls, req, world=1):
        """The sampling keys of a generate_batch / generate_inflight request dict; None when the request is greedy. ``world``: the
        number of tensor-parallel ranks that each build these parameters in their own process. Every rank must draw the same ids
        from the gathered logits, so with world > 1 a sampled request has to NAME its seed: ``seed=None`` would give every rank its
        own os.urandom value and is refused."""
        if not req.get("do_sample"):
            return None
        if int(world) > 1 and req.get("seed") is None:
            raise ValueError(f"do_sample with seed=None on {int(world)} tensor-parallel ranks: every rank would take its own random seed "
                             "and draw different tokens. Pass the same explicit seed on every rank.")
        kw = {k: req[k] for k in ("temperature", "top_k", "top_p", "seed") if req.get(k) is not None}
        return cls(do_sample=True, **kw)

    def __repr__(self):
        return (f"SamplingParams(do_sample={self.do_sample}, temperature={self.temperature}, top_k={self.top_k}, "
                f"top_p={self.top_p}, seed={self.seed})")


# ---- per-request logits controls: repetition / presence / frequency penalties, logit bias, min_new_tokens ---------------------------
MAX_LOGIT_BIAS = 16
COUNT_MARK = 1 << 30          # bit 30 of a count word: the id occurs in the prompt
COUNT_MASK = 0xFFFFFF         # low 24 bits of a count word: how often the id was generated
CONTROL_KEYS = ("repetition_penalty", "presence_penalty", "frequency_penalty", "logit_bias", "min_new_tokens")


class ControlParams:
    """The logits controls of one request (the rule: ``apply_controls``). ``repetition_penalty`` finite > 0 (1.0: off, transformers'
    RepetitionPenaltyLogitsProcessor over prompt and generated ids); ``presence_penalty`` / ``frequency_penalty`` finite (0.0: off, the
    OpenAI definition: generated ids only, the prompt does not count); ``logit_bias`` {id: bias} or None, at most 16 entries, a bias
    finite or -inf (-inf bans the id; the ids are checked against the vocabulary by ``check_vocab``); ``min_new_tokens`` >= 0 (the EOS
    column is -inf while fewer tokens were generated; no-op in a call without an EOS id). Malformed values are a ValueError.
    ``rep_inv`` is float32(1 / repetition_penalty), computed in fp64 and rounded once: what the kernel multiplies by."""
    __slots__ = ("repetition_penalty", "presence_penalty", "frequency_penalty", "logit_bias", "min_new_tokens", "rep_inv")

    def __init__(self, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None, min_new_tokens=0):
        def num(name, v):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise ValueError(f"{name} must be a number, got {v!r}")
            return float(v)
        r = num("repetition_penalty", repetition_penalty)
        def fin32(v):                                   # finite as the float32 the device holds
            with np.errstate(over="ignore", under="ignore"):
                return bool(np.isfinite(np.float32(v)))
        if not (np.isfinite(r) and r > 0 and np.float32(r) > 0 and fin32(r) and fin32(1.0 / r)):
            raise ValueError(f"repetition_penalty must be a finite number > 0 (1.0 disables it), got {repetition_penalty!r}")
        a, f = num("presence_penalty", presence_penalty), num("frequency_penalty", frequency_penalty)
        for name, v in (("presence_penalty", a), ("frequency_penalty", f)):
            if not fin32(v):
                raise ValueError(f"{name} must be a finite number, got {v!r}")
        bias = []
        if logit_bias is not None:
            if not isinstance(logit_bias, dict):
                raise ValueError(f"logit_bias must be a dict {{id: bias}} or None, got {logit_bias!r}")
            if len(logit_bias) > MAX_LOGIT_BIAS:
                raise ValueError(f"logit_bias holds {len(logit_bias)} entries, at most {MAX_LOGIT_BIAS} are supported")
            for i, b in logit_bias.items():
                if isinstance(i, bool) or not isinstance(i, (int, np.integer)) or int(i) < 0:
                    raise ValueError(f"logit_bias ids must be ints >= 0, got {i!r}")
                b = num(f"logit_bias[{i!r}]", b)
                if not (fin32(b) or b == -np.inf):
                    raise ValueError(f"logit_bias[{i!r}] must be finite or -inf (-inf bans the id), got {b!r}")
                bias.append((int(i), b))
        m = min_new_tokens
        if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or int(m) < 0:
            raise ValueError(f"min_new_tokens must be an int >= 0, got {min_new_tokens!r}")
        self.repetition_penalty, self.presence_penalty, self.frequency_penalty = r, a, f
        self.logit_bias, self.min_new_tokens = tuple(bias), int(m)
        self.rep_inv = float(np.float32(1.0 / r))

    def is_default(self):
        return (np.float32(self.repetition_penalty) == 1 and np.float32(self.presence_penalty) == 0
                and np.float32(self.frequency_penalty) == 0 and not self.logit_bias and self.min_new_tokens == 0)

    def check_vocab(self, vocab):
        for i, _ in self.logit_bias:
            if not i < int(vocab):
                raise ValueError(f"logit_bias id {i} lies outside the vocabulary [0, {int(vocab)})")
        return self

    @classmethod
    def from_request(cls, req, vocab=None):
        """The control keys of a generate_batch / generate_inflight request dict (``generate`` takes the same names as kwargs); None
        when every one of them is absent, None or at its default: such a request runs the calls and graphs it always ran."""
        kw = {k: req[k] for k in CONTROL_KEYS if req.get(k) is not None}
        if not kw:
            return None
        p = cls(**kw)
        if vocab is not None:
            p.check_vocab(vocab)
        return None if p.is_default() else p

    def as_dict(self):
        """What a result's ``'controls'`` entry holds: the values the device used."""
        return {"repetition_penalty": self.repetition_penalty, "presence_penalty": self.presence_penalty,
                "frequency_penalty": self.frequency_penalty, "logit_bias": dict(self.logit_bias), "min_new_tokens": self.min_new_tokens}

    def __repr__(self):
        return "ControlParams(" + ", ".join(f"{k}={v!r}" for k, v in self.as_dict().items()) + ")"


def count_words(vocab, prompt_ids=(), generated_ids=()):
    """The count words c[0..vocab) of a request: bit 30 set for every id of the prompt, the low 24 bits the number of times the id was
    generated. Ids outside [0, vocab) (placeholders of image rows) leave no trace."""
    c = np.zeros(int(vocab), dtype=np.int32)
    p = np.asarray(list(prompt_ids), dtype=np.int64).reshape(-1)
    c[p[(p >= 0) & (p < vocab)]] = COUNT_MARK
    g = np.asarray(list(generated_ids), dtype=np.int64).reshape(-1)
    g = g[(g >= 0) & (g < vocab)]
    c += np.bincount(g, minlength=int(vocab)).astype(np.int32)
    return c


def apply_controls(row, counts, params, eos_id=-1, token_index=0):
    """The rule of the device-side logits controls (next_token_kernel<.., CTL> in csrc/decode.hip, sx_next_b_ctl / sx_next_slots_ctl), in
    numpy FLOAT32 with one IEEE rounding per written operation: the kernel, the tests and a user are held to these words, bit for bit.

    ``row``: the raw fp32 logits x[0..V). ``counts``: int32 [V], per id the word c with mark = bit 30 (the id occurs in the prompt) and
    n = c & 0xFFFFFF (times generated so far). ``params``: a ControlParams. ``token_index`` k: the 0-based index of the token being
    chosen within its request (the sampler's). Returns y, a new fp32 array:

      1. r != 1 and (mark or n > 0):   y = y * r if y < 0 else y * rinv,  rinv = float32(1 / r) rounded once from fp64. A MULTIPLY by
         the rounded reciprocal, where transformers' RepetitionPenaltyLogitsProcessor divides (x / r): the two may differ by one ulp.
      2. n > 0:                        t = f * float32(n);  t = t + a;  y = y - t     (a = presence, f = frequency penalty; with
         a = f = 0 the identity on the bits)
      3. every logit_bias entry, in the dict's order:  y[id] = y[id] + b             (b = -inf bans the id)
      4. eos_id >= 0 and k < min_new_tokens:  y[eos_id] = -inf

    The image-token rule then runs on y (a row inside the image chain is forced whatever the controls say; otherwise the image columns
    img_ids[1:] are zeroed, which overwrites any control on them), and then the arg-max or the seeded draw of the uncontrolled call."""
    f32 = np.float32
    y = np.array(row, dtype=f32).reshape(-1).copy()
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    assert c.size == y.size
    n = c & COUNT_MASK
    seen = ((c & COUNT_MARK) != 0) | (n > 0)
    r, rinv = f32(params.repetition_penalty), f32(params.rep_inv)
    a, f = f32(params.presence_penalty), f32(params.frequency_penalty)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if r != f32(1):
            y = np.where(seen, np.where(y < 0, y * r, y * rinv), y).astype(f32)
        t = (f * n.astype(f32)).astype(f32)
        t = (t + a).astype(f32)
        y = np.where(n > 0, (y - t).astype(f32), y).astype(f32)
        for i, b in params.logit_bias:
            y[i] = f32(y[i] + f32(b))
    if int(eos_id) >= 0 and int(token_index) < params.min_new_tokens:
        y[int(eos_id)] = -np.inf
    return y


# ---- per-request sequence rules: stop sequences and no_repeat_ngram_size ----------------------------------------------------------
MAX_STOP = 4                  # stop sequences per request
MAX_STOP_LEN = 8              # ids per stop sequence
MAX_NGRAM = 8                 # largest no_repeat_ngram_size
SEQ_KEYS = ("stop", "no_repeat_ngram_size")


class SeqParams:
    """The sequence rules of one request (the rules: ``ngram_banned`` / ``apply_no_repeat`` / ``stop_match``). ``stop``: at most 4 stop
    sequences of 1 .. 8 token ids each ([[ids], ...]; one flat list of ints counts as one sequence; the ids are checked against the
    vocabulary by ``check_vocab``); a request ends on the token that completes one of them, and the matched ids stay in its result, as
    the EOS id does. Strings are refused: how a string tokenises depends on what precedes it, so the caller passes ids.
    ``no_repeat_ngram_size`` n in 0 .. 8 (0 or None: off): no n-gram of prompt + generated ids occurs twice (transformers'
    NoRepeatNGramLogitsProcessor). Malformed values are a ValueError."""
    __slots__ = ("stop", "no_repeat_ngram_size")

    def __init__(self, stop=None, no_repeat_ngram_size=0):
        is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
        seqs = []
        if stop is not None:
            if isinstance(stop, (str, bytes)) or (isinstance(stop, (list, tuple)) and any(isinstance(s, (str, bytes)) for s in stop)):
                raise ValueError(f"stop must hold token ids, not strings (got {stop!r}): how a string tokenises depends on what precedes "
                                 "it, so encode the stop sequences yourself and pass their ids")
            if not isinstance(stop, (list, tuple)):
                raise ValueError(f"stop must be a list of stop sequences [[ids], ...] (or one flat list of ids), got {stop!r}")
            if stop and all(is_int(s) for s in stop):
                stop = [stop]
            if len(stop) > MAX_STOP:
                raise ValueError(f"stop holds {len(stop)} sequences, at most {MAX_STOP} are supported")
            for s in stop:
                if not isinstance(s, (list, tuple)) or not all(is_int(t) for t in s):
                    raise ValueError(f"every stop sequence must be a list of int token ids, got {s!r}")
                if not 1 <= len(s) <= MAX_STOP_LEN:
                    raise ValueError(f"a stop sequence must hold 1 .. {MAX_STOP_LEN} ids, got {len(s)}: {list(s)!r}")
                if any(int(t) < 0 for t in s):
                    raise ValueError(f"stop ids must be ints >= 0, got {list(s)!r}")
                seqs.append(tuple(int(t) for t in s))
        n = 0 if no_repeat_ngram_size is None else no_repeat_ngram_size
        if not is_int(n) or not 0 <= int(n) <= MAX_NGRAM:
            raise ValueError(f"no_repeat_ngram_size must be an int in 0 .. {MAX_NGRAM} (0 disables it), got {no_repeat_ngram_size!r}")
        self.stop, self.no_repeat_ngram_size = tuple(seqs), int(n)

    def is_default(self):
        return not self.stop and self.no_repeat_ngram_size == 0

    def check_vocab(self, vocab):
        for s in self.stop:
            for t in s:
                if not t < int(vocab):
                    raise ValueError(f"stop id {t} lies outside the vocabulary [0, {int(vocab)})")
        return self

    @classmethod
    def from_request(cls, req, vocab=None):
        """The sequence-rule keys of a generate_batch / generate_inflight request dict (``generate`` takes the same names as kwargs);
        None when both are absent or off (None, 0, []): such a request runs the calls and graphs it always ran."""
        kw = {k: req[k] for k in SEQ_KEYS if req.get(k) is not None}
        if not kw:
            return None
        p = cls(**kw)
        if vocab is not None:
            p.check_vocab(vocab)
        return None if p.is_default() else p

    def as_dict(self):
        """What a result's ``'seq_rules'`` entry starts from: the values the device used (the engines add ``'matched'``)."""
        return {"stop": [list(s) for s in self.stop], "no_repeat_ngram_size": self.no_repeat_ngram_size}

    def __repr__(self):
        return "SeqParams(" + ", ".join(f"{k}={v!r}" for k, v in self.as_dict().items()) + ")"


def ngram_banned(hist, n, vocab=None):
    """The ids no_repeat_ngram_size = n bans for the next token (next_token_kernel<.., SEQ> in csrc/decode.hip, sx_next_b_seq /
    sx_next_slots_seq). ``hist``: the request's prompt ids followed by every id generated so far, L = len(hist). For n >= 1 and every
    i in [0, L - n]: if hist[i : i+n-1] == hist[L-n+1 : L] then hist[i+n-1] is banned (n = 1: the compared prefix is empty, every id of
    the history is banned; L < n: no n-gram exists yet, nothing is banned). With ``vocab`` = V ids outside [0, V) — image placeholders —
    ban nothing; they still take part in the comparison. This is transformers' NoRepeatNGramLogitsProcessor on one sequence."""
    h = [int(t) for t in hist]
    n, L = int(n), len(h)
    out = set()
    if n < 1:
        return out
    tail = h[L - n + 1:L] if n > 1 else []
    for i in range(0, L - n + 1):
        if h[i:i + n - 1] == tail:
            t = h[i + n - 1]
            if vocab is None or 0 <= t < int(vocab):
                out.add(t)
    return out


def apply_no_repeat(row, hist, n):
    """``row`` (fp32 [V]; a raw row or apply_controls' result) with the columns of ngram_banned(hist, n, V) set to -inf: a new array,
    nothing else changes. The grammar mask, the image-token rule and the arg-max or draw then run on it."""
    y = np.array(row, dtype=np.float32).reshape(-1).copy()
    ban = sorted(ngram_banned(hist, n, y.size))
    if ban:
        y[ban] = -np.inf
    return y


def stop_match(generated, stops):
    """The lowest index j for which the GENERATED ids end with stops[j], else None. Only generated ids are compared: a stop that would
    straddle the end of the prompt does not match. The matched ids stay in the result, the way the EOS id does."""
    g = [int(t) for t in generated]
    for j, s in enumerate(stops):
        s = [int(t) for t in s]
        if 1 <= len(s) <= len(g) and g[len(g) - len(s):] == s:
            return j
    return None
