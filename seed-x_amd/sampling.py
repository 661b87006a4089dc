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
