"""Lossless speculative decoding, host side: the accept rule and the prompt-lookup drafter of seedx_amd.spec (what the device kernels
sx_spec_accept / sx_spec_draft_ngram must equal), the refusals of LlamaForCausalLM(spec_tokens=K), the step-count simulator and the
argument structs."""
import os
import random
import re

import pytest

from oracle import weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG, EOS, FORCE = 400, 7, 401


def _toy_next(history):
    """A deterministic next-token function of the whole history (ids 0 .. 15; 7 = EOS turns up now and then)."""
    h = 0
    for i, t in enumerate(history[-5:]):
        h = (h * 31 + (t + 3) * (i + 11)) % 1009
    return h % 16


def _plain(prompt, first, max_new, force_at=-1, eos=-1):
    """The one-token-at-a-time transcript of the plain slot step: token 0 is ``first`` (the prefill's), then the rule."""
    out = [first]
    while True:
        if len(out) >= max_new or (eos >= 0 and out[-1] == eos):
            return out
        tok = _toy_next(prompt + out)
        if force_at >= 0 and len(out) == force_at:
            tok = FORCE
        out.append(tok)


def _speculative(prompt, first, max_new, drafter, K, force_at=-1, eos=-1, img=-1):
    """The same request through verify steps: drafts from ``drafter(history, step index)``, candidates from the toy function on
    (history + cur + draft[:t]), spec.accept for what is kept. Returns (transcript, emitted counts per step)."""
    from seedx_amd import spec
    out, counts, k = [first], [], 0
    if len(out) >= max_new or (eos >= 0 and first == eos):
        return out, counts
    while True:
        draft = list(drafter(prompt + out, k))[:K]
        cand = [_toy_next(prompt + out + draft[:t]) for t in range(len(draft) + 1)]
        emitted, stopped = spec.accept(cand, draft, len(out), max_new, force_at, FORCE, eos, img)
        assert 1 <= len(emitted) <= len(draft) + 1
        out += emitted
        counts.append(len(emitted))
        k += 1
        if stopped:
            return out, counts


def _oracle_drafter(prompt, plain, n_right, wrong=True):
    """Drafts cut from the plain transcript: ``n_right(k)`` correct ids at step k, then (``wrong``) one id the model does not emit."""
    def d(history, k):
        done = len(history) - len(prompt)
        right = plain[done:done + n_right(k)]
        nxt = plain[done + len(right)] if done + len(right) < len(plain) else 0
        return right + ([(nxt + 1) % 16] if wrong else [])
    return d


@pytest.mark.parametrize("K", [1, 3, 7])
def test_accept_reproduces_the_plain_transcript(K):
    """Right, wrong, partially right and empty drafts; EOS inside an accepted run; the budget inside a run; force_at inside a run."""
    rng = random.Random(5)
    for case in range(60):
        prompt = [rng.randrange(16) for _ in range(rng.randrange(1, 9))]
        first, max_new = rng.randrange(16), rng.randrange(1, 40)
        force_at = rng.choice([-1, -1, 0, 1, 2, 5, 11])
        eos = rng.choice([-1, EOS])
        plain = _plain(prompt, first, max_new, force_at, eos)
        drafters = {
            "all right": _oracle_drafter(prompt, plain, lambda k: K, wrong=False),
            "cycling": _oracle_drafter(prompt, plain, lambda k: k % (K + 1)),
            "wrong": lambda h, k: [(_toy_next(h) + 1) % 16] * K,
            "empty": lambda h, k: [],
            "random": lambda h, k: [rng.randrange(16) for _ in range(rng.randrange(K + 1))],
        }
        for name, d in drafters.items():
            got, counts = _speculative(prompt, first, max_new, d, K, force_at, eos)
            assert got == plain, (case, name, got, plain)
            if name == "empty":
                assert counts == [1] * (len(plain) - 1)
            if name == "all right" and force_at < 0 and len(plain) > 1:
                assert len(counts) == -(-(len(plain) - 1) // (K + 1)), (case, counts, plain)      # every step keeps K + 1 ids


def test_accept_hand_cases():
    from seedx_amd import spec
    # all drafts right: K + 1 ids
    assert spec.accept([5, 6, 7, 8], [5, 6, 7], 3, 100) == ([5, 6, 7, 8], False)
    # the second draft is wrong: the model's own id replaces it and the walk ends
    assert spec.accept([5, 9, 7, 8], [5, 6, 7], 3, 100) == ([5, 9], False)
    # no draft: the plain step
    assert spec.accept([5], [], 3, 100) == ([5], False)
    # EOS inside an accepted run stops there, although the next draft would match
    assert spec.accept([5, EOS, 7, 8], [5, EOS, 7], 3, 100, eos_id=EOS) == ([5, EOS], True)
    # the budget inside the run: n_new 3, max_new 5 → two ids
    assert spec.accept([5, 6, 7, 8], [5, 6, 7], 3, 5) == ([5, 6], True)
    # force_at inside the run: generated token 4 becomes force_id AFTER the rule; the draft fed there was 6, so the walk ends
    assert spec.accept([5, 6, 7, 8], [5, 6, 7], 3, 100, force_at=4, force_id=IMG) == ([5, IMG], False)
    # ... unless the draft was the forced id itself and it is not <img>
    assert spec.accept([5, 6, 7, 8], [5, FORCE, 7], 3, 100, force_at=4, force_id=FORCE) == ([5, FORCE, 7, 8], False)
    # <img> ends a run even when the draft matches: the host-driven image chunk takes over
    assert spec.accept([5, IMG, 7, 8], [5, IMG, 7], 3, 100, img_id=IMG) == ([5, IMG], False)
    # the last id of a run that hits the budget exactly
    assert spec.accept([5, 6], [5], 3, 5) == ([5, 6], True)


def test_propose_ngram_hand_cases():
    from seedx_amd.spec import propose_ngram
    assert propose_ngram([1, 2, 3, 4, 5], 4) == []                              # no id occurs twice
    assert propose_ngram([9], 4) == [] and propose_ngram([], 4) == []           # nothing before the current token
    # n = 3 preferred over n = 1: "1 2 3" occurred at 0 (followed by 7 8), the lone 3 also later at 6 (followed by 5)
    assert propose_ngram([1, 2, 3, 7, 8, 9, 3, 5, 1, 2, 3], 2) == [7, 8]
    assert propose_ngram([1, 2, 3, 7, 8, 9, 3, 5, 1, 2, 3], 2, ngram_max=1) == [5, 1]
    # the latest occurrence wins
    assert propose_ngram([4, 1, 4, 2, 4, 3, 4], 1) == [3]
    assert propose_ngram([4, 1, 0, 4, 2, 0, 4], 3, ngram_max=1) == [2, 0, 4]
    # the draft is clipped at L: the match ends one id before the end
    assert propose_ngram([6, 6], 4) == [6]
    assert propose_ngram([1, 2, 1, 2, 1], 7) == [2, 1]                          # n = 3 "1 2 1" at 0, then only two ids are known
    # ngram_min above 1: a lone repeated id is not enough
    assert propose_ngram([4, 1, 4], 2, ngram_max=3, ngram_min=2) == []
    # an overlapping occurrence counts (i + n <= L - 1)
    assert propose_ngram([5, 5, 5, 5], 3) == [5]


def test_propose_ngram_against_brute_force():
    from seedx_amd.spec import propose_ngram
    rng = random.Random(11)
    for _ in range(300):
        L, K = rng.randrange(0, 30), rng.randrange(1, 8)
        nmax = rng.randrange(1, 5)
        nmin = rng.randrange(1, nmax + 1)
        h = [rng.randrange(3) for _ in range(L)]
        want = []
        for n in range(nmax, nmin - 1, -1):
            starts = [i for i in range(0, L - n) if h[i:i + n] == h[L - n:L]] if n <= L - 1 else []
            if starts:
                i = max(starts)
                want = h[i + n:i + n + K][:L - (i + n)]
                break
        assert propose_ngram(h, K, nmax, nmin) == want, (h, K, nmax, nmin)


def test_spec_tokens_refusals():
    """Every configuration the verify step does not cover is a ValueError at construction; 0 is the model as it was."""
    from seedx_amd.llama import LlamaForCausalLM
    cfg = dict(weights.MINI_LLM)
    assert LlamaForCausalLM(dict(cfg), max_batch=2).spec_tokens == 0
    m = LlamaForCausalLM(dict(cfg), max_batch=4, precise=True, spec_tokens=7)
    assert m.spec_tokens == 7 and "spec_decode" in m.memory_footprint()
    assert "spec_decode" not in LlamaForCausalLM(dict(cfg), max_batch=4, precise=True).memory_footprint()
    for wf, wr, v16 in (("fp8_e4m3", None, None), ("mxfp4", "tiles", True), (None, None, False)):
        assert LlamaForCausalLM(dict(cfg), max_batch=2, precise=True, spec_tokens=3, weight_format=wf, weight_residency=wr, kv_v16=v16).spec_tokens == 3
    bad = [
        (dict(max_batch=2, precise=True, spec_tokens=8), "1 .. 7"),
        (dict(max_batch=2, precise=True, spec_tokens=-1), "1 .. 7"),
        (dict(max_batch=2, precise=False, spec_tokens=3), "precise"),
        (dict(max_batch=5, precise=True, spec_tokens=7), "32 rows"),
        (dict(max_batch=17, precise=True, spec_tokens=1), "32 rows"),
        (dict(max_batch=2, precise=True, spec_tokens=3, kv_format="fp8_e4m3"), "kv_format"),
        (dict(max_batch=2, precise=True, spec_tokens=3, kv_format="fp8_e4m3_emulated"), "kv_format"),
        (dict(max_batch=2, precise=True, spec_tokens=3, max_adapters=2), "max_adapters"),
    ]
    for kw, word in bad:
        with pytest.raises(ValueError, match=word):
            LlamaForCausalLM(dict(cfg), **kw)
    with pytest.raises(ValueError, match="head_dim 128"):                       # H 256 with 4 heads: head_dim 64
        LlamaForCausalLM(dict(cfg, num_attention_heads=4), max_batch=2, precise=True, spec_tokens=3)
    with pytest.raises(ValueError, match="tiled precise decode path"):          # FFN 208: no multiple of 64
        LlamaForCausalLM(dict(cfg, intermediate_size=208), max_batch=2, precise=True, spec_tokens=3)

    class TwoRanks:
        world, rank, graph_safe = 2, 0, False
    with pytest.raises(ValueError, match="single rank"):
        LlamaForCausalLM(dict(cfg, num_attention_heads=4, hidden_size=512, intermediate_size=1024), max_batch=2, precise=True, spec_tokens=3, comm=TwoRanks())
    m = LlamaForCausalLM(dict(cfg), max_batch=2, precise=True)                  # the verify step is refused without spec_tokens
    m._P = {}
    with pytest.raises(ValueError, match="spec_tokens"):
        m.decode_step(None, None, None, slots=object(), spec=True)


def test_simulate_spec_against_brute_force():
    """The step-count simulator: with every count 1 it is inflight.simulate; otherwise a hand-rolled loop over the same schedule."""
    from seedx_amd.inflight import simulate, simulate_spec
    from seedx_amd.spec import steps_for
    rng = random.Random(3)
    for _ in range(40):
        G, N = rng.randrange(1, 5), rng.randrange(1, 12)
        lengths = [rng.randrange(1, 30) for _ in range(N)]
        ones = simulate_spec(lengths, G, [[1] * 64 for _ in lengths])
        base = simulate(lengths, G)
        assert {k: ones[k] for k in base} == base and ones["emitted_tokens"] == sum(n - 1 for n in lengths)
        emitted = [[rng.randrange(1, 9) for _ in range(64)] for _ in lengths]
        got = simulate_spec(lengths, G, emitted)
        # brute force: before every step free slots take the queue head, lowest slot first, in rounds (a request of length 1 ends at
        # its admission and frees the slot for the next round), at most G admissions per pass
        queue, slot, left, steps, live_steps, order = list(range(N)), [None] * G, {}, 0, 0, []
        while queue or any(s is not None for s in slot):
            quota, took = G, True
            while took:
                took = False
                for g in range(G):
                    if slot[g] is None and queue and quota > 0:
                        r, quota, took = queue.pop(0), quota - 1, True
                        if lengths[r] <= 1:
                            order.append(r)
                        else:
                            slot[g], left[g] = r, [lengths[r] - 1, 0]
            live = [g for g in range(G) if slot[g] is not None]
            if not live:
                continue
            steps += 1
            live_steps += len(live)
            for g in live:
                left[g][0] -= emitted[slot[g]][left[g][1]]
                left[g][1] += 1
                if left[g][0] <= 0:
                    order.append(slot[g])
                    slot[g] = None
        assert sorted(order) == sorted(got["finish_order"]) == list(range(N))
        assert got["emitted_tokens"] == sum(n - 1 for n in lengths)
        assert got["live_slot_steps"] == sum(steps_for(n, e) for n, e in zip(lengths, emitted)) == live_steps
        assert got["decode_steps"] == steps <= base["decode_steps"], (lengths, G, got, steps)
    assert simulate_spec([9], 1, [[8]])["decode_steps"] == 1 and simulate_spec([10], 1, [[8, 8]])["decode_steps"] == 2


def test_spec_structs_mirror_the_header():
    """Field order / count of sx_spec_accept_args and sx_spec_draft_args (the parsing of test_ctypes_struct_layout_matches_header); the
    three entries are declared, bound and exported."""
    import ctypes
    from seedx_amd import _lib
    src = open(os.path.join(ROOT, "include", "seedx_hip.h")).read()
    for cname, cls in (("sx_spec_accept_args", _lib.SpecAcceptArgs), ("sx_spec_draft_args", _lib.SpecDraftArgs)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            decl = re.sub(r"^(const\s+)?(void|float|double|int32_t|int64_t|uint32_t|uint64_t)\s*\*?", "", decl)
            names += [n.strip().lstrip("*") for n in decl.split(",")]
        assert names == [f[0] for f in cls._fields_], (cname, names)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("sx_spec_accept", "sx_spec_draft_ngram", "sx_scatter_rows_spec"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and re.search(r"\bint %s\(" % name, src)
