"""Lossless speculative decoding, host side: the two rules the device kernels implement (sx_spec_draft_ngram / sx_spec_accept in
csrc/decode.hip), stated in plain Python. The kernels must equal them exactly; tests/test_spec_decode_*.py hold them to it.

The verify step of ``LlamaForCausalLM(spec_tokens=K)`` carries T = K + 1 rows per slot: row 0 is fed the slot's current token ``cur``,
rows 1 .. n_draft the drafted continuation. Row t produces the candidate the model emits after (history, cur, draft[:t]) — by the
greedy rule or by the seeded sampler, which is a pure function of (logits row, parameters, seed, token index), so candidate t is the
token plain decoding would emit there PROVIDED draft[:t] is what plain decoding emitted before it. ``accept`` keeps exactly that
prefix, hence the transcript is the plain one, token for token, for greedy and for sampled requests alike.
"""


def propose_ngram(hist, K, ngram_max=3, ngram_min=1):
    """Prompt-lookup draft. ``hist``: the L known ids of a sequence by cache position, the current token last. For n = ngram_max down
    to ngram_min: the LARGEST start i with hist[i:i+n] == hist[L-n:L] and i + n <= L - 1 (an earlier occurrence of the last n ids that
    has at least one id after it); the first n with a match proposes what followed it, hist[i+n : min(i+n+K, L)]. No match: []."""
    hist = [int(x) for x in hist]
    L = len(hist)
    for n in range(int(ngram_max), int(ngram_min) - 1, -1):
        if n < 1 or n > L - 1:
            continue
        tail = hist[L - n:]
        for i in range(L - 1 - n, -1, -1):
            if hist[i:i + n] == tail:
                return hist[i + n:min(i + n + int(K), L)]
    return []


def accept(cand, draft, n_new, max_new, force_at=-1, force_id=-1, eos_id=-1, img_id=-1):
    """The accept rule for one live slot. ``cand[t]``: the id row t of the verify step produced (row 0 was fed the current token, row
    t >= 1 was fed draft[t-1]); ``draft``: the n_draft ids fed; ``n_new``: tokens generated before this step. Walks t = 0, 1, ...:
    emits cand[t] — force_id instead if n_new + t == force_at, after the rule as in the plain slot step — and goes on to t + 1 only
    while t < len(draft), the emitted id equals draft[t] (row t + 1 was fed what the model really produced), it is neither EOS nor
    <img> (``img_id``: the host-driven image chunk takes over), and the budget ``max_new`` is not reached.
    Returns (emitted ids, stopped): ``stopped`` is the plain step's stop rule (EOS or budget) on the last emitted id."""
    emitted, t = [], 0
    while True:
        tok = int(cand[t])
        if force_at >= 0 and n_new + t == force_at:
            tok = int(force_id)
        emitted.append(tok)
        stopped = (eos_id >= 0 and tok == eos_id) or (n_new + t + 1 >= max_new)
        if stopped or t >= len(draft) or tok != int(draft[t]) or tok == img_id:
            return emitted, stopped
        t += 1


def steps_for(length, emitted):
    """Verify steps one request takes to produce ``length`` tokens (the first comes from its prefill) when its k-th step emits
    ``emitted[k]`` ids (>= 1 each; the last one may overshoot, the accept rule cuts it at the budget)."""
    made, k = 1, 0
    while made < length:
        made += int(emitted[k])
        k += 1
    return k
