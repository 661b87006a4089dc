"""Device-side logits controls, host side: the float32 rule the tail kernel is held to (seedx_amd.sampling.apply_controls), the request
keys (ControlParams.from_request), every refusal of the engines, and the C-ABI of the two new entry points."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from seedx_amd import sampling
from seedx_amd.sampling import COUNT_MARK, ControlParams, apply_controls, count_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _row(V=97, seed=0):
    x = (np.random.default_rng(seed).normal(size=V) * 3).astype(F32)
    x[5], x[6] = F32(-0.0), F32(0.0)
    return x


def _bits(a):
    return np.asarray(a, dtype=F32).view(np.uint32)


def test_defaults_are_the_identity_on_the_bits():
    x = _row()
    c = count_words(97, prompt_ids=[1, 5, 9, 9], generated_ids=[5, 5, 6, 40])
    y = apply_controls(x, c, ControlParams(), eos_id=7, token_index=0)
    assert y.dtype == F32 and y is not x and np.array_equal(_bits(y), _bits(x))
    assert _bits(y)[5] == 0x80000000                                         # -0.0 stays -0.0 through y - (0 * n + 0)
    assert ControlParams().is_default() and ControlParams().rep_inv == 1.0


def test_count_words():
    c = count_words(10, prompt_ids=[3, 3, 9, 12, -1], generated_ids=[3, 4, 4, 4, 11])
    assert c.dtype == np.int32 and c[3] == COUNT_MARK + 1 and c[9] == COUNT_MARK and c[4] == 3 and c[0] == 0 and c.sum() == 2 * COUNT_MARK + 4


def test_repetition_penalty_is_a_multiply_over_prompt_and_generated():
    x = _row()
    c = count_words(97, prompt_ids=[1, 2], generated_ids=[2, 3, 3])
    for r in (1.3, 0.7, 3.0):
        p = ControlParams(repetition_penalty=r)
        assert p.rep_inv == float(F32(1.0 / r))
        y = apply_controls(x, c, p)
        exp = x.copy()
        for v in (1, 2, 3):                                                  # prompt only, both, generated only
            exp[v] = x[v] * F32(r) if x[v] < 0 else x[v] * F32(p.rep_inv)
        assert np.array_equal(_bits(y), _bits(exp))
        hf = np.where(x < 0, x * F32(r), x / F32(r)).astype(F32)             # transformers divides: at most one ulp away
        d = np.abs(_bits(y)[[1, 2, 3]].astype(np.int64) - _bits(hf)[[1, 2, 3]].astype(np.int64))
        assert d.max() <= 1


def test_presence_and_frequency_count_generated_ids_only():
    x = _row()
    c = count_words(97, prompt_ids=[1, 2], generated_ids=[2, 3, 3, 3])
    a, f = 0.4, 0.15
    y = apply_controls(x, c, ControlParams(presence_penalty=a, frequency_penalty=f))
    exp = x.copy()
    for v, n in ((2, 1), (3, 3)):
        t = F32(F32(f) * F32(n))
        t = F32(t + F32(a))
        exp[v] = F32(x[v] - t)
    assert np.array_equal(_bits(y), _bits(exp)) and _bits(y)[1] == _bits(x)[1]       # id 1 is in the prompt only: untouched
    # one rounding per operation, not a fused multiply-add: f * n rounds up here, and the fused form would not
    f2, n2, a2 = F32(0.1), 3, F32(-0.3)
    assert F32(F32(f2 * F32(n2)) + a2) != F32(np.float64(f2) * n2 + np.float64(a2))
    y2 =apply_controls(np.zeros(4, F32), count_words(4, generated_ids=[0] * n2), ControlParams(presence_penalty=float(a2), frequency_penalty=float(f2)))
    assert _bits(y2)[0] == _bits(F32(F32(0) - F32(F32(f2 * F32(n2)) + a2)))[()]


def test_logit_bias_and_ban():
    x = _row()
    y = apply_controls(x, count_words(97), ControlParams(logit_bias={4: 2.5, 8: -np.inf, 96: -1.0}))
    exp = x.copy()
    exp[4], exp[8], exp[96] = F32(x[4] + F32(2.5)), -np.inf, F32(x[96] - F32(1.0))
    assert np.array_equal(_bits(y), _bits(exp))


def test_min_new_tokens_masks_eos_by_token_index():
    x = _row()
    p = ControlParams(min_new_tokens=3)
    for k in range(5):
        y = apply_controls(x, count_words(97), p, eos_id=2, token_index=k)
        assert (y[2] == -np.inf) == (k < 3) and np.array_equal(_bits(np.delete(y, 2)), _bits(np.delete(x, 2)))
    assert np.array_equal(_bits(apply_controls(x, count_words(97), p, eos_id=-1, token_index=0)), _bits(x))     # no EOS id: no-op


def test_order_of_the_steps():
    """repetition → presence / frequency → bias → EOS mask, on one column that every step touches."""
    x = np.full(8, 2.0, F32)
    x[1] = F32(-2.0)
    c = count_words(8, prompt_ids=[0, 1], generated_ids=[0, 0, 1])
    p = ControlParams(repetition_penalty=1.7, presence_penalty=0.3, frequency_penalty=0.2, logit_bias={0: 0.9, 1: 0.9, 3: 5.0}, min_new_tokens=2)
    y = apply_controls(x, c, p, eos_id=3, token_index=1)
    for v, n in ((0, 2), (1, 1)):
        e = x[v] * F32(1.7) if x[v] < 0 else x[v] * F32(p.rep_inv)
        t = F32(F32(F32(0.2) * F32(n)) + F32(0.3))
        e = F32(F32(e - t) + F32(0.9))
        assert _bits(y)[v] == _bits(e)[()]
        wrong = F32(x[v] + F32(0.9))                                          # bias first would scale the bias too
        wrong = wrong * F32(1.7) if wrong < 0 else wrong * F32(p.rep_inv)
        assert _bits(F32(wrong - t))[()] != _bits(y)[v]
    assert y[3] == -np.inf                                                    # the mask beats the +5 bias on the EOS column
    assert apply_controls(x, c, p, eos_id=3, token_index=2)[3] == F32(7.0)


def test_from_request():
    assert ControlParams.from_request({}) is None
    assert ControlParams.from_request(dict(repetition_penalty=None, presence_penalty=None, logit_bias=None)) is None
    assert ControlParams.from_request(dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0, logit_bias={}, min_new_tokens=0)) is None
    p = ControlParams.from_request(dict(repetition_penalty=1.2, logit_bias={3: -np.inf}, min_new_tokens=np.int64(4), do_sample=True), vocab=10)
    assert p.repetition_penalty == 1.2 and p.logit_bias == ((3, -np.inf),) and p.min_new_tokens == 4
    assert p.as_dict() == dict(repetition_penalty=1.2, presence_penalty=0.0, frequency_penalty=0.0, logit_bias={3: -np.inf}, min_new_tokens=4)
    with pytest.raises(ValueError, match="outside the vocabulary"):
        ControlParams.from_request(dict(logit_bias={10: 1.0}), vocab=10)


BAD = [dict(repetition_penalty=0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("inf")), dict(repetition_penalty=float("nan")),
       dict(repetition_penalty="1.2"), dict(repetition_penalty=True), dict(repetition_penalty=1e-45), dict(presence_penalty=float("nan")),
       dict(presence_penalty=float("inf")), dict(frequency_penalty=float("-inf")), dict(frequency_penalty=[0.1]), dict(frequency_penalty=1e39),
       dict(logit_bias=[(1, 2.0)]), dict(logit_bias={i: 0.5 for i in range(17)}), dict(logit_bias={-1: 0.5}), dict(logit_bias={1.5: 0.5}),
       dict(logit_bias={"3": 0.5}), dict(logit_bias={3: float("inf")}), dict(logit_bias={3: float("nan")}), dict(logit_bias={3: None}),
       dict(min_new_tokens=-1), dict(min_new_tokens=2.5), dict(min_new_tokens=True)]


@pytest.mark.parametrize("bad", BAD, ids=[f"{list(b)[0]}-{i}" for i, b in enumerate(BAD)])
def test_malformed_values_are_refused(bad):
    with pytest.raises(ValueError, match=list(bad)[0]):
        ControlParams.from_request(bad)
    assert ControlParams(logit_bias={i: 0.5 for i in range(16)}).logit_bias[15] == (15, 0.5)


def _stub_agent(world=1):
    from seedx_amd.seed_x import ContinuousLVLM
    llm = types.SimpleNamespace(comm=types.SimpleNamespace(world=world), V=500)
    return ContinuousLVLM(llm, None, None)


def test_engines_refuse_before_touching_anything():
    """Malformed values, agent.speculative, force_image_at on the same request and tp > 1: ValueError from a stand-in LLM that has
    nothing but ``comm.world`` and ``V`` — nothing else was looked at. Each message names the follow-up."""
    from seedx_amd.seed_x import ContinuousLVLM
    bare = ContinuousLVLM(object(), None, None)
    ok, bad = dict(input_ids=[[1, 2]]), dict(input_ids=[[1, 2]], repetition_penalty=0.0)
    for call in (bare.generate_batch, bare.generate_inflight):
        with pytest.raises(ValueError, match="repetition_penalty must be a finite number > 0"):
            call(None, [ok, bad])
    ctl = dict(input_ids=[[1, 2]], repetition_penalty=1.3)
    with pytest.raises(ValueError, match="force_image_at.*follow-up"):
        bare.generate_batch(None, [ok, ctl], force_image_at=2)
    with pytest.raises(ValueError, match="request 1 carries logits controls and force_image_at.*follow-up"):
        bare.generate_inflight(None, [ok, dict(ctl, force_image_at=2)])
    bare.speculative = True
    with pytest.raises(ValueError, match="logits controls with agent.speculative are not built \\(follow-up"):
        bare.generate_inflight(None, [ok, ctl])
    tp = _stub_agent(world=2)
    with pytest.raises(ValueError, match="logits controls on tp=2 tensor-parallel ranks are not built \\(follow-up"):
        tp.generate_batch(None, [ok, dict(ctl, do_sample=True, seed=1)])
    with pytest.raises(ValueError, match="logits controls on tp=2 tensor-parallel ranks are not built \\(follow-up"):
        tp.generate_inflight(None, [ok, ctl])
    one = _stub_agent()
    for call in (one.generate_batch, one.generate_inflight):
        with pytest.raises(ValueError, match="logit_bias id 500 lies outside the vocabulary"):
            call(None, [dict(ctl, logit_bias={500: 1.0})])


def test_generate_takes_the_keys_as_kwargs():
    """generate forwards the five names to generate_batch's request dict; a malformed one is refused there before the LLM is used."""
    import inspect
    from seedx_amd.seed_x import ContinuousLVLM
    sig = inspect.signature(ContinuousLVLM.generate)
    assert all(k in sig.parameters for k in sampling.CONTROL_KEYS)
    agent = ContinuousLVLM(types.SimpleNamespace(G=1), None, None)
    with pytest.raises(ValueError, match="min_new_tokens must be an int >= 0"):
        agent.generate(None, input_ids=[[1, 2]], min_new_tokens=-3)


def test_decode_step_refusals_are_spelled_out():
    src = open(os.path.join(ROOT, "seed-x_amd", "llama.py")).read()
    assert "logits controls in the verify step of speculative decoding" in src and "logits controls on tp={self.tp}" in src


def test_abi():
    """sx_logits_ctl_args: header field order == ctypes struct; the two entry points declared, bound and exported."""
    from seedx_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "seedx_hip.h")).read()
    body = re.search(r"typedef struct sx_logits_ctl_args \{(.*?)\} sx_logits_ctl_args;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip().lstrip("*") for n in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl).split(",")]
    assert names == [f[0] for f in _lib.LogitsCtlArgs._fields_]
    assert names == ["on", "counts", "work", "rep", "rep_inv", "presence", "frequency", "min_new", "bias_ids", "bias", "token_index",
                     "ld_counts", "eos_id"]
    assert ctypes.sizeof(_lib.LogitsCtlArgs) == 11 * 8 + 2 * 4
    for name in ("sx_next_b_ctl", "sx_next_slots_ctl"):
        assert name in _lib.SIGNATURES and re.search(r"\bint " + name + r"\(", src)
    assert len(_lib.SIGNATURES["sx_next_b_ctl"]) == len(_lib.SIGNATURES["sx_sample_next_b_lp"]) + 1
    assert len(_lib.SIGNATURES["sx_next_slots_ctl"]) == len(_lib.SIGNATURES["sx_sample_next_slots_lp"]) + 1
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, n) for n in ("sx_next_b_ctl", "sx_next_slots_ctl"))
    assert callable(ops.next_b_ctl) and callable(ops.next_slots_ctl)
