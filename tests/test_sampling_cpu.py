"""Seeded sampling, host side: Philox known answers, the fp64 statement of the rule against transformers' own warpers, the C-ABI of
the two sampling entry points and the validation of SamplingParams (no GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAM_SETS = [(0.7, 50, 0.5), (1.0, 0, 0.9), (1.3, 8, 1.0), (1.0, 50, 0.95)]
DELTA = 1e-5


def boundary_margin(larger, kept, top_p):
    """Distance of the nucleus decision from top_p: over the kept tokens and the first dropped one (the smallest larger-mass among the
    top-k survivors that were dropped)."""
    m = np.abs(larger[kept] - top_p).min()
    dropped = np.isfinite(larger) & ~kept
    if dropped.any():
        m = min(m, abs(larger[dropped].min() - top_p))
    return m


def test_philox_known_answers():
    from seedx_amd.sampling import philox4x32_10
    cases = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
             ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in cases:
        assert " ".join("%08x" % w for w in philox4x32_10(ctr, key)) == want


def test_uniform_is_a_24_bit_fraction():
    from seedx_amd.sampling import philox4x32_10, uniform
    seen = set()
    for seed in (0, 1, 0xdeadbeef, (1 << 64) - 1, 0x0123456789abcdef):
        for n in (0, 1, 2, 77, 100000):
            u = uniform(seed, n)
            assert 0.0 <= u < 1.0 and (u * 2 ** 24) == int(u * 2 ** 24)
            assert u == (philox4x32_10((n, 0, 0, 0), (seed & 0xffffffff, seed >> 32))[0] >> 8) / 2 ** 24
            seen.add(u)
    assert len(seen) == 25
    assert uniform(1 << 32, 0) != uniform(0, 0)           # the high word of the seed is part of the key


@pytest.mark.parametrize("T,top_k,top_p", PARAM_SETS)
def test_reference_next_agrees_with_transformers_warpers(T, top_k, top_p):
    """kept_mask == the finite scores and probs == softmax of the warped scores (1e-6) after TemperatureLogitsWarper → TopKLogitsWarper
    → TopPLogitsWarper, in fp64; rows decided within 1e-5 of top_p are left out (at most 10 %). The id follows from probs and u."""
    torch = pytest.importorskip("torch")
    lp = pytest.importorskip("transformers.generation.logits_process")
    from seedx_amd.sampling import nucleus, reference_next
    rows = np.random.default_rng(0).normal(size=(64, 500)) * 3.0
    warpers = [lp.TemperatureLogitsWarper(T)] + ([lp.TopKLogitsWarper(top_k)] if top_k > 0 else []) + [lp.TopPLogitsWarper(top_p)]
    left_out = 0
    for r, x in enumerate(rows):
        kept_n, _, larger = nucleus(x, T, top_k, top_p)
        if boundary_margin(larger, kept_n, top_p) < DELTA:
            left_out += 1
            continue
        scores = torch.from_numpy(x.copy()).unsqueeze(0)
        for wp in warpers:
            scores = wp(None, scores)
        u = ((r * 0.61803398875) % 1.0)
        idx, kept, probs = reference_next(x, T, top_k, top_p, u)
        want_kept = torch.isfinite(scores[0]).numpy()
        assert np.array_equal(kept, want_kept), (r, kept.sum(), want_kept.sum())
        want = torch.softmax(scores[0], dim=-1).numpy()
        assert np.abs(probs - want).max() < 1e-6
        assert abs(probs.sum() - 1.0) < 1e-12 and kept[idx]
        cdf = np.cumsum(want)
        assert idx == int(np.nonzero(cdf > u * cdf[-1])[0][0])
    assert left_out <= 0.1 * len(rows), left_out


def test_reference_next_hand_cases():
    from seedx_amd.sampling import reference_next
    x = np.log(np.array([0.1, 0.4, 0.2, 0.3]))
    # top_p 0.5: larger masses are 0.9, 0, 0.7, 0.4 → kept {1, 3}; renormalised 4/7, 3/7
    idx, kept, probs = reference_next(x, 1.0, 0, 0.5, 0.5)
    assert kept.tolist() == [False, True, False, True] and np.allclose(probs, [0, 4 / 7, 0, 3 / 7]) and idx == 1
    assert reference_next(x, 1.0, 0, 0.5, 0.6)[0] == 3
    # equal values are kept or dropped together; ties at the k-th value survive top-k
    idx, kept, _ = reference_next(np.array([1.0, 2.0, 1.0, 0.0]), 1.0, 2, 1.0, 0.999)
    assert kept.tolist() == [True, True, True, False] and idx == 2
    assert reference_next(np.array([1.0, 2.0, 1.0, 0.0]), 1.0, 1, 1.0, 0.999)[0] == 1
    assert reference_next(x, 1.0, 0, 1e-6, 0.99)[0] == 1     # the maximum is always kept


def test_sample_abi_in_sync():
    """sx_sample_args: header field order == ctypes struct; both entry points declared, bound and exported."""
    from seedx_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "seedx_hip.h")).read()
    body = re.search(r"typedef struct sx_sample_args \{(.*?)\} sx_sample_args;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            decl = re.sub(r"^(const\s+)?(void|float|int32_t|uint32_t)\s*\*?", "", decl)
            names += [n.strip().lstrip("*") for n in decl.split(",")]
    assert names == [f[0] for f in _lib.SampleArgs._fields_]
    assert names == ["do_sample", "temperature", "top_k", "top_p", "seed", "token_index", "n_kept", "p_chosen"]
    assert ctypes.sizeof(_lib.SampleArgs) == 8 * 8
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("sx_sample_next_b", "sx_sample_next_slots"):
        assert re.search(r"\bint %s\s*\(" % name, plain) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["sx_sample_next_b"]) == len(_lib.SIGNATURES["sx_greedy_next_b"]) + 1
    assert re.search(r"sx_sample_next_slots\(const sx_slot_step_args\* args, const sx_sample_args\* sample, void\* stream\)", plain)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "sx_sample_next_b") and hasattr(lib, "sx_sample_next_slots")
    assert callable(ops.sample_next_b) and callable(ops.sample_next_slots)


def test_sampling_params_validation():
    from seedx_amd.sampling import SamplingParams
    p = SamplingParams(do_sample=True)
    assert (p.temperature, p.top_k, p.top_p) == (0.7, 50, 0.5) and 0 <= p.seed < 1 << 64      # seed=None: drawn and reported
    assert SamplingParams(do_sample=True).seed != p.seed or SamplingParams(do_sample=True).seed != p.seed
    assert SamplingParams(True, 1.0, 0, 1.0, (1 << 64) - 1).seed == (1 << 64) - 1
    for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan")),
                dict(top_p=0.0), dict(top_p=1.0001), dict(top_p=-0.1), dict(top_k=-1), dict(seed=-1), dict(seed=1 << 64)):
        with pytest.raises(ValueError):
            SamplingParams(do_sample=True, **bad)
    assert SamplingParams.from_request(dict(prompt="x")) is None and SamplingParams.from_request(dict(do_sample=False, seed=3)) is None
    q = SamplingParams.from_request(dict(do_sample=True, top_p=0.9, seed=7, temperature=None))
    assert (q.do_sample, q.temperature, q.top_k, q.top_p, q.seed) == (True, 0.7, 50, 0.9, 7)


def test_unseeded_sampling_is_refused_on_tensor_parallel_ranks():
    """Each tensor-parallel rank builds its own SamplingParams, so seed=None would give every rank another os.urandom seed and other
    ids: from_request refuses it for world > 1, and generate / generate_batch reach that guard before they touch the device."""
    from types import SimpleNamespace

    from seedx_amd.sampling import SamplingParams
    from seedx_amd.seed_x import ContinuousLVLM
    with pytest.raises(ValueError, match="seed"):
        SamplingParams.from_request(dict(do_sample=True), world=2)
    with pytest.raises(ValueError, match="seed"):
        SamplingParams.from_request(dict(do_sample=True, seed=None, top_p=0.9), world=8)
    assert SamplingParams.from_request(dict(do_sample=True, seed=5), world=2).seed == 5
    assert SamplingParams.from_request(dict(do_sample=False), world=2) is None            # greedy requests need no seed
    assert SamplingParams.from_request(dict(do_sample=True), world=1).seed >= 0           # single rank: drawn and reported
    agent = object.__new__(ContinuousLVLM)
    agent.llm = SimpleNamespace(G=1, comm=SimpleNamespace(world=2, rank=0))
    with pytest.raises(ValueError, match="seed"):
        agent.generate_batch(None, [dict(input_ids=[[1, 2]], do_sample=True)])
    with pytest.raises(ValueError, match="seed"):
        agent.generate(None, input_ids=[[1, 2]], do_sample=True)


def test_entry_points_carry_the_sampling_arguments():
    import inspect

    from seedx_amd.llama import LlamaForCausalLM, SampleState, SlotState
    from seedx_amd.seed_x import ContinuousLVLM
    sig = inspect.signature(ContinuousLVLM.generate).parameters
    assert sig["do_sample"].default is False and sig["top_k"].default == 50 and sig["seed"].default is None
    assert sig["temperature"].default == 0.7 and sig["top_p"].default == 0.5
    assert inspect.signature(LlamaForCausalLM.decode_step).parameters["sampling"].default is None
    assert inspect.signature(LlamaForCausalLM.slot_state).parameters["sampling"].default is False
    assert "sampling" in inspect.signature(SlotState.__init__).parameters and hasattr(SampleState, "key")
