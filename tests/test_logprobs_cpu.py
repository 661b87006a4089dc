"""Token log-probabilities, host side: the fp64 rule the kernels are held to (seedx_amd.sampling.token_logprobs), the validation of the
``"logprobs"`` request key, the assembly of a result's ``'logprobs'`` entry, and the C-ABI of the three new entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from seedx_amd import sampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rule_normalises_and_orders():
    rng = np.random.default_rng(0)
    x = (rng.normal(size=(6, 333)) * 4).astype(np.float32)
    chosen, ids, top = sampling.token_logprobs(x, targets=[0, 5, 332, 7, 7, 100], n_top=8)
    _, all_ids, full = sampling.token_logprobs(x, n_top=333)
    assert np.abs(np.log(np.exp(full).sum(axis=1))).max() < 1e-12           # logsumexp(lp) = 0
    for r, t in enumerate([0, 5, 332, 7, 7, 100]):
        assert chosen[r] == full[r][list(all_ids[r]).index(t)]
        assert list(ids[r]) == list(np.argsort(-x[r], kind="stable")[:8]) and (np.diff(top[r]) <= 0).all()
        assert np.array_equal(top[r], full[r][:8])
    one = sampling.token_logprobs(x[2], targets=332, n_top=3)                # a 1-D row: no leading axis
    assert one[0] == chosen[2] and list(one[1]) == list(ids[2][:3]) and one[2].shape == (3,)
    assert sampling.token_logprobs(x[2], n_top=0)[0] is None


def test_rule_ties_inf_and_short_rows():
    x = np.array([1.0, 3.0, 3.0, -np.inf, 0.0, 3.0], dtype=np.float32)
    chosen, ids, top = sampling.token_logprobs(x, targets=3, n_top=8)
    assert list(ids) == [1, 2, 5, 0, 4, 3, -1, -1]                           # ties: lowest index first; past V: -1
    assert chosen == -np.inf and top[5] == -np.inf and (top[6:] == -np.inf).all() and top[0] == top[1] == top[2]
    assert abs(np.exp(top[:5]).sum() - 1.0) < 1e-12
    flat = sampling.token_logprobs(np.full(5, 7.0, dtype=np.float32), targets=4, n_top=2)
    assert abs(flat[0] + np.log(5)) < 1e-15 and list(flat[1]) == [0, 1]
    big = sampling.token_logprobs(np.array([3e4, -3e4, 3e4 - 1], dtype=np.float32), targets=2, n_top=1)
    assert abs(big[0] - (-1 - np.log1p(np.exp(-1.0)))) < 1e-12 and list(big[1]) == [0]
    assert np.isnan(sampling.token_logprobs(x, targets=6)[0]) and np.isnan(sampling.token_logprobs(x, targets=-1)[0])


def test_rule_nan_rows():
    x = np.array([[0.0, np.nan, 2.0], [0.0, 1.0, 2.0], [-np.inf] * 3], dtype=np.float32)
    chosen, ids, top = sampling.token_logprobs(x, targets=[0, 0, 0], n_top=2)
    assert np.isnan(chosen[0]) and np.isnan(top[0]).all() and list(ids[0]) == [-1, -1]
    assert np.isfinite(chosen[1]) and list(ids[1]) == [2, 1]
    assert np.isnan(chosen[2]) and list(ids[2]) == [-1, -1]                  # nothing but -inf: no distribution


@pytest.mark.parametrize("bad", [9, -1, 1.5, True, False, "3", [1]])
def test_request_validation_refuses(bad):
    with pytest.raises(ValueError, match="logprobs must be an int in 0 .. 8"):
        sampling.logprobs_from_request({"logprobs": bad})


def test_request_validation_accepts():
    assert sampling.logprobs_from_request({}) is None and sampling.logprobs_from_request({"logprobs": None}) is None
    assert [sampling.logprobs_from_request({"logprobs": n}) for n in (0, 3, 8, np.int64(2))] == [0, 3, 8, 2]


def test_engine_refuses_bad_n_before_touching_anything():
    """generate_batch / generate_inflight / score validate before they look at the LLM: a stand-in without a single attribute suffices."""
    from seedx_amd.seed_x import ContinuousLVLM
    agent = ContinuousLVLM(object(), None, None)
    for call in (agent.generate_batch, agent.generate_inflight):
        with pytest.raises(ValueError, match="logprobs must be an int in 0 .. 8"):
            call(None, [dict(input_ids=[[1, 2]]), dict(input_ids=[[1, 2]], logprobs=9)])
    with pytest.raises(ValueError, match="n_top must be an int in 0 .. 8"):
        agent.score(None, [dict(input_ids=[[1, 2]], continuations=[[3]])], n_top=9)


def test_result_assembly_and_trimming():
    ids = torch.tensor([5, 6, 7])
    chosen = torch.tensor([-0.5, float("nan"), -2.0])
    top_ids = torch.arange(12).reshape(3, 4)
    top = -torch.arange(12, dtype=torch.float32).reshape(3, 4)
    r = sampling.logprobs_result(ids, chosen, top_ids, top, 2)
    assert sorted(r) == ["token_ids", "token_logprobs", "top_ids", "top_logprobs"]
    assert r["token_ids"] is ids and r["token_logprobs"] is chosen
    assert torch.equal(r["top_ids"], top_ids[:, :2]) and torch.equal(r["top_logprobs"], top[:, :2])
    r0 = sampling.logprobs_result(ids, chosen, top_ids, top, 0)
    assert r0["top_ids"].shape == (3, 0) and r0["top_logprobs"].shape == (3, 0)
    with pytest.raises(AssertionError):
        sampling.logprobs_result(ids, chosen[:2], top_ids, top, 1)
    with pytest.raises(AssertionError):
        sampling.logprobs_result(ids, chosen, top_ids, top, 5)               # more than the buffers hold


def test_abi():
    """sx_logprob_args: header field order == ctypes struct; the three entry points declared, bound and exported."""
    from seedx_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "seedx_hip.h")).read()
    body = re.search(r"typedef struct sx_logprob_args \{(.*?)\} sx_logprob_args;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip().lstrip("*") for n in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl).split(",")]
    assert names == [f[0] for f in _lib.LogprobArgs._fields_]
    for name in ("sx_token_logprobs", "sx_sample_next_b_lp", "sx_sample_next_slots_lp"):
        assert name in _lib.SIGNATURES and re.search(r"\bint " + name + r"\(", src)
    assert len(_lib.SIGNATURES["sx_sample_next_b_lp"]) == len(_lib.SIGNATURES["sx_sample_next_b"]) + 1
    assert len(_lib.SIGNATURES["sx_sample_next_slots_lp"]) == len(_lib.SIGNATURES["sx_sample_next_slots"]) + 1
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, n) for n in ("sx_token_logprobs", "sx_sample_next_b_lp", "sx_sample_next_slots_lp"))
    assert callable(ops.token_logprobs) and callable(ops.next_b_lp) and callable(ops.next_slots_lp)
