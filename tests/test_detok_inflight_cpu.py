"""In-flight batching of the de-tokenizer, host side (no GPU): the per-request schedule tables, the request checks of
``generate_inflight`` and the schedule that ``inflight.simulate`` predicts for it."""
import numpy as np
import pytest
import torch

from seedx_amd import inflight
from seedx_amd.detokenizer import EulerDiscreteScheduler, SDXLAdapter, SDXLAdapterWithLatentImage, slot_schedule


@pytest.mark.parametrize("n", [1, 2, 7, 30, 50, 128])
def test_slot_tables_equal_set_timesteps(n):
    """A slot's table rows are the scheduler's own tables for the request's step count, zero padded to max_steps; the padding holds
    sigma_next = 0 of the last step and nothing a live slot reads beyond it."""
    max_steps = 128
    sig, ts, init, s0 = slot_schedule(EulerDiscreteScheduler(), n, max_steps)
    ref = EulerDiscreteScheduler()
    ref.set_timesteps(n)
    assert sig.shape == (max_steps + 1,) and ts.shape == (max_steps,) and sig.dtype == ts.dtype == torch.float32
    assert torch.equal(sig[:n + 1], ref.sigmas) and torch.equal(ts[:n], ref.timesteps)
    assert float(sig[n]) == 0.0 and not sig[n + 1:].any() and not ts[n:].any()
    assert init == ref.init_noise_sigma and s0 == float(ref.sigmas[0])


def test_slot_tables_refuse_steps_out_of_range():
    for n in (0, -1, 9):
        with pytest.raises(ValueError, match=r"num_inference_steps must be in 1\.\.8"):
            slot_schedule(EulerDiscreteScheduler(), n, 8)


def _ok(**kw):
    r = dict(image_embeds=torch.zeros(1, 16, 256), seed=1, num_inference_steps=3, guidance_scale=5.0)
    r.update(kw)
    return r


def _drop(r, *keys):
    return {k: v for k, v in r.items() if k not in keys}


BAD = [
    ("not a dict", [3], "a request is a dict"),
    ("unknown key", _ok(steps=3), r"unknown keys \['steps'\]"),
    ("edit key on the t2i adapter", _ok(image_guidance_scale=1.5), r"unknown keys \['image_guidance_scale'\]"),
    ("no image source", _drop(_ok(), "image_embeds"), "exactly one of image_pil / image_tensor / image_embeds"),
    ("two image sources", _ok(image_tensor=torch.zeros(3, 8, 8)), "exactly one of image_pil / image_tensor / image_embeds"),
    ("neither seed nor latents", _drop(_ok(), "seed"), "exactly one of seed / latents"),
    ("seed and latents", _ok(latents=torch.zeros(1, 4, 16, 16)), "exactly one of seed / latents"),
    ("steps 0", _ok(num_inference_steps=0), r"num_inference_steps must be an int in 1\.\.8"),
    ("steps past max_steps", _ok(num_inference_steps=9), r"num_inference_steps must be an int in 1\.\.8"),
    ("steps not an int", _ok(num_inference_steps=2.5), "num_inference_steps must be an int"),
    ("default steps past max_steps", _drop(_ok(), "num_inference_steps"), r"num_inference_steps must be an int in 1\.\.8"),
    ("guidance not a number", _ok(guidance_scale="7"), "guidance_scale must be a finite number"),
    ("guidance not finite", _ok(guidance_scale=float("nan")), "guidance_scale must be a finite number"),
    ("two generations of embeds", _ok(image_embeds=torch.zeros(2, 16, 256)), "image_embeds must be .*ONE generation"),
    ("two generations of image tensors", _drop(_ok(image_tensor=torch.zeros(2, 3, 8, 8)), "image_embeds"), "image_tensor must be .*ONE generation"),
    ("image_pil not an image", _drop(_ok(image_pil=[1, 2]), "image_embeds"), "image_pil must be a PIL image"),
    ("a list of seeds", _ok(seed=[1, 2]), "seed must be one int"),
    ("two generations of latents", _drop(_ok(latents=torch.zeros(2, 4, 16, 16)), "seed"), "latents must be .*ONE generation"),
    ("latents of another size", _drop(_ok(latents=torch.zeros(1, 4, 32, 32)), "seed"), r"latents must be \[4, 16, 16\] or \[1, 4, 16, 16\] for 128x128"),
]


@pytest.mark.parametrize("what,req,msg", BAD, ids=[b[0] for b in BAD])
def test_request_validation_messages(what, req, msg):
    """Every malformed request is a ValueError that names the request, raised before anything is touched: the adapter here has no
    models and no pipe, so touching anything would be another error."""
    ad = SDXLAdapter(None, None)
    with pytest.raises(ValueError, match=msg) as ei:
        ad.generate_inflight([_ok(), req], slots=2, height=128, width=128, max_steps=8)
    assert "request 1" in str(ei.value) and ad.last_inflight_stats is None


def test_edit_adapter_request_keys_and_call_arguments():
    ad = SDXLAdapterWithLatentImage(None, None, set_trainable_late=True)
    good = _ok(image_guidance_scale=2.0, image_latents=torch.zeros(1, 4, 16, 16))
    with pytest.raises(RuntimeError, match="init_pipe"):                # a well-formed queue gets as far as the missing pipe
        ad.generate_inflight([good], slots=2, height=128, width=128, max_steps=8)
    with pytest.raises(ValueError, match="image_latents must be .*ONE generation"):
        ad.generate_inflight([_ok(image_latents=torch.zeros(2, 4, 16, 16))], slots=2, height=128, width=128, max_steps=8)
    with pytest.raises(ValueError, match="image_guidance_scale must be a finite number"):
        ad.generate_inflight([_ok(image_guidance_scale=None)], slots=2, height=128, width=128, max_steps=8)
    t2i = SDXLAdapter(None, None)
    for kw, msg in ((dict(slots=0), "slots must be an int >= 1"), (dict(max_steps=0), "max_steps must be an int >= 1"),
                    (dict(max_admit=0), "max_admit must be None or an int >= 1"), (dict(height=100), "multiples of 8")):
        with pytest.raises(ValueError, match=msg):
            t2i.generate_inflight([_ok()], **dict(dict(slots=2, height=128, width=128, max_steps=8), **kw))
    assert t2i.generate_inflight([], slots=2, height=128, width=128) == [] and t2i.last_inflight_stats["unet_steps"] == 0


@pytest.mark.parametrize("G,max_admit", [(4, None), (3, None), (2, 1), (8, 3)])
def test_predicted_schedule(G, max_admit):
    """A request of s steps is a 'sequence of s + 1 tokens' for inflight.simulate: the admission stands for token 1 and takes no UNet
    step, every UNet step for one more. The counts are what generate_inflight reports (decode_steps -> unet_steps, prefill_passes ->
    admission_passes). No request finishes at its admission, so a pass is one round; the steps of a queue are never more than those
    of lock-step waves and never fewer than the work divided by the slots."""
    steps = [2, 5, 3, 1, 4, 2, 3]
    sim = inflight.simulate([s + 1 for s in steps], G, max_admit)
    assert sim["live_slot_steps"] == sum(steps) and sim["admissions"] == len(steps)
    assert sim["live_slot_steps"] + sim["parked_slot_steps"] == G * sim["decode_steps"]
    assert -(-sum(steps) // G) <= sim["decode_steps"]
    if max_admit is None:
        assert sim["decode_steps"] <= inflight.lockstep_wave_steps([s + 1 for s in steps], G)
    # the engine's loop, restated on the host: admit rounds, then one step for the live slots, harvest by the host mirror
    sch = inflight.SlotScheduler(G, len(steps), max_admit)
    left, got = {}, dict(unet_steps=0, admission_passes=0, order=[])
    while not sch.done:
        sch.new_pass()
        while True:
            adm = sch.admit()
            if not adm:
                break
            got["admission_passes"] += 1
            left.update({g: steps[r] for g, r in adm})
        live = sch.live_slots()
        if not live:
            continue
        got["unet_steps"] += 1
        for g in live:
            left[g] -= 1
            if left[g] == 0:
                got["order"].append(sch.finish(g))
    assert got == dict(unet_steps=sim["decode_steps"], admission_passes=sim["prefill_passes"], order=sim["finish_order"])


def test_mixed_queue_step_ratio_of_the_bench_workload():
    """The workload of tools/bench_detok_inflight.py: 32 requests, steps drawn from 20..50 by default_rng(0), 8 slots."""
    steps = [int(s) for s in np.random.default_rng(0).integers(20, 51, 32)]
    sim = inflight.simulate([s + 1 for s in steps], 8)
    waves = inflight.lockstep_wave_steps([s + 1 for s in steps], 8)
    assert waves == sum(max(steps[i:i + 8]) for i in range(0, 32, 8)) and sim["decode_steps"] < waves
