"""In-flight batching of the de-tokenizer on the GPU: the three per-slot kernels against the lock-step kernels they are compiled with
(``torch.equal``), and ``generate_inflight`` of both adapters against ``_DenoiseLoop.run`` at the same G filled with G copies of each
request (``torch.equal``: same UNet launches at the same batch shape, and the rows of a UNet batch do not see each other — which the
precondition test establishes first). Mini models of tests/test_adapter_e2e_gpu.py, 128 px, ``image_embeds`` conditioning."""
import types

import pytest
import torch

from seedx_amd import inflight
from tests.test_adapter_e2e_gpu import _build
from tests.test_detok_inflight_cpu import BAD

pytestmark = pytest.mark.gpu

SENTINEL = 1234.5
KW = dict(height=128, width=128, max_steps=8, output_type="latent")


# ---------------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------------
def _sig_tab(n_steps, ld, dev):
    from seedx_amd.detokenizer import EulerDiscreteScheduler, slot_schedule
    return torch.stack([slot_schedule(EulerDiscreteScheduler(), n, ld - 1)[0] for n in n_steps]).to(dev)


@pytest.mark.parametrize("mode,nb,ld", [(0, 2, 4), (1, 3, 8)])
def test_cfg_euler_step_slots_equals_lockstep_kernel_per_slot(dev, mode, nb, ld):
    """G = 3 slots of 35 x 4 = 140 elements (no multiple of a wave) at steps [0, n - 1, parked]: the first step, the last one
    (sigma_next = 0) and a parked slot, each with its own guidance scales, equal sx_cfg_euler_step run on clones of the slot's rows.
    Then a slot with step >= n_steps. A parked slot's latents, all its rows of scaled_next, and channels 4..7 everywhere keep the
    sentinel the buffers were filled with."""
    from seedx_amd import ops
    G, HW, C = 3, 35, 4
    n_steps = [4, 6, 5]
    g_ = torch.Generator().manual_seed(mode)
    eps = torch.randn(nb * G, HW, C, generator=g_).to(dev)
    lat0 = (torch.randn(G, HW, C, generator=g_) * 5).to(dev)
    sig = _sig_tab(n_steps, 9, dev)
    nst = torch.tensor(n_steps, dtype=torch.int32, device=dev)
    gs, igs = [7.5, 3.25, 1.1], [1.5, 2.75, 0.3]
    gs_d, igs_d = torch.tensor(gs, device=dev), torch.tensor(igs, device=dev)
    for steps in ([0, n_steps[1] - 1, -1], [n_steps[0], 1, n_steps[2] + 3]):
        live = [0 <= s < n for s, n in zip(steps, n_steps)]
        assert not all(live) and any(live)
        lat = lat0.clone()
        for g in range(G):
            if not live[g]:
                lat[g] = SENTINEL
        start = lat.clone()
        scaled = torch.full((nb * G, HW, ld), SENTINEL, device=dev)
        ops.cfg_euler_step_slots(eps, lat, scaled, sig, torch.tensor(steps, dtype=torch.int32, device=dev), nst, gs_d, igs_d, nb, C, ld, mode)
        sc = scaled.view(nb, G, HW, ld)
        for g in range(G):
            if not live[g]:
                assert (lat[g] == SENTINEL).all() and (sc[:, g] == SENTINEL).all(), (steps, g)
                continue
            lat_r = start[g:g + 1].clone()
            sc_r = torch.full((nb, HW, ld), SENTINEL, device=dev)
            ops.cfg_euler_step(eps.view(nb, G, HW, C)[:, g].contiguous(), lat_r, sc_r, sig[g].contiguous(),
                               torch.tensor([steps[g]], dtype=torch.int32, device=dev), nb, C, ld, gs[g], igs[g], mode)
            assert torch.equal(lat[g], lat_r[0]) and not torch.equal(lat[g], start[g]), (steps, g)
            assert torch.equal(sc[:, g], sc_r), (steps, g)
            assert (sc[:, g, :, C:] == SENTINEL).all() and not (sc[:, g, :, :C] == SENTINEL).any()
    # the last step of slot 1 ends on sigma_next = 0: its scaled input is the latents themselves
    assert float(sig[1, n_steps[1]]) == 0.0


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("nb", [2, 3])
@pytest.mark.parametrize("dim", [32, 320])
def test_timestep_embedding_slots_equals_lockstep_kernel_row_by_row(dev, dim, nb, dtype):
    from seedx_amd import ops
    from seedx_amd.detokenizer import EulerDiscreteScheduler, slot_schedule
    G, steps = 3, [2, -1, 0]
    t_tab = torch.stack([slot_schedule(EulerDiscreteScheduler(), n, 8)[1] for n in (3, 5, 8)]).to(dev)
    out = ops.timestep_embedding_slots(t_tab, torch.tensor(steps, dtype=torch.int32, device=dev), nb, dim, dtype)
    assert out.shape == (nb * G, dim) and out.dtype == dtype and torch.isfinite(out.float()).all()
    for g, s in enumerate(steps):
        t = t_tab[g, s:s + 1].contiguous() if s >= 0 else torch.zeros(1, device=dev)         # a parked slot embeds t = 0
        ref = ops.timestep_embedding(t, dim, dtype)
        for k in range(nb):
            assert torch.equal(out[k * G + g], ref[0]), (g, k)
    assert not torch.equal(out[0], out[2])


def test_denoise_advance(dev):
    from seedx_amd import ops
    step = torch.tensor([0, 3, -1, 4], dtype=torch.int32, device=dev)
    n = torch.tensor([1, 5, 5, 5], dtype=torch.int32, device=dev)
    ops.denoise_advance(step, n)
    assert step.tolist() == [-1, 4, -1, -1]
    ops.denoise_advance(step, n)
    assert step.tolist() == [-1, -1, -1, -1] and n.tolist() == [1, 5, 5, 5]


# ---------------------------------------------------------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------------------------------------------------------
STEPS = [2, 5, 3, 1, 4, 2, 3]
GUIDANCE = [7.5, 3.0, 5.25, 1.0, 9.5, 2.125, 6.0]


@pytest.fixture(scope="module")
def t2i(dev):
    from seedx_amd.detokenizer import SDXLAdapter
    ad, _ = _build(dev, torch.float16, 4, SDXLAdapter)
    g = torch.Generator().manual_seed(11)
    feats = torch.randn(len(STEPS), 1, 16, 256, generator=g).to(dev)
    noise = torch.randn(len(STEPS), 1, 4, 16, 16, generator=g)
    reqs = [dict(image_embeds=feats[i], latents=noise[i], num_inference_steps=STEPS[i], guidance_scale=GUIDANCE[i], input_image_size=112)
            for i in range(len(STEPS))]
    return ad, reqs


def _reference(ad, loop, req, G, mode=0):
    """Row 0 of _DenoiseLoop.run at G filled with G copies of the request: conditioning from get_image_embeds on the request alone,
    the request's own steps and guidance."""
    pe, pe_neg, pool, pool_neg = ad.get_image_embeds(image_embeds=req["image_embeds"], return_negative=True, image_size=112)
    n = req["num_inference_steps"]
    ad.scheduler.set_timesteps(n)
    lat = req["latents"].to(ad.device, torch.float32) * ad.scheduler.init_noise_sigma
    rep = lambda t: t.expand(G, *t.shape[1:])
    if mode == 0:
        ehs, pooled = torch.cat([rep(pe_neg), rep(pe)]), torch.cat([rep(pool_neg), rep(pool)])
        out = loop.run(0, rep(lat).contiguous(), ehs, pooled, ad._time_ids(128, 128, 2 * G), ad.scheduler, n, req["guidance_scale"])
    else:
        il = req["image_latents"].to(ad.device, torch.float32) if req.get("image_latents") is not None else torch.zeros(1, 4, 16, 16, device=ad.device)
        il3 = torch.cat([rep(il), rep(il), torch.zeros_like(rep(il))])
        ehs, pooled = torch.cat([rep(pe), rep(pe_neg), rep(pe_neg)]), torch.cat([rep(pool), rep(pool_neg), rep(pool_neg)])
        out = loop.run(1, rep(lat).contiguous(), ehs, pooled, ad._time_ids(128, 128, 3 * G), ad.scheduler, n, req["guidance_scale"],
                       req["image_guidance_scale"], il3)
    return out[:1].clone()


def _expect_stats(stats, steps, G, captures, max_admit=None):
    sim = inflight.simulate([s + 1 for s in steps], G, max_admit)
    assert stats == dict(unet_steps=sim["decode_steps"], live_slot_steps=sim["live_slot_steps"], parked_slot_steps=sim["parked_slot_steps"],
                         admissions=sim["admissions"], admission_passes=sim["prefill_passes"], graph_captures=captures), (stats, sim)


def test_precondition_rows_of_a_unet_batch_do_not_see_each_other(dev, t2i):
    """What per-slot equality rests on, in the lock-step loop as it stands: at G = 4, permuting the generations permutes the output,
    and replacing a generation's neighbours leaves its row unchanged. If this fails, a slot cannot equal a lock-step row bit for bit,
    and the engine tests below say nothing."""
    from seedx_amd.detokenizer import _DenoiseLoop
    ad, reqs = t2i
    G, n, gs = 4, 3, 6.0
    loop = _DenoiseLoop(ad.unet, use_graph=True)
    cond = [ad.get_image_embeds(image_embeds=r["image_embeds"], return_negative=True, image_size=112) for r in reqs]
    ad.scheduler.set_timesteps(n)
    init = ad.scheduler.init_noise_sigma

    def run(order):
        pe, pe_neg, pool, pool_neg = (torch.cat([cond[i][k] for i in order]) for k in range(4))
        lat = torch.cat([reqs[i]["latents"] for i in order]).to(dev, torch.float32) * init
        return loop.run(0, lat, torch.cat([pe_neg, pe]), torch.cat([pool_neg, pool]), ad._time_ids(128, 128, 2 * G), ad.scheduler, n, gs).clone()

    base = run([0, 1, 2, 3])
    perm = [2, 0, 3, 1]
    assert torch.equal(run(perm), base[perm]), "permuting the generations of a UNet batch does not permute its output"
    assert torch.equal(run([0, 4, 5, 6])[0], base[0]), "a generation's row depends on its neighbours"
    assert torch.equal(run([6, 5, 4, 3])[3], base[3])
    assert not torch.equal(base[0], base[1])


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("G", [4, 3])
def test_t2i_queue_equals_lockstep_rows(dev, t2i, G, graph):
    """7 requests with steps [2, 5, 3, 1, 4, 2, 3] and seven guidance scales on 4 slots (UNet batch 8: two kernel chains) and on 3
    (batch 6: also two chains, of 3 rows): every result equals row 0 of the lock-step loop at the same G filled with copies of the
    request; the step counts are the simulated schedule's; the slot step is captured once for the whole queue, and not again for a
    second queue with other steps and guidance."""
    from seedx_amd.detokenizer import _DenoiseLoop
    ad, reqs = t2i
    ad._loop.use_graph = graph
    ad._slot_loop = None
    try:
        outs = ad.generate_inflight(reqs, slots=G, **KW)
        stats = dict(ad.last_inflight_stats)
        ref_loop = _DenoiseLoop(ad.unet, use_graph=graph)
        assert ref_loop._chains_for(2 * G) == 2
        refs = [_reference(ad, ref_loop, r, G) for r in reqs]
        for i, (o, r) in enumerate(zip(outs, refs)):
            assert o.shape == (1, 4, 16, 16) and torch.isfinite(o).all()
            assert torch.equal(o, r), f"request {i} ({STEPS[i]} steps, guidance {GUIDANCE[i]}) on {G} slots: max |diff| {(o - r).abs().max().item():.3e}"
        assert len({tuple(o.flatten().tolist()[:8]) for o in outs}) == len(outs)
        _expect_stats(stats, STEPS, G, 1 if graph else 0)
        # a second queue, other steps and guidance, with an admission quota: same state, same graph
        second = [dict(reqs[i], num_inference_steps=n, guidance_scale=gs) for i, n, gs in ((4, 1, 4.5), (0, 6, 8.0), (2, 2, 1.75), (5, 3, 7.5))]
        outs2 = ad.generate_inflight(second, slots=G, max_admit=1, **KW)
        _expect_stats(ad.last_inflight_stats, [r["num_inference_steps"] for r in second], G, 1 if graph else 0, max_admit=1)
        assert torch.equal(outs2[1], _reference(ad, ref_loop, second[1], G))
        assert torch.equal(outs2[3], _reference(ad, ref_loop, second[3], G))
    finally:
        ad._loop.use_graph = True
        ad._slot_loop = None


def test_seed_requests_draw_generate_s_noise(dev, t2i):
    """A request with a seed gets the noise generate() draws for that seed."""
    ad, reqs = t2i
    r = dict(reqs[2])
    del r["latents"]
    r["seed"] = 5
    out = ad.generate_inflight([r, dict(reqs[2], latents=ad._noise(5, 128, 128, 1))], slots=2, **KW)
    assert torch.equal(out[0], out[1])
    ad._slot_loop = None


def test_edit_queue_equals_lockstep_rows(dev):
    """The edit adapter (8-channel UNet, three guidance branches): 3 requests on 2 slots with distinct image_guidance_scale, one
    without a source image (zero image latents)."""
    from seedx_amd.detokenizer import SDXLAdapterWithLatentImage, _DenoiseLoop
    ad, _ = _build(dev, torch.float16, 8, SDXLAdapterWithLatentImage)
    g = torch.Generator().manual_seed(12)
    feats = torch.randn(3, 1, 16, 256, generator=g).to(dev)
    noise = torch.randn(3, 1, 4, 16, 16, generator=g)
    il = torch.randn(3, 1, 4, 16, 16, generator=g)
    steps, gs, igs = [3, 1, 2], [7.5, 4.0, 2.5], [1.5, 2.25, 0.75]
    reqs = [dict(image_embeds=feats[i], latents=noise[i], num_inference_steps=steps[i], guidance_scale=gs[i], image_guidance_scale=igs[i],
                 input_image_size=112) for i in range(3)]
    reqs[0]["image_latents"], reqs[2]["image_latents"] = il[0], il[2]            # request 1: no source image
    outs = ad.generate_inflight(reqs, slots=2, **KW)
    _expect_stats(ad.last_inflight_stats, steps, 2, 1)
    ref_loop = _DenoiseLoop(ad.unet, use_graph=True)
    for i, o in enumerate(outs):
        r = _reference(ad, ref_loop, reqs[i], 2, mode=1)
        assert torch.equal(o, r), f"edit request {i}: max |diff| {(o - r).abs().max().item():.3e}"


def test_generate_is_unchanged_by_an_inflight_call(dev, t2i):
    """The lock-step loop's state and graph are its own: generate() before and after a generate_inflight call returns equal latents
    and keeps its graph."""
    ad, reqs = t2i
    kw = dict(image_embeds=torch.cat([reqs[0]["image_embeds"], reqs[1]["image_embeds"]]), latents=torch.cat([reqs[0]["latents"], reqs[1]["latents"]]),
              num_inference_steps=3, height=128, width=128, input_image_size=112, output_type="latent")
    before = ad.generate(**kw).clone()
    graph = ad._loop._graph
    assert graph is not None
    ad.generate_inflight(reqs[:3], slots=2, **KW)
    after = ad.generate(**kw)
    assert torch.equal(before, after) and ad._loop._graph is graph
    ad._slot_loop = None


@pytest.mark.parametrize("what,req,msg", BAD, ids=[b[0] for b in BAD])
def test_refusals_touch_nothing(dev, t2i, what, req, msg):
    ad, reqs = t2i
    ad.last_inflight_stats, ad._slot_loop = None, None
    with pytest.raises(ValueError, match=msg):
        ad.generate_inflight([reqs[0], req], slots=2, height=128, width=128, max_steps=8)
    assert ad.last_inflight_stats is None and ad._slot_loop is None


@pytest.mark.parametrize("where", ["loop", "unet"])
def test_refuses_more_than_one_rank(dev, t2i, where):
    from seedx_amd.detokenizer import _SlotDenoiseLoop
    ad, reqs = t2i
    holder = ad._loop if where == "loop" else ad.unet
    real = holder.comm
    holder.comm = types.SimpleNamespace(world=2, rank=0, graph_safe=True)
    try:
        ad.last_inflight_stats, ad._slot_loop = None, None
        with pytest.raises(ValueError, match=r"one rank: the (denoise loop|UNet) has comm.world = 2"):
            ad.generate_inflight(reqs[:2], slots=2, **KW)
        assert ad.last_inflight_stats is None and ad._slot_loop is None
        with pytest.raises(ValueError, match="comm.world = 2"):
            _SlotDenoiseLoop(ad.unet, comm=holder.comm if where == "loop" else None)
    finally:
        holder.comm = real
