"""DPM-Solver++(2M) next to Euler in the de-tokenizer (bench.py's adapter construction at full SDXL dimensions, synthetic weights, fp16, no
VAE decode: latents out). ONE process, device-synchronised clocks:

  kernel : us per launch of sx_cfg_dpmpp2m_step and sx_cfg_dpmpp2m_step_slots (and their Euler twins beside them) on 128 x 128 x 4 latents
           (a 1024 px generation), modes 0 and 1, --launches launches between two device events, the median of --reps such windows.
  gen    : ms per generation at --size px, one generation per call: Euler at 50 steps against 2M over Karras sigmas at 25 and at 20
           steps, the median of --gen-reps calls after one warm-up call (which captures the graph). One UNet evaluation per step for
           both solvers, so the time follows the step count.

No gate is set on either: the step kernel costs microseconds beside a UNet step. WHAT IS NOT MEASURED: image quality at fewer steps on the
real checkpoint. The accuracy figures of the solver are those of the Gaussian toy of tests/test_dpm_solver_cpu.py.

    python tools/bench_dpm_solver.py --out profiles/dpm_solver.md
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from seedx_amd import ops
from seedx_amd.detokenizer import DPMSolverMultistepScheduler, EulerDiscreteScheduler, slot_schedule

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--gen-reps", type=int, default=3)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--skip-gen", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda:0")
LINES = []


def emit(d):
    LINES.append(json.dumps(d))
    print(LINES[-1], flush=True)


def us_per_launch(fn):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / a.launches)
    return out


# ---- kernel -------------------------------------------------------------------------------------------------------------------
HW, Cl, STEPS = (a.size // 8) ** 2, 4, 25
sch = DPMSolverMultistepScheduler(use_karras_sigmas=True)
sig, _, _, _, coef = slot_schedule(sch, STEPS, STEPS)
sig, coef = sig.to(dev), coef.to(dev)
g = torch.Generator(device=dev).manual_seed(0)
for mode in (0, 1):
    nb, ld = 2 + mode, 4 * (1 + mode)
    eps = torch.randn(nb, HW, Cl, device=dev, generator=g)
    lat, old = torch.randn(1, HW, Cl, device=dev, generator=g), torch.randn(1, HW, Cl, device=dev, generator=g)
    scaled = torch.zeros(nb, HW, ld, device=dev)
    step = torch.full((1,), 7, dtype=torch.int32, device=dev)                    # mid-way: c != 0, x0_prev is read
    nst = torch.full((1,), STEPS, dtype=torch.int32, device=dev)
    gs, igs = torch.full((1,), 7.5, device=dev), torch.full((1,), 1.5, device=dev)
    runs = {
        "sx_cfg_euler_step": lambda: ops.cfg_euler_step(eps, lat, scaled, sig, step, nb, Cl, ld, 7.5, 1.5, mode),
        "sx_cfg_dpmpp2m_step": lambda: ops.cfg_dpmpp2m_step(eps, lat, old, scaled, sig, coef[:STEPS], step, nb, Cl, ld, 7.5, 1.5, mode),
        "sx_cfg_euler_step_slots": lambda: ops.cfg_euler_step_slots(eps, lat, scaled, sig[None], step, nst, gs, igs, nb, Cl, ld, mode),
        "sx_cfg_dpmpp2m_step_slots": lambda: ops.cfg_dpmpp2m_step_slots(eps, lat, old, scaled, sig[None], coef[None], step, nst, gs, igs, nb, Cl, ld, mode),
    }
    for name, fn in runs.items():
        lat.normal_(generator=g)                                                  # the step is applied over and over: start each kernel from fresh, finite latents
        us = us_per_launch(fn)
        emit(dict(what="kernel", entry=name, mode=mode, HW=HW, C=Cl, ld_scaled=ld, launches=a.launches, us=[round(x, 2) for x in us],
                  median_us=round(statistics.median(us), 2)))

# ---- generation ---------------------------------------------------------------------------------------------------------------
if not a.skip_gen:
    bench.USE_VAE = False
    _, _, ad = bench.build_models(dev, torch.float16, need=("adapter",))
    gen = torch.Generator().manual_seed(0)
    feats = torch.randn(1, 64, 4096, generator=gen).to(dev)                      # what the LLM's output resampler hands over
    noise = torch.randn(1, 4, a.size // 8, a.size // 8, generator=gen)
    for name, scheduler, steps in (("Euler", EulerDiscreteScheduler(), 50), ("2M + Karras", DPMSolverMultistepScheduler(use_karras_sigmas=True), 25),
                                   ("2M + Karras", DPMSolverMultistepScheduler(use_karras_sigmas=True), 20)):
        ad.scheduler = scheduler
        ms = []
        for rep in range(a.gen_reps + 1):                                         # call 0 captures the graph
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = ad.generate(image_embeds=feats, latents=noise, num_inference_steps=steps, guidance_scale=7.5, height=a.size, width=a.size,
                              output_type="latent")
            torch.cuda.synchronize()
            if rep:
                ms.append((time.perf_counter() - t0) * 1e3)
        assert bool(torch.isfinite(out).all())
        emit(dict(what="gen", solver=name, steps=steps, size=a.size, ms=[round(x, 1) for x in ms], median_ms=round(statistics.median(ms), 1),
                  ms_per_step=round(statistics.median(ms) / steps, 2)))

if a.out:
    rows = [json.loads(x) for x in LINES]
    k = "\n".join(f"| `{r['entry']}` | {r['mode']} | {r['median_us']} | {r['us']} |" for r in rows if r["what"] == "kernel")
    gen_rows = [r for r in rows if r["what"] == "gen"]
    gtab = "\n".join(f"| {r['solver']} | {r['steps']} | {r['median_ms']} | {r['ms_per_step']} | {r['ms']} |" for r in gen_rows) or "| not measured (--skip-gen) | | | | |"
    with open(a.out, "w") as fh:
        fh.write(f"""# DPM-Solver++(2M) in the de-tokenizer: step kernels and generation time

`python tools/bench_dpm_solver.py --out {a.out}` — MI355X, one process, device-synchronised clocks. No gate is set on these numbers.

## Step kernels

{HW} x {Cl} latents (one {a.size} px generation), step 7 of a 25-step Karras schedule (c != 0: `x0_prev` is read), {a.launches} launches between
two device events, {a.reps} windows; launches from Python through ctypes, so the figure holds the launch path as well as the kernel. The
slot kernels run G = 1 live slot.

| entry point | mode | median us per launch | windows |
|---|---|---|---|
{k}

## Generation

Full SDXL UNet (synthetic weights), fp16, {a.size} x {a.size}, one generation per call, latents out (no VAE decode), graph replay; the median
of {a.gen_reps} calls after the call that captures the graph. Both solvers take one UNet evaluation per step.

| solver | steps | median ms per generation | ms per step | calls |
|---|---|---|---|---|
{gtab}

## Not measured

Image quality at fewer steps on the real checkpoint. The solver's accuracy is known on the Gaussian toy model of
`tests/test_dpm_solver_cpu.py` only (error at sigma = 0 over Karras sigmas: 2M at 25 steps 5.2e-3, Euler at 50 steps 3.1e-2 and at 100
steps 1.6e-2); whether 25 or 20 steps of 2M match 50 Euler steps on images is for whoever holds the checkpoint to judge.

## Raw lines

```
""" + "\n".join(LINES) + "\n```\n")
