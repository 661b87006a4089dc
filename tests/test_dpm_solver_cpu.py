"""DPM-Solver++(2M) on the host, numpy and fp64 only (seedx_amd/solvers.py and the scheduler class that fills its tables): the rule is
pinned by its own properties, because no other implementation of it is installed.

The toy model of the convergence test is Gaussian data of standard deviation S = 0.8: denoised(x, sigma) = x S^2 / (S^2 + sigma^2). Its
probability-flow ODE dx/dsigma = (x - denoised) / sigma = x sigma / (S^2 + sigma^2) has the closed form
x(sigma) = x(sigma_0) sqrt((S^2 + sigma^2) / (S^2 + sigma_0^2)), so the error of a solver at sigma = 0 is known exactly. The model is
linear in x, so the error relative to the largest exact value is the same for every element of x."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 0.8


def train_sigmas():
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float32).astype(np.float64) ** 2
    ac = np.cumprod(1.0 - betas)
    return ((1.0 - ac) / ac) ** 0.5


def leading_sigmas(n):
    """The SDXL schedule of EulerDiscreteScheduler in fp64: n sigmas at the `leading` timesteps (offset 1), then 0."""
    ts = (np.arange(0, n) * (1000 // n)).round()[::-1].astype(np.float64) + 1
    tr = train_sigmas()
    return np.concatenate([np.interp(ts, np.arange(len(tr)), tr), [0.0]])


def karras(n):
    from seedx_amd import solvers
    s = leading_sigmas(n)
    return np.concatenate([solvers.karras_sigmas(s[-2], s[0], n), [0.0]])


def denoised(x, sigma):
    return x * S * S / (S * S + sigma * sigma)


def toy_eps(x, sigma):
    """The noise prediction of the toy model, once per guidance branch (both branches alike: guidance changes nothing)."""
    e = (x - denoised(x, sigma)) / sigma
    return np.stack([e, e])


def run_2m(sig, x):
    from seedx_amd import solvers
    co = solvers.dpmpp2m_coefficients(sig, np.float64)
    old = None
    for i in range(len(sig) - 1):
        x, old, _ = solvers.dpmpp2m_step(x, toy_eps(x, sig[i]), old, sig[i], sig[i + 1], co[i], 7.5, 1.5, 0)
    return x


def run_euler(sig, x):
    for i in range(len(sig) - 1):
        x = x + (x - denoised(x, sig[i])) / sig[i] * (sig[i + 1] - sig[i])
    return x


def toy_errors(n):
    sig = karras(n)
    x = np.random.default_rng(0).standard_normal(16) * np.sqrt(sig[0] ** 2 + S * S)
    exact = x * np.sqrt(S * S / (S * S + sig[0] ** 2))
    rel = lambda got: float(np.abs(got - exact).max() / np.abs(exact).max())
    return rel(run_2m(sig, x.copy())), rel(run_euler(sig, x.copy()))


def test_order_of_convergence_on_the_gaussian_toy():
    """Over Karras sigmas: halving the step size cuts the 2M error by more than 3 (10 -> 20 -> 40 steps), Euler's by less than 2.1, and
    2M at 25 steps is below Euler at 100."""
    err = {n: toy_errors(n) for n in (10, 20, 25, 40, 100)}
    for n, (m2, eu) in err.items():
        print(f"{n:4d} steps: 2M {m2:.3e}  Euler {eu:.3e}")
    assert err[10][0] / err[20][0] > 3.0 and err[20][0] / err[40][0] > 3.0, err
    assert err[10][1] / err[20][1] < 2.1 and err[20][1] / err[40][1] < 2.1, err
    assert err[10][1] / err[20][1] > 1.0 and err[20][1] / err[40][1] > 1.0, err
    assert err[25][0] < err[100][1], err


@pytest.mark.parametrize("mode", [0, 1])
def test_first_order_identity_with_euler(mode):
    """With c = 0 every step is the Euler step x + (x - x0) / sigma (sigma' - sigma), to 1e-12 relative: 1 - e^-h = 1 - sigma' / sigma."""
    from seedx_amd import solvers
    rng = np.random.default_rng(1)
    gs, igs = 7.5, 1.5
    for sig in (leading_sigmas(50), karras(25)):
        co = solvers.dpmpp2m_coefficients(sig, np.float64)
        co[:, 2] = 0.0
        x = rng.standard_normal(64) * sig[0]
        for i in range(len(sig) - 1):
            eps = rng.standard_normal((2 + mode, 64))
            xn, x0, scaled = solvers.dpmpp2m_step(x, eps, np.full(64, np.nan), sig[i], sig[i + 1], co[i], gs, igs, mode)
            ref = x + (x - solvers.guided_x0(x, eps, sig[i], gs, igs, mode)) / sig[i] * (sig[i + 1] - sig[i])
            scale = np.abs(x).max() + sig[i] * np.abs(eps).max() * (1 + 2 * gs + 2 * igs)
            assert np.abs(xn - ref).max() <= 1e-12 * scale, (mode, i)
            assert np.array_equal(scaled, xn / np.sqrt(sig[i + 1] ** 2 + 1.0)) and np.isfinite(xn).all()
            x = xn
        assert np.array_equal(x, x0)                                # the last step lands on the denoised sample


def test_guided_x0_combinations():
    """mode 0 is x - sigma (e_u + gs (e_t - e_u)); mode 1 with x0_i == x0_u reduces to x0_u + gs (x0_t - x0_u)."""
    from seedx_amd import solvers
    rng = np.random.default_rng(2)
    x, eu, et = rng.standard_normal((3, 8))
    a = solvers.guided_x0(x, np.stack([eu, et]), 2.5, 6.0, 1.5, 0)
    b = solvers.guided_x0(x, np.stack([et, eu, eu]), 2.5, 6.0, 1.5, 1)
    assert np.allclose(a, x - 2.5 * (eu + 6.0 * (et - eu)), rtol=0, atol=1e-13) and np.allclose(a, b, rtol=0, atol=1e-12)
    with pytest.raises(ValueError, match="mode"):
        solvers.guided_x0(x, np.stack([eu, et]), 1.0, 1.0, 1.0, 2)


def test_coefficient_table():
    """50 leading steps: 0 < a < 1 and a + b = 1 to 1e-15 on every step but the last, 0 <= c <= 1.74, c[0] = 0, the last row (0, 1, 0);
    the fp32 table is the fp64 one rounded once."""
    from seedx_amd import solvers
    sig = leading_sigmas(50)
    co = solvers.dpmpp2m_coefficients(sig, np.float64)
    assert co.shape == (50, 3) and co.dtype == np.float64
    a, b, c = co[:-1, 0], co[:-1, 1], co[:-1, 2]
    assert (a > 0).all() and (a < 1).all() and np.abs(a + b - 1.0).max() <= 1e-15
    assert c[0] == 0.0 and (c[1:] > 0).all() and c.max() <= 1.74 and c.max() > 1.7
    assert tuple(co[-1]) == (0.0, 1.0, 0.0)
    co32 = solvers.dpmpp2m_coefficients(sig)
    assert co32.dtype == np.float32 and np.array_equal(co32, co.astype(np.float32))
    assert solvers.dpmpp2m_coefficients(sig[-2:]).tolist() == [[0.0, 1.0, 0.0]]           # one step: straight onto sigma' = 0
    with pytest.raises(ValueError, match="decrease"):
        solvers.dpmpp2m_coefficients([1.0, 2.0, 0.0])


def test_karras_sigmas_and_sigma_to_t():
    from seedx_amd import solvers
    tr = train_sigmas()
    for n in (2, 10, 25):
        s = solvers.karras_sigmas(0.0413, 13.04, n)
        assert s.shape == (n,) and s[0] == 13.04 and s[-1] == 0.0413 and (np.diff(s) < 0).all()
    assert solvers.karras_sigmas(0.5, 2.0, 1).tolist() == [2.0]
    mid = solvers.karras_sigmas(1.0, 128.0, 3, rho=7.0)[1]
    assert abs(mid - ((1.0 + 2.0) / 2) ** 7) < 1e-9                    # uniform in sigma^(1/7): 128^(1/7) = 2
    with pytest.raises(ValueError):
        solvers.karras_sigmas(2.0, 1.0, 5)
    t = solvers.sigma_to_t(tr, tr)
    assert np.abs(t - np.arange(1000)).max() <= 1e-9
    half = solvers.sigma_to_t([np.sqrt(tr[10] * tr[11])], tr)           # the midpoint in ln sigma is t + 1/2: not rounded
    assert abs(half[0] - 10.5) < 1e-9


def test_solvers_module_needs_no_torch():
    """solvers.py is numpy only: loaded on its own as a file in a fresh interpreter, torch stays unimported."""
    import subprocess
    code = ("import importlib.util, sys\n"
            f"spec = importlib.util.spec_from_file_location('solvers', {os.path.join(ROOT, 'seed-x_amd', 'solvers.py')!r})\n"
            "m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)\n"
            "assert m.dpmpp2m_coefficients([2.0, 1.0, 0.0]).shape == (2, 3)\n"
            "assert 'torch' not in sys.modules\n")
    subprocess.run([sys.executable, "-c", code], check=True)


def test_scheduler_tables():
    import torch
    from seedx_amd import solvers
    from seedx_amd.detokenizer import DPMSolverMultistepScheduler, EulerDiscreteScheduler, slot_schedule
    assert DPMSolverMultistepScheduler.order == 2 and EulerDiscreteScheduler.order == 1
    for n in (1, 2, 5, 30, 50):
        e, d = EulerDiscreteScheduler(), DPMSolverMultistepScheduler()
        e.set_timesteps(n)
        d.set_timesteps(n)
        assert torch.equal(e.sigmas, d.sigmas) and torch.equal(e.timesteps, d.timesteps) and e.init_noise_sigma == d.init_noise_sigma
        assert d.coefficients.shape == (n, 3) and d.coefficients.dtype == torch.float32
        assert np.array_equal(d.coefficients.numpy(), solvers.dpmpp2m_coefficients(d.sigmas.numpy()))
        k = DPMSolverMultistepScheduler(use_karras_sigmas=True)
        k.set_timesteps(n)
        assert k.sigmas.shape == (n + 1,) and float(k.sigmas[-1]) == 0.0 and k.sigmas[0] == e.sigmas[0] and k.sigmas[n - 1] == e.sigmas[n - 1]
        assert k.timesteps.shape == (n,) and k.timesteps.dtype == torch.float32 and k.init_noise_sigma == e.init_noise_sigma
        assert (k.sigmas[1:] < k.sigmas[:-1]).all() and k.coefficients.shape == (n, 3) and k.coefficients[-1].tolist() == [0.0, 1.0, 0.0]
        if n > 2:
            assert not torch.equal(k.sigmas, e.sigmas) and (k.timesteps[1:] < k.timesteps[:-1]).all()
            assert float((k.timesteps - k.timesteps.round()).abs().max()) > 0.01           # fractional: not rounded
    # the slot loop's rows: the Euler class keeps its four entries, order 2 adds the zero-padded coefficient rows
    assert len(slot_schedule(EulerDiscreteScheduler(), 3, 8)) == 4
    k = DPMSolverMultistepScheduler(use_karras_sigmas=True)
    sig, ts, init, s0, coef = slot_schedule(k, 3, 8)
    assert coef.shape == (9, 3) and torch.equal(coef[:3], k.coefficients) and not coef[3:].any() and sig.shape == (9,) and ts.shape == (8,)
    assert torch.equal(sig[:4], k.sigmas) and s0 == float(k.sigmas[0])


def test_scheduler_refusals_and_names(tmp_path):
    import json
    from seedx_amd import diffusers_names
    from seedx_amd.detokenizer import DPMSolverMultistepScheduler
    for kw, word in ((dict(solver_order=3), "3"), (dict(algorithm_type="dpmsolver"), "'dpmsolver'"), (dict(timestep_spacing="trailing"), "'trailing'"),
                     (dict(beta_schedule="linear"), "'linear'")):
        with pytest.raises(ValueError, match=word):
            DPMSolverMultistepScheduler(**kw)
    assert diffusers_names.DPMSolverMultistepScheduler is DPMSolverMultistepScheduler
    cfg = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, steps_offset=1, beta_schedule="scaled_linear",
               timestep_spacing="leading", use_karras_sigmas=True, algorithm_type="dpmsolver++", solver_order=2)
    os.makedirs(tmp_path / "scheduler")
    json.dump(cfg, open(tmp_path / "scheduler" / "scheduler_config.json", "w"))
    s = DPMSolverMultistepScheduler.from_pretrained(str(tmp_path), subfolder="scheduler")
    assert s.config["use_karras_sigmas"] is True and s.config["steps_offset"] == 1
    json.dump(dict(cfg, solver_order=3), open(tmp_path / "scheduler" / "scheduler_config.json", "w"))
    with pytest.raises(ValueError, match="solver_order"):
        DPMSolverMultistepScheduler.from_pretrained(str(tmp_path), subfolder="scheduler")


def test_entry_points_declared_and_bound():
    """Both entry points are declared in the header and bound with one ctypes argument per parameter; neither kernel source names LDS or
    an atomic, and the lock-step kernel stays out of elementwise.hip (whose launches the glue matrix pins to its case tables)."""
    import re
    from seedx_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "seedx_hip.h")).read(), flags=re.S)
    for name in ("sx_cfg_dpmpp2m_step", "sx_cfg_dpmpp2m_step_slots"):
        m = re.search(r"\bint " + name + r"\((.*?)\);", src, flags=re.S)
        assert m and name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == m.group(1).count(",") + 1, name
    assert len(_lib.SIGNATURES["sx_cfg_dpmpp2m_step"]) == len(_lib.SIGNATURES["sx_cfg_euler_step"]) + 2           # x0_prev, coef_dev
    assert len(_lib.SIGNATURES["sx_cfg_dpmpp2m_step_slots"]) == len(_lib.SIGNATURES["sx_cfg_euler_step_slots"]) + 2
    csrc = os.path.join(ROOT, "seed-x_amd", "csrc")
    slots, glue = open(os.path.join(csrc, "denoise_slots.hip")).read(), open(os.path.join(csrc, "glue_inline.h")).read()
    assert "cfg_dpmpp2m_kernel" in slots and "cfg_dpmpp2m_slots_kernel" in slots and "cfg_dpmpp2m_elem" in glue
    assert "dpmpp2m" not in open(os.path.join(csrc, "elementwise.hip")).read()
    for text in (slots, glue):
        assert "__shared__" not in text and "atomic" not in text


def test_dropin_serves_the_scheduler():
    """Where the drop-in serves `diffusers`, the name resolves to this class (the same condition as for EulerDiscreteScheduler)."""
    from seedx_amd import dropin
    from seedx_amd.detokenizer import DPMSolverMultistepScheduler
    saved = {k: v for k, v in sys.modules.items() if k == "diffusers" or k == "any_res" or k == "src" or k.startswith("src.")}
    for k in saved:
        del sys.modules[k]
    try:
        dropin.install()
        from diffusers import DPMSolverMultistepScheduler as served, EulerDiscreteScheduler  # noqa: F401
        assert served is DPMSolverMultistepScheduler
    finally:
        dropin.uninstall()
        sys.modules.update(saved)
