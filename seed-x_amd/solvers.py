"""The DPM-Solver++(2M) rule of the de-tokenizer, stated once, on the host, in numpy (no torch, no GPU): the Karras sigma spacing, the
sigma -> timestep map, the per-step coefficient table that the device kernels read, and one step in fp64 — the reference of
sx_cfg_dpmpp2m_step(_slots) (csrc/glue_inline.h: cfg_dpmpp2m_elem).

Lu et al. 2022, "DPM-Solver++" [PAPERS.md], Algorithm 2 (multistep, second order, data prediction) in the sigma parametrisation of the
denoise loops: the sample x is the sigma-space latent (x = x0 + sigma * noise), the model sees x / sqrt(sigma^2 + 1), lambda = -ln sigma.
Step i goes from sigma = sig[i] to sigma' = sig[i + 1] with h = lambda' - lambda and h_last = lambda - lambda_prev:

    a = sigma' / sigma,  b = -expm1(-h),  c = h / (2 h_last)          (c = 0 on step 0 and on the step with sigma' = 0, where a = 0, b = 1)
    d  = x0 + c (x0 - x0_prev)                                        (x0_prev is NOT read when c = 0)
    x' = a x + b d,  x0_prev <- x0,  scaled = x' / sqrt(sigma'^2 + 1)

x0 is the guided denoised sample: mode 0 (branches [uncond, text]) e = e_u + gs (e_t - e_u), x0 = x - sigma e; mode 1 (branches [text,
image, uncond]) x0_b = x - sigma e_b, x0 = x0_u + gs (x0_t - x0_i) + igs (x0_i - x0_u). With c = 0 a step is the Euler step
x + (x - x0) / sigma (sigma' - sigma), because 1 - e^-h = 1 - sigma' / sigma. The table is computed here; the kernels take no logarithm
and no exponential."""
import numpy as np


def karras_sigmas(sig_min, sig_max, n, rho=7.0):
    """n sigmas from sig_max down to sig_min, uniform in sigma^(1/rho) (Karras et al. 2022, eq. 5); the end points are the inputs."""
    if n < 1:
        raise ValueError(f"karras_sigmas: n must be >= 1, got {n}")
    if not 0.0 < sig_min < sig_max:
        raise ValueError(f"karras_sigmas: need 0 < sig_min < sig_max, got {sig_min}, {sig_max}")
    lo, hi = float(sig_min) ** (1.0 / rho), float(sig_max) ** (1.0 / rho)
    s = (hi + np.linspace(0.0, 1.0, n) * (lo - hi)) ** rho
    s[-1] = sig_min
    s[0] = sig_max
    return s


def sigma_to_t(sigmas, train_sigmas):
    """Fractional training timestep of every sigma: linear interpolation in ln sigma over the (increasing) training sigmas. Not rounded."""
    train = np.asarray(train_sigmas, dtype=np.float64)
    return np.interp(np.log(np.asarray(sigmas, dtype=np.float64)), np.log(train), np.arange(len(train), dtype=np.float64))


def dpmpp2m_coefficients(sigmas, dtype=np.float32):
    """sigmas: the n + 1 decreasing sigmas of a schedule (the last may be 0). Returns [n, 3] rows (a, b, c) of the module docstring,
    computed in fp64 and rounded once to ``dtype``."""
    sig = np.asarray(sigmas, dtype=np.float64)
    n = len(sig) - 1
    out = np.zeros((max(n, 0), 3), dtype=np.float64)
    for i in range(n):
        s, sn = sig[i], sig[i + 1]
        if not s > sn >= 0.0:
            raise ValueError(f"dpmpp2m_coefficients: sigmas must decrease and stay >= 0, got {s} -> {sn} at step {i}")
        if sn == 0.0:
            out[i] = (0.0, 1.0, 0.0)
            continue
        h = np.log(s) - np.log(sn)                               # lambda' - lambda
        c = h / (2.0 * (np.log(sig[i - 1]) - np.log(s))) if i > 0 else 0.0
        out[i] = (sn / s, -np.expm1(-h), c)
    return out.astype(dtype)


def guided_x0(x, eps, sigma, gs, igs, mode):
    """The guided denoised sample of the module docstring; eps [nb, ...] ordered by guidance branch."""
    if mode == 0:
        eu, et = eps[0], eps[1]
        return x - sigma * (eu + gs * (et - eu))
    if mode == 1:
        x0t, x0i, x0u = x - sigma * eps[0], x - sigma * eps[1], x - sigma * eps[2]
        return x0u + gs * (x0t - x0i) + igs * (x0i - x0u)
    raise ValueError(f"dpmpp2m_step: mode must be 0 or 1, got {mode}")


def dpmpp2m_step(x, eps, x0_prev, sigma, sigma_next, abc, gs, igs, mode):
    """One step in fp64. x [...], eps [nb, ...], x0_prev [...] (not read when c = 0: may be None or hold NaN), abc = (a, b, c) of this
    step. Returns (x', x0, x' / sqrt(sigma_next^2 + 1))."""
    x, eps = np.asarray(x, dtype=np.float64), np.asarray(eps, dtype=np.float64)
    a, b, c = (float(v) for v in abc)
    x0 = guided_x0(x, eps, float(sigma), float(gs), float(igs), mode)
    d = x0 if c == 0.0 else x0 + c * (x0 - np.asarray(x0_prev, dtype=np.float64))
    xn = a * x + b * d
    return xn, x0, xn / np.sqrt(float(sigma_next) ** 2 + 1.0)
