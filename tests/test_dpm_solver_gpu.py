"""DPM-Solver++(2M) on the device: sx_cfg_dpmpp2m_step and sx_cfg_dpmpp2m_step_slots against the fp64 rule of seedx_amd/solvers.py, and the
two denoise loops with a scheduler of order 2 (mini models of tests/test_adapter_e2e_gpu.py, 128 px).

THE BOUND of the kernel against ``solvers.dpmpp2m_step`` in fp64 is derived by counting roundings, in the manner of tests/test_glue_matrix_gpu.py
(section 5, the Euler step). u = 2^-24 is the unit roundoff of fp32. The reference computes from the same fp32 x, eps, x0_prev, sigma, gs and igs,
and from the fp64 coefficients (a, b, c) = solvers.dpmpp2m_coefficients(sigmas, float64) of the fp32 sigmas; the kernel reads that table
rounded once to fp32, which costs one relative u per coefficient and is counted below. Terms of order u^2 are dropped, as there.

x0, the guided denoised sample, E0 = its error in units of u, X0 >= |x0|:
  mode 0 (e = e_u + gs (e_t - e_u); x0 = x - sigma e), M = |e_u| + gs |e_t - e_u| >= |e|:
      the subtraction (1, times gs: <= M), gs * (..) + e_u as product and sum (2 of <= M): err(e) <= 3 M. sigma * e: 3 sigma M inherited and 1 of
      its own; the sum: 1 of |x0| <= |x| + sigma M.        E0 = |x| + 5 sigma M,  X0 = |x| + sigma M
  mode 1 (x0_b = x - sigma e_b; x0 = x0_u + gs (x0_t - x0_i) + igs (x0_i - x0_u)), S = (1 + igs) |e_u| + (gs + igs) |e_i| + gs |e_t|:
      the count of test_glue_matrix_gpu.py for the same expression: each x0_b 2 (|x| + sigma |e_b|); each difference inherits two of those and
      adds 1 of its own, times the scale and the product's rounding; the two sums add 1 of the partial sum and 1 of |x0|. Collected:
                                                        E0 = 4 (1 + gs + igs) |x| + 6 sigma S,  X0 = |x| + sigma S
  Where the compiler fuses a product into an fma, or cancels x out of x0_t - x0_i, there are fewer roundings, never more.
d = x0 + c (x0 - x0_prev), T = X0 + |x0_prev| >= |x0 - x0_prev| (T = 0 and d = x0 where c = 0: the kernel does not read x0_prev), D = X0 + c T >= |d|:
      the difference inherits E0 and adds 1 of T; times c: the table's rounding of c (1 of c T), the product (1 of c T); the sum: E0 and 1 of D:
                                                        err(d) <= (1 + c) E0 + X0 + 4 c T
x' = a x + b d: the table's roundings of a and b (1 of a |x|, 1 of b D), the two products (1 of each), the sum (1 of |x'| <= a |x| + b D), and b err(d):
                                                        |x' - ref| <= u (b ((1 + c) E0 + X0 + 4 c T) + 3 (a |x| + b D))
x0_prev' = x0:                                          |x0_prev' - ref| <= u E0
scaled = x' rsqrt(sigma'^2 + 1) against the fp64 quotient of the reference: the bound of x' times the factor, plus 3 u |ref| (the argument's fma
at half weight, v_rsq_f32 within its documented 1 ulp, the product: as for the Euler step).
Every bound has the floor 2^-126, the smallest normal of fp32 (a product may flush below it).

On the last step the table row is (0, 1, 0) exactly, so x' = 0 x + 1 x0 = x0: the test asks for equal values there, on top of the bound.

FIRST-ORDER EQUIVALENCE: with c = 0 the fp64 rule is the fp64 Euler step to 1e-12 (tests/test_dpm_solver_cpu.py), so the two kernels differ by
at most the sum of their two bounds (this one and euler_ref's of tests/test_glue_matrix_gpu.py) plus that 1e-12 of the magnitudes."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests.test_gemm_matrix_gpu import U32
from tests.test_gemv_matrix_gpu import GBuf, same_bits, stops_on_gpu_fault
from tests.test_glue_matrix_gpu import euler_ref, nan_lead

pytestmark = pytest.mark.gpu

F32 = torch.float32
GS, IGS = 7.5, 1.5
FLOOR = 2.0 ** -126
WORST = {}


def lib_():
    from seedx_amd import _lib
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(st, what):
    from seedx_amd import _lib
    _lib.check(st, what)
    torch.cuda.synchronize()


def schedule(n, karras):
    """(sigmas fp32 [n + 1], coefficients fp64 [n, 3] of those sigmas, the fp32 table the kernel reads) of the scheduler class."""
    from seedx_amd import solvers
    from seedx_amd.detokenizer import DPMSolverMultistepScheduler
    s = DPMSolverMultistepScheduler(use_karras_sigmas=karras)
    s.set_timesteps(n)
    co64 = solvers.dpmpp2m_coefficients(s.sigmas.numpy(), np.float64)
    assert np.array_equal(co64.astype(np.float32), s.coefficients.numpy())
    return s.sigmas.clone(), co64, s.coefficients.clone(), s.init_noise_sigma


def ref_step(mode, x, eps, x0p, sigma, sigma_next, abc, gs=GS, igs=IGS):
    """One step in fp64 (solvers.dpmpp2m_step) from the fp32 operands x [n], eps [nb, n], x0p [n] (numpy) and the fp64 coefficients, with the bounds of
    the module docstring: (x', bound, x0, bound, scaled, bound)."""
    from seedx_amd import solvers
    x, eps = x.astype(np.float64), eps.astype(np.float64)
    a, b, c = (float(v) for v in abc)
    xn, x0, sc = solvers.dpmpp2m_step(x, eps, x0p, sigma, sigma_next, abc, gs, igs, mode)
    ax = np.abs(x)
    if mode == 0:
        M = np.abs(eps[0]) + gs * np.abs(eps[1] - eps[0])
        E0, X0 = ax + 5.0 * sigma * M, ax + sigma * M
    else:
        S = (1.0 + igs) * np.abs(eps[2]) + (gs + igs) * np.abs(eps[1]) + gs * np.abs(eps[0])
        E0, X0 = 4.0 * (1.0 + gs + igs) * ax + 6.0 * sigma * S, ax + sigma * S
    T = X0 + np.abs(x0p.astype(np.float64)) if c != 0.0 else 0.0
    D = X0 + c * T
    bx = np.maximum(U32 * (b * ((1.0 + c) * E0 + X0 + 4.0 * c * T) + 3.0 * (a * ax + b * D)), FLOOR)
    b0 = np.maximum(U32 * E0, FLOOR)
    inv = 1.0 / math.sqrt(sigma_next * sigma_next + 1.0)
    return xn, bx, x0, b0, sc, bx * inv + 3.0 * U32 * np.abs(sc)


def held(key, got, ref, bound, what):
    """Every element within its bound (got: an fp32 device tensor, ref / bound: fp64 numpy); prints nothing, records and returns the worst ratio."""
    g = got.detach().cpu().double().numpy().reshape(ref.shape)
    ratio = np.abs(g - ref) / bound
    worst = float(ratio.max()) if ratio.size else 0.0
    WORST[key] = max(WORST.get(key, 0.0), worst)
    if not worst <= 1.0:
        i = int(np.nan_to_num(ratio, nan=np.inf).argmax())
        raise AssertionError(f"{what} [{key}]: {int((~(ratio <= 1.0)).sum())} of {ratio.size} elements beyond the fp64 bound; worst at flat index {i}: got "
                             f"{g.reshape(-1)[i]!r}, ref {ref.reshape(-1)[i]!r}, |diff| {abs(g.reshape(-1)[i] - ref.reshape(-1)[i]):.3e} > bound "
                             f"{bound.reshape(-1)[i]:.3e}")
    return worst


class Bufs:
    """latents, x0_prev and scaled_next of one generation inside guard buffers: only the n elements of the first two and channels < Cc of every
    scaled row may change."""

    def __init__(self, n, nb, HW, Cc, ld, dev, scaled=True):
        self.lat, self.old = GBuf(n, F32, dev), GBuf(n, F32, dev)
        self.lat.allow()[:] = True
        self.old.allow()[:] = True
        self.sc = None
        if scaled:
            self.sc = GBuf(nb * HW * ld, F32, dev)
            self.sc.allow().view(nb * HW, ld)[:, :Cc] = True
        self.nb, self.HW, self.Cc, self.ld = nb, HW, Cc, ld

    def load(self, lat, old):
        self.lat.body.copy_(lat)
        self.old.body.copy_(old)

    def check(self, what):
        self.lat.check(what + " (latents)")
        self.old.check(what + " (x0_prev)")
        if self.sc is not None:
            self.sc.check(what + " (scaled copy: guards and channels >= C)")

    def scaled(self):
        return self.sc.body.view(self.nb, self.HW, self.ld)[:, :, :self.Cc].reshape(self.nb, -1)


def launch(lib, B, eb, sigb, cob, step, nb, n, Cc, ld, mode, what, gs=GS, igs=IGS):
    ok(lib.sx_cfg_dpmpp2m_step(eb.data_ptr(), B.lat.ptr(), B.old.ptr(), B.sc.ptr() if B.sc is not None else None, sigb.data_ptr(), cob.data_ptr(),
                               step.data_ptr(), nb, n, Cc, ld, gs, igs, mode, stream()), what)
    B.check(what)


# ----------------------------------------------------------------------------------------------------------------------------
# the lock-step kernel
# ----------------------------------------------------------------------------------------------------------------------------
WALK = [dict(id=f"mode{mode}-hw{HW}-ld{ld}", mode=mode, HW=HW, ld=ld) for mode in (0, 1) for HW in (1, 63, 64, 4099) for ld in (4, 8)]


@pytest.mark.parametrize("c", WALK, ids=lambda c: c["id"])
@stops_on_gpu_fault
def test_dpmpp2m_step_walks_vs_fp64(dev, c):
    """All steps of a 5-step Karras schedule and of the 50-step leading schedule (sigma 13.1 .. 0.041, then 0), C = 4: the kernel's own latents and
    x0_prev are carried from launch to launch and every step is judged alone against an fp64 step from them. HW = 1, 63, 64 and 4099 (16396
    elements: 65 workgroups, the last one partly filled). x0_prev holds the guard NaN before step 0 and must not reach any output; two identical launches give
    equal bits; guard elements round all three outputs and channels 4..ld-1 of the scaled copy stay untouched; on the last step the latents equal x0."""
    lib = lib_()
    mode, HW, ld, Cc = c["mode"], c["HW"], c["ld"], 4
    n, nb = HW * Cc, 2 + mode
    g = torch.Generator(device=dev).manual_seed(1000 * mode + HW + ld)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    for steps, karras in ((5, True), (50, False)):
        sig, co64, co32, init = schedule(steps, karras)
        assert sig.numel() == steps + 1 and float(sig[steps]) == 0.0 and co32.shape == (steps, 3)
        sigb, cob = nan_lead(sig.to(dev)), nan_lead(co32.to(dev))
        eps = torch.randn(steps, nb, n, device=dev, generator=g)
        A, B = Bufs(n, nb, HW, Cc, ld, dev), Bufs(n, nb, HW, Cc, ld, dev)
        A.lat.body.copy_(torch.randn(n, device=dev, generator=g) * init)
        assert bool(torch.isnan(A.old.body).all()), "x0_prev starts as NaN: step 0 must not read it"
        worst = (0.0, -1)
        for i in range(steps):
            what = f"{c['id']} {steps} steps, step {i}"
            s, sn = float(sig[i]), float(sig[i + 1])
            step.fill_(i)
            prev, prev_old = A.lat.body.clone(), A.old.body.clone()
            B.load(prev, prev_old)
            eb = nan_lead(eps[i])
            xn, bx, x0, b0, sc, bs = ref_step(mode, prev.cpu().numpy(), eps[i].cpu().numpy(), prev_old.cpu().numpy(), s, sn, co64[i])
            launch(lib, A, eb, sigb, cob, step, nb, n, Cc, ld, mode, what)
            launch(lib, B, eb, sigb, cob, step, nb, n, Cc, ld, mode, what + " (second launch)")
            assert same_bits(A.lat.body, B.lat.body) and same_bits(A.old.body, B.old.body) and same_bits(A.scaled(), B.scaled()), f"{what}: two launches differ"
            assert bool(torch.isfinite(A.lat.body).all()) and bool(torch.isfinite(A.old.body).all()) and bool(torch.isfinite(A.scaled()).all()), what
            w = held(("cfg_dpmpp2m_kernel", f"mode {mode}"), A.lat.body, xn, bx, what + " (latents)")
            worst = max(worst, (w, i))
            held(("cfg_dpmpp2m_kernel", f"mode {mode} x0_prev"), A.old.body, x0, b0, what + " (x0_prev)")
            for k in range(nb):
                held(("cfg_dpmpp2m_kernel", f"mode {mode} scaled copy"), A.scaled()[k], sc, bs, what + f" (scaled copy {k})")
            if i == 0:
                assert co64[0][2] == 0.0
            if 0 < i < steps - 1:
                assert co64[i][2] > 0.0
        assert tuple(co64[steps - 1]) == (0.0, 1.0, 0.0)
        assert torch.equal(A.lat.body, A.old.body), f"{c['id']} {steps} steps: the last step must land on x0 (a = 0, b = 1, c = 0)"
        print(f"{c['id']} {steps} steps: worst |diff| / bound {worst[0]:.3f} at step {worst[1]}")


@pytest.mark.parametrize("mode", [0, 1])
@stops_on_gpu_fault
def test_dpmpp2m_step_buffers_and_refusals(dev, mode):
    """scaled_next = NULL gives the same latents and x0_prev; n = 0 is SX_OK and writes nothing; a negative step reads row 0; every documented
    SX_ERR_INVALID case of both entry points returns 1 with a message naming the entry point, and writes nothing."""
    lib = lib_()
    HW, Cc, ld = 37, 4, 8
    n, nb = HW * Cc, 2 + mode
    g = torch.Generator(device=dev).manual_seed(7 + mode)
    sig, co64, co32, init = schedule(5, True)
    sigb, cob = nan_lead(sig.to(dev)), nan_lead(co32.to(dev))
    eb = nan_lead(torch.randn(nb, n, device=dev, generator=g))
    lat0, old0 = torch.randn(n, device=dev, generator=g) * 3, torch.randn(n, device=dev, generator=g)
    step = torch.full((1,), 2, dtype=torch.int32, device=dev)
    A, N = Bufs(n, nb, HW, Cc, ld, dev), Bufs(n, nb, HW, Cc, ld, dev, scaled=False)
    A.load(lat0, old0)
    N.load(lat0, old0)
    launch(lib, A, eb, sigb, cob, step, nb, n, Cc, ld, mode, "with scaled")
    launch(lib, N, eb, sigb, cob, step, nb, n, Cc, ld, mode, "scaled_next = NULL")
    assert same_bits(A.lat.body, N.lat.body) and same_bits(A.old.body, N.old.body) and not torch.equal(A.lat.body, lat0)
    # a negative step is row 0 (c = 0: x0_prev, NaN here, is not read)
    Z, M1 = Bufs(n, nb, HW, Cc, ld, dev), Bufs(n, nb, HW, Cc, ld, dev)
    Z.lat.body.copy_(lat0)
    M1.lat.body.copy_(lat0)
    launch(lib, Z, eb, sigb, cob, step.clone().fill_(0), nb, n, Cc, ld, mode, "step 0")
    launch(lib, M1, eb, sigb, cob, step.clone().fill_(-3), nb, n, Cc, ld, mode, "step -3")
    assert same_bits(Z.lat.body, M1.lat.body) and same_bits(Z.old.body, M1.old.body) and same_bits(Z.scaled(), M1.scaled())
    assert bool(torch.isfinite(Z.lat.body).all())
    # refusals: nothing may be written
    R = Bufs(n, nb, HW, Cc, ld, dev)
    R.lat.allow()[:] = False
    R.old.allow()[:] = False
    R.sc.allow()[:] = False
    s = stream()
    P = dict(eps=eb.data_ptr(), lat=R.lat.ptr(), old=R.old.ptr(), sc=R.sc.ptr(), sig=sigb.data_ptr(), co=cob.data_ptr(), step=step.data_ptr())

    def lock(nb_=nb, n_=n, C_=Cc, ld_=ld, mode_=mode, **null):
        p = dict(P, **{k: None for k in null})
        return lib.sx_cfg_dpmpp2m_step(p["eps"], p["lat"], p["old"], p["sc"], p["sig"], p["co"], p["step"], nb_, n_, C_, ld_, GS, IGS, mode_, s)

    assert lock(n_=0) == 0, "n = 0 is SX_OK"
    bad = [lock(**{k: 1}) for k in ("eps", "lat", "old", "sig", "co", "step")]
    bad += [lock(nb_=5 - nb), lock(nb_=1), lock(nb_=4), lock(mode_=2), lock(mode_=-1), lock(mode_=1 - mode), lock(ld_=Cc - 1), lock(C_=0), lock(n_=n - 1)]
    assert bad == [1] * len(bad), bad
    assert lock(mode_=2) == 1 and b"sx_cfg_dpmpp2m_step: mode/nb" in lib.sx_last_error()
    assert lock(eps=1) == 1 and b"sx_cfg_dpmpp2m_step: null pointer" in lib.sx_last_error()
    assert lock(ld_=3) == 1 and b"sx_cfg_dpmpp2m_step: C/ld" in lib.sx_last_error()
    G = 1
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=dev)
    f32 = lambda v: torch.tensor([v], dtype=F32, device=dev)
    nst, gsd, igsd = i32(5), f32(GS), f32(IGS)
    Q = dict(P, nst=nst.data_ptr(), gs=gsd.data_ptr(), igs=igsd.data_ptr())

    def slots(nb_=nb, G_=G, n_=n, C_=Cc, ld_=ld, mode_=mode, ld_sig=6, **null):
        p = dict(Q, **{k: None for k in null})
        return lib.sx_cfg_dpmpp2m_step_slots(p["eps"], p["lat"], p["old"], p["sc"], p["sig"], p["co"], ld_sig, p["step"], p["nst"], p["gs"], p["igs"], nb_, G_,
                                             n_, C_, ld_, mode_, s)

    bad = [slots(**{k: 1}) for k in ("eps", "lat", "old", "sig", "co", "step", "nst", "gs", "igs")]
    bad += [slots(nb_=5 - nb), slots(nb_=1), slots(mode_=2), slots(mode_=-1), slots(mode_=1 - mode), slots(ld_=Cc - 1), slots(C_=0), slots(n_=n - 1), slots(n_=0),
            slots(G_=0), slots(G_=65536), slots(ld_sig=1)]
    assert bad == [1] * len(bad), bad
    assert slots(old=1) == 1 and b"sx_cfg_dpmpp2m_step_slots: null pointer" in lib.sx_last_error()
    assert slots(mode_=2) == 1 and b"sx_cfg_dpmpp2m_step_slots: mode/nb" in lib.sx_last_error()
    assert slots(ld_=3) == 1 and b"sx_cfg_dpmpp2m_step_slots: C/ld" in lib.sx_last_error()
    torch.cuda.synchronize()
    R.check("refused calls")


@pytest.mark.parametrize("mode", [0, 1])
@stops_on_gpu_fault
def test_zero_c_column_is_the_euler_kernel_within_both_bounds(dev, mode):
    """The 5 Karras steps with an all-zero c column, from the same latents and eps as sx_cfg_euler_step: the latents of the two kernels differ by no more
    than the sum of the two derived bounds (this file's and euler_ref's), plus the 1e-12 by which the two fp64 rules differ."""
    from seedx_amd import ops
    HW, Cc, ld = 257, 4, 4
    n, nb = HW * Cc, 2 + mode
    g = torch.Generator(device=dev).manual_seed(40 + mode)
    sig, co64, co32, init = schedule(5, True)
    co64, co32 = co64.copy(), co32.clone()
    co64[:, 2] = 0.0
    co32[:, 2] = 0.0
    sigd, cod = sig.to(dev), co32.to(dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    lat = torch.randn(1, HW, Cc, device=dev, generator=g) * init
    for i in range(5):
        s, sn = float(sig[i]), float(sig[i + 1])
        step.fill_(i)
        eps = torch.randn(nb, HW, Cc, device=dev, generator=g)
        lat_e, lat_d = lat.clone(), lat.clone()
        old = torch.full_like(lat, float("nan"))
        sce, scd = torch.zeros(nb, HW, ld, device=dev), torch.zeros(nb, HW, ld, device=dev)
        ops.cfg_euler_step(eps, lat_e, sce, sigd, step, nb, Cc, ld, GS, IGS, mode)
        ops.cfg_dpmpp2m_step(eps, lat_d, old, scd, sigd, cod, step, nb, Cc, ld, GS, IGS, mode)
        x, e = lat.reshape(-1), eps.reshape(nb, -1)
        ref_e, be, _, _ = euler_ref(mode, x, e, s, sn, GS, IGS)
        ref_d, bd, _, _, _, _ = ref_step(mode, x.cpu().numpy(), e.cpu().numpy(), old.reshape(-1).cpu().numpy(), s, sn, co64[i])
        ref_e, be = ref_e.cpu().numpy(), be.cpu().numpy()
        scale = np.abs(ref_e) + np.abs(x.cpu().numpy().astype(np.float64))
        assert (np.abs(ref_e - ref_d) <= 1e-12 * (scale + 1.0) * (1.0 + GS + IGS) * 4).all(), f"step {i}: the two fp64 rules differ"
        diff = np.abs(lat_e.reshape(-1).cpu().double().numpy() - lat_d.reshape(-1).cpu().double().numpy())
        ratio = float((diff / (be + bd + np.abs(ref_e - ref_d))).max())
        print(f"mode {mode} step {i}: |euler - 2M(c=0)| / (sum of the bounds) {ratio:.3f}")
        assert ratio <= 1.0, (mode, i, ratio)
        assert bool(torch.isfinite(old).all())
        lat = lat_d


# ----------------------------------------------------------------------------------------------------------------------------
# the per-slot kernel
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,nb,ld", [(0, 2, 4), (1, 3, 8)])
@stops_on_gpu_fault
def test_dpmpp2m_step_slots_equals_lockstep_kernel_per_slot(dev, mode, nb, ld):
    """G = 3 slots with n_steps (1, 2, 5), 35 x 4 elements each and their own guidance scales. Three launches: [step 0 of 1 (first and last at once),
    parked (-1), mid-way]; [step >= n_steps (parked), step 0, the last step]; [parked, the last of two steps, step 1]. Live rows of latents, x0_prev and
    scaled_next equal sx_cfg_dpmpp2m_step on clones of the slot's rows bit for bit; a parked slot keeps the sentinel in all three; channels >= 4 keep it
    everywhere."""
    from seedx_amd import ops
    from seedx_amd.detokenizer import DPMSolverMultistepScheduler, slot_schedule
    SENT = 1234.5
    G, HW, Cc = 3, 35, 4
    n_steps = [1, 2, 5]
    sch = DPMSolverMultistepScheduler(use_karras_sigmas=True)
    rows = [slot_schedule(sch, k, 8) for k in n_steps]
    sig = torch.stack([r[0] for r in rows]).to(dev)
    coef = torch.stack([r[4] for r in rows]).to(dev)
    assert sig.shape == (G, 9) and coef.shape == (G, 9, 3)
    g_ = torch.Generator().manual_seed(5 + mode)
    eps = torch.randn(nb * G, HW, Cc, generator=g_).to(dev)
    lat0 = (torch.randn(G, HW, Cc, generator=g_) * 5).to(dev)
    old0 = torch.randn(G, HW, Cc, generator=g_).to(dev)
    nst = torch.tensor(n_steps, dtype=torch.int32, device=dev)
    gs, igs = [7.5, 3.25, 1.1], [1.5, 2.75, 0.3]
    gs_d, igs_d = torch.tensor(gs, device=dev), torch.tensor(igs, device=dev)
    for steps in ([0, -1, 2], [1, 0, 4], [-1, 1, 1]):
        live = [0 <= s < k for s, k in zip(steps, n_steps)]
        assert not all(live) and sum(live) == 2
        lat, old = lat0.clone(), old0.clone()
        for g in range(G):
            if not live[g]:
                lat[g] = SENT
                old[g] = SENT
            elif steps[g] == 0:
                old[g] = float("nan")                                   # step 0 does not read it
        start, start_old = lat.clone(), old.clone()
        scaled = torch.full((nb * G, HW, ld), SENT, device=dev)
        ops.cfg_dpmpp2m_step_slots(eps, lat, old, scaled, sig, coef, torch.tensor(steps, dtype=torch.int32, device=dev), nst, gs_d, igs_d, nb, Cc, ld, mode)
        sc = scaled.view(nb, G, HW, ld)
        for g in range(G):
            if not live[g]:
                assert (lat[g] == SENT).all() and (old[g] == SENT).all() and (sc[:, g] == SENT).all(), (steps, g)
                continue
            lat_r, old_r = start[g:g + 1].clone(), start_old[g:g + 1].clone()
            sc_r = torch.full((nb, HW, ld), SENT, device=dev)
            ops.cfg_dpmpp2m_step(eps.view(nb, G, HW, Cc)[:, g].contiguous(), lat_r, old_r, sc_r, sig[g].contiguous(), coef[g, :8].contiguous(),
                                 torch.tensor([steps[g]], dtype=torch.int32, device=dev), nb, Cc, ld, gs[g], igs[g], mode)
            assert same_bits(lat[g], lat_r[0]) and not torch.equal(lat[g], start[g]), (steps, g)
            assert same_bits(old[g], old_r[0]) and bool(torch.isfinite(old[g]).all()) and bool(torch.isfinite(lat[g]).all()), (steps, g)
            assert same_bits(sc[:, g], sc_r), (steps, g)
            assert (sc[:, g, :, Cc:] == SENT).all() and not (sc[:, g, :, :Cc] == SENT).any()
            if steps[g] == n_steps[g] - 1:
                assert torch.equal(lat[g], old[g]), "the last step lands on x0"


# ----------------------------------------------------------------------------------------------------------------------------
# the loops
# ----------------------------------------------------------------------------------------------------------------------------
KW = dict(height=128, width=128, max_steps=8, output_type="latent")


@pytest.fixture(scope="module", params=[0, 1], ids=["t2i", "edit"])
def pipe(request, dev):
    """(adapter with the Euler scheduler it was built with, mode, three requests of 2, 3 and 5 steps)."""
    from seedx_amd.detokenizer import SDXLAdapter, SDXLAdapterWithLatentImage
    from tests.test_adapter_e2e_gpu import _build
    mode = request.param
    ad, _ = _build(dev, torch.float16, 4 if mode == 0 else 8, SDXLAdapter if mode == 0 else SDXLAdapterWithLatentImage)
    g = torch.Generator().manual_seed(21 + mode)
    feats = torch.randn(3, 1, 16, 256, generator=g).to(dev)
    noise = torch.randn(3, 1, 4, 16, 16, generator=g)
    il = torch.randn(3, 1, 4, 16, 16, generator=g)
    reqs = [dict(image_embeds=feats[i], latents=noise[i], num_inference_steps=n, guidance_scale=gs, input_image_size=112)
            for i, (n, gs) in enumerate(((2, 7.5), (3, 4.0), (5, 5.25)))]
    if mode == 1:
        for i, r in enumerate(reqs):
            r.update(image_latents=il[i], image_guidance_scale=(1.5, 2.25, 0.75)[i])
    return ad, mode, reqs


def _generate(ad, mode, req, steps):
    kw = dict(image_embeds=req["image_embeds"], latents=req["latents"], num_inference_steps=steps, guidance_scale=req["guidance_scale"], height=128, width=128,
              input_image_size=112, output_type="latent")
    if mode == 1:
        kw.update(image_latents=req["image_latents"], image_guidance_scale=req["image_guidance_scale"])
    return ad.generate(**kw).clone()


def test_loop_graph_replay_equals_eager_and_feeds_the_kernel_its_tables(dev, pipe, monkeypatch):
    """Karras 2M through _DenoiseLoop.run at 1, 2 and 4 steps: the graph replay equals the eager run bit for bit. In the eager run every call of
    ops.cfg_dpmpp2m_step is watched: its step counter walks 0 .. n - 1, its tables are the scheduler's, and its outputs are within the derived bound of
    the fp64 rule from ITS inputs (so x0_prev is carried, and the right row is read)."""
    from seedx_amd import ops, solvers
    from seedx_amd.detokenizer import DPMSolverMultistepScheduler
    ad, mode, reqs = pipe
    euler = ad.scheduler
    real = ops.cfg_dpmpp2m_step
    seen = []

    def watched(eps, lat, old, scaled, sig, coef, step, nb, C_lat, ld, gs, igs, m):
        before = (eps.clone(), lat.clone(), old.clone(), int(step.item()))
        real(eps, lat, old, scaled, sig, coef, step, nb, C_lat, ld, gs, igs, m)
        seen.append(before + (lat.clone(), old.clone(), sig.clone(), coef.clone(), gs, igs, nb))

    try:
        ad.scheduler = DPMSolverMultistepScheduler(use_karras_sigmas=True)
        for steps in (1, 2, 4):
            ad._loop.use_graph = True
            graph = _generate(ad, mode, reqs[1], steps)
            assert ad._loop._graph is not None and "x0_prev" in ad._loop._state and ad._loop._graph_key[-1] == 2
            ad._loop.use_graph = False
            del seen[:]
            monkeypatch.setattr(ops, "cfg_dpmpp2m_step", watched)
            eager = _generate(ad, mode, reqs[1], steps)
            monkeypatch.setattr(ops, "cfg_dpmpp2m_step", real)
            assert torch.isfinite(graph).all() and torch.equal(graph, eager), f"{steps} steps: graph replay and eager run differ"
            assert [s[3] for s in seen] == list(range(steps))
            sch = ad.scheduler
            co64 = solvers.dpmpp2m_coefficients(sch.sigmas.numpy(), np.float64)
            for eps, lat, old, i, lat_n, old_n, sig, coef, gs, igs, nb in seen:
                assert torch.equal(sig.cpu(), sch.sigmas) and torch.equal(coef.cpu(), sch.coefficients) and nb == 2 + mode
                xn, bx, x0, b0, _, _ = ref_step(mode, lat.reshape(-1).cpu().numpy(), eps.reshape(nb, -1).cpu().numpy(), old.reshape(-1).cpu().numpy(),
                                                float(sch.sigmas[i]), float(sch.sigmas[i + 1]), co64[i], gs, igs)
                held(("loop", f"mode {mode}"), lat_n.reshape(-1), xn, bx, f"{steps} steps, step {i} (latents)")
                held(("loop", f"mode {mode} x0_prev"), old_n.reshape(-1), x0, b0, f"{steps} steps, step {i} (x0_prev)")
                if i > 0:
                    assert torch.equal(old, seen[i - 1][5]), "x0_prev is the previous step's x0"
    finally:
        ad.scheduler = euler
        ad._loop.use_graph = True


def test_inflight_equals_lockstep_and_euler_keeps_its_bits(dev, pipe):
    """The Euler result of the pipe first. Then, with Karras 2M: generate_inflight on 2 slots with requests of 2, 3 and 5 steps gives each request the
    latents of its own lock-step run (row 0 of _DenoiseLoop.run at G = 2 filled with copies of the request: the same UNet launches), bit for bit, with one
    capture of the slot step. Then the Euler scheduler again, through the same loops: the bits it gave before, after a re-capture; and the two solvers
    differ."""
    from seedx_amd.detokenizer import DPMSolverMultistepScheduler, _DenoiseLoop
    from tests.test_detok_inflight_gpu import _reference
    ad, mode, reqs = pipe
    euler = ad.scheduler
    assert euler.order == 1
    try:
        before = _generate(ad, mode, reqs[2], 5)
        before_q = [o.clone() for o in ad.generate_inflight(reqs, slots=2, **KW)]
        assert ad._loop._graph_key[-1] == 1 and "x0_prev" not in ad._loop._state and "x0_prev" not in ad._slot_loop._state
        ad.scheduler = DPMSolverMultistepScheduler(use_karras_sigmas=True)
        outs = [o.clone() for o in ad.generate_inflight(reqs, slots=2, **KW)]
        assert ad.last_inflight_stats["graph_captures"] == 1 and ad._slot_loop._dims["order"] == 2
        again = ad.generate_inflight(list(reversed(reqs)), slots=2, **KW)                  # other steps per slot: tables are data
        assert ad.last_inflight_stats["graph_captures"] == 1
        ref_loop = _DenoiseLoop(ad.unet, use_graph=True)
        for i, o in enumerate(outs):
            r = _reference(ad, ref_loop, reqs[i], 2, mode=mode)
            assert torch.isfinite(o).all() and torch.equal(o, r), f"request {i}: max |diff| {(o - r).abs().max().item():.3e}"
            assert torch.equal(again[2 - i], o)
            assert not torch.equal(o, before_q[i]), "the two solvers must differ"
        dpm = _generate(ad, mode, reqs[2], 5)
        assert ad._loop._graph_key[-1] == 2 and not torch.equal(dpm, before)
        ad.scheduler = euler
        assert torch.equal(_generate(ad, mode, reqs[2], 5), before), "Euler after a 2M run: the graph key must separate the solvers"
        after_q = ad.generate_inflight(reqs, slots=2, **KW)
        for a, b in zip(after_q, before_q):
            assert torch.equal(a, b)
        assert "x0_prev" not in ad._loop._state and "x0_prev" not in ad._slot_loop._state
    finally:
        ad.scheduler = euler
        ad._slot_loop = None


def test_print_worst_ratio_per_kernel(dev):
    """Not a check of its own: the worst |diff| / bound per kernel and output (run the file as a whole)."""
    for key, w in sorted(WORST.items(), key=lambda kv: str(kv[0])):
        print(f"worst |diff| / bound  {str(key):60s} {w:.3f}")
