"""scipy's RK45 (scipy 1.15), traced evaluation by evaluation: the reference for the device RK45 stepper (use_ode_*, csrc/use_ode.hip),
and the drift families that drive it into each of its branches.  Used by tests/test_hip_ode_stepper.py (GPU) and by
tests/test_ode_sampler_host.py (CPU: every family must still reach its branch in scipy).

A drift is ``f(t, x, items) -> complex64 [nb, n]``: t float32 [nb] (one time per item: on the device a finished group carries its own),
x complex64 [nb, n], items the item indices (per-item parameters).  Each element-wise step is one float32 numpy operation on the real
or the imaginary parts, so it is correctly rounded and its bits do not depend on how numpy vectorises an array of a given length;
per-item transcendentals are taken in float64 and rounded once.  The same (t, x) therefore give the same bits whether a group is
evaluated alone (scipy) or inside the whole batch (the device stepper).  scipy sees the drift as the reference's ode_func hands it
over: ``fun(t, y) = f(float32(t), complex64(y)).astype(complex128)`` (sampling/__init__.py of the reference)."""
import math

import numpy as np
from scipy.integrate import RK45

F32 = np.float32
STATUS = {"running": 1, "finished": 0, "failed": -1}
TOO_SMALL_STEP, MAX_NFE = -1, -2


def c64(re, im):
    out = np.empty(np.broadcast(re, im).shape, np.complex64)
    out.real, out.imag = re, im
    return out


def per_item(fn, t):
    """fn(float t) -> float, per item, rounded once to float32."""
    return np.array([fn(float(ti)) for ti in np.atleast_1d(t)], dtype=F32)[:, None]


def complex_normal(shape, seed, scale=1.0, mean=0.0):
    rng = np.random.default_rng(seed)
    return (mean + scale * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))).astype(np.complex64)


# ---- drift families ----------------------------------------------------------------------------------------------------------
class Linear:
    """f = -lam_b (x - m_b): smooth; the rate lam_b = 0.5 + 1.5 (b mod 7) differs per item, so that groups need different NFE."""
    name = "linear"

    @staticmethod
    def x0(B, n, seed=0):
        return complex_normal((B, n), seed)

    @staticmethod
    def f(t, x, items):
        lam = (F32(0.5) + F32(1.5) * (items % 7).astype(F32))[:, None]
        m_re = (F32(0.25) * (items % 3).astype(F32))[:, None]
        return c64(-(lam * (x.real - m_re)), -(lam * (x.imag - F32(-0.2))))


class Jump:
    """f = -(1 + 50 (tanh((t - 0.5) / 0.01) + 1)) x: the rate drops from 101 to 1 within ~0.02 around t = 0.5.  Rejected steps
    (the first attempt from select_initial_step's h is too long).  The accepted retries here have step factors <= 1 anyway, so the
    cap factor = min(1, factor) after a rejection does not act on this family (BlowUp's retries reach it: Trace.capped)."""
    name = "jump"

    @staticmethod
    def x0(B, n, seed=0):
        return complex_normal((B, n), seed)

    @staticmethod
    def f(t, x, items):
        r = per_item(lambda s: 1.0 + 50.0 * (math.tanh((s - 0.5) / 0.01) + 1.0), t)
        return c64(-(r * x.real), -(r * x.imag))


class BlowUp:
    """f = -x^2 from real x0 ~ 4: integrated from t = 1 downwards, x = 1 / (t - 1 + 1 / x0) blows up at t ~ 0.75.  The step size shrinks
    below scipy's min_step (status -1, TOO_SMALL_STEP) while |y| ~ 1e14 is still finite in float32 (x^2 < 3.4e38).  On the way,
    retries after a rejection are accepted with error norms small enough that factor = min(1, factor) caps them (Trace.capped)."""
    name = "blowup"

    @staticmethod
    def x0(B, n, seed=0):
        return (4.0 + 1e-3 * np.random.default_rng(seed).random((B, n))).astype(np.complex64)     # real: the pole is on the t axis

    @staticmethod
    def f(t, x, items):
        a, b = x.real, x.imag
        return c64(-(a * a - b * b), -((F32(2) * a) * b))


class Zero:
    """x0 = 0 and f = 0: select_initial_step's d0 < 1e-5 (h0 = 1e-6) and d1, d2 <= 1e-15 (h1 = max(1e-6, 1e-3 h0)); every step's
    error norm is exactly 0 (factor = MAX_FACTOR)."""
    name = "zero"

    @staticmethod
    def x0(B, n, seed=0):
        return np.zeros((B, n), np.complex64)

    @staticmethod
    def f(t, x, items):
        return c64(x.real * F32(0), x.imag * F32(0))


class ZeroStart(Linear):
    """x0 = 0 with the nonzero drift of Linear: d0 < 1e-5 (h0 = 1e-6) but d1, d2 > 0."""
    name = "zerostart"

    @staticmethod
    def x0(B, n, seed=0):
        return np.zeros((B, n), np.complex64)


FAMILIES = {c.name: c for c in (Linear, Jump, BlowUp, Zero, ZeroStart)}


# OUVE (sdes.py) with the engine's defaults theta = 1.5, sigma_min = 0.05, sigma_max = 0.5, as torch forms it in float32
THETA, SIGMA_MIN, SIGMA_MAX = 1.5, 0.05, 0.5


def ouve_cg(t):
    """g(t)^2 / 2 per item in float32: sigma_min * (sigma_max / sigma_min) ** t * sqrt(2 log(sigma_max / sigma_min)), each constant a
    Python float met by a float32 tensor (numpy's float32 pow here, the device's powf there: they may differ by one ulp)."""
    base, sq2ls = F32(SIGMA_MAX / SIGMA_MIN), F32(math.sqrt(2 * math.log(SIGMA_MAX / SIGMA_MIN)))
    t = np.atleast_1d(t).astype(F32)
    g = (F32(SIGMA_MIN) * np.power(base, t)) * sq2ls
    return ((g * g) * F32(0.5))[:, None]


def analytic_score(t, x, y, items):
    """A smooth stand-in for the network: -(x - 0.8 y) / (0.5 + t^2), the factor per item in float32."""
    s = per_item(lambda u: 1.0 / (0.5 + u * u), t)
    return c64(-((x.real - F32(0.8) * y.real) * s), -((x.imag - F32(0.8) * y.imag) * s))


def pf_drift(t, x, y, score):
    """theta (y - x) - g(t)^2 / 2 * score in float32 (RSDE.sde with probability_flow, sdes.py): the drift kind 1 forms on the device."""
    th, cg = F32(THETA), ouve_cg(t)
    return c64(th * (y.real - x.real) - cg * score.real, th * (y.imag - x.imag) - cg * score.imag)


# ---- scipy's RK45, traced ----------------------------------------------------------------------------------------------------
class Trace:
    """One scipy RK45 integration: ``records`` (t, h_abs, nfev, status, accepted steps) after the constructor and after every step();
    ``err_norms`` every error norm (_estimate_error_norm); ``call_t`` the time (float64) of every fun call; ``y`` the final solution (complex128;
    with max_nfe: the state after the last step whose evaluations fit, as the device keeps it); ``capped`` the steps accepted after a
    rejection whose step factor min(MAX_FACTOR, SAFETY en^(-1/5)) exceeded 1, i.e. where scipy's factor = min(1, factor) acted."""

    def __init__(self):
        self.records, self.err_norms, self.call_t, self.y, self.capped = [], [], [], None, 0

    @property
    def calls(self):
        return len(self.call_t)

    @property
    def status(self):
        return self.records[-1][3]

    @property
    def nfev(self):
        return self.records[-1][2]

    @property
    def steps(self):
        return self.records[-1][4]

    @property
    def rejected(self):
        return (self.nfev - self.records[0][2]) // 6 - self.steps


def scipy_rk45(f, x0, items, rtol, atol, t_eps=0.03, first_step=None, max_step=np.inf, max_nfe=None, on_call=None):
    """scipy's RK45 over one group: x0 complex64 [nb, n] of the items `items`, integrated from t = 1 down to t_eps as one flattened
    complex128 vector.  on_call(k, t32, x_c64 [nb, n]) sees every evaluation.  max_nfe: stop as the device stepper does, before an
    attempt whose 6 evaluations would exceed it; then the last record has status MAX_NFE and nfev = what the device has spent."""
    tr = Trace()
    nb, n = x0.shape
    items = np.asarray(items)

    class TracedRK45(RK45):
        def _estimate_error_norm(self, K, h, scale):
            en = super()._estimate_error_norm(K, h, scale)
            tr.err_norms.append(float(en))
            return en

    def fun(t, y):
        t32 = F32(t)
        x = y.astype(np.complex64).reshape(nb, n)
        if on_call is not None:
            on_call(tr.calls, t32, x)
        tr.call_t.append(float(t))
        return f(np.full(nb, t32), x, items).reshape(-1).astype(np.complex128)

    s = TracedRK45(fun, 1.0, x0.reshape(-1).astype(np.complex128), t_eps, rtol=rtol, atol=atol, max_step=max_step,
                   first_step=first_step)
    steps = 0
    tr.records.append((float(s.t), float(s.h_abs), s.nfev, STATUS[s.status], steps))
    while s.status == "running":
        before = (float(s.t), float(s.h_abs), s.nfev, s.y.copy())
        n_en = len(tr.err_norms)
        s.step()
        ens = tr.err_norms[n_en:]                             # one per attempt of this step; the last one accepted if en < 1
        if len(ens) > 1 and ens[-1] < 1 and (ens[-1] == 0 or 0.9 * ens[-1] ** -0.2 > 1):
            tr.capped += 1
        if max_nfe is not None and s.nfev > max_nfe:           # the device stops inside this step, at its last accepted state
            t, h_abs, nfev, y = before
            tr.records.append((t, h_abs, nfev + 6 * ((max_nfe - nfev) // 6), MAX_NFE, steps))
            tr.y = y
            return tr
        if s.status != "failed":
            steps += 1
        tr.records.append((float(s.t), float(s.h_abs), s.nfev, STATUS[s.status], steps))
    tr.y = s.y.copy()
    return tr


def groups_of(B, group):
    G = B if group == 0 or group > B else group
    return [np.arange(b0, min(B, b0 + G)) for b0 in range(0, B, G)]
