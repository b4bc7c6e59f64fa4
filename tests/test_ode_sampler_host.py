"""CPU-only checks of the probability-flow ODE sampler: the C ABI is exported and declared, the Python entry point refuses what it
does not implement before touching a device, and the golden fixtures tests/golden/ode_*.npz (made by scripts/gen_golden_ode.py from
the reference's own get_ode_sampler) are reproduced by a scipy RK45 integration of the same problem here."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from universal_speech_enhancement_amd import _lib
from universal_speech_enhancement_amd.sgmse import sampling
from universal_speech_enhancement_amd.sgmse.sdes import OUVESDE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ODE_SYMBOLS = ["use_set_ode", "use_sample_ode", "use_ode_create", "use_ode_start", "use_ode_request", "use_ode_supply", "use_ode_result",
               "use_ode_state", "use_ode_num_groups", "use_ode_destroy"]
FIXTURES = ["ode_batch", "ode_items", "ode_tight", "ode_nodenoise"]


def test_ode_entry_points_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "use_hip.h")).read()
    declared = set(re.findall(r"\b(use_[a-z_0-9]+)\s*\(", header))
    L = C.CDLL(_lib.LIB_PATH)
    for name in ODE_SYMBOLS:
        assert name in declared, f"{name} is not declared in use_hip.h"
        assert hasattr(L, name), f"{name} is not exported by libuse_hip.so"
        assert name in _lib.SYMBOLS
    assert "use_ode_config" in header


@pytest.mark.parametrize("kw,word", [({"method": "RK23"}, "RK23"), ({"method": "DOP853"}, "DOP853"), ({"vectorized": True}, "vectorized"),
                                     ({"atol": np.array([1e-5, 1e-6])}, "atol")])
def test_unimplemented_solver_options_raise_before_any_device_work(kw, word):
    y = torch.zeros(1, 1, 4, 4, dtype=torch.complex64)          # a CPU tensor: any device work would fail differently

    def score_fn(*a, **k):
        raise AssertionError("the score must not be evaluated")

    with pytest.raises(NotImplementedError, match=word):
        sampling.get_ode_sampler(OUVESDE(), score_fn, y, **kw)


def test_ode_stepper_validates_its_configuration_without_a_device():
    L = _lib.lib()
    cfg = _lib.UseConfig()
    cfg.nf, cfg.n_levels, cfg.num_res_blocks, cfg.n_freq, cfg.precision = 128, 7, 2, 512, 1
    for i, m in enumerate((1, 1, 2, 2, 2, 2, 2)):
        cfg.ch_mult[i] = m
    cfg.theta, cfg.sigma_min, cfg.sigma_max = 1.5, 0.05, 0.5
    h = C.c_void_p()
    assert L.use_create(C.byref(cfg), 0, C.byref(h)) == 0
    try:
        o = C.c_void_p()
        for bad in (dict(rtol=0.0), dict(rtol=-1e-5), dict(group=-1), dict(t_eps=1.5), dict(first_step=2.0)):
            oc = _lib.UseOdeConfig(**{**dict(rtol=1e-5, atol=1e-5, t_eps=0.03, N=30, group=1, denoise=1, first_step=0.0, max_step=0.0,
                                             max_nfe=0, use_graph=1), **bad})
            assert L.use_ode_create(h, 3, 128, C.byref(oc), C.byref(o)) == -1, bad          # USE_E_INVALID
            assert not o.value
        # use_set_ode on a handle without weights / plan: the state error, not a crash
        oc = _lib.UseOdeConfig(1e-5, 1e-5, 0.03, 30, 1, 1, 0.0, 0.0, 0, 1)
        assert L.use_set_ode(h, C.byref(oc)) == -3                                             # USE_E_STATE
    finally:
        L.use_destroy(h)


def _reintegrate(g):
    """The reference's ODE sampler algorithm (sampling/__init__.py:93-159) with scipy's RK45 on the CPU, per group."""
    from scipy import integrate
    Y, A, prior = (torch.from_numpy(g[k]) for k in ("Y", "A", "prior"))
    c0, amp, eps, N = float(g["c0"]), float(g["amp"]), float(g["eps"]), int(g["N"])
    sde = OUVESDE()
    sde.N = N
    mb = int(g["minibatch"])
    groups = [slice(0, Y.shape[0])] if mb < 0 else [slice(i, i + mb) for i in range(0, Y.shape[0], mb)]
    xs, nfev, times = [], [], []
    for sl in groups:
        Yc = Y[sl]

        def score(x, t):
            return -(x - 0.8 * Yc) / (c0 + t[:, None, None, None] ** 2) + amp * A * torch.tanh(x.abs())

        def ode_func(t, x):
            x = torch.from_numpy(x.reshape(Yc.shape)).type(torch.complex64)
            vec_t = torch.ones(Yc.shape[0]) * t
            drift, diffusion = sde.sde(x, vec_t, Yc)
            return (drift - diffusion[:, None, None, None] ** 2 * score(x, vec_t) * 0.5).numpy().reshape((-1,))

        x0 = Yc + prior[sl] * sde._std(torch.ones(Yc.shape[0]))[:, None, None, None]
        sol = integrate.solve_ivp(ode_func, (1, eps), x0.numpy().reshape((-1,)), rtol=float(g["rtol"]), atol=float(g["atol"]), method="RK45")
        x = torch.tensor(sol.y[:, -1]).reshape(Yc.shape).type(torch.complex64)
        if int(g["denoise"]):                                   # ReverseDiffusionPredictor at eps, x_mean
            vec_eps = torch.ones(Yc.shape[0]) * eps
            dt = 1 / N
            drift, diffusion = sde.sde(x, vec_eps, Yc)
            f, G = drift * dt, diffusion * torch.sqrt(torch.tensor(dt))
            x = x - (f - G[:, None, None, None] ** 2 * score(x, vec_eps))
        xs.append(x.numpy()); nfev.append(sol.nfev); times.append(sol.t)
    return np.concatenate(xs), nfev, times


@pytest.mark.parametrize("name", FIXTURES)
def test_golden_ode_fixture_is_reproduced_by_scipy(golden_dir, name):
    g = dict(np.load(os.path.join(golden_dir, f"{name}.npz")))
    x, nfev, times = _reintegrate(g)
    assert nfev == g["nfev"].tolist()
    for k, t in enumerate(times):
        np.testing.assert_allclose(t, g["times"][k, : int(g["n_times"][k])], rtol=0, atol=1e-12)
    np.testing.assert_allclose(x, g["x"], rtol=1e-5, atol=1e-6)
    if name == "ode_items":
        assert int(g["rejected"].sum()) >= 1


def test_ode_ref_drift_families_reach_their_branches_in_scipy():
    """tests/test_hip_ode_stepper.py compares the device stepper with scipy on the drift families of tests/ode_ref.py; each family is
    there for a branch of scipy's RK45, and this checks, without a device, that scipy still takes it."""
    import ode_ref as R                                                         # scipy.integrate, imported by this test only
    x = {name: fam.x0(5, 16) for name, fam in R.FAMILIES.items()}
    run = {name: [R.scipy_rk45(R.FAMILIES[name].f, x[name][it], it, 1e-5, 1e-5) for it in R.groups_of(5, 2)] for name in R.FAMILIES}
    for name, trs in run.items():
        for tr in trs:
            assert tr.calls == tr.nfev and tr.rejected == (tr.nfev - 2) // 6 - tr.steps
            assert tr.status == (R.TOO_SMALL_STEP if name == "blowup" else 0), name
    assert sum(tr.rejected for tr in run["jump"]) > 0                           # rejected steps
    assert all(tr.rejected > 0 and tr.records[-1][0] > 0.7 for tr in run["blowup"])   # status -1 before the pole at t ~ 0.75
    assert all(tr.capped > 0 for tr in run["blowup"])                           # retries where factor = min(1, factor) acts
    for name in ("zero", "zerostart"):                                          # d0 < 1e-5: h0 = 1e-6, the probe at t0 - h0
        assert all(tr.call_t[1] == 1.0 - 1e-6 for tr in run[name]), name
    for tr in run["zero"]:                                                      # d1, d2 <= 1e-15: h1 = 1e-6; every error norm 0
        assert tr.records[0][1] == 1e-6 and tr.err_norms and set(tr.err_norms) == {0.0}
        # factor = MAX_FACTOR (of the attempt's h = t_new - t, which is h_abs up to the rounding of t_new)
        assert all(abs(b[1] / a[1] - 10) < 1e-6 or b[3] == 0 for a, b in zip(tr.records, tr.records[1:]))
    for tr in run["zerostart"]:                                                 # d1 > 0: h0 = 1e-6, h_abs = 100 h0
        assert tr.records[0][1] == 100 * 1e-6 and min(tr.err_norms) > 0
    assert len({tr.nfev for tr in run["linear"]}) == 3                          # the groups need different NFE
