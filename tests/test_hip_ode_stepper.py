"""GPU tests of the device RK45 stepper (use_ode_*, csrc/use_ode.hip) against scipy's own RK45 class, evaluation by evaluation.

The stepper is driven through hip_engine.OdeStepper with a drift computed on the host (kind 0): every request (x, t) is copied back,
the drift of tests/ode_ref.py is evaluated on it and supplied.  scipy's RK45 runs per group on the same drift (ode_ref.scipy_rk45).
The drift is bit-reproducible on the host, so the two sides differ only where the fp64 stage sums and norms are formed in another
order (and where the compiler contracts a product and a sum into one FMA): per request, t is bit-equal, and x is bit-equal apart from
rare rounding flips, each one float32 ulp where it first appears (see check_requests); nfev, accepted steps, rejections and status
are equal; t and h_abs after every step agree to rel_t_h(rtol, atol).  The error estimate sum(K_i E_i) h cancels: it is ~rtol |y| while each term is ~|y|, so the fp64 rounding of the
summation order reaches the error norm amplified by ~1 / rtol, and the step factor (its -1/5 power) and the accepted times with it.  Then the fused sampler (use_sample_ode) against the same stepper driven by the same network."""
import numpy as np
import pytest
import torch

import ode_ref as R
from universal_speech_enhancement_amd.testing import noise as tnoise
from universal_speech_enhancement_amd.testing import weights as tw

pytestmark = pytest.mark.gpu

# Request x, element by element.  A stage input formed in fp64 in another order can round to the other complex64 neighbour: a "flip",
# one ulp where it first appears (ONSET_ULP).  At most FLIP_FRAC of the compared values may flip (and at least one flip is tolerated
# in a case that compares fewer than 1 / FLIP_FRAC values).  A flipped element then has its own slightly different drift, so it can
# stay apart in the later requests, by at most LATER_ULP.  Measured over every case: see the [measured] lines ("flips", "later").
ONSET_ULP = 1
FLIP_FRAC = 1e-6
LATER_ULP = 16         # measured at most 7 (n = 262144), with 37 flips among 8.1e7 values (4.6e-7); one flip in the small cases


def rel_t_h(rtol, atol):
    """t and h_abs, relative: 1e-13 / the tolerance (measured at most 2.1e-14 / tolerance over every case here)."""
    return 1e-13 / min(rtol, atol or rtol)


@pytest.fixture(scope="module")
def eng():
    from universal_speech_enhancement_amd.hip_engine import HipScoreEngine
    e = HipScoreEngine(precision="fp32")          # the stepper uses only the handle's OUVE constants (ode_ref's THETA, SIGMA_*)
    yield e
    e.close()


def _ordered(a):
    i = np.ascontiguousarray(a).view(np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def ulps(a, b):
    """Per complex element: the larger float32 ulp distance of its two components."""
    d = np.abs(_ordered(a) - _ordered(b)).reshape(a.shape + (2,))
    return d.max(axis=-1)


def run_device(eng, f, x0, kind="drift", y=None, **cfg):
    """Drive OdeStepper to its end: f(t [B] float32, x [B, n] complex64) -> complex64 supplied per request.  Returns the requests
    (t on the host, x kept on the device), the per-group state() after every attempt, and result()."""
    from universal_speech_enhancement_amd.hip_engine import OdeStepper
    B, n = x0.shape
    y_sde = torch.from_numpy(np.zeros((B, n), np.complex64) if y is None else y).cuda()
    st = OdeStepper(eng, y_sde, torch.from_numpy(x0).cuda(), record_times=False, **cfg)
    n_init = 1 if cfg.get("first_step") else 2
    reqs, states, k = [], [], 0
    try:
        while (req := st.request()) is not None:
            x, t = req
            th = t.cpu().numpy().copy()
            reqs.append((th, x.clone()))
            st.supply(torch.from_numpy(f(th, x.cpu().numpy())).cuda(), kind)
            k += 1
            if k >= n_init and (k - n_init) % 6 == 0:       # an attempt ended (the first record: after select_initial_step)
                states.append(list(zip(*st.state())))
        out, nfev, status = st.result()
        return reqs, states, out.cpu().numpy(), nfev, status
    finally:
        st.close()


def check_against_scipy(tag, fam, x0, group, rtol, atol, t_eps=0.03, first_step=None, max_step=None, max_nfe=None, eng=None,
                        dev_states=None):
    """The device stepper and scipy's RK45 per group on fam's drift: every request, every step, the result.  Returns the scipy traces
    (and appends the device's per-attempt states to dev_states)."""
    B, n = x0.shape
    cfg = dict(rtol=rtol, atol=atol, t_eps=t_eps, group=group, first_step=first_step, max_step=max_step, max_nfe=max_nfe or 0,
               denoise=False, use_graph=False)
    reqs, states, out, nfev, status = run_device(eng, lambda t, x: fam.f(t, x, np.arange(B)), x0, **cfg)
    groups = R.groups_of(B, group)
    assert len(nfev) == len(groups)
    n_cmp = n_el = n_diff = n_flip = later = 0
    worst = 0.0
    traces = []
    for g, items in enumerate(groups):
        b0, b1 = int(items[0]), int(items[-1]) + 1
        apart = np.zeros((b1 - b0, n), bool)       # elements that have flipped in an earlier request

        def on_call(k, t32, x):
            nonlocal n_cmp, n_el, n_diff, n_flip, later
            if k >= nfev[g]:                       # max_nfe: scipy goes on inside the step the device never starts
                return
            dt, dx = reqs[k]
            assert np.all(dt[b0:b1] == t32), (tag, g, k, dt[b0:b1], t32)
            u = ulps(dx[b0:b1].cpu().numpy(), x)
            new = (u > 0) & ~apart
            if new.any():
                assert u[new].max() <= ONSET_ULP, (tag, g, k, "flip", int(u[new].max()))
            if apart.any():
                later = max(later, int(u[apart].max()))
                assert later <= LATER_ULP, (tag, g, k, "later", later)
            apart[new] = True
            n_cmp += 1; n_el += u.size; n_diff += int((u > 0).sum()); n_flip += int(new.sum())

        tr = R.scipy_rk45(fam.f, x0[b0:b1], items, rtol, atol, t_eps=t_eps, first_step=first_step,
                          max_step=np.inf if max_step is None else max_step, max_nfe=max_nfe, on_call=on_call)
        traces.append(tr)
        assert (nfev[g], status[g]) == (tr.nfev, tr.status), (tag, g, nfev[g], status[g], tr.nfev, tr.status)
        ref = {r[2]: r for r in tr.records}        # by nfev (with max_nfe the last record replaces the one it repeats)
        seen = set()
        for s in states:
            t, h_abs, nf, stt, steps = s[g]
            if nf in seen:                         # a frozen group: the same state again
                continue
            seen.add(nf)
            below = [r for r in tr.records if r[2] <= nf]
            assert below, (tag, g, nf)
            r = ref.get(nf, below[-1])             # not a scipy record: an attempt inside a step that rejected it - nothing moves
            for dev, want, what in ((t, r[0], "t"), (h_abs, r[1], "h_abs")):
                e = abs(dev - want) / abs(want)
                worst = max(worst, e)
                assert e <= rel_t_h(rtol, atol), (tag, g, nf, what, dev, want)
            assert steps == r[4], (tag, g, nf, steps, r[4])
            assert stt == (r[3] if nf in ref else 1), (tag, g, nf, stt, r[3])
        assert seen >= {r[2] for r in tr.records}, (tag, g, sorted(seen), [r[2] for r in tr.records])
        u = ulps(out[b0:b1], tr.y.astype(np.complex64).reshape(b1 - b0, n))
        assert u.max() <= 1, (tag, g, "result", int(u.max()))
    n_init = 1 if first_step else 2
    dev = [(nfev[g], states[-1][g][4], (nfev[g] - n_init) // 6 - states[-1][g][4]) for g in range(len(groups))]
    ref = [(tr.nfev, tr.steps, tr.rejected) for tr in traces]
    show = (lambda v: v) if len(groups) <= 8 else (lambda v: [sum(c) for c in zip(*v)])
    print(f"[measured] {tag}: {n_cmp} requests, {n_el} values, {n_flip} flips (1 ulp), {n_diff} values apart, later max {later} ulp, "
          f"worst rel t/h_abs {worst:.1e}, (nfev, steps, rejected) device {show(dev)} scipy {show(ref)}, status {status}")
    assert n_flip <= max(FLIP_FRAC * n_el, 1), (tag, n_flip, n_el)
    assert dev == ref
    if dev_states is not None:
        dev_states.extend(states)
    return traces


# ---- 1. drift families x tolerances --------------------------------------------------------------------------------------------
TOLS = [(1e-3, 1e-5), (1e-5, 1e-5), (1e-7, 1e-7), (1e-4, 0.0)]


# Left out: x0 = 0 with atol = 0 (scipy's own scale is 0, y0 / scale is nan), and rtol 1e-7 where the drift is not 0: there the error
# norm of a step sits at the float32 rounding level of the stages, so one stage input one ulp apart moves the next step size and
# the runs separate (measured: float32 stage times one ulp apart after 160-480 evaluations).  So the pair (1e-7, 1e-7) is effectively
# untested: it runs only on the zero drift, whose error norm is always 0.
FAMILY_CASES = [(f, r, a) for f in ["linear", "jump", "blowup", "zero", "zerostart"] for r, a in TOLS
                if not (a == 0 and f in ("zero", "zerostart")) and not (r == 1e-7 and f != "zero")]


@pytest.mark.parametrize("family,rtol,atol", FAMILY_CASES)
def test_stepper_matches_scipy_per_family(eng, family, rtol, atol):
    """B = 5 in groups of 2, 2, 1; 16 elements per item.  Each family reaches its branch in scipy (tests/test_ode_sampler_host.py)."""
    fam = R.FAMILIES[family]
    traces = check_against_scipy(f"{family} rtol={rtol} atol={atol}", fam, fam.x0(5, 16), 2, rtol, atol, eng=eng)
    if family == "jump" and rtol < 1e-3:
        assert sum(tr.rejected for tr in traces) > 0
    if family == "blowup":                                # also the family where factor = min(1, factor) after a rejection acts
        assert all(tr.status == R.TOO_SMALL_STEP and tr.capped > 0 for tr in traces)


# ---- 2. first_step, max_step, t_eps, max_nfe --------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["linear", "jump"])
@pytest.mark.parametrize("first_step,max_step,t_eps", [(0.01, None, 0.03), (None, 0.05, 0.03), (0.01, 0.05, 0.1), (None, None, 0.1)])
def test_stepper_first_step_max_step_t_eps(eng, family, first_step, max_step, t_eps):
    """first_step / max_step / t_eps reach scipy as the Python floats 0.01 / 0.05 / 0.03, 0.1: what float_as_decimal claims to make of
    the float32 fields.  first_step: one evaluation before the first step (nfev = 1 + 6 k).  Exactly, on the device alone: h_abs
    before the first step is first_step; a step clamped to max_step and accepted at once ends at t - max_step; the last t is t_eps.
    (float32 values promoted to double would be 1.5e-8 to 2.2e-8 off.)"""
    fam = R.FAMILIES[family]
    # jump with first_step at (1e-5, 1e-5): measured, the runs separate after ~360 evaluations (float32 stage times one ulp apart, the
    # error norm of a step there at the float32 rounding level); (1e-5, 1e-5) without these options runs in FAMILY_CASES
    rtol = 1e-5 if family == "linear" else 1e-4
    states = []
    traces = check_against_scipy(f"{family} first_step={first_step} max_step={max_step} t_eps={t_eps}", fam, fam.x0(5, 16), 2, rtol,
                                 1e-5, t_eps=t_eps, first_step=first_step, max_step=max_step, eng=eng, dev_states=states)
    clamped = 0
    for g, tr in enumerate(traces):
        rec = list({s[g][2]: s[g] for s in states}.values())          # per nfev: (t, h_abs, nfev, status, steps)
        if first_step:
            assert rec[0][1] == first_step, (g, rec[0])
        assert tr.status == 0 and rec[-1][0] == t_eps, (g, rec[-1])
        starts = list({r[4]: r for r in reversed(rec)}.values())[::-1]    # per accepted-step count: the state the next step starts from
        for a, b in zip(starts, starts[1:]):                                  # b[2] == a[2] + 6: the step was accepted at its first attempt
            if max_step and a[1] > max_step and b[2] == a[2] + 6 and b[0] != t_eps:
                assert b[0] == a[0] - max_step, (g, a, b)
                clamped += 1
    if max_step:
        assert clamped > 0


def test_stepper_max_nfe_stops_at_scipys_state(eng):
    """max_nfe: status -2, nfev <= max_nfe, and the state of scipy after the last step whose evaluations fit.  Once between two steps,
    once inside a step that rejected its first attempt (the device has spent the rejected attempt; y, t and h_abs do not move)."""
    fam = R.Jump
    x0 = fam.x0(1, 16)
    tr = R.scipy_rk45(fam.f, x0, np.arange(1), 1e-5, 1e-5)
    r = tr.records
    k = next(i for i in range(1, len(r)) if r[i][2] - r[i - 1][2] > 6 and r[i][4] > r[i - 1][4])   # a step with a rejection
    for max_nfe in (r[k - 1][2] + 3, r[k - 1][2] + 6 + 3):
        (t,) = check_against_scipy(f"jump max_nfe={max_nfe}", fam, x0, 1, 1e-5, 1e-5, max_nfe=max_nfe, eng=eng)
        assert t.status == R.MAX_NFE and t.nfev <= max_nfe and t.steps == r[k - 1][4]
    (t,) = check_against_scipy("linear max_nfe=17", R.Linear, R.Linear.x0(1, 16), 1, 1e-5, 1e-5, max_nfe=17, eng=eng)   # needs 20
    assert t.status == R.MAX_NFE and t.nfev == 14


# ---- 3. sizes and groups -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 2048, 2049, 262144, 327680])
def test_stepper_sizes(eng, n):
    """nblk = ceil(n / 2048) workgroups per item, at most 128: n = 1 (one workgroup, 255 idle threads), 2048 / 2049 (the step to two),
    262144 (exactly 128), 327680 (the benchmark's 512 x 640: clamped to 128, a strided loop)."""
    B, group = (8, 3) if n >= 262144 else (5, 2)
    check_against_scipy(f"linear n={n} B={B} group={group}", R.Linear, R.Linear.x0(B, n), group, 1e-3, 1e-5, eng=eng)


@pytest.mark.parametrize("B,group,n", [(5, 2, 64), (5, 0, 64), (5, 1, 64), (300, 1, 4)])
def test_stepper_groups(eng, B, group, n):
    """Groups that do not divide B (a short last group: group_norm's (b1 - b0)), one group, one item per group, and 300 groups (more
    than the controller's 256 threads: a thread runs two groups)."""
    traces = check_against_scipy(f"linear B={B} group={group}", R.Linear, R.Linear.x0(B, n), group, 1e-3, 1e-5, eng=eng)
    if len(traces) > 1:
        assert len({tr.nfev for tr in traces}) > 1, "the groups should need different NFE"


def test_frozen_groups_do_not_move(eng):
    """B = 5 in groups of 2, 2, 1 finish at different NFE; a finished group is frozen while the others step.  Each group's result and
    state are bit-identical to a run of its items alone (nblk depends on n only, so every partial sum is formed the same way)."""
    B, n = 5, 300
    x0 = R.Linear.x0(B, n)
    cfg = dict(rtol=1e-5, atol=1e-5, group=2, denoise=False, use_graph=False)
    _, states, out, nfev, status = run_device(eng, lambda t, x: R.Linear.f(t, x, np.arange(B)), x0, **cfg)
    assert len(set(nfev)) == 3, nfev
    for g, items in enumerate(R.groups_of(B, 2)):
        _, s1, o1, nf1, st1 = run_device(eng, lambda t, x, items=items: R.Linear.f(t, x, items), x0[items], **cfg)
        assert np.array_equal(out[items].view(np.int32), o1.view(np.int32)), g
        assert (nfev[g], status[g]) == (nf1[0], st1[0])
        assert states[-1][g] == s1[-1][0], (g, states[-1][g], s1[-1][0])
    print(f"[measured] frozen groups: nfev {nfev} equal to the groups' own runs, results and states bit-identical")


# ---- 4. kind 1: the drift formed from a score on the device --------------------------------------------------------------------
def test_stepper_kind_score_matches_scipy(eng):
    """kind 1: the device forms theta (y - x) - g(t)^2 / 2 score itself (g with the device's powf), scipy gets the same drift formed in
    numpy (ode_ref.pf_drift, numpy's float32 pow).  powf and numpy's pow may differ by one ulp at some stage times; that moves the drift
    by ~6e-8 relative, so requests are not compared bit for bit.  Most steps then move by ~1e-8.  But on this smooth drift the long
    step from t ~ 0.91 has an error norm of ~1e-5 at rtol 1e-3: the float32 rounding level of the stages, where one ulp of g moves the
    norm by tens of percent and the step factor (its -1/5 power, ~9 there) by a few percent.  So the accepted times may move by a few
    percent of one step (measured 7.1e-3 on a step of 0.84): bound 2e-2.  Equal NFE and status: no accept / reject decision may flip."""
    B, n = 3, 256
    x0, y = R.Linear.x0(B, n, seed=1), R.complex_normal((B, n), 2, scale=0.5)
    items = np.arange(B)
    cfg = dict(rtol=1e-3, atol=1e-3, t_eps=0.03, group=1, denoise=False, use_graph=False)
    _, states, out, nfev, status = run_device(eng, lambda t, x: R.analytic_score(t, x, y, items), x0, kind="score", y=y, **cfg)
    worst, res = 0.0, 0.0
    for g in range(B):
        sl = slice(g, g + 1)
        tr = R.scipy_rk45(lambda t, x, it: R.pf_drift(t, x, y[it], R.analytic_score(t, x, y[it], it)), x0[sl], items[sl], 1e-3, 1e-3)
        assert (nfev[g], status[g]) == (tr.nfev, tr.status), (g, nfev[g], status[g], tr.nfev, tr.status)
        dev_t = sorted({s[g][0] for s in states}, reverse=True)
        ref_t = [r[0] for r in tr.records]
        print(f"[measured] kind 1 group {g}: accepted t device {dev_t} scipy {ref_t}")
        assert len(dev_t) == len(ref_t)
        worst = max(worst, float(np.abs(np.array(dev_t) - ref_t).max()))
        res = max(res, float(np.abs(out[g] - tr.y.astype(np.complex64)).max() / np.abs(tr.y).max()))
    print(f"[measured] kind 1: nfev {nfev}, status {status}, accepted times max |dt| {worst:.1e}, result rel-max {res:.1e}")
    assert worst < 2e-2
    assert res < 1e-5


# ---- 5. the fused sampler at the benchmark shape ---------------------------------------------------------------------------------
FB, FF, FT = 8, 512, 640


@pytest.fixture(scope="module")
def sd_np():
    return tw.make_state_dict(1234, **tw.LARGE)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_fused_sampler_equals_the_stepper_on_the_same_network(sd_np, precision):
    """use_sample_ode (graph and eager) against OdeStepper driven by the same engine's score (kind 1) from the same prior: the same
    kernels on the same inputs, so the outputs are bit-identical, and per group nfev / status, and the handle's ode_steps /
    ode_rejected / ode_nfev_max equal what the stepper's state() implies.  B = 8, 512 x 640, groups of 3, 3, 2 and the whole batch."""
    from universal_speech_enhancement_amd.hip_engine import HipScoreEngine, OdeStepper
    e = HipScoreEngine(precision=precision)
    try:
        e.load_state_dict(sd_np)
        Y = torch.from_numpy(tnoise.complex_normal(5, "ode_y", (FB, 1, FF, FT))).cuda() * 0.5
        z = torch.from_numpy(tnoise.complex_normal(5, "ode_z", (FB, 1, FF, FT))).cuda()
        e.plan(FB, FT)
        for group in (3, 0):
            cfg = dict(rtol=1e-3, atol=1e-3, t_eps=0.03, N=30, group=group, denoise=False)
            runs = {}
            for use_graph in (True, False):
                e.set_ode(use_graph=use_graph, **cfg)
                x, nfev, status = e.sample_ode(Y, noise=z)
                runs[use_graph] = (x, nfev, status, e.stat("ode_steps"), e.stat("ode_rejected"), e.stat("ode_nfev_max"))
            x0 = e.sde_prior(Y, noise=z)
            st = OdeStepper(e, Y, x0, record_times=False, **cfg)
            try:
                xs, nfs, sts = st.run(lambda x, t: e.score(x, Y, t), kind="score")
                _, _, nf, _, steps = st.state()
            finally:
                st.close()
            rej = [(nf[g] - 2) // 6 - steps[g] for g in range(len(nf))]
            print(f"[measured] fused {precision} group={group}: nfev {nfs}, steps {steps}, rejected {rej}, status {sts}")
            for use_graph, (x, nfev, status, s_steps, s_rej, s_nfmax) in runs.items():
                assert (nfev, status) == (nfs, sts), (use_graph, nfev, status, nfs, sts)
                assert torch.equal(x.view(torch.float32), xs.view(torch.float32)), \
                    f"graph={use_graph}: {float((x - xs).abs().max())} apart"
                assert (s_steps, s_rej, s_nfmax) == (sum(steps), sum(rej), max(nf)), (use_graph, s_steps, s_rej, s_nfmax)
            assert sts == [0] * len(sts)
    finally:
        e.close()
