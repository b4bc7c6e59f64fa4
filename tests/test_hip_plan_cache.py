"""GPU tests of the plan's life cycle (use_engine.cpp: struct Plan, the handle's current plan and its parked ones): eviction at
capacity, capacity 0, plans built under older options, what a parked plan brings back, new weights, and the FLOP count after a hit.
Public API and ctypes only; the smallest plans (B = 1 or 2, T' = 64 ... 256), since the shape is irrelevant to what can go wrong here.
Every test sets "plan_cache" before its first plan: each use_set_option makes the plans built before it stale."""
import ctypes as C

import pytest
import torch

from universal_speech_enhancement_amd import _lib
from universal_speech_enhancement_amd._lib import UseHipError
from universal_speech_enhancement_amd.testing import noise as tnoise
from universal_speech_enhancement_amd.testing import weights as tw

pytestmark = pytest.mark.gpu

F = 512
USE_E_STATE = -3


@pytest.fixture(scope="module")
def sd_np():
    return tw.make_state_dict(1234, **tw.LARGE)


@pytest.fixture
def eng(sd_np):
    """A fresh handle per test (its counters start at 0 and nothing is parked); the option goes back to its default afterwards."""
    from universal_speech_enhancement_amd.hip_engine import HipScoreEngine, set_option
    e = HipScoreEngine(precision="bf16")
    e.load_state_dict(sd_np)
    try:
        yield e
    finally:
        e.close()
        set_option("plan_cache", 4)


def _score_inputs(B, Tp):
    x = torch.from_numpy(tnoise.complex_normal(31, f"pc_x{Tp}", (B, 1, F, Tp))).cuda() * 0.5
    y = torch.from_numpy(tnoise.complex_normal(31, f"pc_y{Tp}", (B, 1, F, Tp))).cuda() * 0.5
    return x, y, torch.full((B,), 0.4, device="cuda")


def _score(eng, Tp, B=1):
    """(score bits at (B, T'), plans_parked right after the plan) - eng.score plans first."""
    eng.plan(B, Tp)
    parked = eng.stat("plans_parked")
    out = eng.score(*_score_inputs(B, Tp)).clone()
    torch.cuda.synchronize()
    return out, parked


def _counters(eng):
    return eng.stat("plans_built"), eng.stat("plan_cache_hits")


def test_the_least_recently_used_plan_is_evicted_at_capacity(eng):
    from universal_speech_enhancement_amd.hip_engine import set_option
    set_option("plan_cache", 2)
    first, parked = {}, []
    for Tp in (64, 128, 192, 256):
        first[Tp], n = _score(eng, Tp)
        parked.append(n)
    assert parked == [0, 1, 2, 2]                             # 256 pushed 64 out
    assert _counters(eng) == (4, 0)
    out, n = _score(eng, 192)                                 # still parked: a hit
    assert _counters(eng) == (4, 1) and n == 2 and torch.equal(out, first[192])
    out, n = _score(eng, 64)                                  # evicted: built again, and the same bits as the first time
    assert _counters(eng) == (5, 1) and n == 2
    assert torch.isfinite(torch.view_as_real(out)).all() and torch.equal(out, first[64])


def test_capacity_zero_parks_nothing_and_every_shape_change_builds(eng):
    from universal_speech_enhancement_amd.hip_engine import set_option
    set_option("plan_cache", 0)
    first = {}
    for i, Tp in enumerate((64, 128, 64, 128, 64)):
        out, n = _score(eng, Tp)
        assert n == 0 and _counters(eng) == (i + 1, 0), (i, Tp)
        assert torch.equal(out, first.setdefault(Tp, out)), (i, Tp)


def test_a_plan_built_under_older_options_is_not_a_hit(eng):
    from universal_speech_enhancement_amd.hip_engine import set_option
    set_option("plan_cache", 4)
    eng.plan(1, 64)
    eng.plan(1, 128)
    assert eng.stat("plans_parked") == 1 and eng.stat("plan_stale") == 0
    set_option("stagger_level", 2)                            # its default: changes nothing but the option generation
    assert eng.stat("plan_stale") == 1
    eng.plan(1, 64)
    assert _counters(eng) == (3, 0)                           # the parked (1, 64) is stale: built anew
    # the stale current plan (1, 128) was dropped, not parked; the stale parked one stays until it is evicted
    assert eng.stat("plans_parked") == 1 and eng.stat("plan_stale") == 0
    out, _ = _score(eng, 64)
    assert torch.isfinite(torch.view_as_real(out)).all()


def test_a_hit_brings_back_sampler_tables_graphs_workspace_and_taps(eng):
    from universal_speech_enhancement_amd.hip_engine import set_option, _stream_ptr
    set_option("plan_cache", 4)
    L = _lib.lib()
    B = 2
    y64 = torch.from_numpy(tnoise.complex_normal(32, "pc_s64", (B, 1, F, 64))).cuda() * 0.5
    y128 = torch.from_numpy(tnoise.complex_normal(32, "pc_s128", (B, 1, F, 128))).cuda() * 0.5

    def sample(y, out):
        return L.use_sample(eng.h, y.data_ptr(), None, 11, out.data_ptr(), _stream_ptr(y.device))

    assert L.use_plan(eng.h, B, 64) == 0
    sc = _lib.UseSamplerConfig(2, _lib.PREDICTORS["reverse_diffusion"], _lib.CORRECTORS["langevin"], 1, 0.5, 3e-2, 1)
    assert L.use_set_sampler(eng.h, C.byref(sc)) == 0
    a = torch.empty_like(y64)
    assert sample(y64, a) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(torch.view_as_real(a)).all()
    ws, captures = eng.workspace_bytes(), eng.stat("graph_captures")
    assert captures == 1

    assert L.use_plan(eng.h, B, 128) == 0                     # a new plan: no sampler, no ODE configuration
    assert eng.workspace_bytes() > ws
    out = torch.full_like(y128, 7.0)
    assert sample(y128, out) == USE_E_STATE and b"use_set_sampler has not been called" in L.use_last_error()
    nf, st = (C.c_int * B)(), (C.c_int * B)()
    rc = L.use_sample_ode(eng.h, y128.data_ptr(), None, None, None, 11, out.data_ptr(), nf, st, _stream_ptr(out.device))
    assert rc == USE_E_STATE and b"use_set_ode has not been called" in L.use_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused sampler must not launch anything"

    assert L.use_plan(eng.h, B, 64) == 0                      # the parked plan: sampler configuration, tables and graph come with it
    assert _counters(eng) == (2, 1)
    again = torch.empty_like(y64)
    assert sample(y64, again) == 0
    torch.cuda.synchronize()
    assert torch.equal(again, a)
    assert eng.stat("graph_captures") == captures
    assert eng.workspace_bytes() == ws
    assert tuple(eng.debug_tensor("h_in").shape[:3]) == (B, F, 64)


def test_new_weights_drop_the_parked_plans_and_the_sampler_tables(eng, sd_np):
    from universal_speech_enhancement_amd.hip_engine import set_option
    set_option("plan_cache", 4)
    y = torch.from_numpy(tnoise.complex_normal(33, "pc_w", (2, 1, F, 128))).cuda() * 0.5
    eng.plan(2, 64)
    eng.plan(2, 128)
    eng.set_sampler(2, "reverse_diffusion", "langevin", 1, 0.5, 3e-2, use_graph=True)
    before = eng.sample(y, seed=11).clone()
    assert eng.stat("plans_parked") == 1
    eng.load_state_dict(sd_np)
    assert eng.stat("plans_parked") == 0
    with pytest.raises(UseHipError, match="use_set_sampler has not been called"):
        eng.sample(y, seed=11)
    eng.set_sampler(2, "reverse_diffusion", "langevin", 1, 0.5, 3e-2, use_graph=True)
    after = eng.sample(y, seed=11)
    torch.cuda.synchronize()
    assert torch.equal(after, before)                         # the same weights again: the same bits


def test_flops_per_score_right_after_a_hit_is_that_plans_own(eng):
    """The FLOP count belongs to the plan: a parked plan that returns reports its own, not the count of the plan that was current
    before it (which it did, until the next evaluation, while the count was a field of the handle outside the plan)."""
    from universal_speech_enhancement_amd.hip_engine import set_option
    set_option("plan_cache", 4)
    eng.plan(1, 64)
    f64 = eng.flops_per_score()
    _score(eng, 64)
    assert eng.flops_per_score() == f64 > 0
    eng.plan(1, 128)
    f128 = eng.flops_per_score()
    assert f128 > f64
    eng.plan(1, 64)
    assert _counters(eng) == (2, 1)
    assert eng.flops_per_score() == f64
