"""The fused predictor-corrector loop (run_sampler in csrc/use_engine.cpp, behind use_sample* and use_sample_items), update by update
against float64, through the sampler step trace (use_set_option("sampler_trace", 1); use_sampler_trace_entry in include/use_hip.h).

What only the fused loop does, and what this file therefore holds against an independent reference: every update in place (x and x_out
the same buffer), the per-item addressing (items = B, noise of seeds[b] at the in-item index, one Langevin step per item), the Langevin
reduction at the plan's lang_blocks = min(256, ceil(F T' / 256)), the draw counter restarted at every captured segment, time embeddings
and t from the tables of use_set_sampler (row i, stride 0), x_mean at the last step alone (a copy under USE_PRED_NONE), the ALD step
from timesteps[i] on the host, and all of it above the sub-batch pipeline.

References and bounds are those of tests/test_hip_sde_kernels.py (tests/philox_ref.py: prior, predictor, corrector, ald_eps, ratio,
unchanged; langevin_eps generalised to the loop's blocks and to the per-item step, pinned below against its old values); the
derivations are in that module's docstring.  Every bound is per element and per real component, counts worst-case float32 roundings and
was fixed before the first GPU run; the step snapshot must lie within e_eps 2^-24 of the float64 eps, the traced host scalars within
E_CD, E_CS, E_CN, E_STD, E_ALD units of 2^-24.  tests/sampler_steps_ref.py walks a trace and is tested here under `-m "not gpu"` on a
float32 emulation of the loop with nine mutations (its docstring), on the GPU cases' shapes.

Every network evaluation of a traced run is tied to the network tests (tests/test_hip_network_layers.py) bit for bit: the score snapshot
equals use_score on the X snapshot the evaluation read, the conditioning and t = timesteps[i] in every item - in per-item runs the exact
negation of use_forward_items.  Table row i of use_set_sampler comes from the same temb_mlp / temb_dense launches over the same float32
t, strides 0 and 1 address equal values, and the sub-batch split belongs to the plan.

Shapes: the LARGE synthetic weights (seed 1234), F = 512, T' = 64 (0.4 s), gains an order of magnitude apart - the smallest at which
the network runs; 32768 elements per item, lang_blocks = 128; one case at T' = 256 (lang_blocks = 256, two serial terms per thread).

Measured on the MI355X (2026-10-20, this file's first commit, on a8753d6), worst |err| / bound per kind, fp32 unless said otherwise:
    case               prior   Langevin step  corrector  predictor  host scalars
    B1-N3              0.965   0.077          0.933      0.602      0.187
    B3-shared          0.965   0.086          0.948      0.643      0.187        (bf16: 0.965, 0.010, 0.946, 0.711, 0.187)
    B3-items           0.965   0.077          0.947      0.774      0.187        (bf16: 0.965, 0.061, 0.953, 0.658, 0.187)
    B5-shared          0.965   0.026          0.947      0.565      0.176
    B5-items           0.965   0.057          0.948      0.646      0.176
    B3-items-em-ald2   0.965   -              0.973      0.565      0.176
    B1-none-langevin   0.965   0.013          0.928      -          0.176
    B1-N1-rd-none      0.965   -              -          0.493      0.176
    B1-N33-graph       0.965   0.104          0.973      0.897      0.326
    B1-N1-T256         0.922   0.007          0.788      0.642      0.176
and on the device's own draws (B1-N3, B3-shared, B3-items, B3-items-em-ald2) prior 0.992, step 0.094, corrector 0.967, predictor 0.819.
The updates' worst elements are output roundings at the bottom of a binade, as in test_hip_sde_kernels.py.  Every evaluation was
bit-equal to use_score / -use_forward_items, every mode comparison bit-equal, in every case: no finding, and the __restrict__ qualifiers
of the update kernels stay (each thread reads element i of x before it writes element i of x_out).  No constant changed after a
measurement.  The GPU part takes about 10 s, the CPU part about 6 s."""
import numpy as np
import pytest
import torch

import philox_ref as pr
import sampler_steps_ref as ss
from universal_speech_enhancement_amd.testing import noise as tnoise
from universal_speech_enhancement_amd.testing import weights as tw

GAINS = (1.0, 5.0, 0.2, 2.5, 0.5)
SEEDS = [0x0123456789ABCDEF, 7, 2 ** 64 - 1, 0xDEADBEEF00000000, 31337]
SNR, T_EPS, F = 0.5, 3e-2, 512


def _case(B, per_item, N, predictor="reverse_diffusion", corrector="langevin", steps=1, use_graph=False, T=64):
    return dict(B=B, per_item=per_item, N=N, predictor=predictor, corrector=corrector, corrector_steps=steps, use_graph=use_graph, T=T,
                snr=SNR, t_eps=T_EPS)


CASES = {
    "B1-N3": _case(1, False, 3),                                            # both halves of the float32 linspace, x_mean at the last step only
    "B3-shared": _case(3, False, 3),                                        # batch-coupled step ...
    "B3-items": _case(3, True, 3),                                          # ... against per-item steps, distinct gains
    "B5-shared": _case(5, False, 2),                                        # 3 + 2 sub-batches under a batch-coupled step
    "B5-items": _case(5, True, 2),
    "B3-items-em-ald2": _case(3, True, 2, "euler_maruyama", "ald", 2),      # two corrector draws per step, host ALD step size
    "B1-none-langevin": _case(1, False, 2, "none", "langevin"),             # USE_PRED_NONE: Xmean is a copy
    "B1-N1-rd-none": _case(1, False, 1, "reverse_diffusion", "none"),       # linspace with one point
    "B1-N33-graph": _case(1, False, 33, use_graph=True),                    # two captured segments (32 + 1 steps)
    "B1-N1-T256": _case(1, False, 1, T=256),                                # lang_blocks = 256, two serial terms per thread
}
RUNS = [(k, "fp32") for k in CASES] + [("B3-shared", "bf16"), ("B3-items", "bf16")]


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the generalised langevin_eps, the walker and its mutation controls
# ---------------------------------------------------------------------------------------------------------------------------
def _cn(seed, shape):
    return tnoise.complex_normal(seed, "sampler_steps", shape)


def test_langevin_eps_keeps_its_values_at_128_blocks():
    """blocks = SDE_BLOCKS = 128 and the shared form are what test_hip_sde_kernels.py has always used: same eps, same error count."""
    for shape in ((3, 1, 33, 7), (2, 1, 512, 64), (1, 1, 512, 256), (1024, 1, 8, 1)):
        B = shape[0]
        g, z = _cn(1, shape) * np.logspace(-1, 1, B).astype(np.float32).reshape(B, 1, 1, 1), _cn(2, shape)
        g2, z2 = g.reshape(B, -1).astype(np.complex128), z.reshape(B, -1).astype(np.complex128)
        old_eps = 2.0 * (float(np.float32(SNR)) * np.linalg.norm(z2, axis=1).mean() / np.linalg.norm(g2, axis=1).mean()) ** 2
        old_e = 2.0 * (-(-g2.shape[1] // (128 * 256)) + 17) + 1.0
        assert pr.langevin_eps(g, z, SNR) == (old_eps, old_e) == pr.langevin_eps(g, z, SNR, blocks=128)
        eps_b, e_b = pr.langevin_eps(g, z, SNR, per_item=True)
        assert eps_b.shape == (B,) and e_b == old_e
        for b in range(min(B, 3)):                                          # the per-item step is the shared step of the item alone
            assert eps_b[b] == pr.langevin_eps(g[b:b + 1], z[b:b + 1], SNR)[0]
    assert pr.SDE_BLOCKS == 128
    g, z = _cn(3, (1, 1, 512, 256)), _cn(4, (1, 1, 512, 256))
    assert pr.langevin_eps(g, z, SNR, blocks=256)[1] == 2.0 * (2 + 17) + 1.0     # 131072 elements over 256 x 256 threads: k = 2
    assert pr.langevin_eps(g, z, SNR, blocks=128)[1] == 2.0 * (4 + 17) + 1.0
    assert ss.lang_blocks(512 * 64) == 128 and ss.lang_blocks(512 * 256) == 256 and ss.lang_blocks(1000) == 4


def test_expected_layout_counts():
    for name, cfg in CASES.items():
        lay = ss.expected_layout(cfg)
        ds = [d for _, _, _, d in lay if d >= 0]
        upd = [d for kind, _, _, d in lay if kind in ("prior", "corrector", "predictor")]
        assert upd == list(range(ss.n_draws(cfg))), name                   # every draw consumed once, in order, by an update
        assert set(ds) == set(upd)
        assert sum(kind == "score" for kind, *_ in lay) == cfg["N"] * (ss.n_corr(cfg) + (cfg["predictor"] != "none"))
    assert [e[0] for e in ss.expected_layout(CASES["B1-none-langevin"])][-1] == "copy_mean"


_emu = {}


def _emu_inputs(name):
    cfg = CASES[name]
    if name not in _emu:
        shape = (cfg["B"], 1, F, cfg["T"])
        gains = np.asarray(GAINS[:cfg["B"]], np.float32).reshape(-1, 1, 1, 1)
        _emu[name] = (_cn(11, shape) * gains, tnoise.sampler_noise(55, ss.n_draws(cfg), shape), _cn(12, (1,) + shape[1:]))
    return (cfg,) + _emu[name]


@pytest.mark.parametrize("name", list(CASES))
def test_the_unmutated_emulation_stays_within_the_bounds(name):
    cfg, y, draws, a = _emu_inputs(name)
    w = ss.walk(ss.emulate(cfg, y, draws, a), y, draws, cfg)
    print(f"[emulation] {name}: " + ", ".join(f"{k} {v:.3f}" for k, v in w.items() if v))
    assert max(w.values()) < 1.0, w
    if not cfg["use_graph"]:                                                # the segments change nothing when the counter is right
        seg = ss.emulate(cfg, y, draws, a, segmented=True)
        assert max(ss.walk(seg, y, draws, cfg).values()) < 1.0


def _applies(mut, cfg):
    lang, pred, nc = cfg["corrector"] == "langevin", cfg["predictor"] != "none", ss.n_corr(cfg)
    return {"swap_draws": pred and nc > 0, "segment_counter": cfg["use_graph"] and cfg["N"] * (nc + 1) > ss.SEGMENT_EVALS,
            "coeffs_next_t": pred and cfg["N"] > 1, "eps_batch_mean": lang and cfg["per_item"] and cfg["B"] > 1,
            "eps_prev_score": lang and cfg["N"] > 1, "mean_with_noise": pred, "mean_early": pred, "sqrt_eps": nc > 0,
            "aliased_neighbour": True}[mut]


@pytest.mark.parametrize("mut", ss.MUTATIONS)
def test_mutations_exceed_the_bounds(mut):
    """Each mutation on every case it can show in (exempt where it changes nothing: no corrector or no predictor to swap with, one
    segment, N = 1, a batch of one or the shared form for the batch-mean step, no earlier evaluation)."""
    hit = 0
    for name in CASES:
        cfg, y, draws, a = _emu_inputs(name)
        if not _applies(mut, cfg):
            continue
        w = ss.walk(ss.emulate(cfg, y, draws, a, mut=mut), y, draws, cfg)
        print(f"[mutation] {mut} on {name}: " + ", ".join(f"{k} {v:.3g}" for k, v in w.items() if v > 1))
        assert max(w.values()) > 1.0, (mut, name, w)
        assert w["layout"] == 0.0, "the mutations leave the record alone: the values must give them away"
        hit += 1
    assert hit >= {"segment_counter": 1, "eps_batch_mean": 2}.get(mut, 3), (mut, hit)


def test_the_walker_refuses_a_wrong_record():
    cfg, y, draws, a = _emu_inputs("B3-items")
    good = ss.emulate(cfg, y, draws, a)
    for change in (lambda e: e.pop(3), lambda e: e[5].update(d=e[5]["d"] + 1), lambda e: e[-1].update(x_mean=None),
                   lambda e: e[1].update(t=np.float32(np.nextafter(e[1]["t"], np.float32(0)))), lambda e: e[2].update(items=1),
                   lambda e: e[4].update(x_out=None)):
        bad = [dict(e) for e in good]
        change(bad)
        assert ss.walk(bad, y, draws, cfg)["layout"] == np.inf
    bad = [dict(e) for e in good]
    bad[5]["x_in"] = bad[5]["x_in"].copy()
    bad[5]["x_in"].view(np.uint32)[0, 0, 0, 0] ^= 1                          # one bit of what the next evaluation read
    assert ss.walk(bad, y, draws, cfg)["chain"] == np.inf
    bad = [dict(e) for e in good]
    bad[4]["x_out"] = np.full_like(bad[4]["x_out"], np.nan)                 # an update that wrote nothing
    assert ss.walk(bad, y, draws, cfg)["corrector"] == np.inf


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sd_np():
    return tw.make_state_dict(1234, **tw.LARGE)


@pytest.fixture()
def traced():
    from universal_speech_enhancement_amd import hip_engine
    hip_engine.set_option("sampler_trace", 1)
    yield hip_engine
    hip_engine.set_option("sampler_trace", 0)


_models, _specs, _runs = {}, {}, {}


def _model(sd_np, precision):
    if precision not in _models:
        from universal_speech_enhancement_amd.sgmse.model_wrapper import ScoreModel
        m = ScoreModel(backbone="ncsnpplarge", sde="ouve", t_eps=T_EPS, condition="noisy", n_fft=1022, hop_length=160, num_frames=512,
                       window="hann", sde_input="noisy", predictor="reverse_diffusion", corrector="langevin", precision=precision)
        m.score_net.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
        _models[precision] = m
    return _models[precision]


def _engine(sd_np, precision):
    m = _model(sd_np, precision)
    return m.score_net.engine(512, torch.device("cuda", torch.cuda.current_device()),
                              sde_constants=(m.sde.theta, m.sde.sigma_min, m.sde.sigma_max))


def _spec(sd_np, B, T):
    """Y [B,1,512,T']: 0.4 s utterances (1.67 s for T' = 256) with GAINS between the items"""
    if (B, T) not in _specs:
        wav = torch.from_numpy(tnoise.synth_noisy_speech(B, 9600 if T == 64 else 40000, seed=321)) * torch.tensor(GAINS[:B]).view(B, 1)
        Y = _model(sd_np, "fp32")._spectrogram(wav.cuda()).contiguous()
        assert tuple(Y.shape) == (B, 1, F, T)
        _specs[(B, T)] = Y
    return _specs[(B, T)]


def _draws(cfg):
    return tnoise.sampler_noise(55, ss.n_draws(cfg), (cfg["B"], 1, F, cfg["T"]))


def _configure(eng, cfg, use_graph=None):
    eng.plan(cfg["B"], cfg["T"])
    eng.set_sampler(cfg["N"], cfg["predictor"], cfg["corrector"], cfg["corrector_steps"], SNR, T_EPS,
                    use_graph=cfg["use_graph"] if use_graph is None else use_graph)


def _sample(eng, cfg, Y, use_graph=None, **kw):
    """one sampler call -> (output on the host, its trace)"""
    _configure(eng, cfg, use_graph)
    if cfg["per_item"] and "item_seeds" not in kw:
        kw["per_item"] = True
    out = eng.sample(Y, **kw)
    torch.cuda.synchronize()
    return out.cpu(), eng.sampler_trace()


def _run(sd_np, name, prec):
    """the traced run of a case on injected noise, once per module: (cfg, Y, draws on the host, noise on the device, out, entries)"""
    if (name, prec) not in _runs:
        cfg = CASES[name]
        eng, Y, draws = _engine(sd_np, prec), _spec(sd_np, cfg["B"], cfg["T"]), _draws(cfg)
        noise = torch.from_numpy(draws).cuda()
        out, entries = _sample(eng, cfg, Y, noise=noise)
        _runs[(name, prec)] = (cfg, Y, draws, noise, out, entries)
    return _runs[(name, prec)]


SNAPS = ("x_in", "score", "step", "x_out", "x_mean")
SCALARS = ("kind", "i", "k", "d", "items", "n_per_item", "blocks_per_b", "per_item", "t", "std1", "c_drift", "c_score", "c_noise", "step_host")


def _eq(a, b):
    """both absent, or the same shape and the same bits"""
    if a is None or b is None:
        return a is None and b is None
    a, b = a.contiguous().numpy(), b.contiguous().numpy()
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _same_trace(a, b, what):
    assert len(a) == len(b) and len(a) > 0, (what, len(a), len(b))
    for ea, eb in zip(a, b):
        for f in SCALARS:
            assert ea[f] == eb[f], (what, ea["index"], f, ea[f], eb[f])
        for f in SNAPS:
            assert _eq(ea[f], eb[f]), (what, ea["index"], ea["kind"], f)


@pytest.mark.gpu
@pytest.mark.parametrize("name,prec", RUNS)
def test_every_update_against_float64(sd_np, traced, name, prec):
    """Assertions 1 and 2: the layout of the reference loop, and every update, step size and host scalar within its bound."""
    cfg, Y, draws, noise, out, entries = _run(sd_np, name, prec)
    eng = _engine(sd_np, prec)
    n = Y.numel()
    _configure(eng, cfg)
    assert eng.num_noise_draws() == ss.n_draws(cfg) == 1 + max(e["d"] for e in entries)
    ts = eng.timesteps()
    assert np.array_equal(ts.view(np.uint32), torch.linspace(1, T_EPS, cfg["N"]).numpy().view(np.uint32))
    for e in entries:
        if e["kind"] != "prior":
            assert np.float32(e["t"]).view(np.uint32) == ts[e["i"]].view(np.uint32), (e["index"], e["t"])
        if e["kind"] in ("langevin_norms", "langevin_step"):
            assert e["blocks_per_b"] == ss.lang_blocks(F * cfg["T"]) == (128 if cfg["T"] == 64 else 256)
        if e["d"] >= 0 and not cfg["use_graph"]:                            # eager: the launch read the caller's draw d itself
            assert e["noise"] == noise.data_ptr() + e["d"] * n * 8, (e["index"], e["d"])
    w = ss.walk(entries, Y.cpu(), draws, cfg)
    print(f"[measured] {name} {prec}: worst |err| / bound " + ", ".join(f"{k} {w[k]:.3f}" for k in ss.KINDS if any(e["kind"] == k for e in entries) or (k == "scalars")))
    assert w["layout"] == 0.0 and w["chain"] == 0.0, w
    assert max(w.values()) <= 1.0, w
    last = entries[-1]
    assert last["kind"] == ("copy_mean" if cfg["predictor"] == "none" else "predictor") and _eq(last["x_mean"], out), "the output is Xmean"
    assert torch.isfinite(torch.view_as_real(out)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name,prec", RUNS)
def test_every_evaluation_is_the_network_of_use_score(sd_np, traced, name, prec):
    """Assertion 3.  Bit for bit: the loop's evaluation i (time-embedding table row i, t from ts_dev + i, strides 0) against use_score on
    the same plan with t = timesteps[i] in every item (row b of a fresh temb launch, stride 1); per item against -use_forward_items."""
    cfg, Y, draws, noise, out, entries = _run(sd_np, name, prec)
    eng = _engine(sd_np, prec)
    eng.plan(cfg["B"], cfg["T"])
    k = 0
    for e in entries:
        if e["kind"] != "score":
            continue
        x, t = e["x_in"].cuda(), torch.full((cfg["B"],), float(e["t"]), dtype=torch.float32, device="cuda")
        if cfg["per_item"]:
            got = -eng.forward(x, Y, t, per_image=True)
        else:
            got = eng.score(x, Y, t)
        assert _eq(got.cpu(), e["score"]), f"{name} {prec}: evaluation {k} (step {e['i']}, corrector {e['k']}) differs from the network called alone"
        k += 1
    assert k == cfg["N"] * (ss.n_corr(cfg) + (cfg["predictor"] != "none"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_graph_replay_equals_eager_snapshot_by_snapshot(sd_np, traced, name):
    """Assertion 4, first half: graph against eager (the two segments of N = 33 included), and a second replay against the first."""
    cfg, Y, draws, noise, out, entries = _run(sd_np, name, "fp32")
    eng = _engine(sd_np, "fp32")
    other = not cfg["use_graph"]
    o1, t1 = _sample(eng, cfg, Y, use_graph=other, noise=noise)
    assert _eq(o1, out)
    _same_trace(t1, entries, f"{name}: graph against eager")
    c0 = eng.stat("graph_captures")
    o2, t2 = _sample(eng, cfg, Y, use_graph=True, noise=noise)
    if other:
        assert eng.stat("graph_captures") == c0, "the second call replays"
    assert _eq(o2, out)
    _same_trace(t2, entries, f"{name}: second replay")
    if name == "B1-N33-graph":
        assert eng.stat("graph_captures") - c0 == 2, "33 steps of two evaluations: segments of 32 + 1 steps"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["B1-N3", "B3-shared", "B3-items", "B3-items-em-ald2"])
def test_device_noise_equals_its_replay_snapshot_by_snapshot(sd_np, traced, name):
    cfg = CASES[name]
    eng, Y = _engine(sd_np, "fp32"), _spec(sd_np, cfg["B"], cfg["T"])
    seeds = SEEDS[:cfg["B"]]
    for use_graph in (False, True):
        kw = dict(item_seeds=seeds) if cfg["per_item"] else dict(seed=SEEDS[4])
        o1, t1 = _sample(eng, cfg, Y, use_graph=use_graph, **kw)
        assert all(e["noise"] is None for e in t1)
        fill = (lambda d: eng.fill_noise_items(seeds, d, Y.shape)) if cfg["per_item"] else (lambda d: eng.fill_noise(SEEDS[4], d, Y.shape))
        z = torch.stack([fill(d) for d in range(ss.n_draws(cfg))])
        o2, t2 = _sample(eng, cfg, Y, use_graph=use_graph, noise=z)
        assert _eq(o1, o2)
        _same_trace(t1, t2, f"{name} graph={use_graph}: device noise against its replay")
    w = ss.walk(t1, Y.cpu(), z.cpu().numpy(), cfg)                          # and the device's own draws through the same bounds
    print(f"[measured] {name} on device noise: worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in w.items() if v))
    assert max(w.values()) <= 1.0, w


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["B3-items", "B5-items"])
def test_an_item_in_a_batch_is_the_item_alone_snapshot_by_snapshot(sd_np, traced, name):
    cfg = CASES[name]
    eng, Y = _engine(sd_np, "fp32"), _spec(sd_np, cfg["B"], cfg["T"])
    seeds = SEEDS[:cfg["B"]]
    _, tb = _sample(eng, cfg, Y, item_seeds=seeds)
    one = dict(cfg, B=1)
    for b in range(cfg["B"]):
        _, ta = _sample(eng, one, Y[b:b + 1].contiguous(), item_seeds=seeds[b:b + 1])
        assert len(ta) == len(tb)
        for ea, eb in zip(ta, tb):
            assert (ea["kind"], ea["i"], ea["k"], ea["d"], ea["t"]) == (eb["kind"], eb["i"], eb["k"], eb["d"], eb["t"])
            for f in SNAPS:
                if ea[f] is not None:
                    assert _eq(ea[f], eb[f][b:b + 1]), (name, b, ea["index"], ea["kind"], f)


@pytest.mark.gpu
def test_the_trace_is_inert(sd_np):
    """Assertion 5: no bit of the result moves; off, nothing is recorded; on against graphs captured with it off, the trace is complete;
    a configuration past the 256 MB cap is refused and the library goes on."""
    from universal_speech_enhancement_amd import hip_engine
    cfg = CASES["B3-items"]
    eng, Y = _engine(sd_np, "fp32"), _spec(sd_np, 3, 64)
    noise = torch.from_numpy(_draws(cfg)).cuda()
    try:
        hip_engine.set_option("sampler_trace", 0)
        off = {}
        for g in (False, True):
            off[g], t = _sample(eng, cfg, Y, use_graph=g, noise=noise)
            assert t == [] and eng.L.use_sampler_trace_count(eng.h) == 0
        hip_engine.set_option("sampler_trace", 1)                           # against the graphs just captured with it off
        assert eng.stat("plan_stale") == 0
        c0 = eng.stat("graph_captures")
        on_g, tg = _sample(eng, cfg, Y, use_graph=True, noise=noise)
        assert eng.stat("graph_captures") > c0, "graphs captured without the snapshot copies are not replayed for a traced call"
        on_e, te = _sample(eng, cfg, Y, use_graph=False, noise=noise)
        assert _eq(on_g, off[True]) and _eq(on_e, off[False]) and _eq(on_g, on_e)
        assert [e["kind"] for e in tg] == [k for k, *_ in ss.expected_layout(cfg)]
        _same_trace(tg, te, "traced graph after untraced graphs against eager")
        hip_engine.set_option("sampler_trace", 0)                           # and back: the traced graphs are not replayed either
        back, t = _sample(eng, cfg, Y, use_graph=True, noise=noise)
        assert t == [] and eng.L.use_sampler_trace_count(eng.h) == 0 and _eq(back, off[True])
        # the cap: B = 3, N = 200 with one corrector step keeps 802 fields of 768 KiB
        hip_engine.set_option("sampler_trace", 1)
        eng.set_sampler(200, "reverse_diffusion", "langevin", 1, SNR, T_EPS, use_graph=False)
        sent = torch.full_like(Y, complex(3.0, 4.0))
        rc = eng.L.use_sample_cond2(eng.h, Y.data_ptr(), None, None, None, 1, sent.data_ptr(), torch.cuda.current_stream().cuda_stream)
        msg = eng.L.use_last_error().decode()
        assert rc == -1 and "MB" in msg and "sampler_trace" in msg, (rc, msg)
        torch.cuda.synchronize()
        assert bool((sent == complex(3.0, 4.0)).all()) and eng.L.use_sampler_trace_count(eng.h) == 0
        again, ta = _sample(eng, cfg, Y, use_graph=False, noise=noise)
        assert _eq(again, on_e)
        _same_trace(ta, te, "after a refusal")
    finally:
        hip_engine.set_option("sampler_trace", 0)
