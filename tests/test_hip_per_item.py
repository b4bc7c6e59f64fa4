"""GPU tests of batch-invariant sampling (use_sample_items / use_fill_noise_items; ``per_item=True`` of the Python layers): every
item draws from its own Philox stream and takes its own Langevin step, so at equal padded frame count T' an item's output has the same
bits whatever batch it rides in.  Shapes as in test_hip_fused_batch.py: the LARGE synthetic weights, 0.4 s utterances (T' = 64) with
gains an order of magnitude apart, N = 2 reverse steps, Langevin corrector x 1 at snr 0.5; B = 5 runs as 3 + 2 sub-batches.

The bit-identity tests work on spectrograms through the engine (one call of the library per result); the oracle comparisons go
through ``ScoreModel.sample`` to the waveform, as the batch-coupled tests do.
"""
import numpy as np
import pytest
import torch

import lowprec as lp
from oracle import ncsnpp_oracle as no
from oracle import sde_oracle as so
from universal_speech_enhancement_amd.testing import noise as tnoise
from universal_speech_enhancement_amd.testing import weights as tw
from universal_speech_enhancement_amd.testing.cpu import usable_cores

pytestmark = pytest.mark.gpu

GAINS = (1.0, 5.0, 0.2, 2.5, 0.5, 1.5, 0.1, 3.0)
N_STEPS = 2
B = 5
SEEDS = [0x0123456789ABCDEF, 7, 2**64 - 1, 0xDEADBEEF00000000, 31337]
N_DRAWS = 1 + 2 * N_STEPS


def _relmax(a, b):
    a, b = torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu()
    return float((a - b).abs().max() / b.abs().max())


@pytest.fixture(scope="module")
def sd_np():
    return tw.make_state_dict(1234, **tw.LARGE)


_models = {}


def _model(sd_np, precision):
    """One ScoreModel (and so one engine) per precision for the whole module."""
    if precision not in _models:
        from universal_speech_enhancement_amd.sgmse.model_wrapper import ScoreModel
        m = ScoreModel(backbone="ncsnpplarge", sde="ouve", t_eps=3e-2, condition="noisy", n_fft=1022, hop_length=160, num_frames=512,
                       window="hann", sde_input="noisy", predictor="reverse_diffusion", corrector="langevin", precision=precision)
        m.score_net.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
        _models[precision] = m
    return _models[precision]


def _engine(sd_np, precision):
    m = _model(sd_np, precision)
    return m.score_net.engine(512, torch.device("cuda", torch.cuda.current_device()),
                              sde_constants=(m.sde.theta, m.sde.sigma_min, m.sde.sigma_max))


_wavs = {}


def _wav(seed=321, n=B):
    if (seed, n) not in _wavs:
        _wavs[(seed, n)] = torch.from_numpy(tnoise.synth_noisy_speech(n, 9600, seed=seed)) * torch.tensor(GAINS[:n]).view(n, 1)
    return _wavs[(seed, n)]


def _spec(sd_np, wav):
    return _model(sd_np, "fp32")._spectrogram(wav.cuda()).contiguous()


def _run(eng, Y, corrector="langevin", use_graph=True, **kw):
    eng.plan(Y.shape[0], Y.shape[3])
    eng.set_sampler(N_STEPS, "reverse_diffusion", corrector, 1, 0.5, 3e-2, use_graph=use_graph)
    out = eng.sample(Y, **kw)
    torch.cuda.synchronize()
    return out.cpu()


_item_oracle = {}


def _per_item_oracle(sd_np):
    """The CPU oracle run on every item ALONE with its slice of the injected draws (computed once)."""
    if not _item_oracle:
        torch.set_num_threads(usable_cores())
        wav = _wav()
        draws = tnoise.sampler_noise(55, N_DRAWS, (B, 1, 512, 64))
        sd = no.to_torch(sd_np)
        refs = []
        with torch.no_grad():
            for b in range(B):
                ref, _, _, nfe = so.score_model_sample(lambda xx, t: no.ncsnpp_forward(sd, xx, t), wav[b:b + 1], N=N_STEPS,
                                                       predictor="reverse_diffusion", corrector="langevin", corrector_steps=1, snr=0.5,
                                                       noise=so.NoiseSource(replay=[torch.from_numpy(d[b:b + 1]) for d in draws]))
                assert nfe == 2 * N_STEPS
                refs.append(ref[0])
        _item_oracle["v"] = (wav, draws, torch.stack(refs))
    return _item_oracle["v"]


# ---- 1. the noise stream -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 1, 10, 100), (3, 1, 512, 64)])        # 1000 elements per item: no multiple of the 256-thread block
def test_item_noise_is_the_one_item_stream_of_its_seed(shape):
    from universal_speech_enhancement_amd.hip_engine import HipScoreEngine
    eng = HipScoreEngine()
    try:
        n = shape[1] * shape[2] * shape[3]
        seeds = [SEEDS[0], SEEDS[1], SEEDS[0]]
        for d in (0, 1, 7):
            z = eng.fill_noise_items(seeds, d, shape)
            for b in range(3):
                assert torch.equal(z[b:b + 1], eng.fill_noise(seeds[b], d, (1,) + tuple(shape[1:]))), (d, b)
            assert torch.equal(z[0], z[2]), "equal seeds, equal noise"
            corr = abs(complex((z[0].flatten() * z[1].flatten().conj()).sum() / (z[0].abs().pow(2).sum().sqrt() * z[1].abs().pow(2).sum().sqrt())))
            print(f"[measured] draw {d} n={n}: |correlation| of two seeds {corr:.3g} (bound {4 / np.sqrt(n):.3g})")
            assert corr < 4 / np.sqrt(n)
        assert not torch.equal(eng.fill_noise_items(seeds, 0, shape), eng.fill_noise_items(seeds, 1, shape))
    finally:
        eng.close()


# ---- 2. one item = the existing sampler ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("corrector", ["langevin", "ald", "none"])
def test_one_item_equals_use_sample(sd_np, prec, corrector):
    eng = _engine(sd_np, prec)
    Y = _spec(sd_np, _wav())[1:2].contiguous()
    for use_graph in (True, False):
        want = _run(eng, Y, corrector, use_graph, seed=SEEDS[0])
        got = _run(eng, Y, corrector, use_graph, item_seeds=[SEEDS[0]])
        assert torch.isfinite(torch.view_as_real(got)).all()
        assert torch.equal(got, want), (prec, corrector, use_graph)
    assert not torch.equal(_run(eng, Y, corrector, True, item_seeds=[SEEDS[1]]), want)


# ---- 3. invariance at one plan shape -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_position_and_companions_do_not_matter_at_one_plan_shape(sd_np, prec):
    """B = 5 runs as 3 + 2 sub-batches, so the reversed order moves items between sub-batches of different sizes.  In fp32 that pins the
    per-image kernel choice of the per-item loop: conv_sk picks its tile form (K passes of 64 or of 128 channels, i.e. another order
    of additions) by the workgroup count of the whole sub-batch in the default sampler, which on the 128 x 16 maps of this shape
    differs between 2 and 3 items."""
    eng = _engine(sd_np, prec)
    Y = _spec(sd_np, _wav())
    others = _spec(sd_np, _wav(seed=99) * 1.7)
    Yc = torch.cat([Y[:1], others[1:]]).contiguous()                           # items 1..4 replaced by other utterances
    rev = list(range(B))[::-1]
    outs = {}
    for use_graph in (True, False):
        a = _run(eng, Y, use_graph=use_graph, item_seeds=SEEDS)
        p = _run(eng, Y[rev].contiguous(), use_graph=use_graph, item_seeds=[SEEDS[b] for b in rev])
        c = _run(eng, Yc, use_graph=use_graph, item_seeds=SEEDS)
        for b in range(B):
            assert torch.equal(p[B - 1 - b], a[b]), (prec, use_graph, b)
        assert torch.equal(c[0], a[0]), (prec, use_graph)
        assert not torch.equal(c[1], a[1])
        outs[use_graph] = a
    assert torch.equal(outs[True], outs[False]), "hipGraph replay must be bit-identical to eager launches"
    # what the test can see: the batch-coupled form does move item 0 when its companions change
    a = _run(eng, Y, seed=5)
    c = _run(eng, Yc, seed=5)
    assert not torch.equal(a[0], c[0])


# ---- 4. invariance across batch sizes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_an_item_alone_and_as_item_3_of_5(sd_np, prec):
    """Item 3 of B = 5 sits in the sub-batch of 2 items, item 0 in that of 3: both are checked against the item alone."""
    eng = _engine(sd_np, prec)
    Y = _spec(sd_np, _wav())
    x = Y + torch.from_numpy(tnoise.complex_normal(17, "per_item_x", tuple(Y.shape))).cuda() * 0.3
    t = torch.tensor([0.9, 0.7, 0.5, 0.4, 0.2]).cuda()
    s5 = eng.score(x, Y, t).cpu()
    s1 = eng.score(x[3:4].contiguous(), Y[3:4].contiguous(), t[3:4].contiguous()).cpu()
    assert torch.equal(s1[0], s5[3]), f"{prec}: one score evaluation of an item differs between B = 1 and item 3 of B = 5"
    for use_graph in (True, False):
        a = _run(eng, Y, use_graph=use_graph, item_seeds=SEEDS)
        one = _run(eng, Y[3:4].contiguous(), use_graph=use_graph, item_seeds=SEEDS[3:4])
        assert torch.equal(one[0], a[3]), (prec, use_graph)
        assert torch.equal(_run(eng, Y[0:1].contiguous(), use_graph=use_graph, item_seeds=SEEDS[0:1])[0], a[0]), (prec, use_graph)
    assert torch.equal(one, _run(eng, Y[3:4].contiguous(), seed=SEEDS[3])), "... which is use_sample of that item with that seed"


# ---- 5. against the oracle, item by item ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
def test_every_item_matches_the_oracle_run_on_it_alone(sd_np, prec):
    wav, draws, ref = _per_item_oracle(sd_np)
    tol = 2e-3 if prec == "fp32" else lp.chain_bound(prec, "wav", "relmax")
    m = _model(sd_np, prec)
    out = m.sample({"perturbed": wav.cuda()}, N=N_STEPS, corrector_steps=1, snr=0.5, noise=torch.from_numpy(draws).cuda(),
                   per_item=True)["enhanced"].cpu()
    errs = [_relmax(out[b], ref[b]) for b in range(B)]
    for b in range(B):
        print(f"[measured] per-item langevin {prec} item {b} (gain {GAINS[b]}): {errs[b]:.3g} (bound {tol:g})")
    assert max(errs) < tol, (prec, errs)


# ---- 6. negative control -------------------------------------------------------------------------------------------------------
def test_the_batch_coupled_form_does_not_match_the_per_item_oracle(sd_np):
    """The default sampler on the same call: its Langevin step is a batch mean, so it is off the item-alone oracle by far more than the
    bound of the test above (the oracle itself shows 1.7e-2 ... 0.33 between B = 5 coupled and the five runs at B = 1 on these gains)."""
    wav, draws, ref = _per_item_oracle(sd_np)
    m = _model(sd_np, "fp32")
    out = m.sample({"perturbed": wav.cuda()}, N=N_STEPS, corrector_steps=1, snr=0.5, noise=torch.from_numpy(draws).cuda())["enhanced"].cpu()
    errs = [_relmax(out[b], ref[b]) for b in range(B)]
    print("[measured] batch-coupled against the per-item oracle:", ["%.3g" % e for e in errs])
    assert max(errs) > 2e-2, errs


# ---- 7. device noise = its own replay ------------------------------------------------------------------------------------------
def test_device_noise_equals_its_replay(sd_np):
    eng = _engine(sd_np, "fp32")
    Y = _spec(sd_np, _wav())
    z = torch.stack([eng.fill_noise_items(SEEDS, d, Y.shape) for d in range(N_DRAWS)])
    for use_graph in (True, False):
        a = _run(eng, Y, use_graph=use_graph, item_seeds=SEEDS)
        r = _run(eng, Y, use_graph=use_graph, noise=z, per_item=True)
        assert torch.equal(a, r), use_graph
    m = _model(sd_np, "fp32")                                                  # and through the public keywords
    w = m.sample({"perturbed": _wav().cuda()}, N=N_STEPS, corrector_steps=1, snr=0.5, per_item=True, item_seeds=SEEDS)["enhanced"]
    w2 = m.sample({"perturbed": _wav().cuda()}, N=N_STEPS, corrector_steps=1, snr=0.5, per_item=True, noise=z)["enhanced"]
    assert torch.equal(w, w2)


# ---- 8. chunked ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_chunked_result_does_not_depend_on_chunk_batch(sd_np, prec):
    """Groups of 2, 3 and 8 windows are plans of other sizes with other sub-batch splits (2, 3, 3 + 3 + 2)."""
    m = _model(sd_np, prec)
    Y = (torch.from_numpy(tnoise.complex_normal(23, "per_item_chunk", (2, 1, 512, 192))) * torch.tensor([0.4, 0.05]).view(2, 1, 1, 1)).cuda()
    kw = dict(N=N_STEPS, corrector_steps=1, snr=0.5, chunk_frames=64, chunk_overlap=16)
    outs = {cb: m.sample_spec_chunked(Y, [Y], chunk_batch=cb, per_item=True, item_seeds=SEEDS[:2], **kw).cpu() for cb in (2, 3, 8)}
    assert torch.isfinite(torch.view_as_real(outs[2])).all()
    assert torch.equal(outs[2], outs[3]) and torch.equal(outs[2], outs[8])
    one = m.sample_spec_chunked(Y[1:2].contiguous(), [Y[1:2].contiguous()], chunk_batch=3, per_item=True, item_seeds=SEEDS[1:2], **kw).cpu()
    assert torch.equal(one[0], outs[2][1]), "a file alone gives the bits it has beside another file"
    d2 = m.sample_spec_chunked(Y, [Y], chunk_batch=2, seed=4, **kw).cpu()        # the default form: groups are coupled
    d3 = m.sample_spec_chunked(Y, [Y], chunk_batch=3, seed=4, **kw).cpu()
    assert not torch.equal(d2, d3)


# ---- 9. graph bookkeeping ------------------------------------------------------------------------------------------------------
def test_both_forms_keep_their_graphs_on_one_plan(sd_np):
    eng = _engine(sd_np, "bf16")
    Y = _spec(sd_np, _wav())
    eng.plan(B, 64)
    eng.set_sampler(N_STEPS, "reverse_diffusion", "langevin", 1, 0.5, 3e-2, use_graph=False)   # another configuration: the graphs below are new
    first = _run(eng, Y, seed=11)
    c0 = eng.stat("graph_captures")
    item = _run(eng, Y, item_seeds=SEEDS)
    c1 = eng.stat("graph_captures")
    assert c1 > c0, "the per-item loop has graphs of its own"
    for _ in range(2):
        assert torch.equal(_run(eng, Y, seed=11), first)
        assert torch.equal(_run(eng, Y, item_seeds=SEEDS), item)
    assert eng.stat("graph_captures") == c1, "switching between the forms re-captured a graph"
    assert not torch.equal(_run(eng, Y, item_seeds=SEEDS[::-1]), item), "a replayed graph reads the new seeds"
    assert eng.stat("graph_captures") == c1


# ---- 10. the ODE sampler -------------------------------------------------------------------------------------------------------
def test_ode_prior_is_per_item(sd_np):
    m = _model(sd_np, "fp32")
    Y = _spec(sd_np, _wav())[:3].contiguous()
    Y2 = torch.cat([Y[:1], _spec(sd_np, _wav(seed=99) * 1.7)[1:3]]).contiguous()
    kw = dict(N=30, per_item=True, item_seeds=SEEDS[:3], minibatch=1, rtol=1e-3, atol=1e-3)
    a, na = m.get_ode_sampler(Y, conditioning=[Y], **kw)()
    b, nb = m.get_ode_sampler(Y2, conditioning=[Y2], **kw)()
    print("[measured] per-item ODE nfev", na, nb)
    assert torch.equal(a[0], b[0]) and na[0] == nb[0]
    assert not torch.equal(a[1], b[1])
    c, nc = m.get_ode_sampler(Y, conditioning=[Y], **{**kw, "item_seeds": [SEEDS[3]] + SEEDS[1:3]})()
    assert not torch.equal(c[0], a[0]), "the prior of item 0 comes from its own seed"
    assert torch.equal(c[1], a[1]) and nc[1] == na[1]
