"""Chunked sampling of long recordings on the GPU: the split and cross-fade merge kernels against numpy (tests/chunk_ref.py: bit-equal
copies, float64 cross-fades with the float32 bound 4 * 2^-24 * (|A| + |B|) per real component, no element left out), and the chunked
paths of ScoreModel / NCSNPP_Wrapper / predict against their own composition: numpy split -> the un-chunked entry point per group ->
float64 merge.  The sampler is bit-reproducible for equal inputs, so the merge bound is the only slack there as well."""
import numpy as np
import pytest
import torch

import chunk_ref as cr
from universal_speech_enhancement_amd.testing import noise as tnoise
from universal_speech_enhancement_amd.testing import weights as tw

pytestmark = pytest.mark.gpu

GEOMETRIES = cr.CASES + [cr.ODD_HOP]
SHAPES = [(1, 512), (3, 512), (1, 3), (3, 3)]          # (B, F); F = 3 catches row-stride assumptions


def _cn(seed, tag, shape):
    return tnoise.complex_normal(seed, tag, shape)


def _bits(a):
    """complex64 [..., T] -> uint32 [..., T, 2]: the bit patterns of the real and imaginary parts."""
    a = np.ascontiguousarray(a)
    assert a.dtype == np.complex64
    return a.view(np.uint32).reshape(a.shape + (2,))


def _unaligned(a):
    """The same values in a CUDA tensor that starts 8 bytes off a 16-byte boundary (contiguous: it is used as it is)."""
    flat = torch.empty(a.size + 1, dtype=torch.complex64, device="cuda")
    t = flat[1:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.is_contiguous() and t.data_ptr() % 16 == 8
    return t


@pytest.mark.parametrize("Tp,C,overlap", GEOMETRIES)
def test_split_is_numpy_slicing_with_a_zero_tail(Tp, C, overlap):
    from universal_speech_enhancement_amd.hip_engine import chunk_split
    for B, F in SHAPES:
        Y = _cn(Tp + overlap, f"split{B}x{F}", (B, 1, F, Tp))
        want = cr.ref_split(Y, C, overlap)
        for tag, dev in (("aligned", torch.from_numpy(Y).cuda()), ("unaligned", _unaligned(Y))):
            got = chunk_split(dev, C, overlap).cpu().numpy()
            assert got.shape == want.shape and got.dtype == np.complex64
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (tag, B, F)


@pytest.mark.parametrize("Tp,C,overlap", GEOMETRIES)
def test_merge_cross_fades_random_chunks(Tp, C, overlap):
    """Random windows, so that the two sides of an overlap differ."""
    from universal_speech_enhancement_amd.hip_engine import chunk_merge
    n = cr.ref_plan(Tp, C, overlap)[0]
    for B, F in SHAPES:
        chunks = _cn(Tp + overlap, f"merge{B}x{F}", (B * n, 1, F, C))
        ref, bound = cr.ref_merge(chunks, B, Tp, C, overlap)
        for tag, dev in (("aligned", torch.from_numpy(chunks).cuda()), ("unaligned", _unaligned(chunks))):
            a = chunk_merge(dev, B, Tp, C, overlap)
            assert tuple(a.shape) == (B, 1, F, Tp)
            cr.check_merged(a.cpu().numpy(), ref, bound, f"merge {tag} B={B} F={F} ({Tp}, {C}, {overlap})")
            assert torch.equal(a, chunk_merge(dev, B, Tp, C, overlap))            # deterministic


@pytest.mark.parametrize("Tp,C,overlap", GEOMETRIES)
def test_round_trip(Tp, C, overlap):
    from universal_speech_enhancement_amd.hip_engine import chunk_merge, chunk_split
    fade = cr.overlap_mask(Tp, C, overlap)
    for B, F in SHAPES:
        Y = _cn(Tp + overlap, f"rt{B}x{F}", (B, 1, F, Tp))
        X = chunk_merge(chunk_split(torch.from_numpy(Y).cuda(), C, overlap), B, Tp, C, overlap).cpu().numpy()
        bound = np.zeros((B, 1, F, Tp, 2))
        bound[..., fade, 0] = 4 * 2.0 ** -24 * 2 * np.abs(Y.real[..., fade])            # A = B = Y in the overlaps
        bound[..., fade, 1] = 4 * 2.0 ** -24 * 2 * np.abs(Y.imag[..., fade])
        cr.check_merged(X, Y.astype(np.complex128), bound, f"round trip B={B} F={F} ({Tp}, {C}, {overlap})")
        assert np.array_equal(_bits(X)[..., ~fade, :], _bits(Y)[..., ~fade, :])


def test_wrappers_refuse_what_the_geometry_refuses():
    from universal_speech_enhancement_amd.hip_engine import chunk_merge, chunk_split
    Y = torch.zeros((1, 1, 3, 192), dtype=torch.complex64, device="cuda")
    with pytest.raises(ValueError, match="chunk_frames"):
        chunk_split(Y, 100, 16)
    with pytest.raises(ValueError, match="overlap"):
        chunk_split(Y, 64, 33)
    with pytest.raises(ValueError, match="expected"):
        chunk_merge(torch.zeros((3, 1, 3, 64), dtype=torch.complex64, device="cuda"), 1, 192, 64, 16)     # 4 windows, not 3


# ---- through the sampler -------------------------------------------------------------------------------------------------------
C_, OV_, CB_ = 64, 16, 2
N_ = 2


@pytest.fixture(scope="module")
def sd_np():
    return tw.make_state_dict(1234, **tw.LARGE)


def _score_model(sd_np, precision):
    from universal_speech_enhancement_amd.sgmse.model_wrapper import ScoreModel
    m = ScoreModel(backbone="ncsnpplarge", sde="ouve", t_eps=3e-2, condition="noisy", n_fft=1022, hop_length=160, num_frames=512,
                   window="hann", sde_input="noisy", predictor="reverse_diffusion", corrector="langevin", precision=precision)
    m.score_net.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
    return m


@pytest.fixture(scope="module")
def models(sd_np):
    return {prec: _score_model(sd_np, prec) for prec in ("fp32", "bf16")}


def _wav(frames, seed=7, n=1):
    """`frames` STFT frames of signal at hop 160 (T = 1 + L // 160)."""
    return torch.from_numpy(tnoise.synth_noisy_speech(n, (frames - 1) * 160, seed=seed)).cuda()


def _composition(m, Y, noise, seed):
    """numpy split -> fused_sample on groups of two windows -> float64 numpy merge."""
    B, _, _, Tp = Y.shape
    chunks = cr.ref_split(Y.cpu().numpy(), C_, OV_)
    outs = []
    for g, lo in enumerate(range(0, chunks.shape[0], CB_)):
        yg = torch.from_numpy(chunks[lo:lo + CB_]).cuda()
        outs.append(m.fused_sample(yg, N=N_, predictor="reverse_diffusion", corrector="langevin", corrector_steps=1, snr=0.5, t_eps=m.t_eps,
                                   noise=None if noise is None else noise[:, lo:lo + CB_].contiguous(), seed=seed + g).cpu().numpy())
    return cr.ref_merge(np.concatenate(outs), B, Tp, C_, OV_)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_chunked_sampler_is_the_composition(models, prec):
    """B = 1, 150 frames of signal (T' = 192): four windows of 64 frames, 16 shared, in two groups of two; injected noise."""
    m = models[prec]
    Y = m._spectrogram(_wav(150))
    assert tuple(Y.shape) == (1, 1, 512, 192)
    noise = torch.from_numpy(tnoise.sampler_noise(11, 1 + 2 * N_, (4, 1, 512, C_))).cuda()
    out = m.sample_spec_chunked(Y, [Y], N=N_, corrector_steps=1, snr=0.5, noise=noise, chunk_frames=C_, chunk_overlap=OV_, chunk_batch=CB_)
    assert tuple(out.shape) == (1, 1, 512, 192) and m.last_nfe == [2 * N_, 2 * N_]
    ref, bound = _composition(m, Y, noise, 0)
    cr.check_merged(out.cpu().numpy(), ref, bound, f"chunked sampler, injected noise, {prec}")
    with pytest.raises(ValueError, match="windows"):
        m.sample_spec_chunked(Y, [Y], N=N_, noise=noise[:, :3], chunk_frames=C_, chunk_overlap=OV_, chunk_batch=CB_)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_group_g_samples_with_seed_plus_g(models, prec):
    m = models[prec]
    Y = m._spectrogram(_wav(150))
    out = m.sample_spec_chunked(Y, [Y], N=N_, corrector_steps=1, snr=0.5, seed=40, chunk_frames=C_, chunk_overlap=OV_, chunk_batch=CB_)
    ref, bound = _composition(m, Y, None, 40)
    cr.check_merged(out.cpu().numpy(), ref, bound, f"chunked sampler, device noise, {prec}")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_chunked_ode_sampler_is_the_composition(models, prec):
    """The ODE sampler over four windows in two groups: the prior's draw [B * n, 1, F, C] sliced per group, then device noise with
    seed + g; against numpy split -> the un-chunked ODE sampler per group -> float64 merge."""
    m = models[prec]
    Y = m._spectrogram(_wav(150))
    chunks = cr.ref_split(Y.cpu().numpy(), C_, OV_)
    ode = dict(N=N_, rtol=1e-2, atol=1e-2)
    prior = torch.from_numpy(tnoise.sampler_noise(13, 1, (4, 1, 512, C_))[0]).cuda()
    for noise, seed in ((prior, 0), (None, 21)):
        out = m.sample_spec_chunked(Y, [Y], sampler_type="ode", noise=noise, seed=seed, chunk_frames=C_, chunk_overlap=OV_, chunk_batch=CB_, **ode)
        nfe, outs = [], []
        for g, lo in enumerate(range(0, 4, CB_)):
            yg = torch.from_numpy(chunks[lo:lo + CB_]).cuda()
            x, n = m.get_ode_sampler(yg, conditioning=[yg], noise=None if noise is None else noise[lo:lo + CB_], seed=seed + g, **ode)()
            outs.append(x.cpu().numpy()); nfe.append(n)
        assert m.last_nfe == nfe and all(len(n) == CB_ for n in nfe)          # one RK45 integration per window (minibatch = 1)
        ref, bound = cr.ref_merge(np.concatenate(outs), 1, 192, C_, OV_)
        cr.check_merged(out.cpu().numpy(), ref, bound, f"chunked ODE sampler, {'injected' if seed == 0 else 'device'} noise, {prec}")


@pytest.mark.parametrize("sampler", ["pc", "ode"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_a_single_chunk_is_the_unchunked_path(models, prec, sampler):
    m = models[prec]
    wav = _wav(61)                                                        # T' = 64
    kw = dict(N=N_, seed=3) if sampler == "pc" else dict(sampler_type="ode", N=N_, seed=3, rtol=1e-2, atol=1e-2)
    plain = m.sample({"perturbed": wav}, **kw)["enhanced"].clone()
    for C in (64, 128):                                                   # T' = C and T' < C
        chunked = m.sample({"perturbed": wav}, chunk_frames=C, chunk_overlap=16, chunk_batch=2, **kw)["enhanced"]
        assert torch.equal(plain, chunked), (prec, sampler, C)
    with pytest.raises(ValueError, match="chunk_frames"):
        m.sample({"perturbed": wav}, chunk_frames=100, **kw)
    with pytest.raises(ValueError, match="overlap"):
        m.sample({"perturbed": wav}, chunk_frames=64, **kw)               # the default overlap of 64 exceeds 64 / 2


def test_sample_and_enhance_take_the_chunked_path(models):
    """sample() / enhance() with T' above chunk_frames: the waveform of sample_spec_chunked's spectrogram."""
    m = models["bf16"]
    wav = _wav(150)
    Y = m._spectrogram(wav)
    kw = dict(N=N_, corrector_steps=1, snr=0.5, seed=9, chunk_frames=C_, chunk_overlap=OV_, chunk_batch=CB_)
    want = m._waveform(m.sample_spec_chunked(Y, [Y], **kw), wav.shape[1])
    got = m.sample({"perturbed": wav}, **kw)["enhanced"]
    assert got.shape == wav.shape and torch.equal(got, want)
    peak = wav.abs().max().item()
    Yn = m._spectrogram(wav / peak)
    want = (m._waveform(m.sample_spec_chunked(Yn, [Yn], predictor="reverse_diffusion", corrector="ald", **kw), wav.shape[1]) * peak).squeeze().cpu()
    got = m.enhance(wav, predictor="reverse_diffusion", corrector="ald", **kw)
    assert torch.equal(got, want)
    # timeit: the NFE of a "pc" run is an int as un-chunked, and ODE options are ignored for "pc" as un-chunked
    got, nfe, rtf = m.enhance(wav, predictor="reverse_diffusion", corrector="ald", timeit=True, rtol=1e-2, **kw)
    assert torch.equal(got, want) and nfe == 2 * N_ and rtf > 0


def test_plans_and_workspace_do_not_depend_on_the_file_length(sd_np):
    from universal_speech_enhancement_amd.hip_engine import HipScoreEngine
    m = _score_model(sd_np, "bf16")
    kw = dict(N=N_, corrector_steps=1, snr=0.5, seed=1, chunk_frames=C_, chunk_overlap=OV_, chunk_batch=CB_)
    a = m.sample({"perturbed": _wav(150)}, **kw)["enhanced"]             # B = 1, T' = 192: 4 windows
    eng = m.score_net.engine(512, a.device)
    first = (eng.stat("plans_built"), eng.stat("graph_captures"))
    b = m.sample({"perturbed": _wav(100, n=2)}, **kw)["enhanced"]        # B = 2, T' = 128: 2 x 3 windows
    assert torch.isfinite(a).all() and torch.isfinite(b).all() and b.shape == (2, 99 * 160)
    assert (eng.stat("plans_built"), eng.stat("graph_captures")) == first and first[0] == 1
    fresh = HipScoreEngine(precision="bf16")
    fresh.load_state_dict(sd_np)
    fresh.plan(CB_, C_)
    assert eng.workspace_bytes() == fresh.workspace_bytes()
    fresh.close()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_refine_stage_chunked_is_the_composition(prec):
    from universal_speech_enhancement_amd.LSGAN_module import GANModule
    from universal_speech_enhancement_amd.gan.ncsnpp_wrapper import NCSNPP_Wrapper
    w = NCSNPP_Wrapper(n_fft=1022, hop_length=160, num_frames=480, precision=prec)
    w.net.load_state_dict({k: torch.from_numpy(v) for k, v in tw.make_state_dict(4321, **tw.REFINE).items()}, strict=True)
    wav = _wav(150)
    spec = w._spectrogram(wav)
    out = w.refine_spec_chunked(spec, C_, OV_, CB_)
    chunks = cr.ref_split(spec.cpu().numpy(), C_, OV_)
    fwd = [w.net(torch.from_numpy(chunks[lo:lo + CB_]).cuda()).cpu().numpy() for lo in range(0, chunks.shape[0], CB_)]
    ref, bound = cr.ref_merge(np.concatenate(fwd), 1, 192, C_, OV_)
    cr.check_merged(out.cpu().numpy(), ref, bound, f"refine stage, {prec}")
    # the module passes the keys on; the waveform is that spectrogram's
    got = GANModule(G=w, sampler_kwargs=dict(chunk_frames=C_, chunk_overlap=OV_, chunk_batch=CB_)).predict_step({"perturbed": wav})["fake"]
    assert torch.equal(got, w._waveform(out, wav.shape[1]))
    short = _wav(61)                                                      # one window: bit-identical to the plain forward
    plain = w({"perturbed": short})["fake"].clone()
    assert torch.equal(plain, w({"perturbed": short}, chunk_frames=64, chunk_overlap=16)["fake"])


def test_predict_cli_with_chunk_frames(tmp_path):
    from scipy.io import wavfile
    from universal_speech_enhancement_amd import predict as P
    src, dst = tmp_path / "noisy", tmp_path / "enhanced"
    src.mkdir()
    w = tnoise.synth_noisy_speech(1, 36000, seed=3)[0]                    # 1.5 s at 24 kHz: T' = 256, five windows of 64 frames, 16 shared
    wavfile.write(str(src / "a.wav"), 24000, w.astype(np.float32))
    n = P.predict(P.compose(["model=SGMSE_Large", f"data.data_folder={src}", f"data.target_folder={dst}", "random_init_seed=1",
                             "model.sampler_kwargs.N=2", "model.sampler_kwargs.chunk_frames=64", "model.sampler_kwargs.chunk_overlap=16",
                             "model.wav_subtype=FLOAT"]))              # float32 samples: a NaN or Inf of the sampler reaches the file
    assert n == 1
    sr, a = wavfile.read(str(dst / "a.wav"))
    assert sr == 24000 and a.dtype == np.float32 and a.shape == (36000,) and np.isfinite(a).all() and np.abs(a).max() > 0


def test_c_host_with_chunk_flags(tmp_path, sd_np):
    """examples/enhance_wav --chunk-frames / --chunk-overlap: use_chunk_count / _split / _merge from a C host, groups of eight windows
    with seed + g, against the Python host on the same file.  1 s at 24 kHz is T' = 192: four windows of 64 frames, one group.  The
    two hosts differ in the last bit of the Hann window, which the randomly initialised network amplifies; the bounds are those of
    the un-chunked comparison in test_hip_parity.py, where that difference is the same."""
    import os
    import subprocess
    from scipy.io import wavfile
    from universal_speech_enhancement_amd import wavio
    from universal_speech_enhancement_amd.hip_engine import HipScoreEngine
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "enhance_wav")
    if not os.path.exists(exe):
        pytest.fail("examples/enhance_wav is not built (run __graft_entry__.build())")
    blob, src, dst = str(tmp_path / "large_fp32.usehip"), str(tmp_path / "in.wav"), str(tmp_path / "out.wav")
    e = HipScoreEngine(precision="fp32"); e.load_state_dict(sd_np); e.save_weight_blob(blob); e.close()
    wavfile.write(src, 24000, (tnoise.synth_noisy_speech(1, 24000, seed=21)[0] * 0.5 * 32767).astype(np.int16))
    r = subprocess.run([exe, blob, src, dst, "2", "7", "fp32", "--chunk-frames", "64", "--chunk-overlap", "16"], capture_output=True, text=True)
    assert r.returncode == 0 and "4 windows of 64 frames" in r.stdout, r.stderr + r.stdout
    sr, got = wavfile.read(dst)
    x, _ = wavio.load_utterance(src, 24000, True)
    assert sr == 24000 and got.dtype == np.int16 and got.shape == x.shape == (24000,)
    m = _score_model(sd_np, "fp32")
    want = m.sample({"perturbed": torch.from_numpy(x)[None].cuda()}, N=2, corrector_steps=1, snr=0.5, seed=7, chunk_frames=64, chunk_overlap=16,
                    chunk_batch=8)["enhanced"][0].cpu().numpy()
    want16 = np.clip(np.rint(want.astype(np.float64) * 32767.0), -32768, 32767).astype(np.int16)
    d = np.abs(got.astype(np.int32) - want16.astype(np.int32))
    print(f"C host against Python host, chunked: max {int(d.max())} LSB, mean {float(d.mean()):.3f} LSB")
    assert d.max() <= 164 and d.mean() < 2.0, (int(d.max()), float(d.mean()))
    # the flags' values are checked: nothing unparsable or refused by the geometry turns chunking off silently
    for flags, word in ((["--chunk-frames", "64x"], "frame count"), (["--chunk-frames", "0"], "chunk_frames"), (["--chunk-frames", "100"], "chunk_frames"),
                        (["--chunk-frames", "64", "--chunk-overlap", "33"], "overlap"), (["--chunk-frames"], "needs a value")):
        bad = subprocess.run([exe, blob, src, str(tmp_path / "o.wav")] + flags, capture_output=True, text=True)
        assert bad.returncode != 0 and word in bad.stderr and not os.path.exists(str(tmp_path / "o.wav")), (flags, bad.stderr)
