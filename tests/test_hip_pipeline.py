"""GPU tests of the one-run pipeline: the hand-off kernel (``use_wav_handoff``) against tests/handoff_ref.py, bit for bit, and
``USEModule`` / ``predict model=USE`` / ``enhance_wav --refine`` against the two-run flow they replace, byte for byte: the refine stage
over the pipeline's own stage-1 files must write what the pipeline wrote.  Weights: the LARGE / REFINE synthetic ones, n_fft 1022, hop
160, N = 2 reverse steps."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import handoff_ref as hr
from universal_speech_enhancement_amd.testing import noise as tnoise
from universal_speech_enhancement_amd.testing import weights as tw

pytestmark = pytest.mark.gpu

COMBOS = [("PCM_16", True), ("PCM_16", False), ("FLOAT", True), ("FLOAT", False)]
TIES = np.array([0.5, -0.5, 1.5, -1.5], np.float32)                               # x * 32767 is an exact .5 tie only for x = odd / 2


def _same(got: torch.Tensor, want: np.ndarray) -> bool:
    """torch.equal with NaNs allowed in the same places."""
    got, want = got.cpu(), torch.from_numpy(np.ascontiguousarray(want))
    return (got.shape == want.shape and got.dtype == want.dtype and torch.equal(torch.isnan(got), torch.isnan(want))
            and torch.equal(torch.nan_to_num(got, nan=7.0), torch.nan_to_num(want, nan=7.0)))


def _base_batch():
    """B = 4, stride 4099 (odd: rows are misaligned for vector loads), lengths (4099, 4097, 65, 1); the padding of every row holds 1e9."""
    rng = np.random.default_rng(99)
    lens = (4099, 4097, 65, 1)
    wav = np.full((4, 4099), 1e9, np.float32)
    for b, L in enumerate(lens):
        wav[b, :L] = (rng.standard_normal(L) * (0.05, 0.6, 0.2, 0.3)[b]).astype(np.float32)
    wav[0, 4098] = 0.71                                                            # row 0: the peak is the last valid sample
    wav[1, 1234] = -3.25                                                           # row 1: beyond +-1, the peak a negative sample ...
    wav[1, 10:14] = TIES                                                           # ... and the exact ties
    wav[1, 14:18] = np.nextafter(TIES, np.float32(0))
    wav[2, 60:64] = TIES
    return wav, lens


# ---- 1. the kernel against the reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("subtype,normalize", COMBOS)
def test_handoff_equals_the_reference_bit_for_bit(subtype, normalize):
    from universal_speech_enhancement_amd.handoff import wav_handoff
    wav, lens = _base_batch()
    want, wpeak = hr.handoff_batch(wav, lens, subtype, normalize)
    src = torch.from_numpy(wav).cuda()
    out, peaks = wav_handoff(src, lens, subtype, normalize)
    assert out is not src and torch.equal(src.cpu(), torch.from_numpy(wav))        # the input is untouched
    assert _same(out, want) and _same(peaks, wpeak), (subtype, normalize)
    assert not out[1, 4097:].any() and not out[2, 65:].any() and not out[3, 1:].any()   # 1e9 of the padding neither read nor kept
    if normalize:
        assert abs(float(out[0, 4098])) == np.float32(0.8) and float(out[1, 1234]) == -np.float32(0.8)
    # in place
    same, peaks2 = wav_handoff(src, lens, subtype, normalize, out=src)
    assert same is src and _same(src, want) and _same(peaks2, wpeak)
    # the same bits in another batch composition and at another stride: row 1 alone, in a wider buffer at an even offset
    solo = torch.full((1, 4200), 1e9, device="cuda")
    solo[0, :4097] = torch.from_numpy(wav[1, :4097]).cuda()
    o1, p1 = wav_handoff(solo, [4097], subtype, normalize)
    assert _same(o1[0, :4099], want[1]) and not o1[0, 4097:].any() and float(p1[0]) == wpeak[1]
    # 1-D: one signal
    o2, p2 = wav_handoff(torch.from_numpy(wav[2, :65]).cuda(), None, subtype, normalize)
    assert o2.shape == (65,) and _same(o2, want[2, :65]) and float(p2[0]) == wpeak[2]


@pytest.mark.parametrize("subtype", ["PCM_16", "FLOAT"])
def test_a_silent_row_gives_nan_as_the_loader_does(subtype):
    from universal_speech_enhancement_amd.handoff import wav_handoff
    wav, lens = _base_batch()
    wav[2, :65] = 0.0
    wav[2, 3] = 1e-6 if subtype == "PCM_16" else 0.0                               # below half an LSB: silent once it is a 16-bit file
    want, wpeak = hr.handoff_batch(wav, lens, subtype, True)
    out, peaks = wav_handoff(torch.from_numpy(wav).cuda(), lens, subtype, True)
    assert np.isnan(want[2, :65]).all() and not want[2, 65:].any() and wpeak[2] == 0.0
    assert _same(out, want) and _same(peaks, wpeak)
    out, peaks = wav_handoff(torch.from_numpy(wav).cuda(), lens, subtype, False)
    assert not torch.isnan(out).any() and float(peaks[2]) == 0.0


def test_handoff_reduces_the_peak_over_many_slices():
    """B = 1, L = 3 * 2^20 + 5: 193 slices; the peak lies in the last one, five samples from the end."""
    from universal_speech_enhancement_amd.handoff import wav_handoff
    L = 3 * 2**20 + 5
    wav = (np.random.default_rng(3).standard_normal((1, L)) * 0.1).astype(np.float32)
    wav[0, L - 5] = -0.97
    want, wpeak = hr.handoff_batch(wav, [L])
    out, peaks = wav_handoff(torch.from_numpy(wav).cuda(), [L])
    assert wpeak[0] == 31784 / 32768 and _same(peaks, wpeak) and _same(out, want)
    want, wpeak = hr.handoff_batch(wav, [L], "FLOAT")
    out, peaks = wav_handoff(torch.from_numpy(wav).cuda(), [L], "FLOAT")
    assert _same(peaks, wpeak) and _same(out, want)


def test_handoff_row_offsets_are_64_bit():
    """B = 3, stride 2^30 + 3: row 2 starts 2^31 + 6 elements into one 12.9 GB buffer.  In place; the 1000 valid samples of every row
    are compared (the reference takes them row by row - tests/test_handoff_host.py), and the zero padding is probed."""
    from universal_speech_enhancement_amd.handoff import wav_handoff
    stride, L = 2**30 + 3, 1000
    rows = (np.random.default_rng(8).standard_normal((3, L)) * np.array([[0.05], [0.3], [0.9]])).astype(np.float32)
    buf = torch.empty((3, stride), dtype=torch.float32, device="cuda")             # uninitialised past the valid samples: never read
    buf[:, :L] = torch.from_numpy(rows).cuda()
    buf[:, L:L + 64] = 1e9
    buf[:, -64:] = 1e9
    out, peaks = wav_handoff(buf, [L] * 3, "PCM_16", True, out=buf)
    assert out is buf
    for b, (want, mx) in enumerate(hr.handoff_rows(rows, [L] * 3)):
        assert _same(buf[b, :L], want) and float(peaks[b]) == mx, b
        assert not buf[b, L:L + 4096].any() and not buf[b, -4096:].any() and not buf[b, 2**29:2**29 + 4096].any(), b
    del buf, out
    torch.cuda.empty_cache()


def test_handoff_error_codes():
    """Every refusal is USE_E_INVALID (-1) with the argument named, before anything is launched."""
    from universal_speech_enhancement_amd import _lib
    from universal_speech_enhancement_amd.handoff import wav_handoff
    lib = _lib.lib()
    B, stride = 2, 300
    wav = torch.full((B, stride), 0.25, device="cuda")
    out = torch.full((B, stride), 5.0, device="cuda")
    peak = torch.full((B,), 5.0, dtype=torch.float64, device="cuda")
    nbytes = lib.use_wav_handoff_workspace(B, stride)
    assert nbytes >= B * 4 + B * 8 and lib.use_wav_handoff_workspace(0, stride) == 0 and lib.use_wav_handoff_workspace(B, 0) == 0
    work = torch.zeros((nbytes + 7) // 8, dtype=torch.float64, device="cuda")
    lens = (C.c_int * B)(300, 1)
    stream = torch.cuda.current_stream().cuda_stream

    def call(**kw):
        a = dict(inp=wav.data_ptr(), out=out.data_ptr(), stride=stride, lens=lens, B=B, subtype=0, normalize=1, work=work.data_ptr(),
                 nbytes=nbytes, peak=peak.data_ptr())
        a.update(kw)
        rc = lib.use_wav_handoff(a["inp"], a["out"], a["stride"], a["lens"], a["B"], a["subtype"], a["normalize"], a["work"], a["nbytes"],
                                 a["peak"], stream)
        return rc, lib.use_last_error().decode()

    cases = [(dict(inp=None), "in is null"), (dict(out=None), "out is null"), (dict(lens=None), "len_host is null"),
             (dict(work=None), "work is null"), (dict(peak=None), "peak_dev is null"), (dict(B=0), "B=0"), (dict(B=-3), "B=-3"),
             (dict(lens=(C.c_int * B)(300, 0)), "len[1]=0"), (dict(lens=(C.c_int * B)(301, 5)), "len[0]=301"),
             (dict(lens=(C.c_int * B)(7, -2)), "len[1]=-2"), (dict(subtype=2), "subtype=2"), (dict(subtype=-1), "subtype=-1"),
             (dict(nbytes=nbytes - 1), f"work_bytes={nbytes - 1}"), (dict(nbytes=0), "work_bytes=0")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == -1 and word in msg and "use_wav_handoff" in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert float(out.min()) == 5.0 and float(peak.min()) == 5.0                    # nothing was launched
    rc, msg = call()
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert float(out[0, 0]) == np.float32(0.8) and float(out[1, 0]) == np.float32(0.8) and not out[1, 1:].any()
    assert peak.tolist() == [8192 / 32768, 8192 / 32768]
    # the wrapper's own checks (those of metrics._run)
    with pytest.raises(TypeError, match="float32"):
        wav_handoff(wav.double(), [300, 1])
    with pytest.raises(ValueError, match="entries"):
        wav_handoff(wav, [300])
    with pytest.raises(ValueError, match="must lie in"):
        wav_handoff(wav, [300, 301])
    with pytest.raises(ValueError, match="subtype"):
        wav_handoff(wav, [300, 1], subtype="PCM_24")
    with pytest.raises(ValueError, match="shape"):
        wav_handoff(wav, [300, 1], out=torch.zeros(2, 299, device="cuda"))


# ---- 2. the pipeline is the two-run flow ----------------------------------------------------------------------------------------
N_FFT, HOP = 1022, 160
_cache = {}


def _stages():
    """One ScoreModel and one generator (and so two engines) for the whole module, bf16 as the shipped configs."""
    if not _cache:
        from universal_speech_enhancement_amd.gan.ncsnpp_wrapper import NCSNPP_Wrapper
        from universal_speech_enhancement_amd.sgmse.model_wrapper import ScoreModel
        score = ScoreModel(backbone="ncsnpplarge", sde="ouve", t_eps=3e-2, condition="noisy", n_fft=N_FFT, hop_length=HOP, num_frames=512,
                           window="hann", sde_input="noisy", predictor="reverse_diffusion", corrector="langevin", precision="bf16")
        score.score_net.load_state_dict({k: torch.from_numpy(v) for k, v in tw.make_state_dict(1234, **tw.LARGE).items()})
        G = NCSNPP_Wrapper(n_fft=N_FFT, hop_length=HOP, num_frames=480, precision="bf16")
        G.net.load_state_dict({k: torch.from_numpy(v) for k, v in tw.make_state_dict(4321, **tw.REFINE).items()}, strict=True)
        _cache["stages"] = (score, G)
    return _cache["stages"]


def _write_noisy(folder, lens, seed=40):
    from universal_speech_enhancement_amd.wavio import FLOAT32, write_wav
    names = ["a.wav", "sub/b.wav", "c.wav"][: len(lens)]
    for i, (name, L) in enumerate(zip(names, lens)):
        os.makedirs(os.path.dirname(str(folder / name)), exist_ok=True)
        w = tnoise.synth_noisy_speech(1, L, seed=seed + i)[0]
        write_wav(str(folder / name), w / np.abs(w).max() * 0.5, 24000, FLOAT32)
    return names


def _one_run_against_two(tmp_path, lens, handoff_subtype, sampler_kwargs):
    """USEModule over the noisy folder into R1 (stage-1 files into S); then GANModule over LoadWavData(S) into R2, with the same batch
    size and the generator keywords the pipeline used.  -> the file names."""
    from universal_speech_enhancement_amd.data import LoadWavData
    from universal_speech_enhancement_amd.LSGAN_module import GANModule
    from universal_speech_enhancement_amd.USE_module import USEModule
    from universal_speech_enhancement_amd.wavio import read_wav
    score, G = _stages()
    noisy, S, R1, R2 = (tmp_path / d for d in ("noisy", "stage1", "one_run", "two_runs"))
    names = _write_noisy(noisy, lens)
    pipe = USEModule(Score=score, G=G, sampler_kwargs=sampler_kwargs, handoff_subtype=handoff_subtype, stage1_folder=str(S))
    for i, batch in enumerate(LoadWavData(str(noisy), str(R1), batch_size=2).predict_batches("cuda", frame_hop=HOP)):
        out = pipe.predict_step(batch, i)
        assert out["fake"].shape == out["enhanced"].shape == batch["perturbed"].shape
        for b, p in enumerate(out["audio_path"]):                                  # the peak the second run's loader finds in the stage-1 file
            x, _ = read_wav(p.replace(str(noisy), str(S)))
            assert float(out["handoff_peak"][b]) == np.abs(x).max(), p
    second = GANModule(G=G, sampler_kwargs=pipe.refine_kwargs)
    for i, batch in enumerate(LoadWavData(str(S), str(R2), batch_size=2).predict_batches("cuda", frame_hop=HOP)):
        second.predict_step(batch, i)
    for name, L in zip(names, lens):
        x, sr = read_wav(str(R1 / name))
        assert sr == 24000 and x.shape == (L,) and np.isfinite(x).all() and np.abs(x).max() > 0, name
        s1, _ = read_wav(str(S / name))
        assert s1.shape == (L,) and np.abs(s1).max() > 0
        assert (R1 / name).read_bytes() == (R2 / name).read_bytes(), (handoff_subtype, name)
    return names


@pytest.mark.parametrize("handoff_subtype", ["PCM_16", "FLOAT"])
def test_one_run_writes_what_the_two_runs_write(tmp_path, handoff_subtype):
    """Three files of 9000, 7300 and 8100 samples (T' = 64), batch_size 2: a batch of two lengths and a batch of one."""
    _one_run_against_two(tmp_path, (9000, 7300, 8100), handoff_subtype, dict(N=2, corrector_steps=1, snr=0.5))


def test_one_run_with_per_item_and_own_length(tmp_path):
    from universal_speech_enhancement_amd.USE_module import shared_refine_kwargs
    kw = dict(N=2, corrector_steps=1, snr=0.5, per_item=True, own_length=True, seed=3)
    assert shared_refine_kwargs(kw) == {"own_length": True}
    _one_run_against_two(tmp_path, (9000, 7300, 8100), "PCM_16", kw)
    assert _stages()[1].last_groups == [(64, 1)]                                   # the generator ran per group too


def test_one_run_chunked_in_both_stages(tmp_path):
    """24 000 samples: 151 frames, T' = 192, four windows of 64 frames with 16 shared, in the sampler and in the generator."""
    from universal_speech_enhancement_amd.chunking import chunk_plan
    assert chunk_plan(192, 64, 16).n == 4
    _one_run_against_two(tmp_path, (24000,), "PCM_16", dict(N=2, corrector_steps=1, snr=0.5, chunk_frames=64, chunk_overlap=16))


def test_predict_model_use_against_the_two_single_stage_runs(tmp_path):
    from universal_speech_enhancement_amd import predict as P
    noisy, E, R1, R2 = (tmp_path / d for d in ("noisy", "enhanced", "one_run", "two_runs"))
    names = _write_noisy(noisy, (9000, 7300, 8100))
    common = ["random_init_seed=7", "data.batch_size=2"]
    sampler = ["model.Score.corrector=langevin", "model.sampler_kwargs.N=2"]
    assert P.predict(P.compose(["model=USE", f"data.data_folder={noisy}", f"data.target_folder={R1}", "model.wav_subtype=FLOAT"]
                               + common + sampler)) == 3
    assert P.predict(P.compose(["model=SGMSE_Large", f"data.data_folder={noisy}", f"data.target_folder={E}"] + common + sampler)) == 3
    assert P.predict(P.compose(["model=LSGAN", f"data.data_folder={E}", f"data.target_folder={R2}", "model.wav_subtype=FLOAT"] + common)) == 3
    for name in names:
        assert (R1 / name).read_bytes() == (R2 / name).read_bytes(), name
        assert (R1 / name).read_bytes() != (E / name).read_bytes()
    with pytest.raises(SystemExit, match="refine_ckpt_path"):
        P.predict(P.compose(["model=USE", f"data.data_folder={noisy}", f"data.target_folder={R1}", "ckpt_path=score.usehip"]))
    # the same weights from two packed weight files
    from universal_speech_enhancement_amd.pack_checkpoint import pack
    blobs = []
    for model, arch in (("SGMSE_Large", tw.LARGE), ("LSGAN", tw.REFINE)):
        blobs.append(str(tmp_path / f"{model}.usehip"))
        pack({k: torch.from_numpy(v) for k, v in tw.make_state_dict(7, **arch).items()}, blobs[-1], model, "bf16")
    R3 = tmp_path / "packed"
    assert P.predict(P.compose(["model=USE", f"data.data_folder={noisy}", f"data.target_folder={R3}", "model.wav_subtype=FLOAT",
                                f"ckpt_path={blobs[0]}", f"refine_ckpt_path={blobs[1]}", "data.batch_size=2"] + sampler)) == 3
    for name in names:
        assert (R3 / name).read_bytes() == (R1 / name).read_bytes(), name


# ---- 3. the C host --------------------------------------------------------------------------------------------------------------
def test_c_host_refine_flag(tmp_path):
    """examples/enhance_wav --refine: the sampler, use_wav_handoff and the generator (use_stft_fwd -> use_forward -> use_istft_back on a
    second handle) in one run, against enhance_wav without the flag followed by the refine steps from Python on ITS output file (the
    loader, then the generator).  As in the C-host tests of test_hip_parity.py / test_hip_chunking.py the two hosts differ in the last
    bit of the Hann window (C: double cos -> float, torch: float32), which a randomly initialised network amplifies; the bounds are
    theirs - there for four evaluations of the large network, here for one of the smaller generator."""
    import subprocess
    from scipy.io import wavfile
    from universal_speech_enhancement_amd import wavio
    from universal_speech_enhancement_amd.gan.ncsnpp_wrapper import NCSNPP_Wrapper
    from universal_speech_enhancement_amd.hip_engine import HipScoreEngine
    from universal_speech_enhancement_amd.pack_checkpoint import pack
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "enhance_wav")
    if not os.path.exists(exe):
        pytest.fail("examples/enhance_wav is not built (run __graft_entry__.build())")
    blob, gblob = str(tmp_path / "large_fp32.usehip"), str(tmp_path / "refine_fp32.usehip")
    src, one, two = str(tmp_path / "in.wav"), str(tmp_path / "stage1.wav"), str(tmp_path / "refined.wav")
    e = HipScoreEngine(precision="fp32"); e.load_state_dict(tw.make_state_dict(1234, **tw.LARGE)); e.save_weight_blob(blob); e.close()
    gsd = tw.make_state_dict(4321, **tw.REFINE)
    pack({k: torch.from_numpy(v) for k, v in gsd.items()}, gblob, "LSGAN", "fp32")
    wavfile.write(src, 24000, (tnoise.synth_noisy_speech(1, 9600, seed=21)[0] * 0.5 * 32767).astype(np.int16))
    r1 = subprocess.run([exe, blob, src, one, "2", "7", "fp32"], capture_output=True, text=True)
    assert r1.returncode == 0 and "refined" not in r1.stdout, r1.stderr + r1.stdout
    r2 = subprocess.run([exe, blob, src, two, "2", "7", "fp32", "--refine", gblob], capture_output=True, text=True)
    assert r2.returncode == 0 and "refined by" in r2.stdout, r2.stderr + r2.stdout
    sr, got = wavfile.read(two)
    assert sr == 24000 and got.dtype == np.int16 and got.shape == (9600,) and np.abs(got).max() > 0
    x, _ = wavio.load_utterance(one, 24000, True)                                  # the second run's loader on the stage-1 file
    G = NCSNPP_Wrapper(n_fft=N_FFT, hop_length=HOP, num_frames=480, precision="fp32")
    G.net.load_state_dict({k: torch.from_numpy(v) for k, v in gsd.items()}, strict=True)
    want = G({"perturbed": torch.from_numpy(x)[None].cuda()})["fake"][0].cpu().numpy()
    want16 = np.clip(np.rint(want.astype(np.float64) * 32767.0), -32768, 32767).astype(np.int16)
    d = np.abs(got.astype(np.int32) - want16.astype(np.int32))
    print(f"C host --refine against the refine steps from Python: max {int(d.max())} LSB, mean {float(d.mean()):.3f} LSB")
    assert d.max() <= 164 and d.mean() < 2.0, (int(d.max()), float(d.mean()))
    assert not np.array_equal(got, wavfile.read(one)[1])
    for flags, word in ((["--refine"], "needs a value"), (["--refine", str(tmp_path / "missing.usehip")], "failed")):
        bad = subprocess.run([exe, blob, src, str(tmp_path / "o.wav")] + flags, capture_output=True, text=True)
        assert bad.returncode != 0 and word in bad.stderr and not os.path.exists(str(tmp_path / "o.wav")), (flags, bad.stderr)
