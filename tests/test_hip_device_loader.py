"""GPU checks of the device-side loader (csrc/use_resample.hip: ``use_resample_fft_dev`` / ``use_load_items_dev``; ``wavio.
resample_fft_device`` / ``load_batch_device``; ``LoadWavData(device_load=True)``; ``predict data.device_load=true``).

The resampler is pinned to ``scipy.signal.resample`` in float64 and to the host ``wavio.resample_fft`` with the project's own bound
for this function (tests/test_io.py): ``atol = 1e-11 * max(1, max|want|)``, ``rtol = 0``.  The loader is pinned to the host
``load_utterance`` at ``atol = 1e-7`` (one float32 ulp at 0.8 is 6e-8) and bit for bit where no resampling happens.

Sizes at which the implementation changes its decomposition (``fft_plan``; a transform of length N runs at M = N when N is a power of
two, else at Bluestein's M = pow2 >= 2 N - 1), each with a case at, just below and just above it in ``THRESHOLD_CASES``:
  M = 2^11 = the LDS piece: one pass in one workgroup up to it, two Stockham passes above.
      N = 2048 (direct, M = 2^11) and N = 1023 (Bluestein, M = 2^11) are at it; N = 1025 (M = 2^12), N = 2047 (M = 2^12), N = 2049
      (M = 2^13) and N = 4096 (direct, M = 2^12) are above; N = 1024 (direct, M = 2^10) is below.
  M = 2^18: two passes (radices 2^9, 2^9) up to it, three above.
      N = 131071 (Bluestein, M = 2^18) and N = 262144 (direct) are at it; N = 131072 (direct, M = 2^17: 2^9, 2^8) is below;
      N = 131073 (M = 2^19: 2^7, 2^6, 2^6) and N = 524288 (direct, M = 2^19) are above.
Every figure is printed before it is asserted (``pytest -s``)."""
import ctypes as C

import numpy as np
import pytest
import torch

from universal_speech_enhancement_amd import _lib, wavio
from universal_speech_enhancement_amd._lib import UseHipError
from universal_speech_enhancement_amd.data import LoadWavData

pytestmark = pytest.mark.gpu

ISSUE_CASES = [(1, 1), (1, 3), (2, 1), (2, 3), (3, 2), (5, 8), (16, 8), (17, 16),
               (255, 256), (256, 255), (256, 128), (257, 129), (1000, 1500),
               (4096, 2048), (4097, 2049),
               (44100, 24000), (48000, 24000), (16000, 24000),
               (65537, 32769), (262145, 131073), (1048577, 524289)]
THRESHOLD_CASES = [(1023, 1024), (1024, 1023), (1025, 2047), (2047, 1025), (2048, 1024), (2049, 2048), (1024, 2048),
                   (131071, 65536), (131072, 131071), (131073, 65537), (65537, 131073), (262144, 131072), (524288, 262144),
                   (262144, 524288)]
CASES = ISSUE_CASES + THRESHOLD_CASES


def _bound(want):
    return 1e-11 * max(1.0, float(np.abs(want).max()))


def _dev_resample(x, num):
    return wavio.resample_fft_device(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda(), num).cpu().numpy()


@pytest.mark.parametrize("n,num", CASES)
def test_resample_fft_dev_equals_scipy_and_the_host(n, num):
    from scipy.signal import resample
    x = np.random.default_rng(1000 * n + num).standard_normal(n)
    got = _dev_resample(x, num)
    want = resample(x, num)
    host = wavio.resample_fft(x, num)
    assert got.shape == want.shape and got.dtype == np.float64
    e_scipy, e_host = float(np.abs(got - want).max()), float(np.abs(got - host).max())
    print(f"n={n} num={num}: |dev - scipy| = {e_scipy:.3e}, |dev - host| = {e_host:.3e}, bound = {_bound(want):.3e}")
    np.testing.assert_allclose(got, want, rtol=0, atol=_bound(want))
    np.testing.assert_allclose(got, host, rtol=0, atol=_bound(want))


def _structured():
    k = np.arange(256)
    out = [("alternating", (-1.0) ** k, [128, 255, 512, 257, 100])]
    out.append(("constant", np.full(100, 0.7), [50, 99, 101, 200, 33]))
    out.append(("constant_odd", np.full(101, -1.3), [50, 99, 102, 202]))
    imp = np.zeros(64); imp[5] = 1.0
    out.append(("impulse", imp, [32, 63, 65, 128, 31]))
    imp2 = np.zeros(63); imp2[0] = 1.0
    out.append(("impulse_odd", imp2, [32, 31, 64, 127]))
    out.append(("cosine_bin3", np.cos(2 * np.pi * 3 * np.arange(96) / 96), [48, 95, 97, 192, 7, 6, 8]))
    out.append(("cosine_bin3_odd", np.cos(2 * np.pi * 3 * np.arange(97) / 97), [48, 49, 96, 194, 7, 6]))
    return out


@pytest.mark.parametrize("name,x,nums", _structured(), ids=[s[0] for s in _structured()])
def test_structured_inputs_follow_the_nyquist_and_hermitian_rules(name, x, nums):
    from scipy.signal import resample
    for num in nums:
        got, want = _dev_resample(x, num), resample(x, num)
        err = float(np.abs(got - want).max())
        print(f"{name} {len(x)} -> {num}: |dev - scipy| = {err:.3e}, bound = {_bound(want):.3e}")
        np.testing.assert_allclose(got, want, rtol=0, atol=_bound(want))


def test_resample_runs_agree_bit_for_bit():
    for n, num in [(48000, 24000), (4097, 2049), (256, 512), (131073, 65537)]:
        x = torch.from_numpy(np.random.default_rng(n).standard_normal(n)).cuda()
        a = wavio.resample_fft_device(x, num)
        wavio.resample_fft_device(torch.flip(x, [0]), num + 1)          # something else through the same workspace in between
        b = wavio.resample_fft_device(x, num)
        assert torch.equal(a, b), (n, num)
    same = wavio.resample_fft_device(x, x.shape[0])
    assert torch.equal(same, x) and same.data_ptr() != x.data_ptr()     # num == n: a copy


# ---- files ----
def _pcm(rng, frames, ch=1):
    return (rng.standard_normal((frames, ch) if ch > 1 else frames) * 0.2).clip(-0.99, 0.99).astype(np.float32)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """name -> path.  Mono 16-bit at 48 / 44.1 / 16 / 8 / 24 kHz, a stereo file, a FLOAT file, 147 k frames at 44.1 kHz (the ratio-first
    length rule gives one sample more than ceil(len * 24000 / 44100)), and a silent file; 0.05 ... 1 s."""
    d = tmp_path_factory.mktemp("loader_corpus")
    rng = np.random.default_rng(7)
    spec = {"m48000": (48000, 48000, 1, wavio.PCM16), "m44100": (44100, 22050, 1, wavio.PCM16), "m16000": (16000, 4801, 1, wavio.PCM16),
            "m8000": (8000, 400, 1, wavio.PCM16), "m24000": (24000, 5000, 1, wavio.PCM16), "stereo": (48000, 4800, 2, wavio.PCM16),
            "float": (44100, 11025, 1, wavio.FLOAT32), "r147": (44100, 147 * 37, 1, wavio.PCM16)}
    paths = {}
    for name, (rate, frames, ch, sub) in spec.items():
        paths[name] = str(d / f"{name}.wav")
        wavio.write_wav(paths[name], _pcm(rng, frames, ch), rate, sub)
    paths["silent"] = str(d / "silent.wav")
    wavio.write_wav(paths["silent"], np.zeros(3000, np.float32), 48000)
    assert wavio.resampled_length(147 * 37, 44100, 24000) == -(-147 * 37 * 24000 // 44100) + 1
    return paths


NAMES = ["m48000", "m44100", "m16000", "m8000", "m24000", "stereo", "float", "r147"]


@pytest.fixture(scope="module")
def host_rows(corpus):
    """(name, normalize, sampling_rate) -> (float32 row, rate) of the host loader, computed once."""
    return {(k, norm, sr): wavio.load_utterance(p, sr, norm) for k, p in corpus.items() for norm in (True, False) for sr in (24000, 0)}


def _check_batch(wav, lens, rates, names, host_rows, norm, sr=24000):
    assert wav.dtype == torch.float32 and wav.is_cuda and lens.dtype == np.int32
    got = wav.cpu().numpy()
    assert got.shape == (len(names), max(len(host_rows[(k, norm, sr)][0]) for k in names))
    for b, k in enumerate(names):
        want, rate = host_rows[(k, norm, sr)]
        assert lens[b] == len(want) and rates[b] == rate, k
        err = float(np.abs(got[b, : lens[b]] - want).max())
        print(f"{k} normalize={norm} sampling_rate={sr}: L = {lens[b]}, |dev - host| = {err:.3e}")
        np.testing.assert_allclose(got[b, : lens[b]], want, rtol=0, atol=1e-7)
        assert not got[b, lens[b]:].any() and not np.signbit(got[b, lens[b]:]).any(), k       # the padding: exact zeros
        if sr == 0 or k == "m24000":                                                          # an unchanged rate: the host loader's bits
            assert np.array_equal(got[b, : lens[b]].view(np.uint32), want.view(np.uint32)), k


@pytest.mark.parametrize("norm", [True, False])
def test_load_batch_device_is_the_host_loader(corpus, host_rows, norm):
    paths = [corpus[k] for k in NAMES]
    wav, lens, rates = wavio.load_batch_device(paths, 24000, norm, "cuda")
    _check_batch(wav, lens, rates, NAMES, host_rows, norm)
    wav, lens, rates = wavio.load_batch_device(paths, 0, norm, "cuda")                        # sampling_rate=None: every rate unchanged
    _check_batch(wav, lens, rates, NAMES, host_rows, norm, sr=0)


def test_silent_file_gives_what_the_host_gives(corpus, host_rows):
    want, rate = host_rows[("silent", True, 24000)]
    assert np.isnan(want).all()
    wav, lens, rates = wavio.load_batch_device([corpus["m8000"], corpus["silent"]], 24000, True, "cuda")
    got = wav.cpu().numpy()
    assert lens[1] == len(want) and rates[1] == rate and np.isnan(got[1, : lens[1]]).all()
    assert np.isfinite(got[0]).all()
    quiet, _ = host_rows[("silent", False, 24000)]
    wav, lens, _ = wavio.load_batch_device([corpus["silent"]], 24000, False, "cuda")
    np.testing.assert_allclose(wav.cpu().numpy()[0], quiet, rtol=0, atol=1e-7)


def test_a_row_does_not_depend_on_its_batch(corpus):
    alone, lens, _ = wavio.load_batch_device([corpus["m44100"]], 24000, True, "cuda")
    L = int(lens[0])
    others = [corpus[k] for k in ("m48000", "m8000", "float", "m24000")]
    for pos in range(3):
        paths = others[:pos] + [corpus["m44100"]] + others[pos:pos + 2]
        wav, lens, _ = wavio.load_batch_device(paths, 24000, True, "cuda")
        assert int(lens[pos]) == L and torch.equal(wav[pos, :L], alone[0]), pos
        assert not wav[pos, L:].any()
    again, _, _ = wavio.load_batch_device([corpus["m44100"]], 24000, True, "cuda")
    assert torch.equal(again, alone)


def test_device_load_max_samples_sends_long_files_to_the_host(corpus, host_rows):
    names = ["m16000", "m48000", "m24000", "m44100"]                      # 48000 frames > 30000: the host path for row 1 alone
    wav, lens, rates = wavio.load_batch_device([corpus[k] for k in names], 24000, True, "cuda", max_samples=30000)
    _check_batch(wav, lens, rates, names, host_rows, True)
    want, _ = host_rows[("m48000", True, 24000)]
    assert np.array_equal(wav.cpu().numpy()[1, : lens[1]].view(np.uint32), want.view(np.uint32))
    ref, _, _ = wavio.load_batch_device([corpus[k] for k in names], 24000, True, "cuda")
    for b in (0, 2, 3):                                                   # the device rows: as without the limit
        assert torch.equal(wav[b], ref[b])


def test_errors_are_reported_and_nothing_is_written():
    L = _lib.lib()
    n, num = 3000, 1500
    x = torch.from_numpy(np.random.default_rng(0).standard_normal(n)).cuda()
    need = L.use_resample_workspace(n, num)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    wav = torch.full((2, 2000), 7.0, dtype=torch.float32, device="cuda")
    y = torch.full((num,), 7.0, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ptrs = (C.c_void_p * 2)(x.data_ptr(), x.data_ptr())

    def items(ns, nums, stride=2000, work_bytes=need):
        return L.use_load_items_dev(ptrs, (C.c_int64 * 2)(*ns), (C.c_int64 * 2)(*nums), 2, 1, wav.data_ptr(), stride, work.data_ptr(),
                                    work_bytes, stream)

    def one(n_, num_, work_bytes=need):
        return L.use_resample_fft_dev(x.data_ptr(), n_, num_, y.data_ptr(), work.data_ptr(), work_bytes, stream)

    for what, call, word in [("short workspace", lambda: items([n, n], [num, num], work_bytes=need - 1), b"work_bytes"),
                             ("n = 0", lambda: items([n, 0], [num, num]), b"positive"),
                             ("num = 0", lambda: items([n, n], [num, 0]), b"positive"),
                             ("stride < num", lambda: items([n, n], [num, num], stride=num - 1), b"stride"),
                             ("max(n, num) > 2^24", lambda: items([n, n], [num, 2 ** 24 + 1], stride=2 ** 24 + 1), b"2^24"),
                             ("short workspace (one)", lambda: one(n, num, need - 1), b"work_bytes"),
                             ("n = 0 (one)", lambda: one(0, num), b"positive"),
                             ("max(n, num) > 2^24 (one)", lambda: one(2 ** 24 + 1, num), b"2^24"),
                             ("null x (one)", lambda: L.use_resample_fft_dev(None, n, num, y.data_ptr(), work.data_ptr(), need, stream),
                              b"null")]:
        rc, msg = call(), L.use_last_error()
        print(what, rc, msg)
        assert rc == -1 and word in msg, (what, rc, msg)                  # USE_E_INVALID
    torch.cuda.synchronize()
    assert bool((wav == 7.0).all()) and bool((y == 7.0).all())
    assert items([n, n], [num, num]) == 0 and one(n, num) == 0            # the same arguments, valid: it runs
    torch.cuda.synchronize()
    assert torch.equal(wav[0], wav[1]) and not bool((wav[:, :num] == 7.0).any()) and not wav[:, num:].any()
    with pytest.raises(UseHipError):
        wavio.resample_fft_device(torch.zeros(4, dtype=torch.float64), 2)                     # a CPU tensor
    with pytest.raises(TypeError):
        wavio.resample_fft_device(torch.zeros(4, dtype=torch.float32, device="cuda"), 2)
    with pytest.raises(ValueError):
        wavio.load_batch_device([], 24000, True, "cpu")


# ---- LoadWavData and predict ----
@pytest.fixture(scope="module")
def folder(tmp_path_factory, corpus):
    """Five files of mixed rates and lengths under one folder (one in a sub-folder)."""
    d = tmp_path_factory.mktemp("loader_folder")
    (d / "sub").mkdir()
    for i, k in enumerate(["m48000", "m44100", "m16000", "m24000", "float"]):
        a, sr = wavio.read_wav(corpus[k])
        wavio.write_wav(str(d / ("sub" if i == 2 else "") / f"f{i}_{k}.wav"), a.astype(np.float32), sr)
    return str(d)


@pytest.mark.parametrize("bucket", [False, True])
def test_predict_batches_match_the_host_loader(folder, tmp_path, bucket):
    kw = dict(data_folder=folder, target_folder=str(tmp_path), batch_size=2, bucket_by_length=bucket)
    host = list(LoadWavData(**kw).predict_batches("cuda", frame_hop=160))
    dev = list(LoadWavData(device_load=True, **kw).predict_batches("cuda", frame_hop=160))
    assert len(host) == len(dev) and sum(len(b["name"]) for b in dev) == 5
    for h, d in zip(host, dev):
        assert list(h) == list(d)
        for k in ("name", "sampling_rate", "audio_path", "data_folder", "target_folder"):
            assert h[k] == d[k], k
        assert d["sample_length"].dtype == h["sample_length"].dtype and torch.equal(d["sample_length"], h["sample_length"])
        assert d["perturbed"].shape == h["perturbed"].shape and d["perturbed"].dtype == h["perturbed"].dtype
        assert d["perturbed"].device == h["perturbed"].device
        err = float((d["perturbed"] - h["perturbed"]).abs().max())
        print(f"bucket={bucket} {h['name']}: |dev - host| = {err:.3e}")
        assert err <= 1e-7


def test_predict_with_device_load_writes_the_files(tmp_path):
    from universal_speech_enhancement_amd import predict as P
    from universal_speech_enhancement_amd.testing import noise as tnoise
    src, dst = tmp_path / "noisy", tmp_path / "enhanced"
    src.mkdir()
    for i in range(3):
        wavio.write_wav(str(src / f"u{i}.wav"), tnoise.synth_noisy_speech(1, 14400, seed=40 + i)[0].astype(np.float32), 48000)
    n = P.predict(P.compose(["model=SGMSE_Large", f"data.data_folder={src}", f"data.target_folder={dst}", "random_init_seed=1",
                             "model.sampler_kwargs.N=1", "data.batch_size=2", "data.device_load=true"]))
    assert n == 3
    for i in range(3):
        assert wavio.wav_info(str(dst / f"u{i}.wav")) == (7200, 1, 24000)
