"""GPU checks of ``data.channels=all``: the device loader of files of several channels (``use_load_files_dev``), the writer
(``use_store_files_dev``) and the hand-off (``use_wav_handoff_files``) against tests/multichannel_ref.py and against the per-row entry
points they extend, and the whole path - loader, sampler, writer, the two-stage pipeline - on random LARGE / REFINE weights.

The bounds are the project's: a row at an unchanged rate is bit-equal to the reference, a resampled row within the device loader's
1e-7 absolute (tests/test_hip_device_loader.py: one float32 ulp at 0.8 is 6e-8); the writer is held to tests/store_ref.py and, bit for
bit, to ``use_store_items_dev``; the hand-off is bit for bit.  Every figure is printed before it is asserted (``pytest -s``)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import multichannel_ref as mr
import store_ref as sr
from universal_speech_enhancement_amd import _lib, wavio
from universal_speech_enhancement_amd.testing import noise as tnoise
from universal_speech_enhancement_amd.testing import weights as tw

pytestmark = pytest.mark.gpu

CHANNELS = [2, 1, 8, 3]                                       # the files of one call, in this mixed order
POISON = 77


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- the loader -------------------------------------------------------------------------------------------------------------------
def _files(n, seed, chans=CHANNELS):
    """Decoded files ``[n, C]`` (float64) whose channels lie at very different levels; the peak of a file is never in channel 0 of a
    file of several channels."""
    rng = np.random.default_rng(seed)
    out = []
    for c in chans:
        level = np.array([0.03, 0.3, 0.1, 0.2, 0.05, 0.15, 0.25, 0.01][:c]) if c > 1 else np.array([0.2])
        out.append(rng.standard_normal((n, c)) * level)
    return out


def _load_files(files, nums, normalize=True, stride=None):
    """``use_load_files_dev`` on decoded files -> host ``[rows, stride]``; ``wav`` is poisoned before the call."""
    L = _lib.lib()
    F = len(files)
    ns, chs = [f.shape[0] for f in files], [f.shape[1] for f in files]
    stride = stride or max(nums)
    xs = [torch.from_numpy(np.ascontiguousarray(f).reshape(-1)).cuda() for f in files]
    wav = torch.full((sum(chs), stride), float(POISON), dtype=torch.float32, device="cuda")
    need = max(L.use_load_files_workspace(n, num, c) for n, num, c in zip(ns, nums, chs))
    assert need > 0
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc = L.use_load_files_dev((C.c_void_p * F)(*[x.data_ptr() for x in xs]), (C.c_int64 * F)(*ns), (C.c_int64 * F)(*nums), (C.c_int * F)(*chs),
                              F, int(normalize), wav.data_ptr(), stride, work.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.use_last_error()
    return wav.cpu().numpy()


def _load_items(signals, nums, normalize=True, stride=None):
    L = _lib.lib()
    B = len(signals)
    stride = stride or max(nums)
    xs = [torch.from_numpy(np.ascontiguousarray(s)).cuda() for s in signals]
    wav = torch.full((B, stride), float(POISON), dtype=torch.float32, device="cuda")
    need = max(L.use_resample_workspace(len(s), num) for s, num in zip(signals, nums))
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc = L.use_load_items_dev((C.c_void_p * B)(*[x.data_ptr() for x in xs]), (C.c_int64 * B)(*[len(s) for s in signals]),
                              (C.c_int64 * B)(*nums), B, int(normalize), wav.data_ptr(), stride, work.data_ptr(), need,
                              torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.use_last_error()
    return wav.cpu().numpy()


@pytest.mark.parametrize("rate", [24000, 48000, 44100])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4800])
def test_load_files_dev_follows_the_reference(n, rate):
    """Files of 2, 1, 8 and 3 channels through ONE call: 24 kHz is an unchanged rate, 48 kHz halves (powers of two for n = 256), 44.1 kHz
    goes through Bluestein.  The stride is wider than the longest row."""
    num = wavio.resampled_length(n, rate, 24000)
    files = _files(n, 1000 * n + rate)
    files[3][:, 1] = 0.0                                          # a silent channel of a file that is not silent
    got = _load_files(files, [num] * 4, stride=num + 37)
    row = 0
    for f, c in zip(files, CHANNELS):
        want = mr.load_file(f, num)
        rows = got[row: row + c]
        err = float(np.abs(rows[:, :num].astype(np.float64) - want).max())
        print(f"n={n} {rate} -> 24000 (num={num}) C={c}: max |dev - ref| = {err:.3e}")
        if num == n:
            assert np.array_equal(_bits(rows[:, :num]), _bits(want)), (n, rate, c)
        else:
            assert err <= 1e-7, (n, rate, c, err)
        assert not rows[:, num:].any() and not np.signbit(rows[:, num:]).any()                    # the padding: exact zeros
        assert np.abs(rows).max() == np.float32(0.8)                                             # one gain per file ...
        if c > 1 and n > 1:
            assert np.abs(rows[0]).max() < 0.8                                                   # ... and not one per channel
        if c == 1:                                                                               # the loader of mono items, bit for bit
            item = _load_items([f[:, 0]], [num], stride=num + 5)
            assert np.array_equal(_bits(rows[0, :num]), _bits(item[0, :num]))
        # alone, at another stride: the same bits
        alone = _load_files([f], [num])
        assert alone.shape == (c, num) and np.array_equal(_bits(alone), _bits(rows[:, :num])), (n, rate, c)
        row += c
    assert not got[row - 3 + 1].any()                                                            # the silent channel: zeros
    plain = _load_files(files[:2], [num] * 2, normalize=False)
    want = np.concatenate([mr.load_file(f, num, False) for f in files[:2]])
    np.testing.assert_allclose(plain, want, rtol=0, atol=1e-7)
    if num == n:
        assert np.array_equal(_bits(plain), _bits(want))


@pytest.mark.parametrize("n,num", [(256, 256), (4800, 2400), (441, 240)])
def test_a_silent_file_gives_nan_and_runs_agree(n, num):
    files = [np.zeros((n, 2)), _files(n, 5, [3])[0]]
    a = _load_files(files, [num, num], stride=num + 3)
    assert np.isnan(a[:2, :num]).all() and not a[:2, num:].any()                                 # as a silent mono file
    assert np.isfinite(a[2:]).all() and np.abs(a[2:]).max() == np.float32(0.8)
    b = _load_files(files[::-1], [num, num], stride=num + 11)                                    # another order, another stride
    assert np.array_equal(_bits(b[:3, :num]), _bits(a[2:, :num])) and np.isnan(b[3:, :num]).all()
    quiet = _load_files(files, [num, num], normalize=False)
    assert not quiet[:2].any()


def test_load_batch_device_with_all_channels(tmp_path):
    """``wavio.load_batch_device(channels="all")`` and ``LoadWavData(device_load=True, channels="all")`` against the host loader of
    the same option: the same keys, lengths and rates; rows at an unchanged rate bit for bit, the others within 1e-7."""
    from universal_speech_enhancement_amd.data import LoadWavData
    src = tmp_path / "noisy"
    src.mkdir()
    rng = np.random.default_rng(11)
    spec = [("a.wav", 48000, 4800, 2), ("b.wav", 24000, 3000, 3), ("c.wav", 44100, 2205, 1), ("d.wav", 16000, 1601, 2)]
    for name, rate, frames, c in spec:
        a = (rng.standard_normal((frames, c) if c > 1 else frames) * 0.2 * np.array([1.0, 0.3, 0.1][:c])).clip(-0.99, 0.99).astype(np.float32)
        wavio.write_wav(str(src / name), a, rate)
    paths = [str(src / s[0]) for s in spec]
    wav, lens, rates, chans = wavio.load_batch_device(paths, 24000, True, "cuda", channels="all")
    assert chans == [2, 3, 1, 2] and wav.shape == (8, 3000) and lens.dtype == np.int32 and rates == [24000] * 8
    got = wav.cpu().numpy()
    row = 0
    for p, (name, rate, frames, c) in zip(paths, spec):
        want, _ = wavio.load_file_channels(p, 24000, True)
        assert lens[row: row + c].tolist() == [want.shape[1]] * c
        err = float(np.abs(got[row: row + c, : want.shape[1]] - want).max())
        print(f"{name}: |dev - host| = {err:.3e}")
        assert err <= 1e-7 and not got[row: row + c, want.shape[1]:].any()
        if rate == 24000:
            assert np.array_equal(_bits(got[row: row + c, : want.shape[1]]), _bits(want))
        row += c
    # files beyond max_samples (frames x channels) take the host path: a.wav (9600) and b.wav (9000) here
    mixed, _, _, _ = wavio.load_batch_device(paths, 24000, True, "cuda", max_samples=5000, channels="all")
    m = mixed.cpu().numpy()
    for r0, c, p in ((0, 2, paths[0]), (2, 3, paths[1])):
        want, _ = wavio.load_file_channels(p, 24000, True)
        assert np.array_equal(_bits(m[r0: r0 + c, : want.shape[1]]), _bits(want)) and not m[r0: r0 + c, want.shape[1]:].any()
    assert np.array_equal(_bits(m[5:]), _bits(got[5:]))
    kw = dict(data_folder=str(src), target_folder=str(tmp_path / "o"), batch_size=4, channels="all")
    host = list(LoadWavData(**kw).predict_batches("cuda", frame_hop=160))
    dev = list(LoadWavData(device_load=True, **kw).predict_batches("cuda", frame_hop=160))
    assert [b["file_rows"] for b in dev] == [[(0, 2)], [(0, 3), (3, 1)], [(0, 2)]]
    for h, d in zip(host, dev):
        assert list(h) == list(d)
        for k in h:
            if k == "perturbed":
                assert d[k].shape == h[k].shape and d[k].dtype == h[k].dtype and d[k].device == h[k].device
                assert float((d[k] - h[k]).abs().max()) <= 1e-7
            elif k == "sample_length":
                assert d[k].dtype == h[k].dtype and torch.equal(d[k], h[k])
            else:
                assert d[k] == h[k], k


# ---- the writer -------------------------------------------------------------------------------------------------------------------
DTYPES = {wavio.PCM16: torch.int16, wavio.FLOAT32: torch.float32}


def _store_rows(rows, stride):
    wav = np.full((len(rows), stride), np.nan, np.float32)        # the padding of a row is never read
    for b, r in enumerate(rows):
        wav[b, : len(r)] = r
    return torch.from_numpy(wav).cuda()


@pytest.mark.parametrize("subtype", [wavio.PCM16, wavio.FLOAT32])
@pytest.mark.parametrize("n,num", [(2400, 2400), (2400, 4410), (257, 257), (255, 512)])
def test_store_files_dev_interleaves_the_rows_of_store_items_dev(n, num, subtype):
    L = _lib.lib()
    chans = [2, 1, 8, 3]
    rng = np.random.default_rng(100 * n + num)
    rows = [(rng.standard_normal(n) * 0.3).astype(np.float32) for _ in range(sum(chans))]
    if n == num:
        rows[2][5] = np.nan                                       # the mono file: a NaN is stored as code 0 (a float keeps its bits)
    wav = _store_rows(rows, n + 13)
    stream = torch.cuda.current_stream().cuda_stream
    need = L.use_store_workspace(n, num)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    B, F = len(rows), len(chans)
    items = torch.full((B, num), POISON, dtype=DTYPES[subtype], device="cuda")
    assert L.use_store_items_dev(wav.data_ptr(), n + 13, (C.c_int * B)(*[n] * B), (C.c_int64 * B)(*[num] * B), B, subtype, items.data_ptr(),
                                 num, work.data_ptr(), need, stream) == 0, L.use_last_error()
    items = items.cpu().numpy()
    offs = np.concatenate([[0], np.cumsum([num * c for c in chans])])          # the files lie one after another, no gap
    out = torch.full((int(offs[-1]) + 64,), POISON, dtype=DTYPES[subtype], device="cuda")
    assert L.use_store_files_dev(wav.data_ptr(), n + 13, (C.c_int * F)(*[n] * F), (C.c_int64 * F)(*[num] * F), (C.c_int * F)(*chans),
                                 (C.c_int64 * F)(*offs[:-1].tolist()), F, subtype, out.data_ptr(), work.data_ptr(), need, stream) == 0, \
        L.use_last_error()
    got = out.cpu().numpy()
    assert (got[offs[-1]:] == POISON).all()                                                       # the guard words are untouched
    row = 0
    for f, c in enumerate(chans):
        block = got[offs[f]: offs[f + 1]].reshape(num, c)
        assert np.array_equal(_bits(block), _bits(mr.interleave(items[row: row + c]))), (n, num, subtype, c)
        for k in range(c):
            x = rows[row + k]
            if np.isnan(x).any():
                continue
            want64 = sr.oracle(x, num)
            if subtype == wavio.FLOAT32:
                sr.check_float32(np.ascontiguousarray(block[:, k]), want64, f"{n} -> {num} C={c} channel {k}")
            else:
                sr.check_codes(np.ascontiguousarray(block[:, k]), want64, f"{n} -> {num} C={c} channel {k}")
        row += c
    if n == num and subtype == wavio.PCM16:
        assert got[offs[1] + 5] == 0                                                              # the mono file's NaN
    # wavio.store_batch_device(channels=...): the same files, one call and one copy
    files = wavio.store_batch_device(wav, [n] * F, [num] * F, subtype, channels=chans)
    assert [a.shape for a in files] == [(num, c) for c in chans]
    assert np.array_equal(_bits(np.concatenate([a.reshape(-1) for a in files])), _bits(got[: offs[-1]]))
    host = wavio.store_batch_device(wav, [n] * F, [num] * F, subtype, max_samples=max(n, num) - 1, channels=chans)   # every file on the host
    for a, h in zip(files, host):
        assert a.shape == h.shape and a.dtype == h.dtype


def test_store_files_dev_with_files_of_different_shapes():
    """Three files of different lengths and targets through one call and through ``wavio``, a file alone gives the same bits."""
    shapes = [(2400, 4410, 2), (256, 512, 3), (1000, 1000, 2)]
    rng = np.random.default_rng(9)
    rows = [(rng.standard_normal(n) * 0.3).astype(np.float32) for n, _, c in shapes for _ in range(c)]
    wav = _store_rows(rows, 2500)
    for subtype in (wavio.FLOAT32, wavio.PCM16):
        files = wavio.store_batch_device(wav, [s[0] for s in shapes], [s[1] for s in shapes], subtype, channels=[s[2] for s in shapes])
        row = 0
        for a, (n, num, c) in zip(files, shapes):
            assert a.shape == (num, c)
            items = wavio.store_batch_device(wav[row: row + c], [n] * c, [num] * c, subtype)
            assert np.array_equal(_bits(a), _bits(mr.interleave(items[:, :num])))
            alone = wavio.store_batch_device(wav[row: row + c].clone(), [n], [num], subtype, channels=[c])[0]
            assert np.array_equal(_bits(a), _bits(alone))
            row += c


# ---- the hand-off -----------------------------------------------------------------------------------------------------------------
def _same(got: torch.Tensor, want: np.ndarray) -> bool:
    got, want = got.cpu(), torch.from_numpy(np.ascontiguousarray(want))
    return (got.shape == want.shape and got.dtype == want.dtype and torch.equal(torch.isnan(got), torch.isnan(want))
            and torch.equal(torch.nan_to_num(got, nan=7.0), torch.nan_to_num(want, nan=7.0)))


def _handoff_batch():
    """Files of 2, 1, 8 and 3 rows with lengths (4099, 4097, 65, 20000), stride 20001 (odd); the padding holds 1e9.  The peak of file 0
    lies in its second row, beyond full scale and negative; file 3 spans two slices, its peak at the end of its last row, and its
    middle row is silent; exact .5 ties of the quantiser in file 2."""
    rng = np.random.default_rng(77)
    chans, lens, stride = [2, 1, 8, 3], [4099, 4097, 65, 20000], 20001
    wav = np.full((sum(chans), stride), 1e9, np.float32)
    row = 0
    for c, L in zip(chans, lens):
        for k in range(c):
            wav[row + k, :L] = (rng.standard_normal(L) * (0.05, 0.3, 0.1, 0.2, 0.02, 0.15, 0.25, 0.01)[k]).astype(np.float32)
        row += c
    wav[1, 1234] = -3.25
    wav[5, 10:14] = np.array([0.5, -0.5, 1.5, -1.5], np.float32)
    wav[12, :20000] = 0.0
    wav[13, 19999] = 0.97
    return wav, chans, lens


@pytest.mark.parametrize("subtype,normalize", [("PCM_16", True), ("PCM_16", False), ("FLOAT", True), ("FLOAT", False)])
def test_handoff_files_equals_the_reference_bit_for_bit(subtype, normalize):
    from universal_speech_enhancement_amd.handoff import wav_handoff, wav_handoff_files
    wav, chans, lens = _handoff_batch()
    src = torch.from_numpy(wav).cuda()
    out, peaks = wav_handoff_files(src, lens, chans, subtype, normalize)
    assert out is not src and torch.equal(src.cpu(), torch.from_numpy(wav)) and peaks.shape == (4,) and peaks.dtype == torch.float64
    row = 0
    for f, (c, L) in enumerate(zip(chans, lens)):
        want, mx = mr.handoff_file(wav[row: row + c, :L], subtype, normalize)
        assert _same(out[row: row + c, :L], want), (subtype, normalize, f)
        assert float(peaks[f]) == mx, (f, float(peaks[f]), mx)
        assert not out[row: row + c, L:].any()                                                   # 1e9 of the padding neither read nor kept
        row += c
    if normalize:
        # file 0: one gain for both rows (row 0 alone would peak at 0.8; -3.25 is clamped to full scale in a 16-bit file)
        assert float(out[1, 1234]) == -np.float32(0.8) and float(out[0].abs().max()) < 0.25
        assert not out[12].any() and float(out[13, 19999]) == np.float32(0.8)                    # file 3: the silent row stays zeros
    # in place, and a file alone at another stride
    same, peaks2 = wav_handoff_files(src, lens, chans, subtype, normalize, out=src)
    assert same is src and torch.equal(torch.nan_to_num(src, nan=7.0), torch.nan_to_num(out, nan=7.0)) and torch.equal(peaks2, peaks)
    solo = torch.full((8, 100), 1e9, device="cuda")
    solo[:, :65] = torch.from_numpy(wav[3:11, :65]).cuda()
    o1, p1 = wav_handoff_files(solo, [65], [8], subtype, normalize)
    assert torch.equal(o1[:, :65], out[3:11, :65]) and not o1[:, 65:].any() and float(p1[0]) == float(peaks[2])
    # F = 1, C = 1: use_wav_handoff, bit for bit
    one = torch.from_numpy(wav[2:3]).cuda()
    a, pa = wav_handoff_files(one, [4097], [1], subtype, normalize)
    b, pb = wav_handoff(one, [4097], subtype, normalize)
    assert torch.equal(a, b) and torch.equal(pa, pb) and torch.equal(a[0, :4097], out[2, :4097])
    # rows that are files of their own: use_wav_handoff on the batch
    c_, pc = wav_handoff_files(torch.from_numpy(wav[:3]).cuda(), [4099, 4099, 4097], [1, 1, 1], subtype, normalize)
    d_, pd = wav_handoff(torch.from_numpy(wav[:3]).cuda(), [4099, 4099, 4097], subtype, normalize)
    assert torch.equal(c_, d_) and torch.equal(pc, pd)


@pytest.mark.parametrize("subtype", ["PCM_16", "FLOAT"])
def test_a_silent_file_is_nan_after_the_handoff(subtype):
    from universal_speech_enhancement_amd.handoff import wav_handoff_files
    wav, chans, lens = _handoff_batch()
    wav[3:11, :65] = 0.0
    wav[4, 3] = 1e-6 if subtype == "PCM_16" else 0.0              # below half an LSB: silent once it is a 16-bit file
    out, peaks = wav_handoff_files(torch.from_numpy(wav).cuda(), lens, chans, subtype, True)
    want, mx = mr.handoff_file(wav[3:11, :65], subtype, True)
    assert mx == 0.0 and np.isnan(want).all() and float(peaks[2]) == 0.0
    assert torch.isnan(out[3:11, :65]).all() and not out[3:11, 65:].any() and torch.isfinite(out[:3]).all() and torch.isfinite(out[11:]).all()
    with pytest.raises(ValueError, match="channels"):
        wav_handoff_files(torch.from_numpy(wav).cuda(), lens, [2, 1, 8, 2], subtype)
    with pytest.raises(ValueError, match="entries"):
        wav_handoff_files(torch.from_numpy(wav).cuda(), lens[:3], chans, subtype)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
N_FFT, HOP = 1022, 160
SAMPLER = dict(N=2, corrector_steps=1, snr=0.5, per_item=True, seed=0)
_cache = {}


def _stages(precision):
    """One ScoreModel and one generator per precision for the whole module (random LARGE / REFINE weights, Langevin corrector)."""
    if precision not in _cache:
        from universal_speech_enhancement_amd.gan.ncsnpp_wrapper import NCSNPP_Wrapper
        from universal_speech_enhancement_amd.sgmse.model_wrapper import ScoreModel
        score = ScoreModel(backbone="ncsnpplarge", sde="ouve", t_eps=3e-2, condition="noisy", n_fft=N_FFT, hop_length=HOP, num_frames=512,
                           window="hann", sde_input="noisy", predictor="reverse_diffusion", corrector="langevin", precision=precision)
        score.score_net.load_state_dict({k: torch.from_numpy(v) for k, v in tw.make_state_dict(1234, **tw.LARGE).items()})
        G = NCSNPP_Wrapper(n_fft=N_FFT, hop_length=HOP, num_frames=480, precision=precision)
        G.net.load_state_dict({k: torch.from_numpy(v) for k, v in tw.make_state_dict(4321, **tw.REFINE).items()}, strict=True)
        _cache[precision] = (score, G)
    return _cache[precision]


def _speech(L, seed):
    w = tnoise.synth_noisy_speech(1, L, seed=seed)[0]
    return (w / np.abs(w).max() * 0.5).astype(np.float32)


def _enhance(module, src, dst, channels="all", batch_size=4, **data_kw):
    """``predict``'s loop over one folder; -> the batches ``predict_step`` returned."""
    from universal_speech_enhancement_amd.data import LoadWavData
    out = []
    for i, batch in enumerate(LoadWavData(str(src), str(dst), batch_size=batch_size, channels=channels, **data_kw).predict_batches("cuda", frame_hop=HOP)):
        out.append(module.predict_step(batch, i))
    return out


def _samples(path):
    """The sample bytes of a canonical WAV file (44-byte header) and its header triple."""
    return wavio.wav_info(str(path)), open(str(path), "rb").read()[44:]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_equal_channels_come_out_equal_and_swapped_channels_swapped(tmp_path, precision):
    """(a) a dual-mono file: its two output channels are bit-identical, and bit-identical to the output of the mono file at the same
    relative path; (b) a stereo file with its channels swapped gives the swapped output; (c) a mono file under ``channels="all"`` gives
    the bytes ``channels="first"`` gives.  9000 samples at 24 kHz: 57 frames, T' = 64.  Float files: they carry every bit."""
    from universal_speech_enhancement_amd.SGMSE_module import SGMSEModule
    module = SGMSEModule(Score=_stages(precision)[0], sampler_kwargs=SAMPLER, wav_subtype="FLOAT")
    left, right = _speech(9000, 81), _speech(9000, 82) * np.float32(0.5)
    folders = {k: tmp_path / k for k in ("dual", "mono", "lr", "rl")}
    for d in folders.values():
        (d / "sub").mkdir(parents=True)
    wavio.write_wav(str(folders["dual"] / "sub" / "x.wav"), np.stack([left, left], axis=1), 24000, wavio.FLOAT32)
    wavio.write_wav(str(folders["mono"] / "sub" / "x.wav"), left, 24000, wavio.FLOAT32)
    wavio.write_wav(str(folders["lr"] / "sub" / "x.wav"), np.stack([left, right], axis=1), 24000, wavio.FLOAT32)
    wavio.write_wav(str(folders["rl"] / "sub" / "x.wav"), np.stack([right, left], axis=1), 24000, wavio.FLOAT32)
    out = {k: tmp_path / f"out_{k}" for k in folders}
    for k in folders:
        batches = _enhance(module, folders[k], out[k])
        assert len(batches) == 1 and batches[0]["file_rows"] == [(0, 1 if k == "mono" else 2)]
    _enhance(module, folders["mono"], tmp_path / "out_first", channels="first")
    info, dual = _samples(out["dual"] / "sub" / "x.wav")
    assert info == (9000, 2, 24000)
    dual = np.frombuffer(dual, np.float32).reshape(9000, 2)
    info, mono = _samples(out["mono"] / "sub" / "x.wav")
    assert info == (9000, 1, 24000)
    mono = np.frombuffer(mono, np.float32)
    assert np.isfinite(dual).all() and np.abs(mono).max() > 0
    assert np.array_equal(_bits(dual[:, 0]), _bits(dual[:, 1]))                                   # (a)
    assert np.array_equal(_bits(dual[:, 0]), _bits(mono))
    lr = np.frombuffer(_samples(out["lr"] / "sub" / "x.wav")[1], np.float32).reshape(9000, 2)
    rl = np.frombuffer(_samples(out["rl"] / "sub" / "x.wav")[1], np.float32).reshape(9000, 2)
    assert not np.array_equal(lr[:, 0], lr[:, 1])
    assert np.array_equal(_bits(lr[:, ::-1]), _bits(rl))                                          # (b)
    assert (out["mono"] / "sub" / "x.wav").read_bytes() == (tmp_path / "out_first" / "sub" / "x.wav").read_bytes()   # (c)


@pytest.mark.parametrize("precision,subtype,device_load", [("fp32", "FLOAT", True), ("bf16", "PCM_16", False)])
def test_restore_rate_writes_a_stereo_file_at_its_source_rate(tmp_path, precision, subtype, device_load):
    """(d) a 48 kHz stereo source of 16 000 frames (8000 samples at the model's rate, T' = 64) and a mono one beside it."""
    from universal_speech_enhancement_amd.SGMSE_module import SGMSEModule
    module = SGMSEModule(Score=_stages(precision)[0], sampler_kwargs=SAMPLER, wav_subtype=subtype)
    src = tmp_path / "noisy"
    src.mkdir()
    a = np.stack([_speech(16000, 91), _speech(16000, 92) * np.float32(0.3)], axis=1)
    wavio.write_wav(str(src / "s.wav"), a, 48000)
    wavio.write_wav(str(src / "m.wav"), _speech(12000, 93), 48000)
    batches = _enhance(module, src, tmp_path / "restored", restore_rate=True, device_load=device_load)
    assert len(batches) == 1 and batches[0]["file_rows"] == [(0, 1), (1, 2)] and batches[0]["source_length"] == [12000, 16000, 16000]
    enhanced = batches[0]["enhanced"].detach().float().cpu().numpy()
    dt = np.float32 if subtype == "FLOAT" else np.int16
    info, raw = _samples(tmp_path / "restored" / "s.wav")
    assert info == (16000, 2, 48000)                                                              # the source's channels, frames and rate
    got = np.frombuffer(raw, dt).reshape(16000, 2)
    for c in range(2):
        want64 = sr.oracle(enhanced[1 + c, :8000], 16000)
        (sr.check_float32 if subtype == "FLOAT" else sr.check_codes)(np.ascontiguousarray(got[:, c]), want64, f"s.wav channel {c}")
    info, raw = _samples(tmp_path / "restored" / "m.wav")
    assert info == (12000, 1, 48000)
    (sr.check_float32 if subtype == "FLOAT" else sr.check_codes)(np.frombuffer(raw, dt), sr.oracle(enhanced[0, :6000], 12000), "m.wav")


@pytest.mark.parametrize("precision,handoff_subtype", [("fp32", "PCM_16"), ("bf16", "PCM_16"), ("bf16", "FLOAT")])
def test_one_run_on_a_stereo_file_is_the_two_run_flow(tmp_path, precision, handoff_subtype):
    """(e) ``USEModule`` over a stereo and a mono file, stage-1 files kept; then ``GANModule`` over ``LoadWavData(stage-1 folder,
    channels="all")``: the refined files agree byte for byte, and the stage-1 file of the stereo source holds two channels."""
    from universal_speech_enhancement_amd.LSGAN_module import GANModule
    from universal_speech_enhancement_amd.USE_module import USEModule
    score, G = _stages(precision)
    noisy, S, R1, R2 = (tmp_path / d for d in ("noisy", "stage1", "one_run", "two_runs"))
    noisy.mkdir()
    wavio.write_wav(str(noisy / "s.wav"), np.stack([_speech(9000, 71) * np.float32(0.2), _speech(9000, 72)], axis=1), 24000, wavio.FLOAT32)
    wavio.write_wav(str(noisy / "m.wav"), _speech(7300, 73), 24000, wavio.FLOAT32)
    pipe = USEModule(Score=score, G=G, sampler_kwargs=SAMPLER, handoff_subtype=handoff_subtype, stage1_folder=str(S))
    batches = _enhance(pipe, noisy, R1)
    assert len(batches) == 1 and batches[0]["file_rows"] == [(0, 1), (1, 2)] and batches[0]["handoff_peak"].shape == (2,)
    x, _ = wavio.read_wav(str(S / "s.wav"))
    assert x.shape == (9000, 2) and float(batches[0]["handoff_peak"][1]) == np.abs(x).max()      # the peak of the whole stage-1 file
    _enhance(GANModule(G=G, sampler_kwargs=pipe.refine_kwargs), S, R2)
    for name, info in (("s.wav", (9000, 2, 24000)), ("m.wav", (7300, 1, 24000))):
        assert wavio.wav_info(str(R1 / name)) == wavio.wav_info(str(S / name)) == info, name
        assert (R1 / name).read_bytes() == (R2 / name).read_bytes(), (handoff_subtype, name)
        assert (R1 / name).read_bytes() != (S / name).read_bytes()


def test_predict_with_all_channels_scores_every_channel(tmp_path):
    """``predict data.channels=all`` with ``data.clean_folder``: one CSV row per (file, channel) and a channel column; a clean file with
    another channel count is skipped; the default CSV keeps its columns."""
    from universal_speech_enhancement_amd import predict as P
    src, clean = tmp_path / "noisy", tmp_path / "clean"
    src.mkdir()
    clean.mkdir()
    s = np.stack([_speech(9000, 61), _speech(9000, 62) * np.float32(0.4)], axis=1)
    wavio.write_wav(str(src / "s.wav"), s, 24000)
    wavio.write_wav(str(clean / "s.wav"), (s * 0.9).astype(np.float32), 24000)
    wavio.write_wav(str(src / "t.wav"), s[::-1].copy(), 24000)
    wavio.write_wav(str(clean / "t.wav"), s[:, 0].copy(), 24000)                                  # mono: another channel count
    common = ["model=SGMSE_Large", f"data.data_folder={src}", f"data.clean_folder={clean}", "random_init_seed=1", "model.sampler_kwargs.N=1",
              "data.batch_size=4", "data.convergence_losses=true", "model.sampler_kwargs.per_item=true"]
    assert P.predict(P.compose(common + [f"data.target_folder={tmp_path / 'all'}", "data.channels=all"])) == 2      # files, not rows
    assert P.predict(P.compose(common + [f"data.target_folder={tmp_path / 'first'}"])) == 2
    assert wavio.wav_info(str(tmp_path / "all" / "s.wav")) == (9000, 2, 24000)
    assert wavio.wav_info(str(tmp_path / "first" / "s.wav")) == (9000, 1, 24000)
    for name in ("metrics.csv", "losses.csv"):
        lines = (tmp_path / "all" / name).read_text().splitlines()
        assert lines[0].startswith("file,channel,") and [ln.split(",")[:2] for ln in lines[1:]] == [["s.wav", "0"], ["s.wav", "1"], ["mean", ""]]
        assert not any(np.isnan(float(v)) for ln in lines[1:] for v in ln.split(",")[2:])
        first = (tmp_path / "first" / name).read_text().splitlines()
        assert first[0].startswith("file,") and "channel" not in first[0] and len(first) == 4
