"""CPU checks of ``data.restore_level`` (the host functions need no device): the new entry points exist, ``use_load_utterance_peak``
hands out the divisor itself, ``wavio.store_items_host(gains=)`` is the numpy formula of tests/level_ref.py, and a file that goes
through the host loader, an identity stand-in for the sampler and the shared writer comes back at its source's level."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import level_ref as lv
import store_ref as sr
from universal_speech_enhancement_amd import _lib, wavio
from universal_speech_enhancement_amd.data import LoadWavData
from universal_speech_enhancement_amd.SGMSE_module import SGMSEModule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["use_load_utterance_peak", "use_load_items_dev_peak", "use_load_files_dev_peak", "use_store_items_dev_gain", "use_store_files_dev_gain"]
TODAY = {"perturbed", "name", "sample_length", "sampling_rate", "audio_path", "data_folder", "target_folder"}


def test_the_new_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "use_hip.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint " + name + r"\s*\(", header), name
        assert hasattr(L, name) and name in _lib.SYMBOLS, name


def _speech(n, seed, level):
    """A smooth signal with its peak at exactly float32(level)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 24000.0
    w = sum(rng.standard_normal() * np.sin(2 * np.pi * f * t + rng.uniform(0, 6)) for f in (110.0, 220.0, 450.0, 1300.0, 3100.0))
    w = w * (0.3 + 0.7 * np.sin(2 * np.pi * 3.0 * t) ** 2)
    return (w / np.abs(w).max() * level).astype(np.float32)


@pytest.mark.parametrize("rate", [24000, 48000, 44100])
def test_load_utterance_peak_is_the_divisor(tmp_path, rate):
    path = str(tmp_path / "s.wav")
    a = np.stack([_speech(3000, 1, 0.21), _speech(3000, 2, 0.9)], axis=1)          # the louder channel is not the first
    wavio.write_wav(path, a, rate)
    x = wavio.read_wav(path)[0][:, 0]
    if rate != 24000:
        x = wavio.resample_fft(x, wavio.resampled_length(3000, rate, 24000))
    row, sr_, mx = wavio.load_utterance(path, 24000, True, return_peak=True)
    plain, _ = wavio.load_utterance(path, 24000, True)
    assert sr_ == 24000 and isinstance(mx, np.float64) and mx == np.abs(x).max() and mx > 0         # bit for bit
    assert np.array_equal(row.view(np.uint32), plain.view(np.uint32))
    assert np.array_equal(row.view(np.uint32), (x / mx * 0.8).astype(np.float32).view(np.uint32))
    assert wavio.source_gain(mx) == mx / np.float64(0.8) and wavio.source_gain(None) == 1.0
    # normalize = 0: the pointer is not written
    p, n, r, poison = C.POINTER(C.c_float)(), C.c_int64(), C.c_int(), C.c_double(-77.0)
    assert _lib.lib().use_load_utterance_peak(os.fsencode(path), 24000, 0, C.byref(p), C.byref(n), C.byref(r), C.byref(poison)) == 0
    _lib.lib().use_free(p)
    assert poison.value == -77.0
    assert wavio.load_utterance(path, 24000, False, return_peak=True)[2] is None


def test_load_file_channels_peak_is_taken_over_all_channels(tmp_path):
    path = str(tmp_path / "s.wav")
    a = np.stack([_speech(3000, 3, 0.1), _speech(3000, 4, 0.6)], axis=1)
    wavio.write_wav(path, a, 48000)
    rows, _, mx = wavio.load_file_channels(path, 24000, True, return_peak=True)
    x = np.stack([wavio.resample_fft(c, 1500) for c in wavio.read_wav(path)[0].T])
    assert mx == np.abs(x).max() and mx == np.abs(x[1]).max() > np.abs(x[0]).max()
    assert np.array_equal(rows.view(np.uint32), wavio.load_file_channels(path, 24000, True)[0].view(np.uint32))
    assert wavio.load_file_channels(path, 24000, False, return_peak=True)[2] is None
    wavio.write_wav(path, a[:, 0].copy(), 24000)                                                   # mono: load_utterance's peak
    assert wavio.load_file_channels(path, 24000, True, return_peak=True)[2] == wavio.load_utterance(path, 24000, True, return_peak=True)[2]


@pytest.mark.parametrize("n,num", lv.SHAPES)
def test_store_items_host_with_gains_is_the_numpy_formula(n, num):
    x = sr.signal(n, num)
    wav = torch.from_numpy(np.stack([x] * len(lv.GAINS)))
    f = wavio.store_items_host(wav, [n] * 4, [num] * 4, wavio.FLOAT32, gains=lv.GAINS)
    q = wavio.store_items_host(wav, [n] * 4, [num] * 4, wavio.PCM16, gains=lv.GAINS)
    for b, g in enumerate(lv.GAINS):
        lv.check_row(f[b], x, num, g, f"host {n} -> {num}, g = {g}")
        assert np.array_equal(q[b], sr.quantise(f[b])), g
    assert not f[3].any() and not q[3].any()                                                        # g = 0
    plain = wavio.store_items_host(wav[:1], [n], [num], wavio.FLOAT32)
    assert np.array_equal(plain.view(np.uint32), wavio.store_items_host(wav[:1], [n], [num], wavio.FLOAT32, gains=None).view(np.uint32))
    if n >= 255:
        clamped = q[2].astype(np.int32)
        print(f"{n} -> {num}: {(clamped == 32767).sum()} codes at +32767 and {(clamped == -32768).sum()} at -32768 of {num} at g = 3")
        assert (clamped == 32767).sum() > 0 and (clamped == -32768).sum() > 0


def test_store_host_refuses_bad_gains_and_files_take_one_gain_per_file():
    x = torch.from_numpy(np.stack([sr.signal(300, 300), sr.signal(300, 301)[:300], sr.signal(300, 302)[:300]]))
    for bad in (float("nan"), float("inf"), -1.0):
        with pytest.raises(ValueError):
            wavio.store_items_host(x, [300] * 3, [300] * 3, wavio.PCM16, gains=[1.0, bad, 1.0])
    with pytest.raises(ValueError):
        wavio.store_items_host(x, [300] * 3, [300] * 3, wavio.PCM16, gains=[1.0, 1.0])
    for num in (300, 450):
        files = wavio.store_files_host(x, [300, 300], [num, num], [1, 2], wavio.FLOAT32, gains=[0.25, 2.5])
        rows = wavio.store_items_host(x, [300] * 3, [num] * 3, wavio.FLOAT32, gains=[0.25, 2.5, 2.5])
        assert files[0].shape == (num, 1) and files[1].shape == (num, 2)
        assert np.array_equal(files[0][:, 0].view(np.uint32), rows[0].view(np.uint32))
        assert np.array_equal(np.ascontiguousarray(files[1].T).view(np.uint32), rows[1:].view(np.uint32))


class _Identity(torch.nn.Module):
    """The stand-in for ``Score.sample``: the enhanced batch is the perturbed one."""

    def sample(self, batch, **kw):
        batch["enhanced"] = batch["perturbed"]
        return batch


def _run(src, dst, subtype="FLOAT", **data_kw):
    module = SGMSEModule(Score=_Identity(), wav_subtype=subtype)
    return [module.predict_step(b, i) for i, b in enumerate(LoadWavData(str(src), str(dst), batch_size=4, **data_kw).predict_batches("cpu"))]


@pytest.fixture()
def corpus(tmp_path):
    src = tmp_path / "noisy"
    src.mkdir()
    levels = {"a.wav": 0.1, "b.wav": 0.5, "c.wav": 0.9, "d.wav": 0.03}
    for i, (name, level) in enumerate(levels.items()):
        w = _speech(2000 + 700 * i, 10 + i, level)
        w[5:9] = 0.0                                                                                # exact zeros stay zeros
        wavio.write_wav(str(src / name), w, 24000, wavio.PCM16 if i % 2 else wavio.FLOAT32)         # half of them 16-bit sources
    return src, levels


def test_round_trip_brings_every_file_back_at_its_level(corpus, tmp_path):
    src, levels = corpus
    batches = _run(src, tmp_path / "out", restore_level=True)
    assert len(batches) == 1 and set(batches[0]) == TODAY | {"source_gain", "enhanced"}
    g = batches[0]["source_gain"]
    assert isinstance(g, torch.Tensor) and g.dtype == torch.float64 and g.device.type == "cpu" and g.shape == (4,)
    plain = _run(src, tmp_path / "plain")
    assert torch.equal(batches[0]["perturbed"], plain[0]["perturbed"])                              # the tensors do not move
    for i, name in enumerate(levels):
        want, rate = wavio.read_wav(str(src / name))
        got, rate2 = wavio.read_wav(str(tmp_path / "out" / name))
        assert rate == rate2 == 24000 and got.shape == want.shape
        assert float(g[i]) == np.abs(want).max() / np.float64(0.8)
        err = np.abs(got - want)
        worst = float((err[want != 0] / np.abs(want[want != 0])).max())
        print(f"{name}: peak {np.abs(want).max():.6f} -> {np.abs(got).max():.6f}, worst relative error 2^{np.log2(max(worst, 1e-300)):.2f}")
        assert (err <= lv.ROUND_TRIP * np.abs(want)).all(), name
        assert not got[want == 0].any() and (want == 0).sum() >= 4
        flat, _ = wavio.read_wav(str(tmp_path / "plain" / name))
        assert abs(np.abs(flat).max() - 0.8) < 1e-6                                                 # without the flag: every file near 0.8


@pytest.mark.parametrize("subtype", ["PCM_16", "FLOAT"])
def test_without_normalisation_the_gain_is_one_and_the_files_do_not_change(corpus, tmp_path, subtype):
    src, levels = corpus
    on = _run(src, tmp_path / "on", subtype, restore_level=True, normalize=False)
    off = _run(src, tmp_path / "off", subtype, normalize=False)
    assert set(off[0]) == TODAY | {"enhanced"}                                                      # flag off: exactly today's keys
    assert on[0]["source_gain"].tolist() == [1.0] * 4
    for name in levels:
        assert (tmp_path / "on" / name).read_bytes() == (tmp_path / "off" / name).read_bytes(), name


def test_flag_off_is_todays_batch_for_every_loader_mode(corpus, tmp_path):
    src, _ = corpus
    for kw in ({}, {"channels": "all"}, {"restore_rate": True}):
        b = next(iter(LoadWavData(str(src), str(tmp_path / "x"), batch_size=4, **kw).predict_batches("cpu")))
        extra = ({"channel", "n_channels", "file_rows"} if "channels" in kw else set()) | ({"source_rate", "source_length"} if "restore_rate" in kw else set())
        assert set(b) == TODAY | extra, kw
        on = next(iter(LoadWavData(str(src), str(tmp_path / "x"), batch_size=4, restore_level=True, **kw).predict_batches("cpu")))
        assert set(on) == TODAY | extra | {"source_gain"} and torch.equal(on["perturbed"], b["perturbed"]), kw


def test_a_stereo_file_takes_one_gain_and_restore_rate_combines(tmp_path):
    src = tmp_path / "noisy"
    src.mkdir()
    a = np.stack([_speech(4800, 21, 0.05), _speech(4800, 22, 0.4)], axis=1)
    wavio.write_wav(str(src / "s.wav"), a, 48000, wavio.FLOAT32)
    batches = _run(src, tmp_path / "out", channels="all", restore_level=True, restore_rate=True)
    g = batches[0]["source_gain"]
    assert g.shape == (2,) and float(g[0]) == float(g[1]) > 0
    assert wavio.wav_info(str(tmp_path / "out" / "s.wav")) == (4800, 2, 48000)
    got = wavio.read_wav(str(tmp_path / "out" / "s.wav"))[0]
    want = wavio.store_files_host(batches[0]["enhanced"], [2400], [4800], [2], wavio.FLOAT32, gains=[float(g[0])])[0]
    assert np.array_equal(got.astype(np.float32).view(np.uint32), want.view(np.uint32))
    # down to the model's rate and back up: the band above 12 kHz is gone, the level is the source's
    ratio = np.abs(got).max(axis=0) / np.abs(a).max(axis=0)
    print("peak ratios of the two channels after 48 -> 24 -> 48 kHz:", ratio)
    assert (np.abs(ratio - 1) < 0.05).all()
