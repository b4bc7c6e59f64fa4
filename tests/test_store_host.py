"""Host-side checks of the device-side store path (csrc/use_resample.hip: ``use_store_workspace`` / ``use_store_items_dev``;
csrc/use_io.cpp: ``use_wav_write_pcm16``; ``wavio.store_items_host``; ``LoadWavData(restore_rate=...)``): the exported entries, the
argument checks (they run before any device call), the raw writer, the host arithmetic against scipy, the round trip through the
model's rate, and the batch keys.  No device is touched.  Every figure is printed before it is asserted (``pytest -s``)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import store_ref as sr
from universal_speech_enhancement_amd import _lib, predict as P, wavio
from universal_speech_enhancement_amd.data import LoadWavData

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_are_declared_exported_and_listed():
    L = C.CDLL(_lib.LIB_PATH)
    i, i64, vp = C.c_int, C.c_int64, C.c_void_p
    want = {"use_store_workspace": (C.c_size_t, [i64, i64]),
            "use_store_items_dev": (i, [vp, i64, C.POINTER(i), C.POINTER(i64), i, i, vp, i64, vp, C.c_size_t, vp]),
            "use_wav_write_pcm16": (i, [C.c_char_p, vp, i64, i, i])}
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "use_hip.h")).read(), flags=re.S)
    for name, (res, args) in want.items():
        assert hasattr(L, name), name
        assert _lib.SYMBOLS[name] == (res, args), name
        decl = re.search(r"\b" + name + r"\s*\(([^;]*)\);", header)
        assert decl and len(decl.group(1).split(",")) == len(args), name              # one parameter per declared argument type


def test_workspace_size_and_refusals():
    ws = _lib.lib().use_store_workspace
    for n, num in [(0, 5), (5, 0), (-1, 5), (5, -1), (2 ** 24 + 1, 100), (100, 2 ** 24 + 1)]:
        assert ws(n, num) == 0, (n, num)
    for n, num in [(1, 1), (2400, 4800), (2400, 2400), (2 ** 24, 2 ** 24), (2 ** 24, 1), (1, 2 ** 24)]:
        assert ws(n, num) > 0, (n, num)
    # the resampler's workspace and the row widened to fp64
    assert ws(2400, 4800) >= _lib.lib().use_resample_workspace(2400, 4800) + 8 * 2400


def test_store_items_dev_rejects_bad_arguments_without_a_device():
    L = _lib.lib()
    good, big = 0x10000, 2 ** 25                                      # an aligned address that is never dereferenced: nothing is launched
    need = L.use_store_workspace(3000, 6000)
    base = dict(wav=good, stride=4000, lens=[3000, 2000], nums=[6000, 2000], B=2, subtype=wavio.PCM16, out=good, out_stride=6000,
                work=good, work_bytes=need)

    def call(**kw):
        a = {**base, **kw}
        lens = None if a["lens"] is None else (C.c_int * len(a["lens"]))(*a["lens"])
        nums = None if a["nums"] is None else (C.c_int64 * len(a["nums"]))(*a["nums"])
        return L.use_store_items_dev(a["wav"], a["stride"], lens, nums, a["B"], a["subtype"], a["out"], a["out_stride"], a["work"],
                                     a["work_bytes"], None)

    cases = [("null wav", dict(wav=None), b"null"), ("null out", dict(out=None), b"null"), ("null work", dict(work=None), b"null"),
             ("null len_host", dict(lens=None), b"null"), ("null num_host", dict(nums=None), b"null"),
             ("misaligned wav", dict(wav=good + 2), b"aligned"), ("misaligned PCM16 out", dict(out=good + 1), b"aligned"),
             ("misaligned FLOAT32 out", dict(out=good + 2, subtype=wavio.FLOAT32), b"aligned"),
             ("misaligned work", dict(work=good + 8), b"aligned"),
             ("B = 0", dict(B=0), b"B=0"), ("B < 0", dict(B=-1), b"B=-1"),
             ("len = 0", dict(lens=[3000, 0]), b"positive"), ("len > stride", dict(lens=[3000, 4001]), b"stride"),
             ("num = 0", dict(nums=[0, 2000]), b"positive"), ("num > out_stride", dict(nums=[6000, 6001]), b"out_stride"),
             ("len > 2^24", dict(lens=[2 ** 24 + 1, 2000], stride=big, work_bytes=2 ** 40), b"2^24"),
             ("num > 2^24", dict(nums=[6000, 2 ** 24 + 1], out_stride=big, work_bytes=2 ** 40), b"2^24"),
             ("unknown subtype", dict(subtype=2), b"subtype"), ("negative subtype", dict(subtype=-1), b"subtype"),
             ("short workspace", dict(work_bytes=need - 1), b"work_bytes"), ("no workspace", dict(work_bytes=0), b"work_bytes")]
    for what, kw, word in cases:
        rc, msg = call(**kw), L.use_last_error()
        print(what, rc, msg)
        assert rc == -1 and word in msg and b"use_store_items_dev" in msg, (what, rc, msg)          # USE_E_INVALID


def test_wav_write_pcm16_writes_the_bytes_of_wav_write(tmp_path):
    q = np.concatenate([np.array([-32768, 32767, 0, -1, 1, -32767, 32766], np.int16), np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)])
    x = (q.astype(np.float64) / 32767).astype(np.float32)
    for ch, rate in [(1, 48000), (2, 44100), (1, 8000)]:
        n = len(q) // ch * ch
        a, b = str(tmp_path / f"raw{ch}.wav"), str(tmp_path / f"float{ch}.wav")
        wavio.write_wav_pcm16(a, q[:n] if ch == 1 else q[:n].reshape(-1, ch), rate)
        wavio.write_wav(b, x[:n] if ch == 1 else x[:n].reshape(-1, ch), rate)
        raw = open(a, "rb").read()
        assert raw == open(b, "rb").read() and len(raw) == 44 + 2 * n, (ch, rate)
        assert wavio.wav_info(a) == (n // ch, ch, rate)
        assert np.array_equal(np.frombuffer(raw[44:], np.int16), q[:n])
    empty = str(tmp_path / "empty.wav")
    wavio.write_wav_pcm16(empty, np.zeros(0, np.int16), 16000)
    assert wavio.wav_info(empty) == (0, 1, 16000)
    with pytest.raises(TypeError):
        wavio.write_wav_pcm16(empty, np.zeros(4, np.float32), 16000)
    assert _lib.lib().use_wav_write_pcm16(os.fsencode(empty), None, 4, 1, 16000) == -1
    assert _lib.lib().use_wav_write_pcm16(os.fsencode(empty), q.ctypes.data_as(C.c_void_p), 4, 0, 16000) == -1


@pytest.mark.parametrize("n,num", sr.SHAPES)
def test_store_items_host_follows_scipy_and_the_writer(n, num):
    x = sr.signal(n, num)
    wav = np.full((2, n + 5), np.nan, np.float32)                     # the padding of a row is never read
    wav[0, :n] = x
    wav[1, :1] = 0.25
    got = wavio.store_items_host(torch.from_numpy(wav), [n, 1], [num, 1], wavio.FLOAT32)
    assert got.dtype == np.float32 and got.shape == (2, num) and np.isfinite(got).all()
    sr.check_float32(got[0], sr.oracle(x, num), f"host {n} -> {num}")
    assert got[1, 0] == np.float32(0.25) and not got[1, 1:].any()
    codes = wavio.store_items_host(torch.from_numpy(wav), [n, 1], [num, 1], wavio.PCM16)
    assert codes.dtype == np.int16 and codes.shape == (2, num)
    assert np.array_equal(codes[0], sr.quantise(got[0])) and codes[1, 0] == 8192 and not codes[1, 1:].any()


def test_store_items_host_at_an_unchanged_length_is_the_writer(tmp_path):
    x = np.array([0.0, -0.0, 1.0, -1.0, 1.5, -1.5, 1e9, -1e9, np.nan, 0.5 / 32767, 1.5 / 32767, -0.5 / 32767, -2.5 / 32767, 0.3], np.float32)
    got = wavio.store_items_host(torch.from_numpy(x)[None], [len(x)], [len(x)], wavio.FLOAT32)
    assert np.array_equal(got[0].view(np.uint32), x.view(np.uint32))
    codes = wavio.store_items_host(torch.from_numpy(x)[None], [len(x)], [len(x)], wavio.PCM16)
    path = str(tmp_path / "w.wav")
    wavio.write_wav(path, x, 24000)
    assert codes[0].tobytes() == open(path, "rb").read()[44:]
    assert np.array_equal(codes[0], sr.quantise(x))
    for bad in (dict(lens=[0]), dict(lens=[len(x) + 1]), dict(nums=[0]), dict(lens=[1, 1])):
        with pytest.raises(ValueError):
            wavio.store_items_host(torch.from_numpy(x)[None], **{**dict(lens=[3], nums=[3]), **bad})
    with pytest.raises(ValueError):
        wavio.store_items_host(torch.from_numpy(x)[None], [3], [3], 2)


@pytest.mark.parametrize("source,model", [(4800, 2400), (4410, 2400), (1600, 2400), (4799, 2400)])
def test_round_trip_through_the_models_rate(source, model):
    """A periodic signal with every component below 0.45 of the lower rate (bins below 0.45 * min(source, model)), peak 0.8: source
    rate -> the model's rate -> float32 -> back to ``source`` frames.  Both resamplings are exact for such a signal, so what comes back
    differs by the two float32 roundings (half an ulp at 0.8 = 3e-8 each) and the fp64 arithmetic: within 2^-23, one ulp at full scale."""
    rng = np.random.default_rng(source)
    kmax = int(0.45 * min(source, model))
    t = np.arange(source) / source
    x = sum(rng.uniform(0.2, 1.0) * np.cos(2 * np.pi * (k * t + rng.uniform())) for k in rng.choice(np.arange(1, kmax), 12, replace=False))
    x = x / np.abs(x).max() * 0.8
    at_model = wavio.resample_fft(x, model).astype(np.float32)
    back = wavio.store_items_host(torch.from_numpy(at_model)[None], [model], [source], wavio.FLOAT32)[0]
    err = float(np.abs(back.astype(np.float64) - x).max())
    print(f"{source} -> {model} -> {source}: max |back - x| = {err:.3e}, bound = {2.0 ** -23:.3e}")
    assert back.shape == (source,) and err <= 2.0 ** -23


def _folder(tmp_path):
    src = tmp_path / "noisy"
    (src / "sub").mkdir(parents=True)
    rng = np.random.default_rng(3)
    spec = [("a.wav", 48000, 3000), ("b.wav", 24000, 2000), ("sub/c.wav", 44100, 147 * 10), ("d.wav", 16000, 1001)]
    for rel, rate, frames in spec:
        wavio.write_wav(str(src / rel), (rng.standard_normal(frames) * 0.2).astype(np.float32), rate)
    return src, spec


def test_batches_carry_the_source_only_with_restore_rate(tmp_path):
    src, _ = _folder(tmp_path)
    plain = LoadWavData(str(src), str(tmp_path / "out"), batch_size=3)
    keys = ["perturbed", "name", "sample_length", "sampling_rate", "audio_path", "data_folder", "target_folder"]
    assert plain.restore_rate is False
    plain_batches = list(plain.predict_batches(device="cpu"))
    assert all(list(b) == keys for b in plain_batches)
    data = LoadWavData(str(src), str(tmp_path / "out"), batch_size=3, restore_rate=True)
    assert data.restore_rate is True
    batches = list(data.predict_batches(device="cpu"))
    assert len(batches) == len(plain_batches) == 2
    for b, p in zip(batches, plain_batches):
        assert list(b) == keys + ["source_rate", "source_length"]
        info = [wavio.wav_info(path) for path in b["audio_path"]]
        assert b["source_rate"] == [sr_ for _, _, sr_ in info] and b["source_length"] == [f for f, _, _ in info]
        assert b["sampling_rate"] == [24000] * len(info)
        for k in keys:                                                # everything else: what the loader yields without the option
            assert torch.equal(b[k], p[k]) if isinstance(b[k], torch.Tensor) else b[k] == p[k], k
    cfg = P.compose([])
    assert cfg["data"]["restore_rate"] is False and P.compose(["data.restore_rate=true"])["data"]["restore_rate"] is True
    assert "data.restore_rate" in P.__doc__


@pytest.mark.parametrize("subtype", ["PCM_16", "FLOAT"])
def test_write_items_restores_a_cpu_batch(tmp_path, subtype):
    """``_write_items`` on CPU tensors (``store_items_host``): every file at its source's rate and frame count, its samples
    ``store_items_host`` of the model-rate row; the 24 kHz file and a batch without the keys: the bytes written today."""
    from universal_speech_enhancement_amd.SGMSE_module import _write_items
    src, spec = _folder(tmp_path)
    batch = next(iter(LoadWavData(str(src), str(tmp_path / "out"), batch_size=4, restore_rate=True).predict_batches(device="cpu")))
    wavs = batch["perturbed"] * 0.5
    code = wavio.PCM16 if subtype == "PCM_16" else wavio.FLOAT32
    _write_items(batch, wavs, str(tmp_path / "restored"), subtype)
    _write_items(batch, wavs, str(tmp_path / "stage1"), subtype, restore=False)
    _write_items({k: v for k, v in batch.items() if not k.startswith("source_")}, wavs, str(tmp_path / "plain"), subtype)
    want = wavio.store_items_host(wavs, batch["sample_length"], batch["source_length"], code)
    by_name = {os.path.basename(rel): (rate, frames) for rel, rate, frames in spec}
    for i, path in enumerate(batch["audio_path"]):
        rate, frames = by_name[os.path.basename(path)]
        out = path.replace(str(src), str(tmp_path / "restored"))
        assert wavio.wav_info(out) == (frames, 1, rate), path
        raw = open(out, "rb").read()
        assert raw[44:] == want[i, :frames].tobytes(), path
        plain = open(path.replace(str(src), str(tmp_path / "plain")), "rb").read()
        assert open(path.replace(str(src), str(tmp_path / "stage1")), "rb").read() == plain
        assert wavio.wav_info(path.replace(str(src), str(tmp_path / "plain")))[2] == 24000
        assert (raw == plain) == (rate == 24000), path
