"""Host-side checks of the device loader (csrc/use_resample.hip, wavio.load_batch_device, LoadWavData(device_load=...)): the exported
entries and their prototypes, the workspace size, the refusal of a CPU device, and that the default loader yields what it always did.
No device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from universal_speech_enhancement_amd import _lib, predict as P, wavio
from universal_speech_enhancement_amd.data import LoadWavData

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_are_exported_with_the_declared_prototypes():
    L = C.CDLL(_lib.LIB_PATH)
    i64, vp = C.c_int64, C.c_void_p
    want = {"use_resample_workspace": (C.c_size_t, [i64, i64]),
            "use_resample_fft_dev": (C.c_int, [vp, i64, i64, vp, vp, C.c_size_t, vp]),
            "use_load_items_dev": (C.c_int, [C.POINTER(vp), C.POINTER(i64), C.POINTER(i64), C.c_int, C.c_int, vp, i64, vp, C.c_size_t, vp])}
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "use_hip.h")).read(), flags=re.S)
    for name, (res, args) in want.items():
        assert hasattr(L, name), name
        assert _lib.SYMBOLS[name] == (res, args), name
        decl = re.search(r"\b" + name + r"\s*\(([^;]*)\);", header)
        assert decl and len(decl.group(1).split(",")) == len(args), name              # one parameter per declared argument type


def test_workspace_size():
    ws = _lib.lib().use_resample_workspace
    for ratio in (0.5, 1.5, 24000 / 44100):
        pairs = [(n, max(1, int(np.ceil(n * ratio)))) for n in (1, 2, 3, 100, 1023, 1024, 1025, 4800, 48000, 131073, 480000, 2 ** 22, 2 ** 23,
                                                                 2 ** 24)]
        sizes = [ws(n, num) for n, num in pairs if max(n, num) <= 2 ** 24]
        assert len(sizes) >= 13 and all(s > 0 for s in sizes) and sizes == sorted(sizes), (ratio, sizes)
    assert ws(48000, 48000) > 0                                                      # no resampling: the partial maxima alone
    assert ws(48000, 48000) < ws(48000, 24000)
    # three FFT buffers of Bluestein's M = 2^17 >= 2 * 48000 - 1 points, 16 bytes each, are the bulk of it
    assert 3 * 16 * 2 ** 17 <= ws(48000, 24000) <= 3 * 16 * 2 ** 17 + 16 * 48000
    for n, num in [(2 ** 24 + 1, 100), (100, 2 ** 24 + 1), (0, 5), (5, 0), (-1, 5)]:
        assert ws(n, num) == 0, (n, num)


def _folder(tmp_path):
    src = tmp_path / "noisy"
    (src / "sub").mkdir(parents=True)
    rng = np.random.default_rng(3)
    for rel, rate, frames in [("a.wav", 48000, 3000), ("b.wav", 24000, 2000), ("sub/c.wav", 44100, 147 * 10)]:
        wavio.write_wav(str(src / rel), (rng.standard_normal(frames) * 0.2).astype(np.float32), rate)
    return src


def test_device_load_on_a_cpu_device_raises(tmp_path):
    data = LoadWavData(str(_folder(tmp_path)), str(tmp_path / "out"), device_load=True)
    assert data.device_load and data.device_load_max_samples == 2 ** 24
    with pytest.raises(ValueError, match="device_load"):
        data.predict_batches(device="cpu")
    with pytest.raises(ValueError):
        wavio.load_batch_device(data.filepaths, 24000, True, torch.device("cpu"))


def test_the_default_loader_is_unchanged(tmp_path):
    src = _folder(tmp_path)
    data = LoadWavData(str(src), str(tmp_path / "out"), batch_size=2)
    assert data.device_load is False
    batches = list(data.predict_batches(device="cpu"))
    assert [b["name"] for b in batches] == [["a", "b"], ["c"]]
    for b in batches:
        assert list(b) == ["perturbed", "name", "sample_length", "sampling_rate", "audio_path", "data_folder", "target_folder"]
        rows = [wavio.load_utterance(p, 24000, True)[0] for p in b["audio_path"]]
        lens = [len(r) for r in rows]
        assert b["perturbed"].dtype == torch.float32 and tuple(b["perturbed"].shape) == (len(rows), max(lens))
        assert b["sample_length"].dtype == torch.int32 and b["sample_length"].tolist() == lens and b["sampling_rate"] == [24000] * len(rows)
        for k, r in enumerate(rows):
            assert np.array_equal(b["perturbed"][k, : lens[k]].numpy().view(np.uint32), r.view(np.uint32))
            assert not b["perturbed"][k, lens[k]:].any()
    cfg = P.compose([])
    assert cfg["data"]["device_load"] is False and cfg["data"]["device_load_max_samples"] == 2 ** 24
    assert P.compose(["data.device_load=true"])["data"]["device_load"] is True
