"""CPU-only checks of own-length sampling: the grouping rule at its boundaries, the header-derived lengths the bucketing loader
relies on, the bucketed batches (a disjoint cover of the rank's shard, one T' per batch, stable), the exact frame counts of the
mixed-length measurement, and the argument errors of ``use_stft_fwd_items`` / ``use_istft_back_items`` that need no device."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from universal_speech_enhancement_amd import _lib
from universal_speech_enhancement_amd.data import LoadWavData
from universal_speech_enhancement_amd.distributed import shard_list
from universal_speech_enhancement_amd.sgmse.util.spectral import SpectralGlue
from universal_speech_enhancement_amd.wavio import FLOAT32, load_utterance, read_wav, resampled_length, wav_info, write_wav

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _glue(n_fft=1022, hop=160):
    g = SpectralGlue()
    g._init_spectral(n_fft, hop, 512, "hann", 0.15, 0.5)
    return g


# ---- length_groups ---------------------------------------------------------------------------------------------------------------
def test_length_groups_at_the_64_frame_boundary():
    g = _glue()
    assert 1 + 10239 // 160 == 64 and 1 + 10240 // 160 == 65
    assert g.length_groups([10239]) == [(64, [0])]
    assert g.length_groups([10240]) == [(128, [0])]
    assert g.length_groups([10240, 10239]) == [(64, [1]), (128, [0])]
    assert g.length_groups(torch.tensor([12000, 9600, 4000, 9600, 10240])) == [(64, [1, 2, 3]), (128, [0, 4])]
    assert g.length_groups(np.array([12000, 9600, 4000, 9600, 10240], dtype=np.int32)) == [(64, [1, 2, 3]), (128, [0, 4])]


def test_length_groups_shortest_legal_item_and_the_refusal():
    g = _glue()
    assert g.length_groups([512]) == [(64, [0])]                               # n_fft // 2 = 511: reflect padding needs more than that
    with pytest.raises(ValueError, match="item 1"):
        g.length_groups([9600, 511, 4000])
    with pytest.raises(ValueError, match="item 0"):
        g.length_groups([0])


def test_length_groups_are_stable_in_order():
    g = _glue()
    lens = [30000, 4000, 9600, 30001, 512, 20480, 20479, 4000]
    want = [(64, [1, 2, 4, 7]), (128, [6]), (192, [0, 3, 5])]
    assert g.length_groups(lens) == want
    assert g.length_groups(list(lens)) == want
    for Tp, idx in want:
        assert idx == sorted(idx) and all((1 + lens[i] // 160 + 63) // 64 * 64 == Tp for i in idx)
    assert [Tp for Tp, _ in want] == sorted(Tp for Tp, _ in want)


# ---- header-derived lengths ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,frames", [(16000, 5000), (22050, 4999), (44100, 147 * 40), (48000, 7001), (24000, 6000)])
def test_resampled_length_is_what_the_loader_gives(tmp_path, sr, frames):
    x = (np.random.RandomState(sr).randn(frames) * 0.1).astype(np.float32)
    p = str(tmp_path / f"f{sr}.wav")
    write_wav(p, x, sr, FLOAT32)
    n, ch, rate = wav_info(p)
    assert (n, ch, rate) == (frames, 1, sr)
    wav, out_sr = load_utterance(p, 24000, True)
    assert out_sr == 24000
    assert resampled_length(n, rate, 24000) == len(wav)
    if sr == 44100:                      # the ratio-first rounding: one sample more than ceil(frames * 24000 / 44100) in exact arithmetic
        assert len(wav) == -(-frames * 24000 // 44100) + 1
    assert resampled_length(n, rate, 0) == n and resampled_length(n, rate, rate) == n
    with pytest.raises(ValueError):
        resampled_length(-1, rate, 24000)


def test_wav_info_agrees_with_read_wav(tmp_path):
    from scipy.io import wavfile
    rng = np.random.RandomState(1)
    cases = {"pcm16_stereo.wav": (48000, (rng.randn(801, 2) * 3000).astype(np.int16)),
             "float_mono.wav": (22050, (rng.randn(1234) * 0.1).astype(np.float32)),
             "pcm32_mono.wav": (8000, (rng.randn(77) * 1e6).astype(np.int32)),
             "u8_mono.wav": (16000, rng.randint(0, 255, 301).astype(np.uint8))}
    for name, (sr, a) in cases.items():
        p = str(tmp_path / name)
        wavfile.write(p, sr, a)
        x, rate = read_wav(p)
        frames, ch, sr2 = wav_info(p)
        assert (frames, sr2) == (x.shape[0], rate) == (a.shape[0], sr), name
        assert ch == (1 if x.ndim == 1 else x.shape[1]), name
    p = str(tmp_path / "odd_chunk.wav")                                        # a LIST chunk of odd length in front of the data
    raw = open(str(tmp_path / "float_mono.wav"), "rb").read()
    i = raw.index(b"data")
    open(p, "wb").write(raw[:i] + b"LIST" + (3).to_bytes(4, "little") + b"abc\0" + raw[i:])
    assert wav_info(p) == (1234, 1, 22050) and read_wav(p)[0].shape[0] == 1234
    with pytest.raises(_lib.UseHipError):
        wav_info(str(tmp_path / "missing.wav"))
    open(str(tmp_path / "not.wav"), "wb").write(b"hello, this is no wave file")
    with pytest.raises(_lib.UseHipError):
        wav_info(str(tmp_path / "not.wav"))


# ---- the bucketing loader --------------------------------------------------------------------------------------------------------
LENS = [12000, 9600, 4000, 9600, 10240, 10239, 30000, 600, 20480, 4001, 9600]   # at 24 kHz; file 5 is written at 48 kHz with 2 x as many


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    d = tmp_path_factory.mktemp("own_length")
    src = d / "in"
    (src / "sub").mkdir(parents=True)
    rng = np.random.RandomState(3)
    for i, L in enumerate(LENS):
        sr, n = (48000, 2 * L) if i == 5 else (24000, L)
        write_wav(str((src / "sub" if i % 3 == 0 else src) / f"u{i:02d}.wav"), (rng.randn(n) * 0.1).astype(np.float32), sr, FLOAT32)
    return str(src), str(d / "out")


def _tp(L, hop=160):
    return (1 + L // hop + 63) // 64 * 64


@pytest.mark.parametrize("world,rank", [(1, 0), (2, 0), (2, 1)])
@pytest.mark.parametrize("batch_size", [1, 3, 4])
def test_bucketed_batches_cover_the_shard_and_never_mix_frame_counts(folder, world, rank, batch_size):
    src, dst = folder
    plain = LoadWavData(src, dst, batch_size=batch_size, rank=rank, world_size=world)
    data = LoadWavData(src, dst, batch_size=batch_size, rank=rank, world_size=world, bucket_by_length=True)
    all_files = sorted(os.path.join(r, n) for r, _, ns in os.walk(src) for n in ns)
    assert data.filepaths == plain.filepaths == shard_list(all_files, rank, world)      # the rank's file set does not change
    batches = data.batch_files(frame_hop=160)
    flat = [p for b in batches for p in b]
    assert sorted(flat) == sorted(data.filepaths) and len(set(flat)) == len(flat)       # a disjoint cover
    tp_of = {p: _tp(LENS[int(os.path.basename(p)[1:3])]) for p in flat}
    for b in batches:
        assert 1 <= len(b) <= batch_size
        assert len({tp_of[p] for p in b}) == 1, [tp_of[p] for p in b]
    keys = [(tp_of[p], os.path.relpath(p, src).replace(os.sep, "/")) for p in flat]
    assert keys == sorted(keys)                                                          # ordered by (T', relative path)
    for a, b in zip(batches, batches[1:]):                                               # cut only where T' changes or a batch is full
        assert tp_of[a[0]] != tp_of[b[0]] or len(a) == batch_size
    assert data.batch_files(frame_hop=160) == batches                                    # identical on two calls
    # what the loader then yields: the decoded lengths give the T' the headers promised
    got = list(data.predict_batches(device="cpu", frame_hop=160))
    assert [b["audio_path"] for b in got] == batches
    for b in got:
        assert {_tp(int(L)) for L in b["sample_length"]} == {tp_of[b["audio_path"][0]]}
        assert b["perturbed"].shape == (len(b["name"]), int(b["sample_length"].max()))


def test_without_the_flag_the_batches_are_todays(folder):
    src, dst = folder
    data = LoadWavData(src, dst, batch_size=4)
    assert data.bucket_by_length is False
    want = [data.filepaths[i:i + 4] for i in range(0, len(data.filepaths), 4)]
    assert data.batch_files() == want == data.batch_files(frame_hop=160)
    for kw in ({}, {"frame_hop": 160}):
        got = list(data.predict_batches(device="cpu", **kw))
        assert [b["audio_path"] for b in got] == want
        for b in got:
            assert b["perturbed"].shape[1] == int(b["sample_length"].max())
            for k, p in enumerate(b["audio_path"]):
                x = torch.from_numpy(load_utterance(p, 24000, True)[0])
                assert torch.equal(b["perturbed"][k, : len(x)], x) and not b["perturbed"][k, len(x):].any()


def test_bucketing_needs_the_frame_hop(folder):
    src, dst = folder
    data = LoadWavData(src, dst, batch_size=4, bucket_by_length=True)
    with pytest.raises(ValueError, match="frame_hop"):
        next(iter(data.predict_batches(device="cpu")))
    from universal_speech_enhancement_amd import predict as P
    assert P.compose([])["data"]["bucket_by_length"] is False
    assert P.compose(["data.bucket_by_length=true"])["data"]["bucket_by_length"] is True


# ---- the frame counts of the mixed-length measurement ----------------------------------------------------------------------------
def test_frame_counts_of_the_mixed_length_measurement():
    spec = importlib.util.spec_from_file_location("mixed_length_predict", os.path.join(ROOT, "scripts", "mixed_length_predict.py"))
    mlp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mlp)
    # the example of the issue: one 4 s file and seven 2 s files at hop 160
    assert mlp.frame_counts([96000] + [48000] * 7, 8) == (640 + 7 * 320, 8 * 640)
    lens = mlp.lengths(64, 0)
    assert len(lens) == 64 and min(lens) >= 24000 and max(lens) < 8 * 24000 and lens == mlp.lengths(64, 0)
    own, padded = mlp.frame_counts(lens, 8)
    g = _glue()
    # own-length: what last_groups reports, [(T', items)], summed over the batches of any loader
    assert own == sum(Tp * len(idx) for Tp, idx in g.length_groups(lens))
    assert padded == sum(len(lens[i:i + 8]) * max(Tp for Tp, _ in g.length_groups(lens[i:i + 8])) for i in range(0, 64, 8))
    assert own < padded
    print(f"[derived] 64 files uniform 1-8 s, batch 8: {padded} padded frames by batch, {own} at own length, ratio {padded / own:.3f}")


# ---- argument errors that need no device -----------------------------------------------------------------------------------------
def test_library_exports_the_own_length_entry_points():
    L = C.CDLL(_lib.LIB_PATH)
    for name, nargs in (("use_stft_fwd_items", 12), ("use_istft_back_items", 12), ("use_wav_info", 4), ("use_resampled_length", 3),
                        ("use_forward_items", 6)):
        assert hasattr(L, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs


def test_invalid_arguments_are_refused_before_anything_is_launched():
    """Every refusal comes before the first HIP call; the pointers below are never dereferenced."""
    L = _lib.lib()
    P = C.c_void_p(4096)                                                       # non-null stand-in for a device pointer
    ok = (C.c_int * 2)(9600, 4000)

    def fwd(wav=P, stride=9600, lens=ok, Y=P, B=2, n_fft=1022, hop=160, win=P, Tpad=64):
        return L.use_stft_fwd_items(wav, stride, lens, Y, B, n_fft, hop, win, Tpad, 0.15, 0.5, None)

    def back(X=P, wav=P, stride=9600, lens=ok, B=2, n_fft=1022, hop=160, win=P, Tpad=64):
        return L.use_istft_back_items(X, wav, stride, lens, B, n_fft, hop, win, Tpad, 0.15, 0.5, None)

    for call, nulls in ((fwd, ("wav", "Y", "win", "lens")), (back, ("X", "wav", "win", "lens"))):
        for name in nulls:
            assert call(**{name: None}) == -1, name                            # USE_E_INVALID
            assert {"win": b"window", "lens": b"len_host"}.get(name, name.encode()) in L.use_last_error(), L.use_last_error()
        assert call(B=0) == -1 and b"B=0" in L.use_last_error()
        assert call(n_fft=1021) == -1 and b"n_fft=1021" in L.use_last_error()
        assert call(lens=(C.c_int * 2)(9600, 511)) == -1 and b"len[1]=511" in L.use_last_error()          # <= n_fft / 2
        assert call(lens=(C.c_int * 2)(9601, 4000)) == -1 and b"len[0]=9601" in L.use_last_error() and b"stride" in L.use_last_error()
        assert call(lens=(C.c_int * 2)(4000, 10240), stride=10240) == -1 and b"len[1]=10240" in L.use_last_error() \
            and b"Tpad" in L.use_last_error()                                                                 # 65 frames > Tpad = 64
    assert L.use_forward_items(None, P, None, None, P, None) == -1 and b"null handle" in L.use_last_error()
