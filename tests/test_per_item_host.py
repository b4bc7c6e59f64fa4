"""CPU-only checks of batch-invariant (``per_item``) sampling: the two entry points are exported and bound, the seed derivation is
SplitMix64 as published, the chunked loop hands window k of item b the same seed whatever ``chunk_batch`` is, and the argument errors
that need no device."""
import ctypes as C

import numpy as np
import pytest
import torch

import chunk_ref as cr
from universal_speech_enhancement_amd import _lib
from universal_speech_enhancement_amd import seeding as sg
from universal_speech_enhancement_amd.sgmse import sampling
from universal_speech_enhancement_amd.sgmse.model_wrapper import ScoreModel
from universal_speech_enhancement_amd.sgmse.sdes import OUVESDE


def test_library_exports_the_per_item_entry_points():
    L = C.CDLL(_lib.LIB_PATH)
    for name, nargs in (("use_sample_items", 8), ("use_fill_noise_items", 7)):
        assert hasattr(L, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs
    assert _lib.SYMBOLS["use_sample_items"][1][5] == C.POINTER(C.c_uint64)          # seeds_host
    assert _lib.SYMBOLS["use_fill_noise_items"][1][1] == C.POINTER(C.c_uint64)


def test_null_seeds_and_null_noise_are_invalid_without_a_device():
    """The refusal comes before the handle is looked at, so it needs neither a plan nor a GPU."""
    L = _lib.lib()
    assert L.use_sample_items(None, None, None, None, None, None, None, None) == -1            # USE_E_INVALID
    assert b"seeds" in L.use_last_error()
    seeds = (C.c_uint64 * 2)(1, 2)
    assert L.use_fill_noise_items(None, None, 2, 0, None, 4, None) == -1
    assert L.use_fill_noise_items(None, seeds, 2, 0, seeds, 5, None) == -1                      # n is no multiple of B
    assert L.use_fill_noise_items(None, seeds, 2, -1, seeds, 4, None) == -1


def test_splitmix64_published_vectors():
    assert sg.splitmix64(0) == 0xE220A8397B1DCDAF
    assert sg.splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    # the generator form: state += gamma per output, i.e. output k of seed 0 is splitmix64(k * gamma)
    assert sg.splitmix64(2 * 0x9E3779B97F4A7C15) == 0x06C45D188009454F


def test_derived_seeds_are_deterministic_64_bit_and_distinct():
    assert sg.item_seed(7, 3) == sg.splitmix64(7 ^ sg.splitmix64(3)) == sg.item_seed(7, 3)
    assert sg.window_seed(11, 2) == sg.splitmix64(14) == sg.window_seed(11, 2)
    assert sg.window_seed(2**64 - 1, 0) == sg.splitmix64(0)                           # the sum wraps at 64 bits
    assert sg.item_seeds(5, 4) == [sg.item_seed(5, b) for b in range(4)]
    paths = [f"speaker{i % 37}/utt_{i:04d}.wav" for i in range(1000)]
    for vals in ([sg.item_seed(42, k) for k in range(1000)], [sg.path_key(p) for p in paths],
                 [sg.item_seed(42, sg.path_key(p)) for p in paths], [sg.window_seed(sg.item_seed(42, 0), k) for k in range(1000)]):
        assert all(isinstance(v, int) and 0 <= v < 2**64 for v in vals)
        assert len(set(vals)) == 1000
    assert sg.item_seed(1, 5) != sg.item_seed(2, 5)
    assert sg.path_key("a/b.wav") == sg.path_key("a/b.wav")


def test_path_key_is_blake2b_of_the_posix_path():
    import hashlib
    import pathlib
    want = int.from_bytes(hashlib.blake2b("dir/sub/ü.wav".encode("utf-8")).digest()[:8], "little")
    assert sg.path_key("dir/sub/ü.wav") == want
    assert sg.path_key("dir\\sub\\ü.wav") == want                                     # the OS separator does not matter
    assert sg.path_key(pathlib.PurePosixPath("dir/sub/ü.wav")) == want
    assert sg.path_key(pathlib.PureWindowsPath("dir\\sub\\ü.wav")) == want


@pytest.fixture
def host_chunks(monkeypatch):
    import universal_speech_enhancement_amd.hip_engine as he
    monkeypatch.setattr(he, "chunk_split", lambda Y, Cf, ov: torch.from_numpy(cr.ref_split(Y.numpy(), Cf, ov)))
    monkeypatch.setattr(he, "chunk_merge", lambda ch, B, Tp, Cf, ov: torch.from_numpy(cr.ref_merge(ch.numpy(), B, Tp, Cf, ov)[0].astype(np.complex64)))
    rng = np.random.default_rng(0)
    return torch.from_numpy((rng.standard_normal((2, 1, 5, 192)) + 1j * rng.standard_normal((2, 1, 5, 192))).astype(np.complex64))


def test_chunked_windows_get_the_same_seed_at_any_chunk_batch(host_chunks, monkeypatch):
    """A recording stand-in for the sampler: with per_item the seed that reaches window k of item b is window_seed(item_seeds[b], k)
    for chunk_batch 1, 3 and 8; without it the groups sample with seed + g, as before."""
    Y = host_chunks
    m = ScoreModel(backbone="none", condition="noisy", sde_input="noisy", n_fft=1022, hop_length=160, num_frames=512)
    calls = []

    def fake_pc(predictor, corrector, y, N=None, **kw):
        def sampler():
            calls.append((y.shape[0], kw["seed"], kw.get("per_item", False), kw.get("item_seeds")))
            return y * 2, 4
        return sampler
    monkeypatch.setattr(m, "get_pc_sampler", fake_pc)
    S = [0x1234, 0xFFFFFFFFFFFFFFF0]
    want = [sg.window_seed(S[b], k) for b in range(2) for k in range(4)]              # [2,1,5,192] at C = 64, overlap 16: 4 windows per item
    for cb in (1, 3, 8):
        calls.clear()
        m.sample_spec_chunked(Y, [Y], N=2, seed=10, chunk_frames=64, chunk_overlap=16, chunk_batch=cb, per_item=True, item_seeds=S)
        assert [c[0] for c in calls] == [min(cb, 8 - lo) for lo in range(0, 8, cb)]
        assert all(c[2] is True for c in calls)
        assert [s for c in calls for s in c[3]] == want, cb
    calls.clear()                                                                     # item_seeds default: item_seed(seed, b)
    m.sample_spec_chunked(Y, [Y], N=2, seed=10, chunk_frames=64, chunk_overlap=16, chunk_batch=3, per_item=True)
    assert [s for c in calls for s in c[3]] == [sg.window_seed(sg.item_seed(10, b), k) for b in range(2) for k in range(4)]
    calls.clear()                                                                     # one window: the items' own seeds
    short = Y[..., :64].contiguous()
    m.sample_spec_chunked(short, [short], N=2, seed=10, chunk_frames=64, chunk_overlap=16, per_item=True, item_seeds=S)
    assert calls == [(2, 10, True, S)]
    calls.clear()                                                                     # the default rule is untouched
    m.sample_spec_chunked(Y, [Y], N=2, seed=10, chunk_frames=64, chunk_overlap=16, chunk_batch=3)
    assert calls == [(3, 10, False, None), (3, 11, False, None), (2, 12, False, None)]
    with pytest.raises(ValueError, match="item_seeds"):
        m.sample_spec_chunked(Y, [Y], N=2, chunk_frames=64, chunk_overlap=16, per_item=True, item_seeds=[1])
    with pytest.raises(ValueError, match="per_item"):
        m.sample_spec_chunked(Y, [Y], N=2, chunk_frames=64, chunk_overlap=16, item_seeds=S)


def test_minibatches_keep_the_seed_of_the_item_not_of_its_slot(monkeypatch):
    m = ScoreModel(backbone="none", condition="noisy", sde_input="noisy", n_fft=1022, hop_length=160, num_frames=512)
    seen = []
    monkeypatch.setattr(sampling, "get_pc_sampler", lambda p, c, sde, score_fn, y, **kw: (seen.append(kw.get("item_seeds")), lambda: (y, 1))[1])
    Y = torch.zeros((5, 1, 5, 64), dtype=torch.complex64)
    m.get_pc_sampler("reverse_diffusion", "langevin", Y, N=2, minibatch=2, conditioning=[Y], per_item=True, seed=3)()
    assert seen == [[sg.item_seed(3, 0), sg.item_seed(3, 1)], [sg.item_seed(3, 2), sg.item_seed(3, 3)], [sg.item_seed(3, 4)]]
    seen.clear()
    m.get_pc_sampler("reverse_diffusion", "langevin", Y, N=2, minibatch=2, conditioning=[Y], seed=3)()
    assert seen == [None, None, None]


def test_per_item_refuses_what_stays_batch_coupled():
    from universal_speech_enhancement_amd.sgmse.sampling import CorrectorRegistry
    from universal_speech_enhancement_amd.sgmse.sampling.correctors import LangevinCorrector
    name = "per_item_host_test_corrector"
    if name not in getattr(CorrectorRegistry, "_registry", {}):
        try:
            CorrectorRegistry.register(name=name)(type("UserCorrector", (LangevinCorrector,), {}))
        except Exception:            # registered by an earlier run in this process
            pass
    m = ScoreModel(backbone="none", condition="noisy", sde_input="noisy", n_fft=1022, hop_length=160, num_frames=512)
    Y = torch.zeros((3, 1, 5, 64), dtype=torch.complex64)
    with pytest.raises(NotImplementedError, match="batch-coupled"):
        sampling.get_pc_sampler("reverse_diffusion", name, OUVESDE(N=2), m, Y, conditioning=[Y], per_item=True)
    with pytest.raises(NotImplementedError, match="batch-coupled"):
        m.get_pc_sampler("reverse_diffusion", name, Y, N=2, conditioning=[Y], per_item=True)
    assert callable(sampling.get_pc_sampler("reverse_diffusion", name, OUVESDE(N=2), m, Y, conditioning=[Y]))     # the seam path itself stays
    with pytest.raises(NotImplementedError, match="fused"):                           # a score_fn that is not the HIP-backed model
        sampling.get_pc_sampler("reverse_diffusion", "langevin", OUVESDE(N=2), lambda *a, **k: None, Y, conditioning=[Y], per_item=True)
    with pytest.raises(ValueError, match="minibatch=1"):
        m.get_ode_sampler(Y, N=2, conditioning=[Y], per_item=True, minibatch=2)
    with pytest.raises(ValueError, match="minibatch=1"):
        sampling.get_ode_sampler(OUVESDE(N=2), m, Y, conditioning=[Y], per_item=True)   # minibatch=None: one controller for the batch
    with pytest.raises(ValueError, match="item_seeds"):
        sampling.get_pc_sampler("reverse_diffusion", "langevin", OUVESDE(N=2), m, Y, conditioning=[Y], per_item=True, item_seeds=[1, 2])
    with pytest.raises(ValueError, match="per_item"):
        sampling.get_pc_sampler("reverse_diffusion", "langevin", OUVESDE(N=2), m, Y, conditioning=[Y], item_seeds=[1, 2, 3])
    assert callable(sampling.get_pc_sampler("reverse_diffusion", "langevin", OUVESDE(N=2), m, Y, conditioning=[Y], per_item=True))
    assert callable(m.get_ode_sampler(Y, N=2, conditioning=[Y], per_item=True, minibatch=1))


def test_predict_step_names_the_noise_by_the_relative_path(monkeypatch, tmp_path):
    """model.sampler_kwargs.per_item: item_seed(S, path_key(path relative to data_folder)), whatever the batch order and the folder."""
    import os

    from universal_speech_enhancement_amd.SGMSE_module import SGMSEModule
    seen = []

    class Score(torch.nn.Module):
        def sample(self, batch, **kw):
            seen.append(kw)
            batch["enhanced"] = torch.zeros((len(batch["audio_path"]), 8))
            return batch

    def batch_of(folder, rels):
        return {"audio_path": [os.path.join(folder, *r.split("/")) for r in rels], "data_folder": folder, "target_folder": str(tmp_path / "out"),
                "sample_length": [8] * len(rels), "sampling_rate": [16000] * len(rels)}
    monkeypatch.setattr("universal_speech_enhancement_amd.SGMSE_module._write_wav", lambda *a, **k: None)
    mod = SGMSEModule(Score(), sampler_kwargs={"per_item": True, "seed": 9, "N": 2})
    rels = ["a/x.wav", "b/y.wav", "z.wav"]
    mod.predict_step(batch_of(str(tmp_path / "in1"), rels))
    mod.predict_step(batch_of(str(tmp_path / "elsewhere" / "in2"), rels[::-1]))
    want = [sg.item_seed(9, sg.path_key(r)) for r in rels]
    assert seen[0]["item_seeds"] == want and seen[1]["item_seeds"] == want[::-1]
    assert seen[0]["per_item"] is True and seen[0]["seed"] == 9 and seen[0]["N"] == 2
    seen.clear()
    SGMSEModule(Score(), sampler_kwargs={"N": 2}).predict_step(batch_of(str(tmp_path / "in1"), rels))
    assert seen == [{"N": 2}]                                                         # off by default
