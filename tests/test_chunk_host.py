"""CPU-only checks of chunked sampling: the window geometry in its two mirrors (``chunking.chunk_plan`` and ``use_chunk_count``
through ctypes), the arguments both refuse, the partition of unity of the cross-fade weights in float64 - which pins the weight
definition the GPU tests use as their reference - and the path of the keys from the predict command line."""
import numpy as np
import pytest

import chunk_ref as cr
from universal_speech_enhancement_amd import _lib
from universal_speech_enhancement_amd.chunking import check_chunk_batch, chunk_groups, chunk_plan

ALL_CASES = cr.CASES + [cr.ODD_HOP]


@pytest.mark.parametrize("Tp,C,overlap", ALL_CASES)
def test_chunk_plan_and_use_chunk_count_agree(Tp, C, overlap):
    L = _lib.lib()
    n, starts = cr.ref_plan(Tp, C, overlap)
    p = chunk_plan(Tp, C, overlap)
    assert L.use_chunk_count(Tp, C, overlap) == p.n == n
    assert list(p.starts) == starts and p.hop == C - overlap and (p.chunk_frames, p.overlap, p.Tp) == (C, overlap, Tp)
    assert starts[-1] + C >= Tp                                  # the windows reach the last frame
    assert n == 1 or starts[-1] + overlap < Tp                   # and the last one owns at least one frame


def test_the_named_geometries():
    assert chunk_plan(64, 64, 16).n == 1 and chunk_plan(64, 128, 64).n == 1             # Tp <= C: no chunking
    assert chunk_plan(128, 64, 16).starts == (0, 48, 96)
    p = chunk_plan(192, 64, 16)
    assert p.starts == (0, 48, 96, 144) and p.starts[-1] + 64 - 192 == 16                # the last window runs 16 frames past Tp
    assert chunk_plan(192, 64, 0).starts == (0, 64, 128)
    assert chunk_plan(192, 64, 32).starts == (0, 32, 64, 96, 128)
    assert _lib.lib().use_chunk_count(64, 128, 64) == 1


@pytest.mark.parametrize("args,name", [((192, 100, 16), "chunk_frames"),     # C not a multiple of 64
                                       ((192, 0, 0), "chunk_frames"),
                                       ((192, -64, 0), "chunk_frames"),      # negative values
                                       ((192, 64, 33), "overlap"),           # overlap > C / 2
                                       ((192, 64, -1), "overlap"),
                                       ((100, 64, 16), "Tp"),
                                       ((-64, 64, 16), "Tp")])
def test_bad_arguments_are_an_error_code_and_a_value_error(args, name):
    L = _lib.lib()
    assert L.use_chunk_count(*args) == -1                                     # USE_E_INVALID, no abort
    assert name.encode() in L.use_last_error(), L.use_last_error()
    with pytest.raises(ValueError, match=name):
        chunk_plan(*args)
    # the device entry points check the geometry before they touch a pointer (host-only call: nothing is launched)
    dummy = np.zeros(4, np.complex64).ctypes.data
    assert L.use_chunk_split(dummy, dummy, 1, 3, *args, None) == -1 and name.encode() in L.use_last_error()
    assert L.use_chunk_merge(dummy, dummy, 1, 3, *args, None) == -1 and name.encode() in L.use_last_error()


def test_other_refusals():
    L = _lib.lib()
    dummy = np.zeros(4, np.complex64).ctypes.data
    assert L.use_chunk_split(None, dummy, 1, 3, 192, 64, 16, None) == -1
    assert L.use_chunk_merge(dummy, dummy, 0, 3, 192, 64, 16, None) == -1 and b"B=0" in L.use_last_error()
    with pytest.raises(ValueError, match="chunk_frames"):
        chunk_plan(192, 64.0, 16)
    with pytest.raises(ValueError, match="chunk_batch"):
        chunk_groups(4, 0)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="chunk_batch"):
            check_chunk_batch(bad)
    assert check_chunk_batch(np.int64(3)) == 3
    assert chunk_groups(5, 2) == [(0, 2), (2, 4), (4, 5)]                     # the last group may be smaller


@pytest.mark.parametrize("Tp,C,overlap", ALL_CASES)
def test_partition_of_unity(Tp, C, overlap):
    rng = np.random.default_rng(Tp * 1000 + C + overlap)
    for B, F in ((1, 3), (3, 5)):
        Y = rng.standard_normal((B, 1, F, Tp)) + 1j * rng.standard_normal((B, 1, F, Tp))
        chunks = cr.ref_split(Y, C, overlap)
        n = cr.ref_plan(Tp, C, overlap)[0]
        assert chunks.shape == (B * n, 1, F, C)
        X, bound = cr.ref_merge(chunks, B, Tp, C, overlap)
        assert np.abs(X - Y).max() <= 1e-15
        assert ((bound[0, 0, 0, :, 0] > 0) == cr.overlap_mask(Tp, C, overlap)).all()


def test_merge_reference_weights():
    """Two constant windows: the merged overlap is the ramp (j + 1) / (overlap + 1) itself."""
    C, overlap, Tp = 64, 16, 112
    chunks = np.zeros((2, 1, 1, C), np.complex128)
    chunks[1] = 1.0
    X, _ = cr.ref_merge(chunks, 1, Tp, C, overlap)
    np.testing.assert_allclose(X[0, 0, 0, 48:64].real, (np.arange(16) + 1) / 17, rtol=0, atol=1e-16)
    assert (X[0, 0, 0, :48] == 0).all() and (X[0, 0, 0, 64:] == 1).all()


def test_predict_overrides_carry_the_chunk_keys_as_integers():
    from universal_speech_enhancement_amd.predict import compose
    cfg = compose(["model.sampler_kwargs.chunk_frames=512", "model.sampler_kwargs.chunk_overlap=64"])
    kw = cfg["model"]["sampler_kwargs"]
    assert kw == {"chunk_frames": 512, "chunk_overlap": 64} and all(type(v) is int for v in kw.values())
    cfg = compose(["model=LSGAN", "model.sampler_kwargs.chunk_frames=512"])
    assert cfg["model"]["sampler_kwargs"] == {"chunk_frames": 512}


def test_keywords_exist_with_chunking_off_by_default():
    import inspect

    from universal_speech_enhancement_amd.gan.ncsnpp_wrapper import NCSNPP_Wrapper
    from universal_speech_enhancement_amd.sgmse.model_wrapper import ScoreModel
    for fn in (ScoreModel.sample, ScoreModel.enhance, NCSNPP_Wrapper.forward):
        p = inspect.signature(fn).parameters
        assert p["chunk_frames"].default is None and p["chunk_overlap"].default == 64 and p["chunk_batch"].default == 8


def test_chunked_control_flow_on_the_host(monkeypatch):
    """The loop around the device pieces, with numpy stand-ins for the two kernels and a recording stand-in for the sampler: groups of
    at most chunk_batch consecutive windows, seed + g, the noise sliced per group, `conditioning[0] is y` kept inside a group (the
    engine recognises the SDE's y among the conditioning by identity), and the results merged."""
    import torch

    import universal_speech_enhancement_amd.hip_engine as he
    from universal_speech_enhancement_amd.gan.ncsnpp_wrapper import NCSNPP_Wrapper
    from universal_speech_enhancement_amd.sgmse.model_wrapper import ScoreModel
    monkeypatch.setattr(he, "chunk_split", lambda Y, C, ov: torch.from_numpy(cr.ref_split(Y.numpy(), C, ov)))
    monkeypatch.setattr(he, "chunk_merge", lambda ch, B, Tp, C, ov: torch.from_numpy(cr.ref_merge(ch.numpy(), B, Tp, C, ov)[0].astype(np.complex64)))
    m = ScoreModel(backbone="none", condition="noisy", sde_input="noisy", n_fft=1022, hop_length=160, num_frames=512)
    calls = []

    def fake_pc(predictor, corrector, y, N=None, **kw):
        def sampler():
            calls.append((tuple(y.shape), kw["seed"], None if kw["noise"] is None else tuple(kw["noise"].shape), kw["conditioning"][0] is y))
            return y * 2, 4
        return sampler
    monkeypatch.setattr(m, "get_pc_sampler", fake_pc)
    rng = np.random.default_rng(0)
    Y = torch.from_numpy((rng.standard_normal((2, 1, 5, 192)) + 1j * rng.standard_normal((2, 1, 5, 192))).astype(np.complex64))
    noise = torch.zeros((5, 8, 1, 5, 64), dtype=torch.complex64)                  # [n_draws, B * n = 2 * 4, 1, F, C]
    out = m.sample_spec_chunked(Y, [Y], N=2, noise=noise, seed=10, chunk_frames=64, chunk_overlap=16, chunk_batch=3)
    assert calls == [((3, 1, 5, 64), 10, (5, 3, 1, 5, 64), True), ((3, 1, 5, 64), 11, (5, 3, 1, 5, 64), True),
                     ((2, 1, 5, 64), 12, (5, 2, 1, 5, 64), True)]
    assert m.last_nfe == [4, 4, 4] and float((out - 2 * Y).abs().max()) <= 4 * 2.0 ** -24 * 4 * float(Y.abs().max())
    with pytest.raises(ValueError, match="windows"):
        m.sample_spec_chunked(Y, [Y], N=2, noise=noise[:, :7], chunk_frames=64, chunk_overlap=16)
    # the ODE sampler: the prior's draw [B * n, 1, F, C] is sliced along its first axis, the solver options reach every group
    def fake_ode(y, N=None, **kw):
        def sampler():
            calls.append((tuple(y.shape), kw["seed"], None if kw["noise"] is None else tuple(kw["noise"].shape), kw["conditioning"][0] is y, kw["rtol"]))
            return y * 2, [7] * y.shape[0]
        return sampler
    calls.clear()
    prior = torch.arange(8, dtype=torch.float32).view(8, 1, 1, 1).expand(8, 1, 5, 64).to(torch.complex64)
    seen = []
    monkeypatch.setattr(m, "get_ode_sampler", lambda y, N=None, **kw: (seen.append(kw["noise"][:, 0, 0, 0].real.tolist()), fake_ode(y, N, **kw))[1])
    out = m.sample_spec_chunked(Y, [Y], sampler_type="ode", N=2, noise=prior, seed=20, rtol=1e-3, chunk_frames=64, chunk_overlap=16, chunk_batch=3)
    assert calls == [((3, 1, 5, 64), 20, (3, 1, 5, 64), True, 1e-3), ((3, 1, 5, 64), 21, (3, 1, 5, 64), True, 1e-3),
                     ((2, 1, 5, 64), 22, (2, 1, 5, 64), True, 1e-3)]
    assert seen == [[0, 1, 2], [3, 4, 5], [6, 7]]                                  # window w draws row w of the prior
    assert m.last_nfe == [[7] * 3, [7] * 3, [7] * 2] and float((out - 2 * Y).abs().max()) <= 4 * 2.0 ** -24 * 4 * float(Y.abs().max())
    with pytest.raises(ValueError, match="windows"):
        m.sample_spec_chunked(Y, [Y], sampler_type="ode", N=2, noise=prior[:7], chunk_frames=64, chunk_overlap=16)
    with pytest.raises(TypeError, match="rtol"):
        m.sample_spec_chunked(Y, [Y], N=2, rtol=1e-3, chunk_frames=64, chunk_overlap=16)
    monkeypatch.setattr(m, "get_pc_sampler", fake_pc)
    calls.clear()
    short = Y[..., :64].contiguous()                                               # one window: the sampler on the input as it is
    assert m.sample_spec_chunked(short, [short], N=2, seed=5, chunk_frames=64, chunk_overlap=16) is not None
    assert calls == [((2, 1, 5, 64), 5, None, True)]
    assert (m._chunked(192, None, 64, 8), m._chunked(64, 64, 16, 8), m._chunked(192, 64, 16, 8)) == (False, False, True)
    w = NCSNPP_Wrapper.__new__(NCSNPP_Wrapper)
    torch.nn.Module.__init__(w)
    w.net = lambda x: x * 3
    assert float((w.refine_spec_chunked(Y, 64, 16, 2) - 3 * Y).abs().max()) <= 4 * 2.0 ** -24 * 6 * float(Y.abs().max())
