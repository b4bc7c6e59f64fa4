"""CPU-only checks of the convergence losses: the two entry points in the header, the library and the ctypes table; the host-side
refusals of ``use_spec_losses_workspace`` / ``use_spec_losses`` (nothing is launched) and of the Python surface; and the fixture
``tests/golden/spec_losses.npz`` (the reference's own ``WavSpecConvergence_Loss`` in float32, scripts/gen_golden_spec_losses.py) against
the float64 restatement in ``spec_losses_ref.py`` - which the GPU tests then lean on - with the conditioning the fixture's inputs were
chosen for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import spec_losses_ref as sl
from universal_speech_enhancement_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("use_spec_losses_workspace", "use_spec_losses")
CASE_NAMES = [c[0] for c in sl.CASES]


@pytest.fixture(scope="module")
def golden():
    return np.load(sl.GOLDEN)


@pytest.fixture(scope="module")
def restated(golden):
    """The float64 restatement on every item of the fixture, once: {case: [B, 15]}."""
    out = {}
    for case, rate, B, stride, lengths in sl.CASES:
        c = sl.load_case(golden, case)
        out[case] = np.stack([sl.item_values(c["est"][b, :L], c["clean"][b, :L], rate) for b, L in enumerate(lengths)])
    return out


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "use_hip.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in use_hip.h"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS
    assert all(f"USE_SPECLOSS_{k}" in header for k in ("WAV_L1 = 0", "MAG_L2 = 1", "MAG_LOG = 5", "MAG_NORM = 9", "MEL_LOG = 13",
                                                      "MEL_L2 = 14", "COUNT = 15"))
    assert _lib.SYMBOLS["use_spec_losses_workspace"][0] is C.c_size_t
    from universal_speech_enhancement_amd import losses
    assert (losses.WAV_L1, losses.MAG_L2, losses.MAG_LOG, losses.MAG_NORM, losses.MEL_LOG, losses.MEL_L2, losses.COUNT) == (0, 1, 5, 9, 13, 14, 15)
    assert losses.NAMES == sl.TERMS


def test_workspace_is_zero_for_bad_arguments_and_grows_with_the_batch():
    L = _lib.lib()
    for B, stride, rate in ((0, 4096, 24000), (-1, 4096, 24000), (65536, 4096, 24000), (3, 0, 24000), (3, -5, 24000), (3, 4096, 16000),
                            (3, 4096, 44100), (3, 4096, 0)):
        assert L.use_spec_losses_workspace(B, stride, rate) == 0, (B, stride, rate)
    one, three = L.use_spec_losses_workspace(1, 4096, 24000), L.use_spec_losses_workspace(3, 4096, 24000)
    assert 0 < one < three and three % 8 == 0
    assert L.use_spec_losses_workspace(1, 24000, 24000) > one
    assert L.use_spec_losses_workspace(1, 1 << 33, 48000) > 0     # a 64-bit stride is a stride


def test_refusals_name_the_argument_and_launch_nothing():
    """Host-only: every check is in front of the first launch, so host memory stands in for the device buffers."""
    L = _lib.lib()
    buf = np.zeros(8, np.float64)
    p = buf.ctypes.data

    def call(est=p, clean=p, lens=(4096,), B=1, stride=4096, rate=24000, work=p, nbytes=1 << 40, out=p):
        arr = (C.c_int * max(len(lens), 1))(*lens) if lens is not None else None
        return L.use_spec_losses(est, clean, arr, B, stride, rate, work, nbytes, out, None)

    for kw, word in ((dict(rate=16000), b"sampling_rate=16000"), (dict(rate=44100), b"sampling_rate=44100"), (dict(B=0), b"B=0"),
                     (dict(B=65536), b"B=65536"), (dict(stride=0), b"stride=0"), (dict(est=None), b"est"), (dict(clean=None), b"clean"),
                     (dict(lens=None), b"len_host"), (dict(work=None), b"work"), (dict(out=None), b"out_dev"),
                     (dict(lens=(1024,)), b"len[0]=1024"), (dict(lens=(4097,)), b"len[0]=4097"),
                     (dict(lens=(4096, 100), B=2), b"len[1]=100"), (dict(lens=(2048,), rate=48000), b"len[0]=2048"),
                     (dict(nbytes=L.use_spec_losses_workspace(1, 4096, 24000) - 1), b"work_bytes")):
        assert call(**kw) == -1, kw                                # USE_E_INVALID
        assert word in L.use_last_error(), (kw, L.use_last_error())


def test_python_surface_refuses_what_it_cannot_run():
    import torch
    from universal_speech_enhancement_amd import losses
    x = torch.zeros(2, 4096)
    with pytest.raises(_lib.UseHipError, match="CUDA"):            # no CPU implementation, no quiet fall-back
        losses.spec_loss_terms(x, x)
    with pytest.raises(_lib.UseHipError, match="CUDA"):
        losses.WavSpecConvergence_Loss(sampling_rate=24000)({"clean": x, "fake": x})
    with pytest.raises(TypeError, match="float32"):
        losses.spec_loss_terms(x.double(), x.double())
    with pytest.raises(TypeError, match="Tensor"):
        losses.spec_loss_terms(x.numpy(), x)
    with pytest.raises(ValueError, match="shape"):
        losses.spec_loss_terms(x.reshape(2, 2, 2048), x)
    with pytest.raises(ValueError, match="shape"):
        losses.convergence_losses(x, x[:1])
    with pytest.raises(ValueError, match="sampling_rate"):
        losses.spec_loss_terms(x, x, sampling_rate=16000)
    assert losses.min_length(24000) == sl.min_length(24000) == 1025 and losses.min_length(48000) == sl.min_length(48000) == 2049
    for bad, rate in (([1024, 4096], 24000), ([4096, 4097], 24000), ([4096], 24000), ([2048, 4096], 48000)):
        with pytest.raises(ValueError, match="lengths"):
            losses._lengths(bad, 2, 4096, rate)
    assert losses._lengths(None, 2, 4096, 24000).tolist() == [4096, 4096] and losses._lengths([1025, 4096], 2, 4096, 24000).dtype == np.int32
    assert losses.LSGAN_ALPHAS == dict(alpha_wav_l1=0.1, alpha_mag_l2=1.0, alpha_mag_log=1.0, alpha_mag_norm_l2=0.5, alpha_mel_log=0.5,
                                       alpha_mel_l2=0.5)


def test_predict_refuses_the_option_without_a_clean_folder():
    from universal_speech_enhancement_amd import predict as P
    with pytest.raises(SystemExit, match="clean_folder"):
        P.predict(P.compose(["model=SGMSE_Large", "data.convergence_losses=true", "random_init_seed=1"]))
    assert P.compose([])["data"].get("convergence_losses") in (None, False)


@pytest.mark.parametrize("case", CASE_NAMES)
def test_restatement_reproduces_the_fixture(golden, restated, case):
    """Per term within 4 x the stored ``f32_vs_f64`` (the LSD test's convention): the fixture's values are the reference's float32
    evaluation, the stored figure its distance to the same modules in float64, and this restatement is a second float64 evaluation."""
    c = sl.load_case(golden, case)
    _, rate, B, stride, lengths = next(x for x in sl.CASES if x[0] == case)
    assert c["est"].shape == (B, stride) and c["est"].dtype == np.float32 and tuple(c["lengths"]) == lengths
    assert c["ref_f32"].shape == c["f32_vs_f64"].shape == (B, 6)
    got = sl.six_terms(restated[case])
    for b, L in enumerate(lengths):
        assert not c["est"][b, L:].any() and not c["clean"][b, L:].any()                 # zero padding
        e, s = sl.signals(case, b, L, rate)
        assert np.array_equal(e, c["est"][b, :L]) and np.array_equal(s, c["clean"][b, :L])   # the recipe gives the stored signals
        d, bound = np.abs(got[b] - c["ref_f32"][b]), c["f32_vs_f64"][b]
        print(f"{case}[{b}]: off by {d} (relative {d / np.abs(c['ref_f32'][b])}), stored f32 vs f64 {bound}")
        assert (bound > 0).all() and (d <= 4 * bound).all()


@pytest.mark.parametrize("case", CASE_NAMES)
def test_fixture_is_well_conditioned(golden, case):
    c = sl.load_case(golden, case)
    _, rate, _, _, lengths = next(x for x in sl.CASES if x[0] == case)
    for b, L in enumerate(lengths):
        for x in (c["est"][b, :L], c["clean"][b, :L]):
            for M in sl.maps(x, rate):
                assert M.min() >= sl.MAG_FLOOR and np.mean(1.0 / M) <= sl.INV_MEAN_CAP, (case, b, M.min(), np.mean(1.0 / M))
    assert os.path.getsize(sl.GOLDEN) < 1 << 20


def test_aggregation_to_the_six_terms_and_to_the_batch_value(golden, restated):
    """``six_terms``: mag_l2 is the SUM over the resolutions, mag_log and mag_norm_l2 their means.  The reference's value for the ``edge``
    batch at full width (every row evaluated over all 4096 samples, zero padding included) is the mean over the items of the per-item
    terms, and its ``loss_G`` their sum: within 4 x the stored float32-against-float64 distance of that batch run."""
    v = np.arange(15, dtype=np.float64)
    assert sl.six_terms(v).tolist() == [0.0, 1 + 2 + 3 + 4, (5 + 6 + 7 + 8) / 4, (9 + 10 + 11 + 12) / 4, 13.0, 14.0]
    c = sl.load_case(golden, "edge")
    full = sl.six_terms(np.stack([sl.item_values(e, s, 24000) for e, s in zip(c["est"], c["clean"])])).mean(axis=0)
    got, want, bound = np.append(full, full.sum()), golden["edge_batch"], golden["edge_batch_f32_vs_f64"]
    print(f"edge at full width: {got}, reference {want}, off by {np.abs(got - want)}, stored f32 vs f64 {bound}")
    assert want.shape == (7,) and (np.abs(got - want) <= 4 * bound).all()
    # trimmed to its length an item is another signal: the last item is at full width in both
    assert np.array_equal(sl.six_terms(restated["edge"][3]), sl.six_terms(sl.item_values(c["est"][3], c["clean"][3], 24000)))
