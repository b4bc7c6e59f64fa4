"""CPU-only checks of device-side STOI / ESTOI: the two entry points in the header, the library and the ctypes table; the host-side
refusals of ``use_stoi_workspace`` / ``use_stoi`` (nothing is launched) and of the Python surface; the float64 restatement in
``stoi_ref.py`` - which the GPU tests lean on - against the definition's fixed points; and the conditioning of every GPU case."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import stoi_ref as sr
from universal_speech_enhancement_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("use_stoi_workspace", "use_stoi")
ITEMS = [(name, b) for name, _, _, items in sr.CASES for b in range(len(items))]


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "use_hip.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in use_hip.h"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS
    assert all(f"USE_STOI_{k}" in header for k in ("STOI = 0", "ESTOI = 1", "FRAMES = 2", "COUNT = 3"))
    assert _lib.SYMBOLS["use_stoi_workspace"][0] is C.c_size_t
    from universal_speech_enhancement_amd import metrics
    assert metrics.STOI_NAMES == ("stoi", "estoi") and metrics.STOI_RATES == sr.RATES and metrics.STOI_MIN_FRAMES == sr.N


def test_workspace_is_zero_for_bad_arguments_and_grows_with_the_batch():
    L = _lib.lib()
    for B, stride, rate in ((0, 9829, 24000), (-1, 9829, 24000), (65536, 9829, 24000), (3, 0, 24000), (3, -5, 24000), (3, 9829, 44100),
                            (3, 9829, 8000), (3, 9829, 0)):
        assert L.use_stoi_workspace(B, stride, rate) == 0, (B, stride, rate)
    one, three = L.use_stoi_workspace(1, 9829, 24000), L.use_stoi_workspace(3, 9829, 24000)
    assert 0 < one < three and three % 8 == 0
    assert L.use_stoi_workspace(1, 36001, 24000) > one
    assert all(L.use_stoi_workspace(1, 9829, r) > 0 for r in sr.RATES)
    assert L.use_stoi_workspace(1, 1 << 33, 48000) > 0             # a 64-bit stride is a stride


def test_refusals_name_the_argument_and_launch_nothing():
    """Host-only: every check is in front of the first launch, so host memory stands in for the device buffers."""
    L = _lib.lib()
    buf = np.zeros(8, np.float64)
    p = buf.ctypes.data

    def call(est=p, clean=p, lens=(9829,), B=1, stride=9829, rate=24000, work=p, nbytes=1 << 40, out=p):
        arr = (C.c_int * max(len(lens), 1))(*lens) if lens is not None else None
        return L.use_stoi(est, clean, arr, B, stride, rate, work, nbytes, out, None)

    for kw, word in ((dict(rate=44100), b"sampling_rate=44100"), (dict(rate=8000), b"sampling_rate=8000"), (dict(B=0), b"B=0"),
                     (dict(B=65536), b"B=65536"), (dict(stride=0), b"stride=0"), (dict(est=None), b"est"), (dict(clean=None), b"clean"),
                     (dict(lens=None), b"len_host"), (dict(work=None), b"work"), (dict(out=None), b"out_dev"),
                     (dict(lens=(9830,)), b"len[0]=9830"), (dict(lens=(9829, 9900), B=2), b"len[1]=9900"),
                     (dict(lens=(612,)), b"len[0]=612"), (dict(lens=(408,), rate=16000), b"len[0]=408"),
                     (dict(lens=(1224,), rate=48000), b"len[0]=1224"), (dict(lens=(255,), rate=10000), b"len[0]=255"),
                     (dict(lens=(9829, 0), B=2), b"len[1]=0"),
                     (dict(nbytes=L.use_stoi_workspace(1, 9829, 24000) - 1), b"work_bytes")):
        assert call(**kw) == -1, kw                                # USE_E_INVALID
        assert word in L.use_last_error(), (kw, L.use_last_error())


def test_python_surface_refuses_what_it_cannot_run():
    import torch
    from universal_speech_enhancement_amd import metrics
    from universal_speech_enhancement_amd.sgmse.util import other
    x = torch.zeros(2, 9829)
    with pytest.raises(_lib.UseHipError, match="CUDA"):            # no CPU implementation, no quiet fall-back
        metrics.stoi(x, x)
    with pytest.raises(_lib.UseHipError, match="CUDA"):
        metrics.intelligibility(x, x)
    with pytest.raises(_lib.UseHipError, match="CUDA"):
        other.stoi(x, x, 24000)
    assert [metrics.stoi_min_length(r) for r in sr.RATES] == [256, 409, 613, 1225]
    assert all(sr.resampled_length(metrics.stoi_min_length(r), r) == 256 and sr.resampled_length(metrics.stoi_min_length(r) - 1, r) == 255
               for r in sr.RATES)
    with pytest.raises(ValueError, match="sampling_rate"):
        metrics.stoi_min_length(44100)


def test_predict_refuses_the_option_without_a_clean_folder():
    from universal_speech_enhancement_amd import predict as P
    with pytest.raises(SystemExit, match="clean_folder"):
        P.predict(P.compose(["model=SGMSE_Large", "data.intelligibility=true", "random_init_seed=1"]))
    assert P.compose([])["data"].get("intelligibility") in (None, False)


def test_write_csv_keeps_its_four_columns_unless_asked(tmp_path):
    from universal_speech_enhancement_amd import metrics
    row = dict(si_sdr=1.0, si_sir=2.0, si_sar=3.0, lsd=4.0, stoi=0.5, estoi=0.25, stoi_frames=31.0)
    metrics.write_csv(str(tmp_path / "a.csv"), [("f.wav", row)])
    metrics.write_csv(str(tmp_path / "b.csv"), [("f.wav", row)], names=metrics.NAMES + metrics.STOI_NAMES)
    assert (tmp_path / "a.csv").read_text().splitlines() == ["file,si_sdr,si_sir,si_sar,lsd", "f.wav,1.0,2.0,3.0,4.0", "mean,1.0,2.0,3.0,4.0"]
    assert (tmp_path / "b.csv").read_text().splitlines() == ["file,si_sdr,si_sir,si_sar,lsd,stoi,estoi", "f.wav,1.0,2.0,3.0,4.0,0.5,0.25",
                                                             "mean,1.0,2.0,3.0,4.0,0.5,0.25"]


# ---- the restatement ------------------------------------------------------------------------------------------------------------

def test_band_table_and_filter_length():
    assert sr.thirdoct() == sr.BANDS and sr.BANDS[0] == (7, 9) and sr.BANDS[-1] == (174, 219)
    h, L = sr.taps(24000)
    assert L == 435 and len(h) == 871 and abs(h.sum() - 5.0) < 1e-12 and np.array_equal(h, h[::-1])
    assert [sr.ratio(r) for r in sr.RATES] == [(1, 1), (5, 8), (5, 12), (5, 24)]
    assert sr.EPS == 2.0 ** -52


def test_resampler_is_the_sum_of_the_definition():
    """``scipy.signal.resample_poly`` against y[n] = sum_j x[j] h'[L + n q - j p], term by term, on a short odd length per rate."""
    for rate, n in ((24000, 1501), (16000, 1203), (48000, 2999)):
        x = sr.am_noise(n, rate, 40)
        a, b = sr.resample(x, rate), sr.resample_direct(x, rate)
        assert len(a) == len(b) == sr.resampled_length(n, rate)
        assert np.abs(a - b).max() <= 1e-14 * np.abs(b).max()
    x = sr.am_noise(700, 10000, 41)
    assert np.array_equal(sr.resample(x, 10000), x.astype(np.float64))


def test_identity_gives_one():
    for name in ("one_segment", "gaps", "rate16k", "rate48k", "rate10k"):
        rate, _, lengths, clean, _ = sr.build(name)
        d, e, _ = sr.scores(clean[0, :lengths[0]], clean[0, :lengths[0]], rate)
        assert abs(d - 1) <= 1e-12 and abs(e - 1) <= 1e-12, (name, d, e)


def test_thirty_frames_is_the_threshold():
    rate, _, (n,), clean, est = sr.build("one_segment")
    d, e, T = sr.scores(clean[0], est[0], rate)
    assert n == 9829 and T == 30 and sr.keep_mask(sr.resample(clean[0], rate)).all() and 0 < e < d < 1
    rate, _, (n,), clean, est = sr.build("too_short")
    assert n == 9828 and sr.keep_mask(sr.resample(clean[0], rate)).all()
    assert sr.scores(clean[0], est[0], rate) == (1e-5, 1e-5, 29)


def test_noise_lowers_the_scores_in_order():
    clean = sr.am_noise(36000, 24000, 50)
    got = [sr.scores(clean, sr.degrade(clean, snr, 50), 24000) for snr in (20.0, 0.0, -10.0)]
    print("STOI / ESTOI at 20, 0, -10 dB:", got)
    assert got[0][0] > 0.98 and 0.6 < got[1][0] < 0.9 and got[2][0] < 0.5
    assert got[0][0] > got[1][0] > got[2][0] and got[0][1] > got[1][1] > got[2][1]


def test_zero_rows_are_scaled_by_zero_not_by_infinity():
    """A band that is exactly 0 over a whole segment (and a frame that is 0 in every band) gives finite scores."""
    v = np.zeros((1, 15, 30))
    assert np.array_equal(sr._row_col_normalize(v), v)
    rng = np.random.default_rng(3)
    v = rng.uniform(1, 2, (2, 15, 30))
    v[0, 4] = 0.0
    assert np.isfinite(sr._row_col_normalize(v)).all()


def test_pystoi_agrees_where_it_is_installed():
    pystoi = pytest.importorskip("pystoi")
    rate, _, (n,), clean, est = sr.build("gaps")
    for ext, tol in ((False, 1e-6), (True, 1e-6)):
        want = pystoi.stoi(clean[0].astype(np.float64), est[0].astype(np.float64), rate, extended=ext)
        assert abs(sr.stoi(clean[0], est[0], rate, ext) - want) <= tol


# ---- conditioning of the GPU cases (on the reference alone) -----------------------------------------------------------------------

@pytest.mark.parametrize("name,b", ITEMS)
def test_case_is_well_conditioned(name, b):
    rate, stride, lengths, clean, est = sr.build(name)
    n = lengths[b]
    assert clean.shape == est.shape == (len(lengths), stride) and clean.dtype == est.dtype == np.float32
    assert not clean[b, n:].any() and not est[b, n:].any()
    margin = sr.keep_margin(sr.resample(clean[b, :n], rate))
    sens = sr.sensitivity(clean[b, :n], est[b, :n], rate)
    print(f"{name}[{b}]: {sr.expected(name)[b]}, keep margin {margin:.3f} dB, sens {sens:.2e}")
    assert margin >= 1e-3
    assert sens <= 1e-12
    assert all(np.isfinite(v) for v in sr.expected(name)[b])


def test_cases_cover_removed_frames_the_clip_and_exact_zeros():
    rate, _, (n,), clean, est = sr.build("gaps")
    assert n == 36001 and n % 12 != 0
    keep = sr.keep_mask(sr.resample(clean[0], rate))
    runs = np.flatnonzero(np.diff(np.concatenate(([1], keep.astype(int), [1]))))     # boundaries of the removed stretches
    assert not keep[0] and not keep[-1] and len(runs) == 6, (keep.astype(int), runs)      # start, middle and end
    x, y = sr.resample(clean[0], rate), sr.resample(est[0], rate)
    assert sr.scores_10k(x, y, detail=True)[3]                     # the clip min(.) binds on some element
    assert sr.CASES[3][0] == "mixed" and sr.build("mixed")[1:3] == (36064, (36001, 11000, 9829))
    _, _, _, _, ez = sr.build("zeros_in_est")
    assert not ez[0, sr.ZEROED[0]:sr.ZEROED[1]].any() and sr.ZEROED[1] - sr.ZEROED[0] == 8000
    assert [sr.build(k)[0] for k in ("rate16k", "rate48k", "rate10k")] == [16000, 48000, 10000]
    assert [sr.build(k)[2] for k in ("rate16k", "rate48k", "rate10k")] == [(16000,), (24000,), (5000,)]
    assert sr.expected("too_short")[0] == (1e-5, 1e-5, 29) and sr.expected("one_segment")[0][2] == 30
