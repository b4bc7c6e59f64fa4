"""CPU-only checks of the evaluation metrics: the two entry points in the header, the library and the ctypes table; the host-side
refusals of ``use_metrics_workspace`` / ``use_metrics`` (nothing is launched); and the fixture ``tests/golden/metrics.npz`` (the
reference's own ``energy_ratios`` and ``lsd``, scripts/gen_golden_metrics.py) against the float64 restatement of the two formulas in
``metrics_ref.py`` - which the GPU tests then lean on - with the conditioning the fixture's inputs were chosen for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import metrics_ref as mr
from universal_speech_enhancement_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("use_metrics_workspace", "use_metrics")


@pytest.fixture(scope="module")
def golden():
    return np.load(mr.GOLDEN)


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "use_hip.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in use_hip.h"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS
    assert all(f"USE_METRIC_{k}" in header for k in ("SI_SDR = 0", "SI_SIR = 1", "SI_SAR = 2", "LSD = 3", "COUNT = 4"))
    assert _lib.SYMBOLS["use_metrics_workspace"][0] is C.c_size_t


def test_workspace_is_zero_for_bad_arguments_and_grows_with_the_batch():
    L = _lib.lib()
    for B, stride in ((0, 4096), (-1, 4096), (3, 0), (3, -5), (0, 0)):
        assert L.use_metrics_workspace(B, stride) == 0
    one, three = L.use_metrics_workspace(1, 4096), L.use_metrics_workspace(3, 4096)
    assert 0 < one < three and three % 8 == 0
    assert L.use_metrics_workspace(1, 24000) > one


def test_refusals_name_the_argument_and_launch_nothing():
    """Host-only: every check is in front of the first launch, so host memory stands in for the device buffers."""
    L = _lib.lib()
    buf = np.zeros(8, np.float64)
    p = buf.ctypes.data

    def call(est=p, clean=p, noise=p, lens=(4096,), B=1, stride=4096, work=p, nbytes=1 << 30, out=p):
        arr = (C.c_int * max(len(lens), 1))(*lens) if lens is not None else None
        return L.use_metrics(est, clean, noise, arr, B, stride, work, nbytes, out, None)

    for kw, word in ((dict(B=0), b"B="), (dict(stride=0), b"stride"), (dict(est=None), b"est"), (dict(clean=None), b"clean"),
                     (dict(lens=None), b"len"), (dict(work=None), b"work"), (dict(out=None), b"out_dev"),
                     (dict(lens=(255,)), b"len[0]=255"), (dict(lens=(4097,)), b"len[0]=4097"),
                     (dict(lens=(4096, 100), B=2), b"len[1]=100"),
                     (dict(nbytes=L.use_metrics_workspace(1, 4096) - 1), b"work_bytes")):
        assert call(**kw) == -1, kw                                # USE_E_INVALID
        assert word in L.use_last_error(), (kw, L.use_last_error())


def test_python_surface_refuses_what_it_cannot_run():
    import torch
    from universal_speech_enhancement_amd import metrics
    from universal_speech_enhancement_amd.sgmse.util import other
    x = torch.zeros(2, 512)
    with pytest.raises(_lib.UseHipError, match="CUDA"):            # no CPU implementation, no quiet fall-back
        metrics.evaluate(x, x, x)
    with pytest.raises(ValueError, match="eps"):
        other.lsd(x, x, eps=1e-8)
    assert {"pad_spec", "lsd", "si_sdr_components", "energy_ratios"} <= set(dir(other))


def test_si_sdr_components_add_up_and_give_the_fixture_ratios(golden):
    """The plain-torch ``si_sdr_components``: s_target + e_noise + e_art = s_hat, and the ratios of its components are the
    reference's (float64 both sides: 1e-9 dB)."""
    import torch
    from universal_speech_enhancement_amd.sgmse.util.other import si_sdr_components
    c = mr.load_case(golden, "long")
    e, s, n = (torch.from_numpy(c[k][0]) for k in ("est", "clean", "noise"))
    st, en, ea = si_sdr_components(e, s, n)
    assert st.dtype == torch.float64 and torch.allclose(st + en + ea, e.double(), rtol=0, atol=1e-15)
    p = lambda v: float((v * v).sum())
    got = [10 * np.log10(1e-10 + p(st) / (1e-10 + p(v))) for v in (en + ea, en, ea)]
    assert np.abs(np.array(got) - c["ratios"][0]).max() <= 1e-9


@pytest.mark.parametrize("case", [c[0] for c in mr.CASES])
def test_restatement_reproduces_the_fixture(golden, case):
    """Ratios to 1e-9 dB (float64 against the reference's float64).  LSD within the stored ``lsd_f32_vs_f64``: the fixture's LSD is
    the reference's float32 evaluation and the stored figure is its distance to ``torch.stft`` in float64; this restatement is a
    second float64 evaluation (numpy rfft), 1e-15 from the first, and the 1e-12 added to the bound is for that distance alone -
    five orders below the smallest stored figure."""
    c = mr.load_case(golden, case)
    _, B, stride, lengths = next(x for x in mr.CASES if x[0] == case)
    assert c["est"].shape == (B, stride) and c["est"].dtype == np.float32 and tuple(c["lengths"]) == lengths
    for b, L in enumerate(lengths):
        e, s, n = (c[k][b, :L] for k in ("est", "clean", "noise"))
        assert not c["est"][b, L:].any() and not c["clean"][b, L:].any() and not c["noise"][b, L:].any()   # zero padding
        d = np.abs(np.array(mr.ratios(e, s, n)) - c["ratios"][b]).max()
        dl, bound = abs(mr.lsd(e, s) - c["lsd"][b]), c["lsd_f32_vs_f64"][b]
        print(f"{case}[{b}]: ratios off by {d:.3e} dB, lsd off by {dl:.3e} (stored f32 vs f64 {bound:.3e})")
        assert d <= 1e-9
        assert 0 < bound and dl <= bound + 1e-12


@pytest.mark.parametrize("case", [c[0] for c in mr.CASES])
def test_fixture_is_well_conditioned(golden, case):
    c = mr.load_case(golden, case)
    lo, hi = mr.RATIO_RANGE_DB
    assert lo <= c["ratios"].min() and c["ratios"].max() <= hi
    for b, L in enumerate(c["lengths"]):
        assert min(mr.spectrum(c["est"][b, :L]).min(), mr.spectrum(c["clean"][b, :L]).min()) >= mr.BIN_FLOOR
    assert os.path.getsize(mr.GOLDEN) < 1 << 20
