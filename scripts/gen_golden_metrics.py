#!/usr/bin/env python3
"""Golden vectors of the evaluation metrics -- runs ONLY in the build container (needs the reference checkout).

Same method as ``oracle/gen_golden.py``: the reference's own ``lsd`` and ``energy_ratios`` (``sgmse/util/other.py:15-62``) are
imported, with in-memory stub modules for what that file imports and never uses on this path (matplotlib, torchaudio, pydub, tqdm),
and run on seeded signals.  Data only is written: ``tests/golden/metrics.npz``.

    python scripts/gen_golden_metrics.py --reference <reference checkout>      (or USE_REFERENCE_DIR=<reference checkout>)

How the reference is called.  ``energy_ratios`` gets float64 copies of the stored float32 waveforms - its evaluation scripts pass
what ``soundfile.read`` returns, float64 - so numpy works in float64 there.  ``lsd`` gets the float32 arrays themselves: its
``torch.stft`` window is the float32 ``torch.hann_window(510)`` and takes a float32 signal.  ``lsd_f32_vs_f64`` is, per item, the
distance between that formula with ``torch.stft`` in float32 and in float64 (window and signal): the reference's own rounding
sensitivity, which the tests use as the scale of their LSD bounds.

Signals (per item; shapes and lengths: ``tests/metrics_ref.py: CASES``), chosen so that the reference itself is well-conditioned:
  s     three decaying sinusoids + white noise at 1e-3 RMS (the floor keeps every STFT bin far above eps = 1e-10)
  n     white noise at 0.1 RMS
  s^    s + a n + b w, w independent white noise at 0.1 RMS, (a, b) per item so that the three ratios lie in -10 ... +40 dB
Asserted here: every stored ratio is in that range, and no |S| or |S^| bin is below 1e-6.  Samples past an item's length are zero.
"""
import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "metrics.npz")
SEED = 97
# (a, b) of s^ = s + a n + b w, cycled over the items of a case: ratios from about 5 dB to about 35 dB
MIX = [(0.3, 0.1), (2.0, 0.02), (0.03, 1.0), (0.3, 0.05), (1.0, 1.0)]


def signals(case: str, b: int, L: int):
    from universal_speech_enhancement_amd.testing import noise as tnoise
    t = np.arange(L, dtype=np.float64) / 24000.0
    s = np.zeros(L)
    for j, (f, amp, tau) in enumerate([(220.0, 0.5, 0.30), (1370.0, 0.3, 0.08), (5210.0, 0.2, 0.02)]):
        s += amp * np.exp(-t / tau) * np.sin(2.0 * np.pi * f * (1.0 + 0.07 * b) * t + j)
    s = (s + 1e-3 * tnoise.normal(SEED, f"{case}{b}floor", L)).astype(np.float32)
    n = (0.1 * tnoise.normal(SEED, f"{case}{b}n", L)).astype(np.float32)
    w = (0.1 * tnoise.normal(SEED, f"{case}{b}w", L)).astype(np.float32)
    a, c = MIX[b % len(MIX)]
    return (s + np.float32(a) * n + np.float32(c) * w).astype(np.float32), s, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("USE_REFERENCE_DIR"), help="the reference project's checkout")
    a = ap.parse_args()
    if not a.reference:
        ap.error("--reference (or USE_REFERENCE_DIR) is required")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, a.reference)
    for m in ("matplotlib", "matplotlib.pyplot", "torchaudio", "pydub", "tqdm"):
        sys.modules.setdefault(m, types.ModuleType(m))
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.modules["pydub"].AudioSegment = object

    import torch

    import metrics_ref as mr
    from src.models.components.sgmse.util import other as ref

    torch.set_num_threads(8)

    def mags(x, dtype):
        return torch.stft(torch.from_numpy(x).to(dtype), n_fft=510, hop_length=128, window=torch.hann_window(510, dtype=dtype),
                          return_complex=True).abs()

    def lsd_as(x_hat, x, dtype):
        d = 2 * torch.log(1e-10 + mags(x_hat, dtype)) - 2 * torch.log(1e-10 + mags(x, dtype))
        return torch.sqrt(torch.mean(torch.abs(d))).item()

    out = {}
    for case, B, stride, lengths in mr.CASES:
        est, clean, noise = (np.zeros((B, stride), np.float32) for _ in range(3))
        ratios, lsd, sens = np.zeros((B, 3)), np.zeros(B), np.zeros(B)
        for b, L in enumerate(lengths):
            e, s, n = signals(case, b, L)
            est[b, :L], clean[b, :L], noise[b, :L] = e, s, n
            ratios[b] = ref.energy_ratios(e.astype(np.float64), s.astype(np.float64), n.astype(np.float64))
            lsd[b] = ref.lsd(e, s)
            l32, l64 = lsd_as(e, s, torch.float32), lsd_as(e, s, torch.float64)
            assert l32 == lsd[b], (case, b, l32, lsd[b])               # the restatement above IS the reference's formula
            sens[b] = abs(l32 - l64)
            floor = min(float(mags(e, torch.float64).min()), float(mags(s, torch.float64).min()))
            assert mr.RATIO_RANGE_DB[0] <= ratios[b].min() and ratios[b].max() <= mr.RATIO_RANGE_DB[1], (case, b, ratios[b])
            assert floor >= mr.BIN_FLOOR, (case, b, floor)
            print(f"{case}[{b}] L={L}: si_sdr {ratios[b, 0]:.3f} si_sir {ratios[b, 1]:.3f} si_sar {ratios[b, 2]:.3f} dB, lsd {lsd[b]:.6f} "
                  f"(f32 vs f64 {sens[b]:.3e}), smallest bin {floor:.3e}")
        out.update({f"{case}_est": est, f"{case}_clean": clean, f"{case}_noise": noise, f"{case}_lengths": np.asarray(lengths, np.int32),
                    f"{case}_ratios": ratios, f"{case}_lsd": lsd, f"{case}_lsd_f32_vs_f64": sens})
    np.savez(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
