"""Float64 numpy restatement of the two evaluation metrics, written from their formulas, and the shapes and fixture access the metric
tests share.

    alpha_s = <s^, s> / (eps + |s|^2)        alpha_n = <s^, n> / (eps + |n|^2)         eps = 1e-10
    s_t = alpha_s s,  e_n = alpha_n n,  e_a = s^ - s_t - e_n
    SI-SDR, SI-SIR, SI-SAR = 10 log10(eps + |s_t|^2 / (eps + |e_n + e_a|^2, |e_n|^2, |e_a|^2))
    LSD = sqrt(mean over bins and frames of |2 log(eps + |S^|) - 2 log(eps + |S|)|)
          S = STFT, n_fft 510, hop 128, periodic Hann of 510, frames centred on t * 128 over the signal reflect-padded by 255 samples:
          256 bins x (1 + L // 128) frames
"""
import os

import numpy as np

EPS = 1e-10
N_FFT, HOP = 510, 128
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics.npz")

# the smallest shapes at which each thing can go wrong: (name, B, stride, lengths)
CASES = [("mixed", 3, 4096, (4096, 257, 1300)),      # full width / just above the reflect-padding limit (3 frames) / no multiple of 128 or 256
         ("long", 1, 24000, (24000,)),               # more than one workgroup's slice per item
         ("short", 5, 512, (512,) * 5)]
RATIO_RANGE_DB = (-10.0, 40.0)                       # where the fixture's ratios lie (asserted by the generator and by the host test)
BIN_FLOOR = 1e-6                                     # no |S| or |S^| bin of the fixture is below this: log(eps + |S|) is well-conditioned


def ratios(s_hat, s, n):
    """-> (si_sdr, si_sir, si_sar) in dB for 1-D signals, float64."""
    s_hat, s, n = (np.asarray(x, dtype=np.float64) for x in (s_hat, s, n))
    alpha_s = np.dot(s_hat, s) / (EPS + np.dot(s, s))
    alpha_n = np.dot(s_hat, n) / (EPS + np.dot(n, n))
    s_t, e_n = alpha_s * s, alpha_n * n
    e_a = s_hat - s_t - e_n
    pt = np.dot(s_t, s_t)
    return tuple(10.0 * np.log10(EPS + pt / (EPS + np.dot(v, v))) for v in (e_n + e_a, e_n, e_a))


def spectrum(x):
    """|STFT| of a 1-D signal, float64 [256, 1 + L // 128]."""
    x = np.asarray(x, dtype=np.float64)
    assert x.ndim == 1 and x.shape[0] > N_FFT // 2
    T = 1 + x.shape[0] // HOP
    xp = np.pad(x, N_FFT // 2, mode="reflect")
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)
    frames = np.stack([xp[t * HOP: t * HOP + N_FFT] * w for t in range(T)])
    return np.abs(np.fft.rfft(frames, n=N_FFT, axis=1)).T


def lsd(s_hat, s):
    d = np.abs(2.0 * np.log(EPS + spectrum(s_hat)) - 2.0 * np.log(EPS + spectrum(s)))
    return float(np.sqrt(d.mean()))


def load_case(g, name):
    """-> dict(est, clean, noise float32 [B, stride]; lengths int32 [B]; ratios float64 [B, 3]; lsd, lsd_f32_vs_f64 float64 [B])"""
    return {k: g[f"{name}_{k}"] for k in ("est", "clean", "noise", "lengths", "ratios", "lsd", "lsd_f32_vs_f64")}
