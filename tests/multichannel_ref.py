"""numpy float64 restatement of the rules ``data.channels=all`` adds (tests/test_multichannel_host.py, tests/test_hip_multichannel.py).
Nothing here calls the library.

  one gain per file   ``load_file``: every channel resampled on its own (``scipy.signal.resample``: the loader's FFT method), then
                      ``mx = max |v|`` over ALL channels and samples in float64, a NaN never the peak, every channel ``v / mx * 0.8`` with
                      two roundings, then float32.  A silent file gives NaN, a silent channel of another file exact zeros.
  the writer          ``store_file``: every row of a file the way of tests/store_ref.py (float32 -> float64 -> resampled -> float32 -> the
                      writer's 16-bit code, or the float32 itself), then interleaved ``[num, C]``.
  the hand-off        ``handoff_file``: the per-sample arithmetic of tests/handoff_ref.py (the 16-bit file and its decode), the peak over
                      all rows of the file.
"""
import numpy as np

import store_ref as sr
from handoff_ref import handoff_row


def joint_gain(x64: np.ndarray, normalize: bool = True) -> np.ndarray:
    """x64 float64 ``[C, L]`` (all channels of one file, after resampling) -> float32 ``[C, L]`` under the file's one gain."""
    x = np.asarray(x64, dtype=np.float64)
    if normalize:
        mag = np.abs(x)
        mag = mag[~np.isnan(mag)]                            # `fabs(v) > mx` is false for a NaN
        mx = np.float64(mag.max()) if mag.size else np.float64(0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            x = x / mx * 0.8                                 # in this order: two roundings; mx = 0 gives NaN
    return x.astype(np.float32)


def load_file(frames64: np.ndarray, num: int, normalize: bool = True) -> np.ndarray:
    """frames64 float64 ``[n, C]`` (a decoded file, interleaved as a WAV reader returns it) -> float32 ``[C, num]``."""
    from scipy.signal import resample
    a = np.asarray(frames64, dtype=np.float64)
    a = a[:, None] if a.ndim == 1 else a
    x = np.ascontiguousarray(a.T)
    if num != x.shape[1]:
        x = np.stack([resample(c, num) for c in x])
    return joint_gain(x, normalize)


def store_file_float(rows32: np.ndarray, num: int) -> np.ndarray:
    """rows32 float32 ``[C, len]`` (a file's rows over their valid samples) -> the oracle's float64 ``[num, C]``."""
    return np.stack([sr.oracle(np.asarray(r, dtype=np.float32), num) for r in rows32], axis=1)


def interleave(rows: np.ndarray) -> np.ndarray:
    """``[C, num]`` -> ``[num, C]`` contiguous: the sample order of a WAV file."""
    return np.ascontiguousarray(np.asarray(rows).T)


def handoff_file(rows32: np.ndarray, subtype: str = "PCM_16", normalize: bool = True):
    """rows32 float32 ``[C, L]`` (a file's rows over their valid samples) -> (float32 ``[C, L]``, the file's peak as a float64): every
    sample decoded as ``handoff_row`` decodes it, ONE peak over the file."""
    dec = np.stack([handoff_row(r, subtype, normalize=False)[0].astype(np.float64) for r in rows32])
    # handoff_row without normalisation returns float32(v); v is q / 32768 (exact in float32) or a widened float32: the round trip is exact
    peaks = [handoff_row(r, subtype, normalize=False)[1] for r in rows32]
    mx = np.float64(max(peaks))
    if not normalize:
        return dec.astype(np.float32), mx
    with np.errstate(invalid="ignore", divide="ignore"):
        out = dec / mx * 0.8
    return out.astype(np.float32), mx
