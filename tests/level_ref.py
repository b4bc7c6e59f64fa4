"""What tests/test_level_host.py and tests/test_hip_level.py share: the arithmetic ``data.restore_level`` is held to, and the shapes.

The gain of a file is ``g = mx / 0.8`` (one float64 division; ``mx`` the peak the loader divided by).  A store function with a gain forms
``x32 = float32(v * g)``: ``v`` the float64 value it holds - the widened row sample at ``num == len``, the resampled value otherwise - one
float64 product, one rounding to float32; then the writer's rule (tests/store_ref.py: the float itself, or ``quantise``).
  ``num == len``   bit-equal to ``exact(x, g)``.
  resampled        ``store_ref.check_float32(got, oracle(x, num) * g)``.  Its bound ``1e-11 * max(1, max|want|)`` is never tighter than
                   the resampler's own bound times g: for g < 1 the floor of 1 holds it up, for g > 1 it scales with g.
The round trip (loader -> identity sampler -> writer, FLOAT files) is held to ``2^-22 * |v|`` per sample: two float32 roundings of
relative ``2^-24`` each (the loader's cast, the writer's cast) plus float64 roundings of ``2^-53`` each leave ``(1 + 2^-24)^2 - 1 <
2^-22.99``; ``2^-22`` is twice that."""
import numpy as np

import store_ref as sr

# (len, num): the 256-thread and 4096-sample slice edges on the pass-through (float source) and on the resampled (double source) kernels,
# powers of two and Bluestein
SHAPES = [(1, 1), (2, 3), (255, 512), (256, 512), (257, 512), (4095, 4095), (4096, 4096), (4097, 4097), (4096, 8192), (2400, 4410),
          (2401, 801)]
GAINS = [1.0, 0.4625, 3.0, 0.0]
ROUND_TRIP = 2.0 ** -22


def exact(x32: np.ndarray, g: float) -> np.ndarray:
    """``num == len``: float32 -> float64, times g, -> float32."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (x32.astype(np.float64) * np.float64(g)).astype(np.float32)


def want64(x32: np.ndarray, num: int, g: float) -> np.ndarray:
    """The float64 values a store function rounds: the scipy oracle times g."""
    return sr.oracle(x32, num) * np.float64(g)


def check_row(got: np.ndarray, x32: np.ndarray, num: int, g: float, what: str = "") -> None:
    """A FLOAT32 row under the rules above."""
    if num == len(x32):
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), exact(x32, g).view(np.uint32)), what
    else:
        sr.check_float32(got, want64(x32, num, g), what)


def source_gain(mx) -> np.float64:
    return np.float64(mx) / np.float64(0.8)


def peak(v64: np.ndarray) -> np.float64:
    """The loader's peak: ``fabs(v) > mx`` from 0, so a NaN is never the peak."""
    mag = np.abs(np.asarray(v64, dtype=np.float64)).reshape(-1)
    mag = mag[~np.isnan(mag)]
    return np.float64(mag.max()) if mag.size else np.float64(0.0)
