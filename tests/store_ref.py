"""What tests/test_store_host.py and tests/test_hip_device_store.py share: the rules a restored row is held to.

FLOAT32 rows are compared with ``scipy.signal.resample(float64(x), num).astype(float32)``.  The resampler's own bound is the project's
``D = 1e-11 * max(1, max|want|)`` (tests/test_hip_device_loader.py); a result within D of the oracle's fp64 value rounds to another
float32 than the oracle's only where that value lies within D of a rounding midpoint, and then to the neighbour across that midpoint.
So: bit-equal everywhere else, one ulp apart there.  PCM16 rows are pinned to the implementation's own FLOAT32 row by the writer's
rule, ``nearbyint(float64(x32) * 32767)`` clamped to [-32768, 32767], NaN -> 0, bit for bit."""
import numpy as np

# len -> num: trivial sizes; the edges of a 256-thread workgroup; powers of two both ways (no Bluestein; 8192 -> 4096 halves onto an even
# num, the doubled Nyquist bin); Bluestein both ways (2400 -> 4800: an even len going up, the halved Nyquist bin; 2400 -> 1600: an even num
# going down); odd and prime lengths
SHAPES = [(1, 1), (1, 3), (2, 3), (2, 1), (3, 2), (255, 512), (256, 512), (257, 512), (4096, 8192), (8192, 4096),
          (2400, 4800), (2400, 4410), (2400, 1600), (2401, 801), (2399, 4799)]


def signal(n: int, num: int) -> np.ndarray:
    """The float32 input of a shape: noise at speech level, the same in every test."""
    return (np.random.default_rng(1000 * n + num).standard_normal(n) * 0.3).astype(np.float32)


def oracle(x32: np.ndarray, num: int) -> np.ndarray:
    """scipy.signal.resample in float64 (``num == len``: the signal itself)."""
    from scipy.signal import resample
    x = x32.astype(np.float64)
    return x if num == len(x) else resample(x, num)


def bound(want64: np.ndarray) -> float:
    return 1e-11 * max(1.0, float(np.abs(want64).max()))


def check_float32(got: np.ndarray, want64: np.ndarray, what: str = "") -> int:
    """``got`` (float32) against the oracle's fp64 values under the rule above; -> the number of samples that took the other side of a
    rounding midpoint."""
    assert got.dtype == np.float32 and got.shape == want64.shape, (what, got.dtype, got.shape, want64.shape)
    want32 = want64.astype(np.float32)
    D = bound(want64)
    err = float(np.abs(got.astype(np.float64) - want64).max())
    differ = np.nonzero(got.view(np.uint32) != want32.view(np.uint32))[0]
    print(f"{what}: max |got - oracle64| = {err:.3e}, D = {D:.3e}, {len(differ)} of {len(got)} samples on the other side of a midpoint")
    if len(differ):
        g, w = got[differ], want32[differ]
        neighbour = np.nextafter(w, g)                                           # one ulp from the oracle's float32 towards got
        assert np.array_equal(g.view(np.uint32), neighbour.view(np.uint32)), (what, "more than one ulp", differ[:5], g[:5], w[:5])
        mid = (w.astype(np.float64) + neighbour.astype(np.float64)) / 2
        off = np.abs(want64[differ] - mid)
        print(f"{what}: largest distance of such an oracle value from its midpoint = {float(off.max()):.3e}")
        assert (off <= D).all(), (what, "differs away from a midpoint", differ[:5], off[:5], D)
    return len(differ)


def quantise(x32: np.ndarray) -> np.ndarray:
    """The codes ``use_wav_write`` stores for float32 samples."""
    v = np.nan_to_num(np.rint(x32.astype(np.float64) * 32767.0), nan=0.0, posinf=np.inf, neginf=-np.inf)
    return np.clip(v, -32768.0, 32767.0).astype(np.int16)


def check_codes(codes: np.ndarray, want64: np.ndarray, what: str = "") -> int:
    """16-bit ``codes`` whose float32 values are not at hand (a file) against fp64 values ``want64``: every code is the writer's code of
    a float32 the FLOAT32 rule allows - the rounded oracle value, or its neighbour across a midpoint within D.  -> the number of the
    latter."""
    assert codes.dtype == np.int16 and codes.shape == want64.shape, (what, codes.dtype, codes.shape, want64.shape)
    want32 = want64.astype(np.float32)
    D = bound(want64)
    differ = np.nonzero(codes != quantise(want32))[0]
    print(f"{what}: {len(differ)} of {len(codes)} codes are not the code of the rounded oracle value, D = {D:.3e}")
    if len(differ):
        w, v = want32[differ], want64[differ]
        other = np.nextafter(w, np.where(v > w, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        off = np.abs(v - (w.astype(np.float64) + other.astype(np.float64)) / 2)
        assert (off <= D).all() and np.array_equal(codes[differ], quantise(other)), (what, differ[:5], codes[differ][:5], off[:5], D)
    return len(differ)
