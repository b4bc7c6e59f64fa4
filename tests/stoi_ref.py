"""Float64 restatement of STOI / ESTOI as ``use_stoi`` defines them (csrc/use_stoi.hip; Taal et al. 2011, Jensen & Taal 2016, in the
shape of ``pystoi.stoi(clean, processed, fs, extended)``), and the cases the host and GPU tests share.  Two departures from pystoi, both
on purpose: no ``EPS * randn`` dither in ESTOI's normalisations, and a row or column whose sum of squares is exactly 0 is scaled by 0
(what the dither gives in expectation) instead of by 1 / 0.

Cases are built from fixed seeds at import: no fixture file."""
from fractions import Fraction
from functools import lru_cache

import numpy as np
from scipy.signal import resample_poly

FS, N_FRAME, NFFT, NUMBAND, MINFREQ, N, BETA, DYN_RANGE = 10000, 256, 512, 15, 150, 30, -15.0, 40.0
HOP = N_FRAME // 2
EPS = np.finfo(np.float64).eps                                  # 2^-52
SHORT = 1e-5                                                    # pystoi's value for fewer than N frames
RATES = (10000, 16000, 24000, 48000)
BANDS = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109), (109, 138),
         (138, 174), (174, 219))
W = np.hanning(N_FRAME + 2)[1:-1]


def ratio(fs):
    f = Fraction(FS, fs)
    return f.numerator, f.denominator


def taps(fs):
    """-> (h', L): the 2 L + 1 taps of the resampler, scaled as ``resample_poly(x, p, q, window=h / sum(h))`` applies them."""
    p, q = ratio(fs)
    fc = 1.0 / (2 * max(p, q))
    L = int(np.ceil(52.0 / (28.714 * fc / 10)))
    t = np.arange(-L, L + 1)
    h = np.kaiser(2 * L + 1, 0.1102 * (60.0 - 8.7)) * (2 * p * fc * np.sinc(2 * fc * t))
    return p * (h / np.sum(h)), L


def resampled_length(n, fs):
    p, q = ratio(fs)
    return -(-n * p // q)


def resample(x, fs):
    x = np.asarray(x, np.float64)
    if fs == FS:
        return x.copy()
    p, q = ratio(fs)
    h, _ = taps(fs)
    return resample_poly(x, p, q, window=h / p)                 # resample_poly multiplies the window by p itself


def resample_direct(x, fs):
    """The sum of the definition, term by term (slow; the host test holds ``resample`` against it)."""
    p, q = ratio(fs)
    h, L = taps(fs)
    x = np.asarray(x, np.float64)
    y = np.zeros(resampled_length(len(x), fs))
    for n in range(len(y)):
        j = np.arange(max(0, -(-(n * q - L) // p)), min(len(x) - 1, (n * q + L) // p) + 1)
        y[n] = np.sum(x[j] * h[L + n * q - j * p])
    return y


def thirdoct(fs=FS, nfft=NFFT, num_bands=NUMBAND, min_freq=MINFREQ):
    """-> the [lo, hi) bin ranges of the third-octave bands."""
    f = np.linspace(0, fs, nfft + 1)[:nfft // 2 + 1]
    k = np.arange(num_bands, dtype=np.float64)
    lo, hi = min_freq * 2.0 ** ((2 * k - 1) / 6), min_freq * 2.0 ** ((2 * k + 1) / 6)
    return tuple((int(np.argmin((f - a) ** 2)), int(np.argmin((f - b) ** 2))) for a, b in zip(lo, hi))


def frame_energies(x):
    fr = np.array([W * x[i:i + N_FRAME] for i in range(0, len(x) - N_FRAME + 1, HOP)])
    return 20 * np.log10(np.linalg.norm(fr, axis=1) + EPS)


def keep_mask(x):
    e = frame_energies(x)
    return (np.max(e) - DYN_RANGE - e) < 0


def keep_margin(x):
    """min_k |max(E) - 40 - E_k| in dB: how far the nearest keep decision is from flipping."""
    e = frame_energies(x)
    return float(np.min(np.abs(np.max(e) - DYN_RANGE - e)))


def remove_silent_frames(x, y):
    mask = keep_mask(x)
    out = []
    for s in (x, y):
        fr = np.array([W * s[i:i + N_FRAME] for i in range(0, len(s) - N_FRAME + 1, HOP)])[mask]
        sig = np.zeros((len(fr) - 1) * HOP + N_FRAME)
        for j, f in enumerate(fr):
            sig[j * HOP:j * HOP + N_FRAME] += f
        out.append(sig)
    return out


def tob(x):
    """-> [15, T] third-octave band magnitudes of the compacted signal x."""
    spec = np.array([np.fft.rfft(W * x[i:i + N_FRAME], n=NFFT) for i in range(0, len(x) - N_FRAME, HOP)]).reshape(-1, NFFT // 2 + 1)
    pw = np.abs(spec.T) ** 2
    return np.sqrt(np.stack([pw[lo:hi].sum(axis=0) for lo, hi in BANDS]))


def _unit(v, axis):
    ss = np.sum(v * v, axis=axis, keepdims=True)
    return v * np.where(ss > 0, 1.0 / np.sqrt(np.where(ss > 0, ss, 1.0)), 0.0)


def _row_col_normalize(s):
    s = _unit(s - s.mean(axis=2, keepdims=True), 2)
    return _unit(s - s.mean(axis=1, keepdims=True), 1)


def scores_10k(x, y, detail=False):
    """(stoi, estoi, T) of the clean x and the processed y, both already at 10 kHz."""
    x, y = remove_silent_frames(np.asarray(x, np.float64), np.asarray(y, np.float64))
    X, Y = tob(x), tob(y)
    T = X.shape[1]
    if T < N:
        return (SHORT, SHORT, T) + ((False,) if detail else ())
    xs = np.array([X[:, m:m + N] for m in range(T - N + 1)])
    ys = np.array([Y[:, m:m + N] for m in range(T - N + 1)])
    c = np.linalg.norm(xs, axis=2, keepdims=True) / (np.linalg.norm(ys, axis=2, keepdims=True) + EPS)
    bound = xs * (1 + 10 ** (-BETA / 20))
    clipped = bool((c * ys > bound).any())
    yp = np.minimum(c * ys, bound)
    yp = yp - yp.mean(axis=2, keepdims=True)
    xm = xs - xs.mean(axis=2, keepdims=True)
    yp = yp / (np.linalg.norm(yp, axis=2, keepdims=True) + EPS)
    xm = xm / (np.linalg.norm(xm, axis=2, keepdims=True) + EPS)
    d = float(np.sum(xm * yp) / (xs.shape[0] * NUMBAND))
    e = float(np.sum(_row_col_normalize(xs) * _row_col_normalize(ys)) / (N * xs.shape[0]))
    return (d, e, T) + ((clipped,) if detail else ())


def scores(clean, est, fs):
    """(stoi, estoi, T) of float signals at ``fs``: the yardstick of the GPU tests."""
    return scores_10k(resample(clean, fs), resample(est, fs))


def stoi(x, y, fs_sig, extended=False):
    """pystoi's signature: clean first."""
    return scores(x, y, fs_sig)[1 if extended else 0]


def sensitivity(clean, est, fs, trials=8, seed=99):
    """Largest change of either score when the 10 kHz signals move by 2^-43 max|x| u, u uniform in [-1, 1]: a bound on what any
    reordering of the resampler's filter sum (at most 1741 terms) can do to the scores."""
    x, y = resample(clean, fs), resample(est, fs)
    base = scores_10k(x, y)
    rng = np.random.default_rng(seed)
    worst = 0.0
    for _ in range(trials):
        got = scores_10k(x + 2.0 ** -43 * np.abs(x).max() * rng.uniform(-1, 1, len(x)),
                         y + 2.0 ** -43 * np.abs(y).max() * rng.uniform(-1, 1, len(y)))
        assert got[2] == base[2]
        worst = max(worst, abs(got[0] - base[0]), abs(got[1] - base[1]))
    return worst


# ---- the cases ------------------------------------------------------------------------------------------------------------------

def am_noise(n, fs, seed, silence=()):
    """Amplitude-modulated noise (4 Hz and 11 Hz envelopes), float32; ``silence``: [a, b) stretches scaled by 1e-4."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    x = rng.standard_normal(n) * (0.55 + 0.3 * np.sin(2 * np.pi * 4 * t + seed) + 0.15 * np.sin(2 * np.pi * 11 * t)) * 0.1
    for a, b in silence:
        x[a:b] *= 1e-4
    return x.astype(np.float32)


def degrade(clean, snr_db, seed):
    rng = np.random.default_rng(1000 + seed)
    noise = rng.standard_normal(len(clean))
    g = np.sqrt(np.mean(clean.astype(np.float64) ** 2) / np.mean(noise ** 2)) * 10 ** (-snr_db / 20)
    return (clean + g * noise).astype(np.float32)


GAPS = ((0, 2500), (15000, 18000), (33200, 36001))

# name, rate, stride, ((length, snr dB, seed, silence), ...)
CASES = (
    ("one_segment", 24000, 9829, ((9829, 0.0, 1, ()),)),
    ("too_short", 24000, 9828, ((9828, 0.0, 2, ()),)),
    ("gaps", 24000, 36001, ((36001, -10.0, 3, GAPS),)),
    ("mixed", 24000, 36064, ((36001, 20.0, 4, GAPS), (11000, 0.0, 5, ()), (9829, -10.0, 6, ()))),
    ("zeros_in_est", 24000, 30000, ((30000, 0.0, 7, ()),)),
    ("rate16k", 16000, 16000, ((16000, 0.0, 8, ()),)),
    ("rate48k", 48000, 24000, ((24000, 20.0, 9, ()),)),
    ("rate10k", 10000, 5000, ((5000, -10.0, 10, ()),)),
)
CASE_NAMES = tuple(c[0] for c in CASES)
ZEROED = (10000, 18000)                                         # zeros_in_est: the estimate is exactly 0 there


@lru_cache(maxsize=None)
def build(name):
    """-> (rate, stride, lengths, clean [B, stride], est [B, stride]) float32, zero past each length."""
    _, rate, stride, items = next(c for c in CASES if c[0] == name)
    clean, est = np.zeros((len(items), stride), np.float32), np.zeros((len(items), stride), np.float32)
    for b, (n, snr, seed, silence) in enumerate(items):
        clean[b, :n] = am_noise(n, rate, seed, silence)
        est[b, :n] = degrade(clean[b, :n], snr, seed)
        if name == "zeros_in_est":
            est[b, ZEROED[0]:ZEROED[1]] = 0.0
    for a in (clean, est):
        a.setflags(write=False)
    return rate, stride, tuple(i[0] for i in items), clean, est


@lru_cache(maxsize=None)
def expected(name):
    """The restatement on every item of a case, once: ((stoi, estoi, T), ...)."""
    rate, _, lengths, clean, est = build(name)
    return tuple(scores(clean[b, :n], est[b, :n], rate) for b, n in enumerate(lengths))
