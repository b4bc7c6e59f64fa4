"""Float64 numpy / scipy restatement of the degradation simulator ``use_distort`` runs (csrc/use_distort.hip), stage by stage and as
the whole chain, in the order of the reference's ``comm_distort_simu_dataset.__getitem__``; the same stages in ``np.longdouble`` (with a
direct convolution for the reverberation), which measures the restatement's own error; and the builder of the cases the GPU tests run.

The restatement uses ``scipy.signal.fftconvolve`` and ``np.histogram`` directly, as the reference does.  It needs no librosa:
``vad_keep`` restates ``librosa.effects.split(w, top_db=50)`` - frame RMS over 2048 samples at hop 512, centred, zero-padded,
``1 + len // 512`` frames, ``power_to_db(rms ** 2, ref=np.max, top_db=None) > -50`` - and ``split_intervals`` the interval arithmetic
that follows it there.  librosa is not installed where this was written: both are written from librosa 0.10's source as remembered,
not checked against the package.
"""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np
from scipy.signal import fftconvolve

from universal_speech_enhancement_amd.distort import Recipe, prepare_rir

HOP, FRAME, TOP_DB, AMIN = 512, 2048, 50.0, 1e-10
LD = np.longdouble
SLICE = 4096                       # samples per workgroup of the device's elementwise kernels
PAD = np.float32(1e3)              # what the cases fill the padding of every input row with


# ---- stage 2: the masked power --------------------------------------------------------------------------------------------------------

def frame_db(w: np.ndarray) -> np.ndarray:
    """dB of every frame's power against the loudest frame's."""
    w = np.asarray(w)
    nf = 1 + len(w) // HOP
    padded = np.concatenate([np.zeros(FRAME // 2, w.dtype), w, np.zeros(FRAME // 2, w.dtype)])
    frames = np.lib.stride_tricks.sliding_window_view(padded, FRAME)[::HOP][:nf]
    rms = np.sqrt(np.mean(np.abs(frames) ** 2, axis=-1))
    p = rms ** 2
    ten = w.dtype.type(10.0)
    return ten * np.log10(np.maximum(w.dtype.type(AMIN), p)) - ten * np.log10(np.maximum(w.dtype.type(AMIN), p.max()))


def vad_frames(w: np.ndarray) -> np.ndarray:
    return frame_db(w) > -TOP_DB


def vad_keep(w: np.ndarray) -> np.ndarray:
    """The sample mask of ``vad_merge``: sample s is kept iff frame ``s // 512`` is."""
    return vad_frames(w)[np.arange(len(w)) // HOP]


def split_intervals(w: np.ndarray) -> np.ndarray:
    """``librosa.effects.split``'s own way from the frame flags to sample intervals ``[start, end)``."""
    non_silent = vad_frames(w)
    edges = np.flatnonzero(np.diff(non_silent.astype(int)))
    edges = [edges + 1]
    if non_silent[0]:
        edges.insert(0, [0])
    if non_silent[-1]:
        edges.append([len(non_silent)])
    edges = np.minimum(np.concatenate(edges) * HOP, len(w))
    return edges.reshape(-1, 2)


def masked_power(w: np.ndarray, keep=None) -> float:
    keep = vad_keep(w) if keep is None else keep
    return np.mean(w[keep] ** 2)


def keep_margin(w: np.ndarray) -> float:
    """The smallest distance of a frame from the -50 dB threshold, in dB."""
    return float(np.abs(frame_db(np.asarray(w, np.float64)) + TOP_DB).min())


# ---- the stages -----------------------------------------------------------------------------------------------------------------------

def convolve_direct(x: np.ndarray, h: np.ndarray) -> np.ndarray:
    """``np.convolve(x, h)[:len(x)]`` tap by tap in the dtype of ``x`` (longdouble: the yardstick of the FFT convolutions)."""
    y = np.zeros(len(x), x.dtype)
    for j in range(min(len(h), len(x))):
        y[j:] += h[j] * x[: len(x) - j]
    return y


def reverberate(x, h):
    """-> (full, early): ``(x * h)[:len]`` and ``(x * h[:6])[:len]``."""
    if x.dtype == LD:
        return convolve_direct(x, h), convolve_direct(x, h[:6])
    return fftconvolve(x, h, mode="full")[: len(x)], fftconvolve(x, h[:6], mode="full")[: len(x)]


def add_noise(clean, noise, snr, keeps=None):
    """-> (noisy, scale, P(clean), P(noise)); ``keeps``: the two sample masks, to hold the decisions fixed."""
    T = clean.dtype.type
    pc = masked_power(clean, keeps[0] if keeps else None)
    pn = masked_power(noise, keeps[1] if keeps else None)
    scale = np.sqrt(pc / (pn + T(1e-8)) / T(np.power(10.0, snr / 10.0)) + T(1e-8))
    return clean + noise * scale, scale, pc, pn


def loudness(x, factors):
    x = x.copy()
    n = len(factors)
    step = len(x) // n
    for i, f in enumerate(factors):
        x[i * step: (i + 1) * step] = x.dtype.type(f) * x[i * step: (i + 1) * step]
    return x


def rate_threshold(x64: np.ndarray, rate: float) -> float:
    hist, edges = np.histogram(np.abs(x64), bins=1000)
    return edges[:-1][np.cumsum(hist) > (1 - rate) * len(x64)][0]


def edge_margin(x64: np.ndarray) -> float:
    """The smallest relative distance of an ``|x|`` from an edge of the 1000-bin histogram (the two end edges are samples themselves)."""
    a = np.abs(x64)
    edges = np.histogram_bin_edges(a, bins=1000)
    i = np.clip(np.searchsorted(edges, a), 1, 1000)
    d = np.minimum(np.abs(a - edges[i - 1]), np.abs(edges[i] - a))
    inner = (a != a.min()) & (a != a.max())
    return float((d[inner] / a.max()).min())


def clip(x, kind, a, b=0.0, threshold=None):
    """-> (clipped, threshold or 0, energy scale or 1)."""
    T = x.dtype.type
    if kind == "hard":
        return np.clip(x, -T(a), T(a)), a, 1.0
    if kind == "hard_on_rate":
        thr = rate_threshold(x.astype(np.float64), a) if threshold is None else threshold
        return np.clip(x, -T(thr), T(thr)), thr, 1.0
    if kind == "soft":
        m = x.max()
        return m * x / (np.abs(m) ** T(a) + np.abs(x) ** T(a) + T(1e-5)) ** (T(1) / T(a)), 0.0, 1.0
    orig = np.sqrt(np.mean(x ** 2))
    if kind == "sigmoid1":
        y = (2 / (1 + np.exp(-T(a) * x)) - 1) * T(b)
        thr = 0.0
    elif kind == "sigmoid2":
        xc = np.clip(x, -T(a), T(a))
        bb = T(1.5) * xc - T(0.3) * xc ** 2
        aa = np.where(bb > 0, T(4), T(0.5))
        y = T(b) * (2 / (1 + np.exp(-aa * bb)) - 1)
        thr = a
    else:
        raise ValueError(kind)
    es = orig / (np.sqrt(np.mean(y ** 2)) + T(1e-8))
    return y * es, thr, es


def packet_loss(x, frame, factors):
    f = np.asarray(factors, x.dtype)[np.arange(len(x)) // frame]
    return x * f


def volume(noisy, clean, mode, target, normalize, keeps=None):
    """The volume steps on the pair -> (noisy, clean, volume scale, clip scale, norm factor)."""
    T = noisy.dtype.type
    vs = cs = T(1)
    if mode != "none":
        if mode == "rms":
            ly = np.sqrt(masked_power(noisy, keeps[0] if keeps else None) + T(1e-8))
            lc = np.sqrt(masked_power(clean, keeps[1] if keeps else None) + T(1e-8))
        else:
            ly, lc = np.abs(noisy).max(), np.abs(clean).max()
        vs = T(target) / (max(ly, lc) + T(1e-6))
        noisy, clean = noisy * vs, clean * vs
        m = max(np.abs(noisy).max(), np.abs(clean).max())
        if m > 0.99:
            cs = T(0.99) / m
            noisy, clean = noisy * cs, clean * cs
    nf = max(np.abs(noisy).max(), np.abs(clean).max())
    if normalize:
        noisy, clean = noisy / nf * T(0.8), clean / nf * T(0.8)
    return noisy, clean, vs, cs, (nf if normalize else T(1))


def chain(x32, r: Recipe, noise32=None, h32=None, dtype=np.float64, decisions=None) -> dict:
    """The chain on one item (float32 inputs, everything after the load in ``dtype``).  -> the two outputs, the scalars in the order of
    ``_lib.DISTORT_SCALARS``, and the decisions taken: the kept frames, the clip-on-rate threshold, whether the volume clip fired.
    ``decisions`` (a dict from an earlier evaluation): hold those fixed, so that a longdouble evaluation measures rounding alone."""
    x = np.asarray(x32).astype(dtype)
    n = len(x)
    out = {"keep_clean": None, "keep_noise": None}
    d = decisions or {}
    full = target = x
    if r.reverb:
        full, target = reverberate(x, np.asarray(h32).astype(dtype))
    scale = pc = pn = 0.0
    noisy = full
    if r.snr is not None:
        nz = np.asarray(noise32[:n]).astype(dtype)
        fk = (vad_frames(full), vad_frames(nz)) if not d else (d["keep_clean"], d["keep_noise"])
        keeps = tuple(k[np.arange(n) // HOP] for k in fk)
        noisy, scale, pc, pn = add_noise(full, nz, r.snr, keeps)
        out["keep_clean"], out["keep_noise"] = fk
    if r.loudness:
        noisy = loudness(noisy, r.loudness)
    thr, es = 0.0, 1.0
    if r.clip_kind != "none":
        noisy, thr, es = clip(noisy, r.clip_kind, r.clip_a, r.clip_b, d.get("threshold") if r.clip_kind == "hard_on_rate" else None)
    out["threshold"] = thr
    if r.dc_offset is not None:
        noisy = noisy + dtype(r.dc_offset)
    if r.packet_frame:
        noisy = packet_loss(noisy, r.packet_frame, r.packet_factors)
    vk = None
    if r.volume == "rms":
        fk = (vad_frames(noisy), vad_frames(target)) if not d else d["keep_volume"]
        out["keep_volume"] = fk
        vk = tuple(k[np.arange(n) // HOP] for k in fk)
    out["peak_before_clip"] = None
    if r.volume != "none":
        lv = (max(math.sqrt(masked_power(noisy, vk[0]) + 1e-8), math.sqrt(masked_power(target, vk[1]) + 1e-8)) if r.volume == "rms"
              else max(np.abs(noisy).max(), np.abs(target).max()))
        out["peak_before_clip"] = float(max(np.abs(noisy).max(), np.abs(target).max()) * (r.volume_target / (lv + 1e-6)))
    noisy, target, vs, cs, nf = volume(noisy, target, r.volume, r.volume_target, r.normalize, vk)
    out.update(perturbed=noisy, clean=target,
               scalars=np.array([scale, thr, vs, nf, cs, pc, pn, es], dtype))
    return out


def err_ref(x32, r: Recipe, noise32=None, h32=None):
    """-> (the float64 restatement's result, its distance from the longdouble evaluation under the same decisions, relative to the peak)
    per output: ``{"perturbed": .., "clean": ..}``."""
    a = chain(x32, r, noise32, h32, np.float64)
    b = chain(x32, r, noise32, h32, LD, decisions=a)
    err = {}
    for k in ("perturbed", "clean"):
        peak = float(np.abs(b[k]).max())
        err[k] = float(np.abs(a[k].astype(LD) - b[k]).max()) / peak if peak > 0 else 0.0
    return a, err


# ---- signals --------------------------------------------------------------------------------------------------------------------------

def speechlike(n: int, seed: int, gaps: bool = True) -> np.ndarray:
    """float32 [n]: white noise under a 3 Hz syllabic envelope, peak 0.6; ``gaps``: 4000 samples of every 9000, from 2500 on, are 80 dB down
    (longer than a frame: the -50 dB rule drops the frames inside), with 200-sample ramps."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 24000.0
    x = rng.standard_normal(n) * (0.55 + 0.45 * np.sin(2 * np.pi * 3.0 * t + seed))
    if gaps:
        g = np.ones(n)
        for s in range(2500, n, 9000):
            g[s: s + 4000] = 1e-4
        k = np.ones(200) / 200
        x = x * np.convolve(np.pad(g, 100, mode="edge"), k, mode="same")[100: 100 + n]
    return (x / np.abs(x).max() * 0.6).astype(np.float32)


def make_rir(r: int, seed: int) -> np.ndarray:
    """float32 [r] through ``prepare_rir``: decaying noise behind a direct path of 1 at tap 0."""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal(r) * np.exp(-np.arange(r) / max(r / 6.0, 1.0)) * 0.3
    h[0] = 1.0
    out = prepare_rir(h)
    assert len(out) == r and out[0] == 1.0
    return out


def packet_factors(n: int, frame: int, seed: int):
    rng = np.random.default_rng(seed)
    return tuple(float(rng.choice([1.0, 1.0, 0.0, 0.125 * rng.uniform(0.1, 1.0)])) for _ in range(-(-n // frame)))


# ---- the cases ------------------------------------------------------------------------------------------------------------------------

# lengths: below one slice (and one VAD frame), just over one slice, a few slices and no multiple of 512; all leave a tail behind 5
# loudness intervals, and 480-sample packets leave a short last frame
SMALL = (1003, 4097, 10007)
SMALL_STRIDE = 10240
# past the re-reduction's 256 partials, next to a tiny item
SEAM = (256 * SLICE + 2 * SLICE + 77, 600)
SEAM_STRIDE = 257 * SLICE + 2 * SLICE
assert -(-SEAM[0] // SLICE) > 256

STAGES = {                          # one stage each; exact: one rounded operation per sample
    "hard": (True, dict(clip_kind="hard", clip_a=10 ** (-10.5 / 20))),
    "dc": (True, dict(dc_offset=0.0537)),
    "loud1": (True, dict(loudness=(0.37,))),
    "loud5": (True, dict(loudness=(0.37, 2.9, 1.0, 0.11, 9.3))),
    "packet": (True, dict(packet_frame=480)),
    "noise": (False, dict(snr=7.5)),
    "hard_on_rate": (False, dict(clip_kind="hard_on_rate", clip_a=0.1)),
    "soft": (False, dict(clip_kind="soft", clip_a=2.5)),
    "sigmoid1": (False, dict(clip_kind="sigmoid1", clip_a=2.0, clip_b=1.5)),
    "sigmoid2": (False, dict(clip_kind="sigmoid2", clip_a=10 ** (-6.0 / 20), clip_b=2.0)),
    "volume_peak": (False, dict(volume="peak", volume_target=0.31)),
    "volume_clip": (False, dict(volume="peak", volume_target=4.7)),
    "volume_rms": (False, dict(volume="rms", volume_target=0.05)),
    "normalize": (False, dict(normalize=True)),
}
CHAIN_CLIPS = (dict(clip_kind="hard_on_rate", clip_a=0.07), dict(clip_kind="sigmoid2", clip_a=10 ** (-3.0 / 20), clip_b=1.7),
               dict(clip_kind="soft", clip_a=3.1))
# (len, r): len + r - 1 = 1000 (identity), 1024 exactly (early == full), 1025, and two- and three-pass transforms
REVERB = ((1000, 1), (1019, 6), (1019, 7), (3000, 300), (40000, 900), ((1 << 19) - 6, 7))
REVERB_STRIDE, REVERB_RIR_STRIDE = 1 << 19, 1024
assert [1 << int(n + r - 2).bit_length() if n + r > 2 else 1 for n, r in REVERB] == [1024, 1024, 2048, 4096, 65536, 1 << 19]


def _recipe(n: int, seed: int, **kw) -> Recipe:
    r = Recipe(**kw)
    if r.packet_frame:
        r = dataclasses.replace(r, packet_factors=packet_factors(n, r.packet_frame, seed))
    return r


def _batch(lengths, stride, recipes, seed, rirs=None, rir_stride=1):
    B = len(lengths)
    clean = np.full((B, stride), PAD, np.float32)
    noise = np.full((B, stride), PAD, np.float32)
    rir = np.full((B, rir_stride), PAD, np.float32)
    for b, n in enumerate(lengths):
        clean[b, :n] = speechlike(n, seed + 10 * b)
        noise[b, :n] = 0.3 * speechlike(n, seed + 10 * b + 5)
        if rirs is not None:
            rir[b, : len(rirs[b])] = rirs[b]
    return dict(lengths=tuple(lengths), stride=stride, recipes=list(recipes), clean=clean, noise=noise, rir=rir,
                rir_lengths=[len(h) for h in rirs] if rirs is not None else None)


@functools.lru_cache(maxsize=None)
def build(name: str) -> dict:
    """The batch ``name``: float32 input rows (padding filled with 1e3), lengths and recipes.  Names: ``<stage>`` (the small lengths),
    ``<stage>@seam``, ``reverb``, ``chain``, ``chain@seam``."""
    stage, _, where = name.partition("@")
    lengths, stride = (SEAM, SEAM_STRIDE) if where == "seam" else (SMALL, SMALL_STRIDE)
    if stage == "reverb":
        rirs = [make_rir(r, 300 + i) for i, (_, r) in enumerate(REVERB)]
        return _batch([n for n, _ in REVERB], REVERB_STRIDE, [Recipe(reverb=True) for _ in REVERB], 77, rirs, REVERB_RIR_STRIDE)
    if stage == "chain":
        rirs = [make_rir(r, 400 + b) for b, r in zip(range(len(lengths)), (7, 130, 40))]
        recipes = [_recipe(n, 500 + b, reverb=True, snr=(12.5, 3.0, 21.0)[b], loudness=((0.4, 3.0), (2.2,), (0.3, 1.7, 0.9, 4.0, 0.6))[b],
                           dc_offset=(0.01, None, 0.12)[b], packet_frame=(480, 199, 0)[b], volume=("peak", "rms", "peak")[b],
                           volume_target=(0.4, 0.08, 6.0)[b], normalize=(True, False, True)[b], **CHAIN_CLIPS[b])
                   for b, n in enumerate(lengths)]
        return _batch(lengths, stride, recipes, 88, rirs, 256)
    if stage not in STAGES:
        raise KeyError(name)
    recipes = [_recipe(n, 600 + b, **STAGES[stage][1]) for b, n in enumerate(lengths)]
    return _batch(lengths, stride, recipes, 99)


CASES = tuple(STAGES) + tuple(s + "@seam" for s in ("noise", "hard_on_rate", "soft", "sigmoid1", "volume_rms", "packet")) + \
    ("reverb", "chain", "chain@seam")


def item(case: dict, b: int):
    """-> (x32, recipe, noise32, h32) of item b, trimmed to its lengths."""
    n = case["lengths"][b]
    h = case["rir"][b, : case["rir_lengths"][b]] if case["rir_lengths"] else None
    return case["clean"][b, :n], case["recipes"][b], case["noise"][b, :n], h


@functools.lru_cache(maxsize=None)
def expected(name: str):
    """Per item of ``build(name)``: (the float64 restatement's ``chain`` result, its ``err_ref``)."""
    case = build(name)
    return tuple(err_ref(*item(case, b)) for b in range(len(case["lengths"])))
