"""The degradation simulator of the training data on the device (``use_distort``, csrc/use_distort.hip): what the reference's
``comm_distort_simu_dataset.__getitem__`` does to a clean excerpt - reverberation with the early part as the target, a noise recording
at a drawn SNR over the non-silent samples, loudness intervals, one of five clippers, a DC offset, packet loss and the volume steps
on the pair - per item of a batch, in fp64 after the load.  The host draws every parameter (``draw_recipes``: one numpy Generator per
item, seeded from the run's seed and the item's key as ``seeding.py`` seeds the sampler's noise, so that a file's recipe does not
depend on its batch); the device draws nothing.  ``distort_batch`` returns the reference's collated batch (``collate.py``), ready for
``SGMSEModule.training_step``.

    python -m universal_speech_enhancement_amd.distort clean_folder=clean/ noise_folder=noise/ rir_folder=rirs/ out_folder=out/ seed=0 [n=100]

writes ``out/clean/<rel>`` and ``out/noisy/<rel>`` for the first ``n`` files under ``clean/`` - the folder pair that
``predict ... data.data_folder=out/noisy data.clean_folder=out/clean`` scores into ``metrics.csv``.  RIRs are WAV or ``.npy`` files
(pickled RIRs are not read).  The stages that are not built - EQ, band reject, bass boost, spectral leakage, coloured noise, low-pass,
time-frequency holes, WebRTC, DRC, codecs, bit crush, speed / pitch - are refused by name.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import sys
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import CLIP_KINDS, DISTORT_SCALARS, VOLUME_MODES, UseDistortParams, UseHipError, check
from .seeding import item_seed, path_key

EARLY_TAPS = 6                 # the part of the RIR that stays in the clean target
VAD_HOP = 512
UNBUILT_CLIPS = ("sox", "pedal")
# probabilities of the reference's configuration whose stages use_distort does not run
UNBUILT_PROBS = ("eq_perturb_prob", "eq_much_gain_prob", "band_reject_prob", "bass_boost_prob", "spectral_leakage_prob", "colored_noise_prob",
                 "colored_noise_post_prob", "lowpass_prob", "spectral_time_freq_holes_prob", "webrtc_ns_prob", "webrtc_agc_prob", "drc_prob",
                 "codecs_prob", "bit_crush_prob", "speed_perturb_prob", "pitch_shift_prob", "only_noise_prob")


@dataclass
class Recipe:
    """One item's parameters, drawn by the host.  ``snr`` (dB): ``None`` adds no noise.  ``loudness``: one factor per interval (at most
    5).  ``clip_kind`` with ``clip_a`` / ``clip_b``: ``hard`` (the linear threshold ``10 ** (dB / 20)``), ``hard_on_rate`` (the rate
    of clipped samples, in (0, 1]), ``soft`` (the slope p), ``sigmoid1`` (slope, shape), ``sigmoid2`` (the linear threshold, the gain).
    ``packet_factors``: one factor per frame of ``packet_frame`` samples - 1 (kept), 0 (lost) or a decay.  ``volume``: ``none``,
    ``peak`` or ``rms`` with the linear ``volume_target``."""
    reverb: bool = False
    snr: Optional[float] = None
    loudness: Tuple[float, ...] = ()
    clip_kind: str = "none"
    clip_a: float = 0.0
    clip_b: float = 0.0
    dc_offset: Optional[float] = None
    packet_frame: int = 0
    packet_factors: Tuple[float, ...] = ()
    volume: str = "none"
    volume_target: float = 1.0
    normalize: bool = False


def default_config() -> dict:
    """``configs/data/distort.yaml`` of the package."""
    import yaml
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs", "data", "distort.yaml")) as f:
        return yaml.safe_load(f)


def check_config(cfg: dict) -> None:
    """``ValueError`` naming the key for a configuration that asks for a stage that is not built."""
    for k in UNBUILT_PROBS:
        if float(cfg.get(k) or 0) != 0:
            raise ValueError(f"{k}={cfg[k]}: this stage of the simulator is not built (its probability must be 0)")
    if float(cfg.get("clip_prob") or 0) > 0 and float(cfg.get("hard_clip_portion", 1)) < 1:
        bad = [t for t in cfg.get("soft_clip_types", ()) if t in UNBUILT_CLIPS or t not in CLIP_KINDS]
        if bad or not cfg.get("soft_clip_types"):
            raise ValueError(f"soft_clip_types={cfg.get('soft_clip_types')}: {bad or 'an empty list'} is not built (soft, sigmoid1, sigmoid2 are)")
    if cfg.get("packet_loss_on_vad") and float(cfg.get("packet_loss_prob") or 0) > 0:
        raise ValueError("packet_loss_on_vad=True: packet loss on WebRTC's VAD is not built")
    if cfg.get("random_volume") and not cfg.get("sync_random_volume", True):
        raise ValueError("sync_random_volume=False: only the volume steps on the pair are built")
    if cfg.get("random_volume") and cfg.get("volume_min_dB") is None and cfg.get("volume_min_sample") is None:
        raise ValueError("random_volume=True needs volume_min_dB / volume_max_dB or volume_min_sample / volume_max_sample")


def draw_recipe(cfg: dict, length: int, rng: np.random.Generator) -> Recipe:
    """One item's recipe from ``rng``, the stages in the reference's order."""
    r = Recipe()
    p = lambda k: float(cfg.get(k) or 0)                                           # noqa: E731
    add_noise = rng.random() < p("add_noise_prob")
    r.reverb = bool(rng.random() < p("reverb_prob"))
    if add_noise:
        r.snr = float(rng.uniform(cfg["snr_min"], cfg["snr_max"]))
    if rng.random() < p("loudness_perturb_prob"):
        lo, hi = float(cfg["loudness_min_factor"]), float(cfg["loudness_max_factor"])
        n = int(rng.integers(1, min(int(cfg["loudness_max_n_intervals"]), 5) + 1))
        r.loudness = tuple(float(rng.uniform(lo, 1.0) if rng.random() < 0.5 else rng.uniform(1.0, hi)) for _ in range(n))
    if rng.random() < p("clip_prob"):
        if rng.random() < float(cfg.get("hard_clip_portion", 1)):
            if cfg.get("hard_clip_on_rate", True):
                rate = 0.0
                while not rate > 0.0:                                              # the device refuses a rate of exactly 0
                    rate = float(rng.uniform(cfg["hard_clip_rate_min"], cfg["hard_clip_rate_max"]))
                r.clip_kind, r.clip_a = "hard_on_rate", rate
            else:
                db = float(rng.uniform(cfg["hard_clip_threshold_db_min"], cfg["hard_clip_threshold_db_max"]))
                r.clip_kind, r.clip_a = "hard", 10 ** (db / 20)
        else:
            kind = str(cfg["soft_clip_types"][int(rng.integers(len(cfg["soft_clip_types"])))])
            r.clip_kind = kind                                                     # the ranges are the defaults of the reference's classes
            if kind == "soft":
                r.clip_a = float(rng.uniform(1, 5))
            elif kind == "sigmoid1":
                r.clip_a, r.clip_b = float(rng.uniform(1, 5)), float(rng.uniform(1, 5))
            else:
                r.clip_a, r.clip_b = 10 ** (float(rng.uniform(-10, -1)) / 20), float(rng.uniform(1, 4))
    if rng.random() < p("dc_offset_prob"):
        r.dc_offset = float(rng.uniform(cfg["dc_offset_min"], cfg["dc_offset_max"]))
    if rng.random() < p("packet_loss_prob"):
        loss_rate = rng.uniform(cfg["packet_loss_rate_min"], cfg["packet_loss_rate_max"])
        frame_time = rng.uniform(cfg["packet_loss_frame_time_min"], cfg["packet_loss_frame_time_max"])
        r.packet_frame = max(1, int(int(cfg.get("sampling_rate", 24000)) * frame_time))
        factors = []
        for _ in range(-(-int(length) // r.packet_frame)):
            f = 1.0
            if rng.random() < loss_rate:
                hard = rng.random() < float(cfg.get("packet_loss_hard_loss_prob", 1.0))
                f = 0.0 if hard else float(rng.uniform(cfg["packet_loss_decay_rate_min"], cfg["packet_loss_decay_rate_max"]))
            factors.append(f)
        r.packet_factors = tuple(factors)
    if cfg.get("random_volume"):
        if cfg.get("volume_min_dB") is not None and cfg.get("volume_max_dB") is not None:
            r.volume_target = float(np.power(10.0, rng.uniform(cfg["volume_min_dB"], cfg["volume_max_dB"]) / 20.0))
        else:
            r.volume_target = float(rng.uniform(cfg["volume_min_sample"], cfg["volume_max_sample"]))
        r.volume = "rms" if cfg.get("use_rms_volume") else "peak"
    r.normalize = bool(cfg.get("output_normalize", False))
    return r


def draw_recipes(cfg: dict, lengths: Sequence[int], seed: int, keys: Sequence[int]) -> List[Recipe]:
    """One ``Recipe`` per item from the probabilities and ranges of ``cfg`` (``default_config()``: configs/data/distort.yaml).  Item b is
    drawn from ``np.random.default_rng(seeding.item_seed(seed, keys[b]))`` - ``keys[b]`` names the item independently of the batch (its
    index in the data set, or ``seeding.path_key`` of its relative path) - so the same key gives the same recipe in any batch."""
    check_config(cfg)
    if len(lengths) != len(keys):
        raise ValueError(f"{len(lengths)} lengths for {len(keys)} keys")
    return [draw_recipe(cfg, int(n), np.random.default_rng(item_seed(seed, int(k)))) for n, k in zip(lengths, keys)]


def prepare_rir(rir: np.ndarray) -> np.ndarray:
    """What the reference's ``get_rir`` does to a loaded impulse response, in float64: trimmed to start at its peak, divided by the
    peak; then cast to float32 for the device."""
    a = np.asarray(rir, dtype=np.float64)
    if a.ndim == 2:
        a = a[:, 0]
    if a.ndim != 1 or a.shape[0] < 1:
        raise ValueError(f"a RIR must be a non-empty 1-D array (or [taps, channels]), got shape {np.shape(rir)}")
    a = a[np.argmax(np.abs(a)):]
    peak = np.abs(a).max()
    if not peak > 0:
        raise ValueError("a RIR must not be all zeros")
    return (a / peak).astype(np.float32)


def params_of(recipes: Sequence[Recipe], lengths: Sequence[int], rir_lengths=None):
    """The ``use_distort_params`` records of a batch and the packet factors of all its items, one after another
    -> (ctypes array, float64 array)."""
    P = (UseDistortParams * len(recipes))()
    packets: List[float] = []
    for b, (r, n) in enumerate(zip(recipes, lengths)):
        q = P[b]
        if r.clip_kind not in CLIP_KINDS:
            raise ValueError(f"recipes[{b}].clip_kind={r.clip_kind!r} is not one of {sorted(CLIP_KINDS)}")
        if r.clip_kind in UNBUILT_CLIPS:
            raise ValueError(f"recipes[{b}].clip_kind={r.clip_kind!r} is not built")
        if r.volume not in VOLUME_MODES:
            raise ValueError(f"recipes[{b}].volume={r.volume!r} is not one of {sorted(VOLUME_MODES)}")
        if len(r.loudness) > 5:
            raise ValueError(f"recipes[{b}].loudness has {len(r.loudness)} factors (at most 5)")
        q.reverb = int(bool(r.reverb))
        q.rir_len = int(rir_lengths[b]) if r.reverb and rir_lengths is not None else 0
        q.add_noise = int(r.snr is not None)
        q.snr_lin = float(np.power(10.0, r.snr / 10.0)) if r.snr is not None else 1.0
        q.n_loud = len(r.loudness)
        for i, f in enumerate(r.loudness):
            q.loud[i] = float(f)
        q.clip_kind, q.clip_a, q.clip_b = CLIP_KINDS[r.clip_kind], float(r.clip_a), float(r.clip_b)
        q.dc, q.dc_offset = int(r.dc_offset is not None), float(r.dc_offset or 0.0)
        q.packet_frame = int(r.packet_frame)
        if r.packet_frame > 0:
            frames = -(-int(n) // int(r.packet_frame))
            if len(r.packet_factors) != frames:
                raise ValueError(f"recipes[{b}].packet_factors has {len(r.packet_factors)} entries, {frames} frames of {r.packet_frame} cover {n} samples")
            q.packet_off = len(packets)
            packets.extend(float(f) for f in r.packet_factors)
        q.volume, q.volume_target, q.normalize = VOLUME_MODES[r.volume], float(r.volume_target), int(bool(r.normalize))
    return P, np.asarray(packets, dtype=np.float64)


def _rows(name: str, t, B: int, dev) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise UseHipError(f"{name} must be a CUDA (ROCm) tensor: the simulator has no CPU implementation")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    if t.dim() == 1:
        t = t.unsqueeze(0)
    if t.dim() != 2 or t.shape[0] != B or t.device != dev:
        raise ValueError(f"{name} must be [{B}, width] on {dev}, got shape {tuple(t.shape)} on {t.device}")
    return t.contiguous()


def _int_array(name: str, v, B: int, default: int) -> np.ndarray:
    a = np.full(B, default, np.int64) if v is None else np.asarray(torch.as_tensor(v).cpu(), dtype=np.int64).reshape(-1)
    if a.shape[0] != B:
        raise ValueError(f"{name} has {a.shape[0]} entries for a batch of {B}")
    return np.ascontiguousarray(a, dtype=np.int32)


def distort_batch(clean: torch.Tensor, lengths, recipes: Sequence[Recipe], noise: Optional[torch.Tensor] = None,
                  rir: Optional[torch.Tensor] = None, out_dtype=torch.float32, noise_lengths=None, rir_lengths=None,
                  return_keep: bool = False) -> Dict:
    """One ``use_distort`` call on ``clean`` (float32 CUDA ``[B, L]``, item b valid for ``lengths[b]`` samples) under ``recipes``.
    ``noise``: float32 ``[B, Ln]`` rows of at least ``lengths[b]`` samples (``noise_lengths``: their own lengths, default ``Ln``) for the
    items with an ``snr``; ``rir``: float32 ``[B, R]`` rows from ``prepare_rir`` (``rir_lengths``: the taps of each, default ``R``) for
    the items with ``reverb``.  -> the reference's collated batch: ``clean`` (the target: the early-reverberated signal) and
    ``perturbed`` ``[B, L]`` in ``out_dtype`` (float32, or float64 whose cast the float32 rows are), zero past each length,
    ``sample_length`` (int32), ``SNR`` (``inf`` without noise), and ``scalars``: float64 ``[B, 8]`` in the order of
    ``_lib.DISTORT_SCALARS``.  ``return_keep``: also ``keep``, uint8 ``[B, 2, 1 + L // 512]``, the frames stage 2 kept in the clean signal
    and in the noise (items with an ``snr``)."""
    if not isinstance(clean, torch.Tensor) or not clean.is_cuda:
        raise UseHipError("clean must be a CUDA (ROCm) tensor: the simulator has no CPU implementation")
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError(f"out_dtype must be torch.float32 or torch.float64, got {out_dtype}")
    dev = clean.device
    B = 1 if clean.dim() == 1 else clean.shape[0]
    clean = _rows("clean", clean, B, dev)
    L = clean.shape[1]
    if len(recipes) != B:
        raise ValueError(f"{len(recipes)} recipes for a batch of {B}")
    lens = _int_array("lengths", lengths, B, L)
    if (lens < 1).any() or (lens > L).any():
        raise ValueError(f"lengths={lens.tolist()} must lie in 1 ... {L} (the width of the batch)")
    if noise is None and any(r.snr is not None for r in recipes):
        raise ValueError("a recipe has an snr and noise is None")
    if rir is None and any(r.reverb for r in recipes):
        raise ValueError("a recipe has reverb and rir is None")
    noise = _rows("noise", noise, B, dev) if noise is not None else None
    rir = _rows("rir", rir, B, dev) if rir is not None else None
    nlens = _int_array("noise_lengths", noise_lengths, B, noise.shape[1]) if noise is not None else None
    rlens = _int_array("rir_lengths", rir_lengths, B, rir.shape[1]) if rir is not None else None
    P, packets = params_of(recipes, lens, rlens)
    lib = _lib.lib()
    nbytes = 0
    for b in range(B):
        need = lib.use_distort_workspace(int(lens[b]), int(P[b].rir_len))
        if not need:
            raise ValueError(f"use_distort_workspace refuses len={int(lens[b])}, rir_len={int(P[b].rir_len)} (item {b}): len + rir_len - 1 is at most 2^24")
        nbytes = max(nbytes, need)
    work = torch.empty((nbytes + 15) // 16 * 2, dtype=torch.float64, device=dev)
    pert = torch.empty((B, L), dtype=out_dtype, device=dev)
    target = torch.empty((B, L), dtype=out_dtype, device=dev)
    scalars = torch.empty((B, len(DISTORT_SCALARS)), dtype=torch.float64, device=dev)
    pk = torch.from_numpy(packets).to(dev) if packets.size else None
    kstride = 1 + L // VAD_HOP
    keep = torch.zeros((B, 2, kstride), dtype=torch.uint8, device=dev) if return_keep else None
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int)) if a is not None else None                      # noqa: E731
    with torch.cuda.device(dev):
        check(lib.use_distort(clean.data_ptr(), noise.data_ptr() if noise is not None else None, rir.data_ptr() if rir is not None else None,
                              pk.data_ptr() if pk is not None else None, int(packets.size), ip(lens), ip(nlens), P, B, L,
                              noise.shape[1] if noise is not None else 0, rir.shape[1] if rir is not None else 0,
                              int(out_dtype == torch.float64), pert.data_ptr(), target.data_ptr(), scalars.data_ptr(),
                              keep.data_ptr() if keep is not None else None, kstride, work.data_ptr(), nbytes,
                              torch.cuda.current_stream(dev).cuda_stream), "use_distort")
    out = {"clean": target, "perturbed": pert, "sample_length": torch.from_numpy(lens.copy()),
           "SNR": [float(r.snr) if r.snr is not None else math.inf for r in recipes], "scalars": scalars}
    if return_keep:
        out["keep"] = keep
    return out


# ---- the command line ----------------------------------------------------------------------------------------------------------------

CLI_KEYS = ("clean_folder", "noise_folder", "rir_folder", "out_folder", "seed", "n", "sampling_rate", "batch_size", "device")


def parse_args(argv: Sequence[str]) -> dict:
    """``key=value`` arguments -> a dict; ``SystemExit`` naming an unknown key, a missing folder or a malformed number."""
    args: dict = {"seed": 0, "n": None, "sampling_rate": None, "batch_size": 4, "device": "cuda", "noise_folder": None, "rir_folder": None}
    for a in argv:
        k, sep, v = a.partition("=")
        if not sep or k not in CLI_KEYS:
            raise SystemExit(f"distort: {a!r} is not one of {', '.join(k + '=' for k in CLI_KEYS)}")
        args[k] = v
    for k in ("clean_folder", "out_folder"):
        if not args.get(k):
            raise SystemExit(f"distort: {k}= is required")
    for k in ("seed", "n", "sampling_rate", "batch_size"):
        if args[k] is not None:
            try:
                args[k] = int(args[k])
            except ValueError:
                raise SystemExit(f"distort: {k}={args[k]!r} must be an integer") from None
    if args["n"] is not None and args["n"] < 1 or args["batch_size"] < 1:
        raise SystemExit("distort: n= and batch_size= must be positive")
    for k in ("noise_folder", "rir_folder"):
        args[k] = args[k] or None
    return args


def list_files(folder: str, exts: Sequence[str]) -> List[str]:
    """The files under ``folder`` with one of ``exts``, as sorted POSIX-style relative paths."""
    out = []
    for root, _, names in os.walk(folder):
        out += [os.path.relpath(os.path.join(root, f), folder).replace(os.sep, "/") for f in names if f.lower().endswith(tuple(exts))]
    return sorted(out)


def load_rir(path: str, sampling_rate: int) -> np.ndarray:
    """A RIR from a WAV file (first channel, resampled to ``sampling_rate``) or a ``.npy`` array (no pickles), through ``prepare_rir``."""
    if path.lower().endswith(".npy"):
        return prepare_rir(np.load(path, allow_pickle=False))
    from .wavio import load_utterance
    return prepare_rir(load_utterance(path, sampling_rate, False)[0])


def fit_noise(noise: np.ndarray, length: int, rng: np.random.Generator) -> np.ndarray:
    """``length`` samples of a noise recording: a random excerpt of a longer one, a shorter one repeated (``get_noise``'s two cases)."""
    if len(noise) < 1:
        raise ValueError("an empty noise file")
    if len(noise) < length:
        noise = np.tile(noise, -(-length // len(noise)))
    start = int(rng.integers(0, len(noise) - length + 1))
    return noise[start: start + length]


def simulate_folder(args: dict, cfg: Optional[dict] = None) -> int:
    """The command line's work -> the number of pairs written."""
    from . import wavio
    cfg = dict(cfg or default_config())
    rate = int(args["sampling_rate"] or cfg.get("sampling_rate", 24000))
    cfg["sampling_rate"] = rate
    files = list_files(args["clean_folder"], (".wav",))[: args["n"]]
    if not files:
        raise SystemExit(f"distort: no .wav file under {args['clean_folder']}")
    noises = list_files(args["noise_folder"], (".wav",)) if args["noise_folder"] else []
    rirs = list_files(args["rir_folder"], (".wav", ".npy")) if args["rir_folder"] else []
    if not noises:
        cfg["add_noise_prob"] = 0
    if not rirs:
        cfg["reverb_prob"] = 0
    check_config(cfg)
    dev = torch.device(args["device"])
    for i in range(0, len(files), args["batch_size"]):
        rels = files[i: i + args["batch_size"]]
        keys = [path_key(r) for r in rels]
        clean = [wavio.load_utterance(os.path.join(args["clean_folder"], r), rate, False)[0] for r in rels]
        lens = [len(c) for c in clean]
        recipes = draw_recipes(cfg, lens, args["seed"], keys)
        L, B = max(lens), len(rels)
        x = np.zeros((B, L), np.float32)
        nz = np.zeros((B, L), np.float32)
        hs, hl = [np.zeros(1, np.float32)] * B, [1] * B
        for b, (r, k) in enumerate(zip(recipes, keys)):
            x[b, : lens[b]] = clean[b]
            pick = np.random.default_rng(item_seed(args["seed"] + 1, k))          # which noise, which excerpt, which RIR: the item's own stream
            if r.snr is not None:
                rec = wavio.load_utterance(os.path.join(args["noise_folder"], noises[int(pick.integers(len(noises)))]), rate, False)[0]
                nz[b, : lens[b]] = fit_noise(rec, lens[b], pick)
            if r.reverb:
                hs[b] = load_rir(os.path.join(args["rir_folder"], rirs[int(pick.integers(len(rirs)))]), rate)
                hl[b] = len(hs[b])
        h = np.zeros((B, max(hl)), np.float32)
        for b in range(B):
            h[b, : hl[b]] = hs[b]
        out = distort_batch(torch.from_numpy(x).to(dev), lens, recipes, noise=torch.from_numpy(nz).to(dev), rir=torch.from_numpy(h).to(dev),
                            rir_lengths=hl)
        pert, target = out["perturbed"].cpu().numpy(), out["clean"].cpu().numpy()
        for b, rel in enumerate(rels):
            for sub, a in (("clean", target), ("noisy", pert)):
                path = os.path.join(args["out_folder"], sub, rel)
                os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
                wavio.write_wav(path, a[b, : lens[b]], rate, wavio.FLOAT32)
    return len(files)


def main(argv=None) -> None:
    args = parse_args(sys.argv[1:] if argv is None else argv)
    n = simulate_folder(args)
    print(f"distort: wrote {n} pairs under {args['out_folder']}/clean and {args['out_folder']}/noisy")


if __name__ == "__main__":
    main()
