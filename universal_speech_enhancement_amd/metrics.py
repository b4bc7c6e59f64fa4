"""Evaluation metrics on the device (``use_metrics``, csrc/use_metrics.hip): the reference's ``energy_ratios`` (SI-SDR, SI-SIR, SI-SAR
over ``si_sdr_components``) and ``lsd`` of ``sgmse/util/other.py:15-62``, per item of a batch, in fp64, without a copy of the
waveforms to the host.

All functions take float32 CUDA tensors, 1-D (one signal) or ``[B, L]`` (a zero-padded batch), and ``lengths`` (``None``: the full
width; else ``B`` ints, ``256 <= lengths[b] <= L``): samples past an item's length are never read.  Results are float64 CUDA tensors
``[B]``.  There is no CPU implementation.

``stoi`` / ``intelligibility`` (``use_stoi``, csrc/use_stoi.hip) are STOI and ESTOI as ``pystoi.stoi(clean, est, fs, extended)`` defines
them, on the same terms: per item, fp64, bit-reproducible.  Their shortest item is one frame of 256 samples at 10 kHz.

``score_files`` / ``write_csv`` are the file-level step of ``predict ... data.clean_folder=DIR``."""
from __future__ import annotations

import csv
import ctypes as C
import os
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import UseHipError, check

NAMES = ("si_sdr", "si_sir", "si_sar", "lsd")              # USE_METRIC_SI_SDR ... USE_METRIC_LSD
MIN_LENGTH = 256                                           # reflect padding of the 510-point STFT needs more than 255 samples
STOI_NAMES = ("stoi", "estoi")                             # USE_STOI_STOI, USE_STOI_ESTOI; USE_STOI_FRAMES follows
STOI_RATES = (10000, 16000, 24000, 48000)
STOI_MIN_FRAMES = 30                                       # fewer STFT frames: both scores are 1e-5, as pystoi returns


def _signals(named) -> Tuple[list, int, int]:
    out, shape = [], None
    for name, t in named:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise UseHipError(f"{name} must be a CUDA (ROCm) tensor: the metrics have no CPU implementation")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {t.dtype}")
        if t.dim() == 1:
            t = t.unsqueeze(0)
        if t.dim() != 2:
            raise ValueError(f"{name} must be 1-D or [B, L], got shape {tuple(t.shape)}")
        shape = shape or tuple(t.shape)
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {shape}")
        out.append(t.contiguous())
    return out, shape[0], shape[1]


def _lengths(lengths, B: int, L: int, shortest: int = MIN_LENGTH):
    lens = np.full(B, L, np.int32) if lengths is None else np.asarray(torch.as_tensor(lengths).cpu(), dtype=np.int64).reshape(-1)
    if lens.shape[0] != B:
        raise ValueError(f"lengths has {lens.shape[0]} entries for a batch of {B}")
    if (lens < shortest).any() or (lens > L).any():
        raise ValueError(f"lengths={lens.tolist()} must lie in {shortest} ... {L} (the width of the batch)")
    return np.ascontiguousarray(lens, dtype=np.int32)


def _run(est: torch.Tensor, clean: torch.Tensor, noise: Optional[torch.Tensor], lengths) -> torch.Tensor:
    """-> float64 CUDA [B, 4] in the order of ``NAMES``; ``noise=None``: the three ratios are NaN."""
    sig, B, L = _signals([("s_hat", est), ("s", clean)] + ([("n", noise)] if noise is not None else []))
    lens = _lengths(lengths, B, L)
    lib = _lib.lib()
    dev = sig[0].device
    nbytes = lib.use_metrics_workspace(B, L)
    if not nbytes:
        raise ValueError(f"use_metrics_workspace refuses B={B}, L={L}")
    work = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    out = torch.empty((B, len(NAMES)), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib.use_metrics(sig[0].data_ptr(), sig[1].data_ptr(), sig[2].data_ptr() if noise is not None else None,
                              lens.ctypes.data_as(C.POINTER(C.c_int)), B, L, work.data_ptr(), nbytes, out.data_ptr(),
                              torch.cuda.current_stream(dev).cuda_stream), "use_metrics")
    return out


def energy_ratios(s_hat: torch.Tensor, s: torch.Tensor, n: torch.Tensor, lengths=None):
    """``(si_sdr, si_sir, si_sar)`` in dB, the reference's ``energy_ratios(s_hat, s, n)`` per item."""
    out = _run(s_hat, s, n, lengths)
    return out[:, 0], out[:, 1], out[:, 2]


def lsd(s_hat: torch.Tensor, s: torch.Tensor, lengths=None) -> torch.Tensor:
    """The reference's ``lsd(s_hat, s)`` per item: ``sqrt(mean |2 log(eps + |S_hat|) - 2 log(eps + |S|)|)`` at n_fft 510, hop 128."""
    return _run(s_hat, s, None, lengths)[:, 3]


def evaluate(est: torch.Tensor, clean: torch.Tensor, noisy: torch.Tensor, lengths=None) -> Dict[str, torch.Tensor]:
    """All four metrics of ``est`` against ``clean``; the noise is ``noisy - clean``.  -> ``{name: float64 [B]}``, names ``NAMES``."""
    sig, _, _ = _signals([("est", est), ("clean", clean), ("noisy", noisy)])
    out = _run(sig[0], sig[1], sig[2] - sig[1], lengths)
    return {name: out[:, i] for i, name in enumerate(NAMES)}


def stoi_min_length(sampling_rate: int) -> int:
    """The shortest item ``use_stoi`` takes: one frame of 256 samples after resampling to 10 kHz (613 samples at 24 kHz)."""
    if sampling_rate not in STOI_RATES:
        raise ValueError(f"sampling_rate={sampling_rate}: STOI is built for {STOI_RATES}")
    return 255 * sampling_rate // 10000 + 1


def _run_stoi(est: torch.Tensor, clean: torch.Tensor, lengths, sampling_rate: int) -> torch.Tensor:
    """-> float64 CUDA [B, 3]: stoi, estoi, and the number of STFT frames they were taken over."""
    sig, B, L = _signals([("s_hat", est), ("s", clean)])
    lens = _lengths(lengths, B, L, stoi_min_length(sampling_rate))
    lib = _lib.lib()
    dev = sig[0].device
    nbytes = lib.use_stoi_workspace(B, L, sampling_rate)
    if not nbytes:
        raise ValueError(f"use_stoi_workspace refuses B={B}, L={L}, sampling_rate={sampling_rate}")
    work = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    out = torch.empty((B, 3), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib.use_stoi(sig[0].data_ptr(), sig[1].data_ptr(), lens.ctypes.data_as(C.POINTER(C.c_int)), B, L, sampling_rate,
                           work.data_ptr(), nbytes, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "use_stoi")
    return out


def stoi(s_hat: torch.Tensor, s: torch.Tensor, lengths=None, sampling_rate: int = 24000, extended: bool = False) -> torch.Tensor:
    """STOI (``extended``: ESTOI) of ``s_hat`` against the clean ``s`` per item, ``pystoi.stoi(s, s_hat, sampling_rate, extended)`` without
    its dither; ``1e-5`` for an item with fewer than 30 frames left after the silent frames are removed."""
    return _run_stoi(s_hat, s, lengths, sampling_rate)[:, 1 if extended else 0]


def intelligibility(s_hat: torch.Tensor, s: torch.Tensor, lengths=None, sampling_rate: int = 24000) -> Dict[str, torch.Tensor]:
    """Both scores from one call -> ``{"stoi", "estoi", "stoi_frames"}``, float64 ``[B]`` each; ``stoi_frames`` is the number of STFT
    frames behind the scores (under 30: both are ``1e-5``)."""
    out = _run_stoi(s_hat, s, lengths, sampling_rate)
    return {"stoi": out[:, 0], "estoi": out[:, 1], "stoi_frames": out[:, 2]}


def score_files(enhanced_path: str, clean_path: str, noisy_path: str, sampling_rate: int = 24000, normalize: bool = True,
                device="cuda", est=None, channel=None, intelligibility: bool = False) -> Dict[str, float]:
    """One row of ``metrics.csv``: the written enhanced file (its samples as they are in the file) against the clean file, with the
    noisy input as the noise source; clean and noisy through the inference loader (``wavio.load_utterance``: first channel,
    resampled to ``sampling_rate``, peak-normalised when ``normalize``).  Files of different lengths are scored over the shortest,
    as the reference's ``si_sdr_torch`` does (``other.py:111-113``).  ``est`` (float32 ``[n]``): the enhanced file's samples where the
    file itself is not at ``sampling_rate`` (``data.restore_rate``); ``enhanced_path`` then only names the row.  ``channel`` c
    (``data.channels=all``): channel c of the enhanced file against channel c of the clean file, channel c of the noisy file as the
    noise source, clean and noisy through ``wavio.load_file_channels`` (one gain per file).  ``intelligibility``: the row also holds
    ``stoi`` and ``estoi`` of the same samples, and ``stoi_frames``, which is no column of the CSV."""
    from .wavio import load_file_channels, load_utterance, read_wav
    if est is None:
        est, _ = read_wav(enhanced_path)
        est = (est if est.ndim == 1 else est[:, channel or 0]).astype(np.float32)
    if channel is None:
        clean, _ = load_utterance(clean_path, sampling_rate, normalize)
        noisy, _ = load_utterance(noisy_path, sampling_rate, normalize)
    else:
        clean = load_file_channels(clean_path, sampling_rate, normalize)[0][channel]
        noisy = load_file_channels(noisy_path, sampling_rate, normalize)[0][channel]
    n = min(len(est), len(clean), len(noisy))
    if n < MIN_LENGTH:
        raise ValueError(f"{enhanced_path}: {n} common samples, the metrics need at least {MIN_LENGTH}")
    t = [torch.from_numpy(np.ascontiguousarray(a[:n])).to(device) for a in (est, clean, noisy)]
    row = {k: float(v[0]) for k, v in evaluate(*t).items()}
    if intelligibility:
        if n < stoi_min_length(sampling_rate):
            raise ValueError(f"{enhanced_path}: {n} common samples, STOI needs at least {stoi_min_length(sampling_rate)}")
        out = _run_stoi(t[0], t[1], None, sampling_rate)[0].tolist()
        row.update(stoi=out[0], estoi=out[1], stoi_frames=out[2])
    return row


def write_csv(path: str, rows: Sequence[Tuple], channel_column: bool = False, names: Sequence[str] = NAMES) -> None:
    """``file, si_sdr, si_sir, si_sar, lsd`` (``names``; ``NAMES + STOI_NAMES`` appends ``stoi, estoi``): one row per file and a last row
    ``mean``; values with 17 significant digits (they read back as the same float64).  ``channel_column`` (``data.channels=all``): rows
    are ``(file, channel, metrics)``, one per file and
    channel, and a ``channel`` column follows ``file`` (empty in the ``mean`` row)."""
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    lead = ("file", "channel") if channel_column else ("file",)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(lead + tuple(names))
        for *name, r in rows:
            w.writerow(list(name) + [repr(float(r[k])) for k in names])
        if rows:
            w.writerow(["mean"] + [""] * (len(lead) - 1) + [repr(float(np.mean([row[-1][k] for row in rows]))) for k in names])
