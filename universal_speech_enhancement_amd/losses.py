"""The convergence losses of the refine stage on the device (``use_spec_losses``, csrc/use_spec_loss.hip): the reference's
``WavSpecConvergence_Loss`` (``loss_function/monaural_loss.py:59-178``; the same arithmetic inside
``WavSpecConvergence_HIFIGAN_Vocoder_G_Loss``, the generator criterion of ``configs/model/LSGAN.yaml``) - a waveform L1, three magnitude
distances at four STFT resolutions and two mel distances - forward only, per item of a batch, in fp64, without a copy of the waveforms
to the host.  There is no backward pass, and the adversarial and feature-matching terms of the generator criterion are not here.

The functions take what ``metrics`` takes: float32 CUDA tensors, 1-D (one signal) or ``[B, L]`` (a zero-padded batch), and ``lengths``
(``None``: the full width; else ``B`` ints, ``min_length(sampling_rate) <= lengths[b] <= L``): samples past an item's length are never
read.  ``sampling_rate`` is 24000 or 48000, the rates at which the four frame lengths are powers of two.  There is no CPU implementation.

``score_files`` / ``write_csv`` are the file-level step of ``predict ... data.clean_folder=DIR data.convergence_losses=true``."""
from __future__ import annotations

import csv
import ctypes as C
import os
from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import UseHipError, check

COUNT = 15                                                 # USE_SPECLOSS_COUNT
WAV_L1, MAG_L2, MAG_LOG, MAG_NORM, MEL_LOG, MEL_L2 = 0, 1, 5, 9, 13, 14     # USE_SPECLOSS_*; the three MAG_* + r, r = 0..3
NAMES = ("wav_l1", "mag_l2", "mag_log", "mag_norm_l2", "mel_log", "mel_l2")
# the convergence weights of the reference's configs/model/LSGAN.yaml (loss_G)
LSGAN_ALPHAS = dict(alpha_wav_l1=0.1, alpha_mag_l2=1.0, alpha_mag_log=1.0, alpha_mag_norm_l2=0.5, alpha_mel_log=0.5, alpha_mel_l2=0.5)


def min_length(sampling_rate: int) -> int:
    """Reflect padding of the longest frame (2048 samples at 24 kHz, 4096 at 48 kHz) needs more than half of it."""
    return max(int(4096 * (sampling_rate / 48000)), 2048) // 2 + 1


def _signals(named) -> Tuple[list, int, int]:
    """What ``metrics._signals`` accepts; type, dtype and shape are judged before the device, so a host can see every refusal."""
    out, shape = [], None
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {t.dtype}")
        if t.dim() == 1:
            t = t.unsqueeze(0)
        if t.dim() != 2:
            raise ValueError(f"{name} must be 1-D or [B, L], got shape {tuple(t.shape)}")
        shape = shape or tuple(t.shape)
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {shape}")
        out.append(t)
    for (name, _), t in zip(named, out):
        if not t.is_cuda:
            raise UseHipError(f"{name} must be a CUDA (ROCm) tensor: the convergence losses have no CPU implementation")
    return [t.contiguous() for t in out], shape[0], shape[1]


def _lengths(lengths, B: int, L: int, sampling_rate: int):
    lens = np.full(B, L, np.int64) if lengths is None else np.asarray(torch.as_tensor(lengths).cpu(), dtype=np.int64).reshape(-1)
    if lens.shape[0] != B:
        raise ValueError(f"lengths has {lens.shape[0]} entries for a batch of {B}")
    lo = min_length(sampling_rate)
    if (lens < lo).any() or (lens > L).any():
        raise ValueError(f"lengths={lens.tolist()} must lie in {lo} ... {L} (the width of the batch)")
    return np.ascontiguousarray(lens, dtype=np.int32)


def spec_loss_terms(est: torch.Tensor, clean: torch.Tensor, lengths=None, sampling_rate: int = 24000) -> torch.Tensor:
    """-> float64 CUDA ``[B, 15]``, per item and unweighted: ``[WAV_L1]``, ``[MAG_L2 + r]``, ``[MAG_LOG + r]``, ``[MAG_NORM + r]`` for the
    four resolutions r in ascending n_fft, ``[MEL_LOG]``, ``[MEL_L2]`` - the reference's values at batch size 1 on exactly those samples."""
    if sampling_rate not in (24000, 48000):
        raise ValueError(f"sampling_rate={sampling_rate} must be 24000 or 48000 (the rates at which the four frame lengths are powers of two)")
    sig, B, L = _signals([("est", est), ("clean", clean)])
    lens = _lengths(lengths, B, L, sampling_rate)
    lib = _lib.lib()
    dev = sig[0].device
    nbytes = lib.use_spec_losses_workspace(B, L, sampling_rate)
    if not nbytes:
        raise ValueError(f"use_spec_losses_workspace refuses B={B}, L={L}, sampling_rate={sampling_rate}")
    work = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    out = torch.empty((B, COUNT), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib.use_spec_losses(sig[0].data_ptr(), sig[1].data_ptr(), lens.ctypes.data_as(C.POINTER(C.c_int)), B, L, sampling_rate,
                                  work.data_ptr(), nbytes, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "use_spec_losses")
    return out


def _six(v: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The reference's aggregation over the resolutions: mag_l2 is their SUM (monaural_loss.py:127, never divided), the other two means."""
    return {"wav_l1": v[:, WAV_L1], "mag_l2": v[:, MAG_L2:MAG_L2 + 4].sum(1), "mag_log": v[:, MAG_LOG:MAG_LOG + 4].sum(1) / 4,
            "mag_norm_l2": v[:, MAG_NORM:MAG_NORM + 4].sum(1) / 4, "mel_log": v[:, MEL_LOG], "mel_l2": v[:, MEL_L2]}


def convergence_losses(est: torch.Tensor, clean: torch.Tensor, lengths=None, sampling_rate: int = 24000) -> Dict[str, torch.Tensor]:
    """The six terms of the reference per item, unweighted: ``{name: float64 CUDA [B]}``, names ``NAMES``."""
    return _six(spec_loss_terms(est, clean, lengths, sampling_rate))


class WavSpecConvergence_Loss(torch.nn.Module):
    """The reference's class of that name: its constructor and its batch-dict contract.  ``forward(batch)`` reads ``batch["clean"]`` and
    ``batch[enhanced_key]`` (float32 CUDA ``[B, L]``) at full width and writes ``f"{loss_prefix}_wav_l1"`` ... ``f"{loss_prefix}_mel_l2"``
    and ``loss_prefix`` as 0-dim float64 CUDA tensors: the mean over the items of the weighted per-item value - at equal widths the
    reference's batch value.  Forward only: the tensors carry no graph."""

    def __init__(self, sampling_rate=48000, alpha_wav_l1=1.0, alpha_mag_l2=1.0, alpha_mag_log=1.0, alpha_mag_norm_l2=1.0, alpha_mel_log=1.0,
                 alpha_mel_l2=1.0, enhanced_key="fake", loss_prefix="loss_G"):
        super().__init__()
        self.sampling_rate = int(sampling_rate)
        self.alpha_wav_l1, self.alpha_mag_l2, self.alpha_mag_log = alpha_wav_l1, alpha_mag_l2, alpha_mag_log
        self.alpha_mag_norm_l2, self.alpha_mel_log, self.alpha_mel_l2 = alpha_mag_norm_l2, alpha_mel_log, alpha_mel_l2
        self.enhanced_key, self.loss_prefix = enhanced_key, loss_prefix

    def calc_convergence_loss(self, clean, enhanced):
        terms = convergence_losses(enhanced, clean, None, self.sampling_rate)
        return tuple(float(getattr(self, f"alpha_{k}")) * terms[k].mean() for k in NAMES)

    def forward(self, batch_data):
        terms = self.calc_convergence_loss(batch_data["clean"], batch_data[self.enhanced_key])
        for k, v in zip(NAMES, terms):
            batch_data[f"{self.loss_prefix}_{k}"] = v
        total = terms[0]
        for v in terms[1:]:
            total = total + v
        batch_data[f"{self.loss_prefix}"] = total
        return batch_data


def score_files(enhanced_path: str, clean_path: str, sampling_rate: int = 24000, normalize: bool = True, device="cuda",
                est=None, channel=None) -> Dict[str, float]:
    """One row of ``losses.csv``: the written enhanced file (its samples as they are in the file) against the clean file through the
    inference loader (``wavio.load_utterance``: first channel, resampled to ``sampling_rate``, peak-normalised when ``normalize``), over
    the shortest common length.  -> the six unweighted terms and ``total``, their ``LSGAN_ALPHAS``-weighted sum.  ``est`` (float32
    ``[n]``): the enhanced file's samples where the file itself is not at ``sampling_rate`` (``data.restore_rate``).  ``channel`` c
    (``data.channels=all``): channel c of the enhanced file against channel c of the clean file (``wavio.load_file_channels``)."""
    from .wavio import load_file_channels, load_utterance, read_wav
    if est is None:
        est, _ = read_wav(enhanced_path)
        est = (est if est.ndim == 1 else est[:, channel or 0]).astype(np.float32)
    if channel is None:
        clean, _ = load_utterance(clean_path, sampling_rate, normalize)
    else:
        clean = load_file_channels(clean_path, sampling_rate, normalize)[0][channel]
    n = min(len(est), len(clean))
    if n < min_length(sampling_rate):
        raise ValueError(f"{enhanced_path}: {n} common samples, the convergence losses need at least {min_length(sampling_rate)}")
    e, c = (torch.from_numpy(np.ascontiguousarray(a[:n])).to(device) for a in (est, clean))
    row = {k: float(v[0]) for k, v in convergence_losses(e, c, None, sampling_rate).items()}
    row["total"] = float(sum(LSGAN_ALPHAS[f"alpha_{k}"] * row[k] for k in NAMES))
    return row


def write_csv(path: str, rows: Sequence[Tuple], channel_column: bool = False) -> None:
    """``file, wav_l1, mag_l2, mag_log, mag_norm_l2, mel_log, mel_l2, total``: one row per file and a last row ``mean``; values as
    ``repr(float)`` (they read back as the same float64).  ``channel_column`` (``data.channels=all``): rows are ``(file, channel,
    losses)`` and a ``channel`` column follows ``file`` (empty in the ``mean`` row)."""
    cols = NAMES + ("total",)
    lead = ("file", "channel") if channel_column else ("file",)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(lead + cols)
        for *name, r in rows:
            w.writerow(list(name) + [repr(float(r[k])) for k in cols])
        if rows:
            w.writerow(["mean"] + [""] * (len(lead) - 1) + [repr(float(np.mean([row[-1][k] for row in rows]))) for k in cols])
