"""The hand-off between the two stages of the pipeline on the device (``use_wav_handoff``, csrc/use_handoff.hip): what the two-run
flow does to a stage-1 waveform between ``SGMSEModule.predict_step``'s writer and the batch ``LoadWavData`` hands to the refine stage -
the 16-bit quantisation of the file (or none, for float files), the loader's peak normalisation to 0.8 in float64, and its zero
padding - without the file, the host, or a second pass of the loader.  There is no CPU implementation.  ``wav_handoff_files``
(``use_wav_handoff_files``) is the same for a batch whose rows are the channels of files (``data.channels=all``): one peak per file."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import UseHipError, check
from .wavio import FLOAT32, PCM16

SUBTYPES = {"PCM_16": PCM16, "FLOAT": FLOAT32}             # the names of SGMSEModule(wav_subtype=...)


def _lengths(lengths, B: int, L: int) -> np.ndarray:
    lens = np.full(B, L, np.int64) if lengths is None else np.asarray(torch.as_tensor(lengths).cpu(), dtype=np.int64).reshape(-1)
    if lens.shape[0] != B:
        raise ValueError(f"lengths has {lens.shape[0]} entries for a batch of {B}")
    if (lens < 1).any() or (lens > L).any():
        raise ValueError(f"lengths={lens.tolist()} must lie in 1 ... {L} (the width of the batch)")
    return np.ascontiguousarray(lens, dtype=np.int32)


def wav_handoff(wav: torch.Tensor, lengths=None, subtype: str = "PCM_16", normalize: bool = True,
                out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``wav``: float32 CUDA ``[B, L]`` (or 1-D: one signal), item b valid for ``lengths[b]`` samples (``None``: the full width; the
    rest of a row is never read).  -> ``(out, peaks)``: ``out`` float32 ``[B, L]`` = what ``LoadWavData(normalize=normalize)`` yields
    for the files ``SGMSEModule(wav_subtype=subtype)`` writes from ``wav``, bit for bit, zero past each item's length; ``peaks``
    float64 ``[B]``, every item's peak after the quantisation.  ``out=wav`` works in place."""
    if not isinstance(wav, torch.Tensor) or not wav.is_cuda:
        raise UseHipError("wav must be a CUDA (ROCm) tensor: the hand-off has no CPU implementation")
    if wav.dtype != torch.float32:
        raise TypeError(f"wav must be float32, got {wav.dtype}")
    if subtype not in SUBTYPES:
        raise ValueError(f"unsupported WAV subtype {subtype!r} (PCM_16 or FLOAT)")
    one = wav.dim() == 1
    src = wav.unsqueeze(0) if one else wav
    if src.dim() != 2:
        raise ValueError(f"wav must be 1-D or [B, L], got shape {tuple(wav.shape)}")
    if out is not None and out is not wav:
        if not isinstance(out, torch.Tensor) or out.device != wav.device or out.dtype != torch.float32 or out.shape != wav.shape:
            raise ValueError("out must be a float32 tensor of wav's shape on wav's device")
    if not src.is_contiguous():
        if out is wav:
            raise ValueError("in place (out is wav) needs a contiguous wav")
        src = src.contiguous()
    dst = torch.empty_like(src) if out is None else (src if out is wav else (out.unsqueeze(0) if one else out))
    if not dst.is_contiguous():
        raise ValueError("out must be contiguous")
    B, L = src.shape
    lens = _lengths(lengths, B, L)
    lib = _lib.lib()
    dev = src.device
    nbytes = lib.use_wav_handoff_workspace(B, L)
    if not nbytes:
        raise ValueError(f"use_wav_handoff_workspace refuses B={B}, L={L}")
    work = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    peaks = torch.empty(B, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib.use_wav_handoff(src.data_ptr(), dst.data_ptr(), L, lens.ctypes.data_as(C.POINTER(C.c_int)), B, SUBTYPES[subtype],
                                  int(bool(normalize)), work.data_ptr(), nbytes, peaks.data_ptr(),
                                  torch.cuda.current_stream(dev).cuda_stream), "use_wav_handoff")
    return (dst[0] if one else dst), peaks


def wav_handoff_files(wav: torch.Tensor, lengths, channels, subtype: str = "PCM_16", normalize: bool = True,
                      out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The hand-off of a batch whose rows are the channels of files (``LoadWavData(channels="all")``; ``use_wav_handoff_files``):
    ``channels[f]`` consecutive rows of ``wav`` (float32 CUDA ``[rows, L]``) belong to file f and are valid for ``lengths[f]`` samples
    each (``None``: the full width).  Every sample goes through ``wav_handoff``'s arithmetic, but the peak is ONE per file, over all its
    rows: what ``LoadWavData(channels="all", normalize=normalize)`` yields for the C-channel files ``SGMSEModule(wav_subtype=subtype)``
    writes from ``wav``, bit for bit.  -> ``(out, peaks)``, ``peaks`` float64 ``[F]``.  ``out=wav`` works in place."""
    if not isinstance(wav, torch.Tensor) or not wav.is_cuda:
        raise UseHipError("wav must be a CUDA (ROCm) tensor: the hand-off has no CPU implementation")
    if wav.dtype != torch.float32:
        raise TypeError(f"wav must be float32, got {wav.dtype}")
    if subtype not in SUBTYPES:
        raise ValueError(f"unsupported WAV subtype {subtype!r} (PCM_16 or FLOAT)")
    if wav.dim() != 2:
        raise ValueError(f"wav must be [rows, L], got shape {tuple(wav.shape)}")
    chans = np.ascontiguousarray(np.asarray(channels, dtype=np.int64).reshape(-1), dtype=np.int32)
    if chans.shape[0] < 1 or (chans < 1).any() or int(chans.sum()) != wav.shape[0]:
        raise ValueError(f"channels={chans.tolist()} must be positive and add up to the {wav.shape[0]} rows of the batch")
    if out is not None and out is not wav:
        if not isinstance(out, torch.Tensor) or out.device != wav.device or out.dtype != torch.float32 or out.shape != wav.shape:
            raise ValueError("out must be a float32 tensor of wav's shape on wav's device")
    src = wav
    if not src.is_contiguous():
        if out is wav:
            raise ValueError("in place (out is wav) needs a contiguous wav")
        src = src.contiguous()
    dst = torch.empty_like(src) if out is None else (src if out is wav else out)
    if not dst.is_contiguous():
        raise ValueError("out must be contiguous")
    B, L = src.shape
    F = chans.shape[0]
    lens = _lengths(lengths, F, L)
    lib = _lib.lib()
    dev = src.device
    nbytes = lib.use_wav_handoff_files_workspace(B, L)
    if not nbytes:
        raise ValueError(f"use_wav_handoff_files_workspace refuses rows={B}, L={L}")
    work = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    peaks = torch.empty(F, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib.use_wav_handoff_files(src.data_ptr(), dst.data_ptr(), L, lens.ctypes.data_as(C.POINTER(C.c_int)),
                                        chans.ctypes.data_as(C.POINTER(C.c_int)), F, SUBTYPES[subtype], int(bool(normalize)),
                                        work.data_ptr(), nbytes, peaks.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
              "use_wav_handoff_files")
    return dst, peaks
