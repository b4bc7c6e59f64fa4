"""Chunked sampling of long recordings (no reference counterpart): the window geometry shared by the host code and the
``use_chunk_*`` entry points of libuse_hip.so, and the loop that runs a per-window function over groups of windows.

A spectrogram [B,1,F,T'] is cut along the frame axis into ``n`` windows of ``chunk_frames`` frames that start ``hop = chunk_frames -
overlap`` frames apart; frames of the last window beyond T' are zero.  The windows are the batch of the existing sampler, so one plan
and one captured graph per (group size, chunk_frames) serve every file length.  The enhanced windows are cross-faded back: for the
first ``overlap`` frames of window k >= 1 (j = 0 .. overlap - 1) window k weighs ``a_j = (j + 1) / (overlap + 1)`` and window k - 1
``1 - a_j``; every other frame is a copy from the one window that owns it.  ``overlap <= chunk_frames / 2``: no frame has more than
two sources.
"""
from __future__ import annotations

from numbers import Integral
from typing import Callable, NamedTuple, Sequence, Tuple


class ChunkPlan(NamedTuple):
    n: int                       # windows per item; 1 = no chunking (T' <= chunk_frames)
    hop: int                     # chunk_frames - overlap
    starts: Tuple[int, ...]      # first frame of every window, k * hop
    chunk_frames: int
    overlap: int
    Tp: int


def chunk_plan(Tp: int, chunk_frames: int, overlap: int) -> ChunkPlan:
    """The geometry of ``use_chunk_count`` (csrc/use_engine.cpp: chunk_geometry), with ``ValueError`` for what it refuses."""
    for name, v in (("Tp", Tp), ("chunk_frames", chunk_frames), ("overlap", overlap)):
        if isinstance(v, bool) or not isinstance(v, Integral):
            raise ValueError(f"{name}={v!r} must be an integer")
    Tp, chunk_frames, overlap = int(Tp), int(chunk_frames), int(overlap)
    if Tp < 64 or Tp % 64 != 0:
        raise ValueError(f"Tp={Tp}: the padded frame count must be a positive multiple of 64")
    if chunk_frames < 64 or chunk_frames % 64 != 0:
        raise ValueError(f"chunk_frames={chunk_frames} must be a positive multiple of 64")
    if overlap < 0 or overlap > chunk_frames // 2:
        raise ValueError(f"overlap={overlap} must lie in 0 ... chunk_frames / 2 = {chunk_frames // 2}")
    hop = chunk_frames - overlap
    n = 1 if Tp <= chunk_frames else -(-(Tp - overlap) // hop)
    return ChunkPlan(n, hop, tuple(k * hop for k in range(n)), chunk_frames, overlap, Tp)


def check_chunk_batch(chunk_batch: int) -> int:
    """``chunk_batch`` as an int, or ``ValueError``."""
    if isinstance(chunk_batch, bool) or not isinstance(chunk_batch, Integral) or chunk_batch < 1:
        raise ValueError(f"chunk_batch={chunk_batch!r} must be a positive integer")
    return int(chunk_batch)


def chunk_groups(total: int, chunk_batch: int) -> Sequence[Tuple[int, int]]:
    """[lo, hi) of every group of at most ``chunk_batch`` consecutive windows; the last group may be smaller."""
    chunk_batch = check_chunk_batch(chunk_batch)
    return [(lo, min(lo + chunk_batch, total)) for lo in range(0, total, chunk_batch)]


def map_chunked(fn: Callable, inputs: Sequence, chunk_frames: int, overlap: int, chunk_batch: int):
    """split -> ``fn`` per group -> merge.  ``inputs``: complex64 CUDA spectrograms [B,1,F,T'] of one shape (the same object may appear
    twice: it is split once); ``fn(g, lo, hi, windows)`` gets the windows [lo, hi) of every input and returns the group's result
    [hi - lo, 1, F, chunk_frames].  Returns the merged [B,1,F,T'] and the list of whatever else ``fn`` returned beside it."""
    import torch

    from .hip_engine import chunk_merge, chunk_split
    B, _, _, Tp = inputs[0].shape
    plan = chunk_plan(int(Tp), chunk_frames, overlap)
    # Tensors are told apart by identity, not by value: the samplers recognise the SDE's y among the conditioning with `c is y`
    # (ScoreModel.get_pc_sampler, the engine's cond argument), so an input that appears twice must give the same window object twice,
    # in the whole and in every group's slice.  tests/test_chunk_host.py pins this.
    split = {}
    for y in inputs:
        if id(y) not in split:
            split[id(y)] = chunk_split(y, chunk_frames, overlap)
    windows = [split[id(y)] for y in inputs]
    outs, extras = [], []
    for g, (lo, hi) in enumerate(chunk_groups(B * plan.n, chunk_batch)):
        sl = {id(w): w[lo:hi] for w in windows}             # one slice per distinct tensor: `c is y` stays true inside a group
        out, extra = fn(g, lo, hi, [sl[id(w)] for w in windows])
        outs.append(out); extras.append(extra)
    return chunk_merge(torch.cat(outs, dim=0), B, int(Tp), chunk_frames, overlap), extras
