"""WAV files and the loader's FFT resampling through the library's host functions (``use_wav_read`` / ``use_wav_write`` /
``use_resample_fft`` / ``use_load_utterance``, include/use_hip.h): the reference's ``sf.read`` -> first channel ->
``librosa.resample(res_type="fft")`` -> peak normalisation (``src/data/components/loadwav_dataset.py:90-120``) and
``sf.write`` (``src/models/SGMSE_module.py:80``) without soundfile / librosa / scipy.

``resample_fft_device`` / ``load_batch_device`` (``use_resample_fft_dev`` / ``use_load_items_dev``, csrc/use_resample.hip): the same
resampling, peak normalisation, cast and the loader's zero-padded collation on the device; the host only decodes the files.  There is
no CPU implementation of the two.

``store_batch_device`` (``use_store_items_dev``, csrc/use_resample.hip): the way out - a batch of model-rate float32 rows on the device,
resampled back to each file's own frame count and quantised to the writer's 16-bit codes (or kept as float32), one call and one copy per
batch; ``store_items_host`` is the same arithmetic on the host, ``write_wav_pcm16`` (``use_wav_write_pcm16``) writes ready-made codes.

Files of several channels (``data.channels=all``): ``load_file_channels`` (host) and ``load_batch_device(channels="all")``
(``use_load_files_dev``) make every channel of a file a row under one gain per file; ``store_batch_device(channels=...)``
(``use_store_files_dev``) / ``store_files_host`` bring the rows of a file back as one interleaved ``[frames, channels]`` array.

The source's level (``data.restore_level``): the loaders can hand out the peak they divided by (``return_peak`` / ``return_peaks``),
``source_gain`` makes the gain of it, and every store function takes ``gains`` and applies them in fp64 before its rounding to float32."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._lib import UseHipError, check, lib

PCM16, FLOAT32 = 0, 1


def read_wav(path: str):
    """-> (float64 array [frames] or [frames, channels], sample rate), scaled like ``soundfile.read``."""
    p, n, ch, sr = C.POINTER(C.c_double)(), C.c_int64(), C.c_int(), C.c_int()
    check(lib().use_wav_read(os.fsencode(path), C.byref(p), C.byref(n), C.byref(ch), C.byref(sr)), "use_wav_read")
    try:
        a = np.ctypeslib.as_array(p, shape=(n.value * ch.value,)).copy() if n.value else np.zeros(0)
    finally:
        lib().use_free(p)
    return (a if ch.value == 1 else a.reshape(n.value, ch.value)), sr.value


def write_wav(path: str, wav: np.ndarray, sample_rate: int, subtype: int = PCM16) -> None:
    """``soundfile.write(path, wav, sample_rate)``: 16-bit PCM by default (soundfile's default WAV subtype), or 32-bit float."""
    a = np.ascontiguousarray(wav, dtype=np.float32)
    frames, ch = (a.shape[0], 1) if a.ndim == 1 else a.shape
    check(lib().use_wav_write(os.fsencode(path), a.ctypes.data_as(C.c_void_p), frames, ch, int(sample_rate), subtype), "use_wav_write")


def wav_info(path: str):
    """-> (frames, channels, sample rate) from the file's chunk headers alone (``use_wav_info``): what ``read_wav`` would report."""
    n, ch, sr = C.c_int64(), C.c_int(), C.c_int()
    check(lib().use_wav_info(os.fsencode(path), C.byref(n), C.byref(ch), C.byref(sr)), "use_wav_info")
    return n.value, ch.value, sr.value


def resampled_length(frames: int, sr: int, target: int) -> int:
    """The length ``load_utterance`` gives a file of ``frames`` frames at ``sr`` (``use_resampled_length``: librosa's ratio-first
    rounding; ``target`` 0 / None or equal to ``sr``: ``frames``)."""
    n = lib().use_resampled_length(int(frames), int(sr), int(target or 0))
    if n < 0:
        raise ValueError(f"resampled_length: bad arguments frames={frames}, sr={sr}")
    return n


def resample_fft(x: np.ndarray, num: int) -> np.ndarray:
    """``scipy.signal.resample(x, num)`` for a real 1-D signal (float64)."""
    a = np.ascontiguousarray(x, dtype=np.float64)
    y = np.empty(int(num), np.float64)
    check(lib().use_resample_fft(a.ctypes.data_as(C.c_void_p), a.shape[0], int(num), y.ctypes.data_as(C.c_void_p)), "use_resample_fft")
    return y


def load_utterance(path: str, sampling_rate: int = 24000, normalize: bool = True, return_peak: bool = False):
    """One item of the reference's inference dataset: -> (float32 [L], sample rate).  ``return_peak``: -> (..., peak), the float64 ``mx``
    the loader divided by (``use_load_utterance_peak``), or ``None`` without ``normalize``."""
    p, n, sr = C.POINTER(C.c_float)(), C.c_int64(), C.c_int()
    if return_peak:
        mx = C.c_double(0.0)
        check(lib().use_load_utterance_peak(os.fsencode(path), int(sampling_rate or 0), int(bool(normalize)), C.byref(p), C.byref(n),
                                            C.byref(sr), C.byref(mx)), "use_load_utterance_peak")
    else:
        check(lib().use_load_utterance(os.fsencode(path), int(sampling_rate or 0), int(bool(normalize)), C.byref(p), C.byref(n), C.byref(sr)),
              "use_load_utterance")
    try:
        a = np.ctypeslib.as_array(p, shape=(n.value,)).copy()
    finally:
        lib().use_free(p)
    if return_peak:
        return a, sr.value, (np.float64(mx.value) if normalize else None)
    return a, sr.value


def source_gain(peak) -> np.float64:
    """The gain that undoes the loader's peak normalisation (``data.restore_level``): ``mx / 0.8``, one float64 division; exactly 1
    without a peak (``normalize=false``), 0 for a silent file."""
    return np.float64(1.0) if peak is None else np.float64(peak) / np.float64(0.8)


CHANNEL_MODES = ("first", "all")                            # data.channels


def check_channels(channels: str) -> str:
    if channels not in CHANNEL_MODES:
        raise ValueError(f"channels={channels!r}: 'first' (the first channel of every file, the reference's loader) or 'all'")
    return channels


def load_file_channels(path: str, sampling_rate: int = 24000, normalize: bool = True, return_peak: bool = False):
    """Every channel of a file as an item of its own (``data.channels=all``): -> (float32 ``[C, L]``, sample rate).  Each channel is
    resampled like ``load_utterance``'s; the gain is ONE per file, so that the channels keep their level relation: ``mx = max |v|`` over
    all channels after resampling, in float64, by ``fabs(v) > mx`` (a NaN is never the peak), every channel ``v / mx * 0.8`` with two
    roundings.  A silent channel of a file that is not silent stays exact zeros, a silent file gives NaN, a mono file is
    ``load_utterance``'s row.  ``return_peak``: -> (..., peak), that ``mx`` (``None`` without ``normalize``)."""
    frames, ch, _ = wav_info(path)
    if ch == 1:
        a, sr, mx = load_utterance(path, sampling_rate, normalize, return_peak=True)
        return (a[None], sr, mx) if return_peak else (a[None], sr)
    a, sr = read_wav(path)
    if frames < 1:
        raise UseHipError(f"load_file_channels: '{path}' holds no samples")
    target = int(sampling_rate or 0)
    x = np.ascontiguousarray(a.T)                           # [C, frames], float64
    if target > 0 and target != sr:
        num = resampled_length(frames, sr, target)
        x = np.stack([resample_fft(c, num) for c in x])
        sr = target
    mx = None
    if normalize:
        mag = np.abs(x)
        mag = mag[~np.isnan(mag)]
        mx = np.float64(mag.max()) if mag.size else np.float64(0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            x = x / mx * 0.8
    return (x.astype(np.float32), sr, mx) if return_peak else (x.astype(np.float32), sr)


_WORK = {}                                                  # device -> the cached workspace of the device loader (uint8, grown on demand)


def _workspace(dev, nbytes: int):
    import torch
    w = _WORK.get(dev)
    if w is None or w.numel() < nbytes:
        _WORK.pop(dev, None)                                # let the old one go before the larger one is allocated
        w = _WORK[dev] = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)
    return w


def _device_workspace_bytes(n: int, num: int) -> int:
    nbytes = lib().use_resample_workspace(int(n), int(num))
    if not nbytes:
        raise ValueError(f"use_resample_workspace refuses n={n}, num={num} (each must lie in 1 ... 2^24)")
    return nbytes


def resample_fft_device(x, num: int):
    """``scipy.signal.resample(x, num)`` for a real 1-D signal on the device: ``x`` a float64 CUDA tensor -> float64 CUDA ``[num]``
    (``use_resample_fft_dev``)."""
    import torch
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise UseHipError("x must be a CUDA (ROCm) tensor: the device resampler has no CPU implementation")
    if x.dtype != torch.float64 or x.dim() != 1:
        raise TypeError(f"x must be a 1-D float64 tensor, got {x.dtype} of shape {tuple(x.shape)}")
    x = x.contiguous()
    n, num = x.shape[0], int(num)
    nbytes = _device_workspace_bytes(n, num)
    dev = x.device
    y = torch.empty(num, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        work = _workspace(dev, nbytes)
        check(lib().use_resample_fft_dev(x.data_ptr(), n, num, y.data_ptr(), work.data_ptr(), work.numel(),
                                         torch.cuda.current_stream(dev).cuda_stream), "use_resample_fft_dev")
    return y


def _load_files_device(paths, sampling_rate, normalize, dev, max_samples, return_peaks=False):
    """``load_batch_device(channels="all")``: every file uploaded once, interleaved as ``read_wav`` returns it; the rows of the device
    files are formed by one ``use_load_files_dev`` call per run of them."""
    import torch
    target = int(sampling_rate or 0)
    limit = min(int(max_samples), 2 ** 24)
    sigs, ns, nums, chans, rates, host_files = [], [], [], [], [], {}
    for f, path in enumerate(paths):
        a, sr = read_wav(path)
        n, ch = a.shape[0], (1 if a.ndim == 1 else a.shape[1])
        if n < 1:
            raise UseHipError(f"load_batch_device: '{path}' holds no samples")
        num = resampled_length(n, sr, target)
        if max(n, num) * ch > limit or ch > 64:             # counted as frames x channels
            host_files[f] = load_file_channels(path, target, normalize, return_peak=True)[::2]
            sigs.append(None)
        else:
            sigs.append(np.ascontiguousarray(a).reshape(-1))
        ns.append(n)
        nums.append(num)
        chans.append(ch)
        rates += [target if target > 0 else sr] * ch
    F, stride = len(ns), max(nums)
    row0 = np.concatenate([[0], np.cumsum(chans)]).astype(np.int64)
    lens = np.repeat(np.asarray(nums, dtype=np.int32), chans)
    want = bool(return_peaks and normalize)
    with torch.cuda.device(dev):
        wav = torch.empty(int(row0[-1]), stride, dtype=torch.float32, device=dev)
        peaks = torch.zeros(F, dtype=torch.float64, device=dev) if want else None
        xs = [None if s is None else torch.from_numpy(s).to(dev) for s in sigs]
        stream = torch.cuda.current_stream(dev).cuda_stream
        f = 0
        while f < F:
            if f in host_files:
                rows = torch.from_numpy(host_files[f][0])
                wav[row0[f]: row0[f + 1], : rows.shape[1]] = rows.to(dev)
                wav[row0[f]: row0[f + 1], rows.shape[1]:] = 0
                f += 1
                continue
            e = f
            while e < F and e not in host_files:
                e += 1
            k = e - f
            work = _workspace(dev, max(lib().use_load_files_workspace(ns[i], nums[i], chans[i]) for i in range(f, e)))
            ptrs = (C.c_void_p * k)(*[xs[i].data_ptr() for i in range(f, e)])
            args = (ptrs, (C.c_int64 * k)(*ns[f:e]), (C.c_int64 * k)(*nums[f:e]), (C.c_int * k)(*chans[f:e]), k, int(bool(normalize)),
                    wav[int(row0[f])].data_ptr(), stride, work.data_ptr(), work.numel())
            if want:
                check(lib().use_load_files_dev_peak(*args, peaks[f:].data_ptr(), stream), "use_load_files_dev_peak")
            else:
                check(lib().use_load_files_dev(*args, stream), "use_load_files_dev")
            f = e
        if want:
            peaks = peaks.cpu().numpy()                     # the one small copy of the batch
    if not return_peaks:
        return wav, lens, rates, chans
    if want:
        for f, (_, mx) in host_files.items():
            peaks[f] = mx
    return wav, lens, rates, chans, peaks


def load_batch_device(paths, sampling_rate: int = 24000, normalize: bool = True, device="cuda", max_samples: int = 2 ** 24,
                      channels: str = "first", return_peaks: bool = False):
    """The batch ``LoadWavData`` builds from ``paths``, formed on the device: -> (float32 ``[B, Lmax]`` on ``device``, int32 lengths
    ``[B]`` (host), sample rates).  The host decodes every file (``read_wav``) and uploads the first channel as float64; resampling to
    ``sampling_rate`` (0 / None: keep) at the length ``resampled_length`` gives, peak normalisation, the cast and the zero padding run
    in one ``use_load_items_dev`` call.  A file with more than ``max_samples`` samples before or after resampling goes through
    ``load_utterance`` on the host instead: its row has the host loader's bits.

    ``channels="all"``: a file of C channels gives C consecutive rows, in channel order, under ONE gain (``load_file_channels``); the
    whole interleaved file is uploaded and ``use_load_files_dev`` forms its rows.  -> (wav ``[rows, Lmax]``, lengths and rates per ROW,
    channel counts per FILE).  ``max_samples`` then counts frames x channels; a longer file takes ``load_file_channels`` on the host.

    ``return_peaks``: -> (..., peaks), the float64 ``mx`` every file was divided by (host array, one per FILE; ``use_load_items_dev_peak``
    / ``use_load_files_dev_peak`` write the divisor itself and one small copy brings the batch's home; a host row has the host loader's),
    or ``None`` without ``normalize``."""
    import torch
    check_channels(channels)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"load_batch_device needs a CUDA (ROCm) device, got {dev}: the device loader has no CPU implementation")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if channels == "all":
        return _load_files_device(paths, sampling_rate, normalize, dev, max_samples, return_peaks)
    target = int(sampling_rate or 0)
    limit = min(int(max_samples), 2 ** 24)
    sigs, ns, nums, rates, host_rows = [], [], [], [], {}
    for b, path in enumerate(paths):
        a, sr = read_wav(path)
        n = a.shape[0]
        if n < 1:
            raise UseHipError(f"load_batch_device: '{path}' holds no samples")
        num = resampled_length(n, sr, target)
        if max(n, num) > limit:
            host_rows[b] = load_utterance(path, target, normalize, return_peak=True)[::2]
            sigs.append(None)
        else:
            sigs.append(np.ascontiguousarray(a if a.ndim == 1 else a[:, 0]))      # first channel (loadwav_dataset.py:93-94)
        ns.append(n)
        nums.append(num)
        rates.append(target if target > 0 else sr)
    B, stride = len(ns), max(nums)
    lens = np.asarray(nums, dtype=np.int32)
    want = bool(return_peaks and normalize)
    with torch.cuda.device(dev):
        wav = torch.empty(B, stride, dtype=torch.float32, device=dev)
        peaks = torch.zeros(B, dtype=torch.float64, device=dev) if want else None
        xs = [None if s is None else torch.from_numpy(s).to(dev) for s in sigs]
        stream = torch.cuda.current_stream(dev).cuda_stream
        b = 0
        while b < B:                                        # one call per run of rows that the device forms: one call without host rows
            if b in host_rows:
                row = torch.from_numpy(host_rows[b][0])
                wav[b, : row.shape[0]] = row.to(dev)
                wav[b, row.shape[0]:] = 0
                b += 1
                continue
            e = b
            while e < B and e not in host_rows:
                e += 1
            k = e - b
            work = _workspace(dev, max(_device_workspace_bytes(ns[i], nums[i]) for i in range(b, e)))
            ptrs = (C.c_void_p * k)(*[xs[i].data_ptr() for i in range(b, e)])
            args = (ptrs, (C.c_int64 * k)(*ns[b:e]), (C.c_int64 * k)(*nums[b:e]), k, int(bool(normalize)), wav[b].data_ptr(), stride,
                    work.data_ptr(), work.numel())
            if want:
                check(lib().use_load_items_dev_peak(*args, peaks[b:].data_ptr(), stream), "use_load_items_dev_peak")
            else:
                check(lib().use_load_items_dev(*args, stream), "use_load_items_dev")
            b = e
        if want:
            peaks = peaks.cpu().numpy()                     # the one small copy of the batch
    if not return_peaks:
        return wav, lens, rates
    if want:
        for b, (_, mx) in host_rows.items():
            peaks[b] = mx
    return wav, lens, rates, peaks


def write_wav_pcm16(path: str, codes: np.ndarray, sample_rate: int) -> None:
    """The 16-bit file ``write_wav`` writes, from ready-made codes (int16 ``[frames]`` or ``[frames, channels]``, ``use_wav_write_pcm16``)."""
    a = np.ascontiguousarray(codes)
    if a.dtype != np.int16:
        raise TypeError(f"codes must be int16, got {a.dtype}")
    frames, ch = (a.shape[0], 1) if a.ndim == 1 else a.shape
    check(lib().use_wav_write_pcm16(os.fsencode(path), a.ctypes.data_as(C.c_void_p), frames, ch, int(sample_rate)), "use_wav_write_pcm16")


def _store_args(wav, lens, nums, subtype):
    if subtype not in (PCM16, FLOAT32):
        raise ValueError(f"unknown subtype {subtype!r} (wavio.PCM16 or wavio.FLOAT32)")
    if wav.dim() != 2:
        raise ValueError(f"wav must be [B, L], got shape {tuple(wav.shape)}")
    B, L = wav.shape
    lens = np.asarray(lens.cpu() if hasattr(lens, "cpu") else lens, dtype=np.int64).reshape(-1)
    nums = np.asarray(nums.cpu() if hasattr(nums, "cpu") else nums, dtype=np.int64).reshape(-1)
    if lens.shape[0] != B or nums.shape[0] != B:
        raise ValueError(f"lens has {lens.shape[0]} and nums {nums.shape[0]} entries for a batch of {B}")
    if (lens < 1).any() or (lens > L).any() or (nums < 1).any():
        raise ValueError(f"lens={lens.tolist()} must lie in 1 ... {L} (the width of the batch) and nums={nums.tolist()} must be positive")
    return lens, nums


def _gain_args(gains, count: int):
    """``gains`` of a store call -> float64 ``[count]`` (or ``None``): finite and not negative, as the library demands."""
    if gains is None:
        return None
    g = np.asarray(gains.cpu() if hasattr(gains, "cpu") else gains, dtype=np.float64).reshape(-1)
    if g.shape[0] != count:
        raise ValueError(f"gains has {g.shape[0]} entries for {count} items")
    if not (np.isfinite(g) & (g >= 0)).all():
        raise ValueError(f"gains={g.tolist()} must be finite and not negative")
    return np.ascontiguousarray(g)


def _quantise(x32: np.ndarray) -> np.ndarray:
    """The 16-bit codes ``use_wav_write`` stores for float32 samples: ``nearbyint(float64(x) * 32767)``, NaN -> 0, clamped."""
    v = np.rint(x32.astype(np.float64) * 32767.0)
    v[np.isnan(v)] = 0.0
    return np.clip(v, -32768.0, 32767.0).astype(np.int16)


def store_items_host(wav, lens, nums, subtype: int = PCM16, gains=None) -> np.ndarray:
    """``store_batch_device`` on the host, for CPU tensors and for items beyond the device's 2^24 samples: item b's first ``lens[b]``
    float32 samples -> float64 -> ``resample_fft`` to ``nums[b]`` samples (``nums[b] == lens[b]``: as they are) -> float32 -> the
    16-bit code ``write_wav`` stores (``PCM16``) or the float32 itself (``FLOAT32``).  -> host ``[B, max(nums)]``, zero past ``nums[b]``.

    ``gains`` (float64, one per item; ``data.restore_level``): the float64 value - resampled, or the widened sample at ``num == len`` -
    times ``gains[b]``, one float64 product, before the rounding to float32.  ``None``: no product at all."""
    import torch
    wav = torch.as_tensor(wav)
    lens, nums = _store_args(wav, lens, nums, subtype)
    gains = _gain_args(gains, wav.shape[0])
    out = np.zeros((wav.shape[0], int(nums.max())), np.int16 if subtype == PCM16 else np.float32)
    for b, (n, num) in enumerate(zip(lens.tolist(), nums.tolist())):
        x32 = wav[b, :n].detach().cpu().numpy().astype(np.float32)
        if gains is not None:
            v = x32.astype(np.float64) if num == n else resample_fft(x32.astype(np.float64), num)
            with np.errstate(over="ignore", invalid="ignore"):
                x32 = (v * gains[b]).astype(np.float32)
        elif num != n:
            x32 = resample_fft(x32.astype(np.float64), num).astype(np.float32)
        out[b, :num] = _quantise(x32) if subtype == PCM16 else x32
    return out


def _file_args(wav, lens, nums, channels, subtype):
    """Per-FILE ``lens`` / ``nums`` / ``channels`` of a batch whose rows are the channels of its files -> (lens, nums, channels, first
    rows) as int64 arrays."""
    chans = np.asarray(channels, dtype=np.int64).reshape(-1)
    if chans.shape[0] < 1 or (chans < 1).any() or int(chans.sum()) != wav.shape[0]:
        raise ValueError(f"channels={chans.tolist()} must be positive and add up to the {wav.shape[0]} rows of the batch")
    row0 = np.concatenate([[0], np.cumsum(chans)]).astype(np.int64)
    lens, nums = _store_args(wav[: chans.shape[0]], lens, nums, subtype)   # one entry per file; a view of F rows carries the width
    return lens, nums, chans, row0


def store_files_host(wav, lens, nums, channels, subtype: int = PCM16, gains=None):
    """``store_batch_device(channels=...)`` on the host: file f's rows through ``store_items_host``, interleaved.  -> a list of host
    arrays ``[nums[f], channels[f]]``.  ``gains``: one per FILE, for all its channels."""
    import torch
    wav = torch.as_tensor(wav)
    lens, nums, chans, row0 = _file_args(wav, lens, nums, channels, subtype)
    gains = _gain_args(gains, chans.shape[0])
    out = []
    for f, c in enumerate(chans.tolist()):
        rows = store_items_host(wav[row0[f]: row0[f] + c], [lens[f]] * c, [nums[f]] * c, subtype,
                                None if gains is None else [gains[f]] * c)
        out.append(np.ascontiguousarray(rows[:, : nums[f]].T))
    return out


def _store_files_device(wav, lens, nums, channels, subtype, max_samples, gains=None):
    import torch
    lens, nums, chans, row0 = _file_args(wav, lens, nums, channels, subtype)
    gains = _gain_args(gains, chans.shape[0])
    if wav.stride(1) != 1 or wav.stride(0) < wav.shape[1]:
        wav = wav.contiguous()
    F, stride = len(chans), wav.stride(0)
    limit = min(int(max_samples), 2 ** 24)
    host = [f for f in range(F) if max(lens[f], nums[f]) > limit or chans[f] > 64]
    offs = np.concatenate([[0], np.cumsum(nums * chans)]).astype(np.int64)     # the files lie one after another, no gap
    dev = wav.device
    with torch.cuda.device(dev):
        out = torch.empty(max(int(offs[-1]), 1), dtype=torch.int16 if subtype == PCM16 else torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        f = 0
        while f < F:                                        # one call per run of files that the device forms: one call without host files
            if f in host:
                f += 1
                continue
            e = f
            while e < F and e not in host:
                e += 1
            k = e - f
            work = _workspace(dev, max(lib().use_store_workspace(int(lens[i]), int(nums[i])) for i in range(f, e)))
            head = (wav[int(row0[f])].data_ptr(), stride, (C.c_int * k)(*lens[f:e].tolist()), (C.c_int64 * k)(*nums[f:e].tolist()),
                    (C.c_int * k)(*chans[f:e].tolist()), (C.c_int64 * k)(*offs[f:e].tolist()))
            tail = (k, subtype, out.data_ptr(), work.data_ptr(), work.numel(), stream)
            if gains is None:
                check(lib().use_store_files_dev(*head, *tail), "use_store_files_dev")
            else:
                check(lib().use_store_files_dev_gain(*head, (C.c_double * k)(*gains[f:e].tolist()), *tail), "use_store_files_dev_gain")
            f = e
        flat = out.cpu().numpy()
    res = [flat[offs[f]: offs[f + 1]].reshape(int(nums[f]), int(chans[f])) for f in range(F)]
    for f in host:
        res[f] = store_files_host(wav[row0[f]: row0[f + 1]], lens[f: f + 1], nums[f: f + 1], chans[f: f + 1], subtype,
                                  None if gains is None else gains[f: f + 1])[0]
    return res


def store_batch_device(wav, lens, nums, subtype: int = PCM16, max_samples: int = 2 ** 24, channels=None, gains=None):
    """The way out of a batch on the device (``use_store_items_dev``): ``wav`` float32 CUDA ``[B, L]``, item b valid for ``lens[b]``
    samples (the rest of a row is never read) and resampled to ``nums[b]`` samples in fp64, then rounded to float32 and stored as it is
    (``FLOAT32``) or as the 16-bit code ``write_wav`` stores (``PCM16``).  -> host array ``[B, max(nums)]`` (float32 / int16), zero past
    ``nums[b]``: one call, one device-to-host copy, one synchronisation.  An item with more than ``max_samples`` samples before or after
    resampling goes through ``store_items_host`` instead.

    ``channels`` (one count per FILE; ``lens`` and ``nums`` then per file too): the rows are the channels of files, file after file
    (``data.channels=all``); every row goes the same way and the files come back interleaved (``use_store_files_dev``), as
    ``write_wav`` / ``write_wav_pcm16`` store them.  -> a list of host arrays ``[nums[f], channels[f]]``, views of the one copy.

    ``gains`` (float64 on the host, one per item, or per FILE with ``channels``; ``data.restore_level``): every output sample is
    ``(float)(v * g)``, ``v`` the fp64 value before the rounding to float32 (``use_store_items_dev_gain`` /
    ``use_store_files_dev_gain``; ``store_items_host`` for the items that go there).  ``None``: the calls without a gain."""
    import torch
    if not isinstance(wav, torch.Tensor) or not wav.is_cuda:
        raise UseHipError("wav must be a CUDA (ROCm) tensor: use store_items_host for a CPU tensor")
    if wav.dtype != torch.float32:
        raise TypeError(f"wav must be float32, got {wav.dtype}")
    if channels is not None:
        return _store_files_device(wav, lens, nums, channels, subtype, max_samples, gains)
    lens, nums = _store_args(wav, lens, nums, subtype)
    gains = _gain_args(gains, wav.shape[0])
    if wav.stride(1) != 1 or wav.stride(0) < wav.shape[1]:
        wav = wav.contiguous()
    B, stride, out_stride = wav.shape[0], wav.stride(0), int(nums.max())
    limit = min(int(max_samples), 2 ** 24)
    host = [b for b in range(B) if max(lens[b], nums[b]) > limit]
    dev = wav.device
    with torch.cuda.device(dev):
        out = torch.empty(B, out_stride, dtype=torch.int16 if subtype == PCM16 else torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        b = 0
        while b < B:                                        # one call per run of rows that the device forms: one call without host rows
            if b in host:
                b += 1
                continue
            e = b
            while e < B and e not in host:
                e += 1
            k = e - b
            nbytes = max(lib().use_store_workspace(int(lens[i]), int(nums[i])) for i in range(b, e))
            work = _workspace(dev, nbytes)
            head = (wav[b].data_ptr(), stride, (C.c_int * k)(*lens[b:e].tolist()), (C.c_int64 * k)(*nums[b:e].tolist()))
            tail = (k, subtype, out[b].data_ptr(), out_stride, work.data_ptr(), work.numel(), stream)
            if gains is None:
                check(lib().use_store_items_dev(*head, *tail), "use_store_items_dev")
            else:
                check(lib().use_store_items_dev_gain(*head, (C.c_double * k)(*gains[b:e].tolist()), *tail), "use_store_items_dev_gain")
            b = e
        res = out.cpu().numpy()
    for b in host:
        res[b] = 0
        res[b, : nums[b]] = store_items_host(wav[b: b + 1], lens[b: b + 1], nums[b: b + 1], subtype,
                                             None if gains is None else gains[b: b + 1])[0]
    return res
