"""Inference input side: walks a folder for .wav files and yields the batch dict the reference's
``pad_to_longest_monaural_inference`` produces (``src/data/components/collate.py:42-73``): first channel, resampled to
``sampling_rate`` (FFT method), peak-normalised to 0.8 (``src/data/components/loadwav_dataset.py:90-120``), zero-padded to
the longest item.  Multi-process runs shard the file list over ranks like the reference's per-rank batches
(``src/data/loadwav_datamodule.py:53-60``).

``bucket_by_length`` (no reference counterpart, off by default): the rank's shard - the same file set as without it - is ordered by
(padded frame count T', relative path) and cut into batches of files of EQUAL T', so that ``sample(own_length=True)`` runs full
batches of one plan shape; T' comes from the WAV headers (``wav_info`` + ``resampled_length``), no file is decoded for it.

``device_load`` (no reference counterpart, off by default): the host only decodes the files; resampling, peak normalisation, the cast
and the zero-padded collation run on the device (``wavio.load_batch_device``).  The batch dict is the same; a resampled row is the host
loader's to within the last float32 bit, a row at an unchanged rate is bit-equal.  A file of more than ``device_load_max_samples``
samples (before or after resampling) takes the host path.

``restore_rate`` (no reference counterpart, off by default): every batch also carries ``source_rate`` and ``source_length``, the
rate and frame count of each file as ``wav_info`` reports them, and the writers of the models (``SGMSE_module._write_items``) then
write every output at its source's rate with exactly its frame count.  Off: the batch dict is what it always was.

``restore_level`` (no reference counterpart, off by default): every batch also carries ``source_gain``, a float64 host tensor with one
entry per row: ``mx / 0.8``, ``mx`` the peak the loader divided the file by (exactly 1 with ``normalize=false``, 0 for a silent file;
the same for all channels of a file under ``channels=all``).  The writers multiply every output sample by it, in fp64 before their
rounding to float32, so that a file comes out at its source's level; the tensors of the batch are not touched.  Off: the batch dict
and the loader calls are what they always were.

``channels`` (no reference counterpart; ``first`` by default: the reference's loader, which keeps the first channel of a file and drops the
rest).  ``all``: a file of C channels gives C consecutive rows of the batch, in channel order, and the writers put them back together as
one C-channel file.  The rules:
  whole files   a batch holds whole files only: files are taken in the usual order while the row count stays <= ``batch_size``; a file of
                more channels than that is a batch of its own.  ``bucket_by_length`` orders the files as before (T' comes from the header
                and is the same for every channel of a file); sharding over ranks stays per file.
  one gain      the peak normalisation is one gain per file, taken over all channels after resampling (``wavio.load_file_channels``), so
                that the channels keep their level relation; a mono file gets the bits it gets with ``first``.
  one seed      ``audio_path``, ``name``, ``sample_length`` and ``sampling_rate`` repeat for the rows of a file, so the ``per_item``
                seeds, which are named by the path, are shared by its channels: equal channels come out equal.  Without ``per_item`` the
                shared noise stream gives every row different noise.
The batch gains ``channel`` and ``n_channels`` (per row) and ``file_rows`` (per file: ``(first row, C)``)."""
from __future__ import annotations

import os
from typing import Dict, Iterator, List

import numpy as np
import torch

from .distributed import shard_list
from .wavio import check_channels, load_batch_device, load_file_channels, load_utterance, resampled_length, source_gain, wav_info


def _gains(peaks, counts) -> torch.Tensor:
    """``source_gain`` of a batch: from the peak of every file (``peaks`` ``None``: not normalised, gain 1), repeated over the
    ``counts[f]`` rows of file f."""
    g = np.array([source_gain(None if peaks is None else peaks[f]) for f in range(len(counts))], dtype=np.float64)
    return torch.from_numpy(np.repeat(g, counts))


class LoadWavData:
    def __init__(self, data_folder: str, target_folder: str, normalize: bool = True, sampling_rate: int = 24000,
                 batch_size: int = 1, num_workers: int = 0, rank: int = 0, world_size: int = 1, bucket_by_length: bool = False,
                 device_load: bool = False, device_load_max_samples: int = 2 ** 24, restore_rate: bool = False, channels: str = "first",
                 restore_level: bool = False, **ignored):
        self.data_folder, self.target_folder = data_folder, target_folder
        self.normalize, self.sampling_rate, self.batch_size = normalize, sampling_rate, batch_size
        self.bucket_by_length = bool(bucket_by_length)
        self.device_load, self.device_load_max_samples = bool(device_load), int(device_load_max_samples)
        self.restore_rate, self.restore_level = bool(restore_rate), bool(restore_level)
        self.channels = check_channels(channels)
        files: List[str] = []
        for root, _, names in os.walk(data_folder):
            files += [os.path.join(root, n) for n in sorted(names) if n.endswith(".wav")]
        self.filepaths = shard_list(sorted(files), rank, world_size)

    def __len__(self):
        return len(self.filepaths)

    def _item(self, path: str) -> Dict:
        if self.restore_level:
            x, sr, mx = load_utterance(path, self.sampling_rate, self.normalize, return_peak=True)
            return {"perturbed": x, "name": os.path.basename(path).split(".wav")[0], "audio_path": path, "sampling_rate": sr, "peak": mx}
        x, sr = load_utterance(path, self.sampling_rate, self.normalize)       # native loader (csrc/use_io.cpp)
        return {"perturbed": x, "name": os.path.basename(path).split(".wav")[0], "audio_path": path, "sampling_rate": sr}

    def padded_frames(self, path: str, frame_hop: int) -> int:
        """T' = pad64(1 + L // frame_hop) of a file, L from its header: the length ``load_utterance`` will give it."""
        frames, _, sr = wav_info(path)
        L = resampled_length(frames, sr, self.sampling_rate)
        return (1 + L // int(frame_hop) + 63) // 64 * 64

    def batch_files(self, frame_hop=None) -> List[List[str]]:
        """The file lists of the batches ``predict_batches`` yields, in its order.  Default: consecutive ``batch_size`` files of the
        shard.  ``bucket_by_length``: the shard ordered by (T', path relative to ``data_folder``), cut where T' changes or a batch is
        full - a batch never mixes two values of T'; the same on every call.  ``channels="all"``: a file counts as many rows as it has
        channels (from its header) and a batch is full at ``batch_size`` rows; a file of more channels than that is a batch of its own."""
        if not self.bucket_by_length and self.channels == "first":
            return [self.filepaths[i:i + self.batch_size] for i in range(0, len(self.filepaths), self.batch_size)]
        if self.bucket_by_length and frame_hop is None:
            raise ValueError("bucket_by_length needs frame_hop (the model's hop_length): predict_batches(device, frame_hop=...)")
        if self.bucket_by_length:
            keyed = sorted((self.padded_frames(p, frame_hop), os.path.relpath(p, self.data_folder).replace(os.sep, "/"), p)
                           for p in self.filepaths)
        else:
            keyed = [(None, None, p) for p in self.filepaths]
        batches: List[List[str]] = []
        last, rows = None, 0
        for Tp, _, p in keyed:
            c = wav_info(p)[1] if self.channels == "all" else 1
            if not batches or Tp != last or rows + c > self.batch_size:
                batches.append([])
                last, rows = Tp, 0
            batches[-1].append(p)
            rows += c
        return batches

    def predict_batches(self, device="cuda", frame_hop=None) -> Iterator[Dict]:
        if self.device_load:
            if torch.device(device).type != "cuda":
                raise ValueError(f"device_load=True needs a CUDA (ROCm) device, got {device!r}: the device loader has no CPU implementation")
            batches = self._device_batches(device, frame_hop) if self.channels == "first" else self._channel_batches(device, frame_hop)
        else:
            batches = self._host_batches(device, frame_hop) if self.channels == "first" else self._channel_batches(device, frame_hop)
        return self._with_source(batches) if self.restore_rate else batches

    def _channel_batches(self, device, frame_hop) -> Iterator[Dict]:
        """``channels="all"``: the rows of a batch are the channels of its files, file after file."""
        for paths in self.batch_files(frame_hop):
            peaks = None
            if self.device_load and self.restore_level:
                wav, lens, rates, chans, peaks = load_batch_device(paths, self.sampling_rate, self.normalize, device,
                                                                   self.device_load_max_samples, channels="all", return_peaks=True)
            elif self.device_load:
                wav, lens, rates, chans = load_batch_device(paths, self.sampling_rate, self.normalize, device, self.device_load_max_samples,
                                                            channels="all")
            else:
                if self.restore_level:
                    files = [load_file_channels(p, self.sampling_rate, self.normalize, return_peak=True) for p in paths]
                    peaks = [mx for _, _, mx in files] if self.normalize else None
                    files = [(x, sr) for x, sr, _ in files]
                else:
                    files = [load_file_channels(p, self.sampling_rate, self.normalize) for p in paths]
                chans = [x.shape[0] for x, _ in files]
                lens = np.repeat(np.array([x.shape[1] for x, _ in files], dtype=np.int32), chans)
                rates = [sr for (_, sr), c in zip(files, chans) for _ in range(c)]
                wav = torch.zeros(int(sum(chans)), int(lens.max()))
                row = 0
                for x, _ in files:
                    wav[row: row + x.shape[0], : x.shape[1]] = torch.from_numpy(x)
                    row += x.shape[0]
                wav = wav.to(device)
            rows = [p for p, c in zip(paths, chans) for _ in range(c)]
            first = np.concatenate([[0], np.cumsum(chans)])[:-1]
            batch = {"perturbed": wav, "name": [os.path.basename(p).split(".wav")[0] for p in rows],
                     "sample_length": torch.from_numpy(lens), "sampling_rate": rates, "audio_path": rows,
                     "data_folder": self.data_folder, "target_folder": self.target_folder,
                     "channel": [k for c in chans for k in range(c)], "n_channels": [c for c in chans for _ in range(c)],
                     "file_rows": [(int(r), int(c)) for r, c in zip(first, chans)]}
            if self.restore_level:
                batch["source_gain"] = _gains(peaks, list(chans))
            yield batch

    @staticmethod
    def _with_source(batches) -> Iterator[Dict]:
        """``restore_rate``: every file's own rate and frame count, from its header."""
        for batch in batches:
            info = [wav_info(p) for p in batch["audio_path"]]
            batch["source_rate"] = [sr for _, _, sr in info]
            batch["source_length"] = [frames for frames, _, _ in info]
            yield batch

    def _device_batches(self, device, frame_hop) -> Iterator[Dict]:
        for paths in self.batch_files(frame_hop):
            if self.restore_level:
                wav, lens, rates, peaks = load_batch_device(paths, self.sampling_rate, self.normalize, device, self.device_load_max_samples,
                                                            return_peaks=True)
            else:
                wav, lens, rates = load_batch_device(paths, self.sampling_rate, self.normalize, device, self.device_load_max_samples)
            batch = {"perturbed": wav, "name": [os.path.basename(p).split(".wav")[0] for p in paths],
                     "sample_length": torch.from_numpy(lens), "sampling_rate": rates, "audio_path": list(paths),
                     "data_folder": self.data_folder, "target_folder": self.target_folder}
            if self.restore_level:
                batch["source_gain"] = _gains(peaks, [1] * len(paths))
            yield batch

    def _host_batches(self, device, frame_hop) -> Iterator[Dict]:
        for paths in self.batch_files(frame_hop):
            items = [self._item(p) for p in paths]
            lens = np.array([len(it["perturbed"]) for it in items], dtype=np.int32)
            wav = torch.zeros(len(items), int(lens.max()))
            for k, it in enumerate(items):
                wav[k, : lens[k]] = torch.from_numpy(it["perturbed"])
            batch = {"perturbed": wav.to(device), "name": [it["name"] for it in items],
                     "sample_length": torch.from_numpy(lens), "sampling_rate": [it["sampling_rate"] for it in items],
                     "audio_path": [it["audio_path"] for it in items], "data_folder": self.data_folder,
                     "target_folder": self.target_folder}
            if self.restore_level:
                batch["source_gain"] = _gains([it["peak"] for it in items] if self.normalize else None, [1] * len(items))
            yield batch
