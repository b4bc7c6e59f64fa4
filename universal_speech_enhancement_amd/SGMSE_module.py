"""``SGMSEModule`` with the constructor and step contract of the reference's ``src/models/SGMSE_module.py:10-82``:
``predict_step(batch, batch_idx)`` runs ``Score.sample(batch)``, trims every item to ``sample_length`` and writes it to
``audio_path.replace(data_folder, target_folder)``; ``training_step`` / ``validation_step`` / ``test_step`` /
``configure_optimizers`` as there.  The base class is ``lightning.LightningModule`` where Lightning is installed (the reference's
``Trainer.fit`` / ``Trainer.predict`` then drive it unchanged, with the ``self.log`` calls of the reference) and a plain ``nn.Module``
where it is not (the target image) - the methods are the same either way.
"""
from __future__ import annotations

import os

import numpy as np
import torch


def _write_wav(path: str, wav: np.ndarray, sr: int, subtype: str = "PCM_16"):
    """``sf.write(path, wav, sr)`` of the reference (SGMSE_module.py:80): soundfile's default WAV subtype is 16-bit PCM;
    ``subtype="FLOAT"`` keeps the float32 samples.  Native writer (csrc/use_io.cpp: use_wav_write)."""
    from .wavio import FLOAT32, PCM16, write_wav
    if subtype not in ("PCM_16", "FLOAT"):
        raise ValueError(f"unsupported WAV subtype {subtype!r} (PCM_16 or FLOAT)")
    write_wav(path, wav, int(sr), PCM16 if subtype == "PCM_16" else FLOAT32)


def _with_path_seeds(sampler_kwargs: dict, batch: dict) -> dict:
    """The keywords of ``Score.sample`` for one batch of ``predict_step``: under ``per_item`` (and without ``item_seeds`` of the
    caller's) every file gets the seed named by its path."""
    kw = dict(sampler_kwargs)
    if kw.get("per_item") and kw.get("item_seeds") is None and "audio_path" in batch:
        # batch-invariant sampling: a file's noise is named by its path relative to data_folder, so that its output does not depend
        # on the batch order, on batch_size or on how the files are sharded over the ranks - at equal padded length T', or for any
        # mix of lengths with own_length (every file at its own T')
        from .seeding import item_seed, path_key
        kw["item_seeds"] = [item_seed(int(kw.get("seed", 0)), path_key(os.path.relpath(p, batch["data_folder"]).replace(os.sep, "/")))
                            for p in batch["audio_path"]]
    return kw


def _write_items(batch: dict, wavs, folder, subtype: str, restore: bool = True, gains=None):
    """Item i of ``wavs``, trimmed to ``sample_length[i]``, to ``audio_path[i].replace(data_folder, folder)`` (reference
    SGMSE_module.py:72-80); a batch without ``audio_path`` writes nothing.

    A batch that carries ``source_rate`` and ``source_length`` (``LoadWavData(restore_rate=True)``) is written at its sources' own
    rates instead, unless ``restore`` is off: item i, resampled from its ``sample_length[i]`` samples to exactly ``source_length[i]``
    frames, at ``source_rate[i]`` - the whole batch in one device call and one copy (``wavio.store_batch_device``; a CPU batch through
    ``wavio.store_items_host``).  A file whose rate is the model's has the bytes it has without the keys.

    A batch that carries ``source_gain`` (``LoadWavData(restore_level=True)``) is written at its sources' level, unless ``restore`` is
    off: through the same store functions with ``gains`` = ``source_gain``, or the caller's ``gains`` (one per row) in its place - at
    the source's rate and frame count where the batch has them, else at ``sampling_rate`` / ``sample_length``."""
    if "audio_path" not in batch:
        return
    gains = (batch["source_gain"] if gains is None else gains) if restore and "source_gain" in batch else None
    restored = bool(restore and "source_rate" in batch and "source_length" in batch)
    if "file_rows" in batch:
        return _write_files(batch, wavs, folder, subtype, restored, gains)
    if restored or gains is not None:
        return _write_items_restored(batch, wavs, folder, subtype, restored, gains)
    for i, wav in enumerate(wavs):
        noisy_path = batch["audio_path"][i]
        sample_length = int(batch["sample_length"][i])
        sample_rate = batch["sampling_rate"][i]
        path = noisy_path.replace(batch["data_folder"], folder)
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        _write_wav(path, wav.detach().cpu().numpy().astype(np.float32)[:sample_length], sample_rate, subtype)


def _write_items_restored(batch: dict, wavs, folder, subtype: str, restored: bool = True, gains=None):
    """The batch through the store functions: at ``source_rate`` / ``source_length`` (``restored``) or at the model's rate and
    ``sample_length`` (only ``gains`` to apply), with ``gains`` (float64, one per row) or without."""
    from . import wavio
    if subtype not in ("PCM_16", "FLOAT"):
        raise ValueError(f"unsupported WAV subtype {subtype!r} (PCM_16 or FLOAT)")
    code = wavio.PCM16 if subtype == "PCM_16" else wavio.FLOAT32
    wavs = torch.as_tensor(wavs).detach().float()
    lens = [int(n) for n in batch["sample_length"]]
    nums = [int(n) for n in batch["source_length"]] if restored else lens
    rates = batch["source_rate"] if restored else batch["sampling_rate"]
    kw = {} if gains is None else {"gains": gains}
    rows = (wavio.store_batch_device if wavs.is_cuda else wavio.store_items_host)(wavs, lens, nums, code, **kw)
    for i, num in enumerate(nums):
        path = batch["audio_path"][i].replace(batch["data_folder"], folder)
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        if code == wavio.PCM16:
            wavio.write_wav_pcm16(path, rows[i, :num], int(rates[i]))
        else:
            wavio.write_wav(path, rows[i, :num], int(rates[i]), wavio.FLOAT32)


def _write_files(batch: dict, wavs, folder, subtype: str, restored: bool, gains=None):
    """A batch of ``LoadWavData(channels="all")``: the rows ``file_rows[f] = (first row, C)`` are the channels of one file and go back
    into one C-channel file, ``[frames, C]`` interleaved.  ``restored``: at the source's rate and frame count, the whole batch in one
    device call and one copy (``wavio.store_batch_device(channels=...)``; a CPU batch through ``wavio.store_files_host``); otherwise the
    rows trimmed to ``sample_length`` and stacked, through the writer ``_write_items`` uses.  A mono file has the bytes it has without
    the key.  ``gains`` (one per ROW, equal over the rows of a file): the store functions' way too, with the file's gain, at the
    source's rate (``restored``) or at ``sampling_rate`` / ``sample_length``."""
    from . import wavio
    if subtype not in ("PCM_16", "FLOAT"):
        raise ValueError(f"unsupported WAV subtype {subtype!r} (PCM_16 or FLOAT)")
    code = wavio.PCM16 if subtype == "PCM_16" else wavio.FLOAT32
    wavs = torch.as_tensor(wavs).detach()
    first = [r for r, _ in batch["file_rows"]]
    chans = [c for _, c in batch["file_rows"]]
    lens = [int(batch["sample_length"][r]) for r in first]
    stored = restored or gains is not None
    if stored:
        nums = [int(batch["source_length"][r]) for r in first] if restored else lens
        rates = batch["source_rate"] if restored else batch["sampling_rate"]
        kw = {} if gains is None else {"gains": [float(gains[r]) for r in first]}
        wavs = wavs.float()
        files = (wavio.store_batch_device(wavs, lens, nums, code, channels=chans, **kw) if wavs.is_cuda
                 else wavio.store_files_host(wavs, lens, nums, chans, code, **kw))
    else:
        host = wavs.cpu().numpy().astype(np.float32)
    for f, (r, c) in enumerate(batch["file_rows"]):
        path = batch["audio_path"][r].replace(batch["data_folder"], folder)
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        if stored:
            a = files[f] if c > 1 else files[f][:, 0]
            if code == wavio.PCM16:
                wavio.write_wav_pcm16(path, a, int(rates[r]))
            else:
                wavio.write_wav(path, a, int(rates[r]), wavio.FLOAT32)
        else:
            a = host[r, : lens[f]] if c == 1 else np.ascontiguousarray(host[r: r + c, : lens[f]].T)
            _write_wav(path, a, batch["sampling_rate"][r], subtype)


try:                                                     # reference: class SGMSEModule(LightningModule), SGMSE_module.py:10
    from lightning import LightningModule as _Base
    HAS_LIGHTNING = True
except Exception:                                        # not installed on the target image
    _Base, HAS_LIGHTNING = torch.nn.Module, False


class SGMSEModule(_Base):
    def __init__(self, Score: torch.nn.Module, optimizer=None, scheduler=None, compile: bool = False, sampler_kwargs=None,
                 wav_subtype: str = "PCM_16"):
        super().__init__()
        self.Score = Score
        self.wav_subtype = wav_subtype                       # "PCM_16" = what the reference's sf.write produces; "FLOAT" = float32
        self.optimizer, self.scheduler, self.compile = optimizer, scheduler, compile
        self.sampler_kwargs = dict(sampler_kwargs or {})     # optional N / corrector_steps / snr overrides, sampler_type="ode" (+ rtol / atol / minibatch), chunk_frames (+ chunk_overlap / chunk_batch), per_item (+ seed), own_length

    def load_lightning_checkpoint(self, path: str, map_location="cpu"):
        """Loads ``ckpt['state_dict']`` with the reference's key layout (``Score.score_net.all_modules...``)."""
        ckpt = torch.load(path, map_location=map_location, weights_only=False)
        sd = ckpt.get("state_dict", ckpt)
        missing, unexpected = self.load_state_dict(sd, strict=False)
        if missing:
            raise KeyError(f"checkpoint is missing {len(missing)} tensors, e.g. {missing[:3]}")
        return unexpected

    @torch.no_grad()
    def predict_step(self, batch: dict, batch_idx: int = 0) -> dict:
        batch = self.Score.sample(batch, **_with_path_seeds(self.sampler_kwargs, batch))
        _write_items(batch, batch["enhanced"], batch.get("target_folder"), self.wav_subtype)
        return batch

    def get_score_loss(self, batch: dict) -> torch.Tensor:
        """Reference :42-44."""
        return self.Score.train_step(batch)

    def _log(self, name, value, **kw):
        """``self.log`` of the reference's steps when a Lightning trainer is attached; nothing otherwise."""
        if HAS_LIGHTNING and getattr(self, "_trainer", None) is not None:
            self.log(name, value, **kw)

    @torch.no_grad()
    def validation_step(self, batch: dict, batch_idx: int = 0) -> torch.Tensor:
        """Reference :56-58 (logs ``val/loss_Score``; the value is also returned)."""
        loss = self.get_score_loss(batch)
        self._log("val/loss_Score", loss, on_step=True, on_epoch=True, prog_bar=True)
        return loss

    @torch.no_grad()
    def test_step(self, batch: dict, batch_idx: int = 0) -> torch.Tensor:
        """Reference :61-63."""
        loss = self.get_score_loss(batch)
        self._log("test/loss_Score", loss, on_step=True, on_epoch=True, prog_bar=True)
        return loss

    def training_step(self, batch: dict, batch_idx: int = 0) -> torch.Tensor:
        """Reference :46-54 (there the value is also logged): the score-matching loss WITH its tape, for ``loss.backward()`` and an
        optimiser step.  The score network's parameters are created frozen (the sampling path never differentiates); training needs
        ``module.Score.score_net.requires_grad_(True)`` first, on the GPU."""
        if not getattr(self.Score.score_net, "trainable", False):
            raise RuntimeError("training_step: the score network's parameters are frozen - call Score.score_net.requires_grad_(True) "
                               "(validation_step / test_step give the loss without a tape)")
        with torch.enable_grad():
            loss = self.get_score_loss(batch)
        self._log("train/loss_Score", loss, on_step=True, on_epoch=True, prog_bar=True)
        if HAS_LIGHTNING and getattr(self, "_trainer", None) is not None:       # reference :51-53: the learning rate, per epoch
            self._log("lr", self.optimizers().param_groups[0]["lr"], on_step=False, on_epoch=True, prog_bar=True)
        return loss

    def configure_optimizers(self):
        """Reference :26-40: ``optimizer(params=Score.parameters())`` and ``scheduler(optimizer=...)`` from the constructor's partials,
        in Lightning's dictionary layout (the monitor key is the reference's)."""
        if self.optimizer is None:
            raise RuntimeError("configure_optimizers: SGMSEModule was built without an optimizer factory")
        opt = self.optimizer(params=self.Score.parameters())
        if self.scheduler is None:
            return [{"optimizer": opt}]
        return [{"optimizer": opt,
                 "lr_scheduler": {"scheduler": self.scheduler(optimizer=opt), "monitor": "val/loss_Score_epoch", "interval": "epoch",
                                  "frequency": 1}}]
