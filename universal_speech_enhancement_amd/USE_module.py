"""``USEModule``: the reference's documented pipeline - the SGMSE sampler (``SGMSEModule``), then the LSGAN refine generator
(``GANModule``) over the files the sampler wrote - as ONE ``predict_step``, with the audio on the device from the noisy batch to the
refined file.  What lies between the two runs of the two-run flow (16-bit file, decode, peak normalisation, zero padding) is
``handoff.wav_handoff`` on the device, so that the refined files are, byte for byte, those of

    predict model=SGMSE_Large ckpt_path=score.ckpt data.data_folder=noisy/    data.target_folder=enhanced/
    predict model=LSGAN       ckpt_path=lsgan.ckpt data.data_folder=enhanced/ data.target_folder=refined/

at equal options and batch composition.  Both networks stay resident; there is one process start, one pass of the loader and no
intermediate file (unless ``stage1_folder`` asks for it).  The base class is ``SGMSEModule``'s.
"""
from __future__ import annotations

import inspect

import torch

from .SGMSE_module import _Base, _with_path_seeds, _write_items

_SUBTYPES = ("PCM_16", "FLOAT")


def shared_refine_kwargs(sampler_kwargs: dict) -> dict:
    """The keys of ``sampler_kwargs`` that ``NCSNPP_Wrapper.forward`` accepts too (``chunk_frames``, ``chunk_overlap``,
    ``chunk_batch``, ``own_length``): what a user of the two-run flow passes to both runs."""
    from .gan.ncsnpp_wrapper import NCSNPP_Wrapper
    accepted = [k for k in inspect.signature(NCSNPP_Wrapper.forward).parameters if k not in ("self", "batch_data")]
    return {k: sampler_kwargs[k] for k in accepted if k in sampler_kwargs}


class USEModule(_Base):
    def __init__(self, Score: torch.nn.Module, G: torch.nn.Module, sampler_kwargs=None, refine_kwargs=None,
                 handoff_subtype: str = "PCM_16", normalize: bool = True, wav_subtype: str = "PCM_16", stage1_folder=None,
                 compile: bool = False):
        super().__init__()
        for name, v in (("handoff_subtype", handoff_subtype), ("wav_subtype", wav_subtype)):
            if v not in _SUBTYPES:
                raise ValueError(f"{name}={v!r}: unsupported WAV subtype (PCM_16 or FLOAT)")
        self.Score, self.G = Score, G
        self.sampler_kwargs = dict(sampler_kwargs or {})     # the keywords of Score.sample, as SGMSEModule(sampler_kwargs=...)
        # the keywords of the generator's forward pass, as GANModule(sampler_kwargs=...); None: the shared keys of sampler_kwargs
        self.refine_kwargs = shared_refine_kwargs(self.sampler_kwargs) if refine_kwargs is None else dict(refine_kwargs)
        self.handoff_subtype = handoff_subtype               # the subtype of the stage-1 files of the two-run flow; "FLOAT": no quantisation
        self.normalize = bool(normalize)                     # data.normalize of the second run
        self.wav_subtype = wav_subtype                       # the subtype of the refined files
        self.stage1_folder = stage1_folder                   # set: the stage-1 files are written there too, as SGMSEModule writes them
        self.compile = compile

    def load_lightning_checkpoint(self, path: str, stage: str, map_location="cpu"):
        """``stage="score"``: the ``Score.*`` tensors of ``ckpt['state_dict']``; ``stage="refine"``: the ``G.*`` tensors (the reference's
        key layouts ``Score.score_net.all_modules...`` / ``G.net.all_modules...``)."""
        prefixes = {"score": "Score.", "refine": "G."}
        if stage not in prefixes:
            raise ValueError(f"stage={stage!r} must be 'score' or 'refine'")
        ckpt = torch.load(path, map_location=map_location, weights_only=False)
        sd = {k: v for k, v in ckpt.get("state_dict", ckpt).items() if k.startswith(prefixes[stage])}
        missing, unexpected = self.load_state_dict(sd, strict=False)
        missing = [k for k in missing if k.startswith(prefixes[stage])]
        if missing:
            raise KeyError(f"checkpoint is missing {len(missing)} {stage} tensors, e.g. {missing[:3]}")
        return unexpected

    @torch.no_grad()
    def predict_step(self, batch: dict, batch_idx: int = 0) -> dict:
        """Adds ``enhanced`` (the sampler's output, untouched), ``fake`` (the refined batch) and ``handoff_peak`` (float64 [B]: every
        item's peak as the second run's loader would find it) and writes item i of ``fake`` to
        ``audio_path[i].replace(data_folder, target_folder)``.  A batch with ``source_gain`` (``data.restore_level``): the refined files
        get ``source_gain * (handoff_peak / 0.8)`` - both normalisations undone, in float64 on the host - or ``source_gain`` alone when
        the hand-off does not normalise; the stage-1 files stay at the model's level."""
        from .handoff import wav_handoff, wav_handoff_files
        batch = self.Score.sample(batch, **_with_path_seeds(self.sampler_kwargs, batch))
        enhanced = batch["enhanced"]
        lengths = batch.get("sample_length")
        if self.stage1_folder:
            # at the model's rate whatever data.restore_rate says: these are the files the second run's loader reads
            _write_items(batch, enhanced, self.stage1_folder, self.handoff_subtype, restore=False)
        if "file_rows" in batch:
            # data.channels=all: the stage-1 files hold several channels and the second run's loader gives each ONE gain
            # (handoff_peak then has one entry per file)
            file_lengths = None if lengths is None else [int(lengths[r]) for r, _ in batch["file_rows"]]
            wav, peaks = wav_handoff_files(enhanced, file_lengths, [c for _, c in batch["file_rows"]], self.handoff_subtype, self.normalize)
        else:
            wav, peaks = wav_handoff(enhanced, lengths, self.handoff_subtype, self.normalize)
        stage2 = {"perturbed": wav}
        if lengths is not None:
            stage2["sample_length"] = lengths
        batch["fake"] = self.G(stage2, **self.refine_kwargs)["fake"]
        batch["handoff_peak"] = peaks
        gains = None
        if "source_gain" in batch and self.normalize:
            import numpy as np
            g2 = peaks.detach().cpu().numpy().astype(np.float64) / np.float64(0.8)
            if "file_rows" in batch:
                g2 = np.repeat(g2, [c for _, c in batch["file_rows"]])
            gains = np.asarray(batch["source_gain"], dtype=np.float64) * g2
        _write_items(batch, batch["fake"], batch.get("target_folder"), self.wav_subtype, gains=gains)
        return batch

    def training_step(self, *a, **k):
        raise NotImplementedError("USEModule serves inference; train the score model with SGMSEModule")
