"""Predict entry point with the reference's command-line shape (``src/predict.py:39-92``; README.md:176):

    python -m universal_speech_enhancement_amd.predict model=SGMSE_Large ckpt_path=last.ckpt \
        data.data_folder=noisy/ data.target_folder=enhanced/ [model.Score.precision=fp32] [model.sampler_kwargs.N=30]
        [model.sampler_kwargs.sampler_type=ode [model.sampler_kwargs.rtol=1e-5 model.sampler_kwargs.atol=1e-5
         model.sampler_kwargs.minibatch=1]]      (the probability-flow ODE sampler: RK45, one step-size controller per utterance)
        [model.sampler_kwargs.chunk_frames=512 [model.sampler_kwargs.chunk_overlap=64 model.sampler_kwargs.chunk_batch=8]]
                                                 (long recordings in overlapping windows of 512 frames; also with model=LSGAN)
        [model.sampler_kwargs.per_item=true [model.sampler_kwargs.seed=S]]
                                                 (batch-invariant sampling: every file draws from its own noise stream, seeded from S and
                                                  its path relative to data_folder, and takes its own Langevin step - the output does not
                                                  depend on batch order, world size, or data.batch_size at equal padded length; off by default)
        [model.sampler_kwargs.own_length=true [data.bucket_by_length=true]]
                                                 (every file at its own padded frame count T' instead of its batch's longest: with
                                                  per_item a file's output is that of its batch-size-1 run, for any mix of lengths;
                                                  bucket_by_length orders a rank's files by T' so that batches are full at one T')
    python -m universal_speech_enhancement_amd.predict model=USE ckpt_path=score.ckpt refine_ckpt_path=lsgan.ckpt \
        data.data_folder=noisy/ data.target_folder=refined/
                                                 (both stages in one run: the sampler, the hand-off on the device - what the stage-1 file,
                                                  its 16-bit samples and the second run's loader do to the audio - and the refine generator;
                                                  the refined files are byte for byte those of model=SGMSE_Large followed by model=LSGAN.
                                                  model.sampler_kwargs as above, passed on to the generator where it takes them;
                                                  [model.handoff_subtype=FLOAT] hands over unquantised samples; [model.stage1_folder=enhanced/]
                                                  keeps the stage-1 files as well; each checkpoint a Lightning .ckpt or a packed .usehip file)
    Options of every model:
        [data.device_load=true]                  (the loader's FFT resampling, peak normalisation, cast and collation on the device instead
                                                  of file by file on the host, which then only decodes; off by default.  A resampled input
                                                  equals the host loader's to within the last float32 bit, one at an unchanged rate bit for bit)
        [data.restore_rate=true]                 (every output file at its source's own sample rate and frame count instead of 24 kHz: the
                                                  model-rate output is resampled back on the device, a batch per call, so that a file
                                                  can take the place of its noisy one; off by default.  A source at 24 kHz gives the
                                                  same bytes either way; model.stage1_folder files, metrics.csv and losses.csv stay at
                                                  the model's rate; the loader's peak normalisation is not undone unless
                                                  data.restore_level=true asks for it)
        [data.restore_level=true]                (every output file at its source's level instead of peaking near 0.8: the peak the
                                                  loader divided by is carried to the writer, which multiplies every sample by
                                                  peak / 0.8 in fp64 before its rounding to float32 - with model=USE by the hand-off's
                                                  peak / 0.8 as well - so that quiet and loud recordings keep their level relation; off
                                                  by default, alone or with restore_rate, device_load and channels=all.  16-bit output
                                                  clamps as always, wav_subtype=FLOAT keeps values above 1; model.stage1_folder files,
                                                  metrics.csv and losses.csv stay at the model's level; data.normalize=false: gain 1)
        [data.channels=all]                      (every channel of a multi-channel file instead of the first alone: a file of C channels
                                                  is C rows of the batch under ONE gain and comes back as a C-channel file, also with
                                                  restore_rate and model=USE; a batch holds whole files, at most data.batch_size rows.
                                                  Use it with model.sampler_kwargs.per_item=true: the channels of a file then share
                                                  one noise seed and equal channels come out equal, while without it every row draws
                                                  different noise from the shared stream.  metrics.csv / losses.csv get one row per
                                                  file and channel and a channel column; first by default)
        [data.clean_folder=clean/]               (score every enhanced file whose clean counterpart exists under clean/ at the same
                                                  relative path: SI-SDR / SI-SIR / SI-SAR / LSD on the device -> enhanced/metrics.csv)
        [data.clean_folder=clean/ data.intelligibility=true]
                                                 (two more columns of metrics.csv: STOI and ESTOI of the same files on the device, as
                                                  pystoi defines them; a file with fewer than 30 frames gets 1e-5 and a warning)
        [data.clean_folder=clean/ data.convergence_losses=true]
                                                 (the same files against the refine stage's training objective, forward only: waveform
                                                  L1, multi-resolution STFT and log-mel distances on the device -> enhanced/losses.csv)

Hydra and Lightning are not available on the target image, so this is a small stand-in: the same YAML groups
(``configs/predict.yaml`` -> ``data/``, ``model/``), ``key=value`` / ``group=name`` overrides, ``_target_`` instantiation,
and a loop that plays the part of ``trainer.predict`` (one process per GPU under ``torch.distributed.run``)."""
from __future__ import annotations

import importlib
import os
import re
import sys

import torch
import yaml

from . import distributed as D

CONFIG_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")


_FLOAT = re.compile(r"^[+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?$")


def _scalars(node):
    """PyYAML (YAML 1.1) reads ``3e-2`` as a string; OmegaConf reads a float -- follow OmegaConf."""
    if isinstance(node, dict):
        return {k: _scalars(v) for k, v in node.items()}
    if isinstance(node, list):
        return [_scalars(v) for v in node]
    if isinstance(node, str) and _FLOAT.match(node):
        return float(node)
    return node


def _load_yaml(*parts):
    with open(os.path.join(CONFIG_DIR, *parts)) as f:
        return _scalars(yaml.safe_load(f) or {})


def _set(cfg: dict, dotted: str, value):
    node = cfg
    keys = dotted.split(".")
    for k in keys[:-1]:
        node = node.setdefault(k, {})
    node[keys[-1]] = value


def compose(overrides) -> dict:
    """defaults list + group selection (``model=NAME``) + dotted overrides (values parsed as YAML scalars)."""
    root = _load_yaml("predict.yaml")
    groups = {}
    for d in root.pop("defaults", []):
        groups.update(d)
    dotted = []
    for ov in overrides:
        k, _, v = ov.partition("=")
        if k in groups and "." not in k:
            groups[k] = v
        else:
            dotted.append((k, _scalars(yaml.safe_load(v))))
    cfg = dict(root)
    for g, name in groups.items():
        cfg[g] = _load_yaml(g, f"{name}.yaml")
    for k, v in dotted:
        _set(cfg, k, v)
    return cfg


def instantiate(node, **extra):
    """Minimal ``hydra.utils.instantiate``: dicts with ``_target_`` become objects, recursively."""
    if isinstance(node, dict):
        kw = {k: instantiate(v) for k, v in node.items() if k != "_target_"}
        if "_target_" in node:
            mod, _, name = node["_target_"].rpartition(".")
            return getattr(importlib.import_module(mod), name)(**kw, **extra)
        return kw
    if isinstance(node, list):
        return [instantiate(v) for v in node]
    return node


def _model_rate_samples(batch: dict, model):
    """``data.restore_rate`` / ``data.restore_level``: for every item the samples its file holds without the flags, read back (the 16-bit codes over 32768, or
    the float32 samples) - what ``metrics.csv`` and ``losses.csv`` are computed from, so that the flags do not change them.  The
    quantisation is the hand-off's (``handoff.wav_handoff`` without normalisation: bit for bit the file round trip)."""
    from .handoff import wav_handoff
    wavs = batch["fake" if hasattr(model, "G") else "enhanced"]
    rows = wav_handoff(wavs.detach().float().contiguous(), batch["sample_length"], model.wav_subtype, normalize=False)[0].cpu().numpy()
    return [rows[i, : int(n)] for i, n in enumerate(batch["sample_length"])]


def _scored_files(batch: dict, clean_folder: str):
    """``data.channels=all``: (first row, C, relative path, clean path, enhanced path) of every file of the batch whose clean
    counterpart exists and has the file's channel count; a clean file with another channel count is skipped and named on stderr."""
    from .wavio import wav_info
    for r, c in batch["file_rows"]:
        noisy_path = batch["audio_path"][r]
        rel = os.path.relpath(noisy_path, batch["data_folder"])
        clean_path = os.path.join(clean_folder, rel)
        if not os.path.isfile(clean_path):
            continue
        have = wav_info(clean_path)[1]
        if have != c:
            print(f"skipping {rel}: the clean file has {have} channel(s), the noisy file {c}", file=sys.stderr)
            continue
        yield r, c, rel, clean_path, noisy_path.replace(batch["data_folder"], batch["target_folder"])


def _warn_short(rel: str, row: dict, what: str = ""):
    """``data.intelligibility``: one line for a file too short for a STOI segment (its two scores are pystoi's 1e-5)."""
    from .metrics import STOI_MIN_FRAMES
    if row.get("stoi_frames", STOI_MIN_FRAMES) < STOI_MIN_FRAMES:
        print(f"warning: {rel}{what}: {int(row['stoi_frames'])} frame(s) after the silent ones are removed, STOI needs {STOI_MIN_FRAMES}: "
              f"stoi and estoi are {row['stoi']:g}", file=sys.stderr)


def _score_batch(batch: dict, clean_folder: str, data_cfg: dict, device, est=None):
    """``data.clean_folder``: (relative path, metrics) of every file of the batch whose clean counterpart exists - the enhanced file as
    ``predict_step`` wrote it (``est``: its samples at the model's rate, item by item, where the files are not at that rate) against
    the clean file, the noisy input as the noise source (``metrics.score_files``)."""
    from .metrics import score_files
    rows = []
    stoi = bool(data_cfg.get("intelligibility"))              # data.intelligibility: stoi and estoi join the row
    if "file_rows" in batch:                                  # data.channels=all: one row per (file, channel)
        for r, c, rel, clean_path, enhanced_path in _scored_files(batch, clean_folder):
            for k in range(c):
                rows.append((rel, k, score_files(enhanced_path, clean_path, batch["audio_path"][r], int(data_cfg.get("sampling_rate", 24000) or 0),
                                                 bool(data_cfg.get("normalize", True)), device, None if est is None else est[r + k], channel=k,
                                                 intelligibility=stoi)))
                _warn_short(rel, rows[-1][-1], f" channel {k}")
        return rows
    for i, noisy_path in enumerate(batch["audio_path"]):
        rel = os.path.relpath(noisy_path, batch["data_folder"])
        clean_path = os.path.join(clean_folder, rel)
        if os.path.isfile(clean_path):
            enhanced_path = noisy_path.replace(batch["data_folder"], batch["target_folder"])
            rows.append((rel, score_files(enhanced_path, clean_path, noisy_path, int(data_cfg.get("sampling_rate", 24000) or 0),
                                          bool(data_cfg.get("normalize", True)), device, None if est is None else est[i], intelligibility=stoi)))
            _warn_short(rel, rows[-1][-1])
    return rows


def _loss_batch(batch: dict, clean_folder: str, data_cfg: dict, device, est=None):
    """``data.convergence_losses``: (relative path, convergence losses) of the files ``_score_batch`` scores (``losses.score_files``)."""
    from .losses import score_files
    rows = []
    if "file_rows" in batch:
        for r, c, rel, clean_path, enhanced_path in _scored_files(batch, clean_folder):
            for k in range(c):
                rows.append((rel, k, score_files(enhanced_path, clean_path, int(data_cfg.get("sampling_rate", 24000) or 0),
                                                 bool(data_cfg.get("normalize", True)), device, None if est is None else est[r + k], channel=k)))
        return rows
    for i, noisy_path in enumerate(batch["audio_path"]):
        rel = os.path.relpath(noisy_path, batch["data_folder"])
        clean_path = os.path.join(clean_folder, rel)
        if os.path.isfile(clean_path):
            enhanced_path = noisy_path.replace(batch["data_folder"], batch["target_folder"])
            rows.append((rel, score_files(enhanced_path, clean_path, int(data_cfg.get("sampling_rate", 24000) or 0),
                                          bool(data_cfg.get("normalize", True)), device, None if est is None else est[i])))
    return rows


def _load_pipeline_weights(model, cfg: dict, device):
    """``model=USE``: ``ckpt_path`` serves the score network and ``refine_ckpt_path`` the generator, each a Lightning ``.ckpt`` or a
    packed ``.usehip`` file; without either, ``random_init_seed=S`` gives both networks the weights the two single-stage dry runs get
    from the same seed."""
    stages = (("score", "ckpt_path", model.Score.score_net, model.Score), ("refine", "refine_ckpt_path", model.G.net, model.G))
    paths = [cfg.get(key) for _, key, _, _ in stages]
    if not any(paths):
        if cfg.get("random_init_seed") is None:
            raise SystemExit("ckpt_path and refine_ckpt_path are required (or random_init_seed=<int> for a dry run)")
        from .testing.weights import LARGE, REFINE, make_state_dict
        for (_, _, net, _), arch in zip(stages, (LARGE, REFINE)):
            net.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(int(cfg["random_init_seed"]), **arch).items()})
        return
    for (_, key, _, _), path in zip(stages, paths):
        if not path:
            raise SystemExit(f"model=USE needs both ckpt_path (the score network) and refine_ckpt_path (the generator): {key} is missing")
    for (stage, key, net, owner), path in zip(stages, paths):
        if str(path).endswith(".usehip"):
            net.load_weight_file(path, n_freq=int(owner.n_fft) // 2 + 1, device=device)
        else:
            model.load_lightning_checkpoint(path, stage)


def predict(cfg: dict):
    with_losses = bool(cfg["data"].get("convergence_losses"))   # off by default: nothing of it runs, no losses.csv is written
    if with_losses and not cfg["data"].get("clean_folder"):
        raise SystemExit("data.convergence_losses=true needs data.clean_folder=<the folder of the clean files>")
    with_stoi = bool(cfg["data"].get("intelligibility"))       # off by default: nothing of it runs, metrics.csv keeps its four columns
    if with_stoi and not cfg["data"].get("clean_folder"):
        raise SystemExit("data.intelligibility=true needs data.clean_folder=<the folder of the clean files>")
    rank, world, local = D.init_from_env()
    torch.cuda.set_device(local)
    data = instantiate(cfg["data"], rank=rank, world_size=world)
    model = instantiate(cfg["model"])
    device = torch.device("cuda", local)
    both = hasattr(model, "G") and hasattr(model, "Score")   # model=USE: the two stages in one run
    owner = model.Score if both else model.G if hasattr(model, "G") else model.Score   # the module that carries n_fft and hop_length
    if both:
        _load_pipeline_weights(model, cfg, device)
    elif cfg.get("ckpt_path") and str(cfg["ckpt_path"]).endswith(".usehip"):   # packed weight file (pack_checkpoint)
        net = model.G.net if hasattr(model, "G") else model.Score.score_net
        net.load_weight_file(cfg["ckpt_path"], n_freq=int(owner.n_fft) // 2 + 1, device=device)
    elif cfg.get("ckpt_path"):
        model.load_lightning_checkpoint(cfg["ckpt_path"])
    elif cfg.get("random_init_seed") is not None:
        from .testing.weights import LARGE, REFINE, make_state_dict
        refine = hasattr(model, "G")                          # model=LSGAN: the refine-stage generator
        sd = make_state_dict(int(cfg["random_init_seed"]), **(REFINE if refine else LARGE))
        (model.G.net if refine else model.Score.score_net).load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    else:
        raise SystemExit("ckpt_path is required (or random_init_seed=<int> for a dry run)")
    n = 0
    clean_folder = cfg["data"].get("clean_folder")           # off by default: nothing below runs, no CSV is written
    rows, loss_rows = [], []
    per_channel = cfg["data"].get("channels", "first") == "all"   # one CSV row per (file, channel), and a channel column
    with torch.no_grad():
        for i, batch in enumerate(data.predict_batches(device=device, frame_hop=owner.hop_length)):
            model.predict_step(batch, i)
            n += len(batch["file_rows"] if "file_rows" in batch else batch["name"])   # files, not rows
            est = _model_rate_samples(batch, model) if clean_folder and ("source_rate" in batch or "source_gain" in batch) else None
            if clean_folder:
                rows += _score_batch(batch, clean_folder, cfg["data"], device, est)
            if with_losses:
                loss_rows += _loss_batch(batch, clean_folder, cfg["data"], device, est)
    if clean_folder:
        from .metrics import NAMES, STOI_NAMES, write_csv
        write_csv(os.path.join(cfg["data"]["target_folder"], "metrics.csv" if world == 1 else f"metrics_rank{rank}.csv"), rows, per_channel,
                  NAMES + STOI_NAMES if with_stoi else NAMES)
    if with_losses:
        from .losses import write_csv as write_losses_csv
        write_losses_csv(os.path.join(cfg["data"]["target_folder"], "losses.csv" if world == 1 else f"losses_rank{rank}.csv"), loss_rows,
                         per_channel)
    print(f"[rank {rank}] enhanced {n} file(s) -> {cfg['data']['target_folder']}")
    return n


def main(argv=None):
    predict(compose(list(sys.argv[1:] if argv is None else argv)))


if __name__ == "__main__":
    main()
