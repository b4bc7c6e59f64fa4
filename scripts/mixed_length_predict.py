"""Mixed-length folder through ``predict``: own-length sampling with length buckets against the default (pad to the batch's longest).

Builds a folder of synthetic utterances with a fixed seed (default: 64 files, lengths uniform in 1 ... 8 s at 24 kHz), runs ``predict``
with ``random_init_seed`` at ``data.batch_size`` 8 once with the new options off and once with ``model.sampler_kwargs.own_length`` +
``data.bucket_by_length`` (+ ``per_item``) on, and prints files/s and the total of padded frames the score network saw for both.
The frame totals are exact: sum over files of T'_b with the options on, sum over batches of B x max T' with them off
(``frame_counts``; tests/test_own_length_host.py asserts them).  Each configuration runs the folder twice and the second pass is timed:
what the process pays once (code objects, the file cache) is outside the timed region, while plan building and graph capture are inside it
for both configurations, since every ``predict`` call builds its own model and handle.

    python scripts/mixed_length_predict.py [--files 64] [--batch-size 8] [--N 30] [--precision bf16] [--seed 0] [--keep DIR]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SR, HOP = 24000, 160


def lengths(n=64, seed=0, lo_s=1.0, hi_s=8.0, sr=SR):
    """The stated length distribution: n lengths in samples, uniform in [lo_s, hi_s) seconds, from numpy's RandomState(seed)."""
    return [int(v * sr) for v in np.random.RandomState(seed).uniform(lo_s, hi_s, n)]


def pad64(T):
    return (T + 63) // 64 * 64


def frame_counts(lens, batch_size, hop=HOP):
    """(frames with every file at its own T', frames with consecutive batches padded to their longest file)."""
    Tp = [pad64(1 + L // hop) for L in lens]
    padded = sum(len(Tp[i:i + batch_size]) * max(Tp[i:i + batch_size]) for i in range(0, len(Tp), batch_size))
    return sum(Tp), padded


def build_folder(folder, lens, seed=0):
    from universal_speech_enhancement_amd.testing import noise as tn
    from universal_speech_enhancement_amd.wavio import FLOAT32, write_wav
    os.makedirs(folder, exist_ok=True)
    for i, L in enumerate(lens):                              # names sort in index order: the default loader's batches are lens[i:i+B]
        write_wav(os.path.join(folder, f"utt_{i:03d}.wav"), tn.synth_noisy_speech(1, L, seed=seed * 1000 + i)[0], SR, FLOAT32)


def run(src, dst, args, on):
    import torch
    from universal_speech_enhancement_amd import predict as P
    ov = ["model=SGMSE_Large", f"random_init_seed={args.weights_seed}", f"data.data_folder={src}", f"data.target_folder={dst}",
          f"data.batch_size={args.batch_size}", f"model.Score.precision={args.precision}", f"model.sampler_kwargs.N={args.N}",
          "model.wav_subtype=FLOAT"]
    if on:
        ov += ["model.sampler_kwargs.own_length=true", "model.sampler_kwargs.per_item=true", "data.bucket_by_length=true"]
    cfg = P.compose(ov)
    times = []
    for _ in range(2):                                        # the second pass is the measurement
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = P.predict(cfg)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return n, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--N", type=int, default=30)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--weights-seed", type=int, default=1234)
    ap.add_argument("--keep", default=None, help="build the folders here and keep them (default: a temporary directory)")
    args = ap.parse_args()
    lens = lengths(args.files, args.seed)
    own, padded = frame_counts(lens, args.batch_size)
    with tempfile.TemporaryDirectory() as tmp:
        base = args.keep or tmp
        src = os.path.join(base, "noisy")
        build_folder(src, lens, args.seed)
        res = {"files": args.files, "batch_size": args.batch_size, "N": args.N, "precision": args.precision,
               "seconds_of_audio": sum(lens) / SR, "frames_off": padded, "frames_on": own, "frame_ratio": padded / own}
        for name, on in (("off", False), ("on", True)):
            n, times = run(src, os.path.join(base, "enhanced_" + name), args, on)
            assert n == args.files
            res[f"seconds_{name}_first_pass"] = times[0]
            res[f"seconds_{name}"] = times[1]
            res[f"files_per_s_{name}"] = n / times[1]
        res["speedup"] = res["seconds_off"] / res["seconds_on"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
