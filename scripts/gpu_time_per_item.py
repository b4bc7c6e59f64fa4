#!/usr/bin/env python3
"""GPU measurement of the batch-invariant (per-item) form of the fused PC sampler beside the default form (not a test), at the
BASELINE configs[1] shape: 8 utterances x 4 s of synthetic 24 kHz noisy speech ([8,1,512,640]), N = 30, reverse diffusion + Langevin x 1
(60 NFE), bf16 storage, hipGraph replay, device noise.  Both forms run in one process on one plan, interleaved: warm-up replays of each
(plan, graph capture), then timed replays alternating default / per-item; every replay is timed by a host clock around the call and a
device synchronise.  Prints one JSON line and, with --out, writes the text report kept under profiles/.

    python scripts/gpu_time_per_item.py [--warmup 3] [--reps 10] [--out profiles/per_item_sampling.txt]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from universal_speech_enhancement_amd.seeding import item_seeds  # noqa: E402
from universal_speech_enhancement_amd.sgmse.model_wrapper import ScoreModel  # noqa: E402
from universal_speech_enhancement_amd.testing import noise as tn  # noqa: E402
from universal_speech_enhancement_amd.testing import weights as tw  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_time_per_item.py measures on the GPU: no device found")
    torch.cuda.set_device(0)
    m = ScoreModel(backbone="ncsnpplarge", sde="ouve", t_eps=3e-2, condition="noisy", n_fft=1022, hop_length=160, num_frames=512,
                   window="hann", sde_input="noisy", predictor="reverse_diffusion", corrector="langevin", precision=a.precision)
    m.score_net.load_state_dict({k: torch.from_numpy(v) for k, v in tw.make_state_dict(1234, **tw.LARGE).items()})
    wav = torch.from_numpy(tn.synth_noisy_speech(a.batch, int(24000 * a.seconds), seed=1234)).cuda()
    Y = m._spectrogram(wav).contiguous()
    eng = m.score_net.engine(Y.shape[2], Y.device)
    eng.plan(Y.shape[0], Y.shape[3])
    eng.set_sampler(a.steps, "reverse_diffusion", "langevin", 1, 0.5, 3e-2, use_graph=True)
    seeds = item_seeds(0, a.batch)
    forms = {"default": lambda: eng.sample(Y, seed=0), "per_item": lambda: eng.sample(Y, item_seeds=seeds)}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    outs = {}
    for _ in range(a.warmup):
        for name, fn in forms.items():
            outs[name] = timed(fn)[1]
    captures = eng.stat("graph_captures")
    walls = {name: [] for name in forms}
    for _ in range(a.reps):
        for name, fn in forms.items():
            walls[name].append(timed(fn)[0])
    assert eng.stat("graph_captures") == captures, "a timed replay re-captured a graph"
    nfe = 2 * a.steps
    res = {"shape": list(Y.shape), "precision": a.precision, "N": a.steps, "nfe": nfe, "warmup": a.warmup, "reps": a.reps,
           "graph_captures": captures, "finite": all(bool(torch.isfinite(torch.view_as_real(o)).all()) for o in outs.values())}
    for name, w in walls.items():
        w = np.array(w)
        res[name] = {"mean_s": round(float(w.mean()), 5), "std_s": round(float(w.std(ddof=1)), 5), "min_s": round(float(w.min()), 5),
                     "max_s": round(float(w.max()), 5), "ms_per_evaluation": round(float(w.mean()) / nfe * 1e3, 4),
                     "all_s": [round(float(v), 5) for v in w]}
    d, p = res["default"], res["per_item"]
    res["per_item_minus_default_s"] = round(p["mean_s"] - d["mean_s"], 5)
    res["default_spread_s"] = round(d["max_s"] - d["min_s"], 5)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write("Per-item (batch-invariant) form of the fused PC sampler beside the default form: scripts/gpu_time_per_item.py on one MI355X\n")
            f.write(f"shape {res['shape']}, N = {a.steps}, reverse diffusion + Langevin x 1 ({nfe} NFE), {a.precision}, hipGraph replay, device noise\n")
            f.write(f"one process, one plan, {a.warmup} warm-up replays of each form, then {a.reps} timed replays of each, alternating;\n")
            f.write("wall time of one replay = host clock around the call and a device synchronise\n\n")
            for name in forms:
                r = res[name]
                f.write(f"{name:9s} mean {r['mean_s'] * 1e3:9.2f} ms   std {r['std_s'] * 1e3:6.2f} ms   min {r['min_s'] * 1e3:9.2f}   max {r['max_s'] * 1e3:9.2f}"
                        f"   ({r['ms_per_evaluation']:.3f} ms per network evaluation of the batch)\n")
            f.write(f"\nper-item minus default (means): {res['per_item_minus_default_s'] * 1e3:+.2f} ms\n")
            f.write(f"run-to-run spread of the default form (max - min of its {a.reps} replays): {res['default_spread_s'] * 1e3:.2f} ms\n\n")
            for name in forms:
                f.write(f"{name} replays (s): {res[name]['all_s']}\n")


if __name__ == "__main__":
    main()
