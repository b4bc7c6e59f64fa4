#!/usr/bin/env python3
"""GPU measurement of the probability-flow ODE sampler at the configs[1] shape (not a test): 8 utterances x 4 s of synthetic
24 kHz noisy speech, bf16 storage, RK45 rtol = atol = 1e-5 with one step-size controller per item (ScoreModel.get_ode_sampler's
minibatch=1), denoise step on.  Prints NFE per item, wall time per batch, ms per network evaluation of the batch, and the share of
evaluations spent on items whose integration had already finished (finished items are still evaluated until the last one ends),
then the same batch's PC sampler (N = 30, reverse diffusion + Langevin = 60 NFE) for ms per evaluation on the same box.  One JSON line.

    python scripts/gpu_time_ode.py [--reps 3] [--group 1] [--precision bf16]
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

from universal_speech_enhancement_amd.sgmse.model_wrapper import ScoreModel  # noqa: E402
from universal_speech_enhancement_amd.testing import noise as tn  # noqa: E402
from universal_speech_enhancement_amd.testing import weights as tw  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--group", type=int, default=1, help="items per step-size controller (0: one integration over the batch)")
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=4.0)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    m = ScoreModel(backbone="ncsnpplarge", sde="ouve", t_eps=3e-2, condition="noisy", n_fft=1022, hop_length=160, num_frames=512,
                   window="hann", sde_input="noisy", predictor="reverse_diffusion", corrector="langevin", precision=a.precision)
    m.score_net.load_state_dict({k: torch.from_numpy(v) for k, v in tw.make_state_dict(1234, **tw.LARGE).items()})
    wav = torch.from_numpy(tn.synth_noisy_speech(a.batch, int(24000 * a.seconds), seed=1234)).cuda()
    Y = m._spectrogram(wav).contiguous()
    eng = m.score_net.engine(Y.shape[2], Y.device)
    eng.plan(Y.shape[0], Y.shape[3])

    def ode():
        x, nfev, status = m.fused_sample_ode(Y, N=30, t_eps=3e-2, group=a.group, seed=0, cond=Y)
        torch.cuda.synchronize()
        return x, nfev, status

    x, nfev, status = ode()                                     # warm-up: plan, graph capture
    walls = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        x, nfev, status = ode()
        walls.append(time.perf_counter() - t0)
    wall = float(np.median(walls))
    evals = eng.stat("ode_nfev_max") + 1                        # batch evaluations: every item runs until the last group ends, + denoise
    G = a.group or a.batch
    per_item = [n for n in nfev for _ in range(G)][: a.batch]
    wasted = 1.0 - sum(per_item) / (len(per_item) * eng.stat("ode_nfev_max"))

    pc = m.get_pc_sampler("reverse_diffusion", "langevin", Y, N=30, corrector_steps=1, snr=0.5, conditioning=[Y])
    pc(); torch.cuda.synchronize()
    pw = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        pc(); torch.cuda.synchronize()
        pw.append(time.perf_counter() - t0)
    pc_wall = float(np.median(pw))
    print(json.dumps({
        "shape": list(Y.shape), "precision": a.precision, "group": a.group, "rtol": 1e-5, "atol": 1e-5,
        "nfe_per_group": nfev, "status": status, "accepted_steps": eng.stat("ode_steps"), "rejected_steps": eng.stat("ode_rejected"),
        "batch_evaluations": evals, "wall_s_per_batch": round(wall, 4), "wall_s_all": [round(w, 4) for w in walls],
        "ms_per_batch_evaluation": round(wall / evals * 1e3, 3),
        "evaluations_on_finished_items": round(wasted, 4),
        "pc_wall_s_per_batch": round(pc_wall, 4), "pc_ms_per_batch_evaluation": round(pc_wall / 60 * 1e3, 3),
        "finite": bool(torch.isfinite(torch.view_as_real(x)).all()),
    }))


if __name__ == "__main__":
    main()
