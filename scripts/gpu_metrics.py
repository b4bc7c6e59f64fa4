"""The device metrics on the GPU (profiles/metrics.txt): every item of tests/golden/metrics.npz against the reference's values, and
the time of one ``use_metrics`` call for 8 x 4 s at 24 kHz between HIP events after a warm-up call.  Run from the repository root:

    python scripts/gpu_metrics.py
"""
import os
import sys

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
import torch

import metrics_ref as mr
from universal_speech_enhancement_amd import metrics
from universal_speech_enhancement_amd.testing import noise as tn


def main():
    g = np.load(mr.GOLDEN)
    print("item               |d SI-SDR| |d SI-SIR| |d SI-SAR| dB   LSD device          LSD reference (f32)  |d LSD|     f32 vs f64")
    for name, _, _, _ in mr.CASES:
        c = mr.load_case(g, name)
        e, s, n = (torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("est", "clean", "noise"))
        out = metrics._run(e, s, n, c["lengths"]).cpu().numpy()
        for b, L in enumerate(c["lengths"]):
            d = np.abs(out[b, :3] - c["ratios"][b])
            print(f"{name}[{b}] L={L:<6d} {d[0]:10.3e} {d[1]:10.3e} {d[2]:10.3e}      {out[b, 3]:.15f}   {c['lsd'][b]:.15f}   "
                  f"{abs(out[b, 3] - c['lsd'][b]):.3e}  {c['lsd_f32_vs_f64'][b]:.3e}")
    B, L = 8, 4 * 24000
    clean = torch.from_numpy(tn.synth_noisy_speech(B, L, seed=5)).cuda()
    noise = torch.from_numpy(0.05 * tn.normal(6, "n", B * L).reshape(B, L)).cuda()
    est = clean + 0.3 * noise
    metrics._run(est, clean, noise, None)                                  # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(20):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = metrics._run(est, clean, noise, None)
        z.record()
        z.synchronize()
        ms.append(a.elapsed_time(z))
    print(f"use_metrics, {B} x {L} samples (workspace allocation of the Python wrapper included): "
          f"median {np.median(ms):.3f} ms, min {min(ms):.3f} ms, max {max(ms):.3f} ms over {len(ms)} calls")
    print("values:", out.cpu().numpy().round(4).tolist())


if __name__ == "__main__":
    main()
