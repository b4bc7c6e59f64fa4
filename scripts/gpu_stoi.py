"""Device-side STOI / ESTOI on the GPU (profiles/stoi.txt): every case of tests/stoi_ref.py against the float64 restatement, then the time of
one ``use_stoi`` call between stream events after a warm-up call - a batch of 8 x 4 s at 24 kHz, and one item of 60 s - beside the numpy /
scipy restatement of the same inputs on the host, and beside ``use_metrics`` (SI-SDR / SI-SIR / SI-SAR / LSD) on the same batch: what
``data.intelligibility=true`` adds per file.  Run from the repository root:

    python scripts/gpu_stoi.py
"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
import torch

import stoi_ref as sr
from universal_speech_enhancement_amd import _lib, metrics


def timed(fn, n=20):
    fn()                                                                   # warm-up: code objects, the allocator's pool
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        z.record()
        z.synchronize()
        ms.append(a.elapsed_time(z))
    return out, float(np.median(ms)), f"median {np.median(ms):.3f} ms, min {min(ms):.3f} ms, max {max(ms):.3f} ms over {n} calls"


def shape(B, L, rate, label):
    clean = np.stack([sr.am_noise(L, rate, 70 + b) for b in range(B)])
    est = np.stack([sr.degrade(clean[b], (20.0, 0.0, -10.0)[b % 3], 70 + b) for b in range(B)])
    c, e = torch.from_numpy(clean).cuda(), torch.from_numpy(est).cuda()
    lib = _lib.lib()
    nbytes = lib.use_stoi_workspace(B, L, rate)
    work = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device="cuda")
    out = torch.empty((B, 3), dtype=torch.float64, device="cuda")
    lens = (C.c_int * B)(*([L] * B))
    stream = torch.cuda.current_stream().cuda_stream

    def device():
        assert lib.use_stoi(e.data_ptr(), c.data_ptr(), lens, B, L, rate, work.data_ptr(), nbytes, out.data_ptr(), stream) == 0
        return out

    got, t_dev, line = timed(device)
    print(f"use_stoi, {label}: {B} x {L} samples at {rate} Hz (workspace of {nbytes} bytes allocated once): {line}")
    _, t_py, line = timed(lambda: metrics.intelligibility(e, c, None, rate))
    print(f"metrics.intelligibility, the same call with the workspace allocation of the Python wrapper: {line}")
    noise = (e - c).contiguous()
    _, t_met, line = timed(lambda: metrics._run(e, c, noise, None))
    print(f"use_metrics on the same batch (SI-SDR / SI-SIR / SI-SAR / LSD, wrapper included): {line}")
    print(f"data.intelligibility per file: {t_py / B:.3f} ms on top of {t_met / B:.3f} ms of use_metrics ({t_py / t_met:.2f} x)")
    t0 = time.perf_counter()
    want = np.array([sr.scores(clean[b], est[b], rate) for b in range(B)])
    t_host = (time.perf_counter() - t0) * 1e3
    d = np.abs(got.cpu().numpy() - want)
    print(f"the numpy / scipy restatement of the same {B} item(s) on the host, one pass: {t_host:.1f} ms ({t_host / t_dev:.0f} x the device call); "
          f"largest distance stoi {d[:, 0].max():.2e}, estoi {d[:, 1].max():.2e}, frames equal: {bool((d[:, 2] == 0).all())}")


def main():
    print("case            item  stoi (device)        estoi (device)       frames  |stoi - ref|  |estoi - ref|")
    for name in sr.CASE_NAMES:
        rate, _, lengths, clean, est = sr.build(name)
        r = metrics.intelligibility(torch.tensor(est).cuda(), torch.tensor(clean).cuda(), lengths, rate)
        for b, (d, e, T) in enumerate(sr.expected(name)):
            gd, ge, gT = (float(r[k][b]) for k in ("stoi", "estoi", "stoi_frames"))
            print(f"{name:<15s} {b:<5d} {gd:<20.16g} {ge:<20.16g} {int(gT):<7d} {abs(gd - d):<13.2e} {abs(ge - e):.2e}" + ("" if gT == T else "  FRAMES DIFFER"))
    shape(8, 4 * 24000, 24000, "a batch of 8 x 4 s")
    shape(1, 60 * 24000, 24000, "one item of 60 s")


if __name__ == "__main__":
    main()
