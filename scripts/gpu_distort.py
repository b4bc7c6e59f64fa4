"""The degradation simulator on the GPU (profiles/distort.txt): every case of tests/distort_ref.py against the float64 restatement - the
largest ratio of max |device - restatement| to the bound max(8 err_ref, 16 * 2^-52) * peak per stage - then the time of one
``use_distort`` call between stream events after a warm-up call, all stages on with a RIR of 0.5 s, for 4 x 6 s and 8 x 4 s at 24 kHz,
beside the float64 numpy / scipy restatement of the same batch on the host (one process, one pass) and, for scale, one bf16 training
step of the large score network on a batch of 4.  Run from the repository root:

    python scripts/gpu_distort.py [--no-train]
"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
import torch

import distort_ref as dr
import test_hip_distort as td
from universal_speech_enhancement_amd import _lib, distort


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


def accuracy():
    print("case                 item  output     ratio to the bound   err_ref (x 2^-52)")
    worst = {}
    for name in dr.CASES:
        for b, k, ratio, same in td.ratios(name):
            err = dr.expected(name)[b][1][k] / td.EPS
            print(f"{name:<20s} {b:<5d} {k:<10s} {ratio:<20.3f} {err:.2f}" + ("  bit-equal" if same else ""))
            stage = name.partition("@")[0]
            worst[stage] = max(worst.get(stage, 0.0), ratio)
    print("largest ratio per stage: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def long_rir(taps, seed):
    """float32 [taps] through ``prepare_rir``: decaying noise, clipped under the direct path of 1 at tap 0."""
    rng = np.random.default_rng(seed)
    h = np.clip(rng.standard_normal(taps) * np.exp(-np.arange(taps) / (taps / 6.0)) * 0.3, -0.9, 0.9)
    h[0] = 1.0
    return distort.prepare_rir(h)


def shape(B, seconds, label, rate=24000, taps=12000):
    L = seconds * rate
    clean = np.stack([dr.speechlike(L, 700 + b) for b in range(B)])
    noise = np.stack([0.3 * dr.speechlike(L, 800 + b) for b in range(B)]).astype(np.float32)
    rir = np.stack([long_rir(taps, 900 + b) for b in range(B)])
    kinds = (dict(clip_kind="hard_on_rate", clip_a=0.05), dict(clip_kind="soft", clip_a=2.0), dict(clip_kind="sigmoid1", clip_a=2.0, clip_b=1.5),
             dict(clip_kind="sigmoid2", clip_a=0.5, clip_b=2.0))
    recipes = [dr._recipe(L, 1000 + b, reverb=True, snr=15.0, loudness=(0.5, 2.0, 1.5), dc_offset=0.01, packet_frame=480, volume="peak",
                          volume_target=0.5, normalize=True, **kinds[b % 4]) for b in range(B)]
    c, nz, h = torch.from_numpy(clean).cuda(), torch.from_numpy(noise).cuda(), torch.from_numpy(rir).cuda()
    lib = _lib.lib()
    P, packets = distort.params_of(recipes, [L] * B, [taps] * B)
    pk = torch.from_numpy(packets).cuda()
    nbytes = lib.use_distort_workspace(L, taps)
    work = torch.empty(nbytes // 8 + 2, dtype=torch.float64, device="cuda")
    pert, target = torch.empty((B, L), device="cuda"), torch.empty((B, L), device="cuda")
    scal = torch.empty((B, 8), dtype=torch.float64, device="cuda")
    lens = (C.c_int * B)(*([L] * B))
    stream = torch.cuda.current_stream().cuda_stream

    def device():
        assert lib.use_distort(c.data_ptr(), nz.data_ptr(), h.data_ptr(), pk.data_ptr(), packets.size, lens, lens, P, B, L, L, taps, 0,
                               pert.data_ptr(), target.data_ptr(), scal.data_ptr(), None, 0, work.data_ptr(), nbytes, stream) == 0
        return pert

    got, t_dev, line = timed(device)
    print(f"use_distort, {label}: {B} x {L} samples at {rate} Hz, all stages on, RIR of {taps} taps (workspace of {nbytes} bytes allocated once): {line}")
    _, t_py, line = timed(lambda: distort.distort_batch(c, [L] * B, recipes, noise=nz, rir=h))
    print(f"distort.distort_batch, the same call with the allocations and the parameter records of the Python wrapper: {line}")
    t0 = time.perf_counter()
    want = [dr.chain(clean[b], recipes[b], noise[b], rir[b]) for b in range(B)]
    t_host = (time.perf_counter() - t0) * 1e3
    d = max(float(np.abs(got[b].cpu().numpy() - want[b]["perturbed"].astype(np.float32)).max()) for b in range(B))
    print(f"the float64 numpy / scipy restatement of the same {B} items on the host, one process, one pass: {t_host:.1f} ms "
          f"({t_host / t_dev:.0f} x the device call; {t_host / B:.1f} ms per item); largest float32 distance {d:.2e}")
    return t_dev


def train_step(B=4, frames=512, steps=5):
    from universal_speech_enhancement_amd.sgmse.model_wrapper import ScoreModel
    torch.manual_seed(0)
    m = ScoreModel(backbone="ncsnpplarge", sde="ouve", t_eps=3e-2, condition="noisy", n_fft=1022, hop_length=160, num_frames=frames,
                   window="hann", sde_input="noisy", precision="fp32").cuda()
    m.score_net.requires_grad_(True)
    m.score_net.train_precision = "bf16"
    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=5e-4, weight_decay=1e-7)
    L = (frames - 1) * 160 + 4000
    clean = torch.randn(B, L, device="cuda") * 0.1
    batch = {"clean": clean, "perturbed": clean + 0.05 * torch.randn_like(clean)}

    def step():
        opt.zero_grad(set_to_none=True)
        loss = m.train_step(batch)
        loss.backward()
        opt.step()

    for _ in range(2):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    accuracy()
    a = shape(4, 6, "a batch of 4 x 6 s")
    shape(8, 4, "a batch of 8 x 4 s")
    if "--no-train" not in sys.argv:
        t = train_step()
        print(f"for scale: one bf16 training step of the large score network, batch of 4 x 512 frames: {t:.1f} ms ({a / t * 100:.1f} % of it is the 4 x 6 s use_distort call)")


if __name__ == "__main__":
    main()
