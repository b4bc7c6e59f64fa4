"""The device convergence losses on the GPU (profiles/spec_losses.txt): every item of tests/golden/spec_losses.npz against the float64
restatement and the reference's float32 values, then the time of one ``use_spec_losses`` call for 8 x 4 s at 24 kHz (stride 96000)
between stream events after a warm-up call, beside the same arithmetic written with ``torch.stft`` calls on the same GPU (float64, and
float32 as the reference runs it).  Run from the repository root:

    python scripts/gpu_spec_losses.py
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
import torch

import spec_losses_ref as sl
from universal_speech_enhancement_amd import _lib, losses
from universal_speech_enhancement_amd.testing import noise as tn


def torch_terms(est, clean, sr, dtype, fb):
    """The 15 per-item values from torch.stft calls: five transforms of either signal, the filter bank as a matmul."""
    e, c = est.to(dtype), clean.to(dtype)
    out = [(e - c).abs().mean(1)]
    l2, lg, nm = [], [], []

    def mag(x, n, hop, win):
        return torch.stft(x, n, hop_length=hop, win_length=win, window=torch.hann_window(win, dtype=dtype, device=x.device), center=True,
                          pad_mode="reflect", return_complex=True).abs()

    def log_l1(a, b):
        return (torch.log(a * 32768 + 1e-6) - torch.log(b * 32768 + 1e-6)).abs().mean((1, 2))

    for n in sl.frame_lengths(sr):
        me, mc = mag(e, n, n // 4, n), mag(c, n, n // 4, n)
        l2.append(((me - mc) ** 2).mean((1, 2)))
        lg.append(log_l1(me, mc))
        nm.append(((mc - me) ** 2).sum((1, 2)).sqrt() / ((mc ** 2).sum((1, 2)).sqrt() + 1e-6))
    me, mc = (torch.matmul(fb.T, mag(x, 2048, int(0.010 * sr), int(0.025 * sr))) for x in (e, c))
    return torch.stack(out + l2 + lg + nm + [log_l1(me, mc), ((me - mc) ** 2).mean((1, 2))], 1)


def timed(fn, n=20):
    fn()                                                                   # warm-up: code objects, rocFFT plans, the allocator's pool
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        z.record()
        z.synchronize()
        ms.append(a.elapsed_time(z))
    return out, f"median {np.median(ms):.3f} ms, min {min(ms):.3f} ms, max {max(ms):.3f} ms over {n} calls"


def main():
    g = np.load(sl.GOLDEN)
    print("item              against the float64 restatement: relative (wav_l1, l2_r, norm_r, mel_l2), absolute (log_r, mel_log); "
          "six terms against the reference's float32 values, largest distance / its f32-vs-f64")
    rel_i, abs_i = [0, 1, 2, 3, 4, 9, 10, 11, 12, 14], [5, 6, 7, 8, 13]
    for name, rate, _, _, lengths in sl.CASES:
        c = sl.load_case(g, name)
        e, s = (torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("est", "clean"))
        out = losses.spec_loss_terms(e, s, c["lengths"], rate).cpu().numpy()
        for b, L in enumerate(lengths):
            want = sl.item_values(c["est"][b, :L], c["clean"][b, :L], rate)
            rel, ab = np.abs(out[b, rel_i] - want[rel_i]) / np.abs(want[rel_i]), np.abs(out[b, abs_i] - want[abs_i])
            ratio = np.abs(sl.six_terms(out[b]) - c["ref_f32"][b]) / c["f32_vs_f64"][b]
            print(f"{name}[{b}] L={L:<6d} {rel.max():10.3e} {ab.max():10.3e} {ratio.max():8.3f}")
    B, L, sr = 8, 4 * 24000, 24000
    clean = torch.from_numpy(tn.synth_noisy_speech(B, L, seed=5)).cuda()
    est = (0.9 * clean + 0.03 * torch.from_numpy(tn.normal(6, "w", B * L).reshape(B, L)).cuda()).contiguous()
    lib = _lib.lib()
    nbytes = lib.use_spec_losses_workspace(B, L, sr)
    work = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device="cuda")
    out = torch.empty((B, 15), dtype=torch.float64, device="cuda")
    lens = (C.c_int * B)(*([L] * B))
    stream = torch.cuda.current_stream().cuda_stream

    def device():
        assert lib.use_spec_losses(est.data_ptr(), clean.data_ptr(), lens, B, L, sr, work.data_ptr(), nbytes, out.data_ptr(), stream) == 0
        return out

    got, line = timed(device)
    print(f"use_spec_losses, {B} x {L} samples at {sr} Hz (workspace of {nbytes} bytes allocated once): {line}")
    _, line = timed(lambda: losses.spec_loss_terms(est, clean, None, sr))
    print(f"losses.spec_loss_terms, the same call with the workspace allocation of the Python wrapper: {line}")
    fb64 = torch.from_numpy(sl.mel_fbanks(sr)).cuda()
    t64, line = timed(lambda: torch_terms(est, clean, sr, torch.float64, fb64))
    print(f"the same arithmetic as torch.stft calls, float64: {line}")
    t32, line = timed(lambda: torch_terms(est, clean, sr, torch.float32, fb64.float()))
    print(f"the same arithmetic as torch.stft calls, float32 (as the reference runs it): {line}")
    d64 = ((got - t64).abs() / t64.abs()).max().item()
    d32 = ((got - t32.double()).abs() / t64.abs()).max().item()
    print(f"largest relative distance of the 8 x 15 device values to the float64 torch values {d64:.3e}, to the float32 ones {d32:.3e}")
    print("six terms of item 0:", {k: round(float(v[0]), 6) for k, v in losses._six(got).items()})


if __name__ == "__main__":
    main()
