"""Chunked against un-chunked sampling of one long synthetic recording (profiles/chunked_sampling.txt), bf16, the headline sampler
(N = 30, reverse diffusion + Langevin).  Run from the repository root on the GPU:

    python scripts/gpu_chunked_sampling.py time [seconds=60]      wall time per file (1 warm-up, 5 timed runs), workspace, plans
    python scripts/gpu_chunked_sampling.py time [seconds] chunked the same, without the un-chunked run
    python scripts/gpu_chunked_sampling.py once [seconds=60]      one chunked run, for rocprofv3 --kernel-trace --stats
    python scripts/gpu_chunked_sampling.py ladder T1 T2 ...       un-chunked, one run per padded frame count, rising; the first
                                                                  error code ends the run (nothing is retried)
"""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from universal_speech_enhancement_amd._lib import UseHipError
from universal_speech_enhancement_amd.sgmse.model_wrapper import ScoreModel
from universal_speech_enhancement_amd.testing import noise as tn
from universal_speech_enhancement_amd.testing import weights as tw

CHUNK = dict(chunk_frames=640, chunk_overlap=64, chunk_batch=8)
SAMPLER = dict(N=30, corrector_steps=1, snr=0.5, seed=1)


def model(sd):
    m = ScoreModel(backbone="ncsnpplarge", sde="ouve", t_eps=3e-2, condition="noisy", n_fft=1022, hop_length=160, num_frames=512,
                   window="hann", sde_input="noisy", predictor="reverse_diffusion", corrector="langevin", precision="bf16")
    m.score_net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m


def recording(samples):
    one = tn.synth_noisy_speech(1, 4 * 24000, seed=5)[0]                       # 4 s of synthetic speech, repeated
    return torch.from_numpy(np.tile(one, -(-samples // one.size))[:samples][None].copy()).cuda()


def run(m, wav, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = m.sample({"perturbed": wav}, **SAMPLER, **kw)["enhanced"]
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def report(tag, m, wav, times, out):
    eng = m.score_net.engine(512, wav.device)
    t = np.array(times)
    print(f"{tag}: {wav.shape[1] / 24000:.0f} s file, wall per file median {np.median(t):.3f} s (min {t.min():.3f}, max {t.max():.3f}, n={len(t)}), "
          f"workspace_bytes {eng.workspace_bytes()} ({eng.workspace_bytes() / 2**30:.2f} GiB), plans_built {eng.stat('plans_built')}, "
          f"graph_captures {eng.stat('graph_captures')}, finite {bool(torch.isfinite(out).all())}", flush=True)


def main():
    mode = sys.argv[1]
    sd = tw.make_state_dict(1234, **tw.LARGE)
    if mode == "ladder":
        m = model(sd)
        for Tp in (int(a) for a in sys.argv[2:]):
            wav = recording((Tp - 1) * 160)                                      # 1 + L // 160 = Tp frames: no padding
            try:
                dt, out = run(m, wav)
            except (UseHipError, RuntimeError) as e:
                print(f"ladder: T' = {Tp} ended with: {e}", flush=True)
                return
            report(f"ladder un-chunked T' = {Tp}", m, wav, [dt], out)
        return
    seconds = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    wav = recording(seconds * 24000)
    if mode == "once":
        m = model(sd)
        dt, out = run(m, wav, **CHUNK)
        report("chunked (one run, graph capture included)", m, wav, [dt], out)
        return
    mc, mu = model(sd), model(sd)
    run(mc, wav, **CHUNK)
    tc = [run(mc, wav, **CHUNK) for _ in range(5)]
    report("chunked 640 / 64 / 8", mc, wav, [t for t, _ in tc], tc[-1][1])
    if sys.argv[3:] == ["chunked"]:
        return
    run(mu, wav)
    tu = [run(mu, wav) for _ in range(5)]
    report("un-chunked", mu, wav, [t for t, _ in tu], tu[-1][1])
    a, b = tc[-1][1], tu[-1][1]
    print(f"chunked against un-chunked waveform (different noise realisations, random weights): rel. RMS difference "
          f"{float((a - b).norm() / b.norm()):.3f}", flush=True)


if __name__ == "__main__":
    main()
