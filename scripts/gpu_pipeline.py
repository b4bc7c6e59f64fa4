"""What the one-run pipeline costs and saves, to record (no threshold).

    python scripts/gpu_pipeline.py handoff [--iters 200]
        ``use_wav_handoff`` (PCM_16, normalize: the default) between HIP events at [8, 96 000] samples (8 x 4 s) and at
        [1, 14 400 000] (ten minutes), in place, beside the bytes it moves: two reads and one write of the waveform.

    python scripts/gpu_pipeline.py wall [--files 16] [--seconds 4] [--N 30] [--batch-size 8] [--two-run-tree DIR] [--repeats 3]
        wall clock of ``predict model=USE`` (one process) against ``predict model=SGMSE_Large`` followed by ``predict model=LSGAN``
        over the first run's files (two processes), on the same folder of synthetic files, bf16, ``random_init_seed``; the
        commands alternate.  ``--two-run-tree``: a built checkout whose ``predict`` runs the two-run flow (the parent commit).
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SR = 24000


def handoff(args):
    import torch
    from universal_speech_enhancement_amd.handoff import wav_handoff
    for B, L in ((8, 96000), (1, 14400000)):
        wav = (torch.randn(B, L, device="cuda") * 0.1).contiguous()
        lens = [L] * B
        for _ in range(10):                                   # warm-up: code objects, the allocator's blocks
            wav_handoff(wav, lens, out=wav)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)]
        for a, b in ev:
            a.record()
            wav_handoff(wav, lens, out=wav)
            b.record()
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in ev)
        moved = 3 * B * L * 4
        med = ms[len(ms) // 2]
        print(json.dumps({"what": "use_wav_handoff PCM_16 normalize, in place, wrapper call between HIP events (lens kernel + 2 passes + 2 "
                                  "allocations of the wrapper)", "shape": [B, L], "iters": args.iters, "ms_median": med, "ms_min": ms[0],
                          "ms_p90": ms[int(len(ms) * 0.9)], "bytes_moved": moved, "GB_per_s_at_median": moved / med / 1e6}))


def wall(args):
    from universal_speech_enhancement_amd.testing import noise as tn
    from universal_speech_enhancement_amd.wavio import FLOAT32, write_wav
    two_tree = os.path.abspath(args.two_run_tree or ROOT)
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "noisy")
        os.makedirs(src)
        for i in range(args.files):
            write_wav(os.path.join(src, f"utt_{i:03d}.wav"), tn.synth_noisy_speech(1, int(args.seconds * SR), seed=100 + i)[0], SR, FLOAT32)
        common = ["random_init_seed=7", f"data.batch_size={args.batch_size}"]
        sampler = [f"model.sampler_kwargs.N={args.N}", "model.Score.precision=bf16"]
        exe = [sys.executable, "-m", "universal_speech_enhancement_amd.predict"]

        def run(tree, ov):
            subprocess.run(exe + ov, cwd=tree, check=True, stdout=subprocess.DEVNULL, timeout=300)

        rows = []
        for r in range(args.repeats):
            e, r2, r1 = (os.path.join(tmp, f"{d}_{r}") for d in ("enhanced", "two_runs", "one_run"))
            t0 = time.perf_counter()
            run(two_tree, ["model=SGMSE_Large", f"data.data_folder={src}", f"data.target_folder={e}"] + common + sampler)
            t1 = time.perf_counter()
            run(two_tree, ["model=LSGAN", f"data.data_folder={e}", f"data.target_folder={r2}", "model.G.precision=bf16"] + common)
            t2 = time.perf_counter()
            run(ROOT, ["model=USE", f"data.data_folder={src}", f"data.target_folder={r1}", "model.G.precision=bf16"] + common + sampler)
            t3 = time.perf_counter()
            same = all(open(os.path.join(r1, n), "rb").read() == open(os.path.join(r2, n), "rb").read() for n in sorted(os.listdir(src)))
            rows.append({"repeat": r, "two_runs_s": t2 - t0, "of_which_sampler_run_s": t1 - t0, "of_which_refine_run_s": t2 - t1,
                         "one_run_s": t3 - t2, "refined_files_identical": same})
            print(json.dumps(rows[-1]), flush=True)
        best2, best1 = min(x["two_runs_s"] for x in rows), min(x["one_run_s"] for x in rows)
        print(json.dumps({"files": args.files, "seconds_each": args.seconds, "N": args.N, "batch_size": args.batch_size, "precision": "bf16",
                          "two_run_tree": two_tree, "two_runs_s_best": best2, "one_run_s_best": best1, "saved_s": best2 - best1}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["handoff", "wall"])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--N", type=int, default=30)
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--two-run-tree", default=None)
    args = ap.parse_args()
    (handoff if args.mode == "handoff" else wall)(args)


if __name__ == "__main__":
    main()
