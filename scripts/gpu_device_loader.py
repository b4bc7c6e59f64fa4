"""The device-side loader on the GPU (profiles/device_loader.txt).  Run from the repository root:

    python scripts/gpu_device_loader.py [--parent-lib build_ab/libuse_hip_parent.so] > profiles/device_loader.txt

Steps, each a child process under its own ``timeout``, chained (the first failure ends the run), at most 16 host threads:
  batches   per-batch time of the host loader against ``wavio.load_batch_device`` (decode and upload included), between
            ``torch.cuda.synchronize()`` calls, on the second of two passes; beside it the device time of the ``use_load_items_dev``
            call alone between HIP events.  Batches: 8 files of 4 s and of 10 s at 48 kHz and at 44.1 kHz, and one 60 s file.
  predict   whole ``predict`` runs (model start-up included), 16 files of 4 s at 48 kHz, N = 30, data.batch_size=8, dry-run weights:
            ``data.device_load`` off and on, alternating three times; the best of each and the share of the wall time spent in the loader.
  bench     ``bench.py --gpus 1`` on the parent commit's library (``--parent-lib``: a build of the parent's csrc, loaded through
            USE_HIP_LIB) and on this tree's, alternating; skipped without ``--parent-lib``.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.getcwd())
os.environ.setdefault("OMP_NUM_THREADS", "16")


def _write_files(folder, count, seconds, rate):
    import numpy as np
    from universal_speech_enhancement_amd import wavio
    from universal_speech_enhancement_amd.testing import noise as tn
    os.makedirs(folder, exist_ok=True)
    paths = []
    for i in range(count):
        x = tn.synth_noisy_speech(1, int(seconds * rate), seed=100 + i)[0].astype(np.float32)
        paths.append(os.path.join(folder, f"f{i:02d}.wav"))
        wavio.write_wav(paths[-1], x, rate)
    return paths


def step_batches():
    import numpy as np
    import torch
    from universal_speech_enhancement_amd import _lib, wavio
    from universal_speech_enhancement_amd.data import LoadWavData
    torch.set_num_threads(16)
    print("batch                     host loader   load_batch_device   ratio   use_load_items_dev alone (HIP events)   max |dev - host|")
    with tempfile.TemporaryDirectory() as tmp:
        for count, seconds, rate in [(8, 4, 48000), (8, 4, 44100), (8, 10, 48000), (8, 10, 44100), (1, 60, 48000)]:
            src = os.path.join(tmp, f"{count}x{seconds}s_{rate}")
            paths = _write_files(src, count, seconds, rate)
            host = LoadWavData(src, tmp, batch_size=count)
            dev = LoadWavData(src, tmp, batch_size=count, device_load=True)
            t = {}
            for name, data in (("host", host), ("dev", dev)):
                for _ in range(2):                                        # the second pass counts
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    batch = next(iter(data.predict_batches("cuda")))
                    torch.cuda.synchronize()
                    t[name] = time.perf_counter() - t0
                t[name + "_wav"] = batch["perturbed"]
            err = float((t["host_wav"] - t["dev_wav"]).abs().max())
            # the call alone: the doubles already on the device
            sigs = [torch.from_numpy(np.ascontiguousarray(wavio.read_wav(p)[0])).cuda() for p in paths]
            ns = [s.shape[0] for s in sigs]
            nums = [wavio.resampled_length(n, rate, 24000) for n in ns]
            L = _lib.lib()
            nbytes = max(L.use_resample_workspace(n, m) for n, m in zip(ns, nums))
            work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            wav = torch.empty(count, max(nums), dtype=torch.float32, device="cuda")
            ptrs = (C.c_void_p * count)(*[s.data_ptr() for s in sigs])
            args = (ptrs, (C.c_int64 * count)(*ns), (C.c_int64 * count)(*nums), count, 1, wav.data_ptr(), max(nums), work.data_ptr(), nbytes,
                    torch.cuda.current_stream().cuda_stream)
            ms = []
            for _ in range(6):
                a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                assert L.use_load_items_dev(*args) == 0, L.use_last_error()
                z.record()
                z.synchronize()
                ms.append(a.elapsed_time(z))
            assert torch.equal(wav, t["dev_wav"])
            print(f"{count} x {seconds:2d} s at {rate} Hz   {t['host'] * 1e3:9.1f} ms   {t['dev'] * 1e3:12.1f} ms   {t['host'] / t['dev']:6.1f}x"
                  f"   median {np.median(ms[1:]):8.3f} ms, min {min(ms[1:]):8.3f} ms over {len(ms) - 1} calls   {err:.3e}")


def step_predict_run(mode, src, dst):
    """One whole predict; prints a JSON line: the wall time of predict() and the time spent waiting for the loader's batches."""
    import torch
    from universal_speech_enhancement_amd import data as D, predict as P
    torch.set_num_threads(16)
    spent = [0.0]
    plain = D.LoadWavData.predict_batches

    def timed(self, *a, **kw):
        it = iter(plain(self, *a, **kw))
        while True:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            try:
                batch = next(it)
            except StopIteration:
                return
            torch.cuda.synchronize()
            spent[0] += time.perf_counter() - t0
            yield batch

    D.LoadWavData.predict_batches = timed
    t0 = time.perf_counter()
    n = P.predict(P.compose(["model=SGMSE_Large", f"data.data_folder={src}", f"data.target_folder={dst}", "random_init_seed=1",
                             "model.sampler_kwargs.N=30", "data.batch_size=8", f"data.device_load={'true' if mode == 'on' else 'false'}"]))
    torch.cuda.synchronize()
    print(json.dumps({"mode": mode, "files": n, "predict_s": time.perf_counter() - t0, "loader_s": spent[0]}))


def _child(args, seconds, env=None):
    r = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable] + args, stdout=subprocess.PIPE, text=True,
                       env=dict(os.environ, **(env or {})))
    if r.returncode != 0:
        sys.stdout.write(r.stdout)
        raise SystemExit(f"step {' '.join(args)} ended with status {r.returncode}: nothing more is started")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-steps", type=int, default=3)
    ap.add_argument("rest", nargs="*")
    a = ap.parse_args()
    me = os.path.abspath(__file__)
    if a.step == "batches":
        return step_batches()
    if a.step == "predict":
        return step_predict_run(*a.rest)
    sys.stdout.write(_child([me, "--step", "batches"], 420))
    sys.stdout.flush()
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "noisy")
        _write_files(src, 16, 4, 48000)
        runs = {"off": [], "on": []}
        for rep in range(3):
            for mode in ("off", "on"):
                out = _child([me, "--step", "predict", mode, src, os.path.join(tmp, f"out_{mode}_{rep}")], 300)
                runs[mode].append(json.loads(out.strip().splitlines()[-1]))
        print("\nwhole predict, 16 x 4 s at 48 kHz, N = 30, data.batch_size=8, dry-run weights (predict() wall time, loader = waiting for batches)")
        for mode in ("off", "on"):
            best = min(runs[mode], key=lambda r: r["predict_s"])
            print(f"data.device_load={mode:3s}: predict {[round(r['predict_s'], 2) for r in runs[mode]]} s, best {best['predict_s']:.2f} s; "
                  f"loader {best['loader_s']:.3f} s = {100 * best['loader_s'] / best['predict_s']:.1f} % of it")
        sys.stdout.flush()
    if a.parent_lib:
        print(f"\nbench.py --gpus 1 --steps {a.bench_steps} --warmup 1: the parent commit's library against this tree's, alternating")
        for rep in range(2):
            for name, env in (("parent", {"USE_HIP_LIB": os.path.abspath(a.parent_lib)}), ("this tree", {})):
                out = _child(["bench.py", "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", "1"], 420, env)
                line = json.loads(out.strip().splitlines()[-1])
                print(f"{name:9s}: {line['value']:.2f} {line['unit']}, {line['ms_per_step']:.2f} ms per step")
                sys.stdout.flush()


if __name__ == "__main__":
    main()
