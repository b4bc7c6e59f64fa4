"""What the gain of ``data.restore_level`` costs on the GPU (profiles/restore_level.txt).  Run from the repository root:

    python scripts/gpu_restore_level.py > profiles/restore_level.txt

One child process under its own ``timeout``, at most 16 host threads.
  store   for each batch of model-rate (24 kHz) float32 rows on the device - 8 x 4 s restored to 48 kHz, 8 x 4 s at 24 kHz (``num == len``:
          the pass-through becomes widen - multiply - narrow), one 60 s row restored to 48 kHz, 16-bit codes - the store call alone
          between HIP events, alternating in one process between ``use_store_items_dev_gain`` with gains and ``use_store_items_dev``
          (the instantiation without a gain) with the same arguments: ``--runs`` pairs after warm-up.
  load    ``wavio.load_batch_device`` of 8 x 4 s files at 48 kHz with and without ``return_peaks`` (the one small device-to-host copy),
          wall clock from the call to a ``torch.cuda.synchronize()``, alternating as well.
Medians, and the spread (min ... max) beside them.
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.getcwd())
os.environ.setdefault("OMP_NUM_THREADS", "16")

BATCHES = [(8, 4, 48000), (8, 4, 24000), (1, 60, 48000)]


def step_measure(runs):
    import numpy as np
    import torch
    from universal_speech_enhancement_amd import _lib, wavio
    from universal_speech_enhancement_amd.testing import noise as tn
    torch.set_num_threads(16)
    L = _lib.lib()
    print(f"box: {torch.cuda.get_device_name(0)}, HIP {torch.version.hip}, torch {torch.__version__}, {L.use_version().decode()}")
    print(f"{runs} alternating pairs after 3 warm-up pairs: median ms (min ... max)\n")
    print("batch, 24 kHz ->          use_store_items_dev (no gain)          use_store_items_dev_gain               difference of the medians")
    for count, seconds, rate in BATCHES:
        n = seconds * 24000
        num = wavio.resampled_length(n, 24000, rate)
        x = np.stack([tn.synth_noisy_speech(1, n, seed=200 + i)[0] for i in range(count)]).astype(np.float32)
        x *= 0.8 / np.abs(x).max(axis=1, keepdims=True)
        wav = torch.from_numpy(x).cuda()
        lens, nums = [n] * count, [num] * count
        gains = (C.c_double * count)(*[0.05 + 0.1 * i for i in range(count)])
        nbytes = L.use_store_workspace(n, num)
        work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        out = torch.empty(count, num, dtype=torch.int16, device="cuda")
        head = (wav.data_ptr(), n, (C.c_int * count)(*lens), (C.c_int64 * count)(*nums))
        tail = (count, wavio.PCM16, out.data_ptr(), num, work.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)

        def timed(fn):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            assert fn() == 0, L.use_last_error()
            z.record()
            z.synchronize()
            return a.elapsed_time(z)

        t = {"old": [], "gain": []}
        for i in range(runs + 3):
            for name, fn in (("gain", lambda: L.use_store_items_dev_gain(*head, gains, *tail)), ("old", lambda: L.use_store_items_dev(*head, *tail))):
                ms = timed(fn)
                if i >= 3:
                    t[name].append(ms)
        o, g = np.array(t["old"]), np.array(t["gain"])
        print(f"{count} x {seconds:2d} s -> {rate} Hz   {np.median(o):8.4f} ms ({o.min():7.4f} ... {o.max():7.4f})   "
              f"{np.median(g):8.4f} ms ({g.min():7.4f} ... {g.max():7.4f})   {np.median(g) - np.median(o):+8.4f} ms")
        sys.stdout.flush()
    # the loader with and without the peak read-back
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i in range(8):
            w = tn.synth_noisy_speech(1, 4 * 48000, seed=300 + i)[0].astype(np.float32)
            paths.append(os.path.join(d, f"f{i}.wav"))
            wavio.write_wav(paths[-1], w / np.abs(w).max() * np.float32(0.1 * (i + 1)), 48000)
        t = {False: [], True: []}
        for i in range(runs + 3):
            for peaks in (True, False):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                wavio.load_batch_device(paths, 24000, True, "cuda", return_peaks=peaks)
                torch.cuda.synchronize()
                if i >= 3:
                    t[peaks].append((time.perf_counter() - t0) * 1e3)
        o, g = np.array(t[False]), np.array(t[True])
        print("\nload_batch_device, 8 x 4 s at 48 kHz -> 24 kHz (decode, upload, use_load_items_dev[_peak], synchronise)")
        print(f"without peaks   {np.median(o):8.3f} ms ({o.min():7.3f} ... {o.max():7.3f})")
        print(f"with peaks      {np.median(g):8.3f} ms ({g.min():7.3f} ... {g.max():7.3f})   {np.median(g) - np.median(o):+8.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None)
    ap.add_argument("--runs", type=int, default=10)
    a = ap.parse_args()
    if a.step == "measure":
        return step_measure(a.runs)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--step", "measure", "--runs", str(a.runs)])
    if r.returncode != 0:
        raise SystemExit(f"step measure ended with status {r.returncode}: nothing more is started")


if __name__ == "__main__":
    main()
