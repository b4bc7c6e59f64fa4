"""The device-side store path on the GPU (profiles/device_store.txt).  Run from the repository root:

    python scripts/gpu_device_store.py > profiles/device_store.txt

One child process under its own ``timeout``, at most 16 host threads.  For each batch of model-rate (24 kHz) float32 rows on the device -
8 x 4 s restored to 48 kHz, 8 x 4 s restored to 44.1 kHz, one 60 s row restored to 48 kHz, 16-bit codes - it times
  device   ``wavio.store_batch_device``: the ``use_store_items_dev`` call, the one device-to-host copy and its synchronisation;
  host     what a restore without it costs: the batch copied to the host, then ``wavio.store_items_host`` (``use_resample_fft`` item by
           item on one host thread, the cast and the quantiser);
  kernels  the ``use_store_items_dev`` call alone between HIP events.
Wall clock between ``torch.cuda.synchronize()`` calls; every shape is warmed up first (two device calls, one host call); medians over
``--device-runs`` and ``--host-runs`` timed runs, the spread beside them.  The rows of the two paths are compared.
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

sys.path.insert(0, os.getcwd())
os.environ.setdefault("OMP_NUM_THREADS", "16")

BATCHES = [(8, 4, 48000), (8, 4, 44100), (1, 60, 48000)]


def step_batches(device_runs, host_runs):
    import numpy as np
    import torch
    from universal_speech_enhancement_amd import _lib, wavio
    from universal_speech_enhancement_amd.testing import noise as tn
    torch.set_num_threads(16)
    L = _lib.lib()
    print(f"box: {torch.cuda.get_device_name(0)}, HIP {torch.version.hip}, torch {torch.__version__}, {L.use_version().decode()}")
    print(f"medians over {device_runs} device runs and {host_runs} host runs after warm-up (min ... max beside them)\n")
    print("batch, 24 kHz ->          host restore                    store_batch_device              ratio   use_store_items_dev alone"
          " (HIP events)    codes that differ")
    for count, seconds, rate in BATCHES:
        n = seconds * 24000
        num = wavio.resampled_length(n, 24000, rate)
        x = np.stack([tn.synth_noisy_speech(1, n, seed=200 + i)[0] for i in range(count)]).astype(np.float32)
        x *= 0.8 / np.abs(x).max(axis=1, keepdims=True)
        wav = torch.from_numpy(x).cuda()
        lens, nums = [n] * count, [num] * count

        def host():
            return wavio.store_items_host(wav.cpu(), lens, nums, wavio.PCM16)

        def dev():
            return wavio.store_batch_device(wav, lens, nums, wavio.PCM16)

        t = {}
        for name, fn, warm, runs in (("dev", dev, 2, device_runs), ("host", host, 1, host_runs)):
            for _ in range(warm):
                rows = fn()
            ts = []
            for _ in range(runs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rows = fn()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            t[name], t[name + "_rows"] = np.array(ts) * 1e3, rows
        differ = int((t["dev_rows"] != t["host_rows"]).sum())
        # the call alone
        nbytes = L.use_store_workspace(n, num)
        work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        out = torch.empty(count, num, dtype=torch.int16, device="cuda")
        args = (wav.data_ptr(), n, (C.c_int * count)(*lens), (C.c_int64 * count)(*nums), count, wavio.PCM16, out.data_ptr(), num,
                work.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
        ms = []
        for _ in range(device_runs + 2):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            assert L.use_store_items_dev(*args) == 0, L.use_last_error()
            z.record()
            z.synchronize()
            ms.append(a.elapsed_time(z))
        ms = np.array(ms[2:])
        assert np.array_equal(out.cpu().numpy(), t["dev_rows"])
        h, d = t["host"], t["dev"]
        print(f"{count} x {seconds:2d} s -> {rate} Hz   {np.median(h):8.1f} ms ({h.min():7.1f} ... {h.max():7.1f})   "
              f"{np.median(d):8.2f} ms ({d.min():6.2f} ... {d.max():6.2f})   {np.median(h) / np.median(d):6.1f}x   "
              f"median {np.median(ms):7.3f} ms ({ms.min():7.3f} ... {ms.max():7.3f})   {differ} of {count * num}")
        sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None)
    ap.add_argument("--device-runs", type=int, default=10)
    ap.add_argument("--host-runs", type=int, default=3)
    a = ap.parse_args()
    if a.step == "batches":
        return step_batches(a.device_runs, a.host_runs)
    r = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--step", "batches", "--device-runs",
                        str(a.device_runs), "--host-runs", str(a.host_runs)])
    if r.returncode != 0:
        raise SystemExit(f"step batches ended with status {r.returncode}: nothing more is started")


if __name__ == "__main__":
    main()
