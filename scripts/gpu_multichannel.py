"""Loading and storing files of several channels on the GPU (profiles/multichannel.txt).  Run from the repository root:

    python scripts/gpu_multichannel.py > profiles/multichannel.txt

One child process under its own ``timeout``, at most 16 host threads.  A batch of 4 stereo files x 4 s at 48 kHz (16-bit), written to a
temporary folder; ``data.channels=all`` makes 8 rows of it.  It times
  load, device   ``wavio.load_batch_device(channels="all")``: the host decodes and uploads every interleaved file, ``use_load_files_dev``
                 de-interleaves, resamples to 24 kHz, applies the one gain per file, casts and collates;
  load, host     ``wavio.load_file_channels`` file by file (``use_resample_fft`` channel by channel on one host thread) and the copy of
                 the collated batch to the device;
  store, device  ``wavio.store_batch_device(channels=...)``: the 8 rows back to 48 kHz as interleaved 16-bit codes, one
                 ``use_store_files_dev`` call, one copy;
  store, host    the rows copied to the host, then ``wavio.store_files_host``;
  kernels        the ``use_load_files_dev`` and ``use_store_files_dev`` calls alone between HIP events.
Wall clock between ``torch.cuda.synchronize()`` calls; every path is warmed up first (two device calls, one host call); medians over
``--device-runs`` and ``--host-runs`` timed runs, the spread beside them.  Neither store path writes a file: the writer is the same host
code on both.  The rows and codes of the two paths are compared.
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

FILES, SECONDS, RATE, CHANNELS = 4, 4, 48000, 2


def step_batch(device_runs, host_runs):
    import numpy as np
    import torch
    from universal_speech_enhancement_amd import _lib, wavio
    from universal_speech_enhancement_amd.testing import noise as tn
    torch.set_num_threads(16)
    L = _lib.lib()
    print(f"box: {torch.cuda.get_device_name(0)}, HIP {torch.version.hip}, torch {torch.__version__}, {L.use_version().decode()}")
    print(f"medians over {device_runs} device runs and {host_runs} host runs after warm-up (min ... max beside them)\n")
    frames = SECONDS * RATE
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i in range(FILES):
            a = np.stack([tn.synth_noisy_speech(1, frames, sr=RATE, seed=300 + 2 * i + c)[0] * (0.8, 0.4)[c] for c in range(CHANNELS)], axis=1)
            paths.append(os.path.join(d, f"f{i}.wav"))
            wavio.write_wav(paths[-1], a.astype(np.float32), RATE)

        def load_host():
            files = [wavio.load_file_channels(p, 24000, True)[0] for p in paths]
            return torch.from_numpy(np.concatenate(files)).cuda()

        def load_dev():
            return wavio.load_batch_device(paths, 24000, True, "cuda", channels="all")[0]

        def timed(fn, warm, runs):
            for _ in range(warm):
                out = fn()
            ts = []
            for _ in range(runs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            return np.array(ts) * 1e3, out

        def line(what, h, dv):
            print(f"{what:6s} {np.median(h):8.1f} ms ({h.min():7.1f} ... {h.max():7.1f})   {np.median(dv):8.2f} ms ({dv.min():6.2f} ... {dv.max():6.2f})"
                  f"   {np.median(h) / np.median(dv):6.1f}x")

        print(f"{FILES} stereo files x {SECONDS} s at {RATE} Hz <-> 24 kHz        host                            device                        ratio")
        td, wav = timed(load_dev, 2, device_runs)
        th, ref = timed(load_host, 1, host_runs)
        line("load", th, td)
        err = float((wav - ref).abs().max())
        n = wav.shape[1]
        lens, nums, chans = [n] * FILES, [frames] * FILES, [CHANNELS] * FILES

        def store_host():
            return wavio.store_files_host(wav.cpu(), lens, nums, chans, wavio.PCM16)

        def store_dev():
            return wavio.store_batch_device(wav, lens, nums, wavio.PCM16, channels=chans)

        sd, codes = timed(store_dev, 2, device_runs)
        sh, want = timed(store_host, 1, host_runs)
        line("store", sh, sd)
        differ = sum(int((a != b).sum()) for a, b in zip(codes, want))
        print(f"\nloaded rows: max |device - host| = {err:.3e}; stored codes that differ: {differ} of {FILES * frames * CHANNELS}")
        # the two calls alone
        xs = [torch.from_numpy(np.ascontiguousarray(wavio.read_wav(p)[0]).reshape(-1)).cuda() for p in paths]
        nbytes = max(L.use_load_files_workspace(frames, n, CHANNELS), L.use_store_workspace(n, frames))
        work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        rows = torch.empty(FILES * CHANNELS, n, dtype=torch.float32, device="cuda")
        out = torch.empty(FILES * frames * CHANNELS, dtype=torch.int16, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        i64, ci = C.c_int64 * FILES, C.c_int * FILES
        calls = {"use_load_files_dev": lambda: L.use_load_files_dev((C.c_void_p * FILES)(*[x.data_ptr() for x in xs]), i64(*[frames] * FILES),
                                                                    i64(*lens), ci(*chans), FILES, 1, rows.data_ptr(), n, work.data_ptr(),
                                                                    nbytes, stream),
                 "use_store_files_dev": lambda: L.use_store_files_dev(rows.data_ptr(), n, ci(*lens), i64(*nums), ci(*chans),
                                                                      i64(*[f * frames * CHANNELS for f in range(FILES)]), FILES, wavio.PCM16,
                                                                      out.data_ptr(), work.data_ptr(), nbytes, stream)}
        for name, call in calls.items():
            ms = []
            for _ in range(device_runs + 2):
                a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                assert call() == 0, L.use_last_error()
                z.record()
                z.synchronize()
                ms.append(a.elapsed_time(z))
            ms = np.array(ms[2:])
            print(f"{name} alone (HIP events): median {np.median(ms):7.3f} ms ({ms.min():7.3f} ... {ms.max():7.3f})")
        assert torch.equal(rows, wav) and np.array_equal(out.cpu().numpy(), np.concatenate([c.reshape(-1) for c in codes]))
        sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None)
    ap.add_argument("--device-runs", type=int, default=10)
    ap.add_argument("--host-runs", type=int, default=3)
    a = ap.parse_args()
    if a.step == "batch":
        return step_batch(a.device_runs, a.host_runs)
    r = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--step", "batch", "--device-runs",
                        str(a.device_runs), "--host-runs", str(a.host_runs)])
    if r.returncode != 0:
        raise SystemExit(f"step batch ended with status {r.returncode}: nothing more is started")


if __name__ == "__main__":
    main()
