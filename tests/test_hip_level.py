"""GPU checks of ``data.restore_level`` (csrc/use_resample.hip: ``use_store_items_dev_gain`` / ``use_store_files_dev_gain`` /
``use_load_items_dev_peak`` / ``use_load_files_dev_peak``; ``wavio.store_batch_device(gains=)`` / ``load_batch_device(return_peaks=)``;
``predict data.restore_level=true``).

The rules are stated in tests/level_ref.py and tests/store_ref.py: a FLOAT32 row with a gain is ``float32(v * g)`` - bit for bit at an
unchanged length, ``store_ref.check_float32`` against the scipy oracle times g where resampled; a PCM16 row is the writer's code of the
call's own FLOAT32 row; a null gain is the old entry point, bit for bit.  A peak is the very value the scale kernel divides by: bit-equal
to the host loader's at an unchanged rate, within the resampler's ``D = 1e-11 * max(1, max|want|)`` of the scipy oracle's peak otherwise.
Every figure is printed before it is asserted (``pytest -s``)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import level_ref as lv
import store_ref as sr
from universal_speech_enhancement_amd import _lib, wavio

pytestmark = pytest.mark.gpu

DTYPES = {wavio.PCM16: torch.int16, wavio.FLOAT32: torch.float32}
POISON = 77


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _collate(rows, stride, pad):
    wav = np.full((len(rows), stride), pad, np.float32)
    for b, r in enumerate(rows):
        wav[b, : len(r)] = r
    return torch.from_numpy(wav).cuda()


def _store(rows, nums, gains, subtype, stride=None, out_stride=None, pad=np.nan, old=False, expect=0):
    """``use_store_items_dev_gain`` (``old``: ``use_store_items_dev``) on the float32 signals ``rows`` collated at ``stride`` (the padding
    filled with ``pad``) -> host ``[B, out_stride]``; ``out`` is poisoned before the call.  ``gains`` None: a null pointer."""
    L = _lib.lib()
    B, lens = len(rows), [len(r) for r in rows]
    stride, out_stride = stride or max(lens), out_stride or max(nums)
    wav = _collate(rows, stride, pad)
    out = torch.full((B, out_stride), POISON, dtype=DTYPES[subtype], device="cuda")
    need = max(L.use_store_workspace(n, num) for n, num in zip(lens, nums))
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    head = (wav.data_ptr(), stride, (C.c_int * B)(*lens), (C.c_int64 * B)(*nums))
    tail = (B, subtype, out.data_ptr(), out_stride, work.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    if old:
        rc = L.use_store_items_dev(*head, *tail)
    else:
        rc = L.use_store_items_dev_gain(*head, None if gains is None else (C.c_double * B)(*gains), *tail)
    assert rc == expect, (rc, L.use_last_error())
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def alone():
    """(len, num, g) -> (input, FLOAT32 row, PCM16 row): every shape and gain as a batch of one at stride = len, out_stride = num;
    computed once and left unchanged."""
    out = {}
    for n, num in lv.SHAPES:
        x = sr.signal(n, num)
        for g in lv.GAINS:
            out[(n, num, g)] = (x, _store([x], [num], [g], wavio.FLOAT32)[0], _store([x], [num], [g], wavio.PCM16)[0])
    return out


@pytest.mark.parametrize("n,num", lv.SHAPES)
def test_a_row_with_a_gain_is_the_product_rounded_once(alone, n, num):
    for g in lv.GAINS:
        x, f, q = alone[(n, num, g)]
        assert f.shape == q.shape == (num,) and np.isfinite(f).all()
        lv.check_row(f, x, num, g, f"device {n} -> {num}, g = {g}")
        assert np.array_equal(q, sr.quantise(f)), g                                                # the quantiser, exactly
        host = wavio.store_items_host(torch.from_numpy(x)[None], [n], [num], wavio.FLOAT32, gains=[g])[0]
        print(f"device {n} -> {num}, g = {g}: {int((host.view(np.uint32) != f.view(np.uint32)).sum())} samples differ from store_items_host")
    assert not alone[(n, num, 0.0)][1].any() and not alone[(n, num, 0.0)][2].any()
    if n >= 255:                                                                                   # the clamp is exercised, not assumed
        q = alone[(n, num, 3.0)][2].astype(np.int32)
        print(f"{n} -> {num}: {(q == 32767).sum()} codes at +32767 and {(q == -32768).sum()} at -32768 of {num} at g = 3")
        assert (q == 32767).sum() > 0 and (q == -32768).sum() > 0
        f = alone[(n, num, 3.0)][1]
        assert f.max() > 1 and f.min() < -1                                                        # FLOAT keeps what lies above full scale


@pytest.mark.parametrize("n,num", lv.SHAPES)
def test_the_padding_is_never_read_and_the_tail_is_zero(alone, n, num):
    for g in (0.4625, 3.0):
        x, f, q = alone[(n, num, g)]
        for subtype, ref in ((wavio.FLOAT32, f), (wavio.PCM16, q)):
            got = _store([x], [num], [g], subtype, stride=n + 301, out_stride=num + 259)           # NaN from len to stride
            assert np.array_equal(_bits(got[0, :num]), _bits(ref)) and np.isfinite(got[0].astype(np.float64)).all(), (subtype, g)
            assert not got[0, num:].any() and not np.signbit(got[0, num:]).any(), (subtype, g)     # exact zeros up to out_stride


def test_an_item_does_not_depend_on_its_batch(alone):
    items = [(2400, 4410, 0.4625), (4097, 4097, 3.0), (2401, 801, 1.0), (256, 512, 0.0)]
    rows, nums, gains = [alone[k][0] for k in items], [k[1] for k in items], [k[2] for k in items]
    for subtype, j in ((wavio.FLOAT32, 1), (wavio.PCM16, 2)):
        a = _store(rows, nums, gains, subtype)
        b = _store(rows, nums, gains, subtype)
        assert np.array_equal(_bits(a), _bits(b))                                                  # two runs agree
        c = _store(rows[::-1], nums[::-1], gains[::-1], subtype, stride=5000, out_stride=4999, pad=3.0)[::-1]
        for i, k in enumerate(items):
            ref = alone[k][j]
            assert np.array_equal(_bits(a[i, : k[1]]), _bits(ref)), (subtype, k)
            assert np.array_equal(_bits(c[i, : k[1]]), _bits(ref)), (subtype, k)
            assert not a[i, k[1]:].any() and not c[i, k[1]:].any()


def test_a_null_gain_is_the_old_entry_point():
    nan = np.array([0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800001, 0xFF923456], np.uint32).view(np.float32)   # payloads, quiet and signalling
    special = np.concatenate([nan, np.array([0.0, -0.0, 1.0, -1.5, 1e9, np.inf, -np.inf, 1e-30, 1e-45, 0.3, 32766.5 / 32767], np.float32)])
    rows = [special, np.concatenate([sr.signal(4097, 4097), special]), sr.signal(2400, 4410), sr.signal(4096, 8192)]
    nums = [len(rows[0]), len(rows[1]), 4410, 8192]
    for subtype in (wavio.FLOAT32, wavio.PCM16):
        old = _store(rows, nums, None, subtype, stride=4200, out_stride=8200, old=True)
        new = _store(rows, nums, None, subtype, stride=4200, out_stride=8200)
        assert np.array_equal(_bits(old), _bits(new)), subtype
        if subtype == wavio.FLOAT32:
            kept = old[0, : len(special)].view(np.uint32)[:5]
            print("NaN bit patterns through the pass-through:", [hex(v) for v in kept])
            assert np.array_equal(old[0, : len(special)].view(np.uint32), special.view(np.uint32))  # the input's bits, the payloads too
        one = _store(rows, nums, [1.0] * 4, subtype, stride=4200, out_stride=8200)                  # g = 1 multiplies: finite values agree
        finite = np.isfinite(old.astype(np.float64))
        assert np.array_equal(old[finite], one[finite])


def test_bad_gains_are_refused_and_out_stays_untouched():
    L = _lib.lib()
    rows, nums = [sr.signal(300, 300), sr.signal(300, 450)], [300, 450]
    for bad in (float("nan"), float("inf"), -1.0, -float("inf")):
        for subtype in (wavio.FLOAT32, wavio.PCM16):
            out = _store(rows, nums, [1.0, bad], subtype, expect=-1)
            msg = L.use_last_error()
            print(bad, msg)
            assert b"gain_host[1]" in msg and (out == POISON).all(), (bad, subtype, msg)
    assert not (_store(rows, nums, [1.0, 0.0], wavio.PCM16) == POISON).any()                        # zero is a gain


# ---- files of several channels ----
def _store_files(rows, lens, nums, chans, gains, subtype, stride, old=False, expect=0):
    """``use_store_files_dev_gain`` (``old``: ``use_store_files_dev``) -> the files ``[num, ch]``, from one poisoned buffer with a gap of
    five elements after every file; the gaps must stay poisoned."""
    L = _lib.lib()
    F = len(chans)
    wav = _collate(rows, stride, np.nan)
    offs, total = [], 0
    for num, c in zip(nums, chans):
        offs.append(total)
        total += num * c + 5
    out = torch.full((total,), POISON, dtype=DTYPES[subtype], device="cuda")
    need = max(L.use_store_workspace(n, num) for n, num in zip(lens, nums))
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    head = (wav.data_ptr(), stride, (C.c_int * F)(*lens), (C.c_int64 * F)(*nums), (C.c_int * F)(*chans), (C.c_int64 * F)(*offs))
    tail = (F, subtype, out.data_ptr(), work.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    if old:
        rc = L.use_store_files_dev(*head, *tail)
    else:
        rc = L.use_store_files_dev_gain(*head, None if gains is None else (C.c_double * F)(*gains), *tail)
    assert rc == expect, (rc, L.use_last_error())
    flat = out.cpu().numpy()
    for o, num, c in zip(offs, nums, chans):
        assert (flat[o + num * c: o + num * c + 5] == POISON).all()
    return [flat[o: o + num * c].reshape(num, c) for o, num, c in zip(offs, nums, chans)]


@pytest.mark.parametrize("subtype", [wavio.FLOAT32, wavio.PCM16])
@pytest.mark.parametrize("n,num", [(257, 257), (4097, 4097), (2400, 4410), (256, 512)])
def test_store_files_dev_gain_gives_every_channel_the_files_gain(n, num, subtype):
    chans, gains = [1, 2, 3], [0.4625, 3.0, 0.125]
    rows = [sr.signal(n, num + k) for k in range(6)]
    per_row = [g for g, c in zip(gains, chans) for _ in range(c)]
    files = _store_files(rows, [n] * 3, [num] * 3, chans, gains, subtype, stride=n + 7)
    items = _store(rows, [num] * 6, per_row, subtype, stride=n + 7)
    row = 0
    for f, c in enumerate(chans):
        assert files[f].shape == (num, c)
        for k in range(c):                                                                         # ch = 1 included: the items call, bitwise
            assert np.array_equal(_bits(files[f][:, k]), _bits(items[row + k])), (f, k)
            if subtype == wavio.FLOAT32:
                lv.check_row(np.ascontiguousarray(files[f][:, k]), rows[row + k], num, gains[f], f"file {f} channel {k}, {n} -> {num}")
        row += c
    old = _store_files(rows, [n] * 3, [num] * 3, chans, None, subtype, stride=n + 7, old=True)     # the layout, and the null gain
    new = _store_files(rows, [n] * 3, [num] * 3, chans, None, subtype, stride=n + 7)
    one = _store_files(rows, [n] * 3, [num] * 3, chans, [1.0] * 3, subtype, stride=n + 7)
    for f in range(3):
        assert np.array_equal(_bits(old[f]), _bits(new[f])) and np.array_equal(old[f], one[f]), f
    for bad in (float("nan"), float("inf"), -1.0):
        got = _store_files(rows, [n] * 3, [num] * 3, chans, [1.0, 1.0, bad], subtype, stride=n + 7, expect=-1)
        assert b"gain_host[2]" in _lib.lib().use_last_error() and all((g == POISON).all() for g in got)


# ---- the peaks ----
def _load_items(signals, nums, normalize=True, peaks=True, stride=None):
    """``use_load_items_dev_peak`` (``peaks`` False: a null pointer) -> (rows, peaks); ``wav`` and ``peak_dev`` poisoned before the call."""
    L = _lib.lib()
    B = len(signals)
    stride = stride or max(nums)
    xs = [torch.from_numpy(np.ascontiguousarray(s, dtype=np.float64)).cuda() for s in signals]
    wav = torch.full((B, stride), float(POISON), dtype=torch.float32, device="cuda")
    pk = torch.full((B,), float(POISON), dtype=torch.float64, device="cuda")
    need = max(L.use_resample_workspace(len(s), num) for s, num in zip(signals, nums))
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc = L.use_load_items_dev_peak((C.c_void_p * B)(*[x.data_ptr() for x in xs]), (C.c_int64 * B)(*[len(s) for s in signals]),
                                   (C.c_int64 * B)(*nums), B, int(normalize), wav.data_ptr(), stride, work.data_ptr(), need,
                                   pk.data_ptr() if peaks else None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.use_last_error()
    return wav.cpu().numpy(), pk.cpu().numpy()


def _load_files(files, nums, normalize=True, peaks=True, stride=None):
    """``use_load_files_dev_peak`` on decoded files ``[n, C]`` -> (rows, peaks per file)."""
    L = _lib.lib()
    F = len(files)
    ns, chs = [f.shape[0] for f in files], [f.shape[1] for f in files]
    stride = stride or max(nums)
    xs = [torch.from_numpy(np.ascontiguousarray(f, dtype=np.float64).reshape(-1)).cuda() for f in files]
    wav = torch.full((sum(chs), stride), float(POISON), dtype=torch.float32, device="cuda")
    pk = torch.full((F,), float(POISON), dtype=torch.float64, device="cuda")
    need = max(L.use_load_files_workspace(n, num, c) for n, num, c in zip(ns, nums, chs))
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc = L.use_load_files_dev_peak((C.c_void_p * F)(*[x.data_ptr() for x in xs]), (C.c_int64 * F)(*ns), (C.c_int64 * F)(*nums),
                                   (C.c_int * F)(*chs), F, int(normalize), wav.data_ptr(), stride, work.data_ptr(), need,
                                   pk.data_ptr() if peaks else None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.use_last_error()
    return wav.cpu().numpy(), pk.cpu().numpy()


def _peaked(n, at, seed):
    """Noise below 0.3 with the maximum, -0.7, at index ``at`` and a NaN beside the middle."""
    x = np.clip(np.random.default_rng(seed).standard_normal(n) * 0.1, -0.3, 0.3)
    x[at] = -0.7
    return x


@pytest.mark.parametrize("n", [4095, 4096, 4097, 8193])
def test_the_peak_is_found_at_the_seams_of_the_slices(n):
    """The maximum at the first and last sample of a slice of 4096, the places a reduction over partial maxima gets wrong; all four
    placements of a length are the items of one call."""
    places = sorted({p for p in (0, 4095, 4096, n - 1) if p < n})
    sigs = [_peaked(n, p, 100 * n + p) for p in places]
    rows, pk = _load_items(sigs, [n] * len(sigs), stride=n + 5)
    plain, untouched = _load_items(sigs, [n] * len(sigs), peaks=False, stride=n + 5)
    print(f"n = {n}: peaks {pk.tolist()} for the maximum at {places}")
    assert (pk == 0.7).all() and (untouched == POISON).all()
    assert np.array_equal(_bits(rows), _bits(plain))                                               # the rows do not depend on the pointer
    for b, s in enumerate(sigs):                                                                   # the host loader's bits at an unchanged rate
        assert np.array_equal(rows[b, :n].view(np.uint32), (s / np.float64(0.7) * 0.8).astype(np.float32).view(np.uint32)), places[b]
    raw, poisoned = _load_items(sigs, [n] * len(sigs), normalize=False, stride=n + 5)
    assert (poisoned == POISON).all() and np.array_equal(raw[0, :n], sigs[0].astype(np.float32))   # normalize = 0: nothing is written
    with_nan = [s.copy() for s in sigs]
    for s in with_nan:
        s[n // 2 + 1] = np.nan
    assert (_load_items(with_nan, [n] * len(sigs))[1] == 0.7).all()                                # a NaN is never the peak
    # files: the maximum in a channel other than the first, at the same places of the ch * n values' slices
    files = [np.stack([_peaked(n, 7, 5 * n + p) * 0.5, _peaked(n, p, 7 * n + p), _peaked(n, 9, 9 * n + p) * 0.25], axis=1) for p in places]
    frows, fpk = _load_files(files, [n] * len(files), stride=n + 5)
    fplain, funtouched = _load_files(files, [n] * len(files), peaks=False, stride=n + 5)
    print(f"n = {n}: file peaks {fpk.tolist()}")
    assert (fpk == 0.7).all() and (funtouched == POISON).all() and np.array_equal(_bits(frows), _bits(fplain))
    assert (_load_files(files, [n] * len(files), normalize=False)[1] == POISON).all()
    mono, mpk = _load_files([s[:, None] for s in sigs], [n] * len(sigs), stride=n + 5)             # one channel: the items call
    assert np.array_equal(_bits(mono), _bits(rows)) and np.array_equal(mpk, pk)


@pytest.mark.parametrize("n,num", [(8193, 4097), (4410, 2400), (2048, 4096)])
def test_a_resampled_peak_is_the_oracles_within_the_resamplers_bound(n, num):
    from scipy.signal import resample
    x = np.random.default_rng(n + num).standard_normal(n) * 0.2
    want = resample(x, num)
    D = 1e-11 * max(1.0, float(np.abs(want).max()))
    rows, pk = _load_items([x], [num])
    host = np.abs(wavio.resample_fft(x, num)).max()
    print(f"{n} -> {num}: peak {pk[0]!r}, oracle {np.abs(want).max()!r}, host {host!r}, D = {D:.3e}")
    assert abs(pk[0] - np.abs(want).max()) <= D
    assert np.array_equal(_bits(rows), _bits(_load_items([x], [num], peaks=False)[0]))
    stereo = np.stack([x * 0.3, x], axis=1)
    frows, fpk = _load_files([stereo], [num])
    assert abs(fpk[0] - np.abs(want).max()) <= D and np.array_equal(_bits(frows), _bits(_load_files([stereo], [num], peaks=False)[0]))
    # the peak is the divisor: the rows are v / peak * 0.8 of values within D of the oracle's
    np.testing.assert_allclose(rows[0, :num], want / pk[0] * 0.8, rtol=0, atol=1e-7)


# ---- wavio ----
def _speech(n, seed, level):
    """A smooth signal with its peak at exactly float32(level)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 24000.0
    w = sum(rng.standard_normal() * np.sin(2 * np.pi * f * t + rng.uniform(0, 6)) for f in (110.0, 220.0, 450.0, 1300.0, 3100.0))
    w = w * (0.3 + 0.7 * np.sin(2 * np.pi * 3.0 * t) ** 2)
    return (w / np.abs(w).max() * level).astype(np.float32)


SOURCES = {"a24.wav": (24000, 6500, 0.1), "b48.wav": (48000, 14400, 0.5), "c44.wav": (44100, 11025, 0.9)}


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """Three short files at 24, 48 and 44.1 kHz with peaks 0.1, 0.5 and 0.9 (float files: the peaks are exact), and clean companions."""
    root = tmp_path_factory.mktemp("level")
    (root / "noisy").mkdir()
    (root / "clean").mkdir()
    for i, (name, (rate, frames, level)) in enumerate(SOURCES.items()):
        w = _speech(frames, 40 + i, level)
        wavio.write_wav(str(root / "noisy" / name), w, rate, wavio.FLOAT32)
        wavio.write_wav(str(root / "clean" / name), (w * np.float32(0.9)).astype(np.float32), rate, wavio.FLOAT32)
    return root


def test_load_batch_device_returns_the_peaks(folder):
    paths = [str(folder / "noisy" / name) for name in SOURCES]
    host = [wavio.load_utterance(p, 24000, True, return_peak=True) for p in paths]
    wav, lens, rates, peaks = wavio.load_batch_device(paths, 24000, True, "cuda", return_peaks=True)
    plain = wavio.load_batch_device(paths, 24000, True, "cuda")
    assert len(plain) == 3 and torch.equal(wav, plain[0]) and peaks.dtype == np.float64 and peaks.shape == (3,)
    print("device peaks", peaks.tolist(), "host peaks", [float(h[2]) for h in host])
    assert peaks[0] == host[0][2] == np.float64(np.float32(0.1))                                   # an unchanged rate: bit-equal
    for b in (1, 2):
        assert abs(peaks[b] - host[b][2]) <= 2e-11                                                 # D of the resampler, twice (both sides)
    mixed = wavio.load_batch_device(paths, 24000, True, "cuda", max_samples=12000, return_peaks=True)   # b48 takes the host path
    assert mixed[3][1] == host[1][2] and mixed[3][0] == peaks[0] and mixed[3][2] == peaks[2]
    assert wavio.load_batch_device(paths, 24000, False, "cuda", return_peaks=True)[3] is None
    # channels="all": one peak per file
    stereo = str(folder / "stereo.wav")
    wavio.write_wav(stereo, np.stack([_speech(9600, 50, 0.05), _speech(9600, 51, 0.4)], axis=1), 48000, wavio.FLOAT32)
    out = wavio.load_batch_device([paths[0], stereo], 24000, True, "cuda", channels="all", return_peaks=True)
    ref = wavio.load_file_channels(stereo, 24000, True, return_peak=True)
    assert len(out) == 5 and out[3] == [1, 2] and out[4].shape == (2,) and out[4][0] == peaks[0] and abs(out[4][1] - ref[2]) <= 2e-11
    assert torch.equal(out[0], wavio.load_batch_device([paths[0], stereo], 24000, True, "cuda", channels="all")[0])
    host_file = wavio.load_batch_device([paths[0], stereo], 24000, True, "cuda", channels="all", max_samples=10000, return_peaks=True)
    assert host_file[4][1] == ref[2]                                                               # 9600 x 2 > 10000: the host's peak


def test_store_batch_device_with_gains(alone):
    items = [(2400, 4410, 0.4625), (4097, 4097, 3.0), (2401, 801, 1.0), (256, 512, 0.0)]
    rows, lens, nums, gains = [alone[k][0] for k in items], [k[0] for k in items], [k[1] for k in items], [k[2] for k in items]
    wav = torch.full((4, 4100), float("nan"))
    for b, r in enumerate(rows):
        wav[b, : len(r)] = torch.from_numpy(r)
    dev = wav.cuda()
    for subtype, j in ((wavio.FLOAT32, 1), (wavio.PCM16, 2)):
        got = wavio.store_batch_device(dev, lens, nums, subtype, gains=torch.tensor(gains, dtype=torch.float64))
        for b, k in enumerate(items):
            assert np.array_equal(_bits(got[b, : k[1]]), _bits(alone[k][j])) and not got[b, k[1]:].any(), (subtype, k)
        mixed = wavio.store_batch_device(dev, lens, nums, subtype, max_samples=4200, gains=gains)   # row 0 takes the host path
        host = wavio.store_items_host(wav, lens, nums, subtype, gains=gains)
        for b in range(4):
            assert np.array_equal(_bits(mixed[b]), _bits((host if b == 0 else got)[b])), (subtype, b)
        files = wavio.store_batch_device(dev[:2], lens[:2], nums[:2], subtype, channels=[1, 1], gains=gains[:2])
        assert np.array_equal(_bits(files[0][:, 0]), _bits(alone[items[0]][j])) and np.array_equal(_bits(files[1][:, 0]), _bits(alone[items[1]][j]))
    with pytest.raises(ValueError):
        wavio.store_batch_device(dev, lens, nums, wavio.PCM16, gains=[1.0, float("nan"), 1.0, 1.0])
    with pytest.raises(ValueError):
        wavio.store_batch_device(dev, lens, nums, wavio.PCM16, gains=[1.0, 1.0])


# ---- predict ----
def _spy(monkeypatch, cls, seen):
    plain_step = cls.predict_step

    def spy(self, batch, batch_idx=0):
        out = plain_step(self, batch, batch_idx)
        seen.append({k: (v.detach().cpu().clone() if isinstance(v, torch.Tensor) else v) for k, v in out.items()})
        return out

    monkeypatch.setattr(cls, "predict_step", spy)


def _check_file(path, row, n, frames, rate, g, subtype, what):
    """A written file against ``store_items_host(gains=)`` of its batch row: bitwise at ``num == len``, the midpoint rule where resampled."""
    assert wavio.wav_info(str(path)) == (frames, 1, rate), what
    raw = path.read_bytes()[44:]
    code = wavio.PCM16 if subtype == "PCM_16" else wavio.FLOAT32
    got = np.frombuffer(raw, np.int16 if subtype == "PCM_16" else np.float32)
    host = wavio.store_items_host(row[None, :n], [n], [frames], code, gains=[g])[0]
    print(f"{what}: {int((host != got).sum())} of {frames} samples differ from store_items_host, gain {g!r}")
    if frames == n:
        assert np.array_equal(_bits(got), _bits(host)), what
    else:
        want64 = lv.want64(row[:n].numpy(), frames, g)
        (sr.check_codes if subtype == "PCM_16" else sr.check_float32)(got, want64, what)


@pytest.mark.parametrize("restore_rate", [False, True])
@pytest.mark.parametrize("device_load,subtype", [(False, "PCM_16"), (False, "FLOAT"), (True, "PCM_16"), (True, "FLOAT")])
def test_predict_with_restore_level_writes_every_file_at_its_sources_level(folder, tmp_path, monkeypatch, restore_rate, device_load, subtype):
    """The three sources of ``folder`` in two batches, dry-run weights, ``data.clean_folder`` set; with and without the flag at equal
    other options."""
    from universal_speech_enhancement_amd import predict as P
    from universal_speech_enhancement_amd.SGMSE_module import SGMSEModule
    seen = []
    _spy(monkeypatch, SGMSEModule, seen)
    common = ["model=SGMSE_Large", f"data.data_folder={folder / 'noisy'}", f"data.clean_folder={folder / 'clean'}", "random_init_seed=1",
              "model.sampler_kwargs.N=1", "data.batch_size=2", "data.convergence_losses=true", f"model.wav_subtype={subtype}",
              f"data.device_load={'true' if device_load else 'false'}", f"data.restore_rate={'true' if restore_rate else 'false'}"]
    off, on = tmp_path / "off", tmp_path / "on"
    assert P.predict(P.compose(common + [f"data.target_folder={off}"])) == 3
    assert all("source_gain" not in b for b in seen)
    plain = list(seen)
    seen.clear()
    assert P.predict(P.compose(common + [f"data.target_folder={on}", "data.restore_level=true"])) == 3
    assert len(seen) == 2 and all("source_gain" in b for b in seen)
    gains = {}
    for b, p in zip(seen, plain):
        assert torch.equal(b["enhanced"], p["enhanced"]) and torch.equal(b["perturbed"], p["perturbed"])   # the tensors do not move
        assert b["source_gain"].dtype == torch.float64 and b["source_gain"].device.type == "cpu"
        for i, path in enumerate(b["audio_path"]):
            name = os.path.basename(path)
            rate, frames, level = SOURCES[name]
            n, g = int(b["sample_length"][i]), float(b["source_gain"][i])
            gains[name] = g
            mx = wavio.load_utterance(path, 24000, True, return_peak=True)[2]
            assert g == lv.source_gain(mx) if (rate == 24000 or not device_load) else abs(g - lv.source_gain(mx)) <= 2e-11 / 0.8, name
            at_rate = (rate, frames) if restore_rate else (24000, n)
            _check_file(on / name, b["enhanced"][i], n, at_rate[1], at_rate[0], g, subtype, f"{name} rr={restore_rate} dl={device_load}")
            assert wavio.wav_info(str(off / name)) == (at_rate[1], 1, at_rate[0])
    print("gains", gains)
    assert gains["a24.wav"] == float(np.float64(np.float32(0.1)) / np.float64(0.8))                 # 0.1 : 0.5 : 0.9, as the sources
    # the sources hold nothing above 3.2 kHz: after resampling their peaks are their own to a fraction of a percent
    assert abs(gains["b48.wav"] / gains["a24.wav"] - 5) < 0.05 and abs(gains["c44.wav"] / gains["a24.wav"] - 9) < 0.09
    for csv in ("metrics.csv", "losses.csv"):
        assert (on / csv).read_bytes() == (off / csv).read_bytes(), csv


def test_predict_with_all_channels_gives_a_stereo_file_one_gain(tmp_path, monkeypatch):
    from universal_speech_enhancement_amd import predict as P
    from universal_speech_enhancement_amd.SGMSE_module import SGMSEModule
    src = tmp_path / "noisy"
    src.mkdir()
    a = np.stack([_speech(9600, 61, 0.05), _speech(9600, 62, 0.4)], axis=1)
    wavio.write_wav(str(src / "s.wav"), a, 48000, wavio.FLOAT32)
    seen = []
    _spy(monkeypatch, SGMSEModule, seen)
    common = ["model=SGMSE_Large", f"data.data_folder={src}", "random_init_seed=1", "model.sampler_kwargs.N=1", "data.batch_size=2",
              "data.channels=all", "model.sampler_kwargs.per_item=true", "model.wav_subtype=FLOAT", "data.restore_rate=true",
              "data.device_load=true"]
    assert P.predict(P.compose(common + [f"data.target_folder={tmp_path / 'on'}", "data.restore_level=true"])) == 1
    b = seen[0]
    g = b["source_gain"]
    ref = wavio.load_file_channels(str(src / "s.wav"), 24000, True, return_peak=True)[2]
    assert g.shape == (2,) and float(g[0]) == float(g[1]) and abs(float(g[0]) - lv.source_gain(ref)) <= 2e-11 / 0.8
    assert wavio.wav_info(str(tmp_path / "on" / "s.wav")) == (9600, 2, 48000)
    got = np.frombuffer((tmp_path / "on" / "s.wav").read_bytes()[44:], np.float32).reshape(9600, 2)
    for c in range(2):
        sr.check_float32(np.ascontiguousarray(got[:, c]), lv.want64(b["enhanced"][c, :4800].numpy(), 9600, float(g[0])), f"s.wav channel {c}")
    assert P.predict(P.compose(common + [f"data.target_folder={tmp_path / 'off'}"])) == 1
    flat = np.frombuffer((tmp_path / "off" / "s.wav").read_bytes()[44:], np.float32).reshape(9600, 2)
    for c in range(2):
        sr.check_float32(np.ascontiguousarray(flat[:, c]), sr.oracle(b["enhanced"][c, :4800].numpy(), 9600), f"s.wav channel {c}, flag off")


def test_predict_model_use_undoes_both_normalisations_on_the_refined_files_only(folder, tmp_path, monkeypatch):
    """``model=USE`` with ``model.stage1_folder``: the refined files carry ``source_gain * handoff_peak / 0.8``, the stage-1 files stay
    what the second run's loader reads, and ``metrics.csv`` / ``losses.csv`` do not change by a byte."""
    from universal_speech_enhancement_amd import predict as P
    from universal_speech_enhancement_amd.USE_module import USEModule
    seen = []
    _spy(monkeypatch, USEModule, seen)
    out = {}
    for flag in ("false", "true"):
        out[flag] = (tmp_path / f"refined_{flag}", tmp_path / f"stage1_{flag}")
        assert P.predict(P.compose(["model=USE", f"data.data_folder={folder / 'noisy'}", f"data.target_folder={out[flag][0]}",
                                    f"model.stage1_folder={out[flag][1]}", f"data.clean_folder={folder / 'clean'}",
                                    "data.convergence_losses=true", "random_init_seed=7", "data.batch_size=4",
                                    "model.Score.corrector=langevin", "model.sampler_kwargs.N=1", "model.wav_subtype=FLOAT",
                                    f"data.restore_level={flag}"])) == 3
    b = seen[1]
    assert "source_gain" not in seen[0] and torch.equal(seen[0]["fake"], b["fake"])
    for i, path in enumerate(b["audio_path"]):
        name = os.path.basename(path)
        n = int(b["sample_length"][i])
        g = float(np.float64(b["source_gain"][i]) * (np.float64(b["handoff_peak"][i]) / np.float64(0.8)))
        _check_file(out["true"][0] / name, b["fake"][i].float(), n, n, 24000, g, "FLOAT", f"USE {name}")
        assert (out["true"][1] / name).read_bytes() == (out["false"][1] / name).read_bytes(), name     # stage 1: the model's level
        assert (out["true"][0] / name).read_bytes() != (out["false"][0] / name).read_bytes(), name
    for csv in ("metrics.csv", "losses.csv"):
        assert (out["true"][0] / csv).read_bytes() == (out["false"][0] / csv).read_bytes(), csv
