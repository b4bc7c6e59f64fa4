"""CPU-only half of the long-waveform tests (tests/long_waveform_ref.py holds the cases; tests/test_hip_long_waveform.py runs them on the
GPU).  Four things are settled here, without a kernel:

  the seams      every constant the cases lean on is read back from the line of csrc/ it was copied from, and the counts of slices,
                 frames, ints and rows of every case are recomputed from those constants: each case crosses its seam by at least two.
  the lengths    the batches of more than 64 items obey ``len[b] != len[b - 64]`` and ``len[b] != len[b % 64]``.
  conditioning   every new input meets the floors the bounds assume (``metrics_ref.BIN_FLOOR`` and ``RATIO_RANGE_DB``,
                 ``spec_losses_ref.MAG_FLOOR`` / ``INV_MEAN_CAP``).
  the controls   each defect the GPU cases are there to catch is emulated in numpy on the case's own input and must exceed the bound of
                 the check meant to catch it; the same emulation without the defect must hold that bound.  A bit-exact check has no
                 bound: there the figure is the number of elements that differ, which must be 0 without the defect.

Every figure is printed before it is asserted (``pytest -s``): ``[control]`` lines give measured / bound, above 1 with the defect."""
import os
import re

import numpy as np
import pytest

import chunk_ref as cr
import handoff_ref as hr
import long_waveform_ref as lw
import metrics_ref as mr
import spec_losses_ref as sl

REL = [0, 1, 2, 3, 4, 9, 10, 11, 12, 14]                          # tests/test_hip_spec_losses.py: 1e-10 relative ...
ABS = [5, 6, 7, 8, 13]                                             # ... 1e-8 absolute
RATIO_BOUND_SHORT = 1e-5                                           # tests/test_hip_metrics.py: derived for n <= 24 000


def _differ(a, b) -> int:
    """Elements of two float32 arrays that are not bit-equal."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


# ---- the seams ---------------------------------------------------------------------------------------------------------------------
def test_constants_are_the_source_lines():
    for name, pattern, value in lw.SOURCE_CONSTANTS:
        found = re.findall(pattern, open(os.path.join(lw.CSRC, name)).read())
        assert found and all(int(v) == value for v in found), (name, pattern, found, value)
    assert lw.CHUNK_FIRST_PASS == 262140


def test_every_case_crosses_its_seam_by_two():
    two = lw.TRIP + 2                                              # partials 256 and 257 exist
    # 1. item lengths: a launch at base > 0, partly filled
    assert lw.launches(len(lw.metrics_many()["lengths"])) == 3 and len(lw.metrics_many()["lengths"]) % lw.PACK == 2
    assert lw.launches(len(lw.losses_many()["lengths"])) == 2 and len(lw.losses_many()["lengths"]) - lw.PACK == 2
    assert lw.launches(len(lw.handoff_many()["lengths"])) == 2 and len(lw.handoff_many()["lengths"]) - lw.PACK == 2
    rows = {k: sum(v) for k, v in lw.FILE_LAYOUTS.items()}
    assert rows == {"19 rows": 19, "70 rows": 70} and all(4 * r >= lw.PACK + 2 for r in rows.values())
    assert lw.launches(4 * 19) == 2 and lw.launches(4 * 70) == 5
    assert lw.straddled_triples(70) == [19, 40]                    # ints 127 | 128, 129 and 190, 191 | 192
    assert sorted(set(lw.FILE_LAYOUTS["70 rows"])) == list(range(1, 9))
    # 2. metrics: slices of 2048 and frames of hop 128, the long item and the short one next to it
    _, stride, (L0, L1) = lw.METRICS_LONG
    assert lw.ceil_div(L0, lw.METRICS_SLICE) == two and lw.lsd_frames(L0) == 4113 and L0 == stride
    assert lw.ceil_div(L1, lw.METRICS_SLICE) == 17 and lw.lsd_frames(L1) == two
    # 3. hand-off: slices of 16384
    L0, L1, L2 = lw.HANDOFF_LENGTHS
    assert lw.HANDOFF_STRIDE % 2 == 1 and lw.ceil_div(L0, lw.HANDOFF_SLICE) == two + 1 and lw.ceil_div(L1, lw.HANDOFF_SLICE) == two
    assert lw.HANDOFF_PEAK_AT // lw.HANDOFF_SLICE == lw.TRIP + 1 and lw.HANDOFF_PEAK_AT < L1
    assert lw.ceil_div(lw.HANDOFF_STRIDE, lw.HANDOFF_SLICE) - lw.ceil_div(L2, lw.HANDOFF_SLICE) >= 257          # slices of pure padding
    # 4. loader: slices of 4096 over the file, and over both channels of the two-channel file
    assert lw.ceil_div(lw.LOAD_FRAMES, lw.LOAD_SLICE) == two and lw.ceil_div(2 * lw.LOAD_FRAMES, lw.LOAD_SLICE) == 2 * lw.TRIP + 3
    # 5. chunk rows against 65535 blocks of 4
    B, F, Tp = lw.SPLIT_SHAPE
    n = cr.ref_plan(Tp, lw.CHUNK_C, lw.CHUNK_OVERLAP)[0]
    assert n == 172 and Tp % 64 == 0 and B * n * F == 264192 and lw.ceil_div(B * n * F, lw.CHUNK_ROWS) >= lw.CHUNK_GRID_Y + 2
    B, F, Tp = lw.MERGE_SHAPE
    assert cr.ref_plan(Tp, lw.CHUNK_C, lw.CHUNK_OVERLAP)[0] == 3 and Tp % 64 == 0
    assert B * F == 262200 and lw.ceil_div(B * F, lw.CHUNK_ROWS) >= lw.CHUNK_GRID_Y + 2
    assert B * 3 * F <= 1 << 30                                    # chunk_args' documented refusal is far away
    # 6. losses: slices of 8192, and every map far beyond 256 frames
    _, stride, (L0, L1), rate = lw.LOSSES_LONG
    assert lw.ceil_div(L0, lw.SL_WAV_SLICE) == two and L1 == sl.min_length(rate) == 1025
    assert all(1 + L0 // (n // 4) >= two for n in sl.frame_lengths(rate)) and 1 + L0 // int(0.010 * rate) >= two


def test_length_rules():
    for lens, lo, hi in ((lw.metrics_many()["lengths"], 256, 512), (lw.losses_many()["lengths"], 1025, 1500), (lw.handoff_many()["lengths"], 1, 97)):
        lens = [int(v) for v in lens]
        assert lw.rule_holds(lens) and lo <= min(lens) and max(lens) <= hi
        for mode in ("previous", "first"):
            wrong = lw.wrong_lengths(lens, mode)
            assert wrong[:lw.PACK] == lens[:lw.PACK] and all(w != v for w, v in zip(wrong[lw.PACK:], lens[lw.PACK:]))
    assert not lw.rule_holds([300] * 65) and not lw.rule_holds(list(range(64)) + [0])
    for layout in lw.FILE_LAYOUTS:
        c = lw.handoff_files(layout)
        assert len(set(c["lengths"])) == len(c["lengths"]) and sum(c["channels"]) == c["wav"].shape[0]


# ---- conditioning -----------------------------------------------------------------------------------------------------------------
def _metric_items(c):
    for b, L in enumerate(int(v) for v in c["lengths"]):
        yield b, L, c["est"][b, :L], c["clean"][b, :L], c["noise"][b, :L]


@pytest.mark.parametrize("case", ["metrics_many", "metrics_long"])
def test_metric_inputs_are_well_conditioned(case):
    c = getattr(lw, case)()
    lo, hi = mr.RATIO_RANGE_DB
    floor, worst_inv, rmin, rmax = np.inf, 0.0, np.inf, -np.inf
    for b, L, e, s, n in _metric_items(c):
        assert (c["est"][b, L:] == 1e3).all() and (c["clean"][b, L:] == 1e3).all() and (c["noise"][b, L:] == 1e3).all()
        t, r = lw.lsd_terms(e, s), mr.ratios(e, s, n)
        floor, worst_inv, rmin, rmax = min(floor, t["floor"]), max(worst_inv, t["inv_mean"]), min(rmin, min(r)), max(rmax, max(r))
    print(f"{case}: smallest bin {floor:.3e}, largest mean 1/|S^| + mean 1/|S| {worst_inv:.3e}, ratios {rmin:.2f} ... {rmax:.2f} dB")
    assert floor >= mr.BIN_FLOOR and lo <= rmin and rmax <= hi


@pytest.mark.parametrize("case", ["losses_many", "losses_long"])
def test_loss_inputs_are_well_conditioned(case):
    c = getattr(lw, case)()
    floor, cap = np.inf, 0.0
    for b, L in enumerate(int(v) for v in c["lengths"]):
        assert np.isnan(c["est"][b, L:]).all() and np.isnan(c["clean"][b, L:]).all()
        for x in (c["est"][b, :L], c["clean"][b, :L]):
            for M in sl.maps(x, c["rate"]):
                floor, cap = min(floor, float(M.min())), max(cap, float(np.mean(1.0 / M)))
    print(f"{case}: smallest magnitude {floor:.3e}, largest mean(1 / M) {cap:.3e}")
    assert floor >= sl.MAG_FLOOR and cap <= sl.INV_MEAN_CAP


def test_the_rederived_bounds():
    """The ratio bound at the old case's size lies inside the old constant; at the long item it is what the docstring of the GPU module
    quotes.  The LSD bound of every input is far below the values it guards."""
    assert lw.ratio_bound_db(24000, 40.0) <= RATIO_BOUND_SHORT
    c = lw.metrics_long()
    for b, L, e, s, n in _metric_items(c):
        sar, t = mr.ratios(e, s, n)[2], lw.lsd_terms(e, s)
        print(f"metrics_long[{b}]: n = {L}, SI-SAR {sar:.2f} dB -> ratio bound {lw.ratio_bound_db(L, sar):.3e} dB; LSD {t['lsd']:.6f}, "
              f"bound {t['bound']:.3e}")
        assert lw.ratio_bound_db(L, sar) < 1e-4 and t["bound"] < 1e-8 * t["lsd"]


# ---- the controls: lengths from the wrong item ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["previous", "first"])
def test_control_wrong_lengths_metrics(mode):
    c = lw.metrics_many()
    lens = [int(v) for v in c["lengths"]]
    worst_r, worst_l = np.inf, np.inf
    for b, W in enumerate(lw.wrong_lengths(lens, mode)):
        if b < lw.PACK:
            continue
        L = lens[b]
        e, s, n = (c[k][b] for k in ("est", "clean", "noise"))
        dr = np.abs(np.array(mr.ratios(e[:W], s[:W], n[:W])) - np.array(mr.ratios(e[:L], s[:L], n[:L]))).max()
        t = lw.lsd_terms(e[:L], s[:L])
        dl = abs(mr.lsd(e[:W], s[:W]) - t["lsd"])
        worst_r, worst_l = min(worst_r, dr / RATIO_BOUND_SHORT), min(worst_l, dl / t["bound"])
    print(f"[control] metrics, lengths of items >= 64 from the {mode} launch: smallest change / bound, ratios {worst_r:.3e}, LSD {worst_l:.3e}")
    assert worst_r > 1 and worst_l > 1


@pytest.mark.parametrize("mode", ["previous", "first"])
def test_control_wrong_lengths_losses(mode):
    c = lw.losses_many()
    lens = [int(v) for v in c["lengths"]]
    for b, W in enumerate(lw.wrong_lengths(lens, mode)):
        if b < lw.PACK:
            continue
        L = lens[b]
        want = sl.item_values(c["est"][b, :L], c["clean"][b, :L], c["rate"])
        got = sl.item_values(c["est"][b, :W], c["clean"][b, :W], c["rate"])       # a longer length reads the NaN of the padding
        if not np.isfinite(got).all():
            print(f"[control] losses[{b}], length {W} for {L} ({mode}): not finite")
            continue
        rel, ab = np.abs(got[REL] - want[REL]) / np.abs(want[REL]), np.abs(got[ABS] - want[ABS])
        print(f"[control] losses[{b}], length {W} for {L} ({mode}): smallest change / bound, relative {rel.min() / 1e-10:.3e}, "
              f"absolute {ab.min() / 1e-8:.3e}")
        assert rel.min() > 1e-10 and ab.min() > 1e-8


@pytest.mark.parametrize("mode", ["previous", "first"])
@pytest.mark.parametrize("subtype,normalize", [("PCM_16", True), ("PCM_16", False), ("FLOAT", True), ("FLOAT", False)])
def test_control_wrong_lengths_handoff(subtype, normalize, mode):
    c = lw.handoff_many()
    want, wpeak = hr.handoff_batch(c["wav"], c["lengths"], subtype, normalize)
    got, _ = hr.handoff_batch(c["wav"], lw.wrong_lengths(c["lengths"], mode), subtype, normalize)
    assert not want[:, max(c["lengths"]):].any() and np.isfinite(want).all()
    rows = [_differ(got[b], want[b]) for b in range(lw.PACK, len(c["lengths"]))]
    print(f"[control] hand-off {subtype} normalize={normalize}, lengths from the {mode} launch: elements that differ per item >= 64: {rows} (0 allowed)")
    assert min(rows) > 1 and _differ(got[:lw.PACK], want[:lw.PACK]) == 0


# ---- the controls: a files triple read one int off ------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(lw.FILE_LAYOUTS))
@pytest.mark.parametrize("subtype,normalize", [("PCM_16", True), ("FLOAT", True)])
def test_control_files_triple_one_int_off(layout, subtype, normalize):
    c = lw.handoff_files(layout)
    ints, B = lw.file_ints(c["lengths"], c["channels"])
    want, wpeak = lw.files_reference(c["wav"], c["lengths"], c["channels"], subtype, normalize)
    same, speak = lw.files_emulated(c["wav"], ints, B, subtype, normalize)
    first = np.cumsum([0] + c["channels"][:-1])
    assert _differ(same, want) == 0 and np.array_equal(speak[first], wpeak)           # the emulation without the defect is the reference
    assert np.isfinite(want).all() and float(np.abs(want).max()) == np.float32(0.8)
    for f, (r0, ch) in enumerate(zip(first, c["channels"])):                          # one gain per file: a louder row than the first
        assert ch == 1 or np.abs(want[r0]).max() < np.float32(0.8), f
    off, _ = lw.files_emulated(c["wav"], ints, B, subtype, normalize, shift=1)
    rows = [_differ(off[b], want[b]) for b in range(B)]
    print(f"[control] hand-off of files ({layout}, {subtype}), triples read one int off: elements that differ per row {rows} (0 allowed)")
    # a shifted triple can by chance still cover the file's loudest row (file 1 of the 70 rows: rows 1 ... 5 of the next files too)
    assert sum(r > 1 for r in rows) >= B - len(c["channels"])


# ---- the controls: partials with an index >= 256 dropped ------------------------------------------------------------------------------
def test_control_dropped_partials_metrics():
    c = lw.metrics_long()
    for b, L, e, s, n in _metric_items(c):
        want = np.array(mr.ratios(e, s, n))
        bound = lw.ratio_bound_db(L, want[2])
        t = lw.lsd_terms(e, s)
        kept = np.abs(np.array(lw.ratios_from_partials(e, s, n)) - want).max() / bound
        kept_l = abs(lw.lsd_from_partials(t["frame_sums"]) - mr.lsd(e, s)) / t["bound"]
        lost = np.abs(np.array(lw.ratios_from_partials(e, s, n, keep=lw.TRIP)) - want).max() / bound
        lost_l = abs(lw.lsd_from_partials(t["frame_sums"], keep=lw.TRIP) - t["lsd"]) / t["bound"]
        print(f"[control] metrics_long[{b}] measured / bound: all partials ratios {kept:.3e} LSD {kept_l:.3e}; partials >= 256 dropped "
              f"ratios {lost:.3e} LSD {lost_l:.3e}")
        assert kept < 1 and kept_l < 1 and lost_l > 1                                 # both items have more than 256 frames ...
        assert (lost > 1) == (b == 0)                                                 # ... and the long one more than 256 slices


def test_control_dropped_partials_loss_wav_term():
    c = lw.losses_long()
    L = int(c["lengths"][0])
    e, s = c["est"][0, :L].astype(np.float64), c["clean"][0, :L].astype(np.float64)
    want = sl.item_values(c["est"][0, :L], c["clean"][0, :L], c["rate"])[0]
    kept = abs(lw.partial_sums(np.abs(e - s), lw.SL_WAV_SLICE) / L - want) / want / 1e-10
    lost = abs(lw.partial_sums(np.abs(e - s), lw.SL_WAV_SLICE, keep=lw.TRIP) / L - want) / want / 1e-10
    print(f"[control] losses_long[0] wav_l1 measured / bound: all partials {kept:.3e}, partials >= 256 dropped {lost:.3e}")
    assert kept < 1 < lost


@pytest.mark.parametrize("subtype", ["PCM_16", "FLOAT"])
def test_control_dropped_partials_handoff_peak(subtype):
    c = lw.handoff_long()
    L0, L1, _ = c["lengths"]
    x = c["wav"][0, :L0]
    want, mx = hr.handoff_row(x, subtype, True)
    dec = np.abs(hr.handoff_row(x, subtype, False)[0].astype(np.float64))
    assert lw.peak_from_partials(dec, lw.HANDOFF_SLICE) == mx and int(dec.argmax()) == lw.HANDOFF_PEAK_AT
    assert _differ(lw.scaled_by(x, subtype, mx), want) == 0
    lost = lw.peak_from_partials(dec, lw.HANDOFF_SLICE, keep=lw.TRIP)
    n = _differ(lw.scaled_by(x, subtype, lost), want)
    print(f"[control] hand-off row 0 ({subtype}): peak {mx!r}, with partials >= 256 dropped {lost!r}: {n} elements differ (0 allowed)")
    assert lost < mx and n > 1
    # row 1 peaks in slice 0; as the second row of a file with row 0, the file's peak is row 0's - in its partial 257
    dec1 = np.abs(hr.handoff_row(c["wav"][1, :L1], subtype, False)[0].astype(np.float64))
    assert int(dec1.argmax()) == 1234 and dec1.max() < np.abs(hr.handoff_row(c["wav"][0, :L1], subtype, False)[0]).max() == mx
    assert (c["wav"][2, 65:] == 1e9).all() and (c["wav"][1, L1:] == 1e9).all()


def test_control_dropped_partials_loader_peak(tmp_path):
    """The three files: where their peaks lie (after resampling for the 48 kHz file), and the 24 kHz file normalised by a peak that
    misses the partials from 256 on."""
    from universal_speech_enhancement_amd import wavio
    paths = lw.write_loader_files(tmp_path)
    assert wavio.wav_info(paths["a"]) == (lw.LOAD_FRAMES, 1, 24000) and wavio.wav_info(paths["b"]) == (2 * lw.LOAD_FRAMES, 1, 48000)
    assert wavio.wav_info(paths["ab"]) == (lw.LOAD_FRAMES, 2, 24000)
    assert wavio.resampled_length(2 * lw.LOAD_FRAMES, 48000, 24000) == lw.LOAD_FRAMES
    last = (lw.TRIP + 1) * lw.LOAD_SLICE                                              # the first sample of slice 257
    raw, _ = wavio.read_wav(paths["a"])
    want, _ = wavio.load_utterance(paths["a"], 24000, True)
    mx = lw.peak_from_partials(np.abs(raw), lw.LOAD_SLICE)
    assert int(np.abs(raw).argmax()) >= last and _differ((raw / mx * 0.8).astype(np.float32), want) == 0
    lost = lw.peak_from_partials(np.abs(raw), lw.LOAD_SLICE, keep=lw.TRIP)
    n = _differ((raw / lost * 0.8).astype(np.float32), want)
    print(f"[control] loader, 24 kHz file: peak {mx!r}, with partials >= 256 dropped {lost!r}: {n} elements differ (0 allowed)")
    assert lost < mx and n > 1
    plain, _ = wavio.load_utterance(paths["b"], 24000, False)
    assert plain.shape == (lw.LOAD_FRAMES,) and int(np.abs(plain).argmax()) >= last
    both, _ = wavio.load_file_channels(paths["ab"], 24000, False)
    flat = np.abs(both.reshape(-1))                                                   # channel after channel, as load_peak_kernel sees the file
    assert int(flat.argmax()) >= 2 * lw.TRIP * lw.LOAD_SLICE + 2 * lw.LOAD_SLICE and np.abs(both[0]).max() < np.abs(both[1]).max()
    res = np.abs(plain.astype(np.float64))
    d = abs(res.max() - lw.peak_from_partials(res, lw.LOAD_SLICE, keep=lw.TRIP)) / res.max() * 0.8
    print(f"[control] loader, 48 kHz file: a peak without partials >= 256 moves the samples by up to {d:.3e} ({d / 1e-7:.3e} x the 1e-7 bound)")
    assert d > 1e-7


# ---- the controls: chunk rows the first grid pass cannot reach ----------------------------------------------------------------------
def test_control_unwritten_chunk_rows():
    B, F, Tp = lw.SPLIT_SHAPE
    want = cr.ref_split(lw.split_input(), lw.CHUNK_C, lw.CHUNK_OVERLAP)
    rows = want.reshape(-1, lw.CHUNK_C).copy()
    assert rows.shape[0] == 264192
    rows[lw.CHUNK_FIRST_PASS:] = np.nan
    n = int((rows.view(np.uint32) != want.reshape(-1, lw.CHUNK_C).view(np.uint32)).any(axis=1).sum())
    print(f"[control] split: rows >= {lw.CHUNK_FIRST_PASS} left unwritten: {n} rows differ (0 allowed)")
    assert n == rows.shape[0] - lw.CHUNK_FIRST_PASS
    # merge: the last item holds every row the first pass cannot reach (the kernel treats the items alike)
    B, F, Tp = lw.MERGE_SHAPE
    chunks = lw.merge_input()
    assert chunks.shape == (B * 3, 1, F, lw.CHUNK_C) and (B - 1) * F < lw.CHUNK_FIRST_PASS
    assert not np.array_equal(chunks[0, 0, 0], chunks[0, 0, 1]) and not np.array_equal(chunks[0, 0, 0], chunks[1, 0, 0])
    ref, bound = cr.ref_merge(chunks[(B - 1) * 3:], 1, Tp, lw.CHUNK_C, lw.CHUNK_OVERLAP)
    out = ref.astype(np.complex64)
    cr.check_merged(out, ref, bound, "merge, last item, float32 rounding of the reference")
    out[0, 0, lw.CHUNK_FIRST_PASS - (B - 1) * F:] = np.nan
    with pytest.raises(AssertionError):
        cr.check_merged(out, ref, bound, f"[control] merge, rows >= {lw.CHUNK_FIRST_PASS} left unwritten")
