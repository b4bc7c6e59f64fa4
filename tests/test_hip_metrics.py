"""GPU checks of the device metrics (``use_metrics``, csrc/use_metrics.hip) against ``tests/golden/metrics.npz`` - the reference's own
``energy_ratios`` (float64) and ``lsd`` (float32 ``torch.stft``) - and of the properties the kernels promise bit for bit: padding is
never read, an item does not depend on its batch, two runs agree.  Then the Python surface and the ``predict`` option.

Bounds.  Ratios: 1e-5 dB - fp64 sums of exact float32 products over at most 24 000 terms carry a relative error of about
n * 2^-53 = 3e-12, which a 40 dB SI-SAR amplifies by at most 1e4: under 1e-6 dB, and the bound leaves a decade.  LSD: 4 x the
fixture's ``lsd_f32_vs_f64`` of the item (the reference's own float32-against-float64 distance, 1e-7 ... 1e-6 here - a float32 ulp
of the result).  Every figure is printed before it is asserted (``pytest -s``)."""
import ctypes as C

import numpy as np
import pytest
import torch

import metrics_ref as mr
from universal_speech_enhancement_amd import _lib, metrics
from universal_speech_enhancement_amd.testing import noise as tnoise

pytestmark = pytest.mark.gpu

CASE_NAMES = [c[0] for c in mr.CASES]


@pytest.fixture(scope="module")
def golden():
    g = np.load(mr.GOLDEN)
    return {name: mr.load_case(g, name) for name in CASE_NAMES}


@pytest.fixture(scope="module")
def device_out(golden):
    """use_metrics on every case of the fixture, once: float64 [B, 4] (host) per case."""
    return {name: _run(c).cpu().numpy() for name, c in golden.items()}


def _dev(c):
    return [torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("est", "clean", "noise")]


def _run(c, noise=True, lengths=None):
    e, s, n = _dev(c)
    return metrics._run(e, s, n if noise else None, c["lengths"] if lengths is None else lengths)


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


@pytest.mark.parametrize("case", CASE_NAMES)
def test_ratios_match_the_reference(golden, device_out, case):
    for b, (got, want) in enumerate(zip(device_out[case][:, :3], golden[case]["ratios"])):
        d = np.abs(got - want)
        print(f"{case}[{b}]: SI-SDR / SI-SIR / SI-SAR {got} dB, off by {d} dB")
        assert np.isfinite(got).all() and d.max() <= 1e-5


@pytest.mark.parametrize("case", CASE_NAMES)
def test_lsd_matches_the_reference(golden, device_out, case):
    c = golden[case]
    for b, (got, want, sens) in enumerate(zip(device_out[case][:, 3], c["lsd"], c["lsd_f32_vs_f64"])):
        print(f"{case}[{b}]: LSD {got!r}, reference {want!r}, off by {abs(got - want):.3e}, bound 4 x {sens:.3e}")
        assert abs(got - want) <= 4 * sens


def test_padding_is_inert(golden, device_out):
    c = dict(golden["mixed"])
    for k in ("est", "clean", "noise"):
        a = c[k].copy()
        for b, L in enumerate(c["lengths"]):
            a[b, L:] = 1e3
        c[k] = a
    assert (c["est"][1, 257:] == 1e3).all()
    assert _same_bits(_run(c).cpu(), torch.from_numpy(device_out["mixed"]))


@pytest.mark.parametrize("case", ["mixed", "short"])
def test_an_item_does_not_depend_on_its_batch(golden, device_out, case):
    """Item b alone - as a batch of one at the same stride, and as a 1-D signal of its own length - gives the bits it has in the batch."""
    c = golden[case]
    e, s, n = _dev(c)
    for b, L in enumerate(int(v) for v in c["lengths"]):
        want = torch.from_numpy(device_out[case][b:b + 1])
        assert _same_bits(metrics._run(e[b:b + 1], s[b:b + 1], n[b:b + 1], [L]).cpu(), want), (case, b, "same stride")
        assert _same_bits(metrics._run(e[b, :L], s[b, :L], n[b, :L], None).cpu(), want), (case, b, "own length")


@pytest.mark.parametrize("case", CASE_NAMES)
def test_two_runs_agree_bit_for_bit(golden, device_out, case):
    assert _same_bits(_run(golden[case]).cpu(), torch.from_numpy(device_out[case]))


def test_without_noise_the_ratios_are_nan_and_lsd_is_unchanged(golden, device_out):
    out = _run(golden["mixed"], noise=False).cpu()
    assert torch.isnan(out[:, :3]).all()
    assert _same_bits(out[:, 3], torch.from_numpy(device_out["mixed"][:, 3].copy()))
    e, s, _ = _dev(golden["mixed"])
    assert _same_bits(metrics.lsd(e, s, golden["mixed"]["lengths"]).cpu(), out[:, 3])


def test_an_all_zero_clean_signal_gives_finite_values():
    """Not value-compared (the reference's result there is rounding noise over eps); it has to be finite."""
    est = torch.from_numpy(0.1 * tnoise.normal(5, "zero_est", 2 * 1024).reshape(2, 1024)).cuda()
    zero = torch.zeros_like(est)
    for clean, noise in ((zero, est), (zero, zero), (est, zero)):
        out = metrics._run(est, clean, noise, [1024, 300]).cpu()
        assert torch.isfinite(out).all(), out
    out = metrics._run(zero, zero, zero, None).cpu()
    assert torch.isfinite(out).all() and (out[:, 3] == 0).all(), out


def test_refusals_leave_the_library_usable(golden, device_out):
    L = _lib.lib()
    c = golden["mixed"]
    e, s, n = _dev(c)
    B, stride = e.shape
    nbytes = L.use_metrics_workspace(B, stride)
    work = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device="cuda")
    out = torch.full((B, 4), -7.0, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(est=e.data_ptr(), lens=tuple(int(v) for v in c["lengths"]), nb=nbytes):
        return L.use_metrics(est, s.data_ptr(), n.data_ptr(), (C.c_int * B)(*lens), B, stride, work.data_ptr(), nb, out.data_ptr(), stream)

    for kw, word in ((dict(lens=(4096, 255, 1300)), b"len[1]=255"), (dict(lens=(4097, 257, 1300)), b"len[0]=4097"),
                     (dict(est=None), b"est"), (dict(nb=nbytes - 1), b"work_bytes")):
        assert call(**kw) == -1, kw                                # USE_E_INVALID
        assert word in L.use_last_error(), (kw, L.use_last_error())
    torch.cuda.synchronize()
    assert (out == -7.0).all()                                     # nothing was launched
    assert call() == 0
    assert _same_bits(out.cpu(), torch.from_numpy(device_out["mixed"]))
    with pytest.raises(ValueError, match="lengths"):
        metrics.lsd(e, s, [4096, 255, 1300])


def test_other_and_evaluate_agree(golden, device_out):
    """``sgmse.util.other`` (the reference's names and argument order) and ``metrics.evaluate`` are the same kernels on the same values."""
    from universal_speech_enhancement_amd.sgmse.util import other
    c = golden["mixed"]
    e, s, n = _dev(c)
    noisy = s + n
    ev = metrics.evaluate(e, s, noisy, c["lengths"])
    assert set(ev) == set(metrics.NAMES) and all(v.dtype == torch.float64 and tuple(v.shape) == (3,) and v.is_cuda for v in ev.values())
    sdr, sir, sar = other.energy_ratios(e, s, noisy - s, lengths=c["lengths"])
    assert _same_bits(sdr, ev["si_sdr"]) and _same_bits(sir, ev["si_sir"]) and _same_bits(sar, ev["si_sar"])
    assert _same_bits(other.lsd(e, s, lengths=c["lengths"]), ev["lsd"])
    assert _same_bits(ev["lsd"].cpu(), torch.from_numpy(device_out["mixed"][:, 3].copy()))
    # 1-D tensors give 0-d tensors, numpy arrays (what the reference takes) Python floats; lengths=None is the full width
    one = metrics.evaluate(e[0], s[0], noisy[0])
    assert float(other.lsd(e[0], s[0])) == float(one["lsd"][0]) == float(ev["lsd"][0]) and other.lsd(e[0], s[0]).dim() == 0
    got = other.energy_ratios(c["est"][0], c["clean"][0], (noisy - s)[0].cpu().numpy())
    assert all(isinstance(v, float) for v in got) and got == tuple(float(ev[k][0]) for k in ("si_sdr", "si_sir", "si_sar"))
    st, en, ea = other.si_sdr_components(e[0], s[0], n[0])
    assert st.is_cuda and torch.allclose(st + en + ea, e[0].double(), rtol=0, atol=1e-15)


def test_predict_with_clean_folder_writes_metrics_csv(tmp_path):
    """Two short files, one in a sub-folder and with a clean file 100 samples shorter (scored over the shorter); a third noisy file
    has no clean counterpart and gets no row.  The rows are ``metrics.evaluate`` on the files that were written; without the option
    the same WAVs are written and no CSV."""
    import csv
    import os

    from scipy.io import wavfile

    from universal_speech_enhancement_amd import predict as P
    from universal_speech_enhancement_amd.wavio import load_utterance, read_wav
    src, clean, dst, dst0 = (tmp_path / k for k in ("noisy", "clean", "enhanced", "plain"))
    (src / "sub").mkdir(parents=True)
    (clean / "sub").mkdir(parents=True)
    files = {"a.wav": (4800, 4800), os.path.join("sub", "b.wav"): (6000, 5900)}
    for i, (rel, (ln, lc)) in enumerate(files.items()):
        w = tnoise.synth_noisy_speech(1, ln, seed=20 + i)[0]
        wavfile.write(str(src / rel), 24000, w.astype(np.float32))
        wavfile.write(str(clean / rel), 24000, (w[:lc] * 0.9 + 0.01 * tnoise.normal(3, rel, lc)).astype(np.float32))
    wavfile.write(str(src / "c.wav"), 24000, tnoise.synth_noisy_speech(1, 4800, seed=30)[0].astype(np.float32))
    common = ["model=SGMSE_Large", f"data.data_folder={src}", "random_init_seed=1", "model.sampler_kwargs.N=1"]
    assert P.predict(P.compose(common + [f"data.target_folder={dst}", f"data.clean_folder={clean}"])) == 3
    assert P.predict(P.compose(common + [f"data.target_folder={dst0}"])) == 3
    assert not (dst0 / "metrics.csv").exists()
    for rel in list(files) + ["c.wav"]:
        assert (dst / rel).read_bytes() == (dst0 / rel).read_bytes(), rel
    rows = list(csv.reader(open(dst / "metrics.csv")))
    assert rows[0] == ["file", "si_sdr", "si_sir", "si_sar", "lsd"] and [r[0] for r in rows[1:]] == list(files) + ["mean"]
    vals = np.array([[float(v) for v in r[1:]] for r in rows[1:]])
    assert np.isfinite(vals).all() and np.array_equal(vals[-1], vals[:-1].mean(axis=0))
    for r, rel in zip(vals, files):
        est = read_wav(str(dst / rel))[0].astype(np.float32)
        c, _ = load_utterance(str(clean / rel), 24000, True)
        y, _ = load_utterance(str(src / rel), 24000, True)
        m = min(len(est), len(c), len(y))
        assert m == files[rel][1]
        ev = metrics.evaluate(*(torch.from_numpy(a[:m].copy()).cuda() for a in (est, c, y)))
        assert [float(ev[k][0]) for k in metrics.NAMES] == list(r), rel
