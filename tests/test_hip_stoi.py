"""Device-side STOI / ESTOI (``use_stoi``, csrc/use_stoi.hip) against the float64 restatement in ``stoi_ref.py``.

Tolerance: ``|device - restatement| <= 1e-10`` for both scores in every case.  Both sides are fp64 and differ only in the order of their
sums; ``stoi_ref.sensitivity`` - the largest change of the restatement when the 10 kHz signals move by 2^-43 max|x|, which bounds any
reordering of the resampler's filter sum - is 2e-14 ... 2e-13 on these cases, and the host test holds it under 1e-12: two decades below
the bound.  The frame count has no tolerance."""
import csv
import ctypes as C

import numpy as np
import pytest
import torch

import stoi_ref as sr
from universal_speech_enhancement_amd import _lib, metrics
from universal_speech_enhancement_amd.sgmse.util import other
from universal_speech_enhancement_amd.testing import noise as tnoise

pytestmark = pytest.mark.gpu
TOL = 1e-10


def run(clean, est, lengths, rate):
    """-> float64 [B, 3] on the host: stoi, estoi, frames."""
    r = metrics.intelligibility(torch.tensor(est).cuda(), torch.tensor(clean).cuda(), lengths, rate)
    return torch.stack([r["stoi"], r["estoi"], r["stoi_frames"]], dim=1).cpu().numpy()


@pytest.fixture(scope="module")
def device_values():
    """Every case through the device once: {case: [B, 3]}."""
    out = {}
    for name in sr.CASE_NAMES:
        rate, _, lengths, clean, est = sr.build(name)
        out[name] = run(clean, est, lengths, rate)
    return out


@pytest.mark.parametrize("name", sr.CASE_NAMES)
def test_scores_match_the_restatement(device_values, name):
    got, want = device_values[name], sr.expected(name)
    for b, (d, e, T) in enumerate(want):
        print(f"{name}[{b}]: device {got[b].tolist()}, restatement {(d, e, T)}, off by {abs(got[b, 0] - d):.2e} / {abs(got[b, 1] - e):.2e}")
    for b, (d, e, T) in enumerate(want):
        assert got[b, 2] == T
        assert np.isfinite(got[b]).all()
        assert abs(got[b, 0] - d) <= TOL and abs(got[b, 1] - e) <= TOL


def test_too_short_gives_pystois_value(device_values):
    assert device_values["too_short"][0].tolist() == [1e-5, 1e-5, 29.0]
    assert device_values["one_segment"][0, 2] == 30.0


def test_padding_is_inert(device_values):
    rate, stride, lengths, clean, est = sr.build("mixed")
    c, e = clean.copy(), est.copy()
    for b, n in enumerate(lengths):
        c[b, n:] = 1e3
        e[b, n:] = 1e3
    assert np.array_equal(run(c, e, lengths, rate), device_values["mixed"])


def test_an_item_has_the_same_bits_alone_and_in_the_batch(device_values):
    rate, stride, lengths, clean, est = sr.build("mixed")
    for b, n in enumerate(lengths):
        alone = run(clean[b:b + 1], est[b:b + 1], [n], rate)                      # same stride
        own = run(clean[b, :n].copy(), est[b, :n].copy(), None, rate)            # 1-D, its own length
        assert np.array_equal(alone[0], device_values["mixed"][b]) and np.array_equal(own[0], device_values["mixed"][b]), b
    # the items in reverse order: each at another row of the batch
    swapped = run(clean[::-1].copy(), est[::-1].copy(), lengths[::-1], rate)
    assert np.array_equal(swapped[::-1], device_values["mixed"])


def test_two_runs_agree_bit_for_bit(device_values):
    for name in ("gaps", "mixed", "rate48k"):
        rate, _, lengths, clean, est = sr.build(name)
        assert np.array_equal(run(clean, est, lengths, rate), device_values[name]), name


@pytest.mark.parametrize("name", ["one_segment", "gaps", "rate16k", "rate48k", "rate10k"])
def test_identity_gives_one(name):
    rate, _, lengths, clean, _ = sr.build(name)
    got = run(clean, clean, lengths, rate)
    print(f"{name}: est == clean gives {got[0].tolist()}")
    assert got[0, 0] >= 1 - 1e-12 and got[0, 1] >= 1 - 1e-12
    assert got[0, 0] <= 1 + 1e-12 and got[0, 1] <= 1 + 1e-12


def test_a_refused_call_leaves_the_library_usable(device_values):
    rate, stride, lengths, clean, est = sr.build("one_segment")
    c, e = torch.tensor(clean).cuda(), torch.tensor(est).cuda()
    L = _lib.lib()
    nbytes = L.use_stoi_workspace(1, stride, rate)
    work = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device="cuda")
    out = torch.full((1, 3), -7.0, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    lens = (C.c_int * 1)(stride + 1)
    assert L.use_stoi(e.data_ptr(), c.data_ptr(), lens, 1, stride, rate, work.data_ptr(), nbytes, out.data_ptr(), stream) == -1
    assert b"len[0]=%d" % (stride + 1) in L.use_last_error()
    torch.cuda.synchronize()
    assert (out.cpu() == -7.0).all()                               # nothing was launched
    with pytest.raises(ValueError, match="lengths"):
        metrics.stoi(e, c, [stride + 1], rate)
    with pytest.raises(ValueError, match="lengths"):
        metrics.stoi(e, c, [612], rate)
    with pytest.raises(TypeError, match="float32"):
        metrics.stoi(e.double(), c.double())
    with pytest.raises(ValueError, match="shape"):
        metrics.stoi(e, torch.cat([c, c]))
    lens = (C.c_int * 1)(stride)
    assert L.use_stoi(e.data_ptr(), c.data_ptr(), lens, 1, stride, rate, work.data_ptr(), nbytes, out.data_ptr(), stream) == 0
    assert np.array_equal(out.cpu().numpy(), device_values["one_segment"])


def test_python_surfaces_agree_bit_for_bit(device_values):
    rate, stride, lengths, clean, est = sr.build("mixed")
    c, e = torch.tensor(clean).cuda(), torch.tensor(est).cuda()
    both = metrics.intelligibility(e, c, lengths, rate)
    assert set(both) == {"stoi", "estoi", "stoi_frames"} and all(v.dtype == torch.float64 and v.shape == (3,) for v in both.values())
    d, x = metrics.stoi(e, c, lengths, rate), metrics.stoi(e, c, lengths, rate, extended=True)
    assert torch.equal(d, both["stoi"]) and torch.equal(x, both["estoi"]) and d.dtype == torch.float64 and d.is_cuda
    assert np.array_equal(d.cpu().numpy(), device_values["mixed"][:, 0]) and np.array_equal(x.cpu().numpy(), device_values["mixed"][:, 1])
    # pystoi's order: clean first
    assert torch.equal(other.stoi(c, e, rate, lengths=lengths), d) and torch.equal(other.stoi(c, e, rate, extended=True, lengths=lengths), x)
    n = lengths[1]
    one = other.stoi(clean[1, :n].copy(), est[1, :n].copy(), rate)               # numpy in, a Python float out
    assert isinstance(one, float) and one == device_values["mixed"][1, 0]
    assert other.stoi(clean[1, :n].copy(), est[1, :n].copy(), rate, extended=True) == device_values["mixed"][1, 1]


def test_predict_with_intelligibility_appends_two_columns(tmp_path, capsys):
    """Two short files with random weights, as ``test_predict_with_clean_folder_writes_metrics_csv`` runs them: with the option the header
    ends in ``stoi,estoi`` and the values are ``score_files``'; without it the CSV is the four columns of before, value for value.  The
    shorter file has fewer than 30 frames: 1e-5 and one warning line that names it."""
    from scipy.io import wavfile

    from universal_speech_enhancement_amd import predict as P
    src, clean, dst, dst0 = (tmp_path / k for k in ("noisy", "clean", "enhanced", "plain"))
    src.mkdir()
    clean.mkdir()
    files = {"a.wav": 19200, "b.wav": 4800}
    for i, (rel, n) in enumerate(files.items()):
        w = tnoise.synth_noisy_speech(1, n, seed=60 + i)[0]
        wavfile.write(str(src / rel), 24000, w.astype(np.float32))
        wavfile.write(str(clean / rel), 24000, (w * 0.9 + 0.01 * tnoise.normal(4, rel, n)).astype(np.float32))
    common = ["model=SGMSE_Large", f"data.data_folder={src}", "random_init_seed=1", "model.sampler_kwargs.N=1", f"data.clean_folder={clean}"]
    capsys.readouterr()
    assert P.predict(P.compose(common + [f"data.target_folder={dst}", "data.intelligibility=true"])) == 2
    err = capsys.readouterr().err
    assert P.predict(P.compose(common + [f"data.target_folder={dst0}"])) == 2
    rows, rows0 = list(csv.reader(open(dst / "metrics.csv"))), list(csv.reader(open(dst0 / "metrics.csv")))
    assert rows0[0] == ["file", "si_sdr", "si_sir", "si_sar", "lsd"]
    assert rows[0] == rows0[0] + ["stoi", "estoi"] and [r[0] for r in rows[1:]] == list(files) + ["mean"]
    assert [r[:5] for r in rows] == rows0                          # the four columns of today, digit for digit
    for rel in files:
        assert (dst / rel).read_bytes() == (dst0 / rel).read_bytes(), rel
    vals = np.array([[float(v) for v in r[1:]] for r in rows[1:]])
    assert np.isfinite(vals).all() and np.array_equal(vals[-1], vals[:-1].mean(axis=0))
    for r, rel in zip(vals, files):
        want = metrics.score_files(str(dst / rel), str(clean / rel), str(src / rel), 24000, True, "cuda", intelligibility=True)
        assert [want[k] for k in metrics.NAMES + metrics.STOI_NAMES] == list(r), rel
    assert -1 <= vals[0, 4] <= 1 and vals[0, 4] != 1e-5 and vals[1, 4] == vals[1, 5] == 1e-5
    warned = [ln for ln in err.splitlines() if ln.startswith("warning:") and "STOI" in ln]
    assert len(warned) == 1 and "b.wav" in warned[0], err
