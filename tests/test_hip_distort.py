"""The degradation simulator on the device (``use_distort``, csrc/use_distort.hip, through ``distort.distort_batch``) against the float64
restatement in ``distort_ref.py``: stage by stage, then the whole chain, on fp64 outputs.

A stage that is one rounded operation per sample - hard clip at a given threshold, DC offset, loudness, packet loss - must have the
restatement's bits.  Every other stage is held to ``max |device - restatement| <= max(8 err_ref, 16 * 2^-52) * peak``: ``err_ref`` is the
restatement's own distance from its longdouble evaluation on that item (``distort_ref.err_ref``; the reverberation there is a direct
convolution), the factor 8 covers another summation order and the ``exp`` / ``pow`` of another libm, the floor is a handful of
roundings.  The clip-on-rate threshold and every keep / drop decision of the -50 dB rule must match exactly (in the chain, where the clipper's
input carries the tolerance of the stages before it: the same edge of the histogram, its value within the scalars' bound).  The other scalars (noise
scale, masked powers, energy ratio, volume and clip scales, normalisation factor) are held to 32 * 2^-52 relative: a mean of n <= 2^21
squares summed pairwise (numpy) or by strided partials and a tree (device) is off by at most about log2(n) roundings either way.

Measured on one MI355X, largest ratio to the bound per stage (profiles/distort.txt): hard, dc, loud1, loud5, packet bit-equal; noise 0.055,
hard_on_rate 0 (bit-equal, threshold exact), soft 0.072, sigmoid1 0.141, sigmoid2 0.156, volume_peak / volume_clip / normalize 0 (bit-equal),
volume_rms 0.093, reverb 0.147 (0.134 at 2^19 points), chain 0.178.  A finding on the way: with x and the RIR packed into ONE complex
transform the reverberation measured 1.495 at 2^19 points next to 7 taps (cross-talk of eps |Z| into the small spectrum; every shorter
case under 0.17) - not a bound to widen: it runs two forward transforms now.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import distort_ref as dr
from universal_speech_enhancement_amd import _lib, distort

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
_cache = {}


def run(name, rows=None, stride=None, out_dtype=torch.float64, pad=dr.PAD, fresh=False):
    """``distort_batch`` on the rows ``rows`` of the case (default: all, in order), re-laid at ``stride`` with ``pad`` behind every row
    -> numpy arrays ``perturbed``, ``clean``, ``scalars``, ``keep``."""
    key = (name, tuple(rows) if rows is not None else None, stride, out_dtype, float(pad))
    if key in _cache and not fresh:
        return _cache[key]
    case = dr.build(name)
    rows = list(range(len(case["lengths"]))) if rows is None else list(rows)
    stride = stride or case["stride"]
    lens = [case["lengths"][b] for b in rows]
    clean = np.full((len(rows), stride), pad, np.float32)
    noise = np.full((len(rows), stride), pad, np.float32)
    rir = np.full((len(rows), case["rir"].shape[1]), pad, np.float32)
    for i, b in enumerate(rows):
        clean[i, : lens[i]] = case["clean"][b, : lens[i]]
        noise[i, : lens[i]] = case["noise"][b, : lens[i]]
        if case["rir_lengths"]:
            rir[i, : case["rir_lengths"][b]] = case["rir"][b, : case["rir_lengths"][b]]
    out = distort.distort_batch(torch.from_numpy(clean).cuda(), lens, [case["recipes"][b] for b in rows], noise=torch.from_numpy(noise).cuda(),
                                rir=torch.from_numpy(rir).cuda() if case["rir_lengths"] else None,
                                rir_lengths=[case["rir_lengths"][b] for b in rows] if case["rir_lengths"] else None,
                                out_dtype=out_dtype, return_keep=True)
    torch.cuda.synchronize()
    got = {k: out[k].cpu().numpy() for k in ("perturbed", "clean", "scalars", "keep")}
    got["SNR"], got["sample_length"] = out["SNR"], out["sample_length"]
    _cache[key] = got
    return got


def ratios(name):
    """Per item and output: max |device - restatement| over the bound.  -> [(b, output, ratio, exact)]"""
    case, got, out = dr.build(name), run(name), []
    for b, n in enumerate(case["lengths"]):
        ref, err = dr.expected(name)[b]
        for k in ("perturbed", "clean"):
            peak = float(np.abs(ref[k]).max())
            diff = float(np.abs(got[k][b, :n] - ref[k]).max())
            out.append((b, k, diff / (max(8 * err[k], 16 * EPS) * peak), np.array_equal(got[k][b, :n], ref[k])))
    return out


@pytest.mark.parametrize("name", dr.CASES)
def test_stage_against_the_restatement(name):
    case, got = dr.build(name), run(name)
    stage = name.partition("@")[0]
    exact = stage in dr.STAGES and dr.STAGES[stage][0]
    for b, k, ratio, same in ratios(name):
        print(f"{name}[{b}] {k}: ratio {ratio:.3f}{' (bit-equal)' if same else ''}")
    for b, k, ratio, same in ratios(name):
        assert same if exact else ratio <= 1.0, (name, b, k, ratio)
    for b, n in enumerate(case["lengths"]):
        ref, _ = dr.expected(name)[b]
        r = case["recipes"][b]
        assert not got["perturbed"][b, n:].any() and not got["clean"][b, n:].any()           # zero from len to the stride
        s, want = got["scalars"][b], ref["scalars"].astype(np.float64)
        rel = np.abs(s - want) / np.maximum(np.abs(want), 1e-300)
        print(f"{name}[{b}] scalars: {dict(zip(_lib.DISTORT_SCALARS, (rel / EPS).round(2)))} (x 2^-52)")
        if r.clip_kind == "hard_on_rate" and (r.reverb or r.snr is not None):
            # behind stages held to a tolerance the histogram's range (min and max |x|) carries their roundings, and so does every
            # edge; what must match exactly is the decision - the same edge of the 1000 - and the edge's value within the scalars' bound
            x32, _, nz32, h32 = dr.item(case, b)
            before = dr.chain(x32, dataclasses.replace(r, clip_kind="none", dc_offset=None, packet_frame=0, packet_factors=(), volume="none",
                                                       normalize=False), nz32, h32)["perturbed"]
            edges = np.histogram_bin_edges(np.abs(before), bins=1000)
            idx = int(np.flatnonzero(edges[:-1] == want[1])[0])
            assert int(np.argmin(np.abs(edges - s[1]))) == idx, (name, b, s[1], want[1])       # its value: `rel` below
        else:
            assert s[1] == want[1], (name, b, s[1], want[1])                                 # the clip threshold: exactly
        assert (rel <= 32 * EPS).all(), (name, b, rel / EPS)
        if r.snr is not None:                                                                # every keep / drop decision
            nf = 1 + n // 512
            assert np.array_equal(got["keep"][b, 0, :nf].astype(bool), ref["keep_clean"]), (name, b)
            assert np.array_equal(got["keep"][b, 1, :nf].astype(bool), ref["keep_noise"]), (name, b)
        assert got["SNR"][b] == (r.snr if r.snr is not None else float("inf")) and int(got["sample_length"][b]) == n


def test_reverb_identity_and_early_equals_full():
    got, case = run("reverb"), dr.build("reverb")
    x = case["clean"][0, :1000].astype(np.float64)
    assert np.array_equal(got["clean"][0, :1000], x)                                         # r = 1: the target is the input
    assert np.abs(got["perturbed"][0, :1000] - x).max() <= 16 * EPS * np.abs(x).max()
    n = case["lengths"][1]                                                                   # r = 6: both are the whole response
    assert np.abs(got["perturbed"][1, :n] - got["clean"][1, :n]).max() <= 2 * 16 * EPS * np.abs(got["clean"][1, :n]).max()


@pytest.mark.parametrize("name", ["chain", "reverb", "noise@seam"])
def test_float32_rows_are_the_cast_of_the_fp64_rows(name):
    a, b = run(name), run(name, out_dtype=torch.float32)
    assert b["perturbed"].dtype == np.float32
    for k in ("perturbed", "clean"):
        assert np.array_equal(torch.from_numpy(a[k]).float().numpy(), b[k]), (name, k)
    assert np.array_equal(a["scalars"], b["scalars"])


def _same(a, b, i, j, n):
    return all(np.array_equal(a[k][i, :n], b[k][j, :n]) for k in ("perturbed", "clean")) and np.array_equal(a["scalars"][i], b["scalars"][j]) \
        and np.array_equal(a["keep"][i, :, : 1 + n // 512], b["keep"][j, :, : 1 + n // 512])


@pytest.mark.parametrize("name", ["chain", "chain@seam"])
def test_an_item_has_the_same_bits_alone_at_another_row_at_another_stride_in_every_run(name):
    case, whole = dr.build(name), run(name)
    B = len(case["lengths"])
    again = run(name, fresh=True)
    order = list(range(B))[::-1]
    moved = run(name, rows=order)
    wide = run(name, stride=case["stride"] + 4133)
    other_pad = run(name, pad=-7.5)                                                          # the padding is inert
    for b, n in enumerate(case["lengths"]):
        assert _same(whole, again, b, b, n), (name, b, "second run")
        assert _same(whole, run(name, rows=[b]), b, 0, n), (name, b, "alone")
        assert _same(whole, moved, b, order.index(b), n), (name, b, "another row")
        assert _same(whole, wide, b, b, n), (name, b, "another stride")
        assert _same(whole, other_pad, b, b, n), (name, b, "other padding")
        assert not wide["perturbed"][b, n:].any() and not wide["clean"][b, n:].any()


def test_batch_goes_through_the_training_step():
    """``distort_batch``'s dict is a batch of ``SGMSEModule.training_step``: a finite loss with its tape, on the synthetic weights."""
    from universal_speech_enhancement_amd.SGMSE_module import SGMSEModule
    from universal_speech_enhancement_amd.sgmse.model_wrapper import ScoreModel
    from universal_speech_enhancement_amd.testing import weights as tw
    n = 6000
    x = torch.from_numpy(np.stack([dr.speechlike(n, 31), dr.speechlike(n, 32)])).cuda()
    nz = torch.from_numpy(np.stack([0.3 * dr.speechlike(n, 33), 0.3 * dr.speechlike(n, 34)])).cuda()
    cfg = distort.default_config()
    cfg.update(reverb_prob=0, add_noise_prob=1, clip_prob=1, packet_loss_prob=1)
    batch = distort.distort_batch(x, [n, n - 700], distort.draw_recipes(cfg, [n, n - 700], 5, [0, 1]), noise=nz)
    assert set(batch) >= {"clean", "perturbed", "sample_length", "SNR", "scalars"} and batch["perturbed"].dtype == torch.float32
    assert batch["sample_length"].tolist() == [n, n - 700] and all(10 <= s < 30 for s in batch["SNR"])
    for b in range(2):                                                                       # output_normalize: the pair's peak is 0.8
        assert max(float(batch["perturbed"][b].abs().max()), float(batch["clean"][b].abs().max())) == pytest.approx(0.8, abs=1e-6)
    assert not batch["perturbed"][1, n - 700:].any() and not batch["clean"][1, n - 700:].any()
    m = ScoreModel(backbone="ncsnpp6M", sde="ouve", t_eps=3e-2, condition="noisy", n_fft=254, hop_length=64, num_frames=64,
                   window="hann", sde_input="noisy", precision="fp32").cuda()
    m.score_net.load_state_dict({k: torch.from_numpy(v) for k, v in tw.make_state_dict(1234, **tw.SMALL6M).items()})
    m.score_net.requires_grad_(True)
    torch.manual_seed(3)
    loss = SGMSEModule(Score=m).training_step(batch, 0)
    assert loss.requires_grad and torch.isfinite(loss), loss


def test_a_refused_call_leaves_the_library_usable():
    L = _lib.lib()
    before = run("sigmoid1")
    x = torch.zeros(1, 1000, device="cuda")
    out = torch.zeros(1, 1000, device="cuda")
    sc = torch.zeros(8, dtype=torch.float64, device="cuda")
    work = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
    P = (_lib.UseDistortParams * 1)()
    P[0].clip_kind = _lib.CLIP_KINDS["sox"]
    lens = (C.c_int * 1)(1000)
    stream = torch.cuda.current_stream().cuda_stream
    args = (x.data_ptr(), None, None, None, 0, lens, None, P, 1, 1000, 0, 0, 0, out.data_ptr(), out.data_ptr(), sc.data_ptr(), None, 0,
            work.data_ptr(), work.numel() * 8, stream)
    assert L.use_distort(*args) == -1 and b"sox" in L.use_last_error()
    torch.cuda.synchronize()
    assert not out.any() and not sc.any()                                                    # nothing was launched
    with pytest.raises(ValueError, match="noise is None"):
        distort.distort_batch(x, [1000], [distort.Recipe(snr=10.0)])
    after = run("sigmoid1", fresh=True)
    assert np.array_equal(before["perturbed"], after["perturbed"]) and np.array_equal(before["scalars"], after["scalars"])


def test_command_line_writes_the_folder_pair(tmp_path):
    """``python -m universal_speech_enhancement_amd.distort`` in process: ``out/clean/<rel>`` and ``out/noisy/<rel>`` for every clean file, the
    same files from the same seed, RIRs from a WAV and a ``.npy`` file."""
    from universal_speech_enhancement_amd import wavio
    for rel, n, seed in (("a.wav", 7000, 1), ("sub/b.wav", 9001, 2), ("sub/c.wav", 5000, 3)):
        (tmp_path / "clean" / rel).parent.mkdir(parents=True, exist_ok=True)
        wavio.write_wav(str(tmp_path / "clean" / rel), dr.speechlike(n, seed), 24000, wavio.FLOAT32)
    (tmp_path / "noise").mkdir()
    wavio.write_wav(str(tmp_path / "noise" / "short.wav"), 0.3 * dr.speechlike(3000, 4), 24000, wavio.FLOAT32)
    wavio.write_wav(str(tmp_path / "noise" / "long.wav"), 0.3 * dr.speechlike(20000, 5), 24000, wavio.FLOAT32)
    (tmp_path / "rir").mkdir()
    wavio.write_wav(str(tmp_path / "rir" / "h.wav"), 0.5 * dr.make_rir(300, 6), 24000, wavio.FLOAT32)
    np.save(tmp_path / "rir" / "g.npy", dr.make_rir(120, 7).astype(np.float64))
    cfg = distort.default_config()
    cfg.update(reverb_prob=1, add_noise_prob=1)
    outs = []
    for out in ("o1", "o2"):
        args = distort.parse_args([f"clean_folder={tmp_path / 'clean'}", f"noise_folder={tmp_path / 'noise'}", f"rir_folder={tmp_path / 'rir'}",
                                   f"out_folder={tmp_path / out}", "seed=11", "batch_size=2"])
        assert distort.simulate_folder(args, cfg) == 3
        outs.append({(sub, rel): wavio.read_wav(str(tmp_path / out / sub / rel))[0] for sub in ("clean", "noisy") for rel in ("a.wav", "sub/b.wav", "sub/c.wav")})
    for (sub, rel), a in outs[0].items():
        n = {"a.wav": 7000, "sub/b.wav": 9001, "sub/c.wav": 5000}[rel]
        assert a.shape == (n,) and np.isfinite(a).all() and np.array_equal(a, outs[1][(sub, rel)]), (sub, rel)
    for rel in ("a.wav", "sub/b.wav", "sub/c.wav"):                                          # output_normalize: the pair peaks at 0.8
        assert max(np.abs(outs[0][("clean", rel)]).max(), np.abs(outs[0][("noisy", rel)]).max()) == pytest.approx(0.8, abs=1e-6)
        assert not np.array_equal(outs[0][("clean", rel)], outs[0][("noisy", rel)])
