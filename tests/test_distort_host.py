"""CPU-only checks of the degradation simulator: the two entry points in the header, the library and the ctypes table; every host-side
refusal of ``use_distort`` (nothing is launched); ``draw_recipes`` and the command line's argument handling; the float64 restatement
in ``distort_ref.py`` - which the GPU tests lean on - against fixed points; the conditioning of every GPU case; and ``err_ref``, the
restatement's distance from its longdouble evaluation, per case."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

import distort_ref as dr
from universal_speech_enhancement_amd import _lib, distort

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("use_distort_workspace", "use_distort")
ITEMS = [(name, b) for name in dr.CASES for b in range(len(dr.build(name)["lengths"]))]


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "use_hip.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in use_hip.h"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS
    for k, v in _lib.CLIP_KINDS.items():
        assert f"USE_CLIP_{k.upper()} = {v}" in header
    for k, v in _lib.VOLUME_MODES.items():
        assert f"USE_VOLUME_{k.upper()} = {v}" in header
    for i, k in enumerate(_lib.DISTORT_SCALARS):
        assert f"USE_DISTORT_{k.upper()} = {i}" in header
    assert f"USE_DISTORT_SCALARS = {len(_lib.DISTORT_SCALARS)}" in header
    assert _lib.SYMBOLS["use_distort_workspace"][0] is C.c_size_t
    # the record: 10 ints, one 64-bit offset, 10 doubles, in the header's order
    assert C.sizeof(_lib.UseDistortParams) == 128 and _lib.UseDistortParams.packet_off.offset == 40
    assert _lib.UseDistortParams.snr_lin.offset == 48 and _lib.UseDistortParams.volume_target.offset == 120
    fields = re.search(r"typedef struct use_distort_params \{(.*?)\} use_distort_params;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.strip().split("[")[0] for decl in fields.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].replace("long ", "").split(",")]
    assert names == [f[0] for f in _lib.UseDistortParams._fields_], names


def test_workspace_is_zero_for_bad_arguments_and_grows():
    L = _lib.lib()
    for n, r in ((0, 0), (-3, 0), (100, -1), ((1 << 24) + 1, 0), (1 << 24, 2), (2, 1 << 24)):
        assert L.use_distort_workspace(n, r) == 0, (n, r)
    a, b, c = L.use_distort_workspace(1000, 0), L.use_distort_workspace(100000, 0), L.use_distort_workspace(100000, 12000)
    assert 0 < a < b < c and a % 16 == 0 and c % 16 == 0
    assert L.use_distort_workspace(1 << 24, 1) > 0 and L.use_distort_workspace((1 << 24) - 6, 7) > 0
    # the FFT buffers hold three transforms of pow2 >= len + r - 1 points
    assert L.use_distort_workspace(1019, 6) - L.use_distort_workspace(1019, 0) == 3 * 16 * 1024
    assert L.use_distort_workspace(1019, 7) - L.use_distort_workspace(1019, 0) == 3 * 16 * 2048


def _params(**kw):
    P = (_lib.UseDistortParams * 2)()
    for q in P:
        q.snr_lin, q.volume_target = 1.0, 1.0
        for k, v in kw.items():
            if k == "loud":
                for i, f in enumerate(v):
                    q.loud[i] = f
            else:
                setattr(q, k, v)
    return P


def test_refusals_name_the_argument_and_launch_nothing():
    """Host-only: every check is in front of the first launch, so host memory stands in for the device buffers."""
    L = _lib.lib()
    buf = np.zeros(8, np.float64)
    p = buf.ctypes.data
    inf, nan = float("inf"), float("nan")

    def call(clean=p, noise=p, rir=p, packet=p, packet_count=1 << 30, lens=(1000, 900), nlens=(1000, 900), params=None, B=2, stride=1000,
             noise_stride=1000, rir_stride=64, out_fp64=0, pert=p, target=p, scalars=p, keep=None, keep_stride=0, work=p, nbytes=1 << 40, **kw):
        la = (C.c_int * len(lens))(*lens) if lens is not None else None
        na = (C.c_int * len(nlens))(*nlens) if nlens is not None else None
        P = _params(**kw) if params is None else params
        return L.use_distort(clean, noise, rir, packet, packet_count, la, na, P if params != "null" else None, B, stride, noise_stride,
                             rir_stride, out_fp64, pert, target, scalars, keep, keep_stride, work, nbytes, None)

    cases = [(dict(clean=None), b"clean is null"), (dict(lens=None), b"len_host"), (dict(params="null"), b"params is null"),
             (dict(pert=None), b"perturbed is null"), (dict(target=None), b"clean_out is null"), (dict(scalars=None), b"scalars_dev"),
             (dict(work=None), b"work is null"), (dict(B=0), b"B=0"), (dict(B=65536), b"B=65536"), (dict(B=-1), b"B=-1"),
             (dict(lens=(1000, 0)), b"len[1]=0"), (dict(lens=(1001, 900)), b"len[0]=1001"), (dict(stride=0), b"stride=0"),
             (dict(out_fp64=2), b"out_fp64=2"),
             (dict(reverb=1, rir_len=0), b"rir_len=0"), (dict(reverb=1, rir_len=65), b"rir_len=65"), (dict(reverb=1, rir_len=8, rir=None), b"rir is null"),
             (dict(reverb=1, rir_len=(1 << 24), rir_stride=1 << 25), b"FFT's limit"),
             (dict(add_noise=1, noise=None), b"noise is null"), (dict(add_noise=1, nlens=None), b"noise_len_host"),
             (dict(add_noise=1, nlens=(1000, 899)), b"noise_len[1]=899"), (dict(add_noise=1, nlens=(1001, 900)), b"noise_len[0]=1001"),
             (dict(add_noise=1, snr_lin=nan), b"snr_lin"), (dict(add_noise=1, snr_lin=inf), b"snr_lin"), (dict(add_noise=1, snr_lin=0.0), b"snr_lin"),
             (dict(n_loud=6), b"n_loud=6"), (dict(n_loud=-1), b"n_loud=-1"), (dict(n_loud=2, loud=(1.0, nan)), b"loud[1]"),
             (dict(clip_kind=8), b"clip_kind=8"), (dict(clip_kind=-1), b"clip_kind=-1"),
             (dict(clip_kind=_lib.CLIP_KINDS["sox"]), b"sox"), (dict(clip_kind=_lib.CLIP_KINDS["pedal"]), b"pedal"),
             (dict(clip_kind=_lib.CLIP_KINDS["hard"], clip_a=nan), b"clip_a"), (dict(clip_kind=_lib.CLIP_KINDS["sigmoid1"], clip_a=1.0, clip_b=inf), b"clip_b"),
             (dict(clip_kind=_lib.CLIP_KINDS["hard_on_rate"], clip_a=0.0), b"rate"), (dict(clip_kind=_lib.CLIP_KINDS["hard_on_rate"], clip_a=1.5), b"rate"),
             (dict(clip_kind=_lib.CLIP_KINDS["hard_on_rate"], clip_a=-0.1), b"rate"), (dict(clip_kind=_lib.CLIP_KINDS["soft"], clip_a=0.0), b"slope"),
             (dict(dc=1, dc_offset=nan), b"dc_offset"), (dict(packet_frame=-1), b"frame_size"), (dict(packet_frame=100, packet=None), b"packet is null"),
             (dict(packet_frame=100, packet_count=9), b"packet_count=9"), (dict(packet_frame=100, packet_off=-1), b"packet_off=-1"),
             (dict(volume=3), b"volume=3"), (dict(volume=1, volume_target=nan), b"volume_target"), (dict(volume=2, volume_target=0.0), b"volume_target"),
             (dict(keep=p, keep_stride=1), b"keep_stride=1"),
             (dict(nbytes=L.use_distort_workspace(1000, 0) - 1), b"work_bytes"),
             (dict(reverb=1, rir_len=64, nbytes=L.use_distort_workspace(1000, 64) - 1), b"work_bytes")]
    for kw, word in cases:
        assert call(**kw) == -1, kw                                # USE_E_INVALID
        assert word in L.use_last_error(), (kw, L.use_last_error())
    # a rate of exactly 1 and a frame of one sample are inside the ranges: the next check (a short workspace) is the one that refuses
    for kw in (dict(clip_kind=_lib.CLIP_KINDS["hard_on_rate"], clip_a=1.0), dict(packet_frame=1)):
        assert call(nbytes=16, **kw) == -1 and b"work_bytes" in L.use_last_error(), kw


def test_python_surface_refuses_what_it_cannot_run():
    import torch
    x = torch.zeros(2, 1000)
    with pytest.raises(_lib.UseHipError, match="CUDA"):            # no CPU implementation, no quiet fall-back
        distort.distort_batch(x, [1000, 900], [distort.Recipe(), distort.Recipe()])
    for bad, word in ((distort.Recipe(clip_kind="sox"), "not built"), (distort.Recipe(clip_kind="pedal"), "not built"),
                      (distort.Recipe(clip_kind="fuzz"), "clip_kind"), (distort.Recipe(volume="lufs"), "volume"),
                      (distort.Recipe(loudness=(1.0,) * 6), "loudness"), (distort.Recipe(packet_frame=300, packet_factors=(1.0,) * 3), "packet_factors")):
        with pytest.raises(ValueError, match=word):
            distort.params_of([bad], [1000])
    P, packets = distort.params_of([distort.Recipe(packet_frame=300, packet_factors=(1.0, 0.0, 0.5, 1.0)), distort.Recipe(snr=20.0),
                                    distort.Recipe(packet_frame=500, packet_factors=(0.0, 1.0))], [1000, 1000, 1000])
    assert packets.tolist() == [1.0, 0.0, 0.5, 1.0, 0.0, 1.0] and (P[0].packet_off, P[2].packet_off) == (0, 4)
    assert P[1].add_noise == 1 and P[1].snr_lin == np.power(10.0, 2.0) and P[0].add_noise == 0


def test_prepare_rir_trims_to_the_peak_and_divides_by_it():
    h = np.array([0.01, -0.02, 0.5, -2.0, 1.0, 0.25])
    out = distort.prepare_rir(h)
    assert out.dtype == np.float32 and out.tolist() == [-1.0, 0.5, 0.125]          # divided by |peak|: the sign stays
    assert distort.prepare_rir(np.stack([h, 3 * h], axis=1)).tolist() == [-1.0, 0.5, 0.125]       # the first channel
    with pytest.raises(ValueError):
        distort.prepare_rir(np.zeros(5))


# ---- draw_recipes and the command line ------------------------------------------------------------------------------------------------

def _all_on():
    cfg = distort.default_config()
    cfg.update(reverb_prob=1, add_noise_prob=1, loudness_perturb_prob=1, clip_prob=1, dc_offset_prob=1, packet_loss_prob=1,
               hard_clip_portion=0.5, packet_loss_hard_loss_prob=0.5)
    return cfg


def test_shipped_configuration_has_the_built_stages_keys_only():
    cfg = distort.default_config()
    assert not [k for k in distort.UNBUILT_PROBS if k in cfg]
    assert cfg["soft_clip_types"] == ["soft", "sigmoid1", "sigmoid2"] and cfg["sampling_rate"] == 24000
    assert (cfg["snr_min"], cfg["snr_max"], cfg["reverb_prob"], cfg["add_noise_prob"]) == (10, 30, 0.5, 0.5)
    distort.check_config(cfg)


def test_draw_recipes_gives_a_key_the_same_recipe_in_any_batch():
    cfg = _all_on()
    keys, lens = [11, 2 ** 63 + 5, 7, 900], [24000, 9000, 31000, 1200]
    whole = distort.draw_recipes(cfg, lens, 42, keys)
    for order in ([2, 0], [3], [1, 3, 0, 2]):
        part = distort.draw_recipes(cfg, [lens[i] for i in order], 42, [keys[i] for i in order])
        assert part == [whole[i] for i in order]
    assert distort.draw_recipes(cfg, lens, 43, keys) != whole
    assert whole[0] != distort.draw_recipes(cfg, lens[:1], 42, [12])[0]
    with pytest.raises(ValueError, match="lengths"):
        distort.draw_recipes(cfg, lens, 42, keys[:2])


def test_draw_recipes_keeps_its_values_inside_the_ranges():
    cfg = _all_on()
    n = 24000
    rs = distort.draw_recipes(cfg, [n] * 300, 1, range(300))
    kinds = set()
    for r in rs:
        assert r.reverb and cfg["snr_min"] <= r.snr < cfg["snr_max"]
        assert 1 <= len(r.loudness) <= 5 and all(0.1 <= f < 10 for f in r.loudness)
        kinds.add(r.clip_kind)
        if r.clip_kind == "hard_on_rate":
            assert 0 < r.clip_a < cfg["hard_clip_rate_max"]
        elif r.clip_kind == "soft":
            assert 1 <= r.clip_a < 5
        elif r.clip_kind == "sigmoid1":
            assert 1 <= r.clip_a < 5 and 1 <= r.clip_b < 5
        elif r.clip_kind == "sigmoid2":
            assert 10 ** (-10 / 20) <= r.clip_a < 10 ** (-1 / 20) and 1 <= r.clip_b < 4
        assert cfg["dc_offset_min"] <= r.dc_offset < cfg["dc_offset_max"]
        assert int(24000 * 0.008) <= r.packet_frame <= int(24000 * 0.04) and len(r.packet_factors) == -(-n // r.packet_frame)
        assert all(f == 1.0 or 0.0 <= f < cfg["packet_loss_decay_rate_max"] for f in r.packet_factors)
        assert r.volume == "peak" and cfg["volume_min_sample"] <= r.volume_target < cfg["volume_max_sample"] and r.normalize
    assert kinds == {"hard_on_rate", "soft", "sigmoid1", "sigmoid2"}
    lost = np.mean([np.mean(np.array(r.packet_factors) != 1.0) for r in rs])
    assert cfg["packet_loss_rate_min"] < lost < cfg["packet_loss_rate_max"]
    cfg.update(hard_clip_on_rate=False, hard_clip_portion=1, use_rms_volume=True)
    for r in distort.draw_recipes(cfg, [n] * 20, 2, range(20)):
        assert r.clip_kind == "hard" and 10 ** (-40 / 20) <= r.clip_a <= 1 and r.volume == "rms"
    off = distort.default_config()
    off.update(reverb_prob=0, add_noise_prob=0, clip_prob=0, dc_offset_prob=0, packet_loss_prob=0, random_volume=False, output_normalize=False)
    assert distort.draw_recipes(off, [n], 3, [0]) == [distort.Recipe()]


def test_draw_recipes_refuses_the_stages_that_are_not_built():
    for k in distort.UNBUILT_PROBS:
        cfg = distort.default_config()
        cfg[k] = 0.1
        with pytest.raises(ValueError, match=k):
            distort.draw_recipes(cfg, [1000], 0, [0])
        cfg[k] = 0
        distort.draw_recipes(cfg, [1000], 0, [0])
    for k, v in (("soft_clip_types", ["sox", "soft"]), ("soft_clip_types", ["pedal"]), ("packet_loss_on_vad", True), ("sync_random_volume", False)):
        cfg = distort.default_config()
        cfg[k] = v
        with pytest.raises(ValueError, match=k):
            distort.draw_recipes(cfg, [1000], 0, [0])


def test_command_line_arguments(tmp_path):
    a = distort.parse_args(["clean_folder=c", "noise_folder=n", "rir_folder=r", "out_folder=o", "seed=7", "n=3"])
    assert (a["clean_folder"], a["noise_folder"], a["rir_folder"], a["out_folder"], a["seed"], a["n"]) == ("c", "n", "r", "o", 7, 3)
    b = distort.parse_args(["clean_folder=c", "out_folder=o"])
    assert b["seed"] == 0 and b["n"] is None and b["noise_folder"] is None and b["rir_folder"] is None
    for argv, word in ((["clean_folder=c"], "out_folder"), (["out_folder=o"], "clean_folder"), (["clean_folder=c", "out_folder=o", "speed=2"], "speed"),
                       (["clean_folder=c", "out_folder=o", "seed=x"], "seed"), (["clean_folder=c", "out_folder=o", "n=0"], "positive"),
                       (["clean_folder=c", "out_folder=o", "--help"], "--help")):
        with pytest.raises(SystemExit, match=word):
            distort.parse_args(argv)
    (tmp_path / "sub").mkdir()
    for f in ("b.wav", "a.WAV", "sub/c.wav", "x.npy", "notes.txt", "h.pkl"):
        (tmp_path / f).write_bytes(b"")
    assert distort.list_files(str(tmp_path), (".wav",)) == ["a.WAV", "b.wav", "sub/c.wav"]
    assert distort.list_files(str(tmp_path), (".wav", ".npy")) == ["a.WAV", "b.wav", "sub/c.wav", "x.npy"]      # no pickles
    with pytest.raises(SystemExit, match="no .wav"):
        distort.simulate_folder(distort.parse_args([f"clean_folder={tmp_path / 'sub' / 'none'}", "out_folder=o"]))
    np.save(tmp_path / "rir.npy", np.array([0.1, -1.0, 0.5]))
    assert distort.load_rir(str(tmp_path / "rir.npy"), 24000).tolist() == [-1.0, 0.5]
    rng = np.random.default_rng(0)
    assert len(distort.fit_noise(np.arange(10.0), 25, rng)) == 25 and len(distort.fit_noise(np.arange(100.0), 25, rng)) == 25


# ---- the restatement ------------------------------------------------------------------------------------------------------------------

def test_vad_mask_equals_the_interval_form_sample_for_sample():
    """``vad_merge`` concatenates the intervals ``librosa.effects.split`` returns; the device keeps sample s iff frame s // 512 is kept."""
    dropped = 0
    for n, seed in ((1003, 1), (4097, 2), (10007, 3), (24000, 4), (512 * 20, 5), (30000, 6)):
        w = dr.speechlike(n, seed).astype(np.float64)
        mask = np.zeros(n, bool)
        for s, e in dr.split_intervals(w):
            mask[s:e] = True
        assert np.array_equal(mask, dr.vad_keep(w)), n
        dropped += int((~mask).sum())
    assert dropped > 0
    assert dr.vad_frames(np.zeros(3000)).all()                       # silence: every frame is at the reference level


def test_restatement_fixed_points():
    x = dr.speechlike(5000, 9).astype(np.float64)
    full, early = dr.reverberate(x, np.array([1.0]))
    assert np.array_equal(full, x) and np.array_equal(early, x)
    h = dr.make_rir(6, 1).astype(np.float64)
    full, early = dr.reverberate(x, h)
    assert np.array_equal(full, early) and np.abs(full - dr.convolve_direct(x, h)).max() < 1e-14
    noisy, scale, pc, pn = dr.add_noise(x, 0.3 * dr.speechlike(5000, 10).astype(np.float64), 10.0)
    got = 10 * np.log10(pc / (scale ** 2 * pn))
    assert abs(got - 10.0) < 1e-4, got                             # the SNR over the kept samples is the one asked for
    assert np.array_equal(dr.loudness(x, (2.0,)), 2.0 * x) and np.array_equal(dr.loudness(x[:1003], (0.5,) * 5)[1000:], x[1000:1003])
    y, thr, _ = dr.clip(x, "hard_on_rate", 0.1)
    assert 0.08 < np.mean(np.abs(x) >= thr) < 0.12 and np.abs(y).max() == thr
    for kind, a, b in (("sigmoid1", 2.0, 1.5), ("sigmoid2", 0.5, 2.0)):
        y, _, es = dr.clip(x, kind, a, b)
        assert abs(np.sqrt(np.mean(y ** 2)) / np.sqrt(np.mean(x ** 2)) - 1) < 1e-6
    y = dr.packet_loss(x[:1000], 480, (1.0, 0.0, 0.5))
    assert np.array_equal(y[:480], x[:480]) and not y[480:960].any() and np.array_equal(y[960:], 0.5 * x[960:1000])
    a, b, vs, cs, nf = dr.volume(x, 0.5 * x, "peak", 4.0, True)
    assert cs < 1 and abs(np.abs(a).max() - 0.8) < 1e-15 and abs(np.abs(b).max() - 0.4) < 1e-15


# ---- conditioning of the GPU cases (on the restatement alone) and err_ref ---------------------------------------------------------------

@pytest.mark.parametrize("name,b", ITEMS)
def test_case_is_well_conditioned(name, b):
    case = dr.build(name)
    n, r = case["lengths"][b], case["recipes"][b]
    assert case["clean"].dtype == np.float32 and (case["clean"][b, n:] == dr.PAD).all() and (case["noise"][b, n:] == dr.PAD).all()
    ref, err = dr.expected(name)[b]
    x32, _, nz32, h32 = dr.item(case, b)
    print(f"{name}[{b}]: len {n}, err_ref perturbed {err['perturbed'] / 2 ** -52:.2f} clean {err['clean'] / 2 ** -52:.2f} (x 2^-52)")
    assert np.isfinite(ref["perturbed"]).all() and np.isfinite(ref["clean"]).all() and np.isfinite(ref["scalars"]).all()
    assert err["perturbed"] < 64 * 2.0 ** -52 and err["clean"] < 64 * 2.0 ** -52
    if r.snr is not None:                                          # no frame within 1e-9 dB of the -50 dB threshold
        full = dr.reverberate(x32.astype(np.float64), h32.astype(np.float64))[0] if r.reverb else x32.astype(np.float64)
        assert dr.keep_margin(full) > 1e-9 and dr.keep_margin(nz32) > 1e-9
    if r.clip_kind != "none" or r.volume == "rms":
        stage_in = dr.chain(x32, dataclasses.replace(r, clip_kind="none", dc_offset=None, packet_frame=0, packet_factors=(), volume="none",
                                                     normalize=False), nz32, h32)["perturbed"]
        if r.clip_kind == "hard_on_rate":                          # no |x| within 1e-12 (relative) of a histogram edge
            assert dr.edge_margin(stage_in) > 1e-12
        if r.clip_kind == "sigmoid2":                              # no b of sigmoid2 at 0, where a jumps from 0.5 to 4
            xc = np.clip(stage_in, -r.clip_a, r.clip_a)
            assert np.abs(1.5 * xc - 0.3 * xc ** 2).min() > 0
    if r.volume == "rms":
        before = dr.chain(x32, dataclasses.replace(r, volume="none", normalize=False), nz32, h32)
        assert dr.keep_margin(before["perturbed"]) > 1e-9 and dr.keep_margin(before["clean"]) > 1e-9
    if r.volume != "none":                                         # no peak within 1e-9 of 0.99
        assert abs(ref["peak_before_clip"] - 0.99) > 1e-9


def test_cases_cover_what_they_are_there_for():
    kept = dr.expected("noise")[1][0]
    assert 0 < kept["keep_clean"].sum() < len(kept["keep_clean"]) and 0 < kept["keep_noise"].sum() < len(kept["keep_noise"])   # both really drop frames
    big = dr.expected("noise@seam")[0][0]
    assert big["keep_clean"].sum() < len(big["keep_clean"]) - 100
    assert -(-dr.SEAM[0] // dr.SLICE) > 256 and dr.SEAM[1] < dr.SLICE
    assert dr.SMALL[0] < dr.SLICE < dr.SMALL[1] == dr.SLICE + 1 and all(n % 512 and n % 5 and n % 480 for n in dr.SMALL)
    assert dr.expected("volume_clip")[0][0]["scalars"][4] < 1 and dr.expected("volume_peak")[0][0]["scalars"][4] == 1
    assert [r.clip_kind for r in dr.build("chain")["recipes"]] == ["hard_on_rate", "sigmoid2", "soft"]
    full, early = dr.expected("reverb")[1][0]["perturbed"], dr.expected("reverb")[1][0]["clean"]
    assert np.array_equal(full, early)                             # r = 6: the early part is the whole response
    x = dr.build("reverb")["clean"][0, :1000].astype(np.float64)
    assert np.array_equal(dr.expected("reverb")[0][0]["perturbed"], x)      # r = 1: the identity
    f = dr.build("packet")["recipes"][0].packet_factors
    assert len(f) == 3 and 1003 - 2 * 480 < 480
