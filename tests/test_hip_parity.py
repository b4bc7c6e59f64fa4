"""GPU parity tests: the HIP path (through the C ABI) against the reference's golden vectors and the CPU oracle.

Tolerances (relative to the reference tensor's max magnitude unless stated):
  fp32 storage  : one score evaluation  <= 5e-4   (measured 3e-6 .. 5e-5)
                  whole sampler, waveform <= 2e-3
  16-bit storage: multiples of the REFERENCE's own 16-bit (CPU autocast) error, tests/lowprec.py + tests/golden/lowprec_reference.npz:
                  one score evaluation <= 1.0 x (bf16 2.33e-2, fp16 3.33e-3; measured 1.8e-2 / 2.1e-3),
                  sampler outputs <= 3 x (rel-max) / 2 x (rel-L2) the reference's 60-evaluation chain drift; single operators: 4 ulps of the storage type.
  Every test prints what it measured (pytest -s, "[measured]").
"""
import math
import os

import numpy as np
import pytest
import torch

from oracle import ncsnpp_oracle as no
from oracle import sde_oracle as so
import lowprec as lp
from universal_speech_enhancement_amd._lib import UseHipError
from universal_speech_enhancement_amd.testing import noise as tnoise
from universal_speech_enhancement_amd.testing import weights as tw
from universal_speech_enhancement_amd.testing.cpu import usable_cores

pytestmark = pytest.mark.gpu


def _relmax(a, b):
    a, b = torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu()
    return float((a - b).abs().max() / b.abs().max())


def _check(err, tol, *tag):
    """Assert with the measured error on record (pytest -s)."""
    print("[measured]", *tag, f"{err:.3g} (bound {tol:g})")
    assert err < tol, (tag, err, tol)


@pytest.fixture(scope="module")
def sd_np():
    return tw.make_state_dict(1234, **tw.LARGE)


@pytest.fixture(scope="module")
def engines(sd_np):
    from universal_speech_enhancement_amd.hip_engine import HipScoreEngine
    out = {}
    for prec in ("fp32", "bf16", "fp16"):
        e = HipScoreEngine(precision=prec)
        e.load_state_dict(sd_np)
        out[prec] = e
    yield out
    for e in out.values():
        e.close()


def _score_model(sd_np, precision, corrector="langevin", use_graph=True):
    from universal_speech_enhancement_amd.sgmse.model_wrapper import ScoreModel
    m = ScoreModel(backbone="ncsnpplarge", sde="ouve", t_eps=3e-2, condition="noisy", n_fft=1022, hop_length=160,
                   num_frames=512, window="hann", sde_input="noisy", predictor="reverse_diffusion", corrector=corrector,
                   precision=precision, use_graph=use_graph)
    m.score_net.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
    return m


@pytest.mark.parametrize("prec,tol", [("fp32", 5e-4), ("bf16", lp.fwd_bound("bf16")), ("fp16", lp.fwd_bound("fp16"))])   # 16-bit: the reference's own autocast error (tests/lowprec.py)
def test_score_matches_reference_golden(golden_dir, engines, prec, tol):
    g = dict(np.load(os.path.join(golden_dir, "forward_large.npz")))
    x = torch.from_numpy(g["x"]).cuda()
    for tag in ("a", "b"):
        out = engines[prec].score(x[:, 0:1].contiguous(), x[:, 1:2].contiguous(), torch.from_numpy(g["t_" + tag]).cuda())
        err = _relmax(out, -torch.from_numpy(g["out_" + tag]))        # library returns score = -net
        _check(err, tol, "score vs forward_large", prec, tag)


@pytest.mark.parametrize("prec,tol", [("fp32", 5e-4), ("bf16", lp.fwd_bound("bf16")), ("fp16", lp.fwd_bound("fp16"))])   # 16-bit: the reference's own autocast error (tests/lowprec.py)
def test_score_golden_with_wide_tile_kernel_forced(golden_dir, engines, prec, tol):
    """conv_wide_kernel (conv_v4 / conv_v5) is normally reserved for maps of >= 128 workgroups per image; force it onto the golden-vector shapes."""
    from universal_speech_enhancement_amd.hip_engine import set_option
    g = dict(np.load(os.path.join(golden_dir, "forward_large.npz")))
    x = torch.from_numpy(g["x"]).cuda()
    set_option("conv_v4_min_blocks", 1)
    try:
        out = engines[prec].score(x[:, 0:1].contiguous(), x[:, 1:2].contiguous(), torch.from_numpy(g["t_a"]).cuda())
    finally:
        set_option("conv_v4_min_blocks", 80)
    err = _relmax(out, -torch.from_numpy(g["out_a"]))
    _check(err, tol, "score vs forward_large, conv_v4 forced", prec)
    with pytest.raises(Exception):
        set_option("no_such_option", 1)


@pytest.mark.parametrize("prec,tol,tol_wav", [("fp32", 5e-4, 2e-3), ("bf16", lp.refine_bound("bf16"), 2 * lp.refine_bound("bf16"))])   # bf16: the reference's own error; waveform: spec_back squares the magnitude (2x)
def test_lsgan_refine_generator_matches_reference(golden_dir, prec, tol, tol_wav):
    """NCSNpp(discriminative=True) through the backbone interface and NCSNPP_Wrapper / GANModule.predict_step
    through the batch-dict contract, against outputs of the reference itself."""
    from universal_speech_enhancement_amd.LSGAN_module import GANModule
    from universal_speech_enhancement_amd.gan.ncsnpp_wrapper import NCSNPP_Wrapper
    g = dict(np.load(os.path.join(golden_dir, "refine.npz")))
    sd_np = tw.make_state_dict(int(g["weights_seed"]), **tw.REFINE)
    w = NCSNPP_Wrapper(n_fft=1022, hop_length=160, num_frames=480, precision=prec)
    missing, unexpected = w.net.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True), None
    out = w.net(torch.from_numpy(g["x"]).cuda())
    _check(_relmax(out, torch.from_numpy(g["out"])), tol, "refine generator", prec)
    mod = GANModule(G=w)
    batch = mod.predict_step({"perturbed": torch.from_numpy(g["wav"]).cuda()})
    assert batch["fake"].shape == g["fake"].shape
    _check(_relmax(batch["fake"], torch.from_numpy(g["fake"])), tol_wav, "refine waveform", prec)
    with pytest.raises(UseHipError):
        w.net(torch.from_numpy(g["x"]))                       # CPU tensors: no fallback
    with pytest.raises(ValueError):
        w.net(torch.from_numpy(g["x"]).cuda().repeat(1, 2, 1, 1))   # a discriminative network takes Y alone


@pytest.mark.parametrize("prec,tol", [("fp32", 5e-4), ("bf16", lp.refine_bound("bf16", 1.25)),   # bf16: 1.25 x the reference's own error on this input (tests/lowprec.py)
                                      ("fp16", lp.refine_bound("fp16", 1.25))])  # fp16: the bf16 figure / 4 (tests/lowprec.py), x 1.25
def test_refine_generator_long_sequence_attention(prec, tol):
    """T' = 128: the bottleneck of the 4-level refine generator is 64 x 16 = 1024 tokens, which takes the GEMM form of the
    attention core (scores and P.V as implicit GEMMs + row softmax; fp32: both GEMMs on conv_sk, 16 bit: on conv_kernel; stage by stage
    in tests/test_hip_attention_gemm.py).  Against the CPU oracle."""
    from universal_speech_enhancement_amd.sgmse.backbones.ncsnpp import NCSNpp
    sd_np = tw.make_state_dict(4321, **tw.REFINE)
    sd = {k: torch.from_numpy(v) for k, v in sd_np.items()}
    Y = torch.from_numpy(tnoise.complex_normal(31, "Y", (1, 1, 512, 128))) * 0.5
    with torch.no_grad():
        ref = no.ncsnpp_forward(sd, Y, None, ch_mult=tw.REFINE["ch_mult"], num_res_blocks=1, discriminative=True)
    net = NCSNpp(discriminative=True, precision=prec)
    net.load_state_dict(sd, strict=True)
    out = net(Y.cuda())
    _check(_relmax(out, ref), tol, "refine generator, 1024-token attention", prec)


def test_packed_weight_file_round_trip(tmp_path, golden_dir, engines, sd_np):
    """an engine started from a packed weight file gives the same score as one fed the state dict; files for
    another precision / configuration or with a damaged payload are refused."""
    from universal_speech_enhancement_amd.hip_engine import HipScoreEngine
    g = dict(np.load(os.path.join(golden_dir, "forward_large.npz")))
    x = torch.from_numpy(g["x"]).cuda()
    t = torch.from_numpy(g["t_a"]).cuda()
    path = str(tmp_path / "large_bf16.usehip")
    engines["bf16"].save_weight_blob(path)                    # from the committed device blob
    e = HipScoreEngine(precision="bf16")
    e.load_weight_blob(path)
    a = engines["bf16"].score(x[:, 0:1].contiguous(), x[:, 1:2].contiguous(), t)
    b = e.score(x[:, 0:1].contiguous(), x[:, 1:2].contiguous(), t)
    assert torch.equal(a, b)
    e.close()
    e32 = HipScoreEngine(precision="fp32")
    with pytest.raises(UseHipError):
        e32.load_weight_blob(path)                            # packed for bf16
    e32.close()
    raw = bytearray(open(path, "rb").read())
    raw[len(raw) // 2] ^= 0xFF
    bad = str(tmp_path / "bad.usehip")
    open(bad, "wb").write(bytes(raw))
    e2 = HipScoreEngine(precision="bf16")
    with pytest.raises(UseHipError):
        e2.load_weight_blob(bad)                              # checksum
    with pytest.raises(UseHipError):
        e2.load_weight_blob(str(tmp_path / "missing.usehip"))
    e2.close()


def test_spectrogram_glue_kernels_match_torch():
    """use_spec_fwd / use_spec_back = spec_fwd + pad_spec / spec_back of the reference (model_wrapper.py:92-103)."""
    from universal_speech_enhancement_amd.hip_engine import spec_compress_pad, spec_decompress_crop
    wav = torch.from_numpy(tnoise.synth_noisy_speech(3, 9000, seed=5))
    S = so.stft(wav)
    S[0, 3, 5] = 0                                            # |z| = 0 stays 0
    ref = so.pad_spec(so.spec_fwd(S).unsqueeze(1))
    Y = spec_compress_pad(S.cuda(), 0.15, 0.5)
    assert Y.shape == ref.shape and _relmax(Y, ref) < 1e-6 and float(Y[0, 0, 3, 5].abs()) == 0.0
    assert float(Y[..., S.shape[2]:].abs().max()) == 0.0
    back = spec_decompress_crop(Y, S.shape[2], 0.15, 0.5)
    assert _relmax(back, S) < 1e-5
    full = spec_decompress_crop(Y, Y.shape[3], 0.15, 0.5)
    assert _relmax(full, so.spec_back(ref.squeeze(1))) < 1e-5
    with pytest.raises(UseHipError):
        spec_compress_pad(S, 0.15, 0.5)                       # CPU tensor


def test_odd_widths_at_the_bottom_of_the_unet_fp32(engines, sd_np):
    """T' = 192 = 3 x 64: feature-map widths 192, 96, 48, 24, 12, 6, 3 -- partially filled tiles in every conv kernel
    (conv_v4 at 512x192, conv_v2 at 48 / 24 columns, conv_kernel at 12 / 6 / 3) and odd FIR sizes.  Against the CPU oracle."""
    x = torch.from_numpy(tnoise.complex_normal(21, "x", (1, 1, 512, 192))) * 0.5
    y = torch.from_numpy(tnoise.complex_normal(21, "y", (1, 1, 512, 192))) * 0.5
    t = torch.tensor([0.37])
    sd = {k: torch.from_numpy(v) for k, v in sd_np.items()}
    with torch.no_grad():
        ref = no.ncsnpp_forward(sd, torch.cat([x, y], dim=1), t)
    out = engines["fp32"].score(x.cuda(), y.cuda(), t.cuda())
    err = _relmax(out, -ref)
    assert err < 5e-4, err


def test_subbatch_pipelining_is_a_pure_rescheduling(sd_np):
    """Batches of >= 4 items run as staggered sub-batches on separate streams: bit-identical to the unsplit evaluation."""
    from universal_speech_enhancement_amd.hip_engine import HipScoreEngine, set_option
    x = torch.from_numpy(tnoise.complex_normal(5, "x", (7, 1, 512, 64))).cuda() * 0.5
    y = torch.from_numpy(tnoise.complex_normal(5, "y", (7, 1, 512, 64))).cuda() * 0.5
    t = torch.linspace(0.9, 0.1, 7).cuda()
    outs = []
    try:
        for n in (1, 2, 3):                                  # 7 items: unsplit, 4 + 3, 3 + 2 + 2 (three streams: the default since round 5)
            set_option("subbatch", n)
            e = HipScoreEngine(precision="bf16")
            e.load_state_dict(sd_np)
            outs.append(e.score(x, y, t).clone())
            e.close()
    finally:
        set_option("subbatch", -1)
    assert torch.isfinite(torch.view_as_real(outs[0])).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_intermediate_taps_match_oracle_fp32(golden_dir, engines, sd_np):
    g = dict(np.load(os.path.join(golden_dir, "forward_large.npz")))
    x = torch.from_numpy(g["x"])
    t = torch.from_numpy(g["t_b"])
    taps = {}
    with torch.no_grad():
        no.ncsnpp_forward(no.to_torch(sd_np), x, t, taps=taps)
    xc = x.cuda()
    engines["fp32"].score(xc[:, 0:1].contiguous(), xc[:, 1:2].contiguous(), t.cuda())
    for name in ("h_in", "pre_attn", "post_attn", "pyramid"):
        got = engines["fp32"].debug_tensor(name).permute(0, 3, 1, 2)
        assert _relmax(got, taps[name]) < 5e-4, name


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_input_convolution_16bit_modes_match_the_oracle(golden_dir, engines, sd_np, prec):
    """conv_in_split_kernel (16-bit storage modes: the fp32 input convolution as a split-bf16 contraction, x w = xh wh + xh wl +
    xl wh) against the CPU oracle's fp32 convolution of the same input, per element: the rounding of the stored output (u |want|), the
    split's dropped terms (< 2^-16 S, S = conv(|x4|, |w|) + |bias|) and the fp32 accumulation of the kernel (K = 108) and of the oracle
    itself (K = 36), 2 x 2^-24 sqrt(K) S each - the bound tests/test_hip_input_head_kernels.py derives and holds launch by launch against
    float64; here on the 512 x 64 map of the whole network."""
    g = dict(np.load(os.path.join(golden_dir, "forward_large.npz")))
    x = torch.from_numpy(g["x"]); t = torch.from_numpy(g["t_b"])
    taps = {}
    with torch.no_grad():
        no.ncsnpp_forward(no.to_torch(sd_np), x, t, taps=taps)
    xc = x.cuda()
    engines[prec].score(xc[:, 0:1].contiguous(), xc[:, 1:2].contiguous(), t.cuda())
    got = engines[prec].debug_tensor("h_in").permute(0, 3, 1, 2).cpu()
    want = taps["h_in"]
    ulp = 2.0 ** -8 if prec == "bf16" else 2.0 ** -11
    err = (got - want).abs()
    sd = no.to_torch(sd_np)
    x4 = torch.cat([p for k in range(x.shape[1]) for p in (x[:, [k]].real, x[:, [k]].imag)], dim=1) * 2 - 1.0
    S = torch.nn.functional.conv2d(x4.double().abs(), sd["all_modules.3.weight"].double().abs(), sd["all_modules.3.bias"].double().abs(), padding=1)
    bound = ulp * want.abs() + (2.0 ** -16 + 2 * 2.0 ** -24 * (math.sqrt(108) + math.sqrt(36))) * S
    print(f"[measured] h_in {prec}: worst err / bound {float((err / bound).max()):.3f} (max err {float(err.max()):.3g}; the bound was ulp |want| + 2e-4, now + {float(bound.max() - (ulp * want.abs()).max()):.2g} at most)")
    assert float((err / bound).max()) <= 1, float(err.max())


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_input_convolution_walk_length_changes_nothing_but_the_statistics_order(engines, prec):
    """conv_in_split_kernel walks `tiles / conv_in_wgs` tiles per workgroup with the next tile's halo prefetched behind the current tile's
    MFMAs and stores (round 5).  The walk length must not change a single stored value (h_in bit-identical for 512 / 256 / 37 / 1 workgroups
    per item: walks of 1, 2, 14 and all 512 tiles at T' = 128), and the score may move only by the summation order of the GroupNorm totals."""
    from universal_speech_enhancement_amd.hip_engine import set_option
    eng = engines[prec]
    B, Tp = 3, 128
    x = torch.from_numpy(tnoise.complex_normal(5, "cx", (B, 1, 512, Tp))).cuda() * 0.7
    y = torch.from_numpy(tnoise.complex_normal(5, "cy", (B, 1, 512, Tp))).cuda() * 0.7
    t = torch.tensor([0.8, 0.3, 0.05], device="cuda")
    h, sc = {}, {}
    try:
        for wgs in (512, 256, 37, 1):
            set_option("conv_in_wgs", wgs)
            eng.plan(B, Tp)
            sc[wgs] = eng.score(x, y, t).clone()
            h[wgs] = eng.debug_tensor("h_in").clone()
    finally:
        set_option("conv_in_wgs", 256)
    assert torch.isfinite(h[512].float()).all() and float(h[512].float().abs().max()) > 0
    for wgs in (256, 37, 1):
        assert torch.equal(h[wgs], h[512]), wgs
        d = float((sc[wgs] - sc[512]).abs().max() / sc[512].abs().max())
        assert d < lp.fwd_bound(prec), (wgs, d)      # two valid 16-bit evaluations differ by less than either may differ from the fp32 oracle


def test_option_change_after_plan_is_an_error_code_not_a_dead_process(sd_np):
    """VERDICT r5 #6 / ADVICE r5: options that size plan buffers (conv_in_wgs, stats_part, gn_inline, subbatch*) are read at use_plan.  The
    Python wrapper re-plans on every call; a C caller that changes one between use_plan and use_score / use_sample used to overflow the
    workspace arena (round 4) or abort() the host process (round 5).  Now: a negative code with a message in use_last_error(), the
    handle stays usable, and after use_plan the same input gives the same result.  Straight through the C ABI."""
    import ctypes as C
    from universal_speech_enhancement_amd import _lib
    from universal_speech_enhancement_amd.hip_engine import HipScoreEngine, set_option, _stream_ptr
    L = _lib.lib()
    eng = HipScoreEngine(precision="bf16")
    eng.load_state_dict(sd_np)
    B, Tp = 4, 128                                            # the 512 x 128 level writes per-workgroup partial totals: sized by conv_in_wgs
    x = (torch.from_numpy(tnoise.complex_normal(7, "x_opt", (B, 1, 512, Tp))) * 0.5).cuda()
    y = (torch.from_numpy(tnoise.complex_normal(7, "y_opt", (B, 1, 512, Tp))) * 0.5).cuda()
    t = torch.full((B,), 0.4, device="cuda")
    out = torch.empty_like(x)
    call = lambda: L.use_score(eng.h, x.data_ptr(), y.data_ptr(), t.data_ptr(), out.data_ptr(), _stream_ptr(x.device))
    assert L.use_plan(eng.h, B, Tp) == 0 and call() == 0
    torch.cuda.synchronize()
    first = out.clone()
    try:
        set_option("conv_in_wgs", 2048)                       # 8 x the partial-totals buffers of the plan
        rc = call()
        assert rc < 0, "a stale plan must be refused"
        assert b"use_plan" in L.use_last_error()
        sc = _lib.UseSamplerConfig() if hasattr(_lib, "UseSamplerConfig") else None
        if sc is not None:
            assert L.use_set_sampler(eng.h, C.byref(sc)) < 0   # the sampler tables belong to the plan as well
        assert L.use_plan(eng.h, B, Tp) == 0 and call() == 0   # re-planned under the new option: fine (and a different walk length)
        torch.cuda.synchronize()
        assert torch.isfinite(torch.view_as_real(out)).all()
    finally:
        set_option("conv_in_wgs", 256)
    assert call() < 0                                         # ... and stale again after the option went back
    assert L.use_plan(eng.h, B, Tp) == 0 and call() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, first)
    eng.close()


def test_backbone_interface_returns_network_output(golden_dir, sd_np):
    from universal_speech_enhancement_amd.sgmse.backbones import BackboneRegistry
    g = dict(np.load(os.path.join(golden_dir, "forward_large.npz")))
    net = BackboneRegistry.get_by_name("ncsnpplarge")(input_channels=4, precision="fp32")
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
    out = net(torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["t_a"]).cuda())
    assert out.shape == (2, 1, 512, 64) and out.dtype == torch.complex64
    assert _relmax(out, g["out_a"]) < 5e-4


@pytest.mark.parametrize("corr", ["none", "langevin", "ald"])
def test_sde_update_kernels_match_reference_sampler(golden_dir, corr):
    """Seam path: reference-style loop over the registries with an analytic score_fn; every update runs in
    use_sde_* kernels; compared with the reference's own sampler output (golden)."""
    from universal_speech_enhancement_amd.sgmse import sampling
    from universal_speech_enhancement_amd.sgmse.sdes import OUVESDE
    g = dict(np.load(os.path.join(golden_dir, f"sampler_rd_{corr}.npz")))
    Y, A = torch.from_numpy(g["Y"]).cuda(), torch.from_numpy(g["A"]).cuda()
    draws = torch.from_numpy(tnoise.sampler_noise(int(g["noise_seed"]), int(g["n_draws"]), tuple(Y.shape))).cuda()

    def score_fn(x, t, score_conditioning=None, sde_input=None):
        return -(x - 0.8 * sde_input) / (0.1 + t[:, None, None, None] ** 2) + 0.05 * A * torch.tanh(x.abs())

    sde = OUVESDE(); sde.N = int(g["N"])
    x, nfe = sampling.get_pc_sampler("reverse_diffusion", corr, sde=sde, score_fn=score_fn, y=Y, eps=float(g["eps"]),
                                     snr=float(g["snr"]), corrector_steps=int(g["corrector_steps"]), conditioning=[Y],
                                     noise=draws)()
    assert nfe == int(g["nfe"])
    np.testing.assert_allclose(x.cpu().numpy(), g["x"], rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("corr", ["none", "langevin"])
def test_euler_maruyama_kernels_match_reference_sampler(golden_dir, corr):
    """Row a8: the Euler-Maruyama update kernel (seam path) against the reference's own sampler output."""
    from universal_speech_enhancement_amd.sgmse import sampling
    from universal_speech_enhancement_amd.sgmse.sdes import OUVESDE
    g = dict(np.load(os.path.join(golden_dir, f"sampler_em_{corr}.npz")))
    Y, A = torch.from_numpy(g["Y"]).cuda(), torch.from_numpy(g["A"]).cuda()
    draws = torch.from_numpy(tnoise.sampler_noise(int(g["noise_seed"]), int(g["n_draws"]), tuple(Y.shape))).cuda()

    def score_fn(x, t, score_conditioning=None, sde_input=None):
        return -(x - 0.8 * score_conditioning[0]) / (0.1 + t[:, None, None, None] ** 2) + 0.05 * A * torch.tanh(x.abs())

    sde = OUVESDE(); sde.N = int(g["N"])
    x, nfe = sampling.get_pc_sampler("euler_maruyama", corr, sde=sde, score_fn=score_fn, y=Y, eps=float(g["eps"]),
                                     snr=float(g["snr"]), corrector_steps=int(g["corrector_steps"]), conditioning=[Y],
                                     noise=draws)()
    assert nfe == int(g["nfe"])
    np.testing.assert_allclose(x.cpu().numpy(), g["x"], rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("pred", ["reverse_diffusion", "euler_maruyama"])
def test_probability_flow_update_kernels_match_reference_sampler(golden_dir, pred):
    """probability_flow=True through the registries' seam path: accepted and - as in the reference, whose Predictor drops the flag
    (predictors.py:17) - without effect on the updates; against the reference's own sampler output with the flag set."""
    from universal_speech_enhancement_amd.sgmse import sampling
    from universal_speech_enhancement_amd.sgmse.sdes import OUVESDE
    g = dict(np.load(os.path.join(golden_dir, f"sampler_pf_{pred}.npz")))
    Y, A = torch.from_numpy(g["Y"]).cuda(), torch.from_numpy(g["A"]).cuda()
    draws = torch.from_numpy(tnoise.sampler_noise(int(g["noise_seed"]), int(g["n_draws"]), tuple(Y.shape))).cuda()

    def score_fn(x, t, *args, score_conditioning=None, sde_input=None):
        return -(x - 0.8 * Y) / (0.1 + t[:, None, None, None] ** 2) + 0.05 * A * torch.tanh(x.abs())

    sde = OUVESDE(); sde.N = int(g["N"])
    x, nfe = sampling.get_pc_sampler(pred, "langevin", sde=sde, score_fn=score_fn, y=Y, eps=float(g["eps"]), snr=float(g["snr"]),
                                     corrector_steps=int(g["corrector_steps"]), probability_flow=True, conditioning=[Y], noise=draws)()
    assert nfe == int(g["nfe"])
    np.testing.assert_allclose(x.cpu().numpy(), g["x"], rtol=2e-4, atol=2e-5)


def test_euler_maruyama_equals_reverse_diffusion_update():
    """For the OUVE SDE the two predictors are the same map up to rounding (f dt, g sqrt(dt))."""
    from universal_speech_enhancement_amd.sgmse.sampling import _sde_engine
    from universal_speech_enhancement_amd.sgmse.sdes import OUVESDE
    eng = _sde_engine(OUVESDE(), "cuda")
    sh = (2, 1, 32, 16)
    x, y, s, z = (torch.from_numpy(tnoise.complex_normal(5, k, sh)).cuda() for k in "xysz")
    a, am = eng.sde_predictor("reverse_diffusion", 0.4, 30, x, y, s, noise=z)
    b, bm = eng.sde_predictor("euler_maruyama", 0.4, 30, x, y, s, noise=z)
    assert torch.allclose(a, b, rtol=1e-5, atol=1e-6) and torch.allclose(am, bm, rtol=1e-5, atol=1e-6)
    ref, ref_mean = so.predictor_euler_maruyama(x.cpu(), torch.full((2,), 0.4), y.cpu(), lambda xx, tt: s.cpu(), 30,
                                                so.NoiseSource(replay=[z.cpu()]))
    assert torch.allclose(b.cpu(), ref, rtol=1e-5, atol=1e-6) and torch.allclose(bm.cpu(), ref_mean, rtol=1e-5, atol=1e-6)


def test_device_philox_noise_statistics():
    from universal_speech_enhancement_amd.sgmse.sampling import _sde_engine
    from universal_speech_enhancement_amd.sgmse.sdes import OUVESDE
    eng = _sde_engine(OUVESDE(), "cuda")
    y = torch.zeros(4, 1, 512, 64, dtype=torch.complex64, device="cuda")
    std1 = float(so.ouve_std(torch.ones(1)))
    z1 = eng.sde_prior(y, seed=7) / std1
    z2 = eng.sde_prior(y, seed=7) / std1
    z3 = eng.sde_prior(y, seed=8) / std1
    assert torch.equal(z1, z2) and not torch.equal(z1, z3)
    r = torch.view_as_real(z1)
    assert abs(float(r.mean())) < 5e-3 and abs(float(r.var()) - 0.5) < 5e-3
    assert abs(float((r[..., 0] * r[..., 1]).mean())) < 5e-3
    assert abs(float((r ** 4).mean()) / float(r.var()) ** 2 - 3.0) < 0.1       # Gaussian kurtosis


def _e2e(golden_dir, name, sd_np, precision, use_graph):
    g = dict(np.load(os.path.join(golden_dir, name)))
    wav = torch.from_numpy(g["wav"]).cuda()
    Tp = (1 + wav.shape[1] // 160 + 63) // 64 * 64
    draws = torch.from_numpy(tnoise.sampler_noise(int(g["noise_seed"]), int(g["n_draws"]), (wav.shape[0], 1, 512, Tp))).cuda()
    m = _score_model(sd_np, precision, use_graph=use_graph)
    out = m.sample({"perturbed": wav}, N=int(g["N"]), corrector_steps=int(g["corrector_steps"]), snr=float(g["snr"]),
                   noise=draws)["enhanced"]
    return out.cpu(), torch.from_numpy(g["enhanced"])


def test_fused_sampler_fp32_matches_reference_end_to_end(golden_dir, sd_np):
    out_graph, ref = _e2e(golden_dir, "sample_e2e.npz", sd_np, "fp32", True)
    assert out_graph.shape == ref.shape
    assert _relmax(out_graph, ref) < 2e-3
    out_eager, _ = _e2e(golden_dir, "sample_e2e.npz", sd_np, "fp32", False)
    assert torch.equal(out_graph, out_eager), "hipGraph replay must be bit-identical to eager launches"


@pytest.mark.parametrize("prec,tol", [("bf16", lp.chain_bound("bf16", "wav", "relmax")), ("fp16", lp.chain_bound("fp16", "wav", "relmax"))])   # tests/lowprec.py
def test_fused_sampler_16bit_end_to_end_tolerance(golden_dir, sd_np, prec, tol):
    out, ref = _e2e(golden_dir, "sample_e2e.npz", sd_np, prec, True)
    err = _relmax(out, ref)
    _check(err, tol, "sample_e2e waveform", prec)


@pytest.mark.parametrize("predictor,corrector", [("euler_maruyama", "langevin"), ("reverse_diffusion", "ald"), ("euler_maruyama", "none")])
def test_fused_sampler_other_predictors_and_correctors_match_the_oracle(sd_np, predictor, corrector):
    """The fused loop (use_sample) with the network in it for the sampler variants the reference goldens cover only with an
    analytic score: euler_maruyama (predictors.py:40-52) and annealed Langevin (correctors.py:66-98).  One 0.4 s utterance
    (T' = 64), N = 3, fp32 storage, same injected noise, against the CPU oracle's ScoreModel.sample (pinned to the reference
    by tests/test_oracle_golden.py)."""
    from universal_speech_enhancement_amd.sgmse.model_wrapper import ScoreModel
    torch.set_num_threads(usable_cores())
    L, N = 9600, 3
    wav = torch.from_numpy(tnoise.synth_noisy_speech(1, L, seed=99))
    n_draws = 1 + N * (2 if corrector != "none" else 1)
    draws = tnoise.sampler_noise(77, n_draws, (1, 1, 512, 64))
    sd = no.to_torch(sd_np)
    with torch.no_grad():
        ref, _, _, nfe = so.score_model_sample(lambda xx, t: no.ncsnpp_forward(sd, xx, t), wav, N=N, predictor=predictor, corrector=corrector,
                                               corrector_steps=1, snr=0.5, noise=so.NoiseSource(replay=[torch.from_numpy(d) for d in draws]))
    m = ScoreModel(backbone="ncsnpplarge", sde="ouve", t_eps=3e-2, condition="noisy", n_fft=1022, hop_length=160, num_frames=512,
                   window="hann", sde_input="noisy", predictor=predictor, corrector=corrector, precision="fp32", use_graph=True)
    m.score_net.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
    out = m.sample({"perturbed": wav.cuda()}, N=N, corrector_steps=1, snr=0.5, noise=torch.from_numpy(draws).cuda())["enhanced"]
    assert nfe == N * (2 if corrector != "none" else 1)
    _check(_relmax(out, ref), 2e-3, "fused sampler vs oracle", predictor, corrector)


def test_cfg1_plumbing_config_matches_reference(golden_dir, sd_np):
    """BASELINE configs[0]: one 2 s utterance, 5 PC steps (reverse_diffusion + langevin)."""
    out, ref = _e2e(golden_dir, "sample_cfg1.npz", sd_np, "fp32", True)
    assert _relmax(out, ref) < 2e-3


def test_seam_path_equals_fused_path_fp32(golden_dir, sd_np):
    """Python-driven loop over the registries (score_fn = ScoreModel.forward -> use_score) vs use_sample."""
    from universal_speech_enhancement_amd.sgmse import sampling
    g = dict(np.load(os.path.join(golden_dir, "sample_e2e.npz")))
    m = _score_model(sd_np, "fp32")
    Y = m._spectrogram(torch.from_numpy(g["wav"]).cuda())
    draws = torch.from_numpy(tnoise.sampler_noise(99, 1 + 2 * 2, tuple(Y.shape))).cuda()
    fused, n1 = m.get_pc_sampler("reverse_diffusion", "ald", Y, N=2, corrector_steps=1, snr=0.5, conditioning=[Y], noise=draws)()
    sde = m.sde.copy(); sde.N = 2
    seam, n2 = sampling.get_pc_sampler("reverse_diffusion", "ald", sde=sde, score_fn=lambda x, t, score_conditioning=None, sde_input=None: m(x, t, score_conditioning, sde_input),
                                       y=Y, eps=m.t_eps, snr=0.5, corrector_steps=1, conditioning=[Y], noise=draws)()
    assert n1 == n2 == 4
    assert _relmax(seam, fused) < 1e-5


def test_full_size_properties_cfg2_bf16(sd_np):
    """BASELINE configs[1] shape (8 x 4 s) with N=2: size-independent properties -- determinism under a fixed seed,
    seed sensitivity, finiteness, and batch-item independence for a sampler without batch coupling (ALD)."""
    m = _score_model(sd_np, "bf16", corrector="ald")
    wav = torch.from_numpy(tnoise.synth_noisy_speech(8, 96000)).cuda()
    a = m.sample({"perturbed": wav}, N=2, seed=11)["enhanced"]
    b = m.sample({"perturbed": wav}, N=2, seed=11)["enhanced"]
    c = m.sample({"perturbed": wav}, N=2, seed=12)["enhanced"]
    assert a.shape == (8, 96000) and torch.isfinite(a).all()
    assert torch.equal(a, b) and not torch.equal(a, c)
    Y = m._spectrogram(wav)
    assert Y.shape == (8, 1, 512, 640)
    draws = torch.from_numpy(tnoise.sampler_noise(3, 5, (8, 1, 512, 640))).cuda()
    full, _ = m.get_pc_sampler("reverse_diffusion", "ald", Y, N=2, conditioning=[Y], noise=draws)()
    Y2 = Y[2:4].contiguous()
    part, _ = m.get_pc_sampler("reverse_diffusion", "ald", Y2, N=2, conditioning=[Y2], noise=draws[:, 2:4].contiguous())()
    assert torch.equal(full[2:4], part), "items must not interact when the corrector has no batch coupling"


def test_langevin_step_couples_the_local_batch_like_the_reference(sd_np):
    """LangevinCorrector averages norms over the batch (correctors.py:55-57): check against the oracle formula."""
    from universal_speech_enhancement_amd.sgmse.sampling import _sde_engine
    from universal_speech_enhancement_amd.sgmse.sdes import OUVESDE
    eng = _sde_engine(OUVESDE(), "cuda")
    sh = (3, 1, 64, 32)
    x, g, z = (torch.from_numpy(tnoise.complex_normal(17, k, sh)) for k in "xgz")
    g = g * torch.tensor([1.0, 5.0, 0.2]).view(3, 1, 1, 1)
    got, got_mean = eng.sde_corrector("langevin", 0.5, 0.5, x.cuda(), g.cuda(), noise=z.cuda())
    ref, ref_mean = so.corrector_langevin(x, torch.full((3,), 0.5), None, lambda xx, tt: g, 0.5, 1, so.NoiseSource(replay=[z]))
    assert torch.allclose(got.cpu(), ref, rtol=1e-5, atol=1e-6) and torch.allclose(got_mean.cpu(), ref_mean, rtol=1e-5, atol=1e-6)


def test_edge_cases_and_error_behaviour(sd_np, engines):
    m = _score_model(sd_np, "bf16", corrector="none")
    # ragged length: 0.25 s + 7 samples -> T = 38 frames -> padded to 64; B = 1; N = 1
    wav = torch.from_numpy(tnoise.synth_noisy_speech(1, 6007)).cuda()
    out = m.sample({"perturbed": wav}, N=1)["enhanced"]
    assert out.shape == (1, 6007) and torch.isfinite(out).all()
    with pytest.raises(UseHipError):
        engines["bf16"].score(torch.zeros(1, 1, 512, 64, dtype=torch.complex64), torch.zeros(1, 1, 512, 64, dtype=torch.complex64), torch.ones(1))
    with pytest.raises(TypeError):
        engines["bf16"].score(torch.zeros(1, 1, 512, 64, device="cuda"), torch.zeros(1, 1, 512, 64, device="cuda"), torch.ones(1))
    with pytest.raises(UseHipError, match="multiple of 64"):
        z = torch.zeros(1, 1, 512, 60, dtype=torch.complex64, device="cuda")
        engines["bf16"].score(z, z, torch.ones(1))
    with pytest.raises(ValueError):
        z = torch.zeros(1, 1, 256, 64, dtype=torch.complex64, device="cuda")
        engines["bf16"].score(z, z, torch.ones(1))


def test_predict_step_writes_trimmed_wavs(tmp_path, sd_np):
    from scipy.io import wavfile
    from universal_speech_enhancement_amd.SGMSE_module import SGMSEModule
    mod = SGMSEModule(Score=_score_model(sd_np, "bf16", corrector="none"), sampler_kwargs=dict(N=1))
    src, dst = str(tmp_path / "in"), str(tmp_path / "out")
    wav = torch.from_numpy(tnoise.synth_noisy_speech(2, 8000)).cuda()
    batch = {"perturbed": wav, "name": ["a", "b"], "sample_length": torch.tensor([8000, 5000], dtype=torch.int32),
             "sampling_rate": [24000, 24000], "audio_path": [f"{src}/x/a.wav", f"{src}/b.wav"], "data_folder": src,
             "target_folder": dst}
    out = mod.predict_step(batch, 0)
    assert out["enhanced"].shape == (2, 8000)
    sr, a = wavfile.read(f"{dst}/x/a.wav"); _, b = wavfile.read(f"{dst}/b.wav")
    # the reference's sf.write default: 16-bit PCM, round(x * 32767)
    assert sr == 24000 and a.shape == (8000,) and b.shape == (5000,) and a.dtype == np.int16
    want = np.clip(np.rint(out["enhanced"][1, :5000].cpu().numpy().astype(np.float64) * 32767.0), -32768, 32767)
    np.testing.assert_array_equal(b.astype(np.float64), want)
    mod.wav_subtype = "FLOAT"
    out = mod.predict_step(batch, 0)
    _, b = wavfile.read(f"{dst}/b.wav")
    assert b.dtype == np.float32
    np.testing.assert_array_equal(b, out["enhanced"][1, :5000].cpu().numpy())


def test_weight_blob_broadcast_equivalence(engines, sd_np):
    """Stand-in for the RCCL weight broadcast on one GPU: a second handle that only *receives* rank 0's packed blob
    (alloc_weight_blob + device copy into the aliased view) must reproduce rank 0's outputs bit for bit."""
    from universal_speech_enhancement_amd.hip_engine import HipScoreEngine
    src = engines["bf16"]
    dst = HipScoreEngine(precision="bf16")
    dst.alloc_weight_blob()
    a, b = src.weight_blob(), dst.weight_blob()
    assert a.dtype == torch.uint8 and a.shape == b.shape and a.data_ptr() != b.data_ptr()
    b.copy_(a)                                   # what dist.broadcast does on the non-root ranks
    assert dst.weight_blob().data_ptr() == b.data_ptr(), "the view must alias the library's blob, not a copy"
    x = torch.from_numpy(tnoise.complex_normal(3, "bx", (1, 1, 512, 64))).cuda()
    y = torch.from_numpy(tnoise.complex_normal(3, "by", (1, 1, 512, 64))).cuda()
    t = torch.tensor([0.4], device="cuda")
    assert torch.equal(src.score(x, y, t), dst.score(x, y, t))
    dst.close()


def test_minibatch_sampler_and_enhance(sd_np):
    """``ScoreModel.get_pc_sampler(minibatch=...)`` (reference model_wrapper.py:220-236): the batch is sampled in slices and
    concatenated; with a corrector without batch coupling each slice must equal the corresponding rows of the whole-batch
    run under the same injected noise.  ``enhance`` (legacy keyword surface, sgmse/model.py:351-402): peak-normalises,
    samples, rescales."""
    m = _score_model(sd_np, "fp32", corrector="ald")
    wav = torch.from_numpy(tnoise.synth_noisy_speech(3, 9600, seed=9)).cuda()
    Y = m._spectrogram(wav)
    draws = torch.from_numpy(tnoise.sampler_noise(5, 1 + 2 * 2, tuple(Y.shape))).cuda()
    full, nfe = m.get_pc_sampler("reverse_diffusion", "ald", Y, N=2, corrector_steps=1, snr=0.5, conditioning=[Y], noise=draws)()
    assert nfe == 4
    parts = []
    for lo, hi in ((0, 2), (2, 3)):                           # what minibatch=2 does, with the matching noise rows
        Ym = Y[lo:hi].contiguous()
        p, _ = m.get_pc_sampler("reverse_diffusion", "ald", Ym, N=2, corrector_steps=1, snr=0.5, conditioning=[Ym],
                                noise=draws[:, lo:hi].contiguous())()
        parts.append(p)
    assert _relmax(torch.cat(parts), full) < 1e-5
    mb, ns = m.get_pc_sampler("reverse_diffusion", "ald", Y, N=2, minibatch=2, corrector_steps=1, snr=0.5, conditioning=[Y], seed=3)()
    assert mb.shape == Y.shape and ns == [4, 4] and torch.isfinite(torch.view_as_real(mb)).all()
    # enhance(): [1, L] waveform in, 1-D CPU waveform out, scale restored
    y1 = wav[:1] * 0.5
    z = torch.from_numpy(tnoise.sampler_noise(6, 1 + 2 * 2, (1, 1, 512, 64))).cuda()
    x_hat = m.enhance(y1, predictor="reverse_diffusion", corrector="ald", N=2, corrector_steps=1, snr=0.5, noise=z)
    assert x_hat.shape == (9600,) and not x_hat.is_cuda and torch.isfinite(x_hat).all()
    nf = y1.abs().max().item()                                # (division by the Python float, as enhance() does: a tensor divisor
    ref = m.sample({"perturbed": y1 / nf}, N=2, corrector_steps=1, snr=0.5, noise=z)   # differs in the last bit of some samples)
    assert _relmax(x_hat, ref["enhanced"][0].cpu() * nf) < 1e-6
    x_hat2, nfe2, rtf = m.enhance(y1, corrector="ald", N=1, timeit=True)
    assert nfe2 == 2 and rtf > 0
    X, Yc, T_orig, nf = m.enhance(y1, corrector="ald", N=1, return_stft=True)
    assert X.shape == (512, 64) and Yc.shape == (512, 64) and T_orig == 9600 and abs(nf - float(y1.abs().max())) < 1e-6


def test_cfg2_shape_score_all_precisions_match_oracle(sd_np):
    """BASELINE configs[1] map sizes against the CPU oracle: one score evaluation at [B, ., 512, 640] -- conv_v4 at its real
    grid (20 tiles per row), the 80-token attention, and (B = 8) the 3+3+2 sub-batch split -- in fp32 storage AND (round 6, VERDICT r5
    #2) in the two 16-bit modes, i.e. the kernels that exist only in 16-bit form at this size (pyr_conv_ws_kernel's rolling halo down
    512-row strips, fir_down_strip_kernel<., 8>, conv_in_split_kernel's ~10-tile walk, conv_v4<bf16 / f16> on 1 920-tile grids) directly
    under the oracle (ncsnpp.py:324-501), not only through small-shape operator tests.  Items 0 and 1 are distinct inputs at different
    t; the other six items are copies of them, so the oracle runs on two items.  Checked per item: the score, and the `pre_attn`
    (bottleneck, after the whole down path) and `pyramid` (fp32 output pyramid before the division by t) taps."""
    from universal_speech_enhancement_amd.hip_engine import HipScoreEngine
    x2 = torch.from_numpy(tnoise.complex_normal(41, "x640", (2, 1, 512, 640))) * 0.5
    y2 = torch.from_numpy(tnoise.complex_normal(41, "y640", (2, 1, 512, 640))) * 0.5
    t2 = torch.tensor([0.71, 0.05])
    idx = [0, 1, 0, 0, 1, 1, 0, 1]                             # sub-batches 0..2, 3..5, 6..7: both inputs in the first (the one the taps show)
    sd = {k: torch.from_numpy(v) for k, v in sd_np.items()}
    torch.set_num_threads(usable_cores())
    taps = {}
    with torch.no_grad():
        ref = no.ncsnpp_forward(sd, torch.cat([x2, y2], dim=1), t2, taps=taps)
    for prec in ("fp32", "bf16", "fp16"):
        eng = HipScoreEngine(precision=prec)
        eng.load_state_dict(sd_np)
        out = eng.score(x2[idx].cuda(), y2[idx].cuda(), t2[idx].cuda()).cpu()
        got = {n: eng.debug_tensor(n).permute(0, 3, 1, 2).float().cpu() for n in ("pre_attn", "pyramid")}
        eng.close()
        assert torch.equal(out[0], out[2]) and torch.equal(out[0], out[6]) and torch.equal(out[1], out[4]) and torch.equal(out[1], out[7]), \
            "an item's result must not depend on its position in the batch / sub-batch"
        tol = 5e-4 if prec == "fp32" else lp.fwd_bound(prec, 1.25)    # a non-fixture input: 1.25 x the reference's own autocast error (tests/lowprec.py)
        for i in (0, 1):
            err = _relmax(out[i], -ref[i])
            print(f"[measured] cfg2-shape score vs oracle, {prec} item {i}: {err:.3e} (bound {tol:.3e})")
            assert err < tol, (prec, i, err)
            for n in ("pre_attn", "pyramid"):
                e = _relmax(got[n][i], taps[n][i])
                print(f"[measured] cfg2-shape tap {n} vs oracle, {prec} item {i}: {e:.3e}")
                assert e < tol, (prec, n, i, e)


def test_cfg2_sampler_16bit_drift_against_fp32(sd_np):
    """The benchmarked precision on the benchmarked workload: BASELINE configs[1] (B=8, 4 s, T'=640, N=30,
    reverse_diffusion + Langevin x1, snr 0.5 => 60 NFE) run through the HIP path under the SAME injected noise in fp32
    storage (validated against the reference elsewhere in this file), bf16 storage (configs[1]) and fp16 storage (the
    per-GPU workload of configs[4]).  Measures how far 16-bit rounding drifts through 60 chained evaluations (h/t
    amplification at t -> 0.03 included).  Bounds relative to the fp32 result: tests/lowprec.py, CHAIN_FACTOR (three statistics).  Measured values are printed
    and recorded in DESIGN.md section 2."""
    B, L, N = 8, 96000, 30
    wav = torch.from_numpy(tnoise.synth_noisy_speech(B, L, seed=1234)).cuda()
    res = {}
    for prec in ("fp32", "bf16", "fp16"):
        m = _score_model(sd_np, prec, corrector="langevin")
        Y = m._spectrogram(wav)
        assert Y.shape == (B, 1, 512, 640)
        g = torch.Generator(device="cuda").manual_seed(777)    # 61 draws x 21 MB, generated on the device, identical for every run
        draws = torch.view_as_complex(torch.randn((1 + 2 * N, B, 1, 512, 640, 2), generator=g, device="cuda") * (0.5 ** 0.5))
        X, nfe = m.get_pc_sampler("reverse_diffusion", "langevin", Y, N=N, corrector_steps=1, snr=0.5, conditioning=[Y], noise=draws)()
        assert nfe == 60
        res[prec] = (X.clone(), m._waveform(X, L).clone())
        del m, draws
        torch.cuda.empty_cache()
    Xf, wf = res["fp32"]
    for prec in ("bf16", "fp16"):
        Xb, wb = res[prec]
        assert torch.isfinite(torch.view_as_real(Xb)).all() and torch.isfinite(wb).all()
        lp.assert_chain(prec, "spec", Xb, Xf, "cfg2 drift")      # rel-L2 <= 1.75 x, 99.99th percentile <= 1.5 x, rel-max <= 3 x the reference's own chain
        lp.assert_chain(prec, "wav", wb, wf, "cfg2 drift")


def test_configs3_long_horizon_batch16_properties(sd_np):
    """BASELINE configs[3]: N = 200 reverse steps, Langevin corrector snr 0.5, batch 16 on one GPU (400 score evaluations per
    sampler call, sub-batches of 8 + 8, one captured hipGraph of ~2e5 kernel nodes).  Size-independent properties: the call
    completes, the result is finite, a replay of the graph with the same seed is bit-identical, another seed differs."""
    m = _score_model(sd_np, "bf16", corrector="langevin")
    wav = torch.from_numpy(tnoise.synth_noisy_speech(16, 96000, seed=77)).cuda()
    a = m.sample({"perturbed": wav}, N=200, corrector_steps=1, snr=0.5, seed=5)["enhanced"]
    assert a.shape == (16, 96000) and torch.isfinite(a).all()
    b = m.sample({"perturbed": wav}, N=200, corrector_steps=1, snr=0.5, seed=5)["enhanced"]
    assert torch.equal(a, b)
    c = m.sample({"perturbed": wav[:, :9600].contiguous()}, N=200, corrector_steps=1, snr=0.5, seed=6)["enhanced"]   # another plan: T' = 64
    assert c.shape == (16, 9600) and torch.isfinite(c).all()


def test_predict_cli_from_lightning_checkpoint(tmp_path, sd_np):
    """SURVEY 8f3 / README.md:176: `predict model=SGMSE_Large ckpt_path=last.ckpt data.data_folder=... data.target_folder=...`
    end to end from a Lightning-format checkpoint file -- `state_dict` under the reference's key layout
    (`Score.score_net.all_modules...`), with the optimizer / EMA / bookkeeping entries such a file carries -- through the WAV
    reader (16 kHz int16 and 24 kHz float32 inputs, i.e. with and without FFT resampling), the sampler and the WAV writer; and
    the same run from the packed weight file (`pack_checkpoint`) gives the same audio."""
    from scipy.io import wavfile
    from universal_speech_enhancement_amd import pack_checkpoint as PC
    from universal_speech_enhancement_amd import predict as P
    sd = {"Score.score_net." + k: torch.from_numpy(v) for k, v in sd_np.items()}
    ckpt = {"epoch": 7, "global_step": 12345, "pytorch-lightning_version": "2.2.0", "state_dict": sd,
            "optimizer_states": [{"state": {0: {"exp_avg": torch.zeros(3)}}, "param_groups": [{"lr": 1e-4}]}],
            "lr_schedulers": [], "loops": {}, "callbacks": {}, "hyper_parameters": {"compile": False}}
    ckpt_path = str(tmp_path / "last.ckpt")
    torch.save(ckpt, ckpt_path)
    src, dst, dst2 = tmp_path / "noisy", tmp_path / "enhanced", tmp_path / "enhanced2"
    (src / "sub").mkdir(parents=True)
    w = tnoise.synth_noisy_speech(2, 9600, seed=3)
    wavfile.write(str(src / "a.wav"), 24000, w[0].astype(np.float32))
    wavfile.write(str(src / "sub" / "b.wav"), 16000, (w[1][:6400] * 32767).astype(np.int16))     # resampled to 24 kHz on load
    common = ["model=SGMSE_Large", f"data.data_folder={src}", "model.sampler_kwargs.N=2", "model.Score.precision=fp32", "data.batch_size=2"]
    n = P.predict(P.compose(common + [f"ckpt_path={ckpt_path}", f"data.target_folder={dst}"]))
    assert n == 2
    sr_a, a = wavfile.read(str(dst / "a.wav")); sr_b, b = wavfile.read(str(dst / "sub" / "b.wav"))
    assert sr_a == sr_b == 24000 and a.shape == (9600,) and b.shape == (9600,) and np.isfinite(a).all() and np.isfinite(b).all()
    assert float(np.abs(a).max()) > 0
    packed = str(tmp_path / "large_fp32.usehip")
    PC.main([f"ckpt={ckpt_path}", f"out={packed}", "precision=fp32"])
    assert P.predict(P.compose(common + [f"ckpt_path={packed}", f"data.target_folder={dst2}"])) == 2
    _, a2 = wavfile.read(str(dst2 / "a.wav"))
    # device Philox noise with the default seed on both runs: same weights -> same samples
    assert a.dtype == np.int16
    np.testing.assert_allclose(a2.astype(np.int32), a.astype(np.int32), rtol=0, atol=1)


def test_device_stft_istft_match_torch():
    """use_stft_fwd = pad_spec(spec_fwd(torch.stft(...))) and use_istft_back = torch.istft(spec_back(...)) with the
    reference's analysis parameters (n_fft 1022, hop 160, periodic Hann, centred / reflect padding; model_wrapper.py:116-122),
    against the CPU oracle (torch.stft / torch.istft).  Tolerances relative to the reference tensor's max magnitude:
    spectrogram 2e-5 (direct fp32 sums of 1022 terms vs an fp32 FFT), waveform 2e-5; ragged lengths, T' > T padding frames
    and the square-root Hann window of the GAN generator config included."""
    from universal_speech_enhancement_amd.hip_engine import istft_decompress, stft_compress_pad
    from universal_speech_enhancement_amd.sgmse.util.spectral import get_window
    for L, wname in ((9600, "hann"), (6007, "hann"), (48000, "sqrthann")):
        wav = torch.from_numpy(tnoise.synth_noisy_speech(2, L, seed=11))
        win = get_window(wname, 1022)
        S = torch.stft(wav, n_fft=1022, hop_length=160, window=win, center=True, return_complex=True)
        ref = so.pad_spec(so.spec_fwd(S).unsqueeze(1))
        Y = stft_compress_pad(wav.cuda(), win, 1022, 160, 0.15, 0.5)
        assert Y.shape == ref.shape and Y.dtype == torch.complex64
        assert _relmax(Y, ref) < 2e-5, (L, wname, _relmax(Y, ref))
        assert float(Y[..., S.shape[2]:].abs().max()) == 0.0
        # synthesis of an arbitrary (non-STFT-consistent) spectrogram, all T' frames entering as in the reference
        X = ref * torch.from_numpy(tnoise.complex_normal(3, f"ph{L}", tuple(ref.shape))).abs().clamp(0.2, 2.0)
        wref = torch.istft(so.spec_back(X.squeeze(1)), n_fft=1022, hop_length=160, window=win, center=True, length=L)
        w = istft_decompress(X.cuda(), win, 1022, 160, L, 0.15, 0.5)
        assert w.shape == wref.shape and _relmax(w, wref) < 2e-5, (L, wname, _relmax(w, wref))
        # round trip of a consistent spectrogram gives the waveform back -- except in the last n_fft/2 samples, which the
        # all-zero padding frames T..T'-1 overlap (they enter the envelope but carry no signal: the reference behaves the same)
        back = istft_decompress(Y, win, 1022, 160, L, 0.15, 0.5).cpu()
        assert _relmax(back[:, : L - 600], wav[:, : L - 600]) < 1e-4
        assert _relmax(back, torch.istft(so.spec_back(Y.cpu().squeeze(1)), n_fft=1022, hop_length=160, window=win, center=True, length=L)) < 2e-5
    with pytest.raises(UseHipError):
        stft_compress_pad(torch.zeros(1, 300, device="cuda"), get_window("hann", 1022), 1022, 160, 0.15, 0.5)   # shorter than the reflect pad


def test_sample_with_device_stft_equals_torch_stft_path(golden_dir, sd_np):
    """ScoreModel.sample with the analysis / synthesis in libuse_hip.so vs the torch.stft / torch.istft glue: same waveform."""
    g = dict(np.load(os.path.join(golden_dir, "sample_e2e.npz")))
    wav = torch.from_numpy(g["wav"]).cuda()
    Tp = (1 + wav.shape[1] // 160 + 63) // 64 * 64
    draws = torch.from_numpy(tnoise.sampler_noise(int(g["noise_seed"]), int(g["n_draws"]), (wav.shape[0], 1, 512, Tp))).cuda()
    outs = []
    for dev in (True, False):
        m = _score_model(sd_np, "fp32")
        m.device_stft = dev
        outs.append(m.sample({"perturbed": wav}, N=int(g["N"]), corrector_steps=int(g["corrector_steps"]), snr=float(g["snr"]),
                             noise=draws)["enhanced"].cpu())
    assert _relmax(outs[0], outs[1]) < 1e-4
    assert _relmax(outs[0], torch.from_numpy(g["enhanced"])) < 2e-3


@pytest.mark.parametrize("name,arch,backbone", [("12m", tw.SMALL12M, "ncsnpp12M"), ("6m", tw.SMALL6M, "ncsnpp6M")])
@pytest.mark.parametrize("prec,tol", [("fp32", 5e-4), ("bf16", lp.fwd_bound("bf16")), ("fp16", lp.fwd_bound("fp16"))])   # 16-bit: the reference's own autocast error (tests/lowprec.py)
def test_nf96_variants_match_reference(golden_dir, name, arch, backbone, prec, tol):
    """NCSNpp12M / NCSNpp6M (nf = 96: 96 / 192 / 288-channel convolutions take the 32-channel-chunk kernels; 24 x 4, 32 x 6
    and 32 x 9 GroupNorm groups; 96-channel attention) through the backbone registry, against outputs of the reference."""
    from universal_speech_enhancement_amd.sgmse.backbones import BackboneRegistry
    g = dict(np.load(os.path.join(golden_dir, f"forward_{name}.npz")))
    sd_np = tw.make_state_dict(int(g["weights_seed"]), **arch)
    net = BackboneRegistry.get_by_name(backbone)(input_channels=4, precision=prec)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
    x = torch.from_numpy(tnoise.complex_normal(int(g["x_seed"]), "small_x", (2, 2, 512, 64))) * 0.5
    out = net(x.cuda(), torch.from_numpy(g["t"]).cuda())
    err = _relmax(out, g["out"])
    _check(err, tol, name, prec)


@pytest.mark.parametrize("sde_input", ["noisy", "denoised"])
def test_condition_denoised_matches_reference(golden_dir, sd_np, sde_input):
    """ScoreModel.sample with condition="denoised" (score conditioning = the GAN-denoised spectrogram, model_wrapper.py:285-286)
    and both choices of sde_input (:293-300; the result key follows :320-328), fused path (use_sample_cond), against outputs of
    the reference; and the seam path (Python-driven loop) agrees with the fused one."""
    from universal_speech_enhancement_amd.sgmse.model_wrapper import ScoreModel
    g = dict(np.load(os.path.join(golden_dir, "sample_denoised.npz")))
    m = ScoreModel(backbone="ncsnpplarge", sde="ouve", t_eps=3e-2, condition="denoised", n_fft=1022, hop_length=160, num_frames=512,
                   window="hann", sde_input=sde_input, predictor="reverse_diffusion", corrector="langevin", precision="fp32")
    m.score_net.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
    draws = torch.from_numpy(tnoise.sampler_noise(int(g["noise_seed"]), int(g["n_draws"]), (1, 1, 512, 64))).cuda()
    batch = {"perturbed": torch.from_numpy(g["wav"]).cuda(), "fake": torch.from_numpy(g["fake"]).cuda()}
    out = m.sample(dict(batch), N=int(g["N"]), corrector_steps=1, snr=0.5, noise=draws)
    key = "enhanced" if sde_input == "noisy" else "fake_sde_enhanced"
    assert key in out and ("fake_sde_enhanced" if sde_input == "noisy" else "enhanced") not in out
    assert _relmax(out[key], g["out_sde_" + sde_input]) < 2e-3
    # seam path: same sampler driven from Python through the registries (score_fn = ScoreModel.forward -> use_score)
    from universal_speech_enhancement_amd.sgmse import sampling
    Y, Yd = m._spectrogram(batch["perturbed"]), m._spectrogram(batch["fake"])
    ysde = Y if sde_input == "noisy" else Yd
    sde = m.sde.copy(); sde.N = int(g["N"])
    seam, _ = sampling.get_pc_sampler("reverse_diffusion", "langevin", sde=sde, y=ysde, eps=m.t_eps, snr=0.5, corrector_steps=1,
                                      score_fn=lambda x, t, score_conditioning=None, sde_input=None: m(x, t, score_conditioning, sde_input),
                                      conditioning=[Yd], noise=draws)()
    assert _relmax(m._waveform(seam, 9600), out[key]) < 1e-4
    with pytest.raises(NotImplementedError):
        m.sample({"perturbed": batch["perturbed"]}, N=1)                    # condition="denoised" without batch["fake"]


@pytest.mark.parametrize("sde_input", ["noisy", "denoised"])
def test_condition_both_matches_reference(golden_dir, sde_input):
    """ScoreModel(condition="both") -- the reference's constructor default (model_wrapper.py:26, 43-46): the 6-channel network sees
    cat[x, Y, Y_denoised] (:287-288).  fp32 against outputs of the reference: one backbone forward (use_score2), ScoreModel.sample
    through the fused loop (use_sample_cond2) for both choices of sde_input, the Python-driven seam path, and the 16-bit modes
    within their drift bounds."""
    from universal_speech_enhancement_amd.sgmse.model_wrapper import ScoreModel
    g = dict(np.load(os.path.join(golden_dir, "both.npz")))
    sd = tw.make_state_dict(int(g["weights_seed"]), **tw.LARGE_BOTH)
    assert tw.weights_checksum(sd) == str(g["weights_crc"])

    def model(prec):
        m = ScoreModel(backbone="ncsnpplarge", sde="ouve", t_eps=3e-2, condition="both", n_fft=1022, hop_length=160, num_frames=512,
                       window="hann", sde_input=sde_input, predictor="reverse_diffusion", corrector="langevin", precision=prec)
        m.score_net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        return m
    m = model("fp32")
    if sde_input == "noisy":
        fwd = m.score_net(torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["t"]).cuda())
        assert _relmax(fwd, g["fwd"]) < 5e-4
    draws = torch.from_numpy(tnoise.sampler_noise(int(g["noise_seed"]), int(g["n_draws"]), (1, 1, 512, 64))).cuda()
    batch = {"perturbed": torch.from_numpy(g["wav"]).cuda(), "fake": torch.from_numpy(g["fake"]).cuda()}
    out = m.sample(dict(batch), N=int(g["N"]), corrector_steps=1, snr=0.5, noise=draws)
    key = "enhanced" if sde_input == "noisy" else "fake_sde_enhanced"
    assert _relmax(out[key], g["out_sde_" + sde_input]) < 2e-3
    from universal_speech_enhancement_amd.sgmse import sampling
    Y, Yd = m._spectrogram(batch["perturbed"]), m._spectrogram(batch["fake"])
    sde = m.sde.copy(); sde.N = int(g["N"])
    seam, _ = sampling.get_pc_sampler("reverse_diffusion", "langevin", sde=sde, y=Y if sde_input == "noisy" else Yd, eps=m.t_eps, snr=0.5,
                                      corrector_steps=1, conditioning=[Y, Yd], noise=draws,
                                      score_fn=lambda x, t, score_conditioning=None, sde_input=None: m(x, t, score_conditioning, sde_input))()
    assert _relmax(m._waveform(seam, 9600), out[key]) < 1e-4
    for prec, tol in (("bf16", lp.chain_bound("bf16", "wav", "relmax")), ("fp16", lp.chain_bound("fp16", "wav", "relmax"))):   # tests/lowprec.py (measured 0.0151 / 0.0019)
        o16 = model(prec).sample(dict(batch), N=int(g["N"]), corrector_steps=1, snr=0.5, noise=draws)
        _check(_relmax(o16[key], out[key]), tol, "denoised-condition sampler", key, prec)
    with pytest.raises(NotImplementedError):
        m.sample({"perturbed": batch["perturbed"]}, N=1)                    # condition="both" without batch["fake"]


@pytest.mark.parametrize("tag,cond,sde_in,arch,losses", [("a", "noisy", "noisy", "LARGE", ("mse",)),
                                                          ("b", "both", "denoised", "LARGE_BOTH", ("mse", "mae"))])
def test_train_step_loss_matches_reference(golden_dir, tag, cond, sde_in, arch, losses):
    """SURVEY 8f4, forward half: ScoreModel.train_step (model_wrapper.py:147-208) -- what the reference module's validation_step /
    test_step log (SGMSE_module.py:56-63) -- through the HIP score network, against losses computed by the reference with the same
    t, z and crop start: random-excerpt and zero-padding branches, conditions noisy / both, mse / mae.  fp32: 2e-4 relative;
    bf16 within 3 % (sum of 65 k squared errors).  With frozen parameters training_step refuses (the taped path: test_hip_training.py)."""
    from universal_speech_enhancement_amd.SGMSE_module import SGMSEModule
    from universal_speech_enhancement_amd.sgmse.model_wrapper import ScoreModel
    g = dict(np.load(os.path.join(golden_dir, "train_loss.npz")))
    sd = tw.make_state_dict(int(g["weights_seed"]), **getattr(tw, arch))
    z = torch.from_numpy(tnoise.complex_normal(int(g["z_seed"]), "train_z_" + tag, (2, 1, 512, 64))).cuda()
    batch = {"clean": torch.from_numpy(g["clean_" + tag]).cuda(), "perturbed": torch.from_numpy(g["noisy_" + tag]).cuda(),
             "fake": torch.from_numpy(g["fake_" + tag]).cuda()}
    t = torch.from_numpy(g["t_" + tag]).cuda()
    for lt in losses:
        for prec, tol in (("fp32", 2e-4), ("bf16", 3e-2)):
            m = ScoreModel(backbone="ncsnpplarge", sde="ouve", t_eps=3e-2, condition=cond, loss_type=lt, n_fft=1022, hop_length=160,
                           num_frames=int(g["num_frames"]), window="hann", sde_input=sde_in, precision=prec)
            m.score_net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
            loss = m.train_step(batch, t=t, z=z, start=int(g["start"]))
            want = float(g[f"loss_{tag}_{lt}"])
            assert abs(float(loss) - want) < tol * want, (lt, prec, float(loss), want)
    mod = SGMSEModule(Score=m)
    v = mod.validation_step(batch)                                       # random t, z, start: finite, same order of magnitude
    assert torch.isfinite(v) and 0.1 * want < float(v) < 10 * want
    with pytest.raises(RuntimeError):                                    # frozen parameters (tests/test_hip_training.py covers the taped path)
        mod.training_step(batch, 0)


def test_replanning_between_shapes_is_transparent(sd_np):
    """A predict run over files of different lengths re-plans the workspace and re-captures the sampler graph per (B, T'); going
    back to an earlier shape must reproduce its earlier result bit for bit (same seed), whatever ran in between."""
    m = _score_model(sd_np, "bf16")
    w = tnoise.synth_noisy_speech(2, 20000, seed=11)
    a = {"perturbed": torch.from_numpy(w[:, :9600]).cuda()}                 # T' = 64
    b = {"perturbed": torch.from_numpy(w[:1, :20000]).cuda()}               # B = 1, T' = 128
    first = m.sample(dict(a), N=2, corrector_steps=1, snr=0.5, seed=5)["enhanced"].clone()
    other = m.sample(dict(b), N=2, corrector_steps=1, snr=0.5, seed=5)["enhanced"]
    assert other.shape == (1, 20000) and torch.isfinite(other).all()
    again = m.sample(dict(a), N=2, corrector_steps=1, snr=0.5, seed=5)["enhanced"]
    assert torch.equal(first, again)
    other2 = m.sample(dict(b), N=2, corrector_steps=1, snr=0.5, seed=5)["enhanced"]
    assert torch.equal(other, other2)


def test_c_host_enhances_a_wav_file_like_the_python_path(tmp_path, sd_np):
    """examples/enhance_wav.c: the reference's predict path for one file through the C ABI alone (use_load_utterance ->
    use_stft_fwd -> use_plan / use_set_sampler / use_sample -> use_istft_back -> use_wav_write), started from a packed weight file.
    Same library, same seed => the same 16-bit samples as the Python host (ScoreModel.sample + the module's writer)."""
    import subprocess
    from scipy.io import wavfile
    from universal_speech_enhancement_amd import wavio
    from universal_speech_enhancement_amd.hip_engine import HipScoreEngine
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "enhance_wav")
    if not os.path.exists(exe):
        pytest.fail("examples/enhance_wav is not built (run __graft_entry__.build())")
    blob = str(tmp_path / "large_fp32.usehip")
    e = HipScoreEngine(precision="fp32"); e.load_state_dict(sd_np); e.save_weight_blob(blob); e.close()
    src = (tnoise.synth_noisy_speech(1, 16000, seed=21)[0] * 0.5 * 32767).astype(np.int16)          # 16 kHz int16: resampled on load
    wavfile.write(str(tmp_path / "in.wav"), 16000, src)
    r = subprocess.run([exe, blob, str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), "2", "7", "fp32"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    sr, got = wavfile.read(str(tmp_path / "out.wav"))
    x, sr_in = wavio.load_utterance(str(tmp_path / "in.wav"), 24000, True)
    assert sr == sr_in == 24000 and got.dtype == np.int16 and got.shape == x.shape == (24000,)
    m = _score_model(sd_np, "fp32")
    want = m.sample({"perturbed": torch.from_numpy(x)[None].cuda()}, N=2, corrector_steps=1, snr=0.5, seed=7)["enhanced"][0].cpu().numpy()
    want16 = np.clip(np.rint(want.astype(np.float64) * 32767.0), -32768, 32767).astype(np.int16)
    # same kernels, same seed; the only difference is the last bit of the Hann window (C: double cos -> float, torch: float32), which
    # the randomly initialised network amplifies: <= 0.5 % of full scale on the worst sample, a fraction of an LSB on average
    d = np.abs(got.astype(np.int32) - want16.astype(np.int32))
    assert d.max() <= 164 and d.mean() < 2.0, (int(d.max()), float(d.mean()))
    bad = subprocess.run([exe, str(tmp_path / "missing.usehip"), str(tmp_path / "in.wav"), str(tmp_path / "o.wav")], capture_output=True, text=True)
    assert bad.returncode != 0 and "failed" in bad.stderr


@pytest.mark.parametrize("dtype,tol", [(0, 2e-5), (1, lp.op_bound(1)), (2, lp.op_bound(2))])   # 4 ulps of the storage type
def test_conv_sk_matches_the_generic_kernel(dtype, tol):
    """conv_sk_kernel (split-K schedule of the small maps) against conv_kernel on the same seeded operands through the
    single-convolution harness (use_conv_bench): plain / concatenated input, fused 1x1 shortcut, residual, no GroupNorm, odd map sizes
    and the 96-channel shapes of the nf = 96 networks, both tile widths (B = 16 selects the 64-channel one).  Tolerance = one
    rounding of the stored type relative to the largest output (different summation order); GroupNorm totals to 1e-3."""
    import ctypes as C
    from universal_speech_enhancement_amd import _lib
    from universal_speech_enhancement_amd._lib import UseConvCase
    # (B, H, W, C0, C1, Cout, XC0, XC1, act, gn, temb, res)
    cases = [(4, 8, 10, 256, 0, 256, 0, 0, 1, 1, 1, 0), (4, 8, 10, 256, 256, 256, 0, 0, 1, 1, 1, 0), (4, 16, 20, 256, 0, 256, 256, 256, 1, 1, 0, 0),
             (2, 16, 20, 256, 0, 256, 0, 0, 1, 1, 0, 1), (4, 8, 10, 256, 0, 256, 0, 0, 0, 0, 1, 0), (3, 7, 9, 96, 0, 96, 96, 96, 1, 1, 0, 0),
             (2, 5, 33, 96, 64, 64, 0, 0, 1, 1, 1, 0), (16, 16, 20, 256, 0, 256, 0, 0, 1, 1, 1, 1)]
    for (B, H, W, C0, C1, Cout, XC0, XC1, act, gn, temb, res) in cases:
        got = {}
        for variant in (1, 7):
            c = UseConvCase(B, H, W, C0, C1, Cout, XC0, XC1, act, gn, temb, res, 1, dtype, variant, 1)
            out = np.empty((B, H, W, Cout), np.float32); st = np.empty((B, Cout, 2), np.float32)
            ms, fl = C.c_double(), C.c_double()
            rc = _lib.lib().use_conv_bench(C.byref(c), out.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p), C.byref(ms), C.byref(fl))
            assert rc == 0, (variant, _lib.lib().use_last_error())
            got[variant] = (out, st)
        ref, sk = got[1], got[7]
        assert np.isfinite(sk[0]).all()
        assert np.abs(sk[0] - ref[0]).max() <= tol * np.abs(ref[0]).max(), (H, W, C0, C1, Cout, XC0)
        assert np.abs(sk[1] - ref[1]).max() <= 1e-3 * np.abs(ref[1]).max()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs in one process")
def test_two_handles_on_two_devices_in_one_process(sd_np):
    """include/use_hip.h: one handle per (process, device).  hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a property of (kernel,
    device): rounds 1-4 cached it in one flag per process, so the second device's > 64 KB-LDS kernels (conv_v4, conv_v2, the attention
    block, the pyramid heads) would have been launched unprepared.  Both devices must produce the same score, bit for bit."""
    from universal_speech_enhancement_amd.hip_engine import HipScoreEngine
    x = torch.from_numpy(tnoise.complex_normal(31, "tx", (2, 1, 512, 128))) * 0.5
    y = torch.from_numpy(tnoise.complex_normal(31, "ty", (2, 1, 512, 128))) * 0.5
    t = torch.tensor([0.8, 0.1])
    outs = []
    for dev in (1, 0):                                       # the NON-default device first: it is the one an unset attribute would hit
        with torch.cuda.device(dev):
            e = HipScoreEngine(precision="bf16", device=dev)
            e.load_state_dict(sd_np)
            e.plan(2, 128)
            outs.append(e.score(x.cuda(dev), y.cuda(dev), t.cuda(dev)).cpu())
            torch.cuda.synchronize(dev)
            e.close()
    assert torch.isfinite(torch.view_as_real(outs[0])).all()
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_partial_totals_and_atomic_totals_give_the_same_score_bit_for_bit(engines, prec):
    """GroupNorm statistics of the large maps: conv_v4 writes per-workgroup partial totals with plain stores (ConvArgs::stats_part) and
    gn_finalize sums them, instead of 64-bit atomics on the item's totals (round 5).  Both are sums of the same fixed-point integers, so the
    whole evaluation must agree BIT FOR BIT with the atomic form (use_set_option("stats_part", 0)); T' = 128 puts the 512 x 128 level
    (65 536 px > the 128 x 160 inline threshold, 128 workgroups per image) on that path, B = 5 on two sub-batch streams (3 + 2)."""
    from universal_speech_enhancement_amd.hip_engine import set_option
    eng = engines[prec]
    B, Tp = 5, 128
    x = torch.from_numpy(tnoise.complex_normal(21, "px", (B, 1, 512, Tp))).cuda() * 0.5
    y = torch.from_numpy(tnoise.complex_normal(21, "py", (B, 1, 512, Tp))).cuda() * 0.5
    t = torch.tensor([0.9, 0.5, 0.2, 0.05, 0.7], device="cuda")
    outs = {}
    try:
        for mode in (1, 0):
            set_option("stats_part", mode)
            eng.plan(B, Tp)
            outs[mode] = eng.score(x, y, t).clone()
    finally:
        set_option("stats_part", 1)
    assert torch.isfinite(torch.view_as_real(outs[1])).all()
    assert torch.equal(outs[1], outs[0])


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_conv_v5_and_conv_v4_give_the_same_score_bit_for_bit(engines, prec):
    """Round 6: the large-map convolution on v_mfma_f32_16x16x32 (conv_wide_kernel<Wide16x16>, conv_v5: less energy per FLOP, the default for 16-bit storage) against the
    same pipeline on v_mfma_f32_32x32x16 (conv_wide_kernel<Wide32x32>, conv_v4: use_set_option("conv_v5", 0)).  Same products, same fp32 accumulation per 32-channel chunk
    and tap, same epilogue arithmetic: the whole evaluation agrees bit for bit (as the single-convolution harness does on random data, maxdiff 0).
    T' = 128 at B = 5 (3 + 2 sub-batches): the 512 x 128 and 256 x 64 levels run on the kernel, with residuals, fused shortcuts, concatenated
    inputs and the Combine epilogue; the wide-tile threshold lowered to also put the smaller maps on it."""
    from universal_speech_enhancement_amd.hip_engine import set_option
    eng = engines[prec]
    B, Tp = 5, 128
    x = torch.from_numpy(tnoise.complex_normal(23, "vx", (B, 1, 512, Tp))).cuda() * 0.5
    y = torch.from_numpy(tnoise.complex_normal(23, "vy", (B, 1, 512, Tp))).cuda() * 0.5
    t = torch.tensor([0.9, 0.5, 0.2, 0.05, 0.7], device="cuda")
    outs = {}
    try:
        for blocks in (80, 1):
            set_option("conv_v4_min_blocks", blocks)
            for mode in (1, 0):
                set_option("conv_v5", mode)
                outs[blocks, mode] = eng.score(x, y, t).clone()
    finally:
        set_option("conv_v5", 1)
        set_option("conv_v4_min_blocks", 80)
    assert torch.isfinite(torch.view_as_real(outs[80, 1])).all()
    assert torch.equal(outs[80, 1], outs[80, 0]) and torch.equal(outs[1, 1], outs[1, 0])


def test_plans_and_graphs_of_recent_shapes_are_kept(engines):
    """A predict run over files of a few distinct lengths: 20 batches cycling through 5 padded lengths build 5 plans and capture 5
    graphs, not 20 (the plans of the most recently used shapes are parked with their graphs, use_engine.cpp: plan cache), and a
    shape that returns reproduces its first result bit for bit."""
    eng = engines["bf16"]
    base = {k: eng.stat(k) for k in ("graph_captures", "plans_built", "plan_cache_hits")}
    first = {}
    for rnd in range(4):
        for Tp in (64, 128, 192, 256, 320):
            y = torch.from_numpy(tnoise.complex_normal(5, f"y{Tp}", (2, 1, 512, Tp))).cuda() * 0.5
            eng.plan(2, Tp)
            eng.set_sampler(2, "reverse_diffusion", "langevin", 1, 0.5, 3e-2, use_graph=True)
            out = eng.sample(y, seed=11)
            torch.cuda.synchronize()
            if rnd == 0:
                first[Tp] = out.clone()
            else:
                assert torch.equal(out, first[Tp]), (rnd, Tp)
    assert eng.stat("plans_built") - base["plans_built"] == 5
    assert eng.stat("graph_captures") - base["graph_captures"] == 5
    assert eng.stat("plan_cache_hits") - base["plan_cache_hits"] == 15


@pytest.mark.parametrize("B", [1, 2, 3])
def test_second_and_third_replay_of_a_small_batch_graph(engines, B):
    """Batches of 1-3 items are evaluated without the sub-batch split; a graph holding four or more score evaluations must replay
    like its first launch (round 2: the captured hipMemsetAsync that cleared the GroupNorm totals did not clear them again on later
    replays - NaN from the second sampler call on; the totals are now cleared by a kernel)."""
    eng = engines["bf16"]
    y = torch.from_numpy(tnoise.complex_normal(8, f"ys{B}", (B, 1, 512, 64))).cuda() * 0.5
    eng.plan(B, 64)
    eng.set_sampler(2, "reverse_diffusion", "langevin", 1, 0.5, 3e-2, use_graph=True)
    outs = [eng.sample(y, seed=21).clone() for _ in range(3)]
    assert all(torch.isfinite(torch.view_as_real(o)).all() for o in outs)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("prec,tol", [("bf16", lp.op_bound("bf16")), ("fp16", lp.op_bound("fp16"))])      # 4 ulps of the storage type (measured 4.9e-3 / 4.3e-4)
def test_fused_attention_block_matches_the_oracle_block(golden_dir, engines, sd_np, prec, tol):
    """attn_fused_kernel (GroupNorm -> q, k, v NIN -> softmax(q k^T / sqrt(C)) v -> NIN_3 -> (x + h) / sqrt(2) in one launch, MFMA
    contractions; AttnBlockpp, layerspp.py:60-93) in isolation: the oracle's fp32 attention block applied to the block input the HIP
    path itself produced (the `pre_attn` tap, 16-bit) against the fused kernel's `post_attn`; and against the unfused path
    (three NIN launches, the VALU attention core, NIN_3) on the same input."""
    from universal_speech_enhancement_amd.hip_engine import set_option
    g = dict(np.load(os.path.join(golden_dir, "forward_large.npz")))
    x = torch.from_numpy(g["x"]).cuda(); t = torch.from_numpy(g["t_b"]).cuda()
    sd = no.to_torch(sd_np)
    prefix = [k[:-len(".NIN_0.W")] for k in sd if k.endswith(".NIN_0.W")][0]
    eng = engines[prec]
    taps = {}
    for fused in (1, 0):
        set_option("attn_fused", fused)
        try:
            eng.plan(x.shape[0], x.shape[3])
            eng.score(x[:, 0:1].contiguous(), x[:, 1:2].contiguous(), t)
            taps[fused] = (eng.debug_tensor("pre_attn").permute(0, 3, 1, 2).cpu(), eng.debug_tensor("post_attn").permute(0, 3, 1, 2).cpu())
        finally:
            set_option("attn_fused", 1)
    assert torch.equal(taps[0][0], taps[1][0])                                   # same block input either way
    with torch.no_grad():
        want = no.attn_block(taps[1][0], sd, prefix)
    _check(_relmax(taps[1][1], want), tol, "fused attention block vs oracle block", prec)
    _check(_relmax(taps[0][1], want), tol, "unfused attention block vs oracle block", prec)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("Tp", [64, 192, 704])
def test_fused_attention_block_at_other_token_counts(engines, prec, Tp):
    """attn_fused_kernel with 8 / 24 / 88 tokens (one, one and three 32-token tiles, the last one partly filled): same block output as
    the unfused path (three NIN launches, VALU attention core, NIN_3) up to the rounding of the probabilities (bound: 4 ulps of the storage type,
    tests/lowprec.py; the T' = 64 golden-shape block measures 4.9e-3 / 4.3e-4 against the oracle)."""
    from universal_speech_enhancement_amd.hip_engine import set_option
    eng = engines[prec]
    x = torch.from_numpy(tnoise.complex_normal(31, f"xa{Tp}", (2, 1, 512, Tp))).cuda() * 0.5
    y = torch.from_numpy(tnoise.complex_normal(32, f"ya{Tp}", (2, 1, 512, Tp))).cuda() * 0.5
    t = torch.tensor([0.7, 0.1]).cuda()
    taps = {}
    for fused in (1, 0):
        set_option("attn_fused", fused)
        try:
            eng.plan(2, Tp)
            eng.score(x, y, t)
            taps[fused] = eng.debug_tensor("post_attn").cpu()
        finally:
            set_option("attn_fused", 1)
    assert torch.isfinite(taps[1]).all()
    _check(_relmax(taps[1], taps[0]), lp.op_bound(prec), "fused vs unfused attention block", prec, Tp)
