"""The fused transforms either side of the network, one launch at a time through the C ABI, against plain float64 references
(tests/spectral_ref.py): stft_fwd_kernel / stft_fwd_items_kernel, istft_back_kernel / istft_back_items_kernel, spec_map_kernel and,
through them, twiddle_table_kernel and the (device, n_fft) table cache.  Same construction as tests/test_hip_forward_kernels.py: the
references see the float32 operands the kernel reads and round nowhere; every bound is per element, derived here, fixed before the first
GPU run and not fitted.  2^-24 = float32 unit roundoff, one per counted rounding; ULP_FN = 2 for hypotf and powf, 3 for a division.

Direct sums.  The kernel keeps two accumulation chains (even / odd n forward; odd / even k inverse), one fma per term.  The reference adds
the same terms in the same order in float64, so its running partial sums P_i are the magnitudes the kernel's roundings act on.  The
roundings are taken as independent, each at most 2^-25 |P_i| in the mean-square sense of Hoeffding's inequality, and every term carries two
more of its own size (the float32 twiddle, the float32 window product; inverse: the twiddle):
    |d| <= LAMBDA 2^-25 sqrt(sum_i P_i^2 + 2 sum_i term_i^2) + 2 x 2^-24 |S|         per real component, both chains in one sum,
LAMBDA = 7: 2 exp(-LAMBDA^2 / 2) = 4.6e-11 per component, nothing over the ~1e5 elements of a case; the last term is the addition of the
two chains.  dS = hypot(d_re, d_im).  (The abs-sum x sqrt(K) form of the other files is looser than the old 2e-5 max|ref| at the median
bin and is not used.)
Compression g(z) = z |z|^(e-1) factor, 0 < e <= 1:  |g(S + d) - g(S)| <= min(dS (|S| - dS)^(e-1) where dS < |S|, 2^(1-e) dS^e) - the
Lipschitz constant on the segment, and the Hoelder bound, which is the one that holds at near-zero bins - plus C_COMP = 2 ULP_FN + 2 = 6
roundings of |ref| (hypotf, powf, x factor, x S).  A bin whose sum is exactly zero (an all-zero frame) has bound 0: it must be 0.
spec_map: (|p - 1| (ULP_FN + 2) + ULP_FN + 4) 2^-24 |ref|, p the power: a = hypotf pre (ULP_FN + 2 with the rounded 1 / factor), carried
through powf |p - 1| times, powf ULP_FN, the rounded pre, three products.
Inverse.  Decompression: the same count less one product, C_DEC = |1 / e - 1| (ULP_FN + 2) + ULP_FN + 3 roundings of |S_k| per bin
(exponents with an exact reciprocal: 0.5 and 1), independent between bins: a frame sample x_t[n] = (S_0 + (-1)^n S_Ny + 2 sum_k ...) / N
takes sqrt(dS_0^2 + dS_Ny^2 + sum_k (2 dS_k)^2) / N from them, 2 x the direct-sum bound above / N from the two chains, and 5 roundings
(s0 + s1, the two additions, 1 / N and the product with it) of A = |S_0| + |S_Ny| + 2 (|s0| + |s1|).  Frames combine linearly through the
window, acc = sum_t w x_t and env = sum_t w^2 by nfr = ceil(N / hop) fmas each:
    bound(y) = (sum_t |w| dx_t + nfr 2^-24 sum_t |w x_t|) / env + (3 + nfr) 2^-24 |y|        (3: the division; env is the reference's).
env <= 1e-11 gives exactly 0 on both sides (torch.istft raises there); no case has an envelope value between 1e-12 and 1e-10.

`-m "not gpu"` pins the references (float64 torch.stft / torch.istft, np.fft, oracle.sde_oracle's spec_fwd / spec_back / pad_spec), holds
a float32 numpy evaluation of the same chains below the bounds on every GPU case (worst forward 0.390, inverse 0.350; per case below), and runs
the mutation controls on the GPU cases' shapes.  Forward: right reflection 2 L - 1 - q, window index shifted by one, twiddles from the
unreduced float32 angle 2 pi k n / N (sincosf without the integer reduction mod N), exponent on the power |S|^2, last frame dropped, frame
t in column t + 1.  Exempt by arithmetic: the right reflection at 64 / 64, L = 300, whose last frame ends at sample 287.  Inverse:
Nyquist term without (-1)^n, envelope over the T signal frames only (exempt where Tpad = T: there are no others), DC term doubled, w for
w^2 in the envelope, scale 1 / (N / 2).

Worst |err| / bound, forward / inverse: the float32 numpy emulation, then the MI355X (2026-10-19, this file's first commit, on f35ed92).
    1022-160-L2400     0.390 / 0.223    0.390 / 0.223          1024-256        0.295 / 0.350    0.295 / 0.383
    1022-160-L2399     0.325 / 0.198    0.325 / 0.200          510-128         0.273 / 0.279    0.273 / 0.292
    1022-160-L512      0.273 / 0.180    0.273 / 0.196          64-64           0.177 / 0.169    0.177 / 0.163
    1022-160-sqrthann  0.296 / 0.169    0.315 / 0.188          16-3            0.173 / 0.117    0.152 / 0.117
    1022-400           0.282 / 0.309    0.282 / 0.297          1022-160-tone   0.324 / 0.216    0.318 / 0.222
    1022-73            0.336 / 0.153    0.336 / 0.166
MI355X only: consistent round trip 0.208; items 64-16, B = 65: 0.298 / 0.171; items 1022-160, B = 3: 0.377 / 0.171; spec_map_kernel 0.351.
No constant changed after a measurement.  A non-finite value anywhere in an output is a ratio of inf (spectral_ref.ratio; max() alone
would drop a NaN).  The CPU part takes about 20 s; the GPU tests build their references without the emulation, 5 s in a process of
their own."""
import functools

import numpy as np
import pytest
import torch

import spectral_ref as sr
from oracle import sde_oracle as so
from universal_speech_enhancement_amd.testing import noise as tnoise

INVALID = -1
EF = (0.5, 0.15)
# name, n_fft, hop, window, L, further Tpad beside T and T + 1, (exponent, factor) pairs, gain of the second item, tone
CASES = (
    ("1022-160-L2400", 1022, 160, "hann", 2400, (64,), (EF, (1.0, 1.0)), 1e-3, False),     # production geometry, L a hop multiple
    ("1022-160-L2399", 1022, 160, "hann", 2399, (), (EF,), 30.0, False),                   # L off a hop multiple
    ("1022-160-L512", 1022, 160, "hann", 512, (), (EF,), 1e-3, False),                     # L = n_fft / 2 + 1: both reflections in one frame
    ("1022-160-sqrthann", 1022, 160, "sqrthann", 2400, (), (EF,), 30.0, False),            # the refine stage's window
    ("1022-400", 1022, 400, "hann", 2400, (), (EF,), 1e-3, False),                         # hop > 256: second trip of the r loop
    ("1022-73", 1022, 73, "hann", 1500, (), (EF,), 30.0, False),                           # nfr = 14: 65 520 bytes of LDS, the most admitted
    ("1024-256", 1024, 256, "hann", 3000, (), (EF,), 1e-3, False),                         # n_fft = 0 mod 4, hop = block size
    ("510-128", 510, 128, "hann", 1000, (), (EF,), 30.0, False),                           # the second shipped geometry
    ("64-64", 64, 64, "hann", 300, (), (EF,), 1e-3, False),                                # nfr = 1, zero-envelope samples (w[0] = 0)
    ("16-3", 16, 3, "hann", 40, (), (EF,), 30.0, False),                                   # hop not dividing n_fft
    ("1022-160-tone", 1022, 160, "hann", 2400, (), (EF,), 1e-3, True),                     # back to the first table; a pure tone added
)
IDS = [c[0] for c in CASES]


def tpads(case):
    T = sr.n_frames(case[4], case[2])
    return (T, T + 1) + case[5]


@functools.lru_cache(maxsize=None)
def case_wav(ci):
    """float32 [2, L]: noisy speech; item 1 at another gain with a region of N + hop zeros (one whole frame of zeros) where L allows."""
    _, N, hop, _, L, _, _, gain, tone = CASES[ci]
    wav = tnoise.synth_noisy_speech(2, L, seed=11 + ci).astype(np.float32)
    if tone:
        wav = (wav + 0.5 * np.sin(2 * np.pi * 0.05 * np.arange(L))[None, :]).astype(np.float32)
    wav[1] *= np.float32(gain)
    if L > N + hop:
        s = (L - (N + hop)) // 2
        wav[1, s:s + N + hop] = 0
    return wav


_REFS = {}


def _cached(key, emulate, make):
    """One reference per key, shared by the tests of a process.  The float32 emulation is run only for a test that asks for it (the
    CPU tests); a reference that already carries one serves the others too."""
    r = _REFS.get(key)
    if r is None or (emulate and "emu" not in r):
        r = _REFS[key] = make(emulate)
    return r


def fwd_ref(ci, b, expo, factor, emulate=False):
    _, N, hop, wname, L = CASES[ci][:5]
    return _cached(("fwd", ci, b, expo, factor), emulate, lambda e: sr.stft_fwd(
        case_wav(ci)[b], sr.window(wname, N), N, hop, max(tpads(CASES[ci])), expo, factor, emulate=e))


def synth_input(ci, b, Tpad, expo, factor):
    """complex64 [F, Tpad]: the reference spectrogram times a random positive gain plus a small perturbation in every bin of every frame -
    not STFT-consistent, no frame zero, DC and Nyquist bins with imaginary parts (which the transform must ignore)."""
    Y = fwd_ref(ci, b, expo, factor)["Y"][:, :Tpad]
    rng = np.random.default_rng(1000 * ci + 10 * Tpad + b)
    pert = 1e-3 * np.abs(Y).max() * (rng.standard_normal(Y.shape) + 1j * rng.standard_normal(Y.shape))
    return (Y * rng.uniform(0.5, 2.0, Y.shape) + pert).astype(np.complex64)


def back_ref(ci, b, Tpad, expo, factor, emulate=False):
    _, N, hop, wname, L = CASES[ci][:5]
    return _cached(("back", ci, b, Tpad, expo, factor), emulate, lambda e: sr.istft_back(
        synth_input(ci, b, Tpad, expo, factor), sr.window(wname, N), N, hop, L, expo, factor, emulate=e))


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: pins, emulation, mutation controls (every reference here carries the emulation, so that each is computed once)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [0, 2, 3, 6, 9], ids=[IDS[i] for i in (0, 2, 3, 6, 9)])
def test_references_match_torch_and_the_oracle(ci):
    _, N, hop, wname, L = CASES[ci][:5]
    win = sr.window(wname, N)
    w64 = torch.from_numpy(win).double()
    for b in (0, 1):
        r = fwd_ref(ci, b, *EF, emulate=True)
        T = r["S"].shape[1]
        S = torch.stft(torch.from_numpy(case_wav(ci)[b]).double(), N, hop, window=w64, center=True, return_complex=True)
        assert S.shape[1] == T and np.abs(S.numpy() - r["S"]).max() <= 1e-12 * np.abs(r["S"]).max()
        Y = so.spec_fwd(S, EF[1], EF[0])
        assert np.abs(Y.numpy() - r["Y"][:, :T]).max() <= 1e-7 * np.abs(r["Y"]).max()         # EF as floats here, doubles there
        fast = sr.stft_fwd(case_wav(ci)[b], win, N, hop, T, *EF, sums=False)
        assert np.abs(fast["Y"] - r["Y"][:, :T]).max() <= 1e-12 * np.abs(r["Y"]).max()
        if ci == 0:                                                                           # pad_spec: to the next multiple of 64
            P = so.pad_spec(Y[None, None])[0, 0].numpy()
            assert P.shape == r["Y"].shape and not r["Y"][:, T:].any() and not P[:, T:].any()
        for Tpad in tpads(CASES[ci])[:2]:
            X = synth_input(ci, b, Tpad, *EF)
            br = back_ref(ci, b, Tpad, *EF, emulate=True)
            Sd = so.spec_back(torch.from_numpy(X.astype(np.complex128)), float(np.float32(EF[1])), EF[0])
            assert np.abs(Sd.numpy() - sr.decompress(X, *EF)[0]).max() <= 1e-12 * float(Sd.abs().max())
            irf = np.fft.irfft(Sd.numpy().T, N, axis=1)                                        # [Tpad, N]; ignores Im of DC and Nyquist
            assert np.abs(irf - br["x"]).max() <= 1e-12 * np.abs(irf).max()
            y = torch.istft(Sd, N, hop, window=w64, center=True, length=L).numpy()
            assert np.abs(y - br["y"]).max() <= 1e-11 * np.abs(y).max()
            fast = sr.istft_back(X, win, N, hop, L, *EF, sums=False)
            assert np.abs(fast["y"] - br["y"]).max() <= 1e-12 * np.abs(br["y"]).max()


def test_zero_envelope_and_zero_frames_in_the_references():
    """64 / 64: w[0] = 0 is the only tap that reaches the samples m = 64 t - 32, and with Tpad = T no frame reaches m >= 288: exact
    zeros, bound 0.  An all-zero frame has bound 0 too."""
    ci = IDS.index("64-64")
    T = sr.n_frames(300, 64)
    r = back_ref(ci, 0, T, *EF, emulate=True)
    zero = np.where(r["env"] <= 1e-11)[0]
    assert set(zero) == set(range(32, 288, 64)) | set(range(288, 300)) and not r["y"][zero].any() and not r["bound"][zero].any()
    # with one more frame, frame T reaches them (sample 288 only through w[0] = 0)
    assert (back_ref(ci, 0, T + 1, *EF, emulate=True)["env"][289:] > 1e-11).all()
    for ci in (0, 4, 6):
        f = fwd_ref(ci, 1, *EF, emulate=True)
        cols = np.where(~f["S"].any(0))[0]
        assert cols.size >= 1 and not f["bound"][:, cols].any()


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_float32_emulation_stays_below_the_bounds(ci):
    case = CASES[ci]
    wf = wb = 0.0
    for expo, factor in case[6]:
        for b in (0, 1):
            r = fwd_ref(ci, b, expo, factor, emulate=True)
            wf = max(wf, sr.ratio(np.abs(r["emu"].astype(np.complex128) - r["Y"]), r["bound"]))
            for Tpad in tpads(case) if (expo, factor) == EF else tpads(case)[:2]:
                br = back_ref(ci, b, Tpad, expo, factor, emulate=True)
                wb = max(wb, sr.ratio(np.abs(br["emu"].astype(np.float64) - br["y"]), br["bound"]))
    print(f"[emulated] {case[0]}: worst |err| / bound forward {wf:.3f}, inverse {wb:.3f}")
    assert wf < 1.0 and wb < 1.0


def test_a_non_finite_output_exceeds_every_bound():
    """The comparison itself: a NaN or an infinity in one element of an output is a ratio of inf, also through the max() the tests
    fold their cases with (max() alone would drop a NaN)."""
    ci = IDS.index("16-3")
    r, br = fwd_ref(ci, 0, *EF, emulate=True), back_ref(ci, 0, tpads(CASES[ci])[0], *EF, emulate=True)
    assert sr.ratio(np.abs(r["Y"].astype(np.complex64) - r["Y"]), r["bound"]) <= 1.0
    for bad in (np.nan, np.inf):
        got = r["Y"].astype(np.complex64)
        got[3, 2] = complex(0.0, bad)
        w = max(0.0, sr.ratio(np.abs(got.astype(np.complex128) - r["Y"]), r["bound"]))
        assert w == np.inf and not w <= 1.0
        y = br["y"].astype(np.float32)
        y[7] = bad
        w = max(0.0, sr.ratio(np.abs(y.astype(np.float64) - br["y"]), br["bound"]))
        assert w == np.inf and not w <= 1.0


FWD_MUT = ("reflect", "win_shift", "f32_angle", "power", "drop_last", "shift")
BACK_MUT = ("nyq_sign", "env_T", "dc2", "env_w", "scale")


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_mutations_exceed_the_bounds(ci):
    case = CASES[ci]
    _, N, hop, wname, L = case[:5]
    win = sr.window(wname, N)
    T = sr.n_frames(L, hop)
    for expo, factor in case[6]:
        for b in (0, 1):
            r = fwd_ref(ci, b, expo, factor, emulate=True)
            for mut in FWD_MUT:
                if mut == "reflect" and (T - 1) * hop + N // 2 - 1 < L:
                    continue                                                                  # exempt: no frame reaches past the end
                m = sr.stft_fwd(case_wav(ci)[b], win, N, hop, T + 1, expo, factor, mut=mut, sums=False)
                assert sr.ratio(np.abs(m["Y"] - r["Y"][:, :T + 1]), r["bound"][:, :T + 1]) > 1.0, (case[0], b, mut)
            for Tpad in tpads(case)[:2]:
                br = back_ref(ci, b, Tpad, expo, factor, emulate=True)
                for mut in BACK_MUT:
                    if mut == "env_T" and Tpad == T:
                        continue                                                              # exempt: every frame is a signal frame
                    m = sr.istft_back(synth_input(ci, b, Tpad, expo, factor), win, N, hop, L, expo, factor, mut=mut, sums=False)
                    assert sr.ratio(np.abs(m["y"] - br["y"]), br["bound"]) > 1.0, (case[0], b, Tpad, mut)


def spec_input(T=7):
    """complex64 [2, 33, T]: magnitudes from 1e-6 to 1e3 and one exact zero."""
    rng = np.random.default_rng(3)
    mag = 10.0 ** rng.uniform(-6, 3, (2, 33, T))
    Z = (mag * np.exp(2j * np.pi * rng.uniform(size=mag.shape))).astype(np.complex64)
    Z[1, 5, 3] = 0
    return Z


def test_spec_map_reference_matches_the_oracle():
    Z = spec_input()
    for expo, factor in (EF, (1.0, 1.0)):
        f64 = float(np.float32(factor))
        for b in (0, 1):
            ref, bound = sr.spec_map(Z[b], 64, expo, factor, back=False)
            P = so.pad_spec(so.spec_fwd(torch.from_numpy(Z[b].astype(np.complex128)), f64, expo)[None, None])[0, 0].numpy()
            assert P.shape == ref.shape and np.abs(P - ref).max() <= 1e-12 * np.abs(ref).max()
            back, _ = sr.spec_map(ref.astype(np.complex64), 7, expo, factor, back=True)
            Sb = so.spec_back(torch.from_numpy(ref.astype(np.complex64).astype(np.complex128)), f64, expo)[:, :7].numpy()
            assert np.abs(Sb - back).max() <= 1e-12 * np.abs(back).max()
            m, _ = sr.spec_map(Z[b], 64, expo, factor, back=False, mut="power")
            assert sr.ratio(np.abs(m - ref), bound) > 1.0


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
SENT = 7.5


def _L():
    from universal_speech_enhancement_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _c64(n):
    return torch.full((n + 4,), complex(SENT, -SENT), dtype=torch.complex64, device="cuda")


def _f32(n):
    return torch.full((n + 8,), SENT, dtype=torch.float32, device="cuda")


def _stft(wav, win, N, hop, Tpad, expo, factor):
    B, L = wav.shape
    F = N // 2 + 1
    out = _c64(B * F * Tpad)
    dwav, dwin = _dev(wav), _dev(win)                                                      # alive until the result is read back
    rc = _L().use_stft_fwd(dwav.data_ptr(), out.data_ptr(), B, L, N, hop, dwin.data_ptr(), Tpad, factor, expo, _stream())
    assert rc == 0, _L().use_last_error()
    got = out.cpu().numpy()
    assert (got[B * F * Tpad:] == np.complex64(complex(SENT, -SENT))).all(), "use_stft_fwd wrote past its output"
    return got[:B * F * Tpad].reshape(B, F, Tpad)


def _istft(X, win, N, hop, L, expo, factor):
    B, F, Tpad = X.shape
    out = _f32(B * L)
    dX, dwin = _dev(X), _dev(win)
    rc = _L().use_istft_back(dX.data_ptr(), out.data_ptr(), B, L, N, hop, dwin.data_ptr(), Tpad, factor, expo, _stream())
    assert rc == 0, _L().use_last_error()
    got = out.cpu().numpy()
    assert (got[B * L:] == np.float32(SENT)).all(), "use_istft_back wrote past its output"
    return got[:B * L].reshape(B, L)


@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_stft_and_istft_per_element(ci):
    case = CASES[ci]
    _, N, hop, wname, L = case[:5]
    win, wav = sr.window(wname, N), case_wav(ci)
    wf = wb = 0.0
    for expo, factor in case[6]:
        for Tpad in tpads(case) if (expo, factor) == EF else tpads(case)[:2]:
            got = _stft(wav, win, N, hop, Tpad, expo, factor)
            X = np.stack([synth_input(ci, b, Tpad, expo, factor) for b in (0, 1)])
            y = _istft(X, win, N, hop, L, expo, factor)
            for b in (0, 1):
                r = fwd_ref(ci, b, expo, factor)
                wf = max(wf, sr.ratio(np.abs(got[b].astype(np.complex128) - r["Y"][:, :Tpad]), r["bound"][:, :Tpad]))
                br = back_ref(ci, b, Tpad, expo, factor)
                wb = max(wb, sr.ratio(np.abs(y[b].astype(np.float64) - br["y"]), br["bound"]))
    print(f"[measured] {case[0]}: worst |err| / bound stft_fwd_kernel {wf:.3f}, istft_back_kernel {wb:.3f}")
    assert wf <= 1.0 and wb <= 1.0


@pytest.mark.gpu
def test_consistent_round_trip():
    """istft(stft(wav)) with Tpad = T: held per element against the reference on the device's own spectrogram, and it is the waveform
    (to 1e-4 of the peak, the round-trip tolerance of test_hip_parity.test_device_stft_istft_match_torch; with Tpad = T no zero frame
    overlaps the tail, so every sample is held)."""
    ci = 0
    _, N, hop, wname, L = CASES[ci][:5]
    win, wav = sr.window(wname, N), case_wav(ci)
    T = sr.n_frames(L, hop)
    Y = _stft(wav, win, N, hop, T, *EF)
    y = _istft(Y, win, N, hop, L, *EF)
    worst = 0.0
    for b in (0, 1):
        br = sr.istft_back(Y[b], win, N, hop, L, *EF)
        worst = max(worst, sr.ratio(np.abs(y[b].astype(np.float64) - br["y"]), br["bound"]))
        assert np.abs(y[b] - wav[b]).max() <= 1e-4 * np.abs(wav[b]).max()
    print(f"[measured] round trip: worst |err| / bound istft_back_kernel {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.gpu
def test_transform_refusals_launch_nothing():
    L_ = _L()
    N, hop, L = 1022, 160, 2400
    T = sr.n_frames(L, hop)
    F = N // 2 + 1
    wav, win = _dev(case_wav(0)), _dev(sr.window("hann", N))
    Y, yo = _c64(2 * F * 64), _f32(2 * L)
    X = _dev(np.ones((2, F, 64), np.complex64))

    def refused(call, word):
        """USE_E_INVALID with `word` in the message of THIS call: another refusal (host only) sets a different message first."""
        assert L_.use_chunk_count(0, 64, 0) == INVALID and b"Tp=0" in L_.use_last_error()
        rc = call()
        msg = L_.use_last_error().decode()
        assert rc == INVALID and word in msg and "Tp=0" not in msg, (rc, word, msg)
    # (n_fft, hop, L, Tpad) -> the rule of check_stft_args that has to refuse it; 1022 / 72 passes every rule but the LDS one
    bad = dict(lds=((N, 72, L, sr.n_frames(L, 72)), "LDS"), hop0=((N, 0, L, T), "bad STFT arguments"),
               hop_big=((N, N + 1, L, T), "bad STFT arguments"), odd=((N - 1, hop, L, T), "bad STFT arguments"),
               short=((N, hop, N // 2, T), "too short for reflect padding"), tpad=((N, hop, L, T - 1), f"Tpad={T - 1} is smaller"))
    for (n, h, l, tp), word in bad.values():
        refused(lambda: L_.use_stft_fwd(wav.data_ptr(), Y.data_ptr(), 2, l, n, h, win.data_ptr(), tp, EF[1], EF[0], _stream()), word)
        refused(lambda: L_.use_istft_back(X.data_ptr(), yo.data_ptr(), 2, l, n, h, win.data_ptr(), tp, EF[1], EF[0], _stream()), word)
    ptrs = [wav.data_ptr(), Y.data_ptr(), win.data_ptr()]
    for k in range(3):
        p = list(ptrs)
        p[k] = None
        refused(lambda: L_.use_stft_fwd(p[0], p[1], 2, L, N, hop, p[2], T, EF[1], EF[0], _stream()), "null argument")
    ptrs = [X.data_ptr(), yo.data_ptr(), win.data_ptr()]
    for k in range(3):
        p = list(ptrs)
        p[k] = None
        refused(lambda: L_.use_istft_back(p[0], p[1], 2, L, N, hop, p[2], T, EF[1], EF[0], _stream()), "bad arguments")
    torch.cuda.synchronize()
    assert bool((Y == complex(SENT, -SENT)).all()) and bool((yo == SENT).all()), "a refused call wrote to its output"


def _items_case(N, hop, lens, stride, Tpad, wname="hann", seed=5):
    import ctypes as C
    B = len(lens)
    F = N // 2 + 1
    win = sr.window(wname, N)
    wav = np.full((B, stride), np.nan, np.float32)
    speech = tnoise.synth_noisy_speech(B, stride, seed=seed).astype(np.float32)
    for b, n in enumerate(lens):
        wav[b, :n] = speech[b, :n] * np.float32(10.0 ** ((b % 5) - 2))
    cl = (C.c_int * B)(*lens)
    lib = _L()
    Y = _c64(B * F * Tpad)
    dwav, dwin = _dev(wav), _dev(win)
    rc = lib.use_stft_fwd_items(dwav.data_ptr(), stride, cl, Y.data_ptr(), B, N, hop, dwin.data_ptr(), Tpad, EF[1], EF[0], _stream())
    assert rc == 0, lib.use_last_error()
    got = Y.cpu().numpy()
    assert (got[B * F * Tpad:] == np.complex64(complex(SENT, -SENT))).all()
    got = got[:B * F * Tpad].reshape(B, F, Tpad)
    assert np.isfinite(got.view(np.float32)).all(), "a sample past an item's length was read"
    refs = [sr.stft_fwd(wav[b, :n], win, N, hop, Tpad, *EF) for b, n in enumerate(lens)]
    rng = np.random.default_rng(seed)
    X = np.stack([(r["Y"] * rng.uniform(0.5, 2.0, r["Y"].shape) + 1e-3 * np.abs(r["Y"]).max() *
                   (rng.standard_normal(r["Y"].shape) + 1j * rng.standard_normal(r["Y"].shape))).astype(np.complex64) for r in refs])
    out = _f32(B * stride)
    dX = _dev(X)
    rc = lib.use_istft_back_items(dX.data_ptr(), out.data_ptr(), stride, cl, B, N, hop, dwin.data_ptr(), Tpad, EF[1], EF[0], _stream())
    assert rc == 0, lib.use_last_error()
    y = out.cpu().numpy()
    assert (y[B * stride:] == np.float32(SENT)).all(), "use_istft_back_items wrote past the stride of the last row"
    y = y[:B * stride].reshape(B, stride)
    wf = wb = 0.0
    for b, n in enumerate(lens):
        wf = max(wf, sr.ratio(np.abs(got[b].astype(np.complex128) - refs[b]["Y"]), refs[b]["bound"]))
        br = sr.istft_back(X[b], win, N, hop, n, *EF)
        wb = max(wb, sr.ratio(np.abs(y[b, :n].astype(np.float64) - br["y"]), br["bound"]))
        assert not y[b, n:].any(), f"row {b}: samples past len are not zero"
    for b in range(max(0, B - 3), B):                                                         # the rows either side of the second launch
        n = lens[b]
        one = _stft(wav[b:b + 1, :n], win, N, hop, Tpad, *EF)
        assert np.array_equal(one[0].view(np.uint32), got[b].view(np.uint32)), f"row {b} != the one-item call, bitwise"
        one = _istft(X[b:b + 1], win, N, hop, n, *EF)
        assert np.array_equal(one[0].view(np.uint32), y[b, :n].view(np.uint32)), f"row {b} != the one-item call, bitwise"
    return wf, wb


@pytest.mark.gpu
def test_items_second_launch_of_65_rows():
    """B = 65 > 64 items per launch: rows 63, 64 (first launch) and 65 (second, through the b0 offsets) also bitwise."""
    rng = np.random.default_rng(1)
    lens = [int(v) for v in rng.integers(33, 301, 65)]
    lens[0], lens[62], lens[63], lens[64] = 33, 300, 33, 257
    wf, wb = _items_case(64, 16, lens, 307, 20)
    print(f"[measured] items 64-16 B=65: worst |err| / bound stft_fwd_items_kernel {wf:.3f}, istft_back_items_kernel {wb:.3f}")
    assert wf <= 1.0 and wb <= 1.0


@pytest.mark.gpu
def test_items_production_geometry():
    wf, wb = _items_case(1022, 160, [2400, 512, 1777], 2403, 16)
    print(f"[measured] items 1022-160 B=3: worst |err| / bound stft_fwd_items_kernel {wf:.3f}, istft_back_items_kernel {wb:.3f}")
    assert wf <= 1.0 and wb <= 1.0


@pytest.mark.gpu
def test_spec_map_per_element():
    lib = _L()
    Z = spec_input()
    B, F, T = Z.shape
    worst = 0.0
    for expo, factor in (EF, (1.0, 1.0)):
        for Tpad in (7, 64):
            Y = _c64(B * F * Tpad)
            dZ = _dev(Z)
            assert lib.use_spec_fwd(dZ.data_ptr(), Y.data_ptr(), B, F, T, Tpad, factor, expo, _stream()) == 0, lib.use_last_error()
            gy = Y.cpu().numpy()
            assert (gy[B * F * Tpad:] == np.complex64(complex(SENT, -SENT))).all()
            gy = gy[:B * F * Tpad].reshape(B, F, Tpad)
            S = _c64(B * F * T)
            dY = _dev(gy)
            assert lib.use_spec_back(dY.data_ptr(), S.data_ptr(), B, F, T, Tpad, factor, expo, _stream()) == 0, lib.use_last_error()
            gs = S.cpu().numpy()
            assert (gs[B * F * T:] == np.complex64(complex(SENT, -SENT))).all()
            gs = gs[:B * F * T].reshape(B, F, T)
            for b in range(B):
                ref, bound = sr.spec_map(Z[b], Tpad, expo, factor, back=False)
                worst = max(worst, sr.ratio(np.abs(gy[b].astype(np.complex128) - ref), bound))
                ref, bound = sr.spec_map(gy[b], T, expo, factor, back=True)
                worst = max(worst, sr.ratio(np.abs(gs[b].astype(np.complex128) - ref), bound))
            assert gy[1, 5, 3] == 0 and gs[1, 5, 3] == 0
    print(f"[measured] spec_map_kernel worst |err| / bound {worst:.3f}")
    assert worst <= 1.0
