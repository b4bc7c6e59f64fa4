"""The device noise generator and the element-wise SDE updates, one launch at a time through the C ABI, against an integer restatement of
Philox4x32-10 and float64 restatements of the OUVE updates (tests/philox_ref.py): fill_noise_kernel (as one item and per item),
prior_kernel, predictor_kernel, langevin_norms_kernel + langevin_step_kernel, corrector_kernel.  Same construction as
tests/test_hip_forward_kernels.py: every reference sees the operands the kernel sees and rounds where the kernel rounds; every bound is
per element and per real component, was fixed before the first GPU run and is not fitted.  2^-24 is the float32 unit roundoff; every
float32 rounding is counted as one 2^-24 of the magnitude it rounds; ULP_FN = 2 (x 2^-24) for logf, sinf, cosf, 3 for a division.

Noise.  The Philox words, u1, u2 (in (0, 1]: the + 0.5f rounds to even above 2^23, so 1.0 occurs and gives z = 0) and the float32 angle
are reproduced bit for bit.  Left to the device: r = sqrtf(-logf(u1)) - ULP_FN on the logarithm is ULP_FN / 2 on its root, the root and
the product r * cs one rounding together (half each) - and sincosf (ULP_FN of a value of at most 1):
    |z - z_ref| <= (ULP_FN / 2 + 1 + ULP_FN) 2^-24 r = 4 x 2^-24 r          per component, no element exempt (r = 0: exact).
The counter's high word (idx >> 32) needs 2^32 elements (32 GiB) and stays untested.

Host coefficients (use_engine.cpp: ouve_std, ouve_diffusion, predictor_coeffs; float32 like the reference's tensors).  sigma =
sigma_min * powf(sigma_max / sigma_min, t): the quotient 1, carried through the power t <= 1 times, powf ULP_FN, the product 1 -> 4;
g = (float)(sigma sqrt(2 logsig)) -> 5.  Reverse diffusion: dt = (float)(1 / N) 1, sqrt(dt) 1.5, G = g sqrt(dt) 7.5, c_score = G G 16,
c_noise = G 7.5, c_drift = theta dt 2.  Euler-Maruyama (double arithmetic, one final rounding each): c_drift 1, c_score = g g dt 12,
c_noise 6.  One set for both: E_CD = 2, E_CS = 16, E_CN = 8.  std(t) is computed in double and rounded once: E_STD = 1; the ALD step
2 (snr std)^2: snr std 2, its square 4, the product 5 = E_ALD.
Prior  x = y + z std1:  2^-24 (|y| + (E_STD + 2) std1 |z|)   (product, sum);  with device noise + std1 (noise bound).
Predictor  m = x - (cd (y - x) - cs s), out = m + cn z:
    bound(m)   = 2^-24 (|x| + (E_CD + 4) cd |y - x| + (E_CS + 3) cs |s|)        (difference, product, inner difference, outer difference)
    bound(out) = bound(m) + 2^-24 (|x| + cd |y - x| + cs |s| + (E_CN + 2) cn |z|)      (product, sum)
The two predictors are the same map in exact arithmetic (theta / N, g^2 / N, g / sqrt N): exchanging their coefficients moves nothing
beyond the bound at any t, which is the exemption of that mutation control; test_the_two_predictors_share_one_reference asserts it.
Langevin step  eps = 2 (snr mean_b ||z_b|| / mean_b ||g_b||)^2: a thread adds k = ceil(n_per_b / 32768) terms g.x^2 + g.y^2 (2 each)
serially (k), then 6 shuffle levels and 3 additions (9): k + 11 on a sum of squares, half of it on a norm; the rest is double until the
two float casts (1 each).  r = snr zm / gm: (k + 11) / 2 twice, 2 casts, product 1, division 3 -> k + 17;  eps = 2 r r: 2 (k + 17) + 1.
Corrector  m = x + eps g, out = m + z sqrtf(2 eps):
    bound(m)   = 2^-24 (|x| + (E_eps + 2) eps |g|),    bound(out) = bound(m) + 2^-24 (|x| + eps |g| + (E_eps / 2 + 3) sqrt(2 eps) |z|).
The step size itself is held through a run with x = 0, where x_mean = eps g and bound(m) = (E_eps + 2) 2^-24 eps |g|.

`-m "not gpu"` pins the references (Random123's known answers, oracle.sde_oracle) and runs the mutation controls on the GPU cases'
shapes: multipliers swapped, counter words (element, draw) swapped, low 24 bits for high, sqrt(-2 log u), item stream indexed by the
global element (item 0 is exempt: its offset is 0); norm of the batch mean for mean of norms (B = 1 exempt: they coincide),
sqrt(eps) for sqrt(2 eps), x_mean carrying the noise term.

Measured on the MI355X (2026-10-19, this file's first commit, on f35ed92), worst |err| / bound: fill_noise_kernel 0.665 (0.817 past the
grid-stride wrap), per item 0.881, prior_kernel 0.981 (0.838 with device noise), predictor_kernel 0.977, corrector_kernel
Langevin 0.995 (0.999 on the device's own noise), ALD 0.996, the Langevin step size alone (x = 0) 0.099.  The updates' worst elements are output roundings at the bottom
of a binade, where half a spacing is 2^-24 |ref| itself.  No constant changed after a measurement.  There is no float32 emulation here:
these bounds count worst-case roundings and need none.  The GPU tests' output buffers start as NaN with a guard element behind them,
and a non-finite value anywhere in an output is a ratio of inf (philox_ref.ratio; max() alone would drop a NaN): an element left unwritten
cannot pass, nor can a stale result in a reused block stand in for one.  The CPU part takes about 1 s."""
import ctypes as C

import numpy as np
import pytest
import torch

import philox_ref as pr
from oracle import sde_oracle as so

INVALID = -1
SEEDS = (0, 1, 2 ** 32, 2 ** 64 - 1, 20260929)
DRAWS = (0, 1, 60, 2 ** 31 - 1)
SIZES = (1, 255, 257)
N_WRAP = 8192 * 256 + 300                                   # past fill_noise_kernel's grid-stride wrap
ITEM_SEEDS = (0x0123456789ABCDEF, 7, 2 ** 64 - 1)
N_ITEM_WRAP = 2730 * 256 + 5                                # past fill_noise_kernel's wrap per item at B = 3 (8192 / 3 = 2730 blocks)
SHAPES = ((3, 1, 33, 7), (2, 1, 512, 64))
GAINS = {3: (1e-2, 1.0, 10.0), 2: (1e-2, 10.0)}             # three decades between the items
TS, NS, SNR = (1.0, 0.4, 0.03), (30, 1), 0.5


def _cn(rng, shape):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.sqrt(0.5)).astype(np.complex64)


def sde_inputs(shape, seed=5):
    """x, y, score, z as complex64 [B,1,F,T]; item b scaled by GAINS[B][b] (score by its inverse, as a score of that state would be)."""
    rng = np.random.default_rng(seed + shape[0] * 1000 + shape[2])
    B = shape[0]
    gains = np.asarray(GAINS.get(B, np.logspace(-2, 1, B)), np.float32).reshape(B, 1, 1, 1)
    x, y, s, z = (_cn(rng, shape) for _ in range(4))
    return x * gains, y * gains, s / gains, z


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: pins of the references
# ---------------------------------------------------------------------------------------------------------------------------
KAT = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10; the vectorised form agrees with the scalar one."""
    for ctr, key, out in KAT:
        assert tuple(int(v) for v in pr.philox4x32(ctr, key)) == out
    ctrs = [np.array([k[0][i] for k in KAT], np.uint64) for i in range(4)]
    for j, (ctr, key, out) in enumerate(KAT):
        got = pr.philox4x32(ctrs, key)
        assert tuple(int(v[j]) for v in got) == out


def test_uniform_is_half_open_at_zero():
    """u = ((float)(c >> 8) + 0.5f) 2^-24 lies in (0, 1]: the largest 24-bit value rounds up to 1.0, the smallest gives 2^-25."""
    top = (np.float32(2 ** 24 - 1) + np.float32(0.5)) * np.float32(2.0 ** -24)
    assert top == np.float32(1.0) and (np.float32(0) + np.float32(0.5)) * np.float32(2.0 ** -24) == np.float32(2.0 ** -25)
    u1, u2, ang = pr.uniforms(SEEDS[4], 0, np.arange(1 << 16))
    assert u1.dtype == u2.dtype == ang.dtype == np.float32 and u1.min() > 0 and u1.max() <= 1 and u2.min() > 0 and u2.max() <= 1
    re, im, b = pr.fill_noise(SEEDS[4], 0, 1 << 16)
    assert abs(re.mean()) < 0.01 and abs(im.mean()) < 0.01 and abs(re.var() - 0.5) < 0.01 and abs(im.var() - 0.5) < 0.01
    assert abs((re * im).mean()) < 0.01


def test_noise_counter_layout():
    """Element i of draw d: counter (i, 0, d, 0), key (seed low, seed high); item streams restart at 0 in every item."""
    c = pr.philox4x32((5, 0, 3, 0), (SEEDS[4] & 0xffffffff, SEEDS[4] >> 32))
    u1, u2, _ = pr.uniforms(SEEDS[4], 3, np.array([5]))
    assert u1[0] == (np.float32(int(c[0]) >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24)
    assert u2[0] == (np.float32(int(c[1]) >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24)
    a = pr.fill_noise_items(ITEM_SEEDS, 2, 300)
    for b, s in enumerate(ITEM_SEEDS):
        one = pr.fill_noise(s, 2, 300)
        assert np.array_equal(a[0][b], one[0]) and np.array_equal(a[1][b], one[1])


@pytest.mark.parametrize("mut", ["swap_mult", "swap_counter", "low24", "sqrt2log"])
def test_noise_mutations_exceed_the_bound(mut):
    worst = np.inf
    for seed in SEEDS:
        for draw in DRAWS[1:] if mut == "swap_counter" else DRAWS:        # draw 0 at element 0 swaps nothing
            for n in SIZES:
                re, im, b = pr.fill_noise(seed, draw, n)
                mre, mim, _ = pr.cnormal(seed, draw, np.arange(n, dtype=np.uint64), mut=mut)
                worst = min(worst, pr.ratio(mre + 1j * mim, re + 1j * im, b, b))
    print(f"[mutation] noise {mut}: smallest worst-element ratio over the cases {worst:.3g}")
    assert worst > 1.0


def test_item_stream_mutation_exceeds_the_bound():
    idx = np.r_[0:300, N_ITEM_WRAP - 300:N_ITEM_WRAP]
    re, im, b = pr.fill_noise_items(ITEM_SEEDS, 1, N_ITEM_WRAP, idx)
    mre, mim, _ = pr.fill_noise_items(ITEM_SEEDS, 1, N_ITEM_WRAP, idx, mut="global_index")
    assert np.array_equal(mre[0], re[0])                                   # exempt: item 0 starts at element 0 either way
    for i in (1, 2):
        assert pr.ratio(mre[i] + 1j * mim[i], re[i] + 1j * im[i], b[i], b[i]) > 1.0


def _t64(a):
    return torch.from_numpy(np.asarray(a).astype(np.complex128))


def _close(a, b):
    """reference against reference: 1e-6 of the item's largest magnitude (the oracle's sqrt(dt) is a float32 tensor, 6e-8, and its
    SDE constants are doubles where the engine holds floats, 1.5e-8; an element may be a difference of larger terms)."""
    a, b = np.asarray(a), np.asarray(b)
    tol = 1e-6 * np.abs(b).reshape(b.shape[0], -1).max(1).reshape((-1,) + (1,) * (b.ndim - 1))
    assert (np.abs(a - b) <= tol).all(), float((np.abs(a - b) / tol).max())


@pytest.mark.parametrize("shape", SHAPES)
def test_sde_references_match_the_oracle(shape):
    """philox_ref's updates against oracle.sde_oracle evaluated in double (its sqrt(dt) is a float32 tensor: 6e-8 relative)."""
    x, y, s, z = sde_inputs(shape)
    B = shape[0]
    assert abs(pr.ouve_std(1.0) - float(so.ouve_std(torch.ones(1, dtype=torch.float64)))) < 1e-7      # THETA etc. as floats
    xp, _, _ = pr.prior(y, z)
    ref = _t64(y) + _t64(z) * so.ouve_std(torch.ones(B, dtype=torch.float64))[:, None, None, None]
    _close(xp, ref.numpy())
    for t in TS:
        tv = torch.full((B,), float(np.float32(t)), dtype=torch.float64)
        for N in NS:
            for name, fn in (("reverse_diffusion", so.predictor_reverse_diffusion), ("euler_maruyama", so.predictor_euler_maruyama)):
                o, m, _, _ = pr.predictor(t, N, x, y, s, z)
                ro, rm = fn(_t64(x), tv, _t64(y), lambda xx, tt: _t64(s), N, so.NoiseSource(replay=[_t64(z)]))
                _close(o, ro.numpy())
                _close(m, rm.numpy())
        for name, fn in (("langevin", so.corrector_langevin), ("ald", so.corrector_ald)):
            eps, e = pr.langevin_eps(s, z, SNR) if name == "langevin" else pr.ald_eps(t, SNR)
            o, m, _, _ = pr.corrector(eps, e, x, s, z)
            ro, rm = fn(_t64(x), tv, None, lambda xx, tt: _t64(s), SNR, 1, so.NoiseSource(replay=[_t64(z)]))
            _close(o, ro.numpy())
            _close(m, rm.numpy())


def test_the_two_predictors_share_one_reference():
    """The exemption of "coefficients exchanged": the reference's two predictors, evaluated in float32 as written, differ by less than the
    bound at every t and N of the cases - there is nothing for that mutation to move."""
    for shape in SHAPES:
        x, y, s, z = sde_inputs(shape)
        B = shape[0]
        for t in TS:
            tv = torch.full((B,), t, dtype=torch.float32)
            for N in NS:
                o, m, bo, bm = pr.predictor(t, N, x, y, s, z)
                for fn in (so.predictor_reverse_diffusion, so.predictor_euler_maruyama):
                    ro, rm = fn(torch.from_numpy(x), tv, torch.from_numpy(y), lambda xx, tt: torch.from_numpy(s), N,
                                so.NoiseSource(replay=[torch.from_numpy(z)]))
                    assert pr.ratio(ro.numpy(), o, *bo) < 1.0 and pr.ratio(rm.numpy(), m, *bm) < 1.0


@pytest.mark.parametrize("shape", SHAPES + ((1, 1, 33, 7), (1024, 1, 8, 1)))
def test_sde_mutations_exceed_the_bound(shape):
    x, y, s, z = sde_inputs(shape)
    eps, e = pr.langevin_eps(s, z, SNR)
    o, m, bo, bm = pr.corrector(eps, e, x, s, z)
    if shape[0] > 1:                                                       # B = 1: the mean of one norm is the norm of the mean
        eps_m, _ = pr.langevin_eps(s, z, SNR, mut="norm_of_mean")
        _, mm, _, _ = pr.corrector(eps_m, e, x, s, z)
        assert pr.ratio(mm, m, *bm) > 1.0
    mo, _, _, _ = pr.corrector(eps, e, x, s, z, mut="sqrt_eps")
    assert pr.ratio(mo, o, *bo) > 1.0
    _, mm, _, _ = pr.corrector(eps, e, x, s, z, mut="mean_with_noise")
    assert pr.ratio(mm, m, *bm) > 1.0
    for t in TS:
        for N in NS:
            o, m, bo, bm = pr.predictor(t, N, x, y, s, z)
            _, mm, _, _ = pr.predictor(t, N, x, y, s, z, mut="mean_with_noise")
            assert pr.ratio(mm, m, *bm) > 1.0


def test_a_non_finite_output_exceeds_every_bound():
    """The comparison itself: one NaN or infinity in an output, in either component, is a ratio of inf (max() would drop a NaN), and so
    is an output that was never written (the GPU tests' buffers start as NaN)."""
    re, im, b = pr.fill_noise(SEEDS[4], 0, 257)
    ref = re + 1j * im
    assert pr.ratio(ref.astype(np.complex64), ref, b, b) <= 1.0
    for bad in (complex(np.nan, 0.0), complex(0.0, np.nan), complex(np.inf, 0.0), complex(0.0, -np.inf)):
        got = ref.astype(np.complex64)
        got[100] = bad
        assert pr.ratio(got, ref, b, b) == np.inf and not pr.ratio(got, ref, b, b) <= 1.0
    assert pr.ratio(np.full(257, np.nan + 1j * np.nan, np.complex64), ref, b, b) == np.inf
    x, y, s, z = sde_inputs(SHAPES[0])
    o, m, bo, bm = pr.predictor(0.4, 30, x, y, s, z)
    got = o.astype(np.complex64)
    got[2, 0, 32, 6] = np.nan
    assert pr.ratio(got, o, *bo) == np.inf and max(0.0, pr.ratio(got, o, *bo)) == np.inf


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from universal_speech_enhancement_amd.hip_engine import HipScoreEngine
    e = HipScoreEngine(precision="fp32")
    yield e
    e.close()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


NAN = complex(float("nan"), float("nan"))


def _empty(n, fill=NAN):
    """n elements holding `fill`.  The default is NaN: an element a kernel leaves unwritten is non-finite, which pr.ratio turns into
    inf - nothing a previous test or call left in the block can stand in for a result."""
    return torch.full((n,), fill, dtype=torch.complex64, device="cuda")


def _out(n):
    """an output of n elements and one guard element behind it"""
    return _empty(n + 1)


def _host(t, shape=None):
    """the n elements of an _out(n) buffer on the host, after checking that the guard behind them is untouched"""
    a = t.cpu().numpy()
    assert np.isnan(a[-1].real) and np.isnan(a[-1].imag), "a kernel wrote past its n elements"
    return a[:-1] if shape is None else a[:-1].reshape(shape)


def _fill(eng, seed, draw, n):
    out = _empty(n + 1, complex(7.0, -7.0))
    assert eng.L.use_fill_noise(eng.h, seed, draw, out.data_ptr(), n, _stream()) == 0, eng.L.use_last_error()
    got = out.cpu().numpy()
    assert got[n] == np.complex64(complex(7.0, -7.0)), "use_fill_noise wrote past n"
    return got[:n]


@pytest.mark.gpu
def test_fill_noise_values(eng):
    worst = 0.0
    for seed in SEEDS:
        for draw in DRAWS:
            for n in SIZES:
                got = _fill(eng, seed, draw, n)
                re, im, b = pr.fill_noise(seed, draw, n)
                worst = max(worst, pr.ratio(got, re + 1j * im, b, b))
    print(f"[measured] fill_noise_kernel worst |err| / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.gpu
def test_fill_noise_past_the_grid_stride_wrap(eng):
    got = _fill(eng, SEEDS[4], 1, N_WRAP)
    re, im, b = pr.fill_noise(SEEDS[4], 1, N_WRAP)
    worst = pr.ratio(got, re + 1j * im, b, b)
    print(f"[measured] fill_noise_kernel past the wrap worst |err| / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.gpu
def test_fill_noise_items_values_and_one_item_bits(eng):
    B, n = len(ITEM_SEEDS), N_ITEM_WRAP
    out = _empty(B * n + 1, complex(7.0, -7.0))
    seeds = (C.c_uint64 * B)(*ITEM_SEEDS)
    assert eng.L.use_fill_noise_items(eng.h, seeds, B, 1, out.data_ptr(), B * n, _stream()) == 0, eng.L.use_last_error()
    got = out.cpu().numpy()
    assert got[B * n] == np.complex64(complex(7.0, -7.0))
    got = got[:B * n].reshape(B, n)
    re, im, b = pr.fill_noise_items(ITEM_SEEDS, 1, n)
    worst = pr.ratio(got, re + 1j * im, b, b)
    print(f"[measured] fill_noise_kernel per item worst |err| / bound {worst:.3f}")
    assert worst <= 1.0
    for i, s in enumerate(ITEM_SEEDS):
        assert np.array_equal(got[i].view(np.uint32), _fill(eng, s, 1, n).view(np.uint32)), f"item {i} != use_fill_noise(seeds[{i}])"


@pytest.mark.gpu
def test_prior_with_device_noise_is_draw_zero(eng):
    n = 33 * 7 * 3
    s1 = pr.ouve_std(1.0)
    re, im, b = pr.fill_noise(SEEDS[4], 0, n)
    z = re + 1j * im
    worst = 0.0
    for y in (np.zeros(n, np.complex64), sde_inputs(SHAPES[0])[1].reshape(-1)):
        x, dy = _out(n), _dev(y)
        assert eng.L.use_sde_prior(eng.h, dy.data_ptr(), None, SEEDS[4], x.data_ptr(), n, _stream()) == 0, eng.L.use_last_error()
        ref, br, bi = pr.prior(y, z, z_bound=b)
        got = _host(x)
        worst = max(worst, pr.ratio(got, ref, br, bi))
        if not y.any():                                                   # (x - y) / std(1) is the draw itself
            worst = max(worst, pr.ratio(got.astype(np.complex128) / s1, z, br / s1, bi / s1))
    print(f"[measured] prior_kernel (device noise) worst |err| / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_prior_and_predictors(eng, shape):
    x, y, s, z = sde_inputs(shape)
    n = x.size
    dx, dy, ds, dz = (_dev(a) for a in (x, y, s, z))
    out = _out(n)
    assert eng.L.use_sde_prior(eng.h, dy.data_ptr(), dz.data_ptr(), 0, out.data_ptr(), n, _stream()) == 0, eng.L.use_last_error()
    ref, br, bi = pr.prior(y, z)
    w_prior = pr.ratio(_host(out, shape), ref, br, bi)
    w_pred = 0.0
    from universal_speech_enhancement_amd import _lib
    for name in ("reverse_diffusion", "euler_maruyama"):
        for t in TS:
            for N in NS:
                xo, xm, xo2 = _out(n), _out(n), _out(n)
                args = (eng.h, _lib.PREDICTORS[name], t, N, dx.data_ptr(), dy.data_ptr(), ds.data_ptr(), dz.data_ptr(), 0)
                assert eng.L.use_sde_predictor(*args, xo.data_ptr(), xm.data_ptr(), n, _stream()) == 0, eng.L.use_last_error()
                assert eng.L.use_sde_predictor(*args, xo2.data_ptr(), None, n, _stream()) == 0, eng.L.use_last_error()
                go, gm = _host(xo, shape), _host(xm, shape)
                o, m, bo, bm = pr.predictor(t, N, x, y, s, z)
                w_pred = max(w_pred, pr.ratio(go, o, *bo), pr.ratio(gm, m, *bm))            # (a NaN anywhere: inf)
                assert np.array_equal(go.view(np.uint32), _host(xo2, shape).view(np.uint32)), "x_out depends on x_mean being asked for"
    print(f"[measured] {shape}: prior_kernel worst |err| / bound {w_prior:.3f}, predictor_kernel {w_pred:.3f}")
    assert w_prior <= 1.0 and w_pred <= 1.0


def _corrector(eng, cid, t, B, x, s, z, seed=0):
    n = x.size
    xo, xm = _out(n), _out(n)
    dx, ds, dz = _dev(x), _dev(s), None if z is None else _dev(z)          # alive until the results are read back
    zp = None if dz is None else dz.data_ptr()
    rc = eng.L.use_sde_corrector(eng.h, cid, t, SNR, B, dx.data_ptr(), ds.data_ptr(), zp, seed, xo.data_ptr(), xm.data_ptr(), n,
                                 _stream())
    assert rc == 0, eng.L.use_last_error()
    return _host(xo, x.shape), _host(xm, x.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES + ((1, 1, 33, 7), (1024, 1, 8, 1)))
def test_correctors(eng, shape):
    """Langevin (step size from the device's norms) and ALD at snr 0.5; B = 1 and B = SDE_MAX_B = 1024 items of 8 elements included.
    With x = 0 the mean is eps g: the step size on its own."""
    from universal_speech_enhancement_amd import _lib
    x, _, s, z = sde_inputs(shape)
    B = shape[0]
    eps, e = pr.langevin_eps(s, z, SNR)
    w = {}
    for label, xx in (("langevin", x), ("langevin step", np.zeros_like(x))):
        go, gm = _corrector(eng, _lib.CORRECTORS["langevin"], 0.4, B, xx, s, z)
        o, m, bo, bm = pr.corrector(eps, e, xx, s, z)
        w[label] = max(pr.ratio(go, o, *bo), pr.ratio(gm, m, *bm))
    w["ald"] = 0.0
    for t in TS:
        ea, e_a = pr.ald_eps(t, SNR)
        go, gm = _corrector(eng, _lib.CORRECTORS["ald"], t, B, x, s, z)
        o, m, bo, bm = pr.corrector(ea, e_a, x, s, z)
        w["ald"] = max(w["ald"], pr.ratio(go, o, *bo), pr.ratio(gm, m, *bm))
    # device noise: the norms kernel and the update see the z of use_fill_noise(seed, 0), bit for bit
    zdev = _fill(eng, SEEDS[4], 0, x.size).reshape(shape)
    a = _corrector(eng, _lib.CORRECTORS["langevin"], 0.4, B, x, s, None, seed=SEEDS[4])
    b = _corrector(eng, _lib.CORRECTORS["langevin"], 0.4, B, x, s, zdev)
    eps_d, e_d = pr.langevin_eps(s, zdev, SNR)
    o, m, bo, bm = pr.corrector(eps_d, e_d, x, s, zdev)
    w["langevin on device noise"] = max(pr.ratio(b[0], o, *bo), pr.ratio(b[1], m, *bm))    # every element written and right, then:
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    print(f"[measured] {shape}: corrector_kernel worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in w.items()))
    assert max(w.values()) <= 1.0


@pytest.mark.gpu
def test_refusals_launch_nothing(eng):
    """USE_E_INVALID with the argument named, and the outputs untouched."""
    from universal_speech_enhancement_amd import _lib
    L, h, n = eng.L, eng.h, 64
    x, y, s = (_dev(_cn(np.random.default_rng(i), (n,))) for i in range(3))
    sent = complex(3.0, 4.0)
    xo, xm = _empty(n, sent), _empty(n, sent)
    X, Y, S, XO, XM = (t.data_ptr() for t in (x, y, s, xo, xm))

    def refused(rc, word):
        assert rc == INVALID and word in L.use_last_error().decode(), (rc, word, L.use_last_error())
    refused(L.use_sde_prior(h, None, None, 0, XO, n, _stream()), "y is null")
    refused(L.use_sde_prior(h, Y, None, 0, None, n, _stream()), "x is null")
    refused(L.use_sde_prior(h, Y, None, 0, XO, 0, _stream()), "n=0")
    refused(L.use_sde_prior(h, Y, None, 0, XO, -5, _stream()), "n=-5")
    refused(L.use_sde_prior(None, Y, None, 0, XO, n, _stream()), "null handle")
    for k, word in enumerate(("x is null", "y is null", "score is null")):
        p = [X, Y, S]
        p[k] = None
        refused(L.use_sde_predictor(h, 0, 0.4, 30, *p, None, 0, XO, XM, n, _stream()), word)
    refused(L.use_sde_predictor(h, 0, 0.4, 30, X, Y, S, None, 0, None, XM, n, _stream()), "x_out is null")
    refused(L.use_sde_predictor(h, 0, 0.4, 30, X, Y, S, None, 0, XO, XM, 0, _stream()), "n=0")
    refused(L.use_sde_predictor(h, 99, 0.4, 30, X, Y, S, None, 0, XO, XM, n, _stream()), "predictor id 99")
    for cid in (_lib.CORRECTORS["langevin"], _lib.CORRECTORS["ald"]):
        refused(L.use_sde_corrector(h, cid, 0.4, SNR, 2, None, S, None, 0, XO, XM, n, _stream()), "x is null")
        refused(L.use_sde_corrector(h, cid, 0.4, SNR, 2, X, None, None, 0, XO, XM, n, _stream()), "score is null")
        refused(L.use_sde_corrector(h, cid, 0.4, SNR, 2, X, S, None, 0, None, XM, n, _stream()), "x_out is null")
        refused(L.use_sde_corrector(h, cid, 0.4, SNR, 2, X, S, None, 0, XO, XM, 0, _stream()), "n=0")
        refused(L.use_sde_corrector(h, cid, 0.4, SNR, 0, X, S, None, 0, XO, XM, n, _stream()), "multiple of B")
        refused(L.use_sde_corrector(h, cid, 0.4, SNR, 3, X, S, None, 0, XO, XM, n, _stream()), "multiple of B")
    refused(L.use_sde_corrector(h, 99, 0.4, SNR, 2, X, S, None, 0, XO, XM, n, _stream()), "corrector id 99")
    # B = 1025 = SDE_MAX_B + 1: the Langevin scratch holds 1024 items
    big = 1025 * 8
    bx, bs, bo = _dev(_cn(np.random.default_rng(9), (big,))), _dev(_cn(np.random.default_rng(10), (big,))), _empty(big, sent)
    refused(L.use_sde_corrector(h, _lib.CORRECTORS["langevin"], 0.4, SNR, 1025, bx.data_ptr(), bs.data_ptr(), None, 0, bo.data_ptr(), None,
                                big, _stream()), "B=1025")
    refused(L.use_fill_noise(h, 0, 0, None, n, _stream()), "")
    refused(L.use_fill_noise(h, 0, 0, XO, 0, _stream()), "")
    refused(L.use_fill_noise(h, 0, -1, XO, n, _stream()), "")
    torch.cuda.synchronize()
    for t in (xo, xm, bo):
        assert bool((t == sent).all()), "a refused call wrote to its output"
