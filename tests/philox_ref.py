"""Integer restatement of the device noise generator (csrc/use_kernels.hip: philox_round, philox_cnormal) and float64 restatements of
the element-wise SDE updates (prior_kernel, predictor_kernel, langevin_norms / langevin_step, corrector_kernel), with their per-element
bounds.  Used by tests/test_hip_sde_kernels.py; the derivations are in that module's docstring.

Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123): per round
    p0 = 0xD2511F53 * c0, p1 = 0xCD9E8D57 * c2 (64-bit products),  c <- (hi(p1) ^ c1 ^ k0, lo(p1), hi(p0) ^ c3 ^ k1, lo(p0)),
    k <- (k0 + 0x9E3779B9, k1 + 0xBB67AE85) mod 2^32,
in numpy uint64 arithmetic (every product of two 32-bit words fits).  Then the kernel's float32 steps bit for bit (np.float32 rounds to
nearest even as the device does): u = ((float)(c >> 8) + 0.5f) * 2^-24 for c0 and c1 - c >> 8 < 2^24 is exact in float32, the + 0.5f is
exact below 2^23 and rounds to even above, so u lies in (0, 1] - and the angle 6.283185307179586f * u2 as one float32 product.  What is
left to the device's libm (logf, sqrtf, sincosf and one product per component) is evaluated in float64."""
import math

import numpy as np

MASK = np.uint64(0xFFFFFFFF)
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
U32 = 2.0 ** -24
ULP_FN = 2.0
TWO_PI_F32 = np.float32(6.283185307179586)
_S32 = np.uint64(32)


def _u64(v):
    return np.asarray(v, dtype=np.uint64)


def philox4x32(counter, key, rounds=10, mut=None):
    """counter: four uint32 words (arrays broadcast), key: two -> the four output words (uint64 arrays holding 32-bit values)."""
    c = [_u64(v) & MASK for v in counter]
    k = [_u64(v) & MASK for v in key]
    m0, m1 = (M1, M0) if mut == "swap_mult" else (M0, M1)
    m0, m1 = np.uint64(m0), np.uint64(m1)
    for _ in range(rounds):
        p0, p1 = m0 * c[0], m1 * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> _S32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return c


def uniforms(seed, draw, idx, mut=None):
    """(u1, u2, angle) as float32 arrays: the kernel's values bit for bit.  idx: element indices (any integer array)."""
    idx, seed, draw = _u64(idx), int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1)
    ctr = (idx & MASK, idx >> _S32, np.uint64(draw & 0xFFFFFFFF), np.uint64(draw >> 32))
    if mut == "swap_counter":
        ctr = (ctr[2], ctr[3], ctr[0], ctr[1])
    c = philox4x32(ctr, (seed & 0xFFFFFFFF, seed >> 32), mut=mut)
    if mut == "low24":
        h0, h1 = c[0] & np.uint64(0xFFFFFF), c[1] & np.uint64(0xFFFFFF)
    else:
        h0, h1 = c[0] >> np.uint64(8), c[1] >> np.uint64(8)
    scale = np.float32(2.0 ** -24)
    u1 = (h0.astype(np.float32) + np.float32(0.5)) * scale
    u2 = (h1.astype(np.float32) + np.float32(0.5)) * scale
    return u1, u2, TWO_PI_F32 * u2


def cnormal(seed, draw, idx, mut=None):
    """float64 (re, im, bound) of philox_cnormal(seed, draw, idx).  bound: the per-component |z - z_ref| allowed."""
    u1, _, ang = uniforms(seed, draw, idx, mut)
    r = np.sqrt(-(2.0 if mut == "sqrt2log" else 1.0) * np.log(u1.astype(np.float64)))
    ang = ang.astype(np.float64)
    return r * np.cos(ang), r * np.sin(ang), (ULP_FN / 2 + 1 + ULP_FN) * U32 * r


def fill_noise(seed, draw, n, start=0):
    """use_fill_noise(seed, draw) over elements start .. start + n - 1: counter = (element index in the whole tensor, draw)."""
    return cnormal(seed, draw, np.arange(start, start + n, dtype=np.uint64))


def fill_noise_items(seeds, draw, n_per_b, idx=None, mut=None):
    """use_fill_noise_items: item b from seeds[b] with counter = (element index INSIDE the item, draw).  idx: the in-item indices to
    evaluate (default all).  -> (re, im, bound) of shape [B, len(idx)]."""
    j = np.arange(n_per_b, dtype=np.uint64) if idx is None else _u64(idx)
    out = [cnormal(s, draw, j + np.uint64(b * n_per_b if mut == "global_index" else 0)) for b, s in enumerate(seeds)]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


# ---------------------------------------------------------------------------------------------------------------------------
# OUVE SDE scalars and updates (float64 on the float32 operands the engine holds)
# ---------------------------------------------------------------------------------------------------------------------------
THETA, SIGMA_MIN, SIGMA_MAX = (float(np.float32(v)) for v in (1.5, 0.05, 0.5))     # use_config carries floats
E_CD, E_CS, E_CN = 2.0, 16.0, 8.0          # relative errors of the host's float32 coefficients in units of 2^-24 (test module docstring)
E_STD, E_ALD = 1.0, 5.0
SDE_BLOCKS = 128                           # workgroups per item of langevin_norms_kernel (use_handle::SDE_BLOCKS)


def logsig():
    return math.log(SIGMA_MAX / SIGMA_MIN)


def ouve_std(t):
    th, ls, t = THETA, logsig(), float(np.float32(t))
    return math.sqrt(SIGMA_MIN ** 2 * math.exp(-2 * th * t) * (math.exp(2 * (th + ls) * t) - 1) * ls / (th + ls))


def ouve_diffusion(t):
    t = float(np.float32(t))
    return SIGMA_MIN * (SIGMA_MAX / SIGMA_MIN) ** t * math.sqrt(2 * logsig())


def predictor_coeffs(t, N):
    """(c_drift, c_score, c_noise): x_mean = x - [c_drift (y - x) - c_score s], x_out = x_mean + c_noise z.  There is no predictor
    argument: in exact arithmetic the two predictors have the same coefficients (theta / N, g^2 / N, g / sqrt N).  The reference's two
    code paths (predictors.py:44-68) differ in the order of the float32 operations alone, which the bound's coefficient term covers."""
    g = ouve_diffusion(t)
    dt = 1.0 / N
    return THETA * dt, g * g * dt, g * math.sqrt(dt)


def prior(y, z, z_bound=None):
    """x = y + z std(1) (sdes.py:254) -> (x, bound).  z_bound: per-component error of a device-drawn z (0 for an injected one)."""
    y, z = y.astype(np.complex128), z.astype(np.complex128)
    s1 = ouve_std(1.0)
    x = y + z * s1

    def comp(yc, zc):
        b = U32 * (np.abs(yc) + (E_STD + 2) * s1 * np.abs(zc))
        return b if z_bound is None else b + s1 * z_bound * (1 + 3 * U32)
    return x, comp(y.real, z.real), comp(y.imag, z.imag)


def predictor(t, N, x, y, s, z, mut=None):
    """Either predictor (one map, see predictor_coeffs) -> (x_out, x_mean, bound_out (re, im), bound_mean (re, im)) in float64 /
    complex128."""
    x, y, s, z = (a.astype(np.complex128) for a in (x, y, s, z))
    cd, cs, cn = predictor_coeffs(t, N)
    mean = x - (cd * (y - x) - cs * s)
    out = mean + cn * z
    if mut == "mean_with_noise":
        mean = out

    def comp(xc, yc, sc, zc):
        a_d, a_s = cd * np.abs(yc - xc), cs * np.abs(sc)
        bm = U32 * (np.abs(xc) + (E_CD + 4) * a_d + (E_CS + 3) * a_s)
        return bm + U32 * (np.abs(xc) + a_d + a_s + (E_CN + 2) * cn * np.abs(zc)), bm
    bo_r, bm_r = comp(x.real, y.real, s.real, z.real)
    bo_i, bm_i = comp(x.imag, y.imag, s.imag, z.imag)
    return out, mean, (bo_r, bo_i), (bm_r, bm_i)


def langevin_eps(g, z, snr, mut=None, blocks=SDE_BLOCKS, per_item=False):
    """eps = 2 (snr mean_b ||z_b|| / mean_b ||g_b||)^2 (correctors.py:55-57) on [B, ...] complex arrays -> (eps, relative error bound in
    units of 2^-24).  blocks: the workgroups per item of langevin_norms_kernel (SDE_BLOCKS in use_sde_corrector, the plan's lang_blocks in
    the sampler loop).  per_item (use_sample_items): eps_b = 2 (snr ||z_b|| / ||g_b||)^2 as an array [B] - the mean of one norm is that
    norm, and the count of roundings is the same."""
    B = g.shape[0]
    g2, z2 = g.reshape(B, -1).astype(np.complex128), z.reshape(B, -1).astype(np.complex128)
    if mut == "norm_of_mean":
        gn, zn = np.linalg.norm(g2.mean(0)), np.linalg.norm(z2.mean(0))
    elif per_item:
        gn, zn = np.linalg.norm(g2, axis=1), np.linalg.norm(z2, axis=1)
    else:
        gn, zn = np.linalg.norm(g2, axis=1).mean(), np.linalg.norm(z2, axis=1).mean()
    snr = float(np.float32(snr))
    k = -(-g2.shape[1] // (blocks * 256))                   # serial terms per thread
    return 2.0 * (snr * zn / gn) ** 2, 2.0 * (k + 17) + 1.0


def ald_eps(t, snr):
    return 2.0 * (float(np.float32(snr)) * ouve_std(t)) ** 2, E_ALD


def corrector(eps, e_eps, x, g, z, mut=None):
    """x_mean = x + eps g, x_out = x_mean + z sqrt(2 eps) (correctors.py:60-62, 96-98) -> (x_out, x_mean, bound_out, bound_mean)."""
    x, g, z = (a.astype(np.complex128) for a in (x, g, z))
    sq = math.sqrt((1.0 if mut == "sqrt_eps" else 2.0) * eps)
    mean = x + eps * g
    out = mean + z * sq
    if mut == "mean_with_noise":
        mean = out

    def comp(xc, gc, zc):
        a_g = eps * np.abs(gc)
        bm = U32 * (np.abs(xc) + (e_eps + 2) * a_g)
        return bm + U32 * (np.abs(xc) + a_g + (e_eps / 2 + 3) * sq * np.abs(zc)), bm
    bo_r, bm_r = comp(x.real, g.real, z.real)
    bo_i, bm_i = comp(x.imag, g.imag, z.imag)
    return out, mean, (bo_r, bo_i), (bm_r, bm_i)


def ratio(got, ref, bound_re, bound_im):
    """worst |err| / bound over both components; an element with bound 0 must be exact (ratio 0 if it is, inf otherwise).  A non-finite
    output is inf: max() drops a NaN, so it never gets that far."""
    got = np.asarray(got).astype(np.complex128)
    if not (np.isfinite(got.real).all() and np.isfinite(got.imag).all()):
        return float("inf")
    worst = 0.0
    for e, b in ((np.abs(got.real - ref.real), bound_re), (np.abs(got.imag - ref.imag), bound_im)):
        b = np.broadcast_to(b, e.shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(b > 0, e / np.where(b > 0, b, 1.0), np.where(e == 0, 0.0, np.inf))
        worst = max(worst, float(r.max()) if r.size else 0.0)
    return worst
