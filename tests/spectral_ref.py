"""float64 references, per-element bounds and float32 emulations of the fused transforms (csrc/use_kernels.hip: stft_fwd_item,
istft_back_item, spec_map_kernel).  Used by tests/test_hip_stft_kernels.py, whose docstring carries the derivations.

Every reference takes the float32 operands the kernel reads (waveform, window, spectrogram, factor, exponent), evaluates the kernel's sums
in float64 IN THE KERNEL'S ORDER - so that the running partial sums P_i the bound needs are the reference's own - and rounds nowhere.
emulate=True evaluates the same chains with every operation rounded to float32 (an fma as one rounding of the float64 result, which is
exact for a float32 product): what the bound has to admit before a GPU is involved."""
import numpy as np
import torch

U32 = 2.0 ** -24
ULP_FN, ULP_DIV = 2.0, 3.0
LAMBDA = 7.0                    # Hoeffding: 2 exp(-LAMBDA^2 / 2) = 4.6e-11 per real component
C_COMP = 2 * ULP_FN + 2         # hypotf, powf, the product with factor, the product with S
F32 = np.float32


def window(name, N):
    """The float32 windows the product builds (sgmse/util/spectral.py): periodic Hann and its square root."""
    w = torch.hann_window(N, periodic=True)
    return (w.sqrt() if name == "sqrthann" else w).numpy()


def n_frames(L, hop):
    return 1 + L // hop


def frame_index(L, N, hop, T, mut=None):
    """sample index of (frame t, tap n) under center=True reflect padding, by index arithmetic."""
    q = np.abs(np.arange(T)[:, None] * hop + np.arange(N)[None, :] - N // 2)
    return np.where(q >= L, (2 * L - 1 if mut == "reflect" else 2 * (L - 1)) - q, q)


def _twiddle(N):
    m = np.arange(N)
    return np.cos(2 * np.pi * m / N), np.sin(2 * np.pi * m / N)


def _compress(S, expo, factor, mut=None):
    """S |S|^(e-1) factor, 0 at S = 0 (mut "power": the exponent applied to |S|^2)."""
    a = np.abs(S)
    p = 2 * expo - 1 if mut == "power" else expo - 1
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(a > 0, S * np.where(a > 0, a, 1.0) ** p * factor, 0.0)


def holder(dS, a, e):
    """|g(S + d) - g(S)| for g(z) = z |z|^(e-1), 0 < e <= 1, |d| <= dS, |S| = a: the Lipschitz constant (a - dS)^(e-1) on the segment where
    dS < a, and the Hoelder bound 2^(1-e) dS^e everywhere (the one that holds at near-zero bins)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        lin = np.where(dS < a, dS * np.where(dS < a, a - dS, 1.0) ** (e - 1), np.inf)
    return np.minimum(lin, 2 ** (1 - e) * dS ** e)


def stft_fwd(wav, win, N, hop, Tpad, expo, factor, mut=None, emulate=False, sums=True):
    """use_stft_fwd on one item: wav float32 [L] -> dict(S [F,T] before compression, Y [F,Tpad], bound [F,Tpad] on |got - Y|,
    dS [F,T], emu: the float32 emulation of Y if asked for).  sums=False: the values alone, as one matrix product (no partial sums,
    hence no bound): what a mutation control needs."""
    L, F, T = wav.shape[0], N // 2 + 1, n_frames(wav.shape[0], hop)
    assert Tpad >= T and L > N // 2
    q = frame_index(L, N, hop, T, mut)
    w = np.roll(win, 1) if mut == "win_shift" else win
    fr = wav.astype(np.float64)[q] * w.astype(np.float64)[None, :]                    # [T, N]
    cs, sn = _twiddle(N)
    k = np.arange(F)
    P = [np.zeros((F, T), np.complex128), np.zeros((F, T), np.complex128)]
    q2r, q2i = np.zeros((F, T)), np.zeros((F, T))
    if emulate:
        fr32 = (wav[q] * w[None, :]).astype(F32)                                      # one float32 product, as xs[n] = row[q] * win[n]
        cs32, sn32 = cs.astype(F32).astype(np.float64), sn.astype(F32).astype(np.float64)
        er = [np.zeros((F, T), F32), np.zeros((F, T), F32)]
        ei = [np.zeros((F, T), F32), np.zeros((F, T), F32)]
    if not sums:
        kn = np.outer(k, np.arange(N))
        if mut == "f32_angle":
            ang = (F32(2 * np.pi) * kn.astype(F32) / F32(N)).astype(np.float64)
            E = np.cos(ang) - 1j * np.sin(ang)
        else:
            E = cs[kn % N] - 1j * sn[kn % N]
        P[0] = E @ fr.T
    for n in range(N if sums else 0):
        idx = (k * n) % N
        if mut == "f32_angle":                                                        # sincosf of the unreduced float32 angle 2 pi k n / N
            ang = (F32(2 * np.pi) * (k * n).astype(F32) / F32(N)).astype(np.float64)
            c, s = np.cos(ang), np.sin(ang)
        else:
            c, s = cs[idx], sn[idx]
        x = fr[:, n][None, :]
        tr, ti = c[:, None] * x, -s[:, None] * x
        ch = n & 1
        P[ch] = P[ch] + (tr + 1j * ti)
        q2r += P[ch].real ** 2 + 2 * tr ** 2
        q2i += P[ch].imag ** 2 + 2 * ti ** 2
        if emulate:
            x32 = fr32[:, n].astype(np.float64)[None, :]
            er[ch] = (er[ch].astype(np.float64) + cs32[idx][:, None] * x32).astype(F32)
            ei[ch] = (ei[ch].astype(np.float64) - sn32[idx][:, None] * x32).astype(F32)
    S = P[0] + P[1]
    a = np.abs(S)
    dr = LAMBDA * 2.0 ** -25 * np.sqrt(q2r) + 2 * U32 * a
    di = LAMBDA * 2.0 ** -25 * np.sqrt(q2i) + 2 * U32 * a
    dS = np.hypot(dr, di)
    e64, f64 = float(F32(expo)), float(F32(factor))
    Yt = _compress(S, e64, f64, mut)
    bt = f64 * holder(dS, a, e64) + C_COMP * U32 * np.abs(Yt)
    if mut == "drop_last":
        Yt[:, T - 1] = 0
    Y, bound = np.zeros((F, Tpad), np.complex128), np.zeros((F, Tpad))
    if mut == "shift":
        Y[:, 1:min(T + 1, Tpad)] = Yt[:, :min(T, Tpad - 1)]
    else:
        Y[:, :T] = Yt
    bound[:, :T] = bt
    out = dict(S=S, Y=Y, bound=bound, dS=dS)
    if emulate:
        re, im = er[0] + er[1], ei[0] + ei[1]
        a32 = np.hypot(re, im)
        with np.errstate(divide="ignore"):
            sc = np.where(a32 > 0, np.power(np.where(a32 > 0, a32, F32(1)), F32(expo) - F32(1)) * F32(factor), F32(0)).astype(F32)
        emu = np.zeros((F, Tpad), np.complex64)
        emu[:, :T] = re * sc + 1j * (im * sc)
        out.update(emu=emu, emuS=re.astype(np.float64) + 1j * im.astype(np.float64))
    return out


def decompress(X, expo, factor):
    """(|X| / factor)^(1/e) e^{j arg X} -> (S, |dS| allowed per bin): C_DEC roundings of |S| (test module docstring)."""
    f64, p = float(F32(factor)), 1.0 / float(F32(expo))
    X = X.astype(np.complex128)
    a = np.abs(X) / f64
    with np.errstate(divide="ignore", invalid="ignore"):
        S = np.where(a > 0, X * np.where(a > 0, a, 1.0) ** (p - 1) / f64, 0.0)
    c_dec = abs(p - 1) * (ULP_FN + 2) + ULP_FN + 3
    return S, c_dec * U32 * np.abs(S)


def _decompress32(X, expo, factor):
    inv_f, p = F32(1) / F32(factor), F32(1) / F32(expo)
    re, im = X.real.astype(F32), X.imag.astype(F32)
    a = (np.hypot(re, im) * inv_f).astype(F32)
    sc = np.where(a > 0, np.power(np.where(a > 0, a, F32(1)), p - F32(1)) * inv_f, F32(0)).astype(F32)
    return (re * sc).astype(F32), (im * sc).astype(F32)


def istft_back(X, win, N, hop, L, expo, factor, mut=None, emulate=False, sums=True):
    """use_istft_back on one item: X complex64 [F, Tpad] -> dict(y [L], bound [L], env [L], x [Tpad, N] the frames' inverse transforms,
    emu: the float32 emulation of y if asked for).  sums=False: the values alone (one matrix product per item, no bound)."""
    F, Tpad = X.shape
    assert F == N // 2 + 1 and L > N // 2
    S, dS = decompress(X, expo, factor)
    cs, sn = _twiddle(N)
    n = np.arange(N)
    sign = np.ones(N) if mut == "nyq_sign" else np.where(n & 1, -1.0, 1.0)
    P = [np.zeros((Tpad, N)), np.zeros((Tpad, N))]
    q2, dec2 = np.zeros((Tpad, N)), (dS[0] ** 2 + dS[F - 1] ** 2)[:, None] * np.ones((1, N))
    if emulate:
        sr, si = _decompress32(X, expo, factor)
        cs32, sn32 = cs.astype(F32).astype(np.float64), sn.astype(F32).astype(np.float64)
        E = [np.zeros((Tpad, N), F32), np.zeros((Tpad, N), F32)]
    if not sums:
        kn = np.outer(np.arange(1, F - 1), n) % N
        P[0] = S[1:F - 1].real.T @ cs[kn] - S[1:F - 1].imag.T @ sn[kn]
    for k in range(1, F - 1) if sums else ():
        idx = (k * n) % N
        ch = (k - 1) & 1                                                              # s0: k = 1, 3, ...; s1: k = 2, 4, ...
        for term in (S[k].real[:, None] * cs[idx][None, :], -S[k].imag[:, None] * sn[idx][None, :]):
            P[ch] = P[ch] + term
            q2 += P[ch] ** 2 + 2 * term ** 2
        dec2 += (4 * dS[k] ** 2)[:, None]                                             # (2 dS_k)^2: an interior bin enters twice
        if emulate:
            E[ch] = (E[ch].astype(np.float64) + sr[k].astype(np.float64)[:, None] * cs32[idx][None, :]).astype(F32)
            E[ch] = (E[ch].astype(np.float64) - si[k].astype(np.float64)[:, None] * sn32[idx][None, :]).astype(F32)
    scale = 2.0 / N if mut == "scale" else 1.0 / N
    dc = (2.0 if mut == "dc2" else 1.0) * S[0].real
    x = (dc[:, None] + sign[None, :] * S[F - 1].real[:, None] + 2 * (P[0] + P[1])) * scale
    A = np.abs(S[0].real)[:, None] + np.abs(S[F - 1].real)[:, None] + 2 * (np.abs(P[0]) + np.abs(P[1]))
    dx = (2 * LAMBDA * 2.0 ** -25 * np.sqrt(q2) + np.sqrt(dec2) + 5 * U32 * A) / N
    w = win.astype(np.float64)
    T = n_frames(L, hop)
    acc, env, bacc, aabs = (np.zeros(L) for _ in range(4))
    if emulate:
        x32 = (sr[0][:, None] + np.where(n & 1, -sr[F - 1][:, None], sr[F - 1][:, None])).astype(F32)
        x32 = ((x32 + F32(2) * (E[0] + E[1])) * (F32(1) / F32(N))).astype(F32)
        acc32, env32 = np.zeros(L, F32), np.zeros(L, F32)
    for t in range(Tpad - 1, -1, -1):                                                 # the kernel meets the frames in descending t
        m0 = t * hop - N // 2
        lo, hi = max(0, -m0), min(N, L - m0)
        if hi <= lo:
            continue
        sl, ns = slice(m0 + lo, m0 + hi), slice(lo, hi)
        acc[sl] += w[ns] * x[t, ns]
        if not (mut == "env_T" and t >= T):
            env[sl] += np.abs(w[ns]) if mut == "env_w" else w[ns] ** 2
        bacc[sl] += np.abs(w[ns]) * dx[t, ns]
        aabs[sl] += np.abs(w[ns] * x[t, ns])
        if emulate:
            acc32[sl] = (acc32[sl].astype(np.float64) + w[ns] * x32[t, ns].astype(np.float64)).astype(F32)
            env32[sl] = (env32[sl].astype(np.float64) + w[ns] * w[ns]).astype(F32)
    assert not ((env > 1e-12) & (env < 1e-10)).any(), "an envelope value next to the kernel's 1e-11 threshold: choose another case"
    ok = env > 1e-11
    nfr = -(-N // hop)
    y = np.where(ok, acc / np.where(ok, env, 1.0), 0.0)
    bound = np.where(ok, (bacc + nfr * U32 * aabs) / np.where(ok, env, 1.0) + (ULP_DIV + nfr) * U32 * np.abs(y), 0.0)
    out = dict(y=y, bound=bound, env=env, x=x)
    if emulate:
        ok32 = env32 > F32(1e-11)
        out["emu"] = np.where(ok32, acc32 / np.where(ok32, env32, F32(1)), F32(0)).astype(F32)
    return out


def spec_map(Z, Tout, expo, factor, back, mut=None):
    """use_spec_fwd (back=False: [F,T] -> [F,Tout] compressed, zero frames behind) and use_spec_back ([F,Tpad] -> [F,Tout] first frames,
    decompressed) on one item -> (ref, bound on |got - ref|)."""
    Z = Z.astype(np.complex128)
    if back:
        ref, _ = decompress(Z[:, :Tout], expo, factor)
        p = 1.0 / float(F32(expo))
    else:
        ref = np.zeros((Z.shape[0], Tout), np.complex128)
        ref[:, :Z.shape[1]] = _compress(Z, float(F32(expo)), float(F32(factor)), mut)
        p = float(F32(expo))
    return ref, (abs(p - 1) * (ULP_FN + 2) + ULP_FN + 4) * U32 * np.abs(ref)


def ratio(err, bound):
    """worst err / bound; where the bound is 0 the value must be exact.  A non-finite error (a NaN or an infinity in the output) is inf:
    no comparison with it, and no max() over it, can come out as a pass."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    if not (np.isfinite(err).all() and np.isfinite(bound).all()):
        return float("inf")
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0
