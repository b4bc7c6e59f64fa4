"""The backward kernels (csrc/use_bwd.hip), one launch at a time through their use_op_* entry points, against plain float64 references:
the weight gradient (wgrad_tile_kernel<., float / bf16 / f16>, wgrad16_kernel, wgrad_kernel with and without atomic slices,
wgrad_reduce_kernel), GroupNorm forward / backward in the sliced form (gn_stats_part / _fin, gn_act_fwdv, gn_act_bwd_part / _fin /
_applyv) and the one-block form (gn_stats_kernel, gn_act_fwd_kernel, gn_act_bwd_reduce, gn_act_bwd_apply), gn_param_grads,
colsum_kernel, colsum_part_kernel + colsum_fin_kernel, dense_bwd_kernel and attn_bwd_rows / _cols.  Same construction as
tests/test_hip_forward_kernels.py, whose helpers (and those of tests/test_hip_conv_kernels.py) are imported.

Every reference is float64 on the operands as stored.  Every bound is per element,

    |got - ref| <= C_OUT u_out |ref| + (C_IN u_in + C_ACC 2^-24 sqrt(K)) S + E,      C_OUT = C_IN = 1, C_ACC = 2, ULP_FN = 2, ULP_DIV = 3,

S the reference expression on absolute values, K the longest serial fp32 chain the kernel has, E derived per operation below.  All
constants and derivations were written before the first GPU run; none is fitted.

Weight gradient.  Products of stored values are exact in fp32 (16-bit x 16-bit, and the fp32 MFMA is exact-fp32): C_IN = 0.  A tiled
workgroup accumulates the real pixels of its slice in one accumulator, per_slice RH CW terms (chunk positions beyond RH CW add exact
zeros); wgrad_reduce_kernel adds nslices partials serially and multiplies by alpha once:
    K = per_slice RH CW + nslices,    S = |alpha| sum |dy| |x|,    u_out = 2^-24 (the product by alpha and the store).
Bias gradient: every lane sums its half of a chunk's pixels serially (32 per chunk) in both tiled kernels, the two halves meet in one
addition, then the slices: K_b = 32 per_slice + 1 + nslices, S_b = |alpha| sum |dy|.  wgrad_kernel: a wave takes every 4th pixel pair
of its slice, four waves fold through LDS, slices meet by atomics (any order): K = per / 4 + 4 + nslices for dW and db alike; no
bit-equality claim.  The tiled kernels have no atomics: two calls give identical bits (asserted).  The structured cases (dy non-zero in
one pixel, small integers) are exact in every type: equality.

GroupNorm statistics.  Sliced form: every thread sums n_t = ceil(per / ppi) values of x and of fma(x, x, q) serially in fp32; all
later folds are fp64; mean and rstd are stored in fp32 (the reference's float64 value may round to either neighbour: 2 x 2^-24).
    d_mean = C_ACC 2^-24 sqrt(n_t) E|x| + 2 x 2^-24 |mean|
    d_var  = C_ACC 2^-24 sqrt(n_t) (E[x^2] + 2 |mean| E|x|)           (var = Q / n - m^2: dQ / n + 2 |m| dS / n)
    d_rstd = rstd d_var / (2 (var + eps)) + 2 x 2^-24 rstd
which grows with (mean / std)^2 and is carried, not absorbed: d_xhat = d_mean rstd + |x - mean| d_rstd + 2 x 2^-24 |xhat| (subtraction,
product), d_u = |gamma| d_xhat + 2^-24 |u| (one fma), d_y = d_u (act 0) or 1.1 d_u + (6 + 2 |u|) 2^-24 |silu(u)| (the forward module's
SiLU term), plus the store rounding u_out |y|.  The one-block kernels accumulate in fp64: n_t = 0.
GroupNorm backward.  g = act'(u) = s (1 + u (1 - s)), s the sigmoid with relative error r 2^-24, r = ULP_FN + 1 + ULP_DIV + 2 |u|
(exp, 1 + e, the division or v_rcp_f32, the rounded exponent argument of the fast form); 1 - s, u (1 - s), 1 + ., the product: one rounding
each; |silu''| <= 1/2:
    d_g  = d_u / 2 + 2^-24 ((r + 2) |g| + s |u| (r s + 2 (1 - s)))
    d_du = |dy| d_g + 2^-24 |du|
    d_s1 = sum_p d_du + C_ACC 2^-24 sqrt(n_t) sum_p |du| + 2^-24 |s1|
    d_s2 = sum_p (d_du |xhat| + |du| d_xhat) + (C_ACC sqrt(n_t) + 1) 2^-24 sum_p |du xhat| + 2^-24 |s2|
    d_m  = mean_group(|gamma| d_s) + 2 x 2^-24 |m|                                    (fp64 sums, one rounding to fp32)
    d_dx = d_rstd |t| + rstd (|gamma| d_du + d_m1 + d_xhat |m2| + |xhat| d_m2) + 5 x 2^-24 rstd (|gamma du| + |m1| + |xhat m2|)
           + 2^-24 (|add_scale add| + |dx|),         t = gamma du - m1 - xhat m2            (five fp32 operations, one fma)
    d_dgamma = sum_b d_s2 + 2^-24 |dgamma|,  d_dbeta = sum_b d_s1 + 2^-24 |dbeta|       (fp64 sums over B of the fp32 values)
A constant group has var = 0 and rstd = eps^-1/2; its d_var / (var + eps) is 3 E[x^2] / eps times the accumulation error.  With the
constant 1/4 that is a relative bound of 3.2 % on rstd at n_t = 8 (C_ACC 2^-24 sqrt(8) x 3/16 / 1e-6 / 2).  It is loose - sums of 1/4 are
exact in fp32, the kernel's real error there is the two store roundings - but it is what the derivation gives for arbitrary data of
that E[x^2], and it stays far below the factor 3.16 that eps = 1e-5 for 1e-6 puts on rstd, the mutation that group is there to catch.  An all-zero group (the
32-channel padding of the network) has every term zero: y = act(beta), dx = rstd gamma du - m1 rstd to rounding.
Tested range: mean / std in {0, 1, 8, 32} in all three types (at 32 the derived bound on rstd is 5e-4 relative for the 16-bit cases'
n_t = 8: the size of the fp16 output rounding, below bf16's).  tests/golden/forward_6m.npz through the oracle: the largest |mean| / std
over all GroupNorm inputs of the network is printed and asserted to lie inside the range by
test_network_groupnorm_inputs_lie_inside_the_tested_range (measured: 1.95).  mean and rstd are read back from the forward workspace and
held to d_mean / d_rstd themselves (an all-zero group has d_mean = 0: its stored mean must be exactly 0).  The comparison of the kernel's
rstd error with the error of torch's own fp32 group_norm is not made: the derived bound is asserted alone, and it held.

colsum.  Sliced: n_t fp32 serial terms per thread, then fp64, one product by the fp32 `scale` in fp64, one rounding:
2^-24 |ref| + C_ACC 2^-24 sqrt(n_t) |scale| sum |x|.  colsum_kernel is fp64 throughout: 2^-24 |ref| (n_t = 0).
dense_bwd.  fp64 accumulation: what remains is the fp32 SiLU (6 x 2^-24 |silu|) inside dW, act' (d_g with d_u = 0) and two roundings in
dtemb, one rounding in db: a few ulps.  expf(-t) overflows below t = -88.72 and the kernel's silu and silu' are 0 from there on, where the
float64 ones are up to |t| e^t = 2.6e-37: E = 92 x 2^-128 sum |g| (dW) and 92 x 2^-128 |a| (dtemb).  (Written as 2^-126 before the first
GPU run, which showed 4 .. 21 x that bound at temb in -88.7 .. -91.9, an absolute error of 2e-37: the term was corrected to the
overflow threshold; nothing else in this file followed from a measurement.)
Attention backward.  Scores and P as in the forward derivation (ds_ij, a row's relative error rp = expm1(2 ds_row) + (ULP_FN + C_ACC
sqrt(N / 128 + 7) + ULP_DIV + 1) 2^-24: the row sum is 128 strided fp32 partial sums and a 7-level tree); dP = dO v^T with K = C;
dot = sum_j P dP with the same tree; dS = P (dP - dot) cancels, so its rounding is taken of P (|dP| + |dot|):
    d_dS = rp P |dP - dot| + P (d_dP + d_dot) + 2 x 2^-24 P (|dP| + |dot|),    d_dot = sum_j (rp P |dP| + P d_dP) + C_ACC sqrt(N / 128 + 7) 2^-24 sum_j P |dP|
    d_dq = scale (sum_j d_dS |k| + C_ACC 2^-24 sqrt(N) sum_j |dS| |k|) + 6 x 2^-24 |dq|   (K = N; 6: 1 / sqrtf(C), the product, the store)
dk alike over i; d_dv = sum_i rp P |dO| + C_ACC 2^-24 sqrt(N) sum_i P |dO| + 2^-24 |dv|.  P and dS pass through HBM in fp32: no rounding.

Which case launches which kernel (the selecting condition is in the case list, `grep` finds it):
wgrad_tile_kernel<., float>: dt 0, tiled; wgrad16_kernel: dt 1 / 2 with mfma16=1 and channels % 8 == 0; wgrad_tile_kernel<., bf16 / f16>:
mfma16=0, or Cout = 36 (% 8 != 0, % 4 == 0); wgrad_kernel: tiled=False, or Cout = 34 with a workspace offered (force_work), atomic slices at [2,64,64] (8 192 pixels);
gn_stats_kernel / gn_act_fwd_kernel / gn_act_bwd_reduce / gn_act_bwd_apply: C = 34, 6 (C % 4 != 0; the forward kernel only there) and
C = 1028; colsum_kernel: work=False; colsum_part_kernel 16-bit: dt 1 / 2; `scale`: 0.70710678, -2.
test_plan_replica_reaches_every_branch holds a Python mirror of wgrad_plan / wgrad_block / wgrad_use16 / gn_slices and asserts the
branch every case reaches.

Mutation controls (-m "not gpu"): a deliberately wrong copy of each reference must exceed the bound on the GPU cases' shapes.  Exempt by
arithmetic: taps transposed / flipped / replicated border with ntaps = 1, taps transposed / flipped with H = W = 1 (only the centre tap is inside the map); replicated border where dy
is zero on the border (structured centre pixel); `alpha` missing with alpha = 1 or db null; items swapped with B = 1; "means over
channels only" with HW = 1; silu' with act = 0; `add_scale` with add null; `eps` on any but the constant group; biased / unbiased with
more than 2 000 values per group (n / (n - 1) - 1 below the bound: caught at every smaller group); "one slice dropped" with a single
slice (the mutant would be dW = 0: every structured case and the small maps; caught at every case with two or more slices);
"weight not transposed" with Cin != Cout (a shape error: caught on the square case); attention with N = 1 (dS = 0, dv = dO),
P^T with flat rows (P is constant); colsum "last pixel" needs HW > 1.

Data gradient (use_op_conv_dev, w_mode 1: pack_conv_dev_kernel writes w'[ci][co][tap] = W[co][ci][8 - tap] and the forward kernel runs on
it; w_mode 2: the NIN matrix [cin][cout]): the convolution bound of tests/test_hip_conv_kernels.py, K = C ntaps of the contraction,
    u_out |ref| + (C_IN u_in + C_ACC 2^-24 sqrt(K)) S,      S = conv(|dy|, |w'|) |scale|,
the reference being torch's float64 autograd of conv2d on the weight rounded to the storage type (x @ W for the NIN).  FIR adjoint:
training.fir under torch.autograd.grad against 4 down(g) / up(g) / 4 of the forward module's float64 FIR with its bound (the factor is a
power of two: exact).

Measured on the MI355X, worst |err| / bound per family: wgrad_tile_kernel<., float> 0.434, wgrad_tile_kernel<., bf16 / f16> 0.136,
wgrad16_kernel 0.178, wgrad_kernel 0.354 (db chains decide: dW itself stays below 0.2 - the sqrt(K) model is a worst case over 10^4
terms); GroupNorm sliced: statistics 0.284, forward 0.998, dx 0.996 (16-bit store roundings at the bottom of a binade: u |ref| itself),
dgamma / dbeta 0.141; one-block: statistics 0.494 (the fp32 rounding of mean and rstd), forward 0.445, dx 0.181, dgamma / dbeta 0.147;
colsum_part_kernel 0.270, colsum_kernel 0.979 and dense_bwd_kernel 0.992 (fp64 sums: the one fp32 rounding of the result);
attn_bwd_rows / _cols 0.070 (the bound sums the per-element terms of dS linearly over a row, and fmaf halves the roundings).
The statistics figures were taken when the stored mean of the groups with d_mean = 0 (the all-zero groups) did not yet enter the
ratio; those groups now demand a mean of exactly 0.  The data-gradient, NIN and FIR-adjoint cases have no measured figure yet.
No kernel bug found.  The CPU part takes about 20 s (most of it the oracle forward and the weight-gradient mutants); the GPU part 9 s
(159 tests), the whole `-m gpu` suite 632 s with it (620 s before; the 505 earlier tests pass and the one earlier skip is unchanged)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_hip_conv_kernels import DT_NAME, GN_EPS, SENTINEL, SQRT1_2, TAIL, TD, UNIT, q
from test_hip_conv_kernels import C_IN, C_OUT
from test_hip_forward_kernels import (REF_TOL, fir_reference, C_ACC, U32, ULP_DIV, ULP_FN, _fir2, _gen, _guarded, _lib, _measured, _ok, _p, _ratio, _set_option,
                                      _silu, _silu_err, _stream, _tail_ok)

USE_E_INVALID = -1                   # include/use_hip.h
OVF32 = 92.0 * 2.0 ** -128          # |t| e^t where expf(-t) overflows (t = -88.72): below it the fp32 SiLU and SiLU' are 0, down to -91.9 not by flushing
ROW_K = lambda N: (N + 127) // 128 + 7            # serial terms of a 128-thread strided sum and its tree


# ---------------------------------------------------------------------------------------------------------------------------
# mirror of the host-side planning in csrc/use_bwd.hip (wgrad_plan, wgrad_block, wgrad_use16, launch_wgrad, gn_slices, gn_sliced).
# A change there must be repeated here, and the case lists revisited: test_plan_replica_reaches_every_branch says which branch is lost.
# ---------------------------------------------------------------------------------------------------------------------------
WG_PX, WG_T, WH_PATCH, WG_PATCH, GN_MAX_SLICES, WGRAD_BLOCKS = 64, 64, 136, 112, 256, 512


def wgrad_use16(dt, Cout, Cin, mfma16=1):
    return dt != 0 and bool(mfma16) and Cout % 8 == 0 and Cin % 8 == 0


def wgrad_plan(B, H, W, Cout, Cin, max_patch, blocks=WGRAD_BLOCKS):
    CW = min(W, 8)
    RH = min(WG_PX // CW, H)
    while H % RH or (RH + 2) * (CW + 2) > max_patch:
        RH -= 1
    chunks_x = (W + CW - 1) // CW
    units = B * (H // RH) * chunks_x
    tiles = ((Cout + WG_T - 1) // WG_T) * ((Cin + WG_T - 1) // WG_T)
    ns = min(max(1, (blocks if blocks > 0 else WGRAD_BLOCKS) // tiles), max(1, units // 4))
    per_slice = (units + ns - 1) // ns
    return dict(RH=RH, CW=CW, chunks_x=chunks_x, units=units, per_slice=per_slice, nslices=(units + per_slice - 1) // per_slice, tiles=tiles,
                patch=(RH + 2) * (CW + 2))


def wgrad_block(L, plan):
    """workgroup id -> (tile, slice)"""
    if plan["nslices"] % 8 == 0:
        r = L >> 3
        return r % plan["tiles"], (L & 7) + 8 * (r // plan["tiles"])
    return L % plan["tiles"], L // plan["tiles"]


def wgrad_dispatch(c):
    """(kernel, plan or None, K of dW, K of db) of a weight-gradient case; kernel None: use_op_wgrad refuses."""
    B, H, W, Cout, Cin, dt = c["B"], c["H"], c["W"], c["Cout"], c["Cin"], c["dt"]
    if c["tiled"] and Cout % 4 == 0 and Cin % 4 == 0:
        m16 = wgrad_use16(dt, Cout, Cin, c["mfma16"])
        p = wgrad_plan(B, H, W, Cout, Cin, WH_PATCH if m16 else WG_PATCH, c["blocks"])
        kern = "wgrad16_kernel" if m16 else "wgrad_tile_kernel<float>" if dt == 0 else "wgrad_tile_kernel<16>"
        return kern, p, p["per_slice"] * p["RH"] * p["CW"] + p["nslices"], 32 * p["per_slice"] + 1 + p["nslices"]
    if dt != 0:
        return None, None, 0, 0
    npix = B * H * W
    ns = min(64, max(1, npix // 4096))
    per = (npix + ns - 1) // ns
    K = (per + 3) // 4 + 4 + ns
    return "wgrad_kernel", dict(nslices=ns, per=per), K, K


def gn_sliced(C_, G, dt):
    v = 4 if dt == 0 else 8
    return C_ % v == 0 and C_ // v <= 256 and C_ <= 1024 and G <= 1024


def gn_slices(HW, C_, vec):
    ppi = 256 // (C_ // vec)
    n = HW // (ppi * 8)
    return 1 if n < 1 else min(n, GN_MAX_SLICES)


def gn_chain(HW, C_, G, dt, cap=GN_MAX_SLICES):
    """(n_t, slices, ppi, threads off) of the sliced reductions; n_t = 0: the fp64 one-block kernels."""
    if not gn_sliced(C_, G, dt):
        return 0, 0, 0, 0
    vec = 4 if dt == 0 else 8
    tpp = C_ // vec
    ppi = 256 // tpp
    ns = min(cap, gn_slices(HW, C_, vec))
    per = (HW + ns - 1) // ns
    return (per + ppi - 1) // ppi, ns, ppi, 256 - tpp * ppi


# ---------------------------------------------------------------------------------------------------------------------------
# references (float64)
# ---------------------------------------------------------------------------------------------------------------------------
def _slice_mask(c, B, H, W):
    """[B,H,W] mask that is 0 on the pixels of the last pixel slice of the case's kernel (mutation "one slice dropped")."""
    kern, p, _, _ = wgrad_dispatch(c)
    m = torch.ones(B, H, W, dtype=torch.float64)
    if kern == "wgrad_kernel":
        m.view(-1)[(p["nslices"] - 1) * p["per"]:] = 0
        return m
    rows = H // p["RH"]
    for u in range((p["nslices"] - 1) * p["per_slice"], p["units"]):
        cx, rr = u % p["chunks_x"], u // p["chunks_x"]
        b, y0, x0 = rr // rows, (rr % rows) * p["RH"], cx * p["CW"]
        m[b, y0:y0 + p["RH"], x0:x0 + p["CW"]] = 0
    return m


def wgrad_reference(dy, x, ntaps, alpha, mut=None, mask=None):
    """dW[co][ci][ky][kx] = alpha sum_{b,h,w} dy[b,h,w,co] x[b,h+ky-1,w+kx-1,ci] (zero border), db[co] = alpha sum dy, on the stored
    values; alpha as the fp32 the kernel receives.  Returns (dW, S of dW, db, S of db).  Runs on the tensors' device."""
    dy, x = dy.double(), x.double()
    B, H, W, Cout = dy.shape
    Cin = x.shape[3]
    alpha = float(np.float32(alpha))
    if mut == "swap_items":
        x = x.flip(0)
    if mut == "drop_slice":
        dy = dy * mask[..., None].to(dy.device)
    dyf, dya = dy.reshape(-1, Cout).T, dy.abs().reshape(-1, Cout).T
    db, sb = dy.sum((0, 1, 2)) * (1.0 if mut == "alpha_db" else alpha), dy.abs().sum((0, 1, 2)) * abs(alpha)
    if ntaps == 1:
        return dyf @ x.reshape(-1, Cin) * alpha, dya @ x.abs().reshape(-1, Cin) * abs(alpha), db, sb
    xp = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate" if mut == "replicate" else "constant").permute(0, 2, 3, 1)
    dw = torch.empty(Cout, Cin, 3, 3, dtype=torch.float64, device=dy.device)
    s = torch.empty_like(dw)
    for ky in range(3):
        for kx in range(3):
            sy, sx = (kx, ky) if mut == "transpose" else (2 - ky, 2 - kx) if mut == "flip" else (ky, kx)
            if mut == "transpose" and (sy + H > H + 2 or sx + W > W + 2):
                raise AssertionError
            xs = xp[:, sy:sy + H, sx:sx + W].reshape(-1, Cin)
            dw[:, :, ky, kx] = dyf @ xs
            s[:, :, ky, kx] = dya @ xs.abs()
    return dw * alpha, s * abs(alpha), db, sb


def gn_reference(x, dy, add, gamma, beta, G, act, add_scale, n_t, eps=GN_EPS, mut=None):
    """act(GroupNorm(x)) and its backward on stored [B,HW,C] values, with every bound of the module docstring (without the output
    rounding).  Returns a dict of float64 tensors: y, dx [B,HW,C]; dgamma, dbeta [C]; mean, rstd [B,G]; and 'd_' + each."""
    x = x.double()
    B, HW, Cc = x.shape
    cpg = Cc // G
    n = HW * cpg
    xg = x.reshape(B, HW, G, cpg)
    e = lambda t: t[:, None, :, None]
    mean, ex2, eabs = xg.mean((1, 3)), (xg * xg).mean((1, 3)), xg.abs().mean((1, 3))
    var = ((xg - e(mean)) ** 2).mean((1, 3))
    if mut == "unbiased":
        var = var * n / max(n - 1, 1)
    if mut == "eps":
        eps = 1e-5
    eps = float(np.float32(eps))
    rstd = 1.0 / torch.sqrt(var + eps)
    ka = C_ACC * U32 * math.sqrt(n_t)
    d_mean = ka * eabs + 2 * U32 * mean.abs()
    d_var = ka * (ex2 + 2 * mean.abs() * eabs)
    d_rstd = 0.5 * d_var / (var + eps) * rstd + 2 * U32 * rstd
    M, R = e(mean), e(rstd)
    xh = (xg - M) * R
    d_xh = e(d_mean) * R + (xg - M).abs() * e(d_rstd) + 2 * U32 * xh.abs()
    gm, bt = gamma.double().reshape(1, 1, G, cpg), beta.double().reshape(1, 1, G, cpg)
    u = gm * xh + bt
    d_u = gm.abs() * d_xh + U32 * u.abs()
    if act:
        y, d_y = _silu(u), 1.1 * d_u + _silu_err(u)
    else:
        y, d_y = u, d_u
    out = dict(y=y.reshape(B, HW, Cc), d_y=d_y.reshape(B, HW, Cc), mean=mean, d_mean=d_mean, rstd=rstd, d_rstd=d_rstd)
    if dy is None:
        return out
    dyg = dy.double().reshape(B, HW, G, cpg)
    if act:
        sg = torch.sigmoid(u)
        g = sg if mut == "sigmoid" else sg * (1 + u * (1 - sg))
        r = ULP_FN + 1 + ULP_DIV + 2 * u.abs()
        d_g = 0.5 * d_u + U32 * ((r + 2) * g.abs() + sg * u.abs() * (r * sg + 2 * (1 - sg)))
    else:
        g, d_g = torch.ones_like(u), torch.zeros_like(u)
    du = dyg * g
    d_du = dyg.abs() * d_g + U32 * du.abs()
    s1, s2 = du.sum(1), (du * xh).sum(1)                                               # [B,G,cpg]
    d_s1 = d_du.sum(1) + ka * du.abs().sum(1) + U32 * s1.abs()
    d_s2 = (d_du * xh.abs() + du.abs() * d_xh).sum(1) + (ka + U32) * (du * xh).abs().sum(1) + U32 * s2.abs()
    gc = gamma.double().reshape(1, G, cpg)
    m1, m2 = (gc * s1).sum(2) / n, (gc * s2).sum(2) / n                                # [B,G]
    d_m1, d_m2 = (gc.abs() * d_s1).sum(2) / n + 2 * U32 * m1.abs(), (gc.abs() * d_s2).sum(2) / n + 2 * U32 * m2.abs()
    m1e, m2e = e(m1), e(m2)
    if mut == "chan_mean":                                                             # group means over the channels of each pixel only
        m1e, m2e = (gm * du).mean(3, keepdim=True), (gm * du * xh).mean(3, keepdim=True)
    t = gm * du - m1e - (0.0 if mut == "m2" else xh * m2e)
    dx = R * t
    d_dx = e(d_rstd) * t.abs() + R * (gm.abs() * d_du + e(d_m1) + d_xh * e(m2).abs() + xh.abs() * e(d_m2)) + \
        5 * U32 * R * ((gm * du).abs() + e(m1).abs() + (xh * e(m2)).abs())
    if add is not None:
        sc = 1.0 if mut == "add_scale" else float(np.float32(add_scale))
        av = add.double().reshape(B, HW, G, cpg)
        dx = dx + sc * av
        d_dx = d_dx + U32 * (float(np.float32(add_scale)) * av).abs()
    d_dx = d_dx + U32 * dx.abs()
    dgamma, dbeta = s2.sum(0).reshape(Cc), s1.sum(0).reshape(Cc)
    out.update(dx=dx.reshape(B, HW, Cc), d_dx=d_dx.reshape(B, HW, Cc), dgamma=dgamma, d_dgamma=d_s2.sum(0).reshape(Cc) + U32 * dgamma.abs(),
               dbeta=dbeta, d_dbeta=d_s1.sum(0).reshape(Cc) + U32 * dbeta.abs())
    return out


def colsum_reference(x, scale, n_t, mut=None):
    x = x.double()
    if mut == "last_pixel":
        x = x[:, :-1]
    sc = 1.0 if mut == "scale" else float(np.float32(scale))
    return sc * x.sum(1), C_ACC * U32 * math.sqrt(n_t) * abs(float(np.float32(scale))) * x.abs().sum(1)


def _act_grad(u):
    """(silu'(u), its fp32 evaluation error with an exact argument)"""
    sg = torch.sigmoid(u)
    g = sg * (1 + u * (1 - sg))
    r = ULP_FN + 1 + ULP_DIV + 2 * u.abs()
    return g, U32 * ((r + 2) * g.abs() + sg * u.abs() * (r * sg + 2 * (1 - sg)))


def dense_bwd_reference(g, temb, Wd, mut=None):
    """Dense_0(silu(temb)) (layerspp.py:303): (dW, db, dtemb) and their bounds without the output rounding."""
    g, temb, Wd = g.double(), temb.double(), Wd.double()
    a = _silu(temb)
    dW, pW = g.T @ a, 6 * U32 * (g.abs().T @ a.abs()) + OVF32 * g.abs().sum(0)[:, None]
    up = g @ Wd
    gr, d_gr = _act_grad(a if mut == "act_of_act" else temb)
    _, d_gr = _act_grad(temb)
    return (dW, pW), (g.sum(0), torch.zeros(g.shape[1], dtype=torch.float64)), (up * gr, up.abs() * (d_gr + U32 * gr.abs()) + OVF32 * up.abs())


def attention_bwd_reference(qq, kk, vv, dO, mut=None):
    """Backward of softmax(q k^T C^-0.5) v on stored fp32 [B,N,C] operands: ((dq, bound), (dk, bound), (dv, bound)), bounds without the
    output rounding."""
    qq, kk, vv, dO = qq.double(), kk.double(), vv.double(), dO.double()
    B, N, Cc = qq.shape
    scale = float(Cc) ** -0.5
    ein = torch.einsum
    s = ein("bic,bjc->bij", qq, kk) * scale
    p = torch.softmax(s, 2)
    ds = (C_ACC * math.sqrt(Cc) + 2 * ULP_FN) * U32 * scale * ein("bic,bjc->bij", qq.abs(), kk.abs()) + U32 * (s - s.max(2, keepdim=True).values).abs()
    kr = C_ACC * math.sqrt(ROW_K(N)) * U32
    rp = torch.expm1(2 * ds.max(2, keepdim=True).values) + kr + (ULP_FN + ULP_DIV + 1) * U32
    dP = ein("bic,bjc->bij", dO, vv)
    d_dP = C_ACC * math.sqrt(Cc) * U32 * ein("bic,bjc->bij", dO.abs(), vv.abs())
    dot = (p * dP).sum(2, keepdim=True)
    d_dot = (rp * p * dP.abs() + p * d_dP).sum(2, keepdim=True) + kr * (p * dP.abs()).sum(2, keepdim=True)
    dS = p * (dP - (0.0 if mut == "rowsum" else dot))
    d_dS = rp * p * (dP - dot).abs() + p * (d_dP + d_dot) + 2 * U32 * p * (dP.abs() + dot.abs())
    kn = C_ACC * math.sqrt(N) * U32
    dq = ein("bij,bjc->bic", dS, kk) * scale
    b_dq = scale * (ein("bij,bjc->bic", d_dS, kk.abs()) + kn * ein("bij,bjc->bic", dS.abs(), kk.abs())) + 5 * U32 * dq.abs()
    dk = ein("bij,bic->bjc", dS, qq) * (1.0 if mut == "dk_scale" else scale)
    b_dk = scale * (ein("bij,bic->bjc", d_dS, qq.abs()) + kn * ein("bij,bic->bjc", dS.abs(), qq.abs())) + 5 * U32 * dk.abs()
    dv = ein("bji,bic->bjc" if mut == "p_transposed" else "bij,bic->bjc", p, dO)
    b_dv = ein("bij,bic->bjc", rp * p, dO.abs()) + kn * ein("bij,bic->bjc", p, dO.abs())
    return (dq, b_dq), (dk, b_dk), (dv, b_dv)


def dgrad_reference(dy, w, dt, scale=1.0, mut=None):
    """dX of y = conv2d(x, w) from dy [B,H,W,Cout] (stored values): conv2d(dy, w'), w'[ci][co][ky][kx] = w[co][ci][2-ky][2-kx], the weight
    [Cout][Cin][3][3] or [Cout][Cin] rounded to the storage type; times the fp32 `scale`.  Returns (dx, S) as [B,H,W,Cin] float64."""
    dy, wq = dy.double().permute(0, 3, 1, 2), q(w.double(), dt)
    if wq.dim() == 2:
        wq = wq[:, :, None, None]
    wt = wq if mut == "no_transpose" else wq.transpose(0, 1)
    wt = wt if mut == "no_flip" else wt.flip(2, 3)
    sc = float(np.float32(scale))
    pad = wq.shape[-1] // 2
    return (F.conv2d(dy, wt, padding=pad) * sc).permute(0, 2, 3, 1), (F.conv2d(dy.abs(), wt.abs(), padding=pad) * abs(sc)).permute(0, 2, 3, 1)


def nin_reference(x, Wm, dt):
    """NIN (layers.py:639-650): x [B,H,W,Cin] @ W [Cin][Cout], the matrix rounded to the storage type."""
    Wq = q(Wm.double(), dt)
    return x.double() @ Wq, x.double().abs() @ Wq.abs()


def _conv_part(s, K, dt):
    """the convolution bound of tests/test_hip_conv_kernels.py without the output rounding (fp32 storage: nothing is rounded on the way in)"""
    return ((C_IN * UNIT[dt] if dt else 0.0) + C_ACC * U32 * math.sqrt(K)) * s


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
WGRAD_CASES = []


def _wg(dt, B, H, W, Cout, Cin, ntaps=9, db=True, alpha=0.75, tiled=True, mfma16=1, blocks=0, data="gauss", creal=None, big=False, force_work=False):
    WGRAD_CASES.append(dict(dt=dt, B=B, H=H, W=W, Cout=Cout, Cin=Cin, ntaps=ntaps, db=db, alpha=alpha, tiled=tiled, mfma16=mfma16, blocks=blocks,
                            data=data, creal=creal, big=big, force_work=force_work))


for _dt in (0, 1, 2):
    _a, _b = (36, 72) if _dt == 0 else (40, 72)
    # geometry: prime heights (RH forced to 1), H = 1, H a multiple of 3 and 5 only, W = 1, 2, 3, 5 (CW < 8), W = 9 / 20 (partial chunk in x)
    _wg(_dt, 2, 13, 9, 64, 64)
    _wg(_dt, 1, 37, 5, _a, 64, db=False)
    _wg(_dt, 3, 1, 20, 64, _b, alpha=SQRT1_2)
    _wg(_dt, 2, 15, 3, 64, 64, ntaps=1)
    _wg(_dt, 1, 64, 2, 64, 64)                                   # RH 32 under the 136-pixel patch limit, 16 under 112
    _wg(_dt, 2, 70, 1, 32, 64, creal=4)                          # the network's padded ends: Cin = 32 of which 28 are zero, Cout = 32
    _wg(_dt, 1, 1, 1, 64, 64, alpha=1.0)                         # one unit: per_slice = 1
    _wg(_dt, 1, 1, 1, 64, 64, ntaps=1, db=False)
    # channels: tiles cut by the guard, several tiles in both directions
    _wg(_dt, 2, 8, 8, 100 if _dt == 0 else 136, 136, alpha=SQRT1_2)
    _wg(_dt, 1, 8, 8, 192, 320)
    _wg(_dt, 2, 8, 12, 136, 72 if _dt else 100, ntaps=1)
    # slices (wgrad_blocks): one; 8 (the remapped workgroup order), with one tile and with four; 3 and 5 with a short last slice
    for _bl, _co in ((1, 64), (8, 64), (32, 128), (3, 64), (5, 64)):
        _wg(_dt, 2, 32, 32, _co, 128 if _co == 128 else 64, blocks=_bl, ntaps=9 if _bl != 5 else 1)
    # the bottom map of the training configuration (batch 4, 8 x 8, 256 x 256 channels)
    _wg(_dt, 4, 8, 8, 256, 256, alpha=SQRT1_2)
    if _dt:
        _wg(_dt, 2, 12, 10, 64, 64, mfma16=0)                    # wgrad_tile_kernel<., bf16 / f16>
        _wg(_dt, 2, 12, 10, 64, 64, mfma16=0, ntaps=1)
        _wg(_dt, 2, 64, 2, 64, 64, mfma16=0)                     # ... which plans under the 112-pixel limit
        _wg(_dt, 2, 12, 10, 36, 64)                              # Cout % 8 != 0, % 4 == 0: the fp32-MFMA tile kernel
    else:
        _wg(0, 2, 12, 10, 64, 64, tiled=False)                   # wgrad_kernel, one slice
        _wg(0, 2, 9, 7, 34, 66, tiled=True)                      # Cout % 4 != 0: the workspace size is 0, none is passed: wgrad_kernel
        _wg(0, 2, 9, 7, 34, 66, tiled=True, force_work=True)     # ... and wgrad_kernel although a real workspace is offered
        _wg(0, 1, 5, 3, 33, 31, tiled=False, ntaps=1, db=False)
        _wg(0, 2, 64, 64, 64, 32, tiled=False)                   # 8 192 pixels: two atomic slices
        _wg(0, 3, 64, 64, 40, 64, tiled=False, ntaps=1)          # three atomic slices
    # structured: dy non-zero in one pixel, small integers - exact in every type
    _wg(_dt, 2, 6, 7, 32, 32, alpha=0.5, data="exact")
    _wg(_dt, 2, 6, 7, 32, 32, alpha=1.0, data="exact", mfma16=0)
    # training size: half of the largest map of the training configuration (batch 4 x 512 frames: [4,512,512] at 128 channels; the float64
    # reference of the whole map is 2 x 155 Gflop and 2 GiB of operands), generated and referenced (torch float64) on the device
    _wg(_dt, 4, 256, 512, 128, 128, alpha=SQRT1_2, big=True)


def _wg_id(c):
    return (f"{DT_NAME[c['dt']]}-B{c['B']}x{c['H']}x{c['W']}-{c['Cout']}x{c['Cin']}-t{c['ntaps']}" + ("" if c["db"] else "-nodb") +
            ("" if c["tiled"] else "-tiled=False") + ("" if c["mfma16"] else "-wgrad_mfma16=0") + (f"-wgrad_blocks={c['blocks']}" if c["blocks"] else "") +
            ("" if c["data"] == "gauss" else "-" + c["data"]) + ("-big" if c["big"] else "") + ("-force_work" if c["force_work"] else ""))


EXACT_PIXELS = [(0, 0), (0, 6), (5, 0), (5, 6), (0, 3), (5, 3), (2, 0), (2, 6), (2, 3)]     # corners, edge midpoints, centre of 6 x 7


def _wg_data(c, pixel=None, device="cpu"):
    B, H, W, Cout, Cin, dt = c["B"], c["H"], c["W"], c["Cout"], c["Cin"], c["dt"]
    if c["data"] == "exact":
        x = ((torch.arange(H * W).reshape(1, H, W, 1) % 61) + (torch.arange(Cin).reshape(1, 1, 1, Cin) % 3) + torch.arange(B).reshape(B, 1, 1, 1)).float()
        dy = torch.zeros(B, H, W, Cout)
        dy[:, pixel[0], pixel[1]] = (torch.arange(Cout) % 5 + 1).float()[None] * (torch.arange(B)[:, None] + 1)
        return dy.to(TD[dt]), x.to(TD[dt])
    g = torch.Generator(device=device).manual_seed(WGRAD_CASES.index(c))
    dy = torch.randn(B, H, W, Cout, generator=g, device=device) * 0.5
    x = torch.randn(B, H, W, Cin, generator=g, device=device) + 0.25
    x[:, 0] *= 3; x[:, -1] *= 3; x[:, :, 0] *= 3; x[:, :, -1] *= 3            # a wrong border shows in the elementwise bound
    x += 0.5 * torch.arange(B, device=device).float()[:, None, None, None]
    if c["creal"]:
        x[..., c["creal"]:] = 0
    return dy.to(TD[dt]), x.to(TD[dt])


GN_CASES = []


def _gn(dt, B, HW, Cc, G, act=1, add=True, ratio=0.0, special=False):
    GN_CASES.append(dict(dt=dt, B=B, HW=HW, C=Cc, G=G, act=act, add=add, ratio=ratio, special=special))


for _dt in (0, 1, 2):
    if _dt == 0:
        _gn(0, 2, 1000, 96, 32)                    # tpp 24: 16 threads off; cpg 3 straddles the float4; 12 slices, the last short
        _gn(0, 1, 50, 384, 32, act=0)              # tpp 96: 64 threads off
        _gn(0, 2, 20, 1024, 32, add=False)         # ppi = 1
        _gn(0, 5, 37, 48, 8)                       # cpg 6; B = 5
        _gn(0, 1, 66000, 32, 32, add=False)        # cpg 1; gn_slices clamps at 256
        # the one-block fp32 kernels (reached by no other test): C % 4 != 0, C > 1 024
        _gn(0, 2, 45, 34, 17)
        _gn(0, 5, 9, 6, 3, act=0, add=False)
        _gn(0, 1, 37, 1028, 4)
        _gn(0, 2, 30, 34, 17, special=True)
    else:
        _gn(_dt, 2, 1000, 48, 24)                  # tpp 6: 4 threads off; cpg 2
        _gn(_dt, 1, 50, 384, 32, act=0)            # tpp 48: 16 threads off
        _gn(_dt, 2, 700, 8, 2, add=False)          # tpp 1
        _gn(_dt, 5, 37, 48, 8)                     # cpg 6; B = 5
        _gn(_dt, 1, 300, 48, 16)                   # cpg 3
        _gn(_dt, 1, 140000, 32, 32, add=False)     # cpg 1; gn_slices clamps at 256
        _gn(_dt, 2, 20, 1024, 32, add=False)       # tpp 128
    _gn(_dt, 3, 1, 32, 16, add=False)              # HW = 1
    _gn(_dt, 1, 5, 64, 1, act=0)                   # G = 1; HW below one slice
    for _r in (0.0, 1.0, 8.0, 32.0):               # mean / std; a constant group and an all-zero group among them
        _gn(_dt, 2, 4096, 128, 32, ratio=_r, special=True)
    _gn(_dt, 1, 4099, 64, 16, act=0, ratio=8.0, special=True)      # HW not divisible by the slice count


def _gn_id(c):
    return (f"{DT_NAME[c['dt']]}-B{c['B']}-HW{c['HW']}-C{c['C']}-G{c['G']}-act{c['act']}" + ("-add" if c["add"] else "") +
            (f"-ratio{c['ratio']:g}" if c["ratio"] else "") + ("-special" if c["special"] else ""))


GN_CONST = 0.25
ADD_SCALE = 0.70710678


def _gn_data(c):
    g = _gen(3000 + GN_CASES.index(c))
    B, HW, Cc, G, dt = c["B"], c["HW"], c["C"], c["G"], c["dt"]
    cpg = Cc // G
    sd = 1.0 + 0.5 * torch.rand(B, 1, G, 1, generator=g, dtype=torch.float64)
    x = (torch.randn(B, HW, G, cpg, generator=g, dtype=torch.float64) + c["ratio"] * torch.where(torch.rand(B, 1, G, 1, generator=g) < 0.5, -1.0, 1.0)) * sd
    if c["special"]:
        x[:, :, 0] = GN_CONST
        x[:, :, -1] = 0.0
    dy = torch.randn(B, HW, Cc, generator=g, dtype=torch.float64)
    add = torch.randn(B, HW, Cc, generator=g, dtype=torch.float64) if c["add"] else None
    gamma, beta = (torch.randn(Cc, generator=g) * 0.5 + 1.0).float(), (torch.randn(Cc, generator=g) * 0.4).float()
    return q(x.reshape(B, HW, Cc), dt), q(dy, dt), None if add is None else q(add, dt), gamma, beta


COLSUM_CASES = [dict(dt=dt, B=B, HW=HW, C=Cc, scale=sc, work=wk) for dt in (0, 1, 2) for B, HW, Cc, sc, wk in
                ((2, 1000, 96 if dt == 0 else 48, 1.0, True), (1, 50, 384, 0.70710678, True), (3, 1, 32, -2.0, True), (2, 20, 1024, -2.0, True),
                 (1, 20000 if dt == 0 else 40000, 32, 0.70710678, True), (2, 700, 8, 1.0, True))]
COLSUM_CASES += [dict(dt=0, B=B, HW=HW, C=Cc, scale=sc, work=False) for B, HW, Cc, sc in ((2, 45, 34, -2.0), (1, 1, 6, 1.0), (3, 37, 1028, 0.70710678),
                                                                                          (2, 1000, 96, 0.70710678))]
COLSUM_CASES += [dict(dt=0, B=2, HW=45, C=34, scale=-2.0, work=True)]                 # workspace offered, C % 4 != 0: colsum_kernel


def _colsum_id(c):
    return f"{DT_NAME[c['dt']]}-B{c['B']}-HW{c['HW']}-C{c['C']}-scale{c['scale']:g}-work={c['work']}"


def _colsum_chain(c):
    if not (c["work"] and gn_sliced(c["C"], 1, c["dt"])):
        return 0, 0
    n_t, ns, _, _ = gn_chain(c["HW"], c["C"], 1, c["dt"], cap=64)
    return n_t, ns


def _colsum_data(c):
    g = _gen(4000 + COLSUM_CASES.index(c))
    return q(torch.randn(c["B"], c["HW"], c["C"], generator=g, dtype=torch.float64) + 0.3, c["dt"])


# data gradient: (dt, out dt, B, H, W, forward Cout, forward Cin, ntaps, scale); w_mode 1.  Cin != Cout both ways, a square case, fp32 out of 16-bit
DGRAD_CASES = [(dt, odt, B, H, W, co, ci, nt, sc) for dt in (0, 1, 2) for odt in ((0,) if dt == 0 else (dt, 0)) for B, H, W, co, ci, nt, sc in
               ((2, 6, 5, 64, 32, 9, 1.0), (1, 9, 4, 32, 96, 9, SQRT1_2), (2, 5, 7, 64, 64, 9, 1.0), (2, 4, 6, 128, 32, 1, SQRT1_2))]
NIN_CASES = [(dt, B, H, W, ci, co) for dt in (0, 1, 2) for B, H, W, ci, co in ((2, 5, 4, 32, 64), (1, 8, 5, 96, 32), (2, 3, 3, 64, 64))]


def _dgrad_data(dt, B, H, W, co, ci, nt):
    g = _gen(7000 + co + ci + nt + dt)
    dy = torch.randn(B, H, W, co, generator=g) + 0.25 * torch.arange(B).float()[:, None, None, None]
    dy[:, 0] *= 3; dy[:, -1] *= 3; dy[:, :, 0] *= 3; dy[:, :, -1] *= 3
    w = torch.randn(co, ci, *((3, 3) if nt == 9 else (1, 1)), generator=g) / math.sqrt(co * nt)
    return dy.to(TD[dt]), w.float()


DENSE_CASES = [(1, 512, 32), (2, 512, 128), (4, 512, 256), (64, 512, 512), (2, 24, 32), (3, 50, 7)]      # (3, 50, 7): Cout K not a multiple of 256


def _dense_data(B, K, Cout):
    g = _gen(5000 + B + Cout)
    temb = torch.randn(B, K, generator=g) * 2.0
    temb[:, 0::7] = -30.0 - torch.rand(B, len(range(0, K, 7)), generator=g) * 70.0       # SiLU' tails: -30 .. -100
    temb[:, 3::7] = 30.0 + torch.rand(B, len(range(3, K, 7)), generator=g) * 70.0
    return torch.randn(B, Cout, generator=g).float(), temb.float(), (torch.randn(Cout, K, generator=g) / math.sqrt(K)).float()


ATTN_BWD_CASES = [dict(N=N, C=(32, 96, 256)[i % 3], B=(1, 3)[i % 2], kind=("ordinary", "peaked", "flat")[i % 3 if N > 2 else 0])
                  for i, N in enumerate((1, 2, 16, 64, 127, 128, 129, 300))]
ATTN_BWD_CASES += [dict(N=64, C=256, B=3, kind="ordinary"), dict(N=300, C=96, B=1, kind="peaked"), dict(N=129, C=256, B=3, kind="flat"),
                   dict(N=64, C=32, B=1, kind="peaked")]


def _attn_bwd_id(c):
    return f"attn_bwd-B{c['B']}-N{c['N']}-C{c['C']}-{c['kind']}"


def _attn_bwd_data(c):
    g = _gen(6000 + c["N"] * 5 + c["C"])
    B, N, Cc = c["B"], c["N"], c["C"]
    sd = {"ordinary": 1.4, "peaked": 3.2, "flat": 1.4}[c["kind"]]              # scores ~ N(0, sd^4): +-6 / +-30 (saturated softmax)
    r = lambda s: torch.randn(B, N, Cc, generator=g) * s
    qq, kk, vv, dO = r(sd), r(sd), r(1.0), r(1.0)
    if c["kind"] == "flat":
        kk = kk[:, :1].expand(B, N, Cc).contiguous()
    return qq.float(), kk.float(), vv.float(), dO.float()


# ---------------------------------------------------------------------------------------------------------------------------
# CPU part
# ---------------------------------------------------------------------------------------------------------------------------
def test_plan_replica_reaches_every_branch():
    """Which branch of the host-side planning every GPU case reaches, from the Python mirror above; the lists as a whole reach them all."""
    seen = set()
    for c in WGRAD_CASES:
        kern, p, K, Kb = wgrad_dispatch(c)
        assert kern is not None, _wg_id(c)
        seen.add(kern)
        if kern == "wgrad_kernel":
            seen.add("atomic" if p["nslices"] > 1 else "single")
            assert c["tiled"] is False or c["Cout"] % 4 or c["Cin"] % 4
            continue
        assert c["H"] % p["RH"] == 0 and p["patch"] <= (WH_PATCH if kern == "wgrad16_kernel" else WG_PATCH) and p["RH"] * p["CW"] <= WG_PX
        ids = sorted(wgrad_block(L, p) for L in range(p["tiles"] * p["nslices"]))
        assert ids == [(t, s) for t in range(p["tiles"]) for s in range(p["nslices"])], "wgrad_block is not a bijection"
        seen.add("remap" if p["nslices"] % 8 == 0 else "plain")
        seen.add(("remap" if p["nslices"] % 8 == 0 else "plain") + ("-tiles>1" if p["tiles"] > 1 else "-tile1"))
        if p["nslices"] == 1: seen.add("one_slice")
        if p["nslices"] * p["per_slice"] > p["units"]: seen.add("short_last_slice")
        if p["per_slice"] == 1: seen.add("per_slice1")
        if p["RH"] * p["CW"] < WG_PX: seen.add("inactive_pofs")
        if c["W"] % p["CW"]: seen.add("partial_chunk_x")
        if p["CW"] < 8: seen.add(f"CW{p['CW']}")
        if p["RH"] < min(WG_PX // p["CW"], c["H"]): seen.add("RH_shrunk")
        if p["RH"] == 1 and c["H"] > 1: seen.add("RH_prime")
        if (c["Cout"] % WG_T or c["Cin"] % WG_T): seen.add("tile_guard")
        if c["blocks"]: assert p["nslices"] == {1: 1, 8: 8, 32: 8, 3: 3, 5: 5}[c["blocks"]], (_wg_id(c), p)
        if (c["H"], c["W"]) == (64, 2):
            assert p["RH"] == (32 if kern == "wgrad16_kernel" else 16), (_wg_id(c), p)
            seen.add(f"W2-RH{p['RH']}")
        if (c["H"], c["W"]) == (70, 1): assert (p["RH"], p["CW"]) == (35, 1)
        if (c["H"], c["W"]) in ((13, 9), (37, 5)): assert p["RH"] == 1
        if (c["H"], c["W"]) == (15, 3): assert (p["RH"], p["CW"], p["patch"]) == (15, 3, 85)
    want = {"wgrad_tile_kernel<float>", "wgrad_tile_kernel<16>", "wgrad16_kernel", "wgrad_kernel", "atomic", "single", "remap-tile1", "remap-tiles>1",
            "plain-tile1", "plain-tiles>1", "one_slice", "short_last_slice", "per_slice1", "inactive_pofs", "partial_chunk_x", "CW1", "CW2", "CW3", "CW5",
            "RH_shrunk", "RH_prime", "tile_guard", "W2-RH32", "W2-RH16"}
    assert want <= seen, want - seen
    # the big cases are the README's training shape at the default wgrad_blocks
    for c in (c for c in WGRAD_CASES if c["big"]):
        _, p, _, _ = wgrad_dispatch(c)
        assert (p["RH"], p["CW"], p["tiles"], p["nslices"]) == (8, 8, 4, 128), p
    gseen = set()
    for c in GN_CASES:
        n_t, ns, ppi, off = gn_chain(c["HW"], c["C"], c["G"], c["dt"])
        cpg, vec = c["C"] // c["G"], 4 if c["dt"] == 0 else 8
        if not ns:
            assert c["dt"] == 0
            gseen.add("oneblock-C%4" if c["C"] % 4 else "oneblock-C>1024")
            continue
        if off: gseen.add("threads_off")
        if ppi == 1: gseen.add("ppi1")
        if c["C"] // vec == 1: gseen.add("tpp1")
        if vec % cpg and cpg % vec: gseen.add("straddle")
        if cpg == 1: gseen.add("cpg1")
        if c["G"] == 1: gseen.add("G1")
        if c["HW"] == 1: gseen.add("HW1")
        if ns == 1 and c["HW"] > 1: gseen.add("below_one_slice")
        if ns == GN_MAX_SLICES and c["HW"] // (ppi * 8) > GN_MAX_SLICES: gseen.add("clamp")
        if c["HW"] % ns: gseen.add("uneven_slices")
        if c["B"] == 5: gseen.add("B5")
        if c["B"] == 1: gseen.add("B1")
    gwant = {"oneblock-C%4", "oneblock-C>1024", "threads_off", "ppi1", "tpp1", "straddle", "cpg1", "G1", "HW1", "below_one_slice", "clamp", "uneven_slices",
             "B5", "B1"}
    assert gwant <= gseen, gwant - gseen
    cs = {(_colsum_chain(c)[1] == 64, bool(_colsum_chain(c)[1]), c["dt"] != 0) for c in COLSUM_CASES}
    assert (True, True, False) in cs and (True, True, True) in cs and (False, False, False) in cs       # the 64-slice cap (fp32, 16-bit); colsum_kernel


def test_references_equal_torch_float64_autograd():
    """The GroupNorm, attention, dense, weight-gradient and colsum references against torch's float64 autograd of the same operation."""
    g = _gen(9)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    close = lambda a, b: float((a - b).abs().max()) <= 1e-11 * max(1.0, float(b.abs().max()))
    for act, G, Cc in ((1, 4, 12), (0, 1, 6), (1, 6, 6)):
        B, HW = 3, 10
        x, dy, add, gamma, beta = r(B, HW, Cc) * 1.5 + 0.7, r(B, HW, Cc), r(B, HW, Cc), r(Cc), r(Cc)
        xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        y = F.group_norm(xr.permute(0, 2, 1), G, gr, br, eps=float(np.float32(GN_EPS)))
        y = F.silu(y) if act else y
        y.backward(dy.permute(0, 2, 1))
        o = gn_reference(x, dy, add, gamma, beta, G, act, 0.5, 8)
        assert close(o["y"], y.detach().permute(0, 2, 1)) and close(o["dx"], xr.grad + 0.5 * add)
        assert close(o["dgamma"], gr.grad) and close(o["dbeta"], br.grad)
        assert all(bool((o[k] >= 0).all()) for k in o if k.startswith("d_"))
    B, N, Cc = 2, 7, 5
    t = [r(B, N, Cc).requires_grad_(True) for _ in range(3)]
    dO = r(B, N, Cc)
    out = torch.softmax(t[0] @ t[1].transpose(1, 2) * Cc ** -0.5, -1) @ t[2]
    out.backward(dO)
    for (got, _), want in zip(attention_bwd_reference(t[0].detach(), t[1].detach(), t[2].detach(), dO), t):
        assert close(got, want.grad)
    gg, temb, Wd = r(3, 4), (r(3, 6) * 3).requires_grad_(True), r(4, 6).requires_grad_(True)
    bias = torch.zeros(4, dtype=torch.float64, requires_grad=True)
    F.linear(F.silu(temb), Wd, bias).backward(gg)
    (dW, _), (db, _), (dt_, _) = dense_bwd_reference(gg, temb.detach(), Wd.detach())
    assert close(dW, Wd.grad) and close(db, bias.grad) and close(dt_, temb.grad)
    for ntaps in (9, 1):
        dy, x = r(2, 4, 5, 3), r(2, 4, 5, 6)
        w = torch.zeros(3, 6, *((3, 3) if ntaps == 9 else (1, 1)), dtype=torch.float64, requires_grad=True)
        bias = torch.zeros(3, dtype=torch.float64, requires_grad=True)
        F.conv2d(x.permute(0, 3, 1, 2), w, bias, padding=ntaps // 9).backward(0.75 * dy.permute(0, 3, 1, 2))
        dw, s, db, sb = wgrad_reference(dy, x, ntaps, 0.75)
        assert close(dw.reshape(w.shape), w.grad) and close(db, bias.grad) and bool((s >= dw.abs() - 1e-12).all())


def _nhwc64(a):
    return torch.from_numpy(np.asarray(a)).double().permute(0, 2, 3, 1).contiguous()


def _rel(got, want):
    want = torch.from_numpy(np.asarray(want)).double()
    return float((got - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("name", ["plain", "widen", "down", "up"])
def test_references_compose_the_resblock_gradient_goldens(golden_dir, name):
    """The backward of ResnetBlockBigGANpp (layerspp.py:282-314) composed from this file's references as training_ops.resblock_backward
    composes it from the operators, against the gradients the reference model's own backward() produced."""
    f, gr = np.load(os.path.join(golden_dir, f"resblock_{name}.npz")), np.load(os.path.join(golden_dir, f"resblock_grads_{name}.npz"))
    W = {k[2:]: torch.from_numpy(f[k]).double() for k in f.files if k.startswith("w.")}
    x, gy, temb = _nhwc64(f["x"]), _nhwc64(gr["gy"]), torch.from_numpy(f["temb"]).double()
    B, H, Wd, Cin = x.shape
    Cout = W["Conv_0.weight"].shape[0]
    G0, G1 = min(Cin // 4, 32), min(Cout // 4, 32)
    up, down = name == "up", name == "down"
    flat = lambda t: t.reshape(B, -1, t.shape[-1])
    res = (lambda t: _fir2(t, 1 if up else 0)) if (up or down) else (lambda t: t)
    back = (lambda t: 4 * _fir2(t, 0)) if up else (lambda t: _fir2(t, 1) / 4) if down else (lambda t: t)
    gn0, gn1 = (W["GroupNorm_0.weight"], W["GroupNorm_0.bias"]), (W["GroupNorm_1.weight"], W["GroupNorm_1.bias"])
    a0r = res(gn_reference(flat(x), None, None, *gn0, G0, 1, 1.0, 0)["y"].reshape(x.shape))
    tv = _silu(temb) @ W["Dense_0.weight"].T + W["Dense_0.bias"]
    h1 = F.conv2d(a0r.permute(0, 3, 1, 2), W["Conv_0.weight"], W["Conv_0.bias"], padding=1).permute(0, 2, 3, 1) + tv[:, None, None, :]
    a1 = gn_reference(flat(h1), None, None, *gn1, G1, 1, 1.0, 0)["y"].reshape(h1.shape)
    g = {}
    g["Conv_1.weight"], _, g["Conv_1.bias"], _ = wgrad_reference(gy, a1, 9, SQRT1_2)
    da1, _ = dgrad_reference(gy, W["Conv_1.weight"], None, SQRT1_2)
    o1 = gn_reference(flat(h1), flat(da1), None, *gn1, G1, 1, 1.0, 0)
    dh1 = o1["dx"].reshape(h1.shape)
    g["GroupNorm_1.weight"], g["GroupNorm_1.bias"] = o1["dgamma"], o1["dbeta"]
    (g["Dense_0.weight"], _), (g["Dense_0.bias"], _), (g["temb"], _) = dense_bwd_reference(colsum_reference(flat(dh1), 1.0, 0)[0], temb, W["Dense_0.weight"])
    g["Conv_0.weight"], _, g["Conv_0.bias"], _ = wgrad_reference(dh1, a0r, 9, 1.0)
    da0 = back(dgrad_reference(dh1, W["Conv_0.weight"], None)[0])
    if "Conv_2.weight" in W:
        dw2, _, g["Conv_2.bias"], _ = wgrad_reference(gy, res(x), 1, SQRT1_2)
        g["Conv_2.weight"] = dw2[:, :, None, None]
        add, sc = back(dgrad_reference(gy, W["Conv_2.weight"][:, :, 0, 0], None, SQRT1_2)[0]), 1.0
    else:
        add, sc = gy, SQRT1_2
    o0 = gn_reference(flat(x), flat(da0), flat(add), *gn0, G0, 1, sc, 0)
    g["GroupNorm_0.weight"], g["GroupNorm_0.bias"] = o0["dgamma"], o0["dbeta"]
    assert _rel(o0["dx"].reshape(x.shape).permute(0, 3, 1, 2), gr["dx"]) < REF_TOL and _rel(g["temb"], gr["dtemb"]) < REF_TOL
    for k in (k[2:] for k in gr.files if k.startswith("d.")):
        assert _rel(g[k].reshape(gr["d." + k].shape), gr["d." + k]) < REF_TOL, (name, k)


def test_references_compose_the_attention_gradient_golden(golden_dir):
    """AttnBlockpp (layerspp.py:60-93) backward composed from the references as training_ops.attn_block_backward composes it."""
    f, gr = np.load(os.path.join(golden_dir, "attn.npz")), np.load(os.path.join(golden_dir, "attn_grads.npz"))
    W = {k[2:]: torch.from_numpy(f[k]).double() for k in f.files if k.startswith("w.")}
    x, gy = _nhwc64(f["x"]), _nhwc64(gr["gy"])
    B, H, Wd, Cc = x.shape
    N, G = H * Wd, min(Cc // 4, 32)
    gn = (W["GroupNorm_0.weight"], W["GroupNorm_0.bias"])
    xf, gyf = x.reshape(B, N, Cc), gy.reshape(B, N, Cc)
    h = gn_reference(xf, None, None, *gn, G, 0, 1.0, 0)["y"]
    qq, kk, vv = (nin_reference(h, W[f"NIN_{i}.W"], None)[0] + W[f"NIN_{i}.b"] for i in range(3))
    a = torch.softmax(qq @ kk.transpose(1, 2) * Cc ** -0.5, -1) @ vv
    as4 = lambda t: t.reshape(B, H, Wd, Cc)
    g = {}
    dw, _, g["NIN_3.b"], _ = wgrad_reference(gy, as4(a), 1, SQRT1_2)
    g["NIN_3.W"] = dw.T
    da, _ = dgrad_reference(gy, W["NIN_3.W"].T, None, SQRT1_2)                   # a NIN is a 1x1 convolution with the weight W^T
    dh = 0.0
    for i, (d, _) in enumerate(attention_bwd_reference(qq, kk, vv, da.reshape(B, N, Cc))):
        dw, _, g[f"NIN_{i}.b"], _ = wgrad_reference(as4(d), as4(h), 1, 1.0)
        g[f"NIN_{i}.W"] = dw.T
        dh = dh + dgrad_reference(as4(d), W[f"NIN_{i}.W"].T, None)[0]
    o = gn_reference(xf, dh.reshape(B, N, Cc), gyf, *gn, G, 0, SQRT1_2, 0)
    g["GroupNorm_0.weight"], g["GroupNorm_0.bias"] = o["dgamma"], o["dbeta"]
    assert _rel(as4(o["dx"]).permute(0, 3, 1, 2), gr["dx"]) < REF_TOL
    for k in (k[2:] for k in gr.files if k.startswith("d.")):
        want = torch.from_numpy(gr["d." + k]).double()
        if float(want.abs().max()) < 1e-6:                     # NIN_1.b: a key bias shifts every score of a row alike - analytically zero
            assert float(g[k].abs().max()) < 1e-12, k
            continue
        assert _rel(g[k], gr["d." + k]) < REF_TOL, k


def test_mutation_controls_data_gradient():
    """Weight not flipped; weight not transposed (a shape error unless Cin = Cout: the square case)."""
    for dt, odt, B, H, W, co, ci, nt, sc in DGRAD_CASES:
        dy, w = _dgrad_data(dt, B, H, W, co, ci, nt)
        w2 = w if nt == 9 else w[:, :, 0, 0]
        ref, s = dgrad_reference(dy, w2, dt, sc)
        part = _conv_part(s, co * nt, dt)
        xz = torch.zeros(B, ci, H, W, dtype=torch.float64, requires_grad=True)
        F.conv2d(xz, q(w, dt), padding=nt // 9).backward(dy.double().permute(0, 3, 1, 2) * float(np.float32(sc)))
        assert float((ref - xz.grad.permute(0, 2, 3, 1)).abs().max()) < 1e-12 * float(ref.abs().max())
        if nt == 9:
            assert _ratio(dgrad_reference(dy, w2, dt, sc, mut="no_flip")[0], ref, part, odt) > 1.0, "no_flip"
        if co == ci:
            assert _ratio(dgrad_reference(dy, w2, dt, sc, mut="no_transpose")[0], ref, part, odt) > 1.0, "no_transpose"
    assert any(c[5] == c[6] and c[7] == 9 for c in DGRAD_CASES)
    for dt, B, H, W, ci, co in NIN_CASES:
        g = _gen(7500 + ci + co + dt)
        x = (torch.randn(B, H, W, ci, generator=g) + 0.3).to(TD[dt])
        Wm = (torch.randn(ci, co, generator=g) / math.sqrt(ci)).float()
        ref, s = nin_reference(x, Wm, dt)
        if ci == co:
            assert _ratio(nin_reference(x, Wm.T.contiguous(), dt)[0], ref, _conv_part(s, ci, dt), dt) > 1.0, "nin transposed"


def test_fir_references_are_mutual_adjoints():
    """autograd(up)(g) = 4 down(g) and autograd(down)(g) = up(g) / 4 on the forward module's float64 FIR references: what
    training._Fir.backward relies on (shapes where down(up(.)) keeps the size: even maps)."""
    g = _gen(4)
    for H, W in ((6, 10), (2, 2), (14, 6)):
        x = torch.randn(2, H, W, 3, generator=g, dtype=torch.float64, requires_grad=True)
        gu = torch.randn(2, 2 * H, 2 * W, 3, generator=g, dtype=torch.float64)
        _fir2(x, 1).backward(gu)
        assert float((x.grad - 4 * _fir2(gu, 0)).abs().max()) < 1e-13
        x2 = torch.randn(2, 2 * H, 2 * W, 3, generator=g, dtype=torch.float64, requires_grad=True)
        gd = torch.randn(2, H, W, 3, generator=g, dtype=torch.float64)
        _fir2(x2, 0).backward(gd)
        assert float((x2.grad - _fir2(gd, 1) / 4).abs().max()) < 1e-13


def test_network_groupnorm_inputs_lie_inside_the_tested_range(golden_dir, monkeypatch):
    """The oracle on the golden forward case: the largest |mean| / std over every (item, group) of every GroupNorm input of the network
    lies inside the mean / std range of GN_CASES (0 .. 32)."""
    from oracle import ncsnpp_oracle as no
    from universal_speech_enhancement_amd.testing import noise as tnoise
    from universal_speech_enhancement_amd.testing import weights as tw
    from universal_speech_enhancement_amd.testing.cpu import usable_cores
    f = np.load(os.path.join(golden_dir, "forward_6m.npz"))
    worst = [0.0]
    real = F.group_norm

    def spy(x, groups, *a, **k):
        xg = x.double().reshape(x.shape[0], groups, -1)
        sd = xg.std(-1, unbiased=False)
        ok = sd > 0
        if bool(ok.any()):
            worst[0] = max(worst[0], float((xg.mean(-1).abs()[ok] / sd[ok]).max()))
        return real(x, groups, *a, **k)
    monkeypatch.setattr(F, "group_norm", spy)
    arch = tw.SMALL6M
    x = torch.from_numpy(tnoise.complex_normal(int(f["x_seed"]), "small_x", (2, 2, 512, 64))) * 0.5
    torch.set_num_threads(usable_cores())
    with torch.no_grad():
        no.ncsnpp_forward(no.to_torch(tw.make_state_dict(int(f["weights_seed"]), **arch)), x, torch.from_numpy(f["t"]), ch_mult=arch["ch_mult"],
                          num_res_blocks=arch["num_res_blocks"])
    print(f"[measured] largest |mean| / std over the network's GroupNorm inputs: {worst[0]:.2f}")
    assert 0.0 < worst[0] <= max(c["ratio"] for c in GN_CASES)


_WG_SMALL = [c for c in WGRAD_CASES if not c["big"]]


@pytest.mark.parametrize("c", _WG_SMALL, ids=[_wg_id(c) for c in _WG_SMALL])
def test_mutation_controls_wgrad(c):
    kern, p, K, Kb = wgrad_dispatch(c)
    for pixel in (EXACT_PIXELS if c["data"] == "exact" else [None]):
        dy, x = _wg_data(c, pixel)
        dw, s, db, sb = wgrad_reference(dy, x, c["ntaps"], c["alpha"])
        pw, pb = C_ACC * U32 * math.sqrt(K) * s, C_ACC * U32 * math.sqrt(Kb) * sb
        interior = pixel is not None and 0 < pixel[0] < c["H"] - 1 and 0 < pixel[1] < c["W"] - 1
        muts = ["drop_slice"] if p["nslices"] > 1 else []
        if c["ntaps"] == 9:
            muts += (["flip", "transpose"] if (c["H"], c["W"]) != (1, 1) else []) + ([] if interior else ["replicate"])
        if c["B"] > 1:
            muts.append("swap_items")
        if c["db"] and c["alpha"] != 1.0:
            muts.append("alpha_db")
        for m in muts:
            mw, _, mb, _ = wgrad_reference(dy, x, c["ntaps"], c["alpha"], mut=m, mask=_slice_mask(c, c["B"], c["H"], c["W"]) if m == "drop_slice" else None)
            if m == "alpha_db":
                assert _ratio(mb, db, pb, 0) > 1.0, m
            elif c["data"] == "exact":
                assert not torch.equal(mw, dw), (m, pixel)              # the structured cases are compared for equality
            else:
                assert _ratio(mw, dw, pw, 0) > 1.0, m


def _gn_muts(c):
    n = c["HW"] * (c["C"] // c["G"])
    return (["m2"] + (["chan_mean"] if c["HW"] > 1 else []) + (["sigmoid"] if c["act"] else []) + (["unbiased"] if n <= 2000 else []) +
            (["eps"] if c["special"] else []) + (["add_scale"] if c["add"] else []))


def _gn_bound(o, key, dt):
    return o[key], o["d_" + key], dt


@pytest.mark.parametrize("c", GN_CASES, ids=[_gn_id(c) for c in GN_CASES])
def test_mutation_controls_groupnorm(c):
    x, dy, add, gamma, beta = _gn_data(c)
    n_t = gn_chain(c["HW"], c["C"], c["G"], c["dt"])[0]
    o = gn_reference(x, dy, add, gamma, beta, c["G"], c["act"], ADD_SCALE, n_t)
    assert all(bool(torch.isfinite(v).all()) for v in o.values())
    cpg = c["C"] // c["G"]
    for m in _gn_muts(c):
        mo = gn_reference(x, dy, add, gamma, beta, c["G"], c["act"], ADD_SCALE, n_t, mut=m)
        sl = slice(0, cpg) if m == "eps" else slice(None)                      # eps: the constant group's channels
        hit = _ratio(mo["dx"][..., sl], o["dx"][..., sl], o["d_dx"][..., sl], c["dt"]) > 1.0
        if m in ("unbiased",):
            hit = hit or _ratio(mo["y"], o["y"], o["d_y"], c["dt"]) > 1.0
        assert hit, m


def test_mutation_controls_small_backward_kernels():
    for c in COLSUM_CASES:
        x = _colsum_data(c)
        ref, part = colsum_reference(x, c["scale"], _colsum_chain(c)[0])
        for m in (["scale"] if c["scale"] != 1.0 else []) + (["last_pixel"] if c["HW"] > 1 else []):
            assert _ratio(colsum_reference(x, c["scale"], 0, mut=m)[0], ref, part, 0) > 1.0, (_colsum_id(c), m)
    for B, K, Cout in DENSE_CASES:
        gg, temb, Wd = _dense_data(B, K, Cout)
        ref = dense_bwd_reference(gg, temb, Wd)[2]
        assert _ratio(dense_bwd_reference(gg, temb, Wd, mut="act_of_act")[2][0], ref[0], ref[1], 0) > 1.0, (B, K, Cout)


_ATTN_MUT = [c for c in ATTN_BWD_CASES if c["N"] > 1]


@pytest.mark.parametrize("c", _ATTN_MUT, ids=[_attn_bwd_id(c) for c in _ATTN_MUT])
def test_mutation_controls_attention_backward(c):
    qq, kk, vv, dO = _attn_bwd_data(c)
    ref = attention_bwd_reference(qq, kk, vv, dO)
    for m, idx in (("rowsum", 0), ("dk_scale", 1), ("p_transposed", 2)):
        if m == "p_transposed" and c["kind"] == "flat":
            continue
        mut = attention_bwd_reference(qq, kk, vv, dO, mut=m)
        assert _ratio(mut[idx][0], ref[idx][0], ref[idx][1], 0) > 1.0, m


# ---------------------------------------------------------------------------------------------------------------------------
# GPU part
# ---------------------------------------------------------------------------------------------------------------------------
WORST = {}


def _family(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print(f"[family] {name}: worst |err| / bound so far {WORST[name]:.3f}")


def _wgrad_call(c, dy, x, guard=True):
    """use_op_wgrad on device tensors -> (dw buffer, dw, db buffer, db), pre-filled with NaN in front of a sentinel tail."""
    L = _lib().lib()
    B, H, W, Cout, Cin, nt, dt = c["B"], c["H"], c["W"], c["Cout"], c["Cin"], c["ntaps"], c["dt"]
    wbuf, dw = _guarded((Cout, Cin, nt), torch.float32)
    bbuf, db = _guarded((Cout,), torch.float32)
    dw.fill_(float("nan")); db.fill_(float("nan"))
    n = L.use_op_wgrad_workspace(B, H, W, Cout, Cin, nt, dt) if c["tiled"] else 0
    kbuf = work = None
    if c["force_work"]:
        assert n == 0
        n = 4096
    if n:
        kbuf, work = _guarded((n,), torch.float32)
    _ok(L.use_op_wgrad(_p(dy), _p(x), dt, _p(dw), _p(db) if c["db"] else None, B, H, W, Cout, Cin, nt, c["alpha"], _p(work), n, _stream()), "use_op_wgrad")
    torch.cuda.synchronize()
    _tail_ok(wbuf, "dw"); _tail_ok(bbuf, "db")
    if kbuf is not None:
        _tail_ok(kbuf, "the workspace")
    assert bool(torch.isfinite(dw).all()), "an element of dw was not written (or is not finite)"
    assert bool(torch.isfinite(db).all()) == bool(c["db"]), "db: every element written when asked for, none otherwise"
    return dw, db


@pytest.mark.gpu
@pytest.mark.parametrize("c", WGRAD_CASES, ids=[_wg_id(c) for c in WGRAD_CASES])
def test_weight_gradient_matches_float64_reference(c):
    kern, p, K, Kb = wgrad_dispatch(c)
    dev = "cuda" if c["big"] else "cpu"
    worst = worst_b = 0.0
    try:
        _set_option("wgrad_mfma16", c["mfma16"])
        _set_option("wgrad_blocks", c["blocks"])
        for pixel in (EXACT_PIXELS if c["data"] == "exact" else [None]):
            dy, x = _wg_data(c, pixel, device=dev)
            d_dy, d_x = dy.cuda(), x.cuda()
            dw, db = _wgrad_call(c, d_dy, d_x)
            rw, s, rb, sb = wgrad_reference(dy, x, c["ntaps"], c["alpha"])
            gw, gb = dw.reshape(rw.shape).to(rw.device), db.to(rw.device)
            if c["data"] == "exact":
                assert torch.equal(gw.double(), rw), f"structured case, pixel {pixel}: not exact"
                assert not c["db"] or torch.equal(gb.double(), rb)
            else:
                worst = max(worst, _ratio(gw, rw, C_ACC * U32 * math.sqrt(K) * s, 0))
                if c["db"]:
                    worst_b = max(worst_b, _ratio(gb, rb, C_ACC * U32 * math.sqrt(Kb) * sb, 0))
                if c["creal"]:
                    assert float(gw[:, c["creal"]:].abs().max()) == 0.0, "zero padding channels in, non-zero gradient out"
            if kern != "wgrad_kernel":                           # no atomics: the same bits from a second call
                dw2, db2 = _wgrad_call(c, d_dy, d_x)
                assert torch.equal(dw, dw2) and (not c["db"] or torch.equal(db, db2)), "two calls on the same inputs differ"
    finally:
        _set_option("wgrad_mfma16", 1)
        _set_option("wgrad_blocks", 0)
    print(f"[measured] {kern} {_wg_id(c)}: K {K} dW {worst:.3f} db {worst_b:.3f}")
    _family(kern, max(worst, worst_b))
    _measured(_wg_id(c), max(worst, worst_b))


def _ratio0(err, bound):
    """worst err / bound with no output-rounding term; a zero bound demands a zero error"""
    r = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


def _gn_work(B, Cc, G):
    n = _lib().lib().use_op_gn_workspace(B, Cc, G)
    buf, work = _guarded((n,), torch.float32)
    return buf, work, 4 * B * GN_MAX_SLICES * max(Cc, G)


@pytest.mark.gpu
@pytest.mark.parametrize("c", GN_CASES, ids=[_gn_id(c) for c in GN_CASES])
def test_groupnorm_operators_match_float64_reference(c):
    L = _lib().lib()
    dt, B, HW, Cc, G, act = c["dt"], c["B"], c["HW"], c["C"], c["G"], c["act"]
    x, dy, add, gamma, beta = _gn_data(c)
    n_t, ns, _, _ = gn_chain(HW, Cc, G, dt)
    d_x, d_dy, d_add = x.to(TD[dt]).cuda(), dy.to(TD[dt]).cuda(), None if add is None else add.to(TD[dt]).cuda()
    d_g, d_b = gamma.cuda(), beta.cuda()
    ybuf, y = _guarded((B, HW, Cc), TD[dt])
    wbuf, work, off = _gn_work(B, Cc, G)
    _ok(L.use_op_gn_act_fwd(_p(d_x), dt, _p(d_g), _p(d_b), G, GN_EPS, act, B, HW, Cc, _p(work), _p(y), _stream()), "use_op_gn_act_fwd")
    torch.cuda.synchronize()
    _tail_ok(ybuf, "y"); _tail_ok(wbuf, "the workspace")
    mean, rstd = work[off:off + B * G].cpu().double().view(B, G), work[off + B * G:off + 2 * B * G].cpu().double().view(B, G)
    outs = []
    for have, wk in ((1, work), (0, _gn_work(B, Cc, G)[1])):                    # statistics reused from the forward workspace / recomputed
        xbuf, dx = _guarded((B, HW, Cc), TD[dt])
        pbuf, pg = _guarded((2, Cc), torch.float32)
        _ok(L.use_op_gn_act_bwd(_p(d_x), _p(d_dy), dt, _p(d_g), _p(d_b), G, GN_EPS, act, _p(d_add), ADD_SCALE, B, HW, Cc, _p(wk), have, _p(dx),
                                _p(pg[0]), _p(pg[1]), _stream()), "use_op_gn_act_bwd")
        torch.cuda.synchronize()
        _tail_ok(xbuf, "dx"); _tail_ok(pbuf, "dgamma / dbeta")
        outs.append((dx.cpu(), pg.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "reused and recomputed statistics give different bits"
    o = gn_reference(x, dy, add, gamma, beta, G, act, ADD_SCALE, n_t)
    got = {"y": y.cpu(), "dx": outs[0][0], "dgamma": outs[0][1][0], "dbeta": outs[0][1][1], "mean": mean, "rstd": rstd}
    ratios = {}
    for k, v in got.items():
        assert bool(torch.isfinite(v.float()).all()), k
        ratios[k] = _ratio(v, o[k], o["d_" + k], dt if k in ("y", "dx") else 0) if k not in ("mean", "rstd") else _ratio0((v - o[k]).abs(), o["d_" + k])
        assert not math.isnan(ratios[k]), k
    print(f"[measured] groupnorm {_gn_id(c)} (n_t {n_t}, slices {ns}): " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    fam = "sliced" if ns else "one-block"
    _family(f"groupnorm {fam} statistics", max(ratios["mean"], ratios["rstd"]))
    _family(f"groupnorm {fam} forward", ratios["y"])
    _family(f"groupnorm {fam} backward dx", ratios["dx"])
    _family(f"groupnorm {fam} dgamma / dbeta", max(ratios["dgamma"], ratios["dbeta"]))
    _measured(_gn_id(c), max(ratios.values()))


@pytest.mark.gpu
@pytest.mark.parametrize("c", COLSUM_CASES, ids=[_colsum_id(c) for c in COLSUM_CASES])
def test_colsum_matches_float64_reference(c):
    L = _lib().lib()
    x = _colsum_data(c)
    B, HW, Cc, dt = c["B"], c["HW"], c["C"], c["dt"]
    d_x = x.to(TD[dt]).cuda()
    obuf, out = _guarded((B, Cc), torch.float32)
    wbuf, work = _guarded((128 * B * Cc,), torch.float32) if c["work"] else (None, None)
    _ok(L.use_op_colsum(_p(d_x), dt, B, HW, Cc, c["scale"], _p(out), _p(work), _stream()), "use_op_colsum")
    torch.cuda.synchronize()
    _tail_ok(obuf, "out")
    if wbuf is not None:
        _tail_ok(wbuf, "the workspace")
    n_t, ns = _colsum_chain(c)
    ref, part = colsum_reference(x, c["scale"], n_t)
    r = _ratio(out.cpu(), ref, part, 0)
    _family("colsum_part_kernel" if ns else "colsum_kernel", r)
    _measured(_colsum_id(c), r)


@pytest.mark.gpu
@pytest.mark.parametrize("B,K,Cout", DENSE_CASES)
def test_dense_bwd_matches_float64_reference(B, K, Cout):
    L = _lib().lib()
    gg, temb, Wd = _dense_data(B, K, Cout)
    bufs = [_guarded(s, torch.float32) for s in ((Cout, K), (Cout,), (B, K))]
    d = [v.cuda() for v in (gg, temb, Wd)]
    _ok(L.use_op_dense_bwd(_p(d[0]), _p(d[1]), _p(d[2]), B, K, Cout, _p(bufs[0][1]), _p(bufs[1][1]), _p(bufs[2][1]), _stream()),
        "use_op_dense_bwd")
    torch.cuda.synchronize()
    worst = 0.0
    for (buf, got), (ref, part), what in zip(bufs, dense_bwd_reference(gg, temb, Wd), ("dW", "db", "dtemb")):
        _tail_ok(buf, what)
        assert bool(torch.isfinite(got).all()), what
        r = _ratio(got.cpu(), ref, part + (U32 * ref.abs() if what == "dtemb" else 0.0), 0)
        if what == "dtemb":
            bound = 2 * U32 * ref.abs() + part
            i = int(((got.cpu().double() - ref).abs() / bound).argmax())
            print(f"[measured] dtemb worst at temb {float(temb.view(-1)[i]):.4f}: got {float(got.view(-1)[i]):.6e} ref {float(ref.view(-1)[i]):.6e} bound {float(bound.view(-1)[i]):.3e}")
        print(f"[measured] dense_bwd_kernel B{B} K{K} Cout{Cout} {what}: {r:.3f}")
        worst = max(worst, r)
    _family("dense_bwd_kernel", worst)
    _measured(f"dense_bwd-B{B}-K{K}-Cout{Cout}", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("c", ATTN_BWD_CASES, ids=[_attn_bwd_id(c) for c in ATTN_BWD_CASES])
def test_attention_backward_matches_float64_reference(c):
    L = _lib().lib()
    B, N, Cc = c["B"], c["N"], c["C"]
    t = _attn_bwd_data(c)
    d = [v.cuda() for v in t]
    wbuf, work = _guarded((2 * B * N * N,), torch.float32)
    bufs = [_guarded((B, N, Cc), torch.float32) for _ in range(3)]
    _ok(L.use_op_attention_bwd(_p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), _p(work), _p(bufs[0][1]), _p(bufs[1][1]), _p(bufs[2][1]), B, N, Cc, _stream()),
        "use_op_attention_bwd")
    torch.cuda.synchronize()
    _tail_ok(wbuf, "the P / dS scratch")
    ratios = []
    for (buf, got), (ref, part), what in zip(bufs, attention_bwd_reference(*t), ("dq", "dk", "dv")):
        _tail_ok(buf, what)
        assert bool(torch.isfinite(got).all()), what
        ratios.append(_ratio(got.cpu(), ref, part, 0))
    print(f"[measured] {_attn_bwd_id(c)}: dq {ratios[0]:.3f} dk {ratios[1]:.3f} dv {ratios[2]:.3f}")
    _family("attn_bwd_rows / _cols", max(ratios))
    _measured(_attn_bwd_id(c), max(ratios))


@pytest.mark.gpu
def test_refusals_return_before_any_launch():
    """Every refusal is an error code from the entry point's argument checks (use_engine.cpp: each returns before the launch wrapper, or
    the launch wrapper returns false before hipLaunchKernelGGL); the message names the cause."""
    L = _lib().lib()
    z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device="cuda")

    def refused(rc, *words):
        msg = L.use_last_error().decode().lower()
        assert rc == USE_E_INVALID and all(w in msg for w in words), (rc, msg, words)
    s = _stream()
    h, f = z(4096, torch.bfloat16), z(65536)
    # use_op_wgrad
    refused(L.use_op_wgrad(_p(h), _p(h), 1, _p(f), _p(f), 1, 2, 2, 8, 8, 9, 1.0, None, 0, s), "16-bit", "workspace")
    refused(L.use_op_wgrad(_p(h), _p(h), 1, _p(f), _p(f), 1, 2, 2, 6, 8, 9, 1.0, _p(f), 65536, s), "16-bit", "multiples of 4")
    need = L.use_op_wgrad_workspace(1, 2, 2, 8, 8, 9, 0)
    assert need > 1
    refused(L.use_op_wgrad(_p(f), _p(f), 0, _p(f), _p(f), 1, 2, 2, 8, 8, 9, 1.0, _p(f), need - 1, s), "workspace too small")
    refused(L.use_op_wgrad(_p(f), _p(f), 0, _p(f), _p(f), 1, 2, 2, 8, 8, 3, 1.0, None, 0, s), "bad argument")
    refused(L.use_op_wgrad(_p(f), _p(f), 3, _p(f), _p(f), 1, 2, 2, 8, 8, 9, 1.0, None, 0, s), "dtype")
    # GroupNorm operators
    big = z(L.use_op_gn_workspace(1, 2056, 8) + 2)
    off1 = C.c_void_p(big.data_ptr() + 4)
    for C_, why in ((12, "multiple of 8"), (2056, "256")):
        xs = z(2 * C_, torch.bfloat16)
        refused(L.use_op_gn_act_fwd(_p(xs), 1, _p(f), _p(f), 4, GN_EPS, 1, 1, 2, C_, _p(big), _p(xs), s), why)
        refused(L.use_op_gn_act_bwd(_p(xs), _p(xs), 1, _p(f), _p(f), 4, GN_EPS, 1, None, 1.0, 1, 2, C_, _p(big), 0, _p(xs), _p(f), _p(f), s), why)
    refused(L.use_op_gn_act_fwd(_p(f), 0, _p(f), _p(f), 4, GN_EPS, 1, 1, 2, 8, off1, _p(f), s), "aligned")
    refused(L.use_op_gn_act_bwd(_p(f), _p(f), 0, _p(f), _p(f), 4, GN_EPS, 1, None, 1.0, 1, 2, 8, off1, 0, _p(f), _p(f), _p(f), s), "aligned")
    refused(L.use_op_gn_act_fwd(_p(f), 0, _p(f), _p(f), 3, GN_EPS, 1, 1, 2, 8, _p(big), _p(f), s), "bad argument")
    refused(L.use_op_gn_act_bwd(_p(f), _p(f), 0, _p(f), _p(f), 3, GN_EPS, 1, None, 1.0, 1, 2, 8, _p(big), 0, _p(f), _p(f), _p(f), s), "bad argument")
    for B_, HW_ in ((0, 2), (1, 0), (-1, 2)):                                    # the checks this file's pull request added
        refused(L.use_op_gn_act_fwd(_p(f), 0, _p(f), _p(f), 4, GN_EPS, 1, B_, HW_, 8, _p(big), _p(f), s), "bad argument")
        refused(L.use_op_gn_act_bwd(_p(f), _p(f), 0, _p(f), _p(f), 4, GN_EPS, 1, None, 1.0, B_, HW_, 8, _p(big), 0, _p(f), _p(f), _p(f), s), "bad argument")
    for B_, K_, Co_ in ((0, 4, 4), (2, 0, 4), (2, 4, 0), (2, -4, 4)):
        refused(L.use_op_dense_bwd(_p(f), _p(f), _p(f), B_, K_, Co_, _p(f), _p(f), _p(f), s), "bad argument")
    # use_op_colsum, use_op_attention_bwd
    refused(L.use_op_colsum(_p(h), 1, 1, 2, 8, 1.0, _p(f), None, s), "16-bit", "workspace")
    refused(L.use_op_attention_bwd(_p(f), _p(f), _p(f), _p(f), _p(f), _p(f), _p(f), _p(f), 1, 7000, 512, s), "lds")
    refused(L.use_op_attention_bwd(_p(f), _p(f), _p(f), _p(f), _p(f), _p(f), _p(f), _p(f), 1, 4, 7500, s), "lds")
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("dt,odt,B,H,W,co,ci,nt,sc", DGRAD_CASES)
def test_data_gradient_matches_float64_autograd(dt, odt, B, H, W, co, ci, nt, sc):
    """use_op_conv_dev with w_mode = 1 (the forward weight [Cout][Cin][taps] in HBM, flipped and transposed on the device) against torch's
    float64 autograd of conv2d."""
    from universal_speech_enhancement_amd import training as T
    dy, w = _dgrad_data(dt, B, H, W, co, ci, nt)
    got = T._conv_dev(dy.cuda(), w.cuda().contiguous(), None, 1, nt, ci, scale=sc, out_dtype=TD[odt])
    torch.cuda.synchronize()
    xz = torch.zeros(B, ci, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(xz, q(w, dt), padding=nt // 9).backward(dy.double().permute(0, 3, 1, 2) * float(np.float32(sc)))
    ref, s = dgrad_reference(dy, w if nt == 9 else w[:, :, 0, 0], dt, sc)
    assert float((ref - xz.grad.permute(0, 2, 3, 1)).abs().max()) < 1e-12 * float(ref.abs().max())
    assert got.dtype == TD[odt] and bool(torch.isfinite(got.float()).all())
    r = _ratio(got.cpu(), ref, _conv_part(s, co * nt, dt), odt)
    _family("data gradient (w_mode 1)", r)
    _measured(f"dgrad-{DT_NAME[dt]}-out{DT_NAME[odt]}-B{B}x{H}x{W}-{co}x{ci}-t{nt}", r)


@pytest.mark.gpu
@pytest.mark.parametrize("dt,B,H,W,ci,co", NIN_CASES)
def test_nin_layout_matches_float64_matmul(dt, B, H, W, ci, co):
    """use_op_conv_dev with w_mode = 2: the NIN matrix [cin][cout] in HBM against float64 x @ W."""
    from universal_speech_enhancement_amd import training as T
    g = _gen(7500 + ci + co + dt)
    x = (torch.randn(B, H, W, ci, generator=g) + 0.3).to(TD[dt])
    Wm = (torch.randn(ci, co, generator=g) / math.sqrt(ci)).float()
    got = T._conv_dev(x.cuda(), Wm.cuda().contiguous(), None, 2, 1, co)
    torch.cuda.synchronize()
    ref, s = nin_reference(x, Wm, dt)
    r = _ratio(got.cpu(), ref, _conv_part(s, ci, dt), dt)
    _family("NIN (w_mode 2)", r)
    _measured(f"nin-{DT_NAME[dt]}-B{B}x{H}x{W}-{ci}x{co}", r)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [0, 1, 2])
def test_fir_adjoint_through_training_fir(dt):
    """torch.autograd.grad through training.fir: backward(up)(g) = 4 down(g), backward(down)(g) = up(g) / 4, against the float64 FIR of the
    forward module with its bound; [2,6,10,32]: the halves (3, 5) are odd."""
    from universal_speech_enhancement_amd import training as T
    gen = _gen(8000 + dt)
    B, H, W, Cc = 2, 6, 10, 32
    worst = 0.0
    for up in (True, False):
        x = torch.randn(B, H, W, Cc, generator=gen).to(TD[dt]).cuda().requires_grad_(True)
        y = T.fir(x, up)
        gy = torch.randn(*y.shape, generator=gen).to(TD[dt])
        (gx,) = torch.autograd.grad(y, x, gy.cuda())
        torch.cuda.synchronize()
        raw, praw, _, _ = fir_reference(gy, None, 0, 0 if up else 1)
        f = 4.0 if up else 0.25
        assert gx.shape == x.shape
        worst = max(worst, _ratio(gx.cpu(), f * raw, f * praw, dt))
    _family("FIR adjoint (training.fir)", worst)
    _measured(f"fir-adjoint-{DT_NAME[dt]}", worst)
