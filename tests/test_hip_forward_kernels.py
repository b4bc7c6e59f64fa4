"""The non-convolution forward kernels of one score evaluation, one launch at a time through their use_op_* entry points, against plain
float64 references: the FIR resamplers (fir_up_blk, fir_down_blk<.,false / true>, fir_down_strip<.,8 / 4>), the attention core
(attention_kernel), the fused attention block (attn_fused_kernel), softmax_rows, transpose_nc, combine_add, temb_mlp + temb_dense,
score_out<4 / 8> and pack_input.  Same construction as tests/test_hip_conv_kernels.py, whose helpers are imported.

Every reference sees the operands the kernel sees (inputs as stored, weights rounded to the storage type where the kernel reads them in
it) and rounds where the kernel rounds and nowhere else.  Every bound is per element,

    |got - ref| <= C_OUT u_out |ref| + (C_IN u_in + C_ACC 2^-24 sqrt(K)) S + E,        C_OUT = C_IN = 1, C_ACC = 2,

u = unit roundoff of the type (2^-24 / 2^-8 / 2^-11), S the reference's expression on absolute values, K the number of serially
accumulated terms, E an operation-specific term derived below.  All constants were fixed before any GPU run; none is fitted.

fp16 results below 2^-14 are subnormal, spaced 2^-24 apart: every fp16 output rounding is u_out |ref| + 2^-25 (first GPU run of this file:
fir_up_blk fp16 measured 40 x a bound without that term, at an output of ~1e-6; no other change followed from a measurement).

Assumptions on the device functions (no accuracy figure in the programming guides; the source calls them "1 ulp-class"):
ULP_FN = 2 fp32 ulps for each of v_exp_f32, v_rcp_f32, expf, logf, sinf, cosf, rsqrtf and 3 for an fp32 division.

SiLU.  y = x rcp(1 + exp2(-x log2 e)): the exponent t = -x log2(e) is rounded once and the constant is a rounding itself, an absolute
exponent error of 2 |t| 2^-24 -> relative (2 ln 2 |t|) 2^-24 < 2 |x| 2^-24 on e = exp2(t), plus ULP_FN; the sigmoid s = 1 / (1 + e) takes
(1 - s) of that, the addition one rounding, rcp ULP_FN, the product one:  |dy| <= (2 ULP_FN + 2 + 2 |x|) 2^-24 |y| = (6 + 2 |x|) 2^-24 |y|.
The affine u = fma(x, a, b) in front is one rounding of at most 2^-24 (|x a| + |b|), which SiLU (|silu'| <= 1.1) passes on.  At the
largest pre-activations of the cases (|u| ~ 25) this is 56 x 2^-24 = 3.3e-6 relative: 1 170 times below the bf16 output rounding
(2^-8 = 3.9e-3) and 146 times below fp16's (2^-11): the ULP_FN assumption decides no 16-bit case.

FIR (K = 16 taps down, 4 up; weights exact in binary).  out_act = FIR(silu(a x + b)) with the activation kept in fp32 (C_IN = 0: nothing
is rounded to the storage type before the filter), one rounding at the store:
    bound = u_out |ref| + FIR(C_ACC 2^-24 sqrt(K) |act| + e_act),      e_act = 1.1 x 2^-24 (|x a| + |b|) + (6 + 2 |u|) 2^-24 |silu(u)|
(S = FIR(|act|) and E = FIR(e_act) folded into one filter pass by linearity; the weights are positive).  Down-sampling passes every
product through 8 serial roundings (4 horizontal, 4 vertical), up-sampling through 4: C_ACC sqrt(K) = 8 / 4 ulps of S, the worst case.

Attention core (K = C for the scores, N for P v).  A score carries ds_ij = (C_ACC sqrt(C) + 2 ULP_FN) 2^-24 scale sum_c |q_ic| |k_jc|
(accumulation, rsqrtf, the product) + 2^-24 |s_ij - max_i| (the subtraction in front of expf); a change of every score of a row by at
most ds_row = max_j ds_ij changes a probability by at most expm1(2 ds_row) p ~ 2 ds_row p.  With expf (ULP_FN), the row sum, 1 / sum
(3) and the product (1):
    bound = u_out |ref| + (expm1(2 ds_row) + (C_ACC sqrt(N) + 2 ULP_FN + 4) 2^-24) sum_j p_j |v_j|.

Fused block (use_attn.hip's rounding points: h, q, k, v, P, O in the storage type; scores and softmax fp32).  The reference rounds at the
same points.  The kernel rounds y + d where the reference rounds y (d: what the fp32 arithmetic in front and the inherited differences
add up to, |d| <= e_pre).  The two roundings agree unless y lies within e_pre of a rounding boundary, and there they differ by at most
e_pre + one spacing of the storage type: flip(y, e_pre), evaluated element by element on the reference's own float64 y - zero for all
but the elements near a boundary (1e-3 .. 4e-2 of h, q, k, v; most of P and O, whose e_pre is of the size of a bf16 spacing).
These differences are rounding events of separate elements, of either sign: a contraction passes them on as the root of the sum of
squares, rss(d, w)_j = sqrt(sum_c d_c^2 w_jc^2) - the probabilistic model behind the sqrt(K) of the accumulation term.  (Their linear
sum, every element off in the direction that hurts, gives a bound of 0.3 .. 13 |H| in bf16, which says nothing.)  The probabilities of
a row are tied together by the normalisation, so dP enters P v linearly.
    dh = flip(a x + b, 8 x 2^-24 (|x a| + |b|))        (8: rsqrt + Newton step, the two roundings of (a, b), the fma)
    d{q,k,v} = flip(h W^T + bias, rss(dh, W) + C_ACC 2^-24 sqrt(C) (|h| |W|^T + |bias|))
    ds_ij = scale sqrt(rss(dq_i, k_j)^2 + rss(q_i, dk_j)^2) + (C_ACC sqrt(C) + 2 ULP_FN) 2^-24 scale (|q| |k|^T)_ij + 2^-24 |s_ij - max_i|
    dP = flip(p, (expm1(2 ds_row) + (2 ULP_FN + 4) 2^-24) p);   dO = flip(P v, dP |v| + rss(P, dv) + C_ACC 2^-24 sqrt(N) P |v|)
    dH = rss(dO, Wo) + C_ACC 2^-24 sqrt(C) (|O| |Wo|^T + |bo|);   bound(out) = u_out |ref| + (dH + 2 x 2^-24 (|x| + |H|)) / sqrt 2
GroupNorm coefficients come from the fixed-point totals the kernel reads (float64 arithmetic on the same integers).  h = out sqrt 2 - x is reconstructed in float64
from the stored out and held to sqrt 2 bound(out) against the reference's H: the cases scale NIN_3 so that |H| ~ 3 |x|, hence the
output rounding u_out |out| is one of H's own size and an error of the attention cannot hide behind the residual.  Output totals: the
kernel sums its fp32 values (u_out each from the stored ones), at most 48 per lane serially, one fixed-point rounding per channel.

softmax_rows: bound = (u_out + (ULP_FN + |x_j - max|) 2^-24 + sum_k p_k (ULP_FN + |x_k - max|) 2^-24 + (cols / 256 + 10 + 4) 2^-24) p_j
(+ 2^-25 absolute in fp16: subnormal results).  transpose_nc, pack_input: bit-exact.
combine_add (K = 10: h, bias, 8 products): u_out |ref| + C_ACC 2^-24 sqrt(10) S; totals: sums of the stored values, at most 64 terms per
workgroup serially (64 x 2^-24 sum |v|), one fixed-point rounding (2^-21) per 64-pixel workgroup and channel.
temb_mlp (K = 2 nf, 4 nf): the Fourier argument xp = log(t) w 2 pi carries (ULP_FN + 2.5) 2^-24 |xp| (logf, two products, the fp32 pi),
a feature that plus ULP_FN 2^-24; da1 = |W1| dfeat + C_ACC 2^-24 sqrt(2 nf) (|b1| + |W1| |feat|); SiLU as above; the same for layer 2.
temb_dense (K = dim): 2^-24 |ref| + C_ACC 2^-24 sqrt(dim) (|bias| + |W| |x|).
score_out (K = PC): 2^-24 |ref| + (3 + C_ACC sqrt(PC)) 2^-24 (|b| + sum |w| |h| / t)      (3: the division).

`-m "not gpu"` checks the references against what already pins the project (fir.npz, attn.npz, the oracle's functions) and runs the
mutation controls: a deliberately wrong copy of each reference must exceed the bound on the GPU cases' shapes.  Exempt by arithmetic:
N = 1 (the output is v), flat rows under the scale mutation (the softmax does not depend on the scale), N % 32 == 0 under the
padding-token mutation (there are no padding tokens), cols = 1, act = 0 under "activation after the filter".  Exempt by precision: bf16
N = 95 under the padding-token mutation - one zero key of 96 moves the output by 0.56 of the bound (0.45 with three items), less than the
bf16 roundings of P and O that the bound has to allow; the same mutation is caught in fp16 at N = 95 (1.46) and in bf16 at N = 1 .. 80.
The strip kernel's grid-stride wrap is reached with 4-row strips ([7,512,640,128]); with 8-row strips it takes 13 items and is left out.

Measured on the MI355X, worst |err| / bound per family: fir_up_blk 0.999, fir_down_blk 0.998, fir_down_strip 0.996, softmax_rows 0.999,
combine_add 0.998 (kernels whose error is the store rounding: half a spacing at the bottom of a binade is u |ref| itself), attention_kernel
0.974, attn_fused_kernel 0.49 on out and h (0.955 on the totals at N = 1, where the one summed fp32 value is u_out from the stored one),
score_out 0.37, temb_dense 0.014, temb_mlp 0.006.  The CPU part takes about 4 s."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_hip_conv_kernels import DT_NAME, GN_EPS, SENTINEL, SQRT1_2, TAIL, TD, UNIT, gn_coef_reference, q

C_OUT, C_IN, C_ACC = 1.0, 1.0, 2.0
U32 = 2.0 ** -24
ULP_FN, ULP_DIV = 2.0, 3.0
SQRT2 = math.sqrt(2.0)
INVALID = -1


def _silu(x):
    return x / (1.0 + torch.exp(-x))


def _silu_err(u):
    """|error| of the device SiLU at pre-activation u (module docstring)."""
    return (2 * ULP_FN + 2 + 2 * u.abs()) * U32 * _silu(u).abs()


# ---------------------------------------------------------------------------------------------------------------------------
# references (float64)
# ---------------------------------------------------------------------------------------------------------------------------
def _pad_axis(x, axis, lo, hi, replicate=False):
    """lo / hi border elements along `axis`: zeros, or (replicate) copies of the edge."""
    first, last = x.narrow(axis, 0, 1), x.narrow(axis, x.shape[axis] - 1, 1)
    rep = [1] * x.dim()
    rep[axis] = lo
    front = first.repeat(rep)
    rep[axis] = hi
    back = last.repeat(rep)
    if not replicate:
        front, back = torch.zeros_like(front), torch.zeros_like(back)
    return torch.cat([front, x, back], axis)


def _fir1(x, axis, up, mut=None):
    """[1,3,3,1] x2 resampling along one axis with zero borders (up_or_down_sampling.py:202-264: upsample_2d = zero-stuffing, pad (2, 1),
    kernel * 4; downsample_2d = pad (1, 1), stride 2), as shifted slices.  mut: a deliberately wrong variant (mutation controls)."""
    n = x.shape[axis]
    p = _pad_axis(x, axis, 1, 2, replicate=(mut == "replicate"))
    if up:
        w0, w1 = (0.75, 0.25) if mut == "swap" else (0.25, 0.75)
        xm, x0, xp = p.narrow(axis, 0, n), p.narrow(axis, 1, n), p.narrow(axis, 2, n)
        even = w0 * xm + w1 * x0
        odd = (0.0 if mut == "drop" else w1) * x0 + w0 * xp                        # (drop: a tap that is inside the map at every size)
        shape = list(x.shape); shape[axis] = 2 * n
        return torch.stack([even, odd], axis + 1).reshape(shape)
    on = n // 2
    every2nd = (slice(None),) * axis + (slice(None, None, 2),)
    t = [p.narrow(axis, k, 2 * on - 1)[every2nd] for k in range(4)]               # p[k + 2 o], o < on
    return (t[0] + (0.0 if mut == "drop" else 3.0) * t[1] + 3.0 * t[2] + t[3]) / 8.0


def _fir2(x, up, mut=None):
    """x [B,H,W,C] -> [B,2H,2W,C] or [B,H/2,W/2,C]"""
    return _fir1(_fir1(x, 2, up, mut), 1, up, None if mut == "drop" else mut)


def fir_reference(x, coef, act, up, mut=None):
    """float64 reference of use_op_fir on the stored values x [B,H,W,C]; coef [B,C,2] or None.  Returns (raw, bound part of raw, act,
    bound part of act): out = FIR(.) before the output rounding and FIR(C_ACC 2^-24 sqrt(K) |.| + e_act)."""
    x = x.double()
    kacc = C_ACC * U32 * math.sqrt(4 if up else 16)
    u, e = x, torch.zeros_like(x)
    if coef is not None:
        a, b = coef[:, None, None, :, 0].double(), coef[:, None, None, :, 1].double()
        u = x * a + b
        e = U32 * ((x * a).abs() + b.abs())
    if mut == "act_after":
        av = _silu(_fir2(u, up))
        return _fir2(x, up), _fir2(kacc * x.abs(), up), av, None
    av = u
    if act:
        av = _silu(u)
        e = 1.1 * e + _silu_err(u)
    return _fir2(x, up, mut), _fir2(kacc * x.abs(), up), _fir2(av, up, mut), _fir2(kacc * av.abs() + e, up)


def attention_reference(qq, kk, vv, mut=None):
    """softmax(q k^T C^-0.5) v (layerspp.py:84-88) on stored [B,N,C] operands: (out before the store rounding, bound without the
    output rounding)."""
    qq, kk, vv = qq.double(), kk.double(), vv.double()
    B, N, Cc = qq.shape
    scale = float(Cc + 1 if mut == "scale" else Cc) ** -0.5
    s = torch.einsum("bic,bjc->bij", qq, kk) * scale
    if mut == "last_key":
        s = s[:, :, :-1]; vv = vv[:, :-1]; kk = kk[:, :-1]
    p = torch.softmax(s, 1 if mut == "axis" else 2)
    out = torch.einsum("bij,bjc->bic", p, vv)
    ds = (C_ACC * math.sqrt(Cc) + 2 * ULP_FN) * U32 * scale * torch.einsum("bic,bjc->bij", qq.abs(), kk.abs()) + \
        U32 * (s - s.max(2, keepdim=True).values).abs()
    ds_row = ds.max(2).values[:, :, None]
    spv = torch.einsum("bij,bjc->bic", p, vv.abs())
    return out, (torch.expm1(2 * ds_row) + (C_ACC * math.sqrt(N) + 2 * ULP_FN + 4) * U32) * spv


def gn_coef_from_totals(st, gamma, beta, groups, n_tok, eps=GN_EPS):
    """(a, b) per (item, channel) from the fixed-point totals [B,C,2] (int64) as gn_coef_of derives them, in float64."""
    B, Cc, _ = st.shape
    cpg = Cc // groups
    inv_n = float(np.float32(1.0) / (np.float32(cpg) * np.float32(n_tok)))
    S = st[..., 0].reshape(B, groups, cpg).sum(-1).double()
    Q = st[..., 1].reshape(B, groups, cpg).sum(-1).double()
    mean = S / 2 ** 20 * inv_n
    var = (Q / 2 ** 20 * inv_n - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var.float().double() + float(np.float32(eps)))
    a = gamma.double()[None] * rstd.repeat_interleave(cpg, 1)
    return torch.stack([a, beta.double()[None] - mean.repeat_interleave(cpg, 1) * a], -1)


def _flip(y, e_pre, dt):
    """Allowance for one rounded intermediate: the kernel rounds y + d, |d| <= e_pre, the reference rounds y.  Both give the same storage
    value unless y lies within e_pre of a rounding boundary (a midpoint between two storage values); there they differ by at most
    e_pre + one spacing.  float64 -> (|difference| allowed per element)."""
    if dt is None:
        return torch.zeros_like(y)
    _, e = torch.frexp(y.abs())                               # |y| = m 2^e, m in [0.5, 1)
    ulp = torch.exp2((e - (8 if dt == 1 else 11)).double())
    if dt == 2:
        ulp = ulp.clamp_min(2.0 ** -24)                       # fp16 subnormals
    t = y.abs() / ulp
    dist = ((t - torch.floor(t)) - 0.5).abs() * ulp
    return torch.where(dist <= e_pre, e_pre + ulp, torch.zeros_like(y))


def _rss(d, w):
    """Independent differences d through a contraction with w: the root of the sum of squares."""
    return torch.sqrt((d * d) @ (w * w))


def attn_block_reference(x, coef, W, bias, dt, mut=None):
    """AttnBlockpp (layerspp.py:77-93) with use_attn.hip's rounding points.  x [B,N,C] stored values, coef [B,C,2] the folded GroupNorm,
    W = (Wq, Wk, Wv, Wo) as [Cout][Cin] (rounded to the storage type here), bias = four [C]; dt None: no rounding anywhere.
    Returns (out before the store rounding, bound(out) without the output rounding, H)."""
    x = x.double()
    B, N, Cc = x.shape
    Wq, Wk, Wv, Wo = (q(w.double(), dt) for w in W)
    bq, bk, bv, bo = (b.double() for b in bias)
    ca, cb = coef[:, None, :, 0], coef[:, None, :, 1]
    hp = x * ca + cb
    h = q(hp, dt)
    dh = _flip(hp, 8 * U32 * ((x * ca).abs() + cb.abs()), dt)
    if mut == "pad_tokens":                                   # the zero rows of the last 32-token tile left in the softmax
        pad = torch.zeros(B, (N + 31) // 32 * 32 - N, Cc, dtype=h.dtype)
        h, dh = torch.cat([h, pad], 1), torch.cat([dh, pad], 1)
    kacc = C_ACC * U32 * math.sqrt(Cc)

    def nin(w, b):
        y = h @ w.T + b
        return q(y, dt), _flip(y, _rss(dh, w.T) + kacc * (h.abs() @ w.abs().T + b.abs()), dt)
    (qq, dq), (kk, dk), (vv, dv) = nin(Wq, bq), nin(Wk, bk), nin(Wv, bv)
    scale = float(Cc) ** -0.5
    s = torch.einsum("bic,bjc->bij", qq, kk) * scale
    ds = scale * torch.sqrt(torch.einsum("bic,bjc->bij", dq * dq, kk * kk) + torch.einsum("bic,bjc->bij", qq * qq, dk * dk)) + \
        (kacc + 2 * ULP_FN * U32) * scale * torch.einsum("bic,bjc->bij", qq.abs(), kk.abs()) + U32 * (s - s.max(2, keepdim=True).values).abs()
    p = torch.softmax(s, 2)
    P = q(p, dt)
    dP = _flip(p, (torch.expm1(2 * ds.max(2).values[:, :, None]) + (2 * ULP_FN + 4) * U32) * p, dt)
    o = torch.einsum("bij,bjc->bic", P, vv)
    O = q(o, dt)
    dO = _flip(o, torch.einsum("bij,bjc->bic", dP, vv.abs()) + torch.sqrt(torch.einsum("bij,bjc->bic", P * P, dv * dv)) +
               C_ACC * U32 * math.sqrt(N) * torch.einsum("bij,bjc->bic", P, vv.abs()), dt)
    H = (O @ Wo.T + bo)[:, :N]
    dH = (_rss(dO, Wo.T) + kacc * (O.abs() @ Wo.abs().T + bo.abs()))[:, :N]
    return (x + H) * SQRT1_2, (dH + 2 * U32 * (x.abs() + H.abs())) * SQRT1_2, H


def softmax_rows_reference(x, dt, mut=None):
    x = x.double()
    cols = x.shape[-1]
    xs = x[..., :-1] if mut == "last_col" else x
    p = torch.softmax(xs, -1)
    if mut == "last_col":
        p = torch.cat([p, torch.zeros_like(x[..., :1])], -1)
    d = (ULP_FN + (x - x.max(-1, keepdim=True).values).abs()) * U32
    rel = d + (p * d).sum(-1, keepdim=True) + (cols / 256 + 10 + 4) * U32
    return p, rel * p + (2.0 ** -25 if dt == 2 else 0.0)


def combine_reference(h, pyr, w8, b8, mut=None):
    """Combine 'sum' (layerspp.py:50-55): h + Conv1x1(pyr); h [B,P,C] stored, pyr [B,P,8], w8 [C,8], b8 [C]."""
    h, pyr, w8, b8 = h.double(), pyr.double(), w8.double(), b8.double()
    y = h + pyr @ w8.T + (0.0 if mut == "bias" else b8)
    return y, C_ACC * U32 * math.sqrt(10) * (h.abs() + pyr.abs() @ w8.abs().T + b8.abs())


def temb_reference(t, gfp_w, w1, b1, w2, b2, mut=None):
    """silu(Linear_2(silu(Linear_1([sin, cos](log(t) W 2 pi))))) (layerspp.py:37-39, ncsnpp.py:351-352, 364-368, layerspp.py:303).
    Returns (silu(temb), bound, temb)."""
    t, gfp_w, w1, b1, w2, b2 = (v.double() for v in (t, gfp_w, w1, b1, w2, b2))
    nf = gfp_w.numel()
    xp = (t if mut == "log" else torch.log(t))[:, None] * gfp_w[None] * 2 * math.pi
    feat = torch.cat([torch.sin(xp), torch.cos(xp)], -1)
    dfeat = ((ULP_FN + 2.5) * xp.abs() + ULP_FN).repeat(1, 2) * U32
    a1 = feat @ w1.T + b1
    da1 = dfeat @ w1.abs().T + C_ACC * U32 * math.sqrt(2 * nf) * (feat.abs() @ w1.abs().T + b1.abs())
    hid = _silu(a1)
    dhid = 1.1 * da1 + _silu_err(a1)
    a2 = hid @ w2.T + b2
    da2 = dhid @ w2.abs().T + C_ACC * U32 * math.sqrt(4 * nf) * (hid.abs() @ w2.abs().T + b2.abs())
    return _silu(a2), 1.1 * da2 + _silu_err(a2) + U32 * _silu(a2).abs(), a2


def dense_reference(x, W, bias):
    x, W, bias = x.double(), W.double(), bias.double()
    y = x @ W.T + bias
    return y, U32 * y.abs() + C_ACC * U32 * math.sqrt(W.shape[1]) * (x.abs() @ W.abs().T + bias.abs())


def score_out_reference(pyr, t, w, bias, sign, mut=None):
    """output_layer(h / t) as complex (ncsnpp.py:492-500), times sign (model_wrapper.py:137).  pyr [B,P,PC], t [B] or None, w [2,PC]."""
    pyr, w, bias = pyr.double(), w.double(), bias.double()
    hk = pyr if (t is None or mut == "no_div") else pyr / t.double()[:, None, None]
    y = sign * (hk @ w.T + bias)
    s = hk.abs() @ w.abs().T + bias.abs()
    return y, U32 * y.abs() + (ULP_DIV + C_ACC * math.sqrt(pyr.shape[-1])) * U32 * s


def pack_reference(x, y, y2):
    """2 (x.re, x.im, y.re, y.im[, y2.re, y2.im, 1/2, 1/2]) - 1 in fp32 (ncsnpp.py:333-347, 372-374); y None: zeros."""
    parts = [x, y if y is not None else torch.full_like(x, 0.5)]
    if y2 is not None:
        parts += [y2, torch.full_like(x, 0.5)]
    return torch.cat(parts, -1).float() * 2.0 - 1.0


# ---------------------------------------------------------------------------------------------------------------------------
# case data (shared by the CPU mutation controls and the GPU tests)
# ---------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _fir_id(c):
    return (f"{c['kern']}-{DT_NAME[c['dt']]}-{'up' if c['up'] else 'down'}-B{c['B']}x{c['H']}x{c['W']}-C{c['C']}-{c['flags']}"
            + (f"-coef{c['pre']}" if c["coef"] else "") + (f"-strip{c['strip']}" if c.get("strip") is not None else ""))


FIR_CASES = []


def _fir(kern, dt, up, B, H, W, Cc, flags="both", coef=True, act=1, pre="1", strip=None, big=False, creal=None):
    FIR_CASES.append(dict(kern=kern, dt=dt, up=up, B=B, H=H, W=W, C=Cc, flags=flags, coef=coef, act=act, pre=pre, strip=strip, big=big, creal=creal))


for _dt in (0, 1, 2):
    _ch = 4 if _dt == 0 else 8
    _dn = "fir_down_blk_false" if _dt == 0 else "fir_down_blk_true"
    # flags (up and down): raw only / activated only / both; coef null; act 0; the hot configuration
    for _up in (1, 0):
        _k = "fir_up_blk" if _up else "fir_down_blk_false"
        _fir(_k, _dt, _up, 2, 6, 10, 32, flags="raw", coef=False, act=0)
        _fir(_k, _dt, _up, 1, 10, 6, _ch, flags="act")
        _fir(_k, _dt, _up, 3, 6, 6, 32, flags="both", coef=False, act=1)
        _fir(_k, _dt, _up, 2, 10, 14, 128, flags="both", coef=True, act=0)
        _fir(_k, _dt, _up, 1, 2, 14, 32, flags="act", coef=False, act=0)                  # H of 2; act 0 without coef: out_act = FIR(x)
    # the hot configuration; geometry: W of 2, OH / OW odd, B 3; channels one chunk .. 384; pre-activations around +-20 and around 0
    _fir("fir_up_blk", _dt, 1, 3, 7, 5, 384, pre="20")
    _fir("fir_up_blk", _dt, 1, 1, 2, 2, _ch, pre="0")
    _fir("fir_up_blk", _dt, 1, 2, 16, 12, 32, creal=20)
    _fir(_dn, _dt, 0, 3, 14, 10, 384, pre="20", strip=0)                                 # OH 7, OW 5
    _fir(_dn, _dt, 0, 1, 6, 2, _ch, pre="0", strip=0)                                    # one output column
    _fir(_dn, _dt, 0, 2, 16, 12, 32, creal=20, strip=0)
    _fir(_dn, _dt, 0, 2, 20, 18, 128, strip=1)                                           # OH 10: OH % 8 != 0 falls back to the block form
    if _dt:
        _fir("fir_down_strip_8", _dt, 0, 2, 32, 22, 32, strip=8)                         # OW 11: the 2-column strip half outside the map
        _fir("fir_down_strip_4", _dt, 0, 3, 16, 10, 128, pre="20", strip=4)
        _fir("fir_down_strip_4", _dt, 0, 1, 16, 2, 8, pre="0", strip=4)
        _fir("fir_down_strip_4", _dt, 0, 2, 16, 20, 384, strip=1)                        # the heuristic's choice on a small grid: 4 rows
        _fir("fir_down_strip_8", _dt, 0, 1, 16, 12, 32, strip=8, creal=24)
    else:
        _fir("fir_down_blk_false", _dt, 0, 2, 16, 12, 32, strip=8)                       # fp32 never strips
# the grid-stride loop's second iteration (block caps 256 * 32 up, 256 * 16 down), the smallest shapes that reach it, compared item by item
_fir("fir_up_blk", 1, 1, 2, 256, 320, 128, big=True)
_fir("fir_down_blk_true", 2, 0, 4, 512, 640, 128, strip=0, big=True)
_fir("fir_down_strip_4", 1, 0, 7, 512, 640, 128, strip=4, big=True)


def _fir_coef(c, g):
    """Affine (a, b) per (item, channel): pre '1' ordinary, '20' pre-activations around +-20, '0' around zero."""
    B, Cc = c["B"], c["C"]
    a = (0.5 + torch.rand(B, Cc, generator=g, dtype=torch.float64)) * (1 + 0.2 * torch.arange(B, dtype=torch.float64)[:, None])
    b = torch.randn(B, Cc, generator=g, dtype=torch.float64) * 0.3
    if c["pre"] == "20":
        a, b = a * 0.5, torch.where(torch.rand(B, Cc, generator=g) < 0.5, -20.0, 20.0).double() + b
    elif c["pre"] == "0":
        a, b = a * 0.1, b * 0.1
    return torch.stack([a, b], -1).float()


def _fir_input(c, g, B=None):
    B = c["B"] if B is None else B
    x = torch.rand(B, c["H"], c["W"], c["C"], generator=g, dtype=torch.float32) * 2 - 1
    x[:, 0] *= 4; x[:, -1] *= 4; x[:, :, 0] *= 4; x[:, :, -1] *= 4           # a wrong border shows in the elementwise bound
    x += 0.25 * torch.arange(B, dtype=torch.float32)[:, None, None, None]
    if c["creal"]:
        x[..., c["creal"]:] = 0
    return x.to(TD[c["dt"]])


def _ratio(got, ref, part, dt):
    bound = C_OUT * UNIT[dt] * ref.abs() + part + (2.0 ** -25 if dt == 2 else 0.0) * (ref != 0)
    err = (got.double() - ref).abs()
    r = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


def _fused_totals_ratio(stats, got, dt):
    """Output totals of the fused attention block (int64 [B,C,2]) against the float64 sums of the stored out [B,N,C] (module docstring)."""
    v = got.double()
    got_s, got_q = stats[..., 0].double() / 2 ** 20, stats[..., 1].double() / 2 ** 20
    tol_s = (48 * U32 + UNIT[dt]) * v.abs().sum(1) + 2.0 ** -20
    tol_q = (48 * U32 + 2.01 * UNIT[dt]) * (v * v).sum(1) + 2.0 ** -20
    return max(float(((got_s - v.sum(1)).abs() / tol_s).max()), float(((got_q - (v * v).sum(1)).abs() / tol_q).max()))


def _combine_totals_ratio(stats, got, pix):
    """Totals of combine_add (int64 [B,C,2]) against the float64 sums of the stored map [B,pix,C] (module docstring)."""
    v = got.double()
    st = stats.double() / 2 ** 20
    nblk = (pix + 63) // 64
    tol_s = 64 * U32 * v.abs().sum(1) + nblk * 2.0 ** -21
    tol_q = 64 * U32 * (v * v).sum(1) + nblk * 2.0 ** -21
    return max(float(((st[..., 0] - v.sum(1)).abs() / tol_s).max()), float(((st[..., 1] - (v * v).sum(1)).abs() / tol_q).max()))


ATTN_NS = (1, 2, 40, 80, 96, 255, 256, 257, 600)
ATTN_CS = (32, 64, 256, 384)
ATTN_KINDS = ("ordinary", "peaked", "flat")
ATTN_CASES = [dict(dt=dt, N=N, C=ATTN_CS[(i + dt) % 4], B=(1, 3)[(i + dt) % 2], kind=ATTN_KINDS[(i + 2 * dt) % 3])
              for dt in (0, 1, 2) for i, N in enumerate(ATTN_NS)]
# both strided loops wrapping at once (N > 256 and C > 256), each type and kind
ATTN_CASES += [dict(dt=dt, N=N, C=384, B=B, kind=kind) for dt, N, B, kind in ((0, 600, 1, "peaked"), (1, 257, 3, "ordinary"), (2, 600, 3, "peaked"),
                                                                            (1, 600, 1, "flat"), (2, 257, 1, "ordinary"), (0, 257, 3, "flat"))]


def _attn_id(c):
    return f"attention_kernel-{DT_NAME[c['dt']]}-B{c['B']}-N{c['N']}-C{c['C']}-{c['kind']}"


def _attn_data(c):
    g = _gen(1000 + c["N"] * 7 + c["C"] + c["dt"])
    B, N, Cc, dt = c["B"], c["N"], c["C"], c["dt"]
    sd = {"ordinary": 1.4, "peaked": 3.2, "flat": 1.4}[c["kind"]]      # scores ~ N(0, sd^4): spread ~ +-6 / +-30
    r = lambda s: torch.randn(B, N, Cc, generator=g, dtype=torch.float64) * s
    qq, kk, vv = r(sd), r(sd), r(1.0) + 0.25 * torch.arange(B, dtype=torch.float64)[:, None, None]
    if c["kind"] == "flat":
        kk = kk[:, :1].expand(B, N, Cc).contiguous()
    return q(qq, dt), q(kk, dt), q(vv, dt)


FUSED_CASES = [dict(dt=dt, N=N, B=(1, 3)[(i + dt) % 2], stats=(i + dt) % 3 != 0, mean=0.0)
               for dt in (1, 2) for i, N in enumerate((1, 8, 31, 32, 33, 64, 80, 95, 96))]
FUSED_CASES += [dict(dt=1, N=80, B=2, stats=True, mean=20.0), dict(dt=2, N=80, B=2, stats=True, mean=20.0)]


def _fused_id(c):
    return f"attn_fused_kernel-{DT_NAME[c['dt']]}-B{c['B']}-N{c['N']}" + ("-stats" if c["stats"] else "") + ("-large_mean" if c["mean"] else "")


def _fused_data(c):
    """x as stored, its fixed-point totals, GroupNorm affine, NIN matrices [Cout][Cin] (storage type) and biases.  NIN_3 is scaled so
    that |H| ~ 3 |x| (module docstring)."""
    g = _gen(5000 + c["N"] * 3 + c["dt"])
    B, N, Cc, dt = c["B"], c["N"], 256, c["dt"]
    x = q(torch.randn(B, N, Cc, generator=g, dtype=torch.float64) * (0.4 if c["mean"] else 1.0) + c["mean"]
          + 0.25 * torch.arange(B, dtype=torch.float64)[:, None, None], dt)
    st = torch.stack([torch.round(x.sum(1) * 2 ** 20), torch.round((x * x).sum(1) * 2 ** 20)], -1).to(torch.int64)
    gamma = (0.5 + torch.rand(Cc, generator=g)).float(); beta = (torch.randn(Cc, generator=g) * 0.3).float()
    W = [q(torch.randn(Cc, Cc, generator=g, dtype=torch.float64) * s / math.sqrt(Cc), dt) for s in (1.5, 1.5, 1.0, 4.0 * max(1.0, c["mean"]))]
    bias = [(torch.randn(Cc, generator=g) * 0.6).float() for _ in range(4)]
    return x, st, gamma, beta, W, bias


SOFTMAX_COLS = (1, 255, 256, 257, 1024, 5120)
COMBINE_CS = (128, 256, 384, 512)
COMBINE_PIX = (1, 63, 64, 65, 5000)
TEMB_TS = (1.0, 0.5, 0.03, 1e-4)


def _softmax_data(cols, dt):
    g = _gen(300 + cols + dt)
    return q(torch.randn(5, cols, generator=g, dtype=torch.float64) * 4.0 + torch.arange(5, dtype=torch.float64)[:, None], dt)


def _combine_data(Cc, pix, dt):
    g = _gen(700 + Cc + pix + dt)
    B = 2
    h = q(torch.randn(B, pix, Cc, generator=g, dtype=torch.float64) + 0.25 * torch.arange(B, dtype=torch.float64)[:, None, None], dt)
    pyr = torch.randn(B, pix, 8, generator=g).float()
    w8 = (torch.randn(Cc, 8, generator=g) * 0.4).float(); b8 = (torch.randn(Cc, generator=g) * 0.5 + 0.25).float()
    return h, pyr, w8, b8


def _temb_data(nf, scale=16.0):
    """GaussianFourierProjection(scale = 16) (ncsnpp.py:351) and the two Linear layers, fp32."""
    g = _gen(900 + nf)
    r = lambda *s: torch.randn(*s, generator=g).float()
    return r(nf) * scale, r(4 * nf, 2 * nf) / math.sqrt(2 * nf), r(4 * nf) * 0.2, r(4 * nf, 4 * nf) / math.sqrt(4 * nf), r(4 * nf) * 0.2


def _score_data(pc, pix, B, seed):
    g = _gen(seed)
    pyr = torch.randn(B, pix, pc, generator=g).float() + 0.25 * torch.arange(B)[:, None, None]
    return pyr, (torch.randn(2, pc, generator=g) * 0.5).float(), (torch.randn(2, generator=g) * 0.3).float()


# ---------------------------------------------------------------------------------------------------------------------------
# CPU part: the references against what already pins the project
# ---------------------------------------------------------------------------------------------------------------------------
REF_TOL = 2e-6          # fp32-level agreement, the tolerance tests/test_hip_conv_kernels.py uses for the same purpose


def _relmax(got, want):
    return float((got.double() - want.double()).abs().max() / want.double().abs().max())


def test_reference_fir_matches_the_golden_and_the_oracle(golden_dir):
    from oracle import ncsnpp_oracle as no
    g = np.load(os.path.join(golden_dir, "fir.npz"))
    x = torch.from_numpy(g["x"]).double()
    for up, key in ((1, "up"), (0, "down")):
        got = _fir2(x.permute(0, 2, 3, 1), up).permute(0, 3, 1, 2)
        assert _relmax(got, torch.from_numpy(g[key])) < REF_TOL, key
    z = torch.randn(2, 3, 7, 6, generator=_gen(1), dtype=torch.float64)       # odd height: the last row is dropped by downsample_2d
    assert _relmax(_fir2(z.permute(0, 2, 3, 1), 1).permute(0, 3, 1, 2), no.fir_upsample2(z)) < 1e-12
    assert _relmax(_fir2(z[:, :, :6].permute(0, 2, 3, 1), 0).permute(0, 3, 1, 2), no.fir_downsample2(z[:, :, :6])) < 1e-12
    # the activated branch: FIR(silu(a x + b)) as the res-block composes it (layerspp.py:291-298)
    coef = torch.randn(2, 3, 2, generator=_gen(2), dtype=torch.float64)
    zl = z[:, :, :6].permute(0, 2, 3, 1)
    _, _, av, _ = fir_reference(zl, coef, 1, 0)
    want = no.fir_downsample2(F.silu(z[:, :, :6] * coef[:, :, None, None, 0] + coef[:, :, None, None, 1]))
    assert _relmax(av.permute(0, 3, 1, 2), want) < 1e-12


def _attn_golden_through_references(g, sd=None):
    x = torch.from_numpy(g["x"]).double()
    B, Cc, H, W = x.shape
    xl = x.permute(0, 2, 3, 1)
    gamma, beta = torch.from_numpy(g["w.GroupNorm_0.weight"]), torch.from_numpy(g["w.GroupNorm_0.bias"])
    coef = gn_coef_reference(xl, gamma, beta, min(Cc // 4, 32))
    W4 = [torch.from_numpy(g[f"w.NIN_{i}.W"]).double().T.contiguous() for i in range(4)]       # NIN.W is [Cin][Cout] (layers.py:639-650)
    b4 = [torch.from_numpy(g[f"w.NIN_{i}.b"]) for i in range(4)]
    out, _, _ = attn_block_reference(xl.reshape(B, H * W, Cc), coef, W4, b4, None)
    # the same block with the core reference in the middle (what use_op_attention computes)
    h = xl.reshape(B, H * W, Cc) * coef[:, None, :, 0] + coef[:, None, :, 1]
    core, _ = attention_reference(*(h @ W4[i].T + b4[i].double() for i in range(3)))
    out2 = (xl.reshape(B, H * W, Cc) + core @ W4[3].T + b4[3].double()) * SQRT1_2
    return out.reshape(B, H, W, Cc).permute(0, 3, 1, 2), out2.reshape(B, H, W, Cc).permute(0, 3, 1, 2)


def test_reference_attention_matches_the_golden_and_the_oracle(golden_dir):
    from oracle import ncsnpp_oracle as no
    g = np.load(os.path.join(golden_dir, "attn.npz"))
    out, out2 = _attn_golden_through_references(g)
    want = torch.from_numpy(g["y"])
    assert _relmax(out, want) < REF_TOL and _relmax(out2, want) < REF_TOL
    sd = {"a." + k[2:]: torch.from_numpy(g[k]).double() for k in g.files if k.startswith("w.")}
    assert _relmax(out, no.attn_block(torch.from_numpy(g["x"]).double(), sd, "a")) < 1e-10
    # the coefficients from fixed-point totals == float64 GroupNorm of the same values (2^-20 fixed point)
    x, st, gamma, beta, _, _ = _fused_data(FUSED_CASES[4])
    a = gn_coef_from_totals(st, gamma, beta, 32, x.shape[1])
    b = gn_coef_reference(x[:, :, None, :], gamma, beta, 32)
    assert float((a - b).abs().max() / b.abs().max()) < 1e-6


def test_reference_small_kernels_match_the_oracle():
    from oracle import ncsnpp_oracle as no
    # time embedding (a Fourier scale of 1 keeps the fp32 oracle's own argument error at the fp32 level)
    nf = 96
    gfp, w1, b1, w2, b2 = _temb_data(nf, scale=1.0)
    t = torch.tensor([1.0, 0.5, 0.03], dtype=torch.float32)
    sd = {"all_modules.0.W": gfp, "all_modules.1.weight": w1, "all_modules.1.bias": b1, "all_modules.2.weight": w2, "all_modules.2.bias": b2}
    out, _, temb = temb_reference(t, gfp, w1, b1, w2, b2)
    want = no.time_embedding(t, sd)
    assert _relmax(temb, want) < REF_TOL and _relmax(out, F.silu(want)) < REF_TOL
    # Combine 'sum' and the output layer as ncsnpp_forward computes them (oracle/ncsnpp_oracle.py, the lines citing layerspp.py:50-55
    # and ncsnpp.py:492-500), on a small input
    h, pyr, w8, b8 = _combine_data(128, 12, 0)
    hm, pm = h.float().reshape(2, 3, 4, 128).permute(0, 3, 1, 2), pyr.reshape(2, 3, 4, 8).permute(0, 3, 1, 2)
    want = F.conv2d(pm, w8[:, :, None, None], b8) + hm
    got, _ = combine_reference(h, pyr, w8, b8)
    assert _relmax(got.reshape(2, 3, 4, 128).permute(0, 3, 1, 2), want) < REF_TOL
    pyr4, w, bias = _score_data(4, 12, 2, 5)
    t = torch.tensor([0.5, 0.03])
    hh = pyr4.reshape(2, 3, 4, 4).permute(0, 3, 1, 2) / t[:, None, None, None]
    hh = F.conv2d(hh, w[:, :, None, None], bias)
    got, _ = score_out_reference(pyr4, t, w, bias, 1.0)
    assert _relmax(got.reshape(2, 3, 4, 2).permute(0, 3, 1, 2), hh) < REF_TOL
    x, y = (torch.randn(1, 6, 2, generator=_gen(k)) for k in (1, 2))
    want = 2 * torch.cat([x, y], -1) - 1.0                                     # ncsnpp.py:333-347, 372-374
    assert torch.equal(pack_reference(x, y, None), want)


def _caught(ref, part, mutant, dt):
    """A mutant is caught when it exceeds the bound the GPU test applies to the kernel."""
    return _ratio(mutant, ref, part, dt) > 1.0


@pytest.mark.parametrize("c", [c for c in FIR_CASES if not c["big"]], ids=[_fir_id(c) for c in FIR_CASES if not c["big"]])
def test_mutation_controls_fir(c):
    g = _gen(FIR_CASES.index(c))
    coef = _fir_coef(c, g) if c["coef"] else None
    x = _fir_input(c, g)
    raw, praw, av, pact = fir_reference(x, coef, c["act"], c["up"])
    muts = ["replicate", "drop"] + (["swap"] if c["up"] else []) + (["act_after"] if c["act"] and c["flags"] != "raw" else [])
    for m in muts:
        mraw, _, mav, _ = fir_reference(x, coef, c["act"], c["up"], mut=m)
        if c["flags"] != "act" and m != "act_after":
            assert _caught(raw, praw, mraw, c["dt"]), (m, "raw")
        if c["flags"] != "raw":
            assert _caught(av, pact, mav, c["dt"]), (m, "act")


@pytest.mark.parametrize("c", [c for c in ATTN_CASES if c["N"] > 1], ids=[_attn_id(c) for c in ATTN_CASES if c["N"] > 1])
def test_mutation_controls_attention(c):
    qq, kk, vv = _attn_data(c)
    ref, part = attention_reference(qq, kk, vv)
    for m in ("scale", "last_key", "axis"):
        if m == "scale" and c["kind"] == "flat":
            continue
        mut, _ = attention_reference(qq, kk, vv, mut=m)
        assert _caught(ref, part, mut, c["dt"]), m


_FUSED_MUT = [c for c in FUSED_CASES if c["N"] % 32 and not (c["dt"] == 1 and c["N"] == 95)]


@pytest.mark.parametrize("c", _FUSED_MUT, ids=[_fused_id(c) for c in _FUSED_MUT])
def test_mutation_controls_fused_block(c):
    x, st, gamma, beta, W, bias = _fused_data(c)
    coef = gn_coef_from_totals(st, gamma, beta, 32, c["N"])
    ref, part, H = attn_block_reference(x, coef, W, bias, c["dt"])
    mut, _, mH = attn_block_reference(x, coef, W, bias, c["dt"], mut="pad_tokens")
    assert _caught(ref, part, mut, c["dt"])
    assert float(H.abs().mean()) > float(x.abs().mean()) * (1.0 if not c["mean"] else 0.2)       # the attention is not hidden behind x


def test_mutation_controls_small_kernels():
    for dt in (0, 1, 2):
        for cols in SOFTMAX_COLS[1:]:
            x = _softmax_data(cols, dt)
            ref, bound = softmax_rows_reference(x, dt)
            mut, _ = softmax_rows_reference(x, dt, mut="last_col")
            assert float(((mut - ref).abs() / (UNIT[dt] * ref + bound)).max()) > 1, ("softmax", cols)
        for Cc in COMBINE_CS:
            for pix in COMBINE_PIX[:4]:
                h, pyr, w8, b8 = _combine_data(Cc, pix, dt)
                ref, part = combine_reference(h, pyr, w8, b8)
                assert _caught(ref, part, combine_reference(h, pyr, w8, b8, mut="bias")[0], dt), ("combine", Cc, pix)
    for pc in (4, 8):
        pyr, w, bias = _score_data(pc, 300, 2, 40 + pc)
        t = torch.tensor([0.5, 0.03])
        ref, bound = score_out_reference(pyr, t, w, bias, -1.0)
        mut, _ = score_out_reference(pyr, t, w, bias, -1.0, mut="no_div")
        assert float(((mut - ref).abs() / bound).max()) > 1
    for nf in (96, 128):
        p = _temb_data(nf)
        t = torch.tensor(TEMB_TS[1:], dtype=torch.float32)
        ref, bound, _ = temb_reference(t, *p)
        mut, _, _ = temb_reference(t, *p, mut="log")
        assert float(((mut - ref).abs() / bound).max()) > 1


# ---------------------------------------------------------------------------------------------------------------------------
# GPU part
# ---------------------------------------------------------------------------------------------------------------------------
def _lib():
    from universal_speech_enhancement_amd import _lib as L
    return L


def _set_option(name, value):
    from universal_speech_enhancement_amd.hip_engine import set_option
    set_option(name, value)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _guarded(shape, dtype, fill=SENTINEL):
    n = int(np.prod(shape))
    buf = torch.full((n + TAIL,), fill, dtype=dtype, device="cuda")
    return buf, buf[:n].view(*shape)


def _tail_ok(buf, what, fill=SENTINEL):
    assert bool((buf[-TAIL:] == fill).all()), f"write past the end of {what}"


def _ok(rc, what):
    assert rc == 0, (what, rc, _lib().lib().use_last_error().decode())


def _measured(case, ratio):
    print(f"[measured] {case}: worst |err| / bound {ratio:.3f}")
    assert ratio < 1.0, (case, ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("c", FIR_CASES, ids=[_fir_id(c) for c in FIR_CASES])
def test_fir_kernel_matches_float64_reference(c):
    L = _lib()
    dt, up, B, H, W, Cc = c["dt"], c["up"], c["B"], c["H"], c["W"], c["C"]
    g = _gen(FIR_CASES.index(c))
    coef = _fir_coef(c, g) if c["coef"] else None
    d_coef = coef.cuda() if coef is not None else None
    if c["big"]:                                             # generated on the device, compared item by item (host memory)
        gd = torch.Generator(device="cuda").manual_seed(FIR_CASES.index(c))
        d_x = (torch.rand(B, H, W, Cc, generator=gd, device="cuda") * 2 - 1).to(TD[dt])
        d_x[:, 0] *= 4; d_x[:, -1] *= 4; d_x[:, :, 0] *= 4; d_x[:, :, -1] *= 4
    else:
        x = _fir_input(c, g)
        d_x = x.cuda()
    OH, OW = (2 * H, 2 * W) if up else (H // 2, W // 2)
    abuf = rbuf = oa = orw = None
    if c["flags"] != "raw":
        abuf, oa = _guarded((B, OH, OW, Cc), TD[dt])
    if c["flags"] != "act":
        rbuf, orw = _guarded((B, OH, OW, Cc), TD[dt])
    try:
        if c["strip"] is not None:
            _set_option("fir_strip", c["strip"])
        rc = L.lib().use_op_fir(_p(d_x), dt, _p(d_coef), c["act"], _p(oa), _p(orw), B, H, W, Cc, up, _stream())
        torch.cuda.synchronize()
    finally:
        _set_option("fir_strip", 1)
    _ok(rc, "use_op_fir")
    worst = 0.0
    # the large cases: one item and 32 channels at a time (channels and items do not interact)
    pieces = [(slice(b, b + 1), slice(c0, c0 + 32)) for b in range(B) for c0 in range(0, Cc, 32)] if c["big"] else [(slice(None), slice(None))]
    for sl, cs in pieces:
        xs = d_x[sl, :, :, cs].cpu()
        raw, praw, av, pact = fir_reference(xs, coef[sl, cs] if coef is not None else None, c["act"], up)
        if orw is not None:
            got = orw[sl, :, :, cs].cpu()
            assert bool(torch.isfinite(got.float()).all())
            worst = max(worst, _ratio(got, raw, praw, dt))
            if c["creal"]:
                assert float(got[..., c["creal"]:].float().abs().max()) == 0.0, "zero padding channels in, non-zero out (raw)"
        if oa is not None:
            got = oa[sl, :, :, cs].cpu()
            assert bool(torch.isfinite(got.float()).all())
            worst = max(worst, _ratio(got, av, pact, dt))
    for buf, what in ((abuf, "out_act"), (rbuf, "out_raw")):
        if buf is not None:
            _tail_ok(buf, what)
    _measured(_fir_id(c), worst)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [1, 2])
def test_fir_dispatch_reaches_the_strip_and_block_forms(dt):
    """What the ids of the FIR cases claim: with the hot configuration and OH % 8 == 0 the strip forms (8, 4 and the heuristic's
    choice) and the block form give bit-identical results from different kernels - and the heuristic's result equals the 4-row form's
    on this small grid.  (That the strip options select other kernels is test_fir_down_strip_walk_equals_the_block_form's subject.)"""
    L = _lib()
    c = dict(dt=dt, B=2, H=16, W=20, C=64, pre="1", creal=None)
    g = _gen(77 + dt)
    coef = _fir_coef(c, g).cuda(); x = _fir_input(c, g).cuda()
    outs = {}
    try:
        for strip in (0, 1, 4, 8):
            _set_option("fir_strip", strip)
            oa, orw = torch.empty(2, 8, 10, 64, dtype=TD[dt], device="cuda"), torch.empty(2, 8, 10, 64, dtype=TD[dt], device="cuda")
            _ok(L.lib().use_op_fir(_p(x), dt, _p(coef), 1, _p(oa), _p(orw), 2, 16, 20, 64, 0, _stream()), "use_op_fir")
            torch.cuda.synchronize()
            outs[strip] = (oa.cpu(), orw.cpu())
    finally:
        _set_option("fir_strip", 1)
    for strip in (1, 4, 8):
        assert torch.equal(outs[strip][0], outs[0][0]) and torch.equal(outs[strip][1], outs[0][1]), strip


@pytest.mark.gpu
@pytest.mark.parametrize("c", ATTN_CASES, ids=[_attn_id(c) for c in ATTN_CASES])
def test_attention_kernel_matches_float64_reference(c):
    L = _lib()
    dt, B, N, Cc = c["dt"], c["B"], c["N"], c["C"]
    qq, kk, vv = _attn_data(c)
    d = [t.to(TD[dt]).cuda() for t in (qq, kk, vv)]
    obuf, out = _guarded((B, N, Cc), TD[dt])
    _ok(L.lib().use_op_attention(_p(d[0]), _p(d[1]), _p(d[2]), _p(out), dt, B, N, Cc, _stream()), "use_op_attention")
    torch.cuda.synchronize()
    _tail_ok(obuf, "out")
    ref, part = attention_reference(qq, kk, vv)
    got = out.cpu()
    assert bool(torch.isfinite(got.float()).all())
    _measured(_attn_id(c), _ratio(got, ref, part, dt))


@pytest.mark.gpu
@pytest.mark.parametrize("c", FUSED_CASES, ids=[_fused_id(c) for c in FUSED_CASES])
def test_fused_attention_block_matches_float64_reference(c):
    L = _lib()
    dt, B, N, Cc = c["dt"], c["B"], c["N"], 256
    x, st, gamma, beta, W, bias = _fused_data(c)
    d_x, d_st = x.to(TD[dt]).cuda(), st.cuda()
    d_g, d_b = gamma.cuda(), beta.cuda()
    d_W = [w.to(TD[dt]).cuda().contiguous() for w in W]
    d_bias = [b.cuda() for b in bias]
    obuf, out = _guarded((B, N, Cc), TD[dt])
    sbuf = stats = None
    if c["stats"]:
        sbuf = torch.full((B * Cc * 2 + TAIL,), 0x5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        sbuf[:B * Cc * 2] = 0
        stats = sbuf[:B * Cc * 2].view(B, Cc, 2)
    _ok(L.lib().use_op_attn_block(_p(d_x), _p(d_st), _p(d_g), _p(d_b), 32, GN_EPS, _p(d_W[0]), _p(d_W[1]), _p(d_W[2]), _p(d_W[3]),
                                  _p(d_bias[0]), _p(d_bias[1]), _p(d_bias[2]), _p(d_bias[3]), _p(out), _p(stats), dt, B, N, Cc, _stream()),
        "use_op_attn_block")
    torch.cuda.synchronize()
    _tail_ok(obuf, "out (rows N.. of the last tile must not be stored)")
    coef = gn_coef_from_totals(st, gamma, beta, 32, N)
    ref, part, H = attn_block_reference(x, coef, W, bias, dt)
    got = out.cpu()
    assert bool(torch.isfinite(got.float()).all())
    r_out = _ratio(got, ref, part, dt)
    # h reconstructed from the stored out, against the reference's H: sqrt 2 times the bound of out
    h_rec = got.double() * SQRT2 - x
    bound_h = SQRT2 * (C_OUT * UNIT[dt] * ref.abs() + part + (2.0 ** -25 if dt == 2 else 0.0))
    r_h = float(((h_rec - H).abs() / bound_h).max())
    rel_h = float((h_rec - H).abs().max() / H.abs().max())
    r_st = 0.0
    if stats is not None:
        assert bool((sbuf[-TAIL:] == 0x5A5A5A5A5A5A).all()), "write past the end of stats"
        r_st = _fused_totals_ratio(stats.cpu(), got, dt)
    print(f"[fused] {_fused_id(c)}: out {r_out:.3f} h {r_h:.3f} (|h err| / max |H| {rel_h:.2e}, mean |H| / mean |x| "
          f"{float(H.abs().mean() / x.abs().mean()):.2f}) totals {r_st:.3f}")
    _measured(_fused_id(c), max(r_out, r_h, r_st))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [0, 1, 2])
def test_softmax_rows_and_transpose_nc(dt):
    L = _lib()
    worst = 0.0
    for cols in SOFTMAX_COLS:
        x = _softmax_data(cols, dt)
        buf, d = _guarded(tuple(x.shape), TD[dt])
        d.copy_(x.to(TD[dt]))
        _ok(L.lib().use_op_softmax_rows(_p(d), dt, x.shape[0], cols, _stream()), "use_op_softmax_rows")
        torch.cuda.synchronize()
        _tail_ok(buf, "x")
        ref, bound = softmax_rows_reference(x, dt)
        r = float(((d.cpu().double() - ref).abs() / (UNIT[dt] * ref + bound)).max())
        print(f"[measured] softmax_rows_kernel-{DT_NAME[dt]}-cols{cols}: worst |err| / bound {r:.3f}")
        worst = max(worst, r)
    assert worst < 1.0
    for B, N, Cc in ((1, 1, 1), (2, 33, 31), (3, 70, 45), (1, 64, 96), (2, 5, 257)):
        src = torch.randn(B, N, Cc, generator=_gen(N + Cc)).to(TD[dt]).cuda()
        buf, dst = _guarded((B, Cc, N), TD[dt])
        _ok(L.lib().use_op_transpose_nc(_p(src), _p(dst), dt, B, N, Cc, _stream()), "use_op_transpose_nc")
        torch.cuda.synchronize()
        _tail_ok(buf, "out")
        assert torch.equal(dst, src.transpose(1, 2).contiguous()), (B, N, Cc)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [0, 1, 2])
@pytest.mark.parametrize("Cc", COMBINE_CS)
def test_combine_add_matches_float64_reference(dt, Cc):
    L = _lib()
    worst = worst_st = 0.0
    for pix in COMBINE_PIX:
        h, pyr, w8, b8 = _combine_data(Cc, pix, dt)
        B = h.shape[0]
        buf, d_h = _guarded((B, pix, Cc), TD[dt])
        d_h.copy_(h.to(TD[dt]))
        sbuf = torch.full((B * Cc * 2 + TAIL,), 0x5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        sbuf[:B * Cc * 2] = 0
        d_pyr, d_w, d_b = pyr.cuda(), w8.cuda(), b8.cuda()
        _ok(L.lib().use_op_combine_add(_p(d_h), dt, _p(d_pyr), _p(d_w), _p(d_b), _p(sbuf), B, pix, Cc, _stream()), "use_op_combine_add")
        torch.cuda.synchronize()
        _tail_ok(buf, "h")
        assert bool((sbuf[-TAIL:] == 0x5A5A5A5A5A5A).all()), "write past the end of stats"
        ref, part = combine_reference(h, pyr, w8, b8)
        got = d_h.cpu()
        worst = max(worst, _ratio(got, ref, part, dt))
        worst_st = max(worst_st, _combine_totals_ratio(sbuf[:B * Cc * 2].view(B, Cc, 2).cpu(), got, pix))
    print(f"[measured] combine_add_kernel-{DT_NAME[dt]}-C{Cc} totals: worst |err| / bound {worst_st:.3f}")
    _measured(f"combine_add_kernel-{DT_NAME[dt]}-C{Cc}", max(worst, worst_st))


@pytest.mark.gpu
@pytest.mark.parametrize("nf", [96, 128])
def test_time_embedding_matches_float64_reference(nf):
    L = _lib()
    gfp, w1, b1, w2, b2 = _temb_data(nf)
    d = [v.cuda() for v in (gfp, w1, b1, w2, b2)]
    worst = 0.0
    for stride in (1, 2):
        B = len(TEMB_TS)
        tb = torch.full((B * stride,), 7.0)
        tb[::stride] = torch.tensor(TEMB_TS)
        d_t = tb.cuda()
        buf, out = _guarded((B, 4 * nf), torch.float32)
        _ok(L.lib().use_op_temb_mlp(_p(d_t), stride, *(_p(v) for v in d), _p(out), B, nf, _stream()), "use_op_temb_mlp")
        torch.cuda.synchronize()
        _tail_ok(buf, "out")
        ref, bound, _ = temb_reference(tb[::stride], gfp, w1, b1, w2, b2)
        r = (out.cpu().double() - ref).abs() / bound
        for i, tv in enumerate(TEMB_TS):
            print(f"[measured] temb_mlp_kernel-nf{nf}-t{tv:g}-stride{stride}: worst |err| / bound {float(r[i].max()):.3f}")
        worst = max(worst, float(r.max()))
        st = out.clone()
        for rows in (1, 3, 128, 130):
            g = _gen(rows)
            Wd, bd = (torch.randn(rows, 4 * nf, generator=g) / math.sqrt(4 * nf)).float(), (torch.randn(rows, generator=g) * 0.3).float()
            dbuf, dout = _guarded((B, rows), torch.float32)
            d_W, d_bd = Wd.cuda(), bd.cuda()
            _ok(L.lib().use_op_temb_dense(_p(st), _p(d_W), _p(d_bd), _p(dout), B, rows, 4 * nf, _stream()), "use_op_temb_dense")
            torch.cuda.synchronize()
            _tail_ok(dbuf, "out")
            dref, dbound = dense_reference(st.cpu(), Wd, bd)
            rd = float(((dout.cpu().double() - dref).abs() / dbound).max())
            print(f"[measured] temb_dense_kernel-nf{nf}-rows{rows}: worst |err| / bound {rd:.3f}")
            worst = max(worst, rd)
    assert worst < 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("pc", [4, 8])
def test_score_out_and_pack_input(pc):
    L = _lib()
    worst = 0.0
    for pix, B, with_t, sign, stride in ((1, 2, True, -1.0, 1), (1000, 3, True, 1.0, 2), (1000, 2, False, -1.0, 1), (2048 * 256 + 777, 1, True, -1.0, 1),
                                        (2048 * 256 + 777, 2, False, 1.0, 1), (300, 2, True, -1.0, 1)):
        pyr, w, bias = _score_data(pc, pix, B, pix % 1000 + pc)
        tb = torch.full((B * stride,), 7.0)
        tb[::stride] = torch.tensor([1e-4, 0.03, 1.0][:B]) if pix == 300 or B == 3 else torch.tensor([0.5, 0.03][:B])
        d_t = tb.cuda() if with_t else None
        buf, out = _guarded((B, pix, 2), torch.float32)
        d_pyr, d_w, d_bias = pyr.cuda(), w.cuda(), bias.cuda()
        _ok(L.lib().use_op_score_out(_p(d_pyr), pc, _p(d_t), stride, _p(d_w), _p(d_bias), _p(out), B, pix, sign, _stream()), "use_op_score_out")
        torch.cuda.synchronize()
        _tail_ok(buf, "score")
        ref, bound = score_out_reference(pyr, tb[::stride] if with_t else None, w, bias, sign)
        r = float(((out.cpu().double() - ref).abs() / bound).max())
        print(f"[measured] score_out_kernel<{pc}>-B{B}-pix{pix}-{'t' if with_t else 'null'}-sign{sign:+.0f}: worst |err| / bound {r:.3f}")
        worst = max(worst, r)
    assert worst < 1.0
    if pc == 4:
        for npix in (1, 255, 8192 * 256 + 5):
            x, y, y2 = (torch.randn(npix, 2, generator=_gen(npix + k)).float() for k in range(3))
            for yy, yy2 in ((None, None), (y, None), (y, y2)):
                ch = 8 if yy2 is not None else 4
                buf, out = _guarded((npix, ch), torch.float32)
                d_in = [None if v is None else v.cuda() for v in (x, yy, yy2)]
                _ok(L.lib().use_op_pack_input(_p(d_in[0]), _p(d_in[1]), _p(d_in[2]), _p(out), npix, _stream()), "use_op_pack_input")
                torch.cuda.synchronize()
                _tail_ok(buf, "x4")
                assert torch.equal(out.cpu(), pack_reference(x, yy, yy2)), (npix, ch)


@pytest.mark.gpu
def test_entry_points_refuse_what_their_kernels_cannot_run():
    """Host-side argument checks in front of the launch: USE_E_INVALID with a message, nothing launched (the outputs keep their fill),
    and a valid call right after works."""
    L = _lib()
    lib = L.lib()
    keep = []                                                 # every device tensor of this test stays alive until its end

    def z(*shape, dt=torch.bfloat16, add=0.0):
        keep.append(torch.zeros(*shape, dtype=dt, device="cuda") + add)
        return keep[-1]
    s = _stream()

    def refused(rc, what):
        msg = lib.use_last_error().decode()
        print(f"[refuse] {what}: rc {rc} '{msg}'")
        assert rc == INVALID and msg, (what, rc, msg)

    out = torch.full((1, 4, 4, 32), 3.0, dtype=torch.bfloat16, device="cuda")
    refused(lib.use_op_fir(_p(z(1, 2, 2, 20)), 1, None, 0, None, _p(out), 1, 2, 2, 20, 1, s), "fir 16-bit C = 20")
    refused(lib.use_op_fir(_p(z(1, 2, 2, 6, dt=torch.float32)), 0, None, 0, None, _p(out), 1, 2, 2, 6, 1, s), "fir fp32 C = 6")
    refused(lib.use_op_fir(_p(z(1, 2, 2, 32)), 7, None, 0, None, _p(out), 1, 2, 2, 32, 1, s), "fir dtype 7")
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    _ok(lib.use_op_fir(_p(z(1, 2, 2, 32, add=1.0)), 1, None, 0, None, _p(out), 1, 2, 2, 32, 1, s), "use_op_fir")
    torch.cuda.synchronize()
    of = out.float()                                          # x = 1 with zero borders: 3/4 at an edge, 9/16 in a corner
    assert float(of[0, 0, 0, 0]) == 0.5625 and float(of[0, 0, 1, 0]) == 0.75 and float(of[0, 1, 1, 0]) == 1.0 and float(of[0, 3, 3, 31]) == 0.5625

    N, Cc = 16384, 256                                        # (C + N) * 4 = 66 560 bytes
    big = z(1, N, Cc); o = torch.full((1, N, Cc), 3.0, dtype=torch.bfloat16, device="cuda")
    refused(lib.use_op_attention(_p(big), _p(big), _p(big), _p(o), 1, 1, N, Cc, s), "attention (C + N) * 4 above the LDS of a launch")
    refused(lib.use_op_attention(_p(big), _p(big), _p(big), _p(o), 5, 1, 8, Cc, s), "attention dtype 5")
    torch.cuda.synchronize()
    assert bool((o == 3.0).all())
    _ok(lib.use_op_attention(_p(big), _p(big), _p(z(1, 8, Cc, add=1.0)), _p(o), 1, 1, 8, Cc, s), "use_op_attention")
    torch.cuda.synchronize()
    assert bool((o[0, :8] == 1.0).all()) and bool((o[0, 8:] == 3.0).all())

    c = FUSED_CASES[1]
    x, st, gamma, beta, W, bias = _fused_data(c)
    a = [x.to(torch.bfloat16).cuda(), st.cuda(), gamma.cuda(), beta.cuda()] + [w.to(torch.bfloat16).cuda() for w in W] + [b.cuda() for b in bias]
    o = torch.full((c["B"], 128, 256), 3.0, dtype=torch.bfloat16, device="cuda")
    call = lambda dt, N, Cc, groups=32: lib.use_op_attn_block(_p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), groups, GN_EPS, *(_p(v) for v in a[4:]),
                                                            _p(o), None, dt, c["B"], N, Cc, s)
    refused(call(0, 8, 256), "attn_block fp32 storage")
    refused(call(1, 97, 256), "attn_block N = 97")
    refused(call(1, 0, 256), "attn_block N = 0")
    refused(call(1, 8, 128), "attn_block C = 128")
    refused(call(1, 8, 256, groups=48), "attn_block 48 groups")
    refused(call(9, 8, 256), "attn_block dtype 9")
    torch.cuda.synchronize()
    assert bool((o == 3.0).all())
    _ok(call(1, c["N"], 256), "use_op_attn_block")
    torch.cuda.synchronize()
    assert bool((o[:, :c["N"]] != 3.0).any()) and bool(torch.isfinite(o.float()).all())

    f32 = lambda *sh, add=0.0: z(*sh, dt=torch.float32, add=add)
    st64 = torch.zeros(2, 520, 2, dtype=torch.int64, device="cuda")
    refused(lib.use_op_combine_add(_p(z(2, 4, 520)), 1, _p(f32(2, 4, 8)), _p(f32(520, 8)), _p(f32(520)), _p(st64), 2, 4, 520, s), "combine_add C = 520")
    refused(lib.use_op_combine_add(_p(z(2, 4, 132)), 1, _p(f32(2, 4, 8)), _p(f32(132, 8)), _p(f32(132)), _p(st64), 2, 4, 132, s), "combine_add C % 8")
    refused(lib.use_op_combine_add(_p(z(2, 4, 128)), 1, _p(f32(2, 4, 8)), _p(f32(128, 8)), _p(f32(128)), None, 2, 4, 128, s), "combine_add without totals")
    refused(lib.use_op_combine_add(_p(z(2, 4, 128)), 4, _p(f32(2, 4, 8)), _p(f32(128, 8)), _p(f32(128)), _p(st64), 2, 4, 128, s), "combine_add dtype 4")
    refused(lib.use_op_score_out(_p(f32(1, 4, 5)), 5, None, 1, _p(f32(2, 5)), _p(f32(2)), _p(f32(1, 4, 2)), 1, 4, 1.0, s), "score_out 5 channels")
    refused(lib.use_op_temb_mlp(_p(f32(1)), 1, _p(f32(1)), _p(f32(1)), _p(f32(1)), _p(f32(1)), _p(f32(1)), _p(f32(1)), 1, 4096, s), "temb_mlp nf = 4096")
    refused(lib.use_op_softmax_rows(_p(z(4, 4)), 3, 4, 4, s), "softmax_rows dtype 3")
    refused(lib.use_op_transpose_nc(_p(z(4, 4)), _p(z(4, 4)), 3, 1, 4, 4, s), "transpose_nc dtype 3")
    refused(lib.use_op_pack_input(_p(f32(4, 2)), None, _p(f32(4, 2)), _p(f32(4, 8)), 4, s), "pack_input y2 without y")
    torch.cuda.synchronize()
    assert int(st64.abs().max()) == 0
    h = z(2, 4, 128)
    _ok(lib.use_op_combine_add(_p(h), 1, _p(f32(2, 4, 8)), _p(f32(128, 8)), _p(f32(128, add=1.0)), _p(st64), 2, 4, 128, s), "use_op_combine_add")
    torch.cuda.synchronize()
    assert bool((h == 1.0).all()) and int(st64[0, 0, 0]) == 4 << 20
