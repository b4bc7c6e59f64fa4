"""Every implicit-GEMM convolution kernel (conv_sk, conv_v2, conv_v4, conv_v5 and the generic conv_kernel) and every prologue /
epilogue feature, one launch at a time through use_op_conv, against a plain float64 reference of the same operation.

The reference (`conv_reference`) sees the operands the kernel sees: sources, shortcut inputs, residual and weights rounded to the
storage type; the prologue a x + b and SiLU evaluated in float64 and rounded to the storage type (the kernels stage the activated
halo in 16 bits); then, in float64,
    out = ((conv3x3|1x1(act) + conv1x1(x0|x1) w2 + bias + temb[b]) + res) * out_scale + (pyr . w4 + b4)
(include/use_hip.h, use_op_conv), rounded once to the output type.

The bound is per element, not relative to the tensor's maximum:
    |got - ref| <= C_OUT u_out |ref| + C_IN u_in S + C_ACC 2^-24 sqrt(K) S,      K = Cin * ntaps + XC0 + XC1
    S = conv(|act|, |w|) + conv(|x|, |w2|) + |bias| + |temb| + |res| + |pyr| |w4| + |b4|      (float64, before the out_scale)
u_in / u_out: unit roundoff of the storage / output type (fp32 storage: u_in = 0 - nothing is rounded that the reference does not
round).  C_IN covers the activated operand rounding to a neighbour (the device SiLU uses v_exp / v_rcp), C_ACC the fp32 MFMA
accumulation and the fp32 epilogue.  The sqrt(K): the kernels accumulate up to K products serially in one fp32 accumulator (which
conv_v4 / conv_v5 start from bias + temb); each addition rounds relative to the running sum, so the accumulated error grows like
sqrt(K) u S (the probabilistic rounding-error bound), not u S.  Measured on fp32 storage: up to 11.8 x 2^-24 S at K = 1728 with the
flat form (0.14 of this bound), while one dropped product of K is ~S / K, hundreds of times the bound.  Each case prints its worst
|err| / bound; every ratio must stay below 1.

conv_sk is not one kernel: launch_conv_sk picks the tile, 32 or 64 output channels per workgroup (NJ) and the channels per K pass (CP) from
the operands.  tests/conv_sk_forms.py mirrors that choice on the host; every conv_sk case asserts from it the form it was written to
reach before it launches (FORMS), so a case cannot drift onto another form unnoticed, and tests/test_conv_sk_forms_host.py checks on the
CPU that the cases cover every form and that defects of the decomposition exceed this bound.  The bound does not depend on the form:
eight-way split-K only shortens the chains (measured: at most 0.32 of it in 16 bits, 0.06 in fp32, at K up to 9216).

`-m "not gpu"` checks the reference itself: against the oracle's res-block goldens (tests/golden/resblock_*.npz) composed from it
as the engine composes the res-block, and against a direct loop implementation on a tiny shape."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lowprec as lp

TD = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
DT_NAME = {0: "fp32", 1: "bf16", 2: "fp16"}
UNIT = {0: 2.0 ** -24, 1: 2.0 ** -8, 2: 2.0 ** -11}      # unit roundoff of each storage type
KERNEL = {1: "generic", 2: "conv_v2", 4: "conv_v4", 5: "conv_v5", 7: "conv_sk"}
C_OUT, C_IN, C_ACC = 1.0, 1.0, 2.0
GN_EPS = 1e-6
SQRT1_2 = 0.70710678118654752440
TAIL = 2048                       # sentinel elements behind `out` and `stats`
SENTINEL = 1536.0                 # exact in every storage type


def q(t, dt):
    """float64 -> the storage type -> float64 (round to nearest even); dt None: no rounding."""
    return t.double() if dt is None else t.to(TD[dt]).double()


def _silu(x):
    return x / (1.0 + torch.exp(-x))


def conv_reference(x, coef, act, w, dt, xs=None, w2=None, bias=None, temb=None, res=None, scale=1.0, pyr=None, w4=None, b4=None):
    """float64 reference of use_op_conv.  x [B,H,W,Cin], xs [B,H,W,XC], res [B,H,W,Cout]: the values as stored; coef [B,Cin,2] or None;
    w [Cout,Cin,3,3] or [Cout,Cin] (rounded to the storage type here); w2 [Cout,XC]; bias [Cout]; temb [B,Cout] (the row each item reads);
    pyr [B,H,W,4]; w4 [Cout,4]; b4 [Cout].  Returns (out before the output rounding, S of the bound), both [B,H,W,Cout] float64."""
    x = x.double()
    a = x * coef[:, None, None, :, 0].double() + coef[:, None, None, :, 1].double() if coef is not None else x
    if act:
        a = _silu(a)
    a = q(a, dt).permute(0, 3, 1, 2)
    wq = q(w.double(), dt)
    if wq.dim() == 2:
        wq = wq[:, :, None, None]
    pad = wq.shape[-1] // 2
    y = F.conv2d(a, wq, padding=pad)
    s = F.conv2d(a.abs(), wq.abs(), padding=pad)
    if xs is not None:
        xn = xs.double().permute(0, 3, 1, 2)
        w2q = q(w2.double(), dt)[:, :, None, None]
        y = y + F.conv2d(xn, w2q)
        s = s + F.conv2d(xn.abs(), w2q.abs())
    y, s = y.permute(0, 2, 3, 1), s.permute(0, 2, 3, 1)
    for v in (bias, None if temb is None else temb[:, None, None, :]):
        if v is not None:
            y = y + v.double(); s = s + v.double().abs()
    if res is not None:
        y = y + res.double(); s = s + res.double().abs()
    y = y * scale
    if pyr is not None:
        p = pyr.double() @ w4.double().T
        pa = pyr.double().abs() @ w4.double().abs().T
        if b4 is not None:
            p = p + b4.double(); pa = pa + b4.double().abs()
        y = y + p; s = s + pa
    return y, s


def gn_coef_reference(src, gamma, beta, groups, eps=GN_EPS):
    """GroupNorm(groups) of the stored source values [B,H,W,C] in float64, folded to (a, b) per (item, channel): [B,C,2]."""
    B, H, W, Cc = src.shape
    xg = src.double().permute(0, 3, 1, 2).reshape(B, groups, -1)
    mean, var = xg.mean(-1), xg.var(-1, unbiased=False)
    cpg = Cc // groups
    a = gamma.double()[None] * (1.0 / torch.sqrt(var + eps)).repeat_interleave(cpg, 1)
    b = beta.double()[None] - mean.repeat_interleave(cpg, 1) * a
    return torch.stack([a, b], -1)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU part: the reference itself
# ---------------------------------------------------------------------------------------------------------------------------
def _pad32(c):
    return (c + 31) // 32 * 32


def _reference_resblock(g, up=False, down=False, split=None):
    """ResnetBlockBigGANpp (layerspp.py:282-314) composed from conv_reference as the engine composes it, channels zero-padded to
    multiples of 32 as tests/test_hip_ops.py pads them; fp32 storage."""
    x, temb = torch.from_numpy(g["x"]).double(), torch.from_numpy(g["temb"]).double()
    W = {k[2:]: torch.from_numpy(g[k]).double() for k in g.files if k.startswith("w.")}
    B, Cin, H, Wd = x.shape
    Cout = W["Conv_0.weight"].shape[0]
    cop = _pad32(Cout)
    parts = [Cin] if split is None else [split, Cin - split]
    pads = [_pad32(c) for c in parts]
    offs, po = np.cumsum([0] + parts), np.cumsum([0] + pads)

    def padc(t, axis):                      # real channels -> padded concatenation along `axis`
        shape = list(t.shape); shape[axis] = sum(pads)
        o = torch.zeros(shape, dtype=t.dtype)
        for i in range(len(parts)):
            o.narrow(axis, int(po[i]), parts[i]).copy_(t.narrow(axis, int(offs[i]), parts[i]))
        return o

    def padn(t, n, axis=0):
        shape = list(t.shape); shape[axis] = n
        o = torch.zeros(shape, dtype=t.dtype)
        o.narrow(axis, 0, t.shape[axis]).copy_(t)
        return o

    xs = padc(q(x, 0).permute(0, 2, 3, 1), 3)                                          # [B,H,W,sum(pads)]
    coef0 = padc(gn_coef_reference(x.permute(0, 2, 3, 1), W["GroupNorm_0.weight"], W["GroupNorm_0.bias"], min(Cin // 4, 32)), 1)
    tv = F.linear(F.silu(temb), W["Dense_0.weight"], W["Dense_0.bias"])
    w0 = padn(padc(W["Conv_0.weight"], 1), cop)
    if up or down:
        assert split is None
        a = xs * coef0[:, None, None, :, 0] + coef0[:, None, None, :, 1]
        a = q(_silu(a), 0).permute(0, 3, 1, 2)
        k = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=torch.float64)
        k2 = (k[:, None] * k[None, :]) / 64.0
        kern = (k2 * 4.0 if up else k2)[None, None].repeat(a.shape[1], 1, 1, 1)

        def fir(t):                         # upfirdn2d with [1,3,3,1] (up_or_down_sampling.py:202-264)
            if up:
                z = torch.zeros(t.shape[0], t.shape[1], t.shape[2] * 2, t.shape[3] * 2, dtype=t.dtype)
                z[:, :, ::2, ::2] = t
                return F.conv2d(F.pad(z, (2, 1, 2, 1)), kern, groups=t.shape[1])
            return F.conv2d(F.pad(t, (1, 1, 1, 1)), kern, stride=2, groups=t.shape[1])
        h_act = q(fir(a), 0).permute(0, 2, 3, 1)
        x_sc = q(fir(xs.permute(0, 3, 1, 2)), 0).permute(0, 2, 3, 1)
        h1, _ = conv_reference(h_act, None, 0, w0, 0, bias=padn(W["Conv_0.bias"], cop), temb=padn(tv, cop, 1))
    else:
        x_sc = xs
        h1, _ = conv_reference(xs, coef0, 1, w0, 0, bias=padn(W["Conv_0.bias"], cop), temb=padn(tv, cop, 1))
    h1 = q(h1, 0)
    coef1 = padn(gn_coef_reference(h1[..., :Cout], W["GroupNorm_1.weight"], W["GroupNorm_1.bias"], min(Cout // 4, 32)), cop, 1)
    w1 = torch.zeros(cop, cop, 3, 3); w1[:Cout, :Cout] = W["Conv_1.weight"]
    if "Conv_2.weight" in W:
        y, _ = conv_reference(h1, coef1, 1, w1, 0, xs=x_sc, w2=padn(padc(W["Conv_2.weight"][:, :, 0, 0], 1), cop),
                              bias=padn(W["Conv_1.bias"] + W["Conv_2.bias"], cop), scale=SQRT1_2)
    else:
        y, _ = conv_reference(h1, coef1, 1, w1, 0, bias=padn(W["Conv_1.bias"], cop), res=padn(xs, cop, 3), scale=SQRT1_2)
    assert Cout == cop or float(y[..., Cout:].abs().max()) == 0.0
    return q(y[..., :Cout], 0).permute(0, 3, 1, 2), torch.from_numpy(g["y"]).double()


@pytest.mark.parametrize("name,kw", [("plain", {}), ("widen", {}), ("down", {"down": True}), ("up", {"up": True}), ("cat", {"split": 32})])
def test_reference_composes_the_oracle_resblock(golden_dir, name, kw):
    """The res-block of the oracle (golden vectors generated from the reference model) rebuilt from conv_reference: a wrong term, order
    or scale in the reference would show here, so a kernel cannot agree with a broken reference by sharing its mistake."""
    g = np.load(os.path.join(golden_dir, f"resblock_{name}.npz"))
    got, want = _reference_resblock(g, **kw)
    err = float((got - want).abs().max() / want.abs().max())
    print(f"reference resblock_{name}: rel-max {err:.3g}")
    assert err < 2e-6, (name, err)


def _loop_reference(x, coef, act, w, xs, w2, bias, temb, res, scale, pyr, w4, b4):
    """use_op_conv written out element by element (fp32 storage, no rounding beyond float64)."""
    B, H, W, Cin = x.shape
    Cout, nt = w.shape[0], w.shape[-1] if w.dim() == 4 else 1
    out = torch.zeros(B, H, W, Cout, dtype=torch.float64)
    for b in range(B):
        for i in range(H):
            for j in range(W):
                for co in range(Cout):
                    acc = 0.0
                    for di in range(nt):
                        for dj in range(nt):
                            ii, jj = i + di - nt // 2, j + dj - nt // 2
                            if not (0 <= ii < H and 0 <= jj < W):
                                continue
                            for ci in range(Cin):
                                v = float(x[b, ii, jj, ci]) * float(coef[b, ci, 0]) + float(coef[b, ci, 1])
                                if act:
                                    v = v / (1.0 + math.exp(-v))
                                acc += v * float(w[co, ci, di, dj] if w.dim() == 4 else w[co, ci])
                    for ci in range(xs.shape[-1]):
                        acc += float(xs[b, i, j, ci]) * float(w2[co, ci])
                    acc += float(bias[co]) + float(temb[b, co]) + float(res[b, i, j, co])
                    acc *= scale
                    acc += float(b4[co]) + sum(float(pyr[b, i, j, k]) * float(w4[co, k]) for k in range(4))
                    out[b, i, j, co] = acc
    return out


@pytest.mark.parametrize("ntaps", [9, 1])
def test_reference_matches_a_direct_loop(ntaps):
    """conv_reference against the operator written as loops, every term present, on 2 x 3 x 4 pixels (border taps on every side)."""
    g = torch.Generator().manual_seed(11 + ntaps)
    B, H, W, Cin, Cout, XC = 2, 3, 4, 3, 2, 2
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, coef, xs = r(B, H, W, Cin), r(B, Cin, 2), r(B, H, W, XC)
    w = r(Cout, Cin, 3, 3) if ntaps == 9 else r(Cout, Cin)
    w2, bias, temb, res, pyr, w4, b4 = r(Cout, XC), r(Cout), r(B, Cout), r(B, H, W, Cout), r(B, H, W, 4), r(Cout, 4), r(Cout)
    want = _loop_reference(x, coef, 1, w, xs, w2, bias, temb, res, 0.7, pyr, w4, b4)
    # without the storage rounding (dt None) conv_reference must agree to float64 accuracy
    got, s = conv_reference(x, coef, 1, w, None, xs=xs, w2=w2, bias=bias, temb=temb, res=res, scale=0.7, pyr=pyr, w4=w4, b4=b4)
    assert float((got - want).abs().max()) < 1e-12 * float(want.abs().max())
    assert bool((s >= (got - (pyr @ w4.T + b4)).abs() / 0.7 - 1e-12).all())      # S bounds the pre-scale sum


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


def _guarded(shape, dtype, fill):
    """A device tensor of `shape` at the front of a buffer with TAIL sentinel elements behind it."""
    n = int(np.prod(shape))
    buf = torch.full((n + TAIL,), fill, dtype=dtype, device="cuda")
    return buf, buf[:n].view(*shape)


def _border_heavy(g, B, H, W, Cc, dt, scale=1.0):
    """Uniform values, four times larger on the first / last row and column (a wrong halo shows in the elementwise bound),
    plus a per-item offset (a wrong item shows)."""
    x = (torch.rand(B, H, W, Cc, generator=g, dtype=torch.float64) * 2 - 1) * scale
    x[:, 0] *= 4; x[:, -1] *= 4; x[:, :, 0] *= 4; x[:, :, -1] *= 4
    x += 0.25 * torch.arange(B, dtype=torch.float64)[:, None, None, None]
    return q(x, dt)


def _conv_op(f, variant, out_ptr, stats_ptr):
    """The use_conv_op of case data `f` (dict)."""
    op = _lib().UseConvOp()
    op.B, op.H, op.W, op.Cout, op.ntaps, op.act, op.dtype, op.out_dtype, op.variant = f["B"], f["H"], f["W"], f["Cout"], f["ntaps"], f["act"], f["dt"], f["odt"], variant
    op.C0, op.src0 = f["C0"], f["d_src0"].data_ptr()
    op.C1, op.src1 = f["C1"], (f["d_src1"].data_ptr() if f["C1"] else None)
    op.XC0, op.x0 = f["XC0"], (f["d_x0"].data_ptr() if f["XC0"] else None)
    op.XC1, op.x1 = f["XC1"], (f["d_x1"].data_ptr() if f["XC1"] else None)
    op.w = f["h_w"].ctypes.data
    op.w2 = f["h_w2"].ctypes.data if f["XC0"] else None
    op.bias = f["h_bias"].ctypes.data
    op.coef = f["d_coef"].data_ptr() if f["d_coef"] is not None else None
    op.temb = f["d_temb"].data_ptr() if f["d_temb"] is not None else None
    op.temb_bstride = f["temb_bstride"]
    op.res = f["d_res"].data_ptr() if f["d_res"] is not None else None
    op.out_scale = f["scale"]
    op.out = out_ptr
    op.stats = stats_ptr
    if f["d_pyr"] is not None:
        op.pyr, op.w4, op.b4 = f["d_pyr"].data_ptr(), f["h_w4"].ctypes.data, f["h_b4"].ctypes.data
    if f["gn"] == "st":
        op.gn_st0, op.gn_st1 = f["d_st0"].data_ptr(), (f["d_st1"].data_ptr() if f["C1"] else None)
        op.gn_gamma, op.gn_beta, op.gn_groups, op.gn_eps = f["d_gamma"].data_ptr(), f["d_beta"].data_ptr(), f["groups"], GN_EPS
    return op


def _conv_choice(f):
    """The kernel the library's dispatcher would run case data `f` on under the current options (use_conv_choice: nothing is launched)."""
    L = _lib()
    op = _conv_op(f, 0, f["d_src0"].data_ptr(), f["d_src0"].data_ptr() if f["stats"] else None)      # (present / absent is all that counts)
    name = C.create_string_buffer(32)
    L.check(L.lib().use_conv_choice(C.byref(op), name, 32, None), "use_conv_choice")
    return name.value.decode()


def _run_conv(f, variant):
    """One use_op_conv of case data `f` (dict) with the given variant: (rc, out, stats) on the CPU, the sentinels checked."""
    L = _lib()
    B, H, W, Cout, odt = f["B"], f["H"], f["W"], f["Cout"], f["odt"]
    obuf, out = _guarded((B, H, W, Cout), TD[odt], SENTINEL)
    sbuf = stats = None
    if f["stats"]:
        sbuf = torch.full((B * Cout * 2 + TAIL,), 0x5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        sbuf[:B * Cout * 2] = 0
        stats = sbuf[:B * Cout * 2].view(B, Cout, 2)
    op = _conv_op(f, variant, out.data_ptr(), stats.data_ptr() if stats is not None else None)
    rc = L.lib().use_op_conv(C.byref(op), _stream())
    torch.cuda.synchronize()
    if rc != 0:
        return rc, None, None
    tail = obuf[-TAIL:].float().cpu()
    assert bool((tail == SENTINEL).all()), "write past the end of out"
    if sbuf is not None:
        assert bool((sbuf[-TAIL:] == 0x5A5A5A5A5A5A).all()), "write past the end of stats"
    return rc, out.cpu(), (stats.cpu() if stats is not None else None)


def _producer(g, B, H, W, Cc, dt):
    """A source map written by a first use_op_conv (generic kernel, 1x1 from 32 channels, stats on), as the engine's producers write
    them: (stored values [B,H,W,Cc] float64, device tensor, device totals)."""
    L = _lib()
    prev = _border_heavy(g, B, H, W, 32, dt)
    w = (torch.randn(Cc, 32, generator=g) * 0.3).numpy().astype(np.float32)
    bias = (torch.randn(Cc, generator=g) * 0.5).numpy().astype(np.float32)
    d_prev = prev.to(TD[dt]).cuda()
    out = torch.empty(B, H, W, Cc, dtype=TD[dt], device="cuda")
    st = torch.zeros(B, Cc, 2, dtype=torch.int64, device="cuda")
    op = L.UseConvOp()
    op.B, op.H, op.W, op.Cout, op.ntaps, op.act, op.dtype, op.out_dtype, op.variant = B, H, W, Cc, 1, 0, dt, dt, 1
    op.C0, op.src0, op.w, op.bias, op.out_scale, op.out, op.stats = 32, d_prev.data_ptr(), w.ctypes.data, bias.ctypes.data, 1.0, out.data_ptr(), st.data_ptr()
    L.check(L.lib().use_op_conv(C.byref(op), _stream()), "use_op_conv (producer)")
    torch.cuda.synchronize()
    return out.double().cpu(), out, st


def _make_case(c, seed):
    """Case description -> operands on the device, host weights, and the float64 reference (ref, S, and the reference GN coefficients)."""
    g = torch.Generator().manual_seed(seed)
    dt, odt = c["dt"], c.get("odt", c["dt"])
    B, H, W, C0, C1, Cout = c["B"], c["H"], c["W"], c["C0"], c.get("C1", 0), c["Cout"]
    XC0, XC1, ntaps, gn, act = c.get("XC0", 0), c.get("XC1", 0), c.get("ntaps", 9), c.get("gn"), c.get("act", 0)
    creal = c.get("creal", Cout)                     # channels >= creal are zero padding: zero weights, bias, temb, res, w4, b4
    Cin = C0 + C1
    f = dict(B=B, H=H, W=W, C0=C0, C1=C1, Cout=Cout, XC0=XC0, XC1=XC1, ntaps=ntaps, act=act, dt=dt, odt=odt, gn=gn,
             stats=c.get("stats", 0), scale=c.get("scale", 1.0))
    if gn == "st":
        s0, f["d_src0"], f["d_st0"] = _producer(g, B, H, W, C0, dt)
        if C1:
            s1, f["d_src1"], f["d_st1"] = _producer(g, B, H, W, C1, dt)
        src = torch.cat([s0, s1], -1) if C1 else s0
        groups = min(Cin // 4, 32)
        gamma = 0.5 + torch.rand(Cin, generator=g, dtype=torch.float64)
        beta = torch.randn(Cin, generator=g, dtype=torch.float64) * 0.3
        f["groups"], f["d_gamma"], f["d_beta"] = groups, gamma.float().cuda(), beta.float().cuda()
        coef = gn_coef_reference(src, gamma.float(), beta.float(), groups)
        f["d_coef"] = None
    else:
        src = _border_heavy(g, B, H, W, Cin, dt)
        f["d_src0"] = src[..., :C0].to(TD[dt]).cuda().contiguous()
        if C1:
            f["d_src1"] = src[..., C0:].to(TD[dt]).cuda().contiguous()
        coef = None
        if gn == "coef":                             # per (item, channel), distinct per item
            a = (0.5 + torch.rand(B, Cin, generator=g, dtype=torch.float64)) * (1 + 0.2 * torch.arange(B, dtype=torch.float64)[:, None])
            b = torch.randn(B, Cin, generator=g, dtype=torch.float64) * 0.3 + 0.1 * torch.arange(B, dtype=torch.float64)[:, None]
            coef = torch.stack([a, b], -1).float().double()
        f["d_coef"] = coef.float().cuda().contiguous() if coef is not None else None
    wsc = 1.0 / math.sqrt(Cin * ntaps)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * wsc if ntaps == 9 else torch.randn(Cout, Cin, generator=g) * wsc
    w[creal:] = 0
    f["h_w"] = np.ascontiguousarray(w.numpy(), dtype=np.float32)
    bias = torch.randn(Cout, generator=g) * 0.2; bias[creal:] = 0
    f["h_bias"] = np.ascontiguousarray(bias.numpy(), dtype=np.float32)
    xs = w2 = None
    if XC0:
        xs = _border_heavy(g, B, H, W, XC0 + XC1, dt, 0.7)
        f["d_x0"] = xs[..., :XC0].to(TD[dt]).cuda().contiguous()
        if XC1:
            f["d_x1"] = xs[..., XC0:].to(TD[dt]).cuda().contiguous()
        w2 = torch.randn(Cout, XC0 + XC1, generator=g) / math.sqrt(XC0 + XC1); w2[creal:] = 0
        f["h_w2"] = np.ascontiguousarray(w2.numpy(), dtype=np.float32)
    temb = None
    f["d_temb"], f["temb_bstride"] = None, 0
    tm = c.get("temb")
    if tm:
        rows = torch.randn(B, Cout, generator=g).float() * 0.5 + torch.arange(B)[:, None]      # distinct per item
        rows[:, creal:] = 0
        if tm == "item":
            f["d_temb"], temb = rows.cuda().contiguous(), rows
        elif tm == "shared":
            f["d_temb"], f["temb_bstride"], temb = rows[:1].cuda().contiguous(), -1, rows[:1].expand(B, Cout)
        else:                                        # rows `stride` elements apart, junk in between
            stride = Cout + 40
            buf = torch.full((B, stride), 1e4)
            buf[:, :Cout] = rows
            f["d_temb"], f["temb_bstride"], temb = buf.cuda().contiguous(), stride, rows
    res = None
    f["d_res"] = None
    if c.get("res"):
        res = _border_heavy(g, B, H, W, Cout, odt, 0.8); res[..., creal:] = 0
        f["d_res"] = res.to(TD[odt]).cuda().contiguous()
    pyr = w4 = b4 = None
    f["d_pyr"] = None
    if c.get("pyr"):
        pyr = _border_heavy(g, B, H, W, 4, 0, 1.5)
        w4 = torch.randn(Cout, 4, generator=g).float() * 0.5; w4[creal:] = 0
        b4 = torch.randn(Cout, generator=g).float() * 0.5 + 0.25; b4[creal:] = 0
        f["d_pyr"] = pyr.float().cuda().contiguous()
        f["h_w4"] = np.ascontiguousarray(w4.numpy()); f["h_b4"] = np.ascontiguousarray(b4.numpy())
    ref, S = conv_reference(src, coef, act, w, dt, xs=xs, w2=w2, bias=bias, temb=temb, res=res, scale=f["scale"], pyr=pyr, w4=w4, b4=b4)
    return f, ref, S, creal


def _bound(ref, S, dt, odt, scale, K):
    u_in = UNIT[dt] if dt else 0.0
    return C_OUT * UNIT[odt] * ref.abs() + (C_IN * u_in + C_ACC * 2.0 ** -24 * math.sqrt(K)) * S * max(1.0, abs(scale))


def _check_stats(stats, out, odt, kern):
    """GroupNorm totals: stats / 2^20 against the float64 sum and sum of squares of the stored output."""
    B, H, W, Cout = out.shape
    v = out.double().reshape(B, H * W, Cout)
    want_s, want_q = v.sum(1), (v * v).sum(1)
    got_s, got_q = stats[..., 0].double() / 2 ** 20, stats[..., 1].double() / 2 ** 20
    # fp32 per-lane / per-workgroup partial sums (log2(H W) + 2 levels of rounding relative to the sum of magnitudes), the fixed-point
    # rounding of every workgroup's contribution (2^-21 each, at most one per pixel), and conv_v4 / conv_v5 summing the fp32 values
    # of which the stored ones are the roundings (u_out per value, 2 u_out for the squares)
    lev = (math.log2(H * W) + 2) * 2.0 ** -24
    u = UNIT[odt] if odt else 0.0
    tol_s = (lev + u) * v.abs().sum(1) + H * W * 2.0 ** -20
    tol_q = (lev + 2.01 * u) * (v * v).sum(1) + H * W * 2.0 ** -20
    rs = float(((got_s - want_s).abs() / tol_s).max())
    rq = float(((got_q - want_q).abs() / tol_q).max())
    assert rs < 1 and rq < 1, (kern, rs, rq)
    return max(rs, rq)


def _case_id(c):
    feats = [k if v is True or v == 1 else f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in c.items()
             if k not in ("kern", "dt", "B", "H", "W", "C0", "Cout") and v not in (0, None, False)]
    return (f"{KERNEL[c['kern']]}-{DT_NAME[c['dt']]}-B{c['B']}x{c['H']}x{c['W']}-C{c['C0']}" + (f"+{c['C1']}" if c.get("C1") else "") +
            f"-O{c['Cout']}" + ("-" + "-".join(feats) if feats else ""))


# The matrix.  Feature profiles follow the engine's conv() call sites (use_engine.cpp, Fwd): Conv_0 after FIR resampling (no GroupNorm,
# temb, stats), Conv_0 of a res-block (GroupNorm + SiLU of one or two concatenated sources, temb, stats), Conv_1 with the fused 1x1
# shortcut (GroupNorm + SiLU, XC0 [+ XC1], 1/sqrt 2, Combine pyr, stats), Conv_1 with the residual (1/sqrt 2, pyr, stats), the attention
# NIN (1x1, GroupNorm without SiLU; NIN_3 with residual and 1/sqrt 2, stats), the pyramid head (16-bit in, fp32 out, 4 channels,
# GroupNorm + SiLU, fp32 residual).  The GroupNorm comes as a coefficient array (large maps) or finalised in the kernel (gn "st").
RS = SQRT1_2
CONV0_FIR = dict(temb="item", stats=1)
CONV0 = dict(gn="st", act=1, temb="shared", stats=1)
CONV0_CAT = dict(gn="coef", act=1, temb="item", stats=1)
CONV1_SC = dict(gn="coef", act=1, scale=RS, pyr=1, stats=1)
CONV1_RES = dict(gn="st", act=1, res=1, scale=RS, stats=1)
CONV1_RES_PYR = dict(gn="coef", act=1, res=1, scale=RS, pyr=1, temb="stride")
PLAIN = dict(gn="coef", act=0)

CASES = []


def _add(kern, dt, B, H, W, C0, Cout, **kw):
    CASES.append(dict(kern=kern, dt=dt, B=B, H=H, W=W, C0=C0, Cout=Cout, **kw))


# conv_v4 / conv_v5: one tile, several tiles in each direction; Cout 128 / 256 / 384; Cin 32 / 64 / 160 (odd chunk count) / 512; split
# sources at a chunk boundary
for kern, dts in ((4, (0, 1, 2)), (5, (1, 2))):
    for i, dt in enumerate(dts):
        _add(kern, dt, 2, 16, 32, 32, 128, **CONV0_FIR)
        _add(kern, dt, 2, 48, 64, 96, 384, C1=64, **CONV0) if i != 1 else _add(kern, dt, 2, 48, 64, 96, 384, C1=64, **CONV0_CAT)
        _add(kern, dt, 1, 32, 160, 160, 256, XC0=96, XC1=64, **CONV1_SC)
        _add(kern, dt, 2, 16, 64, 512, 128, **CONV1_RES) if i != 2 else _add(kern, dt, 2, 16, 64, 512, 128, **CONV1_RES_PYR)
        _add(kern, dt, 2, 16, 32, 64, 256, creal=200, **PLAIN)
# conv_v2: exact and partial 16-pixel tiles; Cin up to 1024
for dt in (0, 1, 2):
    _add(2, dt, 2, 16, 17, 64, 128, **CONV0_FIR)
    _add(2, dt, 2, 31, 40, 128, 256, C1=64, **CONV0)
    _add(2, dt, 1, 17, 16, 1024, 128, XC0=64, XC1=64, **CONV1_SC)
    _add(2, dt, 2, 40, 31, 256, 128, **CONV1_RES_PYR)
    _add(2, dt, 1, 17, 31, 128, 64, creal=48, **CONV1_RES)
# conv_sk: 1 x N, 5 x 33, 7 x 9, 16 x 20; 3x3 and 1x1; the fp32-out pyramid heads (4 / 8 channels from 16-bit inputs)
for dt in (0, 1, 2):
    _add(7, dt, 2, 1, 40, 64, 64, **CONV0_FIR)
    _add(7, dt, 2, 5, 33, 64, 96, C1=32, **CONV0)
    _add(7, dt, 2, 7, 9, 128, 64, XC0=32, XC1=32, **CONV1_SC)
    _add(7, dt, 2, 16, 20, 96, 128, **CONV1_RES_PYR)
    _add(7, dt, 2, 7, 9, 128, 128, ntaps=1, gn="st", act=0, res=1, scale=RS, stats=1)
    _add(7, dt, 2, 16, 20, 64, 64, creal=40, **CONV1_RES)
for dt in (1, 2):
    _add(7, dt, 2, 7, 9, 64, 4, odt=0, gn="coef", act=1, res=1)
    _add(7, dt, 2, 16, 20, 128, 8, odt=0, gn="st", act=1)
# generic: what the dispatcher sends there (16-bit Cout 32 on maps above conv_sk's), and every profile forced
for dt in (0, 1, 2):
    _add(1, dt, 2, 24, 20, 64, 32, **CONV0) if dt else _add(1, dt, 2, 70, 64, 64, 32, **CONV0)
    _add(1, dt, 2, 9, 13, 64, 96, C1=32, **CONV0_CAT)
    _add(1, dt, 2, 12, 20, 64, 128, XC0=32, XC1=32, **CONV1_SC)
    _add(1, dt, 1, 17, 24, 128, 64, **CONV1_RES_PYR)
    _add(1, dt, 2, 10, 12, 64, 64, ntaps=1, gn="coef", act=0, res=1, scale=RS, stats=1)
    _add(1, dt, 2, 11, 19, 96, 64, creal=36, **CONV1_RES)
    _add(1, dt, 2, 8, 16, 32, 64, **CONV0_FIR)
for dt in (1, 2):
    _add(1, dt, 1, 40, 16, 128, 4, odt=0, gn="coef", act=1, res=1)

# ---- the forms launch_conv_sk picks (tests/conv_sk_forms.py mirrors the launcher; tests/test_conv_sk_forms_host.py holds the coverage) ----
# The conv_sk cases above all run NJ = 1 with one K pass per source and cpu_ <= 4.  The cases below are appended (a case's seed depends on
# its index) and each states the form it was written to reach, asserted from the mirror before anything is launched:
#   FORMS[index] = (NJ, CP, workgroups the tile-width rule compares, cpu_ per pass per source, weight branches)
N_CASES_ONE_FORM = len(CASES)
FORMS = {}


def _add_sk(form, dt, B, H, W, C0, Cout, **kw):
    FORMS[len(CASES)] = form
    _add(7, dt, B, H, W, C0, Cout, **kw)


CONV0_ST2 = dict(gn="st", act=1, scale=RS, stats=1, temb="item")                     # Conv_1 with the shortcut, GroupNorm from totals
NIN3 = dict(ntaps=1, gn="st", act=0, res=1, scale=RS, stats=1)
for dt in (1, 2):
    # NJ 1, CP 256: cpu_ 7, 5, 6, 8; a partial last pass with c_loc = 256; four passes on a 2-column map; a 1-column map
    _add_sk((1, 256, 5 * 2 * 4, [[7], [5], [6]], ("slab", "slab")), dt, 2, 16, 20, 224, 128, C1=160, XC0=192, **CONV1_SC)
    _add_sk((1, 256, 5 * 2 * 8, [[8], [8]], ("slab", None)), dt, 2, 16, 20, 256, 256, C1=256, **CONV0)
    _add_sk((1, 256, 2 * 2 * 2, [[8, 4]], ("slab", None)), dt, 2, 8, 10, 384, 64, creal=40, **CONV1_RES)
    _add_sk((1, 256, 1 * 2 * 8, [[8, 8, 8, 8]], ("slab", None)), dt, 2, 16, 2, 1024, 256, **CONV1_RES_PYR)
    _add_sk((1, 256, 1 * 2 * 8, [[8], [8], [8]], ("slab", "slab")), dt, 2, 8, 1, 256, 256, XC0=256, XC1=256, **CONV1_SC)
    # NJ 2, CP 128: two passes per source; a second source behind a partial pass, cpu_ 4, 1, 3, 2; the row-major weight branch (1x1);
    # Cout % 64 != 0 above the threshold stays NJ 1
    _add_sk((2, 128, 5 * 13 * 8, [[4, 4], [4, 4], [4, 4]], ("slab", "slab")), dt, 13, 16, 20, 256, 256, XC0=256, XC1=256, **CONV1_SC)
    _add_sk((2, 128, 2 * 33 * 8, [[4, 1], [3], [2]], ("slab", "slab")), dt, 33, 8, 10, 160, 256, C1=96, XC0=64, creal=200, **CONV0_ST2)
    _add_sk((2, 128, 2 * 33 * 8, [[4, 4]], ("row", None)), dt, 33, 8, 10, 256, 256, **NIN3)
    _add_sk((1, 256, 2 * 33 * 11, [[2]], ("slab", None)), dt, 33, 8, 10, 64, 352, **CONV0_FIR)
    # the fp32-out head with a partial second pass
    _add_sk((1, 256, 5 * 2 * 0, [[8, 4]], ("row", None)), dt, 2, 16, 20, 384, 4, odt=0, gn="coef", act=1, res=1)
# fp32 storage.  NJ 1, CP 128: two passes, a second source behind a partial pass
_add_sk((1, 128, 5 * 2 * 4, [[4, 4]], ("slab", None)), 0, 2, 16, 20, 256, 128, creal=100, **CONV1_RES)
_add_sk((1, 128, 1 * 2 * 2, [[4, 1], [3], [4, 1]], ("slab", "slab")), 0, 2, 7, 9, 160, 64, C1=96, XC0=160, **CONV1_SC)
# NJ 2, CP 64 (what fp32 training runs below 4096 pixels); exactly 512 workgroups (narrow) and 768 (wide): the two sides of the seam
_add_sk((2, 64, 64 * 3 * 4, [[2, 2]], ("slab", None)), 0, 3, 64, 64, 128, 128, **CONV1_RES_PYR)
_add_sk((2, 64, 16 * 3 * 12, [[2, 1], [2], [2, 1]], ("slab", "slab")), 0, 3, 64, 16, 96, 384, C1=64, XC0=96, **CONV1_SC)
_add_sk((1, 128, 64 * 2 * 4, [[2]], ("slab", None)), 0, 2, 64, 64, 64, 128, **CONV0)
_add_sk((2, 64, 64 * 2 * 6, [[2]], ("slab", None)), 0, 2, 64, 64, 64, 192, creal=150, **CONV0)
_add_sk((2, 64, 2 * 33 * 8, [[2, 2, 2, 2]], ("row", None)), 0, 33, 8, 10, 256, 256, **NIN3)
# tall maps of one or two columns, where the tallest tile of every width exceeds the halo: sk_tile's second round (22 x 2 and 21 x 1 tiles;
# before it these maps ran as 128 and 41 one-pixel tiles)
for dt in (0, 1, 2):
    _add_sk((1, 128 if dt == 0 else 256, 3 * 2 * 2, [[2], [1]], ("slab", None)), dt, 2, 64, 2, 64, 64, C1=32, **CONV0)
_add_sk((1, 256, 2 * 2 * 3, [[4], [1]], ("slab", "slab")), 1, 2, 41, 1, 128, 96, XC0=32, **CONV1_SC)

# conv_v4 / conv_v5 / conv_v2 re-order their workgroups per XCD only when gridDim.x % 8 == 0; no case above has such a grid.  2 x 4 = 8
# tiles (ragged in H for conv_v2), and 16 tiles, where the re-ordering is no longer the identity.  XCD_TILES[index] = gridDim.x
XCD_TILES = {}


def _add_xcd(tiles, kern, dt, B, H, W, C0, Cout, **kw):
    XCD_TILES[len(CASES)] = tiles
    _add(kern, dt, B, H, W, C0, Cout, **kw)


for kern, dts in ((4, (0, 1, 2)), (5, (1, 2))):
    for dt in dts:
        _add_xcd(8, kern, dt, 2, 32, 128, 64, 128, **CONV1_RES)
for dt in (0, 1, 2):
    _add_xcd(8, 2, dt, 2, 31, 64, 64, 128, **CONV0_CAT)
_add_xcd(16, 5, 1, 1, 32, 256, 64, 128, **CONV0_FIR)
_add_xcd(16, 2, 1, 1, 32, 128, 64, 128, **CONV0_FIR)


def _assert_form(c):
    """The case reaches the form it was written for (conv_sk: instantiation, workgroup count, passes, weight branches; XCD cases: the grid)."""
    import conv_sk_forms as skf
    i = CASES.index(c)
    if c["kern"] == 7:
        assert skf.sk_eligible(c), "conv_sk does not run this case"
        NJ, CP, tiles, wgs, passes = skf.sk_form(c)
        if i < N_CASES_ONE_FORM:
            assert NJ == 1 and all(len(p) == 1 and p[0] <= 4 for p in passes), (NJ, CP, passes)
        else:
            eNJ, eCP, ewgs, epasses, ebranch = FORMS[i]
            assert (NJ, CP, passes, skf.weight_branch(c)) == (eNJ, eCP, epasses, ebranch), (NJ, CP, wgs, passes, skf.weight_branch(c))
            assert wgs == ewgs, (tiles, wgs, ewgs)
    if i in XCD_TILES:
        n = skf.v2_tiles(c["H"], c["W"]) if c["kern"] == 2 else skf.wide_tiles(c["H"], c["W"])
        assert n == XCD_TILES[i] and n % 8 == 0, (n, XCD_TILES[i])


# what use_conv_choice may name when the dispatcher runs a case on the kernel its forced variant runs (variant 1: the pyramid head is one of its kernels)
CHOICE = {7: ("conv_sk",), 2: ("conv_v2",), 4: ("conv_v4",), 5: ("conv_v5",), 1: ("conv_generic", "pyr_conv", "pyr_conv_ws")}


def _dispatch_options(c):
    """Options under which variant 0 (the library's dispatcher) picks the case's kernel: conv_sk is switched off for the other kernels
    (fp32 sends every map up to 64 x 64 to it), conv_v4_min_blocks lowered for conv_v4 / conv_v5 on these small maps, conv_v5 switched
    off for 16-bit conv_v4."""
    k = c["kern"]
    if k == 7:
        return {}
    opts = {"conv_sk_max_px": 0}
    if k in (4, 5):
        opts["conv_v4_min_blocks"] = 1
        opts["conv_v5"] = 1 if k == 5 else 0
    return opts


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[_case_id(c) for c in CASES])
def test_conv_kernel_matches_float64_reference(c):
    kern, dt = c["kern"], c["dt"]
    _assert_form(c)
    f, ref, S, creal = _make_case(c, seed=len(_case_id(c)) * 7919 + CASES.index(c))
    rc, out, stats = _run_conv(f, kern)
    assert rc == 0, _lib().lib().use_last_error()
    out0 = stats0 = None
    try:
        for k, v in _dispatch_options(c).items():
            _set_option(k, v)
        chosen = _conv_choice(f)
        # the dispatcher picks the case's kernel - except that conv_v2 takes what it can run of the generic kernel's cases
        assert chosen in CHOICE[kern] or (kern == 1 and chosen == "conv_v2"), f"the dispatcher picks {chosen}, not {KERNEL[kern]}"
        if chosen in CHOICE[kern]:
            rc0, out0, stats0 = _run_conv(f, 0)
            assert rc0 == 0
    finally:
        _set_option("conv_sk_max_px", 16 * 20); _set_option("conv_v4_min_blocks", 80); _set_option("conv_v5", 1)
    got = out.double()
    assert bool(torch.isfinite(got).all()), "NaN / Inf in the output"
    if creal < f["Cout"]:
        assert float(got[..., creal:].abs().max()) == 0.0, "padding channels of a zero-padded Cout are not 0"
        assert stats is None or bool((stats[:, creal:] == 0).all()), "GroupNorm totals of padding channels are not 0"
    K = (f["C0"] + f["C1"]) * f["ntaps"] + f["XC0"] + f["XC1"]
    got, ref, S = got[..., :creal], ref[..., :creal], S[..., :creal]     # (the padding channels: exactly 0, above)
    bound = _bound(ref, S, dt, f["odt"], f["scale"], K)
    err = (got - ref).abs()
    ratio = float((err / bound).max())
    rel = float(err.max() / ref.abs().max())
    worst = np.unravel_index(int((err / bound).argmax()), err.shape)
    st_ratio = _check_stats(stats[:, :creal], out[..., :creal], f["odt"], KERNEL[kern]) if stats is not None else None
    print(f"[conv] {KERNEL[kern]:8s} {DT_NAME[dt]}->{DT_NAME[f['odt']]} B{f['B']} {f['H']}x{f['W']} Cin {f['C0']}+{f['C1']} "
          f"Cout {f['Cout']} taps {f['ntaps']} | {_case_id(c).split('-', 5)[-1]} | err/bound {ratio:.3f} at {tuple(int(i) for i in worst)} "
          f"rel-max {rel:.2e}" + (f" stats/bound {st_ratio:.3f}" if st_ratio is not None else ""))
    assert ratio < 1.0, (ratio, tuple(int(i) for i in worst))
    if dt:
        assert rel <= lp.op_bound(dt)
    if out0 is not None:
        assert torch.equal(out0, out), f"the dispatcher did not reach {KERNEL[kern]}"
        if stats is not None:
            assert torch.equal(stats0, stats)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [0, 1, 2])
def test_groupnorm_of_a_large_mean_map(dt):
    """A map whose channel mean is large against its spread (|mean| / std ~ 60; values ~30, within what the network's taps show): the
    fixed-point totals (stats / 2^20) against the float64 sums of the stored output, and the coefficients use_op_gn_finalize derives from
    them (mean and E[x^2] - mean^2 in fp64 from the totals) against float64 GroupNorm of the stored output.  The totals are accumulated
    in fp32 per lane and workgroup (relative error <= L 2^-24, L = log2(H W) + 2 levels) before the fixed-point sum, so the variance
    E[x^2] - mean^2 carries L 2^-24 (mean^2 + var) from the squares and 2 L 2^-24 mean^2 from the mean: a = gamma rstd has the stated
    bound 1.5 (1 + (mean / std)^2) L 2^-24 relative (~3e-3 at mean / std = 70).  That is far above fp32 GroupNorm on the CPU on the same
    data (torch's two-level fp32 reduction, printed beside it); the engine takes it: GroupNorm feeds a 16-bit operand in the
    production modes (2^-8 / 2^-11), and the network's maps measure |mean| / std well below this case's (the sampler parity tests
    bound the whole chain).  Centring the totals would change every GroupNorm of the network."""
    L = _lib()
    g = torch.Generator().manual_seed(99 + dt)
    B, H, W, Cc = 2, 32, 40, 64
    x = q(torch.rand(B, H, W, Cc, generator=g, dtype=torch.float64) * 2 - 1, dt)
    w = torch.randn(Cc, Cc, generator=g) * (0.5 / math.sqrt(Cc))
    bias = 20.0 + torch.rand(Cc, generator=g)                 # mean ~20, spread within a group ~0.4
    out = torch.empty(B, H, W, Cc, dtype=TD[dt], device="cuda")
    st = torch.zeros(B, Cc, 2, dtype=torch.int64, device="cuda")
    d_x = x.to(TD[dt]).cuda()
    hw, hb = np.ascontiguousarray(w.numpy()), np.ascontiguousarray(bias.numpy())
    op = L.UseConvOp()
    op.B, op.H, op.W, op.Cout, op.ntaps, op.act, op.dtype, op.out_dtype, op.variant = B, H, W, Cc, 1, 0, dt, dt, 0
    op.C0, op.src0, op.w, op.bias, op.out_scale, op.out, op.stats = Cc, d_x.data_ptr(), hw.ctypes.data, hb.ctypes.data, 1.0, out.data_ptr(), st.data_ptr()
    L.check(L.lib().use_op_conv(C.byref(op), _stream()), "use_op_conv")
    torch.cuda.synchronize()
    y = out.double().cpu()
    st_ratio = _check_stats(st.cpu(), y, dt, "large-mean")
    groups = 16
    gamma = torch.ones(Cc); beta = torch.zeros(Cc)
    d_gamma, d_beta = gamma.cuda(), beta.cuda()
    coef = torch.empty(B, Cc, 2, device="cuda")
    L.check(L.lib().use_op_gn_finalize(C.c_void_p(st.data_ptr()), Cc, None, 0, C.c_void_p(d_gamma.data_ptr()), C.c_void_p(d_beta.data_ptr()),
                                       groups, H * W, GN_EPS, C.c_void_p(coef.data_ptr()), B, _stream()), "use_op_gn_finalize")
    torch.cuda.synchronize()
    want = gn_coef_reference(y, gamma, beta, groups)
    yg = y.permute(0, 3, 1, 2).reshape(B, groups, -1)
    ratio_ms = float((yg.mean(-1).abs() / yg.std(-1)).min())
    # fp32 GroupNorm (CPU, torch) on the same stored data
    v32, m32 = torch.var_mean(y.float().permute(0, 3, 1, 2).reshape(B, groups, -1), -1, unbiased=False)
    a32 = (1.0 / torch.sqrt(v32 + GN_EPS)).repeat_interleave(Cc // groups, 1).double()
    err_a = float(((coef.double().cpu()[..., 0] - want[..., 0]) / want[..., 0]).abs().max())
    err_a32 = float(((a32 - want[..., 0]) / want[..., 0]).abs().max())
    mean_std = float((yg.mean(-1).abs() / yg.std(-1)).max())
    bound = 1.5 * (1 + mean_std ** 2) * (math.log2(H * W) + 2) * 2.0 ** -24
    # b = beta - mean a = -mean a here: relative error that of a plus that of the mean (~2^-24 L)
    err_b = float(((coef.double().cpu()[..., 1] - want[..., 1]) / want[..., 1]).abs().max())
    print(f"[gn-large-mean] {DT_NAME[dt]} |mean|/std {ratio_ms:.0f}..{mean_std:.0f} stats/bound {st_ratio:.3f} | coefficient a: "
          f"finalize rel err {err_a:.2e}, fp32 CPU GroupNorm {err_a32:.2e}, stated bound {bound:.2e} | b: {err_b:.2e}")
    assert 30 <= ratio_ms and mean_std <= 100
    assert err_a <= bound and err_b <= 2 * bound, (err_a, err_b, bound)


REFUSALS = [
    # (variant, dt, odt, H, W, C0, C1, Cout, what)
    (4, 1, 1, 16, 32, 512, 32, 128, "Ctot 544 > 512"),
    (5, 2, 2, 16, 32, 512, 32, 128, "Ctot 544 > 512"),
    (4, 0, 0, 16, 32, 512, 32, 128, "Ctot 544 > 512 (fp32)"),
    (5, 0, 0, 16, 32, 64, 0, 128, "fp32 storage"),
    (4, 1, 1, 24, 32, 64, 0, 128, "H % 16"),
    (5, 1, 1, 16, 48, 64, 0, 128, "W % 32"),
    (4, 1, 1, 16, 32, 64, 0, 32, "Cout <= 32"),
    (4, 1, 0, 16, 32, 64, 0, 128, "in_dtype != out_dtype"),
    (2, 1, 1, 16, 16, 64, 0, 32, "conv_v2 Cout <= 32"),
    (2, 1, 1, 16, 16, 96, 0, 128, "conv_v2 16-bit Cin % 64"),
    (7, 1, 1, 32, 32, 64, 0, 64, "conv_sk map > 320 px"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("r", REFUSALS, ids=[r[-1] for r in REFUSALS])
def test_forced_variant_refuses_what_its_kernel_cannot_run(r):
    """A forced variant on a case its kernel cannot run returns USE_E_INVALID (nothing is launched; the output keeps its sentinel)."""
    L = _lib()
    variant, dt, odt, H, W, C0, C1, Cout, what = r
    B = 1
    src0 = torch.zeros(B, H, W, C0, dtype=TD[dt], device="cuda")
    src1 = torch.zeros(B, H, W, max(C1, 1), dtype=TD[dt], device="cuda")
    out = torch.full((B, H, W, Cout), 3.0, dtype=TD[odt], device="cuda")
    w = np.zeros((Cout, C0 + C1, 3, 3), dtype=np.float32)
    op = L.UseConvOp()
    op.B, op.H, op.W, op.Cout, op.ntaps, op.act, op.dtype, op.out_dtype, op.variant = B, H, W, Cout, 9, 0, dt, odt, variant
    op.C0, op.src0, op.C1, op.src1 = C0, src0.data_ptr(), C1, (src1.data_ptr() if C1 else None)
    op.w, op.out_scale, op.out = w.ctypes.data, 1.0, out.data_ptr()
    rc = L.lib().use_op_conv(C.byref(op), _stream())
    msg = L.lib().use_last_error().decode()
    print(f"[refuse] variant {variant} {what}: rc {rc} '{msg}'")
    assert rc != 0 and "cannot run" in msg, (what, rc, msg)
    assert bool((out == 3.0).all())
    if variant in (4, 5):                            # the bench harness refuses through the same predicate
        case = L.UseConvCase(B=1, H=H, W=W, C0=C0, C1=C1, Cout=Cout, XC0=0, XC1=0, act=0, gn=0, temb=0, res=0, stats=0,
                             dtype=dt, variant=variant, iters=1) if odt == dt else None
        if case is not None:
            ms, fl = C.c_double(), C.c_double()
            rc2 = L.lib().use_conv_bench(C.byref(case), None, None, C.byref(ms), C.byref(fl))
            assert rc2 != 0 and "cannot run" in L.lib().use_last_error().decode()
