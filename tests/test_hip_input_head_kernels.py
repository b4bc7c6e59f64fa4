"""The two ends of a score evaluation, one launch at a time through use_op_conv, against plain float64 references: the network's input
convolution (conv_in_kernel, conv_in_split_kernel<., FULL / masked>, and conv_kernel<float, ., 4, ...> on the 8-channel input of
condition="both"), the pyramid head (pyr_conv_kernel, pyr_conv_ws_kernel in every walk form), the GroupNorm totals of these kernels in
both forms (atomics on `stats`, per-workgroup partial totals in `stats_part`), the partial totals of the wide conv, and
gn_finalize_part_kernel through use_op_gn_finalize_parts.  Same construction as tests/test_hip_conv_kernels.py, whose reference
(`conv_reference`), bound (`_bound`), sentinels and data helpers are imported.  All constants below were fixed before the first GPU run;
none is fitted.  Every case prints its worst |err| / bound, where it occurs, and the kernel use_conv_choice names; every ratio must stay
below 1.

Bounds, per element.  S is conv_reference's expression on absolute values (conv(|x|, |w|) + |bias| + |res|, before the out_scale),
u_out the unit roundoff of the output type, C_ACC = 2.

conv_in_kernel (fp32 operands on v_mfma_f32_32x32x2f32, K = 4 x 9 = 36 products in one fp32 accumulator, bias and out_scale in the fp32
epilogue): `_bound` with u_in = 0 (fp32 storage: nothing is rounded that the reference does not round),
    u_out |ref| + C_ACC 2^-24 sqrt(36) S max(1, |out_scale|).
conv_kernel<float, ., 4, 128, 2, 2> on the 8-channel input (two 4-channel chunks per tap): the same with K = 72.

conv_in_split_kernel.  The reference is the plain fp32-operand float64 convolution - not a model of the split.  With round-to-nearest
bf16 (relative 2^-9): x = xh + xl + rx, |xl| <= 2^-9 |x|, |rx| <= 2^-18 |x|; likewise w.  The kernel computes xh wh + xh wl + xl wh (exact
bf16 products, fp32 accumulation started from the bias, K = 3 x 36 = 108); what it drops is xl wl + rx w + x rw, at most
3 x 2^-18 (1 + 2^-8) |x| |w| < 2^-16 |x| |w|:
    u_out |ref| + (2^-16 + C_ACC 2^-24 sqrt(108)) S max(1, |out_scale|)            (S contains |bias|).
A float64 model of the kernel (xh / xl / wh / wl formed as pack_conv_in_split and the kernel form them) stays inside this bound on the
GPU cases' shapes in the CPU part below; the output rounding at the bottom of a binade is what takes it to ~0.9.

Pyramid head (16-bit in, fp32 out, K = 9 C0): `_bound` unchanged,  2^-24 |ref| + (u_in + C_ACC 2^-24 sqrt(9 C0)) S  - the u_in S term is
the activated halo value rounding to a neighbour of the reference's (the device SiLU uses v_exp / v_rcp).

GroupNorm totals of the input convolution.  Every kernel here sums the STORED values re-expanded (Vec16::load of the packed chunk), so
there is no u_out term:
    |stats / 2^20 - sum v| <= n_ser 2^-24 sum |v| + parts_per_channel x 2^-21,   |. - sum v^2| <= n_sq 2^-24 sum v^2 + parts x 2^-21.
parts_per_channel = workgroup contributions per (item, channel), each one __float2ll_rn of an fp32 sum scaled by 2^20 (half a unit =
2^-21).  n_ser = the roundings a value can pass through: a serial chain of n terms has n - 1 (the first addition, to 0, is exact):
  conv_in_split_kernel: a lane adds 4 pixels per half tile row pair, 8 per tile, over the `tpw` tiles of its workgroup's walk
      (8 tpw - 1), reduce_lanes_stride<16> (2), the 4 waves summed serially through LDS (3):       n_ser = 8 tpw + 4      (= 8 tpw + 2 + 2)
  conv_in_kernel<float>: 16 passes of 2 pixels (15), reduce_lanes_stride<32> (1), 4 waves (3):     n_ser = 19
  conv_in_kernel<16 bit>: 8 passes of 4 pixels (7), reduce_lanes_stride<16> (2), 4 waves (3):     n_ser = 12
  conv_kernel<float, float, 4, 128, 2, 2>: TM x QN = 2 x 8 pixels (15), stride 16 (2), WM = 2 (1): n_ser = 18
  conv_kernel<float, 16 bit, 4, 128, 2, 2>: 2 x 4 pixels (7), stride 8 (3), WM = 2 (1):            n_ser = 11
Squares: the square of a stored 16-bit value is exact in fp32 (8 / 11 significand bits), so n_sq = n_ser; an fp32 square is rounded
once before it is added (or not at all, if the compiler contracts it into an fma): n_sq = n_ser + 1 for fp32 output.

Partial totals.  stats_part summed over its parts in int64 on the host IS the stats of the same launch in atomic form (the same integers,
bit for bit); `out` is bit-identical between the forms; every (item, part, channel < Cout) entry is written (the buffer is pre-filled
with a pattern) and nothing behind it.  The wide conv (conv_v4 / conv_v5) sums its fp32 values, not the stored ones: its totals keep
`_check_stats`'s bound.

use_op_gn_finalize_parts: coefficients from partials are bit-identical to use_op_gn_finalize on the summed totals (integer sums, the
same arithmetic behind them) and lie within the bound test_groupnorm_of_a_large_mean_map derives against float64 GroupNorm of the
stored map: a relative 1.5 (1 + (mean / std)^2) L 2^-24, L = log2(HW) + 2; b = beta - mean a absolute 2 x that x (|beta| + |mean a|).

`-m "not gpu"`: conv_reference at C0 = 4 / 8 reproduces the oracle's h_in tap (ncsnpp_forward(..., taps=) on a 64 x 64 slice of the golden
inputs), and the mutation controls on the GPU cases' shapes: the float64 model of the split kernel stays under the bound, and each of
{xl wh dropped, xh wl dropped, the lo blocks of one operand swapped (wl meets xl, wh meets xh twice), one halo row of one tile taken from
the tile above unshifted, the residual of the next tile of the walk added, one partial total left out} exceeds it.  No exemption was
needed.

Measured on the MI355X, worst |err| / bound per family: conv_in 0.44 (fp32 output: the accumulation term alone) and 0.988 (16-bit output at
Cout 32), conv_in_split bf16 0.986 / fp16 0.948, conv_generic at C0 = 8 0.27 (fp32 output) and 0.995 (16-bit) - the store-bound ones at
the output rounding at the bottom of a binade, where the float64 model of the split kernel stands too (0.985 / 0.953 on the CPU);
input-convolution totals 0.13; wide-conv partial totals 0.15 (out 0.28); finalize from partials 0.13 on a, 0.05 on b (exact sums
behind the fixed-point totals: the bit identity is what that test is about).  pyr_conv and pyr_conv_ws 0.020 (fp16) / 0.009 (bf16),
0.000 without the SiLU, the same bits in every form: the head stores fp32, so there is no store rounding to fill the bound, and the
bound's u_in S term lets every one of the K = 1152 / 2304 activated operands round to its neighbour in the same direction, where the
device SiLU in fact moves a few per thousand of them, in either direction.  The bound still separates what it is there to catch: a
single wrong halo row is 15 - 24 (bf16) / 136 - 220 (fp16) times the bound, the next tile's residual 52 - 872 times (CPU part).  No
kernel bug was found.  The CPU part takes about 4 s."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_hip_conv_kernels import (C_ACC, CONV0, CONV1_RES, DT_NAME, GN_EPS, SENTINEL, TAIL, TD, UNIT, _bound, _border_heavy, _check_stats,
                                   _conv_op, _dispatch_options, _guarded, _lib, _make_case, _set_option, _stream, conv_reference,
                                   gn_coef_reference, q)

TILE_H, TILE_W = 8, 16
PATTERN = 0x5A5A5A5A5A5A            # pre-fill of the totals buffers: no total of these cases comes near it (9.5e7 x 2^20)
INVALID = -1
U32 = 2.0 ** -24


def _tiles(H, W):
    return (H + TILE_H - 1) // TILE_H, (W + TILE_W - 1) // TILE_W


# ---------------------------------------------------------------------------------------------------------------------------
# input convolution: data, float64 model of the split kernel, bounds
# ---------------------------------------------------------------------------------------------------------------------------
def _in_data(c, seed):
    """Operands of an input-convolution case (CPU): x [B,H,W,C0] (fp32 values in float64, border-heavy, items distinct; with C0 = 8 the
    last two channels are non-zero as well and meet non-zero weights), w [Cout,C0,3,3] fp32, bias [Cout] fp32 or None, the float64
    reference and S."""
    g = torch.Generator().manual_seed(seed)
    B, H, W, C0, Cout = c["B"], c["H"], c["W"], c["C0"], c["Cout"]
    x = _border_heavy(g, B, H, W, C0, 0)
    w = (torch.randn(Cout, C0, 3, 3, generator=g) / math.sqrt(9 * C0)).float()
    bias = (torch.randn(Cout, generator=g) * 0.2).float() if c.get("bias", 1) else None
    ref, S = conv_reference(x, None, 0, w, 0, bias=bias, scale=c.get("scale", 1.0))
    return dict(x=x, w=w, bias=bias, ref=ref, S=S, scale=c.get("scale", 1.0))


def _bf16_split(v32):
    """hi = bf16(v), lo = bf16(v - hi) of an fp32 tensor, as the kernel (x) and pack_conv_in_split (w) form them; float64."""
    hi = v32.to(torch.bfloat16).float()
    lo = (v32 - hi).to(torch.bfloat16).float()          # (v - hi is exact in fp32)
    return hi.double(), lo.double()


def _split_model(d, odt, mut=None):
    """float64 model of conv_in_split_kernel: (bias + xh wh + xh wl + xl wh) * out_scale rounded to the output type.  mut: a
    deliberately wrong variant (mutation controls)."""
    xh, xl = _bf16_split(d["x"].float().permute(0, 3, 1, 2))
    wh, wl = _bf16_split(d["w"])
    cv = lambda a, b: F.conv2d(a, b, padding=1)
    blocks = {"hh": cv(xh, wh), "hl": cv(xh, wl), "lh": cv(xl, wh)}
    if mut == "drop_lh":
        blocks["lh"] = 0.0
    elif mut == "drop_hl":
        blocks["hl"] = 0.0
    elif mut == "swap_lo":                               # x blocks [xh, xl, xh] against w blocks [wh, wl, wh]
        blocks["hl"], blocks["lh"] = cv(xl, wl), cv(xh, wh)
    y = (blocks["hh"] + blocks["hl"] + blocks["lh"]).permute(0, 2, 3, 1)
    if d["bias"] is not None:
        y = y + d["bias"].double()
    return q(y * d["scale"], odt)


def _in_bound(d, odt, kern, C0):
    if kern == "conv_in_split":
        return UNIT[odt] * d["ref"].abs() + (2.0 ** -16 + C_ACC * U32 * math.sqrt(108)) * d["S"] * max(1.0, abs(d["scale"]))
    return _bound(d["ref"], d["S"], 0, odt, d["scale"], 9 * C0)


def _n_ser(kern, odt, tpw):
    """(n_ser, n_sq) of the totals bound (module docstring)."""
    n = {"conv_in_split": 8 * tpw + 4, "conv_in": 19 if odt == 0 else 12, "conv_generic": 18 if odt == 0 else 11}[kern]
    return n, n + (1 if odt == 0 else 0)


def _totals_ratio(stats, out, n_ser, n_sq, parts):
    """GroupNorm totals (stats / 2^20) against the float64 sums of the stored output: worst |err| / bound."""
    B, H, W, Cout = out.shape
    v = out.double().reshape(B, H * W, Cout)
    want_s, want_q = v.sum(1), (v * v).sum(1)
    got_s, got_q = stats[..., 0].double() / 2 ** 20, stats[..., 1].double() / 2 ** 20
    tol_s = n_ser * U32 * v.abs().sum(1) + parts * 2.0 ** -21
    tol_q = n_sq * U32 * want_q + parts * 2.0 ** -21
    return max(float(((got_s - want_s).abs() / tol_s).max()), float(((got_q - want_q).abs() / tol_q).max()))


def _finalize_ratios(got, want, mean, std, beta, HW, cpg):
    """Finalised GroupNorm coefficients got [B,C,2] against float64 ones: worst |err| / bound of a and of b (module docstring); mean, std
    [B,groups] of the map's groups, cpg channels per group."""
    bnd = (1.5 * (1 + (mean / std) ** 2) * (math.log2(HW) + 2) * U32).repeat_interleave(cpg, 1)
    ra = float(((got[..., 0] - want[..., 0]).abs() / (bnd * want[..., 0].abs())).max())
    rb = float(((got[..., 1] - want[..., 1]).abs() / (2 * bnd * (beta.double().abs()[None] + (mean.repeat_interleave(cpg, 1) * want[..., 0]).abs()))).max())
    return ra, rb


def _worst(got, ref, bound):
    r = (got - ref).abs() / bound
    return float(r.max()), tuple(int(i) for i in np.unravel_index(int(r.argmax()), r.shape))


# ---------------------------------------------------------------------------------------------------------------------------
# pyramid head: data on the CPU (the mutation controls; the GPU cases go through test_hip_conv_kernels._make_case)
# ---------------------------------------------------------------------------------------------------------------------------
def _pyr_data(B, H, W, Cc, dt, seed, Cout=4):
    g = torch.Generator().manual_seed(seed)
    x = _border_heavy(g, B, H, W, Cc, dt)
    a = (0.5 + torch.rand(B, Cc, generator=g, dtype=torch.float64)) * (1 + 0.2 * torch.arange(B, dtype=torch.float64)[:, None])
    b = torch.randn(B, Cc, generator=g, dtype=torch.float64) * 0.3 + 0.1 * torch.arange(B, dtype=torch.float64)[:, None]
    coef = torch.stack([a, b], -1).float().double()
    w = torch.randn(Cout, Cc, 3, 3, generator=g) / math.sqrt(9 * Cc)
    bias = torch.randn(Cout, generator=g) * 0.2
    res = _border_heavy(g, B, H, W, Cout, 0, 0.8)
    return dict(x=x, coef=coef, w=w, bias=bias, res=res)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU part
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,arch,key_t", [("forward_large", "LARGE", "t_b"), ("both", "LARGE_BOTH", "t")])
def test_reference_reproduces_the_oracles_input_convolution(golden_dir, name, arch, key_t):
    """conv_reference at C0 = 4 (and 8: the 6-channel input, two zero channels) against the oracle's h_in tap on a 64 x 64 slice of the
    golden input: the reference of this file is pinned to what already pins the project.  The oracle convolves in fp32 (K = 36 / 54):
    its own error is inside C_ACC 2^-24 sqrt(K) S + 2^-24 |ref|."""
    from oracle import ncsnpp_oracle as no
    from universal_speech_enhancement_amd.testing import weights as tw
    g = np.load(os.path.join(golden_dir, f"{name}.npz"))
    sd = no.to_torch(tw.make_state_dict(int(g["weights_seed"]), **getattr(tw, arch)))
    x = torch.from_numpy(g["x"])[:, :, 100:164, :64]
    taps = {}
    with torch.no_grad():
        no.ncsnpp_forward(sd, x, torch.from_numpy(g[key_t]), taps=taps)
    want = taps["h_in"].double().permute(0, 2, 3, 1)
    # the packed input as launch_pack_input writes it: 2 (re, im of each complex input) - 1 in fp32, zero channels behind 6
    x4 = torch.cat([p for k in range(x.shape[1]) for p in (x[:, [k]].real, x[:, [k]].imag)], dim=1).float() * 2 - 1.0
    cin = x4.shape[1]
    C0 = 4 if cin == 4 else 8
    xp = torch.zeros(x4.shape[0], 64, 64, C0, dtype=torch.float64)
    xp[..., :cin] = x4.permute(0, 2, 3, 1).double()
    w = torch.zeros(want.shape[-1], C0, 3, 3)
    w[:, :cin] = sd["all_modules.3.weight"]
    ref, S = conv_reference(xp, None, 0, w, 0, bias=sd["all_modules.3.bias"])
    ratio, pos = _worst(want, ref, C_ACC * U32 * math.sqrt(9 * cin) * S + U32 * ref.abs())
    print(f"[ref] conv_reference C0 {C0} against the oracle's h_in ({name}): err/bound {ratio:.3f} at {pos}")
    assert ratio < 1.0


SPLIT_SHAPES = [(16, 32, 128), (24, 48, 128), (19, 37, 96), (19, 37, 128), (8, 16, 128)]


@pytest.mark.parametrize("odt", [1, 2])
@pytest.mark.parametrize("shape", SPLIT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_split_model_holds_the_bound_and_its_mutations_do_not(shape, odt):
    """The float64 model of conv_in_split_kernel on the GPU cases' shapes: inside the bound; with the xl wh block dropped, the xh wl block
    dropped, or the lo blocks of one operand swapped: outside."""
    H, W, Cout = shape
    d = _in_data(dict(B=2, H=H, W=W, C0=4, Cout=Cout, scale=0.7 if H == 19 and Cout == 128 else 1.0), seed=H * 100 + W + Cout)
    bound = _in_bound(d, odt, "conv_in_split", 4)
    ok, _ = _worst(_split_model(d, odt), d["ref"], bound)
    split_only = float(((_split_model(d, None) - d["ref"] * 1.0).abs() / (2.0 ** -16 * d["S"] * max(1.0, d["scale"]))).max())
    muts = {m: _worst(_split_model(d, odt, m), d["ref"], bound)[0] for m in ("drop_lh", "drop_hl", "swap_lo")}
    print(f"[mut] split model {DT_NAME[odt]} {H}x{W}x{Cout}: model {ok:.3f} (the split alone {split_only:.3f} x 2^-16 S) | " +
          " ".join(f"{m} {r:.1f}" for m, r in muts.items()))
    assert ok < 1.0 and split_only < 1.0
    for m, r in muts.items():
        assert r > 1.0, (m, r)


@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("shape", [(40, 48, 128), (43, 37, 128), (43, 37, 256)], ids=lambda s: "x".join(map(str, s)))
def test_pyramid_reference_mutations_exceed_the_bound(shape, dt):
    """The roll's and the prefetch's failure modes on the GPU cases' shapes: halo row 0 of one tile (the map row above it) taken from the
    tile above unshifted (that tile's halo row 0, eight rows up), and the residual of the next tile of the walk added instead of the
    tile's own.  Either moves the reference far outside the bound."""
    H, W, Cc = shape
    B = 2
    d = _pyr_data(B, H, W, Cc, dt, seed=H + W + Cc + dt)
    ref, S = conv_reference(d["x"], d["coef"], 1, d["w"], dt, bias=d["bias"], res=d["res"])
    bound = _bound(ref, S, dt, 0, 1.0, 9 * Cc)
    ty, tx = 2, 1
    y0, x0 = ty * TILE_H, tx * TILE_W
    # halo row 0 of tile (ty, tx): map row y0 - 1, columns x0 - 1 .. x0 + 16; the tile above has map row y0 - 9 there
    xm = d["x"].clone()
    lo, hi = max(x0 - 1, 0), min(x0 + TILE_W + 1, W)
    xm[:, y0 - 1, lo:hi] = d["x"][:, y0 - 1 - TILE_H, lo:hi]
    refm, _ = conv_reference(xm, d["coef"], 1, d["w"], dt, bias=d["bias"], res=d["res"])
    halo = ref.clone()
    halo[:, y0, x0:x0 + TILE_W] = refm[:, y0, x0:x0 + TILE_W]           # only the tile's first row reads its halo row 0
    r_halo, _ = _worst(halo, ref, bound)
    # the next tile of the walk: the tile below in a column strip (one block), the tile to the right row by row (two blocks)
    ry, rx = 2 * TILE_H, 0
    ny, nx = (ry + TILE_H, rx) if Cc == 128 else (ry, rx + TILE_W)
    resm = ref.clone()
    resm[:, ry:ry + TILE_H, rx:rx + TILE_W] += d["res"][:, ny:ny + TILE_H, nx:nx + TILE_W] - d["res"][:, ry:ry + TILE_H, rx:rx + TILE_W]
    r_res, _ = _worst(resm, ref, bound)
    print(f"[mut] pyramid {DT_NAME[dt]} {H}x{W} C{Cc}: halo row from the tile above {r_halo:.1f}, residual of the next tile {r_res:.1f}")
    assert r_halo > 1.0 and r_res > 1.0


@pytest.mark.parametrize("odt", [1, 2])
def test_a_left_out_partial_total_exceeds_the_totals_bound(odt):
    """Totals of the split model's stored output on the 9-tile case, summed per workgroup as the kernel's walk of 3 sums them (float64,
    then the fixed-point rounding): inside the totals bound; with one workgroup's partial left out: outside."""
    d = _in_data(dict(B=2, H=24, W=48, C0=4, Cout=128), seed=24 * 100 + 48 + 128)
    out = _split_model(d, odt)
    tpw, parts = 3, 3
    ty, tx = _tiles(24, 48)
    tiles = [out[:, (t // tx) * TILE_H:(t // tx + 1) * TILE_H, (t % tx) * TILE_W:(t % tx + 1) * TILE_W].reshape(2, -1, 128) for t in range(ty * tx)]
    part = torch.stack([torch.stack([torch.round(torch.cat(tiles[p * tpw:(p + 1) * tpw], 1).pow(e).sum(1) * 2 ** 20) for e in (1, 2)], -1)
                        for p in range(parts)], 1).long()                                # [B][parts][Cout][2]
    n_ser, n_sq = _n_ser("conv_in_split", odt, tpw)
    ok = _totals_ratio(part.sum(1), out, n_ser, n_sq, parts)
    bad = _totals_ratio(part[:, :2].sum(1), out, n_ser, n_sq, parts)
    print(f"[mut] totals {DT_NAME[odt]}: all partials {ok:.3f}, one left out {bad:.1f}")
    assert ok < 1.0 < bad


# ---------------------------------------------------------------------------------------------------------------------------
# GPU part
# ---------------------------------------------------------------------------------------------------------------------------
def _choice(f, stats):
    """(kernel name, partial totals per (item, channel)) use_conv_choice answers for case data `f` under the current options."""
    L = _lib()
    op = _conv_op(f, 0, f["d_src0"].data_ptr(), f["d_src0"].data_ptr() if stats else None)     # (present / absent is all that counts)
    name, parts = C.create_string_buffer(32), C.c_int(-1)
    L.check(L.lib().use_conv_choice(C.byref(op), name, 32, C.byref(parts)), "use_conv_choice")
    return name.value.decode(), parts.value


def _launch(f, variant, totals):
    """One use_op_conv of case data `f`; totals None / "atomic" / "part".  Returns (out, stats [B,Cout,2] or None, partials
    [B,parts,Cout,2] or None, kernel name, parts), on the CPU; the sentinels behind out, stats and stats_part are checked, and that
    every entry of stats_part was written."""
    L = _lib()
    B, H, W, Cout, odt = f["B"], f["H"], f["W"], f["Cout"], f["odt"]
    name, parts = _choice(f, totals is not None)
    obuf, out = _guarded((B, H, W, Cout), TD[odt], SENTINEL)
    sbuf = pbuf = None
    if totals == "atomic":
        sbuf = torch.full((B * Cout * 2 + TAIL,), PATTERN, dtype=torch.int64, device="cuda")
        sbuf[:B * Cout * 2] = 0
    elif totals == "part":
        assert parts > 0, f"{name} has no partial form"
        pbuf = torch.full((B * parts * Cout * 2 + TAIL,), PATTERN, dtype=torch.int64, device="cuda")
    op = _conv_op(f, variant, out.data_ptr(), sbuf.data_ptr() if sbuf is not None else None)
    if not f.get("bias", 1):
        op.bias = None
    if pbuf is not None:
        op.stats_part, op.stats_parts = pbuf.data_ptr(), parts
    rc = L.lib().use_op_conv(C.byref(op), _stream())
    torch.cuda.synchronize()
    assert rc == 0, L.lib().use_last_error()
    assert bool((obuf[-TAIL:].float() == SENTINEL).all()), "write past the end of out"
    stats = part = None
    if sbuf is not None:
        assert bool((sbuf[-TAIL:] == PATTERN).all()), "write past the end of stats"
        stats = sbuf[:B * Cout * 2].view(B, Cout, 2).cpu()
    if pbuf is not None:
        assert bool((pbuf[-TAIL:] == PATTERN).all()), "write past the end of stats_part"
        part = pbuf[:B * parts * Cout * 2].view(B, parts, Cout, 2).cpu()
        assert not bool((part == PATTERN).any()), "an (item, part, channel) entry of stats_part was not written"
    return out.cpu(), stats, part, name, parts


def _in_case(c, seed):
    """Input-convolution case -> (case data for _conv_op, CPU data with the reference)."""
    d = _in_data(c, seed)
    B, H, W, C0, Cout, odt = c["B"], c["H"], c["W"], c["C0"], c["Cout"], c["odt"]
    f = dict(B=B, H=H, W=W, C0=C0, C1=0, Cout=Cout, XC0=0, XC1=0, ntaps=9, act=0, dt=0, odt=odt, gn=None, scale=d["scale"],
             d_src0=d["x"].float().cuda().contiguous(), d_coef=None, d_temb=None, temb_bstride=0, d_res=None, d_pyr=None,
             h_w=np.ascontiguousarray(d["w"].numpy()), bias=c.get("bias", 1),
             h_bias=np.ascontiguousarray(d["bias"].numpy()) if d["bias"] is not None else np.zeros(Cout, np.float32))
    return f, d


def _check_in(c, f, d, out, stats, name, parts, tpw=1, tag=""):
    """Output against the float64 reference, totals against the float64 sums of the stored output; prints and asserts the ratios."""
    got = out.double()
    assert bool(torch.isfinite(got).all()), "NaN / Inf in the output"
    ratio, pos = _worst(got, d["ref"], _in_bound(d, c["odt"], name, c["C0"]))
    line = (f"[in] {name:13s} fp32->{DT_NAME[c['odt']]} B{c['B']} {c['H']}x{c['W']} C0 {c['C0']} Cout {c['Cout']} bias {c.get('bias', 1)} "
            f"scale {d['scale']:.2g}{tag} | err/bound {ratio:.3f} at {pos}")
    st = None
    if stats is not None:
        n_ser, n_sq = _n_ser(name, c["odt"], tpw)
        st = _totals_ratio(stats, out, n_ser, n_sq, parts)
        line += f" | totals/bound {st:.3f} (n_ser {n_ser}, {parts} parts)"
    print(line)
    assert ratio < 1.0, (ratio, pos)
    assert st is None or st < 1.0, st
    return ratio, st


IN_CASES = [
    # conv_in_kernel<float>: one tile; ragged both ways with the channel mask; a second 128-channel block
    dict(H=8, W=16, Cout=128, odt=0, bias=1, totals="atomic", kern="conv_in"),
    dict(H=19, W=37, Cout=96, odt=0, bias=0, totals="atomic", scale=0.7, kern="conv_in"),
    dict(H=16, W=32, Cout=256, odt=0, bias=1, totals=None, kern="conv_in"),
    dict(H=16, W=32, Cout=256, odt=0, bias=0, totals="atomic", scale=0.7, kern="conv_in"),
    # conv_in_kernel<bf16 / f16>: Cout 32 (cout_pad 32: no split copy)
    dict(H=19, W=37, Cout=32, odt=1, bias=1, totals="atomic", kern="conv_in"),
    dict(H=19, W=37, Cout=32, odt=2, bias=1, totals="atomic", kern="conv_in"),
]
for _odt in (1, 2):
    IN_CASES += [
        # conv_in_split_kernel: FULL; masked (ragged tiles, Cout 96 and 128); one tile
        dict(H=16, W=32, Cout=128, odt=_odt, bias=1, totals="atomic", kern="conv_in_split"),
        dict(H=19, W=37, Cout=96, odt=_odt, bias=0, totals="part", kern="conv_in_split"),
        dict(H=19, W=37, Cout=128, odt=_odt, bias=1, totals="atomic", scale=0.7, kern="conv_in_split"),
        dict(H=8, W=16, Cout=128, odt=_odt, bias=1, totals=None, kern="conv_in_split"),
    ]
for _odt in (0, 1, 2):                                    # the 6 + 2 input of condition="both" on the generic kernel
    IN_CASES.append(dict(H=19, W=37, Cout=96, odt=_odt, bias=1, totals="atomic", C0=8, kern="conv_generic"))
    IN_CASES.append(dict(H=16, W=32, Cout=128, odt=_odt, bias=0, totals=None, C0=8, scale=0.7, kern="conv_generic"))


def _in_id(c):
    return (f"{c['kern']}-{DT_NAME[c['odt']]}-{c['H']}x{c['W']}x{c['Cout']}-C{c.get('C0', 4)}" + ("" if c["bias"] else "-nobias") +
            (f"-{c['totals']}" if c["totals"] else "") + (f"-scale{c['scale']}" if "scale" in c else ""))


@pytest.mark.gpu
@pytest.mark.parametrize("c", IN_CASES, ids=[_in_id(c) for c in IN_CASES])
def test_input_convolution_matches_float64_reference(c):
    c = {"B": 2, "C0": 4, **c}
    f, d = _in_case(c, seed=c["H"] * 1000 + c["W"] * 10 + c["Cout"] + c["odt"])
    out, stats, part, name, parts = _launch(f, 0, c["totals"])
    assert name == c["kern"], f"the dispatcher picks {name}, not {c['kern']}"
    tpw = 1                                              # (conv_in_wgs 256: a workgroup per tile on these maps)
    ntiles = _tiles(c["H"], c["W"])[0] * _tiles(c["H"], c["W"])[1]
    if part is not None:
        assert parts == ntiles
        stats = part.sum(1)
    _check_in(c, f, d, out, stats, name, ntiles, tpw)
    out1, stats1, part1, _, _ = _launch(f, 1, c["totals"])              # variant 1 reaches the same kernel
    assert torch.equal(out1, out)
    if stats1 is not None:
        assert torch.equal(stats1, stats)
    if part1 is not None:
        assert torch.equal(part1, part)


@pytest.mark.gpu
@pytest.mark.parametrize("odt", [1, 2])
def test_input_convolution_walks_and_partial_totals(odt):
    """conv_in_split_kernel on the 9-tile map under conv_in_wgs = 256 / 4 / 2 / 1 (walks of 1; 3; 5 and 4, the last one short; all 9):
    each walk held to the float64 bound with atomic and with partial totals, `out` bit-identical across walks and forms, the partials
    summed in int64 equal to the atomic totals of the same walk bit for bit."""
    c = dict(B=2, H=24, W=48, C0=4, Cout=128, odt=odt, bias=1)
    f, d = _in_case(c, seed=24 * 100 + 48 + 128)
    outs, worst = {}, 0.0
    try:
        for wgs, tpw, nwg in ((256, 1, 9), (4, 3, 3), (2, 5, 2), (1, 9, 1)):
            _set_option("conv_in_wgs", wgs)
            out_n, _, _, name, _ = _launch(f, 0, None)
            out_a, stats, _, _, parts = _launch(f, 0, "atomic")
            out_p, _, part, _, _ = _launch(f, 0, "part")
            assert name == "conv_in_split" and parts == nwg, (name, parts, nwg)
            assert torch.equal(out_a, out_n) and torch.equal(out_p, out_n), "out depends on the form of the totals"
            assert torch.equal(part.sum(1), stats), "the partial totals do not sum to the atomic totals"
            r, _ = _check_in(c, f, d, out_p, stats, name, parts, tpw, tag=f" conv_in_wgs {wgs} (walks of {tpw})")
            worst = max(worst, r)
            outs[wgs] = out_n
    finally:
        _set_option("conv_in_wgs", 256)
    for wgs in (4, 2, 1):
        assert torch.equal(outs[wgs], outs[256]), f"out depends on the walk length (conv_in_wgs {wgs})"


# Pyramid head.  Profiles: GroupNorm as a coefficient array or finalised in the kernel, SiLU or none, with / without the fp32 residual
# and the bias; one / two 128-channel blocks; ragged bottom and right; Cout 2; B = 3 (per_item = pyr_ws / B)
PYR_CASES = [
    dict(B=2, H=40, W=48, C0=128, gn="coef", act=1, res=1, bias=1),
    dict(B=2, H=43, W=37, C0=128, gn="st", act=1, res=0, bias=1),
    dict(B=2, H=43, W=37, C0=256, gn="coef", act=1, res=1, bias=0),
    dict(B=2, H=40, W=48, C0=128, gn="coef", act=0, res=1, bias=1),
    dict(B=2, H=43, W=37, C0=128, gn="coef", act=1, res=1, bias=1, Cout=2),
    dict(B=3, H=40, W=48, C0=128, gn="coef", act=1, res=1, bias=0),
]


def _pyr_id(c):
    return (f"B{c['B']}-{c['H']}x{c['W']}-C{c['C0']}-O{c.get('Cout', 4)}-{c['gn']}-act{c['act']}" + ("-res" if c["res"] else "") +
            ("" if c["bias"] else "-nobias"))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("c", PYR_CASES, ids=[_pyr_id(c) for c in PYR_CASES])
def test_pyramid_head_matches_float64_reference_in_every_form(c, dt):
    """pyr_conv_kernel (pyr_ws 0) and pyr_conv_ws_kernel with 256 workgroups per launch (1: walks of one tile), 2 (one workgroup walks a
    whole item: the halo rolls down every strip and restarts at every strip top) and 8 (walks that begin mid-strip, an odd unit count
    with its padding unit): each form on its own against the float64 bound, and all of them bit-identical."""
    Cout = c.get("Cout", 4)
    case = dict(dt=dt, odt=0, B=c["B"], H=c["H"], W=c["W"], C0=c["C0"], Cout=Cout, gn=c["gn"], act=c["act"], res=c["res"])
    f, ref, S, _ = _make_case(case, seed=c["H"] * 977 + c["W"] * 31 + c["C0"] + dt + Cout)
    f["bias"] = c["bias"]
    if not c["bias"]:                                    # (_make_case's reference carries its bias: the case without it, exactly)
        bias = torch.from_numpy(f["h_bias"]).double()
        ref, S = ref - bias * f["scale"], S - bias.abs()
    bound = _bound(ref, S, dt, 0, f["scale"], 9 * c["C0"])
    outs = {}
    try:
        for ws in (0, 1, 2, 8):
            _set_option("pyr_ws", ws)
            out, _, _, name, _ = _launch(f, 0, None)
            assert name == ("pyr_conv_ws" if ws else "pyr_conv"), (ws, name)
            got = out.double()
            assert bool(torch.isfinite(got).all())
            ratio, pos = _worst(got, ref, bound)
            print(f"[pyr] {name:11s} pyr_ws {ws} {DT_NAME[dt]}->fp32 {_pyr_id(c)} | err/bound {ratio:.3f} at {pos}")
            assert ratio < 1.0, (ws, ratio, pos)
            outs[ws] = out
    finally:
        _set_option("pyr_ws", 1)
    for ws in (1, 2, 8):
        assert torch.equal(outs[ws], outs[0]), f"pyr_ws {ws} differs from pyr_conv_kernel"


WIDE_PART = [(4, 0, "CONV0"), (4, 1, "CONV1_RES"), (5, 1, "CONV0"), (5, 2, "CONV1_RES")]


@pytest.mark.gpu
@pytest.mark.parametrize("kern,dt,prof", WIDE_PART, ids=[f"conv_v{k}-{DT_NAME[dt]}-{p}" for k, dt, p in WIDE_PART])
def test_wide_conv_partial_totals_are_the_atomic_totals(kern, dt, prof):
    """conv_v4 / conv_v5 at 48 x 64 (6 tiles per item) with stats_part: `out` bit-identical to the atomic form, the partials summed in
    int64 equal to its totals bit for bit and inside `_check_stats`'s bound; and use_op_gn_finalize_parts on the partials gives the
    coefficients of use_op_gn_finalize on the totals, bit for bit."""
    L = _lib()
    c = dict(kern=kern, dt=dt, B=2, H=48, W=64, C0=64 if prof == "CONV0" else 128, Cout=128, **(CONV0 if prof == "CONV0" else CONV1_RES))
    f, ref, S, _ = _make_case(c, seed=4864 + kern * 10 + dt)
    try:
        for k, v in _dispatch_options(c).items():
            _set_option(k, v)
        out_a, stats, _, name, parts = _launch(f, 0, "atomic")
        out_p, _, part, _, _ = _launch(f, 0, "part")
    finally:
        _set_option("conv_sk_max_px", 16 * 20); _set_option("conv_v4_min_blocks", 80); _set_option("conv_v5", 1)
    assert name == f"conv_v{kern}" and parts == 6, (name, parts)
    assert torch.equal(out_p, out_a), "out depends on the form of the totals"
    assert torch.equal(part.sum(1), stats), "the partial totals do not sum to the atomic totals"
    K = (f["C0"] + f["C1"]) * 9
    ratio, pos = _worst(out_p.double(), ref, _bound(ref, S, dt, dt, f["scale"], K))
    st = _check_stats(part.sum(1), out_p, dt, name)
    print(f"[part] {name} {DT_NAME[dt]} {prof} 48x64: err/bound {ratio:.3f} at {pos}, totals/bound {st:.3f}, {parts} parts")
    assert ratio < 1.0
    g = torch.Generator().manual_seed(5)
    gamma, beta = (0.5 + torch.rand(128, generator=g)).cuda(), (torch.randn(128, generator=g) * 0.3).cuda()
    d_part, d_st = part.cuda().contiguous(), stats.cuda().contiguous()
    coef_p, coef_t = torch.full((2, 128, 2), 7.0, device="cuda"), torch.full((2, 128, 2), 9.0, device="cuda")
    vp = lambda t: C.c_void_p(t.data_ptr())
    L.check(L.lib().use_op_gn_finalize_parts(None, vp(d_part), parts, 128, None, None, 0, 0, vp(gamma), vp(beta), 32, 48 * 64, GN_EPS, vp(coef_p), 2,
                                             _stream()), "use_op_gn_finalize_parts")
    L.check(L.lib().use_op_gn_finalize(vp(d_st), 128, None, 0, vp(gamma), vp(beta), 32, 48 * 64, GN_EPS, vp(coef_t), 2, _stream()), "use_op_gn_finalize")
    torch.cuda.synchronize()
    assert torch.equal(coef_p, coef_t)


# use_op_gn_finalize_parts: (C0, nt0, C1, nt1, groups); nt 0 = that source as totals.  nt 300 wraps the 256-thread loop; C0 12 + C1 20 in
# 4 groups of 8: the second group straddles the sources; channels per group 1, 4 and 8
FIN_CASES = [(32, 1, 0, 0, 32), (32, 6, 0, 0, 8), (32, 300, 0, 0, 4), (12, 6, 20, 0, 4), (12, 0, 20, 300, 4), (12, 300, 20, 6, 8), (16, 1, 16, 0, 32)]


@pytest.mark.gpu
@pytest.mark.parametrize("C0,nt0,C1,nt1,groups", FIN_CASES, ids=[f"C{a}p{b}+C{c}p{d}-g{e}" for a, b, c, d, e in FIN_CASES])
def test_finalize_from_partials_matches_finalize_from_totals(C0, nt0, C1, nt1, groups):
    """A stored map with a large mean ([B, 32 x 40, C0 + C1], |mean| / std up to ~30) cut into nt slices of pixels whose fixed-point sums
    are the partial totals: the coefficients from the partials are those of use_op_gn_finalize on the int64-summed totals bit for bit,
    and within the stated bound of float64 GroupNorm of the map.  (The totals here are roundings of float64 sums, so the measured ratio
    is far below 1: the bound is sized for the kernels' fp32 accumulation.  What this test is about is the bit identity.)"""
    L = _lib()
    B, HW, Cc = 2, 32 * 40, C0 + C1
    g = torch.Generator().manual_seed(C0 * 7 + nt0 + nt1 * 3 + groups)
    y = (torch.rand(B, HW, Cc, generator=g, dtype=torch.float64) * 2 - 1) * 0.5 + torch.randn(Cc, generator=g, dtype=torch.float64) * 3 + \
        torch.arange(B, dtype=torch.float64)[:, None, None]
    y = y.float().double()
    gamma, beta = 0.5 + torch.rand(Cc, generator=g), torch.randn(Cc, generator=g) * 0.3

    def fixed(v, nt):                                    # [B, HW, C] -> [B, nt, C, 2] fixed-point sums of nt pixel slices
        cuts = np.linspace(0, HW, nt + 1).astype(int)
        return torch.stack([torch.stack([torch.round(v[:, a:b].pow(e).sum(1) * 2 ** 20) for e in (1, 2)], -1)
                            for a, b in zip(cuts[:-1], cuts[1:])], 1).long()
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    p0, p1 = fixed(y[..., :C0], max(nt0, 1)), (fixed(y[..., C0:], max(nt1, 1)) if C1 else None)
    t0, t1 = p0.sum(1).cuda().contiguous(), (p1.sum(1).cuda().contiguous() if C1 else None)
    d0 = p0.cuda().contiguous() if nt0 else None
    d1 = p1.cuda().contiguous() if nt1 else None
    d_gamma, d_beta = gamma.cuda(), beta.cuda()
    buf_p, coef_p = _guarded((B, Cc, 2), torch.float32, SENTINEL)
    coef_t = torch.full((B, Cc, 2), 9.0, device="cuda")
    L.check(L.lib().use_op_gn_finalize_parts(None if nt0 else vp(t0), vp(d0), nt0, C0, None if (nt1 or not C1) else vp(t1), vp(d1), nt1, C1,
                                             vp(d_gamma), vp(d_beta), groups, HW, GN_EPS, vp(coef_p), B, _stream()), "use_op_gn_finalize_parts")
    L.check(L.lib().use_op_gn_finalize(vp(t0), C0, vp(t1), C1, vp(d_gamma), vp(d_beta), groups, HW, GN_EPS, vp(coef_t), B, _stream()), "use_op_gn_finalize")
    torch.cuda.synchronize()
    assert bool((buf_p[-TAIL:] == SENTINEL).all()), "write past the end of coef"
    assert torch.equal(coef_p, coef_t), "coefficients from partials differ from those of the summed totals"
    want = gn_coef_reference(y.reshape(B, 32, 40, Cc), gamma, beta, groups)
    yg = y.permute(0, 2, 1).reshape(B, groups, -1)
    mean, std = yg.mean(-1), yg.std(-1, unbiased=False)
    ra, rb = _finalize_ratios(coef_p.double().cpu(), want, mean, std, beta, HW, Cc // groups)
    print(f"[fin] C {C0}+{C1} partials {nt0}/{nt1} groups {groups} (|mean|/std up to {float((mean.abs() / std).max()):.0f}): a err/bound {ra:.3f}, b {rb:.3f}")
    assert ra < 1.0 and rb < 1.0


@pytest.mark.gpu
def test_refusals_launch_nothing_and_leave_the_library_usable():
    L = _lib()
    c = dict(B=2, H=24, W=48, C0=4, Cout=128, odt=1, bias=1)
    f, d = _in_case(c, seed=3)
    name, parts = _choice(f, True)
    assert (name, parts) == ("conv_in_split", 9)
    out = torch.full((2, 24, 48, 128), 3.0, dtype=torch.bfloat16, device="cuda")
    junk = torch.full((2 * 9 * 128 * 2 + 64,), PATTERN, dtype=torch.int64, device="cuda")
    x16 = torch.zeros(2, 24, 48, 32, dtype=torch.bfloat16, device="cuda")
    h_w2 = np.zeros((128, 32), np.float32)

    def attempt(what, expect, **kw):
        op = _conv_op(f, kw.pop("variant", 0), out.data_ptr(), None)
        for k, v in kw.items():
            setattr(op, k, v)
        rc = L.lib().use_op_conv(C.byref(op), _stream())
        msg = L.lib().use_last_error().decode()
        torch.cuda.synchronize()
        print(f"[refuse] {what}: rc {rc} '{msg}'")
        assert rc == INVALID and expect in msg, (what, rc, msg)
        assert bool((out == 3.0).all()) and bool((junk == PATTERN).all()), what
    attempt("stats_part with a wrong stats_parts", "stats_parts", stats_part=junk.data_ptr(), stats_parts=8)
    attempt("stats_part without a count", "go together", stats_part=junk.data_ptr())
    attempt("stats_part together with stats", "two forms", stats_part=junk.data_ptr(), stats_parts=9, stats=junk.data_ptr())
    attempt("C0 = 4 with dtype bf16", "multiples of 32", dtype=1)
    attempt("C0 = 4 with a shortcut", "multiples of 32", XC0=32, x0=x16.data_ptr(), w2=h_w2.ctypes.data)
    attempt("C0 = 4 with SiLU", "input convolution", act=1)
    attempt("the input convolution on conv_v4", "cannot run", variant=4)
    # a kernel that only knows atomics: conv_in_kernel (fp32 output), and a forced conv_v2
    f32, _ = _in_case(dict(c, odt=0), seed=3)
    out32 = torch.full((2, 24, 48, 128), 3.0, device="cuda")
    op = _conv_op(f32, 0, out32.data_ptr(), None)
    op.stats_part, op.stats_parts = junk.data_ptr(), 9
    rc = L.lib().use_op_conv(C.byref(op), _stream())
    msg = L.lib().use_last_error().decode()
    print(f"[refuse] stats_part on conv_in: rc {rc} '{msg}'")
    assert rc == INVALID and "only knows atomic" in msg and bool((out32 == 3.0).all()) and bool((junk == PATTERN).all())
    fw, _, _, _ = _make_case(dict(dt=1, B=1, H=16, W=32, C0=64, Cout=128), seed=1)
    outw = torch.full((1, 16, 32, 128), 3.0, dtype=torch.bfloat16, device="cuda")
    op = _conv_op(fw, 2, outw.data_ptr(), None)
    op.stats_part, op.stats_parts = junk.data_ptr(), 1
    rc = L.lib().use_op_conv(C.byref(op), _stream())
    msg = L.lib().use_last_error().decode()
    print(f"[refuse] stats_part on a forced conv_v2: rc {rc} '{msg}'")
    assert rc == INVALID and "only knows atomic" in msg and bool((outw == 3.0).all()) and bool((junk == PATTERN).all())
    # use_op_gn_finalize_parts: groups not dividing C0 + C1; both forms for a source; neither
    coef = torch.full((2, 32, 2), 3.0, device="cuda")
    gb = torch.ones(32, device="cuda")
    vp = lambda t: C.c_void_p(t.data_ptr())
    for what, args in (("groups not dividing C0 + C1", (None, vp(junk), 2, 12, vp(junk), None, 0, 20, vp(gb), vp(gb), 5)),
                       ("both forms for source 0", (vp(junk), vp(junk), 2, 32, None, None, 0, 0, vp(gb), vp(gb), 8)),
                       ("neither form for source 1", (vp(junk), None, 0, 12, None, None, 0, 20, vp(gb), vp(gb), 4))):
        rc = L.lib().use_op_gn_finalize_parts(*args, 1280, GN_EPS, vp(coef), 2, _stream())
        msg = L.lib().use_last_error().decode()
        torch.cuda.synchronize()
        print(f"[refuse] use_op_gn_finalize_parts, {what}: rc {rc} '{msg}'")
        assert rc == INVALID and "use_op_gn_finalize_parts" in msg and bool((coef == 3.0).all()), what
    # the library is still usable: the same op, accepted
    out_ok, _, part, _, _ = _launch(f, 0, "part")
    ratio, _ = _worst(out_ok.double(), d["ref"], _in_bound(d, 1, "conv_in_split", 4))
    assert ratio < 1.0 and part.shape == (2, 9, 128, 2)
