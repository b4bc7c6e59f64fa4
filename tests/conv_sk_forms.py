"""Host mirror of what `launch_conv_sk` (csrc/use_conv_sk.hip) picks for a convolution, and a float64 emulation of the decomposition
`conv_sk_kernel` then runs.  Used by tests/test_hip_conv_kernels.py (each conv_sk case asserts the form it was written to reach before it
launches) and tests/test_conv_sk_forms_host.py (coverage of the forms, the mirror against the tile rule, mutation controls).

The launcher does not run one kernel.  From the operands it picks
  tile        `sk_tile(H, W, pad)`: TH x TW <= SK_MT pixels, halo <= SK_HPMAX pixels, fewest tiles, then the smallest halo
  tile width  wide = Cout % 64 == 0 and tiles * B * (Cout / 32) > WIDE_WGS: 64 output channels per workgroup (NJ = 2), else 32 (NJ = 1)
  CP          channels per K pass, by (storage type, NJ): the template arguments of the six `sk_launch<...>` calls (+ the two fp32-out heads)
and the kernel walks each of its four K sources (src0, src1 under all taps; x0, x1 under the centre tap) in passes of CP channels.  A pass
of pc channels has cpu_ = pc / 32 chunks and taps * cpu_ units (tap, chunk); wave w of 8 takes units w, w + 8, ..., stepped without
divisions by d_tap = 8 / cpu_, d_chunk = 8 - d_tap * cpu_ with one carry.  In a second pass (c_loc > 0) or a second source (cg0 > 0) the
weight address, the GroupNorm table offset (c_glob = cg0 + c_loc) and the halo load offset (c_loc) stop being zero.

Every constant is read back from the source text by regular expression (`_read_source`); a pattern that no longer matches raises, so a
changed launcher breaks the mirror loudly instead of leaving the cases on a form the kernel no longer has.

A case is the dict of tests/test_hip_conv_kernels.py's CASES: B, H, W, C0, [C1], Cout, [XC0, XC1], [ntaps], dt, [odt]."""
import functools
import math
import os
import re

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "universal_speech_enhancement_amd", "csrc")
WAVES = 8                         # a workgroup's waves split the units of a pass: `u = wave + 8 i`
_CTYPE = {"float": 0, "__bf16": 1, "_Float16": 2}


def _text(name):
    return open(os.path.join(CSRC, name)).read()


def _one(name, pattern, what):
    found = re.findall(pattern, _text(name))
    if len(found) != 1:
        raise AssertionError(f"tests/conv_sk_forms.py: {what} - the pattern {pattern!r} matches {len(found)} times in csrc/{name}; "
                             f"the launcher changed, mirror it here before trusting any conv_sk case")
    return found[0]


@functools.lru_cache(None)
def _read_source():
    """The launcher's constants as the source states them."""
    sk = "use_conv_sk.hip"
    k = dict(
        SK_MT=int(_one(sk, r"constexpr int SK_MT = (\d+);", "output pixels per workgroup")),
        SK_HPMAX=int(_one(sk, r"constexpr int SK_HPMAX = (\d+);", "halo pixels of a tile")),
        WIDE_WGS=int(_one(sk, r"const bool wide = a\.Cout % 64 == 0 && tiles \* \(a\.Cout / 32\) > (\d+);", "the tile-width rule")),
        MAX_PX=math.prod(int(v) for v in _one(sk, r"long g_sk_max_px = (\d+)L \* (\d+)L;", "largest 16-bit map")),
        MAX_PX_F32=int(_one(sk, r"std::max\(g_sk_max_px, (\d+)L\)", "largest fp32 map")),
        V2_T=int(_one("use_conv_v2.hip", r"constexpr int V2_T = (\d+);", "conv_v2's tile edge")),
    )
    tw, th = _one("use_conv_v4.hip", r"constexpr int V4_TW = (\d+), V4_TH = (\d+);", "the wide tile")
    k["V4_TW"], k["V4_TH"] = int(tw), int(th)
    _one(sk, r"const long tiles = \(long\)\(\(a\.H \+ th - 1\) / th\) \* \(\(a\.W \+ tw - 1\) / tw\) \* \(t_sk_per_image \? 1 : a\.B\);", "the workgroup count")
    _one(sk, r"const long key = tiles \* 1024 \+ halo;", "sk_tile: fewest tiles, then the smallest halo")
    _one(sk, r"const int hcap = SK_HPMAX / \(w \+ 2 \* pad\) - 2 \* pad;", "sk_tile: the halo cap of the second round")
    _one(sk, r"for \(int c_loc = 0; c_loc < Cs; c_loc \+= CP\)", "the pass loop")
    _one(sk, r"const int d_tap = 8 / cpu_, d_chunk = 8 - d_tap \* cpu_;", "the unit stepping")
    _one(sk, r"const int tap0 = wave / cpu_, chunk0 = wave - tap0 \* cpu_;", "a wave's first unit")
    for f in ("use_conv_v2.hip", "use_conv_v4.hip"):
        _one(f, r"if \(\(gridDim\.x & 7\) == 0\) tile = \(blockIdx\.x & 7\) \* \(gridDim\.x >> 3\) \+ \(blockIdx\.x >> 3\);", "the XCD re-ordering")
    # the six sk_launch<T, T, NJ, CP> calls of the same-type outputs and the two fp32-out heads
    same, head = {}, {}
    for tin, tout, nj, cp in re.findall(r"sk_launch<(\w+), (\w+), (\d), (\d+)>\(a, th, tw, s\)", _text(sk)):
        (same if tin == tout else head)[(_CTYPE[tin], int(nj))] = int(cp)
    if sorted(same) != [(0, 1), (0, 2), (1, 1), (1, 2), (2, 1), (2, 2)] or sorted(head) != [(1, 1), (2, 1)]:
        raise AssertionError(f"tests/conv_sk_forms.py: launch_conv_sk no longer has its six same-type and two head instantiations: {same} {head}")
    k["CP"], k["CP_HEAD"] = same, head
    # op_desc's slab-major rule (use_engine.cpp) and conv_v4_chunk (use_kernels.h)
    _one("use_engine.cpp", r"d\.w = true; d\.wb = ntaps == 9 && d\.cout_pad % 128 == 0 && \(C0 \+ C1\) % ck == 0;", "op_desc: the slab-major copy of w")
    _one("use_engine.cpp", r"d\.w2 = XC > 0; d\.w2b = XC > 0 && XC % ck == 0 && d\.cout_pad % 128 == 0;", "op_desc: the slab-major copy of w2")
    _one("use_engine.cpp", r"d\.cout_pad = Cout <= 32 \? 32 : \(Cout \+ 127\) / 128 \* 128;", "op_desc: cout_pad")
    f32, other = _one("use_kernels.h", r"inline int conv_v4_chunk\(int dtype\) \{ return dtype == DT_F32 \? (\d+) : (\d+); \}", "conv_v4_chunk")
    k["CK"] = {0: int(f32), 1: int(other), 2: int(other)}
    return k


def constants():
    return dict(_read_source())


def sk_tile(H, W, pad):
    """(TH, TW) as `sk_tile` picks them."""
    k = _read_source()
    best, bh, bw = -1, 1, 1
    for capped in (False, True):                     # the second round only when the first finds nothing (tall maps of 1 or 2 columns)
        if best >= 0:
            break
        for w in range(1, min(W, k["SK_MT"]) + 1):
            hmax = min(k["SK_MT"] // w, H)
            if capped:
                hmax = min(hmax, k["SK_HPMAX"] // (w + 2 * pad) - 2 * pad)
                if hmax < 1:
                    continue
            ny = (H + hmax - 1) // hmax
            h = (H + ny - 1) // ny
            halo = (h + 2 * pad) * (w + 2 * pad)
            if halo > k["SK_HPMAX"]:
                continue
            key = ny * ((W + w - 1) // w) * 1024 + halo
            if best < 0 or key < best:
                best, bh, bw = key, h, w
    return bh, bw


def _dims(c):
    return (c["B"], c["H"], c["W"], c["C0"], c.get("C1", 0), c.get("XC0", 0), c.get("XC1", 0), c["Cout"], c.get("ntaps", 9), c["dt"],
            c.get("odt", c["dt"]))


def sk_eligible(c):
    """`conv_sk_eligible` for a case of the op surface (weights always present)."""
    k = _read_source()
    B, H, W, C0, C1, XC0, XC1, Cout, ntaps, dt, odt = _dims(c)
    Ctot, XC = C0 + C1, XC0 + XC1
    full = dt == odt and Cout % 32 == 0 and Cout >= 32
    head = odt == 0 and Cout <= 8 and not c.get("pyr") and not c.get("stats")
    max_px = max(k["MAX_PX"], k["MAX_PX_F32"]) if dt == 0 else k["MAX_PX"]
    return (H * W <= max_px and ntaps in (1, 9) and (full or head) and Ctot % 32 == 0 and C0 % 32 == 0 and XC % 32 == 0 and XC0 % 32 == 0 and
            32 <= Ctot <= 1024)


def sk_passes(c, CP):
    """[(source index, cg0, c_loc, pc)] in the kernel's order."""
    B, H, W, C0, C1, XC0, XC1, Cout, ntaps, dt, odt = _dims(c)
    out = []
    for si, (Cs, cg0) in enumerate(((C0, 0), (C1, C0), (XC0, 0), (XC1, XC0))):
        for c_loc in range(0, Cs, CP):
            out.append((si, cg0, c_loc, min(Cs - c_loc, CP)))
    return out


def sk_form(c):
    """(NJ, CP, tiles, workgroups, per_source_passes): what `launch_conv_sk` launches for the case.  workgroups = tiles * B * (Cout // 32)
    is the figure the tile-width rule compares; per_source_passes lists cpu_ per pass, one list per non-empty source in source order."""
    k = _read_source()
    B, H, W, C0, C1, XC0, XC1, Cout, ntaps, dt, odt = _dims(c)
    th, tw = sk_tile(H, W, 1 if ntaps == 9 else 0)
    tiles = ((H + th - 1) // th) * ((W + tw - 1) // tw)
    wgs = tiles * B * (Cout // 32)
    if dt != odt:
        NJ, CP = 1, k["CP_HEAD"][(dt, 1)]
    else:
        NJ = 2 if Cout % 64 == 0 and wgs > k["WIDE_WGS"] else 1
        CP = k["CP"][(dt, NJ)]
    per_source = [[] for _ in range(4)]
    for si, cg0, c_loc, pc in sk_passes(c, CP):
        per_source[si].append(pc // 32)
    return NJ, CP, tiles, wgs, [p for p in per_source if p]


def weight_branch(c):
    """('slab' | 'row', 'slab' | 'row' | None): the weight-addressing branch of the main and of the shortcut weights (`op_desc`: a slab-major
    copy exists iff ntaps == 9, cout_pad % 128 == 0 and Ctot % ck == 0; for w2 iff XC % ck == 0 and cout_pad % 128 == 0)."""
    k = _read_source()
    B, H, W, C0, C1, XC0, XC1, Cout, ntaps, dt, odt = _dims(c)
    cout_pad = 32 if Cout <= 32 else (Cout + 127) // 128 * 128
    ck, XC = k["CK"][dt], XC0 + XC1
    wb = ntaps == 9 and cout_pad % 128 == 0 and (C0 + C1) % ck == 0
    w2b = XC > 0 and XC % ck == 0 and cout_pad % 128 == 0
    return "slab" if wb else "row", (None if XC == 0 else "slab" if w2b else "row")


def wide_tiles(H, W):
    """gridDim.x of conv_wide_kernel (conv_v4 / conv_v5)."""
    k = _read_source()
    return ((H + k["V4_TH"] - 1) // k["V4_TH"]) * ((W + k["V4_TW"] - 1) // k["V4_TW"])


def v2_tiles(H, W):
    """gridDim.x of conv_v2_kernel."""
    t = _read_source()["V2_T"]
    return ((H + t - 1) // t) * ((W + t - 1) // t)


def xcd_tile(bid, n):
    """The tile workgroup `bid` of `n` takes in conv_wide_kernel / conv_v2_kernel."""
    return (bid & 7) * (n >> 3) + (bid >> 3) if n & 7 == 0 else bid


# ---------------------------------------------------------------------------------------------------------------------------------
# the unit walk and the float64 emulation of the decomposition
# ---------------------------------------------------------------------------------------------------------------------------------
def unit_walk(wtaps, cpu_, skip=None, repeat_last=None):
    """Visit counts [wtaps][cpu_] of the pass's (tap, chunk) units under the kernel's stepping: wave w starts at (w / cpu_, w % cpu_) and
    advances by (d_tap, d_chunk) with one carry while w + 8 i < nunits.  skip = (wave, i): that unit is left out; repeat_last = wave: the
    wave's last unit is done under the tap of the one before it again (the tap step lost)."""
    nunits = wtaps * cpu_
    d_tap = WAVES // cpu_
    d_chunk = WAVES - d_tap * cpu_
    umax = (nunits + WAVES - 1) // WAVES
    m = [[0] * cpu_ for _ in range(wtaps)]
    for wave in range(WAVES):
        tap, chunk = wave // cpu_, wave - (wave // cpu_) * cpu_
        n_w = len(range(wave, nunits, WAVES))
        prev_tap = None
        for i in range(umax):
            if wave + 8 * i < nunits:
                t = tap
                if repeat_last == wave and i == n_w - 1 and prev_tap is not None:
                    t = prev_tap
                if skip != (wave, i):
                    m[t][chunk] += 1
                prev_tap = tap
            tap += d_tap; chunk += d_chunk
            if chunk >= cpu_:
                chunk -= cpu_; tap += 1
    return m


def _silu(x):
    return x / (1.0 + torch.exp(-x))


def emulate(c, ops, mutant=None):
    """float64 emulation of conv_sk_kernel's decomposition on operands `ops`, rounded to the output type: the per-source pass loop with its
    three offsets (halo channels from c_loc, GroupNorm table from c_glob, weights from c_glob), the unit walk (each pass's weights times the
    visit counts of `unit_walk`), the channel tiles j of a workgroup, the epilogue in conv_reference's order, the store rounding.
    ops: src [B,H,W,Ctot], coef [B,Ctot,2] | None, act, w [Cout,Ctot,3,3] | [Cout,Ctot], xs, w2, bias, temb [B,Cout], res, scale, pyr, w4, b4
    (float64 tensors, the values as stored; weights rounded here like conv_reference rounds them); q(t, dt) the storage rounding.
    mutant: None or one of 'drop_pass2', 'halo_no_cloc', 'weights_no_cloc', 'table_no_cglob', 'j1_as_j0', 'skip_unit', 'repeat_tap'."""
    q, dt, odt = ops["q"], c["dt"], c.get("odt", c["dt"])
    NJ, CP, _, _, _ = sk_form(c)
    B, H, W, C0, C1, XC0, XC1, Cout, ntaps, _, _ = _dims(c)
    hit = False                                      # the mutant met the structure it needs (a second pass, NJ = 2, ...)
    y = torch.zeros(B, Cout, H, W, dtype=torch.float64)
    w = q(ops["w"].double(), dt)
    w = w if w.dim() == 4 else w[:, :, None, None]
    w2 = q(ops["w2"].double(), dt)[:, :, None, None] if ops.get("w2") is not None else None
    srcs = (ops["src"][..., :C0], ops["src"][..., C0:], None if w2 is None else ops["xs"][..., :XC0], None if w2 is None else ops["xs"][..., XC0:])
    seen = {}                                        # passes met so far per segment (main / shortcut)
    for si, cg0, c_loc, pc in sk_passes(c, CP):
        seg1 = si >= 2
        npass = seen.get(si, 0); seen[si] = npass + 1
        second = npass == 1                          # the second pass of a source
        if mutant == "drop_pass2" and second:
            hit = True
            continue
        c_glob = cg0 + c_loc
        ha = 0 if (mutant == "halo_no_cloc" and second) else c_loc
        wa = cg0 if (mutant == "weights_no_cloc" and second) else c_glob
        ta = 0 if (mutant == "table_no_cglob" and c_glob > 0 and not seg1 and ops["coef"] is not None) else c_glob
        hit |= (ha != c_loc) or (wa != c_glob) or (ta != c_glob)
        a = srcs[si][..., ha:ha + pc].double()
        if not seg1:
            if ops["coef"] is not None:
                cf = ops["coef"][:, ta:ta + pc].double()
                a = a * cf[:, None, None, :, 0] + cf[:, None, None, :, 1]
            if ops["act"]:
                a = _silu(a)
            a = q(a, dt)
        wfull, wtaps = (w2, 1) if seg1 else (w, ntaps)
        wp = wfull[:, wa:wa + pc].clone()
        cpu_ = pc // 32
        skip = rep = None
        if mutant == "skip_unit" and cpu_ & (cpu_ - 1) and not seg1:
            skip = (5, 1)                            # wave 5's second unit
        if mutant == "repeat_tap" and not seg1:
            rep = 3                                  # wave 3
        m = torch.tensor(unit_walk(wtaps, cpu_, skip, rep), dtype=torch.float64)          # [wtaps][cpu_]
        hit |= bool((m != 1).any())
        kk = wp.shape[-1]
        wp = wp * m.reshape(kk, kk, cpu_).permute(2, 0, 1).repeat_interleave(32, 0)[None]
        if mutant == "j1_as_j0" and NJ == 2:
            hit = True
            wp = wp.reshape(Cout // 64, 2, 32, pc, kk, kk)
            wp = torch.stack([wp[:, 0], wp[:, 0]], 1).reshape(Cout, pc, kk, kk)
        y += F.conv2d(a.permute(0, 3, 1, 2), wp, padding=kk // 2)
    y = y.permute(0, 2, 3, 1)
    for v in (ops.get("bias"), None if ops.get("temb") is None else ops["temb"][:, None, None, :]):
        if v is not None:
            y = y + v.double()
    if ops.get("res") is not None:
        y = y + ops["res"].double()
    y = y * ops["scale"]
    if ops.get("pyr") is not None:
        y = y + ops["pyr"].double() @ ops["w4"].double().T + ops["b4"].double()
    return q(y, odt), hit


def transpose_tiles(out, th, tw):
    """The XCD-case defect: every workgroup computes the tile of the transposed tile list (tile t of an ny x nx grid read as nx x ny) and
    stores it where tile t belongs.  out [B,H,W,C]: the correct output; returns the defective one (ragged tiles: the part that fits)."""
    B, H, W, Cc = out.shape
    ny, nx = (H + th - 1) // th, (W + tw - 1) // tw
    bad = out.clone()
    for t in range(ny * nx):
        r, cidx = divmod(t, nx)
        s = (t % ny) * nx + t // ny                  # the tile the transposed list names
        sr, sc = divmod(s, nx)
        hh = min(th, H - r * th, H - sr * th); ww = min(tw, W - cidx * tw, W - sc * tw)
        bad[:, r * th:r * th + hh, cidx * tw:cidx * tw + ww] = out[:, sr * th:sr * th + hh, sc * tw:sc * tw + ww]
    return bad
