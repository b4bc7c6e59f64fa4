"""The GEMM form of the attention core (launch_attention_gemm, csrc/use_kernels.hip: what Fwd::attention runs above 512 tokens, the
bottleneck of the refine generator) through use_op_attention_gemm, stage by stage and composed, against float64.  Its 2 + 2 B launches:
vt = v^T; per item the scores as a 1x1 convolution of q whose weights are the item's keys (out_scale C^-0.5, no bias); softmax_rows in
place over all B N rows; per item a 1x1 convolution of the probabilities whose weights are the item's vt.  Scores and probabilities are
stored in the activation type between the launches.  No reference and no per-kernel bound is stated here: conv_reference / _bound come from
tests/test_hip_conv_kernels.py, attention_reference / softmax_rows_reference / _ratio / _attn_data from tests/test_hip_forward_kernels.py.

Cases (CASES below): the smallest eligible shape with three items, ragged tile rows (5 x 128, 8 x 80), the seam of the fp32 dispatch (P.V
with K = 1024, the last K conv_sk accepts, and K = 1152 on conv_kernel), C = 384 (a multiple of 128, not of 256).  The kernel of either
GEMM is asserted per type through use_conv_choice (host only, also without a GPU): fp32 storage runs the scores on conv_sk (N <= 4096
pixels, K = C <= 1024) and P.V on conv_sk up to K = N = 1024, on conv_kernel ("conv_generic") above; the 16-bit modes run conv_kernel
throughout (conv_sk takes 16-bit maps up to 320 pixels).

Per stage, each against the operands as stored (read back from the workspace: probabilities at offset 0, vt behind them):
  vt       bit-equal to the transpose of the stored v;
  scores   the score GEMM of every item again through use_op_conv with the same arguments (the op runs the softmax in place, so the
           scores themselves are gone): against conv_reference(q, w = k, scale = C^-0.5) with _bound(.., K = C); use_op_softmax_rows over
           all B N rows of them must give the stored probabilities bit for bit, which ties them to what the op computed;
  softmax  the stored probabilities against softmax_rows_reference of those stored scores, u_out p + that function's bound, all B N rows,
           + 2^-126 absolute: in a "peaked" row the scores spread over more than 87 = -ln(2^-126), so a probability lies below the
           smallest normal fp32 number, where the kernel's fp32 exp flushes or rounds to a subnormal and the bf16 store does the same
           (the 5-row cases of softmax_rows_reference's own file spread over +-16 and never get there);
  P.V      the output against conv_reference(P, w = vt) with _bound(.., K = N).

Composed: out against attention_reference(q, k, v) in float64.  The bound, derived and not measured (u = unit roundoff of the storage type):
    u |ref| + part                                               attention_reference's own bound and the output rounding (_ratio)
    + expm1(2 u max_j |s_ij|) sum_j p_ij |v_jc|                  the stored score: |s' - s| <= u |s|, so every score of row i moves by at
                                                                 most d = u max_j |s_ij| and every probability by at most expm1(2 d) p
    + u sum_j p_ij |v_jc|                                        the stored probability: |p' - p| <= u p
(_ratio adds 2^-25 for an fp16 result.)  In bf16 with scores of +-30 .. 50 the third term is 0.26 .. 0.5 of sum p |v|: the price of 16-bit
scores in front of exp.  attention_kernel keeps scores and probabilities in fp32; each GPU case prints the error of both forms on the same
operands as a multiple of attention_kernel's bound.

`-m "not gpu"`: (1) the kernel choice of both GEMMs for every case and type; (2) a float64 emulation of the four stages, rounded to the
storage type at the two intermediate stores and at the output, holds every per-stage bound and the composed bound on every case, every
element included; (3) mutation controls on that emulation, bf16 and fp16, every case with more than one item: each mutant must exceed the
bound of the stage it breaks, as the GPU checks would see it (the stage's reference on the operands the stage actually read).  Printed
beside it: whether the composed bound alone would have caught it.  Measured on the CPU, smallest .. largest |err| / bound at the broken
stage over the cases, bf16 | fp16 (the unmutated emulation: at most 0.996 | 1.000 per stage - the store roundings -, 0.66 | 0.70 composed):
    item b reads item 0's keys                6.9 .. 22   | 67 .. 156        MISSED by the composed bound on "flat" rows (all keys of an item
    score slice stride N C instead of N N     8.8 .. 23   | 73 .. 200        are equal there: the softmax does not depend on the scores),
    the scale omitted                         78 .. 141   | 668 .. 1040      caught elsewhere (4.2e4 .. 5e5 / 9 .. 718 x the composed bound)
    item b reads item 0's vt                  81 .. 3e5   | 661 .. 9e6       caught (57 .. 1.8e5)
    the softmax over the wrong axis           1.3e3 .. 2e16 | 2e4 .. 3e7     caught (11 .. 9e4)
    the last key dropped                      3.3 .. 11   | 40 .. 83         caught (4.8 .. 383) but at 1280 "peaked" tokens, bf16: 3.3 at the stage, 0.66 composed, MISSED
    the last 64-column K chunk of P.V dropped 7.1 .. 128  | 70 .. 1020       caught (3.5 .. 117)
The 1280-token case has one item and takes no part in the three per-item mutants (exempt by arithmetic: there is no item 1).

Measured on the MI355X, worst |err| / bound per stage over the cases, fp32 / bf16 / fp16: vt exact; scores 0.010 / 0.044 / 0.043; softmax 0.79 /
0.996 / 0.9999 (the store rounding, as in softmax_rows' own test); P.V 0.54 / 0.50 / 0.80; composed 0.022 / 0.66 / 0.67.  In the 16-bit modes every
stage ratio equals the emulation's to three digits: the stored values are the roundings of the float64 references.  The error of the GEMM form
as a multiple of attention_kernel's bound (attention_kernel itself on the same operands: 0.49 .. 0.97 of it), by type and kind:
              ordinary       peaked        flat
    bf16      81 .. 176      140 .. 297    1.1 .. 1.4
    fp16      22             29 .. 42      0.6 .. 1.3
    fp32      0.016 .. 0.020 0.019 .. 0.022  0.002
In fp32 storage the GEMM form is the more accurate one (shorter accumulation chains than the one-row kernel); in 16-bit storage the rounding
of the scores in front of exp costs two orders of magnitude in bf16 and one and a half in fp16 wherever the rows are not flat.  It is a
property of the form, recorded here and in DESIGN.md (sections 2 and 7), not asserted and not changed.  Every GPU case runs in under half a
second, the CPU part in about 8 s.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from test_hip_conv_kernels import DT_NAME, SENTINEL, TAIL, TD, UNIT, _bound, conv_reference, q
from test_hip_forward_kernels import (INVALID, _attn_data, _guarded, _lib, _ok, _p, _ratio, _stream, _tail_ok, attention_reference,
                                      softmax_rows_reference)

#        H    W    C   B  kind (None: by case and type, so that every type meets every kind)
CASES = [(16, 40, 128, 3, None), (5, 128, 128, 2, None), (8, 80, 128, 2, None), (64, 16, 256, 2, None), (32, 36, 256, 2, None),
         (16, 80, 384, 1, "peaked")]
KINDS = ("peaked", "ordinary", "flat")
RUNS = [(i, dt) for i, c in enumerate(CASES) for dt in ((0, 1, 2) if c[4] is None else (1,))]


def _kind(i, dt):
    return CASES[i][4] or KINDS[(i + dt) % 3]


def _id(r):
    i, dt = r
    H, W, Cc, B, _ = CASES[i]
    return f"attention_gemm-{DT_NAME[dt]}-B{B}-{H}x{W}-C{Cc}-{_kind(i, dt)}"


def _scale(Cc):
    """out_scale of the score GEMM as launch_attention_gemm computes it in fp32"""
    return float(np.float32(1.0) / np.sqrt(np.float32(Cc)))


@functools.lru_cache(maxsize=None)
def _data(i, dt):
    """q, k, v [B,N,C] float64 holding storage-type values (v offset by 0.25 b: the items differ) and attention_reference of them."""
    H, W, Cc, B, _ = CASES[i]
    qq, kk, vv = _attn_data(dict(N=H * W, C=Cc, B=B, dt=dt, kind=_kind(i, dt)))
    ref, part = attention_reference(qq, kk, vv)
    return qq, kk, vv, ref, part


def expected_kernels(dt, N, Cc):
    """(score GEMM, P.V GEMM) as conv_choose answers under the default options"""
    if dt != 0:
        return "conv_generic", "conv_generic"
    return ("conv_sk" if N <= 4096 and Cc <= 1024 else "conv_generic"), ("conv_sk" if N <= 1024 else "conv_generic")


def gemm_choice(dt, H, W, K, Cout):
    """use_conv_choice for one of the two GEMMs (host only: nothing is launched, the pointers are only tested for null)"""
    L = _lib()
    op = L.UseConvOp()
    op.B, op.H, op.W, op.C0, op.Cout, op.ntaps, op.dtype, op.out_dtype = 1, H, W, K, Cout, 1, dt, dt
    dummy = np.zeros(4, np.float32)
    op.src0 = op.w = op.out = dummy.ctypes.data
    name = C.create_string_buffer(32)
    L.check(L.lib().use_conv_choice(C.byref(op), name, 32, None), "use_conv_choice")
    return name.value.decode()


# ---------------------------------------------------------------------------------------------------------------------------
# the stage checks, shared by the emulation (CPU) and the op (GPU)
# ---------------------------------------------------------------------------------------------------------------------------
def _worst(got, ref, bound):
    err = (got.double() - ref).abs()
    r = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


def score_stage(qq, kk, H, W, dt):
    """Per item conv_reference(q, w = k, scale = C^-0.5, no bias): (ref [B,N,N] before the store rounding, its bound with K = C)."""
    B, N, Cc = qq.shape
    sc = _scale(Cc)
    refs, bounds = [], []
    for b in range(B):
        ref, S = conv_reference(qq[b].reshape(1, H, W, Cc), None, 0, kk[b], dt, scale=sc)
        refs.append(ref.reshape(N, N)); bounds.append(_bound(ref, S, dt, dt, sc, Cc).reshape(N, N))
    return torch.stack(refs), torch.stack(bounds)


def pv_stage(P, vt, H, W, dt):
    """Per item conv_reference(P, w = vt [C,N]): (ref [B,N,C], its bound with K = N)."""
    B, N, _ = P.shape
    Cc = vt.shape[1]
    refs, bounds = [], []
    for b in range(B):
        ref, S = conv_reference(P[b].reshape(1, H, W, N), None, 0, vt[b], dt)
        refs.append(ref.reshape(N, Cc)); bounds.append(_bound(ref, S, dt, dt, 1.0, N).reshape(N, Cc))
    return torch.stack(refs), torch.stack(bounds)


def composed_part(qq, kk, vv, part, dt):
    """attention_reference's bound plus the two terms of the stored intermediates (module docstring); the output rounding is _ratio's."""
    u = UNIT[dt]
    s = torch.einsum("bic,bjc->bij", qq, kk) * float(qq.shape[-1]) ** -0.5
    p = torch.softmax(s, 2)
    spv = torch.einsum("bij,bjc->bic", p, vv.abs())
    return part + (torch.expm1(2 * u * s.abs().max(2).values[:, :, None]) + u) * spv


UNDERFLOW = 2.0 ** -126           # the smallest normal fp32 number (module docstring, "softmax")


def check_stages(i, dt, S_st, P_st, vt_st, out_st):
    """The four stage checks and the composed one on stored values (float64 tensors holding storage-type values) -> {stage: ratio}."""
    H, W, Cc, B, _ = CASES[i]
    qq, kk, vv, ref, part = _data(i, dt)
    N = H * W
    r = {"vt": 0.0 if torch.equal(vt_st, vv.transpose(1, 2)) else float("inf")}
    s_ref, s_bound = score_stage(qq, kk, H, W, dt)
    r["scores"] = _worst(S_st, s_ref, s_bound)
    p_ref, p_bound = softmax_rows_reference(S_st.reshape(B * N, N), dt)
    r["softmax"] = _worst(P_st.reshape(B * N, N), p_ref, UNIT[dt] * p_ref + p_bound + UNDERFLOW)
    o_ref, o_bound = pv_stage(P_st, vt_st, H, W, dt)
    r["pv"] = _worst(out_st, o_ref, o_bound)
    r["composed"] = _ratio(out_st, ref, composed_part(qq, kk, vv, part, dt), dt)
    return r


# ---------------------------------------------------------------------------------------------------------------------------
# CPU part: kernel choice, emulation, mutation controls
# ---------------------------------------------------------------------------------------------------------------------------
MUTANTS = {"keys_of_item_0": "scores", "vt_of_item_0": "pv", "score_stride_NC": "scores", "no_scale": "scores", "softmax_axis": "softmax",
           "last_key_dropped": "scores", "last_k_chunk_dropped": "pv"}
PER_ITEM = ("keys_of_item_0", "vt_of_item_0", "score_stride_NC")


def emulate(i, dt, mut=None):
    """launch_attention_gemm in float64 with q(., dt) at the two intermediate stores and at the output; mut: one stage wrong.
    -> (S_st, P_st, vt_st, out_st)"""
    H, W, Cc, B, _ = CASES[i]
    qq, kk, vv, _, _ = _data(i, dt)
    N = H * W
    vt = vv.transpose(1, 2).contiguous()
    k_used = kk[:1].expand(B, N, Cc) if mut == "keys_of_item_0" else kk
    s = torch.einsum("bic,bjc->bij", qq, k_used) * (1.0 if mut == "no_scale" else _scale(Cc))
    S_st = q(s, dt)
    if mut == "last_key_dropped":                             # Cout = N - 1: the last column of the buffer is never written
        S_st[:, :, -1] = 0.0
    if mut == "score_stride_NC":                              # item b written at b N C of the flat buffer, read at b N N
        flat = torch.zeros(B * N * N, dtype=torch.float64)
        for b in range(B):
            flat[b * N * Cc:b * N * Cc + N * N] = S_st[b].reshape(-1)
        S_st = flat.reshape(B, N, N)
    P_st = q(torch.softmax(S_st, 1 if mut == "softmax_axis" else 2), dt)
    vt_used = vt[:1].expand(B, Cc, N) if mut == "vt_of_item_0" else vt
    Pk = P_st
    if mut == "last_k_chunk_dropped":
        Pk, vt_used = P_st[:, :, :-64], vt_used[:, :, :-64]
    out_st = q(torch.einsum("bij,bcj->bic", Pk, vt_used), dt)
    return S_st, P_st, vt, out_st


@pytest.mark.parametrize("r", RUNS, ids=[_id(r) for r in RUNS])
def test_kernel_choice_of_both_gemms(r):
    i, dt = r
    H, W, Cc, _, _ = CASES[i]
    N = H * W
    got = (gemm_choice(dt, H, W, Cc, N), gemm_choice(dt, H, W, N, Cc))
    assert got == expected_kernels(dt, N, Cc), (_id(r), got)


def test_the_cases_reach_both_sides_of_the_fp32_seam():
    ks = {expected_kernels(0, c[0] * c[1], c[2])[1] for c in CASES if c[4] is None}
    assert ks == {"conv_sk", "conv_generic"}
    assert (64 * 16, 32 * 36) == (1024, 1152)


@pytest.mark.parametrize("r", RUNS, ids=[_id(r) for r in RUNS])
def test_emulation_holds_every_stage_bound_and_the_composed_bound(r):
    i, dt = r
    ratios = check_stages(i, dt, *emulate(i, dt))
    qq, kk, _, _, _ = _data(i, dt)
    smax = float((torch.einsum("bic,bjc->bij", qq, kk) * float(qq.shape[-1]) ** -0.5).abs().max())
    print(f"[emulation] {_id(r)}: max |score| {smax:.1f} | " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("r", [r for r in RUNS if r[1]], ids=[_id(r) for r in RUNS if r[1]])
def test_mutation_controls(r):
    i, dt = r
    B = CASES[i][3]
    bad = []
    for name, stage in MUTANTS.items():
        if name in PER_ITEM and B < 2:
            continue
        ratios = check_stages(i, dt, *emulate(i, dt, name))
        print(f"[mut] {_id((i, dt))} {name:21s}: {stage} |err| / bound {ratios[stage]:10.3g} | composed {ratios['composed']:8.3g} -> "
              f"{'caught' if ratios['composed'] > 1.0 else 'MISSED'} by the composed bound alone")
        if not ratios[stage] > 1.0:
            bad.append((name, stage, ratios[stage]))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------
# GPU part
# ---------------------------------------------------------------------------------------------------------------------------
def _workspace(dt, B, N, Cc):
    """(guarded buffer, view of the workspace in the storage type, offset of vt in elements)"""
    L = _lib()
    es = 4 if dt == 0 else 2
    nbytes = L.lib().use_op_attention_gemm_workspace(dt, B, N, Cc)
    assert nbytes >= (B * N * N + B * Cc * N) * es and nbytes % es == 0
    buf, work = _guarded((nbytes // es,), TD[dt])
    return buf, work, nbytes, nbytes // es - B * Cc * N


def _score_gemm(qd, kk_b, H, W, dt):
    """The score GEMM of one item through use_op_conv with the arguments launch_attention_gemm gives it: [N,N] in the storage type."""
    L = _lib()
    N, Cc = H * W, qd.shape[-1]
    obuf, out = _guarded((1, H, W, N), TD[dt])
    w = np.ascontiguousarray(kk_b.numpy().astype(np.float32))          # (storage-type values: exact in fp32, and back)
    op = L.UseConvOp()
    op.B, op.H, op.W, op.C0, op.Cout, op.ntaps, op.dtype, op.out_dtype = 1, H, W, Cc, N, 1, dt, dt
    op.src0, op.w, op.out, op.out_scale = qd.data_ptr(), w.ctypes.data, out.data_ptr(), _scale(Cc)
    _ok(L.lib().use_op_conv(C.byref(op), _stream()), "use_op_conv")
    torch.cuda.synchronize()
    _tail_ok(obuf, "scores")
    return out.reshape(N, N)


@pytest.mark.gpu
@pytest.mark.parametrize("r", RUNS, ids=[_id(r) for r in RUNS])
def test_attention_gemm_stages_and_composition(r):
    L = _lib()
    i, dt = r
    H, W, Cc, B, _ = CASES[i]
    N = H * W
    assert (gemm_choice(dt, H, W, Cc, N), gemm_choice(dt, H, W, N, Cc)) == expected_kernels(dt, N, Cc)
    qq, kk, vv, ref, part = _data(i, dt)
    d = [t.to(TD[dt]).cuda().contiguous() for t in (qq, kk, vv)]
    obuf, out = _guarded((B, N, Cc), TD[dt])
    wbuf, work, nbytes, vt_off = _workspace(dt, B, N, Cc)
    _ok(L.lib().use_op_attention_gemm(_p(d[0]), _p(d[1]), _p(d[2]), _p(out), _p(work), nbytes, dt, B, H, W, Cc, _stream()), "use_op_attention_gemm")
    torch.cuda.synchronize()
    _tail_ok(obuf, "out"); _tail_ok(wbuf, "the workspace")
    P_dev = work[:B * N * N].reshape(B, N, N)
    vt_st = work[vt_off:].reshape(B, Cc, N).cpu().double()
    got = out.cpu()
    assert bool(torch.isfinite(got.float()).all())
    # the scores, launch by launch again, and the softmax of all B N rows in one launch as the op issues it
    sbuf, S_dev = _guarded((B, N, N), TD[dt])
    for b in range(B):
        S_dev[b].copy_(_score_gemm(d[0][b], kk[b], H, W, dt))
    S_st = S_dev.cpu().double()
    _ok(L.lib().use_op_softmax_rows(_p(S_dev), dt, B * N, N, _stream()), "use_op_softmax_rows")
    torch.cuda.synchronize()
    _tail_ok(sbuf, "the softmax rows")
    assert torch.equal(S_dev, P_dev), "the scores of use_op_conv do not reproduce the stored probabilities bit for bit"
    ratios = check_stages(i, dt, S_st, P_dev.cpu().double(), vt_st, got.double())
    # attention_kernel on the same operands: both forms as multiples of attention_kernel's bound
    abuf, aout = _guarded((B, N, Cc), TD[dt])
    _ok(L.lib().use_op_attention(_p(d[0]), _p(d[1]), _p(d[2]), _p(aout), dt, B, N, Cc, _stream()), "use_op_attention")
    torch.cuda.synchronize()
    _tail_ok(abuf, "out of use_op_attention")
    r_core, r_gemm = _ratio(aout.cpu(), ref, part, dt), _ratio(got, ref, part, dt)
    print(f"[measured] {_id(r)}: " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()) +
          f" | against attention_kernel's bound: attention_kernel {r_core:.3f}, GEMM form {r_gemm:.3f} (x {r_gemm / max(r_core, 1e-30):.1f})")
    assert r_core < 1.0, r_core
    assert all(v < 1.0 for v in ratios.values()), ratios


@pytest.mark.gpu
def test_attention_gemm_refuses_what_it_cannot_run():
    L = _lib()
    lib = L.lib()
    dt, B = 1, 2
    qkv = torch.zeros(B * 640 * 256, dtype=TD[dt], device="cuda")
    obuf, out = _guarded((B * 640 * 256,), TD[dt])
    wbuf, work, nbytes, _ = _workspace(dt, B, 640, 128)
    big = work.numel() * 2
    stream = _stream()

    def call(H, W, Cc, dtype=dt, nb=big, ptrs=None):
        a = [_p(qkv), _p(qkv), _p(qkv), _p(out), _p(work)] if ptrs is None else ptrs
        return lib.use_op_attention_gemm(a[0], a[1], a[2], a[3], a[4], nb, dtype, B, H, W, Cc, stream)
    assert lib.use_op_attention_gemm_workspace(dt, B, 512, 128) == 0 and lib.use_op_attention_gemm_workspace(dt, B, 576, 128) == 0
    assert lib.use_op_attention_gemm_workspace(dt, B, 640, 192) == 0 and lib.use_op_attention_gemm_workspace(3, B, 640, 128) == 0
    assert call(16, 32, 128) == INVALID, "N = 512"
    assert call(16, 36, 128) == INVALID, "N = 576"
    assert call(16, 40, 192) == INVALID, "C = 192"
    assert call(16, 40, 128, nb=nbytes - 1) == INVALID, "a workspace one byte short"
    assert call(16, 40, 128, dtype=3) == INVALID and call(16, 40, 128, dtype=-1) == INVALID, "dtype out of range"
    for k in range(5):
        a = [_p(qkv), _p(qkv), _p(qkv), _p(out), _p(work)]
        a[k] = None
        assert call(16, 40, 128, ptrs=a) == INVALID, f"null pointer {k}"
    torch.cuda.synchronize()
    assert bool((obuf == SENTINEL).all()) and bool((wbuf == SENTINEL).all()), "a refused call wrote"
    assert call(16, 40, 128, nb=nbytes) == 0                   # (and the same call with the exact size runs)
    torch.cuda.synchronize()
    assert bool((obuf[B * 640 * 128:] == SENTINEL).all()), "write past the end of out"
    _tail_ok(wbuf, "the workspace")
