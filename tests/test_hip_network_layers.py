"""The score network layer by layer: every launch of one evaluation, as the engine's launch trace (use_set_option("trace", 1),
HipScoreEngine.trace()) reports it, against the float64 reference of that one operation on the operands the launch read, in fp32, bf16
and fp16.  The per-kernel files test the kernels through use_op_*; this file tests the code that strings them together (Fwd::run,
Fwd::resblock, Fwd::attention, Fwd::conv, gn_coef in csrc/use_engine.cpp): which tensors, totals, coefficient arrays, tembias rows and
biases each launch is given.  No reference and no bound is stated here: they are imported from tests/test_hip_conv_kernels.py,
tests/test_hip_forward_kernels.py and tests/test_hip_input_head_kernels.py.

The network: nf 128, ch_mult (1, 1, 2, 2), one res-block per level, 32 x 64 input, 2 items at t = (0.83, 0.21); maps 32x64, 16x32, 8x16,
4x8; a 256-channel, 32-token bottleneck (fused attention block in the 16-bit modes, three NIN + attention_kernel + NIN_3 in fp32).  Two
option sets: "default" (every map is small: GroupNorm finalised inside the consumer, atomic totals) and "workload" (gn_inline 1024,
conv_v4_min_blocks 1: the 32x64 level as the benchmark's large maps - wide kernel, per-workgroup partial totals, gn_finalize_part,
coefficient arrays into the convolutions).  fp32 storage sends every map of at most 4096 pixels to conv_sk, which only knows atomic
totals: the fp32 workload case reads coefficient arrays but no kernel of it writes partial totals; that assertion is made in bf16 / fp16.
The long-sequence attention path (N > 512 tokens, launch_attention_gemm) has a network of its own, "refine_long": the unconditional
2-channel generator with ch_mult (1, 2) on a 40 x 64 input (use_plan takes T' in multiples of 64, which rules out 32 x 80), two items; its
bottleneck is 20 x 32 = 640 tokens of 256 channels, the smallest map that takes the form.  Its 2 + 2 B launches are traced as transpose /
attn_gemm (one per item and GEMM) / softmax_rows and checked with the references of tests/test_hip_attention_gemm.py.  The softmax rewrites
the scores in place: each score GEMM is issued again through use_op_conv on the operands the trace names and held to its bound, and
use_op_softmax_rows of those scores must give the engine's probabilities bit for bit.  Four items in bf16 (2 + 2 sub-batches: the form on
a secondary stream) equal the unsplit batch and the two-item evaluation bit for bit.

Per launch (test_every_launch_holds_its_bound): inputs copied back as stored, the reference evaluated on them, every element of every
stored output held to the operation's own bound.  Inline GroupNorm: coefficients from the very integers the consumer reads (partial
totals summed first), n and epsilon the test's own (the traced gn_inv_n / gn_eps are asserted to be those).  Finalised arrays: checked as
their own entry against the integers (bound of test_finalize_from_partials_matches_finalize_from_totals), then used as stored.  Written
totals: against the stored output with the bounds of the producing kernel's file.  tembias: the table against the time-embedding
references, a layer's term the row the trace names.  The 6-channel network's separate combine_add rewrites its input in place: the
convolution in front of it and the Combine are held together, to the sum of their two bounds (the Combine passes its input on with unit
gain), the Combine's totals to its own bound; the partial totals that convolution wrote are dropped by the engine and not checked.

Wiring, independently of the per-launch check: (1) fp32 block outputs, attention output, pyramid levels and x4 equal the oracle's taps of
the same name to 5e-4 of the maximum; (2) the graph "which launch wrote what each launch reads" is the same in every precision and option
set once the attention block and the finalise launches are collapsed; (3) every activation read is an input of the evaluation or an
earlier launch's output, every output has one writer (but combine_add's in-place one), the parameter names used are exactly
expected_weights() (the unconditional generator: minus the Fourier W and the Dense_0 layers, which it has and never reads - the
reference does not either), every convolution weight is used once.

`-m "not gpu"`: the same network as a Python walk over the same references.  Without rounding its output and every tap equal
ncsnpp_forward in float64 to 1e-9 of the maximum (measured 8e-15 .. 1e-14).  With rounding to the storage type at every store it emulates the engine
and carries the mutation controls: one layer wrong at a time, which must exceed that layer's bound in bf16 and in fp16; the end-to-end
error of each mutant is printed beside lp.fwd_bound (x 1.25: inputs other than the fixture's).  Measured on the CPU, |mutant - reference| /
bound at the layer, bf16 / fp16, and in brackets the end-to-end error as a multiple of that end-to-end bound (the unmutated walk: 0.54 / 0.51):
    epsilon 1e-5 in one finalised GroupNorm             24 / 24          (0.60 / 0.44: MISSED end to end in both)
    one of four partial totals left out                 7.5e5 / 7.7e5    (2.3 / 14.8)
    inv_n of the quarter-size map                       9e8 / 9e8        (15 / 109)
    the other item's tembias row, t = 0.83 | 0.21       55 / 433         (6.4 / 45)
    out_scale in front of the residual                  12 / 96          (4.9 / 35)
    the shortcut's second source dropped                14 / 110         (9.4 / 65)
    Combine bias omitted                                3.0 / 24         (4.3 / 30)
    activated FIR output into the shortcut              11 / 88          (9.2 / 65)
    the two skips of the coarsest level swapped         18 / 140         (17 / 123)
and on the refine_long network (end to end: lp.refine_bound x 1.25; the unmutated walk: 0.38 / 0.22):
    item 1's score GEMM on item 0's keys                6.5 / 52         (1.7 / 6.6)
    item 1's P.V GEMM on item 0's slice of vt           83 / 648         (1.5 / 6.3)
With these random weights and two far-apart times most mutants are gross end to end as well; the epsilon is not, and one partial of four
exceeds the bf16 end-to-end bound by a factor of 2.3 only, with a quarter of the map missing from the statistics.  No arithmetic
exemption was needed.  The swap of the skip tensors is made inside a level (its two skips have the same shape); across levels the shapes
differ in this network, so that swap cannot be built.

Measured on the MI355X, worst |err| / bound per entry kind over the nine cases of the 4-level networks (each case prints its own line): input convolution conv_in
0.34 (fp32), conv_in_split 0.990 (bf16) / 0.937 (fp16), conv_generic on 8 channels 0.995 - store-bound kernels at the bottom of a binade,
as in their own file; conv_sk 0.19, conv_v2 0.19, conv_v5 0.21, pyr_conv_ws 0.019, convolution + combine_add 0.15; res-block FIR 0.61
(fp32) / 0.999 (16-bit, the store rounding), pyramid FIR 0.55; gn_finalize 0.22, gn_finalize_part 0.12; attn_fused 0.46, attention_kernel
0.009; score_out 0.31, temb_dense 0.013, temb_mlp 0.002, pack_input exact; totals: conv_in 0.07, conv_in_split 0.10, conv_generic 0.06,
conv_sk 0.12, conv_v2 0.15, conv_v5 0.13, attn_fused 0.36, combine_add 0.10.  End to end |err| / max: fp32 2.8e-5, bf16 1.7e-2 (6-channel
2.6e-2), fp16 2.0e-3.  The three refine_long cases, fp32 / bf16 / fp16: score GEMMs 0.004 / 0.025 / 0.025 (conv_sk in fp32, conv_generic in
16 bit), softmax_rows 0.27 / 0.995 / 0.98, P.V GEMMs 0.14 / 0.50 / 0.50, transpose_nc exact, conv_generic (the 256-channel 1x1 NIN on a 640-pixel
map, 16 bit) 0.25; end to end 1.3e-6 / 1.04e-2 / 1.5e-3.  No composition error and no engine bug was found.  Every GPU case takes under 2 s, the CPU part about 25 s (the
mutation controls re-walk the network behind each mutated layer)."""
import functools

import numpy as np
import pytest
import torch

import lowprec as lp
from test_hip_attention_gemm import UNDERFLOW, _score_gemm, expected_kernels
from test_hip_conv_kernels import DT_NAME, GN_EPS, SQRT1_2, TD, UNIT, _bound, _check_stats, conv_reference, gn_coef_reference, q
from test_hip_forward_kernels import (_combine_totals_ratio, _fused_totals_ratio, _ratio, attention_reference, attn_block_reference,
                                      combine_reference, dense_reference, fir_reference, gn_coef_from_totals, pack_reference,
                                      score_out_reference, softmax_rows_reference, temb_reference)
from test_hip_input_head_kernels import _finalize_ratios, _in_bound, _n_ser, _split_model, _totals_ratio

NF, CH_MULT, NRB, NFREQ, TP, NB = 128, (1, 1, 2, 2), 1, 32, 64, 2
TS = (0.83, 0.21)
GN_INLINE_DEFAULT = 128 * 160
OPTSETS = {"default": {"gn_inline": GN_INLINE_DEFAULT, "conv_v4_min_blocks": 80}, "workload": {"gn_inline": 1024, "conv_v4_min_blocks": 1}}
VARIANTS = {"score": dict(input_channels=4, conditional=True), "both": dict(input_channels=6, conditional=True),
            "refine": dict(input_channels=2, conditional=False), "refine_long": dict(input_channels=2, conditional=False)}
# "refine_long": two levels on a 40 x 64 input - the bottleneck is 20 x 32 = 640 tokens of 256 channels, the smallest map that takes the
# GEMM form of the attention core (N > 512; use_plan takes T' in multiples of 64, which rules out a 32 x 80 input); every other variant:
# CH_MULT on NFREQ x TP
GEOM = {"refine_long": ((1, 2), 40, 64)}
LONG = ("refine_long",)


def _geom(variant):
    """(ch_mult, n_freq, T')"""
    return GEOM.get(variant, (CH_MULT, NFREQ, TP))


def _is_refine(variant):
    return not VARIANTS[variant]["conditional"]


PREC = {"fp32": 0, "bf16": 1, "fp16": 2}
CASES = [("score", p, o) for p in ("fp32", "bf16", "fp16") for o in ("default", "workload")] + \
        [("both", "bf16", "workload"), ("refine", "fp32", "default"), ("refine", "bf16", "default")] + \
        [("refine_long", p, "default") for p in ("fp32", "bf16", "fp16")]
CASE_IDS = ["-".join(c) for c in CASES]


# ---------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _state_dict(variant):
    from universal_speech_enhancement_amd.testing import weights as tw
    return tw.make_state_dict(4321, nf=NF, ch_mult=_geom(variant)[0], num_res_blocks=NRB, **VARIANTS[variant])


@functools.lru_cache(maxsize=None)
def _inputs(variant):
    """(x, y, y2, t): complex64 [B,1,F,T'] (y, y2 None where the network has no such input), t float32 [B] (None: unconditional)."""
    from universal_speech_enhancement_amd.testing import noise as tn
    _, nfreq, tp = _geom(variant)
    mk = lambda s: torch.from_numpy(tn.complex_normal(77, s, (NB, 1, nfreq, tp))) * 0.5
    ic = VARIANTS[variant]["input_channels"]
    return mk("x"), (mk("y") if ic >= 4 else None), (mk("y2") if ic == 6 else None), (torch.tensor(TS) if not _is_refine(variant) else None)


@functools.lru_cache(maxsize=None)
def _oracle(variant):
    """float64 oracle output [B,F,T,2] (re, im) and taps (NHWC float64)."""
    from oracle import ncsnpp_oracle as no
    sd = {k: torch.from_numpy(v).double() for k, v in _state_dict(variant).items()}
    x, y, y2, t = _inputs(variant)
    xin = torch.cat([v for v in (x, y, y2) if v is not None], 1).to(torch.complex128)
    taps = {}
    with torch.no_grad():
        out = no.ncsnpp_forward(sd, xin, t.double() if t is not None else None, ch_mult=_geom(variant)[0], num_res_blocks=NRB, taps=taps,
                                discriminative=_is_refine(variant))
    taps = {k: v.permute(0, 2, 3, 1).contiguous() for k, v in taps.items() if v is not None and v.dim() == 4}
    return torch.view_as_real(out[:, 0]).contiguous(), taps


def _cplx(v):
    """complex [B,1,F,T] -> float32 [B,F,T,2]"""
    return torch.view_as_real(v[:, 0]).float().contiguous()


# ---------------------------------------------------------------------------------------------------------------------------
# one operation: operands as stored -> [(reference before the store rounding, ratio(got) -> worst |err| / bound, value as stored)]
# shared by the walk (CPU) and the per-launch check (GPU)
# ---------------------------------------------------------------------------------------------------------------------------
def _worst0(got, ref, bound):
    err = (got.double() - ref).abs()
    r = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


def _par(sd, name):
    return torch.from_numpy(np.ascontiguousarray(sd[name])).float()


def _weight(sd, name, cin, cout):
    """A convolution weight as the kernels see it: [cout, cin, 3, 3] or [cout, cin], zero-padded (NIN: W [Cin, Cout] transposed)."""
    w = _par(sd, name)
    if name.endswith(".W"):
        return w.T.contiguous()
    if w.dim() == 4 and w.shape[-1] == 1:
        w = w[:, :, 0, 0]
    out = torch.zeros((cout, cin) + tuple(w.shape[2:]))
    out[:w.shape[0], :w.shape[1]] = w
    return out


def _vec(sd, name, n):
    v = _par(sd, name)
    out = torch.zeros(n)
    out[:v.numel()] = v
    return out


def _cat(a, b):
    return a if b is None else torch.cat([a, b], -1)


def _input_conv_class(dt, odt, c0, cout):
    """The kernel class of the network's input convolution, for the bound of tests/test_hip_input_head_kernels.py."""
    if c0 == 8:
        return "conv_generic"
    return "conv_in_split" if (odt and cout % 128 == 0) else "conv_in"


def conv_eval(a, sd, dt):
    """a: x [B,H,W,Cin] (both concat halves), xs (both shortcut sources) / res / pyr / coef [B,Cin,2] / temb [B,Cout] or None, act, scale,
    cout, odt, in_dt (storage type of x: 0 for the input convolution), params.  -> (ref, bound, stored)."""
    p, x, cout, odt, in_dt = a["params"], a["x"], a["cout"], a["odt"], a["in_dt"]
    cin = x.shape[-1]
    w = _weight(sd, p["w"], cin, cout)
    bias = _vec(sd, p["b"], cout)
    if "b2" in p:
        # one fp32 array, as the engine packs Conv_1.bias + Conv_2.bias (the unrounded walk: the float64 sum, as the oracle adds them)
        bias = bias + _vec(sd, p["b2"], cout) if dt is not None else bias.double() + _vec(sd, p["b2"], cout).double()
    xs = a.get("xs")
    w2 = _weight(sd, p["w2"], xs.shape[-1], cout) if xs is not None else None
    pyr = a.get("pyr")
    w4 = _weight(sd, p["cb_w"], pyr.shape[-1], cout) if "cb_w" in p and not a.get("no_cb") else None
    b4 = _vec(sd, p["cb_b"], cout) if w4 is not None and not a.get("no_b4") else None
    ref, S = conv_reference(x, a.get("coef"), a["act"], w, in_dt, xs=xs, w2=w2, bias=bias, temb=a.get("temb"), res=a.get("res"), scale=a["scale"],
                            pyr=pyr if w4 is not None else None, w4=w4, b4=b4)
    if dt is None:
        return ref, None, ref
    is_input = cin in (4, 8) and w.dim() == 4
    if is_input:
        d = dict(x=x, w=w, bias=bias, ref=ref, S=S, scale=a["scale"])
        kern = _input_conv_class(dt, odt, cin, cout)
        return ref, _in_bound(d, odt, kern, cin), (_split_model(d, odt) if kern == "conv_in_split" else q(ref, odt))
    K = cin * (9 if w.dim() == 4 else 1) + (xs.shape[-1] if xs is not None else 0)
    return ref, _bound(ref, S, in_dt, odt, a["scale"], K), q(ref, odt)


def op_conv(a, sd, dt):
    ref, bound, stored = conv_eval(a, sd, dt)
    return [(ref, (lambda got: _worst0(got, ref, bound)), stored)]


def op_fir(x, coef, act, up, dt, slots):
    """slots: (activated wanted, raw wanted)"""
    raw, praw, av, pact = fir_reference(x, coef, act, up)
    out = []
    for want, r, part in ((slots[0], av, pact), (slots[1], raw, praw)):
        out.append(None if not want else (r, (lambda got, r=r, part=part: _ratio(got, r, part, dt or 0)), q(r, dt)))
    return out


def _group_moments(tot, groups, hw):
    B, Cc, _ = tot.shape
    cpg = Cc // groups
    n = cpg * hw
    S = tot[..., 0].reshape(B, groups, cpg).sum(-1).double() / 2 ** 20
    Q = tot[..., 1].reshape(B, groups, cpg).sum(-1).double() / 2 ** 20
    mean = S / n
    return mean, torch.sqrt((Q / n - mean * mean).clamp_min(0.0)), cpg


def op_finalize(tot, sd, params, groups, hw, eps=GN_EPS, n_tok=None):
    """tot: int64 [B,C,2] (both sources, partials summed).  The coefficient array [B,C,2] fp32 against float64 on the same integers."""
    gamma, beta = _par(sd, params["gn_w"]), _par(sd, params["gn_b"])
    want = gn_coef_from_totals(tot, gamma, beta, groups, hw)
    mean, std, cpg = _group_moments(tot, groups, hw)

    def ratio(got):
        return max(_finalize_ratios(got.double(), want, mean, std, beta, hw, cpg))
    made = gn_coef_from_totals(tot, gamma, beta, groups, hw if n_tok is None else n_tok, eps)     # (mutants: another epsilon / pixel count)
    return [(want, ratio, made.float().double())]


def op_attn_fused(x, coef, sd, p, dt):
    """x [B,N,C] stored, coef [B,C,2]"""
    W = [_weight(sd, p[k], 0, 0) for k in ("w", "x0", "x2", "x4")]
    bias = [_par(sd, p[k]) for k in ("b", "x1", "x3", "x5")]
    ref, part, _ = attn_block_reference(x, coef, W, bias, dt)
    if dt is None:
        return [(ref, None, ref)]
    return [(ref, (lambda got: _ratio(got, ref, part, dt)), q(ref, dt))]


def op_attn_core(qq, kk, vv, dt):
    ref, part = attention_reference(qq, kk, vv)
    return [(ref, (lambda got: _ratio(got, ref, part, dt if dt is not None else 0)), q(ref, dt))]


def op_transpose(v):
    """v [B,1,N,C] stored -> vt [B,1,C,N], bit for bit"""
    want = v.transpose(2, 3).contiguous()
    return [(want, (lambda got: 0.0 if torch.equal(got.double(), want) else float("inf")), want)]


def op_attn_gemm(x, w, scale, dt):
    """One GEMM of the long-sequence attention: x [1,H,W,K] and the "weights" w [Cout,K], both activations as stored; no bias."""
    ref, S = conv_reference(x, None, 0, w, dt, scale=scale)
    if dt is None:
        return [(ref, None, ref)]
    bound = _bound(ref, S, dt, dt, scale, x.shape[-1])
    return [(ref, (lambda got: _worst0(got, ref, bound)), q(ref, dt))]


def op_softmax_rows(x, dt):
    """x [B,N,1,N]: the stored scores (bound: tests/test_hip_attention_gemm.py, "softmax")"""
    ref, bound = softmax_rows_reference(x, dt)
    if dt is None:
        return [(ref, None, ref)]
    full = UNIT[dt] * ref + bound + UNDERFLOW
    return [(ref, (lambda got: _worst0(got, ref, full)), q(ref, dt))]


def attention_gemm_eligible(N, Cc):
    """attention_gemm_eligible of csrc/use_kernels.hip (N % 128 == 0 implies the K-chunk condition of either storage width)"""
    return N > 512 and N % 128 == 0 and Cc % 128 == 0


def op_combine(h, pyr, sd, p, dt, no_bias=False):
    """h [B,P,C] stored, pyr [B,P,8]"""
    ref, part = combine_reference(h, pyr, _weight(sd, p["cb_w"], pyr.shape[-1], h.shape[-1]), _vec(sd, p["cb_b"], h.shape[-1]), "bias" if no_bias else None)
    return ref, part


def op_temb(t, sd, p):
    silu, bound, _ = temb_reference(t, _par(sd, p["w"]), _par(sd, p["x0"]), _par(sd, p["x1"]), _par(sd, p["x2"]), _par(sd, p["x3"]))
    return silu, bound


def op_score_out(pyr, t, sd, p, sign, dt=0):
    """pyr [B,P,PC] fp32 stored"""
    ref, bound = score_out_reference(pyr, t, _weight(sd, p["w"], pyr.shape[-1], 2), _par(sd, p["b"]), sign)
    return [(ref, (lambda got: _worst0(got, ref, bound)), q(ref, dt))]


def _fixed_totals(v, parts=1):
    """Stored map [B,H,W,C] -> int64 [B,parts,C,2]: the fixed-point totals (sum, sum of squares, x 2^20) of `parts` bands of rows."""
    B, H, W, Cc = v.shape
    cuts = np.linspace(0, H, parts + 1).astype(int)
    return torch.stack([torch.stack([torch.round(v[:, a:b].reshape(B, -1, Cc).pow(e).sum(1) * 2 ** 20) for e in (1, 2)], -1)
                        for a, b in zip(cuts[:-1], cuts[1:])], 1).long()


# ---------------------------------------------------------------------------------------------------------------------------
# the walk: Fwd::run over the references
# ---------------------------------------------------------------------------------------------------------------------------
class Walk:
    """The engine's launch sequence for one evaluation, layer by layer on the CPU.  dt None: float64 throughout (pinned to the oracle);
    dt 0 / 1 / 2: every store rounded to the storage type (the engine's emulation).  compute=False: names and shapes only.
    mut: one deliberately wrong layer; base: the unmutated walk, whose layers in front of the mutated one are taken over."""

    def __init__(self, variant, dt, gn_inline=GN_INLINE_DEFAULT, compute=True, mut=None, base=None, sign=-1.0):
        self.sd, self.variant, self.dt, self.gn_inline, self.compute, self.mut, self.base = _state_dict(variant), variant, dt, gn_inline, compute, mut, base
        self.store = 0 if dt is None else dt
        ic = VARIANTS[variant]["input_channels"]
        self.pc, self.pcp, self.cond = ic, (8 if ic > 4 else 4), VARIANTS[variant]["conditional"]
        self.ch_mult, self.nfreq, self.tp = _geom(variant)
        self.sign = sign
        self.layers, self.taps, self.mut_layer, self.mut_ratio = [], {}, None, None
        self.run()

    # -- bookkeeping --
    def emit(self, kind, params, shapes, fn, tap=None):
        """One launch: fn() -> list per output slot of (ref, ratio, stored) or None.  Returns the stored outputs."""
        i = len(self.layers)
        if self.base is not None and self.mut_layer is None and not self.pending_mut:
            lay = self.base.layers[i]
        elif not self.compute:
            lay = dict(kind=kind, params=dict(params), shapes=shapes, outs=[None if s is None else torch.zeros(s, dtype=torch.float64) for s in shapes], res=None)
        else:
            res = fn()
            lay = dict(kind=kind, params=dict(params), shapes=shapes, outs=[None if r is None else r[2] for r in res], res=res)
        assert lay["kind"] == kind
        self.layers.append(lay)
        if tap:
            self.taps[tap] = lay["outs"][0]
        return lay["outs"]

    pending_mut = False

    def hit(self, name, site=True):
        """True once, at the first site of the mutation `name`."""
        if self.mut == name and site and self.mut_layer is None and self.compute:
            self.pending_mut = True
            return True
        return False

    def mutated(self, outs_mut, slot=0):
        """Called right after the emit of the mutated layer: its unmutated check against the mutant's stored output."""
        i = len(self.layers) - 1
        self.mut_layer, self.pending_mut = i, False
        self.mut_ratio = self.base.layers[i]["res"][slot][1](outs_mut)

    # -- GroupNorm --
    def totals(self, a, parts=1):
        return _fixed_totals(a, parts)

    def coef_inline(self, a, a2, prefix, drop_part=False):
        x = _cat(a, a2)
        Cc = x.shape[-1]
        groups = min(Cc // 4, 32)
        gamma, beta = _par(self.sd, prefix + ".weight"), _par(self.sd, prefix + ".bias")
        if not self.compute:
            return torch.zeros(x.shape[0], Cc, 2, dtype=torch.float64)
        if self.dt is None:
            return gn_coef_reference(x, gamma, beta, groups)
        return gn_coef_from_totals(self.totals(x).sum(1), gamma, beta, groups, x.shape[1] * x.shape[2])

    def finalize(self, a, a2, prefix, parts=1):
        """gn_coef: a gn_finalize launch -> the stored coefficient array"""
        x = _cat(a, a2)
        B, H, Wd, Cc = x.shape
        groups = min(Cc // 4, 32)
        p = {"gn_w": prefix + ".weight", "gn_b": prefix + ".bias"}
        kw = {}
        drop = False
        late = len(self.layers) > 55                           # (sites late in the walk: the layers in front are the unmutated walk's)
        if self.hit("eps", late):
            kw["eps"] = 1e-5
        elif self.hit("inv_n", late):
            kw["n_tok"] = H * Wd // 4
        elif self.hit("partial", late and parts > 1):
            drop = True

        def fn():
            if self.dt is None:
                c = gn_coef_reference(x, _par(self.sd, p["gn_w"]), _par(self.sd, p["gn_b"]), groups)
                return [(c, None, c)]
            tot = self.totals(x, parts)
            full = op_finalize(tot.sum(1), self.sd, p, groups, H * Wd, **kw)
            if drop:                                          # one partial of the totals left out
                return [(full[0][0], full[0][1], op_finalize(tot[:, 1:].sum(1), self.sd, p, groups, H * Wd)[0][2])]
            return full
        was = self.pending_mut
        out = self.emit("gn_finalize", p, [(B, Cc, 2)], fn)[0]
        if was:
            self.mutated(out)
        return out

    def large(self, a):
        return a.shape[1] * a.shape[2] > self.gn_inline

    # -- Fwd::conv --
    def conv(self, a, a2, gn, act, wname, bname, cout, temb_res=None, res=None, scale=1.0, pyr=None, cb=None, odt=None, sx0=None, sx1=None, w2=None, tap=None,
             parts=1):
        dt = self.dt
        odt = self.store if odt is None else odt
        x = _cat(a, a2)
        B, H, Wd, _ = x.shape
        params = {"w": wname, "b": bname}
        coef = None
        if gn is not None:
            if self.large(a):
                coef = self.finalize(a, a2, gn, parts=self.parts_of(a))
            else:
                params.update(gn_w=gn + ".weight", gn_b=gn + ".bias")
                coef = self.coef_inline(a, a2, gn)
        temb = None
        if temb_res is not None and self.cond:
            params.update(dense_w=f"all_modules.{temb_res}.Dense_0.weight", dense_b=f"all_modules.{temb_res}.Dense_0.bias")
            r0 = self.dense_row[temb_res]
            temb = self.tembias[:, r0:r0 + cout]
        if w2 is not None:
            params.update(w2=w2 + ".weight", b2=w2 + ".bias")
        if cb is not None:
            params.update(cb_w=cb + ".weight", cb_b=cb + ".bias")
        in_dt = 0 if (x.shape[-1] in (4, 8) and dt is not None) else dt
        op = dict(params=params, x=x, xs=_cat(sx0, sx1) if w2 is not None else None, res=res, pyr=pyr if cb is not None else None, coef=coef, temb=temb,
                  act=act, scale=scale, cout=cout, odt=odt if dt is not None else None, in_dt=in_dt)
        m = dict(op)
        if temb is not None and self.hit("temb_row", len(self.layers) > 45):
            m["temb"] = temb.flip(0)
        elif res is not None and scale != 1.0 and self.hit("scale_before_res", H <= 8):
            m["res"] = res / scale                            # (conv + res / s) s = conv s + res
        elif w2 is not None and sx1 is not None and self.hit("shortcut_src"):
            m["xs"] = torch.cat([sx0, torch.zeros_like(sx1)], -1)
        elif cb is not None and self.hit("combine_bias", H <= 8):
            m["no_b4"] = True
        was = self.pending_mut
        out = self.emit("conv", params, [(B, H, Wd, cout)], lambda: op_conv(m if was else op, self.sd, dt), tap=tap)[0]
        if was:
            self.mutated(out)
        self.part_count[id(out)] = parts if (self.large(a) and parts > 1) else 1
        return out

    def parts_of(self, a):
        return self.part_count.get(id(a), 1)

    def wide_parts(self, H, Wd):
        """partial totals a wide-kernel producer of a large map writes (conv_v4_tiles); 1: atomic totals"""
        return ((H + 15) // 16) * ((Wd + 31) // 32) if (self.dt not in (None, 0) and H * Wd > self.gn_inline) else 1

    # -- Fwd::resblock --
    def resblock(self, x, skip, idx, in_ch, out_ch, up=False, down=False, pyr=None, cb=None):
        p = f"all_modules.{idx}"
        dt = self.dt
        has_c2 = in_ch != out_ch or up or down
        sx0, sx1 = x, skip
        if up or down:
            B, H, Wd, Cc = x.shape
            H2, W2 = (2 * H, 2 * Wd) if up else (H // 2, Wd // 2)
            coef0 = self.finalize(x, skip, p + ".GroupNorm_0", parts=self.parts_of(x))
            hr, xr = self.emit("fir_up" if up else "fir_down", {}, [(B, H2, W2, Cc)] * 2, lambda: op_fir(x, coef0, 1, up, dt, (True, True)))
            h = self.conv(hr, None, None, 0, p + ".Conv_0.weight", p + ".Conv_0.bias", out_ch, temb_res=idx, parts=self.wide_parts(H2, W2))
            sx0, sx1 = xr, None
            if self.hit("fir_act_raw", up):
                sx0 = hr
        else:
            h = self.conv(x, skip, p + ".GroupNorm_0", 1, p + ".Conv_0.weight", p + ".Conv_0.bias", out_ch, temb_res=idx,
                          parts=self.wide_parts(x.shape[1], x.shape[2]))
        parts = self.wide_parts(h.shape[1], h.shape[2])
        if has_c2:
            return self.conv(h, None, p + ".GroupNorm_1", 1, p + ".Conv_1.weight", p + ".Conv_1.bias", out_ch, scale=SQRT1_2, pyr=pyr, cb=cb, sx0=sx0, sx1=sx1,
                             w2=p + ".Conv_2", tap=f"block.{idx}", parts=parts)
        return self.conv(h, None, p + ".GroupNorm_1", 1, p + ".Conv_1.weight", p + ".Conv_1.bias", out_ch, res=x, scale=SQRT1_2, pyr=pyr, cb=cb,
                         tap=f"block.{idx}", parts=parts)

    # -- Fwd::attention --
    def attention(self, x, idx):
        p = f"all_modules.{idx}"
        B, H, Wd, Cc = x.shape
        gn = p + ".GroupNorm_0"
        if self.dt in (1, 2) and Cc == 256 and H * Wd <= 96:  # the fused block (16-bit storage, C 256, N <= 96)
            params = {"gn_w": gn + ".weight", "gn_b": gn + ".bias", "w": p + ".NIN_0.W", "b": p + ".NIN_0.b", "x0": p + ".NIN_1.W", "x1": p + ".NIN_1.b",
                      "x2": p + ".NIN_2.W", "x3": p + ".NIN_2.b", "x4": p + ".NIN_3.W", "x5": p + ".NIN_3.b"}
            coef = self.coef_inline(x, None, gn)

            def fn():
                r = op_attn_fused(x.reshape(B, H * Wd, Cc), coef, self.sd, params, self.dt)[0]
                return [(r[0].reshape(B, H, Wd, Cc), (lambda got: r[1](got.reshape(B, H * Wd, Cc))), r[2].reshape(B, H, Wd, Cc))]
            return self.emit("attn_fused", params, [(B, H, Wd, Cc)], fn, tap=f"attn.{idx}")[0]
        qkv = [self.conv(x, None, gn, 0, p + f".NIN_{k}.W", p + f".NIN_{k}.b", Cc) for k in range(3)]
        if attention_gemm_eligible(H * Wd, Cc):               # launch_attention_gemm: transpose, B score GEMMs, softmax rows, B P.V GEMMs
            N, dt = H * Wd, self.dt
            qq, kk, vv = qkv
            scale = float(np.float32(1.0) / np.sqrt(np.float32(Cc)))
            vt = self.emit("transpose", {}, [(B, 1, Cc, N)], lambda: op_transpose(vv.reshape(B, 1, N, Cc)))[0]
            sc = []
            for b in range(B):
                kb = kk[0 if (b and self.hit("keys_of_item_0")) else b].reshape(N, Cc)
                was = self.pending_mut
                sc.append(self.emit("attn_gemm", {}, [(1, H, Wd, N)], lambda: op_attn_gemm(qq[b:b + 1], kb, scale, dt))[0])
                if was:
                    self.mutated(sc[-1])
            scores = torch.cat(sc).reshape(B, N, 1, N)
            pr = self.emit("softmax_rows", {}, [(B, N, 1, N)], lambda: op_softmax_rows(scores, dt))[0]
            outs = []
            for b in range(B):
                vb = vt[0 if (b and self.hit("vt_stale")) else b, 0]
                was = self.pending_mut
                outs.append(self.emit("attn_gemm", {}, [(1, H, Wd, Cc)], lambda: op_attn_gemm(pr[b].reshape(1, H, Wd, N), vb, 1.0, dt))[0])
                if was:
                    self.mutated(outs[-1])
            a = torch.cat(outs)
            return self.conv(a, None, None, 0, p + ".NIN_3.W", p + ".NIN_3.b", Cc, res=x, scale=SQRT1_2, tap=f"attn.{idx}")

        def fn():
            r = op_attn_core(*(v.reshape(B, H * Wd, Cc) for v in qkv), self.dt)[0]
            return [(r[0].reshape(B, H, Wd, Cc), (lambda got: r[1](got.reshape(B, H * Wd, Cc))), r[2].reshape(B, H, Wd, Cc))]
        a = self.emit("attn_core", {}, [(B, H, Wd, Cc)], fn)[0]
        return self.conv(a, None, None, 0, p + ".NIN_3.W", p + ".NIN_3.b", Cc, res=x, scale=SQRT1_2, tap=f"attn.{idx}")

    # -- run_temb, run_score, Fwd::run --
    def run(self):
        sd, dt, pcp, pc = self.sd, self.dt, self.pcp, self.pc
        x, y, y2, t = _inputs(self.variant)
        self.part_count = {}
        L = len(self.ch_mult)
        # module indices as the reference numbers them (ncsnpp.py:181-316)
        m = 3 if self.cond else 1
        m_in = m
        m += 1
        # res-block indices and dense rows, in forward order (the order the engine lays out the Dense_0 rows)
        plan, mm, in_ch, hs_c = [], m, NF, [NF]
        for lvl in range(L):
            for _ in range(NRB):
                plan.append((mm, self.ch_mult[lvl] * NF)); mm += 1; hs_c.append(self.ch_mult[lvl] * NF)
            if lvl != L - 1:
                plan.append((mm, self.ch_mult[lvl] * NF)); mm += 2; hs_c.append(self.ch_mult[lvl] * NF)
        plan.append((mm, hs_c[-1])); mm += 2
        plan.append((mm, hs_c[-1])); mm += 1
        for lvl in reversed(range(L)):
            for _ in range(NRB + 1):
                plan.append((mm, self.ch_mult[lvl] * NF)); mm += 1
            mm += 2
            if lvl != 0:
                plan.append((mm, self.ch_mult[lvl] * NF)); mm += 1
        self.dense_row, r0 = {}, 0
        for idx, oc in plan:
            self.dense_row[idx] = r0; r0 += oc
        if self.cond:
            names = {"w": "all_modules.0.W", "x0": "all_modules.1.weight", "x1": "all_modules.1.bias", "x2": "all_modules.2.weight", "x3": "all_modules.2.bias"}

            def temb_fn():
                silu, bound = op_temb(t, sd, names)
                st_silu = silu if dt is None else silu.float().double()
                Wd = torch.cat([_par(sd, f"all_modules.{i}.Dense_0.weight") for i, _ in plan])
                bd = torch.cat([_par(sd, f"all_modules.{i}.Dense_0.bias") for i, _ in plan])
                ref, bnd = dense_reference(st_silu, Wd, bd)
                return [(ref, (lambda got: _worst0(got, ref, bnd)), ref if dt is None else ref.float().double()),
                        (silu, (lambda got: _worst0(got, silu, bound)), st_silu)]
            self.tembias = self.emit("temb", names, [(NB, 1, 1, r0), (NB, 1, 1, 4 * NF)], temb_fn)[0].reshape(NB, -1)
        xs = [_cplx(v) if v is not None else None for v in (x, y, y2)]

        def pack_fn():
            v = pack_reference(xs[0].reshape(-1, 2), None if xs[1] is None else xs[1].reshape(-1, 2), None if xs[2] is None else xs[2].reshape(-1, 2))
            if dt is None:                                    # (the unrounded walk: 2 v - 1 in float64, as the oracle; pack_input itself is fp32)
                v = torch.cat([u.reshape(-1, 2).double() if u is not None else torch.full((NB * self.nfreq * self.tp, 2), 0.5, dtype=torch.float64)
                               for u in (xs[:2] if pcp == 4 else xs + [None])], -1) * 2.0 - 1.0
            v = v.double().reshape(NB, self.nfreq, self.tp, pcp)
            return [(v, (lambda got: 0.0 if torch.equal(got.double(), v) else float("inf")), v)]
        x4 = self.emit("pack_input", {}, [(NB, self.nfreq, self.tp, pcp)], pack_fn, tap="x4")[0]
        hs = [self.conv(x4, None, None, 0, f"all_modules.{m_in}.weight", f"all_modules.{m_in}.bias", NF, parts=self.in_parts(), tap="h_in")]
        ipyr = x4
        in_ch = NF
        for lvl in range(L):
            oc = self.ch_mult[lvl] * NF
            for _ in range(NRB):
                hs.append(self.resblock(hs[-1], None, m, in_ch, oc)); m += 1; in_ch = oc
            if lvl != L - 1:
                B, H, Wd, _ = ipyr.shape
                src = ipyr
                ipyr = self.emit("fir_down", {}, [None, (B, H // 2, Wd // 2, pcp)], lambda: op_fir(src, None, 0, 0, 0 if dt is not None else None, (False, True)))[1]
                cbn = f"all_modules.{m + 1}.Conv_0"
                if pcp == 4:
                    hs.append(self.resblock(hs[-1], None, m, in_ch, in_ch, down=True, pyr=ipyr, cb=cbn))
                else:
                    o = self.resblock(hs[-1], None, m, in_ch, in_ch, down=True)
                    B2, H2, W2, C2 = o.shape
                    pin, params = ipyr, {"cb_w": cbn + ".weight", "cb_b": cbn + ".bias"}

                    def comb_fn():
                        ref, part = op_combine(o.reshape(B2, H2 * W2, C2), pin.reshape(B2, H2 * W2, pcp), sd, params, dt)
                        ref, part = ref.reshape(o.shape), part.reshape(o.shape)
                        return [(ref, (lambda got: _ratio(got, ref, part, self.store)), q(ref, dt))]
                    o = self.emit("combine_add", params, [tuple(o.shape)], comb_fn, tap=f"block.{m}")[0]
                    hs.append(o)
                m += 2
        hc = self.resblock(hs[-1], None, m, in_ch, in_ch); m += 1
        hc = self.attention(hc, m); m += 1
        hc = self.resblock(hc, None, m, in_ch, in_ch); m += 1
        pyr = None
        for lvl in reversed(range(L)):
            oc = self.ch_mult[lvl] * NF
            for k in range(NRB + 1):
                if lvl == L - 1 and k == 0 and self.hit("skip_swap"):   # the two skips of the coarsest level (same shape) in each other's place
                    hs[-1], hs[-2] = hs[-2], hs[-1]
                sk = hs.pop()
                hc = self.resblock(hc, sk, m, in_ch + sk.shape[-1], oc); m += 1; in_ch = oc
            gn = f"all_modules.{m}"; m += 1
            wn = f"all_modules.{m}"
            up = None
            if pyr is not None:
                B, H, Wd, _ = pyr.shape
                src = pyr
                up = self.emit("fir_up", {}, [None, (B, 2 * H, 2 * Wd, pcp)], lambda: op_fir(src, None, 0, 1, 0 if dt is not None else None, (False, True)))[1]
            pyr = self.conv(hc, None, gn, 1, wn + ".weight", wn + ".bias", pcp, res=up, odt=0, tap=f"pyramid.{m}")
            m += 1
            if lvl != 0:
                hc = self.resblock(hc, None, m, in_ch, in_ch, up=True); m += 1
        assert not hs
        B, H, Wd, _ = pyr.shape
        names = {"w": "output_layer.weight", "b": "output_layer.bias"}
        tt = t if (t is not None and not _is_refine(self.variant)) else None
        final = pyr
        self.out = self.emit("score_out", names, [(B, H, Wd, 2)], lambda: [
            (r[0].reshape(B, H, Wd, 2), (lambda got: r[1](got.reshape(B, H * Wd, 2))), r[2].reshape(B, H, Wd, 2))
            for r in op_score_out(final.reshape(B, H * Wd, pcp), tt, sd, names, self.sign, None if dt is None else 0)])[0]

    def in_parts(self):
        """partial totals of the input convolution on a large map: conv_in_split writes one per 8 x 16 tile"""
        return ((self.nfreq + 7) // 8) * ((self.tp + 15) // 16) if (self.dt in (1, 2) and self.pcp == 4 and self.nfreq * self.tp > self.gn_inline) else 1

    def listing(self):
        return [(l["kind"], tuple(sorted(l["params"].items())), tuple(l["shapes"])) for l in self.layers]


@functools.lru_cache(maxsize=None)
def _walk(variant, dt, gn_inline=GN_INLINE_DEFAULT, compute=True):
    return Walk(variant, dt, gn_inline, compute, sign=1.0 if _is_refine(variant) else -1.0)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU part
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_walk_without_rounding_is_the_oracle(variant):
    """float64 against float64 (fp32 weights widened): the output and every tap to 1e-9 of the maximum."""
    w = _walk(variant, None)
    out, taps = _oracle(variant)
    sign = 1.0 if _is_refine(variant) else -1.0
    worst = {"out": float((w.out - sign * out).abs().max() / out.abs().max())}
    for name, v in w.taps.items():
        want = taps[name]
        worst[name] = float((v[..., :want.shape[-1]] - want).abs().max() / want.abs().max())
        if v.shape[-1] > want.shape[-1]:
            assert float(v[..., want.shape[-1]:].abs().max()) == 0.0, name
    must = {"x4", "h_in"} | {k for k in taps if "." in k}
    assert must <= set(w.taps), must - set(w.taps)
    print(f"[walk] {variant}: {len(w.layers)} layers, {len(w.taps)} taps, worst |walk - oracle| / max: {max(worst.values()):.2e} ({max(worst, key=worst.get)})")
    assert max(worst.values()) < 1e-9, worst


@pytest.mark.parametrize("dt", [0, 1, 2])
def test_rounded_walk_holds_every_layer_bound_and_the_end_to_end_bound(dt):
    """The emulation is inside its own bounds by construction (each layer stores the rounding of its reference); end to end it lands where
    the engine does: under 5e-4 (fp32) / lp.fwd_bound of the oracle's maximum."""
    w = _walk("score", dt, 1024)
    out, _ = _oracle("score")
    for i, l in enumerate(w.layers):
        for r, o in zip(l["res"], l["outs"]):
            if r is not None and r[1] is not None:
                assert r[1](o) <= 1.0, (i, l["kind"], l["params"])
    err = float((w.out + out).abs().max() / out.abs().max())
    bound = 5e-4 if dt == 0 else lp.fwd_bound(DT_NAME[dt], 1.25)
    print(f"[walk] score {DT_NAME[dt]} rounded at every store: end-to-end |err| / max {err:.3e} (bound {bound:.3e})")
    assert err < bound


MUTANTS = ("eps", "partial", "inv_n", "temb_row", "scale_before_res", "shortcut_src", "combine_bias", "fir_act_raw", "skip_swap")
LONG_MUTANTS = ("keys_of_item_0", "vt_stale")              # the GEMM form of the attention core: item 1 on item 0's keys / on item 0's slice of vt
MUTANT_SETS = {"score": (1024, MUTANTS), "refine_long": (GN_INLINE_DEFAULT, LONG_MUTANTS)}


@pytest.mark.parametrize("dt", [1, 2])
def test_mutation_controls(dt):
    """One layer wrong at a time in the rounded walk (workload-like options: partial totals exist).  At its layer every mutant exceeds
    the per-element bound; end to end (printed, not asserted) most of them stay under lp.fwd_bound - what the existing tests allow."""
    _mutation_controls("score", dt)


@pytest.mark.parametrize("dt", [1, 2])
def test_mutation_controls_long_attention(dt):
    """The same for the GEMM form of the attention core, on the two-level refine generator (end to end: lp.refine_bound)."""
    _mutation_controls("refine_long", dt)


def _mutation_controls(variant, dt):
    gn_inline, names = MUTANT_SETS[variant]
    base = _walk(variant, dt, gn_inline)
    out, _ = _oracle(variant)
    sign = 1.0 if _is_refine(variant) else -1.0
    mx = float(out.abs().max())
    e2e0 = float((base.out - sign * out).abs().max()) / mx
    bound = (lp.refine_bound if _is_refine(variant) else lp.fwd_bound)(DT_NAME[dt], 1.25)      # (inputs other than the fixture's: factor 1.25, tests/lowprec.py)
    print(f"[mut] {variant} {DT_NAME[dt]}: unmutated end-to-end {e2e0:.3e} = {e2e0 / bound:.2f} x the end-to-end bound ({bound:.3e})")
    bad = []
    for name in names:
        w = Walk(variant, dt, gn_inline, mut=name, base=base, sign=sign)
        assert w.mut_layer is not None, name
        i, ratio = w.mut_layer, w.mut_ratio                    # (a wrong input tensor: at the first convolution that reads it)
        e2e = float((w.out - sign * out).abs().max()) / mx
        lay = w.layers[i]
        print(f"[mut] {DT_NAME[dt]} {name:17s} at layer {i:2d} ({lay['kind']} {lay['params'].get('w', lay['params'].get('gn_w', ''))}): |err| / bound {ratio:9.2f} | "
              f"end to end {e2e:.3e} = {e2e / bound:.2f} x the bound -> {'MISSED' if e2e < bound else 'caught'} by the end-to-end bound")
        if not ratio > 1.0:
            bad.append((name, ratio))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------
# GPU part
# ---------------------------------------------------------------------------------------------------------------------------
def _set_option(name, value):
    from universal_speech_enhancement_amd import hip_engine
    hip_engine.set_option(name, value)


def _fetch(e, tens):
    """A traced tensor (ptr, dims, dtype) -> host tensor in its storage type [B,H,W,C]"""
    ptr, dims, dtc = tens
    n = int(np.prod(dims))
    raw = torch.from_numpy(e.read_device(ptr, n, "<f4" if dtc == 0 else "<u2").copy())
    if dtc == 1:
        raw = raw.view(torch.bfloat16)
    elif dtc == 2:
        raw = raw.view(torch.float16)
    return raw.reshape(*dims)


def _fetch_i64(e, ptr, shape):
    return torch.from_numpy(e.read_device(ptr, int(np.prod(shape)), "<i8").copy()).reshape(*shape)


def _engine(variant, prec):
    from universal_speech_enhancement_amd.hip_engine import HipScoreEngine
    v = VARIANTS[variant]
    ch_mult, nfreq, _ = _geom(variant)
    e = HipScoreEngine(nf=NF, ch_mult=ch_mult, num_res_blocks=NRB, n_freq=nfreq, precision=prec, input_channels=v["input_channels"],
                       conditional=v["conditional"], scale_by_sigma=v["conditional"])
    e.load_state_dict(_state_dict(variant))
    return e


@functools.lru_cache(maxsize=None)
def _case(variant, prec, optset):
    """One evaluation with the trace on: (trace entries with every named tensor copied to the host, output [B,F,T,2], device inputs)."""
    x, y, y2, t = _inputs(variant)
    try:
        for k, val in OPTSETS[optset].items():
            _set_option(k, val)
        _set_option("trace", 1)
        e = _engine(variant, prec)
        dx = [None if a is None else a.cuda().contiguous() for a in (x, y, y2)]
        if _is_refine(variant):
            out = e.forward(dx[0])
        else:
            out = e.score(dx[0], dx[1], t.cuda(), dx[2])
        torch.cuda.synchronize()
        tr = e.trace()
        evin = {a.data_ptr(): n for a, n in zip(dx, ("x", "y", "y2")) if a is not None}
        for ent in tr:
            ent["in_t"] = [None if s is None else _fetch(e, s) for s in ent["in"]]
            ent["out_t"] = [None if s is None else _fetch(e, s) for s in ent["out"]]
            B = next(s for s in ent["in"] + ent["out"] if s is not None)[1][0]
            cs = [s[1][3] if s is not None else 0 for s in ent["in"][:2]]
            ent["totals_in_t"] = [None if not p else _fetch_i64(e, p, (B, c, 2)) for p, c in zip(ent["totals_in"], cs)]
            ent["part_in_t"] = [None if not p else _fetch_i64(e, p, (B, n, c, 2)) for p, n, c in zip(ent["part_in"], ent["parts_in"], cs)]
            co = ent["out"][0][1][3] if ent["out"][0] is not None else 0
            ent["totals_out_t"] = None if not ent["totals_out"] else _fetch_i64(e, ent["totals_out"], (B, co, 2))
            ent["part_out_t"] = None if not ent["part_out"] else _fetch_i64(e, ent["part_out"], (B, ent["parts_out"], co, 2))
            cin = sum(cs)
            ent["coef_t"] = None if not ent["coef"] else torch.from_numpy(e.read_device(ent["coef"], B * cin * 2, "<f4").copy()).reshape(B, cin, 2)
            ent["coef_out_t"] = None if not ent["coef_out"] else torch.from_numpy(e.read_device(ent["coef_out"], B * cin * 2, "<f4").copy()).reshape(B, cin, 2)
            if ent["tembias"]:
                rows = e.read_device(ent["tembias"], (B - 1) * ent["temb_stride"] + ent["temb_row"] + co, "<f4").copy()
                ent["temb_t"] = torch.stack([torch.from_numpy(rows[b * ent["temb_stride"] + ent["temb_row"]:][:co]) for b in range(B)])
            ent["t_t"] = None if not ent["t"] else torch.from_numpy(e.read_device(ent["t"], (B - 1) * max(ent["t_stride"], 0) + 1, "<f4").copy())[::max(ent["t_stride"], 1)]
        expected = e.expected_weights()
        e.close()
    finally:
        _set_option("trace", 0)
        for k, val in OPTSETS["default"].items():
            _set_option(k, val)
    return dict(trace=tr, out=_cplx(out.cpu()), evin=evin, expected=expected)


def _summed(ent, k):
    """The totals of input k a consumer reads: int64 [B,C,2], partial totals summed over their parts"""
    if ent["part_in_t"][k] is not None:
        return ent["part_in_t"][k].sum(1)
    return ent["totals_in_t"][k]


@pytest.mark.gpu
@pytest.mark.parametrize("variant,prec,optset", CASES, ids=CASE_IDS)
def test_every_launch_holds_its_bound(variant, prec, optset):
    c = _case(variant, prec, optset)
    tr, sd, dt = c["trace"], _state_dict(variant), PREC[prec]
    kernels = {e["kernel"] for e in tr}
    kinds = [e["kind"] for e in tr]
    # the kernels the case is meant to reach did run
    if variant in LONG:                                        # (no map of at most 320 pixels: conv_sk takes nothing in 16-bit storage)
        assert {"transpose_nc", "softmax_rows"} <= kernels and not kernels & {"attention", "attn_fused"}, kernels
        assert kinds.count("attn_gemm") == 2 * NB and kinds.count("transpose") == 1 and kinds.count("softmax_rows") == 1
        assert ({"conv_sk", "conv_in"} <= kernels) if dt == 0 else ("conv_v2" in kernels and "conv_sk" not in kernels), kernels
    elif dt == 0:
        assert {"conv_sk", "conv_in", "attention"} <= kernels, kernels
    else:
        assert "attn_fused" in kernels and "conv_sk" in kernels, kernels
        if optset == "default":
            assert "conv_v2" in kernels and "gn_finalize_part" not in kernels and not any(e["part_out"] for e in tr), kernels
        else:
            assert kernels & {"conv_v4", "conv_v5"} and "gn_finalize_part" in kernels, kernels
            assert any(e["part_out"] for e in tr), "no launch wrote partial totals"
    if optset == "workload":
        assert any(e["kind"] == "conv" and e["coef"] for e in tr), "no convolution read a coefficient array"
    else:
        assert not any(e["kind"] == "conv" and e["coef"] for e in tr)
    assert ("combine_add" in kinds) == (variant == "both") and ("temb" in kinds) == (not _is_refine(variant))
    combined = {e["out"][0][0]: e for e in tr if e["kind"] == "combine_add"}
    worst = {}

    def note(kind, r):
        worst[kind] = max(worst.get(kind, 0.0), r)
    for e in tr:
        kind, p, ins, outs = e["kind"], e["params"], e["in_t"], e["out_t"]
        if kind == "temb":
            silu, bound = op_temb(e["t_t"], sd, p)
            note("temb_mlp", _worst0(outs[1].reshape(silu.shape), silu, bound))
            silu_st = outs[1].reshape(silu.shape)
            for u in tr:                                       # the table, by the rows the convolutions read
                if u["kind"] == "conv" and u["tembias"]:
                    ref, bnd = dense_reference(silu_st, _par(sd, u["params"]["dense_w"]), _par(sd, u["params"]["dense_b"]))
                    assert u["tembias"] == e["out"][0][0] and u["temb_stride"] == e["out"][0][1][3]
                    note("temb_dense", _worst0(u["temb_t"], ref, bnd))
        elif kind == "pack_input":
            want = pack_reference(ins[0].reshape(-1, 2), None if ins[1] is None else ins[1].reshape(-1, 2), None if ins[2] is None else ins[2].reshape(-1, 2))
            note("pack_input", 0.0 if torch.equal(outs[0].reshape(want.shape), want) else float("inf"))
        elif kind == "conv":
            x = _cat(ins[0].double(), None if ins[1] is None else ins[1].double())
            B, H, Wd, cin = x.shape
            coef = None
            if e["coef"]:
                coef = e["coef_t"].double()
                assert e["gn_groups"] == 0
            elif e["gn_groups"]:
                groups = min(cin // 4, 32)
                assert e["gn_groups"] == groups and e["gn_eps"] == float(np.float32(GN_EPS)), (e["gn_groups"], e["gn_eps"])
                assert e["gn_inv_n"] == float(np.float32(1.0) / (np.float32(cin // groups) * np.float32(H * Wd)))
                assert e["part_in"][0] is None and e["part_in"][1] is None
                tot = torch.cat([_summed(e, k) for k in (0, 1) if ins[k] is not None], 1)
                coef = gn_coef_from_totals(tot, _par(sd, p["gn_w"]), _par(sd, p["gn_b"]), groups, H * Wd)
            cout, odt = outs[0].shape[-1], e["out"][0][2]
            a = dict(params=p, x=x, xs=None if ins[2] is None else _cat(ins[2].double(), None if ins[3] is None else ins[3].double()),
                     res=None if ins[4] is None else ins[4].double(), pyr=None if ins[5] is None else ins[5].double(), coef=coef,
                     temb=e.get("temb_t"), act=e["act"], scale=e["out_scale"], cout=cout, odt=odt, in_dt=e["in"][0][2])
            assert e["ntaps"] == (1 if ".NIN_" in p["w"] or ".Conv_2" in p["w"] else 9)
            ref, bound, _ = conv_eval(a, sd, dt)
            got = outs[0].double()
            assert bool(torch.isfinite(got).all())
            name = "conv:" + e["kernel"]
            if e["out"][0][0] in combined:                     # rewritten in place by combine_add: both launches against the stored result
                u = combined[e["out"][0][0]]
                pyr = u["in_t"][5].double()
                r2, part2 = op_combine(ref.reshape(B, H * Wd, cout), pyr.reshape(B, H * Wd, -1), sd, u["params"], dt)
                b2 = UNIT[odt] * r2.abs() + part2 + (2.0 ** -25 if odt == 2 else 0.0) + bound.reshape(r2.shape)
                note(name + "+combine_add", _worst0(got.reshape(r2.shape), r2, b2))
                continue
            note(name, _worst0(got, ref, bound))
            stats = e["part_out_t"].sum(1) if e["part_out_t"] is not None else e["totals_out_t"]
            if stats is not None:
                if cin in (4, 8) and e["ntaps"] == 9:
                    n_ser, n_sq = _n_ser(e["kernel"], odt, 1)
                    note("totals:" + e["kernel"], _totals_ratio(stats, outs[0], n_ser, n_sq, ((H + 7) // 8) * ((Wd + 15) // 16)))
                else:
                    note("totals:" + e["kernel"], _check_stats(stats, outs[0], odt, e["kernel"]))
        elif kind in ("fir_down", "fir_up"):
            coef = e["coef_t"].double() if e["coef"] else None
            res = op_fir(ins[0].double(), coef, e["act"], kind == "fir_up", e["in"][0][2], (outs[0] is not None, outs[1] is not None))
            for r, o in zip(res, outs):
                if r is not None:
                    note(kind + ("" if coef is not None else ":pyramid"), r[1](o))
        elif kind == "gn_finalize":
            tot = torch.cat([_summed(e, k) for k in (0, 1) if e["in"][k] is not None], 1)
            B, H, Wd, _ = e["in"][0][1]
            groups = min(tot.shape[1] // 4, 32)
            assert e["gn_groups"] == groups and e["gn_eps"] == float(np.float32(GN_EPS))
            note(e["kernel"], op_finalize(tot, sd, p, groups, H * Wd)[0][1](e["coef_out_t"]))
        elif kind == "attn_fused":
            B, H, Wd, Cc = ins[0].shape
            coef = gn_coef_from_totals(e["totals_in_t"][0], _par(sd, p["gn_w"]), _par(sd, p["gn_b"]), 32, H * Wd)
            r = op_attn_fused(ins[0].double().reshape(B, H * Wd, Cc), coef, sd, p, dt)[0]
            note("attn_fused", r[1](outs[0].reshape(B, H * Wd, Cc)))
            note("totals:attn_fused", _fused_totals_ratio(e["totals_out_t"], outs[0].reshape(B, H * Wd, Cc), dt))
        elif kind == "attn_core":
            B, H, Wd, Cc = ins[0].shape
            r = op_attn_core(*(v.double().reshape(B, H * Wd, Cc) for v in ins[:3]), dt)[0]
            note("attention", r[1](outs[0].reshape(B, H * Wd, Cc)))
        elif kind == "transpose":
            assert e["in"][0][1][2:] == e["out"][0][1][:1:-1] and e["in"][0][0] == next(u for u in tr if u["params"].get("w", "").endswith(".NIN_2.W"))["out"][0][0]
            note("transpose_nc", op_transpose(ins[0].double())[0][1](outs[0]))
        elif kind == "attn_gemm":
            _, H, Wd, K = ins[0].shape
            cout = outs[0].shape[-1]
            assert e["ntaps"] == 1 and e["act"] == 0 and ins[1].shape == (1, 1, cout, K) and not e["params"], (e["ntaps"], e["act"], ins[1].shape)
            is_scores = K != H * Wd
            assert e["kernel"] == expected_kernels(dt, H * Wd, cout if K == H * Wd else K)[0 if is_scores else 1], e["kernel"]
            if is_scores:
                # the softmax has rewritten this launch's output: the launch again through use_op_conv on the operands it read (as
                # tests/test_hip_attention_gemm.py does), tied to the engine's own by the softmax entry below (bit for bit)
                assert e["out_scale"] == float(np.float32(1.0) / np.sqrt(np.float32(K)))
                got = _score_gemm(ins[0].cuda(), ins[1][0, 0].double(), H, Wd, dt).cpu().reshape(1, H, Wd, cout)
                e["scores_t"] = got
            else:
                assert e["out_scale"] == 1.0
                got = outs[0]
            note("attn_gemm:" + ("scores" if is_scores else "pv"), op_attn_gemm(ins[0].double(), ins[1][0, 0].double(), e["out_scale"], dt)[0][1](got))
        elif kind == "softmax_rows":
            from test_hip_forward_kernels import _lib, _ok, _p, _stream
            B, N = outs[0].shape[:2]
            assert e["in"][0] == e["out"][0]
            gem = [u for u in tr if u["kind"] == "attn_gemm" and "scores_t" in u]
            es = 4 if dt == 0 else 2
            assert [u["out"][0][0] for u in gem] == [e["out"][0][0] + b * N * N * es for b in range(B)], "the score GEMMs do not write the items' slices of this buffer"
            scores = torch.cat([u["scores_t"] for u in gem]).reshape(B, N, 1, N)
            d = scores.cuda().contiguous()
            _ok(_lib().lib().use_op_softmax_rows(_p(d), dt, B * N, N, _stream()), "use_op_softmax_rows")
            torch.cuda.synchronize()
            assert torch.equal(d.cpu(), outs[0]), "the score GEMMs through use_op_conv do not reproduce the engine's probabilities bit for bit"
            note("softmax_rows", op_softmax_rows(scores.double(), dt)[0][1](outs[0]))
        elif kind == "combine_add":
            B, H, Wd, Cc = outs[0].shape
            note("totals:combine_add", _combine_totals_ratio(e["totals_out_t"], outs[0].reshape(B, H * Wd, Cc), H * Wd))
        elif kind == "score_out":
            B, H, Wd, pcq = ins[0].shape
            assert (e["t"] is None or e["t"] == 0) == _is_refine(variant) and e["out_scale"] == (1.0 if _is_refine(variant) else -1.0)
            r = op_score_out(ins[0].double().reshape(B, H * Wd, pcq), e["t_t"], sd, p, e["out_scale"])[0]
            note("score_out", r[1](outs[0].reshape(B, H * Wd, 2)))
            assert torch.equal(outs[0].reshape(c["out"].shape), c["out"]), "the traced output is not what the evaluation returned"
        else:
            raise AssertionError(kind)
    print(f"[measured] {variant}-{prec}-{optset}: {len(tr)} launches | " + " ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert all(v <= 1.0 for v in worst.values()), {k: v for k, v in worst.items() if not v <= 1.0}
    # end to end, as the existing tests hold it
    out, _ = _oracle(variant)
    sign = 1.0 if _is_refine(variant) else -1.0
    err = float((c["out"].double() - sign * out).abs().max() / out.abs().max())
    print(f"[measured] {variant}-{prec}-{optset}: end-to-end |err| / max {err:.3e}")
    assert err < (5e-4 if dt == 0 else (lp.refine_bound(prec, 1.25) if _is_refine(variant) else lp.fwd_bound(prec, 1.25)))


@pytest.mark.gpu
@pytest.mark.parametrize("variant,prec,optset", CASES, ids=CASE_IDS)
def test_trace_is_the_walks_layer_list(variant, prec, optset):
    """Kind, parameter names and output shapes of every launch, in order."""
    tr = _case(variant, prec, optset)["trace"]
    def shapes(e):
        if e["kind"] == "gn_finalize":
            return (tuple(e["coef_out_t"].shape), None)
        return tuple(None if s is None else tuple(s[1]) for s in e["out"])
    got = [(e["kind"], tuple(sorted(e["params"].items())), shapes(e)) for e in tr]
    w = _walk(variant, PREC[prec], OPTSETS[optset]["gn_inline"], False)
    want = [(k, p, tuple(s) + (None,) * (2 - len(s))) for k, p, s in w.listing()]
    assert len(got) == len(want), (len(got), len(want), [g[0] for g in got], [x[0] for x in want])
    for i, (g, x) in enumerate(zip(got, want)):
        assert g == x, (i, g, x)


def _labels(c):
    """Trace -> (label per entry, {label: labels of what it reads}) with the finalise launches dropped and the attention block collapsed."""
    tr = c["trace"]
    writer = dict((p, "input:" + n) for p, n in c["evin"].items())
    graph, nfir, spans = {}, {}, []

    def source(s, sliced):
        """the label of what wrote the tensor at s[0]; sliced (the per-item GEMMs of the long attention): of the tensor s lies inside"""
        if s[0] in writer or not sliced:
            return writer[s[0]]
        return next(lab for lo, hi, lab in spans if lo <= s[0] < hi)
    for e in tr:
        p = e["params"]
        attn = e["kind"] in ("attn_fused", "attn_core", "transpose", "attn_gemm", "softmax_rows") or ".NIN_" in p.get("w", "")
        if e["kind"] == "gn_finalize":
            continue
        if attn:
            label = "attn"
        elif e["kind"] in ("fir_down", "fir_up"):
            src = writer[e["in"][0][0]]
            label = f"{e['kind']}({src})"
        else:
            label = e["kind"] + ":" + p.get("w", p.get("cb_w", ""))
        srcs = tuple(None if s is None else source(s, e["kind"] == "attn_gemm") for s in e["in"])
        if attn:
            srcs = tuple(s for s in srcs if s is not None and not s.startswith("attn"))
            graph[label] = tuple(sorted(set(graph.get(label, ()) + srcs)))
        else:
            assert label not in graph, label
            graph[label] = srcs
        for k, s in enumerate(e["out"]):
            if s is not None:
                writer[s[0]] = label + (f"[{k}]" if e["kind"] in ("fir_down", "fir_up") else "")
                spans.append((s[0], s[0] + int(np.prod(s[1])) * (4 if s[2] == 0 else 2), writer[s[0]]))
    return graph


@pytest.mark.gpu
def test_wiring_graph_is_the_same_in_every_mode():
    graphs = {(p, o): _labels(_case("score", p, o)) for p in ("fp32", "bf16", "fp16") for o in ("default", "workload")}
    first = graphs[("fp32", "default")]
    assert len(first) > 30
    for k, g in graphs.items():
        assert g == first, (k, {n: (g.get(n), first.get(n)) for n in set(g) | set(first) if g.get(n) != first.get(n)})
    # the GEMM form of the attention core collapses to the same node: one "attn" that reads the block in front of it and nothing else
    longs = {p: _labels(_case("refine_long", p, "default")) for p in ("fp32", "bf16", "fp16")}
    for k, g in longs.items():
        assert g == longs["fp32"], (k, {n: (g.get(n), longs["fp32"].get(n)) for n in set(g) | set(longs["fp32"]) if g.get(n) != longs["fp32"].get(n)})
    assert len(longs["fp32"]["attn"]) == 1 and longs["fp32"]["attn"][0].startswith("conv:") and len(first["attn"]) == 1, (longs["fp32"]["attn"], first["attn"])


@pytest.mark.gpu
@pytest.mark.parametrize("variant,prec,optset", CASES, ids=CASE_IDS)
def test_trace_is_complete(variant, prec, optset):
    c = _case(variant, prec, optset)
    written = dict((p, -1) for p in c["evin"])
    used, wcount = set(), {}
    spans, nwrites = [], {}                                    # (byte range of every written tensor; writes per buffer of the long attention)
    nbytes = lambda s: int(np.prod(s[1])) * (4 if s[2] == 0 else 2)

    def inside(s):
        """a per-item slice (the GEMMs of the long attention): wholly inside one tensor an earlier launch wrote"""
        return any(lo <= s[0] and s[0] + nbytes(s) <= hi for lo, hi in spans)
    for i, e in enumerate(c["trace"]):
        if e["kind"] != "gn_finalize":                         # (a finalise launch names the maps whose totals it reads, and reads the totals alone)
            for s in e["in"]:
                assert s is None or s[0] in written or (e["kind"] == "attn_gemm" and inside(s)), (i, e["kind"], "reads what no earlier launch wrote")
        for s in e["out"]:
            if s is not None:
                assert s[0] not in written or e["kind"] in ("combine_add", "softmax_rows"), (i, e["kind"], "a second writer")
                assert e["kind"] in ("combine_add", "softmax_rows") or not any(lo < s[0] + nbytes(s) and s[0] < hi for lo, hi in spans), (i, e["kind"], "overlaps a written tensor")
                written[s[0]] = i
                spans.append((s[0], s[0] + nbytes(s)))
        if e["kind"] == "softmax_rows":                        # in place: every item's slice written once (its score GEMM) and rewritten here, once
            lo, hi = e["out"][0][0], e["out"][0][0] + nbytes(e["out"][0])
            B, N = e["out"][0][1][:2]
            gem = [u["out"][0] for u in c["trace"][:i] if u["kind"] == "attn_gemm" and lo <= u["out"][0][0] < hi]
            assert sorted(g[0] for g in gem) == [lo + b * (hi - lo) // B for b in range(B)] and all(nbytes(g) == (hi - lo) // B for g in gem), "sc is not written once"
            assert not any(u["kind"] == "attn_gemm" and lo <= u["out"][0][0] < hi for u in c["trace"][i + 1:]), "sc is written after the softmax"
            nwrites["sc"] = nwrites.get("sc", 0) + 1
        if e["kind"] == "transpose":
            nwrites["vt"] = nwrites.get("vt", 0) + 1
            lo, hi = e["out"][0][0], e["out"][0][0] + nbytes(e["out"][0])
            readers = [u for u in c["trace"][i + 1:] if u["kind"] == "attn_gemm" and lo <= u["in"][1][0] < hi]
            B = e["out"][0][1][0]
            assert [u["in"][1][0] for u in readers] == [lo + b * (hi - lo) // B for b in range(B)], "the P.V GEMMs do not read the items' slices of vt"
        for tot, part in zip(e["totals_in"], e["part_in"]):     # (given partial totals the launch reads those, not the totals pointer beside them)
            assert not (part or tot) or (part or tot) in written, (i, e["kind"], "totals nobody wrote")
        for tot in (e["totals_out"], e["part_out"], e["coef_out"]):
            if tot:
                written[tot] = i
        assert not e["coef"] or e["coef"] in written
        used |= set(e["params"].values())
        for role in ("w", "w2", "cb_w", "x0", "x2", "x4"):
            n = e["params"].get(role)
            if n and e["kind"] in ("conv", "attn_fused", "combine_add", "score_out"):
                wcount[n] = wcount.get(n, 0) + 1
    assert nwrites == ({"sc": 1, "vt": 1} if variant in LONG else {}), nwrites
    expected = set(c["expected"])
    if _is_refine(variant):                                    # unconditional: the module list has them, no launch reads them
        unused = expected - used
        assert unused == {"all_modules.0.W"} | {n for n in expected if ".Dense_0." in n}, unused
        expected -= unused
    assert used == expected, used ^ expected
    weights = {n for n, s in c["expected"].items() if (len(s) == 4 or n.endswith(".W")) and n != "all_modules.0.W"}
    assert {n for n in weights if wcount.get(n, 0) != 1} == set(), {n: wcount.get(n, 0) for n in weights if wcount.get(n, 0) != 1}


@pytest.mark.gpu
@pytest.mark.parametrize("variant,optset", [("score", "default"), ("score", "workload"), ("refine", "default"), ("refine_long", "default")])
def test_fp32_traced_outputs_are_the_oracles_taps(variant, optset):
    c = _case(variant, "fp32", optset)
    _, taps = _oracle(variant)
    seen = set()
    for e in c["trace"]:
        w = e["params"].get("w", "")
        name = None
        if e["kind"] == "pack_input":
            name = "x4"
        elif e["kind"] == "conv" and (w.endswith(".Conv_1.weight") or w.endswith(".NIN_3.W")):
            name = ("block." if "Conv_1" in w else "attn.") + w.split(".")[1]
        elif e["kind"] == "conv" and w.count(".") == 2 and e["out"][0][2] == 0 and e["out_t"][0].shape[-1] in (4, 8) and e["in"][0][1][3] > 8:
            name = "pyramid." + w.split(".")[1]
        elif e["kind"] == "conv" and e["in"][0][1][3] in (4, 8):
            name = "h_in"
        if name is None:
            continue
        want = taps[name]
        got = e["out_t"][0].double()
        err = float((got[..., :want.shape[-1]] - want).abs().max() / want.abs().max())
        assert err < 5e-4, (name, err)
        seen.add(name)
    assert seen == {k for k in taps if k in ("x4", "h_in") or "." in k}, seen


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
def test_trace_changes_no_bit_and_is_empty_when_off(prec):
    for variant in ("score", "refine_long"):
        x, y, _, t = _inputs(variant)
        on = _case(variant, prec, "default")["out"]
        e = _engine(variant, prec)
        off = _cplx((e.forward(x.cuda()) if _is_refine(variant) else e.score(x.cuda(), y.cuda(), t.cuda())).cpu())
        assert e.trace() == [], variant
        e.close()
        assert torch.equal(on, off), variant


@pytest.mark.gpu
def test_long_attention_on_a_secondary_stream_is_bit_identical():
    """bf16, four items: 2 + 2 sub-batches (the second runs the GEMM form on its own stream and in its own arena) against the same batch
    unsplit, and its items 0 / 1 against the two-item evaluation of the cases above."""
    from universal_speech_enhancement_amd.testing import noise as tn
    x = _inputs("refine_long")[0]
    x4 = torch.cat([x, torch.from_numpy(tn.complex_normal(78, "x", tuple(x.shape))) * 0.5]).cuda().contiguous()
    outs = {}
    try:
        for n in (-1, 0):
            _set_option("subbatch", n)
            e = _engine("refine_long", "bf16")
            outs[n] = _cplx(e.forward(x4).cpu())
            e.close()
    finally:
        _set_option("subbatch", -1)
    assert torch.equal(outs[-1], outs[0]), "2 + 2 sub-batches differ from the unsplit batch"
    assert torch.equal(outs[-1][:NB], _case("refine_long", "bf16", "default")["out"]), "items 0 / 1 of the four differ from the two-item evaluation"
    assert not torch.equal(outs[-1][:NB], outs[-1][NB:])
