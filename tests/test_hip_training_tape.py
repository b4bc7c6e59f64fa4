"""The training tape (universal_speech_enhancement_amd/training.py: four torch.autograd.Functions on the HIP operators and the torch glue
between them) call by call against float64, in fp32, bf16 and fp16 - the level between tests/test_hip_backward_kernels.py (every backward
kernel alone) and tests/test_hip_training.py (loss.backward() of the whole network against the reference's goldens, in 16 bits only to
the reference's own autocast error of a percent).  Recorder, checker, mirror and emulation are in tests/training_tape_ref.py.

Recording.  training.py looks up conv / gn_act / fir / attn_core and the eight launches (training._conv_dev; training_ops.conv_wgrad,
colsum, gn_act_fwd, gn_act_bwd, fir, attention_core, attention_core_bwd) as module attributes at call time; the test replaces them by
recording subclasses (whose forward / backward call the parents' unchanged) and by wrappers that note the operands each launch really
got, after the casts, under the call that issued it.  A call index on ctx ties a backward to its forward.  Records keep the tensors
themselves with a checksum each; at the end every checksum still holds (nothing on the tape writes in place), and loss and every .grad
are bit-equal with and without the recorders.  One tensor is scratch by design, the front of the GroupNorm workspace, where forward and
backward kernels both put their partial sums: of the workspace the statistics behind it, which the backward reuses, are held to their
checksum (the first GPU run said so: the checksum of the whole workspace moved, in every precision).

Per call.  Every element of every output of every call against the float64 reference of that one operation on the operands as stored,
held to the bound that operation has in its per-kernel file (imported: conv_reference / nin_reference with _bound, dgrad_reference with
_conv_part, wgrad_reference with wgrad_dispatch's K, colsum_reference, gn_reference, fir_reference, attention_reference,
attention_bwd_reference).  What the tape adds, and its bounds:
  * every launch operand is, bit for bit, the call's operand or the cast the tape is meant to make of it ('*.operands' checks): x rounded
    to 16 bits for the weight gradient of an fp32-input / 16-bit-output convolution, gy rounded to 16 bits in front of the data and weight
    gradients of a 16-bit-input / fp32-output one, q, k, v, dO widened (exact), the forward's workspace handed to the GroupNorm backward;
    weight mode 0 / 1 / 2, ntaps, alpha = scale, FIR direction;
  * gw is the NIN transpose / view(w.shape) of the launch's dw and gb its db, bit for bit; g_temb the colsum launch's output;
  * g_res = gy * scale: one product, stored once: u |ref| (fp16 below 2^-14: 2^-25);
  * the FIR adjoint is 4 down(g) / up(g) / 4: u |f raw| + f part; in fp16 the kernel's own store is 2^-25 absolute below 2^-14, which the
    gain 4 carries on as 4 x 2^-25, and a product by 1/4 that lands below 2^-14 rounds once more: (1 + 1/4) 2^-25;
  * dq, dk, dv as returned: the fp32 result (part + 2^-24 |ref|) stored once, and bit-equal to the launch's output cast;
  * the mixed-type ends, on the UNCAST operands ('*.uncast'): a cast operand is g (1 + d), |d| <= u_in, and both gradients are linear in
    it, so |sum g^ w - sum g w| <= u_in sum |g| |w| = u_in S: the launch's bound plus u_in S of the cast operand (for gb only where gy
    is the cast one).  This pins what the ends compute, not only that the kernel computed it.

Wiring and glue: a float64 mirror.  The network once more, following oracle/ncsnpp_oracle.py, in float64 on the CPU with a pass-through
Function at every operator boundary: forward returns the stored HIP output of the k-th call of that kind (matched by parameter name
where there is one), backward compares the gy the mirror's glue computed from the HIP gradients of its consumers with the recorded gy
and returns the recorded input gradients.  Three more backward passes over the same graph give the bound, per element: |gradients| in
place of the gradients give S = sum |terms|; ones give n, the number of terms; and a pass that injects 1 at the division by t gives e,
the fp32 roundings of the glue itself.  torch accumulates a fan-out in the storage type, one rounding per addition, each relative to a
partial sum of at most S; cat, views, slices and the sum nodes' own backward are exact:
    |gy - ref| <= ((n - 1) u + e 2^-24) S.
With one consumer that is 0: the gy must be the consumer's gradient bit for bit.  The root (d loss / d out of |out - target|^2 mean): |d|
2 ulps, 2 |d| / N two roundings, d / |d| and the product three: 8 x 2^-24 |g|.  Forward, each boundary's operand as the mirror's glue
computes it from the stored outputs upstream is held to one rounding, u |x| (2 x - 1, the Combine sum, the pyramid sum; cat and views are
exact), the output layer's to two (the pyramid sum, then / t: the first CPU run of the emulation measured 1.83 against one rounding,
which had forgotten the second operation).  The torch-only gradients (time-embedding MLP, Dense_0) are computed by hand in float64 from the recorded g_temb of every
Conv_0; forward values and their fp32 bounds as temb_reference derives them, every GEMM C_ACC 2^-24 sqrt(K) S + 2^-24 |ref| (K = B for the
parameter gradients, Cout and 4 nf for the data gradients, summed over the consumers of temb) plus what the fp32 forward values and the
upstream gradients carry in (|G|^T d_act + e_G^T |act|; SiLU' through _act_grad, |silu''| <= 1/2).  Each parameter has exactly one
producing call; its .grad is that call's output, or the leading slice of it for the zero-padded end weights, bit for bit;
all_modules.0.W has none; every call has a boundary and every boundary a call.

Cases.  A: conditional, nf 32, ch_mult (1, 2), one res-block per level (plain, widening, down, up and cat blocks, Combine, 32 -> 64
channels, 96 tokens of 64 channels), input [2, n, 16, 24] with n = 2 and 3, t = (0.35, 0.9).  B: the discriminative generator form
(unconditional, no division by t), ch_mult (1, 1, 2), input [3, 1, 16, 8]: two pyramid up-FIRs, two Combine sums, 8 tokens.  Each in fp32,
bf16 and fp16; the call sequences of the three are identical apart from dtypes; a second forward + backward gives the same bits
(wgrad_kernel with atomic slices would be exempt and named; the dispatcher picks it nowhere here: channels are multiples of 32).

CPU controls (-m "not gpu").  The emulation (training.py's own Functions and helpers over float64 launches stored once in the storage
type, the torch glue in the storage type on the CPU) holds every bound, and each deliberately wrong tape exceeds the bound of the check
named with it: g_res without the scale (conv.g_res), data gradient with the unflipped weight (conv.gx), NIN gw not transposed
(conv.gw.layout), FIR adjoint gains swapped (fir.bwd), GroupNorm backward with the statistics of eps 1e-5 (gn.dx), a skip gradient dropped
at one fan-out, cat halves swapped, the pyramid gradient divided by t[0] for every item (mirror.gy), alpha missing on Conv_1's weight
gradient (conv.gw).  Exempt by arithmetic, each printed with its reason: g_temb without the scale inside the network (temb goes to Conv_0
alone, whose scale is 1: shown on a single call with scale 1 / sqrt 2 instead); eps 1e-5 in 16 bits where 4.5e-6 / var, the relative
change of rstd, stays below the storage rounding (printed; it must be caught in fp32); t[0] for every item needs B > 1, distinct t and
scale_by_sigma.  Each mutant also prints where its parameter gradients land against today's end-to-end bounds (lowprec.train_bound with
the factors of tests/test_hip_training.py; fp32: 6e-6 on norms, 2.5e-5 of the maximum).

Measured on the MI355X, worst |err| / bound over the three networks, fp32 / bf16 / fp16 (`pytest -s` prints one [measured] line per
check family and case): conv.fwd 0.30 / 0.994 / 0.989, conv.gx 0.41 / 0.47 / 0.46 (uncast - / 0.39 / 0.36), conv.gw 0.54 / 0.21 / 0.23
(uncast - / 0.47 / 0.50), conv.gb 0.26 / 0.06 / 0.06 (uncast - / 0.11 / 0.09), conv.g_temb 0.15 / 0.14 / 0.19, conv.g_res 0.998 / 0.93 /
0.98 (one rounding: u |ref| itself), gn.fwd 0.30 / 0.996 / 0.994, gn.dx 0.19 / 0.995 / 0.988, gn.dgamma / dbeta 0.18 / 0.09 / 0.07, fir.fwd
0.53 / 0.996 / 0.999, fir.bwd 0.54 / 0.996 / 0.997, attn.fwd 0.04 / 0.985 / 0.953, attn dq / dk / dv 0.02 / 0.02 / 0.03 (as stored - / 0.98 /
0.87), mirror.gy and mirror.fwd 0.9996 .. 0.99999 (a single rounding of the glue at the bottom of a binade; every boundary with one
consumer and no glue operation is exact), temb.grad 0.26, temb.dense below 0.001 (the bound allows the fp32 sine of an argument of 300 what
the library does not use); every '*.operands' and 'layout' check exact.  No bug was found in training.py or the kernels, and
wgrad_kernel is picked nowhere.  Mutant factors (network A, n = 2; fp32 / bf16 / fp16): g_res 7e6 / 106 / 848, unflipped weight 7e5 / 328 /
2.6e3, NIN gw inf (an equality), FIR gains 5e7 / 1.8e6 / 1.8e6, eps 50 / 7.9 / 9.2, dropped skip 5.6e6 / 85 / 683, cat halves 3.5e9 / 3.8e4 /
4.6e5, alpha 2e5, t[0] 2.6e7, g_temb on the single call 1.5e6 / 2e6 / 2e6; against today's end-to-end bounds on the same small network
every one of them is over as well, the eps mutant by the least (5.9 x the bf16 norm bound, 28 x the tensor bound).  Run time: CPU part
20 s (40 tests), GPU part 10 s (39 tests).  No bound in this
file was fitted to a measurement; the two corrections named above (the second glue rounding in front of the output layer, the scratch
front of the GroupNorm workspace) each follow from reading the code the measurement pointed at."""
import functools

import pytest
import torch

import lowprec as lp
import training_tape_ref as R
from universal_speech_enhancement_amd.testing import noise as tnoise
from universal_speech_enhancement_amd.testing import weights as tw

PREC = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
NETS = {
    "A2": dict(arch=dict(nf=32, ch_mult=(1, 2), num_res_blocks=1, input_channels=4), shape=(2, 2, 16, 24), t=(0.35, 0.9), conditional=True),
    "A3": dict(arch=dict(nf=32, ch_mult=(1, 2), num_res_blocks=1, input_channels=6), shape=(2, 3, 16, 24), t=(0.35, 0.9), conditional=True),
    "B": dict(arch=dict(nf=32, ch_mult=(1, 1, 2), num_res_blocks=1, input_channels=2, conditional=False), shape=(3, 1, 16, 8), t=(1.0, 1.0, 1.0),
              conditional=False),
}
CASES = [(n, p) for n in NETS for p in PREC]
TORCH_ONLY = ("all_modules.1.", "all_modules.2.", ".Dense_0.")


def _inputs(net, device="cpu"):
    c = NETS[net]
    sd = tw.make_state_dict(100 + len(net) + ord(net[0]), **c["arch"])
    P = {k: torch.from_numpy(v.copy()).to(device).requires_grad_(k != "all_modules.0.W") for k, v in sd.items()}
    B = c["shape"][0]
    x = torch.from_numpy(tnoise.complex_normal(31, "tape_x_" + net, c["shape"])).to(device) * 0.5
    target = torch.from_numpy(tnoise.complex_normal(32, "tape_y_" + net, (B, 1) + c["shape"][2:])).to(device)
    return P, x, torch.tensor(c["t"], dtype=torch.float32, device=device), target


def _step(forward, P, x, t, target, net, prec, **kw):
    c = NETS[net]
    for p in P.values():
        p.grad = None
    out = forward(P, x, t, c["arch"]["ch_mult"], c["arch"]["num_res_blocks"], conditional=c["conditional"], scale_by_sigma=c["conditional"],
                  compute_dtype=PREC[prec], **kw)
    loss = (out - target).abs().square().mean()
    loss.backward()
    return loss.detach(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in P.items()}


def _expected(net, P):
    return {k for k in P if k != "all_modules.0.W" and (NETS[net]["conditional"] or ".Dense_0." not in k)}


def _mirror(tape, P, x, t, target, net):
    c = NETS[net]
    cpu = lambda v: v.detach().cpu()
    return R.run_mirror(tape, {k: cpu(v) for k, v in P.items()}, cpu(x), cpu(t), cpu(target), c["arch"]["ch_mult"], c["arch"]["num_res_blocks"],
                        c["conditional"], c["conditional"])


def _report(tag, results):
    fam = {}
    for _, _, c, v in results:
        fam[c] = max(fam.get(c, 0.0), v)
    for c in sorted(fam):
        print(f"[measured] training tape {tag} {c}: worst |err| / bound {fam[c]:.3f}")
    bad = [(i, n, c, v) for i, n, c, v in results if not v < 1.0]
    assert not bad, bad[:12]


def _grad_checks(net, tape, producers, P, grads):
    """every trained parameter's .grad is the output of exactly one call, bit for bit (or its leading slice); no other has a gradient"""
    exp = _expected(net, P)
    only = TORCH_ONLY if NETS[net]["conditional"] else ()              # unconditional: all_modules.1 is the input convolution
    for k in P:
        assert (grads[k] is not None) == (k in exp), k
    for k in sorted(exp):
        if any(s in k for s in only):
            assert k not in producers
            if ".Dense_0." in k:                                       # fed by the g_temb of exactly one Conv_0
                feeders = [r for r in tape.calls if r["kind"] == "conv" and r["temb"] is not None and r["name"] == k.split(".Dense_0.")[0] + ".Conv_0"]
                assert len(feeders) == 1 and feeders[0]["g_temb"] is not None, k
            continue
        assert len(producers.get(k, ())) == 1, (k, producers.get(k))
        idx, field = producers[k][0]
        out = tape.calls[idx][field]
        assert out is not None and torch.equal(out[tuple(slice(0, s) for s in grads[k].shape)], grads[k]), (k, idx, field)
    assert set(producers) == {k for k in exp if not any(s in k for s in only)}


# ---------------------------------------------------------------------------------------------------------------------------
# CPU controls: the emulation and the deliberately wrong tapes
# ---------------------------------------------------------------------------------------------------------------------------
def _t_gres(rec, ctx, gy, o):
    if o[5] is None or rec["scale"] == 1.0:
        return o
    return o[:5] + (gy.to(o[5].dtype),) + o[6:]


def _t_nin(rec, ctx, gy, o):
    return o if rec["w"].dim() != 2 else (o[0], o[1].t().contiguous()) + o[2:]


def _t_fir(rec, ctx, gy, o):
    return (o[0] * (1.0 / 16.0 if rec["up"] else 16.0), None)


# name: (what, launch mutation, tamper, glue mutation, the check that must exceed its bound, kinds to check (None: the mirror))
MUTANTS = {
    "g_res_without_scale": (None, {"conv": _t_gres}, None, "conv.g_res", ("conv",)),
    "dgrad_unflipped_weight": ("unflipped", None, None, "conv.gx", ("conv",)),
    "nin_gw_not_transposed": (None, {"conv": _t_nin}, None, "conv.gw.layout", ("conv",)),
    "fir_adjoint_gains_swapped": (None, {"fir": _t_fir}, None, "fir.bwd", ("fir",)),
    "gn_backward_eps_1e-5": ("gn_eps", None, None, "gn.dx", ("gn",)),
    "skip_gradient_dropped": (None, None, "drop_skip", "mirror.gy", None),
    "cat_halves_swapped": (None, None, "cat_swapped", "mirror.gy", None),
    "alpha_missing_on_conv1_wgrad": ("no_alpha", None, None, "conv.gw", ("conv",)),
    "pyramid_gradient_over_t0": (None, None, "div_t0", "mirror.gy", None),
}


def _emulate(net, prec, launch_mut=None, tamper=None, glue_mut=None):
    P, x, t, target = _inputs(net)
    tape = R.Tape(tamper)
    R.LAUNCH_MUT["v"] = launch_mut
    try:
        with pytest.MonkeyPatch.context() as mp:
            R.install_emulation(mp)
            R.install(mp, tape)
            loss, grads = _step(R.emu_forward_train, P, x, t, target, net, prec, glue_mut=glue_mut)
    finally:
        R.LAUNCH_MUT["v"] = None
    producers = R.name_calls(tape, P)
    return dict(tape=tape, P=P, x=x, t=t, target=target, loss=loss, grads=grads, producers=producers)


@functools.lru_cache(maxsize=None)
def _emu_base(net, prec):
    return _emulate(net, prec)


@pytest.mark.parametrize("net,prec", CASES)
def test_emulated_tape_holds_every_bound(net, prec):
    """The float64 emulation with the storage roundings through the same checker, mirror and completeness assertions as the GPU tape."""
    e = _emu_base(net, prec)
    tape = e["tape"]
    assert tape.unchanged()
    results = R.check_tape(tape)
    mres, loss64 = _mirror(tape, e["P"], e["x"], e["t"], e["target"], net)
    results += mres
    if NETS[net]["conditional"]:
        results += R.temb_checks(tape, {k: v.detach() for k, v in e["P"].items()}, e["t"], e["grads"])
    assert all(r.get("checked") and (r.get("mirrored")) for r in tape.calls)
    assert abs(float(e["loss"]) - loss64) <= 1e-5 * loss64
    _grad_checks(net, tape, e["producers"], e["P"], e["grads"])
    _report(f"emulation {net} {prec}", results)


def test_emulated_call_sequences_are_identical_across_precisions():
    for net in NETS:
        sigs = [R.signature(_emu_base(net, p)["tape"]) for p in PREC]
        assert sigs[0] == sigs[1] == sigs[2], net
        assert len(sigs[0]) > 40


def _landing(prec, base, grads):
    """the mutant's parameter gradients against the emulation's, as multiples of today's end-to-end bounds"""
    wn = wt = wm = 0.0
    for k, g in grads.items():
        b = base[k]
        if b is None or g is None or float(b.abs().max()) == 0:
            continue
        b, g = b.double(), g.double()
        wn = max(wn, abs(float(g.norm()) - float(b.norm())) / float(b.norm()))
        wt = max(wt, float((g - b).norm()) / float(b.norm()))
        wm = max(wm, float((g - b).abs().max()) / float(b.abs().max()))
    if prec == "fp32":
        return wn / 6e-6, wm / 2.5e-5
    return wn / lp.train_bound(prec, "norm_rel_max", 1.25), wt / lp.train_bound(prec, "tensor_rell2_max", 1.5)


@pytest.mark.parametrize("prec", list(PREC))
@pytest.mark.parametrize("name", list(MUTANTS))
def test_deliberately_wrong_tape_exceeds_its_bound(name, prec):
    launch_mut, tamper, glue_mut, check, kinds = MUTANTS[name]
    net = "A2"
    c = NETS[net]
    if name == "pyramid_gradient_over_t0":                            # arithmetic: invisible with one item, equal t or no division by t
        assert c["shape"][0] > 1 and len(set(c["t"])) > 1 and c["conditional"]
    base = _emu_base(net, prec)
    m = _emulate(net, prec, launch_mut, tamper, glue_mut)
    if kinds is None:
        results, _ = _mirror(m["tape"], m["P"], m["x"], m["t"], m["target"], net)
    else:
        results = R.check_tape(m["tape"], kinds)
    factor = R.worst(results, check)
    others = sorted({ck for _, _, ck, v in results if not v < 1.0 and not ck.startswith(check)})
    norm_x, tensor_x = _landing(prec, base["grads"], m["grads"])
    print(f"[measured] mutant {name} {prec}: {check} {factor:.3g} x its bound (also over: {', '.join(others) or 'none'}); end to end: gradient norms "
          f"{norm_x:.3g} x today's bound, tensors {tensor_x:.3g} x -> {'over' if max(norm_x, tensor_x) >= 1 else 'UNDER'} the end-to-end bounds on this network")
    if name == "gn_backward_eps_1e-5" and prec != "fp32" and not factor > 1.0:
        var = min(float(r["x"].double().reshape(r["x"].shape[0], -1, r["groups"], r["x"].shape[3] // r["groups"]).var((1, 3), unbiased=False).min())
                  for r in m["tape"].calls if r["kind"] == "gn")
        print(f"[exempt] {name} {prec}: rstd moves by 4.5e-6 / var <= {4.5e-6 / var:.2g} (smallest group variance {var:.3g}), below the storage "
              f"rounding {R.UNIT[R.DTC[PREC[prec]]]:.2g}; caught in fp32")
        assert 4.5e-6 / var < R.UNIT[R.DTC[PREC[prec]]]
        return
    assert factor > 1.0, (name, prec, factor)


@pytest.mark.parametrize("prec", list(PREC))
def test_g_temb_without_the_scale_on_a_single_call(prec):
    """Inside the network temb goes to Conv_0 alone, whose scale is 1: 'g_temb without the scale' changes nothing there (asserted).  One
    recorded call with temb, a residual and scale 1 / sqrt 2 shows the check."""
    assert all(r["scale"] == 1.0 for r in _emu_base("A2", prec)["tape"].calls if r["kind"] == "conv" and r["temb"] is not None)
    print("[exempt] g_temb_without_scale in the network: every convolution that takes temb has scale 1")
    from universal_speech_enhancement_amd import training as T
    g = torch.Generator().manual_seed(5)
    dt = PREC[prec]
    x = torch.randn(2, 6, 5, 32, generator=g).to(dt).requires_grad_(True)
    w = (torch.randn(64, 32, 3, 3, generator=g) / 17.0).requires_grad_(True)
    b = torch.randn(64, generator=g).mul(0.1).requires_grad_(True)
    temb = torch.randn(2, 64, generator=g).requires_grad_(True)
    res = torch.randn(2, 6, 5, 64, generator=g).to(dt).requires_grad_(True)
    gy = (torch.randn(2, 6, 5, 64, generator=g) + 0.3).to(dt)
    factors = []
    for mut in (None, "colsum_scale"):
        tape = R.Tape()
        R.LAUNCH_MUT["v"] = mut
        try:
            with pytest.MonkeyPatch.context() as mp:
                R.install_emulation(mp)
                R.install(mp, tape)
                T.conv(x, w, b, None, temb, res, 0.70710678118654752440).backward(gy)
        finally:
            R.LAUNCH_MUT["v"] = None
        results = R.check_tape(tape)
        factors.append(R.worst(results, "conv.g_temb"))
        if mut is None:
            assert R.worst(results) < 1.0, results
    print(f"[measured] mutant g_temb_without_scale {prec} (single call): conv.g_temb {factors[1]:.3g} x its bound")
    assert factors[0] < 1.0 < factors[1]


# ---------------------------------------------------------------------------------------------------------------------------
# GPU part
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gpu_case(net, prec):
    """One plain forward + backward, two recorded ones; shared by the tests of a case and left unchanged."""
    from universal_speech_enhancement_amd import training as T
    P, x, t, target = _inputs(net, "cuda")
    loss0, grads0 = _step(T.ncsnpp_forward_train, P, x, t, target, net, prec)
    runs = []
    for _ in range(2):
        tape = R.Tape()
        with pytest.MonkeyPatch.context() as mp:
            R.install(mp, tape)
            loss, grads = _step(T.ncsnpp_forward_train, P, x, t, target, net, prec)
        torch.cuda.synchronize()
        runs.append((tape, loss, grads))
    tape, loss, grads = runs[0]
    producers = R.name_calls(tape, P)
    R.name_calls(runs[1][0], P)
    return dict(tape=tape, tape2=runs[1][0], P=P, x=x, t=t, target=target, loss=loss, grads=grads, loss0=loss0, grads0=grads0, producers=producers)


@pytest.mark.gpu
@pytest.mark.parametrize("net,prec", CASES)
def test_recording_moves_no_bit_and_nothing_writes_in_place(net, prec):
    e = _gpu_case(net, prec)
    assert torch.equal(e["loss"], e["loss0"]) and bool(torch.isfinite(e["loss"]))
    for k, g in e["grads0"].items():
        assert (g is None) == (e["grads"][k] is None) and (g is None or torch.equal(g, e["grads"][k])), k
    assert not e["tape"].changed() and not e["tape2"].changed()
    assert len(e["tape"].calls) > 40 and all(r["launches"] for r in e["tape"].calls)


@pytest.mark.gpu
@pytest.mark.parametrize("net,prec", CASES)
def test_every_call_matches_its_float64_reference(net, prec):
    e = _gpu_case(net, prec)
    results = R.check_tape(e["tape"])
    assert all(r.get("checked") for r in e["tape"].calls)
    exempt = [(r["idx"], r["name"]) for r in e["tape"].calls if r.get("wgrad_kernel", ("", 1))[0] == "wgrad_kernel" and r["wgrad_kernel"][1] > 1]
    assert not exempt, exempt                                          # channels are multiples of 32: the tiled kernels everywhere
    _report(f"{net} {prec}", results)


@pytest.mark.gpu
@pytest.mark.parametrize("net,prec", CASES)
def test_wiring_and_glue_match_the_float64_mirror(net, prec):
    e = _gpu_case(net, prec)
    tape = e["tape"]
    results, loss64 = _mirror(tape, e["P"], e["x"], e["t"], e["target"], net)
    assert all(r.get("mirrored") for r in tape.calls), "a recorded call has no boundary in the mirror"
    assert abs(float(e["loss"]) - loss64) <= 1e-5 * loss64, (float(e["loss"]), loss64)
    grads = {k: (None if g is None else g.cpu()) for k, g in e["grads"].items()}
    if NETS[net]["conditional"]:
        results += R.temb_checks(tape, {k: v.detach().cpu() for k, v in e["P"].items()}, e["t"].cpu(), grads)
    _grad_checks(net, tape, e["producers"], e["P"], e["grads"])
    _report(f"{net} {prec}", results)


@pytest.mark.gpu
@pytest.mark.parametrize("net", list(NETS))
def test_call_sequence_is_identical_across_precisions(net):
    sigs = [R.signature(_gpu_case(net, p)["tape"]) for p in PREC]
    assert sigs[0] == sigs[1] == sigs[2]
    assert sigs[0] == R.signature(_emu_base(net, "fp32")["tape"]), "the emulated tape of the CPU controls is not the tape of the GPU"


@pytest.mark.gpu
@pytest.mark.parametrize("net,prec", CASES)
def test_second_run_gives_the_same_bits(net, prec):
    """The tiled weight-gradient kernels, the sliced GroupNorm and colsum have no atomics: a second forward + backward repeats every
    recorded output.  (wgrad_kernel with atomic slices: its gw / gb alone would be exempt, and printed.)"""
    e = _gpu_case(net, prec)
    assert len(e["tape"].calls) == len(e["tape2"].calls)
    if not any("wgrad_kernel" in r for r in e["tape"].calls):            # which weight-gradient kernel each call took (set by the checker)
        R.check_tape(e["tape"], ("conv",))
    for a, b in zip(e["tape"].calls, e["tape2"].calls):
        assert (a["kind"], a["name"]) == (b["kind"], b["name"])
        atomic = a.get("wgrad_kernel", ("", 1))[0] == "wgrad_kernel" and a["wgrad_kernel"][1] > 1
        for f in R.CALL_OUTPUTS[a["kind"]] + ("gy",):
            if atomic and f in ("gw", "gb"):
                print(f"[exempt] call {a['idx']} {a['name']}: wgrad_kernel with {a['wgrad_kernel'][1]} atomic slices, {f} not compared")
                continue
            u, v = a.get(f), b.get(f)
            assert (u is None) == (v is None) and (u is None or torch.equal(u, v)), (a["idx"], a["name"], f)
