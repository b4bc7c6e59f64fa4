"""Recording, checking and mirroring of the training tape (universal_speech_enhancement_amd/training.py) for
tests/test_hip_training_tape.py, which carries the derivations.  Nothing here needs a GPU: the recorder wraps whatever functions
``training`` holds at the time, the checker and the mirror work on the records as stored (moved to the CPU), and the emulation replaces
the eight launches of the tape by the float64 references of the per-kernel test files rounded once to the storage type.

Every reference and every bound of a launch is imported from tests/test_hip_conv_kernels.py, tests/test_hip_forward_kernels.py and
tests/test_hip_backward_kernels.py; none is restated."""
import inspect
import math

import numpy as np
import torch
import torch.nn.functional as F

from test_hip_conv_kernels import UNIT, _bound, conv_reference
from test_hip_forward_kernels import C_ACC, U32, ULP_FN, _ratio, _silu, _silu_err, attention_reference, fir_reference
from test_hip_backward_kernels import (GN_MAX_SLICES, _act_grad, _colsum_chain, _conv_part, attention_bwd_reference, colsum_reference, dgrad_reference, gn_chain,
                                       gn_reference, nin_reference, wgrad_dispatch, wgrad_reference)

DTC = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
KINDS = ("conv", "gn", "fir", "attn")
LAUNCHES = ("conv_wgrad", "colsum", "gn_act_fwd", "gn_act_bwd", "fir", "attention_core", "attention_core_bwd")     # of training_ops; + training._conv_dev
CALL_OUTPUTS = {"conv": ("y", "gx", "gw", "gb", "g_temb", "g_res"), "gn": ("y", "gx", "dgamma", "dbeta"), "fir": ("y", "gx"), "attn": ("y", "dq", "dk", "dv")}
INF = float("inf")


def _training():
    from universal_speech_enhancement_amd import training, training_ops
    return training, training_ops


def checksum(t):
    """Position-weighted sum of the bytes of a tensor as stored."""
    b = t.detach().contiguous().view(-1).view(torch.uint8).to(torch.int64)
    return int((b * (torch.arange(b.numel(), device=b.device) % 8191 + 1)).sum())


# ---------------------------------------------------------------------------------------------------------------------------
# recording
# ---------------------------------------------------------------------------------------------------------------------------
class Tape:
    """One record per call of the four operators, in forward order.  Records keep the tensors themselves, each with the checksum it had
    when it was recorded.  ``tamper``: {kind: f(rec, ctx, gy, outs) -> outs}, the deliberately wrong tapes of the CPU controls."""

    def __init__(self, tamper=None):
        self.calls, self.kept, self.cur, self.phase, self.tamper = [], [], None, None, tamper or {}

    def keep(self, v, label=""):
        if torch.is_tensor(v):
            self.kept.append((label, v, checksum(v)))
        elif isinstance(v, (tuple, list)):
            for i, e in enumerate(v):
                self.keep(e, f"{label}[{i}]")
        return v

    def open(self, kind, **operands):
        rec = dict(idx=len(self.calls), kind=kind, launches=[], name=None, needs_bwd=any(torch.is_tensor(v) and v.requires_grad for v in operands.values()))
        rec.update({k: self.keep(v, f"call {rec['idx']} {kind} {k}") for k, v in operands.items()})
        self.calls.append(rec)
        self.cur, self.phase = rec, "fwd"
        return rec

    def reopen(self, idx, gy, ctx):
        rec = self.calls[idx]
        assert "gy" not in rec, f"call {idx} ran its backward twice"
        rec["gy"], rec["nig"] = self.keep(gy, f"call {idx} gy"), tuple(ctx.needs_input_grad)
        self.cur, self.phase = rec, "bwd"
        return rec

    def close(self, rec, **outs):
        rec.update({k: self.keep(v, f"call {rec['idx']} {rec['kind']} {k}") for k, v in outs.items()})
        self.cur = None

    def launch(self, op, named, out):
        assert self.cur is not None, f"{op} was launched outside a recorded call"
        lab = f"call {self.cur['idx']} {op} ({self.phase}) "
        if op in ("gn_act_fwd", "gn_act_bwd"):
            # the GroupNorm workspace is scratch in front (both kernels write their partial sums there) and statistics behind it
            # (use_op_gn_act_bwd: mean at 4 B GN_MAX_SLICES max(C, G), rstd B G further): the statistics are what the backward reuses
            work = out[1] if op == "gn_act_fwd" else named["fwd_work"]
            B, Cc, G = named["x"].shape[0], named["x"].shape[3], named["groups"]
            off = 4 * B * GN_MAX_SLICES * max(Cc, G)
            if work is not None and work.numel() >= off + 2 * B * G:
                self.kept.append((lab + "statistics", work.view(-1)[off:off + 2 * B * G], checksum(work.view(-1)[off:off + 2 * B * G])))
                named = {k: v for k, v in named.items() if k != "fwd_work"}
                self.cur["launches"].append(dict(op=op, phase=self.phase, out=(self.keep(out[0], lab + "y"), work) if op == "gn_act_fwd" else self.keep(out, lab + "out"),
                                                 fwd_work=work, **{k: self.keep(v, lab + k) for k, v in named.items()}))
                return
        self.cur["launches"].append(dict(op=op, phase=self.phase, out=self.keep(out, lab + "out"), **{k: self.keep(v, lab + k) for k, v in named.items()}))

    def changed(self):
        """Nothing on the tape writes in place: the recorded tensors that no longer have the checksum taken when they were recorded."""
        return [label for label, t, c in self.kept if checksum(t) != c]

    def unchanged(self):
        return not self.changed()


def install(mp, tape):
    """Replace training.conv / gn_act / fir / attn_core by the .apply of recording subclasses and wrap the eight launches (``mp``: a
    pytest MonkeyPatch).  The subclasses call the parents' forward / backward unchanged."""
    T, ops = _training()

    def wrap(mod, name):
        fn = getattr(mod, name)
        sig = inspect.signature(fn)

        def recorded(*a, **k):
            out = fn(*a, **k)
            b = sig.bind(*a, **k)
            b.apply_defaults()
            tape.launch(name, dict(b.arguments), out)
            return out
        mp.setattr(mod, name, recorded)
    wrap(T, "_conv_dev")
    for n in LAUNCHES:
        wrap(ops, n)

    def back(ctx, gy, parent, kind):
        rec = tape.reopen(ctx.tape_idx, gy, ctx)
        outs = parent.backward(ctx, gy)
        if kind in tape.tamper:
            outs = tape.tamper[kind](rec, ctx, gy, outs)
        return rec, outs

    class RConv(T._Conv):
        @staticmethod
        def forward(ctx, x, w, b, out_dtype=None, temb=None, res=None, scale=1.0):
            rec = tape.open("conv", x=x, w=w, b=b, out_dtype=out_dtype, temb=temb, res=res, scale=float(scale))
            y = T._Conv.forward(ctx, x, w, b, out_dtype, temb, res, scale)
            ctx.tape_idx = rec["idx"]
            tape.close(rec, y=y)
            return y

        @staticmethod
        def backward(ctx, gy):
            rec, o = back(ctx, gy, T._Conv, "conv")
            tape.close(rec, gx=o[0], gw=o[1], gb=o[2], g_temb=o[4], g_res=o[5])
            return o

    class RGNAct(T._GNAct):
        @staticmethod
        def forward(ctx, x, gamma, beta, groups, act):
            rec = tape.open("gn", x=x, gamma=gamma, beta=beta, groups=groups, act=act)
            y = T._GNAct.forward(ctx, x, gamma, beta, groups, act)
            ctx.tape_idx = rec["idx"]
            tape.close(rec, y=y)
            return y

        @staticmethod
        def backward(ctx, gy):
            rec, o = back(ctx, gy, T._GNAct, "gn")
            tape.close(rec, gx=o[0], dgamma=o[1], dbeta=o[2])
            return o

    class RFir(T._Fir):
        @staticmethod
        def forward(ctx, x, up):
            rec = tape.open("fir", x=x, up=bool(up))
            y = T._Fir.forward(ctx, x, up)
            ctx.tape_idx = rec["idx"]
            tape.close(rec, y=y)
            return y

        @staticmethod
        def backward(ctx, gy):
            rec, o = back(ctx, gy, T._Fir, "fir")
            tape.close(rec, gx=o[0])
            return o

    class RAttn(T._AttnCore):
        @staticmethod
        def forward(ctx, q, k, v):
            rec = tape.open("attn", q=q, k=k, v=v)
            y = T._AttnCore.forward(ctx, q, k, v)
            ctx.tape_idx = rec["idx"]
            tape.close(rec, y=y)
            return y

        @staticmethod
        def backward(ctx, gO):
            rec, o = back(ctx, gO, T._AttnCore, "attn")
            tape.close(rec, dq=o[0], dk=o[1], dv=o[2])
            return o

    for name, cls in (("conv", RConv), ("gn_act", RGNAct), ("fir", RFir), ("attn_core", RAttn)):
        mp.setattr(T, name, cls.apply)


def name_calls(tape, P):
    """Give every convolution and GroupNorm call the state-dict prefix of its parameters (by storage, or - the zero-padded end weights -
    by the values of the leading slice) and return {parameter name: (call index, field)}."""
    by_ptr = {p.data_ptr(): k for k, p in P.items()}
    producers = {}

    def add(name, idx, field):
        assert name in P, name
        producers.setdefault(name, []).append((idx, field))
    for r in tape.calls:
        if r["kind"] == "conv":
            w = r["w"]
            key = by_ptr.get(w.data_ptr())
            if key is None:
                hits = [k for k, p in P.items() if p.dim() == w.dim() and all(a <= b for a, b in zip(p.shape, w.shape)) and
                        torch.equal(w[tuple(slice(0, s) for s in p.shape)], p.detach())]
                assert len(hits) == 1, (r["idx"], hits)
                key = hits[0]
            r["name"], leaf = key.rsplit(".", 1)
            add(key, r["idx"], "gw")
            if r["b"] is not None:
                add(r["name"] + (".b" if leaf == "W" else ".bias"), r["idx"], "gb")
        elif r["kind"] == "gn":
            key = by_ptr[r["gamma"].data_ptr()]
            r["name"] = key.rsplit(".", 1)[0]
            add(key, r["idx"], "dgamma")
            add(by_ptr[r["beta"].data_ptr()], r["idx"], "dbeta")
    return producers


def signature(tape):
    """The call sequence without dtypes: kind, parameter, operand shapes, and per launch its name, weight mode and alpha / scale."""
    sig = []
    for r in tape.calls:
        shapes = tuple((k, tuple(v.shape)) for k, v in sorted(r.items()) if torch.is_tensor(v))
        ls = tuple((l["op"], l["phase"], l.get("w_mode"), l.get("ntaps"), l.get("alpha"), l.get("scale"), l.get("up"), l.get("act"), l.get("groups"))
                   for l in r["launches"])
        sig.append((r["kind"], r["name"], shapes, r.get("scale"), r.get("up"), r.get("act"), ls))
    return sig


# ---------------------------------------------------------------------------------------------------------------------------
# per-call checks
# ---------------------------------------------------------------------------------------------------------------------------
def _c(t):
    return None if t is None else t.detach().cpu()


def _same(a, b):
    """0 if the two tensors hold the same bits (same type and shape), else inf"""
    return 0.0 if (a is not None and b is not None and a.dtype == b.dtype and a.shape == b.shape and torch.equal(_c(a), _c(b))) else INF


def _abs_ratio(got, ref, bound):
    err = (_c(got).double() - ref).abs()
    r = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, INF), torch.zeros_like(err)))
    return float(r.max())


def _launches(rec, op, phase):
    return [l for l in rec["launches"] if l["op"] == op and l["phase"] == phase]


def _one(rec, op, phase):
    ls = _launches(rec, op, phase)
    assert len(ls) == 1, (rec["idx"], rec["kind"], op, phase, len(ls))
    return ls[0]


def check_conv(rec):
    res = []
    x, w, b, temb, rs, y = (_c(rec[k]) for k in ("x", "w", "b", "temb", "res", "y"))
    nin = w.dim() == 2
    ntaps = 1 if nin or w.shape[2] == 1 else 9
    cin, cout = (w.shape[0], w.shape[1]) if nin else (w.shape[1], w.shape[0])
    B, H, W, _ = x.shape
    dt, odt = DTC[x.dtype], DTC[y.dtype]
    sc = float(np.float32(rec["scale"]))
    wc = w.t() if nin else w                                          # the [Cout][Cin] form of the NIN matrix
    # ---- forward: one use_op_conv_dev on the operands of the call
    L = _one(rec, "_conv_dev", "fwd")
    ok = max(_same(L["x"], x), _same(L["w"], w), _same(L["out"], y), 0.0 if (L["w_mode"], L["ntaps"], L["cout"]) == (2 if nin else 0, ntaps, cout) else INF,
             0.0 if float(L["scale"]) == rec["scale"] else INF, 0.0 if (L["b"] is None) == (b is None) and (L["temb"] is None) == (temb is None) else INF,
             0.0 if temb is None else _same(L["temb"], temb.float()), 0.0 if rs is None else _same(L["res"], rs),
             0.0 if y.dtype == (rec["out_dtype"] or x.dtype) and (rs is None or rs.dtype == y.dtype) else INF)
    res.append(("conv.fwd.operands", ok))
    if nin:
        ref, S = nin_reference(x, w, dt)
        for v in (b, None if temb is None else temb[:, None, None, :], rs):
            if v is not None:
                ref, S = ref + v.double(), S + v.double().abs()
        ref = ref * sc
    else:
        ref, S = conv_reference(x, None, 0, w, dt, bias=b, temb=temb, res=rs, scale=sc)
    part = _bound(ref, S, dt, odt, sc, cin * ntaps) - UNIT[odt] * ref.abs()
    res.append(("conv.fwd", _ratio(y, ref, part, odt)))
    if "gy" not in rec:
        return res
    # ---- backward
    gy, nig = _c(rec["gy"]), rec["nig"]
    if rec["g_res"] is not None:
        g = _c(rec["g_res"])
        ref = gy.double() * sc                                        # one product, stored once
        res.append(("conv.g_res", INF if g.dtype != rs.dtype else _ratio(g, ref, torch.zeros_like(ref), DTC[g.dtype])))
    else:
        res.append(("conv.g_res", 0.0 if rs is None else INF))
    if rec["g_temb"] is not None:
        L = _one(rec, "colsum", "bwd")
        n_t = _colsum_chain(dict(work=True, C=cout, dt=DTC[gy.dtype], HW=H * W))[0]
        ref, part = colsum_reference(gy.reshape(B, H * W, cout), rec["scale"], n_t)
        res.append(("conv.g_temb", max(_ratio(_c(rec["g_temb"]), ref, part, 0), _same(L["x"], gy), _same(L["out"], rec["g_temb"]),
                                       0.0 if float(L["scale"]) == rec["scale"] else INF)))
    else:
        res.append(("conv.g_temb", 0.0 if temb is None else INF))
    # the operands the launches must have received: the mixed-type ends run their backward in the 16-bit type
    gl, xl = gy, x
    if gy.dtype != x.dtype:
        if x.dtype == torch.float32:
            xl = x.to(gy.dtype)
            assert not nig[0], "an fp32 input of a 16-bit convolution asked for a gradient"
        else:
            gl = gy.to(x.dtype)
    dl = DTC[gl.dtype]
    cast = gy.dtype != x.dtype
    if nig[0]:
        L = _one(rec, "_conv_dev", "bwd")
        ok = max(_same(L["x"], gl), _same(L["w"], w), _same(L["out"], rec["gx"]), 0.0 if L["b"] is None and L["temb"] is None and L["res"] is None else INF,
                 0.0 if (L["w_mode"], L["ntaps"], L["cout"], float(L["scale"])) == (0 if nin else 1, ntaps, cin, rec["scale"]) else INF)
        res.append(("conv.gx.operands", ok))
        gx = _c(rec["gx"])
        ref, s = dgrad_reference(gl, wc, dl, sc)
        res.append(("conv.gx", _ratio(gx, ref, _conv_part(s, cout * ntaps, dl), DTC[gx.dtype])))
        if cast:                                                      # on gy as received: + u_in S of the cast operand
            ref, s = dgrad_reference(gy, wc, dl, sc)
            res.append(("conv.gx.uncast", _ratio(gx, ref, _conv_part(s, cout * ntaps, dl) + UNIT[dl] * s, DTC[gx.dtype])))
    else:
        res.append(("conv.gx", 0.0 if rec["gx"] is None and not _launches(rec, "_conv_dev", "bwd") else INF))
    L = _one(rec, "conv_wgrad", "bwd")
    dw, db = L["out"]
    ok = max(_same(L["dy"], gl), _same(L["x"], xl), 0.0 if (L["ntaps"], float(L["alpha"]), bool(L["with_bias"])) == (ntaps, rec["scale"], b is not None) else INF)
    res.append(("conv.gw.operands", ok))
    kern, plan, K, Kb = wgrad_dispatch(dict(B=B, H=H, W=W, Cout=cout, Cin=cin, dt=dl, tiled=True, mfma16=1, blocks=0))
    rec["wgrad_kernel"] = (kern, plan["nslices"])
    rw, s, rb, sb = wgrad_reference(gl, xl, ntaps, rec["scale"])
    pw, pb = C_ACC * U32 * math.sqrt(K) * s, C_ACC * U32 * math.sqrt(Kb) * sb
    res.append(("conv.gw", _ratio(_c(dw).reshape(rw.shape), rw, pw, 0)))
    res.append(("conv.gw.layout", _same(rec["gw"], dw.t().contiguous() if nin else dw.view(w.shape))))
    if b is not None:
        res.append(("conv.gb", max(_ratio(_c(db), rb, pb, 0), _same(rec["gb"], db))))
    if cast:
        rw2, s2, rb2, sb2 = wgrad_reference(gy, x, ntaps, rec["scale"])
        u = UNIT[dl]
        res.append(("conv.gw.uncast", _ratio(_c(dw).reshape(rw2.shape), rw2, C_ACC * U32 * math.sqrt(K) * s2 + u * s2, 0)))
        if b is not None:
            res.append(("conv.gb.uncast", _ratio(_c(db), rb2, C_ACC * U32 * math.sqrt(Kb) * sb2 + (u * sb2 if gl is not gy else 0.0), 0)))
    return res


def check_gn(rec):
    x, gamma, beta, y = (_c(rec[k]) for k in ("x", "gamma", "beta", "y"))
    G, act = rec["groups"], rec["act"]
    B, H, W, Cc = x.shape
    dt = DTC[x.dtype]
    n_t = gn_chain(H * W, Cc, G, dt)[0]
    Lf = _one(rec, "gn_act_fwd", "fwd")
    res = [("gn.fwd.operands", max(_same(Lf["x"], x), _same(Lf["out"][0], y), 0.0 if (Lf["groups"], Lf["act"], bool(Lf["return_work"])) == (G, act, True) else INF,
                                   0.0 if abs(Lf["eps"] - 1e-6) < 1e-12 else INF))]
    gy = _c(rec["gy"]) if "gy" in rec else None
    o = gn_reference(x.reshape(B, H * W, Cc), None if gy is None else gy.reshape(B, H * W, Cc), None, gamma, beta, G, act, 1.0, n_t)
    res.append(("gn.fwd", _ratio(y.reshape(B, H * W, Cc), o["y"], o["d_y"], dt)))
    if gy is None:
        return res
    Lb = _one(rec, "gn_act_bwd", "bwd")
    work = Lf["out"][1]
    res.append(("gn.bwd.operands", max(_same(Lb["x"], x), _same(Lb["dy"], gy), 0.0 if Lb["fwd_work"] is not None and Lb["fwd_work"].data_ptr() == work.data_ptr() and Lb["add"] is None else INF,     # the forward's statistics
                                       0.0 if (Lb["groups"], Lb["act"]) == (G, act) and abs(Lb["eps"] - 1e-6) < 1e-12 else INF,
                                       _same(Lb["out"][0], rec["gx"]), _same(Lb["out"][1], rec["dgamma"]), _same(Lb["out"][2], rec["dbeta"]))))
    res.append(("gn.dx", _ratio(_c(rec["gx"]).reshape(B, H * W, Cc), o["dx"], o["d_dx"], dt)))
    res.append(("gn.dgamma", _ratio(_c(rec["dgamma"]), o["dgamma"], o["d_dgamma"], 0)))
    res.append(("gn.dbeta", _ratio(_c(rec["dbeta"]), o["dbeta"], o["d_dbeta"], 0)))
    return res


def check_fir(rec):
    x, y = _c(rec["x"]), _c(rec["y"])
    dt, up = DTC[x.dtype], rec["up"]
    L = _one(rec, "fir", "fwd")
    res = [("fir.fwd.operands", max(_same(L["x"], x), _same(L["out"], y), 0.0 if bool(L["up"]) == up else INF))]
    raw, praw, _, _ = fir_reference(x, None, 0, int(up))
    res.append(("fir.fwd", _ratio(y, raw, praw, dt)))
    if "gy" not in rec:
        return res
    gy, gx = _c(rec["gy"]), _c(rec["gx"])
    L = _one(rec, "fir", "bwd")
    res.append(("fir.bwd.operands", max(_same(L["x"], gy), 0.0 if bool(L["up"]) == (not up) else INF)))
    raw, praw, _, _ = fir_reference(gy, None, 0, 0 if up else 1)
    f = 4.0 if up else 0.25
    # the kernel's store: u |raw| (fp16 below 2^-14: 2^-25); the product by a power of two is exact unless its result is subnormal (2^-25 more)
    sub = (2.0 ** -25 * (f if f > 1 else 1 + f) if dt == 2 else 0.0) * (raw != 0)
    res.append(("fir.bwd", _abs_ratio(gx, f * raw, UNIT[dt] * (f * raw).abs() + f * praw + sub)))
    return res


def check_attn(rec):
    q, k, v, y = (_c(rec[n]) for n in ("q", "k", "v", "y"))
    dt = DTC[q.dtype]
    L = _one(rec, "attention_core", "fwd")
    res = [("attn.fwd.operands", max(_same(L["q"], q), _same(L["k"], k), _same(L["v"], v), _same(L["out"], y)))]
    ref, part = attention_reference(q, k, v)
    res.append(("attn.fwd", _ratio(y, ref, part, dt)))
    if "gy" not in rec:
        return res
    gy = _c(rec["gy"])
    L = _one(rec, "attention_core_bwd", "bwd")
    wide = (q.float(), k.float(), v.float(), gy.float())                                   # widened: exact
    res.append(("attn.bwd.operands", max(_same(L[n], t) for n, t in zip(("q", "k", "v", "dO"), wide))))
    for (ref, part), got, stored, n in zip(attention_bwd_reference(*wide), L["out"], (rec["dq"], rec["dk"], rec["dv"]), ("dq", "dk", "dv")):
        res.append(("attn." + n, _ratio(_c(got), ref, part, 0)))
        # what the call returns: the fp32 result (2^-24 |ref| + part) stored once in the storage type
        res.append(("attn." + n + ".stored", max(_ratio(_c(stored), ref, part + U32 * ref.abs(), dt) if dt else 0.0, _same(stored, got.to(q.dtype)))))
    return res


CHECK = {"conv": check_conv, "gn": check_gn, "fir": check_fir, "attn": check_attn}


def check_tape(tape, kinds=KINDS):
    """[(call index, call name, check, worst |err| / bound)] over every output of every recorded call of ``kinds``."""
    out = []
    for r in tape.calls:
        if r["kind"] in kinds:
            assert ("gy" in r) == r["needs_bwd"], f"call {r['idx']} ({r['kind']} {r['name']}): backward {'ran' if 'gy' in r else 'did not run'}"
            out += [(r["idx"], r["name"], c, v) for c, v in CHECK[r["kind"]](r)]
            r["checked"] = True
    return out


def worst(results, prefix=""):
    return max([v for _, _, c, v in results if c.startswith(prefix)], default=0.0)


# ---------------------------------------------------------------------------------------------------------------------------
# the float64 mirror: wiring and glue
# ---------------------------------------------------------------------------------------------------------------------------
GRAD_OF = {"x": "gx", "res": "g_res", "q": "dq", "k": "dk", "v": "dv"}


class _Boundary(torch.autograd.Function):
    """An operator of the tape as a pass-through: forward returns the stored output of the call, backward compares the gradient the
    mirror's glue computed with the recorded one and hands the recorded input gradients on."""

    @staticmethod
    def forward(ctx, M, rec, names, anchor, *ins):
        ctx.M, ctx.rec, ctx.names = M, rec, names                      # anchor: a leaf that requires a gradient, so that every output does
        for n, v in zip(names, ins):
            if v is not None:                                          # forward glue: one rounding of the operand per glue operation in front of it
                st = _c(rec[n])
                M.results.append((rec["idx"], rec["name"], "mirror.fwd." + n, INF if st is None or st.shape != v.shape else
                                  _abs_ratio(st, v.detach(), M.fwd_roundings.get(rec["idx"], 1) * UNIT[DTC[st.dtype]] * v.detach().abs())))
            elif rec.get(n) is not None:
                M.results.append((rec["idx"], rec["name"], "mirror.fwd." + n, INF))
        return _c(rec["y"]).double().clone()

    @staticmethod
    def backward(ctx, gy):
        M, rec, names = ctx.M, ctx.rec, ctx.names
        i = rec["idx"]

        def grads(f):
            out = []
            for j, n in enumerate(names):
                g = rec.get(GRAD_OF[n])
                if not ctx.needs_input_grad[4 + j]:
                    out.append(None)
                elif g is None:
                    M.results.append((i, rec["name"], "mirror.missing." + GRAD_OF[n], INF))
                    out.append(None)
                else:
                    out.append(f(_c(g).double()))
            return (None, None, None, None) + tuple(out)
        if M.mode == "abs":
            M.S[i] = gy
            return grads(torch.abs)
        if M.mode == "count":
            M.n[i] = gy
            return grads(torch.ones_like)
        if M.mode == "ulps":
            M.e[i] = gy
            return grads(torch.zeros_like)
        got = _c(rec["gy"])
        u = UNIT[DTC[got.dtype]]
        bound = ((M.n[i].round() - 1).clamp(min=0) * u + M.e[i] * U32) * M.S[i]
        M.results.append((i, rec["name"], "mirror.gy", INF if got.shape != gy.shape else _abs_ratio(got, gy, bound)))
        return grads(lambda g: g)


class _DivT(torch.autograd.Function):
    """pyramid / t per item: one fp32 rounding of the gradient (mode 'ulps': one more unit for whoever consumes it)."""

    @staticmethod
    def forward(ctx, M, p, t):
        ctx.M, ctx.t = M, t[:, None, None, None]
        return p / ctx.t

    @staticmethod
    def backward(ctx, g):
        m = ctx.M.mode
        return None, (g if m == "count" else g + 1.0 if m == "ulps" else g / ctx.t), None


class Mirror:
    def __init__(self, tape, P):
        self.q = {k: [r for r in tape.calls if r["kind"] == k] for k in KINDS}
        self.pos = dict.fromkeys(KINDS, 0)
        self.P, self.mode, self.results, self.S, self.n, self.e = P, None, [], {}, {}, {}
        self.anchor = torch.zeros((), dtype=torch.float64, requires_grad=True)
        self.fwd_roundings = {}                                        # call index -> glue operations in front of its operand, where not one

    def take(self, kind, name=None):
        assert self.pos[kind] < len(self.q[kind]), f"the mirror has more {kind} boundaries than the tape has calls"
        r = self.q[kind][self.pos[kind]]
        self.pos[kind] += 1
        assert r["name"] == name, (kind, self.pos[kind] - 1, r["name"], name)
        r["mirrored"] = True
        return r

    def conv(self, name, x, res=None):
        return _Boundary.apply(self, self.take("conv", name), ("x", "res"), self.anchor, x, res)

    def gn(self, name, x):
        return _Boundary.apply(self, self.take("gn", name), ("x",), self.anchor, x)

    def fir(self, x):
        return _Boundary.apply(self, self.take("fir"), ("x",), self.anchor, x)

    def attn(self, q, k, v):
        return _Boundary.apply(self, self.take("attn"), ("q", "k", "v"), self.anchor, q, k, v)

    def resblock(self, x, p, up=False, down=False):
        """ResnetBlockBigGANpp.forward as oracle/ncsnpp_oracle.py states it; Dense_0's row, the shortcut sum and 1 / sqrt 2 belong to the
        convolution calls (their per-call checks)."""
        h = self.gn(p + ".GroupNorm_0", x)
        if up or down:
            h = self.fir(h); x = self.fir(x)
        h = self.conv(p + ".Conv_0", h)
        h = self.gn(p + ".GroupNorm_1", h)
        if (p + ".Conv_2.weight") in self.P:
            x = self.conv(p + ".Conv_2", x)
        return self.conv(p + ".Conv_1", h, res=x)

    def attn_block(self, x, p):
        B, H, W, Cc = x.shape
        h = self.gn(p + ".GroupNorm_0", x)
        q, k, v = (self.conv(f"{p}.NIN_{i}", h).view(B, H * W, Cc) for i in range(3))
        a = self.attn(q, k, v).view(B, H, W, Cc)
        return self.conv(p + ".NIN_3", a, res=x)


def run_mirror(tape, P, x, t, target, ch_mult, num_res_blocks, conditional, scale_by_sigma):
    """The network of oracle/ncsnpp_oracle.py (ncsnpp_forward) in float64 on NHWC tensors with a boundary at every operator.  Returns
    (results, float64 loss on the stored network output)."""
    M = Mirror(tape, P)
    L = len(ch_mult)
    B, nin, Fq, Tq = x.shape
    x4 = torch.cat([p for k in range(nin) for p in (x[:, k].real[..., None], x[:, k].imag[..., None])], dim=3).double()
    x4 = F.pad(2 * x4 - 1.0, (0, 32 - 2 * nin))
    m = 3 if conditional else 1
    pyr_in = x4
    hs = [M.conv(f"all_modules.{m}", x4)]
    m += 1
    for lvl in range(L):
        for _ in range(num_res_blocks):
            hs.append(M.resblock(hs[-1], f"all_modules.{m}")); m += 1
        if lvl != L - 1:
            h = M.resblock(hs[-1], f"all_modules.{m}", down=True); m += 1
            pyr_in = M.fir(pyr_in).detach()                           # the input pyramid carries no gradient
            h = M.conv(f"all_modules.{m}.Conv_0", pyr_in) + h
            m += 1
            hs.append(h)
    h = hs[-1]
    h = M.resblock(h, f"all_modules.{m}"); m += 1
    h = M.attn_block(h, f"all_modules.{m}"); m += 1
    h = M.resblock(h, f"all_modules.{m}"); m += 1
    pyramid = None
    for lvl in reversed(range(L)):
        for _ in range(num_res_blocks + 1):
            h = M.resblock(torch.cat([h, hs.pop()], dim=3), f"all_modules.{m}"); m += 1
        ph = M.gn(f"all_modules.{m}", h); m += 1
        ph = M.conv(f"all_modules.{m}", ph); m += 1
        pyramid = ph if pyramid is None else M.fir(pyramid) + ph
        if lvl != 0:
            h = M.resblock(h, f"all_modules.{m}", up=True); m += 1
    assert not hs
    if scale_by_sigma:
        pyramid = _DivT.apply(M, pyramid, t.double())
    if scale_by_sigma and L > 1:                                      # the pyramid sum and the division: two roundings in front of the output layer
        M.fwd_roundings[M.q["conv"][-1]["idx"]] = 2
    yb = M.conv("output_layer", pyramid)
    out = torch.view_as_complex(yb[..., :2].contiguous()).unsqueeze(1)
    loss = (out - target.to(torch.complex128)).abs().square().mean()
    for k in KINDS:
        assert M.pos[k] == len(M.q[k]), f"{len(M.q[k]) - M.pos[k]} recorded {k} calls have no boundary in the mirror"
    (g,) = torch.autograd.grad(loss, yb, retain_graph=True)
    # root: |d| (2 ulps), 2 |d| / N (two roundings), d / |d| and the product (three): 8 x 2^-24 |g|
    for mode, root in (("abs", g.abs()), ("count", (g != 0).double()), ("ulps", 8.0 * torch.ones_like(g)), ("check", g)):
        M.mode = mode
        yb.backward(gradient=root, retain_graph=True)
    return M.results, float(loss.detach())


def temb_checks(tape, P, t, grads):
    """The torch-only part: GaussianFourierProjection -> Linear -> SiLU -> Linear -> SiLU -> every Dense_0 (library GEMMs on B rows).
    Forward values with their fp32 bounds as temb_reference of tests/test_hip_forward_kernels.py derives them; the gradients by hand in
    float64 from the recorded g_temb of every Conv_0, each GEMM held to C_ACC 2^-24 sqrt(K) S + 2^-24 |ref| plus what the fp32 forward
    values and upstream gradients carry in.  P, grads: CPU tensors by parameter name."""
    d = lambda k: P[k].detach().double()
    W0, W1, b1, W2, b2 = d("all_modules.0.W"), d("all_modules.1.weight"), d("all_modules.1.bias"), d("all_modules.2.weight"), d("all_modules.2.bias")
    nf, B = W0.numel(), t.numel()
    ka = lambda K: C_ACC * U32 * math.sqrt(K)
    xp = torch.log(t.double())[:, None] * W0[None] * 2 * math.pi
    feat = torch.cat([torch.sin(xp), torch.cos(xp)], -1)
    dfeat = ((ULP_FN + 2.5) * xp.abs() + ULP_FN).repeat(1, 2) * U32
    a1 = feat @ W1.T + b1
    da1 = dfeat @ W1.abs().T + ka(2 * nf) * (feat.abs() @ W1.abs().T + b1.abs())
    hid, dhid = _silu(a1), 1.1 * da1 + _silu_err(a1)
    a2 = hid @ W2.T + b2
    da2 = dhid @ W2.abs().T + ka(4 * nf) * (hid.abs() @ W2.abs().T + b2.abs())
    ta, dta = _silu(a2), 1.1 * da2 + _silu_err(a2) + U32 * _silu(a2).abs()
    res = []
    gta, s_gta, Ktot = torch.zeros_like(ta), torch.zeros_like(ta), 0
    for r in tape.calls:
        if r["kind"] != "conv" or r["temb"] is None:
            continue
        p = r["name"].rsplit(".", 1)[0]
        Wd, bd = d(p + ".Dense_0.weight"), d(p + ".Dense_0.bias")
        dense = ta @ Wd.T + bd
        res.append((r["idx"], r["name"], "temb.dense", _ratio(_c(r["temb"]), dense, dta @ Wd.abs().T + ka(4 * nf) * (ta.abs() @ Wd.abs().T + bd.abs()), 0)))
        G = _c(r["g_temb"]).double()
        res.append((r["idx"], p + ".Dense_0.weight", "temb.grad", _ratio(grads[p + ".Dense_0.weight"], G.T @ ta, G.abs().T @ dta + ka(B) * (G.abs().T @ ta.abs()), 0)))
        res.append((r["idx"], p + ".Dense_0.bias", "temb.grad", _ratio(grads[p + ".Dense_0.bias"], G.sum(0), ka(B) * G.abs().sum(0), 0)))
        gta, s_gta, Ktot = gta + G @ Wd, s_gta + G.abs() @ Wd.abs(), Ktot + Wd.shape[0] + 1
    e_gta = ka(Ktot) * s_gta
    g2, dg2 = _act_grad(a2)
    ga2 = gta * g2
    e_ga2 = e_gta * g2.abs() + gta.abs() * (0.5 * da2 + dg2) + U32 * ga2.abs()
    gh = ga2 @ W2
    e_gh = e_ga2 @ W2.abs() + ka(4 * nf) * (ga2.abs() @ W2.abs())
    g1, dg1 = _act_grad(a1)
    ga1 = gh * g1
    e_ga1 = e_gh * g1.abs() + gh.abs() * (0.5 * da1 + dg1) + U32 * ga1.abs()
    for name, ref, part in (("all_modules.2.weight", ga2.T @ hid, ga2.abs().T @ dhid + e_ga2.T @ hid.abs() + ka(B) * (ga2.abs().T @ hid.abs())),
                            ("all_modules.2.bias", ga2.sum(0), e_ga2.sum(0) + ka(B) * ga2.abs().sum(0)),
                            ("all_modules.1.weight", ga1.T @ feat, ga1.abs().T @ dfeat + e_ga1.T @ feat.abs() + ka(B) * (ga1.abs().T @ feat.abs())),
                            ("all_modules.1.bias", ga1.sum(0), e_ga1.sum(0) + ka(B) * ga1.abs().sum(0))):
        res.append((-1, name, "temb.grad", _ratio(grads[name], ref, part, 0)))
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# the float64 emulation of the tape (CPU): every launch is the float64 reference of its kernel, stored once in the storage type
# ---------------------------------------------------------------------------------------------------------------------------
LAUNCH_MUT = {"v": None}              # the deliberately wrong launches of the CPU controls


def emu_conv_dev(x, w, b, w_mode, ntaps, cout, scale=1.0, out_dtype=None, temb=None, res=None):
    dt, sc = DTC[x.dtype], float(np.float32(scale))
    if w_mode == 1:
        ref, _ = dgrad_reference(x, w, dt, sc, mut="no_flip" if LAUNCH_MUT["v"] == "unflipped" else None)
    else:
        ref, _ = conv_reference(x, None, 0, w.t() if w_mode == 2 else w, dt, bias=b, temb=temb, res=res, scale=sc)
    return ref.to(out_dtype or x.dtype).contiguous()


def emu_conv_wgrad(dy, x, ntaps=9, alpha=1.0, with_bias=True, tiled=True):
    assert dy.dtype == x.dtype
    a = 1.0 if LAUNCH_MUT["v"] == "no_alpha" and ntaps == 9 else alpha
    dw, _, db, _ = wgrad_reference(dy, x, ntaps, a)
    return dw.float().contiguous(), (db.float() if with_bias else None)


def emu_colsum(x, scale=1.0):
    B, H, W, Cc = x.shape
    return colsum_reference(x.reshape(B, H * W, Cc), scale, 0, mut="scale" if LAUNCH_MUT["v"] == "colsum_scale" else None)[0].float()


def emu_gn_act_fwd(x, gamma, beta, groups, act=1, eps=1e-6, return_work=False):
    B, H, W, Cc = x.shape
    o = gn_reference(x.reshape(B, H * W, Cc), None, None, gamma, beta, groups, act, 1.0, 0)
    y = o["y"].to(x.dtype).view(B, H, W, Cc)
    return (y, torch.stack([o["mean"], o["rstd"]]).float()) if return_work else y


def emu_gn_act_bwd(x, dy, gamma, beta, groups, act=1, add=None, add_scale=1.0, eps=1e-6, fwd_work=None):
    B, H, W, Cc = x.shape
    assert add is None
    o = gn_reference(x.reshape(B, H * W, Cc), dy.reshape(B, H * W, Cc), None, gamma, beta, groups, act, 1.0, 0, mut="eps" if LAUNCH_MUT["v"] == "gn_eps" else None)
    return o["dx"].to(x.dtype).view(B, H, W, Cc), o["dgamma"].float(), o["dbeta"].float()


def emu_fir(x, up):
    return fir_reference(x, None, 0, int(bool(up)))[0].to(x.dtype).contiguous()


def emu_attention_core(q, k, v):
    return attention_reference(q, k, v)[0].to(q.dtype)


def emu_attention_core_bwd(q, k, v, dO):
    return tuple(r.float() for r, _ in attention_bwd_reference(q, k, v, dO))


def install_emulation(mp):
    T, ops = _training()
    mp.setattr(T, "_conv_dev", emu_conv_dev)
    for n in LAUNCHES:
        mp.setattr(ops, n, globals()["emu_" + n])


class _DropGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return torch.zeros_like(g)


class _CatSwapped(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ctx.n = a.shape[3]
        return torch.cat([a, b], dim=3)

    @staticmethod
    def backward(ctx, g):
        return g[..., ctx.n:].contiguous(), g[..., :ctx.n].contiguous()


class _DivT0(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, t):
        ctx.t0 = t[0]
        return p / t[:, None, None, None]

    @staticmethod
    def backward(ctx, g):
        return g / ctx.t0, None


def emu_forward_train(P, x, t, ch_mult, num_res_blocks, conditional=True, scale_by_sigma=True, compute_dtype=torch.float32, glue_mut=None):
    """training.ncsnpp_forward_train on CPU tensors: the same torch glue in the same types around the same operator calls (training.conv,
    _resblock, _attn_block, _gn, _pad_to as they stand).  glue_mut: 'drop_skip' | 'cat_swapped' | 'div_t0'."""
    T, _ = _training()
    cd = compute_dtype
    L = len(ch_mult)
    B, nin, Fq, Tq = x.shape
    x4 = torch.view_as_real(x.detach()).permute(0, 2, 3, 1, 4).reshape(B, Fq, Tq, 2 * nin).float()
    x4 = F.pad(2.0 * x4 - 1.0, (0, 32 - 2 * nin)).contiguous()
    if not conditional:
        temb_act, m = None, 1
    else:
        xp = torch.log(t.float())[:, None] * P["all_modules.0.W"].detach()[None, :] * (2 * math.pi)
        e = torch.cat([torch.sin(xp), torch.cos(xp)], dim=-1)
        e = F.linear(e, P["all_modules.1.weight"], P["all_modules.1.bias"])
        temb_act = F.silu(F.linear(F.silu(e), P["all_modules.2.weight"], P["all_modules.2.bias"]))
        m = 3
    pyr_in = x4
    hs = [T.conv(x4, T._pad_to(P[f"all_modules.{m}.weight"], 1, 32), P[f"all_modules.{m}.bias"], cd)]
    m += 1
    for lvl in range(L):
        for _ in range(num_res_blocks):
            h = T._resblock(hs[-1], temb_act, P, f"all_modules.{m}"); m += 1
            hs.append(_DropGrad.apply(h) if glue_mut == "drop_skip" and len(hs) == 1 else h)
        if lvl != L - 1:
            h = T._resblock(hs[-1], temb_act, P, f"all_modules.{m}", down=True); m += 1
            pyr_in = T.fir(pyr_in, False)
            h = T.conv(pyr_in, T._pad_to(P[f"all_modules.{m}.Conv_0.weight"], 1, 32), P[f"all_modules.{m}.Conv_0.bias"], cd) + h
            m += 1
            hs.append(h)
    h = T._resblock(hs[-1], temb_act, P, f"all_modules.{m}"); m += 1
    h = T._attn_block(h, P, f"all_modules.{m}"); m += 1
    h = T._resblock(h, temb_act, P, f"all_modules.{m}"); m += 1
    pyramid, first = None, True
    for lvl in reversed(range(L)):
        for _ in range(num_res_blocks + 1):
            skip = hs.pop()
            c = _CatSwapped.apply(h, skip) if glue_mut == "cat_swapped" and first else torch.cat([h, skip], dim=3)
            first = False
            h = T._resblock(c, temb_act, P, f"all_modules.{m}"); m += 1
        ph = T._gn(h, P, f"all_modules.{m}", 1); m += 1
        ph = T.conv(ph, T._pad_to(P[f"all_modules.{m}.weight"], 0, 32), T._pad_to(P[f"all_modules.{m}.bias"], 0, 32), torch.float32); m += 1
        pyramid = ph if pyramid is None else T.fir(pyramid, True) + ph
        if lvl != 0:
            h = T._resblock(h, temb_act, P, f"all_modules.{m}", up=True); m += 1
    assert not hs
    if scale_by_sigma:
        pyramid = _DivT0.apply(pyramid, t.float()) if glue_mut == "div_t0" else pyramid / t.float()[:, None, None, None]
    wo = T._pad_to(T._pad_to(P["output_layer.weight"], 1, 32), 0, 32)
    out = T.conv(pyramid, wo, T._pad_to(P["output_layer.bias"], 0, 32))[..., :2]
    return torch.view_as_complex(out.contiguous()).unsqueeze(1)
