"""The walker of the sampler step trace (use_sampler_trace_entry in include/use_hip.h; HipScoreEngine.sampler_trace()) and a float32 numpy
emulation of run_sampler (csrc/use_engine.cpp) that emits the same entries.  Used by tests/test_hip_sampler_steps.py.

walk() holds every entry of one sampler call against the float64 restatements of tests/philox_ref.py - prior, predictor, corrector,
langevin_eps (at the entry's blocks_per_b, shared or per item), ald_eps - with their per-element bounds, unchanged, and returns the worst
|err| / bound per kind.  What it reads of an entry: the snapshots the launch read (x_in, score, step) and wrote (x_out, x_mean, step), the
float32 scalars it was passed, and the draw index d; z is draw d of the `draws` the caller gives (the injected noise, or the device
stream fetched with use_fill_noise*).  Beside the values it checks the layout - kinds, i, k, d = 0, 1, 2, ... without gaps, t bit-equal
to torch.linspace(1, t_eps, N)[i], items / n_per_item, x_mean at the last step alone - against the reference loop
(sampling/__init__.py:59-71), and the chain: every x_in holds the bits of the newest x_out before it, every update's score those of the
newest evaluation.  A broken layout or chain is a ratio of inf under "layout" / "chain".

emulate() is the "device" of the mutation controls: the loop of run_sampler in float32 numpy, segments included, with an analytic score
(the stand-in of oracle/gen_golden.py's sampler fixtures).  Its reductions are float64 sums rounded once - more accurate than the
kernels', which is all the controls need: unmutated it must stay below 1, and each mutation must exceed 1 somewhere.  A mutation changes
what the loop computes and not what it records: the entry says what the right loop would have done, as a trace of faulty code would."""
import math

import numpy as np
import torch

import philox_ref as pr

KINDS = ("prior", "score", "langevin_norms", "langevin_step", "corrector", "predictor", "copy_mean", "scalars", "layout", "chain")
SNAPSHOTS = {"prior": ("x_out",), "score": ("x_in", "score"), "langevin_norms": ("score",), "langevin_step": ("step",),
             "corrector": ("x_in", "score", "x_out"), "predictor": ("x_in", "score", "x_out"), "copy_mean": ("x_in", "x_mean")}
SEGMENT_EVALS = 64                                        # evaluations per captured graph segment (sample_impl)


def n_corr(cfg):
    return 0 if cfg["corrector"] == "none" else cfg["corrector_steps"]


def n_draws(cfg):
    return 1 + cfg["N"] * (n_corr(cfg) + (cfg["predictor"] != "none"))


def timesteps(cfg):
    return torch.linspace(1, cfg["t_eps"], cfg["N"]).numpy()


def expected_layout(cfg):
    """[(kind, i, k, d)] of the reference loop: the prior, then per step the correctors (evaluation, [norms, step,] update) and the
    predictor (evaluation, update); d counts the draws in the order they are consumed."""
    out, d = [("prior", -1, -1, 0)], 1
    for i in range(cfg["N"]):
        for k in range(n_corr(cfg)):
            out.append(("score", i, k, -1))
            if cfg["corrector"] == "langevin":
                out += [("langevin_norms", i, k, d), ("langevin_step", i, k, -1)]
            out.append(("corrector", i, k, d))
            d += 1
        if cfg["predictor"] == "none":
            if i == cfg["N"] - 1:
                out.append(("copy_mean", i, -1, -1))
        else:
            out += [("score", i, -1, -1), ("predictor", i, -1, d)]
            d += 1
    return out


def _np(a):
    return None if a is None else (a.numpy() if isinstance(a, torch.Tensor) else np.asarray(a))


def _bits(a, b):
    a, b = _np(a), _np(b)
    return a is not None and b is not None and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _rel(got, ref, units):
    """|got - ref| / (units 2^-24 |ref|) of a float32 scalar (array) against its float64 value"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float(np.max(np.abs(got - ref) / (units * pr.U32 * np.abs(ref))))


def walk(entries, y, draws, cfg):
    """-> {kind: worst |err| / bound}.  entries: dicts as HipScoreEngine.sampler_trace() returns them; y [B,1,F,T] complex64; draws
    [n_draws,B,1,F,T] complex64; cfg: N, predictor, corrector, corrector_steps, snr, t_eps, per_item."""
    y, draws = _np(y), _np(draws)
    B, n = y.shape[0], y.size
    w = dict.fromkeys(KINDS, 0.0)

    def worst(kind, v):
        w[kind] = max(w[kind], v)
    ts, N, per_item = timesteps(cfg), cfg["N"], bool(cfg["per_item"])
    want = expected_layout(cfg)
    if [(e["kind"], e["i"], e["k"], e["d"]) for e in entries] != want or len(draws) != n_draws(cfg):
        w["layout"] = float("inf")
        return w
    last_x = last_s = last_step = None
    for e in entries:
        kind, i, d = e["kind"], e["i"], e["d"]
        t = np.float32(1.0) if kind == "prior" else ts[i]
        ok = np.float32(e["t"]).view(np.uint32) == np.float32(t).view(np.uint32)
        ok = ok and e["per_item"] == int(per_item) and (e["items"], e["n_per_item"]) == ((B, n // B) if per_item else (1, n))
        if not ok:
            worst("layout", float("inf"))
        if any(e[f] is None for f in SNAPSHOTS[kind]):                     # a snapshot the kind must name is missing
            worst("layout", float("inf"))
            continue
        z = draws[d] if d >= 0 else None
        x_in, s, x_out = _np(e["x_in"]), _np(e["score"]), _np(e["x_out"])
        if kind in ("score", "corrector", "predictor", "copy_mean") and not _bits(x_in, last_x):
            worst("chain", float("inf"))
        if kind in ("langevin_norms", "corrector", "predictor") and not _bits(s, last_s):
            worst("chain", float("inf"))
        if kind == "prior":
            ref, br, bi = pr.prior(y, z)
            worst("prior", pr.ratio(x_out, ref, br, bi))
            worst("scalars", _rel(e["std1"], pr.ouve_std(1.0), pr.E_STD))
        elif kind == "score":
            last_s = s
            if s is None or not np.isfinite(s.view(np.float32)).all():
                worst("score", float("inf"))
        elif kind == "langevin_norms":
            eps, e_eps = pr.langevin_eps(s, z, cfg["snr"], blocks=e["blocks_per_b"], per_item=per_item)
        elif kind == "langevin_step":
            # (eps, e_eps of the norms entry just before: the layout put it there)
            last_step = _np(e["step"])
            if last_step is None or last_step.shape != ((B,) if per_item else (1,)):
                worst("layout", float("inf"))
            else:
                worst("langevin_step", _rel(last_step, eps, e_eps))
        elif kind == "corrector":
            if cfg["corrector"] == "langevin":
                if not _bits(e["step"], last_step):
                    worst("chain", float("inf"))
            else:
                eps, e_eps = pr.ald_eps(t, cfg["snr"])
                worst("scalars", _rel(e["step_host"], eps, e_eps))
            parts = [(slice(b, b + 1), float(eps[b])) for b in range(B)] if np.ndim(eps) else [(slice(None), float(eps))]
            for sl, eps_b in parts:                                        # per item: item b with its own step
                ref, _, bo, _ = pr.corrector(eps_b, e_eps, x_in[sl], s[sl], z[sl])
                worst("corrector", pr.ratio(x_out[sl], ref, *bo) if x_out is not None else float("inf"))
        elif kind == "predictor":
            ref, mean, bo, bm = pr.predictor(t, N, x_in, y, s, z)
            worst("predictor", pr.ratio(x_out, ref, *bo) if x_out is not None else float("inf"))
            if (e["x_mean"] is not None) != (i == N - 1):
                worst("layout", float("inf"))
            elif i == N - 1:
                worst("predictor", pr.ratio(_np(e["x_mean"]), mean, *bm))
            for got, ref_c, units in zip((e["c_drift"], e["c_score"], e["c_noise"]), pr.predictor_coeffs(t, N), (pr.E_CD, pr.E_CS, pr.E_CN)):
                worst("scalars", _rel(got, ref_c, units))
        elif kind == "copy_mean":
            worst("copy_mean", 0.0 if _bits(e["x_mean"], x_in) else float("inf"))
        if x_out is not None:
            last_x = x_out
    return w


# ---------------------------------------------------------------------------------------------------------------------------
# the float32 emulation of run_sampler
# ---------------------------------------------------------------------------------------------------------------------------
F32 = np.float32
MUTATIONS = ("swap_draws", "segment_counter", "coeffs_next_t", "eps_batch_mean", "eps_prev_score", "mean_with_noise", "mean_early",
             "sqrt_eps", "aliased_neighbour")


def analytic_score(x, t, y, a):
    """the stand-in of the sampler fixtures (oracle/gen_golden.py), in float32: -(x - 0.8 y) / (0.1 + t^2) + 0.05 a tanh|x|"""
    return (-(x - F32(0.8) * y) / F32(F32(0.1) + F32(t) * F32(t)) + F32(0.05) * a * np.tanh(np.abs(x)).astype(F32)).astype(np.complex64)


def coeffs_f32(t, N, predictor):
    """predictor_coeffs of use_engine.cpp, rounding where it rounds"""
    sigma = F32(pr.SIGMA_MIN) * np.power(F32(pr.SIGMA_MAX) / F32(pr.SIGMA_MIN), F32(t), dtype=F32)
    g = F32(float(sigma) * math.sqrt(2 * pr.logsig()))
    if predictor == "reverse_diffusion":
        dt = F32(1.0 / N)
        G = F32(g * np.sqrt(dt))
        return F32(F32(pr.THETA) * dt), F32(G * G), G
    dt = 1.0 / N
    return F32(pr.THETA * dt), F32(float(F32(g * g)) * dt), F32(float(g) * math.sqrt(dt))


def _re(a):
    return a.view(F32)


def _c(a):
    return np.ascontiguousarray(a, F32).view(np.complex64)


def lang_blocks(n_per_b):
    return min(256, -(-n_per_b // 256))


def emulate(cfg, y, draws, a, mut=None, segmented=None):
    """-> entries of one call.  segmented: run as captured segments of SEGMENT_EVALS evaluations (default: cfg["use_graph"])."""
    assert mut is None or mut in MUTATIONS
    y, draws = np.asarray(y, np.complex64), np.asarray(draws, np.complex64)
    B, n = y.shape[0], y.size
    N, per_item, ncorr, pred = cfg["N"], bool(cfg["per_item"]), n_corr(cfg), cfg["predictor"]
    snr, ts = F32(cfg["snr"]), timesteps(cfg)
    npd = ncorr + (pred != "none")
    blocks = lang_blocks(n // B)
    nan = np.full(y.shape, np.nan + 1j * np.nan, np.complex64)
    st = {"X": nan.copy(), "Xmean": nan.copy(), "score": nan.copy(), "prev_score": nan.copy(), "step": None}
    entries = []

    def rec(kind, i, k, d, **kw):
        e = dict(kind=kind, i=i, k=k, d=d, t=F32(1.0) if kind == "prior" else ts[i], std1=F32(0), c_drift=F32(0), c_score=F32(0),
                 c_noise=F32(0), step_host=F32(0), items=B if per_item else 1, n_per_item=n // B if per_item else n, blocks_per_b=0,
                 per_item=int(per_item), x_in=None, score=None, step=None, x_out=None, x_mean=None, noise=None)
        e.update(kw)
        entries.append(e)

    def alias(xin, out_of):
        """the update with every 256th element reading its already-updated left neighbour, as an in-place fault would"""
        out = out_of(xin)
        if mut != "aliased_neighbour":
            return out
        j = np.arange(256, xin.size, 256)
        bad = xin.copy().reshape(-1)
        bad[j] = out.reshape(-1)[j - 1]
        out.reshape(-1)[j] = out_of(bad.reshape(xin.shape)).reshape(-1)[j]
        return out

    def evaluate(i):
        st["prev_score"] = st["score"]
        st["score"] = analytic_score(st["X"], ts[i], y, a)

    def segment(i0, i1):
        d = 1 + i0 * npd
        if mut == "segment_counter" and i0 > 0:
            d = 1
        if i0 == 0:
            std1 = F32(pr.ouve_std(1.0))
            st["X"] = _c(_re(y) + _re(draws[0]) * std1)
            rec("prior", -1, -1, 0, std1=std1, x_out=st["X"])
        for i in range(i0, i1):
            t = ts[i]
            for k in range(ncorr):
                x_in = st["X"]
                evaluate(i)
                rec("score", i, k, -1, x_in=x_in, score=st["score"])
                nominal = 1 + i * npd + k
                zd = d + 1 if mut == "swap_draws" and pred != "none" and k == ncorr - 1 else d
                z = draws[zd]
                if cfg["corrector"] == "langevin":
                    rec("langevin_norms", i, k, nominal, score=st["score"], blocks_per_b=blocks)
                    g = st["prev_score"] if mut == "eps_prev_score" and np.isfinite(_re(st["prev_score"])).all() else st["score"]
                    gn = np.sqrt((np.abs(g.astype(np.complex128)) ** 2).reshape(B, -1).sum(1))
                    zn = np.sqrt((np.abs(z.astype(np.complex128)) ** 2).reshape(B, -1).sum(1))
                    if not per_item or mut == "eps_batch_mean":
                        gn, zn = np.full(B if per_item else 1, gn.mean()), np.full(B if per_item else 1, zn.mean())
                    r = snr * zn.astype(F32) / gn.astype(F32)
                    st["step"] = (r * r * F32(2)).astype(F32)
                    rec("langevin_step", i, k, -1, step=st["step"], blocks_per_b=blocks)
                    eps = st["step"].reshape((-1,) + (1,) * (y.ndim - 1 + 1))               # over the float view [B,1,F,T,2]
                    kw = dict(step=st["step"])
                else:
                    sd = snr * F32(pr.ouve_std(t))
                    eps = F32(sd * sd * F32(2))
                    kw = dict(step_host=eps)
                sq = np.sqrt(eps * F32(1 if mut == "sqrt_eps" else 2)).astype(F32)
                shape5 = y.shape + (2,)
                st["X"] = _c(alias(_re(x_in).reshape(shape5), lambda xv: (xv + eps * _re(st["score"]).reshape(shape5))
                                   + _re(z).reshape(shape5) * sq)).reshape(y.shape)
                rec("corrector", i, k, nominal, x_in=x_in, score=st["score"], x_out=st["X"], **kw)
                d += 1
            if pred == "none":
                if i == N - 1:
                    st["Xmean"] = st["X"].copy()
                    rec("copy_mean", i, -1, -1, x_in=st["X"], x_mean=st["Xmean"])
                continue
            x_in = st["X"]
            evaluate(i)
            rec("score", i, -1, -1, x_in=x_in, score=st["score"])
            cd, cs, cn = coeffs_f32(ts[min(i + 1, N - 1)] if mut == "coeffs_next_t" else t, N, pred)
            z = draws[d - 1 if mut == "swap_draws" and ncorr else d]
            xv, yv, sv, zv = _re(x_in), _re(y), _re(st["score"]), _re(z)
            mean_of = lambda xx: xx - (cd * (yv - xx) - cs * sv)                   # noqa: E731
            mean = mean_of(xv)
            st["X"] = _c(alias(xv, lambda xx: mean_of(xx) + cn * zv)).reshape(y.shape)
            write_mean = i == (N - 2 if mut == "mean_early" else N - 1)
            if write_mean:
                st["Xmean"] = st["X"].copy() if mut == "mean_with_noise" else _c(mean).reshape(y.shape)
            tcoef = coeffs_f32(t, N, pred) if mut != "coeffs_next_t" else (cd, cs, cn)
            rec("predictor", i, -1, 1 + i * npd + ncorr, x_in=x_in, score=st["score"], x_out=st["X"],
                x_mean=st["Xmean"] if i == N - 1 else None, c_drift=tcoef[0], c_score=tcoef[1], c_noise=tcoef[2])
            d += 1

    per_seg = max(1, SEGMENT_EVALS // (ncorr + 1)) if (cfg.get("use_graph") if segmented is None else segmented) else N
    for i0 in range(0, N, per_seg):
        segment(i0, min(N, i0 + per_seg))
    return entries
