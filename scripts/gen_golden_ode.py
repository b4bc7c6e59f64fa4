#!/usr/bin/env python3
"""Golden vectors of the probability-flow ODE sampler -- runs ONLY in the build container (needs the reference checkout).

Same method as ``oracle/gen_golden.py``: the reference's own Python is imported (with the same two in-memory stub modules) and
its ``sampling.get_ode_sampler(..., device="cpu")`` runs with the cheap analytic score of the other sampler fixtures.  The score
captures ``Y`` and ignores its extra arguments, so the reference's ``score_model(x, t, y)`` call works (its own ScoreModel would
raise there).  ``torch.randn_like`` replays ``tnoise.sampler_noise``: draw 0 for the prior, then the unused
draw of the denoise step.  ``integrate.solve_ivp`` is wrapped to record the accepted times, nfev and status.  Data only is written.

    python scripts/gen_golden_ode.py --reference <reference checkout>      (or USE_REFERENCE_DIR=<reference checkout>)

Fixtures, all at [3,1,16,8]:
  ode_batch.npz      minibatch=None: one integration over the flattened batch
  ode_items.npz      minibatch=1 as ScoreModel.get_ode_sampler runs it: one integration per item, each replaying item i's slice of
                     one whole-batch prior draw; at least one step is rejected (asserted)
  ode_tight.npz      rtol = atol = 1e-7 (minibatch=None)
  ode_nodenoise.npz  denoise=False (minibatch=None)
"""
import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
SHAPE = (3, 1, 16, 8)
NOISE_SEED = 41
N = 30
EPS = 0.03
# score = -(x - 0.8 Y) / (C0 + t^2) + AMP A tanh|x|: stiff enough near t_eps for rejected steps, and no accept / reject decision of
# any fixture flips when the drift moves by one float32 ulp (checked when these were chosen), so that a device re-run can match NFE
C0, AMP = 0.01, 0.05


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("USE_REFERENCE_DIR"), help="the reference project's checkout")
    a = ap.parse_args()
    if not a.reference:
        ap.error("--reference (or USE_REFERENCE_DIR) is required")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, a.reference)
    for m in ("torchaudio", "pydub"):
        sys.modules.setdefault(m, types.ModuleType(m))
    sys.modules["pydub"].AudioSegment = object

    import torch
    from scipy import integrate

    from universal_speech_enhancement_amd.testing import noise as tnoise
    from src.models.components.sgmse import sampling as ref_sampling
    from src.models.components.sgmse.sdes import OUVESDE

    torch.set_num_threads(8)
    Y = torch.from_numpy(tnoise.complex_normal(21, "samp_y", SHAPE))
    A = torch.from_numpy(tnoise.complex_normal(21, "samp_a", (1, 1) + SHAPE[2:]))
    draws = tnoise.sampler_noise(NOISE_SEED, 2, SHAPE)      # [prior, denoise step's (unused) draw]

    def make_score(Yc):
        def score_fn(x, t, *args, **kwargs):               # the analytic stand-in of the other sampler fixtures; Y captured
            return -(x - 0.8 * Yc) / (C0 + t[:, None, None, None] ** 2) + AMP * A * torch.tanh(x.abs())
        return score_fn

    def run(Yc, prior, rtol, atol, denoise):
        """One call of the reference's get_ode_sampler: (x, nfe, accepted times, status)."""
        rec = {}
        orig_solve, orig_randn = integrate.solve_ivp, torch.randn_like
        queue = [prior, draws[1][: prior.shape[0]]]

        def solve_ivp(*args, **kw):
            sol = orig_solve(*args, **kw)
            rec.update(t=np.asarray(sol.t, dtype=np.float64), nfev=int(sol.nfev), status=int(sol.status))
            return sol

        def randn_like(like, **kw):
            z = torch.from_numpy(np.ascontiguousarray(queue.pop(0)))
            assert z.shape == like.shape and z.dtype == like.dtype
            return z

        integrate.solve_ivp, torch.randn_like = solve_ivp, randn_like
        try:
            sde = OUVESDE()
            sde.N = N
            x, nfe = ref_sampling.get_ode_sampler(sde, make_score(Yc), Yc, denoise=denoise, rtol=rtol, atol=atol, eps=EPS,
                                                  device="cpu")()
        finally:
            integrate.solve_ivp, torch.randn_like = orig_solve, orig_randn
        assert nfe == rec["nfev"]
        return x.numpy(), rec

    def save(name, minibatch, rtol, atol, denoise):
        if minibatch is None:
            x, rec = run(Y, draws[0], rtol, atol, denoise)
            recs = [rec]
        else:
            xs, recs = [], []
            for i in range(0, SHAPE[0], minibatch):
                xi, rec = run(Y[i:i + minibatch], draws[0][i:i + minibatch], rtol, atol, denoise)
                xs.append(xi); recs.append(rec)
            x = np.concatenate(xs)
        nfev = np.array([r["nfev"] for r in recs], dtype=np.int64)
        nt = np.array([len(r["t"]) for r in recs], dtype=np.int64)
        times = np.full((len(recs), int(nt.max())), np.nan)
        for g, r in enumerate(recs):
            times[g, : len(r["t"])] = r["t"]
        rejected = (nfev - 2) // 6 - (nt - 1)
        print(f"  {name}: nfev {nfev.tolist()}, accepted steps {(nt - 1).tolist()}, rejected {rejected.tolist()}, "
              f"status {[r['status'] for r in recs]}")
        np.savez(os.path.join(OUT, f"{name}.npz"), Y=Y.numpy(), A=A.numpy(), prior=draws[0], x=x, nfev=nfev, times=times, n_times=nt,
                 status=np.array([r["status"] for r in recs]), rejected=rejected, rtol=rtol, atol=atol, eps=EPS, N=N,
                 denoise=int(denoise), minibatch=-1 if minibatch is None else minibatch, noise_seed=NOISE_SEED, c0=C0, amp=AMP)
        return rejected

    os.makedirs(OUT, exist_ok=True)
    save("ode_batch", None, 1e-5, 1e-5, True)
    rej = save("ode_items", 1, 1e-5, 1e-5, True)
    assert rej.sum() >= 1, "ode_items must contain a rejected step"
    save("ode_tight", None, 1e-7, 1e-7, True)
    save("ode_nodenoise", None, 1e-5, 1e-5, False)


if __name__ == "__main__":
    main()
