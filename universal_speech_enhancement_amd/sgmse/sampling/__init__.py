"""Predictor-corrector and probability-flow ODE sampling with the reference's call surface
(``sgmse/sampling/__init__.py:23-73`` ``get_pc_sampler``, ``:76-159`` ``get_ode_sampler``).

Two execution paths each, same numerics:
  * fused  -- when ``score_fn`` is the HIP-backed ``ScoreModel`` and predictor / corrector are built-ins, the whole
              loop (prior sampling, N x (corrector, predictor), all score evaluations) runs inside
              ``use_sample`` and is replayed as one hipGraph;
  * seam   -- any other ``score_fn`` callable or user-registered predictor / corrector: the loop below drives
              ``update_fn`` exactly like the reference (corrector before predictor, returns ``x_mean``).
The ODE sampler integrates with scipy's RK45 reproduced on the device (``use_sample_ode`` when fused, the ``use_ode_*`` stepper
driven from here on the seam path); scipy is not needed at run time.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch

from .correctors import Corrector, CorrectorRegistry, _HipCorrector, NoneCorrector
from .predictors import Predictor, PredictorRegistry, _HipPredictor, NonePredictor

__all__ = ["PredictorRegistry", "CorrectorRegistry", "Predictor", "Corrector", "get_pc_sampler", "get_ode_sampler"]

_SDE_ENGINES: Dict[Tuple, object] = {}


def _sde_engine(sde, device):
    """A weight-less ``use_handle`` carrying the SDE constants, for the stand-alone ``use_sde_*`` kernels."""
    from ...hip_engine import HipScoreEngine
    dev = torch.device(device).index
    dev = torch.cuda.current_device() if dev is None else dev
    key = (dev, float(sde.theta), float(sde.sigma_min), float(sde.sigma_max))
    if key not in _SDE_ENGINES:   # (a weight-less handle: the stepper and the use_sde_* kernels only read its SDE constants)
        _SDE_ENGINES[key] = HipScoreEngine(device=dev, theta=sde.theta, sigma_min=sde.sigma_min, sigma_max=sde.sigma_max)
    return _SDE_ENGINES[key]


def get_pc_sampler(predictor_name, corrector_name, sde, score_fn, y, denoise=True, eps=3e-2, snr=0.1,
                   corrector_steps=1, probability_flow: bool = False, conditioning=None, intermediate=False,
                   noise=None, seed=0, use_graph=True, per_item=False, item_seeds=None, **kwargs):
    """Returns ``pc_sampler() -> (x_result, nfe)``.

    Extra keyword arguments over the reference: ``noise`` (complex64 [n_draws, *y.shape], consumed prior-first
    then per step corrector draws followed by the predictor draw) for bit-reproducible parity runs, ``seed`` for
    the device Philox generator, ``use_graph``.  ``per_item`` (default off): the batch-invariant form of the fused loop
    (``use_sample_items``) - item b draws from its own Philox stream seeded ``item_seeds[b]`` (default
    ``seeding.item_seed(seed, b)``) and takes its own Langevin step, so that at equal T' its result does not depend on
    the batch it rides in; at B > 1 this is the reference run per file (batch size 1), not the reference at batch size B.
    """
    predictor_cls = PredictorRegistry.get_by_name(predictor_name)
    corrector_cls = CorrectorRegistry.get_by_name(corrector_name)
    predictor = predictor_cls(sde, score_fn, probability_flow=probability_flow)
    corrector = corrector_cls(sde, score_fn, snr=snr, n_steps=corrector_steps)

    builtin = (isinstance(predictor, (_HipPredictor, NonePredictor)) and isinstance(corrector, (_HipCorrector, NoneCorrector))
               and type(predictor) in (PredictorRegistry.get_by_name(n) for n in ("reverse_diffusion", "euler_maruyama", "none"))
               and type(corrector) in (CorrectorRegistry.get_by_name(n) for n in ("langevin", "ald", "none")))
    from ..sdes import OUVESDE
    # the fused loop implements the OUVE dynamics of exactly this class (subclasses / other registered SDEs take the seam path);
    # its constants travel with the call so that the engine is rebuilt when they differ from the defaults
    fused = (builtin and type(sde) is OUVESDE and not probability_flow and denoise
             and getattr(score_fn, "supports_fused_sampler", False)
             and conditioning is not None and len(conditioning) in (1, 2) and all(c.shape == y.shape for c in conditioning))

    item_kw = {}
    if per_item:
        # the seam path below goes through use_sde_*, whose noise and Langevin step are those of the whole batch
        if not builtin:
            raise NotImplementedError(f"per_item sampling: predictor {predictor_name!r} / corrector {corrector_name!r} are not both "
                                      "built-in fused ones; the loop driven through update_fn stays batch-coupled")
        if not fused:
            raise NotImplementedError("per_item sampling runs in the fused loop only (HIP-backed ScoreModel, the OUVE SDE, denoise=True, "
                                      "no probability flow, conditioning of y's shape)")
        if item_seeds is None:
            from ...seeding import item_seeds as _derive
            item_seeds = _derive(seed, y.shape[0])
        if len(item_seeds) != y.shape[0]:
            raise ValueError(f"item_seeds has {len(item_seeds)} entries for a batch of {y.shape[0]}")
        item_kw = {"item_seeds": list(item_seeds)}
    elif item_seeds is not None:
        raise ValueError("item_seeds needs per_item=True")

    if fused:
        def pc_sampler():
            with torch.no_grad():
                x = score_fn.fused_sample(y, N=sde.N, predictor=predictor_name, corrector=corrector_name,
                                          corrector_steps=corrector_steps, snr=snr, t_eps=eps, noise=noise, seed=seed,
                                          use_graph=use_graph, sde=sde, cond=conditioning[0],
                                          cond2=conditioning[1] if len(conditioning) == 2 else None, **item_kw)
            return x, sde.N * (corrector.n_steps + 1)
        return pc_sampler

    def pc_sampler():
        with torch.no_grad():
            draw = 0

            def nz(k=1):
                nonlocal draw
                if noise is None:
                    draw += k
                    return None
                out = [noise[draw + i] for i in range(k)]
                draw += k
                return out

            z0 = nz()
            xt = sde.prior_sampling(y.shape, y, noise=None if z0 is None else z0[0], seed=seed)
            timesteps = torch.linspace(sde.T, eps, sde.N, device=y.device)
            xt_mean = xt
            for i in range(sde.N):
                vec_t = torch.ones(y.shape[0], device=y.device) * timesteps[i]
                if corrector.n_steps:
                    xt, xt_mean = corrector.update_fn(xt, vec_t, y, conditioning=conditioning, noise=nz(corrector.n_steps),
                                                      seed=seed + 1000 * (i + 1)) if isinstance(corrector, _HipCorrector) \
                        else corrector.update_fn(xt, vec_t, y, conditioning=conditioning)
                if isinstance(predictor, _HipPredictor):
                    zp = nz()
                    xt, xt_mean = predictor.update_fn(xt, vec_t, y, conditioning=conditioning,
                                                      noise=None if zp is None else zp[0], seed=seed + 1000 * (i + 1) + 999)
                else:
                    xt, xt_mean = predictor.update_fn(xt, vec_t, y, conditioning=conditioning)
            x_result = xt_mean if (denoise and sde.N) else xt
            return x_result, sde.N * (corrector.n_steps + 1)

    return pc_sampler


_ODE_SOLVER_OPTIONS = ("first_step", "max_step", "max_nfe")


def get_ode_sampler(sde, score_fn, y, inverse_scaler=None, denoise=True, rtol=1e-5, atol=1e-5, method="RK45", eps=3e-2,
                    device="cuda", conditioning=None, noise=None, seed=0, minibatch=None, use_graph=True, per_item=False,
                    item_seeds=None, **kwargs):
    """Returns ``ode_sampler() -> (x, nfe)``: the probability-flow ODE of ``sde`` integrated from T = 1 down to ``eps`` by RK45
    (scipy's ``solve_ivp(method="RK45")``, reproduced on the device), then with ``denoise`` one noise-free reverse-diffusion step.

    Over the reference: ``conditioning`` (the score's conditioning, as for ``get_pc_sampler``; the reference's drift calls
    ``score_model(x, t, y)``, which its own ``ScoreModel`` rejects - DESIGN.md section 7), ``noise`` (the prior's draw, complex64 like
    ``y``), ``seed`` (device Philox stream), ``minibatch`` (items per step-size controller: each group is its own integration with its
    own step sizes and NFE, as ``ScoreModel.get_ode_sampler(minibatch=k)`` runs them; ``None`` = one integration over the batch -
    then ``nfe`` is an int, else a list per group), ``use_graph``.  Solver options: scalar ``rtol`` / ``atol``, ``first_step``,
    ``max_step``, and ``max_nfe`` (evaluations per group before the integration stops with status -2, default 10000).  ``device`` is
    accepted for the reference's signature: the sampler runs on ``y``'s device.  ``ode_sampler.stats`` holds NFE and status per group
    after a call (0: reached ``eps``; -1: scipy's step-size failure, the last accepted state is returned; -2: ``max_nfe``), and on the
    seam path the accepted times (``solution.t``).  ``per_item`` (default off): the prior of item b is draw 0 of its own Philox
    stream (``item_seeds[b]``, default ``seeding.item_seed(seed, b)``), drawn with ``use_fill_noise_items`` and injected; needs
    ``minibatch=1`` and the fused path.
    """
    if method != "RK45":
        raise NotImplementedError(f"get_ode_sampler: method={method!r} is not implemented (RK45 only)")
    extra = sorted(k for k in kwargs if k not in _ODE_SOLVER_OPTIONS)
    if extra:
        raise NotImplementedError(f"get_ode_sampler: solver option(s) {extra} are not implemented")
    for name, v in (("rtol", rtol), ("atol", atol)):
        if not isinstance(v, (int, float)) and not (hasattr(v, "ndim") and v.ndim == 0):
            raise NotImplementedError(f"get_ode_sampler: {name} must be a scalar (vector tolerances are not implemented)")
    if float(getattr(sde, "T", 1)) != 1.0:
        raise NotImplementedError("get_ode_sampler: the device stepper integrates from T = 1")
    opts = {k: kwargs[k] for k in _ODE_SOLVER_OPTIONS if k in kwargs}
    group = 0 if minibatch is None else int(minibatch)
    if noise is not None and noise.dim() == y.dim() + 1:
        noise = noise[0]                     # the PC layout [n_draws, *y.shape]: the prior is draw 0

    from ..sdes import OUVESDE
    fused = (type(sde) is OUVESDE and getattr(score_fn, "supports_fused_sampler", False)
             and (conditioning is None or (len(conditioning) in (1, 2) and all(c.shape == y.shape for c in conditioning))))

    item_kw = {}
    if per_item:
        if minibatch != 1:
            raise ValueError(f"per_item ODE sampling needs minibatch=1, got {minibatch!r}: the items of a group share one step-size "
                             "controller and one error norm, so an item's steps would depend on its companions")
        if not fused:
            raise NotImplementedError("per_item ODE sampling runs in the fused path only (HIP-backed ScoreModel and the OUVE SDE)")
        if item_seeds is None:
            from ...seeding import item_seeds as _derive
            item_seeds = _derive(seed, y.shape[0])
        if len(item_seeds) != y.shape[0]:
            raise ValueError(f"item_seeds has {len(item_seeds)} entries for a batch of {y.shape[0]}")
        item_kw = {"item_seeds": list(item_seeds)}
    elif item_seeds is not None:
        raise ValueError("item_seeds needs per_item=True")

    def _nfe(nfev):
        return nfev[0] if minibatch is None else list(nfev)

    if fused:
        def ode_sampler():
            with torch.no_grad():
                cond = [None, None] if conditioning is None else list(conditioning) + [None]
                x, nfev, status = score_fn.fused_sample_ode(y, N=sde.N, t_eps=eps, rtol=rtol, atol=atol, group=group, denoise=denoise,
                                                            noise=noise, seed=seed, use_graph=use_graph, sde=sde, cond=cond[0],
                                                            cond2=cond[1], **opts, **item_kw)
                ode_sampler.stats = {"nfev": nfev, "status": status}
                if inverse_scaler is not None:
                    x = inverse_scaler(x)
            return x, _nfe(nfev)
        return ode_sampler

    def ode_sampler():
        from ...hip_engine import OdeStepper
        from .predictors import ReverseDiffusionPredictor
        with torch.no_grad():
            x0 = (sde.prior_sampling(y.shape, y, noise=noise, seed=seed) if isinstance(sde, OUVESDE)
                  else sde.prior_sampling(y.shape, y))
            rsde = sde.reverse(score_fn, probability_flow=True)
            kw = {} if conditioning is None else {"conditioning": conditioning}
            consts = sde if all(hasattr(sde, a) for a in ("theta", "sigma_min", "sigma_max")) else OUVESDE()
            stepper = OdeStepper(_sde_engine(consts, y.device), y, x0, rtol=rtol, atol=atol, t_eps=eps, N=sde.N, group=group,
                                 denoise=False, use_graph=False, **opts)
            try:
                # the reference's drift_fn: the reverse SDE's drift with probability_flow=True (sampling/__init__.py:112-114)
                x, nfev, status = stepper.run(lambda xs, t: rsde.sde(xs, t, y, **kw)[0])
                ode_sampler.stats = {"times": stepper.times, "nfev": nfev, "status": status}   # solution.t / nfev / status per group
            finally:
                stepper.close()
            if denoise:                      # one reverse-diffusion step at eps, x_mean (sampling/__init__.py:107-110)
                predictor = ReverseDiffusionPredictor(sde, score_fn, probability_flow=False)
                vec_eps = torch.ones(y.shape[0], device=y.device) * eps
                _, x = predictor.update_fn(x, vec_eps, y, **kw)
            if inverse_scaler is not None:
                x = inverse_scaler(x)
        return x, _nfe(nfev)
    return ode_sampler
