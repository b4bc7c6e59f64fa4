"""``ScoreModel`` with the constructor keys, methods and batch-dict contract of the reference's
``sgmse/model_wrapper.py:23-329`` -- STFT glue in core torch (as the reference: ``torch.stft`` :116-122), the
score network and the whole reverse-SDE loop in libuse_hip.so.

Additions over the reference (all optional, defaults reproduce stock behaviour): ``precision`` ("bf16" | "fp32"),
``use_graph``, ``noise`` / ``seed`` keywords on ``sample`` / ``enhance`` for reproducible runs, and ``chunk_frames`` / ``chunk_overlap`` /
``chunk_batch`` for chunked sampling of long recordings (``sample_spec_chunked``).  ``sampler_type="ode"`` runs the
probability-flow ODE sampler (RK45 on the device) with the score's conditioning, which the reference's own ODE path does not pass
(DESIGN.md section 7).
``train_step`` returns the loss with its tape once ``score_net.requires_grad_(True)`` was called (fp32 HIP operators forward and
backward: ``training.py``); with frozen parameters it is the forward-only value of the sampling engine.
"""
from __future__ import annotations

from math import ceil

import torch
import torch.nn as nn

from . import sampling
from .backbones import BackboneRegistry
from .sdes import SDERegistry
from .util.spectral import SpectralGlue, get_window  # noqa: F401  (get_window: part of the reference module's surface)


class ScoreModel(SpectralGlue, nn.Module):
    supports_fused_sampler = True

    def __init__(self, backbone: str = "ncsnpp", sde: str = "ouve", t_eps: float = 3e-2, mode="regen-joint-training",
                 condition="both", loss_type: str = "mse", n_fft=510, hop_length=128, num_frames=256, window="hann",
                 spec_factor=0.15, spec_abs_exponent=0.5, sde_input="denoised", predictor="reverse_diffusion",
                 corrector="none", precision="bf16", use_graph=True):
        super().__init__()
        input_channels = 6 if condition == "both" else 4
        self.score_net = (BackboneRegistry.get_by_name(backbone)(input_channels=input_channels, precision=precision)
                          if backbone != "none" else None)
        self.sde = SDERegistry.get_by_name(sde)()
        self.t_eps, self.condition, self.mode, self.loss_type = t_eps, condition, mode, loss_type
        self._init_spectral(n_fft, hop_length, num_frames, window, spec_factor, spec_abs_exponent)
        self.sde_input, self.predictor, self.corrector = sde_input, predictor, corrector
        self.precision, self.use_graph = precision, use_graph

    # STFT glue (reference :92-122): SpectralGlue

    # ---- score function (reference :135-145) -------------------------------------------------------------
    def forward_score(self, x, t, score_conditioning, sde_input):
        dnn_input = torch.cat([x] + list(score_conditioning), dim=1)
        return -self.score_net(dnn_input, t)

    def forward(self, x, t, score_conditioning, sde_input):
        return self.forward_score(x, t, score_conditioning, sde_input)

    def _loss(self, err):
        """Reference :124-133."""
        if self.loss_type == "mse":
            losses = torch.square(err.abs())
        elif self.loss_type == "mae":
            losses = err.abs()
        else:
            raise NotImplementedError(f"loss_type {self.loss_type!r}")
        return torch.mean(0.5 * torch.sum(losses.reshape(losses.shape[0], -1), dim=-1))

    def train_step(self, batch, t=None, z=None, start=None):
        """The denoising-score-matching loss of one batch (reference :147-208): crop / pad to ``target_len``, spectrograms,
        t ~ U(t_eps, T), x_t = mean(x0, t, y) + std(t) z, err = score(x_t) std + z, ``_loss(err)``.
        With gradients enabled and a trainable score network (``score_net.requires_grad_(True)``) the network runs on the
        differentiable fp32 HIP operators (``training.ncsnpp_forward_train``) and the loss carries the tape -- what
        ``SGMSEModule.training_step`` returns (SGMSE_module.py:46-54).  Otherwise (``validation_step`` / ``test_step``,
        SGMSE_module.py:56-63, or frozen parameters) it is the forward-only value from the sampling engine.
        ``t`` [B], ``z`` complex [B,1,F,T] and ``start`` override the random draws (the reference draws them from the global
        numpy / torch generators)."""
        if torch.is_grad_enabled() and getattr(self.score_net, "trainable", False):
            return self._train_step(batch, t, z, start)
        with torch.no_grad():
            return self._train_step(batch, t, z, start)

    def _train_step(self, batch, t, z, start):
        import numpy as np
        import torch.nn.functional as F
        x, y = batch["clean"], batch["perturbed"]
        y_denoised = batch.get("fake")
        # The reference feeds spec_fwd(stft(.)) of the target_len excerpt - exactly num_frames frames, NOT padded - to the network, whose
        # len(ch_mult) - 1 FIR down / up sampling stages only close for multiples of 2^(levels - 1) frames (64 for the 7-level NCSN++).  _spectrogram() would zero-pad another count silently
        # (extra frames in z, in the loss and in the network input): refuse it, as the reference's own forward pass fails there.
        ch_mult = getattr(self.score_net, "ch_mult", None)              # backbones without resampling stages take any frame count
        mult = 1 << (len(ch_mult) - 1) if ch_mult else 1
        if self.num_frames % mult != 0:
            raise ValueError(f"train_step: num_frames={self.num_frames} is not a multiple of {mult} frames (the excerpt's spectrogram must "
                             "enter the network unpadded, reference model_wrapper.py:168-171)")
        current_len = x.size(-1)
        pad = max(self.target_len - current_len, 0)
        if pad == 0:                                                     # a random target_len excerpt
            if start is None:
                start = int(np.random.uniform(0, current_len - self.target_len))
            cut = lambda a: a[..., start:start + self.target_len]       # noqa: E731
        else:                                                            # centre the short utterance in zeros
            cut = lambda a: F.pad(a, (pad // 2, pad // 2 + (pad % 2)), mode="constant")   # noqa: E731
        X, Y = self._spectrogram(cut(x).contiguous()), self._spectrogram(cut(y).contiguous())
        Yd = None if y_denoised is None else self._spectrogram(cut(y_denoised).contiguous())
        if self.sde_input == "denoised" and Yd is not None:
            sde_input = Yd
        elif self.sde_input == "noisy":
            sde_input = Y
        else:
            raise NotImplementedError(f"Don't know the sde input you have wished for: {self.sde_input}")
        if t is None:
            t = torch.rand(X.shape[0], device=X.device) * (self.sde.T - self.t_eps) + self.t_eps
        t = t.to(device=X.device, dtype=torch.float32)
        mean, std = self.sde.marginal_prob(X, t, sde_input)
        if z is None:
            z = torch.randn_like(X)                                      # complex: variance 1/2 per component
        sigmas = std.view(-1, 1, 1, 1)
        perturbed = mean + sigmas * z
        if self.condition == "noisy":
            score_conditioning = [Y]
        elif self.condition == "denoised" and Yd is not None:
            score_conditioning = [Yd]
        elif self.condition == "both" and Yd is not None:
            score_conditioning = [Y, Yd]
        else:
            raise NotImplementedError(f"Don't know the conditioning you have wished for: {self.condition}")
        score = self.forward_score(perturbed, t, score_conditioning, sde_input)
        return self._loss(score * sigmas + z)

    # ---- samplers (reference :210-260) -------------------------------------------------------------------
    def fused_sample(self, y, N, predictor, corrector, corrector_steps, snr, t_eps, noise=None, seed=0, use_graph=True,
                     sde=None, cond=None, cond2=None, item_seeds=None):
        """Whole PC loop inside libuse_hip.so (``use_sample_cond2``), with the OUVE constants of ``sde`` (default: ``self.sde``);
        ``cond``: the score conditioning when it is not ``y`` itself; ``cond2``: the second one of condition="both".
        ``item_seeds`` (B integers): the batch-invariant form (``use_sample_items``; an injected ``noise`` takes their place)."""
        sde = self.sde if sde is None else sde
        eng = self.score_net.engine(y.shape[2], y.device, sde_constants=(sde.theta, sde.sigma_min, sde.sigma_max))
        eng.plan(y.shape[0], y.shape[3])
        eng.set_sampler(N, predictor, corrector, corrector_steps, snr, t_eps, use_graph=use_graph)
        if item_seeds is not None:
            return eng.sample(y, noise=noise, cond=cond, cond2=cond2, item_seeds=item_seeds, per_item=True)
        return eng.sample(y, noise=noise, seed=seed, cond=cond, cond2=cond2)

    def get_pc_sampler(self, predictor_name, corrector_name, y, N=None, minibatch=None, **kwargs):
        N = self.sde.N if N is None else N
        sde = self.sde.copy()
        sde.N = N
        kwargs = {"eps": self.t_eps, "use_graph": self.use_graph, **kwargs}
        if minibatch is None:
            return sampling.get_pc_sampler(predictor_name, corrector_name, sde=sde, score_fn=self, y=y, **kwargs)
        M = y.shape[0]
        cond = kwargs.pop("conditioning", None)
        seeds = kwargs.pop("item_seeds", None)
        if kwargs.get("per_item") and seeds is None:        # named by the item's index in the whole batch, not in its minibatch
            from ..seeding import item_seeds as derive_item_seeds
            seeds = derive_item_seeds(kwargs.get("seed", 0), M)

        def batched_sampling_fn():
            samples, ns = [], []
            for i in range(int(ceil(M / minibatch))):
                y_mini = y[i * minibatch:(i + 1) * minibatch]
                c_mini = None if cond is None else [y_mini if c is y else c[i * minibatch:(i + 1) * minibatch] for c in cond]
                if seeds is not None:
                    kwargs["item_seeds"] = list(seeds[i * minibatch:(i + 1) * minibatch])
                sample, n = sampling.get_pc_sampler(predictor_name, corrector_name, sde=sde, score_fn=self, y=y_mini,
                                                    conditioning=c_mini, **kwargs)()
                samples.append(sample); ns.append(n)
            return torch.cat(samples, dim=0), ns
        return batched_sampling_fn

    def fused_sample_ode(self, y, N, t_eps, group=0, rtol=1e-5, atol=1e-5, denoise=True, noise=None, seed=0, use_graph=True, sde=None,
                         cond=None, cond2=None, first_step=None, max_step=None, max_nfe=0, item_seeds=None):
        """Probability-flow ODE sampler inside libuse_hip.so (``use_sample_ode``): RK45 with one step-size controller per ``group``
        items (0: the batch); returns (x, nfev per group, status per group).  ``item_seeds``: the prior of item b is draw 0 of its
        own noise stream (``use_fill_noise_items``), injected as ``noise``."""
        sde = self.sde if sde is None else sde
        eng = self.score_net.engine(y.shape[2], y.device, sde_constants=(sde.theta, sde.sigma_min, sde.sigma_max))
        eng.plan(y.shape[0], y.shape[3])
        eng.set_ode(rtol=rtol, atol=atol, t_eps=t_eps, N=N, group=group, denoise=denoise, first_step=first_step, max_step=max_step,
                    max_nfe=max_nfe, use_graph=use_graph)
        if item_seeds is not None and noise is None:
            noise = eng.fill_noise_items(item_seeds, 0, y.shape)
        return eng.sample_ode(y, noise=noise, seed=seed, cond=cond, cond2=cond2)

    def get_ode_sampler(self, y, N=None, minibatch=1, **kwargs):
        """Reference :238-260: ``(x, [nfe per minibatch])``, or ``(x, nfe)`` for ``minibatch=None``.  Every minibatch is its own RK45
        integration, as the reference's loop makes it - here one fused call with one step-size controller per minibatch."""
        N = self.sde.N if N is None else N
        sde = self.sde.copy()
        sde.N = N
        kwargs = {"eps": self.t_eps, "use_graph": self.use_graph, **kwargs}
        return sampling.get_ode_sampler(sde, self, y=y, minibatch=minibatch, **kwargs)

    def sample_spec_chunked(self, sde_input, conditioning, sampler_type="pc", N=50, corrector_steps=1, snr=0.5, noise=None, seed=0,
                            chunk_frames=512, chunk_overlap=64, chunk_batch=8, predictor=None, corrector=None, per_item=False,
                            item_seeds=None, **ode_kwargs):
        """Chunked sampling at the spectrogram level (no reference counterpart; ``chunking``): ``sde_input`` [B,1,F,T'] and every tensor
        of ``conditioning`` are cut into n windows of ``chunk_frames`` frames, ``chunk_overlap`` frames shared by neighbours
        (``use_chunk_split``); the B * n windows run through the un-chunked sampler (``fused_sample`` / ``fused_sample_ode`` for the
        built-in predictors and correctors) in groups of at most ``chunk_batch`` consecutive windows - the last group may be smaller -
        and the results are cross-faded into one [B,1,F,T'] spectrogram (``use_chunk_merge``).  One plan and one captured graph per
        (group size, chunk_frames) serve every file length.  T' <= ``chunk_frames``: one window, i.e. the un-chunked sampler itself.

        Group ``g`` samples with ``seed + g``.  An injected ``noise`` has the sampler's usual layout over all B * n windows
        ([n_draws, B*n, 1, F, chunk_frames] for "pc", the prior's draw [B*n, 1, F, chunk_frames] for "ode") and is sliced per group.
        The step size of the Langevin / annealed-Langevin corrector is a mean over the group, as it is over any batch of the
        un-chunked sampler (``sampling/correctors.py``: norms averaged over the batch): the windows of a group are coupled exactly as
        the utterances of a batch are, so a window's result depends on ``chunk_batch`` and on its neighbours in the group.  Overlapping
        frames of neighbouring windows draw independent noise.  ``self.last_nfe``: the NFE of every group.

        ``per_item=True`` removes that coupling (``use_sample_items``): window k of item b samples with
        ``seeding.window_seed(item_seeds[b], k)`` (``item_seeds`` default: ``seeding.item_seed(seed, b)``) and takes its own Langevin
        step, and every window has the same T' = ``chunk_frames``, so an item's merged result does not depend on ``chunk_batch`` nor
        on the other items of the call.  With one window (T' <= ``chunk_frames``) the items sample with ``item_seeds`` themselves."""
        from ..chunking import chunk_plan, map_chunked
        predictor = self.predictor if predictor is None else predictor
        corrector = self.corrector if corrector is None else corrector
        if sampler_type not in ("pc", "ode"):
            raise NotImplementedError(f"{sampler_type} is not a valid sampler type!")
        if sampler_type == "pc" and ode_kwargs:
            raise TypeError(f"sample(sampler_type='pc') got ODE sampler options {sorted(ode_kwargs)}")

        inputs = [sde_input] + list(conditioning)
        plan = chunk_plan(int(sde_input.shape[3]), chunk_frames, chunk_overlap)
        if per_item:
            from ..seeding import item_seeds as derive_item_seeds, window_seed
            if item_seeds is None:
                item_seeds = derive_item_seeds(seed, sde_input.shape[0])
            if len(item_seeds) != sde_input.shape[0]:
                raise ValueError(f"item_seeds has {len(item_seeds)} entries for a batch of {sde_input.shape[0]}")
            # window w of the split is window w % n of item w // n
            wseeds = list(item_seeds) if plan.n == 1 else [window_seed(s, k) for s in item_seeds for k in range(plan.n)]
        elif item_seeds is not None:
            raise ValueError("item_seeds needs per_item=True")

        def run(g, lo, hi, windows):
            y, cond = windows[0], windows[1:]
            z = None if noise is None else (noise[:, lo:hi] if noise.dim() == y.dim() + 1 else noise[lo:hi])
            kw = {"seed": seed + g} if not per_item else {"seed": seed, "per_item": True, "item_seeds": wseeds[lo:hi]}
            if sampler_type == "pc":
                return self.get_pc_sampler(predictor, corrector, y, N=N, corrector_steps=corrector_steps, snr=snr, intermediate=False,
                                           conditioning=cond, noise=z, **kw)()
            return self.get_ode_sampler(y, N=N, conditioning=cond, noise=z, **kw, **ode_kwargs)()

        if plan.n == 1:
            sample, nfe = run(0, 0, sde_input.shape[0], inputs)
            self.last_nfe = [nfe]
            return sample
        total = sde_input.shape[0] * plan.n
        if noise is not None and noise.shape[noise.dim() - 4] != total:
            raise ValueError(f"noise has shape {tuple(noise.shape)}: chunked sampling takes the sampler's layout over all {total} windows "
                             f"of {plan.chunk_frames} frames ({plan.n} per item)")
        sample, self.last_nfe = map_chunked(run, inputs, chunk_frames, chunk_overlap, chunk_batch)
        return sample

    def _chunked(self, Tp, chunk_frames, chunk_overlap, chunk_batch):
        """True when the call is to be chunked: ``chunk_frames`` given (its arguments are checked either way) and T' above it."""
        if chunk_frames is None:
            return False
        from ..chunking import check_chunk_batch, chunk_plan
        check_chunk_batch(chunk_batch)
        return chunk_plan(int(Tp), chunk_frames, chunk_overlap).n > 1

    def sample(self, batch, sampler_type="pc", N=50, corrector_steps=1, snr=0.5, noise=None, seed=0, chunk_frames=None,
               chunk_overlap=64, chunk_batch=8, per_item=False, item_seeds=None, own_length=False, **ode_kwargs):
        """Reference :262-329: adds ``batch['enhanced']`` (float32 [B, L]) for condition / sde_input 'noisy'.
        ``sampler_type="ode"``: the probability-flow ODE sampler (``get_ode_sampler``; ``ode_kwargs``: ``rtol``, ``atol``,
        ``minibatch`` (default 1), ``first_step``, ``max_step``, ``max_nfe``); its NFE is left in ``self.last_nfe``.
        ``chunk_frames`` (a multiple of 64; default ``None``: off) samples recordings of more padded frames than that in overlapping
        windows (``sample_spec_chunked``, which documents ``chunk_overlap``, ``chunk_batch``, the seed rule and the noise layout);
        shorter ones take the un-chunked path, bit-identically.
        ``per_item`` (default off) / ``item_seeds``: batch-invariant sampling (``sampling.get_pc_sampler``) - every item has its own noise
        stream and its own Langevin step, so that at equal padded frame count T' its result does not depend on the batch it rides in.
        Zero padding to the batch's longest item changes T' and with it what the network sees: un-chunked batches of unequal lengths
        are composition-dependent through T' unless ``own_length`` is set.

        ``own_length`` (default off) runs every item at its own padded frame count: the items are grouped by
        ``T' = pad64(1 + batch["sample_length"][b] // hop)`` (``length_groups``; a missing key raises ``ValueError``), item b is analysed
        over its own ``sample_length[b]`` samples with the reflect padding at its own end (``use_stft_fwd_items``), and each group runs
        through the code path above at its own T', the groups one after the other in ascending T'; the results are scattered into
        ``enhanced`` [B, Lmax], zero past each item's length.  Under ``per_item`` an item keeps the seed it has in the whole batch
        (``item_seeds[b]``, or the one derived from ``seed`` and b), so its samples are those of ``sample`` called on that item alone,
        whatever its companions, their order and the batch size.  Without ``per_item``, group g samples with ``seed + g`` (the rule chunk
        groups follow) and the items of a group are coupled as the items of a batch are: the Langevin step is a mean over the group.
        An injected ``noise`` has the layout of one plan shape, so it raises ``ValueError`` when the batch forms more than one group.
        ``self.last_groups``: ``[(T', items), ...]``; ``self.last_nfe``: a list with one entry per group."""
        item_kw = {"per_item": True, "item_seeds": item_seeds} if per_item else {}
        if item_seeds is not None and not per_item:
            raise ValueError("item_seeds needs per_item=True")
        run_kw = dict(sampler_type=sampler_type, N=N, corrector_steps=corrector_steps, snr=snr, chunk_frames=chunk_frames,
                      chunk_overlap=chunk_overlap, chunk_batch=chunk_batch, ode_kwargs=ode_kwargs)
        if own_length:
            return self._sample_own_length(batch, noise, seed, per_item, item_seeds, run_kw)
        y = batch["perturbed"]
        T_orig = y.size(1)
        Y = self._spectrogram(y)
        Y_denoised = self._spectrogram(batch["fake"]) if "fake" in batch else None
        sample, key = self._sample_spectrograms(Y, Y_denoised, noise=noise, seed=seed, item_kw=item_kw, **run_kw)
        batch[key] = self._waveform(sample, T_orig)
        return batch

    def _sample_own_length(self, batch, noise, seed, per_item, item_seeds, run_kw):
        """``sample(own_length=True)``: one pass of ``_sample_spectrograms`` per group of equal T'."""
        if "sample_length" not in batch:
            raise ValueError("own_length=True needs batch['sample_length'] (the valid samples of every item)")
        y = batch["perturbed"]
        B, stride = y.shape
        lens = [int(v) for v in (batch["sample_length"].tolist() if hasattr(batch["sample_length"], "tolist") else batch["sample_length"])]
        if len(lens) != B:
            raise ValueError(f"sample_length has {len(lens)} entries for a batch of {B}")
        for b, L in enumerate(lens):
            if L > stride:
                raise ValueError(f"item {b}: sample_length {L} exceeds the {stride} samples of a row")
        groups = self.length_groups(lens)
        if noise is not None and len(groups) > 1:
            raise ValueError(f"an injected noise tensor has the layout of one plan shape; this batch forms {len(groups)} groups "
                             f"(T' = {[Tp for Tp, _ in groups]})")
        if per_item:
            if item_seeds is None:
                from ..seeding import item_seeds as derive_item_seeds
                item_seeds = derive_item_seeds(seed, B)                      # named by the item's index in the whole batch
            if len(item_seeds) != B:
                raise ValueError(f"item_seeds has {len(item_seeds)} entries for a batch of {B}")
        out, key, nfes = None, None, []
        for g, (Tp, idx) in enumerate(groups):
            whole = len(idx) == B
            sel = None if whole else torch.as_tensor(idx, device=y.device)
            take = lambda a: a if whole else a.index_select(0, sel)         # noqa: E731
            glens = [lens[i] for i in idx]
            Y = self._spectrogram_items(take(y), glens, Tp)
            Y_denoised = self._spectrogram_items(take(batch["fake"]), glens, Tp) if "fake" in batch else None
            item_kw = {"per_item": True, "item_seeds": [item_seeds[i] for i in idx]} if per_item else {}
            sample, key = self._sample_spectrograms(Y, Y_denoised, noise=noise, seed=seed if per_item else seed + g, item_kw=item_kw,
                                                    **run_kw)
            nfes.append(self.last_nfe)
            wav = self._waveform_items(sample, glens, stride)
            if whole:
                out = wav
            else:
                out = torch.zeros((B, stride), dtype=wav.dtype, device=wav.device) if out is None else out
                out.index_copy_(0, sel, wav)
        self.last_groups = [(Tp, len(idx)) for Tp, idx in groups]
        self.last_nfe = nfes
        batch[key] = out
        return batch

    def _sample_spectrograms(self, Y, Y_denoised, sampler_type, N, corrector_steps, snr, noise, seed, chunk_frames, chunk_overlap,
                             chunk_batch, item_kw, ode_kwargs):
        """The sampler between the analysis and the synthesis of ``sample``: -> (spectrogram [B,1,F,T'], the batch key of the result);
        the NFE is left in ``self.last_nfe``."""
        # conditioning (reference :283-291): the spectrogram(s) the network sees beside x
        if self.condition == "noisy":
            score_conditioning = [Y]
        elif self.condition == "denoised" and Y_denoised is not None:
            score_conditioning = [Y_denoised]
        elif self.condition == "both" and Y_denoised is not None:
            score_conditioning = [Y, Y_denoised]
        else:
            raise NotImplementedError(f"Don't know the conditioning you have wished for: {self.condition}")
        # the SDE's y (reference :293-300)
        if self.sde_input == "denoised" and Y_denoised is not None:
            sde_input = Y_denoised
        elif self.sde_input == "noisy":
            sde_input = Y
        else:
            raise NotImplementedError(f"Don't know the sde input you have wished for: {self.sde_input}")
        # reference :320-328: the key depends on what the SDE started from
        key = "fake_sde_enhanced" if (self.sde_input == "denoised" and Y_denoised is not None) else "enhanced"
        if self._chunked(sde_input.shape[3], chunk_frames, chunk_overlap, chunk_batch):
            sample = self.sample_spec_chunked(sde_input, score_conditioning, sampler_type=sampler_type, N=N, corrector_steps=corrector_steps,
                                              snr=snr, noise=noise, seed=seed, chunk_frames=chunk_frames, chunk_overlap=chunk_overlap,
                                              chunk_batch=chunk_batch, **item_kw, **ode_kwargs)
            return sample, key
        if sampler_type == "pc":
            if ode_kwargs:
                raise TypeError(f"sample(sampler_type='pc') got ODE sampler options {sorted(ode_kwargs)}")
            sampler = self.get_pc_sampler(self.predictor, self.corrector, sde_input, N=N, corrector_steps=corrector_steps, snr=snr,
                                          intermediate=False, conditioning=score_conditioning, noise=noise, seed=seed, **item_kw)
        elif sampler_type == "ode":                                      # reference :314-316
            sampler = self.get_ode_sampler(sde_input, N=N, conditioning=score_conditioning, noise=noise, seed=seed, **item_kw, **ode_kwargs)
        else:
            raise NotImplementedError(f"{sampler_type} is not a valid sampler type!")
        sample, nfe = sampler()
        self.last_nfe = nfe
        return sample, key

    @torch.no_grad()
    def enhance(self, y, sampler_type="pc", predictor="reverse_diffusion", corrector="ald", N=50, corrector_steps=1,
                snr=0.5, timeit=False, return_stft=False, noise=None, seed=0, sr=24000, chunk_frames=None, chunk_overlap=64,
                chunk_batch=8, per_item=False, item_seeds=None, **kwargs):
        """One-call enhancement of noisy speech ``y`` [1, L] -- keyword surface of the legacy
        ``ScoreModel.enhance`` (reference ``sgmse/model.py:351-402``).  ``chunk_frames`` / ``chunk_overlap`` / ``chunk_batch``: chunked
        sampling of a long recording, as for ``sample`` (``sample_spec_chunked``).  As un-chunked, ``kwargs`` are the ODE sampler's options
        and are ignored for "pc"; with ``timeit`` the NFE of a chunked "pc" run is the int every group took (the step count fixes it),
        that of a chunked "ode" run a list with one entry per group, each what the un-chunked call returns.  ``per_item`` /
        ``item_seeds``: batch-invariant sampling, as for ``sample``."""
        item_kw = {"per_item": True, "item_seeds": item_seeds} if per_item else {}
        if item_seeds is not None and not per_item:
            raise ValueError("item_seeds needs per_item=True")
        import time
        start = time.time()
        T_orig = y.size(1)
        norm_factor = y.abs().max().item()
        y = y / norm_factor
        if not y.is_cuda:
            y = y.cuda()
        Y = self._spectrogram(y)
        if self._chunked(Y.shape[3], chunk_frames, chunk_overlap, chunk_batch):
            sample = self.sample_spec_chunked(Y, [Y], sampler_type=sampler_type, N=N, corrector_steps=corrector_steps, snr=snr, noise=noise,
                                              seed=seed, chunk_frames=chunk_frames, chunk_overlap=chunk_overlap, chunk_batch=chunk_batch,
                                              predictor=predictor, corrector=corrector, **item_kw, **(kwargs if sampler_type == "ode" else {}))
            nfe = self.last_nfe[0] if sampler_type == "pc" else self.last_nfe
        elif sampler_type == "pc":
            sample, nfe = self.get_pc_sampler(predictor, corrector, Y, N=N, corrector_steps=corrector_steps, snr=snr,
                                              intermediate=False, conditioning=[Y], noise=noise, seed=seed, **item_kw)()
        elif sampler_type == "ode":                                      # legacy model.py:384-385
            sample, nfe = self.get_ode_sampler(Y, N=N, conditioning=[Y], noise=noise, seed=seed, **item_kw, **kwargs)()
        else:
            raise NotImplementedError(f"{sampler_type} is not a valid sampler type!")
        if return_stft:
            return sample.squeeze(), Y.squeeze(), T_orig, norm_factor
        x_hat = (self._waveform(sample, T_orig) * norm_factor).squeeze().cpu()
        if timeit:
            return x_hat, nfe, (time.time() - start) / (len(x_hat) / sr)
        return x_hat
