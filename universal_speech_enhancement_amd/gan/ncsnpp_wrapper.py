"""``NCSNPP_Wrapper`` with the constructor and inference contract of the reference's
``src/models/components/GAN/generator/ncsnpp/model_wrapper.py:19-121``: STFT -> compress -> pad to a multiple of 64 frames ->
``NCSNpp(discriminative=True)`` (one network evaluation in libuse_hip.so) -> decompress -> iSTFT, adding ``batch["fake"]``.

The training branch (random crops of ``clean`` / ``perturbed`` pairs, reference lines 88-112) is outside the scope of the
library and raises; the state-dict keys (``net.all_modules...``, ``net.output_layer...``) are the reference's.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..sgmse.backbones.ncsnpp import NCSNpp
from ..sgmse.util.spectral import SpectralGlue, get_window  # noqa: F401


class NCSNPP_Wrapper(SpectralGlue, nn.Module):
    def __init__(self, n_fft=510, hop_length=128, num_frames=256, window="hann", spec_factor=0.15, spec_abs_exponent=0.5,
                 precision="bf16"):
        super().__init__()
        self._init_spectral(n_fft, hop_length, num_frames, window, spec_factor, spec_abs_exponent)
        self.net = NCSNpp(discriminative=True, precision=precision)

    @torch.no_grad()
    def refine_spec_chunked(self, spec, chunk_frames=512, chunk_overlap=64, chunk_batch=8, per_image=False):
        """The network over a long spectrogram [B,1,F,T'] in overlapping windows (``chunking``, as ``ScoreModel.sample_spec_chunked``):
        split, one forward pass per group of at most ``chunk_batch`` windows, cross-fade merge.  T' <= ``chunk_frames``: one pass.
        ``per_image``: every pass with the kernel forms of a batch of one (``use_forward_items``)."""
        from ..chunking import chunk_plan, map_chunked
        net = (lambda x: self.net(x, per_image=True)) if per_image else self.net
        if chunk_plan(int(spec.shape[3]), chunk_frames, chunk_overlap).n == 1:
            return net(spec.contiguous())
        return map_chunked(lambda g, lo, hi, windows: (net(windows[0].contiguous()), None), [spec], chunk_frames, chunk_overlap,
                           chunk_batch)[0]

    @torch.no_grad()
    def forward(self, batch_data: dict, chunk_frames=None, chunk_overlap=64, chunk_batch=8, own_length=False) -> dict:
        """``chunk_frames`` (default ``None``: off): recordings of more padded frames than that pass the network in windows
        (``refine_spec_chunked``); shorter ones take the one pass below, bit-identically.
        ``own_length`` (default off): every item at its own padded frame count, as for ``ScoreModel.sample`` - the items are grouped by
        ``T' = pad64(1 + batch_data["sample_length"][b] // hop)`` (``length_groups``; a missing key raises ``ValueError``), each group
        is one pass at its own T' over spectrograms analysed at the items' own lengths, and ``fake`` [B, Lmax] is zero past each item's
        length, and the network runs with the kernel forms of a batch of one (``use_forward_items``): a row is what the call gives
        that item alone.  ``self.last_groups``: ``[(T', items), ...]``."""
        if "clean" in batch_data:
            raise NotImplementedError("the training branch of NCSNPP_Wrapper is outside the scope of the MI355X library")
        noisy = batch_data["perturbed"]
        if own_length:
            if "sample_length" not in batch_data:
                raise ValueError("own_length=True needs batch['sample_length'] (the valid samples of every item)")
            B, stride = noisy.shape
            sl = batch_data["sample_length"]
            lens = [int(v) for v in (sl.tolist() if hasattr(sl, "tolist") else sl)]
            if len(lens) != B or any(L > stride for L in lens):
                raise ValueError(f"sample_length {lens} does not fit a batch of {B} rows of {stride} samples")
            groups = self.length_groups(lens)
            out = None
            for Tp, idx in groups:
                whole = len(idx) == B
                sel = None if whole else torch.as_tensor(idx, device=noisy.device)
                glens = [lens[i] for i in idx]
                spec = self._spectrogram_items(noisy if whole else noisy.index_select(0, sel), glens, Tp)
                # the kernel forms of a batch of one: a row must not depend on how many items share its T'
                refined = (self.net(spec.contiguous(), per_image=True) if chunk_frames is None else
                           self.refine_spec_chunked(spec, chunk_frames, chunk_overlap, chunk_batch, per_image=True))
                wav = self._waveform_items(refined, glens, stride)
                if whole:
                    out = wav
                else:
                    out = torch.zeros((B, stride), dtype=wav.dtype, device=wav.device) if out is None else out
                    out.index_copy_(0, sel, wav)
            self.last_groups = [(Tp, len(idx)) for Tp, idx in groups]
            batch_data["fake"] = out
            return batch_data
        if chunk_frames is None:
            refined = self.net(self._spectrogram(noisy).contiguous())
        else:
            refined = self.refine_spec_chunked(self._spectrogram(noisy), chunk_frames, chunk_overlap, chunk_batch)
        batch_data["fake"] = self._waveform(refined, noisy.size(1))
        return batch_data
