#!/usr/bin/env python3
"""Golden vectors of the convergence losses -- runs ONLY in the build container (needs the reference checkout).

Same method as ``scripts/gen_golden_metrics.py``: the reference's own ``WavSpecConvergence_Loss``
(``src/models/components/loss_function/monaural_loss.py:59-178``) is imported and called with every alpha at 1 on seeded signals.  Data
only is written: ``tests/golden/spec_losses.npz``.

    python scripts/gen_golden_spec_losses.py --reference <reference checkout>      (or USE_REFERENCE_DIR=<reference checkout>)

What is the reference's and what is not.  The loss arithmetic - the L1 / MSE modules, the logs, the norms, the sums over resolutions and
the weighting - is the reference's code.  torchaudio is not installed where this runs, so ``torchaudio.transforms.Spectrogram`` and
``MelSpectrogram`` are in-memory stand-ins, a RESTATEMENT of torchaudio built on ``torch.stft`` (periodic Hann of ``win_length`` centred
in the frame, ``center=True``, reflect padding, one-sided, not normalised, magnitude) and on the ``melscale_fbanks`` formula (HTK scale,
``norm=None``), both in the dtype of the input.  The module ``hifigan_dicriminator``, which the file imports and this class never uses,
is an empty stub.

Stored per case (shapes and lengths: ``tests/spec_losses_ref.py: CASES``):
  est, clean     float32 [B, stride], zero past an item's length (signal recipe: ``spec_losses_ref.signals``)
  ref_f32        [B, 6] the class's six terms on item b alone, trimmed to its length, in float32 (``spec_losses_ref.TERMS`` order)
  f32_vs_f64     [B, 6] per term, the distance between that run and the same modules run in float64: the reference's own rounding
                 sensitivity, which the tests use as the scale of their bounds against ``ref_f32``
  batch          (``edge`` only) [7] the class on the whole batch at full width, float32: the six terms and their sum, and
                 ``edge_batch_f32_vs_f64`` [7], their distance to the float64 run
Asserted here (change the signals if they fail, do not loosen them): over every magnitude and mel map of both signals the smallest value
is >= 1e-7 and mean(1 / M) <= 1e3, so that the logs are well-conditioned; and the float32 restatement used for ``f32_vs_f64`` gives the
class's own float32 result bit for bit."""
import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "spec_losses.npz")


def install_stand_ins():
    import torch

    class Spectrogram(torch.nn.Module):
        def __init__(self, n_fft=400, win_length=None, hop_length=None, power=2.0):
            super().__init__()
            assert power == 1, "the convergence loss uses magnitudes"
            self.n_fft, self.win_length = n_fft, win_length or n_fft
            self.hop_length = hop_length or self.win_length // 2

        def forward(self, x):
            w = torch.hann_window(self.win_length, periodic=True, dtype=x.dtype, device=x.device)
            return torch.stft(x, self.n_fft, hop_length=self.hop_length, win_length=self.win_length, window=w, center=True,
                              pad_mode="reflect", normalized=False, onesided=True, return_complex=True).abs()

    def melscale_fbanks(n_freqs, f_min, f_max, n_mels, dtype):
        all_freqs = torch.linspace(0, f_max, n_freqs, dtype=dtype)
        m_min, m_max = 2595.0 * np.log10(1.0 + f_min / 700.0), 2595.0 * np.log10(1.0 + f_max / 700.0)
        f_pts = 700.0 * (10.0 ** (torch.linspace(m_min, m_max, n_mels + 2, dtype=dtype) / 2595.0) - 1.0)
        f_diff = f_pts[1:] - f_pts[:-1]
        slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
        return torch.clamp(torch.min(-slopes[:, :-2] / f_diff[:-1], slopes[:, 2:] / f_diff[1:]), min=0.0)

    class MelSpectrogram(torch.nn.Module):
        def __init__(self, sample_rate=16000, n_fft=400, win_length=None, hop_length=None, f_min=0.0, f_max=None, n_mels=128, power=2.0):
            super().__init__()
            self.spectrogram = Spectrogram(n_fft=n_fft, win_length=win_length, hop_length=hop_length, power=power)
            self.n_freqs, self.f_min, self.f_max, self.n_mels = n_fft // 2 + 1, f_min, f_max or sample_rate // 2, n_mels

        def forward(self, x):
            fb = melscale_fbanks(self.n_freqs, self.f_min, self.f_max, self.n_mels, x.dtype)
            return torch.matmul(self.spectrogram(x).transpose(-1, -2), fb).transpose(-1, -2)

    ta, tr = types.ModuleType("torchaudio"), types.ModuleType("torchaudio.transforms")
    tr.Spectrogram, tr.MelSpectrogram = Spectrogram, MelSpectrogram
    ta.transforms = tr
    sys.modules["torchaudio"], sys.modules["torchaudio.transforms"] = ta, tr
    chain = "src.models.components.GAN.discriminator.hifigan_vocoder.hifigan_dicriminator".split(".")
    for i in range(4, len(chain) + 1):                        # the packages above the stub, then the stub itself
        sys.modules.setdefault(".".join(chain[:i]), types.ModuleType(".".join(chain[:i])))
    stub = sys.modules[".".join(chain)]
    for name in ("hifigan_vocoder_discriminator_adv_dsc_loss", "hifigan_vocoder_discriminator_adv_gen_loss",
                 "hifigan_vocoder_discriminator_feat_loss"):
        setattr(stub, name, object)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("USE_REFERENCE_DIR"), help="the reference project's checkout")
    a = ap.parse_args()
    if not a.reference:
        ap.error("--reference (or USE_REFERENCE_DIR) is required")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, a.reference)
    install_stand_ins()

    import torch

    import spec_losses_ref as sr_
    from src.models.components.loss_function.monaural_loss import WavSpecConvergence_Loss

    torch.set_num_threads(8)

    def run_class(loss, est, clean):
        """The class's forward on float32 [B, L] -> its six terms and their sum."""
        out = loss({"clean": torch.from_numpy(clean), "fake": torch.from_numpy(est)})
        return np.array([float(out[f"loss_G_{k}"]) for k in sr_.TERMS] + [float(out["loss_G"])])

    def terms_as(loss, est, clean, dtype):
        """calc_convergence_loss with the class's own modules and accumulators of ``dtype`` (the class accumulates in float32 whatever
        the input is, which would round a float64 run); also the floor and mean(1 / M) over every map of both signals."""
        e, c = torch.from_numpy(est).to(dtype), torch.from_numpy(clean).to(dtype)
        l2, lg, nm = (torch.zeros((), dtype=dtype) for _ in range(3))
        floor, inv = np.inf, 0.0
        xforms = list(loss._stft_xforms) + [loss._melspec_xform]
        for x in xforms:
            me, mc = x(e), x(c)
            floor = min(floor, float(me.min()), float(mc.min()))
            inv = max(inv, float((1.0 / me).mean()), float((1.0 / mc).mean()))
            if x is loss._melspec_xform:
                mel_log = loss._l1_loss(torch.log(me * 32768 + 1e-6), torch.log(mc * 32768 + 1e-6))
                mel_l2 = loss._l2_loss(me, mc)
            else:
                l2 += loss._l2_loss(me, mc)
                lg += loss._l1_loss(torch.log(me * 32768 + 1e-6), torch.log(mc * 32768 + 1e-6))
                nm += (((mc - me) ** 2).sum(-1).sum(-1).sqrt() / ((mc ** 2).sum(-1).sum(-1).sqrt() + 1e-6)).mean()
        lg /= 4
        nm /= 4
        return np.array([float(v) for v in (loss._l1_loss(e, c), l2, lg, nm, mel_log, mel_l2)]), floor, inv

    out = {}
    for case, rate, B, stride, lengths in sr_.CASES:
        loss = WavSpecConvergence_Loss(sampling_rate=rate)     # every alpha 1
        est, clean = np.zeros((B, stride), np.float32), np.zeros((B, stride), np.float32)
        ref, sens = np.zeros((B, 6)), np.zeros((B, 6))
        for b, L in enumerate(lengths):
            est[b, :L], clean[b, :L] = sr_.signals(case, b, L, rate)
            e, c = est[b:b + 1, :L].copy(), clean[b:b + 1, :L].copy()
            got = run_class(loss, e, c)
            t32, _, _ = terms_as(loss, e, c, torch.float32)
            t64, floor, inv = terms_as(loss, e, c, torch.float64)
            assert np.array_equal(t32, got[:6]), (case, b, t32, got)    # the restatement above IS the class's arithmetic
            assert floor >= sr_.MAG_FLOOR, (case, b, floor)
            assert inv <= sr_.INV_MEAN_CAP, (case, b, inv)
            ref[b], sens[b] = got[:6], np.abs(t32 - t64)
            print(f"{case}[{b}] L={L}: " + " ".join(f"{k} {v:.6g}" for k, v in zip(sr_.TERMS, ref[b])) +
                  f"; f32 vs f64 (relative) {np.max(sens[b] / np.abs(t64)):.2e}, smallest value {floor:.2e}, mean(1/M) {inv:.0f}")
        out.update({f"{case}_est": est, f"{case}_clean": clean, f"{case}_lengths": np.asarray(lengths, np.int32),
                    f"{case}_ref_f32": ref, f"{case}_f32_vs_f64": sens})
        if case == "edge":
            out["edge_batch"] = run_class(loss, est, clean)
            b32, b64 = terms_as(loss, est, clean, torch.float32)[0], terms_as(loss, est, clean, torch.float64)[0]
            assert np.array_equal(b32, out["edge_batch"][:6])
            out["edge_batch_f32_vs_f64"] = np.abs(np.append(b32, out["edge_batch"][6]) - np.append(b64, b64.sum()))
            print("edge at full width:", out["edge_batch"], "f32 vs f64", out["edge_batch_f32_vs_f64"])
    np.savez(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    main()
