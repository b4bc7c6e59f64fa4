"""The part of the reference's ``sgmse/util/other.py`` this package has: ``pad_spec`` (``:128-135``) and the evaluation metrics
``lsd``, ``si_sdr_components`` and ``energy_ratios`` (``:15-62``), names and argument order as there; and ``stoi`` with the signature of
``pystoi.stoi``, which the reference's validation loop imports (``sgmse/util/inference.py``).

``pad_spec`` zero-pads the frame axis on the right to the next multiple of 64 so the 6 FIR down/up-samplings of NCSN++ round-trip.
The two reductions run on the device (``universal_speech_enhancement_amd.metrics``, kernel file csrc/use_metrics.hip): they take
float32 CUDA tensors, 1-D or a batch ``[B, L]`` (``lengths``: valid samples per item), and return float64 CUDA tensors; numpy
arrays - what the reference takes - are uploaded as float32 and come back as Python floats.  ``eps`` is the reference's 1e-10, a
constant of the kernels."""
import numpy as np
import torch

EPS = 1e-10


def pad_spec(Y: torch.Tensor) -> torch.Tensor:
    T = Y.size(3)
    num_pad = (64 - T % 64) % 64
    return torch.nn.functional.pad(Y, (0, num_pad, 0, 0))


def _to_device(*xs):
    """-> (float32 CUDA tensors, was_numpy, was_1d)"""
    was_numpy = all(isinstance(x, np.ndarray) for x in xs)
    if was_numpy:
        xs = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda() for x in xs]
    return list(xs), was_numpy, xs[0].dim() == 1


def _check_eps(eps):
    if eps != EPS:
        raise ValueError(f"eps={eps!r}: the device metrics are built for the reference's eps = {EPS}")


def _like_reference(t: torch.Tensor, was_numpy: bool, was_1d: bool):
    if was_numpy and was_1d:
        return float(t[0])
    return t[0] if was_1d else t


def lsd(s_hat, s, eps=EPS, lengths=None):
    """``sqrt(mean |2 log(eps + |S_hat|) - 2 log(eps + |S|)|)`` over the STFT with n_fft 510, hop 128 (reference ``:23-30``)."""
    from ... import metrics
    _check_eps(eps)
    (s_hat, s), was_numpy, was_1d = _to_device(s_hat, s)
    return _like_reference(metrics.lsd(s_hat, s, lengths), was_numpy, was_1d)


def si_sdr_components(s_hat, s, n, eps=EPS):
    """``(s_target, e_noise, e_art)`` (reference ``:33-45``) along the last axis, in float64 torch: no reduction to one number, so no
    kernel of its own."""
    s_hat, s, n = (torch.as_tensor(x).to(torch.float64) for x in (s_hat, s, n))
    alpha_s = (s_hat * s).sum(-1, keepdim=True) / (eps + torch.linalg.vector_norm(s, dim=-1, keepdim=True) ** 2)
    s_target = alpha_s * s
    alpha_n = (s_hat * n).sum(-1, keepdim=True) / (eps + torch.linalg.vector_norm(n, dim=-1, keepdim=True) ** 2)
    e_noise = alpha_n * n
    e_art = s_hat - s_target - e_noise
    return s_target, e_noise, e_art


def energy_ratios(s_hat, s, n, eps=EPS, lengths=None):
    """``(si_sdr, si_sir, si_sar)`` in dB (reference ``:48-62``)."""
    from ... import metrics
    _check_eps(eps)
    (s_hat, s, n), was_numpy, was_1d = _to_device(s_hat, s, n)
    return tuple(_like_reference(v, was_numpy, was_1d) for v in metrics.energy_ratios(s_hat, s, n, lengths))


def stoi(x, y, fs_sig, extended=False, lengths=None):
    """``pystoi.stoi(x, y, fs_sig, extended)``: the clean signal FIRST, then the processed one; STOI, or ESTOI with ``extended``
    (``use_stoi``, csrc/use_stoi.hip: without pystoi's dither, so the same inputs give the same bits)."""
    from ... import metrics
    (x, y), was_numpy, was_1d = _to_device(x, y)
    return _like_reference(metrics.stoi(y, x, lengths, int(fs_sig), extended), was_numpy, was_1d)
