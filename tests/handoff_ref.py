"""numpy float64 restatement of what lies between the two stages of the two-run flow (``use_wav_handoff``): the writer of
``SGMSEModule.predict_step`` (``use_wav_write``), the inference loader (``use_load_utterance``) and the loader's collation
(``LoadWavData.predict_batches``).  tests/test_handoff_host.py pins it to that I/O path, file by file, bit for bit."""
import numpy as np


def handoff_row(x, subtype="PCM_16", normalize=True):
    """One item over its valid samples (float32 [L]) -> (float32 [L], the peak as a float64)."""
    x = np.asarray(x, dtype=np.float32)
    if subtype == "PCM_16":
        # 1. the file: nearbyint(x * 32767) in double (np.rint: round half to even, as nearbyint in the default rounding mode), clamped
        # (a NaN is written as 0)
        q = np.clip(np.rint(np.nan_to_num(x.astype(np.float64), nan=0.0, posinf=np.inf, neginf=-np.inf) * 32767.0), -32768.0, 32767.0)
        v = q.astype(np.int16).astype(np.float64) / 32768.0  # 2. the decode of the stored integer (a -0.0 of the rounding is the integer 0)
    elif subtype == "FLOAT":
        v = x.astype(np.float64)
    else:
        raise ValueError(subtype)
    a = np.abs(v)
    a = a[~np.isnan(a)]                                      # `fabs(v) > mx` is false for a NaN: it never becomes the peak
    mx = np.float64(a.max()) if a.size else np.float64(0.0)
    if normalize:                                            # 3. v / mx * 0.8, in this order: two roundings; a silent item gives NaN
        with np.errstate(invalid="ignore", divide="ignore"):
            v = v / mx * 0.8
    return v.astype(np.float32), mx


def handoff_rows(wav, lengths, subtype="PCM_16", normalize=True):
    """wav [B, stride] (any array that can be sliced: only wav[b, :lengths[b]] is touched, so a stride of 2^30 costs nothing) ->
    [(float32 [lengths[b]], peak)] per item."""
    return [handoff_row(wav[b, :L], subtype, normalize) for b, L in enumerate(lengths)]


def handoff_batch(wav, lengths, subtype="PCM_16", normalize=True):
    """wav float32 [B, stride], item b valid for lengths[b] samples (the rest is not looked at) -> (float32 [B, stride], zero past each
    item's length as the loader pads; float64 [B] peaks)."""
    out = np.zeros(wav.shape, np.float32)                    # 4. the loader's zero padding
    peaks = np.zeros(wav.shape[0], np.float64)
    for b, (row, mx) in enumerate(handoff_rows(wav, lengths, subtype, normalize)):
        out[b, :len(row)], peaks[b] = row, mx
    return out, peaks
