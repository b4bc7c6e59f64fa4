"""numpy references of chunked sampling for test_chunk_host.py and test_hip_chunking.py: the split by slicing, the cross-fade merge in
float64 with the per-component error bound of a float32 implementation, and the comparison that leaves no element out.

The weights are written from the definition, window by window (the device kernel goes output frame by output frame): for the first
`overlap` frames of window k >= 1, j = 0 .. overlap - 1, window k weighs a_j = (j + 1) / (overlap + 1) and window k - 1 weighs 1 - a_j;
every other frame is a copy from the one window that owns it.
"""
import numpy as np

# the geometry cases of the issue: (Tp, C, overlap)
CASES = [(64, 64, 16),        # Tp = C: no chunking
         (128, 64, 16),       # Tp = C + 64
         (192, 64, 16),       # starts 0, 48, 96, 144; the last window runs 16 frames past Tp
         (192, 64, 0),        # overlap = 0
         (192, 64, 32),       # overlap = C / 2
         (384, 128, 64)]      # overlap = C / 2 at another window length
ODD_HOP = (192, 64, 15)       # hop = 49: window starts at odd frames, no 16-byte alignment


def ref_plan(Tp, C, overlap):
    """(n, starts) from the issue's formula, independent of chunking.chunk_plan."""
    hop = C - overlap
    if Tp <= C:
        return 1, [0]
    n = int(np.ceil((Tp - overlap) / hop))
    return n, [k * hop for k in range(n)]


def ref_split(Y, C, overlap):
    """[B,1,F,Tp] -> [B*n,1,F,C] by slicing, zero tail; dtype kept."""
    B, _, F, Tp = Y.shape
    n, starts = ref_plan(Tp, C, overlap)
    out = np.zeros((B * n, 1, F, C), Y.dtype)
    for b in range(B):
        for k, s in enumerate(starts):
            w = min(C, Tp - s)
            out[b * n + k, 0, :, :w] = Y[b, 0, :, s:s + w]
    return out


def ref_merge(chunks, B, Tp, C, overlap):
    """[B*n,1,F,C] -> (X complex128 [B,1,F,Tp], bound float64 [B,1,F,Tp,2]).  bound is the most a float32 implementation may differ per
    real component: 0 where a frame has one source (a copy), 4 * 2^-24 * (|A| + |B|) in a cross-fade of the values A and B (two
    rounded weights' products and one rounded sum, or one product and an fma, each 2^-24 relative; the weights themselves carry one
    rounding each)."""
    n, starts = ref_plan(Tp, C, overlap)
    hop = C - overlap
    F = chunks.shape[2]
    ch = chunks.astype(np.complex128).reshape(B, n, F, C)
    X = np.full((B, 1, F, Tp), np.nan + 0j, np.complex128)
    bound = np.zeros((B, 1, F, Tp, 2))
    for k, s in enumerate(starts):
        end = starts[k + 1] if k + 1 < n else Tp
        first = s + (overlap if k >= 1 else 0)
        X[:, 0, :, first:end] = ch[:, k, :, first - s:end - s]
        if k >= 1:
            for j in range(overlap):
                a = (j + 1) / (overlap + 1)
                A, Bv = ch[:, k, :, j], ch[:, k - 1, :, j + hop]
                X[:, 0, :, s + j] = a * A + (1 - a) * Bv
                bound[:, 0, :, s + j, 0] = 4 * 2.0 ** -24 * (np.abs(A.real) + np.abs(Bv.real))
                bound[:, 0, :, s + j, 1] = 4 * 2.0 ** -24 * (np.abs(A.imag) + np.abs(Bv.imag))
    assert not np.isnan(X.real).any(), "the reference left a frame without a source"
    return X, bound


def overlap_mask(Tp, C, overlap):
    """bool [Tp]: frames that are cross-fades of two windows."""
    n, starts = ref_plan(Tp, C, overlap)
    m = np.zeros(Tp, bool)
    for s in starts[1:]:
        m[s:s + overlap] = True
    return m


def check_merged(out, ref, bound, what=""):
    """Every real component of `out` (complex64 [B,1,F,Tp]) within `bound` of `ref`; bit-equal where the bound is 0.  Prints the worst
    excess before asserting."""
    out = np.asarray(out)
    assert out.shape == ref.shape and out.dtype == np.complex64, (out.shape, out.dtype)
    err = np.stack([np.abs(out.real.astype(np.float64) - ref.real), np.abs(out.imag.astype(np.float64) - ref.imag)], axis=-1)
    single = bound == 0
    n_single_off = int((err[single] != 0).sum())
    faded = ~single
    ratio = float((err[faded] / np.maximum(bound[faded], 1e-300)).max()) if faded.any() else 0.0
    print(f"{what}: {int(single.sum())} copied components, {n_single_off} differ; {int(faded.sum())} cross-faded components, "
          f"worst error / bound = {ratio:.3f}")
    assert np.isfinite(err).all(), f"{what}: non-finite output"
    assert n_single_off == 0, f"{what}: {n_single_off} single-source components are not bit-equal"
    assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} cross-faded components exceed the bound (worst ratio {ratio:.3f})"
