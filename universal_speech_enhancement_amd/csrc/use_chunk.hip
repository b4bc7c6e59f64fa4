// Chunked sampling of long recordings (no reference counterpart): the frame axis of a spectrogram [B][1][F][T'] is cut into n
// overlapping windows of C frames, hop = C - overlap apart, which run through the sampler as a batch of B * n items; the enhanced
// windows are cross-faded back into one spectrogram.
//   split: chunks[b * n + k][f][c] = Y[b][f][k * hop + c], zero where k * hop + c >= T'
//   merge: X[b][f][t] = a_j cur[j] + (1 - a_j) prev[j + hop] for k >= 1 and j < overlap (a_j = (j + 1) / (overlap + 1)), else cur[j];
//          k = min(t / hop, n - 1), j = t - k * hop, cur / prev = chunk k / k - 1 of item b.  overlap <= C / 2: at most two sources.
// Both are row copies with frames innermost: one wave moves 64 (or 2 x 64) consecutive complex64 values of one row, and every
// output element is written by exactly one thread (no atomics: the merge is deterministic).  A chunk starts at k * hop frames, so
// 16-byte accesses (V = 2) are taken only when hop is even - then T', C, overlap, every chunk start and every cross-fade boundary
// are even as well - and the buffers are 16-byte aligned; otherwise the kernels stay on 8-byte accesses (V = 1).
#include "use_kernels.h"

#include <algorithm>

namespace use {

namespace {
template <int V> struct chunk_vec;
template <> struct chunk_vec<1> { using type = float2; };
template <> struct chunk_vec<2> { using type = float4; };

__device__ __forceinline__ float2 xfade(float2 cur, float2 prev, int j, int overlap) {
    const float a = (float)(j + 1) / (float)(overlap + 1), b = 1.f - a;
    return make_float2(fmaf(a, cur.x, b * prev.x), fmaf(a, cur.y, b * prev.y));
}
__device__ __forceinline__ float2 xfade_v(float2 cur, float2 prev, int j, int overlap) { return xfade(cur, prev, j, overlap); }
__device__ __forceinline__ float4 xfade_v(float4 cur, float4 prev, int j, int overlap) {
    const float2 lo = xfade(make_float2(cur.x, cur.y), make_float2(prev.x, prev.y), j, overlap);
    const float2 hi = xfade(make_float2(cur.z, cur.w), make_float2(prev.z, prev.w), j + 1, overlap);
    return make_float4(lo.x, lo.y, hi.x, hi.y);
}

// rows = B * n * F chunk rows of C frames; thread (x, y) of a 64 x 4 block: V frames of one row
template <int V>
__global__ __launch_bounds__(256) void chunk_split_kernel(const float2* __restrict__ Y, float2* __restrict__ chunks, int rows, int F,
                                                          int n, int Tp, int C, int hop) {
    using vec = typename chunk_vec<V>::type;
    const int c = (blockIdx.x * 64 + threadIdx.x) * V;
    if (c >= C) return;
    for (int r = blockIdx.y * 4 + threadIdx.y; r < rows; r += gridDim.y * 4) {
        const int f = r % F, bk = r / F, k = bk % n, b = bk / n;
        const int t = k * hop + c;                           // V = 2: t and T' are even, so t < T' covers t + 1
        vec v{};
        if (t < Tp) v = *reinterpret_cast<const vec*>(Y + ((long)b * F + f) * Tp + t);
        *reinterpret_cast<vec*>(chunks + (long)r * C + c) = v;
    }
}

// rows = B * F output rows of T' frames
template <int V>
__global__ __launch_bounds__(256) void chunk_merge_kernel(const float2* __restrict__ chunks, float2* __restrict__ X, int rows, int F,
                                                          int n, int Tp, int C, int hop, int overlap) {
    using vec = typename chunk_vec<V>::type;
    const int t = (blockIdx.x * 64 + threadIdx.x) * V;
    if (t >= Tp) return;
    const int k = min(t / hop, n - 1), j = t - k * hop;       // j < C: (n - 1) * hop + C >= T'
    const bool fade = k >= 1 && j < overlap;                  // V = 2: j and overlap are even, so j + 1 is on the same side
    for (int r = blockIdx.y * 4 + threadIdx.y; r < rows; r += gridDim.y * 4) {
        const int f = r % F, b = r / F;
        const float2* cur = chunks + (((long)b * n + k) * F + f) * C + j;
        vec v = *reinterpret_cast<const vec*>(cur);
        if (fade) v = xfade_v(v, *reinterpret_cast<const vec*>(cur - (long)F * C + hop), j, overlap);   // chunk k - 1, frame j + hop < C
        *reinterpret_cast<vec*>(X + (long)r * Tp + t) = v;
    }
}

bool chunk_wide(const void* a, const void* b, int hop) { return hop % 2 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }
dim3 chunk_grid(int cols, int rows) { return dim3((unsigned)((cols + 63) / 64), (unsigned)std::min((rows + 3) / 4, 65535)); }
}  // namespace

void launch_chunk_split(const float2* Y, float2* chunks, int B, int F, int n, int Tp, int C, int overlap, hipStream_t s) {
    const int hop = C - overlap, rows = B * n * F;
    if (chunk_wide(Y, chunks, hop))
        hipLaunchKernelGGL(chunk_split_kernel<2>, chunk_grid(C / 2, rows), dim3(64, 4), 0, s, Y, chunks, rows, F, n, Tp, C, hop);
    else
        hipLaunchKernelGGL(chunk_split_kernel<1>, chunk_grid(C, rows), dim3(64, 4), 0, s, Y, chunks, rows, F, n, Tp, C, hop);
}

void launch_chunk_merge(const float2* chunks, float2* X, int B, int F, int n, int Tp, int C, int overlap, hipStream_t s) {
    const int hop = C - overlap, rows = B * F;
    if (chunk_wide(chunks, X, hop))
        hipLaunchKernelGGL(chunk_merge_kernel<2>, chunk_grid(Tp / 2, rows), dim3(64, 4), 0, s, chunks, X, rows, F, n, Tp, C, hop, overlap);
    else
        hipLaunchKernelGGL(chunk_merge_kernel<1>, chunk_grid(Tp, rows), dim3(64, 4), 0, s, chunks, X, rows, F, n, Tp, C, hop, overlap);
}

}  // namespace use
