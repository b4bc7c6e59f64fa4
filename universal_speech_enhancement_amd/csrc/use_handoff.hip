// The hand-off between the two stages of the pipeline (SGMSE sampler -> LSGAN refine generator) on the device: what the two-run flow
// does to a stage-1 waveform between SGMSEModule.predict_step's writer and the batch the stage-2 loader hands to the generator.
//   1. use_wav_write (use_io.cpp): PCM-16 q = clamp(nearbyint(x * 32767), -32768, 32767) in double (a NaN is written as 0); float: x
//   2. use_load_utterance:         v = q / 32768 in double; float: x widened
//   3. with normalize:             mx = max |v| by `fabs(v) > mx` (a NaN never becomes the peak), v = v / mx * 0.8 - two roundings,
//                                  a silent item gives NaN - then float32
//   4. LoadWavData.predict_batches: zero from len[b] to the end of the row
// Everything is fp64, so that a sample has the bits of the host path.  A maximum does not depend on the order it is taken in: the
// peak, and with it every output sample, is the same in every run, at every batch composition and at every stride.
//
//   peak   (nblk, B)  max |v| of one HANDOFF_SLICE-sample slice per workgroup -> 1 partial, plain store.  Slices past len[b] return at
//                     once, their partials are never read, and no sample of `in` past len[b] is: after stage 1 the padding holds
//                     whatever the iSTFT left there.
//   scale  (nblk, B)  every workgroup re-reduces the ceil(len[b] / HANDOFF_SLICE) partials of its row, transforms its slice and zeroes
//                     its part of the padding; slice 0 stores the peak.  A workgroup reads and writes its own slice only, so out == in
//                     is allowed.
// use_wav_handoff_files (data.channels=all): the rows are the channels of files, and the second run's loader gives a file ONE gain.  The
// peak kernel is the same; the scale kernel re-reduces the partials of all rows of its file, and the file's first row stores the peak.
// No atomics and nothing to zero-initialise: a captured graph replays as it is.  Rows start wherever b * stride puts them (odd
// strides), so a slice is a scalar head up to the next 16-byte boundary, float4 loads, and a scalar tail.
#include <cstdarg>
#include <cstdio>
#include <vector>

#include "../../include/use_hip.h"
#include "use_kernels.h"

int use_set_error(int code, const char* msg);   // use_engine.cpp

namespace use {

namespace {

constexpr int HANDOFF_SLICE = 16384;                          // samples per workgroup: 16 float4 per thread; ten minutes at 24 kHz are 879 slices

// step 1 and the decode of step 2
template <int SUBTYPE>
__device__ __forceinline__ double handoff_decode(float x) {
    if (SUBTYPE == USE_WAV_PCM16) {
        double q = rint((double)x * 32767.0);                // round to nearest even, as nearbyint in the default rounding mode
        if (!(q == q)) q = 0.0;
        q = q > 32767.0 ? 32767.0 : q < -32768.0 ? -32768.0 : q;
        return (double)(int)q / 32768.0;                     // the stored integer: a -0.0 of the rounding reads back as +0.0
    }
    return (double)x;
}

// a slice of n samples at p: scalar [0, head), float4 j < nvec at head + 4 j, scalar [tail, n)
struct Span { int head, nvec, tail; };
__device__ __forceinline__ Span span_of(const float* p, int n) {
    Span s;
    s.head = min(n, (int)((4 - (((uintptr_t)p >> 2) & 3)) & 3));
    s.nvec = (n - s.head) >> 2;
    s.tail = s.head + 4 * s.nvec;
    return s;
}

// maximum of 256 non-negative doubles (never NaN); every thread gets the result
__device__ __forceinline__ double block_max(double v, double* sh) {
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_down(v, off, 64);
        v = o > v ? o : v;
    }
    __syncthreads();                                          // sh may still be read from a previous call
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double m = sh[0];
    for (int w = 1; w < 4; ++w) m = sh[w] > m ? sh[w] : m;
    return m;
}

template <int SUBTYPE>
__global__ __launch_bounds__(256) void handoff_peak_kernel(const float* in, const int* __restrict__ lens, double* __restrict__ part,
                                                           int64_t stride, int nblk) {
    __shared__ double sh[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t L = lens[b], lo = (int64_t)blockIdx.x * HANDOFF_SLICE;
    if (lo >= L) return;                                      // a slice of padding: its partial is never read
    const int n = (int)min((int64_t)HANDOFF_SLICE, L - lo);
    const float* p = in + (int64_t)b * stride + lo;
    const Span sp = span_of(p, n);
    double mx = 0.0;
    auto take = [&](float x) { const double a = fabs(handoff_decode<SUBTYPE>(x)); mx = a > mx ? a : mx; };
    if (tid < sp.head) take(p[tid]);
    for (int j = tid; j < sp.nvec; j += 256) {
        const float4 x = *reinterpret_cast<const float4*>(p + sp.head + 4 * j);
        take(x.x); take(x.y); take(x.z); take(x.w);
    }
    if (sp.tail + tid < n) take(p[sp.tail + tid]);
    mx = block_max(mx, sh);
    if (tid == 0) part[(size_t)b * nblk + blockIdx.x] = mx;
}

// FILES (use_wav_handoff_files): row b belongs to a file of file_rows[b].y rows that starts at row file_rows[b].x and is file number
// file_rows[b].z; the rows of a file have one length, the peak is taken over the partials of all of them and stored once per file
template <int SUBTYPE, int NORM, int FILES = 0>
__global__ __launch_bounds__(256) void handoff_scale_kernel(const float* in, float* out, const int* __restrict__ lens,
                                                            const double* __restrict__ part, double* __restrict__ peak, int64_t stride,
                                                            int nblk, const int3* __restrict__ file_rows = nullptr) {
    __shared__ double sh[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t L = lens[b], lo = (int64_t)blockIdx.x * HANDOFF_SLICE;
    const int w = (int)min((int64_t)HANDOFF_SLICE, stride - lo);                   // this slice of the row ...
    const int n = (int)max((int64_t)0, min((int64_t)w, L - lo));                   // ... and its valid samples
    const float* p = in + (int64_t)b * stride + lo;
    float* o = out + (int64_t)b * stride + lo;
    double mx = 0.0;
    if ((NORM && n > 0) || blockIdx.x == 0) {
        const int np = (int)((L + HANDOFF_SLICE - 1) / HANDOFF_SLICE);
        if (FILES) {
            const int3 fr = file_rows[b];
            for (int c = 0; c < fr.y; ++c) {
                const double* q = part + (size_t)(fr.x + c) * nblk;
                for (int j = tid; j < np; j += 256) mx = q[j] > mx ? q[j] : mx;
            }
            mx = block_max(mx, sh);
            if (blockIdx.x == 0 && tid == 0 && b == fr.x) peak[fr.z] = mx;
        } else {
            const double* q = part + (size_t)b * nblk;
            for (int j = tid; j < np; j += 256) mx = q[j] > mx ? q[j] : mx;
            mx = block_max(mx, sh);
            if (blockIdx.x == 0 && tid == 0) peak[b] = mx;
        }
    }
    auto conv = [&](float x) -> float {
        double v = handoff_decode<SUBTYPE>(x);
        if (NORM) v = __dmul_rn(__ddiv_rn(v, mx), 0.8);       // v / mx * 0.8: two roundings; mx = 0 gives NaN, as the loader does
        return (float)v;
    };
    if (n > 0) {
        const Span sp = span_of(p, n);
        const bool vec_store = ((uintptr_t)(o + sp.head) & 15) == 0;               // out is aligned as in is (always when out == in)
        if (tid < sp.head) o[tid] = conv(p[tid]);
        for (int j = tid; j < sp.nvec; j += 256) {
            const int i = sp.head + 4 * j;
            const float4 x = *reinterpret_cast<const float4*>(p + i);
            const float4 y = make_float4(conv(x.x), conv(x.y), conv(x.z), conv(x.w));
            if (vec_store) *reinterpret_cast<float4*>(o + i) = y;
            else { o[i] = y.x; o[i + 1] = y.y; o[i + 2] = y.z; o[i + 3] = y.w; }
        }
        if (sp.tail + tid < n) o[sp.tail + tid] = conv(p[sp.tail + tid]);
    }
    if (n < w) {                                              // the loader's zero padding
        float* z = o + n;
        const Span sp = span_of(z, w - n);
        if (tid < sp.head) z[tid] = 0.f;
        for (int j = tid; j < sp.nvec; j += 256) *reinterpret_cast<float4*>(z + sp.head + 4 * j) = make_float4(0.f, 0.f, 0.f, 0.f);
        if (sp.tail + tid < w - n) z[sp.tail + tid] = 0.f;
    }
}

int failf(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    return use_set_error(code, buf);
}

// byte offset of the partials behind the int lens[B], and the slices per row
struct HandoffWork { size_t part, bytes; int64_t nblk; };
HandoffWork handoff_layout(int B, int64_t stride) {
    HandoffWork w;
    w.nblk = (stride + HANDOFF_SLICE - 1) / HANDOFF_SLICE;
    w.part = ((size_t)B * sizeof(int) + 7) & ~(size_t)7;
    w.bytes = w.part + (size_t)B * (size_t)w.nblk * sizeof(double);
    return w;
}
bool handoff_shape_ok(int B, int64_t stride) {                // gridDim = (nblk, B)
    return B >= 1 && B <= 65535 && stride >= 1 && (stride + HANDOFF_SLICE - 1) / HANDOFF_SLICE <= 0x7fffffff;
}
// use_wav_handoff_files: behind lens[B] lie (first row, rows, file) of every row, then the partials
constexpr int HANDOFF_MAX_CHANNELS = 64;
HandoffWork handoff_files_layout(int B, int64_t stride) {
    HandoffWork w = handoff_layout(B, stride);
    w.part = ((size_t)B * 4 * sizeof(int) + 7) & ~(size_t)7;
    w.bytes = w.part + (size_t)B * (size_t)w.nblk * sizeof(double);
    return w;
}

}  // namespace

}  // namespace use

using namespace use;

size_t use_wav_handoff_workspace(int B, int64_t stride) {
    if (!handoff_shape_ok(B, stride)) return 0;
    return handoff_layout(B, stride).bytes;
}

int use_wav_handoff(const float* in, float* out, int64_t stride, const int* len_host, int B, int subtype, int normalize, void* work,
                    size_t work_bytes, double* peak_dev, use_stream_t s) {
    if (B < 1 || B > 65535) return failf(USE_E_INVALID, "use_wav_handoff: B=%d must lie in 1 ... 65535", B);
    if (!handoff_shape_ok(B, stride)) return failf(USE_E_INVALID, "use_wav_handoff: stride=%lld must be positive (and below 2^45)", (long long)stride);
    if (!in) return failf(USE_E_INVALID, "use_wav_handoff: in is null");
    if (!out) return failf(USE_E_INVALID, "use_wav_handoff: out is null");
    if (!len_host) return failf(USE_E_INVALID, "use_wav_handoff: len_host is null");
    if (!work) return failf(USE_E_INVALID, "use_wav_handoff: work is null");
    if (!peak_dev) return failf(USE_E_INVALID, "use_wav_handoff: peak_dev is null");
    if (subtype != USE_WAV_PCM16 && subtype != USE_WAV_FLOAT32)
        return failf(USE_E_INVALID, "use_wav_handoff: subtype=%d is neither USE_WAV_PCM16 nor USE_WAV_FLOAT32", subtype);
    for (int b = 0; b < B; ++b)
        if (len_host[b] < 1 || len_host[b] > stride)
            return failf(USE_E_INVALID, "use_wav_handoff: len[%d]=%d must lie in 1 ... stride = %lld", b, len_host[b], (long long)stride);
    const HandoffWork w = handoff_layout(B, stride);
    if (work_bytes < w.bytes)
        return failf(USE_E_INVALID, "use_wav_handoff: work_bytes=%zu is smaller than use_wav_handoff_workspace(%d, %lld) = %zu", work_bytes, B,
                     (long long)stride, w.bytes);
    if ((uintptr_t)work & 7) return failf(USE_E_INVALID, "use_wav_handoff: work must be 8-byte aligned");
    if (((uintptr_t)in | (uintptr_t)out) & 3) return failf(USE_E_INVALID, "use_wav_handoff: in and out must be 4-byte aligned");

    hipStream_t st = (hipStream_t)s;
    int* lens = static_cast<int*>(work);
    double* part = reinterpret_cast<double*>(static_cast<char*>(work) + w.part);
    launch_item_lengths(lens, len_host, B, st);               // as use_metrics: kernel arguments, no copy, no synchronisation
    const int nblk = (int)w.nblk;
    const dim3 grid(nblk, B), block(256);
    if (subtype == USE_WAV_PCM16) {
        hipLaunchKernelGGL(handoff_peak_kernel<USE_WAV_PCM16>, grid, block, 0, st, in, lens, part, stride, nblk);
        if (normalize) hipLaunchKernelGGL((handoff_scale_kernel<USE_WAV_PCM16, 1>), grid, block, 0, st, in, out, lens, part, peak_dev, stride, nblk);
        else hipLaunchKernelGGL((handoff_scale_kernel<USE_WAV_PCM16, 0>), grid, block, 0, st, in, out, lens, part, peak_dev, stride, nblk);
    } else {
        hipLaunchKernelGGL(handoff_peak_kernel<USE_WAV_FLOAT32>, grid, block, 0, st, in, lens, part, stride, nblk);
        if (normalize) hipLaunchKernelGGL((handoff_scale_kernel<USE_WAV_FLOAT32, 1>), grid, block, 0, st, in, out, lens, part, peak_dev, stride, nblk);
        else hipLaunchKernelGGL((handoff_scale_kernel<USE_WAV_FLOAT32, 0>), grid, block, 0, st, in, out, lens, part, peak_dev, stride, nblk);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(USE_E_HIP, "use_wav_handoff: launch failed: %s", hipGetErrorString(e));
    return USE_OK;
}

size_t use_wav_handoff_files_workspace(int rows, int64_t stride) {
    if (!handoff_shape_ok(rows, stride)) return 0;
    return handoff_files_layout(rows, stride).bytes;
}

int use_wav_handoff_files(const float* in, float* out, int64_t stride, const int* len_host, const int* ch_host, int F, int subtype,
                          int normalize, void* work, size_t work_bytes, double* peak_dev, use_stream_t s) {
    if (F < 1 || F > 65535) return failf(USE_E_INVALID, "use_wav_handoff_files: F=%d must lie in 1 ... 65535", F);
    if (stride < 1 || (stride + HANDOFF_SLICE - 1) / HANDOFF_SLICE > 0x7fffffff)
        return failf(USE_E_INVALID, "use_wav_handoff_files: stride=%lld must be positive (and below 2^45)", (long long)stride);
    if (!in) return failf(USE_E_INVALID, "use_wav_handoff_files: in is null");
    if (!out) return failf(USE_E_INVALID, "use_wav_handoff_files: out is null");
    if (!len_host) return failf(USE_E_INVALID, "use_wav_handoff_files: len_host is null");
    if (!ch_host) return failf(USE_E_INVALID, "use_wav_handoff_files: ch_host is null");
    if (!work) return failf(USE_E_INVALID, "use_wav_handoff_files: work is null");
    if (!peak_dev) return failf(USE_E_INVALID, "use_wav_handoff_files: peak_dev is null");
    if (subtype != USE_WAV_PCM16 && subtype != USE_WAV_FLOAT32)
        return failf(USE_E_INVALID, "use_wav_handoff_files: subtype=%d is neither USE_WAV_PCM16 nor USE_WAV_FLOAT32", subtype);
    int64_t rows = 0;
    for (int f = 0; f < F; ++f) {
        if (len_host[f] < 1 || len_host[f] > stride)
            return failf(USE_E_INVALID, "use_wav_handoff_files: len[%d]=%d must lie in 1 ... stride = %lld", f, len_host[f], (long long)stride);
        if (ch_host[f] < 1 || ch_host[f] > HANDOFF_MAX_CHANNELS)
            return failf(USE_E_INVALID, "use_wav_handoff_files: ch[%d]=%d must lie in 1 ... %d", f, ch_host[f], HANDOFF_MAX_CHANNELS);
        rows += ch_host[f];
    }
    if (rows > 65535) return failf(USE_E_INVALID, "use_wav_handoff_files: the files hold %lld rows, more than 65535", (long long)rows);
    const int B = (int)rows;
    const HandoffWork w = handoff_files_layout(B, stride);
    if (work_bytes < w.bytes)
        return failf(USE_E_INVALID, "use_wav_handoff_files: work_bytes=%zu is smaller than use_wav_handoff_files_workspace(%d, %lld) = %zu",
                     work_bytes, B, (long long)stride, w.bytes);
    if ((uintptr_t)work & 7) return failf(USE_E_INVALID, "use_wav_handoff_files: work must be 8-byte aligned");
    if (((uintptr_t)in | (uintptr_t)out) & 3) return failf(USE_E_INVALID, "use_wav_handoff_files: in and out must be 4-byte aligned");
    if ((uintptr_t)peak_dev & 7) return failf(USE_E_INVALID, "use_wav_handoff_files: peak_dev must be 8-byte aligned");

    hipStream_t st = (hipStream_t)s;
    int* lens = static_cast<int*>(work);
    int* rows_dev = lens + B;
    double* part = reinterpret_cast<double*>(static_cast<char*>(work) + w.part);
    std::vector<int> host((size_t)B * 4);                     // lens[B], then (first row, rows, file) of every row
    for (int f = 0, b = 0; f < F; ++f)
        for (int c = 0, first = b; c < ch_host[f]; ++c, ++b) {
            host[(size_t)b] = len_host[f];
            host[(size_t)B + 3 * (size_t)b] = first; host[(size_t)B + 3 * (size_t)b + 1] = ch_host[f]; host[(size_t)B + 3 * (size_t)b + 2] = f;
        }
    launch_item_lengths(lens, host.data(), 4 * B, st);        // kernel arguments: no copy, no synchronisation
    const int3* fr = reinterpret_cast<const int3*>(rows_dev);
    const int nblk = (int)w.nblk;
    const dim3 grid(nblk, B), block(256);
    if (subtype == USE_WAV_PCM16) {
        hipLaunchKernelGGL(handoff_peak_kernel<USE_WAV_PCM16>, grid, block, 0, st, in, lens, part, stride, nblk);
        if (normalize) hipLaunchKernelGGL((handoff_scale_kernel<USE_WAV_PCM16, 1, 1>), grid, block, 0, st, in, out, lens, part, peak_dev, stride, nblk, fr);
        else hipLaunchKernelGGL((handoff_scale_kernel<USE_WAV_PCM16, 0, 1>), grid, block, 0, st, in, out, lens, part, peak_dev, stride, nblk, fr);
    } else {
        hipLaunchKernelGGL(handoff_peak_kernel<USE_WAV_FLOAT32>, grid, block, 0, st, in, lens, part, stride, nblk);
        if (normalize) hipLaunchKernelGGL((handoff_scale_kernel<USE_WAV_FLOAT32, 1, 1>), grid, block, 0, st, in, out, lens, part, peak_dev, stride, nblk, fr);
        else hipLaunchKernelGGL((handoff_scale_kernel<USE_WAV_FLOAT32, 0, 1>), grid, block, 0, st, in, out, lens, part, peak_dev, stride, nblk, fr);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(USE_E_HIP, "use_wav_handoff_files: launch failed: %s", hipGetErrorString(e));
    return USE_OK;
}
