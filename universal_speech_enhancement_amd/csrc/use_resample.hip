// The front of the inference loader on the device: what use_load_utterance (use_io.cpp) does to the decoded first channel of a file -
// FFT resampling (scipy.signal.resample's rule), peak normalisation to 0.8, the cast to float32 - and the zero-padded collation of
// LoadWavData.predict_batches, in fp64 throughout.  The host still opens and decodes the file (use_wav_read).
//
//   resampling   rfft of length n -> bins 0 ... min(n, num) / 2, the shared Nyquist bin of an even shorter grid times 2 (shortening) or
//                0.5 (lengthening) -> Hermitian extension to length num (the imaginary parts of DC and of an even grid's Nyquist bin are
//                dropped) -> inverse transform of length num -> times (1 / num) * (num / n).  num == n is a copy.
//   a transform  of a power-of-two length is the FFT below; of any other length N it is Bluestein's chirp-z form over FFTs of
//                M = pow2 >= 2 N - 1: a = x * chirp zero-padded, b = conj(chirp) wrapped, ifft(fft(a) * fft(b)) * chirp / M, with
//                chirp[k] = exp(sign * i * pi * (k^2 mod 2N) / N), the square reduced in 64-bit integers as the host does.
//   the FFT      Stockham autosort passes of radix R = 2^r <= 512, out of place between two buffers, so that no bit-reversal pass exists.
//                A workgroup owns C = 2048 / R neighbouring columns j: it reads the R x C tile x[j + r * M / R] (runs of C contiguous
//                points), applies the pass twiddle W_{Ns R}^{r (j mod Ns)} (Ns = the product of the radices before), transforms the C
//                columns in LDS by radix-2 stages over a table of W_R^t (2048 points = 32 KiB, the table at most 16 KiB), and writes
//                y[(j / Ns) Ns R + (j mod Ns) + r Ns] (runs of C, or the whole contiguous tile in the first pass).
//                M <= 2^11: one pass, one workgroup.  M <= 2^18: two passes.  M <= 2^27: three (fft_plan: the radices as equal as possible).
//   twiddles     every twiddle and chirp is sincospi of an exactly reduced argument (an integer times a power of two, or an integer
//                below 2N over N); none comes from a recurrence.
//   peak, scale  the hand-off's pattern (use_handoff.hip): one partial maximum per LOAD_SLICE samples by a plain store, re-reduced by
//                every workgroup of the second kernel, which forms v / mx * 0.8 with two roundings, casts, and zeroes the padding.
// No atomics; every addition has a place fixed by (n, num) alone, so an item's output has the same bits in every run, at every row of
// every batch, with any companions: the items of a batch run one after another on the stream and share nothing but the workspace.
//
// The way out (use_store_items_dev) runs the same resampler from the model's rate back to a file's own: an item's float32 row, read up
// to its length only, is widened to fp64, resampled to the file's frame count, rounded to float32 and stored as it is or as the 16-bit
// code use_wav_write would store, with zeros up to the row's end.  At an unchanged length no transform runs and the row's bits pass.
//
// Files of several channels (use_load_files_dev / use_store_files_dev; data.channels=all): the host uploads a whole decoded file,
// interleaved [n][ch].  On the way in it is de-interleaved into ch contiguous fp64 channels, each goes through resample_launch as an
// item does, and the peak is ONE per file: the slice kernel runs over the ch * num contiguous values, one workgroup takes the maximum
// of its partials (a maximum has no order: fixed shape, no atomics), and the scale kernel writes the file's rows under that one gain.
// On the way out every row of a file takes store_launch's steps and is stored with stride ch, so that the file lies in `out` as
// [num][ch], the order of the samples in a WAV file.  A file of one channel has the bits of the per-item calls.
//
// The bodies of the kernels are __host__ __device__ functions of the thread index (one per phase between two barriers), so that a
// host program can run the same arithmetic without a device.
#include <cstdarg>
#include <cstdio>

#include "../../include/use_hip.h"
#include "use_kernels.h"
#include "use_fft.h"

int use_set_error(int code, const char* msg);   // use_engine.cpp

namespace use {

namespace {

constexpr int64_t RESAMPLE_MAX = (int64_t)1 << 24;              // max(n, num): Bluestein's M is at most 2^25
constexpr int LOAD_SLICE = 4096;                                // samples per workgroup of the peak and scale kernels
static_assert(FFT_MAX_LOG2 <= 3 * FFT_RADIX_LOG2 && 2 * RESAMPLE_MAX <= (int64_t)1 << FFT_MAX_LOG2, "fft_plan: at most three passes");

// exp(sign * i * pi * k^2 / N) with k^2 reduced mod 2N exactly (k < 2^24: the square fits 64 bits)
USE_HD double2 chirp(int64_t k, int64_t N, int sign) {
    const uint64_t k2 = ((uint64_t)k * (uint64_t)k) % (2 * (uint64_t)N);
    return expipi((double)k2 / (double)N, sign);
}

// the FFT length a transform of length N runs at: N itself when it is a power of two, else Bluestein's M = pow2 >= 2 N - 1
int64_t transform_size(int64_t N) { return (N & (N - 1)) == 0 ? N : (int64_t)1 << ceil_log2(2 * N - 1); }

// ---- the source of a transform, the chirp products, the result ----
struct Src { const double* x; const double2* X; int64_t n, num; };

template <int KIND>
USE_HD double2 src_value(const Src s, int64_t i) {
    if (KIND == 0) return make_double2(s.x[i], 0.0);             // the real signal
    // the Hermitian extension to length num of the kept bins X[0 ... min(n, num) / 2] (resample_fft, use_io.cpp)
    const int64_t nh = s.num / 2 + 1, N = s.num < s.n ? s.num : s.n, k = i < nh ? i : s.num - i;
    double2 y = make_double2(0.0, 0.0);
    if (k < N / 2 + 1) y = s.X[k];
    if (N % 2 == 0 && k == N / 2) { const double f = s.num < s.n ? 2.0 : 0.5; y.x *= f; y.y *= f; }
    if (i == 0 || 2 * i == s.num) return make_double2(y.x, 0.0);
    return i < nh ? y : make_double2(y.x, -y.y);
}

// A[i] = src[i] (* chirp[i]) for i < N, 0 up to M; B[i] = conj(chirp[d]) at i = d and i = M - d, d < N, 0 between (B == NULL: no Bluestein)
template <int KIND>
USE_HD void prep_element(int64_t i, const Src s, double2* A, double2* B, int64_t N, int64_t M, int sign) {
    double2 v = make_double2(0.0, 0.0);
    if (i < N) {
        v = src_value<KIND>(s, i);
        if (B) v = cmul(v, chirp(i, N, sign));
    }
    A[i] = v;
    if (B) {
        const int64_t d = i < N ? i : M - i < N ? M - i : -1;
        B[i] = d >= 0 ? chirp(d, N, -sign) : make_double2(0.0, 0.0);
    }
}

// OUT 0: X[k] = result (complex, the kept bins); OUT 1: y[k] = Re(result) * sc
template <int OUT>
USE_HD void post_element(int64_t k, const double2* R, int blue, int64_t N, int64_t M, int sign, double2* X, double* y, double sc) {
    double2 v = R[k];
    if (blue) {
        const double inv = 1.0 / (double)M;
        v = cmul(make_double2(v.x * inv, v.y * inv), chirp(k, N, sign));
    }
    if (OUT == 0) X[k] = v;
    else y[k] = v.x * sc;
}

template <int KIND>
__global__ __launch_bounds__(256) void prep_kernel(const Src s, double2* __restrict__ A, double2* __restrict__ B, int64_t N, int64_t M, int sign) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < M) prep_element<KIND>(i, s, A, B, N, M, sign);
}

__global__ __launch_bounds__(256) void mul_kernel(double2* __restrict__ A, const double2* __restrict__ B, int64_t M) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < M) A[i] = cmul(A[i], B[i]);
}

template <int OUT>
__global__ __launch_bounds__(256) void post_kernel(const double2* __restrict__ R, int blue, int64_t N, int64_t M, int sign, int64_t count,
                                                   double2* __restrict__ X, double* __restrict__ y, double sc) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < count) post_element<OUT>(k, R, blue, N, M, sign, X, y, sc);
}

// ---- peak normalisation, cast, collation ----
// maximum of 256 non-negative doubles (never NaN); every thread gets the result
__device__ __forceinline__ double block_max(double v, double* sh) {
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_down(v, off, 64);
        v = o > v ? o : v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double m = sh[0];
    for (int w = 1; w < 4; ++w) m = sh[w] > m ? sh[w] : m;
    return m;
}

// grid ceil(L / LOAD_SLICE): part[blockIdx.x] = max |v| of the slice, by `fabs(v) > mx` (a NaN never becomes the peak)
__global__ __launch_bounds__(256) void load_peak_kernel(const double* __restrict__ v, int64_t L, double* __restrict__ part) {
    __shared__ double sh[4];
    const int64_t lo = (int64_t)blockIdx.x * LOAD_SLICE, hi = min(L, lo + LOAD_SLICE);
    double mx = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) { const double a = fabs(v[i]); mx = a > mx ? a : mx; }
    mx = block_max(mx, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = mx;
}

// grid ceil(stride / LOAD_SLICE): row[i] = (float)(v[i] / mx * 0.8) (NORM) or (float)v[i] for i < L, 0 for L <= i < stride.
// peak (NORM, or null): the first workgroup, which always holds mx (L >= 1), stores the divisor there
template <int NORM>
__global__ __launch_bounds__(256) void load_scale_kernel(const double* __restrict__ v, int64_t L, const double* __restrict__ part, int np,
                                                         float* __restrict__ row, int64_t stride, double* __restrict__ peak) {
    __shared__ double sh[4];
    const int64_t lo = (int64_t)blockIdx.x * LOAD_SLICE, hi = min(stride, lo + LOAD_SLICE);
    double mx = 0.0;
    if (NORM && lo < L) {
        for (int j = threadIdx.x; j < np; j += 256) mx = part[j] > mx ? part[j] : mx;
        mx = block_max(mx, sh);
        if (peak && blockIdx.x == 0 && threadIdx.x == 0) peak[0] = mx;
    }
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        float o = 0.f;
        if (i < L) {
            double x = v[i];
            if (NORM) x = __dmul_rn(__ddiv_rn(x, mx), 0.8);       // v / mx * 0.8: two roundings; mx = 0 gives NaN, as the loader does
            o = (float)x;
        }
        row[i] = o;
    }
}

// ---- the way out: float32 rows -> file samples (use_store_items_dev) ----
// x[i] = (double)row[i] for i < L: the only read of a row, and none of it past the item's length
__global__ __launch_bounds__(256) void store_widen_kernel(const float* __restrict__ row, int64_t L, double* __restrict__ x) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < L) x[i] = (double)row[i];
}

// the 16-bit code use_wav_write stores for a float32 sample (use_io.cpp): the product is exact (24 + 15 bits), rint rounds to nearest even
// as the host's nearbyint does, a NaN becomes 0
__device__ __forceinline__ int16_t pcm16_code(float x32) {
    double v = rint((double)x32 * 32767.0);
    if (!(v == v)) v = 0.0;
    return (int16_t)(v > 32767.0 ? 32767.0 : v < -32768.0 ? -32768.0 : v);
}

// the float32 sample of the way out: (float)v, or with GAIN (float)(v * g), the product rounded once in fp64 and never contracted (the
// source's level, data.restore_level); without GAIN g is not read and a float's bits pass
template <typename SRC, int GAIN>
__device__ __forceinline__ float store_sample(SRC v, double g) {
    if constexpr (GAIN) return (float)__dmul_rn((double)v, g);
    else return (float)v;
}

// grid ceil(out_stride / LOAD_SLICE): row[i] = x32 = store_sample(v[i]) (DST float) or its 16-bit code (DST int16_t) for i < num, 0 for
// num <= i < out_stride.  SRC double: the resampled signal; SRC float: the item's own row (num == len), whose bits pass unchanged
template <typename SRC, typename DST, int GAIN>
__global__ __launch_bounds__(256) void store_kernel(const SRC* __restrict__ v, int64_t num, DST* __restrict__ row, int64_t out_stride, double g) {
    const int64_t lo = (int64_t)blockIdx.x * LOAD_SLICE, hi = min(out_stride, lo + LOAD_SLICE);
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        DST o = 0;
        if (i < num) {
            const float x32 = store_sample<SRC, GAIN>(v[i], g);
            if constexpr (sizeof(DST) == 2) o = pcm16_code(x32);
            else o = x32;
        }
        row[i] = o;
    }
}

// ---- files of several channels (use_load_files_dev / use_store_files_dev) ----
// interleaved frames x[t * ch + c] -> ch contiguous channels out[c * n + t]; one thread per output element (count = n * ch)
__global__ __launch_bounds__(256) void deinterleave_kernel(const double* __restrict__ x, int64_t n, int ch, int64_t count,
                                                           double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int64_t c = i / n, t = i - c * n;
    out[i] = x[t * ch + c];
}

// one workgroup: fin[0] = the maximum of the np partial maxima of load_peak_kernel, and peak[0] too where the caller asks for it
__global__ __launch_bounds__(256) void load_peak_final_kernel(const double* __restrict__ part, int np, double* __restrict__ fin,
                                                              double* __restrict__ peak) {
    __shared__ double sh[4];
    double mx = 0.0;
    for (int j = threadIdx.x; j < np; j += 256) mx = part[j] > mx ? part[j] : mx;
    mx = block_max(mx, sh);
    if (threadIdx.x == 0) {
        fin[0] = mx;
        if (peak) peak[0] = mx;
    }
}

// store_kernel's sample for one channel of an interleaved file: dst[i * ch] = x32 = store_sample(v[i]) or its 16-bit code, i < num (dst
// points at the channel's first sample)
template <typename SRC, typename DST, int GAIN>
__global__ __launch_bounds__(256) void store_interleave_kernel(const SRC* __restrict__ v, int64_t num, DST* __restrict__ dst, int ch, double g) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= num) return;
    const float x32 = store_sample<SRC, GAIN>(v[i], g);
    if constexpr (sizeof(DST) == 2) dst[i * ch] = pcm16_code(x32);
    else dst[i * ch] = x32;
}

int failf(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    return use_set_error(code, buf);
}

// a gain of the way out: finite and not negative; -> USE_OK, or USE_E_INVALID with the entry named
int gains_ok(const char* fn, const double* gain, int count) {
    for (int i = 0; gain && i < count; ++i)
        if (!(gain[i] >= 0.0) || gain[i] > 1.7976931348623157e308)
            return failf(USE_E_INVALID, "%s: gain_host[%d]=%g must be finite and not negative", fn, i, gain[i]);
    return USE_OK;
}

// ---- host: workspace layout and launches ----
// byte offsets in an item's workspace: the partial maxima, the resampled signal (use_load_items_dev), the kept bins, three FFT buffers
struct ItemWork { size_t part, y, spec, buf, bytes; int64_t M; };
size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
bool item_ok(int64_t n, int64_t num) { return n >= 1 && num >= 1 && n <= RESAMPLE_MAX && num <= RESAMPLE_MAX; }
ItemWork item_layout(int64_t n, int64_t num) {
    ItemWork w;
    // the buffers are sized for Bluestein's M whether or not a length is a power of two: the size never shrinks as n grows
    const int64_t Mn = (int64_t)1 << ceil_log2(2 * n - 1), Mnum = (int64_t)1 << ceil_log2(2 * num - 1), keep = (n < num ? n : num) / 2 + 1;
    w.M = n == num ? 0 : Mn > Mnum ? Mn : Mnum;
    w.part = 0;
    w.y = align16((size_t)((num + LOAD_SLICE - 1) / LOAD_SLICE) * sizeof(double));
    w.spec = w.y + align16((size_t)num * sizeof(double));
    w.buf = w.spec + (n == num ? 0 : align16((size_t)keep * sizeof(double2)));
    w.bytes = w.buf + 3 * (size_t)w.M * sizeof(double2);
    return w;
}

int blocks256(int64_t count) { return (int)((count + 255) / 256); }

// the DFT of length N of src (KIND) with `sign`; OUT 0: `count` bins to X, OUT 1: the N real parts times sc to y
template <int KIND, int OUT>
void dft_launch(const Src src, int64_t N, int sign, int64_t count, double2* X, double* y, double sc, double2* b0, double2* b1, double2* b2,
                hipStream_t st) {
    const int64_t M = transform_size(N);
    const int blue = M != N, m = ceil_log2(M);
    hipLaunchKernelGGL(prep_kernel<KIND>, dim3(blocks256(M)), dim3(256), 0, st, src, b0, blue ? b1 : (double2*)nullptr, N, M, sign);
    double2* R;
    if (blue) {
        double2* B = fft_launch(b1, b2, m, -1, st);
        double2* spare = B == b1 ? b2 : b1;
        double2* A = fft_launch(b0, spare, m, -1, st);
        spare = A == b0 ? spare : b0;
        hipLaunchKernelGGL(mul_kernel, dim3(blocks256(M)), dim3(256), 0, st, A, B, M);
        R = fft_launch(A, spare, m, +1, st);
    } else {
        R = fft_launch(b0, b1, m, sign, st);
    }
    hipLaunchKernelGGL(post_kernel<OUT>, dim3(blocks256(count)), dim3(256), 0, st, R, blue, N, M, sign, count, X, y, sc);
}

// scipy.signal.resample(x, num) for n != num
void resample_launch(const double* x, int64_t n, int64_t num, double* y, char* work, const ItemWork w, hipStream_t st) {
    double2* X = reinterpret_cast<double2*>(work + w.spec);
    double2* b0 = reinterpret_cast<double2*>(work + w.buf);
    double2 *b1 = b0 + w.M, *b2 = b1 + w.M;
    const int64_t keep = (n < num ? n : num) / 2 + 1;
    Src s; s.x = x; s.X = X; s.n = n; s.num = num;
    dft_launch<0, 0>(s, n, -1, keep, X, nullptr, 0.0, b0, b1, b2, st);
    const double sc = (1.0 / (double)num) * ((double)num / (double)n);
    dft_launch<1, 1>(s, num, +1, num, nullptr, y, sc, b0, b1, b2, st);
}

// an item's workspace on the way out: item_layout's, then the row widened to fp64
size_t store_bytes(int64_t len, int64_t num) { return item_layout(len, num).bytes + align16((size_t)len * sizeof(double)); }

// one item of use_store_items_dev: row[0 ... len) -> dst[0 ... out_stride); gain null: the instantiations without a gain
template <typename DST>
void store_launch(const float* row, int64_t len, int64_t num, DST* dst, int64_t out_stride, const double* gain, char* work, hipStream_t st) {
    const dim3 grid((unsigned)((out_stride + LOAD_SLICE - 1) / LOAD_SLICE)), block(256);
    if (len == num) {
        if (gain) hipLaunchKernelGGL((store_kernel<float, DST, 1>), grid, block, 0, st, row, num, dst, out_stride, *gain);
        else hipLaunchKernelGGL((store_kernel<float, DST, 0>), grid, block, 0, st, row, num, dst, out_stride, 1.0);
        return;
    }
    const ItemWork w = item_layout(len, num);
    double* x = reinterpret_cast<double*>(work + w.bytes);
    double* y = reinterpret_cast<double*>(work + w.y);
    hipLaunchKernelGGL(store_widen_kernel, dim3(blocks256(len)), block, 0, st, row, len, x);
    resample_launch(x, len, num, y, work, w, st);
    if (gain) hipLaunchKernelGGL((store_kernel<double, DST, 1>), grid, block, 0, st, (const double*)y, num, dst, out_stride, *gain);
    else hipLaunchKernelGGL((store_kernel<double, DST, 0>), grid, block, 0, st, (const double*)y, num, dst, out_stride, 1.0);
}

// a file's workspace in use_load_files_dev: item_layout's (the transforms of one channel at a time), the partial maxima of all ch * num
// values and their maximum, the ch de-interleaved channels (ch > 1), the ch resampled channels one after another (n != num)
constexpr int FILE_MAX_CHANNELS = 64;
struct FileWork { ItemWork item; size_t part, fin, chan, ys, bytes; int np; };
bool channels_ok(int ch) { return ch >= 1 && ch <= FILE_MAX_CHANNELS; }
FileWork file_layout(int64_t n, int64_t num, int ch) {
    FileWork w;
    w.item = item_layout(n, num);
    w.np = (int)(((int64_t)ch * num + LOAD_SLICE - 1) / LOAD_SLICE);       // at most 64 * 2^24 / 4096 = 2^18
    w.part = align16(w.item.bytes);
    w.fin = w.part + align16((size_t)w.np * sizeof(double));
    w.chan = w.fin + 16;
    w.ys = w.chan + (ch > 1 ? align16((size_t)ch * (size_t)n * sizeof(double)) : 0);
    w.bytes = w.ys + (n != num ? align16((size_t)ch * (size_t)num * sizeof(double)) : 0);
    return w;
}

// one file of use_load_files_dev: x (interleaved [n][ch]) -> rows wav[0 ... ch) of width stride
void load_file_launch(const double* x, int64_t n, int64_t num, int ch, int normalize, float* wav, int64_t stride, double* peak, char* work,
                      hipStream_t st) {
    const FileWork w = file_layout(n, num, ch);
    const dim3 block(256);
    const double* v = x;                                          // ch contiguous channels of num samples
    if (ch > 1) {
        double* chan = reinterpret_cast<double*>(work + w.chan);
        const int64_t count = (int64_t)ch * n;
        hipLaunchKernelGGL(deinterleave_kernel, dim3(blocks256(count)), block, 0, st, x, n, ch, count, chan);
        v = chan;
    }
    if (n != num) {
        double* ys = reinterpret_cast<double*>(work + w.ys);
        for (int c = 0; c < ch; ++c) resample_launch(v + (int64_t)c * n, n, num, ys + (int64_t)c * num, work, w.item, st);
        v = ys;
    }
    double* part = reinterpret_cast<double*>(work + w.part);
    double* fin = reinterpret_cast<double*>(work + w.fin);
    if (normalize) {                                              // one peak over the file: the channels keep their level relation
        hipLaunchKernelGGL(load_peak_kernel, dim3(w.np), block, 0, st, v, (int64_t)ch * num, part);
        hipLaunchKernelGGL(load_peak_final_kernel, dim3(1), block, 0, st, (const double*)part, w.np, fin, peak);
    }
    const dim3 grid((unsigned)((stride + LOAD_SLICE - 1) / LOAD_SLICE));
    for (int c = 0; c < ch; ++c) {
        float* row = wav + (int64_t)c * stride;
        if (normalize) hipLaunchKernelGGL(load_scale_kernel<1>, grid, block, 0, st, v + (int64_t)c * num, num, (const double*)fin, 1, row, stride, (double*)nullptr);
        else hipLaunchKernelGGL(load_scale_kernel<0>, grid, block, 0, st, v + (int64_t)c * num, num, (const double*)fin, 1, row, stride, (double*)nullptr);
    }
}

// one file of use_store_files_dev: rows wav[0 ... ch) of width stride, valid for len -> dst[num][ch]; a row goes the way of store_launch
template <typename DST>
void store_file_launch(const float* wav, int64_t stride, int64_t len, int64_t num, int ch, DST* dst, const double* gain, char* work,
                       hipStream_t st) {
    const dim3 grid(blocks256(num)), block(256);
    const ItemWork w = item_layout(len, num);
    double* x = reinterpret_cast<double*>(work + w.bytes);
    double* y = reinterpret_cast<double*>(work + w.y);
    for (int c = 0; c < ch; ++c) {
        const float* row = wav + (int64_t)c * stride;
        if (len == num) {
            if (gain) hipLaunchKernelGGL((store_interleave_kernel<float, DST, 1>), grid, block, 0, st, row, num, dst + c, ch, *gain);
            else hipLaunchKernelGGL((store_interleave_kernel<float, DST, 0>), grid, block, 0, st, row, num, dst + c, ch, 1.0);
            continue;
        }
        hipLaunchKernelGGL(store_widen_kernel, dim3(blocks256(len)), block, 0, st, row, len, x);
        resample_launch(x, len, num, y, work, w, st);
        if (gain) hipLaunchKernelGGL((store_interleave_kernel<double, DST, 1>), grid, block, 0, st, (const double*)y, num, dst + c, ch, *gain);
        else hipLaunchKernelGGL((store_interleave_kernel<double, DST, 0>), grid, block, 0, st, (const double*)y, num, dst + c, ch, 1.0);
    }
}

}  // namespace

}  // namespace use

using namespace use;

size_t use_resample_workspace(int64_t n, int64_t num) {
    if (!item_ok(n, num)) return 0;
    return item_layout(n, num).bytes;
}

int use_resample_fft_dev(const double* x_dev, int64_t n, int64_t num, double* y_dev, void* work, size_t work_bytes, use_stream_t s) {
    if (n < 1 || num < 1) return failf(USE_E_INVALID, "use_resample_fft_dev: n=%lld and num=%lld must be positive", (long long)n, (long long)num);
    if (!item_ok(n, num))
        return failf(USE_E_INVALID, "use_resample_fft_dev: max(n, num)=%lld exceeds 2^24", (long long)(n > num ? n : num));
    if (!x_dev) return failf(USE_E_INVALID, "use_resample_fft_dev: x_dev is null");
    if (!y_dev) return failf(USE_E_INVALID, "use_resample_fft_dev: y_dev is null");
    if (!work) return failf(USE_E_INVALID, "use_resample_fft_dev: work is null");
    const ItemWork w = item_layout(n, num);
    if (work_bytes < w.bytes)
        return failf(USE_E_INVALID, "use_resample_fft_dev: work_bytes=%zu is smaller than use_resample_workspace(%lld, %lld) = %zu", work_bytes,
                     (long long)n, (long long)num, w.bytes);
    if ((uintptr_t)work & 15) return failf(USE_E_INVALID, "use_resample_fft_dev: work must be 16-byte aligned");
    if (((uintptr_t)x_dev | (uintptr_t)y_dev) & 7) return failf(USE_E_INVALID, "use_resample_fft_dev: x_dev and y_dev must be 8-byte aligned");
    hipStream_t st = (hipStream_t)s;
    if (n == num) {
        if (x_dev != y_dev && hipMemcpyAsync(y_dev, x_dev, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess)
            return failf(USE_E_HIP, "use_resample_fft_dev: copy failed: %s", hipGetErrorString(hipGetLastError()));
        return USE_OK;
    }
    resample_launch(x_dev, n, num, y_dev, static_cast<char*>(work), w, st);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(USE_E_HIP, "use_resample_fft_dev: launch failed: %s", hipGetErrorString(e));
    return USE_OK;
}

int use_load_items_dev(const double* const* x_dev, const int64_t* n_host, const int64_t* num_host, int B, int normalize, float* wav,
                       int64_t stride, void* work, size_t work_bytes, use_stream_t s) {
    return use_load_items_dev_peak(x_dev, n_host, num_host, B, normalize, wav, stride, work, work_bytes, nullptr, s);
}

int use_load_items_dev_peak(const double* const* x_dev, const int64_t* n_host, const int64_t* num_host, int B, int normalize, float* wav,
                            int64_t stride, void* work, size_t work_bytes, double* peak_dev, use_stream_t s) {
    if ((uintptr_t)peak_dev & 7) return failf(USE_E_INVALID, "use_load_items_dev: peak_dev must be 8-byte aligned");
    if (B < 1) return failf(USE_E_INVALID, "use_load_items_dev: B=%d must be positive", B);
    if (!x_dev) return failf(USE_E_INVALID, "use_load_items_dev: x_dev is null");
    if (!n_host) return failf(USE_E_INVALID, "use_load_items_dev: n_host is null");
    if (!num_host) return failf(USE_E_INVALID, "use_load_items_dev: num_host is null");
    if (!wav) return failf(USE_E_INVALID, "use_load_items_dev: wav is null");
    if (!work) return failf(USE_E_INVALID, "use_load_items_dev: work is null");
    if ((uintptr_t)work & 15) return failf(USE_E_INVALID, "use_load_items_dev: work must be 16-byte aligned");
    if ((uintptr_t)wav & 3) return failf(USE_E_INVALID, "use_load_items_dev: wav must be 4-byte aligned");
    if (stride < 1 || (stride + LOAD_SLICE - 1) / LOAD_SLICE > 0x7fffffff)
        return failf(USE_E_INVALID, "use_load_items_dev: stride=%lld must be positive (and below 2^43)", (long long)stride);
    for (int b = 0; b < B; ++b) {
        const int64_t n = n_host[b], num = num_host[b];
        if (n < 1 || num < 1)
            return failf(USE_E_INVALID, "use_load_items_dev: n[%d]=%lld and num[%d]=%lld must be positive", b, (long long)n, b, (long long)num);
        if (!item_ok(n, num))
            return failf(USE_E_INVALID, "use_load_items_dev: max(n[%d], num[%d])=%lld exceeds 2^24", b, b, (long long)(n > num ? n : num));
        if (!x_dev[b] || ((uintptr_t)x_dev[b] & 7)) return failf(USE_E_INVALID, "use_load_items_dev: x_dev[%d] is null or not 8-byte aligned", b);
        if (stride < num)
            return failf(USE_E_INVALID, "use_load_items_dev: stride=%lld is smaller than num[%d]=%lld", (long long)stride, b, (long long)num);
        const size_t need = item_layout(n, num).bytes;
        if (work_bytes < need)
            return failf(USE_E_INVALID, "use_load_items_dev: work_bytes=%zu is smaller than use_resample_workspace(%lld, %lld) = %zu (item %d)",
                         work_bytes, (long long)n, (long long)num, need, b);
    }
    hipStream_t st = (hipStream_t)s;
    char* base = static_cast<char*>(work);
    for (int b = 0; b < B; ++b) {
        const int64_t n = n_host[b], num = num_host[b];
        const ItemWork w = item_layout(n, num);
        const double* v = x_dev[b];
        if (n != num) {
            double* y = reinterpret_cast<double*>(base + w.y);
            resample_launch(x_dev[b], n, num, y, base, w, st);
            v = y;
        }
        double* part = reinterpret_cast<double*>(base + w.part);
        const int np = (int)((num + LOAD_SLICE - 1) / LOAD_SLICE);
        float* row = wav + (int64_t)b * stride;
        const dim3 grid((unsigned)((stride + LOAD_SLICE - 1) / LOAD_SLICE)), block(256);
        if (normalize) {
            hipLaunchKernelGGL(load_peak_kernel, dim3(np), block, 0, st, v, num, part);
            hipLaunchKernelGGL(load_scale_kernel<1>, grid, block, 0, st, v, num, part, np, row, stride, peak_dev ? peak_dev + b : (double*)nullptr);
        } else {
            hipLaunchKernelGGL(load_scale_kernel<0>, grid, block, 0, st, v, num, part, np, row, stride, (double*)nullptr);
        }
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(USE_E_HIP, "use_load_items_dev: launch failed: %s", hipGetErrorString(e));
    return USE_OK;
}

size_t use_store_workspace(int64_t len, int64_t num) {
    if (!item_ok(len, num)) return 0;
    return store_bytes(len, num);
}

int use_store_items_dev(const float* wav, int64_t stride, const int* len_host, const int64_t* num_host, int B, int subtype, void* out,
                        int64_t out_stride, void* work, size_t work_bytes, use_stream_t s) {
    return use_store_items_dev_gain(wav, stride, len_host, num_host, nullptr, B, subtype, out, out_stride, work, work_bytes, s);
}

int use_store_items_dev_gain(const float* wav, int64_t stride, const int* len_host, const int64_t* num_host, const double* gain_host, int B,
                             int subtype, void* out, int64_t out_stride, void* work, size_t work_bytes, use_stream_t s) {
    if (B < 1) return failf(USE_E_INVALID, "use_store_items_dev: B=%d must be positive", B);
    if (subtype != USE_WAV_PCM16 && subtype != USE_WAV_FLOAT32) return failf(USE_E_INVALID, "use_store_items_dev: unknown subtype %d", subtype);
    if (!wav) return failf(USE_E_INVALID, "use_store_items_dev: wav is null");
    if (!len_host) return failf(USE_E_INVALID, "use_store_items_dev: len_host is null");
    if (!num_host) return failf(USE_E_INVALID, "use_store_items_dev: num_host is null");
    if (!out) return failf(USE_E_INVALID, "use_store_items_dev: out is null");
    if (!work) return failf(USE_E_INVALID, "use_store_items_dev: work is null");
    if ((uintptr_t)wav & 3) return failf(USE_E_INVALID, "use_store_items_dev: wav must be 4-byte aligned");
    const int bps = subtype == USE_WAV_PCM16 ? 2 : 4;
    if ((uintptr_t)out & (uintptr_t)(bps - 1)) return failf(USE_E_INVALID, "use_store_items_dev: out must be %d-byte aligned", bps);
    if ((uintptr_t)work & 15) return failf(USE_E_INVALID, "use_store_items_dev: work must be 16-byte aligned");
    if (stride < 1) return failf(USE_E_INVALID, "use_store_items_dev: stride=%lld must be positive", (long long)stride);
    if (out_stride < 1 || (out_stride + LOAD_SLICE - 1) / LOAD_SLICE > 0x7fffffff)
        return failf(USE_E_INVALID, "use_store_items_dev: out_stride=%lld must be positive (and below 2^43)", (long long)out_stride);
    for (int b = 0; b < B; ++b) {
        const int64_t len = len_host[b], num = num_host[b];
        if (len < 1 || num < 1)
            return failf(USE_E_INVALID, "use_store_items_dev: len[%d]=%lld and num[%d]=%lld must be positive", b, (long long)len, b, (long long)num);
        if (len > stride)
            return failf(USE_E_INVALID, "use_store_items_dev: len[%d]=%lld is larger than stride=%lld", b, (long long)len, (long long)stride);
        if (num > out_stride)
            return failf(USE_E_INVALID, "use_store_items_dev: num[%d]=%lld is larger than out_stride=%lld", b, (long long)num, (long long)out_stride);
        if (!item_ok(len, num))
            return failf(USE_E_INVALID, "use_store_items_dev: max(len[%d], num[%d])=%lld exceeds 2^24", b, b, (long long)(len > num ? len : num));
        const size_t need = store_bytes(len, num);
        if (work_bytes < need)
            return failf(USE_E_INVALID, "use_store_items_dev: work_bytes=%zu is smaller than use_store_workspace(%lld, %lld) = %zu (item %d)",
                         work_bytes, (long long)len, (long long)num, need, b);
    }
    if (gains_ok("use_store_items_dev", gain_host, B)) return USE_E_INVALID;
    hipStream_t st = (hipStream_t)s;
    char* base = static_cast<char*>(work);
    for (int b = 0; b < B; ++b) {
        const float* row = wav + (int64_t)b * stride;
        const double* g = gain_host ? gain_host + b : nullptr;
        if (subtype == USE_WAV_PCM16)
            store_launch(row, len_host[b], num_host[b], static_cast<int16_t*>(out) + (int64_t)b * out_stride, out_stride, g, base, st);
        else store_launch(row, len_host[b], num_host[b], static_cast<float*>(out) + (int64_t)b * out_stride, out_stride, g, base, st);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(USE_E_HIP, "use_store_items_dev: launch failed: %s", hipGetErrorString(e));
    return USE_OK;
}

size_t use_load_files_workspace(int64_t n, int64_t num, int channels) {
    if (!item_ok(n, num) || !channels_ok(channels)) return 0;
    return file_layout(n, num, channels).bytes;
}

int use_load_files_dev(const double* const* x_dev, const int64_t* n_host, const int64_t* num_host, const int* ch_host, int F, int normalize,
                       float* wav, int64_t stride, void* work, size_t work_bytes, use_stream_t s) {
    return use_load_files_dev_peak(x_dev, n_host, num_host, ch_host, F, normalize, wav, stride, work, work_bytes, nullptr, s);
}

int use_load_files_dev_peak(const double* const* x_dev, const int64_t* n_host, const int64_t* num_host, const int* ch_host, int F, int normalize,
                            float* wav, int64_t stride, void* work, size_t work_bytes, double* peak_dev, use_stream_t s) {
    if ((uintptr_t)peak_dev & 7) return failf(USE_E_INVALID, "use_load_files_dev: peak_dev must be 8-byte aligned");
    if (F < 1) return failf(USE_E_INVALID, "use_load_files_dev: F=%d must be positive", F);
    if (!x_dev) return failf(USE_E_INVALID, "use_load_files_dev: x_dev is null");
    if (!n_host) return failf(USE_E_INVALID, "use_load_files_dev: n_host is null");
    if (!num_host) return failf(USE_E_INVALID, "use_load_files_dev: num_host is null");
    if (!ch_host) return failf(USE_E_INVALID, "use_load_files_dev: ch_host is null");
    if (!wav) return failf(USE_E_INVALID, "use_load_files_dev: wav is null");
    if (!work) return failf(USE_E_INVALID, "use_load_files_dev: work is null");
    if ((uintptr_t)work & 15) return failf(USE_E_INVALID, "use_load_files_dev: work must be 16-byte aligned");
    if ((uintptr_t)wav & 3) return failf(USE_E_INVALID, "use_load_files_dev: wav must be 4-byte aligned");
    if (stride < 1 || (stride + LOAD_SLICE - 1) / LOAD_SLICE > 0x7fffffff)
        return failf(USE_E_INVALID, "use_load_files_dev: stride=%lld must be positive (and below 2^43)", (long long)stride);
    for (int f = 0; f < F; ++f) {
        const int64_t n = n_host[f], num = num_host[f];
        if (!channels_ok(ch_host[f])) return failf(USE_E_INVALID, "use_load_files_dev: ch[%d]=%d must lie in 1 ... %d", f, ch_host[f], FILE_MAX_CHANNELS);
        if (n < 1 || num < 1)
            return failf(USE_E_INVALID, "use_load_files_dev: n[%d]=%lld and num[%d]=%lld must be positive", f, (long long)n, f, (long long)num);
        if (!item_ok(n, num))
            return failf(USE_E_INVALID, "use_load_files_dev: max(n[%d], num[%d])=%lld exceeds 2^24", f, f, (long long)(n > num ? n : num));
        if (!x_dev[f] || ((uintptr_t)x_dev[f] & 7)) return failf(USE_E_INVALID, "use_load_files_dev: x_dev[%d] is null or not 8-byte aligned", f);
        if (stride < num)
            return failf(USE_E_INVALID, "use_load_files_dev: stride=%lld is smaller than num[%d]=%lld", (long long)stride, f, (long long)num);
        const size_t need = file_layout(n, num, ch_host[f]).bytes;
        if (work_bytes < need)
            return failf(USE_E_INVALID, "use_load_files_dev: work_bytes=%zu is smaller than use_load_files_workspace(%lld, %lld, %d) = %zu (file %d)",
                         work_bytes, (long long)n, (long long)num, ch_host[f], need, f);
    }
    hipStream_t st = (hipStream_t)s;
    int64_t row0 = 0;                                              // file f's rows: row0 ... row0 + ch[f] - 1
    for (int f = 0; f < F; ++f) {
        load_file_launch(x_dev[f], n_host[f], num_host[f], ch_host[f], normalize, wav + row0 * stride, stride,
                         peak_dev ? peak_dev + f : (double*)nullptr, static_cast<char*>(work), st);
        row0 += ch_host[f];
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(USE_E_HIP, "use_load_files_dev: launch failed: %s", hipGetErrorString(e));
    return USE_OK;
}

int use_store_files_dev(const float* wav, int64_t stride, const int* len_host, const int64_t* num_host, const int* ch_host,
                        const int64_t* out_off_host, int F, int subtype, void* out, void* work, size_t work_bytes, use_stream_t s) {
    return use_store_files_dev_gain(wav, stride, len_host, num_host, ch_host, out_off_host, nullptr, F, subtype, out, work, work_bytes, s);
}

int use_store_files_dev_gain(const float* wav, int64_t stride, const int* len_host, const int64_t* num_host, const int* ch_host,
                             const int64_t* out_off_host, const double* gain_host, int F, int subtype, void* out, void* work, size_t work_bytes,
                             use_stream_t s) {
    if (F < 1) return failf(USE_E_INVALID, "use_store_files_dev: F=%d must be positive", F);
    if (subtype != USE_WAV_PCM16 && subtype != USE_WAV_FLOAT32) return failf(USE_E_INVALID, "use_store_files_dev: unknown subtype %d", subtype);
    if (!wav) return failf(USE_E_INVALID, "use_store_files_dev: wav is null");
    if (!len_host) return failf(USE_E_INVALID, "use_store_files_dev: len_host is null");
    if (!num_host) return failf(USE_E_INVALID, "use_store_files_dev: num_host is null");
    if (!ch_host) return failf(USE_E_INVALID, "use_store_files_dev: ch_host is null");
    if (!out_off_host) return failf(USE_E_INVALID, "use_store_files_dev: out_off_host is null");
    if (!out) return failf(USE_E_INVALID, "use_store_files_dev: out is null");
    if (!work) return failf(USE_E_INVALID, "use_store_files_dev: work is null");
    if ((uintptr_t)wav & 3) return failf(USE_E_INVALID, "use_store_files_dev: wav must be 4-byte aligned");
    const int bps = subtype == USE_WAV_PCM16 ? 2 : 4;
    if ((uintptr_t)out & (uintptr_t)(bps - 1)) return failf(USE_E_INVALID, "use_store_files_dev: out must be %d-byte aligned", bps);
    if ((uintptr_t)work & 15) return failf(USE_E_INVALID, "use_store_files_dev: work must be 16-byte aligned");
    if (stride < 1) return failf(USE_E_INVALID, "use_store_files_dev: stride=%lld must be positive", (long long)stride);
    for (int f = 0; f < F; ++f) {
        const int64_t len = len_host[f], num = num_host[f];
        if (!channels_ok(ch_host[f])) return failf(USE_E_INVALID, "use_store_files_dev: ch[%d]=%d must lie in 1 ... %d", f, ch_host[f], FILE_MAX_CHANNELS);
        if (len < 1 || num < 1)
            return failf(USE_E_INVALID, "use_store_files_dev: len[%d]=%lld and num[%d]=%lld must be positive", f, (long long)len, f, (long long)num);
        if (len > stride)
            return failf(USE_E_INVALID, "use_store_files_dev: len[%d]=%lld is larger than stride=%lld", f, (long long)len, (long long)stride);
        if (!item_ok(len, num))
            return failf(USE_E_INVALID, "use_store_files_dev: max(len[%d], num[%d])=%lld exceeds 2^24", f, f, (long long)(len > num ? len : num));
        if (out_off_host[f] < 0) return failf(USE_E_INVALID, "use_store_files_dev: out_off[%d]=%lld must not be negative", f, (long long)out_off_host[f]);
        const size_t need = store_bytes(len, num);
        if (work_bytes < need)
            return failf(USE_E_INVALID, "use_store_files_dev: work_bytes=%zu is smaller than use_store_workspace(%lld, %lld) = %zu (file %d)",
                         work_bytes, (long long)len, (long long)num, need, f);
    }
    if (gains_ok("use_store_files_dev", gain_host, F)) return USE_E_INVALID;
    hipStream_t st = (hipStream_t)s;
    char* base = static_cast<char*>(work);
    int64_t row0 = 0;
    for (int f = 0; f < F; ++f) {
        const float* rows = wav + row0 * stride;
        const double* g = gain_host ? gain_host + f : nullptr;
        if (subtype == USE_WAV_PCM16)
            store_file_launch(rows, stride, len_host[f], num_host[f], ch_host[f], static_cast<int16_t*>(out) + out_off_host[f], g, base, st);
        else store_file_launch(rows, stride, len_host[f], num_host[f], ch_host[f], static_cast<float*>(out) + out_off_host[f], g, base, st);
        row0 += ch_host[f];
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(USE_E_HIP, "use_store_files_dev: launch failed: %s", hipGetErrorString(e));
    return USE_OK;
}
