// The degradation simulator of the training data on the device (use_distort; include/use_hip.h lists the stages): per item of a batch
// reverberation, noise at an SNR over the non-silent samples, loudness intervals, one of five clippers, a DC offset, packet loss, and
// the volume steps on the pair (noisy, clean) - in fp64 after the load, the parameters drawn by the host.
//
//   signals     y (the noisy branch) and c (the clean target) are fp64 arrays of len samples in the workspace, rewritten in place by the
//               elementwise kernels; a workgroup owns a slice of DIST_SLICE = 4096 samples (256 threads x 16, strided by 256).
//   statistics  a stage that needs a statistic of the stage before it gets it from that stage's elementwise pass: every workgroup stores
//               its slice's partial (maximum, minimum, sum of squares) by a plain store, and ONE workgroup of a small kernel re-reduces
//               the partials - thread t takes t, t + 256, ... in that order, then a fixed tree - and leaves the scalar in S[] (workspace).
//               The kernels after it read S[] and derive what they need (the noise scale, the energy ratio) with the same arithmetic in
//               every thread.  More than 256 partials (len > 2^20) only lengthens the strided loop.
//   VAD         sums of squares E_k of the blocks of 512 samples (one wave per block: 8 values per lane in order, then the wave's tree);
//               the power of frame k (2048 samples centred at 512 k, zero-padded) is (E_{k-2} + E_{k-1} + E_k + E_{k+1}) / 2048, and the
//               samples of block k are kept iff frame k is: P = sum of the kept E_k / the number of kept samples.
//   histogram   numpy's rule for 1000 uniform bins (scaled index, then the two corrections against the edges linspace gives); counts
//               are integers, so LDS and global integer atomics leave them order-free.
//   reverb      X = FFT(x), H = FFT(h) at M = pow2 >= len + r - 1 on the shared Stockham passes (use_fft.h), y = Re IFFT(X H) / M: three
//               transforms over three buffers.  The early part is a direct sum of at most 6 taps.
// No float atomics, no contraction of a product into a sum (the whole file is compiled with contraction off: a stage that is one
// rounded operation per sample has numpy's bits).  Items run one after another on the stream and share nothing but the workspace, so
// an item's rows and scalars do not depend on its batch, its row or the strides.
#include <cmath>
#include <cstdarg>
#include <cstdio>

#include "../../include/use_hip.h"
#include "use_fft.h"

#pragma clang fp contract(off)

int use_set_error(int code, const char* msg);   // use_engine.cpp

namespace use {

namespace {

constexpr int DIST_SLICE = 4096;                  // samples per workgroup of the elementwise kernels
constexpr int VAD_HOP = 512, VAD_FRAME = 2048;    // librosa.effects.split's defaults
constexpr int VAD_BLOCKS = 8;                     // blocks of VAD_HOP samples per workgroup of block_energy_kernel (two per wave)
constexpr int HIST_BINS = 1000;
constexpr int64_t DIST_FFT_MAX = (int64_t)1 << 24;   // len + rir_len - 1 at most
constexpr int EARLY_TAPS = 6;

// S[]: the item's scalars on the device
enum { S_P0 = 0, S_P1 = 1, S_XMAX = 2, S_SUMSQ = 3, S_AMIN = 4, S_AMAX = 5, S_THR = 6, S_SUMSQ2 = 7, S_VOL = 8, S_CLIPS = 9, S_CLIPF = 10,
       S_NORM = 11, S_COUNT = 16 };

struct Loud { int n; double f[5]; };

// ---- fixed-shape reductions over the 256 threads of a workgroup; every thread gets the result ----
struct OpSum { __device__ static double f(double a, double b) { return a + b; } };
struct OpMax { __device__ static double f(double a, double b) { return b > a ? b : a; } };
struct OpMin { __device__ static double f(double a, double b) { return b < a ? b : a; } };

template <typename OP>
__device__ __forceinline__ double wave_reduce(double v) {
    for (int off = 32; off > 0; off >>= 1) v = OP::f(v, __shfl_down(v, off, 64));
    return v;
}

template <typename OP>
__device__ __forceinline__ double block_reduce(double v, double* sh) {
    v = wave_reduce<OP>(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return OP::f(OP::f(sh[0], sh[1]), OP::f(sh[2], sh[3]));
}

// ---- stage 1 ----
// y[i] = c[i] = x[i]; with taps (h != null): c[i] = sum_{j < min(6, r), j <= i} x[i - j] h[j], j ascending (y comes from the FFT)
__global__ __launch_bounds__(256) void load_kernel(const float* __restrict__ x, const float* __restrict__ h, int r, int64_t len,
                                                   double* __restrict__ y, double* __restrict__ c) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    const double v = (double)x[i];
    if (!h) { y[i] = v; c[i] = v; return; }
    const int taps = r < EARLY_TAPS ? r : EARLY_TAPS;
    double acc = 0.0;
    for (int j = 0; j < taps && j <= i; ++j) acc = acc + (double)x[i - j] * (double)h[j];
    c[i] = acc;
}

// A[i] = x[i] (i < len), B[i] = h[i] (i < r), both real and zero up to M: two transforms.  One transform of x + i h would be cheaper, but
// it leaves in each spectrum an error of eps |Z|, and next to a long signal (|X| ~ sqrt(len)) a short response (|H| ~ 1) drowns in it
__global__ __launch_bounds__(256) void pack_kernel(const float* __restrict__ x, int64_t len, const float* __restrict__ h, int r,
                                                   double2* __restrict__ A, double2* __restrict__ B, int64_t M) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    A[i] = make_double2(i < len ? (double)x[i] : 0.0, 0.0);
    B[i] = make_double2(i < r ? (double)h[i] : 0.0, 0.0);
}

// X[k] *= H[k]
__global__ __launch_bounds__(256) void product_kernel(double2* __restrict__ X, const double2* __restrict__ H, int64_t M) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= M) return;
    const double2 a = X[k], b = H[k];
    X[k] = make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// y[i] = Re R[i] / M
__global__ __launch_bounds__(256) void unpack_kernel(const double2* __restrict__ R, double inv, int64_t len, double* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < len) y[i] = R[i].x * inv;
}

// ---- the masked power of stage 2 (and of the RMS volume) ----
// E[k] = sum of v^2 over block k (samples 512 k ... min(len, 512 k + 512)); grid ceil(nb / VAD_BLOCKS)
template <typename SRC>
__global__ __launch_bounds__(256) void block_energy_kernel(const SRC* __restrict__ v, int64_t len, int nb, double* __restrict__ E) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int q = 0; q < VAD_BLOCKS / 4; ++q) {
        const int k = blockIdx.x * VAD_BLOCKS + q * 4 + wave;     // uniform over the wave
        if (k >= nb) continue;
        const int64_t base = (int64_t)k * VAD_HOP;
        double s = 0.0;
        for (int j = 0; j < VAD_HOP / 64; ++j) {
            const int64_t i = base + lane + 64 * j;
            const double a = i < len ? (double)v[i] : 0.0;
            s = s + a * a;
        }
        s = wave_reduce<OpSum>(s);
        if (lane == 0) E[k] = s;
    }
}

__device__ __forceinline__ double frame_power(const double* E, int nb, int k) {
    double s = 0.0;
    for (int j = k - 2; j <= k + 1; ++j) s = s + (j >= 0 && j < nb ? E[j] : 0.0);
    return s / (double)VAD_FRAME;
}

__device__ __forceinline__ double power_db(double p) { return 10.0 * log10(p > 1e-10 ? p : 1e-10); }

// grid 2: workgroup g takes the block energies E + g * e_stride -> S[S_P0 + g] = P; keep (or null) + g * keep_stride: the frames' flags
__global__ __launch_bounds__(256) void vad_final_kernel(const double* __restrict__ Eall, int64_t e_stride, int64_t len, int nb, double* __restrict__ S,
                                                        unsigned char* __restrict__ keep, int64_t keep_stride) {
    __shared__ double sh[4];
    const double* E = Eall + blockIdx.x * e_stride;
    const int nf = 1 + (int)(len / VAD_HOP);
    double mx = 0.0;
    for (int k = threadIdx.x; k < nf; k += 256) mx = OpMax::f(mx, frame_power(E, nb, k));
    mx = block_reduce<OpMax>(mx, sh);
    const double ref = power_db(mx);
    double s = 0.0, cnt = 0.0;
    for (int k = threadIdx.x; k < nf; k += 256) {
        const bool kept = power_db(frame_power(E, nb, k)) - ref > -50.0;
        if (keep) keep[blockIdx.x * keep_stride + k] = kept ? 1 : 0;
        if (kept && k < nb) {
            const int64_t left = len - (int64_t)k * VAD_HOP;
            s = s + E[k];
            cnt = cnt + (double)(left < VAD_HOP ? left : VAD_HOP);
        }
    }
    s = block_reduce<OpSum>(s, sh);
    cnt = block_reduce<OpSum>(cnt, sh);                            // integers: exact
    if (threadIdx.x == 0) S[S_P0 + blockIdx.x] = s / cnt;
}

__device__ __forceinline__ double noise_scale(const double* S, double snr_lin) {
    return sqrt(S[S_P0] / (S[S_P1] + 1e-8) / snr_lin + 1e-8);
}

// ---- stages 2 and 3, and the statistics stage 4 asks for ----
// y = (y + scale * noise) * loud; part[0 .. 3][np]: the slice's signed maximum, sum of squares, minimum and maximum of |y|
__global__ __launch_bounds__(256) void mix_kernel(double* __restrict__ y, int64_t len, const float* __restrict__ noise, double snr_lin, const Loud loud,
                                                  const double* __restrict__ S, double* __restrict__ part, int np, double* __restrict__ scal) {
    __shared__ double sh[4];
    const int64_t lo = (int64_t)blockIdx.x * DIST_SLICE, hi = lo + DIST_SLICE < len ? lo + DIST_SLICE : len;
    const double sc = noise ? noise_scale(S, snr_lin) : 0.0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        scal[USE_DISTORT_NOISE_SCALE] = sc;
        scal[USE_DISTORT_P_CLEAN] = noise ? S[S_P0] : 0.0;
        scal[USE_DISTORT_P_NOISE] = noise ? S[S_P1] : 0.0;
    }
    const int64_t interval = loud.n > 0 ? len / loud.n : 0;
    double mx = -INFINITY, ss = 0.0, amin = INFINITY, amax = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        double v = y[i];
        if (noise) v = v + (double)noise[i] * sc;
        if (interval > 0) {
            const int64_t q = i / interval;
            if (q < loud.n) v = loud.f[q] * v;
        }
        y[i] = v;
        const double a = fabs(v);
        mx = OpMax::f(mx, v); ss = ss + v * v; amin = OpMin::f(amin, a); amax = OpMax::f(amax, a);
    }
    mx = block_reduce<OpMax>(mx, sh); ss = block_reduce<OpSum>(ss, sh);
    amin = block_reduce<OpMin>(amin, sh); amax = block_reduce<OpMax>(amax, sh);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = mx; part[np + blockIdx.x] = ss; part[2 * np + blockIdx.x] = amin; part[3 * np + blockIdx.x] = amax;
    }
}

// one workgroup: the partials of mix_kernel -> S; the histogram is zeroed for hist_kernel
__global__ __launch_bounds__(256) void stat_final_kernel(const double* __restrict__ part, int np, double* __restrict__ S, int* __restrict__ hist) {
    __shared__ double sh[4];
    double mx = -INFINITY, ss = 0.0, amin = INFINITY, amax = 0.0;
    for (int j = threadIdx.x; j < np; j += 256) {
        mx = OpMax::f(mx, part[j]); ss = ss + part[np + j]; amin = OpMin::f(amin, part[2 * np + j]); amax = OpMax::f(amax, part[3 * np + j]);
    }
    mx = block_reduce<OpMax>(mx, sh); ss = block_reduce<OpSum>(ss, sh);
    amin = block_reduce<OpMin>(amin, sh); amax = block_reduce<OpMax>(amax, sh);
    if (threadIdx.x == 0) { S[S_XMAX] = mx; S[S_SUMSQ] = ss; S[S_AMIN] = amin; S[S_AMAX] = amax; }
    for (int b = threadIdx.x; b < HIST_BINS; b += 256) hist[b] = 0;
}

// ---- stage 4: the threshold of clip-on-rate ----
struct HistRange { double first, last, denom, step; };
__device__ __forceinline__ HistRange hist_range(const double* S) {
    HistRange g;
    g.first = S[S_AMIN]; g.last = S[S_AMAX];
    if (g.first == g.last) { g.first = g.first - 0.5; g.last = g.last + 0.5; }       // numpy widens an empty range
    g.denom = g.last - g.first;
    g.step = g.denom / (double)HIST_BINS;
    return g;
}
// np.linspace(first, last, 1001)[i]
__device__ __forceinline__ double hist_edge(const HistRange g, int i) { return i == HIST_BINS ? g.last : (double)i * g.step + g.first; }

__global__ __launch_bounds__(256) void hist_kernel(const double* __restrict__ y, int64_t len, const double* __restrict__ S, int* __restrict__ hist) {
    __shared__ int h[HIST_BINS];
    for (int b = threadIdx.x; b < HIST_BINS; b += 256) h[b] = 0;
    __syncthreads();
    const HistRange g = hist_range(S);
    const int64_t lo = (int64_t)blockIdx.x * DIST_SLICE, hi = lo + DIST_SLICE < len ? lo + DIST_SLICE : len;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        const double a = fabs(y[i]);
        if (!(a >= g.first && a <= g.last)) continue;              // a NaN: numpy would have refused the range
        const double f = ((a - g.first) / g.denom) * (double)HIST_BINS;
        if (!(f >= 0.0 && f <= (double)HIST_BINS)) continue;       // an infinite range: no bin (numpy would have refused it)
        int idx = (int)f;
        if (idx == HIST_BINS) idx = HIST_BINS - 1;
        if (a < hist_edge(g, idx)) idx -= 1;
        if (a >= hist_edge(g, idx + 1) && idx != HIST_BINS - 1) idx += 1;
        atomicAdd(&h[idx], 1);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < HIST_BINS; b += 256)
        if (h[b]) atomicAdd(&hist[b], h[b]);
}

// one thread: the first left edge whose cumulative count exceeds (1 - rate) len
__global__ void threshold_kernel(const int* __restrict__ hist, int64_t len, double rate, double* __restrict__ S) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const HistRange g = hist_range(S);
    const double target = (1.0 - rate) * (double)len;
    int64_t cum = 0;
    int idx = HIST_BINS - 1;
    for (int b = 0; b < HIST_BINS; ++b) {
        cum += hist[b];
        if ((double)cum > target) { idx = b; break; }
    }
    S[S_THR] = hist_edge(g, idx);
}

__device__ __forceinline__ double clip_sym(double v, double t) { return fmin(fmax(v, -t), t); }

// y = clip(y); part[np]: the slice's sum of squares after the clipper (the sigmoids' second energy)
__global__ __launch_bounds__(256) void clip_kernel(double* __restrict__ y, int64_t len, int kind, double pa, double pb, const double* __restrict__ S,
                                                   double* __restrict__ part, double* __restrict__ scal) {
    __shared__ double sh[4];
    const int64_t lo = (int64_t)blockIdx.x * DIST_SLICE, hi = lo + DIST_SLICE < len ? lo + DIST_SLICE : len;
    const double thr = kind == USE_CLIP_HARD_ON_RATE ? S[S_THR] : pa, xmax = S[S_XMAX];
    const double inv_p = 1.0 / pa, den0 = kind == USE_CLIP_SOFT ? pow(fabs(xmax), pa) : 0.0;
    if (blockIdx.x == 0 && threadIdx.x == 0)
        scal[USE_DISTORT_CLIP_THRESHOLD] = kind == USE_CLIP_HARD || kind == USE_CLIP_HARD_ON_RATE || kind == USE_CLIP_SIGMOID2 ? thr : 0.0;
    double ss = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        double v = y[i];
        switch (kind) {
        case USE_CLIP_HARD: case USE_CLIP_HARD_ON_RATE: v = clip_sym(v, thr); break;
        case USE_CLIP_SOFT: v = xmax * v / pow(den0 + pow(fabs(v), pa) + 1e-5, inv_p); break;
        case USE_CLIP_SIGMOID1: v = (2.0 / (1.0 + exp(-pa * v)) - 1.0) * pb; break;
        case USE_CLIP_SIGMOID2: {
            const double xc = clip_sym(v, thr), b = 1.5 * xc - 0.3 * (xc * xc), a = b > 0.0 ? 4.0 : 0.5;
            v = pb * (2.0 / (1.0 + exp(-a * b)) - 1.0);
            break;
        }
        default: break;
        }
        y[i] = v;
        ss = ss + v * v;
    }
    ss = block_reduce<OpSum>(ss, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = ss;
}

// one workgroup: S[slot] = the sum of part[0 .. np)
__global__ __launch_bounds__(256) void sum_final_kernel(const double* __restrict__ part, int np, double* __restrict__ S, int slot) {
    __shared__ double sh[4];
    double ss = 0.0;
    for (int j = threadIdx.x; j < np; j += 256) ss = ss + part[j];
    ss = block_reduce<OpSum>(ss, sh);
    if (threadIdx.x == 0) S[slot] = ss;
}

// ---- stages 5 and 6, the sigmoids' energy ratio before them; the peaks stage 7 asks for ----
// part[0 .. 1][np]: the slice's max |y| and max |c|
__global__ __launch_bounds__(256) void post_kernel(double* __restrict__ y, const double* __restrict__ c, int64_t len, int sigmoid, int dc, double dc_offset,
                                                   const double* __restrict__ packet, int frame, const double* __restrict__ S,
                                                   double* __restrict__ part, int np, double* __restrict__ scal) {
    __shared__ double sh[4];
    const int64_t lo = (int64_t)blockIdx.x * DIST_SLICE, hi = lo + DIST_SLICE < len ? lo + DIST_SLICE : len;
    double es = 1.0;
    if (sigmoid) es = sqrt(S[S_SUMSQ] / (double)len) / (sqrt(S[S_SUMSQ2] / (double)len) + 1e-8);
    if (blockIdx.x == 0 && threadIdx.x == 0) scal[USE_DISTORT_ENERGY_SCALE] = es;
    double py = 0.0, pc = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        double v = y[i];
        if (sigmoid) v = v * es;
        if (dc) v = v + dc_offset;
        if (frame > 0) v = v * packet[i / frame];
        y[i] = v;
        py = OpMax::f(py, fabs(v)); pc = OpMax::f(pc, fabs(c[i]));
    }
    py = block_reduce<OpMax>(py, sh); pc = block_reduce<OpMax>(pc, sh);
    if (threadIdx.x == 0) { part[blockIdx.x] = py; part[np + blockIdx.x] = pc; }
}

// ---- stage 7 ----
// one workgroup: the peaks -> the volume scale, the clip scale and its flag, the normalisation factor
__global__ __launch_bounds__(256) void volume_final_kernel(const double* __restrict__ part, int np, int volume, double target, int normalize,
                                                           double* __restrict__ S, double* __restrict__ scal) {
    __shared__ double sh[4];
    double py = 0.0, pc = 0.0;
    for (int j = threadIdx.x; j < np; j += 256) { py = OpMax::f(py, part[j]); pc = OpMax::f(pc, part[np + j]); }
    py = block_reduce<OpMax>(py, sh); pc = block_reduce<OpMax>(pc, sh);
    if (threadIdx.x != 0) return;
    double vs = 1.0, cs = 1.0, cf = 0.0;
    if (volume != USE_VOLUME_NONE) {
        double ly = py, lc = pc;
        if (volume == USE_VOLUME_RMS) { ly = sqrt(S[S_P0] + 1e-8); lc = sqrt(S[S_P1] + 1e-8); }
        vs = target / ((ly > lc ? ly : lc) + 1e-6);
        py = py * vs; pc = pc * vs;                               // rounding is monotonic: the peak of the scaled signal
        const double m = py > pc ? py : pc;
        if (m > 0.99) { cf = 1.0; cs = 0.99 / m; py = py * cs; pc = pc * cs; }
    }
    const double nf = py > pc ? py : pc;
    S[S_VOL] = vs; S[S_CLIPS] = cs; S[S_CLIPF] = cf; S[S_NORM] = nf;
    scal[USE_DISTORT_VOLUME_SCALE] = vs; scal[USE_DISTORT_CLIP_SCALE] = cs; scal[USE_DISTORT_NORM_FACTOR] = normalize ? nf : 1.0;
}

// grid (ceil(stride / DIST_SLICE), 2): row y (0) or c (1) under the volume steps, cast to T, zero from len to stride
template <typename T>
__global__ __launch_bounds__(256) void store_kernel(const double* __restrict__ y, const double* __restrict__ c, int64_t len, int volume, int normalize,
                                                    const double* __restrict__ S, T* __restrict__ out_y, T* __restrict__ out_c, int64_t stride) {
    const int64_t lo = (int64_t)blockIdx.x * DIST_SLICE, hi = lo + DIST_SLICE < stride ? lo + DIST_SLICE : stride;
    const double* src = blockIdx.y ? c : y;
    T* dst = blockIdx.y ? out_c : out_y;
    const double vs = S[S_VOL], cs = S[S_CLIPS], nf = S[S_NORM];
    const bool cf = S[S_CLIPF] != 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        double v = 0.0;
        if (i < len) {
            v = src[i];
            if (volume) v = v * vs;
            if (cf) v = v * cs;
            if (normalize) v = v / nf * 0.8;
        }
        dst[i] = (T)v;
    }
}

int failf(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    return use_set_error(code, buf);
}

// ---- host: the workspace of one item and its launches ----
struct DistWork { size_t y, c, E, part, hist, S, fft, bytes; int64_t M; int nb, np; };
size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
DistWork dist_layout(int64_t len, int64_t r) {
    DistWork w;
    w.nb = (int)((len + VAD_HOP - 1) / VAD_HOP);
    w.np = (int)((len + DIST_SLICE - 1) / DIST_SLICE);
    w.M = r > 0 ? (int64_t)1 << ceil_log2(len + r - 1) : 0;
    w.y = 0;
    w.c = w.y + align16((size_t)len * sizeof(double));
    w.E = w.c + align16((size_t)len * sizeof(double));
    w.part = w.E + align16(2 * (size_t)w.nb * sizeof(double));
    w.hist = w.part + align16(4 * (size_t)w.np * sizeof(double));
    w.S = w.hist + align16(HIST_BINS * sizeof(int));
    w.fft = w.S + align16(S_COUNT * sizeof(double));
    w.bytes = w.fft + 3 * (size_t)w.M * sizeof(double2);
    return w;
}
bool dist_ok(int64_t len, int64_t r) { return len >= 1 && r >= 0 && len + (r > 0 ? r - 1 : 0) <= DIST_FFT_MAX; }

bool is_finite(double v) { return std::isfinite(v); }
int blocks256(int64_t count) { return (int)((count + 255) / 256); }

template <typename T>
void distort_launch(const float* x, const float* noise, const float* h, const double* packet, int64_t len, const use_distort_params& p,
                    T* out_y, T* out_c, int64_t stride, double* scal, unsigned char* keep, int64_t keep_stride, char* work, hipStream_t st) {
    const int r = p.reverb ? p.rir_len : 0;
    const DistWork w = dist_layout(len, r);
    double* y = reinterpret_cast<double*>(work + w.y);
    double* c = reinterpret_cast<double*>(work + w.c);
    double* E = reinterpret_cast<double*>(work + w.E);
    double* part = reinterpret_cast<double*>(work + w.part);
    int* hist = reinterpret_cast<int*>(work + w.hist);
    double* S = reinterpret_cast<double*>(work + w.S);
    const dim3 block(256), slices(w.np), one(1), eblocks((w.nb + VAD_BLOCKS - 1) / VAD_BLOCKS);
    // 1. reverb
    hipLaunchKernelGGL(load_kernel, dim3(blocks256(len)), block, 0, st, x, r ? h : (const float*)nullptr, r, len, y, c);
    if (r) {
        double2* b0 = reinterpret_cast<double2*>(work + w.fft);
        double2 *b1 = b0 + w.M, *b2 = b1 + w.M;
        const int m = ceil_log2(w.M);
        hipLaunchKernelGGL(pack_kernel, dim3(blocks256(w.M)), block, 0, st, x, len, h, r, b0, b2, w.M);
        double2* X = fft_launch(b0, b1, m, -1, st);
        double2* spare = X == b0 ? b1 : b0;
        double2* H = fft_launch(b2, spare, m, -1, st);
        spare = H == b2 ? spare : b2;
        hipLaunchKernelGGL(product_kernel, dim3(blocks256(w.M)), block, 0, st, X, (const double2*)H, w.M);
        double2* R = fft_launch(X, spare, m, +1, st);
        hipLaunchKernelGGL(unpack_kernel, dim3(blocks256(len)), block, 0, st, (const double2*)R, 1.0 / (double)w.M, len, y);
    }
    // 2. the masked powers of the (reverberated) clean signal and of the noise
    const float* nz = p.add_noise ? noise : (const float*)nullptr;
    if (nz) {
        hipLaunchKernelGGL(block_energy_kernel<double>, eblocks, block, 0, st, (const double*)y, len, w.nb, E);
        hipLaunchKernelGGL(block_energy_kernel<float>, eblocks, block, 0, st, nz, len, w.nb, E + w.nb);
        hipLaunchKernelGGL(vad_final_kernel, dim3(2), block, 0, st, (const double*)E, (int64_t)w.nb, len, w.nb, S, keep, keep_stride);
    }
    // 2 + 3, then 4
    Loud loud; loud.n = p.n_loud;
    for (int i = 0; i < 5; ++i) loud.f[i] = p.loud[i];
    hipLaunchKernelGGL(mix_kernel, slices, block, 0, st, y, len, nz, p.snr_lin, loud, (const double*)S, part, w.np, scal);
    hipLaunchKernelGGL(stat_final_kernel, one, block, 0, st, (const double*)part, w.np, S, hist);
    if (p.clip_kind == USE_CLIP_HARD_ON_RATE) {
        hipLaunchKernelGGL(hist_kernel, slices, block, 0, st, (const double*)y, len, (const double*)S, hist);
        hipLaunchKernelGGL(threshold_kernel, one, dim3(64), 0, st, (const int*)hist, len, p.clip_a, S);
    }
    const int sigmoid = p.clip_kind == USE_CLIP_SIGMOID1 || p.clip_kind == USE_CLIP_SIGMOID2;
    hipLaunchKernelGGL(clip_kernel, slices, block, 0, st, y, len, p.clip_kind, p.clip_a, p.clip_b, (const double*)S, part, scal);
    hipLaunchKernelGGL(sum_final_kernel, one, block, 0, st, (const double*)part, w.np, S, (int)S_SUMSQ2);
    // 5 + 6
    hipLaunchKernelGGL(post_kernel, slices, block, 0, st, y, (const double*)c, len, sigmoid, p.dc, p.dc_offset,
                       p.packet_frame > 0 ? packet + p.packet_off : (const double*)nullptr, p.packet_frame, (const double*)S, part, w.np, scal);
    // 7
    if (p.volume == USE_VOLUME_RMS) {
        hipLaunchKernelGGL(block_energy_kernel<double>, eblocks, block, 0, st, (const double*)y, len, w.nb, E);
        hipLaunchKernelGGL(block_energy_kernel<double>, eblocks, block, 0, st, (const double*)c, len, w.nb, E + w.nb);
        hipLaunchKernelGGL(vad_final_kernel, dim3(2), block, 0, st, (const double*)E, (int64_t)w.nb, len, w.nb, S, (unsigned char*)nullptr, (int64_t)0);
    }
    hipLaunchKernelGGL(volume_final_kernel, one, block, 0, st, (const double*)part, w.np, p.volume, p.volume_target, p.normalize, S, scal);
    hipLaunchKernelGGL(store_kernel<T>, dim3((unsigned)((stride + DIST_SLICE - 1) / DIST_SLICE), 2), block, 0, st, (const double*)y, (const double*)c,
                       len, p.volume != USE_VOLUME_NONE, p.normalize, (const double*)S, out_y, out_c, stride);
}

}  // namespace

}  // namespace use

using namespace use;

size_t use_distort_workspace(int64_t len, int64_t rir_len) {
    if (!dist_ok(len, rir_len)) return 0;
    return dist_layout(len, rir_len).bytes;
}

int use_distort(const float* clean, const float* noise, const float* rir, const double* packet, int64_t packet_count, const int* len_host,
                const int* noise_len_host, const use_distort_params* params, int B, int64_t stride, int64_t noise_stride,
                int64_t rir_stride, int out_fp64, void* perturbed, void* clean_out, double* scalars_dev, unsigned char* keep_dev,
                int64_t keep_stride, void* work, size_t work_bytes, use_stream_t s) {
    if (B < 1 || B > 65535) return failf(USE_E_INVALID, "use_distort: B=%d must lie in 1 ... 65535", B);
    if (!clean) return failf(USE_E_INVALID, "use_distort: clean is null");
    if (!len_host) return failf(USE_E_INVALID, "use_distort: len_host is null");
    if (!params) return failf(USE_E_INVALID, "use_distort: params is null");
    if (!perturbed) return failf(USE_E_INVALID, "use_distort: perturbed is null");
    if (!clean_out) return failf(USE_E_INVALID, "use_distort: clean_out is null");
    if (!scalars_dev) return failf(USE_E_INVALID, "use_distort: scalars_dev is null");
    if (!work) return failf(USE_E_INVALID, "use_distort: work is null");
    if ((uintptr_t)work & 15) return failf(USE_E_INVALID, "use_distort: work must be 16-byte aligned");
    if (out_fp64 != 0 && out_fp64 != 1) return failf(USE_E_INVALID, "use_distort: out_fp64=%d must be 0 or 1", out_fp64);
    const uintptr_t omask = out_fp64 ? 7 : 3;
    if (((uintptr_t)perturbed | (uintptr_t)clean_out) & omask) return failf(USE_E_INVALID, "use_distort: perturbed and clean_out must be %d-byte aligned", (int)omask + 1);
    if (((uintptr_t)clean | (uintptr_t)noise | (uintptr_t)rir) & 3) return failf(USE_E_INVALID, "use_distort: clean, noise and rir must be 4-byte aligned");
    if (((uintptr_t)scalars_dev | (uintptr_t)packet) & 7) return failf(USE_E_INVALID, "use_distort: scalars_dev and packet must be 8-byte aligned");
    if (stride < 1 || (stride + DIST_SLICE - 1) / DIST_SLICE > 0x7fffffff)
        return failf(USE_E_INVALID, "use_distort: stride=%lld must be positive (and below 2^43)", (long long)stride);
    for (int b = 0; b < B; ++b) {
        const use_distort_params& p = params[b];
        const int64_t len = len_host[b];
        if (len < 1 || len > stride)
            return failf(USE_E_INVALID, "use_distort: len[%d]=%lld must lie in 1 ... stride=%lld", b, (long long)len, (long long)stride);
        if (len > DIST_FFT_MAX) return failf(USE_E_INVALID, "use_distort: len[%d]=%lld exceeds 2^24", b, (long long)len);
        if (p.reverb) {
            if (!rir) return failf(USE_E_INVALID, "use_distort: params[%d].reverb is set and rir is null", b);
            if (p.rir_len < 1 || p.rir_len > rir_stride)
                return failf(USE_E_INVALID, "use_distort: params[%d].rir_len=%d must lie in 1 ... rir_stride=%lld", b, p.rir_len, (long long)rir_stride);
            if (len + p.rir_len - 1 > DIST_FFT_MAX)
                return failf(USE_E_INVALID, "use_distort: len[%d] + params[%d].rir_len - 1 = %lld exceeds the FFT's limit 2^24", b, b, (long long)(len + p.rir_len - 1));
        }
        if (p.add_noise) {
            if (!noise) return failf(USE_E_INVALID, "use_distort: params[%d].add_noise is set and noise is null", b);
            if (!noise_len_host) return failf(USE_E_INVALID, "use_distort: params[%d].add_noise is set and noise_len_host is null", b);
            if (noise_len_host[b] < len || noise_len_host[b] > noise_stride)
                return failf(USE_E_INVALID, "use_distort: noise_len[%d]=%d must lie in len[%d]=%lld ... noise_stride=%lld: the noise row is shorter than the item",
                             b, noise_len_host[b], b, (long long)len, (long long)noise_stride);
            if (!is_finite(p.snr_lin) || !(p.snr_lin > 0.0)) return failf(USE_E_INVALID, "use_distort: params[%d].snr_lin=%g must be finite and positive", b, p.snr_lin);
        }
        if (p.n_loud < 0 || p.n_loud > 5) return failf(USE_E_INVALID, "use_distort: params[%d].n_loud=%d must lie in 0 ... 5", b, p.n_loud);
        for (int i = 0; i < p.n_loud; ++i)
            if (!is_finite(p.loud[i])) return failf(USE_E_INVALID, "use_distort: params[%d].loud[%d] is not finite", b, i);
        if (p.clip_kind == USE_CLIP_SOX || p.clip_kind == USE_CLIP_PEDAL)
            return failf(USE_E_INVALID, "use_distort: params[%d].clip_kind=%d (%s) is not built", b, p.clip_kind, p.clip_kind == USE_CLIP_SOX ? "sox" : "pedal");
        if (p.clip_kind < USE_CLIP_NONE || p.clip_kind > USE_CLIP_PEDAL) return failf(USE_E_INVALID, "use_distort: params[%d].clip_kind=%d is unknown", b, p.clip_kind);
        if (p.clip_kind != USE_CLIP_NONE) {
            if (!is_finite(p.clip_a) || !is_finite(p.clip_b)) return failf(USE_E_INVALID, "use_distort: params[%d].clip_a / clip_b is not finite", b);
            if (p.clip_kind == USE_CLIP_HARD_ON_RATE && !(p.clip_a > 0.0 && p.clip_a <= 1.0))
                return failf(USE_E_INVALID, "use_distort: params[%d].clip_a=%g: the rate must lie in (0, 1]", b, p.clip_a);
            if (p.clip_kind == USE_CLIP_SOFT && !(p.clip_a > 0.0)) return failf(USE_E_INVALID, "use_distort: params[%d].clip_a=%g: the slope must be positive", b, p.clip_a);
        }
        if (p.dc && !is_finite(p.dc_offset)) return failf(USE_E_INVALID, "use_distort: params[%d].dc_offset is not finite", b);
        if (p.packet_frame < 0) return failf(USE_E_INVALID, "use_distort: params[%d].packet_frame=%d: frame_size must be at least 1 (0: the stage is off)", b, p.packet_frame);
        if (p.packet_frame > 0) {
            if (!packet) return failf(USE_E_INVALID, "use_distort: params[%d].packet_frame is set and packet is null", b);
            const int64_t frames = (len + p.packet_frame - 1) / p.packet_frame;
            if (p.packet_off < 0 || p.packet_off + frames > packet_count)
                return failf(USE_E_INVALID, "use_distort: params[%d].packet_off=%lld + %lld frames must lie inside packet_count=%lld", b, p.packet_off,
                             (long long)frames, (long long)packet_count);
        }
        if (p.volume < USE_VOLUME_NONE || p.volume > USE_VOLUME_RMS) return failf(USE_E_INVALID, "use_distort: params[%d].volume=%d is unknown", b, p.volume);
        if (p.volume != USE_VOLUME_NONE && (!is_finite(p.volume_target) || !(p.volume_target > 0.0)))
            return failf(USE_E_INVALID, "use_distort: params[%d].volume_target=%g must be finite and positive", b, p.volume_target);
        if (keep_dev && keep_stride < 1 + len / VAD_HOP)
            return failf(USE_E_INVALID, "use_distort: keep_stride=%lld is smaller than 1 + len[%d] / 512 = %lld", (long long)keep_stride, b, (long long)(1 + len / VAD_HOP));
        const size_t need = dist_layout(len, p.reverb ? p.rir_len : 0).bytes;
        if (work_bytes < need)
            return failf(USE_E_INVALID, "use_distort: work_bytes=%zu is smaller than use_distort_workspace(%lld, %d) = %zu (item %d)", work_bytes,
                         (long long)len, p.reverb ? p.rir_len : 0, need, b);
    }
    hipStream_t st = (hipStream_t)s;
    char* base = static_cast<char*>(work);
    for (int b = 0; b < B; ++b) {
        const float* x = clean + (int64_t)b * stride;
        const float* nz = noise ? noise + (int64_t)b * noise_stride : nullptr;
        const float* h = rir ? rir + (int64_t)b * rir_stride : nullptr;
        double* scal = scalars_dev + (int64_t)b * USE_DISTORT_SCALARS;
        unsigned char* keep = keep_dev ? keep_dev + (int64_t)b * 2 * keep_stride : nullptr;
        if (out_fp64)
            distort_launch(x, nz, h, packet, (int64_t)len_host[b], params[b], static_cast<double*>(perturbed) + (int64_t)b * stride,
                           static_cast<double*>(clean_out) + (int64_t)b * stride, stride, scal, keep, keep_stride, base, st);
        else
            distort_launch(x, nz, h, packet, (int64_t)len_host[b], params[b], static_cast<float*>(perturbed) + (int64_t)b * stride,
                           static_cast<float*>(clean_out) + (int64_t)b * stride, stride, scal, keep, keep_stride, base, st);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(USE_E_HIP, "use_distort: launch failed: %s", hipGetErrorString(e));
    return USE_OK;
}
