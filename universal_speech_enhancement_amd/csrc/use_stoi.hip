// Short-time objective intelligibility on the device: STOI (Taal et al. 2011) and ESTOI (Jensen & Taal 2016) as pystoi.stoi(clean,
// processed, fs, extended) computes them - the third number of the reference's validation loop (sgmse/util/inference.py: evaluate_model)
// beside SI-SDR (use_metrics.hip) - per item of a batch est / clean [B][stride] with valid lengths len[b].  Everything after the float32
// load is fp64, every sum has a fixed order that depends on len[b] and the item's own data alone, and there are no atomics: an item gives
// the same bits in any batch, at any stride, in every run.
//
// The algorithm (FS 10000, frames of 256 at hop 128, w = np.hanning(258)[1:-1], NFFT 512, 15 third-octave bands from 150 Hz, segments of
// 30 frames, clip at -15 dB, 40 dB of dynamic range, EPS = 2^-52), and the launches that carry it out:
//   taps     (1)          the resampler of pystoi / scipy.signal.resample_poly(x, p, q, window = h / sum h), p / q = 10000 / fs: h =
//                         kaiser(2 L + 1, 0.1102 (60 - 8.7)) 2 p fc sinc(2 fc t), fc = 1 / (2 max(p, q)), L = ceil(52 / (2.8714 fc)), Kaiser's
//                         I0 by its power series until a term no longer changes the sum; h' = p h / sum h, stored phase-major
//                         (tap i at [i mod p][i / p]): one output walks ONE phase downwards, so the lanes of a wave read a handful of
//                         addresses per step instead of a stride of q doubles.
//   resample (nblk, B, 2) y[n] = sum_j x[j] h'[L + n q - j p], n < ceil(len p / q), zeros past both ends of x: one output per thread, j
//                         ascending; the taps and the input span of the block's 256 outputs are staged in LDS.  fs == 10000: a copy.
//   energy   (F, B)       E_k = 20 log10(|w clean_k|_2 + EPS) of frame k (start 128 k, k <= (n - 256) / 128): one workgroup per frame.
//   scan     (B)          max E, keep_k = (max E - 40 - E_k < 0), and the kept frames' indices in order (an integer prefix scan in LDS):
//                         kidx[b][0 .. K_b), K_b.  K is data-dependent and never leaves the device: the grids below are sized for no
//                         frame removed and every workgroup reads K.
//   stft     (F - 1, B)   frame t < K - 1 of the compacted signals.  pystoi rebuilds both signals by overlap-add of their windowed kept
//                         frames; here each of the frame's 256 samples is GATHERED as the sum of its at most two kept source frames
//                         (w x of frames kidx[t - 1], kidx[t] for the first half, kidx[t], kidx[t + 1] for the second), windowed again,
//                         zero-padded to 512 and transformed as in use_spec_loss.hip: z[j] = x[2j] + i x[2j+1], a 256-point radix-2
//                         transform in LDS, then the conjugate-symmetric split.  Both signals side by side with the same code (threads
//                         0-127 clean, 128-255 est), so est == clean gives identical bits.  |X|^2 of bins 7 .. 218 stays in LDS; 30
//                         threads fold the 15 contiguous bands in ascending bin order -> tob[b][signal][band][t] = sqrt(sum).
//   segment  (T - 29, B)  one workgroup per 15 x 30 block tob[:, m : m + 30] of both signals.  STOI, one thread per band row: c = |x| /
//                         (|y| + EPS), y' = min(c y, x (1 + 10^(15/20))), means removed, rows divided by (|.| + EPS), sum x y'.  ESTOI:
//                         rows (one thread each), then columns (one thread each): mean removed, scaled to unit norm; sum x_n y_n.
//                         pystoi's EPS randn dither is left out (bit-reproducible), and a row or column whose sum of squares is exactly
//                         0 is scaled by 0 - what the dither gives in expectation - not by 1 / 0: zeros in est cannot make a NaN.
//   final    (B)          partials summed in segment order; d = sum / (15 (T - 29)), sum / (30 (T - 29)); T = K - 1 < 30: 1e-5 for both
//                         (pystoi's return value).  out[b] = { stoi, estoi, T }.
// Seven launches (+ one per 64 items for the lengths), plain stores only: nothing to zero between calls, a captured graph replays as
// it is.  Samples of a row past len[b] are never read: the resampler treats x as zero there.
#include <cstdarg>
#include <cstdio>

#include "../../include/use_hip.h"
#include "use_kernels.h"

int use_set_error(int code, const char* msg);   // use_engine.cpp

namespace use {

namespace {

constexpr int ST_FS = 10000, ST_FRAME = 256, ST_HOP = 128, ST_BANDS = 15, ST_SEG = 30, ST_LO = 7, ST_HI = 219;
constexpr double ST_EPS = 2.220446049250313e-16, ST_DYN = 40.0, ST_SHORT = 1e-5;
constexpr double ST_CLIP = 1.0 + 5.623413251903491;           // 1 + 10^(15 / 20)
constexpr double ST_KAISER_BETA = 0.1102 * (60.0 - 8.7);
constexpr double ST_PI = 3.141592653589793;
constexpr int ST_TAPS_MAX = 1752;                             // 5 phases x 349 taps at 48 kHz (1741 taps), rounded up
constexpr int ST_SPAN_MAX = 1600;                             // inputs under 256 outputs: (255 q + 2 L) / p + 2 = 1574 at 48 kHz
__device__ const int ST_EDGE[ST_BANDS + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};   // thirdoct(10000, 512, 15, 150)

// fixed-order workgroup sum of 256 doubles; every thread gets the result
__device__ __forceinline__ double block_sum(double v, double* sh) {
    __syncthreads();                                          // sh may still be read from the previous sum
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    return sh[0];
}
__device__ __forceinline__ double hann_w(int i) { return 0.5 - 0.5 * cospi(2.0 * (double)(i + 1) / 257.0); }   // np.hanning(258)[1:-1]
__device__ __forceinline__ int resampled_len(int len, int p, int q) { return (int)(((int64_t)len * p + q - 1) / q); }
__device__ __forceinline__ int frame_count(int n) { return (n - ST_FRAME) / ST_HOP + 1; }                        // n >= 256

__device__ double bessel_i0(double x) {                       // sum ((x / 2)^k / k!)^2 until a term no longer changes the sum
    const double y = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= y / ((double)k * (double)k);
        const double next = sum + term;
        if (next == sum) break;
        sum = next;
    }
    return sum;
}

// tap i of 2 L + 1 at hp[(i % p) * M + i / p]
__global__ __launch_bounds__(256) void stoi_taps_kernel(double* __restrict__ hp, int p, int q, int L, int M) {
    __shared__ double sh[256];
    if (p == q) return;                                       // 10 kHz in: no filter
    const int mx = p > q ? p : q;
    const double fc = 1.0 / (2.0 * (double)mx), gain = 2.0 * (double)p * fc, i0b = bessel_i0(ST_KAISER_BETA);
    double acc = 0.0;
    for (int i = threadIdx.x; i <= 2 * L; i += 256) {
        const double t = (double)(i - L), r = t / (double)L;
        const double k = bessel_i0(ST_KAISER_BETA * sqrt(1.0 - r * r)) / i0b;
        const double y = (2.0 * fc) * t;
        const double h = k * (gain * (i == L ? 1.0 : sinpi(y) / (ST_PI * y)));
        hp[(i % p) * M + i / p] = h;
        acc += h;
    }
    const double sum = block_sum(acc, sh);
    for (int i = threadIdx.x; i <= 2 * L; i += 256) {         // each thread rescales the taps it wrote itself
        double* h = hp + (i % p) * M + i / p;
        *h = (*h / sum) * (double)p;
    }
}

__device__ __forceinline__ int64_t ceil_div(int64_t a, int64_t b) { return a >= 0 ? (a + b - 1) / b : -((-a) / b); }   // b > 0

__global__ __launch_bounds__(256) void stoi_resample_kernel(const float* __restrict__ est, const float* __restrict__ clean,
                                                            const int* __restrict__ lens, const double* __restrict__ hp,
                                                            double* __restrict__ xr, int64_t stride, int p, int q, int L, int M, int n_max) {
    __shared__ double sh_h[ST_TAPS_MAX];
    __shared__ float sh_x[ST_SPAN_MAX];
    const int b = blockIdx.y, sig = blockIdx.z, tid = threadIdx.x, len = lens[b];
    const int n_out = resampled_len(len, p, q);
    const int64_t n0 = (int64_t)blockIdx.x * 256;
    if (n0 >= n_out) return;                                  // a block of padding: its outputs are never read
    const float* row = (sig ? est : clean) + (size_t)b * (size_t)stride;
    double* o = xr + ((size_t)b * 2 + sig) * (size_t)n_max;
    const int64_t n = n0 + tid;
    if (p == q) {                                             // already at 10 kHz
        if (n < n_out) o[n] = (double)row[n];
        return;
    }
    for (int i = tid; i < p * M; i += 256) sh_h[i] = hp[i];
    const int64_t n1 = n0 + 255 < n_out ? n0 + 255 : n_out - 1;
    int64_t jlo = ceil_div(n0 * q - L, p), jhi = (n1 * q + L) / p;
    jlo = jlo < 0 ? 0 : jlo; jhi = jhi > len - 1 ? len - 1 : jhi;
    for (int64_t i = tid; i <= jhi - jlo && i < ST_SPAN_MAX; i += 256) sh_x[i] = row[jlo + i];
    __syncthreads();
    if (n > n1) return;
    const int64_t c = n * q;
    int64_t ja = ceil_div(c - L, p), jb = (c + L) / p;
    ja = ja < jlo ? jlo : ja; jb = jb > jhi ? jhi : jb;
    const int64_t i0 = L + c - ja * p;                        // the largest tap index of this output; its phase is the output's
    const double* h = sh_h + (int)(i0 % p) * M + (int)(i0 / p);
    const float* x = sh_x + (ja - jlo);
    double acc = 0.0;
    for (int t = 0; t <= (int)(jb - ja); ++t) acc = fma((double)x[t], h[-t], acc);
    o[n] = acc;
}

__global__ __launch_bounds__(256) void stoi_energy_kernel(const double* __restrict__ xr, const int* __restrict__ lens, double* __restrict__ E,
                                                          int p, int q, int n_max, int Fmax) {
    __shared__ double sh[256];
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (k >= frame_count(resampled_len(lens[b], p, q))) return;
    const double* x = xr + (size_t)b * 2 * (size_t)n_max;     // the clean signal decides
    const double v = hann_w(tid) * x[(size_t)k * ST_HOP + tid];
    const double s = block_sum(v * v, sh);
    if (tid == 0) E[(size_t)b * Fmax + k] = 20.0 * log10(sqrt(s) + ST_EPS);
}

__global__ __launch_bounds__(256) void stoi_scan_kernel(const double* __restrict__ E, const int* __restrict__ lens, int* __restrict__ kidx,
                                                        int* __restrict__ Kd, int p, int q, int Fmax) {
    __shared__ double shd[256];
    __shared__ int shi[256];
    const int b = blockIdx.x, tid = threadIdx.x, F = frame_count(resampled_len(lens[b], p, q));
    const double* e = E + (size_t)b * Fmax;
    int* out = kidx + (size_t)b * Fmax;
    double mx = -INFINITY;
    for (int k = tid; k < F; k += 256) mx = fmax(mx, e[k]);
    shd[tid] = mx;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) shd[tid] = fmax(shd[tid], shd[tid + w]);
        __syncthreads();
    }
    mx = shd[0];
    int base = 0;
    for (int k0 = 0; k0 < F; k0 += 256) {
        const int k = k0 + tid;
        const int keep = k < F && (mx - ST_DYN) - e[k] < 0.0 ? 1 : 0;
        __syncthreads();                                      // shi may still be read from the previous chunk
        shi[tid] = keep;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {                   // inclusive scan
            const int v = tid >= d ? shi[tid - d] : 0;
            __syncthreads();
            shi[tid] += v;
            __syncthreads();
        }
        if (keep) out[base + shi[tid] - 1] = k;
        base += shi[255];
    }
    if (tid == 0) Kd[b] = base;
}

// b' = a - w b, a' = a + w b
__device__ __forceinline__ void butterfly(double2& a, double2& b, double wr, double wi) {
    const double tr = fma(wr, b.x, -__dmul_rn(wi, b.y)), ti = fma(wr, b.y, __dmul_rn(wi, b.x));
    b = make_double2(__dsub_rn(a.x, tr), __dsub_rn(a.y, ti));
    a = make_double2(__dadd_rn(a.x, tr), __dadd_rn(a.y, ti));
}
// |X[k]|^2 of the real signal packed into Z: a = Z[k mod m], b = Z[(m - k) mod m], w = W_n^k
__device__ __forceinline__ double split_power(double2 a, double2 b, double wr, double wi) {
    const double er = 0.5 * (a.x + b.x), ei = 0.5 * (a.y - b.y);          // Xe = (a + conj b) / 2
    const double qr = 0.5 * (a.y + b.y), qi = -0.5 * (a.x - b.x);         // Xo = (a - conj b) / (2 i)
    const double xr = er + fma(wr, qr, -__dmul_rn(wi, qi)), xi = ei + fma(wr, qi, __dmul_rn(wi, qr));
    return fma(xi, xi, __dmul_rn(xr, xr));
}

__global__ __launch_bounds__(256) void stoi_stft_kernel(const double* __restrict__ xr, const int* __restrict__ kidx, const int* __restrict__ Kd,
                                                        double* __restrict__ tob, int n_max, int Fmax, int Tmax) {
    __shared__ double2 z[2][256], tab[257];                   // tab[k] = (cos, -sin)(2 pi k / 512)
    __shared__ double w[ST_FRAME], pw[2][ST_HI + 1];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (t >= Kd[b] - 1) return;                               // K kept frames give K - 1 STFT frames
    for (int k = tid; k <= 256; k += 256) {
        double sn, cs;
        sincospi(2.0 * (double)k / 512.0, &sn, &cs);
        tab[k] = make_double2(cs, -sn);
    }
    w[tid] = hann_w(tid);
    __syncthreads();
    const int sig = tid >> 7, j = tid & 127;
    {
        const int* ki = kidx + (size_t)b * Fmax;
        const size_t f0 = (size_t)ki[t] * ST_HOP, f1 = (size_t)ki[t + 1] * ST_HOP, fm = t > 0 ? (size_t)ki[t - 1] * ST_HOP : 0;
        const double* x = xr + ((size_t)b * 2 + sig) * (size_t)n_max;
        double v[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int n = 2 * j + h;                          // sample n of the compacted frame: its own frame and the neighbour over it
            double a = w[n] * x[f0 + n];
            if (n < ST_HOP) { if (t > 0) a += w[n + ST_HOP] * x[fm + n + ST_HOP]; }
            else a += w[n - ST_HOP] * x[f1 + n - ST_HOP];
            v[h] = w[n] * a;
        }
        z[sig][__brev((unsigned)j) >> 24] = make_double2(v[0], v[1]);
        z[sig][__brev((unsigned)(j + 128)) >> 24] = make_double2(0.0, 0.0);       // samples 256 .. 511: the zero padding
    }
    __syncthreads();
    for (int s = 0; s < 8; ++s) {                             // stage s: butterflies h = 2^s apart, twiddle W_{2h}^pos = tab[pos 512 / (2h)]
        const int h = 1 << s, pos = j & (h - 1), i = ((j - pos) << 1) + pos;
        const double2 tw = tab[pos << (8 - s)];
        double2 a = z[sig][i], c = z[sig][i + h];
        butterfly(a, c, tw.x, tw.y);
        z[sig][i] = a; z[sig][i + h] = c;
        __syncthreads();
    }
    for (int k = ST_LO + j; k < ST_HI; k += 128) pw[sig][k] = split_power(z[sig][k], z[sig][256 - k], tab[k].x, tab[k].y);
    __syncthreads();
    if (tid < 2 * ST_BANDS) {
        const int sg = tid / ST_BANDS, band = tid % ST_BANDS;
        double acc = 0.0;
        for (int k = ST_EDGE[band]; k < ST_EDGE[band + 1]; ++k) acc += pw[sg][k];
        tob[(((size_t)b * 2 + sg) * ST_BANDS + band) * (size_t)Tmax + t] = sqrt(acc);
    }
}

// v[0 .. n) at stride st: remove the mean, scale to unit norm (by 0 where the sum of squares is exactly 0)
__device__ __forceinline__ void unit_in_place(double* v, int n, int st) {
    double m = 0.0, ss = 0.0;
    for (int i = 0; i < n; ++i) m += v[i * st];
    m /= (double)n;
    for (int i = 0; i < n; ++i) { const double d = v[i * st] - m; v[i * st] = d; ss = fma(d, d, ss); }
    const double sc = ss > 0.0 ? 1.0 / sqrt(ss) : 0.0;
    for (int i = 0; i < n; ++i) v[i * st] *= sc;
}

__global__ __launch_bounds__(64) void stoi_segment_kernel(const double* __restrict__ tob, const int* __restrict__ Kd, double* __restrict__ part,
                                                          int Tmax, int Smax) {
    __shared__ double X[2][ST_BANDS][ST_SEG], Xn[2][ST_BANDS][ST_SEG];    // [0]: clean, [1]: est
    __shared__ double rowdot[ST_BANDS], coldot[ST_SEG];
    const int m = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, T = Kd[b] - 1;
    if (m > T - ST_SEG) return;
    for (int e = tid; e < 2 * ST_BANDS * ST_SEG; e += 64) {
        const int row = e / ST_SEG, t = e % ST_SEG;           // row = signal * 15 + band
        const double v = tob[((size_t)b * 2 * ST_BANDS + row) * (size_t)Tmax + m + t];
        (&X[0][0][0])[e] = v; (&Xn[0][0][0])[e] = v;
    }
    __syncthreads();
    if (tid < ST_BANDS) {                                     // STOI, band row tid
        const double* x = X[0][tid];
        const double* y = X[1][tid];
        double sx = 0.0, sy = 0.0;
        for (int t = 0; t < ST_SEG; ++t) { sx = fma(x[t], x[t], sx); sy = fma(y[t], y[t], sy); }
        const double c = sqrt(sx) / (sqrt(sy) + ST_EPS);
        double yp[ST_SEG], mx = 0.0, my = 0.0;
#pragma unroll
        for (int t = 0; t < ST_SEG; ++t) { yp[t] = fmin(c * y[t], x[t] * ST_CLIP); mx += x[t]; my += yp[t]; }
        mx /= (double)ST_SEG; my /= (double)ST_SEG;
        sx = 0.0; sy = 0.0;
#pragma unroll
        for (int t = 0; t < ST_SEG; ++t) { const double dx = x[t] - mx; yp[t] -= my; sx = fma(dx, dx, sx); sy = fma(yp[t], yp[t], sy); }
        const double nx = sqrt(sx) + ST_EPS, ny = sqrt(sy) + ST_EPS;
        double d = 0.0;
#pragma unroll
        for (int t = 0; t < ST_SEG; ++t) d = fma((x[t] - mx) / nx, yp[t] / ny, d);
        rowdot[tid] = d;
    } else if (tid >= 32 && tid < 32 + 2 * ST_BANDS) {        // ESTOI, rows of either signal
        unit_in_place(&Xn[0][0][0] + (tid - 32) * ST_SEG, ST_SEG, 1);
    }
    __syncthreads();
    if (tid < ST_SEG) {                                       // ESTOI, column tid of both signals
        unit_in_place(&Xn[0][0][tid], ST_BANDS, ST_SEG);
        unit_in_place(&Xn[1][0][tid], ST_BANDS, ST_SEG);
        double d = 0.0;
        for (int r = 0; r < ST_BANDS; ++r) d = fma(Xn[0][r][tid], Xn[1][r][tid], d);
        coldot[tid] = d;
    }
    __syncthreads();
    if (tid == 0) {
        double d = 0.0, e = 0.0;
        for (int r = 0; r < ST_BANDS; ++r) d += rowdot[r];
        for (int t = 0; t < ST_SEG; ++t) e += coldot[t];
        double* o = part + ((size_t)b * Smax + m) * 2;
        o[0] = d; o[1] = e;
    }
}

__global__ __launch_bounds__(256) void stoi_final_kernel(const double* __restrict__ part, const int* __restrict__ Kd, double* __restrict__ out,
                                                         int Smax) {
    __shared__ double sh[256];
    const int b = blockIdx.x, K = Kd[b], T = K > 0 ? K - 1 : 0, S = T - ST_SEG + 1;
    double d = 0.0, e = 0.0;
    const double* p = part + (size_t)b * Smax * 2;
    for (int m = threadIdx.x; m < S; m += 256) { d += p[(size_t)m * 2]; e += p[(size_t)m * 2 + 1]; }
    d = block_sum(d, sh); e = block_sum(e, sh);
    if (threadIdx.x == 0) {
        double* o = out + (size_t)b * USE_STOI_COUNT;
        o[USE_STOI_STOI] = S >= 1 ? d / ((double)S * (double)ST_BANDS) : ST_SHORT;
        o[USE_STOI_ESTOI] = S >= 1 ? e / ((double)ST_SEG * (double)S) : ST_SHORT;
        o[USE_STOI_FRAMES] = (double)T;
    }
}

int failf(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    return use_set_error(code, buf);
}

// the resampler of a rate and the byte offsets of the workspace behind the int lens[B]
struct StoiWork {
    int p, q, L, M;                                           // p / q = 10000 / rate; 2 L + 1 taps in p phases of M
    int n_max, Fmax, Tmax, Smax;                              // of a full row: resampled samples, frames, STFT frames, segments
    size_t K, taps, xr, E, kidx, tob, part, bytes;
};
bool stoi_shape_ok(int B, int64_t stride, int sr) {
    return B >= 1 && B <= 65535 && stride >= 1 && (sr == 10000 || sr == 16000 || sr == 24000 || sr == 48000);
}
int64_t resampled(int64_t n, int p, int q) { return (n * p + q - 1) / q; }
StoiWork stoi_layout(int B, int64_t stride, int sr) {
    StoiWork w;
    int a = ST_FS, c = sr;
    while (c) { const int r = a % c; a = c; c = r; }          // a = gcd
    w.p = ST_FS / a; w.q = sr / a;
    const int mx = w.p > w.q ? w.p : w.q;
    // ceil(52 / (28.714 fc / 10)), fc = 1 / (2 mx): 435 at 24 kHz, 290 at 16 kHz, 870 at 48 kHz
    const double l = 52.0 / (28.714 * (1.0 / (2.0 * (double)mx)) / 10.0);
    w.L = w.p == w.q ? 0 : (int)l + ((double)(int)l < l ? 1 : 0);
    w.M = (2 * w.L + 1 + w.p - 1) / w.p;
    const int64_t width = stride < 0x7fffffff ? stride : 0x7fffffff;      // a length is an int
    w.n_max = (int)resampled(width, w.p, w.q);
    w.Fmax = w.n_max >= ST_FRAME ? (w.n_max - ST_FRAME) / ST_HOP + 1 : 1;
    w.Tmax = w.Fmax > 1 ? w.Fmax - 1 : 1;
    w.Smax = w.Tmax >= ST_SEG ? w.Tmax - ST_SEG + 1 : 1;
    auto up8 = [](size_t v) { return (v + 7) & ~(size_t)7; };
    size_t off = up8((size_t)B * sizeof(int));
    w.K = off; off += up8((size_t)B * sizeof(int));
    w.taps = off; off += (size_t)ST_TAPS_MAX * sizeof(double);
    w.xr = off; off += (size_t)B * 2 * (size_t)w.n_max * sizeof(double);
    w.E = off; off += (size_t)B * w.Fmax * sizeof(double);
    w.kidx = off; off += up8((size_t)B * w.Fmax * sizeof(int));
    w.tob = off; off += (size_t)B * 2 * ST_BANDS * (size_t)w.Tmax * sizeof(double);
    w.part = off; off += (size_t)B * w.Smax * 2 * sizeof(double);
    w.bytes = off;
    return w;
}

}  // namespace

}  // namespace use

using namespace use;

size_t use_stoi_workspace(int B, int64_t stride, int sampling_rate) {
    if (!stoi_shape_ok(B, stride, sampling_rate)) return 0;
    return stoi_layout(B, stride, sampling_rate).bytes;
}

int use_stoi(const float* est, const float* clean, const int* len_host, int B, int64_t stride, int sampling_rate, void* work,
             size_t work_bytes, double* out_dev, use_stream_t s) {
    if (sampling_rate != 10000 && sampling_rate != 16000 && sampling_rate != 24000 && sampling_rate != 48000)
        return failf(USE_E_INVALID, "use_stoi: sampling_rate=%d is none of 10000, 16000, 24000, 48000", sampling_rate);
    if (B < 1 || B > 65535) return failf(USE_E_INVALID, "use_stoi: B=%d must lie in 1 ... 65535", B);
    if (stride < 1) return failf(USE_E_INVALID, "use_stoi: stride=%lld must be positive", (long long)stride);
    if (!est) return failf(USE_E_INVALID, "use_stoi: est is null");
    if (!clean) return failf(USE_E_INVALID, "use_stoi: clean is null");
    if (!len_host) return failf(USE_E_INVALID, "use_stoi: len_host is null");
    if (!work) return failf(USE_E_INVALID, "use_stoi: work is null");
    if (!out_dev) return failf(USE_E_INVALID, "use_stoi: out_dev is null");
    const StoiWork w = stoi_layout(B, stride, sampling_rate);
    int max_len = 0;
    for (int b = 0; b < B; ++b) {
        if (len_host[b] < 1 || len_host[b] > stride || resampled(len_host[b], w.p, w.q) < ST_FRAME)
            return failf(USE_E_INVALID, "use_stoi: len[%d]=%d must lie in %lld ... stride = %lld (one frame of 256 samples at 10 kHz)", b, len_host[b],
                         ((long long)(ST_FRAME - 1) * w.q) / w.p + 1, (long long)stride);
        max_len = len_host[b] > max_len ? len_host[b] : max_len;
    }
    if (work_bytes < w.bytes)
        return failf(USE_E_INVALID, "use_stoi: work_bytes=%zu is smaller than use_stoi_workspace(%d, %lld, %d) = %zu", work_bytes, B,
                     (long long)stride, sampling_rate, w.bytes);
    if ((uintptr_t)work & 7) return failf(USE_E_INVALID, "use_stoi: work must be 8-byte aligned");

    hipStream_t st = (hipStream_t)s;
    char* base = static_cast<char*>(work);
    int* lens = reinterpret_cast<int*>(base);
    int* K = reinterpret_cast<int*>(base + w.K);
    double* taps = reinterpret_cast<double*>(base + w.taps);
    double* xr = reinterpret_cast<double*>(base + w.xr);
    double* E = reinterpret_cast<double*>(base + w.E);
    int* kidx = reinterpret_cast<int*>(base + w.kidx);
    double* tob = reinterpret_cast<double*>(base + w.tob);
    double* part = reinterpret_cast<double*>(base + w.part);
    // grids for the longest item with no frame removed; shorter items and removed frames return at once
    const int n_top = (int)resampled(max_len, w.p, w.q), F = (n_top - ST_FRAME) / ST_HOP + 1;
    const int T = F > 1 ? F - 1 : 1, S = T >= ST_SEG ? T - ST_SEG + 1 : 1;
    launch_item_lengths(lens, len_host, B, st);               // as use_metrics: kernel arguments, no copy, no synchronisation
    hipLaunchKernelGGL(stoi_taps_kernel, dim3(1), dim3(256), 0, st, taps, w.p, w.q, w.L, w.M);
    hipLaunchKernelGGL(stoi_resample_kernel, dim3((n_top + 255) / 256, B, 2), dim3(256), 0, st, est, clean, lens, taps, xr, stride, w.p, w.q, w.L,
                       w.M, w.n_max);
    hipLaunchKernelGGL(stoi_energy_kernel, dim3(F, B), dim3(256), 0, st, xr, lens, E, w.p, w.q, w.n_max, w.Fmax);
    hipLaunchKernelGGL(stoi_scan_kernel, dim3(B), dim3(256), 0, st, E, lens, kidx, K, w.p, w.q, w.Fmax);
    hipLaunchKernelGGL(stoi_stft_kernel, dim3(T, B), dim3(256), 0, st, xr, kidx, K, tob, w.n_max, w.Fmax, w.Tmax);
    hipLaunchKernelGGL(stoi_segment_kernel, dim3(S, B), dim3(64), 0, st, tob, K, part, w.Tmax, w.Smax);
    hipLaunchKernelGGL(stoi_final_kernel, dim3(B), dim3(256), 0, st, part, K, out_dev, w.Smax);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(USE_E_HIP, "use_stoi: launch failed: %s", hipGetErrorString(e));
    return USE_OK;
}
