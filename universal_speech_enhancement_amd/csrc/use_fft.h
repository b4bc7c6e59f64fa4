// The fp64 FFT of the waveform-side kernels (use_resample.hip, use_distort.hip): Stockham autosort passes of radix R = 2^r <= 512, out of
// place between two buffers, so that no bit-reversal pass exists.  A workgroup owns C = 2048 / R neighbouring columns j: it reads the
// R x C tile x[j + r * M / R] (runs of C contiguous points), applies the pass twiddle W_{Ns R}^{r (j mod Ns)} (Ns = the product of the
// radices before), transforms the C columns in LDS by radix-2 stages over a table of W_R^t (2048 points = 32 KiB, the table at most
// 16 KiB), and writes y[(j / Ns) Ns R + (j mod Ns) + r Ns].  M <= 2^11: one pass, one workgroup.  M <= 2^18: two passes.  M <= 2^27:
// three (fft_plan: the radices as equal as possible).  Every twiddle is sincospi of an exactly reduced argument; none comes from a
// recurrence.  The bodies are __host__ __device__ functions of the thread index (one per phase between two barriers).
// Everything lives in an unnamed namespace: each translation unit that includes this header gets its own copy of the kernel.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace use {

namespace {

#define USE_HD __host__ __device__ __forceinline__

constexpr int FFT_THREADS = 256;
constexpr int FFT_LDS_LOG2 = 11, FFT_LDS = 1 << FFT_LDS_LOG2;   // points a workgroup transforms in LDS
constexpr int FFT_RADIX_LOG2 = 9;                               // largest radix of a pass of a transform longer than FFT_LDS
constexpr int FFT_MAX_LOG2 = 26;                                // longest transform (M)

USE_HD double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// exp(sign * i * pi * t), t >= 0
USE_HD double2 expipi(double t, int sign) {
    double s, c;
#ifdef __HIP_DEVICE_COMPILE__
    sincospi(t, &s, &c);
#else
    s = sin(M_PI * t); c = cos(M_PI * t);
#endif
    return make_double2(c, sign < 0 ? -s : s);
}

// ---- one Stockham pass ----
struct FftPass { int log2N, log2R, log2Ns, log2C, sign; };

USE_HD int bitrev(int r, int bits) {
    int o = 0;
    for (int i = 0; i < bits; ++i) o |= ((r >> i) & 1) << (bits - 1 - i);
    return o;
}

// W_R^t, t < R / 2
USE_HD void fft_table_phase(int tid, double2* w, const FftPass g) {
    for (int t = tid; t < (1 << g.log2R) / 2; t += FFT_THREADS) w[t] = expipi(ldexp((double)t, 1 - g.log2R), g.sign);
}

USE_HD void fft_load_phase(int tid, const double2* in, double2* a, const FftPass g, int64_t blk) {
    const int C = 1 << g.log2C, E = 1 << (g.log2R + g.log2C);
    const int64_t stride = (int64_t)1 << (g.log2N - g.log2R), j0 = blk << g.log2C;
    for (int e = tid; e < E; e += FFT_THREADS) {
        const int c = e & (C - 1), r = e >> g.log2C;
        const int64_t j = j0 + c;
        double2 v = in[j + r * stride];
        if (g.log2Ns > 0) {                                       // r * k < Ns * R <= 2^26: exact in a double, and so is the scaling
            const int64_t k = j & (((int64_t)1 << g.log2Ns) - 1);
            v = cmul(v, expipi(ldexp((double)(r * k), 1 - g.log2Ns - g.log2R), g.sign));
        }
        a[(bitrev(r, g.log2R) << g.log2C) + c] = v;
    }
}

// stage ls (1 ... log2R) of the decimation-in-time butterflies over the C columns
USE_HD void fft_stage_phase(int tid, double2* a, const double2* w, const FftPass g, int ls) {
    const int C = 1 << g.log2C, E2 = 1 << (g.log2R + g.log2C - 1), half = 1 << (ls - 1);
    for (int t = tid; t < E2; t += FFT_THREADS) {
        const int c = t & (C - 1), b = t >> g.log2C, pos = b & (half - 1);
        const int i = (((b >> (ls - 1)) << ls) + pos) << g.log2C, i2 = i + (half << g.log2C);
        const double2 u = a[i + c], v = cmul(a[i2 + c], w[pos << (g.log2R - ls)]);
        a[i + c] = make_double2(u.x + v.x, u.y + v.y);
        a[i2 + c] = make_double2(u.x - v.x, u.y - v.y);
    }
}

USE_HD void fft_store_phase(int tid, const double2* a, double2* out, const FftPass g, int64_t blk) {
    const int C = 1 << g.log2C, R = 1 << g.log2R, E = 1 << (g.log2R + g.log2C);
    const int64_t j0 = blk << g.log2C, maskNs = ((int64_t)1 << g.log2Ns) - 1;
    for (int e = tid; e < E; e += FFT_THREADS) {
        int c, r;
        if (g.log2Ns == 0) { r = e & (R - 1); c = e >> g.log2R; }  // first pass: the tile's outputs j R + r are one contiguous run
        else { c = e & (C - 1); r = e >> g.log2C; }
        const int64_t j = j0 + c;
        out[((j >> g.log2Ns) << (g.log2Ns + g.log2R)) + (j & maskNs) + ((int64_t)r << g.log2Ns)] = a[(r << g.log2C) + c];
    }
}

__global__ __launch_bounds__(FFT_THREADS) void fft_pass_kernel(const double2* __restrict__ in, double2* __restrict__ out, const FftPass g) {
    __shared__ double2 a[FFT_LDS];
    __shared__ double2 w[FFT_LDS / 2];
    const int tid = threadIdx.x;
    fft_table_phase(tid, w, g);
    fft_load_phase(tid, in, a, g, blockIdx.x);
    __syncthreads();
    for (int ls = 1; ls <= g.log2R; ++ls) {
        fft_stage_phase(tid, a, w, g, ls);
        __syncthreads();
    }
    fft_store_phase(tid, a, out, g, blockIdx.x);
}

// the radices of the passes of a 2^m-point transform (m <= 27), first pass first; -> the number of passes (0 for m == 0)
int fft_plan(int m, int log2R[3]) {
    if (m <= 0) return 0;
    const int p = m <= FFT_LDS_LOG2 ? 1 : (m + FFT_RADIX_LOG2 - 1) / FFT_RADIX_LOG2;
    for (int i = 0; i < p; ++i) log2R[i] = m / p + (i < m % p ? 1 : 0);
    return p;
}

// the geometry of pass i: its tile is C = min(FFT_LDS / R, M / R) columns wide
FftPass fft_pass(int m, const int log2R[3], int i, int sign) {
    FftPass g;
    g.log2N = m; g.log2R = log2R[i]; g.sign = sign;
    g.log2Ns = 0;
    for (int q = 0; q < i; ++q) g.log2Ns += log2R[q];
    g.log2C = FFT_LDS_LOG2 - g.log2R < m - g.log2R ? FFT_LDS_LOG2 - g.log2R : m - g.log2R;
    return g;
}

// smallest power of two >= v, as its exponent
int ceil_log2(int64_t v) { int m = 0; while (((int64_t)1 << m) < v) ++m; return m; }

// a 2^m-point FFT from `cur`, ping-pong with `other`; -> the buffer that holds the result
double2* fft_launch(double2* cur, double2* other, int m, int sign, hipStream_t st) {
    int log2R[3];
    const int p = fft_plan(m, log2R);
    for (int i = 0; i < p; ++i) {
        const FftPass g = fft_pass(m, log2R, i, sign);
        hipLaunchKernelGGL(fft_pass_kernel, dim3(1u << (m - g.log2R - g.log2C)), dim3(FFT_THREADS), 0, st, cur, other, g);
        double2* t = cur; cur = other; other = t;
    }
    return cur;
}

}  // namespace

}  // namespace use
