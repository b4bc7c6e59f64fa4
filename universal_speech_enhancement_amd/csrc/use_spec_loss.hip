// Convergence losses on the device (reference loss_function/monaural_loss.py:59-178, WavSpecConvergence_Loss - the same arithmetic
// sits in WavSpecConvergence_HIFIGAN_Vocoder_G_Loss, the generator criterion of LSGAN.yaml): a waveform L1, three magnitude distances
// at four STFT resolutions and two mel distances, forward only, per item of a batch est / clean [B][stride] with valid lengths len[b].
// Everything is fp64 - float32 samples in, then window, transform, magnitude, log, products and sums in double - and every sum has a
// fixed order that depends on len[b] alone: an item gives the same bits in any batch, at any stride, in every run (no atomics).
//
// Five magnitude maps per item: r = 0..3 the Spectrograms (n = n0 2^r, n0 = 256 at 24 kHz / 512 at 48 kHz; periodic Hann of n, hop n / 4)
// and the MelSpectrogram's (n = 2048; periodic Hann of 0.025 sr centred in the frame, hop 0.010 sr), all centred with reflect padding:
// n / 2 + 1 bins x (1 + len / hop) frames.
//   tables  (1 launch)   (cos, -sin)(2 pi k / Nt), k <= Nt / 2, Nt the largest n, from sincospi; the 130 HTK band edges f_pts
//   wav     (nblk, B)    sum |e - c| of one 8192-sample slice -> 1 partial
//   frame   (T, B) x 5   one workgroup per (item, map, frame).  The two windowed frames are transformed by the SAME code side by side,
//                        each as a real FFT: z[j] = x[2j] + i x[2j+1], an n/2-point radix-2 transform in LDS (bit-reversed load,
//                        in-place decimation in time, one twiddle load per butterfly pair), then X[k] = Xe[k] + W_n^k Xo[k] from the
//                        conjugate-symmetric split of Z.  est and clean do not share one complex transform: with est == clean that
//                        would leave |E| and |C| a rounding apart, and identical inputs must give exactly 0 in every term.
//                        STFT maps: sum over bins of (Me - Mc)^2, Mc^2, |log(32768 Me + 1e-6) - log(32768 Mc + 1e-6)| -> 3 partials.
//                        Mel map: the 1025 magnitudes of either signal stay in LDS, thread (signal, band j) folds the band's
//                        contiguous support with the triangle evaluated in place from f_pts, then the two sums over 128 bands.
//                        Frames t >= 1 + len[b] / hop return at once, their partials are never read, and no sample past len[b] is.
//   final   (B)          partials summed in frame order -> the 15 values.
// Partials are plain stores: nothing to zero between calls, a captured graph replays as it is.
//
// LDS: two n/2-point complex fp64 arrays = 16 n bytes (64 KB at n = 4096) + 6 KB of reduction scratch, above the default dynamic limit:
// raised per device through LdsAttrOnce.  A butterfly's two operands are 16-byte elements h apart and consecutive lanes take
// consecutive butterflies: in the stages h <= 8 (four of up to eleven) the elements a lane group of a 16-byte read touches are spread
// over 512 bytes, two to a bank (2x); from h = 16 on runs of 16 lanes read 256 contiguous bytes, which the lane groups of a 16-byte
// read serve without conflict, as they do the split pass (z[k] ascending, z[m - k] descending).
#include <cstdarg>
#include <cstdio>

#include "../../include/use_hip.h"
#include "use_kernels.h"

int use_set_error(int code, const char* msg);   // use_engine.cpp

namespace use {

namespace {

constexpr int SL_MAPS = 5, SL_MEL = 4;                        // maps 0..3: the Spectrograms; 4: the MelSpectrogram's
constexpr int SL_MEL_N = 2048, SL_MEL_BINS = SL_MEL_N / 2 + 1, SL_MELS = 128, SL_FPTS = SL_MELS + 2;
constexpr int SL_WAV_SLICE = 8192;                            // samples per workgroup of the waveform pass
constexpr double SL_LOG_SCALE = 32768.0, SL_LOG_EPS = 1e-6, SL_NORM_EPS = 1e-6;   // monaural_loss.py:129, 133
constexpr int SL_RED_BYTES = 3 * 256 * (int)sizeof(double);

// fixed-order workgroup sums of three values per thread (256 threads); every thread gets the results
__device__ __forceinline__ void block_sum3(double& a, double& b, double& c, double* sh) {
    const int tid = threadIdx.x;
    __syncthreads();                                          // sh may still be read from the previous use
    sh[tid] = a; sh[256 + tid] = b; sh[512 + tid] = c;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) { sh[tid] += sh[tid + w]; sh[256 + tid] += sh[256 + tid + w]; sh[512 + tid] += sh[512 + tid + w]; }
        __syncthreads();
    }
    a = sh[0]; b = sh[256]; c = sh[512];
}
// sums of p[j * 3 + c], j < n, c < 3, in an order fixed by n
__device__ __forceinline__ void sum_partials3(const double* p, int n, double& a, double& b, double& c, double* sh) {
    a = b = c = 0.0;
    for (int j = threadIdx.x; j < n; j += 256) { a += p[(size_t)j * 3]; b += p[(size_t)j * 3 + 1]; c += p[(size_t)j * 3 + 2]; }
    block_sum3(a, b, c, sh);
}

__global__ void spec_tables_kernel(double* __restrict__ tab, int Nt, double* __restrict__ fpts, double f_max) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k <= Nt / 2) {
        double sn, cs;
        sincospi(2.0 * (double)k / (double)Nt, &sn, &cs);
        tab[2 * k] = cs; tab[2 * k + 1] = -sn;
    }
    if (k < SL_FPTS) {                                        // melscale_fbanks, HTK: 130 points equally spaced in mel
        const double m_max = 2595.0 * log10(1.0 + f_max / 700.0);
        const double m = k == SL_FPTS - 1 ? m_max : (double)k * (m_max / (double)(SL_FPTS - 1));
        fpts[k] = 700.0 * (pow(10.0, m / 2595.0) - 1.0);
    }
}

__global__ __launch_bounds__(256) void spec_wav_kernel(const float* __restrict__ est, const float* __restrict__ clean,
                                                       const int* __restrict__ lens, double* __restrict__ part, int64_t stride, int nblk) {
    __shared__ double sh[3 * 256];
    const int b = blockIdx.y, L = lens[b];
    const int64_t lo = (int64_t)blockIdx.x * SL_WAV_SLICE;
    if (lo >= L) return;                                      // a slice of padding: its partial is never read
    const int64_t hi = lo + SL_WAV_SLICE < L ? lo + SL_WAV_SLICE : L;
    const size_t row = (size_t)b * (size_t)stride;
    double a = 0.0, z0 = 0.0, z1 = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) a += fabs((double)est[row + i] - (double)clean[row + i]);
    block_sum3(a, z0, z1, sh);
    if (threadIdx.x == 0) part[(size_t)b * nblk + blockIdx.x] = a;
}

struct FrameArgs {
    const float* est; const float* clean; const int* lens; const double* tab; const double* fpts; double* part;
    int64_t stride;
    int Tmax, n, log2m, tab_shift;                            // tab_shift = log2(Nt / n)
    int hop, win, off;                                        // window: periodic Hann of `win` samples at offset `off` of the frame
    double df;                                                // mel: spacing of all_freqs = (sr / 2) / 1024
};

// b' = a - w b, a' = a + w b; the same sequence of roundings for both signals
__device__ __forceinline__ void butterfly(double2& a, double2& b, double wr, double wi) {
    const double tr = fma(wr, b.x, -__dmul_rn(wi, b.y)), ti = fma(wr, b.y, __dmul_rn(wi, b.x));
    b = make_double2(__dsub_rn(a.x, tr), __dsub_rn(a.y, ti));
    a = make_double2(__dadd_rn(a.x, tr), __dadd_rn(a.y, ti));
}
// |X[k]| of the real signal packed into Z: a = Z[k mod m], b = Z[(m - k) mod m], w = W_n^k
__device__ __forceinline__ double split_mag(double2 a, double2 b, double wr, double wi) {
    const double er = 0.5 * (a.x + b.x), ei = 0.5 * (a.y - b.y);          // Xe = (a + conj b) / 2
    const double qr = 0.5 * (a.y + b.y), qi = -0.5 * (a.x - b.x);         // Xo = (a - conj b) / (2 i)
    const double xr = er + fma(wr, qr, -__dmul_rn(wi, qi)), xi = ei + fma(wr, qi, __dmul_rn(wi, qr));
    return sqrt(fma(xi, xi, __dmul_rn(xr, xr)));
}
__device__ __forceinline__ double log_term(double me, double mc) {
    return fabs(log(fma(SL_LOG_SCALE, me, SL_LOG_EPS)) - log(fma(SL_LOG_SCALE, mc, SL_LOG_EPS)));
}

template <int MEL>
__global__ __launch_bounds__(256) void spec_frame_kernel(FrameArgs p) {
    extern __shared__ __attribute__((aligned(16))) char sl_smem[];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, L = p.lens[b];
    if (t >= 1 + L / p.hop) return;                           // padding frame
    const int n = p.n, m = n >> 1, log2m = p.log2m;
    double* sh = reinterpret_cast<double*>(sl_smem);          // [3][256] reduction scratch
    double2* ze = reinterpret_cast<double2*>(sl_smem + SL_RED_BYTES);
    double2* zc = ze + m;
    double* mags = reinterpret_cast<double*>(zc + m);         // mel only: [2][SL_MEL_BINS]
    const float* re = p.est + (size_t)b * (size_t)p.stride;
    const float* rc = p.clean + (size_t)b * (size_t)p.stride;

    // the two windowed frames, even samples to the real and odd samples to the imaginary parts, in bit-reversed order
    const long long base = (long long)t * p.hop - m;          // center=True: frame t starts n / 2 samples before t * hop
    for (int j = tid; j < m; j += 256) {
        double v[4];                                          // e[2j], e[2j+1], c[2j], c[2j+1]
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = 2 * j + h, iw = i - p.off;
            double xe = 0.0, xc = 0.0;
            if (iw >= 0 && iw < p.win) {                      // zeros either side of a window shorter than the frame (mel)
                const double w = 0.5 - 0.5 * cospi(2.0 * (double)iw / (double)p.win);
                long long q = base + i;                       // reflect: x[-i] = x[i], x[L-1+i] = x[L-1-i]; len > n / 2 keeps q in [0, L)
                if (q < 0) q = -q;
                if (q >= L) q = 2ll * (L - 1) - q;
                q = q < 0 ? 0 : q >= L ? L - 1 : q;           // never taken for a checked length
                xe = (double)re[q] * w; xc = (double)rc[q] * w;
            }
            v[h] = xe; v[2 + h] = xc;
        }
        const int r = (int)(__brev((unsigned)j) >> (32 - log2m));
        ze[r] = make_double2(v[0], v[1]);
        zc[r] = make_double2(v[2], v[3]);
    }
    __syncthreads();
    for (int s = 0; s < log2m; ++s) {                         // stage s: butterflies h = 2^s apart, twiddle W_{2h}^pos
        const int h = 1 << s, tw_shift = p.tab_shift + log2m - s;          // W_{2h}^pos = tab[pos * Nt / (2h)], Nt / n = 2^tab_shift
        for (int q = tid; q < (m >> 1); q += 256) {
            const int pos = q & (h - 1), i = ((q - pos) << 1) + pos, ti = pos << tw_shift;
            const double wr = p.tab[2 * ti], wi = p.tab[2 * ti + 1];
            double2 a = ze[i], c = ze[i + h];
            butterfly(a, c, wr, wi);
            ze[i] = a; ze[i + h] = c;
            a = zc[i]; c = zc[i + h];
            butterfly(a, c, wr, wi);
            zc[i] = a; zc[i + h] = c;
        }
        __syncthreads();
    }

    double sq = 0.0, c2 = 0.0, lg = 0.0;
    for (int k = tid; k <= m; k += 256) {                     // bins 0 .. n / 2
        const int ka = k & (m - 1), kb = (m - k) & (m - 1), ti = k << p.tab_shift;
        const double wr = p.tab[2 * ti], wi = p.tab[2 * ti + 1];
        const double me = split_mag(ze[ka], ze[kb], wr, wi), mc = split_mag(zc[ka], zc[kb], wr, wi);
        if (MEL) { mags[k] = me; mags[SL_MEL_BINS + k] = mc; }
        else {
            const double d = me - mc;
            sq = fma(d, d, sq); c2 = fma(mc, mc, c2); lg += log_term(me, mc);
        }
    }
    if (MEL) {
        __syncthreads();
        const int j = tid & (SL_MELS - 1);                    // thread (signal tid >> 7, band j): mel[j] = sum_k fb[k][j] M[k]
        const double* M = mags + (tid >> 7) * SL_MEL_BINS;
        const double f0 = p.fpts[j], f1 = p.fpts[j + 1], f2 = p.fpts[j + 2];
        int klo = (int)floor(f0 / p.df), khi = (int)ceil(f2 / p.df);      // fb is zero outside (f0, f2)
        klo = klo < 0 ? 0 : klo; khi = khi > SL_MEL_BINS - 1 ? SL_MEL_BINS - 1 : khi;
        double acc = 0.0;
        for (int k = klo; k <= khi; ++k) {
            const double f = (double)k * p.df;
            const double up = (f - f0) / (f1 - f0), down = (f2 - f) / (f2 - f1);
            acc = fma(fmax(0.0, fmin(up, down)), M[k], acc);
        }
        sh[tid] = acc;
        __syncthreads();
        if (tid < SL_MELS) {
            const double me = sh[tid], mc = sh[tid + SL_MELS], d = me - mc;
            lg = log_term(me, mc); sq = d * d;
        }
    }
    block_sum3(sq, c2, lg, sh);
    if (tid == 0) {
        double* o = p.part + ((size_t)b * p.Tmax + t) * 3;
        o[0] = sq; o[1] = c2; o[2] = lg;
    }
}

struct FinalArgs {
    const int* lens; const double* wav; const double* part[SL_MAPS]; double* out;
    int nwav, Tmax[SL_MAPS], hop[SL_MAPS], bins[SL_MAPS];     // bins: n / 2 + 1, 128 for the mel map
};
__global__ __launch_bounds__(256) void spec_final_kernel(FinalArgs p) {
    __shared__ double sh[3 * 256];
    const int b = blockIdx.x, L = p.lens[b];
    double* o = p.out + (size_t)b * USE_SPECLOSS_COUNT;
    double a = 0.0, z0 = 0.0, z1 = 0.0;
    const int nw = (L + SL_WAV_SLICE - 1) / SL_WAV_SLICE;
    for (int j = threadIdx.x; j < nw; j += 256) a += p.wav[(size_t)b * p.nwav + j];
    block_sum3(a, z0, z1, sh);
    if (threadIdx.x == 0) o[USE_SPECLOSS_WAV_L1] = a / (double)L;
    for (int r = 0; r < SL_MAPS; ++r) {
        const int T = 1 + L / p.hop[r];
        double sq, c2, lg;
        sum_partials3(p.part[r] + (size_t)b * p.Tmax[r] * 3, T, sq, c2, lg, sh);
        if (threadIdx.x == 0) {
            const double cnt = (double)p.bins[r] * (double)T;
            if (r == SL_MEL) { o[USE_SPECLOSS_MEL_LOG] = lg / cnt; o[USE_SPECLOSS_MEL_L2] = sq / cnt; }
            else {
                o[USE_SPECLOSS_MAG_L2 + r] = sq / cnt;
                o[USE_SPECLOSS_MAG_LOG + r] = lg / cnt;
                o[USE_SPECLOSS_MAG_NORM + r] = sqrt(sq) / (sqrt(c2) + SL_NORM_EPS);
            }
        }
    }
}

int failf(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    return use_set_error(code, buf);
}

int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

// the five maps and the byte offsets of the workspace behind the int lens[B]
struct SpecWork {
    int n[SL_MAPS], hop[SL_MAPS], win[SL_MAPS], off[SL_MAPS], Tmax[SL_MAPS];
    size_t part[SL_MAPS], tab, fpts, wav, bytes;
    int Nt, nwav;
};
bool spec_shape_ok(int B, int64_t stride, int sr) { return B >= 1 && B <= 65535 && stride >= 1 && (sr == 24000 || sr == 48000); }
SpecWork spec_layout(int B, int64_t stride, int sr) {
    SpecWork w;
    const int n0 = sr == 24000 ? 256 : 512;                   // int(512 sr / 48000)
    for (int r = 0; r < 4; ++r) { w.n[r] = n0 << r; w.hop[r] = w.n[r] / 4; w.win[r] = w.n[r]; w.off[r] = 0; }
    w.n[SL_MEL] = SL_MEL_N; w.win[SL_MEL] = sr / 40; w.hop[SL_MEL] = sr / 100; w.off[SL_MEL] = (SL_MEL_N - w.win[SL_MEL]) / 2;
    w.Nt = w.n[3] > SL_MEL_N ? w.n[3] : SL_MEL_N;
    const int64_t width = stride < 0x7fffffff ? stride : 0x7fffffff;      // a length is an int
    w.nwav = (int)((width + SL_WAV_SLICE - 1) / SL_WAV_SLICE);
    size_t off = ((size_t)B * sizeof(int) + 7) & ~(size_t)7;
    w.tab = off; off += (size_t)(w.Nt / 2 + 1) * 2 * sizeof(double);
    w.fpts = off; off += (size_t)SL_FPTS * sizeof(double);
    w.wav = off; off += (size_t)B * w.nwav * sizeof(double);
    for (int r = 0; r < SL_MAPS; ++r) {
        w.Tmax[r] = (int)(1 + width / w.hop[r]);
        w.part[r] = off; off += (size_t)B * w.Tmax[r] * 3 * sizeof(double);
    }
    w.bytes = off;
    return w;
}
int frame_lds_bytes(int n, bool mel) { return SL_RED_BYTES + 16 * n + (mel ? 2 * SL_MEL_BINS * (int)sizeof(double) : 0); }

}  // namespace

}  // namespace use

using namespace use;

size_t use_spec_losses_workspace(int B, int64_t stride, int sampling_rate) {
    if (!spec_shape_ok(B, stride, sampling_rate)) return 0;
    return spec_layout(B, stride, sampling_rate).bytes;
}

int use_spec_losses(const float* est, const float* clean, const int* len_host, int B, int64_t stride, int sampling_rate, void* work,
                    size_t work_bytes, double* out_dev, use_stream_t s) {
    if (sampling_rate != 24000 && sampling_rate != 48000)
        return failf(USE_E_INVALID, "use_spec_losses: sampling_rate=%d is neither 24000 nor 48000 (the rates at which the four frame lengths are powers of two)",
                     sampling_rate);
    if (B < 1 || B > 65535) return failf(USE_E_INVALID, "use_spec_losses: B=%d must lie in 1 ... 65535", B);
    if (stride < 1) return failf(USE_E_INVALID, "use_spec_losses: stride=%lld must be positive", (long long)stride);
    if (!est) return failf(USE_E_INVALID, "use_spec_losses: est is null");
    if (!clean) return failf(USE_E_INVALID, "use_spec_losses: clean is null");
    if (!len_host) return failf(USE_E_INVALID, "use_spec_losses: len_host is null");
    if (!work) return failf(USE_E_INVALID, "use_spec_losses: work is null");
    if (!out_dev) return failf(USE_E_INVALID, "use_spec_losses: out_dev is null");
    const SpecWork w = spec_layout(B, stride, sampling_rate);
    int max_len = 0;
    for (int b = 0; b < B; ++b) {
        if (len_host[b] <= w.Nt / 2 || len_host[b] > stride)
            return failf(USE_E_INVALID, "use_spec_losses: len[%d]=%d must lie in %d ... stride = %lld (reflect padding of the %d-point frames needs more than %d samples)",
                         b, len_host[b], w.Nt / 2 + 1, (long long)stride, w.Nt, w.Nt / 2);
        max_len = len_host[b] > max_len ? len_host[b] : max_len;
    }
    if (work_bytes < w.bytes)
        return failf(USE_E_INVALID, "use_spec_losses: work_bytes=%zu is smaller than use_spec_losses_workspace(%d, %lld, %d) = %zu", work_bytes, B,
                     (long long)stride, sampling_rate, w.bytes);
    if ((uintptr_t)work & 7) return failf(USE_E_INVALID, "use_spec_losses: work must be 8-byte aligned");

    hipStream_t st = (hipStream_t)s;
    char* base = static_cast<char*>(work);
    int* lens = reinterpret_cast<int*>(base);
    double* tab = reinterpret_cast<double*>(base + w.tab);
    double* fpts = reinterpret_cast<double*>(base + w.fpts);
    double* wav = reinterpret_cast<double*>(base + w.wav);
    static LdsAttrOnce attr;                                  // 16 n + 6 KB of LDS per frame: 70 KB at n = 4096
    attr.once([&] {
        const int most = frame_lds_bytes(4096, true);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(spec_frame_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, most);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(spec_frame_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, most);
    });
    launch_item_lengths(lens, len_host, B, st);               // as use_metrics: kernel arguments, no copy, no synchronisation
    hipLaunchKernelGGL(spec_tables_kernel, dim3((w.Nt / 2 + 1 + 255) / 256), dim3(256), 0, st, tab, w.Nt, fpts, (double)(sampling_rate / 2));
    hipLaunchKernelGGL(spec_wav_kernel, dim3((max_len + SL_WAV_SLICE - 1) / SL_WAV_SLICE, B), dim3(256), 0, st, est, clean, lens, wav, stride,
                       w.nwav);
    FinalArgs fa{};
    fa.lens = lens; fa.wav = wav; fa.out = out_dev; fa.nwav = w.nwav;
    for (int r = 0; r < SL_MAPS; ++r) {
        FrameArgs a{};
        a.est = est; a.clean = clean; a.lens = lens; a.tab = tab; a.fpts = fpts;
        a.part = reinterpret_cast<double*>(base + w.part[r]);
        a.stride = stride; a.Tmax = w.Tmax[r]; a.n = w.n[r]; a.log2m = ilog2(w.n[r]) - 1; a.tab_shift = ilog2(w.Nt) - ilog2(w.n[r]);
        a.hop = w.hop[r]; a.win = w.win[r]; a.off = w.off[r];
        a.df = (double)(sampling_rate / 2) / (double)(SL_MEL_N / 2);
        const dim3 grid(1 + max_len / w.hop[r], B);           // frames past an item's own count return at once
        if (r == SL_MEL) hipLaunchKernelGGL(spec_frame_kernel<1>, grid, dim3(256), frame_lds_bytes(a.n, true), st, a);
        else hipLaunchKernelGGL(spec_frame_kernel<0>, grid, dim3(256), frame_lds_bytes(a.n, false), st, a);
        fa.part[r] = a.part; fa.Tmax[r] = w.Tmax[r]; fa.hop[r] = w.hop[r]; fa.bins[r] = r == SL_MEL ? SL_MELS : w.n[r] / 2 + 1;
    }
    hipLaunchKernelGGL(spec_final_kernel, dim3(B), dim3(256), 0, st, fa);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(USE_E_HIP, "use_spec_losses: launch failed: %s", hipGetErrorString(e));
    return USE_OK;
}
