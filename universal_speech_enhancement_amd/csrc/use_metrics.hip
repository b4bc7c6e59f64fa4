// Evaluation metrics on the device (reference sgmse/util/other.py:15-62): SI-SDR / SI-SIR / SI-SAR (si_sdr_components +
// energy_ratios) and the reference's log-spectral distance (lsd), per item of a zero-padded batch est / clean / noise [B][stride]
// with valid lengths len[b].  Everything is fp64 and every sum has a fixed order that depends on len[b] alone - not on B, stride or
// the neighbours - so an item gives the same bits in any batch and in any run (no float atomics).
//
// Energy ratios, two passes as the reference computes them (a one-pass closed form cancels at high SI-SAR):
//   dots    (nblk, B)  <s^,s>, <s^,n>, <s,s>, <n,n> of one 2048-sample slice per workgroup -> 4 partials (float32 x float32 is exact in fp64)
//   alpha   (B)        partials summed in slice order; alpha_s = <s^,s> / (eps + |s|^2), alpha_n = <s^,n> / (eps + |n|^2)
//   energy  (nblk, B)  s_t = alpha_s s, e_n = alpha_n n, e_a = s^ - s_t - e_n: |s_t|^2, |e_n|^2, |e_a|^2, |e_n + e_a|^2 -> 4 partials
//   final   (B)        10 log10(eps + |s_t|^2 / (eps + .)), |.|^2 = (sqrt(sum))^2 as np.linalg.norm(.) ** 2
// LSD: sqrt(mean over 256 bins x T_b frames of |2 log(eps + |S^|) - 2 log(eps + |S|)|), S = STFT(n_fft 510, hop 128, periodic Hann,
// centred, reflect padding), T_b = 1 + len[b] / 128:
//   lsd     (Tmax, B)  one workgroup per (frame, item), thread k owns bin k of BOTH signals: the 510-point DFT as a direct sum in fp64
//                      with fp64 twiddles and window built in LDS, then the frame's sum over bins -> 1 partial.  Frames t >= T_b
//                      return at once and their partials are never read: the batch's padding cannot reach the result.
//   final              partials summed in frame order.
// The spectra are fp64 and never leave the workgroup (no scratch spectrogram): the metric is the float64 evaluation of the reference's
// formula, whose distance from the reference's own float32 torch.stft is that float32 run's rounding error and nothing else.
#include "use_kernels.h"

namespace use {

namespace {
constexpr double M_EPS = 1e-10;            // other.py:23, 33, 48
constexpr int M_NFFT = 510, M_HOP = 128, M_BINS = M_NFFT / 2 + 1;   // other.py:15-20; 256 bins = one per thread

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
// sum of p[j * step], j < n, in an order fixed by n
__device__ __forceinline__ double sum_partials(const double* p, int n, int step, double* sh) {
    double a = 0.0;
    for (int j = threadIdx.x; j < n; j += 256) a += p[(size_t)j * step];
    return block_sum(a, sh);
}

struct LenPack { int v[64]; };
__global__ void item_lengths_kernel(int* lens, LenPack p, int base, int B) {
    const int i = threadIdx.x;
    if (base + i < B) lens[base + i] = p.v[i];
}

// PASS 0: the four dot products; PASS 1: the four energies of the components
template <int PASS>
__global__ __launch_bounds__(256) void metrics_pass_kernel(const float* __restrict__ est, const float* __restrict__ clean,
                                                           const float* __restrict__ noise, const int* __restrict__ lens,
                                                           const double* __restrict__ alpha, double* __restrict__ part, int stride,
                                                           int nblk) {
    __shared__ double sh[256];
    const int b = blockIdx.y, L = lens[b];
    const int lo = blockIdx.x * METRICS_SLICE;
    if (lo >= L) return;                                      // a slice of padding: its partials are never read
    const int hi = min(lo + METRICS_SLICE, L);
    const size_t row = (size_t)b * stride;
    double as = 0.0, an = 0.0;
    if (PASS == 1) { as = alpha[2 * b]; an = alpha[2 * b + 1]; }
    double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += 256) {
        const double e = est[row + i], s = clean[row + i], n = noise[row + i];
        if (PASS == 0) {
            q0 = fma(e, s, q0); q1 = fma(e, n, q1); q2 = fma(s, s, q2); q3 = fma(n, n, q3);
        } else {                                              // rounded product by product, as numpy's array expressions are
            const double st = __dmul_rn(as, s), en = __dmul_rn(an, n);
            const double ea = __dsub_rn(__dsub_rn(e, st), en), na = __dadd_rn(en, ea);
            q0 = fma(st, st, q0); q1 = fma(en, en, q1); q2 = fma(ea, ea, q2); q3 = fma(na, na, q3);
        }
    }
    double* out = part + ((size_t)b * nblk + blockIdx.x) * 4;
    q0 = block_sum(q0, sh); q1 = block_sum(q1, sh); q2 = block_sum(q2, sh); q3 = block_sum(q3, sh);
    if (threadIdx.x == 0) { out[0] = q0; out[1] = q1; out[2] = q2; out[3] = q3; }
}

__global__ __launch_bounds__(256) void metrics_alpha_kernel(const double* __restrict__ part, const int* __restrict__ lens,
                                                            double* __restrict__ alpha, int nblk) {
    __shared__ double sh[256];
    const int b = blockIdx.x, n = (lens[b] + METRICS_SLICE - 1) / METRICS_SLICE;
    const double* p = part + (size_t)b * nblk * 4;
    const double es = sum_partials(p + 0, n, 4, sh), en = sum_partials(p + 1, n, 4, sh);
    const double ss = sum_partials(p + 2, n, 4, sh), nn = sum_partials(p + 3, n, 4, sh);
    if (threadIdx.x == 0) {
        const double ns = sqrt(ss), nm = sqrt(nn);            // np.linalg.norm(.) ** 2
        alpha[2 * b] = es / (M_EPS + ns * ns);
        alpha[2 * b + 1] = en / (M_EPS + nm * nm);
    }
}

__global__ __launch_bounds__(256) void metrics_lsd_kernel(const float* __restrict__ est, const float* __restrict__ clean,
                                                          const int* __restrict__ lens, double* __restrict__ part, int stride,
                                                          int Tmax) {
    __shared__ double xe[M_NFFT], xc[M_NFFT], sh[256];
    __shared__ double2 tw[M_NFFT];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, L = lens[b];
    if (t >= 1 + L / M_HOP) return;                           // padding frame
    const size_t row = (size_t)b * stride;
    for (int n = tid; n < M_NFFT; n += 256) {
        double sn, cs;
        sincospi(2.0 * (double)n / (double)M_NFFT, &sn, &cs);
        tw[n] = make_double2(cs, sn);
        const double w = 0.5 - 0.5 * cs;                      // periodic Hann (torch.hann_window(510))
        int q = t * M_HOP + n - M_NFFT / 2;                   // center=True: reflect padding of 255 samples; L >= 256 keeps q in [0, L)
        if (q < 0) q = -q;
        if (q >= L) q = 2 * (L - 1) - q;
        xe[n] = (double)est[row + q] * w;
        xc[n] = (double)clean[row + q] * w;
    }
    __syncthreads();
    const int k = tid;                                        // M_BINS == 256 == blockDim.x
    double er = 0.0, ei = 0.0, cr = 0.0, ci = 0.0;
    int idx = 0;                                              // (k n) mod 510
    for (int n = 0; n < M_NFFT; ++n) {
        const double2 c = tw[idx];
        idx += k; if (idx >= M_NFFT) idx -= M_NFFT;
        const double a = xe[n], s = xc[n];
        er = fma(a, c.x, er); ei = fma(-a, c.y, ei);
        cr = fma(s, c.x, cr); ci = fma(-s, c.y, ci);
    }
    const double d = fabs(2.0 * log(M_EPS + hypot(er, ei)) - 2.0 * log(M_EPS + hypot(cr, ci)));
    const double sum = block_sum(d, sh);
    if (tid == 0) part[(size_t)b * Tmax + t] = sum;
}

__global__ __launch_bounds__(256) void metrics_final_kernel(const double* __restrict__ part2, const double* __restrict__ lsd_part,
                                                            const int* __restrict__ lens, double* __restrict__ out, int nblk,
                                                            int Tmax, int has_noise) {
    __shared__ double sh[256];
    const int b = blockIdx.x, L = lens[b], T = 1 + L / M_HOP;
    double sdr = __builtin_nan(""), sir = sdr, sar = sdr;
    if (has_noise) {
        const int n = (L + METRICS_SLICE - 1) / METRICS_SLICE;
        const double* p = part2 + (size_t)b * nblk * 4;
        double st = sqrt(sum_partials(p + 0, n, 4, sh)), en = sqrt(sum_partials(p + 1, n, 4, sh));
        double ea = sqrt(sum_partials(p + 2, n, 4, sh)), na = sqrt(sum_partials(p + 3, n, 4, sh));
        st *= st; en *= en; ea *= ea; na *= na;
        sdr = 10.0 * log10(M_EPS + st / (M_EPS + na));
        sir = 10.0 * log10(M_EPS + st / (M_EPS + en));
        sar = 10.0 * log10(M_EPS + st / (M_EPS + ea));
    }
    const double m = sum_partials(lsd_part + (size_t)b * Tmax, T, 1, sh) / ((double)M_BINS * (double)T);
    if (threadIdx.x == 0) {
        double* o = out + (size_t)b * 4;                      // USE_METRIC_SI_SDR, _SI_SIR, _SI_SAR, _LSD
        o[0] = sdr; o[1] = sir; o[2] = sar; o[3] = sqrt(m);
    }
}
}  // namespace

void launch_item_lengths(int* lens, const int* len_host, int B, hipStream_t s) {
    for (int b0 = 0; b0 < B; b0 += 64) {                      // the lengths travel as kernel arguments: no copy, no synchronisation
        LenPack p{};
        for (int i = 0; i < 64 && b0 + i < B; ++i) p.v[i] = len_host[b0 + i];
        hipLaunchKernelGGL(item_lengths_kernel, dim3(1), dim3(64), 0, s, lens, p, b0, B);
    }
}

MetricsWork metrics_layout(int B, int stride) {
    MetricsWork w;
    w.nblk = (stride + METRICS_SLICE - 1) / METRICS_SLICE;
    w.Tmax = 1 + stride / M_HOP;
    size_t off = ((size_t)B * sizeof(int) + 7) & ~(size_t)7;
    w.part1 = off; off += (size_t)B * w.nblk * 4 * sizeof(double);
    w.part2 = off; off += (size_t)B * w.nblk * 4 * sizeof(double);
    w.alpha = off; off += (size_t)B * 2 * sizeof(double);
    w.lsd = off; off += (size_t)B * w.Tmax * sizeof(double);
    w.bytes = off;
    return w;
}

void launch_metrics(const float* est, const float* clean, const float* noise, const int* len_host, int B, int stride, void* work,
                    double* out, hipStream_t s) {
    const MetricsWork w = metrics_layout(B, stride);
    char* base = static_cast<char*>(work);
    int* lens = reinterpret_cast<int*>(base);
    double* part1 = reinterpret_cast<double*>(base + w.part1);
    double* part2 = reinterpret_cast<double*>(base + w.part2);
    double* alpha = reinterpret_cast<double*>(base + w.alpha);
    double* lsd = reinterpret_cast<double*>(base + w.lsd);
    launch_item_lengths(lens, len_host, B, s);
    const dim3 pass_grid(w.nblk, B), lsd_grid(w.Tmax, B);     // the caller has checked B <= 65535 (gridDim.y)
    hipLaunchKernelGGL(metrics_lsd_kernel, lsd_grid, dim3(256), 0, s, est, clean, lens, lsd, stride, w.Tmax);
    if (noise) {
        hipLaunchKernelGGL(metrics_pass_kernel<0>, pass_grid, dim3(256), 0, s, est, clean, noise, lens, (const double*)nullptr, part1,
                           stride, w.nblk);
        hipLaunchKernelGGL(metrics_alpha_kernel, dim3(B), dim3(256), 0, s, part1, lens, alpha, w.nblk);
        hipLaunchKernelGGL(metrics_pass_kernel<1>, pass_grid, dim3(256), 0, s, est, clean, noise, lens, alpha, part2, stride, w.nblk);
    }
    hipLaunchKernelGGL(metrics_final_kernel, dim3(B), dim3(256), 0, s, part2, lsd, lens, out, w.nblk, w.Tmax, noise ? 1 : 0);
}

}  // namespace use
