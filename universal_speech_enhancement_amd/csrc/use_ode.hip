// Probability-flow ODE sampler: the device half of scipy's RK45 (Dormand-Prince 5(4), scipy 1.15
// scipy/integrate/_ivp/rk.py + common.py) as the reference's get_ode_sampler drives it (reference sampling/__init__.py:76-159),
// with one step-size controller per group of items.
//
// scipy sees the state as one complex128 vector per integration.  Mirrored here: y / y_new in fp64 (double2 per complex element),
// the stages K0..K6 in complex64 (the drift scipy receives is complex64, cast up), every stage input formed in fp64 in scipy's
// order (y + (sum_i a_si K_i) h) and rounded to complex64 for the network.  Norms are RMS over complex elements.
//
// Every element-wise pass runs on a (nblk, B) grid: blockIdx.y is the item, so per-item values (h, stage times) are uniform in a
// workgroup; reductions write one fp64 partial per workgroup and the controller sums them in a fixed order (no float atomics:
// bit-reproducible).  The controller is one workgroup, one thread per group.
#include "use_kernels.h"
#include "use_device.h"

namespace use {

namespace {
// Dormand-Prince tableau (rk.py, class RK45)
__constant__ double kC[7] = {0.0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0, 1.0};
__constant__ double kA[6][5] = {
    {0, 0, 0, 0, 0},
    {1.0 / 5, 0, 0, 0, 0},
    {3.0 / 40, 9.0 / 40, 0, 0, 0},
    {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0},
    {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0},
    {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656}};
__constant__ double kB[6] = {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84};
__constant__ double kE[7] = {-71.0 / 57600, 0, 71.0 / 16695, -71.0 / 1920, 17253.0 / 339200, -22.0 / 525, 1.0 / 40};

constexpr double SAFETY = 0.9, MIN_FACTOR = 0.2, MAX_FACTOR = 10.0, ERR_EXP = -1.0 / 5;   // rk.py:9-11, error_estimator_order 4

DEVI double cabs2(double re, double im) { return re * re + im * im; }
DEVI float2 to_c64(double re, double im) { return make_float2((float)re, (float)im); }

// K = theta (y_sde - x) - (g(t)^2 score) / 2 in float32, operation for operation as the reference's RSDE computes it (sdes.py:119-141);
// cg = g^2 / 2 (the factor 1/2 is exact).  No contraction into FMAs: torch rounds every product.
DEVI float2 pf_drift(float2 x, float2 y, float2 sc, float theta, float cg) {
    return make_float2(__fsub_rn(__fmul_rn(theta, __fsub_rn(y.x, x.x)), __fmul_rn(cg, sc.x)),
                       __fsub_rn(__fmul_rn(theta, __fsub_rn(y.y, x.y)), __fmul_rn(cg, sc.y)));
}

// fixed-order workgroup sum of 256 doubles (thread 0 holds the result)
DEVI double block_sum(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    return sh[0];
}
}  // namespace

__global__ __launch_bounds__(256) void ode_load_kernel(OdeDev d) {
    const int b = blockIdx.y;
    for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < d.n_per_b; j += (long)d.nblk * 256) {
        const long i = (long)b * d.n_per_b + j;
        const float2 x = d.xin[i];
        d.y[i] = make_double2(x.x, x.y);
    }
}

// One stage.  ROW = the stage-time row the network was evaluated at: 0 = f(t0, y0); 1..6 = the stages of an RK45 step (6 = FSAL
// f(t + h, y_new)); 7 = f1 of select_initial_step.  f = the network's score (kind 1) or a ready-made drift (kind 0).
template <int ROW>
__global__ __launch_bounds__(256) void ode_stage_kernel(OdeDev d, const float2* __restrict__ f, int kind) {
    __shared__ double sh[256];
    const int b = blockIdx.y;
    const float cg = d.cg[ROW * d.B + b];
    const double h = d.h_item[b];
    const long n = (long)d.B * d.n_per_b;
    double acc0 = 0.0, acc1 = 0.0;
    for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < d.n_per_b; j += (long)d.nblk * 256) {
        const long i = (long)b * d.n_per_b + j;
        const float2 x = d.xin[i];
        const float2 k = kind ? pf_drift(x, d.ysde[i], f[i], d.theta, cg) : f[i];
        const double2 y = d.y[i];
        if (ROW == 0 || ROW == 7) {                          // select_initial_step (common.py:116-127): scale = atol + |y0| rtol
            const double sc = d.atol + hypot(y.x, y.y) * d.rtol;
            if (ROW == 0) {
                d.K[i] = k;
                acc0 += cabs2(y.x / sc, y.y / sc);
                acc1 += cabs2((double)k.x / sc, (double)k.y / sc);
            } else {
                const float2 k0 = d.K[i];
                acc0 += cabs2(((double)k.x - (double)k0.x) / sc, ((double)k.y - (double)k0.y) / sc);
            }
        } else if (ROW <= 4) {                               // next stage input: y + (K[:s+1].T @ a) h   (rk.py:62-64)
            d.K[(size_t)ROW * n + i] = k;
            double sr = 0.0, si = 0.0;
#pragma unroll
            for (int q = 0; q < ROW; ++q) {
                const float2 kq = d.K[(size_t)q * n + i];
                sr += (double)kq.x * kA[ROW + 1][q]; si += (double)kq.y * kA[ROW + 1][q];
            }
            sr += (double)k.x * kA[ROW + 1][ROW]; si += (double)k.y * kA[ROW + 1][ROW];
            d.xin[i] = to_c64(y.x + sr * h, y.y + si * h);
        } else if (ROW == 5) {                               // y_new = y + h (K[:-1].T @ B)   (rk.py:66)
            d.K[(size_t)5 * n + i] = k;
            double sr = 0.0, si = 0.0;
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const float2 kq = d.K[(size_t)q * n + i];
                sr += (double)kq.x * kB[q]; si += (double)kq.y * kB[q];
            }
            sr += (double)k.x * kB[5]; si += (double)k.y * kB[5];
            const double2 yn = make_double2(y.x + h * sr, y.y + h * si);
            d.ynew[i] = yn;
            d.xin[i] = to_c64(yn.x, yn.y);
        } else {                                             // ROW 6: FSAL stage + error estimate (K.T @ E) h / scale   (rk.py:109-113, 145-146)
            d.K[(size_t)6 * n + i] = k;
            double er = 0.0, ei = 0.0;
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const float2 kq = d.K[(size_t)q * n + i];
                er += (double)kq.x * kE[q]; ei += (double)kq.y * kE[q];
            }
            er += (double)k.x * kE[6]; ei += (double)k.y * kE[6];
            const double2 yn = d.ynew[i];
            const double sc = d.atol + fmax(hypot(y.x, y.y), hypot(yn.x, yn.y)) * d.rtol;
            acc0 += cabs2(er * h / sc, ei * h / sc);
        }
    }
    if (ROW == 0 || ROW == 6 || ROW == 7) {
        const double s0 = block_sum(acc0, sh);
        if (threadIdx.x == 0) d.part[(size_t)b * d.nblk + blockIdx.x] = s0;
        if (ROW == 0) {
            __syncthreads();
            const double s1 = block_sum(acc1, sh);
            if (threadIdx.x == 0) d.part[(size_t)(d.B + b) * d.nblk + blockIdx.x] = s1;
        }
    }
}

// After a step: accepted groups take y_new and the FSAL stage (K0 = K6).  Then, for every item, the first stage input of the next
// attempt: y + (K0 coef) h  (coef = a_10 = 1/5; 1 for the probe y0 + h0 f0 of select_initial_step).
__global__ __launch_bounds__(256) void ode_commit_kernel(OdeDev d, double coef) {
    const int b = blockIdx.y;
    const bool acc = d.grp[b / d.G].accepted != 0;
    const double h = d.h_item[b];
    const long n = (long)d.B * d.n_per_b;
    for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < d.n_per_b; j += (long)d.nblk * 256) {
        const long i = (long)b * d.n_per_b + j;
        double2 y;
        float2 k0;
        if (acc) { y = d.ynew[i]; d.y[i] = y; k0 = d.K[(size_t)6 * n + i]; d.K[i] = k0; }
        else { y = d.y[i]; k0 = d.K[i]; }
        d.xin[i] = to_c64(y.x + ((double)k0.x * coef) * h, y.y + ((double)k0.y * coef) * h);
    }
}

__global__ __launch_bounds__(256) void ode_result_kernel(OdeDev d, float2* __restrict__ out) {
    const int b = blockIdx.y;
    for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < d.n_per_b; j += (long)d.nblk * 256) {
        const long i = (long)b * d.n_per_b + j;
        const double2 y = d.y[i];
        out[i] = to_c64(y.x, y.y);
    }
}

namespace {
// g(t)^2 / 2 with g of OUVESDE.sde (sdes.py:218-221) at the item's float32 t, rounded as torch rounds it: sigma_min * base ** t and
// sigma * sqrt(2 logsig) are float32 products with the Python constants cast to float32.  The RK45 error estimate at rtol 1e-5 sits
// near the float32 rounding of the drift, so a one-ulp difference in g moves the accepted step sizes visibly.
DEVI float ode_cg(const OdeCtl& c, float t) {
    const float sigma = __fmul_rn(c.sigma_min, powf(c.base, t));
    const float g = __fmul_rn(sigma, c.sq2ls);
    return 0.5f * __fmul_rn(g, g);
}

// the per-item values of group `g` for its next evaluation(s): rows [r0, r1] of the stage times at t + C_r h
DEVI void ode_write_items(const OdeCtl& c, OdeDev& d, int g, double t, double h, int r0, int r1, const double* coef) {
    const int b0 = g * c.G, b1 = min(c.B, b0 + c.G);
    for (int b = b0; b < b1; ++b) {
        d.h_item[b] = h;
        for (int r = r0; r <= r1; ++r) {
            const float tr = (float)(t + coef[r] * h);
            d.ts[r * c.B + b] = tr;
            d.cg[r * c.B + b] = ode_cg(c, tr);
        }
    }
}

// the start of an attempt (rk.py:118-141): at a new step, the attempt's step size q.ha is q.h_abs clamped to [min_step, max_step]
// (q.h_abs itself, scipy's self.h_abs, is left alone); the failure below min_step, the last step clamped onto t_bound; then the stage
// times.  A group that is done is frozen: h = 0 and every stage at its final t.
DEVI void ode_prepare(const OdeCtl& c, OdeDev& d, int g) {
    OdeGroup& q = d.grp[g];
    if (q.status == 1) {
        if (!q.rejected) {
            q.min_step = 10.0 * fabs(nextafter(q.t, -INFINITY) - q.t);
            q.ha = q.h_abs > c.max_step ? c.max_step : q.h_abs < q.min_step ? q.min_step : q.h_abs;
        }
        if (q.ha < q.min_step) q.status = -1;                                   // scipy: TOO_SMALL_STEP, status -1
        else if (q.nfev + 6 > c.max_nfe) q.status = -2;                          // the max_nfe guard
    }
    if (q.status != 1) {
        q.h = 0.0;
        ode_write_items(c, d, g, q.t, 0.0, 1, 6, kC);
        return;
    }
    double t_new = q.t - q.ha;                                                   // direction -1: from T down to eps
    if (t_new < c.t_bound) t_new = c.t_bound;
    q.h = t_new - q.t;
    q.ha = fabs(q.h);
    q.t_new = t_new;
    ode_write_items(c, d, g, q.t, q.h, 1, 6, kC);
}

DEVI double group_norm(const OdeCtl& c, const OdeDev& d, int k, int g) {   // RMS over the group's complex elements (common.py:63-65)
    const int b0 = g * c.G, b1 = min(c.B, b0 + c.G);
    double s = 0.0;
    for (int b = b0; b < b1; ++b)
        for (int j = 0; j < c.nblk; ++j) s += d.part[((size_t)k * c.B + b) * c.nblk + j];
    return sqrt(s) / sqrt((double)(b1 - b0) * (double)c.n_per_b);
}
}  // namespace

__global__ __launch_bounds__(256) void ode_ctrl_kernel(OdeCtl c, OdeDev d, int mode) {
    __shared__ int busy;
    if (threadIdx.x == 0) busy = 0;
    __syncthreads();
    for (int g = threadIdx.x; g < c.ngroups; g += 256) {
        OdeGroup& q = d.grp[g];
        q.accepted = 0;
        if (mode == ODE_START) {
            q = OdeGroup{};
            q.t = c.t0; q.status = 1; q.nfev = 1;                                  // f0 = fun(t0, y0)
            const double zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            ode_write_items(c, d, g, c.t0, 0.0, 0, 0, zero);
        } else if (mode == ODE_INIT1) {                                            // select_initial_step, common.py:112-126
            const double interval = fabs(c.t_bound - c.t0);
            if (c.first_step > 0) { q.h_abs = c.first_step; ode_prepare(c, d, g); }
            else {
                const double d0 = group_norm(c, d, 0, g), d1 = group_norm(c, d, 1, g);
                double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
                h0 = fmin(h0, interval);
                q.h0 = h0; q.d1 = d1; q.nfev += 1;
                const double dir[8] = {0, 0, 0, 0, 0, 0, 0, 1.0};
                ode_write_items(c, d, g, c.t0, h0 * -1.0, 7, 7, dir);             // f1 = fun(t0 + h0 direction, y0 + h0 direction f0)
            }
        } else if (mode == ODE_INIT2) {                                            // common.py:127-134
            const double interval = fabs(c.t_bound - c.t0);
            const double d2 = group_norm(c, d, 0, g) / q.h0;
            const double h1 = (q.d1 <= 1e-15 && d2 <= 1e-15) ? fmax(1e-6, q.h0 * 1e-3) : pow(0.01 / fmax(q.d1, d2), 1.0 / 5);
            q.h_abs = fmin(fmin(100 * q.h0, h1), fmin(interval, c.max_step));
            ode_prepare(c, d, g);
        } else {                                                                   // ODE_STEP: accept / reject (rk.py:145-166)
            if (q.status == 1) {
                q.nfev += 6;                                                       // counted once spent, as scipy's nfev
                const double en = group_norm(c, d, 0, g);
                if (en < 1) {
                    double factor = en == 0 ? MAX_FACTOR : fmin(MAX_FACTOR, SAFETY * pow(en, ERR_EXP));
                    if (q.rejected) factor = fmin(1.0, factor);
                    q.h_abs = q.ha * factor;
                    q.t = q.t_new; q.rejected = 0; q.accepted = 1; q.steps += 1;
                    if (q.t <= c.t_bound) q.status = 0;                            // base.py: direction * (t - t_bound) >= 0
                } else {
                    q.ha *= fmax(MIN_FACTOR, SAFETY * pow(en, ERR_EXP));
                    q.rejected = 1; q.nrej += 1;
                }
            }
            ode_prepare(c, d, g);
        }
        if (q.status == 1) atomicOr(&busy, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) *d.done = busy ? 0 : 1;
}

void launch_ode_load(const OdeDev& d, hipStream_t s) {
    hipLaunchKernelGGL(ode_load_kernel, dim3(d.nblk, d.B), dim3(256), 0, s, d);
}
void launch_ode_stage(const OdeDev& d, int row, const float2* f, int kind, hipStream_t s) {
    const dim3 g(d.nblk, d.B), blk(256);
    switch (row) {
        case 0: hipLaunchKernelGGL(ode_stage_kernel<0>, g, blk, 0, s, d, f, kind); break;
        case 1: hipLaunchKernelGGL(ode_stage_kernel<1>, g, blk, 0, s, d, f, kind); break;
        case 2: hipLaunchKernelGGL(ode_stage_kernel<2>, g, blk, 0, s, d, f, kind); break;
        case 3: hipLaunchKernelGGL(ode_stage_kernel<3>, g, blk, 0, s, d, f, kind); break;
        case 4: hipLaunchKernelGGL(ode_stage_kernel<4>, g, blk, 0, s, d, f, kind); break;
        case 5: hipLaunchKernelGGL(ode_stage_kernel<5>, g, blk, 0, s, d, f, kind); break;
        case 6: hipLaunchKernelGGL(ode_stage_kernel<6>, g, blk, 0, s, d, f, kind); break;
        default: hipLaunchKernelGGL(ode_stage_kernel<7>, g, blk, 0, s, d, f, kind); break;
    }
}
void launch_ode_commit(const OdeDev& d, double coef, hipStream_t s) {
    hipLaunchKernelGGL(ode_commit_kernel, dim3(d.nblk, d.B), dim3(256), 0, s, d, coef);
}
void launch_ode_ctrl(const OdeCtl& c, const OdeDev& d, int mode, hipStream_t s) {
    hipLaunchKernelGGL(ode_ctrl_kernel, dim3(1), dim3(256), 0, s, c, d, mode);
}
void launch_ode_result(const OdeDev& d, float2* out, hipStream_t s) {
    hipLaunchKernelGGL(ode_result_kernel, dim3(d.nblk, d.B), dim3(256), 0, s, d, out);
}

}  // namespace use
