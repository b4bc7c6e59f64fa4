/* use_hip.h -- C ABI of libuse_hip.so: the MI355X (gfx950) implementation of the SGMSE reverse-SDE
 * sampling path of nanless/universal-speech-enhancement.
 *
 * Boundary (reference file:line, all Python -- the reference has no FFI for this path; the entry points below
 * are what a ctypes binding of the path binds):
 *   use_score        <- ScoreModel.forward / forward_score      src/models/components/sgmse/model_wrapper.py:135-145
 *                       (= -NCSNpp.forward(cat[x, Y], t)         .../backbones/ncsnpp.py:324-501)
 *   use_sample       <- sampling.get_pc_sampler()->pc_sampler()  .../sampling/__init__.py:23-73
 *   use_sample_ode   <- sampling.get_ode_sampler()->ode_sampler() .../sampling/__init__.py:76-159 (scipy RK45, on the device)
 *   use_set_weight   <- LightningModule checkpoint load: state_dict keys "all_modules.<i>....", "output_layer.*"
 *                       (.../backbones/ncsnpp.py:116-316)
 *   use_sde_*        <- OUVESDE.prior_sampling (sdes.py:248-254), ReverseDiffusionPredictor / EulerMaruyamaPredictor
 *                       update_fn (sampling/predictors.py:40-68), LangevinCorrector / AnnealedLangevinDynamics
 *                       update_fn (sampling/correctors.py:37-98)
 *
 * Conventions: every function returns 0 on success or a negative USE_E_* code and never throws; the failing
 * call's message is available from use_last_error() (thread-local).  The caller owns every input / output
 * buffer and passes raw DEVICE pointers (complex64 spectrograms are [B][1][F][T'] == interleaved (re, im)
 * floats, T' a multiple of 64) plus the HIP stream to run on; the library owns weights-on-device, workspace and
 * captured graphs inside the handle.  One handle per (process, device); a handle is not re-entrant.  No call
 * synchronises the device except use_commit_weights / use_plan / use_destroy.
 */
#ifndef USE_HIP_H
#define USE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct use_handle use_handle;
typedef void* use_stream_t; /* hipStream_t */

enum { USE_OK = 0, USE_E_INVALID = -1, USE_E_HIP = -2, USE_E_STATE = -3, USE_E_NOMEM = -4 };
enum { USE_PREC_FP32 = 0, USE_PREC_BF16 = 1, USE_PREC_FP16 = 2 };   /* storage of activations / conv weights; accumulation is always fp32 */
enum { USE_PRED_REVERSE_DIFFUSION = 0, USE_PRED_EULER_MARUYAMA = 1, USE_PRED_NONE = 2 };
enum { USE_CORR_NONE = 0, USE_CORR_LANGEVIN = 1, USE_CORR_ALD = 2 };

typedef struct use_config {
    int nf;                /* base width (128)                                   ncsnpp.py:46            */
    int n_levels;          /* len(ch_mult)                                                             */
    int ch_mult[8];        /* (1,1,2,2,2,2,2) for NCSNppLarge                    ncsnpp.py:512-517       */
    int num_res_blocks;    /* 2                                                                        */
    int n_freq;            /* F = n_fft/2+1 = 512                                SGMSE_Large.yaml:11     */
    int precision;         /* USE_PREC_*: activation/weight storage; accumulation is always fp32        */
    float theta, sigma_min, sigma_max; /* OUVE SDE (1.5, 0.05, 0.5)              sdes.py:184             */
    /* NCSNpp(discriminative=True), the generator of the LSGAN refine stage (ncsnpp.py:86-92,
     * GAN/generator/ncsnpp/model_wrapper.py:54): 0 everywhere = the score network above */
    int input_channels;    /* real input channels: 0 or 4 = (x, y) re/im; 2 = (y) alone; 6 = (x, y, y2)   ncsnpp.py:63,92 */
    int unconditional;     /* 1: no time embedding (conditional=False)                                 ncsnpp.py:89   */
    int no_sigma_scale;    /* 1: output not divided by t (scale_by_sigma=False)                        ncsnpp.py:90   */
} use_config;

typedef struct use_sampler_config {
    int N;                 /* reverse steps                                     model_wrapper.py:266    */
    int predictor;         /* USE_PRED_*                                                               */
    int corrector;         /* USE_CORR_*                                                               */
    int corrector_steps;   /* ignored for USE_CORR_NONE                                                */
    float snr;             /* corrector snr                                                            */
    float t_eps;           /* smallest time (3e-2)                               model_wrapper.py:27     */
    int use_graph;         /* 1: capture the whole loop in a hipGraph and replay it                    */
} use_sampler_config;

/* Process-wide tuning knobs (no reference counterpart).  "subbatch" (default -1 = by batch size: three sub-batches for 6-11 items, else two; round 5: batch 8 as 3 + 3 + 2 is 1.6 % faster than 4 + 4): batches of >= 4 items are evaluated as
 * sub-batches (>= 2 items each) on separate streams, staggered so that the small-map kernels of one run beside the large convolutions of
 * the others; items never interact inside the network, so results are identical to subbatch = 0 (read at use_plan).  "conv_v4_min_blocks": smallest per-image grid (workgroups) the
 * wide-tile convolution kernel is selected for, default 80; results do not depend on it beyond rounding order.  "conv_v5" (default 1): the wide-tile kernel
 * on v_mfma_f32_16x16x32 in the 16-bit storage modes (conv_wide_kernel<Wide16x16>; 0: conv_wide_kernel<Wide32x32>, v_mfma_f32_32x32x16) - bit-identical results, less energy per FLOP.  "stats_part" (default 1): on maps
 * above "gn_inline" pixels (default 128 x 160) the convolutions write per-workgroup GroupNorm partial totals with plain stores and the
 * finalisation sums them, instead of 64-bit atomics on the item's totals - integer sums either way: bit-identical results (read at use_plan).
 * "fir_strip" (default 1): the res-block down-sampler walks 8- or 4-row strips (0: the 2 x 2 block form; 8 / 4: forced) - bit-identical.
 * "conv_in_wgs" (default 256): most workgroups per item of the input convolution (each walks tiles / conv_in_wgs tiles; stored values do not depend on
 * it; read at use_plan).
 * ALL options are read at use_plan (they size workspace buffers - "conv_in_wgs", "stats_part", "gn_inline", "subbatch*" - or choose kernels):
 * every use_set_option marks the plans built before it stale.  use_score / use_forward / use_sample* / use_set_sampler on a stale plan return
 * USE_E_STATE ("... call use_plan (and use_set_sampler) again" in use_last_error()); nothing is launched, the handle stays usable.  Should an
 * evaluation still not fit its workspace the entry point returns USE_E_STATE as well (output invalid) - never a write past the allocation,
 * never abort() (round 6; SURVEY 8b "never throw across the ABI").
 * Others: "stagger_level", "gn_inline", "plan_cache", "attn_fused", "pyr_ws", "conv_sk_max_px", "wgrad_mfma16", "wgrad_blocks" (INTEGRATION.md). */
int use_set_option(const char* name, long long value);
const char* use_last_error(void);
const char* use_version(void);

int use_create(const use_config* cfg, int device, use_handle** out);
int use_destroy(use_handle* h);

/* Weights.  name = reference state-dict key relative to the score net ("all_modules.4.Conv_0.weight", ...);
 * data = HOST float32, C-contiguous, shape as in the reference.  use_commit_weights packs (transposes to
 * [tap][cout][cin], converts to the compute dtype) and uploads one blob. */
int use_set_weight(use_handle* h, const char* name, const float* data, const int64_t* shape, int ndim);
int use_commit_weights(use_handle* h);
/* Multi-GPU: the packed device blob can be broadcast (RCCL) instead of re-packing on every rank:
 * rank 0 commits, the others call use_alloc_weight_blob, all ranks broadcast [ptr, ptr+bytes). */
int use_alloc_weight_blob(use_handle* h);
int use_weight_blob(use_handle* h, void** dev_ptr, size_t* bytes);
/* Packed weight file: a versioned header (architecture, precision, blob layout version, crc32) + the device blob, so that a
 * deployment starts from one read instead of a Lightning checkpoint (which replaces `torch.load` + `load_state_dict`,
 * predict.py:79).  use_save_weight_blob works after use_set_weight of every tensor (packs on the host: no GPU needed) or
 * after a commit / load; use_load_weight_blob replaces use_set_weight x N + use_commit_weights and refuses files packed
 * for another configuration, precision or layout version. */
int use_save_weight_blob(use_handle* h, const char* path);
int use_load_weight_blob(use_handle* h, const char* path);
int use_num_expected_weights(use_handle* h);
int use_expected_weight(use_handle* h, int index, const char** name, int64_t* shape4, int* ndim);

/* Workspace for batch B and T' padded frames (multiple of 64).  Re-planning is allowed.
 * After a failing use_plan the handle has no plan: evaluations answer USE_E_STATE until a use_plan succeeds. */
int use_plan(use_handle* h, int B, int Tpad);
int use_workspace_bytes(use_handle* h, size_t* bytes);

/* One score evaluation: out = -score_net(cat[x, y], t).  x, y, out: complex64 [B,1,F,T']; t: float32 [B] (device). */
int use_score(use_handle* h, const void* x, const void* y, const float* t, void* out, use_stream_t stream);
/* The same for a handle created with input_channels = 6 (ScoreModel(condition="both"), model_wrapper.py:43-46, 287-288):
 * out = -score_net(cat[x, y, y2], t) with the two conditioning spectrograms [Y, Y_denoised]. */
int use_score2(use_handle* h, const void* x, const void* y, const void* y2, const float* t, void* out, use_stream_t stream);

/* Whole PC sampler: prior sampling -> N x (corrector, predictor) -> x_mean of the last predictor step.
 * noise: complex64 [n_draws][B,1,F,T'] consumed in the reference's order (prior, then per step the corrector
 * draws followed by the predictor draw), or NULL to draw on-device (Philox4x32-10, `seed`). */
int use_set_sampler(use_handle* h, const use_sampler_config* sc);
int use_num_noise_draws(use_handle* h);
int use_get_timesteps(use_handle* h, float* out, int n);
int use_sample(use_handle* h, const void* y, const void* noise, uint64_t seed, void* out, use_stream_t stream);
/* The same loop with the score conditioning separated from the SDE's y: the network sees cat[x, cond] while the drift, the
 * prior mean and the result refer to y -- ScoreModel.sample with condition="denoised" (conditioning = the GAN-denoised
 * spectrogram) and sde_input "noisy" or "denoised" (model_wrapper.py:283-301).  cond == NULL is use_sample. */
int use_sample_cond(use_handle* h, const void* y, const void* cond, const void* noise, uint64_t seed, void* out, use_stream_t stream);
/* condition="both": the network sees cat[x, cond, cond2] (6-channel handle; cond == NULL: the SDE's y). */
int use_sample_cond2(use_handle* h, const void* y, const void* cond, const void* cond2, const void* noise, uint64_t seed, void* out,
                     use_stream_t stream);

/* The batch-invariant form of the same loop (the sampler of use_set_sampler; plan, cond / cond2 rules and error codes of
 * use_sample_cond2).  Two differences from use_sample*: item b draws from its own Philox stream, z[b][j] = Philox(seeds_host[b],
 * draw, j) with j the element index INSIDE the item's F*T' complex elements - the stream use_sample gives a one-item batch with
 * seed = seeds_host[b], draws numbered alike - and the Langevin step size is the item's own, eps_b = 2 (snr ||z_b|| / ||g_b||)^2
 * (correctors.py:55-57 at batch size 1; no guard for a zero gradient norm, as there).  ALD and no corrector are per item anyway.
 * At equal padded frame count T', an item's result then depends on its y, its conditioning, its seed and the sampler alone: not
 * on its position in the batch, its companions, B, the sub-batch split, or graph versus eager.  Zero padding to another T'
 * changes what the network sees, so batches padded to different lengths are outside the guarantee.  At B > 1 this reproduces the
 * reference run per file (batch size 1), not the reference at batch size B.  (For this the per-item loop also makes the one
 * batch-size-dependent kernel choice of the network, conv_sk's tile form, from the per-image shape - DESIGN.md section 1.)
 * The update kernels are those of use_sample*, addressed as B items of F*T' elements instead of one item of all B*F*T'.
 * noise != NULL: injected draws in use_sample's layout (per item already).  Otherwise seeds_host: HOST array of B seeds, copied to
 * the seed array of the plan before the call returns and read there by the kernels, so captured graphs replay with new seeds.
 * Both NULL: USE_E_INVALID.  The per-item loop has its own captured graphs beside those of use_sample*; neither form drops the
 * other's, and "graph_captures" counts both. */
int use_sample_items(use_handle* h, const void* y, const void* cond, const void* cond2, const void* noise,
                     const uint64_t* seeds_host /* [B] */, void* out, use_stream_t stream);

/* Probability-flow ODE sampler (reference sampling/__init__.py:76-159 get_ode_sampler; model_wrapper.py:238-260): the ODE
 * dx = [theta (y - x) - g(t)^2 score / 2] dt integrated from T = 1 down to t_eps by scipy's RK45 (Dormand-Prince 5(4), scipy 1.15
 * rk.py / common.py, reproduced on the device), then, with `denoise`, one noise-free reverse-diffusion step at t_eps with dt = 1/N.
 * Each group of `group` consecutive items (0: the whole batch) has its own step-size controller and its own error norm (RMS over
 * the group's complex elements, as scipy's over its flattened vector); every item carries its own t into the network.  A finished
 * group is frozen: its items are still evaluated, their state does not change.  The float fields are taken at their shortest
 * decimal spelling (1e-5f -> 1e-5, 0.03f -> 0.03), so that they mean the Python floats the reference passes.
 * Per group: nfev = 2 + 6 x attempted steps (1 + 6 x ... with first_step), status 0 = reached t_eps, -1 = step below scipy's
 * min_step (the last accepted state is kept, as the reference keeps solution.y[:, -1]), -2 = max_nfe reached. */
typedef struct use_ode_config {
    float rtol, atol;      /* > 0, >= 0                                           sampling/__init__.py:82-83 */
    float t_eps;           /* end of the integration (3e-2)                                                 */
    int N;                 /* the denoise step's dt = 1/N                         model_wrapper.py:239-241   */
    int group;             /* items per step-size controller; 0 = the whole batch (ScoreModel minibatch)    */
    int denoise;           /* 1: one noise-free reverse-diffusion step at t_eps                             */
    float first_step, max_step; /* 0 = scipy's defaults (select_initial_step, inf)                          */
    int max_nfe;           /* evaluations per group before status -2; 0 = 10000                             */
    int use_graph;         /* 1: capture one RK45 step (6 evaluations + the stepper's kernels) as a hipGraph and replay it */
} use_ode_config;
enum { USE_ODE_FINISHED = 0, USE_ODE_TOO_SMALL_STEP = -1, USE_ODE_MAX_NFE = -2 };
/* Belongs to the plan like use_set_sampler (a new use_plan shape needs it again; a stale plan gives USE_E_STATE). */
int use_set_ode(use_handle* h, const use_ode_config* cfg);
/* prior (draw 0 of the Philox stream of `seed`, or noise = that one draw [B,1,F,T']) -> RK45 -> denoise -> out (complex64).
 * cond / cond2 as in use_sample_cond2.  nfev / status: HOST int arrays of n_groups = ceil(B / group) entries (may be null).
 * Synchronises the stream once per RK45 step (the "all groups done" word).  Stats: "ode_steps" (accepted steps, summed over the
 * groups), "ode_rejected", "ode_nfev_max" (what every item was evaluated: finished groups are evaluated until the last one ends). */
int use_sample_ode(use_handle* h, const void* y, const void* cond, const void* cond2, const void* noise, uint64_t seed, void* out,
                   int* nfev, int* status, use_stream_t stream);
/* The same RK45 stepper for callers with their own drift (reverse communication; the seam path of sampling.get_ode_sampler).
 * h: any handle (only its OUVE constants are used).  _start: y_sde = the SDE's y, x0 = the prior sample (complex64, n_per_item x B,
 * both copied).  _request: 1 = evaluate the drift at (x, t) - x complex64 [n], t float32 [B] (device) - and _supply it; 0 = every
 * group is done (synchronises the stream once per step).  _supply: kind 0 = f is the drift, 1 = f is the OUVE score at (x, t)
 * (the drift is formed on the device).  _result: out = complex64 of the solution, per-group nfev / status (host, may be null).
 * _state: per-group t, h_abs, nfev, status, accepted steps (host arrays, may be null; synchronises).  As scipy's solver object:
 * t and h_abs change only when a step is accepted (after status -1 or -2 they are the last accepted step's), and nfev counts the
 * evaluations supplied so far. */
typedef struct use_ode use_ode;
int use_ode_create(use_handle* h, int B, int64_t n_per_item, const use_ode_config* cfg, use_ode** out);
int use_ode_start(use_ode* o, const void* y_sde, const void* x0, use_stream_t stream);
int use_ode_request(use_ode* o, void* x, float* t, use_stream_t stream);
int use_ode_supply(use_ode* o, const void* f, int kind, use_stream_t stream);
int use_ode_result(use_ode* o, void* out, int* nfev, int* status, use_stream_t stream);
int use_ode_state(use_ode* o, double* t, double* h_abs, int* nfev, int* status, int* steps, use_stream_t stream);
int use_ode_num_groups(use_ode* o);
int use_ode_destroy(use_ode* o);

/* Element-wise SDE pieces for callers that drive the loop themselves through the reference's
 * Predictor / Corrector registries (uniform t over the batch). n = number of complex elements.
 * USE_E_INVALID (argument named in use_last_error(), nothing launched): a null handle; a null y / x or n < 1 in use_sde_prior; an unknown
 * predictor id, a null x / y / score / x_out or n < 1 in use_sde_predictor; a null x / score / x_out, n < 1, B < 1, n no multiple of B,
 * an unknown corrector id or (Langevin) B > 1024 in use_sde_corrector.  noise (NULL: drawn on the device from `seed`) and x_mean may be
 * null. */
int use_sde_prior(use_handle* h, const void* y, const void* noise, uint64_t seed, void* x, int64_t n, use_stream_t s);
int use_sde_predictor(use_handle* h, int predictor, float t, int N, const void* x, const void* y, const void* score,
                      const void* noise, uint64_t seed, void* x_out, void* x_mean, int64_t n, use_stream_t s);
int use_sde_corrector(use_handle* h, int corrector, float t, float snr, int B, const void* x, const void* score,
                      const void* noise, uint64_t seed, void* x_out, void* x_mean, int64_t n, use_stream_t s);

/* The device noise stream of use_sample(noise = NULL, seed), draw by draw: out[i] (complex64, n elements = the whole batch tensor
 * [B,1,F,T']) = the z that draw `draw` uses at element i -- draw 0 is the prior's randn_like (sdes.py:254), then per reverse step the
 * corrector draws (sampling/correctors.py:54) followed by the predictor draw (sampling/predictors.py:63), the reference's order of
 * consumption.  use_sample(noise = [use_fill_noise(seed, d) for d in 0..use_num_noise_draws-1]) is bit-identical to
 * use_sample(noise = NULL, seed): this is how the timed (device-noise) branch is pinned to the oracle in tests/.
 * The generator: (c0, c1, c2, c3) = Philox4x32-10(counter = (i low, i high, draw low, draw high), key = (seed low, seed high));
 * u1, u2 = ((float)(c0 >> 8) + 0.5f) 2^-24, ((float)(c1 >> 8) + 0.5f) 2^-24, both in (0, 1] (the + 0.5f rounds to even above 2^23, so 1.0
 * occurs); z = sqrt(-ln u1) (cos, sin)(2 pi u2) in float32 (Box-Muller at variance 1/2 per component). */
int use_fill_noise(use_handle* h, uint64_t seed, int draw, void* out, int64_t n, use_stream_t s);

/* The noise of use_sample_items, draw by draw: out (complex64, n elements = B items of n / B) = item b's z from seeds_host[b]
 * (HOST array, B <= 1024).  Item b equals use_fill_noise(seeds_host[b], draw) over n / B elements.  Needs no plan. */
int use_fill_noise_items(use_handle* h, const uint64_t* seeds_host /* [B] */, int B, int draw, void* out,
                         int64_t n /* complex elements, a multiple of B */, use_stream_t s);

/* Raw backbone output NCSNpp.forward(cat[x, y], t) (ncsnpp.py:324-501), i.e. without the sign flip of use_score.
 * x, y: complex64 [B,1,F,T'] device; y must be null when input_channels == 2 (the input is x alone), t must be null when
 * the handle is unconditional and may be null when it is conditional only if no_sigma_scale... (not supported: give t). */
int use_forward(use_handle* h, const void* x, const void* y, const float* t, void* out, use_stream_t stream);
/* use_forward with the kernel choice of the per-item sampler loop (use_sample_items): every form that use_forward picks from the size
 * of the whole (sub-)batch is picked from one image alone, so that item b's output has the bits use_forward gives that item in a batch
 * of one (own-length refine stage: a group of items of equal T' in one pass).  Same arguments, same plan. */
int use_forward_items(use_handle* h, const void* x, const void* y, const float* t, void* out, use_stream_t stream);

/* Spectrogram glue either side of the sampler, handle-free (ScoreModel.spec_fwd + pad_spec, model_wrapper.py:92-96,275-278,
 * util/other.py:128-135; ScoreModel.spec_back + crop, model_wrapper.py:98-103,320).  stft: complex64 [B,F,T] (torch.stft
 * output), Y / X: complex64 [B,1,F,Tpad].  fwd: Y = |S|^e e^{j arg S} * factor, zero for T <= t < Tpad; back: its inverse. */
int use_spec_fwd(const void* stft, void* Y, int B, int F, int T, int Tpad, float factor, float exponent, use_stream_t s);
int use_spec_back(const void* X, void* stft, int B, int F, int T, int Tpad, float factor, float exponent, use_stream_t s);

/* The transforms themselves on the device, fused with that glue: one kernel per direction, no intermediate
 * buffer.  use_stft_fwd = pad_spec(spec_fwd(torch.stft(wav, n_fft, hop, window, center=True, return_complex=True)))
 * (model_wrapper.py:116-118, 92-96, util/other.py:128-135); use_istft_back = torch.istft(spec_back(X), n_fft, hop, window,
 * center=True, length=L) over all Tpad frames (model_wrapper.py:98-103, 120-122, 320).  wav: float32 [B][L] device, window:
 * float32 [n_fft] device (periodic Hann in the reference's configs), Y / X: complex64 [B][1][n_fft/2+1][Tpad].  n_fft even
 * (1022 in SGMSE_Large.yaml - not a power of two: the transforms are table-driven direct sums, 10 GFLOP per batch of 8 x 4 s),
 * L > n_fft/2 (reflect padding), Tpad >= 1 + L / hop.  The first call per (device, n_fft) builds a twiddle table and
 * synchronises the stream once. */
int use_stft_fwd(const float* wav, void* Y, int B, int L, int n_fft, int hop, const float* window, int Tpad, float factor,
                 float exponent, use_stream_t s);
int use_istft_back(const void* X, float* wav, int B, int L, int n_fft, int hop, const float* window, int Tpad, float factor,
                   float exponent, use_stream_t s);

/* The same two transforms with one valid length per item (own-length sampling): wav float32 DEVICE [B][stride], item b valid for
 * len_host[b] samples (HOST ints, as in use_metrics; they travel as kernel arguments - no copy, no allocation, no synchronisation
 * beyond the first call's twiddle table).  use_stft_fwd_items analyses item b as if it were alone: reflect padding at its own end,
 * T_b = 1 + len[b] / hop frames written, frames T_b <= t < Tpad zero, samples of a row past len[b] never read.
 * use_istft_back_items: all Tpad frames of item b enter, samples m < len[b] are written, len[b] <= m < stride are written as zero.
 * Row b of either call has the bits of use_stft_fwd / use_istft_back called on that item alone with L = len[b] and the same Tpad
 * (same kernel body, same order of additions).  USE_E_INVALID (argument named in use_last_error(), nothing launched): a null
 * pointer, B < 1, odd n_fft, len[b] <= n_fft / 2, len[b] > stride, 1 + len[b] / hop > Tpad. */
int use_stft_fwd_items(const float* wav, int64_t stride, const int* len_host, void* Y, int B, int n_fft, int hop, const float* window,
                       int Tpad, float factor, float exponent, use_stream_t s);
int use_istft_back_items(const void* X, float* wav, int64_t stride, const int* len_host, int B, int n_fft, int hop,
                         const float* window, int Tpad, float factor, float exponent, use_stream_t s);

/* Chunked sampling of long recordings (no reference counterpart), handle-free: the frame axis of Y [B,1,F,Tp] (Tp the padded frame
 * count, a multiple of 64) is cut into n windows of C frames (C a positive multiple of 64) that start hop = C - overlap frames apart,
 * 0 <= overlap <= C / 2; the windows are the batch of use_plan / use_sample* at (B * n, C) - in groups of any size - and the
 * enhanced windows are cross-faded back in front of use_istft_back.  use_chunk_count (host only): n = 1 for Tp <= C (nothing to
 * cut), else ceil((Tp - overlap) / hop); USE_E_INVALID with the offending argument named in use_last_error() otherwise.
 * use_chunk_split: chunks [B * n,1,F,C], window k of item b in row b * n + k = Y[b, 0, :, k * hop : k * hop + C], zero past Tp.
 * use_chunk_merge: X [B,1,F,Tp]; the first `overlap` frames of window k >= 1 (j = 0 .. overlap - 1) are a_j * window k +
 * (1 - a_j) * window k - 1 with a_j = (j + 1) / (overlap + 1), every other frame is a copy from the one window that owns it;
 * one thread per output element, no atomics: deterministic.  Both are one launch on `s`, no synchronisation. */
int use_chunk_count(int Tp, int C, int overlap);
int use_chunk_split(const void* Y, void* chunks, int B, int F, int Tp, int C, int overlap, use_stream_t s);
int use_chunk_merge(const void* chunks, void* X, int B, int F, int Tp, int C, int overlap, use_stream_t s);

/* Evaluation metrics of an enhanced batch against its clean signals, handle-free (reference sgmse/util/other.py:15-62:
 * energy_ratios(s_hat, s, n) over si_sdr_components, and lsd(s_hat, s)).  est, clean, noise: float32 DEVICE [B][stride], item b valid for
 * len_host[b] samples (HOST ints; the rest of a row - the batch's zero padding, or anything else - is never read); noise = noisy - clean,
 * formed by the caller.  out_dev: fp64 DEVICE [B][USE_METRIC_COUNT].  SI-SDR / SI-SIR / SI-SAR = 10 log10(eps + |s_t|^2 / (eps + |e_n +
 * e_a|^2, |e_n|^2, |e_a|^2)) with s_t = alpha_s s, e_n = alpha_n n, e_a = s_hat - s_t - e_n, in two passes and fp64, as the reference
 * computes them; LSD = sqrt(mean |2 log(eps + |S_hat|) - 2 log(eps + |S|)|) over the 256 bins x (1 + len / 128) frames of the STFT with
 * n_fft 510, hop 128, periodic Hann, centred, reflect padding - the reference's sqrt(mean(abs(.))), not the textbook distance -
 * evaluated in fp64.  eps = 1e-10.  noise == NULL: LSD alone, the three ratios are NaN.  Every sum has a fixed order that depends on
 * len[b] alone: an item's four values are the same bits in any batch, at any stride, in every run (no atomics).
 * work: use_metrics_workspace(B, stride) bytes of device scratch, 8-byte aligned (0: bad arguments).  A handful of launches on `s`,
 * no synchronisation, no allocation.  USE_E_INVALID (argument named in use_last_error(), nothing launched): B < 1 or > 65535, stride < 1,
 * a null est / clean / len_host / work / out_dev, len[b] < 256 (reflect padding needs len > n_fft / 2 = 255) or > stride, work_bytes
 * too small. */
enum { USE_METRIC_SI_SDR = 0, USE_METRIC_SI_SIR = 1, USE_METRIC_SI_SAR = 2, USE_METRIC_LSD = 3, USE_METRIC_COUNT = 4 };
size_t use_metrics_workspace(int B, int stride);
int use_metrics(const float* est, const float* clean, const float* noise, const int* len_host, int B, int stride, void* work,
                size_t work_bytes, double* out_dev, use_stream_t s);

/* The hand-off between the two stages of the pipeline (SGMSE sampler, then the LSGAN refine generator), handle-free: what the two-run flow
 * does to a stage-1 waveform between the writer of SGMSEModule.predict_step and the batch the stage-2 loader builds, on the device.  in / out:
 * float32 DEVICE [B][stride] (out == in is allowed; any other overlap is not), item b valid for len_host[b] samples (HOST ints, as in
 * use_metrics and use_stft_fwd_items; they travel as kernel arguments).  For m < len[b], v is formed from in[b][m] in fp64:
 *   subtype USE_WAV_PCM16: q = nearbyint(x * 32767) clamped to [-32768, 32767] (what use_wav_write stores; a NaN is stored as 0), v = q / 32768
 *   (what use_load_utterance reads back); USE_WAV_FLOAT32: v = x;
 *   normalize != 0: mx = max |v| over the item by `fabs(v) > mx` (a NaN never becomes the peak), v = v / mx * 0.8 with two roundings (the
 *   loader's peak normalisation; a silent item gives NaN, as the loader and the reference do);
 * out[b][m] = (float)v, and out[b][m] = 0 for len[b] <= m < stride (the loader's zero padding).  Samples of `in` past len[b] are never read:
 * after stage 1 they hold whatever the iSTFT left in the padding.  peak_dev: fp64 DEVICE [B], receives mx in either mode.  Every output
 * sample has the bits the file round trip gives it, in every run, in any batch and at any stride (a maximum has no order; no atomics).
 * Row offsets b * stride are 64-bit.  work: use_wav_handoff_workspace(B, stride) bytes of device scratch, 8-byte aligned (0: bad arguments).
 * Two launches on `s` (+ one per 64 items for the lengths), no synchronisation, no allocation, nothing to zero between calls.
 * USE_E_INVALID (argument named in use_last_error(), nothing launched): B < 1 or > 65535, stride < 1, a null in / out / len_host / work /
 * peak_dev, len[b] < 1 or > stride, an unknown subtype, work_bytes too small. */
size_t use_wav_handoff_workspace(int B, int64_t stride);
int use_wav_handoff(const float* in, float* out, int64_t stride, const int* len_host, int B, int subtype /* USE_WAV_PCM16 | USE_WAV_FLOAT32 */,
                    int normalize, void* work, size_t work_bytes, double* peak_dev, use_stream_t s);

/* The hand-off for files of several channels (data.channels=all): the rows of in / out are the channels of F files one after another, file f
 * holding ch_host[f] rows (1 ... 64) of len_host[f] valid samples each (HOST ints, one entry per FILE).  Every sample goes through the
 * arithmetic of use_wav_handoff; with normalize, mx is taken over all rows of a file - one gain per file, as the loader gives a file of
 * several channels - and a silent channel of a file that is not silent stays exact zeros.  peak_dev: fp64 DEVICE [F], one peak per file.
 * With F = 1 and ch = 1 the call is use_wav_handoff's, bit for bit.  work: use_wav_handoff_files_workspace(rows, stride) bytes for rows =
 * the sum of ch_host, 8-byte aligned (0: bad arguments).  The same launches, guarantees and refusals as use_wav_handoff; also refused:
 * a null ch_host, ch[f] < 1 or > 64, more than 65535 rows in all. */
size_t use_wav_handoff_files_workspace(int rows, int64_t stride);
int use_wav_handoff_files(const float* in, float* out, int64_t stride, const int* len_host, const int* ch_host, int F,
                          int subtype /* USE_WAV_PCM16 | USE_WAV_FLOAT32 */, int normalize, void* work, size_t work_bytes, double* peak_dev,
                          use_stream_t s);

/* The convergence part of the refine stage's generator criterion, forward only and handle-free (reference
 * loss_function/monaural_loss.py:59-178, WavSpecConvergence_Loss; the same arithmetic inside WavSpecConvergence_HIFIGAN_Vocoder_G_Loss, which
 * LSGAN.yaml selects).  est, clean: float32 DEVICE [B][stride], item b valid for len_host[b] samples (HOST ints, as in use_metrics; the rest of a
 * row is never read).  out_dev: fp64 DEVICE [B][USE_SPECLOSS_COUNT], per item and unweighted - the reference's values at batch size 1 on exactly
 * those samples:
 *   [USE_SPECLOSS_WAV_L1]        mean |e - c|
 *   [USE_SPECLOSS_MAG_L2 + r]    l2_r   = mean (Me - Mc)^2
 *   [USE_SPECLOSS_MAG_LOG + r]   log_r  = mean |log(32768 Me + 1e-6) - log(32768 Mc + 1e-6)|
 *   [USE_SPECLOSS_MAG_NORM + r]  norm_r = sqrt(sum (Mc - Me)^2) / (sqrt(sum Mc^2) + 1e-6)
 *   [USE_SPECLOSS_MEL_LOG], [USE_SPECLOSS_MEL_L2]   the log and l2 formulas on the mel maps
 * r = 0..3 in ascending n_fft: Me, Mc the magnitude Spectrograms with n_fft = int(512 q), int(1024 q), int(2048 q), int(4096 q), q =
 * sampling_rate / 48000 (256 ... 2048 at 24 kHz, 512 ... 4096 at 48 kHz), win_length n_fft, hop n_fft / 4, periodic Hann, power 1, centred,
 * reflect padding, one-sided, not normalised: n_fft / 2 + 1 bins x (1 + len / hop) frames.  Mel maps: the MelSpectrogram with n_fft 2048,
 * win_length int(0.025 sr) (periodic Hann, centred in the frame with zeros either side), hop int(0.010 sr), power 1, 128 HTK bands from 0 to
 * sr / 2, norm None (torchaudio's melscale_fbanks: triangles between 130 points equally spaced in mel, over linspace(0, sr / 2, 1025)).
 * The reference's six terms are wav_l1, mag_l2 = sum_r l2_r (a sum, not a mean), mag_log = mean_r log_r, mag_norm_l2 = mean_r norm_r, mel_log,
 * mel_l2; their weighting (alpha_*) and the mean over a batch are the caller's (universal_speech_enhancement_amd/losses.py).
 * Precision: float32 samples in; window, transform (a real FFT per frame), magnitude, log, filter bank, products and sums in fp64 - the
 * float64 evaluation of the reference's formulas.  est == clean gives exactly 0 in all 15.  Every sum has a fixed order that depends on len[b]
 * alone: an item's 15 values are the same bits in any batch, at any stride, in every run (no atomics).  Row offsets b * stride are 64-bit.
 * work: use_spec_losses_workspace(B, stride, sampling_rate) bytes of device scratch, 8-byte aligned (0: bad arguments).  Eight launches on `s`
 * (+ one per 64 items for the lengths), no synchronisation, no allocation, nothing to zero between calls.  USE_E_INVALID (argument named in
 * use_last_error(), nothing launched): a sampling_rate other than 24000 / 48000 (the rates at which all four frame lengths are powers of two),
 * B < 1 or > 65535, stride < 1, a null est / clean / len_host / work / out_dev, len[b] <= n_max / 2 (reflect padding; the minimum is 1025 at
 * 24 kHz, 2049 at 48 kHz) or > stride, work_bytes too small. */
enum { USE_SPECLOSS_WAV_L1 = 0, USE_SPECLOSS_MAG_L2 = 1, USE_SPECLOSS_MAG_LOG = 5, USE_SPECLOSS_MAG_NORM = 9,
       USE_SPECLOSS_MEL_LOG = 13, USE_SPECLOSS_MEL_L2 = 14, USE_SPECLOSS_COUNT = 15 };
size_t use_spec_losses_workspace(int B, int64_t stride, int sampling_rate);
int use_spec_losses(const float* est, const float* clean, const int* len_host, int B, int64_t stride, int sampling_rate,
                    void* work, size_t work_bytes, double* out_dev, use_stream_t s);

/* Short-time objective intelligibility of an enhanced batch against its clean signals, handle-free: STOI (Taal et al. 2011) and ESTOI (Jensen &
 * Taal 2016) as pystoi.stoi(clean, est, sampling_rate, extended) defines them - with SI-SDR (use_metrics) what the reference's validation loop
 * reports (sgmse/util/inference.py: evaluate_model).  est, clean: float32 DEVICE [B][stride], item b valid for len_host[b] samples (HOST ints, as
 * in use_metrics; the rest of a row is never read).  out_dev: fp64 DEVICE [B][USE_STOI_COUNT]: the two scores and T, the number of STFT frames
 * they were taken over.  Per item:
 *   1. both signals to 10 kHz: y[n] = sum_j x[j] h'[L + n q - j p], n < ceil(len p / q), p / q = 10000 / sampling_rate, x zero past both ends;
 *      h' = p h / sum h, h = kaiser(2 L + 1, 0.1102 (60 - 8.7)) 2 p fc sinc(2 fc t), fc = 1 / (2 max(p, q)), L = ceil(52 / (2.8714 fc)), t = -L..L
 *      (scipy.signal.resample_poly(x, p, q, window = h / sum h); 871 taps at 24 kHz).  10 kHz in: no filter.
 *   2. frames of 256 at hop 128 under w = np.hanning(258)[1:-1]; frame k is kept iff max(E) - 40 - E_k < 0, E_k = 20 log10(|w clean_k| + 2^-52);
 *      both signals are rebuilt by overlap-add of their own windowed kept frames (K kept frames: (K - 1) 128 + 256 samples).
 *   3. T = K - 1 frames (start 128 i, i < K - 1) times w again, zero-padded to 512, |rfft|^2; 15 third-octave bands from 150 Hz:
 *      tob[b][t] = sqrt(sum of bins [lo_b, hi_b)), edges 7 9 11 14 17 22 27 34 43 55 69 87 109 138 174 219.
 *   4. segments m = 0 .. T - 30 of 30 frames.  STOI: per band row c = |x| / (|y| + eps), y' = min(c y, x (1 + 10^(15/20))), row means removed,
 *      rows divided by (|.| + eps), d = sum x y' / (15 (T - 29)).  ESTOI: rows, then columns, freed of their mean and scaled to unit norm,
 *      d = sum x_n y_n / (30 (T - 29)).  eps = 2^-52.  T < 30: both scores are 1e-5 (pystoi's value).
 * Two departures from pystoi: ESTOI's eps * randn dither is left out, and a row or column whose sum of squares is exactly 0 is scaled by 0 (the
 * dither's expectation) instead of 1 / 0 - exact zeros in est cannot turn a score into NaN.
 * Precision: float32 samples in, everything after the load in fp64 (taps by Kaiser's I0 power series to convergence).  Every sum has a fixed
 * order that depends on len[b] and the item's own data alone: an item's three values are the same bits in any batch, at any stride, in every
 * run (no atomics; the kept frames are compacted by an integer scan and gathered, never scattered).  Row offsets b * stride are 64-bit.
 * work: use_stoi_workspace(B, stride, sampling_rate) bytes of device scratch, 8-byte aligned (0: bad arguments).  Seven launches on `s` (+ one
 * per 64 items for the lengths), no synchronisation, no allocation, nothing to zero between calls: K stays on the device, the grids are sized
 * for no frame removed.  USE_E_INVALID (argument named in use_last_error(), nothing launched): a sampling_rate other than 10000 / 16000 /
 * 24000 / 48000, B < 1 or > 65535, stride < 1, a null est / clean / len_host / work / out_dev, len[b] > stride, a len[b] whose resampled
 * length ceil(len p / q) is under 256 (the minimum is 613 at 24 kHz), work_bytes too small. */
enum { USE_STOI_STOI = 0, USE_STOI_ESTOI = 1, USE_STOI_FRAMES = 2, USE_STOI_COUNT = 3 };
size_t use_stoi_workspace(int B, int64_t stride, int sampling_rate);
int use_stoi(const float* est, const float* clean, const int* len_host, int B, int64_t stride, int sampling_rate,
             void* work, size_t work_bytes, double* out_dev, use_stream_t s);

/* The degradation simulator of the training data, handle-free: what the reference's comm_distort_simu_dataset.__getitem__ does to a clean
 * excerpt, per item of a batch on the device, for the stages named below (the others - EQ, STFT masks, codecs, ... - are not built).
 * clean: float32 DEVICE [B][stride], item b valid for len_host[b] samples.  noise: float32 DEVICE [B][noise_stride] or null; the row of an
 * item with add_noise holds noise_len_host[b] >= len[b] samples, of which the first len[b] are read.  rir: float32 DEVICE [B][rir_stride] or
 * null; an item with reverb reads rir_len taps, already trimmed to start at the peak and divided by it (get_rir; the host's work).  packet:
 * fp64 DEVICE [packet_count] factors or null; an item with packet_frame > 0 reads ceil(len / packet_frame) of them from packet_off.  params: HOST [B] records;
 * the host draws every parameter, the device draws nothing.  Per item, in fp64 after the load, each stage optional:
 *   1. reverb    full = (x * rir)[:len] (the noisy branch), early = (x * rir[:6])[:len] (the clean target).  early is a direct sum; full
 *                is an FFT convolution at M = pow2 >= len + rir_len - 1: the transforms of x and of rir, their product, one inverse FFT.
 *   2. add_noise P(w) = mean of w^2 over the samples librosa.effects.split(w, top_db = 50) keeps: frame RMS over 2048 samples at hop 512,
 *                centred and zero-padded, 1 + len / 512 frames; frame k is kept iff 10 log10(max(1e-10, p_k)) - 10 log10(max(1e-10, max p))
 *                > -50; sample s is kept iff frame s / 512 is.  scale = sqrt(P(clean) / (P(noise) + 1e-8) / snr_lin + 1e-8),
 *                noisy = clean + scale * noise (clean: the full-reverb signal).  snr_lin = 10^(snr / 10).
 *   3. loudness  n_loud intervals of len / n_loud samples, interval i times loud[i]; the tail is left as it is.
 *   4. clip      USE_CLIP_HARD: clip(x, -clip_a, clip_a).  USE_CLIP_HARD_ON_RATE: numpy's 1000-bin histogram of |x| over [min, max]; the
 *                threshold is the first left edge whose cumulative count exceeds (1 - clip_a) len.  USE_CLIP_SOFT: m x / (|m|^p + |x|^p +
 *                1e-5)^(1 / p), m the signed maximum, p = clip_a.  USE_CLIP_SIGMOID1: (2 / (1 + exp(-clip_a x)) - 1) clip_b.
 *                USE_CLIP_SIGMOID2: c = clip(x, -clip_a, clip_a), b = 1.5 c - 0.3 c^2, clip_b (2 / (1 + exp(-(b > 0 ? 4 : 0.5) b)) - 1).  Both
 *                sigmoids times sqrt(mean x^2) / (sqrt(mean y^2) + 1e-8).  USE_CLIP_SOX and USE_CLIP_PEDAL are refused: not built.
 *   5. dc        x + dc_offset.
 *   6. packets   frame j of packet_frame samples (the last may be short) times packet[packet_off + j].
 *   7. volume    USE_VOLUME_PEAK: both signals times volume_target / (max(peak_noisy, peak_clean) + 1e-6); USE_VOLUME_RMS: the level is
 *                sqrt(P(.) + 1e-8) with stage 2's P.  Then both times 0.99 / peak iff the peak exceeds 0.99 (volume_clip_dual).  normalize:
 *                both / max(peak_noisy, peak_clean) * 0.8, two roundings.
 * perturbed, clean_out: DEVICE [B][stride] of float32 (out_fp64 = 0) or fp64 (1); the float32 value is the cast of the fp64 one, and both
 * rows are zero from len[b] to stride.  scalars_dev: fp64 DEVICE [B][USE_DISTORT_SCALARS].  keep_dev: null, or uint8 DEVICE [B][2][keep_stride],
 * keep_stride >= 1 + len / 512: the kept frames of stage 2 (clean, then noise), written for the items with add_noise.
 * Every product and sum above is rounded once (no contraction), every reduction has a place fixed by len and rir_len alone: partials by
 * plain store, re-reduced in a fixed order by one workgroup; the histogram counts are integers.  An item's rows and scalars are the same
 * bits alone, at any row of any batch, at any stride, in every run.  The items run one after another on `s` and share only the workspace:
 * use_distort_workspace(len, rir_len) bytes for the largest item (rir_len = 0: no reverb; 0: bad arguments), 16-byte aligned.  No
 * synchronisation, no allocation.  USE_E_INVALID (argument named, nothing launched): a null clean / len_host / params / perturbed / clean_out
 * / scalars_dev / work, B outside 1 ... 65535, len[b] < 1 or > stride, reverb with a null rir, rir_len < 1 or > rir_stride or len + rir_len
 * - 1 > 2^24, add_noise with a null noise or noise_len[b] < len[b] or > noise_stride, an unknown or unbuilt clip_kind, a rate outside
 * (0, 1], n_loud outside 0 ... 5, packet_frame < 0 (the stage is off at 0), a null packet or frames outside packet_count, an unknown volume mode, a non-finite
 * parameter, a short workspace or keep_stride. */
enum { USE_CLIP_NONE = 0, USE_CLIP_HARD = 1, USE_CLIP_HARD_ON_RATE = 2, USE_CLIP_SOFT = 3, USE_CLIP_SIGMOID1 = 4, USE_CLIP_SIGMOID2 = 5,
       USE_CLIP_SOX = 6, USE_CLIP_PEDAL = 7 };
enum { USE_VOLUME_NONE = 0, USE_VOLUME_PEAK = 1, USE_VOLUME_RMS = 2 };
enum { USE_DISTORT_NOISE_SCALE = 0, USE_DISTORT_CLIP_THRESHOLD = 1, USE_DISTORT_VOLUME_SCALE = 2, USE_DISTORT_NORM_FACTOR = 3,
       USE_DISTORT_CLIP_SCALE = 4, USE_DISTORT_P_CLEAN = 5, USE_DISTORT_P_NOISE = 6, USE_DISTORT_ENERGY_SCALE = 7, USE_DISTORT_SCALARS = 8 };
typedef struct use_distort_params {
    int reverb, rir_len;          /* stage 1 */
    int add_noise;                /* stage 2 */
    int n_loud;                   /* stage 3: 0 (off) ... 5 */
    int clip_kind;                /* stage 4: USE_CLIP_* */
    int dc;                       /* stage 5 */
    int packet_frame;             /* stage 6: 0 (off), or the frame size in samples */
    int volume, normalize;        /* stage 7: USE_VOLUME_*; output_normalize */
    int reserved;
    long long packet_off;
    double snr_lin, loud[5], clip_a, clip_b, dc_offset, volume_target;
} use_distort_params;
size_t use_distort_workspace(int64_t len, int64_t rir_len);
int use_distort(const float* clean, const float* noise, const float* rir, const double* packet, int64_t packet_count, const int* len_host,
                const int* noise_len_host, const use_distort_params* params, int B, int64_t stride, int64_t noise_stride,
                int64_t rir_stride, int out_fp64, void* perturbed, void* clean_out, double* scalars_dev, unsigned char* keep_dev,
                int64_t keep_stride, void* work, size_t work_bytes, use_stream_t s);

/* Counters of a handle: "graph_captures" (segments of the sampling loop captured so far), "plans_built", "plan_cache_hits", "ode_steps",
 * "ode_rejected", "ode_nfev_max" (of the last use_sample_ode),
 * "plans_parked", "plan_stale" (1: use_set_option was called since use_plan - the evaluation entry points will refuse the plan).  A handle keeps the plans - workspace, state, time-embedding tables, captured graphs - of the most recently used
 * (B, T') shapes (use_set_option("plan_cache", k), default 4 besides the current one): use_plan of a parked shape costs nothing and
 * its graphs replay as they are. */
int use_get_stat(use_handle* h, const char* name, long long* value);
/* Introspection for tests / profiling */
/* One eager score evaluation with a HIP-event pair around every launch of the dominant kernel (conv_wide_kernel, the
 * wide-tile implicit-GEMM 3x3 convolution of the large feature maps): summed kernel time, their algorithmic FLOPs and
 * algorithmic HBM bytes (every operand once), launch count, and the wall time of the whole evaluation on `stream`.
 * Synchronises the stream. */
int use_profile_score(use_handle* h, const void* x, const void* y, const float* t, void* out, use_stream_t stream,
                      double* conv_ms, double* conv_flops, double* conv_bytes, int* conv_launches, double* total_ms);
/* The HBM-bound kernels of the same evaluation (FIR x2 resampling of the activation maps, pyramid-head convolutions, the input
 * convolution), one record per launch in launch order: kernel class ("fir_up", "fir_down", "pyr_conv", "conv_in"), the map it read
 * (H x W per item of the sub-batch), its algorithmic HBM bytes (every operand once) and its duration between HIP events.  Returns 0,
 * 1 when `index` is past the last record of the most recent use_profile_score, negative on error. */
int use_profile_aux(use_handle* h, int index, char* name, int name_cap, int* H, int* W, double* bytes, double* ms);
/* ... the same list also carries the MFMA-bound kernels beside the dominant one ("conv_v2": 3x3 convolutions of the middle maps,
 * "conv_sk": the smallest maps): their algorithmic FLOPs (0 for the HBM-bound classes). */
int use_profile_aux_flops(use_handle* h, int index, double* flops);
/* Single-convolution harness for kernel bring-up and same-box A/B timing (no reference counterpart): builds one fused
 * implicit-GEMM 3x3 convolution (optional second channel-concat source C1, GroupNorm affine + SiLU on the input, bias +
 * time-embedding bias, fused 1x1 shortcut over XC0+XC1 channels, residual, GroupNorm partial sums) on deterministic
 * pseudo-random device data, runs it `iters` times through the chosen kernel (variant 0: the library's dispatcher, 2 / 4 / 5:
 * conv_v2 / conv_v4 / conv_v5) and returns the average launch time, the algorithmic FLOPs, the output as float32
 * [B][H][W][Cout] (host, may be null) and the per-(item, channel) (sum, sum of squares) totals [B][Cout][2] (host, may be null). */
typedef struct use_conv_case {
    int B, H, W, C0, C1, Cout, XC0, XC1;
    int act, gn, temb, res, stats;   /* flags */
    int dtype;                       /* 0 fp32, 1 bf16, 2 fp16 (storage) */
    int variant, iters;
} use_conv_case;
int use_conv_bench(const use_conv_case* c, float* out_host, float* stats_host, double* ms_avg, double* flops);
/* ---- single operators of the path on caller-owned device tensors (NHWC: [B][H][W][C], C contiguous) with host fp32 weights.
 * Test / bring-up surface: the per-operator golden vectors of the reference reach the HIP kernels through these.
 * use_op_conv: out = ((conv3x3|1x1(act(a x + b)) + conv1x1(x0|x1) + bias + temb[b]) + res) * out_scale, exactly the fused operator of the
 *   res-block (ResnetBlockBigGANpp, layerspp.py:282-314); channel counts are multiples of 32 (zero-pad smaller ones; the one exception
 *   is the network's input convolution, below); `w` is the
 *   reference's [Cout][Cin][3][3] (ntaps 9) or [Cout][Cin] (ntaps 1) tensor, `w2` [Cout][XC]; coef = GroupNorm folded to (a, b) per
 *   (item, channel) or null; stats (zeroed by the caller) receives the fixed-point GroupNorm totals of the output.  variant: 0 = the
 *   library's dispatcher, 1 generic, 2 conv_v2, 4 conv_v4, 5 conv_v5, 7 conv_sk; a forced variant that cannot run the case returns
 *   USE_E_INVALID naming the violated condition.  Synchronises the stream.
 *   Trailing fields (zero: off): pyr / w4 / b4 add the Combine 1x1 over a 4-channel fp32 map after the out_scale (the order of
 *   ConvArgs: out = ((conv + shortcut + bias + temb) + res) * out_scale + (pyr . w4 + b4)); gn_st0 (with coef null) makes the kernel
 *   finalise GroupNorm(gn_groups, eps gn_eps) of concat(src0, src1) itself from the totals its producers accumulated, with the affine
 *   gn_gamma / gn_beta, as the engine does on the small maps; temb_bstride is the distance between temb's rows (0: Cout, -1: shared).
 *   stats_part / stats_parts: the GroupNorm totals as per-workgroup partial totals [B][stats_parts][Cout][2], written with plain stores
 *   (the caller need not zero them) in place of the atomics on `stats`, as the engine's large maps run; stats_parts must be what
 *   use_conv_choice answers for the same op under the same options (> 0), `stats` must be null, and a forced variant whose kernel only
 *   knows atomics refuses (USE_E_INVALID, nothing is launched).  Summed over the parts they are the integers `stats` would hold.
 *   The network's input convolution as the engine issues it also runs here (variant 0 or 1): dtype fp32, ntaps 9, C0 = 4 (or 8: the
 *   6-channel input, two zero channels), no second source, no shortcut, nothing fused in front or behind (bias, out_scale and the totals
 *   only), Cout a multiple of 8 (above 32 with C0 = 8); `w` is [Cout][C0][3][3].  With 16-bit output, C0 = 4 and Cout above 32 it runs
 *   on the engine's split-bf16 weight copy (conv_in_split), else on the fp32 weights (conv_in; C0 = 8: conv_generic).  Variants 2 / 4 /
 *   5 / 7 refuse it as they refuse any case their kernel cannot run.
 * use_op_fir: upsample_2d / downsample_2d with the [1,3,3,1] kernel (up_or_down_sampling.py:202-264); out_act = FIR(act(a x + b)),
 *   out_raw = FIR(x) (either may be null).
 * use_op_attention: softmax(q k^T / sqrt(C)) v per item (AttnBlockpp core, layerspp.py:84-88), q/k/v/out [B][N][C].
 * use_op_attention_gemm: the same core in the form the engine runs above 512 tokens (N = H W; the refine generator's 64x80 bottleneck): vt =
 *   v^T, per item the scores as a 1x1 convolution of q whose weights are the item's keys (out_scale C^-0.5, no bias), the softmax over all
 *   B N rows in place, per item a second 1x1 convolution of the probabilities whose weights are the item's vt; 2 + 2 B launches on `stream`,
 *   no synchronisation.  Scores and probabilities are stored in `dtype` between the launches.  The workspace (16-byte aligned,
 *   use_op_attention_gemm_workspace bytes; 0 for a shape the form does not run) holds, in `dtype`, the probabilities [B][N][N] at offset 0
 *   and vt [B][C][N] at the next multiple of 256 bytes behind them: both can be read back after a synchronise.  USE_E_INVALID (nothing is
 *   launched): a shape outside N > 512, N % 128 == 0, C % 128 == 0 (what the engine tests before it takes this form), a workspace too
 *   small, an unknown dtype, a null pointer.
 * use_op_gn_finalize: GroupNorm totals (as accumulated in `stats`) of up to two concatenated sources -> coef[b][c] = (a, b).
 * use_op_gn_finalize_parts: the same with either form per source: totals st_i [B][C_i][2] (nt_i = 0), or nt_i > 0 per-workgroup partial
 *   totals pt_i [B][nt_i][C_i][2] (use_conv_op::stats_part) - integer sums, so the coefficients are those of the summed totals bit for
 *   bit.  USE_E_INVALID (nothing is launched): both or neither form for a source, groups not dividing C0 + C1, a null pointer.
 * use_op_fir and use_op_attention return USE_E_INVALID (nothing is launched) for an unknown dtype, for C that is not a whole number of
 *   16-byte channel chunks (FIR: C % 8 in 16 bit, C % 4 in fp32) and for a row that does not fit the LDS (attention: (C + N) * 4 bytes).
 * The remaining kernels of one score evaluation, one launch each on `stream`, argument check in front, no synchronisation:
 * use_op_attn_block: the fused AttnBlockpp (layerspp.py:77-93) out = (x + NIN_3(softmax(q k^T / sqrt(C)) v)) / sqrt(2), q / k / v =
 *   NIN_0..2(GroupNorm(x)); x / out [B][N][C] in a 16-bit `dtype`, C = 256, N <= 96 (anything else: USE_E_INVALID); gn_st = the
 *   fixed-point totals of x ([B][C][2], as `stats` accumulates them); the four NIN matrices are DEVICE tensors in `dtype`, [Cout][Cin]
 *   (the transpose of the reference's NIN.W), the four biases device fp32; stats (zeroed by the caller, or null) receives the totals of out.
 * use_op_combine_add: Combine 'sum' of an 8-channel fp32 pyramid (layerspp.py:50-55) in place, h[b,p,:] += b8 + w8 . pyr[b,p,:] with
 *   w8 [C][8], and the totals of the stored h into stats (zeroed by the caller, required); C <= 512, a multiple of the chunk.
 * use_op_temb_mlp: t[b * t_stride] -> silu(Linear_2(silu(Linear_1(fourier(log t))))) [B][4 nf] (layerspp.py:37-39, ncsnpp.py:351-368;
 *   the res-blocks consume act(temb)); use_op_temb_dense: out[b][r] = bias[r] + W[r] . silu_temb[b], every Dense_0 row at once.
 * use_op_score_out: score[b,p] = sign * (bias + w . pyr[b,p,:] / t[b * t_stride]) as complex64 (ncsnpp.py:492-500; t null: no division;
 *   pc = 4 or 8 pyramid channels, w [2][pc]).  use_op_pack_input: x4[p] = 2 (x, y[, y2]) - 1 (ncsnpp.py:333-347, 372-374; y null: 0).
 * use_op_softmax_rows: in place over the last axis of [rows][cols]; use_op_transpose_nc: [B][N][C] -> [B][C][N] (the long-sequence
 *   attention path's helpers). */
typedef struct use_conv_op {
    int B, H, W, C0, C1, Cout, XC0, XC1, ntaps, act, dtype, out_dtype, variant;
    const void *src0, *src1;
    const float* coef;
    const float* w;
    const float* bias;
    const float* temb;
    const void *x0, *x1;
    const float* w2;
    const void* res;
    float out_scale;
    void* out;
    long long* stats;
    /* optional trailing fields: zero = off (the behaviour before they existed) */
    const float* pyr;                     /* device fp32 [B][H][W][4] or null: + pyr . w4[co] + b4[co] (Combine 'sum', layerspp.py:50-55) */
    const float* w4;                      /* host fp32 [Cout][4] */
    const float* b4;                      /* host fp32 [Cout] or null */
    const long long *gn_st0, *gn_st1;     /* coef == null and gn_st0 set: GroupNorm finalised in the kernel from the sources' totals */
    const float *gn_gamma, *gn_beta;      /*   (device [B][C0][2], [B][C1][2] as `stats` accumulates them) and the affine (device [C0+C1]) */
    int gn_groups;                        /*   groups over C0+C1 channels */
    float gn_eps;
    int temb_bstride;                     /* elements between temb's batch rows: 0 = Cout, -1 = one row shared by the batch */
    long long* stats_part;                /* device [B][stats_parts][Cout][2] or null: per-workgroup partial totals in place of `stats` */
    int stats_parts;                      /*   the count use_conv_choice answers for this op */
} use_conv_op;
int use_op_conv(const use_conv_op* c, use_stream_t stream);
/* use_conv_choice: which kernel the library's dispatcher (variant 0) would run this op on under the current options, without running
 *   it (host only: no HIP call; the channel counts are validated as use_op_conv validates them, the variant field is ignored).  For
 *   the network's input convolution (dtype fp32, ntaps 9, C0 = 4 or 8, no second source and no shortcut) it answers for any flags and
 *   Cout, with the engine's split-bf16 weight copy where the engine keeps one; use_op_conv runs the form the engine issues.  name receives one of
 *   "conv_sk", "conv_v4", "conv_v5", "conv_v2", "pyr_conv", "pyr_conv_ws", "conv_in", "conv_in_split", "conv_generic"; stats_parts the
 *   per-workgroup partial GroupNorm totals per (item, channel) that kernel can write in place of atomics (0: it only knows atomics).
 *   Either may be null. */
int use_conv_choice(const use_conv_op* c, char* name, int name_cap, int* stats_parts);
/* use_op_conv_dev: the same operator for the training path (reference SGMSE_module.py:46-54 -> model_wrapper.py:147-208, where the
 *   parameters are nn.Parameters on the device and change every optimiser step): c->w / c->bias are DEVICE fp32 tensors, laid out for
 *   the kernels by a kernel on `stream` into the caller's workspace (use_op_conv_dev_workspace(c) bytes); no allocation, no
 *   synchronisation, no fused shortcut (XC0 = XC1 = 0).  w_mode: 0 = conv weight [Cout][Cin][taps]; 1 = data gradient of the conv whose
 *   weight is c->w [Cin][Cout][taps] (the kernel sees w'[co][ci][tap] = w[ci][co][taps-1-tap]); 2 = NIN matrix [Cin][Cout] (ntaps 1). */
size_t use_op_conv_dev_workspace(const use_conv_op* c);
int use_op_conv_dev(const use_conv_op* c, int w_mode, void* work, size_t work_bytes, use_stream_t stream);
int use_op_fir(const void* src, int dtype, const float* coef, int act, void* out_act, void* out_raw, int B, int H, int W, int C, int up,
               use_stream_t stream);
int use_op_attention(const void* q, const void* k, const void* v, void* out, int dtype, int B, int N, int C, use_stream_t stream);
size_t use_op_attention_gemm_workspace(int dtype, int B, int N, int C);
int use_op_attention_gemm(const void* q, const void* k, const void* v, void* out, void* work, size_t work_bytes, int dtype, int B, int H, int W,
                          int C, use_stream_t stream);
int use_op_gn_finalize(const long long* st0, int C0, const long long* st1, int C1, const float* gamma, const float* beta, int groups,
                       int hw, float eps, float* coef, int B, use_stream_t stream);
int use_op_gn_finalize_parts(const long long* st0, const long long* pt0, int nt0, int C0, const long long* st1, const long long* pt1, int nt1,
                             int C1, const float* gamma, const float* beta, int groups, int hw, float eps, float* coef, int B,
                             use_stream_t stream);
int use_op_attn_block(const void* x, const long long* gn_st, const float* gamma, const float* beta, int groups, float eps, const void* wq,
                      const void* wk, const void* wv, const void* wo, const float* bq, const float* bk, const float* bv, const float* bo,
                      void* out, long long* stats, int dtype, int B, int N, int C, use_stream_t stream);
int use_op_combine_add(void* h, int dtype, const float* pyr, const float* w8, const float* b8, long long* stats, int B, int64_t pix_per_b, int C,
                       use_stream_t stream);
int use_op_temb_mlp(const float* t, int t_stride, const float* gfp_w, const float* w1, const float* b1, const float* w2, const float* b2,
                    float* out_silu, int B, int nf, use_stream_t stream);
int use_op_temb_dense(const float* silu_temb, const float* W, const float* bias, float* out, int B, int rows, int dim, use_stream_t stream);
int use_op_score_out(const float* pyr, int pc, const float* t, int t_stride, const float* w, const float* bias, void* score, int B,
                     int64_t pix_per_b, float sign, use_stream_t stream);
int use_op_pack_input(const void* x, const void* y, const void* y2, float* x4, int64_t npix, use_stream_t stream);
int use_op_softmax_rows(void* x, int dtype, int64_t rows, int cols, use_stream_t stream);
int use_op_transpose_nc(const void* in, void* out, int dtype, int B, int N, int C, use_stream_t stream);
/* ---- backward operators of one res-block (minimum slice of ScoreModel.train_step's gradients, reference
 * model_wrapper.py:147-208 / SGMSE_module.py:46-54).  NHWC device tensors; activations and their gradients in `dtype` (0 fp32 /
 * 1 bf16 / 2 fp16 storage: mixed-precision training keeps fp32 parameters, statistics and parameter gradients) where a dtype
 * argument is present, fp32 elsewhere.  The data gradient of a convolution is use_op_conv
 * itself on the flipped, transposed weights; these are the rest:
 * use_op_wgrad:      dW[co][ci][tap] = alpha * sum dY[b,p,co] X[b,p+tap,ci] (reference weight layout), db[co] = alpha * sum dY (or null).
 *                    work: use_op_wgrad_workspace(...) floats of scratch for the tiled kernel (per-slice partial tiles, summed without
 *                    atomics), or null for the small-tile kernel with atomic accumulation.
 * use_op_gn_act_bwd: gradient of act(GroupNorm(groups, eps)(x)) (act: 0 none, 1 SiLU) against dy: dx (+ add_scale * add when add is
 *                    given), dgamma, dbeta; `work`: use_op_gn_workspace(B, C, groups) floats of scratch, 8-byte aligned; have_stats != 0:
 *                    `work` is the workspace use_op_gn_act_fwd ran in for the same x, whose statistics are reused.
 * use_op_gn_act_fwd: y = act(GroupNorm(x)) (the operand of the following convolution's weight gradient, recomputed); same workspace.
 * use_op_colsum:     out[b][c] = scale * sum_p x[b,p,c] (fp32 out; the gradient reaching Dense_0's output); work: 128 B C floats of
 *                    scratch (8-byte aligned) for the pixel-sliced kernel, or null (fp32 input only: one workgroup per 64 channels).
 * use_op_dense_bwd:  Dense_0(SiLU(temb)): g [B][Cout] -> dW [Cout][K], db [Cout], dtemb [B][K].
 * Refusals (USE_E_INVALID, nothing launched): B, K or Cout < 1 in use_op_dense_bwd; B, HW or C < 1 in the two GroupNorm operators
 * (besides C % groups != 0, an unaligned workspace, and 16-bit tensors with C % 8 != 0 or C / 8 > 256).
 * use_op_attention_bwd: the AttnBlockpp core, out = softmax(q k^T / sqrt(C)) v: dq, dk, dv from dO ([B][N][C] each; work: 2 B N N floats). */
size_t use_op_wgrad_workspace(int B, int H, int W, int Cout, int Cin, int ntaps, int dtype);
int use_op_wgrad(const void* dy, const void* x, int dtype, float* dw, float* db, int B, int H, int W, int Cout, int Cin, int ntaps, float alpha,
                 float* work, size_t work_floats, use_stream_t stream);
size_t use_op_gn_workspace(int B, int C, int groups);
int use_op_gn_act_bwd(const void* x, const void* dy, int dtype, const float* gamma, const float* beta, int groups, float eps, int act, const void* add,
                      float add_scale, int B, int HW, int C, float* work, int have_stats, void* dx, float* dgamma, float* dbeta, use_stream_t stream);
int use_op_gn_act_fwd(const void* x, int dtype, const float* gamma, const float* beta, int groups, float eps, int act, int B, int HW, int C, float* work,
                      void* y, use_stream_t stream);
int use_op_colsum(const void* x, int dtype, int B, int HW, int C, float scale, float* out, float* work, use_stream_t stream);
int use_op_dense_bwd(const float* g, const float* temb, const float* Wd, int B, int K, int Cout, float* dW, float* db, float* dtemb,
                     use_stream_t stream);
int use_op_attention_bwd(const float* q, const float* k, const float* v, const float* dO, float* work, float* dq, float* dk, float* dv, int B, int N,
                         int C, use_stream_t stream);
/* ---- wire formats either side of the path, host functions: no device, no handle ----
 * use_wav_read: RIFF/WAVE (PCM 8/16/24/32-bit, IEEE float 32/64, WAVE_FORMAT_EXTENSIBLE) -> interleaved float64 frames scaled like
 *   libsndfile's sf.read (integer PCM / 2^(bits-1)); *samples is malloc'ed, release it with use_free.
 * use_resample_fft: scipy.signal.resample(x, num) == librosa.resample(res_type="fft") for real x (loadwav_dataset.py:95-98).
 * use_load_utterance: the reference's inference loader for one file (loadwav_dataset.py:90-120): first channel, FFT resampling
 *   to target_rate (0: keep), x / max|x| * 0.8 when normalize, float64 throughout, float32 out (malloc'ed; use_free).
 * use_wav_write: sf.write(path, x, rate) of SGMSE_module.py:80 (USE_WAV_PCM16 = soundfile's default WAV subtype) or 32-bit float.
 * use_wav_info: what use_wav_read reports about a file, from its chunk headers alone (no sample is read).
 * use_resampled_length: the length use_load_utterance gives a file of `frames` frames at sample_rate - librosa's ratio-first
 *   rounding, ceil(frames * (double(target_rate) / sample_rate)); `frames` itself for target_rate <= 0 or == sample_rate; -1 for
 *   frames < 0 or sample_rate < 1. */
enum { USE_WAV_PCM16 = 0, USE_WAV_FLOAT32 = 1 };
int use_wav_read(const char* path, double** samples, int64_t* frames, int* channels, int* sample_rate);
int use_wav_write(const char* path, const float* samples, int64_t frames, int channels, int sample_rate, int subtype);
int use_resample_fft(const double* x, int64_t n, int64_t num, double* y);
int use_load_utterance(const char* path, int target_rate, int normalize, float** wav, int64_t* length, int* sample_rate);
/* use_load_utterance with the peak it divided by: *peak = mx (fp64, by `fabs(v) > mx` over the resampled first channel; 0 for a silent
 * file) when normalize != 0, otherwise *peak is not written.  peak may be null.  The row has use_load_utterance's bits. */
int use_load_utterance_peak(const char* path, int target_rate, int normalize, float** wav, int64_t* length, int* sample_rate, double* peak);
int use_wav_info(const char* path, int64_t* frames, int* channels, int* sample_rate);
int64_t use_resampled_length(int64_t frames, int sample_rate, int target_rate);
void use_free(void* p);

/* The front of the loader on the device (csrc/use_resample.hip), handle-free: what use_load_utterance does to the decoded first channel of a
 * file, in fp64 - the host still opens and decodes the file (use_wav_read).
 * use_resample_fft_dev: the device counterpart of use_resample_fft, x_dev [n] -> y_dev [num], both fp64 DEVICE; num == n is a copy.  The
 *   transforms are power-of-two FFTs (Stockham passes through LDS), and Bluestein's form over them for any other length; twiddles and chirps
 *   are evaluated per element from exactly reduced arguments.
 * use_load_items_dev: B signals, x_dev[b] (HOST array of fp64 DEVICE pointers) of n_host[b] samples -> resampled to num_host[b] samples
 *   (num == n: as it is) -> with normalize: mx = max |v| by `fabs(v) > mx`, v / mx * 0.8 with two roundings (a silent item gives NaN, as the
 *   host loader does) -> float32 -> wav[b][0 ... num), exact zeros from there to stride.  wav: float32 DEVICE [B][stride].  At num == n a row
 *   has the bits use_load_utterance gives it.  The items run one after another on `s`; work_bytes covers the largest item.
 * No atomics, and every addition has a place fixed by (n, num) alone: an item's output has the same bits in every run, at every row of every
 * batch, with any companions.  work: use_resample_workspace(n, num) bytes of device scratch for one item, 16-byte aligned (0: n or num < 1 or
 * above 2^24; a host function, no device needed).  Launches on `s` only: no synchronisation, no allocation.
 * USE_E_INVALID (reason in use_last_error(), nothing launched): a null or misaligned pointer, B < 1, n or num < 1, max(n, num) > 2^24,
 * work_bytes too small, stride < num of any item. */
size_t use_resample_workspace(int64_t n, int64_t num);
int use_resample_fft_dev(const double* x_dev, int64_t n, int64_t num, double* y_dev, void* work, size_t work_bytes, use_stream_t s);
int use_load_items_dev(const double* const* x_dev /* [B] device pointers, held on the host */, const int64_t* n_host, const int64_t* num_host,
                       int B, int normalize, float* wav, int64_t stride, void* work, size_t work_bytes, use_stream_t s);
/* use_load_items_dev that also hands out the peaks: peak_dev[b] = the very mx item b's scale kernel divides by, written by that kernel's first
 * workgroup (no extra pass over the samples).  normalize == 0: nothing is written.  peak_dev null: use_load_items_dev.  The rows have the
 * same bits either way.  USE_E_INVALID also for a peak_dev that is not 8-byte aligned. */
int use_load_items_dev_peak(const double* const* x_dev, const int64_t* n_host, const int64_t* num_host, int B, int normalize, float* wav,
                            int64_t stride, void* work, size_t work_bytes, double* peak_dev /* fp64 DEVICE [B] or null */, use_stream_t s);

/* The way out on the device (csrc/use_resample.hip), handle-free: from the sampler's float32 rows to the samples of files at their own rate.
 * use_store_items_dev: wav float32 DEVICE [B][stride], item b valid for len_host[b] samples (HOST ints; a row is never read past them: after
 *   the iSTFT the padding holds anything) -> widened to fp64 -> resampled to num_host[b] samples with the arithmetic of use_resample_fft_dev
 *   (num == len: no transform) -> rounded to float32, x32 -> USE_WAV_FLOAT32: out is float [B][out_stride] and receives x32;
 *   USE_WAV_PCM16: out is int16_t [B][out_stride] and receives what use_wav_write stores for x32, nearbyint((double)x32 * 32767) clamped to
 *   [-32768, 32767], a NaN as 0.  Exact zeros from num[b] to out_stride.  At num == len a float row has the input's bits.
 * use_wav_write_pcm16 (host): the file use_wav_write(..., USE_WAV_PCM16) writes, from ready-made codes (interleaved, as they are).
 * No atomics, and every addition has a place fixed by (len, num) alone: an item's output has the same bits in every run, at every row of every
 * batch, at any stride and out_stride.  The items run one after another on `s`; row offsets are 64-bit.  work: use_store_workspace(len, num)
 * bytes of device scratch for the largest item, 16-byte aligned (0: len or num < 1 or above 2^24; a host function, no device needed).
 * Launches on `s` only: no synchronisation, no allocation.
 * USE_E_INVALID (reason in use_last_error(), nothing launched): a null or misaligned pointer, B < 1, len[b] < 1 or > stride, num[b] < 1 or
 * > out_stride, max(len, num) > 2^24, an unknown subtype, work_bytes too small. */
size_t use_store_workspace(int64_t len, int64_t num);
int use_store_items_dev(const float* wav, int64_t stride, const int* len_host, const int64_t* num_host, int B,
                        int subtype /* USE_WAV_PCM16 | USE_WAV_FLOAT32 */, void* out, int64_t out_stride, void* work, size_t work_bytes,
                        use_stream_t s);
/* use_store_items_dev at the source's level (data.restore_level): gain_host[b] (HOST doubles, passed on as kernel arguments) multiplies every
 * output sample of item b after the resampling and before the rounding to float32: x32 = (float)(v * g), v the fp64 value the store path
 * holds (the resampled value, or the widened row sample at num == len), the product rounded once in fp64 and never contracted; then as above.
 * gain_host null: use_store_items_dev itself, bit for bit (no multiplication by 1 takes place).  USE_E_INVALID (entry named, nothing
 * launched) also for a gain that is NaN, infinite or negative. */
int use_store_items_dev_gain(const float* wav, int64_t stride, const int* len_host, const int64_t* num_host,
                             const double* gain_host /* HOST [B] or null */, int B, int subtype, void* out, int64_t out_stride, void* work,
                             size_t work_bytes, use_stream_t s);
int use_wav_write_pcm16(const char* path, const int16_t* codes, int64_t frames, int channels, int sample_rate);

/* Files of several channels on the device (data.channels=all; csrc/use_resample.hip), handle-free.
 * use_load_files_dev: F files, x_dev[f] (HOST array of fp64 DEVICE pointers) the whole decoded file as use_wav_read returns it, interleaved
 *   [n_host[f]][ch_host[f]].  A file's channels are de-interleaved, each is resampled to num_host[f] samples with the arithmetic (and the
 *   passes) of use_resample_fft_dev, and with normalize ONE peak is taken per file: mx = max |v| over all ch * num values by `fabs(v) > mx`,
 *   every channel v / mx * 0.8 with two roundings - the channels keep their level relation, a silent channel stays exact zeros, a silent
 *   file gives NaN.  Channel c of file f is row (ch[0] + ... + ch[f - 1]) + c of wav (float32 DEVICE [rows][stride]), zero from num to
 *   stride.  A file of one channel has the bits use_load_items_dev gives it.  work: use_load_files_workspace(n, num, channels) bytes for the
 *   largest file, 16-byte aligned (0: n or num < 1 or above 2^24, channels < 1 or > 64; a host function).
 * use_store_files_dev: the way back.  wav float32 DEVICE [rows][stride], file f's ch_host[f] rows valid for len_host[f] samples each; every
 *   row goes through use_store_items_dev's arithmetic to num_host[f] samples (num == len: no transform), and the file is written interleaved,
 *   [num][ch], at out + out_off_host[f] (an ELEMENT offset; out is int16_t or float by subtype): the layout use_wav_write_pcm16 and
 *   use_wav_write store as it is.  Nothing outside the F blocks of num * ch elements is written.  work: use_store_workspace(len, num) bytes
 *   for the largest file.
 * The guarantees of use_load_items_dev / use_store_items_dev hold: launches on `s` only, no allocation, no synchronisation, no atomics,
 * 64-bit row offsets, and a file's output has the same bits in every run, in any batch and at any stride.
 * USE_E_INVALID (argument named in use_last_error(), nothing launched): a null or misaligned pointer, F < 1, ch[f] < 1 or > 64, n / len or
 * num < 1 or above 2^24, stride < num (load) or < len (store), a negative out_off, an unknown subtype, work_bytes too small. */
size_t use_load_files_workspace(int64_t n, int64_t num, int channels);
int use_load_files_dev(const double* const* x_dev /* [F] device pointers, held on the host */, const int64_t* n_host, const int64_t* num_host,
                       const int* ch_host, int F, int normalize, float* wav, int64_t stride, void* work, size_t work_bytes, use_stream_t s);
int use_store_files_dev(const float* wav, int64_t stride, const int* len_host /* [F] */, const int64_t* num_host /* [F] */, const int* ch_host,
                        const int64_t* out_off_host /* [F] element offset of file f in out */, int F,
                        int subtype /* USE_WAV_PCM16 | USE_WAV_FLOAT32 */, void* out, void* work, size_t work_bytes, use_stream_t s);
/* The two with the file's peak and gain (data.restore_level), ONE per file as the normalisation is: peak_dev[f] = the mx file f's rows were
 * divided by (written by the workgroup that reduces the file's partial maxima; normalize == 0: nothing is written), and gain_host[f] applied
 * to every channel of file f as use_store_items_dev_gain applies it.  A null pointer: the call above, bit for bit.  USE_E_INVALID also for
 * a misaligned peak_dev and a gain that is NaN, infinite or negative. */
int use_load_files_dev_peak(const double* const* x_dev, const int64_t* n_host, const int64_t* num_host, const int* ch_host, int F, int normalize,
                            float* wav, int64_t stride, void* work, size_t work_bytes, double* peak_dev /* fp64 DEVICE [F] or null */,
                            use_stream_t s);
int use_store_files_dev_gain(const float* wav, int64_t stride, const int* len_host, const int64_t* num_host, const int* ch_host,
                             const int64_t* out_off_host, const double* gain_host /* HOST [F], one per file, or null */, int F, int subtype,
                             void* out, void* work, size_t work_bytes, use_stream_t s);

/* timesteps of the sampler, torch.linspace(1, t_eps, N) float32 semantics (sampling/__init__.py:63); host only */
int use_timesteps(int N, float t_eps, float* out);
int use_debug_tensor(use_handle* h, const char* name, void** dev_ptr, int* dims4, int* dtype);
double use_flops_per_score(use_handle* h);   /* 2*MAC of the conv/linear layers for the current plan */

/* Launch trace (test infrastructure; use_set_option("trace", 1), off by default, not a tuning knob: it does not mark plans stale).
 * While it is on, the primary sub-batch of every network evaluation (use_score / use_score2 / use_forward*) records one entry per launch
 * it issues, in launch order; the list belongs to the plan and is replaced by the next evaluation (cleared where the debug tensors are).
 * No launch changes: the entries are filled from the very argument structs the launches take.  The activation arena is only reset at the
 * start of an evaluation, so after a synchronise every pointer below is still valid device memory and holds what that launch wrote
 * (exceptions: USE_TRACE_COMBINE_ADD and USE_TRACE_SOFTMAX_ROWS rewrite their input in place).  Not recorded: the zeroing of the totals
 * region at the start of an evaluation (one launch; every totals pointer lies inside it).
 *
 * Tensors are NHWC; dims = (B, H, W, C) with B the items of the sub-batch, dtype = USE_PREC_* of the storage.  Complex64 tensors (the
 * evaluation's x, y, y2 and its output) are given as fp32 with C = 2.  Totals: [B][C][2] 64-bit fixed point (sum, sum of squares, each
 * * 2^20) of the stored values; partial totals: [B][parts][C][2] in the same format, to be summed over `parts`.  Where part_in[k] is set the
 * launch reads those and not totals_in[k] (the pointer is passed all the same, and nothing was written behind it).
 *
 * kind                  in[]                                               out[]                       further fields
 * USE_TRACE_TEMB        -                                                  0: tembias [n,1,1,dense_rows]   t; params W (Fourier), X0..X3 (Linear 1, 2)
 *                                                                          1: silu(temb) [n,1,1,4 nf]      (the Dense_0 rows: see CONV's DENSE_W / DENSE_B)
 * USE_TRACE_PACK_INPUT  0: x, 1: y, 2: y2 (absent: ptr null)               0: x4 [B,F,T,4 or 8] fp32       (B: the whole batch)
 * USE_TRACE_CONV        0, 1: concat halves; 2, 3: shortcut sources;       0                               kernel, act, out_scale, ntaps, gn_* (inline), coef,
 *                       4: residual; 5: Combine / pyramid input (fp32)                                     totals_in / part_in of in[0], in[1] (inline GroupNorm),
 *                                                                                                          totals_out or part_out + parts_out, tembias + temb_row
 *                                                                                                          + temb_stride; params W, B (bias of W), W2, B2 (bias
 *                                                                                                          of W2: the kernel adds B + B2 as one array), GN_*,
 *                                                                                                          CB_* (Combine), DENSE_* (the layer whose row is read)
 * USE_TRACE_FIR_DOWN/UP 0                                                  0: FIR(act(a x + b)) or absent  coef (read; null: out[1] alone, the input pyramid),
 *                                                                          1: FIR(x)                       act
 * USE_TRACE_GN_FINALIZE 0, 1: the maps whose totals are read (not read     -                               totals_in / part_in + parts_in, coef_out [B][C0+C1][2],
 *                       themselves)                                                                        gn_groups, gn_inv_n, gn_eps; params GN_*
 * USE_TRACE_ATTN_FUSED  0                                                  0                               totals_in[0], totals_out, gn_*; params GN_*, W / B
 *                                                                                                          (NIN_0), X0..X5 (NIN_1 W, b; NIN_2; NIN_3), out_scale
 * USE_TRACE_ATTN_CORE   0: q, 1: k, 2: v                                   0
 * USE_TRACE_COMBINE_ADD 0: the map (in place), 5: pyramid input            0: == in[0]                     totals_out (zeroed by a launch of its own just before);
 *                                                                                                          params CB_*
 * USE_TRACE_SCORE_OUT   0: pyramid fp32                                    0: the evaluation's output      t (null: no division), t_stride, out_scale = sign;
 *                                                                                                          params W, B (output_layer)
 * The GEMM form of the attention core (N > 512 tokens, use_op_attention_gemm), 2 + 2 B entries between the NIN_0..2 and the NIN_3 convolutions:
 * USE_TRACE_TRANSPOSE   0: v [B,1,N,C]                                     0: vt [B,1,C,N]
 * USE_TRACE_ATTN_GEMM   0: one item's operand [1,H,W,K], 1: its "weights"   0: the item's output slice     kernel (conv_choose's answer for this launch), out_scale,
 *                       [1,1,Cout,K].  Scores: q and the item's keys       [1,H,W,Cout] (of the score     ntaps = 1, act = 0; no bias and no parameter: every
 *                       (K = C, Cout = N); P.V: the item's probabilities   buffer; of the block's         operand is an activation.  One entry per launch: B
 *                       and its slice of vt (K = N, Cout = C)              output)                        for the scores, the softmax, then B for P.V
 * USE_TRACE_SOFTMAX_ROWS 0: the score buffer [B,N,1,N] (in place)          0: == in[0]
 * Parameter names are the reference state-dict keys (as use_expected_weight reports them); unused roles are null.  The strings belong
 * to the handle.  use_trace_count: entries of the current plan's last evaluation (0: none, or the trace was off), < 0: error. */
enum { USE_TRACE_TEMB = 1, USE_TRACE_PACK_INPUT, USE_TRACE_CONV, USE_TRACE_FIR_DOWN, USE_TRACE_FIR_UP, USE_TRACE_GN_FINALIZE,
       USE_TRACE_ATTN_FUSED, USE_TRACE_ATTN_CORE, USE_TRACE_COMBINE_ADD, USE_TRACE_SCORE_OUT,
       USE_TRACE_TRANSPOSE, USE_TRACE_ATTN_GEMM, USE_TRACE_SOFTMAX_ROWS };
enum { USE_TP_W = 0, USE_TP_B, USE_TP_W2, USE_TP_B2, USE_TP_GN_W, USE_TP_GN_B, USE_TP_CB_W, USE_TP_CB_B, USE_TP_DENSE_W, USE_TP_DENSE_B,
       USE_TP_X0, USE_TP_X1, USE_TP_X2, USE_TP_X3, USE_TP_X4, USE_TP_X5, USE_TP_COUNT };
typedef struct use_trace_tensor { const void* ptr; int dims[4]; int dtype; } use_trace_tensor;
typedef struct use_trace_entry {
    int kind;
    char kernel[32];                     /* ConvChoice::label for a convolution, else the launch's name */
    use_trace_tensor in[6], out[2];
    const void* totals_in[2]; const void* part_in[2]; int parts_in[2];
    const void* totals_out; const void* part_out; int parts_out;
    const void* coef; const void* coef_out;
    const void* tembias; int temb_row, temb_stride;      /* the launch reads tembias[b * temb_stride + temb_row + c] */
    const void* t; int t_stride;
    int act; float out_scale; int ntaps;
    int gn_groups; float gn_inv_n, gn_eps;               /* gn_groups 0: no GroupNorm finalised by this launch */
    const char* params[USE_TP_COUNT];
} use_trace_entry;
int use_trace_count(use_handle* h);
int use_trace_entry_get(use_handle* h, int index, use_trace_entry* out);

/* Sampler step trace (test infrastructure; use_set_option("sampler_trace", 1), off by default, not a tuning knob: it does not mark plans
 * stale).  While it is on, a call of use_sample / use_sample_cond / use_sample_cond2 / use_sample_items records one entry per launch
 * the predictor-corrector loop issues, in launch order, a network evaluation counting as one launch.  The loop overwrites its state X,
 * the score and the Langevin step in place, so the call also keeps snapshots: device-to-device copies on the loop's own stream into a
 * buffer that belongs to the plan - of X after the prior and after every corrector and predictor launch, of the score after every
 * evaluation, of the Langevin step ([items] floats) after every LANGEVIN_STEP, of Xmean at the end.  The copies are captured into the
 * graph segments and replayed with them; the entries of a captured loop are kept with its graphs and returned for every replay.  No
 * launch changes and no bit of the result does.  The buffer is allocated at the first traced call of a sampler configuration and filled
 * with NaN before every traced call (an untaken snapshot is not finite); one that
 * needs more than 256 MB is refused (USE_E_INVALID, the size named, nothing launched): the trace is for small shapes.  The option may
 * change between calls: graphs captured under the other setting are dropped, a call with the option off records nothing, allocates
 * nothing, copies nothing and leaves use_sampler_trace_count at 0.  use_sample_ode is not traced.
 *
 * Every pointer below is a snapshot (complex64 [B][F][T'] unless said otherwise), valid after a synchronise until the next sampler
 * call, use_set_sampler or use_plan; a field a kind does not use is null / 0 / -1.  i: reverse step, k: corrector index (-1: the prior,
 * and the predictor with its evaluation), d: the noise draw the launch consumed (-1: none), t = timesteps[i] (1 for the prior).  items,
 * n_per_item: the addressing of the element-wise updates (1, B F T' or B, F T'); per_item: 1 in use_sample_items.
 *
 * kind                      reads                               writes      scalars (float32, exactly as passed to the launch)
 * USE_STRACE_PRIOR          noise (draw 0; null: device RNG)    x_out       std1
 * USE_STRACE_SCORE          x_in                                score
 * USE_STRACE_LANGEVIN_NORMS score, noise                        -           blocks_per_b (workgroups per item of the reduction)
 * USE_STRACE_LANGEVIN_STEP  (the norms)                         step [items] float32     blocks_per_b
 * USE_STRACE_CORRECTOR      x_in, score, noise, step (Langevin) x_out       step_host (ALD; Langevin: 0 and step set)
 * USE_STRACE_PREDICTOR      x_in, score, noise                  x_out, x_mean (last step only)   c_drift, c_score, c_noise
 * USE_STRACE_COPY_MEAN      x_in                                x_mean      (USE_PRED_NONE, last step: Xmean is a copy of X)
 * use_sampler_trace_count: entries of the current plan's last sampler call (0: none, or the trace was off), < 0: error. */
enum { USE_STRACE_PRIOR = 1, USE_STRACE_SCORE, USE_STRACE_LANGEVIN_NORMS, USE_STRACE_LANGEVIN_STEP, USE_STRACE_CORRECTOR,
       USE_STRACE_PREDICTOR, USE_STRACE_COPY_MEAN };
typedef struct use_sampler_trace_entry {
    int kind;
    int i, k, d;
    float t;
    float std1, c_drift, c_score, c_noise, step_host;
    int items; int64_t n_per_item; int blocks_per_b, per_item;
    const void *x_in, *score, *step, *x_out, *x_mean;
    const void* noise;                   /* injected noise: the draw this launch read (graph replay: inside the library's staging copy) */
} use_sampler_trace_entry;
int use_sampler_trace_count(use_handle* h);
int use_sampler_trace_get(use_handle* h, int index, use_sampler_trace_entry* out);

#ifdef __cplusplus
}
#endif
#endif
