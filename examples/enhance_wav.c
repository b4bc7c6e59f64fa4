/* enhance_wav.c -- the whole predict path of the reference (src/predict.py -> SGMSEModule.predict_step -> ScoreModel.sample) for one
 * file through the C ABI of libuse_hip.so alone: no Python, no torch.  What a non-Python host of the library looks like.
 *
 *   enhance_wav <weights.usehip> <noisy.wav> <enhanced.wav> [N=30] [seed=0] [precision: bf16|fp16|fp32 = what the file was packed for]
 *               [--chunk-frames C [--chunk-overlap M=64]] [--refine refine.usehip]
 *
 * --chunk-frames C (a multiple of 64; anywhere on the line): a recording of more than C padded frames is sampled in overlapping windows of C
 * frames, groups of at most 8 windows per sampler call with seed + group index, and cross-faded back (use_chunk_count / _split / _merge):
 * one plan per group size whatever the file length.  Without the flag, or for a shorter file, the whole file is one sampler call.
 * --refine refine.usehip (anywhere on the line): the second stage of the reference's pipeline in the same run, on a second handle - the
 * sampler's waveform passes use_wav_handoff (the 16-bit samples a stage-1 file would hold, the loader's peak normalisation to 0.8: what
 * lies between the two predict runs of the reference's README, on the device) and then the LSGAN generator, use_stft_fwd -> use_forward ->
 * use_istft_back, one pass over the whole file; enhanced.wav then holds the refined signal.  refine.usehip: pack_checkpoint model=LSGAN
 * at the precision of weights.usehip.
 * weights.usehip: `python -m universal_speech_enhancement_amd.pack_checkpoint ckpt=last.ckpt out=weights.usehip precision=bf16`
 * Steps (reference file:line): loader (loadwav_dataset.py:90-120) -> STFT + compression + padding (model_wrapper.py:275-278) ->
 * 30-step PC sampler, reverse diffusion + Langevin x1, snr 0.5 (SGMSE_Large.yaml, sampling/__init__.py:59-71) -> decompression +
 * iSTFT (:320) -> sf.write (SGMSE_module.py:80).
 * build: gcc -O2 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude examples/enhance_wav.c -o examples/enhance_wav \
 *            -Luniversal_speech_enhancement_amd -luse_hip -L/opt/rocm/lib -lamdhip64 -lm -Wl,-rpath,'$ORIGIN/../universal_speech_enhancement_amd' */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "use_hip.h"

#define CHECK(call)                                                                          \
    do {                                                                                     \
        int rc_ = (call);                                                                    \
        if (rc_ != 0) { fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, use_last_error()); return 1; } \
    } while (0)
#define HIPCHECK(call)                                                                       \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) { fprintf(stderr, "%s failed: %s\n", #call, hipGetErrorString(e_)); return 1; } \
    } while (0)

/* windows [n,1,F,C] in, sampled in groups of at most 8 with seed + group index, cross-faded out; the two window buffers are freed on
 * every way out */
static int sample_chunked(use_handle* h, const use_sampler_config* sc, const void* d_Y, void* d_X, int F, int Tpad, int C, int overlap,
                          int n_chunks, unsigned long long seed) {
    const size_t win_bytes = (size_t)F * C * 8;
    char *d_cin = NULL, *d_cout = NULL;
    int rc = 1;
#define TRY(call)                                                                            \
    do {                                                                                     \
        if ((call) != 0) { fprintf(stderr, "%s failed: %s\n", #call, use_last_error()); goto done; } \
    } while (0)
    if (hipMalloc((void**)&d_cin, n_chunks * win_bytes) != hipSuccess || hipMalloc((void**)&d_cout, n_chunks * win_bytes) != hipSuccess) {
        fprintf(stderr, "hipMalloc of %d windows failed\n", n_chunks);
        goto done;
    }
    TRY(use_chunk_split(d_Y, d_cin, 1, F, Tpad, C, overlap, NULL));
    for (int lo = 0, g = 0; lo < n_chunks; lo += 8, ++g) {
        const int gb = n_chunks - lo < 8 ? n_chunks - lo : 8;
        TRY(use_plan(h, gb, C));                                           /* at most two shapes: parked plans keep their graphs */
        TRY(use_set_sampler(h, sc));
        TRY(use_sample(h, d_cin + lo * win_bytes, NULL, seed + (unsigned long long)g, d_cout + lo * win_bytes, NULL));
    }
    TRY(use_chunk_merge(d_cout, d_X, 1, F, Tpad, C, overlap, NULL));
    rc = hipDeviceSynchronize() != hipSuccess;                             /* the merge has read d_cout before it is freed */
#undef TRY
done:
    hipFree(d_cin); hipFree(d_cout);
    return rc;
}

int main(int argc, char** argv) {
    int chunk_frames = -1, chunk_overlap = 64;                              /* -1: no --chunk-frames */
    const char* refine_path = NULL;                                         /* NULL: no --refine */
    {   /* take the optional flags out of argv; the positional arguments keep their places */
        int k = 1;
        for (int i = 1; i < argc; ++i) {
            if (!strcmp(argv[i], "--refine")) {
                if (++i >= argc) { fprintf(stderr, "%s needs a value\n", argv[i - 1]); return 2; }
                refine_path = argv[i];
                continue;
            }
            int* dst = !strcmp(argv[i], "--chunk-frames") ? &chunk_frames : !strcmp(argv[i], "--chunk-overlap") ? &chunk_overlap : NULL;
            if (!dst) { argv[k++] = argv[i]; continue; }
            if (++i >= argc) { fprintf(stderr, "%s needs a value\n", argv[i - 1]); return 2; }
            char* end = NULL;
            const long v = strtol(argv[i], &end, 10);                       /* a whole non-negative integer, or the usage error */
            if (end == argv[i] || *end || v < 0 || v > 1 << 30) { fprintf(stderr, "%s %s: not a frame count\n", argv[i - 1], argv[i]); return 2; }
            *dst = (int)v;
        }
        argc = k;
    }
    if (argc < 4) {
        fprintf(stderr, "usage: %s weights.usehip noisy.wav enhanced.wav [N=30] [seed=0] [bf16|fp16|fp32] [--chunk-frames C [--chunk-overlap M]] [--refine refine.usehip]\n", argv[0]);
        return 2;
    }
    const int N = argc > 4 ? atoi(argv[4]) : 30;
    const unsigned long long seed = argc > 5 ? strtoull(argv[5], NULL, 10) : 0ull;
    const char* prec = argc > 6 ? argv[6] : "bf16";
    const int n_fft = 1022, hop = 160, F = n_fft / 2 + 1;
    const float factor = 0.15f, expo = 0.5f;

    float* wav = NULL; int64_t L = 0; int sr = 0;
    CHECK(use_load_utterance(argv[2], 24000, 1, &wav, &L, &sr));           /* first channel, 24 kHz FFT resampling, peak 0.8 */
    const int T = 1 + (int)(L / hop), Tpad = (T + 63) / 64 * 64;
    int n_chunks = 1;                                                       /* 1: the file is one sampler call */
    if (chunk_frames >= 0) { n_chunks = use_chunk_count(Tpad, chunk_frames, chunk_overlap); CHECK(n_chunks < 0 ? n_chunks : 0); }

    use_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.nf = 128; cfg.n_levels = 7; cfg.num_res_blocks = 2; cfg.n_freq = F;
    { const int cm[7] = {1, 1, 2, 2, 2, 2, 2}; memcpy(cfg.ch_mult, cm, sizeof cm); }
    cfg.precision = !strcmp(prec, "fp32") ? USE_PREC_FP32 : !strcmp(prec, "fp16") ? USE_PREC_FP16 : USE_PREC_BF16;
    cfg.theta = 1.5f; cfg.sigma_min = 0.05f; cfg.sigma_max = 0.5f; cfg.input_channels = 4;
    use_handle* h = NULL;
    CHECK(use_create(&cfg, 0, &h));
    CHECK(use_load_weight_blob(h, argv[1]));
    use_handle* hg = NULL;                                                  /* NCSNpp(discriminative=True): GAN/generator/ncsnpp/model_wrapper.py:54 */
    if (refine_path) {
        use_config gcfg;
        memset(&gcfg, 0, sizeof gcfg);
        gcfg.nf = 128; gcfg.n_levels = 4; gcfg.num_res_blocks = 1; gcfg.n_freq = F;
        { const int cm[4] = {1, 2, 2, 2}; memcpy(gcfg.ch_mult, cm, sizeof cm); }
        gcfg.precision = cfg.precision;
        gcfg.theta = 1.5f; gcfg.sigma_min = 0.05f; gcfg.sigma_max = 0.5f;
        gcfg.input_channels = 2; gcfg.unconditional = 1; gcfg.no_sigma_scale = 1;
        CHECK(use_create(&gcfg, 0, &hg));
        CHECK(use_load_weight_blob(hg, refine_path));
    }

    float* win = (float*)malloc(sizeof(float) * n_fft);                     /* periodic Hann (model_wrapper.py:14-20) */
    for (int n = 0; n < n_fft; ++n) win[n] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)n / (double)n_fft));
    float *d_wav = NULL, *d_out = NULL, *d_win = NULL; void *d_Y = NULL, *d_X = NULL;
    const size_t spec_bytes = (size_t)F * Tpad * 8;
    HIPCHECK(hipMalloc((void**)&d_wav, L * 4)); HIPCHECK(hipMalloc((void**)&d_out, L * 4)); HIPCHECK(hipMalloc((void**)&d_win, n_fft * 4));
    HIPCHECK(hipMalloc(&d_Y, spec_bytes)); HIPCHECK(hipMalloc(&d_X, spec_bytes));
    HIPCHECK(hipMemcpy(d_wav, wav, L * 4, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_win, win, n_fft * 4, hipMemcpyHostToDevice));

    CHECK(use_stft_fwd(d_wav, d_Y, 1, (int)L, n_fft, hop, d_win, Tpad, factor, expo, NULL));
    use_sampler_config sc;
    memset(&sc, 0, sizeof sc);
    sc.N = N; sc.predictor = USE_PRED_REVERSE_DIFFUSION; sc.corrector = USE_CORR_LANGEVIN; sc.corrector_steps = 1;
    sc.snr = 0.5f; sc.t_eps = 3e-2f; sc.use_graph = 1;
    if (n_chunks == 1) {
        CHECK(use_plan(h, 1, Tpad));
        CHECK(use_set_sampler(h, &sc));
        CHECK(use_sample(h, d_Y, NULL, seed, d_X, NULL));                  /* device Philox noise */
    } else if (sample_chunked(h, &sc, d_Y, d_X, F, Tpad, chunk_frames, chunk_overlap, n_chunks, seed)) {
        return 1;
    }
    CHECK(use_istft_back(d_X, d_out, 1, (int)L, n_fft, hop, d_win, Tpad, factor, expo, NULL));
    if (hg) {   /* the stage-1 file and the second run's loader, on the device and in place; then the generator over the same buffers */
        const int len = (int)L;
        const size_t work_bytes = use_wav_handoff_workspace(1, L);
        void* d_work = NULL; double* d_peak = NULL;
        HIPCHECK(hipMalloc(&d_work, work_bytes)); HIPCHECK(hipMalloc((void**)&d_peak, sizeof(double)));
        CHECK(use_wav_handoff(d_out, d_out, L, &len, 1, USE_WAV_PCM16, 1, d_work, work_bytes, d_peak, NULL));
        CHECK(use_stft_fwd(d_out, d_Y, 1, (int)L, n_fft, hop, d_win, Tpad, factor, expo, NULL));
        CHECK(use_plan(hg, 1, Tpad));
        CHECK(use_forward(hg, d_Y, NULL, NULL, d_X, NULL));
        CHECK(use_istft_back(d_X, d_out, 1, (int)L, n_fft, hop, d_win, Tpad, factor, expo, NULL));
        HIPCHECK(hipDeviceSynchronize());
        hipFree(d_work); hipFree(d_peak);
    }
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(wav, d_out, L * 4, hipMemcpyDeviceToHost));
    CHECK(use_wav_write(argv[3], wav, L, 1, sr, USE_WAV_PCM16));
    printf("%s: %lld samples at %d Hz, %d frames (T' = %d), %d-step PC sampler -> %s\n", argv[2], (long long)L, sr, T, Tpad, N, argv[3]);
    if (n_chunks > 1) printf("sampled in %d windows of %d frames, %d frames of overlap\n", n_chunks, chunk_frames, chunk_overlap);
    if (hg) { printf("refined by %s\n", refine_path); use_destroy(hg); }
    use_destroy(h); use_free(wav); free(win);
    hipFree(d_wav); hipFree(d_out); hipFree(d_win); hipFree(d_Y); hipFree(d_X);
    return 0;
}
