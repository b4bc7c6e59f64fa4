// Host side of libuse_hip.so: NCSN++ architecture walk (reference backbones/ncsnpp.py:116-316, 324-501),
// weight packing, workspace planning, the score evaluation, the predictor-corrector loop
// (reference sampling/__init__.py:59-71) with hipGraph capture, and the C ABI of include/use_hip.h.
#include "../../include/use_hip.h"
#include "use_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

using namespace use;

// ---------------------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------------------
static thread_local std::string g_err;
static int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    g_err = buf;
    return code;
}
// error reporting for the other translation units of the library (use_io.cpp)
int use_set_error(int code, const char* msg) { g_err = msg ? msg : ""; return code; }
#define HIPCHK(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess) return fail(USE_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

static inline uint16_t f32_to_bf16(float f) {   // round to nearest even
    uint32_t u; memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

static inline uint16_t f32_to_f16(float f) {    // round to nearest even, overflow -> inf, subnormals kept
    uint32_t u; memcpy(&u, &f, 4);
    const uint32_t sign = (u >> 16) & 0x8000u;
    u &= 0x7fffffffu;
    if (u > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);                 // NaN
    if (u >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                // >= 65520 -> inf
    if (u < 0x38800000u) {                                                  // subnormal half (or zero)
        if (u < 0x33000000u) return (uint16_t)sign;
        const int shift = 126 - (int)(u >> 23);                             // 14..24
        uint32_t m = (u & 0x7fffffu) | 0x800000u;
        const uint32_t half = 1u << (shift - 1), rest = m & ((1u << shift) - 1);
        m >>= shift;
        if (rest > half || (rest == half && (m & 1))) ++m;
        return (uint16_t)(sign | m);
    }
    uint32_t v = u - 0x38000000u;                                           // rebias exponent
    const uint32_t rest = v & 0x1fffu;
    v >>= 13;
    if (rest > 0x1000u || (rest == 0x1000u && (v & 1))) ++v;
    return (uint16_t)(sign | v);
}

// ---------------------------------------------------------------------------------------------------------
// architecture description
// ---------------------------------------------------------------------------------------------------------
struct ConvW { std::string wname, bname; int cin = 0, cout = 0, cout_pad = 0, ntaps = 1, w_dtype = DT_F32;
               bool nin = false; size_t w_off = 0, b_off = 0;
               int cin_src = 0, cout_src = 0;                 // extents of the host tensor when it is zero-padded to cin / cout
               size_t wb_off = 0; bool has_wb = false;        // slab-major copy for conv_wide_kernel (see pack_conv)
               bool split_in = false; };                      // wb = the bf16 hi / lo split copy of the input convolution (pack_conv_in_split)
struct GNW { std::string prefix; int C = 0; size_t g_off = 0, b_off = 0; };
struct ResW { int idx = 0, in_ch = 0, out_ch = 0; bool up = false, down = false, has_c2 = false;
              GNW gn0, gn1; ConvW c0, c1, c2; int dense_row0 = 0; size_t b12_off = 0; };   // b12 = Conv_1.bias + Conv_2.bias
struct CombineW { int idx = 0, C = 0; size_t w_off = 0, b_off = 0; };      // conv1x1 4->C, fp32 [C][4]
struct AttnW { int idx = 0, C = 0; GNW gn; ConvW q, k, v, o; };
struct PyrW { GNW gn; ConvW conv; };

struct Expected { std::string name; std::vector<int64_t> shape; };

constexpr int MAX_SUB = 8;                       // sub-batches of the pipelined evaluation (run_score)

struct Act { void* p = nullptr; int C = 0, H = 0, W = 0, dtype = DT_F32; long long* stats = nullptr;     // stats: [B][C][2] fixed-point totals
             long long* part = nullptr; int ntiles = 0; };   // or (large maps, conv_v4 producers) [B][ntiles][C][2] per-workgroup partial totals (ConvArgs::stats_part)

struct Arena {
    char* base = nullptr; size_t cap = 0, off = 0, peak = 0;
    bool overflow = false;           // sticky: an allocation did not fit (cannot happen for the plan the arena was sized for)
    bool* dry_on_overflow = nullptr; // ... and then the evaluation switches itself to the bookkeeping-only mode: no further launch
    void reset() { off = 0; }
    void* alloc(size_t bytes) {
        off = (off + 255) & ~(size_t)255;
        void* p = base ? (void*)(base + off) : nullptr;
        off += bytes;
        if (off > peak) peak = off;
        if (base && off > cap) {     // never a write past the allocation and never abort() behind a C ABI: the entry point that
            overflow = true;         // ran this evaluation reports USE_E_STATE (see eval_status); the tensor that did not fit is not touched
            if (dry_on_overflow) *dry_on_overflow = true;
            p = base;
        }
        return p;
    }
};

// Everything use_plan(B, T') builds for one shape.  A plan is a value with one owner - the handle's `plan` (the current one) or a slot of
// its `parked` list - and its destructor frees what it owns.  Never copied or moved: the arenas point at `dry`, captured graphs hold addresses.
struct Plan {
    int B = 0, T = 0;
    long long opt_gen = -1;                      // g_opt_gen when the plan was built: plans built under other options are not reused
    Arena arena;                                 // base: the workspace allocation (all sub-batch arenas + GroupNorm totals, arena_plan_bytes)
    size_t arena_plan_bytes = 0;
    char* persist = nullptr; size_t persist_bytes = 0;
    float *x4 = nullptr, *silu_temb = nullptr, *tembias = nullptr, *t_dev = nullptr;
    float2 *Y = nullptr, *X = nullptr, *Xmean = nullptr, *score = nullptr, *xin = nullptr;
    float2 *cond_buf = nullptr, *cond2_buf = nullptr;   // cond2: the second conditioning spectrogram of condition="both" (6 input channels)
    float2 *Cond = nullptr;                      // score conditioning of the sampler: == Y unless use_sample_cond gave another
    float *lang_partial = nullptr;
    float* lang_step = nullptr;                  // [B] Langevin steps: one per item (use_sample_items), or [0] for the batch
    unsigned long long* seeds = nullptr;         // [B] Philox seeds: one per item, or [0] for the shared stream.  Every call uploads its own
                                                 // before its launches; the kernels read them, so graphs replay with new seeds
    int lang_blocks = 0;
    // sampler
    use_sampler_config sc{};
    bool sampler_set = false;
    std::vector<float> timesteps;
    float* ts_dev = nullptr; float* temb_table = nullptr; float* silu_table = nullptr;
    float2* noise_copy = nullptr; size_t noise_copy_bytes = 0;
    // sub-batch pipelining (see run_score): the batch is evaluated as up to MAX_SUB sub-batches (default three) on as many streams, the second started when
    // the first reaches its small feature maps, so that one half's latency-bound kernels hide behind the other's large ones
    int nsub = 1, sub_B[MAX_SUB] = {};  // sub-batch sizes (nsub = 1: not split)
    Arena sub_arena[MAX_SUB];                    // workspaces of sub-batches 1.. (inside the same allocation as `arena`)
    Arena st_arena[MAX_SUB];                     // per sub-batch: the GroupNorm totals of all its activations, contiguous (one memset per evaluation)
    std::vector<hipGraphExec_t> graph_exec[4];           // [0]: device RNG, [1]: injected noise, [2], [3]: the same of the per-item loop; one graph per segment of steps
    hipGraphExec_t score_graph = nullptr;
    // probability-flow ODE sampler: the configuration belongs to the plan (use_set_ode), the stepper to the handle
    use_ode_config oc{};
    bool ode_set = false;
    // introspection
    bool dry = false;                            // bookkeeping-only evaluation (sizing, or after an overflow): what the arenas' dry_on_overflow points at
    std::map<std::string, Act> debug;
    int debug_B = 0;
    std::vector<use_trace_entry> trace;          // use_set_option("trace", 1): the launches of the last evaluation's primary sub-batch
    size_t trace_head = 0;                       // ... of which this many were recorded ahead of Fwd::run (time embedding, pack_input)
    double flops = 0.0;
    // sampler step trace (use_set_option("sampler_trace", 1); use_sampler_trace_entry, use_hip.h).  One entry list per graph set ([gi], kept
    // with the graphs it was recorded at the capture of) and one for eager calls ([4]); strace_cur: the list of the last sampler call
    std::vector<use_sampler_trace_entry> strace[5];
    int strace_cur = -1;                         // -1: the last call was not traced
    int strace_rec = -1;                         // the list run_sampler is recording into (-1: not tracing)
    bool graphs_traced = false;                  // the setting graph_exec[] were captured under
    char* strace_buf = nullptr; size_t strace_bytes = 0, strace_off = 0;   // the snapshots: bump-allocated in launch order from offset 0
    const float2 *strace_x = nullptr, *strace_score = nullptr; const float* strace_step = nullptr;   // the newest snapshot of each

    Plan() = default;
    Plan(const Plan&) = delete;
    Plan& operator=(const Plan&) = delete;
    void drop_sampler_graphs() {
        for (auto& v : graph_exec) { for (auto g : v) if (g) (void)hipGraphExecDestroy(g); v.clear(); }
    }
    void drop_graphs() {
        drop_sampler_graphs();
        if (score_graph) { (void)hipGraphExecDestroy(score_graph); score_graph = nullptr; }
    }
    ~Plan() {
        drop_graphs();
        for (void* d : {(void*)arena.base, (void*)persist, (void*)temb_table, (void*)silu_table, (void*)ts_dev, (void*)noise_copy, (void*)strace_buf})
            if (d) (void)hipFree(d);
    }
};

struct use_handle {
    use_config cfg{};
    int device = 0;
    int act_dtype = DT_F32;
    // architecture
    std::vector<Expected> expected;
    std::unordered_map<std::string, size_t> expected_index;
    ConvW conv_in;
    std::vector<ResW> res;            // in forward order
    std::vector<CombineW> combines;   // one per down level
    AttnW attn;
    std::vector<PyrW> pyrs;           // in forward order (coarsest level first)
    int dense_rows = 0;
    size_t gfp_off = 0, l1w_off = 0, l1b_off = 0, l2w_off = 0, l2b_off = 0, dense_w_off = 0, dense_b_off = 0,
           outw_off = 0, outb_off = 0;
    size_t blob_bytes = 0;
    int pcp = 4;                                 // input / pyramid channels as stored: the reference's 2, 4 or 6 zero-padded to 4 or 8
    // weights
    std::unordered_map<std::string, std::vector<float>> host_w;
    char* blob = nullptr; bool weights_ready = false;
    // The current plan (null: use_plan has not been called, or the last one failed) and the plan cache: a predict run over files of
    // different lengths alternates between a handful of (B, T') shapes; the plans of the most recently used ones are parked - workspace,
    // state buffers, time-embedding tables and the captured graphs with the addresses they hold - so that a shape that returns is
    // neither re-planned nor re-captured.  use_set_option("plan_cache", k).
    std::unique_ptr<Plan> plan;
    std::vector<std::unique_ptr<Plan>> parked;   // most recently used last
    long long n_graph_captures = 0, n_plans_built = 0, n_plan_cache_hits = 0;
    // streams and events of the sub-batch pipeline (run_score) and of graph capture: made once, shared by all plans
    hipStream_t cap_stream = nullptr;
    hipStream_t aux_stream[MAX_SUB] = {};
    hipEvent_t ev_fork = nullptr, ev_stagger[MAX_SUB] = {},
               ev_join[MAX_SUB] = {};
    // probability-flow ODE sampler (use_sample_ode): the stepper's buffers and the captured step graph (re-made when the shape, the
    // stepper or a pointer the graph holds changes)
    use_ode* ode_run = nullptr;
    hipGraphExec_t ode_graph = nullptr;
    std::vector<const void*> ode_graph_key;
    long long ode_steps = 0, ode_rejected = 0, ode_nfev_max = 0;
    // scratch for the stand-alone use_sde_* entry points (independent of weights / plan)
    char* sde_buf = nullptr; unsigned long long* sde_seeds = nullptr; float* sde_step = nullptr; float* sde_partial = nullptr;
    static constexpr int SDE_MAX_B = 1024, SDE_BLOCKS = 128;
    // per-launch HIP-event profiling (use_profile_score): one record per timed launch, in launch order - the dominant conv kernel (main),
    // the other convolutions and the HBM-bound kernels around them (FIR resampling, pyramid heads, input convolution).  desc: the line of
    // USE_HIP_PROFILE_VERBOSE, set for the launches it lists (those are reported there, not as records of use_profile_aux)
    bool profile = false, profile_all = false;
    struct ProfRec { std::string label; int H = 0, W = 0; double flops = 0.0, bytes = 0.0; hipEvent_t e0 = nullptr, e1 = nullptr; double ms = 0.0; bool main = false; std::string desc; };
    std::vector<ProfRec> prof;
};

static void add_expected(use_handle* h, const std::string& name, std::vector<int64_t> shape) {
    h->expected_index[name] = h->expected.size();
    h->expected.push_back({name, std::move(shape)});
}

static ConvW make_conv(use_handle* h, const std::string& prefix, int cin, int cout, int ntaps, int w_dtype,
                       int cin_src = 0, int cout_src = 0) {
    ConvW c; c.wname = prefix + ".weight"; c.bname = prefix + ".bias"; c.cin = cin; c.cout = cout; c.ntaps = ntaps;
    c.w_dtype = w_dtype;
    c.cin_src = cin_src ? cin_src : cin; c.cout_src = cout_src ? cout_src : cout;
    c.cout_pad = cout <= 32 ? 32 : (cout + 127) / 128 * 128;
    const int k = ntaps == 9 ? 3 : 1;
    add_expected(h, c.wname, {c.cout_src, c.cin_src, k, k});
    add_expected(h, c.bname, {c.cout_src});
    return c;
}
static ConvW make_nin(use_handle* h, const std::string& prefix, int C, int w_dtype) {
    ConvW c; c.wname = prefix + ".W"; c.bname = prefix + ".b"; c.cin = C; c.cout = C; c.ntaps = 1; c.w_dtype = w_dtype;
    c.nin = true; c.cout_pad = (C + 127) / 128 * 128; c.cin_src = C; c.cout_src = C;
    add_expected(h, c.wname, {C, C});
    add_expected(h, c.bname, {C});
    return c;
}
static GNW make_gn(use_handle* h, const std::string& prefix, int C) {
    GNW g; g.prefix = prefix; g.C = C;
    add_expected(h, prefix + ".weight", {C});
    add_expected(h, prefix + ".bias", {C});
    return g;
}

static ResW make_res(use_handle* h, int idx, int in_ch, int out_ch, bool up, bool down) {
    const std::string p = "all_modules." + std::to_string(idx);
    const int dt = h->act_dtype;
    ResW r; r.idx = idx; r.in_ch = in_ch; r.out_ch = out_ch; r.up = up; r.down = down;
    r.gn0 = make_gn(h, p + ".GroupNorm_0", in_ch);
    r.c0 = make_conv(h, p + ".Conv_0", in_ch, out_ch, 9, dt);
    add_expected(h, p + ".Dense_0.weight", {out_ch, 4 * h->cfg.nf});
    add_expected(h, p + ".Dense_0.bias", {out_ch});
    r.dense_row0 = h->dense_rows; h->dense_rows += out_ch;
    r.gn1 = make_gn(h, p + ".GroupNorm_1", out_ch);
    r.c1 = make_conv(h, p + ".Conv_1", out_ch, out_ch, 9, dt);
    r.has_c2 = (in_ch != out_ch) || up || down;
    if (r.has_c2) r.c2 = make_conv(h, p + ".Conv_2", in_ch, out_ch, 1, dt);
    return r;
}

// Mirrors the module construction order of reference ncsnpp.py:181-316.
static int build_arch(use_handle* h) {
    const use_config& c = h->cfg;
    const int nf = c.nf, L = c.n_levels, nrb = c.num_res_blocks, dt = h->act_dtype;
    // pc real input / pyramid channels in the reference tensors; stored zero-padded to pcp = 4 (8 for the 6 channels of
    // condition="both", model_wrapper.py:43-46) everywhere in the engine
    const int pc = c.input_channels ? c.input_channels : 4;
    const int pcp = pc > 4 ? 8 : 4;
    h->pcp = pcp;
    add_expected(h, "output_layer.weight", {2, pc, 1, 1});
    add_expected(h, "output_layer.bias", {2});
    int m = 0;
    add_expected(h, "all_modules.0.W", {nf}); m++;          // the Fourier projection exists even when unconditional
    if (!c.unconditional) {
        add_expected(h, "all_modules.1.weight", {4 * nf, 2 * nf}); add_expected(h, "all_modules.1.bias", {4 * nf}); m++;
        add_expected(h, "all_modules.2.weight", {4 * nf, 4 * nf}); add_expected(h, "all_modules.2.bias", {4 * nf}); m++;
    }
    h->conv_in = make_conv(h, "all_modules." + std::to_string(m), pcp, nf, 9, DT_F32, pc, 0); m++;   // fp32 input always
    std::vector<int> hs_c{nf};
    int in_ch = nf;
    for (int lvl = 0; lvl < L; ++lvl) {
        for (int k = 0; k < nrb; ++k) {
            const int out_ch = nf * c.ch_mult[lvl];
            h->res.push_back(make_res(h, m++, in_ch, out_ch, false, false));
            in_ch = out_ch; hs_c.push_back(in_ch);
        }
        if (lvl != L - 1) {
            h->res.push_back(make_res(h, m++, in_ch, in_ch, false, true));
            CombineW cb; cb.idx = m; cb.C = in_ch;
            add_expected(h, "all_modules." + std::to_string(m) + ".Conv_0.weight", {in_ch, pc, 1, 1});
            add_expected(h, "all_modules." + std::to_string(m) + ".Conv_0.bias", {in_ch});
            h->combines.push_back(cb); m++;
            hs_c.push_back(in_ch);
        }
    }
    in_ch = hs_c.back();
    h->res.push_back(make_res(h, m++, in_ch, in_ch, false, false));
    {
        const std::string p = "all_modules." + std::to_string(m);
        h->attn.idx = m; h->attn.C = in_ch;
        h->attn.gn = make_gn(h, p + ".GroupNorm_0", in_ch);
        h->attn.q = make_nin(h, p + ".NIN_0", in_ch, dt);
        h->attn.k = make_nin(h, p + ".NIN_1", in_ch, dt);
        h->attn.v = make_nin(h, p + ".NIN_2", in_ch, dt);
        h->attn.o = make_nin(h, p + ".NIN_3", in_ch, dt);
        m++;
    }
    h->res.push_back(make_res(h, m++, in_ch, in_ch, false, false));
    for (int lvl = L - 1; lvl >= 0; --lvl) {
        for (int k = 0; k < nrb + 1; ++k) {
            const int out_ch = nf * c.ch_mult[lvl];
            const int skip = hs_c.back(); hs_c.pop_back();
            h->res.push_back(make_res(h, m++, in_ch + skip, out_ch, false, false));
            in_ch = out_ch;
        }
        PyrW pw;
        pw.gn = make_gn(h, "all_modules." + std::to_string(m), in_ch); m++;
        pw.conv = make_conv(h, "all_modules." + std::to_string(m), in_ch, pcp, 9, dt, 0, pc); m++;
        h->pyrs.push_back(pw);
        if (lvl != 0) h->res.push_back(make_res(h, m++, in_ch, in_ch, true, false));
    }
    if (!hs_c.empty()) return fail(USE_E_INVALID, "internal: skip stack not empty");

    // ---- device blob layout ----
    size_t off = 0;
    auto take = [&](size_t bytes) { off = (off + 255) & ~(size_t)255; size_t o = off; off += bytes; return o; };
    auto lay_conv = [&](ConvW& w) {
        w.w_off = take((size_t)w.ntaps * w.cout_pad * w.cin * dtype_size(w.w_dtype));
        w.b_off = take((size_t)w.cout * 4);
        // 3x3 convolutions and the res-block shortcuts fused into them get a second, slab-major copy
        w.has_wb = !w.nin && w.cout_pad % 128 == 0 && w.cin % conv_v4_chunk(w.w_dtype) == 0 && (w.ntaps == 9 || w.ntaps == 1);
        if (w.has_wb) w.wb_off = take((size_t)w.ntaps * w.cout_pad * w.cin * dtype_size(w.w_dtype));
    };
    // the input convolution in the 16-bit modes: split-bf16 copy [cout_pad][CONV_IN_SPLIT_K] for conv_in_split_kernel
    auto lay_conv_in = [&](ConvW& w) {
        lay_conv(w);
        if (dt != DT_F32 && w.cin == 4 && w.ntaps == 9 && w.cout_pad % 128 == 0) {
            w.split_in = true; w.has_wb = true;
            w.wb_off = take((size_t)w.cout_pad * CONV_IN_SPLIT_K * 2);
        }
    };
    auto lay_gn = [&](GNW& g) { g.g_off = take((size_t)g.C * 4); g.b_off = take((size_t)g.C * 4); };
    h->outw_off = take((size_t)2 * pcp * 4); h->outb_off = take(2 * 4);
    h->gfp_off = take((size_t)nf * 4);
    h->l1w_off = take((size_t)4 * nf * 2 * nf * 4); h->l1b_off = take((size_t)4 * nf * 4);
    h->l2w_off = take((size_t)4 * nf * 4 * nf * 4); h->l2b_off = take((size_t)4 * nf * 4);
    h->dense_w_off = take((size_t)h->dense_rows * 4 * nf * 4); h->dense_b_off = take((size_t)h->dense_rows * 4);
    lay_conv_in(h->conv_in);
    for (auto& r : h->res) {
        lay_gn(r.gn0); lay_conv(r.c0); lay_gn(r.gn1); lay_conv(r.c1);
        if (r.has_c2) { lay_conv(r.c2); r.b12_off = take((size_t)r.out_ch * 4); }
    }
    for (auto& cb : h->combines) { cb.w_off = take((size_t)cb.C * pcp * 4); cb.b_off = take((size_t)cb.C * 4); }
    lay_gn(h->attn.gn); lay_conv(h->attn.q); lay_conv(h->attn.k); lay_conv(h->attn.v); lay_conv(h->attn.o);
    for (auto& p : h->pyrs) { lay_gn(p.gn); lay_conv(p.conv); }
    h->blob_bytes = (off + 255) & ~(size_t)255;
    return USE_OK;
}

// ---------------------------------------------------------------------------------------------------------
// weight packing
// ---------------------------------------------------------------------------------------------------------
// host float weights -> device layouts: dst [cout_pad][tap][cin] (see use_kernels.h) and, when dstb != null, the slab-major
// copy [tap][chunk][cout_pad][ck] with piece-swizzled 64-byte rows (ConvArgs::wb)
static void pack_conv_raw(const float* src, const ConvW& w, char* dst, char* dstb) {
    const size_t es = dtype_size(w.w_dtype);
    auto put = [&](char* base, size_t o, float v) {
        if (w.w_dtype == DT_F32) ((float*)base)[o] = v;
        else ((uint16_t*)base)[o] = w.w_dtype == DT_F16 ? f32_to_f16(v) : f32_to_bf16(v);
    };
    memset(dst, 0, (size_t)w.ntaps * w.cout_pad * w.cin * es);
    for (int tap = 0; tap < w.ntaps; ++tap)
        for (int co = 0; co < w.cout_src; ++co)
            for (int ci = 0; ci < w.cin_src; ++ci) {
                // reference conv weight [cout][cin][kh][kw]; NIN W is [cin][cout] (layers.py:639-650)
                const float v = w.nin ? src[(size_t)ci * w.cout + co] : src[((size_t)co * w.cin_src + ci) * w.ntaps + tap];
                put(dst, ((size_t)co * w.ntaps + tap) * w.cin + ci, v);       // [cout][tap][cin]: see use_kernels.h
            }
    if (dstb) {                                               // [tap][chunk][cout_pad][ck]: one (tap, chunk) slab contiguous
        const int ck = conv_v4_chunk(w.w_dtype), nchunks = w.cin / ck;
        memset(dstb, 0, (size_t)w.ntaps * w.cout_pad * w.cin * es);
        for (int tap = 0; tap < w.ntaps; ++tap)
            for (int co = 0; co < w.cout_src; ++co)
                for (int ci = 0; ci < w.cin_src; ++ci) {
                    const float v = src[((size_t)co * w.cin_src + ci) * w.ntaps + tap];
                    const int vec = 16 / (int)es, e = ci % ck;             // 64-byte rows, 16-byte pieces swizzled by the row
                    put(dstb, (((size_t)tap * nchunks + ci / ck) * w.cout_pad + co) * ck + (((e / vec) ^ ((co >> 2) & 3)) * vec + e % vec), v);
                }
    }
}
// Input convolution, 16-bit modes: w = wh + wl with wh = bf16(w), wl = bf16(w - wh); row n of the copy holds the K = 112 operand
// of conv_in_split_kernel: k = 4 u + ci, unit u = (block, tap): block 0 -> wh (meets xh), block 1 -> wl (meets xh), block 2 -> wh
// (meets xl), unit 27 = zero padding.  x w = xh wh + xh wl + xl wh + O(2^-16 |x w|).
static void pack_conv_in_split(const float* src, const ConvW& w, char* dst) {
    uint16_t* d = (uint16_t*)dst;
    memset(dst, 0, (size_t)w.cout_pad * CONV_IN_SPLIT_K * 2);
    for (int co = 0; co < w.cout_src; ++co)
        for (int tap = 0; tap < 9; ++tap)
            for (int ci = 0; ci < w.cin_src; ++ci) {
                const float v = src[((size_t)co * w.cin_src + ci) * 9 + tap];     // reference conv weight [cout][cin][kh][kw]
                const uint16_t hi = f32_to_bf16(v);
                uint32_t hb = (uint32_t)hi << 16; float hf; memcpy(&hf, &hb, 4);
                const uint16_t lo = f32_to_bf16(v - hf);
                uint16_t* row = d + (size_t)co * CONV_IN_SPLIT_K;
                row[(0 * 9 + tap) * 4 + ci] = hi; row[(1 * 9 + tap) * 4 + ci] = lo; row[(2 * 9 + tap) * 4 + ci] = hi;
            }
}
static void pack_conv(const use_handle* h, const ConvW& w, char* blob) {
    const std::vector<float>& bias = h->host_w.at(w.bname);
    pack_conv_raw(h->host_w.at(w.wname).data(), w, blob + w.w_off, (w.has_wb && !w.split_in) ? blob + w.wb_off : nullptr);
    if (w.split_in) pack_conv_in_split(h->host_w.at(w.wname).data(), w, blob + w.wb_off);
    memset(blob + w.b_off, 0, (size_t)w.cout * 4);
    memcpy(blob + w.b_off, bias.data(), (size_t)w.cout_src * 4);
}
static void pack_gn(const use_handle* h, const GNW& g, char* blob) {
    memcpy(blob + g.g_off, h->host_w.at(g.prefix + ".weight").data(), (size_t)g.C * 4);
    memcpy(blob + g.b_off, h->host_w.at(g.prefix + ".bias").data(), (size_t)g.C * 4);
}

static int pack_all(use_handle* h, char* blob) {
    for (const auto& e : h->expected)
        if (!h->host_w.count(e.name)) return fail(USE_E_STATE, "weight '%s' was never set", e.name.c_str());
    const int nf = h->cfg.nf;
    auto cp = [&](size_t off, const char* name) {
        const auto& v = h->host_w.at(name); memcpy(blob + off, v.data(), v.size() * 4);
    };
    const int pc = h->cfg.input_channels ? h->cfg.input_channels : 4;
    const int pcp = h->pcp;
    auto cp_rows = [&](size_t off, const std::string& name, int rows) {     // [rows][pc] -> [rows][pcp], zero-padded
        const auto& v = h->host_w.at(name);
        float* d = (float*)(blob + off);
        for (int r = 0; r < rows; ++r)
            for (int k = 0; k < pcp; ++k) d[r * pcp + k] = k < pc ? v[(size_t)r * pc + k] : 0.f;
    };
    cp_rows(h->outw_off, "output_layer.weight", 2); cp(h->outb_off, "output_layer.bias");
    cp(h->gfp_off, "all_modules.0.W");
    if (!h->cfg.unconditional) {
        cp(h->l1w_off, "all_modules.1.weight"); cp(h->l1b_off, "all_modules.1.bias");
        cp(h->l2w_off, "all_modules.2.weight"); cp(h->l2b_off, "all_modules.2.bias");
    }
    pack_conv(h, h->conv_in, blob);
    for (const auto& r : h->res) {
        pack_gn(h, r.gn0, blob); pack_conv(h, r.c0, blob); pack_gn(h, r.gn1, blob); pack_conv(h, r.c1, blob);
        const std::string p = "all_modules." + std::to_string(r.idx);
        if (r.has_c2) {
            pack_conv(h, r.c2, blob);
            const auto& b1 = h->host_w.at(p + ".Conv_1.bias"); const auto& b2 = h->host_w.at(p + ".Conv_2.bias");
            float* d = (float*)(blob + r.b12_off);
            for (int i = 0; i < r.out_ch; ++i) d[i] = b1[i] + b2[i];
        }
        memcpy(blob + h->dense_w_off + (size_t)r.dense_row0 * 4 * nf * 4, h->host_w.at(p + ".Dense_0.weight").data(),
               (size_t)r.out_ch * 4 * nf * 4);
        memcpy(blob + h->dense_b_off + (size_t)r.dense_row0 * 4, h->host_w.at(p + ".Dense_0.bias").data(),
               (size_t)r.out_ch * 4);
    }
    for (const auto& cb : h->combines) {
        const std::string p = "all_modules." + std::to_string(cb.idx);
        cp_rows(cb.w_off, p + ".Conv_0.weight", cb.C); cp(cb.b_off, (p + ".Conv_0.bias").c_str());
    }
    pack_gn(h, h->attn.gn, blob);
    pack_conv(h, h->attn.q, blob); pack_conv(h, h->attn.k, blob); pack_conv(h, h->attn.v, blob); pack_conv(h, h->attn.o, blob);
    for (const auto& p : h->pyrs) { pack_gn(h, p.gn, blob); pack_conv(h, p.conv, blob); }
    return USE_OK;
}

// ---------------------------------------------------------------------------------------------------------
// forward pass (one score-network evaluation)
// ---------------------------------------------------------------------------------------------------------
static int g_subbatch_min_items = 2;              // use_set_option("subbatch_min_items", n): no sub-batch smaller than n items
static int g_subbatch = -1;                      // use_set_option("subbatch", n): sub-batches per evaluation (0 / 1: off; -1: by batch size, below)
// GroupNorm finalisation inside the consuming conv (no launch) for maps of at most g_gn_inline pixels per item, a separate
// finalize launch above: on the large maps thousands of workgroups would each redo the finalisation (measured slower), on the
// small, latency-bound maps the saved launch is what counts.  use_set_option("gn_inline", pixels); 0: never inline
static long g_gn_inline = 128L * 160L;
static int g_attn_fused = 1;                     // use_set_option("attn_fused", 0): the unfused attention block (3 NIN, core, NIN_3)
static int g_stats_part = 1;                     // use_set_option("stats_part", 0): GroupNorm totals by atomics on the large maps too
static int g_stagger_level = 2;                  // use_set_option("stagger_level", l): the next sub-batch starts after level l
static int g_trace = 0;                          // use_set_option("trace", 1): record every launch of an evaluation (use_trace_entry, use_hip.h)
static int g_sampler_trace = 0;                  // use_set_option("sampler_trace", 1): record every launch of the PC loop and snapshot what it overwrites (use_sampler_trace_entry)

// ---- launch trace: what each launch read and wrote, for the layer-by-layer tests.  Filled from the launch's own arguments ----
static use_trace_tensor trace_tensor(const void* p, int B, int H, int W, int C, int dtype) {
    use_trace_tensor t{}; t.ptr = p; t.dims[0] = B; t.dims[1] = H; t.dims[2] = W; t.dims[3] = C; t.dtype = dtype; return t;
}
static use_trace_entry trace_new(int kind, const char* kernel) {
    use_trace_entry e{}; e.kind = kind; snprintf(e.kernel, sizeof e.kernel, "%s", kernel); return e;
}
static const char* trace_pname(const use_handle* h, const std::string& name) {      // the handle's own copy of a state-dict key
    auto it = h->expected_index.find(name);
    return it == h->expected_index.end() ? nullptr : h->expected[it->second].name.c_str();
}
// entries ahead of Fwd::run (which drops what the previous evaluation left): the first of them starts the new list
static void trace_push_head(Plan& pl, const use_trace_entry& e) {
    if (!pl.trace_head) pl.trace.clear();
    pl.trace.push_back(e); pl.trace_head = pl.trace.size();
}

__global__ __launch_bounds__(256) void zero16_kernel(uint4* __restrict__ p, size_t n16) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) p[i] = make_uint4(0, 0, 0, 0);
}

struct Fwd {
    use_handle* h; Plan& pl; hipStream_t s;      // pl: the handle's current plan, or the one use_plan is sizing
    const float* tembias; int temb_bstride;     // [B or 1][dense_rows] (already offset to this sub-batch)
    const float* t; int t_stride;                 // per-item time (stride 0: shared)
    int B = 0;                                    // items of this (sub-)batch
    Arena* arena = nullptr;                       // its activation workspace
    Arena* st_arena = nullptr;                    // its GroupNorm-totals region
    bool primary = true;                          // the first sub-batch owns the FLOP count and the debug tensors
    hipEvent_t ev_stagger = nullptr;              // recorded when the large maps of the down path are done (or null)
    int stagger_level = 2;                        // ... i.e. after this level of the down path
    template <typename T> const T* W(size_t off) const { return (const T*)(h->blob + off); }

    use_trace_tensor tt(const Act& a) const { return trace_tensor(a.p, B, a.H, a.W, a.C, a.dtype); }

    Act new_act(int C, int H, int Wd, int dtype, bool stats) {
        Act a; a.C = C; a.H = H; a.W = Wd; a.dtype = dtype;
        a.p = arena->alloc((size_t)B * H * Wd * C * dtype_size(dtype));
        if (stats) a.stats = (long long*)st_arena->alloc((size_t)B * C * 2 * sizeof(long long));
        return a;
    }

    // use_profile_score: HIP events around one launch, recorded with its class, map and algorithmic bytes (every operand once); the record, or null
    template <typename F> use_handle::ProfRec* timed_aux(const char* name, int Hm, int Wm, double bytes, F&& launch) {
        if (!h->profile) { launch(); return nullptr; }
        use_handle::ProfRec r; r.label = name; r.H = Hm; r.W = Wm; r.bytes = bytes;
        (void)hipEventCreate(&r.e0); (void)hipEventCreate(&r.e1);
        (void)hipEventRecord(r.e0, s);
        launch();
        (void)hipEventRecord(r.e1, s);
        h->prof.push_back(std::move(r));
        return &h->prof.back();
    }

    // coefficient array for the consumers that cannot finalise the GroupNorm themselves (the FIR resampling kernels)
    float* gn_coef(const Act& a, const Act* a2, const GNW& g) {
        const int C = a.C + (a2 ? a2->C : 0);
        float* coef = (float*)arena->alloc((size_t)B * C * 2 * 4);
        if (g_trace && primary && !pl.dry) {
            const int groups = std::min(C / 4, 32);
            use_trace_entry e = trace_new(USE_TRACE_GN_FINALIZE, (a.part || (a2 && a2->part)) ? "gn_finalize_part" : "gn_finalize");
            e.in[0] = tt(a); e.totals_in[0] = a.stats; e.part_in[0] = a.part; e.parts_in[0] = a.ntiles;
            if (a2) { e.in[1] = tt(*a2); e.totals_in[1] = a2->stats; e.part_in[1] = a2->part; e.parts_in[1] = a2->ntiles; }
            e.coef_out = coef; e.gn_groups = groups; e.gn_inv_n = 1.0f / ((float)(C / groups) * (float)(a.H * a.W)); e.gn_eps = 1e-6f;
            e.params[USE_TP_GN_W] = trace_pname(h, g.prefix + ".weight"); e.params[USE_TP_GN_B] = trace_pname(h, g.prefix + ".bias");
            pl.trace.push_back(e);
        }
        if (!pl.dry)
            launch_gn_finalize(a.stats, a.C, a2 ? a2->stats : nullptr, a2 ? a2->C : 0, W<float>(g.g_off), W<float>(g.b_off),
                               std::min(C / 4, 32), a.H * a.W, 1e-6f, coef, B, s, a.part, a.ntiles, a2 ? a2->part : nullptr, a2 ? a2->ntiles : 0);
        return coef;
    }

    // the trace entry of one convolution launch, from the arguments it is about to be launched with
    void trace_conv(const ConvArgs& p, const ConvChoice& ch, const GNW* gn, const ConvW& w, const ConvW* w2, const CombineW* cb, int temb_row) {
        use_trace_entry e = trace_new(USE_TRACE_CONV, conv_kernel_name(ch.k));
        e.in[0] = trace_tensor(p.src0, p.B, p.H, p.W, p.C0, p.in_dtype);
        if (p.src1) e.in[1] = trace_tensor(p.src1, p.B, p.H, p.W, p.C1, p.in_dtype);
        if (p.x0) e.in[2] = trace_tensor(p.x0, p.B, p.H, p.W, p.XC0, p.in_dtype);
        if (p.x1) e.in[3] = trace_tensor(p.x1, p.B, p.H, p.W, p.XC1, p.in_dtype);
        if (p.res) e.in[4] = trace_tensor(p.res, p.B, p.H, p.W, p.Cout, p.out_dtype);
        if (p.pyr) e.in[5] = trace_tensor(p.pyr, p.B, p.H, p.W, h->pcp, DT_F32);
        e.out[0] = trace_tensor(p.out, p.B, p.H, p.W, p.Cout, p.out_dtype);
        e.totals_in[0] = p.gn_st0; e.totals_in[1] = p.gn_st1; e.coef = p.coef;
        e.totals_out = p.stats; e.part_out = p.stats_part; e.parts_out = p.stats_part ? ch.stats_parts : 0;
        if (p.temb) { e.tembias = tembias; e.temb_row = temb_row; e.temb_stride = p.temb_bstride; }
        e.act = p.act; e.out_scale = p.out_scale; e.ntaps = p.ntaps;
        if (p.gn_st0) { e.gn_groups = p.gn_groups; e.gn_inv_n = p.gn_inv_n; e.gn_eps = p.gn_eps; }
        e.params[USE_TP_W] = trace_pname(h, w.wname); e.params[USE_TP_B] = trace_pname(h, w.bname);
        if (w2) { e.params[USE_TP_W2] = trace_pname(h, w2->wname); e.params[USE_TP_B2] = trace_pname(h, w2->bname); }
        if (gn && p.gn_st0) { e.params[USE_TP_GN_W] = trace_pname(h, gn->prefix + ".weight"); e.params[USE_TP_GN_B] = trace_pname(h, gn->prefix + ".bias"); }
        if (cb) {
            const std::string c = "all_modules." + std::to_string(cb->idx) + ".Conv_0";
            e.params[USE_TP_CB_W] = trace_pname(h, c + ".weight"); e.params[USE_TP_CB_B] = trace_pname(h, c + ".bias");
        }
        if (p.temb)
            for (const ResW& r : h->res)
                if (r.dense_row0 == temb_row) {
                    const std::string d = "all_modules." + std::to_string(r.idx) + ".Dense_0";
                    e.params[USE_TP_DENSE_W] = trace_pname(h, d + ".weight"); e.params[USE_TP_DENSE_B] = trace_pname(h, d + ".bias");
                }
        pl.trace.push_back(e);
    }

    // gn != null: the input concat(a, a2) goes through this GroupNorm, finalised inside the conv kernel from the producers' totals
    // temb_row >= 0: + the Dense_0(temb) row of this sub-batch's tembias that starts there
    Act conv(const Act& a, const Act* a2, const GNW* gn, int act, const ConvW& w, int temb_row,
             const Act* res, float scale, const float* pyr, const CombineW* cb, int out_dtype, bool stats,
             const Act* sx0 = nullptr, const Act* sx1 = nullptr, const ConvW* w2 = nullptr, size_t bias_off = 0) {
        Act o = new_act(w.cout, a.H, a.W, out_dtype, stats);
        double fl = 2.0 * B * a.H * a.W * (double)w.cout * w.cin * w.ntaps;
        if (w2) fl += 2.0 * B * a.H * a.W * (double)w2->cout * w2->cin;
        pl.flops += fl;
        // large maps: separate finalize launch into a coefficient array (allocated in the dry run as well: the arena is sized by it)
        const bool large = (long)a.H * a.W > g_gn_inline;
        const float* coef_arr = (gn && large) ? gn_coef(a, a2, *gn) : nullptr;
        // The launch as the dispatcher sees it, from shapes and flags alone (the dry run has no pointers): the dry run and the real one ask
        // conv_choose with the same value, once, and its answer sizes the partial-totals buffer, picks stats_part or stats and labels the profile
        ConvDesc d{};
        d.H = a.H; d.W = a.W; d.C0 = a.C; d.C1 = a2 ? a2->C : 0; d.XC0 = w2 ? sx0->C : 0; d.XC1 = (w2 && sx1) ? sx1->C : 0;
        d.Cout = w.cout; d.cout_pad = w.cout_pad; d.ntaps = w.ntaps; d.in_dtype = a.dtype; d.out_dtype = out_dtype; d.act = act;
        d.coef = gn && large; d.w = true; d.wb = w.has_wb; d.w2 = w2 != nullptr; d.w2b = w2 && w2->has_wb;
        d.res = res != nullptr; d.pyr = cb != nullptr; d.temb = temb_row >= 0; d.stats = stats;
        const ConvChoice ch = conv_choose(d);
        // Large maps: the producer writes per-workgroup partial totals instead of queueing 640 atomics per item on each total (where its kernel
        // knows that form: ch.stats_parts workgroups per item); every consumer of such a map goes through gn_coef (same threshold), which sums them
        long long* part = (stats && g_stats_part && ch.stats_parts > 0 && large)
                              ? (long long*)arena->alloc((size_t)B * ch.stats_parts * w.cout * 2 * sizeof(long long)) : nullptr;
        if (pl.dry) return o;
        ConvArgs p{};
        p.src0 = a.p; p.C0 = a.C; p.src1 = a2 ? a2->p : nullptr; p.C1 = a2 ? a2->C : 0; p.in_dtype = a.dtype;
        p.coef = coef_arr; p.act = act; p.w = h->blob + w.w_off; p.cout_pad = w.cout_pad;
        if (gn && !coef_arr) {
            const int C = a.C + (a2 ? a2->C : 0), groups = std::min(C / 4, 32);
            p.gn_st0 = a.stats; p.gn_st1 = a2 ? a2->stats : nullptr;
            p.gn_gamma = W<float>(gn->g_off); p.gn_beta = W<float>(gn->b_off); p.gn_groups = groups;
            p.gn_inv_n = 1.0f / ((float)(C / groups) * (float)(a.H * a.W)); p.gn_eps = 1e-6f;
        }
        p.wb = w.has_wb ? h->blob + w.wb_off : nullptr;
        p.bias = W<float>(w2 ? bias_off : w.b_off);
        if (w2) { p.x0 = sx0->p; p.XC0 = sx0->C; p.x1 = sx1 ? sx1->p : nullptr; p.XC1 = sx1 ? sx1->C : 0; p.w2 = h->blob + w2->w_off;
                  p.w2b = w2->has_wb ? h->blob + w2->wb_off : nullptr; }
        p.temb = temb_row >= 0 ? tembias + temb_row : nullptr; p.temb_bstride = temb_bstride;
        p.res = res ? res->p : nullptr; p.out_scale = scale;
        p.pyr = pyr; p.w4 = cb ? W<float>(cb->w_off) : nullptr; p.b4 = cb ? W<float>(cb->b_off) : nullptr;
        p.out = o.p; p.out_dtype = out_dtype;
        if (part) { p.stats_part = part; o.part = part; o.ntiles = ch.stats_parts; } else p.stats = o.stats;
        p.B = B; p.H = a.H; p.W = a.W; p.Cout = w.cout; p.ntaps = w.ntaps;
        // consumers that read the totals directly (inline GroupNorm below gn_inline pixels, the fused attention) must never meet a producer
        // that wrote partial totals instead: both sides test the same H * W > gn_inline - checked here, where the input is consumed
        if (gn && !coef_arr && (a.part || (a2 && a2->part))) { arena->overflow = true; pl.dry = true; return o; }   // reported by eval_status as a stale plan
        if (g_trace && primary) trace_conv(p, ch, gn, w, w2, cb, temb_row);
        const bool main_variant = ch.k == WIDE32 || ch.k == WIDE16;           // the dominant kernel (conv_wide_kernel, large maps)
        if (!h->profile || (w.ntaps != 9 && !ch.hbm)) { launch_conv(p, s); return o; }       // (the 1x1 convolutions are not timed)
        // algorithmic HBM bytes of this launch: every operand once (input, shortcut input, residual, output, weights; the dominant kernel's Combine input)
        const double es = (double)dtype_size(a.dtype), px = (double)B * a.H * a.W;
        double by = px * (w.cin + (w2 ? w2->cin : 0)) * es + px * w.cout * dtype_size(out_dtype) * (res ? 2.0 : 1.0);
        by += (double)w.ntaps * w.cin * w.cout * es + (w2 ? (double)w2->cin * w2->cout * es : 0.0);
        if (pyr && main_variant) by += px * 4 * 4;
        use_handle::ProfRec* r = timed_aux(ch.label, a.H, a.W, by, [&] { launch_conv(p, s); });
        r->main = main_variant; r->flops = ch.hbm ? 0.0 : fl;          // (HBM-bound layers: no FLOPs in their records)
        // listed by USE_HIP_PROFILE_VERBOSE: the dominant kernel's launches and whatever conv_v2 could run (its own launches and, as before, those conv_sk took from it)
        if (main_variant || (h->profile_all && conv_v2_eligible(d))) {
            char t[160]; snprintf(t, sizeof t, "%-28s H=%3d W=%3d Cin=%3d Cout=%3d taps=%d gn=%d res=%d sc=%d", w.wname.c_str(), a.H, a.W, w.cin, w.cout, w.ntaps, gn != nullptr, res != nullptr, w2 ? w2->cin : 0);
            r->desc = t;
        }
        return o;
    }

    // ResnetBlockBigGANpp.forward (reference layerspp.py:282-314). `skip` = second half of the channel concat.
    Act resblock(const Act& x, const Act* skip, const ResW& r, const float* pyr = nullptr, const CombineW* cb = nullptr) {
        const float rs = 0.70710678118654752440f;   // 1/sqrt(2)
        const int temb = h->cfg.unconditional ? -1 : r.dense_row0;         // unconditional: no Dense_0(temb) term
        const int dt = h->act_dtype;
        Act hcur, xr;
        const Act* sx0 = &x; const Act* sx1 = skip;          // inputs of the 1x1 shortcut (Conv_2)
        if (r.up || r.down) {
            const int H2 = r.up ? x.H * 2 : x.H / 2, W2 = r.up ? x.W * 2 : x.W / 2;
            Act hr = new_act(x.C, H2, W2, dt, false);
            xr = new_act(x.C, H2, W2, dt, false);
            float* coef0 = gn_coef(x, skip, r.gn0);          // the resampling kernels take the GroupNorm as a coefficient array
            if (g_trace && primary && !pl.dry) {
                use_trace_entry e = trace_new(r.up ? USE_TRACE_FIR_UP : USE_TRACE_FIR_DOWN, r.up ? "fir_up" : "fir_down");
                e.in[0] = tt(x); e.out[0] = tt(hr); e.out[1] = tt(xr); e.coef = coef0; e.act = 1;
                pl.trace.push_back(e);
            }
            if (!pl.dry) {
                // reads the map once, writes the activated and the raw resampled copy
                const double by = (double)B * x.H * x.W * x.C * dtype_size(dt) + 2.0 * B * H2 * W2 * x.C * dtype_size(dt);
                if (r.up) timed_aux("fir_up", x.H, x.W, by, [&] { launch_fir_up2(x.p, dt, coef0, 1, hr.p, xr.p, B, x.H, x.W, x.C, s); });
                else      timed_aux("fir_down", x.H, x.W, by, [&] { launch_fir_down2(x.p, dt, coef0, 1, hr.p, xr.p, B, x.H, x.W, x.C, s); });
            }
            hcur = conv(hr, nullptr, nullptr, 0, r.c0, temb, nullptr, 1.f, nullptr, nullptr, dt, true);
            sx0 = &xr; sx1 = nullptr;
        } else {
            hcur = conv(x, skip, &r.gn0, 1, r.c0, temb, nullptr, 1.f, nullptr, nullptr, dt, true);
        }
        if (r.has_c2)   // Conv_1 and the Conv_2 shortcut accumulate into the same MFMA tile (one K loop)
            return conv(hcur, nullptr, &r.gn1, 1, r.c1, -1, nullptr, rs, pyr, cb, dt, true, sx0, sx1, &r.c2, r.b12_off);
        return conv(hcur, nullptr, &r.gn1, 1, r.c1, -1, &x, rs, pyr, cb, dt, true);
    }

    // the trace entries of the GEMM form of the attention core (launch_attention_gemm calls this in front of each of its launches): a
    // GEMM's from the ConvArgs it is about to be launched with and the very conv_choose(conv_desc(p)) launch_conv evaluates
    struct AttnGemmTrace { Fwd* f; int N, C, dt; };
    static void trace_attn_gemm(void* ctx, int stage, const ConvArgs* p, const void* in, const void* out) {
        const AttnGemmTrace& c = *(const AttnGemmTrace*)ctx;
        Fwd& f = *c.f;
        use_trace_entry e{};
        if (stage == ATTN_GEMM_TRANSPOSE) {
            e = trace_new(USE_TRACE_TRANSPOSE, "transpose_nc");
            e.in[0] = trace_tensor(in, f.B, 1, c.N, c.C, c.dt); e.out[0] = trace_tensor(out, f.B, 1, c.C, c.N, c.dt);
        } else if (stage == ATTN_GEMM_SOFTMAX) {
            e = trace_new(USE_TRACE_SOFTMAX_ROWS, "softmax_rows");
            e.in[0] = e.out[0] = trace_tensor(out, f.B, c.N, 1, c.N, c.dt);
        } else {
            e = trace_new(USE_TRACE_ATTN_GEMM, conv_kernel_name(conv_choose(conv_desc(*p)).k));
            e.in[0] = trace_tensor(p->src0, 1, p->H, p->W, p->C0, p->in_dtype);
            e.in[1] = trace_tensor(p->w, 1, 1, p->Cout, p->C0, p->in_dtype);
            e.out[0] = trace_tensor(p->out, 1, p->H, p->W, p->Cout, p->out_dtype);
            e.act = p->act; e.out_scale = p->out_scale; e.ntaps = p->ntaps;
        }
        f.pl.trace.push_back(e);
    }

    // AttnBlockpp.forward (reference layerspp.py:77-93)
    Act attention(const Act& x, const AttnW& aw) {
        const int dt = h->act_dtype;
        if (g_attn_fused && x.stats && attn_fused_eligible(dt, x.H * x.W, x.C)) {       // one launch, MFMA contractions (use_attn.hip)
            Act o = new_act(x.C, x.H, x.W, dt, true);
            pl.flops += 4.0 * 2.0 * B * x.H * x.W * (double)x.C * x.C;                  // the four NIN, as the unfused path counts them
            if (pl.dry) return o;
            if (x.part) { arena->overflow = true; pl.dry = true; return o; }   // (the fused block reads x.stats: a producer with partial totals cannot feed it)
            AttnArgs a{};
            a.x = x.p; a.out = o.p; a.N = x.H * x.W;
            a.gn_st = x.stats; a.gn_gamma = W<float>(aw.gn.g_off); a.gn_beta = W<float>(aw.gn.b_off); a.gn_groups = std::min(x.C / 4, 32); a.gn_eps = 1e-6f;
            a.wq = h->blob + aw.q.w_off; a.wk = h->blob + aw.k.w_off; a.wv = h->blob + aw.v.w_off; a.wo = h->blob + aw.o.w_off;
            a.bq = W<float>(aw.q.b_off); a.bk = W<float>(aw.k.b_off); a.bv = W<float>(aw.v.b_off); a.bo = W<float>(aw.o.b_off);
            a.stats = o.stats;
            if (g_trace && primary) {
                use_trace_entry e = trace_new(USE_TRACE_ATTN_FUSED, "attn_fused");
                e.in[0] = tt(x); e.out[0] = tt(o); e.totals_in[0] = a.gn_st; e.totals_out = a.stats;
                e.gn_groups = a.gn_groups; e.gn_inv_n = 1.0f / ((float)(x.C / a.gn_groups) * (float)a.N); e.gn_eps = a.gn_eps;   // (inv_n: the kernel's own, from N and C)
                e.out_scale = 0.70710678118654752440f;
                e.params[USE_TP_GN_W] = trace_pname(h, aw.gn.prefix + ".weight"); e.params[USE_TP_GN_B] = trace_pname(h, aw.gn.prefix + ".bias");
                e.params[USE_TP_W] = trace_pname(h, aw.q.wname); e.params[USE_TP_B] = trace_pname(h, aw.q.bname);
                e.params[USE_TP_X0] = trace_pname(h, aw.k.wname); e.params[USE_TP_X1] = trace_pname(h, aw.k.bname);
                e.params[USE_TP_X2] = trace_pname(h, aw.v.wname); e.params[USE_TP_X3] = trace_pname(h, aw.v.bname);
                e.params[USE_TP_X4] = trace_pname(h, aw.o.wname); e.params[USE_TP_X5] = trace_pname(h, aw.o.bname);
                pl.trace.push_back(e);
            }
            launch_attn_fused(a, dt, B, s);
            return o;
        }
        Act q = conv(x, nullptr, &aw.gn, 0, aw.q, -1, nullptr, 1.f, nullptr, nullptr, dt, false);
        Act k = conv(x, nullptr, &aw.gn, 0, aw.k, -1, nullptr, 1.f, nullptr, nullptr, dt, false);
        Act v = conv(x, nullptr, &aw.gn, 0, aw.v, -1, nullptr, 1.f, nullptr, nullptr, dt, false);
        Act a = new_act(x.C, x.H, x.W, dt, false);
        const int N = x.H * x.W;
        if (attention_gemm_eligible(dt, N, x.C)) {
            // long sequences (64x80 bottleneck of the refine generator): per batch item two implicit GEMMs on the kernel conv_choose
            // answers for each (launch_attention_gemm, use_kernels.hip)
            const size_t es = dtype_size(dt);
            char* sc = (char*)arena->alloc((size_t)B * N * N * es);           // scores -> probabilities, [B][N][N]
            char* vt = (char*)arena->alloc((size_t)B * x.C * N * es);         // [B][C][N]
            if (!pl.dry) {
                AttnGemmTrace tc{this, N, x.C, dt};
                launch_attention_gemm(q.p, k.p, v.p, a.p, sc, vt, dt, B, x.H, x.W, x.C, s, (g_trace && primary) ? &trace_attn_gemm : nullptr, &tc);
            }
        } else if (!pl.dry) {
            if (g_trace && primary) {
                use_trace_entry e = trace_new(USE_TRACE_ATTN_CORE, "attention");
                e.in[0] = tt(q); e.in[1] = tt(k); e.in[2] = tt(v); e.out[0] = tt(a);
                pl.trace.push_back(e);
            }
            launch_attention(q.p, k.p, v.p, a.p, dt, B, N, x.C, s);
        }
        return conv(a, nullptr, nullptr, 0, aw.o, -1, &x, 0.70710678118654752440f, nullptr, nullptr, dt, true);
    }

    // NCSNpp.forward (reference ncsnpp.py:324-501): x4 = packed network input, returns the fp32 pyramid [B,F,T,4]
    Act run(const float* x4) {
        use_handle* H = h;
        const use_config& c = H->cfg;
        const int L = c.n_levels, nrb = c.num_res_blocks, dt = H->act_dtype;
        arena->reset();
        st_arena->reset();
        // all GroupNorm totals of this evaluation; a kernel, not hipMemsetAsync: a captured memset node of this (small) size does not
        // clear the region again on the second replay of a graph that holds four or more evaluations (ROCm 7.2; seen as NaN from the
        // second sampler call on for batches of 1-3 items, i.e. without the sub-batch split)
        if (!pl.dry && st_arena->base) {
            const size_t n16 = st_arena->cap / 16;
            hipLaunchKernelGGL(zero16_kernel, dim3((unsigned)std::min<size_t>((n16 + 255) / 256, 1024)), dim3(256), 0, s, (uint4*)st_arena->base, n16);
        }
        if (primary) { pl.flops = 0.0; pl.debug.clear(); pl.debug_B = B; pl.trace.resize(pl.trace_head); pl.trace_head = 0; }
        const int pcp = H->pcp;
        Act xin; xin.p = (void*)x4; xin.C = pcp; xin.H = c.n_freq; xin.W = pl.T; xin.dtype = DT_F32;
        std::vector<Act> hs;
        hs.push_back(conv(xin, nullptr, nullptr, 0, H->conv_in, -1, nullptr, 1.f, nullptr, nullptr, dt, true));
        if (primary) pl.debug["h_in"] = hs.back();
        Act ipyr = xin;
        size_t ri = 0, ci = 0;
        for (int lvl = 0; lvl < L; ++lvl) {
            for (int k = 0; k < nrb; ++k) hs.push_back(resblock(hs.back(), nullptr, H->res[ri++]));
            if (lvl == std::min(stagger_level, L - 1) && ev_stagger && !pl.dry) (void)hipEventRecord(ev_stagger, s);   // small maps follow
            if (lvl != L - 1) {
                Act nip = new_act(pcp, ipyr.H / 2, ipyr.W / 2, DT_F32, false);        // pyramid_downsample
                if (g_trace && primary && !pl.dry) {
                    use_trace_entry e = trace_new(USE_TRACE_FIR_DOWN, "fir_down");
                    e.in[0] = tt(ipyr); e.out[1] = tt(nip);
                    pl.trace.push_back(e);
                }
                if (!pl.dry) launch_fir_down2(ipyr.p, DT_F32, nullptr, 0, nullptr, nip.p, B, ipyr.H, ipyr.W, pcp, s);
                ipyr = nip;
                if (pcp == 4) {                                // Combine fused into the block's last convolution
                    hs.push_back(resblock(hs.back(), nullptr, H->res[ri++], (const float*)ipyr.p, &H->combines[ci++]));
                } else {                                       // 6-channel input: Combine as its own pass over the block's output
                    Act o = resblock(hs.back(), nullptr, H->res[ri++]);
                    const CombineW& cb = H->combines[ci++];
                    if (g_trace && primary && !pl.dry) {
                        use_trace_entry e = trace_new(USE_TRACE_COMBINE_ADD, "combine_add");
                        e.in[0] = tt(o); e.in[5] = tt(ipyr); e.out[0] = tt(o); e.totals_out = o.stats;
                        const std::string cn = "all_modules." + std::to_string(cb.idx) + ".Conv_0";
                        e.params[USE_TP_CB_W] = trace_pname(h, cn + ".weight"); e.params[USE_TP_CB_B] = trace_pname(h, cn + ".bias");
                        pl.trace.push_back(e);
                    }
                    if (!pl.dry) {
                        hipLaunchKernelGGL(zero16_kernel, dim3((unsigned)(((size_t)B * o.C + 255) / 256)), dim3(256), 0, s, (uint4*)o.stats,
                                           (size_t)B * o.C);                                             // totals of the combined map (16 bytes per channel)
                        launch_combine_add(o.p, o.dtype, (const float*)ipyr.p, W<float>(cb.w_off), W<float>(cb.b_off), o.stats, B,
                                           (long)o.H * o.W, o.C, s);
                    }
                    o.part = nullptr; o.ntiles = 0;            // (the totals of the combined map are what the consumers read)
                    hs.push_back(o);
                }
            }
        }
        if (primary) pl.debug["down_out"] = hs.back();
        Act hc = resblock(hs.back(), nullptr, H->res[ri++]);
        if (primary) pl.debug["pre_attn"] = hc;
        hc = attention(hc, H->attn);
        if (primary) pl.debug["post_attn"] = hc;
        hc = resblock(hc, nullptr, H->res[ri++]);
        Act pyr; bool have_pyr = false; size_t pi = 0;
        for (int lvl = L - 1; lvl >= 0; --lvl) {
            for (int k = 0; k < nrb + 1; ++k) {
                Act sk = hs.back(); hs.pop_back();
                hc = resblock(hc, &sk, H->res[ri++]);
            }
            const PyrW& pw = H->pyrs[pi++];
            if (!have_pyr) {
                pyr = conv(hc, nullptr, &pw.gn, 1, pw.conv, -1, nullptr, 1.f, nullptr, nullptr, DT_F32, false);
                have_pyr = true;
            } else {
                Act up = new_act(pcp, pyr.H * 2, pyr.W * 2, DT_F32, false);             // pyramid_upsample
                if (g_trace && primary && !pl.dry) {
                    use_trace_entry e = trace_new(USE_TRACE_FIR_UP, "fir_up");
                    e.in[0] = tt(pyr); e.out[1] = tt(up);
                    pl.trace.push_back(e);
                }
                if (!pl.dry) launch_fir_up2(pyr.p, DT_F32, nullptr, 0, nullptr, up.p, B, pyr.H, pyr.W, pcp, s);
                pyr = conv(hc, nullptr, &pw.gn, 1, pw.conv, -1, &up, 1.f, nullptr, nullptr, DT_F32, false);
            }
            if (lvl != 0) hc = resblock(hc, nullptr, H->res[ri++]);
        }
        if (primary) pl.debug["h_last"] = hc;
        if (primary) pl.debug["pyramid"] = pyr;
        return pyr;
    }
};

// time embedding for `rows` time values (batch items, or sampler steps) -> tembias[rows][dense_rows]
static void run_temb(use_handle* h, const float* t, int n, float* silu_buf, float* out, hipStream_t s) {
    const int nf = h->cfg.nf;
    if (g_trace && h->plan && !h->plan->dry) {
        use_trace_entry e = trace_new(USE_TRACE_TEMB, "temb_mlp+temb_dense");
        e.t = t; e.t_stride = 1;
        e.out[0] = trace_tensor(out, n, 1, 1, h->dense_rows, DT_F32); e.out[1] = trace_tensor(silu_buf, n, 1, 1, 4 * nf, DT_F32);
        e.params[USE_TP_W] = trace_pname(h, "all_modules.0.W");
        e.params[USE_TP_X0] = trace_pname(h, "all_modules.1.weight"); e.params[USE_TP_X1] = trace_pname(h, "all_modules.1.bias");
        e.params[USE_TP_X2] = trace_pname(h, "all_modules.2.weight"); e.params[USE_TP_X3] = trace_pname(h, "all_modules.2.bias");
        trace_push_head(*h->plan, e);
    }
    launch_temb_mlp(t, 1, (const float*)(h->blob + h->gfp_off), (const float*)(h->blob + h->l1w_off),
                    (const float*)(h->blob + h->l1b_off), (const float*)(h->blob + h->l2w_off),
                    (const float*)(h->blob + h->l2b_off), silu_buf, n, nf, s);
    launch_temb_dense(silu_buf, (const float*)(h->blob + h->dense_w_off), (const float*)(h->blob + h->dense_b_off), out,
                      n, h->dense_rows, 4 * nf, s);
}

static void trace_score_out(use_handle* h, Plan& pl, const Act& pyr, int B, const float* t, int t_stride, const float2* out, float sign) {
    use_trace_entry e = trace_new(USE_TRACE_SCORE_OUT, "score_out");
    e.in[0] = trace_tensor(pyr.p, B, pyr.H, pyr.W, pyr.C, pyr.dtype);
    e.out[0] = trace_tensor(out, B, pyr.H, pyr.W, 2, DT_F32);
    e.t = t; e.t_stride = t_stride; e.out_scale = sign;
    e.params[USE_TP_W] = trace_pname(h, "output_layer.weight"); e.params[USE_TP_B] = trace_pname(h, "output_layer.bias");
    pl.trace.push_back(e);
}

// score = -net(cat[x, y], t): x, y device complex64
static void run_score(use_handle* h, const float2* x, const float2* y, const float* tembias, int temb_bstride,
                      const float* t, int t_stride, float2* out, hipStream_t s, float sign = -1.f, const float2* y2 = nullptr) {
    Plan& pl = *h->plan;
    if (h->cfg.no_sigma_scale) t = nullptr;                   // score_out: no division by t
    const long n_per_b = (long)h->cfg.n_freq * pl.T;
    const int pcp = h->pcp;
    if (g_trace && !pl.dry) {
        use_trace_entry e = trace_new(USE_TRACE_PACK_INPUT, "pack_input");
        e.in[0] = trace_tensor(x, pl.B, h->cfg.n_freq, pl.T, 2, DT_F32);
        if (y) e.in[1] = trace_tensor(y, pl.B, h->cfg.n_freq, pl.T, 2, DT_F32);
        if (y2) e.in[2] = trace_tensor(y2, pl.B, h->cfg.n_freq, pl.T, 2, DT_F32);
        e.out[0] = trace_tensor(pl.x4, pl.B, h->cfg.n_freq, pl.T, pcp, DT_F32);
        trace_push_head(pl, e);
    }
    launch_pack_input(x, y, y2, pl.x4, (long)pl.B * n_per_b, s);
    const float* outw = (const float*)(h->blob + h->outw_off); const float* outb = (const float*)(h->blob + h->outb_off);
    if (pl.nsub == 1) {
        Fwd f0{h, pl, s, tembias, temb_bstride, t, t_stride};
        f0.B = pl.B; f0.arena = &pl.arena; f0.st_arena = &pl.st_arena[0];
        Act pyr = f0.run(pl.x4);
        if (g_trace && !pl.dry) trace_score_out(h, pl, pyr, pl.B, t, t_stride, out, sign);
        if (!pl.dry) launch_score_out((const float*)pyr.p, pcp, t, t_stride, outw, outb, out, pl.B, n_per_b, sign, s);
        return;
    }
    // Sub-batches on separate streams.  The items are independent inside the network (GroupNorm is per item), so this is
    // a pure re-scheduling: sub-batch i+1 starts when sub-batch i has finished its large down-path maps, and from then on
    // the latency-bound kernels of one sub-batch (small maps, GroupNorm finalisation, attention: a few workgroups each)
    // execute beside the large convolutions of another instead of leaving the chip idle.
    const bool overlap = !h->profile;                         // per-launch timing wants the kernels one at a time
    if (overlap) (void)hipEventRecord(h->ev_fork, s);
    int b0 = 0;
    for (int i = 0; i < pl.nsub; ++i) {
        hipStream_t si = (i == 0 || !overlap) ? s : h->aux_stream[i];
        if (overlap && i) {
            (void)hipStreamWaitEvent(si, h->ev_fork, 0);
            (void)hipStreamWaitEvent(si, h->ev_stagger[i - 1], 0);
        }
        Fwd f{h, pl, si, tembias ? tembias + (size_t)b0 * temb_bstride : nullptr, temb_bstride,
              t ? t + (size_t)b0 * t_stride : nullptr, t_stride};
        f.B = pl.sub_B[i]; f.arena = i ? &pl.sub_arena[i] : &pl.arena; f.st_arena = &pl.st_arena[i]; f.primary = i == 0;
        if (overlap && i + 1 < pl.nsub) { f.ev_stagger = h->ev_stagger[i]; f.stagger_level = g_stagger_level; }
        Act pyr = f.run(pl.x4 + (size_t)b0 * n_per_b * pcp);
        if (g_trace && i == 0 && !pl.dry) trace_score_out(h, pl, pyr, pl.sub_B[0], t, t_stride, out, sign);
        if (!pl.dry)
        launch_score_out((const float*)pyr.p, pcp, t ? t + (size_t)b0 * t_stride : nullptr, t_stride, outw, outb,
                         out + (size_t)b0 * n_per_b, pl.sub_B[i], n_per_b, sign, si);
        if (overlap && i) (void)hipEventRecord(h->ev_join[i], si);
        b0 += pl.sub_B[i];
    }
    if (overlap)
        for (int i = 1; i < pl.nsub; ++i) (void)hipStreamWaitEvent(s, h->ev_join[i], 0);
}

// ---------------------------------------------------------------------------------------------------------
// SDE scalars (reference sdes.py:205-243, 88-92)
// ---------------------------------------------------------------------------------------------------------
static double ouve_logsig(const use_config& c) { return std::log((double)c.sigma_max / (double)c.sigma_min); }
static float ouve_std(const use_config& c, float t) {
    const double th = c.theta, ls = ouve_logsig(c), sm = c.sigma_min, tt = t;
    return (float)std::sqrt(sm * sm * std::exp(-2 * th * tt) * (std::exp(2 * (th + ls) * tt) - 1) * ls / (th + ls));
}
static float ouve_diffusion(const use_config& c, float t) {
    const float sigma = c.sigma_min * std::pow(c.sigma_max / c.sigma_min, t);     // float32 like the reference
    return (float)((double)sigma * std::sqrt(2 * ouve_logsig(c)));
}
// torch.linspace(start, end, steps) float32 CPU semantics: symmetric fill from both ends, each element one fused
// multiply-add (matches the ATen CPU kernel bit-for-bit on the build container for N in 1..200)
static void linspace_f32(float start, float end, int steps, std::vector<float>& out) {
    out.resize(steps);
    if (steps == 1) { out[0] = start; return; }
    const float step = (end - start) / (float)(steps - 1);
    const int half = steps / 2;
    for (int i = 0; i < steps; ++i) out[i] = i < half ? std::fmaf(step, (float)i, start) : std::fmaf(-step, (float)(steps - 1 - i), end);
}

static void predictor_coeffs(const use_config& c, int predictor, float t, int N, float& cd, float& cs, float& cn) {
    const float g = ouve_diffusion(c, t);
    if (predictor == USE_PRED_REVERSE_DIFFUSION) {            // predictors.py:61-68 over sdes.py:88-92,159-173
        const float dt = (float)(1.0 / N);
        const float G = g * std::sqrt(dt);
        cd = c.theta * dt; cs = G * G; cn = G;
    } else {                                                  // Euler-Maruyama: predictors.py:44-53, sdes.py:125-157
        const double dt = 1.0 / N;
        cd = (float)(c.theta * dt); cs = (float)((double)(g * g) * dt); cn = (float)((double)g * std::sqrt(dt));
    }
}

// ---------------------------------------------------------------------------------------------------------
// the PC loop (reference sampling/__init__.py:59-71)
// ---------------------------------------------------------------------------------------------------------
__global__ void set_rng_kernel(unsigned long long* seeds, unsigned long long seed) { seeds[0] = seed; }
__global__ void fill_f32_kernel(float* p, float v, int n) { for (int i = threadIdx.x; i < n; i += blockDim.x) p[i] = v; }

// steps [i0, i1) of the loop (i0 == 0: preceded by the prior sampling); the whole loop is run_sampler(h, noise, s, 0, N).
// per_item (use_sample_items): the SDE updates address the batch as B items - item b's noise from pl.seeds[b], its own
// Langevin step - instead of one item of all n elements; the score evaluations and the stream schedule are the same.
static void run_sampler(use_handle* h, const float2* noise, hipStream_t s, int i0, int i1, bool per_item = false) {
    Plan& pl = *h->plan;
    const use_sampler_config& sc = pl.sc;
    const long n = (long)pl.B * h->cfg.n_freq * pl.T, n_per_b = (long)h->cfg.n_freq * pl.T;
    const int items = per_item ? pl.B : 1;
    const long n_per_item = n / items;
    const int ncorr = sc.corrector == USE_CORR_NONE ? 0 : sc.corrector_steps;
    // the network's kernel choice must not see the (sub-)batch size either: an item of a sub-batch of 3 has to get the bits it gets alone
    struct PerImage { bool on; PerImage(bool o) : on(o) { if (on) conv_sk_set_per_image(true); } ~PerImage() { if (on) conv_sk_set_per_image(false); } } per_image(per_item);
    auto nz = [&](unsigned d) { return noise ? noise + (size_t)d * n : nullptr; };
    unsigned d = 1 + (unsigned)i0 * (unsigned)(ncorr + (sc.predictor == USE_PRED_NONE ? 0 : 1));   // noise draws consumed so far
    // The sampler step trace (use_sampler_trace_entry, use_hip.h): every `if (tr)` below records the launch above it and copies what it
    // wrote, on this stream; off, the loop issues what it always did.  The segments of one call run (or are captured) in order, so the
    // list, the bump offset and the newest snapshots carry over from one segment to the next.
    const bool tr = pl.strace_rec >= 0;
    auto rec = [&](int kind, int i, int k, int dd, float t) -> use_sampler_trace_entry& {
        use_sampler_trace_entry e{};
        e.kind = kind; e.i = i; e.k = k; e.d = dd; e.t = t;
        e.items = items; e.n_per_item = n_per_item; e.per_item = per_item ? 1 : 0;
        pl.strace[pl.strace_rec].push_back(e);
        return pl.strace[pl.strace_rec].back();
    };
    auto snap = [&](const void* src, size_t bytes) -> const void* {
        const size_t step = (bytes + 255) / 256 * 256;
        if (pl.strace_off + step > pl.strace_bytes) return nullptr;       // (sized by strace_need from the same counts: never a write past the buffer)
        char* dst = pl.strace_buf + pl.strace_off;
        pl.strace_off += step;
        (void)hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s);
        return dst;
    };
    if (tr && i0 == 0) { pl.strace[pl.strace_rec].clear(); pl.strace_off = 0; pl.strace_x = pl.strace_score = nullptr; pl.strace_step = nullptr; }
    if (i0 == 0) {
        const float std1 = ouve_std(h->cfg, 1.0f);
        launch_prior(pl.Y, nz(0), SdeRng{pl.seeds, 0}, std1, pl.X, items, n_per_item, s);
        if (tr) {
            use_sampler_trace_entry& e = rec(USE_STRACE_PRIOR, -1, -1, 0, 1.0f);
            e.std1 = std1; e.noise = nz(0); e.x_out = pl.strace_x = (const float2*)snap(pl.X, (size_t)n * 8);
        }
    }
    for (int i = i0; i < i1; ++i) {
        const float t = pl.timesteps[i];
        const float* temb = pl.temb_table + (size_t)i * h->dense_rows;
        for (int k = 0; k < ncorr; ++k) {
            run_score(h, pl.X, pl.Cond, temb, 0, pl.ts_dev + i, 0, pl.score, s, -1.f, h->pcp == 8 ? pl.cond2_buf : nullptr);
            if (tr) {
                use_sampler_trace_entry& e = rec(USE_STRACE_SCORE, i, k, -1, t);
                e.x_in = pl.strace_x; e.score = pl.strace_score = (const float2*)snap(pl.score, (size_t)n * 8);
            }
            const SdeRng rng{pl.seeds, d};
            if (sc.corrector == USE_CORR_LANGEVIN) {
                launch_langevin_norms(pl.score, nz(d), rng, per_item, pl.lang_partial, pl.B, n_per_b, pl.lang_blocks, s);
                if (tr) {
                    use_sampler_trace_entry& e = rec(USE_STRACE_LANGEVIN_NORMS, i, k, (int)d, t);
                    e.score = pl.strace_score; e.noise = nz(d); e.blocks_per_b = pl.lang_blocks;
                }
                launch_langevin_step(pl.lang_partial, pl.B, per_item, pl.lang_blocks, sc.snr, pl.lang_step, s);
                if (tr) {
                    use_sampler_trace_entry& e = rec(USE_STRACE_LANGEVIN_STEP, i, k, -1, t);
                    e.blocks_per_b = pl.lang_blocks; e.step = pl.strace_step = (const float*)snap(pl.lang_step, (size_t)items * 4);
                }
                launch_corrector(pl.X, pl.score, nz(d), rng, pl.lang_step, 0.f, pl.X, nullptr, items, n_per_item, s);
                if (tr) {
                    use_sampler_trace_entry& e = rec(USE_STRACE_CORRECTOR, i, k, (int)d, t);
                    e.x_in = pl.strace_x; e.score = pl.strace_score; e.step = pl.strace_step; e.noise = nz(d);
                    e.x_out = pl.strace_x = (const float2*)snap(pl.X, (size_t)n * 8);
                }
            } else {                                               // ALD: correctors.py:79-98
                const float sd = sc.snr * ouve_std(h->cfg, t);
                launch_corrector(pl.X, pl.score, nz(d), rng, nullptr, sd * sd * 2.f, pl.X, nullptr, items, n_per_item, s);
                if (tr) {
                    use_sampler_trace_entry& e = rec(USE_STRACE_CORRECTOR, i, k, (int)d, t);
                    e.x_in = pl.strace_x; e.score = pl.strace_score; e.step_host = sd * sd * 2.f; e.noise = nz(d);
                    e.x_out = pl.strace_x = (const float2*)snap(pl.X, (size_t)n * 8);
                }
            }
            d++;
        }
        if (sc.predictor == USE_PRED_NONE) {
            if (i == sc.N - 1) {
                (void)hipMemcpyAsync(pl.Xmean, pl.X, (size_t)n * 8, hipMemcpyDeviceToDevice, s);
                if (tr) {
                    use_sampler_trace_entry& e = rec(USE_STRACE_COPY_MEAN, i, -1, -1, t);
                    e.x_in = pl.strace_x; e.x_mean = snap(pl.Xmean, (size_t)n * 8);
                }
            }
        } else {
            run_score(h, pl.X, pl.Cond, temb, 0, pl.ts_dev + i, 0, pl.score, s, -1.f, h->pcp == 8 ? pl.cond2_buf : nullptr);
            if (tr) {
                use_sampler_trace_entry& e = rec(USE_STRACE_SCORE, i, -1, -1, t);
                e.x_in = pl.strace_x; e.score = pl.strace_score = (const float2*)snap(pl.score, (size_t)n * 8);
            }
            float cd, cs, cn; predictor_coeffs(h->cfg, sc.predictor, t, sc.N, cd, cs, cn);
            launch_predictor(pl.X, pl.Y, pl.score, nz(d), SdeRng{pl.seeds, d}, cd, cs, cn, pl.X,
                             i == sc.N - 1 ? pl.Xmean : nullptr, items, n_per_item, s);
            if (tr) {
                use_sampler_trace_entry& e = rec(USE_STRACE_PREDICTOR, i, -1, (int)d, t);
                e.x_in = pl.strace_x; e.score = pl.strace_score; e.noise = nz(d); e.c_drift = cd; e.c_score = cs; e.c_noise = cn;
                e.x_out = pl.strace_x = (const float2*)snap(pl.X, (size_t)n * 8);
                if (i == sc.N - 1) e.x_mean = snap(pl.Xmean, (size_t)n * 8);
            }
            d++;
        }
    }
}

// bytes of the snapshots run_sampler takes with the step trace on (its snap() calls, each rounded up to 256 bytes)
static size_t strace_need(const use_handle* h, const Plan& pl) {
    const use_sampler_config& sc = pl.sc;
    const size_t n = (size_t)pl.B * h->cfg.n_freq * pl.T, field = (n * 8 + 255) / 256 * 256;
    const size_t ncorr = sc.corrector == USE_CORR_NONE ? 0 : (size_t)sc.corrector_steps;
    const size_t evals = (size_t)sc.N * (ncorr + (sc.predictor == USE_PRED_NONE ? 0 : 1));
    const size_t steps = sc.corrector == USE_CORR_LANGEVIN ? (size_t)sc.N * ncorr : 0;
    return (1 + evals + evals + 1) * field + steps * (((size_t)pl.B * 4 + 255) / 256 * 256);    // X, score, Xmean; Langevin steps
}

static void drop_graphs(use_handle* h) {                  // every graph that replays against the current plan
    if (h->plan) h->plan->drop_graphs();
    if (h->ode_graph) { (void)hipGraphExecDestroy(h->ode_graph); h->ode_graph = nullptr; }
}

static long long g_opt_gen = 0;                  // bumped by every use_set_option: plans built under other options are not reused
static int g_plan_cache = 4;                     // plans kept besides the current one

// new contents in the weight blob: what the current plan derived from the old ones goes (time-embedding tables, graphs), and every parked plan
static void weights_changed(use_handle* h) {
    h->weights_ready = true;
    if (h->plan) h->plan->sampler_set = false;
    drop_graphs(h);
    h->parked.clear();
}

static int ensure_sde_scratch(use_handle* h) {
    if (!h) return fail(USE_E_INVALID, "null handle");
    HIPCHK(hipSetDevice(h->device));
    if (!h->sde_buf) {
        const size_t part = (size_t)use_handle::SDE_MAX_B * use_handle::SDE_BLOCKS * 2 * 4;
        const size_t seeds = (size_t)use_handle::SDE_MAX_B * 8;                    // [0] alone but for use_fill_noise_items
        const size_t bytes = seeds + 256 + part;
        HIPCHK(hipMalloc((void**)&h->sde_buf, bytes));
        HIPCHK(hipMemset(h->sde_buf, 0, bytes));
        h->sde_seeds = (unsigned long long*)h->sde_buf; h->sde_step = (float*)(h->sde_buf + seeds);
        h->sde_partial = (float*)(h->sde_buf + seeds + 256);
    }
    return USE_OK;
}

static int ensure_cap_stream(use_handle* h) {
    if (!h->cap_stream) HIPCHK(hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking));
    return USE_OK;
}

// ---------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------
extern "C" {

int use_get_stat(use_handle* h, const char* name, long long* value) {
    if (!h || !name || !value) return fail(USE_E_INVALID, "null argument");
    if (!strcmp(name, "graph_captures")) { *value = h->n_graph_captures; return USE_OK; }      // sampling-loop segments captured so far
    if (!strcmp(name, "plans_built")) { *value = h->n_plans_built; return USE_OK; }
    if (!strcmp(name, "plan_cache_hits")) { *value = h->n_plan_cache_hits; return USE_OK; }
    if (!strcmp(name, "plans_parked")) { *value = (long long)h->parked.size(); return USE_OK; }
    if (!strcmp(name, "ode_steps")) { *value = h->ode_steps; return USE_OK; }                    // of the last use_sample_ode
    if (!strcmp(name, "ode_rejected")) { *value = h->ode_rejected; return USE_OK; }
    if (!strcmp(name, "ode_nfev_max")) { *value = h->ode_nfev_max; return USE_OK; }
    if (!strcmp(name, "plan_stale")) { *value = h->plan && h->plan->opt_gen != g_opt_gen ? 1 : 0; return USE_OK; }   // an option changed since use_plan
    return fail(USE_E_INVALID, "unknown statistic '%s'", name);
}

int use_set_option(const char* name, long long value) {
    if (!name) return fail(USE_E_INVALID, "option name is null");
    if (!strcmp(name, "trace")) { g_trace = value != 0; return USE_OK; }   // records launches, changes none: no plan goes stale
    if (!strcmp(name, "sampler_trace")) { g_sampler_trace = value != 0; return USE_OK; }   // the same for the PC loop's launches (use_sampler_trace_entry)
    ++g_opt_gen;                                               // plans built under the previous options are not reused
    if (!strcmp(name, "attn_fused")) { g_attn_fused = (int)value; return USE_OK; }
    if (!strcmp(name, "plan_cache")) { g_plan_cache = (int)std::max(0LL, std::min(16LL, value)); return USE_OK; }   // parked plans per handle
    if (!strcmp(name, "subbatch_min_items")) { g_subbatch_min_items = (int)std::max(1LL, value); return USE_OK; }
    if (!strcmp(name, "subbatch")) { g_subbatch = (int)value; return USE_OK; }          // takes effect at the next use_plan
    if (!strcmp(name, "stagger_level")) { g_stagger_level = (int)value; return USE_OK; }
    if (!strcmp(name, "stats_part")) { g_stats_part = (int)value; return USE_OK; }                  // takes effect at the next use_plan
    if (!strcmp(name, "gn_inline")) { g_gn_inline = (long)value; return USE_OK; }                  // takes effect at the next use_plan
    if (!strcmp(name, "conv_v4_min_blocks")) { conv_v4_set_min_blocks((long)value); return USE_OK; }
    if (!strcmp(name, "conv_v5")) { conv_v5_set((int)value); return USE_OK; }
    if (!strcmp(name, "fir_strip")) { fir_set_strip((int)value); return USE_OK; }
    if (!strcmp(name, "pyr_ws")) { pyr_conv_set_ws((int)value); return USE_OK; }
    if (!strcmp(name, "wgrad_mfma16")) { wgrad_set_mfma16((int)value); return USE_OK; }
    if (!strcmp(name, "wgrad_blocks")) { wgrad_set_blocks((int)value); return USE_OK; }
    if (!strcmp(name, "conv_in_wgs")) { if (value < 1 || value > 4096) return fail(USE_E_INVALID, "conv_in_wgs: 1 ... 4096"); g_conv_in_wgs = (int)value; return USE_OK; }
    if (!strcmp(name, "conv_sk_max_px")) { conv_sk_set_max_px((long)value); return USE_OK; }             // 0: conv_sk off
    return fail(USE_E_INVALID, "unknown option '%s'", name);
}
const char* use_last_error(void) { return g_err.c_str(); }
const char* use_version(void) { return "use_hip 0.1 (gfx950)"; }

int use_create(const use_config* cfg, int device, use_handle** out) {
    if (!cfg || !out) return fail(USE_E_INVALID, "null argument");
    if (cfg->n_levels < 1 || cfg->n_levels > 8 || cfg->nf % 32 != 0 || cfg->nf < 32 || cfg->num_res_blocks < 1)
        return fail(USE_E_INVALID, "unsupported architecture (nf must be a multiple of 32, 1..8 levels)");
    for (int i = 0; i < cfg->n_levels; ++i)
        if (cfg->ch_mult[i] < 1 || cfg->nf * cfg->ch_mult[i] > 512) return fail(USE_E_INVALID, "unsupported architecture (1 <= nf * ch_mult <= 512)");
    if (cfg->n_freq % (1 << (cfg->n_levels - 1)) != 0)
        return fail(USE_E_INVALID, "n_freq=%d is not divisible by 2^(levels-1)", cfg->n_freq);
    if (cfg->precision != USE_PREC_FP32 && cfg->precision != USE_PREC_BF16 && cfg->precision != USE_PREC_FP16) return fail(USE_E_INVALID, "bad precision");
    if (cfg->input_channels != 0 && cfg->input_channels != 2 && cfg->input_channels != 4 && cfg->input_channels != 6)
        return fail(USE_E_INVALID, "input_channels must be 4 (x and y), 6 (x, y and a second conditioning) or 2 (y alone), got %d", cfg->input_channels);
    use_handle* h = new use_handle();
    h->cfg = *cfg; h->device = device;
    h->act_dtype = cfg->precision == USE_PREC_BF16 ? DT_BF16 : cfg->precision == USE_PREC_FP16 ? DT_F16 : DT_F32;
    int rc = build_arch(h);
    if (rc) { delete h; return rc; }
    *out = h;
    return USE_OK;
}

int use_destroy(use_handle* h) {
    if (!h) return USE_OK;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    drop_graphs(h);                                           // (the plans themselves go with the handle: delete h)
    if (h->ode_run) (void)use_ode_destroy(h->ode_run);
    if (h->cap_stream) (void)hipStreamDestroy(h->cap_stream);
    for (int i = 0; i < MAX_SUB; ++i) {
        if (h->aux_stream[i]) (void)hipStreamDestroy(h->aux_stream[i]);
        if (h->ev_stagger[i]) { (void)hipEventDestroy(h->ev_stagger[i]); (void)hipEventDestroy(h->ev_join[i]); }
    }
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->blob) (void)hipFree(h->blob);
    if (h->sde_buf) (void)hipFree(h->sde_buf);
    delete h;
    return USE_OK;
}

int use_num_expected_weights(use_handle* h) { return h ? (int)h->expected.size() : USE_E_INVALID; }
int use_expected_weight(use_handle* h, int index, const char** name, int64_t* shape4, int* ndim) {
    if (!h || index < 0 || index >= (int)h->expected.size()) return fail(USE_E_INVALID, "bad index");
    const Expected& e = h->expected[index];
    if (name) *name = e.name.c_str();
    if (ndim) *ndim = (int)e.shape.size();
    if (shape4) for (size_t i = 0; i < 4; ++i) shape4[i] = i < e.shape.size() ? e.shape[i] : 1;
    return USE_OK;
}

int use_set_weight(use_handle* h, const char* name, const float* data, const int64_t* shape, int ndim) {
    if (!h || !name || !data || !shape) return fail(USE_E_INVALID, "null argument");
    auto it = h->expected_index.find(name);
    if (it == h->expected_index.end()) return fail(USE_E_INVALID, "unexpected weight name '%s'", name);
    const Expected& e = h->expected[it->second];
    if ((int)e.shape.size() != ndim) return fail(USE_E_INVALID, "weight '%s': rank %d, expected %zu", name, ndim, e.shape.size());
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        if (shape[i] != e.shape[i]) return fail(USE_E_INVALID, "weight '%s': dim %d is %lld, expected %lld", name, i, (long long)shape[i], (long long)e.shape[i]);
        n *= (size_t)shape[i];
    }
    h->host_w[name].assign(data, data + n);
    h->weights_ready = false;
    return USE_OK;
}

int use_alloc_weight_blob(use_handle* h) {
    if (!h) return fail(USE_E_INVALID, "null handle");
    HIPCHK(hipSetDevice(h->device));
    if (!h->blob) HIPCHK(hipMalloc((void**)&h->blob, h->blob_bytes));
    weights_changed(h);        // contents to be filled by the caller's broadcast
    return USE_OK;
}

int use_commit_weights(use_handle* h) {
    if (!h) return fail(USE_E_INVALID, "null handle");
    HIPCHK(hipSetDevice(h->device));
    std::vector<char> host(h->blob_bytes, 0);
    int rc = pack_all(h, host.data());
    if (rc) return rc;
    if (!h->blob) HIPCHK(hipMalloc((void**)&h->blob, h->blob_bytes));
    HIPCHK(hipMemcpy(h->blob, host.data(), h->blob_bytes, hipMemcpyHostToDevice));
    h->host_w.clear();
    weights_changed(h);
    return USE_OK;
}

// ---- packed weight file: header + the device blob, so that a deployment starts without a state dict ------
// The blob layout is private to a library build: BLOB_LAYOUT is bumped whenever pack_all / the blob offsets change.
namespace {
constexpr uint32_t BLOB_LAYOUT = 7;          // 7: the 16-channel-chunk copies of round 4 (conv_v10, removed) are gone again; 5: + split-bf16 copy of the input convolution (16-bit modes); 4: piece-swizzled slab copies
struct BlobHeader {
    char magic[8];                           // "USEHIPWB"
    uint32_t header_bytes, layout;
    int32_t nf, n_levels, ch_mult[8], num_res_blocks, precision, input_channels, unconditional, no_sigma_scale;
    uint32_t crc32, reserved;
    uint64_t blob_bytes;
};
uint32_t crc32_of(const unsigned char* p, size_t n) {
    static uint32_t table[256]; static bool init = false;
    if (!init) {
        for (uint32_t i = 0; i < 256; ++i) { uint32_t c = i; for (int k = 0; k < 8; ++k) c = c & 1 ? 0xEDB88320u ^ (c >> 1) : c >> 1; table[i] = c; }
        init = true;
    }
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 0xFF] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}
BlobHeader make_header(const use_handle* h) {
    BlobHeader hd{};
    memcpy(hd.magic, "USEHIPWB", 8);
    hd.header_bytes = sizeof(BlobHeader); hd.layout = BLOB_LAYOUT;
    const use_config& c = h->cfg;
    hd.nf = c.nf; hd.n_levels = c.n_levels; for (int i = 0; i < 8; ++i) hd.ch_mult[i] = i < c.n_levels ? c.ch_mult[i] : 0;
    hd.num_res_blocks = c.num_res_blocks; hd.precision = c.precision;
    hd.input_channels = c.input_channels ? c.input_channels : 4; hd.unconditional = c.unconditional != 0; hd.no_sigma_scale = c.no_sigma_scale != 0;
    hd.blob_bytes = h->blob_bytes;
    return hd;
}
}  // namespace

int use_save_weight_blob(use_handle* h, const char* path) {
    if (!h || !path) return fail(USE_E_INVALID, "null argument");
    std::vector<char> host(h->blob_bytes, 0);
    if (!h->host_w.empty()) {                                 // weights set but not committed: pack on the host, no GPU needed
        int rc = pack_all(h, host.data());
        if (rc) return rc;
    } else if (h->blob && h->weights_ready) {
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipMemcpy(host.data(), h->blob, h->blob_bytes, hipMemcpyDeviceToHost));
    } else {
        return fail(USE_E_STATE, "no weights to save (use_set_weight every tensor, or commit / load first)");
    }
    BlobHeader hd = make_header(h);
    hd.crc32 = crc32_of((const unsigned char*)host.data(), host.size());
    FILE* f = fopen(path, "wb");
    if (!f) return fail(USE_E_INVALID, "cannot open '%s' for writing", path);
    const bool ok = fwrite(&hd, sizeof hd, 1, f) == 1 && fwrite(host.data(), 1, host.size(), f) == host.size();
    if (fclose(f) != 0 || !ok) return fail(USE_E_INVALID, "short write to '%s'", path);
    return USE_OK;
}

int use_load_weight_blob(use_handle* h, const char* path) {
    if (!h || !path) return fail(USE_E_INVALID, "null argument");
    FILE* f = fopen(path, "rb");
    if (!f) return fail(USE_E_INVALID, "cannot open '%s'", path);
    BlobHeader hd{}, want = make_header(h);
    std::vector<char> host(h->blob_bytes);
    if (fread(&hd, sizeof hd, 1, f) != 1) { fclose(f); return fail(USE_E_INVALID, "'%s' is truncated", path); }
    if (memcmp(hd.magic, want.magic, 8) != 0 || hd.header_bytes != sizeof hd) { fclose(f); return fail(USE_E_INVALID, "'%s' is not a use_hip weight file", path); }
    if (hd.layout != want.layout) { fclose(f); return fail(USE_E_INVALID, "'%s' has blob layout %u, this build reads %u: re-pack the checkpoint", path, hd.layout, want.layout); }
    {
        BlobHeader a = hd; a.crc32 = 0;                       // everything but the checksum describes the network
        if (memcmp(&a, &want, sizeof a) != 0) { fclose(f); return fail(USE_E_INVALID, "'%s' was packed for a different network configuration / precision", path); }
    }
    const bool ok = fread(host.data(), 1, host.size(), f) == host.size();
    fclose(f);
    if (!ok) return fail(USE_E_INVALID, "'%s' is truncated", path);
    if (crc32_of((const unsigned char*)host.data(), host.size()) != hd.crc32) return fail(USE_E_INVALID, "'%s': checksum mismatch", path);
    HIPCHK(hipSetDevice(h->device));
    if (!h->blob) HIPCHK(hipMalloc((void**)&h->blob, h->blob_bytes));
    HIPCHK(hipMemcpy(h->blob, host.data(), h->blob_bytes, hipMemcpyHostToDevice));
    h->host_w.clear();
    weights_changed(h);
    return USE_OK;
}

int use_weight_blob(use_handle* h, void** dev_ptr, size_t* bytes) {
    if (!h) return fail(USE_E_INVALID, "null handle");
    if (dev_ptr) *dev_ptr = h->blob;
    if (bytes) *bytes = h->blob_bytes;
    return USE_OK;
}

int use_plan(use_handle* h, int B, int Tpad) {
    if (!h) return fail(USE_E_INVALID, "null handle");
    if (B < 1 || Tpad < 64 || Tpad % 64 != 0) return fail(USE_E_INVALID, "plan needs B >= 1 and T' a positive multiple of 64 (got B=%d T'=%d)", B, Tpad);
    if ((Tpad >> (h->cfg.n_levels - 1)) < 1) return fail(USE_E_INVALID, "T' too small for %d levels", h->cfg.n_levels);
    HIPCHK(hipSetDevice(h->device));
    auto wanted = [&](const Plan& p) { return p.B == B && p.T == Tpad && p.opt_gen == g_opt_gen; };
    if (h->plan && wanted(*h->plan)) return USE_OK;           // the current plan
    HIPCHK(hipDeviceSynchronize());
    if (h->ode_graph) { (void)hipGraphExecDestroy(h->ode_graph); h->ode_graph = nullptr; }   // it holds the current plan's workspace
    // the requested plan, if it is parked: taken out BEFORE the current one goes in (else a cycle over capacity + 1 shapes would evict what it needs)
    std::unique_ptr<Plan> hit;
    for (auto it = h->parked.begin(); it != h->parked.end(); ++it)
        if (wanted(**it)) { hit = std::move(*it); h->parked.erase(it); break; }
    // park the current plan (with its graphs), unless it is stale or nothing is kept; the least recently used ones go beyond the capacity
    if (h->plan && g_plan_cache > 0 && h->plan->opt_gen == g_opt_gen) h->parked.push_back(std::move(h->plan));
    h->plan.reset();
    while ((int)h->parked.size() > g_plan_cache) h->parked.erase(h->parked.begin());
    if (hit) {
        h->plan = std::move(hit);
        ++h->n_plan_cache_hits;
        return USE_OK;
    }
    // A new plan, built in a local owner and installed last: whatever fails on the way, the handle is left without a current plan
    ++h->n_plans_built;
    auto built = std::make_unique<Plan>();
    Plan& pl = *built;
    pl.opt_gen = g_opt_gen;
    pl.B = B; pl.T = Tpad;
    // sub-batch pipelining (run_score): `subbatch` sub-batches of at least 2 items each
    // How many sub-batches: a question of grid quantisation on the 256 CUs (same-box sweeps, profiles/r5_e2e_ab_subbatch_sweep.txt).  The 3x3
    // convolutions of the 256 x 320 / 128 x 160 maps launch 160 / 80 workgroups per item: sub-batches of 4 items leave 2.5 / 1.25 rounds (83 % /
    // 62 % of the last round's CUs busy), of 3 items 1.9 / 0.94 - batch 8 runs 1.6 % faster as 3 + 3 + 2 than as 4 + 4 (bf16 and fp16), five or
    // more streams 12-17 % slower; batch 16 is fastest as 8 + 8 (5 / 2.5 rounds; 6 + 5 + 5: +0.7 %).
    const int want = g_subbatch >= 0 ? g_subbatch : (B >= 6 && B <= 11) ? 3 : 2;
    pl.nsub = std::max(1, std::min(std::min(want, MAX_SUB), B / std::max(1, g_subbatch_min_items)));
    for (int i = 0; i < MAX_SUB; ++i) pl.sub_B[i] = i < pl.nsub ? B / pl.nsub + (i < B % pl.nsub ? 1 : 0) : 0;
    // dry runs to size the activation arenas (one per sub-batch, carved from one allocation)
    pl.dry = true;
    size_t caps[MAX_SUB] = {}, stcaps[MAX_SUB] = {}, total = 0;
    for (int i = 0; i < pl.nsub; ++i) {
        Arena& ar = i ? pl.sub_arena[i] : pl.arena;
        Fwd f{h, pl, nullptr, nullptr, 0, nullptr, 0};
        f.B = pl.sub_B[i]; f.arena = &ar; f.st_arena = &pl.st_arena[i]; f.primary = i == 0;
        f.run(nullptr);
        caps[i] = (ar.peak + 4096 + 255) & ~(size_t)255; total += caps[i];
        stcaps[i] = (pl.st_arena[i].peak + 255) & ~(size_t)255; total += stcaps[i];
    }
    pl.dry = false;
    auto device_alloc = [&](char** d, size_t bytes) {         // parked plans hold their workspaces: give them up and try once more
        if (hipMalloc((void**)d, bytes) == hipSuccess) return true;
        (void)hipGetLastError();
        h->parked.clear();
        return hipMalloc((void**)d, bytes) == hipSuccess;
    };
    char* base = nullptr;
    if (!device_alloc(&base, total)) return fail(USE_E_NOMEM, "cannot allocate %.1f MB of activation workspace", total / 1e6);
    pl.arena.base = base; pl.arena.cap = caps[0];             // owns the allocation (arena_plan_bytes); its own slice is caps[0]
    pl.arena_plan_bytes = total;
    {
        size_t off = caps[0];
        for (int i = 1; i < pl.nsub; ++i) { pl.sub_arena[i].base = base + off; pl.sub_arena[i].cap = caps[i]; off += caps[i]; }
        for (int i = 0; i < pl.nsub; ++i) { pl.st_arena[i].base = base + off; pl.st_arena[i].cap = stcaps[i]; off += stcaps[i]; }
        pl.arena.dry_on_overflow = &pl.dry;
        for (int i = 0; i < pl.nsub; ++i) { pl.sub_arena[i].dry_on_overflow = &pl.dry; pl.st_arena[i].dry_on_overflow = &pl.dry; }
    }
    if (pl.nsub > 1 && !h->ev_fork) HIPCHK(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    for (int i = 0; i < pl.nsub; ++i) {
        if (i && !h->aux_stream[i]) HIPCHK(hipStreamCreateWithFlags(&h->aux_stream[i], hipStreamNonBlocking));
        if (pl.nsub > 1 && !h->ev_stagger[i]) {
            HIPCHK(hipEventCreateWithFlags(&h->ev_stagger[i], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&h->ev_join[i], hipEventDisableTiming));
        }
    }
    // persistent buffers
    const size_t n = (size_t)B * h->cfg.n_freq * Tpad;
    pl.lang_blocks = (int)std::min<size_t>(256, ((size_t)h->cfg.n_freq * Tpad + 255) / 256);
    size_t off = 0;
    auto take = [&](size_t bytes) { off = (off + 255) & ~(size_t)255; size_t o = off; off += bytes; return o; };
    const size_t o_x4 = take(n * 4 * h->pcp), o_c2 = take(h->pcp == 8 ? n * 8 : 0), o_Y = take(n * 8), o_X = take(n * 8), o_Xm = take(n * 8), o_sc = take(n * 8),
                 o_xin = take(n * 8), o_cond = take(n * 8), o_st = take((size_t)B * 4 * h->cfg.nf * 4), o_tb = take((size_t)B * h->dense_rows * 4),
                 o_t = take((size_t)B * 4), o_lp = take((size_t)B * pl.lang_blocks * 2 * 4), o_ls = take((size_t)B * 4),
                 o_sd = take((size_t)std::max(B, 1) * 8);
    pl.persist_bytes = off;
    if (!device_alloc(&pl.persist, off)) return fail(USE_E_NOMEM, "cannot allocate %.1f MB of state", off / 1e6);
    pl.x4 = (float*)(pl.persist + o_x4); pl.Y = (float2*)(pl.persist + o_Y); pl.X = (float2*)(pl.persist + o_X);
    pl.Xmean = (float2*)(pl.persist + o_Xm); pl.score = (float2*)(pl.persist + o_sc); pl.xin = (float2*)(pl.persist + o_xin);
    pl.cond_buf = (float2*)(pl.persist + o_cond); pl.Cond = pl.Y;
    pl.cond2_buf = h->pcp == 8 ? (float2*)(pl.persist + o_c2) : nullptr;
    pl.silu_temb = (float*)(pl.persist + o_st); pl.tembias = (float*)(pl.persist + o_tb); pl.t_dev = (float*)(pl.persist + o_t);
    pl.lang_partial = (float*)(pl.persist + o_lp); pl.lang_step = (float*)(pl.persist + o_ls);
    pl.seeds = (unsigned long long*)(pl.persist + o_sd);
    HIPCHK(hipMemset(pl.persist, 0, off));
    h->plan = std::move(built);
    return USE_OK;
}

int use_workspace_bytes(use_handle* h, size_t* bytes) {
    if (!h || !bytes) return fail(USE_E_INVALID, "null argument");
    *bytes = (h->plan ? h->plan->arena_plan_bytes + h->plan->persist_bytes : 0) + h->blob_bytes;
    return USE_OK;
}

double use_flops_per_score(use_handle* h) { return h && h->plan ? h->plan->flops : 0.0; }

static int check_ready(use_handle* h) {
    if (!h) return fail(USE_E_INVALID, "null handle");
    if (!h->weights_ready) return fail(USE_E_STATE, "weights not committed (use_commit_weights / use_alloc_weight_blob)");
    if (!h->plan) return fail(USE_E_STATE, "use_plan has not been called");
    // Options are read at plan time (buffer sizes: conv_in_wgs, stats_part, gn_inline, subbatch*; kernel choice: every threshold): a plan
    // built under other options is stale.  An error, not a silent re-plan: a re-plan frees the captured graphs and the sampler tables
    // behind the caller's back (and round 5's answer - overflowing the arena and abort() - was no answer at all).
    if (h->plan->opt_gen != g_opt_gen)
        return fail(USE_E_STATE, "use_set_option was called after use_plan: the plan is stale, call use_plan (and use_set_sampler) again");
    return USE_OK;
}

// after an evaluation was issued: did every tensor fit its arena?  (defence in depth behind check_ready's stale-plan test)
static int eval_status(use_handle* h) {
    Plan& pl = *h->plan;
    bool bad = pl.arena.overflow;
    for (int i = 0; i < MAX_SUB; ++i) bad = bad || pl.sub_arena[i].overflow || pl.st_arena[i].overflow;
    if (!bad) return USE_OK;
    pl.arena.overflow = false; pl.dry = false;
    for (int i = 0; i < MAX_SUB; ++i) pl.sub_arena[i].overflow = pl.st_arena[i].overflow = false;
    return fail(USE_E_STATE, "activation workspace too small for this evaluation (an option that sizes plan buffers changed after use_plan?): call use_plan again; the output is invalid");
}

// one network evaluation; sign -1: the score (use_score), +1: the raw backbone output (use_forward)
static int eval_net(use_handle* h, const void* x, const void* y, const float* t, void* out, use_stream_t stream, float sign,
                    const void* y2 = nullptr) {
    int rc = check_ready(h); if (rc) return rc;
    Plan& pl = *h->plan;
    const use_config& c = h->cfg;
    const bool two_ch = c.input_channels == 2;
    if (!x || !out) return fail(USE_E_INVALID, "null tensor");
    if ((c.input_channels == 6) != (y2 != nullptr))
        return fail(USE_E_INVALID, c.input_channels == 6 ? "a 6-channel network takes two conditioning tensors (use_score2)" : "this network takes one conditioning tensor");
    if (two_ch ? y != nullptr : y == nullptr) return fail(USE_E_INVALID, two_ch ? "a 2-channel network takes x alone (y must be null)" : "null tensor");
    if (!t && (!c.unconditional || !c.no_sigma_scale)) return fail(USE_E_INVALID, "this network needs the time t");
    hipStream_t s = (hipStream_t)stream;
    if (!c.unconditional) run_temb(h, t, pl.B, pl.silu_temb, pl.tembias, s);
    run_score(h, (const float2*)x, (const float2*)y, c.unconditional ? nullptr : pl.tembias, h->dense_rows, t, 1, (float2*)out, s, sign,
              (const float2*)y2);
    HIPCHK(hipGetLastError());
    return eval_status(h);
}
int use_score2(use_handle* h, const void* x, const void* y, const void* y2, const float* t, void* out, use_stream_t stream) {
    return eval_net(h, x, y, t, out, stream, -1.f, y2);
}
int use_score(use_handle* h, const void* x, const void* y, const float* t, void* out, use_stream_t stream) {
    return eval_net(h, x, y, t, out, stream, -1.f);
}
int use_forward(use_handle* h, const void* x, const void* y, const float* t, void* out, use_stream_t stream) {
    return eval_net(h, x, y, t, out, stream, +1.f);
}
int use_forward_items(use_handle* h, const void* x, const void* y, const float* t, void* out, use_stream_t stream) {
    // the kernel choice of the per-item sampler loop (run_sampler): conv_sk picks its tile form from the per-image workgroup count
    struct PerImage { PerImage() { conv_sk_set_per_image(true); } ~PerImage() { conv_sk_set_per_image(false); } } per_image;
    return eval_net(h, x, y, t, out, stream, +1.f);
}

int use_profile_score(use_handle* h, const void* x, const void* y, const float* t, void* out, use_stream_t stream,
                      double* conv_ms, double* conv_flops, double* conv_bytes, int* conv_launches, double* total_ms) {
    int rc = check_ready(h); if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t t0, t1; HIPCHK(hipEventCreate(&t0)); HIPCHK(hipEventCreate(&t1));
    h->profile = true;
    for (auto& r : h->prof) { if (r.e0) (void)hipEventDestroy(r.e0); if (r.e1) (void)hipEventDestroy(r.e1); }
    h->prof.clear();
    const bool verbose = getenv("USE_HIP_PROFILE_VERBOSE") != nullptr;
    h->profile_all = verbose;                                 // verbose: also list the conv_v2_kernel launches
    HIPCHK(hipEventRecord(t0, s));
    rc = use_score(h, x, y, t, out, stream);
    h->profile = false; h->profile_all = false;
    if (rc) return rc;
    HIPCHK(hipEventRecord(t1, s));
    HIPCHK(hipStreamSynchronize(s));
    double ms = 0.0, fl = 0.0, by = 0.0; int nmain = 0;
    for (auto& r : h->prof) {
        float e = 0.f; HIPCHK(hipEventElapsedTime(&e, r.e0, r.e1));
        r.ms = e; (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); r.e0 = r.e1 = nullptr;
        if (r.main) { ms += e; fl += r.flops; by += r.bytes; ++nmain; }
        if (verbose && !r.desc.empty()) fprintf(stderr, "[use_profile] %s  %8.3f ms  %7.1f TFLOP/s\n", r.desc.c_str(), e, r.flops / e / 1e9);
    }
    // what use_profile_aux reports: the records outside the verbose listing in launch order, then the dominant kernel's own launches
    // ("conv_v4"), so that callers can break it down by map (bench.py: roofline.by_map)
    h->prof.erase(std::remove_if(h->prof.begin(), h->prof.end(), [](const use_handle::ProfRec& r) { return !r.main && !r.desc.empty(); }), h->prof.end());
    std::stable_partition(h->prof.begin(), h->prof.end(), [](const use_handle::ProfRec& r) { return !r.main; });
    float tot = 0.f; HIPCHK(hipEventElapsedTime(&tot, t0, t1));
    (void)hipEventDestroy(t0); (void)hipEventDestroy(t1);
    if (conv_ms) *conv_ms = ms;
    if (conv_flops) *conv_flops = fl;
    if (conv_bytes) *conv_bytes = by;
    if (conv_launches) *conv_launches = nmain;
    if (total_ms) *total_ms = tot;
    return USE_OK;
}

int use_profile_aux(use_handle* h, int index, char* name, int name_cap, int* H, int* W, double* bytes, double* ms) {
    if (!h) return fail(USE_E_INVALID, "null handle");
    if (index < 0 || index >= (int)h->prof.size()) return 1;              // past the end (not an error: the caller iterates)
    const auto& a = h->prof[(size_t)index];
    if (name && name_cap > 0) { strncpy(name, a.label.c_str(), (size_t)name_cap - 1); name[name_cap - 1] = 0; }
    if (H) *H = a.H; if (W) *W = a.W; if (bytes) *bytes = a.bytes; if (ms) *ms = a.ms;
    return USE_OK;
}

int use_profile_aux_flops(use_handle* h, int index, double* flops) {
    if (!h) return fail(USE_E_INVALID, "null handle");
    if (index < 0 || index >= (int)h->prof.size()) return 1;
    if (flops) *flops = h->prof[(size_t)index].flops;
    return USE_OK;
}

int use_timesteps(int N, float t_eps, float* out) {
    if (N < 1 || !out) return fail(USE_E_INVALID, "bad arguments");
    std::vector<float> ts; linspace_f32(1.0f, t_eps, N, ts);
    memcpy(out, ts.data(), (size_t)N * 4);
    return USE_OK;
}

int use_set_sampler(use_handle* h, const use_sampler_config* sc) {
    int rc = check_ready(h); if (rc) return rc;
    Plan& pl = *h->plan;
    if (!sc || sc->N < 1) return fail(USE_E_INVALID, "sampler needs N >= 1");
    if (h->cfg.unconditional || h->cfg.input_channels == 2 || h->cfg.no_sigma_scale)
        return fail(USE_E_STATE, "the reverse-SDE sampler needs the conditional 4-channel score network");
    if (sc->predictor < 0 || sc->predictor > 2 || sc->corrector < 0 || sc->corrector > 2) return fail(USE_E_INVALID, "unknown predictor/corrector id");
    if (sc->corrector != USE_CORR_NONE && sc->corrector_steps < 0) return fail(USE_E_INVALID, "negative corrector_steps");
    HIPCHK(hipSetDevice(h->device));
    if (pl.sampler_set && !memcmp(&pl.sc, sc, sizeof *sc)) return USE_OK;       // unchanged (e.g. a parked plan taken back): tables and graphs stay
    HIPCHK(hipDeviceSynchronize());
    drop_graphs(h);
    for (auto& v : pl.strace) v.clear();                        // the step trace of the previous configuration goes with its graphs
    pl.strace_cur = -1;
    pl.sc = *sc;
    linspace_f32(1.0f, sc->t_eps, sc->N, pl.timesteps);         // sampling/__init__.py:63 (sde.T == 1)
    if (pl.temb_table) { HIPCHK(hipFree(pl.temb_table)); pl.temb_table = nullptr; }
    if (pl.silu_table) { HIPCHK(hipFree(pl.silu_table)); pl.silu_table = nullptr; }
    if (pl.ts_dev) { HIPCHK(hipFree(pl.ts_dev)); pl.ts_dev = nullptr; }
    HIPCHK(hipMalloc((void**)&pl.temb_table, (size_t)sc->N * h->dense_rows * 4));
    HIPCHK(hipMalloc((void**)&pl.silu_table, (size_t)sc->N * 4 * h->cfg.nf * 4));
    HIPCHK(hipMalloc((void**)&pl.ts_dev, (size_t)sc->N * 4));
    HIPCHK(hipMemcpy(pl.ts_dev, pl.timesteps.data(), (size_t)sc->N * 4, hipMemcpyHostToDevice));
    run_temb(h, pl.ts_dev, sc->N, pl.silu_table, pl.temb_table, nullptr);   // t is batch-uniform and known up front
    HIPCHK(hipDeviceSynchronize());
    pl.sampler_set = true;
    return USE_OK;
}

int use_num_noise_draws(use_handle* h) {
    if (!h || !h->plan || !h->plan->sampler_set) return fail(USE_E_STATE, "sampler not configured");
    const Plan& pl = *h->plan;
    const int ncorr = pl.sc.corrector == USE_CORR_NONE ? 0 : pl.sc.corrector_steps;
    return 1 + pl.sc.N * (ncorr + (pl.sc.predictor == USE_PRED_NONE ? 0 : 1));
}

int use_get_timesteps(use_handle* h, float* out, int n) {
    if (!h || !h->plan || !h->plan->sampler_set || !out) return fail(USE_E_STATE, "sampler not configured");
    const Plan& pl = *h->plan;
    for (int i = 0; i < n && i < (int)pl.timesteps.size(); ++i) out[i] = pl.timesteps[i];
    return (int)pl.timesteps.size();
}

int use_sample(use_handle* h, const void* y, const void* noise, uint64_t seed, void* out, use_stream_t stream) {
    return use_sample_cond(h, y, nullptr, noise, seed, out, stream);
}

int use_sample_cond(use_handle* h, const void* y, const void* cond, const void* noise, uint64_t seed, void* out, use_stream_t stream) {
    return use_sample_cond2(h, y, cond, nullptr, noise, seed, out, stream);
}

// the sampler's inputs into the plan's buffers: the SDE's y, and the conditioning the network sees beside x - y itself, or a
// separate one (condition="denoised"), and the second one of condition="both"
static int load_sampler_inputs(use_handle* h, const void* y, const void* cond, const void* cond2, hipStream_t s) {
    Plan& pl = *h->plan;
    const size_t n = (size_t)pl.B * h->cfg.n_freq * pl.T;
    HIPCHK(hipMemcpyAsync(pl.Y, y, n * 8, hipMemcpyDeviceToDevice, s));
    if (cond2) HIPCHK(hipMemcpyAsync(pl.cond2_buf, cond2, n * 8, hipMemcpyDeviceToDevice, s));
    float2* want = cond ? pl.cond_buf : pl.Y;
    if (want != pl.Cond) { HIPCHK(hipStreamSynchronize(s)); drop_graphs(h); pl.Cond = want; }    // captured graphs hold the pointer
    if (cond) HIPCHK(hipMemcpyAsync(pl.cond_buf, cond, n * 8, hipMemcpyDeviceToDevice, s));
    return USE_OK;
}

}  // extern "C"

// up to 32 per-item seeds per launch, passed by value: the host array is free again when the call returns, and nothing synchronises
struct SeedPack { unsigned long long v[32]; };
__global__ void set_item_seeds_kernel(unsigned long long* dst, SeedPack p, int n) { if ((int)threadIdx.x < n) dst[threadIdx.x] = p.v[threadIdx.x]; }
static void upload_item_seeds(unsigned long long* dst, const uint64_t* seeds_host, int B, hipStream_t s) {
    for (int b0 = 0; b0 < B; b0 += 32) {
        SeedPack p{};
        const int k = std::min(32, B - b0);
        for (int i = 0; i < k; ++i) p.v[i] = (unsigned long long)seeds_host[b0 + i];
        hipLaunchKernelGGL(set_item_seeds_kernel, dim3(1), dim3(32), 0, s, dst + b0, p, k);
    }
}

// what every sampler checks first; `set` is the plan's flag that the sampler at hand has been configured
static int check_sample_args(use_handle* h, bool Plan::*set, const char* unset, const void* y, const void* cond2, const void* out,
                             const char* six_hint) {
    int rc = check_ready(h); if (rc) return rc;
    if (!((*h->plan).*set)) return fail(USE_E_STATE, "%s", unset);
    if (!y || !out) return fail(USE_E_INVALID, "null tensor");
    if ((h->cfg.input_channels == 6) != (cond2 != nullptr))
        return h->cfg.input_channels == 6 ? fail(USE_E_INVALID, "a 6-channel network samples with two conditioning tensors%s", six_hint)
                                          : fail(USE_E_INVALID, "this network takes one conditioning tensor");
    return USE_OK;
}

// record(cap_stream), captured into an executable graph; what: "the sampling loop", for the error text.  *ge is null on failure, and what
// else has to go then is the caller's business.
template <class F>
static int capture_graph(use_handle* h, const char* what, F&& record, hipGraphExec_t* ge) {
    *ge = nullptr;
    hipGraph_t g = nullptr;
    HIPCHK(hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal));
    record(h->cap_stream);
    // (nothing returns between begin and end: a failed launch invalidates the capture and surfaces here, with the
    // stream out of capture mode either way)
    hipError_t e = hipStreamEndCapture(h->cap_stream, &g);
    if (eval_status(h)) { if (g) (void)hipGraphDestroy(g); (void)hipGetLastError(); return USE_E_STATE; }
    if (e != hipSuccess || !g) {
        if (g) (void)hipGraphDestroy(g);
        (void)hipGetLastError();
        return fail(USE_E_HIP, "capturing %s failed: %s", what, hipGetErrorString(e));
    }
    e = hipGraphInstantiate(ge, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) { *ge = nullptr; return fail(USE_E_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e)); }
    ++h->n_graph_captures;
    return USE_OK;
}

// use_sample_cond2 (seeds_host == null, per_item false) and use_sample_items (per_item)
static int sample_impl(use_handle* h, const void* y, const void* cond, const void* cond2, const void* noise, uint64_t seed,
                       const uint64_t* seeds_host, bool per_item, void* out, use_stream_t stream) {
    int rc = check_sample_args(h, &Plan::sampler_set, "use_set_sampler has not been called", y, cond2, out, " (use_sample_cond2)");
    if (rc) return rc;
    Plan& pl = *h->plan;
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)pl.B * h->cfg.n_freq * pl.T;
    // The sampler step trace.  Off: nothing is recorded, and the count reads 0.  Graphs captured under the other setting hold (or
    // lack) the snapshot copies and are dropped; the snapshot buffer is made at the first traced call of a configuration.
    const bool traced = g_sampler_trace != 0;
    pl.strace_cur = pl.strace_rec = -1;
    struct RecOff { Plan& p; ~RecOff() { p.strace_rec = -1; } } rec_off{pl};
    if (traced != pl.graphs_traced) { HIPCHK(hipDeviceSynchronize()); pl.drop_sampler_graphs(); pl.graphs_traced = traced; }
    if (traced) {
        const size_t need = strace_need(h, pl);
        if (need > ((size_t)256 << 20))
            return fail(USE_E_INVALID, "sampler_trace: the snapshots of this sampler configuration take %.1f MB, more than the 256 MB the trace allows (it is for small shapes)", need / 1048576.0);
        if (need != pl.strace_bytes) {
            HIPCHK(hipDeviceSynchronize());
            pl.drop_sampler_graphs();                                      // they hold addresses inside the old buffer
            if (pl.strace_buf) HIPCHK(hipFree(pl.strace_buf));
            pl.strace_buf = nullptr; pl.strace_bytes = 0;
            if (hipMalloc((void**)&pl.strace_buf, need) != hipSuccess) return fail(USE_E_NOMEM, "cannot allocate %.1f MB of sampler trace snapshots", need / 1e6);
            pl.strace_bytes = need;
        }
        HIPCHK(hipMemsetAsync(pl.strace_buf, 0xFF, pl.strace_bytes, s));   // NaN: a snapshot that is not taken cannot pass for one of an earlier call
    }
    rc = load_sampler_inputs(h, y, cond, cond2, s); if (rc) return rc;
    // both forms keep their seeds in pl.seeds, and so do both forms' graphs: each call uploads its own (per item without seeds: all its noise
    // is injected, and its kernels read none)
    if (per_item) { if (seeds_host) upload_item_seeds(pl.seeds, seeds_host, pl.B, s); }
    else hipLaunchKernelGGL(set_rng_kernel, dim3(1), dim3(1), 0, s, pl.seeds, (unsigned long long)seed);
    if (!pl.sc.use_graph) {
        if (traced) pl.strace_rec = 4;
        run_sampler(h, (const float2*)noise, s, 0, pl.sc.N, per_item);
        rc = eval_status(h); if (rc) return rc;
        if (traced) pl.strace_cur = 4;
    } else {
        const int gi = (noise ? 1 : 0) + (per_item ? 2 : 0);
        const float2* nz = nullptr;
        if (noise) {
            const size_t nb = (size_t)use_num_noise_draws(h) * n * 8;
            if (nb > pl.noise_copy_bytes) {
                HIPCHK(hipStreamSynchronize(s));
                if (pl.noise_copy) HIPCHK(hipFree(pl.noise_copy));
                pl.noise_copy = nullptr; pl.noise_copy_bytes = 0;
                for (int k = 1; k < 4; k += 2) {                           // both forms' injected-noise graphs hold the address
                    for (auto g : pl.graph_exec[k]) if (g) (void)hipGraphExecDestroy(g);
                    pl.graph_exec[k].clear();
                }
                if (hipMalloc((void**)&pl.noise_copy, nb) != hipSuccess) return fail(USE_E_NOMEM, "cannot allocate %.1f MB noise staging", nb / 1e6);
                pl.noise_copy_bytes = nb;
            }
            HIPCHK(hipMemcpyAsync(pl.noise_copy, noise, nb, hipMemcpyDeviceToDevice, s));
            nz = pl.noise_copy;
        }
        if (pl.graph_exec[gi].empty()) {
            // The loop is captured in segments of at most 64 score evaluations (~16 k kernel nodes each, the size the
            // configs[1] graph has): one graph of the N = 200 config's 400 evaluations (~10^5 nodes) crashes the HIP runtime
            // at instantiation.  The segments are launched back to back on the caller's stream.
            rc = ensure_cap_stream(h); if (rc) return rc;
            const int ncorr = pl.sc.corrector == USE_CORR_NONE ? 0 : pl.sc.corrector_steps;
            const int per_seg = std::max(1, 64 / (ncorr + 1));
            if (traced) pl.strace_rec = gi;                                // recorded once, at the capture: the replays refill the snapshots
            for (int i0 = 0; i0 < pl.sc.N; i0 += per_seg) {
                hipGraphExec_t ge = nullptr;
                rc = capture_graph(h, "the sampling loop",
                                   [&](hipStream_t cs) { run_sampler(h, nz, cs, i0, std::min(pl.sc.N, i0 + per_seg), per_item); }, &ge);
                if (rc) { drop_graphs(h); return rc; }
                pl.graph_exec[gi].push_back(ge);
            }
        }
        pl.strace_rec = -1;
        for (auto ge : pl.graph_exec[gi]) HIPCHK(hipGraphLaunch(ge, s));
        if (traced) pl.strace_cur = gi;
    }
    HIPCHK(hipMemcpyAsync(out, pl.Xmean, n * 8, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipGetLastError());
    return USE_OK;
}

extern "C" {

int use_sample_cond2(use_handle* h, const void* y, const void* cond, const void* cond2, const void* noise, uint64_t seed, void* out,
                     use_stream_t stream) {
    return sample_impl(h, y, cond, cond2, noise, seed, nullptr, false, out, stream);
}

int use_sample_items(use_handle* h, const void* y, const void* cond, const void* cond2, const void* noise, const uint64_t* seeds_host,
                     void* out, use_stream_t stream) {
    if (!noise && !seeds_host) return fail(USE_E_INVALID, "use_sample_items needs per-item seeds or injected noise");
    return sample_impl(h, y, cond, cond2, noise, 0, seeds_host, true, out, stream);
}

// ---- probability-flow ODE sampler (reference sampling/__init__.py:76-159): the RK45 stepper of use_ode.hip -------------------
}  // extern "C"

struct use_ode {
    use_handle* h = nullptr;
    use_ode_config cfg{};
    OdeDev d{};
    OdeCtl c{};
    char* buf = nullptr;
    float2* ysde_buf = nullptr;
    int* done_host = nullptr;                 // pinned: the "all groups done" word read back once per step
    int phase = -1;                           // the stage-time row of the next evaluation: 0 f0, 7 f1 of select_initial_step, 1..6 a step
};

namespace {
// the double a float field of use_ode_config stands for: its shortest decimal spelling (1e-5f -> 1e-5), i.e. the Python float the
// reference passes to solve_ivp
double float_as_decimal(float f) {
    char b[48];
    for (int p = 6; p <= 9; ++p) {
        snprintf(b, sizeof b, "%.*g", p, (double)f);
        if (strtof(b, nullptr) == f) break;
    }
    return strtod(b, nullptr);
}

int ode_check_config(const use_ode_config* oc) {
    if (!oc) return fail(USE_E_INVALID, "null ODE configuration");
    if (!(oc->rtol > 0.f) || !(oc->atol >= 0.f)) return fail(USE_E_INVALID, "ODE sampler needs rtol > 0 and atol >= 0 (got %g, %g)", oc->rtol, oc->atol);
    if (!(oc->t_eps > 0.f && oc->t_eps < 1.f)) return fail(USE_E_INVALID, "ODE sampler needs 0 < t_eps < T = 1 (got %g)", oc->t_eps);
    if (oc->group < 0) return fail(USE_E_INVALID, "ODE group must be >= 0 (0 = the whole batch), got %d", oc->group);
    if (oc->denoise && oc->N < 1) return fail(USE_E_INVALID, "the denoise step needs N >= 1");
    if (!(oc->first_step >= 0.f) || !(oc->max_step >= 0.f) || oc->max_nfe < 0) return fail(USE_E_INVALID, "first_step, max_step and max_nfe must be >= 0");
    if (oc->first_step > 0.f && float_as_decimal(oc->first_step) > 1.0 - float_as_decimal(oc->t_eps))
        return fail(USE_E_INVALID, "first_step exceeds the integration interval");   // validate_first_step (common.py:40-48)
    return USE_OK;
}

// one supplied evaluation: the stage kernel of the current row, then the controller where a decision is due
void ode_supply_impl(use_ode* o, const float2* f, int kind, hipStream_t s) {
    launch_ode_stage(o->d, o->phase, f, kind, s);
    switch (o->phase) {
        case 0:                                            // f0: select_initial_step's d0, d1 (or the given first_step)
            launch_ode_ctrl(o->c, o->d, ODE_INIT1, s);
            if (o->c.first_step > 0) { launch_ode_commit(o->d, 0.2, s); o->phase = 1; }
            else { launch_ode_commit(o->d, 1.0, s); o->phase = 7; }   // the probe y0 + h0 direction f0
            break;
        case 7:
            launch_ode_ctrl(o->c, o->d, ODE_INIT2, s);
            launch_ode_commit(o->d, 0.2, s);
            o->phase = 1;
            break;
        case 6:                                            // accept / reject, FSAL, the first stage input of the next attempt
            launch_ode_ctrl(o->c, o->d, ODE_STEP, s);
            launch_ode_commit(o->d, 0.2, s);
            o->phase = 1;
            break;
        default: ++o->phase;
    }
}

void ode_start_impl(use_ode* o, hipStream_t s) {           // d.xin holds the prior sample, d.ysde the SDE's y
    launch_ode_load(o->d, s);
    launch_ode_ctrl(o->c, o->d, ODE_START, s);
    o->phase = 0;
}

int ode_all_done(use_ode* o, hipStream_t s, bool* done) {
    HIPCHK(hipMemcpyAsync(o->done_host, o->d.done, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *done = *o->done_host != 0;
    return USE_OK;
}

int ode_read_groups(use_ode* o, std::vector<OdeGroup>& g, hipStream_t s) {
    g.resize((size_t)o->c.ngroups);
    HIPCHK(hipMemcpyAsync(g.data(), o->d.grp, g.size() * sizeof(OdeGroup), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return USE_OK;
}
}  // namespace

extern "C" {

int use_ode_create(use_handle* h, int B, int64_t n_per_item, const use_ode_config* cfg, use_ode** out) {
    if (!h || !out) return fail(USE_E_INVALID, "null argument");
    *out = nullptr;
    int rc = ode_check_config(cfg); if (rc) return rc;
    if (B < 1 || n_per_item < 1) return fail(USE_E_INVALID, "ODE stepper needs B >= 1 and n_per_item >= 1");
    HIPCHK(hipSetDevice(h->device));
    auto* o = new use_ode();
    o->h = h; o->cfg = *cfg;
    const int G = cfg->group == 0 || cfg->group > B ? B : cfg->group;
    const int ng = (B + G - 1) / G;
    const long n = (long)B * n_per_item;
    const int nblk = (int)std::max(1L, std::min(128L, (long)((n_per_item + 2047) / 2048)));
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o0 = off; off = (off + bytes + 255) & ~(size_t)255; return o0; };
    const size_t o_y = take((size_t)n * 16), o_yn = take((size_t)n * 16), o_K = take((size_t)n * 8 * 7), o_x = take((size_t)n * 8),
                 o_ys = take((size_t)n * 8), o_h = take((size_t)B * 8), o_ts = take((size_t)8 * B * 4), o_cg = take((size_t)8 * B * 4),
                 o_p = take((size_t)2 * B * nblk * 8), o_g = take((size_t)ng * sizeof(OdeGroup)), o_d = take(sizeof(int));
    if (hipMalloc((void**)&o->buf, off) != hipSuccess) { (void)hipGetLastError(); delete o; return fail(USE_E_NOMEM, "cannot allocate %.1f MB for the ODE stepper", off / 1e6); }
    if (hipHostMalloc((void**)&o->done_host, sizeof(int), 0) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(o->buf); delete o; return fail(USE_E_NOMEM, "pinned host word"); }
    if (hipMemset(o->buf, 0, off) != hipSuccess) { (void)use_ode_destroy(o); return fail(USE_E_HIP, "hipMemset of the ODE stepper failed"); }
    OdeDev& d = o->d;
    d.y = (double2*)(o->buf + o_y); d.ynew = (double2*)(o->buf + o_yn); d.K = (float2*)(o->buf + o_K); d.xin = (float2*)(o->buf + o_x);
    o->ysde_buf = (float2*)(o->buf + o_ys); d.ysde = o->ysde_buf;
    d.h_item = (double*)(o->buf + o_h); d.ts = (float*)(o->buf + o_ts); d.cg = (float*)(o->buf + o_cg); d.part = (double*)(o->buf + o_p);
    d.grp = (OdeGroup*)(o->buf + o_g); d.done = (int*)(o->buf + o_d);
    d.n_per_b = (long)n_per_item; d.B = B; d.G = G; d.nblk = nblk;
    d.theta = h->cfg.theta; d.rtol = float_as_decimal(cfg->rtol); d.atol = float_as_decimal(cfg->atol);
    OdeCtl& c = o->c;
    c.t0 = 1.0; c.t_bound = float_as_decimal(cfg->t_eps);                       // sde.T = 1 (sdes.py:201)
    c.first_step = cfg->first_step > 0 ? float_as_decimal(cfg->first_step) : 0.0;
    c.max_step = cfg->max_step > 0 ? float_as_decimal(cfg->max_step) : INFINITY;
    c.max_nfe = cfg->max_nfe > 0 ? cfg->max_nfe : 10000;
    c.ngroups = ng; c.G = G; c.B = B; c.nblk = nblk; c.n_per_b = (long)n_per_item;
    {   // the OUVE constants as the reference's Python floats (sdes.py:205-221), cast to float32 where torch meets a float32 tensor
        const double smin = float_as_decimal(h->cfg.sigma_min), smax = float_as_decimal(h->cfg.sigma_max);
        c.sigma_min = h->cfg.sigma_min; c.base = (float)(smax / smin); c.sq2ls = (float)std::sqrt(2 * std::log(smax / smin));
    }
    *out = o;
    return USE_OK;
}

int use_ode_destroy(use_ode* o) {
    if (!o) return USE_OK;
    (void)hipSetDevice(o->h->device);
    (void)hipDeviceSynchronize();
    if (o->buf) (void)hipFree(o->buf);
    if (o->done_host) (void)hipHostFree(o->done_host);
    delete o;
    return USE_OK;
}

int use_ode_num_groups(use_ode* o) { return o ? o->c.ngroups : fail(USE_E_INVALID, "null stepper"); }

int use_ode_start(use_ode* o, const void* y_sde, const void* x0, use_stream_t stream) {
    if (!o || !y_sde || !x0) return fail(USE_E_INVALID, "null argument");
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)o->d.B * o->d.n_per_b;
    o->d.ysde = o->ysde_buf;
    HIPCHK(hipMemcpyAsync(o->ysde_buf, y_sde, n * 8, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(o->d.xin, x0, n * 8, hipMemcpyDeviceToDevice, s));
    ode_start_impl(o, s);
    HIPCHK(hipGetLastError());
    return USE_OK;
}

int use_ode_request(use_ode* o, void* x, float* t, use_stream_t stream) {
    if (!o || !x || !t) return fail(USE_E_INVALID, "null argument");
    if (o->phase < 0) return fail(USE_E_STATE, "use_ode_start has not been called");
    hipStream_t s = (hipStream_t)stream;
    if (o->phase == 1) {                                   // the start of a step: is any group still running?
        bool done = false;
        int rc = ode_all_done(o, s, &done); if (rc) return rc;
        if (done) return 0;
    }
    const size_t n = (size_t)o->d.B * o->d.n_per_b;
    HIPCHK(hipMemcpyAsync(x, o->d.xin, n * 8, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(t, o->d.ts + (size_t)o->phase * o->d.B, (size_t)o->d.B * 4, hipMemcpyDeviceToDevice, s));
    return 1;
}

int use_ode_supply(use_ode* o, const void* f, int kind, use_stream_t stream) {
    if (!o || !f) return fail(USE_E_INVALID, "null argument");
    if (o->phase < 0) return fail(USE_E_STATE, "use_ode_start has not been called");
    if (kind != 0 && kind != 1) return fail(USE_E_INVALID, "kind: 0 = drift, 1 = score");
    ode_supply_impl(o, (const float2*)f, kind, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return USE_OK;
}

int use_ode_state(use_ode* o, double* t, double* h_abs, int* nfev, int* status, int* steps, use_stream_t stream) {
    if (!o) return fail(USE_E_INVALID, "null stepper");
    std::vector<OdeGroup> g;
    int rc = ode_read_groups(o, g, (hipStream_t)stream); if (rc) return rc;
    for (size_t i = 0; i < g.size(); ++i) {
        if (t) t[i] = g[i].t;
        if (h_abs) h_abs[i] = g[i].h_abs;
        if (nfev) nfev[i] = g[i].nfev;
        if (status) status[i] = g[i].status;
        if (steps) steps[i] = g[i].steps;
    }
    return USE_OK;
}

int use_ode_result(use_ode* o, void* out, int* nfev, int* status, use_stream_t stream) {
    if (!o || !out) return fail(USE_E_INVALID, "null argument");
    launch_ode_result(o->d, (float2*)out, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return use_ode_state(o, nullptr, nullptr, nfev, status, nullptr, stream);
}

int use_set_ode(use_handle* h, const use_ode_config* oc) {
    int rc = check_ready(h); if (rc) return rc;
    if (h->cfg.unconditional || h->cfg.input_channels == 2 || h->cfg.no_sigma_scale)
        return fail(USE_E_STATE, "the ODE sampler needs the conditional 4- or 6-channel score network");
    rc = ode_check_config(oc); if (rc) return rc;
    h->plan->oc = *oc;
    h->plan->ode_set = true;
    return USE_OK;
}

int use_sample_ode(use_handle* h, const void* y, const void* cond, const void* cond2, const void* noise, uint64_t seed, void* out,
                   int* nfev, int* status, use_stream_t stream) {
    int rc = check_sample_args(h, &Plan::ode_set, "use_set_ode has not been called", y, cond2, out, "");
    if (rc) return rc;
    Plan& pl = *h->plan;
    hipStream_t s = (hipStream_t)stream;
    const long n_per_b = (long)h->cfg.n_freq * pl.T, n = (long)pl.B * n_per_b;
    use_ode* o = h->ode_run;
    if (!o || o->d.B != pl.B || o->d.n_per_b != n_per_b || memcmp(&o->cfg, &pl.oc, sizeof pl.oc)) {
        HIPCHK(hipStreamSynchronize(s));
        if (h->ode_graph) { (void)hipGraphExecDestroy(h->ode_graph); h->ode_graph = nullptr; }   // it holds the old stepper's buffers
        if (o) (void)use_ode_destroy(o);
        h->ode_run = nullptr;
        rc = use_ode_create(h, pl.B, n_per_b, &pl.oc, &h->ode_run); if (rc) return rc;
        o = h->ode_run;
    }
    rc = load_sampler_inputs(h, y, cond, cond2, s); if (rc) return rc;
    o->d.ysde = pl.Y;
    const float2* c2 = h->pcp == 8 ? pl.cond2_buf : nullptr;
    auto eval = [&](int row) {                              // the network at the items' stage times, into pl.score
        const float* t = o->d.ts + (size_t)row * pl.B;
        run_temb(h, t, pl.B, pl.silu_temb, pl.tembias, s);
        run_score(h, o->d.xin, pl.Cond, pl.tembias, h->dense_rows, t, 1, pl.score, s, -1.f, c2);
    };
    auto step = [&](hipStream_t st) {                       // one RK45 attempt per running group: 6 evaluations
        for (int r = 1; r <= 6; ++r) {
            const float* t = o->d.ts + (size_t)r * pl.B;
            run_temb(h, t, pl.B, pl.silu_temb, pl.tembias, st);
            run_score(h, o->d.xin, pl.Cond, pl.tembias, h->dense_rows, t, 1, pl.score, st, -1.f, c2);
            ode_supply_impl(o, pl.score, 1, st);
        }
    };
    // 1. prior: draw 0 of the Philox stream (use_sample's), or the given draw
    hipLaunchKernelGGL(set_rng_kernel, dim3(1), dim3(1), 0, s, pl.seeds, (unsigned long long)seed);
    launch_prior(pl.Y, (const float2*)noise, SdeRng{pl.seeds, 0}, ouve_std(h->cfg, 1.0f), o->d.xin, 1, n, s);
    // 2. f0 and select_initial_step
    ode_start_impl(o, s);
    eval(0); ode_supply_impl(o, pl.score, 1, s);
    if (o->phase == 7) { eval(7); ode_supply_impl(o, pl.score, 1, s); }
    HIPCHK(hipGetLastError());
    rc = eval_status(h); if (rc) return rc;
    // 3. steps until every group is done
    if (pl.oc.use_graph) {
        const std::vector<const void*> key = {o, o->buf, pl.persist, pl.arena.base, pl.Cond, c2, pl.Y, h->blob};   // (use_plan drops it too)
        if (h->ode_graph && key != h->ode_graph_key) { (void)hipGraphExecDestroy(h->ode_graph); h->ode_graph = nullptr; }
        if (!h->ode_graph) {
            rc = ensure_cap_stream(h); if (rc) return rc;
            rc = capture_graph(h, "the RK45 step", step, &h->ode_graph);
            o->phase = 1;                                         // (the recording walked the stepper's host-side phase through a step)
            if (rc) return rc;
            h->ode_graph_key = key;
        }
    }
    for (;;) {
        bool done = false;
        rc = ode_all_done(o, s, &done); if (rc) return rc;
        if (done) break;
        if (h->ode_graph && pl.oc.use_graph) HIPCHK(hipGraphLaunch(h->ode_graph, s));
        else { step(s); HIPCHK(hipGetLastError()); rc = eval_status(h); if (rc) return rc; }
    }
    // 4. denoise: one reverse-diffusion step at t_eps without its noise (x_mean); 5. out
    launch_ode_result(o->d, pl.X, s);
    if (pl.oc.denoise) {
        hipLaunchKernelGGL(fill_f32_kernel, dim3(1), dim3(256), 0, s, pl.t_dev, pl.oc.t_eps, pl.B);
        run_temb(h, pl.t_dev, pl.B, pl.silu_temb, pl.tembias, s);
        run_score(h, pl.X, pl.Cond, pl.tembias, h->dense_rows, pl.t_dev, 1, pl.score, s, -1.f, c2);
        float cd, cs, cn; predictor_coeffs(h->cfg, USE_PRED_REVERSE_DIFFUSION, pl.oc.t_eps, pl.oc.N, cd, cs, cn);
        launch_predictor(pl.X, pl.Y, pl.score, nullptr, SdeRng{pl.seeds, 1}, cd, cs, cn, pl.Xmean, (float2*)out, 1, n, s);
    } else {
        HIPCHK(hipMemcpyAsync(out, pl.X, (size_t)n * 8, hipMemcpyDeviceToDevice, s));
    }
    HIPCHK(hipGetLastError());
    rc = eval_status(h); if (rc) return rc;
    std::vector<OdeGroup> g;
    rc = ode_read_groups(o, g, s); if (rc) return rc;
    h->ode_steps = h->ode_rejected = h->ode_nfev_max = 0;
    for (size_t i = 0; i < g.size(); ++i) {
        h->ode_steps += g[i].steps; h->ode_rejected += g[i].nrej; h->ode_nfev_max = std::max<long long>(h->ode_nfev_max, g[i].nfev);
        if (nfev) nfev[i] = g[i].nfev;
        if (status) status[i] = g[i].status;
    }
    return USE_OK;
}

int use_spec_fwd(const void* stft, void* Y, int B, int F, int T, int Tpad, float factor, float exponent, use_stream_t s) {
    if (!stft || !Y || B < 1 || F < 1 || T < 1 || Tpad < T) return fail(USE_E_INVALID, "bad arguments");
    launch_spec_map((const float2*)stft, (float2*)Y, (long)B * F, T, T, Tpad, 1.f, exponent, factor, (hipStream_t)s);
    HIPCHK(hipGetLastError());
    return USE_OK;
}
int use_spec_back(const void* X, void* stft, int B, int F, int T, int Tpad, float factor, float exponent, use_stream_t s) {
    if (!stft || !X || B < 1 || F < 1 || T < 1 || Tpad < T || factor == 0.f || exponent == 0.f) return fail(USE_E_INVALID, "bad arguments");
    launch_spec_map((const float2*)X, (float2*)stft, (long)B * F, T, Tpad, T, 1.f / factor, 1.f / exponent, 1.f, (hipStream_t)s);
    HIPCHK(hipGetLastError());
    return USE_OK;
}

// ---- chunked sampling: window geometry, device split and cross-fade merge (handle-free; no reference counterpart) -----------
// n = 1 for Tp <= C (no chunking), else ceil((Tp - overlap) / hop) windows at k * hop, hop = C - overlap; the last may run past Tp
static int chunk_geometry(int Tp, int C, int overlap, int* n) {
    if (Tp < 64 || Tp % 64 != 0) return fail(USE_E_INVALID, "Tp=%d: the padded frame count must be a positive multiple of 64", Tp);
    if (C < 64 || C % 64 != 0) return fail(USE_E_INVALID, "chunk_frames=%d must be a positive multiple of 64", C);
    if (overlap < 0 || overlap > C / 2) return fail(USE_E_INVALID, "overlap=%d must lie in 0 ... chunk_frames / 2 = %d", overlap, C / 2);
    const int hop = C - overlap;
    *n = Tp <= C ? 1 : (Tp - overlap + hop - 1) / hop;
    return USE_OK;
}
int use_chunk_count(int Tp, int C, int overlap) {
    int n = 0;
    const int rc = chunk_geometry(Tp, C, overlap, &n);
    return rc ? rc : n;
}
static int chunk_args(const void* a, const void* b, int B, int F, int Tp, int C, int overlap, int* n) {
    if (!a || !b) return fail(USE_E_INVALID, "null tensor");
    if (B < 1 || F < 1) return fail(USE_E_INVALID, "B=%d and F=%d must be positive", B, F);
    const int rc = chunk_geometry(Tp, C, overlap, n); if (rc) return rc;
    if ((long long)B * *n * F > (1ll << 30)) return fail(USE_E_INVALID, "B * n * F = %lld rows exceed 2^30", (long long)B * *n * F);
    return USE_OK;
}
int use_chunk_split(const void* Y, void* chunks, int B, int F, int Tp, int C, int overlap, use_stream_t s) {
    int n = 0;
    const int rc = chunk_args(Y, chunks, B, F, Tp, C, overlap, &n); if (rc) return rc;
    launch_chunk_split((const float2*)Y, (float2*)chunks, B, F, n, Tp, C, overlap, (hipStream_t)s);
    HIPCHK(hipGetLastError());
    return USE_OK;
}
int use_chunk_merge(const void* chunks, void* X, int B, int F, int Tp, int C, int overlap, use_stream_t s) {
    int n = 0;
    const int rc = chunk_args(chunks, X, B, F, Tp, C, overlap, &n); if (rc) return rc;
    launch_chunk_merge((const float2*)chunks, (float2*)X, B, F, n, Tp, C, overlap, (hipStream_t)s);
    HIPCHK(hipGetLastError());
    return USE_OK;
}

// ---- evaluation metrics: SI-SDR / SI-SIR / SI-SAR and LSD per item (handle-free; reference sgmse/util/other.py:15-62) -----------
size_t use_metrics_workspace(int B, int stride) {
    if (B < 1 || B > 65535 || stride < 1) return 0;
    return metrics_layout(B, stride).bytes;
}
int use_metrics(const float* est, const float* clean, const float* noise, const int* len_host, int B, int stride, void* work,
                size_t work_bytes, double* out_dev, use_stream_t s) {
    if (B < 1 || B > 65535) return fail(USE_E_INVALID, "B=%d must lie in 1 ... 65535", B);
    if (stride < 1) return fail(USE_E_INVALID, "stride=%d must be positive", stride);
    if (!est) return fail(USE_E_INVALID, "est is null");
    if (!clean) return fail(USE_E_INVALID, "clean is null");
    if (!len_host) return fail(USE_E_INVALID, "len_host is null");
    if (!work) return fail(USE_E_INVALID, "work is null");
    if (!out_dev) return fail(USE_E_INVALID, "out_dev is null");
    for (int b = 0; b < B; ++b)
        if (len_host[b] < 256 || len_host[b] > stride)
            return fail(USE_E_INVALID, "len[%d]=%d must lie in 256 ... stride = %d (reflect padding of the 510-point STFT needs more than 255 samples)",
                        b, len_host[b], stride);
    const size_t need = metrics_layout(B, stride).bytes;
    if (work_bytes < need) return fail(USE_E_INVALID, "work_bytes=%zu is smaller than use_metrics_workspace(%d, %d) = %zu", work_bytes, B, stride, need);
    if ((uintptr_t)work & 7) return fail(USE_E_INVALID, "work must be 8-byte aligned");
    launch_metrics(est, clean, noise, len_host, B, stride, work, out_dev, (hipStream_t)s);
    HIPCHK(hipGetLastError());
    return USE_OK;
}

// ---- device STFT / iSTFT fused with the spectrogram glue (handle-free) -----------------------------------------
namespace {
std::mutex g_tw_mutex;
std::map<std::pair<int, int>, float2*> g_tw_tables;          // (device, n_fft) -> (cos, sin)(2 pi m / n_fft); lives for the process
int twiddles(int n_fft, hipStream_t s, const float2** out) {
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_tw_mutex);
    auto it = g_tw_tables.find({dev, n_fft});
    if (it == g_tw_tables.end()) {                            // first use on this device: build the table (synchronises once)
        float2* tw = nullptr;
        HIPCHK(hipMalloc((void**)&tw, (size_t)n_fft * sizeof(float2)));
        launch_twiddle_table(tw, n_fft, s);
        HIPCHK(hipStreamSynchronize(s));
        it = g_tw_tables.emplace(std::make_pair(dev, n_fft), tw).first;
    }
    *out = it->second;
    return USE_OK;
}
int check_stft_args(int B, int L, int n_fft, int hop, int Tpad) {
    if (B < 1 || L < 1 || n_fft < 4 || (n_fft & 1) || hop < 1 || hop > n_fft) return fail(USE_E_INVALID, "bad STFT arguments (n_fft must be even, 1 <= hop <= n_fft)");
    if (L <= n_fft / 2) return fail(USE_E_INVALID, "signal of %d samples is too short for reflect padding with n_fft=%d", L, n_fft);
    if (Tpad < 1 + L / hop) return fail(USE_E_INVALID, "Tpad=%d is smaller than the %d frames of the signal", Tpad, 1 + L / hop);
    if ((size_t)n_fft * 8 + (size_t)((n_fft + hop - 1) / hop) * (n_fft / 2 + 1) * 8 > 64 * 1024) return fail(USE_E_INVALID, "n_fft / hop combination exceeds the synthesis kernel's LDS");
    return USE_OK;
}
}  // namespace

int use_stft_fwd(const float* wav, void* Y, int B, int L, int n_fft, int hop, const float* window, int Tpad, float factor,
                 float exponent, use_stream_t s) {
    if (!wav || !Y || !window) return fail(USE_E_INVALID, "null argument");
    int rc = check_stft_args(B, L, n_fft, hop, Tpad); if (rc) return rc;
    const float2* tw = nullptr;
    rc = twiddles(n_fft, (hipStream_t)s, &tw); if (rc) return rc;
    launch_stft_fwd(wav, window, tw, (float2*)Y, B, L, n_fft, hop, 1 + L / hop, Tpad, factor, exponent, (hipStream_t)s);
    HIPCHK(hipGetLastError());
    return USE_OK;
}
int use_istft_back(const void* X, float* wav, int B, int L, int n_fft, int hop, const float* window, int Tpad, float factor,
                   float exponent, use_stream_t s) {
    if (!wav || !X || !window || factor == 0.f || exponent == 0.f) return fail(USE_E_INVALID, "bad arguments");
    int rc = check_stft_args(B, L, n_fft, hop, Tpad); if (rc) return rc;
    const float2* tw = nullptr;
    rc = twiddles(n_fft, (hipStream_t)s, &tw); if (rc) return rc;
    launch_istft_back((const float2*)X, window, tw, wav, B, L, n_fft, hop, Tpad, factor, exponent, (hipStream_t)s);
    HIPCHK(hipGetLastError());
    return USE_OK;
}

namespace {
int check_stft_items(const char* who, const int* len_host, int64_t stride, int B, int n_fft, int hop, int Tpad) {
    if (!len_host) return fail(USE_E_INVALID, "%s: len_host is null", who);
    if (B < 1) return fail(USE_E_INVALID, "%s: B=%d must be positive", who, B);
    if (n_fft < 4 || (n_fft & 1)) return fail(USE_E_INVALID, "%s: n_fft=%d must be even and at least 4", who, n_fft);
    if (hop < 1 || hop > n_fft) return fail(USE_E_INVALID, "%s: hop=%d must lie in 1 ... n_fft = %d", who, hop, n_fft);
    if (stride < 1 || stride > INT32_MAX) return fail(USE_E_INVALID, "%s: stride=%lld must lie in 1 ... 2^31 - 1", who, (long long)stride);
    if (Tpad < 1) return fail(USE_E_INVALID, "%s: Tpad=%d must be positive", who, Tpad);
    for (int b = 0; b < B; ++b) {
        const int L = len_host[b];
        if (L <= n_fft / 2) return fail(USE_E_INVALID, "%s: len[%d]=%d is too short for reflect padding with n_fft=%d (needs more than %d samples)", who, b, L, n_fft, n_fft / 2);
        if (L > stride) return fail(USE_E_INVALID, "%s: len[%d]=%d exceeds stride=%lld", who, b, L, (long long)stride);
        if (1 + L / hop > Tpad) return fail(USE_E_INVALID, "%s: len[%d]=%d has %d frames, more than Tpad=%d", who, b, L, 1 + L / hop, Tpad);
    }
    if ((size_t)n_fft * 8 + (size_t)((n_fft + hop - 1) / hop) * (n_fft / 2 + 1) * 8 > 64 * 1024) return fail(USE_E_INVALID, "%s: n_fft / hop combination exceeds the synthesis kernel's LDS", who);
    return USE_OK;
}
}  // namespace

int use_stft_fwd_items(const float* wav, int64_t stride, const int* len_host, void* Y, int B, int n_fft, int hop, const float* window,
                       int Tpad, float factor, float exponent, use_stream_t s) {
    if (!wav) return fail(USE_E_INVALID, "use_stft_fwd_items: wav is null");
    if (!Y) return fail(USE_E_INVALID, "use_stft_fwd_items: Y is null");
    if (!window) return fail(USE_E_INVALID, "use_stft_fwd_items: window is null");
    int rc = check_stft_items("use_stft_fwd_items", len_host, stride, B, n_fft, hop, Tpad); if (rc) return rc;
    const float2* tw = nullptr;
    rc = twiddles(n_fft, (hipStream_t)s, &tw); if (rc) return rc;
    launch_stft_fwd_items(wav, (long)stride, len_host, window, tw, (float2*)Y, B, n_fft, hop, Tpad, factor, exponent, (hipStream_t)s);
    HIPCHK(hipGetLastError());
    return USE_OK;
}
int use_istft_back_items(const void* X, float* wav, int64_t stride, const int* len_host, int B, int n_fft, int hop,
                         const float* window, int Tpad, float factor, float exponent, use_stream_t s) {
    if (!X) return fail(USE_E_INVALID, "use_istft_back_items: X is null");
    if (!wav) return fail(USE_E_INVALID, "use_istft_back_items: wav is null");
    if (!window) return fail(USE_E_INVALID, "use_istft_back_items: window is null");
    if (factor == 0.f || exponent == 0.f) return fail(USE_E_INVALID, "use_istft_back_items: factor and exponent must not be zero");
    int rc = check_stft_items("use_istft_back_items", len_host, stride, B, n_fft, hop, Tpad); if (rc) return rc;
    const float2* tw = nullptr;
    rc = twiddles(n_fft, (hipStream_t)s, &tw); if (rc) return rc;
    launch_istft_back_items((const float2*)X, window, tw, wav, (long)stride, len_host, B, n_fft, hop, Tpad, factor, exponent, (hipStream_t)s);
    HIPCHK(hipGetLastError());
    return USE_OK;
}

int use_sde_prior(use_handle* h, const void* y, const void* noise, uint64_t seed, void* x, int64_t n, use_stream_t s) {
    int rc = ensure_sde_scratch(h); if (rc) return rc;
    if (!y) return fail(USE_E_INVALID, "use_sde_prior: y is null");
    if (!x) return fail(USE_E_INVALID, "use_sde_prior: x is null");
    if (n < 1) return fail(USE_E_INVALID, "use_sde_prior: n=%lld must be positive", (long long)n);
    hipLaunchKernelGGL(set_rng_kernel, dim3(1), dim3(1), 0, (hipStream_t)s, h->sde_seeds, (unsigned long long)seed);
    launch_prior((const float2*)y, (const float2*)noise, SdeRng{h->sde_seeds, 0}, ouve_std(h->cfg, 1.0f), (float2*)x, 1, n, (hipStream_t)s);
    HIPCHK(hipGetLastError());
    return USE_OK;
}

int use_fill_noise_items(use_handle* h, const uint64_t* seeds_host, int B, int draw, void* out, int64_t n, use_stream_t s) {
    if (!seeds_host || !out || B < 1 || draw < 0 || n < 0 || n % B != 0) return fail(USE_E_INVALID, "use_fill_noise_items: null argument, or n is no multiple of B");
    if (B > use_handle::SDE_MAX_B) return fail(USE_E_INVALID, "B=%d exceeds %d", B, use_handle::SDE_MAX_B);
    int rc = ensure_sde_scratch(h); if (rc) return rc;
    if (n == 0) return USE_OK;
    upload_item_seeds(h->sde_seeds, seeds_host, B, (hipStream_t)s);
    launch_fill_noise((float2*)out, SdeRng{h->sde_seeds, (unsigned)draw}, B, (long)(n / B), (hipStream_t)s);
    HIPCHK(hipGetLastError());
    return USE_OK;
}

int use_fill_noise(use_handle* h, uint64_t seed, int draw, void* out, int64_t n, use_stream_t s) {
    // draw `draw` of the device noise stream of use_sample(noise = NULL, seed): element i = Philox4x32-10(key = seed, counter = (i, draw)),
    // Box-Muller on two uniforms u in (0, 1] (24 high bits + 0.5, rounded to float32: 1.0 occurs)
    int rc = ensure_sde_scratch(h); if (rc) return rc;
    if (!out || n < 1 || draw < 0) return fail(USE_E_INVALID, "bad arguments");
    hipLaunchKernelGGL(set_rng_kernel, dim3(1), dim3(1), 0, (hipStream_t)s, h->sde_seeds, (unsigned long long)seed);
    launch_fill_noise((float2*)out, SdeRng{h->sde_seeds, (unsigned)draw}, 1, (long)n, (hipStream_t)s);
    HIPCHK(hipGetLastError());
    return USE_OK;
}

int use_sde_predictor(use_handle* h, int predictor, float t, int N, const void* x, const void* y, const void* score,
                      const void* noise, uint64_t seed, void* x_out, void* x_mean, int64_t n, use_stream_t s) {
    int rc = ensure_sde_scratch(h); if (rc) return rc;
    if (predictor != USE_PRED_REVERSE_DIFFUSION && predictor != USE_PRED_EULER_MARUYAMA) return fail(USE_E_INVALID, "predictor id %d has no update kernel", predictor);
    if (!x) return fail(USE_E_INVALID, "use_sde_predictor: x is null");
    if (!y) return fail(USE_E_INVALID, "use_sde_predictor: y is null");
    if (!score) return fail(USE_E_INVALID, "use_sde_predictor: score is null");
    if (!x_out) return fail(USE_E_INVALID, "use_sde_predictor: x_out is null");
    if (n < 1) return fail(USE_E_INVALID, "use_sde_predictor: n=%lld must be positive", (long long)n);
    float cd, cs, cn; predictor_coeffs(h->cfg, predictor, t, N, cd, cs, cn);
    hipLaunchKernelGGL(set_rng_kernel, dim3(1), dim3(1), 0, (hipStream_t)s, h->sde_seeds, (unsigned long long)seed);
    launch_predictor((const float2*)x, (const float2*)y, (const float2*)score, (const float2*)noise, SdeRng{h->sde_seeds, 0},
                     cd, cs, cn, (float2*)x_out, (float2*)x_mean, 1, n, (hipStream_t)s);
    HIPCHK(hipGetLastError());
    return USE_OK;
}

int use_sde_corrector(use_handle* h, int corrector, float t, float snr, int B, const void* x, const void* score,
                      const void* noise, uint64_t seed, void* x_out, void* x_mean, int64_t n, use_stream_t st) {
    int rc = ensure_sde_scratch(h); if (rc) return rc;
    hipStream_t s = (hipStream_t)st;
    if (!x) return fail(USE_E_INVALID, "use_sde_corrector: x is null");
    if (!score) return fail(USE_E_INVALID, "use_sde_corrector: score is null");
    if (!x_out) return fail(USE_E_INVALID, "use_sde_corrector: x_out is null");
    if (n < 1) return fail(USE_E_INVALID, "use_sde_corrector: n=%lld must be positive", (long long)n);
    if (B < 1 || n % B != 0) return fail(USE_E_INVALID, "n must be a multiple of B");
    // every refusal comes before the first launch (the seed word is written by a kernel)
    if (corrector != USE_CORR_LANGEVIN && corrector != USE_CORR_ALD) return fail(USE_E_INVALID, "corrector id %d has no update kernel", corrector);
    if (corrector == USE_CORR_LANGEVIN && B > use_handle::SDE_MAX_B) return fail(USE_E_INVALID, "B=%d exceeds %d", B, use_handle::SDE_MAX_B);
    hipLaunchKernelGGL(set_rng_kernel, dim3(1), dim3(1), 0, s, h->sde_seeds, (unsigned long long)seed);
    const SdeRng rng{h->sde_seeds, 0};
    if (corrector == USE_CORR_LANGEVIN) {
        launch_langevin_norms((const float2*)score, (const float2*)noise, rng, false, h->sde_partial, B, n / B, use_handle::SDE_BLOCKS, s);
        launch_langevin_step(h->sde_partial, B, false, use_handle::SDE_BLOCKS, snr, h->sde_step, s);
        launch_corrector((const float2*)x, (const float2*)score, (const float2*)noise, rng, h->sde_step, 0.f, (float2*)x_out, (float2*)x_mean, 1, n, s);
    } else {
        const float sd = snr * ouve_std(h->cfg, t);
        launch_corrector((const float2*)x, (const float2*)score, (const float2*)noise, rng, nullptr, sd * sd * 2.f, (float2*)x_out, (float2*)x_mean, 1, n, s);
    }
    HIPCHK(hipGetLastError());
    return USE_OK;
}

// ---- single-convolution harness (kernel bring-up / A-B timing; no reference counterpart) ----------------------------------
namespace {
__global__ void fill_uniform_kernel(void* p, size_t n, int dtype, unsigned seed, float lo, float hi) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned long long z = (unsigned long long)i * 0x9E3779B97F4A7C15ull + ((unsigned long long)seed << 32 | 0x1234567u);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
    const float v = lo + (hi - lo) * (float)((z >> 40) * (1.0 / 16777216.0));
    if (dtype == DT_F32) ((float*)p)[i] = v;
    else if (dtype == DT_BF16) ((__bf16*)p)[i] = (__bf16)v;
    else ((_Float16*)p)[i] = (_Float16)v;
}
__global__ void to_float_kernel(const void* p, float* out, size_t n, int dtype) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = dtype == DT_F32 ? ((const float*)p)[i] : dtype == DT_BF16 ? (float)((const __bf16*)p)[i] : (float)((const _Float16*)p)[i];
}
}  // namespace

// use_conv_op::temb_bstride: 0 = Cout (one row per item), -1 = one row shared by the batch, else the stride in elements
static int op_temb_bstride(const use_conv_op* c) { return c->temb_bstride == 0 ? c->Cout : c->temb_bstride < 0 ? 0 : c->temb_bstride; }

// The network's input convolution as the engine issues it: 3x3 over the 4 (or 8: 6 + 2 padding) packed fp32 input channels: the one op
// whose channel counts are no multiples of 32.  use_op_conv runs it and use_conv_choice answers for it, with the weight copies the engine keeps
static bool op_is_net_input(int C0, int C1, int XC, int ntaps, int dt) { return dt == DT_F32 && (C0 == 4 || C0 == 8) && C1 == 0 && XC == 0 && ntaps == 9; }
// The op surface's weight layout as a launch description: Cout padded to 32 or to a multiple of 128, slab-major copies (wb / w2b) wherever
// conv_wide_kernel's K chunk divides the channels; the dimensions and types; no optional operand
static ConvDesc op_desc(int H, int W, int C0, int C1, int XC0, int XC1, int Cout, int ntaps, int dt, int odt, int act) {
    ConvDesc d{};
    d.H = H; d.W = W; d.C0 = C0; d.C1 = C1; d.XC0 = XC0; d.XC1 = XC1; d.Cout = Cout; d.ntaps = ntaps; d.in_dtype = dt; d.out_dtype = odt; d.act = act;
    d.cout_pad = Cout <= 32 ? 32 : (Cout + 127) / 128 * 128;
    const int XC = XC0 + XC1, ck = conv_v4_chunk(dt);
    d.w = true; d.wb = ntaps == 9 && d.cout_pad % 128 == 0 && (C0 + C1) % ck == 0;
    if (op_is_net_input(C0, C1, XC, ntaps, dt)) d.wb = odt != DT_F32 && C0 == 4 && d.cout_pad % 128 == 0;    // the engine's split-bf16 copy (lay_conv_in)
    d.w2 = XC > 0; d.w2b = XC > 0 && XC % ck == 0 && d.cout_pad % 128 == 0;
    return d;
}
// ... of a use_conv_op: the presence flags from the op's own fields (what use_op_conv launches and use_conv_choice asks about)
static ConvDesc op_conv_desc(const use_conv_op* c) {
    ConvDesc d = op_desc(c->H, c->W, c->C0, c->C1, c->XC0, c->XC1, c->Cout, c->ntaps == 1 ? 1 : 9, c->dtype, c->out_dtype, c->act);
    d.coef = c->coef != nullptr; d.res = c->res != nullptr; d.pyr = c->pyr != nullptr; d.temb = c->temb != nullptr;
    d.stats = c->stats != nullptr || c->stats_part != nullptr;
    return d;
}
// the operands of a use_conv_op other than its weights and its fused shortcut, into the launch arguments
static void op_conv_operands(const use_conv_op* c, const ConvDesc& d, const float* bias, ConvArgs& a) {
    a.B = c->B; a.H = c->H; a.W = c->W; a.Cout = c->Cout; a.ntaps = d.ntaps; a.in_dtype = d.in_dtype; a.out_dtype = d.out_dtype;
    a.src0 = c->src0; a.src1 = c->C1 ? c->src1 : nullptr; a.C0 = c->C0; a.C1 = c->C1; a.coef = c->coef; a.act = c->act;
    a.bias = bias; a.temb = c->temb; a.temb_bstride = op_temb_bstride(c); a.res = c->res; a.out_scale = c->out_scale;
    a.out = c->out; a.stats = c->stats; a.stats_part = c->stats_part;
}
// hipMalloc into a list the caller frees; null: out of memory
static void* dev_alloc(std::vector<void*>& bufs, size_t bytes) { void* q = nullptr; if (hipMalloc(&q, bytes) != hipSuccess) return nullptr; bufs.push_back(q); return q; }
// Host fp32 weights `hw` [Cout][Cin][ntaps] (and `hw2` [Cout][XC] of the fused shortcut) -> the kernels' layouts as `d` describes them, packed,
// uploaded into buffers added to `bufs` and entered into the weight fields of `a`.  false: an allocation failed.
static bool stage_conv_weights(const ConvDesc& d, const float* hw, const float* hw2, std::vector<void*>& bufs, ConvArgs& a) {
    auto stage = [&](const float* src, int cin, int ntaps, bool slab, const void** dst, const void** dstb) {
        ConvW w; w.cin = w.cin_src = cin; w.cout = w.cout_src = d.Cout; w.cout_pad = d.cout_pad; w.ntaps = ntaps; w.w_dtype = d.in_dtype;
        const size_t bytes = (size_t)ntaps * d.cout_pad * cin * dtype_size(d.in_dtype);
        char* q = (char*)dev_alloc(bufs, bytes); char* qb = slab ? (char*)dev_alloc(bufs, bytes) : nullptr;
        if (!q || (slab && !qb)) return false;
        std::vector<char> hp(bytes), hpb(slab ? bytes : 0);
        pack_conv_raw(src, w, hp.data(), slab ? hpb.data() : nullptr);
        (void)hipMemcpy(q, hp.data(), bytes, hipMemcpyHostToDevice);
        if (slab) (void)hipMemcpy(qb, hpb.data(), bytes, hipMemcpyHostToDevice);
        *dst = q; *dstb = qb;
        return true;
    };
    a.cout_pad = d.cout_pad;
    if (op_is_net_input(d.C0, d.C1, d.XC0 + d.XC1, d.ntaps, d.in_dtype)) {
        // the input convolution: the plain [cout_pad][9][C0] fp32 copy and, where op_desc says so, the split-bf16 copy
        // [cout_pad][CONV_IN_SPLIT_K] in the place of the slab-major one, as pack_conv lays them into the blob
        const void* none = nullptr;
        if (!stage(hw, d.C0, 9, false, &a.w, &none)) return false;
        if (d.wb) {
            ConvW w; w.cin = w.cin_src = d.C0; w.cout = w.cout_src = d.Cout; w.cout_pad = d.cout_pad; w.ntaps = 9; w.w_dtype = DT_F32;
            const size_t bytes = (size_t)d.cout_pad * CONV_IN_SPLIT_K * 2;
            char* q = (char*)dev_alloc(bufs, bytes);
            if (!q) return false;
            std::vector<char> hp(bytes);
            pack_conv_in_split(hw, w, hp.data());
            (void)hipMemcpy(q, hp.data(), bytes, hipMemcpyHostToDevice);
            a.wb = q;
        }
        return true;
    }
    return stage(hw, d.C0 + d.C1, d.ntaps, d.wb, &a.w, &a.wb) && (!d.w2 || stage(hw2, d.XC0 + d.XC1, 1, d.w2b, &a.w2, &a.w2b));
}

int use_conv_bench(const use_conv_case* c, float* out_host, float* stats_host, double* ms_avg, double* flops) {
    if (!c || c->B < 1 || c->H < 1 || c->W < 1 || c->C0 < 1 || c->Cout < 1) return fail(USE_E_INVALID, "bad conv case");
    const int dt = c->dtype;
    if (dt != DT_F32 && dt != DT_BF16 && dt != DT_F16) return fail(USE_E_INVALID, "bad dtype");
    const size_t es = dtype_size(dt);
    const int Cin = c->C0 + c->C1, XC = c->XC0 + c->XC1;
    const size_t px = (size_t)c->B * c->H * c->W;
    std::vector<void*> bufs;
    auto dalloc = [&](size_t bytes) { return dev_alloc(bufs, bytes); };
    auto cleanup = [&]() { for (void* q : bufs) (void)hipFree(q); };
    auto fill = [&](void* q, size_t n, int dtype, unsigned seed, float lo, float hi) {
        hipLaunchKernelGGL(fill_uniform_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, q, n, dtype, seed, lo, hi);
    };
    const ConvDesc d = op_desc(c->H, c->W, c->C0, c->C1, c->XC0, c->XC1, c->Cout, 9, dt, dt, c->act);
    ConvArgs a{};
    a.B = c->B; a.H = c->H; a.W = c->W; a.Cout = c->Cout; a.ntaps = 9; a.in_dtype = dt; a.out_dtype = dt;
    a.C0 = c->C0; a.C1 = c->C1; a.XC0 = c->XC0; a.XC1 = c->XC1; a.act = c->act; a.out_scale = c->res || XC ? 0.70710678f : 1.f;
    void* src0 = dalloc(px * c->C0 * es); void* src1 = c->C1 ? dalloc(px * c->C1 * es) : nullptr;
    void* x0 = c->XC0 ? dalloc(px * c->XC0 * es) : nullptr; void* x1 = c->XC1 ? dalloc(px * c->XC1 * es) : nullptr;
    void* res = c->res ? dalloc(px * c->Cout * es) : nullptr;
    void* out = dalloc(px * c->Cout * es);
    float* outf = (float*)dalloc(px * c->Cout * 4);
    float* coef = c->gn ? (float*)dalloc((size_t)c->B * Cin * 2 * 4) : nullptr;
    float* bias = (float*)dalloc((size_t)c->Cout * 4); float* temb = (float*)dalloc((size_t)c->B * c->Cout * 4);
    const size_t stats_bytes = (size_t)c->B * c->Cout * 2 * sizeof(long long);
    long long* stats = c->stats ? (long long*)dalloc(stats_bytes) : nullptr;
    if (!src0 || !out || !outf || (c->stats && !stats)) { cleanup(); return fail(USE_E_NOMEM, "conv bench allocation failed"); }
    fill(src0, px * c->C0, dt, 1, -2.f, 2.f); if (src1) fill(src1, px * c->C1, dt, 2, -2.f, 2.f);
    if (x0) fill(x0, px * c->XC0, dt, 3, -1.f, 1.f); if (x1) fill(x1, px * c->XC1, dt, 4, -1.f, 1.f);
    if (res) fill(res, px * c->Cout, dt, 5, -1.f, 1.f);
    if (coef) fill(coef, (size_t)c->B * Cin * 2, DT_F32, 6, -0.9f, 1.1f);
    fill(bias, c->Cout, DT_F32, 7, -0.5f, 0.5f); fill(temb, (size_t)c->B * c->Cout, DT_F32, 8, -0.5f, 0.5f);
    {
        std::vector<float> hw((size_t)c->Cout * Cin * 9), hw2((size_t)c->Cout * std::max(XC, 1));
        unsigned long long st = 88172645463325252ull;
        auto rnd = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (float)((st >> 40) * (1.0 / 16777216.0)) * 2.f - 1.f; };
        const float sc = 1.0f / std::sqrt((float)Cin * 9.f / 3.f);
        for (auto& v : hw) v = rnd() * sc;
        for (auto& v : hw2) v = rnd() * (1.0f / std::sqrt((float)std::max(XC, 1) / 3.f));
        if (!stage_conv_weights(d, hw.data(), hw2.data(), bufs, a)) { cleanup(); return fail(USE_E_NOMEM, "conv bench allocation failed"); }
    }
    a.src0 = src0; a.src1 = src1; a.x0 = x0; a.x1 = x1; a.coef = coef; a.bias = bias; a.temb = c->temb ? temb : nullptr;
    a.temb_bstride = c->Cout; a.res = res; a.out = out; a.stats = stats;
    const char* why = nullptr;
    auto run = [&]() -> int { return launch_conv_variant(a, c->variant, 0, &why); };
    if (getenv("USE_HIP_DBG")) a.dbg = atoi(getenv("USE_HIP_DBG"));     // ablation bits (USE_HIP_ABLATE kernels)
    unsigned long long* trace = nullptr;
    if (getenv("USE_HIP_TRACE")) {                            // bring-up (USE_HIP_TRACE_BUILD kernels): stamps of workgroup $USE_HIP_TRACE
        trace = (unsigned long long*)dalloc(512 * 8);
        if (trace) { (void)hipMemset(trace, 0, 512 * 8); a.trace = trace; a.dbg = atoi(getenv("USE_HIP_TRACE")); }
    }
    if (stats) (void)hipMemset(stats, 0, stats_bytes);
    if (run() != 0) {
        cleanup(); return fail(USE_E_INVALID, "variant %d cannot run this case%s%s", c->variant, why ? ": needs " : "", why ? why : "");
    }
    if (hipDeviceSynchronize() != hipSuccess) { cleanup(); return fail(USE_E_HIP, "conv bench: launch failed: %s", hipGetErrorString(hipGetLastError())); }
    if (trace) {
        unsigned long long hb[512];
        (void)hipMemcpy(hb, trace, sizeof hb, hipMemcpyDeviceToHost);
        for (int g = 0; g < 2; ++g) {                           // wave 0 / wave 4 (conv_v4 stamps both wave groups)
            unsigned long long prev = hb[g * 256 + 1];
            for (int i = 0; i < 125 && hb[g * 256 + 2 * i]; ++i) {
                fprintf(stderr, "[trace G%d] id %3llu  +%6llu  @%8llu\n", g, hb[g * 256 + 2 * i], hb[g * 256 + 2 * i + 1] - prev, hb[g * 256 + 2 * i + 1] - hb[1]);
                prev = hb[g * 256 + 2 * i + 1];
            }
        }
        a.trace = nullptr;
    }
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    const int iters = std::max(1, c->iters);
    (void)hipEventRecord(e0, 0);
    for (int i = 0; i < iters; ++i) run();
    (void)hipEventRecord(e1, 0);
    (void)hipEventSynchronize(e1);
    float ms = 0.f; (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (ms_avg) *ms_avg = ms / iters;
    if (flops) *flops = 2.0 * (double)px * c->Cout * ((double)Cin * 9 + XC);
    int rc = USE_OK;
    if (out_host) {
        hipLaunchKernelGGL(to_float_kernel, dim3((unsigned)((px * c->Cout + 255) / 256)), dim3(256), 0, 0, out, outf, px * c->Cout, dt);
        if (hipMemcpy(out_host, outf, px * c->Cout * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(USE_E_HIP, "copy back failed");
    }
    if (stats_host && stats) {                                // per (item, channel) totals of ONE launch, as floats
        (void)hipMemset(stats, 0, stats_bytes);
        run();
        std::vector<long long> hs((size_t)c->B * c->Cout * 2);
        if (hipMemcpy(hs.data(), stats, stats_bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(USE_E_HIP, "copy back failed");
        for (size_t i = 0; i < hs.size(); i += 2) {
            stats_host[i] = (float)((double)hs[i] / 1048576.0); stats_host[i + 1] = (float)((double)hs[i + 1] / 1048576.0);
        }
    }
    cleanup();
    return rc;
}

// ---- single operators on caller-owned device tensors (NHWC) with host fp32 weights: the kernels of the path one at a time, so that
// the per-operator golden vectors of the reference (tests/golden/fir.npz, resblock_*.npz, attn.npz) reach the HIP code itself ----
// what use_op_conv accepts (`who`: the entry point, for the message; net_input_ok: and the network's input convolution); no HIP call
static int op_conv_check(const use_conv_op* c, const char* who, bool net_input_ok = false) {
    if (!c || c->B < 1 || c->H < 1 || c->W < 1 || c->C0 < 1 || c->Cout < 1 || !c->src0 || !c->w || !c->out) return fail(USE_E_INVALID, "%s: bad argument", who);
    const int dt = c->dtype, odt = c->out_dtype;
    if ((dt != DT_F32 && dt != DT_BF16 && dt != DT_F16) || (odt != DT_F32 && odt != DT_BF16 && odt != DT_F16)) return fail(USE_E_INVALID, "%s: bad dtype", who);
    const int Cin = c->C0 + c->C1, XC = c->XC0 + c->XC1;
    if ((Cin % 32 != 0 || XC % 32 != 0 || (c->C1 && c->C0 % 32) || (c->XC1 && c->XC0 % 32)) && !(net_input_ok && op_is_net_input(c->C0, c->C1, XC, c->ntaps == 1 ? 1 : 9, dt)))
        return fail(USE_E_INVALID, "%s: channel counts must be multiples of 32 (zero-pad)", who);
    if (c->pyr && !c->w4) return fail(USE_E_INVALID, "%s: pyr without w4", who);
    if (!c->coef && c->gn_st0 && (!c->gn_gamma || !c->gn_beta || c->gn_groups < 1 || Cin % c->gn_groups || (c->C1 && !c->gn_st1)))
        return fail(USE_E_INVALID, "%s: in-kernel GroupNorm needs gn_gamma, gn_beta, gn_st1 (with C1) and groups dividing C0 + C1", who);
    if (XC && (!c->w2 || !c->x0)) return fail(USE_E_INVALID, "%s: shortcut without weights / input", who);
    return USE_OK;
}
// The partial-totals form of a use_op_conv (use_conv_op::stats_part): the count must be the dispatcher's for this op and these options
// (use_conv_choice), and the kernel the variant runs must know the form.  No HIP call.
static int op_conv_check_parts(const use_conv_op* c, const ConvDesc& d) {
    if (!c->stats_part && !c->stats_parts) return USE_OK;
    if (!c->stats_part || c->stats_parts < 1) return fail(USE_E_INVALID, "use_op_conv: stats_part and stats_parts > 0 go together");
    if (c->stats) return fail(USE_E_INVALID, "use_op_conv: stats_part and stats are two forms of the same totals (pass one)");
    const ConvChoice ch = conv_choose(d);
    const int v = c->variant;
    // what the variant's kernel writes: the dispatcher's kernel; the wide conv (a case it cannot run is refused below, with its own
    // message); of the kernels of variant 1 the split input convolution alone
    const bool knows = v == 0 ? ch.stats_parts > 0 : v == 1 ? ch.k == IN_SPLIT : v == 4 ? !conv_v4_unrunnable(d) : v == 5 ? !conv_v5_unrunnable(d) : false;
    if ((v == 4 && conv_v4_unrunnable(d)) || (v == 5 && conv_v5_unrunnable(d))) return USE_OK;
    if (!knows) return fail(USE_E_INVALID, "use_op_conv: the kernel of variant %d (%s) only knows atomic totals (stats)", v, v == 0 ? conv_kernel_name(ch.k) : "forced");
    if (c->stats_parts != ch.stats_parts)
        return fail(USE_E_INVALID, "use_op_conv: stats_parts = %d, but %s writes %d partial totals per (item, channel) here (use_conv_choice)",
                    c->stats_parts, conv_kernel_name(ch.k), ch.stats_parts);
    return USE_OK;
}
int use_op_conv(const use_conv_op* c, use_stream_t stream) {
    int rc = op_conv_check(c, "use_op_conv", true); if (rc) return rc;
    const ConvDesc d = op_conv_desc(c);
    const int Cin = c->C0 + c->C1, XC = c->XC0 + c->XC1;
    if (Cin % 32) {
        // the input convolution as the engine issues it: nothing in front of it and nothing fused behind it; the kernels store 16-byte
        // channel chunks, and the generic kernel that takes the 8-channel input stages 128 weight rows
        if (c->coef || c->gn_st0 || c->act || c->res || c->pyr || c->temb)
            return fail(USE_E_INVALID, "use_op_conv: the input convolution (C0 = %d) takes no GroupNorm, activation, residual, Combine or temb", c->C0);
        if (c->Cout % 8 || (c->C0 == 8 && d.cout_pad % 128))
            return fail(USE_E_INVALID, "use_op_conv: the input convolution needs Cout %% 8 == 0 (and Cout > 32 with C0 = 8), not %d", c->Cout);
    }
    if ((rc = op_conv_check_parts(c, d))) return rc;
    hipStream_t s = (hipStream_t)stream;
    std::vector<void*> bufs;
    auto dalloc = [&](size_t bytes) { return dev_alloc(bufs, bytes); };
    auto cleanup = [&]() { for (void* q : bufs) (void)hipFree(q); };
    ConvArgs a{};
    float* dbias = (float*)dalloc((size_t)d.cout_pad * 4);
    float* dw4 = c->pyr ? (float*)dalloc((size_t)d.cout_pad * 5 * 4) : nullptr;     // [cout_pad][4] then b4 [cout_pad], zero-padded
    if (!dbias || (c->pyr && !dw4) || !stage_conv_weights(d, c->w, c->w2, bufs, a)) { cleanup(); return fail(USE_E_NOMEM, "use_op_conv: allocation failed"); }
    {
        std::vector<float> hb((size_t)d.cout_pad, 0.f);
        if (c->bias) memcpy(hb.data(), c->bias, (size_t)c->Cout * 4);
        (void)hipMemcpy(dbias, hb.data(), hb.size() * 4, hipMemcpyHostToDevice);
        if (c->pyr) {
            std::vector<float> h4((size_t)d.cout_pad * 5, 0.f);
            memcpy(h4.data(), c->w4, (size_t)c->Cout * 4 * 4);
            if (c->b4) memcpy(h4.data() + (size_t)d.cout_pad * 4, c->b4, (size_t)c->Cout * 4);
            (void)hipMemcpy(dw4, h4.data(), h4.size() * 4, hipMemcpyHostToDevice);
        }
    }
    op_conv_operands(c, d, dbias, a);
    a.x0 = XC ? c->x0 : nullptr; a.x1 = c->XC1 ? c->x1 : nullptr; a.XC0 = c->XC0; a.XC1 = c->XC1;
    if (c->pyr) { a.pyr = c->pyr; a.w4 = dw4; a.b4 = dw4 + (size_t)d.cout_pad * 4; }
    if (!c->coef && c->gn_st0) {                              // finalised in the kernel, gn_inv_n as Fwd::conv computes it
        a.gn_st0 = c->gn_st0; a.gn_st1 = c->C1 ? c->gn_st1 : nullptr; a.gn_gamma = c->gn_gamma; a.gn_beta = c->gn_beta;
        a.gn_groups = c->gn_groups; a.gn_eps = c->gn_eps;
        a.gn_inv_n = 1.0f / ((float)(Cin / c->gn_groups) * (float)(c->H * c->W));
    }
    const char* why = nullptr;
    const int lr = launch_conv_variant(a, c->variant, s, &why);
    if (lr == -2) rc = fail(USE_E_INVALID, "use_op_conv: unknown variant %d", c->variant);
    else if (lr) rc = fail(USE_E_INVALID, "%s cannot run this case%s%s", c->variant == 2 ? "conv_v2" : c->variant == 4 ? "conv_v4" : c->variant == 5 ? "conv_v5" : "conv_sk",
                           why ? ": needs " : "", why ? why : "");
    if (hipStreamSynchronize(s) != hipSuccess && rc == USE_OK) rc = fail(USE_E_HIP, "use_op_conv: %s", hipGetErrorString(hipGetLastError()));
    cleanup();
    return rc;
}
// The kernel the dispatcher (variant 0) would run this op on under the current options, and the per-workgroup partial GroupNorm totals per
// (item, channel) that kernel could write (0: atomics only).  Host only: no HIP call, nothing is launched.
int use_conv_choice(const use_conv_op* c, char* name, int name_cap, int* stats_parts) {
    int rc = op_conv_check(c, "use_conv_choice", true); if (rc) return rc;
    const ConvChoice ch = conv_choose(op_conv_desc(c));
    if (name && name_cap > 0) { strncpy(name, conv_kernel_name(ch.k), (size_t)name_cap - 1); name[name_cap - 1] = 0; }
    if (stats_parts) *stats_parts = ch.stats_parts;
    return USE_OK;
}
// use_op_conv with the weights already in HBM (fp32 parameter tensors: the training path, where they change every step) and a
// caller-provided workspace: the weights are laid out by a kernel on `stream`, nothing is allocated and nothing synchronises.
static size_t conv_dev_layout(const use_conv_op* c, size_t* wbytes, bool* slab, int* cout_pad) {
    const ConvDesc d = op_conv_desc(c);                       // (the layout rule of the host-weight entries)
    *cout_pad = d.cout_pad; *slab = d.wb;
    *wbytes = ((size_t)d.ntaps * d.cout_pad * (d.C0 + d.C1) * dtype_size(d.in_dtype) + 255) / 256 * 256;
    return *wbytes * (*slab ? 2 : 1) + (size_t)*cout_pad * 4;
}
size_t use_op_conv_dev_workspace(const use_conv_op* c) {
    if (!c || c->C0 < 1 || c->Cout < 1) return 0;
    size_t wb; bool slab; int cp;
    return conv_dev_layout(c, &wb, &slab, &cp);
}
int use_op_conv_dev(const use_conv_op* c, int w_mode, void* work, size_t work_bytes, use_stream_t stream) {
    if (!c || c->B < 1 || c->H < 1 || c->W < 1 || c->C0 < 1 || c->Cout < 1 || !c->src0 || !c->w || !c->out || !work) return fail(USE_E_INVALID, "use_op_conv_dev: bad argument");
    const int dt = c->dtype, odt = c->out_dtype;
    if ((dt != DT_F32 && dt != DT_BF16 && dt != DT_F16) || (odt != DT_F32 && odt != DT_BF16 && odt != DT_F16)) return fail(USE_E_INVALID, "use_op_conv_dev: bad dtype");
    if (w_mode < 0 || w_mode > 2 || (w_mode == 2 && c->ntaps != 1)) return fail(USE_E_INVALID, "use_op_conv_dev: bad weight layout %d", w_mode);
    const int Cin = c->C0 + c->C1, ntaps = c->ntaps == 1 ? 1 : 9;
    if (Cin % 32 != 0 || (c->C1 && c->C0 % 32)) return fail(USE_E_INVALID, "use_op_conv_dev: channel counts must be multiples of 32 (zero-pad)");
    if (c->XC0 || c->XC1 || c->x0 || c->w2) return fail(USE_E_INVALID, "use_op_conv_dev: no fused shortcut in this form");
    if (c->pyr || c->gn_st0) return fail(USE_E_INVALID, "use_op_conv_dev: no Combine or in-kernel GroupNorm in this form");
    size_t wbytes; bool slab; int cout_pad;
    if (conv_dev_layout(c, &wbytes, &slab, &cout_pad) > work_bytes) return fail(USE_E_INVALID, "use_op_conv_dev: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    char* dw = (char*)work; char* dwb = slab ? dw + wbytes : nullptr;
    float* dbias = (float*)(dw + wbytes * (slab ? 2 : 1));
    launch_pack_conv_dev((const float*)c->w, w_mode, c->Cout, Cin, ntaps, cout_pad, dt, conv_v4_chunk(dt), dw, dwb, (const float*)c->bias, dbias, s);
    ConvArgs a{};
    op_conv_operands(c, op_conv_desc(c), dbias, a);
    a.w = dw; a.wb = dwb; a.cout_pad = cout_pad;
    launch_conv(a, s);
    HIPCHK(hipGetLastError());
    return USE_OK;
}
static bool op_dtype_ok(int dtype) { return dtype == DT_F32 || dtype == DT_BF16 || dtype == DT_F16; }
int use_op_fir(const void* src, int dtype, const float* coef, int act, void* out_act, void* out_raw, int B, int H, int W, int C, int up,
               use_stream_t stream) {
    if (!src || (!out_act && !out_raw) || B < 1 || H < 1 || W < 1 || C < 1) return fail(USE_E_INVALID, "use_op_fir: bad argument");
    if (!op_dtype_ok(dtype)) return fail(USE_E_INVALID, "use_op_fir: bad dtype %d", dtype);
    // a thread owns one 16-byte channel chunk: a remainder would be left unwritten
    const int vec = dtype == DT_F32 ? 4 : 8;
    if (C % vec) return fail(USE_E_INVALID, "use_op_fir: C = %d is not a multiple of %d (16-byte channel chunks)", C, vec);
    if (!up && (H < 2 || W < 2)) return fail(USE_E_INVALID, "use_op_fir: a %d x %d map has no x2 down-sampled output", H, W);
    if (up) launch_fir_up2(src, dtype, coef, act, out_act, out_raw, B, H, W, C, (hipStream_t)stream);
    else    launch_fir_down2(src, dtype, coef, act, out_act, out_raw, B, H, W, C, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return USE_OK;
}
// dynamic LDS a kernel gets without hipFuncAttributeMaxDynamicSharedMemorySize: 64 KB less the kernel's static LDS
static const size_t OP_LDS_DEFAULT = 65536;
int use_op_attention(const void* q, const void* k, const void* v, void* out, int dtype, int B, int N, int C, use_stream_t stream) {
    if (!q || !k || !v || !out || B < 1 || B > 65535 || N < 1 || C < 1) return fail(USE_E_INVALID, "use_op_attention: bad argument");
    if (!op_dtype_ok(dtype)) return fail(USE_E_INVALID, "use_op_attention: bad dtype %d", dtype);
    // one query row [C] and its scores [N] in LDS (fp32) beside 16 bytes of reduction scratch
    if ((size_t)(C + N) * 4 + 16 > OP_LDS_DEFAULT)
        return fail(USE_E_INVALID, "use_op_attention: (C + N) * 4 = %zu bytes of LDS per row, more than a launch gets", (size_t)(C + N) * 4);
    launch_attention(q, k, v, out, dtype, B, N, C, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return USE_OK;
}
// The GEMM form of the same core (launch_attention_gemm, the engine's path above 512 tokens) in a caller-provided workspace: the scores /
// probabilities [B][N][N], then v^T [B][C][N], both in `dtype`; the second starts 256-byte aligned
static size_t attn_gemm_vt_offset(int dtype, int B, int N) { return ((size_t)B * N * N * dtype_size(dtype) + 255) / 256 * 256; }
static bool attn_gemm_shape_ok(int dtype, int B, int N, int C) {
    return op_dtype_ok(dtype) && B >= 1 && B <= 65535 && N >= 1 && C >= 1 && (long long)B * N <= 0x7fffffffLL && attention_gemm_eligible(dtype, N, C);
}
size_t use_op_attention_gemm_workspace(int dtype, int B, int N, int C) {
    if (!attn_gemm_shape_ok(dtype, B, N, C)) return 0;
    return attn_gemm_vt_offset(dtype, B, N) + (size_t)B * C * N * dtype_size(dtype);
}
int use_op_attention_gemm(const void* q, const void* k, const void* v, void* out, void* work, size_t work_bytes, int dtype, int B, int H, int W,
                          int C, use_stream_t stream) {
    if (!q || !k || !v || !out || !work || H < 1 || W < 1 || (long long)H * W > 0x7fffffffLL) return fail(USE_E_INVALID, "use_op_attention_gemm: bad argument");
    if (!op_dtype_ok(dtype)) return fail(USE_E_INVALID, "use_op_attention_gemm: bad dtype %d", dtype);
    const int N = H * W;
    if (!attn_gemm_shape_ok(dtype, B, N, C))
        return fail(USE_E_INVALID, "use_op_attention_gemm: the GEMM form runs N = H W > 512 tokens with N %% 128 == 0 and C %% 128 == 0 (B %d, N %d, C %d)", B, N, C);
    if (work_bytes < use_op_attention_gemm_workspace(dtype, B, N, C)) return fail(USE_E_INVALID, "use_op_attention_gemm: workspace too small");
    if ((uintptr_t)work % 16) return fail(USE_E_INVALID, "use_op_attention_gemm: the workspace must be 16-byte aligned");
    launch_attention_gemm(q, k, v, out, work, (char*)work + attn_gemm_vt_offset(dtype, B, N), dtype, B, H, W, C, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return USE_OK;
}
int use_op_attn_block(const void* x, const long long* gn_st, const float* gamma, const float* beta, int groups, float eps, const void* wq,
                      const void* wk, const void* wv, const void* wo, const float* bq, const float* bk, const float* bv, const float* bo,
                      void* out, long long* stats, int dtype, int B, int N, int C, use_stream_t stream) {
    if (!x || !gn_st || !gamma || !beta || !wq || !wk || !wv || !wo || !bq || !bk || !bv || !bo || !out || B < 1)
        return fail(USE_E_INVALID, "use_op_attn_block: bad argument");
    if (!op_dtype_ok(dtype)) return fail(USE_E_INVALID, "use_op_attn_block: bad dtype %d", dtype);
    if (!attn_fused_eligible(dtype, N, C))
        return fail(USE_E_INVALID, "use_op_attn_block: the fused block runs 16-bit storage, C = 256 and 1 <= N <= 96 (dtype %d, C %d, N %d)", dtype, C, N);
    if (groups < 1 || C % groups) return fail(USE_E_INVALID, "use_op_attn_block: %d groups do not divide C = %d", groups, C);
    AttnArgs a{};
    a.x = x; a.out = out; a.N = N;
    a.gn_st = gn_st; a.gn_gamma = gamma; a.gn_beta = beta; a.gn_groups = groups; a.gn_eps = eps;
    a.wq = wq; a.wk = wk; a.wv = wv; a.wo = wo; a.bq = bq; a.bk = bk; a.bv = bv; a.bo = bo;
    a.stats = stats;
    launch_attn_fused(a, dtype, B, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return USE_OK;
}
int use_op_combine_add(void* h, int dtype, const float* pyr, const float* w8, const float* b8, long long* stats, int B, int64_t pix_per_b, int C,
                       use_stream_t stream) {
    if (!h || !pyr || !w8 || !b8 || !stats || B < 1 || B > 65535 || pix_per_b < 1 || pix_per_b > 64LL * 0x7fffffff)
        return fail(USE_E_INVALID, "use_op_combine_add: bad argument");
    if (!op_dtype_ok(dtype)) return fail(USE_E_INVALID, "use_op_combine_add: bad dtype %d", dtype);
    const int vec = dtype == DT_F32 ? 4 : 8;
    if (C < vec || C > 512 || C % vec) return fail(USE_E_INVALID, "use_op_combine_add: C = %d is not a multiple of %d up to 512", C, vec);
    launch_combine_add(h, dtype, pyr, w8, b8, stats, B, (long)pix_per_b, C, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return USE_OK;
}
int use_op_temb_mlp(const float* t, int t_stride, const float* gfp_w, const float* w1, const float* b1, const float* w2, const float* b2,
                    float* out_silu, int B, int nf, use_stream_t stream) {
    if (!t || !gfp_w || !w1 || !b1 || !w2 || !b2 || !out_silu || B < 1 || nf < 1 || t_stride < 0) return fail(USE_E_INVALID, "use_op_temb_mlp: bad argument");
    if ((size_t)6 * nf * 4 > OP_LDS_DEFAULT) return fail(USE_E_INVALID, "use_op_temb_mlp: nf = %d needs %zu bytes of LDS, more than a launch gets", nf, (size_t)6 * nf * 4);
    launch_temb_mlp(t, t_stride, gfp_w, w1, b1, w2, b2, out_silu, B, nf, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return USE_OK;
}
int use_op_temb_dense(const float* silu_temb, const float* W, const float* bias, float* out, int B, int rows, int dim, use_stream_t stream) {
    if (!silu_temb || !W || !bias || !out || B < 1 || B > 65535 || rows < 1 || dim < 1) return fail(USE_E_INVALID, "use_op_temb_dense: bad argument");
    launch_temb_dense(silu_temb, W, bias, out, B, rows, dim, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return USE_OK;
}
int use_op_score_out(const float* pyr, int pc, const float* t, int t_stride, const float* w, const float* bias, void* score, int B,
                     int64_t pix_per_b, float sign, use_stream_t stream) {
    if (!pyr || !w || !bias || !score || B < 1 || B > 65535 || pix_per_b < 1 || t_stride < 0) return fail(USE_E_INVALID, "use_op_score_out: bad argument");
    if (pc != 4 && pc != 8) return fail(USE_E_INVALID, "use_op_score_out: %d pyramid channels (4 or 8)", pc);
    launch_score_out(pyr, pc, t, t_stride, w, bias, (float2*)score, B, (long)pix_per_b, sign, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return USE_OK;
}
int use_op_pack_input(const void* x, const void* y, const void* y2, float* x4, int64_t npix, use_stream_t stream) {
    if (!x || !x4 || npix < 1 || (y2 && !y)) return fail(USE_E_INVALID, "use_op_pack_input: bad argument");
    launch_pack_input((const float2*)x, (const float2*)y, (const float2*)y2, x4, (long)npix, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return USE_OK;
}
int use_op_softmax_rows(void* x, int dtype, int64_t rows, int cols, use_stream_t stream) {
    if (!x || rows < 1 || rows > 0x7fffffff || cols < 1) return fail(USE_E_INVALID, "use_op_softmax_rows: bad argument");
    if (!op_dtype_ok(dtype)) return fail(USE_E_INVALID, "use_op_softmax_rows: bad dtype %d", dtype);
    launch_softmax_rows(x, dtype, (long)rows, cols, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return USE_OK;
}
int use_op_transpose_nc(const void* in, void* out, int dtype, int B, int N, int C, use_stream_t stream) {
    if (!in || !out || B < 1 || B > 65535 || N < 1 || C < 1 || (C + 31) / 32 > 65535) return fail(USE_E_INVALID, "use_op_transpose_nc: bad argument");
    if (!op_dtype_ok(dtype)) return fail(USE_E_INVALID, "use_op_transpose_nc: bad dtype %d", dtype);
    launch_transpose_nc(in, out, dtype, B, N, C, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return USE_OK;
}
int use_op_gn_finalize(const long long* st0, int C0, const long long* st1, int C1, const float* gamma, const float* beta, int groups,
                       int hw, float eps, float* coef, int B, use_stream_t stream) {
    if (!st0 || !gamma || !beta || !coef || C0 < 1 || groups < 1 || (C0 + C1) % groups) return fail(USE_E_INVALID, "use_op_gn_finalize: bad argument");
    launch_gn_finalize(st0, C0, C1 ? st1 : nullptr, C1, gamma, beta, groups, hw, eps, coef, B, (hipStream_t)stream);
    return USE_OK;
}
// launch_gn_finalize with either form per source: totals st_i [B][C_i][2], or nt_i per-workgroup partial totals pt_i [B][nt_i][C_i][2]
// (use_conv_op::stats_part) - what Fwd::gn_coef issues for the large maps
int use_op_gn_finalize_parts(const long long* st0, const long long* pt0, int nt0, int C0, const long long* st1, const long long* pt1, int nt1, int C1,
                             const float* gamma, const float* beta, int groups, int hw, float eps, float* coef, int B, use_stream_t stream) {
    if (!gamma || !beta || !coef || C0 < 1 || C1 < 0 || B < 1 || hw < 1) return fail(USE_E_INVALID, "use_op_gn_finalize_parts: bad argument");
    if (groups < 1 || groups > 65535 || (C0 + C1) % groups) return fail(USE_E_INVALID, "use_op_gn_finalize_parts: %d groups do not divide C0 + C1 = %d", groups, C0 + C1);
    if ((st0 != nullptr) == (pt0 != nullptr) || (pt0 ? nt0 < 1 : nt0 != 0))
        return fail(USE_E_INVALID, "use_op_gn_finalize_parts: source 0 is either totals (st0, nt0 = 0) or nt0 > 0 partial totals (pt0)");
    if (C1 ? ((st1 != nullptr) == (pt1 != nullptr) || (pt1 ? nt1 < 1 : nt1 != 0)) : (st1 || pt1 || nt1))
        return fail(USE_E_INVALID, "use_op_gn_finalize_parts: source 1 is either totals (st1, nt1 = 0) or nt1 > 0 partial totals (pt1); nothing with C1 = 0");
    // gn_finalize_part_kernel: one 256-thread block per (item, group) writes the group's coefficients, a thread per channel
    if ((pt0 || pt1) && (C0 + C1) / groups > 256) return fail(USE_E_INVALID, "use_op_gn_finalize_parts: more than 256 channels per group");
    launch_gn_finalize(st0, C0, st1, C1, gamma, beta, groups, hw, eps, coef, B, (hipStream_t)stream, pt0, nt0, pt1, nt1);
    HIPCHK(hipGetLastError());
    return USE_OK;
}

// ---- backward operators (fp32 NHWC device tensors; SURVEY 8f4 minimum slice: one res-block) ----
size_t use_op_wgrad_workspace(int B, int H, int W, int Cout, int Cin, int ntaps, int dtype) {
    return (B < 1 || H < 1 || W < 1 || Cout < 1 || Cin < 1) ? 0 : wgrad_workspace_floats(B, H, W, Cout, Cin, ntaps == 1 ? 1 : 9, dtype);
}
int use_op_wgrad(const void* dy, const void* x, int dtype, float* dw, float* db, int B, int H, int W, int Cout, int Cin, int ntaps, float alpha,
                 float* work, size_t work_floats, use_stream_t stream) {
    if (!dy || !x || !dw || B < 1 || H < 1 || W < 1 || Cout < 1 || Cin < 1 || (ntaps != 1 && ntaps != 9)) return fail(USE_E_INVALID, "use_op_wgrad: bad argument");
    if (dtype != DT_F32 && dtype != DT_BF16 && dtype != DT_F16) return fail(USE_E_INVALID, "use_op_wgrad: bad dtype");
    if (work && work_floats < wgrad_workspace_floats(B, H, W, Cout, Cin, ntaps, dtype)) return fail(USE_E_INVALID, "use_op_wgrad: workspace too small");
    if (!launch_wgrad(dy, x, dtype, dw, db, B, H, W, Cout, Cin, ntaps, alpha, (work && work_floats) ? work : nullptr, (hipStream_t)stream))
        return fail(USE_E_INVALID, "use_op_wgrad: 16-bit inputs need the workspace and channel counts that are multiples of 4");
    HIPCHK(hipGetLastError());
    return USE_OK;
}
// workspace of the two GroupNorm operators, in floats (8-byte aligned): [fp64 slice partials][mean, rstd][s1, s2][m1, m2]
size_t use_op_gn_workspace(int B, int C, int groups) { return (B < 1 || C < 1 || groups < 1) ? 0 : gn_workspace_floats(B, C, groups); }
int use_op_gn_act_bwd(const void* x, const void* dy, int dtype, const float* gamma, const float* beta, int groups, float eps, int act, const void* add,
                      float add_scale, int B, int HW, int C, float* work, int have_stats, void* dx, float* dgamma, float* dbeta, use_stream_t stream) {
    if (!x || !dy || !gamma || !beta || !work || !dx || !dgamma || !dbeta || B < 1 || HW < 1 || C < 1 || groups < 1 || C % groups)
        return fail(USE_E_INVALID, "use_op_gn_act_bwd: bad argument");
    if (dtype != DT_F32 && dtype != DT_BF16 && dtype != DT_F16) return fail(USE_E_INVALID, "use_op_gn_act_bwd: bad dtype");
    if ((uintptr_t)work % 8) return fail(USE_E_INVALID, "use_op_gn_act_bwd: workspace must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)work;
    float* mean = work + (size_t)4 * B * GN_MAX_SLICES * std::max(C, groups); float* rstd = mean + (size_t)B * groups;
    float* s1 = rstd + (size_t)B * groups; float* s2 = s1 + (size_t)B * C; float* m12 = s2 + (size_t)B * C;
    // have_stats: `work` is the workspace use_op_gn_act_fwd ran in for the same x - its mean / rstd are reused, one pass over x saved
    if ((!have_stats && !launch_gn_stats(x, dtype, B, HW, C, groups, eps, mean, rstd, part, s)) ||
        !launch_gn_act_bwd(x, dy, dtype, mean, rstd, gamma, beta, act, add, add_scale, B, HW, C, groups, s1, s2, m12, part, dx, dgamma, dbeta, s))
        return fail(USE_E_INVALID, "use_op_gn_act_bwd: 16-bit tensors need C to be a multiple of 8 (and C / 8 <= 256)");
    HIPCHK(hipGetLastError());
    return USE_OK;
}
int use_op_gn_act_fwd(const void* x, int dtype, const float* gamma, const float* beta, int groups, float eps, int act, int B, int HW, int C, float* work,
                      void* y, use_stream_t stream) {
    if (!x || !gamma || !beta || !work || !y || B < 1 || HW < 1 || C < 1 || groups < 1 || C % groups) return fail(USE_E_INVALID, "use_op_gn_act_fwd: bad argument");
    if (dtype != DT_F32 && dtype != DT_BF16 && dtype != DT_F16) return fail(USE_E_INVALID, "use_op_gn_act_fwd: bad dtype");
    if ((uintptr_t)work % 8) return fail(USE_E_INVALID, "use_op_gn_act_fwd: workspace must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)work;
    float* mean = work + (size_t)4 * B * GN_MAX_SLICES * std::max(C, groups); float* rstd = mean + (size_t)B * groups;
    if (!launch_gn_stats(x, dtype, B, HW, C, groups, eps, mean, rstd, part, s) ||
        !launch_gn_act_fwd(x, dtype, mean, rstd, gamma, beta, act, B, HW, C, groups, y, s))
        return fail(USE_E_INVALID, "use_op_gn_act_fwd: 16-bit tensors need C to be a multiple of 8 (and C / 8 <= 256)");
    HIPCHK(hipGetLastError());
    return USE_OK;
}
int use_op_colsum(const void* x, int dtype, int B, int HW, int C, float scale, float* out, float* work, use_stream_t stream) {
    if (!x || !out || B < 1 || HW < 1 || C < 1) return fail(USE_E_INVALID, "use_op_colsum: bad argument");
    if (dtype != DT_F32 && dtype != DT_BF16 && dtype != DT_F16) return fail(USE_E_INVALID, "use_op_colsum: bad dtype");
    if (work && (uintptr_t)work % 8) return fail(USE_E_INVALID, "use_op_colsum: workspace must be 8-byte aligned");
    if (!launch_colsum(x, dtype, B, HW, C, scale, out, (double*)work, (hipStream_t)stream))
        return fail(USE_E_INVALID, "use_op_colsum: 16-bit tensors need the workspace (128 B C floats) and C a multiple of 8");
    HIPCHK(hipGetLastError());
    return USE_OK;
}
int use_op_attention_bwd(const float* q, const float* k, const float* v, const float* dO, float* work, float* dq, float* dk, float* dv, int B, int N,
                         int C, use_stream_t stream) {
    if (!q || !k || !v || !dO || !work || !dq || !dk || !dv || B < 1 || N < 1 || C < 1) return fail(USE_E_INVALID, "use_op_attention_bwd: bad argument");
    if ((size_t)(2 * N + 2 * C) * 4 > 60000) return fail(USE_E_INVALID, "use_op_attention_bwd: N + C too large for one row in LDS");
    launch_attention_bwd(q, k, v, dO, work, dq, dk, dv, B, N, C, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return USE_OK;
}
int use_op_dense_bwd(const float* g, const float* temb, const float* Wd, int B, int K, int Cout, float* dW, float* db, float* dtemb, use_stream_t stream) {
    if (!g || !temb || !Wd || !dW || !db || !dtemb) return fail(USE_E_INVALID, "use_op_dense_bwd: null tensor");
    if (B < 1 || K < 1 || Cout < 1) return fail(USE_E_INVALID, "use_op_dense_bwd: bad argument (B, K and Cout must be at least 1)");
    launch_dense_bwd(g, temb, Wd, B, K, Cout, dW, db, dtemb, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return USE_OK;
}

int use_trace_count(use_handle* h) {
    if (!h) return fail(USE_E_INVALID, "null handle");
    return h->plan ? (int)h->plan->trace.size() : 0;
}
int use_trace_entry_get(use_handle* h, int index, use_trace_entry* out) {
    if (!h || !out) return fail(USE_E_INVALID, "null argument");
    if (!h->plan || index < 0 || index >= (int)h->plan->trace.size()) return fail(USE_E_INVALID, "no trace entry %d", index);
    *out = h->plan->trace[(size_t)index];
    return USE_OK;
}

int use_sampler_trace_count(use_handle* h) {
    if (!h) return fail(USE_E_INVALID, "null handle");
    return h->plan && h->plan->strace_cur >= 0 ? (int)h->plan->strace[h->plan->strace_cur].size() : 0;
}
int use_sampler_trace_get(use_handle* h, int index, use_sampler_trace_entry* out) {
    if (!h || !out) return fail(USE_E_INVALID, "null argument");
    if (index < 0 || index >= use_sampler_trace_count(h)) return fail(USE_E_INVALID, "no sampler trace entry %d", index);
    *out = h->plan->strace[h->plan->strace_cur][(size_t)index];
    return USE_OK;
}

int use_debug_tensor(use_handle* h, const char* name, void** dev_ptr, int* dims4, int* dtype) {
    if (!h || !name) return fail(USE_E_INVALID, "null argument");
    if (!h->plan) return fail(USE_E_INVALID, "no debug tensor '%s'", name);
    const Plan& pl = *h->plan;
    auto it = pl.debug.find(name);
    if (it == pl.debug.end()) return fail(USE_E_INVALID, "no debug tensor '%s'", name);
    if (dev_ptr) *dev_ptr = it->second.p;
    if (dims4) { dims4[0] = pl.debug_B; dims4[1] = it->second.H; dims4[2] = it->second.W; dims4[3] = it->second.C; }
    if (dtype) *dtype = it->second.dtype;
    return USE_OK;
}

}  // extern "C"
