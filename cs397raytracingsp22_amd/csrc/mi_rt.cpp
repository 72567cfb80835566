// mi_rt.cpp — host runtime behind the C ABI of include/mi_rt.h (libmi_rt.so).
//
//   * scene upload: the scene compiler's output (scene_compile.cpp) committed to the device.
//   * render entry points: whole image on one GPU (mi_render) and the device-pointer
//     building blocks used with one process per GPU (tiles, un-permute, tone-map).
//
// There is no CPU implementation of the render path in this library: every entry
// point that produces pixels launches HIP kernels and reports an error when it cannot.
// Compiled with hipcc, -ffp-contract=off: the values hoisted out of the per-ray code
// (e1, e2, r*r, normalize(e1 x e2), -1/density, albedo/PI, the triangle tangent, the
// camera basis) are computed here with the same f32 operations, in the same order,
// the reference performs per ray, so hoisting them does not change a single bit.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <thread>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi_rt.h"
#include "pt_device.h"
#include "render_plan.hpp"

#pragma clang fp contract(off)

namespace pt {
hipError_t launch_megakernel(const K1Args& args, uint32_t n_blocks, bool lds, bool sig, size_t lds_bytes, hipStream_t stream);
hipError_t launch_megakernel_voted(const K1Args& args, uint32_t n_blocks, bool lds, bool sig, bool diag, bool gv,
                                   size_t lds_bytes, hipStream_t stream);
hipError_t launch_wf_main(const WfArgs& a, uint32_t n_blocks, bool sig, bool gv, bool tex, hipStream_t stream);
hipError_t launch_phong(const K1Args& a, uint32_t n_blocks, bool sig, hipStream_t stream);
hipError_t launch_branch(const K1Args& a, uint32_t n_blocks, uint32_t path_samples, bool sig, hipStream_t stream);
hipError_t launch_rq_intersect(const RqArgs& a, bool lds, bool gv, bool resolve, size_t lds_bytes, int n_cus, hipStream_t stream);
hipError_t launch_rq_occluded(const RqOccArgs& a, bool lds, bool gv, size_t lds_bytes, int n_cus, hipStream_t stream);
hipError_t launch_rq_hemi(const RqHemiArgs& a, bool lds, bool gv, size_t lds_bytes, int n_cus, hipStream_t stream);
hipError_t launch_rq_shade(const RqShadeArgs& a, hipStream_t stream);
hipError_t launch_walker(const WfArgs& a, const WalkerPlan& p, uint32_t n_blocks, bool* big_lds_enabled, hipStream_t stream);
hipError_t launch_wf_filter_f(const WfArgs& a, uint32_t blocks_per_shard, hipStream_t stream);
hipError_t launch_wf_trav_f(const WfArgs& a, uint32_t n_blocks, hipStream_t stream);
hipError_t launch_wf_replay(const WfArgs& a, uint32_t n_blocks, hipStream_t stream);
hipError_t launch_wf_prefix(uint32_t* out_count, uint32_t* trav_count, uint32_t* in_count, uint32_t* in_blkpfx,
                            uint32_t* trav_pfx, uint32_t* hdr, uint32_t* host_hdr, uint32_t seq, hipStream_t stream);
hipError_t launch_wf_reduce(const WfArgs& a, bool first_batch, bool last_batch, hipStream_t stream);
hipError_t launch_wf_reduce_sh(const WfArgs& a, bool first_batch, bool last_batch, hipStream_t stream);
hipError_t launch_unpermute(const float* gathered, float* image, uint32_t width, uint32_t height, uint32_t tiles_x,
                            uint32_t world, uint32_t tiles_padded, hipStream_t stream);
hipError_t launch_sig_unpermute(const uint32_t* gathered, uint32_t* image, uint32_t width, uint32_t height,
                                uint32_t tiles_x, uint32_t world, uint32_t tiles_padded, hipStream_t stream);
hipError_t launch_sh_unpermute(const float* gathered, float* image, uint32_t width, uint32_t height, uint32_t tiles_x,
                               uint32_t world, uint32_t tiles_padded, hipStream_t stream);
hipError_t launch_tonemap(const float* image, uint8_t* out, uint32_t n_pixels, float inv_gamma, hipStream_t stream);
hipError_t launch_selftest_rcp(unsigned long long* d_mismatches, hipStream_t stream);
hipError_t launch_lm_count(const LmArgs& a, hipStream_t stream);
hipError_t launch_lm_resolve(const LmArgs& a, hipStream_t stream);
hipError_t launch_lmf_mask(const LmfArgs& a, bool sh, hipStream_t stream);
hipError_t launch_lmf_atrous(const LmfArgs& a, bool lds, bool* big_lds_enabled, hipStream_t stream);
hipError_t launch_lmf_dilate(const LmfArgs& a, bool sh, hipStream_t stream);
hipError_t launch_pv_prepare(const PvArgs& a, hipStream_t stream);
hipError_t launch_pv_sample(const PvArgs& a, hipStream_t stream);
hipError_t launch_wf_reduce_m2(const WfArgs& a, bool first_batch, bool last_batch, hipStream_t stream);
hipError_t launch_lmv_init(const LmvArgs& a, const uint32_t* counts, bool few_inf, hipStream_t stream);
hipError_t launch_lmv_blur(const LmvArgs& a, hipStream_t stream);
hipError_t launch_lmv_atrous(const LmvArgs& a, hipStream_t stream);
hipError_t launch_lma_select(const LmaArgs& a, hipStream_t stream);
hipError_t launch_lma_gather(const LmaListArgs& a, hipStream_t stream);
hipError_t launch_lma_merge(const LmaListArgs& a, hipStream_t stream);
hipError_t launch_wf_reduce_psh(const WfArgs& a, bool first_batch, bool last_batch, hipStream_t stream);
hipError_t launch_lsh_atrous(const LmfArgs& a, hipStream_t stream);
hipError_t launch_lsh_eval(const LshEvalArgs& a, hipStream_t stream);
hipError_t launch_lookup(const LmlArgs& a, uint32_t format, uint32_t channels, hipStream_t stream);
hipError_t launch_lookup(const LmlLodArgs& a, uint32_t format, uint32_t channels, hipStream_t stream);
hipError_t launch_lmm_reduce(const LmmArgs& a, uint32_t channels, hipStream_t stream);
hipError_t launch_lmp_pack(const LmpArgs& a, uint32_t format, bool unpack, hipStream_t stream);
hipError_t launch_lmb_encode(const LmbArgs& a, bool lane_per_block, hipStream_t stream);
hipError_t launch_lmb_decode(const LmbArgs& a, hipStream_t stream);
}  // namespace pt

using namespace pt;

// ------------------------------------------------------------------ errors
static thread_local std::string g_err;
int pt::fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    g_err = buf;
    return code;
}
#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return fail(MI_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
#define MI_TRY(expr)                                                                           \
    do {                                                                                       \
        const int rc_ = (expr);                                                                \
        if (rc_ != MI_OK) return rc_;                                                          \
    } while (0)

// the kernels' seed_key of a caller's seed: lowbias32(seed ^ 0x68e31da4)
static uint32_t seed_key(uint32_t x) {
    x ^= 0x68e31da4u; x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x;
}

// ------------------------------------------------------------------ context
struct mi_ctx {
    int device = 0;
    hipStream_t stream = nullptr;            // own stream for mi_render
    hipStream_t aux_stream = nullptr;        // wavefront pipeline: the class-A part of a pass runs here, beside the walkers of the previous pass
    hipStream_t aux2_stream = nullptr;       // ... and wf_trav_f here, beside wf_trav (scenes with meshes of both kinds)
    hipEvent_t ev_pfx = nullptr, ev_part = nullptr, ev_travf = nullptr;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    bool ev_recorded = false;
    bool ms_summed = false; float ms_sum = 0.0f;             // the host-pointer ray queries run one kernel per chunk: mi_last_kernel_ms reports their sum

    // device scene: the blob, its pools (S), and the compiler's tables for the host side of a render (scene.image is emptied once copied)
    void* blob = nullptr; size_t blob_bytes = 0;
    const uint32_t* d_fin = nullptr;         // inside the blob's allocation, behind the image: WfArgs.fin (flags, then the may-emit bit of every Scene.objects entry)
    DScene S{};
    CompiledScene scene;
    bool have_scene = false;
    void* d_cand = nullptr; size_t cand_bytes = 0;           // two-stage candidates [cap][kCandMax] {t, key}
    void* d_cand_hdr = nullptr; size_t cand_hdr_bytes = 0;   // [cap] {pos, count | flags}

    // scratch for mi_render
    float* d_compact = nullptr; size_t compact_bytes = 0;
    float* d_image = nullptr;   size_t image_bytes = 0;
    uint8_t* d_u8 = nullptr;    size_t u8_bytes = 0;
    uint32_t* d_sigc = nullptr; size_t sigc_bytes = 0;
    uint32_t* d_sigi = nullptr; size_t sigi_bytes = 0;
    unsigned long long* d_diag = nullptr;    // 16 counters of the diagnostic variant
    void* d_rq = nullptr; size_t rq_bytes = 0;               // ray queries, host-pointer forms: rays and results of one chunk (its own buffer: never the pipeline's)
    void* d_rays = nullptr; size_t rays_bytes = 0;           // mi_render_rays / mi_render_points: the uploaded table, origins then dirs / points then normals (its own buffer too)
    void* d_sh = nullptr; size_t sh_bytes = 0;               // mi_render_probes / mi_render_points_sh: the compact SH records, then the un-permuted [H][W][9][3] plane
    // mi_lightmap_texels: the bins' counters and offsets, the bins' list (grown on demand, never the buffers mi_reserve sized), the pinned
    // word lm_scan leaves the list's full length in, and mi_lightmap_texels' / mi_bake_lightmap's uploaded mesh and triangle plane
    void* d_lm_hdr = nullptr; size_t lm_hdr_bytes = 0;
    void* d_lm_list = nullptr; size_t lm_list_bytes = 0;
    unsigned long long* h_lm_total = nullptr; unsigned long long* h_lm_total_dev = nullptr;
    void* d_lm_mesh = nullptr; size_t lm_mesh_bytes = 0;
    void* d_lm_out = nullptr; size_t lm_out_bytes = 0;
    // mi_lightmap_finish: two ping-pong images and two masks (grown on demand, never the buffers mi_reserve sized); lmf_atrous' > 64 KB
    // dynamic-LDS opt-in on THIS context's device
    void* d_lmf = nullptr; size_t lmf_bytes = 0;
    bool lmf_big_lds_enabled = false;
    // mi_lightmap_finish_sh: the same for [H][W][9][3] records
    void* d_lsh = nullptr; size_t lsh_bytes = 0;
    // mi_lightmap_mips_device without out_coverage: the coverage planes of levels 1 .. L - 1 (grown on demand)
    void* d_lmm = nullptr; size_t lmm_bytes = 0;
    // the host forms of the lightmap post-process calls (finish, finish_sh, sh_eval, finish_var, finish_var_counts, select, gather, merge):
    // the uploaded columns and the results of ONE call (staged; every such call synchronises before it returns)
    void* d_io = nullptr; size_t io_bytes = 0;
    // mi_probe_volume_sample: the prepared 112-byte probe records and, behind them, the host form's uploaded sh and valid (grown on
    // demand, never the buffers mi_reserve sized)
    void* d_pv = nullptr; size_t pv_bytes = 0;
    // mi_render_points_moments / mi_bake_lightmap_moments: the compact second-moment records, then the un-permuted [H][W][3] plane;
    // mi_lightmap_finish_var: two variance planes and the colour weight's denominators (all grown on demand, never the buffers
    // mi_reserve sized)
    void* d_m2 = nullptr; size_t m2_bytes = 0;
    void* d_lmv = nullptr; size_t lmv_bytes = 0;
    // mi_lightmap_select: the variance plane, the flags, the block counts and offsets;
    // mi_bake_lightmap_adaptive: the running planes with the centre table, the list with its length, and a round's compact tables and
    // results (all grown on demand, never the buffers mi_reserve sized)
    void* d_lma = nullptr; size_t lma_bytes = 0;
    void* d_lma_bake = nullptr; size_t lma_bake_bytes = 0;
    void* d_lma_list = nullptr; size_t lma_list_bytes = 0;
    void* d_lma_round = nullptr; size_t lma_round_bytes = 0;
    hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;     // mi_render's whole-call timer
    bool big_lds_enabled = false;                    // wf_trav_i<1024>'s > 64 KB dynamic-LDS opt-in, set on THIS context's device
    // wavefront pipeline buffers
    void* d_wf_a = nullptr; size_t wf_a_bytes = 0;   // path state ping
    void* d_wf_b = nullptr; size_t wf_b_bytes = 0;   // path state pong
    void* d_wf_samp = nullptr; size_t wf_samp_bytes = 0;
    void* d_wf_acc = nullptr; size_t wf_acc_bytes = 0;
    uint32_t* d_wf_cnt = nullptr;
    uint32_t* h_hdr = nullptr;                       // pinned + device-mapped ring of kHdrRing header slots (pt_device.h kHdr*), written by wf_prefix
    uint64_t wf_counts[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };   // last frame: passes, class-A paths streamed, class-B paths, queue entries, samples, pixels
    uint32_t* h_hdr_dev = nullptr;                   // its device-side address
    uint32_t hdr_seq = 0;
    // the primary-ray tile masks (render_plan.cpp tile_masks) of the last camera and their device copy; an upload invalidates them
    struct MaskCache {
        bool valid = false, applies = false;
        mi_camera_desc cam{}; uint32_t stride = 0, flags = 0;
        std::vector<uint64_t> words;
        void* d_words = nullptr; size_t d_bytes = 0;
    } masks;
    std::vector<hipEvent_t> wf_ev;                   // event pool for per-kernel timing of the pipeline
    float wf_ms[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };     // last frame: wf_main, wf_trav, wf_reduce totals (ms), launches, wf_trav_f, wf_replay, class A, wf_reduce_sh / wf_reduce_m2 / wf_reduce_psh
    int n_cus = 256;
    // Developer knobs (MI_RT_* environment variables), read ONCE in mi_ctx_create; none is needed for
    // normal operation and none changes a result — what a caller may want to control is in mi_render_opts.
    struct Tuning {
        uint32_t vote_t = 2, vote_a = 1, k_steps = 8;   // voted megakernel
        uint32_t lds_pad = 0;                           // occupancy experiments
        uint32_t refill_min = 16;                       // wf_trav: refill idle lanes when at least this many are idle (A/B round 2: 32 / 16 / 8 -> 36.9 / 35.8 / 38.6 ms on cfg2)
        int trav_lds = -1;                              // reference-tree walker override, a WalkerPlan form (-1 = automatic)
        int trav_bpc = 0;                               // its blocks per CU override (0 = automatic)
        int kernel_timing = -1;                         // per-launch HIP events: -1 = single-rank renders only
        bool global_bvh = false;                        // never stage a BVH in LDS
        bool wf_stamps = false;                         // -DPT_WF_STAMPS builds: collect wf_main phase stamps
        bool debug_mask = false;                        // print tile-mask statistics
        bool dump_launches = false;                     // print every pipeline launch's duration (needs per-launch events)
        ScheduleKnobs sched;                            // the pass schedule's knobs (render_plan.hpp)
        uint32_t lmf_lds_max_step = 1;                  // lmf_atrous: stage the tile and its halo in LDS up to this step, read HBM directly above (measured: DESIGN.md "Lightmap finishing")
        uint32_t lmm_levels_per_launch = kMipFuse;      // lmm_reduce: levels written per launch; 1 is the unfused form (measured: DESIGN.md "Lightmap mips")
        uint32_t lmb_lane_per_block = 1;                // the BC6H encoder: 1 is lmb_encode_block (one lane per block, 1.3 - 1.65 x faster), 0 lmb_encode (one lane per texel); the same bytes (measured: DESIGN.md "BC6H lightmaps")
        uint32_t spin_timeout_ms = 120000;              // header wait: give up after this long without progress
    } tune;
};

static int ensure(void** p, size_t* have, size_t want) {
    if (*have >= want && *p) return MI_OK;
    if (*p) { (void)hipFree(*p); *p = nullptr; *have = 0; }
    hipError_t e = hipMalloc(p, want);
    if (e != hipSuccess) return fail(MI_ERR_OOM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    *have = want;
    return MI_OK;
}

// Is the whole BVH (nodes + triangles) staged in LDS (the K1 megakernels, the ray queries)?  Sets the counts `a` carries (0: walk global memory).
template <class A> static bool stage_in_lds(const mi_ctx* c, A& a) {
    const bool lds = c->S.n_meshes > 0 && c->scene.lds_bytes <= 64u * 1024u && !c->tune.global_bvh;
    a.lds_nodes = lds ? (uint32_t)c->S.n_nodes : 0u; a.lds_tris = lds ? (uint32_t)c->S.n_tris : 0u;
    return lds;
}

extern "C" int mi_abi_version(void) { return MI_RT_ABI_VERSION; }
extern "C" const char* mi_last_error(void) { return g_err.c_str(); }

extern "C" void mi_ctx_destroy(mi_ctx* c);

// The wavefront pipeline's counter buffer (d_wf_cnt), in words.  wf_main appends per (class, shard) into out_count (class A
// shards, then class B shards) and counts path segments in trav_count; trav_head holds the walkers' cursors.  wf_prefix turns
// them into the tables of the next pass (in_count, in_blkpfx, trav_pfx) and the device copy of the header, and re-zeroes the
// head [0, zeroed) after every pass; each table has 8 words of slack.
namespace wfcnt {
constexpr size_t S = (size_t)kWfShards;
constexpr size_t out_count = 0, trav_count = 2 * S, trav_head = 3 * S, zeroed = 3 * S + 8;
constexpr size_t in_count = zeroed, in_blkpfx = in_count + 2 * S, trav_pfx = in_blkpfx + 2 * S + 8, hdr = trav_pfx + S + 8;
constexpr size_t words = hdr + 8;
}  // namespace wfcnt
static const int kHdrRing = 16;        // pinned header slots (wf_prefix -> host), one per pass in flight

static int ctx_init(mi_ctx* c, const hipDeviceProp_t& prop) {
    HIP_TRY(hipStreamCreate(&c->stream));
    HIP_TRY(hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&c->ev_pfx, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&c->ev_part, hipEventDisableTiming));
    HIP_TRY(hipStreamCreateWithFlags(&c->aux2_stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&c->ev_travf, hipEventDisableTiming));
    HIP_TRY(hipEventCreate(&c->ev_start));
    HIP_TRY(hipEventCreate(&c->ev_stop));
    HIP_TRY(hipEventCreate(&c->ev_t0));
    HIP_TRY(hipEventCreate(&c->ev_t1));
    HIP_TRY(hipMalloc((void**)&c->d_diag, 16 * sizeof(unsigned long long)));
    c->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    HIP_TRY(hipMalloc((void**)&c->d_wf_cnt, wfcnt::words * sizeof(uint32_t)));
    HIP_TRY(hipHostMalloc((void**)&c->h_hdr, kHdrRing * kHdrSlotWords * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent));
    memset(c->h_hdr, 0, kHdrRing * kHdrSlotWords * sizeof(uint32_t));
    HIP_TRY(hipHostGetDevicePointer((void**)&c->h_hdr_dev, c->h_hdr, 0));
    // developer knobs: read here, once (never on the render path)
    mi_ctx::Tuning& t = c->tune;
    auto env_u = [](const char* name, uint32_t& v) { if (const char* e = getenv(name)) v = (uint32_t)atoi(e); };
    auto env_i = [](const char* name, int& v) { if (const char* e = getenv(name)) v = atoi(e); };
    env_u("MI_RT_VOTE_T", t.vote_t); env_u("MI_RT_VOTE_A", t.vote_a); env_u("MI_RT_KSTEPS", t.k_steps);
    if (const char* e = getenv("MI_RT_LDS_PAD_KB")) t.lds_pad = (uint32_t)atoi(e) * 1024u;
    env_u("MI_RT_WF_REFILL", t.refill_min);
    env_u("MI_RT_WF_FUSE_MAX", t.sched.fuse_max); env_u("MI_RT_WF_FUSE_MIN", t.sched.fuse_min);
    env_i("MI_RT_WF_SPLIT", t.sched.split); env_u("MI_RT_WF_NOWAIT_BLOCKS", t.sched.nowait_blocks); env_u("MI_RT_WF_TAIL_PATHS", t.sched.tail_paths);
    env_i("MI_RT_WF_CONC", t.sched.conc); env_i("MI_RT_WF_CONC_TRAV_BPC", t.sched.conc_trav_bpc); env_i("MI_RT_WF_CONC_TRAVF_BPC", t.sched.conc_travf_bpc);
    env_i("MI_RT_WF_TRAV_LDS", t.trav_lds); env_i("MI_RT_WF_TRAV_BPC", t.trav_bpc); env_i("MI_RT_WF_TRAVF_BPC", t.sched.travf_bpc); env_i("MI_RT_WF_KERNEL_TIMING", t.kernel_timing);
    t.global_bvh = getenv("MI_RT_GLOBAL_BVH") != nullptr;
    t.wf_stamps = getenv("MI_RT_WF_STAMPS") != nullptr;
    t.debug_mask = getenv("MI_RT_DEBUG_MASK") != nullptr;
    t.dump_launches = getenv("MI_RT_WF_DUMP_LAUNCHES") != nullptr;
    env_u("MI_RT_SPIN_TIMEOUT_MS", t.spin_timeout_ms);
    env_u("MI_RT_LMF_LDS_MAX_STEP", t.lmf_lds_max_step);
    env_u("MI_RT_LMM_LEVELS_PER_LAUNCH", t.lmm_levels_per_launch);
    env_u("MI_RT_LMB_LANE_PER_BLOCK", t.lmb_lane_per_block);
    t.lmm_levels_per_launch = std::min(std::max(t.lmm_levels_per_launch, 1u), kMipFuse);
    if (t.lmf_lds_max_step > kLmfMaxLdsStep) t.lmf_lds_max_step = kLmfMaxLdsStep;
    if (t.vote_t < 1) t.vote_t = 1;
    if (t.k_steps < 1) t.k_steps = 1;
    if (t.refill_min < 1) t.refill_min = 1;
    if (t.refill_min > 64) t.refill_min = 64;
    return MI_OK;
}

extern "C" int mi_ctx_create(int device, mi_ctx** out) {
    if (!out) return fail(MI_ERR_INVALID, "mi_ctx_create: out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(MI_ERR_NO_DEVICE, "no HIP device available (%s); the render path has no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(MI_ERR_INVALID, "device %d out of range (have %d)", device, n);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(MI_ERR_NO_DEVICE, "device %d is %s; this library carries gfx950 (MI355X) code only", device, prop.gcnArchName);
    mi_ctx* c = new mi_ctx();
    c->device = device;
    const int rc = ctx_init(c, prop);
    if (rc != MI_OK) {                 // release whatever was created (the message of the failure is kept)
        const std::string msg = g_err;
        mi_ctx_destroy(c);
        g_err = msg;
        return rc;
    }
    *out = c;
    return MI_OK;
}

extern "C" void mi_ctx_destroy(mi_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    if (c->blob) (void)hipFree(c->blob);
    if (c->d_compact) (void)hipFree(c->d_compact);
    if (c->d_image) (void)hipFree(c->d_image);
    if (c->d_u8) (void)hipFree(c->d_u8);
    if (c->d_sigc) (void)hipFree(c->d_sigc);
    if (c->d_sigi) (void)hipFree(c->d_sigi);
    if (c->d_diag) (void)hipFree(c->d_diag);
    if (c->d_rq) (void)hipFree(c->d_rq);
    if (c->d_rays) (void)hipFree(c->d_rays);
    if (c->d_sh) (void)hipFree(c->d_sh);
    if (c->d_lsh) (void)hipFree(c->d_lsh);
    if (c->d_lmm) (void)hipFree(c->d_lmm);
    if (c->d_lm_hdr) (void)hipFree(c->d_lm_hdr);
    if (c->d_lm_list) (void)hipFree(c->d_lm_list);
    if (c->h_lm_total) (void)hipHostFree(c->h_lm_total);
    if (c->d_lm_mesh) (void)hipFree(c->d_lm_mesh);
    if (c->d_lm_out) (void)hipFree(c->d_lm_out);
    if (c->d_lmf) (void)hipFree(c->d_lmf);
    if (c->d_io) (void)hipFree(c->d_io);
    if (c->d_pv) (void)hipFree(c->d_pv);
    if (c->d_m2) (void)hipFree(c->d_m2);
    if (c->d_lmv) (void)hipFree(c->d_lmv);
    if (c->d_lma) (void)hipFree(c->d_lma);
    if (c->d_lma_bake) (void)hipFree(c->d_lma_bake);
    if (c->d_lma_list) (void)hipFree(c->d_lma_list);
    if (c->d_lma_round) (void)hipFree(c->d_lma_round);
    if (c->d_wf_a) (void)hipFree(c->d_wf_a);
    if (c->d_wf_b) (void)hipFree(c->d_wf_b);
    if (c->d_wf_samp) (void)hipFree(c->d_wf_samp);
    if (c->d_wf_acc) (void)hipFree(c->d_wf_acc);
    if (c->d_cand) (void)hipFree(c->d_cand);
    if (c->d_cand_hdr) (void)hipFree(c->d_cand_hdr);
    if (c->masks.d_words) (void)hipFree(c->masks.d_words);
    if (c->d_wf_cnt) (void)hipFree(c->d_wf_cnt);
    if (c->h_hdr) (void)hipHostFree(c->h_hdr);
    for (hipEvent_t e : c->wf_ev) (void)hipEventDestroy(e);
    if (c->ev_start) (void)hipEventDestroy(c->ev_start);
    if (c->ev_stop) (void)hipEventDestroy(c->ev_stop);
    if (c->ev_t0) (void)hipEventDestroy(c->ev_t0);
    if (c->ev_t1) (void)hipEventDestroy(c->ev_t1);
    if (c->ev_pfx) (void)hipEventDestroy(c->ev_pfx);
    if (c->ev_part) (void)hipEventDestroy(c->ev_part);
    if (c->aux_stream) (void)hipStreamDestroy(c->aux_stream);
    if (c->ev_travf) (void)hipEventDestroy(c->ev_travf);
    if (c->aux2_stream) (void)hipStreamDestroy(c->aux2_stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// ------------------------------------------------------------------ scene upload
// Validate and compile on the host (no device state is touched: a failure there leaves the previous scene as it was), then commit.
// The commit frees the old blob first, so that the peak HBM is one scene; a failure from there on leaves the context with no scene.
extern "C" int mi_scene_upload(mi_ctx* c, const mi_scene_desc* d) {
    if (!c || !d) return fail(MI_ERR_INVALID, "mi_scene_upload: NULL argument");
    CompiledScene sc;
    const int rc = compile_scene(d, &sc);
    if (rc != MI_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (c->blob) (void)hipFree(c->blob);
    c->blob = nullptr; c->blob_bytes = 0; c->d_fin = nullptr; c->S = DScene{}; c->scene = CompiledScene(); c->have_scene = false;
    c->masks.valid = false;
    const size_t total = sc.image.size();
    // behind the image, in the same allocation: the table of wf_main's final-segment cull (WfArgs.fin; not part of the blob)
    std::vector<uint32_t> fin(1, sc.emit.any_mesh ? (uint32_t)kFinMeshEmit : 0u);
    fin.insert(fin.end(), sc.emit.object_bits.begin(), sc.emit.object_bits.end());
    const size_t fin_off = (total + 255) & ~(size_t)255, fin_bytes = fin.size() * sizeof(uint32_t);
    void* blob = nullptr;
    hipError_t e = hipMalloc(&blob, fin_off + fin_bytes);
    if (e != hipSuccess) return fail(MI_ERR_OOM, "hipMalloc(%zu) for the scene failed: %s", fin_off + fin_bytes, hipGetErrorString(e));
    c->blob = blob; c->blob_bytes = total;
    c->d_fin = (const uint32_t*)((const uint8_t*)blob + fin_off);
    HIP_TRY(hipMemcpy(c->blob, sc.image.data(), total, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy((uint8_t*)c->blob + fin_off, fin.data(), fin_bytes, hipMemcpyHostToDevice));
    sc.image = std::vector<uint8_t>();
    c->S = sc.device_scene(c->blob);
    c->scene = std::move(sc);
    c->have_scene = true;
    return MI_OK;
}

// ------------------------------------------------------------------ render
extern "C" int mi_compact_size(const mi_camera_desc* cam, int32_t world, uint32_t* tiles_total, uint32_t* tiles_padded) {
    if (!cam || world < 1 || !tiles_total || !tiles_padded) return fail(MI_ERR_INVALID, "mi_compact_size: bad argument");
    const TileGrid g = tile_grid(cam, world);
    *tiles_total = g.total; *tiles_padded = g.padded;
    return MI_OK;
}

// K1w: the wavefront pipeline (pt_kernels.hip).  The host enqueues one iteration per path segment:
// wf_main, wf_prefix (device-side bookkeeping of the shard counters), wf_trav.  It needs one number back
// per iteration — the grid of the next wf_main — which arrives on a second stream while wf_trav runs, so
// the compute stream never waits for the host; the call still returns only when the frame is done.
// Memory and batch size (wf_first_batch, wf_batch) and every scheduling decision (pass_schedule, pass_gate, plan_pass): render_plan.cpp.

// Allocates the buffers of a batch of s_batch samples (a.npix set), halving the batch while an allocation fails.
static int wf_alloc(mi_ctx* c, WfArgs& a, bool two_stage, uint32_t& s_batch) {
    for (;;) {
        const WfBatch b = wf_batch(a.npix, s_batch);
        a.region = b.region; a.cap = b.cap;
        int rc = ensure(&c->d_wf_a, &c->wf_a_bytes, b.state_bytes);
        if (rc == MI_OK) rc = ensure(&c->d_wf_b, &c->wf_b_bytes, b.state_bytes);
        if (rc == MI_OK) rc = ensure(&c->d_wf_samp, &c->wf_samp_bytes, b.samp_bytes);
        if (rc == MI_OK) rc = ensure(&c->d_wf_acc, &c->wf_acc_bytes, b.acc_bytes);
        if (rc == MI_OK && two_stage) rc = ensure(&c->d_cand, &c->cand_bytes, b.cand_bytes);
        if (rc == MI_OK && two_stage) rc = ensure(&c->d_cand_hdr, &c->cand_hdr_bytes, b.cand_hdr_bytes);
        if (rc == MI_OK) return MI_OK;
        if (rc != MI_ERR_OOM || s_batch == 1) return rc;
        (void)hipGetLastError();
        s_batch = (s_batch + 1) / 2;                                 // back off and retry with half the batch
    }
}

// Sizes and allocates the pipeline for `padded` tiles of this rank (host-side work: must happen BEFORE the timing start event is
// recorded).  The free HBM is asked for only when the caller gives no budget; what this context already holds for the pipeline
// can be reused.
static int wf_prepare(mi_ctx* c, uint32_t padded, uint32_t spp, uint64_t max_state_bytes, bool two_stage, WfArgs& a, uint32_t& s_batch) {
    memset(&a, 0, sizeof a);
    a.npix = padded * (uint32_t)kTilePixels;
    uint64_t free_bytes = 0;
    if (max_state_bytes == 0) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)8 << 30;
        free_bytes = free_b + c->wf_a_bytes + c->wf_b_bytes + c->wf_samp_bytes + c->cand_bytes + c->cand_hdr_bytes;
    }
    const int rc = wf_first_batch(a.npix, spp, max_state_bytes, free_bytes, two_stage, &s_batch);
    if (rc != MI_OK) return rc;
    return wf_alloc(c, a, two_stage, s_batch);
}

// The device copy of the tile masks for `cam` (nullptr: masking does not apply), computed and uploaded when the camera, the
// grid's row length or the flags differ from the cached ones.
static int device_tile_masks(mi_ctx* c, const mi_camera_desc* cam, uint32_t flags, uint32_t stride, hipStream_t stream,
                             const unsigned long long** out) {
    mi_ctx::MaskCache& m = c->masks;
    if (!m.valid || m.stride != stride || m.flags != flags || memcmp(&m.cam, cam, sizeof *cam) != 0) {
        m.valid = false;
        m.applies = tile_masks(c->scene, *cam, flags, stride, m.words);
        if (m.applies) {
            if (c->tune.debug_mask) {
                const int n_ts = c->scene.n_list_tri + c->scene.n_list_sphere, n_mesh = (int)c->scene.meshes.size();
                const size_t n_tiles = m.words.size() / 2;
                size_t bits = 0, mbits = 0, dead = 0;
                for (size_t t = 0; t < n_tiles; t++) {
                    bits += (size_t)__builtin_popcountll(m.words[t] & ((n_ts >= 64) ? ~0ull : ((1ull << n_ts) - 1ull)));
                    mbits += (size_t)__builtin_popcountll(m.words[n_tiles + t] & ((n_mesh >= 32) ? 0xffffffffull : ((1ull << n_mesh) - 1ull)));
                    dead += (size_t)(m.words[n_tiles + t] >> 63);
                }
                fprintf(stderr, "[mi_rt] tile masks: %zu tiles, %.2f of %d list entries and %.2f of %d meshes kept per tile, %zu dead tiles\n",
                        n_tiles, (double)bits / (double)n_tiles, n_ts, (double)mbits / (double)n_tiles, n_mesh, dead);
            }
            const size_t bytes = m.words.size() * sizeof(uint64_t);
            const int rc = ensure(&m.d_words, &m.d_bytes, bytes);
            if (rc != MI_OK) return rc;
            HIP_TRY(hipMemcpyAsync(m.d_words, m.words.data(), bytes, hipMemcpyHostToDevice, stream));
        }
        m.cam = *cam; m.stride = stride; m.flags = flags; m.valid = true;
    }
    *out = m.applies ? (const unsigned long long*)m.d_words : nullptr;
    return MI_OK;
}

// Headers: wf_prefix stores the header of every pass (pt_device.h kHdr*) into a RING of pinned host slots (slot = seq % kHdrRing),
// so the host may run a few passes ahead of the device and still read every header.
class HeaderRing {
public:
    HeaderRing(const mi_ctx* c, hipStream_t stream) : h_((const volatile uint32_t*)c->h_hdr), stream_(stream), timeout_ms_(c->tune.spin_timeout_ms) {}
    static size_t slot(uint32_t seq) { return (size_t)(seq % kHdrRing) * kHdrSlotWords; }
    bool ready(uint32_t seq) const { return h_[slot(seq) + kHdrSeq] == seq; }
    PassHdr read(uint32_t seq) const {          // (it has arrived)
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        const volatile uint32_t* h = h_ + slot(seq);
        PassHdr r = { h[kHdrBlocks], h[kHdrLive], h[kHdrQueue], h[kHdrLiveB], h[kHdrBlocksA], h[kHdrSegments] };
        return r;
    }
    int wait(uint32_t seq) const {
        const auto t_wait = std::chrono::steady_clock::now();
        for (uint32_t spin = 1; !ready(seq); spin++) {
            if ((spin & 63u) == 0) {
                hipError_t q = hipStreamQuery(stream_);
                if (q == hipSuccess) { if (ready(seq)) break; return fail(MI_ERR_HIP, "wavefront pipeline: stream drained without a header"); }
                if (q != hipErrorNotReady) return fail(MI_ERR_HIP, "wavefront pipeline: %s", hipGetErrorString(q));
                // a wedged stream neither drains nor errors: bound the wait by wall clock (one pass is milliseconds)
                const auto waited = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t_wait).count();
                if (waited > (long long)timeout_ms_)
                    return fail(MI_ERR_HIP, "wavefront pipeline: no header from the device after %lld ms (stream wedged?)", (long long)waited);
            }
            // the header of a small pass is there within tens of microseconds: poll without sleeping at first (a sleep
            // costs ~60 us whatever it asks for), then back off
            if (spin < 4096u && std::chrono::steady_clock::now() - t_wait < std::chrono::microseconds(150)) {
#if defined(__x86_64__)
                __builtin_ia32_pause();
#else
                std::this_thread::yield();
#endif
            } else std::this_thread::sleep_for(std::chrono::microseconds(20));
        }
        return MI_OK;
    }
private:
    const volatile uint32_t* h_;
    hipStream_t stream_;
    uint32_t timeout_ms_;
};

// Per-launch timing of the pipeline: one event pair per launch from the context's pool, summed per kind into wf_ms after the
// frame.  One pair is ~0.4 ms per frame of extra barriers: nothing on a whole frame (109 ms), 3 % of a 1/8 share, so multi-rank
// renders skip it unless asked (MI_RT_WF_KERNEL_TIMING=0/1 overrides).
enum LaunchKind { kMain, kTrav, kReduce, kTravF, kReplay, kMainA, kReduceSh, kReduceM2, kReducePsh };      // kTravF: wf_filter_f too; kMainA: wf_main's class-A part on the second stream
class LaunchTimer {
public:
    LaunchTimer(mi_ctx* c, bool on) : c_(c), on_(on) {}
    template <class Launch> int run(LaunchKind kind, hipStream_t on, Launch launch) {
        if (stamp(kind, on) != MI_OK) return fail(MI_ERR_HIP, "event");
        const hipError_t e = launch();
        if (e != hipSuccess) return fail(MI_ERR_HIP, "%s launch failed: %s", kNames[kind], hipGetErrorString(e));
        if (stamp(kind, on) != MI_OK) return fail(MI_ERR_HIP, "event");
        return MI_OK;
    }
    // after the frame (the streams have drained): wf_ms = {wf_main, wf_trav, wf_reduce} ms, launches, {wf_trav_f, wf_replay, class A, wf_reduce_sh} ms;
    // wf_reduce_m2 and wf_reduce_psh share entry 7 with wf_reduce_sh (no render runs two of them)
    void finish() {
        for (int k = 0; k < 8; k++) c_->wf_ms[k] = 0.0f;
        c_->wf_ms[3] = (float)(used_ / 2);
        for (size_t e = 0; e + 1 < used_; e += 2) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, c_->wf_ev[e], c_->wf_ev[e + 1]) == hipSuccess) c_->wf_ms[kinds_[e] < 3 ? kinds_[e] : kinds_[e] >= kReduceSh ? 7 : kinds_[e] + 1] += ms;
            if (c_->tune.dump_launches) fprintf(stderr, "[mi_rt] launch %zu %s %.4f ms\n", e / 2, kNames[kinds_[e]], ms);
        }
    }
private:
    static constexpr const char* kNames[9] = { "wf_main", "wf_trav", "wf_reduce", "wf_trav_f", "wf_replay", "wf_main (class A, beside the walkers)", "wf_reduce_sh",
                                               "wf_reduce_m2", "wf_reduce_psh" };
    int stamp(LaunchKind kind, hipStream_t on) {          // before AND after the launch
        if (!on_) return MI_OK;
        if (used_ == c_->wf_ev.size()) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return MI_ERR_HIP; c_->wf_ev.push_back(e); }
        if (hipEventRecord(c_->wf_ev[used_++], on) != hipSuccess) return MI_ERR_HIP;
        kinds_.push_back(kind);
        return MI_OK;
    }
    mi_ctx* c_;
    bool on_;
    size_t used_ = 0;
    std::vector<int> kinds_;
};

// Samples [begin, end) of every pixel, added in order to `accum` (nullptr = the context's own buffer).
// begin == 0 starts the sums from zero; end == aa_sample_count also writes the per-pixel means.
struct SampleRange { uint32_t begin, end; float4* accum; };
// Ray-table rendering: DEVICE arrays [rows][H][W][3] that replace Camera::generate_rays, rows = 1 or aa_sample_count
// Point-table rendering (points = true): `origins` holds surface points and `dirs` their normals, same layout; the camera pass draws
// the direction of each sample itself (the POINTS form of wf_main)
// Light probes (kind = kTableProbes): `origins` holds probe positions, `dirs` is nullptr; the camera pass draws a full-sphere direction (the
// PROBES form) and `sh`, DEVICE [tiles_padded][1024][27] or nullptr, takes the SH L2 sums (wf_reduce_sh)
// Directional lightmaps (kind = kTablePoints with `sh`): the SH L2 sums over the POINTS form's hemisphere directions (wf_reduce_psh)
// Second moments (point tables): `m2`, DEVICE [tiles_padded][1024][3] or nullptr, takes the sums of squares (wf_reduce_m2)
enum TableKind { kTableRays, kTablePoints, kTableProbes };
struct RayTable { const float* origins; const float* dirs; uint32_t rows; TableKind kind; float* sh; float* m2; };

static int render_tiles_wavefront(mi_ctx* c, const K1Args& k, const mi_camera_desc* cam, WfArgs a, uint32_t s_batch, uint32_t flags,
                                  float* d_compact, uint32_t* d_sig, SampleRange range, hipStream_t stream) {
    a.S = k.S; a.C = k.C; a.R = k.R; a.seed_key = k.seed_key;
    const uint32_t spp = cam->aa_sample_count;
    uint32_t* cnt = c->d_wf_cnt;
    a.out_count = cnt + wfcnt::out_count; a.trav_count = cnt + wfcnt::trav_count; a.trav_head = cnt + wfcnt::trav_head;
    a.in_count = cnt + wfcnt::in_count; a.in_blkpfx = cnt + wfcnt::in_blkpfx; a.trav_pfx = cnt + wfcnt::trav_pfx; a.hdr = cnt + wfcnt::hdr;
    a.samp = (float4*)c->d_wf_samp; a.accum = range.accum ? range.accum : (float4*)c->d_wf_acc;
    a.out = d_compact; a.sig = d_sig;
    // the tile masks are derived from the camera: a ray table renders without them, whatever the flags say
    if (a.ray_o || a.pt_p) a.tile_mask = nullptr;
    else MI_TRY(device_tile_masks(c, cam, flags, a.R.tiles_x, stream, &a.tile_mask));
    a.diag = nullptr;           // developer builds (-DPT_WF_STAMPS): phase stamps of wf_main
    if (c->tune.wf_stamps) { a.diag = c->d_diag; HIP_TRY(hipMemsetAsync(c->d_diag, 0, 16 * sizeof(unsigned long long), stream)); }
    a.refill_min = c->tune.refill_min;
    a.fin = (flags & MI_OPT_NO_FINAL_CULL) ? nullptr : c->d_fin;       // wf_main's final-segment cull (SIG = false forms)
    const WalkMasks masks = walk_masks(c->scene, flags);
    const WalkerPlan walker = plan_walker(c->scene, masks.ref, c->tune.trav_lds, c->tune.trav_bpc, c->tune.global_bvh);
    const PassSchedule sched = pass_schedule(c->scene, masks, walker, c->n_cus, cam->path_depth, c->tune.sched);
    a.R.lds_nodes = walker.lds_nodes; a.R.lds_tris = walker.lds_tris;
    a.cand = (uint2*)c->d_cand; a.cand_hdr = (uint2*)c->d_cand_hdr;
    float4* bufs[2] = { (float4*)c->d_wf_a, (float4*)c->d_wf_b };
    const bool sig = d_sig != nullptr, gv = c->scene.gen_volumes, tex = c->scene.mesh_maps;
    const hipStream_t aux = c->aux_stream, travf_stream = sched.side_by_side ? c->aux2_stream : stream;

    // one event pair per launch (LaunchTimer): single-rank renders only, unless asked
    LaunchTimer timer(c, c->tune.kernel_timing >= 0 ? c->tune.kernel_timing != 0 : a.R.world == 1);
    const HeaderRing ring(c, stream);

    uint64_t counts[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    counts[4] = (uint64_t)a.npix * (range.end - range.begin); counts[5] = a.npix;
    // samples of dead tiles (nothing reachable from the tile: no ray is generated, no slot written or read) — only without signatures
    if (a.tile_mask && !d_sig) counts[7] = dead_pixels(tile_grid(cam, a.R.world), cam, a.R.rank, a.R.world, c->masks.words) * (range.end - range.begin);
    for (uint32_t s0 = range.begin; s0 < range.end; s0 += s_batch) {
        a.s_base = s0; a.s_count = (s0 + s_batch <= range.end) ? s_batch : (range.end - s0);
        int cur = 0;
        a.iter0 = 1;
        a.n_in = a.npix * a.s_count;
        HIP_TRY(hipMemsetAsync(cnt, 0, wfcnt::zeroed * sizeof(uint32_t), stream));   // wf_prefix re-zeroes them after every pass
        const uint32_t seq0 = c->hdr_seq + 1u;          // seq of this batch's pass 0
        uint32_t seen = 0;                              // headers of passes [0, seen) have been read
        PassHdr last = camera_pass_header(a.n_in);
        bool all_dead = false;
        auto consume = [&](bool count_it) {             // read header `seen` (it has arrived)
            last = ring.read(seq0 + seen);
            seen++;
            if (count_it) { counts[0] += 1; counts[1] += last.live - last.live_b; counts[2] += last.live_b; counts[3] += last.queue; }
            counts[6] += last.segments;                 // every launched pass counts: a pass behind the one that ended every path ran no segment
            if (last.live == 0) all_dead = true;
        };
        uint32_t it = 0;
        for (; it <= cam->path_depth + 1u; it++) {
            while (seen < it && !all_dead && ring.ready(seq0 + seen)) consume(true);
            if (all_dead) break;
            const PassGate gate = pass_gate(sched, it, seen, last.live);
            if (gate == PassGate::kWait) {
                while (seen < it && !all_dead) { MI_TRY(ring.wait(seq0 + seen)); consume(true); }
                if (all_dead) break;
            }
            const PassPlan p = plan_pass(sched, it, gate != PassGate::kBound, last);
            if (p.stop) break;
            a.fuse_max = p.fuse_max; a.fuse_min = p.fuse_min;
            a.st_in = a.iter0 ? nullptr : bufs[cur]; a.st_out = bufs[cur ^ 1];
            a.n_blocks_in = p.grid_all;
            if (p.split) {                      // class A beside the previous pass' walkers, class B behind them
                HIP_TRY(hipStreamWaitEvent(aux, c->ev_pfx, 0));
                a.part = 1;
                MI_TRY(timer.run(kMainA, aux, [&] { return launch_wf_main(a, p.grid_a, sig, gv, tex, aux); }));     // its span includes waiting for CUs
                HIP_TRY(hipEventRecord(c->ev_part, aux));
                a.part = 2;
                MI_TRY(timer.run(kMain, stream, [&] { return launch_wf_main(a, p.grid_b, sig, gv, tex, stream); }));
                HIP_TRY(hipStreamWaitEvent(stream, c->ev_part, 0));
            } else {
                a.part = 0;
                MI_TRY(timer.run(kMain, stream, [&] { return launch_wf_main(a, p.grid_all, sig, gv, tex, stream); }));
            }
            // device-side bookkeeping: tables for the next pass and for wf_trav, and the header the host needs (grid of the
            // next pass, anything alive?), which wf_prefix stores straight into pinned host memory: the compute stream never
            // waits for the host
            const uint32_t seq = ++c->hdr_seq;
            HIP_TRY(launch_wf_prefix(cnt + wfcnt::out_count, cnt + wfcnt::trav_count, cnt + wfcnt::in_count, cnt + wfcnt::in_blkpfx, cnt + wfcnt::trav_pfx,
                                     cnt + wfcnt::hdr, c->h_hdr_dev + HeaderRing::slot(seq), seq, stream));
            if (sched.split_enabled) HIP_TRY(hipEventRecord(c->ev_pfx, stream));
            // persistent walkers; they leave at once when the queue is empty.  Successive launches merge their meshes' hits
            // into the hit record (strictly closer wins, ties go to the lower Scene.objects index: order-independent)
            if (sched.side_by_side) {           // wf_trav_f on its own stream, beside wf_trav
                HIP_TRY(hipEventRecord(c->ev_pfx, stream));
                HIP_TRY(hipStreamWaitEvent(travf_stream, c->ev_pfx, 0));
            }
            if (sched.ref_walk) {
                a.trav_mask = sched.ref_mask;
                MI_TRY(timer.run(kTrav, stream, [&] { return launch_walker(a, walker, sched.walker_blocks, &c->big_lds_enabled, stream); }));
            }
            if (sched.ts_mask) {
                a.trav_mask = sched.ts_mask;
                // wf_filter_f keeps the class-B paths whose ray enters a two-stage mesh's root box; wf_trav_f and wf_replay work on that list
                MI_TRY(timer.run(kTravF, travf_stream, [&] { return launch_wf_filter_f(a, sched.filter_blocks_per_shard, travf_stream); }));
                MI_TRY(timer.run(kTravF, travf_stream, [&] { return launch_wf_trav_f(a, sched.travf_blocks, travf_stream); }));
                if (sched.side_by_side) {
                    HIP_TRY(hipEventRecord(c->ev_travf, travf_stream));
                    HIP_TRY(hipStreamWaitEvent(stream, c->ev_travf, 0));
                }
                MI_TRY(timer.run(kReplay, stream, [&] { return launch_wf_replay(a, sched.replay_blocks, stream); }));
            }
            cur ^= 1;
            a.iter0 = 0;
            if (p.last) { it++; break; }
        }
        MI_TRY(timer.run(kReduce, stream, [&] { return launch_wf_reduce(a, s0 == 0, s0 + a.s_count >= spp, stream); }));
        // light probes: the SH sums of the same slots, same batch rules (the slots are rewritten by the next batch only, behind this)
        if (a.sh && a.pt_probes) MI_TRY(timer.run(kReduceSh, stream, [&] { return launch_wf_reduce_sh(a, s0 == 0, s0 + a.s_count >= spp, stream); }));
        // directional lightmaps: the same sums of a point table's samples, whose directions lie about the table's normals
        if (a.sh && !a.pt_probes) MI_TRY(timer.run(kReducePsh, stream, [&] { return launch_wf_reduce_psh(a, s0 == 0, s0 + a.s_count >= spp, stream); }));
        // second moments of a point-table bake: the sums of squares of the same slots, same batch rules
        if (a.m2) MI_TRY(timer.run(kReduceM2, stream, [&] { return launch_wf_reduce_m2(a, s0 == 0, s0 + a.s_count >= spp, stream); }));
        // the headers not read yet (statistics; passes launched behind the one that ended every path are not counted)
        const uint32_t launched = c->hdr_seq + 1u - seq0;
        while (seen < launched) { MI_TRY(ring.wait(seq0 + seen)); consume(!all_dead); }
    }
    HIP_TRY(hipStreamSynchronize(stream));
    for (int k = 0; k < 8; k++) c->wf_counts[k] = counts[k];
    timer.finish();
    return MI_OK;
}

// `table` (ray-table rendering): the caller's rays instead of Camera::generate_rays; `cam` then went through table_camera
static int render_tiles(mi_ctx* c, const mi_camera_desc* cam, const mi_render_opts* o, float* d_compact,
                        uint32_t* d_sig, hipStream_t stream, mi_stats* st, const SampleRange* partial = nullptr, const RayTable* table = nullptr) {
    int rc = table ? check_table_camera(cam, table->rows) : check_camera(cam);
    if (rc != MI_OK) return rc;
    if (!c->have_scene) return fail(MI_ERR_NO_SCENE, "no scene uploaded");
    if (!o || o->world < 1 || o->rank < 0 || o->rank >= o->world) return fail(MI_ERR_INVALID, "bad rank/world");
    if (table && o->variant != MI_VARIANT_DEFAULT && o->variant != MI_VARIANT_WAVEFRONT)
        return fail(MI_ERR_UNSUPPORTED, "ray-table rendering runs on the default (wavefront) variant only, not variant %d: use mi_shade_rays for the recursive estimator", o->variant);
    SampleRange range = { 0u, cam->aa_sample_count, nullptr };
    if (partial) {
        range = *partial;
        if (range.begin >= range.end || range.end > cam->aa_sample_count)
            return fail(MI_ERR_INVALID, "sample range [%u, %u) is not inside [0, %u)", range.begin, range.end, cam->aa_sample_count);
        if (!range.accum) return fail(MI_ERR_INVALID, "accumulator buffer is NULL");
        if (cam->shading_mode != MI_SHADE_PATHTRACE || cam->path_samples != 1 || (o->variant != MI_VARIANT_DEFAULT && o->variant != MI_VARIANT_WAVEFRONT))
            return fail(MI_ERR_UNSUPPORTED, "progressive rendering runs on the default (wavefront) path-tracing variant only");
    }
    const bool writes_image = range.end == cam->aa_sample_count;
    if (!d_compact && writes_image) return fail(MI_ERR_INVALID, "output buffer is NULL");
    K1Args a;
    a.S = c->S;
    if (o->flags & MI_OPT_NO_LIST_TREE) { a.S.top_meshf = -1; a.S.n_list_lin = a.S.n_list_tri; }      // every list Triangle one by one (cross-check)
    a.C = make_camera(cam);
    for (int k = 0; k < 3; k++) { a.C.light[k] = c->scene.point_light_pos[k]; a.C.ambient[k] = c->scene.ambient[k]; }
    const bool phong = cam->shading_mode == MI_SHADE_PHONG;      // debug shader: own kernel, `variant` is ignored
    // path_samples != 1 (tracing.rs:310) branches at every hit: the literal, recursive estimator (pt_branch)
    const bool recursive = !phong && (cam->path_samples != 1 || o->variant == MI_VARIANT_RECURSIVE);
    if (recursive && cam->path_depth > 64) return fail(MI_ERR_UNSUPPORTED, "recursive estimator: path_depth must be <= 64");
    const TileGrid g = tile_grid(cam, o->world);
    a.R.seed = o->seed; a.R.rank = o->rank; a.R.world = o->world;
    a.R.tiles_x = g.tx; a.R.tiles_y = g.ty; a.R.tiles_total = g.total;
    a.R.my_tiles = rank_tiles(g, o->rank, o->world);
    const bool lds = stage_in_lds(c, a.R);
    a.seed_key = seed_key(o->seed);
    a.out = d_compact;
    a.sig = (o->want_signature && d_sig) ? d_sig : nullptr;
    int variant = o->variant == MI_VARIANT_DEFAULT ? MI_VARIANT_WAVEFRONT : o->variant;
    if (variant != MI_VARIANT_SIMPLE && variant != MI_VARIANT_VOTED && variant != MI_VARIANT_VOTED_DIAG &&
        variant != MI_VARIANT_WAVEFRONT && variant != MI_VARIANT_RECURSIVE)
        return fail(MI_ERR_INVALID, "unknown variant %d (2, 5 and 6 were removed in ABI 3)", o->variant);
    const bool diag = variant == MI_VARIANT_VOTED_DIAG;
    a.R.vote_t = c->tune.vote_t; a.R.vote_a = c->tune.vote_a; a.R.k_steps = c->tune.k_steps;
    a.diag = nullptr;
    uint32_t n_blocks = g.padded * (uint32_t)kBlocksPerTile;
    if (diag) {
        a.diag = c->d_diag;
        HIP_TRY(hipMemsetAsync(c->d_diag, 0, 16 * sizeof(unsigned long long), stream));
    }
    WfArgs wa; uint32_t wf_batch = 1;
    if (variant == MI_VARIANT_WAVEFRONT && !phong && !recursive) {
        if (cam->aa_sample_count > 0xffffu) return fail(MI_ERR_UNSUPPORTED, "wavefront variant: aa_sample_count must be <= 65535");
        if (cam->path_depth > 0xffffu) return fail(MI_ERR_UNSUPPORTED, "wavefront variant: path_depth must be <= 65535");
        MI_TRY(wf_prepare(c, g.padded, cam->aa_sample_count, o->max_state_bytes, two_stage_mask(c->scene, o->flags) != 0u, wa, wf_batch));
        if (table && table->kind != kTableRays) {
            wa.pt_p = table->origins; wa.pt_n = table->dirs; wa.pt_rows = table->rows;
            wa.pt_probes = table->kind == kTableProbes ? 1u : 0u; wa.sh = table->sh; wa.m2 = table->m2;
        }
        else if (table) { wa.ray_o = table->origins; wa.ray_d = table->dirs; wa.rays_per_pixel = table->rows; }
    }
    HIP_TRY(hipEventRecord(c->ev_start, stream));
    if (phong)
        HIP_TRY(launch_phong(a, n_blocks, a.sig != nullptr, stream));
    else if (recursive)
        HIP_TRY(launch_branch(a, n_blocks, cam->path_samples, a.sig != nullptr, stream));
    else if (variant == MI_VARIANT_WAVEFRONT) {
        MI_TRY(render_tiles_wavefront(c, a, cam, wa, wf_batch, o->flags, d_compact, a.sig, range, stream));
    } else if (variant == MI_VARIANT_VOTED || variant == MI_VARIANT_VOTED_DIAG)
        HIP_TRY(launch_megakernel_voted(a, n_blocks, lds, a.sig != nullptr, diag, c->scene.gen_volumes, c->scene.lds_bytes + c->tune.lds_pad, stream));
    else
        HIP_TRY(launch_megakernel(a, n_blocks, lds, a.sig != nullptr, c->scene.lds_bytes, stream));
    HIP_TRY(hipEventRecord(c->ev_stop, stream));
    c->ev_recorded = true; c->ms_summed = false;
    if (st) {
        memset(st, 0, sizeof *st);
        st->pixels = rank_pixels(g, cam, o->rank, o->world);
        st->samples = st->pixels * (range.end - range.begin);
        st->tiles = a.R.my_tiles; st->tiles_padded = g.padded;
        st->scene_bytes = (uint32_t)c->blob_bytes; st->scene_in_lds = lds ? 1u : 0u;
    }
    return MI_OK;
}

extern "C" int mi_render_tiles_device(mi_ctx* c, const mi_camera_desc* cam, const mi_render_opts* opts,
                                      void* d_compact_f32, void* d_sig_u32, void* stream, mi_stats* stats) {
    if (!c) return fail(MI_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    return render_tiles(c, cam, opts, (float*)d_compact_f32, (uint32_t*)d_sig_u32, (hipStream_t)stream, stats);
}

extern "C" int mi_render_samples_device(mi_ctx* c, const mi_camera_desc* cam, const mi_render_opts* opts,
                                        uint32_t sample_begin, uint32_t sample_end, void* d_accum_f32x4,
                                        void* d_compact_f32, void* d_sig_u32, void* stream, mi_stats* stats) {
    if (!c) return fail(MI_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    SampleRange r = { sample_begin, sample_end, (float4*)d_accum_f32x4 };
    return render_tiles(c, cam, opts, (float*)d_compact_f32, (uint32_t*)d_sig_u32, (hipStream_t)stream, stats, &r);
}

extern "C" int mi_unpermute_device(mi_ctx* c, const mi_camera_desc* cam, int32_t world, const void* d_gathered_f32,
                                   void* d_image_f32, void* stream) {
    if (!c || !cam || world < 1 || !d_gathered_f32 || !d_image_f32) return fail(MI_ERR_INVALID, "mi_unpermute_device: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    const TileGrid g = tile_grid(cam, world);
    HIP_TRY(launch_unpermute((const float*)d_gathered_f32, (float*)d_image_f32, cam->screen_width, cam->screen_height, g.tx,
                             (uint32_t)world, g.padded, (hipStream_t)stream));
    return MI_OK;
}

extern "C" int mi_tonemap_device(mi_ctx* c, const mi_camera_desc* cam, const void* d_image_f32, void* d_image_u8, void* stream) {
    if (!c || !cam || !d_image_f32 || !d_image_u8) return fail(MI_ERR_INVALID, "mi_tonemap_device: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_tonemap((const float*)d_image_f32, (uint8_t*)d_image_u8, cam->screen_width * cam->screen_height,
                           1.0f / cam->gamma, (hipStream_t)stream));                            // tracing.rs:254
    return MI_OK;
}

extern "C" int mi_last_kernel_ms(mi_ctx* c, float* ms) {
    if (!c || !ms) return fail(MI_ERR_INVALID, "mi_last_kernel_ms: bad argument");
    if (!c->ev_recorded) return fail(MI_ERR_INVALID, "no kernel has been launched on this context");
    if (c->ms_summed) { *ms = c->ms_sum; return MI_OK; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->ev_stop));
    HIP_TRY(hipEventElapsedTime(ms, c->ev_start, c->ev_stop));
    return MI_OK;
}

// What mi_last_kernel_ms measures: `queue` (a callable returning MI_OK or a recorded failure) queues its launches on `stream` between the
// context's two timing events.  The host forms' uploads and downloads stay outside the timed region.
template <class Queue> static int timed(mi_ctx* c, hipStream_t stream, Queue queue) {
    HIP_TRY(hipEventRecord(c->ev_start, stream));
    MI_TRY(queue());
    HIP_TRY(hipEventRecord(c->ev_stop, stream));
    c->ev_recorded = true; c->ms_summed = false;
    return MI_OK;
}

// ------------------------------------------------------------------ ray queries (caller-supplied rays)
// Scene::intersect_ray / Scene::shade_ray for rays the caller made.  The device forms queue ONE kernel on `stream` between the context's
// timing events and return; they own no device memory.  The host forms move one chunk of rays at a time through a buffer of their own
// (never the wavefront pipeline's reserved ones) and advance first_key per chunk — the same answers as one call, by the keying.
static const uint32_t kRqChunk = 1u << 18;      // rays per chunk of the host-pointer forms: 27 MB of device scratch for a full intersect query
// The host forms.  A per-ray column of the caller's: `bytes` per ray at `host` (nullptr: an optional column that is absent), uploaded before
// the launch or (`out`) downloaded after it.  rq_chunked carves d_rq into one array of a chunk per column, in the order given, and for every
// chunk uploads, calls launch(first, n, dev) — dev[i] = column i's device array, nullptr when absent — downloads and synchronises.
struct RqColumn { const void* host; size_t bytes; bool out; };
// max_chunk: rows per chunk (a row is a ray, or a point of the hemisphere query, whose rows stand for n_samples rays each).
template <size_t N, class Launch> static int rq_chunked(mi_ctx* c, uint32_t n_rays, const RqColumn (&cols)[N], Launch launch,
                                                        size_t max_chunk = kRqChunk) {
    if (n_rays == 0) return MI_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t chunk = std::min<size_t>(n_rays, max_chunk);
    size_t off[N + 1] = { 0 };
    for (size_t i = 0; i < N; i++) off[i + 1] = off[i] + chunk * cols[i].bytes;
    MI_TRY(ensure(&c->d_rq, &c->rq_bytes, off[N]));
    void* dev[N];
    for (size_t i = 0; i < N; i++) dev[i] = cols[i].host ? (char*)c->d_rq + off[i] : nullptr;
    float ms_sum = 0.0f, ms = 0.0f;
    for (size_t first = 0; first < n_rays; first += chunk) {
        const size_t n = std::min<size_t>(chunk, (size_t)n_rays - first);
        for (size_t i = 0; i < N; i++) if (dev[i] && !cols[i].out)
            HIP_TRY(hipMemcpyAsync(dev[i], (const char*)cols[i].host + first * cols[i].bytes, n * cols[i].bytes, hipMemcpyHostToDevice, c->stream));
        MI_TRY(launch((uint32_t)first, (uint32_t)n, dev));
        for (size_t i = 0; i < N; i++) if (dev[i] && cols[i].out)
            HIP_TRY(hipMemcpyAsync((char*)cols[i].host + first * cols[i].bytes, dev[i], n * cols[i].bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));          // the next chunk reuses the buffer
        HIP_TRY(hipEventElapsedTime(&ms, c->ev_start, c->ev_stop));
        ms_sum += ms;
    }
    c->ms_summed = true; c->ms_sum = ms_sum;              // mi_last_kernel_ms: the sum over the chunks
    return MI_OK;
}

static int intersect_rays_device(mi_ctx* c, uint32_t n_rays, const float* origins, const float* dirs, float t_min, float t_max,
                                 uint32_t seed, uint32_t first_key, int32_t* out_object, float* out_distance, float* out_hitpoint,
                                 float* out_normal, int32_t* out_flags, float* out_uv, mi_material* out_material, hipStream_t stream) {
    RqArgs a;
    a.S = c->S;
    const bool lds = stage_in_lds(c, a);
    a.seed_key = seed_key(seed);
    a.first_key = first_key; a.n_rays = n_rays; a.t_min = t_min; a.t_max = t_max;
    a.origins = origins; a.dirs = dirs;
    a.out_object = out_object; a.out_distance = out_distance; a.out_hitpoint = out_hitpoint; a.out_normal = out_normal;
    a.out_flags = out_flags; a.out_uv = out_uv; a.out_material = (uint32_t*)out_material;
    const bool resolve = out_hitpoint || out_normal || out_flags || out_uv || out_material;     // else the visibility form
    return timed(c, stream, [&]() -> int {
        HIP_TRY(launch_rq_intersect(a, lds, c->scene.gen_volumes, resolve, c->scene.lds_bytes, c->n_cus, stream));
        return MI_OK;
    });
}

static int check_interval_args(const char* who, const char* out_name, mi_ctx* c, const float* origins, const float* dirs, float t_min, float t_max, const void* out) {
    if (!c) return fail(MI_ERR_INVALID, "ctx is NULL");      // (the intersect and the occluded query check the same things)
    if (!origins || !dirs || !out) return fail(MI_ERR_INVALID, "%s: origins, dirs and %s are required", who, out_name);
    if (t_min != t_min || t_max != t_max) return fail(MI_ERR_INVALID, "%s: t_min / t_max is NaN", who);
    if (!c->have_scene) return fail(MI_ERR_NO_SCENE, "no scene uploaded");
    return MI_OK;
}

extern "C" int mi_intersect_rays_device(mi_ctx* c, uint32_t n_rays, const float* origins, const float* dirs, float t_min, float t_max,
                                        uint32_t seed, uint32_t first_key, int32_t* out_object, float* out_distance,
                                        float* out_hitpoint, float* out_normal, int32_t* out_flags, float* out_uv,
                                        mi_material* out_material, void* stream) {
    MI_TRY(check_interval_args("mi_intersect_rays", "out_object", c, origins, dirs, t_min, t_max, out_object));
    if (n_rays == 0) return MI_OK;
    HIP_TRY(hipSetDevice(c->device));
    return intersect_rays_device(c, n_rays, origins, dirs, t_min, t_max, seed, first_key, out_object, out_distance, out_hitpoint,
                                 out_normal, out_flags, out_uv, out_material, (hipStream_t)stream);
}

extern "C" int mi_intersect_rays(mi_ctx* c, uint32_t n_rays, const float* origins, const float* dirs, float t_min, float t_max,
                                 uint32_t seed, uint32_t first_key, int32_t* out_object, float* out_distance, float* out_hitpoint,
                                 float* out_normal, int32_t* out_flags, float* out_uv, mi_material* out_material) {
    MI_TRY(check_interval_args("mi_intersect_rays", "out_object", c, origins, dirs, t_min, t_max, out_object));
    // 16-byte-friendly order: the 12-byte columns, material (40 B), uv (8 B), then the 4-byte ones
    enum { kO, kD, kHitpoint, kNormal, kMaterial, kUv, kObject, kDistance, kFlags };
    const RqColumn cols[] = { { origins, 12, false }, { dirs, 12, false }, { out_hitpoint, 12, true }, { out_normal, 12, true },
                              { out_material, sizeof(mi_material), true }, { out_uv, 8, true }, { out_object, 4, true },
                              { out_distance, 4, true }, { out_flags, 4, true } };
    return rq_chunked(c, n_rays, cols, [&](uint32_t first, uint32_t n, void* const* d) {
        return intersect_rays_device(c, n, (const float*)d[kO], (const float*)d[kD], t_min, t_max, seed, first_key + first, (int32_t*)d[kObject],
                                     (float*)d[kDistance], (float*)d[kHitpoint], (float*)d[kNormal], (int32_t*)d[kFlags], (float*)d[kUv],
                                     (mi_material*)d[kMaterial], c->stream);
    });
}

// mi_occluded_rays: the any-hit query (rq_occluded).  Same shape as the intersect pair; ray_t_max (may be NULL) replaces t_max per ray.
static int occluded_rays_device(mi_ctx* c, uint32_t n_rays, const float* origins, const float* dirs, float t_min, float t_max,
                                const float* ray_t_max, uint32_t seed, uint32_t first_key, uint8_t* out_occluded, hipStream_t stream) {
    RqOccArgs a;
    a.S = c->S;
    const bool lds = stage_in_lds(c, a);
    a.seed_key = seed_key(seed);
    a.first_key = first_key; a.n_rays = n_rays; a.t_min = t_min; a.t_max = t_max;
    a.origins = origins; a.dirs = dirs; a.ray_t_max = ray_t_max; a.out_occluded = out_occluded;
    return timed(c, stream, [&]() -> int {
        HIP_TRY(launch_rq_occluded(a, lds, c->scene.gen_volumes, c->scene.lds_bytes, c->n_cus, stream));
        return MI_OK;
    });
}

extern "C" int mi_occluded_rays_device(mi_ctx* c, uint32_t n_rays, const float* origins, const float* dirs, float t_min, float t_max,
                                       const float* ray_t_max, uint32_t seed, uint32_t first_key, uint8_t* out_occluded, void* stream) {
    MI_TRY(check_interval_args("mi_occluded_rays", "out_occluded", c, origins, dirs, t_min, t_max, out_occluded));
    if (n_rays == 0) return MI_OK;
    HIP_TRY(hipSetDevice(c->device));
    return occluded_rays_device(c, n_rays, origins, dirs, t_min, t_max, ray_t_max, seed, first_key, out_occluded, (hipStream_t)stream);
}

extern "C" int mi_occluded_rays(mi_ctx* c, uint32_t n_rays, const float* origins, const float* dirs, float t_min, float t_max,
                                const float* ray_t_max, uint32_t seed, uint32_t first_key, uint8_t* out_occluded) {
    MI_TRY(check_interval_args("mi_occluded_rays", "out_occluded", c, origins, dirs, t_min, t_max, out_occluded));
    if (ray_t_max)
        for (size_t i = 0; i < n_rays; i++)
            if (ray_t_max[i] != ray_t_max[i]) return fail(MI_ERR_INVALID, "mi_occluded_rays: ray_t_max[%zu] is NaN", i);
    const RqColumn cols[] = { { origins, 12, false }, { dirs, 12, false }, { ray_t_max, 4, false }, { out_occluded, 1, true } };
    return rq_chunked(c, n_rays, cols, [&](uint32_t first, uint32_t n, void* const* d) {
        return occluded_rays_device(c, n, (const float*)d[0], (const float*)d[1], t_min, t_max, (const float*)d[2], seed, first_key + first,
                                    (uint8_t*)d[3], c->stream);
    });
}

// mi_hemisphere_occlusion: rq_hemi makes the rays of every point on the device and reduces per point.
static int check_hemi_args(mi_ctx* c, const float* points, const float* normals, uint32_t first_sample, uint32_t n_samples, float t_min,
                           float t_max, uint32_t flags, const uint32_t* out_open) {
    if (!c) return fail(MI_ERR_INVALID, "ctx is NULL");
    if (!points || !normals || !out_open) return fail(MI_ERR_INVALID, "mi_hemisphere_occlusion: points, normals and out_open are required");
    if (n_samples == 0 || n_samples > 65535u) return fail(MI_ERR_INVALID, "mi_hemisphere_occlusion: n_samples %u is not in 1 .. 65535", n_samples);
    if ((uint64_t)first_sample + n_samples > (1ull << 31))
        return fail(MI_ERR_INVALID, "mi_hemisphere_occlusion: first_sample + n_samples = %llu exceeds 2^31", (unsigned long long)first_sample + n_samples);
    if (t_min != t_min || t_max != t_max) return fail(MI_ERR_INVALID, "mi_hemisphere_occlusion: t_min / t_max is NaN");
    if (flags & ~(uint32_t)MI_HEMI_WORLD_RADIUS) return fail(MI_ERR_INVALID, "mi_hemisphere_occlusion: unknown flag bits 0x%x", flags & ~(uint32_t)MI_HEMI_WORLD_RADIUS);
    if (!c->have_scene) return fail(MI_ERR_NO_SCENE, "no scene uploaded");
    return MI_OK;
}

static int hemisphere_occlusion_device(mi_ctx* c, uint32_t n_points, const float* points, const float* normals, uint32_t first_sample,
                                       uint32_t n_samples, float t_min, float t_max, uint32_t flags, uint32_t seed, uint32_t first_key,
                                       uint32_t* out_open, float* out_bent, hipStream_t stream) {
    RqHemiArgs a;
    a.S = c->S;
    const bool lds = stage_in_lds(c, a);
    a.seed_key = seed_key(seed);
    a.first_key = first_key; a.n_points = n_points; a.first_sample = first_sample; a.n_samples = n_samples;
    a.group_log2 = 0;
    while (a.group_log2 < 6u && (1u << a.group_log2) < n_samples) a.group_log2++;      // G = min(64, next_pow2(n_samples))
    a.world_radius = (flags & MI_HEMI_WORLD_RADIUS) ? 1u : 0u;
    a.t_min = t_min; a.t_max = t_max;
    a.points = points; a.normals = normals; a.out_open = out_open; a.out_bent = out_bent;
    return timed(c, stream, [&]() -> int {
        HIP_TRY(launch_rq_hemi(a, lds, c->scene.gen_volumes, c->scene.lds_bytes, c->n_cus, stream));
        return MI_OK;
    });
}

extern "C" int mi_hemisphere_occlusion_device(mi_ctx* c, uint32_t n_points, const float* points, const float* normals, uint32_t first_sample,
                                              uint32_t n_samples, float t_min, float t_max, uint32_t flags, uint32_t seed,
                                              uint32_t first_key, uint32_t* out_open, float* out_bent, void* stream) {
    MI_TRY(check_hemi_args(c, points, normals, first_sample, n_samples, t_min, t_max, flags, out_open));
    if (n_points == 0) return MI_OK;
    HIP_TRY(hipSetDevice(c->device));
    return hemisphere_occlusion_device(c, n_points, points, normals, first_sample, n_samples, t_min, t_max, flags, seed, first_key, out_open,
                                       out_bent, (hipStream_t)stream);
}

extern "C" int mi_hemisphere_occlusion(mi_ctx* c, uint32_t n_points, const float* points, const float* normals, uint32_t first_sample,
                                       uint32_t n_samples, float t_min, float t_max, uint32_t flags, uint32_t seed, uint32_t first_key,
                                       uint32_t* out_open, float* out_bent) {
    MI_TRY(check_hemi_args(c, points, normals, first_sample, n_samples, t_min, t_max, flags, out_open));
    // chunked over points: at most about 2^24 rays per launch, and never more points than a chunk of rays (28 B of scratch per point)
    const size_t max_points = std::min<size_t>(kRqChunk, std::max<size_t>(1, ((size_t)1 << 24) / n_samples));
    const RqColumn cols[] = { { points, 12, false }, { normals, 12, false }, { out_bent, 12, true }, { out_open, 4, true } };
    return rq_chunked(c, n_points, cols, [&](uint32_t first, uint32_t n, void* const* d) {
        return hemisphere_occlusion_device(c, n, (const float*)d[0], (const float*)d[1], first_sample, n_samples, t_min, t_max, flags, seed,
                                           first_key + first, (uint32_t*)d[3], (float*)d[2], c->stream);
    }, max_points);
}

static int shade_rays_device(mi_ctx* c, const mi_camera_desc* cam, uint32_t n_rays, const float* origins, const float* dirs,
                             uint32_t seed, uint32_t first_key, float* out_rgb, hipStream_t stream) {
    RqShadeArgs a;
    a.S = c->S;
    a.seed_key = seed_key(seed);
    a.first_key = first_key; a.n_rays = n_rays;
    a.path_depth = cam->path_depth; a.path_samples = cam->path_samples; a.max_trace_dist = cam->max_trace_dist;
    a.origins = origins; a.dirs = dirs; a.out_rgb = out_rgb;
    return timed(c, stream, [&]() -> int {
        HIP_TRY(launch_rq_shade(a, stream));
        return MI_OK;
    });
}

static int check_shade_args(mi_ctx* c, const mi_camera_desc* cam, const float* origins, const float* dirs, const float* out_rgb) {
    if (!c) return fail(MI_ERR_INVALID, "ctx is NULL");
    if (!cam || !origins || !dirs || !out_rgb) return fail(MI_ERR_INVALID, "mi_shade_rays: cam, origins, dirs and out_rgb are required");
    if (cam->shading_mode == MI_SHADE_PHONG) return fail(MI_ERR_UNSUPPORTED, "mi_shade_rays: ShadingMode::Phong is not available for caller-supplied rays");
    if (cam->shading_mode != MI_SHADE_PATHTRACE) return fail(MI_ERR_INVALID, "mi_shade_rays: unknown shading_mode %d", cam->shading_mode);
    if (cam->path_depth > 64) return fail(MI_ERR_UNSUPPORTED, "recursive estimator: path_depth must be <= 64");
    if (cam->path_samples == 0) return fail(MI_ERR_INVALID, "path_samples must be >= 1 (tracing.rs:318 divides by it)");
    if (std::isnan(cam->max_trace_dist)) return fail(MI_ERR_INVALID, "mi_shade_rays: max_trace_dist must not be NaN");
    if (!c->have_scene) return fail(MI_ERR_NO_SCENE, "no scene uploaded");
    return MI_OK;
}

extern "C" int mi_shade_rays_device(mi_ctx* c, const mi_camera_desc* cam, uint32_t n_rays, const float* origins, const float* dirs,
                                    uint32_t seed, uint32_t first_key, float* out_rgb, void* stream) {
    MI_TRY(check_shade_args(c, cam, origins, dirs, out_rgb));
    if (n_rays == 0) return MI_OK;
    HIP_TRY(hipSetDevice(c->device));
    return shade_rays_device(c, cam, n_rays, origins, dirs, seed, first_key, out_rgb, (hipStream_t)stream);
}

extern "C" int mi_shade_rays(mi_ctx* c, const mi_camera_desc* cam, uint32_t n_rays, const float* origins, const float* dirs,
                             uint32_t seed, uint32_t first_key, float* out_rgb) {
    MI_TRY(check_shade_args(c, cam, origins, dirs, out_rgb));
    const RqColumn cols[] = { { origins, 12, false }, { dirs, 12, false }, { out_rgb, 12, true } };
    return rq_chunked(c, n_rays, cols, [&](uint32_t first, uint32_t n, void* const* d) {
        return shade_rays_device(c, cam, n, (const float*)d[0], (const float*)d[1], seed, first_key + first, (float*)d[2], c->stream);
    });
}

extern "C" int mi_reserve(mi_ctx* c, const mi_camera_desc* cam, int32_t world, uint64_t max_state_bytes) {
    if (!c) return fail(MI_ERR_INVALID, "ctx is NULL");
    int rc = check_camera(cam);
    if (rc != MI_OK) return rc;
    if (world < 1) return fail(MI_ERR_INVALID, "bad world");
    HIP_TRY(hipSetDevice(c->device));
    WfArgs a;
    uint32_t s_batch = 1;
    return wf_prepare(c, tile_grid(cam, world).padded, cam->aa_sample_count, max_state_bytes, two_stage_mask(c->scene, 0u) != 0u, a, s_batch);
}

extern "C" int mi_last_pipeline_ms(mi_ctx* c, float* out8) {
    if (!c || !out8) return fail(MI_ERR_INVALID, "mi_last_pipeline_ms: bad argument");
    for (int i = 0; i < 8; i++) out8[i] = c->wf_ms[i];
    return MI_OK;
}

extern "C" int mi_last_pipeline_counts(mi_ctx* c, uint64_t* out8) {
    if (!c || !out8) return fail(MI_ERR_INVALID, "mi_last_pipeline_counts: bad argument");
    for (int i = 0; i < 8; i++) out8[i] = c->wf_counts[i];
    return MI_OK;
}

extern "C" int mi_last_diag(mi_ctx* c, uint64_t* out16) {
    if (!c || !out16) return fail(MI_ERR_INVALID, "mi_last_diag: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out16, c->d_diag, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return MI_OK;
}

extern "C" int mi_selftest(mi_ctx* c, uint64_t* out4) {
    if (!c || !out4) return fail(MI_ERR_INVALID, "mi_selftest: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    for (int k = 0; k < 4; k++) out4[k] = 0;
    HIP_TRY(hipMemsetAsync(c->d_diag, 0, 16 * sizeof(unsigned long long), c->stream));
    HIP_TRY(launch_selftest_rcp(c->d_diag, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    unsigned long long bad = 0;
    HIP_TRY(hipMemcpy(&bad, c->d_diag, sizeof bad, hipMemcpyDeviceToHost));
    out4[0] = bad; out4[1] = 1ull << 32;
    return MI_OK;
}

// The whole image on this GPU into host buffers: render, un-permute, tone-map, download (mi_render; with `table`, mi_render_rays / _points).
// out_sh (mi_render_probes): table->sh holds the compact SH records; un-permuted into the plane behind them and downloaded as well.
// out_m2 (mi_render_points_moments): the same for table->m2, whose 3-float records fb_unpermute un-permutes.
static int render_image(mi_ctx* c, const mi_camera_desc* cam, const mi_render_opts* opts, const RayTable* table, float* out_rgb_f32,
                        uint8_t* out_rgb_u8, uint32_t* out_sig, mi_stats* stats, float* out_sh = nullptr, float* out_m2 = nullptr) {
    int rc;
    const hipEvent_t t0 = c->ev_t0, t1 = c->ev_t1;      // owned by the context: no early return can leak them
    const TileGrid g = tile_grid(cam, 1);
    size_t npix = (size_t)cam->screen_width * cam->screen_height;
    size_t cbytes = (size_t)g.padded * kTilePixels * 3 * sizeof(float);
    if ((rc = ensure((void**)&c->d_compact, &c->compact_bytes, cbytes)) != MI_OK) return rc;
    if ((rc = ensure((void**)&c->d_image, &c->image_bytes, npix * 3 * sizeof(float))) != MI_OK) return rc;
    bool want_sig = opts->want_signature && out_sig;
    if (want_sig) {
        if ((rc = ensure((void**)&c->d_sigc, &c->sigc_bytes, (size_t)g.padded * kTilePixels * 4)) != MI_OK) return rc;
        if ((rc = ensure((void**)&c->d_sigi, &c->sigi_bytes, npix * 4)) != MI_OK) return rc;
    }
    mi_render_opts o = *opts;
    o.want_signature = want_sig ? 1 : 0;
    HIP_TRY(hipEventRecord(t0, c->stream));
    rc = render_tiles(c, cam, &o, c->d_compact, want_sig ? c->d_sigc : nullptr, c->stream, stats, nullptr, table);
    if (rc != MI_OK) return rc;
    HIP_TRY(launch_unpermute(c->d_compact, c->d_image, cam->screen_width, cam->screen_height, g.tx, 1, g.padded, c->stream));
    if (out_rgb_f32) HIP_TRY(hipMemcpyAsync(out_rgb_f32, c->d_image, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (out_rgb_u8) {
        if ((rc = ensure((void**)&c->d_u8, &c->u8_bytes, npix * 3)) != MI_OK) return rc;
        HIP_TRY(launch_tonemap(c->d_image, c->d_u8, (uint32_t)npix, 1.0f / cam->gamma, c->stream));
        HIP_TRY(hipMemcpyAsync(out_rgb_u8, c->d_u8, npix * 3, hipMemcpyDeviceToHost, c->stream));
    }
    if (want_sig) {
        HIP_TRY(launch_sig_unpermute(c->d_sigc, c->d_sigi, cam->screen_width, cam->screen_height, g.tx, 1, g.padded, c->stream));
        HIP_TRY(hipMemcpyAsync(out_sig, c->d_sigi, npix * 4, hipMemcpyDeviceToHost, c->stream));
    }
    if (out_sh) {
        float* plane = table->sh + (size_t)g.padded * kTilePixels * kShFloats;
        HIP_TRY(launch_sh_unpermute(table->sh, plane, cam->screen_width, cam->screen_height, g.tx, 1, g.padded, c->stream));
        HIP_TRY(hipMemcpyAsync(out_sh, plane, npix * kShFloats * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    if (out_m2) {
        float* plane = table->m2 + (size_t)g.padded * kTilePixels * 3;
        HIP_TRY(launch_unpermute(table->m2, plane, cam->screen_width, cam->screen_height, g.tx, 1, g.padded, c->stream));
        HIP_TRY(hipMemcpyAsync(out_m2, plane, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipEventRecord(t1, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (stats) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev_start, c->ev_stop)); stats->kernel_ms = ms;
        HIP_TRY(hipEventElapsedTime(&ms, t0, t1)); stats->total_ms = ms;
    }
    return MI_OK;
}

extern "C" int mi_render(mi_ctx* c, const mi_camera_desc* cam, const mi_render_opts* opts, float* out_rgb_f32,
                         uint8_t* out_rgb_u8, uint32_t* out_sig, mi_stats* stats) {
    if (!c) return fail(MI_ERR_INVALID, "ctx is NULL");
    if (!opts) return fail(MI_ERR_INVALID, "opts is NULL");
    if (opts->rank != 0 || opts->world != 1) return fail(MI_ERR_INVALID, "mi_render renders a whole image: rank/world must be 0/1");
    int rc = check_camera(cam);
    if (rc != MI_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return render_image(c, cam, opts, nullptr, out_rgb_f32, out_rgb_u8, out_sig, stats);
}

// ------------------------------------------------------------------ ray-table rendering (caller-made rays through the wavefront pipeline)
// A table [rows][H][W][3] of origins and one of directions replaces Camera::generate_rays for one render; everything behind the camera
// pass of the pipeline is mi_render's.  Every refusal happens here, before anything is allocated, copied or launched.
static int check_table_args(mi_ctx* c, const mi_camera_desc* cam, const mi_render_opts* opts, const float* origins, const float* dirs,
                            uint32_t rays_per_pixel, TableKind kind = kTableRays) {
    if (!c) return fail(MI_ERR_INVALID, "ctx is NULL");
    if (!opts) return fail(MI_ERR_INVALID, "opts is NULL");
    if (kind == kTableProbes ? !origins : (!origins || !dirs))        // a probe has no second table
        return fail(MI_ERR_INVALID, kind == kTableProbes ? "mi_render_probes: the points table is required" :
                    kind == kTablePoints ? "mi_render_points: the points and normals tables are required" : "mi_render_rays: the origins and dirs tables are required");
    MI_TRY(check_table_camera(cam, rays_per_pixel));
    if (opts->variant != MI_VARIANT_DEFAULT && opts->variant != MI_VARIANT_WAVEFRONT)
        return fail(MI_ERR_UNSUPPORTED, "ray-table rendering runs on the default (wavefront) variant only, not variant %d: use mi_shade_rays for the recursive estimator", opts->variant);
    if (cam->aa_sample_count > 0xffffu) return fail(MI_ERR_UNSUPPORTED, "wavefront variant: aa_sample_count must be <= 65535");
    if (cam->path_depth > 0xffffu) return fail(MI_ERR_UNSUPPORTED, "wavefront variant: path_depth must be <= 65535");
    if (opts->world < 1 || opts->rank < 0 || opts->rank >= opts->world) return fail(MI_ERR_INVALID, "bad rank/world");
    if (!c->have_scene) return fail(MI_ERR_NO_SCENE, "no scene uploaded");
    return MI_OK;
}

// The context's moments buffer for a W x H image: the compact records, then the plane render_image un-permutes them into
static int moments_buffer(mi_ctx* c, const mi_camera_desc* cam, float** out) {
    const size_t slots = (size_t)tile_grid(cam, 1).padded * kTilePixels + (size_t)cam->screen_width * cam->screen_height;
    MI_TRY(ensure(&c->d_m2, &c->m2_bytes, slots * 3 * sizeof(float)));
    *out = (float*)c->d_m2;
    return MI_OK;
}

// The context's SH buffer for a W x H image: the compact records, then the plane render_image un-permutes them into
static int sh_buffer(mi_ctx* c, const mi_camera_desc* cam, float** out) {
    const size_t slots = (size_t)tile_grid(cam, 1).padded * kTilePixels + (size_t)cam->screen_width * cam->screen_height;
    MI_TRY(ensure(&c->d_sh, &c->sh_bytes, slots * kShFloats * sizeof(float)));
    *out = (float*)c->d_sh;
    return MI_OK;
}

// Host pointers: upload the two tables (light probes: the one) into the context's own buffer, then mi_render's body.  `what` names the
// entry point in messages.  out_sh: light probes only, and required there.  out_m2: point tables only (the _moments calls).
static int render_table_host(mi_ctx* c, const mi_camera_desc* cam, const mi_render_opts* opts, const float* first, const float* second,
                             uint32_t rows, TableKind kind, const char* what, float* out_rgb_f32, uint8_t* out_rgb_u8, uint32_t* out_sig,
                             mi_stats* stats, float* out_sh = nullptr, float* out_m2 = nullptr) {
    MI_TRY(check_table_args(c, cam, opts, first, second, rows, kind));
    if (opts->rank != 0 || opts->world != 1) return fail(MI_ERR_INVALID, "%s renders a whole image: rank/world must be 0/1", what);
    if (kind == kTableProbes && !out_sh) return fail(MI_ERR_INVALID, "%s: out_sh is required", what);
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = (size_t)rows * cam->screen_height * cam->screen_width * 3 * sizeof(float);     // of each table
    MI_TRY(ensure(&c->d_rays, &c->rays_bytes, (second ? 2 : 1) * bytes));
    HIP_TRY(hipMemcpyAsync(c->d_rays, first, bytes, hipMemcpyHostToDevice, c->stream));
    if (second) HIP_TRY(hipMemcpyAsync((char*)c->d_rays + bytes, second, bytes, hipMemcpyHostToDevice, c->stream));
    RayTable table = { (const float*)c->d_rays, second ? (const float*)((const char*)c->d_rays + bytes) : nullptr, rows, kind, nullptr, nullptr };
    if (out_sh) MI_TRY(sh_buffer(c, cam, &table.sh));
    if (out_m2) MI_TRY(moments_buffer(c, cam, &table.m2));
    const mi_camera_desc tc = table_camera(cam);
    return render_image(c, &tc, opts, &table, out_rgb_f32, out_rgb_u8, out_sig, stats, out_sh, out_m2);
}

// Device pointers: mi_render_tiles_device and mi_render_samples_device in one call.  d_compact_sh: light probes only, may be NULL;
// d_compact_m2: point tables only, may be NULL.
static int render_table_device(mi_ctx* c, const mi_camera_desc* cam, const mi_render_opts* opts, const float* d_first, const float* d_second,
                               uint32_t rows, TableKind kind, uint32_t sample_begin, uint32_t sample_end, void* d_accum_f32x4,
                               void* d_compact_f32, void* d_sig_u32, void* stream, mi_stats* stats, void* d_compact_sh = nullptr,
                               void* d_compact_m2 = nullptr) {
    MI_TRY(check_table_args(c, cam, opts, d_first, d_second, rows, kind));
    HIP_TRY(hipSetDevice(c->device));
    const RayTable table = { d_first, d_second, rows, kind, (float*)d_compact_sh, (float*)d_compact_m2 };
    const mi_camera_desc tc = table_camera(cam);
    // [0, aa_sample_count) without an accumulator is a whole render (mi_render_tiles_device); anything else a progressive call
    const bool whole = sample_begin == 0 && sample_end == cam->aa_sample_count && !d_accum_f32x4;
    SampleRange r = { sample_begin, sample_end, (float4*)d_accum_f32x4 };
    return render_tiles(c, &tc, opts, (float*)d_compact_f32, (uint32_t*)d_sig_u32, (hipStream_t)stream, stats, whole ? nullptr : &r, &table);
}

extern "C" int mi_render_rays(mi_ctx* c, const mi_camera_desc* cam, const mi_render_opts* opts, const float* origins, const float* dirs,
                              uint32_t rays_per_pixel, float* out_rgb_f32, uint8_t* out_rgb_u8, uint32_t* out_sig, mi_stats* stats) {
    return render_table_host(c, cam, opts, origins, dirs, rays_per_pixel, kTableRays, "mi_render_rays", out_rgb_f32, out_rgb_u8, out_sig, stats);
}

extern "C" int mi_render_rays_device(mi_ctx* c, const mi_camera_desc* cam, const mi_render_opts* opts, const float* d_origins,
                                     const float* d_dirs, uint32_t rays_per_pixel, uint32_t sample_begin, uint32_t sample_end,
                                     void* d_accum_f32x4, void* d_compact_f32, void* d_sig_u32, void* stream, mi_stats* stats) {
    return render_table_device(c, cam, opts, d_origins, d_dirs, rays_per_pixel, kTableRays, sample_begin, sample_end, d_accum_f32x4,
                               d_compact_f32, d_sig_u32, stream, stats);
}

// ------------------------------------------------------------------ point-table rendering (lightmap baking: the rays are made on the GPU)
// mi_render_rays with a table of surface points and one of normals: the camera pass draws sample_hemisphere(normal) per sample on a
// stream of its own, so 24 B per texel cross the bus whatever the sample count.  Same checks, same upload buffer, same body.
extern "C" int mi_render_points(mi_ctx* c, const mi_camera_desc* cam, const mi_render_opts* opts, const float* points, const float* normals,
                                uint32_t rows_per_pixel, float* out_rgb_f32, uint8_t* out_rgb_u8, uint32_t* out_sig, mi_stats* stats) {
    return render_table_host(c, cam, opts, points, normals, rows_per_pixel, kTablePoints, "mi_render_points", out_rgb_f32, out_rgb_u8, out_sig, stats);
}

extern "C" int mi_render_points_device(mi_ctx* c, const mi_camera_desc* cam, const mi_render_opts* opts, const float* d_points,
                                       const float* d_normals, uint32_t rows_per_pixel, uint32_t sample_begin, uint32_t sample_end,
                                       void* d_accum_f32x4, void* d_compact_f32, void* d_sig_u32, void* stream, mi_stats* stats) {
    return render_table_device(c, cam, opts, d_points, d_normals, rows_per_pixel, kTablePoints, sample_begin, sample_end, d_accum_f32x4,
                               d_compact_f32, d_sig_u32, stream, stats);
}

// ------------------------------------------------------------------ second moments of a point-table bake
// mi_render_points with a second output: wf_reduce_m2, behind wf_reduce in every batch, sums the squares of the same samples.  Same
// checks, same upload buffer, same body; the plain outputs are mi_render_points' bits (no timed kernel changes).
extern "C" int mi_render_points_moments(mi_ctx* c, const mi_camera_desc* cam, const mi_render_opts* opts, const float* points,
                                        const float* normals, uint32_t rows_per_pixel, float* out_m2, float* out_rgb_f32,
                                        uint8_t* out_rgb_u8, uint32_t* out_sig, mi_stats* stats) {
    if (!out_m2) return fail(MI_ERR_INVALID, "mi_render_points_moments: out_m2 is required");
    return render_table_host(c, cam, opts, points, normals, rows_per_pixel, kTablePoints, "mi_render_points_moments", out_rgb_f32, out_rgb_u8,
                             out_sig, stats, nullptr, out_m2);
}

extern "C" int mi_render_points_moments_device(mi_ctx* c, const mi_camera_desc* cam, const mi_render_opts* opts, const float* d_points,
                                               const float* d_normals, uint32_t rows_per_pixel, uint32_t sample_begin, uint32_t sample_end,
                                               void* d_accum_f32x4, void* d_compact_m2, void* d_compact_f32, void* d_sig_u32, void* stream,
                                               mi_stats* stats) {
    return render_table_device(c, cam, opts, d_points, d_normals, rows_per_pixel, kTablePoints, sample_begin, sample_end, d_accum_f32x4,
                               d_compact_f32, d_sig_u32, stream, stats, nullptr, d_compact_m2);
}

// ------------------------------------------------------------------ directional lightmaps: the SH L2 projection of a point-table bake
// mi_render_points with a second output: wf_reduce_psh, behind wf_reduce in every batch, weights the same samples by the SH basis of their
// hemisphere directions (mi_render_probes' records, scaled by 2 pi / S).  Same checks, same upload buffer, same body; the plain outputs
// are mi_render_points' bits (no timed kernel changes).  The records live in the buffer mi_render_probes' do.
extern "C" int mi_render_points_sh(mi_ctx* c, const mi_camera_desc* cam, const mi_render_opts* opts, const float* points,
                                   const float* normals, uint32_t rows_per_pixel, float* out_sh, float* out_rgb_f32,
                                   uint8_t* out_rgb_u8, uint32_t* out_sig, mi_stats* stats) {
    if (!out_sh) return fail(MI_ERR_INVALID, "mi_render_points_sh: out_sh is required");
    return render_table_host(c, cam, opts, points, normals, rows_per_pixel, kTablePoints, "mi_render_points_sh", out_rgb_f32, out_rgb_u8,
                             out_sig, stats, out_sh);
}

extern "C" int mi_render_points_sh_device(mi_ctx* c, const mi_camera_desc* cam, const mi_render_opts* opts, const float* d_points,
                                          const float* d_normals, uint32_t rows_per_pixel, uint32_t sample_begin, uint32_t sample_end,
                                          void* d_accum_f32x4, void* d_compact_sh, void* d_compact_f32, void* d_sig_u32, void* stream,
                                          mi_stats* stats) {
    return render_table_device(c, cam, opts, d_points, d_normals, rows_per_pixel, kTablePoints, sample_begin, sample_end, d_accum_f32x4,
                               d_compact_f32, d_sig_u32, stream, stats, d_compact_sh);
}

// ------------------------------------------------------------------ lightmap atlas (the point table of a mesh's uv atlas, made on the GPU)
// tracing.py lightmap_texels as kernels: the table mi_render_points reads is made in HBM from the mesh, one row or one jittered row per
// sample.  The arguments are checked before the context, so that a caller's mistakes are reported the same with and without a device.
static int check_lm_args(const char* who, mi_ctx* c, const mi_mesh* mesh, uint32_t width, uint32_t height, uint32_t rows, uint32_t flags,
                         float offset, const void* out_points, const void* out_normals) {
    if (!mesh) return fail(MI_ERR_INVALID, "%s: mesh is NULL", who);
    if (mesh->n_vertices < 0 || mesh->n_triangles < 0) return fail(MI_ERR_INVALID, "%s: negative n_vertices / n_triangles", who);
    if ((mesh->n_vertices > 0 && (!mesh->positions || !mesh->normals || !mesh->texcoords)) || (mesh->n_triangles > 0 && !mesh->indices))
        return fail(MI_ERR_INVALID, "%s: the mesh's positions, normals, texcoords and indices are required", who);
    if (!out_points || !out_normals) return fail(MI_ERR_INVALID, "%s: out_points and out_normals are required", who);
    if (width == 0 || width > 32768u || height == 0 || height > 32768u)
        return fail(MI_ERR_INVALID, "%s: width %u / height %u is not in 1 .. 32768", who, width, height);
    if (rows == 0 || rows > 65535u) return fail(MI_ERR_INVALID, "%s: rows %u is not in 1 .. 65535", who, rows);
    if (flags & ~(uint32_t)MI_LM_JITTER) return fail(MI_ERR_INVALID, "%s: unknown flag bits 0x%x", who, flags & ~(uint32_t)MI_LM_JITTER);
    if (offset != offset) return fail(MI_ERR_INVALID, "%s: offset is NaN", who);
    if (3ull * width * height > (1ull << 31))
        return fail(MI_ERR_INVALID, "%s: 3 * width * height = %llu exceeds 2^31 (the jitter streams' keys end at 3 W H)", who, 3ull * width * height);
    if (!c) return fail(MI_ERR_INVALID, "ctx is NULL");
    return MI_OK;
}

static int check_lm_indices(const char* who, const mi_mesh* mesh) {
    for (size_t i = 0; i < 3 * (size_t)mesh->n_triangles; i++)
        if (mesh->indices[i] >= (uint32_t)mesh->n_vertices)
            return fail(MI_ERR_INVALID, "%s: index %u of triangle %zu is outside the %d vertices", who, mesh->indices[i], i / 3, mesh->n_vertices);
    return MI_OK;
}

// Queue the kernels on `stream`; `mesh`'s arrays and the outputs are device pointers.  exact: wait for the count pass and size the bins'
// list to its sum (the blocking forms); otherwise size it from what the previous call needed and never wait — a list that turns out too
// short costs time, not correctness (LmArgs).  Growing a buffer frees the old one, which waits for the device.
static int lightmap_texels_device(mi_ctx* c, const mi_mesh* mesh, uint32_t width, uint32_t height, uint32_t rows, uint32_t flags, uint32_t seed,
                                  float offset, float* d_points, float* d_normals, int32_t* d_triangle, hipStream_t stream, bool exact) {
    LmArgs a;
    a.positions = mesh->positions; a.normals = mesh->normals; a.texcoords = mesh->texcoords; a.indices = mesh->indices;
    a.n_vertices = (uint32_t)mesh->n_vertices; a.n_triangles = (uint32_t)mesh->n_triangles;
    a.width = width; a.height = height; a.rows = rows; a.jitter = (flags & MI_LM_JITTER) ? 1u : 0u;
    a.seed_key = seed_key(seed);
    a.tiles_x = (width + kTile - 1) / kTile; a.tiles_y = (height + kTile - 1) / kTile;
    double M[3][4];
    for (int r = 0; r < 3; r++) for (int k = 0; k < 4; k++) a.m[4 * r + k] = M[r][k] = (double)mesh->transform[4 * k + r];     // column-major
    const double cof[9] = { M[1][1] * M[2][2] - M[1][2] * M[2][1], M[1][2] * M[2][0] - M[1][0] * M[2][2], M[1][0] * M[2][1] - M[1][1] * M[2][0],
                            M[0][2] * M[2][1] - M[0][1] * M[2][2], M[0][0] * M[2][2] - M[0][2] * M[2][0], M[0][1] * M[2][0] - M[0][0] * M[2][1],
                            M[0][1] * M[1][2] - M[0][2] * M[1][1], M[0][2] * M[1][0] - M[0][0] * M[1][2], M[0][0] * M[1][1] - M[0][1] * M[1][0] };
    const double det = M[0][0] * cof[0] + M[0][1] * cof[1] + M[0][2] * cof[2];
    for (int k = 0; k < 9; k++) a.nm[k] = cof[k] / det;          // the inverse transpose; a singular transform leaves no finite normal: every texel empty
    a.offset = (double)offset;
    a.out_points = d_points; a.out_normals = d_normals; a.out_triangle = d_triangle;

    const size_t nt = (size_t)a.tiles_x * a.tiles_y;
    if (!c->h_lm_total) {
        HIP_TRY(hipHostMalloc((void**)&c->h_lm_total, sizeof(unsigned long long), hipHostMallocMapped | hipHostMallocCoherent));
        *c->h_lm_total = 0;
        HIP_TRY(hipHostGetDevicePointer((void**)&c->h_lm_total_dev, c->h_lm_total, 0));
    }
    MI_TRY(ensure(&c->d_lm_hdr, &c->lm_hdr_bytes, nt * 8 + (nt + 1) * 8));
    a.counts = (uint32_t*)c->d_lm_hdr; a.cursors = a.counts + nt; a.offsets = (unsigned long long*)(a.cursors + nt);
    a.host_total = c->h_lm_total_dev;
    const unsigned long long kMaxList = 1ull << 30;               // entries: 4 GiB; bins beyond it are resolved from the whole mesh
    auto size_list = [&](unsigned long long entries) {
        MI_TRY(ensure(&c->d_lm_list, &c->lm_list_bytes, (size_t)std::max<unsigned long long>(1, std::min(entries, kMaxList)) * sizeof(uint32_t)));
        a.list = (uint32_t*)c->d_lm_list; a.cap = c->lm_list_bytes / sizeof(uint32_t);
        return (int)MI_OK;
    };
    if (!exact) {
        const unsigned long long last = *(volatile unsigned long long*)c->h_lm_total;      // what the previous call's bins held: a hint only
        MI_TRY(size_list(std::min<unsigned long long>((unsigned long long)a.n_triangles * nt, std::max<unsigned long long>(last, 4ull * a.n_triangles + 1024))));
    }
    return timed(c, stream, [&]() -> int {
        HIP_TRY(hipMemsetAsync(c->d_lm_hdr, 0, nt * 8, stream));
        HIP_TRY(launch_lm_count(a, stream));
        if (exact) {
            HIP_TRY(hipStreamSynchronize(stream));
            MI_TRY(size_list(*(volatile unsigned long long*)c->h_lm_total));
        }
        HIP_TRY(launch_lm_resolve(a, stream));
        return MI_OK;
    });
}

extern "C" int mi_lightmap_texels_device(mi_ctx* c, const mi_mesh* mesh, uint32_t width, uint32_t height, uint32_t rows, uint32_t flags,
                                         uint32_t seed, float offset, float* out_points, float* out_normals, int32_t* out_triangle, void* stream) {
    MI_TRY(check_lm_args("mi_lightmap_texels_device", c, mesh, width, height, rows, flags, offset, out_points, out_normals));
    HIP_TRY(hipSetDevice(c->device));
    return lightmap_texels_device(c, mesh, width, height, rows, flags, seed, offset, out_points, out_normals, out_triangle, (hipStream_t)stream, false);
}

// The mesh's four arrays into the context's mesh buffer (on c->stream); `dev` is `mesh` with device pointers
static int upload_lm_mesh(mi_ctx* c, const mi_mesh* mesh, mi_mesh* dev) {
    const size_t nv = (size_t)mesh->n_vertices, ni = 3 * (size_t)mesh->n_triangles;
    const size_t off[5] = { 0, nv * 12, nv * 24, nv * 32, nv * 32 + ni * 4 };
    MI_TRY(ensure(&c->d_lm_mesh, &c->lm_mesh_bytes, std::max<size_t>(off[4], 16)));
    const void* src[4] = { mesh->positions, mesh->normals, mesh->texcoords, mesh->indices };
    for (int k = 0; k < 4; k++)
        if (off[k + 1] > off[k]) HIP_TRY(hipMemcpyAsync((char*)c->d_lm_mesh + off[k], src[k], off[k + 1] - off[k], hipMemcpyHostToDevice, c->stream));
    *dev = *mesh;
    dev->positions = (const float*)((char*)c->d_lm_mesh + off[0]); dev->normals = (const float*)((char*)c->d_lm_mesh + off[1]);
    dev->texcoords = (const float*)((char*)c->d_lm_mesh + off[2]); dev->indices = (const uint32_t*)((char*)c->d_lm_mesh + off[3]);
    return MI_OK;
}

extern "C" int mi_lightmap_texels(mi_ctx* c, const mi_mesh* mesh, uint32_t width, uint32_t height, uint32_t rows, uint32_t flags, uint32_t seed,
                                  float offset, float* out_points, float* out_normals, int32_t* out_triangle) {
    MI_TRY(check_lm_args("mi_lightmap_texels", c, mesh, width, height, rows, flags, offset, out_points, out_normals));
    MI_TRY(check_lm_indices("mi_lightmap_texels", mesh));
    HIP_TRY(hipSetDevice(c->device));
    mi_mesh dev;
    MI_TRY(upload_lm_mesh(c, mesh, &dev));
    const size_t n = (size_t)rows * height * width;
    MI_TRY(ensure(&c->d_lm_out, &c->lm_out_bytes, n * (out_triangle ? 28 : 24)));
    float* d_points = (float*)c->d_lm_out; float* d_normals = d_points + 3 * n;
    int32_t* d_triangle = out_triangle ? (int32_t*)(d_normals + 3 * n) : nullptr;
    MI_TRY(lightmap_texels_device(c, &dev, width, height, rows, flags, seed, offset, d_points, d_normals, d_triangle, c->stream, true));
    HIP_TRY(hipMemcpyAsync(out_points, d_points, n * 12, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(out_normals, d_normals, n * 12, hipMemcpyDeviceToHost, c->stream));
    if (out_triangle) HIP_TRY(hipMemcpyAsync(out_triangle, d_triangle, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MI_OK;
}

// The whole bake: the mesh up, its table made in the context's table buffer (mi_render_rays'), then mi_render_points' body on it.
// out_m2 (mi_bake_lightmap_moments): the second moments as well, as mi_render_points_moments returns them.
// out_sh (mi_bake_lightmap_sh): the SH L2 records as well, as mi_render_points_sh returns them (never together with out_m2).
static int bake_lightmap(const char* who, mi_ctx* c, const mi_camera_desc* cam, const mi_render_opts* opts, const mi_mesh* mesh, uint32_t flags,
                         float offset, float* out_rgb_f32, uint8_t* out_rgb_u8, uint32_t* out_sig, int32_t* out_triangle, mi_stats* stats,
                         float* out_m2, float* out_sh = nullptr) {
    if (!c) return fail(MI_ERR_INVALID, "ctx is NULL");
    if (!mesh) return fail(MI_ERR_INVALID, "%s: mesh is NULL", who);
    const uint32_t rows = (cam && (flags & MI_LM_JITTER)) ? cam->aa_sample_count : 1u;
    MI_TRY(check_table_args(c, cam, opts, (const float*)mesh, (const float*)mesh, rows, kTablePoints));       // (the tables are made here: any non-NULL)
    if (opts->rank != 0 || opts->world != 1) return fail(MI_ERR_INVALID, "%s renders a whole image: rank/world must be 0/1", who);
    const uint32_t W = cam->screen_width, H = cam->screen_height;
    MI_TRY(check_lm_args(who, c, mesh, W, H, rows, flags, offset, mesh, mesh));
    MI_TRY(check_lm_indices(who, mesh));
    HIP_TRY(hipSetDevice(c->device));
    mi_mesh dev;
    MI_TRY(upload_lm_mesh(c, mesh, &dev));
    const size_t n = (size_t)rows * H * W, bytes = n * 3 * sizeof(float);
    MI_TRY(ensure(&c->d_rays, &c->rays_bytes, 2 * bytes));
    if (out_triangle) MI_TRY(ensure(&c->d_lm_out, &c->lm_out_bytes, n * 4));
    float* d_points = (float*)c->d_rays; float* d_normals = (float*)((char*)c->d_rays + bytes);
    MI_TRY(lightmap_texels_device(c, &dev, W, H, rows, flags, opts->seed, offset, d_points, d_normals, out_triangle ? (int32_t*)c->d_lm_out : nullptr,
                                  c->stream, true));
    if (out_triangle) HIP_TRY(hipMemcpyAsync(out_triangle, c->d_lm_out, n * 4, hipMemcpyDeviceToHost, c->stream));
    RayTable table = { d_points, d_normals, rows, kTablePoints, nullptr, nullptr };
    if (out_m2) MI_TRY(moments_buffer(c, cam, &table.m2));
    if (out_sh) MI_TRY(sh_buffer(c, cam, &table.sh));
    const mi_camera_desc tc = table_camera(cam);
    return render_image(c, &tc, opts, &table, out_rgb_f32, out_rgb_u8, out_sig, stats, out_sh, out_m2);
}

extern "C" int mi_bake_lightmap(mi_ctx* c, const mi_camera_desc* cam, const mi_render_opts* opts, const mi_mesh* mesh, uint32_t flags,
                                float offset, float* out_rgb_f32, uint8_t* out_rgb_u8, uint32_t* out_sig, int32_t* out_triangle, mi_stats* stats) {
    return bake_lightmap("mi_bake_lightmap", c, cam, opts, mesh, flags, offset, out_rgb_f32, out_rgb_u8, out_sig, out_triangle, stats, nullptr);
}

extern "C" int mi_bake_lightmap_moments(mi_ctx* c, const mi_camera_desc* cam, const mi_render_opts* opts, const mi_mesh* mesh, uint32_t flags,
                                        float offset, float* out_m2, float* out_rgb_f32, uint8_t* out_rgb_u8, uint32_t* out_sig,
                                        int32_t* out_triangle, mi_stats* stats) {
    if (!out_m2) return fail(MI_ERR_INVALID, "mi_bake_lightmap_moments: out_m2 is required");
    return bake_lightmap("mi_bake_lightmap_moments", c, cam, opts, mesh, flags, offset, out_rgb_f32, out_rgb_u8, out_sig, out_triangle, stats,
                         out_m2);
}

extern "C" int mi_bake_lightmap_sh(mi_ctx* c, const mi_camera_desc* cam, const mi_render_opts* opts, const mi_mesh* mesh, uint32_t flags,
                                   float offset, float* out_sh, float* out_rgb_f32, uint8_t* out_rgb_u8, uint32_t* out_sig,
                                   int32_t* out_triangle, mi_stats* stats) {
    if (!out_sh) return fail(MI_ERR_INVALID, "mi_bake_lightmap_sh: out_sh is required");
    return bake_lightmap("mi_bake_lightmap_sh", c, cam, opts, mesh, flags, offset, out_rgb_f32, out_rgb_u8, out_sig, out_triangle, stats,
                         nullptr, out_sh);
}

// ------------------------------------------------------------------ lightmap post-processing: what the calls below share
static inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }

// A call's buffers are described ONCE, as a list of columns: `bytes` at `at` (nullptr: an optional column that is absent), read by the call
// (kIn), written by it (kOut), both (kInOut), or scratch that only the host form has to provide (kDevice).  The list serves the host form's
// staging and the device form's overlap test alike, so a byte count cannot be right in one and wrong in the other.  name: what an overlap
// refusal calls an output; an output without one is not tested (the finish calls' out_valid never was).
enum class Stage { kIn, kOut, kInOut, kDevice };
struct StageColumn { const void* at; size_t bytes; Stage dir; const char* name = nullptr; };

// The host forms.  staged lays the columns present out at 256-byte-aligned offsets of the context's ONE staging buffer, in the order given
// (an absent column takes no space and gets a null device pointer), uploads kIn / kInOut on c->stream, calls body(dev) — dev[i] = column
// i's device array — downloads kOut / kInOut and synchronises; of a kDevice column the caller fetches what it needs before the next staged
// call.  All uploads precede all downloads, so an output of the caller's may alias one of its inputs; the copies stay outside the body's
// timed region.
template <size_t N, class Body> static int staged(mi_ctx* c, const StageColumn (&cols)[N], Body body) {
    HIP_TRY(hipSetDevice(c->device));
    size_t off[N + 1] = { 0 };
    for (size_t i = 0; i < N; i++) off[i + 1] = off[i] + (cols[i].at ? up256(cols[i].bytes) : 0);
    MI_TRY(ensure(&c->d_io, &c->io_bytes, off[N]));
    void* dev[N];
    for (size_t i = 0; i < N; i++) dev[i] = cols[i].at ? (char*)c->d_io + off[i] : nullptr;
    for (size_t i = 0; i < N; i++) if (dev[i] && (cols[i].dir == Stage::kIn || cols[i].dir == Stage::kInOut))
        HIP_TRY(hipMemcpyAsync(dev[i], cols[i].at, cols[i].bytes, hipMemcpyHostToDevice, c->stream));
    MI_TRY(body(dev));
    for (size_t i = 0; i < N; i++) if (dev[i] && (cols[i].dir == Stage::kOut || cols[i].dir == Stage::kInOut))
        HIP_TRY(hipMemcpyAsync((void*)cols[i].at, dev[i], cols[i].bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MI_OK;
}

// Both forms of a call whose arguments are checked.  host: the columns are HOST arrays: body(dev, c->stream) runs staged, the call blocks.
// Else they are DEVICE arrays and never work in place: a named output that overlaps an input is refused (a null address is skipped), then
// body(the caller's own pointers — null for a kDevice column —, stream) queues the work.  Between the two sit the only things the families
// place differently: a NULL context is refused here, AFTER the overlap test (a family that refuses it before tests it before it calls),
// and `empty` — a call with nothing to launch — returns MI_OK here: after the overlap test, before any device call.
template <size_t N, class Body>
static int run_columns(const char* who, mi_ctx* c, bool host, void* stream, const StageColumn (&cols)[N], bool empty, Body body) {
    if (!host)
        for (const StageColumn& o : cols) if (o.name && (o.dir == Stage::kOut || o.dir == Stage::kInOut))
            for (const StageColumn& in : cols) if (in.dir == Stage::kIn) {
                const uintptr_t a = (uintptr_t)o.at, b = (uintptr_t)in.at;
                if (a && b && a < b + in.bytes && b < a + o.bytes)
                    return fail(MI_ERR_INVALID, "%s: %s overlaps an input (the passes are never in place)", who, o.name);
            }
    if (!c) return fail(MI_ERR_INVALID, "ctx is NULL");
    if (empty) return MI_OK;
    if (host) return staged(c, cols, [&](void* const* dev) -> int { return body(dev, c->stream); });
    HIP_TRY(hipSetDevice(c->device));
    void* at[N];
    for (size_t i = 0; i < N; i++) at[i] = cols[i].dir == Stage::kDevice ? nullptr : (void*)cols[i].at;
    return body(at, (hipStream_t)stream);
}
// ------------------------------------------------------------------ lightmap finishing (edge-aware a-trous filter, gutter dilation)
// tracing.py lightmap_finish, lightmap_finish_sh and lightmap_finish_var as kernels, one pass per launch, in three forms:
//   plain     [H][W][3] texels; scratch d_lmf; lmf_mask, lmf_atrous per level, lmf_dilate per pass
//   SH        [H][W][9][3] records; scratch of its own (d_lsh: a plain and an SH finish may be queued on two streams); lmf_mask, lsh_atrous, lmf_dilate at 27 floats
//   variance  the plain form's texels, scratch, mask and dilation; lmv_init (with or without counts), then lmv_blur and lmv_atrous per
//             level, the variance planes in d_lmv
// The arguments every form takes, and the variance form's further ones (counts: mi_lightmap_finish_var_counts' per-texel counts, which take
// the place of `samples` in the initial variance — samples is then 2 — or nullptr).
enum class FinishForm { kPlain, kSh, kVar };
struct FinishArgs {
    uint32_t width, height; const float* image; const float* points; const float* normals; uint32_t levels, normal_power_log2;
    float sigma_plane, reach, sigma_color; uint32_t dilate; float* out; uint8_t* out_valid;
};
struct FinishVarArgs { const float* m2; const uint32_t* counts; uint32_t samples; float color_floor; float* out_var; };

// The arguments are checked before the context, as the atlas' are.  What the forms check alike, in their shared order (samples: the
// variance form's, or nullptr):
static int check_finish_args(const char* who, const FinishArgs& f, const uint32_t* samples) {
    if (f.width == 0 || f.width > 32768u || f.height == 0 || f.height > 32768u)
        return fail(MI_ERR_INVALID, "%s: width %u / height %u is not in 1 .. 32768", who, f.width, f.height);
    if (f.levels > 8) return fail(MI_ERR_INVALID, "%s: levels %u is above 8", who, f.levels);
    if (f.normal_power_log2 > 7) return fail(MI_ERR_INVALID, "%s: normal_power_log2 %u is above 7", who, f.normal_power_log2);
    if (f.dilate > 256) return fail(MI_ERR_INVALID, "%s: dilate %u is above 256", who, f.dilate);
    if (samples && (*samples < 2 || *samples > 65535u)) return fail(MI_ERR_INVALID, "%s: samples %u is not in 2 .. 65535", who, *samples);
    if (!(f.sigma_plane > 0.0f)) return fail(MI_ERR_INVALID, "%s: sigma_plane must be > 0 (+inf turns the plane weight off)", who);
    if (!(f.reach > 0.0f)) return fail(MI_ERR_INVALID, "%s: reach must be > 0 (+inf turns the reach test off)", who);
    return MI_OK;
}

static int check_lmf_args(const char* who, const FinishArgs& f) {
    if (!f.image || !f.points || !f.normals || !f.out) return fail(MI_ERR_INVALID, "%s: image, points, normals and out_image are required", who);
    MI_TRY(check_finish_args(who, f, nullptr));
    if (!(f.sigma_color > 0.0f)) return fail(MI_ERR_INVALID, "%s: sigma_color must be > 0 (+inf turns the colour weight off)", who);
    return MI_OK;
}

static int check_lmv_args(const char* who, const FinishArgs& f, const FinishVarArgs& v) {
    if (!f.image || !v.m2 || !f.points || !f.normals || !f.out)
        return fail(MI_ERR_INVALID, "%s: image, m2, points, normals and out_image are required", who);
    MI_TRY(check_finish_args(who, f, &v.samples));
    if (!(f.sigma_color >= 0.0f) || std::isinf(f.sigma_color)) return fail(MI_ERR_INVALID, "%s: sigma_color must be finite and >= 0", who);
    if (!(v.color_floor > 0.0f)) return fail(MI_ERR_INVALID, "%s: color_floor must be > 0 (+inf turns the colour weight off)", who);
    return MI_OK;
}

// Queue a finish on `stream` by its plan (render_plan.cpp finish_plan: which slot the initial step and every pass reads and writes);
// every pointer is a device pointer and no output overlaps an input.  fv: the variance form's arguments, nullptr for the other two.
static int finish_device(mi_ctx* c, FinishForm form, const FinishArgs& f, const FinishVarArgs* fv, hipStream_t stream) {
    const bool sh = form == FinishForm::kSh, var = form == FinishForm::kVar;
    const size_t n = (size_t)f.width * f.height, img = n * (sh ? kShFloats : 3) * sizeof(float), msk = up256(n), pln = msk * sizeof(float);
    MI_TRY(ensure(sh ? &c->d_lsh : &c->d_lmf, sh ? &c->lsh_bytes : &c->lmf_bytes, 2 * img + 2 * msk));
    if (var) MI_TRY(ensure(&c->d_lmv, &c->lmv_bytes, 3 * pln));
    // the plan's slots, by their enums' values: two images and two masks in the form's scratch, two variance planes (and the colour weight's
    // denominators behind them) in d_lmv
    char* const s = (char*)(sh ? c->d_lsh : c->d_lmf);
    float* const image[4] = { (float*)f.image, f.out, (float*)s, (float*)(s + img) };
    uint8_t* const mask[3] = { (uint8_t*)s + 2 * img, (uint8_t*)s + 2 * img + msk, f.out_valid };
    float* const vplane[3] = { (float*)c->d_lmv, var ? (float*)((char*)c->d_lmv + pln) : nullptr, var ? fv->out_var : nullptr };
    LmfArgs a{};
    a.points = f.points; a.normals = f.normals;
    a.width = f.width; a.height = f.height;
    a.tiles_x = (f.width + kTile - 1) / kTile; a.tiles_y = (f.height + kTile - 1) / kTile;
    LmvArgs v{};
    if (var) {              // the weights are lmv_atrous' then: lmf_mask and lmf_dilate read none
        v.m2 = fv->m2; v.points = f.points; v.normals = f.normals;
        v.width = f.width; v.height = f.height; v.tiles_x = a.tiles_x; v.tiles_y = a.tiles_y;
        v.npow = f.normal_power_log2; v.samples = fv->samples;
        v.sigma_plane = f.sigma_plane; v.reach = f.reach; v.sigma_color = f.sigma_color; v.color_floor = fv->color_floor;
        v.den = v.den_out = (float*)((char*)c->d_lmv + 2 * pln);
    } else {
        a.npow = f.normal_power_log2; a.sigma_plane = f.sigma_plane; a.reach = f.reach; a.sigma_color = f.sigma_color;
    }
    const FinishPlan plan = finish_plan(f.levels, f.dilate, f.out_valid != nullptr, var, var && fv->out_var);
    return timed(c, stream, [&]() -> int {
        a.src = f.image; a.dst = f.out; a.copy = plan.copy; a.mask_out = mask[(int)plan.mask_init];
        HIP_TRY(launch_lmf_mask(a, sh, stream));
        a.copy = 0;
        if (var) {
            v.src = f.image; v.var_out = vplane[(int)plan.var_init];
            HIP_TRY(launch_lmv_init(v, fv->counts, false, stream));
        }
        for (const FinishPass& p : plan.passes) {
            a.src = image[(int)p.src]; a.dst = image[(int)p.dst];
            if (!p.level) {
                a.mask_in = mask[(int)p.mask_in]; a.mask_out = mask[(int)p.mask_out];
                HIP_TRY(launch_lmf_dilate(a, sh, stream));
            } else if (var) {
                v.src = a.src; v.dst = a.dst; v.step = p.step;
                v.var_in = vplane[(int)p.var_in]; v.var_out = vplane[(int)p.var_out];
                HIP_TRY(launch_lmv_blur(v, stream));
                HIP_TRY(launch_lmv_atrous(v, stream));
            } else {
                a.step = p.step;            // (the choice between lmf_atrous' two forms is the plain form's alone)
                HIP_TRY(sh ? launch_lsh_atrous(a, stream)
                           : launch_lmf_atrous(a, a.step <= c->tune.lmf_lds_max_step, &c->lmf_big_lds_enabled, stream));
            }
        }
        return MI_OK;
    });
}

// The entry of every form (host: see run_columns; out may alias image there: see staged).  The refusals in order: the arguments, then a
// NULL context — but the variance forms' device calls refuse an overlap first, and a NULL context after it.
static int finish_entry(const char* who, FinishForm form, mi_ctx* c, const FinishArgs& f, const FinishVarArgs* fv, bool host, void* stream) {
    MI_TRY(fv ? check_lmv_args(who, f, *fv) : check_lmf_args(who, f));
    if (!fv && !c) return fail(MI_ERR_INVALID, "ctx is NULL");
    const bool sh = form == FinishForm::kSh;
    const size_t n = (size_t)f.width * f.height, tab = n * 3 * sizeof(float), rec = sh ? n * kShFloats * sizeof(float) : tab;
    enum { kImage, kM2, kPoints, kNormals, kCounts, kOut, kOutVar, kOutValid };
    const StageColumn cols[] = { { f.image, rec, Stage::kIn }, { fv ? fv->m2 : nullptr, tab, Stage::kIn }, { f.points, tab, Stage::kIn },
                                 { f.normals, tab, Stage::kIn }, { fv ? fv->counts : nullptr, n * 4, Stage::kIn },
                                 { f.out, rec, Stage::kOut, sh ? "out_sh" : "out_image" },
                                 { fv ? fv->out_var : nullptr, n * 4, Stage::kOut, "out_var" },
                                 { f.out_valid, n, Stage::kOut } };          // (no name: the device forms have never tested out_valid)
    return run_columns(who, c, host, stream, cols, false, [&](void* const* d, hipStream_t s) -> int {
        FinishArgs df = f;
        df.image = (const float*)d[kImage]; df.points = (const float*)d[kPoints]; df.normals = (const float*)d[kNormals];
        df.out = (float*)d[kOut]; df.out_valid = (uint8_t*)d[kOutValid];
        FinishVarArgs dv{};
        if (fv) { dv = *fv; dv.m2 = (const float*)d[kM2]; dv.counts = (const uint32_t*)d[kCounts]; dv.out_var = (float*)d[kOutVar]; }
        return finish_device(c, form, df, fv ? &dv : nullptr, s);
    });
}

extern "C" int mi_lightmap_finish_device(mi_ctx* c, uint32_t width, uint32_t height, const float* image, const float* points,
                                         const float* normals, uint32_t levels, uint32_t normal_power_log2, float sigma_plane, float reach,
                                         float sigma_color, uint32_t dilate, float* out_image, uint8_t* out_valid, void* stream) {
    return finish_entry("mi_lightmap_finish_device", FinishForm::kPlain, c, { width, height, image, points, normals, levels,
                        normal_power_log2, sigma_plane, reach, sigma_color, dilate, out_image, out_valid }, nullptr, false, stream);
}

extern "C" int mi_lightmap_finish(mi_ctx* c, uint32_t width, uint32_t height, const float* image, const float* points, const float* normals,
                                  uint32_t levels, uint32_t normal_power_log2, float sigma_plane, float reach, float sigma_color,
                                  uint32_t dilate, float* out_image, uint8_t* out_valid) {
    return finish_entry("mi_lightmap_finish", FinishForm::kPlain, c, { width, height, image, points, normals, levels, normal_power_log2,
                        sigma_plane, reach, sigma_color, dilate, out_image, out_valid }, nullptr, true, nullptr);
}

// ------------------------------------------------------------------ directional lightmaps: the finish and the evaluation
// The SH form of the finish: the arguments are mi_lightmap_finish's and are checked by the same function.
extern "C" int mi_lightmap_finish_sh_device(mi_ctx* c, uint32_t width, uint32_t height, const float* sh, const float* points,
                                            const float* normals, uint32_t levels, uint32_t normal_power_log2, float sigma_plane, float reach,
                                            float sigma_color, uint32_t dilate, float* out_sh, uint8_t* out_valid, void* stream) {
    return finish_entry("mi_lightmap_finish_sh_device", FinishForm::kSh, c, { width, height, sh, points, normals, levels,
                        normal_power_log2, sigma_plane, reach, sigma_color, dilate, out_sh, out_valid }, nullptr, false, stream);
}

extern "C" int mi_lightmap_finish_sh(mi_ctx* c, uint32_t width, uint32_t height, const float* sh, const float* points, const float* normals,
                                     uint32_t levels, uint32_t normal_power_log2, float sigma_plane, float reach, float sigma_color,
                                     uint32_t dilate, float* out_sh, uint8_t* out_valid) {
    return finish_entry("mi_lightmap_finish_sh", FinishForm::kSh, c, { width, height, sh, points, normals, levels, normal_power_log2,
                        sigma_plane, reach, sigma_color, dilate, out_sh, out_valid }, nullptr, true, nullptr);
}

// tracing.py lightmap_sh_eval as one kernel (lsh_eval): one lane per point.  Checked before the context; n == 0 launches nothing.
static int check_lsh_eval_args(const char* who, mi_ctx* c, const float* sh, const float* normals, const float* out_irradiance) {
    if (!sh || !normals || !out_irradiance) return fail(MI_ERR_INVALID, "%s: sh, normals and out_irradiance are required", who);
    if (!c) return fail(MI_ERR_INVALID, "ctx is NULL");
    return MI_OK;
}

static int lightmap_sh_eval_device(mi_ctx* c, uint32_t n, const float* d_sh, const float* d_normals, float* d_out, hipStream_t stream) {
    LshEvalArgs a{};
    a.sh = d_sh; a.normals = d_normals; a.out_irradiance = d_out; a.n = n;
    return timed(c, stream, [&]() -> int {
        HIP_TRY(launch_lsh_eval(a, stream));
        return MI_OK;
    });
}

extern "C" int mi_lightmap_sh_eval_device(mi_ctx* c, uint32_t n, const float* sh, const float* normals, float* out_irradiance, void* stream) {
    MI_TRY(check_lsh_eval_args("mi_lightmap_sh_eval_device", c, sh, normals, out_irradiance));
    if (n == 0) return MI_OK;
    HIP_TRY(hipSetDevice(c->device));
    return lightmap_sh_eval_device(c, n, sh, normals, out_irradiance, (hipStream_t)stream);
}

extern "C" int mi_lightmap_sh_eval(mi_ctx* c, uint32_t n, const float* sh, const float* normals, float* out_irradiance) {
    MI_TRY(check_lsh_eval_args("mi_lightmap_sh_eval", c, sh, normals, out_irradiance));
    if (n == 0) return MI_OK;                  // before any device call
    const size_t rec = (size_t)n * kShFloats * sizeof(float), tab = (size_t)n * 3 * sizeof(float);
    const StageColumn cols[] = { { sh, rec, Stage::kIn }, { normals, tab, Stage::kIn }, { out_irradiance, tab, Stage::kOut } };
    return staged(c, cols, [&](void* const* d) -> int {
        return lightmap_sh_eval_device(c, n, (const float*)d[0], (const float*)d[1], (float*)d[2], c->stream);
    });
}

// ------------------------------------------------------------------ lightmap lookup (a finished lightmap read at uv points)
// tracing.py lightmap_sample / lightmap_sh_sample (level 0 alone) and lightmap_sample_lod / lightmap_sh_sample_lod (trilinear over the
// chain of render_plan.cpp mip_plan) as one kernel per form, format and channel count: one lane per point, no scratch, no scene.  ONE
// argument record, checker, device body and entry serve all eighteen calls — f32, packed and BC6H texels, both level forms:
//   format    0 = f32 texels, MI_LP_* (the packed calls further down) or kLpBc6h (the BC6H call, further down still)
//   channels  3 or 27, or 0: the fused SH form, which reads 27 values per texel and the normals and writes three per point
//   admits    which level forms the entry point has: mi_lightmap_sample / _sh_sample level 0 alone (levels 1, no mips, no lod), the
//             _lod calls the chain alone (a NULL lod is a missing argument there), the packed and BC6H calls either: lod == NULL reads
//             level 0 alone, which then wants levels == 1 and no mips, and allows MI_LS_NEAREST, which the chain form refuses.
enum class Levels { kZero, kChain, kEither };
struct LookupArgs {
    uint32_t format, channels; Levels admits;
    uint32_t width, height; const void* image; const uint8_t* valid; uint32_t levels; const void* mips; const uint8_t* mip_valid;
    uint32_t n; const float* uv; const float* normals; const float* lod; uint32_t flags; float* out; float* out_weight;
};
// The bytes of one stored texel of `channels` values
static inline size_t texel_bytes(uint32_t format, size_t channels) {
    return format == MI_LP_RGB9E5 ? sizeof(uint32_t) : channels * (format == MI_LP_F16 ? sizeof(uint16_t) : sizeof(float));
}
// The bytes of one stored level of width x height texels, and of levels 1 .. L - 1 of a chain: texels, or for kLpBc6h 16-byte blocks
static inline size_t level_bytes(uint32_t format, uint32_t width, uint32_t height, size_t channels) {
    if (format == kLpBc6h) return (size_t)bc6h_extent(width) * bc6h_extent(height) * 16u;
    return (size_t)width * height * texel_bytes(format, channels);
}
static inline size_t mips_bytes(uint32_t format, const MipPlan& plan, size_t channels) {
    return format == kLpBc6h ? (size_t)bc6h_plan(plan).blocks * 16u : (size_t)plan.texels * texel_bytes(format, channels);
}

// What every packed call checks of its format, before anything else (sh: the fused form, which reads signed coefficients)
static int check_packed_format(const char* who, uint32_t format, uint32_t channels, bool sh) {
    if (format != MI_LP_F16 && format != MI_LP_RGB9E5)
        return fail(MI_ERR_INVALID, "%s: format %u is not MI_LP_F16 or MI_LP_RGB9E5 (f32 texels take the unpacked calls)", who, format);
    if (sh && format != MI_LP_F16) return fail(MI_ERR_INVALID, "%s: SH coefficients are signed: only MI_LP_F16 holds them", who);
    if (!sh && channels != 3 && channels != (uint32_t)kShFloats) return fail(MI_ERR_INVALID, "%s: channels %u is not 3 or 27", who, channels);
    if (format == MI_LP_RGB9E5 && channels != 3)
        return fail(MI_ERR_INVALID, "%s: MI_LP_RGB9E5 holds 3 unsigned channels, not %u (SH records pack as MI_LP_F16)", who, channels);
    return MI_OK;
}

// Checked before the context, nothing is launched: the alignment of blocks (device pointers only: the host form stages them aligned),
// the level form, the pointers, the size, the channel count, the levels, the flags.  chain: the form the call takes; plan: its levels
// (one for the level-0 form, whose levels is 1).
static int check_lookup_args(const char* who, const LookupArgs& l, bool host, bool chain, MipPlan* plan) {
    const bool sh = l.channels == 0;
    if (l.format == kLpBc6h && !host && (((uintptr_t)l.image | (uintptr_t)l.mips) & 15u))
        return fail(MI_ERR_INVALID, "%s: the blocks are not 16-byte aligned", who);
    if (!chain && l.admits == Levels::kEither && (l.levels != 1 || l.mips || l.mip_valid))
        return fail(MI_ERR_INVALID, "%s: lod == NULL reads level 0 alone: levels must be 1 (not %u) and mips, mip_valid NULL", who, l.levels);
    if (!l.image || !l.uv || !l.out || (sh && !l.normals) || (chain && !l.lod))
        return fail(MI_ERR_INVALID, chain ? (sh ? "%s: sh, uv, normals, lod and out_irradiance are required" : "%s: image, uv, lod and out are required")
                                          : (sh ? "%s: sh, uv, normals and out_irradiance are required" : "%s: image, uv and out are required"), who);
    if (l.width == 0 || l.width > 32768u || l.height == 0 || l.height > 32768u)
        return fail(MI_ERR_INVALID, "%s: width %u / height %u is not in 1 .. 32768", who, l.width, l.height);
    if (!sh && l.channels != 3 && l.channels != (uint32_t)kShFloats) return fail(MI_ERR_INVALID, "%s: channels %u is not 3 or 27", who, l.channels);
    if (!mip_plan(l.width, l.height, l.levels, kMipFuse, plan))
        return fail(MI_ERR_INVALID, "%s: levels %u is above the full chain of %u x %u, %u", who, l.levels, l.width, l.height,
                    mip_full_chain(l.width, l.height));
    if (plan->levels > 1 && !l.mips) return fail(MI_ERR_INVALID, "%s: mips is required with %u levels", who, plan->levels);
    if (chain && (l.flags & MI_LS_NEAREST)) return fail(MI_ERR_INVALID, "%s: MI_LS_NEAREST is refused: nearest addressing has no mips", who);
    if (l.flags & ~MI_LS_NEAREST) return fail(MI_ERR_INVALID, "%s: unknown flag bits 0x%x", who, l.flags & ~MI_LS_NEAREST);
    return MI_OK;
}

// Queue the lookup on `stream`: every pointer is a device pointer
static int lookup_device(mi_ctx* c, const LookupArgs& l, bool chain, const MipPlan& plan, hipStream_t stream) {
    LmlArgs a{};
    a.image = l.image; a.valid = l.valid; a.uv = l.uv; a.normals = l.normals; a.out = l.out; a.out_weight = l.out_weight;
    a.width = l.width; a.height = l.height; a.n = l.n; a.nearest = l.flags & MI_LS_NEAREST;
    LmlLodArgs b{};
    if (chain) {
        b.image = l.image; b.valid = l.valid; b.mips = l.mips; b.mip_valid = l.mip_valid; b.uv = l.uv; b.lod = l.lod; b.normals = l.normals;
        b.out = l.out; b.out_weight = l.out_weight; b.levels = plan.levels; b.n = l.n;
        for (uint32_t k = 0; k < plan.levels; k++) { b.off[k] = plan.level[k].offset; b.lw[k] = plan.level[k].width; b.lh[k] = plan.level[k].height; }
        if (l.format == kLpBc6h) {
            const Bc6hPlan blocks = bc6h_plan(plan);
            for (uint32_t k = 0; k < plan.levels; k++) b.boff[k] = (uint32_t)blocks.level[k].offset;
        }
    }
    return timed(c, stream, [&]() -> int {
        HIP_TRY(chain ? launch_lookup(b, l.format, l.channels, stream) : launch_lookup(a, l.format, l.channels, stream));
        return MI_OK;
    });
}

// The entry of every lookup (host: see run_columns): the arguments, the context, the overlaps; n == 0 launches nothing.  A level-0 call
// has no mips, mip_valid and lod columns, and the host form stages none for a chain of one level.
static int lookup_entry(const char* who, mi_ctx* c, const LookupArgs& l, bool host, void* stream) {
    const bool chain = l.admits == Levels::kChain || (l.admits == Levels::kEither && l.lod);
    MipPlan plan;
    MI_TRY(check_lookup_args(who, l, host, chain, &plan));
    if (!c) return fail(MI_ERR_INVALID, "ctx is NULL");
    const size_t texels = (size_t)l.width * l.height, in_c = l.channels ? l.channels : (uint32_t)kShFloats, out_c = l.channels ? l.channels : 3u;
    const bool no_mips = host && plan.levels == 1;
    enum { kImage, kValid, kMips, kMipValid, kUv, kLod, kNormals, kOut, kWeight };
    const StageColumn cols[] = { { l.image, level_bytes(l.format, l.width, l.height, in_c), Stage::kIn }, { l.valid, texels, Stage::kIn },
                                 { no_mips ? nullptr : l.mips, mips_bytes(l.format, plan, in_c), Stage::kIn },
                                 { no_mips ? nullptr : l.mip_valid, (size_t)plan.texels, Stage::kIn },
                                 { l.uv, (size_t)l.n * 2 * sizeof(float), Stage::kIn }, { l.lod, (size_t)l.n * sizeof(float), Stage::kIn },
                                 { l.normals, (size_t)l.n * 3 * sizeof(float), Stage::kIn },
                                 { l.out, (size_t)l.n * out_c * sizeof(float), Stage::kOut, l.channels ? "out" : "out_irradiance" },
                                 { l.out_weight, (size_t)l.n * sizeof(float), Stage::kOut, "out_weight" } };
    return run_columns(who, c, host, stream, cols, l.n == 0, [&](void* const* d, hipStream_t s) -> int {
        LookupArgs dl = l;
        dl.image = d[kImage]; dl.valid = (const uint8_t*)d[kValid]; dl.mips = d[kMips]; dl.mip_valid = (const uint8_t*)d[kMipValid];
        dl.uv = (const float*)d[kUv]; dl.lod = (const float*)d[kLod]; dl.normals = (const float*)d[kNormals];
        dl.out = (float*)d[kOut]; dl.out_weight = (float*)d[kWeight];
        return lookup_device(c, dl, chain, plan, s);
    });
}

extern "C" int mi_lightmap_sample_device(mi_ctx* c, uint32_t width, uint32_t height, uint32_t channels, const float* image, const uint8_t* valid,
                                         uint32_t n, const float* uv, uint32_t flags, float* out, float* out_weight, void* stream) {
    if (channels == 0) return fail(MI_ERR_INVALID, "mi_lightmap_sample_device: channels 0 is not 3 or 27");
    return lookup_entry("mi_lightmap_sample_device", c, { 0, channels, Levels::kZero, width, height, image, valid, 1, nullptr, nullptr, n, uv,
                        nullptr, nullptr, flags, out, out_weight }, false, stream);
}

extern "C" int mi_lightmap_sample(mi_ctx* c, uint32_t width, uint32_t height, uint32_t channels, const float* image, const uint8_t* valid,
                                  uint32_t n, const float* uv, uint32_t flags, float* out, float* out_weight) {
    if (channels == 0) return fail(MI_ERR_INVALID, "mi_lightmap_sample: channels 0 is not 3 or 27");
    return lookup_entry("mi_lightmap_sample", c, { 0, channels, Levels::kZero, width, height, image, valid, 1, nullptr, nullptr, n, uv, nullptr,
                        nullptr, flags, out, out_weight }, true, nullptr);
}

extern "C" int mi_lightmap_sh_sample_device(mi_ctx* c, uint32_t width, uint32_t height, const float* sh, const uint8_t* valid, uint32_t n,
                                            const float* uv, const float* normals, uint32_t flags, float* out_irradiance, float* out_weight,
                                            void* stream) {
    return lookup_entry("mi_lightmap_sh_sample_device", c, { 0, 0, Levels::kZero, width, height, sh, valid, 1, nullptr, nullptr, n, uv, normals,
                        nullptr, flags, out_irradiance, out_weight }, false, stream);
}

extern "C" int mi_lightmap_sh_sample(mi_ctx* c, uint32_t width, uint32_t height, const float* sh, const uint8_t* valid, uint32_t n,
                                     const float* uv, const float* normals, uint32_t flags, float* out_irradiance, float* out_weight) {
    return lookup_entry("mi_lightmap_sh_sample", c, { 0, 0, Levels::kZero, width, height, sh, valid, 1, nullptr, nullptr, n, uv, normals, nullptr,
                        flags, out_irradiance, out_weight }, true, nullptr);
}

// ------------------------------------------------------------------ lightmap mips (the coverage-aware pyramid and the trilinear lookups)
// tracing.py lightmap_mips as lmm_reduce<3> / lmm_reduce<27>, launched by render_plan.cpp mip_plan (the layout and which level every
// launch reads and how many it writes); the trilinear lookups are the lookup above in its chain form, which reads the same layout.
struct MipsArgs {
    uint32_t width, height, channels; const float* image; const uint8_t* valid; uint32_t levels; float* out_mips; uint8_t* out_valid;
    float* out_coverage;
};

// Checked before the context, nothing is launched: the pointers, the size, the channel count, the levels
static int check_mips_args(const char* who, const MipsArgs& m, MipPlan* plan) {
    if (!m.image || !m.out_mips) return fail(MI_ERR_INVALID, "%s: image and out_mips are required", who);
    if (m.width == 0 || m.width > 32768u || m.height == 0 || m.height > 32768u)
        return fail(MI_ERR_INVALID, "%s: width %u / height %u is not in 1 .. 32768", who, m.width, m.height);
    if (m.channels != 3 && m.channels != (uint32_t)kShFloats) return fail(MI_ERR_INVALID, "%s: channels %u is not 3 or 27", who, m.channels);
    if (!mip_plan(m.width, m.height, m.levels, kMipFuse, plan))
        return fail(MI_ERR_INVALID, "%s: levels %u is above the full chain of %u x %u, %u", who, m.levels, m.width, m.height,
                    mip_full_chain(m.width, m.height));
    return MI_OK;
}

// Queue the pyramid on `stream`: every pointer is a device pointer, cov the coverage planes of levels 1 .. L - 1 (the caller's or scratch)
static int mips_device(mi_ctx* c, const MipsArgs& m, const MipPlan& plan, float* cov, hipStream_t stream) {
    return timed(c, stream, [&]() -> int {
        for (const MipLaunch& l : plan.launches) {
            const MipLevel& src = plan.level[l.src];
            LmmArgs a{};
            a.src = l.src == 0 ? m.image : m.out_mips + src.offset * m.channels;
            a.src_valid = l.src == 0 ? m.valid : nullptr;
            a.src_cov = l.src == 0 ? nullptr : cov + src.offset;
            a.mips = m.out_mips; a.mip_valid = m.out_valid; a.mip_cov = cov;
            for (uint32_t j = 0; j < l.count; j++) a.off[j] = plan.level[l.src + 1 + j].offset;
            a.src_w = src.width; a.src_h = src.height; a.count = l.count; a.tiles_x = (src.width + kTile - 1) / kTile;
            HIP_TRY(launch_lmm_reduce(a, m.channels, stream));
        }
        return MI_OK;
    });
}

// The entry (host: see run_columns): the arguments, the context, the overlaps; one level makes nothing.  Without out_coverage the planes
// still have to exist on the device: the host form stages a column that is neither uploaded nor fetched, the device form uses the
// context's own buffer (one such call at a time).  The launches are planned anew by the context's tuning once the context is known.
static int mips_entry(const char* who, mi_ctx* c, const MipsArgs& m, bool host, void* stream) {
    MipPlan plan;
    MI_TRY(check_mips_args(who, m, &plan));
    if (!c) return fail(MI_ERR_INVALID, "ctx is NULL");
    const size_t texels = (size_t)m.width * m.height, made = (size_t)plan.texels;
    enum { kImage, kValid, kMips, kMipValid, kCov, kScratch };
    static const char kScratchColumn = 0;
    const StageColumn cols[] = { { m.image, texels * m.channels * sizeof(float), Stage::kIn }, { m.valid, texels, Stage::kIn },
                                 { m.out_mips, made * m.channels * sizeof(float), Stage::kOut, "out_mips" },
                                 { m.out_valid, made, Stage::kOut, "out_valid" }, { m.out_coverage, made * sizeof(float), Stage::kOut, "out_coverage" },
                                 { m.out_coverage ? nullptr : &kScratchColumn, made * sizeof(float), Stage::kDevice } };
    return run_columns(who, c, host, stream, cols, plan.levels == 1, [&](void* const* d, hipStream_t s) -> int {
        if (c->tune.lmm_levels_per_launch != kMipFuse) mip_plan(m.width, m.height, m.levels, c->tune.lmm_levels_per_launch, &plan);
        float* cov = (float*)(d[kCov] ? d[kCov] : d[kScratch]);
        if (!cov) {
            MI_TRY(ensure(&c->d_lmm, &c->lmm_bytes, made * sizeof(float)));
            cov = (float*)c->d_lmm;
        }
        MipsArgs dm = m;
        dm.image = (const float*)d[kImage]; dm.valid = (const uint8_t*)d[kValid]; dm.out_mips = (float*)d[kMips];
        dm.out_valid = (uint8_t*)d[kMipValid];
        return mips_device(c, dm, plan, cov, s);
    });
}

extern "C" int mi_lightmap_mips_device(mi_ctx* c, uint32_t width, uint32_t height, uint32_t channels, const float* image, const uint8_t* valid,
                                       uint32_t levels, float* out_mips, uint8_t* out_valid, float* out_coverage, void* stream) {
    return mips_entry("mi_lightmap_mips_device", c, { width, height, channels, image, valid, levels, out_mips, out_valid, out_coverage }, false, stream);
}

extern "C" int mi_lightmap_mips(mi_ctx* c, uint32_t width, uint32_t height, uint32_t channels, const float* image, const uint8_t* valid,
                                uint32_t levels, float* out_mips, uint8_t* out_valid, float* out_coverage) {
    return mips_entry("mi_lightmap_mips", c, { width, height, channels, image, valid, levels, out_mips, out_valid, out_coverage }, true, nullptr);
}

extern "C" int mi_lightmap_sample_lod_device(mi_ctx* c, uint32_t width, uint32_t height, uint32_t channels, const float* image,
                                             const uint8_t* valid, uint32_t levels, const float* mips, const uint8_t* mip_valid, uint32_t n,
                                             const float* uv, const float* lod, uint32_t flags, float* out, float* out_weight, void* stream) {
    if (channels == 0) return fail(MI_ERR_INVALID, "mi_lightmap_sample_lod_device: channels 0 is not 3 or 27");
    return lookup_entry("mi_lightmap_sample_lod_device", c, { 0, channels, Levels::kChain, width, height, image, valid, levels, mips, mip_valid,
                        n, uv, nullptr, lod, flags, out, out_weight }, false, stream);
}

extern "C" int mi_lightmap_sample_lod(mi_ctx* c, uint32_t width, uint32_t height, uint32_t channels, const float* image, const uint8_t* valid,
                                      uint32_t levels, const float* mips, const uint8_t* mip_valid, uint32_t n, const float* uv,
                                      const float* lod, uint32_t flags, float* out, float* out_weight) {
    if (channels == 0) return fail(MI_ERR_INVALID, "mi_lightmap_sample_lod: channels 0 is not 3 or 27");
    return lookup_entry("mi_lightmap_sample_lod", c, { 0, channels, Levels::kChain, width, height, image, valid, levels, mips, mip_valid, n, uv,
                        nullptr, lod, flags, out, out_weight }, true, nullptr);
}

extern "C" int mi_lightmap_sh_sample_lod_device(mi_ctx* c, uint32_t width, uint32_t height, const float* sh, const uint8_t* valid,
                                                uint32_t levels, const float* mips, const uint8_t* mip_valid, uint32_t n, const float* uv,
                                                const float* normals, const float* lod, uint32_t flags, float* out_irradiance,
                                                float* out_weight, void* stream) {
    return lookup_entry("mi_lightmap_sh_sample_lod_device", c, { 0, 0, Levels::kChain, width, height, sh, valid, levels, mips, mip_valid, n, uv,
                        normals, lod, flags, out_irradiance, out_weight }, false, stream);
}

extern "C" int mi_lightmap_sh_sample_lod(mi_ctx* c, uint32_t width, uint32_t height, const float* sh, const uint8_t* valid, uint32_t levels,
                                         const float* mips, const uint8_t* mip_valid, uint32_t n, const float* uv, const float* normals,
                                         const float* lod, uint32_t flags, float* out_irradiance, float* out_weight) {
    return lookup_entry("mi_lightmap_sh_sample_lod", c, { 0, 0, Levels::kChain, width, height, sh, valid, levels, mips, mip_valid, n, uv, normals,
                        lod, flags, out_irradiance, out_weight }, true, nullptr);
}

// ------------------------------------------------------------------ packed lightmaps (f16 and RGB9E5 storage, lookups that read them)
// tracing.py lightmap_pack / lightmap_unpack as lmp_pack<F> / lmp_unpack<F>: a count of texels, whatever their layout.  The packed lookups
// are the lookup above with LookupArgs' format set: the same checks, columns, plan and timing, the lmp_* kernels.
struct PackArgs { uint32_t format, channels; uint64_t n_texels; const void* src; void* dst; bool unpack; };

static int pack_device(mi_ctx* c, const PackArgs& p, hipStream_t stream) {
    LmpArgs a{};
    a.src = p.src; a.dst = p.dst; a.n = p.format == MI_LP_F16 ? p.n_texels * p.channels : p.n_texels;
    return timed(c, stream, [&]() -> int {
        HIP_TRY(launch_lmp_pack(a, p.format, p.unpack, stream));
        return MI_OK;
    });
}

// The entry (host: see run_columns): the arguments, the context, the overlap; no texels launch nothing
static int pack_entry(const char* who, mi_ctx* c, const PackArgs& p, bool host, void* stream) {
    MI_TRY(check_packed_format(who, p.format, p.channels, false));
    if (!p.src || !p.dst) return fail(MI_ERR_INVALID, p.unpack ? "%s: packed and out_texels are required" : "%s: texels and out_packed are required", who);
    if (p.n_texels > (1ull << 32)) return fail(MI_ERR_INVALID, "%s: n_texels %llu is above 2^32", who, (unsigned long long)p.n_texels);
    if (!c) return fail(MI_ERR_INVALID, "ctx is NULL");
    const size_t f32_bytes = (size_t)p.n_texels * p.channels * sizeof(float), packed_bytes = (size_t)p.n_texels * texel_bytes(p.format, p.channels);
    const StageColumn cols[] = { { p.src, p.unpack ? packed_bytes : f32_bytes, Stage::kIn },
                                 { p.dst, p.unpack ? f32_bytes : packed_bytes, Stage::kOut, p.unpack ? "out_texels" : "out_packed" } };
    return run_columns(who, c, host, stream, cols, p.n_texels == 0, [&](void* const* d, hipStream_t s) -> int {
        PackArgs dp = p;
        dp.src = d[0]; dp.dst = d[1];
        return pack_device(c, dp, s);
    });
}

extern "C" int mi_lightmap_pack(mi_ctx* c, uint32_t format, uint32_t channels, uint64_t n_texels, const float* texels, void* out_packed) {
    return pack_entry("mi_lightmap_pack", c, { format, channels, n_texels, texels, out_packed, false }, true, nullptr);
}
extern "C" int mi_lightmap_pack_device(mi_ctx* c, uint32_t format, uint32_t channels, uint64_t n_texels, const float* texels, void* out_packed,
                                       void* stream) {
    return pack_entry("mi_lightmap_pack_device", c, { format, channels, n_texels, texels, out_packed, false }, false, stream);
}
extern "C" int mi_lightmap_unpack(mi_ctx* c, uint32_t format, uint32_t channels, uint64_t n_texels, const void* packed, float* out_texels) {
    return pack_entry("mi_lightmap_unpack", c, { format, channels, n_texels, packed, out_texels, true }, true, nullptr);
}
extern "C" int mi_lightmap_unpack_device(mi_ctx* c, uint32_t format, uint32_t channels, uint64_t n_texels, const void* packed, float* out_texels,
                                         void* stream) {
    return pack_entry("mi_lightmap_unpack_device", c, { format, channels, n_texels, packed, out_texels, true }, false, stream);
}

// The packed lookups: lod != NULL is the trilinear form over the mip plan; lod == NULL the level-0 form, which has no chain.  The format
// is the caller's here (0, f32, is refused: f32 texels take the unpacked calls), so it is checked before anything else.
static int packed_lookup_entry(const char* who, mi_ctx* c, const LookupArgs& l, bool host, void* stream) {
    MI_TRY(check_packed_format(who, l.format, l.channels, l.channels == 0));
    return lookup_entry(who, c, l, host, stream);
}
extern "C" int mi_lightmap_sample_packed(mi_ctx* c, uint32_t format, uint32_t width, uint32_t height, uint32_t channels, const void* image,
                                         const uint8_t* valid, uint32_t levels, const void* mips, const uint8_t* mip_valid, uint32_t n,
                                         const float* uv, const float* lod, uint32_t flags, float* out, float* out_weight) {
    if (channels == 0) return fail(MI_ERR_INVALID, "mi_lightmap_sample_packed: channels 0 is not 3 or 27");
    return packed_lookup_entry("mi_lightmap_sample_packed", c, { format, channels, Levels::kEither, width, height, image, valid, levels, mips, mip_valid,
                        n, uv, nullptr, lod, flags, out, out_weight }, true, nullptr);
}
extern "C" int mi_lightmap_sample_packed_device(mi_ctx* c, uint32_t format, uint32_t width, uint32_t height, uint32_t channels,
                                                const void* image, const uint8_t* valid, uint32_t levels, const void* mips,
                                                const uint8_t* mip_valid, uint32_t n, const float* uv, const float* lod, uint32_t flags,
                                                float* out, float* out_weight, void* stream) {
    if (channels == 0) return fail(MI_ERR_INVALID, "mi_lightmap_sample_packed_device: channels 0 is not 3 or 27");
    return packed_lookup_entry("mi_lightmap_sample_packed_device", c, { format, channels, Levels::kEither, width, height, image, valid, levels, mips,
                        mip_valid, n, uv, nullptr, lod, flags, out, out_weight }, false, stream);
}
extern "C" int mi_lightmap_sh_sample_packed(mi_ctx* c, uint32_t format, uint32_t width, uint32_t height, const void* sh, const uint8_t* valid,
                                            uint32_t levels, const void* mips, const uint8_t* mip_valid, uint32_t n, const float* uv,
                                            const float* normals, const float* lod, uint32_t flags, float* out_irradiance, float* out_weight) {
    return packed_lookup_entry("mi_lightmap_sh_sample_packed", c, { format, 0, Levels::kEither, width, height, sh, valid, levels, mips, mip_valid, n, uv,
                        normals, lod, flags, out_irradiance, out_weight }, true, nullptr);
}
extern "C" int mi_lightmap_sh_sample_packed_device(mi_ctx* c, uint32_t format, uint32_t width, uint32_t height, const void* sh,
                                                   const uint8_t* valid, uint32_t levels, const void* mips, const uint8_t* mip_valid,
                                                   uint32_t n, const float* uv, const float* normals, const float* lod, uint32_t flags,
                                                   float* out_irradiance, float* out_weight, void* stream) {
    return packed_lookup_entry("mi_lightmap_sh_sample_packed_device", c, { format, 0, Levels::kEither, width, height, sh, valid, levels, mips, mip_valid,
                        n, uv, normals, lod, flags, out_irradiance, out_weight }, false, stream);
}

// ------------------------------------------------------------------ BC6H lightmaps (a block encoder, the decoder, the lookup that reads blocks)
// tracing.py lightmap_bc6h_encode / lightmap_bc6h_decode as lmb_encode / lmb_decode, one level per call; the lookup is the lookup above
// with the format kLpBc6h: the same checks, columns, plan and timing, the lmp_* kernels with the block policy.  BC6H is lossy, so it has
// entry points of its own: the MI_LP_* calls keep refusing every format they refused.
struct Bc6hArgs { uint32_t width, height; const float* image; const uint8_t* valid; uint32_t rounds; void* blocks; float* out; bool decode; };

static int bc6h_device(mi_ctx* c, const Bc6hArgs& b, hipStream_t stream) {
    LmbArgs a{};
    a.image = b.image; a.valid = b.valid; a.blocks = b.blocks; a.out = b.out; a.rounds = b.rounds;
    a.width = b.width; a.height = b.height; a.bw = bc6h_extent(b.width); a.bh = bc6h_extent(b.height);
    return timed(c, stream, [&]() -> int {
        HIP_TRY(b.decode ? launch_lmb_decode(a, stream) : launch_lmb_encode(a, c->tune.lmb_lane_per_block != 0, stream));
        return MI_OK;
    });
}

// The entry of the coder (host: see run_columns).  Encoding reads image and valid and writes the blocks; decoding reads the blocks and
// writes out: the columns of the other direction are absent.
static int bc6h_entry(const char* who, mi_ctx* c, const Bc6hArgs& b, bool host, void* stream) {
    if (!b.blocks || (b.decode ? !b.out : !b.image))
        return fail(MI_ERR_INVALID, b.decode ? "%s: blocks and out_image are required" : "%s: image and out_blocks are required", who);
    if (b.width == 0 || b.width > 32768u || b.height == 0 || b.height > 32768u)
        return fail(MI_ERR_INVALID, "%s: width %u / height %u is not in 1 .. 32768", who, b.width, b.height);
    if (b.rounds > kBc6hMaxRounds) return fail(MI_ERR_INVALID, "%s: rounds %u is above %u", who, b.rounds, kBc6hMaxRounds);
    if (!host && ((uintptr_t)b.blocks & 15u)) return fail(MI_ERR_INVALID, "%s: the blocks are not 16-byte aligned", who);
    if (!c) return fail(MI_ERR_INVALID, "ctx is NULL");
    const size_t texels = (size_t)b.width * b.height, f32_bytes = texels * 3 * sizeof(float);
    enum { kImage, kValid, kBlocks, kOut };
    const StageColumn cols[] = { { b.image, f32_bytes, Stage::kIn }, { b.valid, texels, Stage::kIn },
                                 { b.blocks, level_bytes(kLpBc6h, b.width, b.height, 3), b.decode ? Stage::kIn : Stage::kOut, "out_blocks" },
                                 { b.out, f32_bytes, Stage::kOut, "out_image" } };
    return run_columns(who, c, host, stream, cols, false, [&](void* const* d, hipStream_t s) -> int {
        Bc6hArgs db = b;
        db.image = (const float*)d[kImage]; db.valid = (const uint8_t*)d[kValid]; db.blocks = d[kBlocks]; db.out = (float*)d[kOut];
        return bc6h_device(c, db, s);
    });
}

extern "C" int mi_lightmap_bc6h_encode(mi_ctx* c, uint32_t width, uint32_t height, const float* image, const uint8_t* valid, uint32_t rounds,
                                       void* out_blocks) {
    return bc6h_entry("mi_lightmap_bc6h_encode", c, { width, height, image, valid, rounds, out_blocks, nullptr, false }, true, nullptr);
}
extern "C" int mi_lightmap_bc6h_encode_device(mi_ctx* c, uint32_t width, uint32_t height, const float* image, const uint8_t* valid,
                                              uint32_t rounds, void* out_blocks, void* stream) {
    return bc6h_entry("mi_lightmap_bc6h_encode_device", c, { width, height, image, valid, rounds, out_blocks, nullptr, false }, false, stream);
}
extern "C" int mi_lightmap_bc6h_decode(mi_ctx* c, uint32_t width, uint32_t height, const void* blocks, float* out_image) {
    return bc6h_entry("mi_lightmap_bc6h_decode", c, { width, height, nullptr, nullptr, 0, (void*)blocks, out_image, true }, true, nullptr);
}
extern "C" int mi_lightmap_bc6h_decode_device(mi_ctx* c, uint32_t width, uint32_t height, const void* blocks, float* out_image, void* stream) {
    return bc6h_entry("mi_lightmap_bc6h_decode_device", c, { width, height, nullptr, nullptr, 0, (void*)blocks, out_image, true }, false, stream);
}

// The lookup: mi_lightmap_sample_packed's rules word for word, three channels, the texels in blocks
extern "C" int mi_lightmap_sample_bc6h(mi_ctx* c, uint32_t width, uint32_t height, const void* image_blocks, const uint8_t* valid,
                                       uint32_t levels, const void* mip_blocks, const uint8_t* mip_valid, uint32_t n, const float* uv,
                                       const float* lod, uint32_t flags, float* out, float* out_weight) {
    return lookup_entry("mi_lightmap_sample_bc6h", c, { kLpBc6h, 3, Levels::kEither, width, height, image_blocks, valid, levels, mip_blocks,
                        mip_valid, n, uv, nullptr, lod, flags, out, out_weight }, true, nullptr);
}
extern "C" int mi_lightmap_sample_bc6h_device(mi_ctx* c, uint32_t width, uint32_t height, const void* image_blocks, const uint8_t* valid,
                                              uint32_t levels, const void* mip_blocks, const uint8_t* mip_valid, uint32_t n, const float* uv,
                                              const float* lod, uint32_t flags, float* out, float* out_weight, void* stream) {
    return lookup_entry("mi_lightmap_sample_bc6h_device", c, { kLpBc6h, 3, Levels::kEither, width, height, image_blocks, valid, levels,
                        mip_blocks, mip_valid, n, uv, nullptr, lod, flags, out, out_weight }, false, stream);
}

// ------------------------------------------------------------------ variance-guided lightmap finishing
// The variance form of the finish.  The counts forms refuse a missing `counts` before anything else and pass samples = 2 to the checks and
// the kernels: one more form of lmv_init, everything else the same passes.
extern "C" int mi_lightmap_finish_var_device(mi_ctx* c, uint32_t width, uint32_t height, const float* image, const float* m2, uint32_t samples,
                                             const float* points, const float* normals, uint32_t levels, uint32_t normal_power_log2,
                                             float sigma_plane, float reach, float sigma_color, float color_floor, uint32_t dilate,
                                             float* out_image, float* out_var, uint8_t* out_valid, void* stream) {
    const FinishVarArgs fv = { m2, nullptr, samples, color_floor, out_var };
    return finish_entry("mi_lightmap_finish_var_device", FinishForm::kVar, c, { width, height, image, points, normals, levels,
                        normal_power_log2, sigma_plane, reach, sigma_color, dilate, out_image, out_valid }, &fv, false, stream);
}

extern "C" int mi_lightmap_finish_var(mi_ctx* c, uint32_t width, uint32_t height, const float* image, const float* m2, uint32_t samples,
                                      const float* points, const float* normals, uint32_t levels, uint32_t normal_power_log2,
                                      float sigma_plane, float reach, float sigma_color, float color_floor, uint32_t dilate,
                                      float* out_image, float* out_var, uint8_t* out_valid) {
    const FinishVarArgs fv = { m2, nullptr, samples, color_floor, out_var };
    return finish_entry("mi_lightmap_finish_var", FinishForm::kVar, c, { width, height, image, points, normals, levels,
                        normal_power_log2, sigma_plane, reach, sigma_color, dilate, out_image, out_valid }, &fv, true, nullptr);
}

extern "C" int mi_lightmap_finish_var_counts_device(mi_ctx* c, uint32_t width, uint32_t height, const float* image, const float* m2,
                                                    const uint32_t* counts, const float* points, const float* normals, uint32_t levels,
                                                    uint32_t normal_power_log2, float sigma_plane, float reach, float sigma_color,
                                                    float color_floor, uint32_t dilate, float* out_image, float* out_var, uint8_t* out_valid,
                                                    void* stream) {
    if (!counts) return fail(MI_ERR_INVALID, "mi_lightmap_finish_var_counts_device: counts is required");
    const FinishVarArgs fv = { m2, counts, 2, color_floor, out_var };
    return finish_entry("mi_lightmap_finish_var_counts_device", FinishForm::kVar, c, { width, height, image, points, normals, levels,
                        normal_power_log2, sigma_plane, reach, sigma_color, dilate, out_image, out_valid }, &fv, false, stream);
}

extern "C" int mi_lightmap_finish_var_counts(mi_ctx* c, uint32_t width, uint32_t height, const float* image, const float* m2,
                                             const uint32_t* counts, const float* points, const float* normals, uint32_t levels,
                                             uint32_t normal_power_log2, float sigma_plane, float reach, float sigma_color, float color_floor,
                                             uint32_t dilate, float* out_image, float* out_var, uint8_t* out_valid) {
    if (!counts) return fail(MI_ERR_INVALID, "mi_lightmap_finish_var_counts: counts is required");
    const FinishVarArgs fv = { m2, counts, 2, color_floor, out_var };
    return finish_entry("mi_lightmap_finish_var_counts", FinishForm::kVar, c, { width, height, image, points, normals, levels,
                        normal_power_log2, sigma_plane, reach, sigma_color, dilate, out_image, out_valid }, &fv, true, nullptr);
}

// ------------------------------------------------------------------ adaptive lightmap baking (select, gather, merge, the whole bake)
// tracing.py lightmap_select, lightmap_gather and lightmap_merge as kernels, and the bake that composes them with the moments render.
// The arguments are checked before the context, as the finishing pass's are.
static const uint32_t kLmaMaxList = 1u << 25;          // mi_bake_lightmap_adaptive's capacity: 128 MiB of texel numbers
static const uint32_t kLmaCompactWidth = 1024;         // ... and the width of its compact tables

static int check_lma_size(const char* who, uint32_t width, uint32_t height) {
    if (width == 0 || width > 32768u || height == 0 || height > 32768u)
        return fail(MI_ERR_INVALID, "%s: width %u / height %u is not in 1 .. 32768", who, width, height);
    return MI_OK;
}

static int check_select_args(const char* who, uint32_t width, uint32_t height, const float* image, const float* m2, const uint32_t* counts,
                             const float* normals, float target_rel, float target_abs, uint32_t capacity, const uint32_t* out_index,
                             const uint32_t* out_count) {
    if (!image || !m2 || !counts || !normals || !out_count)
        return fail(MI_ERR_INVALID, "%s: image, m2, counts, normals and out_count are required", who);
    if (capacity > 0 && !out_index) return fail(MI_ERR_INVALID, "%s: out_index is required when capacity is not 0", who);
    MI_TRY(check_lma_size(who, width, height));
    if (!(target_rel >= 0.0f)) return fail(MI_ERR_INVALID, "%s: target_rel must be >= 0 and not NaN", who);
    if (!(target_abs >= 0.0f)) return fail(MI_ERR_INVALID, "%s: target_abs must be >= 0 and not NaN (+inf selects nothing)", who);
    return MI_OK;
}

// Queue lmv_init, lma_mark, lma_scan and lma_fill on `stream`; every pointer is a device pointer.  timed: between the context's
// timing events (the public forms; the whole bake keeps the events for its renders).
static int lightmap_select_device(mi_ctx* c, uint32_t width, uint32_t height, const float* d_image, const float* d_m2, const uint32_t* d_counts,
                                  const float* d_normals, float target_rel, float target_abs, uint32_t capacity, uint32_t* d_index,
                                  uint32_t* d_count, float* d_error, hipStream_t stream, bool timed) {
    const size_t n = (size_t)width * height, nb = (n + kLmaBlock - 1) / kLmaBlock;
    const size_t o_flags = up256(n * sizeof(float)), o_counts = o_flags + up256(n), o_offsets = o_counts + up256(nb * 4);
    MI_TRY(ensure(&c->d_lma, &c->lma_bytes, o_offsets + up256(nb * 4)));
    char* const s = (char*)c->d_lma;
    LmvArgs v{};
    v.src = d_image; v.m2 = d_m2; v.normals = d_normals; v.var_out = (float*)s;
    v.width = width; v.height = height;
    LmaArgs a{};
    a.image = d_image; a.normals = d_normals; a.var = (const float*)s; a.error = d_error;
    a.flags = (uint8_t*)(s + o_flags); a.block_counts = (uint32_t*)(s + o_counts); a.block_offsets = (uint32_t*)(s + o_offsets);
    a.out_index = d_index; a.out_count = d_count;
    a.width = width; a.height = height; a.blocks = (uint32_t)nb; a.capacity = capacity;
    a.target_rel = target_rel; a.target_abs = target_abs;
    auto queue = [&]() -> int {
        HIP_TRY(launch_lmv_init(v, d_counts, true, stream));
        HIP_TRY(launch_lma_select(a, stream));
        return MI_OK;
    };
    return timed ? ::timed(c, stream, queue) : queue();          // (the helper, which the parameter hides)
}

extern "C" int mi_lightmap_select_device(mi_ctx* c, uint32_t width, uint32_t height, const float* image, const float* m2,
                                         const uint32_t* counts, const float* normals, float target_rel, float target_abs, uint32_t capacity,
                                         uint32_t* out_index, uint32_t* out_count, float* out_error, void* stream) {
    MI_TRY(check_select_args("mi_lightmap_select_device", width, height, image, m2, counts, normals, target_rel, target_abs, capacity,
                             out_index, out_count));
    if (!c) return fail(MI_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    return lightmap_select_device(c, width, height, image, m2, counts, normals, target_rel, target_abs, capacity, out_index, out_count,
                                  out_error, (hipStream_t)stream, true);
}

extern "C" int mi_lightmap_select(mi_ctx* c, uint32_t width, uint32_t height, const float* image, const float* m2, const uint32_t* counts,
                                  const float* normals, float target_rel, float target_abs, uint32_t capacity, uint32_t* out_index,
                                  uint32_t* out_count, float* out_error) {
    MI_TRY(check_select_args("mi_lightmap_select", width, height, image, m2, counts, normals, target_rel, target_abs, capacity, out_index,
                             out_count));
    if (!c) return fail(MI_ERR_INVALID, "ctx is NULL");
    // The list (no longer than the atlas) stays on the device: only the entries the count says were written are copied out afterwards, so
    // that the entries behind them stay unwritten in the caller's array.
    const size_t n = (size_t)width * height;
    const uint32_t cap = (uint32_t)std::min<size_t>(capacity, n);
    uint32_t count = 0;
    const void* d_list = nullptr;
    enum { kImage, kM2, kNormals, kCounts, kCount, kError, kList };
    const StageColumn cols[] = { { image, n * 12, Stage::kIn }, { m2, n * 12, Stage::kIn }, { normals, n * 12, Stage::kIn },
                                 { counts, n * 4, Stage::kIn }, { &count, 4, Stage::kOut }, { out_error, n * 4, Stage::kOut },
                                 { out_index, (size_t)cap * 4, Stage::kDevice } };
    MI_TRY(staged(c, cols, [&](void* const* d) -> int {
        d_list = d[kList];
        return lightmap_select_device(c, width, height, (const float*)d[kImage], (const float*)d[kM2], (const uint32_t*)d[kCounts],
                                      (const float*)d[kNormals], target_rel, target_abs, cap, (uint32_t*)d[kList], (uint32_t*)d[kCount],
                                      (float*)d[kError], c->stream, true);
    }));
    const uint32_t held = std::min(count, cap);            // the entries behind them are not written
    if (held) HIP_TRY(hipMemcpy(out_index, d_list, (size_t)held * 4, hipMemcpyDeviceToHost));
    *out_count = count;
    return MI_OK;
}

static int check_gather_args(const char* who, uint32_t width, uint32_t height, uint32_t rows, uint32_t n, const uint32_t* index,
                             const float* points, const float* normals, uint32_t cw, const float* out_points, const float* out_normals) {
    if (!index || !points || !normals || !out_points || !out_normals)
        return fail(MI_ERR_INVALID, "%s: index, points, normals, out_points and out_normals are required", who);
    MI_TRY(check_lma_size(who, width, height));
    if (rows == 0 || rows > 65535u) return fail(MI_ERR_INVALID, "%s: rows %u is not in 1 .. 65535", who, rows);
    if (cw == 0 || cw > 32768u) return fail(MI_ERR_INVALID, "%s: cw %u is not in 1 .. 32768", who, cw);
    const uint64_t ch = ((uint64_t)n + cw - 1) / cw;
    if (ch == 0 || ch > 32768u)
        return fail(MI_ERR_INVALID, "%s: n %u entries at cw %u give %llu rows of slots: not in 1 .. 32768", who, n, cw, (unsigned long long)ch);
    return MI_OK;
}

static LmaListArgs gather_args(uint32_t width, uint32_t height, uint32_t rows, uint32_t n, const uint32_t* d_index, const float* d_points,
                               const float* d_normals, uint32_t cw, float* d_out_points, float* d_out_normals) {
    LmaListArgs a{};
    a.index = d_index; a.n = n; a.width = width; a.height = height;
    a.points = d_points; a.normals = d_normals; a.out_points = d_out_points; a.out_normals = d_out_normals;
    a.rows = rows; a.slots = (n + cw - 1) / cw * cw;
    return a;
}

// lma_gather on `stream` between the context's timing events; every pointer is a device pointer
static int lightmap_gather_device(mi_ctx* c, uint32_t width, uint32_t height, uint32_t rows, uint32_t n, const uint32_t* d_index,
                                  const float* d_points, const float* d_normals, uint32_t cw, float* d_out_points, float* d_out_normals,
                                  hipStream_t stream) {
    return timed(c, stream, [&]() -> int {
        HIP_TRY(launch_lma_gather(gather_args(width, height, rows, n, d_index, d_points, d_normals, cw, d_out_points, d_out_normals), stream));
        return MI_OK;
    });
}

extern "C" int mi_lightmap_gather_device(mi_ctx* c, uint32_t width, uint32_t height, uint32_t rows, uint32_t n, const uint32_t* index,
                                         const float* points, const float* normals, uint32_t cw, float* out_points, float* out_normals,
                                         void* stream) {
    MI_TRY(check_gather_args("mi_lightmap_gather_device", width, height, rows, n, index, points, normals, cw, out_points, out_normals));
    if (!c) return fail(MI_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    return lightmap_gather_device(c, width, height, rows, n, index, points, normals, cw, out_points, out_normals, (hipStream_t)stream);
}

extern "C" int mi_lightmap_gather(mi_ctx* c, uint32_t width, uint32_t height, uint32_t rows, uint32_t n, const uint32_t* index,
                                  const float* points, const float* normals, uint32_t cw, float* out_points, float* out_normals) {
    MI_TRY(check_gather_args("mi_lightmap_gather", width, height, rows, n, index, points, normals, cw, out_points, out_normals));
    if (!c) return fail(MI_ERR_INVALID, "ctx is NULL");
    // the list, the two source tables, the two compact tables
    const size_t tab = (size_t)rows * width * height * 12, slots = ((size_t)n + cw - 1) / cw * cw, out = (size_t)rows * slots * 12;
    const StageColumn cols[] = { { index, (size_t)n * 4, Stage::kIn }, { points, tab, Stage::kIn }, { normals, tab, Stage::kIn },
                                 { out_points, out, Stage::kOut }, { out_normals, out, Stage::kOut } };
    return staged(c, cols, [&](void* const* d) -> int {
        return lightmap_gather_device(c, width, height, rows, n, (const uint32_t*)d[0], (const float*)d[1], (const float*)d[2], cw,
                                      (float*)d[3], (float*)d[4], c->stream);
    });
}

static int check_merge_args(const char* who, uint32_t width, uint32_t height, uint32_t n, const uint32_t* index, const float* mean,
                            const float* m2_round, uint32_t round_samples, const float* image, const float* m2, const uint32_t* counts) {
    if (!index || !mean || !m2_round || !image || !m2 || !counts)
        return fail(MI_ERR_INVALID, "%s: index, mean, m2_round, image, m2 and counts are required", who);
    MI_TRY(check_lma_size(who, width, height));
    if (round_samples == 0 || round_samples > 65535u) return fail(MI_ERR_INVALID, "%s: round_samples %u is not in 1 .. 65535", who, round_samples);
    return MI_OK;
}

static LmaListArgs merge_args(uint32_t width, uint32_t height, uint32_t n, const uint32_t* d_index, const float* d_mean, const float* d_m2_round,
                              uint32_t round_samples, float* d_image, float* d_m2, uint32_t* d_counts) {
    LmaListArgs a{};
    a.index = d_index; a.n = n; a.width = width; a.height = height;
    a.mean = d_mean; a.m2_round = d_m2_round; a.image = d_image; a.m2 = d_m2; a.counts = d_counts; a.round_samples = round_samples;
    return a;
}

// lma_merge on `stream` between the context's timing events; every pointer is a device pointer.  n == 0 launches nothing, and still
// records the events.
static int lightmap_merge_device(mi_ctx* c, uint32_t width, uint32_t height, uint32_t n, const uint32_t* d_index, const float* d_mean,
                                 const float* d_m2_round, uint32_t round_samples, float* d_image, float* d_m2, uint32_t* d_counts,
                                 hipStream_t stream) {
    return timed(c, stream, [&]() -> int {
        if (n) HIP_TRY(launch_lma_merge(merge_args(width, height, n, d_index, d_mean, d_m2_round, round_samples, d_image, d_m2, d_counts), stream));
        return MI_OK;
    });
}

extern "C" int mi_lightmap_merge_device(mi_ctx* c, uint32_t width, uint32_t height, uint32_t n, const uint32_t* index, const float* mean,
                                        const float* m2_round, uint32_t round_samples, float* image, float* m2, uint32_t* counts,
                                        void* stream) {
    MI_TRY(check_merge_args("mi_lightmap_merge_device", width, height, n, index, mean, m2_round, round_samples, image, m2, counts));
    if (!c) return fail(MI_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    return lightmap_merge_device(c, width, height, n, index, mean, m2_round, round_samples, image, m2, counts, (hipStream_t)stream);
}

extern "C" int mi_lightmap_merge(mi_ctx* c, uint32_t width, uint32_t height, uint32_t n, const uint32_t* index, const float* mean,
                                 const float* m2_round, uint32_t round_samples, float* image, float* m2, uint32_t* counts) {
    MI_TRY(check_merge_args("mi_lightmap_merge", width, height, n, index, mean, m2_round, round_samples, image, m2, counts));
    {   // one lane per entry: a texel listed twice would be merged by two lanes at once
        std::vector<uint32_t> seen;
        seen.reserve(n);
        for (uint32_t i = 0; i < n; i++) if (index[i] < (uint64_t)width * height) seen.push_back(index[i]);
        std::sort(seen.begin(), seen.end());
        const auto dup = std::adjacent_find(seen.begin(), seen.end());
        if (dup != seen.end()) return fail(MI_ERR_INVALID, "mi_lightmap_merge: the list holds texel %u twice", *dup);
    }
    if (!c) return fail(MI_ERR_INVALID, "ctx is NULL");
    // the list, the round's two tables, the three planes (which make the round trip with n == 0 too)
    const size_t npix = (size_t)width * height;
    const StageColumn cols[] = { { index, (size_t)n * 4, Stage::kIn }, { mean, (size_t)n * 12, Stage::kIn }, { m2_round, (size_t)n * 12, Stage::kIn },
                                 { image, npix * 12, Stage::kInOut }, { m2, npix * 12, Stage::kInOut }, { counts, npix * 4, Stage::kInOut } };
    return staged(c, cols, [&](void* const* d) -> int {
        return lightmap_merge_device(c, width, height, n, (const uint32_t*)d[0], (const float*)d[1], (const float*)d[2], round_samples,
                                     (float*)d[3], (float*)d[4], (uint32_t*)d[5], c->stream);
    });
}

// The whole bake: mi_bake_lightmap_moments' body for round 0, then per round select, gather, the moments render of the compact table and
// merge, all on the context's stream, the planes never leaving the device; one word (the list's length) comes back per round.
extern "C" int mi_bake_lightmap_adaptive(mi_ctx* c, const mi_camera_desc* cam, const mi_render_opts* opts, const mi_mesh* mesh, uint32_t flags,
                                         float offset, const mi_lightmap_adaptive* adaptive, uint32_t* out_counts, float* out_m2,
                                         float* out_rgb_f32, uint8_t* out_rgb_u8, uint32_t* out_sig, int32_t* out_triangle, mi_stats* stats) {
    const char* const who = "mi_bake_lightmap_adaptive";
    if (!out_m2 || !out_counts) return fail(MI_ERR_INVALID, "%s: out_m2 and out_counts are required", who);
    if (!adaptive) return fail(MI_ERR_INVALID, "%s: adaptive is NULL", who);
    const mi_lightmap_adaptive ad = *adaptive;
    if (ad.first_samples < 2 || ad.first_samples > 65535u)
        return fail(MI_ERR_INVALID, "%s: first_samples %u is not in 2 .. 65535", who, ad.first_samples);
    if (ad.round_samples == 0 || ad.round_samples > 65535u)
        return fail(MI_ERR_INVALID, "%s: round_samples %u is not in 1 .. 65535", who, ad.round_samples);
    if ((uint64_t)ad.first_samples + (uint64_t)ad.max_rounds * ad.round_samples > (1ull << 24))
        return fail(MI_ERR_INVALID, "%s: first_samples + max_rounds * round_samples exceeds 2^24 (a count must stay exact in f32)", who);
    if (!(ad.target_rel >= 0.0f) || !(ad.target_abs >= 0.0f))
        return fail(MI_ERR_INVALID, "%s: target_rel and target_abs must be >= 0 and not NaN", who);
    if (!c) return fail(MI_ERR_INVALID, "ctx is NULL");
    if (!cam) return fail(MI_ERR_INVALID, "%s: cam is NULL", who);
    // round 0: mi_bake_lightmap_moments at first_samples (every refusal of that call happens in here, before anything is launched)
    mi_camera_desc cam0 = *cam;
    cam0.aa_sample_count = ad.first_samples;
    mi_stats st0;
    MI_TRY(bake_lightmap(who, c, &cam0, opts, mesh, flags, offset, nullptr, nullptr, out_sig, out_triangle, &st0, out_m2));
    const uint32_t W = cam->screen_width, H = cam->screen_height;
    const size_t n = (size_t)W * H, img = up256(n * 3 * sizeof(float)), pln = up256(n * 4);
    const bool jitter = (flags & MI_LM_JITTER) != 0;
    // the running planes: mean, m2, the centre table's normals and points, the counts, the bytes
    MI_TRY(ensure(&c->d_lma_bake, &c->lma_bake_bytes, 4 * img + pln + up256(n * 3)));
    char* const b = (char*)c->d_lma_bake;
    float* const d_mean = (float*)b; float* const d_m2 = (float*)(b + img);
    float* const d_cn = (float*)(b + 2 * img); float* const d_cp = (float*)(b + 3 * img);
    uint32_t* const d_counts = (uint32_t*)(b + 4 * img); uint8_t* const d_u8 = (uint8_t*)(b + 4 * img + pln);
    const size_t m2_plane = (size_t)tile_grid(&cam0, 1).padded * kTilePixels * 3;        // render_image un-permuted the moments there
    HIP_TRY(hipEventRecord(c->ev_t0, c->stream));
    HIP_TRY(hipMemcpyAsync(d_mean, c->d_image, n * 12, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_m2, (const float*)c->d_m2 + m2_plane, n * 12, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)d_counts, (int)ad.first_samples, n, c->stream));
    uint64_t samples = st0.samples;
    float kernel_ms = st0.kernel_ms;
    if (ad.max_rounds > 0) {
        mi_mesh dev;
        MI_TRY(upload_lm_mesh(c, mesh, &dev));
        MI_TRY(lightmap_texels_device(c, &dev, W, H, 1, 0, opts->seed, offset, d_cp, d_cn, nullptr, c->stream, true));
        const uint32_t cap = (uint32_t)std::min<size_t>(kLmaMaxList, n);
        MI_TRY(ensure(&c->d_lma_list, &c->lma_list_bytes, 256 + (size_t)cap * 4));
        uint32_t* const d_count = (uint32_t*)c->d_lma_list; uint32_t* const d_list = (uint32_t*)((char*)c->d_lma_list + 256);
        for (uint32_t r = 1; r <= ad.max_rounds; r++) {
            MI_TRY(lightmap_select_device(c, W, H, d_mean, d_m2, d_counts, d_cn, ad.target_rel, ad.target_abs, cap, d_list, d_count, nullptr,
                                          c->stream, false));
            uint32_t count = 0;
            HIP_TRY(hipMemcpyAsync(&count, d_count, 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            if (count == 0) break;
            const uint32_t nsel = std::min(count, cap), cw = kLmaCompactWidth, ch = (nsel + cw - 1) / cw, rows = jitter ? ad.round_samples : 1u;
            const size_t slots = (size_t)cw * ch;
            const float* d_sp = d_cp; const float* d_sn = d_cn;
            if (jitter) {           // a fresh table of the whole atlas, in the table buffer round 0 is done with
                const size_t bytes = (size_t)rows * n * 3 * sizeof(float);
                MI_TRY(ensure(&c->d_rays, &c->rays_bytes, 2 * bytes));
                float* d_jp = (float*)c->d_rays; float* d_jn = (float*)((char*)c->d_rays + bytes);
                MI_TRY(lightmap_texels_device(c, &dev, W, H, rows, MI_LM_JITTER, opts->seed + r, offset, d_jp, d_jn, nullptr, c->stream, true));
                d_sp = d_jp; d_sn = d_jn;
            }
            mi_camera_desc camr = *cam;
            camr.screen_width = cw; camr.screen_height = ch; camr.aa_sample_count = ad.round_samples;
            const TileGrid g = tile_grid(&camr, 1);
            // the round's compact tables, its compact results (mean, moments) and their two [ch][cw][3] planes
            const size_t tab = up256((size_t)rows * slots * 12), cmp = up256((size_t)g.padded * kTilePixels * 12), rpl = up256(slots * 12);
            MI_TRY(ensure(&c->d_lma_round, &c->lma_round_bytes, 2 * tab + 2 * cmp + 2 * rpl));
            char* const q = (char*)c->d_lma_round;
            float* const d_tp = (float*)q; float* const d_tn = (float*)(q + tab);
            float* const d_rc = (float*)(q + 2 * tab); float* const d_rm = (float*)(q + 2 * tab + cmp);
            float* const d_pmean = (float*)(q + 2 * tab + 2 * cmp); float* const d_pm2 = (float*)(q + 2 * tab + 2 * cmp + rpl);
            HIP_TRY(launch_lma_gather(gather_args(W, H, rows, nsel, d_list, d_sp, d_sn, cw, d_tp, d_tn), c->stream));
            mi_render_opts o = *opts;
            o.seed = opts->seed + r; o.want_signature = 0;
            const RayTable table = { d_tp, d_tn, rows, kTablePoints, nullptr, d_rm };
            const mi_camera_desc tc = table_camera(&camr);
            mi_stats st;
            MI_TRY(render_tiles(c, &tc, &o, d_rc, nullptr, c->stream, &st, nullptr, &table));
            HIP_TRY(launch_unpermute(d_rc, d_pmean, cw, ch, g.tx, 1, g.padded, c->stream));
            HIP_TRY(launch_unpermute(d_rm, d_pm2, cw, ch, g.tx, 1, g.padded, c->stream));
            HIP_TRY(launch_lma_merge(merge_args(W, H, nsel, d_list, d_pmean, d_pm2, ad.round_samples, d_mean, d_m2, d_counts), c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, c->ev_start, c->ev_stop));
            kernel_ms += ms; samples += st.samples;
        }
    }
    HIP_TRY(hipMemcpyAsync(out_m2, d_m2, n * 12, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(out_counts, d_counts, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (out_rgb_f32) HIP_TRY(hipMemcpyAsync(out_rgb_f32, d_mean, n * 12, hipMemcpyDeviceToHost, c->stream));
    if (out_rgb_u8) {
        HIP_TRY(launch_tonemap(d_mean, d_u8, (uint32_t)n, 1.0f / cam->gamma, c->stream));
        HIP_TRY(hipMemcpyAsync(out_rgb_u8, d_u8, n * 3, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipEventRecord(c->ev_t1, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (stats) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev_t0, c->ev_t1));
        *stats = st0;
        stats->samples = samples; stats->kernel_ms = kernel_ms; stats->total_ms = st0.total_ms + ms;
    }
    return MI_OK;
}

// ------------------------------------------------------------------ irradiance volumes (SH L2 probe grids sampled at surface points)
// tracing.py probe_volume_sample as two kernels: pv_prepare (one 112-byte record per probe) and pv_sample (one lane per point).  The
// arguments are checked before the context, as the finishing pass's are.
static int check_pv_args(const char* who, mi_ctx* c, const mi_probe_volume* v, const float* points, const float* normals,
                         const float* out_irradiance) {
    if (!v) return fail(MI_ERR_INVALID, "%s: volume is NULL", who);
    if (!v->sh || !points || !normals || !out_irradiance)
        return fail(MI_ERR_INVALID, "%s: volume->sh, points, normals and out_irradiance are required", who);
    uint64_t n_probes = 1;
    for (int a = 0; a < 3; a++) {
        if (v->counts[a] == 0 || v->counts[a] > kPvMaxCount)
            return fail(MI_ERR_INVALID, "%s: counts[%d] = %u is not in 1 .. %u", who, a, v->counts[a], kPvMaxCount);
        n_probes *= v->counts[a];
    }
    if (n_probes > kPvMaxProbes) return fail(MI_ERR_INVALID, "%s: %llu probes exceed 2^22", who, (unsigned long long)n_probes);
    if (v->flags & ~(uint32_t)MI_PV_NORMAL_WEIGHT)
        return fail(MI_ERR_INVALID, "%s: unknown flag bits 0x%x", who, v->flags & ~(uint32_t)MI_PV_NORMAL_WEIGHT);
    for (int a = 0; a < 3; a++) {
        if (!std::isfinite(v->lo[a]) || !std::isfinite(v->hi[a])) return fail(MI_ERR_INVALID, "%s: lo[%d] / hi[%d] is not finite", who, a, a);
        if (!(v->hi[a] > v->lo[a])) return fail(MI_ERR_INVALID, "%s: hi[%d] = %g is not above lo[%d] = %g", who, a, v->hi[a], a, v->lo[a]);
    }
    if (!c) return fail(MI_ERR_INVALID, "ctx is NULL");
    return MI_OK;
}

// The volume's part of the kernel arguments: the grid constants in f32, as the helper computes them
static PvArgs pv_volume_args(const mi_probe_volume* v) {
    PvArgs a{};
    a.n_probes = v->counts[0] * v->counts[1] * v->counts[2];
    a.normal_weight = (v->flags & MI_PV_NORMAL_WEIGHT) ? 1u : 0u;
    for (int k = 0; k < 3; k++) {
        const float extent = v->hi[k] - v->lo[k], n = (float)v->counts[k];
        a.counts[k] = v->counts[k]; a.lo[k] = v->lo[k];
        a.cell[k] = extent / n; a.inv[k] = n / extent;
    }
    return a;
}

static size_t pv_record_bytes(uint32_t n_probes) { return (size_t)n_probes * kPvRecordFloats * sizeof(float); }

extern "C" int mi_probe_volume_sample_device(mi_ctx* c, const mi_probe_volume* v, uint32_t n_points, const float* points, const float* normals,
                                             float* out_irradiance, float* out_weight, void* stream) {
    MI_TRY(check_pv_args("mi_probe_volume_sample_device", c, v, points, normals, out_irradiance));
    if (n_points == 0) return MI_OK;
    HIP_TRY(hipSetDevice(c->device));
    PvArgs a = pv_volume_args(v);
    MI_TRY(ensure(&c->d_pv, &c->pv_bytes, pv_record_bytes(a.n_probes)));
    a.sh = v->sh; a.valid = v->valid; a.records = (float*)c->d_pv;
    a.n_points = n_points; a.points = points; a.normals = normals; a.out_irradiance = out_irradiance; a.out_weight = out_weight;
    const hipStream_t s = (hipStream_t)stream;
    return timed(c, s, [&]() -> int {
        HIP_TRY(launch_pv_prepare(a, s));
        HIP_TRY(launch_pv_sample(a, s));
        return MI_OK;
    });
}

extern "C" int mi_probe_volume_sample(mi_ctx* c, const mi_probe_volume* v, uint32_t n_points, const float* points, const float* normals,
                                      float* out_irradiance, float* out_weight) {
    MI_TRY(check_pv_args("mi_probe_volume_sample", c, v, points, normals, out_irradiance));
    if (n_points == 0) return MI_OK;
    HIP_TRY(hipSetDevice(c->device));
    PvArgs a = pv_volume_args(v);
    // the records, then the caller's sh and valid as uploaded (both offsets are multiples of 16)
    const size_t rec = pv_record_bytes(a.n_probes), sh_bytes = (size_t)a.n_probes * 27 * sizeof(float);
    MI_TRY(ensure(&c->d_pv, &c->pv_bytes, rec + sh_bytes + a.n_probes));
    char* const base = (char*)c->d_pv;
    HIP_TRY(hipMemcpyAsync(base + rec, v->sh, sh_bytes, hipMemcpyHostToDevice, c->stream));
    if (v->valid) HIP_TRY(hipMemcpyAsync(base + rec + sh_bytes, v->valid, a.n_probes, hipMemcpyHostToDevice, c->stream));
    a.records = (float*)base; a.sh = (const float*)(base + rec); a.valid = v->valid ? (const uint8_t*)(base + rec + sh_bytes) : nullptr;
    // chunked over points; the first chunk's timed region holds the record pass as well
    const RqColumn cols[] = { { points, 12, false }, { normals, 12, false }, { out_irradiance, 12, true }, { out_weight, 4, true } };
    return rq_chunked(c, n_points, cols, [&](uint32_t first, uint32_t n, void* const* d) {
        a.n_points = n; a.points = (const float*)d[0]; a.normals = (const float*)d[1];
        a.out_irradiance = (float*)d[2]; a.out_weight = (float*)d[3];
        return timed(c, c->stream, [&]() -> int {
            if (first == 0) HIP_TRY(launch_pv_prepare(a, c->stream));
            HIP_TRY(launch_pv_sample(a, c->stream));
            return MI_OK;
        });
    });
}

// ------------------------------------------------------------------ light probes (SH L2 radiance probes: the directions are drawn on the GPU)
// mi_render_points without normals and with a second output: the camera pass draws a full-sphere direction per sample (the PROBES form of
// wf_main) and wf_reduce_sh, behind wf_reduce in every batch, weights the same samples by the SH basis of their directions.  Same checks,
// same upload buffer, same body; the plain outputs are the unchanged wf_reduce's.
extern "C" int mi_render_probes(mi_ctx* c, const mi_camera_desc* cam, const mi_render_opts* opts, const float* points, uint32_t rows_per_pixel,
                                float* out_sh, float* out_rgb_f32, uint8_t* out_rgb_u8, uint32_t* out_sig, mi_stats* stats) {
    return render_table_host(c, cam, opts, points, nullptr, rows_per_pixel, kTableProbes, "mi_render_probes", out_rgb_f32, out_rgb_u8, out_sig,
                             stats, out_sh);
}

extern "C" int mi_render_probes_device(mi_ctx* c, const mi_camera_desc* cam, const mi_render_opts* opts, const float* d_points,
                                       uint32_t rows_per_pixel, uint32_t sample_begin, uint32_t sample_end, void* d_accum_f32x4,
                                       void* d_compact_sh, void* d_compact_f32, void* d_sig_u32, void* stream, mi_stats* stats) {
    return render_table_device(c, cam, opts, d_points, nullptr, rows_per_pixel, kTableProbes, sample_begin, sample_end, d_accum_f32x4,
                               d_compact_f32, d_sig_u32, stream, stats, d_compact_sh);
}

// ------------------------------------------------------------------ multi-GPU behind the ABI
// One process drives N devices: one mi_ctx, one stream and (per frame) one host thread per device, the image cut into
// 32x32 tiles with tile t on device t mod N (the partition of dist.py), and exactly ONE exchange per frame: every peer
// SENDS its compact tile buffer to device 0 over its own xGMI link (RCCL ncclSend / ncclRecv inside one group: a fan-in,
// not a ring — xGMI is point-to-point, 7 links per GPU, so the 7 transfers of 3.1 MB run side by side), then K3 + K4 on
// device 0.  RCCL is resolved at run time (dlopen), so single-GPU users of this library do not need it installed.
#include <dlfcn.h>
#include <rccl/rccl.h>

namespace {
struct Rccl {
    void* so = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    bool load(std::string* why) {
        if (so) return true;
        const char* names[] = { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" };
        for (const char* n : names) { so = dlopen(n, RTLD_NOW | RTLD_LOCAL); if (so) break; }
        if (!so) { *why = std::string("cannot load RCCL: ") + (dlerror() ? dlerror() : "?"); return false; }
#define RCCL_SYM(field, name) field = (decltype(field))dlsym(so, name); if (!field) { *why = std::string("RCCL lacks ") + name; return false; }
        RCCL_SYM(CommInitAll, "ncclCommInitAll"); RCCL_SYM(CommDestroy, "ncclCommDestroy"); RCCL_SYM(GroupStart, "ncclGroupStart");
        RCCL_SYM(GroupEnd, "ncclGroupEnd"); RCCL_SYM(Send, "ncclSend"); RCCL_SYM(Recv, "ncclRecv"); RCCL_SYM(GetErrorString, "ncclGetErrorString");
#undef RCCL_SYM
        return true;
    }
};
Rccl g_rccl;
}  // namespace

struct mi_multi {
    std::vector<int> devices;
    std::vector<mi_ctx*> ctx;
    std::vector<ncclComm_t> comm;
    // device 0: gathered[world][tiles_padded][1024][3] (its own share is rendered straight into slice 0);
    // every other device: its compact buffer.  Signatures likewise.
    std::vector<void*> d_compact; std::vector<size_t> compact_bytes;
    std::vector<void*> d_sig; std::vector<size_t> sig_bytes;
    void* d_sig_image = nullptr; size_t sig_image_bytes = 0;
    // test transport (mi_multi_create_loopback): every rank on ONE device, no RCCL; the exchange is a D2D copy per peer on the
    // peer's stream, ordered into device 0's stream by ev_sent[r]
    bool loopback = false;
    std::vector<hipEvent_t> ev_sent;
};

#define RCCL_TRY(expr)                                                                              \
    do {                                                                                            \
        ncclResult_t r_ = (expr);                                                                   \
        if (r_ != ncclSuccess) return fail(MI_ERR_HIP, "%s failed: %s", #expr, g_rccl.GetErrorString(r_)); \
    } while (0)

extern "C" void mi_multi_destroy(mi_multi* m) {
    if (!m) return;
    for (size_t r = 0; r < m->ctx.size(); r++) {
        if (!m->ctx[r]) continue;
        (void)hipSetDevice(m->devices[r]);
        (void)hipDeviceSynchronize();
        if (r < m->comm.size() && m->comm[r]) (void)g_rccl.CommDestroy(m->comm[r]);
        if (r < m->ev_sent.size() && m->ev_sent[r]) (void)hipEventDestroy(m->ev_sent[r]);
        if (r < m->d_compact.size() && m->d_compact[r]) (void)hipFree(m->d_compact[r]);
        if (r < m->d_sig.size() && m->d_sig[r]) (void)hipFree(m->d_sig[r]);
        if (r == 0 && m->d_sig_image) (void)hipFree(m->d_sig_image);
        mi_ctx_destroy(m->ctx[r]);
    }
    delete m;
}

extern "C" int mi_multi_create(int n_devices, const int* devices, mi_multi** out) {
    if (!out) return fail(MI_ERR_INVALID, "mi_multi_create: out is NULL");
    *out = nullptr;
    if (n_devices < 1 || n_devices > 64) return fail(MI_ERR_INVALID, "mi_multi_create: n_devices %d out of range", n_devices);
    mi_multi* m = new mi_multi();
    for (int r = 0; r < n_devices; r++) {
        m->devices.push_back(devices ? devices[r] : r);
        for (int q = 0; q < r; q++) if (m->devices[(size_t)q] == m->devices[(size_t)r]) {
            const int dup = m->devices[(size_t)r];
            delete m;
            return fail(MI_ERR_INVALID, "mi_multi_create: device %d listed twice", dup);
        }
    }
    m->ctx.assign((size_t)n_devices, nullptr); m->comm.assign((size_t)n_devices, nullptr);
    m->d_compact.assign((size_t)n_devices, nullptr); m->compact_bytes.assign((size_t)n_devices, 0);
    m->d_sig.assign((size_t)n_devices, nullptr); m->sig_bytes.assign((size_t)n_devices, 0);
    for (int r = 0; r < n_devices; r++) {
        const int rc = mi_ctx_create(m->devices[(size_t)r], &m->ctx[(size_t)r]);
        if (rc != MI_OK) { const std::string msg = g_err; mi_multi_destroy(m); g_err = msg; return rc; }
    }
    std::string why;
    if (!g_rccl.load(&why)) { mi_multi_destroy(m); return fail(MI_ERR_UNSUPPORTED, "%s", why.c_str()); }
    const ncclResult_t r = g_rccl.CommInitAll(m->comm.data(), n_devices, m->devices.data());
    if (r != ncclSuccess) {
        for (auto& cm : m->comm) cm = nullptr;
        mi_multi_destroy(m);
        return fail(MI_ERR_HIP, "ncclCommInitAll(%d devices) failed: %s", n_devices, g_rccl.GetErrorString(r));
    }
    *out = m;
    return MI_OK;
}

extern "C" int mi_multi_create_loopback(int n_contexts, int device, mi_multi** out) {
    if (!out) return fail(MI_ERR_INVALID, "mi_multi_create_loopback: out is NULL");
    *out = nullptr;
    if (n_contexts < 1 || n_contexts > 64) return fail(MI_ERR_INVALID, "mi_multi_create_loopback: n_contexts %d out of range", n_contexts);
    mi_multi* m = new mi_multi();
    m->loopback = true;
    m->devices.assign((size_t)n_contexts, device);
    m->ctx.assign((size_t)n_contexts, nullptr); m->ev_sent.assign((size_t)n_contexts, nullptr);
    m->d_compact.assign((size_t)n_contexts, nullptr); m->compact_bytes.assign((size_t)n_contexts, 0);
    m->d_sig.assign((size_t)n_contexts, nullptr); m->sig_bytes.assign((size_t)n_contexts, 0);
    for (int r = 0; r < n_contexts; r++) {
        int rc = mi_ctx_create(device, &m->ctx[(size_t)r]);
        if (rc == MI_OK && hipEventCreateWithFlags(&m->ev_sent[(size_t)r], hipEventDisableTiming) != hipSuccess)
            rc = fail(MI_ERR_HIP, "hipEventCreateWithFlags failed");
        if (rc != MI_OK) { const std::string msg = g_err; mi_multi_destroy(m); g_err = msg; return rc; }
    }
    *out = m;
    return MI_OK;
}

extern "C" int mi_multi_device_count(const mi_multi* m) { return m ? (int)m->ctx.size() : 0; }
extern "C" mi_ctx* mi_multi_context(const mi_multi* m, int rank) {
    if (!m || rank < 0 || (size_t)rank >= m->ctx.size()) { (void)fail(MI_ERR_INVALID, "mi_multi_context: rank %d out of range", rank); return nullptr; }
    return m->ctx[(size_t)rank];
}

// Run fn(rank) on one host thread per device; the first failure (code + message) is reported in the caller's thread.
template <class F> static int on_every_device(mi_multi* m, F fn) {
    const size_t n = m->ctx.size();
    std::vector<int> rc(n, MI_OK); std::vector<std::string> msg(n);
    auto body = [&](size_t r) { rc[r] = fn((int)r); if (rc[r] != MI_OK) msg[r] = g_err; };
    std::vector<std::thread> th;
    for (size_t r = 1; r < n; r++) th.emplace_back(body, r);
    body(0);
    for (auto& t : th) t.join();
    for (size_t r = 0; r < n; r++) if (rc[r] != MI_OK) { g_err = "device " + std::to_string(m->devices[r]) + ": " + msg[r]; return rc[r]; }
    return MI_OK;
}

// Loopback ranks share one card: "60 % of the free HBM" per rank would be claimed `world` times over by threads that all look at
// the same free figure.  With no budget given each rank gets an even share of that default (what the ranks already hold counts as
// free).  ~0 = failure (message recorded).  The RCCL route (one rank per device) passes the caller's value through.
static uint64_t loopback_budget(const mi_multi* m, uint64_t max_state_bytes) {
    if (!m->loopback || max_state_bytes != 0 || m->ctx.size() < 2) return max_state_bytes;
    size_t free_b = 0, total_b = 0;
    if (hipSetDevice(m->devices[0]) != hipSuccess || hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)fail(MI_ERR_HIP, "hipMemGetInfo failed"); return ~0ull; }
    for (const mi_ctx* c : m->ctx) free_b += c->wf_a_bytes + c->wf_b_bytes + c->wf_samp_bytes + c->cand_bytes + c->cand_hdr_bytes;
    return (uint64_t)((double)free_b * 0.6 / (double)m->ctx.size());
}

extern "C" int mi_multi_scene_upload(mi_multi* m, const mi_scene_desc* scene) {
    if (!m || !scene) return fail(MI_ERR_INVALID, "mi_multi_scene_upload: NULL argument");
    // the scene is small (KBs .. a few hundred MB of textures) and 288 GB per GPU make replication free
    return on_every_device(m, [&](int r) { return mi_scene_upload(m->ctx[(size_t)r], scene); });
}

extern "C" int mi_multi_reserve(mi_multi* m, const mi_camera_desc* cam, uint64_t max_state_bytes) {
    if (!m) return fail(MI_ERR_INVALID, "mi_multi_reserve: NULL argument");
    const int world = (int)m->ctx.size();
    if ((max_state_bytes = loopback_budget(m, max_state_bytes)) == ~0ull) return MI_ERR_HIP;
    return on_every_device(m, [&](int r) { return mi_reserve(m->ctx[(size_t)r], cam, world, max_state_bytes); });
}

extern "C" int mi_multi_render(mi_multi* m, const mi_camera_desc* cam, const mi_render_opts* opts, float* out_rgb_f32,
                               uint8_t* out_rgb_u8, uint32_t* out_sig, mi_stats* stats) {
    if (!m || !opts) return fail(MI_ERR_INVALID, "mi_multi_render: NULL argument");
    int rc = check_camera(cam);
    if (rc != MI_OK) return rc;
    const int world = (int)m->ctx.size();
    const TileGrid g = tile_grid(cam, world);
    const size_t slice_f = (size_t)g.padded * kTilePixels * 3, slice_s = (size_t)g.padded * kTilePixels;     // elements per rank
    const size_t npix = (size_t)cam->screen_width * cam->screen_height;
    const bool want_sig = opts->want_signature && out_sig;
    const auto t_begin = std::chrono::steady_clock::now();
    // buffers: device 0 holds the gathered array, the peers their own slice
    for (int r = 0; r < world; r++) {
        HIP_TRY(hipSetDevice(m->devices[(size_t)r]));
        const size_t nf = (r == 0 ? (size_t)world : 1) * slice_f * sizeof(float), ns = (r == 0 ? (size_t)world : 1) * slice_s * 4;
        if ((rc = ensure(&m->d_compact[(size_t)r], &m->compact_bytes[(size_t)r], nf)) != MI_OK) return rc;
        if (want_sig && (rc = ensure(&m->d_sig[(size_t)r], &m->sig_bytes[(size_t)r], ns)) != MI_OK) return rc;
    }
    mi_ctx* c0 = m->ctx[0];
    HIP_TRY(hipSetDevice(m->devices[0]));
    if ((rc = ensure((void**)&c0->d_image, &c0->image_bytes, npix * 3 * sizeof(float))) != MI_OK) return rc;
    if ((rc = ensure((void**)&c0->d_u8, &c0->u8_bytes, npix * 3)) != MI_OK) return rc;     // K4 always runs: the u8 image stays resident on device 0
    if (want_sig && (rc = ensure(&m->d_sig_image, &m->sig_image_bytes, npix * 4)) != MI_OK) return rc;

    // ---- every device renders its tiles (one host thread each; the wavefront pipeline drives its passes from the host) ----
    std::vector<mi_stats> st((size_t)world);
    const uint64_t budget = loopback_budget(m, opts->max_state_bytes);
    if (budget == ~0ull) return MI_ERR_HIP;
    rc = on_every_device(m, [&](int r) {
        mi_ctx* c = m->ctx[(size_t)r];
        if (hipSetDevice(c->device) != hipSuccess) return fail(MI_ERR_HIP, "hipSetDevice failed");
        mi_render_opts o = *opts;
        o.max_state_bytes = budget;
        o.rank = r; o.world = world; o.want_signature = want_sig ? 1 : 0;
        const int rr = render_tiles(c, cam, &o, (float*)m->d_compact[(size_t)r], want_sig ? (uint32_t*)m->d_sig[(size_t)r] : nullptr, c->stream, &st[(size_t)r]);
        if (rr != MI_OK) return rr;
        if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(MI_ERR_HIP, "hipStreamSynchronize failed");
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, c->ev_start, c->ev_stop) == hipSuccess) st[(size_t)r].kernel_ms = ms;
        return (int)MI_OK;
    });
    if (rc != MI_OK) return rc;

    // ---- the frame's single exchange: fan-in of the compact buffers to device 0 (one group, issued from this thread) ----
    // A failure between GroupStart and GroupEnd must not leave the group open (every later RCCL call of this thread would
    // silently join it): the first error is kept, the remaining calls of the group are skipped, GroupEnd always runs.
    if (world > 1 && m->loopback) {
        // test transport: the same slices to the same offsets, each Send / Recv pair replaced by one copy on the SENDER's stream
        // (behind its render) that device 0's stream waits for — the ordering the RCCL pair gives
        for (int r = 1; r < world; r++) {
            hipStream_t sr = m->ctx[(size_t)r]->stream;
            HIP_TRY(hipMemcpyAsync((float*)m->d_compact[0] + (size_t)r * slice_f, m->d_compact[(size_t)r], slice_f * sizeof(float), hipMemcpyDeviceToDevice, sr));
            if (want_sig)
                HIP_TRY(hipMemcpyAsync((uint32_t*)m->d_sig[0] + (size_t)r * slice_s, m->d_sig[(size_t)r], slice_s * 4, hipMemcpyDeviceToDevice, sr));
            HIP_TRY(hipEventRecord(m->ev_sent[(size_t)r], sr));
            HIP_TRY(hipStreamWaitEvent(c0->stream, m->ev_sent[(size_t)r], 0));
        }
    } else if (world > 1) {
        ncclResult_t first = ncclSuccess; const char* what = "";
        auto step = [&](ncclResult_t r, const char* name) { if (first == ncclSuccess && r != ncclSuccess) { first = r; what = name; } return first == ncclSuccess; };
        RCCL_TRY(g_rccl.GroupStart());
        for (int r = 1; r < world; r++) {
            if (!step(g_rccl.Recv((float*)m->d_compact[0] + (size_t)r * slice_f, slice_f, ncclFloat, r, m->comm[0], c0->stream), "ncclRecv")) break;
            if (!step(g_rccl.Send(m->d_compact[(size_t)r], slice_f, ncclFloat, 0, m->comm[(size_t)r], m->ctx[(size_t)r]->stream), "ncclSend")) break;
            if (want_sig) {
                if (!step(g_rccl.Recv((uint32_t*)m->d_sig[0] + (size_t)r * slice_s, slice_s, ncclUint32, r, m->comm[0], c0->stream), "ncclRecv (signatures)")) break;
                if (!step(g_rccl.Send(m->d_sig[(size_t)r], slice_s, ncclUint32, 0, m->comm[(size_t)r], m->ctx[(size_t)r]->stream), "ncclSend (signatures)")) break;
            }
        }
        const ncclResult_t e_end = g_rccl.GroupEnd();
        if (first != ncclSuccess) return fail(MI_ERR_HIP, "%s failed inside the frame's exchange: %s", what, g_rccl.GetErrorString(first));
        if (e_end != ncclSuccess) return fail(MI_ERR_HIP, "ncclGroupEnd failed: %s", g_rccl.GetErrorString(e_end));
    }
    // ---- K3 + K4 on device 0, in stream order behind the receives ----
    HIP_TRY(hipSetDevice(m->devices[0]));
    HIP_TRY(launch_unpermute((const float*)m->d_compact[0], c0->d_image, cam->screen_width, cam->screen_height, g.tx, (uint32_t)world, g.padded, c0->stream));
    if (out_rgb_f32) HIP_TRY(hipMemcpyAsync(out_rgb_f32, c0->d_image, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c0->stream));
    HIP_TRY(launch_tonemap(c0->d_image, c0->d_u8, (uint32_t)npix, 1.0f / cam->gamma, c0->stream));
    if (out_rgb_u8) HIP_TRY(hipMemcpyAsync(out_rgb_u8, c0->d_u8, npix * 3, hipMemcpyDeviceToHost, c0->stream));
    if (want_sig) {
        HIP_TRY(launch_sig_unpermute((const uint32_t*)m->d_sig[0], (uint32_t*)m->d_sig_image, cam->screen_width, cam->screen_height, g.tx, (uint32_t)world, g.padded, c0->stream));
        HIP_TRY(hipMemcpyAsync(out_sig, m->d_sig_image, npix * 4, hipMemcpyDeviceToHost, c0->stream));
    }
    for (int r = world - 1; r >= 0; r--) {          // the peers' sends, then device 0
        HIP_TRY(hipSetDevice(m->devices[(size_t)r]));
        HIP_TRY(hipStreamSynchronize(m->ctx[(size_t)r]->stream));
    }
    if (stats) {
        memset(stats, 0, sizeof *stats);
        for (int r = 0; r < world; r++) {
            stats->samples += st[(size_t)r].samples; stats->pixels += st[(size_t)r].pixels; stats->tiles += st[(size_t)r].tiles;
            stats->kernel_ms = std::max(stats->kernel_ms, st[(size_t)r].kernel_ms);             // the slowest device's pipeline pass
        }
        stats->tiles_padded = g.padded; stats->scene_bytes = st[0].scene_bytes; stats->scene_in_lds = st[0].scene_in_lds;
        stats->total_ms = (float)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_begin).count() * 1e-3f;
    }
    return MI_OK;
}
