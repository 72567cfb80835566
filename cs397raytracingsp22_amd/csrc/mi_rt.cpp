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
#include "scene_compile.hpp"

#pragma clang fp contract(off)

namespace pt {
hipError_t launch_megakernel(const K1Args& args, uint32_t n_blocks, bool lds, bool sig, size_t lds_bytes, hipStream_t stream);
hipError_t launch_megakernel_voted(const K1Args& args, uint32_t n_blocks, bool lds, bool sig, bool diag, bool gv,
                                   size_t lds_bytes, hipStream_t stream);
hipError_t launch_wf_main(const WfArgs& a, uint32_t n_blocks, bool sig, bool gv, bool tex, hipStream_t stream);
hipError_t launch_phong(const K1Args& a, uint32_t n_blocks, bool sig, hipStream_t stream);
hipError_t launch_branch(const K1Args& a, uint32_t n_blocks, uint32_t path_samples, bool sig, hipStream_t stream);
hipError_t launch_walker(const WfArgs& a, const WalkerPlan& p, uint32_t n_blocks, bool* big_lds_enabled, hipStream_t stream);
hipError_t launch_wf_filter_f(const WfArgs& a, uint32_t blocks_per_shard, hipStream_t stream);
hipError_t launch_wf_trav_f(const WfArgs& a, uint32_t n_blocks, hipStream_t stream);
hipError_t launch_wf_replay(const WfArgs& a, uint32_t n_blocks, hipStream_t stream);
hipError_t launch_wf_prefix(uint32_t* out_count, uint32_t* trav_count, uint32_t* in_count, uint32_t* in_blkpfx,
                            uint32_t* trav_pfx, uint32_t* hdr, uint32_t* host_hdr, uint32_t seq, hipStream_t stream);
hipError_t launch_wf_reduce(const WfArgs& a, bool first_batch, bool last_batch, hipStream_t stream);
hipError_t launch_unpermute(const float* gathered, float* image, uint32_t width, uint32_t height, uint32_t tiles_x,
                            uint32_t world, uint32_t tiles_padded, hipStream_t stream);
hipError_t launch_sig_unpermute(const uint32_t* gathered, uint32_t* image, uint32_t width, uint32_t height,
                                uint32_t tiles_x, uint32_t world, uint32_t tiles_padded, hipStream_t stream);
hipError_t launch_tonemap(const float* image, uint8_t* out, uint32_t n_pixels, float inv_gamma, hipStream_t stream);
hipError_t launch_selftest_rcp(unsigned long long* d_mismatches, hipStream_t stream);
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

namespace {
inline uint32_t lowbias32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x;
}
}  // namespace

// ------------------------------------------------------------------ context
struct mi_ctx {
    int device = 0;
    hipStream_t stream = nullptr;            // own stream for mi_render
    hipStream_t aux_stream = nullptr;        // wavefront pipeline: the class-A part of a pass runs here, beside the walkers of the previous pass
    hipStream_t aux2_stream = nullptr;       // ... and wf_trav_f here, beside wf_trav (scenes with meshes of both kinds)
    hipEvent_t ev_pfx = nullptr, ev_part = nullptr, ev_travf = nullptr;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    bool ev_recorded = false;

    // device scene: the blob, its pools (S), and the compiler's tables for the host side of a render (scene.image is emptied once copied)
    void* blob = nullptr; size_t blob_bytes = 0;
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
    hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;     // mi_render's whole-call timer
    bool big_lds_enabled = false;                    // wf_trav_i<1024>'s > 64 KB dynamic-LDS opt-in, set on THIS context's device
    // wavefront pipeline buffers
    void* d_wf_a = nullptr; size_t wf_a_bytes = 0;   // path state ping
    void* d_wf_b = nullptr; size_t wf_b_bytes = 0;   // path state pong
    void* d_wf_samp = nullptr; size_t wf_samp_bytes = 0;
    void* d_wf_acc = nullptr; size_t wf_acc_bytes = 0;
    uint32_t* d_wf_cnt = nullptr;
    uint32_t* h_hdr = nullptr;                       // pinned + device-mapped ring of 8-word slots: wf_prefix writes {blocks, live, queue, seq, live class B, class-A blocks}
    uint64_t wf_counts[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };   // last frame: passes, class-A paths streamed, class-B paths, queue entries, samples, pixels
    uint32_t* h_hdr_dev = nullptr;                   // its device-side address
    uint32_t hdr_seq = 0;
    // per-tile primary-ray masks over the kind-grouped list and the meshes' root boxes (see tile_masks)
    std::vector<unsigned long long> h_tile_mask; void* d_tile_mask = nullptr; size_t tile_mask_bytes = 0;
    mi_camera_desc mask_cam{}; uint32_t mask_stride = 0; bool mask_valid = false;
    std::vector<hipEvent_t> wf_ev;                   // event pool for per-kernel timing of the pipeline
    float wf_ms[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };     // last frame: wf_main, wf_trav, wf_reduce totals (ms), launches, wf_trav_f, wf_replay
    int n_cus = 256;
    // Developer knobs (MI_RT_* environment variables), read ONCE in mi_ctx_create; none is needed for
    // normal operation and none changes a result — what a caller may want to control is in mi_render_opts.
    struct Tuning {
        uint32_t vote_t = 2, vote_a = 1, k_steps = 8;   // voted megakernel
        uint32_t lds_pad = 0;                           // occupancy experiments
        uint32_t refill_min = 16;                       // wf_trav: refill idle lanes when at least this many are idle (A/B round 2: 32 / 16 / 8 -> 36.9 / 35.8 / 38.6 ms on cfg2)
        uint32_t fuse_max = 0, fuse_min = 32;           // wf_main: in-launch continuation (rounds: 0 = automatic; lanes needed)
        int trav_lds = -1;                              // reference-tree walker override, a WalkerPlan form (-1 = automatic)
        int trav_bpc = 0;                               // its blocks per CU override (0 = automatic)
        int travf_bpc = 0;                              // wf_trav_f blocks per CU override (0 = default)
        int kernel_timing = -1;                         // per-launch HIP events: -1 = single-rank renders only
        bool global_bvh = false;                        // never stage a BVH in LDS
        bool wf_stamps = false;                         // -DPT_WF_STAMPS builds: collect wf_main phase stamps
        bool debug_mask = false;                        // print tile-mask statistics
        bool dump_launches = false;                     // print every pipeline launch's duration (needs per-launch events)
        int split = 1;                                  // wf_main in two parts, class A beside the previous pass' walkers (0 = one launch per pass)
        int conc = 1, conc_trav_bpc = 0, conc_travf_bpc = 0;   // wf_trav and wf_trav_f on two streams (0 = one after the other); their blocks per CU then (0 = the usual)
        uint32_t tail_paths = 0xffffffffu;              // a pass that starts with at most this many live paths runs every path as far as it can inside the launch (0 = never; default: automatic)
        uint32_t nowait_blocks = 16384;                 // passes whose grid bound is at most this many blocks are launched without waiting for the previous header (0 = always wait)
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

extern "C" int mi_abi_version(void) { return MI_RT_ABI_VERSION; }
extern "C" const char* mi_last_error(void) { return g_err.c_str(); }

extern "C" void mi_ctx_destroy(mi_ctx* c);

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
    HIP_TRY(hipMalloc((void**)&c->d_wf_cnt, (9 * 256 + 64) * sizeof(uint32_t)));
    HIP_TRY(hipHostMalloc((void**)&c->h_hdr, 16 * 8 * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent));     // kHdrRing slots of 8 words
    memset(c->h_hdr, 0, 16 * 8 * sizeof(uint32_t));
    HIP_TRY(hipHostGetDevicePointer((void**)&c->h_hdr_dev, c->h_hdr, 0));
    // developer knobs: read here, once (never on the render path)
    mi_ctx::Tuning& t = c->tune;
    auto env_u = [](const char* name, uint32_t& v) { if (const char* e = getenv(name)) v = (uint32_t)atoi(e); };
    auto env_i = [](const char* name, int& v) { if (const char* e = getenv(name)) v = atoi(e); };
    env_u("MI_RT_VOTE_T", t.vote_t); env_u("MI_RT_VOTE_A", t.vote_a); env_u("MI_RT_KSTEPS", t.k_steps);
    if (const char* e = getenv("MI_RT_LDS_PAD_KB")) t.lds_pad = (uint32_t)atoi(e) * 1024u;
    env_u("MI_RT_WF_REFILL", t.refill_min);
    env_u("MI_RT_WF_FUSE_MAX", t.fuse_max); env_u("MI_RT_WF_FUSE_MIN", t.fuse_min);
    env_i("MI_RT_WF_SPLIT", t.split); env_u("MI_RT_WF_NOWAIT_BLOCKS", t.nowait_blocks); env_u("MI_RT_WF_TAIL_PATHS", t.tail_paths);
    env_i("MI_RT_WF_CONC", t.conc); env_i("MI_RT_WF_CONC_TRAV_BPC", t.conc_trav_bpc); env_i("MI_RT_WF_CONC_TRAVF_BPC", t.conc_travf_bpc);
    env_i("MI_RT_WF_TRAV_LDS", t.trav_lds); env_i("MI_RT_WF_TRAV_BPC", t.trav_bpc); env_i("MI_RT_WF_TRAVF_BPC", t.travf_bpc); env_i("MI_RT_WF_KERNEL_TIMING", t.kernel_timing);
    t.global_bvh = getenv("MI_RT_GLOBAL_BVH") != nullptr;
    t.wf_stamps = getenv("MI_RT_WF_STAMPS") != nullptr;
    t.debug_mask = getenv("MI_RT_DEBUG_MASK") != nullptr;
    t.dump_launches = getenv("MI_RT_WF_DUMP_LAUNCHES") != nullptr;
    env_u("MI_RT_SPIN_TIMEOUT_MS", t.spin_timeout_ms);
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
    if (c->d_wf_a) (void)hipFree(c->d_wf_a);
    if (c->d_wf_b) (void)hipFree(c->d_wf_b);
    if (c->d_wf_samp) (void)hipFree(c->d_wf_samp);
    if (c->d_wf_acc) (void)hipFree(c->d_wf_acc);
    if (c->d_cand) (void)hipFree(c->d_cand);
    if (c->d_cand_hdr) (void)hipFree(c->d_cand_hdr);
    if (c->d_tile_mask) (void)hipFree(c->d_tile_mask);
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
    c->blob = nullptr; c->blob_bytes = 0; c->S = DScene{}; c->scene = CompiledScene(); c->have_scene = false;
    c->mask_valid = false;
    const size_t total = sc.image.size();
    void* blob = nullptr;
    hipError_t e = hipMalloc(&blob, total);
    if (e != hipSuccess) return fail(MI_ERR_OOM, "hipMalloc(%zu) for the scene failed: %s", total, hipGetErrorString(e));
    c->blob = blob; c->blob_bytes = total;
    HIP_TRY(hipMemcpy(c->blob, sc.image.data(), total, hipMemcpyHostToDevice));
    sc.image = std::vector<uint8_t>();
    c->S = sc.device_scene(c->blob);
    c->scene = std::move(sc);
    c->have_scene = true;
    return MI_OK;
}

// ------------------------------------------------------------------ render
static int check_camera(const mi_camera_desc* cam) {
    if (!cam) return fail(MI_ERR_INVALID, "camera is NULL");
    if (cam->projection_mode != MI_PROJ_PERSPECTIVE && cam->projection_mode != MI_PROJ_ORTHOGRAPHIC)
        return fail(MI_ERR_INVALID, "unknown projection_mode %d", cam->projection_mode);
    if (cam->shading_mode != MI_SHADE_PATHTRACE && cam->shading_mode != MI_SHADE_PHONG)
        return fail(MI_ERR_INVALID, "unknown shading_mode %d", cam->shading_mode);
    if (cam->path_samples == 0) return fail(MI_ERR_INVALID, "path_samples must be >= 1 (tracing.rs:318 divides by it)");
    if (cam->screen_width == 0 || cam->screen_height == 0 || cam->screen_width > 32768 || cam->screen_height > 32768)
        return fail(MI_ERR_INVALID, "bad image size %ux%u", cam->screen_width, cam->screen_height);
    if (cam->aa_sample_count == 0) return fail(MI_ERR_INVALID, "aa_sample_count must be >= 1");
    if ((uint32_t)sqrtf((float)cam->aa_sample_count) == 0) return fail(MI_ERR_INVALID, "aa_sample_count too small");
    if (!(cam->gamma > 0.0f) || !std::isfinite(cam->gamma)) return fail(MI_ERR_INVALID, "gamma must be finite and > 0 (tracing.rs:254 raises to 1/gamma)");
    // A camera that makes every ray non-finite is refused, not rendered.  The reference would render it: its tests then "hit"
    // with a NaN distance wherever every reject comparison is false (geometry.rs:338-349, 401-410) and Scene keeps the FIRST
    // such hit in Scene.objects order (tracing.rs:335, NaN < x is false) — a result that depends on the evaluation order
    // of unordered comparisons, which the kind-grouped object list of the kernels does not keep.
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(cam->eyepoint[k]) || !std::isfinite(cam->view_dir[k]) || !std::isfinite(cam->up[k]))
            return fail(MI_ERR_INVALID, "camera eyepoint / view_dir / up must be finite");
    if (!std::isfinite(cam->focal_length) || !std::isfinite(cam->focus_dist) || !std::isfinite(cam->lens_radius) || std::isnan(cam->max_trace_dist))
        return fail(MI_ERR_INVALID, "camera focal_length / focus_dist / lens_radius must be finite, max_trace_dist not NaN");
    {
        // tracing.rs:188: rotation.x = view_dir.cross(up).normalize(), in f32 as the kernels evaluate it
        const float* v = cam->view_dir; const float* u = cam->up;
        const float cx = v[1] * u[2] - v[2] * u[1], cy = v[2] * u[0] - v[0] * u[2], cz = v[0] * u[1] - v[1] * u[0];
        const float m2 = (cx * cx + cy * cy) + cz * cz;
        if (!(m2 > 0.0f) || !std::isfinite(1.0f / sqrtf(m2)))
            return fail(MI_ERR_INVALID, "view_dir x up is zero or not finite: the camera basis is singular and every ray would be NaN (tracing.rs:188)");
    }
    return MI_OK;
}

// The tile grid of the partition.  Tiles are numbered row-major over a grid whose ROW LENGTH `tx` is the image's tile columns
// rounded up to the next integer coprime with `world` (tile t -> rank t % world, slot t / world): a row length that shares a factor
// with the rank count repeats the same few column classes for a rank in every row (60 columns over 8 ranks: two classes, and the
// ranks whose classes cross the expensive middle of the frame took 7 % longer than the others); a coprime one walks every rank
// through all classes.  The extra columns hold no pixel: their tiles are rendered as "outside the image" (zeros) and never
// copied anywhere.  world = 1 (mi_render) keeps the plain grid.
static void tile_counts(const mi_camera_desc* cam, int world, uint32_t* tx, uint32_t* ty, uint32_t* total, uint32_t* padded) {
    uint32_t stride = (cam->screen_width + MI_TILE - 1) / MI_TILE;
    auto gcd = [](uint32_t a, uint32_t b) { while (b) { const uint32_t r = a % b; a = b; b = r; } return a; };
    while (gcd(stride, (uint32_t)world) != 1u) stride++;
    *tx = stride;
    *ty = (cam->screen_height + MI_TILE - 1) / MI_TILE;
    *total = *tx * *ty;
    *padded = (*total + (uint32_t)world - 1) / (uint32_t)world;
}

extern "C" int mi_compact_size(const mi_camera_desc* cam, int32_t world, uint32_t* tiles_total, uint32_t* tiles_padded) {
    if (!cam || world < 1 || !tiles_total || !tiles_padded) return fail(MI_ERR_INVALID, "mi_compact_size: bad argument");
    uint32_t tx, ty;
    tile_counts(cam, world, &tx, &ty, tiles_total, tiles_padded);
    return MI_OK;
}

static void make_camera(const mi_camera_desc* cam, DCamera* C) {
    memset(C, 0, sizeof *C);
    h3 view = H3p(cam->view_dir), up = H3p(cam->up);
    h3 c0 = normalize(cross(view, up));                                 // tracing.rs:188
    C->eye[0] = cam->eyepoint[0]; C->eye[1] = cam->eyepoint[1]; C->eye[2] = cam->eyepoint[2];
    C->rot[0] = c0.x; C->rot[1] = c0.y; C->rot[2] = c0.z;
    C->rot[3] = up.x; C->rot[4] = up.y; C->rot[5] = up.z;               // :189
    C->rot[6] = -view.x; C->rot[7] = -view.y; C->rot[8] = -view.z;      // :190
    C->pixel_size = 1.0f / (float)cam->screen_height;                   // :160
    C->n = (float)cam->aa_sample_count;                                 // :162
    C->rootn = sqrtf(C->n);                                             // :163
    C->half_rootn = 0.5f * C->rootn;
    C->half_n = 0.5f * C->n;
    C->cx_base = -(0.5f * (float)cam->screen_width);                    // :178
    C->cy_base = 0.5f + 0.5f * (float)cam->screen_height;               // :179
    C->focal_length = cam->focal_length; C->focus_dist = cam->focus_dist; C->lens_radius = cam->lens_radius;
    C->max_trace_dist = cam->max_trace_dist;
    C->rootn_u = (uint32_t)C->rootn;                                    // :169 `rootn as u32`
    C->spp = cam->aa_sample_count;
    C->zone = (C->spp << __builtin_clz(C->spp)) - 1u;                   // rand 0.8.4 UniformInt::sample_single
    C->path_depth = cam->path_depth;
    C->width = cam->screen_width; C->height = cam->screen_height;
    C->ortho = cam->projection_mode == MI_PROJ_ORTHOGRAPHIC ? 1u : 0u;
    // :200,204  rotation * view_dir with cgmath's Matrix3 * Vector3 order: (c0*v.x + c1*v.y) + c2*v.z
    h3 c2 = H3(-view.x, -view.y, -view.z);
    h3 od = add(add(scale(c0, view.x), scale(up, view.y)), scale(c2, view.z));
    C->ortho_dir[0] = od.x; C->ortho_dir[1] = od.y; C->ortho_dir[2] = od.z;
}

// K1w: the wavefront pipeline (pt_kernels.hip).  The host enqueues one iteration per path segment:
// wf_main, wf_prefix (device-side bookkeeping of the shard counters), wf_trav.  It needs one number back
// per iteration — the grid of the next wf_main — which arrives on a second stream while wf_trav runs, so
// the compute stream never waits for the host; the call still returns only when the frame is done.
//
// Memory: path state is streamed through HBM — 2 x 96 B (ping/pong) + 16 B sample slot per path
// (kWfBytesPerPath; the walkers read the class-B lists, there is no traversal queue).  The batch is sized to the free HBM (288 GB on MI355X: the whole 1080p/256 spp
// frame, 531 M paths = 112 GB, is ONE batch), halved on allocation failure.
static const int kHdrRing = 16;        // pinned header slots (wf_prefix -> host), one per pass in flight
static const int kRunAhead = 3;        // passes the host may launch before it has read the header of an earlier one
static const size_t kWfBytesPerPath = 2 * (size_t)kWfPlanes * sizeof(float4) + sizeof(float4);      // ping / pong state, sample slot
static const size_t kWfBytesPerPathTwoStage = (size_t)kCandMax * sizeof(uint2) + sizeof(uint2);     // candidates + header per queue slot

// which meshes this render walks two-stage (bit m = live mesh m)
static uint32_t two_stage_mask(const mi_ctx* c, uint32_t flags) {
    if (flags & MI_OPT_REFERENCE_WALK) return 0u;
    uint32_t m = 0;
    for (size_t i = 0; i < c->scene.meshes.size() && i < (size_t)kTwoStageMaxMeshes; i++)
        if (c->scene.meshes[i].qualifies && ((flags & MI_OPT_TWO_STAGE) || c->scene.meshes[i].default_ts)) m |= 1u << i;
    return m;
}

static int wf_alloc(mi_ctx* c, WfArgs& a, uint32_t spp, uint64_t max_state_bytes, bool two_stage, uint32_t& s_batch) {
    uint64_t max_paths;
    const size_t per_path = kWfBytesPerPath + (two_stage ? kWfBytesPerPathTwoStage : 0);
    if (max_state_bytes != 0) max_paths = max_state_bytes / per_path;        // the caller's budget (mi_render_opts)
    else {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)8 << 30;
        // what this context already holds for the pipeline can be reused
        free_b += c->wf_a_bytes + c->wf_b_bytes + c->wf_samp_bytes + c->cand_bytes + c->cand_hdr_bytes;
        max_paths = (uint64_t)((double)free_b * 0.6 / (double)per_path);
    }
    if (max_paths > (1ull << 31)) max_paths = 1ull << 31;           // 32-bit path indices
    uint64_t sb = max_paths / a.npix;
    // the smallest batch is one sample of every (padded) pixel of this rank: a caller's budget below that cannot be honoured
    if (sb < 1 && max_state_bytes != 0)
        return fail(MI_ERR_INVALID, "max_state_bytes = %llu is below the pipeline's minimum for this image: one sample per pixel = %llu bytes",
                    (unsigned long long)max_state_bytes, (unsigned long long)((uint64_t)a.npix * per_path));
    if (sb < 1) sb = 1;
    if (sb > spp) sb = spp;
    for (;;) {
        s_batch = (uint32_t)sb;
        const uint32_t paths = a.npix * s_batch;
        const uint32_t max_blocks = (paths + kBlock - 1) / kBlock;
        // a shard receives at most the paths of its own input blocks: ceil(n_blocks / shards) blocks, where
        // n_blocks <= max_blocks + 2 * shards (one partial block per (class, shard) range)
        a.region = ((max_blocks + kWfShards - 1) / kWfShards + 3) * kBlock;
        a.cap = a.region * (uint32_t)kWfShards;
        const size_t st_bytes = (size_t)kWfPlanes * sizeof(float4) * a.cap;
        int rc = ensure(&c->d_wf_a, &c->wf_a_bytes, st_bytes);
        if (rc == MI_OK) rc = ensure(&c->d_wf_b, &c->wf_b_bytes, st_bytes);
        if (rc == MI_OK) rc = ensure(&c->d_wf_samp, &c->wf_samp_bytes, (size_t)paths * sizeof(float4));
        if (rc == MI_OK) rc = ensure(&c->d_wf_acc, &c->wf_acc_bytes, (size_t)a.npix * sizeof(float4));
        if (rc == MI_OK && two_stage) rc = ensure(&c->d_cand, &c->cand_bytes, (size_t)a.cap * kCandMax * sizeof(uint2));
        if (rc == MI_OK && two_stage) rc = ensure(&c->d_cand_hdr, &c->cand_hdr_bytes, (size_t)a.cap * sizeof(uint2));
        if (rc == MI_OK) return MI_OK;
        if (rc != MI_ERR_OOM || sb == 1) return rc;
        (void)hipGetLastError();
        sb = (sb + 1) / 2;                                           // back off and retry with half the batch
    }
}

// sizes and allocates (host-side work: must happen BEFORE the timing start event is recorded)
static int wf_prepare(mi_ctx* c, const mi_camera_desc* cam, uint32_t padded, uint64_t max_state_bytes, bool two_stage, WfArgs& a, uint32_t& s_batch) {
    memset(&a, 0, sizeof a);
    a.npix = padded * (uint32_t)kTilePixels;
    const uint32_t spp = cam->aa_sample_count;
    if (spp > 0xffffu) return fail(MI_ERR_UNSUPPORTED, "wavefront variant: aa_sample_count must be <= 65535");
    if (cam->path_depth > 0xffffu) return fail(MI_ERR_UNSUPPORTED, "wavefront variant: path_depth must be <= 65535");
    return wf_alloc(c, a, spp, max_state_bytes, two_stage, s_batch);
}

// Primary-ray culling for the wavefront pipeline.  For every 32x32 tile: which Triangle / Sphere entries of
// the kind-grouped list can a camera ray of that tile reach?  A perspective camera with lens_radius 0
// sends every ray of a tile from the eye through the tile's pixel footprints.  The jitter (tracing.rs:166-173,
// n = aa_sample_count, r = (u32)sqrt(n)) is (floor(i / r) - sqrt(n)/2) / sqrt(n) + (rand - n/2) / n px in x and
// ((i % r) - sqrt(n)/2) / sqrt(n) + (rand - n/2) / n in y: from -1 px up to floor((n-1)/r) / sqrt(n) - 1/n px in x,
// which exceeds +1 px when n is not a square (n = 3: +0.82, 8: +0.94, 31: +1.05, never +1.16 or more), and
// below +1 px in y.  The 2 px margin below covers all of it: the rays lie inside the pyramid spanned by
// the four corner directions of the footprint widened by 2 px (>= 5e-4 rad of slack beyond the jitter at any
// resolution up to 2k rows, against f32 rounding of ~1e-7 in the generated directions).  An object that is
// entirely on the outer side of one of the pyramid's four planes through the eye cannot be hit; it is
// dropped from the tile's mask and its test — which would have missed — is not run.  f64 on the host,
// a further 1e-4 scene-unit slack; any non-finite value or a singular camera basis keeps everything.
// Planes and ConvexVolumes are never masked.  Returns false when masking does not apply.
static bool tile_masks(mi_ctx* c, const mi_camera_desc* cam, uint32_t flags, uint32_t stride) {
    const CompiledScene& sc = c->scene;
    const int n_ts = sc.n_list_tri + sc.n_list_sphere;
    const int n_mesh = (int)sc.meshes.size();
    if ((n_ts == 0 && n_mesh == 0) || n_ts > 64 || n_mesh > 32) return false;
    // rays must leave the eye itself (no lens) towards the image plane (focus_dist > 0 keeps the direction's sign)
    if (cam->projection_mode != MI_PROJ_PERSPECTIVE || cam->lens_radius != 0.0f || !(cam->focus_dist > 0.0f) || (flags & MI_OPT_NO_TILE_MASKS)) return false;
    if (c->mask_valid && c->mask_stride == stride && memcmp(&c->mask_cam, cam, sizeof *cam) == 0) return true;
    const double W = cam->screen_width, H = cam->screen_height, p = 1.0 / H;
    const double view[3] = { cam->view_dir[0], cam->view_dir[1], cam->view_dir[2] };
    const double up[3] = { cam->up[0], cam->up[1], cam->up[2] };
    double c0[3] = { view[1] * up[2] - view[2] * up[1], view[2] * up[0] - view[0] * up[2], view[0] * up[1] - view[1] * up[0] };
    const double l0 = sqrt(c0[0] * c0[0] + c0[1] * c0[1] + c0[2] * c0[2]);
    if (!(l0 > 1e-12) || !std::isfinite(l0)) return false;
    for (double& v : c0) v /= l0;
    // det of R = [c0 up -view]: a (near-)singular basis flattens the pyramid
    const double det = c0[0] * (up[1] * -view[2] - up[2] * -view[1]) - up[0] * (c0[1] * -view[2] - c0[2] * -view[1])
                     + -view[0] * (c0[1] * up[2] - c0[2] * up[1]);
    if (!(fabs(det) > 1e-6) || !std::isfinite(det)) return false;
    auto dir = [&](double px, double py, double* o) {           // R * (camera-space point on the image plane)
        const double x = p * (px - 0.5 * W + 0.5), y = p * (0.5 + 0.5 * H - py), z = -(double)cam->focal_length;
        for (int k = 0; k < 3; k++) o[k] = c0[k] * x + up[k] * y + -view[k] * z;
    };
    // `stride` >= the image's tile columns: the row length of the tile numbering (tile_counts); the surplus columns hold no pixel
    const uint32_t tx = stride, tx_image = (cam->screen_width + MI_TILE - 1) / MI_TILE, ty = (cam->screen_height + MI_TILE - 1) / MI_TILE;
    // [0, tiles): list masks; [tiles, 2*tiles): low 32 bits = mesh mask, bit 63 = DEAD tile (nothing reachable:
    // every camera ray of the tile leaves the scene at once)
    const size_t n_tiles = (size_t)tx * ty;
    c->h_tile_mask.assign(2 * n_tiles, ~0ull);
    for (size_t t = 0; t < n_tiles; t++) c->h_tile_mask[n_tiles + t] = 0xffffffffull;
    const double margin_px = 2.0, slack = 1e-4;
    const double eye[3] = { cam->eyepoint[0], cam->eyepoint[1], cam->eyepoint[2] };
    // Test shapes.  The geometric argument needs the f32 intersection tests to be WELL CONDITIONED for every
    // camera ray, or a test could "hit" a triangle it passes far from.  Moller-Trumbore (geometry.rs:434-446)
    // computes u = (s.h)/a with a = -d.n: the rounding error of u is ~2^-22 |s||h| / |a|, and a test that passes
    // t <= t_max has |a| >= |n| h_E / t_max (t's numerator s.n = h_E |n| does not depend on d; h_E = distance
    // of the eye from the triangle's plane).  So with  G = 2^-22 S t_reach / (h_E alt_min)  (S = eye to
    // farthest vertex, alt_min = smallest altitude, t_reach = max_trace_dist x the column norms of the camera
    // basis) small enough (below) every accepted ray passes inside the triangle scaled by 1.01 about its
    // centroid — which is the shape tested against the pyramid.  Triangles that fail the
    // guard (eye almost in their plane, slivers, huge max_trace_dist) are simply never masked.
    // Spheres (geometry.rs:395-408): the discriminant's rounding moves the silhouette by ~1e-6 relative;
    // the radius is padded by 0.1 % plus 1e-5 of the centre distance.
    struct Shape { bool cullable; double v[3][3]; double r; };
    std::vector<Shape> shapes((size_t)n_ts);
    {
        double colmax = 0.0;
        { const double lu = sqrt(up[0] * up[0] + up[1] * up[1] + up[2] * up[2]), lv = sqrt(view[0] * view[0] + view[1] * view[1] + view[2] * view[2]);
          colmax = 1.0 + lu + lv; }                            // |R d| <= (|c0| + |up| + |view|) |d|, |c0| = 1
        const double t_reach = (double)cam->max_trace_dist * colmax;
        for (int e = 0; e < n_ts; e++) {
            const DObject& ob = sc.list[(size_t)e];
            Shape& sh = shapes[(size_t)e];
            sh.cullable = false; sh.r = 0.0;
            if (e < sc.n_list_tri) {
                double P[3][3], cen[3] = { 0, 0, 0 };
                for (int vtx = 0; vtx < 3; vtx++) for (int q = 0; q < 3; q++) {
                    P[vtx][q] = (double)ob.f[q] + (vtx == 1 ? (double)ob.f[3 + q] : vtx == 2 ? (double)ob.f[6 + q] : 0.0);
                    cen[q] += P[vtx][q] / 3.0;
                }
                const double e1[3] = { P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2] };
                const double e2[3] = { P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2] };
                const double e3[3] = { P[2][0] - P[1][0], P[2][1] - P[1][1], P[2][2] - P[1][2] };
                const double nn[3] = { e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0] };
                const double area2 = sqrt(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]);
                auto len = [](const double* w) { return sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]); };
                const double emax = std::max(len(e1), std::max(len(e2), len(e3)));
                double S = 0.0, hE = 0.0;
                for (int vtx = 0; vtx < 3; vtx++) { const double w[3] = { P[vtx][0] - eye[0], P[vtx][1] - eye[1], P[vtx][2] - eye[2] }; S = std::max(S, len(w)); }
                for (int q = 0; q < 3; q++) hE += (eye[q] - P[0][q]) * nn[q];
                hE = fabs(hE) / area2;
                const double alt_min = area2 / emax;
                const double G = ldexp(1.0, -22) * S * t_reach / (hE * alt_min);
                // (u, v) off by G moves the point by <= 2 G emax in the plane; scaling by 1.01 about the centroid moves
                // every edge out by >= 0.0033 alt_min: G <= 1e-3 alt_min / emax keeps the ray inside the scaled triangle
                sh.cullable = std::isfinite(G) && area2 > 0.0 && G <= 1e-3 * alt_min / emax;
                for (int vtx = 0; vtx < 3; vtx++) for (int q = 0; q < 3; q++) sh.v[vtx][q] = cen[q] + (P[vtx][q] - cen[q]) * 1.01;
            } else {
                double dist = 0.0;
                for (int q = 0; q < 3; q++) { sh.v[0][q] = (double)ob.f[q]; dist += (sh.v[0][q] - eye[q]) * (sh.v[0][q] - eye[q]); }
                sh.r = fabs((double)ob.f[3]) * 1.001 + 1e-5 * sqrt(dist);
                sh.cullable = std::isfinite(sh.r) && std::isfinite(dist);
            }
        }
    }
    for (uint32_t j = 0; j < ty; j++) for (uint32_t i = 0; i < tx; i++) {
        if (i >= tx_image) {                     // a column beyond the image: nothing to render, whatever the scene holds
            c->h_tile_mask[(size_t)j * tx + i] = 0ull; c->h_tile_mask[n_tiles + (size_t)j * tx + i] = 1ull << 63;
            continue;
        }
        const double x0 = (double)i * MI_TILE - margin_px, x1 = std::min<double>(W, (i + 1.0) * MI_TILE) - 1.0 + margin_px;
        const double y0 = (double)j * MI_TILE - margin_px, y1 = std::min<double>(H, (j + 1.0) * MI_TILE) - 1.0 + margin_px;
        double cs[4][3], ctr[3], n[4][3];
        dir(x0, y0, cs[0]); dir(x1, y0, cs[1]); dir(x1, y1, cs[2]); dir(x0, y1, cs[3]);
        dir(0.5 * (x0 + x1), 0.5 * (y0 + y1), ctr);
        bool ok = true;
        for (int k = 0; k < 4 && ok; k++) {
            const double* a = cs[k]; const double* b = cs[(k + 1) & 3];
            double v[3] = { a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0] };
            const double l = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
            if (!(l > 0.0) || !std::isfinite(l)) { ok = false; break; }
            const double sgn = (v[0] * ctr[0] + v[1] * ctr[1] + v[2] * ctr[2]) < 0.0 ? -1.0 : 1.0;      // inward
            for (int q = 0; q < 3; q++) n[k][q] = sgn * v[q] / l;
        }
        if (!ok) continue;
        unsigned long long mask = ~0ull;
        for (int e = 0; e < n_ts; e++) {
            const Shape& sh = shapes[(size_t)e];
            if (!sh.cullable) continue;
            bool cull = false;
            for (int k = 0; k < 4 && !cull; k++) {
                if (e < sc.n_list_tri) {                    // the three (scaled) vertices all outside plane k
                    bool all_out = true;
                    for (int vtx = 0; vtx < 3 && all_out; vtx++) {
                        double d = 0.0;
                        for (int q = 0; q < 3; q++) d += (sh.v[vtx][q] - eye[q]) * n[k][q];
                        all_out = d < -slack;              // false for NaN
                    }
                    cull = all_out;
                } else {
                    double d = 0.0;
                    for (int q = 0; q < 3; q++) d += (sh.v[0][q] - eye[q]) * n[k][q];
                    cull = d < -(sh.r + slack);
                }
            }
            if (cull) mask &= ~(1ull << e);
        }
        c->h_tile_mask[(size_t)j * tx + i] = mask;
        unsigned long long mm = 0xffffffffull;
        for (int m = 0; m < n_mesh && m < 32; m++) {          // the mesh word has 32 bits: meshes 32, 33, ... are never culled
            const CompiledScene::Mesh& B = sc.meshes[(size_t)m];
            if (!B.cullable) continue;
            bool cull = false;
            for (int k = 0; k < 4 && !cull; k++) {
                bool all_out = true;
                for (int v = 0; v < 8 && all_out; v++) {
                    double d = 0.0, len = 0.0;
                    for (int q = 0; q < 3; q++) { const double w = B.corner[v][q] - eye[q]; d += w * n[k][q]; len += fabs(B.corner[v][q]) + fabs(eye[q]); }
                    all_out = d < -(slack + 1e-5 * len);       // f32 rounding of the object-space ray and slabs
                }
                cull = all_out;
            }
            if (cull) mm &= ~(1ull << m);
        }
        const unsigned long long ts_bits = (n_ts >= 64) ? ~0ull : ((1ull << n_ts) - 1ull);
        const unsigned long long mesh_bits = (n_mesh >= 32) ? 0xffffffffull : ((1ull << n_mesh) - 1ull);
        if ((mask & ts_bits) == 0ull && (mm & mesh_bits) == 0ull && sc.n_unmasked == 0 && n_mesh <= 32) mm |= 1ull << 63;
        c->h_tile_mask[n_tiles + (size_t)j * tx + i] = mm;
    }
    c->mask_cam = *cam; c->mask_stride = stride; c->mask_valid = false;              // valid once uploaded
    if (c->tune.debug_mask) {
        size_t bits = 0, mbits = 0, dead = 0;
        for (size_t t = 0; t < n_tiles; t++) {
            bits += (size_t)__builtin_popcountll(c->h_tile_mask[t] & ((n_ts >= 64) ? ~0ull : ((1ull << n_ts) - 1ull)));
            mbits += (size_t)__builtin_popcountll(c->h_tile_mask[n_tiles + t] & ((n_mesh >= 32) ? 0xffffffffull : ((1ull << n_mesh) - 1ull)));
            dead += (size_t)(c->h_tile_mask[n_tiles + t] >> 63);
        }
        fprintf(stderr, "[mi_rt] tile masks: %zu tiles, %.2f of %d list entries and %.2f of %d meshes kept per tile, %zu dead tiles\n",
                n_tiles, (double)bits / (double)n_tiles, n_ts, (double)mbits / (double)n_tiles, n_mesh, dead);
    }
    return true;
}

// Samples [begin, end) of every pixel, added in order to `accum` (nullptr = the context's own buffer).
// begin == 0 starts the sums from zero; end == aa_sample_count also writes the per-pixel means.
struct SampleRange { uint32_t begin, end; float4* accum; };

static int render_tiles_wavefront(mi_ctx* c, const K1Args& k, const mi_camera_desc* cam, WfArgs a, uint32_t s_batch, bool lds, uint32_t flags,
                                  float* d_compact, uint32_t* d_sig, SampleRange range, hipStream_t stream) {
    a.S = k.S; a.C = k.C; a.R = k.R; a.seed_key = k.seed_key;
    const uint32_t spp = cam->aa_sample_count;
    int rc = MI_OK;
    (void)rc;
    // counters: [0..2S) out_count (class A shards, class B shards), [2S..3S) trav_count, [3S] trav_head,
    // then in_count [2S], in_blkpfx [2S+1], trav_pfx [S+1]
    const size_t S_ = (size_t)kWfShards;
    uint32_t* cnt = c->d_wf_cnt;
    a.out_count = cnt; a.trav_count = cnt + 2 * S_; a.trav_head = cnt + 3 * S_;
    uint32_t* d_in_count = cnt + 3 * S_ + 8;
    uint32_t* d_in_pfx = d_in_count + 2 * S_;
    a.in_count = d_in_count; a.in_blkpfx = d_in_pfx;
    uint32_t* d_trav_pfx = d_in_pfx + 2 * S_ + 8;
    a.trav_pfx = d_trav_pfx;
    uint32_t* d_hdr = d_trav_pfx + S_ + 8;
    a.hdr = d_hdr;
    a.samp = (float4*)c->d_wf_samp; a.accum = range.accum ? range.accum : (float4*)c->d_wf_acc;
    a.out = d_compact; a.sig = d_sig;
    a.tile_mask = nullptr;
    if (tile_masks(c, cam, flags, a.R.tiles_x)) {
        if (!c->mask_valid) {
            int rcm = ensure(&c->d_tile_mask, &c->tile_mask_bytes, c->h_tile_mask.size() * sizeof(unsigned long long));
            if (rcm != MI_OK) return rcm;
            HIP_TRY(hipMemcpyAsync(c->d_tile_mask, c->h_tile_mask.data(), c->h_tile_mask.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, stream));
            c->mask_valid = true;
        }
        a.tile_mask = (const unsigned long long*)c->d_tile_mask;
    }
    a.diag = nullptr;           // developer builds (-DPT_WF_STAMPS): phase stamps of wf_main
    if (c->tune.wf_stamps) { a.diag = c->d_diag; HIP_TRY(hipMemsetAsync(c->d_diag, 0, 16 * sizeof(unsigned long long), stream)); }
    a.refill_min = c->tune.refill_min;
    // further shade + intersect rounds inside one wf_main launch: one when meshes park part of every wave's rays for the walker
    // (cfg2: 1 / 2 / 3 rounds -> 99 / 101 / 103 ms), two in a scene without meshes, where every live lane can go on
    // (cfg5 at 512 spp: 1 / 2 / 3 / 5 rounds -> 281.6 / 271.8 / 278.4 / 287.7 ms; the cfg1 scene at 1080p: 46.6 / 42.9 / 47.4 / 48.1 ms)
    a.fuse_max = c->tune.fuse_max ? c->tune.fuse_max : (c->S.n_meshes == 0 ? 2u : 1u);
    a.fuse_min = c->tune.fuse_min < 1 ? 1 : c->tune.fuse_min;
    const uint32_t fuse_max_normal = a.fuse_max, fuse_min_normal = a.fuse_min;
    // Which meshes are walked how: the two-stage meshes (wf_trav_f + wf_replay), the rest through the reference's tree (wf_trav).
    const uint32_t all_meshes = c->S.n_meshes >= 32 ? 0xffffffffu : ((1u << c->S.n_meshes) - 1u);
    const uint32_t ts_mask = two_stage_mask(c, flags) & all_meshes;
    const uint32_t ref_mask = all_meshes & ~ts_mask;
    const WalkerPlan walker = plan_walker(c->scene, ref_mask, c->tune.trav_lds, c->tune.trav_bpc, c->tune.global_bvh);
    a.R.lds_nodes = walker.lds_nodes; a.R.lds_tris = walker.lds_tris;
    a.cand = (uint2*)c->d_cand; a.cand_hdr = (uint2*)c->d_cand_hdr;
    float4* bufs[2] = { (float4*)c->d_wf_a, (float4*)c->d_wf_b };
    const uint32_t trav_bpc = walker.blocks_per_cu;
    const uint32_t trav_blocks = (uint32_t)c->n_cus * trav_bpc;
    const uint32_t travf_blocks = (uint32_t)c->n_cus * (c->tune.travf_bpc > 0 ? (uint32_t)c->tune.travf_bpc : 6u), replay_blocks = (uint32_t)c->n_cus * 8u;
    const uint32_t conc_trav_bpc = c->tune.conc_trav_bpc > 0 ? (uint32_t)c->tune.conc_trav_bpc : trav_bpc;
    const uint32_t conc_travf_bpc = c->tune.conc_travf_bpc > 0 ? (uint32_t)c->tune.conc_travf_bpc : travf_blocks / (uint32_t)c->n_cus;

    // per-kernel timing: one event pair per launch, summed after the frame
    size_t ev_used = 0;
    std::vector<int> ev_kind;
    // one event pair per launch is ~0.4 ms per frame of extra barriers: nothing on a whole frame (109 ms), 3 %
    // of a 1/8 share, so multi-rank renders skip it unless asked (MI_RT_WF_KERNEL_TIMING=0/1 overrides)
    bool per_kernel_timing = a.R.world == 1;
    if (c->tune.kernel_timing >= 0) per_kernel_timing = c->tune.kernel_timing != 0;
    auto stamp = [&](int kind, hipStream_t on) -> int {      // kind: 0 wf_main, 1 wf_trav, 2 wf_reduce, 3 wf_trav_f, 4 wf_replay, 5 wf_main's class-A part on the second stream; call before AND after the launch
        if (!per_kernel_timing) return MI_OK;
        if (ev_used == c->wf_ev.size()) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return MI_ERR_HIP; c->wf_ev.push_back(e); }
        if (hipEventRecord(c->wf_ev[ev_used++], on) != hipSuccess) return MI_ERR_HIP;
        ev_kind.push_back(kind);
        return MI_OK;
    };
#define WF_TIMED_ON(kind, on, call) do { if (stamp(kind, on) != MI_OK) return fail(MI_ERR_HIP, "event"); HIP_TRY(call); if (stamp(kind, on) != MI_OK) return fail(MI_ERR_HIP, "event"); } while (0)
#define WF_TIMED(kind, call) WF_TIMED_ON(kind, stream, call)

    uint64_t counts[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    counts[4] = (uint64_t)a.npix * (range.end - range.begin); counts[5] = a.npix;
    // samples of dead tiles (nothing reachable from the tile: no ray is generated, no slot written or read) — only without signatures
    if (a.tile_mask && !d_sig) {
        uint64_t dead_px = 0;
        for (uint32_t t = (uint32_t)a.R.rank; t < a.R.tiles_total; t += (uint32_t)a.R.world) {
            if (!(c->h_tile_mask[(size_t)a.R.tiles_total + t] >> 63)) continue;
            const uint32_t x0 = (t % a.R.tiles_x) * MI_TILE, y0 = (t / a.R.tiles_x) * MI_TILE;
            if (x0 >= cam->screen_width || y0 >= cam->screen_height) continue;
            dead_px += (uint64_t)std::min<uint32_t>(MI_TILE, cam->screen_width - x0) * std::min<uint32_t>(MI_TILE, cam->screen_height - y0);
        }
        counts[7] = dead_px * (range.end - range.begin);
    }
    const bool have_walkers = ref_mask || ts_mask || c->S.n_meshes > 32;
    // Headers: wf_prefix stores {blocks, live paths, queue length, seq, class-B paths, class-A blocks} of every pass into a RING of
    // pinned host slots (slot = seq % kHdrRing), so the host may run a few passes ahead of the device and still read every header.
    struct PassHdr { uint32_t blocks, live, queue, live_b, blocks_a, segments; };
    auto header_ready = [&](uint32_t seq) { return ((volatile uint32_t*)c->h_hdr)[(size_t)(seq % kHdrRing) * 8 + 3] == seq; };
    auto read_header = [&](uint32_t seq) {
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        const volatile uint32_t* h = (volatile uint32_t*)c->h_hdr + (size_t)(seq % kHdrRing) * 8;
        PassHdr r = { h[0], h[1], h[2], h[4], h[5], h[6] };
        return r;
    };
    auto wait_header = [&](uint32_t seq) -> int {
        const auto t_wait = std::chrono::steady_clock::now();
        for (uint32_t spin = 1; !header_ready(seq); spin++) {
            if ((spin & 63u) == 0) {
                hipError_t q = hipStreamQuery(stream);
                if (q == hipSuccess) { if (header_ready(seq)) break; return fail(MI_ERR_HIP, "wavefront pipeline: stream drained without a header"); }
                if (q != hipErrorNotReady) return fail(MI_ERR_HIP, "wavefront pipeline: %s", hipGetErrorString(q));
                // a wedged stream neither drains nor errors: bound the wait by wall clock (one pass is milliseconds)
                const auto waited = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t_wait).count();
                if (waited > (long long)c->tune.spin_timeout_ms)
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
    };
    for (uint32_t s0 = range.begin; s0 < range.end; s0 += s_batch) {
        a.s_base = s0; a.s_count = (s0 + s_batch <= range.end) ? s_batch : (range.end - s0);
        int cur = 0;
        a.iter0 = 1;
        a.n_in = a.npix * a.s_count;
        HIP_TRY(hipMemsetAsync(cnt, 0, (3 * S_ + 8) * sizeof(uint32_t), stream));   // wf_prefix re-zeroes them after every pass
        const uint32_t seq0 = c->hdr_seq + 1u;          // seq of this batch's pass 0
        uint32_t seen = 0;                              // headers of passes [0, seen) have been read
        PassHdr last = { (a.n_in + kBlock - 1) / kBlock, a.n_in, 0u, 0u, 0u, 0u };      // "header of pass -1": the camera rays
        bool all_dead = false;
        auto consume = [&](bool count_it) {             // read header `seen` (it has arrived)
            last = read_header(seq0 + seen);
            seen++;
            if (count_it) { counts[0] += 1; counts[1] += last.live - last.live_b; counts[2] += last.live_b; counts[3] += last.queue; }
            counts[6] += last.segments;                 // every launched pass counts: a pass behind the one that ended every path ran no segment
            if (last.live == 0) all_dead = true;
        };
        uint32_t it = 0;
        for (; it <= cam->path_depth + 1u; it++) {
            while (seen < it && !all_dead && header_ready(seq0 + seen)) consume(true);
            if (all_dead) break;
            // The grid of pass `it` comes from the header of pass it - 1.  While that pass is still running the host would
            // have to wait for it (the header is on its way while the walkers run, so for a big pass the wait is hidden); a SMALL
            // pass is launched at once instead, on a grid that is an upper bound — live paths only decrease, and every (class,
            // shard) list may end in a partial block — whose surplus blocks leave at their first instruction (wf_main compares
            // its block number with the device-side table).  The host runs at most kRunAhead passes ahead of the headers.
            bool exact = seen == it;
            if (!exact) {
                const uint64_t bound = (uint64_t)last.live / kBlock + 2u * (uint64_t)kWfShards;
                if (c->tune.nowait_blocks == 0 || bound > (uint64_t)c->tune.nowait_blocks || it - seen > (uint32_t)kRunAhead) {
                    while (seen < it && !all_dead) { int rcw = wait_header(seq0 + seen); if (rcw != MI_OK) return rcw; consume(true); }
                    if (all_dead) break;
                    exact = true;
                }
            }
            uint32_t grid_all, grid_a;
            if (exact) { grid_all = last.blocks; grid_a = last.blocks_a; }
            else { grid_all = grid_a = (uint32_t)((uint64_t)last.live / kBlock) + 2u * (uint32_t)kWfShards; }
            if (it == 0) { grid_all = last.blocks; grid_a = 0; }
            if (grid_all == 0) break;
            // THE TAIL.  Once the live paths no longer fill the chip (last.live bounds this pass' input: paths only end), thin waves
            // cost nothing — there is nobody to give their lanes to — while every further pass costs two launches and a header.
            // So each wave keeps shading as long as ANY of its lanes can go on (a path that enters a mesh root still parks for
            // the walker).  Per path the operations and their order are those of the pass-by-pass schedule.  Without meshes
            // nothing ever parks: this launch ends every path and is the last one.
            // Threshold (MI_RT_WF_TAIL_PATHS): without meshes 4 Mi paths, the size below which passes are launched without waiting
            // (cfg1 as BASELINE states it, 400x400 / 16 spp: 0.64 ms at 0, 0.55 at 64 Ki ... 2 Mi, 0.49 from 3 Mi on; cfg1 / cfg5 at
            // 1080p unchanged up to 8 Mi); with meshes 1 Mi (a 1/8 share of cfg2: 11.0 ms up to 2 Mi, 11.1 at 4 Mi, 11.3 at 8 Mi).
            const uint32_t tail_paths = c->tune.tail_paths != 0xffffffffu ? c->tune.tail_paths : (have_walkers ? (1u << 20) : (4u << 20));
            const bool tail = it > 0 && tail_paths != 0 && last.live <= tail_paths;      // (the camera pass in this form too: 0.49 -> 0.58 ms on cfg1 as stated)
            a.fuse_max = tail ? cam->path_depth + 2u : fuse_max_normal;
            a.fuse_min = tail ? 1u : fuse_min_normal;
            a.st_in = a.iter0 ? nullptr : bufs[cur];
            a.st_out = bufs[cur ^ 1];
            a.n_blocks_in = grid_all;
            // A pass after the first is launched in TWO PARTS.  Its class-A blocks (paths whose pending hit is a plain Triangle /
            // Plane: nothing a walker could still change) go to a second stream, ordered only behind the previous pass' wf_prefix:
            // they fill the CUs the persistent walkers of that pass leave idle as their queue runs out (a walker launch ends
            // with ~0.1 ms of tail whatever its queue size, eleven times per frame and per rank).  The class-B blocks follow the
            // walkers on the main stream; wf_prefix waits for both parts.  Same blocks, same work, another schedule.
            const bool split = !a.iter0 && have_walkers && c->tune.split != 0 && (exact ? (grid_a >= 64u && grid_a < grid_all) : true);
            if (split) {
                HIP_TRY(hipStreamWaitEvent(c->aux_stream, c->ev_pfx, 0));
                a.part = 1;
                WF_TIMED_ON(5, c->aux_stream, launch_wf_main(a, grid_a, d_sig != nullptr, c->scene.gen_volumes, c->scene.mesh_maps, c->aux_stream));     // kind 5: its span includes waiting for CUs
                HIP_TRY(hipEventRecord(c->ev_part, c->aux_stream));
                a.part = 2;
                WF_TIMED(0, launch_wf_main(a, exact ? grid_all - grid_a : grid_all, d_sig != nullptr, c->scene.gen_volumes, c->scene.mesh_maps, stream));
                HIP_TRY(hipStreamWaitEvent(stream, c->ev_part, 0));
            } else {
                a.part = 0;
                WF_TIMED(0, launch_wf_main(a, grid_all, d_sig != nullptr, c->scene.gen_volumes, c->scene.mesh_maps, stream));
            }
            // device-side bookkeeping: tables for the next pass and for wf_trav, and the header the host needs (grid of the
            // next pass, anything alive?), which wf_prefix stores straight into pinned host memory: the compute stream never
            // waits for the host
            const uint32_t seq = ++c->hdr_seq;
            HIP_TRY(launch_wf_prefix(cnt, cnt + 2 * S_, d_in_count, d_in_pfx, d_trav_pfx, d_hdr, c->h_hdr_dev + (size_t)(seq % kHdrRing) * 8, seq, stream));
            if (have_walkers && c->tune.split != 0) HIP_TRY(hipEventRecord(c->ev_pfx, stream));
            // persistent walkers; they leave at once when the queue is empty.  Successive launches merge their meshes' hits
            // into the hit record (strictly closer wins, ties go to the lower Scene.objects index: order-independent)
            const bool ref_walk = ref_mask || c->S.n_meshes > 32;      // meshes 32, 33, ... have no mask bit: they always take the reference walk
            // Meshes of both kinds: wf_trav and wf_trav_f read the same work list and write different things (the hit record / the
            // candidate lists; each has its own cursor), so they go to two streams and wf_replay, which merges into the hit
            // record, follows both.  With full grids the F-tree walkers move in as the reference walkers run out of queue and leave
            // (HEAD 98.5 -> 96.5 ms).  Sharing every CU from the start — half the wave slots each — gains nothing: 68 ms for the
            // pair, exactly the 43 + 25 ms they take one after the other (VALU issue 0.71 + 0.34: together they saturate it).
            const bool side_by_side = ref_walk && ts_mask && c->tune.conc != 0;
            if (side_by_side) {
                HIP_TRY(hipEventRecord(c->ev_pfx, stream));
                HIP_TRY(hipStreamWaitEvent(c->aux2_stream, c->ev_pfx, 0));
            }
            if (ref_walk) {
                a.trav_mask = ref_mask;
                const uint32_t blocks = side_by_side ? (uint32_t)c->n_cus * conc_trav_bpc : trav_blocks;
                WF_TIMED(1, launch_walker(a, walker, blocks, &c->big_lds_enabled, stream));
            }
            if (ts_mask) {
                a.trav_mask = ts_mask;
                // wf_filter_f keeps the class-B paths whose ray enters a two-stage mesh's root box; wf_trav_f and wf_replay work on that list
                if (side_by_side) {
                    WF_TIMED_ON(3, c->aux2_stream, launch_wf_filter_f(a, 8u, c->aux2_stream));
                    WF_TIMED_ON(3, c->aux2_stream, launch_wf_trav_f(a, (uint32_t)c->n_cus * conc_travf_bpc, c->aux2_stream));
                    HIP_TRY(hipEventRecord(c->ev_travf, c->aux2_stream));
                    HIP_TRY(hipStreamWaitEvent(stream, c->ev_travf, 0));
                } else {
                    WF_TIMED(3, launch_wf_filter_f(a, 8u, stream));
                    WF_TIMED(3, launch_wf_trav_f(a, travf_blocks, stream));
                }
                WF_TIMED(4, launch_wf_replay(a, replay_blocks, stream));
            }
            cur ^= 1;
            a.iter0 = 0;
            if (tail && !have_walkers) { it++; break; }
        }
        WF_TIMED(2, launch_wf_reduce(a, s0 == 0, s0 + a.s_count >= spp, stream));
        // the headers not read yet (statistics; passes launched behind the one that ended every path are not counted)
        const uint32_t launched = c->hdr_seq + 1u - seq0;
        while (seen < launched) { int rcw = wait_header(seq0 + seen); if (rcw != MI_OK) return rcw; consume(!all_dead); }
    }
#undef WF_TIMED
#undef WF_TIMED_ON
    HIP_TRY(hipStreamSynchronize(stream));
    for (int k = 0; k < 8; k++) c->wf_counts[k] = counts[k];
    for (int k = 0; k < 8; k++) c->wf_ms[k] = 0.0f;
    c->wf_ms[3] = (float)(ev_used / 2);
    for (size_t e = 0; e + 1 < ev_used; e += 2) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, c->wf_ev[e], c->wf_ev[e + 1]) == hipSuccess) c->wf_ms[ev_kind[e] < 3 ? ev_kind[e] : ev_kind[e] + 1] += ms;
        if (c->tune.dump_launches) {
            static const char* const names[6] = { "wf_main", "wf_trav", "wf_reduce", "wf_trav_f", "wf_replay", "wf_main (class A, beside the walkers)" };
            fprintf(stderr, "[mi_rt] launch %zu %s %.4f ms\n", e / 2, names[ev_kind[e]], ms);
        }
    }
    return MI_OK;
}

static int render_tiles(mi_ctx* c, const mi_camera_desc* cam, const mi_render_opts* o, float* d_compact,
                        uint32_t* d_sig, hipStream_t stream, mi_stats* st, const SampleRange* partial = nullptr) {
    int rc = check_camera(cam);
    if (rc != MI_OK) return rc;
    if (!c->have_scene) return fail(MI_ERR_NO_SCENE, "no scene uploaded");
    if (!o || o->world < 1 || o->rank < 0 || o->rank >= o->world) return fail(MI_ERR_INVALID, "bad rank/world");
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
    make_camera(cam, &a.C);
    for (int k = 0; k < 3; k++) { a.C.light[k] = c->scene.point_light_pos[k]; a.C.ambient[k] = c->scene.ambient[k]; }
    const bool phong = cam->shading_mode == MI_SHADE_PHONG;      // debug shader: own kernel, `variant` is ignored
    // path_samples != 1 (tracing.rs:310) branches at every hit: the literal, recursive estimator (pt_branch)
    const bool recursive = !phong && (cam->path_samples != 1 || o->variant == MI_VARIANT_RECURSIVE);
    if (recursive && cam->path_depth > 64) return fail(MI_ERR_UNSUPPORTED, "recursive estimator: path_depth must be <= 64");
    uint32_t tx, ty, total, padded;
    tile_counts(cam, o->world, &tx, &ty, &total, &padded);
    a.R.seed = o->seed; a.R.rank = o->rank; a.R.world = o->world;
    a.R.tiles_x = tx; a.R.tiles_y = ty; a.R.tiles_total = total;
    a.R.my_tiles = (total > (uint32_t)o->rank) ? (total - (uint32_t)o->rank + (uint32_t)o->world - 1) / (uint32_t)o->world : 0;
    bool lds = c->S.n_meshes > 0 && c->scene.lds_bytes <= 64u * 1024u && !c->tune.global_bvh;
    a.R.lds_nodes = lds ? (uint32_t)c->S.n_nodes : 0;
    a.R.lds_tris = lds ? (uint32_t)c->S.n_tris : 0;
    a.seed_key = lowbias32(o->seed ^ 0x68e31da4u);
    a.out = d_compact;
    a.sig = (o->want_signature && d_sig) ? d_sig : nullptr;
    int variant = o->variant == MI_VARIANT_DEFAULT ? MI_VARIANT_WAVEFRONT : o->variant;
    if (variant != MI_VARIANT_SIMPLE && variant != MI_VARIANT_VOTED && variant != MI_VARIANT_VOTED_DIAG &&
        variant != MI_VARIANT_WAVEFRONT && variant != MI_VARIANT_RECURSIVE)
        return fail(MI_ERR_INVALID, "unknown variant %d (2, 5 and 6 were removed in ABI 3)", o->variant);
    const bool diag = variant == MI_VARIANT_VOTED_DIAG;
    a.R.vote_t = c->tune.vote_t; a.R.vote_a = c->tune.vote_a; a.R.k_steps = c->tune.k_steps;
    a.diag = nullptr;
    uint32_t n_blocks = padded * (uint32_t)kBlocksPerTile;
    if (diag) {
        a.diag = c->d_diag;
        HIP_TRY(hipMemsetAsync(c->d_diag, 0, 16 * sizeof(unsigned long long), stream));
    }
    WfArgs wa; uint32_t wf_batch = 1;
    if (variant == MI_VARIANT_WAVEFRONT && !phong && !recursive) {
        int rcp = wf_prepare(c, cam, padded, o->max_state_bytes, two_stage_mask(c, o->flags) != 0u, wa, wf_batch);
        if (rcp != MI_OK) return rcp;
    }
    HIP_TRY(hipEventRecord(c->ev_start, stream));
    if (phong)
        HIP_TRY(launch_phong(a, n_blocks, a.sig != nullptr, stream));
    else if (recursive)
        HIP_TRY(launch_branch(a, n_blocks, cam->path_samples, a.sig != nullptr, stream));
    else if (variant == MI_VARIANT_WAVEFRONT) {
        int rcw = render_tiles_wavefront(c, a, cam, wa, wf_batch, lds, o->flags, d_compact, a.sig, range, stream);
        if (rcw != MI_OK) return rcw;
    } else if (variant == MI_VARIANT_VOTED || variant == MI_VARIANT_VOTED_DIAG)
        HIP_TRY(launch_megakernel_voted(a, n_blocks, lds, a.sig != nullptr, diag, c->scene.gen_volumes, c->scene.lds_bytes + c->tune.lds_pad, stream));
    else
        HIP_TRY(launch_megakernel(a, n_blocks, lds, a.sig != nullptr, c->scene.lds_bytes, stream));
    HIP_TRY(hipEventRecord(c->ev_stop, stream));
    c->ev_recorded = true;
    if (st) {
        memset(st, 0, sizeof *st);
        uint64_t pixels = 0;
        for (uint32_t t = (uint32_t)o->rank; t < total; t += (uint32_t)o->world) {
            uint32_t x0 = (t % tx) * MI_TILE, y0 = (t / tx) * MI_TILE;
            if (x0 >= cam->screen_width) continue;               // a column of the numbering beyond the image (tile_counts)
            uint32_t w = cam->screen_width - x0 < MI_TILE ? cam->screen_width - x0 : MI_TILE;
            uint32_t h = cam->screen_height - y0 < MI_TILE ? cam->screen_height - y0 : MI_TILE;
            pixels += (uint64_t)w * h;
        }
        st->pixels = pixels;
        st->samples = pixels * (range.end - range.begin);
        st->tiles = a.R.my_tiles; st->tiles_padded = padded;
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
    uint32_t tx, ty, total, padded;
    tile_counts(cam, world, &tx, &ty, &total, &padded);
    HIP_TRY(launch_unpermute((const float*)d_gathered_f32, (float*)d_image_f32, cam->screen_width, cam->screen_height, tx,
                             (uint32_t)world, padded, (hipStream_t)stream));
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
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->ev_stop));
    HIP_TRY(hipEventElapsedTime(ms, c->ev_start, c->ev_stop));
    return MI_OK;
}

extern "C" int mi_reserve(mi_ctx* c, const mi_camera_desc* cam, int32_t world, uint64_t max_state_bytes) {
    if (!c) return fail(MI_ERR_INVALID, "ctx is NULL");
    int rc = check_camera(cam);
    if (rc != MI_OK) return rc;
    if (world < 1) return fail(MI_ERR_INVALID, "bad world");
    HIP_TRY(hipSetDevice(c->device));
    uint32_t tx, ty, total, padded;
    tile_counts(cam, world, &tx, &ty, &total, &padded);
    WfArgs a;
    memset(&a, 0, sizeof a);
    a.npix = padded * (uint32_t)kTilePixels;
    uint32_t s_batch = 1;
    return wf_alloc(c, a, cam->aa_sample_count, max_state_bytes, two_stage_mask(c, 0u) != 0u, s_batch);
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

extern "C" int mi_render(mi_ctx* c, const mi_camera_desc* cam, const mi_render_opts* opts, float* out_rgb_f32,
                         uint8_t* out_rgb_u8, uint32_t* out_sig, mi_stats* stats) {
    if (!c) return fail(MI_ERR_INVALID, "ctx is NULL");
    if (!opts) return fail(MI_ERR_INVALID, "opts is NULL");
    if (opts->rank != 0 || opts->world != 1) return fail(MI_ERR_INVALID, "mi_render renders a whole image: rank/world must be 0/1");
    int rc = check_camera(cam);
    if (rc != MI_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const hipEvent_t t0 = c->ev_t0, t1 = c->ev_t1;      // owned by the context: no early return can leak them
    uint32_t tx, ty, total, padded;
    tile_counts(cam, 1, &tx, &ty, &total, &padded);
    size_t npix = (size_t)cam->screen_width * cam->screen_height;
    size_t cbytes = (size_t)padded * kTilePixels * 3 * sizeof(float);
    if ((rc = ensure((void**)&c->d_compact, &c->compact_bytes, cbytes)) != MI_OK) return rc;
    if ((rc = ensure((void**)&c->d_image, &c->image_bytes, npix * 3 * sizeof(float))) != MI_OK) return rc;
    bool want_sig = opts->want_signature && out_sig;
    if (want_sig) {
        if ((rc = ensure((void**)&c->d_sigc, &c->sigc_bytes, (size_t)padded * kTilePixels * 4)) != MI_OK) return rc;
        if ((rc = ensure((void**)&c->d_sigi, &c->sigi_bytes, npix * 4)) != MI_OK) return rc;
    }
    mi_render_opts o = *opts;
    o.want_signature = want_sig ? 1 : 0;
    HIP_TRY(hipEventRecord(t0, c->stream));
    rc = render_tiles(c, cam, &o, c->d_compact, want_sig ? c->d_sigc : nullptr, c->stream, stats);
    if (rc != MI_OK) return rc;
    HIP_TRY(launch_unpermute(c->d_compact, c->d_image, cam->screen_width, cam->screen_height, tx, 1, padded, c->stream));
    if (out_rgb_f32) HIP_TRY(hipMemcpyAsync(out_rgb_f32, c->d_image, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (out_rgb_u8) {
        if ((rc = ensure((void**)&c->d_u8, &c->u8_bytes, npix * 3)) != MI_OK) return rc;
        HIP_TRY(launch_tonemap(c->d_image, c->d_u8, (uint32_t)npix, 1.0f / cam->gamma, c->stream));
        HIP_TRY(hipMemcpyAsync(out_rgb_u8, c->d_u8, npix * 3, hipMemcpyDeviceToHost, c->stream));
    }
    if (want_sig) {
        HIP_TRY(launch_sig_unpermute(c->d_sigc, c->d_sigi, cam->screen_width, cam->screen_height, tx, 1, padded, c->stream));
        HIP_TRY(hipMemcpyAsync(out_sig, c->d_sigi, npix * 4, hipMemcpyDeviceToHost, c->stream));
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
    uint32_t tx, ty, total, padded;
    tile_counts(cam, world, &tx, &ty, &total, &padded);
    const size_t slice_f = (size_t)padded * kTilePixels * 3, slice_s = (size_t)padded * kTilePixels;     // elements per rank
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
    HIP_TRY(launch_unpermute((const float*)m->d_compact[0], c0->d_image, cam->screen_width, cam->screen_height, tx, (uint32_t)world, padded, c0->stream));
    if (out_rgb_f32) HIP_TRY(hipMemcpyAsync(out_rgb_f32, c0->d_image, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c0->stream));
    HIP_TRY(launch_tonemap(c0->d_image, c0->d_u8, (uint32_t)npix, 1.0f / cam->gamma, c0->stream));
    if (out_rgb_u8) HIP_TRY(hipMemcpyAsync(out_rgb_u8, c0->d_u8, npix * 3, hipMemcpyDeviceToHost, c0->stream));
    if (want_sig) {
        HIP_TRY(launch_sig_unpermute((const uint32_t*)m->d_sig[0], (uint32_t*)m->d_sig_image, cam->screen_width, cam->screen_height, tx, (uint32_t)world, padded, c0->stream));
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
        stats->tiles_padded = padded; stats->scene_bytes = st[0].scene_bytes; stats->scene_in_lds = st[0].scene_in_lds;
        stats->total_ms = (float)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_begin).count() * 1e-3f;
    }
    return MI_OK;
}
