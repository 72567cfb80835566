// render_plan.hpp — the host-side decisions of a render: camera validation, the tile grid of the partition, the camera
// constants, the primary-ray tile masks, which meshes are walked two-stage, the wavefront pipeline's batch, and its pass schedule:
// what is fixed for a render (pass_schedule), whether a pass may be launched before the previous header has arrived (pass_gate), and
// its grids, parts and in-launch rounds (plan_pass); the buffers every launch of a lightmap finish reads and writes (finish_plan);
// and the layout and launches of a lightmap's mip chain (mip_plan).
// Host code only: no HIP call, no context; mi_rt.cpp plans with these, then launches.  All of it runs on the CPU:
// tests/test_render_plan_host.py, tests/test_pass_schedule_host.py and tests/test_finish_plan_host.py, through
// tests/cpp/render_plan_shim.cpp (mip_plan: tests/test_lightmap_mips_host.py through tests/cpp/mip_plan_shim.cpp); the launches a schedule leads to are pinned by tests/test_gpu_walkers.py (golden/pass_schedule_counts.json).
#pragma once
#include <cstdint>
#include <vector>

#include "scene_compile.hpp"

#pragma clang fp contract(off)

namespace pt {

// MI_OK, or MI_ERR_INVALID with the reason recorded (fail)
int check_camera(const mi_camera_desc* cam);
// Ray-table rendering (mi_render_rays): the rays are the caller's, so only the fields that call reads are checked — the image size,
// aa_sample_count (any value >= 1: the square exists for generate_rays' jitter grid only), path_samples, shading_mode, max_trace_dist
// and gamma — and rays_per_pixel, which is 1 or aa_sample_count.  eyepoint .. lens_radius may hold anything, non-finite values included.
// MI_OK, MI_ERR_INVALID or MI_ERR_UNSUPPORTED (path_samples != 1, Phong) with the reason recorded.
int check_table_camera(const mi_camera_desc* cam, uint32_t rays_per_pixel);
// `cam` with the fields a ray-table render ignores replaced by fixed finite values (what make_camera and tile_grid may then read)
mi_camera_desc table_camera(const mi_camera_desc* cam);

// The tile grid of the partition for `world` ranks (tile t -> rank t % world, slot t / world): tx tiles per row (the image's tile
// columns, rounded up to the next integer coprime with world), ty rows, total = tx * ty, padded = tiles per rank, rounded up.
struct TileGrid { uint32_t tx, ty, total, padded; };
TileGrid tile_grid(const mi_camera_desc* cam, int world);
uint32_t rank_tiles(const TileGrid& g, int rank, int world);                          // tiles of the numbering rank owns
uint64_t rank_pixels(const TileGrid& g, const mi_camera_desc* cam, int rank, int world);   // image pixels in them

// Camera::generate_rays constants in the reference's f32 operations (light / ambient are the scene's: left zero)
DCamera make_camera(const mi_camera_desc* cam);

// which meshes a render walks two-stage (bit m = live mesh m)
uint32_t two_stage_mask(const CompiledScene& sc, uint32_t flags);

// Primary-ray culling: for every tile of a row-major grid with `stride` tiles per row (tile_grid's tx), out[t] = the list
// Triangles / Spheres a camera ray of tile t can reach, out[tiles + t] = its meshes (low 32 bits) and, in bit 63, DEAD (nothing
// reachable).  Returns false (out untouched) when masking does not apply.
bool tile_masks(const CompiledScene& sc, const mi_camera_desc& cam, uint32_t flags, uint32_t stride, std::vector<uint64_t>& out);
// image pixels in rank's dead tiles (tile_masks' output over the same grid)
uint64_t dead_pixels(const TileGrid& g, const mi_camera_desc* cam, int rank, int world, const std::vector<uint64_t>& masks);

// The wavefront pipeline's memory: path state is streamed through HBM, 2 x 96 B (ping / pong) + 16 B sample slot per path, plus
// the two-stage candidates and header per queue slot when some mesh is walked two-stage.
constexpr size_t kWfBytesPerPath = 2 * (size_t)kWfPlanes * sizeof(float4) + sizeof(float4);
constexpr size_t kWfBytesPerPathTwoStage = (size_t)kCandMax * sizeof(uint2) + sizeof(uint2);

// Samples per pixel of the first batch to try for npix (padded) pixels at spp: the caller's budget max_state_bytes, or 60 % of
// free_bytes when it is 0; at most 2^31 paths, at least one sample, at most spp.  A budget below one sample per pixel is refused
// (MI_ERR_INVALID, recorded).
int wf_first_batch(uint32_t npix, uint32_t spp, uint64_t max_state_bytes, uint64_t free_bytes, bool two_stage, uint32_t* s_batch);

// What a batch of s_batch samples of npix pixels needs: the shards' region and the plane stride, and the bytes of each buffer
struct WfBatch { uint32_t region, cap; size_t state_bytes, samp_bytes, acc_bytes, cand_bytes, cand_hdr_bytes; };
WfBatch wf_batch(uint32_t npix, uint32_t s_batch);

// ---- the wavefront pipeline's pass schedule: what the host decides while it enqueues one pass (wf_main, wf_prefix, the walkers) per path segment
// The scheduling subset of the developer knobs (MI_RT_WF_*): mi_ctx::Tuning embeds it, mi_ctx_create reads it once
struct ScheduleKnobs {
    int split = 1;                          // wf_main in two parts, class A beside the previous pass' walkers (0 = one launch per pass)
    int conc = 1, conc_trav_bpc = 0, conc_travf_bpc = 0;   // wf_trav and wf_trav_f on two streams (0 = one after the other); their blocks per CU then (0 = the usual)
    int travf_bpc = 0;                      // wf_trav_f blocks per CU override (0 = default)
    uint32_t tail_paths = 0xffffffffu;      // a pass that starts with at most this many live paths runs every path as far as it can inside the launch (0 = never; default: automatic)
    uint32_t nowait_blocks = 16384;         // passes whose grid bound is at most this many blocks are launched without waiting for the previous header (0 = always wait)
    uint32_t fuse_max = 0, fuse_min = 32;   // wf_main: in-launch continuation (rounds: 0 = automatic; lanes needed)
};
constexpr uint32_t kRunAhead = 3;           // passes the host may launch before it has read the header of an earlier one
// The header of a pass as the host reads it from wf_prefix's slot (pt_device.h kHdr*), and the "header of pass -1": the camera rays
struct PassHdr { uint32_t blocks, live, queue, live_b, blocks_a, segments; };
PassHdr camera_pass_header(uint32_t n_in);
// Which meshes are walked how: ts = two-stage (wf_trav_f + wf_replay), ref = the rest, through the reference's tree (wf_trav).
// Bit m = live mesh m; meshes 32, 33, ... have no bit: they always take the reference walk.
struct WalkMasks { uint32_t ref, ts; };
WalkMasks walk_masks(const CompiledScene& sc, uint32_t flags);
// What is constant for the passes of one render
struct PassSchedule {
    uint32_t ref_mask, ts_mask;
    bool have_walkers, ref_walk, side_by_side;   // a pass has launches behind wf_prefix / wf_trav among them / wf_trav and wf_trav_f on two streams
    bool split_enabled;                     // passes may be launched in two parts (plan_pass decides per pass)
    uint32_t fuse_max, fuse_min, tail_fuse_max;   // in-launch rounds of a normal pass; a tail pass takes tail_fuse_max and 1
    uint32_t tail_paths, nowait_blocks;     // the knobs, tail_paths resolved (0 = never)
    uint32_t walker_blocks, travf_blocks, replay_blocks, filter_blocks_per_shard;   // grids as launched (side by side: the MI_RT_WF_CONC_*_BPC values)
};
PassSchedule pass_schedule(const CompiledScene& sc, WalkMasks masks, const WalkerPlan& walker, int n_cus, uint32_t path_depth, const ScheduleKnobs& knobs);
// May pass `it` be launched now, and on which grid: that of header it - 1, an upper bound (pass_grid_bound), or wait for the headers
// first?  `seen`: the headers of passes [0, seen) have been read; `live`: live paths in the last of them.
enum class PassGate { kExact, kBound, kWait };
uint32_t pass_grid_bound(uint32_t live);
PassGate pass_gate(const PassSchedule& s, uint32_t it, uint32_t seen, uint32_t live);
// Pass `it` of a batch from the last header read (`exact`: it is that of pass it - 1).  stop: nothing to launch, the batch is done;
// grid_all: the pass as one launch, grid_a / grid_b: its class-A / class-B part when split; last: this launch ends every path.
struct PassPlan { bool stop, split, tail, last; uint32_t grid_all, grid_a, grid_b, fuse_max, fuse_min; };
PassPlan plan_pass(const PassSchedule& s, uint32_t it, bool exact, const PassHdr& last);

// ---- the lightmap finish's pass plan: which buffer every launch of a finish (plain, SH or variance-guided) reads and writes
// A finish is an initial step (the mask kernel; with_var: the initial variance) and levels + dilate passes, the levels first, level p
// at step 1 << p.  The rules:
//   * pass 0 reads the caller's input, pass p what pass p - 1 wrote; pass p writes the caller's output when it is the last one,
//     otherwise image ping p & 1.  With no pass at all the mask kernel copies (copy = 1) the input into the caller's output.
//   * the mask after k dilations lives in the caller's buffer when k == dilate && want_valid, otherwise in mask ping k & 1: the initial
//     step writes the mask after 0, dilation k reads the mask after k and writes the mask after k + 1.
//   * the variance after k levels lives in the caller's buffer when k == levels && want_var, otherwise in variance ping k & 1: the
//     initial step writes the variance after 0, level k reads the variance after k and writes the variance after k + 1; the dilations
//     never touch it.
// kNone: the step does not touch that kind (a level's masks, a dilation's variances, every variance without with_var).
// CPU tests: tests/test_finish_plan_host.py.
enum class FinishImage : uint8_t { kInput, kOutput, kPing0, kPing1 };
enum class FinishMask : uint8_t { kPing0, kPing1, kCaller, kNone };
enum class FinishVar : uint8_t { kPing0, kPing1, kCaller, kNone };
struct FinishPass {
    bool level; uint32_t step;              // a filter level at `step`, or a dilation (step 0)
    FinishImage src, dst;
    FinishMask mask_in, mask_out;
    FinishVar var_in, var_out;
};
struct FinishPlan { uint32_t copy; FinishMask mask_init; FinishVar var_init; std::vector<FinishPass> passes; };
FinishPlan finish_plan(uint32_t levels, uint32_t dilate, bool want_valid, bool with_var, bool want_var);

// ---- the lightmap mip chain's layout and launches (mi_lightmap_mips, the _lod lookups; tracing.py lightmap_mip_layout is the same rule)
// `levels` counts level 0; 0 asks for the full chain, mip_full_chain(W, H) = 1 + ceil(log2(max(W, H))) levels (16 at 32768), whose last
// level is 1 x 1.  Level l is mip_extent(W, l) x mip_extent(H, l) = ceil(W / 2^l) x ceil(H / 2^l): texel (x, y) of level l covers the
// level-0 texels [x 2^l, (x + 1) 2^l) x [y 2^l, (y + 1) 2^l) that lie inside the image, power of two or not.  Levels 1 .. L - 1 lie
// tightly one after the other in one buffer: level[l].offset is where level l starts, in texels (level 0 is the image itself: offset 0).
// launches: lmm_reduce reads level `src` and writes the `count` levels src + 1 .. src + count, at most per_launch (itself at most
// kMipFuse, the levels a 32 x 32 tile reaches: 16, 8, 4, 2, 1); every level 1 .. L - 1 is written exactly once, in order, and a launch
// reads the last level the one before wrote.  CPU tests: tests/test_lightmap_mips_host.py.
// (kMipMaxLevels and kMipFuse: pt_device.h, beside the kernels' argument records)
struct MipLevel { uint32_t width, height; uint64_t offset; };
struct MipLaunch { uint32_t src, count; };
struct MipPlan { uint32_t levels; uint64_t texels; MipLevel level[kMipMaxLevels]; std::vector<MipLaunch> launches; };
inline uint32_t mip_extent(uint32_t n, uint32_t l) { return (n + (1u << l) - 1u) >> l; }
uint32_t mip_full_chain(uint32_t width, uint32_t height);
// false: width or height is not in 1 .. 32768 or `levels` is above the full chain (plan is left alone)
bool mip_plan(uint32_t width, uint32_t height, uint32_t levels, uint32_t per_launch, MipPlan* plan);

// ---- the block layout of a BC6H chain (mi_lightmap_bc6h_*, mi_lightmap_sample_bc6h; tracing.py lightmap_bc6h_layout is the same rule)
// Level l of a mip plan as bc6h_extent(W_l) x bc6h_extent(H_l) blocks of 16 bytes (4 x 4 texels), row-major in the level's own row order.
// Level 0 is a buffer of its own; level[l].offset is where level l >= 1 starts, in blocks, in the buffer that holds levels 1 .. L - 1
// one after the other (`blocks` of them).  CPU test: tests/test_lightmap_bc6h_host.py through tests/cpp/bc6h_lightmap_check.cpp.
struct Bc6hLevel { uint32_t bw, bh; uint64_t offset; };
struct Bc6hPlan { uint32_t levels; uint64_t blocks; Bc6hLevel level[kMipMaxLevels]; };
inline uint32_t bc6h_extent(uint32_t n) { return (n + 3u) >> 2; }
Bc6hPlan bc6h_plan(const MipPlan& mips);

}  // namespace pt
