// render_plan.hpp — the host-side decisions of a render: camera validation, the tile grid of the partition, the camera
// constants, the primary-ray tile masks, which meshes are walked two-stage, and the wavefront pipeline's batch.  Host code
// only: no HIP call, no context; mi_rt.cpp plans with these, then launches.
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

}  // namespace pt
