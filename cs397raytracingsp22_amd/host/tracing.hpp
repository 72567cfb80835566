// tracing.hpp — C++ host mirror of src/util/tracing.rs: Camera and Scene with the reference's
// field names.  Scene::render_to_image() keeps its meaning (tracing.rs:221-263) and becomes
// flatten -> mi_scene_upload -> mi_render through the C ABI of include/mi_rt.h.  Errors that the
// reference raises as panics surface as std::runtime_error carrying mi_last_error().
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "geometry.hpp"

namespace cs397 {

enum class CameraProjectionMode { Orthographic = MI_PROJ_ORTHOGRAPHIC, Perspective = MI_PROJ_PERSPECTIVE };   // tracing.rs:27-30
enum class ShadingMode { Phong = MI_SHADE_PHONG, PathTrace = MI_SHADE_PATHTRACE };                             // tracing.rs:32-35

struct Camera {                                        // tracing.rs:138-155, same fields
    Vec3 eyepoint{0.0f, 2.0f, 5.5f}; Vec3 view_dir{0.0f, 0.0f, -1.0f}; Vec3 up{0.0f, 1.0f, 0.0f};
    CameraProjectionMode projection_mode = CameraProjectionMode::Perspective;
    ShadingMode shading_mode = ShadingMode::PathTrace;
    uint32_t path_depth = 10, path_samples = 1, screen_width = 100, screen_height = 100;
    float focal_length = 0.6f, focus_dist = 5.0f, lens_radius = 0.0f;
    uint32_t aa_sample_count = 100;
    float max_trace_dist = 100.0f, gamma = 2.0f;

    mi_camera_desc flatten() const {
        mi_camera_desc c{};
        for (int i = 0; i < 3; i++) { c.eyepoint[i] = eyepoint[i]; c.view_dir[i] = view_dir[i]; c.up[i] = up[i]; }
        c.projection_mode = (int)projection_mode; c.shading_mode = (int)shading_mode;
        c.path_depth = path_depth; c.path_samples = path_samples; c.screen_width = screen_width; c.screen_height = screen_height;
        c.focal_length = focal_length; c.focus_dist = focus_dist; c.lens_radius = lens_radius;
        c.aa_sample_count = aa_sample_count; c.max_trace_dist = max_trace_dist; c.gamma = gamma;
        return c;
    }
};

struct RgbImage { uint32_t width = 0, height = 0; std::vector<uint8_t> data; };   // image::RgbImage byte layout

// Closest hits of a batch of caller-supplied rays (Scene::intersect_rays): one entry per ray, object = index into Scene.objects, -1 = None
struct RayHits {
    std::vector<int32_t> object; std::vector<float> distance;
    std::vector<float> hitpoint, normal, uv;           // [n][3], [n][3], [n][2]; empty with resolve = false, like flags and material
    std::vector<int32_t> flags;                        // bit 0 frontface, bit 1 has_tex_coords
    std::vector<mi_material> material;
};

inline void mi_check(int rc) { if (rc != MI_OK) throw std::runtime_error(std::string("mi_rt: ") + mi_last_error()); }

struct Scene : Intersectable {                         // tracing.rs:213-218; `impl Intersectable for Scene` :326
    Camera camera;
    std::vector<IntersectableRef> objects;
    const std::vector<IntersectableRef>* scene_objects() const override { return &objects; }
    void flatten(SceneBuilder& sb) const override { for (auto& o : objects) o->flatten(sb); }
    Vec3 point_light_pos{0.0f, 1.0f, 5.0f};            // read by ShadingMode::Phong only (tracing.rs:282,288)
    Vec3 ambient{0.1f, 0.1f, 0.1f};                    // Phong only (:292)

    // Scene::render_to_image (tracing.rs:221-263).  seed: the reference RNG is unseeded; device: HIP ordinal.
    // n_gpus > 0 renders on the first n_gpus devices of the node through mi_multi_* (tiles t % n, one RCCL fan-in per
    // frame inside the library) — the drop-in for rayon's row parallelism (tracing.rs:228); the image is the same.
    RgbImage render_to_image(uint32_t seed = 1, int device = 0, mi_stats* stats = nullptr, std::vector<float>* linear = nullptr,
                             int n_gpus = 0) const {
        SceneBuilder sb;
        for (auto& o : objects) o->flatten(sb);
        mi_scene_desc d = sb.desc();
        for (int k = 0; k < 3; k++) { d.point_light_pos[k] = point_light_pos[k]; d.ambient[k] = ambient[k]; }
        mi_camera_desc cam = camera.flatten();
        RgbImage img; img.width = camera.screen_width; img.height = camera.screen_height;
        img.data.resize((size_t)img.width * img.height * 3);
        if (linear) linear->resize(img.data.size());
        mi_render_opts opts{}; opts.seed = seed; opts.rank = 0; opts.world = 1;
        int rc; std::string err;
        if (n_gpus > 0) {
            mi_multi* m = nullptr;
            mi_check(mi_multi_create(n_gpus, nullptr, &m));
            rc = mi_multi_scene_upload(m, &d);
            if (rc == MI_OK) rc = mi_multi_render(m, &cam, &opts, linear ? linear->data() : nullptr, img.data.data(), nullptr, stats);
            err = rc == MI_OK ? "" : mi_last_error();
            mi_multi_destroy(m);
        } else {
            mi_ctx* ctx = nullptr;
            mi_check(mi_ctx_create(device, &ctx));
            rc = mi_scene_upload(ctx, &d);
            if (rc == MI_OK) rc = mi_render(ctx, &cam, &opts, linear ? linear->data() : nullptr, img.data.data(), nullptr, stats);
            err = rc == MI_OK ? "" : mi_last_error();
            mi_ctx_destroy(ctx);
        }
        if (rc != MI_OK) throw std::runtime_error("mi_rt: " + err);
        return img;
    }

    // `impl Intersectable for Scene`, Scene::intersect_ray (tracing.rs:326-346), for n rays of the caller's making through mi_intersect_rays:
    // origins / dirs are [n][3], directions are used as given.  Ray i draws from the stream (seed, first_key + i, 0).  resolve = false asks
    // for object and distance only (the visibility form).
    RayHits intersect_rays(const std::vector<float>& origins, const std::vector<float>& dirs, float t_min = 0.001f, float t_max = INFINITY,
                           uint32_t seed = 1, uint32_t first_key = 0, bool resolve = true, int device = 0) const {
        if (origins.size() != dirs.size() || origins.size() % 3 != 0) throw std::runtime_error("mi_rt: origins and dirs must both be [n][3]");
        const size_t n = origins.size() / 3;
        RayHits h; h.object.resize(n); h.distance.resize(n);
        if (resolve) { h.hitpoint.resize(3 * n); h.normal.resize(3 * n); h.uv.resize(2 * n); h.flags.resize(n); h.material.resize(n); }
        with_context(device, [&](mi_ctx* ctx) {
            return mi_intersect_rays(ctx, (uint32_t)n, origins.data(), dirs.data(), t_min, t_max, seed, first_key, h.object.data(), h.distance.data(),
                                     resolve ? h.hitpoint.data() : nullptr, resolve ? h.normal.data() : nullptr, resolve ? h.flags.data() : nullptr,
                                     resolve ? h.uv.data() : nullptr, resolve ? h.material.data() : nullptr);
        });
        return h;
    }

    // Is Scene::intersect_ray(ray_i, t_min, t_max_i) (tracing.rs:326-346) Some?  The any-hit query through mi_occluded_rays -> [n] bytes, 0 / 1.
    // ray_t_max: empty, or one t_max per ray (replaces t_max).  Directions are used as given: the segment a -> b is origin a, dir b - a,
    // [eps, 1 - eps].  Ray i draws from the stream (seed, first_key + i, 0).
    std::vector<uint8_t> occluded_rays(const std::vector<float>& origins, const std::vector<float>& dirs, float t_min = 0.001f,
                                       float t_max = INFINITY, const std::vector<float>& ray_t_max = {}, uint32_t seed = 1,
                                       uint32_t first_key = 0, int device = 0) const {
        if (origins.size() != dirs.size() || origins.size() % 3 != 0) throw std::runtime_error("mi_rt: origins and dirs must both be [n][3]");
        const size_t n = origins.size() / 3;
        if (!ray_t_max.empty() && ray_t_max.size() != n) throw std::runtime_error("mi_rt: ray_t_max must hold one value per ray");
        std::vector<uint8_t> occluded(n);
        with_context(device, [&](mi_ctx* ctx) {
            return mi_occluded_rays(ctx, (uint32_t)n, origins.data(), dirs.data(), t_min, t_max, ray_t_max.empty() ? nullptr : ray_t_max.data(),
                                    seed, first_key, occluded.data());
        });
        return occluded;
    }

    // Ambient-occlusion baking with rays made on the GPU through mi_hemisphere_occlusion: per surface point, how many of n_samples hemisphere
    // rays about its normal are NOT occluded within [t_min, t_max] (`open`, [n]) and the sum of the open directions (`bent`, [n][3]).
    // Sample s = first_sample + k of point i: direction from Lambertian::scatter's sample_hemisphere on the stream (seed, first_key + i, 2s),
    // the ray's own stream (seed, first_key + i, 2s + 1); normal and direction are used as given.  flags: 0 or MI_HEMI_WORLD_RADIUS (t_max
    // is a world-space radius).  Split by points (first_key advanced) or by samples (first_sample advanced): the counts of one call, exactly.
    struct HemisphereOcclusion { std::vector<uint32_t> open; std::vector<float> bent; };
    HemisphereOcclusion hemisphere_occlusion(const std::vector<float>& points, const std::vector<float>& normals, uint32_t n_samples,
                                             float t_min = 0.001f, float t_max = INFINITY, uint32_t flags = 0, uint32_t seed = 1,
                                             uint32_t first_key = 0, uint32_t first_sample = 0, int device = 0) const {
        if (points.size() != normals.size() || points.size() % 3 != 0) throw std::runtime_error("mi_rt: points and normals must both be [n][3]");
        if (n_samples == 0 || n_samples > 65535) throw std::runtime_error("mi_rt: n_samples must be in 1 .. 65535");
        const size_t n = points.size() / 3;
        HemisphereOcclusion h; h.open.resize(n); h.bent.resize(3 * n);
        with_context(device, [&](mi_ctx* ctx) {
            return mi_hemisphere_occlusion(ctx, (uint32_t)n, points.data(), normals.data(), first_sample, n_samples, t_min, t_max, flags, seed,
                                           first_key, h.open.data(), h.bent.data());
        });
        return h;
    }

    // Scene::shade_ray (tracing.rs:300-324) at level 0 for n rays through mi_shade_rays -> [n][3] radiance; the camera supplies path_depth,
    // path_samples and max_trace_dist.
    std::vector<float> shade_rays(const std::vector<float>& origins, const std::vector<float>& dirs, uint32_t seed = 1, uint32_t first_key = 0,
                                  int device = 0) const {
        if (origins.size() != dirs.size() || origins.size() % 3 != 0) throw std::runtime_error("mi_rt: origins and dirs must both be [n][3]");
        if (camera.path_samples == 0) throw std::runtime_error("mi_rt: path_samples must be >= 1 (tracing.rs:318 divides by it)");
        if (camera.max_trace_dist != camera.max_trace_dist) throw std::runtime_error("mi_rt: max_trace_dist must not be NaN");
        std::vector<float> rgb(origins.size());
        const mi_camera_desc cam = camera.flatten();
        with_context(device, [&](mi_ctx* ctx) {
            return mi_shade_rays(ctx, &cam, (uint32_t)(origins.size() / 3), origins.data(), dirs.data(), seed, first_key, rgb.data());
        });
        return rgb;
    }

    // Scene::render_to_image (tracing.rs:221-263) with a ray table in place of Camera::generate_rays, through mi_render_rays: origins / dirs
    // are [rays_per_pixel][H][W][3], rays_per_pixel = 1 or camera.aa_sample_count (any value, not only squares).  Sample s of pixel (x, y)
    // draws from the stream (seed, y * W + x, s); directions are used as given; the camera's pose, projection and lens fields are ignored.
    RgbImage render_rays(const std::vector<float>& origins, const std::vector<float>& dirs, uint32_t rays_per_pixel, uint32_t seed = 1,
                         int device = 0, mi_stats* stats = nullptr, std::vector<float>* linear = nullptr) const {
        const size_t n = (size_t)rays_per_pixel * camera.screen_height * camera.screen_width * 3;
        if (origins.size() != n || dirs.size() != n) throw std::runtime_error("mi_rt: origins and dirs must both be [rays_per_pixel][H][W][3]");
        const mi_camera_desc cam = camera.flatten();
        RgbImage img; img.width = camera.screen_width; img.height = camera.screen_height;
        img.data.resize((size_t)img.width * img.height * 3);
        if (linear) linear->resize(img.data.size());
        mi_render_opts opts{}; opts.seed = seed; opts.rank = 0; opts.world = 1;
        with_context(device, [&](mi_ctx* ctx) {
            return mi_render_rays(ctx, &cam, &opts, origins.data(), dirs.data(), rays_per_pixel, linear ? linear->data() : nullptr,
                                  img.data.data(), nullptr, stats);
        });
        return img;
    }

    // Lightmap baking through mi_render_points: points / normals are [rows_per_pixel][H][W][3], rows_per_pixel = 1 or camera.aa_sample_count.
    // Sample s of texel (x, y) leaves its point along sample_hemisphere(normal) (materials.rs:171-178), drawn on the GPU from the stream
    // (seed, W * H + y * W + x, s); its path draws from (seed, y * W + x, s), so the image is render_rays' for those directions.  A zero
    // normal marks an empty texel (black); points are used as given (the caller offsets them along the normal).
    RgbImage render_points(const std::vector<float>& points, const std::vector<float>& normals, uint32_t rows_per_pixel, uint32_t seed = 1,
                           int device = 0, mi_stats* stats = nullptr, std::vector<float>* linear = nullptr) const {
        const size_t n = (size_t)rows_per_pixel * camera.screen_height * camera.screen_width * 3;
        if (points.size() != n || normals.size() != n) throw std::runtime_error("mi_rt: points and normals must both be [rows_per_pixel][H][W][3]");
        const mi_camera_desc cam = camera.flatten();
        RgbImage img; img.width = camera.screen_width; img.height = camera.screen_height;
        img.data.resize((size_t)img.width * img.height * 3);
        if (linear) linear->resize(img.data.size());
        mi_render_opts opts{}; opts.seed = seed; opts.rank = 0; opts.world = 1;
        with_context(device, [&](mi_ctx* ctx) {
            return mi_render_points(ctx, &cam, &opts, points.data(), normals.data(), rows_per_pixel, linear ? linear->data() : nullptr,
                                    img.data.data(), nullptr, stats);
        });
        return img;
    }

    // The lightmap of `mesh` through mi_bake_lightmap: its uv atlas, width x height texels, is rasterised on the GPU into the point table
    // render_points would take and gathered with `samples` samples per texel, each from its own jittered position inside the texel
    // (jitter) or all from the centre; `offset` lifts the points off the surface along the normal.  Of `mesh` the four arrays, the two
    // counts and transform are read.  The camera supplies path_depth, max_trace_dist and gamma.
    RgbImage bake_lightmap(const mi_mesh& mesh, uint32_t width, uint32_t height, uint32_t samples, bool jitter = true, float offset = 1e-3f,
                           uint32_t seed = 1, int device = 0, mi_stats* stats = nullptr) const {
        mi_camera_desc cam = camera.flatten();
        cam.screen_width = width; cam.screen_height = height; cam.aa_sample_count = samples;
        RgbImage img; img.width = width; img.height = height;
        img.data.resize((size_t)width * height * 3);
        mi_render_opts opts{}; opts.seed = seed; opts.rank = 0; opts.world = 1;
        with_context(device, [&](mi_ctx* ctx) {
            return mi_bake_lightmap(ctx, &cam, &opts, &mesh, jitter ? MI_LM_JITTER : 0u, offset, nullptr, img.data.data(), nullptr, nullptr, stats);
        });
        return img;
    }

    // Finish a baked lightmap through mi_lightmap_finish: the edge-aware a-trous filter guided by the atlas's centre table (points / normals:
    // mi_lightmap_texels with rows = 1, no jitter), then `dilate` passes of gutter dilation.  image / points / normals are [H][W][3]; `image` is
    // the bake's f32 image (bake-side `linear`).  INFINITY turns sigma_plane, reach or sigma_color off.  Returns the finished [H][W][3] image;
    // `valid` takes the [H][W] mask (1 = covered or filled by the dilation).  Needs no scene: a static member.
    static std::vector<float> finish_lightmap(const std::vector<float>& image, const std::vector<float>& points, const std::vector<float>& normals,
                                              uint32_t width, uint32_t height, uint32_t levels = 3, uint32_t normal_power_log2 = 5,
                                              float sigma_plane = INFINITY, float reach = INFINITY, float sigma_color = INFINITY,
                                              uint32_t dilate = 4, int device = 0, std::vector<uint8_t>* valid = nullptr) {
        const size_t n = (size_t)width * height;
        if (image.size() != n * 3 || points.size() != n * 3 || normals.size() != n * 3)
            throw std::runtime_error("mi_rt: image, points and normals must all be [H][W][3]");
        std::vector<float> out(n * 3);
        if (valid) valid->resize(n);
        mi_ctx* ctx = nullptr;
        mi_check(mi_ctx_create(device, &ctx));
        const int rc = mi_lightmap_finish(ctx, width, height, image.data(), points.data(), normals.data(), levels, normal_power_log2, sigma_plane,
                                          reach, sigma_color, dilate, out.data(), valid ? valid->data() : nullptr);
        const std::string err = rc == MI_OK ? "" : mi_last_error();
        mi_ctx_destroy(ctx);
        if (rc != MI_OK) throw std::runtime_error("mi_rt: " + err);
        return out;
    }

    // bake_lightmap with the second moments, through mi_bake_lightmap_moments: returns the bake's f32 mean [H][W][3]; `m2` takes, per texel
    // and channel, the mean of the squares of its `samples` samples: what finish_lightmap_var takes.  `image` takes the tone-mapped bytes.
    std::vector<float> bake_lightmap_moments(const mi_mesh& mesh, uint32_t width, uint32_t height, uint32_t samples, std::vector<float>& m2,
                                             bool jitter = true, float offset = 1e-3f, uint32_t seed = 1, int device = 0,
                                             mi_stats* stats = nullptr, RgbImage* image = nullptr) const {
        mi_camera_desc cam = camera.flatten();
        cam.screen_width = width; cam.screen_height = height; cam.aa_sample_count = samples;
        std::vector<float> mean((size_t)width * height * 3);
        m2.resize(mean.size());
        if (image) { image->width = width; image->height = height; image->data.resize(mean.size()); }
        mi_render_opts opts{}; opts.seed = seed; opts.rank = 0; opts.world = 1;
        with_context(device, [&](mi_ctx* ctx) {
            return mi_bake_lightmap_moments(ctx, &cam, &opts, &mesh, jitter ? MI_LM_JITTER : 0u, offset, m2.data(), mean.data(),
                                            image ? image->data.data() : nullptr, nullptr, nullptr, stats);
        });
        return mean;
    }

    // Finish a baked lightmap through mi_lightmap_finish_var: finish_lightmap whose colour weight is `sigma_color` standard errors of each
    // texel's own mean wide (plus color_floor; INFINITY turns the weight off), from the bake's second moments `m2` [H][W][3] and its sample
    // count.  Returns the finished image; `var` takes the [H][W] variance of the result, `valid` the mask.  A static member.
    static std::vector<float> finish_lightmap_var(const std::vector<float>& image, const std::vector<float>& m2, uint32_t samples,
                                                  const std::vector<float>& points, const std::vector<float>& normals, uint32_t width,
                                                  uint32_t height, uint32_t levels = 3, uint32_t normal_power_log2 = 5,
                                                  float sigma_plane = INFINITY, float reach = INFINITY, float sigma_color = 8.0f,
                                                  float color_floor = 1e-6f, uint32_t dilate = 4, int device = 0,
                                                  std::vector<float>* var = nullptr, std::vector<uint8_t>* valid = nullptr) {
        const size_t n = (size_t)width * height;
        if (image.size() != n * 3 || m2.size() != n * 3 || points.size() != n * 3 || normals.size() != n * 3)
            throw std::runtime_error("mi_rt: image, m2, points and normals must all be [H][W][3]");
        std::vector<float> out(n * 3);
        if (var) var->resize(n);
        if (valid) valid->resize(n);
        mi_ctx* ctx = nullptr;
        mi_check(mi_ctx_create(device, &ctx));
        const int rc = mi_lightmap_finish_var(ctx, width, height, image.data(), m2.data(), samples, points.data(), normals.data(), levels,
                                              normal_power_log2, sigma_plane, reach, sigma_color, color_floor, dilate, out.data(),
                                              var ? var->data() : nullptr, valid ? valid->data() : nullptr);
        const std::string err = rc == MI_OK ? "" : mi_last_error();
        mi_ctx_destroy(ctx);
        if (rc != MI_OK) throw std::runtime_error("mi_rt: " + err);
        return out;
    }

    // The adaptive bake, through mi_bake_lightmap_adaptive: every texel gets ad.first_samples samples, then up to ad.max_rounds rounds of
    // ad.round_samples more go to the texels whose blurred standard error exceeds ad.target_rel * luminance + ad.target_abs.  Returns the
    // merged f32 mean [H][W][3]; `m2` takes the merged means of squares, `counts` the samples behind each texel [H][W]: what
    // finish_lightmap_var_counts takes.  `image` takes the tone-mapped bytes.
    std::vector<float> bake_lightmap_adaptive(const mi_mesh& mesh, uint32_t width, uint32_t height, const mi_lightmap_adaptive& ad,
                                              std::vector<float>& m2, std::vector<uint32_t>& counts, bool jitter = true, float offset = 1e-3f,
                                              uint32_t seed = 1, int device = 0, mi_stats* stats = nullptr, RgbImage* image = nullptr) const {
        mi_camera_desc cam = camera.flatten();
        cam.screen_width = width; cam.screen_height = height; cam.aa_sample_count = ad.first_samples;
        std::vector<float> mean((size_t)width * height * 3);
        m2.resize(mean.size());
        counts.resize((size_t)width * height);
        if (image) { image->width = width; image->height = height; image->data.resize(mean.size()); }
        mi_render_opts opts{}; opts.seed = seed; opts.rank = 0; opts.world = 1;
        with_context(device, [&](mi_ctx* ctx) {
            return mi_bake_lightmap_adaptive(ctx, &cam, &opts, &mesh, jitter ? MI_LM_JITTER : 0u, offset, &ad, counts.data(), m2.data(),
                                             mean.data(), image ? image->data.data() : nullptr, nullptr, nullptr, stats);
        });
        return mean;
    }

    // finish_lightmap_var for an adaptive bake, through mi_lightmap_finish_var_counts: `counts` [H][W] holds every texel's own sample
    // count in the place of `samples`.  A static member.
    static std::vector<float> finish_lightmap_var_counts(const std::vector<float>& image, const std::vector<float>& m2,
                                                         const std::vector<uint32_t>& counts, const std::vector<float>& points,
                                                         const std::vector<float>& normals, uint32_t width, uint32_t height,
                                                         uint32_t levels = 3, uint32_t normal_power_log2 = 5, float sigma_plane = INFINITY,
                                                         float reach = INFINITY, float sigma_color = 8.0f, float color_floor = 1e-6f,
                                                         uint32_t dilate = 4, int device = 0, std::vector<float>* var = nullptr,
                                                         std::vector<uint8_t>* valid = nullptr) {
        const size_t n = (size_t)width * height;
        if (image.size() != n * 3 || m2.size() != n * 3 || points.size() != n * 3 || normals.size() != n * 3 || counts.size() != n)
            throw std::runtime_error("mi_rt: image, m2, points and normals must all be [H][W][3] and counts [H][W]");
        std::vector<float> out(n * 3);
        if (var) var->resize(n);
        if (valid) valid->resize(n);
        mi_ctx* ctx = nullptr;
        mi_check(mi_ctx_create(device, &ctx));
        const int rc = mi_lightmap_finish_var_counts(ctx, width, height, image.data(), m2.data(), counts.data(), points.data(), normals.data(),
                                                     levels, normal_power_log2, sigma_plane, reach, sigma_color, color_floor, dilate,
                                                     out.data(), var ? var->data() : nullptr, valid ? valid->data() : nullptr);
        const std::string err = rc == MI_OK ? "" : mi_last_error();
        mi_ctx_destroy(ctx);
        if (rc != MI_OK) throw std::runtime_error("mi_rt: " + err);
        return out;
    }

    // Light probes through mi_render_probes: points is [rows_per_pixel][H][W][3], one probe position per pixel, rows_per_pixel = 1 or
    // camera.aa_sample_count.  Sample s of probe (x, y) leaves its point along rand_sphere_vec (Isotropic::scatter's direction,
    // materials.rs:158-166: uniform over the sphere), drawn on the GPU from the stream (seed, W * H + y * W + x, s); its path draws from
    // (seed, y * W + x, s).  Returns the SH L2 radiance coefficients [H][W][9][3] (the basis and its order: mi_rt.h); `image` takes the
    // tone-mapped mean, `linear` the f32 mean.
    std::vector<float> render_probes(const std::vector<float>& points, uint32_t rows_per_pixel, uint32_t seed = 1, int device = 0,
                                     mi_stats* stats = nullptr, RgbImage* image = nullptr, std::vector<float>* linear = nullptr) const {
        const size_t n = (size_t)camera.screen_height * camera.screen_width;
        if (points.size() != n * rows_per_pixel * 3) throw std::runtime_error("mi_rt: points must be [rows_per_pixel][H][W][3]");
        const mi_camera_desc cam = camera.flatten();
        std::vector<float> sh(n * 27);
        if (image) { image->width = camera.screen_width; image->height = camera.screen_height; image->data.resize(n * 3); }
        if (linear) linear->resize(n * 3);
        mi_render_opts opts{}; opts.seed = seed; opts.rank = 0; opts.world = 1;
        with_context(device, [&](mi_ctx* ctx) {
            return mi_render_probes(ctx, &cam, &opts, points.data(), rows_per_pixel, sh.data(), linear ? linear->data() : nullptr,
                                    image ? image->data.data() : nullptr, nullptr, stats);
        });
        return sh;
    }

    // Sample an irradiance volume through mi_probe_volume_sample: `sh` holds the first nx * ny * nz records ([9][3] each) of render_probes'
    // result for the probe grid of the box [lo, hi] (probe (i, j, k) has number (k * ny + j) * nx + i and sits at the centre of its cell);
    // `valid` is empty (every probe takes part) or one byte per probe (0 = takes no part).  points / normals are [n][3]; every point is lit
    // through its normal: trilinear interpolation of the eight probes around it, convolved with the clamped cosine lobe; normal_weight sets
    // MI_PV_NORMAL_WEIGHT.  An all-zero normal marks an empty texel (+0.0, weight 0).  Returns the irradiance [n][3]; `weight` takes the
    // weight sum per point (0: every corner was invalid).  Needs no scene: a static member.
    static std::vector<float> sample_probe_volume(const float lo[3], const float hi[3], const uint32_t counts[3], const std::vector<float>& sh,
                                                  const std::vector<uint8_t>& valid, bool normal_weight, const std::vector<float>& points,
                                                  const std::vector<float>& normals, int device = 0, std::vector<float>* weight = nullptr) {
        const size_t n_probes = (size_t)counts[0] * counts[1] * counts[2], n = points.size() / 3;
        if (sh.size() != n_probes * 27 || (!valid.empty() && valid.size() != n_probes))
            throw std::runtime_error("mi_rt: sh must be [nx ny nz][9][3] and valid empty or [nx ny nz]");
        if (points.size() != n * 3 || normals.size() != points.size()) throw std::runtime_error("mi_rt: points and normals must both be [n][3]");
        mi_probe_volume v{};
        for (int a = 0; a < 3; a++) { v.lo[a] = lo[a]; v.hi[a] = hi[a]; v.counts[a] = counts[a]; }
        v.flags = normal_weight ? MI_PV_NORMAL_WEIGHT : 0u;
        v.sh = sh.data(); v.valid = valid.empty() ? nullptr : valid.data();
        std::vector<float> out(n * 3);
        if (weight) weight->resize(n);
        if (n == 0) return out;                              // (an empty vector has no address to pass)
        mi_ctx* ctx = nullptr;
        mi_check(mi_ctx_create(device, &ctx));
        const int rc = mi_probe_volume_sample(ctx, &v, (uint32_t)n, points.data(), normals.data(), out.data(), weight ? weight->data() : nullptr);
        const std::string err = rc == MI_OK ? "" : mi_last_error();
        mi_ctx_destroy(ctx);
        if (rc != MI_OK) throw std::runtime_error("mi_rt: " + err);
        return out;
    }

    // A directional lightmap through mi_bake_lightmap_sh: bake_lightmap that returns, per texel, the SH L2 radiance records [H][W][9][3]
    // (mi_render_probes' basis and order, scaled for the hemisphere's uniform directions), from which eval_lightmap_sh gives the
    // irradiance at any normal.  `linear` takes the f32 mean bake_lightmap's image is made of, `image` the tone-mapped bytes.
    std::vector<float> bake_lightmap_sh(const mi_mesh& mesh, uint32_t width, uint32_t height, uint32_t samples, bool jitter = true,
                                        float offset = 1e-3f, uint32_t seed = 1, int device = 0, mi_stats* stats = nullptr,
                                        RgbImage* image = nullptr, std::vector<float>* linear = nullptr) const {
        mi_camera_desc cam = camera.flatten();
        cam.screen_width = width; cam.screen_height = height; cam.aa_sample_count = samples;
        const size_t n = (size_t)width * height;
        std::vector<float> sh(n * 27);
        if (image) { image->width = width; image->height = height; image->data.resize(n * 3); }
        if (linear) linear->resize(n * 3);
        mi_render_opts opts{}; opts.seed = seed; opts.rank = 0; opts.world = 1;
        with_context(device, [&](mi_ctx* ctx) {
            return mi_bake_lightmap_sh(ctx, &cam, &opts, &mesh, jitter ? MI_LM_JITTER : 0u, offset, sh.data(), linear ? linear->data() : nullptr,
                                       image ? image->data.data() : nullptr, nullptr, nullptr, stats);
        });
        return sh;
    }

    // Finish a directional lightmap through mi_lightmap_finish_sh: finish_lightmap for [H][W][9][3] records; the colour weight is taken
    // from the three k = 0 coefficients and one weight per tap serves all 27 channels.  Returns the finished records; `valid` takes the
    // mask.  Needs no scene: a static member.
    static std::vector<float> finish_lightmap_sh(const std::vector<float>& sh, const std::vector<float>& points, const std::vector<float>& normals,
                                                 uint32_t width, uint32_t height, uint32_t levels = 3, uint32_t normal_power_log2 = 5,
                                                 float sigma_plane = INFINITY, float reach = INFINITY, float sigma_color = INFINITY,
                                                 uint32_t dilate = 4, int device = 0, std::vector<uint8_t>* valid = nullptr) {
        const size_t n = (size_t)width * height;
        if (sh.size() != n * 27 || points.size() != n * 3 || normals.size() != n * 3)
            throw std::runtime_error("mi_rt: sh must be [H][W][9][3], points and normals [H][W][3]");
        std::vector<float> out(n * 27);
        if (valid) valid->resize(n);
        mi_ctx* ctx = nullptr;
        mi_check(mi_ctx_create(device, &ctx));
        const int rc = mi_lightmap_finish_sh(ctx, width, height, sh.data(), points.data(), normals.data(), levels, normal_power_log2, sigma_plane,
                                             reach, sigma_color, dilate, out.data(), valid ? valid->data() : nullptr);
        const std::string err = rc == MI_OK ? "" : mi_last_error();
        mi_ctx_destroy(ctx);
        if (rc != MI_OK) throw std::runtime_error("mi_rt: " + err);
        return out;
    }

    // The irradiance of a directional lightmap through mi_lightmap_sh_eval: sh is [n][9][3], normals [n][3] (an atlas: n = W * H, its own
    // normal table for the plain irradiance map, normal-mapped normals for the detail).  An all-zero normal gives +0.0; the result is not
    // clamped (SH ringing can take it slightly below zero).  Returns [n][3].  Needs no scene: a static member.
    static std::vector<float> eval_lightmap_sh(const std::vector<float>& sh, const std::vector<float>& normals, int device = 0) {
        const size_t n = normals.size() / 3;
        if (normals.size() != n * 3 || sh.size() != n * 27) throw std::runtime_error("mi_rt: sh must be [n][9][3] and normals [n][3]");
        std::vector<float> out(n * 3);
        if (n == 0) return out;                              // (an empty vector has no address to pass)
        mi_ctx* ctx = nullptr;
        mi_check(mi_ctx_create(device, &ctx));
        const int rc = mi_lightmap_sh_eval(ctx, (uint32_t)n, sh.data(), normals.data(), out.data());
        const std::string err = rc == MI_OK ? "" : mi_last_error();
        mi_ctx_destroy(ctx);
        if (rc != MI_OK) throw std::runtime_error("mi_rt: " + err);
        return out;
    }

    // Read a finished lightmap at uv points through mi_lightmap_sample: image is [H][W][channels], channels 3 or 27, uv [n][2] (intersect's
    // tex_coords as they stand: row 0 is v = 1), `valid` empty (every texel takes part) or finish_lightmap's mask.  Bilinear over the valid
    // texels, or with `nearest` (MI_LS_NEAREST) the texel Texture::sample addresses.  Returns [n][channels]; `weight` takes the weight sum
    // per point (0: nothing to read).  Needs no scene: a static member.
    static std::vector<float> sample_lightmap(const std::vector<float>& image, const std::vector<uint8_t>& valid, uint32_t width, uint32_t height,
                                              uint32_t channels, const std::vector<float>& uv, bool nearest = false, int device = 0,
                                              std::vector<float>* weight = nullptr) {
        const size_t texels = (size_t)width * height, n = uv.size() / 2;
        if (image.size() != texels * channels || (!valid.empty() && valid.size() != texels) || uv.size() != n * 2)
            throw std::runtime_error("mi_rt: image must be [H][W][channels], valid empty or [H][W] and uv [n][2]");
        std::vector<float> out(n * channels);
        if (weight) weight->resize(n);
        if (n == 0) return out;                              // (an empty vector has no address to pass)
        mi_ctx* ctx = nullptr;
        mi_check(mi_ctx_create(device, &ctx));
        const int rc = mi_lightmap_sample(ctx, width, height, channels, image.data(), valid.empty() ? nullptr : valid.data(), (uint32_t)n, uv.data(),
                                          nearest ? MI_LS_NEAREST : 0u, out.data(), weight ? weight->data() : nullptr);
        const std::string err = rc == MI_OK ? "" : mi_last_error();
        mi_ctx_destroy(ctx);
        if (rc != MI_OK) throw std::runtime_error("mi_rt: " + err);
        return out;
    }

    // The irradiance of a finished directional lightmap at uv points and their normals through mi_lightmap_sh_sample: sample_lightmap and
    // eval_lightmap_sh in one pass (sh is [H][W][9][3], normals [n][3]: a hit's shading normal shows its normal map).  An all-zero normal
    // gives +0.0 and weight 0.  Returns [n][3].  Needs no scene: a static member.
    static std::vector<float> sample_lightmap_sh(const std::vector<float>& sh, const std::vector<uint8_t>& valid, uint32_t width, uint32_t height,
                                                 const std::vector<float>& uv, const std::vector<float>& normals, bool nearest = false,
                                                 int device = 0, std::vector<float>* weight = nullptr) {
        const size_t texels = (size_t)width * height, n = uv.size() / 2;
        if (sh.size() != texels * 27 || (!valid.empty() && valid.size() != texels) || uv.size() != n * 2 || normals.size() != n * 3)
            throw std::runtime_error("mi_rt: sh must be [H][W][9][3], valid empty or [H][W], uv [n][2] and normals [n][3]");
        std::vector<float> out(n * 3);
        if (weight) weight->resize(n);
        if (n == 0) return out;                              // (an empty vector has no address to pass)
        mi_ctx* ctx = nullptr;
        mi_check(mi_ctx_create(device, &ctx));
        const int rc = mi_lightmap_sh_sample(ctx, width, height, sh.data(), valid.empty() ? nullptr : valid.data(), (uint32_t)n, uv.data(),
                                             normals.data(), nearest ? MI_LS_NEAREST : 0u, out.data(), weight ? weight->data() : nullptr);
        const std::string err = rc == MI_OK ? "" : mi_last_error();
        mi_ctx_destroy(ctx);
        if (rc != MI_OK) throw std::runtime_error("mi_rt: " + err);
        return out;
    }

    // The mip chain's layout (include/mi_rt.h "lightmap mips"): {width, height, offset in texels} of levels 0 .. levels - 1, ceil halving,
    // levels 1 .. tightly one after the other (level 0 is the image itself: offset 0); `levels` 0 is the full chain.
    struct MipLevel { uint32_t width, height; size_t offset; };
    static std::vector<MipLevel> lightmap_mip_layout(uint32_t width, uint32_t height, uint32_t levels = 0) {
        uint32_t full = 1;
        for (uint32_t n = std::max(width, height); n > 1; n = (n + 1) >> 1) full++;
        if (width == 0 || width > 32768u || height == 0 || height > 32768u || levels > full)
            throw std::runtime_error("mi_rt: width and height must be in 1 .. 32768 and levels at most the full chain");
        std::vector<MipLevel> out;
        size_t off = 0;
        for (uint32_t l = 0; l < (levels ? levels : full); l++) {
            const uint32_t w = (width + (1u << l) - 1) >> l, h = (height + (1u << l) - 1) >> l;
            out.push_back({ w, h, off });
            if (l) off += (size_t)w * h;
        }
        return out;
    }

    // The coverage-aware mip chain of a finished lightmap through mi_lightmap_mips: image [H][W][channels], channels 3 or 27, `valid`
    // empty (every texel takes part) or finish_lightmap's mask, `levels` counting level 0 (0: the full chain).  Returns levels 1 ..
    // tightly packed as lightmap_mip_layout lays them out; `mip_valid` and `coverage` take the masks and the valid fraction of every
    // texel's footprint.  Needs no scene: a static member.
    static std::vector<float> lightmap_mips(const std::vector<float>& image, const std::vector<uint8_t>& valid, uint32_t width, uint32_t height,
                                            uint32_t channels, uint32_t levels = 0, std::vector<uint8_t>* mip_valid = nullptr,
                                            std::vector<float>* coverage = nullptr, int device = 0) {
        const size_t texels = (size_t)width * height;
        if (image.size() != texels * channels || (!valid.empty() && valid.size() != texels))
            throw std::runtime_error("mi_rt: image must be [H][W][channels] and valid empty or [H][W]");
        const size_t made = mip_texels(width, height, levels);
        std::vector<float> mips(std::max<size_t>(made, 1) * channels);
        if (mip_valid) mip_valid->resize(std::max<size_t>(made, 1));
        if (coverage) coverage->resize(std::max<size_t>(made, 1));
        mi_ctx* ctx = nullptr;
        mi_check(mi_ctx_create(device, &ctx));
        const int rc = mi_lightmap_mips(ctx, width, height, channels, image.data(), valid.empty() ? nullptr : valid.data(), levels, mips.data(),
                                        mip_valid ? mip_valid->data() : nullptr, coverage ? coverage->data() : nullptr);
        const std::string err = rc == MI_OK ? "" : mi_last_error();
        mi_ctx_destroy(ctx);
        if (rc != MI_OK) throw std::runtime_error("mi_rt: " + err);
        mips.resize(made * channels);
        if (mip_valid) mip_valid->resize(made);
        if (coverage) coverage->resize(made);
        return mips;
    }

    // Read a lightmap's mip chain at uv points and levels of detail through mi_lightmap_sample_lod: sample_lightmap's arguments with the
    // chain lightmap_mips returned (`mips`, `mip_valid`: empty = every texel valid) and one `lod` per point; trilinear over the valid
    // texels.  Returns [n][channels]; `weight` takes the weight sum per point.  Needs no scene: a static member.
    static std::vector<float> sample_lightmap_lod(const std::vector<float>& image, const std::vector<uint8_t>& valid, uint32_t width,
                                                  uint32_t height, uint32_t channels, uint32_t levels, const std::vector<float>& mips,
                                                  const std::vector<uint8_t>& mip_valid, const std::vector<float>& uv,
                                                  const std::vector<float>& lod, int device = 0, std::vector<float>* weight = nullptr) {
        const size_t texels = (size_t)width * height, n = uv.size() / 2, made = mip_texels(width, height, levels);
        if (image.size() != texels * channels || (!valid.empty() && valid.size() != texels) || uv.size() != n * 2 || lod.size() != n ||
            mips.size() != made * channels || (!mip_valid.empty() && mip_valid.size() != made))
            throw std::runtime_error("mi_rt: image must be [H][W][channels], valid empty or [H][W], mips and mip_valid the layout's, uv [n][2], lod [n]");
        std::vector<float> out(n * channels);
        if (weight) weight->resize(n);
        if (n == 0) return out;                              // (an empty vector has no address to pass)
        mi_ctx* ctx = nullptr;
        mi_check(mi_ctx_create(device, &ctx));
        const int rc = mi_lightmap_sample_lod(ctx, width, height, channels, image.data(), valid.empty() ? nullptr : valid.data(), levels,
                                              mips.empty() ? nullptr : mips.data(), mip_valid.empty() ? nullptr : mip_valid.data(), (uint32_t)n,
                                              uv.data(), lod.data(), 0u, out.data(), weight ? weight->data() : nullptr);
        const std::string err = rc == MI_OK ? "" : mi_last_error();
        mi_ctx_destroy(ctx);
        if (rc != MI_OK) throw std::runtime_error("mi_rt: " + err);
        return out;
    }

    // The irradiance of a directional lightmap's mip chain at uv points, their normals and levels of detail through
    // mi_lightmap_sh_sample_lod: sample_lightmap_sh's arguments with the chain lightmap_mips returned at 27 channels and one `lod` per
    // point.  Returns [n][3].  Needs no scene: a static member.
    static std::vector<float> sample_lightmap_sh_lod(const std::vector<float>& sh, const std::vector<uint8_t>& valid, uint32_t width,
                                                     uint32_t height, uint32_t levels, const std::vector<float>& mips,
                                                     const std::vector<uint8_t>& mip_valid, const std::vector<float>& uv,
                                                     const std::vector<float>& normals, const std::vector<float>& lod, int device = 0,
                                                     std::vector<float>* weight = nullptr) {
        const size_t texels = (size_t)width * height, n = uv.size() / 2, made = mip_texels(width, height, levels);
        if (sh.size() != texels * 27 || (!valid.empty() && valid.size() != texels) || uv.size() != n * 2 || normals.size() != n * 3 ||
            lod.size() != n || mips.size() != made * 27 || (!mip_valid.empty() && mip_valid.size() != made))
            throw std::runtime_error("mi_rt: sh must be [H][W][9][3], valid empty or [H][W], mips and mip_valid the layout's, uv [n][2], normals [n][3], lod [n]");
        std::vector<float> out(n * 3);
        if (weight) weight->resize(n);
        if (n == 0) return out;                              // (an empty vector has no address to pass)
        mi_ctx* ctx = nullptr;
        mi_check(mi_ctx_create(device, &ctx));
        const int rc = mi_lightmap_sh_sample_lod(ctx, width, height, sh.data(), valid.empty() ? nullptr : valid.data(), levels,
                                                 mips.empty() ? nullptr : mips.data(), mip_valid.empty() ? nullptr : mip_valid.data(), (uint32_t)n,
                                                 uv.data(), normals.data(), lod.data(), 0u, out.data(), weight ? weight->data() : nullptr);
        const std::string err = rc == MI_OK ? "" : mi_last_error();
        mi_ctx_destroy(ctx);
        if (rc != MI_OK) throw std::runtime_error("mi_rt: " + err);
        return out;
    }

    // ---- packed lightmaps (include/mi_rt.h "packed lightmaps"): f16 and RGB9E5 storage and the lookups that read it ----
    // pack_lightmap and unpack_lightmap are the formats' definitions on the host, in integer and f32 arithmetic alone: a storage
    // conversion needs no device, and the bytes equal mi_lightmap_pack's and mi_lightmap_unpack's bit for bit (a NaN widens to a NaN).
    // `texels` is [n][channels] f32, channels 3 or 27 (MI_LP_RGB9E5: 3); the result is n * channels u16 for MI_LP_F16, n u32 for
    // MI_LP_RGB9E5, as raw bytes in the layout the C calls take.
    static std::vector<uint8_t> pack_lightmap(const std::vector<float>& texels, uint32_t format, uint32_t channels) {
        check_packed_format(format, channels);
        const size_t n = texels.size() / channels;
        if (texels.size() != n * channels) throw std::runtime_error("mi_rt: texels must be [n][channels]");
        std::vector<uint8_t> out(n * (format == MI_LP_F16 ? 2u * channels : 4u));
        if (format == MI_LP_F16) {
            for (size_t i = 0; i < texels.size(); i++) {
                const uint16_t h = f16_bits(texels[i]);
                std::memcpy(&out[2 * i], &h, 2);
            }
            return out;
        }
        for (size_t i = 0; i < n; i++) {
            float c[3];
            for (int k = 0; k < 3; k++) { const float x = texels[3 * i + k]; c[k] = x != x ? 0.0f : std::fmin(std::fmax(x, 0.0f), 65408.0f); }
            const float m = std::fmax(std::fmax(c[0], c[1]), c[2]);
            const int eb = (int)((f32_bits(m) >> 23) & 255u) - 127;
            const int ep = std::max(eb, -16) + 16;
            const float ms = std::floor(m * pow2(24 - ep) + 0.5f);
            const int e = ep + (ms == 512.0f ? 1 : 0);
            const float s = pow2(24 - e);
            uint32_t w = (uint32_t)e << 27;
            for (int k = 0; k < 3; k++) w |= (uint32_t)std::floor(c[k] * s + 0.5f) << (9 * k);
            std::memcpy(&out[4 * i], &w, 4);
        }
        return out;
    }

    // The exact decode of pack_lightmap's bytes: [n][channels] f32
    static std::vector<float> unpack_lightmap(const std::vector<uint8_t>& packed, uint32_t format, uint32_t channels) {
        check_packed_format(format, channels);
        const size_t bytes = format == MI_LP_F16 ? 2u * channels : 4u, n = packed.size() / bytes;
        if (packed.size() != n * bytes) throw std::runtime_error("mi_rt: packed must hold whole texels");
        std::vector<float> out(n * channels);
        if (format == MI_LP_F16) {
            for (size_t i = 0; i < out.size(); i++) {
                uint16_t h;
                std::memcpy(&h, &packed[2 * i], 2);
                const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, ex = (h >> 10) & 31u, man = h & 1023u;
                if (ex == 31u) out[i] = bits_f32(sign | 0x7F800000u | (man ? 0x00400000u | man << 13 : 0u));        // inf, or a quiet NaN
                else if (ex) out[i] = bits_f32(sign | (ex + 112u) << 23 | man << 13);
                else out[i] = bits_f32(sign | f32_bits((float)man * pow2(-24)));                                   // a subnormal, or zero
            }
            return out;
        }
        for (size_t i = 0; i < n; i++) {
            uint32_t w;
            std::memcpy(&w, &packed[4 * i], 4);
            const float s = pow2((int)(w >> 27) - 24);
            for (int k = 0; k < 3; k++) out[3 * i + k] = (float)((w >> (9 * k)) & 511u) * s;
        }
        return out;
    }

    // Read a packed lightmap at uv points through mi_lightmap_sample_packed: sample_lightmap_lod's arguments with `image` and `mips`
    // as pack_lightmap made them; an empty `lod` reads level 0 alone (then levels must be 1 and mips empty, and `nearest` is allowed).
    // Returns [n][channels]; equals sample_lightmap(_lod) on the unpacked texels bit for bit.  Needs no scene: a static member.
    static std::vector<float> sample_lightmap_packed(uint32_t format, const std::vector<uint8_t>& image, const std::vector<uint8_t>& valid,
                                                     uint32_t width, uint32_t height, uint32_t channels, uint32_t levels,
                                                     const std::vector<uint8_t>& mips, const std::vector<uint8_t>& mip_valid,
                                                     const std::vector<float>& uv, const std::vector<float>& lod, bool nearest = false,
                                                     int device = 0, std::vector<float>* weight = nullptr) {
        return packed_lookup(format, image, valid, width, height, channels, levels, mips, mip_valid, uv, nullptr, lod, nearest, device, weight);
    }

    // The irradiance of a directional lightmap packed as MI_LP_F16 through mi_lightmap_sh_sample_packed: sample_lightmap_sh_lod's
    // arguments with packed records; an empty `lod` reads level 0 alone.  Returns [n][3].  Needs no scene: a static member.
    static std::vector<float> sample_lightmap_sh_packed(uint32_t format, const std::vector<uint8_t>& sh, const std::vector<uint8_t>& valid,
                                                        uint32_t width, uint32_t height, uint32_t levels, const std::vector<uint8_t>& mips,
                                                        const std::vector<uint8_t>& mip_valid, const std::vector<float>& uv,
                                                        const std::vector<float>& normals, const std::vector<float>& lod,
                                                        bool nearest = false, int device = 0, std::vector<float>* weight = nullptr) {
        if (normals.size() != uv.size() / 2 * 3) throw std::runtime_error("mi_rt: normals must be [n][3]");
        return packed_lookup(format, sh, valid, width, height, 0, levels, mips, mip_valid, uv, &normals, lod, nearest, device, weight);
    }

    // ---- BC6H lightmaps (include/mi_rt.h "BC6H lightmaps"): the block encoder, the decoder and the lookup that reads blocks ----
    // encode_lightmap_bc6h and decode_lightmap_bc6h are the format's definitions on the host, one level per call, in integer arithmetic
    // alone after the binary16 conversion: the bytes equal mi_lightmap_bc6h_encode's and mi_lightmap_bc6h_decode's.  `image` is
    // [height][width][3] f32, `valid` empty (every texel takes part) or [height][width], `rounds` 0 .. 4; the result is
    // ceil(height / 4) x ceil(width / 4) blocks of 16 bytes, row-major.
    struct Bc6hLevel { uint32_t bw, bh; size_t offset; };
    // The one rule for block counts and offsets (in blocks; level 0 is a buffer of its own: offset 0)
    static std::vector<Bc6hLevel> lightmap_bc6h_layout(uint32_t width, uint32_t height, uint32_t levels = 0) {
        std::vector<Bc6hLevel> out;
        size_t off = 0;
        for (const MipLevel& m : lightmap_mip_layout(width, height, levels)) {
            const uint32_t bw = (m.width + 3) >> 2, bh = (m.height + 3) >> 2;
            out.push_back({ bw, bh, off });
            if (out.size() > 1) off += (size_t)bw * bh;
        }
        return out;
    }

    static std::vector<uint8_t> encode_lightmap_bc6h(const std::vector<float>& image, const std::vector<uint8_t>& valid, uint32_t width,
                                                     uint32_t height, uint32_t rounds = 2) {
        const size_t texels = (size_t)width * height;
        if (width == 0 || width > 32768u || height == 0 || height > 32768u || image.size() != texels * 3 || (!valid.empty() && valid.size() != texels))
            throw std::runtime_error("mi_rt: image must be [height][width][3] with 1 .. 32768 texels a side, valid empty or [height][width]");
        if (rounds > 4) throw std::runtime_error("mi_rt: rounds must be in 0 .. 4");
        const uint32_t bw = (width + 3) >> 2, bh = (height + 3) >> 2;
        std::vector<uint8_t> out((size_t)bw * bh * 16);
        for (uint32_t by = 0; by < bh; by++)
            for (uint32_t bx = 0; bx < bw; bx++) {
                int64_t h[16][3] = {};
                bool part[16] = {};
                for (uint32_t t = 0; t < 16; t++) {
                    const uint32_t x = 4 * bx + (t & 3), y = 4 * by + (t >> 2);
                    if (x >= width || y >= height) continue;
                    const size_t q = (size_t)y * width + x;
                    if (!valid.empty() && valid[q] == 0) continue;                       // takes no part: not read
                    part[t] = true;
                    for (int k = 0; k < 3; k++) { const float v = image[3 * q + k]; h[t][k] = f16_bits(v > 0.0f ? std::fmin(v, 65504.0f) : 0.0f); }
                }
                bc6h_encode_block(h, part, rounds, &out[((size_t)by * bw + bx) * 16]);
            }
        return out;
    }

    // The exact decode of a level's blocks: [height][width][3] f32; a block whose low five bits are not 3 gives zeros
    static std::vector<float> decode_lightmap_bc6h(const std::vector<uint8_t>& blocks, uint32_t width, uint32_t height) {
        const uint32_t bw = (width + 3) >> 2, bh = (height + 3) >> 2;
        if (width == 0 || width > 32768u || height == 0 || height > 32768u || blocks.size() != (size_t)bw * bh * 16)
            throw std::runtime_error("mi_rt: blocks must be ceil(height / 4) x ceil(width / 4) x 16 bytes");
        std::vector<float> out((size_t)width * height * 3);
        for (uint32_t y = 0; y < height; y++)
            for (uint32_t x = 0; x < width; x++) {
                const uint8_t* b = &blocks[((size_t)(y >> 2) * bw + (x >> 2)) * 16];
                uint64_t lo = 0, hi = 0;
                for (int i = 0; i < 8; i++) { lo |= (uint64_t)b[i] << (8 * i); hi |= (uint64_t)b[8 + i] << (8 * i); }
                const uint32_t t = (y & 3) * 4 + (x & 3);
                const uint32_t i = t == 0 ? (uint32_t)(hi >> 1) & 7u : (uint32_t)(hi >> (4 * t)) & 15u;
                for (int k = 0; k < 3; k++) {
                    const int64_t a = bc6h_unq(bc6h_field(lo, hi, 5 + 10 * k)), e = bc6h_unq(bc6h_field(lo, hi, 35 + 10 * k));
                    const uint32_t hb = (lo & 31u) == 3u ? (uint32_t)bc6h_interp(a, e, bc6h_weight(i)) : 0u;
                    out[3 * ((size_t)y * width + x) + k] = bits_f32(hb >> 10 ? ((hb >> 10) + 112u) << 23 | (hb & 1023u) << 13
                                                                             : f32_bits((float)hb * pow2(-24)));     // hb <= 0x7BFF: no sign, no infinity
                }
            }
        return out;
    }

    // Read a BC6H lightmap at uv points through mi_lightmap_sample_bc6h: sample_lightmap_packed's arguments, three channels, the levels
    // as encode_lightmap_bc6h made them (level 0 in `image`, levels 1 .. one after the other in `mips`); an empty `lod` reads level 0
    // alone.  Returns [n][3]; equals sample_lightmap(_lod) on the decoded texels bit for bit.  Needs no scene: a static member.
    static std::vector<float> sample_lightmap_bc6h(const std::vector<uint8_t>& image, const std::vector<uint8_t>& valid, uint32_t width,
                                                   uint32_t height, uint32_t levels, const std::vector<uint8_t>& mips,
                                                   const std::vector<uint8_t>& mip_valid, const std::vector<float>& uv,
                                                   const std::vector<float>& lod, bool nearest = false, int device = 0,
                                                   std::vector<float>* weight = nullptr) {
        const std::vector<Bc6hLevel> layout = lightmap_bc6h_layout(width, height, levels);
        const size_t texels = (size_t)width * height, n = uv.size() / 2, made = mip_texels(width, height, levels);
        const size_t made_blocks = layout.back().offset + (layout.size() > 1 ? (size_t)layout.back().bw * layout.back().bh : 0);
        if (image.size() != (size_t)layout[0].bw * layout[0].bh * 16 || (!valid.empty() && valid.size() != texels) || uv.size() != n * 2 ||
            (!lod.empty() && lod.size() != n) || mips.size() != made_blocks * 16 || (!mip_valid.empty() && mip_valid.size() != made))
            throw std::runtime_error("mi_rt: image and mips must hold the layout's blocks, valid empty or [H][W], mip_valid the layout's, uv [n][2], lod empty or [n]");
        std::vector<float> out(n * 3);
        if (weight) weight->resize(n);
        if (n == 0) return out;
        mi_ctx* ctx = nullptr;
        mi_check(mi_ctx_create(device, &ctx));
        const int rc = mi_lightmap_sample_bc6h(ctx, width, height, image.data(), valid.empty() ? nullptr : valid.data(), levels,
                                               mips.empty() ? nullptr : mips.data(), mip_valid.empty() ? nullptr : mip_valid.data(), (uint32_t)n,
                                               uv.data(), lod.empty() ? nullptr : lod.data(), nearest ? MI_LS_NEAREST : 0u, out.data(),
                                               weight ? weight->data() : nullptr);
        const std::string err = rc == MI_OK ? "" : mi_last_error();
        mi_ctx_destroy(ctx);
        if (rc != MI_OK) throw std::runtime_error("mi_rt: " + err);
        return out;
    }

private:
    static uint32_t f32_bits(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }
    static float bits_f32(uint32_t u) { float x; std::memcpy(&x, &u, 4); return x; }
    static float pow2(int e) { return bits_f32((uint32_t)(e + 127) << 23); }                 // exact, -126 <= e <= 127

    static void check_packed_format(uint32_t format, uint32_t channels) {
        if (format != MI_LP_F16 && format != MI_LP_RGB9E5) throw std::runtime_error("mi_rt: format must be MI_LP_F16 or MI_LP_RGB9E5");
        if (channels != 3 && channels != 27) throw std::runtime_error("mi_rt: channels must be 3 or 27");
        if (format == MI_LP_RGB9E5 && channels != 3) throw std::runtime_error("mi_rt: MI_LP_RGB9E5 holds 3 unsigned channels");
    }

    // f32 -> binary16 bits as the header defines them: a NaN is 0x7E00, everything else is clamped to +-65504 and rounded to nearest even
    static uint16_t f16_bits(float x) {
        if (x != x) return 0x7E00u;
        const float c = std::fmin(std::fmax(x, -65504.0f), 65504.0f);
        const uint32_t u = f32_bits(c), sign = (u >> 16) & 0x8000u, mag = u & 0x7FFFFFFFu;
        if (mag >= 0x38800000u) {                              // a normal f16: drop 13 bits of the significand, to nearest even
            const uint32_t r = mag + 0x0FFFu + ((mag >> 13) & 1u);
            return (uint16_t)(sign | ((r >> 13) - (112u << 10)));
        }
        if (mag < 0x33000000u) return (uint16_t)sign;          // below 2^-25: zero (2^-25 itself is a tie, to the even zero, below)
        const uint32_t man = (mag & 0x007FFFFFu) | 0x00800000u, shift = 126u - (mag >> 23);     // 14 .. 24: the value is man * 2^-(shift + 10) steps of 2^-24
        const uint32_t q = man >> shift, rest = man & ((1u << shift) - 1u), half = 1u << (shift - 1);
        return (uint16_t)(sign | (q + ((rest > half || (rest == half && (q & 1u))) ? 1u : 0u)));
    }

    static std::vector<float> packed_lookup(uint32_t format, const std::vector<uint8_t>& image, const std::vector<uint8_t>& valid, uint32_t width,
                                            uint32_t height, uint32_t channels, uint32_t levels, const std::vector<uint8_t>& mips,
                                            const std::vector<uint8_t>& mip_valid, const std::vector<float>& uv,
                                            const std::vector<float>* normals, const std::vector<float>& lod, bool nearest, int device,
                                            std::vector<float>* weight) {
        const uint32_t in_c = channels ? channels : 27u, out_c = channels ? channels : 3u;
        check_packed_format(format, in_c);
        const size_t texels = (size_t)width * height, n = uv.size() / 2, made = mip_texels(width, height, levels);
        const size_t bytes = format == MI_LP_F16 ? 2u * in_c : 4u;
        if (image.size() != texels * bytes || (!valid.empty() && valid.size() != texels) || uv.size() != n * 2 || (!lod.empty() && lod.size() != n) ||
            mips.size() != made * bytes || (!mip_valid.empty() && mip_valid.size() != made))
            throw std::runtime_error("mi_rt: image must be [H][W] packed texels, valid empty or [H][W], mips and mip_valid the layout's, uv [n][2], lod empty or [n]");
        std::vector<float> out(n * out_c);
        if (weight) weight->resize(n);
        if (n == 0) return out;                              // (an empty vector has no address to pass)
        mi_ctx* ctx = nullptr;
        mi_check(mi_ctx_create(device, &ctx));
        const uint8_t* v = valid.empty() ? nullptr : valid.data();
        const uint8_t* m = mips.empty() ? nullptr : mips.data();
        const uint8_t* mv = mip_valid.empty() ? nullptr : mip_valid.data();
        const float* d = lod.empty() ? nullptr : lod.data();
        float* ow = weight ? weight->data() : nullptr;
        const uint32_t flags = nearest ? MI_LS_NEAREST : 0u;
        const int rc = normals ? mi_lightmap_sh_sample_packed(ctx, format, width, height, image.data(), v, levels, m, mv, (uint32_t)n, uv.data(),
                                                              normals->data(), d, flags, out.data(), ow)
                               : mi_lightmap_sample_packed(ctx, format, width, height, channels, image.data(), v, levels, m, mv, (uint32_t)n,
                                                           uv.data(), d, flags, out.data(), ow);
        const std::string err = rc == MI_OK ? "" : mi_last_error();
        mi_ctx_destroy(ctx);
        if (rc != MI_OK) throw std::runtime_error("mi_rt: " + err);
        return out;
    }

    // BC6H, the one mode: the integer pieces of the decoder and the encoder (include/mi_rt.h "BC6H lightmaps")
    static int64_t bc6h_weight(uint32_t i) { static const int W[16] = { 0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64 }; return W[i]; }
    static int64_t bc6h_unq(int64_t q) { return q == 0 ? 0 : q == 1023 ? 0xFFFF : ((q << 16) + 0x8000) >> 10; }
    static int64_t bc6h_interp(int64_t a, int64_t b, int64_t w) { return (((a * (64 - w) + b * w + 32) >> 6) * 31) >> 6; }
    static int64_t bc6h_field(uint64_t lo, uint64_t hi, int bit) { return (int64_t)(((lo >> bit) | (hi << (64 - bit))) & 1023u); }
    static int64_t bc6h_to_c(int64_t h) { return (64 * h + 30) / 31; }
    // the field whose unquantised value is nearest to c (clamped to 0 .. 65535), the lower field on a tie
    static int64_t bc6h_quant(int64_t c) {
        c = std::min<int64_t>(std::max<int64_t>(c, 0), 65535);
        const int64_t q0 = std::min<int64_t>(std::max<int64_t>((c - 1) >> 6, 0), 1023);
        int64_t best = std::max<int64_t>(q0 - 1, 0), bd = std::llabs(bc6h_unq(best) - c);
        for (int64_t step = 0; step < 2; step++) {
            const int64_t q = std::min<int64_t>(q0 + step, 1023), d = std::llabs(bc6h_unq(q) - c);
            if (d < bd) { best = q; bd = d; }
        }
        return best;
    }
    static int64_t bc6h_floor_div(int64_t a, int64_t b) { return a / b - ((a % b != 0 && (a < 0) != (b < 0)) ? 1 : 0); }
    // every texel's index for the fields f: the least squared distance to its target, the lowest index on a tie; returns the error summed
    // over the texels that take part
    static int64_t bc6h_assign(const int64_t (&target)[16][3], const bool (&part)[16], const int64_t (&f)[2][3], int (&idx)[16]) {
        int64_t err = 0;
        for (int t = 0; t < 16; t++) {
            int64_t be = -1;
            for (uint32_t i = 0; i < 16; i++) {
                int64_t e = 0;
                for (int k = 0; k < 3; k++) { const int64_t d = target[t][k] - bc6h_interp(bc6h_unq(f[0][k]), bc6h_unq(f[1][k]), bc6h_weight(i)); e += d * d; }
                if (be < 0 || e < be) { be = e; idx[t] = (int)i; }
            }
            if (part[t]) err += be;
        }
        return err;
    }
    static void bc6h_encode_block(const int64_t (&h)[16][3], const bool (&part)[16], uint32_t rounds, uint8_t* out) {
        std::memset(out, 0, 16);
        out[0] = 3;
        int64_t n = 0, sum[3] = { 0, 0, 0 };
        for (int t = 0; t < 16; t++) if (part[t]) { n++; for (int k = 0; k < 3; k++) sum[k] += h[t][k]; }
        if (n == 0) return;
        int fi = -1, fj = -1;
        int64_t far = -1;
        for (int i = 0; i < 16; i++)
            for (int j = i; j < 16; j++) {
                if (!part[i] || !part[j]) continue;
                int64_t d = 0;
                for (int k = 0; k < 3; k++) d += (h[i][k] - h[j][k]) * (h[i][k] - h[j][k]);
                if (d > far) { far = d; fi = i; fj = j; }
            }
        int64_t f[2][3], target[16][3], ct[16][3];
        for (int k = 0; k < 3; k++) { f[0][k] = bc6h_quant(bc6h_to_c(h[fi][k])); f[1][k] = bc6h_quant(bc6h_to_c(h[fj][k])); }
        if (f[0][0] == f[1][0] && f[0][1] == f[1][1] && f[0][2] == f[1][2])             // a flat start: the two fields around c where the one is far
            for (int k = 0; k < 3; k++) {
                const int64_t c = bc6h_to_c(h[fi][k]);
                if (std::llabs(bc6h_unq(f[0][k]) - c) > 32) { f[0][k] = c < 96 ? 0 : 1022; f[1][k] = f[0][k] + 1; }
            }
        for (int t = 0; t < 16; t++)
            for (int k = 0; k < 3; k++) { target[t][k] = part[t] ? h[t][k] : sum[k] / n; ct[t][k] = bc6h_to_c(h[t][k]); }
        int idx[16];
        int64_t err = bc6h_assign(target, part, f, idx);
        for (uint32_t r = 0; r < rounds; r++) {
            int64_t suu = 0, suv = 0, svv = 0, suc[3] = { 0, 0, 0 }, svc[3] = { 0, 0, 0 };
            for (int t = 0; t < 16; t++) {
                if (!part[t]) continue;
                const int64_t v = bc6h_weight((uint32_t)idx[t]), u = 64 - v;
                suu += u * u; suv += u * v; svv += v * v;
                for (int k = 0; k < 3; k++) { suc[k] += u * ct[t][k]; svc[k] += v * ct[t][k]; }
            }
            const int64_t det = suu * svv - suv * suv;
            int64_t cf[2][3];
            for (int k = 0; k < 3; k++) {
                cf[0][k] = f[0][k]; cf[1][k] = f[1][k];
                if (det == 0) continue;
                cf[0][k] = bc6h_quant(bc6h_floor_div(2 * (64 * (svv * suc[k] - suv * svc[k])) + det, 2 * det));
                cf[1][k] = bc6h_quant(bc6h_floor_div(2 * (64 * (suu * svc[k] - suv * suc[k])) + det, 2 * det));
            }
            int cidx[16];
            const int64_t cerr = bc6h_assign(target, part, cf, cidx);
            if (cerr < err) {                                                            // kept only if strictly lower
                err = cerr;
                std::memcpy(f, cf, sizeof f);
                std::memcpy(idx, cidx, sizeof idx);
            }
        }
        if (idx[0] >= 8) {
            for (int k = 0; k < 3; k++) std::swap(f[0][k], f[1][k]);
            for (int t = 0; t < 16; t++) idx[t] = 15 - idx[t];
        }
        uint64_t lo = 3, hi = (uint64_t)f[1][2] >> 9 | (uint64_t)idx[0] << 1;
        for (int k = 0; k < 6; k++) lo |= (uint64_t)f[k / 3][k % 3] << (5 + 10 * k);       // (the last field's top bit falls off: it is hi's bit 0)
        for (int t = 1; t < 16; t++) hi |= (uint64_t)idx[t] << (4 * t);
        for (int i = 0; i < 8; i++) { out[i] = (uint8_t)(lo >> (8 * i)); out[8 + i] = (uint8_t)(hi >> (8 * i)); }
    }

    // the texels of levels 1 .. of a chain
    static size_t mip_texels(uint32_t width, uint32_t height, uint32_t levels) {
        const std::vector<MipLevel> layout = lightmap_mip_layout(width, height, levels);
        return layout.size() < 2 ? 0 : layout.back().offset + (size_t)layout.back().width * layout.back().height;
    }

    // flatten -> context -> upload -> `call(ctx)` -> destroy; a failure surfaces as std::runtime_error carrying mi_last_error()
    template <class F> void with_context(int device, F call) const {
        SceneBuilder sb;
        for (auto& o : objects) o->flatten(sb);
        mi_scene_desc d = sb.desc();
        for (int k = 0; k < 3; k++) { d.point_light_pos[k] = point_light_pos[k]; d.ambient[k] = ambient[k]; }
        mi_ctx* ctx = nullptr;
        mi_check(mi_ctx_create(device, &ctx));
        int rc = mi_scene_upload(ctx, &d);
        if (rc == MI_OK) rc = call(ctx);
        const std::string err = rc == MI_OK ? "" : mi_last_error();
        mi_ctx_destroy(ctx);
        if (rc != MI_OK) throw std::runtime_error("mi_rt: " + err);
    }
};

}  // namespace cs397
