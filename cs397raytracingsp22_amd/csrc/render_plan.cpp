// render_plan.cpp — the host-side decisions of a render (render_plan.hpp).  Compiled with -ffp-contract=off: make_camera's
// values are the reference's f32 operations in its order, and the tile masks' f64 geometry must not change with the compiler.
#include "render_plan.hpp"

#include <algorithm>
#include <cstring>

#pragma clang fp contract(off)

namespace pt {

int check_camera(const mi_camera_desc* cam) {
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

int check_table_camera(const mi_camera_desc* cam, uint32_t rays_per_pixel) {
    if (!cam) return fail(MI_ERR_INVALID, "camera is NULL");
    if (cam->shading_mode != MI_SHADE_PATHTRACE && cam->shading_mode != MI_SHADE_PHONG)
        return fail(MI_ERR_INVALID, "unknown shading_mode %d", cam->shading_mode);
    if (cam->path_samples == 0) return fail(MI_ERR_INVALID, "path_samples must be >= 1 (tracing.rs:318 divides by it)");
    if (cam->screen_width == 0 || cam->screen_height == 0 || cam->screen_width > 32768 || cam->screen_height > 32768)
        return fail(MI_ERR_INVALID, "bad image size %ux%u", cam->screen_width, cam->screen_height);
    if (cam->aa_sample_count == 0) return fail(MI_ERR_INVALID, "aa_sample_count must be >= 1");
    if (!(cam->gamma > 0.0f) || !std::isfinite(cam->gamma)) return fail(MI_ERR_INVALID, "gamma must be finite and > 0 (tracing.rs:254 raises to 1/gamma)");
    if (std::isnan(cam->max_trace_dist)) return fail(MI_ERR_INVALID, "max_trace_dist must not be NaN");
    if (rays_per_pixel != 1u && rays_per_pixel != cam->aa_sample_count)
        return fail(MI_ERR_INVALID, "rays_per_pixel is %u: a ray table holds 1 row or aa_sample_count = %u rows", rays_per_pixel, cam->aa_sample_count);
    if (cam->shading_mode == MI_SHADE_PHONG)
        return fail(MI_ERR_UNSUPPORTED, "ray-table rendering: ShadingMode::Phong is not available for caller-supplied rays (mi_shade_rays has no Phong either)");
    if (cam->path_samples != 1)
        return fail(MI_ERR_UNSUPPORTED, "ray-table rendering runs the wavefront pipeline, path_samples == 1 only: use mi_shade_rays for path_samples = %u", cam->path_samples);
    return MI_OK;
}

mi_camera_desc table_camera(const mi_camera_desc* cam) {
    mi_camera_desc t = *cam;
    const float eye[3] = { 0.0f, 0.0f, 0.0f }, view[3] = { 0.0f, 0.0f, -1.0f }, up[3] = { 0.0f, 1.0f, 0.0f };
    for (int k = 0; k < 3; k++) { t.eyepoint[k] = eye[k]; t.view_dir[k] = view[k]; t.up[k] = up[k]; }
    t.projection_mode = MI_PROJ_PERSPECTIVE;
    t.focal_length = 1.0f; t.focus_dist = 1.0f; t.lens_radius = 0.0f;
    return t;
}

// The tile grid of the partition.  Tiles are numbered row-major over a grid whose ROW LENGTH `tx` is the image's tile columns
// rounded up to the next integer coprime with `world` (tile t -> rank t % world, slot t / world): a row length that shares a factor
// with the rank count repeats the same few column classes for a rank in every row (60 columns over 8 ranks: two classes, and the
// ranks whose classes cross the expensive middle of the frame took 7 % longer than the others); a coprime one walks every rank
// through all classes.  The extra columns hold no pixel: their tiles are rendered as "outside the image" (zeros) and never
// copied anywhere.  world = 1 (mi_render) keeps the plain grid.
TileGrid tile_grid(const mi_camera_desc* cam, int world) {
    uint32_t stride = (cam->screen_width + MI_TILE - 1) / MI_TILE;
    auto gcd = [](uint32_t a, uint32_t b) { while (b) { const uint32_t r = a % b; a = b; b = r; } return a; };
    while (gcd(stride, (uint32_t)world) != 1u) stride++;
    TileGrid g;
    g.tx = stride;
    g.ty = (cam->screen_height + MI_TILE - 1) / MI_TILE;
    g.total = g.tx * g.ty;
    g.padded = (g.total + (uint32_t)world - 1) / (uint32_t)world;
    return g;
}

uint32_t rank_tiles(const TileGrid& g, int rank, int world) {
    return (g.total > (uint32_t)rank) ? (g.total - (uint32_t)rank + (uint32_t)world - 1) / (uint32_t)world : 0;
}

namespace {
// fn(t, w, h) for every tile t of `rank` (t = rank, rank + world, ...) that holds pixels, w x h = its rectangle inside the image
// (the columns of the numbering beyond the image are skipped)
template <class F> void for_each_rank_tile(const TileGrid& g, const mi_camera_desc* cam, int rank, int world, F fn) {
    for (uint32_t t = (uint32_t)rank; t < g.total; t += (uint32_t)world) {
        const uint32_t x0 = (t % g.tx) * MI_TILE, y0 = (t / g.tx) * MI_TILE;
        if (x0 >= cam->screen_width || y0 >= cam->screen_height) continue;
        fn(t, std::min<uint32_t>(MI_TILE, cam->screen_width - x0), std::min<uint32_t>(MI_TILE, cam->screen_height - y0));
    }
}
}  // namespace

uint64_t rank_pixels(const TileGrid& g, const mi_camera_desc* cam, int rank, int world) {
    uint64_t pixels = 0;
    for_each_rank_tile(g, cam, rank, world, [&](uint32_t, uint32_t w, uint32_t h) { pixels += (uint64_t)w * h; });
    return pixels;
}

uint64_t dead_pixels(const TileGrid& g, const mi_camera_desc* cam, int rank, int world, const std::vector<uint64_t>& masks) {
    uint64_t pixels = 0;
    for_each_rank_tile(g, cam, rank, world, [&](uint32_t t, uint32_t w, uint32_t h) {
        if (masks[(size_t)g.total + t] >> 63) pixels += (uint64_t)w * h;
    });
    return pixels;
}

DCamera make_camera(const mi_camera_desc* cam) {
    DCamera C;
    memset(&C, 0, sizeof C);
    h3 view = H3p(cam->view_dir), up = H3p(cam->up);
    h3 c0 = normalize(cross(view, up));                                 // tracing.rs:188
    C.eye[0] = cam->eyepoint[0]; C.eye[1] = cam->eyepoint[1]; C.eye[2] = cam->eyepoint[2];
    C.rot[0] = c0.x; C.rot[1] = c0.y; C.rot[2] = c0.z;
    C.rot[3] = up.x; C.rot[4] = up.y; C.rot[5] = up.z;                  // :189
    C.rot[6] = -view.x; C.rot[7] = -view.y; C.rot[8] = -view.z;         // :190
    C.pixel_size = 1.0f / (float)cam->screen_height;                    // :160
    C.n = (float)cam->aa_sample_count;                                  // :162
    C.rootn = sqrtf(C.n);                                               // :163
    C.half_rootn = 0.5f * C.rootn;
    C.half_n = 0.5f * C.n;
    C.cx_base = -(0.5f * (float)cam->screen_width);                     // :178
    C.cy_base = 0.5f + 0.5f * (float)cam->screen_height;                // :179
    C.focal_length = cam->focal_length; C.focus_dist = cam->focus_dist; C.lens_radius = cam->lens_radius;
    C.max_trace_dist = cam->max_trace_dist;
    C.rootn_u = (uint32_t)C.rootn;                                      // :169 `rootn as u32`
    C.spp = cam->aa_sample_count;
    C.zone = (C.spp << __builtin_clz(C.spp)) - 1u;                      // rand 0.8.4 UniformInt::sample_single
    C.path_depth = cam->path_depth;
    C.width = cam->screen_width; C.height = cam->screen_height;
    C.ortho = cam->projection_mode == MI_PROJ_ORTHOGRAPHIC ? 1u : 0u;
    // :200,204  rotation * view_dir with cgmath's Matrix3 * Vector3 order: (c0*v.x + c1*v.y) + c2*v.z
    h3 c2 = H3(-view.x, -view.y, -view.z);
    h3 od = add(add(scale(c0, view.x), scale(up, view.y)), scale(c2, view.z));
    C.ortho_dir[0] = od.x; C.ortho_dir[1] = od.y; C.ortho_dir[2] = od.z;
    return C;
}

uint32_t two_stage_mask(const CompiledScene& sc, uint32_t flags) {
    if (flags & MI_OPT_REFERENCE_WALK) return 0u;
    uint32_t m = 0;
    for (size_t i = 0; i < sc.meshes.size() && i < (size_t)kTwoStageMaxMeshes; i++)
        if (sc.meshes[i].qualifies && ((flags & MI_OPT_TWO_STAGE) || sc.meshes[i].default_ts)) m |= 1u << i;
    return m;
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
bool tile_masks(const CompiledScene& sc, const mi_camera_desc& cam, uint32_t flags, uint32_t stride, std::vector<uint64_t>& out) {
    const int n_ts = sc.n_list_tri + sc.n_list_sphere;
    const int n_mesh = (int)sc.meshes.size();
    if ((n_ts == 0 && n_mesh == 0) || n_ts > 64 || n_mesh > 32) return false;
    // rays must leave the eye itself (no lens) towards the image plane (focus_dist > 0 keeps the direction's sign)
    if (cam.projection_mode != MI_PROJ_PERSPECTIVE || cam.lens_radius != 0.0f || !(cam.focus_dist > 0.0f) || (flags & MI_OPT_NO_TILE_MASKS)) return false;
    const double W = cam.screen_width, H = cam.screen_height, p = 1.0 / H;
    const double view[3] = { cam.view_dir[0], cam.view_dir[1], cam.view_dir[2] };
    const double up[3] = { cam.up[0], cam.up[1], cam.up[2] };
    double c0[3] = { view[1] * up[2] - view[2] * up[1], view[2] * up[0] - view[0] * up[2], view[0] * up[1] - view[1] * up[0] };
    const double l0 = sqrt(c0[0] * c0[0] + c0[1] * c0[1] + c0[2] * c0[2]);
    if (!(l0 > 1e-12) || !std::isfinite(l0)) return false;
    for (double& v : c0) v /= l0;
    // det of R = [c0 up -view]: a (near-)singular basis flattens the pyramid
    const double det = c0[0] * (up[1] * -view[2] - up[2] * -view[1]) - up[0] * (c0[1] * -view[2] - c0[2] * -view[1])
                     + -view[0] * (c0[1] * up[2] - c0[2] * up[1]);
    if (!(fabs(det) > 1e-6) || !std::isfinite(det)) return false;
    auto dir = [&](double px, double py, double* o) {           // R * (camera-space point on the image plane)
        const double x = p * (px - 0.5 * W + 0.5), y = p * (0.5 + 0.5 * H - py), z = -(double)cam.focal_length;
        for (int k = 0; k < 3; k++) o[k] = c0[k] * x + up[k] * y + -view[k] * z;
    };
    // `stride` >= the image's tile columns: the row length of the tile numbering (tile_grid); the surplus columns hold no pixel
    const uint32_t tx = stride, tx_image = (cam.screen_width + MI_TILE - 1) / MI_TILE, ty = (cam.screen_height + MI_TILE - 1) / MI_TILE;
    // [0, tiles): list masks; [tiles, 2*tiles): low 32 bits = mesh mask, bit 63 = DEAD tile (nothing reachable:
    // every camera ray of the tile leaves the scene at once)
    const size_t n_tiles = (size_t)tx * ty;
    out.assign(2 * n_tiles, ~0ull);
    for (size_t t = 0; t < n_tiles; t++) out[n_tiles + t] = 0xffffffffull;
    const double margin_px = 2.0, slack = 1e-4;
    const double eye[3] = { cam.eyepoint[0], cam.eyepoint[1], cam.eyepoint[2] };
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
        const double t_reach = (double)cam.max_trace_dist * colmax;
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
            out[(size_t)j * tx + i] = 0ull; out[n_tiles + (size_t)j * tx + i] = 1ull << 63;
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
        out[(size_t)j * tx + i] = mask;
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
        out[n_tiles + (size_t)j * tx + i] = mm;
    }
    return true;
}

// The batch is sized to the free HBM (288 GB on MI355X: the whole 1080p/256 spp frame, 531 M paths = 112 GB, is ONE batch);
// mi_rt.cpp halves it when an allocation fails.
int wf_first_batch(uint32_t npix, uint32_t spp, uint64_t max_state_bytes, uint64_t free_bytes, bool two_stage, uint32_t* s_batch) {
    const size_t per_path = kWfBytesPerPath + (two_stage ? kWfBytesPerPathTwoStage : 0);
    uint64_t max_paths;
    if (max_state_bytes != 0) max_paths = max_state_bytes / per_path;        // the caller's budget (mi_render_opts)
    else max_paths = (uint64_t)((double)free_bytes * 0.6 / (double)per_path);
    if (max_paths > (1ull << 31)) max_paths = 1ull << 31;           // 32-bit path indices
    uint64_t sb = max_paths / npix;
    // the smallest batch is one sample of every (padded) pixel of this rank: a caller's budget below that cannot be honoured
    if (sb < 1 && max_state_bytes != 0)
        return fail(MI_ERR_INVALID, "max_state_bytes = %llu is below the pipeline's minimum for this image: one sample per pixel = %llu bytes",
                    (unsigned long long)max_state_bytes, (unsigned long long)((uint64_t)npix * per_path));
    if (sb < 1) sb = 1;
    if (sb > spp) sb = spp;
    *s_batch = (uint32_t)sb;
    return MI_OK;
}

WfBatch wf_batch(uint32_t npix, uint32_t s_batch) {
    WfBatch b;
    const uint32_t paths = npix * s_batch;
    const uint32_t max_blocks = (paths + kBlock - 1) / kBlock;
    // a shard receives at most the paths of its own input blocks: ceil(n_blocks / shards) blocks, where
    // n_blocks <= max_blocks + 2 * shards (one partial block per (class, shard) range)
    b.region = ((max_blocks + kWfShards - 1) / kWfShards + 3) * kBlock;
    b.cap = b.region * (uint32_t)kWfShards;
    b.state_bytes = (size_t)kWfPlanes * sizeof(float4) * b.cap;      // each of ping and pong
    b.samp_bytes = (size_t)paths * sizeof(float4);
    b.acc_bytes = (size_t)npix * sizeof(float4);
    b.cand_bytes = (size_t)b.cap * kCandMax * sizeof(uint2);         // two-stage only
    b.cand_hdr_bytes = (size_t)b.cap * sizeof(uint2);
    return b;
}

// ---- the pass schedule (K1w).  mi_rt.cpp's pass loop asks pass_gate, waits if told to, asks plan_pass and launches what it names.
PassHdr camera_pass_header(uint32_t n_in) { return PassHdr{ (n_in + kBlock - 1) / kBlock, n_in, 0u, 0u, 0u, 0u }; }

WalkMasks walk_masks(const CompiledScene& sc, uint32_t flags) {
    const uint32_t all_meshes = sc.S.n_meshes >= 32 ? 0xffffffffu : ((1u << sc.S.n_meshes) - 1u);
    const uint32_t ts = two_stage_mask(sc, flags) & all_meshes;
    return WalkMasks{ all_meshes & ~ts, ts };
}

PassSchedule pass_schedule(const CompiledScene& sc, WalkMasks masks, const WalkerPlan& walker, int n_cus, uint32_t path_depth, const ScheduleKnobs& knobs) {
    PassSchedule s;
    s.ref_mask = masks.ref; s.ts_mask = masks.ts; s.nowait_blocks = knobs.nowait_blocks;
    s.have_walkers = masks.ref || masks.ts || sc.S.n_meshes > 32;
    s.ref_walk = masks.ref || sc.S.n_meshes > 32;      // meshes 32, 33, ... have no mask bit: they always take the reference walk
    // Meshes of both kinds: wf_trav and wf_trav_f read the same work list and write different things (the hit record / the
    // candidate lists; each has its own cursor), so they go to two streams and wf_replay, which merges into the hit
    // record, follows both.  With full grids the F-tree walkers move in as the reference walkers run out of queue and leave
    // (HEAD 98.5 -> 96.5 ms).  Sharing every CU from the start — half the wave slots each — gains nothing: 68 ms for the
    // pair, exactly the 43 + 25 ms they take one after the other (VALU issue 0.71 + 0.34: together they saturate it).
    s.side_by_side = s.ref_walk && masks.ts && knobs.conc != 0;
    s.split_enabled = s.have_walkers && knobs.split != 0;
    // further shade + intersect rounds inside one wf_main launch: one when meshes park part of every wave's rays for the walker
    // (cfg2: 1 / 2 / 3 rounds -> 99 / 101 / 103 ms), two in a scene without meshes, where every live lane can go on
    // (cfg5 at 512 spp: 1 / 2 / 3 / 5 rounds -> 281.6 / 271.8 / 278.4 / 287.7 ms; the cfg1 scene at 1080p: 46.6 / 42.9 / 47.4 / 48.1 ms)
    s.fuse_max = knobs.fuse_max ? knobs.fuse_max : (sc.S.n_meshes == 0 ? 2u : 1u);
    s.fuse_min = knobs.fuse_min < 1 ? 1 : knobs.fuse_min; s.tail_fuse_max = path_depth + 2u;
    // Tail threshold (MI_RT_WF_TAIL_PATHS): without meshes 4 Mi paths, the size below which passes are launched without waiting
    // (cfg1 as BASELINE states it, 400x400 / 16 spp: 0.64 ms at 0, 0.55 at 64 Ki ... 2 Mi, 0.49 from 3 Mi on; cfg1 / cfg5 at
    // 1080p unchanged up to 8 Mi); with meshes 1 Mi (a 1/8 share of cfg2: 11.0 ms up to 2 Mi, 11.1 at 4 Mi, 11.3 at 8 Mi).
    s.tail_paths = knobs.tail_paths != 0xffffffffu ? knobs.tail_paths : (s.have_walkers ? (1u << 20) : (4u << 20));
    const uint32_t cus = (uint32_t)n_cus, travf_bpc = knobs.travf_bpc > 0 ? (uint32_t)knobs.travf_bpc : 6u;
    const uint32_t conc_trav_bpc = knobs.conc_trav_bpc > 0 ? (uint32_t)knobs.conc_trav_bpc : walker.blocks_per_cu;
    const uint32_t conc_travf_bpc = knobs.conc_travf_bpc > 0 ? (uint32_t)knobs.conc_travf_bpc : travf_bpc;
    s.walker_blocks = cus * (s.side_by_side ? conc_trav_bpc : walker.blocks_per_cu);
    s.travf_blocks = cus * (s.side_by_side ? conc_travf_bpc : travf_bpc);
    s.replay_blocks = cus * 8u; s.filter_blocks_per_shard = 8u;
    return s;
}

// The grid of pass `it` comes from the header of pass it - 1.  While that pass is still running the host would have to wait for
// it (the header is on its way while the walkers run, so for a big pass the wait is hidden); a SMALL pass is launched at once
// instead, on a grid that is an upper bound — live paths only decrease, and every (class, shard) list may end in a partial
// block — whose surplus blocks leave at their first instruction (wf_main compares its block number with the device-side table).
// The host runs at most kRunAhead passes ahead of the headers.
uint32_t pass_grid_bound(uint32_t live) { return live / (uint32_t)kBlock + 2u * (uint32_t)kWfShards; }

PassGate pass_gate(const PassSchedule& s, uint32_t it, uint32_t seen, uint32_t live) {
    if (seen == it) return PassGate::kExact;
    if (s.nowait_blocks == 0 || pass_grid_bound(live) > s.nowait_blocks || it - seen > kRunAhead) return PassGate::kWait;
    return PassGate::kBound;
}

PassPlan plan_pass(const PassSchedule& s, uint32_t it, bool exact, const PassHdr& last) {
    PassPlan p;
    p.grid_all = exact ? last.blocks : pass_grid_bound(last.live);
    p.grid_a = exact ? last.blocks_a : p.grid_all;
    if (it == 0) { p.grid_all = last.blocks; p.grid_a = 0; }          // the camera pass: last = camera_pass_header
    p.stop = p.grid_all == 0;
    // THE TAIL.  Once the live paths no longer fill the chip (last.live bounds this pass' input: paths only end), thin waves
    // cost nothing — there is nobody to give their lanes to — while every further pass costs two launches and a header.
    // So each wave keeps shading as long as ANY of its lanes can go on (a path that enters a mesh root still parks for
    // the walker).  Per path the operations and their order are those of the pass-by-pass schedule.  Without meshes
    // nothing ever parks: this launch ends every path and is the last one.  (Threshold: pass_schedule.)
    p.tail = it > 0 && s.tail_paths != 0 && last.live <= s.tail_paths;      // (the camera pass in this form too: 0.49 -> 0.58 ms on cfg1 as stated)
    p.last = p.tail && !s.have_walkers;
    p.fuse_max = p.tail ? s.tail_fuse_max : s.fuse_max; p.fuse_min = p.tail ? 1u : s.fuse_min;
    // A pass after the first is launched in TWO PARTS.  Its class-A blocks (paths whose pending hit is a plain Triangle /
    // Plane: nothing a walker could still change) go to a second stream, ordered only behind the previous pass' wf_prefix:
    // they fill the CUs the persistent walkers of that pass leave idle as their queue runs out (a walker launch ends
    // with ~0.1 ms of tail whatever its queue size, eleven times per frame and per rank).  The class-B blocks follow the
    // walkers on the main stream; wf_prefix waits for both parts.  Same blocks, same work, another schedule.
    p.split = it > 0 && s.split_enabled && (!exact || (p.grid_a >= 64u && p.grid_a < p.grid_all));
    p.grid_b = exact ? p.grid_all - p.grid_a : p.grid_all;
    return p;
}

FinishPlan finish_plan(uint32_t levels, uint32_t dilate, bool want_valid, bool with_var, bool want_var) {
    const uint32_t passes = levels + dilate;
    auto mask_after = [&](uint32_t k) { return k == dilate && want_valid ? FinishMask::kCaller : k & 1u ? FinishMask::kPing1 : FinishMask::kPing0; };
    auto var_after = [&](uint32_t k) {
        return !with_var ? FinishVar::kNone : k == levels && want_var ? FinishVar::kCaller : k & 1u ? FinishVar::kPing1 : FinishVar::kPing0;
    };
    FinishPlan plan{ passes == 0 ? 1u : 0u, mask_after(0), var_after(0), {} };
    FinishImage src = FinishImage::kInput;
    for (uint32_t p = 0; p < passes; p++) {
        const bool level = p < levels;
        const uint32_t k = p - levels;                                      // a dilation's number
        const FinishImage dst = p + 1 == passes ? FinishImage::kOutput : p & 1u ? FinishImage::kPing1 : FinishImage::kPing0;
        plan.passes.push_back({ level, level ? 1u << p : 0u, src, dst,
                                level ? FinishMask::kNone : mask_after(k), level ? FinishMask::kNone : mask_after(k + 1),
                                level ? var_after(p) : FinishVar::kNone, level ? var_after(p + 1) : FinishVar::kNone });
        src = dst;
    }
    return plan;
}

uint32_t mip_full_chain(uint32_t width, uint32_t height) {
    uint32_t levels = 1;
    for (uint32_t n = std::max(width, height); n > 1; n = (n + 1) >> 1) levels++;
    return levels;
}

bool mip_plan(uint32_t width, uint32_t height, uint32_t levels, uint32_t per_launch, MipPlan* plan) {
    if (width == 0 || width > 32768u || height == 0 || height > 32768u) return false;
    const uint32_t full = mip_full_chain(width, height);
    if (levels > full) return false;
    MipPlan p{};
    p.levels = levels ? levels : full;
    for (uint32_t l = 0; l < p.levels; l++) {
        p.level[l] = { mip_extent(width, l), mip_extent(height, l), p.texels };
        if (l) p.texels += (uint64_t)p.level[l].width * p.level[l].height;
    }
    per_launch = std::min(std::max(per_launch, 1u), kMipFuse);
    for (uint32_t src = 0; src + 1 < p.levels; src += per_launch) p.launches.push_back({ src, std::min(per_launch, p.levels - 1 - src) });
    *plan = p;
    return true;
}

// The block layout of a BC6H chain, stated once: level l of W_l x H_l texels is ceil(W_l / 4) x ceil(H_l / 4) blocks of 16 bytes,
// row-major; level 0 is a buffer of its own and levels 1 .. L - 1 lie one after the other in a second one, offsets in blocks.
Bc6hPlan bc6h_plan(const MipPlan& mips) {
    Bc6hPlan p{};
    p.levels = mips.levels;
    for (uint32_t l = 0; l < p.levels; l++) {
        p.level[l] = { bc6h_extent(mips.level[l].width), bc6h_extent(mips.level[l].height), p.blocks };
        if (l) p.blocks += (uint64_t)p.level[l].bw * p.level[l].bh;
    }
    return p;
}

}  // namespace pt
