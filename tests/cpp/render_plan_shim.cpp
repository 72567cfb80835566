// render_plan_shim.cpp — CPU entry into the render planner (TEST INFRASTRUCTURE, compiled with render_plan.cpp and
// scene_compile.cpp by tests/test_render_plan_host.py with g++ -ffp-contract=off into a shared object loaded with ctypes).
// It stands in for mi_rt.cpp: it defines pt::fail and runs what a render plans, without a GPU.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../cs397raytracingsp22_amd/csrc/render_plan.hpp"

namespace {
char g_err[512];
}

int pt::fail(int code, const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
    return code;
}

// mirrored by PlanQuery in tests/test_render_plan_host.py
struct PlanQuery {
    // op 0, tile masks: the scene compiled from `scene`, seen by `cam` on the grid of `world` ranks
    const mi_scene_desc* scene;
    const mi_camera_desc* cam;
    uint32_t flags;
    int32_t world;                 // 1 .. 8
    uint64_t* words;               // [words_cap]
    uint64_t words_cap;
    // op 1, batch: the first batch for (npix, spp, max_state_bytes, free_bytes, two_stage), then its sizes
    uint32_t npix, spp;
    uint64_t max_state_bytes, free_bytes;
    int32_t two_stage;
    // out
    int32_t applies;               // op 0: tile_masks returned true
    uint64_t n_words;              // op 0: mask words written
    uint64_t dead_samples[8];      // op 0: per rank, samples [0, spp) of its dead tiles
    uint64_t pixels[8];            // op 0: per rank, image pixels in its tiles
    uint32_t s_batch, region, cap;
    uint64_t state_bytes, samp_bytes, acc_bytes;
    char err[512];                 // the recorded message of a failure
};

// MI_OK or the failing call's code (message in q->err)
extern "C" int render_plan_query(int op, PlanQuery* q) {
    g_err[0] = 0;
    int rc = MI_OK;
    if (op == 0) {
        pt::CompiledScene sc;
        if ((rc = pt::compile_scene(q->scene, &sc)) == MI_OK && (rc = pt::check_camera(q->cam)) == MI_OK) {
            if (q->world < 1 || q->world > 8) return -100;
            const pt::TileGrid g = pt::tile_grid(q->cam, q->world);
            std::vector<uint64_t> masks;
            q->applies = pt::tile_masks(sc, *q->cam, q->flags, g.tx, masks) ? 1 : 0;
            q->n_words = q->applies ? masks.size() : 0;
            if (q->n_words > q->words_cap) return -101;
            if (q->n_words) memcpy(q->words, masks.data(), q->n_words * sizeof(uint64_t));
            for (int r = 0; r < q->world; r++) {
                q->dead_samples[r] = q->applies ? pt::dead_pixels(g, q->cam, r, q->world, masks) * q->cam->aa_sample_count : 0;
                q->pixels[r] = pt::rank_pixels(g, q->cam, r, q->world);
            }
        }
    } else if (op == 1) {
        if ((rc = pt::wf_first_batch(q->npix, q->spp, q->max_state_bytes, q->free_bytes, q->two_stage != 0, &q->s_batch)) == MI_OK) {
            const pt::WfBatch b = pt::wf_batch(q->npix, q->s_batch);
            q->region = b.region; q->cap = b.cap;
            q->state_bytes = b.state_bytes; q->samp_bytes = b.samp_bytes; q->acc_bytes = b.acc_bytes;
        }
    } else {
        return -102;
    }
    snprintf(q->err, sizeof q->err, "%s", g_err);
    return rc;
}
