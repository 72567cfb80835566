// render_plan_shim.cpp — CPU entry into the render planner (TEST INFRASTRUCTURE, compiled with render_plan.cpp and
// scene_compile.cpp by tests/test_render_plan_host.py, tests/test_pass_schedule_host.py and tests/test_finish_plan_host.py with
// g++ -ffp-contract=off into a shared object loaded with ctypes).
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

// mirrored by ScheduleQuery in tests/test_pass_schedule_host.py: the wavefront pipeline's pass schedule for a scene of n_meshes live
// meshes (bit m of qualifies / default_ts: CompiledScene::Mesh m, m < 32), then the gate and the plan of one pass under it
struct ScheduleQuery {
    // pass_schedule's inputs.  have_masks: ref_mask / ts_mask are given instead of taken from walk_masks(scene, flags)
    int32_t n_meshes; uint32_t qualifies, default_ts, flags;
    int32_t have_masks; uint32_t ref_mask, ts_mask;
    uint32_t walker_bpc; int32_t n_cus; uint32_t path_depth;
    int32_t split, conc, conc_trav_bpc, conc_travf_bpc, travf_bpc;
    uint32_t tail_paths, nowait_blocks, fuse_max, fuse_min;
    // the pass: gate(it, seen, hdr_live), plan(it, exact, header); n_in != 0: the header is camera_pass_header(n_in)
    uint32_t it, seen; int32_t exact; uint32_t n_in, hdr_blocks, hdr_live, hdr_blocks_a;
    // out: the schedule
    uint32_t s_ref_mask, s_ts_mask; int32_t have_walkers, ref_walk, side_by_side, split_enabled;
    uint32_t s_fuse_max, s_fuse_min, tail_fuse_max, s_tail_paths, s_nowait_blocks;
    uint32_t walker_blocks, travf_blocks, replay_blocks, filter_blocks_per_shard;
    // out: the gate (0 exact, 1 upper bound, 2 wait) and the bound for hdr_live; the plan
    int32_t gate; uint32_t bound;
    int32_t stop, p_split, tail, last; uint32_t grid_all, grid_a, grid_b, p_fuse_max, p_fuse_min;
};

// the knobs as a context without any MI_RT_WF_* variable has them
extern "C" void pass_schedule_defaults(ScheduleQuery* q) {
    const pt::ScheduleKnobs k;
    q->split = k.split; q->conc = k.conc; q->conc_trav_bpc = k.conc_trav_bpc; q->conc_travf_bpc = k.conc_travf_bpc; q->travf_bpc = k.travf_bpc;
    q->tail_paths = k.tail_paths; q->nowait_blocks = k.nowait_blocks; q->fuse_max = k.fuse_max; q->fuse_min = k.fuse_min;
}

extern "C" void pass_schedule_query(ScheduleQuery* q) {
    pt::CompiledScene sc;
    sc.S.n_meshes = q->n_meshes;
    for (int m = 0; m < q->n_meshes; m++) {
        pt::CompiledScene::Mesh mesh{};
        mesh.qualifies = m < 32 && ((q->qualifies >> m) & 1u); mesh.default_ts = m < 32 && ((q->default_ts >> m) & 1u);
        sc.meshes.push_back(mesh);
    }
    pt::ScheduleKnobs k;
    k.split = q->split; k.conc = q->conc; k.conc_trav_bpc = q->conc_trav_bpc; k.conc_travf_bpc = q->conc_travf_bpc; k.travf_bpc = q->travf_bpc;
    k.tail_paths = q->tail_paths; k.nowait_blocks = q->nowait_blocks; k.fuse_max = q->fuse_max; k.fuse_min = q->fuse_min;
    pt::WalkerPlan walker{};
    walker.blocks_per_cu = q->walker_bpc;
    const pt::WalkMasks masks = q->have_masks ? pt::WalkMasks{ q->ref_mask, q->ts_mask } : pt::walk_masks(sc, q->flags);
    const pt::PassSchedule s = pt::pass_schedule(sc, masks, walker, q->n_cus, q->path_depth, k);
    q->s_ref_mask = s.ref_mask; q->s_ts_mask = s.ts_mask;
    q->have_walkers = s.have_walkers; q->ref_walk = s.ref_walk; q->side_by_side = s.side_by_side; q->split_enabled = s.split_enabled;
    q->s_fuse_max = s.fuse_max; q->s_fuse_min = s.fuse_min; q->tail_fuse_max = s.tail_fuse_max;
    q->s_tail_paths = s.tail_paths; q->s_nowait_blocks = s.nowait_blocks;
    q->walker_blocks = s.walker_blocks; q->travf_blocks = s.travf_blocks; q->replay_blocks = s.replay_blocks;
    q->filter_blocks_per_shard = s.filter_blocks_per_shard;
    q->gate = (int32_t)pt::pass_gate(s, q->it, q->seen, q->hdr_live);
    q->bound = pt::pass_grid_bound(q->hdr_live);
    pt::PassHdr h = { q->hdr_blocks, q->hdr_live, 0u, 0u, q->hdr_blocks_a, 0u };
    if (q->n_in) h = pt::camera_pass_header(q->n_in);
    const pt::PassPlan p = pt::plan_pass(s, q->it, q->exact != 0, h);
    q->stop = p.stop; q->p_split = p.split; q->tail = p.tail; q->last = p.last;
    q->grid_all = p.grid_all; q->grid_a = p.grid_a; q->grid_b = p.grid_b; q->p_fuse_max = p.fuse_max; q->p_fuse_min = p.fuse_min;
}

// mirrored by FinishPlanQuery in tests/test_finish_plan_host.py: finish_plan as plain numbers, the slots by their enums' values
// (images: 0 input, 1 output, 2 ping 0, 3 ping 1; masks and variances: 0 ping 0, 1 ping 1, 2 the caller's, 3 untouched).  A pass is
// eight words: level, step, image in, image out, mask in, mask out, variance in, variance out.  Returns the number of passes, or
// -1 when they do not fit passes_cap.
struct FinishPlanQuery {
    uint32_t levels, dilate; int32_t want_valid, with_var, want_var;
    uint32_t copy, mask_init, var_init;
    uint32_t* passes; uint32_t passes_cap;
};

extern "C" int finish_plan_query(FinishPlanQuery* q) {
    const pt::FinishPlan plan = pt::finish_plan(q->levels, q->dilate, q->want_valid != 0, q->with_var != 0, q->want_var != 0);
    q->copy = plan.copy; q->mask_init = (uint32_t)plan.mask_init; q->var_init = (uint32_t)plan.var_init;
    if (plan.passes.size() > q->passes_cap) return -1;
    uint32_t* w = q->passes;
    for (const pt::FinishPass& p : plan.passes) {
        const uint32_t words[8] = { p.level ? 1u : 0u, p.step, (uint32_t)p.src, (uint32_t)p.dst, (uint32_t)p.mask_in, (uint32_t)p.mask_out,
                                    (uint32_t)p.var_in, (uint32_t)p.var_out };
        memcpy(w, words, sizeof words);
        w += 8;
    }
    return (int)plan.passes.size();
}
