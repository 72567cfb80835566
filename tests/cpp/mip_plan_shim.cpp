// The lightmap mip chain's plan as plain numbers: cs397raytracingsp22_amd/csrc/render_plan.cpp mip_plan, compiled with g++ beside
// render_plan.cpp and scene_compile.cpp by tests/test_lightmap_mips_host.py.  No GPU, no libmi_rt.so.
#include <cstdint>

#include "../../cs397raytracingsp22_amd/csrc/render_plan.hpp"

// (scene_compile.cpp reports through pt::fail, which libmi_rt.so defines in mi_rt.cpp: nothing here can fail that way)
int pt::fail(int code, const char*, ...) { return code; }

// mirrored by MipPlanQuery in tests/test_lightmap_mips_host.py.  level_size: 2 words per level (width, height), level_offset: its offset
// in texels; launches: 2 words each (the level read, the levels written).  Returns the number of launches, or -1: refused.
struct MipPlanQuery {
    uint32_t width, height, levels, per_launch;
    uint32_t n_levels, full_chain;
    uint64_t texels;
    uint32_t level_size[2 * 16];
    uint64_t level_offset[16];
    uint32_t launches[2 * 16];
};

extern "C" int mip_plan_query(MipPlanQuery* q) {
    pt::MipPlan plan;
    if (!pt::mip_plan(q->width, q->height, q->levels, q->per_launch, &plan)) return -1;
    q->n_levels = plan.levels; q->texels = plan.texels; q->full_chain = pt::mip_full_chain(q->width, q->height);
    for (uint32_t l = 0; l < plan.levels; l++) {
        q->level_size[2 * l] = plan.level[l].width; q->level_size[2 * l + 1] = plan.level[l].height;
        q->level_offset[l] = plan.level[l].offset;
    }
    if (plan.launches.size() > 16) return -2;
    for (size_t i = 0; i < plan.launches.size(); i++) { q->launches[2 * i] = plan.launches[i].src; q->launches[2 * i + 1] = plan.launches[i].count; }
    return (int)plan.launches.size();
}
