// The block layout of a BC6H chain as plain numbers: cs397raytracingsp22_amd/csrc/render_plan.cpp bc6h_plan over mip_plan, compiled with
// g++ beside render_plan.cpp and scene_compile.cpp by tests/test_lightmap_bc6h_host.py.  No GPU, no libmi_rt.so.
#include <cstdint>

#include "../../cs397raytracingsp22_amd/csrc/render_plan.hpp"

// (scene_compile.cpp reports through pt::fail, which libmi_rt.so defines in mi_rt.cpp: nothing here can fail that way)
int pt::fail(int code, const char*, ...) { return code; }

// out: 3 words per level (blocks per row, block rows, offset in blocks); returns the number of levels, or -1: refused.  *blocks: the
// blocks of levels 1 ..
extern "C" int bc6h_plan_query(uint32_t width, uint32_t height, uint32_t levels, uint64_t* out, uint64_t* blocks) {
    pt::MipPlan mips;
    if (!pt::mip_plan(width, height, levels, 5, &mips)) return -1;
    const pt::Bc6hPlan plan = pt::bc6h_plan(mips);
    for (uint32_t l = 0; l < plan.levels; l++) { out[3 * l] = plan.level[l].bw; out[3 * l + 1] = plan.level[l].bh; out[3 * l + 2] = plan.level[l].offset; }
    *blocks = plan.blocks;
    return (int)plan.levels;
}
