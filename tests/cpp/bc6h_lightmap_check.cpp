// Stand-alone driver of the host mirror's BC6H code (host/tracing.hpp Scene::encode_lightmap_bc6h, Scene::decode_lightmap_bc6h,
// Scene::lightmap_bc6h_layout) for tests/test_lightmap_bc6h_host.py: no GPU, no context.
//   bc6h_lightmap_check encode <width> <height> <rounds> <in: f32 image file> <valid file, or -> <out: block file>
//   bc6h_lightmap_check decode <width> <height> <in: block file> <out: f32 image file>
//   bc6h_lightmap_check layout <width> <height> <levels>          (prints "bw bh offset" per level)
// The files are raw little-endian arrays, the bytes the numpy helpers lightmap_bc6h_encode / lightmap_bc6h_decode read and write.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../cs397raytracingsp22_amd/host/tracing.hpp"

static std::vector<uint8_t> slurp(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) { std::perror(path); std::exit(2); }
    std::vector<uint8_t> data;
    uint8_t buf[65536];
    for (size_t got; (got = std::fread(buf, 1, sizeof buf, f)) > 0;) data.insert(data.end(), buf, buf + got);
    std::fclose(f);
    return data;
}

static void spill(const char* path, const void* data, size_t bytes) {
    FILE* f = std::fopen(path, "wb");
    if (!f || std::fwrite(data, 1, bytes, f) != bytes) { std::perror(path); std::exit(2); }
    std::fclose(f);
}

int main(int argc, char** argv) {
    if (argc < 5) { std::fprintf(stderr, "usage: %s encode|decode|layout width height ...\n", argv[0]); return 2; }
    const uint32_t width = (uint32_t)std::atoi(argv[2]), height = (uint32_t)std::atoi(argv[3]);
    try {
        if (!std::strcmp(argv[1], "encode") && argc == 8) {
            const std::vector<uint8_t> in = slurp(argv[5]);
            std::vector<float> image(in.size() / 4);
            std::memcpy(image.data(), in.data(), image.size() * 4);
            const std::vector<uint8_t> valid = std::strcmp(argv[6], "-") ? slurp(argv[6]) : std::vector<uint8_t>();
            const std::vector<uint8_t> out = cs397::Scene::encode_lightmap_bc6h(image, valid, width, height, (uint32_t)std::atoi(argv[4]));
            spill(argv[7], out.data(), out.size());
        } else if (!std::strcmp(argv[1], "decode") && argc == 6) {
            const std::vector<float> out = cs397::Scene::decode_lightmap_bc6h(slurp(argv[4]), width, height);
            spill(argv[5], out.data(), out.size() * 4);
        } else if (!std::strcmp(argv[1], "layout") && argc == 5) {
            for (const auto& l : cs397::Scene::lightmap_bc6h_layout(width, height, (uint32_t)std::atoi(argv[4])))
                std::printf("%u %u %zu\n", l.bw, l.bh, l.offset);
        } else {
            std::fprintf(stderr, "usage: %s encode|decode|layout width height ...\n", argv[0]);
            return 2;
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
