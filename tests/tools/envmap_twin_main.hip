// envmap_twin_main.hip -- a stand-alone host program over the rules of bevyray_amd/csrc/brt_envmap.h for a sanitizer build (no GPU is
// touched): cubes of edge 1, 2, 3, 8, 16 and 17 with NaN / INF / 3e38 / denormal / -0.0 texels at an address that is only 4-byte
// aligned, tables of 1, 63 and 256 taps with NaN, INF, zero and negative components and weights, every size pair, the box level, the
// directions and the resolve.
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Ibevyray_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -o envmap_twin_main tests/tools/envmap_twin_main.hip && ./envmap_twin_main
// prints "ok <hash>".  tests/test_envmap.py builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "brt_envmap.h"
using namespace brt;
static uint64_t mix(uint64_t h, float4 t) {
    return h * 1315423911u + envmap_bits(t.x) + envmap_bits(t.y) * 3u + envmap_bits(t.z) * 7u + envmap_bits(t.w) * 11u;
}
int main() {
    std::mt19937 g(7);
    std::uniform_real_distribution<float> u(-1.f, 4.f), s(-1.5f, 1.5f);
    const float special[] = {3e38f, -3e38f, 1e-42f, -0.0f, NAN, INFINITY, -INFINITY, 0.0f};
    const uint32_t sizes[] = {1, 2, 3, 8, 16, 17}, taps_n[] = {1, 63, 256};
    uint64_t h = 0;
    for (uint32_t src : sizes) {
        // the cube deliberately at an address that is only 4-byte aligned, and exactly as long as the rule may read
        std::vector<float> cube((size_t)envmap_texels(src) * 4 + 1);
        for (auto& x : cube) x = (g() % 40 == 0) ? special[g() % 8] : u(g);
        for (uint32_t n : taps_n) {
            std::vector<float> taps((size_t)n * 4 + 1);
            for (auto& x : taps) x = (g() % 30 == 0) ? special[g() % 8] : s(g);      // (directions of any length, the zero vector among them)
            for (uint32_t dst : sizes)
                for (uint32_t i = 0; i < envmap_texels(dst); i++) h = mix(h, envmap_filter(cube.data() + 1, src, taps.data() + 1, n, dst, i));
        }
        if (src % 2 == 0)
            for (uint32_t i = 0; i < envmap_texels(src / 2); i++) h = mix(h, envmap_box(cube.data() + 1, src, i));
        for (uint32_t i = 0; i < envmap_texels(src); i++) {
            uint32_t face, x, y;
            float d[3];
            envmap_texel_of(src, i, &face, &x, &y);
            envmap_direction(src, face, x, y, d);
            h = mix(h, envmap_resolve(make_float4(d[0], d[1], d[2], cube[1 + i]), g() % 16));
        }
    }
    {   // the largest cube of the step exports: the last texel's index and direction
        uint32_t face, x, y;
        float d[3];
        envmap_texel_of(kEnvmapMaxSize, envmap_texels(kEnvmapMaxSize) - 1u, &face, &x, &y);
        envmap_direction(kEnvmapMaxSize, face, x, y, d);
        if (face != 5u || x != kEnvmapMaxSize - 1u || y != kEnvmapMaxSize - 1u) return 1;
        h = mix(h, make_float4(d[0], d[1], d[2], 0.f));
    }
    std::printf("ok %llx\n", (unsigned long long)h);
    return 0;
}
