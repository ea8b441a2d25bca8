// lens_twin_main.hip -- a stand-alone host program over the rule of bevyray_amd/csrc/brt_lens.h for a sanitizer build (no GPU is
// touched): cameras, windows and lenses of random and special values (NaN, INF, 3e38, denormal and -0.0 fields, radii 0, 1e-42 and 1e30,
// a zero `up`, a zero direction) read from buffers at odd addresses, every mode, chained samples, the origin bound.  The rejection loop
// must end for each of them: its test reads the two draws alone.
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Ibevyray_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -o lens_twin_main tests/tools/lens_twin_main.hip && ./lens_twin_main
// prints "ok <hash>".  tests/test_lens.py builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "brt_lens.h"
using namespace brt;
static uint32_t bits(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }
static uint64_t mix(uint64_t h, const float v[3]) { return h * 1315423911u + bits(v[0]) + bits(v[1]) * 3u + bits(v[2]) * 7u; }
// a float at an address that is odd
static float at(const std::vector<unsigned char>& buf, size_t i) { float f; std::memcpy(&f, buf.data() + 1 + 4 * i, 4); return f; }
int main() {
    std::mt19937 g(11);
    std::uniform_real_distribution<float> u(-20.f, 20.f), p(0.f, 3.f);
    const float special[] = {3e38f, -3e38f, 1e-42f, -0.0f, NAN, INFINITY, -INFINITY, 0.0f};
    const float radii[] = {0.0f, 1e-42f, 1e30f, 0.05f, 0.5f, NAN, INFINITY};
    uint64_t h = 0;
    for (uint32_t c = 0; c < 4000u; c++) {
        // 16 floats: position, direction, up, aspect, fov term, radius, focus, ortho_height, ndc0x, ndc0y -- 65 bytes, read from byte 1 on
        std::vector<unsigned char> buf(1 + 16 * 4);
        for (size_t i = 0; i < 16; i++) {
            float x = (c % 3 == 0 && g() % 6 == 0) ? special[g() % 8] : (i >= 9 ? p(g) : u(g));
            if (i == 11) x = radii[g() % 7];
            std::memcpy(buf.data() + 1 + 4 * i, &x, 4);
        }
        float pos[3], dir[3], up[3];
        for (int k = 0; k < 3; k++) { pos[k] = at(buf, k); dir[k] = at(buf, 3 + k); up[k] = (c % 17 == 0) ? 0.0f : at(buf, 6 + k); }
        if (c % 19 == 0) dir[0] = dir[1] = dir[2] = 0.0f;
        const uint32_t win_h = c % 23 == 0 ? 0u : 1u + g() % 2000u;
        const LensCam cam = lens_cam_of(pos, dir, up, at(buf, 9), at(buf, 10), win_h);
        for (uint32_t proj = 0; proj < 2u; proj++) {
            const LensView lv = lens_view_of(dir, proj, at(buf, 11), at(buf, 12), at(buf, 13));
            if (lv.mode > LENS_ORTHO || (proj == 1u) != (lv.mode == LENS_ORTHO)) return 1;
            uint32_t state = g();
            for (int s = 0; s < 3; s++) {
                float o[3], w[3], d[3];
                const uint32_t before = state;
                if (lens_ray_raw(cam, lv, lv.mode, at(buf, 14) - 1.5f, at(buf, 15) - 1.5f, state, o, w)) lens_normalize(w, d);
                else std::memcpy(d, w, sizeof d);
                if (state == before) return 2;      // (every mode draws the jitter)
                h = mix(mix(h, o), d) + state;
            }
            const float b = lens_origin_bound(cam, lv);
            h = h * 31u + bits(b);
        }
    }
    std::printf("ok %llx\n", (unsigned long long)h);
    return 0;
}
