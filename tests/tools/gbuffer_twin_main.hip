// gbuffer_twin_main.hip -- a stand-alone host program over the rule of bevyray_amd/csrc/brt_gbuffer.h for a sanitizer build (no GPU is
// touched): cameras, previous cameras, spheres and hit distances of random and special values (NaN, INF, 3e38, denormal and -0.0 fields,
// a zero `up`, a zero direction) read from buffers at odd addresses, every depth mode, hits and misses, moved and unmoved spheres; the
// invariants of the rule (the identity case, the NO_PREVIOUS contract, the packed words); the Rgb10a2Unorm channel over its clamp, NaN
// and every level; and the f32 -> f16 conversion against the
// compiler's own (_Float16, round to nearest even) on every f32 whose low 13 bits sit at, just below or just above a tie.
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Ibevyray_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -o gbuffer_twin_main tests/tools/gbuffer_twin_main.hip && ./gbuffer_twin_main
// prints "ok <hash>".  tests/test_gbuffer.py builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "brt_gbuffer.h"
using namespace brt;
static uint32_t bits(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }
static float at(const std::vector<unsigned char>& buf, size_t i) { float f; std::memcpy(&f, buf.data() + 1 + 4 * i, 4); return f; }
static uint32_t f16_of(float f) {
    const _Float16 h = (_Float16)f;
    uint16_t u;
    std::memcpy(&u, &h, 2);
    return u;
}
int main() {
    std::mt19937 g(13);
    std::uniform_real_distribution<float> u(-20.f, 20.f), p(0.05f, 3.f);
    const float special[] = {3e38f, -3e38f, 1e-42f, -0.0f, NAN, INFINITY, -INFINITY, 0.0f};
    uint64_t h = 0;
    for (uint32_t c = 0; c < 4000u; c++) {
        // 36 floats from byte 1 on: two cameras (position, direction, up, aspect, tan_half, near, far), sphere now, sphere before, t
        std::vector<unsigned char> buf(1 + 36 * 4);
        for (size_t i = 0; i < 36; i++) {
            float x = (c % 3 == 0 && g() % 6 == 0) ? special[g() % 8] : ((i % 13) >= 9 && i < 26 ? p(g) : u(g));
            std::memcpy(buf.data() + 1 + 4 * i, &x, 4);
        }
        GbufferCam cams[2];
        for (int k = 0; k < 2; k++) {
            float pos[3], dir[3], up[3];
            for (int j = 0; j < 3; j++) {
                pos[j] = at(buf, 13 * k + j);
                dir[j] = (c % 19 == 0) ? 0.0f : at(buf, 13 * k + 3 + j);
                up[j] = (c % 17 == 0) ? 0.0f : at(buf, 13 * k + 6 + j);
            }
            cams[k] = gbuffer_cam_of(pos, dir, up, at(buf, 13 * k + 9), at(buf, 13 * k + 10), at(buf, 13 * k + 11), 1000.0f * at(buf, 13 * k + 12));
        }
        if (c % 5 == 0) cams[1] = cams[0];
        const GbufferView gv = gbuffer_view_of(cams[0], cams[1]);
        if ((c % 5 == 0) && !gv.same_camera) return 1;
        float sn[4], so[4];
        for (int j = 0; j < 4; j++) { sn[j] = at(buf, 26 + j); so[j] = (c % 2) ? sn[j] : at(buf, 30 + j); }
        const float ts[3] = {std::fabs(at(buf, 34)), INFINITY, at(buf, 35)};
        const uint32_t W = 1u + g() % 4000u, H = 1u + g() % 3000u, px = g() % W, py = g() % H;
        float d[3];
        gbuffer_host_dir(cams[0], 1.0f / (float)(1u + g() % 2000u), 1.0f / 777.0f, W, H, px, py, d);
        for (uint32_t mode = 0; mode < 3u; mode++)
            for (float t : ts) {
                GbufferPixel q;
                gbuffer_pixel(cams[0], gv, mode, W, H, px, py, d, t, sn, so, q);
                const bool hit = t < INFINITY;
                if (((q.status & GBUF_HIT) != 0u) != hit) return 2;
                if (q.status & GBUF_NO_PREVIOUS) {
                    if (q.xp == q.xp || q.yp == q.yp || bits(q.mu) != 0u || bits(q.mv) != 0u) return 3;
                } else if (!(q.xp > -1.0f && q.xp < (float)W && q.yp > -1.0f && q.yp < (float)H)) {
                    return 4;
                }
                if (gv.same_camera && !(q.status & GBUF_MOVED)) {           // the identity
                    if (q.status & GBUF_NO_PREVIOUS) return 5;
                    if (q.xp != (float)px || q.yp != (float)py || bits(q.mu) != 0u || bits(q.mv) != 0u) return 6;
                }
                if (!hit && (q.status & (GBUF_MOVED | GBUF_FRONT_FACE))) return 7;
                const uint32_t packed = gbuffer_rgb10a2(q.n, hit);
                if (hit ? (packed >> 30) != 3u : packed != 0u) return 8;
                if (gbuffer_f16(q.mu) != f16_of(q.mu) || gbuffer_f16(q.mv) != f16_of(q.mv)) return 9;
                h = h * 1315423911u + bits(q.depth) * 3u + q.status + packed + (q.xp == q.xp ? bits(q.xp) : 1u) + bits(q.mu) * 7u;
            }
    }
    // the Rgb10a2Unorm channel on the values no unit normal reaches: the clamp on both sides, NaN, the infinities, the zeros
    // (tests/test_gbuffer.py holds the numpy restatement to the same table)
    {
        const float edge[12] = {-1.0f, 1.0f, -1.5f, 1.5f, NAN, INFINITY, -INFINITY, -0.0f, 0.0f, 3e38f, -3e38f, 1e-45f};
        const uint32_t want[12] = {0u, 1023u, 0u, 1023u, 0u, 1023u, 0u, 512u, 512u, 1023u, 0u, 512u};
        for (int i = 0; i < 12; i++)
            if (gbuffer_unorm10(edge[i]) != want[i]) { std::printf("unorm10 of entry %d: %u, want %u\n", i, gbuffer_unorm10(edge[i]), want[i]); return 12; }
        const float n[3] = {NAN, 1.5f, -1.5f};
        if (gbuffer_rgb10a2(n, true) != ((3u << 30) | (1023u << 10)) || gbuffer_rgb10a2(n, false) != 0u) return 13;
        for (uint32_t k = 0; k < 1024u; k++) {                  // every level, by its own value
            const float v = (float)(((double)k / 1023.0) * 2.0 - 1.0);
            if (gbuffer_unorm10(v) != k) return 14;
        }
    }
    // the f16 conversion on every rounding boundary: all exponents and high mantissa bits, the low 13 bits around the tie
    for (uint32_t hi = 0; hi < (1u << 19); hi++)
        for (uint32_t lo : {0x0000u, 0x0001u, 0x0fffu, 0x1000u, 0x1001u, 0x1fffu}) {
            const uint32_t w = (hi << 13) | lo;
            const float f = gbuffer_float(w);
            if (f != f) continue;                       // (which NaN comes back is the converter's choice)
            if (gbuffer_f16(f) != f16_of(f)) { std::printf("f16 of %08x: %04x, want %04x\n", w, gbuffer_f16(f), f16_of(f)); return 10; }
        }
    // subnormal halves: the tie sits lower in the word
    for (uint32_t e = 0x32800000u; e < 0x38800000u; e += 0x00800000u)
        for (uint32_t m = 0; m < (1u << 23); m += 0x3ffu) {
            const float f = gbuffer_float(e | m);
            if (gbuffer_f16(f) != f16_of(f) || gbuffer_f16(-f) != f16_of(-f)) return 11;
        }
    std::printf("ok %llx\n", (unsigned long long)h);
    return 0;
}
