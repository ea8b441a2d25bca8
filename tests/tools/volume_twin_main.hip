// volume_twin_main.hip -- a stand-alone host program over the sampling rule of bevyray_amd/csrc/brt_volume.h for a sanitizer build (no GPU
// is touched): seven lattices, records with NaN / INF / 3e38 / denormal coefficients, refused statuses and wrong basis words at an
// address that is only 4-byte aligned, 20 000 points with the same specials, all four instantiations, and the lattice's probes.
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Ibevyray_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -o volume_twin_main tests/tools/volume_twin_main.hip && ./volume_twin_main
// prints "ok <hash>".  Its first run found the records addressed through a misaligned uint4 pointer on the host; volume_load16 now
// takes the buffer as bytes there.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "brt_volume.h"
using namespace brt;
template <uint32_t B, bool W>
static uint64_t run(const VolumeDesc& v, const std::vector<uint32_t>& rec, const std::vector<float>& pts, size_t n) {
    uint64_t h = 0;
    for (size_t i = 0; i < n; i++) {
        float rgb[3];
        // records deliberately at an address that is only 4-byte aligned
        uint32_t st = volume_sample<B, W>(v, rec.data() + 1, &pts[8 * i], &pts[8 * i + 4], rgb);
        h = h * 1315423911u + st + volume_bits(rgb[0]) + volume_bits(rgb[1]) * 3u + volume_bits(rgb[2]) * 7u;
    }
    return h;
}
int main() {
    std::mt19937 g(5);
    std::uniform_real_distribution<float> u(-3.f, 5.f);
    const uint32_t counts[][3] = {{1, 1, 1}, {2, 1, 1}, {1, 3, 1}, {2, 2, 2}, {5, 4, 3}, {3, 1, 7}, {1024, 1, 1}};
    const float special[] = {3e38f, -3e38f, 1e-42f, -0.0f, NAN, INFINITY, -INFINITY, 0.0f};
    uint64_t h = 0;
    for (auto& c : counts) {
        VolumeDesc v{{-1.5f, 0.25f, -2.0f}, 7u, {0.7f, 1.3f, 0.9f}, 0u, {c[0], c[1], c[2]}, 0u};
        const size_t n = (size_t)c[0] * c[1] * c[2], np = 20000;
        std::vector<uint32_t> rec(n * 32 + 1);
        for (size_t i = 0; i < n; i++) {
            for (int k = 0; k < 27; k++) rec[1 + i * 32 + k] = volume_bits((g() % 50 == 0) ? special[g() % 8] : u(g));
            rec[1 + i * 32 + 28] = (g() % 6 == 0) ? 4u : 0u;
            rec[1 + i * 32 + 30] = g() % 8 == 0 ? 1u : 0u;
        }
        std::vector<float> pts(np * 8);
        for (auto& x : pts) x = (g() % 40 == 0) ? special[g() % 8] : u(g);
        for (uint32_t basis = 0; basis < 2; basis++) {
            v.basis = basis;
            h += basis == 0 ? run<0, false>(v, rec, pts, np) + run<0, true>(v, rec, pts, np) : run<1, false>(v, rec, pts, np) + run<1, true>(v, rec, pts, np);
        }
        std::vector<uint4> pr(n);
        for (size_t i = 0; i < n; i++) pr[i] = volume_probe(v, (uint32_t)i);
        h += pr[n - 1].w;
    }
    std::printf("ok %llx\n", (unsigned long long)h);
    return 0;
}
