// progressive_twin_main.hip -- a stand-alone host program over the record and the rule of bevyray_amd/csrc/brt_progressive.h for a
// sanitizer build (no GPU is touched).  It reads a board written by tests/test_progressive.py -- {u32 width, height, target, radius,
// f32 threshold, u32 n_colours}, width * height 32-byte records, n_colours rgb triples -- into buffers at odd addresses, classifies every
// pixel from its 3x3 window clipped to the frame, then accumulates every colour into every record, and writes the class bytes followed
// by the accumulated records.  The board holds NaN, +-INF, 3e38, denormal and -0.0 in every float field, counts 0, 1, 2, T - 1 and T.
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Ibevyray_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -o progressive_twin_main tests/tools/progressive_twin_main.hip
//   ./progressive_twin_main board.bin out.bin
// prints "ok <pixels>".  tests/test_progressive.py builds and runs it and holds the output to the numpy restatement.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "brt_progressive.h"
using namespace brt;

static std::vector<unsigned char> slurp(const char* path) {
    std::vector<unsigned char> v;
    FILE* f = std::fopen(path, "rb");
    if (!f) return v;
    unsigned char buf[4096];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return v;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const std::vector<unsigned char> in = slurp(argv[1]);
    if (in.size() < 24) return 3;
    uint32_t head[6];
    std::memcpy(head, in.data(), sizeof head);
    const uint32_t w = head[0], h = head[1], target = head[2], radius = head[3], n_col = head[5];
    float threshold;
    std::memcpy(&threshold, &head[4], 4);
    const size_t px = (size_t)w * h;
    if (radius > 1u || in.size() != 24 + px * 32 + (size_t)n_col * 12) return 4;
    // the records and colours at odd addresses
    std::vector<unsigned char> recs(1 + px * 32), cols(1 + (size_t)n_col * 12);
    std::memcpy(recs.data() + 1, in.data() + 24, px * 32);
    std::memcpy(cols.data() + 1, in.data() + 24 + px * 32, (size_t)n_col * 12);
    auto rec_at = [&](size_t p) { ProgPixel r; std::memcpy(&r, recs.data() + 1 + p * 32, 32); return r; };
    std::vector<unsigned char> out(px + px * 32);
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            const size_t p = (size_t)y * w + x;
            out[p] = (unsigned char)prog_classify(rec_at(p).n, target, (int)radius, [&](int dx, int dy) {
                const int qx = (int)x + dx, qy = (int)y + dy;
                if (qx < 0 || qy < 0 || qx >= (int)w || qy >= (int)h) return false;
                const ProgPixel q = rec_at((size_t)qy * w + (size_t)qx);
                return prog_noisy(q.m1, q.m2, q.n, threshold);
            });
        }
    for (size_t p = 0; p < px; p++) {
        ProgPixel r = rec_at(p);
        for (uint32_t c = 0; c < n_col; c++) {
            float rgb[3];
            std::memcpy(rgb, cols.data() + 1 + (size_t)c * 12, 12);
            prog_accumulate(r, rgb[0], rgb[1], rgb[2]);
        }
        std::memcpy(out.data() + px + p * 32, &r, 32);
    }
    FILE* f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), 1, out.size(), f) != out.size()) return 5;
    std::fclose(f);
    std::printf("ok %zu\n", px);
    return 0;
}
