// brt_progressive.h -- progressive frames (DESIGN.md "Progressive frames"): the record that describes a pixel of a Pure frame between two
// of its samples, the rule that says from a pixel's own samples whether it is still noisy, and the class of a pixel for a target sample
// count; shared by the kernels (brt_progressive.hip) and the host (brt_host_progressive_accumulate / _class) so that both are the same f32
// operations in the same order (-ffp-contract=off on both sides); and the host-callable launchers of the kernels.
// tests/progressive_ref.py restates the record and the rule in numpy.
#pragma once
#include <cstdint>

#include "brt_ploc.h"   // BRT_HD

namespace brt {

// ---- the record -------------------------------------------------------------------------------------------------------------------
// A pixel threads one RNG state through its samples (raytrace.wgsl:161-163) and the sample count enters only the final division (:169):
// between two samples a pixel is {rng, colour sum, samples so far}.  The record adds the two moments of the samples' luminance and the
// rays cast.  32 bytes, two 16-byte words: {sum.r, sum.g, sum.b, m1} {m2, rng, n, rays}.
//   all zero           a pixel without samples: its first sample starts from pixel_begin's seed; rng is ignored while n == 0
//   one sample c       (what the shader adds at :165) sum += c, then l = (0.2126 r + 0.7152 g) + 0.0722 b of c (the adaptive rule's and the
//                      denoiser's luminance), m1 += l, m2 += l * l, n += 1; rays gains the sample's raycasts
//   the pixel's value  {sum / (float)n, 1}; four zeros at n == 0
struct ProgPixel {
    float sum[3];
    float m1, m2;
    uint32_t rng, n, rays;
};
static_assert(sizeof(ProgPixel) == 32, "two 16-byte words");

constexpr uint32_t kProgSelected = 1u;             // BRT_PROG_SELECTED (include/bevyray_amd.h)
constexpr float kProgMeanFloor = 0.01f;
constexpr float kProgDefaultThreshold = 0.05f;      // brt_set_progressive's default: the lowest R of the grid of DESIGN.md section 26
constexpr uint32_t kProgMaxSamples = 65535u;

BRT_HD float prog_luma(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// the moments of one more sample of colour (r, g, b)
BRT_HD void prog_moments(float& m1, float& m2, float r, float g, float b) {
    const float l = prog_luma(r, g, b);
    m1 = m1 + l;
    m2 = m2 + l * l;
}
BRT_HD void prog_accumulate(ProgPixel& rec, float r, float g, float b) {
    rec.sum[0] = rec.sum[0] + r;
    rec.sum[1] = rec.sum[1] + g;
    rec.sum[2] = rec.sum[2] + b;
    prog_moments(rec.m1, rec.m2, r, g, b);
    rec.n = rec.n + 1u;
}

// ---- the rule ---------------------------------------------------------------------------------------------------------------------
// OWN FLAG of a pixel with n >= 2 samples (a pixel with fewer is quiet): m = m1 / n, v = max(0, m2 / n - m * m), e = v / n (the variance
// of the pixel's MEAN), t = threshold * max(m, 0.01); the pixel is NOISY iff e > t * t.  max(a, b) is a > b ? a : b: a NaN on the left
// gives b.  Non-finite moments: every compare with a NaN is false, so a NaN m1 or m2 leaves the pixel QUIET (v is 0, or e > t * t is
// false); m1 and m2 both +INF are quiet too (m2 / n - m * m = INF - INF = NaN, v = 0; and t * t = +INF).  The one non-finite case the
// formulas select is m2 alone overflowing while m * m stays finite (luminances of about 1e19): e = +INF, noisy at every threshold whose
// t * t stays finite.  The flag does not look at the colour sum: a non-finite sum does not improve with samples, and is not a reason
// to select.  tests/test_progressive.py pins all three cases.
// No exp, log or sqrt.
BRT_HD bool prog_noisy(float m1, float m2, uint32_t n, float threshold) {
    if (n < 2u) return false;
    const float nf = (float)n;
    const float m = m1 / nf;
    const float d = m2 / nf - m * m;
    const float v = d > 0.0f ? d : 0.0f;
    const float e = v / nf;
    const float t = threshold * (m > kProgMeanFloor ? m : kProgMeanFloor);
    return e > t * t;
}
// CLASS of pixel p for the target T: SELECTED iff n_p < T and a pixel of the (2 radius + 1)^2 window around p, clipped to the frame, is
// noisy (radius 0 or 1; p itself included).  noisy(dx, dy): the own flag of that pixel, false outside the frame.
template <class Noisy>
BRT_HD uint32_t prog_classify(uint32_t n_p, uint32_t target, int radius, Noisy&& noisy) {
    if (!(n_p < target)) return 0u;
    bool any = false;
    for (int dy = -radius; dy <= radius; dy++)
        for (int dx = -radius; dx <= radius; dx++) any = noisy(dx, dy) || any;
    return any ? kProgSelected : 0u;
}

}  // namespace brt

// ---- the kernels' launchers ---------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#include "brt_pixels.h"

namespace brt {

// What the progressive forms of the sparse pixel tracer take beyond a list of pixels (PixelsLaunch: the list, its count word, the frame
// the values are scattered into -- args.out null: no value is stored; args.scatter is 1).  Entry i names pixel p; the lane continues p's
// record to `target` samples and stores record and value.  A record with n >= target is left byte for byte (its value is still stored);
// an entry >= width * height is refused and touches nothing.  A pixel may be named once per launch: two entries of one pixel race.
// args.pixels null: every pixel of the frame -- order 0: entry i is pixel i (args.n_pixels = width * height); order 1: 64 consecutive
// entries are one 8x8 tile, row-major, tiles along x (args.n_pixels = 64 * tiles; the slots of a partial tile that lie outside the frame
// are passed over): a wave of the plain form holds one tile, a wave of the streaming form does with its first fetch (later refills take
// single entries).
struct ProgSample {
    ProgPixel* state;                // width * height records
    uint32_t target;                 // 1 .. 65535
    uint32_t order;
    unsigned long long* samples;     // the samples run, added up (nullptr: not counted)
};
hipError_t launch_prog_sample(const PixelsLaunch& pl, const ProgSample& pg);

// One selection over the width x height state plane: the class of every pixel for `target` (prog_classify).  list / count: the selected
// pixels are appended (count zeroed by the caller; the order is that of the waves' arrival), both null: nothing is appended.  mask: the
// class byte of every pixel (nullptr: not written).  One of the two must be there.
struct ProgSelect {
    uint32_t width, height;
    const ProgPixel* state;
    uint32_t target;
    float threshold;
    uint32_t radius;
    uint32_t* count;
    uint32_t* list;             // width * height words
    uint8_t* mask;
};
hipError_t launch_prog_select(const ProgSelect& ps, hipStream_t stream);

}  // namespace brt
#endif
