// brt_adaptive.h -- adaptive sampling (DESIGN.md "Adaptive sampling"): the rule that selects the pixels of a base frame that are traced
// again at the camera's own sample count, shared by the kernel (brt_adaptive.hip) and the host (brt_host_adaptive_class) so that both
// are the same f32 operations in the same order (-ffp-contract=off on both sides); and the host-callable launcher of the kernel.
// tests/adaptive_ref.py restates the rule in numpy.
#pragma once
#include <cstdint>

#include "brt_ploc.h"   // BRT_HD

namespace brt {

// ---- the rule ---------------------------------------------------------------------------------------------------------------------
// Pixel p of the base frame B with the full-size guides {t_p, id_p} (brt_denoise.h g0.w, g1.w):
//   l(c)   = (0.2126 r + 0.7152 g) + 0.0722 b, every operation separately rounded (the denoiser's luminance)
//   p has no class if it is sky (t_p = +INF) or l(B_p) is not finite
//   taps   the 5x5 window around p, dy outer and dx inner, both -2 .. 2, p included; a tap counts iff it is inside the frame, id_q == id_p
//          and l(B_q) is finite.  n = their number, S1 = sum l_q, S2 = sum l_q * l_q in f32 in that order
//   BRT_ADAPT_SPARSE (1)  iff n < min_taps
//   BRT_ADAPT_NOISY (2)   else iff v > thr * thr with m = S1 / n, v = max(0, S2 / n - m * m), thr = threshold * max(m, 0.01)
// max(a, b) is a > b ? a : b: a NaN on the left gives b.  Where S2 and m * m both overflow, S2 / n - m * m is INF - INF = NaN, v is 0 and
// the pixel is not NOISY.  Where S2 alone overflows (luminances of about 3.7e18 to 1.8e19 over a flat 25-tap window: m * m is still
// finite) v is +INF and the pixel is NOISY at every threshold for which thr * thr stays finite (at +INF, INF > INF is false).
// tests/test_adaptive_synthetic.py pins all three.
constexpr uint32_t kAdaptSparse = 1u, kAdaptNoisy = 2u;      // BRT_ADAPT_SPARSE, BRT_ADAPT_NOISY (include/bevyray_amd.h)
constexpr int kAdaptRadius = 2;
constexpr float kAdaptMeanFloor = 0.01f;
constexpr float kAdaptDefaultThreshold = 0.025f;      // brt_set_adaptive's default: the lowest R of the grid of DESIGN.md section 17

BRT_HD float adapt_luma(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
BRT_HD bool adapt_finite(float x) { return x - x == 0.0f; }      // false for +-INF and NaN

struct AdaptSums {
    uint32_t n;
    float s1, s2;
};
BRT_HD void adapt_tap(AdaptSums& a, bool inside, uint32_t id_p, uint32_t id_q, float l_q) {
    if (!inside || id_q != id_p || !adapt_finite(l_q)) return;
    a.n = a.n + 1u;
    a.s1 = a.s1 + l_q;
    a.s2 = a.s2 + l_q * l_q;
}
BRT_HD uint32_t adapt_class_of(const AdaptSums& a, float threshold, uint32_t min_taps) {
    if (a.n < min_taps) return kAdaptSparse;
    const float nf = (float)a.n;
    const float m = a.s1 / nf;
    const float d = a.s2 / nf - m * m;
    const float v = d > 0.0f ? d : 0.0f;
    const float thr = threshold * (m > kAdaptMeanFloor ? m : kAdaptMeanFloor);
    return v > thr * thr ? kAdaptNoisy : 0u;
}
// The class of p.  tap(dx, dy, &id_q, &l_q) -> whether the tap lies inside the frame (then with its material id and luminance).
template <class Tap>
BRT_HD uint32_t adapt_classify(float t_p, uint32_t id_p, float l_p, float threshold, uint32_t min_taps, Tap&& tap) {
    if (!(t_p < __builtin_inff()) || !adapt_finite(l_p)) return 0u;
    AdaptSums a = {0u, 0.0f, 0.0f};
    for (int dy = -kAdaptRadius; dy <= kAdaptRadius; dy++)
        for (int dx = -kAdaptRadius; dx <= kAdaptRadius; dx++) {
            uint32_t id_q = 0u;
            float l_q = 0.0f;
            const bool inside = tap(dx, dy, &id_q, &l_q);
            adapt_tap(a, inside, id_p, id_q, l_q);
        }
    return adapt_class_of(a, threshold, min_taps);
}

}  // namespace brt

// ---- the kernel's launcher ----------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace brt {

// One selection over the width x height base frame `base` (RGBA32F) with the full-size guide planes g0 {n, t} / g1 {a, id} of the same
// view.  mask == nullptr: every pixel's base value is stored at out[p] in out_format (BRT_FLAG_OUT_*; `out` overlaps neither `base` nor a
// guide plane) and a pixel with a class is appended to list (count: its count word, zeroed by the caller; the order is that of the waves'
// arrival).  mask != nullptr: the class byte of every pixel goes to mask, nothing else is written.  min_taps 0 with threshold +INF
// selects nothing.
struct AdaptiveSelect {
    uint32_t width, height;
    float threshold;
    uint32_t min_taps;
    const float4* base;
    const float4* g0;
    const float4* g1;
    void* out;
    uint32_t out_format;
    uint32_t* count;
    uint32_t* list;             // width * height words
    uint8_t* mask;
};
hipError_t launch_adaptive_select(const AdaptiveSelect& as, hipStream_t stream);

}  // namespace brt
#endif
