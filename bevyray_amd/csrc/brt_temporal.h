// brt_temporal.h -- host-callable launcher of the temporal reprojection and accumulation (brt_temporal.hip).  The formulas: DESIGN.md
// section 11 "Temporal accumulation"; tests/temporal_ref.py restates them in numpy.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "brt_denoise.h"
#include "brt_layout.h"

namespace brt {

// From this history length on, the variance of the accumulated colour is taken from the moments (var = (m2 - m1^2) / n) instead of the
// 7x7 neighbourhood, and sigma_l is no longer scaled by the sample count
constexpr float kTemporalConverged = 4.0f;

// The history of one width x height frame, carved out of one allocation (temporal_history_bytes): 108 bytes per pixel.
//   a[2]  float4 {normal.xyz, t}                           the guide of the frame that wrote the set (t = +INF: sky)
//   b[2]  float4 {h.rgb, n}                                the accumulated demodulated colour and its history length (0: none)
//   c[2]  float4 {m1, m2, sphere id bits, material id bits}  the moments of the luminance of c'; the caller's sphere index
//   xy    float2 {x', y'}                                  the reprojected position of the last temporal frame (NaN: rejected)
//   sid   u32                                              this frame's caller sphere index (the guide kernel's output)
// The sets a/b/c ping-pong: a frame reads set `prev` at four bilinear taps and writes set prev ^ 1.
struct TemporalHistory {
    float4* a[2];
    float4* b[2];
    float4* c[2];
    float2* xy;
    uint32_t* sid;
};
size_t temporal_history_bytes(uint32_t width, uint32_t height);
TemporalHistory temporal_history(char* base, uint32_t width, uint32_t height);

// The previous temporal frame's camera, inverted: X_prev - o = z (D + s_x R + s_y U) solved as [z, z s_x, z s_y] = inv . (X_prev - o)
struct TemporalCamera {
    float o[3];
    float inv[3][3];          // rows (R x U, U x D, D x R) / det, det = D . (R x U)
};
TemporalCamera temporal_camera(const FrameParams& prev);

struct TemporalArgs {
    uint32_t prev;            // the set the previous temporal frame wrote
    uint32_t has_history;     // 0: the history is empty (n = 0 everywhere)
    uint32_t same_camera;     // the camera is bitwise the previous one's
    uint32_t motion;          // the sphere count is that of the snapshot: the object-motion term applies
    float max_history;        // 1 .. 65535
    const float4* sph_new;    // the spheres {centre, r^2} in the caller's order: now ...
    const float4* sph_old;    // ... and as the previous temporal frame saw them
};

// After the guides (with hist.sid) and the demodulation: reprojects, validates and accumulates every pixel into set args.prev ^ 1.
// d_out == nullptr: ds.dm becomes {h.rgb, n} for the filter (BRT_FLAG_TEMPORAL | BRT_FLAG_DENOISE); else the accumulated frame h a
// (the input itself where n = 1 or the pixel passes through: the demodulation's copy in ds.cv[0]) is stored into d_out in out_format
// (d_out may be the input frame, or ds.cv[0] itself).  bp.on (the guides came from the coverage frame): a covered pixel's store is its
// raster texel.
hipError_t launch_temporal(const FrameParams& fp, const FrameParams& prev, const TemporalArgs& args, const DenoiseScratch& ds,
                           const TemporalHistory& hist, void* d_out, uint32_t out_format, hipStream_t stream,
                           const BlendPost& bp = BlendPost());

}  // namespace brt
