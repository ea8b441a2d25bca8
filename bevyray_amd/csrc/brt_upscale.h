// brt_upscale.h -- host-callable launcher of the guide-buffer upsampling (brt_upscale.hip).  The rule: DESIGN.md "Guide-buffer upsampling".
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "brt_denoise.h"
#include "brt_layout.h"

namespace brt {

// The three constants that only keep a stage's weight sum above zero: the floor of the bilinear weight, the floor of
// the edge-stopping weight, and the 1 of stage B's 1 / (1 + d^2).  The bilinear floor is 2^-26 so that a tap of bilinear weight 0 moves
// the result by less than an ulp when another one is eligible: at ratio 1 the upsampling is the identity to rounding.  The edge floor is
// 1 / 4: on spheres a few low pixels wide w_n = cos^128 alone leaves one tap, and the frame keeps the noise bilinear averaging removes
constexpr float kUpscaleBilinearFloor = 0x1p-26f;
constexpr float kUpscaleEdgeFloor = 0.25f;
// Every weight of a stage is scaled by a power of two that keeps the stage's weight sum below 1 (stage A: at most 1.25 (1 + 4 x 2^-26),
// stage B: at most 5.7 x 1.25 over its 16 taps, stage C: at most 1 + 4 x 2^-26), so that no sum of w c' over finite taps passes FLT_MAX:
// a tap of 3e38 on a refracting sphere (a = 1: c' is finite) at a stage A weight of 1.2 no longer stores +Inf.  The scaling is exact:
// the quotient sum / weight sum keeps its bits wherever no product is denormal.
constexpr float kUpscaleScaleA = 0.5f;
constexpr float kUpscaleScaleB = 0.125f;
constexpr float kUpscaleScaleC = 0.5f;

// The raster inputs of a frame of a level that blends (1 / 2; DESIGN.md "Upsampling blended frames"): RGBA32F colour and reverse-Z f32
// depth, both full.width x full.height on the device of the launch, either may be nullptr (zeros).
struct UpscaleBlend {
    const float4* raster_rgba;
    const float* raster_depth;
};

// Refined upsampling (DESIGN.md "Refined upsampling"): the classes of an output pixel whose guide is a hit -- BRT_REFINE_EDGES: no tap of
// its 2x2 footprint is eligible (stage A's weight sum is zero: the pixel would go to stage B or C); BRT_REFINE_SPECULAR: its sphere's
// material has metallic > 0 or specular_transmission > 0.  mask == nullptr: a pixel in one of `classes` is SELECTED -- its index is
// appended to list (count: its count word, zeroed by the caller; the order is that of the waves' arrival) and nothing is stored for
// it; any other pixel is the plain kernel's.  mask != nullptr: the class bits of every output pixel (0 for the sky) go to mask, nothing
// else is written.
struct UpscaleSelect {
    uint32_t classes;
    uint32_t* count;            // the list's count word
    uint32_t* list;             // full.width * full.height words
    uint8_t* mask;
};

// full: the frame parameters of the width x height output (its pixel-centre rays are cast by the kernel itself); low: those of the traced
// frame; ds_low: the scratch whose g0 / g1 hold the guides of the low frame (launch_denoise_guides with `low`); d_low: the low frame,
// RGBA32F low.width x low.height; d_out: full.width x full.height in out_format (BRT_FLAG_OUT_*), not overlapping d_low.  The sigmas of
// the edge-stopping weights are st's (brt_set_denoise).  blend != nullptr: `full` is made for level 1 or 2 (its near_, far_ and
// fallback_far decide the blend) and a covered output pixel is its raster texel; d_out overlaps neither raster buffer.  select != nullptr
// (level 3 only, blend == nullptr): see UpscaleSelect; with a mask d_out is not written and may be nullptr.
hipError_t launch_upscale(const DeviceSceneView& sv, const FrameParams& full, const FrameParams& low, const DenoiseSettings& st,
                          const DenoiseScratch& ds_low, const float* d_low, void* d_out, uint32_t out_format, hipStream_t stream,
                          const UpscaleBlend* blend = nullptr, const UpscaleSelect* select = nullptr);

}  // namespace brt
