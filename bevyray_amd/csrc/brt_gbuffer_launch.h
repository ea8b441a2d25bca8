// brt_gbuffer_launch.h -- host-callable launcher of the G-buffer kernel (brt_gbuffer.hip).  The rule: brt_gbuffer.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "brt_gbuffer.h"
#include "brt_layout.h"

namespace brt {

// One frame.  Every plane may be null (not produced); all of them DEVICE memory of width * height entries.
struct GbufferArgs {
    GbufferView gv;
    uint32_t depth_mode, normal_format, motion_format;      // BRT_GBUFFER_DEPTH_*; 0: RGBA32F, 1: RGB10A2; 0: RG32F uv, 1: RG16F uv, 2: RG32F (x', y')
    const uint32_t* rmap;           // resident sphere index -> the caller's (nullptr: the identity)
    const float4* prev_models;      // the previous frame's 32-byte models in the caller's order (nullptr: nothing moved)
    const float4* cov;              // a coverage frame (RGBA32F): alpha +0.0 casts no ray and writes nothing (nullptr: none)
    float* depth;
    void* normal;
    void* motion;
    uint4* ids;                     // {sphere (caller's index), material, status, 0}
    float4* albedo;
    uint32_t* stat;                 // [0] pixels cast, [1] hits, [2] covered, [3] moved, [4] no-previous, zeroed by the caller (nullptr: not counted)
};

hipError_t launch_gbuffer(const DeviceSceneView& scene, const FrameParams& fp, const GbufferArgs& args, hipStream_t stream);

}  // namespace brt
