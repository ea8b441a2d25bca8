// brt_radiance.h -- host-callable launcher of the radiance queries (brt_radiance.hip).  The rules: DESIGN.md "Radiance queries".
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "brt_layout.h"

namespace brt {

// One list.  rays / out: two float4 per record (include/bevyray_amd.h "radiance queries"): {origin.xyz, seed | direction.xyz, user} in,
// {t, r, g, b | sphere, material, status, user} out.
struct RadianceArgs {
    const float4* rays;
    float4* out;
    uint32_t n_rays;
    uint32_t samples, bounces;  // paths per entry (>= 1) and camera.bounce_count of raytrace.wgsl:189
    float bound;                // an entry whose (|o.x| + |o.y|) + |o.z| exceeds it is refused (+INF: none is)
    const uint32_t* rmap;       // resident sphere index -> the caller's (nullptr: the identity)
    unsigned long long* stat;   // [0] walks performed, [1] entries whose own ray hit, [2] entries refused, zeroed by the caller (nullptr: not counted)
    uint32_t* counter;          // streaming form: the batch counter, zeroed by the caller
};

enum RadianceForm : int { RADIANCE_PLAIN = 0, RADIANCE_STREAM = 1 };

struct RadianceLaunch {
    DeviceSceneView scene;      // (lds_pairs set for SCENE_LDS_TOP)
    RadianceArgs args;
    int form;                   // RadianceForm
    int scene_mode;             // streaming form: SceneMode
    uint32_t grid, block;       // streaming form
    size_t lds_bytes;           // streaming form: trace_lds_bytes(scene, scene_mode, block, 0)
    hipStream_t stream;
};
hipError_t launch_radiance(const RadianceLaunch& rl);

}  // namespace brt
