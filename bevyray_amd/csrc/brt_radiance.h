// brt_radiance.h -- host-callable launcher of the radiance queries (brt_radiance.hip).  The rules: DESIGN.md "Radiance queries".
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "brt_kernels.h"

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

struct RadianceLaunch : StreamLaunch {
    RadianceArgs args;
};
hipError_t launch_radiance(const RadianceLaunch& rl);

}  // namespace brt
