// brt_query.h -- host-callable launcher of the batched ray queries (brt_query.hip).  The rules: DESIGN.md "Ray queries".
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "brt_kernels.h"

namespace brt {

// One batch.  rays / hits: two float4 per record (include/bevyray_amd.h "ray queries").
struct QueryArgs {
    const float4* rays;
    float4* hits;
    uint32_t n_rays, mode;      // BRT_QUERY_CLOSEST / BRT_QUERY_ANY
    float bound;                // a ray whose (|o.x| + |o.y|) + |o.z| exceeds it is refused (+INF: none is)
    const uint32_t* rmap;       // resident sphere index -> the caller's (nullptr: the identity)
    uint32_t* stat;             // [0] rays walked, [1] hits, [2] refused, zeroed by the caller (nullptr: not counted)
    uint32_t* counter;          // streaming form: the batch counter, zeroed by the caller
};

// walk_run's exit_lanes of the streaming form: a wave comes back for new rays once no more than min(this, half of the lanes that
// entered) still walk
constexpr uint32_t kQueryExitLanes = 32;

struct QueryLaunch : StreamLaunch {
    QueryArgs args;
};
hipError_t launch_query(const QueryLaunch& ql);

}  // namespace brt
