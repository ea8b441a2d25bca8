// brt_wave.h -- what the lanes of one wave (64) do together: a lane's number, its rank in a mask, a sum over the wave, and the append of
// the selecting kernels (k_upscale, k_adaptive_select, k_prog_select).  Device code without the tracer: brt_trace.h includes it, and so
// may a kernel that never casts a ray.
#pragma once
#include <hip/hip_runtime.h>

#include "brt_device.h"

namespace brt {

BRT_DEV uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
BRT_DEV uint32_t mbcnt64(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

BRT_DEV uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// The lanes of the wave that are here and have `sel` set append p to the list: one ballot, one atomicAdd of the wave on the count word
// (none in a wave without a selected lane), plain vector stores.  Every lane of the wave that is here calls it.
BRT_DEV void wave_append(uint32_t* count, uint32_t* list, bool sel, uint32_t p) {
    const uint64_t m = __ballot(sel);
    if (m == 0ull) return;
    const uint32_t lane = lane_id();
    const uint32_t leader = (uint32_t)__builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
    uint32_t first = 0u;
    if (lane == leader) first = atomicAdd(count, (uint32_t)__popcll(m));
    first = (uint32_t)__builtin_amdgcn_readlane((int)first, (int)leader);
    if (sel) list[first + mbcnt64(m)] = p;
}

}  // namespace brt
