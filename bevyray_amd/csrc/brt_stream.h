// brt_stream.h -- what the streaming list kernels share (k_query_stream, k_radiance_stream, and k_list_stream of the pixel lists): the
// scene in global memory or staged in LDS, a lane's stack and idle walk, and the launch of the streaming form.  Included by
// brt_query.hip, brt_radiance.hip and (through brt_pixels_dev.h) brt_pixels.hip and brt_lens.hip only.  The counter claim of a round
// stays written out in each kernel: as a function it changes their instructions.
#pragma once
#include "brt_trace.h"

namespace brt {

BRT_DEV ScenePtrs scene_global(const DeviceSceneView& sv) {      // the scene in global memory, as k_trace_simple walks it
    ScenePtrs sc = {};
    sc.pairs = reinterpret_cast<const char*>(sv.pairs);
    sc.pairs_far = sc.pairs;
    sc.boxes_ordered = sv.boxes_ordered != 0u;
    sc.spheres_bounded = sv.spheres_bounded != 0u;
    sc.spheres = reinterpret_cast<const float4*>(sv.spheres);
    sc.sphere_material = sv.sphere_material;
    sc.materials = reinterpret_cast<const float4*>(sv.materials);
    sc.sphere_mats = reinterpret_cast<const float4*>(sv.sphere_mats);
    sc.leaf_table = reinterpret_cast<const uint2*>(sv.leaf_table);
    return sc;
}

// The workgroup's dynamic LDS array `smem`, carved as k_trace_persistent carves it (brt_trace.h) without drain pool and row scratch:
// the hand-written loops address the pair records from LDS address 0, so they come first (every carve offset is a multiple of 16),
// then spheres, leaf table and the stacks.  Stages what MODE stages, points sc (scene_global) at it and returns the stacks.  All
// threads of the workgroup call it: it ends in the barrier behind the copies.
template <int MODE, typename StackT>
BRT_DEV StackT* stream_stage(const DeviceSceneView& sv, uint4* smem, ScenePtrs& sc) {
    StackT* stacks;
    if (MODE == SCENE_LDS) {
        const uint32_t pair_granules = (uint32_t)(pair_array_bytes(sv.n_pairs) / 16);
        float4* p = reinterpret_cast<float4*>(smem);
        float4* l_pairs = p; p += pair_granules;
        float4* l_sp = p; p += sv.n_models;
        uint2* l_lt = reinterpret_cast<uint2*>(p);
        stacks = reinterpret_cast<StackT*>(l_lt + sv.n_leaf_table);
        const float4* g_pairs = reinterpret_cast<const float4*>(sv.pairs);
        const float4* g_sp = reinterpret_cast<const float4*>(sv.spheres);
        const uint2* g_lt = reinterpret_cast<const uint2*>(sv.leaf_table);
        for (uint32_t i = threadIdx.x; i < pair_granules; i += blockDim.x) l_pairs[i] = g_pairs[i];
        for (uint32_t i = threadIdx.x; i < sv.n_models; i += blockDim.x) l_sp[i] = g_sp[i];
        for (uint32_t i = threadIdx.x; i < sv.n_leaf_table; i += blockDim.x) l_lt[i] = g_lt[i];
        sc.pairs = reinterpret_cast<const char*>(l_pairs);
        sc.near_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)reinterpret_cast<char*>(l_pairs);
        sc.sph_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)reinterpret_cast<char*>(l_sp);
        sc.spheres = l_sp;
        sc.leaf_table = l_lt;
    } else if (MODE == SCENE_LDS_TOP) {
        const uint32_t pair_granules = sv.lds_pairs * PAIR_UNITS;
        float4* l_pairs = reinterpret_cast<float4*>(smem);
        const float4* g_pairs = reinterpret_cast<const float4*>(sv.pairs);
        for (uint32_t i = threadIdx.x; i < pair_granules; i += blockDim.x) l_pairs[i] = g_pairs[i];
        sc.pairs = reinterpret_cast<const char*>(l_pairs);
        sc.near_bytes = sv.lds_pairs * PAIR_BYTES;
        sc.near_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)reinterpret_cast<char*>(l_pairs);
        stacks = reinterpret_cast<StackT*>(l_pairs + pair_granules);
    } else {
        stacks = reinterpret_cast<StackT*>(smem);
    }
    __syncthreads();
    return stacks;
}

// lane `lane`'s column of its wave's [entry][64] stack array (16-bit entries: lanes l and l + 32 share a dword, brt_trace.h)
template <bool D16, typename StackT>
BRT_DEV StackT* stream_stack(const DeviceSceneView& sv, StackT* stacks, uint32_t lane) {
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t stack_col = D16 ? ((lane & 31u) * 2u + (lane >> 5)) : lane;
    return stacks + wave * ((sv.stack_entries + 2u) * 64u) + stack_col;
}

// the walk of a lane that holds nothing: walk_run passes over it
template <bool D16, typename StackT>
BRT_DEV WalkState<StackT> walk_idle(StackT* stk) {
    WalkState<StackT> walk;
    walk.a = 0.0f; walk.inv = mk3(0.0f, 0.0f, 0.0f); walk.closest = kInf; walk.closest_idx = 0xffffffffu;
    walk.cur = Desc<D16>::DONE; walk.sp = stk; walk.n = 0;
    walk.ox = walk.oy = walk.oz = 0u;
    return walk;
}

// ---- the launch of the streaming form ------------------------------------------------------------------------------------------------
// Family: a struct whose kernel<MODE, D16, SIMPLE>() is the family's kernel template; args: what the kernel takes behind the scene.

template <class Family, int MODE, bool D, bool S, class... Args>
static hipError_t launch_stream_t(const StreamLaunch& sl, const Args&... args) {
    auto kern = Family::template kernel<MODE, D, S>();
    if (MODE == SCENE_LDS || MODE == SCENE_LDS_TOP) {
        // the hand-written walk loops address the pair records from LDS address 0: the dynamic LDS must start there
        static const size_t static_lds = [&] {
            hipFuncAttributes at{};
            return hipFuncGetAttributes(&at, reinterpret_cast<const void*>(kern)) == hipSuccess ? at.sharedSizeBytes : (size_t)1;
        }();
        if (static_lds != 0) return hipErrorInvalidConfiguration;
    }
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sl.lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(sl.grid), dim3(sl.block), sl.lds_bytes, sl.stream, sl.scene, args...);
    return hipGetLastError();
}

template <class Family, int MODE, bool D, class... Args>
static hipError_t launch_stream_md(const StreamLaunch& sl, const Args&... args) {
    return sl.scene.simple_tree ? launch_stream_t<Family, MODE, D, true>(sl, args...) : launch_stream_t<Family, MODE, D, false>(sl, args...);
}

// counter: the batch counter among args
template <class Family, class... Args>
static hipError_t launch_stream(const StreamLaunch& sl, const uint32_t* counter, const Args&... args) {
    if (sl.grid == 0u || sl.block == 0u || (sl.block & 63u) != 0u || sl.block > BRT_BLOCK || !counter) return hipErrorInvalidValue;
    switch (sl.scene_mode) {
        case SCENE_LDS:
            if (!sl.scene.desc16) return hipErrorInvalidValue;
            return launch_stream_md<Family, SCENE_LDS, true>(sl, args...);
        case SCENE_LDS_TOP:
            if (!sl.scene.desc16) return hipErrorInvalidValue;
            return launch_stream_md<Family, SCENE_LDS_TOP, true>(sl, args...);
        default:
            return sl.scene.desc16 ? launch_stream_md<Family, SCENE_GLOBAL, true>(sl, args...) : launch_stream_md<Family, SCENE_GLOBAL, false>(sl, args...);
    }
}

}  // namespace brt
