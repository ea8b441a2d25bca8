// brt_query.hip -- batched ray queries against the resident scene (brt_query_rays*, DESIGN.md "Ray queries").  Every ray is walked by
// the walk of the trace kernels as it stands (walk_begin / walk_run / raycast, brt_device.h): per ray the same steps in the same order
// as the reference's raycast (raytrace.wgsl:313-362), whichever form runs it.
//
// k_query_plain<D16>                one thread per ray, the scene in global memory, a private stack: what k_denoise_guides does per pixel.
//                                   Every scene representation and tree.  ANY mode leaves the walk at the first step after which
//                                   closest < t_max.
// k_query_stream<MODE, D16, SIMPLE> persistent workgroups: the scene (SCENE_LDS) or the top of the tree (SCENE_LDS_TOP) staged in LDS as
//                                   k_trace_persistent stages it, the stacks in LDS, so the hand-written walk loops serve it.  A wave takes
//                                   rays from the batch counter for the lanes whose walk has ended and walks on next to the lanes that
//                                   are still under way (walk_run's early exit and WalkState), instead of waiting for its longest walk.
//                                   ANY mode ends a lane's walk at the first return of walk_run at which closest < t_max.
// Both forms write the same bytes: a lane's result depends on its own ray alone.  No atomics touch a result.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "brt_device.h"
#include "brt_kernels.h"
#include "brt_query.h"

namespace brt {

namespace {

constexpr float kPosInf = __builtin_inff();

struct QueryRay {
    f3 o, d;
    float t_max;
    uint32_t user;
};

BRT_DEV uint32_t q_lane() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
BRT_DEV uint32_t q_rank(uint64_t mask) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u)); }

BRT_DEV QueryRay query_load(const QueryArgs& qa, uint32_t i) {
    const float4 r0 = qa.rays[2 * (size_t)i], r1 = qa.rays[2 * (size_t)i + 1];
    QueryRay r;
    r.o = mk3(r0.x, r0.y, r0.z);
    r.t_max = r0.w;
    r.d = mk3(r1.x, r1.y, r1.z);
    r.user = __float_as_uint(r1.w);
    return r;
}

// 0: the ray is walked; else the refusal
BRT_DEV uint32_t query_refusal(const QueryRay& r, float bound) {
    const bool finite = __builtin_isfinite(r.o.x) && __builtin_isfinite(r.o.y) && __builtin_isfinite(r.o.z) && __builtin_isfinite(r.d.x) &&
                        __builtin_isfinite(r.d.y) && __builtin_isfinite(r.d.z);
    if (!finite || !(r.t_max > 0.0f)) return BRT_QUERY_STATUS_INVALID;           // (a NaN t_max fails the comparison)
    const float l1 = (__builtin_fabsf(r.o.x) + __builtin_fabsf(r.o.y)) + __builtin_fabsf(r.o.z);
    return l1 > bound ? (uint32_t)BRT_QUERY_STATUS_OUT_OF_REACH : 0u;
}

BRT_DEV void query_store_miss(const QueryArgs& qa, uint32_t i, uint32_t status, uint32_t user) {
    qa.hits[2 * (size_t)i] = make_float4(kPosInf, 0.0f, 0.0f, 0.0f);
    qa.hits[2 * (size_t)i + 1] = make_float4(__uint_as_float(BRT_QUERY_NONE), __uint_as_float(BRT_QUERY_NONE), __uint_as_float(status), __uint_as_float(user));
}

// the record of a walk that has ended with (t, idx) (t == kInf: nothing accepted); returns whether it is a hit.  spheres: the resident
// spheres (global memory or their LDS copy: the same values)
BRT_DEV bool query_store(const QueryArgs& qa, const DeviceSceneView& sv, const float4* spheres, uint32_t i, const QueryRay& r, float t,
                         uint32_t idx) {
    const bool hit = t != kInf && t < r.t_max;
    if (!hit || qa.mode == BRT_QUERY_ANY) {
        query_store_miss(qa, i, hit ? BRT_QUERY_STATUS_HIT : BRT_QUERY_STATUS_MISS, r.user);
        return hit;
    }
    const float4 s = spheres[idx];
    const f3 pos = mk3(r.o.x + t * r.d.x, r.o.y + t * r.d.y, r.o.z + t * r.d.z);      // ray_at (raytrace.wgsl:130-132)
    const f3 n = normalize3(mk3(pos.x - s.x, pos.y - s.y, pos.z - s.z));              // :356
    const bool front = dot3(r.d, n) < 0.0f;                                            // :358
    qa.hits[2 * (size_t)i] = make_float4(t, n.x, n.y, n.z);
    qa.hits[2 * (size_t)i + 1] = make_float4(__uint_as_float(qa.rmap ? qa.rmap[idx] : idx), __uint_as_float(sv.sphere_material[idx]),
                                             __uint_as_float(BRT_QUERY_STATUS_HIT | (front ? BRT_QUERY_STATUS_FRONT_FACE : 0u)),
                                             __uint_as_float(r.user));
    return hit;
}

BRT_DEV uint32_t q_wave_sum(uint32_t v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += (uint32_t)__shfl_xor((int)v, s, 64);
    return v;
}

// the wave's counts into qa.stat (all lanes of the wave call it)
BRT_DEV void query_count(const QueryArgs& qa, uint32_t walked, uint32_t hits, uint32_t refused) {
    if (!qa.stat) return;
    walked = q_wave_sum(walked);
    hits = q_wave_sum(hits);
    refused = q_wave_sum(refused);
    if (q_lane() == 0u) {
        if (walked) atomicAdd(qa.stat + 0, walked);
        if (hits) atomicAdd(qa.stat + 1, hits);
        if (refused) atomicAdd(qa.stat + 2, refused);
    }
}

BRT_DEV ScenePtrs query_scene_global(const DeviceSceneView& sv) {      // the scene in global memory, as k_trace_simple walks it
    ScenePtrs sc = {};
    sc.pairs = reinterpret_cast<const char*>(sv.pairs);
    sc.pairs_far = sc.pairs;
    sc.boxes_ordered = sv.boxes_ordered != 0u;
    sc.spheres = reinterpret_cast<const float4*>(sv.spheres);
    sc.sphere_material = sv.sphere_material;
    sc.materials = reinterpret_cast<const float4*>(sv.materials);
    sc.sphere_mats = reinterpret_cast<const float4*>(sv.sphere_mats);
    sc.leaf_table = reinterpret_cast<const uint2*>(sv.leaf_table);
    return sc;
}

}  // namespace

// ---- plain form ----------------------------------------------------------------------------------------------------------------------

template <bool D16>
__global__ __launch_bounds__(256) void k_query_plain(DeviceSceneView sv, QueryArgs qa) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t walked = 0u, hits = 0u, refused = 0u;
    if (i < qa.n_rays) {
        const QueryRay r = query_load(qa, i);
        const uint32_t refusal = query_refusal(r, qa.bound);
        if (refusal != 0u) {
            query_store_miss(qa, i, refusal, r.user);
            refused = 1u;
        } else {
            const ScenePtrs sc = query_scene_global(sv);
            uint32_t stack[34];   // DONE sentinel + 32 entries + one spare
            HitCounters hc = {};
            float t;
            uint32_t idx;
            if (qa.mode == BRT_QUERY_ANY) {
                // walk_run's per-lane loop with one more way out: the walk is the same walk up to the step at which it is left
                using DS = Desc<D16>;
                WalkState<uint32_t> w;
                walk_begin<D16>(w, sc, sv.root_desc, stack, r.d);
                uint32_t* sp = w.sp;
                const bool unsafe = !sc.boxes_ordered || !ray_is_safe(r.o, w.inv);
                const float lim = min_f(r.t_max, kInf);      // (closest starts at kInf, the reference's "no hit", which is below a t_max of +INF)
                while (w.cur != DS::DONE && w.n < 31u && !(w.closest < lim)) {
                    if (DS::is_leaf(w.cur))
                        walk_leaf_step<1, false, D16, false>(sc, r.o, r.d, w.a, w.closest, w.closest_idx, w.cur, sp, w.n, hc);
                    else if (unsafe)
                        walk_interior_step<1, false, true, D16, SCENE_GLOBAL>(sc, r.o, w.inv, w.ox, w.oy, w.oz, float_below(w.closest), w.cur, sp, w.n, hc);
                    else
                        walk_interior_step<1, false, false, D16, SCENE_GLOBAL>(sc, r.o, w.inv, w.ox, w.oy, w.oz, float_below(w.closest), w.cur, sp, w.n, hc);
                }
                t = w.closest;
                idx = w.closest_idx;
            } else {
                raycast<1, false, D16, false>(sc, sv.root_desc, stack, r.o, r.d, t, idx, hc);
            }
            walked = 1u;
            hits = query_store(qa, sv, sc.spheres, i, r, t, idx) ? 1u : 0u;
        }
    }
    query_count(qa, walked, hits, refused);
}

// ---- streaming form ------------------------------------------------------------------------------------------------------------------

template <int MODE, bool D16, bool SIMPLE>
__global__ __launch_bounds__(BRT_BLOCK) void k_query_stream(DeviceSceneView sv, QueryArgs qa) {
    static_assert(MODE == SCENE_GLOBAL || D16, "a scene staged in LDS always uses 16-bit descriptors");
    using StackT = typename std::conditional<D16, int16_t, int32_t>::type;   // sign-extending loads: brt_layout.h
    using DS = Desc<D16>;
    extern __shared__ uint4 smem[];
    // the carve of k_trace_persistent (brt_trace.h): the hand-written loops address the pair records from LDS address 0
    ScenePtrs sc = query_scene_global(sv);
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
    const uint32_t lane = q_lane();
    const uint32_t wave = threadIdx.x >> 6;
    // this lane's column of the wave's [entry][64] stack array (16-bit entries: lanes l and l + 32 share a dword, brt_trace.h)
    const uint32_t stack_col = D16 ? ((lane & 31u) * 2u + (lane >> 5)) : lane;
    StackT* stk = stacks + wave * ((sv.stack_entries + 2u) * 64u) + stack_col;

    WalkState<StackT> walk;
    walk.a = 0.0f; walk.inv = mk3(0.0f, 0.0f, 0.0f); walk.closest = kInf; walk.closest_idx = 0xffffffffu;
    walk.cur = DS::DONE; walk.sp = stk; walk.n = 0;
    walk.ox = walk.oy = walk.oz = 0u;
    QueryRay r;
    r.o = mk3(0.0f, 0.0f, 0.0f); r.d = mk3(0.0f, 0.0f, 1.0f); r.t_max = kPosInf; r.user = 0u;
    uint32_t ray_i = 0u;
    bool in_flight = false;          // this lane holds a ray whose walk has not ended
    bool exhausted = false;          // wave-uniform: the batch counter has passed the last ray
    uint32_t walked = 0u, hits = 0u, refused = 0u;
    HitCounters hc = {};
    for (;;) {
        if (!exhausted) {
            // rays for the idle lanes: one fetch-add of the wave
            const uint64_t idle = __ballot(!in_flight);
            const uint32_t cnt = (uint32_t)__popcll(idle);
            uint32_t base = 0u;
            if (lane == 0u) base = atomicAdd(qa.counter, cnt);
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            exhausted = base >= qa.n_rays || qa.n_rays - base <= cnt;
            const uint32_t mine = base + q_rank(idle);
            if (!in_flight && base < qa.n_rays && mine < qa.n_rays) {
                r = query_load(qa, mine);
                ray_i = mine;
                const uint32_t refusal = query_refusal(r, qa.bound);
                if (refusal != 0u) {
                    query_store_miss(qa, mine, refusal, r.user);
                    refused++;
                } else {
                    walk_begin<D16>(walk, sc, sv.root_desc, stk, r.d);
                    in_flight = true;
                    walked++;
                }
            }
        }
        walk_run<64, false, D16, SIMPLE, MODE, StackT>(sc, walk, stk, r.o, r.d, kQueryExitLanes, kLeafVote, hc);
        if (in_flight) {
            const bool ended = !walk_pending<D16, SIMPLE>(walk) || (qa.mode == BRT_QUERY_ANY && walk.closest < min_f(r.t_max, kInf));
            if (ended) {
                hits += query_store(qa, sv, sc.spheres, ray_i, r, walk.closest, walk.closest_idx) ? 1u : 0u;
                walk.cur = DS::DONE;
                in_flight = false;
            }
        }
        if (exhausted && __ballot(in_flight) == 0ull) break;
    }
    query_count(qa, walked, hits, refused);
}

// ---- host-callable launcher ----------------------------------------------------------------------------------------------------------

template <int MODE, bool D, bool S>
static hipError_t launch_stream_t(const QueryLaunch& ql) {
    auto kern = k_query_stream<MODE, D, S>;
    if (MODE == SCENE_LDS || MODE == SCENE_LDS_TOP) {
        // the hand-written walk loops address the pair records from LDS address 0: the dynamic LDS must start there
        static const size_t static_lds = [&] {
            hipFuncAttributes at{};
            return hipFuncGetAttributes(&at, reinterpret_cast<const void*>(kern)) == hipSuccess ? at.sharedSizeBytes : (size_t)1;
        }();
        if (static_lds != 0) return hipErrorInvalidConfiguration;
    }
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ql.lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(ql.grid), dim3(ql.block), ql.lds_bytes, ql.stream, ql.scene, ql.args);
    return hipGetLastError();
}

template <int MODE, bool D>
static hipError_t launch_stream_md(const QueryLaunch& ql) {
    return ql.scene.simple_tree ? launch_stream_t<MODE, D, true>(ql) : launch_stream_t<MODE, D, false>(ql);
}

hipError_t launch_query(const QueryLaunch& ql) {
    if (ql.args.n_rays == 0u) return hipSuccess;
    if (ql.form == QUERY_PLAIN) {
        const dim3 grid((ql.args.n_rays + 255u) / 256u);
        if (ql.scene.desc16) hipLaunchKernelGGL(k_query_plain<true>, grid, dim3(256), 0, ql.stream, ql.scene, ql.args);
        else hipLaunchKernelGGL(k_query_plain<false>, grid, dim3(256), 0, ql.stream, ql.scene, ql.args);
        return hipGetLastError();
    }
    if (ql.grid == 0u || ql.block == 0u || (ql.block & 63u) != 0u || ql.block > BRT_BLOCK || !ql.args.counter) return hipErrorInvalidValue;
    switch (ql.scene_mode) {
        case SCENE_LDS:
            if (!ql.scene.desc16) return hipErrorInvalidValue;
            return launch_stream_md<SCENE_LDS, true>(ql);
        case SCENE_LDS_TOP:
            if (!ql.scene.desc16) return hipErrorInvalidValue;
            return launch_stream_md<SCENE_LDS_TOP, true>(ql);
        default:
            return ql.scene.desc16 ? launch_stream_md<SCENE_GLOBAL, true>(ql) : launch_stream_md<SCENE_GLOBAL, false>(ql);
    }
}

}  // namespace brt
