// brt_query.hip -- batched ray queries against the resident scene (brt_query_rays*, DESIGN.md "Ray queries").  Every ray is walked by
// the walk of the trace kernels as it stands (walk_begin / walk_run / raycast, brt_device.h): per ray the same steps in the same order
// as the reference's raycast (raytrace.wgsl:313-362), whichever form runs it.
//
// k_query_plain<D16>                one thread per ray, the scene in global memory, a private stack: what k_denoise_guides does per pixel.
//                                   Every scene representation and tree.  ANY mode leaves the walk at the first step after which
//                                   closest < t_max.
// k_query_stream<MODE, D16, SIMPLE> persistent workgroups: the scene (SCENE_LDS) or the top of the tree (SCENE_LDS_TOP) staged in LDS
//                                   (stream_stage, brt_stream.h), the stacks in LDS, so the hand-written walk loops serve it.  A wave takes
//                                   rays from the batch counter for the lanes whose walk has ended and walks on next to the lanes that
//                                   are still under way (walk_run's early exit and WalkState), instead of waiting for its longest walk.
//                                   ANY mode ends a lane's walk at the first return of walk_run at which closest < t_max.
// Both forms write the same bytes: a lane's result depends on its own ray alone.  No atomics touch a result.
// What the streaming form shares with k_radiance_stream and k_list_stream (brt_pixels_dev.h), its launch included: brt_stream.h.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "brt_query.h"
#include "brt_stream.h"

namespace brt {

namespace {

constexpr float kPosInf = __builtin_inff();

struct QueryRay {
    f3 o, d;
    float t_max;
    uint32_t user;
};

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

// (wave_sum of brt_trace.h sums downwards: lane 0 would hold the same value, from other instructions)
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
    if (lane_id() == 0u) {
        if (walked) atomicAdd(qa.stat + 0, walked);
        if (hits) atomicAdd(qa.stat + 1, hits);
        if (refused) atomicAdd(qa.stat + 2, refused);
    }
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
            const ScenePtrs sc = scene_global(sv);
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
    ScenePtrs sc = scene_global(sv);
    StackT* stacks = stream_stage<MODE, StackT>(sv, smem, sc);
    const uint32_t lane = lane_id();
    StackT* stk = stream_stack<D16>(sv, stacks, lane);

    WalkState<StackT> walk = walk_idle<D16>(stk);
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
            const uint32_t mine = base + mbcnt64(idle);
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

struct QueryStream {
    template <int MODE, bool D16, bool SIMPLE>
    static auto kernel() { return k_query_stream<MODE, D16, SIMPLE>; }
};

hipError_t launch_query(const QueryLaunch& ql) {
    if (ql.args.n_rays == 0u) return hipSuccess;
    if (ql.form == LIST_PLAIN) {
        const dim3 grid((ql.args.n_rays + 255u) / 256u);
        if (ql.scene.desc16) hipLaunchKernelGGL(k_query_plain<true>, grid, dim3(256), 0, ql.stream, ql.scene, ql.args);
        else hipLaunchKernelGGL(k_query_plain<false>, grid, dim3(256), 0, ql.stream, ql.scene, ql.args);
        return hipGetLastError();
    }
    return launch_stream<QueryStream>(ql, ql.args.counter, ql.args);
}

}  // namespace brt
