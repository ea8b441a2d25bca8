// brt_radiance.hip -- radiance queries (brt_radiance_rays*; DESIGN.md "Radiance queries"): path-traced colour for a list of the
// caller's rays.  An entry {o, seed, d, user} is trace_multisampled (raytrace.wgsl:159-172) with the caller's ray in place of
// random_ray_from_uv: rng_state = seed, `samples` times raytrace(Ray(o, d)) (:174-224) at level 3 with camera.bounce_count = bounces,
// summed and divided by f32(samples).  Per entry the draws and operations are those of the trace kernels (walk / shade_segment /
// scatter, brt_device.h, brt_trace.h), whichever form runs it; the first-hit fields are those of a CLOSEST ray query of {o, +INF, d}.
//
// The entry's own ray is walked ONCE.  Every sample starts on the same (o, d), and the walk draws no random number, so its (t, idx) is
// the same for every sample: it is kept (o0, d0, t0, idx0) and every sample after the first begins with shade_segment on it.  A sample
// that ends on that segment (sky, absorbed, bounces = 0) goes on to the next sample at once.
//
// k_radiance_plain<D16>                one thread per entry, the scene in global memory, a private 34-entry stack: the thread's column
//                                      of a [34][256] LDS array (no scratch).  Every scene representation and tree.
// k_radiance_stream<MODE, D16, SIMPLE> persistent workgroups: the scene (SCENE_LDS) or the top of the tree (SCENE_LDS_TOP) staged in LDS
//                                      (stream_stage, brt_stream.h), the stacks in LDS, so the hand-written walk
//                                      loops serve it.  A lane carries one path.  A round: the wave takes entries from the batch counter
//                                      (one fetch-add) for the lanes whose entry has ended, walk_run for all lanes, and the lanes whose
//                                      walk has ended shade their segment and begin the next one, end the sample or end the entry.
// Both forms write the same bytes: an entry's result depends on its own record alone.  No atomic touches a result; a result goes out as
// two float4 stores.
// What the streaming form shares with k_query_stream and k_list_stream (brt_pixels_dev.h), its launch included: brt_stream.h.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "brt_radiance.h"
#include "brt_stream.h"

namespace brt {

namespace {

constexpr float kPosInf = __builtin_inff();

struct RadianceRay {
    f3 o, d;
    uint32_t seed, user;
};

BRT_DEV RadianceRay radiance_load(const RadianceArgs& ra, uint32_t i) {
    const float4 r0 = ra.rays[2 * (size_t)i], r1 = ra.rays[2 * (size_t)i + 1];
    RadianceRay r;
    r.o = mk3(r0.x, r0.y, r0.z);
    r.seed = __float_as_uint(r0.w);
    r.d = mk3(r1.x, r1.y, r1.z);
    r.user = __float_as_uint(r1.w);
    return r;
}

// 0: the entry is traced; else the refusal (the ray queries' rule without its t_max clause)
BRT_DEV uint32_t radiance_refusal(const RadianceRay& r, float bound) {
    const bool finite = __builtin_isfinite(r.o.x) && __builtin_isfinite(r.o.y) && __builtin_isfinite(r.o.z) && __builtin_isfinite(r.d.x) &&
                        __builtin_isfinite(r.d.y) && __builtin_isfinite(r.d.z);
    if (!finite) return BRT_QUERY_STATUS_INVALID;
    const float l1 = (__builtin_fabsf(r.o.x) + __builtin_fabsf(r.o.y)) + __builtin_fabsf(r.o.z);
    return l1 > bound ? (uint32_t)BRT_QUERY_STATUS_OUT_OF_REACH : 0u;
}

// a refused entry: a miss with rgb = 0
BRT_DEV void radiance_store_refused(const RadianceArgs& ra, uint32_t i, uint32_t status, uint32_t user) {
    ra.out[2 * (size_t)i] = make_float4(kPosInf, 0.0f, 0.0f, 0.0f);
    ra.out[2 * (size_t)i + 1] = make_float4(__uint_as_float(BRT_QUERY_NONE), __uint_as_float(BRT_QUERY_NONE), __uint_as_float(status), __uint_as_float(user));
}

// The record of an entry whose samples have ended: rgb = sum / f32(samples) (raytrace.wgsl:169), the first-hit fields from the walk of
// its own ray (t0, idx0; t0 == kInf: nothing accepted) as a CLOSEST ray query of {o, +INF, d} reports them.  Returns whether that ray hit.
// spheres: the resident spheres (global memory or their LDS copy: the same values)
BRT_DEV bool radiance_store(const RadianceArgs& ra, const DeviceSceneView& sv, const float4* spheres, uint32_t i, f3 o, f3 d, uint32_t user,
                            float t0, uint32_t idx0, f3 sum) {
    const float n_f = (float)ra.samples;
    const f3 rgb = mk3(sum.x / n_f, sum.y / n_f, sum.z / n_f);
    if (t0 == kInf) {
        ra.out[2 * (size_t)i] = make_float4(kPosInf, rgb.x, rgb.y, rgb.z);
        ra.out[2 * (size_t)i + 1] = make_float4(__uint_as_float(BRT_QUERY_NONE), __uint_as_float(BRT_QUERY_NONE), __uint_as_float(BRT_QUERY_STATUS_MISS),
                                                __uint_as_float(user));
        return false;
    }
    const float4 s = spheres[idx0];
    const f3 pos = mk3(o.x + t0 * d.x, o.y + t0 * d.y, o.z + t0 * d.z);               // ray_at (raytrace.wgsl:130-132)
    const f3 n = normalize3(mk3(pos.x - s.x, pos.y - s.y, pos.z - s.z));              // :356
    const bool front = dot3(d, n) < 0.0f;                                              // :358
    ra.out[2 * (size_t)i] = make_float4(t0, rgb.x, rgb.y, rgb.z);
    ra.out[2 * (size_t)i + 1] = make_float4(__uint_as_float(ra.rmap ? ra.rmap[idx0] : idx0), __uint_as_float(sv.sphere_material[idx0]),
                                            __uint_as_float(BRT_QUERY_STATUS_HIT | (front ? BRT_QUERY_STATUS_FRONT_FACE : 0u)), __uint_as_float(user));
    return true;
}

// the wave's counts into ra.stat (all lanes of the wave call it)
BRT_DEV void radiance_count(const RadianceArgs& ra, uint32_t walks, uint32_t hits, uint32_t refused) {
    if (!ra.stat) return;
    walks = wave_sum(walks);
    hits = wave_sum(hits);
    refused = wave_sum(refused);
    if (lane_id() == 0u) {
        if (walks) atomicAdd(ra.stat + 0, (unsigned long long)walks);
        if (hits) atomicAdd(ra.stat + 1, (unsigned long long)hits);
        if (refused) atomicAdd(ra.stat + 2, (unsigned long long)refused);
    }
}

// what shade_segment reads of the frame: the bounce limit (raytrace.wgsl:189)
BRT_DEV FrameParams radiance_frame(const RadianceArgs& ra) {
    FrameParams fp = {};
    fp.level = 3u;
    fp.bounce_count = ra.bounces;
    return fp;
}

}  // namespace

// ---- plain form ----------------------------------------------------------------------------------------------------------------------

// The stack of a thread is column threadIdx.x of stacks[34][256] (DONE sentinel + 32 entries + one spare; raycast's STRIDE = 256): a
// private array indexed by the walk would live in scratch memory.  Consecutive lanes hit consecutive banks.  The scene is not staged,
// so the 34 KiB cost nothing but occupancy (4 workgroups per CU), which the launch does not miss.
template <bool D16>
__global__ __launch_bounds__(256) void k_radiance_plain(DeviceSceneView sv, RadianceArgs ra) {
    __shared__ uint32_t stacks[34 * 256];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t walks = 0u, hits = 0u, refused = 0u;
    if (i < ra.n_rays) {
        const RadianceRay r = radiance_load(ra, i);
        const uint32_t refusal = radiance_refusal(r, ra.bound);
        if (refusal != 0u) {
            radiance_store_refused(ra, i, refusal, r.user);
            refused = 1u;
        } else {
            const ScenePtrs sc = scene_global(sv);
            const FrameParams fp = radiance_frame(ra);
            HitCounters hc = {};
            uint32_t* stack = stacks + threadIdx.x;
            float t0;
            uint32_t idx0;
            raycast<256, false, D16, false>(sc, sv.root_desc, stack, r.o, r.d, t0, idx0, hc);      // the entry's own ray: once
            walks = 1u;
            uint32_t rng = r.seed;
            f3 sum = mk3(0.0f, 0.0f, 0.0f);
            for (uint32_t s = 0; s < ra.samples; s++) {               // raytrace.wgsl:161
                f3 o = r.o, d = r.d, tput = mk3(1.0f, 1.0f, 1.0f);
                float first_depth = kInf, t = t0;
                uint32_t bounce = 0u, idx = idx0;
                f3 color;
                while (!shade_segment<false>(sc, fp, o, d, tput, bounce, first_depth, t, idx, rng, color, hc)) {
                    raycast<256, false, D16, false>(sc, sv.root_desc, stack, o, d, t, idx, hc);
                    walks++;
                }
                sum = sum + color;                                    // :165
            }
            hits = radiance_store(ra, sv, sc.spheres, i, r.o, r.d, r.user, t0, idx0, sum) ? 1u : 0u;
        }
    }
    radiance_count(ra, walks, hits, refused);
}

// ---- streaming form ------------------------------------------------------------------------------------------------------------------

template <int MODE, bool D16, bool SIMPLE>
__global__ __launch_bounds__(BRT_BLOCK) void k_radiance_stream(DeviceSceneView sv, RadianceArgs ra) {
    static_assert(MODE == SCENE_GLOBAL || D16, "a scene staged in LDS always uses 16-bit descriptors");
    using StackT = typename std::conditional<D16, int16_t, int32_t>::type;   // sign-extending loads: brt_layout.h
    using DS = Desc<D16>;
    extern __shared__ uint4 smem[];
    ScenePtrs sc = scene_global(sv);
    StackT* stacks = stream_stage<MODE, StackT>(sv, smem, sc);
    const uint32_t lane = lane_id();
    StackT* stk = stream_stack<D16>(sv, stacks, lane);
    const FrameParams fp = radiance_frame(ra);

    WalkState<StackT> walk = walk_idle<D16>(stk);
    // the entry: its own ray and the walk of it (kept for every sample), its random state, sum and sample number
    f3 o0 = mk3(0.0f, 0.0f, 0.0f), d0 = mk3(0.0f, 0.0f, 1.0f);
    float t0 = kInf;
    uint32_t idx0 = 0xffffffffu;
    uint32_t entry = 0u, user = 0u, rng = 0u, sample = 0u;
    f3 sum = mk3(0.0f, 0.0f, 0.0f);
    // the path under way
    f3 o = o0, d = d0, tput = mk3(1.0f, 1.0f, 1.0f);
    uint32_t bounce = 0u;
    float first_depth = kInf;
    bool in_flight = false;          // this lane holds an entry whose samples have not ended
    bool exhausted = false;          // wave-uniform: the batch counter has passed the last entry
    uint32_t walks = 0u, hits = 0u, refused = 0u;
    HitCounters hc = {};
    for (;;) {
        if (!exhausted) {
            // entries for the idle lanes: one fetch-add of the wave
            const uint64_t idle = __ballot(!in_flight);
            const uint32_t cnt = (uint32_t)__popcll(idle);
            uint32_t base = 0u;
            if (lane == 0u) base = atomicAdd(ra.counter, cnt);
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            exhausted = base >= ra.n_rays || ra.n_rays - base <= cnt;
            const uint32_t mine = base + mbcnt64(idle);
            if (!in_flight && base < ra.n_rays && mine < ra.n_rays) {
                const RadianceRay r = radiance_load(ra, mine);
                const uint32_t refusal = radiance_refusal(r, ra.bound);
                if (refusal != 0u) {
                    radiance_store_refused(ra, mine, refusal, r.user);
                    refused++;
                } else {
                    entry = mine;
                    user = r.user;
                    rng = r.seed;
                    o0 = o = r.o;
                    d0 = d = r.d;
                    sum = mk3(0.0f, 0.0f, 0.0f);
                    sample = 0u;
                    tput = mk3(1.0f, 1.0f, 1.0f);
                    first_depth = kInf;
                    bounce = 0u;
                    walk_begin<D16>(walk, sc, sv.root_desc, stk, d);
                    in_flight = true;
                }
            }
        }
        walk_run<64, false, D16, SIMPLE, MODE, StackT>(sc, walk, stk, o, d, kWalkExitLanes, kLeafVote, hc);
        if (in_flight && !walk_pending<D16, SIMPLE>(walk)) {
            walks++;
            float t = walk.closest;
            uint32_t idx = walk.closest_idx;
            // the only walk of an entry that ends at bounce 0 is that of its own ray: later samples begin on the stored hit below, and a
            // path that goes on from it has bounce >= 1
            if (bounce == 0u) { t0 = t; idx0 = idx; }
            for (;;) {
                f3 color;
                if (!shade_segment<false>(sc, fp, o, d, tput, bounce, first_depth, t, idx, rng, color, hc)) break;      // the path goes on: a walk
                sum = sum + color;                                      // :165
                sample++;
                if (sample >= ra.samples) {
                    hits += radiance_store(ra, sv, sc.spheres, entry, o0, d0, user, t0, idx0, sum) ? 1u : 0u;
                    in_flight = false;
                    break;
                }
                // the next sample: the entry's own ray again, on the walk it already has (raytrace.wgsl:162 without the jitter)
                o = o0; d = d0;
                tput = mk3(1.0f, 1.0f, 1.0f);
                first_depth = kInf;
                bounce = 0u;
                t = t0; idx = idx0;
            }
            if (in_flight) walk_begin<D16>(walk, sc, sv.root_desc, stk, d);
            else walk.cur = DS::DONE;
        }
        if (exhausted && __ballot(in_flight) == 0ull) break;
    }
    radiance_count(ra, walks, hits, refused);
}

// ---- host-callable launcher ----------------------------------------------------------------------------------------------------------

struct RadianceStream {
    template <int MODE, bool D16, bool SIMPLE>
    static auto kernel() { return k_radiance_stream<MODE, D16, SIMPLE>; }
};

hipError_t launch_radiance(const RadianceLaunch& rl) {
    if (rl.args.n_rays == 0u) return hipSuccess;
    if (!rl.args.rays || !rl.args.out || rl.args.samples == 0u) return hipErrorInvalidValue;
    if (rl.form == LIST_PLAIN) {
        const dim3 grid((rl.args.n_rays + 255u) / 256u);
        if (rl.scene.desc16) hipLaunchKernelGGL(k_radiance_plain<true>, grid, dim3(256), 0, rl.stream, rl.scene, rl.args);
        else hipLaunchKernelGGL(k_radiance_plain<false>, grid, dim3(256), 0, rl.stream, rl.scene, rl.args);
        return hipGetLastError();
    }
    return launch_stream<RadianceStream>(rl, rl.args.counter, rl.args);
}

}  // namespace brt
