// brt_pixels_dev.h -- the two forms of the kernel that traces a list of pixels, and what they are made of: a list's length, an entry's
// store and refusal, the wave's counts, a pixel's begin and value; and their launch (launch_list).  Device code: included by
// brt_pixels.hip and brt_lens.hip only, which each instantiate the kernels with a start rule of their own (PinholeStart,
// LensStart<LENS>):
//   Start::pixel_of(pa, i)                       the pixel entry i names (whether a null list means "entry i is pixel i")
//   Start::sample(fp, ps, rng, o, d, extra...)   one sample's primary ray on the RNG state of its pixel
// extra: what the rule takes beyond the frame, as trailing kernel arguments (scalar registers) -- nothing, or the lens terms.  (A rule
// passed as an empty struct would take kernel-argument space, and a shared body behind thin __global__ wrappers changes the
// instruction selection of pixels_store: with the rule a type and the terms a pack, every instantiation keeps its instructions.  A
// rule holds functions only: with a static data member in it, the kernels' hand-written walk loops do not compile for the host.)
//
// k_list_plain<Start, D16, Extra...>                one thread per entry: k_trace_simple's loop over a list, the scene in global memory, a
//                                                   private stack.  Every scene representation and tree.
// k_list_stream<Start, MODE, D16, SIMPLE, Extra...> persistent workgroups: the scene (SCENE_LDS) or the top of the tree (SCENE_LDS_TOP) staged
//                                                   in LDS (stream_stage, brt_stream.h), the stacks in LDS, so the hand-written walk loops
//                                                   serve it.  A lane carries one path.  A round: the wave takes entries from the batch
//                                                   counter (one fetch-add) for the lanes whose pixel has ended, walk_run for all lanes, and
//                                                   the lanes whose walk has ended shade their segment and begin the next one, end the
//                                                   sample or end the pixel.
// Both forms write the same bytes: an entry's result depends on its pixel alone.  No atomic touches a result.
// What the streaming form shares with k_query_stream and k_radiance_stream, its launch included: brt_stream.h.
#pragma once
#include <type_traits>

#include "brt_pixels.h"
#include "brt_store.h"
#include "brt_stream.h"

namespace brt {

// the wave's counts into pa.stat (all lanes of the wave call it)
BRT_DEV void pixels_count(const PixelsArgs& pa, uint32_t rays, uint32_t refused) {
    if (!pa.stat) return;
    rays = wave_sum(rays);
    refused = wave_sum(refused);
    if (lane_id() == 0u) {
        if (rays) atomicAdd(pa.stat + 0, (unsigned long long)rays);
        if (refused) atomicAdd(pa.stat + 1, (unsigned long long)refused);
    }
}

BRT_DEV uint32_t pixels_n(const PixelsArgs& pa) {
    if (!pa.count) return pa.n_pixels;
    const uint32_t n = *pa.count;
    return n < pa.n_pixels ? n : pa.n_pixels;
}

// entry i, pixel p: its value where the call wants it
BRT_DEV void pixels_store(const PixelsArgs& pa, uint32_t i, uint32_t p, float4 v) {
    if (!pa.scatter) {
        reinterpret_cast<float4*>(pa.out)[i] = v;
        return;
    }
    switch (pa.out_format) {
        case BRT_FLAG_OUT_RGBA8_UNORM_SRGB: reinterpret_cast<uint32_t*>(pa.out)[p] = OutPixel<BRT_FLAG_OUT_RGBA8_UNORM_SRGB>::make(v); break;
        case BRT_FLAG_OUT_RGBA16F: reinterpret_cast<uint2*>(pa.out)[p] = OutPixel<BRT_FLAG_OUT_RGBA16F>::make(v); break;
        case BRT_FLAG_OUT_RGBA8_UNORM: reinterpret_cast<uint32_t*>(pa.out)[p] = OutPixel<BRT_FLAG_OUT_RGBA8_UNORM>::make(v); break;
        default: reinterpret_cast<float4*>(pa.out)[p] = OutPixel<BRT_FLAG_OUT_RGBA32F>::make(v); break;
    }
}

// entry i names no pixel of the frame
BRT_DEV void pixels_refuse(const PixelsArgs& pa, uint32_t i) {
    if (!pa.scatter) reinterpret_cast<float4*>(pa.out)[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

BRT_DEV void pixels_begin(const FrameParams& fp, uint32_t p, PixelState& ps) {
    PixelCoord c;
    c.py = p / fp.width;
    c.px = p - c.py * fp.width;
    c.local_row = c.py;
    c.tile = 0u;
    c.t = 0u;
    c.inside = true;
    pixel_begin(fp, c, ps);
}

// the Pure frame's value of a pixel whose samples have ended (pixel_finish<true>, raytrace.wgsl:169, :122)
BRT_DEV float4 pixels_value(const FrameParams& fp, const PixelState& ps) {
    return make_float4(ps.sum.x / fp.spp_f, ps.sum.y / fp.spp_f, ps.sum.z / fp.spp_f, 1.0f);
}

// ---- plain form ----------------------------------------------------------------------------------------------------------------------

template <class Start, bool D16, class... Extra>
__global__ __launch_bounds__(256) void k_list_plain(DeviceSceneView sv, FrameParams fp, PixelsArgs pa, Extra... extra) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t n_rays = 0u, refused = 0u;
    if (i < pixels_n(pa)) {
        const uint32_t p = Start::pixel_of(pa, i);
        if (p >= fp.width * fp.height) {
            pixels_refuse(pa, i);
            refused = 1u;
        } else {
            const ScenePtrs sc = scene_global(sv);
            HitCounters hc = {};
            PixelState ps;
            pixels_begin(fp, p, ps);
            uint32_t stack[34];   // DONE sentinel + 32 entries + one spare
            for (uint32_t s = 0; s < fp.sample_count; s++) {          // raytrace.wgsl:161
                f3 o, d;
                Start::sample(fp, ps, ps.rng, o, d, extra...);
                f3 tput = mk3(1.0f, 1.0f, 1.0f);
                float first_depth = kInf;
                uint32_t bounce = 0;
                f3 color;
                for (;;) {
                    float t;
                    uint32_t idx;
                    raycast<1, false, D16, false>(sc, sv.root_desc, stack, o, d, t, idx, hc);
                    n_rays++;
                    if (shade_segment<false>(sc, fp, o, d, tput, bounce, first_depth, t, idx, ps.rng, color, hc)) break;
                }
                ps.sum = ps.sum + color;
            }
            pixels_store(pa, i, p, pixels_value(fp, ps));
        }
    }
    pixels_count(pa, n_rays, refused);
}

// ---- streaming form ------------------------------------------------------------------------------------------------------------------

template <class Start, int MODE, bool D16, bool SIMPLE, class... Extra>
__global__ __launch_bounds__(BRT_BLOCK) void k_list_stream(DeviceSceneView sv, FrameParams fp, PixelsArgs pa, Extra... extra) {
    static_assert(MODE == SCENE_GLOBAL || D16, "a scene staged in LDS always uses 16-bit descriptors");
    using StackT = typename std::conditional<D16, int16_t, int32_t>::type;   // sign-extending loads: brt_layout.h
    using DS = Desc<D16>;
    extern __shared__ uint4 smem[];
    ScenePtrs sc = scene_global(sv);
    StackT* stacks = stream_stage<MODE, StackT>(sv, smem, sc);
    const uint32_t lane = lane_id();
    StackT* stk = stream_stack<D16>(sv, stacks, lane);
    const uint32_t n = pixels_n(pa), frame_px = fp.width * fp.height;

    WalkState<StackT> walk = walk_idle<D16>(stk);
    PixelState ps = {};
    f3 o = mk3(0.0f, 0.0f, 0.0f), d = mk3(0.0f, 0.0f, 1.0f), tput = mk3(1.0f, 1.0f, 1.0f);
    uint32_t bounce = 0u;
    float first_depth = kInf;
    uint32_t entry = 0u, pixel = 0u;
    bool in_flight = false;          // this lane holds a pixel whose samples have not ended
    bool exhausted = false;          // wave-uniform: the batch counter has passed the last entry
    uint32_t n_rays = 0u, refused = 0u;
    HitCounters hc = {};
    for (;;) {
        if (!exhausted) {
            // entries for the idle lanes: one fetch-add of the wave
            const uint64_t idle = __ballot(!in_flight);
            const uint32_t cnt = (uint32_t)__popcll(idle);
            uint32_t base = 0u;
            if (lane == 0u) base = atomicAdd(pa.counter, cnt);
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            exhausted = base >= n || n - base <= cnt;
            const uint32_t mine = base + mbcnt64(idle);
            if (!in_flight && base < n && mine < n) {
                const uint32_t p = Start::pixel_of(pa, mine);
                if (p >= frame_px) {
                    pixels_refuse(pa, mine);
                    refused++;
                } else {
                    entry = mine;
                    pixel = p;
                    pixels_begin(fp, p, ps);
                    if (fp.sample_count == 0u) {                       // (no sample: the average of nothing)
                        pixels_store(pa, entry, pixel, pixels_value(fp, ps));
                    } else {
                        Start::sample(fp, ps, ps.rng, o, d, extra...);
                        tput = mk3(1.0f, 1.0f, 1.0f);
                        first_depth = kInf;
                        bounce = 0u;
                        walk_begin<D16>(walk, sc, sv.root_desc, stk, d);
                        in_flight = true;
                    }
                }
            }
        }
        walk_run<64, false, D16, SIMPLE, MODE, StackT>(sc, walk, stk, o, d, kWalkExitLanes, kLeafVote, hc);
        if (in_flight && !walk_pending<D16, SIMPLE>(walk)) {
            n_rays++;
            f3 color;
            if (shade_segment<false>(sc, fp, o, d, tput, bounce, first_depth, walk.closest, walk.closest_idx, ps.rng, color, hc)) {
                ps.sum = ps.sum + color;                                // :165
                ps.sample++;
                if (ps.sample < fp.sample_count) {
                    Start::sample(fp, ps, ps.rng, o, d, extra...);
                    tput = mk3(1.0f, 1.0f, 1.0f);
                    first_depth = kInf;
                    bounce = 0u;
                } else {
                    pixels_store(pa, entry, pixel, pixels_value(fp, ps));
                    in_flight = false;
                }
            }
            if (in_flight) walk_begin<D16>(walk, sc, sv.root_desc, stk, d);
            else walk.cur = DS::DONE;
        }
        if (exhausted && __ballot(in_flight) == 0ull) break;
    }
    pixels_count(pa, n_rays, refused);
}

// ---- host-callable launcher ----------------------------------------------------------------------------------------------------------

template <class Start, class... Extra>
struct ListStream {
    template <int MODE, bool D16, bool SIMPLE>
    static auto kernel() { return k_list_stream<Start, MODE, D16, SIMPLE, Extra...>; }
};

// The list of pl under the rule Start, in the form pl names.  null_list: a null list means "entry i is pixel i" (else it is refused).
template <class Start, class... Extra>
static hipError_t launch_list(const PixelsLaunch& pl, bool null_list, const Extra&... extra) {
    if (pl.args.n_pixels == 0u) return hipSuccess;
    if ((!pl.args.pixels && !null_list) || !pl.args.out || pl.frame.policy_flags != 0u) return hipErrorInvalidValue;
    if (pl.form == LIST_PLAIN) {
        const dim3 grid((pl.args.n_pixels + 255u) / 256u);
        if (pl.scene.desc16) hipLaunchKernelGGL((k_list_plain<Start, true, Extra...>), grid, dim3(256), 0, pl.stream, pl.scene, pl.frame, pl.args, extra...);
        else hipLaunchKernelGGL((k_list_plain<Start, false, Extra...>), grid, dim3(256), 0, pl.stream, pl.scene, pl.frame, pl.args, extra...);
        return hipGetLastError();
    }
    return launch_stream<ListStream<Start, Extra...>>(pl, pl.args.counter, pl.frame, pl.args, extra...);
}

}  // namespace brt
