// brt_pixels_dev.h -- the two forms of the kernel that traces a list of pixels, and what they are made of: a list's length, an entry's
// store and refusal, the wave's counts, a pixel's begin and value; and their launch (launch_list).  Device code: included by
// brt_pixels.hip, brt_lens.hip and brt_progressive.hip only, which each instantiate the kernels with a rule of their own that says WHAT A
// PIXEL IS (PinholeStart, LensStart<LENS>, ProgStart).  A rule is a type of static functions:
//   Rule::Lane                                        what a lane keeps for its pixel beyond PixelState (empty, or the record's moments)
//   Rule::pixel_of(fp, pa, i, extra...)               the pixel entry i names (whether a null list means "entry i is pixel i")
//   Rule::pads()                                      whether pixel_of answers kListPad for an entry of a null list that names no pixel and is
//                                                     passed over: not traced, not refused (a constant, and the test is the kernel's own: behind
//                                                     a hook the progressive kernels' round is laid out differently)
//   Rule::refuse(pa, i, extra...)                     entry i names no pixel of the frame
//   Rule::begin(fp, pa, i, p, ps, lane, extra...)     pixel p before its next sample; false: it has ended already and has been dealt with
//   Rule::begins_ended(fp, extra...)                  whether a pixel that began may have no sample to run (the round then ends it at once)
//   Rule::target(fp, extra...)                        the pixel ends once ps.sample has reached it
//   Rule::sample(fp, ps, rng, o, d, extra...)         one sample's primary ray on the RNG state of its pixel
//   Rule::walked(lane) / Rule::sampled(lane, color)   one more walk / one more sample of the lane's pixel
//   Rule::end(fp, p, ps, lane, extra...)              the pixel's samples have ended: what the rule keeps of it besides its value
//   Rule::stores(pa) / Rule::value(fp, ps, extra...)  whether the call wants the value of an ended pixel (host and device: a launch that
//                                                     does needs an output plane), and the value.  The kernel calls pixels_store with it
//                                                     itself: behind a hook of the rule pixels_store's format switch is selected differently.
//   Rule::count(pa, rays, refused, lane, extra...)    the wave's counts (all lanes of the wave call it)
// WholePixel is the rule of brt_pixels.h's list but for pixel_of and sample: a pixel from pixel_begin's seed to fp.sample_count samples.
// extra: what the rule takes beyond the frame, as trailing kernel arguments (scalar registers) -- nothing, the lens terms, or the
// progressive terms.  (A rule passed as an empty struct would take kernel-argument space, and a shared body behind thin __global__
// wrappers changes the instruction selection of pixels_store: with the rule a type and the terms a pack, every instantiation keeps its
// instructions.  A rule holds functions only: with a static data member in it, the kernels' hand-written walk loops do not compile for
// the host.)
//
// k_list_plain<Rule, D16, Extra...>                 one thread per entry: k_trace_simple's loop over a list, the scene in global memory, a
//                                                   private stack.  Every scene representation and tree.
// k_list_stream<Rule, MODE, D16, SIMPLE, Extra...>  persistent workgroups: the scene (SCENE_LDS) or the top of the tree (SCENE_LDS_TOP) staged
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

constexpr uint32_t kListPad = 0xffffffffu;      // a slot of a null list that names no pixel (Rule::pads)

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

// A whole pixel of the Pure frame: from pixel_begin's seed through fp.sample_count samples to the frame's value.  An entry that names no
// pixel of the frame stores four zeros where the list is packed.
struct WholePixel {
    struct Lane {};
    static constexpr bool pads() { return false; }
    template <class... Extra>
    static BRT_DEV void refuse(const PixelsArgs& pa, uint32_t i, const Extra&...) {
        if (!pa.scatter) reinterpret_cast<float4*>(pa.out)[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    template <class... Extra>
    static BRT_DEV bool begin(const FrameParams& fp, const PixelsArgs&, uint32_t, uint32_t p, PixelState& ps, Lane&, const Extra&...) {
        pixels_begin(fp, p, ps);
        return true;
    }
    template <class... Extra>
    static BRT_DEV bool begins_ended(const FrameParams& fp, const Extra&...) { return fp.sample_count == 0u; }      // (the average of nothing)
    template <class... Extra>
    static BRT_DEV uint32_t target(const FrameParams& fp, const Extra&...) { return fp.sample_count; }
    static BRT_DEV void walked(Lane&) {}
    static BRT_DEV void sampled(Lane&, f3) {}
    template <class... Extra>
    static BRT_DEV void end(const FrameParams&, uint32_t, const PixelState&, Lane&, const Extra&...) {}
    static constexpr bool stores(const PixelsArgs&) { return true; }
    template <class... Extra>
    static BRT_DEV float4 value(const FrameParams& fp, const PixelState& ps, const Extra&...) { return pixels_value(fp, ps); }
    template <class... Extra>
    static BRT_DEV void count(const PixelsArgs& pa, uint32_t rays, uint32_t refused, Lane&, const Extra&...) { pixels_count(pa, rays, refused); }
};

// ---- plain form ----------------------------------------------------------------------------------------------------------------------

template <class Rule, bool D16, class... Extra>
__global__ __launch_bounds__(256) void k_list_plain(DeviceSceneView sv, FrameParams fp, PixelsArgs pa, Extra... extra) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t n_rays = 0u, refused = 0u;
    typename Rule::Lane lane{};
    if (i < pixels_n(pa)) {
        const uint32_t p = Rule::pixel_of(fp, pa, i, extra...);
        PixelState ps;
        if (Rule::pads() && p == kListPad && !pa.pixels) {
        } else if (p >= fp.width * fp.height) {
            Rule::refuse(pa, i, extra...);
            refused = 1u;
        } else if (Rule::begin(fp, pa, i, p, ps, lane, extra...)) {
            const ScenePtrs sc = scene_global(sv);
            HitCounters hc = {};
            uint32_t stack[34];   // DONE sentinel + 32 entries + one spare
            for (const uint32_t target = Rule::target(fp, extra...); ps.sample < target; ps.sample++) {          // raytrace.wgsl:161
                f3 o, d;
                Rule::sample(fp, ps, ps.rng, o, d, extra...);
                f3 tput = mk3(1.0f, 1.0f, 1.0f);
                float first_depth = kInf;
                uint32_t bounce = 0;
                f3 color;
                for (;;) {
                    float t;
                    uint32_t idx;
                    raycast<1, false, D16, false>(sc, sv.root_desc, stack, o, d, t, idx, hc);
                    n_rays++;
                    Rule::walked(lane);
                    if (shade_segment<false>(sc, fp, o, d, tput, bounce, first_depth, t, idx, ps.rng, color, hc)) break;
                }
                ps.sum = ps.sum + color;
                Rule::sampled(lane, color);
            }
            Rule::end(fp, p, ps, lane, extra...);
            if (Rule::stores(pa)) pixels_store(pa, i, p, Rule::value(fp, ps, extra...));
        }
    }
    Rule::count(pa, n_rays, refused, lane, extra...);
}

// ---- streaming form ------------------------------------------------------------------------------------------------------------------

template <class Rule, int MODE, bool D16, bool SIMPLE, class... Extra>
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
    typename Rule::Lane own{};
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
                const uint32_t p = Rule::pixel_of(fp, pa, mine, extra...);
                if (Rule::pads() && p == kListPad && !pa.pixels) {
                } else if (p >= frame_px) {
                    Rule::refuse(pa, mine, extra...);
                    refused++;
                } else if (Rule::begin(fp, pa, mine, p, ps, own, extra...)) {
                    entry = mine;
                    pixel = p;
                    if (Rule::begins_ended(fp, extra...)) {
                        Rule::end(fp, pixel, ps, own, extra...);
                        if (Rule::stores(pa)) pixels_store(pa, entry, pixel, Rule::value(fp, ps, extra...));
                    } else {
                        Rule::sample(fp, ps, ps.rng, o, d, extra...);
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
            Rule::walked(own);
            f3 color;
            if (shade_segment<false>(sc, fp, o, d, tput, bounce, first_depth, walk.closest, walk.closest_idx, ps.rng, color, hc)) {
                ps.sum = ps.sum + color;                                // :165
                Rule::sampled(own, color);
                ps.sample++;
                if (ps.sample < Rule::target(fp, extra...)) {
                    Rule::sample(fp, ps, ps.rng, o, d, extra...);
                    tput = mk3(1.0f, 1.0f, 1.0f);
                    first_depth = kInf;
                    bounce = 0u;
                } else {
                    Rule::end(fp, pixel, ps, own, extra...);
                    if (Rule::stores(pa)) pixels_store(pa, entry, pixel, Rule::value(fp, ps, extra...));
                    in_flight = false;
                }
            }
            if (in_flight) walk_begin<D16>(walk, sc, sv.root_desc, stk, d);
            else walk.cur = DS::DONE;
        }
        if (exhausted && __ballot(in_flight) == 0ull) break;
    }
    Rule::count(pa, n_rays, refused, own, extra...);
}

// ---- host-callable launcher ----------------------------------------------------------------------------------------------------------

template <class Rule, class... Extra>
struct ListStream {
    template <int MODE, bool D16, bool SIMPLE>
    static auto kernel() { return k_list_stream<Rule, MODE, D16, SIMPLE, Extra...>; }
};

// The list of pl under the rule Rule, in the form pl names.  null_list: a null list means "entry i is pixel i" (else it is refused).
template <class Rule, class... Extra>
static hipError_t launch_list(const PixelsLaunch& pl, bool null_list, const Extra&... extra) {
    if (pl.args.n_pixels == 0u) return hipSuccess;
    if ((!pl.args.pixels && !null_list) || (Rule::stores(pl.args) && !pl.args.out) || pl.frame.policy_flags != 0u) return hipErrorInvalidValue;
    if (pl.form == LIST_PLAIN) {
        const dim3 grid((pl.args.n_pixels + 255u) / 256u);
        if (pl.scene.desc16) hipLaunchKernelGGL((k_list_plain<Rule, true, Extra...>), grid, dim3(256), 0, pl.stream, pl.scene, pl.frame, pl.args, extra...);
        else hipLaunchKernelGGL((k_list_plain<Rule, false, Extra...>), grid, dim3(256), 0, pl.stream, pl.scene, pl.frame, pl.args, extra...);
        return hipGetLastError();
    }
    return launch_stream<ListStream<Rule, Extra...>>(pl, pl.args.counter, pl.frame, pl.args, extra...);
}

}  // namespace brt
