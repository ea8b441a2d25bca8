// brt_lens.hip -- Pure frames and pixel lists under the lens rule (brt_render_lens*; DESIGN.md "Lens frames"): the two forms of the
// sparse pixel tracer (brt_pixels.hip) with one change -- a sample starts with lens_sample (THE LENS RULE, brt_lens.h: a pinhole, a thin
// lens or an orthographic ray; the kernels are compiled per mode) where those call camera_ray_dir and take the camera's position.
// Everything else is theirs: pixels_begin's seed, walk / shade_segment, the value and its store, the counter claim of a round, the
// launch (launch_stream, brt_stream.h).  The lens terms are kernel arguments (scalar registers); a lane's origin is the `o` a path
// carries anyway.
//
// k_lens_plain<LENS, D16>                 one thread per entry, the scene in global memory, a private stack.
// k_lens_stream<LENS, MODE, D16, SIMPLE>  persistent workgroups, a lane carries one path (k_trace_pixels_stream).
// A null list: entry i is pixel i, in raster order.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "brt_pixels_dev.h"

namespace brt {

namespace {

// one sample's primary ray on the RNG state of its pixel
template <uint32_t LENS>
BRT_DEV void lens_sample(const FrameParams& fp, const LensView& lv, const PixelState& ps, uint32_t& rng, f3& o, f3& d) {
    float oo[3], w[3];
    const bool raw = lens_ray_raw(fp, lv, LENS, ps.ndc0x, ps.ndc0y, rng, oo, w);
    o = mk3(oo[0], oo[1], oo[2]);
    d = mk3(w[0], w[1], w[2]);
    if (raw) d = normalize3(d);
}

BRT_DEV uint32_t lens_pixel_of(const PixelsArgs& pa, uint32_t i) { return pa.pixels ? pa.pixels[i] : i; }

}  // namespace

// ---- plain form ----------------------------------------------------------------------------------------------------------------------

template <uint32_t LENS, bool D16>
__global__ __launch_bounds__(256) void k_lens_plain(DeviceSceneView sv, FrameParams fp, PixelsArgs pa, LensView lv) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t n_rays = 0u, refused = 0u;
    if (i < pixels_n(pa)) {
        const uint32_t p = lens_pixel_of(pa, i);
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
                lens_sample<LENS>(fp, lv, ps, ps.rng, o, d);
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

template <uint32_t LENS, int MODE, bool D16, bool SIMPLE>
__global__ __launch_bounds__(BRT_BLOCK) void k_lens_stream(DeviceSceneView sv, FrameParams fp, PixelsArgs pa, LensView lv) {
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
                const uint32_t p = lens_pixel_of(pa, mine);
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
                        lens_sample<LENS>(fp, lv, ps, ps.rng, o, d);
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
                    lens_sample<LENS>(fp, lv, ps, ps.rng, o, d);
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

template <uint32_t LENS>
struct LensStream {
    template <int MODE, bool D16, bool SIMPLE>
    static auto kernel() { return k_lens_stream<LENS, MODE, D16, SIMPLE>; }
};

template <uint32_t LENS>
static hipError_t launch_lens_mode(const LensLaunch& ll) {
    if (ll.form == LIST_PLAIN) {
        const dim3 grid((ll.args.n_pixels + 255u) / 256u);
        if (ll.scene.desc16) hipLaunchKernelGGL((k_lens_plain<LENS, true>), grid, dim3(256), 0, ll.stream, ll.scene, ll.frame, ll.args, ll.lens);
        else hipLaunchKernelGGL((k_lens_plain<LENS, false>), grid, dim3(256), 0, ll.stream, ll.scene, ll.frame, ll.args, ll.lens);
        return hipGetLastError();
    }
    return launch_stream<LensStream<LENS>>(ll, ll.args.counter, ll.frame, ll.args, ll.lens);
}

hipError_t launch_trace_lens(const LensLaunch& ll) {
    if (ll.args.n_pixels == 0u) return hipSuccess;
    if (!ll.args.out || ll.frame.policy_flags != 0u) return hipErrorInvalidValue;
    switch (ll.lens.mode) {
        case LENS_PINHOLE: return launch_lens_mode<LENS_PINHOLE>(ll);
        case LENS_THIN: return launch_lens_mode<LENS_THIN>(ll);
        case LENS_ORTHO: return launch_lens_mode<LENS_ORTHO>(ll);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace brt
