// brt_progressive.hip -- progressive frames (brt_*progressive*; DESIGN.md "Progressive frames"): the two forms of the sparse pixel tracer
// (brt_pixels_dev.h) with a pixel that starts from and ends in its 32-byte record (brt_progressive.h), and the kernel that selects from
// the records the pixels a target sample count is still worth.
//
// k_prog_plain<D16>                 one thread per entry, the scene in global memory, a private stack (k_list_plain's loop).
// k_prog_stream<MODE, D16, SIMPLE>  persistent workgroups, the scene or the top of the tree staged in LDS, the stacks in LDS, entries from
//                                   the batch counter (k_list_stream's round).
// A lane that takes an entry loads the pixel's record as two 16-byte words; with n >= target it stores the value and is done; else it
// begins the pixel as pixels_begin does, takes rng and sum from the record where n > 0, runs samples until n == target, and stores the
// record as two 16-byte words and the value through pixels_store's scatter path.  What they share with the list kernels is shared, not
// copied: pixels_begin / pixels_n / pixels_store / pixels_count, walk_run, shade_segment, stream_stage, the stacks, launch_stream.  Both
// forms write the same bytes; no atomic touches a record or a frame.
//
// k_prog_select<MASK_ONLY>          one thread per pixel, 256 threads = one 16x16 tile.  The own flags (prog_noisy) of the tile and a
//                                   one-pixel apron are staged in LDS (18 x 18 bytes; outside the frame: quiet), then every thread takes
//                                   its class from LDS (prog_classify), writes the class byte and appends a selected pixel to the list as
//                                   k_adaptive_select does: one ballot and one atomicAdd per wave on the count word, plain vector stores.
#include <hip/hip_runtime.h>

#include "brt_pixels_dev.h"
#include "brt_progressive.h"

namespace brt {

namespace {

constexpr uint32_t kProgPad = 0xffffffffu;      // a slot of a partial tile outside the frame (tile order)

// the pixel entry i names; kProgPad: none, and nothing is refused
BRT_DEV uint32_t prog_pixel_of(const FrameParams& fp, const PixelsArgs& pa, const ProgSample& pg, uint32_t i) {
    if (pa.pixels) return pa.pixels[i];
    if (pg.order == 0u) return i;
    const uint32_t tiles_x = (fp.width + 7u) >> 3, tile = i >> 6, t = i & 63u;
    const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const uint32_t px = tx * 8u + (t & 7u), py = ty * 8u + (t >> 3);
    return (px < fp.width && py < fp.height) ? py * fp.width + px : kProgPad;
}

// a sample starts as k_trace_simple's does (raytrace.wgsl:162, :175-186)
BRT_DEV void prog_ray(const FrameParams& fp, const PixelState& ps, uint32_t& rng, f3& o, f3& d) {
    d = camera_ray_dir(fp, ps.ndc0x, ps.ndc0y, rng);
    o = mk3(fp.cam_pos[0], fp.cam_pos[1], fp.cam_pos[2]);
}

struct ProgWords { uint4 a, b; };      // {sum.r, sum.g, sum.b, m1} {m2, rng, n, rays}
BRT_DEV ProgWords prog_load(const ProgSample& pg, uint32_t p) {
    const uint4* r = reinterpret_cast<const uint4*>(pg.state + p);
    ProgWords w;
    w.a = r[0];
    w.b = r[1];
    return w;
}
BRT_DEV void prog_store(const ProgSample& pg, uint32_t p, const PixelState& ps, float m1, float m2, uint32_t rays) {
    uint4* r = reinterpret_cast<uint4*>(pg.state + p);
    r[0] = make_uint4(__float_as_uint(ps.sum.x), __float_as_uint(ps.sum.y), __float_as_uint(ps.sum.z), __float_as_uint(m1));
    r[1] = make_uint4(__float_as_uint(m2), ps.rng, ps.sample, rays);
}
// the value of a pixel with n samples and the colour sum `sum` (raytrace.wgsl:169, :122)
BRT_DEV float4 prog_value(f3 sum, uint32_t n) {
    if (n == 0u) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float nf = (float)n;
    return make_float4(sum.x / nf, sum.y / nf, sum.z / nf, 1.0f);
}
BRT_DEV void prog_store_value(const PixelsArgs& pa, uint32_t i, uint32_t p, f3 sum, uint32_t n) {
    if (pa.out) pixels_store(pa, i, p, prog_value(sum, n));
}
// the pixel p from its record: false if the record has the target's samples already (its value is stored)
BRT_DEV bool prog_begin(const FrameParams& fp, const PixelsArgs& pa, const ProgSample& pg, uint32_t i, uint32_t p, PixelState& ps,
                        float& m1, float& m2, uint32_t& rays) {
    const ProgWords w = prog_load(pg, p);
    const f3 sum = mk3(__uint_as_float(w.a.x), __uint_as_float(w.a.y), __uint_as_float(w.a.z));
    const uint32_t n = w.b.z;
    if (n >= pg.target) {
        prog_store_value(pa, i, p, sum, n);
        return false;
    }
    pixels_begin(fp, p, ps);
    m1 = 0.0f;
    m2 = 0.0f;
    rays = 0u;
    if (n != 0u) {
        ps.sum = sum;
        ps.rng = w.b.y;
        ps.sample = n;
        m1 = __uint_as_float(w.a.w);
        m2 = __uint_as_float(w.b.x);
        rays = w.b.w;
    }
    return true;
}

BRT_DEV void prog_count(const PixelsArgs& pa, const ProgSample& pg, uint32_t rays, uint32_t refused, uint32_t samples) {
    pixels_count(pa, rays, refused);
    if (!pg.samples) return;
    samples = wave_sum(samples);
    if (lane_id() == 0u && samples) atomicAdd(pg.samples, (unsigned long long)samples);
}

// ---- plain form ----------------------------------------------------------------------------------------------------------------------

template <bool D16>
__global__ __launch_bounds__(256) void k_prog_plain(DeviceSceneView sv, FrameParams fp, PixelsArgs pa, ProgSample pg) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t n_rays = 0u, refused = 0u, n_samples = 0u;
    if (i < pixels_n(pa)) {
        const uint32_t p = prog_pixel_of(fp, pa, pg, i);
        if (p == kProgPad && !pa.pixels) {
        } else if (p >= fp.width * fp.height) {
            refused = 1u;
        } else {
            PixelState ps;
            float m1, m2;
            uint32_t rays;
            if (prog_begin(fp, pa, pg, i, p, ps, m1, m2, rays)) {
                const ScenePtrs sc = scene_global(sv);
                HitCounters hc = {};
                uint32_t stack[34];   // DONE sentinel + 32 entries + one spare
                for (; ps.sample < pg.target; ps.sample++) {          // raytrace.wgsl:161
                    f3 o, d;
                    prog_ray(fp, ps, ps.rng, o, d);
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
                    prog_moments(m1, m2, color.x, color.y, color.z);
                    n_samples++;
                }
                prog_store(pg, p, ps, m1, m2, rays + n_rays);
                prog_store_value(pa, i, p, ps.sum, ps.sample);
            }
        }
    }
    prog_count(pa, pg, n_rays, refused, n_samples);
}

// ---- streaming form ------------------------------------------------------------------------------------------------------------------

template <int MODE, bool D16, bool SIMPLE>
__global__ __launch_bounds__(BRT_BLOCK) void k_prog_stream(DeviceSceneView sv, FrameParams fp, PixelsArgs pa, ProgSample pg) {
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
    float m1 = 0.0f, m2 = 0.0f;
    uint32_t entry = 0u, pixel = 0u, px_rays = 0u;
    bool in_flight = false;          // this lane holds a pixel whose samples have not ended
    bool exhausted = false;          // wave-uniform: the batch counter has passed the last entry
    uint32_t n_rays = 0u, refused = 0u, n_samples = 0u;
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
                const uint32_t p = prog_pixel_of(fp, pa, pg, mine);
                if (p == kProgPad && !pa.pixels) {
                } else if (p >= frame_px) {
                    refused++;
                } else if (prog_begin(fp, pa, pg, mine, p, ps, m1, m2, px_rays)) {
                    entry = mine;
                    pixel = p;
                    prog_ray(fp, ps, ps.rng, o, d);
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
            n_rays++;
            px_rays++;
            f3 color;
            if (shade_segment<false>(sc, fp, o, d, tput, bounce, first_depth, walk.closest, walk.closest_idx, ps.rng, color, hc)) {
                ps.sum = ps.sum + color;                                // :165
                prog_moments(m1, m2, color.x, color.y, color.z);
                ps.sample++;
                n_samples++;
                if (ps.sample < pg.target) {
                    prog_ray(fp, ps, ps.rng, o, d);
                    tput = mk3(1.0f, 1.0f, 1.0f);
                    first_depth = kInf;
                    bounce = 0u;
                } else {
                    prog_store(pg, pixel, ps, m1, m2, px_rays);
                    prog_store_value(pa, entry, pixel, ps.sum, ps.sample);
                    in_flight = false;
                }
            }
            if (in_flight) walk_begin<D16>(walk, sc, sv.root_desc, stk, d);
            else walk.cur = DS::DONE;
        }
        if (exhausted && __ballot(in_flight) == 0ull) break;
    }
    prog_count(pa, pg, n_rays, refused, n_samples);
}

struct ProgStream {
    template <int MODE, bool D16, bool SIMPLE>
    static auto kernel() { return k_prog_stream<MODE, D16, SIMPLE>; }
};

// ---- selection -----------------------------------------------------------------------------------------------------------------------

constexpr uint32_t kTile = 16u, kSpan = kTile + 2u;      // the tile and its one-pixel apron

// k_adaptive_select's append: the lanes of the wave with `sel` set append p to the list.  Every lane of the wave calls it.
BRT_DEV void prog_append(const ProgSelect& sl, bool sel, uint32_t p) {
    const uint64_t m = __ballot(sel);
    if (m == 0ull) return;
    const uint32_t lane = lane_id();
    const uint32_t leader = (uint32_t)__builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
    uint32_t first = 0u;
    if (lane == leader) first = atomicAdd(sl.count, (uint32_t)__popcll(m));
    first = (uint32_t)__builtin_amdgcn_readlane((int)first, (int)leader);
    if (sel) sl.list[first + mbcnt64(m)] = p;
}

template <bool MASK_ONLY>
__global__ __launch_bounds__(256) void k_prog_select(ProgSelect sl) {
    __shared__ uint8_t flags[kSpan * kSpan];
    const int x0 = (int)(blockIdx.x * kTile) - 1, y0 = (int)(blockIdx.y * kTile) - 1;
    for (uint32_t i = threadIdx.x; i < kSpan * kSpan; i += 256u) {
        const int tx = x0 + (int)(i % kSpan), ty = y0 + (int)(i / kSpan);
        uint8_t f = 0u;                             // outside the frame: quiet
        if (tx >= 0 && tx < (int)sl.width && ty >= 0 && ty < (int)sl.height) {
            const uint4* r = reinterpret_cast<const uint4*>(sl.state + ((uint32_t)ty * sl.width + (uint32_t)tx));
            const uint4 a = r[0], b = r[1];
            f = prog_noisy(__uint_as_float(a.w), __uint_as_float(b.x), b.z, sl.threshold) ? 1u : 0u;
        }
        flags[i] = f;
    }
    __syncthreads();
    const uint32_t lx = threadIdx.x & (kTile - 1u), ly = threadIdx.x / kTile;
    const uint32_t px = blockIdx.x * kTile + lx, py = blockIdx.y * kTile + ly;
    const bool inside = px < sl.width && py < sl.height;
    const uint32_t p = py * sl.width + px;
    uint32_t cls = 0u;
    if (inside) {
        const int at = (int)((ly + 1u) * kSpan + lx + 1u);
        cls = prog_classify(sl.state[p].n, sl.target, (int)sl.radius, [&](int dx, int dy) { return flags[at + dy * (int)kSpan + dx] != 0u; });
    }
    if (inside && sl.mask) sl.mask[p] = (uint8_t)cls;
    if constexpr (!MASK_ONLY) prog_append(sl, cls != 0u, p);
}

}  // namespace

// ---- host-callable launchers ---------------------------------------------------------------------------------------------------------

hipError_t launch_prog_sample(const PixelsLaunch& pl, const ProgSample& pg) {
    if (pl.args.n_pixels == 0u) return hipSuccess;
    if (!pg.state || pg.target == 0u || pg.target > kProgMaxSamples || pg.order > 1u || pl.frame.policy_flags != 0u || !pl.args.scatter)
        return hipErrorInvalidValue;
    if (pl.form == LIST_PLAIN) {
        const dim3 grid((pl.args.n_pixels + 255u) / 256u);
        if (pl.scene.desc16) hipLaunchKernelGGL((k_prog_plain<true>), grid, dim3(256), 0, pl.stream, pl.scene, pl.frame, pl.args, pg);
        else hipLaunchKernelGGL((k_prog_plain<false>), grid, dim3(256), 0, pl.stream, pl.scene, pl.frame, pl.args, pg);
        return hipGetLastError();
    }
    return launch_stream<ProgStream>(pl, pl.args.counter, pl.frame, pl.args, pg);
}

hipError_t launch_prog_select(const ProgSelect& ps, hipStream_t stream) {
    if (ps.width == 0u || ps.height == 0u || ps.width > 32768u || ps.height > 32768u || !ps.state || ps.radius > 1u) return hipErrorInvalidValue;
    if ((ps.list == nullptr) != (ps.count == nullptr) || (!ps.list && !ps.mask)) return hipErrorInvalidValue;
    const dim3 grid((ps.width + kTile - 1u) / kTile, (ps.height + kTile - 1u) / kTile);
    if (ps.list) hipLaunchKernelGGL((k_prog_select<false>), grid, dim3(256), 0, stream, ps);
    else hipLaunchKernelGGL((k_prog_select<true>), grid, dim3(256), 0, stream, ps);
    return hipGetLastError();
}

}  // namespace brt
