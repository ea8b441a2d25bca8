// brt_progressive.hip -- progressive frames (brt_*progressive*; DESIGN.md "Progressive frames"): the rule under which the two forms of
// the sparse pixel tracer (k_list_plain, k_list_stream: brt_pixels_dev.h) continue a pixel from its 32-byte record (brt_progressive.h),
// and the kernel that selects from the records the pixels a target sample count is still worth.
//
// ProgStart                         the rule.  A lane that takes an entry loads the pixel's record as two 16-byte words; with n >= target
//                                   it stores the value and is done; else it begins the pixel as pixels_begin does, takes rng and sum from
//                                   the record where n > 0, runs samples until n == target, and stores the record as two 16-byte words and
//                                   the value through pixels_store's scatter path.  A null list names every pixel in raster or in tile
//                                   order, where the slots of a partial tile outside the frame are pads.  The kernels are the list
//                                   kernels themselves: the round, the counter claim, the walk, the stacks and the launch exist once.  Both
//                                   forms write the same bytes; no atomic touches a record or a frame.
//
// k_prog_select<MASK_ONLY>          one thread per pixel, 256 threads = one 16x16 tile.  The own flags (prog_noisy) of the tile and a
//                                   one-pixel apron are staged in LDS (18 x 18 bytes; outside the frame: quiet), then every thread takes
//                                   its class from LDS (prog_classify), writes the class byte and appends a selected pixel to the list as
//                                   k_adaptive_select does (wave_append, brt_wave.h): one ballot and one atomicAdd per wave on the count
//                                   word, plain vector stores.
#include <hip/hip_runtime.h>

#include "brt_pixels_dev.h"
#include "brt_progressive.h"

namespace brt {

namespace {

// the value of a pixel with n samples and the colour sum `sum` (raytrace.wgsl:169, :122)
BRT_DEV float4 prog_value(f3 sum, uint32_t n) {
    if (n == 0u) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float nf = (float)n;
    return make_float4(sum.x / nf, sum.y / nf, sum.z / nf, 1.0f);
}

}  // namespace

struct ProgStart {
    struct Lane {
        float m1, m2;          // of the lane's pixel
        uint32_t rays;         // of the lane's pixel
        uint32_t samples;      // the lane has run, over all its pixels
    };
    // the pixel entry i names; kListPad: none, and nothing is refused
    static BRT_DEV uint32_t pixel_of(const FrameParams& fp, const PixelsArgs& pa, uint32_t i, const ProgSample& pg) {
        if (pa.pixels) return pa.pixels[i];
        if (pg.order == 0u) return i;
        const uint32_t tiles_x = (fp.width + 7u) >> 3, tile = i >> 6, t = i & 63u;
        const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const uint32_t px = tx * 8u + (t & 7u), py = ty * 8u + (t >> 3);
        return (px < fp.width && py < fp.height) ? py * fp.width + px : kListPad;
    }
    static constexpr bool pads() { return true; }      // (the slots of a partial tile outside the frame, tile order)
    static BRT_DEV void refuse(const PixelsArgs&, uint32_t, const ProgSample&) {}
    // the pixel p from its record {sum.r, sum.g, sum.b, m1} {m2, rng, n, rays}: false if the record has the target's samples already (its
    // value is stored, the record untouched)
    static BRT_DEV bool begin(const FrameParams& fp, const PixelsArgs& pa, uint32_t i, uint32_t p, PixelState& ps, Lane& lane, const ProgSample& pg) {
        const uint4* r = reinterpret_cast<const uint4*>(pg.state + p);
        const uint4 a = r[0], b = r[1];
        const f3 sum = mk3(__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z));
        const uint32_t n = b.z;
        if (n >= pg.target) {
            if (stores(pa)) pixels_store(pa, i, p, prog_value(sum, n));
            return false;
        }
        pixels_begin(fp, p, ps);
        lane.m1 = 0.0f;
        lane.m2 = 0.0f;
        lane.rays = 0u;
        if (n != 0u) {
            ps.sum = sum;
            ps.rng = b.y;
            ps.sample = n;
            lane.m1 = __uint_as_float(a.w);
            lane.m2 = __uint_as_float(b.x);
            lane.rays = b.w;
        }
        return true;
    }
    static BRT_DEV bool begins_ended(const FrameParams&, const ProgSample&) { return false; }      // (begin has said so)
    static BRT_DEV uint32_t target(const FrameParams&, const ProgSample& pg) { return pg.target; }
    // a sample starts as k_trace_simple's does (raytrace.wgsl:162, :175-186)
    static BRT_DEV void sample(const FrameParams& fp, const PixelState& ps, uint32_t& rng, f3& o, f3& d, const ProgSample&) {
        d = camera_ray_dir(fp, ps.ndc0x, ps.ndc0y, rng);
        o = mk3(fp.cam_pos[0], fp.cam_pos[1], fp.cam_pos[2]);
    }
    static BRT_DEV void walked(Lane& lane) { lane.rays++; }
    static BRT_DEV void sampled(Lane& lane, f3 color) {
        prog_moments(lane.m1, lane.m2, color.x, color.y, color.z);
        lane.samples++;
    }
    static BRT_DEV void end(const FrameParams&, uint32_t p, const PixelState& ps, const Lane& lane, const ProgSample& pg) {
        uint4* r = reinterpret_cast<uint4*>(pg.state + p);
        r[0] = make_uint4(__float_as_uint(ps.sum.x), __float_as_uint(ps.sum.y), __float_as_uint(ps.sum.z), __float_as_uint(lane.m1));
        r[1] = make_uint4(__float_as_uint(lane.m2), ps.rng, ps.sample, lane.rays);
    }
    static constexpr bool stores(const PixelsArgs& pa) { return pa.out != nullptr; }      // (args.out null: no value is stored)
    static BRT_DEV float4 value(const FrameParams&, const PixelState& ps, const ProgSample&) { return prog_value(ps.sum, ps.sample); }
    static BRT_DEV void count(const PixelsArgs& pa, uint32_t rays, uint32_t refused, const Lane& lane, const ProgSample& pg) {
        pixels_count(pa, rays, refused);
        if (!pg.samples) return;
        const uint32_t samples = wave_sum(lane.samples);
        if (lane_id() == 0u && samples) atomicAdd(pg.samples, (unsigned long long)samples);
    }
};

namespace {

// ---- selection -----------------------------------------------------------------------------------------------------------------------

constexpr uint32_t kTile = 16u, kSpan = kTile + 2u;      // the tile and its one-pixel apron

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
    if constexpr (!MASK_ONLY) wave_append(sl.count, sl.list, cls != 0u, p);
}

}  // namespace

// ---- host-callable launchers ---------------------------------------------------------------------------------------------------------

hipError_t launch_prog_sample(const PixelsLaunch& pl, const ProgSample& pg) {
    if (pl.args.n_pixels == 0u) return hipSuccess;
    if (!pg.state || pg.target == 0u || pg.target > kProgMaxSamples || pg.order > 1u || pl.frame.policy_flags != 0u || !pl.args.scatter)
        return hipErrorInvalidValue;
    return launch_list<ProgStart>(pl, true, pg);
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
