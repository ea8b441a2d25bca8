// brt_api_envmap.cpp -- reflection probes (brt_envmap.h, brt_envmap.hip; DESIGN.md "Reflection probes") on the first device: a cube map
// traced from one position and its mip chain prefiltered by roughness.  The texels' rays are radiance entries and are traced by the
// radiance kernels as they are (brt_api_radiance.cpp radiance_enqueue); the skeleton of a bake export, its chunk loop, the cached tap
// tables, streams, ordering behind ev_q, the staging rule and the round trip of the host form's buffer are those of every list call
// (brt_frame.h: bake_call, bake_call_host over host_round_trip, bake_chunks, cached_table, staged, list_step_run, device_aligned); the stats are the probe bakes' (bake_stats).  Here: the checks, the
// tap tables' maths, the argument packing, the level loop and the host twins.
#include "brt_envmap.h"
#include "brt_frame.h"

using namespace brt;

namespace {

int32_t size_check(brt_ctx* ctx, uint32_t size, const char* what) {
    if (size < 1u || size > kEnvmapMaxSize) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, std::string(what) + " must be in [1, 4096]");
    return BRT_OK;
}

int32_t taps_count_check(brt_ctx* ctx, uint32_t n_taps) {
    if (n_taps < 1u || n_taps > kEnvmapMaxTaps) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "n_taps must be in [1, 4096]");
    return BRT_OK;
}

// The tap table: float64, rounded to f32 at the end; the only place that computes it (the device reads a table uploaded from here).
void envmap_taps(uint32_t kind, float roughness, uint32_t n, float* out) {
    for (uint32_t i = 0; i < n; i++) {
        uint32_t r = i;
        r = (r << 16) | (r >> 16);
        r = ((r & 0x00ff00ffu) << 8) | ((r & 0xff00ff00u) >> 8);
        r = ((r & 0x0f0f0f0fu) << 4) | ((r & 0xf0f0f0f0u) >> 4);
        r = ((r & 0x33333333u) << 2) | ((r & 0xccccccccu) >> 2);
        r = ((r & 0x55555555u) << 1) | ((r & 0xaaaaaaaau) >> 1);
        const double xi1 = ((double)i + 0.5) / (double)n, xi2 = (double)r * (1.0 / 4294967296.0);
        const double phi = kTwoPi * xi1, cp = std::cos(phi), sp = std::sin(phi);
        double lx, ly, lz, w;
        if (kind == ENVMAP_TAPS_GGX) {
            const double a = (double)roughness * (double)roughness;
            const double ct = std::sqrt((1.0 - xi2) / (1.0 + (a * a - 1.0) * xi2));
            const double st = std::sqrt(std::max(0.0, 1.0 - ct * ct));
            const double hx = st * cp, hy = st * sp, hz = ct;
            lx = 2.0 * hz * hx;
            ly = 2.0 * hz * hy;
            lz = 2.0 * hz * hz - 1.0;
            w = std::max(lz, 0.0);
        } else {
            const double rr = std::sqrt(xi2);
            lx = rr * cp;
            ly = rr * sp;
            lz = std::sqrt(1.0 - xi2);
            w = 1.0;
        }
        out[4u * (size_t)i] = (float)lx;
        out[4u * (size_t)i + 1u] = (float)ly;
        out[4u * (size_t)i + 2u] = (float)lz;
        out[4u * (size_t)i + 3u] = (float)w;
    }
}

// the roughness of level l of a chain of `levels` levels: an f32 divide
float level_roughness(uint32_t l, uint32_t levels) { return (float)l / (float)(levels - 1u); }

int32_t rays_enqueue(brt_ctx* ctx, hipStream_t stream, const float* position3, uint32_t seed, uint32_t size, uint32_t first, uint32_t n,
                     void* d_rays) {
    EnvmapRaysArgs a;
    for (uint32_t k = 0; k < 3u; k++) a.position[k] = position3[k];
    a.seed = seed;
    a.size = size;
    a.first = first;
    a.n = n;
    a.rays = static_cast<uint4*>(d_rays);
    HIP_TRY(ctx, launch_envmap_rays(a, stream));
    return BRT_OK;
}

int32_t resolve_enqueue(brt_ctx* ctx, hipStream_t stream, const void* d_results, uint32_t n, void* d_out, void* d_out16) {
    EnvmapResolveArgs a;
    a.results = static_cast<const float4*>(d_results);
    a.out = static_cast<float4*>(d_out);
    a.out16 = static_cast<uint2*>(d_out16);
    a.n = n;
    HIP_TRY(ctx, launch_envmap_resolve(a, stream));
    return BRT_OK;
}

int32_t downsample_enqueue(brt_ctx* ctx, hipStream_t stream, const void* d_src, uint32_t src_size, void* d_out) {
    EnvmapDownsampleArgs a;
    a.src = static_cast<const float4*>(d_src);
    a.out = static_cast<float4*>(d_out);
    a.src_size = src_size;
    HIP_TRY(ctx, launch_envmap_downsample(a, stream));
    return BRT_OK;
}

int32_t filter_enqueue(brt_ctx* ctx, hipStream_t stream, const void* d_src, uint32_t src_size, const void* d_taps, uint32_t n_taps,
                       uint32_t dst_size, void* d_out, uint32_t out_format) {
    EnvmapFilterArgs a;
    a.src = static_cast<const float4*>(d_src);
    a.taps = static_cast<const float4*>(d_taps);
    a.out = d_out;
    a.src_size = src_size;
    a.n_taps = n_taps;
    a.dst_size = dst_size;
    a.out_format = out_format;
    HIP_TRY(ctx, launch_envmap_filter(a, stream));
    return BRT_OK;
}

// what the two downsample exports check (device or host addresses alike)
int32_t downsample_check(brt_ctx* ctx, const void* src, uint32_t src_size, const void* out) {
    if (src_size < 2u || src_size > kEnvmapMaxSize || (src_size & 1u))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "src_size must be even and in [2, 4096]");
    if (!src || !out) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "src / out is null");
    if (overlaps(src, (size_t)envmap_texels(src_size) * 16u, out, (size_t)envmap_texels(src_size / 2u) * 16u))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "the buffers overlap");
    return BRT_OK;
}

// ... and the two filter exports
int32_t filter_check(brt_ctx* ctx, const void* src, uint32_t src_size, const void* taps, uint32_t n_taps, uint32_t dst_size, const void* out) {
    int32_t rc = size_check(ctx, src_size, "src_size");
    if (rc == BRT_OK) rc = size_check(ctx, dst_size, "dst_size");
    if (rc == BRT_OK) rc = taps_count_check(ctx, n_taps);
    if (rc != BRT_OK) return rc;
    if (!src || !taps || !out) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "src / taps / out is null");
    const size_t out_bytes_ = (size_t)envmap_texels(dst_size) * 16u;
    if (overlaps(out, out_bytes_, src, (size_t)envmap_texels(src_size) * 16u) || overlaps(out, out_bytes_, taps, (size_t)n_taps * 16u))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "the buffers overlap");
    return BRT_OK;
}

int32_t position_check(brt_ctx* ctx, const float* position3) {
    if (!position3) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "position3 is null");
    for (uint32_t k = 0; k < 3u; k++)
        if (!std::isfinite(position3[k])) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "the position must be finite");
    return BRT_OK;
}

// what both bakes check before anything is enqueued
int32_t envmap_bake_check(brt_ctx* ctx, const float* position3, uint32_t size, uint32_t levels, uint32_t samples, uint32_t bounces,
                          uint32_t n_taps, float origin_bound, const void* out) {
    int32_t rc = position_check(ctx, position3);
    if (rc != BRT_OK) return rc;
    if (size < 1u || size > kEnvmapMaxBakeSize || (size & (size - 1u)))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "size must be a power of two in [1, 1024]");
    uint32_t log2 = 0u;
    while ((size >> (log2 + 1u)) != 0u) log2++;
    if (levels < 1u || levels > log2 + 1u) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "levels must be in [1, log2(size) + 1]");
    if (samples < 1u || samples > 65535u) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "samples must be in [1, 65535]");
    if (bounces > 65535u) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "bounces must be in [0, 65535]");
    if ((rc = taps_count_check(ctx, n_taps)) != BRT_OK) return rc;
    if ((rc = origin_bound_check(ctx, origin_bound)) != BRT_OK) return rc;
    if (!out) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "out is null");
    if (!ctx->has_scene) return ctx_fail(ctx, BRT_ERR_NO_SCENE, "brt_upload_scene has not succeeded yet");
    if (ctx->policy_flags & kPolicyMask)
        return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, "reflection probes implement the default policy only (brt_set_policy)");
    return BRT_OK;
}

// The device tables of the levels 1 .. levels - 1 of a chain (GGX, roughness l / (levels - 1), n_taps taps each, level l at record
// (l - 1) * n_taps) for work on `stream`, which is then behind ev_q.  Kept per context by (levels, n_taps) (cached_table); a chain of
// one level has no table.
int32_t envmap_tables(brt_ctx* ctx, DeviceCtx& dc, uint32_t levels, uint32_t n_taps, hipStream_t stream) {
    if (levels < 2u) { HIP_TRY(ctx, hipStreamWaitEvent(stream, dc.ev_q, 0)); return BRT_OK; }
    return cached_table(ctx, dc, dc.envmap_taps, (uint64_t)levels << 32 | n_taps, stream, [&](std::vector<float>& h) {
        h.resize((size_t)(levels - 1u) * n_taps * 4u);
        for (uint32_t l = 1; l < levels; l++)
            envmap_taps(ENVMAP_TAPS_GGX, level_roughness(l, levels), n_taps, h.data() + (size_t)(l - 1u) * n_taps * 4u);
    });
}

// The bake into the DEVICE buffer d_out on `stream`: the texels in chunks of BRT_PROBE_CHUNK_RAYS entries, generate -> the radiance
// launch -> resolve; then per level the box level and its filter.  All behind ev_q, which the last step records.  The lists are staged
// in d_qrays / d_qhits, the box levels (and the f32 level 0 of an RGBA16F bake) in d_envmap (one user at a time: `staged`).
int32_t envmap_bake_enqueue(brt_ctx* ctx, DeviceCtx& dc, hipStream_t stream, const float* position3, uint32_t seed, uint32_t size,
                            uint32_t levels, uint32_t samples, uint32_t bounces, uint32_t n_taps, void* d_out, uint32_t out_format,
                            bool counted, BakeRun* run) {
    const bool half = out_format == BRT_FLAG_OUT_RGBA16F;
    const size_t texel = half ? 8u : 16u;
    const uint32_t n0 = envmap_texels(size);
    const uint32_t per_chunk = std::min(std::max(ctx->knobs[K_PROBE_CHUNK_RAYS], 1u), n0);
    const size_t list_bytes = (size_t)per_chunk * 32u;
    // d_envmap: [level 0 in f32, if the target is not] [box level 1] .. [box level levels - 1]
    const size_t lvl0_bytes = half ? (size_t)n0 * 16u : 0u;
    const size_t work_bytes = std::max<size_t>(lvl0_bytes + (size_t)(envmap_level_offset(size, levels) - n0) * 16u, 16u);
    int32_t rc = staged(ctx, dc, {{&dc.d_qrays, &dc.qrays_cap, list_bytes}, {&dc.d_qhits, &dc.qhits_cap, list_bytes},
                                  {&dc.d_envmap, &dc.envmap_cap, work_bytes}});
    if (rc == BRT_OK) rc = envmap_tables(ctx, dc, levels, n_taps, stream);
    if (rc != BRT_OK) return rc;
    char* lvl0 = half ? dc.d_envmap : static_cast<char*>(d_out);
    rc = bake_chunks(ctx, dc, stream, n0, per_chunk, counted, run, [&](uint32_t first, uint32_t n) {
        int32_t r = rays_enqueue(ctx, stream, position3, seed, size, first, n, dc.d_qrays);
        if (r == BRT_OK) r = radiance_enqueue(ctx, dc, stream, dc.d_qrays, n, samples, bounces, dc.d_qhits, counted, &run->rl);
        if (r == BRT_OK) r = resolve_enqueue(ctx, stream, dc.d_qhits, n, lvl0 + (size_t)first * 16u,
                                             half ? static_cast<char*>(d_out) + (size_t)first * 8u : nullptr);
        return r;
    });
    if (rc != BRT_OK) return rc;
    const char* box = lvl0;
    char* next = dc.d_envmap + lvl0_bytes;
    for (uint32_t l = 1; l < levels; l++) {
        const uint32_t s = size >> l;
        rc = downsample_enqueue(ctx, stream, box, s * 2u, next);
        if (rc == BRT_OK) rc = filter_enqueue(ctx, stream, next, s, dc.envmap_taps.d + (size_t)(l - 1u) * n_taps * 4u, n_taps, s,
                                              static_cast<char*>(d_out) + (size_t)envmap_level_offset(size, l) * texel, out_format);
        if (rc != BRT_OK) return rc;
        box = next;
        next += (size_t)envmap_texels(s) * 16u;
    }
    HIP_TRY(ctx, hipEventRecord(dc.ev_q, stream));
    return BRT_OK;
}

// after the reach step: the position lies within the tree's bound, as every entry of the cube would be judged
int32_t position_reach_check(brt_ctx* ctx, const float* position3) {
    const float norm1 = (std::fabs(position3[0]) + std::fabs(position3[1])) + std::fabs(position3[2]);
    if (norm1 > query_bound_of(ctx))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "the position lies beyond the resident tree's bound (brt_query_origin_bound)");
    return BRT_OK;
}

template <class T>
void store_texel(void* out, size_t i, const T& v) { std::memcpy(static_cast<char*>(out) + i * sizeof(T), &v, sizeof(T)); }

}  // namespace

extern "C" {

int32_t brt_host_envmap_directions(uint32_t size, float* out_xyz) {
    return guard(nullptr, [&]() -> int32_t {
    const int32_t rc = size_check(nullptr, size, "size");
    if (rc != BRT_OK) return rc;
    if (!out_xyz) return fail(BRT_ERR_INVALID_ARGUMENT, "out_xyz is null");
    for (uint32_t i = 0; i < envmap_texels(size); i++) {
        uint32_t face, x, y;
        float d[3];
        envmap_texel_of(size, i, &face, &x, &y);
        envmap_direction(size, face, x, y, d);
        std::memcpy(reinterpret_cast<char*>(out_xyz) + (size_t)i * 12u, d, 12u);
    }
    return BRT_OK;
    });
}

int32_t brt_host_envmap_taps(uint32_t kind, float roughness, uint32_t n_taps, void* out) {
    return guard(nullptr, [&]() -> int32_t {
    if (kind > ENVMAP_TAPS_COSINE) return fail(BRT_ERR_INVALID_ARGUMENT, "kind must be BRT_ENVMAP_TAPS_GGX or BRT_ENVMAP_TAPS_COSINE");
    if (kind == ENVMAP_TAPS_GGX && !(roughness >= 0.0f && roughness <= 1.0f)) return fail(BRT_ERR_INVALID_ARGUMENT, "roughness must be in [0, 1]");
    const int32_t rc = taps_count_check(nullptr, n_taps);
    if (rc != BRT_OK) return rc;
    if (!out) return fail(BRT_ERR_INVALID_ARGUMENT, "out is null");
    std::vector<float> t((size_t)n_taps * 4u);
    envmap_taps(kind, roughness, n_taps, t.data());
    std::memcpy(out, t.data(), t.size() * sizeof(float));
    return BRT_OK;
    });
}

int32_t brt_host_envmap_downsample(const void* src, uint32_t src_size, void* out) {
    return guard(nullptr, [&]() -> int32_t {
    const int32_t rc = downsample_check(nullptr, src, src_size, out);
    if (rc != BRT_OK) return rc;
    for (uint32_t i = 0; i < envmap_texels(src_size / 2u); i++) store_texel(out, i, envmap_box(src, src_size, i));
    return BRT_OK;
    });
}

int32_t brt_host_envmap_filter(const void* src, uint32_t src_size, const void* taps, uint32_t n_taps, uint32_t dst_size, void* out) {
    return guard(nullptr, [&]() -> int32_t {
    const int32_t rc = filter_check(nullptr, src, src_size, taps, n_taps, dst_size, out);
    if (rc != BRT_OK) return rc;
    for (uint32_t i = 0; i < envmap_texels(dst_size); i++) store_texel(out, i, envmap_filter(src, src_size, taps, n_taps, dst_size, i));
    return BRT_OK;
    });
}

int32_t brt_envmap_rays_device(brt_ctx* ctx, const float* position3, uint32_t seed, uint32_t size, void* d_rays, void* hip_stream,
                               uint32_t flags) {
    return ctx_guard(ctx, [&]() -> int32_t {
    int32_t rc = caller_stream_flags_check(ctx, flags);
    if (rc == BRT_OK) rc = position_check(ctx, position3);
    if (rc == BRT_OK) rc = size_check(ctx, size, "size");
    if (rc != BRT_OK) return rc;
    if (!d_rays) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "null device pointer");
    if ((rc = device_aligned(ctx, {d_rays})) != BRT_OK) return rc;
    return list_step_run(ctx, hip_stream, flags, [&](DeviceCtx&, hipStream_t stream) {
        return rays_enqueue(ctx, stream, position3, seed, size, 0u, envmap_texels(size), d_rays);
    });
    });
}

int32_t brt_envmap_resolve_device(brt_ctx* ctx, const void* d_results, uint32_t size, void* d_out, void* hip_stream, uint32_t flags) {
    return ctx_guard(ctx, [&]() -> int32_t {
    int32_t rc = caller_stream_flags_check(ctx, flags);
    if (rc == BRT_OK) rc = size_check(ctx, size, "size");
    if (rc != BRT_OK) return rc;
    if (!d_results || !d_out) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "null device pointer");
    if (overlaps(d_results, (size_t)envmap_texels(size) * 32u, d_out, (size_t)envmap_texels(size) * 16u))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "the buffers overlap");
    if ((rc = device_aligned(ctx, {d_results, d_out})) != BRT_OK) return rc;
    return list_step_run(ctx, hip_stream, flags, [&](DeviceCtx&, hipStream_t stream) {
        return resolve_enqueue(ctx, stream, d_results, envmap_texels(size), d_out, nullptr);
    });
    });
}

int32_t brt_envmap_downsample_device(brt_ctx* ctx, const void* d_src, uint32_t src_size, void* d_out, void* hip_stream, uint32_t flags) {
    return ctx_guard(ctx, [&]() -> int32_t {
    int32_t rc = caller_stream_flags_check(ctx, flags);
    if (rc == BRT_OK) rc = downsample_check(ctx, d_src, src_size, d_out);
    if (rc == BRT_OK) rc = device_aligned(ctx, {d_src, d_out});
    if (rc != BRT_OK) return rc;
    return list_step_run(ctx, hip_stream, flags, [&](DeviceCtx&, hipStream_t stream) {
        return downsample_enqueue(ctx, stream, d_src, src_size, d_out);
    });
    });
}

int32_t brt_envmap_filter_device(brt_ctx* ctx, const void* d_src, uint32_t src_size, const void* d_taps, uint32_t n_taps, uint32_t dst_size,
                                 void* d_out, void* hip_stream, uint32_t flags) {
    return ctx_guard(ctx, [&]() -> int32_t {
    int32_t rc = caller_stream_flags_check(ctx, flags);
    if (rc == BRT_OK) rc = filter_check(ctx, d_src, src_size, d_taps, n_taps, dst_size, d_out);
    if (rc == BRT_OK) rc = device_aligned(ctx, {d_src, d_taps, d_out});
    if (rc != BRT_OK) return rc;
    return list_step_run(ctx, hip_stream, flags, [&](DeviceCtx&, hipStream_t stream) {
        return filter_enqueue(ctx, stream, d_src, src_size, d_taps, n_taps, dst_size, d_out, BRT_FLAG_OUT_RGBA32F);
    });
    });
}

int32_t brt_bake_envmap_device(brt_ctx* ctx, const float* position3, uint32_t seed, uint32_t size, uint32_t levels, uint32_t samples,
                               uint32_t bounces, uint32_t n_taps, float origin_bound, void* d_out, void* hip_stream, uint32_t flags,
                               uint64_t* out_stats8) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (flags & ~(uint32_t)(BRT_FLAG_CALLER_STREAM | BRT_FLAG_OUT_RGBA16F))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "flags: BRT_FLAG_CALLER_STREAM and BRT_FLAG_OUT_RGBA16F only");
    int32_t rc = envmap_bake_check(ctx, position3, size, levels, samples, bounces, n_taps, origin_bound, d_out);
    if (rc == BRT_OK) rc = device_aligned(ctx, {d_out});
    if (rc != BRT_OK) return rc;
    const float pos[3] = {position3[0], position3[1], position3[2]};
    return bake_call(ctx, origin_bound, hip_stream, flags & BRT_FLAG_CALLER_STREAM, out_stats8,
                     [&](DeviceCtx& dc, hipStream_t stream, bool counted, BakeRun* run) {
        const int32_t r = position_reach_check(ctx, pos);
        if (r != BRT_OK) return r;
        return envmap_bake_enqueue(ctx, dc, stream, pos, seed, size, levels, samples, bounces, n_taps, d_out, flags & BRT_FLAG_OUT_MASK,
                                   counted, run);
    });
    });
}

int32_t brt_bake_envmap(brt_ctx* ctx, const float* position3, uint32_t seed, uint32_t size, uint32_t levels, uint32_t samples,
                        uint32_t bounces, uint32_t n_taps, float origin_bound, void* out, uint32_t flags, uint64_t* out_stats8) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (flags & ~(uint32_t)BRT_FLAG_OUT_RGBA16F) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "flags: BRT_FLAG_OUT_RGBA16F only");
    const int32_t rc = envmap_bake_check(ctx, position3, size, levels, samples, bounces, n_taps, origin_bound, out);
    if (rc != BRT_OK) return rc;
    const float pos[3] = {position3[0], position3[1], position3[2]};
    const size_t bytes = (size_t)envmap_level_offset(size, levels) * (flags == BRT_FLAG_OUT_RGBA16F ? 8u : 16u);
    return bake_call_host(ctx, origin_bound, {{nullptr, out, bytes}}, out_stats8,
                          [&](DeviceCtx& dc, hipStream_t stream, bool counted, BakeRun* run, char* const* d) {
        return envmap_bake_enqueue(ctx, dc, stream, pos, seed, size, levels, samples, bounces, n_taps, d[0], flags, counted, run);
    }, [&] { return position_reach_check(ctx, pos); });
    });
}

}  // extern "C"
