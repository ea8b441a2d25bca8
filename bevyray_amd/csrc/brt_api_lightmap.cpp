// brt_api_lightmap.cpp -- lightmaps (brt_lightmap.h, brt_lightmap.hip; DESIGN.md "Lightmaps") on the first device: per surface point the
// mean radiance over the cosine-weighted hemisphere of its normal, resolved to the texels of a chart and dilated past the chart's edge.
// The rays are radiance entries and are traced by the radiance kernels as they are (brt_api_radiance.cpp radiance_enqueue); the skeleton
// of a bake export, its chunk loop, the cached direction table, streams, ordering behind ev_q, the staging rule and the round trip of the
// host form's buffers are those of every list call (brt_frame.h: bake_call, bake_call_host over host_round_trip, bake_chunks,
// cached_table, staged, list_step_run, device_aligned, flags_check); the stats are the probe bakes' (bake_stats).  Here: the checks, the direction table's maths, the argument packing, the pass loop and the host twins.
#include "brt_frame.h"
#include "brt_lightmap.h"

using namespace brt;

namespace {

constexpr uint32_t kMaxEntries = 0x7fff0000u;        // of one radiance list (radiance_check)
constexpr double kGolden = 0.6180339887498949;       // (sqrt(5) - 1) / 2
constexpr double kPi = 3.141592653589793;

// Direction k of the table of n: the unit disc stratified by radius and turned by the golden angle, lifted onto the hemisphere about +z
// (cosine-weighted, equal weights).  float64, rounded to f32 at the end; the only place that computes it.
void lightmap_direction(uint32_t n, uint32_t k, float out[3]) {
    const double u = ((double)k + 0.5) / (double)n;
    const double r = std::sqrt(u);
    const double t = (double)k * kGolden;
    const double phi = kTwoPi * (t - std::floor(t));
    out[0] = (float)(r * std::cos(phi));
    out[1] = (float)(r * std::sin(phi));
    out[2] = (float)std::sqrt(1.0 - u);
}

int32_t dirs_check(brt_ctx* ctx, uint32_t n_dirs) {
    if (n_dirs < 1u || n_dirs > kLightmapMaxDirs) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "n_dirs must be in [1, 65536]");
    return BRT_OK;
}

int32_t image_check(brt_ctx* ctx, uint32_t width, uint32_t height, uint32_t passes, uint32_t wrap_u) {
    if (width < 1u || width > kLightmapMaxSize || height < 1u || height > kLightmapMaxSize)
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "width and height must be in [1, 16384]");
    if (passes > kLightmapMaxPasses) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "passes must be in [0, 64]");
    if (wrap_u > 1u) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "wrap_u must be 0 or 1");
    return BRT_OK;
}

size_t texel_bytes(uint32_t flags) { return (flags & BRT_FLAG_OUT_RGBA16F) ? 8u : 16u; }

// The device table of n_dirs directions {x, y, z, 0} for work on `stream`, which is then behind ev_q: kept per context by n_dirs
int32_t lightmap_table(brt_ctx* ctx, DeviceCtx& dc, uint32_t n_dirs, hipStream_t stream) {
    return cached_table(ctx, dc, dc.lightmap_dirs, n_dirs, stream, [&](std::vector<float>& h) {
        h.assign((size_t)n_dirs * 4u, 0.0f);
        for (uint32_t k = 0; k < n_dirs; k++) lightmap_direction(n_dirs, k, h.data() + (size_t)k * 4u);
    });
}

int32_t rays_enqueue(brt_ctx* ctx, DeviceCtx& dc, hipStream_t stream, const void* d_points, uint32_t n_points, uint32_t n_dirs, void* d_rays) {
    LightmapRaysArgs a;
    a.points = static_cast<const float4*>(d_points);
    a.dirs = reinterpret_cast<const float4*>(dc.lightmap_dirs.d);
    a.rays = static_cast<uint4*>(d_rays);
    a.n_points = n_points;
    a.n_dirs = n_dirs;
    HIP_TRY(ctx, launch_lightmap_rays(a, stream));
    return BRT_OK;
}

int32_t resolve_enqueue(brt_ctx* ctx, hipStream_t stream, const void* d_results, const void* d_points, uint32_t n_points, uint32_t n_dirs,
                        void* d_out, void* d_info, bool f16) {
    LightmapResolveArgs a;
    a.results = static_cast<const float4*>(d_results);
    a.points = static_cast<const float4*>(d_points);
    a.out = d_out;
    a.info = static_cast<uint2*>(d_info);
    a.n_points = n_points;
    a.n_dirs = n_dirs;
    a.f16 = f16 ? 1u : 0u;
    HIP_TRY(ctx, launch_lightmap_resolve(a, stream));
    return BRT_OK;
}

// The passes over the f32 image d_src into d_out (f16: as RGBA16F): pass i writes ping[i & 1], the last one d_out; no pass at all is one
// launch that copies (and converts).  ping[0] must not be d_src; ping[1] may be.
int32_t dilate_enqueue(brt_ctx* ctx, hipStream_t stream, const void* d_src, char* const ping[2], uint32_t width, uint32_t height,
                       uint32_t passes, uint32_t wrap_u, void* d_out, bool f16) {
    LightmapDilateArgs a;
    a.width = width;
    a.height = height;
    a.wrap_u = wrap_u;
    a.fill = passes ? 1u : 0u;
    const void* src = d_src;
    for (uint32_t i = 0; i < std::max(passes, 1u); i++) {
        const bool last = i + 1u >= passes;
        a.src = static_cast<const float4*>(src);
        a.out = last ? d_out : static_cast<void*>(ping[i & 1u]);
        a.f16 = last && f16 ? 1u : 0u;
        HIP_TRY(ctx, launch_lightmap_dilate(a, stream));
        src = a.out;
    }
    return BRT_OK;
}

// what both bakes check before anything is enqueued (device or host addresses alike)
int32_t lightmap_bake_check(brt_ctx* ctx, const void* points, uint32_t width, uint32_t height, uint32_t n_dirs, uint32_t bounces,
                            uint32_t passes, uint32_t wrap_u, float origin_bound, const void* out, const void* info, uint32_t flags) {
    int32_t rc = image_check(ctx, width, height, passes, wrap_u);
    if (rc == BRT_OK) rc = dirs_check(ctx, n_dirs);
    if (rc != BRT_OK) return rc;
    if (bounces > 65535u) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "bounces must be in [0, 65535]");
    if ((rc = origin_bound_check(ctx, origin_bound)) != BRT_OK) return rc;
    if (!points || !out) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "points / out is null");
    const size_t n = (size_t)width * height;
    if (overlaps(points, n * 32u, out, n * texel_bytes(flags)) ||
        (info && (overlaps(points, n * 32u, info, n * 8u) || overlaps(out, n * texel_bytes(flags), info, n * 8u))))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "the buffers overlap");
    if (!ctx->has_scene) return ctx_fail(ctx, BRT_ERR_NO_SCENE, "brt_upload_scene has not succeeded yet");
    if (ctx->policy_flags & kPolicyMask)
        return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, "lightmaps implement the default policy only (brt_set_policy)");
    return BRT_OK;
}

// The bake of DEVICE buffers on `stream`: in chunks of whole points (bake_chunks), generate -> the radiance launch -> resolve; then the
// passes.  All behind ev_q, which the last step records.  The lists are staged in d_qrays / d_qhits, the resolved f32 image and the
// second image of the passes in d_lightmap (one user at a time: `staged`); a bake without passes resolves into d_out itself.
int32_t lightmap_bake_enqueue(brt_ctx* ctx, DeviceCtx& dc, hipStream_t stream, const void* d_points, uint32_t width, uint32_t height,
                              uint32_t n_dirs, uint32_t bounces, uint32_t passes, uint32_t wrap_u, void* d_out, void* d_info, uint32_t flags,
                              bool counted, BakeRun* run) {
    const bool f16 = (flags & BRT_FLAG_OUT_RGBA16F) != 0u;
    const uint32_t n_points = width * height;
    const uint32_t chunk_rays = std::min(std::max(ctx->knobs[K_PROBE_CHUNK_RAYS], 1u), kMaxEntries);
    const uint32_t per_chunk = std::min(std::max(1u, chunk_rays / n_dirs), n_points);
    const size_t list_bytes = (size_t)per_chunk * n_dirs * 32u, image_bytes = (size_t)n_points * 16u;
    int32_t rc = staged(ctx, dc, {{&dc.d_qrays, &dc.qrays_cap, list_bytes}, {&dc.d_qhits, &dc.qhits_cap, list_bytes},
                                  {&dc.d_lightmap, &dc.lightmap_cap, passes ? 2u * image_bytes : 16u}});
    if (rc == BRT_OK) rc = lightmap_table(ctx, dc, n_dirs, stream);
    if (rc != BRT_OK) return rc;
    char* resolved = passes ? dc.d_lightmap : static_cast<char*>(d_out);
    const size_t texel = passes ? 16u : texel_bytes(flags);
    rc = bake_chunks(ctx, dc, stream, n_points, per_chunk, counted, run, [&](uint32_t first, uint32_t n) {
        const char* pts = static_cast<const char*>(d_points) + (size_t)first * 32u;
        int32_t r = rays_enqueue(ctx, dc, stream, pts, n, n_dirs, dc.d_qrays);
        if (r == BRT_OK) r = radiance_enqueue(ctx, dc, stream, dc.d_qrays, n * n_dirs, 1u, bounces, dc.d_qhits, counted, &run->rl);
        if (r == BRT_OK) r = resolve_enqueue(ctx, stream, dc.d_qhits, pts, n, n_dirs, resolved + (size_t)first * texel,
                                             d_info ? static_cast<char*>(d_info) + (size_t)first * 8u : nullptr, !passes && f16);
        return r;
    });
    if (rc != BRT_OK || !passes) return rc;
    char* const ping[2] = {dc.d_lightmap + image_bytes, dc.d_lightmap};
    rc = dilate_enqueue(ctx, stream, dc.d_lightmap, ping, width, height, passes, wrap_u, d_out, f16);
    if (rc != BRT_OK) return rc;
    HIP_TRY(ctx, hipEventRecord(dc.ev_q, stream));
    return BRT_OK;
}

// what the rays and resolve exports check of a list of n_points x n_dirs entries
int32_t list_check(brt_ctx* ctx, uint32_t n_points, uint32_t n_dirs) {
    const int32_t rc = dirs_check(ctx, n_dirs);
    if (rc != BRT_OK) return rc;
    if ((uint64_t)n_points * n_dirs > kMaxEntries) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "n_points * n_dirs too large");
    return BRT_OK;
}

template <class T>
void store16(void* out, size_t i, const T& v) { std::memcpy(static_cast<char*>(out) + i * 16u, &v, 16u); }

}  // namespace

extern "C" {

int32_t brt_host_lightmap_directions(uint32_t n_dirs, float* out_xyz) {
    return guard(nullptr, [&]() -> int32_t {
    const int32_t rc = dirs_check(nullptr, n_dirs);
    if (rc != BRT_OK) return rc;
    if (!out_xyz) return fail(BRT_ERR_INVALID_ARGUMENT, "out_xyz is null");
    for (uint32_t k = 0; k < n_dirs; k++) {
        float d[3];
        lightmap_direction(n_dirs, k, d);
        std::memcpy(reinterpret_cast<char*>(out_xyz) + (size_t)k * 12u, d, 12u);
    }
    return BRT_OK;
    });
}

int32_t brt_host_lightmap_ray(const void* point32, uint32_t n_dirs, uint32_t k, void* out_ray32) {
    return guard(nullptr, [&]() -> int32_t {
    const int32_t rc = dirs_check(nullptr, n_dirs);
    if (rc != BRT_OK) return rc;
    if (k >= n_dirs) return fail(BRT_ERR_INVALID_ARGUMENT, "k must be below n_dirs");
    if (!point32 || !out_ray32) return fail(BRT_ERR_INVALID_ARGUMENT, "null pointer");
    if (overlaps(point32, 32u, out_ray32, 32u)) return fail(BRT_ERR_INVALID_ARGUMENT, "the buffers overlap");
    const float4 p0 = lightmap_load16(point32, 0u), p1 = lightmap_load16(point32, 1u);
    float l[3];
    lightmap_direction(n_dirs, k, l);
    uint4 r0, r1;
    lightmap_entry(p0, lightmap_frame(p0, p1), make_float4(l[0], l[1], l[2], 0.0f), k, &r0, &r1);
    store16(out_ray32, 0u, r0);
    store16(out_ray32, 1u, r1);
    return BRT_OK;
    });
}

int32_t brt_host_lightmap_sphere_points(const float* centre3, float radius, uint32_t seed, float offset, uint32_t width, uint32_t height,
                                        void* out_points) {
    return guard(nullptr, [&]() -> int32_t {
    const int32_t rc = image_check(nullptr, width, height, 0u, 0u);
    if (rc != BRT_OK) return rc;
    if (!centre3 || !out_points) return fail(BRT_ERR_INVALID_ARGUMENT, "null pointer");
    if (!std::isfinite(centre3[0]) || !std::isfinite(centre3[1]) || !std::isfinite(centre3[2]) || !std::isfinite(radius) || !(radius > 0.0f) ||
        !std::isfinite(offset) || !(offset >= 0.0f))
        return fail(BRT_ERR_INVALID_ARGUMENT, "the centre must be finite, the radius finite and > 0, the offset finite and >= 0");
    for (uint32_t y = 0; y < height; y++) {
        const double theta = kPi * (((double)y + 0.5) / (double)height);
        for (uint32_t x = 0; x < width; x++) {
            const double phi = kTwoPi * (((double)x + 0.5) / (double)width);
            const double n[3] = {std::sin(theta) * std::cos(phi), std::cos(theta), std::sin(theta) * std::sin(phi)};
            const uint32_t i = y * width + x;
            float rec[8];
            for (uint32_t c = 0; c < 3u; c++) {
                rec[c] = (float)((double)centre3[c] + (double)radius * n[c]);
                rec[4u + c] = (float)n[c];
            }
            rec[3] = lightmap_float(seed + i * kLightmapSeedStep);
            rec[7] = offset;
            std::memcpy(static_cast<char*>(out_points) + (size_t)i * 32u, rec, 32u);
        }
    }
    return BRT_OK;
    });
}

int32_t brt_host_lightmap_dilate(const void* texels_f32, uint32_t width, uint32_t height, uint32_t passes, uint32_t wrap_u, void* out_f32) {
    return guard(nullptr, [&]() -> int32_t {
    const int32_t rc = image_check(nullptr, width, height, passes, wrap_u);
    if (rc != BRT_OK) return rc;
    if (!texels_f32 || !out_f32) return fail(BRT_ERR_INVALID_ARGUMENT, "texels / out is null");
    const size_t n = (size_t)width * height;
    if (overlaps(texels_f32, n * 16u, out_f32, n * 16u)) return fail(BRT_ERR_INVALID_ARGUMENT, "the buffers overlap");
    std::vector<float4> image[2];
    const void* src = texels_f32;
    for (uint32_t i = 0; i < passes; i++) {
        std::vector<float4>& dst = image[i & 1u];
        dst.resize(n);
        for (uint32_t y = 0; y < height; y++)
            for (uint32_t x = 0; x < width; x++) dst[(size_t)y * width + x] = lightmap_dilate_texel(src, width, height, wrap_u, 1u, x, y);
        src = dst.data();
    }
    std::memcpy(out_f32, src, n * 16u);
    return BRT_OK;
    });
}

int32_t brt_lightmap_rays_device(brt_ctx* ctx, const void* d_points, uint32_t n_points, uint32_t n_dirs, void* d_rays, void* hip_stream,
                                 uint32_t flags) {
    return ctx_guard(ctx, [&]() -> int32_t {
    int32_t rc = caller_stream_flags_check(ctx, flags);
    if (rc == BRT_OK) rc = list_check(ctx, n_points, n_dirs);
    if (rc != BRT_OK || n_points == 0u) return rc;
    if (!d_points || !d_rays) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "null device pointer");
    if (overlaps(d_points, (size_t)n_points * 32u, d_rays, (size_t)n_points * n_dirs * 32u))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "the buffers overlap");
    if ((rc = device_aligned(ctx, {d_points, d_rays})) != BRT_OK) return rc;
    return list_step_run(ctx, hip_stream, flags, [&](DeviceCtx& dc, hipStream_t stream) { return lightmap_table(ctx, dc, n_dirs, stream); },
                         [&](DeviceCtx& dc, hipStream_t stream) { return rays_enqueue(ctx, dc, stream, d_points, n_points, n_dirs, d_rays); });
    });
}

int32_t brt_lightmap_resolve_device(brt_ctx* ctx, const void* d_results, const void* d_points, uint32_t n_points, uint32_t n_dirs, void* d_out,
                                    void* d_info_or_null, void* hip_stream, uint32_t flags) {
    return ctx_guard(ctx, [&]() -> int32_t {
    int32_t rc = flags_check(ctx, flags, BRT_FLAG_CALLER_STREAM | BRT_FLAG_OUT_RGBA16F, "flags: BRT_FLAG_CALLER_STREAM and BRT_FLAG_OUT_RGBA16F only");
    if (rc == BRT_OK) rc = list_check(ctx, n_points, n_dirs);
    if (rc != BRT_OK || n_points == 0u) return rc;
    if (!d_results || !d_points || !d_out) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "null device pointer");
    const size_t res_bytes = (size_t)n_points * n_dirs * 32u, pts_bytes = (size_t)n_points * 32u, out_bytes_ = n_points * texel_bytes(flags);
    if (overlaps(d_out, out_bytes_, d_results, res_bytes) || overlaps(d_out, out_bytes_, d_points, pts_bytes) ||
        (d_info_or_null && (overlaps(d_info_or_null, (size_t)n_points * 8u, d_results, res_bytes) ||
                            overlaps(d_info_or_null, (size_t)n_points * 8u, d_points, pts_bytes) ||
                            overlaps(d_info_or_null, (size_t)n_points * 8u, d_out, out_bytes_))))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "the buffers overlap");
    if ((rc = device_aligned(ctx, {d_results, d_points, d_out, d_info_or_null})) != BRT_OK) return rc;
    return list_step_run(ctx, hip_stream, flags & BRT_FLAG_CALLER_STREAM, [&](DeviceCtx&, hipStream_t stream) {
        return resolve_enqueue(ctx, stream, d_results, d_points, n_points, n_dirs, d_out, d_info_or_null, (flags & BRT_FLAG_OUT_RGBA16F) != 0u);
    });
    });
}

int32_t brt_lightmap_dilate_device(brt_ctx* ctx, const void* d_texels_f32, uint32_t width, uint32_t height, uint32_t passes, uint32_t wrap_u,
                                   void* d_out, void* hip_stream, uint32_t flags) {
    return ctx_guard(ctx, [&]() -> int32_t {
    int32_t rc = flags_check(ctx, flags, BRT_FLAG_CALLER_STREAM | BRT_FLAG_OUT_RGBA16F, "flags: BRT_FLAG_CALLER_STREAM and BRT_FLAG_OUT_RGBA16F only");
    if (rc == BRT_OK) rc = image_check(ctx, width, height, passes, wrap_u);
    if (rc != BRT_OK) return rc;
    if (!d_texels_f32 || !d_out) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "null device pointer");
    const size_t image_bytes = (size_t)width * height * 16u;
    if (overlaps(d_texels_f32, image_bytes, d_out, (size_t)width * height * texel_bytes(flags)))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "the buffers overlap");
    if ((rc = device_aligned(ctx, {d_texels_f32, d_out})) != BRT_OK) return rc;
    // the images between the passes are the context's: behind ev_q like every staging buffer
    return list_step_run(ctx, hip_stream, flags & BRT_FLAG_CALLER_STREAM, [&](DeviceCtx& dc, hipStream_t stream) -> int32_t {
        const int32_t r = staged(ctx, dc, {{&dc.d_lightmap, &dc.lightmap_cap, passes > 1u ? 2u * image_bytes : 16u}});
        if (r != BRT_OK) return r;
        HIP_TRY(ctx, hipStreamWaitEvent(stream, dc.ev_q, 0));
        return BRT_OK;
    }, [&](DeviceCtx& dc, hipStream_t stream) {
        char* const ping[2] = {dc.d_lightmap, dc.d_lightmap + image_bytes};
        return dilate_enqueue(ctx, stream, d_texels_f32, ping, width, height, passes, wrap_u, d_out, (flags & BRT_FLAG_OUT_RGBA16F) != 0u);
    });
    });
}

int32_t brt_bake_lightmap_device(brt_ctx* ctx, const void* d_points, uint32_t width, uint32_t height, uint32_t n_dirs, uint32_t bounces,
                                 uint32_t passes, uint32_t wrap_u, float origin_bound, void* d_out, void* d_info_or_null, void* hip_stream,
                                 uint32_t flags, uint64_t* out_stats8) {
    return ctx_guard(ctx, [&]() -> int32_t {
    int32_t rc = flags_check(ctx, flags, BRT_FLAG_CALLER_STREAM | BRT_FLAG_OUT_RGBA16F, "flags: BRT_FLAG_CALLER_STREAM and BRT_FLAG_OUT_RGBA16F only");
    if (rc == BRT_OK) rc = lightmap_bake_check(ctx, d_points, width, height, n_dirs, bounces, passes, wrap_u, origin_bound, d_out, d_info_or_null, flags);
    if (rc == BRT_OK) rc = device_aligned(ctx, {d_points, d_out, d_info_or_null});
    if (rc != BRT_OK) return rc;
    return bake_call(ctx, origin_bound, hip_stream, flags & BRT_FLAG_CALLER_STREAM, out_stats8,
                     [&](DeviceCtx& dc, hipStream_t stream, bool counted, BakeRun* run) {
        return lightmap_bake_enqueue(ctx, dc, stream, d_points, width, height, n_dirs, bounces, passes, wrap_u, d_out, d_info_or_null,
                                     flags & BRT_FLAG_OUT_MASK, counted, run);
    });
    });
}

int32_t brt_bake_lightmap(brt_ctx* ctx, const void* points, uint32_t width, uint32_t height, uint32_t n_dirs, uint32_t bounces, uint32_t passes,
                          uint32_t wrap_u, float origin_bound, void* out, void* info_or_null, uint32_t flags, uint64_t* out_stats8) {
    return ctx_guard(ctx, [&]() -> int32_t {
    int32_t rc = flags_check(ctx, flags, BRT_FLAG_OUT_RGBA16F, "flags: BRT_FLAG_OUT_RGBA16F only");
    if (rc == BRT_OK) rc = lightmap_bake_check(ctx, points, width, height, n_dirs, bounces, passes, wrap_u, origin_bound, out, info_or_null, flags);
    if (rc != BRT_OK) return rc;
    const size_t n = (size_t)width * height;
    return bake_call_host(ctx, origin_bound, {{points, nullptr, n * 32u}, {nullptr, out, n * texel_bytes(flags)},
                                              {nullptr, info_or_null, info_or_null ? n * 8u : 0u}}, out_stats8,
                          [&](DeviceCtx& dc, hipStream_t stream, bool counted, BakeRun* run, char* const* d) {
        return lightmap_bake_enqueue(ctx, dc, stream, d[0], width, height, n_dirs, bounces, passes, wrap_u, d[1], d[2], flags, counted, run);
    });
    });
}

}  // extern "C"
