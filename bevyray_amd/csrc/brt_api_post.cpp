// brt_api_post.cpp -- the post-passes on the first device: denoiser (brt_denoise.hip), temporal accumulation (brt_temporal.hip), blend-post.
// The skeleton of an export (tree, device, stream, synchronisation, stats) is that of every call on a whole frame (brt_frame.h frame_call),
// and so are the flag and size checks (flags_check, size_check).  Here: the denoiser's scratch and its ordering behind ev_dn
// (denoise_begin), the temporal history, the pass sequence (run_denoise), the post-pass flags of a render, the settings and debug reads.
#include "brt_frame.h"

using namespace brt;

namespace {

// ---- temporal accumulation (brt_temporal.hip) on the first device ----

// the history of fp's frame and the arguments of its accumulation, for work on `stream` (which denoise_begin has ordered behind the
// previous denoise, temporal or not, of the context): the planes (a new size: a reset), the spheres of this frame and of the previous
// temporal frame in the caller's order, and the map from the resident sphere numbering to the caller's
int32_t temporal_begin(brt_ctx* ctx, DeviceCtx& dc, const FrameParams& fp, hipStream_t stream, TemporalHistory* th, TemporalArgs* ta,
                       const uint32_t** rmap) {
    auto& tp = ctx->temporal;
    bool had = tp.valid && tp.width == fp.width && tp.height == fp.height;
    tp.valid = false;                               // (until this frame is enqueued)
    const size_t bytes = temporal_history_bytes(fp.width, fp.height);
    if (dc.temporal_cap < bytes) HIP_TRY(ctx, hipEventSynchronize(dc.ev_dn));
    int32_t rc = ensure(ctx, &dc.d_temporal, &dc.temporal_cap, bytes);
    if (rc != BRT_OK) return rc;
    *th = temporal_history(dc.d_temporal, fp.width, fp.height);
    const uint32_t m = dc.view.n_models;
    const std::vector<float>& sph = ctx->enc.spheres;          // {centre, r^2} in the caller's order (validate_and_encode)
    if (m == 0u || sph.size() != (size_t)m * 4u) return ctx_fail(ctx, BRT_ERR_NO_SCENE, "no resident spheres for the temporal history");
    const size_t sb = (size_t)m * 36u;
    if (dc.tsph_cap < sb) HIP_TRY(ctx, hipEventSynchronize(dc.ev_dn));
    rc = ensure(ctx, &dc.d_tsph, &dc.tsph_cap, sb);
    if (rc != BRT_OK) return rc;
    if (tp.slot_models != m) {                       // (another layout: what the slots held is gone)
        tp.slot_models = m;
        tp.slot_epoch[0] = tp.slot_epoch[1] = -1;
        tp.h_rmap.clear();
    }
    float4* slots[2] = {reinterpret_cast<float4*>(dc.d_tsph), reinterpret_cast<float4*>(dc.d_tsph) + m};
    uint32_t* d_rmap = reinterpret_cast<uint32_t*>(slots[1] + m);
    const int64_t epoch = ctx->scene_epoch;
    const int old = !had ? -1 : tp.slot_epoch[0] == tp.prev_epoch ? 0 : tp.slot_epoch[1] == tp.prev_epoch ? 1 : -1;
    int cur = tp.slot_epoch[0] == epoch ? 0 : tp.slot_epoch[1] == epoch ? 1 : -1;
    bool copied = false;
    if (cur < 0) {                                  // a new upload: into the slot the previous frame's spheres are not in
        cur = old == 0 ? 1 : 0;
        HIP_TRY(ctx, hipMemcpyAsync(slots[cur], sph.data(), (size_t)m * 16u, hipMemcpyHostToDevice, stream));
        tp.slot_epoch[cur] = epoch;
        copied = true;
    }
    // the hot order (apply_hot_order) renumbers the resident spheres: h_total_srank[caller index] = resident index
    *rmap = nullptr;
    if (dc.hot_tree == ctx->tree_epoch && dc.h_total_srank.size() == m) {
        std::vector<uint32_t> map(m);
        for (uint32_t i = 0; i < m; i++) map[dc.h_total_srank[i]] = i;
        if (map != tp.h_rmap) {
            tp.h_rmap.swap(map);
            HIP_TRY(ctx, hipMemcpyAsync(d_rmap, tp.h_rmap.data(), (size_t)m * 4u, hipMemcpyHostToDevice, stream));
            copied = true;
        }
        *rmap = d_rmap;
    }
    if (copied) HIP_TRY(ctx, hipStreamSynchronize(stream));     // (pageable sources; a frame after an upload or a renumbering only)
    had = had && old >= 0;
    const FrameParams& pp = tp.prev;
    auto same = [](const float* a, const float* b, int n) { return std::memcmp(a, b, sizeof(float) * (size_t)n) == 0; };
    ta->prev = tp.set;
    ta->has_history = had ? 1u : 0u;
    ta->same_camera = had && same(fp.cam_pos, pp.cam_pos, 3) && same(fp.cam_dir, pp.cam_dir, 3) && same(fp.cam_up, pp.cam_up, 3) &&
                      same(fp.cam_right, pp.cam_right, 3) && same(&fp.aspect, &pp.aspect, 1) && same(&fp.tan_half_fov, &pp.tan_half_fov, 1);
    ta->motion = had && tp.prev_models == m ? 1u : 0u;
    ta->max_history = (float)tp.max_history;
    ta->sph_new = slots[cur];
    ta->sph_old = slots[old >= 0 ? old : cur];
    if (!had) tp.prev = fp;                         // (no previous camera: the kernel reads none)
    return BRT_OK;
}

}  // namespace

namespace brt {

// ---- denoiser (brt_denoise.hip) on the first device ----

// the frame parameters the guides are cast with (one part, level 3) and the scratch of a width x height frame for work on `stream`:
// the stream first waits for the last denoise (on whichever stream), so that what is enqueued next -- an assembled frame into
// ds->frame included -- finds the scratch free; a larger one is allocated only once that denoise has finished
int32_t denoise_begin(brt_ctx* ctx, DeviceCtx& dc, const void* camera80, const void* window16, uint32_t width, uint32_t height,
                      hipStream_t stream, FrameParams* fp, DenoiseScratch* ds) {
    int32_t rc = make_frame_params(ctx, camera80, window16, BRT_LEVEL_PURE, width, height, 0u, 1u, fp);
    if (rc != BRT_OK) return rc;
    const size_t bytes = denoise_scratch_bytes(width, height);
    if (dc.denoise_cap < bytes) HIP_TRY(ctx, hipEventSynchronize(dc.ev_dn));
    rc = ensure(ctx, &dc.d_denoise, &dc.denoise_cap, bytes);
    if (rc != BRT_OK) return rc;
    HIP_TRY(ctx, hipStreamWaitEvent(stream, dc.ev_dn, 0));
    *ds = denoise_scratch(dc.d_denoise, width, height);
    return BRT_OK;
}

// guides of fp's frame on the resident scene, then the passes (BRT_FLAG_DENOISE) and / or the temporal accumulation
// (BRT_FLAG_TEMPORAL) from d_in (RGBA32F) into d_out (out_format), on `stream` (which denoise_begin has ordered behind the
// previous denoise of the context).  bp.on: d_in is a coverage frame (BRT_FLAG_BLEND_POST / brt_blend_post_device)
int32_t run_denoise(brt_ctx* ctx, DeviceCtx& dc, const FrameParams& fp, const DenoiseScratch& ds, const float* d_in, void* d_out,
                    uint32_t out_format, hipStream_t stream, uint32_t flags, const BlendPost& bp) {
    const float* d_cov = bp.on ? d_in : nullptr;
    if (!(flags & BRT_FLAG_TEMPORAL)) {
        HIP_TRY(ctx, launch_denoise_guides(dc.view, fp, ds, stream, nullptr, nullptr, d_cov));
        HIP_TRY(ctx, launch_denoise(fp, ctx->denoise, ds, d_in, d_out, out_format, stream, bp));
        HIP_TRY(ctx, hipEventRecord(dc.ev_dn, stream));
        return BRT_OK;
    }
    TemporalHistory th;
    TemporalArgs ta;
    const uint32_t* rmap = nullptr;
    int32_t rc = temporal_begin(ctx, dc, fp, stream, &th, &ta, &rmap);
    if (rc != BRT_OK) return rc;
    const bool filter = (flags & BRT_FLAG_DENOISE) != 0u;
    HIP_TRY(ctx, launch_denoise_guides(dc.view, fp, ds, stream, rmap, th.sid, d_cov));
    HIP_TRY(ctx, launch_denoise_demod(fp, ds, d_in, !filter, stream));
    HIP_TRY(ctx, launch_temporal(fp, ctx->temporal.prev, ta, ds, th, filter ? nullptr : d_out, out_format, stream, bp));
    if (filter) HIP_TRY(ctx, launch_denoise_filter(fp, ctx->denoise, ds, d_out, out_format, stream, th.c[ta.prev ^ 1u], bp));
    HIP_TRY(ctx, hipEventRecord(dc.ev_dn, stream));
    auto& tp = ctx->temporal;
    tp.valid = true;
    tp.width = fp.width;
    tp.height = fp.height;
    tp.set = ta.prev ^ 1u;
    tp.prev = fp;
    tp.prev_models = dc.view.n_models;
    tp.prev_epoch = ctx->scene_epoch;
    return BRT_OK;
}

// BRT_FLAG_BLEND_POST takes effect at the levels that blend (1 / 2); level 3 ignores it (post_flags_check has refused the rest)
bool blend_post_on(uint32_t level, uint32_t flags) {
    return (flags & BRT_FLAG_BLEND_POST) != 0u && (level == BRT_LEVEL_FALLBACK_RASTER || level == BRT_LEVEL_FALLBACK_RAYTRACED);
}

// the post-pass flags of brt_render / brt_render_device against the level
int32_t post_flags_check(brt_ctx* ctx, uint32_t level, uint32_t flags) {
    const bool post = (flags & (BRT_FLAG_DENOISE | BRT_FLAG_TEMPORAL)) != 0u;
    if ((flags & BRT_FLAG_BLEND_POST) && !post)
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "BRT_FLAG_BLEND_POST needs BRT_FLAG_DENOISE and / or BRT_FLAG_TEMPORAL");
    if (post && level != BRT_LEVEL_PURE && !blend_post_on(level, flags))
        return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, (flags & BRT_FLAG_BLEND_POST)
                            ? "BRT_FLAG_BLEND_POST needs level 1, 2 or 3: level 0 traces nothing"
                            : "BRT_FLAG_DENOISE / BRT_FLAG_TEMPORAL need level 3 (Pure): the raster blend of levels 1 / 2 is not known to the guides");
    return BRT_OK;
}

}  // namespace brt

namespace {

// brt_denoise_device, and brt_blend_post_device (bp.on: d_frame_rgba is a coverage frame)
int32_t denoise_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height, const float* d_frame_rgba,
                       void* d_out, void* hip_stream, uint32_t flags, brt_stats* stats, const BlendPost& bp) {
    if (!d_frame_rgba || !d_out) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, bp.on ? "d_coverage_rgba / d_out is null" : "d_frame_rgba / d_out is null");
    if (const int32_t bad = flags_check(ctx, flags, kOutPostFlags, "flags: BRT_FLAG_CALLER_STREAM, BRT_FLAG_OUT_*, BRT_FLAG_DENOISE and BRT_FLAG_TEMPORAL only"))
        return bad;
    if (!ctx->has_scene) return ctx_fail(ctx, BRT_ERR_NO_SCENE, "brt_upload_scene has not succeeded yet");
    return frame_call(ctx, camera80, hip_stream, flags, stats, FRAME_STATS_CLEAR, [&](DeviceCtx& dc, const StreamChoice& sc) -> int32_t {
        FrameParams fp;
        DenoiseScratch ds;
        const int32_t rc = denoise_begin(ctx, dc, camera80, window16, width, height, sc.stream, &fp, &ds);
        if (rc != BRT_OK) return rc;
        // without BRT_FLAG_TEMPORAL the call denoises (BRT_FLAG_DENOISE implied); with it, it accumulates, and filters if BRT_FLAG_DENOISE is set too
        const uint32_t post = (flags & BRT_FLAG_TEMPORAL) ? flags & (BRT_FLAG_DENOISE | BRT_FLAG_TEMPORAL) : (uint32_t)BRT_FLAG_DENOISE;
        return run_denoise(ctx, dc, fp, ds, d_frame_rgba, d_out, flags & BRT_FLAG_OUT_MASK, sc.stream, post, bp);
    });
}

}  // namespace

extern "C" {

int32_t brt_set_denoise(brt_ctx* ctx, uint32_t iterations, float sigma_luminance, float sigma_normal, float sigma_depth) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (iterations < 1u || iterations > 6u) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "iterations must be in [1, 6]");
    for (float v : {sigma_luminance, sigma_normal, sigma_depth})
        if (!std::isfinite(v) || !(v > 0.0f)) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "the sigmas must be finite and > 0");
    ctx->denoise.iterations = iterations;
    ctx->denoise.sigma_l = sigma_luminance;
    ctx->denoise.sigma_n = sigma_normal;
    ctx->denoise.sigma_z = sigma_depth;
    return BRT_OK;
    });
}

int32_t brt_denoise_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height,
                           const float* d_frame_rgba, void* d_out, void* hip_stream, uint32_t flags, brt_stats* stats) {
    return ctx_guard(ctx, [&]() -> int32_t {
    return denoise_device(ctx, camera80, window16, width, height, d_frame_rgba, d_out, hip_stream, flags, stats, BlendPost());
    });
}

int32_t brt_blend_post_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height,
                              const float* d_coverage_rgba, const float* d_raster_rgba, void* d_out, void* hip_stream, uint32_t flags,
                              brt_stats* stats) {
    return ctx_guard(ctx, [&]() -> int32_t {
    BlendPost bp;
    bp.on = true;
    bp.d_raster_rgba = d_raster_rgba;
    return denoise_device(ctx, camera80, window16, width, height, d_coverage_rgba, d_out, hip_stream, flags, stats, bp);
    });
}

int32_t brt_debug_denoise_guides(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height, float* out8) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (!out8) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "out8 is null");
    if (!ctx->has_scene) return ctx_fail(ctx, BRT_ERR_NO_SCENE, "brt_upload_scene has not succeeded yet");
    return frame_call(ctx, camera80, nullptr, 0u, nullptr, FRAME_STATS_KEEP, [&](DeviceCtx& dc, const StreamChoice& sc) -> int32_t {
        FrameParams fp;
        DenoiseScratch ds;
        const int32_t rc = denoise_begin(ctx, dc, camera80, window16, width, height, sc.stream, &fp, &ds);
        if (rc != BRT_OK) return rc;
        HIP_TRY(ctx, launch_denoise_guides(dc.view, fp, ds, sc.stream));
        const size_t n = (size_t)width * height;
        HIP_TRY(ctx, hipMemcpy2DAsync(out8, 32, ds.g0, 16, 16, n, hipMemcpyDeviceToHost, sc.stream));
        HIP_TRY(ctx, hipMemcpy2DAsync(out8 + 4, 32, ds.g1, 16, 16, n, hipMemcpyDeviceToHost, sc.stream));
        HIP_TRY(ctx, hipEventRecord(dc.ev_dn, sc.stream));
        return BRT_OK;
    });
    });
}

int32_t brt_set_temporal(brt_ctx* ctx, uint32_t max_history) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (max_history < 1u || max_history > 65535u) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "max_history must be in [1, 65535]");
    ctx->temporal.max_history = max_history;
    ctx->temporal.valid = false;
    return BRT_OK;
    });
}

int32_t brt_reset_temporal(brt_ctx* ctx) {
    return ctx_guard(ctx, [&]() -> int32_t {
    ctx->temporal.valid = false;
    return BRT_OK;
    });
}

int32_t brt_debug_temporal_state(brt_ctx* ctx, uint32_t width, uint32_t height, float* out8) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (!out8) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "out8 is null");
    if (const int32_t bad = size_check(ctx, width, height)) return bad;
    const auto& tp = ctx->temporal;
    const size_t n = (size_t)width * height;
    if (!tp.valid) {                                 // an empty history: n = 0, nothing reprojected
        const float nan = std::numeric_limits<float>::quiet_NaN();
        for (size_t i = 0; i < n; i++) {
            float* o = out8 + i * 8;
            o[0] = o[1] = o[2] = o[3] = o[4] = o[5] = 0.0f;
            o[6] = o[7] = nan;
        }
        return BRT_OK;
    }
    if (width != tp.width || height != tp.height) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "the history is of another size");
    DeviceCtx& dc = ctx->devs[0];
    HIP_TRY(ctx, hipSetDevice(dc.device));
    const TemporalHistory th = temporal_history(dc.d_temporal, width, height);
    HIP_TRY(ctx, hipStreamWaitEvent(dc.stream, dc.ev_dn, 0));
    HIP_TRY(ctx, hipMemcpy2DAsync(out8, 32, th.b[tp.set], 16, 16, n, hipMemcpyDeviceToHost, dc.stream));
    HIP_TRY(ctx, hipMemcpy2DAsync(out8 + 4, 32, th.c[tp.set], 16, 8, n, hipMemcpyDeviceToHost, dc.stream));
    HIP_TRY(ctx, hipMemcpy2DAsync(out8 + 6, 32, th.xy, 8, 8, n, hipMemcpyDeviceToHost, dc.stream));
    HIP_TRY(ctx, hipEventRecord(dc.ev_dn, dc.stream));
    HIP_TRY(ctx, hipStreamSynchronize(dc.stream));
    return BRT_OK;
    });
}

}  // extern "C"
