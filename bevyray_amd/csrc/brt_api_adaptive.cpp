// brt_api_adaptive.cpp -- adaptive sampling on the first device (brt_adaptive.hip; DESIGN.md "Adaptive sampling"): a base frame at
// base_spp samples, the pixels the rule of brt_adaptive.h selects traced again at the camera's own sample count by the sparse pixel tracer.
// The skeleton of an export and its stats rule (frame_call), the base frame the context keeps (context_frame, ordered by ev_dn), the
// selection list and its re-trace (refine_list, trace_selected, ordered by ev_q) and the flag, size and overlap helpers are those of every
// call on a whole frame (brt_frame.h); the guides and their scratch are the denoiser's (brt_api_post.cpp denoise_begin).  Here: the checks
// of each export in their order, the settings, the dispatch history of base frames, and the enqueue of the selecting kernel.
#include "brt_frame.h"

using namespace brt;

namespace {

int32_t adaptive_check(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height) {
    if (!camera80 || !window16) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "camera/window is null");
    if (const int32_t bad = size_check(ctx, width, height)) return bad;
    if (!ctx->has_scene) return ctx_fail(ctx, BRT_ERR_NO_SCENE, "brt_upload_scene has not succeeded yet");
    Camera cam;
    std::memcpy(&cam, camera80, sizeof cam);
    if (cam.projection_type != 0) return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, "only perspective projection (0) is supported (extract.rs:148)");
    if (ctx->policy_flags & kPolicyMask)
        return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, "the pixel tracer implements the default policy only (brt_set_policy)");
    return BRT_OK;
}

uint32_t sample_count_of(const void* camera80) {
    Camera cam;
    std::memcpy(&cam, camera80, sizeof cam);
    return cam.sample_count;
}

// The settings of one call: a base frame that already has the camera's samples (or more) selects nothing
struct Rule {
    float threshold;
    uint32_t min_taps;
};
Rule rule_of(const brt_ctx* ctx, const void* camera80) {
    if (ctx->adaptive.base_spp >= sample_count_of(camera80)) return {std::numeric_limits<float>::infinity(), 0u};
    return {ctx->adaptive.threshold, ctx->adaptive.min_taps};
}

// The base trace runs with the ray count of the view's last BASE frame (DeviceCtx::base_view_rays), and leaves the one of its last plain
// frame as it found it: the two have different sample counts, so one slot would be a miss for both on every alternation
struct BaseHistory {
    brt_ctx* ctx;
    void swap() {
        for (auto& dc : ctx->devs) {
            std::swap(dc.view_rays, dc.base_view_rays);
            std::swap_ranges(dc.view_key, dc.view_key + 8, dc.base_view_key);
        }
    }
    explicit BaseHistory(brt_ctx* c) : ctx(c) { swap(); }
    ~BaseHistory() { swap(); }
};

// behind the base frame at d_base on `stream`: the full-size guides, the selection into d_out (mask: into d_mask, nothing else), then the
// selected pixels traced into d_out with the call's own camera; the count to d_count (or nullptr)
int32_t adaptive_enqueue(brt_ctx* ctx, DeviceCtx& dc, const void* camera80, const void* window16, uint32_t width, uint32_t height,
                         const float* d_base, void* d_out, uint32_t out_format, uint8_t* d_mask, uint32_t* d_count, hipStream_t stream) {
    FrameParams fp;
    DenoiseScratch ds;
    int32_t rc = denoise_begin(ctx, dc, camera80, window16, width, height, stream, &fp, &ds);
    if (rc != BRT_OK) return rc;
    HIP_TRY(ctx, launch_denoise_guides(dc.view, fp, ds, stream));
    const Rule rule = rule_of(ctx, camera80);
    AdaptiveSelect as{};
    as.width = width;
    as.height = height;
    as.threshold = rule.threshold;
    as.min_taps = rule.min_taps;
    as.base = reinterpret_cast<const float4*>(d_base);
    as.g0 = ds.g0;
    as.g1 = ds.g1;
    as.out_format = out_format;
    if (d_mask) {
        as.mask = d_mask;
        HIP_TRY(ctx, launch_adaptive_select(as, stream));
        HIP_TRY(ctx, hipEventRecord(dc.ev_dn, stream));
        return BRT_OK;
    }
    SelectList sl;
    rc = refine_list(ctx, dc, width, height, stream, &sl);
    if (rc != BRT_OK) return rc;
    as.out = d_out;
    as.count = sl.count;
    as.list = sl.list;
    HIP_TRY(ctx, launch_adaptive_select(as, stream));
    HIP_TRY(ctx, hipEventRecord(dc.ev_dn, stream));      // (the guides and a base frame of the context are free again)
    return trace_selected(ctx, dc, camera80, window16, width, height, sl, d_out, out_format, d_count, stream);
}

}  // namespace

extern "C" {

int32_t brt_set_adaptive(brt_ctx* ctx, uint32_t base_spp, float threshold, uint32_t min_taps) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (base_spp < 1u || base_spp > 65535u) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "base_spp must be in [1, 65535]");
    if (!adapt_finite(threshold) || !(threshold > 0.0f)) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "threshold must be finite and > 0");
    if (min_taps < 1u || min_taps > 25u) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "min_taps must be in [1, 25]");
    ctx->adaptive.base_spp = base_spp;
    ctx->adaptive.threshold = threshold;
    ctx->adaptive.min_taps = min_taps;
    return BRT_OK;
    });
}

int32_t brt_render_adaptive_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height, void* d_frame,
                                   uint32_t* d_selected_count_or_null, void* hip_stream, uint32_t flags, brt_stats* stats) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (!d_frame) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_frame is null");
    if (const int32_t bad = flags_check(ctx, flags, kOutFlags, "flags: BRT_FLAG_CALLER_STREAM and BRT_FLAG_OUT_* only (pixels of two sample counts: no post-pass)"))
        return bad;
    if (const int32_t bad = adaptive_check(ctx, camera80, window16, width, height)) return bad;
    const uint32_t fmt = flags & BRT_FLAG_OUT_MASK;
    if (overlaps(d_frame, out_bytes(width, height, fmt), d_selected_count_or_null, 4u))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_frame overlaps d_selected_count");
    const bool plain = ctx->adaptive.base_spp >= sample_count_of(camera80);
    Camera base_cam;
    std::memcpy(&base_cam, camera80, sizeof base_cam);
    base_cam.sample_count = ctx->adaptive.base_spp;
    // the stats are the traced frame's, with the rays of the re-trace added where there is one
    return frame_call(ctx, camera80, hip_stream, flags, stats, plain ? FRAME_STATS_KEEP : FRAME_STATS_ADD_RETRACE,
                      [&](DeviceCtx& dc, const StreamChoice& sc) -> int32_t {
        if (plain) {      // the base frame would have the camera's samples or more: the plain frame, nothing selected
            const int32_t r = render_frame_device(ctx, camera80, window16, BRT_LEVEL_PURE, width, height, nullptr, nullptr, d_frame, hip_stream, flags, stats);
            if (r != BRT_OK) return r;
            HIP_TRY(ctx, hipSetDevice(dc.device));
            if (d_selected_count_or_null) HIP_TRY(ctx, hipMemsetAsync(d_selected_count_or_null, 0, 4, sc.stream));
            return BRT_OK;
        }
        int32_t r = context_frame(ctx, dc, (size_t)width * height * 16u, sc.stream);
        if (r != BRT_OK) return r;
        {
            BaseHistory slot(ctx);
            r = render_frame_device(ctx, &base_cam, window16, BRT_LEVEL_PURE, width, height, nullptr, nullptr, dc.d_uplow, hip_stream,
                                    flags & BRT_FLAG_CALLER_STREAM, stats);
        }
        if (r != BRT_OK) return r;
        HIP_TRY(ctx, hipSetDevice(dc.device));
        return adaptive_enqueue(ctx, dc, camera80, window16, width, height, dc.d_uplow, d_frame, fmt, nullptr, d_selected_count_or_null, sc.stream);
    });
    });
}

int32_t brt_adaptive_refine_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height,
                                   const float* d_base_rgba, void* d_out, uint32_t* d_selected_count_or_null, void* hip_stream,
                                   uint32_t flags, brt_stats* stats) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (!d_base_rgba || !d_out) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_base_rgba / d_out is null");
    if (const int32_t bad = flags_check(ctx, flags, kOutFlags, "flags: BRT_FLAG_CALLER_STREAM and BRT_FLAG_OUT_* only")) return bad;
    if (const int32_t bad = adaptive_check(ctx, camera80, window16, width, height)) return bad;
    const uint32_t fmt = flags & BRT_FLAG_OUT_MASK;
    if (overlaps(d_out, out_bytes(width, height, fmt), d_base_rgba, (size_t)width * height * 16u))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_out overlaps d_base_rgba");
    if (overlaps(d_out, out_bytes(width, height, fmt), d_selected_count_or_null, 4u))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_out overlaps d_selected_count");
    // the stats: the rays of the re-trace, total_ms, and the tree
    return frame_call(ctx, camera80, hip_stream, flags, stats, FRAME_STATS_CLEAR | FRAME_STATS_ADD_RETRACE,
                      [&](DeviceCtx& dc, const StreamChoice& sc) -> int32_t {
        return adaptive_enqueue(ctx, dc, camera80, window16, width, height, d_base_rgba, d_out, fmt, nullptr, d_selected_count_or_null, sc.stream);
    });
    });
}

int32_t brt_adaptive_mask_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height,
                                 const float* d_base_rgba, void* d_mask_u8, void* hip_stream, uint32_t flags) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (!d_base_rgba || !d_mask_u8) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_base_rgba / d_mask_u8 is null");
    if (const int32_t bad = caller_stream_flags_check(ctx, flags)) return bad;
    if (const int32_t bad = adaptive_check(ctx, camera80, window16, width, height)) return bad;
    if (overlaps(d_mask_u8, (size_t)width * height, d_base_rgba, (size_t)width * height * 16u))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_mask_u8 overlaps d_base_rgba");
    return frame_call(ctx, camera80, hip_stream, flags, nullptr, FRAME_STATS_KEEP, [&](DeviceCtx& dc, const StreamChoice& sc) -> int32_t {
        return adaptive_enqueue(ctx, dc, camera80, window16, width, height, d_base_rgba, nullptr, BRT_FLAG_OUT_RGBA32F,
                                static_cast<uint8_t*>(d_mask_u8), nullptr, sc.stream);
    });
    });
}

// the rule of brt_adaptive.h for ONE pixel from its 25 taps in the rule's order (dy outer, dx inner): the code k_adaptive_select compiles
int32_t brt_host_adaptive_class(float t, uint32_t material_id, const float* rgb, const uint32_t* taps_inside25, const uint32_t* taps_id25,
                                const float* taps_rgb75, float threshold, uint32_t min_taps, uint32_t* out_class) {
    return guard(nullptr, [&]() -> int32_t {
    if (!rgb || !taps_inside25 || !taps_id25 || !taps_rgb75 || !out_class) return fail(BRT_ERR_INVALID_ARGUMENT, "null pointer");
    const int span = 2 * kAdaptRadius + 1;
    *out_class = adapt_classify(t, material_id, adapt_luma(rgb[0], rgb[1], rgb[2]), threshold, min_taps,
                                [&](int dx, int dy, uint32_t* id_q, float* l_q) {
                                    const int k = (dy + kAdaptRadius) * span + dx + kAdaptRadius;
                                    *id_q = taps_id25[k];
                                    *l_q = adapt_luma(taps_rgb75[3 * k], taps_rgb75[3 * k + 1], taps_rgb75[3 * k + 2]);
                                    return taps_inside25[k] != 0;
                                });
    return BRT_OK;
    });
}

}  // extern "C"
