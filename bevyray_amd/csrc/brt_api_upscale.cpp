// brt_api_upscale.cpp -- guide-buffer upsampling on the first device (brt_upscale.hip): of a low frame the caller holds, and of one the
// call traces (and post-processes) itself.  DESIGN.md "Guide-buffer upsampling"; with a level and the full-size raster inputs
// (brt_upscale_blend_device, brt_render_upscaled_blend_device): "Upsampling blended frames"; with the selected pixels traced again at
// full size: "Refined upsampling".  The skeleton of an export, the low frame the context keeps (context_frame, ordered by ev_dn), the
// selection list and its re-trace (refine_list, trace_selected, ordered by ev_q) and the flag, level and overlap helpers are those of
// every call on a whole frame (brt_frame.h); the scratch and ev_dn are the denoiser's (brt_api_post.cpp denoise_begin).  Here: the size
// rule of a pair of frames, the low window, the checks of each export in their order, and the enqueue of the upsampling kernel.
#include "brt_frame.h"

using namespace brt;

namespace {

// full <= kMaxRatio * low per axis.  The kernel is correct at any ratio (its taps are counted in low pixels); the bound is one of quality:
// beyond it a low pixel stands for more than 16 output pixels and the quality of DESIGN.md "Guide-buffer upsampling" was not measured.
constexpr uint32_t kMaxRatio = 4;

// the window of the low frame: random_seed as it is, height scaled in integer arithmetic and at least 1 (the jitter of a low frame's
// samples is sized by it, raytrace.wgsl:139-147)
void low_window(const void* window16, uint32_t height, uint32_t low_height, void* out_window16) {
    Window w;
    std::memcpy(&w, window16, sizeof w);
    w.height = (uint32_t)std::max<uint64_t>(1u, (uint64_t)w.height * low_height / height);
    std::memcpy(out_window16, &w, sizeof w);
}

int32_t sizes_check(brt_ctx* ctx, uint32_t low_width, uint32_t low_height, uint32_t width, uint32_t height) {
    const uint32_t lo[2] = {low_width, low_height}, hi[2] = {width, height};
    for (int k = 0; k < 2; k++)
        if (lo[k] < 1u || lo[k] > hi[k] || hi[k] > 32768u || hi[k] > kMaxRatio * lo[k])
            return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "sizes: 1 <= low <= full <= 32768 and full <= 4 x low, per axis");
    return BRT_OK;
}

// The frame an upsampling presents: level 3 (what the calls without a level pass), or a level that blends with its full-size raster
// inputs on the first device (either may be null: zeros) -- the low frame is a Pure frame in both
struct Blend {
    uint32_t level = BRT_LEVEL_PURE;
    const float* d_raster_rgba = nullptr;
    const float* d_raster_depth = nullptr;
    bool on() const { return level != BRT_LEVEL_PURE; }
};

// the level of a blended call: 3 is the call without a level (the raster inputs are not read), 0 traces nothing
int32_t level_check(brt_ctx* ctx, Blend* bl) {
    if (const int32_t bad = frame_level_check(ctx, bl->level, "level 0 traces nothing: there is no frame to upsample")) return bad;
    if (!bl->on()) bl->d_raster_rgba = bl->d_raster_depth = nullptr;
    return BRT_OK;
}

// the output of a blended frame is written while other pixels' raster texels and depths are still to be read
int32_t raster_overlap_check(brt_ctx* ctx, const Blend& bl, const void* d_out, uint32_t width, uint32_t height, uint32_t fmt) {
    const size_t n = (size_t)width * height, ob = out_bytes(width, height, fmt);
    if (overlaps(d_out, ob, bl.d_raster_rgba, n * 16u)) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "the output overlaps d_raster_rgba");
    if (overlaps(d_out, ob, bl.d_raster_depth, n * 4u)) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "the output overlaps d_raster_depth");
    return BRT_OK;
}

// behind the low frame at d_low on `stream`: its guides unless a post-pass has just left them in the scratch, then the upsampling into
// d_out; the scratch is the denoiser's and the event its ordering event, so the call queues up with the context's other post-passes
int32_t upscale_enqueue(brt_ctx* ctx, DeviceCtx& dc, const void* camera80, const void* low_window16, uint32_t low_width, uint32_t low_height,
                        const float* d_low, const void* window16, uint32_t width, uint32_t height, void* d_out, uint32_t out_format,
                        hipStream_t stream, bool guides_resident, const Blend& bl, const UpscaleSelect* select = nullptr) {
    FrameParams low, full;
    DenoiseScratch ds;
    int32_t rc = make_frame_params(ctx, camera80, window16, bl.level, width, height, 0u, 1u, &full);      // (near, far, fallback_far)
    if (rc == BRT_OK) rc = denoise_begin(ctx, dc, camera80, low_window16, low_width, low_height, stream, &low, &ds);
    if (rc != BRT_OK) return rc;
    if (!guides_resident) HIP_TRY(ctx, launch_denoise_guides(dc.view, low, ds, stream));
    const UpscaleBlend ub = {reinterpret_cast<const float4*>(bl.d_raster_rgba), bl.d_raster_depth};
    HIP_TRY(ctx, launch_upscale(dc.view, full, low, ctx->denoise, ds, d_low, d_out, out_format, stream, bl.on() ? &ub : nullptr, select));
    HIP_TRY(ctx, hipEventRecord(dc.ev_dn, stream));
    return BRT_OK;
}

int32_t upscale_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t low_width, uint32_t low_height,
                       const float* d_low_rgba, uint32_t width, uint32_t height, void* d_out, void* hip_stream, uint32_t flags,
                       brt_stats* stats, Blend bl) {
    if (!camera80 || !window16) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "camera/window is null");
    if (!d_low_rgba || !d_out) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_low_rgba / d_out is null");
    if (const int32_t bad = flags_check(ctx, flags, kOutFlags, "flags: BRT_FLAG_CALLER_STREAM and BRT_FLAG_OUT_* only")) return bad;
    if (const int32_t bad = level_check(ctx, &bl)) return bad;
    if (const int32_t bad = sizes_check(ctx, low_width, low_height, width, height)) return bad;
    const uint32_t fmt = flags & BRT_FLAG_OUT_MASK;
    if (overlaps(d_out, out_bytes(width, height, fmt), d_low_rgba, (size_t)low_width * low_height * 16u))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_out overlaps d_low_rgba");
    if (const int32_t bad = raster_overlap_check(ctx, bl, d_out, width, height, fmt)) return bad;
    if (!ctx->has_scene) return ctx_fail(ctx, BRT_ERR_NO_SCENE, "brt_upload_scene has not succeeded yet");
    return frame_call(ctx, camera80, hip_stream, flags, stats, FRAME_STATS_CLEAR, [&](DeviceCtx& dc, const StreamChoice& sc) -> int32_t {
        return upscale_enqueue(ctx, dc, camera80, window16, low_width, low_height, d_low_rgba, window16, width, height, d_out, fmt, sc.stream,
                               false, bl);
    });
}

// The low frame of a call that traces it, into the context's frame (context_frame) on the call's stream: exactly brt_render_device's
// low_width x low_height Pure frame (every device of the context) with the post-passes `post` on it, whatever the level of the presented
// frame -- its raster blend is decided per output pixel by the upsampling.  Leaves the first device current.
int32_t low_frame(brt_ctx* ctx, DeviceCtx& dc, const StreamChoice& sc, const void* camera80, const void* low_window16, uint32_t low_width,
                  uint32_t low_height, void* hip_stream, uint32_t flags, uint32_t post, brt_stats* stats) {
    int32_t r = context_frame(ctx, dc, (size_t)low_width * low_height * 16u, sc.stream);
    if (r == BRT_OK)
        r = render_frame_device(ctx, camera80, low_window16, BRT_LEVEL_PURE, low_width, low_height, nullptr, nullptr, dc.d_uplow, hip_stream,
                                (flags & BRT_FLAG_CALLER_STREAM) | post, stats);
    if (r != BRT_OK) return r;
    HIP_TRY(ctx, hipSetDevice(dc.device));
    return BRT_OK;
}

int32_t render_upscaled_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t low_width, uint32_t low_height,
                               uint32_t width, uint32_t height, void* d_frame, void* hip_stream, uint32_t flags, brt_stats* stats,
                               Blend bl) {
    if (!camera80 || !window16) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "camera/window is null");
    if (!d_frame) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_frame is null");
    if (const int32_t bad = flags_check(ctx, flags, kOutPostFlags, "flags: BRT_FLAG_CALLER_STREAM, BRT_FLAG_OUT_*, BRT_FLAG_DENOISE and BRT_FLAG_TEMPORAL only"))
        return bad;
    if (const int32_t bad = level_check(ctx, &bl)) return bad;
    if (const int32_t bad = sizes_check(ctx, low_width, low_height, width, height)) return bad;
    if (const int32_t bad = raster_overlap_check(ctx, bl, d_frame, width, height, flags & BRT_FLAG_OUT_MASK)) return bad;
    if (!ctx->has_scene) return ctx_fail(ctx, BRT_ERR_NO_SCENE, "brt_upload_scene has not succeeded yet");
    char low_win[16];
    low_window(window16, height, low_height, low_win);
    const uint32_t post = flags & (BRT_FLAG_DENOISE | BRT_FLAG_TEMPORAL);
    return frame_call(ctx, camera80, hip_stream, flags, stats, FRAME_STATS_KEEP, [&](DeviceCtx& dc, const StreamChoice& sc) -> int32_t {
        const int32_t r = low_frame(ctx, dc, sc, camera80, low_win, low_width, low_height, hip_stream, flags, post, stats);
        if (r != BRT_OK) return r;
        return upscale_enqueue(ctx, dc, camera80, low_win, low_width, low_height, dc.d_uplow, window16, width, height, d_frame,
                               flags & BRT_FLAG_OUT_MASK, sc.stream, post != 0u, bl);  // (the post-passes cast the low guides: not cast twice)
    });
}

// ---- refined upsampling (DESIGN.md "Refined upsampling") ------------------------------------------------------------------------------

int32_t refine_check(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t low_width, uint32_t low_height, uint32_t width,
                     uint32_t height, uint32_t classes) {
    if (!camera80 || !window16) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "camera/window is null");
    if (classes == 0u || (classes & ~(uint32_t)(BRT_REFINE_EDGES | BRT_REFINE_SPECULAR)))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "classes: a non-empty mask of BRT_REFINE_EDGES and BRT_REFINE_SPECULAR");
    if (const int32_t bad = sizes_check(ctx, low_width, low_height, width, height)) return bad;
    if (!ctx->has_scene) return ctx_fail(ctx, BRT_ERR_NO_SCENE, "brt_upload_scene has not succeeded yet");
    if (ctx->policy_flags & kPolicyMask)
        return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, "the pixel tracer implements the default policy only (brt_set_policy)");
    return BRT_OK;
}

// behind the low frame at d_low on `stream`: the selecting upsampling into d_out, then the selected pixels traced into it with the
// full-size window; the count to d_count (or nullptr)
int32_t refine_enqueue(brt_ctx* ctx, DeviceCtx& dc, const void* camera80, const void* window16, const void* low_window16, uint32_t low_width,
                       uint32_t low_height, const float* d_low, uint32_t width, uint32_t height, void* d_out, uint32_t out_format,
                       uint32_t classes, uint32_t* d_count, hipStream_t stream) {
    SelectList sl;
    int32_t rc = refine_list(ctx, dc, width, height, stream, &sl);
    if (rc != BRT_OK) return rc;
    const UpscaleSelect us = {classes, sl.count, sl.list, nullptr};
    rc = upscale_enqueue(ctx, dc, camera80, low_window16, low_width, low_height, d_low, window16, width, height, d_out, out_format, stream,
                         false, Blend(), &us);
    if (rc != BRT_OK) return rc;
    return trace_selected(ctx, dc, camera80, window16, width, height, sl, d_out, out_format, d_count, stream);
}

}  // namespace

extern "C" {

int32_t brt_upscale_refine_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t low_width, uint32_t low_height,
                                  const float* d_low_rgba, uint32_t width, uint32_t height, void* d_out, uint32_t classes,
                                  uint32_t* d_refined_count_or_null, void* hip_stream, uint32_t flags, brt_stats* stats) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (!d_low_rgba || !d_out) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_low_rgba / d_out is null");
    if (const int32_t bad = flags_check(ctx, flags, kOutFlags, "flags: BRT_FLAG_CALLER_STREAM and BRT_FLAG_OUT_* only")) return bad;
    if (const int32_t bad = refine_check(ctx, camera80, window16, low_width, low_height, width, height, classes)) return bad;
    const uint32_t fmt = flags & BRT_FLAG_OUT_MASK;
    if (overlaps(d_out, out_bytes(width, height, fmt), d_low_rgba, (size_t)low_width * low_height * 16u))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_out overlaps d_low_rgba");
    if (overlaps(d_out, out_bytes(width, height, fmt), d_refined_count_or_null, 4u))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_out overlaps d_refined_count");
    return frame_call(ctx, camera80, hip_stream, flags, stats, FRAME_STATS_CLEAR, [&](DeviceCtx& dc, const StreamChoice& sc) -> int32_t {
        return refine_enqueue(ctx, dc, camera80, window16, window16, low_width, low_height, d_low_rgba, width, height, d_out, fmt, classes,
                              d_refined_count_or_null, sc.stream);
    });
    });
}

int32_t brt_render_upscaled_refined_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t low_width,
                                           uint32_t low_height, uint32_t width, uint32_t height, void* d_frame, uint32_t classes,
                                           uint32_t* d_refined_count_or_null, void* hip_stream, uint32_t flags, brt_stats* stats) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (!d_frame) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_frame is null");
    if (const int32_t bad = flags_check(ctx, flags, kOutFlags, "flags: BRT_FLAG_CALLER_STREAM and BRT_FLAG_OUT_* only (refined pixels are raw samples: no post-pass)"))
        return bad;
    if (const int32_t bad = refine_check(ctx, camera80, window16, low_width, low_height, width, height, classes)) return bad;
    const uint32_t fmt = flags & BRT_FLAG_OUT_MASK;
    if (overlaps(d_frame, out_bytes(width, height, fmt), d_refined_count_or_null, 4u))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_frame overlaps d_refined_count");
    char low_win[16];
    low_window(window16, height, low_height, low_win);
    return frame_call(ctx, camera80, hip_stream, flags, stats, FRAME_STATS_KEEP, [&](DeviceCtx& dc, const StreamChoice& sc) -> int32_t {
        const int32_t r = low_frame(ctx, dc, sc, camera80, low_win, low_width, low_height, hip_stream, flags, 0u, stats);
        if (r != BRT_OK) return r;
        return refine_enqueue(ctx, dc, camera80, window16, low_win, low_width, low_height, dc.d_uplow, width, height, d_frame, fmt, classes,
                              d_refined_count_or_null, sc.stream);
    });
    });
}

int32_t brt_upscale_refine_mask_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t low_width, uint32_t low_height,
                                       const float* d_low_rgba, uint32_t width, uint32_t height, void* d_mask_u8, void* hip_stream,
                                       uint32_t flags) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (!d_low_rgba || !d_mask_u8) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_low_rgba / d_mask_u8 is null");
    if (const int32_t bad = caller_stream_flags_check(ctx, flags)) return bad;
    if (const int32_t bad = refine_check(ctx, camera80, window16, low_width, low_height, width, height, BRT_REFINE_EDGES | BRT_REFINE_SPECULAR))
        return bad;
    if (overlaps(d_mask_u8, (size_t)width * height, d_low_rgba, (size_t)low_width * low_height * 16u))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_mask_u8 overlaps d_low_rgba");
    return frame_call(ctx, camera80, hip_stream, flags, nullptr, FRAME_STATS_KEEP, [&](DeviceCtx& dc, const StreamChoice& sc) -> int32_t {
        const UpscaleSelect us = {BRT_REFINE_EDGES | BRT_REFINE_SPECULAR, nullptr, nullptr, static_cast<uint8_t*>(d_mask_u8)};
        return upscale_enqueue(ctx, dc, camera80, window16, low_width, low_height, d_low_rgba, window16, width, height, nullptr,
                               BRT_FLAG_OUT_RGBA32F, sc.stream, false, Blend(), &us);
    });
    });
}

int32_t brt_upscale_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t low_width, uint32_t low_height,
                           const float* d_low_rgba, uint32_t width, uint32_t height, void* d_out, void* hip_stream, uint32_t flags,
                           brt_stats* stats) {
    return ctx_guard(ctx, [&]() -> int32_t {
    return upscale_device(ctx, camera80, window16, low_width, low_height, d_low_rgba, width, height, d_out, hip_stream, flags, stats, Blend());
    });
}

int32_t brt_upscale_blend_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t level, uint32_t low_width,
                                 uint32_t low_height, const float* d_low_rgba, uint32_t width, uint32_t height,
                                 const float* d_raster_rgba_or_null, const float* d_raster_depth_or_null, void* d_out, void* hip_stream,
                                 uint32_t flags, brt_stats* stats) {
    return ctx_guard(ctx, [&]() -> int32_t {
    return upscale_device(ctx, camera80, window16, low_width, low_height, d_low_rgba, width, height, d_out, hip_stream, flags, stats,
                          Blend{level, d_raster_rgba_or_null, d_raster_depth_or_null});
    });
}

int32_t brt_render_upscaled_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t low_width, uint32_t low_height,
                                   uint32_t width, uint32_t height, void* d_frame, void* hip_stream, uint32_t flags, brt_stats* stats) {
    return ctx_guard(ctx, [&]() -> int32_t {
    return render_upscaled_device(ctx, camera80, window16, low_width, low_height, width, height, d_frame, hip_stream, flags, stats, Blend());
    });
}

int32_t brt_render_upscaled_blend_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t level, uint32_t low_width,
                                         uint32_t low_height, uint32_t width, uint32_t height, const float* d_raster_rgba_or_null,
                                         const float* d_raster_depth_or_null, void* d_frame, void* hip_stream, uint32_t flags,
                                         brt_stats* stats) {
    return ctx_guard(ctx, [&]() -> int32_t {
    return render_upscaled_device(ctx, camera80, window16, low_width, low_height, width, height, d_frame, hip_stream, flags, stats,
                                  Blend{level, d_raster_rgba_or_null, d_raster_depth_or_null});
    });
}

// resolve_pixel's compare (brt_device.h) for ONE sample of depth t, every operation a separately rounded f32 one: the rule of k_upscale's
// blended form (brt_upscale.hip blend_covered) on the host
int32_t brt_host_blend_covered(const void* camera80, uint32_t level, float t, float raster_depth, uint32_t* out_covered) {
    return guard(nullptr, [&]() -> int32_t {
    if (!camera80 || !out_covered) return fail(BRT_ERR_INVALID_ARGUMENT, "null pointer");
    if (const int32_t bad = frame_level_check(nullptr, level, "level 0 traces nothing")) return bad;
    Camera cam;
    std::memcpy(&cam, camera80, sizeof cam);
    *out_covered = 0u;
    if (level == BRT_LEVEL_PURE) return BRT_OK;                                   // (no blend)
    const float fallback_far = level == BRT_LEVEL_FALLBACK_RASTER ? cam.far_ + 10.0f : cam.far_ - 1.0f;
    const float depth = t == std::numeric_limits<float>::infinity() ? fallback_far : t;
    const float rd = depth > cam.far_ ? -1.0f : cam.near_ / depth;
    *out_covered = raster_depth > rd ? 1u : 0u;
    return BRT_OK;
    });
}

int32_t brt_host_upscale_window(const void* window16, uint32_t height, uint32_t low_height, void* out_window16) {
    return guard(nullptr, [&]() -> int32_t {
    if (!window16 || !out_window16) return fail(BRT_ERR_INVALID_ARGUMENT, "null pointer");
    if (height == 0u || low_height == 0u || low_height > height) return fail(BRT_ERR_INVALID_ARGUMENT, "1 <= low_height <= height");
    low_window(window16, height, low_height, out_window16);
    return BRT_OK;
    });
}

}  // extern "C"
