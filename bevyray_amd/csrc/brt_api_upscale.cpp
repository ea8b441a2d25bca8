// brt_api_upscale.cpp -- guide-buffer upsampling on the first device (brt_upscale.hip): of a low frame the caller holds, and of one the
// call traces (and post-processes) itself.  DESIGN.md "Guide-buffer upsampling"; with a level and the full-size raster inputs
// (brt_upscale_blend_device, brt_render_upscaled_blend_device): "Upsampling blended frames".
#include "brt_frame.h"

using namespace brt;

namespace brt {

bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const char* pa = static_cast<const char*>(a);
    const char* pb = static_cast<const char*>(b);
    return a && b && pa < pb + b_bytes && pb < pa + a_bytes;
}

size_t out_bytes(uint32_t width, uint32_t height, uint32_t fmt) {
    return (size_t)width * height * (fmt == BRT_FLAG_OUT_RGBA32F ? 16u : fmt == BRT_FLAG_OUT_RGBA16F ? 8u : 4u);
}

// The control words and the list of a width x height refinement or adaptive frame (DeviceCtx::d_pxbuf) for work on `stream`: a larger
// one is allocated only once the last user of the old one has ended; the control words are zeroed behind that user
int32_t refine_list(brt_ctx* ctx, DeviceCtx& dc, uint32_t width, uint32_t height, hipStream_t stream) {
    const size_t bytes = 32u + (size_t)width * height * 4u;
    if (dc.pxbuf_cap < bytes) HIP_TRY(ctx, hipEventSynchronize(dc.ev_q));
    const int32_t rc = ensure(ctx, &dc.d_pxbuf, &dc.pxbuf_cap, bytes);
    if (rc != BRT_OK) return rc;
    HIP_TRY(ctx, hipStreamWaitEvent(stream, dc.ev_q, 0));
    HIP_TRY(ctx, hipMemsetAsync(dc.d_pxbuf, 0, 32, stream));
    return BRT_OK;
}

}  // namespace brt

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
    if (bl->level == BRT_LEVEL_SKIP) return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, "level 0 traces nothing: there is no frame to upsample");
    if (bl->level != BRT_LEVEL_FALLBACK_RASTER && bl->level != BRT_LEVEL_FALLBACK_RAYTRACED && bl->level != BRT_LEVEL_PURE)
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "level must be 1, 2 or 3");
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
    const auto t0 = std::chrono::steady_clock::now();
    if (!ctx) return fail(BRT_ERR_INVALID_ARGUMENT, "ctx is null");
    if (!camera80 || !window16) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "camera/window is null");
    if (!d_low_rgba || !d_out) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_low_rgba / d_out is null");
    if (flags & ~(uint32_t)(BRT_FLAG_CALLER_STREAM | BRT_FLAG_OUT_MASK))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "flags: BRT_FLAG_CALLER_STREAM and BRT_FLAG_OUT_* only");
    if (const int32_t bad = level_check(ctx, &bl)) return bad;
    if (const int32_t bad = sizes_check(ctx, low_width, low_height, width, height)) return bad;
    const uint32_t fmt = flags & BRT_FLAG_OUT_MASK;
    if (overlaps(d_out, out_bytes(width, height, fmt), d_low_rgba, (size_t)low_width * low_height * 16u))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_out overlaps d_low_rgba");
    if (const int32_t bad = raster_overlap_check(ctx, bl, d_out, width, height, fmt)) return bad;
    if (!ctx->has_scene) return ctx_fail(ctx, BRT_ERR_NO_SCENE, "brt_upload_scene has not succeeded yet");
    DeviceCtx& dc = ctx->devs[0];
    const int32_t rc = with_tree_reach(ctx, camera80, BRT_LEVEL_PURE, stats, [&]() -> int32_t {     // (the guides walk the tree of the frame)
        HIP_TRY(ctx, hipSetDevice(dc.device));
        const StreamChoice sc = stream_of(dc, hip_stream, flags);
        const int32_t r = upscale_enqueue(ctx, dc, camera80, window16, low_width, low_height, d_low_rgba, window16, width, height, d_out, fmt,
                                          sc.stream, false, bl);
        if (r == BRT_OK && sc.own) HIP_TRY(ctx, hipStreamSynchronize(sc.stream));
        if (r == BRT_OK && stats) std::memset(stats, 0, sizeof *stats);      // (total_ms only, and the tree)
        return r;
    });
    if (rc == BRT_OK && stats) stats->total_ms = ms_since(t0);
    return rc;
}

int32_t render_upscaled_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t low_width, uint32_t low_height,
                               uint32_t width, uint32_t height, void* d_frame, void* hip_stream, uint32_t flags, brt_stats* stats,
                               Blend bl) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!ctx) return fail(BRT_ERR_INVALID_ARGUMENT, "ctx is null");
    if (!camera80 || !window16) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "camera/window is null");
    if (!d_frame) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_frame is null");
    if (flags & ~(uint32_t)(BRT_FLAG_CALLER_STREAM | BRT_FLAG_OUT_MASK | BRT_FLAG_DENOISE | BRT_FLAG_TEMPORAL))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "flags: BRT_FLAG_CALLER_STREAM, BRT_FLAG_OUT_*, BRT_FLAG_DENOISE and BRT_FLAG_TEMPORAL only");
    if (const int32_t bad = level_check(ctx, &bl)) return bad;
    if (const int32_t bad = sizes_check(ctx, low_width, low_height, width, height)) return bad;
    if (const int32_t bad = raster_overlap_check(ctx, bl, d_frame, width, height, flags & BRT_FLAG_OUT_MASK)) return bad;
    if (!ctx->has_scene) return ctx_fail(ctx, BRT_ERR_NO_SCENE, "brt_upload_scene has not succeeded yet");
    char low_win[16];
    low_window(window16, height, low_height, low_win);
    DeviceCtx& dc = ctx->devs[0];
    const uint32_t post = flags & (BRT_FLAG_DENOISE | BRT_FLAG_TEMPORAL);
    const int32_t rc = with_tree_reach(ctx, camera80, BRT_LEVEL_PURE, stats, [&]() -> int32_t {
        HIP_TRY(ctx, hipSetDevice(dc.device));
        const StreamChoice sc = stream_of(dc, hip_stream, flags);
        // the low frame lives in the context: a larger one is allocated only once the last upsampling has read the old one, and the
        // trace writes it behind that upsampling on whatever stream it ran
        const size_t bytes = (size_t)low_width * low_height * 16u;
        if (dc.uplow_cap < bytes) HIP_TRY(ctx, hipEventSynchronize(dc.ev_dn));
        int32_t r = ensure(ctx, &dc.d_uplow, &dc.uplow_cap, bytes);
        if (r != BRT_OK) return r;
        HIP_TRY(ctx, hipStreamWaitEvent(sc.stream, dc.ev_dn, 0));
        // exactly brt_render_device's low_width x low_height Pure frame (every device of the context), post-passes on the low frame;
        // whatever the level of the presented frame: its raster blend is decided per output pixel by the upsampling
        r = render_frame_device(ctx, camera80, low_win, BRT_LEVEL_PURE, low_width, low_height, nullptr, nullptr, dc.d_uplow, hip_stream,
                                (flags & BRT_FLAG_CALLER_STREAM) | post, stats);
        if (r != BRT_OK) return r;
        HIP_TRY(ctx, hipSetDevice(dc.device));
        r = upscale_enqueue(ctx, dc, camera80, low_win, low_width, low_height, dc.d_uplow, window16, width, height, d_frame,
                            flags & BRT_FLAG_OUT_MASK, sc.stream, post != 0u, bl);  // (the post-passes cast the low guides: not cast twice)
        if (r == BRT_OK && sc.own) HIP_TRY(ctx, hipStreamSynchronize(sc.stream));
        return r;
    });
    if (rc == BRT_OK && stats) stats->total_ms = ms_since(t0);
    return rc;
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
    int32_t rc = refine_list(ctx, dc, width, height, stream);
    if (rc != BRT_OK) return rc;
    const UpscaleSelect us = {classes, dc.d_pxbuf + 5, dc.d_pxbuf + 8, nullptr};
    rc = upscale_enqueue(ctx, dc, camera80, low_window16, low_width, low_height, d_low, window16, width, height, d_out, out_format, stream,
                         false, Blend(), &us);
    if (rc != BRT_OK) return rc;
    PixelsLaunch pl{};
    rc = pixels_enqueue(ctx, dc, camera80, window16, width, height, us.list, width * height, us.count, {d_out, true, out_format}, dc.d_pxbuf,
                        stream, false, &pl);
    if (rc != BRT_OK) return rc;
    if (d_count) HIP_TRY(ctx, hipMemcpyAsync(d_count, us.count, 4, hipMemcpyDeviceToDevice, stream));
    HIP_TRY(ctx, hipEventRecord(dc.ev_q, stream));
    return BRT_OK;
}

}  // namespace

extern "C" {

int32_t brt_upscale_refine_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t low_width, uint32_t low_height,
                                  const float* d_low_rgba, uint32_t width, uint32_t height, void* d_out, uint32_t classes,
                                  uint32_t* d_refined_count_or_null, void* hip_stream, uint32_t flags, brt_stats* stats) {
    return guard(ctx ? &ctx->last_error : nullptr, [&]() -> int32_t {
    const auto t0 = std::chrono::steady_clock::now();
    if (!ctx) return fail(BRT_ERR_INVALID_ARGUMENT, "ctx is null");
    if (!d_low_rgba || !d_out) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_low_rgba / d_out is null");
    if (flags & ~(uint32_t)(BRT_FLAG_CALLER_STREAM | BRT_FLAG_OUT_MASK))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "flags: BRT_FLAG_CALLER_STREAM and BRT_FLAG_OUT_* only");
    if (const int32_t bad = refine_check(ctx, camera80, window16, low_width, low_height, width, height, classes)) return bad;
    const uint32_t fmt = flags & BRT_FLAG_OUT_MASK;
    if (overlaps(d_out, out_bytes(width, height, fmt), d_low_rgba, (size_t)low_width * low_height * 16u))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_out overlaps d_low_rgba");
    if (overlaps(d_out, out_bytes(width, height, fmt), d_refined_count_or_null, 4u))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_out overlaps d_refined_count");
    DeviceCtx& dc = ctx->devs[0];
    const int32_t rc = with_tree_reach(ctx, camera80, BRT_LEVEL_PURE, stats, [&]() -> int32_t {
        HIP_TRY(ctx, hipSetDevice(dc.device));
        const StreamChoice sc = stream_of(dc, hip_stream, flags);
        const int32_t r = refine_enqueue(ctx, dc, camera80, window16, window16, low_width, low_height, d_low_rgba, width, height, d_out, fmt,
                                         classes, d_refined_count_or_null, sc.stream);
        if (r == BRT_OK && sc.own) HIP_TRY(ctx, hipStreamSynchronize(sc.stream));
        if (r == BRT_OK && stats) std::memset(stats, 0, sizeof *stats);      // (total_ms only, and the tree)
        return r;
    });
    if (rc == BRT_OK && stats) stats->total_ms = ms_since(t0);
    return rc;
    });
}

int32_t brt_render_upscaled_refined_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t low_width,
                                           uint32_t low_height, uint32_t width, uint32_t height, void* d_frame, uint32_t classes,
                                           uint32_t* d_refined_count_or_null, void* hip_stream, uint32_t flags, brt_stats* stats) {
    return guard(ctx ? &ctx->last_error : nullptr, [&]() -> int32_t {
    const auto t0 = std::chrono::steady_clock::now();
    if (!ctx) return fail(BRT_ERR_INVALID_ARGUMENT, "ctx is null");
    if (!d_frame) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_frame is null");
    if (flags & ~(uint32_t)(BRT_FLAG_CALLER_STREAM | BRT_FLAG_OUT_MASK))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "flags: BRT_FLAG_CALLER_STREAM and BRT_FLAG_OUT_* only (refined pixels are raw samples: no post-pass)");
    if (const int32_t bad = refine_check(ctx, camera80, window16, low_width, low_height, width, height, classes)) return bad;
    const uint32_t fmt = flags & BRT_FLAG_OUT_MASK;
    if (overlaps(d_frame, out_bytes(width, height, fmt), d_refined_count_or_null, 4u))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_frame overlaps d_refined_count");
    char low_win[16];
    low_window(window16, height, low_height, low_win);
    DeviceCtx& dc = ctx->devs[0];
    const int32_t rc = with_tree_reach(ctx, camera80, BRT_LEVEL_PURE, stats, [&]() -> int32_t {
        HIP_TRY(ctx, hipSetDevice(dc.device));
        const StreamChoice sc = stream_of(dc, hip_stream, flags);
        // the low frame of the context, as brt_render_upscaled_device keeps it
        const size_t bytes = (size_t)low_width * low_height * 16u;
        if (dc.uplow_cap < bytes) HIP_TRY(ctx, hipEventSynchronize(dc.ev_dn));
        int32_t r = ensure(ctx, &dc.d_uplow, &dc.uplow_cap, bytes);
        if (r != BRT_OK) return r;
        HIP_TRY(ctx, hipStreamWaitEvent(sc.stream, dc.ev_dn, 0));
        r = render_frame_device(ctx, camera80, low_win, BRT_LEVEL_PURE, low_width, low_height, nullptr, nullptr, dc.d_uplow, hip_stream,
                                flags & BRT_FLAG_CALLER_STREAM, stats);
        if (r != BRT_OK) return r;
        HIP_TRY(ctx, hipSetDevice(dc.device));
        r = refine_enqueue(ctx, dc, camera80, window16, low_win, low_width, low_height, dc.d_uplow, width, height, d_frame, fmt, classes,
                           d_refined_count_or_null, sc.stream);
        if (r == BRT_OK && sc.own) HIP_TRY(ctx, hipStreamSynchronize(sc.stream));
        return r;
    });
    if (rc == BRT_OK && stats) stats->total_ms = ms_since(t0);
    return rc;
    });
}

int32_t brt_upscale_refine_mask_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t low_width, uint32_t low_height,
                                       const float* d_low_rgba, uint32_t width, uint32_t height, void* d_mask_u8, void* hip_stream,
                                       uint32_t flags) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (!d_low_rgba || !d_mask_u8) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_low_rgba / d_mask_u8 is null");
    if (flags & ~(uint32_t)BRT_FLAG_CALLER_STREAM) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "flags: BRT_FLAG_CALLER_STREAM only");
    if (const int32_t bad = refine_check(ctx, camera80, window16, low_width, low_height, width, height, BRT_REFINE_EDGES | BRT_REFINE_SPECULAR))
        return bad;
    if (overlaps(d_mask_u8, (size_t)width * height, d_low_rgba, (size_t)low_width * low_height * 16u))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_mask_u8 overlaps d_low_rgba");
    DeviceCtx& dc = ctx->devs[0];
    return with_tree_reach(ctx, camera80, BRT_LEVEL_PURE, nullptr, [&]() -> int32_t {
        HIP_TRY(ctx, hipSetDevice(dc.device));
        const StreamChoice sc = stream_of(dc, hip_stream, flags);
        const UpscaleSelect us = {BRT_REFINE_EDGES | BRT_REFINE_SPECULAR, nullptr, nullptr, static_cast<uint8_t*>(d_mask_u8)};
        const int32_t r = upscale_enqueue(ctx, dc, camera80, window16, low_width, low_height, d_low_rgba, window16, width, height, nullptr,
                                          BRT_FLAG_OUT_RGBA32F, sc.stream, false, Blend(), &us);
        if (r == BRT_OK && sc.own) HIP_TRY(ctx, hipStreamSynchronize(sc.stream));
        return r;
    });
    });
}

int32_t brt_upscale_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t low_width, uint32_t low_height,
                           const float* d_low_rgba, uint32_t width, uint32_t height, void* d_out, void* hip_stream, uint32_t flags,
                           brt_stats* stats) {
    return guard(ctx ? &ctx->last_error : nullptr, [&]() -> int32_t {
    return upscale_device(ctx, camera80, window16, low_width, low_height, d_low_rgba, width, height, d_out, hip_stream, flags, stats, Blend());
    });
}

int32_t brt_upscale_blend_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t level, uint32_t low_width,
                                 uint32_t low_height, const float* d_low_rgba, uint32_t width, uint32_t height,
                                 const float* d_raster_rgba_or_null, const float* d_raster_depth_or_null, void* d_out, void* hip_stream,
                                 uint32_t flags, brt_stats* stats) {
    return guard(ctx ? &ctx->last_error : nullptr, [&]() -> int32_t {
    Blend bl;
    bl.level = level;
    bl.d_raster_rgba = d_raster_rgba_or_null;
    bl.d_raster_depth = d_raster_depth_or_null;
    return upscale_device(ctx, camera80, window16, low_width, low_height, d_low_rgba, width, height, d_out, hip_stream, flags, stats, bl);
    });
}

int32_t brt_render_upscaled_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t low_width, uint32_t low_height,
                                   uint32_t width, uint32_t height, void* d_frame, void* hip_stream, uint32_t flags, brt_stats* stats) {
    return guard(ctx ? &ctx->last_error : nullptr, [&]() -> int32_t {
    return render_upscaled_device(ctx, camera80, window16, low_width, low_height, width, height, d_frame, hip_stream, flags, stats, Blend());
    });
}

int32_t brt_render_upscaled_blend_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t level, uint32_t low_width,
                                         uint32_t low_height, uint32_t width, uint32_t height, const float* d_raster_rgba_or_null,
                                         const float* d_raster_depth_or_null, void* d_frame, void* hip_stream, uint32_t flags,
                                         brt_stats* stats) {
    return guard(ctx ? &ctx->last_error : nullptr, [&]() -> int32_t {
    Blend bl;
    bl.level = level;
    bl.d_raster_rgba = d_raster_rgba_or_null;
    bl.d_raster_depth = d_raster_depth_or_null;
    return render_upscaled_device(ctx, camera80, window16, low_width, low_height, width, height, d_frame, hip_stream, flags, stats, bl);
    });
}

// resolve_pixel's compare (brt_device.h) for ONE sample of depth t, every operation a separately rounded f32 one: the rule of k_upscale's
// blended form (brt_upscale.hip blend_covered) on the host
int32_t brt_host_blend_covered(const void* camera80, uint32_t level, float t, float raster_depth, uint32_t* out_covered) {
    return guard(nullptr, [&]() -> int32_t {
    if (!camera80 || !out_covered) return fail(BRT_ERR_INVALID_ARGUMENT, "null pointer");
    if (level == BRT_LEVEL_SKIP) return fail(BRT_ERR_UNSUPPORTED, "level 0 traces nothing");
    if (level != BRT_LEVEL_FALLBACK_RASTER && level != BRT_LEVEL_FALLBACK_RAYTRACED && level != BRT_LEVEL_PURE)
        return fail(BRT_ERR_INVALID_ARGUMENT, "level must be 1, 2 or 3");
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
