// brt_api_upscale.cpp -- guide-buffer upsampling on the first device (brt_upscale.hip): of a low frame the caller holds, and of one the
// call traces (and post-processes) itself.  DESIGN.md "Guide-buffer upsampling".
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

// behind the low frame at d_low on `stream`: its guides unless a post-pass has just left them in the scratch, then the upsampling into
// d_out; the scratch is the denoiser's and the event its ordering event, so the call queues up with the context's other post-passes
int32_t upscale_enqueue(brt_ctx* ctx, DeviceCtx& dc, const void* camera80, const void* low_window16, uint32_t low_width, uint32_t low_height,
                        const float* d_low, const void* window16, uint32_t width, uint32_t height, void* d_out, uint32_t out_format,
                        hipStream_t stream, bool guides_resident) {
    FrameParams low, full;
    DenoiseScratch ds;
    int32_t rc = make_frame_params(ctx, camera80, window16, BRT_LEVEL_PURE, width, height, 0u, 1u, &full);
    if (rc == BRT_OK) rc = denoise_begin(ctx, dc, camera80, low_window16, low_width, low_height, stream, &low, &ds);
    if (rc != BRT_OK) return rc;
    if (!guides_resident) HIP_TRY(ctx, launch_denoise_guides(dc.view, low, ds, stream));
    HIP_TRY(ctx, launch_upscale(dc.view, full, low, ctx->denoise, ds, d_low, d_out, out_format, stream));
    HIP_TRY(ctx, hipEventRecord(dc.ev_dn, stream));
    return BRT_OK;
}

int32_t upscale_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t low_width, uint32_t low_height,
                       const float* d_low_rgba, uint32_t width, uint32_t height, void* d_out, void* hip_stream, uint32_t flags,
                       brt_stats* stats) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!ctx) return fail(BRT_ERR_INVALID_ARGUMENT, "ctx is null");
    if (!camera80 || !window16) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "camera/window is null");
    if (!d_low_rgba || !d_out) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_low_rgba / d_out is null");
    if (flags & ~(uint32_t)(BRT_FLAG_CALLER_STREAM | BRT_FLAG_OUT_MASK))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "flags: BRT_FLAG_CALLER_STREAM and BRT_FLAG_OUT_* only");
    if (const int32_t bad = sizes_check(ctx, low_width, low_height, width, height)) return bad;
    const uint32_t fmt = flags & BRT_FLAG_OUT_MASK;
    const size_t out_px = fmt == BRT_FLAG_OUT_RGBA32F ? 16u : fmt == BRT_FLAG_OUT_RGBA16F ? 8u : 4u;
    const char* lo = reinterpret_cast<const char*>(d_low_rgba);
    const char* out = static_cast<const char*>(d_out);
    if (lo < out + (size_t)width * height * out_px && out < lo + (size_t)low_width * low_height * 16u)
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_out overlaps d_low_rgba");
    if (!ctx->has_scene) return ctx_fail(ctx, BRT_ERR_NO_SCENE, "brt_upload_scene has not succeeded yet");
    DeviceCtx& dc = ctx->devs[0];
    const int32_t rc = with_tree_reach(ctx, camera80, BRT_LEVEL_PURE, stats, [&]() -> int32_t {     // (the guides walk the tree of the frame)
        HIP_TRY(ctx, hipSetDevice(dc.device));
        const StreamChoice sc = stream_of(dc, hip_stream, flags);
        const int32_t r = upscale_enqueue(ctx, dc, camera80, window16, low_width, low_height, d_low_rgba, window16, width, height, d_out, fmt,
                                          sc.stream, false);
        if (r == BRT_OK && sc.own) HIP_TRY(ctx, hipStreamSynchronize(sc.stream));
        if (r == BRT_OK && stats) std::memset(stats, 0, sizeof *stats);      // (total_ms only, and the tree)
        return r;
    });
    if (rc == BRT_OK && stats) stats->total_ms = ms_since(t0);
    return rc;
}

int32_t render_upscaled_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t low_width, uint32_t low_height,
                               uint32_t width, uint32_t height, void* d_frame, void* hip_stream, uint32_t flags, brt_stats* stats) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!ctx) return fail(BRT_ERR_INVALID_ARGUMENT, "ctx is null");
    if (!camera80 || !window16) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "camera/window is null");
    if (!d_frame) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_frame is null");
    if (flags & ~(uint32_t)(BRT_FLAG_CALLER_STREAM | BRT_FLAG_OUT_MASK | BRT_FLAG_DENOISE | BRT_FLAG_TEMPORAL))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "flags: BRT_FLAG_CALLER_STREAM, BRT_FLAG_OUT_*, BRT_FLAG_DENOISE and BRT_FLAG_TEMPORAL only");
    if (const int32_t bad = sizes_check(ctx, low_width, low_height, width, height)) return bad;
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
        // exactly brt_render_device's low_width x low_height Pure frame (every device of the context), post-passes on the low frame
        r = render_frame_device(ctx, camera80, low_win, BRT_LEVEL_PURE, low_width, low_height, nullptr, nullptr, dc.d_uplow, hip_stream,
                                (flags & BRT_FLAG_CALLER_STREAM) | post, stats);
        if (r != BRT_OK) return r;
        HIP_TRY(ctx, hipSetDevice(dc.device));
        r = upscale_enqueue(ctx, dc, camera80, low_win, low_width, low_height, dc.d_uplow, window16, width, height, d_frame,
                            flags & BRT_FLAG_OUT_MASK, sc.stream, post != 0u);  // (the post-passes cast the low guides: not cast twice)
        if (r == BRT_OK && sc.own) HIP_TRY(ctx, hipStreamSynchronize(sc.stream));
        return r;
    });
    if (rc == BRT_OK && stats) stats->total_ms = ms_since(t0);
    return rc;
}

}  // namespace

extern "C" {

int32_t brt_upscale_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t low_width, uint32_t low_height,
                           const float* d_low_rgba, uint32_t width, uint32_t height, void* d_out, void* hip_stream, uint32_t flags,
                           brt_stats* stats) {
    return guard(ctx ? &ctx->last_error : nullptr, [&]() -> int32_t {
    return upscale_device(ctx, camera80, window16, low_width, low_height, d_low_rgba, width, height, d_out, hip_stream, flags, stats);
    });
}

int32_t brt_render_upscaled_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t low_width, uint32_t low_height,
                                   uint32_t width, uint32_t height, void* d_frame, void* hip_stream, uint32_t flags, brt_stats* stats) {
    return guard(ctx ? &ctx->last_error : nullptr, [&]() -> int32_t {
    return render_upscaled_device(ctx, camera80, window16, low_width, low_height, width, height, d_frame, hip_stream, flags, stats);
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
