// brt_api_gbuffer.cpp -- the G-buffer of a frame (brt_gbuffer.h, brt_gbuffer.hip; DESIGN.md "G-buffer") on the first device.  A call is a
// list call in everything but its shape: the tree follows the camera (ensure_tree_reach, as for a render), the kernel runs behind the
// previous query or list of the context (ev_q, which it records, so uploads and tree rebuilds wait for it as they do for queries), with the
// queries' resident -> caller sphere map (query_rmap) and their control words (d_qctl).  It keeps nothing in the context: no frame, no
// dispatch history, no temporal history, no denoiser scratch.  The skeleton of a call is written once for both forms (gbuffer_call); the
// host form is the device form's enqueue inside the round trip of the caller's planes (brt_frame.h host_round_trip), its stats are
// list_stats8's.  The host twin of the rule (brt_host_gbuffer_pixel) needs no context.
#include "brt_frame.h"
#include "brt_gbuffer_launch.h"

using namespace brt;

namespace {

struct GbufferCall {
    brt_gbuffer desc;
    Camera cam, prev;
    Window win;
};

// what needs no context: the message names the field
int32_t gbuffer_desc_check(brt_ctx* ctx, const void* camera80, const void* window16, const void* gbuffer32, const void* prev_camera80,
                           uint32_t width, uint32_t height, GbufferCall* gc) {
    if (!camera80 || !window16) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "camera/window is null");
    if (!gbuffer32) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "gbuffer is null");
    std::memcpy(&gc->desc, gbuffer32, sizeof gc->desc);
    std::memcpy(&gc->cam, camera80, sizeof gc->cam);
    std::memcpy(&gc->prev, prev_camera80 ? prev_camera80 : camera80, sizeof gc->prev);
    std::memcpy(&gc->win, window16, sizeof gc->win);
    for (uint32_t r : gc->desc.reserved)
        if (r != 0u) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "gbuffer.reserved must be 0");
    if (gc->desc.depth_mode > BRT_GBUFFER_DEPTH_DISTANCE)
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "gbuffer.depth_mode must be BRT_GBUFFER_DEPTH_VIEW, _SHADER or _DISTANCE");
    if (gc->desc.normal_format > BRT_GBUFFER_NORMAL_RGB10A2)
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "gbuffer.normal_format must be BRT_GBUFFER_NORMAL_RGBA32F or _RGB10A2");
    if (gc->desc.motion_format > BRT_GBUFFER_MOTION_PIXEL)
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "gbuffer.motion_format must be BRT_GBUFFER_MOTION_UV32F, _UV16F or _PIXEL");
    if (const int32_t bad = size_check(ctx, width, height)) return bad;
    if (gc->cam.projection_type != 0u)
        return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, "camera.projection_type: the G-buffer casts pinhole rays (perspective, 0) only");
    if (gc->prev.projection_type != 0u)
        return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, "prev_camera.projection_type: the previous frame is a pinhole frame (perspective, 0) too");
    // (the rule reads neither count of the previous camera: it takes the current one's, so that nothing below refuses it under the
    //  current camera's name)
    gc->prev.sample_count = gc->cam.sample_count;
    gc->prev.bounce_count = gc->cam.bounce_count;
    return BRT_OK;
}

GbufferCam cam_of(const Camera& c) {
    return gbuffer_cam_of(c.position, c.direction, c.up, c.aspect, tan_half_fov(c.fov), c.near_, c.far_);
}

size_t normal_bytes(const brt_gbuffer& d, size_t n) { return n * (d.normal_format == BRT_GBUFFER_NORMAL_RGBA32F ? 16u : 4u); }
size_t motion_bytes(const brt_gbuffer& d, size_t n) { return n * (d.motion_format == BRT_GBUFFER_MOTION_UV16F ? 4u : 8u); }

// one frame on `stream`, behind the previous query or list of the context; counted: the five counts are gathered in d_qctl
int32_t gbuffer_enqueue(brt_ctx* ctx, DeviceCtx& dc, hipStream_t stream, const GbufferCall& gc, const void* camera80, const void* window16,
                        uint32_t width, uint32_t height, const void* d_prev_models, const void* d_cov, void* d_depth, void* d_normal,
                        void* d_motion, void* d_ids, void* d_albedo, bool counted) {
    FrameParams fp, pp;
    int32_t rc = make_frame_params(ctx, camera80, window16, BRT_LEVEL_PURE, width, height, 0u, 1u, &fp);
    if (rc == BRT_OK) rc = make_frame_params(ctx, &gc.prev, window16, BRT_LEVEL_PURE, width, height, 0u, 1u, &pp);
    if (rc != BRT_OK) return rc;
    HIP_TRY(ctx, hipStreamWaitEvent(stream, dc.ev_q, 0));
    const uint32_t* rmap = nullptr;
    rc = query_rmap(ctx, dc, stream, &rmap);
    if (rc != BRT_OK) return rc;
    GbufferArgs ga{};
    ga.gv = gbuffer_view_of(fp, pp);
    ga.depth_mode = gc.desc.depth_mode;
    ga.normal_format = gc.desc.normal_format;
    ga.motion_format = gc.desc.motion_format;
    ga.rmap = rmap;
    ga.prev_models = static_cast<const float4*>(d_prev_models);
    ga.cov = static_cast<const float4*>(d_cov);
    ga.depth = static_cast<float*>(d_depth);
    ga.normal = d_normal;
    ga.motion = d_motion;
    ga.ids = static_cast<uint4*>(d_ids);
    ga.albedo = static_cast<float4*>(d_albedo);
    ga.stat = counted ? dc.d_qctl : nullptr;
    if (counted) HIP_TRY(ctx, hipMemsetAsync(dc.d_qctl, 0, 32, stream));
    HIP_TRY(ctx, launch_gbuffer(dc.view, fp, ga, stream));
    HIP_TRY(ctx, hipEventRecord(dc.ev_q, stream));
    return BRT_OK;
}

// what every entry point checks before it touches the device
int32_t gbuffer_call_check(brt_ctx* ctx, const void* camera80, const void* window16, const void* gbuffer32, const void* prev_camera80,
                           uint32_t width, uint32_t height, uint32_t flags, GbufferCall* gc) {
    if (const int32_t bad = gbuffer_desc_check(ctx, camera80, window16, gbuffer32, prev_camera80, width, height, gc)) return bad;
    if (const int32_t bad = caller_stream_flags_check(ctx, flags)) return bad;
    if (!ctx->has_scene) return ctx_fail(ctx, BRT_ERR_NO_SCENE, "brt_upload_scene has not succeeded yet");
    if (ctx->policy_flags & kPolicyMask)
        return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, "the G-buffer implements the default policy only (brt_set_policy)");
    return BRT_OK;
}

// A call behind its argument checks, both forms: the tree a frame of this camera is traced in; a call without a plane reports its stats
// and enqueues nothing; else enqueue(dc, stream, counted) on the call's stream -- the host form's is the device form's inside
// host_round_trip; the own stream copies the five counts out and synchronises (a caller's stream is not waited for: its counts stay 0).
// out_stats8: pixels cast, hits, covered (counted calls), tree rebuilt, the callee-built tree's reach (bits), moved, no-previous, 0 (the
// two are counts of pixels: below 1 << 31)
template <class Enqueue>
int32_t gbuffer_call(brt_ctx* ctx, const void* camera80, bool any_plane, void* hip_stream, uint32_t flags, uint64_t* out_stats8, Enqueue&& enqueue) {
    uint32_t rebuilt = 0u, counts[5] = {0u, 0u, 0u, 0u, 0u};
    int32_t rc = ensure_tree_reach(ctx, camera80, &rebuilt);
    if (rc != BRT_OK) { drain_all_streams(ctx); return rc; }
    if (any_plane)
        rc = with_list_call(ctx, hip_stream, flags, [&](DeviceCtx& dc, const StreamChoice& sc) -> int32_t {
            const int32_t r = enqueue(dc, sc.stream, sc.own);
            if (r != BRT_OK || !sc.own) return r;
            HIP_TRY(ctx, hipMemcpyAsync(counts, dc.d_qctl, sizeof counts, hipMemcpyDeviceToHost, sc.stream));
            HIP_TRY(ctx, hipStreamSynchronize(sc.stream));
            return BRT_OK;
        });
    if (rc == BRT_OK) list_stats8(ctx, counts, rebuilt, (int)counts[3], counts[4], out_stats8);
    return rc;
}

}  // namespace

extern "C" {

int32_t brt_render_gbuffer_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height,
                                  const void* gbuffer32, const void* prev_camera80_or_null, const void* d_prev_models_or_null,
                                  const float* d_coverage_rgba_or_null, void* d_depth, void* d_normal, void* d_motion, void* d_ids,
                                  void* d_albedo, void* hip_stream, uint32_t flags, uint64_t* out_stats8_or_null) {
    return ctx_guard(ctx, [&]() -> int32_t {
    GbufferCall gc{};
    int32_t rc = gbuffer_call_check(ctx, camera80, window16, gbuffer32, prev_camera80_or_null, width, height, flags, &gc);
    if (rc == BRT_OK) rc = device_aligned(ctx, {d_prev_models_or_null, d_coverage_rgba_or_null, d_depth, d_normal, d_motion, d_ids, d_albedo});
    if (rc != BRT_OK) return rc;
    return gbuffer_call(ctx, camera80, d_depth || d_normal || d_motion || d_ids || d_albedo, hip_stream, flags, out_stats8_or_null,
                        [&](DeviceCtx& dc, hipStream_t stream, bool counted) {
        return gbuffer_enqueue(ctx, dc, stream, gc, camera80, window16, width, height, d_prev_models_or_null, d_coverage_rgba_or_null, d_depth,
                               d_normal, d_motion, d_ids, d_albedo, counted);
    });
    });
}

int32_t brt_render_gbuffer(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height, const void* gbuffer32,
                           const void* prev_camera80_or_null, const void* prev_models_or_null, const float* coverage_rgba_or_null,
                           void* depth, void* normal, void* motion, void* ids, void* albedo, uint64_t* out_stats8_or_null) {
    return ctx_guard(ctx, [&]() -> int32_t {
    GbufferCall gc{};
    const int32_t rc = gbuffer_call_check(ctx, camera80, window16, gbuffer32, prev_camera80_or_null, width, height, 0u, &gc);
    if (rc != BRT_OK) return rc;
    return gbuffer_call(ctx, camera80, depth || normal || motion || ids || albedo, nullptr, 0u, out_stats8_or_null,
                        [&](DeviceCtx& dc, hipStream_t stream, bool counted) {
        // a covered pixel keeps what the caller's plane holds: the planes go in as well as out when a coverage frame is bound
        const size_t n = (size_t)width * height, m = dc.view.n_models;
        auto plane = [&](void* p, size_t bytes) { return HostPlane{coverage_rgba_or_null ? p : nullptr, p, p ? bytes : 0u}; };
        return host_round_trip(ctx, dc, stream, {{prev_models_or_null, nullptr, prev_models_or_null ? m * 32u : 0u},
                                                 {coverage_rgba_or_null, nullptr, coverage_rgba_or_null ? n * 16u : 0u},
                                                 plane(depth, n * 4u), plane(normal, normal_bytes(gc.desc, n)),
                                                 plane(motion, motion_bytes(gc.desc, n)), plane(ids, n * 16u), plane(albedo, n * 16u)},
                               [&](char* const* d) {
            return gbuffer_enqueue(ctx, dc, stream, gc, camera80, window16, width, height, d[0], d[1], d[2], d[3], d[4], d[5], d[6], counted);
        });
    });
    });
}

int32_t brt_host_gbuffer_pixel(const void* camera80, const void* window16, uint32_t width, uint32_t height, uint32_t px, uint32_t py,
                               const void* gbuffer32, const void* prev_camera80_or_null, float t, const float* sphere_new4,
                               const float* sphere_old4_or_null, void* out_pixel64) {
    return guard(nullptr, [&]() -> int32_t {
    if (!out_pixel64) return fail(BRT_ERR_INVALID_ARGUMENT, "out_pixel64 is null");
    GbufferCall gc{};
    if (const int32_t bad = gbuffer_desc_check(nullptr, camera80, window16, gbuffer32, prev_camera80_or_null, width, height, &gc)) return bad;
    if (px >= width || py >= height) return fail(BRT_ERR_INVALID_ARGUMENT, "pixel outside the frame");
    const bool hit = t < std::numeric_limits<float>::infinity();
    if (hit && !sphere_new4) return fail(BRT_ERR_INVALID_ARGUMENT, "sphere_new4 is null for a hit");
    const GbufferCam cur = cam_of(gc.cam), prev = cam_of(gc.prev);
    const GbufferView gv = gbuffer_view_of(cur, prev);
    const float heightf = (float)gc.win.height;
    const float widthf = (float)gc.win.height * gc.cam.aspect;
    float d[3];
    gbuffer_host_dir(cur, 1.0f / widthf, 1.0f / heightf, width, height, px, py, d);
    const float zero[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const float* sn = hit ? sphere_new4 : zero;
    const float* so = hit && sphere_old4_or_null ? sphere_old4_or_null : sn;
    GbufferPixel g;
    gbuffer_pixel(cur, gv, gc.desc.depth_mode, width, height, px, py, d, t, sn, so, g);
    brt_gbuffer_pixel out;
    std::memset(&out, 0, sizeof out);
    out.depth = g.depth;
    out.status = g.status;
    out.normal_rgb10a2 = gbuffer_rgb10a2(g.n, hit);
    for (int k = 0; k < 3; k++) {
        out.normal[k] = g.n[k];
        out.direction[k] = d[k];
    }
    out.normal[3] = hit ? 1.0f : 0.0f;
    if (gc.desc.motion_format == BRT_GBUFFER_MOTION_UV32F) {
        std::memcpy(&out.motion[0], &g.mu, 4);
        std::memcpy(&out.motion[1], &g.mv, 4);
    } else if (gc.desc.motion_format == BRT_GBUFFER_MOTION_UV16F) {
        out.motion[0] = gbuffer_f16(g.mu) | (gbuffer_f16(g.mv) << 16);
    } else {
        std::memcpy(&out.motion[0], &g.xp, 4);
        std::memcpy(&out.motion[1], &g.yp, 4);
    }
    out.xy_prev[0] = g.xp;
    out.xy_prev[1] = g.yp;
    std::memcpy(out_pixel64, &out, sizeof out);
    return BRT_OK;
    });
}

}  // extern "C"
