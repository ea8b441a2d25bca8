// brt_api_lens.cpp -- Pure frames and pixel lists under the lens rule (brt_lens.h, brt_lens.hip; DESIGN.md "Lens frames") on the first
// device: a thin lens (depth of field) or an orthographic projection where every other entry point has a pinhole.  The call is the
// sparse pixel tracer's (pixels_call, brt_api_pixels.cpp) with the lens attached: the launch plan of every list kernel (plan_list), the
// control words and the staging buffers of the pixel lists.  The tree follows the call's camera (with_tree_reach) and then, for origins
// off the camera's position, the rule's origin bound (ensure_query_reach), which persists in query_level as after a ray query.  The
// host twin of the rule (brt_host_lens_ray, brt_host_lens_seed, brt_host_lens_origin_bound) needs no context.
#include "brt_frame.h"

using namespace brt;

namespace {

struct LensCall {
    Camera cam;                 // the caller's, projection_type included
    Window win;
    LensCam lc;
    LensView lv;
    float bound;                // lens_bound_of
};

// The rule's origin bound without a window: lens_origin_bound with |inv_height| <= 1 and |inv_width * aspect| <= 1 + 2^-22 (a window
// of at least one row; two roundings of a normal product and quotient), which needs |aspect| to be an ordinary number.
float lens_bound_of(const LensCam& c, const LensView& lv) {
    LensCam w = c;
    if (lv.mode == LENS_ORTHO) {
        if (!(std::fabs(c.aspect) >= 0x1p-100f) || !std::isfinite(c.aspect)) return std::numeric_limits<float>::infinity();
        w.inv_height = 1.0f;
        w.inv_width = (float)((1.0 + 0x1p-22) / std::fabs((double)c.aspect));
        if (!((double)w.inv_width * std::fabs((double)c.aspect) >= 1.0 + 0x1p-23)) w.inv_width = std::nextafter(w.inv_width, INFINITY);
    }
    return lens_origin_bound(w, lv);
}

// the descriptor against the camera (what no entry point takes): the message names the field
int32_t lens_check(brt_ctx* ctx, const void* camera80, const void* window16, const void* lens, LensCall* lc) {
    if (!camera80 || !window16) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "camera/window is null");
    if (!lens) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "lens is null");
    brt_lens l;
    std::memcpy(&l, lens, sizeof l);
    std::memcpy(&lc->cam, camera80, sizeof lc->cam);
    std::memcpy(&lc->win, window16, sizeof lc->win);
    const Camera& cam = lc->cam;
    for (uint32_t r : l.reserved)
        if (r != 0u) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "lens.reserved must be 0");
    if (cam.projection_type > 1u) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "camera.projection_type must be 0 (perspective) or 1 (orthographic)");
    if (!(l.aperture_radius >= 0.0f) || !std::isfinite(l.aperture_radius))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "lens.aperture_radius must be finite and >= 0");
    if (cam.projection_type == 1u) {
        if (l.aperture_radius > 0.0f) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "lens.aperture_radius must be 0 for an orthographic camera");
        if (!(l.ortho_height > 0.0f) || !std::isfinite(l.ortho_height))
            return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "lens.ortho_height must be finite and > 0 for an orthographic camera");
        if (lc->win.height == 0u) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "window.height must be > 0 for an orthographic camera");
    } else if (l.aperture_radius > 0.0f && (!(l.focus_distance > 0.0f) || !std::isfinite(l.focus_distance))) {
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "lens.focus_distance must be finite and > 0 when aperture_radius > 0");
    }
    lc->lc = lens_cam_of(cam.position, cam.direction, cam.up, cam.aspect, tan_half_fov(cam.fov), lc->win.height);
    lc->lv = lens_view_of(cam.direction, cam.projection_type, l.aperture_radius, l.focus_distance, l.ortho_height);
    lc->bound = lens_bound_of(lc->lc, lc->lv);
    return BRT_OK;
}

// what every render entry point checks before it touches the device
int32_t lens_call_check(brt_ctx* ctx, const void* camera80, const void* window16, const void* lens, uint32_t width, uint32_t height,
                        uint32_t flags, uint32_t allowed, LensCall* lc) {
    int32_t rc = lens_check(ctx, camera80, window16, lens, lc);
    if (rc == BRT_OK) rc = size_check(ctx, width, height);
    if (rc != BRT_OK) return rc;
    if (flags & (BRT_FLAG_DENOISE | BRT_FLAG_TEMPORAL | BRT_FLAG_BLEND_POST))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "flags: the post-passes (BRT_FLAG_DENOISE / TEMPORAL / BLEND_POST) assume pinhole rays");
    if (flags & ~allowed)
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "flags: BRT_FLAG_CALLER_STREAM, BRT_FLAG_OUT_* (device frames) and BRT_FLAG_KERNEL_SIMPLE only");
    if (lc->cam.bounce_count >= 0x7fffffffu) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "bounce_count too large");
    if (!ctx->has_scene) return ctx_fail(ctx, BRT_ERR_NO_SCENE, "brt_upload_scene has not succeeded yet");
    if (ctx->policy_flags & kPolicyMask)
        return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, "lens frames implement the default policy only (brt_set_policy)");
    if (!std::isfinite(lc->bound))
        return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, "the lens origins have no finite 1-norm bound (brt_host_lens_origin_bound): no tree can be raised to cover them");
    return BRT_OK;
}

// The tree for the call, then body(): ensure_tree_reach for the camera, and for origins off its position the origin bound
template <class Body>
int32_t with_lens_reach(brt_ctx* ctx, const void* camera80, const LensCall& lc, brt_stats* stats, Body&& body) {
    uint32_t raised = 0u;
    const int32_t rc = with_tree_reach(ctx, camera80, BRT_LEVEL_PURE, stats, [&]() -> int32_t {
        if (lc.lv.mode != LENS_PINHOLE) {
            const int32_t r = ensure_query_reach(ctx, lc.bound, &raised);
            if (r != BRT_OK) return r;
            if (lc.bound > query_bound_of(ctx))
                return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, "the resident tree cannot be raised to cover the lens origins (brt_host_lens_origin_bound)");
        }
        return body();
    });
    if (rc == BRT_OK && stats && raised) stats->tree_rebuilt = 1u;      // (tree_reach is the raised tree's: tree_stats runs behind the body)
    return rc;
}

// A list (pixels null: entry i is pixel i), or a frame, behind its checks: the sparse pixel tracer's call (pixels_call) with the lens
// attached.  out_host: the host form, of host buffers; else `target` of DEVICE buffers on the call's stream.
int32_t lens_call(brt_ctx* ctx, const void* camera80, const void* window16, const LensCall& lc, uint32_t width, uint32_t height,
                  const uint32_t* pixels, uint32_t n_pixels, const PixelsTarget& target, float* out_host, void* hip_stream, uint32_t flags,
                  brt_stats* stats) {
    Camera pinhole = lc.cam;
    pinhole.projection_type = 0u;       // (the frame terms of an orthographic camera are the perspective ones; the rule ignores fov)
    const PixelsCall pc = {&pinhole, window16, width, height, pixels, n_pixels, &lc.lv, flags, target, hip_stream, out_host};
    return pixels_call(ctx, pc, stats, [&](auto&& body) { return with_lens_reach(ctx, camera80, lc, stats, body); });
}

// raytrace.wgsl:95 and :146-147 for pixel (px, py): pixel_begin's expressions (brt_trace.h)
void host_pixel_terms(const Window& win, uint32_t width, uint32_t height, uint32_t px, uint32_t py, uint32_t* seed, float* ndc0x, float* ndc0y) {
    const float uvx = ((float)px + 0.5f) / (float)width;
    const float uvy = ((float)py + 0.5f) / (float)height;
    const float seed_scaled = win.random_seed * 10000.0f;
    const float f = (seed_scaled * (uvx * 402.0f)) * (uvy * 31.5f);
    *seed = !(f > 0.0f) ? 0u : (f >= 4294967296.0f ? 0xffffffffu : (uint32_t)f);
    *ndc0x = uvx * 2.0f - 1.0f;
    *ndc0y = 1.0f - uvy * 2.0f;
}

}  // namespace

extern "C" {

int32_t brt_render_lens_device(brt_ctx* ctx, const void* camera80, const void* window16, const void* lens32, uint32_t width, uint32_t height,
                               void* d_frame, void* hip_stream, uint32_t flags, brt_stats* stats) {
    return ctx_guard(ctx, [&]() -> int32_t {
    LensCall lc{};
    if (!d_frame) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_frame is null");
    if (const int32_t bad = lens_call_check(ctx, camera80, window16, lens32, width, height, flags,
                                            BRT_FLAG_CALLER_STREAM | BRT_FLAG_KERNEL_SIMPLE | BRT_FLAG_OUT_MASK, &lc))
        return bad;
    if (stats) std::memset(stats, 0, sizeof *stats);
    return lens_call(ctx, camera80, window16, lc, width, height, nullptr, width * height, {d_frame, true, flags & BRT_FLAG_OUT_MASK}, nullptr,
                     hip_stream, flags, stats);
    });
}

int32_t brt_render_lens(brt_ctx* ctx, const void* camera80, const void* window16, const void* lens32, uint32_t width, uint32_t height,
                        float* out_rgba32f, uint32_t flags, brt_stats* stats) {
    return ctx_guard(ctx, [&]() -> int32_t {
    LensCall lc{};
    if (!out_rgba32f) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "out_rgba32f is null");
    if (const int32_t bad = lens_call_check(ctx, camera80, window16, lens32, width, height, flags, BRT_FLAG_KERNEL_SIMPLE, &lc)) return bad;
    if (stats) std::memset(stats, 0, sizeof *stats);
    return lens_call(ctx, camera80, window16, lc, width, height, nullptr, width * height, {}, out_rgba32f, nullptr, flags, stats);
    });
}

int32_t brt_render_lens_pixels_device(brt_ctx* ctx, const void* camera80, const void* window16, const void* lens32, uint32_t width,
                                      uint32_t height, const uint32_t* d_pixels, uint32_t n_pixels, float* d_out_rgba32f, void* hip_stream,
                                      uint32_t flags, brt_stats* stats) {
    return ctx_guard(ctx, [&]() -> int32_t {
    LensCall lc{};
    if (const int32_t bad = list_check(ctx, d_pixels, n_pixels, d_out_rgba32f)) return bad;
    if (const int32_t bad = lens_call_check(ctx, camera80, window16, lens32, width, height, flags, BRT_FLAG_CALLER_STREAM | BRT_FLAG_KERNEL_SIMPLE, &lc))
        return bad;
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n_pixels == 0u) return BRT_OK;
    return lens_call(ctx, camera80, window16, lc, width, height, d_pixels, n_pixels, {d_out_rgba32f, false, 0u}, nullptr, hip_stream, flags, stats);
    });
}

int32_t brt_render_lens_pixels(brt_ctx* ctx, const void* camera80, const void* window16, const void* lens32, uint32_t width, uint32_t height,
                               const uint32_t* pixels, uint32_t n_pixels, float* out_rgba32f, uint32_t flags, brt_stats* stats) {
    return ctx_guard(ctx, [&]() -> int32_t {
    LensCall lc{};
    if (const int32_t bad = list_check(ctx, pixels, n_pixels, out_rgba32f)) return bad;
    if (const int32_t bad = lens_call_check(ctx, camera80, window16, lens32, width, height, flags, BRT_FLAG_KERNEL_SIMPLE, &lc)) return bad;
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n_pixels == 0u) return BRT_OK;
    return lens_call(ctx, camera80, window16, lc, width, height, pixels, n_pixels, {}, out_rgba32f, nullptr, flags, stats);
    });
}

int32_t brt_host_lens_seed(const void* window16, uint32_t width, uint32_t height, uint32_t px, uint32_t py, uint32_t* out_seed) {
    return guard(nullptr, [&]() -> int32_t {
    if (!window16 || !out_seed) return fail(BRT_ERR_INVALID_ARGUMENT, "null pointer");
    if (const int32_t bad = size_check(nullptr, width, height)) return bad;
    if (px >= width || py >= height) return fail(BRT_ERR_INVALID_ARGUMENT, "pixel outside the frame");
    Window win;
    std::memcpy(&win, window16, sizeof win);
    float nx, ny;
    host_pixel_terms(win, width, height, px, py, out_seed, &nx, &ny);
    return BRT_OK;
    });
}

int32_t brt_host_lens_ray(const void* camera80, const void* window16, const void* lens32, uint32_t width, uint32_t height, uint32_t px,
                          uint32_t py, uint32_t* state_inout, float* o3, float* d3) {
    return guard(nullptr, [&]() -> int32_t {
    if (!state_inout || !o3 || !d3) return fail(BRT_ERR_INVALID_ARGUMENT, "null pointer");
    LensCall lc{};
    if (const int32_t bad = lens_check(nullptr, camera80, window16, lens32, &lc)) return bad;
    if (const int32_t bad = size_check(nullptr, width, height)) return bad;
    if (px >= width || py >= height) return fail(BRT_ERR_INVALID_ARGUMENT, "pixel outside the frame");
    uint32_t seed;
    float ndc0x, ndc0y, w[3];
    host_pixel_terms(lc.win, width, height, px, py, &seed, &ndc0x, &ndc0y);
    if (lens_ray_raw(lc.lc, lc.lv, lc.lv.mode, ndc0x, ndc0y, *state_inout, o3, w)) lens_normalize(w, d3);
    else std::memcpy(d3, w, sizeof w);
    return BRT_OK;
    });
}

int32_t brt_host_lens_origin_bound(const void* camera80, const void* lens32, float* out_bound) {
    return guard(nullptr, [&]() -> int32_t {
    if (!out_bound) return fail(BRT_ERR_INVALID_ARGUMENT, "out_bound is null");
    const Window win = {0.0f, 1u, {0.0f, 0.0f}};      // (the bound holds for every window of at least one row)
    LensCall lc{};
    if (const int32_t bad = lens_check(nullptr, camera80, &win, lens32, &lc)) return bad;
    *out_bound = lc.bound;
    return BRT_OK;
    });
}

}  // extern "C"
