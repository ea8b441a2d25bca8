// brt_api_radiance.cpp -- radiance queries (brt_radiance.hip; DESIGN.md "Radiance queries") on the first device: path-traced colour
// for a list of the caller's rays.  Reach, refusal bound, sphere numbering and launch plan are the ray queries' (brt_api_query.cpp); the
// skeleton of a call and the round trip of the host form's buffers are brt_frame.h's (ray_list_call, host_round_trip).
#include "brt_frame.h"

using namespace brt;

namespace {

// The default rule streams from this many entries on: below one streaming workgroup's lanes a persistent launch has nothing to refill,
// and every workgroup of it pays for staging the scene
constexpr uint32_t kRadianceStreamMin = BRT_BLOCK;

// the control words of the first device (DeviceCtx::d_radctl), for work behind ev_q
int32_t radiance_ctl(brt_ctx* ctx, DeviceCtx& dc) {
    if (dc.d_radctl) return BRT_OK;
    return ensure(ctx, &dc.d_radctl, &dc.radctl_cap, 64u);
}

}  // namespace

// one list on `stream`, behind the previous list or query of the context; counted: the counts are gathered (the caller synchronises and
// reads d_radctl).  Shared with the probe bake (brt_api_probe.cpp).
int32_t brt::radiance_enqueue(brt_ctx* ctx, DeviceCtx& dc, hipStream_t stream, const void* d_rays, uint32_t n_rays, uint32_t samples,
                         uint32_t bounces, void* d_out, bool counted, RadianceLaunch* rl) {
    int32_t rc = radiance_ctl(ctx, dc);
    if (rc != BRT_OK) return rc;
    HIP_TRY(ctx, hipStreamWaitEvent(stream, dc.ev_q, 0));
    // The form: BRT_RADIANCE_FORM 1 / 2 force the plain / the streaming form; else a list of at least kRadianceStreamMin entries streams
    // where the scene or the top of its tree is staged in LDS (no LDS form: 32-bit descriptors, BRT_FORCE_GLOBAL_SCENE).  Waves per SIMD
    // where nothing is staged: 114 VGPRs with the hand-written loop (4), 89 without (5)
    const uint32_t form = ctx->knobs[K_RADIANCE_FORM];
    plan_list(ctx, dc, n_rays, list_streams(form, kRadianceStreamMin, n_rays), 4u, 5u, form != 2u, rl);
    const uint32_t* rmap = nullptr;
    rc = query_rmap(ctx, dc, stream, &rmap);
    if (rc != BRT_OK) return rc;
    RadianceArgs& ra = rl->args;
    ra.rays = static_cast<const float4*>(d_rays);
    ra.out = static_cast<float4*>(d_out);
    ra.n_rays = n_rays;
    ra.samples = samples;
    ra.bounces = bounces;
    ra.bound = query_bound_of(ctx);
    ra.rmap = rmap;
    ra.stat = counted ? reinterpret_cast<unsigned long long*>(dc.d_radctl) : nullptr;
    ra.counter = dc.d_radctl + 8;
    rl->stream = stream;
    if (counted || rl->form == LIST_STREAM) HIP_TRY(ctx, hipMemsetAsync(dc.d_radctl, 0, 64, stream));
    HIP_TRY(ctx, launch_radiance(*rl));
    HIP_TRY(ctx, hipEventRecord(dc.ev_q, stream));
    return BRT_OK;
}

namespace {

int32_t radiance_check(brt_ctx* ctx, const void* rays, uint32_t n_rays, uint32_t samples, uint32_t bounces, float origin_bound,
                       const void* out) {
    if (samples < 1u || samples > 65535u) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "samples must be in [1, 65535]");
    if (bounces > 65535u) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "bounces must be in [0, 65535]");
    if (const int32_t rc = origin_bound_check(ctx, origin_bound)) return rc;
    if (n_rays > 0x7fff0000u) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "n_rays too large");
    if (n_rays != 0u && (!rays || !out)) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "rays / out is null");
    if (n_rays != 0u && overlaps(rays, (size_t)n_rays * 32u, out, (size_t)n_rays * 32u))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "rays and out overlap");
    if (!ctx->has_scene) return ctx_fail(ctx, BRT_ERR_NO_SCENE, "brt_upload_scene has not succeeded yet");
    if (ctx->policy_flags & kPolicyMask)
        return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, "radiance queries implement the default policy only (brt_set_policy)");
    return BRT_OK;
}

}  // namespace

extern "C" {

int32_t brt_radiance_rays_device(brt_ctx* ctx, const void* d_rays, uint32_t n_rays, uint32_t samples, uint32_t bounces, float origin_bound,
                                 void* d_out, void* hip_stream, uint32_t flags, uint64_t* out_stats8) {
    return ctx_guard(ctx, [&]() -> int32_t {
    int32_t rc = caller_stream_flags_check(ctx, flags);
    if (rc == BRT_OK) rc = radiance_check(ctx, d_rays, n_rays, samples, bounces, origin_bound, d_out);
    if (rc != BRT_OK) return rc;
    return ray_list_call<unsigned long long, RadianceLaunch>(ctx, n_rays, origin_bound, hip_stream, flags, &DeviceCtx::d_radctl, out_stats8,
                                                             [&](DeviceCtx& dc, hipStream_t stream, bool counted, RadianceLaunch* rl) {
        return radiance_enqueue(ctx, dc, stream, d_rays, n_rays, samples, bounces, d_out, counted, rl);
    });
    });
}

int32_t brt_radiance_rays(brt_ctx* ctx, const void* rays, uint32_t n_rays, uint32_t samples, uint32_t bounces, float origin_bound, void* out,
                          uint64_t* out_stats8) {
    return ctx_guard(ctx, [&]() -> int32_t {
    const int32_t rc = radiance_check(ctx, rays, n_rays, samples, bounces, origin_bound, out);
    if (rc != BRT_OK) return rc;
    const size_t bytes = (size_t)n_rays * 32u;
    return ray_list_call<unsigned long long, RadianceLaunch>(ctx, n_rays, origin_bound, nullptr, 0u, &DeviceCtx::d_radctl, out_stats8,
                                                             [&](DeviceCtx& dc, hipStream_t stream, bool counted, RadianceLaunch* rl) {
        return host_round_trip(ctx, dc, stream, {{rays, nullptr, bytes}, {nullptr, out, bytes}}, [&](char* const* d) {
            return radiance_enqueue(ctx, dc, stream, d[0], n_rays, samples, bounces, d[1], counted, rl);
        });
    });
    });
}

}  // extern "C"
