// brt_api_pixels.cpp -- the sparse pixel tracer (brt_pixels.hip; DESIGN.md "Refined upsampling") on the first device: a list of pixels
// of a Pure frame, each traced alone to the value the whole frame holds there.  The tree follows the call's camera (with_tree_reach),
// not an origin bound; the launch plan is that of every list kernel (plan_list).  The lens exports (brt_api_lens.cpp) are the same
// calls with a lens attached: the enqueue, the two bodies of a call and its stats are here for both; the host body is the device body's
// enqueue inside the round trip of its buffers (brt_frame.h host_round_trip).  A pass of a progressive frame
// (brt_api_progressive.cpp) is the same enqueue with the progressive terms attached.
#include "brt_frame.h"

using namespace brt;

namespace brt {

// Which form a list takes: BRT_FLAG_KERNEL_SIMPLE or BRT_PIXELS_FORM 1 the plain form (what brt_api_query.cpp hands to k_query_plain
// goes to it here: every representation and tree), else the streaming form (plan_list).
int32_t pixels_enqueue(brt_ctx* ctx, DeviceCtx& dc, const void* camera80, const void* window16, uint32_t width, uint32_t height,
                       const uint32_t* d_pixels, uint32_t n_pixels, const uint32_t* d_count, const PixelsTarget& target, uint32_t* d_ctl,
                       hipStream_t stream, bool force_plain, PixelsLaunch* pl, const LensView* lens, const ProgPass* prog) {
    int32_t rc = make_frame_params(ctx, camera80, window16, BRT_LEVEL_PURE, width, height, 0u, 1u, &pl->frame);
    if (rc != BRT_OK) return rc;
    if (pl->frame.policy_flags != 0u)
        return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, lens ? "lens frames implement the default policy only (brt_set_policy)"
                                                       : "the pixel tracer implements the default policy only (brt_set_policy)");
    const uint32_t form = ctx->knobs[K_PIXELS_FORM];
    // waves per SIMD where nothing is staged (make usage-lens, usage-progressive): 114 VGPRs with the hand-written loop (4), 74-94 without (5)
    plan_list(ctx, dc, n_pixels, !(form == 1u || (force_plain && form != 2u)), 4u, 5u, false, pl);
    PixelsArgs& pa = pl->args;
    pa.pixels = d_pixels;
    pa.n_pixels = n_pixels;
    pa.count = d_count;
    pa.out = target.d_out;
    pa.scatter = target.scatter ? 1u : 0u;
    pa.out_format = target.out_format;
    pa.stat = reinterpret_cast<unsigned long long*>(d_ctl);
    pa.counter = d_ctl + 4;
    pl->stream = stream;
    if (prog && !prog->first) HIP_TRY(ctx, hipMemsetAsync(pa.counter, 0, 4, stream));
    else HIP_TRY(ctx, hipMemsetAsync(d_ctl, 0, 20, stream));
    if (prog && prog->first) HIP_TRY(ctx, hipMemsetAsync(prog->sample.samples, 0, 8, stream));
    HIP_TRY(ctx, prog ? launch_prog_sample(*pl, prog->sample) : lens ? launch_trace_lens(*pl, *lens) : launch_trace_pixels(*pl));
    return BRT_OK;
}

int32_t list_check(brt_ctx* ctx, const void* pixels, uint32_t n_pixels, const void* out) {
    if (n_pixels > 0x7fff0000u) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "n_pixels too large");
    if (n_pixels != 0u && (!pixels || !out)) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "pixels / out is null");
    return BRT_OK;
}

// the control words of the first device (DeviceCtx::d_pxbuf), for work behind ev_q
static int32_t pixels_ctl(brt_ctx* ctx, DeviceCtx& dc) {
    if (dc.d_pxbuf) return BRT_OK;
    return ensure(ctx, &dc.d_pxbuf, &dc.pxbuf_cap, kPxListWord * 4u);
}

static int32_t call_enqueue(brt_ctx* ctx, DeviceCtx& dc, const PixelsCall& pc, const uint32_t* d_pixels, const PixelsTarget& target,
                            hipStream_t stream, PixelsRun* run) {
    return pixels_enqueue(ctx, dc, pc.camera80, pc.window16, pc.width, pc.height, d_pixels, pc.n_pixels, nullptr, target, dc.d_pxbuf, stream,
                          (pc.flags & BRT_FLAG_KERNEL_SIMPLE) != 0u, &run->pl, pc.lens);
}

int32_t pixels_run_device(brt_ctx* ctx, const PixelsCall& pc, PixelsRun* run) {
    DeviceCtx& dc = ctx->devs[0];
    HIP_TRY(ctx, hipSetDevice(dc.device));
    const StreamChoice sc = stream_of(dc, pc.hip_stream, pc.flags);
    run->counted = sc.own;
    int32_t r = pixels_ctl(ctx, dc);
    if (r != BRT_OK) return r;
    HIP_TRY(ctx, hipStreamWaitEvent(sc.stream, dc.ev_q, 0));
    r = call_enqueue(ctx, dc, pc, pc.pixels, pc.target, sc.stream, run);
    if (r != BRT_OK) return r;
    HIP_TRY(ctx, hipEventRecord(dc.ev_q, sc.stream));
    if (!sc.own) return BRT_OK;
    HIP_TRY(ctx, hipMemcpyAsync(run->counts, dc.d_pxbuf, sizeof run->counts, hipMemcpyDeviceToHost, sc.stream));
    HIP_TRY(ctx, hipStreamSynchronize(sc.stream));
    return BRT_OK;
}

int32_t pixels_run_host(brt_ctx* ctx, const PixelsCall& pc, PixelsRun* run) {
    DeviceCtx& dc = ctx->devs[0];
    HIP_TRY(ctx, hipSetDevice(dc.device));
    run->counted = true;
    int32_t r = pixels_ctl(ctx, dc);
    if (r != BRT_OK) return r;
    // (a lens call without a list has no list plane: entry i is pixel i)
    r = host_round_trip(ctx, dc, dc.stream, {{pc.pixels, nullptr, pc.pixels ? (size_t)pc.n_pixels * 4u : 0u},
                                             {nullptr, pc.out_rgba32f, (size_t)pc.n_pixels * 16u}}, [&](char* const* d) {
        return call_enqueue(ctx, dc, pc, reinterpret_cast<const uint32_t*>(d[0]), {d[1], false, 0u}, dc.stream, run);
    });
    if (r != BRT_OK) return r;
    HIP_TRY(ctx, hipMemcpyAsync(run->counts, dc.d_pxbuf, sizeof run->counts, hipMemcpyDeviceToHost, dc.stream));
    HIP_TRY(ctx, hipStreamSynchronize(dc.stream));
    return BRT_OK;
}

void pixels_stats(const PixelsCall& pc, const PixelsRun& run, double total_ms, brt_stats* stats) {
    // (the tree fields are the reach wrapper's)
    const PixelsLaunch& pl = run.pl;
    stats->rays = run.counted ? run.counts[0] : 0u;
    stats->reserved = run.counted ? (uint32_t)std::min<unsigned long long>(run.counts[1], 0xffffffffull) : 0u;      // entries refused
    stats->paths = run.counted ? ((uint64_t)pc.n_pixels - run.counts[1]) * pl.frame.sample_count : 0u;
    list_launch_stats(pl, pc.n_pixels, pc.lens ? 34u : 32u, stats);
    stats->total_ms = total_ms;
}

}  // namespace brt

namespace {

int32_t pixels_check(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height, const void* pixels,
                     uint32_t n_pixels, const void* out, uint32_t flags, uint32_t allowed) {
    if (!camera80 || !window16) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "camera/window is null");
    if (flags & ~allowed) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "flags: BRT_FLAG_CALLER_STREAM (device form) and BRT_FLAG_KERNEL_SIMPLE only");
    int32_t rc = size_check(ctx, width, height);
    if (rc == BRT_OK) rc = list_check(ctx, pixels, n_pixels, out);
    if (rc != BRT_OK) return rc;
    if (!ctx->has_scene) return ctx_fail(ctx, BRT_ERR_NO_SCENE, "brt_upload_scene has not succeeded yet");
    Camera cam;
    std::memcpy(&cam, camera80, sizeof cam);
    if (cam.projection_type != 0) return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, "only perspective projection (0) is supported (extract.rs:148)");
    if (ctx->policy_flags & kPolicyMask)
        return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, "the pixel tracer implements the default policy only (brt_set_policy)");
    return BRT_OK;
}

// brt_render_pixels (host: host buffers) and brt_render_pixels_device behind the null check of the context
int32_t render_pixels(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height, const uint32_t* pixels,
                      uint32_t n_pixels, float* out, bool host, void* hip_stream, uint32_t flags, brt_stats* stats) {
    if (const int32_t bad = pixels_check(ctx, camera80, window16, width, height, pixels, n_pixels, out, flags,
                                         BRT_FLAG_KERNEL_SIMPLE | (host ? 0u : BRT_FLAG_CALLER_STREAM)))
        return bad;
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n_pixels == 0u) return BRT_OK;
    const PixelsCall pc = {camera80, window16, width, height, pixels, n_pixels, nullptr, flags, {out, false, 0u}, hip_stream, host ? out : nullptr};
    return pixels_call(ctx, pc, stats, [&](auto&& body) { return with_tree_reach(ctx, camera80, BRT_LEVEL_PURE, stats, body); });
}

}  // namespace

extern "C" {

int32_t brt_render_pixels_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height,
                                 const uint32_t* d_pixels, uint32_t n_pixels, float* d_out_rgba32f, void* hip_stream, uint32_t flags,
                                 brt_stats* stats) {
    return ctx_guard(ctx, [&]() -> int32_t {
    return render_pixels(ctx, camera80, window16, width, height, d_pixels, n_pixels, d_out_rgba32f, false, hip_stream, flags, stats);
    });
}

int32_t brt_render_pixels(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height, const uint32_t* pixels,
                          uint32_t n_pixels, float* out_rgba32f, uint32_t flags, brt_stats* stats) {
    return ctx_guard(ctx, [&]() -> int32_t {
    return render_pixels(ctx, camera80, window16, width, height, pixels, n_pixels, out_rgba32f, true, nullptr, flags, stats);
    });
}

}  // extern "C"
