// brt_api_progressive.cpp -- progressive frames on the first device (brt_progressive.hip; DESIGN.md "Progressive frames"): a plane of
// 32-byte pixel records the caller holds, pixels of it continued to a target sample count by the sparse pixel tracer under the
// progressive rule, and the pixels worth a higher target selected from the records' own moments (brt_progressive.h).  The skeleton of an
// export is frame_call's (brt_frame.h); every call runs behind the context's other list work (ev_q) and records it; a pass is enqueued
// by pixels_enqueue (brt_api_pixels.cpp); a host form is its device form's enqueue inside the round trip of the caller's planes
// (host_round_trip).  No call here goes through render_frame_device: the dispatch-order and lean history of plain frames,
// and the base-frame slot of adaptive frames, are never looked at.  Here: the checks of each export in their order, the settings, the
// enqueue of a pass, the passes of the one-call form, and the host twins of the record and the rule.
#include "brt_frame.h"

using namespace brt;

namespace {

constexpr uint32_t kProgFlags = kOutFlags | BRT_FLAG_KERNEL_SIMPLE;
constexpr uint32_t kPxSamplesWord = 6u;      // of DeviceCtx::d_pxbuf's control words: u64 samples run (words 6, 7)

int32_t prog_size_check(brt_ctx* ctx, uint32_t width, uint32_t height, uint32_t target) {
    if (const int32_t bad = size_check(ctx, width, height)) return bad;
    if (target < 1u || target > kProgMaxSamples) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "target must be in [1, 65535]");
    return BRT_OK;
}

int32_t prog_check(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height, uint32_t target, uint32_t flags,
                   uint32_t allowed) {
    if (!camera80 || !window16) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "camera/window is null");
    if (const int32_t bad = flags_check(ctx, flags, allowed,
                                        "flags: BRT_FLAG_CALLER_STREAM (device form), BRT_FLAG_KERNEL_SIMPLE and BRT_FLAG_OUT_* only (pixels of "
                                        "several sample counts: no post-pass)"))
        return bad;
    if (const int32_t bad = prog_size_check(ctx, width, height, target)) return bad;
    if (!ctx->has_scene) return ctx_fail(ctx, BRT_ERR_NO_SCENE, "brt_upload_scene has not succeeded yet");
    Camera cam;
    std::memcpy(&cam, camera80, sizeof cam);
    if (cam.projection_type != 0) return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, "only perspective projection (0) is supported (extract.rs:148)");
    if (ctx->policy_flags & kPolicyMask)
        return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, "the pixel tracer implements the default policy only (brt_set_policy)");
    return BRT_OK;
}

int32_t plane_check(brt_ctx* ctx, uint32_t width, uint32_t height, const void* state, const void* frame, uint32_t fmt) {
    if (!state) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "state is null");
    if (overlaps(state, (size_t)width * height * sizeof(ProgPixel), frame, out_bytes(width, height, fmt)))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "the state plane overlaps the frame");
    return BRT_OK;
}

// the targets of the one-call form: first_spp, then doubling, the last one max_spp
std::vector<uint32_t> prog_targets(uint32_t first_spp, uint32_t max_spp) {
    std::vector<uint32_t> t{first_spp};
    while (t.back() < max_spp) t.push_back(t.back() > max_spp / 2u ? max_spp : t.back() * 2u);
    return t;
}

// What the passes of a call leave for its stats: the launch of the last pass, and the control words (counted runs)
struct ProgRun {
    PixelsLaunch pl{};
    uint32_t entries = 0u;       // of the last launch
    bool counted = false;
};

// One pass on `stream`: the entries of d_pixels (null: every pixel, in the order of BRT_PROGRESSIVE_ORDER, the tile order padded to whole
// 8x8 tiles) continued to `target` -- pixels_enqueue under the progressive rule, on DeviceCtx::d_pxbuf's control words.
int32_t prog_enqueue(brt_ctx* ctx, DeviceCtx& dc, const void* camera80, const void* window16, uint32_t width, uint32_t height, void* d_state,
                     const uint32_t* d_pixels, uint32_t n_pixels, const uint32_t* d_count, uint32_t target, void* d_frame, uint32_t fmt,
                     bool first, hipStream_t stream, uint32_t flags, ProgRun* run) {
    ProgPass pp{};
    pp.first = first;
    pp.sample.state = static_cast<ProgPixel*>(d_state);
    pp.sample.target = target;
    pp.sample.order = (!d_pixels && ctx->knobs[K_PROGRESSIVE_ORDER] != 0u) ? 1u : 0u;
    if (pp.sample.order) n_pixels = ((width + 7u) / 8u) * ((height + 7u) / 8u) * 64u;
    pp.sample.samples = reinterpret_cast<unsigned long long*>(dc.d_pxbuf + kPxSamplesWord);
    run->entries = n_pixels;
    return pixels_enqueue(ctx, dc, camera80, window16, width, height, d_pixels, n_pixels, d_count, {d_frame, true, fmt}, dc.d_pxbuf, stream,
                          (flags & BRT_FLAG_KERNEL_SIMPLE) != 0u, &run->pl, nullptr, &pp);
}

// the one pass of brt_progressive_sample* on DEVICE planes: behind ev_q on the control words (list_buffer), and recorded in it
int32_t sample_enqueue(brt_ctx* ctx, DeviceCtx& dc, const void* camera80, const void* window16, uint32_t width, uint32_t height, void* d_state,
                       const uint32_t* d_pixels, uint32_t n_pixels, const uint32_t* d_count, uint32_t target, void* d_frame, uint32_t fmt,
                       hipStream_t stream, uint32_t flags, ProgRun* run) {
    int32_t r = list_buffer(ctx, dc, 0u, stream);
    if (r == BRT_OK)
        r = prog_enqueue(ctx, dc, camera80, window16, width, height, d_state, d_pixels, n_pixels, d_count, target, d_frame, fmt, true, stream, flags, run);
    if (r != BRT_OK) return r;
    HIP_TRY(ctx, hipEventRecord(dc.ev_q, stream));
    return BRT_OK;
}

int32_t select_enqueue(brt_ctx* ctx, uint32_t width, uint32_t height, const void* d_state, uint32_t target, float threshold, uint32_t radius,
                       uint32_t* d_list, uint32_t* d_count, void* d_mask, hipStream_t stream) {
    ProgSelect ps{};
    ps.width = width;
    ps.height = height;
    ps.state = static_cast<const ProgPixel*>(d_state);
    ps.target = target;
    ps.threshold = threshold;
    ps.radius = radius;
    ps.count = d_count;
    ps.list = d_list;
    ps.mask = static_cast<uint8_t*>(d_mask);
    HIP_TRY(ctx, launch_prog_select(ps, stream));
    return BRT_OK;
}

// the passes of the one-call form on DEVICE planes
int32_t passes_enqueue(brt_ctx* ctx, DeviceCtx& dc, const void* camera80, const void* window16, uint32_t width, uint32_t height, void* d_state,
                       void* d_frame, uint32_t fmt, hipStream_t stream, uint32_t flags, ProgRun* run) {
    const uint32_t px = width * height;
    int32_t r = list_buffer(ctx, dc, px, stream);
    if (r != BRT_OK) return r;
    uint32_t* count = dc.d_pxbuf + kPxCountWord;
    uint32_t* list = dc.d_pxbuf + kPxListWord;
    bool first = true;
    for (const uint32_t target : prog_targets(ctx->progressive.first_spp, ctx->progressive.max_spp)) {
        if (first) {
            r = prog_enqueue(ctx, dc, camera80, window16, width, height, d_state, nullptr, px, nullptr, target, d_frame, fmt, true, stream, flags, run);
        } else {
            HIP_TRY(ctx, hipMemsetAsync(count, 0, 4, stream));
            r = select_enqueue(ctx, width, height, d_state, target, ctx->progressive.threshold, ctx->progressive.radius, list, count, nullptr, stream);
            if (r == BRT_OK)
                r = prog_enqueue(ctx, dc, camera80, window16, width, height, d_state, list, px, count, target, d_frame, fmt, false, stream, flags, run);
        }
        if (r != BRT_OK) return r;
        first = false;
    }
    HIP_TRY(ctx, hipEventRecord(dc.ev_q, stream));
    return BRT_OK;
}

// a call behind its checks: frame_call (rays on the context's own stream), then the launch fields and the other counts
template <class Body>
int32_t prog_call(brt_ctx* ctx, const void* camera80, void* hip_stream, uint32_t flags, brt_stats* stats, ProgRun* run, Body&& body) {
    const int32_t rc = frame_call(ctx, camera80, hip_stream, flags & BRT_FLAG_CALLER_STREAM, stats, FRAME_STATS_CLEAR | FRAME_STATS_ADD_RETRACE,
                                  [&](DeviceCtx& dc, const StreamChoice& sc) -> int32_t {
        run->counted = sc.own;
        return body(dc, sc);
    });
    if (rc != BRT_OK || !stats) return rc;
    if (run->counted) {      // (the own stream has been synchronised, and nothing of this context has run since)
        uint32_t ctl[kPxListWord];
        HIP_TRY(ctx, hipMemcpy(ctl, ctx->devs[0].d_pxbuf, sizeof ctl, hipMemcpyDeviceToHost));
        unsigned long long refused, samples;
        std::memcpy(&refused, ctl + 2, 8);
        std::memcpy(&samples, ctl + kPxSamplesWord, 8);
        stats->reserved = (uint32_t)std::min<unsigned long long>(refused, 0xffffffffull);      // entries refused
        stats->paths = samples;
    }
    list_launch_stats(run->pl, run->entries, 36u, stats);      // (the pixel lists' variants are 32 .. 35)
    return rc;
}

}  // namespace

extern "C" {

int32_t brt_set_progressive(brt_ctx* ctx, uint32_t first_spp, uint32_t max_spp, float threshold, uint32_t radius) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (first_spp < 2u || first_spp > max_spp || max_spp > kProgMaxSamples)
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "2 <= first_spp <= max_spp <= 65535 must hold");
    if (!adapt_finite(threshold) || !(threshold > 0.0f)) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "threshold must be finite and > 0");
    if (radius > 1u) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "radius must be 0 or 1");
    ctx->progressive.first_spp = first_spp;
    ctx->progressive.max_spp = max_spp;
    ctx->progressive.threshold = threshold;
    ctx->progressive.radius = radius;
    return BRT_OK;
    });
}

int32_t brt_progressive_sample_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height, void* d_state,
                                      const uint32_t* d_pixels_or_null, uint32_t n_pixels, const uint32_t* d_count_or_null, uint32_t target,
                                      void* d_frame_or_null, void* hip_stream, uint32_t flags, brt_stats* stats) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (const int32_t bad = prog_check(ctx, camera80, window16, width, height, target, flags, kProgFlags)) return bad;
    const uint32_t fmt = flags & BRT_FLAG_OUT_MASK;
    if (const int32_t bad = plane_check(ctx, width, height, d_state, d_frame_or_null, fmt)) return bad;
    if (n_pixels > 0x7fff0000u) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "n_pixels too large");
    if (!d_pixels_or_null && (n_pixels != width * height || d_count_or_null))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "a null list is every pixel: n_pixels must be width * height and d_count null");
    if (const int32_t bad = device_aligned(ctx, {d_state, d_frame_or_null})) return bad;
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n_pixels == 0u) return BRT_OK;
    ProgRun run;
    return prog_call(ctx, camera80, hip_stream, flags, stats, &run, [&](DeviceCtx& dc, const StreamChoice& sc) {
        return sample_enqueue(ctx, dc, camera80, window16, width, height, d_state, d_pixels_or_null, n_pixels, d_count_or_null, target,
                              d_frame_or_null, fmt, sc.stream, flags, &run);
    });
    });
}

int32_t brt_progressive_sample(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height, void* state,
                               const uint32_t* pixels_or_null, uint32_t n_pixels, uint32_t target, void* frame_or_null, uint32_t flags,
                               brt_stats* stats) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (const int32_t bad = prog_check(ctx, camera80, window16, width, height, target, flags, kProgFlags & ~BRT_FLAG_CALLER_STREAM)) return bad;
    const uint32_t fmt = flags & BRT_FLAG_OUT_MASK;
    if (const int32_t bad = plane_check(ctx, width, height, state, frame_or_null, fmt)) return bad;
    if (n_pixels > 0x7fff0000u) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "n_pixels too large");
    if (!pixels_or_null && n_pixels != width * height)
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "a null list is every pixel: n_pixels must be width * height");
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n_pixels == 0u) return BRT_OK;
    ProgRun run;
    return prog_call(ctx, camera80, nullptr, flags, stats, &run, [&](DeviceCtx& dc, const StreamChoice& sc) -> int32_t {
        // (a frame holds the listed pixels' values and, elsewhere, what the caller's frame held: it goes in as well as out)
        return host_round_trip(ctx, dc, sc.stream, {{state, state, (size_t)width * height * sizeof(ProgPixel)},
                                                    {pixels_or_null, nullptr, pixels_or_null ? (size_t)n_pixels * 4u : 0u},
                                                    {frame_or_null, frame_or_null, frame_or_null ? out_bytes(width, height, fmt) : 0u}},
                               [&](char* const* d) {
            return sample_enqueue(ctx, dc, camera80, window16, width, height, d[0], reinterpret_cast<const uint32_t*>(d[1]), n_pixels, nullptr,
                                  target, d[2], fmt, sc.stream, flags, &run);
        });
    });
    });
}

int32_t brt_progressive_select_device(brt_ctx* ctx, uint32_t width, uint32_t height, const void* d_state, uint32_t target, uint32_t* d_list,
                                      uint32_t* d_count, void* d_mask_u8_or_null, void* hip_stream, uint32_t flags) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (const int32_t bad = caller_stream_flags_check(ctx, flags)) return bad;
    if (const int32_t bad = prog_size_check(ctx, width, height, target)) return bad;
    if (!d_state) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_state is null");
    if ((d_list == nullptr) != (d_count == nullptr)) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_list and d_count go together");
    if (!d_list && !d_mask_u8_or_null) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_list / d_count and d_mask_u8 are all null");
    if (const int32_t bad = device_aligned(ctx, {d_state})) return bad;
    const size_t px = (size_t)width * height;
    if (overlaps(d_state, px * sizeof(ProgPixel), d_list, px * 4u) || overlaps(d_state, px * sizeof(ProgPixel), d_count, 4u) ||
        overlaps(d_state, px * sizeof(ProgPixel), d_mask_u8_or_null, px))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "the state plane overlaps an output");
    return list_step_run(ctx, hip_stream, flags, [&](DeviceCtx&, hipStream_t stream) -> int32_t {
        if (d_count) HIP_TRY(ctx, hipMemsetAsync(d_count, 0, 4, stream));
        return select_enqueue(ctx, width, height, d_state, target, ctx->progressive.threshold, ctx->progressive.radius, d_list, d_count,
                              d_mask_u8_or_null, stream);
    });
    });
}

int32_t brt_render_progressive_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height, void* d_state,
                                      void* d_frame, void* hip_stream, uint32_t flags, brt_stats* stats) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (!d_frame) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_frame is null");
    if (const int32_t bad = prog_check(ctx, camera80, window16, width, height, ctx->progressive.max_spp, flags, kProgFlags)) return bad;
    const uint32_t fmt = flags & BRT_FLAG_OUT_MASK;
    if (const int32_t bad = plane_check(ctx, width, height, d_state, d_frame, fmt)) return bad;
    if (const int32_t bad = device_aligned(ctx, {d_state, d_frame})) return bad;
    if (stats) std::memset(stats, 0, sizeof *stats);
    ProgRun run;
    return prog_call(ctx, camera80, hip_stream, flags, stats, &run, [&](DeviceCtx& dc, const StreamChoice& sc) -> int32_t {
        return passes_enqueue(ctx, dc, camera80, window16, width, height, d_state, d_frame, fmt, sc.stream, flags, &run);
    });
    });
}

int32_t brt_render_progressive(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height, void* state,
                               void* frame, uint32_t flags, brt_stats* stats) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (!frame) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "frame is null");
    if (const int32_t bad = prog_check(ctx, camera80, window16, width, height, ctx->progressive.max_spp, flags, kProgFlags & ~BRT_FLAG_CALLER_STREAM))
        return bad;
    const uint32_t fmt = flags & BRT_FLAG_OUT_MASK;
    if (const int32_t bad = plane_check(ctx, width, height, state, frame, fmt)) return bad;
    if (stats) std::memset(stats, 0, sizeof *stats);
    ProgRun run;
    return prog_call(ctx, camera80, nullptr, flags, stats, &run, [&](DeviceCtx& dc, const StreamChoice& sc) -> int32_t {
        // (the first pass writes every pixel of the frame: it goes out only)
        return host_round_trip(ctx, dc, sc.stream, {{state, state, (size_t)width * height * sizeof(ProgPixel)},
                                                    {nullptr, frame, out_bytes(width, height, fmt)}}, [&](char* const* d) {
            return passes_enqueue(ctx, dc, camera80, window16, width, height, d[0], d[1], fmt, sc.stream, flags, &run);
        });
    });
    });
}

// one sample of colour rgb added to the record: the code the kernels compile
int32_t brt_host_progressive_accumulate(void* record32, const float* rgb) {
    return guard(nullptr, [&]() -> int32_t {
    if (!record32 || !rgb) return fail(BRT_ERR_INVALID_ARGUMENT, "null pointer");
    ProgPixel rec;
    std::memcpy(&rec, record32, sizeof rec);
    prog_accumulate(rec, rgb[0], rgb[1], rgb[2]);
    std::memcpy(record32, &rec, sizeof rec);
    return BRT_OK;
    });
}

// the class of ONE pixel from the records of its 3x3 window (dy outer, dx inner, both -1 .. 1: the pixel is records9[4])
int32_t brt_host_progressive_class(const void* records9, const uint32_t* inside9, uint32_t target, float threshold, uint32_t radius,
                                   uint32_t* out_class) {
    return guard(nullptr, [&]() -> int32_t {
    if (!records9 || !inside9 || !out_class) return fail(BRT_ERR_INVALID_ARGUMENT, "null pointer");
    if (radius > 1u) return fail(BRT_ERR_INVALID_ARGUMENT, "radius must be 0 or 1");
    ProgPixel rec[9];
    std::memcpy(rec, records9, sizeof rec);
    *out_class = prog_classify(rec[4].n, target, (int)radius, [&](int dx, int dy) {
        const int k = (dy + 1) * 3 + dx + 1;
        return inside9[k] != 0u && prog_noisy(rec[k].m1, rec[k].m2, rec[k].n, threshold);
    });
    return BRT_OK;
    });
}

}  // extern "C"
