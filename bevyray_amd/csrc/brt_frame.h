// brt_frame.h -- what the host units of the C ABI (brt_api*.cpp) share beyond the context of brt_ctx.h.  Internal and host only:
// no .hip, and no header a .hip includes, may include it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <string>
#include <vector>

#include "brt_ctx.h"

namespace brt {

constexpr uint32_t kPolicyMask = BRT_POLICY_OR_SHORT_CIRCUIT | BRT_POLICY_MINMAX_SELECT | BRT_POLICY_POW_EXP2_LOG2;
constexpr double kTwoPi = 6.283185307179586;   // of the host-computed tables (probe directions, envmap taps)
constexpr uint32_t kLptAfterUpload = 4;     // frames after a scene upload within which the tile costs are measured again (brt_api_order.cpp)

inline double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The stream of an asynchronous entry point: the context's own (the call then synchronises, measures and reads the counters) unless the
// caller passes one or sets BRT_FLAG_CALLER_STREAM (a null stream is then the caller's null stream).
struct StreamChoice { bool own; hipStream_t stream; };
inline StreamChoice stream_of(const DeviceCtx& dc, void* hip_stream, uint32_t flags) {
    const bool own = (hip_stream == nullptr) && !(flags & BRT_FLAG_CALLER_STREAM);
    return {own, own ? dc.stream : static_cast<hipStream_t>(hip_stream)};
}

// The strips of part `part` when the strips of a frame go to n_parts parts in turn: its k-th strip is frame strip part + k * n_parts
// and lies at row k * BRT_STRIP_ROWS of its tile.  All of them are whole but the frame's last one, if that is partial and this part's.
struct PartStrips {
    uint32_t part, n_parts;
    uint32_t n_full;         // whole strips: k = 0 .. n_full - 1
    uint32_t tail_rows;      // rows of the partial strip k = n_full (0: none)
    PartStrips(uint32_t height, uint32_t part_, uint32_t n_parts_) : part(part_), n_parts(n_parts_) {
        const uint32_t full = height / BRT_STRIP_ROWS;
        n_full = full > part ? (full - part + n_parts - 1u) / n_parts : 0u;
        tail_rows = full % n_parts == part ? height - full * BRT_STRIP_ROWS : 0u;
    }
    uint32_t count() const { return n_full + (tail_rows ? 1u : 0u); }
    uint32_t frame_row(uint32_t k) const { return (part + k * n_parts) * BRT_STRIP_ROWS; }
    uint32_t rows(uint32_t k) const { return k < n_full ? BRT_STRIP_ROWS : tail_rows; }
    uint64_t total_rows() const { return (uint64_t)n_full * BRT_STRIP_ROWS + tail_rows; }
};

// ---- argument checks and sizes that more than one family states (the list calls; post, upscale, adaptive, G-buffer, lightmap) ----
// `text` names what the export allows, in its own words
inline int32_t flags_check(brt_ctx* ctx, uint32_t flags, uint32_t allowed, const char* text) {
    if (flags & ~allowed) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, text);
    return BRT_OK;
}
// what a call that writes a frame in a BRT_FLAG_OUT_* format allows, and with the post-passes of a frame it traces itself
constexpr uint32_t kOutFlags = BRT_FLAG_CALLER_STREAM | BRT_FLAG_OUT_MASK;
constexpr uint32_t kOutPostFlags = kOutFlags | BRT_FLAG_DENOISE | BRT_FLAG_TEMPORAL;
inline int32_t caller_stream_flags_check(brt_ctx* ctx, uint32_t flags) {
    return flags_check(ctx, flags, BRT_FLAG_CALLER_STREAM, "flags: BRT_FLAG_CALLER_STREAM only");
}
// the size of a frame (a host twin without a context passes nullptr, as to every check here)
inline int32_t size_check(brt_ctx* ctx, uint32_t width, uint32_t height) {
    if (width == 0 || height == 0 || width > 32768u || height > 32768u)
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "width/height must be in [1, 32768]");
    return BRT_OK;
}
// the level of a frame that is presented: 0 traces nothing (`nothing`: the call's words for it), else 1, 2 or 3
inline int32_t frame_level_check(brt_ctx* ctx, uint32_t level, const char* nothing) {
    if (level == BRT_LEVEL_SKIP) return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, nothing);
    if (level != BRT_LEVEL_FALLBACK_RASTER && level != BRT_LEVEL_FALLBACK_RAYTRACED && level != BRT_LEVEL_PURE)
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "level must be 1, 2 or 3");
    return BRT_OK;
}
inline bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const char* pa = static_cast<const char*>(a);
    const char* pb = static_cast<const char*>(b);
    return a && b && pa < pb + b_bytes && pb < pa + a_bytes;
}
// of a width x height frame in the BRT_FLAG_OUT_* format fmt
inline size_t out_bytes(uint32_t width, uint32_t height, uint32_t fmt) {
    return (size_t)width * height * (fmt == BRT_FLAG_OUT_RGBA32F ? 16u : fmt == BRT_FLAG_OUT_RGBA16F ? 8u : 4u);
}

// ---- brt_api.cpp ----
// brt_upload_scene; with `rebuild`, the resident scene's bytes again in a callee-built SAH tree of reach level `level`
int32_t upload_scene(brt_ctx* ctx, const void* models, uint32_t n_models, const void* materials, uint32_t n_materials,
                     const void* bvh_nodes, uint32_t n_nodes, uint32_t level, bool rebuild);
int32_t ensure_tree_reach(brt_ctx* ctx, const void* camera80, uint32_t* rebuilt);
void tree_stats(const brt_ctx* ctx, uint32_t rebuilt, brt_stats* stats);

// ---- brt_api_launch.cpp ----
struct LaunchPlan {
    int scene_mode;              // SceneMode (brt_layout.h)
    uint32_t lds_pairs;          // SCENE_LDS_TOP: pair records staged in LDS
    uint32_t block, grid, wg_per_cu;
    uint32_t pool_cap;           // records of the drain pool per workgroup (0: none)
    uint32_t rows;               // 1: with the scratch of the row-mode walk (SCENE_LDS)
    size_t lds_bytes;
    uint32_t variant;            // brt_stats::kernel_variant of the launch
    uint32_t measured;           // the launch measured the tile costs
};
int32_t make_frame_params(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t level, uint32_t width,
                          uint32_t height, uint32_t part, uint32_t n_parts, FrameParams* out);
LaunchPlan plan_launch(const Knobs& kn, const DeviceCtx& dc, const FrameParams& fp);
int32_t launch_part(brt_ctx* ctx, DeviceCtx& dc, const FrameParams& fp, const float* d_raster_rgba,
                    const float* d_raster_depth, float* d_out_tile, hipStream_t stream, uint32_t flags, bool timed,
                    LaunchPlan* plan_out);
uint64_t part_pixels(const FrameParams& fp);
// the launch fields of brt_stats: the plan of the (last) launch, and the hot records of dc
void launch_stats(const brt_ctx* ctx, const DeviceCtx& dc, const LaunchPlan& lp, brt_stats* stats);
// behind the frame of fp enqueued on dc's `stream`: the order of the next frames, then -- synchronising -- the counters added to *st and
// the kernel and pre-pass times as running maxima in st->kernel_ms / st->prepass_ms
int32_t collect_part(brt_ctx* ctx, DeviceCtx& dc, const FrameParams& fp, hipStream_t stream, bool prepass_ran, brt_stats* st);

// ---- brt_api_order.cpp ----
void view_key_of(const brt_ctx* ctx, const FrameParams& fp, uint32_t key[8]);
int32_t attach_tile_order(brt_ctx* ctx, DeviceCtx& dc, FrameParams& fp, hipStream_t stream, bool may_measure, uint32_t flags);
int32_t update_tile_order(brt_ctx* ctx, DeviceCtx& dc, const FrameParams& fp, hipStream_t stream);
int32_t prepass_order(brt_ctx* ctx, DeviceCtx& dc, const FrameParams& fp, const float* d_raster_rgba,
                      const float* d_raster_depth, float* d_out_tile, hipStream_t stream, uint32_t flags, bool* ran);
uint64_t tree_shape_hash(const EncodedScene& e);
void permute_scene(const std::vector<float>& pairs, const std::vector<float>& spheres, const std::vector<uint32_t>& sphmat,
                   const std::vector<float>& sphmats, uint32_t root, const std::vector<uint32_t>& rank, const std::vector<uint32_t>& srank,
                   std::vector<float>* out_pairs, std::vector<float>* out_spheres, std::vector<uint32_t>* out_sphmat,
                   std::vector<float>* out_sphmats, uint32_t* out_root);

// ---- brt_api_render.cpp ----
void drain_all_streams(brt_ctx* ctx);
// What the entry points that trace or cast rays share: the resident tree serves this camera (ensure_tree_reach; level 0 traces nothing)
// before `body` runs; a failed call leaves nothing in flight on the context's own streams (a caller's stream is the caller's to drain), a
// successful one reports the tree in its stats.
template <class Body>
int32_t with_tree_reach(brt_ctx* ctx, const void* camera80, uint32_t level, brt_stats* stats, Body&& body) {
    uint32_t rebuilt = 0u;
    int32_t rc = level != 0u ? ensure_tree_reach(ctx, camera80, &rebuilt) : BRT_OK;
    if (rc == BRT_OK) rc = body();
    if (rc != BRT_OK) drain_all_streams(ctx);
    else tree_stats(ctx, rebuilt, stats);
    return rc;
}
// brt_render_device behind its argument checks: the frame of every device of the context, assembled on the first one
int32_t render_frame_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t level, uint32_t width, uint32_t height,
                            const float* d_raster_rgba, const float* d_raster_depth, void* d_frame, void* hip_stream, uint32_t flags,
                            brt_stats* stats);

// ---- brt_api_query.cpp ----
// The launch of a list kernel over n_items (brt_kernels.h StreamLaunch): the plain form, or -- with `streams` -- the streaming form in the
// launch shape of plan_stream: what it stages in LDS, its block and its fixed grid.  waves_by_hand / waves_other: the waves per SIMD the
// kernel's registers admit where nothing is staged -- of the instantiation that holds the hand-written walk loop (16-bit descriptors,
// simple tree) and of the others.  need_lds: where nothing can be staged the list takes the plain form after all.
void plan_list(const brt_ctx* ctx, const DeviceCtx& dc, uint32_t n_items, bool streams, uint32_t waves_by_hand, uint32_t waves_other,
               bool need_lds, StreamLaunch* sl);
// What lists of caller rays share (ray queries, radiance queries): the largest origin 1-norm the resident tree covers (+INF: any; < 0:
// none); origin_bound > 0: a callee-built tree's reach raised, if needed, to what origins of that 1-norm need; the form rule of a list
// of n rays (knob value 1 / 2: plain / streaming, else streaming from stream_min rays on, 0: never); the resident -> caller sphere map
// of the first device for work on `stream` (nullptr: the identity)
float query_bound_of(const brt_ctx* ctx);
int32_t ensure_query_reach(brt_ctx* ctx, float origin_bound, uint32_t* rebuilt);
bool list_streams(uint32_t form, uint32_t stream_min, uint32_t n);
int32_t query_rmap(brt_ctx* ctx, DeviceCtx& dc, hipStream_t stream, const uint32_t** rmap);

// ---- brt_api_radiance.cpp ----
// One radiance list (brt_radiance.h) on `stream` of the first device, behind the previous list or query of the context (ev_q, which it
// records); the form is reported in *rl.  counted: the three counts are gathered in dc.d_radctl.
int32_t radiance_enqueue(brt_ctx* ctx, DeviceCtx& dc, hipStream_t stream, const void* d_rays, uint32_t n_rays, uint32_t samples,
                         uint32_t bounces, void* d_out, bool counted, RadianceLaunch* rl);

// ---- brt_api_probe.cpp ----
// What the bakes of light probes share with the bake of an irradiance volume (brt_api_volume.cpp).  bake_check: the arguments of a bake
// (with n_probes = 0 the two pointers are not looked at).  bake_enqueue: the bake of DEVICE buffers on `stream`, in chunks of whole
// probes (bake_chunks), all behind ev_q, which the last step records.  bake_stats: the out_stats8 of every bake (bake_call).
struct BakeRun {
    RadianceLaunch rl{};
    uint32_t chunks = 0u;
    std::vector<unsigned long long> counts;      // 3 per chunk (counted runs)
};
int32_t bake_check(brt_ctx* ctx, const void* probes, uint32_t n_probes, uint32_t n_dirs, uint32_t bounces, uint32_t basis,
                   float origin_bound, const void* out);
int32_t bake_enqueue(brt_ctx* ctx, DeviceCtx& dc, hipStream_t stream, const void* d_probes, uint32_t n_probes, uint32_t n_dirs,
                     uint32_t bounces, uint32_t basis, void* d_out, bool counted, BakeRun* run);
void bake_stats(const brt_ctx* ctx, const BakeRun& run, uint32_t rebuilt, uint64_t* out8);

// ---- brt_api_pixels.cpp ----
// What a list of pixels is traced into (brt_pixels.h PixelsArgs): packed RGBA32F, or scattered into a frame in a BRT_FLAG_OUT_* format
struct PixelsTarget {
    void* d_out;
    bool scatter;
    uint32_t out_format;
};
// Behind whatever wrote the list on `stream`: the list traced as pixels of the width x height Pure frame of camera80 / window16 on the
// first device.  d_count: a device word holding the number of entries (nullptr: n_pixels, which is else the list's capacity).  ctl: 8
// words of the caller's {u64 rays, u64 refused, u32 batch counter, ...}, zeroed here.  Refuses a non-default policy.  lens: the list
// under the lens rule (brt_lens.hip), where a null d_pixels means that entry i is pixel i; camera80 is then the pinhole camera of the
// frame terms.  prog: the list under the progressive rule (brt_progressive.hip), a pass of a call (brt_api_progressive.cpp): the first
// pass zeroes the samples word as well, a later one the batch counter alone, so that the counts of a call's passes add up.
struct ProgPass {
    ProgSample sample;
    bool first;
};
int32_t pixels_enqueue(brt_ctx* ctx, DeviceCtx& dc, const void* camera80, const void* window16, uint32_t width, uint32_t height,
                       const uint32_t* d_pixels, uint32_t n_pixels, const uint32_t* d_count, const PixelsTarget& target, uint32_t* d_ctl,
                       hipStream_t stream, bool force_plain, PixelsLaunch* pl, const LensView* lens = nullptr, const ProgPass* prog = nullptr);
// What brt_render_pixels* and brt_render_lens* (brt_api_lens.cpp) share.  The check of a list with its output; a call behind its checks,
// of n_pixels > 0 entries; its two bodies, which run once the tree is settled; and the launch fields of its stats (counts2 null: not
// counted; kernel_variant 32 / 33, under a lens 34 / 35).
int32_t list_check(brt_ctx* ctx, const void* pixels, uint32_t n_pixels, const void* out);
struct PixelsCall {
    const void *camera80, *window16;     // as pixels_enqueue takes them
    uint32_t width, height;
    const uint32_t* pixels;              // the device form's DEVICE list, the host form's host list
    uint32_t n_pixels;
    const LensView* lens;
    uint32_t flags;
    PixelsTarget target;                 // the device form's
    void* hip_stream;
    float* out_rgba32f;                  // the host form's (null: the device form)
};
struct PixelsRun {
    PixelsLaunch pl{};
    unsigned long long counts[2] = {0u, 0u};
    bool counted = false;
};
int32_t pixels_run_device(brt_ctx* ctx, const PixelsCall& pc, PixelsRun* run);      // DEVICE buffers on the call's stream
int32_t pixels_run_host(brt_ctx* ctx, const PixelsCall& pc, PixelsRun* run);        // host buffers, synchronous on the context's own stream
void pixels_stats(const PixelsCall& pc, const PixelsRun& run, double total_ms, brt_stats* stats);
// reach(body): the tree for the call, then body() -- with_tree_reach, or brt_api_lens.cpp's with_lens_reach
template <class Reach>
int32_t pixels_call(brt_ctx* ctx, const PixelsCall& pc, brt_stats* stats, Reach&& reach) {
    const auto t0 = std::chrono::steady_clock::now();
    PixelsRun run;
    const int32_t rc = reach([&]() -> int32_t { return pc.out_rgba32f ? pixels_run_host(ctx, pc, &run) : pixels_run_device(ctx, pc, &run); });
    if (rc == BRT_OK && stats) pixels_stats(pc, run, ms_since(t0), stats);
    return rc;
}

// ---- brt_api_post.cpp ----
// the guides' frame parameters (one part, level 3) and the denoiser's scratch of a width x height frame for work on `stream`
int32_t denoise_begin(brt_ctx* ctx, DeviceCtx& dc, const void* camera80, const void* window16, uint32_t width, uint32_t height,
                      hipStream_t stream, FrameParams* fp, DenoiseScratch* ds);
int32_t run_denoise(brt_ctx* ctx, DeviceCtx& dc, const FrameParams& fp, const DenoiseScratch& ds, const float* d_in, void* d_out,
                    uint32_t out_format, hipStream_t stream, uint32_t flags, const BlendPost& bp);
bool blend_post_on(uint32_t level, uint32_t flags);
int32_t post_flags_check(brt_ctx* ctx, uint32_t level, uint32_t flags);

// ---- what the calls on a whole frame behind the tracer share (brt_api_post.cpp, brt_api_upscale.cpp, brt_api_adaptive.cpp) ----
// What a successful call leaves in its brt_stats besides total_ms and the tree: what render_frame_device filled in, or nothing; and on the
// context's own stream the rays of the re-trace (trace_selected) added to either.
enum FrameStats : uint32_t { FRAME_STATS_KEEP = 0u, FRAME_STATS_CLEAR = 1u, FRAME_STATS_ADD_RETRACE = 2u };
// A call behind its argument checks: the tree settled for the camera (with_tree_reach: a failed call leaves nothing in flight on the
// context's own streams), then body(dc, sc) on the first device with the call's stream; an own stream is synchronised; the stats rule;
// total_ms.
template <class Body>
int32_t frame_call(brt_ctx* ctx, const void* camera80, void* hip_stream, uint32_t flags, brt_stats* stats, uint32_t stats_rule, Body&& body) {
    const auto t0 = std::chrono::steady_clock::now();
    const int32_t rc = with_tree_reach(ctx, camera80, BRT_LEVEL_PURE, stats, [&]() -> int32_t {     // (the guides walk the tree of the frame)
        DeviceCtx& dc = ctx->devs[0];
        HIP_TRY(ctx, hipSetDevice(dc.device));
        const StreamChoice sc = stream_of(dc, hip_stream, flags);
        const int32_t r = body(dc, sc);
        if (r != BRT_OK) return r;
        unsigned long long rays = 0u;
        if (sc.own) {
            if (stats_rule & FRAME_STATS_ADD_RETRACE) HIP_TRY(ctx, hipMemcpyAsync(&rays, dc.d_pxbuf, sizeof rays, hipMemcpyDeviceToHost, sc.stream));
            HIP_TRY(ctx, hipStreamSynchronize(sc.stream));
        }
        if (stats && (stats_rule & FRAME_STATS_CLEAR)) std::memset(stats, 0, sizeof *stats);
        if (stats) stats->rays += rays;
        return BRT_OK;
    });
    if (rc == BRT_OK && stats) stats->total_ms = ms_since(t0);
    return rc;
}

// The frame the context keeps between two stages of one call (DeviceCtx::d_uplow: the low frame of an upsampling that traces it, the base
// frame of adaptive sampling), of at least `bytes`, for work on `stream`.  Its last reader recorded ev_dn: the frame grows only once
// ev_dn has passed, and the stream waits for ev_dn before the trace writes it.
inline int32_t context_frame(brt_ctx* ctx, DeviceCtx& dc, size_t bytes, hipStream_t stream) {
    if (dc.uplow_cap < bytes) HIP_TRY(ctx, hipEventSynchronize(dc.ev_dn));
    const int32_t rc = ensure(ctx, &dc.d_uplow, &dc.uplow_cap, bytes);
    if (rc != BRT_OK) return rc;
    HIP_TRY(ctx, hipStreamWaitEvent(stream, dc.ev_dn, 0));
    return BRT_OK;
}

// DeviceCtx::d_pxbuf: kPxListWord control words -- the {u64 rays, u64 refused, u32 batch counter} pixels_enqueue zeroes, at kPxCountWord
// the number of selected pixels, two spare -- then the list of a selecting call, one word per pixel of its frame.
constexpr uint32_t kPxCountWord = 5u, kPxListWord = 8u;
struct SelectList { uint32_t *ctl, *count, *list; };
// d_pxbuf with room for a list of list_words entries (0: the control words alone) for work on `stream`, ordered by ev_q: a larger one is
// allocated only once the last user of the old one has ended, and the stream is put behind that user
inline int32_t list_buffer(brt_ctx* ctx, DeviceCtx& dc, size_t list_words, hipStream_t stream) {
    const size_t bytes = (list_words + kPxListWord) * 4u;
    if (dc.pxbuf_cap < bytes) HIP_TRY(ctx, hipEventSynchronize(dc.ev_q));
    const int32_t rc = ensure(ctx, &dc.d_pxbuf, &dc.pxbuf_cap, bytes);
    if (rc != BRT_OK) return rc;
    HIP_TRY(ctx, hipStreamWaitEvent(stream, dc.ev_q, 0));
    return BRT_OK;
}
// The list of a width x height refinement or adaptive frame: list_buffer, and the control words zeroed behind the last user
inline int32_t refine_list(brt_ctx* ctx, DeviceCtx& dc, uint32_t width, uint32_t height, hipStream_t stream, SelectList* sl) {
    const int32_t rc = list_buffer(ctx, dc, (size_t)width * height, stream);
    if (rc != BRT_OK) return rc;
    HIP_TRY(ctx, hipMemsetAsync(dc.d_pxbuf, 0, kPxListWord * 4u, stream));
    *sl = {dc.d_pxbuf, dc.d_pxbuf + kPxCountWord, dc.d_pxbuf + kPxListWord};
    return BRT_OK;
}
// Behind the kernel that selected into sl on `stream`: the selected pixels of the width x height frame traced into d_out, the count copied
// to d_count (or nullptr), and ev_q recorded, which frees the list for the next selecting call
inline int32_t trace_selected(brt_ctx* ctx, DeviceCtx& dc, const void* camera80, const void* window16, uint32_t width, uint32_t height,
                              const SelectList& sl, void* d_out, uint32_t out_format, uint32_t* d_count, hipStream_t stream) {
    PixelsLaunch pl{};
    const int32_t rc = pixels_enqueue(ctx, dc, camera80, window16, width, height, sl.list, width * height, sl.count, {d_out, true, out_format},
                                      sl.ctl, stream, false, &pl);
    if (rc != BRT_OK) return rc;
    if (d_count) HIP_TRY(ctx, hipMemcpyAsync(d_count, sl.count, 4, hipMemcpyDeviceToDevice, stream));
    HIP_TRY(ctx, hipEventRecord(dc.ev_q, stream));
    return BRT_OK;
}

// ---- what the list entry points share (brt_api_query.cpp, brt_api_radiance.cpp, brt_api_probe.cpp, brt_api_volume.cpp,
// brt_api_envmap.cpp, brt_api_lightmap.cpp, brt_api_pixels.cpp, brt_api_progressive.cpp, brt_api_gbuffer.cpp) ----
inline int32_t origin_bound_check(brt_ctx* ctx, float origin_bound) {
    if (!(origin_bound >= 0.0f) || !std::isfinite(origin_bound)) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "origin_bound must be finite and >= 0");
    return BRT_OK;
}
// the kernels read and write whole 16-byte words: a DEVICE buffer of the caller's must be 16-byte aligned (hipMalloc's are)
inline int32_t device_aligned(brt_ctx* ctx, std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if (reinterpret_cast<uintptr_t>(p) & 15u) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "device buffers must be 16-byte aligned");
    return BRT_OK;
}

// The context's staging buffers of a call, each of at least its `bytes`.  Their users run one behind the other, ordered by ev_q, so a
// buffer grows only once no list uses it: ev_q is waited for on the host if any of them is short.
struct StagedBuf { char** ptr; size_t* cap; size_t bytes; };
inline int32_t staged(brt_ctx* ctx, DeviceCtx& dc, std::initializer_list<StagedBuf> bufs) {
    for (const StagedBuf& b : bufs)
        if (*b.cap < b.bytes) { HIP_TRY(ctx, hipEventSynchronize(dc.ev_q)); break; }
    for (const StagedBuf& b : bufs) {
        const int32_t rc = ensure(ctx, b.ptr, b.cap, b.bytes);
        if (rc != BRT_OK) return rc;
    }
    return BRT_OK;
}

// The round trip of a host form: the caller's host planes laid out in d_list_io, each at a multiple of 256 bytes (`staged`: at least 16
// bytes), `stream` put behind ev_q, the planes with an `in` copied to the device, body(d) -- d[i]: plane i on the device, null for an
// absent one -- which enqueues what the device form enqueues, the planes with an `out` copied back, and ev_q recorded behind them: the
// copies out read the buffer.  Nothing is synchronised and no count is read: that is the call's around it.  d_list_io holds nothing else.
struct HostPlane {
    const void* in;      // copied to the device before the body (null: not copied in)
    void* out;           // copied back after it (null: not copied out)
    size_t bytes;        // 0: the plane is absent
};
template <size_t N, class Body>
int32_t host_round_trip(brt_ctx* ctx, DeviceCtx& dc, hipStream_t stream, const HostPlane (&planes)[N], Body&& body) {
    size_t at[N], total = 0u;
    for (size_t i = 0; i < N; i++) { at[i] = total; total += align256(planes[i].bytes); }
    int32_t r = staged(ctx, dc, {{&dc.d_list_io, &dc.list_io_cap, std::max<size_t>(total, 16u)}});
    if (r != BRT_OK) return r;
    HIP_TRY(ctx, hipStreamWaitEvent(stream, dc.ev_q, 0));
    char* d[N];
    for (size_t i = 0; i < N; i++) {
        d[i] = planes[i].bytes ? dc.d_list_io + at[i] : nullptr;
        if (d[i] && planes[i].in) HIP_TRY(ctx, hipMemcpyAsync(d[i], planes[i].in, planes[i].bytes, hipMemcpyHostToDevice, stream));
    }
    r = body(d);
    if (r != BRT_OK) return r;
    for (size_t i = 0; i < N; i++)
        if (d[i] && planes[i].out) HIP_TRY(ctx, hipMemcpyAsync(planes[i].out, d[i], planes[i].bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipEventRecord(dc.ev_q, stream));
    return BRT_OK;
}

// The device table `t` of `key` (not 0) for work on `stream`, which is then behind ev_q.  Another key rewrites the host copy (fill(t.h)
// resizes and fills it) and the device copy only once every list of the context has ended (the upload of the old table among them),
// and the upload is recorded in ev_q, so that a list on another stream starts behind it.
template <class Fill>
int32_t cached_table(brt_ctx* ctx, DeviceCtx& dc, DeviceTable& t, uint64_t key, hipStream_t stream, Fill&& fill) {
    HIP_TRY(ctx, hipStreamWaitEvent(stream, dc.ev_q, 0));
    if (t.key == key && t.d) return BRT_OK;
    HIP_TRY(ctx, hipEventSynchronize(dc.ev_q));
    t.key = 0u;
    fill(t.h);
    const size_t bytes = t.h.size() * sizeof(float);
    const int32_t rc = ensure(ctx, &t.d, &t.cap, bytes);
    if (rc != BRT_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(t.d, t.h.data(), bytes, hipMemcpyHostToDevice, stream));
    HIP_TRY(ctx, hipEventRecord(dc.ev_q, stream));
    t.key = key;
    return BRT_OK;
}

// A call on the first device: body(dc, sc) with the call's stream (stream_of; the host forms pass nullptr, 0: the context's own).  A
// failed call leaves nothing in flight on the context's own streams.  with_reach: behind ensure_query_reach, for the calls that trace.
template <class Body>
int32_t with_list_call(brt_ctx* ctx, void* hip_stream, uint32_t flags, Body&& body) {
    DeviceCtx& dc = ctx->devs[0];
    HIP_TRY(ctx, hipSetDevice(dc.device));
    const int32_t rc = body(dc, stream_of(dc, hip_stream, flags));
    if (rc != BRT_OK) drain_all_streams(ctx);
    return rc;
}
template <class Body>
int32_t with_reach(brt_ctx* ctx, float origin_bound, uint32_t* rebuilt, void* hip_stream, uint32_t flags, Body&& body) {
    const int32_t rc = ensure_query_reach(ctx, origin_bound, rebuilt);
    if (rc != BRT_OK) { drain_all_streams(ctx); return rc; }
    return with_list_call(ctx, hip_stream, flags, body);
}

// One kernel alone on the call's stream: behind(dc, stream) puts the stream behind ev_q (without one: a wait for ev_q; the probe steps
// pass probe_table), enqueue(dc, stream) launches, ev_q is recorded; the own stream synchronises.
template <class Behind, class Enqueue>
int32_t list_step_run(brt_ctx* ctx, void* hip_stream, uint32_t flags, Behind&& behind, Enqueue&& enqueue) {
    return with_list_call(ctx, hip_stream, flags, [&](DeviceCtx& dc, const StreamChoice& sc) -> int32_t {
        int32_t r = behind(dc, sc.stream);
        if (r == BRT_OK) r = enqueue(dc, sc.stream);
        if (r != BRT_OK) return r;
        HIP_TRY(ctx, hipEventRecord(dc.ev_q, sc.stream));
        if (sc.own) HIP_TRY(ctx, hipStreamSynchronize(sc.stream));
        return BRT_OK;
    });
}
template <class Enqueue>
int32_t list_step_run(brt_ctx* ctx, void* hip_stream, uint32_t flags, Enqueue&& enqueue) {
    return list_step_run(ctx, hip_stream, flags, [&](DeviceCtx& dc, hipStream_t stream) -> int32_t {
        HIP_TRY(ctx, hipStreamWaitEvent(stream, dc.ev_q, 0));
        return BRT_OK;
    }, enqueue);
}

// The chunks of a bake on `stream`: n_units units (probes, texels), per_chunk at a time.  body(first, n) enqueues generate ->
// radiance_enqueue -> reduce of one chunk, which runs behind ev_q and records it (the chunks share d_qrays / d_qhits); a counted run
// copies the chunk's three counts out of d_radctl before the next chunk zeroes them.
template <class Body>
int32_t bake_chunks(brt_ctx* ctx, DeviceCtx& dc, hipStream_t stream, uint32_t n_units, uint32_t per_chunk, bool counted, BakeRun* run,
                    Body&& body) {
    run->chunks = (n_units + per_chunk - 1u) / per_chunk;
    if (counted) run->counts.assign((size_t)run->chunks * 3u, 0u);
    for (uint32_t c = 0; c < run->chunks; c++) {
        const uint32_t first = c * per_chunk;
        HIP_TRY(ctx, hipStreamWaitEvent(stream, dc.ev_q, 0));
        const int32_t rc = body(first, std::min(per_chunk, n_units - first));
        if (rc != BRT_OK) return rc;
        if (counted) HIP_TRY(ctx, hipMemcpyAsync(&run->counts[(size_t)c * 3u], dc.d_radctl, 24u, hipMemcpyDeviceToHost, stream));
        HIP_TRY(ctx, hipEventRecord(dc.ev_q, stream));
    }
    return BRT_OK;
}

// A bake export behind its argument checks: the tree's reach (with_reach), then enqueue(dc, stream, counted, &run) on the call's stream;
// the own stream synchronises and is counted; a successful call reports its stats (bake_stats).
template <class Enqueue>
int32_t bake_call(brt_ctx* ctx, float origin_bound, void* hip_stream, uint32_t flags, uint64_t* out_stats8, Enqueue&& enqueue) {
    BakeRun run;
    uint32_t rebuilt = 0u;
    const int32_t rc = with_reach(ctx, origin_bound, &rebuilt, hip_stream, flags, [&](DeviceCtx& dc, const StreamChoice& sc) -> int32_t {
        const int32_t r = enqueue(dc, sc.stream, sc.own, &run);
        if (r != BRT_OK || !sc.own) return r;
        HIP_TRY(ctx, hipStreamSynchronize(sc.stream));
        return BRT_OK;
    });
    if (rc == BRT_OK) bake_stats(ctx, run, rebuilt, out_stats8);
    return rc;
}
// The host form: the bake on the context's own stream over the caller's planes (host_round_trip), enqueue(dc, stream, counted, &run, d)
// with the planes' device addresses.  reached(): what the call checks once the tree is settled, before anything is staged.
template <size_t N, class Enqueue, class Reached = int32_t (*)()>
int32_t bake_call_host(brt_ctx* ctx, float origin_bound, const HostPlane (&planes)[N], uint64_t* out_stats8, Enqueue&& enqueue,
                       Reached reached = [] { return (int32_t)BRT_OK; }) {
    return bake_call(ctx, origin_bound, nullptr, 0u, out_stats8, [&](DeviceCtx& dc, hipStream_t stream, bool counted, BakeRun* run) -> int32_t {
        const int32_t r = reached();
        if (r != BRT_OK) return r;
        return host_round_trip(ctx, dc, stream, planes, [&](char* const* d) { return enqueue(dc, stream, counted, run, d); });
    });
}

// The out_stats8 of a list call: three counts (nullptr: not gathered), tree rebuilt, the callee-built tree's reach (bits), the form, and
// the family's word 6.  list_groups: the workgroups of a launch over n items.  list_launch_stats: the launch fields of the brt_stats of a
// list of pixels; variant: the streaming form's kernel_variant (the plain form's is one more; the persistent kernel's are below 32).
inline uint32_t list_groups(const StreamLaunch& sl, uint32_t n) { return sl.form == LIST_STREAM ? sl.grid : (n + 255u) / 256u; }
inline void list_launch_stats(const StreamLaunch& sl, uint32_t n, uint32_t variant, brt_stats* stats) {
    stats->n_workgroups = list_groups(sl, n);
    stats->threads_per_workgroup = sl.form == LIST_STREAM ? sl.block : 256u;
    stats->lds_bytes = (uint32_t)sl.lds_bytes;
    stats->scene_in_lds = sl.form != LIST_STREAM ? 0u : sl.scene_mode == SCENE_LDS ? 1u : (sl.scene_mode == SCENE_LDS_TOP ? 2u : 0u);
    stats->kernel_variant = variant + (sl.form == LIST_STREAM ? 0u : 1u);
}
template <class Count>
void list_stats8(const brt_ctx* ctx, const Count* counts3, uint32_t rebuilt, int form, uint64_t word6, uint64_t* out8) {
    if (!out8) return;
    const float reach = ctx->tree_callee_sah ? ctx->tree_reach : 0.0f;
    uint32_t reach_bits;
    std::memcpy(&reach_bits, &reach, 4);
    for (uint32_t i = 0; i < 3u; i++) out8[i] = counts3 ? counts3[i] : 0u;
    out8[3] = rebuilt;
    out8[4] = reach_bits;
    out8[5] = (uint64_t)form;
    out8[6] = word6;
    out8[7] = 0u;
}

// A list of caller rays behind its argument checks, both forms (ray queries: QueryLaunch, u32 counts in d_qctl; radiance queries:
// RadianceLaunch, u64 counts in d_radctl).  An empty list reports its stats and touches nothing; else the tree's reach (with_reach), then
// enqueue(dc, stream, counted, &launch) on the call's stream -- the host form's is the device form's inside host_round_trip; the own
// stream copies the three counts out and synchronises (a caller's stream is not waited for: its counts stay 0); the stats (list_stats8,
// word 6: the workgroups of the launch).
template <class Count, class Launch, class Enqueue>
int32_t ray_list_call(brt_ctx* ctx, uint32_t n_rays, float origin_bound, void* hip_stream, uint32_t flags, uint32_t* DeviceCtx::*ctl,
                      uint64_t* out_stats8, Enqueue&& enqueue) {
    Launch l{};
    uint32_t rebuilt = 0u;
    Count counts[3] = {0u, 0u, 0u};
    int32_t rc = BRT_OK;
    if (n_rays != 0u)
        rc = with_reach(ctx, origin_bound, &rebuilt, hip_stream, flags, [&](DeviceCtx& dc, const StreamChoice& sc) -> int32_t {
            const int32_t r = enqueue(dc, sc.stream, sc.own, &l);
            if (r != BRT_OK || !sc.own) return r;
            HIP_TRY(ctx, hipMemcpyAsync(counts, dc.*ctl, sizeof counts, hipMemcpyDeviceToHost, sc.stream));
            HIP_TRY(ctx, hipStreamSynchronize(sc.stream));
            return BRT_OK;
        });
    if (rc == BRT_OK) list_stats8(ctx, counts, rebuilt, l.form, list_groups(l, l.args.n_rays), out_stats8);
    return rc;
}

}  // namespace brt
