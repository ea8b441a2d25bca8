// brt_api_render.cpp -- the three render paths: one part on one device, a frame to the host, a frame assembled on the first device.
#include "brt_frame.h"

using namespace brt;

namespace brt {

// After a failure inside brt_render some devices may still be tracing, or copying into the caller's
// (possibly page-locked) frame: wait for every stream of the context before the error is returned, so that
// nothing of this call is in flight when the caller gets its buffers back.  The first error message stays.
void drain_all_streams(brt_ctx* ctx) {
    const std::string keep = ctx->last_error;
    for (auto& dc : ctx->devs) {
        if (!dc.stream) continue;
        if (hipSetDevice(dc.device) != hipSuccess) continue;
        (void)hipStreamSynchronize(dc.stream);
    }
    (void)hipGetLastError();
    ctx->last_error = keep;
    g_last_error = keep;
}

}  // namespace brt

namespace {

bool is_pinned(const brt_ctx* ctx, const void* p, size_t bytes) {
    const char* c = static_cast<const char*>(p);
    for (const auto& b : ctx->pinned)
        if (c >= b.first && c + bytes <= b.first + b.second) return true;
    return false;
}

int32_t render_part_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t level, uint32_t width,
                               uint32_t height, uint32_t part, uint32_t n_parts, const float* d_raster_rgba,
                               const float* d_raster_depth, float* d_out_tile, void* hip_stream, uint32_t flags,
                               brt_stats* stats) {
    const auto t0 = std::chrono::steady_clock::now();
    FrameParams fp;
    int32_t rc = make_frame_params(ctx, camera80, window16, level, width, height, part, n_parts, &fp);
    if (rc != BRT_OK) return rc;
    DeviceCtx& dc = ctx->devs[0];
    HIP_TRY(ctx, hipSetDevice(dc.device));
    const auto [own_stream, stream] = stream_of(dc, hip_stream, flags);
    rc = strip_table_attach(ctx, dc, &fp, nullptr, stream);        // the context's strip table, if it is one for this frame and split
    if (rc != BRT_OK) return rc;
    bool prepass_ran = false;
    if (own_stream) {
        rc = prepass_order(ctx, dc, fp, d_raster_rgba, d_raster_depth, d_out_tile, stream, flags, &prepass_ran);
        if (rc != BRT_OK) return rc;
    }
    rc = attach_tile_order(ctx, dc, fp, stream, own_stream, flags);
    if (rc != BRT_OK) return rc;
    LaunchPlan lp{};
    rc = launch_part(ctx, dc, fp, d_raster_rgba, d_raster_depth, d_out_tile, stream, flags, own_stream, &lp);
    if (rc != BRT_OK) return rc;
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        stats->paths = (fp.strip_of ? part_pixels_table(ctx, fp) : part_pixels(fp)) * (uint64_t)fp.sample_count;
        launch_stats(ctx, dc, lp, stats);
    }
    if (own_stream) {      // (a caller's stream is not synchronised: no counters, no times)
        brt_stats tmp{};
        rc = collect_part(ctx, dc, fp, stream, prepass_ran, &tmp);
        if (rc != BRT_OK) return rc;
        if (stats) {
            stats->rays = tmp.rays; stats->node_pops = tmp.node_pops; stats->interior_visits = tmp.interior_visits;
            stats->sphere_tests = tmp.sphere_tests; stats->hits = tmp.hits;
            stats->kernel_ms = tmp.kernel_ms; stats->prepass_ms = tmp.prepass_ms;
            stats->total_ms = ms_since(t0);
        }
    }
    return BRT_OK;
}

int32_t render_frame(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t level, uint32_t width, uint32_t height,
                     const float* raster_rgba, const float* raster_depth, float* out_rgba, uint32_t flags, brt_stats* stats) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t n_parts = (uint32_t)ctx->devs.size();
    std::vector<FrameParams> fps(n_parts);
    for (uint32_t p = 0; p < n_parts; p++) {
        int32_t rc = make_frame_params(ctx, camera80, window16, level, width, height, p, n_parts, &fps[p]);
        if (rc != BRT_OK) return rc;
    }
    const uint32_t tile_rows = brt_tile_rows(height, n_parts);
    const size_t tile_bytes = (size_t)tile_rows * width * 16;
    const size_t frame_px = (size_t)width * height;
    brt_stats st{};
    LaunchPlan lp{};
    std::vector<char> prepass_ran(n_parts, 0);
    const bool direct = is_pinned(ctx, out_rgba, frame_px * 16);
    const bool denoise = (flags & (BRT_FLAG_DENOISE | BRT_FLAG_TEMPORAL)) != 0u;
    const uint32_t post = flags & (BRT_FLAG_DENOISE | BRT_FLAG_TEMPORAL);
    // BRT_FLAG_BLEND_POST: the trace gets the depth and no raster colour (a coverage frame); the colour goes to the first device alone,
    // whole, where the post-passes composite it
    BlendPost bp;
    bp.on = blend_post_on(level, flags);

    // launch every device, then collect: the devices trace their strips concurrently
    for (uint32_t p = 0; p < n_parts; p++) {
        DeviceCtx& dc = ctx->devs[p];
        HIP_TRY(ctx, hipSetDevice(dc.device));
        int32_t rc = ensure(ctx, &dc.d_tile, &dc.tile_cap, tile_bytes);
        if (rc != BRT_OK) return rc;
        const float* d_rgba = nullptr;
        const float* d_depth = nullptr;
        const PartStrips ps(height, p, n_parts);
        // raster inputs: the whole frame for a one-device context; else this device's strips only, densely in the tile's own layout
        // (FrameParams::raster_dense) -- a strided 2-D copy, 1 / n_parts of the bytes over PCIe per device
        auto send = [&](const float* src, float** d_buf, size_t* cap, uint32_t fpp) -> int32_t {
            const size_t px_bytes = (size_t)fpp * 4u;
            if (n_parts == 1) {
                int32_t r = ensure(ctx, d_buf, cap, frame_px * px_bytes);
                if (r != BRT_OK) return r;
                HIP_TRY(ctx, hipMemcpyAsync(*d_buf, src, frame_px * px_bytes, hipMemcpyHostToDevice, dc.stream));
                return BRT_OK;
            }
            int32_t r = ensure(ctx, d_buf, cap, (size_t)tile_rows * width * px_bytes);
            if (r != BRT_OK) return r;
            const size_t row_bytes = (size_t)width * px_bytes, strip_bytes = BRT_STRIP_ROWS * row_bytes;
            if (ps.n_full)                                                                  // the whole strips: one strided copy
                HIP_TRY(ctx, hipMemcpy2DAsync(*d_buf, strip_bytes, reinterpret_cast<const char*>(src) + (size_t)p * strip_bytes,
                                              strip_bytes * n_parts, strip_bytes, ps.n_full, hipMemcpyHostToDevice, dc.stream));
            if (ps.tail_rows)                                                               // the frame's last, partial strip is this part's
                HIP_TRY(ctx, hipMemcpyAsync(reinterpret_cast<char*>(*d_buf) + (size_t)ps.n_full * strip_bytes,
                                            reinterpret_cast<const char*>(src) + ps.frame_row(ps.n_full) * row_bytes,
                                            ps.tail_rows * row_bytes, hipMemcpyHostToDevice, dc.stream));
            return BRT_OK;
        };
        if (raster_rgba && !bp.on) {
            rc = send(raster_rgba, &dc.d_raster_rgba, &dc.raster_rgba_cap, 4u);
            if (rc != BRT_OK) return rc;
            d_rgba = dc.d_raster_rgba;
        }
        if (raster_rgba && bp.on && p == 0) {
            rc = ensure(ctx, &dc.d_raster_rgba, &dc.raster_rgba_cap, frame_px * 16);
            if (rc != BRT_OK) return rc;
            HIP_TRY(ctx, hipMemcpyAsync(dc.d_raster_rgba, raster_rgba, frame_px * 16, hipMemcpyHostToDevice, dc.stream));
            bp.d_raster_rgba = dc.d_raster_rgba;
        }
        if (raster_depth) {
            rc = send(raster_depth, &dc.d_raster_depth, &dc.raster_depth_cap, 1u);
            if (rc != BRT_OK) return rc;
            d_depth = dc.d_raster_depth;
        }
        fps[p].raster_dense = n_parts > 1 ? 1u : 0u;
        if (!direct && dc.stage_cap < tile_bytes) {
            if (dc.h_stage) HIP_TRY(ctx, hipHostFree(dc.h_stage));
            dc.h_stage = nullptr;
            dc.stage_cap = 0;
            HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void**>(&dc.h_stage), tile_bytes, hipHostMallocDefault));
            dc.stage_cap = tile_bytes;
        }
        bool ran = false;
        rc = prepass_order(ctx, dc, fps[p], d_rgba, d_depth, dc.d_tile, dc.stream, flags, &ran);
        if (rc != BRT_OK) return rc;
        prepass_ran[p] = ran;
        rc = attach_tile_order(ctx, dc, fps[p], dc.stream, true, flags);
        if (rc != BRT_OK) return rc;
        rc = launch_part(ctx, dc, fps[p], d_rgba, d_depth, dc.d_tile, dc.stream, flags, true, &lp);
        if (rc != BRT_OK) return rc;
        if (denoise && n_parts == 1) {     // the tile IS the frame: denoised in place before it is copied out
            DenoiseScratch ds;
            FrameParams gp;
            rc = denoise_begin(ctx, dc, camera80, window16, width, height, dc.stream, &gp, &ds);
            if (rc == BRT_OK) rc = run_denoise(ctx, dc, gp, ds, dc.d_tile, dc.d_tile, BRT_FLAG_OUT_RGBA32F, dc.stream, post, bp);
            if (rc != BRT_OK) return rc;
        }
        if (direct && n_parts == 1) {     // page-locked destination, and the tile IS the frame: one copy
            HIP_TRY(ctx, hipMemcpyAsync(out_rgba, dc.d_tile, frame_px * 16, hipMemcpyDeviceToHost, dc.stream));
        } else if (direct) {              // ... else DMA every strip to its place in the frame, no CPU copy
            for (uint32_t k = 0; k < ps.count(); k++)
                HIP_TRY(ctx, hipMemcpyAsync(out_rgba + (size_t)ps.frame_row(k) * width * 4, dc.d_tile + (size_t)k * BRT_STRIP_ROWS * width * 4,
                                            (size_t)ps.rows(k) * width * 16, hipMemcpyDeviceToHost, dc.stream));
        } else {
            HIP_TRY(ctx, hipMemcpyAsync(dc.h_stage, dc.d_tile, tile_bytes, hipMemcpyDeviceToHost, dc.stream));
        }
    }
    for (uint32_t p = 0; p < n_parts; p++) {
        DeviceCtx& dc = ctx->devs[p];
        HIP_TRY(ctx, hipSetDevice(dc.device));
        int32_t rc = collect_part(ctx, dc, fps[p], dc.stream, prepass_ran[p] != 0, &st);
        if (rc != BRT_OK) return rc;
        const auto g0 = std::chrono::steady_clock::now();
        const PartStrips ps(height, p, n_parts);
        for (uint32_t k = 0; !direct && k < ps.count(); k++)
            std::memcpy(out_rgba + (size_t)ps.frame_row(k) * width * 4, dc.h_stage + (size_t)k * BRT_STRIP_ROWS * width * 4,
                        (size_t)ps.rows(k) * width * 16);
        st.gather_ms += ms_since(g0);
        st.paths += part_pixels(fps[p]) * (uint64_t)fps[p].sample_count;
    }
    if (denoise && n_parts > 1) {      // the strips of N devices: the assembled frame goes back to the first device to be denoised
        DeviceCtx& d0 = ctx->devs[0];
        HIP_TRY(ctx, hipSetDevice(d0.device));
        DenoiseScratch ds;
        FrameParams gp;
        int32_t rc = denoise_begin(ctx, d0, camera80, window16, width, height, d0.stream, &gp, &ds);
        if (rc != BRT_OK) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(ds.frame, out_rgba, frame_px * 16, hipMemcpyHostToDevice, d0.stream));
        float4* result = denoise_result_plane(ds, ctx->denoise);      // (a plane the last pass does not read)
        rc = run_denoise(ctx, d0, gp, ds, reinterpret_cast<float*>(ds.frame), result, BRT_FLAG_OUT_RGBA32F, d0.stream, post, bp);
        if (rc != BRT_OK) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(out_rgba, result, frame_px * 16, hipMemcpyDeviceToHost, d0.stream));
        HIP_TRY(ctx, hipStreamSynchronize(d0.stream));
    }
    if (stats) {
        *stats = st;
        stats->total_ms = ms_since(t0);
        launch_stats(ctx, ctx->devs[0], lp, stats);
    }
    return BRT_OK;
}

}  // namespace

namespace brt {

// The frame of an N-device context assembled on its FIRST device: every device traces its strips, the tiles of the
// others travel to the first device's gather buffer by peer copy (xGMI between the GPUs of a node; a plain device copy
// when an ordinal repeats), and k_deinterleave writes the frame -- what bevyray_amd/parallel.py does with one process per
// GPU and an RCCL gather, for a single-process host (the Rust node).
int32_t render_frame_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t level, uint32_t width, uint32_t height,
                            const float* d_raster_rgba, const float* d_raster_depth, void* d_frame, void* hip_stream, uint32_t flags,
                            brt_stats* stats) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t n_parts = (uint32_t)ctx->devs.size();
    // BRT_FLAG_BLEND_POST: no device traces with the raster colour (a coverage frame), so it is not forwarded -- the post-passes read it
    // on the first device, where the caller holds it
    BlendPost bp;
    bp.on = blend_post_on(level, flags);
    if (bp.on) {
        bp.d_raster_rgba = d_raster_rgba;
        d_raster_rgba = nullptr;
    }
    std::vector<FrameParams> fps(n_parts);
    for (uint32_t p = 0; p < n_parts; p++) {
        int32_t rc = make_frame_params(ctx, camera80, window16, level, width, height, p, n_parts, &fps[p]);
        if (rc != BRT_OK) return rc;
    }
    const uint32_t tile_rows = brt_tile_rows(height, n_parts);
    const size_t tile_floats = (size_t)tile_rows * width * 4, tile_bytes = tile_floats * 4;
    DeviceCtx& d0 = ctx->devs[0];
    HIP_TRY(ctx, hipSetDevice(d0.device));
    const auto [own_stream, stream0] = stream_of(d0, hip_stream, flags);
    // A previous asynchronous frame (caller's stream) may still be copying into the gather buffer or reading a tile / raster copy:
    // hipFree only synchronises the current device, so buffers grow only once every device of the context has drained.
    {
        bool grow = d0.gather_cap < tile_bytes * n_parts;
        for (uint32_t p = 1; p < n_parts; p++) {
            const DeviceCtx& dc = ctx->devs[p];
            grow = grow || dc.tile_cap < tile_bytes || (d_raster_rgba && dc.raster_rgba_cap < tile_bytes) ||
                   (d_raster_depth && level != 0u && dc.raster_depth_cap < tile_bytes / 4);
        }
        grow = grow || ((d_raster_rgba || d_raster_depth) && d0.pack_cap < (tile_bytes + tile_bytes / 4) * (n_parts - 1u));
        if (grow)
            for (auto& dc : ctx->devs) {
                HIP_TRY(ctx, hipSetDevice(dc.device));
                for (hipEvent_t e : {dc.ev_last, dc.ev_copy, dc.ev_asm}) HIP_TRY(ctx, hipEventSynchronize(e));
            }
        HIP_TRY(ctx, hipSetDevice(d0.device));
    }
    int32_t rc = ensure(ctx, &d0.d_gather, &d0.gather_cap, tile_bytes * n_parts);
    if (rc != BRT_OK) return rc;
    // the other devices start behind whatever the caller enqueued before this call (its raster inputs)
    HIP_TRY(ctx, hipEventRecord(d0.ev_in, stream0));
    // Raster inputs of the other devices: a device reads only its own strips, so only those travel -- packed per part on the first
    // device (k_pack_strips, the tile's own layout: FrameParams::raster_dense), one peer copy per device and input: 1 / n_parts of
    // the frame each instead of the whole frame (round 4: 41 MB at 1080p, 166 MB at 4K, x 7 devices, every frame at levels 1 / 2)
    const bool fwd_rgba = n_parts > 1 && d_raster_rgba != nullptr, fwd_depth = n_parts > 1 && d_raster_depth != nullptr && level != 0u;
    uint64_t forwarded = 0;
    float* pack_rgba = nullptr;
    float* pack_depth = nullptr;
    if (fwd_rgba || fwd_depth) {
        rc = ensure(ctx, &d0.d_pack, &d0.pack_cap, (tile_bytes + tile_bytes / 4) * (n_parts - 1u));
        if (rc != BRT_OK) return rc;
        pack_rgba = d0.d_pack;
        pack_depth = d0.d_pack + tile_floats * (n_parts - 1u);
        HIP_TRY(ctx, hipStreamWaitEvent(stream0, d0.ev_asm, 0));    // (the previous frame's devices have read the pack buffer: ev_copy sits behind their reads)
        for (uint32_t q = 1; q < n_parts; q++) HIP_TRY(ctx, hipStreamWaitEvent(stream0, ctx->devs[q].ev_last, 0));
        if (fwd_rgba) HIP_TRY(ctx, launch_pack_strips(d_raster_rgba, pack_rgba, width, height, n_parts, tile_rows, 4u, stream0));
        if (fwd_depth) HIP_TRY(ctx, launch_pack_strips(d_raster_depth, pack_depth, width, height, n_parts, tile_rows, 1u, stream0));
        HIP_TRY(ctx, hipEventRecord(d0.ev_pack, stream0));
    }
    LaunchPlan lp{};
    std::vector<char> prepass_ran(n_parts, 0);
    for (uint32_t p = 0; p < n_parts; p++) {
        DeviceCtx& dc = ctx->devs[p];
        HIP_TRY(ctx, hipSetDevice(dc.device));
        hipStream_t sp = p == 0 ? stream0 : dc.stream;
        float* out = d0.d_gather + (size_t)p * tile_floats;
        const float* d_rgba = d_raster_rgba;
        const float* d_depth = d_raster_depth;
        if (p != 0) {
            rc = ensure(ctx, &dc.d_tile, &dc.tile_cap, tile_bytes);
            if (rc != BRT_OK) return rc;
            out = dc.d_tile;
            HIP_TRY(ctx, hipStreamWaitEvent(sp, d0.ev_in, 0));
            HIP_TRY(ctx, hipStreamWaitEvent(sp, d0.ev_asm, 0));     // the gather buffer is free again (previous frame assembled)
            // (level 0 reads the raster colour too -- k_passthrough, raytrace.wgsl:97-99 -- so it is forwarded at every level: a
            //  device must never be handed a pointer into another device's memory, peer access is not enabled)
            if (fwd_rgba || fwd_depth) HIP_TRY(ctx, hipStreamWaitEvent(sp, d0.ev_pack, 0));
            if (fwd_rgba) {
                rc = ensure(ctx, &dc.d_raster_rgba, &dc.raster_rgba_cap, tile_bytes);
                if (rc != BRT_OK) return rc;
                HIP_TRY(ctx, hipMemcpyPeerAsync(dc.d_raster_rgba, dc.device, pack_rgba + (size_t)(p - 1u) * tile_floats, d0.device, tile_bytes, sp));
                d_rgba = dc.d_raster_rgba;
                forwarded += tile_bytes;
            }
            if (fwd_depth) {
                rc = ensure(ctx, &dc.d_raster_depth, &dc.raster_depth_cap, tile_bytes / 4);
                if (rc != BRT_OK) return rc;
                HIP_TRY(ctx, hipMemcpyPeerAsync(dc.d_raster_depth, dc.device, pack_depth + (size_t)(p - 1u) * (tile_floats / 4), d0.device, tile_bytes / 4, sp));
                d_depth = dc.d_raster_depth;
                forwarded += tile_bytes / 4;
            } else if (level == 0u) {
                d_depth = nullptr;
            }
            fps[p].raster_dense = 1u;
        } else {
            HIP_TRY(ctx, hipStreamWaitEvent(sp, d0.ev_asm, 0));
        }
        if (own_stream) {
            bool ran = false;
            rc = prepass_order(ctx, dc, fps[p], d_rgba, d_depth, out, sp, flags, &ran);
            if (rc != BRT_OK) return rc;
            prepass_ran[p] = ran;
        }
        rc = attach_tile_order(ctx, dc, fps[p], sp, own_stream, flags);
        if (rc != BRT_OK) return rc;
        rc = launch_part(ctx, dc, fps[p], d_rgba, d_depth, out, sp, flags, true, &lp);
        if (rc != BRT_OK) return rc;
        if (p != 0) {
            HIP_TRY(ctx, hipMemcpyPeerAsync(d0.d_gather + (size_t)p * tile_floats, d0.device, dc.d_tile, dc.device, tile_bytes, sp));
            HIP_TRY(ctx, hipEventRecord(dc.ev_copy, sp));
            HIP_TRY(ctx, hipEventRecord(dc.ev_last, sp));
        }
    }
    HIP_TRY(ctx, hipSetDevice(d0.device));
    HIP_TRY(ctx, hipEventRecord(d0.ev_g0, stream0));
    for (uint32_t p = 1; p < n_parts; p++) HIP_TRY(ctx, hipStreamWaitEvent(stream0, ctx->devs[p].ev_copy, 0));
    if (flags & (BRT_FLAG_DENOISE | BRT_FLAG_TEMPORAL)) {
        // the assembled RGBA f32 frame (one device: its tile, row for row) is denoised / accumulated into d_frame in the requested format
        DenoiseScratch ds;
        FrameParams gp;
        rc = denoise_begin(ctx, d0, camera80, window16, width, height, stream0, &gp, &ds);
        if (rc != BRT_OK) return rc;
        const float* assembled = d0.d_gather;
        if (n_parts > 1) {
            HIP_TRY(ctx, launch_deinterleave(d0.d_gather, ds.frame, width, height, n_parts, tile_rows, BRT_FLAG_OUT_RGBA32F, stream0));
            assembled = reinterpret_cast<const float*>(ds.frame);
        }
        HIP_TRY(ctx, hipEventRecord(d0.ev_g1, stream0));
        rc = run_denoise(ctx, d0, gp, ds, assembled, d_frame, flags & BRT_FLAG_OUT_MASK, stream0, flags & (BRT_FLAG_DENOISE | BRT_FLAG_TEMPORAL), bp);
        if (rc != BRT_OK) return rc;
    } else {
        HIP_TRY(ctx, launch_deinterleave(d0.d_gather, d_frame, width, height, n_parts, tile_rows, flags & BRT_FLAG_OUT_MASK, stream0));
        HIP_TRY(ctx, hipEventRecord(d0.ev_g1, stream0));
    }
    HIP_TRY(ctx, hipEventRecord(d0.ev_asm, stream0));
    HIP_TRY(ctx, hipEventRecord(d0.ev_last, stream0));
    brt_stats st{};
    st.forwarded_bytes = forwarded;
    for (uint32_t p = 0; p < n_parts; p++) st.paths += part_pixels(fps[p]) * (uint64_t)fps[p].sample_count;
    if (own_stream) {
        for (uint32_t p = 0; p < n_parts; p++) {
            DeviceCtx& dc = ctx->devs[p];
            HIP_TRY(ctx, hipSetDevice(dc.device));
            rc = collect_part(ctx, dc, fps[p], p == 0 ? stream0 : dc.stream, prepass_ran[p] != 0, &st);
            if (rc != BRT_OK) return rc;
        }
        float gms = 0.0f;
        HIP_TRY(ctx, hipEventElapsedTime(&gms, d0.ev_g0, d0.ev_g1));
        st.gather_ms = gms;        // from the end of the first device's trace to the assembled frame (waits for the slowest device)
    }
    if (stats) {
        *stats = st;
        stats->total_ms = ms_since(t0);
        launch_stats(ctx, d0, lp, stats);
    }
    return BRT_OK;
}

}  // namespace brt

namespace {

// What the three render exports share around their own argument checks.  scene_ready: a level that traces needs a scene.  with_tree_reach
// (brt_frame.h) runs each of them on a tree that serves the camera.
int32_t scene_ready(brt_ctx* ctx, uint32_t level) {
    if (!ctx->has_scene && level != 0u) return ctx_fail(ctx, BRT_ERR_NO_SCENE, "brt_upload_scene has not succeeded yet");
    return BRT_OK;
}

}  // namespace

extern "C" {

int32_t brt_render(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t level, uint32_t width, uint32_t height,
                   const float* raster_rgba, const float* raster_depth, float* out_rgba, uint32_t flags, brt_stats* stats) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (!out_rgba) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "out_rgba is null");
    if (const int32_t bad = post_flags_check(ctx, level, flags)) return bad;
    if (const int32_t bad = scene_ready(ctx, level)) return bad;
    if (flags & BRT_FLAG_OUT_MASK) return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, "brt_render writes RGBA f32 (BRT_FLAG_OUT_* apply to the device frame of brt_render_device / brt_gather_rccl / brt_deinterleave_device)");
    return with_tree_reach(ctx, camera80, level, stats, [&] {
        return render_frame(ctx, camera80, window16, level, width, height, raster_rgba, raster_depth, out_rgba, flags, stats);
    });
    });
}

int32_t brt_render_part_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t level, uint32_t width,
                               uint32_t height, uint32_t part, uint32_t n_parts, const float* d_raster_rgba,
                               const float* d_raster_depth, float* d_out_tile, void* hip_stream, uint32_t flags,
                               brt_stats* stats) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (flags & (BRT_FLAG_DENOISE | BRT_FLAG_TEMPORAL | BRT_FLAG_BLEND_POST))
        return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, "a rank's strips have no neighbours: denoise / accumulate the assembled frame (brt_denoise_device, brt_blend_post_device)");
    if (!d_out_tile) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_out_tile is null");
    if (const int32_t bad = scene_ready(ctx, level)) return bad;
    if (flags & BRT_FLAG_OUT_MASK) return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, "a rank's tile is RGBA f32 (the format is applied where the frame is assembled: brt_gather_rccl / brt_deinterleave_device)");
    return with_tree_reach(ctx, camera80, level, stats, [&] {
        return render_part_device(ctx, camera80, window16, level, width, height, part, n_parts, d_raster_rgba, d_raster_depth, d_out_tile,
                                  hip_stream, flags, stats);
    });
    });
}

int32_t brt_render_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t level, uint32_t width, uint32_t height,
                          const float* d_raster_rgba, const float* d_raster_depth, void* d_frame, void* hip_stream, uint32_t flags,
                          brt_stats* stats) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (!d_frame) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "d_frame is null");
    if (const int32_t bad = post_flags_check(ctx, level, flags)) return bad;
    if (const int32_t bad = scene_ready(ctx, level)) return bad;
    if (flags & BRT_FLAG_KERNEL_SIMPLE) return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, "brt_render_device runs the persistent kernel only");
    return with_tree_reach(ctx, camera80, level, stats, [&] {
        return render_frame_device(ctx, camera80, window16, level, width, height, d_raster_rgba, d_raster_depth, d_frame, hip_stream, flags, stats);
    });
    });
}

int32_t brt_deinterleave_device(brt_ctx* ctx, const float* d_tiles, uint32_t n_parts, uint32_t width, uint32_t height,
                                void* d_frame, void* hip_stream, uint32_t flags) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (flags & (BRT_FLAG_DENOISE | BRT_FLAG_TEMPORAL | BRT_FLAG_BLEND_POST))
        return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, "the de-interleave does not denoise or accumulate: brt_denoise_device on the assembled frame");
    if (!d_tiles || !d_frame || n_parts == 0) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "null buffer / n_parts == 0");
    DeviceCtx& dc = ctx->devs[0];
    HIP_TRY(ctx, hipSetDevice(dc.device));
    const auto [own_stream, stream] = stream_of(dc, hip_stream, flags);
    const uint32_t* part_of_strip = nullptr;
    {
        FrameParams key{};                                        // (which frame and split: the table must be one for them)
        key.height = height; key.n_parts = n_parts; key.part = 0u;
        int32_t rc = strip_table_attach(ctx, dc, &key, &part_of_strip, stream);
        if (rc != BRT_OK) return rc;
    }
    HIP_TRY(ctx, launch_deinterleave(d_tiles, d_frame, width, height, n_parts, brt_tile_rows(height, n_parts), flags & BRT_FLAG_OUT_MASK, stream, part_of_strip));
    int32_t rc = strip_table_read(ctx, dc, part_of_strip, stream);
    if (rc != BRT_OK) return rc;
    if (own_stream) HIP_TRY(ctx, hipStreamSynchronize(stream));
    return BRT_OK;
    });
}

}  // extern "C"
