// brt_api_volume.cpp -- irradiance volumes (brt_volume.h, brt_volume.hip; DESIGN.md "Irradiance volumes") on the first device: a regular
// lattice of light probes baked in one call, and lists of {position, normal} shaded from the baked records.  The bake is the light
// probes' (brt_api_probe.cpp bake_enqueue) over probes that k_volume_probes writes; the skeleton of a bake export, streams, ordering
// behind ev_q, the staging rule and the round trip of the host forms' buffers are those of every list call (brt_frame.h: bake_call,
// bake_call_host, host_round_trip, with_list_call, staged, list_step_run, device_aligned).  Here: the descriptor's checks, the argument
// packing and the host twins.
#include "brt_frame.h"
#include "brt_volume.h"

using namespace brt;

namespace {

// the caller's 48 bytes -> *v and the number of probes, or the refusal of a descriptor (ctx may be null: the host exports)
int32_t volume_check(brt_ctx* ctx, const void* volume48, VolumeDesc* v, uint32_t* n_probes) {
    if (!volume48) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "volume48 is null");
    std::memcpy(v, volume48, sizeof *v);
    uint64_t n = 1u;
    for (uint32_t a = 0; a < 3u; a++) {
        if (!std::isfinite(v->origin[a])) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "volume: origin must be finite");
        if (!std::isfinite(v->spacing[a]) || !(v->spacing[a] > 0.0f)) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "volume: spacing must be finite and > 0");
        if (v->count[a] < 1u || v->count[a] > kVolumeMaxCount) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "volume: every count must be in [1, 1024]");
        n *= v->count[a];
    }
    if (n > kVolumeMaxProbes) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "volume: more than 1 << 20 probes");
    if (v->basis > PROBE_AMBIENT_CUBE) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "volume: basis must be BRT_PROBE_SH9 or BRT_PROBE_AMBIENT_CUBE");
    if (v->flags & ~kVolumeWrap) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "volume: flags must be 0 or BRT_VOLUME_WRAP");
    *n_probes = (uint32_t)n;
    return BRT_OK;
}

// what the sampling exports check of their buffers (device or host addresses alike); n_points = 0 looks at no pointer
int32_t sample_check(brt_ctx* ctx, uint32_t n_probes, const void* records, const void* points, uint32_t n_points, const void* out) {
    if (n_points > kVolumeMaxPoints) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "n_points too large");
    if (n_points == 0u) return BRT_OK;
    if (!records || !points || !out) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "records / points / out is null");
    if (overlaps(out, (size_t)n_points * 16u, points, (size_t)n_points * 32u) || overlaps(out, (size_t)n_points * 16u, records, (size_t)n_probes * 128u))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "the buffers overlap");
    return BRT_OK;
}

// the rule over a host list
template <uint32_t BASIS, bool WRAP>
void sample_host(const VolumeDesc& v, const void* records, const void* points, uint32_t n_points, void* out) {
    for (uint32_t i = 0; i < n_points; i++) {
        float pt[8], rgb[3];
        std::memcpy(pt, static_cast<const char*>(points) + (size_t)i * 32u, sizeof pt);
        const uint32_t status = volume_sample<BASIS, WRAP>(v, records, pt, pt + 4, rgb);
        char* o = static_cast<char*>(out) + (size_t)i * 16u;
        std::memcpy(o, rgb, 12u);
        std::memcpy(o + 12u, &status, 4u);
    }
}

int32_t volume_probes_enqueue(brt_ctx* ctx, hipStream_t stream, const VolumeDesc& v, uint32_t n_probes, void* d_probes) {
    VolumeProbesArgs a;
    a.volume = v;
    a.probes = static_cast<uint4*>(d_probes);
    a.n_probes = n_probes;
    HIP_TRY(ctx, launch_volume_probes(a, stream));
    return BRT_OK;
}

int32_t volume_sample_enqueue(brt_ctx* ctx, hipStream_t stream, const VolumeDesc& v, const void* d_records, const void* d_points,
                              uint32_t n_points, void* d_out) {
    VolumeSampleArgs a;
    a.volume = v;
    a.records = static_cast<const uint4*>(d_records);
    a.points = static_cast<const uint4*>(d_points);
    a.out = static_cast<uint4*>(d_out);
    a.n_points = n_points;
    HIP_TRY(ctx, launch_volume_sample(a, stream));
    return BRT_OK;
}

// The bake into the DEVICE buffer d_records on `stream`: the lattice's probes in the context's buffer (`staged`), behind ev_q and
// recorded in it, then the light probes' bake over them
int32_t volume_bake_enqueue(brt_ctx* ctx, DeviceCtx& dc, hipStream_t stream, const VolumeDesc& v, uint32_t n_probes, uint32_t n_dirs,
                            uint32_t bounces, void* d_records, bool counted, BakeRun* run) {
    const size_t bytes = (size_t)n_probes * 16u;
    int32_t rc = staged(ctx, dc, {{&dc.d_volume_probes, &dc.volume_probes_cap, bytes}});
    if (rc != BRT_OK) return rc;
    HIP_TRY(ctx, hipStreamWaitEvent(stream, dc.ev_q, 0));
    rc = volume_probes_enqueue(ctx, stream, v, n_probes, dc.d_volume_probes);
    if (rc != BRT_OK) return rc;
    HIP_TRY(ctx, hipEventRecord(dc.ev_q, stream));
    return bake_enqueue(ctx, dc, stream, dc.d_volume_probes, n_probes, n_dirs, bounces, v.basis, d_records, counted, run);
}

// what both bakes check before anything is enqueued
int32_t volume_bake_check(brt_ctx* ctx, const void* volume48, uint32_t n_dirs, uint32_t bounces, float origin_bound, const void* records,
                          VolumeDesc* v, uint32_t* n_probes) {
    int32_t rc = volume_check(ctx, volume48, v, n_probes);
    if (rc != BRT_OK) return rc;
    if (!records) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "records is null");
    return bake_check(ctx, nullptr, 0u, n_dirs, bounces, v->basis, origin_bound, nullptr);      // (the probes are the context's own)
}

}  // namespace

extern "C" {

int32_t brt_host_volume_probes(const void* volume48, void* out_probes) {
    return guard(nullptr, [&]() -> int32_t {
    VolumeDesc v;
    uint32_t n_probes = 0u;
    const int32_t rc = volume_check(nullptr, volume48, &v, &n_probes);
    if (rc != BRT_OK) return rc;
    if (!out_probes) return fail(BRT_ERR_INVALID_ARGUMENT, "out_probes is null");
    for (uint32_t i = 0; i < n_probes; i++) {
        const uint4 pr = volume_probe(v, i);
        std::memcpy(static_cast<char*>(out_probes) + (size_t)i * 16u, &pr, 16u);
    }
    return BRT_OK;
    });
}

int32_t brt_host_volume_sample(const void* volume48, const void* records, const void* points, uint32_t n_points, void* out) {
    return guard(nullptr, [&]() -> int32_t {
    VolumeDesc v;
    uint32_t n_probes = 0u;
    int32_t rc = volume_check(nullptr, volume48, &v, &n_probes);
    if (rc == BRT_OK) rc = sample_check(nullptr, n_probes, records, points, n_points, out);
    if (rc != BRT_OK || n_points == 0u) return rc;
    const bool wrap = (v.flags & kVolumeWrap) != 0u;
    if (v.basis == PROBE_SH9) {
        if (wrap) sample_host<PROBE_SH9, true>(v, records, points, n_points, out);
        else sample_host<PROBE_SH9, false>(v, records, points, n_points, out);
    } else {
        if (wrap) sample_host<PROBE_AMBIENT_CUBE, true>(v, records, points, n_points, out);
        else sample_host<PROBE_AMBIENT_CUBE, false>(v, records, points, n_points, out);
    }
    return BRT_OK;
    });
}

int32_t brt_volume_probes_device(brt_ctx* ctx, const void* volume48, void* d_probes, void* hip_stream, uint32_t flags) {
    return ctx_guard(ctx, [&]() -> int32_t {
    VolumeDesc v;
    uint32_t n_probes = 0u;
    int32_t rc = caller_stream_flags_check(ctx, flags);
    if (rc == BRT_OK) rc = volume_check(ctx, volume48, &v, &n_probes);
    if (rc != BRT_OK) return rc;
    if (!d_probes) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "null device pointer");
    rc = device_aligned(ctx, {d_probes});
    if (rc != BRT_OK) return rc;
    return list_step_run(ctx, hip_stream, flags, [&](DeviceCtx&, hipStream_t stream) { return volume_probes_enqueue(ctx, stream, v, n_probes, d_probes); });
    });
}

int32_t brt_bake_volume_device(brt_ctx* ctx, const void* volume48, uint32_t n_dirs, uint32_t bounces, float origin_bound, void* d_records,
                               void* hip_stream, uint32_t flags, uint64_t* out_stats8) {
    return ctx_guard(ctx, [&]() -> int32_t {
    VolumeDesc v;
    uint32_t n_probes = 0u;
    int32_t rc = caller_stream_flags_check(ctx, flags);
    if (rc == BRT_OK) rc = volume_bake_check(ctx, volume48, n_dirs, bounces, origin_bound, d_records, &v, &n_probes);
    if (rc == BRT_OK) rc = device_aligned(ctx, {d_records});
    if (rc != BRT_OK) return rc;
    return bake_call(ctx, origin_bound, hip_stream, flags, out_stats8, [&](DeviceCtx& dc, hipStream_t stream, bool counted, BakeRun* run) {
        return volume_bake_enqueue(ctx, dc, stream, v, n_probes, n_dirs, bounces, d_records, counted, run);
    });
    });
}

int32_t brt_bake_volume(brt_ctx* ctx, const void* volume48, uint32_t n_dirs, uint32_t bounces, float origin_bound, void* records,
                        uint64_t* out_stats8) {
    return ctx_guard(ctx, [&]() -> int32_t {
    VolumeDesc v;
    uint32_t n_probes = 0u;
    const int32_t rc = volume_bake_check(ctx, volume48, n_dirs, bounces, origin_bound, records, &v, &n_probes);
    if (rc != BRT_OK) return rc;
    return bake_call_host(ctx, origin_bound, {{nullptr, records, (size_t)n_probes * 128u}}, out_stats8,
                          [&](DeviceCtx& dc, hipStream_t stream, bool counted, BakeRun* run, char* const* d) {
        return volume_bake_enqueue(ctx, dc, stream, v, n_probes, n_dirs, bounces, d[0], counted, run);
    });
    });
}

int32_t brt_sample_volume_device(brt_ctx* ctx, const void* volume48, const void* d_records, const void* d_points, uint32_t n_points,
                                 void* d_out, void* hip_stream, uint32_t flags) {
    return ctx_guard(ctx, [&]() -> int32_t {
    VolumeDesc v;
    uint32_t n_probes = 0u;
    int32_t rc = caller_stream_flags_check(ctx, flags);
    if (rc == BRT_OK) rc = volume_check(ctx, volume48, &v, &n_probes);
    if (rc == BRT_OK) rc = sample_check(ctx, n_probes, d_records, d_points, n_points, d_out);
    if (rc == BRT_OK && n_points != 0u) rc = device_aligned(ctx, {d_records, d_points, d_out});
    if (rc != BRT_OK || n_points == 0u) return rc;
    return list_step_run(ctx, hip_stream, flags, [&](DeviceCtx&, hipStream_t stream) {
        return volume_sample_enqueue(ctx, stream, v, d_records, d_points, n_points, d_out);
    });
    });
}

int32_t brt_sample_volume(brt_ctx* ctx, const void* volume48, const void* records, const void* points, uint32_t n_points, void* out) {
    return ctx_guard(ctx, [&]() -> int32_t {
    VolumeDesc v;
    uint32_t n_probes = 0u;
    int32_t rc = volume_check(ctx, volume48, &v, &n_probes);
    if (rc == BRT_OK) rc = sample_check(ctx, n_probes, records, points, n_points, out);
    if (rc != BRT_OK || n_points == 0u) return rc;
    return with_list_call(ctx, nullptr, 0u, [&](DeviceCtx& dc, const StreamChoice&) -> int32_t {
        const int32_t r = host_round_trip(ctx, dc, dc.stream, {{records, nullptr, (size_t)n_probes * 128u}, {points, nullptr, (size_t)n_points * 32u},
                                                               {nullptr, out, (size_t)n_points * 16u}}, [&](char* const* d) {
            return volume_sample_enqueue(ctx, dc.stream, v, d[0], d[1], n_points, d[2]);
        });
        if (r != BRT_OK) return r;
        HIP_TRY(ctx, hipStreamSynchronize(dc.stream));
        return BRT_OK;
    });
    });
}

}  // extern "C"
