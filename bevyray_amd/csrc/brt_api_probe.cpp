// brt_api_probe.cpp -- light probes (brt_probe.hip; DESIGN.md "Light probes") on the first device: irradiance records for a list of
// positions.  The rays are radiance entries and are traced by the radiance kernels as they are (brt_api_radiance.cpp radiance_enqueue);
// reach and refusal bound are the ray queries' (brt_api_query.cpp); the skeleton of a bake export, its chunk loop, the cached direction
// table, the round trip of the host form's buffers and the runner of a step export are brt_frame.h's (bake_call, bake_call_host over
// host_round_trip, bake_chunks, cached_table, staged, list_step_run, list_stats8).  Here: the checks, the direction table's maths, the
// argument packing and the host twins.
#include "brt_frame.h"
#include "brt_probe.h"

using namespace brt;

namespace {

constexpr uint32_t kMaxEntries = 0x7fff0000u;        // of one radiance list (radiance_check)
constexpr double kGolden = 0.6180339887498949;       // (sqrt(5) - 1) / 2

// The direction table: a Fibonacci sphere stratified along the up axis, equal weights.  float64, rounded to f32 at the end; the only
// place that computes it (the device reads a table uploaded from here).
void probe_directions(uint32_t n, float* out, uint32_t stride) {
    for (uint32_t k = 0; k < n; k++) {
        const double y = 1.0 - (2.0 * (double)k + 1.0) / (double)n;
        const double r = std::sqrt(std::max(0.0, 1.0 - y * y));
        const double t = (double)k * kGolden;
        const double phi = kTwoPi * (t - std::floor(t));
        out[(size_t)k * stride + 0] = (float)(r * std::cos(phi));
        out[(size_t)k * stride + 1] = (float)y;
        out[(size_t)k * stride + 2] = (float)(r * std::sin(phi));
        if (stride > 3u) out[(size_t)k * stride + 3] = 0.0f;
    }
}

int32_t probe_dirs_check(brt_ctx* ctx, uint32_t n_dirs) {
    if (n_dirs < 1u || n_dirs > kProbeMaxDirs) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "n_dirs must be in [1, 65536]");
    return BRT_OK;
}

// what the step exports check of a list of n_probes x n_dirs entries
int32_t probe_list_check(brt_ctx* ctx, uint32_t n_probes, uint32_t n_dirs) {
    const int32_t rc = probe_dirs_check(ctx, n_dirs);
    if (rc != BRT_OK) return rc;
    if ((uint64_t)n_probes * n_dirs > kMaxEntries) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "n_probes * n_dirs too large");
    return BRT_OK;
}

// The device table of n_dirs directions for work on `stream`, which is then behind ev_q: kept per context by n_dirs (cached_table)
int32_t probe_table(brt_ctx* ctx, DeviceCtx& dc, uint32_t n_dirs, hipStream_t stream) {
    return cached_table(ctx, dc, dc.probe_dirs, n_dirs, stream, [&](std::vector<float>& h) {
        h.resize((size_t)n_dirs * 4u);
        probe_directions(n_dirs, h.data(), 4u);
    });
}

int32_t probe_rays_enqueue(brt_ctx* ctx, DeviceCtx& dc, hipStream_t stream, const void* d_probes, uint32_t n_probes, uint32_t n_dirs,
                           void* d_rays) {
    ProbeRaysArgs a;
    a.probes = static_cast<const uint4*>(d_probes);
    a.dirs = reinterpret_cast<const float4*>(dc.probe_dirs.d);
    a.rays = static_cast<uint4*>(d_rays);
    a.n_probes = n_probes;
    a.n_dirs = n_dirs;
    HIP_TRY(ctx, launch_probe_rays(a, stream));
    return BRT_OK;
}

int32_t probe_project_enqueue(brt_ctx* ctx, DeviceCtx& dc, hipStream_t stream, const void* d_results, uint32_t n_probes, uint32_t n_dirs,
                              uint32_t basis, void* d_out) {
    ProbeProjectArgs a;
    a.results = static_cast<const float4*>(d_results);
    a.dirs = reinterpret_cast<const float4*>(dc.probe_dirs.d);
    a.out = static_cast<uint32_t*>(d_out);
    a.n_probes = n_probes;
    a.n_dirs = n_dirs;
    a.basis = basis;
    HIP_TRY(ctx, launch_probe_project(a, stream));
    return BRT_OK;
}

// what the two step exports check: flags, the list's size, the basis, and `in` / `out` of in_each / out_each bytes per probe
int32_t step_check(brt_ctx* ctx, const void* in, size_t in_each, const void* out, size_t out_each, uint32_t n_probes, uint32_t n_dirs,
                   uint32_t basis, uint32_t flags) {
    int32_t rc = caller_stream_flags_check(ctx, flags);
    if (rc == BRT_OK) rc = probe_list_check(ctx, n_probes, n_dirs);
    if (rc != BRT_OK) return rc;
    if (basis > PROBE_AMBIENT_CUBE) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "basis must be BRT_PROBE_SH9 or BRT_PROBE_AMBIENT_CUBE");
    if (n_probes == 0u) return BRT_OK;
    if (!in || !out) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "null device pointer");
    if (overlaps(in, n_probes * in_each, out, n_probes * out_each)) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "the buffers overlap");
    return BRT_OK;
}

// one step kernel alone on the call's stream (list_step_run), behind ev_q with the table of n_dirs
template <class Enqueue>
int32_t step_run(brt_ctx* ctx, uint32_t n_dirs, void* hip_stream, uint32_t flags, Enqueue&& enqueue) {
    return list_step_run(ctx, hip_stream, flags, [&](DeviceCtx& dc, hipStream_t stream) { return probe_table(ctx, dc, n_dirs, stream); }, enqueue);
}

}  // namespace

namespace brt {

int32_t bake_check(brt_ctx* ctx, const void* probes, uint32_t n_probes, uint32_t n_dirs, uint32_t bounces, uint32_t basis,
                   float origin_bound, const void* out) {
    int32_t rc = probe_dirs_check(ctx, n_dirs);
    if (rc != BRT_OK) return rc;
    if (basis > PROBE_AMBIENT_CUBE) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "basis must be BRT_PROBE_SH9 or BRT_PROBE_AMBIENT_CUBE");
    if (bounces > 65535u) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "bounces must be in [0, 65535]");
    if ((rc = origin_bound_check(ctx, origin_bound)) != BRT_OK) return rc;
    if (n_probes != 0u && (!probes || !out)) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "probes / out is null");
    if (n_probes != 0u && overlaps(probes, (size_t)n_probes * 16u, out, (size_t)n_probes * 128u))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "probes and out overlap");
    if (!ctx->has_scene) return ctx_fail(ctx, BRT_ERR_NO_SCENE, "brt_upload_scene has not succeeded yet");
    if (ctx->policy_flags & kPolicyMask)
        return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, "light probes implement the default policy only (brt_set_policy)");
    return BRT_OK;
}

// The bake of device buffers on `stream`: in chunks of whole probes (bake_chunks), generate -> the radiance launch -> project, all
// behind ev_q, which the last step records.  The lists are staged in d_qrays / d_qhits (one user at a time: `staged`).
int32_t bake_enqueue(brt_ctx* ctx, DeviceCtx& dc, hipStream_t stream, const void* d_probes, uint32_t n_probes, uint32_t n_dirs,
                     uint32_t bounces, uint32_t basis, void* d_out, bool counted, BakeRun* run) {
    const uint32_t chunk_rays = std::min(std::max(ctx->knobs[K_PROBE_CHUNK_RAYS], 1u), kMaxEntries);
    const uint32_t per_chunk = std::min(std::max(1u, chunk_rays / n_dirs), n_probes);
    const size_t bytes = (size_t)per_chunk * n_dirs * 32u;
    int32_t rc = staged(ctx, dc, {{&dc.d_qrays, &dc.qrays_cap, bytes}, {&dc.d_qhits, &dc.qhits_cap, bytes}});
    if (rc == BRT_OK) rc = probe_table(ctx, dc, n_dirs, stream);
    if (rc != BRT_OK) return rc;
    return bake_chunks(ctx, dc, stream, n_probes, per_chunk, counted, run, [&](uint32_t first, uint32_t n) {
        int32_t r = probe_rays_enqueue(ctx, dc, stream, static_cast<const char*>(d_probes) + (size_t)first * 16u, n, n_dirs, dc.d_qrays);
        if (r == BRT_OK) r = radiance_enqueue(ctx, dc, stream, dc.d_qrays, n * n_dirs, 1u, bounces, dc.d_qhits, counted, &run->rl);
        if (r == BRT_OK) r = probe_project_enqueue(ctx, dc, stream, dc.d_qhits, n, n_dirs, basis, static_cast<char*>(d_out) + (size_t)first * 128u);
        return r;
    });
}

void bake_stats(const brt_ctx* ctx, const BakeRun& run, uint32_t rebuilt, uint64_t* out8) {
    uint64_t sums[3] = {0u, 0u, 0u};
    for (size_t i = 0; i < run.counts.size(); i++) sums[i % 3u] += run.counts[i];
    list_stats8(ctx, sums, rebuilt, run.rl.form, run.chunks, out8);
}

}  // namespace brt

namespace {

// E(n) = sum_j A_l(j) c_j Y_j(n): the cosine lobe's band factors pi, 2 pi / 3, pi / 4
constexpr double kPi = 3.141592653589793;
const double kShA[9] = {kPi, 2.0 * kPi / 3.0, 2.0 * kPi / 3.0, 2.0 * kPi / 3.0, kPi / 4.0, kPi / 4.0, kPi / 4.0, kPi / 4.0, kPi / 4.0};

}  // namespace

extern "C" {

int32_t brt_host_probe_directions(uint32_t n_dirs, float* out_xyz) {
    return guard(nullptr, [&]() -> int32_t {
    if (n_dirs < 1u || n_dirs > kProbeMaxDirs) return fail(BRT_ERR_INVALID_ARGUMENT, "n_dirs must be in [1, 65536]");
    if (!out_xyz) return fail(BRT_ERR_INVALID_ARGUMENT, "out_xyz is null");
    probe_directions(n_dirs, out_xyz, 3u);
    return BRT_OK;
    });
}

int32_t brt_host_probe_irradiance(const void* record128, const float* normal3, float* out_rgb3) {
    return guard(nullptr, [&]() -> int32_t {
    if (!record128 || !normal3 || !out_rgb3) return fail(BRT_ERR_INVALID_ARGUMENT, "null pointer");
    float c[kProbeCoeffs];
    uint32_t tail[5];
    std::memcpy(c, record128, sizeof c);
    std::memcpy(tail, static_cast<const char*>(record128) + sizeof c, sizeof tail);
    const uint32_t basis = tail[3];
    const float x = normal3[0], y = normal3[1], z = normal3[2];
    double e[3] = {0.0, 0.0, 0.0};
    if (basis == PROBE_SH9) {
        float Y[9];
        probe_sh9(x, y, z, Y);
        for (uint32_t j = 0; j < 9u; j++)
            for (uint32_t ch = 0; ch < 3u; ch++) e[ch] += kShA[j] * (double)c[3u * j + ch] * (double)Y[j];
    } else if (basis == PROBE_AMBIENT_CUBE) {
        const float n[3] = {x, y, z};
        for (uint32_t axis = 0; axis < 3u; axis++) {
            const uint32_t face = 2u * axis + (n[axis] < 0.0f ? 1u : 0u);
            for (uint32_t ch = 0; ch < 3u; ch++) e[ch] += (double)n[axis] * (double)n[axis] * (double)c[3u * face + ch];
        }
    } else {
        return fail(BRT_ERR_INVALID_ARGUMENT, "the record's basis is neither BRT_PROBE_SH9 nor BRT_PROBE_AMBIENT_CUBE");
    }
    for (uint32_t ch = 0; ch < 3u; ch++) out_rgb3[ch] = (float)e[ch];
    return BRT_OK;
    });
}

int32_t brt_probe_rays_device(brt_ctx* ctx, const void* d_probes, uint32_t n_probes, uint32_t n_dirs, void* d_rays, void* hip_stream,
                              uint32_t flags) {
    return ctx_guard(ctx, [&]() -> int32_t {
    const int32_t rc = step_check(ctx, d_probes, 16u, d_rays, (size_t)n_dirs * 32u, n_probes, n_dirs, PROBE_SH9, flags);
    if (rc != BRT_OK || n_probes == 0u) return rc;
    return step_run(ctx, n_dirs, hip_stream, flags, [&](DeviceCtx& dc, hipStream_t stream) {
        return probe_rays_enqueue(ctx, dc, stream, d_probes, n_probes, n_dirs, d_rays);
    });
    });
}

int32_t brt_probe_project_device(brt_ctx* ctx, const void* d_results, uint32_t n_probes, uint32_t n_dirs, uint32_t basis, void* d_out,
                                 void* hip_stream, uint32_t flags) {
    return ctx_guard(ctx, [&]() -> int32_t {
    const int32_t rc = step_check(ctx, d_results, (size_t)n_dirs * 32u, d_out, 128u, n_probes, n_dirs, basis, flags);
    if (rc != BRT_OK || n_probes == 0u) return rc;
    return step_run(ctx, n_dirs, hip_stream, flags, [&](DeviceCtx& dc, hipStream_t stream) {
        return probe_project_enqueue(ctx, dc, stream, d_results, n_probes, n_dirs, basis, d_out);
    });
    });
}

int32_t brt_bake_probes_device(brt_ctx* ctx, const void* d_probes, uint32_t n_probes, uint32_t n_dirs, uint32_t bounces, uint32_t basis,
                               float origin_bound, void* d_out, void* hip_stream, uint32_t flags, uint64_t* out_stats8) {
    return ctx_guard(ctx, [&]() -> int32_t {
    int32_t rc = caller_stream_flags_check(ctx, flags);
    if (rc == BRT_OK) rc = bake_check(ctx, d_probes, n_probes, n_dirs, bounces, basis, origin_bound, d_out);
    if (rc != BRT_OK) return rc;
    if (n_probes == 0u) { bake_stats(ctx, BakeRun(), 0u, out_stats8); return BRT_OK; }
    return bake_call(ctx, origin_bound, hip_stream, flags, out_stats8, [&](DeviceCtx& dc, hipStream_t stream, bool counted, BakeRun* run) {
        return bake_enqueue(ctx, dc, stream, d_probes, n_probes, n_dirs, bounces, basis, d_out, counted, run);
    });
    });
}

int32_t brt_bake_probes(brt_ctx* ctx, const void* probes, uint32_t n_probes, uint32_t n_dirs, uint32_t bounces, uint32_t basis,
                        float origin_bound, void* out, uint64_t* out_stats8) {
    return ctx_guard(ctx, [&]() -> int32_t {
    int32_t rc = bake_check(ctx, probes, n_probes, n_dirs, bounces, basis, origin_bound, out);
    if (rc != BRT_OK) return rc;
    if (n_probes == 0u) { bake_stats(ctx, BakeRun(), 0u, out_stats8); return BRT_OK; }
    return bake_call_host(ctx, origin_bound, {{probes, nullptr, (size_t)n_probes * 16u}, {nullptr, out, (size_t)n_probes * 128u}}, out_stats8,
                          [&](DeviceCtx& dc, hipStream_t stream, bool counted, BakeRun* run, char* const* d) {
        return bake_enqueue(ctx, dc, stream, d[0], n_probes, n_dirs, bounces, basis, d[1], counted, run);
    });
    });
}

}  // extern "C"
