// brt_api_query.cpp -- ray queries (brt_query.hip; DESIGN.md "Ray queries") on the first device, and the launch plan of every list
// kernel (plan_list).  The skeleton of a call -- reach, stream, counts, drain, stats -- and the round trip of the host form's buffers are
// brt_frame.h's (ray_list_call, host_round_trip).
#include "brt_frame.h"

using namespace brt;

namespace {

// The reach level an origin of 1-norm l1 needs of the callee-built tree: tree_level_for's rule for a camera there.  A query gives no
// position, so the tangent to every big sphere is taken from as far as a point of that norm can be from it (|p|_2 <= |p|_1: the
// distance to the centre is at most l1 + |c|_2) -- never less than the camera rule gives at any such position OUTSIDE the sphere, and
// monotone in l1.  Only a big sphere that holds the coordinate origin (a dome) is charged its chord, as the camera rule charges a camera
// inside it; an origin inside any other big sphere (under the ground) gets less here than a camera there would.
uint32_t query_level_for(const TreeScene& ts, double l1) {
    const double S = ts.scale;
    if (!(S > 0.0) || !std::isfinite(S)) return 0u;
    double L = 0.0;
    for (size_t i = 0; i + 3 < ts.big.size(); i += 4) {
        const double cx = ts.big[i], cy = ts.big[i + 1], cz = ts.big[i + 2], r = ts.big[i + 3];
        const double c = std::sqrt(cx * cx + cy * cy + cz * cz), h = l1 + c - r;
        double t = h > 0.0 ? std::sqrt(h * (2.0 * r + h)) : 0.0;
        if (c < r && t < 2.0 * r) t = 2.0 * r;
        if (t > L) L = t;
    }
    const double need = l1 + S + L;
    if (!std::isfinite(need)) return kTreeLevelMax;
    if (need <= 2.0 * S) return 0u;
    const double k = std::ceil(4.0 * std::log2(need / (2.0 * S)));
    return k < 1.0 ? 1u : (k > (double)kTreeLevelMax ? kTreeLevelMax : (uint32_t)k);
}

// the resident callee-built tree serves an origin that needs `level`: it was built for that level or a higher one, or for the same pads
bool tree_covers(const brt_ctx* ctx, uint32_t level) {
    return level <= ctx->tree_level || tree_pads_equal(ctx->tree_scene, ctx->tree_reach, tree_reach_of(ctx->tree_scene.scale, level));
}

}  // namespace

namespace brt {

// the largest origin 1-norm the resident tree covers (+INF: any; < 0: none)
float query_bound_of(const brt_ctx* ctx) {
    const float inf = std::numeric_limits<float>::infinity();
    if (!ctx->tree_callee_sah) return inf;                      // a caller's tree (and the callee's PLOC tree) is honoured as it comes
    const TreeScene& ts = ctx->tree_scene;
    if (!(ts.scale > 0.0f) || !std::isfinite(ts.scale)) return inf;
    if (tree_covers(ctx, kTreeLevelMax)) return inf;
    if (!tree_covers(ctx, query_level_for(ts, 0.0))) return -1.0f;
    double lo = 0.0, hi = 1.0;
    while (hi < 1.0e39 && tree_covers(ctx, query_level_for(ts, hi))) { lo = hi; hi *= 2.0; }
    if (hi >= 1.0e39) return inf;
    for (int i = 0; i < 100 && hi - lo > 0.0; i++) {
        const double mid = 0.5 * (lo + hi);
        if (mid <= lo || mid >= hi) break;
        if (tree_covers(ctx, query_level_for(ts, mid))) lo = mid; else hi = mid;
    }
    float b = (float)lo;
    if ((double)b > lo) b = std::nextafter(b, 0.0f);            // (rounded down: every f32 norm <= b is covered)
    return b;
}

// origin_bound > 0: the tree's reach raised, if needed, to what origins of that 1-norm need
int32_t ensure_query_reach(brt_ctx* ctx, float origin_bound, uint32_t* rebuilt) {
    *rebuilt = 0u;
    if (!(origin_bound > 0.0f) || !ctx->tree_callee_sah) return BRT_OK;
    const uint32_t need = query_level_for(ctx->tree_scene, (double)origin_bound);
    if (!tree_covers(ctx, need)) {
        const int32_t rc = upload_scene(ctx, ctx->last_models.data(), (uint32_t)(ctx->last_models.size() / sizeof(Model)), ctx->last_materials.data(),
                                        (uint32_t)(ctx->last_materials.size() / sizeof(Material)), nullptr, 0u, need, true);
        if (rc != BRT_OK) return rc;
        *rebuilt = 1u;
    }
    if (need > ctx->query_level) ctx->query_level = need;       // (cameras keep it from now on: ensure_tree_reach)
    return BRT_OK;
}

// The form rule of a list of n rays: knob value 1 / 2 force the plain / the streaming form; else a list of at least stream_min rays
// streams (0: none does)
bool list_streams(uint32_t form, uint32_t stream_min, uint32_t n) {
    return !(form == 1u || (form != 2u && (stream_min == 0u || n < stream_min)));
}

}  // namespace brt

namespace {

// The streaming forms stage what k_trace_persistent would (plan_launch): the whole scene where it fits a workgroup's LDS beside the
// stacks, else the top of the tree, else nothing (scenes of 32-bit descriptors, BRT_FORCE_GLOBAL_SCENE); BRT_FORCE_LDS_TOP=<records> as
// there.
void plan_stream(const brt_ctx* ctx, const DeviceCtx& dc, uint32_t n_items, uint32_t waves_by_hand, uint32_t waves_other, StreamLaunch* sp) {
    const Knobs& kn = ctx->knobs;
    sp->form = LIST_STREAM;
    const bool force_global = kn[K_FORCE_GLOBAL_SCENE] != 0u;
    const uint32_t force_top = kn[K_FORCE_LDS_TOP];
    uint32_t per_cu = 1u;
    if (!force_global && !force_top && dc.view.desc16) {
        for (uint32_t block : {1024u, 512u, 256u}) {
            const size_t need = trace_lds_bytes(dc.view, SCENE_LDS, block, 0u);
            if (need <= dc.max_lds) { sp->scene_mode = SCENE_LDS; sp->block = block; sp->lds_bytes = need; break; }
        }
    }
    if (sp->scene_mode != SCENE_LDS && !force_global && dc.view.desc16) {
        const size_t fixed = trace_lds_bytes(sp->scene, SCENE_LDS_TOP, BRT_BLOCK, 0u);       // (lds_pairs = 0: stacks only)
        if (fixed + 64 * PAIR_BYTES <= dc.max_lds) {
            uint32_t k = (uint32_t)((dc.max_lds - fixed) / PAIR_BYTES);
            if (k > dc.view.n_pairs) k = dc.view.n_pairs;
            if (force_top && force_top < k) k = force_top;
            sp->scene.lds_pairs = k;
            sp->scene_mode = SCENE_LDS_TOP;
            sp->block = BRT_BLOCK;
            sp->lds_bytes = trace_lds_bytes(sp->scene, SCENE_LDS_TOP, BRT_BLOCK, 0u);
        }
    }
    if (sp->scene_mode == SCENE_GLOBAL) {
        sp->block = 256u;
        sp->lds_bytes = trace_lds_bytes(dc.view, SCENE_GLOBAL, 256u, 0u);
        per_cu = (uint32_t)(dc.max_lds / (sp->lds_bytes ? sp->lds_bytes : 1));
        const uint32_t by_regs = (dc.view.desc16 && dc.view.simple_tree) ? waves_by_hand : waves_other;
        if (per_cu > by_regs) per_cu = by_regs;
        if (per_cu < 1u) per_cu = 1u;
    }
    sp->grid = (uint32_t)dc.num_cus * per_cu;
    const uint32_t useful = (n_items + sp->block - 1u) / sp->block;
    if (sp->grid > useful) sp->grid = useful;
    if (sp->grid < 1u) sp->grid = 1u;
}

}  // namespace

namespace brt {

void plan_list(const brt_ctx* ctx, const DeviceCtx& dc, uint32_t n_items, bool streams, uint32_t waves_by_hand, uint32_t waves_other,
               bool need_lds, StreamLaunch* sl) {
    StreamLaunch plain{};
    plain.scene = dc.view;
    plain.scene.lds_pairs = 0u;
    plain.form = LIST_PLAIN;
    plain.scene_mode = SCENE_GLOBAL;
    *sl = plain;
    if (!streams) return;
    plan_stream(ctx, dc, n_items, waves_by_hand, waves_other, sl);
    if (need_lds && sl->scene_mode == SCENE_GLOBAL) *sl = plain;
}

// the resident -> caller sphere map of the first device for work on `stream` (nullptr: the resident order is the upload order)
int32_t query_rmap(brt_ctx* ctx, DeviceCtx& dc, hipStream_t stream, const uint32_t** rmap) {
    *rmap = nullptr;
    const uint32_t m = dc.view.n_models;
    if (dc.hot_tree != ctx->tree_epoch || dc.h_total_srank.size() != m || m == 0u) return BRT_OK;
    if (dc.qmap_tree != ctx->tree_epoch || dc.qmap_serial != dc.hot_serial || !dc.d_qmap) {
        int32_t rc = ensure(ctx, &dc.d_qmap, &dc.qmap_cap, (size_t)m * 4u);
        if (rc != BRT_OK) return rc;
        std::vector<uint32_t> map(m);
        for (uint32_t i = 0; i < m; i++) map[dc.h_total_srank[i]] = i;      // h_total_srank[caller index] = resident index
        HIP_TRY(ctx, hipMemcpyAsync(dc.d_qmap, map.data(), (size_t)m * 4u, hipMemcpyHostToDevice, stream));
        HIP_TRY(ctx, hipStreamSynchronize(stream));                          // (a pageable source; after a renumbering only)
        dc.qmap_tree = ctx->tree_epoch;
        dc.qmap_serial = dc.hot_serial;
    }
    *rmap = dc.d_qmap;
    return BRT_OK;
}

}  // namespace brt

namespace {

// one batch on `stream`, behind the previous query of the context; counted: the counts are gathered (the caller synchronises and reads d_qctl)
int32_t query_enqueue(brt_ctx* ctx, DeviceCtx& dc, hipStream_t stream, const void* d_rays, uint32_t n_rays, uint32_t mode, void* d_hits,
                      bool counted, QueryLaunch* ql) {
    HIP_TRY(ctx, hipStreamWaitEvent(stream, dc.ev_q, 0));
    // the form: list_streams under BRT_QUERY_FORM and BRT_QUERY_STREAM_MIN.  Waves per SIMD: the simple-tree instantiation of 16-bit
    // descriptors holds the hand-written loop's 114 VGPRs (4), the others 60-64 (8)
    const Knobs& kn = ctx->knobs;
    plan_list(ctx, dc, n_rays, list_streams(kn[K_QUERY_FORM], kn[K_QUERY_STREAM_MIN], n_rays), 4u, 8u, false, ql);
    const uint32_t* rmap = nullptr;
    int32_t rc = query_rmap(ctx, dc, stream, &rmap);
    if (rc != BRT_OK) return rc;
    QueryArgs& qa = ql->args;
    qa.rays = static_cast<const float4*>(d_rays);
    qa.hits = static_cast<float4*>(d_hits);
    qa.n_rays = n_rays;
    qa.mode = mode;
    qa.bound = query_bound_of(ctx);
    qa.rmap = rmap;
    qa.stat = counted ? dc.d_qctl : nullptr;
    qa.counter = dc.d_qctl + 4;
    ql->stream = stream;
    if (counted || ql->form == LIST_STREAM) HIP_TRY(ctx, hipMemsetAsync(dc.d_qctl, 0, 32, stream));
    HIP_TRY(ctx, launch_query(*ql));
    HIP_TRY(ctx, hipEventRecord(dc.ev_q, stream));
    return BRT_OK;
}

int32_t query_check(brt_ctx* ctx, const void* rays, uint32_t n_rays, uint32_t mode, float origin_bound, const void* hits) {
    if (mode != BRT_QUERY_CLOSEST && mode != BRT_QUERY_ANY) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "mode must be BRT_QUERY_CLOSEST or BRT_QUERY_ANY");
    if (const int32_t rc = origin_bound_check(ctx, origin_bound)) return rc;
    if (n_rays > 0x7fff0000u) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "n_rays too large");
    if (n_rays != 0u && (!rays || !hits)) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "rays / hits is null");
    if (!ctx->has_scene) return ctx_fail(ctx, BRT_ERR_NO_SCENE, "brt_upload_scene has not succeeded yet");
    return BRT_OK;
}

}  // namespace

extern "C" {

int32_t brt_query_rays_device(brt_ctx* ctx, const void* d_rays, uint32_t n_rays, uint32_t mode, float origin_bound, void* d_hits,
                              void* hip_stream, uint32_t flags, uint64_t* out_stats8) {
    return ctx_guard(ctx, [&]() -> int32_t {
    int32_t rc = caller_stream_flags_check(ctx, flags);
    if (rc == BRT_OK) rc = query_check(ctx, d_rays, n_rays, mode, origin_bound, d_hits);
    if (rc != BRT_OK) return rc;
    return ray_list_call<uint32_t, QueryLaunch>(ctx, n_rays, origin_bound, hip_stream, flags, &DeviceCtx::d_qctl, out_stats8,
                                                [&](DeviceCtx& dc, hipStream_t stream, bool counted, QueryLaunch* ql) {
        return query_enqueue(ctx, dc, stream, d_rays, n_rays, mode, d_hits, counted, ql);
    });
    });
}

int32_t brt_query_rays(brt_ctx* ctx, const void* rays, uint32_t n_rays, uint32_t mode, float origin_bound, void* hits, uint64_t* out_stats8) {
    return ctx_guard(ctx, [&]() -> int32_t {
    const int32_t rc = query_check(ctx, rays, n_rays, mode, origin_bound, hits);
    if (rc != BRT_OK) return rc;
    const size_t bytes = (size_t)n_rays * 32u;
    return ray_list_call<uint32_t, QueryLaunch>(ctx, n_rays, origin_bound, nullptr, 0u, &DeviceCtx::d_qctl, out_stats8,
                                                [&](DeviceCtx& dc, hipStream_t stream, bool counted, QueryLaunch* ql) {
        return host_round_trip(ctx, dc, stream, {{rays, nullptr, bytes}, {nullptr, hits, bytes}}, [&](char* const* d) {
            return query_enqueue(ctx, dc, stream, d[0], n_rays, mode, d[1], counted, ql);
        });
    });
    });
}

int32_t brt_query_origin_bound(brt_ctx* ctx, float* out_bound) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (!out_bound) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "out_bound is null");
    if (!ctx->has_scene) return ctx_fail(ctx, BRT_ERR_NO_SCENE, "brt_upload_scene has not succeeded yet");
    *out_bound = query_bound_of(ctx);
    return BRT_OK;
    });
}

}  // extern "C"
