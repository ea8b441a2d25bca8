// brt_api.cpp -- the extern "C" boundary (include/bevyray_amd.h): context lifecycle, knobs, scene upload, tree builds.  Its other
// units: brt_api_launch.cpp, brt_api_order.cpp, brt_api_render.cpp, brt_api_post.cpp, brt_api_upscale.cpp, brt_api_query.cpp, brt_api_radiance.cpp, brt_api_probe.cpp, brt_api_volume.cpp, brt_api_envmap.cpp, brt_api_lightmap.cpp; brt_frame.h is what they share.
//
// What each export replaces in the reference is cited in the header.  This file holds no ray
// arithmetic: rays are traced only by the HIP kernels (brt_kernels.hip).  Without a usable
// HIP device brt_create fails with BRT_ERR_NO_DEVICE -- there is no CPU fallback.
#include "brt_frame.h"
#include "brt_sah.h"

using namespace brt;

namespace {

uint32_t env_u32(const char* name, uint32_t dflt) {
    const char* v = std::getenv(name);
    if (!v || !*v) return dflt;
    return (uint32_t)std::strtoul(v, nullptr, 10);
}

void free_device(DeviceCtx& dc) {
    if (hipSetDevice(dc.device) != hipSuccess) return;
    for (void* p : std::initializer_list<void*>{dc.d_scene, dc.d_ctrl, dc.d_strip_table, dc.d_tile, dc.d_gather, dc.d_pack, dc.d_raster_rgba,
             dc.d_raster_depth, dc.d_bvh_scratch, dc.d_tile_cost, dc.d_tile_order, dc.d_order_meta, dc.d_order_scratch, dc.d_slice_state,
             dc.d_record_hits, dc.d_bvh_models, dc.d_denoise, dc.d_temporal, dc.d_tsph, dc.d_uplow, dc.d_qctl, dc.d_qmap, dc.d_qrays, dc.d_qhits,
             dc.d_pxbuf, dc.d_radctl, dc.probe_dirs.d, dc.d_list_io, dc.d_volume_probes,
             dc.d_envmap, dc.envmap_taps.d, dc.d_lightmap, dc.lightmap_dirs.d})
        if (p) (void)hipFree(p);
    if (dc.h_stage) (void)hipHostFree(dc.h_stage);
    for (hipEvent_t e : {dc.ev_copy, dc.ev_asm, dc.ev_in, dc.ev_g0, dc.ev_g1, dc.ev_pack, dc.ev_strip, dc.ev_strip_read, dc.ev_q, dc.ev_dn,
                         dc.ev0, dc.ev1, dc.ev_last, dc.ev_p0, dc.ev_p1})
        if (e) (void)hipEventDestroy(e);
    if (dc.stream) (void)hipStreamDestroy(dc.stream);
    dc = DeviceCtx();
}

constexpr uint32_t kMaxSahModels = 1u << 16;         // host-side binned SAH for callee-built trees up to here
constexpr uint32_t kMaxGpuBuildModels = 1u << 24;   // scratch ~ 250 B per sphere; the grid version of the builder has no structural limit

// A BVH built on the context's first device: models (host) -> nodes (host vector), kernel time in ms.  sah: the binned-SAH tree of
// brt_sah.h (brt_sah.hip), else PLOC (brt_bvh.hip); each byte-identical to its CPU twin.
int32_t build_bvh_on_device(brt_ctx* ctx, const Model* models, uint32_t n, bool sah, float reach, std::vector<BVHNode>* out, double* build_ms) {
    out->clear();
    if (n == 0) return BRT_OK;
    if (n > (sah ? kMaxSahModels : kMaxGpuBuildModels))
        return ctx_fail(ctx, BRT_ERR_UNSUPPORTED, sah ? "GPU SAH build supports up to 65 536 spheres" : "GPU BVH build supports up to 2^24 spheres");
    DeviceCtx& dc = ctx->devs[0];
    HIP_TRY(ctx, hipSetDevice(dc.device));
    int32_t rc = ensure(ctx, &dc.d_bvh_scratch, &dc.bvh_scratch_cap,
                        sah ? sah_scratch_bytes(n) : ploc_scratch_bytes(n, nullptr, ctx->knobs[K_PLOC_ONE_BLOCK_MAX]));
    if (rc != BRT_OK) return rc;
    rc = ensure(ctx, &dc.d_bvh_models, &dc.bvh_models_cap, (size_t)n * sizeof(Model));
    if (rc != BRT_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(dc.d_bvh_models, models, (size_t)n * sizeof(Model), hipMemcpyHostToDevice, dc.stream));
    BVHNode* d_out = nullptr;
    uint32_t* d_info = nullptr;
    HIP_TRY(ctx, hipEventRecord(dc.ev0, dc.stream));
    if (sah) HIP_TRY(ctx, launch_build_sah(reinterpret_cast<const Model*>(dc.d_bvh_models), n, reach, dc.d_bvh_scratch, &d_out, &d_info, dc.stream));
    else HIP_TRY(ctx, launch_build_ploc(reinterpret_cast<const Model*>(dc.d_bvh_models), n, dc.d_bvh_scratch, &d_out, &d_info, ctx->knobs[K_PLOC_ONE_BLOCK_MAX], dc.stream));
    HIP_TRY(ctx, hipEventRecord(dc.ev1, dc.stream));
    out->resize(2 * (size_t)n - 1);
    HIP_TRY(ctx, hipMemcpyAsync(out->data(), d_out, out->size() * sizeof(BVHNode), hipMemcpyDeviceToHost, dc.stream));
    uint32_t info[2] = {0u, 0u};
    HIP_TRY(ctx, hipMemcpyAsync(info, d_info, sizeof info, hipMemcpyDeviceToHost, dc.stream));
    HIP_TRY(ctx, hipStreamSynchronize(dc.stream));
    if (info[0] != 2u * n - 1u) {
        out->clear();
        return ctx_fail(ctx, BRT_ERR_HIP, "GPU BVH build made no progress after " + std::to_string(info[1]) + " rounds");
    }
    if (sah) sah_giant_leaves_first(out->data(), (uint32_t)out->size(), models, n);      // (the rule's last step: brt_sah.h)
    float kernel_ms = 0.0f;
    HIP_TRY(ctx, hipEventElapsedTime(&kernel_ms, dc.ev0, dc.ev1));
    if (build_ms) *build_ms = kernel_ms;
    return BRT_OK;
}

}  // namespace

namespace brt {

// brt_upload_scene; and, with rebuild_level != 0 / `rebuild`, the same scene bytes again (ctx->last_*) in a callee-built SAH tree whose
// leaf pads cover a longer reach (ensure_tree_reach): the dispatch-order history and the dirty-tracking state stay as they are.
int32_t upload_scene(brt_ctx* ctx, const void* models, uint32_t n_models, const void* materials, uint32_t n_materials,
                     const void* bvh_nodes, uint32_t n_nodes, uint32_t level, bool rebuild) {
    if (const uint32_t k = ctx->knobs[K_TEST_THROW]) { ctx->knobs.v[K_TEST_THROW] = 0u; throw_for_test(k); }   // (tests: the exception barrier)
    // Dirty tracking (the reference re-uploads everything every frame, README.md:17 lists that as
    // future work): identical bytes as the last successful upload -> nothing to do, and the tile-cost
    // history stays valid.  BRT_NO_DIRTY_TRACKING=1 disables.
    const size_t mb = (size_t)n_models * sizeof(Model), tb = (size_t)n_materials * sizeof(Material),
                 bb = (bvh_nodes ? (size_t)n_nodes : 0) * sizeof(BVHNode);
    auto same = [](const std::vector<char>& v, const void* p, size_t n) {
        return v.size() == n && (n == 0 || (p && std::memcmp(v.data(), p, n) == 0));
    };
    if (!rebuild && ctx->has_scene && ctx->knobs[K_NO_DIRTY_TRACKING] == 0 && same(ctx->last_models, models, mb) &&
        same(ctx->last_materials, materials, tb) && same(ctx->last_bvh, bvh_nodes, bb))
        return BRT_OK;
    // a frame of an asynchronous entry point (caller's stream) may still be reading the resident scene, or the build scratch: the
    // scene buffers are rewritten only once every device of the context has drained
    for (auto& dc : ctx->devs) {
        HIP_TRY(ctx, hipSetDevice(dc.device));
        for (hipEvent_t e : {dc.ev_last, dc.ev_copy, dc.ev_asm, dc.ev_q}) HIP_TRY(ctx, hipEventSynchronize(e));
    }
    ctx->has_scene = false;
    // the scale of the scene and its big spheres, for the reach a camera needs (brt_sah.h; ensure_tree_reach)
    float reach = 0.0f;
    if (!rebuild) {
        ctx->tree_scene = tree_scene_of(static_cast<const Model*>(models), models ? n_models : 0u);
        ctx->tree_callee_sah = false;
        ctx->tree_level = 0;
        ctx->tree_reach = 0.0f;
        ctx->query_level = 0;
    } else {
        reach = tree_reach_of(ctx->tree_scene.scale, level);
    }
    std::vector<BVHNode> built;
    const BVHNode* nodes = static_cast<const BVHNode*>(bvh_nodes);
    if (n_models > 0 && models && (!bvh_nodes || n_nodes == 0)) {
        // no BVH from the caller: build it here, on the GPU.  Default: the binned-SAH tree of brt_sah.h up to kMaxSahModels spheres
        // (fewer node visits per ray than PLOC: DESIGN.md section 9), PLOC above that or with the knob BRT_BVH_QUALITY=0.
        // BRT_CPU_BVH=1: the CPU twin of either (the same bytes).
        const bool sah = ctx->knobs[K_BVH_QUALITY] != 0u && n_models <= kMaxSahModels;
        const bool on_gpu = ctx->knobs[K_CPU_BVH] == 0u && n_models <= kMaxGpuBuildModels;
        int32_t rc;
        if (on_gpu) rc = build_bvh_on_device(ctx, static_cast<const Model*>(models), n_models, sah, reach, &built, nullptr);
        else rc = sah ? build_bvh_sah(static_cast<const Model*>(models), n_models, reach, &built)
                      : build_bvh_ploc(static_cast<const Model*>(models), n_models, &built);
        if (rc != BRT_OK) return rc;
        ctx->tree_callee_sah = sah;
        ctx->tree_level = level;
        ctx->tree_reach = reach;
        nodes = built.data();
        n_nodes = (uint32_t)built.size();
    }
    std::string err;
    int32_t rc = validate_and_encode(static_cast<const Model*>(models), n_models, static_cast<const Material*>(materials),
                                     n_materials, nodes, n_nodes, &ctx->enc, &err);
    if (rc != BRT_OK) return ctx_fail(ctx, rc, err);
    const EncodedScene& e = ctx->enc;

    // one blob per device, sections 256-byte aligned
    struct Sec { const void* src; size_t bytes; size_t off; };
    Sec secs[6] = {
        {e.pairs.data(), e.pairs.size() * 4, 0}, {e.spheres.data(), e.spheres.size() * 4, 0},
        {e.sphere_material.data(), e.sphere_material.size() * 4, 0}, {e.materials.data(), e.materials.size() * 4, 0},
        {e.leaf_table.data(), e.leaf_table.size() * 4, 0}, {e.sphere_mats.data(), e.sphere_mats.size() * 4, 0}};
    size_t total = 0;
    for (auto& s : secs) { s.off = total; total += align256(s.bytes ? s.bytes : 16); }

    // A tree of the same shape as the one a device last counted the record visits of (an animated scene: the reference re-extracts
    // and re-uploads every frame, extract.rs:299-336, and the spheres move a little) goes up in THAT numbering straight away: the
    // records the view uses stay the ones the LDS tile holds (apply_hot_order), without a pre-pass per upload
    const uint64_t shape = (ctx->knobs[K_HOT_RECORDS] != 0u && !rebuild && e.desc16 && e.simple_tree && e.n_pairs > 64u) ? tree_shape_hash(e) : 0ull;
    ctx->tree_epoch++;          // (the numbering on the devices is the encoder's again unless a device re-applies its own below)
    for (auto& dc : ctx->devs) {
        HIP_TRY(ctx, hipSetDevice(dc.device));
        int32_t r2 = ensure(ctx, &dc.d_scene, &dc.scene_cap, total);
        if (r2 != BRT_OK) return r2;
        const bool reuse = shape != 0ull && dc.hot_shape == shape && dc.hot_records != 0u && dc.h_total_rank.size() == e.n_pairs &&
                           dc.h_total_srank.size() == e.n_models;
        uint32_t root = e.root_desc;
        Sec mine[6];
        for (int q = 0; q < 6; q++) mine[q] = secs[q];
        if (reuse) {
            permute_scene(e.pairs, e.spheres, e.sphere_material, e.sphere_mats, e.root_desc, dc.h_total_rank, dc.h_total_srank, &dc.h_pairs_cur,
                          &dc.h_spheres_cur, &dc.h_sphmat_cur, &dc.h_sphmats_cur, &root);
            mine[0].src = dc.h_pairs_cur.data(); mine[1].src = dc.h_spheres_cur.data(); mine[2].src = dc.h_sphmat_cur.data(); mine[5].src = dc.h_sphmats_cur.data();
        }
        for (auto& s : mine)
            if (s.bytes) HIP_TRY(ctx, hipMemcpyAsync(dc.d_scene + s.off, s.src, s.bytes, hipMemcpyHostToDevice, dc.stream));
        const uint32_t kept_hot = reuse ? dc.hot_records : 0u;
        DeviceSceneView v{};
        v.pairs = reinterpret_cast<const float*>(dc.d_scene + secs[0].off);
        v.spheres = reinterpret_cast<const float*>(dc.d_scene + secs[1].off);
        v.sphere_material = reinterpret_cast<const uint32_t*>(dc.d_scene + secs[2].off);
        v.materials = reinterpret_cast<const float*>(dc.d_scene + secs[3].off);
        v.leaf_table = reinterpret_cast<const uint32_t*>(dc.d_scene + secs[4].off);
        v.sphere_mats = reinterpret_cast<const float*>(dc.d_scene + secs[5].off);
        v.n_pairs = e.n_pairs;
        v.n_models = e.n_models;
        v.n_materials = e.n_materials;
        v.n_leaf_table = (uint32_t)(e.leaf_table.size() / 2);
        v.root_desc = root;
        v.stack_entries = e.stack_entries;
        v.desc16 = e.desc16 ? 1u : 0u;
        v.simple_tree = e.simple_tree ? 1u : 0u;
        v.boxes_ordered = e.boxes_ordered ? 1u : 0u;
        v.spheres_bounded = e.spheres_bounded ? 1u : 0u;
        dc.view = v;
        dc.hot_records = kept_hot;
        if (reuse) dc.hot_tree = ctx->tree_epoch;
        dc.frames_since_upload = 0u;
    }
    for (auto& dc : ctx->devs) {
        HIP_TRY(ctx, hipSetDevice(dc.device));
        HIP_TRY(ctx, hipStreamSynchronize(dc.stream));  // the caller's vectors are no longer referenced
    }
    ctx->has_scene = true;
    if (rebuild) {                                            // (the bytes are ctx->last_* themselves; centre, dirty tracking: unchanged)
        ctx->tree_rebuilds++;
        // another tree: its records have no visit counts yet -- the next frame of a view is a first frame again (pre-pass), as after
        // the camera jump that usually comes with a rebuild
        if (ctx->enc.n_models != 0u && !ctx->enc.pairs.empty())
            for (auto& dc : ctx->devs) if (dc.hot_tree != 0u) { dc.order_valid = false; dc.view_rays = 0; }
        return BRT_OK;
    }
    if (n_models != ctx->last_n_models || tb != ctx->last_materials.size()) ctx->temporal.valid = false;   // another scene: no history
    ctx->last_models.assign(static_cast<const char*>(models), static_cast<const char*>(models) + mb);
    ctx->last_materials.assign(static_cast<const char*>(materials), static_cast<const char*>(materials) + tb);
    if (bb) ctx->last_bvh.assign(static_cast<const char*>(bvh_nodes), static_cast<const char*>(bvh_nodes) + bb);
    else ctx->last_bvh.clear();
    ctx->scene_epoch++;
    {
        double c[3] = {0, 0, 0};
        uint32_t cnt = 0;
        const Model* m = static_cast<const Model*>(models);
        for (uint32_t i = 0; i < n_models; i++) {
            const float* q = m[i].position;
            if (!(std::fabs(m[i].radius) <= 100.0f) || !std::isfinite(q[0]) || !std::isfinite(q[1]) || !std::isfinite(q[2])) continue;
            c[0] += q[0]; c[1] += q[1]; c[2] += q[2];
            cnt++;
        }
        for (int k = 0; k < 3; k++) ctx->scene_centre[k] = cnt ? (float)(c[k] / cnt) : 0.0f;
    }
    // the dispatch order of the views rendered so far stays in use as a hint, but is measured again within kLptAfterUpload
    // frames (a scene that changes every frame: every kLptAfterUpload-th frame is a measuring frame)
    // (a scene with a different number of spheres is a different scene, not the next frame of an animation: its views start
    //  from scratch, with a pre-pass)
    const bool same_shape = ctx->last_n_models == n_models;
    ctx->last_n_models = n_models;
    for (auto& dc : ctx->devs) {
        if (!same_shape) { dc.order_valid = false; dc.view_rays = 0; }
        else if (dc.order_valid && (dc.remeasure_in == 0u || dc.remeasure_in > kLptAfterUpload)) dc.remeasure_in = kLptAfterUpload;
    }
    return BRT_OK;
}

// ---- the callee-built SAH tree and the camera (brt_sah.h "leaf boxes of the tree the CALLEE builds") -------------------------------
// The leaf pads of that tree cover the rounding of the sphere test for rays of up to `reach`; at upload the camera is unknown and the
// tree is built for the scene's own extent, reach = 2 S.  Every render call checks its camera: need = |camera|_1 + S + L (L: the longest
// tangent from the camera to a big sphere -- how far from the camera a primary ray can land on the ground, from where it bounces back
// into the scene).  Reaches come in steps of 2^(1/4) (level k: 2 S * 2^(k / 4), the pads grow by 2^(1/2) per step): a camera that needs
// a higher level than the resident tree has -- or at least two levels less: it has come back -- gets the tree rebuilt on the GPU before
// its frame is launched (brt_sah.hip: 0.2-0.5 ms + the re-encode); never a tree whose pads are below what the camera needs.  A
// caller's tree (and the callee's PLOC tree: the reference's flat 0.1) is honoured as it comes.
// (the rule itself -- tree_scene_of, tree_level_for, tree_reach_of, tree_pads_equal -- is host arithmetic: brt_host.cpp, exported as brt_host_tree_reach)
// before a frame is launched: *rebuilt = the tree was rebuilt for this camera
int32_t ensure_tree_reach(brt_ctx* ctx, const void* camera80, uint32_t* rebuilt) {
    *rebuilt = 0u;
    if (!ctx->has_scene || !ctx->tree_callee_sah || !camera80) return BRT_OK;
    Camera cam;
    std::memcpy(&cam, camera80, sizeof cam);
    uint32_t need = tree_level_for(ctx->tree_scene.scale, ctx->tree_scene.big, cam.position);
    if (need < ctx->query_level) need = ctx->query_level;      // (a ray query asked for more since the upload: brt_query_rays*, origin_bound)
    if (tree_pads_equal(ctx->tree_scene, 0.0f, tree_reach_of(ctx->tree_scene.scale, need))) need = 0u;   // the tree of the scene's own extent is that tree
    if (need <= ctx->tree_level && need + 2u > ctx->tree_level) return BRT_OK;
    // (the cover camera at its usual place already "needs" level 5 -- with every pad still at the 0.01 floor: same bytes, level 0)
    if (tree_pads_equal(ctx->tree_scene, ctx->tree_reach, tree_reach_of(ctx->tree_scene.scale, need))) return BRT_OK;
    *rebuilt = 1u;
    return upload_scene(ctx, ctx->last_models.data(), (uint32_t)(ctx->last_models.size() / sizeof(Model)), ctx->last_materials.data(),
                        (uint32_t)(ctx->last_materials.size() / sizeof(Material)), nullptr, 0u, need, true);
}
void tree_stats(const brt_ctx* ctx, uint32_t rebuilt, brt_stats* stats) {
    if (!stats) return;
    stats->tree_rebuilt = rebuilt;
    stats->tree_reach = ctx->tree_callee_sah ? ctx->tree_reach : 0.0f;
}

}  // namespace brt

namespace {

// brt_build_bvh_device / brt_build_bvh_sah_device: build_bvh_on_device into the caller's node array
int32_t build_bvh_export(brt_ctx* ctx, const void* models, uint32_t n_models, bool sah, float reach, void* out_nodes, uint32_t capacity,
                         uint32_t* out_n_nodes, double* out_build_ms) {
    if (!ctx) return fail(BRT_ERR_INVALID_ARGUMENT, "ctx is null");
    if (!out_n_nodes) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "out_n_nodes is null");
    *out_n_nodes = 0;
    if (n_models == 0) return BRT_OK;
    if (!models) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "models is null");
    std::vector<BVHNode> nodes;
    int32_t rc = build_bvh_on_device(ctx, static_cast<const Model*>(models), n_models, sah, reach, &nodes, out_build_ms);
    if (rc != BRT_OK) return rc;
    *out_n_nodes = (uint32_t)nodes.size();
    if (nodes.size() > capacity || !out_nodes)
        return ctx_fail(ctx, BRT_ERR_CAPACITY, "BVH needs " + std::to_string(nodes.size()) + " nodes, capacity " + std::to_string(capacity));
    std::memcpy(out_nodes, nodes.data(), nodes.size() * sizeof(BVHNode));
    return BRT_OK;
}

}  // namespace

extern "C" {

uint32_t brt_abi_version(void) { return BRT_ABI_VERSION; }

const char* brt_last_error(const brt_ctx* ctx) { return ctx ? ctx->last_error.c_str() : g_last_error.c_str(); }

int32_t brt_create(const int32_t* device_ids, int32_t n_devices, brt_ctx** out_ctx) {
    return guard(nullptr, [&]() -> int32_t {
    if (!out_ctx) return fail(BRT_ERR_INVALID_ARGUMENT, "out_ctx is null");
    *out_ctx = nullptr;
    if (!device_ids || n_devices < 1 || n_devices > 64) return fail(BRT_ERR_INVALID_ARGUMENT, "need 1..64 device ids");
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count < 1)
        return fail(BRT_ERR_NO_DEVICE, std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "count 0") +
                                           " (this library has no CPU path)");
    brt_ctx* ctx = new (std::nothrow) brt_ctx();
    if (!ctx) return guard_fail(nullptr, BRT_ERR_OUT_OF_MEMORY, "out of memory");
    // (anything below that throws -- the vector, a std::string of an error text -- must not leak the context and its device objects)
    struct Cleanup {
        brt_ctx* c;
        ~Cleanup() { if (c) { for (auto& d : c->devs) free_device(d); delete c; } }
    } cleanup{ctx};
    ctx->devs.resize((size_t)n_devices);
    for (int i = 0; i < n_devices; i++) {
        DeviceCtx& dc = ctx->devs[(size_t)i];
        dc.device = device_ids[i];
        int32_t rc = BRT_OK;
        auto body = [&]() -> int32_t {
            if (dc.device < 0 || dc.device >= count)
                return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "device id " + std::to_string(dc.device) + " out of range");
            HIP_TRY(ctx, hipSetDevice(dc.device));
            hipDeviceProp_t prop;
            HIP_TRY(ctx, hipGetDeviceProperties(&prop, dc.device));
            if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
                return ctx_fail(ctx, BRT_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950");
            dc.num_cus = prop.multiProcessorCount;
            int lds = 0;
            HIP_TRY(ctx, hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dc.device));
            dc.max_lds = (size_t)lds;
            HIP_TRY(ctx, hipStreamCreateWithFlags(&dc.stream, hipStreamNonBlocking));
            for (hipEvent_t* e : {&dc.ev0, &dc.ev1, &dc.ev_p0, &dc.ev_p1, &dc.ev_g0, &dc.ev_g1}) HIP_TRY(ctx, hipEventCreate(e));
            for (hipEvent_t* e : {&dc.ev_last, &dc.ev_copy, &dc.ev_asm, &dc.ev_in, &dc.ev_pack, &dc.ev_dn, &dc.ev_strip, &dc.ev_q, &dc.ev_strip_read})
                HIP_TRY(ctx, hipEventCreateWithFlags(e, hipEventDisableTiming));
            // (the events that order work across streams start out complete)
            for (hipEvent_t e : {dc.ev_asm, dc.ev_last, dc.ev_dn, dc.ev_strip, dc.ev_q, dc.ev_strip_read}) HIP_TRY(ctx, hipEventRecord(e, dc.stream));
            HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&dc.d_ctrl), 512));
            HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&dc.d_qctl), 32));
            return BRT_OK;
        };
        rc = body();
        if (rc != BRT_OK) {
            g_last_error = ctx->last_error;
            return rc;          // (cleanup frees the devices and the context)
        }
    }
    // tuning knobs from the environment: once, here, and only on request (BRT_ENABLE_TUNING=1)
    if (env_u32("BRT_ENABLE_TUNING", 0) != 0u)
        for (int k = 0; k < K_COUNT; k++) ctx->knobs.v[k] = env_u32(kKnobs[k].name, kKnobs[k].dflt);
    cleanup.c = nullptr;
    *out_ctx = ctx;
    return BRT_OK;
    });
}

int32_t brt_set_policy(brt_ctx* ctx, uint32_t flags) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (flags & ~kPolicyMask) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "unknown policy flag");
    ctx->policy_flags = flags;
    return BRT_OK;
    });
}

int32_t brt_set_tuning(brt_ctx* ctx, const char* name, uint32_t value) {
    return guard(ctx ? &ctx->last_error : nullptr, [&]() -> int32_t {
    if (!ctx || !name) return fail(BRT_ERR_INVALID_ARGUMENT, "null pointer");
    for (int k = 0; k < K_COUNT; k++)
        if (std::strcmp(name, kKnobs[k].name) == 0) {
            ctx->knobs.v[k] = value;
            if (k == K_QUERY_FORM || k == K_QUERY_STREAM_MIN || k == K_PIXELS_FORM || k == K_RADIANCE_FORM || k == K_PROBE_CHUNK_RAYS) return BRT_OK;   // (ray and radiance queries, pixel lists and probe bakes only: no frame's order depends on them)
            // a knob may change how the dispatch order is built or used: forget the history of every view (the next frame of
            // a view is a "first frame" again: pre-pass, measuring frame)
            for (auto& dc : ctx->devs) { dc.order_valid = false; dc.view_rays = 0; }
            // ... and a knob of the callee's BVH build changes what the same scene bytes upload to: no dirty-tracking shortcut
            if (k == K_BVH_QUALITY || k == K_CPU_BVH || k == K_PLOC_ONE_BLOCK_MAX) ctx->last_models.clear();
            return BRT_OK;
        }
    return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, std::string("unknown tuning knob ") + name);
    });
}

int32_t brt_get_tuning(const brt_ctx* ctx, const char* name, uint32_t* out_value, uint32_t* out_default) {
    return guard(nullptr, [&]() -> int32_t {
    if (!ctx || !name) return fail(BRT_ERR_INVALID_ARGUMENT, "null pointer");
    for (int k = 0; k < K_COUNT; k++)
        if (std::strcmp(name, kKnobs[k].name) == 0) {
            if (out_value) *out_value = ctx->knobs.v[k];
            if (out_default) *out_default = kKnobs[k].dflt;
            return BRT_OK;
        }
    return fail(BRT_ERR_INVALID_ARGUMENT, std::string("unknown tuning knob ") + name);
    });
}

int32_t brt_host_alloc(brt_ctx* ctx, uint64_t bytes, void** out_ptr) {
    return guard(ctx ? &ctx->last_error : nullptr, [&]() -> int32_t {
    if (!ctx || !out_ptr || bytes == 0) return fail(BRT_ERR_INVALID_ARGUMENT, "null pointer / zero size");
    *out_ptr = nullptr;
    HIP_TRY(ctx, hipSetDevice(ctx->devs[0].device));
    void* p = nullptr;
    HIP_TRY(ctx, hipHostMalloc(&p, (size_t)bytes, hipHostMallocPortable));
    ctx->pinned.emplace_back(static_cast<char*>(p), (size_t)bytes);
    *out_ptr = p;
    return BRT_OK;
    });
}

int32_t brt_host_free(brt_ctx* ctx, void* ptr) {
    return ctx_guard(ctx, [&]() -> int32_t {
    for (size_t i = 0; i < ctx->pinned.size(); i++)
        if (ctx->pinned[i].first == ptr) {
            HIP_TRY(ctx, hipHostFree(ptr));
            ctx->pinned.erase(ctx->pinned.begin() + (long)i);
            return BRT_OK;
        }
    return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "pointer was not allocated by brt_host_alloc");
    });
}

int32_t brt_destroy(brt_ctx* ctx) {
    return guard(ctx ? &ctx->last_error : nullptr, [&]() -> int32_t {
    if (!ctx) return BRT_OK;
    release_external_frames(ctx);
    for (auto& b : ctx->pinned) (void)hipHostFree(b.first);
    for (auto& d : ctx->devs) free_device(d);
    delete ctx;
    return BRT_OK;
    });
}

int32_t brt_upload_scene(brt_ctx* ctx, const void* models, uint32_t n_models, const void* materials, uint32_t n_materials,
                         const void* bvh_nodes, uint32_t n_nodes) {
    return ctx_guard(ctx, [&]() -> int32_t {
    return upload_scene(ctx, models, n_models, materials, n_materials, bvh_nodes, n_nodes, 0u, false);
    });
}

int32_t brt_build_bvh_device(brt_ctx* ctx, const void* models, uint32_t n_models, void* out_nodes, uint32_t capacity,
                             uint32_t* out_n_nodes, double* out_build_ms) {
    return guard(ctx ? &ctx->last_error : nullptr, [&]() -> int32_t {
    return build_bvh_export(ctx, models, n_models, false, 0.0f, out_nodes, capacity, out_n_nodes, out_build_ms);
    });
}

int32_t brt_build_bvh_sah_device(brt_ctx* ctx, const void* models, uint32_t n_models, float reach, void* out_nodes, uint32_t capacity,
                                 uint32_t* out_n_nodes, double* out_build_ms) {
    return guard(ctx ? &ctx->last_error : nullptr, [&]() -> int32_t {
    return build_bvh_export(ctx, models, n_models, true, reach, out_nodes, capacity, out_n_nodes, out_build_ms);
    });
}

int32_t brt_debug_profile(brt_ctx* ctx, uint64_t* out64) {
    return guard(ctx ? &ctx->last_error : nullptr, [&]() -> int32_t {
    if (!ctx || !out64) return fail(BRT_ERR_INVALID_ARGUMENT, "null pointer");
    DeviceCtx& dc = ctx->devs[0];
    HIP_TRY(ctx, hipSetDevice(dc.device));
    HIP_TRY(ctx, hipMemcpy(out64, dc.d_ctrl, 512, hipMemcpyDeviceToHost));
    // [40], [41]: critical tiles and longest pixel (rays) of the view's last MEASURED frame, when the order was built on the GPU
    out64[40] = out64[41] = 0;
    out64[42] = (dc.order_valid && !dc.order_on_device) ? dc.order_split : 0u;      // [42]: tiles handed out as two half-sample jobs
    if (dc.order_valid && dc.order_on_device && dc.d_order_meta) {
        uint32_t meta[4] = {0u, 0u, 0u, 0u};
        HIP_TRY(ctx, hipStreamSynchronize(dc.stream));
        HIP_TRY(ctx, hipMemcpy(meta, dc.d_order_meta, sizeof meta, hipMemcpyDeviceToHost));
        out64[40] = meta[0];
        out64[41] = meta[1];
        out64[42] = meta[3];
    }
    return BRT_OK;
    });
}

int32_t brt_debug_eval(brt_ctx* ctx, uint32_t op, const float* in16, float* out8, uint32_t n) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (!in16 || !out8) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "null buffer");
    if (n == 0) return BRT_OK;
    DeviceCtx& dc = ctx->devs[0];
    HIP_TRY(ctx, hipSetDevice(dc.device));
    float* d_in = nullptr;
    float* d_out = nullptr;
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&d_in), (size_t)n * 64));
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d_out), (size_t)n * 32);
    if (e != hipSuccess) { (void)hipFree(d_in); return ctx_fail(ctx, BRT_ERR_HIP, hipGetErrorString(e)); }
    int32_t rc = BRT_OK;
    auto body = [&]() -> int32_t {
        HIP_TRY(ctx, hipMemcpyAsync(d_in, in16, (size_t)n * 64, hipMemcpyHostToDevice, dc.stream));
        HIP_TRY(ctx, launch_debug_eval(op, d_in, d_out, n, dc.stream));
        HIP_TRY(ctx, hipMemcpyAsync(out8, d_out, (size_t)n * 32, hipMemcpyDeviceToHost, dc.stream));
        HIP_TRY(ctx, hipStreamSynchronize(dc.stream));
        return BRT_OK;
    };
    rc = body();
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    return rc;
    });
}

}  // extern "C"
