// brt_ctx.h -- the opaque context of the C ABI (include/bevyray_amd.h) and the helpers its translation units share:
// brt_api*.cpp (upload, launch, order, render, post-passes, upsampling, queries, radiance queries, light probes, irradiance volumes; what only they share: brt_frame.h) and brt_interop.cpp (RCCL
// gather, external-memory frames).  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "brt_adaptive.h"
#include "brt_denoise.h"
#include "brt_temporal.h"
#include "brt_host.h"
#include "brt_kernels.h"
#include "brt_pixels.h"
#include "brt_progressive.h"
#include "brt_query.h"
#include "brt_radiance.h"
#include "brt_upscale.h"

namespace brt {

// A table computed on the host and kept on the device by a key (0: none), with the host copy its upload reads (brt_frame.h cached_table)
struct DeviceTable {
    float* d = nullptr;
    size_t cap = 0;
    uint64_t key = 0;
    std::vector<float> h;
};

struct DeviceCtx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_last = nullptr;   // end of the last launch that used the control block (any stream)
    hipEvent_t ev_p0 = nullptr, ev_p1 = nullptr;   // around the dispatch-order pre-pass of a first frame
    int num_cus = 0;
    size_t max_lds = 0;
    // scene
    char* d_scene = nullptr;
    size_t scene_cap = 0;
    DeviceSceneView view{};
    // control block: 32 x u64 counters @0 (5 stats + section profile @8..23), queue counter @256
    char* d_ctrl = nullptr;
    // frame-sized buffers owned by the context (brt_render)
    float* d_tile = nullptr;
    size_t tile_cap = 0;
    float* d_raster_rgba = nullptr;
    size_t raster_rgba_cap = 0;
    float* d_raster_depth = nullptr;
    size_t raster_depth_cap = 0;
    float* d_gather = nullptr;   // first device only: the tiles of all devices back to back (brt_render_device)
    size_t gather_cap = 0;
    float* d_pack = nullptr;     // first device only: the raster inputs' strips of parts 1 .. N-1, packed per part (brt_render_device)
    size_t pack_cap = 0;
    hipEvent_t ev_pack = nullptr;   // first device: the strips are packed (the other devices' peer copies start behind it)
    hipEvent_t ev_copy = nullptr;   // this device's tile has arrived in the first device's gather buffer
    hipEvent_t ev_asm = nullptr;    // first device: the frame of the last brt_render_device call is assembled (the gather buffer is free)
    hipEvent_t ev_in = nullptr;     // first device: the caller's stream at the start of a brt_render_device call
    hipEvent_t ev_g0 = nullptr, ev_g1 = nullptr;   // first device: around waiting for the tiles + de-interleave
    float* h_stage = nullptr;  // pinned
    size_t stage_cap = 0;
    // longest-first dispatch (see plan_tile_order): this frame's per-tile ray counts and the
    // order derived from the previous frame of the same view
    uint32_t* d_tile_cost = nullptr;
    size_t tile_cost_cap = 0;
    uint32_t* d_tile_order = nullptr;
    uint32_t order_nonsky = 0, order_split = 0;          // host-built order: TileOrder::n_nonsky, n_split (a GPU-built one has them in d_order_meta)
    uint32_t* d_slice_state = nullptr;                   // FrameParams::slice_state
    size_t slice_state_cap = 0;
    uint32_t slice_serial = 0;
    uint32_t order_lane = 0;                             // tiles of the lane queue; the rest of d_tile_order is the tile queue
    uint32_t order_crit = 0;                             // d_tile_order[0 .. crit) are the CRITICAL tiles
    size_t tile_order_cap = 0;
    uint32_t* d_order_meta = nullptr;                    // order built on the GPU: [0] critical tiles, [1] longest pixel
    // strip table on this device (brt_set_strip_table), made once per table: part_of_strip[n_strips], then strip_of[local_strips] of
    // every part in turn -- a call for another part reads its own slice and rewrites nothing
    char* d_strip_table = nullptr;
    size_t strip_table_cap = 0;
    uint32_t strip_epoch = 0;                            // the ctx->strip_epoch the device copy was made for
    std::vector<uint32_t> h_strip_table;                 // the source of its upload (read by the copy after the call has returned)
    hipEvent_t ev_strip = nullptr;                       // the device copy is written (a reader on another stream starts behind it)
    hipEvent_t ev_strip_read = nullptr;                  // end of the last assembly that read it and of every one before (any stream)
    char* d_order_scratch = nullptr;
    size_t order_scratch_cap = 0;
    bool order_on_device = false;                        // d_tile_order / d_order_meta were written by brt_order.hip
    uint64_t view_rays = 0;                              // rays of the last completed frame of the view `view_key` (0: unknown)
    uint32_t view_key[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // order key + sample_count, bounce_count
    // the same pair for the base trace of brt_render_adaptive_device: swapped in around that trace, so that the view's plain frames and
    // its base frames (another sample_count: another key) each find the ray count of their own last frame (brt_api_adaptive.cpp)
    uint64_t base_view_rays = 0;
    uint32_t base_view_key[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool order_valid = false;
    uint32_t remeasure_in = 0;                    // frames until the costs are measured again (0: nothing pending); set by scene uploads
    uint64_t order_cam = 0;                       // hash of the camera the costs were last measured with
    // the last measurement itself stays in d_tile_cost until the next one: a frame whose camera has moved since re-ranks the
    // tiles from it with a neighbourhood radius that covers the motion (attach_tile_order, brt_order.hip)
    bool costs_valid = false;
    float cost_cam_pos[3] = {0, 0, 0}, cost_cam_dir[3] = {0, 0, 0};
    uint32_t cost_spp = 0;
    uint32_t order_key[6] = {0, 0, 0, 0, 0, 0};   // width, height, part, n_parts, scene epoch, n_tiles
    std::vector<uint32_t> h_cost;
    std::vector<uint32_t> h_order;
    // pair records re-numbered by how often the view visits them (brt_api_order.cpp apply_hot_order)
    uint32_t* d_record_hits = nullptr;                   // FrameParams::record_hits of a pre-pass
    size_t record_hits_cap = 0;
    uint32_t hot_tree = 0;                               // brt_ctx::tree_epoch of the tree whose records are in hot order on this device (0: none)
    uint32_t hot_records = 0;                            // ... and how many of them the measuring pre-pass visited at all
    float hot_cam_pos[3] = {0, 0, 0}, hot_cam_dir[3] = {0, 0, 1};   // the camera they were counted with
    uint32_t frames_since_upload = 0;                    // frames this device has rendered since the last scene upload / tree rebuild
    std::vector<uint32_t> h_hits, h_rank;
    std::vector<uint32_t> h_total_rank, h_total_srank;   // the numbering of the records / spheres on this device as a map from the encoder's numbering
    uint64_t hot_shape = 0;                              // tree_shape_hash of the tree that numbering was counted on (0: none)
    std::vector<float> h_spheres_cur, h_sphmats_cur;
    std::vector<uint32_t> h_sphmat_cur;
    std::vector<float> h_pairs_hot, h_pairs_cur;          // scratch / the records as they are on the device (when hot_tree matches)
    // denoiser scratch (brt_denoise.h DenoiseScratch), first device only
    char* d_denoise = nullptr;
    size_t denoise_cap = 0;
    hipEvent_t ev_dn = nullptr;     // end of the last denoise (any stream): the scratch is free again
    // temporal history (brt_temporal.h TemporalHistory), first device only; ordered by ev_dn like the scratch (every temporal frame
    // runs the denoiser's guides and demodulation)
    char* d_temporal = nullptr;
    size_t temporal_cap = 0;
    char* d_tsph = nullptr;         // two slots of float4[n_models] {centre, r^2} in the caller's order, then u32[n_models] resident -> caller
    size_t tsph_cap = 0;
    // the low frame of brt_render_upscaled_device / the base frame of brt_render_adaptive_device (RGBA32F), first device only; ordered
    // by ev_dn like the denoiser's scratch
    float* d_uplow = nullptr;
    size_t uplow_cap = 0;
    // ray queries (brt_query.h), first device only.  Queries of the context run one behind the other (every one waits for ev_q and
    // records it), so the batch counter, the resident -> caller map and the lists of the bakes have one user at a time
    hipEvent_t ev_q = nullptr;      // end of the last query (any stream): uploads, rebuilds and the hot-order renumbering wait for it
    uint32_t* d_qctl = nullptr;     // [0..2] rays walked, hits, refused; [4] the streaming form's batch counter
    uint32_t* d_qmap = nullptr;     // resident sphere index -> the caller's, when the hot order has renumbered the spheres
    size_t qmap_cap = 0;
    uint32_t qmap_tree = 0, qmap_serial = 0;   // the tree_epoch / hot_serial d_qmap was made for (0: none)
    uint32_t hot_serial = 0;        // bumped by every renumbering of the resident spheres (apply_hot_order)
    char* d_qrays = nullptr;        // the probe, envmap and lightmap bakes: the rays of a chunk, and their results
    size_t qrays_cap = 0;
    char* d_qhits = nullptr;
    size_t qhits_cap = 0;
    // sparse pixel tracer, refined upsampling and adaptive sampling (brt_pixels.h), first device only: 8 control words {u64 rays, u64
    // refused entries, the streaming form's batch counter, the entries of the list, -, -}, then the list of brt_upscale_refine* /
    // brt_*adaptive* (one word per output pixel).
    // Its users run one behind the other, ordered by ev_q like the queries (so uploads and renumberings wait for them too)
    uint32_t* d_pxbuf = nullptr;
    size_t pxbuf_cap = 0;
    // radiance queries (brt_radiance.h), first device only: 3 x u64 {walks performed, entries whose own ray hit, entries refused}, then
    // the streaming form's batch counter at word 8.  A radiance list runs behind ev_q and records it, like the ray queries and the pixel
    // lists (so they all run one behind the other, and uploads, rebuilds and renumberings wait for them)
    uint32_t* d_radctl = nullptr;
    size_t radctl_cap = 0;
    // light probes (brt_probe.h), first device only: the direction table {x, y, z, 0}, kept by n_dirs.  A bake stages its lists in
    // d_qrays / d_qhits and is ordered by ev_q like the radiance lists it launches; the table is rewritten only once every list of the
    // context has ended (brt_frame.h cached_table)
    DeviceTable probe_dirs;
    // the device side of every export that takes host buffers of the list families (queries, radiance, bakes, volume samples, pixel and
    // lens lists, progressive frames, the G-buffer): the caller's planes of one call, laid out by host_round_trip (brt_frame.h), and
    // nothing else.  Every user is synchronous on `stream` and reaches the buffer through `staged`: it grows only once every list of the
    // context has ended, and a call has returned before the next one takes it over
    char* d_list_io = nullptr;
    size_t list_io_cap = 0;
    // irradiance volumes (brt_volume.h), first device only: the probes k_volume_probes generates for a bake.  Ordered by ev_q like the
    // staging buffers: it grows only once every list of the context has ended
    char* d_volume_probes = nullptr;
    size_t volume_probes_cap = 0;
    // reflection probes (brt_envmap.h), first device only: the box levels of a bake (and the f32 level 0 of an RGBA16F one), and the tap
    // tables of the levels 1 .. levels - 1 (n_taps taps each), kept by (levels, n_taps).  Ordered by ev_q like the probe buffers
    char* d_envmap = nullptr;
    size_t envmap_cap = 0;
    DeviceTable envmap_taps;
    // lightmaps (brt_lightmap.h), first device only: the resolved f32 image of a bake and the second image of the dilation passes, and
    // the hemisphere's direction table {x, y, z, 0}, kept by n_dirs.  Ordered by ev_q like the probe buffers
    char* d_lightmap = nullptr;
    size_t lightmap_cap = 0;
    DeviceTable lightmap_dirs;
    // GPU BVH build
    char* d_bvh_scratch = nullptr;
    size_t bvh_scratch_cap = 0;
    char* d_bvh_models = nullptr;
    size_t bvh_models_cap = 0;
};


// ---- tuning knobs -----------------------------------------------------------------------------------------------------
// Scheduling / launch-shape knobs of the trace path.  None of them changes a pixel (every one has a test that says so).
// They live in the context: brt_set_tuning(ctx, name, value) sets one; brt_create reads the environment variables of the
// same names ONCE, and only when BRT_ENABLE_TUNING=1 is set -- nothing reads the environment per frame, and the one
// switch that does change pixels (the reading of `||` in raytrace.wgsl:269) is not a knob at all: brt_set_policy.
enum Knob : int {
    K_BOTTOM_UP, K_REFILL_MIN, K_WALK_EXIT, K_LEAF_VOTE, K_DRAIN_DONATE, K_POOL_ADOPT, K_WGQ_BATCH, K_LPT_LANE_PERMILLE, K_TUNABLE,
    K_FORCE_GLOBAL_SCENE, K_FORCE_LDS_TOP, K_BLOCK_THREADS, K_WG_PER_CU, K_POOL_CAP, K_LPT, K_LPT_SORT, K_LPT_SKY_SLACK, K_CRIT,
    K_ORDER_ON_HOST, K_NO_LEAN, K_PREPASS_SPP, K_NO_DIRTY_TRACKING, K_CPU_BVH, K_PLOC_ONE_BLOCK_MAX, K_BVH_QUALITY, K_POOL_FORCE, K_LPT_REFRESH_EVERY, K_LEAN_MEASURE, K_LPT_DILATE, K_SPLIT_TAIL, K_SPLIT_FORCE, K_HOT_RECORDS, K_TEST_THROW, K_QUERY_FORM, K_QUERY_STREAM_MIN, K_PIXELS_FORM, K_RADIANCE_FORM, K_PROBE_CHUNK_RAYS, K_PROGRESSIVE_ORDER, K_COUNT
};
struct KnobDef { const char* name; uint32_t dflt; };
constexpr KnobDef kKnobs[K_COUNT] = {
    {"BRT_BOTTOM_UP", 0}, {"BRT_REFILL_MIN", kRefillMin}, {"BRT_WALK_EXIT", kWalkExitLanes}, {"BRT_LEAF_VOTE", kLeafVote},
    {"BRT_DRAIN_DONATE", kDrainDonate}, {"BRT_POOL_ADOPT", kPoolAdopt}, {"BRT_WGQ_BATCH", 0}, {"BRT_LPT_LANE_PERMILLE", 0},
    {"BRT_TUNABLE", 0}, {"BRT_FORCE_GLOBAL_SCENE", 0}, {"BRT_FORCE_LDS_TOP", 0}, {"BRT_BLOCK_THREADS", 0}, {"BRT_WG_PER_CU", 0},
    {"BRT_POOL_CAP", 384}, {"BRT_LPT", 1}, {"BRT_LPT_SORT", 1}, {"BRT_LPT_SKY_SLACK", 20}, {"BRT_CRIT", 1}, {"BRT_ORDER_ON_HOST", 0},
    {"BRT_NO_LEAN", 0}, {"BRT_PREPASS_SPP", 4}, {"BRT_NO_DIRTY_TRACKING", 0}, {"BRT_CPU_BVH", 0},
    {"BRT_PLOC_ONE_BLOCK_MAX", kPlocOneBlockMax}, {"BRT_BVH_QUALITY", 1}, {"BRT_POOL_FORCE", 0}, {"BRT_LPT_REFRESH_EVERY", 0}, {"BRT_LEAN_MEASURE", 1}, {"BRT_LPT_DILATE", 3}, {"BRT_SPLIT_TAIL", 16}, {"BRT_SPLIT_FORCE", 0}, {"BRT_HOT_RECORDS", 1}, {"BRT_TEST_THROW", 0},
    // ray queries: the form of a call (0: by batch size, 1 plain, 2 streaming) and the batch size from which the default rule streams (0: never)
    {"BRT_QUERY_FORM", 0}, {"BRT_QUERY_STREAM_MIN", 0},
    // sparse pixel tracer: the form of a call (0: streaming unless BRT_FLAG_KERNEL_SIMPLE, 1 plain, 2 streaming)
    {"BRT_PIXELS_FORM", 0},
    // radiance queries: the form of a call (0: streaming from kRadianceStreamMin entries on where the scene has an LDS form, 1 plain, 2 streaming)
    {"BRT_RADIANCE_FORM", 0},
    // light probes: the entries of one chunk of a bake (whole probes, at least one; 64 bytes of staging per entry)
    {"BRT_PROBE_CHUNK_RAYS", 1u << 21},
    // progressive frames: the order of a whole-frame pass (0: raster order, 1: entries in 8x8 tiles, so that a wave's FIRST fetch is one
    // tile -- the streaming form's later refills take single entries; measured 0.25 % faster at 1080p, inside the spread)
    {"BRT_PROGRESSIVE_ORDER", 1}};
struct Knobs {
    uint32_t v[K_COUNT];
    Knobs() { for (int i = 0; i < K_COUNT; i++) v[i] = kKnobs[i].dflt; }
    uint32_t operator[](Knob k) const { return v[k]; }
};

}  // namespace brt

namespace brt {
// a frame target that lives in memory allocated elsewhere (brt_import_frame_fd, brt_interop.cpp)
struct ExternalFrame {
    void* ptr = nullptr;
    size_t bytes = 0, mapped = 0;
    uint32_t type = 0;                                   // BRT_EXTMEM_*
    hipExternalMemory_t ext = nullptr;                   // BRT_EXTMEM_OPAQUE_FD
    hipMemGenericAllocationHandle_t vmm{};               // BRT_EXTMEM_DMABUF_FD (and allocations exported by brt_debug_export_frame_fd)
};
}  // namespace brt

struct brt_ctx {
    std::vector<brt::ExternalFrame> external;   // imported / exported frame targets, released by brt_release_frame / brt_destroy
    std::vector<brt::DeviceCtx> devs;
    brt::EncodedScene enc;
    bool has_scene = false;
    uint32_t scene_epoch = 0;   // bumped by every upload
    // Strip table (brt_set_strip_table): strip_part[s] = the part that renders frame strip s, a permutation of the parts inside every
    // group of n_parts consecutive strips (so that a part's k-th local strip lies in group k: tile layout and gather stay as they are).
    // Empty: strip s belongs to part s % n_parts.
    std::vector<uint32_t> strip_part;
    uint32_t strip_n_parts = 0, strip_epoch = 0;
    uint32_t tree_epoch = 0;    // bumped whenever the encoded tree on the devices is rewritten (uploads, rebuilds for the camera's reach)
    uint32_t last_n_models = 0; // spheres of the last successful upload
    std::vector<std::pair<char*, size_t>> pinned;   // brt_host_alloc blocks
    // bytes of the last successful upload (dirty tracking: an unchanged scene is not re-sent)
    std::vector<char> last_models, last_materials, last_bvh;
    float scene_centre[3] = {0, 0, 0};   // mean centre of the scene's ordinary spheres (radius <= 100): what a camera translation is judged against
    // the callee-built SAH tree and the camera (brt_sah.h "leaf boxes", brt_api.cpp ensure_tree_reach): the leaf pads of the resident
    // tree cover rays of up to tree_reach; a camera that needs more has the tree rebuilt before its frame is launched
    bool tree_callee_sah = false;        // the resident tree was built here with the binned-SAH builder (a caller's tree is honoured as it comes)
    brt::TreeScene tree_scene;           // scale, radii and big spheres of the resident scene (brt_host.h)
    uint32_t tree_level = 0;             // reach of the resident tree = 2 S * 2^(level / 4); level 0: the scene's own extent
    float tree_reach = 0.0f;             // ... as passed to the builder (0 at level 0)
    uint32_t tree_rebuilds = 0;          // rebuilds since brt_create (diagnostic)
    uint32_t query_level = 0;            // the highest level a ray query has asked for since the last upload: cameras do not lower the tree below it
    brt::Knobs knobs;           // tuning knobs (brt_set_tuning; environment once at brt_create under BRT_ENABLE_TUNING=1)
    uint32_t policy_flags = 0;  // brt_set_policy
    brt::DenoiseSettings denoise;   // brt_set_denoise
    struct Adaptive {               // brt_set_adaptive
        uint32_t base_spp = 8;
        float threshold = brt::kAdaptDefaultThreshold;
        uint32_t min_taps = 6;
    } adaptive;
    struct Progressive {            // brt_set_progressive
        uint32_t first_spp = 8, max_spp = 64;
        float threshold = brt::kProgDefaultThreshold;
        uint32_t radius = 1;
    } progressive;
    struct Temporal {               // BRT_FLAG_TEMPORAL
        uint32_t max_history = 32;  // brt_set_temporal
        bool valid = false;         // the history holds a frame (false: n = 0 everywhere)
        uint32_t width = 0, height = 0, set = 0;   // that frame's size and the plane set it wrote
        brt::FrameParams prev{};    // its parameters (camera)
        uint32_t prev_models = 0;   // its sphere count ...
        int64_t prev_epoch = -1;    // ... and the scene_epoch of its spheres
        uint32_t slot_models = 0;   // the sphere count d_tsph is laid out for
        int64_t slot_epoch[2] = {-1, -1};   // the scene_epoch of the spheres in each slot of d_tsph (-1: none)
        std::vector<uint32_t> h_rmap;       // the resident -> caller map on the device (empty: none)
    } temporal;
    std::string last_error;
};

namespace brt {

inline int32_t ctx_fail(brt_ctx* ctx, int32_t code, const std::string& msg) {
    if (ctx) ctx->last_error = msg;
    g_last_error = msg;
    return code;
}

// guard() (brt_host.h) for an export that owns a context: an exception's text is left in the context too, and a null context is refused
template <class F>
inline int32_t ctx_guard(brt_ctx* ctx, F&& body) noexcept {
    return guard(ctx ? &ctx->last_error : nullptr, [&]() -> int32_t {
        if (!ctx) return fail(BRT_ERR_INVALID_ARGUMENT, "ctx is null");
        return body();
    });
}

#define HIP_TRY(ctx, expr)                                                                             \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess)                                                                           \
            return ctx_fail(ctx, BRT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));       \
    } while (0)

template <typename T>
int32_t ensure(brt_ctx* ctx, T** ptr, size_t* cap, size_t bytes) {
    if (*cap >= bytes && *ptr) return BRT_OK;
    if (*ptr) HIP_TRY(ctx, hipFree(*ptr));
    *ptr = nullptr;
    *cap = 0;
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(ptr), bytes));
    *cap = bytes;
    return BRT_OK;
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

void release_external_frames(brt_ctx* ctx);   // brt_interop.cpp; called by brt_destroy

}  // namespace brt

namespace brt {
// strip table (brt_api_order.cpp): the device copy on dc, for work on `stream`; *part_of_strip (frame strip -> part) for the assembly,
// fp->strip_of (fp->part's k-th local strip -> frame strip) for the kernel.  Nothing is attached when the context holds no table for
// fp's frame and split.  An assembly that got a table calls strip_table_read behind its launch.
bool strip_table_valid(const uint32_t* part_of_strip, uint32_t n_strips, uint32_t n_parts);
int32_t strip_table_attach(brt_ctx* ctx, DeviceCtx& dc, FrameParams* fp, const uint32_t** part_of_strip, hipStream_t stream);
int32_t strip_table_read(brt_ctx* ctx, DeviceCtx& dc, const uint32_t* part_of_strip, hipStream_t stream);
uint64_t part_pixels_table(const brt_ctx* ctx, const FrameParams& fp);
}  // namespace brt
