// brt_api_order.cpp -- the dispatch order of the tiles (measured costs, pre-pass), pair records in the order of their use, the strip table.
#include "brt_frame.h"

using namespace brt;

namespace {

// Dispatch order of the 8x8 tiles (brt_host.cpp build_tile_order has the rule).  The cost of a tile is not
// known in advance, but a renderer draws nearly the same frame again and again: the kernel measures the rays
// each tile needed (sum and longest pixel: two atomics per finished pixel, on the frames named below) and the next
// frames use the order built from that.  Pixels never change, only the queue order does.
// BRT_LPT=0 disables (raster order); BRT_LPT_SORT, BRT_LPT_LANE_PERMILLE, BRT_LPT_SKY_SLACK, BRT_CRIT: see
// update_tile_order.
// When the costs are measured again (round 4; the measurement itself runs in the LEAN instantiations now and costs a frame ~1 %):
//   * never for a view whose camera and scene do not change: there is nothing new to measure (until round 3: every 64th frame);
//   * EVERY frame while the camera moves (the reference's demo is a fly-camera app, src/main.rs:40): the order a frame runs in
//     is then the one measured on the frame before it -- one frame stale instead of up to 64;
//   * within kLptAfterUpload frames of a scene upload (an animated scene re-uploads every frame, extract.rs:299-336).
// The order is a hint: a stale one costs speed, never a pixel.
bool lpt_enabled(const brt_ctx* ctx) { return ctx->knobs[K_LPT] != 0; }
uint64_t camera_hash(const FrameParams& fp) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const float* f, int n) {
        for (int i = 0; i < n; i++) { uint32_t u; std::memcpy(&u, f + i, 4); h = (h ^ u) * 1099511628211ull; }
    };
    mix(fp.cam_pos, 3); mix(fp.cam_dir, 3); mix(fp.cam_up, 3); mix(&fp.tan_half_fov, 1); mix(&fp.aspect, 1);
    return h | 1ull;    // never 0 (= "not measured yet")
}

// The dispatch order only depends on which tiles hold long pixels: it survives a scene upload (an animated scene
// re-uploads every frame, extract.rs:299-336, and moves little between two frames) and is measured again soon after one
// (brt_upload_scene ages it); it never affects pixels.  The ray count of a view (LEAN = 2: "no pixel chain can be
// critical") additionally depends on sample and bounce counts; a wrong guess after a scene change only costs speed.
void order_key_of(const brt_ctx* ctx, const FrameParams& fp, uint32_t key[6]) {
    key[0] = fp.width; key[1] = fp.height; key[2] = fp.part; key[3] = fp.n_parts;
    key[4] = fp.strip_of ? ctx->strip_epoch : 0u;      // (another strip table: other strips, other costs)
    key[5] = fp.local_strips * fp.tiles_x;
}

// How far, in 8-pixel tiles, the picture has moved since the costs were measured: the angle between the two viewing directions
// and a translation as seen at the distance of the scene's centre, in pixels of this frame, plus one tile.
constexpr uint32_t kMaxDilate = 8;      // beyond this the old costs say nothing about the new view: a first frame again (pre-pass)
// how far, in pixels of this frame, the picture has moved between a remembered camera and this frame's (NaN-safe: "very far")
double camera_motion_px(const brt_ctx* ctx, const float* pos0, const float* dir0, const FrameParams& fp) {
    const float* a = dir0;
    const float* b = fp.cam_dir;
    const double la = std::sqrt((double)a[0] * a[0] + (double)a[1] * a[1] + (double)a[2] * a[2]);
    const double lb = std::sqrt((double)b[0] * b[0] + (double)b[1] * b[1] + (double)b[2] * b[2]);
    double c = ((double)a[0] * b[0] + (double)a[1] * b[1] + (double)a[2] * b[2]) / (la * lb);
    if (!(c == c)) return 1e30;
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    const double px_per_rad = 0.5 * (double)fp.height / (double)fp.tan_half_fov;
    double dp = 0.0, dist = 0.0;
    for (int k = 0; k < 3; k++) {
        dp += ((double)fp.cam_pos[k] - pos0[k]) * ((double)fp.cam_pos[k] - pos0[k]);
        dist += ((double)fp.cam_pos[k] - ctx->scene_centre[k]) * ((double)fp.cam_pos[k] - ctx->scene_centre[k]);
    }
    const double rot_px = std::acos(c) * px_per_rad, trans_px = std::sqrt(dp) / std::max(std::sqrt(dist), 1e-3) * px_per_rad;
    const double px = std::max(rot_px, trans_px);
    return px == px ? px : 1e30;
}
uint32_t dilation_tiles(const brt_ctx* ctx, const DeviceCtx& dc, const FrameParams& fp) {
    const double px = camera_motion_px(ctx, dc.cost_cam_pos, dc.cost_cam_dir, fp);
    if (!(px < 8.0 * kMaxDilate)) return kMaxDilate + 1u;
    return (uint32_t)std::ceil(px / 8.0) + 1u;
}
// the camera has moved further than the old costs can follow
bool camera_jumped(const brt_ctx* ctx, const DeviceCtx& dc, const FrameParams& fp) {
    return dc.costs_valid && camera_hash(fp) != dc.order_cam && dilation_tiles(ctx, dc, fp) > kMaxDilate;
}

// Tiles at the end of the order that are handed out as two half-sample jobs (brt_host.cpp build_tile_order): BRT_SPLIT_TAIL quarters of
// the wave slots (default 16: four tiles per wave slot), but at least half the launch's tiles.  The second halves must come up late
// enough behind the first ones to find their states: on the headline frame 0 / 4 / 8 / 12 / 16 / 24 / every non-sky tile give 9.49 /
// 9.53 / 9.40 / 9.33 / 9.21 / 9.28 / 9.25 ms -- with 8, 1 % of the second halves come too early, leave the pixel to its first-half
// lane, and those lanes are the new stragglers; and where the jobs are longer the gap must be wider: the 4K / 1024 spp frame (129 600
// tiles) 589 ms without, 596 with 16, 587 with 64 or all -- hence the half (profiles/r04/split_tail.txt).  The builders cap the number
// at the non-sky tiles that are not critical.  Only for launches of at least 6 tiles per wave slot, like the neighbourhood ranking: a rank's share
// of a frame split 2 or 4 ways has nothing to balance at its end.
uint32_t split_tail_of(const brt_ctx* ctx, const DeviceCtx& dc, uint32_t n_tiles) {
    const uint64_t wave_slots = (uint64_t)dc.num_cus * (BRT_BLOCK / 64u);
    if (ctx->knobs[K_SPLIT_FORCE] != 0u) return ctx->knobs[K_SPLIT_FORCE] < n_tiles ? ctx->knobs[K_SPLIT_FORCE] : n_tiles;   // (tests: that many tiles, whatever the frame)
    if ((uint64_t)n_tiles < 6u * wave_slots) return 0u;
    uint64_t r = (uint64_t)ctx->knobs[K_SPLIT_TAIL] * wave_slots / 4u;
    if (r != 0u && r < n_tiles / 2u) r = n_tiles / 2u;
    return (uint32_t)(r < n_tiles ? r : n_tiles);
}

// the order of brt_order.hip from the costs in d_tile_cost (measured at `spp` samples per pixel), on `stream`
int32_t build_order_on_device(brt_ctx* ctx, DeviceCtx& dc, uint32_t n_tiles, uint32_t tiles_x, uint32_t spp, uint32_t rx, uint32_t ry,
                              hipStream_t stream) {
    if (!dc.d_order_meta) HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&dc.d_order_meta), 256));
    int32_t rc = ensure(ctx, &dc.d_order_scratch, &dc.order_scratch_cap, order_scratch_bytes(n_tiles));
    if (rc != BRT_OK) return rc;
    const uint32_t split_tail = split_tail_of(ctx, dc, n_tiles);
    rc = ensure(ctx, &dc.d_tile_order, &dc.tile_order_cap, ((size_t)n_tiles + split_tail) * 4);
    if (rc != BRT_OK) return rc;
    const uint64_t sky_cost = (uint64_t)64 * spp * (1000 + ctx->knobs[K_LPT_SKY_SLACK]) / 1000;   // as build_tile_order
    HIP_TRY(ctx, launch_build_order(dc.d_tile_cost, dc.d_tile_cost + n_tiles, n_tiles, sky_cost, (uint64_t)dc.num_cus * BRT_BLOCK, tiles_x, rx,
                                    ry, split_tail, dc.d_tile_order, dc.d_order_meta, dc.d_order_scratch, stream));
    HIP_TRY(ctx, hipEventRecord(dc.ev_last, stream));   // a later launch on another stream starts behind the order build
    return BRT_OK;
}

// ---- pair records in the order of their use ------------------------------------------------------------------------------------
// A scene whose tree does not fit the LDS is walked from a tile of the first K records in LDS and the rest from L2 (SCENE_LDS_TOP).
// validate_and_encode numbers the records breadth first, so the tile is the top ~9.8 levels of the tree, everywhere in the scene; a
// view, though, walks a small part of the tree over and over: of the 10 004-sphere frame's interior visits the breadth-first tile
// of 879 records serves 78 %, the 879 records this view visits most would serve 98 % (3.7 -> 0.3 global steps per ray;
// profiles/r05/visit_hist_config5.txt), and the global steps are what the walk waits on (40 % of the wave cycles parked, the texture
// addresser 71 % busy: profiles/r05/config5_memory_side_before.json).  So the pre-pass of a first frame counts the visits per record
// (FrameParams::record_hits), and here the records are re-numbered by them, most visited first (ties: breadth-first order), the child
// descriptors and the root re-written, the records re-sent -- 1.1 MB and a host sort of 10 003 counts per pre-pass and device.
// The spheres are re-numbered with them (an internal numbering: nothing outside sees a sphere's index), see below.
// Only the NUMBERING of the records changes: the walk visits the same nodes in the same order, pixels and all five counters stay.
int32_t apply_hot_order(brt_ctx* ctx, DeviceCtx& dc, hipStream_t stream) {
    const uint32_t n = dc.view.n_pairs, m = dc.view.n_models;
    const EncodedScene& e = ctx->enc;
    if (n == 0u || e.pairs.size() != (size_t)n * PAIR_WORDS || e.spheres.size() != (size_t)m * 4u || e.sphere_material.size() != m || e.sphere_mats.size() != (size_t)m * 8u) return BRT_OK;
    // the records (and spheres) as they are on the device now: as encoded after an upload, else in the order of this device's last
    // pre-pass (the counts are indexed by THAT numbering)
    if (dc.hot_tree != ctx->tree_epoch) { dc.h_pairs_cur = e.pairs; dc.h_spheres_cur = e.spheres; dc.h_sphmat_cur = e.sphere_material; dc.h_sphmats_cur = e.sphere_mats; }
    const std::vector<float>& cur = dc.h_pairs_cur;
    const uint32_t cur_root = dc.hot_tree != ctx->tree_epoch ? e.root_desc : dc.view.root_desc;
    dc.h_hits.resize(n);
    HIP_TRY(ctx, hipMemcpyAsync(dc.h_hits.data(), dc.d_record_hits, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    std::vector<uint32_t>& rank = dc.h_rank;        // rank[old index] = new index
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return dc.h_hits[a] > dc.h_hits[b]; });
    rank.resize(n);
    uint32_t visited = 0;
    for (uint32_t i = 0; i < n; i++) { rank[order[i]] = i; visited += dc.h_hits[order[i]] != 0u ? 1u : 0u; }
    // the spheres likewise, by the visits of the record they hang under (a sphere is tested when its parent is visited and its box is
    // hit: the parent's count ranks it well enough -- the first 1 024 take 97 % of the 10 004-sphere frame's tests -- and needs no
    // second histogram): the leaf steps' sphere reads then fall on a few hot lines of the L1 (staging the first 512 / 1 024 / 2 048 of them
    // in LDS for the leaf step of the hand-written loop was built and measured: 13.88 / 13.97 / 14.2 ms against 13.92 without, not kept:
    // profiles/r05/config5_hot_records_ab.txt)
    using D = Desc<true>;
    constexpr uint32_t kDescWord = PAIR_DESC / 4u;
    std::vector<uint32_t> score(m, 0u), sorder(m), srank(m);
    auto leaf_sphere = [&](uint32_t d, uint32_t* id) {
        if ((int32_t)d < -1 && (d & D::LEAF1)) { *id = d & D::INDEX_MASK; return *id < m; }
        return false;
    };
    for (uint32_t r = 0; r < n; r++)
        for (uint32_t k = 0; k < 2u; k++) {
            uint32_t d, id;
            std::memcpy(&d, cur.data() + (size_t)r * PAIR_WORDS + kDescWord + k, 4);
            if (leaf_sphere(d, &id) && dc.h_hits[r] > score[id]) score[id] = dc.h_hits[r];
        }
    for (uint32_t i = 0; i < m; i++) sorder[i] = i;
    std::stable_sort(sorder.begin(), sorder.end(), [&](uint32_t a, uint32_t b) { return score[a] > score[b]; });
    for (uint32_t i = 0; i < m; i++) srank[sorder[i]] = i;
    std::vector<float> sph, mats;
    std::vector<uint32_t> mat;
    uint32_t new_root = 0;
    permute_scene(cur, dc.h_spheres_cur, dc.h_sphmat_cur, dc.h_sphmats_cur, cur_root, rank, srank, &dc.h_pairs_hot, &sph, &mat, &mats, &new_root);
    HIP_TRY(ctx, hipEventSynchronize(dc.ev_q));        // (a ray query on another stream may still be walking the old numbering)
    dc.hot_serial++;
    HIP_TRY(ctx, hipMemcpyAsync(const_cast<float*>(dc.view.pairs), dc.h_pairs_hot.data(), dc.h_pairs_hot.size() * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(ctx, hipMemcpyAsync(const_cast<float*>(dc.view.spheres), sph.data(), sph.size() * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(ctx, hipMemcpyAsync(const_cast<uint32_t*>(dc.view.sphere_material), mat.data(), mat.size() * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(ctx, hipMemcpyAsync(const_cast<float*>(dc.view.sphere_mats), mats.data(), mats.size() * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));       // (the vectors are reused by the next call)
    // the numbering as a map from the ENCODER's numbering (what the next upload of a tree of the same shape starts from): composed with
    // the one the counts were indexed by
    if (dc.hot_tree == ctx->tree_epoch && dc.h_total_rank.size() == n && dc.h_total_srank.size() == m) {
        for (uint32_t i = 0; i < n; i++) dc.h_total_rank[i] = rank[dc.h_total_rank[i]];
        for (uint32_t i = 0; i < m; i++) dc.h_total_srank[i] = srank[dc.h_total_srank[i]];
    } else {
        dc.h_total_rank = rank;
        dc.h_total_srank = srank;
    }
    dc.hot_shape = tree_shape_hash(e);
    dc.h_pairs_cur.swap(dc.h_pairs_hot);
    dc.h_spheres_cur.swap(sph);
    dc.h_sphmat_cur.swap(mat);
    dc.h_sphmats_cur.swap(mats);
    dc.view.root_desc = new_root;
    dc.hot_tree = ctx->tree_epoch;
    dc.hot_records = visited;
    return BRT_OK;
}

}  // namespace

namespace brt {

void view_key_of(const brt_ctx* ctx, const FrameParams& fp, uint32_t key[8]) {
    order_key_of(ctx, fp, key);
    key[6] = fp.sample_count; key[7] = fp.bounce_count;
}

// before the launch: attach the order table if the history matches this view, and -- when the
// history is missing, the camera has moved or a scene upload asks for it -- the (zeroed) cost buffer to measure again
int32_t attach_tile_order(brt_ctx* ctx, DeviceCtx& dc, FrameParams& fp, hipStream_t stream, bool may_measure, uint32_t flags) {
    fp.tile_order = nullptr;
    fp.tile_cost = nullptr;
    // (the bring-up kernel takes slot q = tile q / 64 of a plain order: an order with half-sample jobs -- n_tiles + n_split entries,
    //  [non-sky | second halves | sky] -- would have it render the split tiles twice and the last sky tiles never: raster order there)
    if (!lpt_enabled(ctx) || fp.level == 0u || (flags & BRT_FLAG_KERNEL_SIMPLE)) return BRT_OK;
    const uint32_t n_tiles = fp.local_strips * fp.tiles_x;
    uint32_t key[6];
    order_key_of(ctx, fp, key);
    const bool match = dc.order_valid && std::memcmp(key, dc.order_key, sizeof key) == 0;
    if (match && dc.costs_valid && dc.order_on_device && camera_hash(fp) != dc.order_cam && ctx->knobs[K_LPT_DILATE] != 0u) {
        // the camera has moved since the costs were measured (one frame ago, while it keeps moving): rank every tile by its
        // neighbourhood of the radius the motion covers.  Behind the previous frame's work, ahead of this frame's launch.
        uint32_t r = dilation_tiles(ctx, dc, fp);
        if (r <= kMaxDilate && ctx->knobs[K_LPT_DILATE] >= 2u && r < ctx->knobs[K_LPT_DILATE] - 1u &&
            (uint64_t)n_tiles >= 6u * (uint64_t)dc.num_cus * (BRT_BLOCK / 64u))
            r = ctx->knobs[K_LPT_DILATE] - 1u;
        if (r <= kMaxDilate) {
            HIP_TRY(ctx, hipStreamWaitEvent(stream, dc.ev_last, 0));
            const int32_t rc = build_order_on_device(ctx, dc, n_tiles, fp.tiles_x, dc.cost_spp, r, (r + fp.n_parts - 1u) / fp.n_parts, stream);
            if (rc != BRT_OK) return rc;
        }
    }
    if (match) {
        fp.tile_order = dc.d_tile_order;
        fp.queue_lane = dc.order_lane * 64u;
        fp.crit_begin = 0u;
        fp.crit_end = dc.order_crit * 64u;
        fp.order_meta = dc.order_on_device ? dc.d_order_meta : nullptr;   // then the kernel reads the critical count there
        // half-sample jobs at the end of the order: where they are (a GPU-built order says so in d_order_meta) and where the pixel
        // states wait between a tile's two jobs
        if (split_tail_of(ctx, dc, n_tiles) != 0u) {
            const size_t bytes = (size_t)fp.queue_size * 36u;       // three planes of 16 + 16 + 4 bytes per queue slot (brt_trace.h slice_slot)
            const bool fresh = bytes > dc.slice_state_cap;
            int32_t rc = ensure(ctx, &dc.d_slice_state, &dc.slice_state_cap, bytes);
            if (rc != BRT_OK) return rc;
            if (fresh || dc.slice_serial >= 0x3fffffffu) {      // flags of a new buffer (or after 2^30 launches: a flag holds serial << 2) must not look valid
                HIP_TRY(ctx, hipMemsetAsync(dc.d_slice_state, 0, dc.slice_state_cap, stream));
                dc.slice_serial = 0u;
            }
            fp.slice_state = dc.d_slice_state;
            fp.slice_serial = ++dc.slice_serial;
            if (!dc.order_on_device) { fp.split_nonsky = dc.order_nonsky; fp.split_tiles = dc.order_split; }
        }
    }
    bool due = !match || camera_hash(fp) != dc.order_cam || ctx->knobs[K_LPT_REFRESH_EVERY] == 1u;
    if (may_measure && match && dc.remeasure_in != 0u && --dc.remeasure_in == 0u) due = true;
    if (may_measure && due) {
        int32_t rc = ensure(ctx, &dc.d_tile_cost, &dc.tile_cost_cap, (size_t)n_tiles * 8);   // sums, then maxima
        if (rc != BRT_OK) return rc;
        HIP_TRY(ctx, hipMemsetAsync(dc.d_tile_cost, 0, (size_t)n_tiles * 8, stream));
        fp.tile_cost = dc.d_tile_cost;
    }
    return BRT_OK;
}

// after a measuring frame has been enqueued on `stream`: build the order of the next frames.  Default settings: on the
// GPU, on the same stream, no host round trip (brt_order.hip).  BRT_ORDER_ON_HOST=1, or any non-default ordering knob
// (BRT_LPT_SORT, BRT_LPT_SKY_SLACK, BRT_LPT_LANE_PERMILLE, BRT_CRIT): counts to the host, build_tile_order, order back up.
int32_t update_tile_order(brt_ctx* ctx, DeviceCtx& dc, const FrameParams& fp, hipStream_t stream) {
    if (!fp.tile_cost) return BRT_OK;
    const uint32_t n_tiles = fp.local_strips * fp.tiles_x;
    TileOrderParams tp{};
    tp.sample_count = fp.sample_count;
    tp.grid_lanes = (uint64_t)dc.num_cus * BRT_BLOCK;
    tp.sorted = ctx->knobs[K_LPT_SORT];
    tp.sky_slack_permille = ctx->knobs[K_LPT_SKY_SLACK];
    tp.lane_permille = ctx->knobs[K_LPT_LANE_PERMILLE];
    tp.critical = ctx->knobs[K_CRIT];
    tp.tiles_x = fp.tiles_x;
    tp.split_tail = split_tail_of(ctx, dc, n_tiles);
    int32_t rc = ensure(ctx, &dc.d_tile_order, &dc.tile_order_cap, ((size_t)n_tiles + tp.split_tail) * 4);
    if (rc != BRT_OK) return rc;
    const bool on_device = tp.sorted == 1u && tp.critical == 1u && tp.lane_permille == 0u && ctx->knobs[K_ORDER_ON_HOST] == 0u;
    dc.costs_valid = false;
    if (on_device) {
        // BRT_LPT_DILATE (default 3): 0 = every tile ranked by itself; 1 = by a neighbourhood only when the camera has moved since the
        // measurement (attach_tile_order); v >= 2 = a neighbourhood of radius at least v - 1 always.  Radius 2 is the default also for
        // the view the costs were measured in: same box A/B, config 2 10.88 -> 10.64 ms, config 3 68.4 -> 66.7, config 5 25.4 -> 24.3
        // (profiles/r04/static_dilate_configs.txt) -- expensive pixels come in clusters (glass and metal silhouettes), and handing out
        // a cluster's tiles together starts all of its long chains early instead of ranking each tile on one noisy maximum.
        // Only for launches of at least 6 tiles per wave slot: a rank's share of a frame split 2 or 4 ways hands every wave 2-4 tiles, there
        // the truly longest tiles must be in the first hand-out and neighbours ranked up beside them push some of them into the second
        // (slowest share of config 2 in 2 / 4 parts 6.24 / 5.13 ms without, 6.60 / 5.31 with; profiles/r04/parts_dilate.txt).
        const uint64_t wave_slots = (uint64_t)dc.num_cus * (BRT_BLOCK / 64u);
        const uint32_t r0 = (ctx->knobs[K_LPT_DILATE] >= 2u && (uint64_t)n_tiles >= 6u * wave_slots) ? ctx->knobs[K_LPT_DILATE] - 1u : 0u;
        // (the same radius for the costs of a first frame's pre-pass: radius 0 / 1 / 2 / 3 / 4 / 6 there gave 11.2 / 11.6 / 11.6 / 12.0 /
        //  12.5 / 13.2 ms for pre-pass + frame, profiles/r04/first_frame_prepass.txt)
        tp.dilate_x = r0;
        tp.dilate_y = r0 ? (r0 + fp.n_parts - 1u) / fp.n_parts : 0u;
        rc = build_order_on_device(ctx, dc, n_tiles, fp.tiles_x, tp.sample_count, tp.dilate_x, tp.dilate_y, stream);
        if (rc != BRT_OK) return rc;
        dc.order_lane = 0;
        dc.order_crit = 0;
        dc.order_on_device = true;
        dc.costs_valid = true;
        dc.cost_spp = tp.sample_count;
        for (int k = 0; k < 3; k++) { dc.cost_cam_pos[k] = fp.cam_pos[k]; dc.cost_cam_dir[k] = fp.cam_dir[k]; }
    } else {
        dc.h_cost.resize(2 * (size_t)n_tiles);
        HIP_TRY(ctx, hipMemcpyAsync(dc.h_cost.data(), dc.d_tile_cost, (size_t)n_tiles * 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(ctx, hipStreamSynchronize(stream));
        TileOrder to;
        build_tile_order(dc.h_cost.data(), dc.h_cost.data() + n_tiles, n_tiles, tp, &to);   // sums, then longest pixels (brt_host.cpp)
        dc.h_order.swap(to.order);
        dc.order_lane = to.n_lane;
        dc.order_crit = to.n_critical;
        dc.order_on_device = false;
        dc.order_nonsky = to.n_nonsky;
        dc.order_split = to.n_split;
        HIP_TRY(ctx, hipMemcpyAsync(dc.d_tile_order, dc.h_order.data(), dc.h_order.size() * 4, hipMemcpyHostToDevice, stream));
        HIP_TRY(ctx, hipStreamSynchronize(stream));   // h_order may be reused by the next call
    }
    order_key_of(ctx, fp, dc.order_key);
    dc.order_valid = true;
    dc.remeasure_in = 0;
    dc.order_cam = camera_hash(fp);
    return BRT_OK;
}

// the shape of the encoded tree: both child descriptors of every record, in the encoder's (breadth-first) numbering.  Two uploads with
// the same hash have the same records in the same places holding the same spheres -- only boxes and centres may have moved
uint64_t tree_shape_hash(const EncodedScene& e) {
    uint64_t h = 1469598103934665603ull ^ ((uint64_t)e.n_pairs << 32) ^ e.n_models;
    constexpr uint32_t kDescWord = PAIR_DESC / 4u;
    for (uint32_t r = 0; r < e.n_pairs; r++)
        for (uint32_t k = 0; k < 2u; k++) {
            uint32_t d;
            std::memcpy(&d, e.pairs.data() + (size_t)r * PAIR_WORDS + kDescWord + k, 4);
            h = (h ^ d) * 1099511628211ull;
        }
    return h | 1ull;
}

// records and spheres of `e` in the numbering rank / srank (old index -> new index) into the four host arrays; the root's descriptor
void permute_scene(const std::vector<float>& pairs, const std::vector<float>& spheres, const std::vector<uint32_t>& sphmat,
                   const std::vector<float>& sphmats, uint32_t root, const std::vector<uint32_t>& rank, const std::vector<uint32_t>& srank,
                   std::vector<float>* out_pairs, std::vector<float>* out_spheres, std::vector<uint32_t>* out_sphmat,
                   std::vector<float>* out_sphmats, uint32_t* out_root) {
    using D = Desc<true>;
    constexpr uint32_t kDescWord = PAIR_DESC / 4u;
    const uint32_t n = (uint32_t)rank.size(), m = (uint32_t)srank.size();
    auto remap = [&](uint32_t d) {
        if ((int32_t)d >= 0 && d < n) return rank[d];                                                  // interior (16-bit form: the record's index)
        if ((int32_t)d < -1 && (d & D::LEAF1) && (d & D::INDEX_MASK) < m) return (d & ~D::INDEX_MASK) | srank[d & D::INDEX_MASK];   // single-sphere leaf
        return d;
    };
    out_pairs->resize(pairs.size());
    for (uint32_t i = 0; i < n; i++) {
        const float* src = pairs.data() + (size_t)i * PAIR_WORDS;
        float* dst = out_pairs->data() + (size_t)rank[i] * PAIR_WORDS;
        std::memcpy(dst, src, PAIR_BYTES);
        for (uint32_t k = 0; k < 2u; k++) {
            uint32_t d;
            std::memcpy(&d, src + kDescWord + k, 4);
            d = remap(d);
            std::memcpy(dst + kDescWord + k, &d, 4);
        }
    }
    out_spheres->resize(spheres.size());
    out_sphmats->resize(sphmats.size());
    out_sphmat->resize(m);
    for (uint32_t i = 0; i < m; i++) {
        std::memcpy(out_spheres->data() + (size_t)srank[i] * 4, spheres.data() + (size_t)i * 4, 16);
        std::memcpy(out_sphmats->data() + (size_t)srank[i] * 8, sphmats.data() + (size_t)i * 8, 32);
        (*out_sphmat)[srank[i]] = sphmat[i];
    }
    *out_root = remap(root);
}

// The first frame of a view has no measured dispatch order (raster order: 12.9 instead of 9.6 ms on the headline
// frame).  A pre-pass of the same view at a few samples per pixel measures the tile costs first -- pixels are sequential
// chains of samples, so k samples predict the chain lengths of the full frame -- and the frame itself then runs in that
// order (and measures again, for the frames that follow).  k = min(BRT_PREPASS_SPP, samples / 16): default 4, 0 = off;
// measured on the headline frame (pre-pass + frame, ms): none 12.9, k = 1 14.2 (worse than raster order: one sample ranks
// the wrong tiles first), 2 11.5, 3 11.3, 4 11.0, 5 11.2, 6 11.3, 8 11.7 (profiles/r04/first_frame_prepass.txt) -- so no
// pre-pass where the rule would leave k = 1.  Enqueued on the context's own stream ahead of the frame (the order is built
// on the GPU behind it: no host round trip); only on the entry points that own their stream.  The pre-pass renders into
// the frame's own tile buffer; the frame overwrites every pixel of it afterwards.
int32_t prepass_order(brt_ctx* ctx, DeviceCtx& dc, const FrameParams& fp, const float* d_raster_rgba,
                      const float* d_raster_depth, float* d_out_tile, hipStream_t stream, uint32_t flags, bool* ran) {
    *ran = false;
    const uint32_t knob = ctx->knobs[K_PREPASS_SPP];
    const uint32_t k = knob < fp.sample_count / 16u ? knob : fp.sample_count / 16u;
    if (k == 0u || (k == 1u && knob != 1u) || !lpt_enabled(ctx) || fp.level == 0u || (flags & BRT_FLAG_KERNEL_SIMPLE)) return BRT_OK;
    uint32_t key[6];
    order_key_of(ctx, fp, key);
    // the records of a scene walked from an LDS tile were numbered for another view: once the picture has moved a quarter of the
    // frame's height since they were counted (a tile that holds another view's records serves fewer visits than the breadth-first one
    // would), this frame is a first frame again -- a pre-pass of ~2 ms every dozen frames of a steady orbit
    bool hot_stale = ctx->knobs[K_HOT_RECORDS] != 0u && dc.hot_tree == ctx->tree_epoch && dc.hot_records != 0u &&
                     camera_motion_px(ctx, dc.hot_cam_pos, dc.hot_cam_dir, fp) > std::max(64.0, 0.25 * (double)fp.height);
    // ... or were never numbered for this tree although the scene has stood still for two frames (an upload of a scene with the same
    // number of spheres keeps the dispatch order and runs no pre-pass -- right for a scene that is re-uploaded every frame, whose
    // tree changes under any count; a scene that then stays gets its records counted on its second frame)
    if (dc.frames_since_upload < 1000u) dc.frames_since_upload++;
    if (!hot_stale && ctx->knobs[K_HOT_RECORDS] != 0u && dc.hot_tree != ctx->tree_epoch && dc.frames_since_upload == 2u && dc.view.desc16 &&
        dc.view.simple_tree && dc.view.n_pairs > 64u && plan_launch(ctx->knobs, dc, fp).scene_mode == SCENE_LDS_TOP)
        hot_stale = true;
    // history matches and the camera has not jumped out of its reach: nothing to do
    if (dc.order_valid && std::memcmp(key, dc.order_key, sizeof key) == 0 && !(ctx->knobs[K_LPT_DILATE] != 0u && camera_jumped(ctx, dc, fp)) && !hot_stale)
        return BRT_OK;
    FrameParams pp = fp;
    pp.sample_count = k;
    pp.spp_f = (float)k;
    pp.tile_order = nullptr;
    pp.order_meta = nullptr;
    pp.slice_state = nullptr;     // (raster order: nothing is split)
    pp.split_nonsky = pp.split_tiles = 0u;
    pp.tunable = 1u;   // the knobs-live instantiation (all knobs at their defaults): the pre-pass then shows up under its own
                       // kernel name in rocprofv3 --stats instead of pulling down the average of the frame kernel
    pp.queue_lane = 0u;
    pp.crit_begin = pp.crit_end = 0u;
    const uint32_t n_tiles = pp.local_strips * pp.tiles_x;
    int32_t rc = ensure(ctx, &dc.d_tile_cost, &dc.tile_cost_cap, (size_t)n_tiles * 8);
    if (rc != BRT_OK) return rc;
    HIP_TRY(ctx, hipMemsetAsync(dc.d_tile_cost, 0, (size_t)n_tiles * 8, stream));
    pp.tile_cost = dc.d_tile_cost;
    // a scene that is walked from the LDS tile + global memory: the pre-pass also counts the interior visits per pair record, and the
    // records are then re-numbered by them (apply_hot_order): every pre-pass does (first frame of a view, camera jump)
    bool count_hits = false;
    if (ctx->knobs[K_HOT_RECORDS] != 0u && dc.view.desc16 && dc.view.simple_tree && dc.view.n_pairs > 64u &&
        plan_launch(ctx->knobs, dc, pp).scene_mode == SCENE_LDS_TOP) {
        rc = ensure(ctx, &dc.d_record_hits, &dc.record_hits_cap, (size_t)dc.view.n_pairs * 4);
        if (rc != BRT_OK) return rc;
        HIP_TRY(ctx, hipMemsetAsync(dc.d_record_hits, 0, (size_t)dc.view.n_pairs * 4, stream));
        pp.record_hits = dc.d_record_hits;
        count_hits = plan_launch(ctx->knobs, dc, pp).scene_mode == SCENE_LDS_TOP;      // (the histogram must leave room for a tile)
        if (!count_hits) pp.record_hits = nullptr;
    }
    HIP_TRY(ctx, hipEventRecord(dc.ev_p0, stream));
    rc = launch_part(ctx, dc, pp, d_raster_rgba, d_raster_depth, d_out_tile, stream, flags & ~(uint32_t)BRT_FLAG_COUNTERS, false, nullptr);
    if (rc != BRT_OK) return rc;
    HIP_TRY(ctx, hipEventRecord(dc.ev_p1, stream));
    rc = update_tile_order(ctx, dc, pp, stream);      // on the GPU, behind the pre-pass, no host round trip (default settings)
    if (rc != BRT_OK) return rc;
    if (count_hits) {
        rc = apply_hot_order(ctx, dc, stream);
        if (rc != BRT_OK) return rc;
        for (int q = 0; q < 3; q++) { dc.hot_cam_pos[q] = fp.cam_pos[q]; dc.hot_cam_dir[q] = fp.cam_dir[q]; }
    }
    dc.remeasure_in = 1u;                             // the frame that follows measures again, at full sample count
    *ran = true;
    return BRT_OK;
}

// ---- strip table (brt_set_strip_table) ------------------------------------------------------------------------------
// Strips go to parts by `s mod N` unless the caller sets a table.  A table permutes the parts INSIDE every group of N consecutive strips,
// so a part still has exactly one strip per group: its k-th local strip lies in group k, tiles keep their size and layout, the ONE gather
// stays as it is, and only two lookups change -- the kernel's "local strip -> frame strip" (FrameParams::strip_of) and the assembly's
// "frame strip -> part" (k_deinterleave).  Pixels cannot change: a pixel's seed depends on its frame coordinates (raytrace.wgsl:95).
// brt_plan_strips makes such a table from measured costs: the frame is rendered once at a few samples per pixel on THIS device with the
// per-tile ray counts switched on, and the strips of every group are dealt out, dearest strip to the part with the least so far.  Every
// rank computes the same table from the same integers (the kernel is deterministic), so no second collective is needed.
bool strip_table_valid(const uint32_t* t, uint32_t n_strips, uint32_t n_parts) {
    if (n_parts == 0u || n_parts > 64u) return false;
    for (uint32_t g = 0; g * n_parts < n_strips; g++) {
        uint64_t seen = 0;
        for (uint32_t s = g * n_parts; s < n_strips && s < (g + 1u) * n_parts; s++) {
            if (t[s] >= n_parts || (seen >> t[s]) & 1ull) return false;
            seen |= 1ull << t[s];
        }
    }
    return true;
}
// The device copy of the table on dc, made once per table for every part, so that a call for another part rewrites nothing.  A new
// table is written on `stream` behind every call that may still read the old one -- kernels (ev_last) and assemblies (ev_strip_read)
// on any stream -- and every reader on another stream starts behind the write (ev_strip): a call uses the table in force when it is
// called.  No host synchronisation while the table is unchanged.
int32_t strip_table_attach(brt_ctx* ctx, DeviceCtx& dc, FrameParams* fp, const uint32_t** part_of_strip, hipStream_t stream) {
    if (part_of_strip) *part_of_strip = nullptr;
    const uint32_t strips = (fp->height + BRT_STRIP_ROWS - 1u) / BRT_STRIP_ROWS, n_parts = fp->n_parts;
    if (ctx->strip_part.empty() || ctx->strip_n_parts != n_parts || ctx->strip_part.size() != strips || n_parts < 2u) return BRT_OK;
    const uint32_t local = (strips + n_parts - 1u) / n_parts;
    if (dc.strip_epoch != ctx->strip_epoch || !dc.d_strip_table) {
        const size_t words = (size_t)strips + (size_t)n_parts * local;
        HIP_TRY(ctx, hipEventSynchronize(dc.ev_strip));                      // the previous upload has read h_strip_table (a new table only)
        if (dc.strip_table_cap < words * 4u)                                 // a larger buffer: the old one goes once nothing reads it
            for (hipEvent_t e : {dc.ev_last, dc.ev_strip_read}) HIP_TRY(ctx, hipEventSynchronize(e));
        int32_t rc = ensure(ctx, &dc.d_strip_table, &dc.strip_table_cap, words * 4u);
        if (rc != BRT_OK) return rc;
        std::vector<uint32_t>& h = dc.h_strip_table;
        h.assign(words, 0xffffffu);                                          // strip_of: a group without a strip of the part: padding
        std::copy(ctx->strip_part.begin(), ctx->strip_part.end(), h.begin());
        for (uint32_t s = 0; s < strips; s++) h[(size_t)strips + (size_t)ctx->strip_part[s] * local + s / n_parts] = s;
        HIP_TRY(ctx, hipStreamWaitEvent(stream, dc.ev_last, 0));
        HIP_TRY(ctx, hipStreamWaitEvent(stream, dc.ev_strip_read, 0));
        HIP_TRY(ctx, hipMemcpyAsync(dc.d_strip_table, h.data(), words * 4u, hipMemcpyHostToDevice, stream));
        HIP_TRY(ctx, hipEventRecord(dc.ev_strip, stream));
        dc.strip_epoch = ctx->strip_epoch;
    } else {
        HIP_TRY(ctx, hipStreamWaitEvent(stream, dc.ev_strip, 0));           // (written on another stream, perhaps not yet)
    }
    const uint32_t* d = reinterpret_cast<const uint32_t*>(dc.d_strip_table);
    if (part_of_strip) *part_of_strip = d;
    fp->strip_of = d + strips + (size_t)fp->part * local;
    return BRT_OK;
}
// behind an assembly on `stream` that read the table: ev_strip_read then marks the end of it and of every assembly before it
int32_t strip_table_read(brt_ctx* ctx, DeviceCtx& dc, const uint32_t* part_of_strip, hipStream_t stream) {
    if (!part_of_strip) return BRT_OK;
    HIP_TRY(ctx, hipStreamWaitEvent(stream, dc.ev_strip_read, 0));
    HIP_TRY(ctx, hipEventRecord(dc.ev_strip_read, stream));
    return BRT_OK;
}
uint64_t part_pixels_table(const brt_ctx* ctx, const FrameParams& fp) {
    uint64_t rows = 0;
    for (uint32_t s = 0; s < (uint32_t)ctx->strip_part.size(); s++)
        if (ctx->strip_part[s] == fp.part) {
            const uint32_t r0 = s * BRT_STRIP_ROWS;
            rows += (r0 + BRT_STRIP_ROWS <= fp.height) ? BRT_STRIP_ROWS : (fp.height - r0);
        }
    return rows * fp.width;
}

}  // namespace brt

extern "C" {

uint32_t brt_tile_rows(uint32_t height, uint32_t n_parts) {
    if (n_parts == 0) return 0;
    const uint32_t strips = (height + BRT_STRIP_ROWS - 1u) / BRT_STRIP_ROWS;
    return ((strips + n_parts - 1u) / n_parts) * BRT_STRIP_ROWS;
}

int32_t brt_set_strip_table(brt_ctx* ctx, uint32_t n_parts, uint32_t n_strips, const uint32_t* part_of_strip) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (!part_of_strip) { ctx->strip_epoch++; ctx->strip_part.clear(); ctx->strip_n_parts = 0u; return BRT_OK; }
    // (a refused table changes nothing: the table in force stays)
    if (n_parts < 1u || n_strips < 1u || n_strips > 4096u) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "n_parts / n_strips out of range");
    if (!strip_table_valid(part_of_strip, n_strips, n_parts))
        return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "strip table: every group of n_parts consecutive strips must hold each part at most once");
    ctx->strip_epoch++;
    ctx->strip_part.assign(part_of_strip, part_of_strip + n_strips);
    ctx->strip_n_parts = n_parts;
    return BRT_OK;
    });
}

int32_t brt_plan_strips(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t level, uint32_t width, uint32_t height,
                        uint32_t n_parts, uint32_t probe_spp, uint32_t* out_part_of_strip) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (!ctx->has_scene) return ctx_fail(ctx, BRT_ERR_NO_SCENE, "no scene uploaded");
    if (n_parts < 1u || n_parts > 64u || probe_spp < 1u) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "n_parts must be 1..64, probe_spp >= 1");
    FrameParams fp;
    int32_t rc = make_frame_params(ctx, camera80, window16, level == 0u ? 3u : level, width, height, 0u, 1u, &fp);
    if (rc != BRT_OK) return rc;
    fp.sample_count = probe_spp;
    fp.spp_f = (float)probe_spp;
    DeviceCtx& dc = ctx->devs[0];
    HIP_TRY(ctx, hipSetDevice(dc.device));
    const uint32_t n_tiles = fp.local_strips * fp.tiles_x, strips = fp.local_strips;
    rc = ensure(ctx, &dc.d_tile, &dc.tile_cap, (size_t)strips * BRT_STRIP_ROWS * width * 16u);
    if (rc != BRT_OK) return rc;
    rc = ensure(ctx, &dc.d_tile_cost, &dc.tile_cost_cap, (size_t)n_tiles * 8u);
    if (rc != BRT_OK) return rc;
    HIP_TRY(ctx, hipStreamWaitEvent(dc.stream, dc.ev_last, 0));
    HIP_TRY(ctx, hipMemsetAsync(dc.d_tile_cost, 0, (size_t)n_tiles * 8u, dc.stream));
    fp.tile_cost = dc.d_tile_cost;                              // ray sums per tile (then maxima)
    rc = launch_part(ctx, dc, fp, nullptr, nullptr, dc.d_tile, dc.stream, 0u, false, nullptr);
    if (rc != BRT_OK) return rc;
    std::vector<uint32_t> cost(n_tiles);
    HIP_TRY(ctx, hipMemcpyAsync(cost.data(), dc.d_tile_cost, (size_t)n_tiles * 4u, hipMemcpyDeviceToHost, dc.stream));
    HIP_TRY(ctx, hipStreamSynchronize(dc.stream));
    dc.costs_valid = false;                                     // (the cost buffer no longer holds a view's measurement)
    std::vector<uint64_t> strip_cost(strips, 0);
    for (uint32_t t = 0; t < n_tiles; t++) strip_cost[t / fp.tiles_x] += cost[t];
    std::vector<uint32_t> table(strips, 0u);
    plan_strip_table(strip_cost.data(), strips, n_parts, table.data());          // the rule: brt_host.cpp
    if (out_part_of_strip) std::memcpy(out_part_of_strip, table.data(), (size_t)strips * 4u);
    ctx->strip_epoch++;
    ctx->strip_part = table;
    ctx->strip_n_parts = n_parts;
    return BRT_OK;
    });
}

int32_t brt_debug_tile_order(brt_ctx* ctx, const uint32_t* ray_sum, const uint32_t* longest_pixel, uint32_t n_tiles,
                             uint32_t sample_count, uint64_t grid_lanes, uint32_t tiles_x, uint32_t dilate, uint32_t split_tail,
                             uint32_t* out_order, uint32_t* out_info4) {
    return ctx_guard(ctx, [&]() -> int32_t {
    if (!ray_sum || !longest_pixel || !out_order || !out_info4 || n_tiles == 0) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "null buffer / no tiles");
    if (dilate != 0u && (tiles_x == 0u || n_tiles % tiles_x != 0u)) return ctx_fail(ctx, BRT_ERR_INVALID_ARGUMENT, "dilate needs a tiles_x that divides n_tiles");
    DeviceCtx& dc = ctx->devs[0];
    HIP_TRY(ctx, hipSetDevice(dc.device));
    uint32_t* d_cost = nullptr;
    uint32_t* d_order = nullptr;
    uint32_t* d_meta = nullptr;
    char* d_scratch = nullptr;
    auto body = [&]() -> int32_t {
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&d_cost), (size_t)n_tiles * 8));
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&d_order), ((size_t)n_tiles + split_tail) * 4));
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&d_meta), 256));
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&d_scratch), order_scratch_bytes(n_tiles)));
        HIP_TRY(ctx, hipMemcpyAsync(d_cost, ray_sum, (size_t)n_tiles * 4, hipMemcpyHostToDevice, dc.stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_cost + n_tiles, longest_pixel, (size_t)n_tiles * 4, hipMemcpyHostToDevice, dc.stream));
        const uint64_t sky_cost = (uint64_t)64 * sample_count * (1000 + 20) / 1000;
        HIP_TRY(ctx, launch_build_order(d_cost, d_cost + n_tiles, n_tiles, sky_cost, grid_lanes, tiles_x, dilate, dilate, split_tail, d_order, d_meta, d_scratch, dc.stream));
        HIP_TRY(ctx, hipMemcpyAsync(out_info4, d_meta, 16, hipMemcpyDeviceToHost, dc.stream));
        HIP_TRY(ctx, hipStreamSynchronize(dc.stream));
        HIP_TRY(ctx, hipMemcpy(out_order, d_order, ((size_t)n_tiles + out_info4[3]) * 4, hipMemcpyDeviceToHost));
        return BRT_OK;
    };
    const int32_t rc = body();
    if (d_cost) (void)hipFree(d_cost);
    if (d_order) (void)hipFree(d_order);
    if (d_meta) (void)hipFree(d_meta);
    if (d_scratch) (void)hipFree(d_scratch);
    return rc;
    });
}

}  // extern "C"
