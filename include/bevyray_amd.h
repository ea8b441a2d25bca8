/*
 * bevyray_amd.h -- C ABI of the MI355X path-tracing render node.
 *
 * This is the drop-in boundary for ONE path of GrandmasterB42/bevyray: the wgpu
 * fragment pass that `RayTracingNode::run` encodes
 * (reference src/raytracing/pipeline.rs:58-220) together with the per-pixel ray
 * loop it dispatches (reference assets/shaders/raytrace.wgsl:93-421,
 * random.wgsl:3-30, const.wgsl:1-2).  The Rust node keeps its registration,
 * ViewQuery and extract stage; the body of `run` calls these functions instead
 * of `write_buffer` x3 + bind groups + `draw(0..3, 0..1)`.  INTEGRATION.md shows
 * the Rust `extern "C"` block and the replacement body.
 *
 * Conventions
 *   - Every function returns int32: BRT_OK (0) or a negative BRT_ERR_* code; none
 *     throws or aborts across the boundary (every export body runs inside an exception
 *     barrier: a failed host allocation is BRT_ERR_OUT_OF_MEMORY, anything else
 *     BRT_ERR_INTERNAL).  brt_last_error() gives the text.
 *     (Reference: every "not ready" condition returns Ok(()) and skips the pass,
 *     pipeline.rs:82-85,89-102,113-115,141-151; the Rust side maps non-zero to a
 *     logged warning + Ok(()).)
 *   - The caller owns every pointer it passes; the callee copies during the call
 *     and retains nothing.  All device memory lives in the opaque context.
 *   - A context is single-caller (not re-entrant), like a render-graph node that
 *     the runner executes sequentially.
 *   - Wire formats are the encase/WGSL layouts the reference's extract stage
 *     already produces (extract.rs:56-61, 83-104, 181-189, 213-218, 229-237):
 *       Model            32 B  position vec3 @0, radius f32 @12, material_id u32 @16
 *       RaytraceMaterial 32 B  base_color vec3 @0, metallic @12, roughness @16,
 *                              reflectance @20, ior @24, specular_transmission @28
 *       BVHNode          48 B  bounds_min vec3 @0, bounds_max vec3 @16, index u32 @28,
 *                              model_count u32 @32
 *       CameraExtract    80 B  sample_count u32 @0, bounce_count @4, projection @8,
 *                              near f32 @12, far @16, fov @20, aspect @24,
 *                              position vec3 @32, direction vec3 @48, up vec3 @64
 *       WindowExtract    16 B  random_seed f32 @0, height u32 @4
 *   - Frames are RGBA f32, row-major, top row first, width*height*16 bytes (device frames optionally in the colour
 *     target's own format: BRT_FLAG_OUT_*).
 */
#ifndef BEVYRAY_AMD_H
#define BEVYRAY_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BRT_ABI_VERSION 6u

/* Rows per strip of the interleaved row tiling. */
#define BRT_STRIP_ROWS 8u

enum {
    BRT_OK = 0,
    BRT_ERR_INVALID_ARGUMENT = -1,
    BRT_ERR_NO_DEVICE = -2,        /* no HIP device / HIP runtime failure at create */
    BRT_ERR_HIP = -3,              /* a HIP call failed; text in brt_last_error */
    BRT_ERR_INVALID_BVH = -4,      /* node index out of range, cycle, leaf range out of range */
    BRT_ERR_INVALID_SCENE = -5,    /* material_id out of range (non-finite spheres are accepted, as in the reference) */
    BRT_ERR_EMPTY_SCENE = -6,      /* zero spheres: the reference skips the pass (pipeline.rs:141-151) */
    BRT_ERR_NO_SCENE = -7,         /* render before upload */
    BRT_ERR_UNSUPPORTED = -8,      /* e.g. orthographic projection (extract.rs:148) */
    BRT_ERR_CAPACITY = -9,         /* caller buffer too small */
    BRT_ERR_RCCL = -10,            /* librccl could not be loaded, or an RCCL call failed; text in brt_last_error */
    BRT_ERR_OUT_OF_MEMORY = -11,   /* a host allocation failed (std::bad_alloc caught at the boundary); the context stays usable */
    BRT_ERR_INTERNAL = -12         /* any other exception caught at the boundary; text in brt_last_error */
};

/* Raytracing level, reference src/raytracing/mod.rs:94-101 (#[repr(u32)]). */
enum {
    BRT_LEVEL_SKIP = 0,
    BRT_LEVEL_FALLBACK_RASTER = 1,
    BRT_LEVEL_FALLBACK_RAYTRACED = 2,
    BRT_LEVEL_PURE = 3
};

/* brt_render* flags */
enum {
    BRT_FLAG_COUNTERS = 1u,        /* also count node pops / interior visits / sphere tests / hits */
    BRT_FLAG_KERNEL_SIMPLE = 2u,   /* one-thread-per-pixel bring-up kernel instead of the persistent one */
    BRT_FLAG_CALLER_STREAM = 4u,   /* device entry points: `hip_stream` is the caller's stream even when it is NULL
                                      (NULL is then the legacy default stream, not "the context's own stream"):
                                      the work is enqueued there, ordered with whatever the caller enqueued before
                                      (e.g. an RCCL gather), and the call does not synchronise */
    /* Format of the assembled DEVICE frame (brt_render_device, brt_gather_rccl, brt_deinterleave_device): the reference's pass writes
     * into post_process.destination, whose format is TextureFormat::bevy_default() (pipeline.rs:311-315) -- an 8-bit sRGB target, or
     * Rgba16Float under HDR -- so with brt_import_frame_fd the frame can be stored where the next pass reads it, in that format.
     * The pass's result IS the RGBA f32 frame (parity is stated on it); the other formats are its store conversion, exactly:
     *   RGBA8_UNORM_SRGB  r, g, b: round(255 * OETF(clamp(c, 0, 1))), OETF the sRGB encode (12.92 c below 0.0031308, else
     *                     1.055 c^(1/2.4) - 0.055), evaluated exactly (as the number of decision thresholds <= c, see
     *                     bevyray_amd/csrc/brt_srgb_table.h); alpha: the RGBA8_UNORM rule.  NaN stores 0.  4 bytes per pixel, r first.
     *   RGBA8_UNORM       round-half-even(255 * clamp(c, 0, 1)), exact.  4 bytes per pixel.
     *   RGBA16F           f32 -> f16, round to nearest even.  8 bytes per pixel.
     * brt_render / brt_render_part_device always write RGBA f32 (host frame / a rank's tile: the tiles travel as f32). */
    BRT_FLAG_OUT_RGBA32F = 0u,
    BRT_FLAG_OUT_RGBA8_UNORM_SRGB = 8u,
    BRT_FLAG_OUT_RGBA16F = 16u,
    BRT_FLAG_OUT_RGBA8_UNORM = 24u,
    BRT_FLAG_OUT_MASK = 24u,
    /* brt_render / brt_render_device: the frame is traced exactly as without the flag (RGBA f32), then the context's denoiser
     * (brt_set_denoise) runs on the assembled frame on the first device and its result is what is written, in the requested format.
     * Level 3 (Pure) only: BRT_ERR_UNSUPPORTED at levels 0-2 (the raster blend of levels 1 / 2 leaves no mark of the pixels that took
     * the raster colour) and on brt_render_part_device / brt_gather_rccl / brt_deinterleave_device (a rank's strips have no
     * neighbours: denoise the assembled frame with brt_denoise_device).  The denoiser's time is part of brt_stats::total_ms only.
     * Levels 1 / 2 take the flag together with BRT_FLAG_BLEND_POST (below). */
    BRT_FLAG_DENOISE = 32u,
    /* brt_render / brt_render_device / brt_denoise_device: the frame is traced exactly as without the flag, then accumulated into the
     * context's temporal history (brt_set_temporal) on the first device: reprojected through the camera and sphere motion, blended with
     * alpha = 1 / n.  Alone: the accumulated frame is written.  With BRT_FLAG_DENOISE: the denoiser filters the accumulation.  A frame
     * with an empty history is bit-identical to the same frame without the flag.  Same restrictions as BRT_FLAG_DENOISE (level 3; not on
     * brt_render_part_device / brt_gather_rccl / brt_deinterleave_device), and levels 1 / 2 with BRT_FLAG_BLEND_POST likewise. */
    BRT_FLAG_TEMPORAL = 64u,
    /* brt_render / brt_render_device, together with BRT_FLAG_DENOISE and / or BRT_FLAG_TEMPORAL: the post-passes on a level-1 / level-2
     * frame.  The frame is traced with the caller's raster depth and WITHOUT the raster colour, which makes it a coverage frame: alpha
     * 1 and the ray-traced colour where the pixel is ray-traced, all four channels +0.0 where the raster wins.  The post-passes run on
     * the ray-traced pixels; a covered pixel passes through them like a sky pixel (never a tap of another pixel, no temporal history:
     * n = 0, x' = y' = NaN) and is written as the raster_rgba texel of its own index, all four channels (NULL: zeros), in the requested
     * BRT_FLAG_OUT_* format.  With an empty history BRT_FLAG_BLEND_POST | BRT_FLAG_TEMPORAL is the level's plain frame bit for bit.
     * The raster colour is read on the first device only: an N-device context no longer forwards it, and brt_stats::forwarded_bytes
     * counts the depth alone.  Pure-level and blended temporal frames of one size share one history.  brt_render_device: the kernel that
     * stores d_frame reads d_raster_rgba, so with the flag the two must not overlap (without it the trace has consumed the colour
     * before anything is stored).
     * Without BRT_FLAG_DENOISE / BRT_FLAG_TEMPORAL: BRT_ERR_INVALID_ARGUMENT.  Level 0: BRT_ERR_UNSUPPORTED (nothing is ray-traced).
     * Level 3: ignored (Pure has no blend).  brt_render_part_device / brt_gather_rccl / brt_deinterleave_device:
     * BRT_ERR_UNSUPPORTED, as BRT_FLAG_DENOISE (the per-rank form is brt_blend_post_device). */
    BRT_FLAG_BLEND_POST = 128u
};

typedef struct brt_ctx brt_ctx;

/* Per-call statistics.  `rays` (one per raycast() call, raytrace.wgsl:190) is always
 * counted; the other four only with BRT_FLAG_COUNTERS (else 0). */
typedef struct brt_stats {
    uint64_t rays;
    uint64_t node_pops;        /* raytrace.wgsl:321-323 */
    uint64_t interior_visits;  /* raytrace.wgsl:327-341 */
    uint64_t sphere_tests;     /* raytrace.wgsl:350-352 */
    uint64_t hits;             /* scatter() calls, raytrace.wgsl:204 */
    uint64_t paths;            /* pixels * sample_count rendered by this call */
    double   kernel_ms;        /* HIP-event time of the trace kernel on its own stream (max over devices) */
    double   gather_ms;        /* tile copy-out / gather time */
    double   total_ms;         /* host wall time of the call */
    uint32_t lds_bytes;        /* dynamic LDS per workgroup of the trace kernel */
    uint32_t scene_in_lds;     /* 1: BVH + spheres LDS-resident; 2: the top levels of the BVH in LDS, the rest from L2; 0: all from L2 */
    uint32_t n_workgroups;
    uint32_t threads_per_workgroup;
    double   prepass_ms;       /* kernel time of the dispatch-order pre-pass that ran before this frame (first frame
                                  of a view on the synchronous paths; else 0).  Not part of kernel_ms. */
    uint32_t kernel_variant;   /* instantiation of the trace kernel that ran: 0 general, 1 / 2 the LEAN ones (Pure level; 2: no
                                  pixel chain can be critical), + 16: knobs live (a tuning knob off its default) */
    uint32_t measured_tile_costs; /* 1: this frame measured the per-tile ray counts for the dispatch order of the next ones
                                  (first frames of a view, every frame while the camera moves, after scene uploads) */
    uint32_t tree_rebuilt;     /* 1: the callee-built tree was rebuilt for this call's camera before the launch (see brt_upload_scene) */
    float    tree_reach;       /* the `reach` the resident callee-built SAH tree was built with (what brt_build_bvh_sah takes: 0 = the
                                  scene's own extent); 0 for a caller's tree */
    uint64_t forwarded_bytes;  /* brt_render_device: bytes of the raster inputs forwarded to the other devices of the context
                                  (BRT_FLAG_BLEND_POST: the depth alone) */
    uint32_t hot_records;      /* a scene walked from an LDS tile + L2 (scene_in_lds == 2): the tree's records are numbered by how often this
                                  view visits them (measured by the pre-pass of a first frame), so that the tile holds the ones the walk
                                  uses; this many of them were visited at all.  0: breadth-first numbering (no pre-pass yet / another mode) */
    uint32_t reserved;         /* brt_render_pixels*, brt_render_lens_pixels*: list entries refused (they name no pixel of the frame); else 0 */
} brt_stats;

uint32_t brt_abi_version(void);

/* Text of the last error on this context (ctx may be NULL: last error of brt_create /
 * the host-only helpers on this thread).  The pointer stays valid until the next call. */
const char* brt_last_error(const brt_ctx* ctx);

/* Replaces: RaytracingPipeline::from_world (pipeline.rs:233-331) -- one-time GPU setup.
 * device_ids[n_devices] are HIP ordinals; the frame is row-tiled over them in strips of
 * BRT_STRIP_ROWS rows (strip s -> device s % n_devices).  An ordinal may repeat.
 * Threads: all state lives in the context; calls on ONE context must not overlap, different contexts may be driven from different
 * host threads at the same time (tests/test_parity_gpu.py::test_two_contexts_driven_from_two_host_threads). */
int32_t brt_create(const int32_t* device_ids, int32_t n_devices, brt_ctx** out_ctx);
int32_t brt_destroy(brt_ctx* ctx);

/* The readings of the shader that WGSL leaves to the implementation and that nothing in the reference pins (naga /
 * the driver decide them; no wgpu run is possible where this library was built).  They change pixels, so they are an API option,
 * not environment variables.  Default (flags = 0) is what the parity tests are stated on; each flag switches ONE reading to its
 * alternative (the frames run in the knobs-live instantiation of the kernel then), so that the day a real wgpu frame can be compared
 * (scripts/compare_wgpu_frame.py names the combination it matches) the product can follow it:
 *   BRT_POLICY_OR_SHORT_CIRCUIT  `if cannot_refract || reflectance(cos_theta, ri) > rngNextFloat(state)` (raytrace.wgsl:269): default =
 *                                both operands evaluated, the RNG draw always happens; flag = the WGSL-spec reading, no draw when
 *                                cannot_refract.  Differs only for glass with ior < 1.
 *   BRT_POLICY_MINMAX_SELECT     min / max (raytrace.wgsl:391-394, :263, :405): default = IEEE minNum / maxNum (a NaN operand yields the
 *                                other one); flag = compare-select, min(a, b) = b < a ? b : a, max(a, b) = a < b ? b : a.  Differs
 *                                only when a bound or a ray component is a NaN.
 *   BRT_POLICY_POW_EXP2_LOG2     pow(x, 5.0) (raytrace.wgsl:415): default = (x x)(x x) x; flag = exp2(5 log2 x) evaluated in f64 and
 *                                rounded to f32 once.  Differs in the last bits of Schlick's reflectance.
 * Applies to the frames rendered after the call.  The bring-up kernel (BRT_FLAG_KERNEL_SIMPLE) implements the default only. */
enum { BRT_POLICY_OR_SHORT_CIRCUIT = 1u, BRT_POLICY_MINMAX_SELECT = 2u, BRT_POLICY_POW_EXP2_LOG2 = 4u };
int32_t brt_set_policy(brt_ctx* ctx, uint32_t flags);

/* Scheduling / launch-shape knobs of the trace path (names and meaning: DESIGN.md section 6, "Tuning aids").  None
 * changes a pixel.  They live in the context; nothing reads the environment per frame.  brt_create takes initial values
 * from the environment variables of the same names, once, and only when BRT_ENABLE_TUNING=1 is set.  No reference
 * counterpart (the reference has one fullscreen draw and nothing to tune, pipeline.rs:206-217). */
int32_t brt_set_tuning(brt_ctx* ctx, const char* name, uint32_t value);
int32_t brt_get_tuning(const brt_ctx* ctx, const char* name, uint32_t* out_value, uint32_t* out_default);

/* Replaces: model_buffer / material_buffer / bvh_buffer .write_buffer (pipeline.rs:136-138).
 * Takes the three CPU vectors that prepare_buffers builds (extract.rs:299-336), validates
 * them (indices in range, BVH reachable from node 0 without cycles) and copies them to
 * every device of the context.  If bvh_nodes == NULL / n_nodes == 0 the callee builds the
 * BVH itself (see brt_build_bvh_sah / brt_build_bvh_device): recommended, the ray loop runs faster in that tree than in
 * the caller's PLOC tree and the caller saves its own per-frame build (extract.rs:315-332).
 * The callee's tree pads a sphere's box by what the f32 arithmetic of the two intersection tests needs for the distances rays travel
 * (0.01 ... 0.1) instead of the reference's flat 0.1 (Model::aabb, extract.rs:220-227).  Those distances depend on the camera, which
 * an upload does not know: the tree is built for the scene's own extent, and every brt_render* call checks its camera first -- one
 * that is further out than the resident tree covers has the tree rebuilt on the GPU (same scene bytes, larger pads, up to the
 * reference's 0.1; 0.3-1 ms, brt_stats::tree_rebuilt) before its frame is launched.  The rule is brt_host_tree_reach.  A caller's
 * tree is used as it comes. */
int32_t brt_upload_scene(brt_ctx* ctx,
                         const void* models, uint32_t n_models,
                         const void* materials, uint32_t n_materials,
                         const void* bvh_nodes, uint32_t n_nodes);

/* Replaces: set_bind_group x2 + draw(0..3, 0..1) (pipeline.rs:160-217) and the whole
 * fragment() invocation grid (raytrace.wgsl:93-123).  Renders a width x height frame into
 * out_rgba (HOST pointer).  raster_rgba / raster_depth (host, width*height*4 / width*height
 * floats, reverse-Z depth) are the `screen_texture` and depth prepass the shader samples
 * (raytrace.wgsl:98,106,116); either may be NULL = cleared to 0.  Synchronous. */
int32_t brt_render(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t level,
                   uint32_t width, uint32_t height,
                   const float* raster_rgba, const float* raster_depth,
                   float* out_rgba, uint32_t flags, brt_stats* stats_or_null);

/* Optional fast path for brt_render: page-locked host memory owned by the context.  When
 * out_rgba (and/or raster_rgba / raster_depth) lies inside such an allocation the frame is DMA'd
 * straight into it (no staging copy on the CPU: ~2 ms less per 1080p frame).  The memory stays
 * valid until brt_host_free / brt_destroy.  Any other pointer keeps working through staging. */
int32_t brt_host_alloc(brt_ctx* ctx, uint64_t bytes, void** out_ptr);
int32_t brt_host_free(brt_ctx* ctx, void* ptr);

/* Same frame, but only the strips of `part` out of `n_parts` (strip s belongs to part
 * s % n_parts), written densely into a DEVICE tile buffer of brt_tile_rows() rows on the
 * context's first device: tile row (k*BRT_STRIP_ROWS + r) is frame row
 * ((k*n_parts + part)*BRT_STRIP_ROWS + r).  d_raster_* are optional DEVICE full-frame
 * buffers.  `hip_stream` is a hipStream_t.  NULL without BRT_FLAG_CALLER_STREAM = the context's own
 * (non-blocking) stream: the call then SYNCHRONISES before it returns, fills every field of stats and
 * refreshes the dispatch-order history.  A non-NULL stream, or BRT_FLAG_CALLER_STREAM: asynchronous on that
 * stream; only the launch-shape fields and `paths` of stats are filled.
 * One render per context is in flight at a time: the control block (counters, tile queue) is per context, so
 * a call first makes its stream wait (hipStreamWaitEvent) for the previous call's kernel, whichever stream
 * that ran on.  d_out_tile must not be read or overwritten by other streams before this call's work is done. */
int32_t brt_render_part_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t level,
                               uint32_t width, uint32_t height, uint32_t part, uint32_t n_parts,
                               const float* d_raster_rgba, const float* d_raster_depth,
                               float* d_out_tile, void* hip_stream, uint32_t flags,
                               brt_stats* stats_or_null);

/* The whole frame of an N-device context (brt_create with N ordinals), assembled ON ITS FIRST DEVICE: every device traces its
 * strips, the tiles of devices 1..N-1 travel to the first device by peer copy (hipMemcpyPeerAsync: xGMI inside a node) and a
 * copy kernel de-interleaves them into d_frame (DEVICE pointer on the first device, width*height*4 floats) -- the single
 * gather of tile buffers at frame end, for a single-process host.  Replaces, together with brt_upload_scene, the pass that
 * RayTracingNode::run encodes on post_process.destination (pipeline.rs:191-217); the caller copies or maps d_frame into its
 * colour target.  d_raster_rgba / d_raster_depth: optional full-frame DEVICE buffers on the first device (the callee forwards
 * them to the other devices).  Stream rule as for brt_render_part_device: NULL without BRT_FLAG_CALLER_STREAM = the context's
 * own stream, synchronous, every field of stats filled (gather_ms = from the end of the first device's trace to the
 * assembled frame); otherwise the de-interleave is enqueued on `hip_stream` (a stream of the first device) behind the
 * tiles' arrival and the call does not synchronise.  One frame per context in flight. */
int32_t brt_render_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t level,
                          uint32_t width, uint32_t height,
                          const float* d_raster_rgba, const float* d_raster_depth,
                          void* d_frame, void* hip_stream, uint32_t flags, brt_stats* stats_or_null);

/* Rows in the dense tile of `part` (same for every part: padded to whole strips). */
uint32_t brt_tile_rows(uint32_t height, uint32_t n_parts);

/* Root side of the gather: d_tiles holds n_parts tiles back to back (each
 * brt_tile_rows()*width*4 floats, i.e. the receive buffer of a gather); writes the
 * de-interleaved width x height frame to d_frame.  Stream rule as for brt_render_part_device: NULL without
 * BRT_FLAG_CALLER_STREAM = the context's own stream, synchronous; otherwise asynchronous on `hip_stream` --
 * pass the stream the gather was enqueued on (with BRT_FLAG_CALLER_STREAM if that is the default stream), or
 * the copy kernel is not ordered behind the gather. */
int32_t brt_deinterleave_device(brt_ctx* ctx, const float* d_tiles, uint32_t n_parts,
                                uint32_t width, uint32_t height, void* d_frame, void* hip_stream, uint32_t flags);

/* ---- strips by measured cost (one process per GPU) ------------------------------------------------------------------------------------
 * By default strip s of BRT_STRIP_ROWS rows belongs to part s % n_parts (interleaved, because bands are badly
 * imbalanced).  A STRIP TABLE assigns the strips by their cost instead: part_of_strip[s] = the part that renders frame strip s, a
 * permutation of the parts inside every group of n_parts consecutive strips -- so every part still has exactly one strip per group (its
 * k-th local strip lies in group k): tile size and layout, brt_tile_rows and the ONE gather stay as they are, only the two lookups
 * "local strip -> frame strip" (trace kernel) and "frame strip -> part" (assembly) go through the table.  Pixels cannot change: a
 * pixel's seed depends on its frame coordinates only (raytrace.wgsl:95).
 *   brt_set_strip_table   installs the table for frames of n_strips = ceil(height / 8) strips split n_parts ways (NULL: back to s % n_parts);
 *                         brt_render_part_device, brt_deinterleave_device and brt_gather_rccl of such frames use it; EVERY rank must set
 *                         the same table.  BRT_ERR_INVALID_ARGUMENT (and brt_last_error) if a group holds a part twice or a part >= n_parts,
 *                         if n_parts > 64 or n_strips > 4096: a refused table changes nothing, the table in force stays.  A frame whose
 *                         height or split does not fit the table in force renders and assembles by s % n_parts, in render and assembly
 *                         alike.  (brt_render / brt_render_device -- one context over N devices -- keep s % n_parts.)
 *                         A call uses the table in force WHEN IT IS CALLED: calls still in flight on any stream keep the table they were
 *                         called under, and a new table (or NULL) affects only the calls after it.  Changing the part from call to call
 *                         rewrites nothing; with an unchanged table no call waits on the host for a caller's stream.
 *   brt_plan_strips       makes a table from measured costs and installs it: the frame of this camera is rendered once at `probe_spp`
 *                         samples per pixel on the context's first device with the per-tile ray counts switched on; per group the dearest
 *                         strip goes to the part with the least so far.  Deterministic: every rank of a job computes the same table from
 *                         the same integers, no second collective.  out_part_of_strip (n_strips words) may be NULL. */
int32_t brt_set_strip_table(brt_ctx* ctx, uint32_t n_parts, uint32_t n_strips, const uint32_t* part_of_strip);
int32_t brt_plan_strips(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t level, uint32_t width, uint32_t height,
                        uint32_t n_parts, uint32_t probe_spp, uint32_t* out_part_of_strip);
/* the assignment rule of brt_plan_strips on given costs (host arithmetic, no device: what the CPU tests hold it to) */
int32_t brt_host_plan_strips(const uint64_t* strip_cost, uint32_t n_strips, uint32_t n_parts, uint32_t* out_part_of_strip);

/* ---- the one collective of the path: one process per GPU, one RCCL gather per frame -----------------
 * For a host that runs one process per GPU (instead of one N-device context, brt_render_device): every rank renders its part
 * with brt_render_part_device, then all ranks call brt_gather_rccl -- ONE ncclGather (rccl.h:745) of the tiles to rank 0, and on
 * rank 0 the de-interleave kernel (brt_deinterleave_device) behind it on the same stream.  librccl is resolved with dlopen at
 * the first of these calls (a copy already in the process is used; a single-GPU host needs none); BRT_ERR_RCCL if that fails.
 *   brt_rccl_unique_id    ncclGetUniqueId: on ONE rank; hand the 128 bytes to the others by whatever the host has (a pipe, MPI, a file)
 *   brt_rccl_comm_create  ncclCommInitRank on the context's first device; every rank calls it (it blocks until all have)
 *   brt_gather_rccl       d_tile: this rank's tile (brt_tile_rows(height, world) x width x 4 floats); d_tiles_on_root: `world` such
 *                         tiles on rank 0 (NULL elsewhere); d_frame_on_root: width x height x 4 floats on rank 0, or NULL to skip
 *                         the de-interleave.  Stream rule as for brt_render_part_device (NULL without BRT_FLAG_CALLER_STREAM = the
 *                         context's own stream, synchronous).  The tile must not be rendered into again before the gather is done.
 * A communicator created elsewhere (ncclComm_t of the host's own RCCL binding) may be passed as `nccl_comm` as well. */
int32_t brt_rccl_unique_id(void* out_id128);
int32_t brt_rccl_comm_create(brt_ctx* ctx, const void* id128, int32_t rank, int32_t world, void** out_comm);
int32_t brt_rccl_comm_destroy(brt_ctx* ctx, void* comm);
int32_t brt_gather_rccl(brt_ctx* ctx, void* nccl_comm, int32_t rank, int32_t world, const float* d_tile, float* d_tiles_on_root,
                        uint32_t width, uint32_t height, void* d_frame_on_root, void* hip_stream, uint32_t flags);

/* ---- a frame target in another API's memory -----------------------------------------------------------
 * Replaces: the pass writing straight into post_process.destination (pipeline.rs:191-203).  The host exports the memory behind
 * its colour target (or a buffer it copies from on the GPU) as a file descriptor; brt_import_frame_fd maps it on the context's
 * first device and returns a device pointer that brt_render_device / brt_render_part_device / brt_gather_rccl accept as
 * d_frame.  handle_type: BRT_EXTMEM_OPAQUE_FD = a Vulkan allocation exported with
 * VK_EXTERNAL_MEMORY_HANDLE_TYPE_OPAQUE_FD_BIT (hipImportExternalMemory; the runtime owns the descriptor on success);
 * BRT_EXTMEM_DMABUF_FD = a dma-buf of a HIP virtual-memory allocation (hipMemImportFromShareableHandle; the caller keeps and
 * closes its descriptor).  brt_release_frame unmaps (after the context's pending work); brt_destroy releases what is left. */
enum { BRT_EXTMEM_OPAQUE_FD = 1, BRT_EXTMEM_DMABUF_FD = 2 };
int32_t brt_import_frame_fd(brt_ctx* ctx, int32_t fd, uint64_t bytes, uint32_t handle_type, void** out_d_frame);
int32_t brt_release_frame(brt_ctx* ctx, void* d_frame);
/* Diagnostic (tests): allocates `bytes` of exportable device memory on the first device (hipMemCreate), maps it and exports it
 * as a dma-buf descriptor -- the other side of brt_import_frame_fd when no Vulkan is at hand.  Release with brt_release_frame;
 * the caller closes the descriptor. */
int32_t brt_debug_export_frame_fd(brt_ctx* ctx, uint64_t bytes, int32_t* out_fd, void** out_d_ptr);
/* Diagnostic: hipMemcpy device -> host on the context's first device (for pointers that are no tensor of the caller's). */
int32_t brt_debug_copy_to_host(brt_ctx* ctx, const void* d_src, void* h_dst, uint64_t bytes);

/* Diagnostic: evaluates one device function of the ray loop on n inputs (16 floats in,
 * 8 floats out per element; op codes BRT_DBG_* below) so that tests can compare single
 * reference functions (rngNextFloat, ray_bounding_dst, hit_sphere, the seed formula,
 * min/max/sqrt/divide) bit for bit.  Host pointers, synchronous. */
enum {
    BRT_DBG_MINMAX = 0,    /* in: a, b            out: min(a,b), max(a,b) */
    BRT_DBG_SQRT_DIV = 1,  /* in: a, b            out: sqrt(a), a / b */
    BRT_DBG_RNG = 2,       /* in: state (bits)    out: float, state', ball.xyz, state'' (bits) */
    BRT_DBG_SLAB = 3,      /* in: o3 d3 bmin3 bmax3 closest   out: child pushed (0/1) */
    BRT_DBG_SPHERE = 4,    /* in: o3 d3 center3 radius        out: accepted t or INF */
    BRT_DBG_SEED = 5,      /* in: seed px py W H (floats)     out: rng seed (bits) */
    BRT_DBG_DIV = 6,       /* in: n, d            out: n / d, shared-reciprocal short form, 1 / d, its short form (brt_device.h) */
    BRT_DBG_DIV_SWEEP = 7, /* in: seed (bits), count          out: mismatches of the short forms over `count` random plain-range pairs,
                              bits of the first mismatching n and d */
    BRT_DBG_SQRT_SWEEP = 8,/* in: first (bits), count, form   out: mismatches of the short sqrt (form 0; form != 0: of the rsq form, positive arguments only) over `count` consecutive floats per element
                              (element i starts at first + i * count; element 0 also checks +0 and -0), bits of the first mismatching argument */
    BRT_DBG_ENCODE = 9     /* in: c               out (as floats holding integers): the 8-bit sRGB code, the 8-bit unorm code, the f16 bits of c
                              (the store conversions of BRT_FLAG_OUT_*) */
};
int32_t brt_debug_eval(brt_ctx* ctx, uint32_t op, const float* in16, float* out8, uint32_t n);

/* ---- denoiser ----------------------------------------------------------------------------------------------------------------------
 * An edge-avoiding a-trous wavelet filter (Dammertz et al. 2010, with the spatial edge-stopping and variance terms of SVGF) guided by the
 * first hit of every pixel-centre ray: normal, distance, and the first bounce's base colour, which is divided out before the filter and
 * multiplied back after it.  Formulas and kernels: DESIGN.md "Denoiser".  Deterministic: the same input gives the same output bits.
 *   brt_set_denoise          the context's settings: iterations 1..6 (pass i has step 2^i), sigma_luminance, sigma_normal, sigma_depth
 *                            finite and > 0.  Defaults 5, 4, 128, 1.  Anything else: BRT_ERR_INVALID_ARGUMENT, settings unchanged.
 *   brt_denoise_device       denoises an RGBA f32 width x height DEVICE frame the caller holds (e.g. the root's frame after
 *                            brt_gather_rccl) rendered with camera80 / window16 on the resident scene, into d_out (DEVICE, the
 *                            BRT_FLAG_OUT_* format of `flags`; may equal d_frame_rgba).  flags: BRT_FLAG_CALLER_STREAM, BRT_FLAG_OUT_*
 *                            (and BRT_FLAG_DENOISE, implied); other bits BRT_ERR_INVALID_ARGUMENT.  Stream rule as for
 *                            brt_render_device; stats_or_null: total_ms only.  BRT_ERR_NO_SCENE before an upload.
 *                            With BRT_FLAG_TEMPORAL the frame is accumulated into the temporal history, and denoised only if
 *                            BRT_FLAG_DENOISE is set as well (the per-rank form: the root accumulates the assembled frame).
 *   brt_debug_denoise_guides diagnostic: the guide buffer of that frame, out8[(y * width + x) * 8 + k] = normal.xyz, t (+INF: no hit),
 *                            a.rgb (the demodulation factor), material id as bits (0xFFFFFFFF: no hit).  Host memory, synchronous. */
int32_t brt_set_denoise(brt_ctx* ctx, uint32_t iterations, float sigma_luminance, float sigma_normal, float sigma_depth);
int32_t brt_denoise_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height,
                           const float* d_frame_rgba, void* d_out, void* hip_stream, uint32_t flags, brt_stats* stats_or_null);
int32_t brt_debug_denoise_guides(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height, float* out8);

/* ---- post-passes on blended frames ---------------------------------------------------------------------------------------------------
 * brt_blend_post_device is brt_denoise_device for a level-1 / level-2 frame the caller holds (the per-rank form of BRT_FLAG_BLEND_POST).
 * d_coverage_rgba: the assembled RGBA f32 width x height DEVICE frame of that level rendered with d_raster_rgba = NULL and the raster
 * depth (any entry point, brt_render_part_device + brt_gather_rccl included) -- a pixel counts as covered iff its alpha is exactly +0.0.
 * d_raster_rgba_or_null: the raster colour, RGBA f32 width x height on the first device (NULL: zeros); it must not overlap d_out.
 * The covered pixels of d_out are their raster texels, the others are denoised / accumulated as brt_denoise_device does with a Pure
 * frame; d_out (the BRT_FLAG_OUT_* format of `flags`) may equal d_coverage_rgba.  flags: BRT_FLAG_CALLER_STREAM, BRT_FLAG_OUT_*,
 * BRT_FLAG_DENOISE, BRT_FLAG_TEMPORAL (BRT_FLAG_DENOISE is implied without BRT_FLAG_TEMPORAL); other bits BRT_ERR_INVALID_ARGUMENT.
 * Stream rule and stats as for brt_denoise_device.  Formulas: DESIGN.md "Post-passes on blended frames". */
int32_t brt_blend_post_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height,
                              const float* d_coverage_rgba, const float* d_raster_rgba_or_null, void* d_out, void* hip_stream,
                              uint32_t flags, brt_stats* stats_or_null);

/* ---- temporal accumulation ---------------------------------------------------------------------------------------------------------
 * The context keeps, on its first device, a per-pixel history of BRT_FLAG_TEMPORAL frames: the accumulated demodulated colour, the two
 * moments of its luminance, a history length n, and the previous frame's guides.  Every temporal frame carries each hit pixel's first
 * hit back through its sphere's motion and into the previous camera, keeps the bilinear taps of the history there that lie on the same
 * sphere and material with a similar normal and distance, and blends its demodulated colour in with alpha = 1 / min(n + 1, max_history).
 * Sky and non-finite pixels pass through.  Formulas: DESIGN.md "Temporal accumulation".  Deterministic.
 * The history is emptied by brt_reset_temporal (call it on a camera cut), by a frame of another width or height, by an upload with
 * another sphere or material count, and by brt_set_temporal.  Frames without the flag neither read nor change it.  One temporal frame
 * per context is in flight: the next one is ordered behind it on any stream.  Samples come from brt_window's random_seed: a caller who
 * renders the same seed twice adds no new samples, only weight to the old ones -- change the seed every frame.
 *   brt_set_temporal           max_history 1..65535 (default 32; 1: no accumulation), and an empty history.  Else
 *                              BRT_ERR_INVALID_ARGUMENT, settings unchanged.
 *   brt_reset_temporal         an empty history.
 *   brt_debug_temporal_state   diagnostic: the history after the last temporal frame, out8[(y * width + x) * 8 + k] = h.rgb, n, m1, m2,
 *                              x', y' (the reprojected position in the previous frame; NaN where the history was rejected, the pixel
 *                              itself in the identity case).  An empty history: n = 0, x' = y' = NaN everywhere.  Host memory,
 *                              synchronous.  BRT_ERR_INVALID_ARGUMENT for a size other than the history's. */
int32_t brt_set_temporal(brt_ctx* ctx, uint32_t max_history);
int32_t brt_reset_temporal(brt_ctx* ctx);
int32_t brt_debug_temporal_state(brt_ctx* ctx, uint32_t width, uint32_t height, float* out8);

/* ---- ray queries ---------------------------------------------------------------------------------------------------------------------
 * Batches of rays against the resident scene and tree (picking, line of sight, probes): the reference's `raycast`
 * (raytrace.wgsl:313-362: push and pop order, strict `<` ties, root box untested, the 32-entry overflow rule) for every ray, on the
 * context's first device.  Rules, kernels and costs: DESIGN.md "Ray queries".  Deterministic.
 *   ray, 32 bytes    { origin.xyz, t_max, direction.xyz, user }: f32 x 7 and a u32 that is carried into the result untouched.  The
 *                    direction is used as given (not normalised): t is in units of |direction|.  t_max = +INF: unbounded.
 *   hit, 32 bytes    { t, normal.xyz, sphere, material, status, user }: f32 x 4 and u32 x 4.  sphere: the index into the `models` of
 *                    the last brt_upload_scene (whatever numbering is resident); normal = normalize(ray_at(t) - centre)
 *                    (raytrace.wgsl:356, not flipped); status: BRT_QUERY_STATUS_*.  A miss: t = +INF, normal 0, sphere = material =
 *                    BRT_QUERY_NONE.  The reference's lower bound stays: a hit has t > 0.001.
 *   mode             BRT_QUERY_CLOSEST: the reference's closest hit; with a finite t_max it is reported iff its t < t_max, else a
 *                    miss.  BRT_QUERY_ANY: status only (BRT_QUERY_STATUS_HIT iff CLOSEST would report a hit under the same t_max;
 *                    the other fields read as a miss's); the walk may stop at the first accepted sphere.
 *   refusals         a ray with a non-finite component, or t_max NaN or <= 0: BRT_QUERY_STATUS_INVALID.  A ray whose
 *                    (|o.x| + |o.y|) + |o.z| (f32) exceeds what the resident tree covers (brt_query_origin_bound):
 *                    BRT_QUERY_STATUS_OUT_OF_REACH.  Neither is walked; both read as a miss otherwise.
 *   origin_bound     0: the tree is used as it stands.  > 0 (finite): a callee-built tree whose bound is below it is first rebuilt
 *                    for a reach that covers origins of that 1-norm (the rule of a camera there, judged without its position); a
 *                    query never lowers the reach, and later frames are traced on that tree too until the next upload (a side effect on
 *                    the frames: same walk rule, longer leaf pads).  NaN or < 0:
 *                    BRT_ERR_INVALID_ARGUMENT.  A caller's tree is honoured as it comes: its bound is +INF.
 *   brt_query_rays_device   d_rays / d_hits: DEVICE buffers of n_rays records on the first device (they must not overlap).  flags:
 *                    BRT_FLAG_CALLER_STREAM only.  Stream rule as for brt_denoise_device: on the context's own stream the call
 *                    returns when the results are there; on a caller's stream it only enqueues.  Queries of one context run one
 *                    behind the other on whatever streams they come; uploads and tree rebuilds wait for them.  A query changes no
 *                    frame and no frame changes a query.
 *   brt_query_rays   the same for HOST buffers, synchronous.
 *   out_stats8_or_null   [0] rays walked, [1] hits, [2] rays refused (these three are counted only by calls that synchronise: the own
 *                    stream and brt_query_rays; 0 on a caller's stream), [3] the tree was rebuilt, [4] its reach (f32 bits in the low
 *                    word; brt_stats::tree_reach), [5] the kernel form taken (0 plain, 1 streaming), [6] workgroups (both diagnostic: what the launch decision was), [7] reserved.
 *   brt_query_origin_bound  *out_bound = the largest origin 1-norm the resident tree covers (+INF: any).
 *   brt_host_pixel_ray      host arithmetic, no context: the pixel-centre ray of pixel (px, py) of a width x height frame of that camera
 *                    and window, as the guide buffer casts it (f32, the kernel's order of operations), t_max = +INF, user =
 *                    py * width + px.  BRT_ERR_INVALID_ARGUMENT for a pixel outside the frame.
 * n_rays = 0 is BRT_OK and launches nothing.  BRT_ERR_NO_SCENE before an upload; null pointers and unknown modes
 * BRT_ERR_INVALID_ARGUMENT.  Which kernel form a call takes is a launch decision (tuning knob BRT_QUERY_FORM: 0 the default rule, 1 plain,
 * 2 streaming); the results do not depend on it. */
#define BRT_QUERY_CLOSEST 0u
#define BRT_QUERY_ANY 1u
#define BRT_QUERY_STATUS_MISS 0u
#define BRT_QUERY_STATUS_HIT 1u
#define BRT_QUERY_STATUS_FRONT_FACE 2u     /* set beside HIT (CLOSEST only): dot(direction, normal) < 0 (raytrace.wgsl:358) */
#define BRT_QUERY_STATUS_INVALID 4u
#define BRT_QUERY_STATUS_OUT_OF_REACH 8u
#define BRT_QUERY_NONE 4294967295u
int32_t brt_query_rays_device(brt_ctx* ctx, const void* d_rays, uint32_t n_rays, uint32_t mode, float origin_bound, void* d_hits,
                              void* hip_stream, uint32_t flags, uint64_t* out_stats8_or_null);
int32_t brt_query_rays(brt_ctx* ctx, const void* rays, uint32_t n_rays, uint32_t mode, float origin_bound, void* hits,
                       uint64_t* out_stats8_or_null);
int32_t brt_query_origin_bound(brt_ctx* ctx, float* out_bound);
int32_t brt_host_pixel_ray(const void* camera80, const void* window16, uint32_t width, uint32_t height, uint32_t px, uint32_t py,
                           void* out_ray32);

/* ---- radiance queries ----------------------------------------------------------------------------------------------------------------
 * Path-traced colour for batches of the caller's rays (reflection rays from a G-buffer, light probes, cube maps, fisheye or orthographic
 * views -- whole orthographic frames: brt_render_lens* --, a host integrator): what a ray SEES, where a ray query answers what it
 * hits.  On the context's first device.  Rule, kernels and costs: DESIGN.md "Radiance queries".  Deterministic; the default policy only (brt_set_policy: else BRT_ERR_UNSUPPORTED).
 *   ray, 32 bytes    { origin.xyz, seed, direction.xyz, user }: f32 x 3, u32, f32 x 3, u32 -- the query ray with `seed` where t_max is.
 *                    The direction is used as given, as in ray queries; raytrace normalises where the shader does.
 *   result, 32 bytes { t, r, g, b, sphere, material, status, user }: f32 x 4 and u32 x 4 -- the query hit with the colour where the
 *                    normal is.
 *   the rule         state = seed; sum = 0; `samples` times: sum += raytrace(Ray(origin, direction), &state).color; rgb = sum /
 *                    f32(samples).  raytrace is raytrace.wgsl:174-224 at level 3 with camera.bounce_count = `bounces`; state is
 *                    random.wgsl's rng_state, set to `seed` and threaded through the samples: trace_multisampled (:159-172) with the
 *                    caller's ray in place of random_ray_from_uv.  No jitter: a caller that wants anti-aliasing varies the ray.  Every
 *                    operation is a separately rounded f32 operation.  t, sphere, material, status and user are exactly what
 *                    brt_query_rays reports in BRT_QUERY_CLOSEST mode for { origin, +INF, direction, user }, BRT_QUERY_STATUS_FRONT_FACE
 *                    and the sphere numbering included; a miss has t = +INF and sphere = material = BRT_QUERY_NONE (and the sky's
 *                    colour).
 *   refusals         those of ray queries without the t_max clause: a non-finite component of origin or direction:
 *                    BRT_QUERY_STATUS_INVALID; (|o.x| + |o.y|) + |o.z| (f32) above the resident tree's bound
 *                    (brt_query_origin_bound): BRT_QUERY_STATUS_OUT_OF_REACH.  A refused ray is not walked and reads as a miss with
 *                    rgb = 0.
 *   samples, bounces samples in [1, 65535], bounces in [0, 65535]; else BRT_ERR_INVALID_ARGUMENT.
 *   origin_bound     as for brt_query_rays: 0 uses the tree as it stands; > 0 may first raise a callee-built tree's reach to what
 *                    origins of that 1-norm need, and never lowers it; NaN or < 0: BRT_ERR_INVALID_ARGUMENT.  A path's later bounces
 *                    start inside the scene, exactly as a frame's do, so the reach rule that covers a camera at that origin covers the
 *                    query.  The same side effect on later frames applies (they are traced on that tree until the next upload).
 *   brt_radiance_rays_device   d_rays / d_out: DEVICE buffers of n_rays records on the first device; overlapping ones are
 *                    BRT_ERR_INVALID_ARGUMENT.  flags: BRT_FLAG_CALLER_STREAM only.  Stream rule as for brt_query_rays_device: on the
 *                    context's own stream the call returns when the results are there; on a caller's stream it only enqueues.  Radiance
 *                    lists of one context run one behind the other, and behind its ray queries, pixel lists and post-pass calls, on
 *                    whatever streams they come; uploads and tree rebuilds wait for them.  A radiance call changes no frame and no frame
 *                    changes a radiance result.
 *   brt_radiance_rays   the same for HOST buffers, synchronous.
 *   out_stats8_or_null   [0] walks performed (an entry's own ray is walked once, whatever `samples` is), [1] entries whose own ray hit,
 *                    [2] entries refused (these three are counted only by calls that synchronise: the own stream and
 *                    brt_radiance_rays; 0 on a caller's stream), [3] the tree was rebuilt, [4] its reach (f32 bits in the low word;
 *                    brt_stats::tree_reach), [5] the kernel form taken (0 plain, 1 streaming), [6] workgroups (both diagnostic), [7]
 *                    reserved.
 * n_rays = 0 is BRT_OK and launches nothing.  BRT_ERR_NO_SCENE before an upload; null pointers BRT_ERR_INVALID_ARGUMENT.  A refused call
 * leaves the context usable.  Which kernel form a call takes is a launch decision (tuning knob BRT_RADIANCE_FORM: 0 the default rule, 1
 * plain, 2 streaming); the bytes written do not depend on it. */
int32_t brt_radiance_rays_device(brt_ctx* ctx, const void* d_rays, uint32_t n_rays, uint32_t samples, uint32_t bounces, float origin_bound,
                                 void* d_out, void* hip_stream, uint32_t flags, uint64_t* out_stats8_or_null);
int32_t brt_radiance_rays(brt_ctx* ctx, const void* rays, uint32_t n_rays, uint32_t samples, uint32_t bounces, float origin_bound, void* out,
                          uint64_t* out_stats8_or_null);

/* ---- light probes ---------------------------------------------------------------------------------------------------------------------
 * Irradiance records for a list of positions (the ambient terms of a level-1 / level-2 host: L2 spherical harmonics, or the six colours
 * of an ambient cube): per probe a fixed direction set is traced as radiance entries, the colours are made linear and projected, all on
 * the context's first device.  Rule, kernels and costs: DESIGN.md "Light probes".  Deterministic; the default policy only.
 *   probe, 16 bytes   { position.xyz, seed }: f32 x 3, u32.
 *   directions        n_dirs = N in [1, 65536]; for k = 0 .. N-1, in float64: y = 1 - (2k+1)/N, r = sqrt(max(0, 1 - y*y)),
 *                     phi = 2 pi frac(k (sqrt(5)-1)/2), d_k = (f32(r cos phi), f32(y), f32(r sin phi)): a Fibonacci sphere stratified
 *                     along the up axis, equal weights.  brt_host_probe_directions is the only place that computes it.
 *   rays              entry k of a probe is the radiance entry { position, seed + k * 0x9E3779B9 (mod 2^32), d_k, user = k }, traced
 *                     with samples = 1 and the call's `bounces` under the rule of "radiance queries".  More paths: more directions, or
 *                     the average of bakes with other seeds (the records are linear).
 *   linear radiance   L_k = rgb_k * rgb_k per channel (the shader returns sqrt(colour) per sample).
 *   projection        f32, every operation separately rounded; lane l of 64 sums k = l, l + 64, ... in order from +0.0, then for off =
 *                     32, 16, 8, 4, 2, 1: acc[l] = acc[l] + acc[l + off]; lane 0 holds the sums.
 *                     BRT_PROBE_SH9: c[j][ch] = (12.566371f / f32(N)) * sum_k Y_j(d_k) * L_k[ch] with Y0 = 0.282095, Y1..3 = 0.488603 *
 *                     (y, z, x), Y4 = 1.092548 x y, Y5 = 1.092548 y z, Y6 = 0.315392 (3 z z - 1), Y7 = 1.092548 x z, Y8 = 0.546274 (x x -
 *                     y y).  BRT_PROBE_AMBIENT_CUBE: faces +X, -X, +Y, -Y, +Z, -Z; per face m = max(+-component, 0), m2 = m * m,
 *                     value = (sum m2 * L) / (sum m2), 0 where the denominator is 0.
 *   record, 128 bytes { f32 coeff[27], u32 hits, status, n_dirs, basis, reserved = 0 }.  SH9: coeff[3 j + ch]; cube: coeff[3 face + ch],
 *                     words 18..26 are 0.  hits: the probe's entries whose own ray hit.  status: entry 0's BRT_QUERY_STATUS_INVALID /
 *                     BRT_QUERY_STATUS_OUT_OF_REACH bits (a probe with a non-finite component; a probe beyond the tree's bound,
 *                     brt_query_origin_bound); a refused probe has all coefficients 0 and hits 0.
 *   list layout       the step exports read and write lists of n_probes * n_dirs radiance entries / results in PROBE-MAJOR order: entry
 *                     k of probe p is record p * n_dirs + k.
 *   brt_host_probe_directions   host arithmetic, no context: out_xyz[3 k ..] = d_k.  n_dirs 0 or above 65536: BRT_ERR_INVALID_ARGUMENT.
 *   brt_host_probe_irradiance   host arithmetic, no context: out_rgb3 = the record evaluated for the unit normal normal3.  SH9: E(n) =
 *                     sum_j A_l c_j Y_j(n) with A = pi, 2 pi / 3, pi / 4 for bands 0, 1, 2 (the irradiance); cube: the n^2-weighted sum of
 *                     the three faces n points into.  A record of another basis: BRT_ERR_INVALID_ARGUMENT.
 *   brt_probe_rays_device       the generation kernel alone: n_probes probes at d_probes -> n_probes * n_dirs radiance entries at d_rays
 *                     (DEVICE buffers; NaN and INF components are copied through).
 *   brt_probe_project_device    the projection kernel alone, on any list of radiance results in that layout -> n_probes records at d_out
 *                     (DEVICE buffers).  Needs no scene.
 *   brt_bake_probes_device      everything in one call on DEVICE buffers: in chunks of whole probes, generate -> the radiance kernels ->
 *                     project.  A chunk is max(1, BRT_PROBE_CHUNK_RAYS / n_dirs) probes (tuning knob, default 2^21 entries: 128 MiB of
 *                     staging in the context); the records do not depend on it, nor on BRT_RADIANCE_FORM.  origin_bound: as for
 *                     brt_radiance_rays.
 *   brt_bake_probes             the same for HOST buffers, synchronous.
 *   out_stats8_or_null   [0..2] walks performed, entries whose own ray hit, entries refused, summed over the chunks (counted only by calls
 *                     that synchronise: the own stream and brt_bake_probes; 0 on a caller's stream), [3] the tree was rebuilt, [4] its
 *                     reach (f32 bits in the low word), [5] the radiance form of the last chunk (0 plain, 1 streaming), [6] chunks, [7] 0.
 * flags: BRT_FLAG_CALLER_STREAM only; stream rule as for brt_radiance_rays_device, and the calls run one behind the other with the
 * context's radiance lists, ray queries and pixel lists on whatever streams they come.  Overlapping buffers, null pointers, bounces above
 * 65535, a basis other than the two, n_dirs outside [1, 65536] and, for the step exports, n_probes * n_dirs above 0x7fff0000:
 * BRT_ERR_INVALID_ARGUMENT.  The bakes: BRT_ERR_NO_SCENE before an upload, BRT_ERR_UNSUPPORTED under a set policy.  n_probes = 0 is BRT_OK
 * and launches nothing.  A refused call leaves the context usable; a bake changes no frame. */
#define BRT_PROBE_SH9 0u
#define BRT_PROBE_AMBIENT_CUBE 1u
int32_t brt_host_probe_directions(uint32_t n_dirs, float* out_xyz);
int32_t brt_host_probe_irradiance(const void* record128, const float* normal3, float* out_rgb3);
int32_t brt_probe_rays_device(brt_ctx* ctx, const void* d_probes, uint32_t n_probes, uint32_t n_dirs, void* d_rays, void* hip_stream,
                              uint32_t flags);
int32_t brt_probe_project_device(brt_ctx* ctx, const void* d_results, uint32_t n_probes, uint32_t n_dirs, uint32_t basis, void* d_out,
                                 void* hip_stream, uint32_t flags);
int32_t brt_bake_probes_device(brt_ctx* ctx, const void* d_probes, uint32_t n_probes, uint32_t n_dirs, uint32_t bounces, uint32_t basis,
                               float origin_bound, void* d_out, void* hip_stream, uint32_t flags, uint64_t* out_stats8_or_null);
int32_t brt_bake_probes(brt_ctx* ctx, const void* probes, uint32_t n_probes, uint32_t n_dirs, uint32_t bounces, uint32_t basis,
                        float origin_bound, void* out, uint64_t* out_stats8_or_null);

/* ---- irradiance volumes --------------------------------------------------------------------------------------------------------------
 * A regular lattice of light probes over an axis-aligned box, baked in one call, and lists of { position, normal } lit from the baked
 * records on the device: the ambient term of a level-1 / level-2 host's raster pixels.  On the context's first device.  Rule, kernels and
 * costs: DESIGN.md "Irradiance volumes".  Deterministic: f32, every operation separately rounded, in the order written here.
 *   volume, 48 bytes  { f32 origin[3]; u32 seed; f32 spacing[3]; u32 basis; u32 count[3]; u32 flags }.  basis: BRT_PROBE_SH9 or
 *                     BRT_PROBE_AMBIENT_CUBE; flags: 0 or BRT_VOLUME_WRAP.  Probe (ix, iy, iz) has index i = (iz * count[1] + iy) *
 *                     count[0] + ix, position origin[a] + f32(i_a) * spacing[a] per axis (a multiply, then an add) and seed
 *                     seed + i * 0x85EBCA6B (mod 2^32).  Valid: origin finite, spacing finite and > 0, every count in [1, 1024], the
 *                     product of the counts <= 1 << 20, a known basis and flags; anything else is BRT_ERR_INVALID_ARGUMENT.
 *   records           the 128-byte records of "light probes", one per probe in index order.
 *   point, 32 bytes   { f32 position[3]; u32 ignored; f32 normal[3]; u32 ignored }.  The normal is used as given.
 *   sample, 16 bytes  { f32 rgb[3]; u32 status }, status: BRT_VOLUME_STATUS_* bits.
 *   the rule          1. a non-finite component of position or normal: rgb = 0, status = INVALID, nothing else.
 *                     2. per axis a: t = (p_a - origin_a) / spacing_a; hi = f32(count_a - 1); CLAMPED is set if t < 0 or t > hi;
 *                        t = t > 0 ? t : 0; t = t < hi ? t : hi; i0 = min(u32(floor(t)), max(count_a, 2) - 2); f = t - f32(i0);
 *                        i1 = min(i0 + 1, count_a - 1).
 *                     3. SH9: AY_j = A_j * Y_j(n) with the basis of "light probes" and A = 3.1415927f, 2.0943952f, 0.7853982f for
 *                        bands 0, 1, 2.  Cube: n2_a = n_a * n_a, face_a = 2 a + (n_a < 0).
 *                     4. corners c = 0 .. 7 in order, bit 0 / 1 / 2 selecting i1 on x / y / z: w = (wx * wy) * wz with w_a = f for a
 *                        set bit, 1 - f otherwise.  A corner whose record has status != 0 or a basis other than the descriptor's
 *                        contributes nothing.  Under BRT_VOLUME_WRAP: d = probe position - p; len2 = (dx dx + dy dy) + dz dz;
 *                        cs = len2 > 0 ? ((dx nx + dy ny) + dz nz) / sqrt(len2) : 1; h = (cs + 1) * 0.5; w = w * (h * h + 0.2).
 *                        SH9: E_c[ch] from +0.0, E_c = E_c + AY_j * coeff[3 j + ch] for j = 0 .. 8.  Cube: E_c[ch] = (n2_x *
 *                        c[3 face_x + ch] + n2_y * c[3 face_y + ch]) + n2_z * c[3 face_z + ch].  acc[ch] = acc[ch] + w * E_c[ch];
 *                        sw = sw + w.
 *                     5. sw > 0: E = acc / sw, then E = E < 0 ? 0 : E (a NaN stays a NaN).  Otherwise rgb = 0 and NO_PROBE is set.
 *   brt_host_volume_probes     host arithmetic, no context: the lattice's 16-byte probes in index order.
 *   brt_host_volume_sample     host arithmetic, no context: the rule over a list of n_points points; the compiled twin of the kernel.
 *   brt_volume_probes_device   the generation kernel alone: the lattice's probes at d_probes (DEVICE).
 *   brt_bake_volume_device     the lattice's probes into a buffer of the context, then brt_bake_probes_device's chunked bake of them into
 *                     d_records (DEVICE, product-of-counts records).  n_dirs, bounces, origin_bound, out_stats8_or_null: as there.
 *   brt_bake_volume            the same for a HOST buffer, synchronous.
 *   brt_sample_volume_device   n_points points at d_points -> samples at d_out from the records at d_records (DEVICE).  Needs no scene.
 *   brt_sample_volume          the same for HOST buffers, synchronous (all three lists are staged in one buffer of the context).
 * flags: BRT_FLAG_CALLER_STREAM only; stream rule and ordering as for the step exports of "light probes".  A bad descriptor, null
 * pointers, a DEVICE buffer that is not 16-byte aligned (the kernels move whole 16-byte words), an output that overlaps the points or
 * the records, n_points above 0x7fff0000: BRT_ERR_INVALID_ARGUMENT.  The bakes add the
 * probe bakes' refusals (BRT_ERR_NO_SCENE, BRT_ERR_UNSUPPORTED under a set policy, n_dirs, bounces, origin_bound).  n_points = 0 is
 * BRT_OK and launches nothing.  A refused call leaves the context usable; no call here changes a frame or the dispatch history. */
#define BRT_VOLUME_WRAP 1u
#define BRT_VOLUME_STATUS_CLAMPED 1u
#define BRT_VOLUME_STATUS_INVALID 4u
#define BRT_VOLUME_STATUS_NO_PROBE 8u
int32_t brt_host_volume_probes(const void* volume48, void* out_probes);
int32_t brt_host_volume_sample(const void* volume48, const void* records, const void* points, uint32_t n_points, void* out);
int32_t brt_volume_probes_device(brt_ctx* ctx, const void* volume48, void* d_probes, void* hip_stream, uint32_t flags);
int32_t brt_bake_volume_device(brt_ctx* ctx, const void* volume48, uint32_t n_dirs, uint32_t bounces, float origin_bound, void* d_records,
                               void* hip_stream, uint32_t flags, uint64_t* out_stats8_or_null);
int32_t brt_bake_volume(brt_ctx* ctx, const void* volume48, uint32_t n_dirs, uint32_t bounces, float origin_bound, void* records,
                        uint64_t* out_stats8_or_null);
int32_t brt_sample_volume_device(brt_ctx* ctx, const void* volume48, const void* d_records, const void* d_points, uint32_t n_points,
                                 void* d_out, void* hip_stream, uint32_t flags);
int32_t brt_sample_volume(brt_ctx* ctx, const void* volume48, const void* records, const void* points, uint32_t n_points, void* out);

/* ---- reflection probes ----------------------------------------------------------------------------------------------------------------
 * A cube map traced from one position and its mip chain prefiltered by roughness: the specular map of a level-1 / level-2 host's
 * environment light (Bevy's EnvironmentMapLight), and -- through the filter step with a cosine table -- its diffuse map.  On the
 * context's first device.  Rule, kernels and costs: DESIGN.md "Reflection probes".  Deterministic: f32, every operation separately
 * rounded, in the order written here.
 *   cube              6 faces of size x size texels, stored [face][y][x]; a texel is 16 bytes { f32 r, g, b, a }.  Faces in the order +X,
 *                     -X, +Y, -Y, +Z, -Z (wgpu, Vulkan, D3D).
 *   texel direction   u = f32(2x+1) / f32(size) - 1, v = f32(2y+1) / f32(size) - 1; raw = +X (1, -v, -u), -X (-1, -v, u), +Y (u, 1, v),
 *                     -Y (u, -1, -v), +Z (u, -v, 1), -Z (-u, -v, -1); len = sqrt((x x + y y) + z z); d = raw / len (three divides).
 *   texel index       i = (face * size + y) * size + x.  Its radiance entry is { position, seed + i * 0x9E3779B9 (mod 2^32), d_i,
 *                     user = i }, traced with the call's `samples` and `bounces` under the rule of "radiance queries".
 *   resolve           rgb_linear = rgb * rgb per channel (as "light probes"); a = 1.0 where the texel's own ray hit
 *                     (BRT_QUERY_STATUS_HIT), 0.0 where it missed or was refused: a host composites its own skybox there.
 *   box level         a texel of the next smaller level (edge size / 2) is ((t00 + t01) + (t10 + t11)) * 0.25 per channel, alpha
 *                     included, t_yx the four texels it covers.  The edge of the larger level must be even.
 *   tap table         n_taps in [1, 4096] records of 16 bytes { f32 lx, ly, lz, w } in the tangent space of the lobe axis.
 *                     brt_host_envmap_taps is the only place that computes one: in float64, rounded once to f32.  For tap i:
 *                     xi1 = (i + 0.5) / n, xi2 = the base-2 radical inverse of i, phi = 2 pi xi1.
 *                     BRT_ENVMAP_TAPS_GGX, roughness in [0, 1]: a = roughness^2 (the f32 argument squared in float64); cos t = sqrt((1 -
 *                     xi2) / (1 + (a a - 1) xi2)); sin t = sqrt(max(0, 1 - cos t cos t)); h = (sin t cos phi, sin t sin phi, cos t);
 *                     l = (2 h.z h.x, 2 h.z h.y, 2 h.z h.z - 1); w = max(l.z, 0).
 *                     BRT_ENVMAP_TAPS_COSINE (roughness is not read): r = sqrt(xi2); l = (r cos phi, r sin phi, sqrt(1 - xi2)); w = 1.
 *                     The kernel takes the table as data and does no trigonometry; a caller may pass a table of its own.
 *   the filter rule   the source cube (edge src_size) -> the destination cube (edge dst_size).  Per destination texel:
 *                     1. N = the texel's direction (dst_size).
 *                     2. |N.z| < 0.999f: t = (-N.y, N.x, 0) [= (0, 0, 1) x N]; otherwise t = (0, -N.z, N.y) [= (1, 0, 0) x N].
 *                     3. T = t / sqrt((t.x t.x + t.y t.y) + t.z t.z) (three divides); B = N x T = (N.y T.z - N.z T.y, N.z T.x - N.x T.z,
 *                        N.x T.y - N.y T.x).
 *                     4. acc[4] = +0.0, sw = +0.0; the taps k = 0 .. n_taps - 1 in order; a tap with w <= 0 is skipped (a NaN w is not).
 *                     5. L = (lx * T + ly * B) + lz * N per component.
 *                     6. the face by the major axis, ties to X, then Y: ax >= ay && ax >= az: X (ma = ax; L.x < 0: face -X, sc = L.z,
 *                        else face +X, sc = -L.z; tc = -L.y); else ay >= az: Y (ma = ay; sc = L.x; L.y < 0: face -Y, tc = -L.z, else
 *                        face +Y, tc = L.z); else Z (ma = az; tc = -L.y; L.z < 0: face -Z, sc = -L.x, else face +Z, sc = L.x).
 *                     7. u = sc / ma, v = tc / ma.
 *                     8. with S = src_size: px = ((u + 1) * 0.5) * f32(S) - 0.5; px = px > 0 ? px : 0 (a NaN becomes 0); px = px <
 *                        f32(S - 1) ? px : f32(S - 1).
 *                     9. i0 = min(u32(floor(px)), max(S, 2) - 2); i1 = min(i0 + 1, S - 1); g = px - f32(i0).  The same for v -> j0, j1, gy.
 *                     10. inside that face: c = (c00 * (1 - gx) + c01 * gx) * (1 - gy) + (c10 * (1 - gx) + c11 * gx) * gy per channel,
 *                        c_ji the texel (x = i_i, y = j_j).
 *                     11. acc = acc + w * c for all four channels; sw = sw + w.
 *                     12. sw > 0: acc / sw; otherwise 0 in all four channels.
 *                     A NaN or INF texel propagates as the arithmetic says.  LIMITATION: a tap's four texels are taken inside the face
 *                     its direction falls on (clamped at the face's edge): taps do not filter across face edges.
 *   the chain         `levels` in [1, log2(size) + 1]; level l has edge size >> l.  The levels are concatenated, level 0 first, each a
 *                     cube: level l begins at texel offset(l) = sum over j < l of 6 * (size >> j)^2.  Level 0 is the resolved cube.
 *                     Box level 0 is level 0; box level l >= 1 is the box level of box level l - 1.  Level l >= 1 is the filter of box
 *                     level l at its own resolution (src_size = dst_size = size >> l) with the GGX table of roughness f32(l) / f32(levels
 *                     - 1) (an f32 divide) and the call's n_taps.
 *   brt_host_envmap_directions   host arithmetic, no context: out_xyz[3 i ..] = d_i for the 6 size^2 texels.  size in [1, 4096].
 *   brt_host_envmap_taps         host arithmetic, no context: the table of `kind` at `out` (16 n_taps bytes).
 *   brt_host_envmap_downsample   host arithmetic, no context: the box level of the cube at `src` (src_size even, in [2, 4096]).
 *   brt_host_envmap_filter       host arithmetic, no context: the filter rule; the compiled twin of the kernel.  Sizes in [1, 4096].
 *   brt_envmap_rays_device       the generation kernel alone: the 6 size^2 radiance entries of a cube at d_rays (DEVICE), size in [1, 4096].
 *   brt_envmap_resolve_device    the resolve kernel alone: 6 size^2 radiance results at d_results -> texels at d_out.  Needs no scene.
 *   brt_envmap_downsample_device the box-level kernel alone.  Needs no scene.
 *   brt_envmap_filter_device     the filter kernel alone (RGBA32F texels).  Needs no scene.  With a BRT_ENVMAP_TAPS_COSINE table over the
 *                     resolved cube (or a box level of it) the result is the diffuse map: the cosine-weighted mean radiance per direction.
 *   brt_bake_envmap_device       everything in one call: the texels in chunks of BRT_PROBE_CHUNK_RAYS entries (the light probes' tuning
 *                     knob), generate -> the radiance kernels -> resolve; then per level the box level and its filter.  d_out: DEVICE,
 *                     offset(levels) texels of 16 bytes, or of 8 bytes { f16 r, g, b, a } with BRT_FLAG_OUT_RGBA16F (every level is
 *                     computed in f32 and rounded to nearest even once, when it is written).  size: a power of two in [1, 1024];
 *                     samples, bounces, origin_bound: as for brt_radiance_rays.  The bytes written depend neither on the chunk size
 *                     nor on BRT_RADIANCE_FORM.  flags: BRT_FLAG_CALLER_STREAM, BRT_FLAG_OUT_RGBA16F.
 *   brt_bake_envmap              the same for a HOST buffer, synchronous.  flags: BRT_FLAG_OUT_RGBA16F only.
 *   out_stats8_or_null   as for brt_bake_probes: [0..2] walks, entries whose own ray hit, entries refused, summed over the chunks (only
 *                     calls that synchronise count), [3] the tree was rebuilt, [4] its reach, [5] the radiance form of the last chunk,
 *                     [6] chunks, [7] 0.
 * The step exports' flags: BRT_FLAG_CALLER_STREAM only; stream rule and ordering as for the step exports of "light probes".  Refused with
 * BRT_ERR_INVALID_ARGUMENT and nothing written: a non-finite position; a bake position whose 1-norm (|x| + |y|) + |z| exceeds the tree's
 * bound (brt_query_origin_bound) after the reach step of origin_bound; null pointers; a DEVICE buffer that is not 16-byte aligned; an
 * output that overlaps an input; a size, n_taps, kind, roughness, levels, samples or bounces out of range; unknown flags.  The bakes:
 * BRT_ERR_NO_SCENE before an upload, BRT_ERR_UNSUPPORTED under a set policy.  A refused call leaves the context usable; no call here
 * changes a frame or the dispatch history. */
#define BRT_ENVMAP_TAPS_GGX 0u
#define BRT_ENVMAP_TAPS_COSINE 1u
int32_t brt_host_envmap_directions(uint32_t size, float* out_xyz);
int32_t brt_host_envmap_taps(uint32_t kind, float roughness, uint32_t n_taps, void* out);
int32_t brt_host_envmap_downsample(const void* src, uint32_t src_size, void* out);
int32_t brt_host_envmap_filter(const void* src, uint32_t src_size, const void* taps, uint32_t n_taps, uint32_t dst_size, void* out);
int32_t brt_envmap_rays_device(brt_ctx* ctx, const float* position3, uint32_t seed, uint32_t size, void* d_rays, void* hip_stream,
                               uint32_t flags);
int32_t brt_envmap_resolve_device(brt_ctx* ctx, const void* d_results, uint32_t size, void* d_out, void* hip_stream, uint32_t flags);
int32_t brt_envmap_downsample_device(brt_ctx* ctx, const void* d_src, uint32_t src_size, void* d_out, void* hip_stream, uint32_t flags);
int32_t brt_envmap_filter_device(brt_ctx* ctx, const void* d_src, uint32_t src_size, const void* d_taps, uint32_t n_taps, uint32_t dst_size,
                                 void* d_out, void* hip_stream, uint32_t flags);
int32_t brt_bake_envmap_device(brt_ctx* ctx, const float* position3, uint32_t seed, uint32_t size, uint32_t levels, uint32_t samples,
                               uint32_t bounces, uint32_t n_taps, float origin_bound, void* d_out, void* hip_stream, uint32_t flags,
                               uint64_t* out_stats8_or_null);
int32_t brt_bake_envmap(brt_ctx* ctx, const float* position3, uint32_t seed, uint32_t size, uint32_t levels, uint32_t samples,
                        uint32_t bounces, uint32_t n_taps, float origin_bound, void* out, uint32_t flags, uint64_t* out_stats8_or_null);

/* ---- lightmaps --------------------------------------------------------------------------------------------------------------------------
 * What light arrives at points ON SURFACES: per point the rays of a fixed direction set over the cosine-weighted hemisphere of its normal
 * are traced as radiance entries, made linear and averaged into the texel of a chart, and the chart's edge is dilated so that the texture
 * holds under bilinear filtering -- the image of a level-1 / level-2 host's baked lighting (Bevy's `Lightmap { image, uv_rect }`).  On the
 * context's first device.  Rule, kernels and costs: DESIGN.md "Lightmaps".  Deterministic: f32, every operation separately rounded,
 * divide and sqrt correctly rounded, in the order written here; the default policy only.
 *   point, 32 bytes   { f32 position[3]; u32 seed; f32 normal[3]; f32 offset }, one per texel, row-major, width * height of them.  The
 *                     host rasterises its own UV charts into points; brt_host_lightmap_sphere_points gives one chart of one sphere.
 *                     EMPTY: the three normal words are all +0.0 / -0.0 (no chart covers the texel); not an error, and looked at first.
 *                     INVALID: len2 (below) is 0, INF or NaN; a position word is INF or NaN; offset is INF, NaN or < 0.
 *   direction table   n_dirs in [1, 65536]; for k = 0 .. n_dirs - 1: u = (k + 0.5) / n_dirs, r = sqrt(u), phi = 2 pi frac(k *
 *                     0.6180339887498949), l_k = (r cos phi, r sin phi, sqrt(1 - u)): cosine-weighted about +z, equal weights.
 *                     brt_host_lightmap_directions is the only place that computes it: in float64, rounded once to f32.
 *   frame             len2 = (nx nx + ny ny) + nz nz; len = sqrt(len2); n = (nx / len, ny / len, nz / len).  s = copysign(1, n.z);
 *                     a = -1 / (s + n.z); b = (n.x n.y) a; t = (1 + (s (n.x n.x)) a, s b, (-s) n.x); bt = (b, s + (n.y n.y) a, -n.y).
 *                     |s + n.z| >= 1 for a unit n: the basis is never singular.
 *   rays              o = position + offset * n per component (one multiply, one add); d_k = (l.x * t + l.y * bt) + l.z * n per
 *                     component.  Entry k of a point is the radiance entry { o, seed + k * 0x9E3779B9 (mod 2^32), d_k, user = k }, traced
 *                     with samples = 1 and the call's `bounces` under the rule of "radiance queries".  An EMPTY or INVALID point has the
 *                     position's words as o and 0x7fc00000 in the three direction words: the radiance kernels refuse such an entry
 *                     without a walk.  Lists are POINT-MAJOR: entry k of point p is record p * n_dirs + k.
 *   resolve           L = c * c per channel of an entry's colour (as "light probes").  Lane l of 64 sums its entries k = l, l + 64, ...
 *                     in order from +0.0; then for off = 32, 16, 8, 4, 2, 1: acc[l] = acc[l] + acc[l + off]; rgb = acc[0] / f32(n_dirs),
 *                     a = 1.0.  rgb is the MEAN LINEAR RADIANCE over the cosine-weighted hemisphere: the irradiance is pi * rgb.
 *   texel             RGBA32F (16 bytes), or RGBA16F (8 bytes) under BRT_FLAG_OUT_RGBA16F (round to nearest even, once, at the final
 *                     store).  a = 1.0 traced, 0.5 filled by dilation, 0.0 neither.
 *   info, 8 bytes     { u32 hits; u32 status }, an optional buffer.  hits: the point's entries whose own ray hit, so 1 - hits / n_dirs is
 *                     its openness to the sky.  status: entry 0's BRT_QUERY_STATUS_INVALID / BRT_QUERY_STATUS_OUT_OF_REACH bits (a point
 *                     beyond the tree's bound, brt_query_origin_bound), or BRT_LIGHTMAP_STATUS_EMPTY alone for an EMPTY point.  A point
 *                     with a status has rgb = 0, a = 0 and hits = 0.
 *   dilate            `passes` in [0, 64] passes over the f32 image, each from the image the pass before wrote.  A texel with a > 0 is
 *                     copied.  Any other visits its eight neighbours, dy = -1, 0, 1 outer and dx = -1, 0, 1 inner, the centre skipped;
 *                     wrap_u = 1: x wraps modulo width (the seam of a latitude-longitude chart), else a neighbour outside the image is
 *                     skipped, as one above or below it always is.  The neighbours with a > 0 in the pass's SOURCE add their rgb from
 *                     +0.0 in that order; count > 0: rgb = sum / f32(count), a = 0.5; else the texel is copied.  A NaN rgb propagates and
 *                     never changes coverage.
 *   brt_host_lightmap_directions     host arithmetic, no context: out_xyz[3 k ..] = l_k.
 *   brt_host_lightmap_ray            host arithmetic, no context: entry k (< n_dirs) of the point at point32 -> the 32-byte radiance entry
 *                     at out_ray32; the compiled twin of the generation kernel.
 *   brt_host_lightmap_sphere_points  host arithmetic, no context: the latitude-longitude chart of one sphere as width * height points.
 *                     Texel (x, y), i = y * width + x: phi = 2 pi (x + 0.5) / width about +Y, theta = pi (y + 0.5) / height from +Y;
 *                     normal = (sin theta cos phi, cos theta, sin theta sin phi); position = centre + radius * normal; in float64,
 *                     rounded once to f32; seed + i * 0x9E3779B9; `offset` as given.  A finite centre, radius > 0, offset >= 0.  This is
 *                     ONE parameterisation, for tests and demos: a host whose meshes carry other UVs supplies its own points.
 *   brt_host_lightmap_dilate         host arithmetic, no context: the passes over width * height RGBA32F texels -> out_f32; the compiled
 *                     twin of the dilation kernel.  The buffers need no alignment and must not overlap.
 *   brt_lightmap_rays_device         the generation kernel alone: n_points points at d_points -> n_points * n_dirs radiance entries at
 *                     d_rays (DEVICE), n_points * n_dirs <= 0x7fff0000.  Needs no scene.
 *   brt_lightmap_resolve_device      the resolve kernel alone, on any list of radiance results in that layout and its points -> n_points
 *                     texels at d_out and, if not null, info records at d_info_or_null.  Needs no scene.  flags: BRT_FLAG_CALLER_STREAM,
 *                     BRT_FLAG_OUT_RGBA16F.
 *   brt_lightmap_dilate_device       the passes alone: the RGBA32F image at d_texels_f32 -> d_out; passes = 0 copies (and converts).  The
 *                     images between the passes are the context's.  Needs no scene.  flags: BRT_FLAG_CALLER_STREAM, BRT_FLAG_OUT_RGBA16F.
 *   brt_bake_lightmap_device         everything in one call on DEVICE buffers: in chunks of whole points, generate -> the radiance kernels
 *                     -> resolve into an f32 image of the context; after the last chunk the passes into d_out.  A chunk is max(1,
 *                     BRT_PROBE_CHUNK_RAYS / n_dirs) points (the light probes' tuning knob).  The bytes written depend neither on the
 *                     chunk size nor on BRT_RADIANCE_FORM.  bounces, origin_bound: as for brt_radiance_rays.  flags:
 *                     BRT_FLAG_CALLER_STREAM, BRT_FLAG_OUT_RGBA16F.
 *   brt_bake_lightmap                the same for HOST buffers, synchronous.  flags: BRT_FLAG_OUT_RGBA16F only.
 *   out_stats8_or_null   as for brt_bake_probes: [0..2] walks, entries whose own ray hit, entries refused, summed over the chunks (only
 *                     calls that synchronise count), [3] the tree was rebuilt, [4] its reach, [5] the radiance form of the last chunk,
 *                     [6] chunks, [7] 0.
 * The rays export's flags: BRT_FLAG_CALLER_STREAM only; stream rule and ordering as for the step exports of "light probes".  Refused with
 * BRT_ERR_INVALID_ARGUMENT and nothing written: null pointers (but d_info_or_null); a DEVICE buffer that is not 16-byte aligned; buffers
 * that overlap; n_dirs outside [1, 65536]; k >= n_dirs; bounces above 65535; a bad origin_bound; width or height of 0 or above 16384;
 * passes above 64; wrap_u above 1; n_points * n_dirs above 0x7fff0000; unknown flags.  The bakes: BRT_ERR_NO_SCENE before an upload,
 * BRT_ERR_UNSUPPORTED under a set policy.  n_points = 0 is BRT_OK for the rays and resolve exports.  A refused call leaves the context
 * usable; no call here changes a frame or the dispatch history. */
#define BRT_LIGHTMAP_STATUS_EMPTY 16u
int32_t brt_host_lightmap_directions(uint32_t n_dirs, float* out_xyz);
int32_t brt_host_lightmap_ray(const void* point32, uint32_t n_dirs, uint32_t k, void* out_ray32);
int32_t brt_host_lightmap_sphere_points(const float* centre3, float radius, uint32_t seed, float offset, uint32_t width, uint32_t height,
                                        void* out_points);
int32_t brt_host_lightmap_dilate(const void* texels_f32, uint32_t width, uint32_t height, uint32_t passes, uint32_t wrap_u, void* out_f32);
int32_t brt_lightmap_rays_device(brt_ctx* ctx, const void* d_points, uint32_t n_points, uint32_t n_dirs, void* d_rays, void* hip_stream,
                                 uint32_t flags);
int32_t brt_lightmap_resolve_device(brt_ctx* ctx, const void* d_results, const void* d_points, uint32_t n_points, uint32_t n_dirs,
                                    void* d_out, void* d_info_or_null, void* hip_stream, uint32_t flags);
int32_t brt_lightmap_dilate_device(brt_ctx* ctx, const void* d_texels_f32, uint32_t width, uint32_t height, uint32_t passes,
                                   uint32_t wrap_u, void* d_out, void* hip_stream, uint32_t flags);
int32_t brt_bake_lightmap_device(brt_ctx* ctx, const void* d_points, uint32_t width, uint32_t height, uint32_t n_dirs, uint32_t bounces,
                                 uint32_t passes, uint32_t wrap_u, float origin_bound, void* d_out, void* d_info_or_null, void* hip_stream,
                                 uint32_t flags, uint64_t* out_stats8_or_null);
int32_t brt_bake_lightmap(brt_ctx* ctx, const void* points, uint32_t width, uint32_t height, uint32_t n_dirs, uint32_t bounces,
                          uint32_t passes, uint32_t wrap_u, float origin_bound, void* out, void* info_or_null, uint32_t flags,
                          uint64_t* out_stats8_or_null);

/* ---- guide-buffer upsampling ----------------------------------------------------------------------------------------------------------
 * A frame traced at low_width x low_height is presented at width x height: every OUTPUT pixel casts its own pixel-centre ray (the guide
 * buffer's), so sphere silhouettes, the first bounce's base colour and the sky are at full sharpness, and gathers the demodulated colour
 * of the low frame's taps that lie on the same material, weighted bilinearly and by the denoiser's normal and depth terms (sigma_normal,
 * sigma_depth of brt_set_denoise).  Rule, kernel and costs: DESIGN.md "Guide-buffer upsampling".  Deterministic.  Pure (level 3) frames
 * only: neither call takes a level -- levels 1 / 2 go through the two calls of "upsampling blended frames" below.
 * Sizes, per axis: 1 <= low <= full <= 32768 and full <= 4 x low; else BRT_ERR_INVALID_ARGUMENT.  camera80: the frame's camera, the same
 * for both sizes.  BRT_ERR_NO_SCENE before an upload.
 *   brt_upscale_device          upsamples an RGBA f32 low_width x low_height DEVICE frame the caller holds -- a Pure frame of any entry
 *                               point (the root's frame after brt_gather_rccl), denoised / accumulated or not, rendered with camera80 on
 *                               the resident scene and the window of brt_host_upscale_window -- into d_out (DEVICE, width x height in the
 *                               BRT_FLAG_OUT_* format of `flags`; it must not overlap d_low_rgba).  window16: the full-size or the low
 *                               window (only pixel-centre rays are cast: its height is not read).  flags: BRT_FLAG_CALLER_STREAM,
 *                               BRT_FLAG_OUT_*; other bits BRT_ERR_INVALID_ARGUMENT.  Stream rule and stats (total_ms only) as for
 *                               brt_denoise_device; the call shares the denoiser's scratch and runs one behind another with the context's
 *                               denoise / temporal calls on whatever streams they come.
 *   brt_render_upscaled_device  trace, post-passes and upsampling in one call.  The low frame is exactly the low_width x low_height Pure
 *                               frame of brt_render_device (every device of the context) with the same camera and the window of
 *                               brt_host_upscale_window(window16, height, low_height); it stays in the context.  With BRT_FLAG_DENOISE
 *                               and / or BRT_FLAG_TEMPORAL the post-passes run on the LOW frame (the temporal history is that of the low
 *                               size) and the upsampling comes last.  d_frame: DEVICE, width x height in the BRT_FLAG_OUT_* format of
 *                               `flags`.  flags: BRT_FLAG_CALLER_STREAM, BRT_FLAG_OUT_*, BRT_FLAG_DENOISE, BRT_FLAG_TEMPORAL; other bits
 *                               BRT_ERR_INVALID_ARGUMENT.  Stream rule as for brt_render_device; stats_or_null as brt_render_device
 *                               fills them for the low frame, total_ms for the whole call.
 *   brt_host_upscale_window     host arithmetic, no context: out_window16 = window16 with height = max(1, window.height * low_height /
 *                               height) in integer arithmetic -- the window a low frame is traced with (the reference sizes the jitter
 *                               of a sample by window.height, raytrace.wgsl:139-147).  1 <= low_height <= height, else
 *                               BRT_ERR_INVALID_ARGUMENT. */
int32_t brt_upscale_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t low_width, uint32_t low_height,
                           const float* d_low_rgba, uint32_t width, uint32_t height, void* d_out, void* hip_stream, uint32_t flags,
                           brt_stats* stats_or_null);
int32_t brt_render_upscaled_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t low_width, uint32_t low_height,
                                   uint32_t width, uint32_t height, void* d_frame, void* hip_stream, uint32_t flags,
                                   brt_stats* stats_or_null);
int32_t brt_host_upscale_window(const void* window16, uint32_t height, uint32_t low_height, void* out_window16);

/* ---- upsampling blended frames (levels 1 / 2) -----------------------------------------------------------------------------------------
 * The two upsampling calls with a level and the FULL-SIZE raster inputs: the host traces low and presents a frame of the shipping level.
 * The low frame stays a Pure frame (the colour of a ray-traced pixel does not depend on the level); the raster blend of the reference
 * (raytrace.wgsl:104-120) is decided per OUTPUT pixel p by the upsampling kernel, which holds the distance t_p of p's centre ray:
 *   depth = t_p, or on a miss far + 10 at level 1 and far - 1 at level 2;  rd = depth > far ? -1 : near / depth;
 *   p is covered iff d_raster_depth[p] > rd   (f32, each operation rounded; a null depth reads as 0, a NaN depth never covers).
 * A covered pixel is the raster texel of its own index, all four channels (a null colour reads as zeros), in the BRT_FLAG_OUT_* format; any
 * other pixel is bit for bit what the call without a level stores.  Rule, kernel, costs: DESIGN.md "Upsampling blended frames".
 * level: 3 is exactly the call without a level (the raster inputs are not read); 0 BRT_ERR_UNSUPPORTED; others BRT_ERR_INVALID_ARGUMENT.
 * d_raster_rgba_or_null (RGBA f32) / d_raster_depth_or_null (reverse-Z f32): DEVICE, width x height, on the context's first device; the
 * output must overlap neither (BRT_ERR_INVALID_ARGUMENT).  Sizes, flags, stream rule, stats, scratch and ordering: those of the call
 * without a level.
 *   brt_upscale_blend_device          brt_upscale_device; d_low_rgba is a PURE low frame of any entry point.
 *   brt_render_upscaled_blend_device  brt_render_upscaled_device: the low frame is traced at level 3 on every device of the context -- no
 *                                     raster input is forwarded to another device -- and BRT_FLAG_DENOISE / BRT_FLAG_TEMPORAL run on it
 *                                     with the low size's history.
 *   brt_host_blend_covered            host arithmetic, no context: the rule above for one (t, raster_depth) pair, t = +INF meaning a miss,
 *                                     into *out_covered (0 / 1; always 0 at level 3).  Lets a host predict the seam. */
int32_t brt_upscale_blend_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t level, uint32_t low_width,
                                 uint32_t low_height, const float* d_low_rgba, uint32_t width, uint32_t height,
                                 const float* d_raster_rgba_or_null, const float* d_raster_depth_or_null, void* d_out, void* hip_stream,
                                 uint32_t flags, brt_stats* stats_or_null);
int32_t brt_render_upscaled_blend_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t level, uint32_t low_width,
                                         uint32_t low_height, uint32_t width, uint32_t height, const float* d_raster_rgba_or_null,
                                         const float* d_raster_depth_or_null, void* d_frame, void* hip_stream, uint32_t flags,
                                         brt_stats* stats_or_null);
int32_t brt_host_blend_covered(const void* camera80, uint32_t level, float t, float raster_depth, uint32_t* out_covered);

/* ---- sparse pixel tracer ----------------------------------------------------------------------------------------------------------------
 * Traces SOME pixels of a Pure (level 3) frame.  A list entry is p = py * width + px (uint32); for entry i the call computes the value
 * {rgb, 1} that brt_render_device stores at pixel p for the same camera, window, width, height and resident scene, bit for bit: the seed
 * of a pixel depends on its frame coordinates alone.  The output is packed: entry i goes to out[i] (RGBA f32).  A pixel may be named any
 * number of times.  Kernel forms and costs: DESIGN.md "Refined upsampling".
 *   brt_render_pixels_device  d_pixels / d_out_rgba32f: DEVICE buffers of n_pixels entries on the first device (the whole pass runs there,
 *                             whatever the number of devices of the context).  flags: BRT_FLAG_CALLER_STREAM, and BRT_FLAG_KERNEL_SIMPLE
 *                             (the one-thread-per-entry form instead of the persistent one; the bytes are the same); other bits
 *                             BRT_ERR_INVALID_ARGUMENT.  Stream rule and tree reach as for brt_render_device.  Lists of one context run
 *                             one behind the other, and behind its ray queries, on whatever streams they come.
 *   brt_render_pixels         the same for HOST buffers, synchronous.  flags: BRT_FLAG_KERNEL_SIMPLE only.
 *   stats_or_null             rays, paths (entries traced x sample_count), reserved (= entries refused), total_ms, the tree fields, and the
 *                             launch (lds_bytes, scene_in_lds, n_workgroups, threads_per_workgroup; kernel_variant 32: the persistent
 *                             form, 33: the plain form).  rays, paths and reserved only where the call synchronises (the own stream,
 *                             brt_render_pixels); 0 on a caller's stream.
 * Refusals: n_pixels = 0 is BRT_OK and writes nothing.  An entry >= width * height is never traced: it stores four zeros and is counted
 * as refused.  A non-default policy (brt_set_policy): BRT_ERR_UNSUPPORTED, as for the bring-up kernel.  Orthographic projection
 * BRT_ERR_UNSUPPORTED, BRT_ERR_NO_SCENE before an upload, null pointers and sizes outside [1, 32768] BRT_ERR_INVALID_ARGUMENT.  A refused
 * call leaves the context usable. */
int32_t brt_render_pixels_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height,
                                 const uint32_t* d_pixels, uint32_t n_pixels, float* d_out_rgba32f, void* hip_stream, uint32_t flags,
                                 brt_stats* stats_or_null);
int32_t brt_render_pixels(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height, const uint32_t* pixels,
                          uint32_t n_pixels, float* out_rgba32f, uint32_t flags, brt_stats* stats_or_null);

/* ---- lens frames: depth of field and orthographic projection ----------------------------------------------------------------------------
 * Pure (level 3) frames and pixel lists whose primary rays come from a thin lens or an orthographic camera instead of the pinhole.  Only
 * ray generation differs: the seed of a pixel (raytrace.wgsl:95), the RNG state its samples share, raytrace() at level 3 and the average
 * (raytrace.wgsl:161-171, alpha 1) are the Pure frame's.  On the context's first device, by the kernels of the sparse pixel tracer with
 * another sample start.  Rule (csrc/brt_lens.h holds the operation order), kernels and costs: DESIGN.md "Lens frames".
 *   brt_lens, 32 bytes   { aperture_radius, focus_distance, ortho_height, reserved[5] }; the reserved words must be 0.  The entry
 *                        points take it as lens32, 32 bytes at any address, like the camera and the window.
 *   the rule, per sample 1. the two jitter draws and ndc_x, ndc_y as in the Pure frame; v = (direction + sx * right) + sy * up as there.
 *                        2. perspective (camera.projection_type 0), aperture_radius == 0: origin = position, direction = normalize(v); no
 *                           further draw: the frame is the Pure frame of brt_render_device bit for bit.
 *                        3. perspective, aperture_radius r > 0: a point (x, y) of the unit disk by rejection (x = 2 u1 - 1, y = 2 u2 - 1,
 *                           draws in that order, accepted when x * x + y * y <= 1.0); l = (r * x) * right + (r * y) * up; origin =
 *                           position + l, direction = normalize(focus_distance * v - l).  All rays of one jitter draw meet in one point
 *                           of the plane at focus_distance along camera.direction; what lies there is sharp.
 *                        4. orthographic (camera.projection_type 1): half = 0.5 * ortho_height; origin = (position + ((ndc_x * aspect) *
 *                           half) * right) + (ndc_y * half) * up, direction = normalize(camera.direction).  ortho_height is the height
 *                           of the view volume in units of |up| (aspect * ortho_height its width in units of |right|); fov, near and far
 *                           are not read; aperture_radius must be 0.
 *   brt_render_lens_device   the whole width x height frame into d_frame (DEVICE) in the store format of BRT_FLAG_OUT_*.  flags:
 *                            BRT_FLAG_OUT_*, BRT_FLAG_CALLER_STREAM, BRT_FLAG_KERNEL_SIMPLE (the one-thread-per-pixel form; the bytes are the
 *                            same).  Stream rule as for brt_render_device; lens calls run one behind the other with the context's pixel
 *                            lists and queries, on whatever streams they come.
 *   brt_render_lens          the same into a HOST buffer of RGBA f32, synchronous.  flags: BRT_FLAG_KERNEL_SIMPLE only.
 *   brt_render_lens_pixels_device / brt_render_lens_pixels   the list form, with the conventions of brt_render_pixels*: entry i is pixel
 *                            p = py * width + px, its value goes to out[i] (RGBA f32); an entry >= width * height is not traced, stores
 *                            four zeros and is counted in stats.reserved; n_pixels = 0 is BRT_OK.
 *   stats_or_null            as for brt_render_pixels* (kernel_variant 34: the persistent form, 35: the plain form).
 *   tree reach               the call first settles the tree for the camera, as every render call does; with aperture_radius > 0 or an
 *                            orthographic camera it then raises a callee-built tree's reach, if needed, to what origins within
 *                            brt_host_lens_origin_bound need -- as brt_query_rays does for its origin_bound, and with the same side
 *                            effect: later frames are traced on that tree until the next upload (stats.tree_rebuilt reports a rebuild).
 *   brt_host_lens_seed       host arithmetic, no context: the seed of pixel (px, py) of a width x height frame.
 *   brt_host_lens_ray        host arithmetic, no context: the rule for ONE sample of that pixel on the RNG state *state_inout, which it
 *                            advances as the kernel does (start from brt_host_lens_seed; the state after a sample's raytrace() is the next
 *                            sample's).  o3 / d3 receive origin and direction.
 *   brt_host_lens_origin_bound  host arithmetic: *out = a 1-norm that no origin of the rule exceeds for this camera and lens, whatever the
 *                            window (of at least one row) and the frame size, rounding included (+INF: there is none).
 * Refusals: BRT_ERR_INVALID_ARGUMENT for a null pointer, non-zero reserved words, an aperture_radius that is NaN, negative or infinite, a
 * focus_distance that is not finite and > 0 while the radius is > 0, an ortho_height that is not finite and > 0 or a window height of 0
 * for an orthographic camera, a radius > 0 on an orthographic camera, projection_type > 1, sizes outside [1, 32768], any other flag --
 * the post-passes BRT_FLAG_DENOISE / BRT_FLAG_TEMPORAL / BRT_FLAG_BLEND_POST included: their guide buffers assume pinhole rays.
 * BRT_ERR_UNSUPPORTED for a non-default policy (brt_set_policy) and for an origin bound that is not finite or that the callee's tree
 * cannot be raised to cover.  BRT_ERR_NO_SCENE before an upload.  brt_last_error names the field.  A refused call leaves the context
 * usable.  Every other entry point keeps answering BRT_ERR_UNSUPPORTED for an orthographic camera. */
typedef struct brt_lens {
    float aperture_radius;     /* radius of the lens disk in units of |right| / |up|; 0: a pinhole */
    float focus_distance;      /* distance of the focus plane along camera.direction, in units of |direction| (read when the radius is > 0) */
    float ortho_height;        /* orthographic cameras: height of the view volume in units of |up| */
    uint32_t reserved[5];      /* must be 0 */
} brt_lens;
int32_t brt_render_lens_device(brt_ctx* ctx, const void* camera80, const void* window16, const void* lens32, uint32_t width,
                               uint32_t height, void* d_frame, void* hip_stream, uint32_t flags, brt_stats* stats_or_null);
int32_t brt_render_lens(brt_ctx* ctx, const void* camera80, const void* window16, const void* lens32, uint32_t width, uint32_t height,
                        float* out_rgba32f, uint32_t flags, brt_stats* stats_or_null);
int32_t brt_render_lens_pixels_device(brt_ctx* ctx, const void* camera80, const void* window16, const void* lens32, uint32_t width,
                                      uint32_t height, const uint32_t* d_pixels, uint32_t n_pixels, float* d_out_rgba32f, void* hip_stream,
                                      uint32_t flags, brt_stats* stats_or_null);
int32_t brt_render_lens_pixels(brt_ctx* ctx, const void* camera80, const void* window16, const void* lens32, uint32_t width,
                               uint32_t height, const uint32_t* pixels, uint32_t n_pixels, float* out_rgba32f, uint32_t flags,
                               brt_stats* stats_or_null);
int32_t brt_host_lens_seed(const void* window16, uint32_t width, uint32_t height, uint32_t px, uint32_t py, uint32_t* out_seed);
int32_t brt_host_lens_ray(const void* camera80, const void* window16, const void* lens32, uint32_t width, uint32_t height, uint32_t px,
                          uint32_t py, uint32_t* state_inout, float* o3, float* d3);
int32_t brt_host_lens_origin_bound(const void* camera80, const void* lens32, float* out_bound);

/* ---- G-buffer: depth, normal, motion vectors, ids and albedo of a frame ------------------------------------------------------------------
 * The attributes of the first hit of every pixel-centre ray of a width x height frame -- the hit the denoiser, the temporal pass and the
 * upsampling work on -- in the layouts a render node hands on: one kernel, one walk per pixel, every requested plane written from its
 * registers.  On the context's first device.  Rule (csrc/brt_gbuffer.h holds the operation order), kernel and costs: DESIGN.md "G-buffer".
 *   the ray      uv = (p + 0.5) / size, direction = the camera's pixel-centre direction, origin = camera.position: brt_host_pixel_ray's.
 *   the hit      the reference's raycast on the resident scene: t, the sphere, n = normalize(ray_at(t) - centre), not flipped.
 *   brt_gbuffer, 32 bytes  { depth_mode, normal_format, motion_format, reserved[5] }; the reserved words must be 0.
 *   depth        one f32.  BRT_GBUFFER_DEPTH_VIEW: near / (t * dot(d, normalize(direction))), a miss +0.0 -- reverse-Z planar depth, what an
 *                infinite reverse-Z depth prepass holds.  BRT_GBUFFER_DEPTH_SHADER: the reference's own compare value for the centre ray
 *                (raytrace.wgsl:108-113): t > far ? -1.0 : near / t; a miss: the same test on fallback_far = far - 1 (the level that keeps
 *                the traced sky; level 1's far + 10 always gives -1.0, which the HIT bit lets a host substitute).
 *                BRT_GBUFFER_DEPTH_DISTANCE: t, a miss +INF.
 *   normal       world space.  BRT_GBUFFER_NORMAL_RGBA32F: four f32 {n, 1}.  BRT_GBUFFER_NORMAL_RGB10A2: one u32 in the layout of an
 *                Rgb10a2Unorm texel: channel = u32(floor(clamp(n * 0.5 + 0.5, 0, 1) * 1023 + 0.5)) (a NaN: 0), R in the low bits, alpha 3.
 *                A miss: zeros.
 *   ids          four u32 { sphere, material, status, 0 }: sphere is the index into the models of the last upload; status is
 *                BRT_GBUFFER_STATUS_* bits.  A miss: sphere = material = BRT_QUERY_NONE.
 *   albedo       four f32: the first four words of the hit's material (base_color.rgb, metallic), bit for bit.  A miss: zeros.
 *   motion       the previous pixel position (x', y') of the hit point: carried back through its sphere's motion (d_prev_models: the
 *                previous frame's models, 32 bytes each, in the caller's order and of the same count; null: nothing moved; a sphere has
 *                MOVED iff its {centre, radius * radius} differ bitwise) and projected into prev_camera80 (null: the current camera) by
 *                the temporal pass's expressions.  A miss is carried by the camera's rotation alone.  The previous camera bitwise the
 *                current one and the sphere not moved: (x', y') = (px, py) exactly.  z <= 0 or a position outside (-1, W) x (-1, H):
 *                BRT_GBUFFER_STATUS_NO_PREVIOUS.  BRT_GBUFFER_MOTION_UV32F: two f32 uv - uv_prev, uv_prev = ((x' + 0.5) / W,
 *                (y' + 0.5) / H) -- current minus previous in uv units, y down; (0, 0) under NO_PREVIOUS.  BRT_GBUFFER_MOTION_UV16F: the
 *                same pair as two f16 (round to nearest even), x in the low half of one u32.  BRT_GBUFFER_MOTION_PIXEL: two f32 (x', y'),
 *                NaN under NO_PREVIOUS: where a host fetches its history.
 *   coverage     d_coverage_rgba_or_null: the assembled level-1 / 2 coverage frame brt_blend_post_device takes.  A pixel whose alpha is
 *                exactly +0.0 casts no ray and NONE of its planes is written.
 *   brt_render_gbuffer_device  DEVICE buffers (16-byte aligned) of width * height entries; every plane pointer may be null (not produced;
 *                all null is BRT_OK and launches nothing).  flags: BRT_FLAG_CALLER_STREAM only; stream rule as for brt_query_rays_device,
 *                and G-buffer calls run one behind the other with the context's queries and lists.  out_stats8_or_null: [0] pixels cast,
 *                [1] hits, [2] covered, [3] tree rebuilt, [4] the callee-built tree's reach (f32 bits), [5] moved, [6] no-previous, [7] 0;
 *                the counts are filled only by calls that synchronise (the context's own stream).
 *   brt_render_gbuffer         the same for HOST buffers, synchronous; with a coverage frame the planes are read as well as written.
 *   brt_host_gbuffer_pixel     host arithmetic, no context: the rule for pixel (px, py) whose ray hits at t (+INF: a miss) the sphere
 *                {centre, radius * radius} = sphere_new4, which was sphere_old4_or_null (null: not moved) in the previous frame.
 *                out_pixel64 receives a brt_gbuffer_pixel: the depth of depth_mode, the normal in both formats, the two motion words of
 *                motion_format, (x', y'), the status bits (HIT, FRONT_FACE, MOVED, NO_PREVIOUS) and the ray's direction.
 * The call keeps no state: no frame, dispatch history, temporal history or denoiser scratch changes.
 * Refusals: BRT_ERR_INVALID_ARGUMENT for a null camera, window or descriptor, non-zero reserved words, an unknown mode or format, sizes
 * outside [1, 32768], any other flag, a misaligned device buffer, a pixel outside the frame.  BRT_ERR_UNSUPPORTED for projection_type 1
 * (either camera) and for a non-default policy.  BRT_ERR_NO_SCENE before an upload.  brt_last_error names the field. */
#define BRT_GBUFFER_DEPTH_VIEW 0u
#define BRT_GBUFFER_DEPTH_SHADER 1u
#define BRT_GBUFFER_DEPTH_DISTANCE 2u
#define BRT_GBUFFER_NORMAL_RGBA32F 0u
#define BRT_GBUFFER_NORMAL_RGB10A2 1u
#define BRT_GBUFFER_MOTION_UV32F 0u
#define BRT_GBUFFER_MOTION_UV16F 1u
#define BRT_GBUFFER_MOTION_PIXEL 2u
#define BRT_GBUFFER_STATUS_HIT 1u
#define BRT_GBUFFER_STATUS_FRONT_FACE 2u
#define BRT_GBUFFER_STATUS_MOVED 4u
#define BRT_GBUFFER_STATUS_NO_PREVIOUS 8u
typedef struct brt_gbuffer {
    uint32_t depth_mode;       /* BRT_GBUFFER_DEPTH_* */
    uint32_t normal_format;    /* BRT_GBUFFER_NORMAL_* */
    uint32_t motion_format;    /* BRT_GBUFFER_MOTION_* */
    uint32_t reserved[5];      /* must be 0 */
} brt_gbuffer;
typedef struct brt_gbuffer_pixel {      /* 64 bytes: what brt_host_gbuffer_pixel returns */
    float depth;
    uint32_t status;
    uint32_t normal_rgb10a2;
    uint32_t reserved0;
    float normal[4];
    uint32_t motion[2];        /* the motion plane's words in motion_format (UV16F: one word, then 0) */
    float xy_prev[2];
    float direction[3];
    uint32_t reserved1;
} brt_gbuffer_pixel;
int32_t brt_render_gbuffer_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height,
                                  const void* gbuffer32, const void* prev_camera80_or_null, const void* d_prev_models_or_null,
                                  const float* d_coverage_rgba_or_null, void* d_depth, void* d_normal, void* d_motion, void* d_ids,
                                  void* d_albedo, void* hip_stream, uint32_t flags, uint64_t* out_stats8_or_null);
int32_t brt_render_gbuffer(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height, const void* gbuffer32,
                           const void* prev_camera80_or_null, const void* prev_models_or_null, const float* coverage_rgba_or_null,
                           void* depth, void* normal, void* motion, void* ids, void* albedo, uint64_t* out_stats8_or_null);
int32_t brt_host_gbuffer_pixel(const void* camera80, const void* window16, uint32_t width, uint32_t height, uint32_t px, uint32_t py,
                               const void* gbuffer32, const void* prev_camera80_or_null, float t, const float* sphere_new4,
                               const float* sphere_old4_or_null, void* out_pixel64);

/* ---- refined upsampling ---------------------------------------------------------------------------------------------------------------
 * The guide-buffer upsampling with the pixels it cannot reconstruct traced at FULL size by the sparse pixel tracer.  An output pixel p
 * whose own guide is a hit has the classes
 *   BRT_REFINE_EDGES     no tap of p's 2x2 footprint is eligible (p would be gathered by stage B or C: thin spheres, silhouettes);
 *   BRT_REFINE_SPECULAR  p's material has metallic > 0 or specular_transmission > 0 (what makes its image lies behind the first hit).
 * p is SELECTED under `classes` (a mask of these, 1 .. 3) iff it has one of them; sky pixels never are.  A selected pixel holds exactly
 * the full-size Pure frame's value there (brt_render_device with the full-size window), any other pixel exactly what brt_upscale_device
 * stores, both in the BRT_FLAG_OUT_* format.  Pure frames only.  Rule, kernels, costs and quality: DESIGN.md "Refined upsampling".
 * Sizes and BRT_ERR_NO_SCENE as for brt_upscale_device; `classes` 0 or above 3 BRT_ERR_INVALID_ARGUMENT; a non-default policy
 * (brt_set_policy) BRT_ERR_UNSUPPORTED.  Everything runs on the first device and on the call's stream, one behind another with the context's
 * denoise / upsampling calls, pixel lists and ray queries.
 *   brt_upscale_refine_device           brt_upscale_device for a low frame the caller holds.  window16 must be the FULL-SIZE window: its
 *                                       height sizes the jitter of the refined pixels' samples.  d_refined_count_or_null: a DEVICE word
 *                                       that receives the number of selected pixels.  flags: BRT_FLAG_CALLER_STREAM, BRT_FLAG_OUT_*.
 *                                       stats_or_null: total_ms and the tree fields.
 *   brt_render_upscaled_refined_device  the one-call form: the low trace of brt_render_upscaled_device, then the above.  BRT_FLAG_DENOISE /
 *                                       BRT_FLAG_TEMPORAL are BRT_ERR_INVALID_ARGUMENT here: refined pixels are raw samples and would sit
 *                                       unfiltered among filtered ones.  stats_or_null as brt_render_upscaled_device.
 *   brt_upscale_refine_mask_device      the class bits of every output pixel into d_mask_u8 (DEVICE, width x height bytes; 0 for the sky);
 *                                       traces nothing: what a refinement would cost.  flags: BRT_FLAG_CALLER_STREAM only. */
#define BRT_REFINE_EDGES 1u
#define BRT_REFINE_SPECULAR 2u
int32_t brt_upscale_refine_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t low_width, uint32_t low_height,
                                  const float* d_low_rgba, uint32_t width, uint32_t height, void* d_out, uint32_t classes,
                                  uint32_t* d_refined_count_or_null, void* hip_stream, uint32_t flags, brt_stats* stats_or_null);
int32_t brt_render_upscaled_refined_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t low_width,
                                           uint32_t low_height, uint32_t width, uint32_t height, void* d_frame, uint32_t classes,
                                           uint32_t* d_refined_count_or_null, void* hip_stream, uint32_t flags, brt_stats* stats_or_null);
int32_t brt_upscale_refine_mask_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t low_width, uint32_t low_height,
                                       const float* d_low_rgba, uint32_t width, uint32_t height, void* d_mask_u8, void* hip_stream,
                                       uint32_t flags);

/* ---- adaptive sampling -----------------------------------------------------------------------------------------------------------------
 * A Pure (level 3) frame whose pixels get the camera's sample_count only where a noise estimate asks for it: a BASE frame B is traced at
 * base_spp samples per pixel (otherwise the call's camera and window), a rule selects pixels from B and the full-size guides
 * G0 = {n, t}, G1 = {a, id} of the denoiser, and the sparse pixel tracer traces the selected pixels again with the call's own camera.  A
 * pixel's samples share one RNG state and the sample count enters only the final division, so a selected pixel holds exactly what
 * brt_render_device stores there at the camera's sample_count, and any other pixel exactly the base frame's value, both in the
 * BRT_FLAG_OUT_* format, alpha 1.  The rule, for output pixel p, every operation a separately rounded f32 one:
 *   l(c) = (0.2126 r + 0.7152 g) + 0.0722 b.  p has no class if it is sky (t = +INF) or l(B_p) is not finite.
 *   taps q: the 5x5 window around p, dy outer and dx inner, both -2 .. 2, p included; a tap counts iff it is inside the frame,
 *   id_q == id_p and l(B_q) is finite.  n = the number of taps, S1 = sum l_q and S2 = sum l_q * l_q in f32 in that order.
 *   BRT_ADAPT_SPARSE  iff n < min_taps (silhouettes, thin spheres: no estimate is possible);
 *   BRT_ADAPT_NOISY   else iff v > thr * thr, with m = S1 / n, v = max(0, S2 / n - m * m), thr = threshold * max(m, 0.01)
 *                     (max(a, b) = a > b ? a : b).
 * A pixel with a class is SELECTED.  Kernel, costs and quality: DESIGN.md "Adaptive sampling".
 *   brt_set_adaptive            base_spp in [1, 65535] (default 8), threshold finite and > 0 (default 0.025), min_taps in [1, 25] (default
 *                               6); anything else BRT_ERR_INVALID_ARGUMENT and the settings stay as they were.
 *   brt_render_adaptive_device  the one-call form, on the call's stream: the base trace by the persistent kernel (every device of the
 *                               context, as brt_render_device), then on the first device the guides, the selection and the re-trace.
 *                               d_selected_count_or_null: a DEVICE word that receives the number of selected pixels.  base_spp >=
 *                               the camera's sample_count: the plain frame is stored, nothing is selected, the count is 0.
 *                               stats_or_null as brt_render_device for the base trace; where the call synchronises (its own stream)
 *                               rays is base plus re-trace.
 *   brt_adaptive_refine_device  the same for a base frame the caller holds (RGBA f32, width x height, on the first device), which d_out
 *                               must not overlap.  stats_or_null: rays of the re-trace (own stream), total_ms and the tree fields.
 *   brt_adaptive_mask_device    the class byte of every pixel into d_mask_u8 (DEVICE, width x height bytes); traces nothing: what a frame
 *                               would cost.  flags: BRT_FLAG_CALLER_STREAM only.
 *   brt_host_adaptive_class     the rule for ONE pixel on the host, the code the kernel compiles: its t, material id and base colour,
 *                               and its 25 taps in the rule's order (inside the frame or not, material id, base colour rgb).
 * flags: BRT_FLAG_CALLER_STREAM and BRT_FLAG_OUT_*; any other bit is BRT_ERR_INVALID_ARGUMENT -- BRT_FLAG_DENOISE / BRT_FLAG_TEMPORAL
 * included: pixels of two sample counts sit side by side, and the denoiser's strength is set by one.  A non-default policy
 * (brt_set_policy) and orthographic projection: BRT_ERR_UNSUPPORTED; BRT_ERR_NO_SCENE before an upload; sizes outside [1, 32768] and null
 * pointers BRT_ERR_INVALID_ARGUMENT.  A refused call leaves the context usable.  Calls of one context run one behind the other with its
 * denoise / upsampling calls, pixel lists and ray queries, on whatever streams they come. */
#define BRT_ADAPT_SPARSE 1u
#define BRT_ADAPT_NOISY 2u
int32_t brt_set_adaptive(brt_ctx* ctx, uint32_t base_spp, float threshold, uint32_t min_taps);
int32_t brt_render_adaptive_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height, void* d_frame,
                                   uint32_t* d_selected_count_or_null, void* hip_stream, uint32_t flags, brt_stats* stats_or_null);
int32_t brt_adaptive_refine_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height,
                                   const float* d_base_rgba, void* d_out, uint32_t* d_selected_count_or_null, void* hip_stream,
                                   uint32_t flags, brt_stats* stats_or_null);
int32_t brt_adaptive_mask_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height,
                                 const float* d_base_rgba, void* d_mask_u8, void* hip_stream, uint32_t flags);
int32_t brt_host_adaptive_class(float t, uint32_t material_id, const float* rgb, const uint32_t* taps_inside25, const uint32_t* taps_id25,
                                const float* taps_rgb75, float threshold, uint32_t min_taps, uint32_t* out_class);

/* ---- progressive frames ---------------------------------------------------------------------------------------------------------------
 * A Pure (level 3) frame that gains samples call after call, and whose pixels can stop at different sample counts.  A pixel's samples
 * share one RNG state and the sample count enters only the final division, so between two samples a pixel is fully described by a
 * RECORD the caller holds, 32 bytes per pixel, width x height of them (the STATE plane):
 *   { float sum[3]; float m1; float m2; uint32_t rng; uint32_t n; uint32_t rays; }
 * An all-zero record is a pixel without samples (rng is ignored while n == 0).  One sample of colour c: sum += c, then
 * l = (0.2126 r + 0.7152 g) + 0.0722 b, m1 += l, m2 += l * l, n += 1; rays gains the sample's raycasts.  The value of the pixel is
 * {sum / (float)n, 1}, four zeros at n == 0: a pixel continued to n samples holds exactly what brt_render_device stores there at
 * sample_count n, whatever its neighbours got.  The rule, every operation a separately rounded f32 one:
 *   OWN FLAG of a pixel with n >= 2 (fewer: quiet): m = m1 / n, v = max(0, m2 / n - m * m), e = v / n, t = threshold * max(m, 0.01);
 *   NOISY iff e > t * t  (max(a, b) = a > b ? a : b).  Non-finite moments: a NaN moment, or m1 and m2 both +INF (INF - INF = NaN, v = 0),
 *   compares false and the pixel is quiet.  The one non-finite case the rule selects: m2 ALONE overflowing while m * m stays finite
 *   (luminances of about 1e19) gives e = +INF, which is noisy at every threshold whose t * t is finite.  The flag does not read `sum`.
 *   CLASS for a target T: BRT_PROG_SELECTED iff n_p < T and a pixel of the (2 radius + 1)^2 window around p, clipped to the frame, is
 *   noisy (radius 0 or 1).
 * Kernels, costs and quality: DESIGN.md "Progressive frames".
 *   brt_set_progressive             2 <= first_spp <= max_spp <= 65535 (defaults 8, 64), threshold finite and > 0 (default 0.05), radius 0
 *                                   or 1 (default 1); anything else BRT_ERR_INVALID_ARGUMENT and the settings stay as they were.
 *   brt_progressive_sample_device   continues the listed pixels (DEVICE list of n_pixels entries p = y * width + x; d_count_or_null: a
 *                                   DEVICE word that holds the number of entries, n_pixels is then the capacity) to `target` samples:
 *                                   records in d_state, values scattered into d_frame_or_null (width x height, BRT_FLAG_OUT_* format).
 *                                   A record with n >= target is left byte for byte, its value is still stored; an entry outside the
 *                                   frame is refused and touches nothing; pixels not listed are not touched.  A PIXEL MAY BE NAMED AT MOST
 *                                   ONCE PER CALL (two entries of one pixel race).  d_pixels_or_null null: every pixel (n_pixels = width *
 *                                   height, no count word).  camera.sample_count is not read.  flags: BRT_FLAG_OUT_*,
 *                                   BRT_FLAG_CALLER_STREAM, BRT_FLAG_KERNEL_SIMPLE (the plain form).  stats_or_null as brt_render_pixels*
 *                                   (rays, paths = samples run, reserved = entries refused on the context's own stream); kernel_variant
 *                                   36 (streaming form) / 37 (plain form).
 *   brt_progressive_sample          the same for host buffers (no count word), synchronous; pixels of `frame` that are not listed keep
 *                                   what the caller's frame held.
 *   brt_progressive_select_device   the class of every pixel for `target` under the context's threshold and radius: the selected pixels
 *                                   appended to d_list (width * height words) with their number in d_count (zeroed here; only the list's
 *                                   order is not deterministic), the class bytes to d_mask_u8_or_null.  d_list and d_count both null: the
 *                                   mask alone.  Traces nothing.  flags: BRT_FLAG_CALLER_STREAM only.
 *   brt_render_progressive_device   the one-call form: every pixel to first_spp, then for the targets first_spp * 2, * 4, ... (the last one
 *                                   max_spp) a selection and the selected pixels continued, the count taken from the device word: no host
 *                                   round trip, a fixed number of passes.  The state is NOT cleared: a zeroed plane starts a new frame, a
 *                                   held plane with a larger max_spp carries a finished frame on.  d_frame holds every pixel's value.
 *   brt_render_progressive          the same for host buffers, synchronous.
 *   brt_host_progressive_accumulate one sample's colour rgb added to the record at record32, on the host (the code the kernels compile).
 *   brt_host_progressive_class      the class of ONE pixel from the records of its 3x3 window (dy outer, dx inner, both -1 .. 1: the pixel
 *                                   itself is records9[4]; inside9[k] = 0: outside the frame), on the host.
 * Any other flag bit is BRT_ERR_INVALID_ARGUMENT, BRT_FLAG_DENOISE / BRT_FLAG_TEMPORAL included.  A non-default policy (brt_set_policy)
 * and orthographic projection: BRT_ERR_UNSUPPORTED; BRT_ERR_NO_SCENE before an upload; null pointers, a target of 0 or above 65535,
 * sizes outside [1, 32768] and a state plane that overlaps the frame: BRT_ERR_INVALID_ARGUMENT.  DEVICE planes are 16-byte aligned.  A
 * refused call leaves the context usable.  Calls of one context run one behind the other with its pixel lists, ray queries and
 * adaptive calls, on whatever streams they come; plain frames and their dispatch history are not touched. */
#define BRT_PROG_SELECTED 1u
int32_t brt_set_progressive(brt_ctx* ctx, uint32_t first_spp, uint32_t max_spp, float threshold, uint32_t radius);
int32_t brt_progressive_sample_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height,
                                      void* d_state, const uint32_t* d_pixels_or_null, uint32_t n_pixels, const uint32_t* d_count_or_null,
                                      uint32_t target, void* d_frame_or_null, void* hip_stream, uint32_t flags, brt_stats* stats_or_null);
int32_t brt_progressive_sample(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height, void* state,
                               const uint32_t* pixels_or_null, uint32_t n_pixels, uint32_t target, void* frame_or_null, uint32_t flags,
                               brt_stats* stats_or_null);
int32_t brt_progressive_select_device(brt_ctx* ctx, uint32_t width, uint32_t height, const void* d_state, uint32_t target, uint32_t* d_list,
                                      uint32_t* d_count, void* d_mask_u8_or_null, void* hip_stream, uint32_t flags);
int32_t brt_render_progressive_device(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height,
                                      void* d_state, void* d_frame, void* hip_stream, uint32_t flags, brt_stats* stats_or_null);
int32_t brt_render_progressive(brt_ctx* ctx, const void* camera80, const void* window16, uint32_t width, uint32_t height, void* state,
                               void* frame, uint32_t flags, brt_stats* stats_or_null);
int32_t brt_host_progressive_accumulate(void* record32, const float* rgb);
int32_t brt_host_progressive_class(const void* records9, const uint32_t* inside9, uint32_t target, float threshold, uint32_t radius,
                                   uint32_t* out_class);

/* Diagnostic: the 64 raw control words of the last launch on the context's first device: out64[0..4]
 * = the brt_stats counters; after a BRT_FLAG_COUNTERS launch out64[8+2k], out64[9+2k] = how
 * often the waves executed code section k and the sum of active lanes over those executions
 * (k: 0 interior step, 1 leaf step, 2 camera ray made where a sample ended, 3 scatter, 4 sky, 5 rejection-sampler iteration,
 * 6 camera ray made at the top of a round (first sample of a pixel, late sample ends), 7 ray round); wave timeline in 100 MHz ticks: [24] ~first start, [25] ~first / [26] last "lane queue empty",
 * [27] last end, [28] sum of (end - empty) over waves, [29] waves, [30]/[31] live lanes and rounds after "empty";
 * wave time summed over waves: [5] pixel refill, [6] walk loop, [7] shading, [43] drain logic + camera ray +
 * walk begin, [44] rejection-sampler loop; [40] critical tiles and [41] longest pixel (rays) of the view's last measured frame, [42] tiles its
 * order hands out as two half-sample jobs, [62] / [63] pixels of the last launch whose second-half lane took the first half's state over /
 * left the pixel to the first-half lane (whose state was not there yet).
 * out64 must hold 64 words. */
int32_t brt_debug_profile(brt_ctx* ctx, uint64_t* out64);

/* Diagnostic: the dispatch order as the GPU builds it (bevyray_amd/csrc/brt_order.hip, used behind every measuring
 * frame with default settings) for given per-tile ray counts: out_order as brt_host_tile_order's (n_tiles + split_tail words),
 * out_info4 = {critical tiles at the front, longest pixel, non-sky tiles, tiles handed out as two half-sample jobs}.  Tests
 * compare it with brt_host_tile_order.  Host pointers, synchronous. */
int32_t brt_debug_tile_order(brt_ctx* ctx, const uint32_t* ray_sum, const uint32_t* longest_pixel, uint32_t n_tiles,
                             uint32_t sample_count, uint64_t grid_lanes, uint32_t tiles_x, uint32_t dilate, uint32_t split_tail,
                             uint32_t* out_order, uint32_t* out_info4);

/* ---- host-only helpers (no GPU needed) --------------------------------------------- */

/* The dispatch order brt_render derives from one frame's per-tile ray counts (sum and longest pixel of each
 * 8x8 tile): out_order[k] = k-th tile to hand out -- the non-sky tiles (longest pixel
 * first when `sorted`), then the one-ray-per-sample "sky" tiles; out_info5[0..2] = {tiles at the front that go to the
 * lane queue (pixel by pixel to single lanes; the rest are handed out as whole tiles), critical tiles at the
 * front, longest pixel}.  grid_lanes = CUs x threads per workgroup.  dilate > 0: a tile is ranked by the longest pixel of the
 * (2 dilate + 1)^2 tiles around it in the tiles_x-wide tile grid, and is "sky" only if all of them were (what brt_render does by
 * default with radius 2, and with the radius the motion covers when the camera has moved since the costs were measured).
 * split_tail > 0: the last min(split_tail, non-sky tiles) non-sky tiles are in the order TWICE -- [other non-sky tiles | those, first
 * half of the samples | the same, second half | sky tiles] -- so that the jobs ahead of the cheap sky tiles are half as long and the
 * end of a launch is balanced (brt_render does this for frames of at least 6 tiles per wave slot); out_order then holds
 * n_tiles + that many words (room for n_tiles + split_tail), out_info5 = {lane-queue tiles, critical tiles, longest pixel,
 * non-sky tiles, tiles that are split}.  No reference counterpart: the reference draws one fullscreen triangle
 * (pipeline.rs:206-215). */
int32_t brt_host_tile_order(const uint32_t* ray_sum, const uint32_t* longest_pixel, uint32_t n_tiles, uint32_t sample_count,
                            uint64_t grid_lanes, uint32_t sorted, uint32_t lane_permille, uint32_t tiles_x, uint32_t dilate,
                            uint32_t split_tail, uint32_t* out_order, uint32_t* out_info5);

/* Replaces: obvhs::ploc::build_ploc::<24>(aabbs, identity, SortPrecision::U64, 0) and the
 * flatten into BVHNode (extract.rs:315-332), including Model::aabb's 0.1 pad
 * (extract.rs:220-227).  Writes up to `capacity` 48-byte nodes; contract: node 0 is the
 * root, an interior node's children are `index` and `index+1`, leaf iff model_count > 0 and
 * then `index` addresses the model buffer directly.  2*n_models-1 nodes for n_models >= 1. */
int32_t brt_build_bvh(const void* models, uint32_t n_models,
                      void* out_nodes, uint32_t capacity, uint32_t* out_n_nodes);

/* A better tree for the same contract: top-down binned SAH (16 bins, single-sphere leaves, depth capped below the
 * shader's 32-entry stack).  The reference rebuilds PLOC on the CPU every frame (extract.rs:315-321, "TODO" at
 * extract.rs:264-267); the shader only needs the node contract above, and an SAH tree costs the ray loop fewer node
 * visits (10 004-sphere grid: 23.6 -> 19.1 interior visits per ray).  This is the CPU statement of the tree
 * brt_upload_scene builds ON THE GPU (brt_build_bvh_sah_device, the same bytes) when the caller passes no BVH (up to 65 536
 * spheres; above that, or with the knob BRT_BVH_QUALITY=0: PLOC on the GPU).
 * reach: the longest distance a ray has travelled when it reaches a sphere, camera included (it sizes the leaf pads: brt_upload_scene
 * above); 0 = the scene's own extent (what an upload builds); otherwise what brt_host_tree_reach returns for a camera. */
int32_t brt_build_bvh_sah(const void* models, uint32_t n_models, float reach,
                          void* out_nodes, uint32_t capacity, uint32_t* out_n_nodes);

/* The reach rule of the callee-built SAH tree (host arithmetic; brt_render* applies it before every launch): out_scene_scale = S, the
 * largest |centre|_1 + radius over the scene's ordinary spheres (radius <= 100); the camera needs |position|_1 + S + L (L: the longest
 * tangent from the camera to a sphere of radius > 100, i.e. how far away a primary ray can land on the ground); out_level = 0 when
 * that is within 2 S, else the smallest k with 2 S * 2^(k/4) >= it (at most 80); out_reach = the `reach` of that level for
 * brt_build_bvh_sah (0 at level 0).  The resident tree is rebuilt when a camera needs a higher level than it has, or at least two
 * levels less.  camera80: a CameraExtract.  No reference counterpart (the reference pads by 0.1 whatever the camera). */
int32_t brt_host_tree_reach(const void* models, uint32_t n_models, const void* camera80, float* out_scene_scale, uint32_t* out_level,
                            float* out_reach);

/* The same build on the GPU (PLOC in one workgroup, bevyray_amd/csrc/brt_bvh.hip): takes the
 * host model vector, returns byte-identical nodes to brt_build_bvh plus the kernel time.
 * brt_upload_scene uses it when the caller passes no BVH and the scene has more than 65 536 spheres (or BRT_BVH_QUALITY=0).
 * Needs a context (a GPU). */
int32_t brt_build_bvh_device(brt_ctx* ctx, const void* models, uint32_t n_models,
                             void* out_nodes, uint32_t capacity, uint32_t* out_n_nodes, double* out_build_ms);

/* The binned-SAH tree of brt_build_bvh_sah built on the GPU (bevyray_amd/csrc/brt_sah.hip: one workgroup for the nodes of more
 * than 1024 spheres, then a workgroup per subtree, a wave per node): byte-identical nodes plus the kernel time.  This is what
 * brt_upload_scene runs when the caller passes no BVH (up to 65 536 spheres), so that a scene that changes every frame --
 * the reference rebuilds and re-uploads per frame, extract.rs:299-336 -- costs no host-side build.  Needs a context (a GPU). */
int32_t brt_build_bvh_sah_device(brt_ctx* ctx, const void* models, uint32_t n_models, float reach,
                                 void* out_nodes, uint32_t capacity, uint32_t* out_n_nodes, double* out_build_ms);

/* The 255 decision thresholds of the exact 8-bit sRGB encode (BRT_FLAG_OUT_RGBA8_UNORM_SRGB): out255[k - 1] = the smallest f32 >=
 * EOTF((k - 0.5) / 255); the code of a linear value c is the number of thresholds <= c.  For hosts / tests that want to state the
 * same encode on the CPU. */
int32_t brt_host_srgb_thresholds(float* out255);

/* Checks what brt_upload_scene checks, without a context. */
int32_t brt_validate_scene(const void* models, uint32_t n_models,
                           const void* materials, uint32_t n_materials,
                           const void* bvh_nodes, uint32_t n_nodes, uint32_t* out_max_depth);

/* Seeded, deterministic versions of the demo scene (reference src/main.rs:49-240 uses an
 * unseeded RNG) and of the other BASELINE.json scenes.  Writes 32-byte Models and one
 * 32-byte RaytraceMaterial per model (material_id = index, extract.rs:301-310). */
enum {
    BRT_SCENE_COVER = 0,       /* main.rs:87-239, sRGB colours decoded like extract.rs:201 */
    BRT_SCENE_RTIOW_FINAL = 1, /* "Ray Tracing in One Weekend" final scene, linear albedos */
    BRT_SCENE_STRESS_GRID = 2  /* ground + 100 x 100 grid of r=0.2 spheres + 3 big spheres */
};
int32_t brt_scene_generate(uint32_t kind, uint64_t seed,
                           void* out_models, void* out_materials, uint32_t capacity,
                           uint32_t* out_n_models);

/* Host-side mirror of the reference's extract stage, so that a non-Rust host (the C++ /
 * Python harnesses in this repo) produces the same bytes the Rust plugin would:
 *   brt_host_camera_extract  = CameraExtract::extract_component (extract.rs:118-157) for a
 *                              Transform::from_translation(t).looking_at(target, up)
 *   brt_host_window_extract  = WindowExtract::extract_component (extract.rs:70-80), seed explicit
 *   brt_host_material        = RaytraceMaterial::prepare_asset (extract.rs:196-208) */
int32_t brt_host_camera_extract(const float* translation3, const float* target3, const float* up3,
                                float fov, float aspect_ratio, float near_, float far_,
                                uint32_t sample_count, uint32_t bounces, void* out_camera80);
int32_t brt_host_window_extract(float random_seed, uint32_t physical_height, void* out_window16);
int32_t brt_host_material(const float* base_color_srgb3, float metallic, float perceptual_roughness,
                          float reflectance, float ior, float specular_transmission,
                          void* out_material32);

#ifdef __cplusplus
}
#endif
#endif /* BEVYRAY_AMD_H */
