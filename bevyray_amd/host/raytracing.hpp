// raytracing.hpp -- C++ host side of the render node, mirroring bevyray's plugin surface
// (reference src/raytracing/mod.rs, extract.rs, pipeline.rs) on top of the C ABI
// (include/bevyray_amd.h).  The reference is Rust on Bevy; no Rust toolchain exists in this
// environment, so the host layer is C++17 with the reference's names, fields and error
// behaviour.  INTEGRATION.md shows the Rust `extern "C"` block a maintainer would add instead.
//
//   bevyray::RaytracePlugin         mod.rs:24-84      (GPU context = RaytracingPipeline::from_world)
//   bevyray::RaytracedCamera        mod.rs:86-91
//   bevyray::Raytracing             mod.rs:94-101     #[repr(u32)] Skip..Pure = 0..3
//   bevyray::RaytracedSphere        mod.rs:103-106
//   bevyray::StandardMaterial       the fields extract.rs:200-207 reads, bevy 0.14 defaults
//   bevyray::CameraExtract / WindowExtract / RaytraceLevelExtract / RaytraceMaterial / Model / BVHNode
//                                   extract.rs:56-237 (byte-exact GPU layouts)
//   bevyray::prepare_buffers        extract.rs:280-337
//   bevyray::RayTracingNode::run    pipeline.rs:58-220
#pragma once
#include <array>
#include <cstdint>
#include <cstring>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/bevyray_amd.h"

namespace bevyray {

using Vec3 = std::array<float, 3>;

enum class Raytracing : uint32_t { Skip = 0, FallbackRaster = 1, FallbackRaytraced = 2, Pure = 3 };

struct RaytracedCamera {
    Raytracing level = Raytracing::FallbackRaytraced;
    uint32_t sample_count = 4;
    uint32_t bounces = 4;
};
struct RaytracedSphere { float radius = 1.0f; };

struct StandardMaterial {            // bevy 0.14 defaults; base_color is sRGB
    Vec3 base_color{1.0f, 1.0f, 1.0f};
    float metallic = 0.0f, perceptual_roughness = 0.5f, reflectance = 0.5f, ior = 1.5f, specular_transmission = 0.0f;
};
struct Transform {                   // Transform::from_translation(t).looking_at(target, up)
    Vec3 translation{0.0f, 0.0f, 5.0f}, target{0.0f, 0.0f, 0.0f}, up{0.0f, 1.0f, 0.0f};
};
struct PerspectiveProjection { float fov = 0.7853982f, aspect_ratio = 1.0f, near = 0.1f, far = 1000.0f; };
struct OrthographicProjection {};    // unsupported by the reference (extract.rs:148)

// ---- GPU-layout structs (extract.rs:56-61, 83-104, 181-189, 213-218, 229-237) ----
struct alignas(16) WindowExtract { float random_seed; uint32_t height; float _padding[2]; };
struct alignas(16) CameraExtract {
    uint32_t sample_count, bounce_count, projection; float near, far, fov, aspect, _p0;
    float position[3], _p1, direction[3], _p2, up[3], _p3;
};
struct alignas(16) RaytraceLevelExtract { uint32_t level; uint32_t _p0[3]; float _padding[3]; uint32_t _p1; };
struct alignas(16) RaytraceMaterial { float base_color[3], metallic, roughness, reflectance, ior, specular_transmission; };
struct alignas(16) Model { float position[3], radius; uint32_t material_id, _p[3]; };
struct alignas(16) BVHNode { float bounds_min[3], _p0, bounds_max[3]; uint32_t index, model_count, _p1[3]; };
static_assert(sizeof(WindowExtract) == 16 && sizeof(CameraExtract) == 80 && sizeof(RaytraceLevelExtract) == 32, "uniform layouts");
static_assert(sizeof(RaytraceMaterial) == 32 && sizeof(Model) == 32 && sizeof(BVHNode) == 48, "storage layouts");

struct Error : std::runtime_error {
    int32_t code;
    Error(int32_t c, const std::string& what) : std::runtime_error(what), code(c) {}
};
inline void check(int32_t rc, const brt_ctx* ctx = nullptr) {
    if (rc != BRT_OK) throw Error(rc, std::string("bevyray_amd error ") + std::to_string(rc) + ": " + brt_last_error(ctx));
}

// extract.rs:118-157; nullopt for anything but a perspective projection
inline std::optional<std::pair<RaytraceLevelExtract, CameraExtract>> extract_camera(const RaytracedCamera& cam, const Transform& t,
                                                                                   const PerspectiveProjection& p) {
    CameraExtract c{};
    check(brt_host_camera_extract(t.translation.data(), t.target.data(), t.up.data(), p.fov, p.aspect_ratio, p.near, p.far,
                                  cam.sample_count, cam.bounces, &c));
    RaytraceLevelExtract l{};
    l.level = static_cast<uint32_t>(cam.level);
    return std::make_pair(l, c);
}
inline std::optional<std::pair<RaytraceLevelExtract, CameraExtract>> extract_camera(const RaytracedCamera&, const Transform&,
                                                                                   const OrthographicProjection&) {
    return std::nullopt;
}
// extract.rs:70-80; the reference draws the seed from thread_rng every frame, here it is explicit
inline WindowExtract extract_window(uint32_t physical_height, float random_seed) {
    WindowExtract w{};
    check(brt_host_window_extract(random_seed, physical_height, &w));
    return w;
}
// extract.rs:196-208
inline RaytraceMaterial prepare_asset(const StandardMaterial& m) {
    RaytraceMaterial r{};
    check(brt_host_material(m.base_color.data(), m.metallic, m.perceptual_roughness, m.reflectance, m.ior, m.specular_transmission, &r));
    return r;
}

// ModelBuffer / MaterialBuffer / BVHBuffer (extract.rs:252-262)
struct Buffers {
    std::vector<Model> models;
    std::vector<RaytraceMaterial> materials;
    std::vector<BVHNode> bvh;
};
struct SphereEntity { Vec3 translation; RaytracedSphere sphere; StandardMaterial material; };

// extract.rs:280-337: one Model and one material entry per sphere, then the BVH
inline Buffers prepare_buffers(const std::vector<SphereEntity>& data) {
    Buffers b;
    for (size_t i = 0; i < data.size(); i++) {
        b.materials.push_back(prepare_asset(data[i].material));
        Model m{};
        std::memcpy(m.position, data[i].translation.data(), 12);
        m.radius = data[i].sphere.radius;
        m.material_id = static_cast<uint32_t>(i);
        b.models.push_back(m);
    }
    b.bvh.resize(b.models.empty() ? 0 : 2 * b.models.size() - 1);
    uint32_t n = 0;
    check(brt_build_bvh(b.models.data(), static_cast<uint32_t>(b.models.size()), b.bvh.data(), static_cast<uint32_t>(b.bvh.size()), &n));
    b.bvh.resize(n);
    return b;
}

// Seeded version of the demo's setup() (main.rs:49-240) and the other benchmark scenes
inline Buffers generate_scene(uint32_t kind, uint64_t seed) {
    Buffers b;
    b.models.resize(16384);
    b.materials.resize(16384);
    uint32_t n = 0;
    check(brt_scene_generate(kind, seed, b.models.data(), b.materials.data(), 16384, &n));
    b.models.resize(n);
    b.materials.resize(n);
    b.bvh.resize(n ? 2 * n - 1 : 0);
    uint32_t nn = 0;
    check(brt_build_bvh(b.models.data(), n, b.bvh.data(), static_cast<uint32_t>(b.bvh.size()), &nn));
    b.bvh.resize(nn);
    return b;
}

class RaytracePlugin;

// pipeline.rs:29-221
class RayTracingNode {
public:
    explicit RayTracingNode(brt_ctx* ctx) : ctx_(ctx) {}
    // pipeline.rs:136-138
    // (an empty b.bvh: the callee builds the tree itself -- binned SAH, the recommended path: include/bevyray_amd.h)
    void write_buffers(const Buffers& b) {
        check(brt_upload_scene(ctx_, b.models.data(), static_cast<uint32_t>(b.models.size()), b.materials.data(),
                               static_cast<uint32_t>(b.materials.size()), b.bvh.empty() ? nullptr : b.bvh.data(),
                               static_cast<uint32_t>(b.bvh.size())), ctx_);
    }
    // Returns false when the pass is skipped the way the reference skips it (no camera extract,
    // empty buffers: pipeline.rs:82-151); throws Error for real failures.
    bool run(const std::optional<std::pair<RaytraceLevelExtract, CameraExtract>>& view, const WindowExtract& window,
             uint32_t width, uint32_t height, const Buffers* buffers, const float* raster_rgba, const float* raster_depth,
             std::vector<float>& destination, brt_stats* stats = nullptr, uint32_t flags = 0, bool denoise = false) {
        if (!view) return false;
        if (buffers) {
            const int32_t rc = brt_upload_scene(ctx_, buffers->models.data(), static_cast<uint32_t>(buffers->models.size()),
                                                buffers->materials.data(), static_cast<uint32_t>(buffers->materials.size()),
                                                buffers->bvh.data(), static_cast<uint32_t>(buffers->bvh.size()));
            if (rc == BRT_ERR_EMPTY_SCENE) return false;
            check(rc, ctx_);
        }
        destination.resize(static_cast<size_t>(width) * height * 4);
        check(brt_render(ctx_, &view->second, &window, view->first.level, width, height, raster_rgba, raster_depth,
                         destination.data(), flags | (denoise ? BRT_FLAG_DENOISE : 0u), stats), ctx_);
        return true;
    }
    // The context's denoiser (RaytracePlugin::set_denoise) on an RGBA f32 device frame the caller holds -- e.g. the root's frame after
    // gather() -- into d_out in the BRT_FLAG_OUT_* format of `flags` (d_out may be d_frame).  run / run_device denoise with
    // denoise = true / BRT_FLAG_DENOISE (level 3 only).
    void denoise_device(const CameraExtract& camera, const WindowExtract& window, uint32_t width, uint32_t height, const float* d_frame,
                        void* d_out, void* hip_stream = nullptr, uint32_t flags = 0, brt_stats* stats = nullptr) {
        check(brt_denoise_device(ctx_, &camera, &window, width, height, d_frame, d_out, hip_stream, flags, stats), ctx_);
    }
    // denoise_device for a level-1 / level-2 frame (brt_blend_post_device): d_coverage is that level's RGBA f32 device frame rendered with
    // the raster depth and no raster colour (alpha exactly 0: covered), d_raster_rgba the raster colour on the first device (nullptr:
    // zeros).  Covered pixels of d_out are the raster texels; the rest is denoised / accumulated.  run / run_device do the same with
    // BRT_FLAG_BLEND_POST | BRT_FLAG_DENOISE (| BRT_FLAG_TEMPORAL) in `flags`.
    void blend_post_device(const CameraExtract& camera, const WindowExtract& window, uint32_t width, uint32_t height, const float* d_coverage,
                           const float* d_raster_rgba, void* d_out, void* hip_stream = nullptr, uint32_t flags = 0, brt_stats* stats = nullptr) {
        check(brt_blend_post_device(ctx_, &camera, &window, width, height, d_coverage, d_raster_rgba, d_out, hip_stream, flags, stats), ctx_);
    }
    // Guide-buffer upsampling (include/bevyray_amd.h "guide-buffer upsampling"; Pure frames only).  upscale_device: the RGBA f32
    // low_width x low_height device frame d_low -- rendered with `camera` and upscale_window(window, height, low_height) -- into d_out
    // (width x height, the BRT_FLAG_OUT_* format of `flags`; not overlapping d_low).  render_upscaled_device: trace at the low size,
    // post-passes on the low frame with BRT_FLAG_DENOISE / BRT_FLAG_TEMPORAL in `flags`, upsampling into d_destination.
    void upscale_device(const CameraExtract& camera, const WindowExtract& window, uint32_t low_width, uint32_t low_height, const float* d_low,
                        uint32_t width, uint32_t height, void* d_out, void* hip_stream = nullptr, uint32_t flags = 0, brt_stats* stats = nullptr) {
        check(brt_upscale_device(ctx_, &camera, &window, low_width, low_height, d_low, width, height, d_out, hip_stream, flags, stats), ctx_);
    }
    void render_upscaled_device(const CameraExtract& camera, const WindowExtract& window, uint32_t low_width, uint32_t low_height,
                                uint32_t width, uint32_t height, void* d_destination, void* hip_stream = nullptr, uint32_t flags = 0,
                                brt_stats* stats = nullptr) {
        check(brt_render_upscaled_device(ctx_, &camera, &window, low_width, low_height, width, height, d_destination, hip_stream, flags, stats), ctx_);
    }
    // The same two for a frame of level 1 / 2 (include/bevyray_amd.h "upsampling blended frames"): the low frame is a Pure frame, and every
    // output pixel the full-size raster depth wins is its texel of d_raster_rgba (either raster pointer may be null: zeros; both on the
    // first device, not overlapping the output).  level 3: the calls above.
    void upscale_blend_device(const CameraExtract& camera, const WindowExtract& window, uint32_t level, uint32_t low_width, uint32_t low_height,
                              const float* d_low, uint32_t width, uint32_t height, const float* d_raster_rgba, const float* d_raster_depth,
                              void* d_out, void* hip_stream = nullptr, uint32_t flags = 0, brt_stats* stats = nullptr) {
        check(brt_upscale_blend_device(ctx_, &camera, &window, level, low_width, low_height, d_low, width, height, d_raster_rgba, d_raster_depth,
                                       d_out, hip_stream, flags, stats), ctx_);
    }
    void render_upscaled_blend_device(const CameraExtract& camera, const WindowExtract& window, uint32_t level, uint32_t low_width,
                                      uint32_t low_height, uint32_t width, uint32_t height, const float* d_raster_rgba,
                                      const float* d_raster_depth, void* d_destination, void* hip_stream = nullptr, uint32_t flags = 0,
                                      brt_stats* stats = nullptr) {
        check(brt_render_upscaled_blend_device(ctx_, &camera, &window, level, low_width, low_height, width, height, d_raster_rgba,
                                               d_raster_depth, d_destination, hip_stream, flags, stats), ctx_);
    }
    // whether the raster wins a pixel whose centre ray hits at distance t (+INF: a miss) against raster_depth, at `level`
    static bool blend_covered(const CameraExtract& camera, uint32_t level, float t, float raster_depth) {
        uint32_t c = 0;
        check(brt_host_blend_covered(&camera, level, t, raster_depth, &c), nullptr);
        return c != 0;
    }
    // The sparse pixel tracer (include/bevyray_amd.h "sparse pixel tracer"): entry i of the list (p = py * width + px) -> out[i] = the Pure
    // frame's value at pixel p, bit for bit what run_device stores there.  flags: BRT_FLAG_KERNEL_SIMPLE, BRT_FLAG_CALLER_STREAM (device).
    void render_pixels(const CameraExtract& camera, const WindowExtract& window, uint32_t width, uint32_t height, const uint32_t* pixels,
                       uint32_t n_pixels, float* out_rgba, uint32_t flags = 0, brt_stats* stats = nullptr) {
        check(brt_render_pixels(ctx_, &camera, &window, width, height, pixels, n_pixels, out_rgba, flags, stats), ctx_);
    }
    void render_pixels_device(const CameraExtract& camera, const WindowExtract& window, uint32_t width, uint32_t height,
                              const uint32_t* d_pixels, uint32_t n_pixels, float* d_out_rgba, void* hip_stream = nullptr, uint32_t flags = 0,
                              brt_stats* stats = nullptr) {
        check(brt_render_pixels_device(ctx_, &camera, &window, width, height, d_pixels, n_pixels, d_out_rgba, hip_stream, flags, stats), ctx_);
    }
    // Lens frames (include/bevyray_amd.h "lens frames"): the Pure frame, or a list of its pixels, with a thin lens (depth of field) or an
    // orthographic camera (camera.projection_type = 1) in place of the pinhole.  flags: BRT_FLAG_KERNEL_SIMPLE, and for the device forms
    // BRT_FLAG_CALLER_STREAM and (frames) BRT_FLAG_OUT_*.
    void render_lens(const CameraExtract& camera, const WindowExtract& window, const brt_lens& lens, uint32_t width, uint32_t height,
                     float* out_rgba, uint32_t flags = 0, brt_stats* stats = nullptr) {
        check(brt_render_lens(ctx_, &camera, &window, &lens, width, height, out_rgba, flags, stats), ctx_);
    }
    void render_lens_device(const CameraExtract& camera, const WindowExtract& window, const brt_lens& lens, uint32_t width, uint32_t height,
                            void* d_frame, void* hip_stream = nullptr, uint32_t flags = 0, brt_stats* stats = nullptr) {
        check(brt_render_lens_device(ctx_, &camera, &window, &lens, width, height, d_frame, hip_stream, flags, stats), ctx_);
    }
    void render_lens_pixels(const CameraExtract& camera, const WindowExtract& window, const brt_lens& lens, uint32_t width, uint32_t height,
                            const uint32_t* pixels, uint32_t n_pixels, float* out_rgba, uint32_t flags = 0, brt_stats* stats = nullptr) {
        check(brt_render_lens_pixels(ctx_, &camera, &window, &lens, width, height, pixels, n_pixels, out_rgba, flags, stats), ctx_);
    }
    void render_lens_pixels_device(const CameraExtract& camera, const WindowExtract& window, const brt_lens& lens, uint32_t width,
                                   uint32_t height, const uint32_t* d_pixels, uint32_t n_pixels, float* d_out_rgba, void* hip_stream = nullptr,
                                   uint32_t flags = 0, brt_stats* stats = nullptr) {
        check(brt_render_lens_pixels_device(ctx_, &camera, &window, &lens, width, height, d_pixels, n_pixels, d_out_rgba, hip_stream, flags,
                                            stats), ctx_);
    }
    // Refined upsampling (include/bevyray_amd.h "refined upsampling"): upscale_device / render_upscaled_device with the output pixels of
    // `classes` (BRT_REFINE_EDGES | BRT_REFINE_SPECULAR) traced at full size.  `window` is the FULL-SIZE window.  d_refined_count: a device
    // word that receives the number of refined pixels (or nullptr).  upscale_refine_mask_device: the class bits per pixel, nothing traced.
    void upscale_refine_device(const CameraExtract& camera, const WindowExtract& window, uint32_t low_width, uint32_t low_height,
                               const float* d_low, uint32_t width, uint32_t height, void* d_out, uint32_t classes,
                               uint32_t* d_refined_count = nullptr, void* hip_stream = nullptr, uint32_t flags = 0, brt_stats* stats = nullptr) {
        check(brt_upscale_refine_device(ctx_, &camera, &window, low_width, low_height, d_low, width, height, d_out, classes, d_refined_count,
                                        hip_stream, flags, stats), ctx_);
    }
    void render_upscaled_refined_device(const CameraExtract& camera, const WindowExtract& window, uint32_t low_width, uint32_t low_height,
                                        uint32_t width, uint32_t height, void* d_destination, uint32_t classes,
                                        uint32_t* d_refined_count = nullptr, void* hip_stream = nullptr, uint32_t flags = 0,
                                        brt_stats* stats = nullptr) {
        check(brt_render_upscaled_refined_device(ctx_, &camera, &window, low_width, low_height, width, height, d_destination, classes,
                                                 d_refined_count, hip_stream, flags, stats), ctx_);
    }
    void upscale_refine_mask_device(const CameraExtract& camera, const WindowExtract& window, uint32_t low_width, uint32_t low_height,
                                    const float* d_low, uint32_t width, uint32_t height, void* d_mask_u8, void* hip_stream = nullptr,
                                    uint32_t flags = 0) {
        check(brt_upscale_refine_mask_device(ctx_, &camera, &window, low_width, low_height, d_low, width, height, d_mask_u8, hip_stream, flags), ctx_);
    }
    // Adaptive sampling (include/bevyray_amd.h "adaptive sampling"): a base frame at the context's base_spp (RaytracePlugin::set_adaptive), the
    // pixels its noise rule selects traced again at the camera's sample_count.  d_selected_count: a device word that receives their number
    // (or nullptr).  adaptive_refine_device: for a base frame the caller holds; adaptive_mask_device: the class byte per pixel, nothing traced.
    void render_adaptive_device(const CameraExtract& camera, const WindowExtract& window, uint32_t width, uint32_t height, void* d_destination,
                                uint32_t* d_selected_count = nullptr, void* hip_stream = nullptr, uint32_t flags = 0, brt_stats* stats = nullptr) {
        check(brt_render_adaptive_device(ctx_, &camera, &window, width, height, d_destination, d_selected_count, hip_stream, flags, stats), ctx_);
    }
    void adaptive_refine_device(const CameraExtract& camera, const WindowExtract& window, uint32_t width, uint32_t height, const float* d_base,
                                void* d_out, uint32_t* d_selected_count = nullptr, void* hip_stream = nullptr, uint32_t flags = 0,
                                brt_stats* stats = nullptr) {
        check(brt_adaptive_refine_device(ctx_, &camera, &window, width, height, d_base, d_out, d_selected_count, hip_stream, flags, stats), ctx_);
    }
    void adaptive_mask_device(const CameraExtract& camera, const WindowExtract& window, uint32_t width, uint32_t height, const float* d_base,
                              void* d_mask_u8, void* hip_stream = nullptr, uint32_t flags = 0) {
        check(brt_adaptive_mask_device(ctx_, &camera, &window, width, height, d_base, d_mask_u8, hip_stream, flags), ctx_);
    }
    // Progressive frames (include/bevyray_amd.h "progressive frames"): a plane of 32-byte pixel records (ProgressivePixel) the caller holds;
    // the listed pixels (d_pixels nullptr: every pixel, n_pixels = width * height) continued to `target` samples, each named at most once;
    // the pixels a target is still worth selected from the records' own moments; and the one-call form under RaytracePlugin::set_progressive.
    struct ProgressivePixel { float sum[3]; float m1, m2; uint32_t rng, n, rays; };
    void progressive_sample_device(const CameraExtract& camera, const WindowExtract& window, uint32_t width, uint32_t height, void* d_state,
                                   const uint32_t* d_pixels, uint32_t n_pixels, const uint32_t* d_count, uint32_t target, void* d_frame = nullptr,
                                   void* hip_stream = nullptr, uint32_t flags = 0, brt_stats* stats = nullptr) {
        check(brt_progressive_sample_device(ctx_, &camera, &window, width, height, d_state, d_pixels, n_pixels, d_count, target, d_frame, hip_stream,
                                            flags, stats), ctx_);
    }
    void progressive_sample(const CameraExtract& camera, const WindowExtract& window, uint32_t width, uint32_t height, ProgressivePixel* state,
                            const uint32_t* pixels, uint32_t n_pixels, uint32_t target, void* frame = nullptr, uint32_t flags = 0,
                            brt_stats* stats = nullptr) {
        check(brt_progressive_sample(ctx_, &camera, &window, width, height, state, pixels, n_pixels, target, frame, flags, stats), ctx_);
    }
    void progressive_select_device(uint32_t width, uint32_t height, const void* d_state, uint32_t target, uint32_t* d_list, uint32_t* d_count,
                                   void* d_mask_u8 = nullptr, void* hip_stream = nullptr, uint32_t flags = 0) {
        check(brt_progressive_select_device(ctx_, width, height, d_state, target, d_list, d_count, d_mask_u8, hip_stream, flags), ctx_);
    }
    void render_progressive_device(const CameraExtract& camera, const WindowExtract& window, uint32_t width, uint32_t height, void* d_state,
                                   void* d_destination, void* hip_stream = nullptr, uint32_t flags = 0, brt_stats* stats = nullptr) {
        check(brt_render_progressive_device(ctx_, &camera, &window, width, height, d_state, d_destination, hip_stream, flags, stats), ctx_);
    }
    void render_progressive(const CameraExtract& camera, const WindowExtract& window, uint32_t width, uint32_t height, ProgressivePixel* state,
                            void* frame, uint32_t flags = 0, brt_stats* stats = nullptr) {
        check(brt_render_progressive(ctx_, &camera, &window, width, height, state, frame, flags, stats), ctx_);
    }
    // the window a low_height frame is traced with when it is presented at `height` rows
    static WindowExtract upscale_window(const WindowExtract& window, uint32_t height, uint32_t low_height) {
        WindowExtract w{};
        check(brt_host_upscale_window(&window, height, low_height, &w), nullptr);
        return w;
    }
    // Ray queries against the resident scene (brt_query_rays*, include/bevyray_amd.h "ray queries"): 32-byte rays in, 32-byte hits out.
    // mode: BRT_QUERY_CLOSEST / BRT_QUERY_ANY; origin_bound > 0 first raises the callee-built tree's reach for origins of that 1-norm.
    struct Ray { float origin[3]; float t_max; float direction[3]; uint32_t user; };
    struct Hit { float t; float normal[3]; uint32_t sphere, material, status, user; };
    void query_rays(const Ray* rays, uint32_t n_rays, Hit* hits, uint32_t mode = BRT_QUERY_CLOSEST, float origin_bound = 0.0f,
                    uint64_t* stats8 = nullptr) {
        check(brt_query_rays(ctx_, rays, n_rays, mode, origin_bound, hits, stats8), ctx_);
    }
    void query_rays_device(const void* d_rays, uint32_t n_rays, void* d_hits, uint32_t mode = BRT_QUERY_CLOSEST, float origin_bound = 0.0f,
                           void* hip_stream = nullptr, uint32_t flags = 0, uint64_t* stats8 = nullptr) {
        check(brt_query_rays_device(ctx_, d_rays, n_rays, mode, origin_bound, d_hits, hip_stream, flags, stats8), ctx_);
    }
    // the pixel-centre ray of pixel (px, py): what the guide buffer casts there (picking)
    static Ray pixel_ray(const CameraExtract& camera, const WindowExtract& window, uint32_t width, uint32_t height, uint32_t px, uint32_t py) {
        Ray r{};
        check(brt_host_pixel_ray(&camera, &window, width, height, px, py, &r), nullptr);
        return r;
    }
    // The same pass on an N-device context with the frame assembled ON THE FIRST DEVICE (brt_render_device: tiles by peer
    // copy over xGMI, one de-interleave kernel): `d_destination` is a device pointer, e.g. the mapped colour target
    // (pipeline.rs:191-203).  d_raster_* are optional device buffers on the first device.
    bool run_device(const std::optional<std::pair<RaytraceLevelExtract, CameraExtract>>& view, const WindowExtract& window,
                    uint32_t width, uint32_t height, const float* d_raster_rgba, const float* d_raster_depth, void* d_destination,
                    void* hip_stream = nullptr, brt_stats* stats = nullptr, uint32_t flags = 0) {
        if (!view) return false;
        check(brt_render_device(ctx_, &view->second, &window, view->first.level, width, height, d_raster_rgba, d_raster_depth,
                                d_destination, hip_stream, flags, stats), ctx_);
        return true;
    }
    // One process per GPU: this rank's strips into a device tile, then ONE ncclGather of the tiles to rank 0 and the
    // de-interleave kernel behind it, both inside the library (brt_gather_rccl; `comm` from RaytracePlugin::rccl_comm).
    bool run_part(const std::optional<std::pair<RaytraceLevelExtract, CameraExtract>>& view, const WindowExtract& window, uint32_t width,
                  uint32_t height, uint32_t rank, uint32_t world, float* d_tile, brt_stats* stats = nullptr, uint32_t flags = 0) {
        if (!view) return false;
        check(brt_render_part_device(ctx_, &view->second, &window, view->first.level, width, height, rank, world, nullptr, nullptr, d_tile,
                                     nullptr, flags, stats), ctx_);
        return true;
    }
    void gather(void* comm, int32_t rank, int32_t world, const float* d_tile, float* d_tiles_on_root, uint32_t width, uint32_t height,
                void* d_frame_on_root, void* hip_stream = nullptr, uint32_t flags = 0) {
        check(brt_gather_rccl(ctx_, comm, rank, world, d_tile, d_tiles_on_root, width, height, d_frame_on_root, hip_stream, flags), ctx_);
    }
private:
    brt_ctx* ctx_;
};

// mod.rs:24-84
class RaytracePlugin {
public:
    explicit RaytracePlugin(const std::vector<int32_t>& device_ids = {0}) {
        check(brt_create(device_ids.data(), static_cast<int32_t>(device_ids.size()), &ctx_));
    }
    ~RaytracePlugin() { brt_destroy(ctx_); }
    RaytracePlugin(const RaytracePlugin&) = delete;
    RaytracePlugin& operator=(const RaytracePlugin&) = delete;
    RayTracingNode node() { return RayTracingNode(ctx_); }
    // page-locked frame memory: brt_render DMAs straight into it (brt_host_alloc)
    float* alloc_frame(uint32_t width, uint32_t height) {
        void* p = nullptr;
        check(brt_host_alloc(ctx_, static_cast<uint64_t>(width) * height * 16, &p), ctx_);
        return static_cast<float*>(p);
    }
    // the reading of `||` in raytrace.wgsl:269 (BRT_POLICY_OR_SHORT_CIRCUIT or 0); scheduling knobs (never change a pixel)
    void set_policy(uint32_t flags) { check(brt_set_policy(ctx_, flags), ctx_); }
    void set_tuning(const char* name, uint32_t value) { check(brt_set_tuning(ctx_, name, value), ctx_); }
    // the denoiser's settings (brt_set_denoise; the defaults are the library's)
    void set_denoise(uint32_t iterations = 5, float sigma_luminance = 4.0f, float sigma_normal = 128.0f, float sigma_depth = 1.0f) {
        check(brt_set_denoise(ctx_, iterations, sigma_luminance, sigma_normal, sigma_depth), ctx_);
    }
    // the settings of adaptive frames (brt_set_adaptive; the defaults are the library's)
    void set_adaptive(uint32_t base_spp = 8, float threshold = 0.025f, uint32_t min_taps = 6) {
        check(brt_set_adaptive(ctx_, base_spp, threshold, min_taps), ctx_);
    }
    // the settings of progressive frames (brt_set_progressive; the defaults are the library's)
    void set_progressive(uint32_t first_spp = 8, uint32_t max_spp = 64, float threshold = 0.05f, uint32_t radius = 1) {
        check(brt_set_progressive(ctx_, first_spp, max_spp, threshold, radius), ctx_);
    }
    // the temporal history of BRT_FLAG_TEMPORAL frames (brt_set_temporal: 1..65535, empties it; brt_reset_temporal: on a camera cut)
    void set_temporal(uint32_t max_history = 32) { check(brt_set_temporal(ctx_, max_history), ctx_); }
    void reset_temporal() { check(brt_reset_temporal(ctx_), ctx_); }
    // diagnostic: h.rgb, n, m1, m2, x', y' per pixel of the history after the last temporal frame (brt_debug_temporal_state)
    std::vector<float> debug_temporal_state(uint32_t width, uint32_t height) {
        std::vector<float> out(static_cast<size_t>(width) * height * 8);
        check(brt_debug_temporal_state(ctx_, width, height, out.data()), ctx_);
        return out;
    }
    // one process per GPU: the strips dealt out to the ranks by measured cost instead of s % world (brt_plan_strips: every rank computes
    // the same table from the same probe frame; an empty vector to set_strip_table: back to s % world)
    std::vector<uint32_t> plan_strips(const std::pair<RaytraceLevelExtract, CameraExtract>& view, const WindowExtract& window, uint32_t width,
                                      uint32_t height, uint32_t world, uint32_t probe_spp = 4) {
        std::vector<uint32_t> table((height + BRT_STRIP_ROWS - 1u) / BRT_STRIP_ROWS);
        check(brt_plan_strips(ctx_, &view.second, &window, view.first.level, width, height, world, probe_spp, table.data()), ctx_);
        return table;
    }
    void set_strip_table(uint32_t world, const std::vector<uint32_t>& part_of_strip) {
        check(brt_set_strip_table(ctx_, world, static_cast<uint32_t>(part_of_strip.size()), part_of_strip.empty() ? nullptr : part_of_strip.data()), ctx_);
    }
    // the colour target's memory, exported by the host's graphics API as a file descriptor (pipeline.rs:191-203 renders straight
    // into post_process.destination): a device pointer that run_device / gather accept as the frame (brt_import_frame_fd)
    void* import_frame(int32_t fd, uint64_t bytes, uint32_t handle_type = BRT_EXTMEM_OPAQUE_FD) {
        void* d = nullptr;
        check(brt_import_frame_fd(ctx_, fd, bytes, handle_type, &d), ctx_);
        return d;
    }
    void release_frame(void* d_frame) { check(brt_release_frame(ctx_, d_frame), ctx_); }
    // the communicator of the one-process-per-GPU form: `id` from rccl_unique_id() on rank 0, handed to the others by the host's means
    static std::array<char, 128> rccl_unique_id() {
        std::array<char, 128> id{};
        check(brt_rccl_unique_id(id.data()));
        return id;
    }
    void* rccl_comm(const std::array<char, 128>& id, int32_t rank, int32_t world) {
        void* comm = nullptr;
        check(brt_rccl_comm_create(ctx_, id.data(), rank, world, &comm), ctx_);
        return comm;
    }
    void rccl_comm_destroy(void* comm) { check(brt_rccl_comm_destroy(ctx_, comm), ctx_); }
    brt_ctx* context() { return ctx_; }
private:
    brt_ctx* ctx_ = nullptr;
};

}  // namespace bevyray
