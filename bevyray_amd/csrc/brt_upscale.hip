// brt_upscale.hip -- guide-buffer upsampling: a frame traced at low_width x low_height is rebuilt at width x height with the first hit of
// every OUTPUT pixel's centre ray as the guide (a joint-bilateral upsampling, Kopf et al. 2007, on the denoiser's guides and demodulation).
// The rule is pinned in DESIGN.md "Guide-buffer upsampling"; tests/upscale_ref.py restates it in numpy.
//
// k_upscale   one thread per output pixel p, 256 threads = one 16x16 tile (a wave is 4 rows of 16), no atomics, a fixed tap order
//             (bitwise deterministic).  The thread casts p's pixel-centre ray through the resident scene in global memory -- the walk of
//             denoise_guides_pixel (brt_denoise.hip), so the full-size guide planes never exist in memory -- then gathers from the low frame
//             and its guide planes: the 2x2 bilinear footprint (stage A), the 4x4 around it when none of those taps lies on p's material
//             (stage B), the plain bilinear colour when none of those does either (stage C).  A pixel whose ray misses gets the sky of its
//             own ray.  The result is stored in the requested BRT_FLAG_OUT_* format (OutPixel, brt_store.h).
//             With the trailing UpscaleBlend argument (levels 1 / 2, DESIGN.md "Upsampling blended frames") the raster blend is decided
//             per output pixel between the walk and the gather: a covered pixel stores its raster texel and reads no tap.
//             With a trailing UpscaleSelect instead (DESIGN.md "Refined upsampling") a pixel of the call's classes is appended to the
//             call's list -- one ballot and one atomicAdd per wave -- and leaves before stages B and C; or, with a mask, only the class
//             bits of every pixel are written.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "brt_store.h"
#include "brt_upscale.h"
#include "brt_wave.h"

namespace brt {

namespace {

constexpr uint32_t kTile = 16;
constexpr float kLog2e = 1.44269504088896340736f;
constexpr float kSky = __builtin_inff();          // G0.w of a sky pixel

struct UpscaleArgs {
    uint32_t low_width, low_height;
    float theta_low;            // the angle of one LOW pixel: 2 tan(fov / 2) / low_height
    float sigma_n, sigma_z;
    const float4* low;          // the low frame, RGBA32F
    const float4* g0;           // its guides {normal, t}
    const float4* g1;           // {a, material id}
};

BRT_DEV bool finite3(float x, float y, float z) { return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z); }

// the first hit of p, and what stage A / B weigh a tap against
struct Pixel {
    f3 n;
    float t, zden;              // zden = sigma_z zscale_p + 1e-6
    uint32_t material;
};

// the tap q of the low frame: false unless its guide is a hit on p's material and both its colour and c / a are finite; else c' = c / a
// and w_n w_z as ONE exp2 of the summed logarithms (the denoiser's edge_log2 at distance 1, in the low frame's pixel)
BRT_DEV bool tap(const UpscaleArgs& ua, const Pixel& pp, uint32_t q, f3& cd, float& e) {
    const float4 gq = ua.g0[q], aq = ua.g1[q];
    if (!(gq.w < kSky) || __float_as_uint(aq.w) != pp.material) return false;
    const float4 c = ua.low[q];
    cd = mk3(c.x / aq.x, c.y / aq.y, c.z / aq.z);
    if (!finite3(c.x, c.y, c.z) || !finite3(cd.x, cd.y, cd.z)) return false;
    const float nd = max_f(0.0f, dot3(pp.n, mk3(gq.x, gq.y, gq.z)));
    const float dz = __builtin_fabsf(pp.t - gq.w) / pp.zden;
    e = __builtin_exp2f(ua.sigma_n * __builtin_log2f(nd) - dz * kLog2e);
    return true;
}

// resolve_pixel's compare (brt_device.h, raytrace.wgsl:104-120) fed with ONE sample whose depth is t: a miss has the depth fallback_far
// of fp's level, and a NaN raster depth never covers
BRT_DEV bool blend_covered(const FrameParams& fp, float t, uint32_t p, const UpscaleBlend& b) {
    const float depth_p = b.raster_depth ? b.raster_depth[p] : 0.0f;
    const float depth = t == kInf ? fp.fallback_far : t;
    const float rd = depth > fp.far_ ? -1.0f : fp.near_ / depth;
    return depth_p > rd;
}
BRT_DEV float4 blend_texel(uint32_t p, const UpscaleBlend& b) { return raster_texel(p, b.raster_rgba); }
BRT_DEV uint8_t* select_mask(const UpscaleSelect& us) { return us.mask; }
BRT_DEV uint32_t select_classes(const UpscaleSelect& us) { return us.classes; }

// the lanes of the wave that are here and have `sel` set append p to the call's list (wave_append, brt_wave.h)
BRT_DEV void select_append(const UpscaleSelect& us, bool sel, uint32_t p) { wave_append(us.count, us.list, sel, p); }

// whether the kernel's optional pack holds a T
template <typename T, typename... Opt> constexpr bool opt_is() { return (std::is_same<T, Opt>::value || ...); }

// Blend: empty, or one UpscaleBlend -- the frame of a level that blends, fp.level 1 or 2: a covered pixel stores the raster texel of its
// own index (no raster colour: zeros) and returns before the gather, so a wave whose lanes are all covered branches over it; the others
// are the kernel of the empty pack bit for bit.  Or one UpscaleSelect (level 3): see select_append and brt_upscale.h; a pixel that is not
// selected is the kernel of the empty pack bit for bit.  The empty pack is the kernel as it always was, name and arguments included.
template <bool D16, uint32_t FMT, typename... Blend>
__global__ __launch_bounds__(256) void k_upscale(DeviceSceneView sv, FrameParams fp, UpscaleArgs ua,
                                                 typename OutPixel<FMT>::type* __restrict__ out, Blend... blend) {
    const uint32_t px = blockIdx.x * kTile + (threadIdx.x & (kTile - 1u)), py = blockIdx.y * kTile + threadIdx.x / kTile;
    if (px >= fp.width || py >= fp.height) return;
    const uint32_t p = py * fp.width + px;
    // ---- p's own guide: denoise_guides_pixel's walk (brt_denoise.hip), kept in registers.  The eligibility of a tap compares p's material
    // bits with the low planes' and the weights use both normals and depths, so the ray, the normal, a and the material id here and there
    // must move together (the GPU tests hold this kernel to a restatement fed with that kernel's planes at both sizes).
    ScenePtrs sc;
    sc.pairs = reinterpret_cast<const char*>(sv.pairs);
    sc.pairs_far = sc.pairs;
    sc.near_bytes = 0u;
    sc.near_base = 0u;
    sc.sph_base = 0u;
    sc.rows_scratch = 0u;
    sc.hits = nullptr;
    sc.minmax_select = false;
    sc.boxes_ordered = sv.boxes_ordered != 0u;
    sc.spheres_bounded = sv.spheres_bounded != 0u;
    sc.spheres = reinterpret_cast<const float4*>(sv.spheres);
    sc.sphere_material = sv.sphere_material;
    sc.materials = reinterpret_cast<const float4*>(sv.materials);
    sc.sphere_mats = reinterpret_cast<const float4*>(sv.sphere_mats);
    sc.leaf_table = reinterpret_cast<const uint2*>(sv.leaf_table);
    const float uvx = ((float)px + 0.5f) / (float)fp.width;
    const float uvy = ((float)py + 0.5f) / (float)fp.height;
    const f3 d = camera_ray_dir_center(fp, uvx * 2.0f - 1.0f, 1.0f - uvy * 2.0f);
    const f3 o = mk3(fp.cam_pos[0], fp.cam_pos[1], fp.cam_pos[2]);
    uint32_t stack[34];   // DONE sentinel + 32 entries + one spare
    HitCounters hc = {};
    float t;
    uint32_t idx;
    raycast<1, false, D16, false>(sc, sv.root_desc, stack, o, d, t, idx, hc);
    if constexpr (opt_is<UpscaleBlend, Blend...>()) {
        if (blend_covered(fp, t, p, blend...)) {
            out[p] = OutPixel<FMT>::make(blend_texel(p, blend...));
            return;
        }
    }
    if constexpr (opt_is<UpscaleSelect, Blend...>()) {
        if (t == kInf && select_mask(blend...)) {      // (the sky is in no class)
            select_mask(blend...)[p] = 0u;
            return;
        }
    }
    if (t == kInf) {      // sky: what one sample of the ray loop stores for a ray that misses everything, on the centre ray
        const f3 bg = background_gradient(d);
        out[p] = OutPixel<FMT>::make(make_float4(__builtin_sqrtf(bg.x), __builtin_sqrtf(bg.y), __builtin_sqrtf(bg.z), 1.0f));
        return;
    }
    const float4 s = sc.spheres[idx];
    const f3 pos = mk3(o.x + t * d.x, o.y + t * d.y, o.z + t * d.z);
    Pixel pp;
    pp.n = normalize3(mk3(pos.x - s.x, pos.y - s.y, pos.z - s.z));
    pp.t = t;
    pp.material = sv.sphere_material[idx];
    const float4 m0 = sc.sphere_mats[2 * idx], m1 = sc.sphere_mats[2 * idx + 1];
    const bool plain = m1.w == 0.0f;
    const f3 a = plain ? mk3(__builtin_sqrtf(max_f(m0.x, 1e-3f)), __builtin_sqrtf(max_f(m0.y, 1e-3f)), __builtin_sqrtf(max_f(m0.z, 1e-3f)))
                       : mk3(1.0f, 1.0f, 1.0f);
    // the denoiser's depth scale of p, with the angle of one LOW pixel: a tap's distance is measured in low pixels
    const float zscale = (t * ua.theta_low) / max_f(__builtin_fabsf(dot3(pp.n, d)), 0.1f);
    pp.zden = ua.sigma_z * zscale + 1e-6f;
    // ---- p in the low frame's pixel units
    const uint32_t lw = ua.low_width, lh = ua.low_height;
    const float xl = min_f(max_f((((float)px + 0.5f) * (float)lw) / (float)fp.width - 0.5f, 0.0f), (float)(lw - 1u));
    const float yl = min_f(max_f((((float)py + 0.5f) * (float)lh) / (float)fp.height - 0.5f, 0.0f), (float)(lh - 1u));
    const float x0f = __builtin_floorf(xl), y0f = __builtin_floorf(yl);
    const float fx = xl - x0f, fy = yl - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const uint32_t qx[2] = {(uint32_t)x0, min((uint32_t)x0 + 1u, lw - 1u)}, qy[2] = {(uint32_t)y0, min((uint32_t)y0 + 1u, lh - 1u)};
    const float bx[2] = {1.0f - fx, fx}, by[2] = {1.0f - fy, fy};
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
    // ---- stage A: the 2x2 bilinear footprint
#pragma unroll
    for (int j = 0; j < 2; j++) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
            f3 cd;
            float e;
            if (!tap(ua, pp, qy[j] * lw + qx[i], cd, e)) continue;
            const float w = ((bx[i] * by[j] + kUpscaleBilinearFloor) * (e + kUpscaleEdgeFloor)) * kUpscaleScaleA;
            sw = sw + w;
            sr = sr + w * cd.x;
            sg = sg + w * cd.y;
            sb = sb + w * cd.z;
        }
    }
    if constexpr (opt_is<UpscaleSelect, Blend...>()) {
        // p's classes: both tests are exact (a material word, and the weight sum of stage A, whose every term is positive)
        const uint32_t cls = (sw == 0.0f ? BRT_REFINE_EDGES : 0u) | ((m0.w > 0.0f || m1.w > 0.0f) ? BRT_REFINE_SPECULAR : 0u);
        if (select_mask(blend...)) {
            select_mask(blend...)[p] = (uint8_t)cls;
            return;
        }
        const bool sel = (cls & select_classes(blend...)) != 0u;
        select_append(blend..., sel, p);
        if (sel) return;
    }
    // ---- stage B: no tap of the footprint lies on p's material -- the 4x4 around it, by inverse square distance
    if (sw == 0.0f) {
        for (int j = -1; j <= 2; j++) {
            const int ty = y0 + j;
            if (ty < 0 || ty >= (int)lh) continue;
            for (int i = -1; i <= 2; i++) {
                const int tx = x0 + i;
                if (tx < 0 || tx >= (int)lw) continue;
                f3 cd;
                float e;
                if (!tap(ua, pp, (uint32_t)ty * lw + (uint32_t)tx, cd, e)) continue;
                const float dx = (float)tx - xl, dy = (float)ty - yl;
                const float w = ((e + kUpscaleEdgeFloor) / (1.0f + (dx * dx + dy * dy))) * kUpscaleScaleB;
                sw = sw + w;
                sr = sr + w * cd.x;
                sg = sg + w * cd.y;
                sb = sb + w * cd.z;
            }
        }
    }
    if (sw != 0.0f) {
        // the products are f32 values before the store converts them: without the (empty) barrier the RGBA16F instantiations fuse multiply
        // and conversion into one v_fma_mixlo_f16 -- one rounding where the store of the f32 result has two (they differ on f16 ties)
        float r = (sr / sw) * a.x, g = (sg / sw) * a.y, b = (sb / sw) * a.z;
        asm volatile("" : "+v"(r), "+v"(g), "+v"(b));
        out[p] = OutPixel<FMT>::make(make_float4(r, g, b, 1.0f));
        return;
    }
    // ---- stage C: p's sphere is thinner than a low pixel -- the bilinear colour of the finite taps, not demodulated
#pragma unroll
    for (int j = 0; j < 2; j++) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const float4 c = ua.low[qy[j] * lw + qx[i]];
            if (!finite3(c.x, c.y, c.z)) continue;
            const float w = (bx[i] * by[j] + kUpscaleBilinearFloor) * kUpscaleScaleC;
            sw = sw + w;
            sr = sr + w * c.x;
            sg = sg + w * c.y;
            sb = sb + w * c.z;
        }
    }
    out[p] = OutPixel<FMT>::make(sw != 0.0f ? make_float4(sr / sw, sg / sw, sb / sw, 1.0f) : make_float4(0.0f, 0.0f, 0.0f, 1.0f));
}

template <uint32_t FMT, typename... Blend>
void launch_t(const DeviceSceneView& sv, const FrameParams& fp, const UpscaleArgs& ua, void* out, hipStream_t stream, Blend... blend) {
    const dim3 grid((fp.width + kTile - 1u) / kTile, (fp.height + kTile - 1u) / kTile);
    auto* o = reinterpret_cast<typename OutPixel<FMT>::type*>(out);
    if (sv.desc16) hipLaunchKernelGGL((k_upscale<true, FMT, Blend...>), grid, dim3(256), 0, stream, sv, fp, ua, o, blend...);
    else hipLaunchKernelGGL((k_upscale<false, FMT, Blend...>), grid, dim3(256), 0, stream, sv, fp, ua, o, blend...);
}

template <typename... Blend>
hipError_t launch_f(uint32_t out_format, const DeviceSceneView& sv, const FrameParams& fp, const UpscaleArgs& ua, void* out,
                    hipStream_t stream, Blend... blend) {
    switch (out_format) {
        case BRT_FLAG_OUT_RGBA32F: launch_t<BRT_FLAG_OUT_RGBA32F>(sv, fp, ua, out, stream, blend...); break;
        case BRT_FLAG_OUT_RGBA8_UNORM_SRGB: launch_t<BRT_FLAG_OUT_RGBA8_UNORM_SRGB>(sv, fp, ua, out, stream, blend...); break;
        case BRT_FLAG_OUT_RGBA16F: launch_t<BRT_FLAG_OUT_RGBA16F>(sv, fp, ua, out, stream, blend...); break;
        case BRT_FLAG_OUT_RGBA8_UNORM: launch_t<BRT_FLAG_OUT_RGBA8_UNORM>(sv, fp, ua, out, stream, blend...); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_upscale(const DeviceSceneView& sv, const FrameParams& full, const FrameParams& low, const DenoiseSettings& st,
                          const DenoiseScratch& ds_low, const float* d_low, void* d_out, uint32_t out_format, hipStream_t stream,
                          const UpscaleBlend* blend, const UpscaleSelect* select) {
    UpscaleArgs ua;
    ua.low_width = low.width;
    ua.low_height = low.height;
    ua.theta_low = (2.0f * low.tan_half_fov) / (float)low.height;
    ua.sigma_n = st.sigma_n;
    ua.sigma_z = st.sigma_z;
    ua.low = reinterpret_cast<const float4*>(d_low);
    ua.g0 = ds_low.g0;
    ua.g1 = ds_low.g1;
    if (blend && select) return hipErrorInvalidValue;
    if (select) return launch_f(select->mask ? (uint32_t)BRT_FLAG_OUT_RGBA32F : out_format, sv, full, ua, d_out, stream, *select);
    if (blend) return launch_f(out_format, sv, full, ua, d_out, stream, *blend);
    return launch_f(out_format, sv, full, ua, d_out, stream);
}

}  // namespace brt
