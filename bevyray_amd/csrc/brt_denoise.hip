// brt_denoise.hip -- the guide-buffer a-trous denoiser (Dammertz et al. 2010, with the spatial edge-stopping and variance terms of
// SVGF) on an assembled RGBA32F frame.  The formulas are pinned in DESIGN.md "Denoiser"; tests/denoise_ref.py restates them in numpy.
//
// k_denoise_guides    one thread per pixel: the pixel-centre primary ray (camera_ray_dir_center) walked through the resident scene
//                     with the bring-up kernel's raycast (k_trace_simple): G0 = {normal, t}, G1 = {a, material id}.
// k_denoise_demod     c' = c / a, the alpha and the pixel's depth scale; marks the pixels that pass through (sky, non-finite colour).
// k_denoise_variance  the 7x7 variance of the luminance of c' (SVGF's short-history fallback).
// k_denoise_pass      one a-trous iteration of step s = 2^i: 5x5 taps, weights h(dx) h(dy) w_n w_z w_l; the last one blends with the
//                     demodulated input by the strength of the sample count, remodulates and stores in the requested BRT_FLAG_OUT_*
//                     format (OutPixel, brt_store.h).
// Post-passes on a blended (level 1 / 2) frame: the input is a coverage frame, alpha exactly +0.0 where the raster
// colour wins.  k_denoise_guides_cov gives those pixels the miss guide without casting their ray (everything downstream then treats
// them as pass-through), and k_denoise_pass<true, FMT, const float4*>, the last pass with the raster colour bound, stores their raster texel instead of the input's zeros.
// Every kernel: 256 threads = one 16x16 pixel tile (a wave is 4 rows of 16), one thread per pixel, no atomics (bitwise deterministic).
#include <hip/hip_runtime.h>

#include "brt_denoise.h"
#include "brt_store.h"
#include "brt_temporal.h"

namespace brt {

namespace {

constexpr uint32_t kTile = 16;
constexpr float kLog2e = 1.44269504088896340736f;
constexpr uint32_t kPassThrough = 0xffffffffu;   // (G1.w of a sky pixel)
constexpr float kSky = __builtin_inff();          // G0.w of a sky pixel (the ray loop's own "no hit" is FLT_MAX, kInf)

BRT_DEV float luminance(float4 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }
BRT_DEV bool finite3(float4 c) { return __builtin_isfinite(c.x) && __builtin_isfinite(c.y) && __builtin_isfinite(c.z); }

struct PassArgs {
    uint32_t width, height, step;
    float sigma_l, sigma_n, sigma_z;
    const float4* g0;
    const float4* g1;
    const float2* aux;
    const float4* dm;       // the demodulated input {c', var0}: what the last pass blends towards (strength < 1)
    float strength;         // the last pass returns c'_0 + strength (c'_out - c'_0)
    // a temporal frame: dm holds {h.rgb, n}, and the strength k = min(1, sqrt(kStrengthSpp / (spp n))) is per pixel; sigma_l (unscaled
    // here) is scaled by k below kTemporalConverged, where the variance also comes from the 7x7 neighbourhood, else from the moments
    const float4* moments;  // {m1, m2, ..}; nullptr: not a temporal frame
    float spp;
    const float4* cv_in;
    float4* cv_out;
};

// log2 of w_n * w_z for the tap q of pixel p at pixel distance `dist` (w_n = max(0, n_p . n_q)^sigma_n, w_z = exp(-|t_p - t_q| /
// (sigma_z |q - p| zscale_p + 1e-6))): the pass multiplies the three edge-stopping terms as ONE exp2 of the summed logarithms
BRT_DEV float edge_log2(f3 np, float tp, float zscale, float4 gq, float dist, float sigma_n, float sigma_z) {
    const float nd = max_f(0.0f, dot3(np, mk3(gq.x, gq.y, gq.z)));
    const float dz = __builtin_fabsf(tp - gq.w) / ((sigma_z * dist) * zscale + 1e-6f);
    return sigma_n * __builtin_log2f(nd) - dz * kLog2e;
}

}  // namespace

// ---- guide buffer ------------------------------------------------------------------------------------------------------------------

// (k_upscale, brt_upscale.hip, casts the same guide into registers: the ray, normal, a and material id below and there must move together)
template <bool D16>
BRT_DEV void denoise_guides_pixel(const DeviceSceneView& sv, const FrameParams& fp, float4* __restrict__ g0, float4* __restrict__ g1,
                                  const uint32_t* __restrict__ rmap, uint32_t* __restrict__ sid, uint32_t px, uint32_t py) {
    ScenePtrs sc;                      // the scene in global memory, as k_trace_simple walks it
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
    const float uvx = ((float)px + 0.5f) / (float)fp.width;        // pixel_begin (brt_trace.h)
    const float uvy = ((float)py + 0.5f) / (float)fp.height;
    const f3 d = camera_ray_dir_center(fp, uvx * 2.0f - 1.0f, 1.0f - uvy * 2.0f);
    const f3 o = mk3(fp.cam_pos[0], fp.cam_pos[1], fp.cam_pos[2]);
    uint32_t stack[34];   // DONE sentinel + 32 entries + one spare
    HitCounters hc = {};
    float t;
    uint32_t idx;
    raycast<1, false, D16, false>(sc, sv.root_desc, stack, o, d, t, idx, hc);
    const uint32_t p = py * fp.width + px;
    if (t == kInf) {
        g0[p] = make_float4(0.0f, 0.0f, 0.0f, kSky);
        g1[p] = make_float4(1.0f, 1.0f, 1.0f, __uint_as_float(kPassThrough));
        if (sid) sid[p] = kPassThrough;
        return;
    }
    if (sid) sid[p] = rmap ? rmap[idx] : idx;      // (the resident order is the caller's unless the hot order renumbered it)
    const float4 s = sc.spheres[idx];
    const f3 pos = mk3(o.x + t * d.x, o.y + t * d.y, o.z + t * d.z);           // ray_at (raytrace.wgsl:130-132)
    const f3 n = normalize3(mk3(pos.x - s.x, pos.y - s.y, pos.z - s.z));      // the shading normal (:356)
    const float4 m0 = sc.sphere_mats[2 * idx], m1 = sc.sphere_mats[2 * idx + 1];
    // the first bounce multiplies the path by base_color (scatter's attenuation) unless the material refracts; the frame averages sqrt
    const bool plain = m1.w == 0.0f;
    g0[p] = make_float4(n.x, n.y, n.z, t);
    g1[p] = make_float4(plain ? __builtin_sqrtf(max_f(m0.x, 1e-3f)) : 1.0f, plain ? __builtin_sqrtf(max_f(m0.y, 1e-3f)) : 1.0f,
                        plain ? __builtin_sqrtf(max_f(m0.z, 1e-3f)) : 1.0f, __uint_as_float(sv.sphere_material[idx]));
}

template <bool D16>
__global__ __launch_bounds__(256) void k_denoise_guides(DeviceSceneView sv, FrameParams fp, float4* __restrict__ g0,
                                                        float4* __restrict__ g1, const uint32_t* __restrict__ rmap,
                                                        uint32_t* __restrict__ sid) {
    const uint32_t px = blockIdx.x * kTile + (threadIdx.x & (kTile - 1u)), py = blockIdx.y * kTile + threadIdx.x / kTile;
    if (px >= fp.width || py >= fp.height) return;
    denoise_guides_pixel<D16>(sv, fp, g0, g1, rmap, sid, px, py);
}

// The guides of a coverage frame `cov` (RGBA32F): a covered pixel (alpha +0.0) reads as a miss and casts no ray -- a wave (4 rows of a
// tile) whose pixels are all covered skips the walk, a fully covered tile does none
template <bool D16>
__global__ __launch_bounds__(256) void k_denoise_guides_cov(DeviceSceneView sv, FrameParams fp, float4* __restrict__ g0,
                                                            float4* __restrict__ g1, const uint32_t* __restrict__ rmap,
                                                            uint32_t* __restrict__ sid, const float4* __restrict__ cov) {
    const uint32_t px = blockIdx.x * kTile + (threadIdx.x & (kTile - 1u)), py = blockIdx.y * kTile + threadIdx.x / kTile;
    if (px >= fp.width || py >= fp.height) return;
    const uint32_t p = py * fp.width + px;
    if (covered(cov[p].w)) {
        g0[p] = make_float4(0.0f, 0.0f, 0.0f, kSky);
        g1[p] = make_float4(1.0f, 1.0f, 1.0f, __uint_as_float(kPassThrough));
        if (sid) sid[p] = kPassThrough;
        return;
    }
    denoise_guides_pixel<D16>(sv, fp, g0, g1, rmap, sid, px, py);
}

// ---- demodulation, variance --------------------------------------------------------------------------------------------------------

// cv = {c / a, 0} for a hit pixel with a finite colour; {c.rgb, -1} (passes through, never a tap) for sky and non-finite pixels
__global__ __launch_bounds__(256) void k_denoise_demod(FrameParams fp, const float4* __restrict__ in, const float4* __restrict__ g0,
                                                       const float4* __restrict__ g1, float4* __restrict__ cv, float2* __restrict__ aux,
                                                       float4* __restrict__ keep) {
    const uint32_t px = blockIdx.x * kTile + (threadIdx.x & (kTile - 1u)), py = blockIdx.y * kTile + threadIdx.x / kTile;
    if (px >= fp.width || py >= fp.height) return;
    const uint32_t p = py * fp.width + px;
    const float4 c = in[p], g = g0[p], a = g1[p];
    if (keep) keep[p] = c;
    const float4 cd = make_float4(c.x / a.x, c.y / a.y, c.z / a.z, 0.0f);
    const bool through = !(g.w < kSky) || !finite3(c) || !finite3(cd);
    // depth scale of the pixel: t * theta_px / max(|n . dir|, 0.1), theta_px = 2 tan(fov / 2) / height
    float zscale = 0.0f;
    if (!through) {
        const float uvx = ((float)px + 0.5f) / (float)fp.width;
        const float uvy = ((float)py + 0.5f) / (float)fp.height;
        const f3 d = camera_ray_dir_center(fp, uvx * 2.0f - 1.0f, 1.0f - uvy * 2.0f);
        const float theta = (2.0f * fp.tan_half_fov) / (float)fp.height;
        zscale = (g.w * theta) / max_f(__builtin_fabsf(dot3(mk3(g.x, g.y, g.z), d)), 0.1f);
    }
    cv[p] = through ? make_float4(c.x, c.y, c.z, -1.0f) : cd;
    aux[p] = make_float2(c.w, zscale);
}

// var = the variance of l over the 7x7 neighbourhood, taps of the pixel's class weighted by w_n w_z: sum w l^2 / sum w - (sum w l / sum w)^2
__global__ __launch_bounds__(256) void k_denoise_variance(PassArgs pa) {
    const uint32_t px = blockIdx.x * kTile + (threadIdx.x & (kTile - 1u)), py = blockIdx.y * kTile + threadIdx.x / kTile;
    if (px >= pa.width || py >= pa.height) return;
    const uint32_t p = py * pa.width + px;
    const float4 cp = pa.cv_in[p];
    if (cp.w < 0.0f) { pa.cv_out[p] = cp; return; }
    if (pa.moments && cp.w >= kTemporalConverged) {             // a converged history: the noise of h is var(l) / n
        const float4 m = pa.moments[p];
        pa.cv_out[p] = make_float4(cp.x, cp.y, cp.z, max_f(0.0f, m.y - m.x * m.x) / cp.w);
        return;
    }
    const float4 gp = pa.g0[p];
    const f3 np = mk3(gp.x, gp.y, gp.z);
    const float zscale = pa.aux[p].y;
    float sw = 0.0f, sl = 0.0f, sl2 = 0.0f;
#pragma unroll
    for (int dy = -3; dy <= 3; dy++) {
#pragma unroll
        for (int dx = -3; dx <= 3; dx++) {
            const int qx = (int)px + dx, qy = (int)py + dy;
            if (qx < 0 || qy < 0 || qx >= (int)pa.width || qy >= (int)pa.height) continue;
            const uint32_t q = (uint32_t)qy * pa.width + (uint32_t)qx;
            const float4 cq = pa.cv_in[q];
            if (cq.w < 0.0f) continue;
            const float w = __builtin_exp2f(edge_log2(np, gp.w, zscale, pa.g0[q], __builtin_sqrtf((float)(dx * dx + dy * dy)), pa.sigma_n,
                                                      pa.sigma_z));
            const float l = luminance(cq);
            sw = sw + w;
            sl = sl + w * l;
            sl2 = sl2 + w * (l * l);
        }
    }
    const float mean = sl / sw;
    pa.cv_out[p] = make_float4(cp.x, cp.y, cp.z, max_f(0.0f, sl2 / sw - mean * mean));
}

// ---- a-trous passes ----------------------------------------------------------------------------------------------------------------

// Raster: empty, or one `const float4*` -- the last pass of a coverage frame, in which a covered pixel stores its raster texel (nullptr:
// zeros), never the input's zeros.  The empty pack is the kernel as it always was, name and arguments included.
template <bool LAST, uint32_t FMT, typename... Raster>
__global__ __launch_bounds__(256) void k_denoise_pass(PassArgs pa, typename OutPixel<FMT>::type* __restrict__ out, Raster... raster) {
    const uint32_t px = blockIdx.x * kTile + (threadIdx.x & (kTile - 1u)), py = blockIdx.y * kTile + threadIdx.x / kTile;
    if (px >= pa.width || py >= pa.height) return;
    const uint32_t p = py * pa.width + px;
    const float4 cp = pa.cv_in[p];
    if (cp.w < 0.0f) {                                              // sky / non-finite: unchanged
        if constexpr (LAST && sizeof...(Raster) != 0) {
            if (covered(pa.aux[p].x)) {
                out[p] = OutPixel<FMT>::make(raster_texel(p, raster...));
                return;
            }
        }
        if (LAST) out[p] = OutPixel<FMT>::make(make_float4(cp.x, cp.y, cp.z, pa.aux[p].x));
        else pa.cv_out[p] = cp;
        return;
    }
    // w_l's scale: sigma_l sqrt(gauss3x3(var)), the 3x3 Gaussian (1 2 1)^2 / 16 over the taps of the pixel's class
    float gv = 0.0f, gw = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = (int)px + dx, qy = (int)py + dy;
            if (qx < 0 || qy < 0 || qx >= (int)pa.width || qy >= (int)pa.height) continue;
            const float v = pa.cv_in[(uint32_t)qy * pa.width + (uint32_t)qx].w;
            if (v < 0.0f) continue;
            const float k = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
            gv = gv + k * v;
            gw = gw + k;
        }
    }
    float sigma_l = pa.sigma_l, strength = pa.strength;
    if (pa.moments) {
        const float n = pa.dm[p].w;
        strength = min_f(1.0f, __builtin_sqrtf((float)kStrengthSpp / (pa.spp * n)));
        if (n < kTemporalConverged) sigma_l = pa.sigma_l * strength;
    }
    const float inv_l = 1.0f / (sigma_l * __builtin_sqrtf(max_f(0.0f, gv / gw)) + 1e-6f);
    const float4 gp = pa.g0[p];
    const f3 np = mk3(gp.x, gp.y, gp.z);
    const float zscale = pa.aux[p].y;
    const float lp = luminance(cp);
    constexpr float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    const float stepf = (float)pa.step;
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = (int)px + dx * (int)pa.step, qy = (int)py + dy * (int)pa.step;
            if (qx < 0 || qy < 0 || qx >= (int)pa.width || qy >= (int)pa.height) continue;
            const uint32_t q = (uint32_t)qy * pa.width + (uint32_t)qx;
            const float4 cq = pa.cv_in[q];
            if (cq.w < 0.0f) continue;
            const float e = edge_log2(np, gp.w, zscale, pa.g0[q], stepf * __builtin_sqrtf((float)(dx * dx + dy * dy)), pa.sigma_n,
                                      pa.sigma_z) -
                            (__builtin_fabsf(lp - luminance(cq)) * inv_l) * kLog2e;
            const float w = (h[dx + 2] * h[dy + 2]) * __builtin_exp2f(e);
            sw = sw + w;
            sr = sr + w * cq.x;
            sg = sg + w * cq.y;
            sb = sb + w * cq.z;
            sv = sv + (w * w) * cq.w;
        }
    }
    const float4 c = make_float4(sr / sw, sg / sw, sb / sw, sv / (sw * sw));
    if (LAST) {
        const float4 a = pa.g1[p], c0 = pa.dm[p];
        const float r = c0.x + strength * (c.x - c0.x), g = c0.y + strength * (c.y - c0.y), b = c0.z + strength * (c.z - c0.z);
        out[p] = OutPixel<FMT>::make(make_float4(r * a.x, g * a.y, b * a.z, pa.aux[p].x));
    } else {
        pa.cv_out[p] = c;
    }
}

// ---- host-callable launchers -------------------------------------------------------------------------------------------------------

size_t denoise_scratch_bytes(uint32_t width, uint32_t height) {
    const size_t n = (size_t)width * height;
    return n * 16 * 5 + n * 8;   // g0, g1, cv[2], dm, aux
}

DenoiseScratch denoise_scratch(char* base, uint32_t width, uint32_t height) {
    const size_t n = (size_t)width * height;
    DenoiseScratch ds;
    ds.g0 = reinterpret_cast<float4*>(base);
    ds.g1 = ds.g0 + n;
    ds.cv[0] = ds.g1 + n;
    ds.cv[1] = ds.cv[0] + n;
    ds.dm = ds.cv[1] + n;
    ds.aux = reinterpret_cast<float2*>(ds.dm + n);
    ds.frame = ds.cv[1];          // (read by the demodulation only; pass 0 is the first to write cv[1])
    return ds;
}

static dim3 tiles_of(uint32_t width, uint32_t height) { return dim3((width + kTile - 1u) / kTile, (height + kTile - 1u) / kTile); }

hipError_t launch_denoise_guides(const DeviceSceneView& sv, const FrameParams& fp, const DenoiseScratch& ds, hipStream_t stream,
                                 const uint32_t* rmap, uint32_t* sid, const float* d_coverage) {
    const float4* cov = reinterpret_cast<const float4*>(d_coverage);
    if (cov && sv.desc16)
        hipLaunchKernelGGL(k_denoise_guides_cov<true>, tiles_of(fp.width, fp.height), dim3(256), 0, stream, sv, fp, ds.g0, ds.g1, rmap, sid, cov);
    else if (cov)
        hipLaunchKernelGGL(k_denoise_guides_cov<false>, tiles_of(fp.width, fp.height), dim3(256), 0, stream, sv, fp, ds.g0, ds.g1, rmap, sid, cov);
    else if (sv.desc16)
        hipLaunchKernelGGL(k_denoise_guides<true>, tiles_of(fp.width, fp.height), dim3(256), 0, stream, sv, fp, ds.g0, ds.g1, rmap, sid);
    else
        hipLaunchKernelGGL(k_denoise_guides<false>, tiles_of(fp.width, fp.height), dim3(256), 0, stream, sv, fp, ds.g0, ds.g1, rmap, sid);
    return hipGetLastError();
}

template <uint32_t FMT>
static void launch_last_t(const PassArgs& pa, void* out, hipStream_t stream, const BlendPost& bp) {
    if (bp.on)
        hipLaunchKernelGGL((k_denoise_pass<true, FMT, const float4*>), tiles_of(pa.width, pa.height), dim3(256), 0, stream, pa,
                           reinterpret_cast<typename OutPixel<FMT>::type*>(out), reinterpret_cast<const float4*>(bp.d_raster_rgba));
    else
        hipLaunchKernelGGL((k_denoise_pass<true, FMT>), tiles_of(pa.width, pa.height), dim3(256), 0, stream, pa,
                           reinterpret_cast<typename OutPixel<FMT>::type*>(out));
}

hipError_t launch_denoise(const FrameParams& fp, const DenoiseSettings& st, const DenoiseScratch& ds, const float* d_in, void* d_out,
                          uint32_t out_format, hipStream_t stream, const BlendPost& bp) {
    const hipError_t e = launch_denoise_demod(fp, ds, d_in, false, stream);
    return e != hipSuccess ? e : launch_denoise_filter(fp, st, ds, d_out, out_format, stream, nullptr, bp);
}

hipError_t launch_denoise_demod(const FrameParams& fp, const DenoiseScratch& ds, const float* d_in, bool keep_input, hipStream_t stream) {
    hipLaunchKernelGGL(k_denoise_demod, tiles_of(fp.width, fp.height), dim3(256), 0, stream, fp, reinterpret_cast<const float4*>(d_in),
                       ds.g0, ds.g1, ds.dm, ds.aux, keep_input ? ds.cv[0] : nullptr);
    return hipGetLastError();
}

hipError_t launch_denoise_filter(const FrameParams& fp, const DenoiseSettings& st, const DenoiseScratch& ds, void* d_out,
                                 uint32_t out_format, hipStream_t stream, const float4* temporal_moments, const BlendPost& bp) {
    const dim3 grid = tiles_of(fp.width, fp.height);
    PassArgs pa;
    pa.width = fp.width;
    pa.height = fp.height;
    pa.step = 1u;
    // the noise std of the frame falls as 1 / sqrt(spp): above kStrengthSpp samples the luminance tolerance and the strength fall with it
    const float k = fp.sample_count > kStrengthSpp ? __builtin_sqrtf((float)kStrengthSpp / (float)fp.sample_count) : 1.0f;
    pa.sigma_l = temporal_moments ? st.sigma_l : st.sigma_l * k;
    pa.strength = k;
    pa.moments = temporal_moments;
    pa.spp = (float)fp.sample_count;
    pa.dm = ds.dm;
    pa.sigma_n = st.sigma_n;
    pa.sigma_z = st.sigma_z;
    pa.g0 = ds.g0;
    pa.g1 = ds.g1;
    pa.aux = ds.aux;
    pa.cv_in = ds.dm;
    pa.cv_out = ds.cv[0];
    hipLaunchKernelGGL(k_denoise_variance, grid, dim3(256), 0, stream, pa);
    for (uint32_t i = 0; i < st.iterations; i++) {
        pa.step = 1u << i;
        pa.cv_in = ds.cv[i & 1u];
        pa.cv_out = ds.cv[(i + 1u) & 1u];
        if (i + 1u < st.iterations) {
            hipLaunchKernelGGL((k_denoise_pass<false, BRT_FLAG_OUT_RGBA32F>), grid, dim3(256), 0, stream, pa, nullptr);
            continue;
        }
        switch (out_format) {
            case BRT_FLAG_OUT_RGBA32F: launch_last_t<BRT_FLAG_OUT_RGBA32F>(pa, d_out, stream, bp); break;
            case BRT_FLAG_OUT_RGBA8_UNORM_SRGB: launch_last_t<BRT_FLAG_OUT_RGBA8_UNORM_SRGB>(pa, d_out, stream, bp); break;
            case BRT_FLAG_OUT_RGBA16F: launch_last_t<BRT_FLAG_OUT_RGBA16F>(pa, d_out, stream, bp); break;
            case BRT_FLAG_OUT_RGBA8_UNORM: launch_last_t<BRT_FLAG_OUT_RGBA8_UNORM>(pa, d_out, stream, bp); break;
            default: return hipErrorInvalidValue;
        }
    }
    return hipGetLastError();
}

}  // namespace brt
