// brt_lightmap.h -- lightmaps (DESIGN.md "Lightmaps"): the point record, THE RULE of a point's frame, of its rays and of a dilated texel
// that the host twins (brt_api_lightmap.cpp) and the kernels (brt_lightmap.hip) both call, and the host-callable launchers of the three
// kernels.  tests/lightmap_ref.py restates all of it in numpy.  f32, every operation separately rounded (-ffp-contract=off), divide and
// sqrt correctly rounded, in the order written here.
//
//   point    { position.xyz, seed | normal.xyz, offset }.  EMPTY: the three normal words are all +0.0 / -0.0 (no chart covers the texel);
//            looked at before anything else.  INVALID: len2 is 0, INF or NaN; a position word is INF or NaN; offset is INF, NaN or < 0
//            (-0.0 is 0).
//   frame    len2 = (nx * nx + ny * ny) + nz * nz;  len = sqrt(len2);  n = (nx / len, ny / len, nz / len)
//            s = copysign(1, n.z);  a = -1 / (s + n.z);  b = (n.x * n.y) * a
//            t  = (1 + (s * (n.x * n.x)) * a,  s * b,  (-s) * n.x)
//            bt = (b,  s + (n.y * n.y) * a,  -n.y)
//            (the branch-free basis of Duff et al. 2017: s + n.z is at least 1 in magnitude for a unit n, so it is never singular)
//   origin   o = position + offset * n per component (one multiply, one add)
//   entry k  d_k = (l.x * t + l.y * bt) + l.z * n per component, l the table's direction k;
//            { o, seed + k * 0x9E3779B9 (mod 2^32) | d_k, user = k }.  An EMPTY or INVALID point: { position's words, the same seed |
//            0x7fc00000 x 3, user = k }, which the radiance kernels refuse without a walk.
//   dilate   see lightmap_dilate_texel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

namespace brt {

constexpr uint32_t kLightmapMaxDirs = 65536u;
constexpr uint32_t kLightmapMaxSize = 16384u;          // texels per axis
constexpr uint32_t kLightmapMaxPasses = 64u;
constexpr uint32_t kLightmapSeedStep = 0x9E3779B9u;    // entry k of a point is seeded seed + k * this (mod 2^32)
constexpr uint32_t kLightmapNaN = 0x7fc00000u;
constexpr uint32_t kLightmapHit = 1u;                  // BRT_QUERY_STATUS_HIT
constexpr uint32_t kLightmapRefused = 4u | 8u;         // BRT_QUERY_STATUS_INVALID | BRT_QUERY_STATUS_OUT_OF_REACH
constexpr uint32_t kLightmapInvalid = 4u;              // BRT_QUERY_STATUS_INVALID
constexpr uint32_t kLightmapEmpty = 16u;               // BRT_LIGHTMAP_STATUS_EMPTY

__host__ __device__ inline uint32_t lightmap_bits(float x) { return __builtin_bit_cast(uint32_t, x); }
__host__ __device__ inline float lightmap_float(uint32_t x) { return __builtin_bit_cast(float, x); }

// 16-byte word `index` of a buffer: one load on the device; the host's buffer need not be aligned
__host__ __device__ inline float4 lightmap_load16(const void* buf, size_t index) {
#if defined(__HIP_DEVICE_COMPILE__)
    return static_cast<const float4*>(buf)[index];
#else
    float4 v;
    std::memcpy(&v, static_cast<const char*>(buf) + index * 16u, sizeof v);
    return v;
#endif
}

struct LightmapFrame {
    uint32_t status;            // 0, kLightmapEmpty or kLightmapInvalid
    float o[3], n[3], t[3], bt[3];
};

// THE FRAME of a point given as its two 16-byte words
__host__ __device__ inline LightmapFrame lightmap_frame(float4 p0, float4 p1) {
    LightmapFrame f;
    const float nx = p1.x, ny = p1.y, nz = p1.z, offset = p1.w;
    const float len2 = (nx * nx + ny * ny) + nz * nz;
    const bool empty = ((lightmap_bits(nx) | lightmap_bits(ny) | lightmap_bits(nz)) & 0x7fffffffu) == 0u;
    const bool bad = !(len2 > 0.0f) || !__builtin_isfinite(len2) || !__builtin_isfinite(p0.x) || !__builtin_isfinite(p0.y) ||
                     !__builtin_isfinite(p0.z) || !(offset >= 0.0f) || !__builtin_isfinite(offset);
    f.status = empty ? kLightmapEmpty : bad ? kLightmapInvalid : 0u;
    const float len = sqrtf(len2);
    f.n[0] = nx / len;
    f.n[1] = ny / len;
    f.n[2] = nz / len;
    const float s = __builtin_copysignf(1.0f, f.n[2]);
    const float a = -1.0f / (s + f.n[2]);
    const float b = (f.n[0] * f.n[1]) * a;
    f.t[0] = 1.0f + (s * (f.n[0] * f.n[0])) * a;
    f.t[1] = s * b;
    f.t[2] = (-s) * f.n[0];
    f.bt[0] = b;
    f.bt[1] = s + (f.n[1] * f.n[1]) * a;
    f.bt[2] = -f.n[1];
    f.o[0] = p0.x + offset * f.n[0];
    f.o[1] = p0.y + offset * f.n[1];
    f.o[2] = p0.z + offset * f.n[2];
    return f;
}

// ENTRY k of the point {p0, p1} with the frame f and the table's direction l = {x, y, z, -}: the two 16-byte words of the radiance entry
__host__ __device__ inline void lightmap_entry(float4 p0, const LightmapFrame& f, float4 l, uint32_t k, uint4* r0, uint4* r1) {
    const uint32_t seed = lightmap_bits(p0.w) + k * kLightmapSeedStep;
    if (f.status != 0u) {
        *r0 = make_uint4(lightmap_bits(p0.x), lightmap_bits(p0.y), lightmap_bits(p0.z), seed);
        *r1 = make_uint4(kLightmapNaN, kLightmapNaN, kLightmapNaN, k);
        return;
    }
    const float dx = (l.x * f.t[0] + l.y * f.bt[0]) + l.z * f.n[0];
    const float dy = (l.x * f.t[1] + l.y * f.bt[1]) + l.z * f.n[1];
    const float dz = (l.x * f.t[2] + l.y * f.bt[2]) + l.z * f.n[2];
    *r0 = make_uint4(lightmap_bits(f.o[0]), lightmap_bits(f.o[1]), lightmap_bits(f.o[2]), seed);
    *r1 = make_uint4(lightmap_bits(dx), lightmap_bits(dy), lightmap_bits(dz), k);
}

// DILATE.  Texel (x, y) of one pass over the width x height RGBA32F image `src`.  A texel with a > 0 is copied.  Any other visits its
// eight neighbours, dy = -1, 0, 1 outer and dx = -1, 0, 1 inner, the centre skipped; with wrap_u x wraps modulo width (the seam of a
// latitude-longitude chart), else a neighbour outside the image is skipped, as every one above or below it is.  The neighbours with
// a > 0 add their rgb from +0.0 in that order; count > 0: rgb = sum / f32(count), a = 0.5; else the texel is copied.  fill = 0: every
// texel is copied (the store of a call with no passes).
__host__ __device__ inline float4 lightmap_dilate_texel(const void* src, uint32_t width, uint32_t height, uint32_t wrap_u, uint32_t fill,
                                                        uint32_t x, uint32_t y) {
    const float4 c = lightmap_load16(src, (size_t)y * width + x);
    if (fill == 0u || c.w > 0.0f) return c;
    float sum[3] = {0.0f, 0.0f, 0.0f};
    uint32_t count = 0u;
    for (int32_t dy = -1; dy <= 1; dy++) {
        const int64_t yy = (int64_t)y + dy;
        if (yy < 0 || yy >= (int64_t)height) continue;
        for (int32_t dx = -1; dx <= 1; dx++) {
            if (dx == 0 && dy == 0) continue;
            int64_t xx = (int64_t)x + dx;
            if (wrap_u) xx = xx < 0 ? xx + width : xx >= (int64_t)width ? xx - width : xx;
            else if (xx < 0 || xx >= (int64_t)width) continue;
            const float4 t = lightmap_load16(src, (size_t)yy * width + (size_t)xx);
            if (!(t.w > 0.0f)) continue;
            sum[0] = sum[0] + t.x;
            sum[1] = sum[1] + t.y;
            sum[2] = sum[2] + t.z;
            count++;
        }
    }
    if (count == 0u) return c;
    const float n = (float)count;
    return make_float4(sum[0] / n, sum[1] / n, sum[2] / n, 0.5f);
}

// k_lightmap_rays: points {position, seed | normal, offset} x the direction table {x, y, z, 0} -> radiance entries (include/bevyray_amd.h
// "radiance queries") at p * n_dirs + k; one thread per entry.  n_points * n_dirs <= 0x7fff0000.
struct LightmapRaysArgs {
    const float4* points;       // two per point
    const float4* dirs;
    uint4* rays;                // two per entry
    uint32_t n_points, n_dirs;
};
hipError_t launch_lightmap_rays(const LightmapRaysArgs& a, hipStream_t stream);

// k_lightmap_resolve<f16>: the radiance results of n_points x n_dirs entries and their points -> one texel per point (RGBA32F, or RGBA16F
// with f16) and, where info is not null, { hits, status } per point; one wave per point.
struct LightmapResolveArgs {
    const float4* results;      // two per entry
    const float4* points;       // two per point
    void* out;
    uint2* info;
    uint32_t n_points, n_dirs, f16;
};
hipError_t launch_lightmap_resolve(const LightmapResolveArgs& a, hipStream_t stream);

// k_lightmap_dilate<f16>: one pass of lightmap_dilate_texel over `src` -> out (RGBA32F, or RGBA16F with f16); one thread per texel
struct LightmapDilateArgs {
    const float4* src;
    void* out;
    uint32_t width, height, wrap_u, fill, f16;
};
hipError_t launch_lightmap_dilate(const LightmapDilateArgs& a, hipStream_t stream);

}  // namespace brt
