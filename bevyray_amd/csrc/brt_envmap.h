// brt_envmap.h -- reflection probes (DESIGN.md "Reflection probes"): the cube-map conventions (texel direction, texel index), the box
// level and THE FILTER RULE that the host twin (brt_api_envmap.cpp) and the kernel (brt_envmap.hip) both call, and the host-callable
// launchers of the four kernels.  tests/envmap_ref.py restates all of it in numpy.  f32, every operation separately rounded
// (-ffp-contract=off) and in the order written here.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

namespace brt {

constexpr uint32_t kEnvmapSeedStep = 0x9E3779B9u;    // texel i of a cube is seeded seed + i * this (mod 2^32)
constexpr uint32_t kEnvmapMaxSize = 4096u;           // texels per edge: the step exports
constexpr uint32_t kEnvmapMaxBakeSize = 1024u;       // ... and the bakes (a power of two)
constexpr uint32_t kEnvmapMaxTaps = 4096u;
constexpr uint32_t kEnvmapHit = 1u;                  // BRT_QUERY_STATUS_HIT
enum EnvmapTaps : uint32_t { ENVMAP_TAPS_GGX = 0u, ENVMAP_TAPS_COSINE = 1u };

__host__ __device__ inline uint32_t envmap_bits(float x) { return __builtin_bit_cast(uint32_t, x); }

// the texels of a cube of edge `size`, and of the first `levels` levels of its chain (level l has edge size >> l)
__host__ __device__ inline uint32_t envmap_texels(uint32_t size) { return 6u * size * size; }
inline uint64_t envmap_level_offset(uint32_t size, uint32_t level) {
    uint64_t n = 0u;
    for (uint32_t l = 0; l < level; l++) n += envmap_texels(size >> l);
    return n;
}

// 16-byte word `index` of a buffer: the device reads it in one load; the host's buffer need not be aligned, so there it is never
// addressed through a float4 pointer
__host__ __device__ inline float4 envmap_load16(const void* buf, size_t index) {
#if defined(__HIP_DEVICE_COMPILE__)
    return static_cast<const float4*>(buf)[index];
#else
    float4 v;
    std::memcpy(&v, static_cast<const char*>(buf) + index * 16u, sizeof v);
    return v;
#endif
}

// TEXEL DIRECTION.  Texel (x, y) of face `face` (+X, -X, +Y, -Y, +Z, -Z) of a cube of edge `size`.
__host__ __device__ inline void envmap_direction(uint32_t size, uint32_t face, uint32_t x, uint32_t y, float d[3]) {
    const float fs = (float)size;
    const float u = (float)(2u * x + 1u) / fs - 1.0f;
    const float v = (float)(2u * y + 1u) / fs - 1.0f;
    float rx, ry, rz;
    switch (face) {
        case 0u: rx = 1.0f; ry = -v; rz = -u; break;
        case 1u: rx = -1.0f; ry = -v; rz = u; break;
        case 2u: rx = u; ry = 1.0f; rz = v; break;
        case 3u: rx = u; ry = -1.0f; rz = -v; break;
        case 4u: rx = u; ry = -v; rz = 1.0f; break;
        default: rx = -u; ry = -v; rz = -1.0f; break;
    }
    const float len = sqrtf((rx * rx + ry * ry) + rz * rz);
    d[0] = rx / len;
    d[1] = ry / len;
    d[2] = rz / len;
}

// texel index i = (face * size + y) * size + x -> (face, x, y)
__host__ __device__ inline void envmap_texel_of(uint32_t size, uint32_t i, uint32_t* face, uint32_t* x, uint32_t* y) {
    const uint32_t row = i / size;
    *x = i - row * size;
    *face = row / size;
    *y = row - *face * size;
}

// RESOLVE.  One radiance result {t, r, g, b | sphere, material, status, user} -> the level-0 texel: the colour made linear (the shader
// returns sqrt(colour) per sample), alpha 1.0 where the texel's own ray hit and 0.0 where it missed.
__host__ __device__ inline float4 envmap_resolve(float4 r0, uint32_t status) {
    return make_float4(r0.y * r0.y, r0.z * r0.z, r0.w * r0.w, (status & kEnvmapHit) ? 1.0f : 0.0f);
}

// BOX LEVEL.  Texel i of the cube of edge src_size / 2 from the four texels of `src` (edge src_size, even) it covers.
__host__ __device__ inline float4 envmap_box(const void* src, uint32_t src_size, uint32_t i) {
    const uint32_t half = src_size / 2u;
    uint32_t face, x, y;
    envmap_texel_of(half, i, &face, &x, &y);
    const size_t row0 = ((size_t)face * src_size + 2u * y) * src_size + 2u * x, row1 = row0 + src_size;
    const float4 t00 = envmap_load16(src, row0), t01 = envmap_load16(src, row0 + 1u);
    const float4 t10 = envmap_load16(src, row1), t11 = envmap_load16(src, row1 + 1u);
    return make_float4(((t00.x + t01.x) + (t10.x + t11.x)) * 0.25f, ((t00.y + t01.y) + (t10.y + t11.y)) * 0.25f,
                       ((t00.z + t01.z) + (t10.z + t11.z)) * 0.25f, ((t00.w + t01.w) + (t10.w + t11.w)) * 0.25f);
}

// one axis of the bilinear footprint: u in [-1, 1] -> the two texel columns (rows) and the weight of the second
__host__ __device__ inline void envmap_axis(float u, uint32_t size, uint32_t* i0, uint32_t* i1, float* g) {
    const float hi = (float)(size - 1u);
    float px = ((u + 1.0f) * 0.5f) * (float)size - 0.5f;
    px = px > 0.0f ? px : 0.0f;                    // (a NaN becomes 0)
    px = px < hi ? px : hi;
    const uint32_t cell = (uint32_t)floorf(px), last = (size > 2u ? size : 2u) - 2u;
    *i0 = cell < last ? cell : last;
    *i1 = *i0 + 1u < size - 1u ? *i0 + 1u : size - 1u;
    *g = px - (float)*i0;
}

// THE FILTER RULE.  Texel i of the destination cube (edge dst_size) from the source cube `src` (edge src_size, 16-byte texels) and the
// table `taps` of n_taps records {lx, ly, lz, w} in the tangent space of the lobe axis.
__host__ __device__ inline float4 envmap_filter(const void* src, uint32_t src_size, const void* taps, uint32_t n_taps, uint32_t dst_size,
                                                uint32_t i) {
    // 1. the lobe axis
    uint32_t face, x, y;
    envmap_texel_of(dst_size, i, &face, &x, &y);
    float N[3];
    envmap_direction(dst_size, face, x, y, N);
    // 2., 3. the frame: up = (0, 0, 1) unless N is within ~2.6 degrees of +-z, then (1, 0, 0); T = normalize(up x N), B = N x T
    float T[3], B[3];
    if (fabsf(N[2]) < 0.999f) { T[0] = -N[1]; T[1] = N[0]; T[2] = 0.0f; }
    else { T[0] = 0.0f; T[1] = -N[2]; T[2] = N[1]; }
    const float tl = sqrtf((T[0] * T[0] + T[1] * T[1]) + T[2] * T[2]);
    T[0] = T[0] / tl;
    T[1] = T[1] / tl;
    T[2] = T[2] / tl;
    B[0] = N[1] * T[2] - N[2] * T[1];
    B[1] = N[2] * T[0] - N[0] * T[2];
    B[2] = N[0] * T[1] - N[1] * T[0];
    // 4. the taps, in order
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, sw = 0.0f;
    for (uint32_t k = 0; k < n_taps; k++) {
        const float4 tap = envmap_load16(taps, k);
        if (tap.w <= 0.0f) continue;               // (a NaN weight is kept)
        // 5. the tap's direction
        const float Lx = (tap.x * T[0] + tap.y * B[0]) + tap.z * N[0];
        const float Ly = (tap.x * T[1] + tap.y * B[1]) + tap.z * N[1];
        const float Lz = (tap.x * T[2] + tap.y * B[2]) + tap.z * N[2];
        // 6., 7. the face by the major axis (ties: X, then Y) and the inverse of the direction table
        const float ax = fabsf(Lx), ay = fabsf(Ly), az = fabsf(Lz);
        uint32_t f;
        float sc, tc, ma;
        if (ax >= ay && ax >= az) {
            ma = ax;
            tc = -Ly;
            if (Lx < 0.0f) { f = 1u; sc = Lz; } else { f = 0u; sc = -Lz; }
        } else if (ay >= az) {
            ma = ay;
            sc = Lx;
            if (Ly < 0.0f) { f = 3u; tc = -Lz; } else { f = 2u; tc = Lz; }
        } else {
            ma = az;
            tc = -Ly;
            if (Lz < 0.0f) { f = 5u; sc = -Lx; } else { f = 4u; sc = Lx; }
        }
        // 8., 9. the footprint inside that face
        uint32_t x0, x1, y0, y1;
        float gx, gy;
        envmap_axis(sc / ma, src_size, &x0, &x1, &gx);
        envmap_axis(tc / ma, src_size, &y0, &y1, &gy);
        // 10. four 16-byte loads
        const size_t r0 = ((size_t)f * src_size + y0) * src_size, r1 = ((size_t)f * src_size + y1) * src_size;
        const float4 c00 = envmap_load16(src, r0 + x0), c01 = envmap_load16(src, r0 + x1);
        const float4 c10 = envmap_load16(src, r1 + x0), c11 = envmap_load16(src, r1 + x1);
        const float hx = 1.0f - gx, hy = 1.0f - gy;
        const float c[4] = {(c00.x * hx + c01.x * gx) * hy + (c10.x * hx + c11.x * gx) * gy,
                            (c00.y * hx + c01.y * gx) * hy + (c10.y * hx + c11.y * gx) * gy,
                            (c00.z * hx + c01.z * gx) * hy + (c10.z * hx + c11.z * gx) * gy,
                            (c00.w * hx + c01.w * gx) * hy + (c10.w * hx + c11.w * gx) * gy};
        // 11.
#pragma unroll
        for (uint32_t ch = 0; ch < 4u; ch++) acc[ch] = acc[ch] + tap.w * c[ch];
        sw = sw + tap.w;
    }
    // 12.
    if (!(sw > 0.0f)) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return make_float4(acc[0] / sw, acc[1] / sw, acc[2] / sw, acc[3] / sw);
}

// k_envmap_rays: texels first .. first + n - 1 of a cube of edge `size` at `position` -> radiance entries {position, seed + i *
// kEnvmapSeedStep | d_i, user = i} at rays[2 (i - first) ..]; one thread per texel.
struct EnvmapRaysArgs {
    float position[3];
    uint32_t seed, size, first, n;
    uint4* rays;                // two per entry
};
hipError_t launch_envmap_rays(const EnvmapRaysArgs& a, hipStream_t stream);

// k_envmap_resolve: n radiance results -> n level-0 texels at out (RGBA32F) and, where out16 is not null, at out16 (RGBA16F) as well
struct EnvmapResolveArgs {
    const float4* results;      // two per entry
    float4* out;
    uint2* out16;
    uint32_t n;
};
hipError_t launch_envmap_resolve(const EnvmapResolveArgs& a, hipStream_t stream);

// k_envmap_downsample: the box level of the cube `src` of edge src_size (even); one thread per texel of the smaller cube
struct EnvmapDownsampleArgs {
    const float4* src;
    float4* out;
    uint32_t src_size;
};
hipError_t launch_envmap_downsample(const EnvmapDownsampleArgs& a, hipStream_t stream);

// k_envmap_filter<fmt>: the filter rule; one thread per destination texel, written as RGBA32F (out_format 0) or RGBA16F
// (BRT_FLAG_OUT_RGBA16F)
struct EnvmapFilterArgs {
    const float4* src;
    const float4* taps;
    void* out;
    uint32_t src_size, n_taps, dst_size, out_format;
};
hipError_t launch_envmap_filter(const EnvmapFilterArgs& a, hipStream_t stream);

}  // namespace brt
