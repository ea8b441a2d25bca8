// brt_lightmap.hip -- lightmaps (DESIGN.md "Lightmaps"): k_lightmap_rays writes the radiance entries of a list of surface points over the
// hemisphere of each point's normal, the radiance kernels (brt_radiance.hip) trace them as they are, k_lightmap_resolve<F16> reduces the
// results to one texel per point and k_lightmap_dilate<LAST_F16> runs one dilation pass.  Every f32 operation is separately rounded
// (-ffp-contract=off) and in the order brt_lightmap.h writes and tests/lightmap_ref.py restates.
#include "brt_lightmap.h"
#include "brt_store.h"

namespace brt {

namespace {

constexpr uint32_t kLightmapBlock = 256u;
constexpr uint32_t kWave = 64u;

// One thread per entry.  The 64 lanes of a wave share one point (or two, at a point's end): its two words come through the cache once,
// and every lane builds the frame for itself -- some thirty f32 operations against two 16-byte stores.
__global__ __launch_bounds__(kLightmapBlock) void k_lightmap_rays(LightmapRaysArgs a) {
    const uint32_t total = a.n_points * a.n_dirs;
    const uint32_t e = blockIdx.x * kLightmapBlock + threadIdx.x;
    if (e >= total) return;
    const uint32_t p = e / a.n_dirs, k = e - p * a.n_dirs;
    const float4 p0 = a.points[2u * (size_t)p], p1 = a.points[2u * (size_t)p + 1u];
    const LightmapFrame f = lightmap_frame(p0, p1);
    uint4 r0, r1;
    lightmap_entry(p0, f, a.dirs[k], k, &r0, &r1);
    a.rays[2u * (size_t)e] = r0;
    a.rays[2u * (size_t)e + 1u] = r1;
}

__device__ inline float wave_sum(float v) {
#pragma unroll
    for (uint32_t off = 32u; off >= 1u; off >>= 1) v = v + __shfl_down(v, off, kWave);    // (lane 0's tree: acc[l] = acc[l] + acc[l + off])
    return v;
}

// One wave per point.  Lane l accumulates entries k = l, l + 64, ... in order from +0.0; six shuffle steps leave the sums in lane 0,
// which writes the texel and the info record.
template <bool F16>
__global__ __launch_bounds__(kLightmapBlock) void k_lightmap_resolve(LightmapResolveArgs a) {
    const uint32_t lane = threadIdx.x & (kWave - 1u);
    const uint32_t p = blockIdx.x * (kLightmapBlock / kWave) + threadIdx.x / kWave;
    if (p >= a.n_points) return;                       // (whole waves leave: p is uniform in a wave)
    float acc[3] = {0.0f, 0.0f, 0.0f};
    uint32_t hits = 0u, status0 = 0u;
    const size_t base = (size_t)p * a.n_dirs;
    for (uint32_t k = lane; k < a.n_dirs; k += kWave) {
        const float4 r0 = a.results[2u * (base + k)];
        const uint32_t st = __float_as_uint(a.results[2u * (base + k) + 1u].z);
        if (k == 0u) status0 = st & kLightmapRefused;
        hits += (st & kLightmapHit) ? 1u : 0u;
        acc[0] = acc[0] + r0.y * r0.y;                 // (the shader returns sqrt(colour) per sample)
        acc[1] = acc[1] + r0.z * r0.z;
        acc[2] = acc[2] + r0.w * r0.w;
    }
#pragma unroll
    for (uint32_t ch = 0; ch < 3u; ch++) acc[ch] = wave_sum(acc[ch]);
#pragma unroll
    for (uint32_t off = 32u; off >= 1u; off >>= 1) hits += __shfl_down(hits, off, kWave);
    if (lane != 0u) return;
    const float4 p1 = a.points[2u * (size_t)p + 1u];
    const bool empty = ((__float_as_uint(p1.x) | __float_as_uint(p1.y) | __float_as_uint(p1.z)) & 0x7fffffffu) == 0u;
    const uint32_t status = empty ? kLightmapEmpty : status0;
    const float n_f = (float)a.n_dirs;
    float4 t = make_float4(acc[0] / n_f, acc[1] / n_f, acc[2] / n_f, 1.0f);
    if (status != 0u) {                                // a refused or EMPTY point: every entry of it was refused
        t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        hits = 0u;
    }
    if (F16) static_cast<uint2*>(a.out)[p] = OutPixel<BRT_FLAG_OUT_RGBA16F>::make(t);
    else static_cast<float4*>(a.out)[p] = t;
    if (a.info) a.info[p] = make_uint2(hits, status);
}

// One thread per texel; a wave covers 64 neighbouring texels of a row, so the nine 16-byte reads of its lanes fall on three rows' cache
// lines, which the neighbouring waves read again through L2.  A covered texel reads its own word alone.
template <bool LAST_F16>
__global__ __launch_bounds__(kLightmapBlock) void k_lightmap_dilate(LightmapDilateArgs a) {
    const uint32_t i = blockIdx.x * kLightmapBlock + threadIdx.x;
    if (i >= a.width * a.height) return;
    const uint32_t y = i / a.width, x = i - y * a.width;
    const float4 t = lightmap_dilate_texel(a.src, a.width, a.height, a.wrap_u, a.fill, x, y);
    if (LAST_F16) static_cast<uint2*>(a.out)[i] = OutPixel<BRT_FLAG_OUT_RGBA16F>::make(t);
    else static_cast<float4*>(a.out)[i] = t;
}

inline dim3 grid_of(uint32_t n) { return dim3((n + kLightmapBlock - 1u) / kLightmapBlock); }

}  // namespace

hipError_t launch_lightmap_rays(const LightmapRaysArgs& a, hipStream_t stream) {
    const uint32_t total = a.n_points * a.n_dirs;
    if (total == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_lightmap_rays, grid_of(total), dim3(kLightmapBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_lightmap_resolve(const LightmapResolveArgs& a, hipStream_t stream) {
    if (a.n_points == 0u) return hipSuccess;
    constexpr uint32_t per_block = kLightmapBlock / kWave;
    const dim3 grid((a.n_points + per_block - 1u) / per_block), block(kLightmapBlock);
    if (a.f16) hipLaunchKernelGGL(k_lightmap_resolve<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(k_lightmap_resolve<false>, grid, block, 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_lightmap_dilate(const LightmapDilateArgs& a, hipStream_t stream) {
    const uint32_t n = a.width * a.height;
    if (n == 0u) return hipSuccess;
    if (a.f16) hipLaunchKernelGGL(k_lightmap_dilate<true>, grid_of(n), dim3(kLightmapBlock), 0, stream, a);
    else hipLaunchKernelGGL(k_lightmap_dilate<false>, grid_of(n), dim3(kLightmapBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace brt
