// brt_envmap.hip -- reflection probes (DESIGN.md "Reflection probes"): k_envmap_rays writes the radiance entries of a cube map's texels,
// the radiance kernels (brt_radiance.hip) trace them as they are, k_envmap_resolve turns the results into the level-0 texels,
// k_envmap_downsample makes a box level and k_envmap_filter<FMT> evaluates the filter rule of brt_envmap.h for every texel of a
// destination cube.  Every f32 operation is separately rounded (-ffp-contract=off) and in the order tests/envmap_ref.py restates.
#include "brt_envmap.h"
#include "brt_store.h"

namespace brt {

namespace {

constexpr uint32_t kEnvmapBlock = 256u;

// One thread per texel: {position, seed + i * kEnvmapSeedStep | d_i, user = i}.
__global__ __launch_bounds__(kEnvmapBlock) void k_envmap_rays(EnvmapRaysArgs a) {
    const uint32_t e = blockIdx.x * kEnvmapBlock + threadIdx.x;
    if (e >= a.n) return;
    const uint32_t i = a.first + e;
    uint32_t face, x, y;
    envmap_texel_of(a.size, i, &face, &x, &y);
    float d[3];
    envmap_direction(a.size, face, x, y, d);
    a.rays[2u * (size_t)e] = make_uint4(__float_as_uint(a.position[0]), __float_as_uint(a.position[1]), __float_as_uint(a.position[2]),
                                        a.seed + i * kEnvmapSeedStep);
    a.rays[2u * (size_t)e + 1u] = make_uint4(__float_as_uint(d[0]), __float_as_uint(d[1]), __float_as_uint(d[2]), i);
}

// One thread per result: two 16-byte loads, one 16-byte store (and the 8-byte one of an RGBA16F target).
__global__ __launch_bounds__(kEnvmapBlock) void k_envmap_resolve(EnvmapResolveArgs a) {
    const uint32_t e = blockIdx.x * kEnvmapBlock + threadIdx.x;
    if (e >= a.n) return;
    const float4 r0 = a.results[2u * (size_t)e];
    const uint32_t status = __float_as_uint(a.results[2u * (size_t)e + 1u].z);
    const float4 t = envmap_resolve(r0, status);
    a.out[e] = t;
    if (a.out16) a.out16[e] = OutPixel<BRT_FLAG_OUT_RGBA16F>::make(t);
}

// One thread per texel of the smaller cube: four 16-byte loads, one 16-byte store.
__global__ __launch_bounds__(kEnvmapBlock) void k_envmap_downsample(EnvmapDownsampleArgs a) {
    const uint32_t half = a.src_size / 2u;
    const uint32_t i = blockIdx.x * kEnvmapBlock + threadIdx.x;
    if (i >= envmap_texels(half)) return;
    a.out[i] = envmap_box(a.src, a.src_size, i);
}

// THE HOT KERNEL.  One thread per destination texel; a wave covers 64 neighbouring texels of one row (or of a few short rows), so the
// footprints of its lanes for one tap are neighbours in the source and share cache lines.  The tap index is uniform: the table is read
// through the scalar cache, one 16-byte scalar load per tap and wave, and costs no LDS and no barrier; the source is gathered with four
// 16-byte loads per tap.  The result does not depend on the launch shape: every texel is computed by one lane alone, in tap order.
template <uint32_t FMT>
__global__ __launch_bounds__(kEnvmapBlock) void k_envmap_filter(EnvmapFilterArgs a) {
    const uint32_t i = blockIdx.x * kEnvmapBlock + threadIdx.x;
    if (i >= envmap_texels(a.dst_size)) return;
    const float4 t = envmap_filter(a.src, a.src_size, a.taps, a.n_taps, a.dst_size, i);
    static_cast<typename OutPixel<FMT>::type*>(a.out)[i] = OutPixel<FMT>::make(t);
}

inline dim3 grid_of(uint32_t n) { return dim3((n + kEnvmapBlock - 1u) / kEnvmapBlock); }

}  // namespace

hipError_t launch_envmap_rays(const EnvmapRaysArgs& a, hipStream_t stream) {
    if (a.n == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_envmap_rays, grid_of(a.n), dim3(kEnvmapBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_envmap_resolve(const EnvmapResolveArgs& a, hipStream_t stream) {
    if (a.n == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_envmap_resolve, grid_of(a.n), dim3(kEnvmapBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_envmap_downsample(const EnvmapDownsampleArgs& a, hipStream_t stream) {
    const uint32_t n = envmap_texels(a.src_size / 2u);
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_envmap_downsample, grid_of(n), dim3(kEnvmapBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_envmap_filter(const EnvmapFilterArgs& a, hipStream_t stream) {
    const uint32_t n = envmap_texels(a.dst_size);
    if (n == 0u) return hipSuccess;
    if (a.out_format == BRT_FLAG_OUT_RGBA16F) hipLaunchKernelGGL(k_envmap_filter<BRT_FLAG_OUT_RGBA16F>, grid_of(n), dim3(kEnvmapBlock), 0, stream, a);
    else hipLaunchKernelGGL(k_envmap_filter<BRT_FLAG_OUT_RGBA32F>, grid_of(n), dim3(kEnvmapBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace brt
