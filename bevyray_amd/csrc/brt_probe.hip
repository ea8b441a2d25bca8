// brt_probe.hip -- light probes (DESIGN.md "Light probes"): k_probe_rays writes the radiance entries of a list of probes, the radiance
// kernels (brt_radiance.hip) trace them as they are, k_probe_project<BASIS> reduces the results to one irradiance record per probe.
// Every f32 operation is separately rounded (-ffp-contract=off) and in the order tests/probe_ref.py restates.
#include "brt_probe.h"

namespace brt {

namespace {

constexpr uint32_t kProbeBlock = 256u;
constexpr uint32_t kWave = 64u;

// One thread per entry: {position, seed + k * kProbeSeedStep | d_k, user = k}.  The probe's words are copied as bits (a NaN keeps its payload).
__global__ __launch_bounds__(kProbeBlock) void k_probe_rays(ProbeRaysArgs a) {
    const uint32_t total = a.n_probes * a.n_dirs;
    const uint32_t e = blockIdx.x * kProbeBlock + threadIdx.x;
    if (e >= total) return;
    uint32_t p, k;
    if (kProbeLayout == 0u) { p = e / a.n_dirs; k = e - p * a.n_dirs; }
    else { k = e / a.n_probes; p = e - k * a.n_probes; }
    const uint4 pr = a.probes[p];
    const float4 d = a.dirs[k];
    a.rays[2u * (size_t)e] = make_uint4(pr.x, pr.y, pr.z, pr.w + k * kProbeSeedStep);
    a.rays[2u * (size_t)e + 1u] = make_uint4(__float_as_uint(d.x), __float_as_uint(d.y), __float_as_uint(d.z), k);
}

__device__ inline float wave_sum(float v) {
#pragma unroll
    for (uint32_t off = 32u; off >= 1u; off >>= 1) v = v + __shfl_down(v, off, kWave);    // (lane 0's tree: acc[l] = acc[l] + acc[l + off])
    return v;
}

// One wave per probe.  Lane l accumulates entries k = l, l + 64, ... in order from +0.0; six shuffle steps leave the sums in lane 0,
// which writes the record.
template <uint32_t BASIS>
__global__ __launch_bounds__(kProbeBlock) void k_probe_project(ProbeProjectArgs a) {
    const uint32_t lane = threadIdx.x & (kWave - 1u);
    const uint32_t p = blockIdx.x * (kProbeBlock / kWave) + threadIdx.x / kWave;
    if (p >= a.n_probes) return;                       // (whole waves leave: p is uniform in a wave)
    constexpr uint32_t kAcc = BASIS == PROBE_SH9 ? 27u : 24u;   // SH9: [3 j + ch]; cube: numerators [3 face + ch], then denominators [18 + face]
    float acc[kAcc];
#pragma unroll
    for (uint32_t i = 0; i < kAcc; i++) acc[i] = 0.0f;
    uint32_t hits = 0u, status0 = 0u;
    for (uint32_t k = lane; k < a.n_dirs; k += kWave) {
        const size_t e = probe_entry(p, k, a.n_probes, a.n_dirs);
        const float4 r0 = a.results[2u * e];
        const uint32_t st = __float_as_uint(a.results[2u * e + 1u].z);
        const float4 d = a.dirs[k];
        if (k == 0u) status0 = st & kProbeStatusMask;
        hits += (st & kProbeHit) ? 1u : 0u;
        const float L[3] = {r0.y * r0.y, r0.z * r0.z, r0.w * r0.w};      // (the shader returns sqrt(colour) per sample)
        if (BASIS == PROBE_SH9) {
            float Y[9];
            probe_sh9(d.x, d.y, d.z, Y);
#pragma unroll
            for (uint32_t j = 0; j < 9u; j++)
#pragma unroll
                for (uint32_t ch = 0; ch < 3u; ch++) acc[3u * j + ch] = acc[3u * j + ch] + Y[j] * L[ch];
        } else {
            const float c[6] = {d.x, -d.x, d.y, -d.y, d.z, -d.z};
#pragma unroll
            for (uint32_t f = 0; f < 6u; f++) {
                const float m = c[f] > 0.0f ? c[f] : 0.0f;
                const float m2 = m * m;
#pragma unroll
                for (uint32_t ch = 0; ch < 3u; ch++) acc[3u * f + ch] = acc[3u * f + ch] + m2 * L[ch];
                acc[18u + f] = acc[18u + f] + m2;
            }
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < kAcc; i++) acc[i] = wave_sum(acc[i]);
#pragma unroll
    for (uint32_t off = 32u; off >= 1u; off >>= 1) hits += __shfl_down(hits, off, kWave);
    if (lane != 0u) return;
    float coeff[28];
    if (BASIS == PROBE_SH9) {
        const float scale = 12.566371f / (float)a.n_dirs;
#pragma unroll
        for (uint32_t i = 0; i < 27u; i++) coeff[i] = scale * acc[i];
    } else {
#pragma unroll
        for (uint32_t f = 0; f < 6u; f++)
#pragma unroll
            for (uint32_t ch = 0; ch < 3u; ch++) coeff[3u * f + ch] = acc[18u + f] == 0.0f ? 0.0f : acc[3u * f + ch] / acc[18u + f];
#pragma unroll
        for (uint32_t i = 18u; i < 27u; i++) coeff[i] = 0.0f;
    }
    if (status0 != 0u) {                               // a refused probe: every entry of it was refused
#pragma unroll
        for (uint32_t i = 0; i < 27u; i++) coeff[i] = 0.0f;
        hits = 0u;
    }
    uint4* out = reinterpret_cast<uint4*>(a.out + (size_t)p * kProbeRecordWords);
#pragma unroll
    for (uint32_t q = 0; q < 6u; q++)
        out[q] = make_uint4(__float_as_uint(coeff[4u * q]), __float_as_uint(coeff[4u * q + 1u]), __float_as_uint(coeff[4u * q + 2u]),
                            __float_as_uint(coeff[4u * q + 3u]));
    out[6] = make_uint4(__float_as_uint(coeff[24]), __float_as_uint(coeff[25]), __float_as_uint(coeff[26]), hits);
    out[7] = make_uint4(status0, a.n_dirs, BASIS, 0u);
}

}  // namespace

hipError_t launch_probe_rays(const ProbeRaysArgs& a, hipStream_t stream) {
    const uint32_t total = a.n_probes * a.n_dirs;
    if (total == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_probe_rays, dim3((total + kProbeBlock - 1u) / kProbeBlock), dim3(kProbeBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_probe_project(const ProbeProjectArgs& a, hipStream_t stream) {
    if (a.n_probes == 0u) return hipSuccess;
    constexpr uint32_t per_block = kProbeBlock / kWave;
    const dim3 grid((a.n_probes + per_block - 1u) / per_block), block(kProbeBlock);
    if (a.basis == PROBE_SH9) hipLaunchKernelGGL(k_probe_project<PROBE_SH9>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(k_probe_project<PROBE_AMBIENT_CUBE>, grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace brt
