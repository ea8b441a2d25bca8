// brt_probe.h -- light probes (DESIGN.md "Light probes"): the basis, the record and the list layout shared by the host (brt_api_probe.cpp)
// and the device (brt_probe.hip), and the host-callable launchers of the two kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace brt {

constexpr uint32_t kProbeMaxDirs = 65536u;
constexpr uint32_t kProbeSeedStep = 0x9E3779B9u;     // entry k of a probe is seeded seed + k * this (mod 2^32)
constexpr uint32_t kProbeRecordWords = 32u;          // f32 coeff[27], u32 hits, status, n_dirs, basis, reserved
constexpr uint32_t kProbeCoeffs = 27u;
constexpr uint32_t kProbeStatusMask = 4u | 8u;       // BRT_QUERY_STATUS_INVALID | BRT_QUERY_STATUS_OUT_OF_REACH
constexpr uint32_t kProbeHit = 1u;                   // BRT_QUERY_STATUS_HIT
enum ProbeBasis : uint32_t { PROBE_SH9 = 0u, PROBE_AMBIENT_CUBE = 1u };

// Where entry k of probe p of a list of n_probes x n_dirs entries lies.  0: probe-major, p * n_dirs + k (a wave of the tracer holds 64
// directions of one probe); 1: direction-major, k * n_probes + p (a wave holds one direction of 64 neighbouring probes).  The records do
// not depend on it.  Both were timed (DESIGN.md "Light probes"); the shipped one is documented at the step exports.
#ifndef BRT_PROBE_LAYOUT
#define BRT_PROBE_LAYOUT 0
#endif
constexpr uint32_t kProbeLayout = BRT_PROBE_LAYOUT;
__host__ __device__ inline uint32_t probe_entry(uint32_t p, uint32_t k, uint32_t n_probes, uint32_t n_dirs) {
    return kProbeLayout == 0u ? p * n_dirs + k : k * n_probes + p;
}

// The real SH basis of bands 0..2 on the f32 components of a table direction, every operation separately rounded, in this order
// (tests/probe_ref.py sh9_basis restates it).
__host__ __device__ inline void probe_sh9(float x, float y, float z, float Y[9]) {
    Y[0] = 0.282095f;
    Y[1] = 0.488603f * y;
    Y[2] = 0.488603f * z;
    Y[3] = 0.488603f * x;
    Y[4] = (1.092548f * x) * y;
    Y[5] = (1.092548f * y) * z;
    Y[6] = 0.315392f * ((3.0f * z) * z - 1.0f);
    Y[7] = (1.092548f * x) * z;
    Y[8] = 0.546274f * (x * x - y * y);
}

// k_probe_rays: probes {position.xyz, seed} x the direction table {x, y, z, 0} -> radiance entries (include/bevyray_amd.h "radiance
// queries") at probe_entry(p, k).  n_probes * n_dirs <= 0x7fff0000.
struct ProbeRaysArgs {
    const uint4* probes;
    const float4* dirs;
    uint4* rays;                // two per entry
    uint32_t n_probes, n_dirs;
};
hipError_t launch_probe_rays(const ProbeRaysArgs& a, hipStream_t stream);

// k_probe_project<basis>: the radiance results of n_probes x n_dirs entries at probe_entry(p, k) -> one 128-byte record per probe; one
// wave per probe.
struct ProbeProjectArgs {
    const float4* results;      // two per entry
    const float4* dirs;
    uint32_t* out;              // kProbeRecordWords per probe
    uint32_t n_probes, n_dirs, basis;
};
hipError_t launch_probe_project(const ProbeProjectArgs& a, hipStream_t stream);

}  // namespace brt
