// brt_volume.hip -- irradiance volumes (DESIGN.md "Irradiance volumes"): k_volume_probes writes the probes of a lattice, which the
// light-probe bake (brt_api_probe.cpp bake_enqueue) turns into records as they are; k_volume_sample<BASIS, WRAP> evaluates the sampling
// rule of brt_volume.h for a list of points.  Every f32 operation is separately rounded (-ffp-contract=off) and in the order
// tests/volume_ref.py restates.
#include "brt_volume.h"

namespace brt {

namespace {

constexpr uint32_t kVolumeBlock = 256u;

__global__ __launch_bounds__(kVolumeBlock) void k_volume_probes(VolumeProbesArgs a) {
    const uint32_t i = blockIdx.x * kVolumeBlock + threadIdx.x;
    if (i >= a.n_probes) return;
    a.probes[i] = volume_probe(a.volume, i);
}

// One thread per point: two 16-byte loads of the point, the eight corner records by 16-byte loads through the caches (neighbouring
// points share them; no LDS), one 16-byte store.  The descriptor is uniform: it stays in scalar registers.
template <uint32_t BASIS, bool WRAP>
__global__ __launch_bounds__(kVolumeBlock) void k_volume_sample(VolumeSampleArgs a) {
    const uint32_t i = blockIdx.x * kVolumeBlock + threadIdx.x;
    if (i >= a.n_points) return;
    const uint4 q0 = a.points[2u * (size_t)i], q1 = a.points[2u * (size_t)i + 1u];
    const float p[3] = {__uint_as_float(q0.x), __uint_as_float(q0.y), __uint_as_float(q0.z)};
    const float n[3] = {__uint_as_float(q1.x), __uint_as_float(q1.y), __uint_as_float(q1.z)};
    float rgb[3];
    const uint32_t status = volume_sample<BASIS, WRAP>(a.volume, a.records, p, n, rgb);
    a.out[i] = make_uint4(__float_as_uint(rgb[0]), __float_as_uint(rgb[1]), __float_as_uint(rgb[2]), status);
}

}  // namespace

hipError_t launch_volume_probes(const VolumeProbesArgs& a, hipStream_t stream) {
    if (a.n_probes == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_volume_probes, dim3((a.n_probes + kVolumeBlock - 1u) / kVolumeBlock), dim3(kVolumeBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_volume_sample(const VolumeSampleArgs& a, hipStream_t stream) {
    if (a.n_points == 0u) return hipSuccess;
    const dim3 grid((a.n_points + kVolumeBlock - 1u) / kVolumeBlock), block(kVolumeBlock);
    const bool wrap = (a.volume.flags & kVolumeWrap) != 0u;
    if (a.volume.basis == PROBE_SH9) {
        if (wrap) hipLaunchKernelGGL((k_volume_sample<PROBE_SH9, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((k_volume_sample<PROBE_SH9, false>), grid, block, 0, stream, a);
    } else {
        if (wrap) hipLaunchKernelGGL((k_volume_sample<PROBE_AMBIENT_CUBE, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((k_volume_sample<PROBE_AMBIENT_CUBE, false>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

}  // namespace brt
