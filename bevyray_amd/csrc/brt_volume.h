// brt_volume.h -- irradiance volumes (DESIGN.md "Irradiance volumes"): the descriptor of a regular lattice of light probes, the one
// sampling rule that the host twin (brt_api_volume.cpp) and the kernel (brt_volume.hip) both call, and the host-callable launchers of the
// two kernels.  tests/volume_ref.py restates the rule in numpy.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "brt_probe.h"

namespace brt {

constexpr uint32_t kVolumeSeedStep = 0x85EBCA6Bu;    // probe i of a lattice is seeded seed + i * this (mod 2^32)
constexpr uint32_t kVolumeMaxCount = 1024u;          // probes per axis
constexpr uint32_t kVolumeMaxProbes = 1u << 20;      // probes of a lattice
constexpr uint32_t kVolumeMaxPoints = 0x7fff0000u;   // points of one list
constexpr uint32_t kVolumeWrap = 1u;                 // BRT_VOLUME_WRAP
constexpr uint32_t kVolumeClamped = 1u, kVolumeInvalid = 4u, kVolumeNoProbe = 8u;     // BRT_VOLUME_STATUS_*

// The descriptor as the caller passes it (include/bevyray_amd.h "irradiance volumes"): probe (ix, iy, iz) has index
// (iz * count[1] + iy) * count[0] + ix, position origin + f32(i) * spacing per axis and seed `seed + index * kVolumeSeedStep`.
struct VolumeDesc {
    float origin[3];
    uint32_t seed;
    float spacing[3];
    uint32_t basis;             // ProbeBasis
    uint32_t count[3];
    uint32_t flags;             // 0 or kVolumeWrap
};
static_assert(sizeof(VolumeDesc) == 48, "the volume descriptor is 48 bytes");

__host__ __device__ inline uint32_t volume_bits(float x) { return __builtin_bit_cast(uint32_t, x); }
__host__ __device__ inline float volume_float(uint32_t x) { return __builtin_bit_cast(float, x); }
__host__ __device__ inline bool volume_finite(float x) { return (volume_bits(x) & 0x7f800000u) != 0x7f800000u; }

// 16-byte word `index` of the records: the device reads it in one load; the host's buffer need not be aligned, so there it is never
// addressed through a uint4 pointer
__host__ __device__ inline uint4 volume_load16(const void* records, size_t index) {
#if defined(__HIP_DEVICE_COMPILE__)
    return static_cast<const uint4*>(records)[index];
#else
    uint4 v;
    std::memcpy(&v, static_cast<const char*>(records) + index * 16u, sizeof v);
    return v;
#endif
}

// the position of lattice node i of axis a: a multiply, then an add
__host__ __device__ inline float volume_node(const VolumeDesc& v, uint32_t a, uint32_t i) { return v.origin[a] + (float)i * v.spacing[a]; }

// probe `index` of the lattice as its 16 bytes {position.xyz, seed}
__host__ __device__ inline uint4 volume_probe(const VolumeDesc& v, uint32_t index) {
    const uint32_t ix = index % v.count[0], rest = index / v.count[0];
    const uint32_t iy = rest % v.count[1], iz = rest / v.count[1];
    return make_uint4(volume_bits(volume_node(v, 0u, ix)), volume_bits(volume_node(v, 1u, iy)), volume_bits(volume_node(v, 2u, iz)),
                      v.seed + index * kVolumeSeedStep);
}

// THE SAMPLING RULE.  One point {p, n} against the lattice v of 128-byte records (8 x 16 bytes each, lattice order) -> rgb and the
// BRT_VOLUME_STATUS_* bits.  f32, every operation separately rounded (-ffp-contract=off) and in this order; BASIS and WRAP are the
// descriptor's basis and its BRT_VOLUME_WRAP bit.
template <uint32_t BASIS, bool WRAP>
__host__ __device__ inline uint32_t volume_sample(const VolumeDesc& v, const void* records, const float p[3], const float n[3], float rgb[3]) {
    rgb[0] = rgb[1] = rgb[2] = 0.0f;
    // 1. refusal
    if (!volume_finite(p[0]) || !volume_finite(p[1]) || !volume_finite(p[2]) || !volume_finite(n[0]) || !volume_finite(n[1]) ||
        !volume_finite(n[2]))
        return kVolumeInvalid;
    // 2. the cell
    uint32_t status = 0u, i0[3], i1[3];
    float f[3];
#pragma unroll
    for (uint32_t a = 0; a < 3u; a++) {
        float t = (p[a] - v.origin[a]) / v.spacing[a];
        const float hi = (float)(v.count[a] - 1u);
        if (t < 0.0f || t > hi) status |= kVolumeClamped;
        t = t > 0.0f ? t : 0.0f;
        t = t < hi ? t : hi;
        const uint32_t cell = (uint32_t)floorf(t), last = (v.count[a] > 2u ? v.count[a] : 2u) - 2u;
        i0[a] = cell < last ? cell : last;
        f[a] = t - (float)i0[a];
        i1[a] = i0[a] + 1u < v.count[a] - 1u ? i0[a] + 1u : v.count[a] - 1u;
    }
    // 3. the normal's terms
    float ay[9];                 // SH9: A_j Y_j(n)
    float n2[3];                 // cube: n_a * n_a
    if (BASIS == PROBE_SH9) {
        probe_sh9(n[0], n[1], n[2], ay);
        ay[0] = 3.1415927f * ay[0];
#pragma unroll
        for (uint32_t j = 1; j < 4u; j++) ay[j] = 2.0943952f * ay[j];
#pragma unroll
        for (uint32_t j = 4; j < 9u; j++) ay[j] = 0.7853982f * ay[j];
    } else {
#pragma unroll
        for (uint32_t a = 0; a < 3u; a++) n2[a] = n[a] * n[a];
    }
    // 4. the corners
    float acc[3] = {0.0f, 0.0f, 0.0f}, sw = 0.0f;
#pragma unroll
    for (uint32_t c = 0; c < 8u; c++) {
        const bool bx = (c & 1u) != 0u, by = (c & 2u) != 0u, bz = (c & 4u) != 0u;
        const uint32_t ix = bx ? i1[0] : i0[0], iy = by ? i1[1] : i0[1], iz = bz ? i1[2] : i0[2];
        const size_t rec = (size_t)((iz * v.count[1] + iy) * v.count[0] + ix) * 8u;      // the record's first 16-byte word
        constexpr uint32_t kQuads = BASIS == PROBE_SH9 ? 7u : 5u;          // 27 coefficients, or the 18 of the six faces
        uint4 q[kQuads];
#pragma unroll
        for (uint32_t k = 0; k < kQuads; k++) q[k] = volume_load16(records, rec + k);
        const uint4 tail = volume_load16(records, rec + 7u);                          // {status, n_dirs, basis, reserved}
        if (tail.x != 0u || tail.z != BASIS) continue;                      // a refused record, or one of another basis: weight 0
        float w = ((bx ? f[0] : 1.0f - f[0]) * (by ? f[1] : 1.0f - f[1])) * (bz ? f[2] : 1.0f - f[2]);
        if (WRAP) {
            const float dx = volume_node(v, 0u, ix) - p[0], dy = volume_node(v, 1u, iy) - p[1], dz = volume_node(v, 2u, iz) - p[2];
            const float len2 = (dx * dx + dy * dy) + dz * dz;
            const float cs = len2 > 0.0f ? ((dx * n[0] + dy * n[1]) + dz * n[2]) / sqrtf(len2) : 1.0f;
            const float h = (cs + 1.0f) * 0.5f;
            w = w * (h * h + 0.2f);
        }
        float co[4u * kQuads];
#pragma unroll
        for (uint32_t k = 0; k < kQuads; k++) {
            co[4u * k] = volume_float(q[k].x);
            co[4u * k + 1u] = volume_float(q[k].y);
            co[4u * k + 2u] = volume_float(q[k].z);
            co[4u * k + 3u] = volume_float(q[k].w);
        }
#pragma unroll
        for (uint32_t ch = 0; ch < 3u; ch++) {
            float e;
            if (BASIS == PROBE_SH9) {
                e = 0.0f;
#pragma unroll
                for (uint32_t j = 0; j < 9u; j++) e = e + ay[j] * co[3u * j + ch];
            } else {
                const float ex = n[0] < 0.0f ? co[3u + ch] : co[ch];
                const float ey = n[1] < 0.0f ? co[9u + ch] : co[6u + ch];
                const float ez = n[2] < 0.0f ? co[15u + ch] : co[12u + ch];
                e = (n2[0] * ex + n2[1] * ey) + n2[2] * ez;
            }
            acc[ch] = acc[ch] + w * e;
        }
        sw = sw + w;
    }
    // 5. the result
    if (!(sw > 0.0f)) return status | kVolumeNoProbe;
#pragma unroll
    for (uint32_t ch = 0; ch < 3u; ch++) {
        const float e = acc[ch] / sw;
        rgb[ch] = e < 0.0f ? 0.0f : e;
    }
    return status;
}

// k_volume_probes: the lattice's probes {position.xyz, seed} in lattice order; one thread and one 16-byte store per probe.
struct VolumeProbesArgs {
    VolumeDesc volume;
    uint4* probes;
    uint32_t n_probes;          // count[0] * count[1] * count[2] <= kVolumeMaxProbes
};
hipError_t launch_volume_probes(const VolumeProbesArgs& a, hipStream_t stream);

// k_volume_sample<basis, wrap>: points {position.xyz, -, normal.xyz, -} -> samples {rgb, status}; one thread per point.
struct VolumeSampleArgs {
    VolumeDesc volume;
    const uint4* records;       // eight per probe, lattice order
    const uint4* points;        // two per point
    uint4* out;                 // one per point
    uint32_t n_points;          // <= kVolumeMaxPoints
};
hipError_t launch_volume_sample(const VolumeSampleArgs& a, hipStream_t stream);

}  // namespace brt
