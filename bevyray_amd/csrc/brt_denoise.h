// brt_denoise.h -- host-callable launchers of the guide-buffer a-trous denoiser (brt_denoise.hip).  The formulas: DESIGN.md "Denoiser".
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "brt_layout.h"

namespace brt {

struct DenoiseSettings {
    uint32_t iterations = 5;           // a-trous passes, step 2^i in pass i (1 .. 6)
    float sigma_l = 4.0f, sigma_n = 128.0f, sigma_z = 1.0f;
};

// Above this many samples per pixel the filter's strength falls as the noise std does: sigma_l and the blend weight
// of the filtered result both scale by k = sqrt(kStrengthSpp / spp)
constexpr uint32_t kStrengthSpp = 4;

// The context-owned scratch of one width x height frame, carved out of one allocation (denoise_scratch_bytes): 88 bytes per pixel, every
// plane read by every denoise.
//   g0    float4 {normal.xyz, t}                  first hit of the pixel-centre ray (t = +INF: sky)
//   g1    float4 {a.rgb, material id as bits}     demodulation factor (1, 1, 1 and 0xFFFFFFFF for sky)
//   cv    float4 {c'.rgb, var} x 2                the ping-pong planes of the passes (var < 0: the pixel passes through)
//   dm    float4 {c'.rgb, 0 or -1}                the demodulated input, kept for the last pass's blend
//   aux   float2 {alpha, depth scale}             the input's alpha; t * theta_px / max(|n . dir|, 0.1)
// `frame` is cv[1] under another name: room for an assembled RGBA32F frame (brt_render_device / brt_render on N devices) -- only the
// demodulation reads it, and pass 0 is the first kernel that writes cv[1].
struct DenoiseScratch {
    float4* g0;
    float4* g1;
    float4* cv[2];
    float4* dm;
    float2* aux;
    float4* frame;
};
size_t denoise_scratch_bytes(uint32_t width, uint32_t height);
// a plane of the scratch the last of st.iterations passes does not read: room for the RGBA32F result of a denoise of ds.frame
inline float4* denoise_result_plane(const DenoiseScratch& ds, const DenoiseSettings& st) { return ds.cv[st.iterations & 1u]; }
DenoiseScratch denoise_scratch(char* base, uint32_t width, uint32_t height);

// Post-passes on a blended (level 1 / 2) frame.  on: the input is a coverage frame -- the level's frame traced with
// the raster depth and no raster colour, alpha exactly +0.0 where the raster wins: those pixels pass through (miss guides, never a tap, no
// history) and their output is the texel of d_raster_rgba at the pixel's own index (RGBA32F width x height; nullptr: zeros).  Coverage is
// read from the input's alpha and the guides: no plane of its own.
#ifdef __HIPCC__
// the coverage rule of the kernels: a pixel of a coverage frame is covered iff its alpha is exactly +0.0; its output is its raster texel
__device__ __forceinline__ bool covered(float alpha) { return __float_as_uint(alpha) == 0u; }
__device__ __forceinline__ float4 raster_texel(uint32_t p, const float4* raster) {
    return raster ? raster[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}
#endif

struct BlendPost {
    bool on = false;
    const float* d_raster_rgba = nullptr;
};

// the guide buffer of fp's frame (fp: level 3, one part) on the resident scene.  sid != nullptr (a temporal frame): also the caller's
// index of the sphere every pixel hit (0xFFFFFFFF: sky), the resident index mapped through rmap (nullptr: the identity).  d_coverage !=
// nullptr: the coverage frame (RGBA32F) whose covered pixels get the miss guide and cast no ray
hipError_t launch_denoise_guides(const DeviceSceneView& sv, const FrameParams& fp, const DenoiseScratch& ds, hipStream_t stream,
                                 const uint32_t* rmap = nullptr, uint32_t* sid = nullptr, const float* d_coverage = nullptr);
// guides must be in ds; d_in: RGBA32F width x height (may be ds.frame); d_out: out_format (BRT_FLAG_OUT_*), may equal d_in.  bp.on: the
// last pass stores the raster texel of the covered pixels
hipError_t launch_denoise(const FrameParams& fp, const DenoiseSettings& st, const DenoiseScratch& ds, const float* d_in, void* d_out,
                          uint32_t out_format, hipStream_t stream, const BlendPost& bp = BlendPost());
// launch_denoise in two halves, with the temporal accumulation (brt_temporal.h) between them.  The demodulation: ds.dm, ds.aux, and
// with keep_input a copy of d_in in ds.cv[0].  The filter: from ds.dm into d_out; temporal_moments != nullptr: ds.dm holds {h.rgb, n}
// and the moments plane {m1, m2, ..} of a temporal frame, whose noise estimate and strength are then per pixel
hipError_t launch_denoise_demod(const FrameParams& fp, const DenoiseScratch& ds, const float* d_in, bool keep_input, hipStream_t stream);
hipError_t launch_denoise_filter(const FrameParams& fp, const DenoiseSettings& st, const DenoiseScratch& ds, void* d_out,
                                 uint32_t out_format, hipStream_t stream, const float4* temporal_moments = nullptr,
                                 const BlendPost& bp = BlendPost());

}  // namespace brt
