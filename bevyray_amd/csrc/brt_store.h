// brt_store.h -- the store conversion of a device frame into the colour target's format (BRT_FLAG_OUT_*), shared by the
// de-interleave (brt_kernels.hip) and the last pass of the denoiser (brt_denoise.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <hip/hip_fp16.h>

#include "../../include/bevyray_amd.h"   // BRT_FLAG_OUT_*
#include "brt_device.h"
#include "brt_srgb_table.h"

namespace brt {

// The frame is written in the colour target's own format (reference: the pass renders into post_process.destination, whose format is
// TextureFormat::bevy_default() -- 8-bit sRGB, or Rgba16Float under HDR, pipeline.rs:311-315).  The conversions, exactly:
//   RGBA8 sRGB   colour: v = round(255 * OETF(clamp(c, 0, 1))) as the number of thresholds <= c (brt_srgb_table.h: exact for every f32, a
//                NaN encodes as 0 like the hardware's clamp); alpha: the linear rule below
//   RGBA8        v = round-half-even(255 * clamp(c, 0, 1)), the product exact in f64
//   RGBA16F      f32 -> f16, round to nearest even (v_cvt_f16_f32; overflow to infinity, denormals kept)
BRT_DEV uint32_t encode_srgb8(float c) {
    uint32_t n = 0;                                       // thresholds <= c so far: binary search over the 255 of them
#pragma unroll
    for (uint32_t step = 128u; step != 0u; step >>= 1)
        if (n + step <= 255u && c >= kSrgbThreshold[n + step - 1u]) n += step;
    return n;
}
BRT_DEV uint32_t encode_unorm8(float c) {
    const double x = c > 0.0f ? (c < 1.0f ? (double)c : 1.0) : 0.0;      // (a NaN fails the first test: 0)
    return (uint32_t)__double2int_rn(x * 255.0);
}
template <uint32_t FMT> struct OutPixel;
template <> struct OutPixel<BRT_FLAG_OUT_RGBA32F> {
    typedef float4 type;
    static BRT_DEV float4 make(float4 v) { return v; }
};
template <> struct OutPixel<BRT_FLAG_OUT_RGBA8_UNORM_SRGB> {
    typedef uint32_t type;
    static BRT_DEV uint32_t make(float4 v) { return encode_srgb8(v.x) | (encode_srgb8(v.y) << 8) | (encode_srgb8(v.z) << 16) | (encode_unorm8(v.w) << 24); }
};
template <> struct OutPixel<BRT_FLAG_OUT_RGBA8_UNORM> {
    typedef uint32_t type;
    static BRT_DEV uint32_t make(float4 v) { return encode_unorm8(v.x) | (encode_unorm8(v.y) << 8) | (encode_unorm8(v.z) << 16) | (encode_unorm8(v.w) << 24); }
};
template <> struct OutPixel<BRT_FLAG_OUT_RGBA16F> {
    typedef uint2 type;
    static BRT_DEV uint2 make(float4 v) {
        const uint32_t x = __half_as_ushort(__float2half_rn(v.x)), y = __half_as_ushort(__float2half_rn(v.y));
        const uint32_t z = __half_as_ushort(__float2half_rn(v.z)), w = __half_as_ushort(__float2half_rn(v.w));
        return make_uint2(x | (y << 16), z | (w << 16));
    }
};

}  // namespace brt
