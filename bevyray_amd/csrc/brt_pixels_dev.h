// brt_pixels_dev.h -- what the kernels that trace a list of pixels share on the device (brt_pixels.hip, brt_lens.hip): a list's length,
// an entry's store and refusal, the wave's counts, a pixel's begin and value.  Device code: included by those two files only.
#pragma once
#include "brt_pixels.h"
#include "brt_store.h"
#include "brt_stream.h"

namespace brt {

// the wave's counts into pa.stat (all lanes of the wave call it)
BRT_DEV void pixels_count(const PixelsArgs& pa, uint32_t rays, uint32_t refused) {
    if (!pa.stat) return;
    rays = wave_sum(rays);
    refused = wave_sum(refused);
    if (lane_id() == 0u) {
        if (rays) atomicAdd(pa.stat + 0, (unsigned long long)rays);
        if (refused) atomicAdd(pa.stat + 1, (unsigned long long)refused);
    }
}

BRT_DEV uint32_t pixels_n(const PixelsArgs& pa) {
    if (!pa.count) return pa.n_pixels;
    const uint32_t n = *pa.count;
    return n < pa.n_pixels ? n : pa.n_pixels;
}

// entry i, pixel p: its value where the call wants it
BRT_DEV void pixels_store(const PixelsArgs& pa, uint32_t i, uint32_t p, float4 v) {
    if (!pa.scatter) {
        reinterpret_cast<float4*>(pa.out)[i] = v;
        return;
    }
    switch (pa.out_format) {
        case BRT_FLAG_OUT_RGBA8_UNORM_SRGB: reinterpret_cast<uint32_t*>(pa.out)[p] = OutPixel<BRT_FLAG_OUT_RGBA8_UNORM_SRGB>::make(v); break;
        case BRT_FLAG_OUT_RGBA16F: reinterpret_cast<uint2*>(pa.out)[p] = OutPixel<BRT_FLAG_OUT_RGBA16F>::make(v); break;
        case BRT_FLAG_OUT_RGBA8_UNORM: reinterpret_cast<uint32_t*>(pa.out)[p] = OutPixel<BRT_FLAG_OUT_RGBA8_UNORM>::make(v); break;
        default: reinterpret_cast<float4*>(pa.out)[p] = OutPixel<BRT_FLAG_OUT_RGBA32F>::make(v); break;
    }
}

// entry i names no pixel of the frame
BRT_DEV void pixels_refuse(const PixelsArgs& pa, uint32_t i) {
    if (!pa.scatter) reinterpret_cast<float4*>(pa.out)[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

BRT_DEV void pixels_begin(const FrameParams& fp, uint32_t p, PixelState& ps) {
    PixelCoord c;
    c.py = p / fp.width;
    c.px = p - c.py * fp.width;
    c.local_row = c.py;
    c.tile = 0u;
    c.t = 0u;
    c.inside = true;
    pixel_begin(fp, c, ps);
}

// the Pure frame's value of a pixel whose samples have ended (pixel_finish<true>, raytrace.wgsl:169, :122)
BRT_DEV float4 pixels_value(const FrameParams& fp, const PixelState& ps) {
    return make_float4(ps.sum.x / fp.spp_f, ps.sum.y / fp.spp_f, ps.sum.z / fp.spp_f, 1.0f);
}


}  // namespace brt
