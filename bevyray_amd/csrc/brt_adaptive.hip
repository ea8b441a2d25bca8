// brt_adaptive.hip -- adaptive sampling: which pixels of a base frame are traced again at the camera's own sample count.  The rule is
// pinned in brt_adaptive.h (shared with the host) and DESIGN.md "Adaptive sampling"; tests/adaptive_ref.py restates it in numpy.
//
// k_adaptive_select   one thread per pixel p, 256 threads = one 16x16 tile (a wave is 4 rows of 16).  The workgroup first stages
//                     {luminance, material id} of its tile and a 2-pixel apron in LDS (20 x 20 entries of 8 bytes: the 25 taps of a
//                     pixel overlap its neighbours', and the luminance of a base pixel is computed once instead of 25 times); an entry
//                     outside the frame holds a NaN luminance, which no tap counts.  Then every thread evaluates the rule from LDS, stores
//                     the base value of p in the requested BRT_FLAG_OUT_* format (OutPixel, brt_store.h) and, if p has a class, appends p
//                     to the call's list: one ballot and one atomicAdd per wave, none in a wave without a selected lane.  The output is
//                     never read.  MASK_ONLY: the class byte of every pixel, nothing else.  Deterministic apart from the list's order.
#include <hip/hip_runtime.h>

#include "brt_adaptive.h"
#include "brt_store.h"
#include "brt_wave.h"

namespace brt {

namespace {

constexpr uint32_t kTile = 16;
constexpr uint32_t kSpan = kTile + 2u * (uint32_t)kAdaptRadius;      // the tile and its apron

struct AdaptiveArgs {
    uint32_t width, height;
    float threshold;
    uint32_t min_taps;
    const float4* base;
    const float4* g0;
    const float4* g1;
    uint32_t* count;
    uint32_t* list;
    uint8_t* mask;
};

template <uint32_t FMT, bool MASK_ONLY>
__global__ __launch_bounds__(256) void k_adaptive_select(AdaptiveArgs aa, typename OutPixel<FMT>::type* __restrict__ out) {
    __shared__ uint2 tile[kSpan * kSpan];      // {luminance bits, material id}
    const int x0 = (int)(blockIdx.x * kTile) - kAdaptRadius, y0 = (int)(blockIdx.y * kTile) - kAdaptRadius;
    for (uint32_t i = threadIdx.x; i < kSpan * kSpan; i += 256u) {
        const int tx = x0 + (int)(i % kSpan), ty = y0 + (int)(i / kSpan);
        uint2 e = make_uint2(0x7fc00000u, 0u);      // outside the frame: a NaN luminance
        if (tx >= 0 && tx < (int)aa.width && ty >= 0 && ty < (int)aa.height) {
            const uint32_t q = (uint32_t)ty * aa.width + (uint32_t)tx;
            const float4 c = aa.base[q];
            e = make_uint2(__float_as_uint(adapt_luma(c.x, c.y, c.z)), __float_as_uint(aa.g1[q].w));
        }
        tile[i] = e;
    }
    __syncthreads();
    const uint32_t lx = threadIdx.x & (kTile - 1u), ly = threadIdx.x / kTile;
    const uint32_t px = blockIdx.x * kTile + lx, py = blockIdx.y * kTile + ly;
    const bool inside = px < aa.width && py < aa.height;
    const uint32_t p = py * aa.width + px;
    uint32_t cls = 0u;
    if (inside) {
        const uint32_t at = (ly + (uint32_t)kAdaptRadius) * kSpan + lx + (uint32_t)kAdaptRadius;
        const uint2 own = tile[at];
        cls = adapt_classify(aa.g0[p].w, own.y, __uint_as_float(own.x), aa.threshold, aa.min_taps,
                             [&](int dx, int dy, uint32_t* id_q, float* l_q) {
                                 const uint2 e = tile[(int)at + dy * (int)kSpan + dx];
                                 *l_q = __uint_as_float(e.x);
                                 *id_q = e.y;
                                 return true;
                             });
    }
    if constexpr (MASK_ONLY) {
        if (inside) aa.mask[p] = (uint8_t)cls;
    } else {
        if (inside) out[p] = OutPixel<FMT>::make(aa.base[p]);
        wave_append(aa.count, aa.list, cls != 0u, p);
    }
}

template <uint32_t FMT, bool MASK_ONLY>
void launch_t(const AdaptiveArgs& aa, void* out, hipStream_t stream) {
    const dim3 grid((aa.width + kTile - 1u) / kTile, (aa.height + kTile - 1u) / kTile);
    hipLaunchKernelGGL((k_adaptive_select<FMT, MASK_ONLY>), grid, dim3(256), 0, stream, aa, reinterpret_cast<typename OutPixel<FMT>::type*>(out));
}

}  // namespace

hipError_t launch_adaptive_select(const AdaptiveSelect& as, hipStream_t stream) {
    if (as.width == 0u || as.height == 0u || as.width > 32768u || as.height > 32768u || !as.base || !as.g0 || !as.g1) return hipErrorInvalidValue;
    if (as.mask ? false : (!as.out || !as.count || !as.list)) return hipErrorInvalidValue;
    const AdaptiveArgs aa = {as.width, as.height, as.threshold, as.min_taps, as.base, as.g0, as.g1, as.count, as.list, as.mask};
    if (as.mask) {
        launch_t<BRT_FLAG_OUT_RGBA32F, true>(aa, nullptr, stream);
        return hipGetLastError();
    }
    switch (as.out_format) {
        case BRT_FLAG_OUT_RGBA32F: launch_t<BRT_FLAG_OUT_RGBA32F, false>(aa, as.out, stream); break;
        case BRT_FLAG_OUT_RGBA8_UNORM_SRGB: launch_t<BRT_FLAG_OUT_RGBA8_UNORM_SRGB, false>(aa, as.out, stream); break;
        case BRT_FLAG_OUT_RGBA16F: launch_t<BRT_FLAG_OUT_RGBA16F, false>(aa, as.out, stream); break;
        case BRT_FLAG_OUT_RGBA8_UNORM: launch_t<BRT_FLAG_OUT_RGBA8_UNORM, false>(aa, as.out, stream); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace brt
