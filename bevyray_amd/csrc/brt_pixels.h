// brt_pixels.h -- host-callable launchers of the sparse pixel tracer (brt_pixels.hip, brt_lens.hip; the kernels: brt_pixels_dev.h).  The
// rules: DESIGN.md "Refined upsampling" and "Lens frames".
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "brt_kernels.h"
#include "brt_lens.h"

namespace brt {

// One list of pixels of the width x height Pure frame of `frame`.  Entry i names pixel p = py * width + px; its value is what the frame
// holds there ({rgb, 1}).  Packed: entry i is stored at out[i] as RGBA32F; scatter: at out[p] of a width x height frame in out_format.
// An entry >= width * height is never traced: packed it stores four zeros, scattered it stores nothing; both count it as refused.
struct PixelsArgs {
    const uint32_t* pixels;
    uint32_t n_pixels;          // entries of the list (its capacity when count is set)
    const uint32_t* count;      // a device word that holds the number of entries, read by the kernel (nullptr: n_pixels)
    void* out;
    uint32_t scatter;           // 0: packed RGBA32F; 1: out[p] in out_format
    uint32_t out_format;        // BRT_FLAG_OUT_* (scatter only)
    unsigned long long* stat;   // [0] rays, [1] refused entries, zeroed by the caller (nullptr: not counted)
    uint32_t* counter;          // streaming form: the batch counter, zeroed by the caller
};

struct PixelsLaunch : StreamLaunch {
    FrameParams frame;          // one part, level 3, the default policy
    PixelsArgs args;
};
hipError_t launch_trace_pixels(const PixelsLaunch& pl);

// The same list under the lens rule (brt_lens.h, brt_lens.hip): a sample's primary ray is lens_ray_raw's instead of the pinhole's.
// args.pixels may be null: entry i is pixel i (a whole frame, n_pixels = width * height).
hipError_t launch_trace_lens(const PixelsLaunch& pl, const LensView& lens);

}  // namespace brt
