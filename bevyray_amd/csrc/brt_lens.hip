// brt_lens.hip -- Pure frames and pixel lists under the lens rule (brt_render_lens*; DESIGN.md "Lens frames"): the two forms of the
// sparse pixel tracer (k_list_plain, k_list_stream: brt_pixels_dev.h) under a rule of its own -- a whole pixel whose samples start with
// THE LENS RULE (brt_lens.h: a pinhole, a thin lens or an orthographic ray; the kernels are compiled per mode) where brt_pixels.hip calls
// camera_ray_dir and takes the camera's position, and a null list means that entry i is pixel i, in raster order.  Everything else
// is the shared kernels' and WholePixel's: pixels_begin's seed, walk / shade_segment, the value and its store, the counter claim of a
// round, the launch.  The lens terms are kernel arguments (scalar registers); a lane's origin is the `o` a path carries anyway.
#include <hip/hip_runtime.h>

#include "brt_pixels_dev.h"

namespace brt {

template <uint32_t LENS>
struct LensStart : WholePixel {
    static BRT_DEV uint32_t pixel_of(const FrameParams&, const PixelsArgs& pa, uint32_t i, const LensView&) { return pa.pixels ? pa.pixels[i] : i; }
    static BRT_DEV void sample(const FrameParams& fp, const PixelState& ps, uint32_t& rng, f3& o, f3& d, const LensView& lv) {
        float oo[3], w[3];
        const bool raw = lens_ray_raw(fp, lv, LENS, ps.ndc0x, ps.ndc0y, rng, oo, w);
        o = mk3(oo[0], oo[1], oo[2]);
        d = mk3(w[0], w[1], w[2]);
        if (raw) d = normalize3(d);
    }
};

hipError_t launch_trace_lens(const PixelsLaunch& pl, const LensView& lens) {
    switch (lens.mode) {
        case LENS_PINHOLE: return launch_list<LensStart<LENS_PINHOLE>>(pl, true, lens);
        case LENS_THIN: return launch_list<LensStart<LENS_THIN>>(pl, true, lens);
        case LENS_ORTHO: return launch_list<LensStart<LENS_ORTHO>>(pl, true, lens);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace brt
