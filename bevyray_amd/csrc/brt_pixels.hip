// brt_pixels.hip -- the sparse pixel tracer (brt_render_pixels*, and the refinement of brt_upscale_refine*; DESIGN.md "Refined
// upsampling").  A list entry names a pixel of the width x height Pure frame; its value is that frame's: the seed of a pixel depends on
// its frame coordinates alone (pixel_seed), and per pixel the draws and operations are k_trace_simple's (pixel_begin / camera_ray_dir /
// walk / shade_segment), whichever form runs it.  The kernels are k_list_plain and k_list_stream (brt_pixels_dev.h) under the rule of a
// whole pixel that starts at the pinhole; brt_lens.hip instantiates them under the lens rule, brt_progressive.hip under the rule of a
// pixel that is continued from its record.
#include <hip/hip_runtime.h>

#include "brt_pixels_dev.h"

namespace brt {

// a sample starts as k_trace_simple's does (raytrace.wgsl:162, :175-186); every entry names its pixel
struct PinholeStart : WholePixel {
    static BRT_DEV uint32_t pixel_of(const FrameParams&, const PixelsArgs& pa, uint32_t i) { return pa.pixels[i]; }
    static BRT_DEV void sample(const FrameParams& fp, const PixelState& ps, uint32_t& rng, f3& o, f3& d) {
        d = camera_ray_dir(fp, ps.ndc0x, ps.ndc0y, rng);
        o = mk3(fp.cam_pos[0], fp.cam_pos[1], fp.cam_pos[2]);
    }
};

hipError_t launch_trace_pixels(const PixelsLaunch& pl) { return launch_list<PinholeStart>(pl, false); }

}  // namespace brt
