// brt_lens.h -- thin-lens depth of field and orthographic projection for Pure frames (DESIGN.md "Lens frames"): THE LENS RULE, one
// sample's primary ray, that the kernels (brt_lens.hip) and the host twin (brt_host_lens_ray, brt_api_lens.cpp) both call;
// tests/lens_ref.py restates it in numpy.  f32, every operation separately rounded (-ffp-contract=off) and in the order written here.
//
// The pixel's seed is pixel_seed unchanged (raytrace.wgsl:95); its samples share one RNG state.  One sample, in this order:
//   1. jitter   rx = draw - 0.5, ry = draw - 0.5 (two draws, random.wgsl:3-6); ndc_x = ndc0x + inv_width * rx, ndc_y = ndc0y +
//               inv_height * ry -- camera_dir_raw's (brt_device.h).  Every mode draws them.
//   2. pinhole  (perspective, aperture_radius == 0)  sx = (ndc_x * aspect) * tan_half_fov, sy = ndc_y * tan_half_fov,
//               v = (direction + sx * right) + sy * up; o = position, w = v.  No further draw.
//   3. thin     (perspective, aperture_radius r > 0)  v as in 2.  A point of the unit disk by rejection, the image of
//               randomVec3InUnitSphere (random.wgsl:17-26) in two dimensions: x = 2 * draw - 1, then y = 2 * draw - 1 (each rounded once,
//               as the unit-ball sampler's coordinates are), accepted when x * x + y * y <= 1.0.  lx = r * x, ly = r * y,
//               l = lx * right + ly * up, o = position + l, w = focus_distance * v - l: whatever the disk point, o + w is
//               position + focus_distance * v, a point of the plane at focus_distance along `direction`.
//   4. ortho    (projection_type 1)  half = 0.5 * ortho_height (once per call); ax = (ndc_x * aspect) * half, ay = ndc_y * half,
//               o = (position + ax * right) + ay * up; d = normalize(direction), the same for every sample (once per call: ortho_dir).
//               No lens draw; fov, near and far are not read.
//   5. d = normalize(w): sqrt((w.x * w.x + w.y * w.y) + w.z * w.z), three quotients -- normalize3 of brt_device.h on the device, whose
//      short form is the correctly rounded sqrt and quotient that lens_normalize's are on the host.
// raytrace(Ray(o, d)) then runs at level 3 on the same RNG state (raytrace.wgsl:174-224).
//
// The rejection loop ends for whatever the camera and the lens hold: its test reads the two draws alone, which are finite and in
// [-1, 1]; a NaN or infinite radius, position or axis only reaches the products behind it (and brt_render_lens* refuses such a radius).
// Like the shader's unit-ball loop it is as long as the RNG's orbit makes it.
#pragma once
#include <cmath>
#include <cstdint>

#include "brt_ploc.h"   // BRT_HD

namespace brt {

enum LensMode : uint32_t { LENS_PINHOLE = 0u, LENS_THIN = 1u, LENS_ORTHO = 2u };

// What the rule reads, uniform over a call.  The camera terms, under FrameParams' names (brt_layout.h): the kernels pass their
// FrameParams, the host twin a LensCam filled with make_frame_params' expressions (lens_cam_of) ...
struct LensCam {
    float cam_pos[3], cam_dir[3], cam_up[3], cam_right[3];      // right = cross(direction, up)
    float aspect, tan_half_fov;
    float inv_width, inv_height;                // 1.0 / (f32(window.height) * aspect), 1.0 / f32(window.height)
};
// ... and the lens terms (kernel arguments: seven scalar registers)
struct LensView {
    uint32_t mode;                              // LensMode
    float radius, focus;                        // LENS_THIN
    float half;                                 // LENS_ORTHO: 0.5 * ortho_height
    float ortho_dir[3];                         // LENS_ORTHO: normalize(direction)
};

// random.wgsl:8-15 and :3-6 (rng_next / rng_float of brt_device.h); lens_rng_coord: 2 * draw - 1 rounded once (rng_ball_coord)
BRT_HD uint32_t lens_rng_next(uint32_t state) {
    const uint32_t old = state + 747796405u + 2891336453u;
    const uint32_t word = ((old >> ((old >> 28u) + 4u)) ^ old) * 277803737u;
    return (word >> 22u) ^ word;
}
BRT_HD float lens_rng_float(uint32_t& state) {
    state = lens_rng_next(state);
    return (float)state * 2.3283064365386963e-10f;
}
BRT_HD float lens_rng_coord(uint32_t& state) {
    state = lens_rng_next(state);
    return __builtin_fmaf((float)state, 4.656612873077392578125e-10f, -1.0f);
}

// Steps 1-4.  mode: lv.mode (the kernels are compiled per mode and pass a constant).  true: w is to be normalised (step 5); false: w
// is the call's unit direction already (ortho).
template <class Cam>
BRT_HD bool lens_ray_raw(const Cam& c, const LensView& lv, uint32_t mode, float ndc0x, float ndc0y, uint32_t& rng, float o[3], float w[3]) {
    const float rx = lens_rng_float(rng) - 0.5f;
    const float ry = lens_rng_float(rng) - 0.5f;
    const float ndc_x = ndc0x + c.inv_width * rx;
    const float ndc_y = ndc0y + c.inv_height * ry;
    if (mode == LENS_ORTHO) {
        const float ax = (ndc_x * c.aspect) * lv.half;
        const float ay = ndc_y * lv.half;
        for (int k = 0; k < 3; k++) {
            o[k] = (c.cam_pos[k] + ax * c.cam_right[k]) + ay * c.cam_up[k];
            w[k] = lv.ortho_dir[k];
        }
        return false;
    }
    const float sx = (ndc_x * c.aspect) * c.tan_half_fov;
    const float sy = ndc_y * c.tan_half_fov;
    float v[3];
    for (int k = 0; k < 3; k++) v[k] = (c.cam_dir[k] + sx * c.cam_right[k]) + sy * c.cam_up[k];
    if (mode != LENS_THIN) {
        for (int k = 0; k < 3; k++) {
            o[k] = c.cam_pos[k];
            w[k] = v[k];
        }
        return true;
    }
    float x, y;
    for (;;) {
        x = lens_rng_coord(rng);
        y = lens_rng_coord(rng);
        if (x * x + y * y <= 1.0f) break;
    }
    const float lx = lv.radius * x, ly = lv.radius * y;
    for (int k = 0; k < 3; k++) {
        const float l = lx * c.cam_right[k] + ly * c.cam_up[k];
        o[k] = c.cam_pos[k] + l;
        w[k] = lv.focus * v[k] - l;
    }
    return true;
}

// step 5 on the host (and what normalize3 computes on the device)
inline void lens_normalize(const float w[3], float d[3]) {
    const float len = sqrtf((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    d[0] = w[0] / len;
    d[1] = w[1] / len;
    d[2] = w[2] / len;
}

// The uniform terms from the camera's and the window's fields.  lens_cam_of: make_frame_params' expressions (brt_api_launch.cpp);
// tan_half: tan_half_fov(fov) (brt_host.h) -- not read by LENS_ORTHO.
inline LensCam lens_cam_of(const float position[3], const float direction[3], const float up[3], float aspect, float tan_half,
                           uint32_t window_height) {
    LensCam c{};
    for (int k = 0; k < 3; k++) {
        c.cam_pos[k] = position[k];
        c.cam_dir[k] = direction[k];
        c.cam_up[k] = up[k];
    }
    const float* a = direction;
    const float* b = up;
    c.cam_right[0] = a[1] * b[2] - a[2] * b[1];
    c.cam_right[1] = a[2] * b[0] - a[0] * b[2];
    c.cam_right[2] = a[0] * b[1] - a[1] * b[0];
    c.aspect = aspect;
    c.tan_half_fov = tan_half;
    const float heightf = (float)window_height;
    const float widthf = (float)window_height * aspect;
    c.inv_width = 1.0f / widthf;
    c.inv_height = 1.0f / heightf;
    return c;
}
inline LensView lens_view_of(const float direction[3], uint32_t projection_type, float aperture_radius, float focus_distance,
                             float ortho_height) {
    LensView lv{};
    lv.mode = projection_type == 1u ? LENS_ORTHO : (aperture_radius > 0.0f ? LENS_THIN : LENS_PINHOLE);
    lv.radius = aperture_radius;
    lv.focus = focus_distance;
    lv.half = 0.5f * ortho_height;
    lens_normalize(direction, lv.ortho_dir);
    return lv;
}

// A 1-norm that no origin of the rule exceeds, rounding included (+INF or NaN: none can be given).  In double, from the exact bounds
// |x|, |y| <= 1 and |ndc| <= 1 + |inv| / 2 (uv lies in (0, 1), the jitter in [-0.5, 0.5]): an origin component is at most six f32
// operations deep (thin: r * x, its product with an axis, the sum of two, the sum with the position; ortho: ndc, * aspect, * half,
// * axis, two sums -- on terms of one sign at worst), each of relative error <= 2^-24 or, in the subnormal range, of absolute error
// <= 2^-150: the factor 1 + 2^-20 covers (1 + 2^-24)^8, the term 2^-140 eight such absolute errors in each component.  Rounded up
// to f32.
inline float lens_origin_bound(const LensCam& c, const LensView& lv) {
    auto n1 = [](const float v[3]) { return (std::fabs((double)v[0]) + std::fabs((double)v[1])) + std::fabs((double)v[2]); };
    double b = n1(c.cam_pos);
    if (lv.mode == LENS_THIN) b += (double)lv.radius * (n1(c.cam_right) + n1(c.cam_up));
    if (lv.mode == LENS_ORTHO) {
        const double nx = 1.0 + 0.5 * std::fabs((double)c.inv_width), ny = 1.0 + 0.5 * std::fabs((double)c.inv_height);
        const double half = std::fabs((double)lv.half);
        b += (nx * std::fabs((double)c.aspect)) * half * n1(c.cam_right) + ny * half * n1(c.cam_up);
    }
    b = b * (1.0 + 0x1p-20) + 0x1p-140;
    float f = (float)b;
    if ((double)f < b) f = std::nextafter(f, INFINITY);
    return f;
}

}  // namespace brt
