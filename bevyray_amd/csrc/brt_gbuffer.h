// brt_gbuffer.h -- the G-buffer of a frame (DESIGN.md "G-buffer"): THE RULE, one pixel's depth, normal, status bits and previous pixel
// position from its pixel-centre ray and first hit, that the kernel (brt_gbuffer.hip) and the host twin (brt_host_gbuffer_pixel,
// brt_api_gbuffer.cpp) both call; tests/gbuffer_ref.py restates it in numpy.  f32, every operation separately rounded
// (-ffp-contract=off) and in the order written here; sqrt and `/` are the correctly rounded ones on both sides.
//
// The caller brings the ray and the hit: d = camera_ray_dir_center(fp, 2 uvx - 1, 1 - 2 uvy) with uv = (p + 0.5) / size (what
// denoise_guides_pixel and brt_host_pixel_ray cast), o = cam_pos, t (+INF: a miss; a NaN reads as a miss), the hit sphere's {centre, r^2}
// now and in the previous frame.  The rule, in this order:
//   1. hit      X = o + t d (ray_at), n = normalize(X - c_new) (not flipped), FRONT_FACE = dot(d, n) < 0.  A miss: n = 0.
//   2. depth    VIEW: near / (t * dot(d, fwd)), fwd = normalize(direction) once per call; a miss +0.0.  SHADER: t > far ? -1 : near / t
//               (raytrace.wgsl:108-113 applied to the centre ray); a miss: the same test on the level's fallback_far (gv.miss_depth, once
//               per call).  DISTANCE: t; a miss +INF.
//   3. motion   MOVED = the two sphere records differ bitwise.  Then X_prev = c_old + (X - c_new) * (sqrt(q_old) / sqrt(q_new)).
//               v = X_prev - o_prev; a miss: v = d (the sky turns with the camera, no translation).  The previous camera bitwise the
//               current one and not MOVED: (x', y') = (px, py).  Else k_temporal's expressions (brt_temporal.hip): z, a, b = the cofactor
//               rows of the previous camera dotted with v; z > 0: ndc_x = ((a / z) / tan_half) / aspect, ndc_y = (b / z) / tan_half,
//               x' = ((ndc_x + 1) * 0.5) * W - 0.5, y' = ((1 - ndc_y) * 0.5) * H - 0.5; else NaN.  Outside (-1, W) x (-1, H) (a NaN
//               included): NO_PREVIOUS, (x', y') = NaN, motion (0, 0).  Else motion = uv - uv_prev, uv_prev = ((x' + 0.5) / W,
//               (y' + 0.5) / H): the identity case is exactly (+0.0, +0.0).
// k_temporal's reprojection is RESTATED here, not shared with it through a header: brt_temporal.hip stays as it is, instruction for
// instruction (profiles/gbuffer/kernel_isa_diff.txt).
#pragma once
#include <cmath>
#include <cstdint>

#include "brt_ploc.h"   // BRT_HD

namespace brt {

enum GbufferDepth : uint32_t { GBUF_DEPTH_VIEW = 0u, GBUF_DEPTH_SHADER = 1u, GBUF_DEPTH_DISTANCE = 2u };
enum GbufferStatus : uint32_t { GBUF_HIT = 1u, GBUF_FRONT_FACE = 2u, GBUF_MOVED = 4u, GBUF_NO_PREVIOUS = 8u };

// What the rule reads of the current camera, under FrameParams' names (brt_layout.h): the kernel passes its FrameParams, the host twin
// a GbufferCam filled with make_frame_params' expressions (gbuffer_cam_of)
struct GbufferCam {
    float cam_pos[3], cam_dir[3], cam_up[3], cam_right[3];      // right = cross(direction, up)
    float aspect, tan_half_fov;
    float near_, far_;
};
// ... and the terms of a call (kernel arguments, wave-uniform)
struct GbufferView {
    float fwd[3];               // normalize(direction)
    float miss_depth;           // DEPTH_SHADER: the depth of a miss
    float prev_o[3];            // the previous camera: position ...
    float prev_inv[3][3];       // ... cofactor rows (R x U, U x D, D x R) / det, det = D . (R x U): TemporalCamera's
    float prev_aspect, prev_tan_half_fov;
    uint32_t same_camera;       // the previous camera is bitwise the current one
};

struct GbufferPixel {
    float depth;
    uint32_t status;            // GbufferStatus bits
    float n[3];
    float xp, yp;               // NaN under NO_PREVIOUS
    float mu, mv;               // uv - uv_prev; (0, 0) under NO_PREVIOUS
};

BRT_HD uint32_t gbuffer_bits(float f) { union { float f; uint32_t u; } c; c.f = f; return c.u; }
BRT_HD float gbuffer_float(uint32_t u) { union { float f; uint32_t u; } c; c.u = u; return c.f; }
BRT_HD float gbuffer_dot(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// mode: the depth mode of the call's descriptor (wave-uniform in the kernel, which reads it behind the walk)
template <class Cam>
BRT_HD void gbuffer_pixel(const Cam& c, const GbufferView& gv, uint32_t mode, uint32_t W, uint32_t H, uint32_t px, uint32_t py,
                          const float d[3], float t, const float sn[4], const float so[4], GbufferPixel& g) {
    const float inf = __builtin_inff(), nan = __builtin_nanf("");
    const bool hit = t < inf;
    uint32_t status = 0u;
    float v[3];
    bool moved = false;
    if (hit) {
        status = GBUF_HIT;
        float x[3], w[3];
        for (int k = 0; k < 3; k++) {
            x[k] = c.cam_pos[k] + t * d[k];
            w[k] = x[k] - sn[k];
        }
        const float len = __builtin_sqrtf(gbuffer_dot(w, w));
        for (int k = 0; k < 3; k++) g.n[k] = w[k] / len;
        if (gbuffer_dot(d, g.n) < 0.0f) status |= GBUF_FRONT_FACE;
        if (mode == GBUF_DEPTH_VIEW) g.depth = c.near_ / (t * gbuffer_dot(d, gv.fwd));
        else if (mode == GBUF_DEPTH_SHADER) g.depth = t > c.far_ ? -1.0f : c.near_ / t;
        else g.depth = t;
        moved = gbuffer_bits(sn[0]) != gbuffer_bits(so[0]) || gbuffer_bits(sn[1]) != gbuffer_bits(so[1]) ||
                gbuffer_bits(sn[2]) != gbuffer_bits(so[2]) || gbuffer_bits(sn[3]) != gbuffer_bits(so[3]);
        if (moved) {
            status |= GBUF_MOVED;
            const float s = __builtin_sqrtf(so[3]) / __builtin_sqrtf(sn[3]);
            for (int k = 0; k < 3; k++) x[k] = so[k] + (x[k] - sn[k]) * s;
        }
        for (int k = 0; k < 3; k++) v[k] = x[k] - gv.prev_o[k];
    } else {
        for (int k = 0; k < 3; k++) {
            g.n[k] = 0.0f;
            v[k] = d[k];
        }
        g.depth = mode == GBUF_DEPTH_VIEW ? 0.0f : (mode == GBUF_DEPTH_SHADER ? gv.miss_depth : inf);
    }
    float xp = nan, yp = nan;
    if (gv.same_camera && !moved) {
        xp = (float)px;
        yp = (float)py;
    } else {
        const float z = gbuffer_dot(gv.prev_inv[0], v);
        const float a = gbuffer_dot(gv.prev_inv[1], v);
        const float b = gbuffer_dot(gv.prev_inv[2], v);
        if (z > 0.0f) {
            const float ndc_x = ((a / z) / gv.prev_tan_half_fov) / gv.prev_aspect;
            const float ndc_y = (b / z) / gv.prev_tan_half_fov;
            xp = ((ndc_x + 1.0f) * 0.5f) * (float)W - 0.5f;
            yp = ((1.0f - ndc_y) * 0.5f) * (float)H - 0.5f;
        }
    }
    if (!(xp > -1.0f && xp < (float)W && yp > -1.0f && yp < (float)H)) {
        status |= GBUF_NO_PREVIOUS;
        xp = yp = nan;
        g.mu = g.mv = 0.0f;
    } else {
        const float uvx = ((float)px + 0.5f) / (float)W, uvy = ((float)py + 0.5f) / (float)H;
        g.mu = uvx - (xp + 0.5f) / (float)W;
        g.mv = uvy - (yp + 0.5f) / (float)H;
    }
    g.xp = xp;
    g.yp = yp;
    g.status = status;
}

// ---- the encoded planes ----

// One channel of an Rgb10a2Unorm texel: u32(floor(clamp(n * 0.5 + 0.5, 0, 1) * 1023 + 0.5)); a NaN gives 0
BRT_HD uint32_t gbuffer_unorm10(float n) {
    const float x = n * 0.5f + 0.5f;
    const float cl = x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f;       // (a NaN fails the first test: 0)
    return (uint32_t)__builtin_floorf(cl * 1023.0f + 0.5f);
}
// R in the low bits, alpha = 3; a miss (hit false) is a zero word
BRT_HD uint32_t gbuffer_rgb10a2(const float n[3], bool hit) {
    if (!hit) return 0u;
    return gbuffer_unorm10(n[0]) | (gbuffer_unorm10(n[1]) << 10) | (gbuffer_unorm10(n[2]) << 20) | (3u << 30);
}
// f32 -> f16 bits, round to nearest even, overflow to infinity, subnormals kept, a NaN stays a quiet NaN: what v_cvt_f16_f32
// (brt_store.h's conversion) returns, in integer arithmetic for the host twin
BRT_HD uint32_t gbuffer_f16(float f) {
    const uint32_t u = gbuffer_bits(f), sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return sign | 0x7e00u | ((a >> 13) & 0x3ffu);        // NaN: quiet, payload's top bits
    if (a >= 0x47800000u) return sign | 0x7c00u;                              // >= 65536 (INF included): infinity
    if (a < 0x33000000u) return sign;                                         // < 2^-25: rounds to zero
    uint32_t mant = a & 0x7fffffu, shift;
    const int32_t e = (int32_t)(a >> 23) - 127;
    uint32_t base;
    if (e < -14) {                       // a subnormal half: the implicit bit joins the mantissa
        mant |= 0x800000u;
        shift = (uint32_t)(-e - 14) + 13u;      // 14 .. 24
        base = 0u;
    } else {
        shift = 13u;
        base = (uint32_t)(e + 15) << 10;
    }
    const uint32_t q = mant >> shift, rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    uint32_t h = base + q;                       // (a carry out of the mantissa moves into the exponent: 65520 becomes infinity)
    if (rem > half || (rem == half && (q & 1u))) h++;
    return sign | h;
}

// ---- the uniform terms, on the host ----

// make_frame_params' expressions (brt_api_launch.cpp); tan_half: tan_half_fov(fov) (brt_host.h)
inline GbufferCam gbuffer_cam_of(const float position[3], const float direction[3], const float up[3], float aspect, float tan_half,
                                 float near_, float far_) {
    GbufferCam c{};
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
    c.near_ = near_;
    c.far_ = far_;
    return c;
}

// The pixel-centre direction on the host: camera_ray_dir_center (brt_device.h) operation for operation, as brt_host_pixel_ray's
template <class Cam>
inline void gbuffer_host_dir(const Cam& c, float inv_width, float inv_height, uint32_t W, uint32_t H, uint32_t px, uint32_t py, float d[3]) {
    const float uvx = ((float)px + 0.5f) / (float)W;
    const float uvy = ((float)py + 0.5f) / (float)H;
    const float ndc_x = (uvx * 2.0f - 1.0f) + inv_width * 0.0f;
    const float ndc_y = (1.0f - uvy * 2.0f) + inv_height * 0.0f;
    const float sx = (ndc_x * c.aspect) * c.tan_half_fov;
    const float sy = ndc_y * c.tan_half_fov;
    float v[3];
    for (int k = 0; k < 3; k++) v[k] = (c.cam_dir[k] + sx * c.cam_right[k]) + sy * c.cam_up[k];
    const float len = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    for (int k = 0; k < 3; k++) d[k] = v[k] / len;
}

// cur / prev: the two cameras' terms (prev == cur where the call has no previous camera).  temporal_camera's expressions
// (brt_temporal.hip) for the cofactor rows; same_camera compares what temporal_begin (brt_api_post.cpp) compares.
template <class Cam>
inline GbufferView gbuffer_view_of(const Cam& cur, const Cam& prev) {
    GbufferView gv{};
    const float* D = prev.cam_dir;
    const float* R = prev.cam_right;
    const float* U = prev.cam_up;
    auto cross = [](const float* a, const float* b, float* r) {
        r[0] = a[1] * b[2] - a[2] * b[1];
        r[1] = a[2] * b[0] - a[0] * b[2];
        r[2] = a[0] * b[1] - a[1] * b[0];
    };
    float rows[3][3];
    cross(R, U, rows[0]);
    cross(U, D, rows[1]);
    cross(D, R, rows[2]);
    const float det = (D[0] * rows[0][0] + D[1] * rows[0][1]) + D[2] * rows[0][2];
    for (int i = 0; i < 3; i++) {
        gv.prev_o[i] = prev.cam_pos[i];
        for (int j = 0; j < 3; j++) gv.prev_inv[i][j] = rows[i][j] / det;
    }
    gv.prev_aspect = prev.aspect;
    gv.prev_tan_half_fov = prev.tan_half_fov;
    const float len = sqrtf((cur.cam_dir[0] * cur.cam_dir[0] + cur.cam_dir[1] * cur.cam_dir[1]) + cur.cam_dir[2] * cur.cam_dir[2]);
    for (int k = 0; k < 3; k++) gv.fwd[k] = cur.cam_dir[k] / len;
    // the shader's own miss: the depth fallback_far = far - 1 of the level that keeps the traced sky (FallbackRaytraced) through the
    // same test as a hit's; level 1's far + 10 always fails it (-1.0), which the HIT bit lets a host substitute
    const float fb = cur.far_ - 1.0f;
    gv.miss_depth = fb > cur.far_ ? -1.0f : cur.near_ / fb;
    auto same = [](const float* a, const float* b, int n) {
        for (int i = 0; i < n; i++)
            if (gbuffer_bits(a[i]) != gbuffer_bits(b[i])) return false;
        return true;
    };
    gv.same_camera = same(cur.cam_pos, prev.cam_pos, 3) && same(cur.cam_dir, prev.cam_dir, 3) && same(cur.cam_up, prev.cam_up, 3) &&
                     same(cur.cam_right, prev.cam_right, 3) && same(&cur.aspect, &prev.aspect, 1) &&
                     same(&cur.tan_half_fov, &prev.tan_half_fov, 1) ? 1u : 0u;
    return gv;
}

}  // namespace brt
