// brt_temporal.hip -- temporal reprojection and accumulation of Pure-level frames (BRT_FLAG_TEMPORAL).  The formulas are pinned in
// DESIGN.md section 11; tests/temporal_ref.py restates them in numpy.
//
// k_temporal  one thread per pixel, after the denoiser's guides and demodulation: the pixel's first hit X = o + t d is carried back
//             through the motion of its sphere and projected into the previous camera; the four bilinear taps of the previous history
//             around that position are validated (same sphere and material, normals, distance), and the surviving ones give the
//             history the demodulated colour c' is blended into with alpha = 1 / n.  Writes the next history set, and either {h, n}
//             into the filter's input plane or the remodulated frame h a in the requested BRT_FLAG_OUT_* format.
// k_temporal<true, FMT, const float4*>  the same with the raster colour bound, on a coverage frame: covered pixels store their texel.
// 256 threads = one 16x16 pixel tile, as the denoise kernels; no atomics, a fixed tap order (bitwise deterministic).
#include <hip/hip_runtime.h>

#include "brt_store.h"
#include "brt_temporal.h"

namespace brt {

namespace {

constexpr uint32_t kTile = 16;

BRT_DEV float luminance(float4 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }
BRT_DEV bool same_bits(float4 a, float4 b) {
    return __float_as_uint(a.x) == __float_as_uint(b.x) && __float_as_uint(a.y) == __float_as_uint(b.y) &&
           __float_as_uint(a.z) == __float_as_uint(b.z) && __float_as_uint(a.w) == __float_as_uint(b.w);
}

struct Kernel {
    FrameParams fp, pp;           // this frame's and the previous temporal frame's parameters
    TemporalCamera cam;           // pp's camera, inverted
    TemporalArgs ta;
    const float4* g0;
    const float4* g1;
    const float2* aux;
    const uint32_t* sid;
    const float4* in;             // a copy of the input frame (RGBA32F) the demodulation made: d_out may be the input itself
    float4* dm;                   // the demodulated input {c', 0 or -1}; {h, n} after a TEMPORAL | DENOISE frame
    const float4 *a_in, *b_in, *c_in;
    float4 *a_out, *b_out, *c_out;
    float2* xy;
};

}  // namespace

// Raster: empty, or one `const float4*` -- a coverage frame, in which a covered pixel (alpha +0.0 in the input, a
// miss in the guides, so it passes through) stores its raster texel (nullptr: zeros) instead of the input's zeros.  The empty pack is the
// kernel as it always was, name and arguments included.
template <bool STORE, uint32_t FMT, typename... Raster>
__global__ __launch_bounds__(256) void k_temporal(Kernel k, typename OutPixel<FMT>::type* __restrict__ out, Raster... raster) {
    const uint32_t px = blockIdx.x * kTile + (threadIdx.x & (kTile - 1u)), py = blockIdx.y * kTile + threadIdx.x / kTile;
    const uint32_t W = k.fp.width, H = k.fp.height;
    if (px >= W || py >= H) return;
    const uint32_t p = py * W + px;
    const float4 gp = k.g0[p], cd = k.dm[p];
    const uint32_t sp = k.sid[p], mp = __float_as_uint(k.g1[p].w);
    const float nan = __builtin_nanf("");
    k.a_out[p] = gp;
    if (cd.w < 0.0f) {                                       // sky / non-finite colour: passes through, no history
        k.b_out[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        k.c_out[p] = make_float4(0.0f, 0.0f, __uint_as_float(sp), __uint_as_float(mp));
        k.xy[p] = make_float2(nan, nan);
        if constexpr (STORE && sizeof...(Raster) != 0) {
            if (covered(k.in[p].w)) {
                out[p] = OutPixel<FMT>::make(raster_texel(p, raster...));
                return;
            }
        }
        if (STORE) out[p] = OutPixel<FMT>::make(k.in[p]);
        return;
    }
    // ---- reproject: X = o + t d, carried by its sphere's motion, into the previous camera
    float xp = nan, yp = nan, dist = 0.0f;
    if (k.ta.has_history) {
        const float uvx = ((float)px + 0.5f) / (float)W;
        const float uvy = ((float)py + 0.5f) / (float)H;
        const f3 d = camera_ray_dir_center(k.fp, uvx * 2.0f - 1.0f, 1.0f - uvy * 2.0f);
        const f3 o = mk3(k.fp.cam_pos[0], k.fp.cam_pos[1], k.fp.cam_pos[2]);
        f3 x = mk3(o.x + gp.w * d.x, o.y + gp.w * d.y, o.z + gp.w * d.z);
        bool moved = false;
        if (k.ta.motion) {
            const float4 sn = k.ta.sph_new[sp], so = k.ta.sph_old[sp];
            moved = !same_bits(sn, so);
            if (moved) {       // X_prev = c_old + (X - c_new) r_old / r_new
                const float s = __builtin_sqrtf(so.w) / __builtin_sqrtf(sn.w);
                x = mk3(so.x + (x.x - sn.x) * s, so.y + (x.y - sn.y) * s, so.z + (x.z - sn.z) * s);
            }
        }
        const f3 v = mk3(x.x - k.cam.o[0], x.y - k.cam.o[1], x.z - k.cam.o[2]);
        dist = __builtin_sqrtf(dot3(v, v));
        if (k.ta.same_camera && !moved) {                    // the identity: p's own history, no resampling
            xp = (float)px;
            yp = (float)py;
        } else {
            const float z = dot3(mk3(k.cam.inv[0][0], k.cam.inv[0][1], k.cam.inv[0][2]), v);
            const float a = dot3(mk3(k.cam.inv[1][0], k.cam.inv[1][1], k.cam.inv[1][2]), v);
            const float b = dot3(mk3(k.cam.inv[2][0], k.cam.inv[2][1], k.cam.inv[2][2]), v);
            if (z > 0.0f) {      // s -> ndc -> uv -> pixel: camera_ray_dir_center's mapping inverted
                const float ndc_x = ((a / z) / k.pp.tan_half_fov) / k.pp.aspect;
                const float ndc_y = (b / z) / k.pp.tan_half_fov;
                xp = ((ndc_x + 1.0f) * 0.5f) * (float)W - 0.5f;
                yp = ((1.0f - ndc_y) * 0.5f) * (float)H - 0.5f;
            }
        }
        if (!(xp > -1.0f && xp < (float)W && yp > -1.0f && yp < (float)H)) xp = yp = nan;   // (NaN fails every test)
    }
    // ---- validate the 4 bilinear taps and resample the history from the valid ones
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sn = 0.0f, s1 = 0.0f, s2 = 0.0f;
    if (xp == xp) {
        const float x0 = __builtin_floorf(xp), y0 = __builtin_floorf(yp);
        const float fx = xp - x0, fy = yp - y0;
        const f3 np = mk3(gp.x, gp.y, gp.z);
        const float theta = (2.0f * k.pp.tan_half_fov) / (float)H;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int dx = j & 1, dy = j >> 1;
            const float w = (dx ? fx : 1.0f - fx) * (dy ? fy : 1.0f - fy);
            const int qx = (int)x0 + dx, qy = (int)y0 + dy;
            if (!(w > 0.0f) || qx < 0 || qy < 0 || qx >= (int)W || qy >= (int)H) continue;
            const uint32_t q = (uint32_t)qy * W + (uint32_t)qx;
            const float4 cq = k.c_in[q];
            if (__float_as_uint(cq.z) != sp || __float_as_uint(cq.w) != mp) continue;
            const float4 aq = k.a_in[q];
            if (!(dot3(np, mk3(aq.x, aq.y, aq.z)) >= 0.9f)) continue;
            const float uqx = ((float)qx + 0.5f) / (float)W;
            const float uqy = ((float)qy + 0.5f) / (float)H;
            const f3 dq = camera_ray_dir_center(k.pp, uqx * 2.0f - 1.0f, 1.0f - uqy * 2.0f);
            const float zs = (aq.w * theta) / max_f(__builtin_fabsf(dot3(mk3(aq.x, aq.y, aq.z), dq)), 0.1f);   // the depth scale
            if (!(__builtin_fabsf(aq.w - dist) <= 0.01f * dist + 2.0f * zs)) continue;
            const float4 bq = k.b_in[q];
            if (!(bq.w > 0.0f)) continue;                   // (no history there)
            sw = sw + w;
            sr = sr + w * bq.x;
            sg = sg + w * bq.y;
            sb = sb + w * bq.z;
            sn = sn + w * bq.w;
            s1 = s1 + w * cq.x;
            s2 = s2 + w * cq.y;
        }
    }
    // ---- accumulate: n = min(n_hist + 1, max_history), h = h_hist + (c' - h_hist) / n; n = 1: c' itself
    const float l = luminance(cd);
    float4 h = make_float4(cd.x, cd.y, cd.z, 1.0f);
    float m1 = l, m2 = l * l;
    if (sw > 0.0f) {
        const float n = min_f(sn / sw + 1.0f, k.ta.max_history);
        if (n > 1.0f) {
            const float alpha = 1.0f / n;
            const float hr = sr / sw, hg = sg / sw, hb = sb / sw, h1 = s1 / sw, h2 = s2 / sw;
            h = make_float4(hr + (cd.x - hr) * alpha, hg + (cd.y - hg) * alpha, hb + (cd.z - hb) * alpha, n);
            m1 = h1 + (l - h1) * alpha;
            m2 = h2 + (l * l - h2) * alpha;
        }
    } else {
        xp = yp = nan;
    }
    k.b_out[p] = h;
    k.c_out[p] = make_float4(m1, m2, __uint_as_float(sp), __uint_as_float(mp));
    k.xy[p] = make_float2(xp, yp);
    if (STORE) {
        const float4 c = k.in[p];
        if (h.w == 1.0f) {
            out[p] = OutPixel<FMT>::make(c);                // (c / a) a need not round back to c
        } else {
            const float4 a = k.g1[p];
            out[p] = OutPixel<FMT>::make(make_float4(h.x * a.x, h.y * a.y, h.z * a.z, k.aux[p].x));
        }
    } else {
        k.dm[p] = h;
    }
}

// ---- host-callable -----------------------------------------------------------------------------------------------------------------

size_t temporal_history_bytes(uint32_t width, uint32_t height) {
    const size_t n = (size_t)width * height;
    return n * 16 * 6 + n * 8 + n * 4;   // a/b/c x 2, xy, sid
}

TemporalHistory temporal_history(char* base, uint32_t width, uint32_t height) {
    const size_t n = (size_t)width * height;
    TemporalHistory t;
    float4* f = reinterpret_cast<float4*>(base);
    for (int s = 0; s < 2; s++) {
        t.a[s] = f + (3 * s + 0) * n;
        t.b[s] = f + (3 * s + 1) * n;
        t.c[s] = f + (3 * s + 2) * n;
    }
    t.xy = reinterpret_cast<float2*>(f + 6 * n);
    t.sid = reinterpret_cast<uint32_t*>(t.xy + n);
    return t;
}

TemporalCamera temporal_camera(const FrameParams& pp) {
    // [D R U] [z, a, b]^T = v: Cramer's rule with the cofactor rows R x U, U x D, D x R (tests/temporal_ref.py: the same order)
    auto cross = [](const float* a, const float* b, float* r) {
        r[0] = a[1] * b[2] - a[2] * b[1];
        r[1] = a[2] * b[0] - a[0] * b[2];
        r[2] = a[0] * b[1] - a[1] * b[0];
    };
    const float* D = pp.cam_dir;
    const float* R = pp.cam_right;
    const float* U = pp.cam_up;
    float rows[3][3];
    cross(R, U, rows[0]);
    cross(U, D, rows[1]);
    cross(D, R, rows[2]);
    const float det = (D[0] * rows[0][0] + D[1] * rows[0][1]) + D[2] * rows[0][2];
    TemporalCamera c;
    for (int i = 0; i < 3; i++) {
        c.o[i] = pp.cam_pos[i];
        for (int j = 0; j < 3; j++) c.inv[i][j] = rows[i][j] / det;
    }
    return c;
}

static dim3 tiles_of(uint32_t width, uint32_t height) { return dim3((width + kTile - 1u) / kTile, (height + kTile - 1u) / kTile); }

template <bool STORE, uint32_t FMT>
static void launch_t(const Kernel& k, void* out, hipStream_t stream, const BlendPost& bp) {
    if (STORE && bp.on)       // (without a store nothing of a covered pixel leaves the kernel: the filter's last pass composites)
        hipLaunchKernelGGL((k_temporal<true, FMT, const float4*>), tiles_of(k.fp.width, k.fp.height), dim3(256), 0, stream, k,
                           reinterpret_cast<typename OutPixel<FMT>::type*>(out), reinterpret_cast<const float4*>(bp.d_raster_rgba));
    else
        hipLaunchKernelGGL((k_temporal<STORE, FMT>), tiles_of(k.fp.width, k.fp.height), dim3(256), 0, stream, k,
                           reinterpret_cast<typename OutPixel<FMT>::type*>(out));
}

hipError_t launch_temporal(const FrameParams& fp, const FrameParams& prev, const TemporalArgs& args, const DenoiseScratch& ds,
                           const TemporalHistory& hist, void* d_out, uint32_t out_format, hipStream_t stream, const BlendPost& bp) {
    Kernel k;
    k.fp = fp;
    k.pp = prev;
    k.cam = temporal_camera(prev);
    k.ta = args;
    k.g0 = ds.g0;
    k.g1 = ds.g1;
    k.aux = ds.aux;
    k.sid = hist.sid;
    k.in = ds.cv[0];              // (launch_denoise_demod's copy)
    k.dm = ds.dm;
    const uint32_t s = args.prev & 1u;
    k.a_in = hist.a[s];
    k.b_in = hist.b[s];
    k.c_in = hist.c[s];
    k.a_out = hist.a[s ^ 1u];
    k.b_out = hist.b[s ^ 1u];
    k.c_out = hist.c[s ^ 1u];
    k.xy = hist.xy;
    if (!d_out) {
        launch_t<false, BRT_FLAG_OUT_RGBA32F>(k, nullptr, stream, bp);
        return hipGetLastError();
    }
    switch (out_format) {
        case BRT_FLAG_OUT_RGBA32F: launch_t<true, BRT_FLAG_OUT_RGBA32F>(k, d_out, stream, bp); break;
        case BRT_FLAG_OUT_RGBA8_UNORM_SRGB: launch_t<true, BRT_FLAG_OUT_RGBA8_UNORM_SRGB>(k, d_out, stream, bp); break;
        case BRT_FLAG_OUT_RGBA16F: launch_t<true, BRT_FLAG_OUT_RGBA16F>(k, d_out, stream, bp); break;
        case BRT_FLAG_OUT_RGBA8_UNORM: launch_t<true, BRT_FLAG_OUT_RGBA8_UNORM>(k, d_out, stream, bp); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace brt
