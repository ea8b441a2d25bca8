// brt_gbuffer.hip -- the G-buffer of a frame (brt_render_gbuffer*, DESIGN.md "G-buffer"): depth, normal, motion, ids and albedo of the
// first hit of every pixel-centre ray, in one kernel.
//
// k_gbuffer<D16, COV>  one thread per pixel: the ray denoise_guides_pixel casts (camera_ray_dir_center), walked through the resident scene
//                      in global memory with the bring-up kernel's raycast, as k_denoise_guides and k_query_plain walk it; then the rule
//                      (brt_gbuffer.h) on the registers of the hit, and every requested plane stored from them: no ray and no hit record
//                      of a pixel is ever in memory.  COV: a coverage frame is bound; a covered pixel (alpha +0.0) casts no ray and stores
//                      nothing, and a wave whose pixels are all covered skips the walk (k_denoise_guides_cov's shape).
// 256 threads = one 16x16 pixel tile (a wave is 4 rows of 16: its float4 stores are four runs of 256 contiguous bytes), as the guide kernel.
// The depth mode and the two formats are wave-uniform kernel arguments read behind the walk: nothing of them is live across it (usage:
// profiles/gbuffer/usage_gbuffer.txt).  No atomic touches a plane; a counted call sums its five counts per wave and adds them to args.stat.
#include <hip/hip_runtime.h>

#include <hip/hip_fp16.h>

#include "brt_denoise.h"     // covered
#include "brt_gbuffer_launch.h"
#include "brt_stream.h"      // scene_global

namespace brt {

namespace {

constexpr uint32_t kTile = 16;
constexpr uint32_t kNone = 0xffffffffu;      // BRT_QUERY_NONE

BRT_DEV uint32_t g_wave_sum(uint32_t v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += (uint32_t)__shfl_xor((int)v, s, 64);
    return v;
}

}  // namespace

template <bool D16, bool COV>
__global__ __launch_bounds__(256) void k_gbuffer(DeviceSceneView sv, FrameParams fp, GbufferArgs ga) {
    const uint32_t px = blockIdx.x * kTile + (threadIdx.x & (kTile - 1u)), py = blockIdx.y * kTile + threadIdx.x / kTile;
    const bool inside = px < fp.width && py < fp.height;
    const uint32_t p = inside ? py * fp.width + px : 0u;
    bool cast = inside;
    uint32_t n_cov = 0u;
    if constexpr (COV) {
        if (inside && covered(ga.cov[p].w)) {
            cast = false;
            n_cov = 1u;
        }
    }
    uint32_t n_hit = 0u, n_moved = 0u, n_noprev = 0u;
    if (cast) {
        const ScenePtrs sc = scene_global(sv);
        const float uvx = ((float)px + 0.5f) / (float)fp.width;        // pixel_begin (brt_trace.h)
        const float uvy = ((float)py + 0.5f) / (float)fp.height;
        const f3 dv = camera_ray_dir_center(fp, uvx * 2.0f - 1.0f, 1.0f - uvy * 2.0f);
        const f3 o = mk3(fp.cam_pos[0], fp.cam_pos[1], fp.cam_pos[2]);
        uint32_t stack[34];   // DONE sentinel + 32 entries + one spare
        HitCounters hc = {};
        float t;
        uint32_t idx;
        raycast<1, false, D16, false>(sc, sv.root_desc, stack, o, dv, t, idx, hc);
        const bool hit = t != kInf;
        const float d[3] = {dv.x, dv.y, dv.z};
        float sn[4] = {0.0f, 0.0f, 0.0f, 0.0f}, so[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t sphere = kNone, material = kNone;
        float4 alb = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (hit) {
            const float4 s = sc.spheres[idx];
            sn[0] = so[0] = s.x;
            sn[1] = so[1] = s.y;
            sn[2] = so[2] = s.z;
            sn[3] = so[3] = s.w;
            sphere = ga.rmap ? ga.rmap[idx] : idx;      // (the resident order is the caller's unless the hot order renumbered it)
            material = sv.sphere_material[idx];
            alb = sc.sphere_mats[2 * idx];
            if (ga.prev_models) {
                const float4 m = ga.prev_models[2 * (size_t)sphere];
                so[0] = m.x;
                so[1] = m.y;
                so[2] = m.z;
                so[3] = m.w * m.w;                      // validate_and_encode's r^2 (raytrace.wgsl:375)
            }
        }
        GbufferPixel g;
        gbuffer_pixel(fp, ga.gv, ga.depth_mode, fp.width, fp.height, px, py, d, hit ? t : __builtin_inff(), sn, so, g);
        if (ga.depth) ga.depth[p] = g.depth;
        if (ga.normal) {
            if (ga.normal_format == 0u) reinterpret_cast<float4*>(ga.normal)[p] = make_float4(g.n[0], g.n[1], g.n[2], hit ? 1.0f : 0.0f);
            else reinterpret_cast<uint32_t*>(ga.normal)[p] = gbuffer_rgb10a2(g.n, hit);
        }
        if (ga.motion) {
            if (ga.motion_format == 0u) reinterpret_cast<float2*>(ga.motion)[p] = make_float2(g.mu, g.mv);
            else if (ga.motion_format == 1u)
                reinterpret_cast<uint32_t*>(ga.motion)[p] = (uint32_t)__half_as_ushort(__float2half_rn(g.mu)) |
                                                            ((uint32_t)__half_as_ushort(__float2half_rn(g.mv)) << 16);
            else reinterpret_cast<float2*>(ga.motion)[p] = make_float2(g.xp, g.yp);
        }
        if (ga.ids) ga.ids[p] = make_uint4(sphere, material, g.status, 0u);
        if (ga.albedo) ga.albedo[p] = alb;
        n_hit = hit ? 1u : 0u;
        n_moved = (g.status & GBUF_MOVED) ? 1u : 0u;
        n_noprev = (g.status & GBUF_NO_PREVIOUS) ? 1u : 0u;
    }
    if (ga.stat) {                  // (wave-uniform; every lane of the wave is here)
        const uint32_t c0 = g_wave_sum(cast ? 1u : 0u), c1 = g_wave_sum(n_hit), c2 = g_wave_sum(n_cov), c3 = g_wave_sum(n_moved),
                       c4 = g_wave_sum(n_noprev);
        if (lane_id() == 0u) {
            if (c0) atomicAdd(ga.stat + 0, c0);
            if (c1) atomicAdd(ga.stat + 1, c1);
            if (c2) atomicAdd(ga.stat + 2, c2);
            if (c3) atomicAdd(ga.stat + 3, c3);
            if (c4) atomicAdd(ga.stat + 4, c4);
        }
    }
}

hipError_t launch_gbuffer(const DeviceSceneView& scene, const FrameParams& fp, const GbufferArgs& args, hipStream_t stream) {
    const dim3 grid((fp.width + kTile - 1u) / kTile, (fp.height + kTile - 1u) / kTile);
    if (args.cov) {
        if (scene.desc16) hipLaunchKernelGGL((k_gbuffer<true, true>), grid, dim3(256), 0, stream, scene, fp, args);
        else hipLaunchKernelGGL((k_gbuffer<false, true>), grid, dim3(256), 0, stream, scene, fp, args);
    } else {
        if (scene.desc16) hipLaunchKernelGGL((k_gbuffer<true, false>), grid, dim3(256), 0, stream, scene, fp, args);
        else hipLaunchKernelGGL((k_gbuffer<false, false>), grid, dim3(256), 0, stream, scene, fp, args);
    }
    return hipGetLastError();
}

}  // namespace brt
