"""numpy float32 restatement of the guide-buffer upsampling (DESIGN.md "Guide-buffer upsampling", bevyray_amd/csrc/brt_upscale.hip) in the
kernel's order of operations: the position of an output pixel in the low frame, the eligibility of a tap, the sky of a missing ray, and
the three stages.  w_n and w_z are evaluated separately as written (pow, exp); the kernel folds them into one exp2, hence the tolerance
of the GPU comparison.  Guides come from denoise_ref.guides (the oracle's raycast) or brt_debug_denoise_guides, at both sizes."""
import numpy as np

import denoise_ref as dr

F32 = np.float32
INF = F32(np.inf)
BILINEAR_FLOOR = F32(2.0 ** -26)     # kUpscaleBilinearFloor
EDGE_FLOOR = F32(0.25)               # kUpscaleEdgeFloor
SCALE_A, SCALE_B, SCALE_C = F32(0.5), F32(0.125), F32(0.5)     # kUpscaleScaleA / B / C: exact, they keep every sum of w c' finite
SKY, STAGE_A, STAGE_B, STAGE_C, STAGE_NONE = 0, 1, 2, 3, 4     # what upscale() reports per output pixel


def low_positions(n_full, n_low):
    """Per output column (row) of an axis of n_full pixels over n_low low pixels: (position in low pixel units, clamped; floor as
    int; the neighbour min(floor + 1, n_low - 1); the fraction)."""
    x = ((np.arange(n_full, dtype=F32) + F32(0.5)) * F32(n_low)) / F32(n_full) - F32(0.5)
    x = np.fmin(np.fmax(x, F32(0)), F32(n_low - 1)).astype(F32)
    x0f = np.floor(x).astype(F32)
    x0 = x0f.astype(np.int64)
    return x, x0, np.minimum(x0 + 1, n_low - 1), (x - x0f).astype(F32)


def sky_colour(dirs):
    """sqrt(background_gradient(d)) per channel (raytrace.wgsl:364-369, :223) for unit directions dirs (..., 3)."""
    ln = np.sqrt((dirs[..., 0] * dirs[..., 0] + dirs[..., 1] * dirs[..., 1]) + dirs[..., 2] * dirs[..., 2])
    a = F32(0.5) * ((dirs[..., 1] / ln).astype(F32) + F32(1.0))
    b = F32(1.0) - a
    return np.sqrt(np.stack([b * F32(1.0) + a * F32(0.5), b * F32(1.0) + a * F32(0.7), b * F32(1.0) + a * F32(1.0)], -1)).astype(F32)


def upscale(low, g_low, g_full, dirs_full, tan_half_fov, sigma_n=128.0, sigma_z=1.0, bilinear_floor=BILINEAR_FLOOR,
            edge_floor=EDGE_FLOOR, scales=(SCALE_A, SCALE_B, SCALE_C)):
    """(out (h, w, 4) f32, stage (h, w) u8) of the low frame `low` (lh, lw, 4) with guides g_low (lh, lw, 8), for the output pixels
    whose guides are g_full (h, w, 8) and whose unit pixel-centre directions are dirs_full (h, w, 3).  scales: the powers of two the
    weights of stages A, B, C are multiplied by ((1, 1, 1): the rule before the scaling, for the test that the scaling keeps the bits)."""
    low = low.astype(F32)
    lh, lw = low.shape[:2]
    h, w = g_full.shape[:2]
    sigma_n, sigma_z = F32(sigma_n), F32(sigma_z)
    bilinear_floor, edge_floor = F32(bilinear_floor), F32(edge_floor)
    scale_a, scale_b, scale_c = (F32(s) for s in scales)
    n_p, t_p, a_p = g_full[..., 0:3], g_full[..., 3], g_full[..., 4:7]
    mat_p = np.ascontiguousarray(g_full[..., 7]).view(np.uint32)
    hit_p = t_p < INF
    out = np.zeros((h, w, 4), F32)
    out[..., 3] = 1
    stage = np.full((h, w), STAGE_NONE, np.uint8)
    with np.errstate(all="ignore"):
        # the low frame's taps: eligibility apart from the material, and c' = c / a
        c_l = low[..., :3]
        cd_l = (c_l / g_low[..., 4:7]).astype(F32)
        fin_l = np.isfinite(c_l).all(-1)
        ok_l = (g_low[..., 3] < INF) & fin_l & np.isfinite(cd_l).all(-1)
        mat_l = np.ascontiguousarray(g_low[..., 7]).view(np.uint32)
        theta = (F32(2.0) * F32(tan_half_fov)) / F32(lh)
        zscale = ((t_p * theta) / np.fmax(np.abs(dr._dot(n_p, dirs_full)), F32(0.1))).astype(F32)
        zden = (sigma_z * zscale + F32(1e-6)).astype(F32)
        xl, x0, x1, fx = low_positions(w, lw)
        yl, y0, y1, fy = low_positions(h, lh)

        def tap(qy, qx, inside):
            """(eligible (h, w), c' (h, w, 3), w_n w_z (h, w)) of the taps (qy, qx) (h, w) int, clipped where not `inside`."""
            qy, qx = np.clip(qy, 0, lh - 1), np.clip(qx, 0, lw - 1)
            el = inside & hit_p & ok_l[qy, qx] & (mat_l[qy, qx] == mat_p)
            gq = g_low[qy, qx]
            nd = np.fmax(F32(0), dr._dot(n_p, gq[..., 0:3]))
            wn = np.power(nd, sigma_n).astype(F32)
            wz = np.exp(-(np.abs(t_p - gq[..., 3]) / zden)).astype(F32)
            return el, cd_l[qy, qx], (wn * wz).astype(F32)

        def add(acc, el, wgt, col):
            sw, sc = acc
            wgt = np.where(el, wgt, F32(0)).astype(F32)
            col = np.where(el[..., None], col, F32(0)).astype(F32)
            return (sw + wgt).astype(F32), (sc + wgt[..., None] * col).astype(F32)

        ones = np.ones((h, w), bool)
        bx, by = (F32(1.0) - fx, fx), (F32(1.0) - fy, fy)
        qxs, qys = (x0, x1), (y0, y1)
        # stage A: the 2x2 bilinear footprint, in the order (x0, y0), (x1, y0), (x0, y1), (x1, y1)
        acc = (np.zeros((h, w), F32), np.zeros((h, w, 3), F32))
        n_a = np.zeros((h, w), np.int32)
        for j in range(2):
            for i in range(2):
                qy, qx = np.broadcast_to(qys[j][:, None], (h, w)), np.broadcast_to(qxs[i][None, :], (h, w))
                el, cd, e = tap(qy, qx, ones)
                b = (bx[i][None, :] * by[j][:, None]).astype(F32)
                acc = add(acc, el, ((b + bilinear_floor) * (e + edge_floor)) * scale_a, cd)
                n_a += el
        in_a = hit_p & (n_a > 0)
        # stage B: the 4x4 taps x0 - 1 .. x0 + 2, y0 - 1 .. y0 + 2 inside the frame
        acc_b = (np.zeros((h, w), F32), np.zeros((h, w, 3), F32))
        n_b = np.zeros((h, w), np.int32)
        for j in range(-1, 3):
            for i in range(-1, 3):
                qy, qx = np.broadcast_to((y0 + j)[:, None], (h, w)), np.broadcast_to((x0 + i)[None, :], (h, w))
                inside = (qy >= 0) & (qy < lh) & (qx >= 0) & (qx < lw)
                el, cd, e = tap(qy, qx, inside)
                dx, dy = (qx.astype(F32) - xl[None, :]).astype(F32), (qy.astype(F32) - yl[:, None]).astype(F32)
                acc_b = add(acc_b, el, ((e + edge_floor) / (F32(1.0) + (dx * dx + dy * dy))) * scale_b, cd)
                n_b += el
        in_b = hit_p & ~in_a & (n_b > 0)
        # stage C: the bilinear colour of the finite taps of the footprint, not demodulated
        acc_c = (np.zeros((h, w), F32), np.zeros((h, w, 3), F32))
        n_c = np.zeros((h, w), np.int32)
        for j in range(2):
            for i in range(2):
                qy, qx = np.broadcast_to(qys[j][:, None], (h, w)), np.broadcast_to(qxs[i][None, :], (h, w))
                el = fin_l[qy, qx]
                b = (bx[i][None, :] * by[j][:, None]).astype(F32)
                acc_c = add(acc_c, el, np.broadcast_to((b + bilinear_floor) * scale_c, (h, w)), c_l[qy, qx])
                n_c += el
        in_c = hit_p & ~in_a & ~in_b & (n_c > 0)
        for mask, (sw, sc), remod, code in ((in_a, acc, True, STAGE_A), (in_b, acc_b, True, STAGE_B), (in_c, acc_c, False, STAGE_C)):
            col = (sc / sw[..., None]).astype(F32)
            if remod:
                col = (col * a_p).astype(F32)
            out[..., :3][mask] = col[mask]
            stage[mask] = code
        out[..., :3][~hit_p] = sky_colour(dirs_full)[~hit_p]
        stage[~hit_p] = SKY
    return out, stage


def upscale_frame(oracle, low, g_low, g_full, cam, **settings):
    """upscale() with the pixel-centre rays of `cam` at g_full's size and the denoiser's default sigmas."""
    h, w = g_full.shape[:2]
    _, dirs, scale = dr.pixel_center_rays(oracle, cam, w, h)
    s = {"sigma_n": dr.DEFAULTS["sigma_n"], "sigma_z": dr.DEFAULTS["sigma_z"], **settings}
    return upscale(low, g_low, g_full, dirs, scale, **s)
