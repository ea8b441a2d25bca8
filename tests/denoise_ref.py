"""numpy float32 restatement of the denoiser (DESIGN.md "Denoiser", bevyray_amd/csrc/brt_denoise.hip): the guide buffer from the CPU
oracle's raycast on pixel-centre rays, and the a-trous filter with its formulas as written (pow and the two exps evaluated separately;
the kernel folds them into one exp2, hence the tolerance of the GPU comparison).  np.fmax / np.fmin stand for the kernel's max_f /
min_f (fmaxf / fminf: max(0, NaN) is 0)."""
import ctypes as C

import numpy as np

F32 = np.float32
INF = F32(np.inf)
NO_HIT = np.finfo(F32).max
H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], F32)
DEFAULTS = dict(iterations=5, sigma_l=4.0, sigma_n=128.0, sigma_z=1.0)
STRENGTH_SPP = 4          # above this many samples per pixel sigma_l and the blend weight scale by k = sqrt(STRENGTH_SPP / spp)


def strength(spp):
    return F32(1.0) if spp <= STRENGTH_SPP else np.sqrt(F32(STRENGTH_SPP) / F32(spp))


def pixel_center_rays(oracle, cam, w, h, window=None):
    """(origin (3,), unit directions (h, w, 3)) of the pixel-centre primary rays: the camera ray of tests/helpers.py:sky_color with
    rand_square = (0, 0), i.e. no jitter.  window: the jitter term the kernels keep (camera_ray_dir_center adds (1 / window size) * 0
    to the pixel's position): +0.0 and no bit of any ray for a finite window size, INF * 0 = NaN in every ray under a window of
    height 0 -- every ray then misses ("a window of height 0")."""
    c = cam[0]
    aspect = F32(c["aspect"])
    cd, cu = c["direction"].astype(F32), c["up"].astype(F32)
    right = np.array([cd[1] * cu[2] - cd[2] * cu[1], cd[2] * cu[0] - cd[0] * cu[2], cd[0] * cu[1] - cd[1] * cu[0]], F32)
    scale = F32(oracle.lib.oracle_tan_half_fov(float(c["fov"])))
    uvx = (np.arange(w, dtype=F32) + F32(0.5)) / F32(w)
    uvy = (np.arange(h, dtype=F32) + F32(0.5)) / F32(h)
    ndc_x = (uvx * F32(2.0) - F32(1.0))[None, :, None]
    ndc_y = (F32(1.0) - uvy * F32(2.0))[:, None, None]
    if window is not None:
        with np.errstate(all="ignore"):
            height = F32(window[0]["height"])
            ndc_x = ndc_x + (F32(1.0) / (height * aspect)) * F32(0.0)
            ndc_y = ndc_y + (F32(1.0) / height) * F32(0.0)
    d = (cd + ((ndc_x * aspect) * scale) * right) + (ndc_y * scale) * cu
    ln = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])[..., None]
    return c["position"].astype(F32), (d / ln).astype(F32), scale


def guides(oracle, buffers, cam, w, h, window=None):
    """(h, w, 8) f32: normal.xyz, t (inf: sky), a.rgb, material id as bits (0xFFFFFFFF: sky) -- brt_debug_denoise_guides' layout.
    window: see pixel_center_rays."""
    o, dirs, _ = pixel_center_rays(oracle, cam, w, h, window)
    models = np.ascontiguousarray(buffers.models)
    bvh = np.ascontiguousarray(buffers.bvh)
    mats = buffers.materials
    out = np.zeros((h, w, 8), F32)
    o3 = (C.c_float * 3)(*[float(x) for x in o])
    d3, r7 = (C.c_float * 3)(), (C.c_float * 7)()
    mid, front = C.c_uint32(0), C.c_int(0)
    for y in range(h):
        for x in range(w):
            d3[0], d3[1], d3[2] = (float(v) for v in dirs[y, x])
            oracle.lib.oracle_raycast(models.ctypes.data, len(models), bvh.ctypes.data, len(bvh), o3, d3, r7, C.byref(mid), C.byref(front))
            t = F32(r7[0])
            if t == NO_HIT:                    # (the reference's INF is FLT_MAX, const.wgsl:2; the guide holds +inf)
                out[y, x] = [0, 0, 0, INF, 1, 1, 1, 0]
                out[y, x, 7:8].view(np.uint32)[0] = 0xFFFFFFFF
                continue
            out[y, x, :4] = [r7[4], r7[5], r7[6], t]
            m = mats[mid.value]
            if F32(m["specular_transmission"]) == 0:
                out[y, x, 4:7] = np.sqrt(np.fmax(m["base_color"].astype(F32), F32(1e-3)))
            else:
                out[y, x, 4:7] = 1
            out[y, x, 7:8].view(np.uint32)[0] = mid.value
    return out


def _shift(a, dx, dy, fill):
    """a[y + dy, x + dx] for every (y, x); `fill` where that lies outside the frame."""
    h, w = a.shape[:2]
    out = np.empty_like(a)
    out[...] = fill
    if abs(dx) >= w or abs(dy) >= h:
        return out
    ys, yd = slice(max(0, dy), h + min(0, dy)), slice(max(0, -dy), h + min(0, -dy))
    xs, xd = slice(max(0, dx), w + min(0, dx)), slice(max(0, -dx), w + min(0, -dx))
    out[yd, xd] = a[ys, xs]
    return out


def _taps(cv, g0, dx, dy):
    """cv and g0 at the tap (dx, dy) of every pixel; a tap that is skipped (outside the frame, passes through) reads as {0, 0, 0, -1}
    and contributes nothing at all (the kernel does not read it)."""
    cq = _shift(cv, dx, dy, np.array([0, 0, 0, -1], F32))
    cq[cq[..., 3] < 0] = (0, 0, 0, -1)
    return cq, _shift(g0, dx, dy, 0)


def _lum(c):
    return (F32(0.2126) * c[..., 0] + F32(0.7152) * c[..., 1]) + F32(0.0722) * c[..., 2]


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def denoise(frame, g, dirs, tan_half_fov, iterations=5, sigma_l=4.0, sigma_n=128.0, sigma_z=1.0, spp=1):
    """The denoised RGBA f32 frame of `frame` (h, w, 4), rendered at `spp` samples per pixel, with guides g (h, w, 8) and pixel-centre
    ray directions dirs (h, w, 3)."""
    ks = strength(spp)
    sigma_l, sigma_n, sigma_z = F32(sigma_l) * ks, F32(sigma_n), F32(sigma_z)
    h, w = frame.shape[:2]
    frame = frame.astype(F32)
    n, t, a = g[..., 0:3], g[..., 3], g[..., 4:7]
    with np.errstate(all="ignore"):
        cd = frame[..., :3] / a
        fin = np.isfinite(frame[..., :3]).all(-1) & np.isfinite(cd).all(-1)
        through = ~(t < INF) | ~fin
        theta = (F32(2.0) * F32(tan_half_fov)) / F32(h)
        zscale = np.where(through, F32(0), (t * theta) / np.fmax(np.abs(_dot(n, dirs)), F32(0.1))).astype(F32)
        cv = np.concatenate([cd, np.zeros((h, w, 1), F32)], -1).astype(F32)
        cv[through] = np.concatenate([frame[..., :3], -np.ones((h, w, 1), F32)], -1)[through]
        c0 = cv[..., :3].copy()
        g0 = np.concatenate([n, t[..., None]], -1)
        fill_cv = np.array([0, 0, 0, -1], F32)

        def edge(dx, dy, step, cq, g0q):
            nd = np.fmax(F32(0), _dot(n, g0q[..., :3]))
            wn = np.power(nd, sigma_n).astype(F32)
            dist = F32(step) * np.sqrt(F32(dx * dx + dy * dy))
            wz = np.exp(-np.abs(t - g0q[..., 3]) / ((sigma_z * dist) * zscale + F32(1e-6))).astype(F32)
            return wn, wz

        # 7x7 variance of the luminance, taps weighted by w_n w_z
        lp = _lum(cv)
        sw = np.zeros((h, w), F32)
        sl = np.zeros((h, w), F32)
        sl2 = np.zeros((h, w), F32)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                cq, g0q = _taps(cv, g0, dx, dy)
                wn, wz = edge(dx, dy, 1, cq, g0q)
                wgt = np.where(~(cq[..., 3] < 0), wn * wz, F32(0)).astype(F32)
                lq = _lum(cq)
                sw = sw + wgt
                sl = sl + wgt * lq
                sl2 = sl2 + wgt * (lq * lq)
        mean = sl / sw
        cv[..., 3] = np.where(through, F32(-1), np.fmax(F32(0), sl2 / sw - mean * mean))

        for i in range(iterations):
            step = 1 << i
            gv = np.zeros((h, w), F32)
            gw = np.zeros((h, w), F32)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    vq = _shift(cv, dx, dy, fill_cv)[..., 3]
                    k = F32((0.5 if dx == 0 else 0.25) * (0.5 if dy == 0 else 0.25))
                    ok = ~(vq < 0)                  # (the kernel skips var < 0 only: a NaN variance is a tap)
                    gv = gv + np.where(ok, k * vq, F32(0))
                    gw = gw + np.where(ok, k, F32(0))
            lscale = sigma_l * np.sqrt(np.fmax(F32(0), gv / gw)) + F32(1e-6)
            lp = _lum(cv)
            sw = np.zeros((h, w), F32)
            sc = np.zeros((h, w, 3), F32)
            sv = np.zeros((h, w), F32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    cq, g0q = _taps(cv, g0, dx * step, dy * step)
                    wn, wz = edge(dx, dy, step, cq, g0q)
                    wl = np.exp(-np.abs(lp - _lum(cq)) / lscale).astype(F32)
                    wgt = np.where(~(cq[..., 3] < 0), (((H5[dx + 2] * H5[dy + 2]) * wn) * wz) * wl, F32(0)).astype(F32)
                    sw = sw + wgt
                    sc = sc + wgt[..., None] * cq[..., :3]
                    sv = sv + (wgt * wgt) * cq[..., 3]
            new = np.concatenate([sc / sw[..., None], (sv / (sw * sw))[..., None]], -1).astype(F32)
            cv = np.where(through[..., None], cv, new)
        blended = (c0 + ks * (cv[..., :3] - c0)).astype(F32)        # (pass-through pixels are not taken from it)
    out = np.empty_like(frame)
    out[..., :3] = np.where(through[..., None], cv[..., :3], blended * a)
    out[..., 3] = frame[..., 3]
    return out


def denoise_frame(oracle, frame, g, cam, **settings):
    """denoise() with the pixel-centre rays of `cam`."""
    h, w = frame.shape[:2]
    _, dirs, scale = pixel_center_rays(oracle, cam, w, h)
    return denoise(frame, g, dirs, scale, spp=int(cam[0]["sample_count"]), **{**DEFAULTS, **settings})


def hit_mse(frame, ref, g):
    """Mean squared error of the colour over the pixels whose centre ray hits."""
    hit = g[..., 3] < INF
    d = frame[..., :3][hit].astype(np.float64) - ref[..., :3][hit].astype(np.float64)
    return float(np.mean(d * d))
