"""numpy float32 restatement of the upsampling of blended (level 1 / 2) frames (DESIGN.md "Upsampling blended frames",
brt_upscale_blend_device, bevyray_amd/csrc/brt_upscale.hip): a thin layer over upscale_ref.  The low frame is a Pure frame; the raster
blend of the reference (raytrace.wgsl:104-120, resolve_pixel in brt_device.h) is decided per OUTPUT pixel from the distance t of its
centre ray -- the t plane of the full-size guides -- against the full-size raster depth.  A covered pixel is its raster texel, all four
channels; any other pixel is upscale_ref's, bit for bit.  Also the raster fixture the CPU and GPU tests share."""
import numpy as np

import upscale_ref as ur

F32 = np.float32
INF = F32(np.inf)
COVERED = 5                          # what upscale() reports for a covered pixel, beside upscale_ref's stages
WALL_SHARE, DISC_RADIUS, PLANE_DISTANCE = 0.40, 0.30, 0.65     # the fixture (raster_depth)


def fallback_far(cam, level):
    """The depth of a ray that misses: far + 10 at level 1, far - 1 at level 2 (raytrace.wgsl:177-182), in f32."""
    far = F32(cam[0]["far"])
    return F32(far + F32(10.0)) if int(level) == 1 else F32(far - F32(1.0))


def covered(cam, level, t, raster_depth):
    """(...) bool: resolve_pixel's compare fed with ONE sample of depth t (inf: a miss), every operation a separately rounded f32 one.
    raster_depth None reads as 0; a NaN depth never covers; level 3 never blends."""
    t = np.asarray(t, F32)
    depth_p = np.zeros(t.shape, F32) if raster_depth is None else np.broadcast_to(np.asarray(raster_depth, F32), t.shape)
    if int(level) == 3:
        return np.zeros(t.shape, bool)
    assert int(level) in (1, 2)
    near, far = F32(cam[0]["near"]), F32(cam[0]["far"])
    with np.errstate(all="ignore"):
        depth = np.where(t == INF, fallback_far(cam, level), t).astype(F32)
        rd = np.where(depth > far, F32(-1.0), (near / depth).astype(F32)).astype(F32)
        return depth_p > rd


def upscale(low, g_low, g_full, dirs_full, tan_half_fov, cam, level, raster_rgba, raster_depth, **settings):
    """(out (h, w, 4) f32, stage (h, w) u8): upscale_ref.upscale with the covered pixels replaced by their raster texels (raster_rgba
    None: zeros) and reported as COVERED."""
    out, stage = ur.upscale(low, g_low, g_full, dirs_full, tan_half_fov, **settings)
    cov = covered(cam, level, g_full[..., 3], raster_depth)
    out[cov] = 0 if raster_rgba is None else np.asarray(raster_rgba, F32)[cov]
    stage[cov] = COVERED
    return out, stage


def upscale_frame(oracle, low, g_low, g_full, cam, level, raster_rgba, raster_depth, **settings):
    """upscale() with the pixel-centre rays of `cam` at g_full's size and the denoiser's default sigmas (upscale_ref.upscale_frame)."""
    import denoise_ref as dr
    h, w = g_full.shape[:2]
    _, dirs, scale = dr.pixel_center_rays(oracle, cam, w, h)
    s = {"sigma_n": dr.DEFAULTS["sigma_n"], "sigma_z": dr.DEFAULTS["sigma_z"], **settings}
    return upscale(low, g_low, g_full, dirs, scale, cam, level, raster_rgba, raster_depth, **s)


# ---- the raster fixture -------------------------------------------------------------------------------------------------------------

def _uv(w, h):
    u = ((np.arange(w, dtype=np.float64) + 0.5) / w)[None, :]
    v = ((np.arange(h, dtype=np.float64) + 0.5) / h)[:, None]
    return u, v


def raster_depth(w, h, near=0.1):
    """Reverse-Z depth (h, w): 1.0 in the left WALL_SHARE of the columns (a wall at the near plane), near / PLANE_DISTANCE inside the
    centred disc of radius DISC_RADIUS (in units of the height; a camera-facing plane in the middle of the scene's hit distances, so
    that hits in front of it and behind it both occur), 0 elsewhere."""
    u, v = _uv(w, h)
    depth = np.zeros((h, w), F32)
    depth[(u - 0.5) ** 2 * (w / h) ** 2 + (v - 0.5) ** 2 < DISC_RADIUS ** 2] = F32(near) / F32(PLANE_DISTANCE)
    depth[np.broadcast_to(u < WALL_SHARE, (h, w))] = F32(1.0)
    return depth


def special_texels(w, h):
    """((y, x) of the NaN texel, (y, x) of the Inf texel): both in the wall."""
    return (h // 3, w // 10), ((2 * h) // 3, w // 5)


def raster_rgba(w, h):
    """Raster colour (h, w, 4): {u, v, 0.25 + u v / 2, 0.5 + u / 4}, with one NaN (red) and one Inf (green) texel in the wall."""
    u, v = _uv(w, h)
    rgba = np.empty((h, w, 4), F32)
    rgba[..., 0], rgba[..., 1], rgba[..., 2], rgba[..., 3] = u, v, 0.25 + 0.5 * u * v, 0.5 + 0.25 * u
    (ny, nx), (iy, ix) = special_texels(w, h)
    rgba[ny, nx, 0] = np.nan
    rgba[iy, ix, 1] = np.inf
    return rgba


def class_shares(cov):
    """(covered share, uncovered share) of a frame."""
    c = float(np.mean(cov))
    return c, 1.0 - c
