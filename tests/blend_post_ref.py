"""numpy restatement of the post-passes on blended (level 1 / 2) frames (BRT_FLAG_BLEND_POST,
brt_blend_post_device): a thin layer over denoise_ref / temporal_ref.  The input is a coverage frame -- the level's frame traced with
the raster depth and no raster colour; a pixel is covered iff its alpha is exactly +0.0.  Covered guides become misses (t = +inf, a = 1,
material and sphere id 0xFFFFFFFF), which makes the pixel pass through every formula of the two references unchanged, and the covered
pixels of the result are the raster texels, all four channels."""
import numpy as np

import denoise_ref as dr
import temporal_ref as tr

F32 = np.float32
U32 = np.uint32


def raster_inputs(w, h):
    """The synthetic raster inputs of the tests: (rgba (h, w, 4), depth (h, w)).  Depth 0 (the far plane), a wall at u < 0.35 with
    reverse-Z depth 0.1 / 9, a disc around (0.65, 0.55) of radius 0.18 (in units of the height) with depth 0.1 / 6; colour
    {u, v, 0.25, 0.5}."""
    return raster_rgba(w, h), raster_depth(w, h)


def _uv(w, h):
    u = ((np.arange(w, dtype=np.float64) + 0.5) / w)[None, :]
    v = ((np.arange(h, dtype=np.float64) + 0.5) / h)[:, None]
    return u, v


def raster_depth(w, h, disc_u=0.65):
    u, v = _uv(w, h)
    depth = np.zeros((h, w), F32)
    depth[np.broadcast_to(u < 0.35, (h, w))] = F32(0.1 / 9)
    depth[(u - disc_u) ** 2 * (w / h) ** 2 + (v - 0.55) ** 2 < 0.18 ** 2] = F32(0.1 / 6)
    return depth


def raster_rgba(w, h):
    u, v = _uv(w, h)
    rgba = np.empty((h, w, 4), F32)
    rgba[..., 0], rgba[..., 1], rgba[..., 2], rgba[..., 3] = u, v, 0.25, 0.5
    return rgba


def coverage(frame):
    """(h, w) bool: alpha exactly +0.0."""
    return np.ascontiguousarray(frame[..., 3], F32).view(U32) == 0


def composite(frame, cov, raster):
    """`frame` with the covered pixels replaced by the raster texels (raster None: zeros)."""
    out = np.array(frame, F32)
    out[cov] = 0 if raster is None else np.asarray(raster, F32)[cov]
    return out


def cover_guides(g, cov):
    """The guides (h, w, 8) with the covered pixels as misses."""
    g = g.copy()
    miss = np.array([0, 0, 0, np.inf, 1, 1, 1, 0], F32)
    miss[7:8].view(U32)[0] = 0xFFFFFFFF
    g[cov] = miss
    return g


def cover_sid(sid, cov):
    return np.where(cov, tr.NO_SPHERE, sid).astype(U32)


def denoise_frame(oracle, cov_frame, g, cam, raster, **settings):
    """BRT_FLAG_BLEND_POST | BRT_FLAG_DENOISE: g are the Pure-level guides of the camera."""
    cov = coverage(cov_frame)
    return composite(dr.denoise_frame(oracle, cov_frame, cover_guides(g, cov), cam, **settings), cov, raster)


def frame_step(hist, cov_frame, g, sid, cam, spheres, spp, denoise_on, raster, **settings):
    """One BRT_FLAG_BLEND_POST | BRT_FLAG_TEMPORAL (| BRT_FLAG_DENOISE) frame on the history `hist` (temporal_ref.History, shared with
    Pure-level frames); cam: temporal_ref.Camera."""
    cov = coverage(cov_frame)
    out = tr.frame_step(hist, cov_frame, cover_guides(g, cov), cover_sid(sid, cov), cam, spheres, spp, denoise_on, **settings)
    return composite(out, cov, raster)


def mse(frame, ref, mask):
    d = frame[..., :3][mask].astype(np.float64) - ref[..., :3][mask].astype(np.float64)
    return float(np.mean(d * d))
