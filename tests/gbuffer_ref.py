"""Reference side of tests/test_gbuffer.py: the G-buffer rule of bevyray_amd/csrc/brt_gbuffer.h restated in numpy -- in f32, operation
for operation (`pixel` with T = np.float32: what brt_host_gbuffer_pixel and the kernel compute, bit for bit), and in float64 (T =
np.float64: what the f32 result is an approximation of) -- and the two encodings (Rgb10a2Unorm, f16 pairs)."""
import math

import numpy as np

F32 = np.float32
F64 = np.float64
HIT, FRONT_FACE, MOVED, NO_PREVIOUS = 1, 2, 4, 8
DEPTH_VIEW, DEPTH_SHADER, DEPTH_DISTANCE = 0, 1, 2


def _dot(T, a, b):
    return T(T(T(a[0] * b[0]) + T(a[1] * b[1])) + T(a[2] * b[2]))


def _cross(T, a, b):
    return [T(T(a[1] * b[2]) - T(a[2] * b[1])), T(T(a[2] * b[0]) - T(a[0] * b[2])), T(T(a[0] * b[1]) - T(a[1] * b[0]))]


def camera_terms(cam, T=F32):
    """make_frame_params' camera terms of one CAMERA_DTYPE record."""
    c = cam[0] if getattr(cam, "shape", ()) else cam
    pos, cd, cu = ([T(x) for x in c[k]] for k in ("position", "direction", "up"))
    half = F32(c["fov"]) * F32(0.5)
    with np.errstate(all="ignore"):
        tan64 = math.tan(float(half)) if np.isfinite(half) else np.nan        # (the C library's tan(inf) is a NaN)
    tan_half = T(F32(tan64)) if T is F32 else T(tan64)
    return dict(pos=pos, dir=cd, up=cu, right=_cross(T, cd, cu), aspect=T(c["aspect"]), tan_half=tan_half, near=T(c["near"]), far=T(c["far"]))


def direction(ct, win_height, W, H, px, py, T=F32):
    """camera_ray_dir_center for pixel (px, py): the pixel-centre direction (f32: brt_host_pixel_ray's bits)."""
    with np.errstate(all="ignore"):
        heightf = T(win_height)
        widthf = T(heightf * ct["aspect"])
        inv_w, inv_h = T(T(1.0) / widthf), T(T(1.0) / heightf)
        uvx = T(T(T(px) + T(0.5)) / T(W))
        uvy = T(T(T(py) + T(0.5)) / T(H))
        ndc_x = T(T(T(uvx * T(2.0)) - T(1.0)) + T(inv_w * T(0.0)))
        ndc_y = T(T(T(1.0) - T(uvy * T(2.0))) + T(inv_h * T(0.0)))
        if T is F64:            # (the jitter term is the reference's; in exact arithmetic it is nothing)
            ndc_x, ndc_y = T(uvx * 2.0 - 1.0), T(1.0 - uvy * 2.0)
        sx = T(T(ndc_x * ct["aspect"]) * ct["tan_half"])
        sy = T(ndc_y * ct["tan_half"])
        v = [T(T(ct["dir"][k] + T(sx * ct["right"][k])) + T(sy * ct["up"][k])) for k in range(3)]
        ln = T(np.sqrt(_dot(T, v, v)))
        return [T(v[k] / ln) for k in range(3)]


def view_terms(cur, prev, T=F32):
    """gbuffer_view_of: fwd, the DEPTH_SHADER miss value, the previous camera's cofactor rows, same_camera."""
    with np.errstate(all="ignore"):
        D, R, U = prev["dir"], prev["right"], prev["up"]
        rows = [_cross(T, R, U), _cross(T, U, D), _cross(T, D, R)]
        det = _dot(T, D, rows[0])
        inv = [[T(rows[i][j] / det) for j in range(3)] for i in range(3)]
        ln = T(np.sqrt(_dot(T, cur["dir"], cur["dir"])))
        fwd = [T(cur["dir"][k] / ln) for k in range(3)]
        fb = T(cur["far"] - T(1.0))
        miss_depth = T(-1.0) if fb > cur["far"] else T(cur["near"] / fb)
    bits = lambda v: np.array(v, F32).tobytes()
    same = all(bits(cur[k]) == bits(prev[k]) for k in ("pos", "dir", "up", "right", "aspect", "tan_half"))
    return dict(fwd=fwd, miss_depth=miss_depth, o=prev["pos"], inv=inv, aspect=prev["aspect"], tan_half=prev["tan_half"], same=same)


def pixel(cam, win, W, H, px, py, depth_mode, t, sn=None, so=None, prev_cam=None, T=F32, same=None):
    """The rule for one pixel -> dict(depth, status, n (3), xp, yp, mu, mv, d (3)).  sn / so: {centre, r^2} now and before (so None: not
    moved), as f32 values; t: an f32 value, inf (or NaN): a miss.  same: overrides the bitwise camera compare (float64 property tests)."""
    cur = camera_terms(cam, T)
    prv = cur if prev_cam is None else camera_terms(prev_cam, T)
    gv = view_terms(cur, prv, T)
    if prev_cam is not None:        # (the compare is of the f32 terms, whatever T)
        gv["same"] = view_terms(camera_terms(cam, F32), camera_terms(prev_cam, F32), F32)["same"]
    if same is not None:
        gv["same"] = same
    w = win[0] if getattr(win, "shape", ()) else win
    d = direction(cur, w["height"], W, H, px, py, T)
    out = dict(d=d)
    with np.errstate(all="ignore"):
        t32 = F32(t)
        hit = bool(t32 < F32(np.inf))
        t = T(t32)
        status = 0
        moved = False
        if hit:
            status = HIT
            sn_ = [T(F32(x)) for x in sn]
            so_ = sn_ if so is None else [T(F32(x)) for x in so]
            x = [T(cur["pos"][k] + T(t * d[k])) for k in range(3)]
            wv = [T(x[k] - sn_[k]) for k in range(3)]
            ln = T(np.sqrt(_dot(T, wv, wv)))
            n = [T(wv[k] / ln) for k in range(3)]
            if _dot(T, d, n) < 0:
                status |= FRONT_FACE
            if depth_mode == DEPTH_VIEW:
                depth = T(cur["near"] / T(t * _dot(T, d, gv["fwd"])))
            elif depth_mode == DEPTH_SHADER:
                depth = T(-1.0) if t > cur["far"] else T(cur["near"] / t)
            else:
                depth = t
            moved = so is not None and np.array(sn, F32).tobytes() != np.array(so, F32).tobytes()
            if moved:
                status |= MOVED
                s = T(T(np.sqrt(so_[3])) / T(np.sqrt(sn_[3])))
                x = [T(so_[k] + T(T(x[k] - sn_[k]) * s)) for k in range(3)]
            v = [T(x[k] - gv["o"][k]) for k in range(3)]
            out["dist_prev"] = float(np.sqrt(_dot(F64, [F64(c) for c in v], [F64(c) for c in v])))      # (|X_prev - o_prev|: for the tests)
        else:
            n = [T(0.0)] * 3
            v = d
            depth = T(0.0) if depth_mode == DEPTH_VIEW else (gv["miss_depth"] if depth_mode == DEPTH_SHADER else T(np.inf))
        xp = yp = T(np.nan)
        if gv["same"] and not moved:
            xp, yp = T(px), T(py)
        else:
            z, a, b = (_dot(T, gv["inv"][i], v) for i in range(3))
            if z > 0:
                ndc_x = T(T(T(a / z) / gv["tan_half"]) / gv["aspect"])
                ndc_y = T(T(b / z) / gv["tan_half"])
                xp = T(T(T(T(ndc_x + T(1.0)) * T(0.5)) * T(W)) - T(0.5))
                yp = T(T(T(T(T(1.0) - ndc_y) * T(0.5)) * T(H)) - T(0.5))
        if not (xp > -1 and xp < W and yp > -1 and yp < H):
            status |= NO_PREVIOUS
            xp = yp = T(np.nan)
            mu = mv = T(0.0)
        else:
            uvx = T(T(T(px) + T(0.5)) / T(W))
            uvy = T(T(T(py) + T(0.5)) / T(H))
            mu = T(uvx - T(T(xp + T(0.5)) / T(W)))
            mv = T(uvy - T(T(yp + T(0.5)) / T(H)))
    out.update(depth=depth, status=status, n=n, xp=xp, yp=yp, mu=mu, mv=mv, hit=hit)
    return out


# ---- encodings (vectorised) ----

def unorm10(n):
    """One Rgb10a2Unorm channel of f32 values: u32(floor(clamp(n * 0.5 + 0.5, 0, 1) * 1023 + 0.5)), a NaN 0."""
    n = np.asarray(n, F32)
    with np.errstate(all="ignore"):
        x = (n * F32(0.5) + F32(0.5)).astype(F32)
        cl = np.where(x > 0, np.where(x < 1, x, F32(1.0)), F32(0.0)).astype(F32)      # (a NaN fails the first test)
        return np.floor((cl * F32(1023.0)).astype(F32) + F32(0.5)).astype(np.uint32)


def rgb10a2(n3, hit=True):
    """(..., 3) f32 normals -> u32 texels: R in the low bits, alpha 3; a miss is 0."""
    n3 = np.asarray(n3, F32)
    q = unorm10(n3)
    word = (q[..., 0] | (q[..., 1] << np.uint32(10)) | (q[..., 2] << np.uint32(20)) | np.uint32(3 << 30)).astype(np.uint32)
    return np.where(hit, word, np.uint32(0)).astype(np.uint32)


def f16_pair(mu, mv):
    """Two f32 arrays -> u32: numpy's f32 -> f16 conversion (round to nearest even), mu in the low half."""
    with np.errstate(all="ignore"):
        a = np.asarray(mu, F32).astype(np.float16).view(np.uint16).astype(np.uint32)
        b = np.asarray(mv, F32).astype(np.float16).view(np.uint16).astype(np.uint32)
    return (a | (b << np.uint32(16))).astype(np.uint32)


def record(r, depth_mode, motion_format):
    """The dict of `pixel` (T = f32) as brt_host_gbuffer_pixel's GBUFFER_PIXEL_DTYPE record (a (1,) array)."""
    import bevyray_amd as brt
    out = np.zeros(1, brt.GBUFFER_PIXEL_DTYPE)
    out["depth"] = r["depth"]
    out["status"] = r["status"]
    n = np.array(r["n"], F32)
    out["normal_rgb10a2"] = rgb10a2(n, r["hit"])
    out["normal"][0, :3] = n
    out["normal"][0, 3] = 1.0 if r["hit"] else 0.0
    if motion_format == 0:
        out["motion"] = np.array([r["mu"], r["mv"]], F32).view(np.uint32)
    elif motion_format == 1:
        out["motion"] = [f16_pair(r["mu"], r["mv"]), 0]
    else:
        out["motion"] = np.array([r["xp"], r["yp"]], F32).view(np.uint32)
    out["xy_prev"] = [r["xp"], r["yp"]]
    out["direction"] = np.array(r["d"], F32)
    return out
