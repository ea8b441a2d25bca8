"""A numpy float64 evaluation of the guide-buffer upsampling rule, written from the formulas of DESIGN.md section 14 after the manner of
tests/denoise_ref64.py.  It shares nothing with tests/upscale_ref.py but the stage codes and how its inputs are loaded (guides,
pixel-centre rays, tan(fov / 2)): positions, weights, sums, the remodulation and the sky are float64, and the taps are walked per
output pixel from padded planes, not in the kernel's order of roundings.

The decisions that the rule defines on float32 values stay as the rule defines them: a guide is a hit iff its f32 t < inf, two
material words are compared as bits, a tap's colour is eligible iff the f32 colour and the f32 quotient c / a are finite, and "stage
A (B, C) has no tap" is a count of eligible taps (the rule's "weight sum is zero", exact because every weight is positive).  The
floor of a position is taken from the float64 position: the exact position ((2 px + 1) low_w - width) / (2 width) is either an integer,
which both precisions compute exactly, or at least 1 / (2 width) away from one, which float32 resolves for every width below 2^10 or
so -- the sizes this reference is used at.

What float64 does not restate is float32 overflow in the middle of a sum.  Before the stage weights were scaled (kUpscaleScaleA / B /
C) a finite tap of 3e38 at weight 1.2 was +Inf in the f32 rule and 3.6e38 / 1.2 here; with the scaling no f32 sum over finite taps
overflows and the two agree there as well."""
import numpy as np

from upscale_ref import SKY, STAGE_A, STAGE_B, STAGE_C, STAGE_NONE

F64 = np.float64
BILINEAR_FLOOR = 2.0 ** -26
EDGE_FLOOR = 0.25


def _positions(n_full, n_low):
    """(position in low pixel units clamped to [0, n_low - 1], its floor as int, the fraction) per output column (row), float64."""
    x = np.clip((np.arange(n_full, dtype=F64) + 0.5) * n_low / n_full - 0.5, 0.0, float(n_low - 1))
    x0 = np.floor(x)
    return x, x0.astype(np.int64), x - x0


def _sky(dirs):
    d = np.asarray(dirs, F64)
    u = d / np.sqrt((d * d).sum(-1, keepdims=True))
    a = 0.5 * (u[..., 1] + 1.0)
    return np.sqrt(np.stack([(1.0 - a) + a * 0.5, (1.0 - a) + a * 0.7, (1.0 - a) + a * 1.0], -1))


def upscale(low, g_low, g_full, dirs_full, tan_half_fov, sigma_n=128.0, sigma_z=1.0):
    """(out (h, w, 4) float64, stage (h, w) u8): the arguments of upscale_ref.upscale."""
    low32, gl32, gf32 = np.asarray(low, np.float32), np.asarray(g_low, np.float32), np.asarray(g_full, np.float32)
    lh, lw = low32.shape[:2]
    h, w = gf32.shape[:2]
    # ---- the f32 decisions
    with np.errstate(all="ignore"):
        colour_ok = np.isfinite(low32[..., :3]).all(-1)
        tap_ok = (gl32[..., 3] < np.inf) & colour_ok & np.isfinite(low32[..., :3] / gl32[..., 4:7]).all(-1)
    mat_l = np.ascontiguousarray(gl32[..., 7]).view(np.uint32).astype(np.int64)
    mat_p = np.ascontiguousarray(gf32[..., 7]).view(np.uint32).astype(np.int64)
    hit = gf32[..., 3] < np.inf
    # ---- float64 from here on; a tap outside the frame reads material -1 from the padding and is never eligible
    R = 2                                                     # stage B reaches x0 - 1 .. x0 + 2
    pad = lambda a, fill: np.pad(a, [(R, R), (R, R)] + [(0, 0)] * (a.ndim - 2), constant_values=fill)
    with np.errstate(all="ignore"):
        cd = np.where(tap_ok[..., None], low32[..., :3].astype(F64) / gl32[..., 4:7].astype(F64), 0.0)
    cd_p, c_p = pad(cd, 0.0), pad(np.where(colour_ok[..., None], low32[..., :3].astype(F64), 0.0), 0.0)
    ok_p, fin_p, mat_lp = pad(tap_ok, False), pad(colour_ok, False), pad(mat_l, -1)
    n_lp, t_lp = pad(gl32[..., 0:3].astype(F64), 0.0), pad(np.where(gl32[..., 3] < np.inf, gl32[..., 3], 0.0).astype(F64), 0.0)
    n = gf32[..., 0:3].astype(F64)
    t = np.where(hit, gf32[..., 3], 0.0).astype(F64)
    a = gf32[..., 4:7].astype(F64)
    d = np.asarray(dirs_full, F64)
    theta = 2.0 * float(tan_half_fov) / lh
    zs = t * theta / np.fmax(np.abs((n * d).sum(-1)), 0.1)
    zden = float(sigma_z) * zs + 1e-6
    xl, x0, fx = _positions(w, lw)
    yl, y0, fy = _positions(h, lh)
    X0, Y0 = np.broadcast_to(x0[None, :], (h, w)), np.broadcast_to(y0[:, None], (h, w))

    def gather(plane, qy, qx):
        return plane[qy + R, qx + R]

    def edge_tap(qy, qx):
        """(eligible, c', w_n w_z) of the low pixels (qy, qx), which may lie up to R outside the frame."""
        el = hit & gather(ok_p, qy, qx) & (gather(mat_lp, qy, qx) == mat_p)
        wn = np.fmax(0.0, (n * gather(n_lp, qy, qx)).sum(-1)) ** float(sigma_n)
        wz = np.exp(-np.abs(t - gather(t_lp, qy, qx)) / zden)
        return el, gather(cd_p, qy, qx), wn * wz

    sums = {s: [np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w), np.int64)] for s in (STAGE_A, STAGE_B, STAGE_C)}

    def add(s, el, wgt, col):
        wgt = np.where(el, wgt, 0.0)
        sums[s][0] += wgt
        sums[s][1] += wgt[..., None] * np.where(el[..., None], col, 0.0)
        sums[s][2] += el

    with np.errstate(all="ignore"):
        for j in (0, 1):
            for i in (0, 1):
                # the footprint's second tap on an axis is min(x0 + 1, low_w - 1)
                qx, qy = np.minimum(X0 + i, lw - 1), np.minimum(Y0 + j, lh - 1)
                b = ((fx if i else 1.0 - fx)[None, :] * (fy if j else 1.0 - fy)[:, None]) + BILINEAR_FLOOR
                el, col, e = edge_tap(qy, qx)
                add(STAGE_A, el, b * (e + EDGE_FLOOR), col)
                add(STAGE_C, gather(fin_p, qy, qx), b, gather(c_p, qy, qx))
        for j in range(-1, 3):
            for i in range(-1, 3):
                qx, qy = X0 + i, Y0 + j
                el, col, e = edge_tap(qy, qx)
                d2 = (qx - xl[None, :]) ** 2 + (qy - yl[:, None]) ** 2
                add(STAGE_B, el, (e + EDGE_FLOOR) / (1.0 + d2), col)
        out = np.zeros((h, w, 4), F64)
        out[..., 3] = 1.0
        stage = np.full((h, w), STAGE_NONE, np.uint8)
        left = hit.copy()
        for s, remodulate in ((STAGE_A, True), (STAGE_B, True), (STAGE_C, False)):
            sw, sc, count = sums[s]
            take = left & (count > 0)
            col = sc / sw[..., None]
            out[..., :3][take] = (col * a if remodulate else col)[take]
            stage[take] = s
            left &= ~take
        out[..., :3][~hit] = _sky(d)[~hit]
        stage[~hit] = SKY
    return out, stage


def upscale_frame(oracle, low, g_low, g_full, cam, sigma_n=128.0, sigma_z=1.0):
    """upscale() with the pixel-centre rays of `cam` at g_full's size."""
    import denoise_ref as dr
    h, w = g_full.shape[:2]
    _, dirs, tan = dr.pixel_center_rays(oracle, cam, w, h)
    return upscale(low, g_low, g_full, dirs, tan, sigma_n=sigma_n, sigma_z=sigma_z)


def compare(got, want):
    """(the largest |got - want| / max(1, |want|) over the channels where `want` is finite, whether every other channel has `want`'s
    class: NaN, +Inf or -Inf)."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    fin = np.isfinite(want)
    with np.errstate(invalid="ignore"):
        err = np.abs(got[fin] - want[fin]) / np.fmax(1.0, np.abs(want[fin]))
    err = np.where(np.isnan(err), np.inf, err)               # (a NaN or an Inf where `want` is finite is an infinite error)
    g, wt = got[~fin], want[~fin]
    same = np.array_equal(np.isnan(g), np.isnan(wt)) and np.array_equal(g[~np.isnan(wt)], wt[~np.isnan(wt)])
    return (float(err.max()) if err.size else 0.0), bool(same)
