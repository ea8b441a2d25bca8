"""numpy float32 restatement of the temporal accumulation (bevyray_amd/csrc/brt_temporal.hip) and of the denoiser
with per-pixel strength on top of it, in the kernels' order of operations.  Builds on denoise_ref (guides, pixel-centre rays, the
filter's helpers).  The oracle's raycast reports the material, not the sphere: sphere_ids() recovers the sphere by brute force."""
import numpy as np

import denoise_ref as dr

F32 = np.float32
U32 = np.uint32
NO_SPHERE = np.uint32(0xFFFFFFFF)
CONVERGED = F32(4.0)        # kTemporalConverged: from this n on, the variance comes from the moments and sigma_l is unscaled
NORMAL_MIN = F32(0.9)       # validation: n_p . n_q >= NORMAL_MIN
DEPTH_REL = F32(0.01)       # validation: |t_q - |X_prev - o_prev|| <= DEPTH_REL |X_prev - o_prev| + DEPTH_ZS zs_q
DEPTH_ZS = F32(2.0)
TIE = 1e-3                  # sphere_ids: a pixel whose two nearest surfaces are within TIE of each other is a tie


def luminance(c):
    return (F32(0.2126) * c[..., 0] + F32(0.7152) * c[..., 1]) + F32(0.0722) * c[..., 2]


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F32)


class Camera:
    """A frame's camera as the kernels see it: origin, basis, tan(fov / 2), aspect, and the pixel-centre ray directions."""

    def __init__(self, oracle, cam, w, h):
        c = cam[0]
        self.w, self.h = w, h
        self.o, self.dirs, self.tan = dr.pixel_center_rays(oracle, cam, w, h)
        self.aspect = F32(c["aspect"])
        self.D, self.U = c["direction"].astype(F32), c["up"].astype(F32)
        self.R = _cross(self.D, self.U)

    @classmethod
    def synthetic(cls, o, D, U, tan, w, h):
        """A camera from its numbers alone (tests without the oracle): aspect w / h."""
        self = cls.__new__(cls)
        self.w, self.h = w, h
        self.o, self.D, self.U = np.asarray(o, F32), np.asarray(D, F32), np.asarray(U, F32)
        self.R = _cross(self.D, self.U)
        self.tan, self.aspect = F32(tan), F32(F32(w) / F32(h))
        self.dirs = self.ray_dirs(np.arange(w, dtype=F32)[None, :], np.arange(h, dtype=F32)[:, None])
        return self

    def key(self):
        return [a.tobytes() for a in (self.o, self.D, self.U, self.R, np.array([self.aspect, self.tan], F32))]

    def inverse(self):
        """temporal_camera(): the rows (R x U, U x D, D x R) / det."""
        rows = [_cross(self.R, self.U), _cross(self.U, self.D), _cross(self.D, self.R)]
        det = (self.D[0] * rows[0][0] + self.D[1] * rows[0][1]) + self.D[2] * rows[0][2]
        return np.array([r / det for r in rows], F32)

    def ray_dirs(self, px, py):
        """camera_ray_dir_center at integer pixels px, py (broadcast)."""
        uvx = (px.astype(F32) + F32(0.5)) / F32(self.w)
        uvy = (py.astype(F32) + F32(0.5)) / F32(self.h)
        ndc_x, ndc_y = uvx * F32(2.0) - F32(1.0), F32(1.0) - uvy * F32(2.0)
        sx = (ndc_x * self.aspect) * self.tan
        sy = ndc_y * self.tan
        d = [(self.D[k] + sx * self.R[k]) + sy * self.U[k] for k in range(3)]
        d = np.stack(np.broadcast_arrays(*d), -1).astype(F32)
        ln = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])[..., None]
        return (d / ln).astype(F32)


def sphere_ids(g, cam, models):
    """(sid (h, w) u32, ties (h, w) bool): the caller's index of the sphere each hit pixel lies on -- among the spheres of the hit's
    material, the one with the smallest |‖X - c‖ - r| at X = o + t d -- and the pixels whose nearest two candidates are within TIE of
    each other (their id is not trusted)."""
    h, w = g.shape[:2]
    t = g[..., 3]
    hit = t < np.inf
    sid = np.full((h, w), NO_SPHERE, U32)
    ties = np.zeros((h, w), bool)
    c = models["position"].astype(np.float64)
    r = np.abs(models["radius"].astype(np.float64))
    mat = models["material_id"].astype(np.int64)
    idx = np.flatnonzero(hit.ravel())
    x = (cam.o[None, :] + t.ravel()[idx, None] * cam.dirs.reshape(-1, 3)[idx]).astype(np.float64)
    mid = g[..., 7].view(U32).ravel()[idx].astype(np.int64)
    for m in np.unique(mid):                         # (the candidates of a pixel are the spheres of its material: one group each)
        cand = np.flatnonzero(mat == m)
        rows = np.flatnonzero(mid == m)
        for k in range(0, len(rows), 4096):
            r_ = rows[k:k + 4096]
            e = np.abs(np.sqrt(((x[r_, None, :] - c[None, cand, :]) ** 2).sum(-1)) - r[None, cand])
            order = np.argsort(e, axis=1, kind="stable")[:, :2]
            best = np.take_along_axis(e, order, 1)
            sid.ravel()[idx[r_]] = cand[order[:, 0]]
            if len(cand) > 1:
                ties.ravel()[idx[r_]] = best[:, 1] - best[:, 0] < TIE
    return sid, ties


def spheres_of(models):
    """{centre, r^2} per sphere in the caller's order, as the encoder stores them."""
    s = np.zeros((len(models), 4), F32)
    s[:, :3] = models["position"]
    s[:, 3] = models["radius"].astype(F32) * models["radius"].astype(F32)
    return s


class History:
    """The context's temporal history: planes a {n, t}, b {h, n}, c {m1, m2, sid bits, mid bits} of the last temporal frame, its
    camera and spheres; `xy` is the reprojected position of that frame's pixels (NaN: rejected)."""

    def __init__(self, max_history=32):
        self.max_history = F32(max_history)
        self.valid = False

    def reset(self):
        self.valid = False


def accumulate(hist, frame, g, sid, cam, spheres, motion=True):
    """One temporal frame: reprojects, validates and accumulates `frame` (h, w, 4) with guides g (h, w, 8), caller sphere ids `sid` and
    `spheres` ({c, r^2}, caller order) into `hist`.  Returns (h_plane (h, w, 4) {h.rgb, n}, moments (h, w, 2), through (h, w) bool).
    motion=False: the object-motion term is left out (a test shows it matters)."""
    H, W = frame.shape[:2]
    with np.errstate(all="ignore"):
        n_p, t, a = g[..., 0:3], g[..., 3], g[..., 4:7]
        mid = g[..., 7].view(U32)
        cd = frame[..., :3] / a
        fin = np.isfinite(frame[..., :3]).all(-1) & np.isfinite(cd).all(-1)
        through = ~(t < np.inf) | ~fin
        had = hist.valid and hist.shape == (H, W)
        xp = np.full((H, W), np.nan, F32)
        yp = np.full((H, W), np.nan, F32)
        dist = np.zeros((H, W), F32)
        if had:
            pc = hist.cam
            x = (cam.o + t[..., None] * cam.dirs).astype(F32)
            moved = np.zeros((H, W), bool)
            use_motion = motion and len(hist.spheres) == len(spheres)
            if use_motion:
                s = np.where(through, U32(0), sid).astype(np.int64)
                sn, so = spheres[s], hist.spheres[s]
                moved = (sn.view(U32) != so.view(U32)).any(-1) & ~through
                sc = np.sqrt(so[..., 3]) / np.sqrt(sn[..., 3])
                xm = (so[..., :3] + (x - sn[..., :3]) * sc[..., None]).astype(F32)
                x = np.where(moved[..., None], xm, x)
            v = (x - pc.o).astype(F32)
            dist = np.sqrt(_dot(v, v))
            inv = pc.inverse()
            z, aa, bb = (_dot(inv[k], v) for k in range(3))
            ndc_x = ((aa / z) / pc.tan) / pc.aspect
            ndc_y = (bb / z) / pc.tan
            xr = ((ndc_x + F32(1.0)) * F32(0.5)) * F32(W) - F32(0.5)
            yr = ((F32(1.0) - ndc_y) * F32(0.5)) * F32(H) - F32(0.5)
            xr = np.where(z > 0, xr, np.nan).astype(F32)
            yr = np.where(z > 0, yr, np.nan).astype(F32)
            ident = (pc.key() == cam.key()) & ~moved
            gy, gx = np.mgrid[0:H, 0:W]
            xp = np.where(ident, gx.astype(F32), xr).astype(F32)
            yp = np.where(ident, gy.astype(F32), yr).astype(F32)
            ok = (xp > -1) & (xp < W) & (yp > -1) & (yp < H) & ~through
            xp = np.where(ok, xp, np.nan).astype(F32)
            yp = np.where(ok, yp, np.nan).astype(F32)
        sw = np.zeros((H, W), F32)
        sr, sg, sb, sn_, s1, s2 = (np.zeros((H, W), F32) for _ in range(6))
        if had:
            live = xp == xp
            x0, y0 = np.floor(np.where(live, xp, 0)), np.floor(np.where(live, yp, 0))
            fx, fy = (np.where(live, xp, 0) - x0).astype(F32), (np.where(live, yp, 0) - y0).astype(F32)
            theta = (F32(2.0) * pc.tan) / F32(H)
            A, B, Cm = hist.a, hist.b, hist.c
            for j in range(4):
                dx, dy = j & 1, j >> 1
                w = ((fx if dx else F32(1.0) - fx) * (fy if dy else F32(1.0) - fy)).astype(F32)
                qx, qy = x0.astype(np.int64) + dx, y0.astype(np.int64) + dy
                ok = live & (w > 0) & (qx >= 0) & (qy >= 0) & (qx < W) & (qy < H)
                qxc, qyc = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                aq, bq, cq = A[qyc, qxc], B[qyc, qxc], Cm[qyc, qxc]
                ok &= (cq[..., 2].view(U32) == sid) & (cq[..., 3].view(U32) == mid)
                ok &= _dot(n_p, aq[..., :3]) >= NORMAL_MIN
                dq = pc.ray_dirs(qxc, qyc)
                zs = (aq[..., 3] * theta) / np.fmax(np.abs(_dot(aq[..., :3], dq)), F32(0.1))
                ok &= np.abs(aq[..., 3] - dist) <= DEPTH_REL * dist + DEPTH_ZS * zs
                ok &= bq[..., 3] > 0
                wz = np.where(ok, w, F32(0))
                add = lambda s_, v_: np.where(ok, s_ + wz * v_, s_).astype(F32)   # noqa: E731
                sw = np.where(ok, sw + wz, sw).astype(F32)
                sr, sg, sb = add(sr, bq[..., 0]), add(sg, bq[..., 1]), add(sb, bq[..., 2])
                sn_, s1, s2 = add(sn_, bq[..., 3]), add(s1, cq[..., 0]), add(s2, cq[..., 1])
        l = luminance(cd)
        hp = np.concatenate([cd, np.ones((H, W, 1), F32)], -1).astype(F32)
        m1, m2 = l.astype(F32), (l * l).astype(F32)
        valid = (sw > 0) & ~through
        n = np.fmin(sn_ / sw + F32(1.0), hist.max_history).astype(F32)
        blend = valid & (n > 1)
        alpha = F32(1.0) / n
        for k, s_ in enumerate((sr, sg, sb)):
            hh = s_ / sw
            hp[..., k] = np.where(blend, hh + (cd[..., k] - hh) * alpha, hp[..., k])
        hp[..., 3] = np.where(blend, n, F32(1.0))
        h1, h2 = s1 / sw, s2 / sw
        m1 = np.where(blend, h1 + (l - h1) * alpha, m1).astype(F32)
        m2 = np.where(blend, h2 + (l * l - h2) * alpha, m2).astype(F32)
        xp = np.where(valid, xp, np.nan).astype(F32)
        yp = np.where(valid, yp, np.nan).astype(F32)
    # the next history
    b = np.where(through[..., None], F32(0), hp).astype(F32)
    c = np.zeros((H, W, 4), F32)
    c[..., 0], c[..., 1] = np.where(through, 0, m1), np.where(through, 0, m2)
    c[..., 2] = sid.view(F32)
    c[..., 3] = mid.view(F32)
    hist.a = np.concatenate([n_p, t[..., None]], -1).astype(F32)
    hist.b, hist.c = b, c
    hist.xy = np.stack([xp, yp], -1)
    hist.cam, hist.spheres, hist.shape, hist.valid = cam, spheres.copy(), (H, W), True
    return hp, np.stack([m1, m2], -1), through


def state(hist):
    """brt_debug_temporal_state's layout: (h, w, 8) h.rgb, n, m1, m2, x', y'."""
    return np.concatenate([hist.b, hist.c[..., :2], hist.xy], -1).astype(F32)


def accumulated_frame(frame, g, hp, through):
    """FLAG_TEMPORAL alone: h a, the input itself where n = 1 or the pixel passes through."""
    out = frame.astype(F32).copy()
    keep = through | (hp[..., 3] == 1)
    rgb = (hp[..., :3] * g[..., 4:7]).astype(F32)
    out[..., :3] = np.where(keep[..., None], frame[..., :3], rgb)
    return out


def denoise(frame, g, dirs, tan_half_fov, hp, moments, through, iterations=5, sigma_l=4.0, sigma_n=128.0, sigma_z=1.0, spp=1):
    """FLAG_TEMPORAL | FLAG_DENOISE: denoise_ref.denoise on h instead of c', with the per-pixel strength k = min(1, sqrt(4 / (spp n)))
    (sigma_l scaled by k below CONVERGED, unscaled from it on) and, from CONVERGED on, var = max(0, m2 - m1^2) / n."""
    h, w = frame.shape[:2]
    n = hp[..., 3]
    with np.errstate(all="ignore"):
        k = np.fmin(F32(1.0), np.sqrt(F32(dr.STRENGTH_SPP) / (F32(spp) * n))).astype(F32)
        sl = np.where(n < CONVERGED, F32(sigma_l) * k, F32(sigma_l)).astype(F32)
        sigma_n, sigma_z = F32(sigma_n), F32(sigma_z)
        nrm, t, a = g[..., 0:3], g[..., 3], g[..., 4:7]
        theta = (F32(2.0) * F32(tan_half_fov)) / F32(h)
        zscale = np.where(through, F32(0), (t * theta) / np.fmax(np.abs(dr._dot(nrm, dirs)), F32(0.1))).astype(F32)
        cv = np.concatenate([hp[..., :3], np.zeros((h, w, 1), F32)], -1).astype(F32)
        cv[through] = np.concatenate([frame[..., :3], -np.ones((h, w, 1), F32)], -1)[through]
        c0 = cv[..., :3].copy()
        g0 = np.concatenate([nrm, t[..., None]], -1)
        fill_cv = np.array([0, 0, 0, -1], F32)

        def edge(dx, dy, step, g0q):
            nd = np.fmax(F32(0), dr._dot(nrm, g0q[..., :3]))
            wn = np.power(nd, sigma_n).astype(F32)
            dist = F32(step) * np.sqrt(F32(dx * dx + dy * dy))
            wz = np.exp(-np.abs(t - g0q[..., 3]) / ((sigma_z * dist) * zscale + F32(1e-6))).astype(F32)
            return wn, wz

        sw = np.zeros((h, w), F32)
        s_l = np.zeros((h, w), F32)
        sl2 = np.zeros((h, w), F32)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                cq, g0q = dr._taps(cv, g0, dx, dy)
                wn, wz = edge(dx, dy, 1, g0q)
                wgt = np.where(~(cq[..., 3] < 0), wn * wz, F32(0)).astype(F32)
                lq = dr._lum(cq)
                sw = sw + wgt
                s_l = s_l + wgt * lq
                sl2 = sl2 + wgt * (lq * lq)
        mean = s_l / sw
        var7 = np.fmax(F32(0), sl2 / sw - mean * mean)
        var_m = np.fmax(F32(0), moments[..., 1] - moments[..., 0] * moments[..., 0]) / n
        cv[..., 3] = np.where(through, F32(-1), np.where(n >= CONVERGED, var_m, var7))

        for i in range(iterations):
            step = 1 << i
            gv = np.zeros((h, w), F32)
            gw = np.zeros((h, w), F32)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    vq = dr._shift(cv, dx, dy, fill_cv)[..., 3]
                    kk = F32((0.5 if dx == 0 else 0.25) * (0.5 if dy == 0 else 0.25))
                    ok = ~(vq < 0)                  # (the kernel skips var < 0 only: a NaN variance is a tap)
                    gv = gv + np.where(ok, kk * vq, F32(0))
                    gw = gw + np.where(ok, kk, F32(0))
            lscale = sl * np.sqrt(np.fmax(F32(0), gv / gw)) + F32(1e-6)
            lp = dr._lum(cv)
            sw = np.zeros((h, w), F32)
            sc = np.zeros((h, w, 3), F32)
            sv = np.zeros((h, w), F32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    cq, g0q = dr._taps(cv, g0, dx * step, dy * step)
                    wn, wz = edge(dx, dy, step, g0q)
                    wl = np.exp(-np.abs(lp - dr._lum(cq)) / lscale).astype(F32)
                    wgt = np.where(~(cq[..., 3] < 0), (((dr.H5[dx + 2] * dr.H5[dy + 2]) * wn) * wz) * wl, F32(0)).astype(F32)
                    sw = sw + wgt
                    sc = sc + wgt[..., None] * cq[..., :3]
                    sv = sv + (wgt * wgt) * cq[..., 3]
            new = np.concatenate([sc / sw[..., None], (sv / (sw * sw))[..., None]], -1).astype(F32)
            cv = np.where(through[..., None], cv, new)
        blended = (c0 + k[..., None] * (cv[..., :3] - c0)).astype(F32)
    out = np.empty_like(frame, dtype=F32)
    out[..., :3] = np.where(through[..., None], cv[..., :3], blended * a)
    out[..., 3] = frame[..., 3]
    return out


def frame_step(hist, frame, g, sid, cam, spheres, spp, denoise_on, motion=True, **settings):
    """One FLAG_TEMPORAL (denoise_on=False) or FLAG_TEMPORAL | FLAG_DENOISE frame: the output frame."""
    hp, mom, through = accumulate(hist, frame, g, sid, cam, spheres, motion=motion)
    if not denoise_on:
        return accumulated_frame(frame, g, hp, through)
    return denoise(frame, g, cam.dirs, cam.tan, hp, mom, through, spp=spp, **{**dr.DEFAULTS, **settings})
