"""An independent numpy float64 reference of the a-trous filter, written from the formulas of DESIGN.md section 10 (not from the kernel's
order of operations, and sharing nothing with tests/denoise_ref.py but how its inputs are loaded: guides, pixel-centre rays, tan(fov/2)).

Every plane is padded by the largest tap offset of its pass, so a tap is one slice of the padded array; a padded cell is "not a tap".

NaN rules (the ones the kernel means to follow): wherever the kernel calls max_f / min_f (fmaxf / fminf, IEEE
maxNum / minNum) this reference calls np.fmax / np.fmin, which return the other operand when one is NaN -- so max(0, NaN) is 0, not NaN.
The pass-through decision is a property of the f32 input: a pixel passes through when its centre ray misses (t = +inf) or when c.rgb or
the f32 quotient c.rgb / a is not finite; those pixels are never taps and come out as their input, bit for bit."""
import numpy as np

F64 = np.float64
H5 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0           # (1/16, 1/4, 3/8, 1/4, 1/16)
G3 = np.array([1.0, 2.0, 1.0]) / 4.0                      # the 3x3 Gaussian (1 2 1) x (1 2 1) / 16, renormalised over its taps
STRENGTH_SPP = 4


def strength(spp):
    """k: 1 up to STRENGTH_SPP samples per pixel, then sqrt(STRENGTH_SPP / spp)."""
    return 1.0 if spp <= STRENGTH_SPP else float(np.sqrt(STRENGTH_SPP / float(spp)))


def passes_through(frame, g):
    """(h, w) bool: sky, or a colour (or its f32 quotient by a) that is not finite."""
    f32 = np.asarray(frame, np.float32)
    with np.errstate(all="ignore"):
        cd = f32[..., :3] / np.asarray(g[..., 4:7], np.float32)
    return ~(g[..., 3] < np.inf) | ~np.isfinite(f32[..., :3]).all(-1) | ~np.isfinite(cd).all(-1)


def _pad(a, r, fill):
    return np.pad(a, [(r, r), (r, r)] + [(0, 0)] * (a.ndim - 2), constant_values=fill)


def _at(ap, r, dx, dy, h, w):
    """the tap (dx, dy) of every pixel, from a plane padded by r."""
    return ap[r + dy:r + dy + h, r + dx:r + dx + w]


def _lum(c):
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def denoise(frame, g, dirs, tan_half_fov, iterations=5, sigma_l=4.0, sigma_n=128.0, sigma_z=1.0, spp=1):
    """The denoised RGBA frame (h, w, 4) float64 of `frame` (h, w, 4) rendered at `spp` samples per pixel, with guides g (h, w, 8) and
    pixel-centre ray directions dirs (h, w, 3).  Pass-through pixels hold the input's f32 values."""
    h, w = frame.shape[:2]
    through = passes_through(frame, g)
    live = ~through
    c = np.asarray(frame, F64)
    n, t, a = np.asarray(g[..., 0:3], F64), np.asarray(g[..., 3], F64), np.asarray(g[..., 4:7], F64)
    k = strength(spp)
    sl = sigma_l * k
    with np.errstate(all="ignore"):
        cd = np.where(live[..., None], c[..., :3] / a, 0.0)
        t = np.where(live, t, 0.0)
        n = np.where(live[..., None], n, 0.0)
        theta = 2.0 * float(tan_half_fov) / h
        zs = t * theta / np.fmax(np.abs((n * np.asarray(dirs, F64)).sum(-1)), 0.1)

        def edge(r, dx, dy, dist, npad, tpad):
            """w_n w_z of the tap (dx, dy) at pixel distance dist."""
            nq, tq = _at(npad, r, dx, dy, h, w), _at(tpad, r, dx, dy, h, w)
            wn = np.fmax(0.0, (n * nq).sum(-1)) ** sigma_n
            wz = np.exp(-np.abs(t - tq) / (sigma_z * dist * zs + 1e-6))
            return wn * wz

        # the 7x7 variance of l(c'), taps weighted by w_n w_z
        r = 3
        lpad, vpad, npad, tpad = _pad(_lum(cd), r, 0.0), _pad(live, r, False), _pad(n, r, 0.0), _pad(t, r, 0.0)
        sw, s1, s2 = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w))
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                wq = np.where(_at(vpad, r, dx, dy, h, w), edge(r, dx, dy, np.hypot(dx, dy), npad, tpad), 0.0)
                lq = _at(lpad, r, dx, dy, h, w)
                sw, s1, s2 = sw + wq, s1 + wq * lq, s2 + wq * lq * lq
        var = np.fmax(0.0, s2 / sw - (s1 / sw) ** 2)

        cur = cd
        for i in range(iterations):
            step = 1 << i
            # g_p: the 3x3 Gaussian of var over the pixel's live neighbours
            vp, lvp = _pad(var, 1, 0.0), _pad(live, 1, False)
            gv, gw = np.zeros((h, w)), np.zeros((h, w))
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    kq = np.where(_at(lvp, 1, dx, dy, h, w), G3[dx + 1] * G3[dy + 1], 0.0)
                    gv, gw = gv + kq * _at(vp, 1, dx, dy, h, w), gw + kq
            lscale = sl * np.sqrt(np.fmax(0.0, gv / gw)) + 1e-6
            r = 2 * step
            cpad, varpad, vpad = _pad(cur, r, 0.0), _pad(var, r, 0.0), _pad(live, r, False)
            npad, tpad = _pad(n, r, 0.0), _pad(t, r, 0.0)
            lp = _lum(cur)
            sw, sc, sv = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    ox, oy = dx * step, dy * step
                    cq = _at(cpad, r, ox, oy, h, w)
                    wl = np.exp(-np.abs(lp - _lum(cq)) / lscale)
                    wq = H5[dx + 2] * H5[dy + 2] * edge(r, ox, oy, step * np.hypot(dx, dy), npad, tpad) * wl
                    wq = np.where(_at(vpad, r, ox, oy, h, w), wq, 0.0)
                    sw, sc, sv = sw + wq, sc + wq[..., None] * cq, sv + wq * wq * _at(varpad, r, ox, oy, h, w)
            cur = np.where(live[..., None], sc / sw[..., None], 0.0)
            var = np.where(live, sv / (sw * sw), 0.0)
        out = np.array(c)
        out[..., :3] = np.where(live[..., None], (cd + k * (cur - cd)) * a, c[..., :3])
    return out


def denoise_frame(oracle, frame, g, cam, rays=None, **settings):
    """denoise() of `frame` rendered with camera `cam`: its pixel-centre rays (or `rays` = (dirs, tan_half_fov)) and its sample count."""
    import denoise_ref as dr
    h, w = frame.shape[:2]
    if rays is None:
        _, dirs, tan = dr.pixel_center_rays(oracle, cam, w, h)
    else:
        dirs, tan = rays
    return denoise(frame, g, dirs, tan, spp=int(cam[0]["sample_count"]), **{**dr.DEFAULTS, **settings})


def inject(frame, g, seed=3):
    """A copy of `frame` with values the filter must survive written into hit pixels (shared with the GPU tests)."""
    f = np.asarray(frame, np.float32).copy()
    h, w = f.shape[:2]
    hit = np.argwhere(g[..., 3] < np.inf)
    rng = np.random.default_rng(seed)
    pick = hit[rng.permutation(len(hit))]
    k = max(1, len(pick) // 40)
    it = iter(range(0, len(pick), k))

    def take():
        i = next(it, None)
        return pick[i:i + k] if i is not None else pick[:0]

    for (y, x), v in zip(take(), (np.nan, np.inf, -np.inf) * len(pick)):
        f[y, x, (y + x) % 3] = v
    for y, x in take():                                                    # finite, but c / a is not (where a < 1)
        if g[y, x, 5] < 1:
            f[y, x, 1] = np.finfo(np.float32).max
    for y, x in take():
        f[y, x, :3] = -np.abs(f[y, x, :3]) - np.float32(0.25)
    for (y, x), v in zip(take(), (1e2, 1e4, 1e6) * len(pick)):
        f[y, x, :3] = np.float32(v)
    for y, x in take():
        f[y, x, 3] = np.float32(0.375)
    return f


def rel_err(got, want, mask=None):
    """|got - want| / max(1, |want|) per pixel (the max over the channels); `mask` (h, w): only those pixels, else all of them."""
    with np.errstate(invalid="ignore"):
        e = (np.abs(np.asarray(got, F64) - want) / np.fmax(1.0, np.abs(want))).max(-1)
    return e if mask is None else e[mask]
