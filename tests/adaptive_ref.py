"""numpy f32 restatement of the adaptive-sampling rule (DESIGN.md "Adaptive sampling", brt_adaptive.h): the class of every pixel of a base
frame from the frame and its full-size guides, and the adaptive frame as "the base frame with the selected pixels replaced by the full
frame's".  Every operation is a separately rounded f32 one in the kernel's order, so with a base frame and guides that are bitwise the
kernel's the mask is the kernel's."""
import numpy as np

F32 = np.float32
SPARSE, NOISY = 1, 2            # BRT_ADAPT_SPARSE, BRT_ADAPT_NOISY
MEAN_FLOOR = F32(0.01)


def luma(rgb):
    """(0.2126 r + 0.7152 g) + 0.0722 b of (..., >= 3) f32, each operation rounded to f32."""
    c = np.asarray(rgb, F32)
    with np.errstate(all="ignore"):
        return (F32(0.2126) * c[..., 0] + F32(0.7152) * c[..., 1]) + F32(0.0722) * c[..., 2]


def _shift(a, dx, dy, fill):
    """a[y + dy, x + dx] for every (y, x); `fill` where that lies outside the frame."""
    h, w = a.shape
    out = np.full_like(a, fill)
    if abs(dx) >= w or abs(dy) >= h:
        return out
    ys, yd = slice(max(0, dy), h + min(0, dy)), slice(max(0, -dy), h + min(0, -dy))
    xs, xd = slice(max(0, dx), w + min(0, dx)), slice(max(0, -dx), w + min(0, -dx))
    out[yd, xd] = a[ys, xs]
    return out


def class_of_sums(n, s1, s2, threshold, min_taps):
    """The class from the tap count and the two f32 sums (arrays or scalars): SPARSE iff n < min_taps, else NOISY iff v > thr * thr."""
    n, s1, s2 = np.asarray(n), np.asarray(s1, F32), np.asarray(s2, F32)
    with np.errstate(all="ignore"):
        nf = n.astype(F32)
        m = s1 / nf
        d = s2 / nf - m * m
        v = np.where(d > 0, d, F32(0))
        thr = F32(threshold) * np.where(m > MEAN_FLOOR, m, MEAN_FLOOR)
        noisy = v > thr * thr
    return np.where(n < min_taps, SPARSE, np.where(noisy, NOISY, 0)).astype(np.uint8)


def class_from_taps(t_p, id_p, l_p, inside, ids, ls, threshold, min_taps):
    """One pixel from its 25 taps in (dy outer, dx inner) order: inside (25,) bool, ids (25,) u32, ls (25,) f32."""
    if not (F32(t_p) < np.inf) or not np.isfinite(F32(l_p)):
        return 0
    n, s1, s2 = 0, F32(0), F32(0)
    with np.errstate(all="ignore"):
        for k in range(25):
            l = F32(ls[k])
            if not inside[k] or int(ids[k]) != int(id_p) or not np.isfinite(l):
                continue
            n += 1
            s1 = F32(s1 + l)
            s2 = F32(s2 + F32(l * l))
    return int(class_of_sums(n, s1, s2, threshold, min_taps))


def class_mask(base, guides, threshold, min_taps):
    """(h, w) u8 classes.  base: (h, w, >= 3) f32 base frame; guides: (h, w, 8) f32 in brt_debug_denoise_guides' layout."""
    base = np.asarray(base, F32)
    h, w = base.shape[:2]
    l = luma(base)
    t = np.asarray(guides[..., 3], F32)
    ids = np.ascontiguousarray(guides[..., 7]).view(np.uint32).reshape(h, w)
    n = np.zeros((h, w), np.uint32)
    s1, s2 = np.zeros((h, w), F32), np.zeros((h, w), F32)
    inside = np.ones((h, w), bool)
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ok = _shift(inside, dx, dy, False)
                lq, iq = _shift(l, dx, dy, F32(0)), _shift(ids, dx, dy, np.uint32(0))
                ok = ok & (iq == ids) & np.isfinite(lq)
                lq = np.where(ok, lq, F32(0))
                n = n + ok
                s1 = np.where(ok, s1 + lq, s1).astype(F32)
                s2 = np.where(ok, s2 + lq * lq, s2).astype(F32)
    cls = class_of_sums(np.maximum(n, 1), s1, s2, threshold, min_taps)
    cls = np.where(n < min_taps, SPARSE, cls)
    classed = (t < np.inf) & np.isfinite(l)
    return np.where(classed, cls, 0).astype(np.uint8)


def adaptive(base, full, mask):
    """The adaptive frame: `base` (h, w, c) with the selected pixels (mask != 0) replaced by those of `full` (same shape and dtype)."""
    out = base.copy()
    sel = mask != 0
    out[sel] = full[sel]
    return out


def mse(frame, ref):
    d = frame[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64)
    return float(np.mean(d * d))
