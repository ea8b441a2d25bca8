"""Reference side of tests/test_lightmap.py: the rule of lightmaps (DESIGN.md "Lightmaps", bevyray_amd/csrc/brt_lightmap.h) restated in
numpy, in f32 (every operation separately rounded, in the header's order) and in float64.

Directions (float64, rounded to f32 at the end), N in [1, 65536], k = 0 .. N-1:
    u = (k + 0.5) / N;  r = sqrt(u);  phi = 2 pi frac(k (sqrt(5)-1)/2);  l_k = (r cos phi, r sin phi, sqrt(1 - u))
`directions64` is that formula; the tests that compare bitwise take the table from the library's export (brt.lightmap_directions), so
that no libm difference reaches them.

Point {position, seed | normal, offset}.  EMPTY: the normal's words are all +-0.0 (looked at first).  INVALID: len2 is 0 or not finite,
a position word is not finite, offset is not finite or < 0.
    len2 = (nx nx + ny ny) + nz nz;  len = sqrt(len2);  n = normal / len
    s = copysign(1, n.z);  a = -1 / (s + n.z);  b = (n.x n.y) a
    t = (1 + (s (n.x n.x)) a,  s b,  (-s) n.x);  bt = (b,  s + (n.y n.y) a,  -n.y)
    o = position + offset * n;  d_k = (l.x * t + l.y * bt) + l.z * n
Entry k: {o, seed + k * 0x9E3779B9 (mod 2^32) | d_k, user = k}; an EMPTY or INVALID point: {position's words, that seed | 0x7fc00000 x 3,
k}.  Lists are point-major: entry k of point p is record p * N + k.

Resolve: L = rgb * rgb.  Lane l of 64 sums its entries k = l, l + 64, ... in order from +0.0; then for off = 32 .. 1: acc[l] = acc[l] +
acc[l + off]; rgb = acc[0] / f32(N), a = 1.  hits: the entries with the HIT bit.  status: entry 0's INVALID / OUT_OF_REACH bits, or EMPTY
alone for an EMPTY point; a point with a status has rgb = 0, a = 0, hits = 0.

Dilate: a texel with a > 0 is copied; any other sums the rgb of its neighbours with a > 0 (dy = -1, 0, 1 outer, dx = -1, 0, 1 inner, the
centre skipped; wrap_u: x modulo width, else outside is skipped) from +0.0 in that order; count > 0: rgb = sum / f32(count), a = 0.5."""
import numpy as np

import bevyray_amd as brt

F32 = np.float32
SEED_STEP = 0x9E3779B9
NAN_WORD = 0x7FC00000
HIT = brt.QUERY_STATUS_HIT
INVALID = brt.QUERY_STATUS_INVALID
REFUSED = brt.QUERY_STATUS_INVALID | brt.QUERY_STATUS_OUT_OF_REACH
EMPTY = brt.LIGHTMAP_STATUS_EMPTY
SKY_A, SKY_B = np.array([0.75, 0.85, 1.0]), np.array([-0.25, -0.15, 0.0])      # raytrace.wgsl background_gradient, linear: A + B d_y


def directions64(n):
    """The direction formula in numpy float64 -> (n, 3) float64 (not rounded)."""
    k = np.arange(n, dtype=np.float64)
    u = (k + 0.5) / float(n)
    r = np.sqrt(u)
    t = k * 0.6180339887498949
    phi = 2.0 * np.pi * (t - np.floor(t))
    return np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - u)], axis=1)


def sphere_points64(centre, radius, width, height):
    """(position, normal) of the latitude-longitude chart of a sphere in float64 -> two (height, width, 3) arrays."""
    theta = np.pi * ((np.arange(height, dtype=np.float64) + 0.5) / height)[:, None]
    phi = 2.0 * np.pi * ((np.arange(width, dtype=np.float64) + 0.5) / width)[None, :]
    n = np.stack([np.sin(theta) * np.cos(phi), np.cos(theta) * np.ones_like(phi), np.sin(theta) * np.sin(phi)], axis=2)
    return np.asarray(centre, np.float64) + float(radius) * n, n


def seeds(seed, count):
    return ((np.uint64(seed) + np.arange(count, dtype=np.uint64) * np.uint64(SEED_STEP)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def point_status(points):
    """0, EMPTY or INVALID per point, by the f32 rule."""
    p = np.ascontiguousarray(points, brt.LIGHTMAP_POINT_DTYPE).reshape(-1)
    nrm = p["normal"].astype(F32)
    with np.errstate(all="ignore"):
        len2 = ((nrm[:, 0] * nrm[:, 0]).astype(F32) + (nrm[:, 1] * nrm[:, 1]).astype(F32)).astype(F32) + (nrm[:, 2] * nrm[:, 2]).astype(F32)
    empty = ((nrm.view(np.uint32) & np.uint32(0x7FFFFFFF)) == 0).all(axis=1)
    off = p["offset"]
    bad = ~(len2 > 0) | ~np.isfinite(len2) | ~np.isfinite(p["position"]).all(axis=1) | ~(off >= 0) | ~np.isfinite(off)
    return np.where(empty, EMPTY, np.where(bad, INVALID, 0)).astype(np.uint32)


def frame(points, dtype=F32):
    """-> (o, n, t, bt), each (P, 3) of `dtype`: the f32 rule step by step, or the same formulas in float64 on the points' f32 words."""
    p = np.ascontiguousarray(points, brt.LIGHTMAP_POINT_DTYPE).reshape(-1)
    pos, nrm, off = p["position"].astype(dtype), p["normal"].astype(dtype), p["offset"].astype(dtype)
    one = dtype(1.0)
    with np.errstate(all="ignore"):
        len2 = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
        n = nrm / np.sqrt(len2)[:, None]
        s = np.copysign(one, n[:, 2])
        a = -one / (s + n[:, 2])
        b = (n[:, 0] * n[:, 1]) * a
        t = np.stack([one + (s * (n[:, 0] * n[:, 0])) * a, s * b, (-s) * n[:, 0]], axis=1)
        bt = np.stack([b, s + (n[:, 1] * n[:, 1]) * a, -n[:, 1]], axis=1)
        o = pos + off[:, None] * n
    assert o.dtype == dtype and t.dtype == dtype and bt.dtype == dtype and n.dtype == dtype
    return o, n, t, bt


def directions_of(points, dirs, dtype=F32):
    """d_k of every point -> (P, N, 3) of `dtype` (status not looked at)."""
    _, n, t, bt = frame(points, dtype)
    l = np.ascontiguousarray(dirs, F32).reshape(-1, 3).astype(dtype)
    with np.errstate(all="ignore"):
        d = (l[None, :, 0:1] * t[:, None, :] + l[None, :, 1:2] * bt[:, None, :]) + l[None, :, 2:3] * n[:, None, :]
    assert d.dtype == dtype
    return d


def make_rays(points, dirs):
    """The point-major list of RADIANCE_RAY_DTYPE entries of `points` for the f32 table `dirs`."""
    p = np.ascontiguousarray(points, brt.LIGHTMAP_POINT_DTYPE).reshape(-1)
    dirs = np.ascontiguousarray(dirs, F32).reshape(-1, 3)
    np_, n = len(p), len(dirs)
    status = point_status(p)
    o = frame(p)[0]
    d = directions_of(p, dirs)
    words = np.zeros((np_, n, 8), np.uint32)
    words[:, :, 0:3] = np.where(status[:, None] != 0, p["position"].view(np.uint32), o.view(np.uint32))[:, None, :]
    k = np.arange(n, dtype=np.uint64)
    words[:, :, 3] = ((p["seed"].astype(np.uint64)[:, None] + k[None, :] * np.uint64(SEED_STEP)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    words[:, :, 4:7] = np.where(status[:, None, None] != 0, np.uint32(NAN_WORD), d.view(np.uint32))
    words[:, :, 7] = k.astype(np.uint32)[None, :]
    return words.reshape(np_ * n, 8).view(brt.RADIANCE_RAY_DTYPE).reshape(np_ * n)


def _wave_sum(terms):
    """terms (P, N, A) f32 -> (P, A): the lane-strided accumulation and the six-step tree."""
    p, n, a = terms.shape
    with np.errstate(all="ignore"):
        acc = np.zeros((p, 64, a), F32)
        for i in range(-(-n // 64)):
            chunk = terms[:, 64 * i: 64 * i + 64, :]
            w = chunk.shape[1]
            acc[:, :w, :] = acc[:, :w, :] + chunk
        off = 32
        while off >= 1:
            acc[:, :off, :] = acc[:, :off, :] + acc[:, off: 2 * off, :]
            off //= 2
    return acc[:, 0, :]


def resolve(results, points, n_dirs):
    """results: (P * N,) RADIANCE_DTYPE, point-major; points: their (P,) points -> ((P, 4) f32 texels, (P,) LIGHTMAP_INFO_DTYPE)."""
    res = np.ascontiguousarray(results, brt.RADIANCE_DTYPE).reshape(-1, n_dirs)
    p = len(res)
    with np.errstate(all="ignore"):
        rgb = res["rgb"].astype(F32)
        sums = _wave_sum((rgb * rgb).astype(F32))
        texels = np.concatenate([(sums / F32(n_dirs)).astype(F32), np.ones((p, 1), F32)], axis=1)
    info = np.zeros(p, brt.LIGHTMAP_INFO_DTYPE)
    info["hits"] = ((res["status"] & HIT) != 0).sum(axis=1)
    info["status"] = np.where(point_status(points) == EMPTY, EMPTY, res["status"][:, 0] & REFUSED)
    off = info["status"] != 0
    texels[off] = 0
    info["hits"][off] = 0
    return texels, info


def resolve64(rgb):
    """The mean of the linear colours (P, N, 3) in float64, plain sums."""
    return (np.asarray(rgb, F32).astype(np.float64) ** 2).mean(axis=1)


def dilate(image, passes, wrap_u, dtype=F32):
    """`passes` passes over an (H, W, 4) image -> (H, W, 4) of `dtype`."""
    cur = np.ascontiguousarray(image, F32).astype(dtype)
    h, w = cur.shape[:2]
    for _ in range(passes):
        covered = cur[..., 3] > 0
        total = np.zeros((h, w, 3), dtype)
        count = np.zeros((h, w), np.uint32)
        with np.errstate(all="ignore"):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dx == 0 and dy == 0:
                        continue
                    ys = np.arange(h) + dy
                    xs = np.arange(w) + dx
                    y_ok = (ys >= 0) & (ys < h)
                    x_ok = np.ones(w, bool) if wrap_u else (xs >= 0) & (xs < w)
                    ys, xs = np.clip(ys, 0, h - 1), xs % w
                    nb = cur[ys][:, xs]
                    ok = y_ok[:, None] & x_ok[None, :] & covered[ys][:, xs]
                    total = np.where(ok[..., None], total + nb[..., :3], total)
                    count += ok
            filled = np.concatenate([total / np.maximum(count, 1).astype(dtype)[..., None], np.full((h, w, 1), 0.5, dtype)], axis=2)
        cur = np.where((~covered & (count > 0))[..., None], filled, cur).astype(dtype)
    return cur


def sky_mean64(normal, dirs):
    """The mean over the table of the linear sky A + B d_y for a unit normal, float64 -> (3,); and its closed form A + (2/3) B n_y."""
    p = np.zeros(1, brt.LIGHTMAP_POINT_DTYPE)
    p["normal"] = normal
    d = directions_of(p, dirs, np.float64)[0]
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    return (SKY_A + SKY_B * d[:, 1:2]).mean(axis=0), SKY_A + (2.0 / 3.0) * SKY_B * float(p["normal"][0][1])


def assert_texels_equal(got, want, what=""):
    """Bitwise, but a NaN for a NaN whatever its sign and payload (the host's and the device's default NaNs differ)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaNs at other places"
    bits = np.uint16 if got.dtype == np.float16 else np.uint32
    same = got.view(bits) == want.view(bits)
    assert (same | gn).all(), f"{what}: {np.count_nonzero(~(same | gn))} values differ, first at {np.argwhere(~(same | gn))[0]}"
