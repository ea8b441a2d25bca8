"""Synthetic base frames for the adaptive selection rule (brt_adaptive.h, brt_adaptive.hip; tests/test_adaptive_synthetic.py): frames the
tracer never renders -- non-finite, overflowing, negative and denormal values, frame edges on, before and after a 16-pixel tile edge, and
selection patterns that put no, one or all 64 lanes of a wave on the list.  Seeded numpy only; the guides {t, id} of the cover view come
from tests/denoise_ref.py (CPU) or brt_debug_denoise_guides (GPU)."""
import functools

import numpy as np

import adaptive_ref as ar
import bevyray_amd as brt
import denoise_ref as dr

F32 = np.float32
SIZES = [(15, 15), (16, 16), (17, 17), (31, 33), (32, 32), (48, 20), (1, 40), (40, 1), (2, 2), (257, 3)]       # width x height
FRAMES = ("noise", "flat", "lanes_one", "lanes_alternate", "lanes_all", "nonfinite", "huge", "signed")
PAIRS = ((0.4, 6), (brt.ADAPT_DEFAULT_THRESHOLD, 6), (0.4, 25), (0.1, 1))      # (threshold, min_taps) every frame is classed with
OWN_PAIR = {"lanes_one": (0.4, 6), "lanes_alternate": (0.4, 6), "lanes_all": (1e-30, 6)}      # the pair a lanes frame is made for
FLAT = (0.3, 0.5, 0.7, 1.0)
HUGE = (1e19, 1e20, 3e38)       # S2 overflows and m * m does not / both overflow / l * l overflows in one tap
EDGE_COORDS = (0, 1, 14, 15, 16, 17)
BOUNCES, BASE_SPP, FULL_SPP = 4, 2, 8


def size_id(size):
    return "%dx%d" % size


@functools.lru_cache(maxsize=None)
def view(w, h):
    """-> (Buffers, level, camera at FULL_SPP, window) of the cover view at w x h."""
    lvl, cam, win = brt.cover_camera(w, h, FULL_SPP, BOUNCES)
    return brt.generate_scene(brt.SCENE_COVER, 1), lvl, cam, win


@functools.lru_cache(maxsize=None)
def cpu_guides(oracle, w, h):
    b, _, cam, _ = view(w, h)
    g = dr.guides(oracle, b, cam, w, h)
    g.setflags(write=False)
    return g


def hit_of(guides):
    return np.asarray(guides[..., 3], F32) < np.inf


def ids_of(guides):
    h, w = guides.shape[:2]
    return np.ascontiguousarray(guides[..., 7]).view(np.uint32).reshape(h, w)


def wave_blocks(w, h):
    """(h, w) i64: the number of the wave of k_adaptive_select a pixel belongs to -- a 16 x 4 block of a 16 x 16 tile."""
    y, x = np.mgrid[0:h, 0:w]
    return (y // 4) * ((w + 15) // 16) + x // 16


def region_of(w, h):
    """(h, w) of 0 / 1 / 2: three bands along the longer axis (the `huge` frame's flat regions)."""
    y, x = np.mgrid[0:h, 0:w]
    return (3 * x) // w if w >= h else (3 * y) // h


def _special(n):
    return sorted({c for c in EDGE_COORDS + (n - 2, n - 1) if 0 <= c < n})


def _seed(kind, w, h):
    return [FRAMES.index(kind), w, h]


def frame(kind, w, h, guides):
    """-> (base (h, w, 4) f32, info).  info: "selected" (h, w) bool for the lanes frames (the pixels they are made to select under
    OWN_PAIR), "poisoned" (h, w) bool for `nonfinite`, "region" for `huge`."""
    rng = np.random.default_rng(_seed(kind, w, h))
    hit = hit_of(guides)
    info = {}
    if kind == "noise":
        base = rng.random((h, w, 4), dtype=F32)
    elif kind == "flat":
        base = np.empty((h, w, 4), F32)
        base[:] = FLAT
    elif kind in ("lanes_one", "lanes_alternate"):
        # a NaN frame (no class, no tap) with one finite hit pixel in a wave's 16 x 4 block: alone in its window, so n = 1 .. 5 < min_taps
        # and the pixel is SPARSE.  one: every wave that has a hit pixel; alternate: every second wave, the others select no lane
        base = np.full((h, w, 4), np.nan, F32)
        blocks, sel = wave_blocks(w, h), np.zeros((h, w), bool)
        for k in np.unique(blocks[hit]):
            if kind == "lanes_alternate" and k % 2 == 1:
                continue
            ys, xs = np.nonzero(hit & (blocks == k))
            j = int(rng.integers(0, ys.size))
            sel[ys[j], xs[j]] = True
        base[sel] = FLAT
        info["selected"] = sel
    elif kind == "lanes_all":
        # two luminances in a checker: every window of six or more taps has a positive variance, and at threshold 1e-30 thr * thr is 0
        y, x = np.mgrid[0:h, 0:w]
        base = np.empty((h, w, 4), F32)
        base[:] = FLAT
        base[(x + y) % 2 == 1, :3] *= F32(0.5)
        info["selected"] = hit.copy()
    elif kind == "nonfinite":
        base = rng.random((h, w, 4), dtype=F32)
        bad = rng.random((h, w)) < 0.05
        cols, rows = _special(w), _special(h)
        for i, x in enumerate(cols):
            bad[rows[i % len(rows)], x] = True
            bad[int(rng.integers(0, h)), x] = True
        for i, y in enumerate(rows):
            bad[y, cols[(i + 1) % len(cols)]] = True
            bad[y, int(rng.integers(0, w))] = True
        ys, xs = np.nonzero(bad)
        base[ys, xs, rng.integers(0, 3, ys.size)] = rng.choice(np.array([np.nan, np.inf, -np.inf], F32), ys.size)
        info["poisoned"] = bad
    elif kind == "huge":
        region = region_of(w, h)
        base = np.ones((h, w, 4), F32)
        for k, v in enumerate(HUGE):
            base[region == k, :3] = F32(v)
        info["region"] = region
    elif kind == "signed":
        base = -rng.random((h, w, 4), dtype=F32)                       # a negative mean: below the 0.01 floor
        what = np.arange(w * h).reshape(h, w) % 5                        # (also in a 2 x 2 frame: pixel 1 is -0.0, pixel 3 denormal)
        base[what == 1] = F32(-0.0)
        tiny = what == 3
        base[tiny] = ((rng.random((int(tiny.sum()), 4)) + 0.5) * 1e-40).astype(F32)      # denormals
        base[..., 3] = 1.0
    else:
        raise ValueError(kind)
    base.setflags(write=False)
    return base, info


def taps_of(base, guides, x, y):
    """The 25 taps of pixel (x, y) in the rule's order -> (inside (25,) bool, ids (25,) u32, colours (25, 3) f32)."""
    h, w = base.shape[:2]
    ids = ids_of(guides)
    inside, tid, cols = np.zeros(25, bool), np.zeros(25, np.uint32), np.zeros((25, 3), F32)
    k = 0
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            qx, qy = x + dx, y + dy
            if 0 <= qx < w and 0 <= qy < h:
                inside[k], tid[k], cols[k] = True, ids[qy, qx], base[qy, qx, :3]
            k += 1
    return inside, tid, cols


def host_masks(base, guides, pairs):
    """brt_host_adaptive_class pixel by pixel, once per (threshold, min_taps) of `pairs`: the compiled rule on the taps class_mask sees."""
    h, w = base.shape[:2]
    ids = ids_of(guides)
    out = [np.zeros((h, w), np.uint8) for _ in pairs]
    for y in range(h):
        for x in range(w):
            inside, tid, cols = taps_of(base, guides, x, y)
            for m, (thr, mt) in zip(out, pairs):
                m[y, x] = brt.adaptive_class(guides[y, x, 3], ids[y, x], base[y, x, :3], inside, tid, cols, thr, mt)
    return out


def tap_counts(base, guides):
    """(n (h, w): the taps the rule counts per pixel, pure (h, w) bool: every counted tap lies in the pixel's own `huge` region)."""
    h, w = base.shape[:2]
    ids, l, region = ids_of(guides), ar.luma(base), region_of(w, h)
    n, pure = np.zeros((h, w), np.int64), np.ones((h, w), bool)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            ok = ar._shift(np.ones((h, w), bool), dx, dy, False) & (ar._shift(ids, dx, dy, np.uint32(0)) == ids)
            ok &= np.isfinite(ar._shift(l, dx, dy, F32(np.nan)))
            n += ok
            pure &= ~ok | (ar._shift(region, dx, dy, -1) == region)
    return n, pure
