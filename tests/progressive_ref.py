"""The record and the rule of progressive frames (bevyray_amd/csrc/brt_progressive.h) restated in numpy f32 -- every operation separately
rounded, in the header's order -- with what the tests of the feature share: the synthetic state planes and their non-vacuity condition,
the board of special records, the window of a pixel for the host twin, and the CPU model of the one-call form on the oracle."""
import numpy as np

import bevyray_amd as brt

F = np.float32
REC = brt.PROG_PIXEL_DTYPE
# ten frame sizes around the 16-pixel tile of the selecting kernel (every one holds the three crafted waves of synthetic_plane)
SIZES = ((16, 12), (17, 13), (16, 16), (17, 17), (31, 15), (32, 16), (33, 17), (47, 31), (48, 32), (49, 33))
SPECIAL = (np.nan, np.inf, -np.inf, 3e38, -3e38, 1e-42, -0.0, 0.0)


def luma(r, g, b):
    return (F(0.2126) * F(r) + F(0.7152) * F(g)) + F(0.0722) * F(b)


def accumulate(rec, rgb):
    """One more sample of colour rgb: a new 1-element REC array (rng and rays stay)."""
    out = np.array(rec, REC).reshape(1).copy()
    c = np.asarray(rgb, F)
    with np.errstate(all="ignore"):
        out["sum"][0] = out["sum"][0] + c
        l = luma(c[0], c[1], c[2])
        out["m1"][0] = out["m1"][0] + l
        out["m2"][0] = out["m2"][0] + l * l
    out["n"][0] = (int(out["n"][0]) + 1) & 0xFFFFFFFF
    return out


def noisy(state, threshold):
    """The own flag of every record of `state` (any shape)."""
    with np.errstate(all="ignore"):
        nf = state["n"].astype(F)
        m = state["m1"] / nf
        d = state["m2"] / nf - m * m
        v = np.where(d > 0, d, F(0))
        e = v / nf
        t = F(threshold) * np.where(m > F(0.01), m, F(0.01))
        return (e > t * t) & (state["n"] >= 2)


def classes(state, target, threshold, radius):
    """(H, W) u8 of PROG_SELECTED / 0 for the (H, W) state plane."""
    h, w = state.shape
    own = noisy(state, threshold)
    pad = np.zeros((h + 2, w + 2), bool)
    pad[1:-1, 1:-1] = own
    around = np.zeros((h, w), bool)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            around |= pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    return ((state["n"] < target) & around).astype(np.uint8) * brt.PROG_SELECTED


def window(state, x, y):
    """(records9, inside9) of pixel (x, y) for brt_host_progressive_class: dy outer, dx inner, clipped to the frame."""
    h, w = state.shape
    recs, inside = np.zeros(9, REC), np.zeros(9, np.uint32)
    for k in range(9):
        qx, qy = x + k % 3 - 1, y + k // 3 - 1
        if 0 <= qx < w and 0 <= qy < h:
            recs[k], inside[k] = state[qy, qx], 1
        else:
            recs[k]["m1"], recs[k]["m2"], recs[k]["n"] = 1.0, 1e6, 4      # a record that would be noisy, were it looked at
    return recs, inside


def value(state):
    """(H, W, 4) f32: the frame of a state plane."""
    out = np.zeros(state.shape + (4,), F)
    has = state["n"] > 0
    with np.errstate(all="ignore"):
        out[..., :3][has] = state["sum"][has] / state["n"][has].astype(F)[:, None]
    out[..., 3][has] = 1.0
    return out


def _record(rng, n, noisy_one, threshold):
    """A plausible record of n samples whose own flag is `noisy_one` at `threshold` (checked by the caller)."""
    r = np.zeros(1, REC)
    mean = F(rng.uniform(0.05, 1.5))
    rel = F(threshold) * F(np.sqrt(max(n, 1))) * F(rng.uniform(3.0, 6.0) if noisy_one else rng.uniform(0.0, 0.3))
    r["n"], r["m1"] = n, mean * F(n)
    r["m2"] = (mean * mean) * (F(1) + rel * rel) * F(n)
    r["sum"] = (mean * F(n) * rng.uniform(0.5, 1.5, 3)).astype(F)
    r["rng"], r["rays"] = rng.integers(0, 2 ** 32), rng.integers(n, 9 * n + 1)
    return r[0]


def synthetic_plane(w, h, seed, target=16, threshold=0.1):
    """An (h, w) state plane: random quiet and noisy records at counts below, at and above the target, and three crafted waves of the
    selecting kernel (a wave is rows 4k .. 4k + 3 of a 16-wide tile): rows 0-3 of the first tile all selected, rows 4-7 none, rows 8-11 one."""
    assert w >= 16 and h >= 12
    rng = np.random.default_rng(seed)
    counts = (2, target // 2, target - 1, target, target + 5)
    s = np.zeros((h, w), REC)
    for y in range(h):
        for x in range(w):
            s[y, x] = _record(rng, int(rng.choice(counts)), rng.random() < 0.08, threshold)
    for y in range(12):
        for x in range(16):
            if y < 4:
                s[y, x] = _record(rng, target // 2, True, threshold)
            else:
                s[y, x] = _record(rng, target, False, threshold)
    s[9, 5] = _record(rng, target - 1, True, threshold)
    # (the columns right of the first tile and the row below it would reach into the crafted waves at radius 1: keep them quiet)
    for y in range(min(13, h)):
        for x in range(min(17, w)):
            if (x == 16 or y == 12) and noisy(s[y:y + 1, x:x + 1], threshold).any():
                s[y, x] = _record(rng, int(s[y, x]["n"]), False, threshold)
    return s


def wave_counts(cls):
    """The selected lanes of every wave of the selecting kernel for the class map cls."""
    h, w = cls.shape
    out = []
    for ty in range(0, h, 16):
        for tx in range(0, w, 16):
            for wy in range(ty, min(ty + 16, h), 4):
                out.append(int((cls[wy:wy + 4, tx:tx + 16] != 0).sum()))
    return out


def non_vacuous(cls):
    """Selected and unselected pixels are present, and at least one wave has 0, 1 and 64 selected lanes."""
    wc = wave_counts(cls)
    return bool(cls.any() and not cls.all() and 0 in wc and 1 in wc and 64 in wc)


def special_board(target=16):
    """An (h, w) plane of special records: counts 0, 1, 2, T - 1, T; NaN, +-INF, 3e38, denormal and -0.0 in every float field; m2
    overflowing while m * m stays finite, and both overflowing; ordinary quiet and noisy neighbours between them."""
    rng = np.random.default_rng(99)
    recs = []
    for n in (0, 1, 2, target - 1, target):
        for noisy_one in (False, True):
            recs.append(_record(rng, n, noisy_one, 0.1))
        for field in ("sum", "m1", "m2"):
            for v in SPECIAL:
                r = _record(rng, n, False, 0.1)
                if field == "sum":
                    r["sum"][int(rng.integers(0, 3))] = v
                else:
                    r[field] = v
                recs.append(r)
        for m1, m2 in ((1e19 * max(n, 1), np.inf), (3e38, np.inf), (np.inf, np.inf), (1e19 * max(n, 1), 3.4e38), (2e19 * max(n, 1), 3.4e38)):
            r = _record(rng, n, False, 0.1)
            r["m1"], r["m2"] = m1, m2
            recs.append(r)
    w = 13
    h = (len(recs) + w - 1) // w
    while len(recs) < w * h:
        recs.append(_record(rng, int(rng.choice((2, target - 1, target))), rng.random() < 0.3, 0.1))
    order = rng.permutation(len(recs))
    return np.array(recs, REC)[order].reshape(h, w)


class CoverModel:
    """The cover scene at 96x54, 8 bounces on the oracle: the prefix frames F_1 .. F_max (cached), and the modelled per-sample luminances
    -- f32 luminance of the float64 differences k F_k - (k - 1) F_(k-1).  A MODEL of what the kernel accumulates (the f32 colours of the
    samples themselves), good for shares and for quality, not for bits."""
    W, H, BOUNCES = 96, 54, 8

    def __init__(self, oracle, max_spp=64, seed=0.5):
        self.oracle, self.max_spp, self.seed = oracle, max_spp, seed
        self.buffers = brt.generate_scene(brt.SCENE_COVER, 1)
        self._frames = {}
        self._luma = None

    def view(self, spp, seed=None):
        return brt.cover_camera(self.W, self.H, spp, self.BOUNCES, brt.Raytracing.Pure, self.seed if seed is None else seed)

    def frame(self, spp):
        if spp not in self._frames:
            f = self.oracle.render(self.buffers, *self.view(spp), self.W, self.H)[0]
            f.setflags(write=False)
            self._frames[spp] = f
        return self._frames[spp]

    def luma(self):
        if self._luma is None:
            out = np.zeros((self.max_spp, self.H, self.W), F)
            prev = np.zeros((self.H, self.W, 3), np.float64)
            for k in range(1, self.max_spp + 1):
                cur = self.frame(k)[..., :3].astype(np.float64) * k
                c = (cur - prev).astype(F)
                out[k - 1] = luma(c[..., 0], c[..., 1], c[..., 2])
                prev = cur
            self._luma = out
        return self._luma

    def counts(self, first, targets, threshold, radius):
        return model_counts(self.luma(), first, targets, threshold, radius)

    def progressive_frame(self, n):
        """The frame whose pixel p holds the oracle's n_p-sample value."""
        out = np.zeros((self.H, self.W, 4), F)
        for k in np.unique(n):
            out[n == k] = self.frame(int(k))[n == k]
        return out


def targets_of(first, max_spp):
    """The targets of the one-call form behind its whole-frame pass: doubling, the last one max_spp."""
    t, out = first, []
    while t < max_spp:
        t = max_spp if t > max_spp // 2 else 2 * t
        out.append(t)
    return out


def distribution_ok(n, first, max_spp):
    """The one-call test's condition: every count is one of the targets, and at least three distinct counts each hold >= 3 % of the pixels."""
    allowed = [first] + targets_of(first, max_spp)
    shares = {k: float((n == k).mean()) for k in allowed}
    return bool(np.isin(n, allowed).all() and sum(s >= 0.03 for s in shares.values()) >= 3), shares


def mse(a, b):
    return float(((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2).mean())


def model_counts(per_sample_luma, first, targets, threshold, radius):
    """The CPU model of the one-call form on modelled per-sample luminances (S, H, W) f32 (a MODEL: the samples' luminances are taken
    from prefix frames, not from the f32 colours the kernel adds): the sample count every pixel ends at."""
    s, h, w = per_sample_luma.shape
    n = np.full((h, w), first, np.uint32)

    def plane():
        st = np.zeros((h, w), REC)
        idx = np.arange(s)[:, None, None] < n[None]
        l = np.where(idx, per_sample_luma, F(0))
        st["m1"] = np.add.accumulate(l, axis=0, dtype=F)[-1]
        st["m2"] = np.add.accumulate(l * l, axis=0, dtype=F)[-1]
        st["n"] = n
        return st
    for t in targets:
        n = np.where(classes(plane(), t, threshold, radius) != 0, np.uint32(t), n)
    return n
