"""Synthetic low frames for the guide-buffer upsampling (brt_upscale.hip; tests/test_upscale_synthetic.py), after the manner of
tests/adaptive_synth.py: frames the tracer never renders, chosen so that the input-dependent branches of k_upscale run -- the finite3
rejections of tap() and of stage C, stage B's 4x4 gather at the frame border, stage C, the zero store.  Seeded numpy only.  Every
generator takes the low guides g_low (lh, lw, 8) (tests/denoise_ref.py on the CPU, brt_debug_denoise_guides on the GPU) and returns a
low frame (lh, lw, 4) f32 that starts from seeded uniform [0.25, 1) colour with alpha 1.

Non-vacuity: CONDITIONS names, per pattern, the least number of output pixels per stage that upscale_ref.upscale must report for the
frame to do its work; check_conditions asserts it.  The conditions are held at the four size pairs of PAIRS on the cover view
(tests/test_upscale_synthetic.py, CPU), and again wherever a GPU test relies on them."""
import numpy as np

import upscale_ref as ur

F32 = np.float32
PATTERNS = ("checker", "blocks2", "blocks6", "overflow", "all_nan", "signs_and_small", "alpha_junk")
PAIRS = [(64, 36, 32, 18), (65, 37, 17, 10), (17, 15, 5, 4), (40, 24, 39, 23)]      # (width, height, low_width, low_height)
NON_FINITE = (np.nan, np.inf, -np.inf)
OVERFLOW = 3.0e38               # finite; OVERFLOW / a is not, wherever a < 0.88
MIN_PIXELS = 8
STAGE_NAMES = {ur.SKY: "sky", ur.STAGE_A: "A", ur.STAGE_B: "B", ur.STAGE_C: "C", ur.STAGE_NONE: "none"}
# pattern -> {stage: the least number of output pixels}; "all_hit" names the stage every hit pixel must have
CONDITIONS = {
    "checker": {ur.STAGE_A: MIN_PIXELS, ur.STAGE_B: MIN_PIXELS, ur.STAGE_C: MIN_PIXELS},
    "blocks2": {ur.STAGE_A: MIN_PIXELS, ur.STAGE_B: MIN_PIXELS, ur.STAGE_C: MIN_PIXELS, ur.STAGE_NONE: MIN_PIXELS},
    "blocks6": {ur.STAGE_NONE: MIN_PIXELS},
    "overflow": {ur.STAGE_C: MIN_PIXELS},
    "all_nan": {"all_hit": ur.STAGE_NONE},
    "signs_and_small": {ur.STAGE_A: MIN_PIXELS},
    "alpha_junk": {ur.STAGE_A: MIN_PIXELS, ur.STAGE_B: MIN_PIXELS, ur.STAGE_C: MIN_PIXELS},
}
BLOCKS6_PAIRS = PAIRS[:2] + PAIRS[3:]       # a 5x4 low frame is one block of six: `blocks6` is held at the three larger pairs


def pair_id(pair):
    return "%dx%d_from_%dx%d" % tuple(pair)


def base_frame(g_low, seed=0):
    """Seeded uniform [0.25, 1) colour, alpha 1."""
    lh, lw = g_low.shape[:2]
    low = np.ones((lh, lw, 4), F32)
    low[..., :3] = np.random.default_rng([seed, lw, lh]).uniform(0.25, 1.0, (lh, lw, 3)).astype(F32)
    return low


def _poison(low, where):
    """One channel of every pixel of `where`, (x + y) % 3, is set to NaN, +Inf, -Inf in rotation (in raster order)."""
    ys, xs = np.nonzero(where)
    low[ys, xs, (xs + ys) % 3] = np.array(NON_FINITE, F32)[np.arange(ys.size) % 3]


def checker(g_low):
    """Every second low pixel, (x + y) % 2 == 0, has one non-finite channel: stage A loses taps but keeps some wherever two of its
    taps lie on the pixel's material; where the only taps on the material are poisoned ones, stages B and C follow.
    Condition: A, B and C each in at least 8 output pixels."""
    low = base_frame(g_low, 1)
    y, x = np.mgrid[0:low.shape[0], 0:low.shape[1]]
    _poison(low, (x + y) % 2 == 0)
    return low


def _blocks(g_low, k, seed):
    low = base_frame(g_low, seed)
    y, x = np.mgrid[0:low.shape[0], 0:low.shape[1]]
    _poison(low, (y // k + x // k) % 2 == 0)
    return low


def blocks2(g_low):
    """The low pixels of every second 2x2 block, (y // 2 + x // 2) % 2 == 0, have one non-finite channel: whole footprints go, stage B
    gathers from the ring around them (at the frame border: the part of the ring inside the frame), stage C finds a finite tap or none.
    Condition: A, B, C and none each in at least 8 output pixels."""
    return _blocks(g_low, 2, 2)


def blocks6(g_low):
    """The same with 6x6 blocks: whole 4x4 neighbourhoods are non-finite, so the (0, 0, 0, 1) store is reached.
    Condition: none in at least 8 output pixels (low frames of at least 6 pixels on an axis)."""
    return _blocks(g_low, 6, 3)


def overflow(g_low):
    """Every third low pixel, (x + y) % 3 == 0, is 3e38 on all channels: finite, but c / a is not wherever a < 0.88, so the pixel is no
    tap of stages A and B and is one of stage C, whose weights sum to 1 + 4 x 2^-26 at the most.  Where a is 1 (a refracting sphere)
    the pixel stays a tap of stage A.  Before the stage weights were scaled (kUpscaleScaleA / B / C) a weight above 1.134 took w c' past
    FLT_MAX there and the f32 rule stored +Inf; now every output of this frame is finite.
    Condition: C in at least 8 output pixels."""
    low = base_frame(g_low, 4)
    y, x = np.mgrid[0:low.shape[0], 0:low.shape[1]]
    low[(x + y) % 3 == 0, :3] = F32(OVERFLOW)
    return low


def all_nan(g_low):
    """Every colour channel is NaN.  Condition: every hit pixel is none."""
    low = base_frame(g_low, 5)
    low[..., :3] = np.nan
    return low


def signs_and_small(g_low):
    """By a seeded choice per pixel: the base colour, its negative, -0.0, f32 denormals, 1e-30, 1e30.  Everything is finite and so is
    every c / a (a >= sqrt(1e-3)): every tap stays eligible.  Condition: A in at least 8 output pixels, every kind present."""
    low = base_frame(g_low, 6)
    lh, lw = low.shape[:2]
    rng = np.random.default_rng([7, lw, lh])
    kind = rng.integers(0, 6, (lh, lw))
    kind.ravel()[:6] = np.arange(6)                 # (every kind, in a 5x4 frame too)
    low[kind == 1, :3] *= F32(-1.0)
    low[kind == 2, :3] = F32(-0.0)
    tiny = kind == 3
    low[tiny, :3] = ((rng.random((int(tiny.sum()), 3)) + 0.5) * 1e-40).astype(F32)
    low[kind == 4, :3] = F32(1e-30)
    low[kind == 5, :3] = F32(1e30)
    return low


def alpha_junk(g_low):
    """The `checker` frame with alpha NaN / +Inf / -1 by x % 3.  The rule never reads the low frame's alpha: the output is checker's,
    bit for bit.  Condition: checker's."""
    low = checker(g_low)
    x = np.arange(low.shape[1])
    low[..., 3] = np.array([np.nan, np.inf, -1.0], F32)[x % 3][None, :]
    return low


_GENERATORS = {"checker": checker, "blocks2": blocks2, "blocks6": blocks6, "overflow": overflow, "all_nan": all_nan,
               "signs_and_small": signs_and_small, "alpha_junk": alpha_junk}


def frame(pattern, g_low):
    low = _GENERATORS[pattern](g_low)
    low.setflags(write=False)
    return low


def stage_counts(stage):
    """[sky, A, B, C, none]"""
    return np.bincount(stage.ravel(), minlength=5)[:5].tolist()


def check_conditions(pattern, stage, where=""):
    """Asserts CONDITIONS[pattern] on the stage plane upscale_ref.upscale reports for the pattern's frame."""
    counts = stage_counts(stage)
    for key, need in CONDITIONS[pattern].items():
        if key == "all_hit":
            assert (stage[stage != ur.SKY] == need).all() and (stage != ur.SKY).any(), (pattern, where, counts)
        else:
            assert counts[key] >= need, (pattern, where, STAGE_NAMES[key], counts)
    return counts
